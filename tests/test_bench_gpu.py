"""GPU: a plain `bench.py` run measures the headline only; `--full` adds the extra legs to the same line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("fp32", "ref_cached", "contract_224", "train", "roofline", "roofline_other", "cpu_baseline")


def _bench(args):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--img", "224", "--batch", "4", "--steps", "3", "--warmup", "1"] + args,
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_bench_plain_run_has_no_extra_legs():
    res, err = _bench([])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["dtype"] == "bf16" and res["ms_per_step"] > 0
    assert abs(res["value"] - 4 * 3 / (res["ms_per_step"] * 3e-3)) < 1e-6 * res["value"]
    assert not set(EXTRA) & set(res), sorted(res)
    assert "leg done" not in err


@pytest.mark.gpu
def test_bench_full_adds_the_extra_legs():
    res, err = _bench(["--full", "--no-cpu-baseline", "--no-extra", "--no-roofline"])
    assert res["fp32"]["value"] > 0 and res["fp32"]["steps"] == 3
    assert not {"ref_cached", "contract_224", "train", "roofline", "roofline_other", "cpu_baseline"} & set(res), sorted(res)
    assert "fp32 leg done" in err
