"""CPU: the device-preparation option is off by default and visible in the CLI's plan; nothing here touches a GPU
(the device path itself is tests/test_device_prep_gpu.py's)."""
import json
import os
import subprocess
import sys

import numpy as np

import bop_synth
from unopose_amd import provider as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_print_plan_reports_device_prep_and_default_provider_stays_on_the_host(tmp_path):
    cfg = dict(model=dict(cfg={}), dataloader=dict(test=dict(dataset=dict(eval_dataset_name="ycbv", detetion_path="dets.json"))),
               test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="out", load_from="ckpt.pth"), bop_eval=dict(split="test"))
    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(cfg))
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    plans = []
    for flags in ([], ["--device-prep"]):
        r = subprocess.run([sys.executable, "-m", "unopose_amd.cli", "--config-file", str(cfgf), "--print-plan", *flags],
                           capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        plans.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert plans[0]["device_prep"] is False and plans[1]["device_prep"] is True
    assert {k: v for k, v in plans[0].items() if k != "device_prep"} == {k: v for k, v in plans[1].items() if k != "device_prep"}

    dcfg, det_path = bop_synth.build(str(tmp_path / "bop"))
    ds = P.BOPTestsetOneRef(dcfg, "ycbv", det_path)
    assert ds.device is None
    np.random.seed(1)
    item = ds[0]
    assert all(not v.is_cuda for v in item.values() if hasattr(v, "is_cuda"))
    assert item["pts"].shape == (2, dcfg["n_sample_observed_point"], 3)
