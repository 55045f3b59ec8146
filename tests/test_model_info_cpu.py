"""CPU: `models_info.json` on the host -- `model_info.extent_host` against the toolkit's own `calc_model_info.py` / `misc.calc_pts_diameter`
values (tests/golden/model_info.npz) to the last bit, the pruning step, the files `write_models_info` writes, `--check`, the scorer's
`models_info="compute"` and the plan the CLI prints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import model_info_case as C
from unopose_amd import bop_eval, model_info

ROOT = C.ROOT


@pytest.mark.parametrize("prune", [True, False])
def test_extent_host_equals_the_toolkit_bit_for_bit(prune):
    for name, (pts, exp) in C.golden().items():
        lo, size, diameter = model_info.extent_host(pts, prune=prune)
        assert lo.dtype == size.dtype == np.float64 and isinstance(diameter, float)
        assert (lo == exp[:3]).all() and (size == exp[3:6]).all() and diameter == exp[6], (name, prune, diameter, exp[6])
    assert C.bits(model_info.extent_host(C.golden()["duplicates"][0], prune=prune)[2]) == 0  # +0.0


def test_the_block_size_does_not_change_a_bit():
    for name in ("lattice", "random", "far"):
        pts, exp = C.golden()[name]
        for block in (1, 7, 1000, 1 << 30):
            assert model_info.extent_host(pts, prune=False, block=block)[2] == exp[6], (name, block)
    with pytest.raises(ValueError, match="model_info"):
        model_info.extent_host(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="model_info"):
        model_info.extent_host(np.array([[0.0, np.nan, 1.0]]))


def test_pruning_happens_and_never_drops_the_farthest_pair():
    share = {name: float(model_info.prune_keep(pts).mean()) for name, (pts, _) in C.golden().items()}
    print(share)
    assert share["box"] <= 0.10 and share["clusters"] <= 0.10  # the rule alone, no tuning: a few points near the corners / the far ends
    assert share["duplicates"] == 1.0 and share["one"] == 1.0 and share["two"] == 1.0
    for name, (pts, exp) in C.golden().items():  # the shell keeps whatever it keeps: the value is the toolkit's all the same
        keep = model_info.prune_keep(pts)
        assert keep.dtype == bool and keep.shape == (len(pts),)
        assert np.sqrt(model_info.max_d2_host(pts[keep])) == exp[6], name


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("models") / "models_eval")
    return path, C.write_model_folder(path)


def test_write_models_info_writes_the_host_values_and_keeps_annotations(folder):
    path, pts = folder
    out = model_info.write_models_info(path, device=None)
    stored = C.load_info(path)
    assert sorted(stored) == sorted(str(o) for o in pts) and {int(k): v for k, v in stored.items()} == out
    for obj_id, p in pts.items():
        assert np.array_equal(bop_eval.read_ply(os.path.join(path, f"obj_{obj_id:06d}.ply"))["pts"], p)  # binary and ASCII read back alike
        lo, size, diameter = model_info.extent_host(p)
        e = stored[str(obj_id)]
        assert sorted(e) == sorted(model_info.INFO_KEYS)
        assert [e["min_x"], e["min_y"], e["min_z"]] == lo.tolist() and [e["size_x"], e["size_y"], e["size_z"]] == size.tolist() and e["diameter"] == diameter
    assert stored["12"]["diameter"] == float(np.sqrt(((pts[12][0] - pts[12][1]) ** 2).sum()))
    with pytest.raises(FileExistsError, match="models_info.json"):
        model_info.write_models_info(path, device=None)
    sym = [[-1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]]
    stored["4"].update(symmetries_discrete=sym, diameter=1.0, note="not carried over")
    stored["7"]["symmetries_continuous"] = [dict(axis=[0, 0, 1], offset=[0, 0, 0])]
    json.dump(stored, open(os.path.join(path, "models_info.json"), "w"))
    again = model_info.write_models_info(path, device=None, force=True)
    kept = C.load_info(path)
    assert kept["4"]["symmetries_discrete"] == sym and kept["7"]["symmetries_continuous"] == [dict(axis=[0, 0, 1], offset=[0, 0, 0])]
    assert "note" not in kept["4"] and kept["4"]["diameter"] == out[4]["diameter"] and "symmetries_discrete" not in kept["1"]
    assert {o: {k: e[k] for k in model_info.INFO_KEYS} for o, e in again.items()} == out
    assert len(bop_eval.symmetry_transformations(kept["4"])) == 2


def test_check_reports_a_changed_diameter_and_fails_only_for_a_missing_object(folder, capsys):
    path, pts = folder
    model_info.write_models_info(path, device=None, force=True)
    before = open(os.path.join(path, "models_info.json")).read()
    argv = ["--data-dir", os.path.dirname(os.path.dirname(path)), "--dataset", os.path.basename(os.path.dirname(path)), "--models", "models_eval", "--host", "--check"]
    assert model_info.main(argv) == 0
    assert "DIFFERENT" not in capsys.readouterr().out
    stored = json.loads(before)
    right = stored["7"]["diameter"]
    stored["7"]["diameter"] = right * 1.25
    json.dump(stored, open(os.path.join(path, "models_info.json"), "w"))
    assert model_info.main(argv) == 0  # a difference is reported, not an error
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(pts)
    line = next(ln for ln in lines if ln.startswith(f"obj {7:6d} "))
    assert repr(right * 1.25) in line and repr(right) in line and "2.500e-01" in line and "DIFFERENT" in line
    assert sum("DIFFERENT" in ln for ln in lines) == 1
    del stored["12"]
    json.dump(stored, open(os.path.join(path, "models_info.json"), "w"))
    assert model_info.main(argv) != 0
    assert "missing" in capsys.readouterr().out
    assert json.load(open(os.path.join(path, "models_info.json"))) == stored  # --check writes nothing
    with pytest.raises(FileExistsError):
        model_info.main(argv[:-1])  # without --force the file stays
    open(os.path.join(path, "models_info.json"), "w").write(before)


def test_the_module_has_a_command_line():
    r = subprocess.run([sys.executable, "-m", "unopose_amd.model_info", "--help"], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0 and all(flag in r.stdout for flag in ("--data-dir", "--dataset", "--models", "--host", "--force", "--check"))


SCORE = dict(device_scoring=False, error_types="mssd,mspd,add")


def test_score_csv_computes_the_diameters_of_a_dataset_without_the_file(tmp_path):
    csv, models_eval = C.write_score_dataset(str(tmp_path), symmetric=False)
    model_info.write_models_info(models_eval, device=None, force=True)
    plain = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", **SCORE)
    from_file = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="file", **SCORE)
    assert "models_info" not in plain and from_file["models_info"] == "file" and {k: v for k, v in from_file.items() if k != "models_info"} == plain
    os.remove(os.path.join(models_eval, "models_info.json"))
    with pytest.raises(FileNotFoundError):
        bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="file", **SCORE)
    computed = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="compute", **SCORE)
    assert computed["models_info"] == "compute" and json.load(open(os.path.join(os.path.dirname(csv), "scores_bop19.json")))["models_info"] == "compute"
    assert sorted(k for k in set(computed) | set(from_file) if computed.get(k) != from_file.get(k)) == ["models_info"]
    assert computed["recalls_mssd"] == from_file["recalls_mssd"] and computed["errors"]["add"]["recalls"] == from_file["errors"]["add"]["recalls"]
    assert 0.0 < computed["AR_MSSD"] < 1.0  # a graded problem: the diameters matter
    with pytest.raises(ValueError, match="models_info"):
        bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="maybe", **SCORE)
    with pytest.raises(ValueError, match="models_info"):
        bop_eval.load_dataset(str(tmp_path), "synth", "test", models_info="maybe")


def test_compute_ignores_the_stored_diameter_and_keeps_the_stored_symmetries(tmp_path):
    csv, models_eval = C.write_score_dataset(str(tmp_path), symmetric=True)
    model_info.write_models_info(models_eval, device=None, force=True)
    right = bop_eval.load_dataset(str(tmp_path), "synth", "test")["models"]
    stored = C.load_info(models_eval)
    assert "symmetries_discrete" in stored["2"]
    for e in stored.values():
        e["diameter"] *= 3.0
    json.dump(stored, open(os.path.join(models_eval, "models_info.json"), "w"))
    wrong = bop_eval.load_dataset(str(tmp_path), "synth", "test")["models"]
    computed = bop_eval.load_dataset(str(tmp_path), "synth", "test", models_info="compute")["models"]
    for o in right:
        assert computed[o]["diameter"] == right[o]["diameter"] == wrong[o]["diameter"] / 3.0
        assert len(computed[o]["symmetries"]) == len(right[o]["symmetries"]) == (2 if o == 2 else 1)
    os.remove(os.path.join(models_eval, "models_info.json"))
    alone = bop_eval.load_dataset(str(tmp_path), "synth", "test", models_info="compute")["models"]
    assert all(alone[o]["diameter"] == right[o]["diameter"] and len(alone[o]["symmetries"]) == 1 for o in right)


BASE = dict(model=dict(cfg=dict(coarse_npoint=196)),
            dataloader=dict(test=dict(dataset=dict(eval_dataset_name="tless", detetion_path="d.json", cfg=dict(img_size=224, data_dir="/data/bop")))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"),
            bop_eval=dict(split="test"))


def _plan(tmp_path, capsys, *extra):
    """`cli.main(--print-plan)` in this process: it touches no GPU and imports no torch."""
    from unopose_amd import cli

    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(BASE))
    assert cli.main(["--config-file", str(cfgf), "--print-plan", *extra]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_print_plan_names_models_info_only_when_set(tmp_path, capsys):
    plain = _plan(tmp_path, capsys, "--eval")
    assert "eval_models_info" not in plain
    for mode in ("compute", "file"):
        plan = _plan(tmp_path, capsys, "--eval", f"bop_eval.models_info={mode}")
        assert plan["eval_models_info"] == mode and {k: v for k, v in plan.items() if k != "eval_models_info"} == plain
    assert "eval_models_info" not in _plan(tmp_path, capsys, "bop_eval.models_info=compute")  # without --eval nothing is scored
    with pytest.raises(ValueError, match="bop_eval.models_info"):
        _plan(tmp_path, capsys, "--eval", "bop_eval.models_info=maybe")
