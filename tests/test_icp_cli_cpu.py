"""CPU: `--icp [ITERS]` and the `model.fine_point_matching.icp_iters=K` override of `python -m unopose_amd.cli`, as `--print-plan` shows them
(no GPU is touched), and the config defaults."""
import json

import pytest

BASE = dict(model=dict(cfg=dict(coarse_npoint=196, fine_point_matching=dict(nblock=3))),
            dataloader=dict(test=dict(dataset=dict(eval_dataset_name="ycbv", detetion_path="d.json", cfg=dict(img_size=224, data_dir="/data/bop")))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"),
            bop_eval=dict(split="test"))


def _plan(tmp_path, capsys, *extra, cfg=BASE):
    from unopose_amd import cli

    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(cfg))
    assert cli.main(["--config-file", str(cfgf), "--print-plan", *extra]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_print_plan_shows_the_refinement(tmp_path, capsys):
    plain = _plan(tmp_path, capsys)
    assert "icp_iters" not in plain and "icp_inlier_thres" not in plain
    for extra, want in ((["--icp"], (10, 0.1)), (["--icp", "5"], (5, 0.1)), (["model.fine_point_matching.icp_iters=7"], (7, 0.1)),
                        (["model.cfg.fine_point_matching.icp_iters=7"], (7, 0.1)),
                        (["--icp", "4", "model.fine_point_matching.icp_inlier_thres=0.05"], (4, 0.05)),
                        (["--icp", "misc.exp_name=_x"], (10, 0.1)),
                        (["--icp", "3", "--pipeline", "--ref-cache", "--eval"], (3, 0.1))):
        plan = _plan(tmp_path, capsys, *extra)
        assert (plan["icp_iters"], plan["icp_inlier_thres"]) == want, extra
        rest = {k: v for k, v in plan.items() if not k.startswith(("icp_", "eval"))}
        assert rest == {k: v for k, v in plain.items() if not k.startswith("eval")} or "misc.exp_name=_x" in extra
    assert "icp_iters" not in _plan(tmp_path, capsys, "--icp", "0")
    flat = dict(BASE, model=dict(coarse_npoint=196))  # a config whose `model` is the model cfg itself
    assert _plan(tmp_path, capsys, "--icp", "2", cfg=flat)["icp_iters"] == 2


def test_icp_rejects_what_is_no_count(tmp_path, capsys):
    from unopose_amd import cli

    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(BASE))
    with pytest.raises(SystemExit):
        cli.main(["--config-file", str(cfgf), "--print-plan", "--icp", "many"])
    assert "--icp" in capsys.readouterr().err


def test_config_defaults():
    from unopose_amd.model import default_model_cfg

    f = default_model_cfg()["fine_point_matching"]
    assert f["icp_iters"] == 0 and f["icp_inlier_thres"] == 0.1
    assert default_model_cfg(fine_point_matching=dict(icp_iters=5)).fine_point_matching.icp_iters == 5
