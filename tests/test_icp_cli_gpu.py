"""GPU: `python -m unopose_amd.cli --icp 5` on the synthetic BOP folder (the builders of tests/test_cli_gpu.py): the CSV differs from the plain
run's in the score, R, t and time columns only, and its R and t are those of a model built with `icp_iters = 5` driven directly."""
import json

import numpy as np
import pytest
import torch

import bop_synth

pytestmark = pytest.mark.gpu


@torch.no_grad()
def test_cli_icp_changes_only_the_pose_columns(tmp_path):
    from unopose_amd import cli
    from unopose_amd import provider as P
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.runner import inference_and_save
    from unopose_amd.synthetic import trained_like_

    root = str(tmp_path / "bop")
    dcfg, det_path = bop_synth.build(root)
    mcfg = default_model_cfg(fine_npoint=256, feature_extraction=dict(img_size=dcfg["img_size"]))
    torch.manual_seed(3)
    model = trained_like_(UNOPose(mcfg))
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": model.state_dict(), "iteration": 7}, ckpt)
    cfg = dict(model=dict(cfg=dict(mcfg)), dataloader=dict(test=dict(dataset=dict(cfg=dcfg, eval_dataset_name="ycbv", detetion_path=det_path))),
               test=dict(amp=dict(enabled=False), instance_batch_size=2), misc=dict(output_dir=str(tmp_path / "out"), load_from=""), bop_eval=dict(split="test"))
    cfgf = tmp_path / "cfg.json"
    cfgf.write_text(json.dumps(cfg))

    def run(tag, *extra):
        np.random.seed(11)
        torch.manual_seed(5)  # the coarse stage draws inside forward
        assert cli.main(["--config-file", str(cfgf), *extra, f"misc.load_from={ckpt}", f"misc.exp_name=_{tag}"]) == 0
        path = tmp_path / "out" / "inference_model_final" / "ycbv" / f"result_{tag}_ycbv-test.csv"
        return [line.strip().split(",") for line in path.read_text().splitlines()]

    plain = run("plain")
    icp = run("icp", "--icp", "5")
    over = run("over", "model.fine_point_matching.icp_iters=5")  # the override beside model.cfg reaches the model too
    assert len(plain) == len(icp) == len(over) >= 3
    # runner.csv_line: scene_id,im_id,obj_id,score,R,t,time
    assert all(len(r) == 7 for r in plain + icp)
    for a, b in zip(plain, icp):
        assert a[:3] == b[:3]
    assert any(a[4:6] != b[4:6] for a, b in zip(plain, icp))
    strip = lambda rows: [r[:-1] for r in rows]  # noqa: E731  (last field = wall-clock time)
    assert strip(icp) == strip(over)

    mcfg5 = default_model_cfg(fine_npoint=256, feature_extraction=dict(img_size=dcfg["img_size"]), fine_point_matching=dict(icp_iters=5))
    model5 = UNOPose(mcfg5)
    model5.load_state_dict(model.state_dict(), strict=True)
    ds = P.BOPTestsetOneRef(dcfg, "ycbv", det_path)
    np.random.seed(11)
    images = [P.collate_image(ds[i]) for i in range(len(ds))]
    torch.manual_seed(5)
    want = inference_and_save(model5.cuda().eval(), images, str(tmp_path / "direct.csv"), instance_batch_size=2, device="cuda")
    assert strip([line.strip().split(",") for line in want]) == strip(icp)
