"""GPU: the gated training step (train.train_step_gated on optim.FusedAdam's fused route) and the run (fit.fit) on the model and batch of
tests/test_train_gpu.py: make_train_batch() defaults, tamed weights, frozen backbone."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from train_case import make_train_batch

pytestmark = pytest.mark.gpu


def _model():
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    m = UNOPose(default_model_cfg(fine_npoint=512))
    m.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    return freeze_backbone(m.cuda())


def _optimizer(model, lr=2e-4):
    """train.build_optimizer's configuration (Adam betas (0.5, 0.999), eps 1e-6, flat-and-anneal schedule) on FusedAdam."""
    from unopose_amd.optim import FusedAdam
    from unopose_amd.train import flat_and_anneal_factor

    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=lr, betas=(0.5, 0.999), eps=1e-6, weight_decay=0.0)
    return opt, torch.optim.lr_scheduler.LambdaLR(opt, lambda it: flat_and_anneal_factor(it, 100, warmup_iters=0))


def _batch():
    return {k: v.cuda() for k, v in make_train_batch()[0].items()}


def _same_tree(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return a == b


def test_gated_steps_reduce_the_loss_fp32_and_bf16():
    from unopose_amd.train import train_step_gated

    batch = _batch()
    for amp in (None, torch.bfloat16):
        torch.manual_seed(0)
        np.random.seed(0)
        model = _model()
        opt, sched = _optimizer(model)
        w0 = model.fine_point_matching.out_proj.weight.detach().clone()
        infos = [train_step_gated(model, batch, opt, sched, amp_dtype=amp) for _ in range(6)]
        assert opt.launches == 3  # the fused route: three launches for every trainable tensor of the model
        losses = [float(i["loss"]) for i in infos]
        assert all(np.isfinite(losses)) and min(losses[3:]) < losses[0], (amp, losses)
        assert not torch.equal(model.fine_point_matching.out_proj.weight, w0)
        assert all(np.isfinite(float(i["total_grad_norm"])) and float(i["total_grad_norm"]) > 0 for i in infos) and sched.last_epoch == 6


def test_nonfinite_label_raises_and_leaves_every_state_untouched():
    """A NaN in a label does not make the LOSS non-finite on this model (the labels enter it through threshold comparisons only: measured
    19.9 -> 31.4 with translation_label[1, 2] = NaN, finite for every placement tried in either label); it shows in the `*_dis` monitors,
    which is why the gate's flag covers every scalar of process_loss."""
    from unopose_amd.train import train_step_gated

    torch.manual_seed(0)
    np.random.seed(0)
    model = _model()
    opt, sched = _optimizer(model)
    batch = _batch()
    for _ in range(2):
        train_step_gated(model, batch, opt, sched, clip_max_norm=35.0)
    sd_model, sd_opt, epoch = copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()), sched.last_epoch
    lr = opt.param_groups[0]["lr"]
    bad = dict(batch, translation_label=batch["translation_label"].clone())
    bad["translation_label"][1, 2] = float("nan")
    with pytest.raises(FloatingPointError):
        train_step_gated(model, bad, opt, sched, clip_max_norm=35.0)
    assert opt.launches == 3
    assert _same_tree(dict(model.state_dict()), dict(sd_model))  # parameters AND buffers (BatchNorm's running statistics are put back)
    assert _same_tree(opt.state_dict(), sd_opt) and sched.last_epoch == epoch == 2 and opt.param_groups[0]["lr"] == lr
    info = train_step_gated(model, batch, opt, sched, clip_max_norm=35.0)  # and the run can go on from there
    assert np.isfinite(float(info["loss"])) and sched.last_epoch == 3


def test_fit_writes_checkpoints_metrics_and_a_loadable_final_model(tmp_path):
    from unopose_amd import cli
    from unopose_amd.fit import fit
    from unopose_amd.model import UNOPose, default_model_cfg

    torch.manual_seed(0)
    np.random.seed(0)
    model = _model()
    opt, sched = _optimizer(model)
    batch = _batch()
    loader = [batch, {k: v.clone() for k, v in batch.items()}, batch, batch]  # 4 resident batches
    records = fit(model, None, loader, opt, sched, str(tmp_path), 4, period=2, log_period=1, clip_max_norm=35.0, device="cuda", log=lambda line: None)
    assert sorted(os.listdir(tmp_path)) == ["last_checkpoint", "metrics.json", "model_0000001.pth", "model_0000003.pth", "model_final.pth"]
    assert open(tmp_path / "last_checkpoint").read() == "model_final.pth"
    lines = [json.loads(line) for line in open(tmp_path / "metrics.json")]
    assert len(lines) == 4 and lines == records and [r["iteration"] for r in lines] == [0, 1, 2, 3]
    for r in lines:
        losses = [k for k in r if "_loss" in k and k != "total_loss"]
        assert len(losses) == 18 and abs(sum(r[k] for k in losses) - r["total_loss"]) < 1e-9 and np.isfinite(r["total_loss"])
        assert {"lr", "total_grad_norm", "time", "data_time"} <= set(r) and r["total_grad_norm"] > 0 and r["time"] > 0
    fresh = UNOPose(default_model_cfg(fine_npoint=512))
    cli.load_checkpoint(fresh, str(tmp_path / "model_final.pth"))  # strict
    assert _same_tree({k: v.cpu() for k, v in model.state_dict().items()}, dict(fresh.state_dict()))
    ck = torch.load(tmp_path / "model_final.pth", map_location="cpu")
    assert set(ck) >= {"model", "optimizer", "scheduler", "iteration", "rng"} and ck["iteration"] == 3
    assert all(float(st["step"]) == 4 for st in ck["optimizer"]["state"].values())
