"""CPU: the training run (unopose_amd/fit.py) and the gated step's torch route (optim.FusedAdam on CPU tensors, train.train_step_gated) on
a toy model with UNOPose's training contract; the loader on the synthetic MegaPose tree (tests/megapose_synth.py)."""
import copy
import gc
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import megapose_synth
from unopose_amd import fit as F
from unopose_amd import train
from unopose_amd.optim import FusedAdam


class _Toy(torch.nn.Module):
    """Stand-in with UNOPose's training contract (as in test_train_cpu.py): returns an end_points dict holding per-sample `*_loss*` entries.
    `spare` is a parameter no forward reads: its gradient stays None."""

    def __init__(self, spare=True):
        super().__init__()
        self.lin = torch.nn.Linear(6, 3)
        if spare:
            self.spare = torch.nn.Parameter(torch.ones(2))

    def forward(self, ep):
        y = self.lin(ep["x"])
        ep["fine_atten_loss0"] = ((y - ep["y"]) ** 2).mean(1)
        ep["coarse_hard_acc"] = torch.ones(y.shape[0])
        return ep


def _batches(n=4, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(4, 6, generator=g), "y": torch.randn(4, 3, generator=g)} for _ in range(n)]


def _setup(seed=0):
    torch.manual_seed(seed)
    model = _Toy()
    opt = FusedAdam(model.parameters(), lr=1e-2, betas=(0.5, 0.999), eps=1e-6)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: train.flat_and_anneal_factor(it, 100, warmup_iters=2))
    return model, opt, sched


def _run(out, max_iter, resume=False, seed=0, **kw):
    model, opt, sched = _setup(seed)
    kw = dict(dict(period=3, log_period=1, clip_max_norm=35.0, log=lambda line: None), **kw)
    recs = F.fit(model, None, _batches(), opt, sched, str(out), max_iter, resume=resume, **kw)
    return model, opt, sched, recs


def _same_tree(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return a == b


def _no_clock(rec):
    return {k: v for k, v in rec.items() if k not in ("time", "data_time")}


def test_resumed_run_equals_the_uninterrupted_one(tmp_path):
    m6, o6, s6, r6 = _run(tmp_path / "straight", 6)
    _run(tmp_path / "split", 3)
    assert open(tmp_path / "split" / "last_checkpoint").read() == "model_final.pth"
    m33, o33, s33, r33 = _run(tmp_path / "split", 6, resume=True, seed=123)  # a fresh process' state: other weights, empty optimiser
    assert [r["iteration"] for r in r6] == list(range(6)) and [r["iteration"] for r in r33] == [3, 4, 5]
    assert _same_tree(m6.state_dict(), m33.state_dict()) and _same_tree(o6.state_dict(), o33.state_dict())
    assert s6.last_epoch == s33.last_epoch == 6
    assert [_no_clock(r) for r in r6[3:]] == [_no_clock(r) for r in r33]
    lines = [json.loads(line) for line in open(tmp_path / "split" / "metrics.json")]
    assert [r["iteration"] for r in lines] == list(range(6)) and [_no_clock(r) for r in lines] == [_no_clock(r) for r in r6]
    for r in lines:
        assert set(r) == {"iteration", "total_loss", "fine_atten_loss0", "lr", "total_grad_norm", "time", "data_time"}
        assert r["total_loss"] == r["fine_atten_loss0"] and r["total_grad_norm"] > 0 and r["time"] >= r["data_time"] >= 0
    assert r6[-1]["total_loss"] < r6[0]["total_loss"]


def test_retention_keeps_the_newest_periodic_files_and_the_final_one(tmp_path):
    _run(tmp_path, 6, period=1, max_to_keep=2)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["model_0000004.pth", "model_0000005.pth", "model_final.pth"]
    _run(tmp_path, 9, period=1, max_to_keep=0, resume=True)  # a resumed run prunes what the earlier one left, never model_final.pth
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["model_final.pth"]
    assert torch.load(tmp_path / "model_final.pth")["iteration"] == 8


def test_checkpoint_writes_are_atomic(tmp_path, monkeypatch):
    (tmp_path / "model_0000002.pth.tmp77").write_bytes(b"half a checkpoint")  # what a killed writer leaves behind
    (tmp_path / "last_checkpoint.tmp77").write_text("model_0000002.pth")
    model, opt, sched, recs = _run(tmp_path, 3, resume=True)
    assert [r["iteration"] for r in recs] == [0, 1, 2]  # nothing to resume from: the partial files are not checkpoints
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f and not f.endswith(".tmp77")]
    before = (tmp_path / "model_final.pth").read_bytes()

    def dies(obj, path, *a, **k):
        with open(path, "wb") as f:
            f.write(b"partial")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(OSError):
        F.save_checkpoint(str(tmp_path), "model_final.pth", model, opt, sched, 99)
    monkeypatch.undo()
    assert (tmp_path / "model_final.pth").read_bytes() == before and open(tmp_path / "last_checkpoint").read() == "model_final.pth"
    assert F._restore(F.last_checkpoint(str(tmp_path)), *_setup(5), None, None) == 3
    F.prune_checkpoints(str(tmp_path), 0)
    assert (tmp_path / "model_0000002.pth.tmp77").exists()  # only model_{iteration:07d}.pth is ever pruned


def _snapshot(model, opt):
    return copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()), {k: v["step"].clone() for k, v in opt.state.items() if "step" in v}


def test_gate_on_the_torch_route():
    model, opt, sched = _setup()
    batch = _batches(1)[0]
    for _ in range(2):
        train.train_step_gated(model, batch, opt, sched, clip_max_norm=35.0)
    assert opt.launches == 0  # CPU tensors: the torch route
    assert not opt.state.get(model.spare)  # no gradient, no state, no count

    def plant():
        g = torch.Generator().manual_seed(3)
        for p in model.lin.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        model.lin.weight.grad[0, 0], model.lin.weight.grad[-1, -1], model.lin.bias.grad[1] = float("nan"), float("inf"), -float("inf")
        model.spare.grad = None

    plant()
    want = [torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5) for p in model.lin.parameters()]
    sd_m, sd_o, steps = _snapshot(model, opt)
    norm = opt.step(torch.tensor([False]), 35.0)
    assert _same_tree(model.state_dict(), sd_m) and _same_tree(opt.state_dict(), sd_o)
    assert all(torch.equal(opt.state[k]["step"], v) for k, v in steps.items())
    assert all(torch.equal(p.grad, w) for p, w in zip(model.lin.parameters(), want))  # cleaned in place, not scaled by the clip coefficient
    ref = torch.cat([w.flatten() for w in want]).double().norm()
    assert abs(float(norm) - float(ref)) <= 1e-6 * float(ref)
    for flag in (torch.tensor([True]), None):
        plant()
        sd_m, sd_o, steps = _snapshot(model, opt)
        opt.step(flag, 35.0)
        assert not _same_tree(model.state_dict(), sd_m) and not _same_tree(opt.state_dict(), sd_o)
        assert all(int(opt.state[k]["step"]) == int(v) + 1 for k, v in steps.items())
        assert torch.equal(model.spare, torch.ones(2)) and not opt.state.get(model.spare)

    # the whole step: a NaN label -> FloatingPointError and nothing moved, the schedule included
    sd_m, sd_o, _ = _snapshot(model, opt)
    epoch = sched.last_epoch
    bad = {"x": batch["x"], "y": batch["y"].clone()}
    bad["y"][1, 2] = float("nan")
    with pytest.raises(FloatingPointError):
        train.train_step_gated(model, bad, opt, sched, clip_max_norm=35.0)
    assert _same_tree(model.state_dict(), sd_m) and _same_tree(opt.state_dict(), sd_o) and sched.last_epoch == epoch


def test_torch_route_follows_adam_and_exchanges_state_with_it():
    """The torch route against torch.optim.Adam on the same gradients (no clipping, finite values): 3 + 2 steps with the state handed over
    through state_dict() in both directions."""
    def grads(model, k):
        g = torch.Generator().manual_seed(50 + k)
        for p in model.lin.parameters():
            p.grad = torch.randn(p.shape, generator=g)

    def chain(first, second):
        torch.manual_seed(0)
        model = _Toy()
        a = first(model.lin.parameters(), lr=1e-2, betas=(0.5, 0.999), eps=1e-6)
        for k in range(3):
            grads(model, k)
            a.step()
        b = second(model.lin.parameters(), lr=1e-2, betas=(0.5, 0.999), eps=1e-6)
        b.load_state_dict(a.state_dict())
        for k in range(3, 5):
            grads(model, k)
            b.step()
        assert all(float(st["step"]) == 5 for st in b.state_dict()["state"].values())
        return torch.cat([p.detach().flatten() for p in model.lin.parameters()])

    runs = [chain(a, b) for a in (FusedAdam, torch.optim.Adam) for b in (FusedAdam, torch.optim.Adam)]
    for r in runs[:3]:
        assert torch.allclose(r, runs[3], rtol=0, atol=4 * 2.0 ** -24)  # values of magnitude < 1: a few roundings of the last place


def test_chunk_table_cuts_tensors_into_fixed_chunks_with_64_bit_offsets():
    from unopose_amd.optim import chunk_table

    big = 2 ** 31 + 5
    t = chunk_table([1, 0, 4096, 4097, big], 4096)
    assert t.dtype == np.int32 and t.shape == (1 + 0 + 1 + 2 + 2 ** 19 + 1, 4)
    off = t[:, 2:4].copy().view("<i8").reshape(-1)
    assert t[:4, :2].tolist() == [[0, 1], [2, 4096], [3, 4096], [3, 1]] and off[:4].tolist() == [0, 0, 0, 4096]
    assert t[-1, :2].tolist() == [4, 5] and off[-1] == 2 ** 31 and t[-2, :2].tolist() == [4, 4096] and off[-2] == 2 ** 31 - 4096
    for k in (0, 2, 3, 4):  # every tensor is covered exactly once, in order
        rows = t[:, 0] == k
        assert int(t[rows, 1].sum()) == [1, 0, 4096, 4097, big][k] and (np.diff(off[rows]) == 4096).all()
    assert chunk_table([], 4096).shape == (0, 4) and chunk_table([0, 0], 4096).shape == (0, 4)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return megapose_synth.build(str(tmp_path_factory.mktemp("megapose_fit")))


def _two_batches(tree, seed):
    from unopose_amd.provider_train import MegaPoseOneRefTrainSet

    ds = MegaPoseOneRefTrainSet(tree, num_img_per_epoch=8, color_augmentor="default", seed=seed)
    np.random.seed(seed)
    ds.reset()
    it = iter(F.build_loader(ds, 2, workers=2, seed=seed))
    out = [next(it) for _ in range(2)]
    del it  # the workers stop here, not at some later collection
    gc.collect()
    return out


def test_loader_on_the_synthetic_tree_is_seeded(tree):
    a, b = _two_batches(tree, 5), _two_batches(tree, 5)
    shapes = {"pts": (2, 192, 3), "rgb": (2, 3, 56, 56), "rgb_choose": (2, 192), "translation_label": (2, 3), "rotation_label": (2, 3, 3),
              "tem1_rgb": (2, 3, 56, 56), "tem1_choose": (2, 300), "tem1_pts": (2, 300, 3), "K": (2, 3, 3)}
    for x, y in zip(a, b):
        assert {k: tuple(v.shape) for k, v in x.items()} == shapes
        assert all(torch.equal(x[k], y[k]) for k in shapes)
    assert not torch.equal(a[0]["pts"], a[1]["pts"])


def test_rank_streams_share_one_permutation():
    import itertools

    take = lambda s, n: list(itertools.islice(iter(s), n))  # noqa: E731
    r0, r1 = take(F.RankSampler(10, 7, 0, 2), 10), take(F.RankSampler(10, 7, 1, 2), 10)
    whole = take(F.RankSampler(10, 7), 20)
    assert sorted(r0[:5] + r1[:5]) == list(range(10)) and sorted(whole[:10]) == sorted(whole[10:]) == list(range(10))
    assert r0 == whole[0::2] and r1 == whole[1::2]
    assert take(F.RankSampler(10, 7, 1, 2, start=3), 4) == r1[3:7]  # a resumed run picks the stream up where it stopped
    assert take(F.RankSampler(10, 8), 10) != whole[:10]


def _world2(rank, world, port, out, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    model = train.wrap_ddp(_Toy(spare=False))  # (every parameter takes part in the reduction)
    opt = FusedAdam([p for p in model.parameters()], lr=1e-2, betas=(0.5, 0.999), eps=1e-6)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: train.flat_and_anneal_factor(it, 100, warmup_iters=2))
    recs = F.fit(model, None, _batches(4, seed=100 + rank), opt, sched, out, 8, period=4, log_period=4, clip_max_norm=35.0, rank=rank, world=world,
                 log=lambda line: None)
    w = torch.cat([p.detach().flatten() for p in model.parameters()])
    ws = [torch.empty_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    if rank == 0:
        q.put((float((ws[0] - ws[1]).abs().max()), [r["iteration"] for r in recs], recs[0]["total_loss"], recs[-1]["total_loss"]))
    else:
        assert recs == []
    dist.destroy_process_group()


def test_fit_world2_gloo_keeps_the_replicas_identical(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    mp.spawn(_world2, args=(2, 29541, str(tmp_path), q), nprocs=2, join=True)
    spread, iters, first, last = q.get()
    assert spread == 0.0 and iters == [3, 7] and last < first
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["model_0000003.pth", "model_0000007.pth", "model_final.pth"]
    assert len(open(tmp_path / "metrics.json").readlines()) == 2  # rank 0 alone writes


def test_command_line_and_config_keys(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        F.main(["--help"])
    assert e.value.code == 0 and "--resume" in capsys.readouterr().out
    cfg = {"train": {"max_iter": 1000, "resample_times": 4, "checkpointer": {"period": 100, "max_to_keep": 3}, "seed": 9, "log_period": 10,
                     "clip_grad": {"enabled": True, "params": {"max_norm": 35, "norm_type": 2}}, "amp": {"enabled": True}, "amp_dtype": "bfloat16"},
           "dataloader": {"train": {"total_batch_size": 16, "num_workers": 24, "dataset": {"cfg": {}}}}, "misc": {"output_dir": "/somewhere"}, "model": {}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))

    def plan(*argv):
        assert F.main(["--config", str(path), "--print-plan", *argv]) == 0
        return json.loads(capsys.readouterr().out)

    p = plan()
    assert (p["max_iter"], p["resample_times"], p["period"], p["max_to_keep"], p["seed"], p["log_period"]) == (1000, 4, 100, 3, 9, 10)
    assert p["clip_max_norm"] == 35.0 and p["amp"] is True and p["batch_size"] == 16 and p["output_dir"] == "/somewhere"
    assert p["workers"] == 15  # 24 asked for; one rank and its workers are held to 16 processes
    p = plan("--gpus", "2", "--max-iter", "50", "--batch-size", "8", "--workers", "3", "--seed", "4", "--output-dir", "/else", "--resume",
             "train.clip_grad.enabled=False", "train.log_period=5", "train.amp.enabled=False")
    assert (p["max_iter"], p["batch_size"], p["workers"], p["seed"], p["output_dir"], p["resume"], p["gpus"]) == (50, 8, 3, 4, "/else", True, 2)
    assert p["clip_max_norm"] is None and p["log_period"] == 5 and p["amp"] is False
    assert plan("--gpus", "2")["workers"] == 7 and plan("--gpus", "2")["batch_size"] == 8  # 2 x (7 + 1) = 16; total_batch_size over the ranks
    path.write_text(json.dumps(dict(cfg, train=dict(cfg["train"], amp_dtype="float16"))))
    with pytest.raises(ValueError):
        F.main(["--config", str(path), "--print-plan"])
