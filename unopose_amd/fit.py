"""The training run: what ``engine.do_train`` (core/unopose/engine/engine.py:87-220) does, on this package:

    python -m unopose_amd.fit --config CFG --output-dir DIR [--gpus N] [--resume | --load-from CKPT] [key=value ...]

* CFG is read by ``cli.load_config`` (json / yaml / py); ``key=value`` overrides as in ``cli``.  Keys, spelled as in ``configs/main_cfg.py:56-85``:
  ``train.max_iter``, ``train.resample_times``, ``train.checkpointer.period`` / ``.max_to_keep``, ``train.clip_grad.enabled`` /
  ``.params.max_norm``, ``train.amp.enabled`` with ``train.amp_dtype`` (only ``bfloat16``: no GradScaler here), ``train.seed``,
  ``train.log_period``; ``dataloader.train.dataset.cfg`` + ``.num_img_per_epoch`` (the provider's fields), ``dataloader.train.batch_size``
  (pairs per rank; else ``total_batch_size`` divided by the ranks) and ``.num_workers``; ``model.cfg``; optional ``optimizer.lr / betas / eps /
  weight_decay`` and ``lr_multiplier.warmup_iters / warmup_factor / anneal_point / target_lr_factor`` (defaults: the configured Adam and schedule).
  ``--max-iter --batch-size --workers --seed --output-dir`` override the file.
* one step = ``train.train_step_gated``: forward, loss, backward, then ``optim.FusedAdam`` (gradient hygiene, clipping and Adam in three HIP
  launches) gated on the device by the finite-loss flag; one host wait per step.
* data: ``provider_train.MegaPoseOneRefTrainSet`` behind ``torch.utils.data.DataLoader`` (``collate_pairs``, pinned, ``drop_last``, spawned
  CPU-only workers).  ``dataset.reset()`` at the start and whenever ``iteration % (max_iter // resample_times) == 0``, as the reference.  Rank r of
  W reads positions r, r + W, ... of ONE endless stream of seeded permutations (:class:`RankSampler`, TrainingSampler's rule).  Worker w of a
  rank seeds ``random``, ``np.random`` and torch with base + w, base = seed + rank * workers.
* ``--device-crops`` (or ``dataloader.train.device_crops=true``): the workers stop at the window crop and draw the colour augmentation's
  parameters only (``ColorAugmentor.plan``); ``collate_pairs_device`` ships the crops as one uint8 atlas and ``ops.finish_crops`` runs the
  augmentation, the mask, the resize and the normalisation on the rank's GPU when the batch is taken.  Same samples as the host route but for
  the grayscale operator's last bit (``ColorAugmentor``).  Off by default.
* ``--online-models DIR`` (or ``dataloader.train.online.models=DIR``; ``--online-obj-ids`` / ``.obj_ids``): no dataset at all.  ``provider_online.OnlinePairs``
  renders (query, reference) pairs of the folder's ``obj_XXXXXX.ply`` models on the rank's GPU and builds the items there (``dataloader.train.online.*``:
  canvas, focal, fill, offset, occluder_prob, ssaa, shading, ambient, max_chunks; the provider's fields still come from ``dataloader.train.dataset.cfg``).
  Batch i is a function of (seed, rank, i): ``--workers`` is ignored, ``--resume`` needs the iteration only.  ``--host`` builds the items with the numpy
  rule from the renders read back (the same batches).  Off by default.  ``--online-scene`` (or any ``dataloader.train.online.scene.KEY=VALUE``)
  adds the scene stage of ``provider_online`` (part 4 of its docstring): a textured background plane behind the query and a depth-sensor
  model on both views; without it the batches are the same bits as before the stage existed.
* ranks: ``--gpus N`` starts N fresh processes before this one touches a GPU (RCCL through ``nccl``; ``gloo`` without GPUs); each runs
  ``freeze_backbone`` + ``wrap_ddp``.
* rank 0 writes, into the output directory, ``model_{iteration:07d}.pth`` every ``period`` iterations (the newest ``max_to_keep`` are kept),
  ``model_final.pth`` and the text file ``last_checkpoint`` (detectron2's convention); a checkpoint is ``{"model", "optimizer", "scheduler",
  "iteration", "rng", "img_idx"}``, written under a temporary name and renamed.  ``--resume`` continues from ``last_checkpoint``;
  ``--load-from`` reads weights only.  A resumed run repeats the uninterrupted one bit for bit when the loader has no workers; with workers the
  permutation stream resumes where it stopped and the workers' random streams start afresh.
* ``metrics.json``: one JSON object per ``log_period`` iterations (and for the last): ``iteration, total_loss, every *_loss*, lr,
  total_grad_norm, time, data_time`` (seconds per iteration since the previous line); the same on the console.  The scalars are stacked into one
  device vector and copied at those iterations only.
* a non-finite loss (or any other non-finite scalar of ``process_loss``: how a NaN label shows) ends the run with ``FloatingPointError`` after ``model_nonfinite_{iteration}.pth`` has been written: the gate kept the update
  off, so that file holds the state before the failing step.
Out of scope: tensorboard, visualisation, model EMA, fp16 + GradScaler, evaluation during training."""
import argparse
import itertools
import json
import os
import os.path as osp
import random
import re
import sys
import time

import numpy as np
import torch

from .cli import _launch_ranks, apply_overrides, load_checkpoint, load_config
from .optim import FusedAdam
from .train import flat_and_anneal_factor, freeze_backbone, train_step_gated, wrap_ddp

PERIODIC = re.compile(r"^model_\d{7}\.pth$")


class RankSampler(torch.utils.data.Sampler):
    """Positions rank, rank + world, ... of an endless stream of permutations of range(size) drawn from ONE generator seeded with `seed` on every
    rank (detectron2's TrainingSampler, my_distributed_sampler.py:58-67), starting `start` draws of this rank into the stream."""

    def __init__(self, size, seed, rank=0, world=1, start=0):
        if size <= 0:
            raise ValueError(f"RankSampler: size {size}")
        self.size, self.seed, self.rank, self.world, self.start = int(size), int(seed), rank, world, start

    def _stream(self):
        g = torch.Generator()
        g.manual_seed(self.seed)
        while True:
            yield from torch.randperm(self.size, generator=g).tolist()

    def __iter__(self):
        return itertools.islice(self._stream(), self.rank + self.start * self.world, None, self.world)


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed % 2 ** 32)
    torch.manual_seed(seed)


class _WorkerInit:
    """Worker w: base + w into `random`, `np.random` and torch, and into the dataset copy's colour augmentation (a picklable callable: spawn)."""

    def __init__(self, base):
        self.base = base

    def __call__(self, worker_id):
        seed_all(self.base + worker_id)
        ds = torch.utils.data.get_worker_info().dataset
        if getattr(ds, "color_augmentor", None) is not None and hasattr(ds.color_augmentor, "rng"):
            ds.color_augmentor.rng = np.random.default_rng(self.base + worker_id)


def build_loader(dataset, batch_size, workers=8, seed=1, rank=0, world=1, start_iteration=0, pin_memory=False):
    """The training loader over `dataset` (already `reset()`), positioned at the batch of `start_iteration`.  A `device_crops` dataset is
    collated by `collate_pairs_device`: its batches are finished by `ops.finish_crops` (fit does that when it takes a batch)."""
    import functools

    from .provider_train import collate_pairs, collate_pairs_device

    collate = collate_pairs
    if getattr(dataset, "device_crops", False):
        collate = functools.partial(collate_pairs_device, img_size=dataset.img_size, rgb_mask_flag=dataset.rgb_mask_flag)
    sampler = RankSampler(len(dataset), seed, rank, world, start=start_iteration * batch_size)
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler, num_workers=workers, collate_fn=collate,
                                       pin_memory=pin_memory, drop_last=True, worker_init_fn=_WorkerInit(seed + rank * max(workers, 1)),
                                       multiprocessing_context="spawn" if workers else None)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
def _atomic(path, write):
    tmp = f"{path}.tmp{os.getpid()}"
    write(tmp)
    os.replace(tmp, path)


def save_checkpoint(out_dir, name, model, optimizer, scheduler, iteration, dataset=None, device=None, last=True):
    """{"model", "optimizer", "scheduler", "iteration"} + the random states and the epoch's view indices a resume needs -> out_dir/name, atomically."""
    net = model.module if hasattr(model, "module") else model
    # (plain Python values and tensors only: the file loads under torch.load's weights_only rule, which cli.load_checkpoint relies on)
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    rng = {"python": random.getstate(), "numpy": (kind, torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(gauss)),
           "torch": torch.get_rng_state()}
    if device is not None and torch.device(device).type == "cuda":
        rng["cuda"] = torch.cuda.get_rng_state(device)
    ck = {"model": net.state_dict(), "optimizer": optimizer.state_dict(), "scheduler": None if scheduler is None else scheduler.state_dict(),
          "iteration": iteration, "rng": rng,
          "img_idx": None if getattr(dataset, "img_idx", None) is None else torch.from_numpy(np.asarray(dataset.img_idx, dtype=np.int64))}
    _atomic(osp.join(out_dir, name), lambda tmp: torch.save(ck, tmp))
    if last:
        def text(tmp):
            with open(tmp, "w") as f:
                f.write(name)
        _atomic(osp.join(out_dir, "last_checkpoint"), text)


def prune_checkpoints(out_dir, max_to_keep):
    """Keep the newest `max_to_keep` periodic files (model_{iteration:07d}.pth); nothing else is ever deleted."""
    if max_to_keep is None or max_to_keep < 0:
        return
    files = sorted(f for f in os.listdir(out_dir) if PERIODIC.match(f))
    for f in files[:max(len(files) - max_to_keep, 0)]:
        os.remove(osp.join(out_dir, f))


def last_checkpoint(out_dir):
    path = osp.join(out_dir, "last_checkpoint")
    if not osp.exists(path):
        return None
    with open(path) as f:
        name = f.read().strip()
    return osp.join(out_dir, name) if name and osp.exists(osp.join(out_dir, name)) else None


def _restore(path, model, optimizer, scheduler, dataset, device):
    ck = torch.load(path, map_location="cpu")
    net = model.module if hasattr(model, "module") else model
    net.load_state_dict(ck["model"], strict=True)
    optimizer.load_state_dict(ck["optimizer"])
    if scheduler is not None and ck.get("scheduler") is not None:
        scheduler.load_state_dict(ck["scheduler"])
    rng = ck.get("rng") or {}
    if "python" in rng:
        version, words, gauss_next = rng["python"]
        random.setstate((version, tuple(words), gauss_next))
        kind, keys, pos, has_gauss, gauss = rng["numpy"]
        np.random.set_state((kind, keys.numpy().astype(np.uint32), pos, has_gauss, gauss))
        torch.set_rng_state(rng["torch"])
    if "cuda" in rng and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(rng["cuda"], device)
    if dataset is not None and ck.get("img_idx") is not None:
        dataset.img_idx = ck["img_idx"].numpy()
        if getattr(dataset, "num_img_per_epoch", None) == -1:
            dataset.num_img_per_epoch = len(ck["img_idx"])
    return ck["iteration"] + 1


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
def _batches(loader, iteration):
    """An iterator whose first item is the batch of `iteration`.  `loader`: a callable (iteration -> iterable; the run's DataLoader factory), a
    sequence of resident batches (walked round and round: position = iteration mod length) or any re-iterable (restarted when exhausted)."""
    if callable(loader):
        return iter(loader(iteration))
    if hasattr(loader, "__getitem__") and hasattr(loader, "__len__"):
        return (loader[i % len(loader)] for i in itertools.count(iteration))
    return itertools.chain.from_iterable(itertools.repeat(loader))


def fit(model, dataset, loader, optimizer, scheduler, output_dir, max_iter, *, period=5000, max_to_keep=2, log_period=50, clip_max_norm=None,
        amp_dtype=None, resample_times=1, resume=False, device=None, rank=0, world=1, seed=1, log=print):
    """Iterations start .. max_iter - 1 of the run; returns the list of metric records this call wrote (rank 0; [] elsewhere).
    `dataset`: None or an object with reset() (called at the start and at the resample points, before the loader is re-opened).
    `loader`: see :func:`_batches`.  `optimizer`: an `optim.FusedAdam`; `model`: already on `device`, wrapped for data parallelism if world > 1."""
    import torch.distributed as dist

    dev = torch.device(device) if device is not None else next(model.parameters()).device
    main = rank == 0
    if main:
        os.makedirs(output_dir, exist_ok=True)
    start = 0
    ck = last_checkpoint(output_dir) if resume else None
    if ck is not None:
        start = _restore(ck, model, optimizer, scheduler, dataset, dev)
        if rank:  # rank 0's random states are the ones on file; the others restart theirs from (seed, rank, iteration)
            seed_all(seed + rank + 7919 * start)
    elif dataset is not None:
        dataset.reset()
    segment = max(max_iter // max(resample_times, 1), 1)
    batches = _batches(loader, start)
    records, keys = [], None
    t_mark, data_s, n_mark = time.perf_counter(), 0.0, 0
    metrics = open(osp.join(output_dir, "metrics.json"), "a") if main else None
    try:
        for iteration in range(start, max_iter):
            if iteration > 0 and iteration % segment == 0 and dataset is not None:
                dataset.reset()
                batches = _batches(loader, iteration)
            t0 = time.perf_counter()
            batch = next(batches)
            if "crop_atlas" in batch:  # a device_crops loader: the colour augmentation, mask, resize and normalisation happen here
                from .ops import finish_crops

                batch = finish_crops(batch, dev)
            else:
                batch = {k: v.to(dev, non_blocking=True) for k, v in batch.items()}
            data_s += time.perf_counter() - t0
            lr = optimizer.param_groups[0]["lr"]
            try:
                info = train_step_gated(model, batch, optimizer, scheduler, clip_max_norm=clip_max_norm, amp_dtype=amp_dtype)
            except FloatingPointError:
                if main:  # the gate kept the update off: this is the state before the failing step
                    save_checkpoint(output_dir, f"model_nonfinite_{iteration}.pth", model, optimizer, scheduler, iteration - 1, dataset, dev, last=False)
                raise
            n_mark += 1
            if (iteration + 1) % log_period == 0 or iteration == max_iter - 1:
                if keys is None:
                    keys = sorted(k for k in info if "loss" in k and k != "loss")
                vec = torch.stack([info[k].float().reshape(()) for k in keys + ["total_grad_norm"]])
                if world > 1:  # the ranks' mean, as comm.reduce_dict; every rank reaches this line at the same iterations
                    dist.all_reduce(vec)
                    vec = vec / world
                vals = vec.cpu().tolist()  # the only copy of scalars to the host
                now = time.perf_counter()
                rec = {"iteration": iteration, "total_loss": sum(vals[:-1])}
                rec.update(zip(keys, vals[:-1]))
                rec.update(lr=lr, total_grad_norm=vals[-1], time=(now - t_mark) / n_mark, data_time=data_s / n_mark)
                t_mark, data_s, n_mark = now, 0.0, 0
                if main:
                    records.append(rec)
                    metrics.write(json.dumps(rec) + "\n")
                    metrics.flush()
                    log("iter %d  total_loss %.4g  %s  lr %.3g  grad_norm %.4g  time %.4f  data_time %.4f" % (
                        iteration, rec["total_loss"], "  ".join("%s %.4g" % (k, rec[k]) for k in keys), lr, rec["total_grad_norm"], rec["time"], rec["data_time"]))
            if main and (iteration + 1) % period == 0:
                save_checkpoint(output_dir, f"model_{iteration:07d}.pth", model, optimizer, scheduler, iteration, dataset, dev)
                prune_checkpoints(output_dir, max_to_keep)
            if main and iteration >= max_iter - 1:
                save_checkpoint(output_dir, "model_final.pth", model, optimizer, scheduler, iteration, dataset, dev)
    finally:
        if metrics is not None:
            metrics.close()
    return records


# ---- command line --------------------------------------------------------------------------------------------------------------------
def run_settings(cfg, args, world=1):
    """The run's numbers from the config mapping and the command line (the command line wins)."""
    tr = cfg.get("train", {})
    dl = cfg.get("dataloader", {}).get("train", {})
    clip = tr.get("clip_grad", {})
    amp = bool(tr.get("amp", {}).get("enabled", False))
    if amp and tr.get("amp_dtype", "bfloat16") != "bfloat16":
        raise ValueError("train.amp_dtype: only bfloat16 (fp16 needs a GradScaler, which this run does not have)")
    batch = args.batch_size or dl.get("batch_size") or max(int(dl.get("total_batch_size", world)) // world, 1)
    workers = args.workers if args.workers is not None else int(dl.get("num_workers", 8))
    if world * (workers + 1) > args.max_procs:  # every rank is a process and so is each of its workers
        workers = max(args.max_procs // world - 1, 0)
    return dict(max_iter=int(args.max_iter or tr.get("max_iter", 188340)), resample_times=int(tr.get("resample_times", 1)),
                period=int(tr.get("checkpointer", {}).get("period", 5000)), max_to_keep=int(tr.get("checkpointer", {}).get("max_to_keep", 2)),
                clip_max_norm=float(clip.get("params", {}).get("max_norm", 35)) if clip.get("enabled", False) else None,
                amp=amp, seed=int(args.seed if args.seed is not None else tr.get("seed", 1)), log_period=int(tr.get("log_period", 50)),
                batch_size=int(batch), workers=int(workers), output_dir=args.output_dir or cfg.get("misc", {}).get("output_dir"),
                load_from=args.load_from or cfg.get("misc", {}).get("load_from") or None,
                device_crops=bool(args.device_crops or dl.get("device_crops", False)),
                online_models=args.online_models or dl.get("online", {}).get("models") or None,
                online_obj_ids=args.online_obj_ids or dl.get("online", {}).get("obj_ids") or None, online_host=bool(args.host),
                online_scene=bool(args.online_scene or dl.get("online", {}).get("scene") is not None))


def _parser():
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.fit", description="Train UNOPose: a resumable run on the fused HIP Adam step.")
    ap.add_argument("--config", required=True, help="json / yaml / py file with the reference's train.*, dataloader.train.*, model keys")
    ap.add_argument("--output-dir", help="checkpoints, last_checkpoint and metrics.json go here (default: misc.output_dir)")
    ap.add_argument("--load-from", help="weights only (default: misc.load_from)")
    ap.add_argument("--resume", action="store_true", help="continue from the output directory's last_checkpoint")
    ap.add_argument("--max-iter", type=int)
    ap.add_argument("--batch-size", type=int, help="pairs per rank")
    ap.add_argument("--workers", type=int, help="loader processes per rank (default: dataloader.train.num_workers, else 8)")
    ap.add_argument("--max-procs", type=int, default=16, help="ranks x (workers + 1) is held to this many processes by lowering the workers")
    ap.add_argument("--gpus", type=int, default=1, help="ranks; 0 = one rank on the CPU")
    ap.add_argument("--seed", type=int)
    ap.add_argument("--device-crops", action="store_true",
                    help="finish the crops of a batch on the GPU (colour augmentation, mask, resize, normalise); also dataloader.train.device_crops=true")
    ap.add_argument("--online-models", help="train on pairs rendered on the GPU from this folder of obj_XXXXXX.ply models (provider_online.OnlinePairs) "
                    "in place of the MegaPose files; also dataloader.train.online.models=DIR.  --workers is ignored")
    ap.add_argument("--online-obj-ids", type=int, nargs="*", help="with --online-models: these objects only (default: every model of the folder)")
    ap.add_argument("--online-scene", action="store_true",
                    help="with --online-models: a textured background plane behind the query and a depth-sensor model (holes, edge drop-outs, "
                    "axial noise, disparity quantisation) on both views, at the defaults; dataloader.train.online.scene.KEY=VALUE sets single keys")
    ap.add_argument("--host", action="store_true", help="with --online-models: build the items with the numpy rule from the renders read back")
    ap.add_argument("--print-plan", action="store_true", help="resolve the settings, print them as JSON and stop (touches no GPU)")
    ap.add_argument("opts", nargs="*", help="key=value overrides")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    cfg = apply_overrides(load_config(args.config), args.opts)
    ranks = max(args.gpus, 1)
    s = run_settings(cfg, args, world=ranks)
    if args.print_plan:
        print(json.dumps(dict(s, gpus=args.gpus, resume=bool(args.resume))))
        return 0
    if not s["output_dir"]:
        raise SystemExit("no output directory: --output-dir or misc.output_dir")
    if ranks > 1 and "WORLD_SIZE" not in os.environ:
        return _launch_ranks(ranks, list(argv if argv is not None else sys.argv[1:]), module="unopose_amd.fit")

    import torch.distributed as dist

    from .model import UNOPose
    from .provider_train import MegaPoseOneRefTrainSet

    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    on_gpu = args.gpus > 0
    dev = torch.device("cuda", local) if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(local)
    if world > 1:
        import datetime

        dist.init_process_group("nccl" if on_gpu else "gloo", timeout=datetime.timedelta(minutes=10), **({"device_id": dev} if on_gpu else {}))
    seed_all(s["seed"] + rank)
    mcfg = cfg["model"].get("cfg", cfg["model"])
    model = UNOPose(mcfg)
    if s["load_from"] and not args.resume:
        load_checkpoint(model, s["load_from"])
    model = freeze_backbone(model.to(dev))
    if world > 1:
        model = wrap_ddp(model, dev)
    oc, lm = cfg.get("optimizer", {}), cfg.get("lr_multiplier", {})
    optimizer = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=oc.get("lr", 1e-4), betas=tuple(oc.get("betas", (0.5, 0.999))),
                          eps=oc.get("eps", 1e-6), weight_decay=oc.get("weight_decay", 0.0))
    sched_kw = {k: lm[k] for k in ("warmup_iters", "warmup_factor", "anneal_point", "target_lr_factor") if k in lm}
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda it: flat_and_anneal_factor(it, s["max_iter"], **sched_kw))
    dc = cfg["dataloader"]["train"]["dataset"]
    if s["device_crops"] and not on_gpu:
        raise SystemExit("--device-crops needs a GPU rank (--gpus >= 1)")
    if s["online_models"]:  # rendered pairs: no dataset state, no workers; batch i is a function of (seed, rank, i), so a resume needs the iteration only
        if not on_gpu:
            raise SystemExit("--online-models needs a GPU rank (--gpus >= 1)")
        from .provider_online import OnlinePairs

        online = dict(cfg["dataloader"]["train"].get("online", {}))
        if s["online_scene"] and online.get("scene") is None:
            online["scene"] = {}  # the stage at its defaults
        dataset = None
        loader = OnlinePairs(s["online_models"], dict(dc.get("cfg", dc), online=online), dev, s["seed"], rank=rank, world=world, host=s["online_host"],
                             batch_size=s["batch_size"], obj_ids=s["online_obj_ids"])
    else:
        dataset = MegaPoseOneRefTrainSet(dc.get("cfg", dc), num_img_per_epoch=int(dc.get("num_img_per_epoch", -1)), seed=s["seed"] + rank,
                                         device_crops=s["device_crops"])

        def loader(iteration):
            return build_loader(dataset, s["batch_size"], s["workers"], s["seed"], rank, world, start_iteration=iteration, pin_memory=on_gpu)

    try:
        fit(model, dataset, loader, optimizer, scheduler, s["output_dir"], s["max_iter"], period=s["period"], max_to_keep=s["max_to_keep"],
            log_period=s["log_period"], clip_max_norm=s["clip_max_norm"], amp_dtype=torch.bfloat16 if s["amp"] else None,
            resample_times=s["resample_times"], resume=args.resume, device=dev, rank=rank, world=world, seed=s["seed"])
    finally:
        if world > 1:
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
