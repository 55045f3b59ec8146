"""Command-line entry of the test run (SURVEY.md 8(b) "CLI / config boundary"): what ``core/unopose/save_unopose.sh`` ->
``main_unopose.py --config-file CFG --num-gpus N test.save_results_only=True misc.load_from=CKPT [key=value ...]`` ->
``engine.do_save_results`` (core/unopose/engine/engine.py:36-72) does, on this package:

    python -m unopose_amd.cli --config-file CFG --num-gpus N misc.load_from=CKPT [key=value ...]

* CFG: a ``.json`` / ``.yaml`` file, or a ``.py`` file that leaves a mapping named ``cfg`` (or the LazyConfig layout's top-level
  names ``model``, ``dataloader``, ``test``, ``misc``, ``bop_eval``) -- the keys ``do_save_results`` reads: ``model.cfg`` (or ``model``),
  ``dataloader.test.dataset`` (the provider's fields + ``eval_dataset_name`` + ``detetion_path``, spelled as in the reference),
  ``test.amp.enabled``, ``test.instance_batch_size``, ``misc.output_dir``, ``misc.load_from``, ``misc.exp_name``, ``bop_eval.split``;
  ``key=value`` overrides use dotted keys and Python literals, like detectron2's LazyConfig.apply_overrides.
* result path = the reference's: ``<misc.output_dir>/inference_<checkpoint stem>/<dataset>/result<exp_name>_<dataset>-<split>.csv`` plus
  the sibling ``.json`` (runner.inference_and_save).
* ``--num-gpus N`` > 1 starts N ranks (one per GPU, RCCL) before this process touches a GPU; images are sharded by the
  InferenceSampler rule and rows gathered to rank 0.
* two deliberate differences from ``engine.do_save_results``: (1) ``test.amp.enabled=True`` selects **bf16** autocast here (the reference's
  ``torch.cuda.amp.autocast`` is fp16; bf16 is what the MI355X kernels are built and parity-tested for), ``False`` = fp32 as in the
  reference; (2) the reference always goes on to the BOP evaluation (``bop_eval_utils``) after saving -- this entry stops at the CSV
  unless ``--eval`` is given.  Then rank 0 scores the CSV with ``unopose_amd.bop_eval.score_csv`` on its GPU (VSD + MSSD + MSPD -> AR;
  HIP depth renderer, pose errors in HIP kernels; ``--eval-device-off`` keeps the renders but computes the errors on the host, for
  comparison), writes ``scores_bop19.json`` beside the CSV and prints one line with AR_VSD / AR_MSSD / AR_MSPD / AR.  It reads
  ``<data_dir>/<dataset>``: ``bop_eval.targets_filename`` (default ``test_targets_bop19.json``), ``models_eval/``, the ``bop_eval.split``
  folder; ``bop_eval.n_top`` (default -1: the targets' instance counts) and ``bop_eval.vsd_delta`` (default 15 mm, ITODD 5 mm,
  bop_eval_utils.py:348-362) are spelled as in the reference's ``val_cfg``.  So is ``bop_eval.error_types``, a comma-separated string (or a
  list) of the error types of ``lib/pysixd/scripts/eval_pose_results_more.py``: ``vsd, mssd, mspd, add, adi, ad, ABSadd, ABSadi, ABSad, AUCadd,
  AUCadi, AUCad, re, te, rete, proj, reS, teS, reteS, projS`` (``bop_eval.error_types=ad,rete,proj`` is the reference's default table and needs
  no renderer).  Each type beyond the BOP'19 three is scored on the same route -- ``ops.pose_metrics`` / ``ops.adi`` on the GPU, numpy with
  ``--eval-device-off`` --, gets a line with its recalls after the AR line, and one per-object table follows (objects in rows,
  ``type_threshold`` in columns, an ``Avg`` row, as ``bop_eval_utils.summary_scores`` lays it out); the scores file gains an ``errors`` key.
  ``bop_eval.symmetric_obj_ids`` lists the objects that take ADI under ``ad / ABSad / AUCad`` (default: the objects whose ``models_info.json``
  entry lists a symmetry -- not the reference's per-dataset id tables).  An unknown type is an error before any GPU work.  The mask-overlap
  error ``cus`` stays out.  ``bop_eval.gt_visibility`` (``off`` -- the default: every ground truth of a targeted object counts --, ``file`` or
  ``compute``) selects the toolkit's rule for which ground truths count, from ``scene_gt_info.json`` or computed on the GPU
  (``unopose_amd.gt_info``), with ``bop_eval.visib_gt_min`` as in the reference's ``eval_calc_scores.py`` (-1: the ``inst_count`` most visible) and, for ``compute``,
  ``bop_eval.gt_delta``, the visibility tolerance in mm (default: the one BOP's files are made with, 15, ITODD 5); either key without the mode it
  belongs to is an error.  ``bop_eval.models_info`` (``file`` -- the default: the diameters of ``models_eval/models_info.json`` --, or ``compute``)
  takes the diameters from the ``models_eval`` vertices of the targeted objects instead (``unopose_amd.model_info``: on the GPU, on the host with
  ``--eval-device-off``; the same bits), so meshes that come without the file can be scored; symmetries are still read from the file where it
  exists.  Any other value is an error before any GPU work.
* extras beyond the reference's line: ``--pipeline`` (two forwards in flight), ``--ref-cache`` (reference views encoded once),
  ``--device-prep`` (the provider builds each image's query crops, clouds and pixel indices on the rank's GPU: same items, same rows),
  ``--device-masks`` (with it: the detections' run-length masks are decoded there as well),
  ``--vis [DIR]`` (after the CSV is written rank 0 draws its estimates over the test images with ``unopose_amd.vis_poses`` -- the selection of
  ``bop_eval.n_top``, the dataset folder of ``--eval`` -- into DIR, by default ``vis/`` beside the CSV),
  ``--print-plan`` (resolve config and paths, touch no GPU: used by the CPU tests)."""
import argparse
import ast
import json
import os
import os.path as osp
import subprocess
import sys

from .model.config import Cfg


def load_config(path):
    if path.endswith(".json"):
        with open(path) as f:
            return json.load(f)
    if path.endswith((".yaml", ".yml")):
        import yaml

        with open(path) as f:
            return yaml.safe_load(f)
    if path.endswith(".py"):
        scope = {"__file__": path}
        with open(path) as f:
            exec(compile(f.read(), path, "exec"), scope)
        if isinstance(scope.get("cfg"), dict):
            return dict(scope["cfg"])
        return {k: scope[k] for k in ("model", "dataloader", "test", "misc", "bop_eval", "train") if k in scope}
    raise ValueError(f"unsupported config file {path} (json / yaml / py)")


def apply_overrides(cfg, overrides):
    """``a.b.c=value`` with Python-literal values (strings that are not literals stay strings)."""
    for item in overrides:
        if "=" not in item:
            raise ValueError(f"override {item!r} is not key=value")
        key, val = item.split("=", 1)
        try:
            val = ast.literal_eval(val)
        except (ValueError, SyntaxError):
            pass
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
            if not isinstance(node, dict):
                raise ValueError(f"override {key}: {p} is not a mapping")
        node[parts[-1]] = val
    return cfg


def fine_matching_cfg(cfg):
    """The ``fine_point_matching`` mapping the model is built from (``model.cfg`` where the config has one, else ``model``), created
    when absent.  An override written as ``model.fine_point_matching.key=value`` beside a ``model.cfg`` is moved into it."""
    model = cfg.setdefault("model", {})
    if not isinstance(model, dict):
        raise ValueError("config: model is not a mapping")
    inner = model["cfg"] if isinstance(model.get("cfg"), dict) else model
    fine = inner.setdefault("fine_point_matching", {})
    if inner is not model and isinstance(model.get("fine_point_matching"), dict):
        fine.update(model.pop("fine_point_matching"))
    return fine


def result_paths(cfg, iteration=None):
    """engine.py:37-52 -> (directory, csv path)."""
    cfg = Cfg(cfg)
    dataset_name = cfg.dataloader.test.dataset.eval_dataset_name
    sub = f"inference_iter_{iteration}" if iteration is not None else f"inference_{osp.splitext(osp.basename(cfg.misc.load_from))[0]}"
    out_dir = osp.join(cfg.misc.output_dir, sub, dataset_name)
    name = f"result{cfg.misc.get('exp_name', '')}_{dataset_name}-{cfg.bop_eval.split}.csv"
    return out_dir, osp.join(out_dir, name)


def eval_settings(cfg):
    """What ``--eval`` hands to ``bop_eval.score_csv``: the dataset folder of the provider and the ``bop_eval`` keys of the reference's
    ``val_cfg`` (bop_eval_utils.py:340-366)."""
    from .bop_eval import VSD_DELTA, VSD_DELTAS, parse_error_types

    dcfg = cfg["dataloader"]["test"]["dataset"]
    name = dcfg["eval_dataset_name"]
    data_dir = dcfg.get("cfg", dcfg).get("data_dir")
    if data_dir is None:
        raise ValueError("--eval: dataloader.test.dataset has no data_dir")
    be = cfg.get("bop_eval", {})
    sym_ids = be.get("symmetric_obj_ids")
    if isinstance(sym_ids, (str, int)):
        sym_ids = [v for v in str(sym_ids).split(",") if v.strip()]
    return dict(root=data_dir, name=name, split=be.get("split", "test"), targets_filename=be.get("targets_filename", "test_targets_bop19.json"),
                n_top=int(be.get("n_top", -1)), vsd_delta=float(be.get("vsd_delta", VSD_DELTAS.get(name, VSD_DELTA))),
                error_types=parse_error_types(be["error_types"]) if be.get("error_types") is not None else None,
                symmetric_obj_ids=None if sym_ids is None else sorted(int(v) for v in sym_ids),
                **_gt_visibility(be), models_info=_models_info(be))


def _models_info(be):
    """`bop_eval.models_info`: file or compute; None when the key is not given."""
    mode = be.get("models_info")
    if mode is not None and mode not in ("file", "compute"):
        raise ValueError(f"bop_eval.models_info={mode!r} (file or compute)")
    return mode


def _gt_visibility(be):
    """`bop_eval.gt_visibility`, `bop_eval.visib_gt_min` and `bop_eval.gt_delta`; the last two mean nothing without the first and are an error then."""
    mode, least, delta = be.get("gt_visibility"), be.get("visib_gt_min"), be.get("gt_delta")
    if mode is not None and mode not in ("off", "file", "compute"):
        raise ValueError(f"bop_eval.gt_visibility={mode!r} (off, file or compute)")
    if least is not None and mode in (None, "off"):
        raise ValueError("bop_eval.visib_gt_min needs bop_eval.gt_visibility=file or compute: without it every ground truth of a targeted object counts")
    if delta is not None and mode != "compute":
        raise ValueError("bop_eval.gt_delta is the visibility tolerance of bop_eval.gt_visibility=compute")
    return dict(gt_visibility=mode, visib_gt_min=None if least is None else float(least), gt_delta=None if delta is None else float(delta))


def _launch_ranks(n, argv, poll_s=0.2, module="unopose_amd.cli"):
    """N fresh interpreters with the torchrun environment contract; the parent has not initialised HIP.  All children are polled:
    when any one exits non-zero the others are terminated and that code is returned (as torchrun does) -- a rank that dies must not
    leave the rest blocked in a collective until the watchdog fires."""
    import socket
    import time

    with socket.socket() as s:  # a free port (bind-and-close: the window before rank 0 re-binds it is small; MASTER_PORT overrides)
        s.bind(("127.0.0.1", 0))
        port = os.environ.get("MASTER_PORT") or str(s.getsockname()[1])
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, "-m", module] + argv, env=env))
    while True:
        codes = [p.poll() for p in procs]
        bad = [c for c in codes if c not in (None, 0)]
        if bad:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
            return abs(bad[0])
        if all(c == 0 for c in codes):
            return 0
        time.sleep(poll_s)


def load_checkpoint(model, path):
    """A checkpoint as MyCheckpointer writes it ({"model": state_dict, ...}) or a bare state dict; strict."""
    import torch

    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.cli", description=__doc__.split("\n\n")[0],
                                 epilog="Differences from engine.do_save_results: test.amp.enabled=True means bf16 autocast (reference: fp16); "
                                        "the BOP evaluation is started after saving only with --eval (unopose_amd.bop_eval.score_csv).")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--num-gpus", type=int, default=1)
    ap.add_argument("--eval-only", action="store_true", help="accepted for compatibility with main_unopose.py")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--ref-cache", action="store_true")
    ap.add_argument("--device-prep", action="store_true", help="build the query side of every item on the GPU (provider device path)")
    ap.add_argument("--device-masks", action="store_true",
                    help="with --device-prep: decode the detections' run-length masks on the GPU as well (same items)")
    ap.add_argument("--eval", action="store_true", help="score the CSV after saving (BOP'19 AR; rank 0, on its GPU)")
    ap.add_argument("--eval-device-off", action="store_true", help="with --eval: compute the pose errors on the host (same renders), for comparison")
    ap.add_argument("--vis", nargs="?", const="", default=None, metavar="DIR",
                    help="draw the saved estimates over the test images after saving (unopose_amd.vis_poses; rank 0, on its GPU); DIR defaults to vis/ beside the CSV")
    ap.add_argument("--icp", nargs="?", const="10", default=None, metavar="ITERS",
                    help="refine every fine pose against its two clouds by at most ITERS (default 10) iterations of ops.icp_refine: sets "
                         "model.fine_point_matching.icp_iters (and icp_inlier_thres = 0.1 unless an override gives it)")
    ap.add_argument("--print-plan", action="store_true")
    ap.add_argument("opts", nargs="*", help="key=value overrides")
    args = ap.parse_args(argv)
    if args.device_masks and not args.device_prep:
        ap.error("--device-masks requires --device-prep")
    if args.vis and "=" in args.vis:  # `--vis key=value`: an override, not a folder
        args.opts, args.vis = [args.vis] + list(args.opts), ""
    if args.icp and "=" in args.icp:  # `--icp key=value`: an override, not a count
        args.opts, args.icp = [args.icp] + list(args.opts), "10"
    if args.icp is not None and not (args.icp.isdigit() and int(args.icp) >= 0):
        ap.error(f"--icp: ITERS must be a non-negative integer, got {args.icp!r}")
    cfg = apply_overrides(load_config(args.config_file), args.opts)
    fine = fine_matching_cfg(cfg)
    if args.icp is not None:
        fine["icp_iters"] = int(args.icp)
        fine.setdefault("icp_inlier_thres", 0.1)
    out_dir, save_path = result_paths(cfg)
    c = Cfg(cfg)
    if args.eval and isinstance(cfg.get("bop_eval"), dict):  # an unknown error type stops the run here, before any GPU work
        from .bop_eval import parse_error_types

        parse_error_types(cfg["bop_eval"].get("error_types"))
        _models_info(cfg["bop_eval"])
    if args.print_plan:
        plan = dict(save_path=save_path, dataset=c.dataloader.test.dataset.eval_dataset_name, checkpoint=c.misc.load_from,
                    amp=bool(c.test.amp.enabled), instance_batch_size=c.test.instance_batch_size, num_gpus=args.num_gpus,
                    device_prep=bool(args.device_prep), eval=bool(args.eval))
        if args.device_masks:
            plan.update(device_masks=True)
        if int(fine.get("icp_iters", 0) or 0) > 0:
            plan.update(icp_iters=int(fine["icp_iters"]), icp_inlier_thres=float(fine.get("icp_inlier_thres", 0.1)))
        if args.eval:
            from .bop_eval import dataset_paths

            ev = eval_settings(cfg)
            plan.update(eval_device=not args.eval_device_off, eval_paths=dataset_paths(ev["root"], ev["name"], ev["split"], ev["targets_filename"]),
                        eval_scores=osp.join(out_dir, "scores_bop19.json"), eval_n_top=ev["n_top"], eval_vsd_delta=ev["vsd_delta"])
            if ev["error_types"] is not None:
                plan.update(eval_error_types=list(ev["error_types"]))
            if ev["symmetric_obj_ids"] is not None:
                plan.update(eval_symmetric_obj_ids=ev["symmetric_obj_ids"])
            if ev["gt_visibility"] is not None:
                plan.update(eval_gt_visibility=ev["gt_visibility"])
            if ev["visib_gt_min"] is not None:
                plan.update(eval_visib_gt_min=ev["visib_gt_min"])
            if ev["gt_delta"] is not None:
                plan.update(eval_gt_delta=ev["gt_delta"])
            if ev["models_info"] is not None:
                plan.update(eval_models_info=ev["models_info"])
        if args.vis is not None:
            plan.update(vis_dir=args.vis or osp.join(out_dir, "vis"))
        print(json.dumps(plan))
        return 0
    if not osp.exists(c.misc.load_from):  # save_unopose.sh:15-18
        print(f"{c.misc.load_from} does not exist.", file=sys.stderr)
        return 1
    if args.num_gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _launch_ranks(args.num_gpus, list(argv if argv is not None else sys.argv[1:]))

    import torch
    import torch.distributed as dist

    from .model import UNOPose
    from .provider import BOPTestsetOneRef, collate_image
    from .runner import ReferenceCache, inference_and_save

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import datetime

        dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(minutes=10))
    torch.set_grad_enabled(False)
    model_cfg = cfg["model"].get("cfg", cfg["model"]) if isinstance(cfg.get("model"), dict) else cfg["model"]
    model = UNOPose(model_cfg)
    if world == 1 or int(os.environ.get("RANK", "0")) == 0:
        load_checkpoint(model, c.misc.load_from)
    model = model.to(dev).eval()
    if world > 1:  # rank 0 read the checkpoint; the weights travel once over RCCL / xGMI (north_star: "RCCL broadcast of DINOv2 weights")
        from .runner import broadcast_module_

        broadcast_module_(model, src=0)
    dcfg = dict(cfg["dataloader"]["test"]["dataset"])
    name, det_path = dcfg.pop("eval_dataset_name"), dcfg.pop("detetion_path", None)
    dataset = BOPTestsetOneRef(dcfg.get("cfg", dcfg), name, det_path, device=dev if args.device_prep else None, device_masks=bool(args.device_masks))

    class Images:  # batch dim 1, like DataLoader(batch_size=1) over the dataset
        dets = getattr(dataset, "dets", None)

        def __len__(self):
            return len(dataset)

        def __getitem__(self, i):
            return collate_image(dataset[i])

    os.makedirs(out_dir, exist_ok=True)
    amp = bool(c.test.amp.enabled)
    pipe = None
    if args.pipeline:
        from .pipeline import PipelinedForward

        pipe = PipelinedForward(model, depth=2 if amp else 1, autocast_dtype=torch.bfloat16 if amp else None)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp and pipe is None):
        lines = inference_and_save(model, Images(), save_path, instance_batch_size=c.test.instance_batch_size, device=dev,
                                   ref_cache=ReferenceCache(model) if args.ref_cache else None, pipeline=pipe)
    if pipe is not None:
        pipe.close()
    if lines is not None:
        print(f"{len(lines)} estimates -> {save_path}")
    if args.eval and int(os.environ.get("RANK", "0")) == 0:  # the other ranks wait at the teardown below
        from .bop_eval import format_error_table, score_csv

        ev = eval_settings(cfg)
        sc = score_csv(save_path, ev["root"], ev["name"], ev["split"], device=dev, device_scoring=not args.eval_device_off, n_top=ev["n_top"],
                       vsd_delta=ev["vsd_delta"], targets_filename=ev["targets_filename"], error_types=ev["error_types"],
                       symmetric_obj_ids=ev["symmetric_obj_ids"], gt_visibility=ev["gt_visibility"] or "off",
                       visib_gt_min=-1 if ev["visib_gt_min"] is None else ev["visib_gt_min"], gt_delta=ev["gt_delta"], models_info=ev["models_info"])
        ar = lambda v: "   n/a" if v is None else "%.4f" % v  # noqa: E731  (AR_VSD and AR need "vsd" among the error types)
        print("BOP19 %s-%s: AR_VSD %s  AR_MSSD %s  AR_MSPD %s  AR %s  (%d targets, %d estimates scored on the %s)"
              % (ev["name"], ev["split"], ar(sc["AR_VSD"]), ar(sc["AR_MSSD"]), ar(sc["AR_MSPD"]), ar(sc["AR"]), sc["n_targets"], sc["n_scored_estimates"],
                 sc["scorer"]))
        for T, blk in sc.get("errors", {}).items():
            if T != "vsd":
                print("%s %s: recalls %s  average recall %.4f" % (T, " ".join("-".join("%g" % v for v in th) for th in blk["thresholds"]),
                                                                  " ".join("%.4f" % v for v in blk["recalls"]), blk["mean_recall"]))
        if "errors" in sc:
            print(format_error_table(sc["errors"]))
    if args.vis is not None and int(os.environ.get("RANK", "0")) == 0:
        from .vis_poses import vis_dataset

        ev = eval_settings(cfg)
        shown = vis_dataset(ev["root"], ev["name"], ev["split"], results=save_path, targets_filename=ev["targets_filename"], n_top=ev["n_top"],
                            out_dir=args.vis or osp.join(out_dir, "vis"), device=dev)
        print(f"{len(shown)} visualisation files -> {args.vis or osp.join(out_dir, 'vis')}")
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
