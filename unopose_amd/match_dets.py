"""Label and score class-agnostic mask proposals against the one reference view of each targeted object, and write the detection
file `provider.BOPTestsetOneRef` reads as `detetion_path` (`python -m unopose_amd.match_dets`).

The reference ships such a file for YCB-V only and publishes no generator.  Only the file contract is pinned (the keys
`BOPTestsetOneRef.get_instance` reads and `seg_filter_score`); THE SCORING RULE IS THIS PROJECT'S OWN STATEMENT of CNOS / SAM-6D style
descriptor matching, as remembered, unpinned, and no detection accuracy is claimed.  The numpy functions below are the specification and the
`--host` route; `ops.patch_valid`, `ops.token_unit_rows`, `ops.patch_match_score`, `ops.class_cosine` and `ops.mask_nms`
(csrc/detmatch.hip) are the device route.  Everything after the tokens is float64 or integer on the host route.

Per query image (scene, image): its objects are the obj_ids with a key "{scene}_{im}_{obj}" in the one-reference list, its proposals
p = 0 .. P - 1 the entries of the proposal file for it, in file order.
  views     the reference crop and window mask are `provider.ReferenceViews`' (`tem1_rgb`); a proposal's crop is what the provider would
            feed as `rgb` for that detection (mask AND depth > 0, `Window.around`, the same crop chain).  A proposal with
            `minimum_n_point` or fewer pixels left, or a window of side 0, is dropped before any scoring.
  tokens    the last block's final-normed output of the model's own ViT on the crop: row 0 the class token, rows 5 .. the
            (img_size / 14)^2 patch tokens.  Each distinct reference view is encoded once per run.
  validity  pixel (Y, X) of the resized crop reads window pixel (Y s // img_size, X s // img_size) of the s x s window mask; patch (r, c)
            is valid iff 2 x (set pixels among its 14 x 14) >= 196.
  scores    rows divided by their fp32 norm and rounded once to bf16 (a zero norm gives zeros); s_sem = class row . class row;
            s_appe = mean over the valid patches i of p of the max over the valid patches j of o of their products, 0 when either side
            has no valid patch; score = clip((w_sem s_sem + w_appe s_appe) / (w_sem + w_appe), 0, 1).
  label     the arg max of score over the image's objects, a tie to the smaller obj_id; the detection's score is that maximum.
  suppress  per (image, category): by (score descending, proposal index ascending) keep a detection iff no kept one has
            float(inter) > nms_iou * float(union) with it (exact pixel counts of the depth-restricted masks); then the first
            `max_per_object` (0: all)."""
import argparse
import json
import os
import os.path as osp
import sys

import numpy as np
import torch

from .provider import BOPTestsetOneRef, ReferenceViews, SceneFiles, Window, _normalised_crop, load_json, ref_split_folder, rle_decode

PATCH = 14
N_PREFIX = 5  # class token + 4 register tokens before the patch tokens


# ---- the rule, in numpy ---------------------------------------------------------------------------------------------------------------
def patch_valid_host(window_mask, img_size):
    """(s, s) window mask -> ((img_size / 14)^2,) uint8: the patches of the resized crop that lie on the mask."""
    m = np.asarray(window_mask) != 0
    s = m.shape[0]
    if m.ndim != 2 or m.shape != (s, s) or s < 1 or img_size < PATCH or img_size % PATCH:
        raise ValueError(f"patch_valid_host: mask {m.shape}, img_size {img_size}")
    idx = np.arange(img_size, dtype=np.int64) * s // img_size
    side = img_size // PATCH
    cnt = m[np.ix_(idx, idx)].reshape(side, PATCH, side, PATCH).sum(axis=(1, 3), dtype=np.int64)
    return (2 * cnt >= PATCH * PATCH).astype(np.uint8).reshape(-1)


def round_bf16(x):
    """float32 values rounded to bf16 (nearest, ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def unit_rows_host(x):
    """(..., D) tokens -> float64 rows of unit length as the kernels hold them: x / |x| with the norm and the quotient in fp32, rounded
    once to bf16; a zero norm gives zeros."""
    x = np.asarray(x, dtype=np.float32)
    n = np.sqrt(np.sum(x * x, axis=-1, dtype=np.float32, keepdims=True))
    u = np.where(n > 0, x / np.where(n > 0, n, np.float32(1)), np.float32(0)).astype(np.float32)
    return round_bf16(u).astype(np.float64)


def appearance_host(q_unit, q_valid, r_unit, r_valid):
    """s_appe of one (proposal, object) pair: (T, D) unit patch rows and (T,) validities of both."""
    qi, rj = np.flatnonzero(q_valid), np.flatnonzero(r_valid)
    if not len(qi) or not len(rj):
        return 0.0
    return float((q_unit[qi] @ r_unit[rj].T).max(axis=1).mean())


def combine_scores(s_sem, s_appe, weights=(1.0, 1.0)):
    w_sem, w_appe = (float(w) for w in weights)
    return np.clip((w_sem * np.asarray(s_sem, np.float64) + w_appe * np.asarray(s_appe, np.float64)) / (w_sem + w_appe), 0.0, 1.0)


def scores_host(q_tokens, q_valid, r_tokens, r_valid):
    """Tokens (P, 5 + T, D) / (O, 5 + T, D) and validities (P, T) / (O, T) -> (s_sem, s_appe), both (P, O) float64."""
    qu, ru = unit_rows_host(q_tokens), unit_rows_host(r_tokens)
    s_sem = qu[:, 0] @ ru[:, 0].T
    s_appe = np.array([[appearance_host(qu[p, N_PREFIX:], q_valid[p], ru[o, N_PREFIX:], r_valid[o]) for o in range(len(ru))]
                       for p in range(len(qu))], dtype=np.float64).reshape(len(qu), len(ru))
    return s_sem, s_appe


def label_host(score, obj_ids):
    """score (P, O), the objects' ids -> (category_id (P,), its score (P,)): the arg max per row, a tie to the smaller obj_id."""
    obj_ids = np.asarray(obj_ids, dtype=np.int64)
    order = np.argsort(obj_ids, kind="stable")
    best = order[np.argmax(np.asarray(score)[:, order], axis=1)]
    return obj_ids[best], np.asarray(score)[np.arange(len(best)), best]


def nms_host(masks, category, score, nms_iou=0.5, max_per_object=0):
    """`ops.mask_nms` in numpy: -> (keep (N,) uint8, area (N,) int64, inter (N, N) int64)."""
    m = np.asarray(masks).reshape(len(masks), -1) != 0
    N = len(m)
    category, score = np.asarray(category).reshape(N), np.asarray(score, dtype=np.float64).reshape(N)
    area = m.sum(axis=1, dtype=np.int64)
    inter = np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        for j in range(i, N):
            if category[i] == category[j]:
                inter[i, j] = inter[j, i] = np.count_nonzero(m[i] & m[j])
    keep, kept = np.zeros(N, dtype=np.uint8), []
    for i in sorted((i for i in range(N) if score[i] == score[i]), key=lambda i: (-score[i], i)):
        same = [j for j in kept if category[j] == category[i]]
        if any(float(inter[i, j]) > float(nms_iou) * float(area[i] + area[j] - inter[i, j]) for j in same):
            continue
        kept.append(i)
        keep[i] = max_per_object == 0 or len(same) < max_per_object
    return keep, area, inter


# ---- tokens ---------------------------------------------------------------------------------------------------------------------------
class VitTokens:
    """crops (B, 3, S, S) float32 (host or device) -> the last block's final-normed tokens (B, 5 + T, D) on the device, through the
    model's own `ViT.forward` (bf16 autocast, or fp32), `chunk` crops at a time."""

    def __init__(self, vit, device, bf16=True, chunk=64):
        self.vit, self.device, self.bf16, self.chunk = vit.to(device).eval(), torch.device(device), bool(bf16), int(chunk)
        self.seconds = 0.0  # device time spent here, when `timed` (events)
        self.timed = False

    def __call__(self, crops):
        crops = crops.to(self.device, torch.float32).contiguous()
        outs = []
        if self.timed:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
        with torch.no_grad():
            for b in range(0, len(crops), self.chunk):
                x = crops[b:b + self.chunk]
                if self.bf16:
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        outs.append(self.vit(x)[-1])
                else:
                    outs.append(self.vit(x)[-1])
        if self.timed:
            t1.record()
            t1.synchronize()
            self.seconds += t0.elapsed_time(t1) * 1e-3
        return torch.cat(outs, 0) if len(outs) > 1 else outs[0]


def _tokens_numpy(t):
    return t.detach().to(torch.float32).cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float32)


# ---- one run --------------------------------------------------------------------------------------------------------------------------
class Matcher:
    """The rule over a dataset.  `tokens_fn`: crops (B, 3, S, S) float32 tensor -> tokens (B, 5 + T, D) (tensor or array); `device`:
    a CUDA device selects the device route, None the host route (numpy after the tokens)."""

    def __init__(self, data_dir, dataset, ref_targets_name, tokens_fn, split="test", img_size=224, rgb_mask_flag=True, rgb_to_bgr=False,
                 min_points=8, weights=(1.0, 1.0), nms_iou=0.5, max_per_object=0, device=None, suppress=True, out=None):
        check_rule_arguments(img_size, weights, nms_iou, max_per_object, min_points)
        self.data_dir, self.dataset, self.img_size = data_dir, dataset, int(img_size)
        self.folder = osp.join(data_dir, dataset, split)
        self.rgb_mask_flag, self.bgr, self.min_points = bool(rgb_mask_flag), bool(rgb_to_bgr), int(min_points)
        self.weights, self.nms_iou, self.max_per_object, self.suppress = tuple(float(w) for w in weights), float(nms_iou), int(max_per_object), suppress
        self.tokens_fn, self.out = tokens_fn, sys.stdout if out is None else out
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("match_dets: the device route on CPU is not supported (leave `device` unset for the host route)")
        self.files = SceneFiles()
        self.views = ReferenceViews(self.files, self.img_size, self.rgb_mask_flag, self.bgr, max_views=1 << 30)
        self.objects = {}  # (scene, image) -> {obj_id: (ref scene, ref image)}
        for key, ref in BOPTestsetOneRef.load_ref(osp.join(data_dir, dataset, ref_targets_name)).items():
            s, i, o = (int(v) for v in key.split("_"))
            self.objects.setdefault((s, i), {})[o] = tuple(int(v) for v in ref.split("_"))
        self._ref = {}  # (folder, scene, image, object) -> (unit class row, unit patch rows, validity) or None; encoded once per run
        self.counts = dict(images=0, skipped_images=0, skipped_targets=0, proposals=0, dropped=0, scored=0, kept=0, references=0)

    # -- reference side
    def _references(self, scene_id, im_id):
        """-> (obj_ids, class rows (O, D), patch rows (O, T, D), validity (O, T)) of the image's objects with a reference view."""
        todo, keys = [], {}
        for obj_id, (rs, ri) in sorted(self.objects[(scene_id, im_id)].items()):
            key = keys[obj_id] = (ref_split_folder(self.data_dir, self.dataset, rs, self.folder), rs, ri, obj_id)
            if key not in self._ref:
                view = self.views.get(*key)
                if view is None:
                    self._ref[key] = None
                    continue
                inside = np.zeros(view["window"].side ** 2, dtype=np.uint8)
                inside[view["pixels"]] = 1
                todo.append((key, view["crop"], patch_valid_host(inside.reshape(view["window"].side, -1), self.img_size)))
        if todo:
            cls, patches = self._unit(self.tokens_fn(torch.stack([c for _, c, _ in todo])))
            for n, (key, _, valid) in enumerate(todo):
                self._ref[key] = (cls[n], patches[n], torch.from_numpy(valid).to(self.device) if self.device is not None else valid)
            self.counts["references"] += len(todo)
        obj_ids = []
        for obj_id, key in keys.items():
            if self._ref[key] is None:
                self.counts["skipped_targets"] += 1
                print(f"scene {scene_id} image {im_id} object {obj_id}: no reference view in scene {key[1]} image {key[2]}, target skipped", file=self.out)
            else:
                obj_ids.append(obj_id)
        if not obj_ids:
            return [], None, None, None
        stack = torch.stack if self.device is not None else np.stack
        return (obj_ids,) + tuple(stack([self._ref[keys[o]][k] for o in obj_ids]) for k in range(3))

    def _unit(self, tokens):
        """tokens (B, 5 + T, D) -> (unit class rows (B, D), unit patch rows (B, T, D)) on the route's side."""
        if self.device is None:
            u = unit_rows_host(_tokens_numpy(tokens))
            return u[:, 0], u[:, N_PREFIX:]
        from . import ops

        u = ops.token_unit_rows(tokens.to(self.device).contiguous())
        return u[:, 0].contiguous(), u[:, N_PREFIX:].contiguous()

    # -- query side
    def _views_host(self, props, depth, colour):
        """-> (surviving proposal numbers, crops tensor, validity (P, T), depth-restricted masks (P, H, W))."""
        slots, crops, valid, masks = [], [], [], []
        for p, prop in enumerate(props):
            m = np.logical_and(rle_decode(prop["segmentation"]) > 0, depth > 0)
            if not np.sum(m) > self.min_points:
                continue
            win = Window.around(m)
            if win.side < 1:
                continue
            inside = win.crop(m)
            slots.append(p)
            crops.append(_normalised_crop(colour, win, self.img_size, inside if self.rgb_mask_flag else None, self.bgr))
            valid.append(patch_valid_host(inside, self.img_size))
            masks.append(m)
        if not slots:
            return slots, None, None, None
        return slots, torch.stack(crops), np.stack(valid), np.stack(masks)

    def _views_device(self, props, depth, colour):
        from . import ops

        depth_dev = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float64)).to(self.device)
        masks, _, stats = ops.rle_decode([p["segmentation"] for p in props], self.device, depth_dev, with_host_stats=True)
        if tuple(masks.shape[1:]) != depth.shape:
            raise ValueError(f"match_dets: segmentation size {tuple(masks.shape[1:])} for a {depth.shape} image")
        slots, wins = [], []
        for p in range(len(props)):
            n, top, bottom, left, right = (int(v) for v in stats[p, :5])
            if not n > self.min_points:
                continue
            win = Window.from_extents(depth.shape, top, bottom, left, right)
            if win.side < 1:
                continue
            slots.append(p)
            wins.append(win)
        if not slots:
            return slots, None, None, None
        packed, row_counts = ops.window_masks(masks, wins, slots)
        plan = ops.PrepPlan.from_device(depth.shape, wins, packed, row_counts, self.img_size, self.device)
        crops = ops.prep_crop_resize(torch.from_numpy(np.ascontiguousarray(colour)).to(self.device), plan, bgr=self.bgr, use_mask=self.rgb_mask_flag)
        valid = ops.patch_valid(packed, wins, self.img_size)
        return slots, crops, valid, masks[torch.as_tensor(slots, device=self.device)].contiguous()

    def image(self, scene_id, im_id, props):
        """The rule for one image -> a record dict (proposal numbers, objects, s_sem, s_appe, score, category, best, keep), or None when
        the image was skipped."""
        if self.device is not None:
            from . import ops
        c = self.counts
        c["images"] += 1
        c["proposals"] += len(props)
        if (scene_id, im_id) not in self.objects:
            c["skipped_images"] += 1
            print(f"scene {scene_id} image {im_id}: {len(props)} proposals, no targeted object, image skipped", file=self.out)
            return None
        obj_ids, r_cls, r_patch, r_valid = self._references(scene_id, im_id)
        if not obj_ids:
            c["skipped_images"] += 1
            print(f"scene {scene_id} image {im_id}: {len(props)} proposals, no reference view for any target, image skipped", file=self.out)
            return None
        K, depth_scale = self.files.camera(self.folder, scene_id, im_id)
        depth = self.files.depth_m(self.folder, scene_id, im_id, depth_scale)
        colour = self.files.colour(self.folder, scene_id, im_id)
        slots, crops, valid, masks = (self._views_host if self.device is None else self._views_device)(props, depth, colour)
        c["dropped"] += len(props) - len(slots)
        if not slots:
            return dict(slots=[], obj_ids=obj_ids, keep=np.zeros(0, np.uint8))
        q_cls, q_patch = self._unit(self.tokens_fn(crops))
        if self.device is None:
            s_sem = q_cls @ r_cls.T
            s_appe = np.array([[appearance_host(q_patch[p], valid[p], r_patch[o], r_valid[o]) for o in range(len(obj_ids))]
                               for p in range(len(slots))], dtype=np.float64)
        else:
            s_sem = ops.class_cosine(q_cls, r_cls).double().cpu().numpy()
            s_appe = ops.patch_match_score(q_patch, valid, r_patch, r_valid).double().cpu().numpy()
        score = combine_scores(s_sem, s_appe, self.weights)
        category, best = label_host(score, obj_ids)
        if not self.suppress:
            keep = np.ones(len(slots), dtype=np.uint8)
        elif self.device is None:
            keep = nms_host(masks, category, best, self.nms_iou, self.max_per_object)[0]
        else:
            keep = ops.mask_nms(masks, torch.from_numpy(category.astype(np.int32)).to(self.device), torch.from_numpy(best).to(self.device),
                                self.nms_iou, self.max_per_object)[0].cpu().numpy()
        c["scored"] += len(slots)
        c["kept"] += int(keep.sum())
        return dict(slots=slots, obj_ids=obj_ids, s_sem=s_sem, s_appe=s_appe, score=score, category=category, best=best, keep=keep)

    def run(self, proposals):
        """proposals: the proposal file's list -> (detection entries sorted by (scene, image, proposal number), {(scene, image): record})."""
        by_image = {}
        for prop in proposals:
            by_image.setdefault((int(prop["scene_id"]), int(prop["image_id"])), []).append(prop)
        entries, records = [], {}
        for (scene_id, im_id), props in sorted(by_image.items()):
            rec = self.image(scene_id, im_id, props)
            if rec is None:
                continue
            records[(scene_id, im_id)] = rec
            for n, p in enumerate(rec["slots"]):
                if rec["keep"][n]:
                    prop = props[p]
                    entries.append(dict(scene_id=scene_id, image_id=im_id, category_id=int(rec["category"][n]), score=float(rec["best"][n]),
                                        bbox=prop["bbox"] if prop.get("bbox") is not None else _mask_xywh(prop["segmentation"]),
                                        time=prop.get("time", -1), segmentation=prop["segmentation"]))
        return entries, records

    def summary(self):
        c = self.counts
        return (f"{c['images']} images ({c['skipped_images']} skipped), {c['proposals']} proposals: {c['dropped']} dropped before scoring, "
                f"{c['scored']} scored, {c['kept']} kept; {c['references']} reference views encoded, {c['skipped_targets']} targets without one")


def _mask_xywh(seg):
    ys, xs = np.nonzero(rle_decode(seg))
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()) + 1, int(ys.max() - ys.min()) + 1]


def check_rule_arguments(img_size, weights, nms_iou, max_per_object, min_points):
    if int(img_size) < PATCH or int(img_size) % PATCH:
        raise ValueError(f"match_dets: img_size {img_size} is not a positive multiple of {PATCH}")
    w = [float(v) for v in weights]
    if len(w) != 2 or not all(np.isfinite(w)) or min(w) < 0 or sum(w) <= 0:
        raise ValueError(f"match_dets: weights {tuple(weights)}: two numbers >= 0 that do not both vanish")
    if not 0.0 <= float(nms_iou) <= 1.0:
        raise ValueError(f"match_dets: nms_iou {nms_iou} outside [0, 1]")
    if int(max_per_object) < 0 or int(min_points) < 0:
        raise ValueError(f"match_dets: max_per_object {max_per_object} and min_points {min_points} must not be negative")


def save_detections(path, entries):
    """One entry per line, under a temporary name first."""
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w") as f:
        f.write("[\n" + ",\n".join("  " + json.dumps(e) for e in entries) + "\n]")
    os.replace(tmp, path)


def check_detections(matcher, dets, out=None):
    """`--check`: the entries of an existing detection file as proposals, without suppression -> the number labelled differently.
    Prints per object (the file's category_id) the entries, those dropped or skipped by the rule, those the rule labels differently and
    the largest score difference."""
    out = sys.stdout if out is None else out
    matcher.suppress = False
    by_image = {}
    for d in dets:
        by_image.setdefault((int(d["scene_id"]), int(d["image_id"])), []).append(d)
    per = {}
    for (scene_id, im_id), props in sorted(by_image.items()):
        rec = matcher.image(scene_id, im_id, props)
        seen = {} if rec is None else {p: n for n, p in enumerate(rec["slots"])}
        for p, d in enumerate(props):
            row = per.setdefault(int(d["category_id"]), dict(n=0, unscored=0, differ=0, diff=0.0))
            row["n"] += 1
            if p not in seen:
                row["unscored"] += 1
                continue
            n = seen[p]
            row["differ"] += int(rec["category"][n]) != int(d["category_id"])
            row["diff"] = max(row["diff"], abs(float(rec["best"][n]) - float(d["score"])))
    for obj_id, row in sorted(per.items()):
        print(f"object {obj_id}: {row['n']} entries, {row['unscored']} not scored, {row['differ']} labelled differently, largest score difference {row['diff']:.6f}",
              file=out)
    total = sum(r["differ"] for r in per.values())
    print(f"total: {sum(r['n'] for r in per.values())} entries, {total} labelled differently; {matcher.summary()}", file=out)
    return total


def load_vit(checkpoint, vit_ckpt, img_size):
    """The frozen DINOv2 of a UNOPose checkpoint, or of a timm checkpoint ({"model": state_dict})."""
    from .model import UNOPose, default_model_cfg

    cfg = default_model_cfg(feature_extraction=dict(img_size=int(img_size)))
    if checkpoint is not None:
        from .cli import load_checkpoint

        return load_checkpoint(UNOPose(cfg), checkpoint).feature_extraction.rgb_net.vit
    from .model.modules import ViT_AE

    net = ViT_AE(cfg.feature_extraction)
    net.load_dinov2(vit_ckpt)
    return net.vit


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.match_dets", description="Write the detection file of a one-reference test run "
                                 "(dataloader.test.dataset.detetion_path) from class-agnostic mask proposals: each proposal is labelled and scored "
                                 "against the reference view of every targeted object of its image by DINOv2 class- and patch-token cosines, then "
                                 "suppressed per object by mask IoU.  The rule is this project's own (unpinned); --check compares an existing file.")
    ap.add_argument("--data-dir", required=True, help="the folder that holds the dataset folder")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--proposals", default=None, help="json list of {scene_id, image_id, segmentation (COCO RLE), [bbox], [time]}")
    ap.add_argument("--out", default=None, help="the detection file to write")
    ap.add_argument("--split", default="test")
    ap.add_argument("--ref-targets", default="test_ref_targets_crossscene_rot50.json", help="the one-reference list inside the dataset folder")
    ap.add_argument("--checkpoint", default=None, help="a UNOPose checkpoint: its ViT is used")
    ap.add_argument("--vit-ckpt", default=None, help="a timm DINOv2 checkpoint ({'model': state_dict})")
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--fp32", action="store_true", help="run the ViT without autocast (default: bf16 autocast)")
    ap.add_argument("--weights", type=float, nargs=2, default=(1.0, 1.0), metavar=("SEM", "APPE"))
    ap.add_argument("--nms-iou", type=float, default=0.5)
    ap.add_argument("--max-per-object", type=int, default=0, help="detections kept per (image, object); 0: all")
    ap.add_argument("--min-points", type=int, default=8, help="the provider's minimum_n_point: a proposal with this many valid pixels or fewer is dropped")
    ap.add_argument("--no-rgb-mask", action="store_true", help="crops are not masked (rgb_mask_flag off in the run's config)")
    ap.add_argument("--bgr", action="store_true", help="rgb_to_bgr of the run's config")
    ap.add_argument("--host", action="store_true", help="numpy after the tokens instead of the kernels: same rule, for comparison")
    ap.add_argument("--check", metavar="FILE", default=None, help="write nothing: report per object how many entries of FILE the rule labels differently")
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args(argv)
    # every argument error before any GPU work
    if (args.checkpoint is None) == (args.vit_ckpt is None):
        ap.error("exactly one of --checkpoint and --vit-ckpt is needed")
    if args.check is None and (args.proposals is None or args.out is None):
        ap.error("--proposals and --out are needed (or --check FILE)")
    try:
        check_rule_arguments(args.img_size, args.weights, args.nms_iou, args.max_per_object, args.min_points)
    except ValueError as e:
        ap.error(str(e))
    source = args.check if args.check is not None else args.proposals
    for path in (source, args.checkpoint or args.vit_ckpt, osp.join(args.data_dir, args.dataset, args.ref_targets), osp.join(args.data_dir, args.dataset, args.split)):
        if not osp.exists(path):
            raise FileNotFoundError(f"match_dets: {path} does not exist")
    if args.check is None and osp.exists(args.out) and not args.overwrite:
        raise FileExistsError(f"match_dets: {args.out} exists; pass --overwrite to replace")
    proposals = load_json(source)
    if not isinstance(proposals, list) or not all(isinstance(p, dict) and {"scene_id", "image_id", "segmentation"} <= set(p) for p in proposals):
        raise ValueError(f"match_dets: {source} is not a list of entries with scene_id, image_id and segmentation")
    if not torch.cuda.is_available():
        raise RuntimeError("match_dets: no GPU: the ViT has no CPU path (--host only moves the scoring after the tokens to numpy)")
    from ._lib import lib

    lib()  # a missing library raises here
    device = torch.device("cuda", torch.cuda.current_device())
    tokens = VitTokens(load_vit(args.checkpoint, args.vit_ckpt, args.img_size), device, bf16=not args.fp32)
    matcher = Matcher(args.data_dir, args.dataset, args.ref_targets, tokens, split=args.split, img_size=args.img_size, rgb_mask_flag=not args.no_rgb_mask,
                      rgb_to_bgr=args.bgr, min_points=args.min_points, weights=args.weights, nms_iou=args.nms_iou, max_per_object=args.max_per_object,
                      device=None if args.host else device)
    if args.check is not None:
        check_detections(matcher, proposals)
        return 0
    entries, _ = matcher.run(proposals)
    save_detections(args.out, entries)
    print(matcher.summary())
    print(f"{len(entries)} detections -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
