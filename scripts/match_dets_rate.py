"""Time the proposal-matching kernel (csrc/detmatch.hip, `ops.patch_match_score`) against the same rule written as a composite of torch
operators, and the whole stage of `python -m unopose_amd.match_dets` beside the ViT's share of it.

    kernel   128 proposals x 5 objects, T = 256 patch tokens, D = 768, random unit bf16 rows, once with about half of the patches valid
             on both sides (at random, so no 16-patch tile is empty) and once with all of them valid.  Legs, in one process on identical inputs: the HIP kernel; the composite GEMM -> masked `amax` -> masked mean on
             the bf16 rows (the products leave the GEMM rounded to bf16); the same composite on the rows widened to fp32 (fp32 products,
             as the kernel accumulates).  The composite's GEMM is the `bmm` over the (proposal, object) pairs written as one `mm` of all
             proposal rows against all object rows, which spares it the expanded operand copies; both composites store the
             P x O x T x T matrix.  Every leg is warmed up, the legs alternate
             over the rounds, a round is `--inner` calls between device events; min .. max over the rounds.  Peak device memory of a leg =
             `max_memory_allocated` above what was allocated before it, from a call of its own.
    stage    one 480 x 640 image with 5 objects and 128 proposals written to a temporary BOP folder, a ViT-B/14 at 224 with seeded random
             weights under bf16 autocast: `Matcher.run` on the device route (decode -> crops -> ViT -> unit rows -> scores -> suppression,
             the 5 reference views encoded anew each run, files and reference crops cached), wall clock to a device synchronise, and the
             part of it spent between the events around the ViT calls.
Prints one JSON line and, with --out, writes the lines as text.

    python scripts/match_dets_rate.py [--rounds 7] [--inner 100] [--out profiles/match_dets_rate.txt]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

P, O, T, D = 128, 5, 256, 768
H, W = 480, 640


def write_dataset(root, n_props, rs):
    """One test image (scene 1, image 1) with 5 elliptic objects, one reference image per object (scene 2), the target list and
    `n_props` proposals: the objects' masks shifted and scaled at random."""
    import numpy as np
    from PIL import Image

    from unopose_amd.provider import rle_counts_to_string, rle_encode

    yy, xx = np.mgrid[:H, :W]
    ell = lambda cy, cx, ry, rx: ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0  # noqa: E731
    centres = [(120, 130), (130, 420), (330, 160), (340, 470), (240, 300)]

    def scene(scene_id, images):
        folder = os.path.join(root, "synth", "test", f"{scene_id:06d}")
        cam, gt = {}, {}
        for im_id, objs in images.items():
            depth = np.zeros((H, W), np.uint16)
            for sub in ("rgb", "depth", "mask_visib"):
                os.makedirs(os.path.join(folder, sub), exist_ok=True)
            gts = []
            for j, (obj_id, shape) in enumerate(objs):
                m = ell(*shape)
                depth[m] = 800 + 40 * obj_id
                Image.fromarray((m * 255).astype(np.uint8)).save(os.path.join(folder, "mask_visib", f"{im_id:06d}_{j:06d}.png"))
                gts.append(dict(cam_R_m2c=[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], cam_t_m2c=[0.0, 0.0, 800.0], obj_id=obj_id))
            Image.fromarray(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(os.path.join(folder, "rgb", f"{im_id:06d}.png"))
            Image.fromarray(depth).save(os.path.join(folder, "depth", f"{im_id:06d}.png"))
            cam[str(im_id)] = dict(cam_K=[600.0, 0, 320.0, 0, 600.0, 240.0, 0, 0, 1], depth_scale=1.0)
            gt[str(im_id)] = gts
        json.dump(cam, open(os.path.join(folder, "scene_camera.json"), "w"))
        json.dump(gt, open(os.path.join(folder, "scene_gt.json"), "w"))

    scene(1, {1: [(o + 1, (cy, cx, 70, 90)) for o, (cy, cx) in enumerate(centres)]})
    scene(2, {o + 1: [(o + 1, (240, 320, 150, 190))] for o in range(O)})
    json.dump([dict(scene_id=1, im_id=1, obj_id=o + 1, ref_scene_id=2, ref_im_id=o + 1) for o in range(O)],
              open(os.path.join(root, "synth", "targets.json"), "w"))
    props = []
    for n in range(n_props):
        cy, cx = centres[n % O]
        m = ell(cy + rs.randint(-25, 26), cx + rs.randint(-25, 26), 70 * rs.uniform(0.6, 1.2), 90 * rs.uniform(0.6, 1.2))
        seg = rle_encode(m)
        props.append(dict(scene_id=1, image_id=1, segmentation=dict(size=seg["size"], counts=rle_counts_to_string(seg["counts"]))))
    return props


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import match_dets, ops
    from unopose_amd.model.modules import ViT

    assert torch.cuda.is_available(), "match_dets_rate.py measures on a GPU"
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(P, T, D, generator=g), dim=2).bfloat16().to(dev)
    r = torch.nn.functional.normalize(torch.randn(O, T, D, generator=g), dim=2).bfloat16().to(dev)
    q32, r32 = q.float(), r.float()
    flop = 2.0 * P * O * T * T * D
    lines = [f"patch_match_score: {P} proposals x {O} objects, T = {T}, D = {D}; {args.rounds} rounds of {args.inner} calls between device events, legs "
             f"alternating, after a warm-up of every leg; {flop / 1e9:.1f} GFLOP of products per call when every patch is valid"]
    rec = {}

    def kernel_legs(fraction):
        """The three legs with about `fraction` of the patches valid on both sides (1.0: all)."""
        qv = (torch.rand(P, T, generator=g) < fraction).to(torch.uint8).to(dev)
        rv = (torch.rand(O, T, generator=g) < fraction).to(torch.uint8).to(dev)
        qv[:, 0], rv[:, 0] = 1, 1

        def composite(a, b):
            prod = (a.reshape(P * T, D) @ b.reshape(O * T, D).T).reshape(P, T, O, T)  # the bmm over the pairs as ONE GEMM: no operand copies
            best = prod.masked_fill(~rv.bool()[None, None, :, :], float("-inf")).amax(dim=3).float()  # (P, T, O)
            return (best * qv[:, :, None]).sum(dim=1) / qv.sum(dim=1, dtype=torch.float32)[:, None]

        legs = {"hip kernel": lambda: ops.patch_match_score(q, qv, r, rv),
                "torch composite, bf16 GEMM": lambda: composite(q, r),
                "torch composite, fp32 GEMM": lambda: composite(q32, r32)}
        results = {k: fn() for k, fn in legs.items()}  # warm-up, and the outputs to compare
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        peak = {}
        for k, fn in legs.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
            del out
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():  # the legs alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e-3 / args.inner)
        name = f"valid {fraction:g}"
        lines.append(f" about {100 * fraction:.0f} % of the patches valid on both sides ({int(qv.sum())} of {P * T} proposal patches, {int(rv.sum())} of {O * T} object patches):")
        ref = results["torch composite, fp32 GEMM"].double()
        rec[name] = {}
        for k in legs:
            t = sorted(times[k])
            diff = float((results[k].double() - ref).abs().max())
            rec[name][k] = dict(ms=[round(t[0] * 1e3, 4), round(t[-1] * 1e3, 4)], peak_bytes=int(peak[k]), max_diff_to_fp32_composite=diff)
            lines.append(f"  {k:28s}: {t[0] * 1e3:8.3f} .. {t[-1] * 1e3:8.3f} ms per call (min .. max), peak memory {peak[k] / 2 ** 20:8.2f} MiB above the inputs, "
                         f"largest difference to the fp32 composite {diff:.2e}")
        hip, bf, f32 = (sorted(times[k]) for k in legs)
        lines.append(f"  composite time over kernel time: bf16 GEMM {bf[0] / hip[-1]:.2f} .. {bf[-1] / hip[0]:.2f} (worst .. best pairing of the rounds), "
                     f"fp32 GEMM {f32[0] / hip[-1]:.2f} .. {f32[-1] / hip[0]:.2f}")

    kernel_legs(0.5)
    kernel_legs(1.0)

    # ---- the whole stage
    rs = np.random.RandomState(5)
    with tempfile.TemporaryDirectory() as root:
        props = write_dataset(root, P, rs)
        torch.manual_seed(0)
        vit = ViT(768, 12, 12, 14, 224)
        with torch.no_grad():
            for p in (vit.cls_token, vit.reg_token, vit.pos_embed):
                p.normal_(std=0.02)
        tokens = match_dets.VitTokens(vit, dev, bf16=True)
        tokens.timed = True
        m = match_dets.Matcher(root, "synth", "targets.json", tokens, img_size=224, device=dev, out=io.StringIO())
        walls, shares, kept = [], [], 0
        for run in range(args.rounds + 1):
            m._ref.clear()  # the reference views are encoded again; their host crops and the image files stay cached
            tokens.seconds = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            entries, records = m.run(props)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if run:  # the first run warms up
                walls.append(wall)
                shares.append(tokens.seconds / wall)
            kept, scored = len(entries), len(records[(1, 1)]["slots"])
    rec["stage"] = dict(seconds=[round(min(walls), 4), round(max(walls), 4)], proposals_per_s=[P / max(walls), P / min(walls)],
                        vit_share=[round(min(shares), 3), round(max(shares), 3)], scored=scored, kept=kept)
    lines.append(f"whole stage, one {H} x {W} image, {P} proposals ({scored} scored, {kept} kept) x {O} objects, ViT-B/14 at 224 with random weights, bf16 autocast, "
                 f"{args.rounds} runs after a warm-up: {min(walls):.4f} .. {max(walls):.4f} s per image = {P / max(walls):.0f} .. {P / min(walls):.0f} proposals/s; "
                 f"the ViT calls (133 crops) take {100 * min(shares):.1f} .. {100 * max(shares):.1f} % of it")
    print(json.dumps(rec))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
