"""Training pairs without a dataset: (query, reference) pairs of one object rendered under two known poses from a folder of
`obj_XXXXXX.ply` models, turned into the item dict of `provider_train.MegaPoseOneRefTrainSet` and handed out as batches
(`OnlinePairs`; `python -m unopose_amd.fit --online-models DIR`).  No files, no loader workers: a batch is a pure function of
(seed, rank, iteration).

Four parts.

1. `draw_recipe(seed, rank, iteration, candidates, models, cfg, chunk=0)` draws everything random for `candidates` pairs from a private
   `np.random.Generator` over Philox, key = (seed, rank << 44 | iteration), counter word 3 = chunk; the global `np.random` is never touched.
   Per pair, in this order: the object (integers); the reference rotation (4 normals -> unit quaternion) and its fill fraction (uniform);
   the query rotation, fill fraction and centre offset (2 uniforms in [-1, 1]); the occluder coin (uniform), model (integers), rotation,
   lateral direction and reach (2 uniforms), depth fraction (uniform); the dilation coin (uniform); the three spin angles (`random(3) * 2 pi`:
   `provider_train.random_rotation_xyz`'s formula, `rotation_xyz`); the shift (`uniform(-shift_range, shift_range, 3)`); the (n_obs, 3)
   standard-normal noise field; two 64-bit draw keys.  Every draw happens whatever the coins say, so pair k's values do not depend on
   pair k - 1's coins.
   Pose rule (model units, camera looking down +z, x right, y down; K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]): rotations are uniform;
   a view's depth z = f * diameter / (fill * min(H, W)), so that the projected diameter covers `fill` of the canvas's shorter side; the
   reference's model centre sits on the optical axis and it has no occluder, so it is whole and unoccluded (what MegaPose's candidate
   lists guarantee with visibility >= 0.8); the query's centre projects to (W / 2 + ox * offset * W / 2, H / 2 + oy * offset * H / 2);
   the occluder (with probability `occluder_prob`, another model where there is one) sits at depth max(frac * z, its diameter),
   frac in [0.45, 0.75], on the ray to a point beside the query's centre: in a uniform direction, 0.4 to 1.0 times the mean of the two
   diameters away (at 1.0 the two bounding spheres would touch at equal depth; nearer to the camera the occluder looks larger and overlaps).
   Keys under `dataloader.train.online.*` and their defaults: `canvas` [H, W] = [240, 320]; `focal` = 300.0; `fill` = [0.35, 0.8];
   `offset` = 0.6; `occluder_prob` = 0.5; `ssaa` = 2; `shading` = "phong"; `ambient` = 0.5; `max_chunks` = 8; `scene` = None (part 4).

2. `items_from_views_host(views, recipe, cfg)` is the item rule, `MegaPoseOneRefTrainSet.read_data` / `reference_view` restated on rendered
   canvases (colour (H, W, 3) uint8 and depth (H, W) float32 in model units of the reference, the query and the query's occluder, 0 =
   nothing), in numpy, on `provider.Window.from_extents`, `lift_depth`, `Window.to_resized`, `provider_train.dilate_cross` and
   `_normalised_crop`'s steps (`finish_item`).  It does not render.  Where the provider leaves an order to numpy this rule fixes one, and csrc/train_items.hip
   follows the same:
   * depth to metres: `depth.astype(np.float64) * 0.001` (models are in millimetres, as BOP's);
   * reference: mask = depth > 0; window around it; the set window pixels in row-major order; `draw_index(key0, i, n, n_tpl)` for
     i < n_tpl picks among them; `tem1_choose` = `to_resized` of the picks, points = `lift_depth` at the picks (float64); mean = the sum
     of the drawn points in draw order / n_tpl; radius = max sqrt((dx dx + dy dy) + dz dz);
   * query: visible = object depth > 0 and (occluder depth == 0 there or object depth <= occluder depth); scene depth / colour = the
     object's where visible, else the occluder's where it has depth, else 0; invalid when visible < `min_px_count_visib` or visible / full
     < `min_visib_fract` (float64); the dilation (coin and `dilate_mask`) is `dilate_cross(visible, 4)`; window around the final mask, its
     set pixels in row-major order, the lift of the SCENE depth; mean = (each window row's points added left to right, the row sums added
     top to bottom) / n; keep = sqrt((dx dx + dy dy) + dz dz) < 1.2 * radius; invalid below 32 kept; `draw_index(key1, i, n_kept, n_obs)`;
   * labels and augmentation: rel = T_q T_r^-1 with T^-1 = [R^T | -R^T t], translations in metres (t * 0.001), all float64;
     `tem1_pts` = points @ spin with every element (p0 S0k + p1 S1k) + p2 S2k; target = rel @ spin (4 x 4, float64); `rotation_label` =
     float32(target[:3, :3]), `translation_label` = float32(target[:3, 3] + shift); `pts` = float32(points + (shift + 0.001 * noise)).
   `draw_index(key, i, n_have, n_want)` is a pure integer function, here in numpy and in csrc/train_items.hip: for n_have > n_want a keyed
   bijection of [0, n_have) (a 6-round balanced Feistel network on the next even number of bits, walked until it lands inside), so the
   draw is without repetition; else a keyed hash modulo n_have -- the provider's `replace = n_have <= n_want`.

3. `OnlinePairs(models, cfg, device, seed, rank=0, world=1, host=False)`: `batch(iteration)` -> the dict `collate_pairs` returns, on the
   device.  Candidates come in chunks of the batch size (chunk c of an iteration = `draw_recipe(..., chunk=c)`); a batch is the first B
   valid candidates of its iteration in candidate order; after `max_chunks` chunks without B valid pairs it raises.  Views are rendered
   grouped by object (`render.HipShadedRenderer` / `HipDepthRenderer`, models read once through `bop_eval.read_ply_model`).  Per chunk two
   small tables come back to the host: the view table (counts and extents per view: the windows and the visibility rule need them) and,
   after the points, the kept counts with the set pixels per window row (the batch choice and `finish_crops`' plan need them); no
   per-pixel or per-point data does.  The colour augmentation is `ColorAugmentor.plan` on a Philox generator of the iteration's own
   (chunk number `AUG_CHUNK`), per taken pair the query's 0.8 coin and plan, then the reference's; `ops.finish_crops` applies it.
   `host=True` reads the renders back and runs `items_from_views_host` and `ColorAugmentor.apply`: the same batch, tensor for tensor.
   Iterating from `start` prepares batch i + 1 on a side stream (`pipeline._pool_streams`) while step i runs, and hands a batch over with an
   event and `record_stream`.

4. The scene stage, `dataloader.train.online.scene` (default None: absent, no launch, no draw, the batches above bit for bit; a dict, `{}`
   included, turns it on): a textured background plane behind the query and a depth-sensor model on both views, between the renders and the
   item rule.  Without it the rim of a dilated mask has depth 0 and lifts to the camera centre, which pulls the centroid towards the camera
   by (rim share) x z and moves the keep sphere with it; MegaPose's images have the depth of whatever stands behind the object there.
   `draw_scene` draws per candidate, from a generator of its own (chunk `SCENE_CHUNK0 + chunk`, so the recipe is the same with the stage on or
   off): two view keys, the plane (unit normal n = (0, 0, -1) tilted by up to `plane_tilt` degrees about an in-image axis; point p0 on the ray
   through the query's model centre at depth z_q + (0.5 + g) diameter, g uniform in `plane_gap`; two in-plane axes; a texture key).
   `sense_views_host(depth, rgb, desc)` is the pixel rule, one descriptor row per view (`scene_rows`), float64 on metres with + - x / floor
   rint and comparisons only, every stage reading the INPUT canvas, so no pixel waits for another's output; csrc/scene.hip equals it bit for
   bit.  Random numbers are `_scene_hash(key, stream, index)` = mix(key ^ mix((stream << 40 | index) + gold)); probabilities are integer
   thresholds on the hash's upper 32 bits.
   * (a) background (a query with a plane, where the view has no depth): r = ((x - cx) / f, (y - cy) / f, 1), nr = (n0 rx + n1 ry) + n2,
     z = (n . p0) / nr; nothing where nr >= 0 or z is outside (0, 10 m].  Colour: plane coordinates s, t = ((z r - p0) . u, v) / cell with
     cell = `texture_cell` diameters; three octaves (s, t times 1, 2, 4; weights 0.5, 0.3, 0.2, added in that order) of value noise, the
     lattice byte of channel c = byte c of hash(texture key, 3 + octave, (iu & 0xFFFFF) << 20 | iv & 0xFFFFF), blended
     (b00 + (b10 - b00) fu, b01 + (b11 - b01) fu, then top + (bottom - top) fv); floor(x + 0.5).
   * (b) drop-outs, decided on the noise-free depth after (a), for pixels with depth: the hole of cell (y // hole_cell, x // hole_cell)
     (stream 0, index = the cell's row-major number, `hole_prob`); an edge pixel -- a 4-neighbour inside the canvas without depth or with
     |z - z_n| > `edge_thres` z -- drops with `edge_drop` (stream 1, pixel number).  A dropped pixel gets depth 0 and keeps its colour.
   * (c) on the others, when the noise or the quantisation is on: z <- z + (a + b (z - z0)^2) g with g = (the sum of the four 16-bit fields
     of hash(key, 2, pixel) - 131070) sqrt(3) / 65536 (Irwin-Hall, unit variance, |g| <= 2 sqrt 3); no return (depth 0) if z <= 0; then with
     `disparity_steps` s > 0 and fb = focal x `baseline_m`: k = rint((s fb) / z), no return if k < 1, z <- fb / (k / s); float32(z * 1000.0).
   A pixel no stage touches keeps its input bits.  The references are sensed by (b), (c) before the item rule reads their depth; the
   queries by (a), (b), (c) on the composed scene depth and colour, after the mask and the table are taken from the renders.
   Keys under `online.scene.*`: `background` = "plane" (or "none"), `plane_gap` = [0.0, 1.5], `plane_tilt` = 35.0, `texture_cell` = 0.25,
   `noise` = [0.0012, 0.0019, 0.4] (a, b, z0 of the Kinect axial model of Nguyen et al. 2012 as remembered: NOT pinned to the paper),
   `baseline_m` = 0.075, `disparity_steps` = 8 (0: no quantisation), `edge_thres` = 0.03, `edge_drop` = 0.5, `hole_prob` = 0.01,
   `hole_cell` = 6.  One occluder at most and no lateral or colour noise remain."""
import os
import os.path as osp

import numpy as np
import torch

from .provider import Window, lift_depth, resize_bilinear_u8, to_tensor_normalize
from .provider_train import AugPlan, ColorAugmentor, dilate_cross, pack_plans

DEPTH_TO_M = 0.001
MIN_KEPT = 32
AUG_CHUNK = 2 ** 32 - 1
SCENE_CHUNK0 = 2 ** 32  # the scene draw of recipe chunk c uses generator chunk SCENE_CHUNK0 + c: above every recipe chunk and AUG_CHUNK
ONLINE_DEFAULTS = dict(canvas=(240, 320), focal=300.0, fill=(0.35, 0.8), offset=0.6, occluder_prob=0.5, ssaa=2, shading="phong", ambient=0.5,
                       max_chunks=8, scene=None)
# `noise`: sigma(z) = a + b (z - z0)^2 in metres, the shape of the Kinect axial model of Nguyen et al. 2012; the three constants are written
# from memory and NOT pinned to the paper.
SCENE_DEFAULTS = dict(background="plane", plane_gap=(0.0, 1.5), plane_tilt=35.0, texture_cell=0.25, noise=(0.0012, 0.0019, 0.4), baseline_m=0.075,
                      disparity_steps=8, edge_thres=0.03, edge_drop=0.5, hole_prob=0.01, hole_cell=6)
SCENE_DESC = 32  # 64-bit words per view descriptor (`scene_rows`)
SCENE_Z_MAX_M = 10.0  # a background farther than this stays empty
SCENE_OCTAVE_WEIGHTS = (0.5, 0.3, 0.2)
SCENE_STREAM_HOLE, SCENE_STREAM_EDGE, SCENE_STREAM_NOISE, SCENE_STREAM_TEXTURE = 0, 1, 2, 3  # texture octave o: stream 3 + o
SCENE_G_SCALE = 1.7320508075688772 / 65536.0  # sqrt(3) / 2^16: the sum of four 16-bit fields, centred, has variance (2^32 - 1) / 3
_M64 = (1 << 64) - 1
_GOLD_INT = 0x9E3779B97F4A7C15
_GOLD = np.uint64(_GOLD_INT)
_ROUNDS = 6


def _get(cfg, key, *default):
    return cfg.get(key, *default) if hasattr(cfg, "get") else getattr(cfg, key, *default)


def online_cfg(cfg):
    """The `online.*` keys of a dataset cfg with the defaults filled in."""
    given = _get(cfg, "online", None) or {}
    out = dict(ONLINE_DEFAULTS)
    unknown = sorted(set(given) - set(out) - {"models", "obj_ids"})
    if unknown:
        raise ValueError(f"dataloader.train.online: unknown keys {unknown}")
    out.update({k: given[k] for k in given})
    H, W = (int(v) for v in out["canvas"])
    lo, hi = (float(v) for v in out["fill"])
    if H < 2 or W < 2 or not 0 < lo <= hi <= 1 or not 0 <= float(out["offset"]) <= 1 or not 0 <= float(out["occluder_prob"]) <= 1:
        raise ValueError(f"dataloader.train.online: canvas {out['canvas']}, fill {out['fill']}, offset {out['offset']}, occluder_prob {out['occluder_prob']}")
    out["canvas"], out["fill"] = (H, W), (lo, hi)
    out["scene"] = scene_cfg(out["scene"])
    return out


def scene_cfg(given):
    """The `online.scene.*` keys with the defaults filled in; None (the stage is absent) stays None."""
    if given is None:
        return None
    out = dict(SCENE_DEFAULTS)
    unknown = sorted(set(given) - set(out))
    if unknown:
        raise ValueError(f"dataloader.train.online.scene: unknown keys {unknown}")
    out.update({k: given[k] for k in given})
    gap, noise = tuple(float(v) for v in out["plane_gap"]), tuple(float(v) for v in out["noise"])
    steps, cell = int(out["disparity_steps"]), int(out["hole_cell"])
    if (out["background"] not in ("plane", "none") or len(gap) != 2 or not 0 <= gap[0] <= gap[1] or not 0 <= float(out["plane_tilt"]) < 90
            or not float(out["texture_cell"]) > 0 or len(noise) != 3 or min(noise[:2]) < 0 or not float(out["baseline_m"]) > 0
            or steps != out["disparity_steps"] or not 0 <= steps < 2 ** 20 or float(out["edge_thres"]) < 0 or not 0 <= float(out["edge_drop"]) <= 1
            or not 0 <= float(out["hole_prob"]) <= 1 or cell != out["hole_cell"] or cell < 1):
        raise ValueError(f"dataloader.train.online.scene: {out}")
    out.update(plane_gap=gap, noise=noise, disparity_steps=steps, hole_cell=cell)
    return out


def camera_matrix(oc):
    H, W = oc["canvas"]
    f = float(oc["focal"])
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def _mix(z):
    """splitmix64's finaliser on uint64 arrays (wrap-around arithmetic)."""
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_index(key, i, n_have, n_want):
    """Sample i of a keyed draw of n_want out of n_have -> an index in [0, n_have) (int64; `i` a scalar or an array of numbers in [0, n_want)).
    Without repetition over i exactly when n_have > n_want; no state between the i."""
    n_have, n_want = int(n_have), int(n_want)
    if not 1 <= n_have < 2 ** 31:
        raise ValueError(f"draw_index: n_have {n_have}")
    key_int = int(key) & _M64
    key = np.uint64(key_int)
    x = np.atleast_1d(np.asarray(i)).astype(np.uint64)
    if n_have > n_want:
        k = 1
        while (1 << (2 * k)) < n_have:
            k += 1
        k64, mask = np.uint64(k), np.uint64((1 << k) - 1)
        x = x.copy()
        todo = np.ones(x.shape, dtype=bool)
        while todo.any():
            L, R = x[todo] >> k64, x[todo] & mask
            for r in range(_ROUNDS):
                L, R = R, L ^ (_mix(np.uint64((key_int + _GOLD_INT * (r + 1)) & _M64) + R) & mask)  # key + gold (r + 1) + R mod 2^64
            x[todo] = (L << k64) | R
            todo = x >= np.uint64(n_have)
        out = x
    else:
        out = _mix(key ^ _mix(x + _GOLD)) % np.uint64(n_have)
    out = out.astype(np.int64)
    return out if np.ndim(i) else int(out[0])


# ---- the recipe ----------------------------------------------------------------------------------------------------------------------
def rotation_xyz(a):
    """`provider_train.random_rotation_xyz` for given angles: Rx(a0) Ry(a1) Rz(a2), float64."""
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    return rx @ ry @ rz


def _uniform_rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def recipe_generator(seed, rank, iteration, chunk=0):
    """The private generator of (seed, rank, iteration, chunk)."""
    if not (0 <= int(rank) < 2 ** 20 and 0 <= int(iteration) < 2 ** 44 and 0 <= int(chunk) < 2 ** 64):
        raise ValueError(f"recipe_generator: rank {rank}, iteration {iteration}, chunk {chunk}")
    key = np.array([int(seed) & _M64, (int(rank) << 44) | int(iteration)], dtype=np.uint64)
    return np.random.Generator(np.random.Philox(key=key, counter=np.array([0, 0, 0, int(chunk)], dtype=np.uint64)))


def pose_matrix(R, t_model_units):
    """4 x 4 float64 object-to-camera pose with the translation in metres."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, np.asarray(t_model_units, dtype=np.float64) * DEPTH_TO_M
    return T


def rigid_inverse(T):
    """[R^T | -R^T t]: the stated inverse of a pose."""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def draw_recipe(seed, rank, iteration, candidates, models, cfg, chunk=0):
    """Everything random for `candidates` pairs (module docstring, part 1).  models: {obj_id: {"diameter": d, "centre": (3,)}} in model
    units (the model's bounding sphere; `OnlinePairs.model_table` builds it); cfg: the dataset cfg (`n_sample_observed_point`,
    `shift_range`, `online.*`).  -> dict of arrays with a leading `candidates` axis: obj, occ_obj (object ids), R_ref, t_ref, R_q, t_q,
    R_occ, t_occ (model units), occ, dilate (bool coins), spin (3, 3), shift (3,), noise (n_obs, 3), keys (2,) uint64, labels: target
    (4, 4) float64 = T_q T_r^-1 spin, rotation_label / translation_label float32."""
    oc = online_cfg(cfg)
    H, W = oc["canvas"]
    f, short = float(oc["focal"]), min(H, W)
    n_obs, shift_range = int(_get(cfg, "n_sample_observed_point")), float(_get(cfg, "shift_range"))
    ids = sorted(models)
    if not ids:
        raise ValueError("draw_recipe: no models")
    rng = recipe_generator(seed, rank, iteration, chunk)
    C = int(candidates)
    out = dict(obj=np.zeros(C, np.int64), occ_obj=np.zeros(C, np.int64), R_ref=np.zeros((C, 3, 3)), t_ref=np.zeros((C, 3)), R_q=np.zeros((C, 3, 3)),
               t_q=np.zeros((C, 3)), R_occ=np.zeros((C, 3, 3)), t_occ=np.zeros((C, 3)), occ=np.zeros(C, bool), dilate=np.zeros(C, bool),
               spin=np.zeros((C, 3, 3)), shift=np.zeros((C, 3)), noise=np.zeros((C, n_obs, 3)), keys=np.zeros((C, 2), np.uint64),
               target=np.zeros((C, 4, 4)), rotation_label=np.zeros((C, 3, 3), np.float32), translation_label=np.zeros((C, 3), np.float32))

    def place(R, centre, position):  # the translation that puts the model's centre at `position`
        return np.asarray(position, dtype=np.float64) - R @ np.asarray(centre, dtype=np.float64)

    for k in range(C):
        obj = ids[int(rng.integers(len(ids)))]
        m = models[obj]
        diam = float(m["diameter"])
        R_ref = _uniform_rotation(rng)
        z_ref = f * diam / (rng.uniform(*oc["fill"]) * short)
        R_q = _uniform_rotation(rng)
        z_q = f * diam / (rng.uniform(*oc["fill"]) * short)
        ox, oy = rng.uniform(-1.0, 1.0, 2) * float(oc["offset"])
        p_q = np.array([ox * (W / 2.0) * z_q / f, oy * (H / 2.0) * z_q / f, z_q])
        occ = rng.random() < float(oc["occluder_prob"])
        others = [o for o in ids if o != obj] or ids
        occ_obj = others[int(rng.integers(len(others)))]
        R_occ = _uniform_rotation(rng)
        angle, reach = rng.uniform(0.0, 2 * np.pi), rng.uniform(0.4, 1.0) * 0.5 * (diam + float(models[occ_obj]["diameter"]))
        z_occ = max(rng.uniform(0.45, 0.75) * z_q, float(models[occ_obj]["diameter"]))
        p_occ = np.array([p_q[0] + reach * np.cos(angle), p_q[1] + reach * np.sin(angle), z_q]) * (z_occ / z_q)
        dilate = rng.random() < 0.5
        spin = rotation_xyz(rng.random(3) * 2 * np.pi)
        shift = rng.uniform(-shift_range, shift_range, 3)
        noise = rng.standard_normal((n_obs, 3))
        keys = rng.integers(0, 2 ** 64, 2, dtype=np.uint64)
        t_ref, t_q = place(R_ref, m["centre"], (0.0, 0.0, z_ref)), place(R_q, m["centre"], p_q)
        spin4 = np.eye(4)
        spin4[:3, :3] = spin
        target = pose_matrix(R_q, t_q) @ rigid_inverse(pose_matrix(R_ref, t_ref)) @ spin4
        for name, value in (("obj", obj), ("occ_obj", occ_obj), ("R_ref", R_ref), ("t_ref", t_ref), ("R_q", R_q), ("t_q", t_q), ("R_occ", R_occ),
                            ("t_occ", place(R_occ, models[occ_obj]["centre"], p_occ)), ("occ", occ), ("dilate", dilate), ("spin", spin),
                            ("shift", shift), ("noise", noise), ("keys", keys), ("target", target),
                            ("rotation_label", target[:3, :3].astype(np.float32)), ("translation_label", (target[:3, 3] + shift).astype(np.float32))):
            out[name][k] = value
    return out


# ---- the scene: a background plane and a depth-sensor model ---------------------------------------------------------------------------
def draw_scene(seed, rank, iteration, candidates, recipe, models, cfg, chunk=0):
    """Everything random of the scene stage for the `candidates` pairs of `recipe` (module docstring, part 4), from the generator
    `recipe_generator(seed, rank, iteration, SCENE_CHUNK0 + chunk)`: `draw_recipe`'s stream is not touched.  Per candidate, whatever the
    configuration says: two 64-bit view keys (query, reference); the plane's gap (uniform in `plane_gap`), tilt (uniform in [0, plane_tilt])
    and tilt direction, the turn of its in-plane axes (both uniform in [0, 2 pi)); a 64-bit texture key.  All trigonometry happens here, in
    float64.  -> dict of arrays with a leading `candidates` axis: keys (2,) uint64, plane (bool: the query has a background), n, p0, u, v
    (3,) float64 in model units, camera frame (unit normal facing the camera, a point of the plane, two in-plane unit axes), cell (texture
    cell in model units), tex_key uint64."""
    sc = online_cfg(cfg)["scene"]
    if sc is None:
        raise ValueError("draw_scene: dataloader.train.online.scene is not set")
    rng = recipe_generator(seed, rank, iteration, SCENE_CHUNK0 + int(chunk))
    C = int(candidates)
    out = dict(keys=np.zeros((C, 2), np.uint64), plane=np.full(C, sc["background"] == "plane"), n=np.zeros((C, 3)), p0=np.zeros((C, 3)),
               u=np.zeros((C, 3)), v=np.zeros((C, 3)), cell=np.zeros(C), tex_key=np.zeros(C, np.uint64))
    for k in range(C):
        m = models[int(recipe["obj"][k])]
        diam = float(m["diameter"])
        keys = rng.integers(0, 2 ** 64, 2, dtype=np.uint64)
        gap = rng.uniform(*sc["plane_gap"])
        tilt, phi, psi = rng.uniform(0.0, np.deg2rad(float(sc["plane_tilt"]))), rng.uniform(0.0, 2 * np.pi), rng.uniform(0.0, 2 * np.pi)
        tex_key = rng.integers(0, 2 ** 64, 1, dtype=np.uint64)[0]
        centre = recipe["R_q"][k] @ np.asarray(m["centre"], dtype=np.float64) + recipe["t_q"][k]  # the query's model centre, z_q its depth
        axis = np.array([np.cos(phi), np.sin(phi), 0.0])  # (0, 0, -1) turned by `tilt` about this in-image axis (Rodrigues; axis . n = 0)
        n = np.array([-np.sin(phi) * np.sin(tilt), np.cos(phi) * np.sin(tilt), -np.cos(tilt)])
        side = np.cross(n, axis)  # axis and side span the plane
        for name, value in (("keys", keys), ("n", n), ("p0", centre * ((centre[2] + (0.5 + gap) * diam) / centre[2])),
                            ("u", np.cos(psi) * axis + np.sin(psi) * side), ("v", np.cos(psi) * side - np.sin(psi) * axis),
                            ("cell", float(sc["texture_cell"]) * diam), ("tex_key", tex_key)):
            out[name][k] = value
    return out


def _threshold(prob):
    """A probability as the integer threshold both routes compare the upper 32 bits of a hash with (`hash >> 32 < threshold`)."""
    return int(np.rint(float(prob) * 2.0 ** 32))


def scene_rows(scene, oc, which):
    """The per-view descriptors of `sense_views_host` / `ops.sense_views`, (C, SCENE_DESC) uint64 words (floats are float64 bit patterns),
    for the C queries (`which` = "query": key 0, the background plane where the pair has one), the C references ("reference": key 1, no
    plane) or C views no stage touches ("off").  Words: 0 view key, 1 texture key, 2 plane (0 / 1), 3 hole threshold, 4 edge-drop threshold,
    5 hole cell (pixels), 6 disparity steps, 7 unused; float64 from here: 8 9 10 the noise's a, b, z0, 11 focal x baseline (pixel metres),
    12 edge threshold, 13-15 n, 16 n . p0 (metres), 17-19 p0 (metres), 20-22 u, 23-25 v, 26 texture cell (metres), 27 z_max (metres),
    28 29 30 the camera's f, cx, cy, 31 unused."""
    sc = oc["scene"]
    C = len(scene["keys"])
    H, W = oc["canvas"]
    words, fl = np.zeros((C, SCENE_DESC), np.uint64), np.zeros((C, SCENE_DESC))
    words[:, 5] = 1
    fl[:, 11], fl[:, 13:16], fl[:, 26], fl[:, 27], fl[:, 28], fl[:, 29], fl[:, 30] = 1.0, (0.0, 0.0, -1.0), 1.0, SCENE_Z_MAX_M, float(oc["focal"]), W / 2.0, H / 2.0
    if which != "off":
        words[:, 0] = scene["keys"][:, 0 if which == "query" else 1]
        words[:, 3], words[:, 4], words[:, 5], words[:, 6] = _threshold(sc["hole_prob"]), _threshold(sc["edge_drop"]), sc["hole_cell"], sc["disparity_steps"]
        fl[:, 8:11], fl[:, 11], fl[:, 12] = sc["noise"], float(oc["focal"]) * float(sc["baseline_m"]), float(sc["edge_thres"])
    if which == "query":
        words[:, 1], words[:, 2] = scene["tex_key"], scene["plane"]
        p0 = scene["p0"] * DEPTH_TO_M
        fl[:, 13:16], fl[:, 17:20], fl[:, 20:23], fl[:, 23:26], fl[:, 26] = scene["n"], p0, scene["u"], scene["v"], scene["cell"] * DEPTH_TO_M
        fl[:, 16] = (scene["n"][:, 0] * p0[:, 0] + scene["n"][:, 1] * p0[:, 1]) + scene["n"][:, 2] * p0[:, 2]
    words[:, 8:31] = fl[:, 8:31].view(np.uint64)
    return words


def check_scene_rows(desc, H, W):
    """Range-check descriptors for (H, W) canvases (both routes call this before they touch a pixel) -> (V, SCENE_DESC) uint64, contiguous."""
    desc = np.ascontiguousarray(desc, dtype=np.uint64)
    if desc.ndim != 2 or desc.shape[1] != SCENE_DESC:
        raise ValueError(f"scene descriptors {desc.shape} are not (views, {SCENE_DESC})")
    fl = desc.view(np.float64)
    ints = desc[:, 2:7]
    if (ints[:, 0] > 1).any() or (ints[:, 1:3] > 2 ** 32).any() or (ints[:, 3] < 1).any() or (ints[:, 3] > 2 ** 15).any() or (ints[:, 4] >= 2 ** 20).any():
        raise ValueError("scene descriptors: plane flag, thresholds, hole cell or disparity steps out of range")
    if not np.isfinite(fl[:, 8:31]).all() or (fl[:, 8:10] < 0).any() or (fl[:, 12] < 0).any() or (fl[:, [11, 26, 27, 28]] <= 0).any():
        raise ValueError("scene descriptors: a constant is not finite or has the wrong sign")
    # lattice coordinates stay inside the 20 bits the texture hash packs: |point - p0| <= z_max |r| + |p0|, the last octave scales by 4
    reach = fl[:, 27] * np.sqrt(1.0 + ((W + np.abs(fl[:, 29])) / fl[:, 28]) ** 2 + ((H + np.abs(fl[:, 30])) / fl[:, 28]) ** 2) + np.linalg.norm(fl[:, 17:20], axis=1)
    if ((desc[:, 2] == 1) & (4.0 * reach / fl[:, 26] >= 2.0 ** 19 - 2)).any():
        raise ValueError("scene descriptors: the texture cell is too small for the reach of the background plane")
    return desc


def _scene_hash(key, stream, index):
    """The random word of (view or texture key, stream number, pixel / cell / lattice index < 2^40): uint64 array."""
    return _mix(np.uint64(key) ^ _mix((np.asarray(index).astype(np.uint64) | np.uint64(int(stream) << 40)) + _GOLD))


def _scene_texture(tex_key, s, t):
    """Three octaves of value noise at plane coordinates (s, t) (float64 arrays, in texture cells) -> (..., 3) uint8.  Octave o looks up the
    lattice at (2^o s, 2^o t): the four corners' bytes (byte c of the hash of (texture key, stream 3 + o, corner) for channel c) are blended
    along s, then along t; the octaves are weighted 0.5, 0.3, 0.2 and added in that order; floor(x + 0.5)."""
    out = np.zeros(s.shape + (3,), np.uint8)
    total = [None, None, None]
    for o, weight in enumerate(SCENE_OCTAVE_WEIGHTS):
        so, to = s * float(1 << o), t * float(1 << o)
        fu_floor, fv_floor = np.floor(so), np.floor(to)
        fu, fv = so - fu_floor, to - fv_floor
        iu, iv = fu_floor.astype(np.int64), fv_floor.astype(np.int64)
        corner = lambda du, dv: _scene_hash(tex_key, SCENE_STREAM_TEXTURE + o, (((iu + du) & 0xFFFFF) << 20) | ((iv + dv) & 0xFFFFF))  # noqa: E731
        h00, h10, h01, h11 = corner(0, 0), corner(1, 0), corner(0, 1), corner(1, 1)
        for c in range(3):
            b00, b10, b01, b11 = (((h >> np.uint64(8 * c)) & np.uint64(255)).astype(np.float64) for h in (h00, h10, h01, h11))
            top, bottom = b00 + (b10 - b00) * fu, b01 + (b11 - b01) * fu
            value = (top + (bottom - top) * fv) * weight
            total[c] = value if total[c] is None else total[c] + value
    for c in range(3):
        out[..., c] = np.floor(total[c] + 0.5).astype(np.uint8)
    return out


def sense_views_host(depth, rgb, desc, with_intermediates=False):
    """The pixel rule of the scene stage (module docstring, part 4): depth (V, H, W) float32 in model units and rgb (V, H, W, 3) uint8 with
    one descriptor row per view (`scene_rows`) -> new (depth, rgb).  with_intermediates: also a list with, per view, dict(z = the float64
    depth in metres after the background and before drop-outs and noise, background, edge, dropped (bool masks), g (the unit noise))."""
    depth, rgb = np.asarray(depth, dtype=np.float32), np.asarray(rgb, dtype=np.uint8)
    V, H, W = depth.shape
    if rgb.shape != (V, H, W, 3):
        raise ValueError(f"sense_views_host: rgb {rgb.shape} for depth {depth.shape}")
    desc = check_scene_rows(desc, H, W)
    if len(desc) != V:
        raise ValueError(f"sense_views_host: {len(desc)} descriptors for {V} views")
    out_depth, out_rgb, infos = depth.copy(), rgb.copy(), []
    ys, xs = np.mgrid[0:H, 0:W]
    pix = ys * W + xs
    for v in range(V):
        w, fl = desc[v], desc[v].view(np.float64)
        key, hole_thr, edge_thr, hole_cell, steps = w[0], np.uint64(w[3]), np.uint64(w[4]), int(w[5]), int(w[6])
        a, b, z0, fb, edge_thres = fl[8:13]
        raw = depth[v]
        z = np.where(raw > 0, raw.astype(np.float64) * DEPTH_TO_M, 0.0)
        # (a) the background plane where the view is empty
        background = np.zeros((H, W), bool)
        if int(w[2]):
            f, cx, cy = fl[28:31]
            rx, ry = (xs.astype(np.float64) - cx) / f, (ys.astype(np.float64) - cy) / f
            nr = (fl[13] * rx + fl[14] * ry) + fl[15]
            facing = ~(raw > 0) & (nr < 0.0)
            zb = fl[16] / np.where(facing, nr, -1.0)
            background = facing & (zb > 0.0) & (zb <= fl[27])
            z = np.where(background, zb, z)
            dx, dy, dz = rx * zb - fl[17], ry * zb - fl[18], zb - fl[19]
            s = ((dx * fl[20] + dy * fl[21]) + dz * fl[22]) / fl[26]
            t = ((dx * fl[23] + dy * fl[24]) + dz * fl[25]) / fl[26]
            s, t = np.where(background, s, 0.0), np.where(background, t, 0.0)
            out_rgb[v] = np.where(background[:, :, None], _scene_texture(w[1], s, t), rgb[v])
        # (b) drop-outs on the noise-free depth: holes per cell, and edge pixels
        surface = z > 0.0
        cells = (ys // hole_cell) * ((W + hole_cell - 1) // hole_cell) + xs // hole_cell
        dropped = surface & ((_scene_hash(key, SCENE_STREAM_HOLE, cells) >> np.uint64(32)) < hole_thr)
        edge = np.zeros((H, W), bool)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = ys + dy, xs + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            zn = z[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            edge |= inside & (~(zn > 0.0) | (np.abs(z - zn) > edge_thres * z))
        edge &= surface
        dropped |= edge & ((_scene_hash(key, SCENE_STREAM_EDGE, pix) >> np.uint64(32)) < edge_thr)
        # (c) axial noise, then disparity quantisation
        h = _scene_hash(key, SCENE_STREAM_NOISE, pix)
        fields = sum(((h >> np.uint64(16 * i)) & np.uint64(0xFFFF)).astype(np.int64) for i in range(4))
        g = (fields - 131070).astype(np.float64) * SCENE_G_SCALE
        sensed = surface & ~dropped
        new = z
        if a != 0.0 or b != 0.0 or steps:
            new = z + (a + b * ((z - z0) * (z - z0))) * g
            ok = new > 0.0  # noise below the camera plane: no return
            if steps:
                with np.errstate(divide="ignore", invalid="ignore"):
                    k = np.rint((float(steps) * fb) / np.where(ok, new, 1.0))
                    ok &= k >= 1.0  # less than one disparity step: beyond the sensor's range
                    new = fb / (np.where(ok, k, 1.0) / float(steps))
            new = np.where(ok, new, 0.0)
            touched = sensed
        else:
            touched = sensed & background
        out_depth[v] = np.where(dropped, np.float32(0), np.where(touched, (new * 1000.0).astype(np.float32), raw))
        infos.append(dict(z=z, background=background, edge=edge, dropped=dropped, g=g))
    return (out_depth, out_rgb, infos) if with_intermediates else (out_depth, out_rgb)


# ---- the item rule -------------------------------------------------------------------------------------------------------------------
def _extents(mask):
    """Half-open extents (top, bottom, left, right) of a mask; (H, 0, W, 0) when empty (the device table's convention)."""
    ys, xs = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if len(ys) == 0:
        return mask.shape[0], 0, mask.shape[1], 0
    return int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1


def query_valid(full, visible, cfg):
    """The visibility rule on the table's counts."""
    return visible > 0 and visible >= int(_get(cfg, "min_px_count_visib")) and np.float64(visible) / np.float64(max(full, 1)) >= float(_get(cfg, "min_visib_fract"))


def _ordered_mean(points, n):
    """Sum in the given order (np.cumsum adds sequentially) / n."""
    return np.cumsum(points, axis=0)[-1] / np.float64(n)


def _distance(points, mean):
    d = points - mean.reshape(1, 3)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def view_table_row(obj_depth, occ_depth, dilate):
    """One view's masks and table row -> (final mask, visible, scene depth selector `front`, row [full, visible, set, top, bottom, left, right, 0])."""
    full = obj_depth > 0
    has_occ = occ_depth > 0
    visible = full & (~has_occ | (obj_depth <= occ_depth))
    mask = dilate_cross(visible, 4) > 0 if dilate else visible
    front = ~visible & has_occ
    row = np.array([full.sum(), visible.sum(), mask.sum(), *_extents(mask), 0], dtype=np.int32)
    return mask, visible, front, row


def items_from_views_host(views, recipe, cfg, with_intermediates=False, scene=None):
    """The item rule (module docstring, part 2).  views: ref_rgb, q_rgb, occ_rgb (C, H, W, 3) uint8 and ref_depth, q_depth, occ_depth
    (C, H, W) float32 (occluder canvases 0 where the pair has none).  -> a list of C entries: None for an invalid pair, else the
    `device_crops` form of the provider's item: pts, rgb_choose, translation_label, rotation_label, tem1_choose, tem1_pts, K and
    rgb_crop / rgb_cropmask, tem1_crop / tem1_cropmask (uint8 window crops of the scene colour and the window masks; `finish_item` turns
    them into rgb / tem1_rgb).  with_intermediates: (items, info) with info[k] = dict of every intermediate (tables, masks, scene, windows,
    counts, radius, why an invalid pair is invalid).  scene: `draw_scene`'s dict; the references' depth is then sensed (drop-outs, noise)
    before anything reads it, and each query's composed scene depth and colour (background, drop-outs, noise) after its mask and table row
    are taken from the renders: the mask stays the detector's, as the provider's is, and a hole inside it lifts to the camera centre."""
    oc = online_cfg(cfg)
    K = camera_matrix(oc)
    S, n_obs, n_tpl = int(_get(cfg, "img_size")), int(_get(cfg, "n_sample_observed_point")), int(_get(cfg, "n_sample_template_point"))
    use_dilation = bool(_get(cfg, "dilate_mask"))
    C = len(recipe["obj"])
    items, infos = [], []
    ref_depth = views["ref_depth"]
    if scene is not None:
        ref_depth, _ = sense_views_host(ref_depth, views["ref_rgb"], scene_rows(scene, oc, "reference"))
        q_rows = scene_rows(scene, oc, "query")
    for k in range(C):
        info = dict(valid=False, why=None)
        infos.append(info)
        items.append(None)
        # -- reference
        rd = np.asarray(ref_depth[k], dtype=np.float32)
        r_mask, _, _, r_row = view_table_row(rd, np.zeros_like(rd), False)
        qd, cd = np.asarray(views["q_depth"][k], dtype=np.float32), np.asarray(views["occ_depth"][k], dtype=np.float32)
        q_mask, q_visible, front, q_row = view_table_row(qd, cd, use_dilation and bool(recipe["dilate"][k]))
        scene_depth = np.where(q_visible, qd, np.where(front, cd, np.float32(0))).astype(np.float32)
        scene_rgb = np.where(q_visible[:, :, None], views["q_rgb"][k], np.where(front[:, :, None], views["occ_rgb"][k], 0)).astype(np.uint8)
        if scene is not None:
            scene_depth, scene_rgb = (a[0] for a in sense_views_host(scene_depth[None], scene_rgb[None], q_rows[k:k + 1]))
        info.update(ref_row=r_row, q_row=q_row, ref_mask=r_mask, q_mask=q_mask, q_visible=q_visible, scene_depth=scene_depth, scene_rgb=scene_rgb)
        if r_row[2] == 0:
            info["why"] = "reference empty"
            continue
        if not query_valid(int(q_row[0]), int(q_row[1]), cfg):
            info["why"] = "query visibility"
            continue
        r_win = Window.from_extents(rd.shape, *r_row[3:7])
        r_inside = r_win.crop(r_mask)
        r_pix = np.flatnonzero(r_inside)
        info.update(ref_window=r_win.as_list(), ref_set=len(r_pix), ref_rows=r_inside.sum(axis=1))
        if len(r_pix) == 0:
            info["why"] = "reference window empty"
            continue
        r_choose = r_pix[draw_index(recipe["keys"][k, 0], np.arange(n_tpl), len(r_pix), n_tpl)]
        tem_pts = lift_depth(rd.astype(np.float64) * DEPTH_TO_M, K, r_win).reshape(-1, 3)[r_choose]
        radius = _distance(tem_pts, _ordered_mean(tem_pts, n_tpl)).max()
        info.update(radius=radius)
        # -- query
        q_win = Window.from_extents(qd.shape, *q_row[3:7])
        q_inside = q_win.crop(q_mask)
        q_pix = np.flatnonzero(q_inside)
        info.update(q_window=q_win.as_list(), q_set=len(q_pix), q_rows=q_inside.sum(axis=1))
        if len(q_pix) == 0:
            info["why"] = "query window empty"
            continue
        cloud = lift_depth(scene_depth.astype(np.float64) * DEPTH_TO_M, K, q_win)
        row_sums = np.cumsum(cloud * q_inside[:, :, None], axis=1)[:, -1, :]  # a row left to right (an unset pixel adds 0.0) ...
        mean = _ordered_mean(row_sums, len(q_pix))  # ... the rows top to bottom
        pts = cloud.reshape(-1, 3)[q_pix]
        keep = _distance(pts, mean) < 1.2 * radius
        pts, q_pix = pts[keep], q_pix[keep]
        info.update(q_mean=mean, q_kept=len(q_pix))
        if len(q_pix) < MIN_KEPT:
            info["why"] = "kept points"
            continue
        sel = draw_index(recipe["keys"][k, 1], np.arange(n_obs), len(q_pix), n_obs)
        q_choose, pts = q_pix[sel], pts[sel]
        # -- labels and augmentation
        spin, shift = recipe["spin"][k], recipe["shift"][k]
        tem_spun = np.stack([(tem_pts[:, 0] * spin[0, j] + tem_pts[:, 1] * spin[1, j]) + tem_pts[:, 2] * spin[2, j] for j in range(3)], axis=1)
        pts = pts + (shift.reshape(1, 3) + 0.001 * recipe["noise"][k])
        info.update(valid=True)
        items[k] = {"pts": torch.from_numpy(pts.astype(np.float32)), "rgb_choose": torch.from_numpy(q_win.to_resized(q_choose, S)),
                    "translation_label": torch.from_numpy(recipe["translation_label"][k].copy()),
                    "rotation_label": torch.from_numpy(recipe["rotation_label"][k].copy()),
                    "tem1_choose": torch.from_numpy(r_win.to_resized(r_choose, S)), "tem1_pts": torch.from_numpy(tem_spun.astype(np.float32)),
                    "K": torch.from_numpy(K.copy()),
                    "rgb_crop": np.ascontiguousarray(q_win.crop(scene_rgb)), "rgb_cropmask": np.ascontiguousarray(q_inside).view(np.uint8),
                    "tem1_crop": np.ascontiguousarray(r_win.crop(np.where(r_mask[:, :, None], views["ref_rgb"][k], 0).astype(np.uint8))),
                    "tem1_cropmask": np.ascontiguousarray(r_inside).view(np.uint8)}
    return (items, infos) if with_intermediates else items


def finish_item(item, img_size, rgb_mask_flag=True, plans=(None, None)):
    """An entry of `items_from_views_host` -> the provider's 9-key item: the crops through (`ColorAugmentor.apply` of the plan) -> mask ->
    `resize_bilinear_u8` -> `to_tensor_normalize`, as `MegaPoseOneRefTrainSet._crop_tensor`."""
    out = {k: v for k, v in item.items() if not k.endswith(("_crop", "_cropmask"))}
    for (key, stem), plan in zip((("rgb", "rgb_"), ("tem1_rgb", "tem1_")), plans):
        crop, mask = item[stem + "crop"], item[stem + "cropmask"]
        if plan is not None and len(plan):
            crop = ColorAugmentor(0).apply(crop, plan)
        if rgb_mask_flag:
            crop = crop * (mask[:, :, None] > 0).astype(np.uint8)
        out[key] = to_tensor_normalize(resize_bilinear_u8(np.ascontiguousarray(crop), img_size))
    order = ("pts", "rgb", "rgb_choose", "translation_label", "rotation_label", "tem1_rgb", "tem1_choose", "tem1_pts", "K")
    return {k: out[k] for k in order}


def draw_plans(seed, rank, iteration, sizes):
    """The colour-augmentation plans of a batch: sizes = per taken pair ((h, w) of the query crop, (h, w) of the reference crop) -> a list of
    (query plan, reference plan); per image the provider's 0.8 coin, then `ColorAugmentor.plan`, on the iteration's `AUG_CHUNK` generator."""
    aug = ColorAugmentor()
    aug.rng = recipe_generator(seed, rank, iteration, AUG_CHUNK)
    plans = []
    for pair in sizes:
        plans.append(tuple(aug.plan(h, w) if aug.rng.random() < 0.8 else AugPlan() for h, w in pair))
    return plans


# ---- the batch source ----------------------------------------------------------------------------------------------------------------
class OnlinePairs:
    """Module docstring, part 3.  models: a folder of `obj_XXXXXX.ply` files or {obj_id: path}; cfg: the dataset cfg (the provider's fields
    plus `online.*`, `batch_size` given here); `augment`: False leaves the crops unaugmented (empty plans; no generator draw)."""

    def __init__(self, models, cfg, device, seed, rank=0, world=1, host=False, batch_size=None, obj_ids=None, augment=True):
        from .bop_eval import read_ply_model
        from .render import HipDepthRenderer, HipShadedRenderer
        from .render_train import load_model

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("OnlinePairs: CPU not supported (the views are rendered on the GPU)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cfg, self.oc = cfg, online_cfg(cfg)
        self.seed, self.rank, self.world, self.host, self.augment = int(seed), int(rank), int(world), bool(host), bool(augment)
        self.B = int(batch_size if batch_size is not None else _get(cfg, "batch_size", 8))
        self.S, self.n_obs, self.n_tpl = int(_get(cfg, "img_size")), int(_get(cfg, "n_sample_observed_point")), int(_get(cfg, "n_sample_template_point"))
        self.rgb_mask_flag = bool(_get(cfg, "rgb_mask_flag"))
        self.K = camera_matrix(self.oc)
        if isinstance(models, (str, os.PathLike)):
            folder = os.fspath(models)
            found = {int(f[4:10]): osp.join(folder, f) for f in sorted(os.listdir(folder)) if f.startswith("obj_") and f.endswith(".ply") and f[4:10].isdigit()}
        else:
            found = {int(k): os.fspath(v) for k, v in models.items()}
        if obj_ids is not None:
            found = {int(o): found[int(o)] for o in obj_ids}
        if not found:
            raise ValueError(f"OnlinePairs: no obj_XXXXXX.ply model in {models}")
        H, W = self.oc["canvas"]
        self.ren_rgb = HipShadedRenderer(W, H, device=self.device, ambient=float(self.oc["ambient"]), shading=self.oc["shading"], ssaa=int(self.oc["ssaa"]))
        self.ren_depth = HipDepthRenderer(W, H, device=self.device)
        self.models = {}
        for o, path in found.items():
            kw = load_model(osp.dirname(path), o) if osp.basename(path) == f"obj_{o:06d}.ply" else None
            if kw is None:
                m = read_ply_model(path)
                kw = dict(verts=m["pts"], faces=m["faces"], normals=m["normals"])
                if m["colors"] is not None:
                    kw["colors"] = m["colors"]
            self.ren_rgb.add_object(o, **kw)
            self.ren_depth.add_object(o, kw["verts"], kw["faces"])
            self.models[o] = self.model_table(kw["verts"])
        self._side = None

    @staticmethod
    def model_table(verts):
        """The bounding sphere the recipe places: centre of the bounding box, diameter = twice the farthest vertex from it."""
        v = np.asarray(verts, dtype=np.float64)
        centre = (v.min(axis=0) + v.max(axis=0)) / 2
        return dict(centre=centre, diameter=2.0 * float(np.linalg.norm(v - centre, axis=1).max()))

    # -- rendering: grouped by object
    def _render(self, objs, Rs, ts, colour, depth):
        """View n shows object objs[n] under (Rs[n], ts[n]); rows of `colour` / `depth` are filled in place, one render per object."""
        H, W = self.oc["canvas"]
        k4 = [float(self.K[0, 0]), float(self.K[1, 1]), float(self.K[0, 2]), float(self.K[1, 2])]
        for o in sorted(set(int(v) for v in objs)):
            idx = np.flatnonzero(np.asarray(objs) == o)
            rgb = self.ren_rgb.render_batch(o, Rs[idx], ts[idx], k4)
            dep = self.ren_depth.render_batch(o, Rs[idx], ts[idx], k4)
            at = torch.from_numpy(idx).to(self.device)
            colour.index_copy_(0, at, rgb)
            depth.index_copy_(0, at, dep)

    def render_chunk(self, recipe):
        """-> canvases on the device: views 0 .. C - 1 the queries, C .. 2 C - 1 the references, and the C occluder canvases (zero where the
        coin failed)."""
        C = len(recipe["obj"])
        H, W = self.oc["canvas"]
        colour = torch.zeros((2 * C, H, W, 3), dtype=torch.uint8, device=self.device)
        depth = torch.zeros((2 * C, H, W), dtype=torch.float32, device=self.device)
        self._render(np.concatenate([recipe["obj"], recipe["obj"]]), np.concatenate([recipe["R_q"], recipe["R_ref"]]),
                     np.concatenate([recipe["t_q"], recipe["t_ref"]]), colour, depth)
        occ_colour = torch.zeros((C, H, W, 3), dtype=torch.uint8, device=self.device)
        occ_depth = torch.zeros((C, H, W), dtype=torch.float32, device=self.device)
        on = np.flatnonzero(recipe["occ"])
        if len(on):
            sub_c = torch.zeros((len(on), H, W, 3), dtype=torch.uint8, device=self.device)
            sub_d = torch.zeros((len(on), H, W), dtype=torch.float32, device=self.device)
            self._render(recipe["occ_obj"][on], recipe["R_occ"][on], recipe["t_occ"][on], sub_c, sub_d)
            at = torch.from_numpy(on).to(self.device)
            occ_colour.index_copy_(0, at, sub_c)
            occ_depth.index_copy_(0, at, sub_d)
        return colour, depth, occ_colour, occ_depth

    # -- one chunk on the device
    def chunk_device(self, recipe, canvases, scene=None):
        """The device form of `items_from_views_host` for one chunk -> dict(valid (C,) bool, windows, win_rows, tensors ...) with everything
        per pixel and per point left on the device.  scene: `draw_scene`'s dict: `ops.sense_views` runs on the references before
        `ops.item_views` and on the composed queries after it (the other half of the views passes through either launch unchanged)."""
        from . import ops
        from .ops.rle import _to_host

        colour, depth, occ_colour, occ_depth = canvases
        C = len(recipe["obj"])
        H, W = self.oc["canvas"]
        use_dilation = bool(_get(self.cfg, "dilate_mask"))
        occ_slot = np.concatenate([np.where(recipe["occ"], np.arange(C), -1), np.full(C, -1)])
        dilate = np.concatenate([recipe["dilate"] & use_dilation, np.zeros(C, bool)])
        if scene is not None:
            off = scene_rows(scene, self.oc, "off")
            depth, colour = ops.sense_views(depth, colour, np.concatenate([off, scene_rows(scene, self.oc, "reference")]))
        mask, scene_depth, scene_rgb, table = ops.item_views(depth, colour, occ_depth, occ_colour, occ_slot, dilate)
        if scene is not None:
            scene_depth, scene_rgb = ops.sense_views(scene_depth, scene_rgb, np.concatenate([scene_rows(scene, self.oc, "query"), off]))
        tab = _to_host(table)  # readback 1: counts and extents per view
        valid = np.zeros(C, bool)
        q_win, r_win = [None] * C, [None] * C
        for k in range(C):
            q, r = tab[k], tab[C + k]
            if r[2] == 0 or not query_valid(int(q[0]), int(q[1]), self.cfg):
                continue
            valid[k] = True
            q_win[k], r_win[k] = Window.from_extents((H, W), *q[3:7]), Window.from_extents((H, W), *r[3:7])
        out = dict(valid=valid, table=tab, mask=mask, scene_depth=scene_depth, scene_rgb=scene_rgb, q_win=q_win, r_win=r_win)
        if not valid.any():
            return out
        radius = torch.zeros(C, dtype=torch.float64, device=self.device)
        noise = torch.from_numpy(np.ascontiguousarray(recipe["noise"])).to(self.device)
        pairs = np.arange(C)
        common = (C, recipe["keys"], recipe["spin"], recipe["shift"])
        tem_pts, tem_choose, r_counts, r_rows = ops.item_points(mask, scene_depth, self.K, C + pairs, r_win, pairs, *common, None, self.n_tpl, self.S, True, radius)
        pts, choose, q_counts, q_rows = ops.item_points(mask, scene_depth, self.K, pairs, q_win, pairs, *common, noise, self.n_obs, self.S, False, radius)
        side = int(q_rows.shape[1])
        back = _to_host(torch.cat([q_counts.reshape(-1), r_counts.reshape(-1), q_rows.reshape(-1), r_rows.reshape(-1)]))  # readback 2
        q_counts, r_counts = back[:2 * C].reshape(C, 2), back[2 * C:4 * C].reshape(C, 2)
        q_rows, r_rows = back[4 * C:4 * C + C * side].reshape(C, side), back[4 * C + C * side:].reshape(C, side)
        valid &= (r_counts[:, 0] > 0) & (q_counts[:, 1] >= MIN_KEPT)
        out.update(valid=valid, pts=pts, rgb_choose=choose, tem1_pts=tem_pts, tem1_choose=tem_choose, q_counts=q_counts, r_counts=r_counts,
                   q_rows=q_rows, r_rows=r_rows, radius=radius)
        return out

    def _labels(self, recipe, take):
        take = np.asarray(take)
        return {"translation_label": torch.from_numpy(recipe["translation_label"][take]).to(self.device),
                "rotation_label": torch.from_numpy(recipe["rotation_label"][take]).to(self.device),
                "K": torch.from_numpy(np.repeat(self.K[None], len(take), axis=0)).to(self.device)}

    def _plans(self, iteration, sizes):
        if not self.augment:
            return [(AugPlan(), AugPlan()) for _ in sizes]
        return draw_plans(self.seed, self.rank, iteration, sizes)

    def batch(self, iteration):
        """The batch of `iteration` on the device, enqueued on the current stream."""
        from . import ops

        with torch.cuda.device(self.device):
            taken = []  # (recipe, chunk result or host items, candidate number)
            for chunk in range(int(self.oc["max_chunks"])):
                recipe = draw_recipe(self.seed, self.rank, iteration, self.B, self.models, self.cfg, chunk=chunk)
                canvases = self.render_chunk(recipe)
                scene = None
                if self.oc["scene"] is not None:
                    scene = draw_scene(self.seed, self.rank, iteration, self.B, recipe, self.models, self.cfg, chunk=chunk)
                if self.host:
                    colour, depth, occ_colour, occ_depth = (t.cpu().numpy() for t in canvases)
                    C = self.B
                    views = dict(q_rgb=colour[:C], ref_rgb=colour[C:], q_depth=depth[:C], ref_depth=depth[C:], occ_rgb=occ_colour, occ_depth=occ_depth)
                    res = items_from_views_host(views, recipe, self.cfg, scene=scene)
                    good = [k for k in range(C) if res[k] is not None]
                else:
                    res = self.chunk_device(recipe, canvases, scene=scene)
                    good = [int(k) for k in np.flatnonzero(res["valid"])]
                taken += [(recipe, res, k) for k in good[:self.B - len(taken)]]
                if len(taken) == self.B:
                    break
            else:
                raise RuntimeError(f"OnlinePairs: iteration {iteration}: {len(taken)} valid pairs of {self.B} after {self.oc['max_chunks']} chunks "
                                   "(dataloader.train.online.max_chunks, min_px_count_visib, min_visib_fract)")
            if self.host:
                sizes = [(res[k]["rgb_crop"].shape[:2], res[k]["tem1_crop"].shape[:2]) for _, res, k in taken]
                plans = self._plans(iteration, sizes)
                items = [finish_item(res[k], self.S, self.rgb_mask_flag, p) for (_, res, k), p in zip(taken, plans)]
                return {key: torch.stack([it[key] for it in items]).to(self.device) for key in items[0]}
            out = ops.finish_crops(self.collate_device(iteration, taken), self.device)
            order = ("pts", "rgb", "rgb_choose", "translation_label", "rotation_label", "tem1_rgb", "tem1_choose", "tem1_pts", "K")
            return {key: out[key] for key in order}

    def collate_device(self, iteration, taken):
        """taken: (recipe, `chunk_device` result, candidate number) per pair of the batch -> the batch as `provider_train.collate_pairs_device`
        lays it out (the `crop_*` keys for `ops.finish_crops`), atlas, masks and points on the device."""
        from . import ops

        B = len(taken)
        with torch.cuda.device(self.device):
            # the atlas: the B query crops, then the B reference crops (`collate_pairs_device`'s order)
            wins = [res["q_win"][k] for _, res, k in taken] + [res["r_win"][k] for _, res, k in taken]
            plans = self._plans(iteration, [((q.side, q.side), (r.side, r.side)) for q, r in zip(wins[:B], wins[B:])])
            boxes, y = [], 0
            for w in wins:
                boxes.append((y, w.side, w.side))
                y += w.side
            desc, aug_ops, grids, noise = pack_plans(boxes, [p[0] for p in plans] + [p[1] for p in plans])
            sides = np.array([w.side for w in wins], dtype=np.int64)
            mask_off = np.cumsum(sides * sides) - sides * sides
            atlas = torch.zeros((y, int(sides.max()), 3), dtype=torch.uint8, device=self.device)
            packed = torch.empty(int((sides * sides).sum()), dtype=torch.uint8, device=self.device)
            rows = np.concatenate([res["q_rows"][k][:res["q_win"][k].side] for _, res, k in taken] + [res["r_rows"][k][:res["r_win"][k].side] for _, res, k in taken])
            seen = []
            for _, res, _ in taken:  # one crop launch per contributing chunk
                if any(res is s for s in seen):
                    continue
                seen.append(res)
                C = len(res["valid"])
                slots = [i for i, (_, r, _) in enumerate(taken) if r is res]
                views = [taken[i][2] for i in slots] + [C + taken[i][2] for i in slots]
                at = slots + [B + i for i in slots]
                ops.item_crops(res["mask"], res["scene_rgb"], views, [wins[i] for i in at], atlas, packed, [boxes[i][0] for i in at], mask_off[at])
            batch = {"crop_atlas": atlas, "crop_desc": torch.from_numpy(desc), "crop_ops": torch.from_numpy(aug_ops), "crop_grids": torch.from_numpy(grids),
                     "crop_noise": torch.from_numpy(noise), "crop_masks": packed, "crop_rows": torch.from_numpy(rows.astype(np.int32)),
                     "crop_cfg": torch.tensor([self.S, int(self.rgb_mask_flag)], dtype=torch.int32)}
            for key in ("pts", "rgb_choose", "tem1_choose", "tem1_pts"):
                batch[key] = torch.stack([res[key][k] for _, res, k in taken])
            labels = [self._labels(recipe, [k]) for recipe, _, k in taken]
            for key in labels[0]:
                batch[key] = torch.cat([lab[key] for lab in labels])
            return batch

    # -- iteration with one batch of run-ahead
    def side_stream(self):
        from .pipeline import _pool_streams

        if self._side is None:
            self._side = _pool_streams(self.device, "features", 1)[0]
        return self._side

    def _prepare(self, iteration):
        side = self.side_stream()
        with torch.cuda.device(self.device), torch.cuda.stream(side):
            batch = self.batch(iteration)
            done = torch.cuda.Event()
            done.record(side)
        return batch, done

    def iterate(self, start=0):
        """Batches start, start + 1, ...: while the consumer runs step i, one helper thread prepares batch i + 1 on the side stream (the two
        table readbacks make the preparation wait on the host, so it cannot simply be enqueued ahead); a batch is handed over ordered by
        its event, its tensors recorded on the consumer's stream."""
        import itertools
        from concurrent.futures import ThreadPoolExecutor

        pool = ThreadPoolExecutor(1)
        try:
            pending = pool.submit(self._prepare, int(start))
            for iteration in itertools.count(int(start) + 1):
                batch, done = pending.result()
                pending = pool.submit(self._prepare, iteration)
                current = torch.cuda.current_stream(self.device)
                current.wait_event(done)
                for t in batch.values():
                    t.record_stream(current)
                yield batch
        finally:
            pool.shutdown(wait=True, cancel_futures=True)

    def __call__(self, iteration):  # fit's loader protocol: iteration -> iterable
        return self.iterate(iteration)

    def __iter__(self):
        return self.iterate(0)
