"""GPU: the proposal-matching kernels (csrc/detmatch.hip, ops/detect.py) against the numpy rule of unopose_amd/match_dets.py and against
float64, and the device route against the host route on the bop_synth dataset.

Tolerances.  `patch_valid` and `mask_nms` are integers: equality.  `token_unit_rows`: 2^-8 relative per element (half a bf16 ulp is at
most 2^-8 / (1 + 2^-8) of the value; the fp32 norm and quotient add about 2^-22).  `patch_match_score`, absolute 1e-4 against float64 on the kernel's own bf16 inputs: products of
bf16 values are exact in fp32, a dot product of unit rows accumulates at most K 2^-24 = 4.6e-5 at K = 768, the maximum selects among
values perturbed by at most that, and the mean over up to T rows adds T 2^-24 relative (8.2e-5 at T = 1369 in the worst case, far less on
average).  Planted maxima sit at the first and the last valid column and in the last partial tile, and a planted row on a masked column
must not be seen: a mis-masked tail moves the answer by about 1 / (valid rows), far above the tolerance."""
import functools
import io

import numpy as np
import pytest
import torch

import match_dets_case as C
from unopose_amd import match_dets as M
from unopose_amd.provider import Window

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- patch_valid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_size", [56, 70])
def test_patch_valid_equals_the_numpy_rule(img_size):
    from unopose_amd import ops

    masks, wins = [], []
    for s in (2, 14, 15, 56):
        for m in C.validity_masks(s, img_size) + (C.validity_masks(s, s) if s == 56 and img_size == 56 else []):
            masks.append(m)
            wins.append((0, s, 0, s))
    packed = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks]).astype(np.uint8)).to(DEV)
    got = ops.patch_valid(packed, wins, img_size).cpu().numpy()
    want = np.stack([M.patch_valid_host(m, img_size) for m in masks])
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert want.any() and not want.all()


@functools.lru_cache(maxsize=None)
def mask_case(N, H, W, n_cat):
    """N masks of an (H, W) image in clusters that overlap, one of them empty (the second, when there is one), with scores that tie."""
    rs = np.random.RandomState(N * 1000 + H + n_cat)
    yy, xx = np.mgrid[:H, :W]
    centres = rs.rand(4, 2) * [H, W]
    masks = np.zeros((N, H, W), bool)
    for n in range(N):
        cy, cx = centres[n % 4] + rs.randn(2) * 2.5
        masks[n] = ((yy - cy) / (8 + 3 * rs.rand())) ** 2 + ((xx - cx) / (11 + 3 * rs.rand())) ** 2 <= 1.0
    if N > 1:
        masks[1] = False
    masks[0, -1, -1] = True  # the last pixel of the image: the last bit of the last word
    category = (rs.randint(0, n_cat, size=N) * 3 + 2).astype(np.int32)
    score = np.round(rs.rand(N), 1)
    return masks, category, score


@pytest.mark.parametrize("n_cat", [1, 3])
@pytest.mark.parametrize("H,W", [(96, 128), (95, 127)])
@pytest.mark.parametrize("N", [1, 2, 65])
def test_mask_nms_equals_the_numpy_rule(N, H, W, n_cat):
    from unopose_amd import ops

    masks, category, score = mask_case(N, H, W, n_cat)
    dev_masks = torch.from_numpy(masks.astype(np.uint8)).to(DEV)
    for iou, cap in ((0.5, 0), (0.3, 2), (0.0, 0)):
        want = M.nms_host(masks, category, score, iou, cap)
        got = ops.mask_nms(dev_masks, torch.from_numpy(category).to(DEV), torch.from_numpy(score).to(DEV), iou, cap)
        for g, w, what in zip(got, want, ("keep", "area", "inter")):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), w.astype(np.int64)), (what, iou, cap)
    if N == 65:
        keep = M.nms_host(masks, category, score, 0.5, 0)[0]
        assert 0 < keep.sum() < N and keep[64] in (0, 1)  # something is suppressed, something stays, past the 64th proposal too
    again = ops.mask_nms(dev_masks.bool(), torch.from_numpy(category).to(DEV), torch.from_numpy(score.astype(np.float32)).to(DEV), 0.5, 0)[0]
    assert np.array_equal(again.cpu().numpy(), M.nms_host(masks, category, score.astype(np.float32), 0.5, 0)[0])


def test_window_masks_feed_patch_valid():
    """The layout `ops.window_masks` writes is the one `ops.patch_valid` reads: decoded masks -> windows -> validity, as the run does."""
    from unopose_amd import ops

    masks, _, _ = mask_case(65, 95, 127, 3)
    idx = [n for n in range(len(masks)) if masks[n].sum() > 8]
    wins = [Window.around(masks[n]) for n in idx]
    packed, _ = ops.window_masks(torch.from_numpy(masks.astype(np.uint8)).to(DEV), wins, idx)
    got = ops.patch_valid(packed, wins, 56).cpu().numpy()
    want = np.stack([M.patch_valid_host(w.crop(masks[n]), 56) for w, n in zip(wins, idx)])
    assert np.array_equal(got, want) and want.any()


# ---- token_unit_rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 768])
def test_token_unit_rows_against_float64(D, dtype):
    from unopose_amd import ops

    g = torch.Generator().manual_seed(D)
    x = torch.randn(3, 21, D, generator=g) * torch.logspace(-3, 3, 21)[None, :, None]
    x[0, 1] = 0.0
    x[1, 2] *= 1e4 / x[1, 2].norm()
    x = x.to(dtype)
    got = ops.token_unit_rows(x.to(DEV))
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    got = got.double().cpu()
    x64 = x.double()
    n = x64.norm(dim=2, keepdim=True)
    want = torch.where(n > 0, x64 / n.clamp_min(1e-300), torch.zeros_like(x64))
    assert abs(float(n[1, 2]) - 1e4) < 40 and float(n[0, 1]) == 0.0
    assert torch.equal(got[0, 1], torch.zeros(D, dtype=torch.float64))
    err = (got - want).abs()
    print(f"token_unit_rows D={D} {dtype}: worst relative error {float((err / want.abs().clamp_min(1e-30)).max()):.3e}")
    assert bool((err <= 2.0 ** -8 * want.abs()).all())
    assert float((got.norm(dim=2)[n[..., 0] > 0] - 1).abs().max()) < 2.0 ** -8


# ---- patch_match_score ----------------------------------------------------------------------------------------------------------------
def _pattern(name, T, rs):
    v = np.zeros(T, np.uint8)
    if name == "all":
        v[:] = 1
    elif name == "one":
        v[rs.randint(T)] = 1
    elif name == "half":
        v[:] = rs.rand(T) < 0.5
        v[3] = 0  # at least one masked column to plant a decoy on
        v[4 + rs.randint(T - 4)] = 1  # and at least one valid one
    return v


@functools.lru_cache(maxsize=None)
def match_case(T, P, O, D):
    """Unit bf16 rows and validities on the device, with planted partners, and the float64 answer (computed once, on the device)."""
    rs = np.random.RandomState(T * 31 + P * 7 + O * 3 + D)
    g = torch.Generator().manual_seed(T * 31 + P * 7 + O * 3 + D)
    q = torch.nn.functional.normalize(torch.randn(P, T, D, generator=g), dim=2)
    r = torch.nn.functional.normalize(torch.randn(O, T, D, generator=g), dim=2)
    qv = np.stack([_pattern(("half", "all", "one", "none", "half")[p % 5], T, rs) for p in range(P)])
    rv = np.stack([_pattern(("half", "all", "none", "one", "half")[o % 5], T, rs) for o in range(O)])
    # proposal 0's first and last valid patch find their twins at the FIRST and the LAST valid column of object 0 (T = 25: inside the partial
    # tile when it is valid there), and a masked column of object 0 carries a decoy twin of another valid patch
    qi, rj = np.flatnonzero(qv[0]), np.flatnonzero(rv[0])
    r[0, rj[0]] = q[0, qi[0]]
    r[0, rj[-1]] = q[0, qi[-1]]
    masked = np.flatnonzero(rv[0] == 0)
    if len(masked) and len(qi) > 2:
        r[0, masked[-1]] = q[0, qi[1]]
    if P > 1:  # the last column of all (also in the partial tile) for a fully valid proposal against a fully valid object
        rv[O - 1 if O > 1 else 0, T - 1] = 1
        r[O - 1 if O > 1 else 0, T - 1] = q[1, T - 1]
    q, r = q.bfloat16().to(DEV), r.bfloat16().to(DEV)
    qv_d, rv_d = torch.from_numpy(qv).to(DEV), torch.from_numpy(rv).to(DEV)
    prod = torch.einsum("ptd,osd->pots", q.double(), r.double())
    prod = prod.masked_fill(~rv_d.bool()[None, :, None, :], -np.inf).amax(dim=3)  # (P, O, T)
    nq = qv_d.sum(dim=1).double()[:, None]
    want = (prod.masked_fill(~qv_d.bool()[:, None, :], 0.0).sum(dim=2) / nq.clamp_min(1)).nan_to_num(neginf=0.0, posinf=0.0)
    want = torch.where((nq > 0) & (rv_d.sum(dim=1)[None, :] > 0), want, torch.zeros_like(want))
    return q, qv_d, r, rv_d, want.cpu().numpy()


SHAPES = [(T, P, O, D) for T in (16, 25, 256) for P, O in ((1, 1), (3, 2), (37, 5)) for D in (64, 768)] + [(1369, 2, 1, 768)]


@pytest.mark.parametrize("T,P,O,D", SHAPES)
def test_patch_match_score_against_float64(T, P, O, D):
    from unopose_amd import ops

    q, qv, r, rv, want = match_case(T, P, O, D)
    got = ops.patch_match_score(q, qv, r, rv)
    again = ops.patch_match_score(q, qv, r, rv)
    assert got.dtype == torch.float32 and tuple(got.shape) == (P, O)
    assert torch.equal(got, again)  # one reduction order, no atomics
    got = got.double().cpu().numpy()
    err = np.abs(got - want)
    print(f"patch_match_score T={T} P={P} O={O} D={D}: worst error {err.max():.3e}, scores {want.min():.4f} .. {want.max():.4f}")
    dead = (qv.sum(dim=1).cpu().numpy()[:, None] == 0) | (rv.sum(dim=1).cpu().numpy()[None, :] == 0)
    assert np.array_equal(got[dead], np.zeros(int(dead.sum())))
    assert err.max() <= 1e-4
    sem = ops.class_cosine(q[:, 0].contiguous(), r[:, 0].contiguous()).double().cpu().numpy()
    assert np.abs(sem - (q[:, 0].double() @ r[:, 0].double().T).cpu().numpy()).max() <= 1e-4


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from unopose_amd import ops

    q, qv, r, rv, _ = match_case(16, 1, 1, 64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.patch_match_score(q.cpu(), qv, r, rv)
    with pytest.raises(RuntimeError):
        ops.patch_match_score(q.float(), qv, r, rv)
    with pytest.raises(ValueError):
        ops.patch_match_score(q[:, :, :48].contiguous(), qv, r[:, :, :48].contiguous(), rv)  # D % 32
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.token_unit_rows(torch.zeros(1, 2, 32))
    with pytest.raises(ValueError):
        ops.patch_valid(torch.zeros(12, dtype=torch.uint8, device=DEV), [(0, 3, 0, 4)], 56)  # not square
    with pytest.raises(ValueError):
        ops.patch_valid(torch.zeros(9, dtype=torch.uint8, device=DEV), [(0, 3, 0, 3)], 60)
    with pytest.raises(RuntimeError):
        ops.mask_nms(torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, device=DEV))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
class _SharedTokens:
    """One ViT pass per distinct crop batch: the device route and the host route then score the same tokens."""

    def __init__(self, fn):
        self.fn, self.memo = fn, {}

    def __call__(self, crops):
        key = crops.detach().cpu().numpy().tobytes()
        if key not in self.memo:
            self.memo[key] = self.fn(crops)
        return self.memo[key]


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """Both routes over the extended bop_synth dataset, once: {route: (entries, records, counts)}."""
    from unopose_amd.model.modules import ViT

    root = str(tmp_path_factory.mktemp("match_dets_gpu"))
    cfg, _, props = C.build(root)
    torch.manual_seed(0)
    vit = ViT(768, 12, 12, 14, cfg["img_size"])
    with torch.no_grad():
        for p in (vit.cls_token, vit.reg_token, vit.pos_embed):
            p.normal_(std=0.5)
    tokens = _SharedTokens(M.VitTokens(vit, DEV, bf16=True))
    out = {}
    for route, device in (("device", DEV), ("host", None)):
        m = M.Matcher(root, "ycbv", cfg["ref_targets_name"], tokens, img_size=cfg["img_size"], min_points=cfg["minimum_n_point"], device=device,
                      out=io.StringIO())
        entries, records = m.run(props)
        out[route] = (entries, records, dict(m.counts))
    return out


def test_device_route_agrees_with_the_host_route(routes):
    (dev_entries, dev, dev_counts), (host_entries, host, host_counts) = routes["device"], routes["host"]
    assert set(dev) == set(host) == {(48, 1), (48, 2), (48, C.SELF_IMAGE)}
    assert {k: v for k, v in dev_counts.items() if k != "kept"} == {k: v for k, v in host_counts.items() if k != "kept"}
    assert host_counts["proposals"] == 10 and host_counts["dropped"] == 1 and host_counts["skipped_images"] == 1
    compared = []
    for key in sorted(host):
        d, h = dev[key], host[key]
        assert d["slots"] == h["slots"] and d["obj_ids"] == h["obj_ids"]
        for name in ("s_sem", "s_appe", "score"):
            diff = float(np.abs(d[name] - h[name]).max())
            print(f"image {key}: {name} device - host {diff:.3e}; host values {h[name].min():.4f} .. {h[name].max():.4f}")
            assert diff <= 1e-4
        top = np.sort(h["score"], axis=1)
        gap = top[:, -1] - top[:, -2] if top.shape[1] > 1 else np.full(len(top), np.inf)
        print(f"image {key}: top-two gaps of the labels {np.array2string(gap, precision=5)}")
        clear = gap > 2e-4
        assert np.array_equal(d["category"][clear], h["category"][clear])
        # the walk order is by score: two proposals within 2e-4 of each other may legitimately change places between the routes
        best = np.sort(h["best"])
        near_tie = (~clear).any() or (len(best) > 1 and float(np.diff(best).min()) <= 2e-4)
        if not near_tie:
            assert np.array_equal(d["keep"], h["keep"])
            compared.append(key)
    assert (48, C.SELF_IMAGE) in compared
    print(f"kept sets compared for {compared}; {len(dev_entries)} device and {len(host_entries)} host detections")
    if len(compared) == len(host):
        strip = lambda es: [{k: v for k, v in e.items() if k != "score"} for e in es]  # noqa: E731
        assert strip(dev_entries) == strip(host_entries)


def test_a_view_matched_against_itself_scores_one(routes):
    for route in ("device", "host"):
        rec = routes[route][1][(48, C.SELF_IMAGE)]
        s_sem, s_appe = float(rec["s_sem"][0, 0]), float(rec["s_appe"][0, 0])
        print(f"{route}: self reference s_sem {s_sem:.6f}, s_appe {s_appe:.6f}")
        assert rec["slots"] == [0] and rec["category"].tolist() == [2] and rec["keep"].tolist() == [1]
        assert abs(s_sem - 1.0) <= 1e-3 and abs(s_appe - 1.0) <= 1e-3
