"""CPU: the float64 reference of the geometric embedding (tests/geo_embed_ref.py) against the oracle and the golden fixture, the teeth of
test_geo_embedding_gpu.py -- every mutant a kernel could turn into leaves the bound on one of that file's own cases, the unmutated float32
restatement of each route stays inside it --, and the conditions on the inputs that the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_embed_ref as G  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def _case(case):
    """(points, module, knn_exact, reference) of one of the GPU test's cases, shared and never changed."""
    route, ob, reduction, regime, kind, B, n = case
    key = (reduction, regime, kind, B, n)
    if key not in _CACHE:
        if len(_CACHE) > 6:
            _CACHE.clear()
        pts = G.make_batch(kind, B, n)
        m = G.make_module(regime, reduction)
        knn, _ = G.knn_exact(pts)
        _CACHE[key] = (pts, m, knn, G.embedding64(pts, m, knn))
    return _CACHE[key]


def _check(case, mutant=None):
    route, ob = case[0], case[1]
    route = "table6" if route == "train" else route
    pts, m, knn, ref = _case(case)
    got = G.emulate(pts, m, knn, route, ob, mutant=mutant)
    return G.within(got, ref, G.bound(pts, m, knn, route, ob, ref=ref))


@torch.no_grad()
def test_reference_equals_the_oracle_on_a_separated_cloud():
    from oracle import unopose_ref as R

    pts = G.make_batch("random", 2, 24, seed=7)
    knn, gap = G.knn_exact(pts)
    assert gap > 1e-3, gap
    for reduction in ("max", "mean"):
        m = G.make_module("trained", reduction)
        sd = {"geo.proj_d.weight": m.proj_d.weight.detach().double(), "geo.proj_d.bias": m.proj_d.bias.detach().double(),
              "geo.proj_a.weight": m.proj_a.weight.detach().double(), "geo.proj_a.bias": m.proj_a.bias.detach().double()}
        cfg = R.Cfg(dict(hidden_dim=256, sigma_d=G.SIGMA_D, sigma_a=G.SIGMA_A, angle_k=3, reduction_a=reduction))
        want = R.geo_embedding(pts.double(), sd, "geo", cfg)
        got = G.embedding64(pts, m, knn)
        # (the oracle's div_term is float32 arithmetic widened by the float64 index, like the module's buffer; its matmul-form distances
        #  lose ~1e-8 off the diagonal and are rounding noise ON it, so the diagonal is compared with the direct form alone)
        eye = torch.eye(24, dtype=torch.bool)
        assert float((got - want).abs().amax(-1)[:, ~eye].max()) < 1e-6
        # the diagonal of the direct form: distance 0, angle 0
        zero = torch.zeros(1, dtype=torch.float64)
        d0 = G._sinus(zero, m.embedding.div_term.double()) @ (m.proj_d.weight.double().t() + m.proj_a.weight.double().t())
        assert float((got[:, eye] - (d0 + m.proj_d.bias.double() + m.proj_a.bias.double())).abs().max()) < 1e-12


def test_reference_reproduces_the_golden_fixture_off_the_diagonal():
    from oracle import unopose_ref as R
    from unopose_amd.model import UNOPose, default_model_cfg

    z = np.load(os.path.join(GOLD, "geo_embedding.npz"))
    pts, want = torch.from_numpy(z["points"]), torch.from_numpy(z["out"])
    model = UNOPose(default_model_cfg())
    model.load_state_dict(R.random_state_dict(R.default_cfg(), seed=0), strict=True)
    m = model.geo_embedding
    knn, gap = G.knn_exact(pts)
    assert gap > G.MIN_GAP
    got = G.embedding64(pts, m, knn)
    eye = torch.eye(pts.shape[1], dtype=torch.bool)
    assert float((got - want.double()).abs().amax(-1)[:, ~eye].max()) <= 1e-4   # (test_oracle_golden.py::test_geo_embedding's tolerance)


def test_knn_mutants_are_told_from_the_truth():
    for kind, B, n in G.KNN_CASES:
        pts = G.make_batch(kind, B, n)
        knn, _ = G.knn_exact(pts)
        assert bool(G.knn_valid(pts, knn).all()), (kind, B, n)
        assert not bool(G.knn_valid(pts, G.knn_mutant(pts, "self_included")).any())
    pts = G.make_batch("lattice", 3, 65)
    knn, gap = G.knn_exact(pts)
    assert gap == 0.0                                      # the lattice has exact ties among the first four candidates
    tie = G.knn_mutant(pts, "tie_second")
    assert bool(G.knn_valid(pts, tie).all()) and not torch.equal(tie, knn)   # valid, and caught by the exact comparison alone
    assert not torch.equal(G.knn_mutant(pts, "self_included"), knn)
    # near-tie flips are legitimate: a list with two equidistant neighbours exchanged stays valid
    assert bool(G.knn_valid(pts, knn[:, :, [0, 2, 1]]).any())


SMALL = [c for c in G.CASES if c[6] <= 33]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(map(str, c)))
def test_unmutated_emulation_stays_inside_the_bound(case):
    assert _check(case)


def _candidates(mutant):
    c = [c for c in G.CASES if c[6] <= 65]
    if mutant == "hi_only":
        return [x for x in c if x[0] == "split" and x[6] <= 33]
    if mutant == "four_for_six":
        return [x for x in c if x[0] in ("table6", "train") and not x[1] and x[6] <= 33]   # (a bf16 result hides it: fp32 results only)
    if mutant == "shift_j":
        return [x for x in c if x[6] == 65]
    if mutant == "mean_for_max":
        return [x for x in c if x[6] <= 33 and x[4] in ("random", "wide", "rings")]
    if mutant == "lds_row_for_global":
        return [x for x in c if x[0].startswith("t") and x[4] in ("rings", "wide") and x[6] <= 33]
    if mutant == "drop_tail":
        return [x for x in c if (x[6] * x[6]) % 32 and x[6] <= 33]
    return [x for x in c if x[6] <= 33]


@pytest.mark.parametrize("mutant", [m for m in G.MUTANTS if m not in ("tie_second", "self_included")])
def test_every_embedding_mutant_leaves_the_bound_on_a_gpu_case(mutant):
    """On EVERY candidate case the unmutated emulation passes and the mutant fails |got - ref| <= bound (drop_tail: through the NaN that
    the test's pre-fill leaves)."""
    cands = _candidates(mutant)
    assert cands
    caught = 0
    for case in cands[:6]:
        assert _check(case), case
        caught += not _check(case, mutant)
    assert caught == len(cands[:6]), (mutant, caught, len(cands[:6]))


def test_random_and_object_clouds_have_no_near_ties():
    """(The embedding cases need no gap: they validate the kernel's own list and use it.)"""
    for kind, B, n in G.KNN_CASES:
        if kind in G.EXACT_KINDS and kind != "lattice":
            _, gap = G.knn_exact(G.make_batch(kind, B, n), ignore_ties=kind == "dup_heavy")
            assert gap > G.MIN_GAP, (kind, B, n, gap)


def test_lattice_distances_are_exact_in_fp32():
    for B, n in sorted({(B, n) for k, B, n in G.KNN_CASES if k == "lattice"} | {(c[5], c[6]) for c in G.CASES if c[4] == "lattice"}):
        p = G.make_batch("lattice", B, n)
        d32 = ((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)
        assert d32.dtype == torch.float32 and torch.equal(d32.double(), G._d2(p))
    p = G.make_batch("line", 3, 65)   # and the line: exact differences, cross products exactly 0
    a = p[:, 1:] - p[:, :1]
    assert float(torch.cross(a, a.flip(1), dim=-1).abs().max()) == 0.0
    assert torch.equal(a.double(), p.double()[:, 1:] - p.double()[:, :1])


def test_backward_clouds_stay_inside_the_table():
    m = G.make_module()
    for kind, _, B, n in G.BACKWARD_CASES:
        x = G.distance_index64(G.make_batch(kind, B, n), m)
        assert float(x.max()) <= G.MAX_BWD_INDEX, (kind, B, n, float(x.max()))
        assert float(x.max()) > G.D_LDS + 8     # and reach well into the rows that only the global branch holds
    x = G.distance_index64(G.make_batch("rings", 2, 130), m)[:, 0, 1:8]
    assert torch.allclose(x, torch.tensor(G.RING_RADII, dtype=torch.float64).expand(2, 7), rtol=1e-6)


def test_an_empty_batch_needs_no_storage():
    """B = 0: the tensors of an empty batch have no storage (null data pointers).  Every entry point returns before it looks at them -- and
    before it touches the device, so this runs without one.  (The pointer checks used to come first and refused the empty batch.)"""
    import ctypes

    from unopose_amd._lib import call

    w = (ctypes.c_float * 8)()
    p = ctypes.cast(w, ctypes.c_void_p)
    call("unopose_geo_embedding", None, 0, 33, p, p, p, p, p, p, 0.2, 3.8, 0, 1, 0, None, None, None)
    call("unopose_geo_embedding_table", None, 0, 33, p, 260, p, 53, p, p, p, 4, 4, 0.2, 3.8, 0, 0, None, None, None)
    call("unopose_geo_embedding_train_forward", None, 0, 33, p, 262, p, 55, p, p, p, 4, 0.2, 3.8, 0, None, None, None, None)
    call("unopose_geo_embedding_train_backward", None, None, 0, 33, 262, 55, 4, 0.2, 3.8, 0, None, None, None, p, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call("unopose_geo_embedding", None, 1, 33, p, p, p, p, p, p, 0.2, 3.8, 0, 1, 0, None, None, None)
