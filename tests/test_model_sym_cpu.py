"""CPU: the symmetry search on the host route (unopose_amd/model_sym.py): the specification of the deviation against a brute-force double
loop, the groups of the small polyhedra of tests/model_sym_case.py (tol 0.02, 1024 axes, orders 2 .. 6; the cylinder and the cone run on the
GPU only), the centre rule, the toolkit's reading of the written entries, and the command line with --host."""
import io
import json
import math
import os.path as osp
import sys

import numpy as np
import pytest

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
import model_sym_case as case  # noqa: E402

from unopose_amd import bop_eval, model_sym  # noqa: E402

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden", "model_sym_toolkit.json")


@pytest.fixture(scope="module")
def found():
    """`find_symmetries` on the host for every polyhedron in both poses, computed once."""
    out = {}
    for name in case.POLYHEDRA:
        for pose in (0, 1):
            pts = case.model(name, pose)
            out[name, pose] = (pts, model_sym.find_symmetries(pts, tol=case.TOL, axes=case.AXES, max_order=case.MAX_ORDER))
    return out


def test_specification_against_a_double_loop():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-50.0, 50.0, (37, 3))
    T = np.zeros((6, 4, 4))
    T[:, 3, 3] = 1.0
    T[0, :3, :3] = np.eye(3)
    for k in range(1, 6):
        T[k, :3, :3], T[k, :3, 3] = case.random_rotation(k), rng.uniform(-30.0, 30.0, 3) * (k % 2)
    got = model_sym.sym_deviation_host(pts, T)
    assert got[0] == 0.0
    for k in range(6):
        want = case.brute_deviation(pts, T[k])
        assert abs(got[k] - want) <= 1e-12 * max(1.0, want), (k, got[k], want)
    inv = np.linalg.inv(T)
    inv[:, :3, :3] = T[:, :3, :3].transpose(0, 2, 1)  # the exact transposes; the translations to rounding
    back = model_sym.sym_deviation_host(pts, inv)
    assert np.abs(back - got).max() <= 1e-12 * got.max()
    # an exact pair: a half-turn about z and its inverse (itself) on a cloud the half-turn maps onto itself
    sym = np.concatenate([pts, pts * [-1.0, -1.0, 1.0]])
    half = np.diag([-1.0, -1.0, 1.0, 1.0])[None]
    assert model_sym.sym_deviation_host(sym, half)[0] == 0.0
    # blocks and the bound change no bit of what is kept; what exceeds the bound is +inf
    small = model_sym.sym_deviation_host(pts, T, block=100)
    assert (small == got).all()
    order = np.sort(got)
    bounded = model_sym.sym_deviation_host(pts, T, bound=0.5 * (order[2] + order[3]))
    assert (bounded[got <= order[2]] == got[got <= order[2]]).all() and np.isinf(bounded[got >= order[3]]).all()


def test_inputs_are_checked():
    pts = np.zeros((4, 3))
    with pytest.raises(ValueError, match="sym_deviation"):
        model_sym.sym_deviation_host(pts, np.full((1, 4, 4), np.nan))
    with pytest.raises(ValueError, match="sym_deviation"):
        model_sym.sym_deviation_host(np.full((4, 3), np.inf), np.eye(4)[None])
    with pytest.raises(ValueError, match="sym_deviation"):
        model_sym.sym_deviation_host(pts, np.eye(4)[None], bound=-1.0)
    with pytest.raises(ValueError, match="sym_deviation"):
        model_sym.sym_deviation_host(pts, np.eye(3)[None])


def test_axes_outside_the_checked_range_are_refused():
    assert model_sym.AXES_RANGE == (256, 4096)
    for axes in (1, 64, 255, 4097):
        with pytest.raises(ValueError, match="axes"):
            model_sym.find_symmetries(case.box(40, 60, 90), axes=axes)
    # the thinning radius 4 delta stays under the 36 degrees between two 2-fold axes of the icosahedral group
    assert 4.0 * model_sym.covering_angle(256) < math.radians(36.0)


@pytest.mark.parametrize("axes", [256, 512, 1024, 2048, 4096])
def test_covering_angle_bounds_the_grid(axes):
    grid = model_sym.fibonacci_axes(axes)
    assert np.abs(np.linalg.norm(grid, axis=1) - 1.0).max() < 1e-12 and (grid[:, 2] > 0).all()
    v = np.random.default_rng(0).standard_normal((100000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rim = np.stack([np.cos(np.linspace(0, 2 * math.pi, 20000)), np.sin(np.linspace(0, 2 * math.pi, 20000)), np.zeros(20000)], axis=1)
    parts = [v[k:k + 10000] for k in range(0, len(v), 10000)] + [rim, np.array([[0.0, 0.0, 1.0]])]
    worst = max(np.arccos(np.minimum(1.0, np.abs(part @ grid.T).max(axis=1))).max() for part in parts)
    print(f"axes {axes}: sampled covering angle {worst:.4f} rad, bound {model_sym.covering_angle(axes):.4f}")
    assert worst <= model_sym.covering_angle(axes)


@pytest.mark.parametrize("pose", [0, 1])
@pytest.mark.parametrize("name", case.POLYHEDRA)
def test_groups_of_the_polyhedra(found, name, pose):
    pts, res = found[name, pose]
    assert len(pts) == case.MODELS[name][1]
    assert res["report"]["status"] == "ok"
    order, continuous, d = case.group_facts(res, pts)
    assert (order, continuous) == case.MODELS[name][2:]
    for T, listed in zip(res["symmetries_discrete"], res["report"]["symmetries"]):
        brute = case.brute_deviation(pts, T)
        print(f"{name} pose {pose}: order {listed['order']} deviation / d {brute / d:.3e}")
        assert brute <= case.TOL * d and abs(brute / d - listed["deviation"]) <= 1e-9
    assert len(bop_eval.symmetry_transformations(res)) == order


@pytest.mark.parametrize("name", ["box", "tetrahedron", "sheared_box"])
def test_groups_survive_noise(name):
    """Noise of 0.02 units (2e-4 d) on every coordinate of the posed model: no symmetry is exact, every axis is refined to the smallest step
    and found to about 1e-3 rad; the group is the table's all the same."""
    pts = case.noisy(case.model(name, 1))
    res = model_sym.find_symmetries(pts, tol=case.TOL, axes=case.AXES, max_order=case.MAX_ORDER)
    assert case.noisy_facts(res, pts) == case.MODELS[name][2:]


def test_axis_aligned_model_gets_exact_matrices(found):
    res = found["box", 0][1]
    assert sorted(tuple(np.diag(np.asarray(m).reshape(4, 4))) for m in res["symmetries_discrete"]) == [(-1.0, -1.0, 1.0, 1.0), (-1.0, 1.0, -1.0, 1.0),
                                                                                                     (1.0, -1.0, -1.0, 1.0)]
    assert all(np.count_nonzero(m) == 4 for m in res["symmetries_discrete"])


def test_toolkit_reads_the_entries_as_the_scorer_does(found):
    """tests/golden/model_sym_toolkit.json (tests/golden/make_model_sym_golden.py): entries in the written format and what the toolkit's
    `misc.get_symmetry_transformations` makes of them.  `bop_eval.symmetry_transformations` gives the same list, and so it does for the entries
    found here (same count; the recorded discrete entries are the ones found for these models in their own frame)."""
    golden = json.load(open(GOLDEN))
    assert set(golden) >= {"box", "prism", "cube", "tetrahedron", "cylinder"}
    for name, rec in golden.items():
        mine = bop_eval.symmetry_transformations(rec["entry"])
        assert len(mine) == len(rec["toolkit"]) == rec["count"]
        for a, b in zip(mine, rec["toolkit"]):
            assert np.abs(a["R"] - np.asarray(b["R"]).reshape(3, 3)).max() <= 1e-12 and np.abs(np.reshape(a["t"], 3) - np.reshape(b["t"], 3)).max() <= 1e-9
        if (name, 0) in found:
            fresh = bop_eval.symmetry_transformations(found[name, 0][1])
            assert len(fresh) == rec["count"]
            for a in fresh:
                assert min(np.abs(a["R"] - np.asarray(b["R"]).reshape(3, 3)).max() for b in rec["toolkit"]) <= 1e-6


def test_degenerate_input_gives_an_empty_result():
    flat = np.random.default_rng(1).uniform(-1.0, 1.0, (50, 3)) * [1.0, 1.0, 0.0]
    for pts in (np.eye(3), flat, flat @ case.random_rotation(2).T + 5.0, np.outer(np.arange(9.0), [1.0, 2.0, 3.0])):
        res = model_sym.find_symmetries(pts)
        assert res["symmetries_discrete"] == [] and res["symmetries_continuous"] == [] and res["report"]["status"] == "degenerate"


def _box_mesh(refine):
    """The 40 x 60 x 90 box as 12 triangles; `refine` cuts the two triangles of the face x = +20 into 4^refine each (midpoint subdivision)."""
    s = np.array([20.0, 30.0, 45.0])
    tris = []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for side in (-1.0, 1.0):
            quad = []
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis], p[u], p[v] = side * s[axis], a * s[u], b * s[v]
                quad.append(p)
            face = [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
            for _ in range(refine if (axis == 0 and side > 0) else 0):
                face = [t for a, b, c in face for t in ((a, (a + b) / 2, (a + c) / 2), ((a + b) / 2, b, (b + c) / 2), ((a + c) / 2, (b + c) / 2, c),
                                                        ((a + b) / 2, (b + c) / 2, (a + c) / 2))]
            tris += face
    verts, index = np.unique(np.round(np.array([p for t in tris for p in t]), 9), axis=0, return_inverse=True)
    return verts, index.reshape(-1, 3)


def test_area_centroid_ignores_the_tessellation():
    shift = np.array([31.0, -17.0, 55.0])
    plain, fine = _box_mesh(0), _box_mesh(2)
    assert len(fine[0]) > len(plain[0]) + 10
    for verts, faces in (plain, fine):
        assert np.abs(model_sym.surface_centroid(verts + shift, faces) - shift).max() <= 1e-9
    assert np.abs((fine[0] + shift).mean(axis=0) - shift).max() > 1.0  # the vertex mean follows the finer face
    res = model_sym.find_symmetries(fine[0] + shift, fine[1], axes=256)
    assert np.abs(np.asarray(res["report"]["centre"]) - shift).max() <= 1e-9


def _run(args):
    buf = io.StringIO()
    assert model_sym.main(args, out=buf) == 0
    return buf.getvalue()


def test_command_line_on_the_host(tmp_path):
    from bop_score_case import write_ply

    folder = tmp_path / "own" / "models_eval"
    for o, pts in ((1, case.box(40, 60, 90)), (2, case.sheared_box())):
        write_ply(str(folder / f"obj_{o:06d}.ply"), pts, np.array([[0, 1, 2]]), binary=True, vertex_type="double")
    args = ["--data-dir", str(tmp_path), "--dataset", "own", "--host", "--axes", "512"]
    path = folder / "models_info.json"
    text = _run(args)  # no file yet: computed first
    info = json.load(open(path))
    assert "2 objects" in text
    assert len(info["1"]["symmetries_discrete"]) == 3 and "symmetries_continuous" not in info["1"] and info["1"]["diameter"] > 100.0
    assert not any(k in info["2"] for k in ("symmetries_discrete", "symmetries_continuous"))
    assert open(path).read().startswith('{\n  "1": {"diameter"')
    # an annotated object is left alone without --force
    info["1"]["symmetries_discrete"] = info["1"]["symmetries_discrete"][:1]
    json.dump(info, open(path, "w"))
    assert "left alone" in _run(args)
    assert len(json.load(open(path))["1"]["symmetries_discrete"]) == 1
    # --check writes nothing and prints the stored symmetries' deviations
    before = open(path).read()
    text = _run(args + ["--check"])
    assert open(path).read() == before
    assert "stored group 2  found 4" in text and "stored symmetry 1: deviation / d" in text and f"max(15, 0.1 d) / d {15.0 / info['1']['diameter']:.4f}" in text
    assert "--force" not in text
    # a file all of whose objects are annotated is not written again, whatever its layout
    info["2"]["symmetries_discrete"] = []
    json.dump(info, open(path, "w"), indent=3)
    before = open(path).read()
    assert _run(args).count("left alone") == 2
    assert open(path).read() == before
    _run(args + ["--force", "--obj-ids", "1"])
    assert len(json.load(open(path))["1"]["symmetries_discrete"]) == 3
