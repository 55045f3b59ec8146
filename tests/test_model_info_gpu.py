"""GPU: `models_info.json` on the device (csrc/modelinfo.hip through `ops.pts_extent`, `model_info.compute_models_info(device=...)`,
`write_models_info` and `bop_eval.score_csv(models_info="compute")`) against `model_info.extent_host` and the toolkit's recorded values
(tests/golden/model_info.npz): every value with `==`, equal bits on a second call, sizes and positions about the kernel's tile, object
borders, ties and zeros, pruning on and off, and the entry point's own checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import model_info_case as C
from unopose_amd import bop_eval, model_info

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from unopose_amd.ops import score

    t = score.pts_extent_tile()
    assert t >= 64 and t % 64 == 0
    return t


def _device(points, prune=True):
    from unopose_amd import ops

    lo, size, diameter = ops.pts_extent(points, "cuda", prune=prune)
    assert lo.dtype == size.dtype == diameter.dtype == np.float64 and lo.shape == size.shape == (len(points), 3) and diameter.shape == (len(points),)
    return lo, size, diameter


def _equal_host(points, got, prune=True):
    lo, size, diameter = got
    for k, p in enumerate(points):
        h_lo, h_size, h_d = model_info.extent_host(p, prune=prune)
        assert (lo[k] == h_lo).all() and (size[k] == h_size).all() and diameter[k] == h_d, (k, len(p), diameter[k], h_d)


def _cloud(rs, n, scale=90.0):
    return rs.uniform(-scale, scale, (n, 3)).astype(np.float32).astype(np.float64)


def test_single_objects_about_the_tile_size(T):
    rs = np.random.RandomState(5)
    for V in (1, 2, 3, T - 1, T, T + 1, 2 * T + 5):
        pts = _cloud(rs, V)
        for prune in (True, False):
            got = _device([pts], prune)
            _equal_host([pts], got, prune)
            again = _device([pts], prune)
            assert all((C.bits(a) == C.bits(b)).all() for a, b in zip(got, again)), V  # the same bits from a second call


def test_the_farthest_pair_is_found_wherever_it_sits(T):
    rs = np.random.RandomState(6)
    V = 2 * T + 5
    d = rs.randn(V, 3)
    ball = (d / np.linalg.norm(d, axis=1, keepdims=True) * rs.uniform(0, 1, (V, 1))).astype(np.float32).astype(np.float64)
    far = np.array([[40.0, -3.0, 7.5], [-35.25, 12.0, -20.0]])
    dx, dy, dz = far[0] - far[1]
    planted = float(np.sqrt((dx * dx + dy * dy) + dz * dz))
    for i, j in ((0, V - 1), (T - 1, T), (2 * T + 1, 2 * T + 4), (T + 10, 2 * T - 3), (700 % V, 700 % V + 1)):
        pts = ball.copy()
        pts[i], pts[j] = far[0], far[1]
        for prune in (True, False):
            assert _device([pts], prune)[2][0] == planted, (i, j, prune)
        swapped = ball.copy()
        swapped[i], swapped[j] = far[1], far[0]
        assert _device([swapped], False)[2][0] == planted, (i, j)


def test_objects_in_one_call_keep_to_themselves(T):
    rs = np.random.RandomState(7)
    sizes = [1, T + 3, 2, 2 * T + 1, 7]
    objs = [_cloud(rs, v, 50.0) + 1e4 * k for k, v in enumerate(sizes)]  # a pair across two objects would exceed every true diameter
    for prune in (True, False):
        got = _device(objs, prune)
        _equal_host(objs, got, prune)
        assert got[2].max() < 400.0
        for k, p in enumerate(objs):
            alone = _device([p], prune)
            assert all((C.bits(a[k]) == C.bits(b[0])).all() for a, b in zip(got, alone)), k


def test_ties_zeros_offsets_and_signs_equal_the_toolkit():
    gold = C.golden()
    names = list(gold)
    pts = [gold[n][0] for n in names]
    for prune in (True, False):
        lo, size, diameter = _device(pts, prune)
        for k, n in enumerate(names):
            exp = gold[n][1]
            assert (lo[k] == exp[:3]).all() and (size[k] == exp[3:6]).all() and diameter[k] == exp[6], (n, prune, diameter[k], exp[6])
        for n in ("one", "duplicates"):
            assert C.bits(diameter[names.index(n)]) == 0 and (C.bits(size[names.index(n)]) == 0).all()  # +0.0
    negative = -np.abs(gold["random"][0]) - 3.0
    _equal_host([negative, gold["far"][0]], _device([negative, gold["far"][0]]))
    assert (_device([negative])[0] < 0).all() and (_device([negative])[0] + _device([negative])[1] < 0).all()


def test_pruning_changes_no_bit_on_the_device():
    gold = C.golden()
    pts = [gold[n][0] for n in ("box", "shell", "clusters", "duplicates")]
    on, off = _device(pts, True), _device(pts, False)
    assert all((C.bits(a) == C.bits(b)).all() for a, b in zip(on, off))
    _equal_host(pts, on)


def _raw(pts, offsets, offsets_dev=None, prune=1, M=None):
    """unopose_pts_extent through `_lib.call` on buffers filled with 0x7f bytes -> out (M, 7) on the host."""
    from unopose_amd._lib import call, lib, ptr, stream_ptr

    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    M = len(offsets) - 1 if M is None else M
    n = int(lib().unopose_pts_extent_doubles())
    p_d = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda()
    o_d = torch.from_numpy(offsets if offsets_dev is None else np.ascontiguousarray(offsets_dev, dtype=np.int64)).cuda()
    fill = lambda *shape, dtype: torch.full(shape, 0x7f, dtype=torch.uint8, device="cuda").view(dtype)  # noqa: E731
    out, kept, count = fill(max(M, 1) * n * 8, dtype=torch.float64), fill(p_d.numel() * 8, dtype=torch.float64), fill(max(M, 1) * 8, dtype=torch.int64)
    call("unopose_pts_extent", ptr(p_d), ctypes.c_void_p(offsets.ctypes.data), ptr(o_d), M, prune, ptr(kept), ptr(count), ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1, n), count.cpu().numpy()


def test_the_entry_point_initialises_its_outputs_and_validates_its_table(T):
    rs = np.random.RandomState(8)
    a, b = _cloud(rs, T + 9), _cloud(rs, 5)
    for prune in (1, 0):
        out, count = _raw(np.concatenate([a, b]), [0, len(a), len(a) + len(b)], prune=prune)
        for k, p in enumerate((a, b)):
            lo, size, d = model_info.extent_host(p)
            assert (out[k, :3] == lo).all() and (out[k, 3:6] - out[k, :3] == size).all() and np.sqrt(out[k, 6]) == d
        if prune:
            assert 2 <= count[0] <= len(a) and 2 <= count[1] <= len(b)
    pts = np.zeros((8, 3))
    for offsets, M, text in (([0], 0, "0 objects"), ([0, 3, 3, 8], None, "object 1 is empty"), ([0, 5, 3, 8], None, "offsets decrease at object 1"),
                             ([0, 3, 3 + (1 << 24) + 1], None, "at most 2^24"), ([1, 8], None, "offsets start at 1")):
        with pytest.raises(RuntimeError, match="unopose_pts_extent failed") as e:  # nothing is launched: the table is refused on the host
            _raw(pts, offsets, M=M)
        assert text in str(e.value), (text, str(e.value))
    out, _ = _raw(pts + 2.5, [0, 8])  # the library still works after the refusals
    assert out[0].tolist() == [2.5] * 6 + [0.0]


def test_the_wrapper_checks_on_the_host():
    from unopose_amd import ops

    ok = np.zeros((4, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.pts_extent([ok], "cpu")
    bad = ok.copy()
    bad[2, 1] = np.nan
    for pts in ([ok, bad], [np.full((2, 3), 2e150)], [np.zeros((0, 3))], [np.zeros((4, 2))], []):
        with pytest.raises(ValueError, match="pts_extent"):
            ops.pts_extent(pts, "cuda")


def test_write_models_info_writes_the_same_bytes_on_both_routes(tmp_path):
    host, dev = str(tmp_path / "host" / "models_eval"), str(tmp_path / "dev" / "models_eval")
    pts = C.write_model_folder(host)
    C.write_model_folder(dev)
    model_info.write_models_info(host, device=None)
    out = model_info.write_models_info(dev, device="cuda")
    assert open(os.path.join(dev, "models_info.json"), "rb").read() == open(os.path.join(host, "models_info.json"), "rb").read()
    assert sorted(out) == sorted(pts) and out[4]["diameter"] == model_info.extent_host(pts[4])[2]
    argv = ["--data-dir", str(tmp_path), "--dataset", "dev", "--check"]
    assert model_info.main(argv) == 0


def test_score_csv_computes_the_diameters_on_the_device(tmp_path):
    csv, models_eval = C.write_score_dataset(str(tmp_path), symmetric=False)
    model_info.write_models_info(models_eval, device="cuda", force=True)
    kw = dict(device="cuda", device_scoring=True, error_types="mssd,mspd,add")
    from_file = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="file", **kw)
    os.remove(os.path.join(models_eval, "models_info.json"))
    computed = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", models_info="compute", **kw)
    assert sorted(k for k in set(computed) | set(from_file) if computed.get(k) != from_file.get(k)) == ["models_info"]
    assert computed["scorer"] == "device" and 0.0 < computed["AR_MSSD"] < 1.0
    assert json.load(open(os.path.join(os.path.dirname(csv), "scores_bop19.json")))["models_info"] == "compute"
