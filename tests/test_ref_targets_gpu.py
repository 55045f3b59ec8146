"""GPU: the reference-view search on the device (csrc/reftargets.hip through `ops.ref_select`) against `ref_targets.select_host`: all four
outputs with `np.array_equal`, the nearest trace bit for bit, at sizes about the kernel's query tile, entry tile and slab size, for 1, 2 and 315
symmetries at 20 and 50 degrees, for several slab sizes, on the exact boundary, on ties and on empty inputs -- and the command line, which
writes the same bytes on both routes."""
import os.path as osp

import numpy as np
import pytest

import bop_synth
import ref_targets_case as K
from unopose_amd import ref_targets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sizes():
    from unopose_amd.ops import score

    q_tile, e_tile = score.ref_select_sizes()
    assert q_tile >= 64 and q_tile % 64 == 0 and e_tile >= 1
    return q_tile, e_tile


_HOST = {}


def _host(seed, Q, C, S, max_rot, cross=True, select_seed=0):
    """One host computation per case, shared by the tests that need it and left unchanged."""
    key = (seed, Q, C, S, max_rot, cross, select_seed)
    if key not in _HOST:
        case = K.make_case(seed, Q, C, S)
        _HOST[key] = (case, K.host(case, max_rot, select_seed, cross))
    return _HOST[key]


def _device(case, trace_min, seed=0, cross=True, slab=None):
    from unopose_amd import ops

    got = ops.ref_select(case["Rq"], case["q_scene"], case["q_key"], case["Rc"], case["c_scene"], case["c_key"], case["syms"], trace_min, seed, cross, "cuda", slab=slab)
    Q = len(case["Rq"])
    assert [a.dtype for a in got] == [np.int64, np.int64, np.int64, np.float64] and all(a.shape == (Q,) for a in got)
    return got


def _equal(got, want, what):
    for name, a, b in zip(("pick", "n_eligible", "nearest"), got, want):
        assert np.array_equal(a, b), (what, name, np.flatnonzero(a != b)[:5])
    assert np.array_equal(K.bits(got[3]), K.bits(want[3])), (what, "nearest_trace")


@pytest.mark.parametrize("max_rot", [20.0, 50.0])
@pytest.mark.parametrize("shape", [(1, 1, 1), (70, 257, 1), (70, 257, 2), (33, 130, 315)])
def test_equals_the_host_rule(shape, max_rot):
    case, want = _host(11, *shape, max_rot)
    _equal(_device(case, ref_targets.trace_min_of(max_rot)), want, (shape, max_rot))


@pytest.mark.parametrize("max_rot", [20.0, 50.0])
def test_sizes_about_the_tiles_and_the_slab(sizes, max_rot):
    from unopose_amd.ops import score

    q_tile, e_tile = sizes
    trace_min = ref_targets.trace_min_of(max_rot)
    for Q, C, S, slab in ((q_tile - 1, e_tile - 1, 1, None), (q_tile + 1, e_tile + 1, 1, e_tile + 1),  # one query tile / two; one entry tile / two
                          (q_tile // 2 + 1, 3 * 7 - 1, 2, 7), (5, 3 * 7 + 1, 2, 7),                # a short last slab; a last slab of one candidate
                          (3, 9, 315, 2)):                                                          # a candidate's symmetries across entry tiles
        case, want = _host(12, Q, C, S, max_rot)
        _equal(_device(case, trace_min, slab=slab), want, (Q, C, S, slab))
        auto = score.ref_select_slab(Q, C, S)
        assert 1 <= auto <= C
    # more slabs than a wave of the finish kernel has lanes
    case, want = _host(13, 9, 150, 1, max_rot)
    _equal(_device(case, trace_min, slab=1), want, "150 slabs")


def test_the_result_does_not_depend_on_the_slab_size():
    case, want = _host(11, 70, 257, 2, 50.0, select_seed=99)
    trace_min = ref_targets.trace_min_of(50.0)
    first = _device(case, trace_min, seed=99, slab=5)
    for slab in (64, 257):
        again = _device(case, trace_min, seed=99, slab=slab)
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and np.array_equal(K.bits(first[3]), K.bits(again[3]))
    _equal(first, want, "slab 5")
    _equal(_device(case, trace_min, seed=99), _device(case, trace_min, seed=99), "second call")


def test_same_scene_rule_and_seeds():
    case, want = _host(14, 40, 90, 2, 50.0, cross=False, select_seed=(1 << 64) - 1)
    _equal(_device(case, ref_targets.trace_min_of(50.0), seed=(1 << 64) - 1, cross=False), want, "same scene, largest seed")
    own = dict(case, Rc=np.concatenate([case["Rq"][:1], case["Rc"]]), c_scene=np.concatenate([case["q_scene"][:1], case["c_scene"]]),
               c_key=np.concatenate([case["q_key"][:1], case["c_key"]]))
    for cross in (False, True):
        _equal(_device(own, 3.0, cross=cross), K.host(own, 0.0, 0, cross), ("the view itself", cross))
    got = _device(own, -1.0, cross=False)
    assert got[1][0] == 90 and got[1][1:].tolist() == [91] * 39 and got[0][0] != 0 and got[2][0] != 0


def test_the_boundary_pair():
    case = K.make_case(5, 3, 4, 315)
    best = ref_targets.best_traces(case["Rq"], case["Rc"], case["syms"])
    one = dict(case, Rq=case["Rq"][1:2], q_scene=np.array([0]), q_key=case["q_key"][1:2], Rc=case["Rc"][2:3], c_scene=np.array([1]), c_key=case["c_key"][2:3])
    at, above = _device(one, float(best[1, 2])), _device(one, float(np.nextafter(best[1, 2], np.inf)))
    assert at[0].tolist() == [0] and at[1].tolist() == [1] and above[0].tolist() == [-1] and above[1].tolist() == [0]
    assert above[2].tolist() == [0] and K.bits(above[3])[0] == K.bits(best[1, 2])[0] == K.bits(at[3])[0]
    # every pair of the small case on its own boundary
    for q in range(3):
        got = _device(case, float(best[q].max()), cross=False)
        assert got[1][q] == 1 and got[0][q] == got[2][q] == int(np.argmax(best[q]))


def test_ties_and_cases_without_a_view():
    case = K.make_case(4, 6, 20, 1)
    dup = dict(case, Rc=np.repeat(case["Rc"][:1], 20, axis=0), c_key=np.repeat(case["c_key"][:1], 20), c_scene=np.full(20, 99, np.int64))
    for slab in (None, 3, 20):  # equal priorities and equal traces inside a slab and across slabs: the lower index
        got = _device(dup, -1.0, slab=slab)
        assert (got[0] == 0).all() and (got[2] == 0).all() and (got[1] == 20).all()
        _equal(got, K.host(dup, 180.0), ("duplicates", slab))
    same = dict(case, c_scene=np.full(20, 7, np.int64), q_scene=np.full(6, 7, np.int64))
    got = _device(same, -1.0, slab=4)
    assert (got[0] == -1).all() and (got[1] == 0).all() and (got[2] == -1).all() and np.isneginf(got[3]).all()
    # a trace of zero leaves as +0.0 whichever zero the sum gave
    turn = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    minus = np.where(np.eye(3) > 0, -0.0, -1.0)  # no rotation: with the identity the hardware's fma makes every product, and the trace, -0.0 (the host's emulated fma +0.0)
    zero = dict(case, syms=K.symmetries(2), Rq=np.stack([turn, minus]), q_scene=np.array([0, 0]), q_key=np.array([1, 2], np.uint64), Rc=np.eye(3)[None],
                c_scene=np.array([1]), c_key=np.array([1 << 32], np.uint64))
    want = ref_targets.select_host(zero["Rq"], zero["q_scene"], zero["q_key"], zero["Rc"], zero["c_scene"], zero["c_key"], zero["syms"], 0.0)
    assert want[3].tolist() == [0.0, 0.0] and not np.signbit(want[3]).any() and want[1].tolist() == [1, 1]
    _equal(_device(zero, 0.0), want, "zero traces")


def test_empty_inputs_and_the_checks_in_front_of_the_launch():
    from unopose_amd import ops

    case = K.make_case(4, 6, 20, 1)
    empty = dict(case, Rc=np.zeros((0, 3, 3)), c_scene=np.zeros(0, np.int64), c_key=np.zeros(0, np.uint64))
    got = _device(empty, 0.0)
    assert got[0].tolist() == [-1] * 6 and got[1].tolist() == [0] * 6 and got[2].tolist() == [-1] * 6 and np.isneginf(got[3]).all()
    none = dict(case, Rq=np.zeros((0, 3, 3)), q_scene=np.zeros(0, np.int64), q_key=np.zeros(0, np.uint64))
    assert [len(a) for a in _device(none, 0.0)] == [0, 0, 0, 0]
    args = lambda c: (c["Rq"], c["q_scene"], c["q_key"], c["Rc"], c["c_scene"], c["c_key"], c["syms"])
    with pytest.raises(ValueError, match="symmetries"):
        ops.ref_select(*args(dict(case, syms=np.zeros((0, 3, 3)))), 0.0)
    with pytest.raises(ValueError, match="finite"):
        ops.ref_select(*args(dict(case, Rq=np.full((6, 3, 3), np.inf))), 0.0)
    with pytest.raises(ValueError, match="trace_min"):
        ops.ref_select(*args(case), float("nan"))
    with pytest.raises(ValueError, match="slab"):
        ops.ref_select(*args(case), 0.0, slab=21)
    with pytest.raises(ValueError, match="candidates"):
        ops.ref_select(*args(dict(case, c_key=case["c_key"][:5])), 0.0)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.ref_select(*args(case), 0.0, device="cpu")


def test_command_line_writes_the_same_bytes_on_both_routes(tmp_path):
    cfg, _ = bop_synth.build(str(tmp_path))
    K.write_gt_info(str(tmp_path))
    argv = ["--data-dir", str(tmp_path), "--dataset", "ycbv", "--all-images", "--seed", "3"]
    for extra in ([], ["--same-scene"], ["--max-rot", "20"]):
        assert ref_targets.main(argv + extra + ["--out", "device.json"] + ["--overwrite"]) == 0
        assert ref_targets.main(argv + extra + ["--host", "--out", "host.json", "--overwrite"]) == 0
        a, b = (open(osp.join(str(tmp_path), "ycbv", n), "rb").read() for n in ("device.json", "host.json"))
        assert a == b and len(a) > 100
