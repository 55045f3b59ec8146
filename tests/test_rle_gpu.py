"""GPU: the run-length kernels (csrc/rle.hip, ops/rle.py) against the host functions they restate: `provider.rle_decode` /
`provider.rle_counts_from_string` for the decode, `provider.rle_encode` (= the toolkit's `binary_mask_to_rle`, tests/test_coco_gt_cpu.py)
plus numpy's area and box for the encode, `Window.crop` plus row sums for the window crops.  Everything is integers: held to equality.
The sizes hold an odd one, single rows and columns, more than one workgroup of every kernel (4096 output pixels in the fill, 256 counts
in the parse, 64 columns and 64 rows in the compaction), and at 64 x 65 a checkerboard of 4160 runs, which is past the 4096 run starts
the fill stages in LDS."""
import functools

import numpy as np
import pytest
import torch

import coco_gt_case
from unopose_amd import provider as P

pytestmark = pytest.mark.gpu

SIZES = [(24, 36), (23, 35), (1, 4), (5, 1), (64, 65)]


def _ellipse(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y - 0.45 * H) / max(0.4 * H, 0.6)) ** 2 + ((x - 0.55 * W) / max(0.35 * W, 0.6)) ** 2 <= 1.0


@functools.lru_cache(maxsize=None)
def case(H, W):
    """-> (segs, host masks): per mask its list form and, from the second on alternately, its string form, mixed in one list."""
    rs, n = np.random.RandomState(H * 100 + W), H * W
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[-1] = True, True
    canonical = [np.zeros((H, W), bool), np.ones((H, W), bool), first.reshape((H, W), order="F"), last.reshape((H, W), order="F"),
                 (np.arange(n) & 1).astype(bool).reshape((H, W), order="F"), rs.rand(H, W) < 0.5, rs.rand(H, W) < 0.02, _ellipse(H, W)]
    lists = [P.rle_encode(m)["counts"] for m in canonical]
    assert lists[0] == [n] and lists[1] == [0, n] and lists[4] == [1] * n
    lists.append([1, 0, 0, 1, 0, 1, n - 3])  # zero-length runs mid-stream
    lists.append([1, 2])  # short of H * W
    segs = []
    for i, c in enumerate(lists):
        segs.append(dict(size=[H, W], counts=list(c)))
        text = P.rle_counts_to_string(c)
        segs.append(dict(size=[H, W], counts=text if i % 2 else text.encode()))
    want = np.stack([P.rle_decode(s) for s in segs])
    assert all(np.array_equal(want[2 * i], m) and np.array_equal(want[2 * i + 1], m) for i, m in enumerate(canonical))
    return segs, want


def depth_with_holes(H, W, seed=1):
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.3, 2.0, size=(H, W))
    depth[rs.rand(H, W) < 0.3] = 0.0
    depth.flat[rs.randint(0, H * W)] = -1.0
    depth.flat[rs.randint(0, H * W)] = np.nan
    return depth


def want_stats(masks):
    out = np.zeros((len(masks), 6), np.int32)
    for d, m in enumerate(masks):
        ys, xs = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
        out[d, :5] = (m.sum(), ys[0], ys[-1] + 1, xs[0], xs[-1] + 1) if m.any() else (0, m.shape[0], 0, m.shape[1], 0)
    return out


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


@pytest.mark.parametrize("H,W", SIZES)
def test_decode_equals_the_host(H, W):
    from unopose_amd import ops

    segs, want = case(H, W)
    masks, stats = ops.rle_decode(segs, "cuda")
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == want.shape and stats.dtype == torch.int32
    assert np.array_equal(masks.cpu().numpy(), want)
    assert np.array_equal(stats.cpu().numpy(), want_stats(want))
    depth = depth_with_holes(H, W)
    valid = np.logical_and(want > 0, depth > 0)
    for part in (slice(0, 12), slice(5, 6), slice(14, 15)):  # D = 12, and D = 1 as a string and as a list
        masks, stats, host = ops.rle_decode(segs[part], "cuda", depth=torch.from_numpy(depth).cuda(), with_host_stats=True)
        assert np.array_equal(masks.cpu().numpy(), valid[part].astype(np.uint8))
        assert np.array_equal(stats.cpu().numpy(), want_stats(valid[part])) and np.array_equal(host, stats.cpu().numpy())


def test_decode_equals_the_toolkits_recorded_masks():
    from unopose_amd import ops

    fx = coco_gt_case.fixture()
    segs = [dict(size=e["size"], counts=e["counts"]) for e in fx["decoded"]]
    want = np.stack([np.array([[c == "1" for c in row] for row in e["rows"]]) for e in fx["decoded"]])
    masks, _ = ops.rle_decode(segs, "cuda")
    assert len(segs) == 7 and np.array_equal(masks.cpu().numpy(), want.astype(np.uint8))
    counts, area, bbox = ops.rle_encode(masks)
    anns = [a for sid in fx["coco"]["modal"] for a in fx["coco"]["modal"][sid]["annotations"]]
    for e, c, n, b, a in zip(fx["decoded"], counts, area, bbox, anns):
        assert c.tolist() == e["counts"] and int(n) == a["area"] and b == a["bbox"]


@pytest.mark.parametrize("H,W", SIZES)
def test_encode_equals_the_host_and_inverts_the_decode(H, W):
    from unopose_amd import ops

    segs, want = case(H, W)
    masks, _ = ops.rle_decode(segs, "cuda")
    for dev_masks, host_masks in ((masks, want), (masks[3:4].clone(), want[3:4]), ((masks[:12] * 7).contiguous(), want[:12]),
                                  (masks[4:16].bool(), want[4:16])):
        counts, area, bbox = ops.rle_encode(dev_masks)
        stats = want_stats(host_masks)
        for d, m in enumerate(host_masks):
            assert counts[d].dtype == np.int32 and counts[d].tolist() == P.rle_encode(m)["counts"], d
            assert int(area[d]) == int(m.sum())
            n, y0, y1, x0, x1 = (int(v) for v in stats[d, :5])
            assert bbox[d] == ([x0, y0, x1 - x0, y1 - y0] if n else None)
    counts, _, _ = ops.rle_encode(masks)
    for i in range(8):  # the canonical lists come back as they went in, from the list and from the string
        assert counts[2 * i].tolist() == segs[2 * i]["counts"] == counts[2 * i + 1].tolist()


@pytest.mark.parametrize("H,W", [(24, 36), (23, 35), (64, 65)])
def test_window_masks_and_plan_from_device(H, W):
    from unopose_amd import ops

    segs, want = case(H, W)
    depth = depth_with_holes(H, W, seed=2)
    valid = np.logical_and(want > 0, depth > 0)
    masks, stats = ops.rle_decode(segs, "cuda", depth=torch.from_numpy(depth).cuda())
    stats = stats.cpu().numpy()
    index = [d for d in range(len(valid)) if valid[d].sum() > 1]
    wins = [P.Window.around(valid[d]) for d in index]
    for d, w in zip(index, wins):
        assert P.Window.from_extents((H, W), *stats[d, 1:5]).as_list() == w.as_list()
    spans = [(valid[d].any(axis=0).sum(), valid[d].any(axis=1).sum()) for d in index]
    assert any(max(s) > min(H, W) for s in spans), "a box longer than the shorter image side"
    wins.append(P.Window(0, 1, W - 1, W))  # one pixel, of the first mask again
    index.append(index[0])
    packed, rows = ops.window_masks(masks, wins, index)
    crops = [w.crop(valid[d]) for d, w in zip(index, wins)]
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([c.reshape(-1) for c in crops]).astype(np.uint8))
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), np.concatenate([c.sum(axis=1) for c in crops]))
    keep = [k for k, c in enumerate(crops) if c.any()]
    packed, rows = ops.window_masks(masks, [wins[k] for k in keep], [index[k] for k in keep])
    a = ops.PrepPlan((H, W), [wins[k] for k in keep], [crops[k] for k in keep], 8, "cuda")
    for row_counts in (rows, rows.cpu().numpy()):
        b = ops.PrepPlan.from_device((H, W), [wins[k] for k in keep], packed, row_counts, 8, "cuda")
        for name in ("desc", "row_base", "taps", "masks"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert b.masks.data_ptr() == packed.data_ptr()  # kept, not copied
        assert (a.n_points, a.n_rows, a.D, a.S, a.H, a.W) == (b.n_points, b.n_rows, b.D, b.S, b.H, b.W)
        for name in ("h", "w", "n", "pt_off"):
            assert np.array_equal(getattr(a, name), getattr(b, name))
    with pytest.raises(ValueError, match="empty mask"):
        ops.PrepPlan.from_device((H, W), wins[:1], packed[:wins[0].side ** 2], np.zeros(wins[0].side, np.int32), 8, "cuda")
    with pytest.raises(ValueError):
        ops.window_masks(masks, [P.Window(0, H + 1, 0, 1)], [0])
    with pytest.raises(ValueError):
        ops.window_masks(masks, wins[:1], [len(valid)])


def test_outputs_fully_written_and_guards_untouched():
    from unopose_amd import ops

    H, W = 23, 35
    segs, want = case(H, W)
    D = len(segs)
    mbuf, masks = _guarded((D, H, W), torch.uint8, 9)
    sbuf, stats = _guarded((D, 6), torch.int32, -7)
    ops.rle_decode(segs, "cuda", out=(masks, stats))
    wins = [P.Window(0, 23, 3, 26), P.Window(5, 9, 30, 35), P.Window(22, 23, 0, 35)]
    pbuf, packed = _guarded((sum((w.y1 - w.y0) * (w.x1 - w.x0) for w in wins),), torch.uint8, 9)
    rbuf, rows = _guarded((sum(w.y1 - w.y0 for w in wins),), torch.int32, -7)
    ops.window_masks(masks, wins, [5, 10, 2], out=(packed, rows))
    total = sum(len(P.rle_encode(m)["counts"]) for m in want)
    cbuf, flat = _guarded((total,), torch.int32, -7)
    counts, _, _ = ops.rle_encode(masks, out=flat)
    torch.cuda.synchronize()
    for buf, fill in ((mbuf, 9), (sbuf, -7), (pbuf, 9), (rbuf, -7), (cbuf, -7)):
        assert bool((buf[-64:] == fill).all())
    assert np.array_equal(masks.cpu().numpy(), want) and int(masks.max()) == 1  # every byte written: no 9 left
    assert np.array_equal(stats.cpu().numpy(), want_stats(want))
    crops = [w.crop(want[d]) for w, d in zip(wins, [5, 10, 2])]
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([c.reshape(-1) for c in crops]))
    assert np.array_equal(rows.cpu().numpy(), np.concatenate([c.sum(axis=1) for c in crops]))
    assert np.concatenate(counts).tolist() == flat.cpu().tolist() == [c for m in want for c in P.rle_encode(m)["counts"]]


def test_bad_counts_raise_with_guards_untouched():
    from unopose_amd import ops

    H, W = 24, 36
    good = dict(size=[H, W], counts=[10, 20])
    negative = dict(size=[H, W], counts=P.rle_counts_to_string([5, 3, -2, 4]))
    assert P.rle_counts_from_string(negative["counts"]) == [5, 3, -2, 4]
    by_delta = dict(size=[H, W], counts=P.rle_counts_to_string([5, 3, 2, 1])[:3] + P.rle_counts_to_string([0, 0, 0, -4])[3:])  # 3 + (-4)
    assert P.rle_counts_from_string(by_delta["counts"]) == [5, 3, 2, -1]
    for bad, what in ((negative, "negative"), (by_delta, "negative"), (dict(size=[H, W], counts=[0, H * W + 1]), "summing above"),
                      (dict(size=[H, W], counts=[H * W, 1]), "summing above"), (dict(size=[H, W], counts=[3, -1, 5]), "negative"),
                      (dict(size=[H, W], counts=P.rle_counts_to_string([400, 400, 400])), "summing above"),
                      (dict(size=[H, W], counts=[2 ** 40, 1]), "summing above")):
        mbuf, masks = _guarded((3, H, W), torch.uint8, 9)
        sbuf, stats = _guarded((3, 6), torch.int32, -7)
        with pytest.raises(ValueError, match=f"mask 1: .*{what}"):
            ops.rle_decode([good, bad, good], "cuda", out=(masks, stats))
        torch.cuda.synchronize()
        assert bool((mbuf[-64:] == 9).all()) and bool((sbuf[-64:] == -7).all())
        assert np.array_equal(masks[0].cpu().numpy(), P.rle_decode(good)) and int(masks.max()) <= 1  # the others are decoded, all bytes written


def test_real_size_call():
    from unopose_amd import ops

    H, W = 480, 640
    rs = np.random.RandomState(12)
    y, x = np.mgrid[:H, :W]
    segs = []
    for d in range(12):
        cy, cx, ry, rx = rs.uniform(60, H - 60), rs.uniform(60, W - 60), rs.uniform(20, 200), rs.uniform(20, 200)
        blob = (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0) ^ (rs.rand(H, W) < (0.02 if d % 3 else 0.0))  # a noisy rim and interior
        seg = P.rle_encode(blob)
        segs.append(seg if d % 2 else dict(size=seg["size"], counts=P.rle_counts_to_string(seg["counts"])))
    assert max(len(P.rle_encode(P.rle_decode(s))["counts"]) for s in segs) > 4096 > min(len(P.rle_encode(P.rle_decode(s))["counts"]) for s in segs)
    depth = depth_with_holes(H, W, seed=3)
    valid = np.stack([np.logical_and(P.rle_decode(s) > 0, depth > 0) for s in segs])
    masks, stats = ops.rle_decode(segs, "cuda", depth=torch.from_numpy(depth).cuda())
    assert np.array_equal(masks.cpu().numpy(), valid.astype(np.uint8)) and np.array_equal(stats.cpu().numpy(), want_stats(valid))
    counts, area, bbox = ops.rle_encode(masks)
    for d, m in enumerate(valid):
        assert counts[d].tolist() == P.rle_encode(m)["counts"] and int(area[d]) == int(m.sum())
        assert bbox[d] == [int(stats[d, 3]), int(stats[d, 1]), int(stats[d, 4] - stats[d, 3]), int(stats[d, 2] - stats[d, 1])]


def test_cpu_tensors_raise():
    from unopose_amd import ops

    seg = dict(size=[4, 5], counts=[3, 4])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.rle_decode([seg], "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.rle_decode([seg], "cuda", depth=torch.ones(4, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.rle_encode(torch.zeros(1, 4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.window_masks(torch.zeros(1, 4, 5, dtype=torch.uint8), [(0, 2, 0, 2)])
    masks, _ = ops.rle_decode([seg], "cuda")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.PrepPlan.from_device((4, 5), [(0, 2, 0, 2)], masks.reshape(-1)[:4].cpu(), np.ones(2, np.int32), 8, "cuda")
    with pytest.raises(RuntimeError):
        ops.rle_decode([seg], "cuda", depth=torch.ones(4, 5, device="cuda"))  # float32
    with pytest.raises(ValueError, match="different sizes"):
        ops.rle_decode([seg, dict(size=[5, 4], counts=[3, 4])], "cuda")
