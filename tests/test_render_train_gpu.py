"""GPU: the shaded, textured, supersampled rasteriser (csrc/raster_shade.hip through render.HipShadedRenderer) bit for bit against its numpy
mirror (tests/raster_shade_np.py), tied to the existing renderers where their jobs overlap, and the command `unopose_amd.render_train` against
its --host route.  tests/test_render_train_cpu.py pins the mirror's shared part to tests/raster_rgb_np.py and the sampler and the scene
files to bop_toolkit."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 3


@functools.lru_cache(maxsize=None)
def mirror(W, H, colour, shading, ssaa):
    from raster_shade_np import render_views
    from render_train_case import colour_kwargs, views

    k4, Rs, ts = views(W, H)
    out = render_views(Rs, ts, k4, H, W, shading=shading, ssaa=ssaa, **colour_kwargs(colour))
    out.setflags(write=False)
    return out


def device_render(W, H, colour, shading, ssaa, **kw):
    from render_train_case import colour_kwargs, views
    from unopose_amd.render import HipShadedRenderer

    ren = HipShadedRenderer(W, H, shading=shading, ssaa=ssaa, **kw)
    ren.add_object(3, **colour_kwargs(colour))
    k4, Rs, ts = views(W, H)
    return ren, ren.render_batch(3, Rs, ts, k4)


@pytest.mark.parametrize("colour", ["colors", "surf", "texture"])
@pytest.mark.parametrize("shading", ["phong", "flat"])
@pytest.mark.parametrize("ssaa", [1, 2, 3, 4])
def test_shaded_rasteriser_equals_the_numpy_mirror_bit_for_bit(ssaa, shading, colour):
    """The tricky model of render_train_case (a face behind the camera, a degenerate face and a sliver, a zero-length and an over-long normal,
    two coplanar duplicates at equal depth, texture coordinates 0, 1 and outside) in three views, one cut by the left and upper border."""
    W, H = 40, 32
    want = mirror(W, H, colour, shading, ssaa)
    rgb = device_render(W, H, colour, shading, ssaa)[1].cpu().numpy()
    assert rgb.shape == (P, H, W, 3) and rgb.dtype == np.uint8
    assert np.array_equal(rgb, want)
    drawn = (want > 0).any(axis=3)
    assert drawn[0].sum() > 250 and drawn[1].sum() > 250 and 30 < drawn[2].sum() and drawn[2][0].any() and drawn[2][:, 0].any()
    if colour == "colors":
        assert not ((want[..., 2] > 0) & (want[..., 0] == 0) & (want[..., 1] == 0)).any()  # the blue duplicates never win


@pytest.mark.parametrize("ssaa,shading,colour", [(3, "phong", "texture"), (4, "flat", "colors"), (2, "phong", "surf"), (1, "phong", "colors")])
def test_odd_image_size(ssaa, shading, colour):
    W, H = 37, 29
    assert np.array_equal(device_render(W, H, colour, shading, ssaa)[1].cpu().numpy(), mirror(W, H, colour, shading, ssaa))


@pytest.mark.parametrize("size", [(40, 32), (37, 29)])
@pytest.mark.parametrize("colour", ["colors", "surf"])
def test_flat_1x_equals_the_colour_renderer_and_covers_the_depth_renderers_pixels(size, colour):
    from render_train_case import SURF, colour_kwargs, views
    from unopose_amd.render import HipColorRenderer, HipDepthRenderer

    W, H = size
    kw = colour_kwargs(colour)
    k4, Rs, ts = views(W, H)
    rgb = device_render(W, H, colour, "flat", 1)[1]
    old, plain = HipColorRenderer(W, H), HipDepthRenderer(W, H)
    old.add_object(1, kw["verts"], kw["faces"], colors=kw.get("colors"), surf_color=SURF if colour == "surf" else None)
    plain.add_object(1, kw["verts"], kw["faces"])
    want = old.render_batch(1, Rs, ts, k4)[1]
    assert np.array_equal(rgb.cpu().numpy(), want.cpu().numpy()) and int((want > 0).sum()) > 500
    # full ambient: every covered pixel is lit, so the coverage is the depth renderer's
    depth = plain.render_batch(1, Rs, ts, k4).cpu().numpy()
    for shading in ("phong", "flat"):
        lit = device_render(W, H, "surf", shading, 1, ambient=1.0)[1].cpu().numpy()
        assert np.array_equal((lit > 0).all(axis=3), depth > 0)


def test_chunking_does_not_change_a_byte():
    W, H, ssaa = 40, 32, 3
    whole_ren, whole = device_render(W, H, "texture", "phong", ssaa)
    single_ren, single = device_render(W, H, "texture", "phong", ssaa, chunk_bytes=8 * ssaa * ssaa * W * H)
    tiny_ren, tiny = device_render(W, H, "texture", "phong", ssaa, chunk_bytes=1)
    assert whole_ren.views_per_chunk() >= P and single_ren.views_per_chunk() == 1 and tiny_ren.views_per_chunk() == 1
    assert np.array_equal(whole.cpu().numpy(), mirror(W, H, "texture", "phong", ssaa))
    assert np.array_equal(single.cpu().numpy(), whole.cpu().numpy()) and np.array_equal(tiny.cpu().numpy(), whole.cpu().numpy())


def test_out_argument_and_refusals():
    import torch

    from render_train_case import colour_kwargs, views
    from unopose_amd.render import HipShadedRenderer

    W, H = 40, 32
    k4, Rs, ts = views(W, H)
    ren = HipShadedRenderer(W, H, ssaa=2)
    ren.add_object(1, **colour_kwargs("colors"))
    stack = torch.full((5, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    assert ren.render_batch(1, Rs[:2], ts[:2], k4, out=stack[:2]).data_ptr() == stack.data_ptr()
    ren.render_batch(1, Rs[2:], ts[2:], k4, out=stack[2:3])
    assert np.array_equal(stack[:3].cpu().numpy(), mirror(W, H, "colors", "phong", 2)) and bool((stack[3:] == 9).all())
    assert np.array_equal(ren.render_object(1, Rs[1], ts[1], *k4)["rgb"], mirror(W, H, "colors", "phong", 2)[1])
    on_device = ren.render_batch(1, torch.as_tensor(Rs, dtype=torch.float32).cuda(), torch.as_tensor(ts, dtype=torch.float32).cuda(), k4)
    assert np.array_equal(on_device.cpu().numpy(), mirror(W, H, "colors", "phong", 2))
    for bad in (torch.zeros(3, H, W, 3, device="cuda"),                          # dtype
                torch.zeros(3, H, W + 1, 3, dtype=torch.uint8, device="cuda"),   # shape
                torch.zeros(4, H, W, 3, dtype=torch.uint8, device="cuda"),       # views
                torch.zeros(3, H, W, 6, dtype=torch.uint8, device="cuda")[..., ::2]):  # not contiguous
        with pytest.raises(RuntimeError, match="out must be"):
            ren.render_batch(1, Rs, ts, k4, out=bad)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ren.render_batch(1, Rs, ts, k4, out=torch.zeros(3, H, W, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ren.render_batch(1, torch.as_tensor(Rs), ts, k4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        HipShadedRenderer(W, H, device="cpu").add_object(1, **colour_kwargs("colors"))
    with pytest.raises(ValueError):
        ren.add_object(2, **dict(colour_kwargs("colors"), normals=None))  # Phong without normals
    with pytest.raises(ValueError):
        ren.add_object(2, **dict(colour_kwargs("texture"), surf_color=(1, 1, 1)))
    with pytest.raises(ValueError):
        HipShadedRenderer(W, H, ssaa=5)
    from unopose_amd._lib import call, ptr, stream_ptr

    v, f, n = ren.models[1][:3]
    keys = torch.empty(16 * H * W, dtype=torch.int64, device="cuda")
    Rt, K4 = torch.zeros(1, 12, device="cuda"), torch.ones(1, 4, device="cuda")
    for bad, text in ((dict(ssaa=0), "ssaa"), (dict(ssaa=5), "ssaa"), (dict(P=0), "bad sizes"), (dict(P=65536), "bad sizes"), (dict(normals=None), "needs normals")):
        a = dict(dict(P=1, ssaa=2, normals=ptr(n)), **bad)  # nothing is launched on a refused call
        with pytest.raises(RuntimeError, match="render_shaded: .*" + text):
            call("unopose_render_shaded", ptr(v), v.shape[0], ptr(f), f.shape[0], a["normals"], None, None, None, 0, 0, 0.5, 0.5, 0.5, 0.5, 1, a["ssaa"],
                 ptr(Rt), ptr(K4), a["P"], H, W, ptr(keys), ptr(stack), stream_ptr())
    torch.cuda.synchronize()


def test_render_train_on_the_gpu_writes_the_host_routes_files(tmp_path):
    from render_train_case import RENDER_ARGS, write_dataset
    from unopose_amd import render_train as rt

    write_dataset(str(tmp_path))
    args = ["--data-dir", str(tmp_path), "--dataset", "synth"] + RENDER_ARGS
    assert rt.main(args + ["--out", str(tmp_path / "gpu")]) == 0
    assert rt.main(args + ["--out", str(tmp_path / "host"), "--host"]) == 0
    n = 0
    for folder, _, names in os.walk(tmp_path / "host"):
        for name in names:
            other = os.path.join(str(tmp_path / "gpu"), os.path.relpath(os.path.join(folder, name), str(tmp_path / "host")))
            assert open(os.path.join(folder, name), "rb").read() == open(other, "rb").read(), other
            n += 1
    assert n == 2 * (12 + 12 + 2) and sum(len(names) for _, _, names in os.walk(tmp_path / "gpu")) == n
    assert rt.main(args + ["--out", str(tmp_path / "host"), "--check"]) == 0  # the GPU route checks the host route's files
