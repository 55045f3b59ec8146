"""Test infrastructure: the float32 numpy mirror of the shaded rasteriser (csrc/raster_shade.hip), operation for operation.  The arithmetic
is `unopose_amd.shade_host.render_shaded` -- the package carries it because `render_train --host` renders with it -- and this module hands
it to the tests next to the mirror it grew from: `flat_reference` is tests/raster_rgb_np.py's `render_rgbd`, which the flat, 1 x, untextured
case must equal byte for byte (tests/test_render_train_cpu.py), so the shared part of the chain is pinned twice."""
import numpy as np

from raster_rgb_np import render_rgbd
from unopose_amd.shade_host import AMBIENT, GREY, NumpyShadedRenderer, render_shaded  # noqa: F401

f32 = np.float32


def flat_reference(verts, faces, R, t, k4, H, W, colors=None, surf_color=GREY, ambient=AMBIENT):
    """The rgb of tests/raster_rgb_np.py for the same view."""
    return render_rgbd(verts, faces, R, t, *k4, H, W, colors=colors, surf_color=surf_color, ambient=ambient)[1]


def render_views(Rs, ts, k4, H, W, dt=f32, **model_and_mode):
    """(P,H,W,3): `render_shaded` for every view."""
    return np.stack([render_shaded(R=R, t=t, fx=k4[0], fy=k4[1], cx=k4[2], cy=k4[3], H=H, W=W, dt=dt, **model_and_mode) for R, t in zip(Rs, ts)])
