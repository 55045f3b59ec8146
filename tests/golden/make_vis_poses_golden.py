"""Expected visualisations for tests/vis_poses_case.py from the REFERENCE's vendored bop_toolkit_lib:
    python tests/golden/make_vis_poses_golden.py <reference checkout>   ->  tests/golden/vis_poses.npz
The toolkit's own `visualization.vis_object_poses` (third_party/bop_toolkit/bop_toolkit_lib/visualization.py:93-235) runs on the scenes, for
both values of `vis_rgb_resolve_visib`.  The renderer handed to it is the numpy mirror of the colour rasteriser (tests/raster_rgb_np.py: the
toolkit's OpenGL renderers are not needed, both sides compose the same renders).  Four things around the function are replaced, none inside it:
`imageio`, `png` and `cv2` (file formats `inout` imports and this call never uses) are stand-in modules; `write_text_on_image` is the identity
(it needs `font.getsize`, which the installed Pillow no longer has, and text is never compared); `inout.save_im` captures the array instead
of writing a file, and `misc.ensure_dir` creates no folder for it.  Only arrays of the 36 x 24 canvas are stored.  The generator asserts
that the scenes contain every situation the tests rely on, so the fixture cannot quietly lose one."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "third_party", "bop_toolkit")):
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "third_party", "bop_toolkit"))
for absent in ("imageio", "png", "cv2"):
    try:
        __import__(absent)
    except ImportError:
        sys.modules[absent] = types.ModuleType(absent)

from bop_toolkit_lib import inout, visualization  # noqa: E402
from raster_rgb_np import NumpyColorRenderer  # noqa: E402
from vis_poses_case import LAYOUT, add_objects, make_scene, scene_facts  # noqa: E402

W, H = 36, 24


def toolkit_images(scene, resolve_visib):
    saved = {}
    visualization.write_text_on_image = lambda im, *a, **k: im
    inout.save_im = lambda path, im, jpg_quality=95: saved.__setitem__(os.path.basename(path), np.array(im))
    K = scene["K"]
    poses = [dict(obj_id=p["obj_id"], R=p["R"], t=p["t"].reshape(3, 1)) for p in scene["poses"]]
    visualization.vis_object_poses(poses=poses, K=K, renderer=RENDERER, rgb=scene["photo"], depth=scene["depth"], vis_rgb_path="/nowhere/rgb",
                                   vis_depth_diff_path="/nowhere/diff", vis_rgb_resolve_visib=resolve_visib)
    return saved["rgb"], saved["diff"]


def main():
    global RENDERER
    RENDERER = add_objects(NumpyColorRenderer(W, H))
    visualization.misc.ensure_dir = lambda path: None
    out = {}
    for name in LAYOUT:
        scene = make_scene(name, RENDERER.render_object, W, H)
        if name == "main":
            facts = scene_facts(scene)
            assert all(facts.values()), facts
        for resolve in (True, False):
            rgb, diff = toolkit_images(scene, resolve)
            assert rgb.dtype == np.uint8 and rgb.shape == (H, W, 3) and diff.dtype == np.uint8 and diff.shape == (H, W, 3)
            out[f"{name}_rgb_{int(resolve)}"], out[f"{name}_diff_{int(resolve)}"] = rgb, diff
        assert np.array_equal(out[f"{name}_diff_1"], out[f"{name}_diff_0"])
        print(name, "vis_rgb mean", out[f"{name}_rgb_1"].mean(), out[f"{name}_rgb_0"].mean(), "saturated", int((out[f"{name}_rgb_0"] == 255).sum()),
              "diff red", int((out[f"{name}_diff_1"][..., 0] == 255).sum()), "green levels", len(np.unique(out[f"{name}_diff_1"][..., 1])))
    assert not np.array_equal(out["main_rgb_1"], out["main_rgb_0"])
    np.savez_compressed(os.path.join(HERE, "vis_poses.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "vis_poses.npz")), "bytes")


if __name__ == "__main__":
    main()
