"""Point sets and the toolkit's box and diameter for them, from the REFERENCE's vendored bop_toolkit:
    python tests/golden/make_model_info_golden.py <reference checkout>   ->  tests/golden/model_info.npz
Per set the three statements of scripts/calc_model_info.py that form `ref_pt`, `size` and `diameter` -- the script's own lines, read from the
checkout and executed here with `misc.calc_pts_diameter` of bop_toolkit_lib, not restated; the script is Python 2, so `map` is given its
Python 2 meaning (a list).  The file holds `pts_<name>` (float32 where the set is float32-valued, the tests widen it) and `exp_<name>` =
min x, y, z, size x, y, z, diameter as float64.  The generator asserts what the tests rely on in each set."""
import builtins
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "third_party", "bop_toolkit")):
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
sys.path.insert(0, os.path.join(REFERENCE, "third_party", "bop_toolkit"))

from bop_toolkit_lib import misc  # noqa: E402


def point_sets():
    rs = np.random.RandomState(61)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sets = {}
    sets["one"] = np.array([[3.5, -2.25, 7.0]])
    sets["two"] = np.array([[0.1, 0.2, 0.3], [-4.7, 11.3, 2.9]])
    sets["duplicates"] = np.tile(np.array([[12.125, -3.0625, 0.7]]), (5, 1))
    g = np.arange(4.0)
    sets["lattice"] = f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * 7.0 - 9.0)
    sets["random"] = f32(rs.uniform(-80, 120, (300, 3)))
    d = rs.randn(1500, 3)
    sets["shell"] = f32(55.0 * d / np.linalg.norm(d, axis=1, keepdims=True) + np.array([4.0, -6.0, 11.0]))
    u = rs.uniform(-1, 1, (1500, 3))
    u[np.arange(1500), rs.randint(0, 3, 1500)] = rs.choice([-1.0, 1.0], 1500)  # one coordinate on a face
    sets["box"] = f32(u * np.array([60.0, 35.0, 90.0]) + np.array([-5.0, 20.0, 3.0]))
    sets["clusters"] = f32(rs.randn(1500, 3) * 6.0 + np.where(np.arange(1500)[:, None] < 750, 0.0, 1.0) * np.array([300.0, 0.0, 0.0]))
    sets["far"] = 1e6 + rs.randn(300, 3) * 25.0
    return sets


def toolkit_model_info(pts):
    """calc_model_info.py's statements for one model."""
    lines = open(os.path.join(REFERENCE, "third_party", "bop_toolkit", "scripts", "calc_model_info.py")).read().splitlines()
    first = next(i for i, line in enumerate(lines) if "ref_pt = map(" in line)
    last = next(i for i, line in enumerate(lines) if "diameter = misc.calc_pts_diameter" in line)
    scope = dict(model=dict(pts=pts), misc=misc, map=lambda f, it: list(builtins.map(f, it)))
    exec(textwrap.dedent("\n".join(lines[first:last + 1])), scope)
    return np.array(list(scope["ref_pt"]) + list(scope["size"]) + [scope["diameter"]], np.float64)


def main():
    out = {}
    for name, pts in point_sets().items():
        wide = np.asarray(pts, np.float64)
        exp = toolkit_model_info(wide)
        out["pts_" + name], out["exp_" + name] = pts, exp
        print(name, pts.dtype, pts.shape, exp.tolist())
    assert out["exp_one"][6] == 0.0 and out["exp_duplicates"][6] == 0.0 and (out["exp_duplicates"][3:6] == 0.0).all()
    lat = np.asarray(out["pts_lattice"], np.float64)
    d2 = ((lat[:, None] - lat[None]) ** 2).sum(axis=2)
    assert (d2 == d2.max()).sum() == 8, "the lattice's four space diagonals, both ways"
    assert out["exp_far"][6] < 400 and out["exp_far"][0] > 9e5, "a small cloud far from the origin"
    assert abs(out["exp_shell"][6] - 110.0) < 1.0 and out["exp_clusters"][6] > 300.0
    np.savez_compressed(os.path.join(HERE, "model_info.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "model_info.npz")), "bytes")


if __name__ == "__main__":
    main()
