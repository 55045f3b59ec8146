"""tests/golden/model_sym_toolkit.json: `models_info.json` entries in the format `unopose_amd.model_sym` writes, and what the REFERENCE's vendored
bop_toolkit_lib makes of them (`misc.get_symmetry_transformations` with the toolkit's default max_sym_disc_step = 0.01).  The discrete entries
are the ones `find_symmetries` finds for the polyhedra of tests/model_sym_case.py in their own frame; the cylinder's entry is written by hand
in the same format (one continuous axis through a centre off the origin, one half-turn about a perpendicular axis).  Build container only."""
import json
import os.path as osp
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, "/root/reference/third_party/bop_toolkit")
sys.path.insert(0, osp.dirname(HERE))
sys.path.insert(0, osp.dirname(osp.dirname(HERE)))

from bop_toolkit_lib import misc  # noqa: E402

import model_sym_case as case  # noqa: E402
from unopose_amd import model_sym  # noqa: E402

entries = {}
for name in ("box", "prism", "cube", "tetrahedron"):
    res = model_sym.find_symmetries(case.model(name, 0), tol=case.TOL, axes=case.AXES, max_order=case.MAX_ORDER)
    entries[name] = {"symmetries_discrete": res["symmetries_discrete"]}
c = np.array([3.0, -4.0, 12.0])
flip = np.eye(4)
flip[:3, :3] = np.diag([1.0, -1.0, -1.0])
flip[:3, 3] = c - flip[:3, :3] @ c
entries["cylinder"] = {"symmetries_discrete": [flip.reshape(-1).tolist()], "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": c.tolist()}]}
out = {}
for name, entry in entries.items():
    trans = misc.get_symmetry_transformations(entry, 0.01)
    out[name] = dict(entry=entry, count=len(trans), toolkit=[dict(R=np.asarray(t["R"]).reshape(-1).tolist(), t=np.asarray(t["t"]).reshape(-1).tolist()) for t in trans])
    print(name, len(trans))
json.dump(out, open(osp.join(HERE, "model_sym_toolkit.json"), "w"))
