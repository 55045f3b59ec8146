"""What tests/test_model_info_cpu.py and tests/test_model_info_gpu.py share: the recorded point sets with the toolkit's values
(tests/golden/model_info.npz, made by tests/golden/make_model_info_golden.py), a small PLY writer, a folder of model files and a small
BOP dataset folder to score on."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_NAMES = ("one", "two", "duplicates", "lattice", "random", "shell", "box", "clusters", "far")
_cache = {}


def golden():
    """{name: (points (V, 3) float64, expected = min x, y, z, size x, y, z, diameter)}; loaded once, never written to."""
    if not _cache:
        z = np.load(os.path.join(ROOT, "tests", "golden", "model_info.npz"))
        for name in SET_NAMES:
            pts, exp = z["pts_" + name].astype(np.float64), z["exp_" + name].astype(np.float64)
            pts.setflags(write=False), exp.setflags(write=False)
            _cache[name] = (pts, exp)
    return _cache


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def write_ply(path, pts, binary):
    """Vertices alone, float32 binary little-endian or ASCII."""
    pts = np.asarray(pts, np.float32)
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(pts),
            "property float x", "property float y", "property float z", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(pts.astype("<f4").tobytes())
        else:
            f.write("".join("%s %s %s\n" % tuple(repr(float(v)) for v in p) for p in pts).encode("ascii"))


MODEL_SETS = {1: "random", 4: "box", 7: "clusters", 12: "two"}  # obj_id -> point set; object 4 is the ASCII file


def write_model_folder(folder):
    """Four small model files -> {obj_id: points as read_ply returns them (float32 values in float64)}."""
    os.makedirs(folder, exist_ok=True)
    out = {}
    for obj_id, name in MODEL_SETS.items():
        pts = golden()[name][0]
        write_ply(os.path.join(folder, f"obj_{obj_id:06d}.ply"), pts, binary=obj_id != 4)
        out[obj_id] = pts.astype(np.float32).astype(np.float64)
    return out


def write_score_dataset(root, symmetric):
    """`bop_eval_case.make_vsd_case` as a dataset folder (tests/bop_score_case.py's writer).  symmetric=False strips object 2's symmetry, so
    that the dataset means the same with and without its models_info.json.  -> (csv path, models_eval folder)."""
    import bop_score_case
    from bop_eval_case import make_vsd_case

    case = list(make_vsd_case())
    if not symmetric:
        case[0] = {o: dict(m, symmetries=m["symmetries"][:1]) for o, m in case[0].items()}
    csv, _ = bop_score_case.write_dataset(root, tuple(case))
    return csv, os.path.join(root, "synth", "models_eval")


def load_info(folder):
    return json.load(open(os.path.join(folder, "models_info.json")))
