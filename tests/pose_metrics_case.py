"""The problems of the further pose errors' tests (tests/test_pose_metrics_cpu.py, tests/test_pose_metrics_gpu.py,
tests/golden/make_pose_metrics_golden.py, scripts/pose_metrics_rate.py).

`kernel_cases()`: point sets whose sizes straddle what the ADI kernel tiles by -- TILE points per LDS tile, SLAB query points per
workgroup (the GPU test checks both against the library's query entry points) -- n in {1, 2, 63, 64, 65, SLAB - 1, SLAB + 1, TILE - 1, TILE,
TILE + 1, 2 TILE + 3}, one set with duplicated points, and 65-point sets under 2, 5 (an axis off the origin: non-zero translations) and
315 (one continuous axis, discretised) symmetries.  Each set is scored under six graded poses, `POSE_KINDS`.
`make_scoring_case()`: `bop_score_case.make_large_case()` plus a handful of high-scored estimates that are right in rotation (< 1 degree)
and off in translation by 30 - 80 mm: with them `rete` is neither `re` nor `te`.  `scoring_case_facts` is the check that it is graded."""
import numpy as np

import bop_score_case as C
from bop_eval_case import rot

TILE, SLAB = 1024, 256
POSE_KINDS = ("identical", "twin", "small", "gross", "behind", "apart")
K = np.array([[572.4, 0.3, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])  # with a skew term: the whole matrix is used
NEW_TYPES = ("add", "adi", "ad", "ABSadd", "ABSadi", "ABSad", "AUCadd", "AUCadi", "AUCad", "re", "te", "rete", "proj", "reS", "teS", "reteS", "projS")
AXIS_POINT = np.array([3.0, -2.0, 0.0])  # a point of the 5-fold and of the continuous axis (direction z)
IDENTITY = dict(R=np.eye(3), t=np.zeros(3))


def _blob(rs, n):
    """n points on a bumpy ellipsoid of about 110 mm."""
    d = rs.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * np.array([40.0, 55.0, 30.0]) * (1.0 + 0.2 * np.sin(4.0 * d[:, [1, 2, 0]]))


def _five_fold(rs):
    """65 points = 13 x the five rotations about the z direction through AXIS_POINT."""
    base = _blob(rs, 13)
    return np.concatenate([(base - AXIS_POINT) @ rot([0, 0, 1], 2.0 * np.pi * k / 5.0).T + AXIS_POINT for k in range(5)])


def _diameter(pts):
    return float(np.linalg.norm(pts[:, None] - pts[None], axis=2).max()) if len(pts) > 1 else 50.0


def _poses(rs, pts, syms, diameter):
    """The six graded (R_est, t_est, R_gt, t_gt) of a set, in the order of POSE_KINDS."""
    out = []
    for kind in POSE_KINDS:
        Rg = rot(rs.randn(3), rs.rand() * 3)
        tg = np.array([rs.uniform(-120, 120), rs.uniform(-90, 90), rs.uniform(650, 1000)])
        if kind == "identical":
            Re, te = Rg.copy(), tg.copy()
        elif kind == "twin":  # the ground truth composed with the last symmetry (the identity where there is no other): an exact twin
            s = syms[126] if len(syms) == 315 else syms[-1]  # 126 = 2 x 63 steps of 2 pi / 315: two fifths of a turn
            Re, te = Rg @ s["R"], Rg @ s["t"] + tg
        elif kind == "small":
            Re, te = Rg @ rot(rs.randn(3), 0.02), tg + rs.randn(3) * 1.5
        elif kind == "gross":
            Re, te = Rg @ rot(rs.randn(3), 1.3), tg + rs.randn(3) * 0.2 * diameter
        elif kind == "behind":
            Re, te = Rg @ rot(rs.randn(3), 0.1), tg * np.array([1.0, 1.0, -1.0])
        else:  # the centres more than a diameter apart, in front of the camera
            Re, te = Rg @ rot(rs.randn(3), 0.05), tg + np.array([0.8, -0.5, 0.6]) * 1.5 * diameter
        out.append((Re, te, Rg, tg))
    return out


def kernel_cases(seed=5):
    """-> [dict(name, pts (n,3), symmetries, diameter, K, poses: the six of POSE_KINDS)]."""
    from unopose_amd import bop_eval

    rs = np.random.RandomState(seed)
    sets = [("n%d" % n, _blob(rs, n), [IDENTITY]) for n in (1, 2, 63, 64, 65, SLAB - 1, SLAB + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
    dup = _blob(rs, 40)
    sets.append(("duplicates", np.concatenate([dup, dup[::3], dup[:5]]), [IDENTITY]))
    half = _blob(rs, 32)
    sets.append(("two_fold", np.concatenate([half, half @ rot([0, 0, 1], np.pi).T, [[0.0, 0.0, 21.0]]]), [IDENTITY, dict(R=rot([0, 0, 1], np.pi), t=np.zeros(3))]))
    five = [IDENTITY]
    for k in range(1, 5):
        R = rot([0, 0, 1], 2.0 * np.pi * k / 5.0)
        five.append(dict(R=R, t=AXIS_POINT - R @ AXIS_POINT))
    sets.append(("five_fold", _five_fold(rs), five))
    cont = bop_eval.symmetry_transformations(dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=AXIS_POINT.tolist())]))
    assert len(cont) == 315
    sets.append(("continuous", _five_fold(rs), cont))  # five-fold points: step 63 k of the 315 is a symmetry of the set
    out = []
    for name, pts, syms in sets:
        diameter = _diameter(pts)
        out.append(dict(name=name, pts=np.ascontiguousarray(pts), symmetries=syms, diameter=diameter, K=K, poses=_poses(rs, pts, syms, diameter)))
    return out


def host_values(case, adi_fn=None):
    """The eight errors of every pose of a kernel case with the host functions -> {name: [per pose]}."""
    from unopose_amd import bop_eval as B

    out = {k: [] for k in ("add", "adi", "proj", "re", "te", "projS", "reS", "teS")}
    pts, syms, Kc = case["pts"], case["symmetries"], case["K"]
    for Re, te, Rg, tg in case["poses"]:
        out["add"].append(B.add(Re, te, Rg, tg, pts))
        out["adi"].append((adi_fn or B.adi)(Re, te, Rg, tg, pts))
        out["proj"].append(B.proj(Re, te, Rg, tg, Kc, pts))
        out["re"].append(B.re(Re, Rg))
        out["te"].append(B.te(te, tg))
        out["projS"].append(B.proj_sym(Re, te, Rg, tg, Kc, pts, syms))
        out["reS"].append(B.re_sym(Re, Rg, syms))
        out["teS"].append(B.te_sym(te, tg, Rg, syms))
    return out


def kernel_case_facts(case, values):
    """The grading of a kernel case's poses, on its host (or golden) values."""
    v = {k: dict(zip(POSE_KINDS, values[k])) for k in values}
    d = case["diameter"]
    facts = dict(identical=all(v[k]["identical"] <= 1e-5 for k in v), small=0.0 < v["add"]["small"] < 0.1 * d and v["re"]["small"] < 2.0,
                 gross=v["re"]["gross"] > 30.0, apart=v["te"]["apart"] >= d, behind=v["te"]["behind"] > 1000.0)
    if len(case["symmetries"]) > 1:
        facts["twin"] = v["add"]["twin"] > 0.2 * d and v["re"]["twin"] > 30.0 and all(v[k]["twin"] <= 1e-5 for k in ("adi", "projS", "reS", "teS"))
    return facts


def make_scoring_case(n_added=8, seed=41, case=None):
    """-> the tuple of `make_large_case` with `n_added` estimates appended: top-scored, rotation within 1 degree of a ground truth of
    objects 1 .. 3 in turn, translation off by 30 .. 80 mm."""
    case = C.make_large_case() if case is None else case  # `case`: an unmodified large case, left as it is
    models, scene_gt, cameras, results = case[:4]
    rs = np.random.RandomState(seed)
    spots = [(sid, iid, gid) for sid in sorted(scene_gt) for iid in sorted(scene_gt[sid]) for gid, g in enumerate(scene_gt[sid][iid]) if g["valid"]]
    added = []
    for k in range(n_added):
        want = 1 + k % 3
        sid, iid, gid = [s for s in spots if scene_gt[s[0]][s[1]][s[2]]["obj_id"] == want][3 + 2 * (k // 3)]
        g = scene_gt[sid][iid][gid]
        d = rs.randn(3)
        added.append(dict(scene_id=sid, im_id=iid, obj_id=want, score=1.5 + 0.01 * k, R=g["R"] @ rot(rs.randn(3), np.deg2rad(rs.uniform(0.2, 0.9))),
                          t=g["t"] + d / np.linalg.norm(d) * rs.uniform(30.0, 80.0), time=0.1))
    return (models, scene_gt, cameras, results + added) + tuple(case[4:])


def scoring_case_facts(errors, pairs):
    """What `average_recall(..., error_types=NEW_TYPES)["errors"]` of a scoring case must show for the equality tests to mean something;
    `pairs`: `bop_eval.metric_pairs` of the same walk."""
    facts = {}
    for T in NEW_TYPES:
        r = errors[T]["recalls"]
        facts[T] = 0.0 < min(r) and max(r) < 1.0 and all(a <= b for a, b in zip(r, r[1:]))
    facts["ad_is_not_add"] = errors["ad"]["recalls"] != errors["add"]["recalls"]
    facts["rete_is_neither"] = errors["rete"]["recalls"] != errors["re"]["recalls"] and errors["rete"]["recalls"] != errors["te"]["recalls"]
    facts["sphere_rule"] = sum(p["apart"] for p in pairs) >= 1
    return facts
