"""Expected values for tests/pose_metrics_case.py from the REFERENCE's own evaluation layer (lib/pysixd): pose_error.add / adi /
arp_2d / arp_2d_sym / re / te / re_sym / te_sym on the kernel cases, and -- with the thresholds, units, normalisation and sphere rule of
scripts/eval_pose_results_more.py:74-155, eval_calc_errors.py:367-591 and eval_calc_scores.py:70 -- pose_matching.match_poses_scene +
score.calc_localization_scores on the large case of tests/bop_score_case.py and on the scoring case, n_top = -1.  Numbers only.
    python tests/golden/make_pose_metrics_golden.py   ->  tests/golden/pose_metrics.json"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")


class _Permissive(types.ModuleType):
    """A third-party package the reference imports at module level and none of the functions used here touches."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        mod = _Permissive(self.__name__ + "." + name)
        sys.modules[mod.__name__] = mod
        return mod

    def __call__(self, *a, **k):
        return self


for _name in ("termcolor", "cv2", "mmcv", "mmengine", "imageio", "png", "chardet"):
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = _Permissive(_name)

import bop_score_case as C  # noqa: E402
import pose_metrics_case as M  # noqa: E402
from lib.pysixd import pose_error, pose_matching, score  # noqa: E402

TYPES = {  # eval_pose_results_more.py:74-155
    "add": [[th] for th in [0.02, 0.05, 0.1]], "adi": [[th] for th in [0.02, 0.05, 0.1]], "ad": [[th] for th in [0.02, 0.05, 0.1]],
    "ABSadd": [[2]], "ABSadi": [[2]], "ABSad": [[2]],
    "AUCadd": [[th] for th in np.linspace(10 / 10, 10, num=10)], "AUCadi": [[th] for th in np.linspace(10 / 10, 10, num=10)],
    "AUCad": [[th] for th in np.linspace(10 / 10, 10, num=10)],
    "re": [[th] for th in [2, 5, 10]], "te": [[th] for th in [2, 5, 10]], "rete": [[2, 2], [5, 5], [10, 10]], "proj": [[th] for th in [2, 5, 10]],
    "reS": [[th] for th in [2, 5, 10]], "teS": [[th] for th in [2, 5, 10]], "reteS": [[2, 2], [5, 5], [10, 10]], "projS": [[th] for th in [2, 5, 10]],
}


def kernel_values():
    out = {}
    for case in M.kernel_cases():
        syms = [dict(R=s["R"], t=s["t"].reshape(3, 1)) for s in case["symmetries"]]
        v = {k: [] for k in ("add", "adi", "proj", "re", "te", "projS", "reS", "teS")}
        for Re, te, Rg, tg in case["poses"]:
            a = (Re, te.reshape(3, 1), Rg, tg.reshape(3, 1))
            v["add"].append(float(pose_error.add(*a, case["pts"])))
            v["adi"].append(float(pose_error.adi(*a, case["pts"])))
            v["proj"].append(float(pose_error.arp_2d(*a, pts=case["pts"], K=case["K"])))
            v["projS"].append(float(pose_error.arp_2d_sym(*a, pts=case["pts"], K=case["K"], syms=syms)))
            v["re"].append(float(pose_error.re(Re, Rg)))
            v["te"].append(float(pose_error.te(a[1], a[3])))
            v["reS"].append(float(pose_error.re_sym(Re, Rg, syms=syms)))
            v["teS"].append(float(pose_error.te_sym(a[1], a[3], R_gt=Rg, syms=syms)))
        out[case["name"]] = v
    return out


def pair_errors(e_type, R_e, t_e, R_g, t_g, K, m, symmetric):
    """eval_calc_errors.py:364-591 for one pair, then eval_calc_scores.py:248-253."""
    pts, syms, diameter = m["pts"], m["symmetries_bop"], m["diameter"]
    if e_type in ("ad", "add", "adi"):
        if not np.linalg.norm(t_e - t_g) < diameter:
            return [float("inf")]
        fn = pose_error.adi if e_type == "adi" or (e_type == "ad" and symmetric) else pose_error.add
        return [fn(R_e, t_e, R_g, t_g, pts) / diameter]
    if e_type[:3] in ("ABS", "AUC"):
        fn = pose_error.adi if e_type[3:] == "adi" or (e_type[3:] == "ad" and symmetric) else pose_error.add
        return [fn(R_e, t_e, R_g, t_g, pts) / 10]
    if e_type == "proj":
        return [pose_error.arp_2d(R_e, t_e, R_g, t_g, pts=pts, K=K)]
    if e_type == "projS":
        return [pose_error.arp_2d_sym(R_e, t_e, R_g, t_g, pts=pts, K=K, syms=syms)]
    if e_type == "rete":
        return [pose_error.re(R_e, R_g), pose_error.te(t_e, t_g) / 10]
    if e_type == "reteS":
        return [pose_error.re_sym(R_e, R_g, syms=syms), pose_error.te_sym(t_e, t_g, R_gt=R_g, syms=syms) / 10]
    if e_type == "re":
        return [pose_error.re(R_e, R_g)]
    if e_type == "reS":
        return [pose_error.re_sym(R_e, R_g, syms=syms)]
    if e_type == "te":
        return [pose_error.te(t_e, t_g) / 10]
    if e_type == "teS":
        return [pose_error.te_sym(t_e, t_g, R_gt=R_g, syms=syms) / 10]
    raise ValueError(e_type)


def scoring(case):
    models, scene_gt, cameras, results = case[:4]
    for m in models.values():
        m["symmetries_bop"] = [dict(R=s["R"], t=s["t"].reshape(3, 1)) for s in m["symmetries"]]
    symmetric = [o for o, m in models.items() if len(m["symmetries"]) > 1]
    n_top, out, n_pairs, n_apart = -1, {}, 0, 0
    for e_type, ths in TYPES.items():
        scene_errs = {sid: [] for sid in scene_gt}
        for est_id, r in enumerate(results):
            m = models[r["obj_id"]]
            errs = {}
            for gid, g in enumerate(scene_gt[r["scene_id"]][r["im_id"]]):
                if g["obj_id"] == r["obj_id"]:
                    errs[gid] = [float(v) for v in pair_errors(e_type, r["R"], r["t"].reshape(3, 1), g["R"], g["t"].reshape(3, 1),
                                                               cameras[r["scene_id"]][r["im_id"]], m, r["obj_id"] in symmetric)]
                    if e_type == "add":
                        n_pairs, n_apart = n_pairs + 1, n_apart + (errs[gid][0] == float("inf"))
            scene_errs[r["scene_id"]].append(dict(im_id=r["im_id"], obj_id=r["obj_id"], est_id=est_id, score=r["score"], errors=errs))
        recalls, obj_recalls = [], {str(o): [] for o in models}
        for th in ths:
            matches = []
            for sid in scene_gt:
                gt_valid = {iid: [g["valid"] for g in gts] for iid, gts in scene_gt[sid].items()}
                matches += pose_matching.match_poses_scene(sid, scene_gt[sid], gt_valid, scene_errs[sid], th, n_top)
            sc = score.calc_localization_scores(list(scene_gt), list(models), matches, n_top, do_print=False)
            recalls.append(float(sc["recall"]))
            for o, v in sc["obj_recalls"].items():
                obj_recalls[str(o)].append(float(v))
        out[e_type] = dict(recalls=recalls, obj_recalls=obj_recalls, mean_recall=float(np.mean(recalls)))
    return dict(errors=out, n_pairs=n_pairs, n_apart=n_apart)


def main():
    out = dict(kernel=kernel_values(), large=scoring(C.make_large_case()), scoring=scoring(M.make_scoring_case()))
    json.dump(out, open(os.path.join(HERE, "pose_metrics.json"), "w"), indent=0)
    for k in ("large", "scoring"):
        print(k, out[k]["n_pairs"], out[k]["n_apart"], {t: [round(r, 2) for r in v["recalls"]] for t, v in out[k]["errors"].items()})


if __name__ == "__main__":
    main()
