"""Generate tests/golden/icp_post_refinement.npz from the REFERENCE's own `post_refinement` (utils/model_utils.py:649-664).

Runs ONLY in the build container (needs the reference checkout; never on the GPU box, never from tests), like make_golden.py, whose
import scaffolding it uses.  `post_refinement` works on FIXED correspondences and on batch 1: a few problems of tests/icp_ref.py
(`problem(seed)`), the correspondences being the nearest neighbours at the start pose, are run through it, and the inputs, the final
pose and the number of `rigid_transform_3d` steps it took (counted by wrapping the module's function for the run) are stored.

    python tests/golden/make_icp_golden.py

Only arrays are written; no reference source is copied.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save  # noqa: E402  (sets sys.path for the repo root and tests/)

import icp_ref as I  # noqa: E402

CASES = [(1, 0.03, 16), (2, 0.03, 16), (3, 0.05, 16), (4, 0.1, 16), (5, 0.02, 3)]  # (seed of icp_ref.problem, inlier_threshold, iters)


def main():
    import_reference()
    import core.unopose.utils.model_utils as mu

    steps = [0]
    inner = mu.rigid_transform_3d

    def counted(*a, **k):
        steps[0] += 1
        return inner(*a, **k)

    mu.rigid_transform_3d = counted
    out = {}
    try:
        for c, (seed, tau, iters) in enumerate(CASES):
            z = I.problem(seed)
            corr, _ = I.search(I.transform(z["P"].astype(np.float64), z["R0"].astype(np.float64), z["t0"].astype(np.float64)), z["Q"].astype(np.float64))
            T0 = torch.eye(4)[None].clone()
            T0[0, :3, :3], T0[0, :3, 3] = torch.from_numpy(z["R0"]), torch.from_numpy(z["t0"])
            src, tgt = torch.from_numpy(z["Q"][corr])[None], torch.from_numpy(z["P"])[None]   # p ~ R q + t: the source is Q's side
            steps[0] = 0
            T = mu.post_refinement(T0, src, tgt, iters, inlier_threshold=tau)
            print(f"  case {c}: seed {seed} tau {tau}: {steps[0]} steps")
            out.update({f"c{c}_P": z["P"], f"c{c}_Q": z["Q"], f"c{c}_corr": corr.astype(np.int32), f"c{c}_R0": z["R0"], f"c{c}_t0": z["t0"],
                        f"c{c}_tau": np.float32(tau), f"c{c}_iters": np.int32(iters), f"c{c}_R": T[0, :3, :3].numpy().copy(),
                        f"c{c}_t": T[0, :3, 3].numpy().copy(), f"c{c}_steps": np.int32(steps[0])})
    finally:
        mu.rigid_transform_3d = inner
    save("icp_post_refinement", n_cases=np.int32(len(CASES)), **out)


if __name__ == "__main__":
    main()
