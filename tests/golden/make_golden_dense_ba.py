#!/usr/bin/env python3
"""Golden vectors for the depth covariance of the dense bundle adjustment, produced BY THE
REFERENCE's own lines.

/root/reference/nerf_vo/tracking/droid_slam.py cannot be imported (lietorch, gtsam and droid_backends do not exist
here), but the covariance block of ``ba`` (:685-725, from ``identity = ...`` to the write into ``cam0_depths_cov``) is
plain torch.  Those statements are parsed out of the reference file and executed AT GENERATION TIME on the CPU (nothing
is copied into the repository), with stand-ins for ``self`` (device, ht, wd, cam0_idepths, cam0_depths_cov) and for the
inputs the lines above them leave behind: ``L`` (the float32 Cholesky factor of ``H``, as :680-681 form it), ``E``, ``Q``,
``ii``, ``jj``, ``kf0``, ``kf1``, ``N``, ``HW``, and an empty ``pose_keys`` (the loop over it computes nothing that is used).

``H``, ``E``, ``Q`` and the updated inverse depths come from tests/helpers/dense_ba_oracle.py on two small cases of
helpers/dense_ba_cases.py whose graphs the reference's indexing accepts (every frame a source, no repeated edge): one
with the first pose free and the prior, one with two fixed poses.  Stored: the inputs and the resulting z_cov / depth_cov.
Writes tests/golden/dense_ba_cov_golden.npz.   python tests/golden/make_golden_dense_ba.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

from helpers import dense_ba_cases as cases  # noqa: E402
from helpers import dense_ba_oracle as orc  # noqa: E402

REF = "/root/reference/nerf_vo/tracking/droid_slam.py"
CASES = {"prior": dict(K=4, ht=5, wd=7, t0=0, noise=0.05, damping=cases.GRID_DAMPING, full=True),
         "fixed2": dict(K=5, ht=6, wd=9, t0=2, noise=0.05, damping=cases.GRID_DAMPING, full=True)}


def reference_block():
    """The statements of the reference's covariance block, compiled."""
    tree = ast.parse(open(REF).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "ba")
    outer = next(n for n in fn.body if isinstance(n, ast.If) and getattr(n.test, "id", "") == "compute_covariances")
    inner = next(n for n in outer.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare))  # if L is not None:
    first = next(k for k, n in enumerate(inner.body) if isinstance(n, ast.Assign) and n.targets[0].id == "identity")
    return compile(ast.Module(body=inner.body[first:], type_ignores=[]), os.path.basename(REF), "exec")


def build():
    code = reference_block()
    out = {}
    for tag, kw in CASES.items():
        c = cases.make(**kw)
        run = orc.ba(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"], c["target"], c["weight"], c["eta"], c["t0"],
                     c["t1"], prior_sigma=c["prior_sigma"])
        last = run["its"][-1]
        H = last["S"].astype(np.float32)
        E = np.concatenate([last["Ei"], last["Ej"]]).astype(np.float32)
        Q = last["Q"].astype(np.float32)
        idepths = run["disps"].astype(np.float32)
        me = types.SimpleNamespace(device=torch.device("cpu"), ht=c["ht"], wd=c["wd"], cam0_idepths=torch.from_numpy(idepths.copy()),
                                   cam0_depths_cov=torch.ones(c["K"], c["ht"], c["wd"]), f_idx_to_kf_idx={})
        ns = {"torch": torch, "self": me, "L": torch.linalg.cholesky(torch.as_tensor(H, dtype=torch.float)),
              "E": torch.from_numpy(E.copy()), "Q": torch.from_numpy(Q.copy()), "ii": torch.from_numpy(c["ii"]),
              "jj": torch.from_numpy(c["jj"]), "kf0": c["t0"], "kf1": c["t1"], "N": c["t1"] - c["t0"], "HW": c["ht"] * c["wd"],
              "pose_keys": []}
        exec(code, ns)
        for name, val in (("H", H), ("E", E), ("Q", Q), ("idepths", idepths), ("ii", c["ii"]), ("jj", c["jj"]),
                          ("kf0", np.array(c["t0"])), ("kf1", np.array(c["t1"])), ("z_cov", ns["z_cov"].numpy().copy()),
                          ("kx", ns["kx"].numpy().copy()), ("depth_cov", me.cam0_depths_cov.numpy().copy())):
            out[f"{tag}_{name}"] = val
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "dense_ba_cov_golden.npz")
    np.savez_compressed(path, **build())
    print("wrote", path, os.path.getsize(path), "bytes")
