#!/usr/bin/env python3
"""Golden vectors for the trajectory table (metrics_trajectory.csv), produced BY THE REFERENCE.

/root/reference/evaluation/evaluation_utils.py cannot be imported here (cv2, open3d, lpips are not installed), but
kabsch_umeyama_alignment (:230-252) and calculate_absolute_trajectory_error (:255-286) are plain numpy: their definitions
are parsed out of the reference file and executed AT GENERATION TIME (nothing is copied into the repository).

Three seeded trajectories: 40 poses on a helix, compared with scale; 5 poses on a nearly planar, nearly collinear layout
whose cross-covariance has a tiny third singular value (the reflection guard decides the last axis), with scale; 17 poses
compared WITHOUT scale.  Writes tests/golden/trajectory_golden.npz.   python tests/golden/make_golden_trajectory.py
"""
import ast
import os

import numpy as np

ATE_KEYS = ("absolute_trajectory_error_rmse", "absolute_trajectory_error_mean", "absolute_trajectory_error_median",
            "absolute_trajectory_error_std", "absolute_trajectory_error_max", "absolute_trajectory_error_min")


def _functions(path, names):
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"np": np}
    exec(compile(ast.Module(body=picked, type_ignores=[]), os.path.basename(path), "exec"), ns)
    return ns


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def _poses(centres, rng):
    m = np.tile(np.eye(4), (centres.shape[0], 1, 1))
    m[:, :3, :3] = np.stack([_rotation(rng) for _ in range(centres.shape[0])])
    m[:, :3, 3] = centres
    return m


def _similar(centres, rng, scale, noise):
    """The centres in another frame: rotated, scaled, shifted, with tracker-like noise."""
    r, t = _rotation(rng), rng.normal(size=3)
    return (centres - t) @ r / scale + noise * rng.normal(size=centres.shape)


def build():
    utils = _functions("/root/reference/evaluation/evaluation_utils.py",
                       {"kabsch_umeyama_alignment", "calculate_absolute_trajectory_error"})
    rng = np.random.default_rng(20)  # (a seed at which the planar case's two SVD bases disagree in handedness: d = -1)
    out = {}
    s = np.linspace(0.0, 4.0 * np.pi, 40)
    helix = np.stack([1.5 * np.cos(s), 1.5 * np.sin(s), 0.15 * s], axis=1)
    flat = np.stack([np.linspace(-1.0, 1.0, 5), 0.05 * rng.normal(size=5), 1e-4 * rng.normal(size=5)], axis=1)
    walk = np.cumsum(0.2 * rng.normal(size=(17, 3)), axis=0)
    cases = ((helix, 2.3, 0.01, True), (flat, 0.7, 0.02, True), (walk, 1.0, 0.03, False))
    for i, (centres, scale, noise, with_scale) in enumerate(cases):
        gt, pred = _poses(centres, rng), _poses(_similar(centres, rng, scale, noise), rng)
        rotation, translation, sc = utils["kabsch_umeyama_alignment"](gt[:, :3, 3], pred[:, :3, 3], with_scale=with_scale)
        ate = utils["calculate_absolute_trajectory_error"](gt, pred, with_scale=with_scale)
        out[f"traj{i}_gt"], out[f"traj{i}_pred"] = gt, pred
        out[f"traj{i}_with_scale"] = np.array(with_scale)
        out[f"traj{i}_rotation"], out[f"traj{i}_translation"], out[f"traj{i}_scale"] = rotation, translation, np.array(sc)
        out[f"traj{i}_ate"] = np.array([ate[k] for k in ATE_KEYS])
    out["ate_names"] = np.array(ATE_KEYS)
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trajectory_golden.npz")
    np.savez_compressed(path, **build())
    print("wrote", path, os.path.getsize(path), "bytes")
