#!/usr/bin/env python3
"""Golden vectors for the 3-D mesh metrics, produced BY THE REFERENCE.

/root/reference/evaluation/evaluation_utils.py cannot be imported here (open3d, cv2, lpips are not installed), so, as in
make_golden_evaluation.py, the definition of ``calculate_metrics_3d`` (:466-512) is parsed out of the reference file and
executed AT GENERATION TIME (nothing is copied into the repository).  Its Open3D calls are served by small stand-in
objects that hand back fixed clouds -- ``mesh.sample_points_uniformly``, ``PointCloud.from_legacy``,
``voxel_down_sample``, ``transform`` pass the cloud through, ``.point.positions.numpy()`` returns it, and
``get_pcd_alignment_transformation`` returns the identity -- which leaves the reference's own part: the two
``scipy.spatial.cKDTree`` queries (recorded through a subclass) and the five formulae.  scipy is needed only here.

Stored per cloud pair i: ``gt{i}``, ``pred{i}`` (float32 points), ``d_pred_to_gt{i}`` / ``i_pred_to_gt{i}`` (for every
ground-truth point: distance to and index of its nearest predicted point, the reference's ``distances_pred_to_gt``),
``d_gt_to_pred{i}`` / ``i_gt_to_pred{i}`` (the reverse) and ``metrics{i}`` in the order of ``metric_names``.
Writes tests/golden/metrics3d_golden.npz.   python tests/golden/make_golden_metrics3d.py
"""
import ast
import os
import types

import numpy as np
import scipy.spatial


def _function(path, name, ns):
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    exec(compile(ast.Module(body=picked, type_ignores=[]), os.path.basename(path), "exec"), ns)
    return ns[name]


class _Cloud:
    """Stands in for the legacy and the tensor point cloud alike: every Open3D step hands the fixed cloud on."""

    def __init__(self, points):
        self._points = points
        self.point = types.SimpleNamespace(positions=types.SimpleNamespace(numpy=lambda: self._points))

    def sample_points_uniformly(self, number_of_points):
        return self

    def voxel_down_sample(self, voxel_size):
        return self

    def transform(self, transformation):
        assert np.array_equal(transformation, np.eye(4))
        return self


def _surface(rng, n, lower, upper, jitter):
    lo, hi = np.asarray(lower), np.asarray(upper)
    p = rng.uniform(lo, hi, size=(n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return (p + jitter * rng.normal(size=p.shape)).astype(np.float32)


def build():
    queries = []

    class RecordingTree(scipy.spatial.cKDTree):
        def query(self, *args, **kwargs):
            out = super().query(*args, **kwargs)
            queries.append(out)
            return out

    ns = {"np": np,
          "scipy": types.SimpleNamespace(spatial=types.SimpleNamespace(cKDTree=RecordingTree)),
          "o3d": types.SimpleNamespace(
              geometry=types.SimpleNamespace(TriangleMesh=object),
              t=types.SimpleNamespace(geometry=types.SimpleNamespace(PointCloud=types.SimpleNamespace(from_legacy=lambda c: c)))),
          "get_pcd_alignment_transformation": lambda source, target: np.eye(4)}
    metrics_3d = _function("/root/reference/evaluation/evaluation_utils.py", "calculate_metrics_3d", ns)

    rng = np.random.default_rng(31)
    lo, hi = (-1.0, -0.8, -0.5), (1.0, 0.8, 0.5)
    pairs = []
    # 0: two jittered samplings of the same room surface, a few millimetres apart
    pairs.append((_surface(rng, 3000, lo, hi, 0.002), _surface(rng, 2500, lo, hi, 0.006)))
    # 1: the prediction misses the part of the room beyond x = 0.55 and has a slab of clutter 12 cm inside the floor's
    # level: precision and recall strictly between 0 and 1
    gt = _surface(rng, 3000, lo, hi, 0.002)
    pred = _surface(rng, 3200, lo, hi, 0.004)
    pred = pred[pred[:, 0] < 0.55][:2100]
    clutter = rng.uniform((-0.5, -0.4, -0.38), (0.3, 0.4, -0.36), size=(400, 3)).astype(np.float32)
    pairs.append((gt, np.concatenate([pred, clutter])))

    out = {}
    for i, (points_gt, points_pred) in enumerate(pairs):
        del queries[:]
        m = metrics_3d(_Cloud(points_gt), _Cloud(points_pred))
        (d_pred_to_gt, i_pred_to_gt), (d_gt_to_pred, i_gt_to_pred) = queries  # the order of the reference's two queries
        assert d_pred_to_gt.shape[0] == points_gt.shape[0] and d_gt_to_pred.shape[0] == points_pred.shape[0]
        out[f"gt{i}"], out[f"pred{i}"] = points_gt, points_pred
        out[f"d_pred_to_gt{i}"], out[f"i_pred_to_gt{i}"] = d_pred_to_gt, i_pred_to_gt.astype(np.int32)
        out[f"d_gt_to_pred{i}"], out[f"i_gt_to_pred{i}"] = d_gt_to_pred, i_gt_to_pred.astype(np.int32)
        out[f"metrics{i}"] = np.array([m[k] for k in sorted(m)])
        print(i, points_gt.shape, points_pred.shape, m)
    out["metric_names"] = np.array(sorted(m))
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics3d_golden.npz")
    np.savez_compressed(path, **build())
    print("wrote", path, os.path.getsize(path), "bytes")
