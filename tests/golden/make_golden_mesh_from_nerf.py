#!/usr/bin/env python3
"""Golden vectors for the box arithmetic of render_mesh(source='nerf'), produced BY THE REFERENCE.

The reference's evaluation/renderer.py cannot be imported here (open3d and cv2 are not installed), so, as in
make_golden_metrics3d.py, the definition of ``Renderer._render_mesh_from_nerf`` (:166-210) is parsed out of the reference
file and executed AT GENERATION TIME (nothing is copied into the repository).  Stand-ins serve its Open3D calls:
``o3d.io.read_point_cloud`` hands back the ground-truth vertices, ``o3d.io.read_triangle_mesh`` an object whose
``transform`` and ``crop`` record their argument, ``o3d.geometry.AxisAlignedBoundingBox`` keeps its two corners and
``o3d.io.write_triangle_mesh`` does nothing; a recording ``nerf.render_mesh`` stands in for the renderer.  That leaves the
reference's own part: the ground-truth box, its eight corners mapped by inv(matrix_pred2gt_scaled), the bounds and the
resolution handed to the renderer, the matrix given to ``transform`` and the box given to ``crop``.

Three cases: identity; scale 1.25 with a rigid motion; an anisotropic ground-truth box (with another motion and scale).
Stored per case i: the inputs ``gt_vertices{i}``, ``gt0_{i}`` / ``pred0_{i}`` (frame-0 poses), ``scale{i}``, ``matrix{i}``
(matrix_pred2gt_scaled = gt0 @ diag(s, s, s, 1) @ inv(pred0)), and what the reference handed over: ``resolution{i}``,
``lower_bound{i}``, ``upper_bound{i}``, ``transform{i}``, ``crop_lower{i}``, ``crop_upper{i}``.
Writes tests/golden/mesh_from_nerf_golden.npz.   python tests/golden/make_golden_mesh_from_nerf.py <reference tree>
"""
import ast
import os
import tempfile
import types

import numpy as np


def _method(path, cls, name, ns):
    tree = ast.parse(open(path).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    picked = [n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name == name]
    exec(compile(ast.Module(body=picked, type_ignores=[]), os.path.basename(path), "exec"), ns)
    return ns[name]


def _rigid(rng, angle, translation):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m[:3, 3] = translation
    return m


def build(reference):
    rng = np.random.default_rng(47)
    cases = [
        # identity
        (rng.uniform((-1.0, -0.8, -0.5), (1.0, 0.8, 0.5), size=(200, 3)), np.eye(4), np.eye(4), 1.0),
        # scale 1.25 with a rigid motion
        (rng.uniform((-1.0, -0.8, -0.5), (1.0, 0.8, 0.5), size=(200, 3)), _rigid(rng, 0.4, (0.3, -0.2, 0.1)),
         _rigid(rng, -0.7, (-0.1, 0.25, 0.05)), 1.25),
        # an anisotropic ground-truth box
        (rng.uniform((-3.1, -0.4, 0.2), (2.7, 0.45, 2.9), size=(200, 3)), _rigid(rng, 1.1, (0.5, 0.1, -0.3)),
         _rigid(rng, 0.2, (0.0, -0.4, 0.2)), 0.8),
    ]
    out = {"n_cases": np.int64(len(cases))}
    for i, (gt_vertices, gt0, pred0, scale) in enumerate(cases):
        record = {}

        class Mesh:
            def transform(self, matrix):
                record["transform"] = np.array(matrix)
                return self

            def crop(self, box):
                record["crop"] = box
                return self

        o3d = types.SimpleNamespace(
            io=types.SimpleNamespace(read_point_cloud=lambda file: types.SimpleNamespace(points=gt_vertices),
                                     read_triangle_mesh=lambda file: Mesh(), write_triangle_mesh=lambda file, mesh: None),
            geometry=types.SimpleNamespace(AxisAlignedBoundingBox=lambda lo, hi: (np.array(lo), np.array(hi))))
        render = _method(os.path.join(reference, "evaluation", "renderer.py"), "Renderer", "_render_mesh_from_nerf", {"np": np, "os": os, "o3d": o3d})

        def render_mesh(file_mesh, resolution, lower_bound, upper_bound):
            record["call"] = (np.array(resolution), np.array(lower_bound), np.array(upper_bound))

        matrix = gt0 @ np.diag([scale, scale, scale, 1.0]) @ np.linalg.inv(pred0)
        with tempfile.TemporaryDirectory() as tmp:
            this = types.SimpleNamespace(dir_prediction=tmp, dataset=types.SimpleNamespace(mesh=lambda: (None, "gt.ply")),
                                         nerf=types.SimpleNamespace(render_mesh=render_mesh),
                                         pred2gt_transformation={"scale_pred2gt": scale, "matrix_pred2gt_scaled": matrix})
            render(this)
        out[f"gt_vertices{i}"], out[f"gt0_{i}"], out[f"pred0_{i}"] = gt_vertices, gt0, pred0
        out[f"scale{i}"], out[f"matrix{i}"] = np.float64(scale), matrix
        out[f"resolution{i}"], out[f"lower_bound{i}"], out[f"upper_bound{i}"] = record["call"]
        out[f"transform{i}"] = record["transform"]
        out[f"crop_lower{i}"], out[f"crop_upper{i}"] = record["crop"]
        print(i, record["call"], record["crop"])
    return out


if __name__ == "__main__":
    import sys

    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_mesh_from_nerf.py <directory of the reference tree>")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_from_nerf_golden.npz")
    np.savez_compressed(path, **build(sys.argv[1]))
    print("wrote", path, os.path.getsize(path), "bytes")
