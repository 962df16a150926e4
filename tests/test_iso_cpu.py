"""The edge-owned iso-surface rule on the CPU: its numpy restatement (tests/helpers/iso_oracle.py)
against ``marching_tetrahedra`` on the inputs where the torch extractor's merge is known to work, the case where it is
not (a crack), the generated case-table header, the crop / transform helpers and the box arithmetic of
``EvaluationRenderer.render_mesh(source='nerf')`` against what the reference hands to its renderer."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import iso_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER, UPPER = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
MARGINS = {}  # case -> largest nearest-vertex distance between oracle and torch extractor, in cells


def _case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}" + (f"-{case[2]}" if case[2] else "")


def _signed_volume(v, f):
    v = np.asarray(v, dtype=np.float64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def _nearest(a, b):
    """for every row of a, the L-inf distance to the nearest row of b"""
    out = np.empty(a.shape[0])
    for s in range(0, a.shape[0], 512):
        out[s:s + 512] = np.abs(a[s:s + 512, None, :] - b[None, :, :]).max(axis=2).min(axis=1)
    return out


@pytest.mark.parametrize("case", O.CASES, ids=_case_id)
def test_oracle_against_marching_tetrahedra(case):
    from nerf_vo_amd.meshing import marching_tetrahedra

    name, shape, spec, n_vert, n_face = case
    values, valid, v, f = O.reference(case)
    tv, tf = marching_tetrahedra(values, LOWER, UPPER, 0.0, valid=valid)
    print(f"{_case_id(case)}: oracle {v.shape[0]} vertices {f.shape[0]} faces, torch {tv.shape[0]} / {tf.shape[0]}")
    assert (v.shape[0], f.shape[0]) == (n_vert, n_face)
    assert (tv.shape[0], tf.shape[0]) == (n_vert, n_face)
    # every vertex of one has a vertex of the other within 2^-14 cell: each side is within about 2^-16 cell of the exact
    # cut (a few float32 roundings of a grid coordinate below 256) and the world mapping adds under 2^-17
    cell = O.lattice_step(LOWER, UPPER, shape).astype(np.float64)
    a, b = v.astype(np.float64) / cell, tv.numpy().astype(np.float64) / cell
    worst = max(_nearest(a, b).max(), _nearest(b, a).max())
    MARGINS[_case_id(case)] = float(worst)
    print(f"  largest nearest-vertex distance {worst:.3e} cell (bound {2.0 ** -14:.3e})")
    assert worst <= 2.0 ** -14
    if name == "sphere" and spec is None:
        vol, tvol = _signed_volume(v, f), _signed_volume(tv.numpy(), tf.numpy())
        print(f"  signed volume {vol:.6f}, torch {tvol:.6f}")
        assert vol > 0 and abs(vol - tvol) <= 1e-4 * abs(tvol)
    if spec is not None:
        assert np.array_equal(np.unique(f), np.arange(v.shape[0])), "a vertex no face refers to"
    # the parity-margins file: NVO_ISO_MARGINS=profiles/iso_parity_margins.json rewrites the committed record
    path = os.environ.get("NVO_ISO_MARGINS")
    if path and len(MARGINS) == len(O.CASES):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"bound_cells": 2.0 ** -14, "nearest_vertex_cells": MARGINS}, fh, indent=1)


def test_crack_case():
    """open 3 x 2 x 130: two copies of one vertex, 1.2e-7 apart at grid z = 84.49987, fall on either side of the torch
    extractor's 1/4096 rounding and stay unmerged (388 vertices for 387 cut edges).  The edge-owned rule has no merge."""
    from nerf_vo_amd.meshing import marching_tetrahedra

    values, _, v, f = O.reference(O.CRACK)
    assert (v.shape[0], f.shape[0]) == (387, 462)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert np.unique(directed, axis=0).shape[0] == directed.shape[0], "a directed edge occurs twice"
    und, count = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    on_boundary = (np.abs(v.astype(np.float64)) >= 1.0 - 1e-6).any(axis=1)
    assert set(count.tolist()) <= {1, 2}
    open_edges = und[count == 1]
    assert on_boundary[open_edges].all(), "an edge inside the lattice that only one face uses: a crack"
    tv, tf = marching_tetrahedra(values, LOWER, UPPER, 0.0)
    print(f"crack case: oracle {v.shape[0]} vertices, torch extractor {tv.shape[0]} (387 cut edges)")
    assert tv.shape[0] == 388  # a record of the finding: marching_tetrahedra is left as it is


def test_empty_results():
    v, f = O.extract(np.full((4, 5, 3), -1.0, np.float32), np.zeros(3, np.float32), np.ones(3, np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int64
    v, f = O.extract(np.full((4, 5, 3), 2.0, np.float32), np.zeros(3, np.float32), np.ones(3, np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_generated_header_is_up_to_date():
    from nerf_vo_amd.meshing import iso_tables_header

    committed = open(os.path.join(ROOT, "nerf-vo_amd", "csrc", "iso_tables.h")).read()
    assert committed == iso_tables_header(), "run python tools/gen_iso_tables.py"


def test_winding_is_a_function_of_tetrahedron_and_case():
    """the exported table against marching_tetrahedra's own geometric test at cuts that are NOT the midpoints"""
    from nerf_vo_amd import meshing as M

    rng = np.random.default_rng(3)
    corners = M._CORNERS.double().numpy()
    for t in range(6):
        tp = corners[M._TETS[t].numpy()]
        for case in range(1, 15):
            pin = tp[int(M._INSIDE_REF[case])]
            for r in range(2):
                e = M._TABLE[case, r].numpy()
                if e[0, 0] < 0:
                    continue
                for _ in range(8):
                    w = rng.uniform(0.02, 0.98, size=(3, 1))
                    pts = tp[e[:, 0]] + w * (tp[e[:, 1]] - tp[e[:, 0]])
                    s = np.dot(np.cross(pts[1] - pts[0], pts[2] - pts[0]), pts.mean(axis=0) - pin)
                    assert (s < 0) == bool(M._WINDING[t, case, r])


def test_crop_and_transform_mesh():
    from nerf_vo_amd.meshing import crop_mesh, transform_mesh

    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 0.0, 0.0], [1.0, 1.0, 0.5], [0.5, 0.5, -0.25]])
    f = torch.tensor([[0, 1, 2], [1, 3, 2], [1, 4, 2], [4, 5, 0]])
    cv, cf, keep = crop_mesh(v, f, [0.0, 0.0, 0.0], [1.0, 1.0, 0.5])
    assert keep.tolist() == [True, True, True, False, True, False]  # (1, 1, 0.5) lies exactly on the bound: kept
    assert torch.equal(cv, v[[0, 1, 2, 4]])
    assert cf.tolist() == [[0, 1, 2], [1, 3, 2]]  # faces with a vertex outside are dropped, indices remapped, order kept
    ev, ef, _ = crop_mesh(v, f, [5.0, 5.0, 5.0], [6.0, 6.0, 6.0])
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    m = np.eye(4)
    m[:3, :3] = 2.0 * np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    m[:3, 3] = [0.5, -1.0, 3.0]
    out = transform_mesh(v, m)
    assert out.dtype == torch.float32
    p = v.double().numpy()
    expect = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)
    assert np.array_equal(out.numpy(), expect)
    assert out[1].tolist() == [0.5, 1.0, 3.0]


def test_extract_isosurface_rejects_cpu_tensor():
    from nerf_vo_amd.meshing import extract_isosurface

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_isosurface(torch.zeros(4, 4, 4), LOWER, UPPER, 0.0)


# ---- render_mesh(source='nerf'): the reference's box arithmetic ----
class _Dataset:
    camera_intrinsics = {"fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0, "height": 2, "width": 2, "depth_scale": 1000.0}
    evaluation_frames = [0]
    num_frames = 1

    def __init__(self, vertices, extrinsics_gt0, depth_gt):
        self._vertices = torch.from_numpy(np.asarray(vertices, dtype=np.float64))
        self.camera_extrinsics = [extrinsics_gt0]
        self._depth = depth_gt

    def frames_depth(self, mode="keyframes", keyframes=None):
        return [self._depth]

    def mesh(self):
        return (self._vertices, torch.zeros(0, 3, dtype=torch.long), None, None), "unused.ply"


class _RecordingNerf:
    def __init__(self, extrinsics_pred0, depth_pred, raw_mesh):
        self._pose, self._depth, self._raw = extrinsics_pred0, depth_pred, raw_mesh
        self.calls = []

    def get_camera_extrinsics(self, frame_index):
        return self._pose

    def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
        return self._depth

    def render_mesh(self, file_mesh, resolution, lower_bound, upper_bound):
        from nerf_vo_amd.meshing import write_mesh

        self.calls.append((file_mesh, np.asarray(resolution), np.asarray(lower_bound), np.asarray(upper_bound)))
        write_mesh(file_mesh, *self._raw)


def _renderer(tmp_path, gt_vertices, gt0, pred0, scale, raw_mesh):
    """the depth ratio the alignment estimates is within an ulp of ``scale``; the golden's own scale and matrix are then
    put in its place, as the generator handed them to the reference"""
    from nerf_vo_amd.evaluation import EvaluationRenderer

    depth_gt = np.full((2, 2), 2.0)
    nerf = _RecordingNerf(pred0, depth_gt / scale, raw_mesh)
    ds = _Dataset(gt_vertices, gt0, depth_gt)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=[0], dir_prediction=str(tmp_path / "pred"))
    est = renderer.pred2gt_transformation
    matrix = gt0 @ np.diag([scale, scale, scale, 1.0]) @ np.linalg.inv(pred0)
    np.testing.assert_allclose(est["scale_pred2gt"], scale, rtol=1e-14)
    np.testing.assert_allclose(est["matrix_pred2gt_scaled"], matrix, rtol=1e-12, atol=1e-14)
    renderer.pred2gt_transformation = dict(est, scale_pred2gt=scale, matrix_pred2gt_scaled=matrix)
    return renderer, nerf


def test_box_arithmetic_matches_the_reference(tmp_path):
    from nerf_vo_amd.meshing import read_mesh

    golden = np.load(os.path.join(ROOT, "tests", "golden", "mesh_from_nerf_golden.npz"))
    n_cases = int(golden["n_cases"])
    assert n_cases == 3
    for i in range(n_cases):
        gt_vertices, gt0, pred0, scale = golden[f"gt_vertices{i}"], golden[f"gt0_{i}"], golden[f"pred0_{i}"], float(golden[f"scale{i}"])
        # a raw mesh that survives the crop: one triangle around the centre of the ground-truth box, mapped to the model's frame
        centre = 0.5 * (gt_vertices.min(axis=0) + gt_vertices.max(axis=0))
        tri_gt = centre + 0.05 * np.eye(3)
        m = golden[f"matrix{i}"]
        tri_pred = (np.linalg.inv(m) @ np.concatenate([tri_gt, np.ones((3, 1))], axis=1).T).T[:, :3]
        raw = (torch.from_numpy(tri_pred.astype(np.float32)), torch.tensor([[0, 1, 2]]))
        sub = tmp_path / str(i)
        renderer, nerf = _renderer(sub, gt_vertices, gt0, pred0, scale, raw)
        assert np.array_equal(renderer.pred2gt_transformation["matrix_pred2gt_scaled"], m)
        assert np.array_equal(golden[f"transform{i}"], m)
        path = renderer.render_mesh(source="nerf")
        (file_mesh, resolution, lower, upper), = nerf.calls
        assert file_mesh.endswith("/mesh/mesh_from_nerf_raw.ply") and path.endswith("/mesh/mesh_from_nerf.ply")
        assert np.array_equal(np.asarray(resolution), golden[f"resolution{i}"]), (resolution, golden[f"resolution{i}"])
        np.testing.assert_allclose(lower, golden[f"lower_bound{i}"], rtol=1e-12)
        np.testing.assert_allclose(upper, golden[f"upper_bound{i}"], rtol=1e-12)
        np.testing.assert_allclose(gt_vertices.min(axis=0), golden[f"crop_lower{i}"], rtol=1e-12)
        np.testing.assert_allclose(gt_vertices.max(axis=0), golden[f"crop_upper{i}"], rtol=1e-12)
        v, f = read_mesh(path)[:2]
        assert v.shape == (3, 3) and f.tolist() == [[0, 1, 2]]
        np.testing.assert_allclose(v.numpy(), tri_gt, atol=1e-5)


def test_empty_crop_and_missing_render_mesh(tmp_path):
    from nerf_vo_amd.evaluation import EvaluationRenderer

    gt_vertices = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    far = (torch.tensor([[50.0, 50.0, 50.0], [51.0, 50.0, 50.0], [50.0, 51.0, 50.0]]), torch.tensor([[0, 1, 2]]))
    renderer, _ = _renderer(tmp_path, gt_vertices, np.eye(4), np.eye(4), 1.0, far)
    with pytest.raises(RuntimeError, match="thresh"):
        renderer.render_mesh(source="nerf")
    assert os.path.exists(tmp_path / "pred" / "mesh" / "mesh_from_nerf_raw.ply")
    assert not os.path.exists(tmp_path / "pred" / "mesh" / "mesh_from_nerf.ply")

    class _NoMesh:
        def get_camera_extrinsics(self, frame_index):
            return np.eye(4)

        def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
            return np.full((2, 2), 2.0)

    ds = _Dataset(gt_vertices, np.eye(4), np.full((2, 2), 2.0))
    bare = EvaluationRenderer(dataset=ds, nerf=_NoMesh(), keyframes=[0], dir_prediction=str(tmp_path / "bare"))
    with pytest.raises(NotImplementedError, match="compute_and_save_marching_cubes_mesh"):
        bare.render_mesh(source="nerf")
