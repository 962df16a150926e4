"""EvaluationRenderer.render_mesh(source='nerf') on the GPU: the plumbing with an analytic stand-in renderer (deterministic)
and the whole path on a trained occupancy-grid field (no quality bound: the training is not deterministic)."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HALF_EXTENT = (0.58, 0.45, 0.47)  # of the analytic box, ground-truth coordinates


def _ply_layout(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    n_vert = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_face = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l]
    return n_vert, n_face, props, len(body)


class _BoxNerf:
    """A model whose world is the ground truth's moved rigidly and shrunk by 1.25: depths are the ground truth's divided by
    1.25, the frame-0 pose is ``pred0``, and ``render_mesh`` extracts (with the HIP extractor) the surface of an analytic
    box given in ground-truth coordinates."""

    def __init__(self, dataset, keyframes, pred0, half_extent, device):
        self.dataset, self.keyframes, self.pred0, self.device = dataset, keyframes, pred0, device
        self.half_extent = torch.tensor(half_extent, dtype=torch.float64, device=device)
        gt0 = np.asarray(dataset.camera_extrinsics[keyframes[0]], dtype=np.float64)
        self.pred2gt = gt0 @ np.diag([1.25, 1.25, 1.25, 1.0]) @ np.linalg.inv(pred0)
        self.calls = []

    def get_camera_extrinsics(self, frame_index):
        assert frame_index == 0
        return self.pred0.copy()

    def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
        return self.dataset.render(self.dataset.camera_extrinsics[self.keyframes[frame_index]])[1] / 1.25

    def render_mesh(self, file_mesh, resolution, lower_bound, upper_bound):
        from nerf_vo_amd.meshing import extract_isosurface, write_mesh

        self.calls.append((file_mesh, np.asarray(resolution), np.asarray(lower_bound), np.asarray(upper_bound)))
        res = [int(r) for r in resolution]
        axes = [torch.linspace(float(lower_bound[x]), float(upper_bound[x]), res[x], dtype=torch.float64, device=self.device)
                for x in range(3)]
        p = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
        m = torch.as_tensor(self.pred2gt, device=self.device)
        p_gt = p @ m[:3, :3].T + m[:3, 3]
        values = (self.half_extent - p_gt.abs()).min(dim=-1).values.float()  # > 0 inside the box
        v, f = extract_isosurface(values, lower_bound, upper_bound, 0.0)
        write_mesh(file_mesh, v, f)


def test_plumbing_with_an_analytic_renderer(device, tmp_path):
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.meshing import read_mesh
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=72, width=96, scene_scale=0.25, device=device,
                                    dir_dataset=str(tmp_path / "dataset" / "room"))
    keyframes = list(range(0, 24, 4))
    a = 0.6
    pred0 = np.eye(4)
    pred0[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ \
        np.asarray(ds.camera_extrinsics[0])[:3, :3]
    pred0[:3, 3] = [0.3, -0.2, 0.15]
    # the room is [-0.5, 0.5]^3.  The model's frame is turned by 0.6 rad about z, so the lattice (the box of the mapped
    # corners) reaches beyond the ground-truth box on x and y and not on z: the analytic box lies inside the room on y and
    # z and sticks out on x, where the lattice holds a part of its faces that the crop has to cut
    nerf = _BoxNerf(ds, keyframes, pred0, HALF_EXTENT, device)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    t = renderer.pred2gt_transformation
    assert abs(t["scale_pred2gt"] - 1.25) < 1e-9
    np.testing.assert_allclose(t["matrix_pred2gt_scaled"], nerf.pred2gt, atol=1e-9)
    path = renderer.render_mesh(source="nerf")
    raw_path = str(tmp_path / "pred" / "mesh" / "mesh_from_nerf_raw.ply")
    assert path == str(tmp_path / "pred" / "mesh" / "mesh_from_nerf.ply") and os.path.exists(path) and os.path.exists(raw_path)
    (_, resolution, lower, upper), = nerf.calls
    assert resolution.dtype.kind == "i" and (resolution >= 64).all() and (upper > lower).all()

    gt_vertices = ds.mesh()[0][0].double().numpy()
    box_lo, box_hi = gt_vertices.min(axis=0), gt_vertices.max(axis=0)
    assert (box_hi < 0.56).all() and (box_lo > -0.56).all()
    v, f = read_mesh(path)[:2]
    rv, rf = read_mesh(raw_path)[:2]
    assert v.shape[0] > 1000 and f.shape[0] > 1000
    assert bool(((v.double().numpy() >= box_lo) & (v.double().numpy() <= box_hi)).all()), "a vertex outside the ground-truth box"
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    # the cropped mesh is the transformed raw mesh restricted to the box
    # (in float64, one product or sum per step in transform_mesh's order: a matrix product's summation order is the BLAS's)
    m, r64 = t["matrix_pred2gt_scaled"], rv.double().numpy()
    moved = np.stack([((m[r, 0] * r64[:, 0] + m[r, 1] * r64[:, 1]) + m[r, 2] * r64[:, 2]) + m[r, 3] for r in range(3)],
                     axis=1).astype(np.float32)
    keep = ((moved.astype(np.float64) >= box_lo) & (moved.astype(np.float64) <= box_hi)).all(axis=1)
    assert 0 < keep.sum() < keep.shape[0], "the crop cut nothing: the box does not stick out of the ground truth's"
    assert np.array_equal(v.numpy(), moved[keep])
    new_index = np.cumsum(keep) - 1
    rf = rf.numpy()
    assert np.array_equal(f.numpy(), new_index[rf[keep[rf].all(axis=1)]])
    # and lies on the analytic box, within the longest lattice edge: a linear cut of a piecewise linear field lies on the
    # edge it cuts, whose far end is at most a cube diagonal away -- sqrt(3) cells of at most (res + 1) / (res - 1) / 64
    # in ground-truth units at res >= 64, i.e. under 2 / 64
    d = np.abs(np.abs(v.double().numpy()) - np.array(HALF_EXTENT)).min(axis=1)
    assert d.max() < 2.0 / 64


def test_trained_field(device, tmp_path):
    """12 keyframes of 68 x 120, 400 steps, as tests/test_mapping_gpu.py::test_instant_ngp_mapper_end_to_end trains"""
    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator3D
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGP, InstantNGPRenderer
    from nerf_vo_amd.meshing import read_mesh
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    n, H, W, iters = 12, 68, 120, 400
    ds = SyntheticEvaluationDataset(num_frames=2 * n, height=H, width=W, scene_scale=0.2, device=device,
                                    dir_dataset=str(tmp_path / "dataset" / "room"))
    kf = list(range(0, 2 * n, 2))
    args = argparse.Namespace(num_keyframes=n, frame_height=H, frame_width=W, mapping_iterations=iters,
                              mapping_snapshot_iterations=iters, dir_prediction=str(tmp_path / "pred"))
    mapper = InstantNGP(args, device=device)
    frames = [ds.render(ds.camera_extrinsics[i]) for i in kf]
    color = torch.stack([torch.from_numpy(c) for c, _ in frames]).permute(0, 3, 1, 2).float() / 255.0
    depth = torch.stack([torch.from_numpy(d) for _, d in frames])[:, None].float().clamp(0.0, 5.0)
    ci = ds.camera_intrinsics
    intr = torch.tensor([ci["fx"], ci["fy"], ci["cx"], ci["cy"]])
    poses = torch.from_numpy(ds.camera_extrinsics[kf]).float()
    mapper(input={"keyframe_indices": torch.arange(n), "camera_intrinsics": intr.repeat(n, 1).to(device),
                  "camera_extrinsics": opencv_to_opengl(poses.to(device)), "frames_color": color.to(device),
                  "frames_depth": depth.to(device), "last_frame": True})
    while mapper.step < iters:
        mapper(input=None)
    mapper(input=None)
    assert mapper.is_shut_down
    renderer = EvaluationRenderer(dataset=ds, nerf=InstantNGPRenderer(mapping_model=mapper), keyframes=kf,
                                  dir_prediction=args.dir_prediction)
    path = renderer.render_mesh(source="nerf")
    raw_path = args.dir_prediction + "/mesh/mesh_from_nerf_raw.ply"
    assert os.path.exists(path) and os.path.exists(raw_path)
    n_vert, n_face, props, n_body = _ply_layout(raw_path)
    assert props == ["x", "y", "z"] and n_body == 12 * n_vert + 13 * n_face and n_vert > 0
    v, f = read_mesh(path)[:2]
    gt_vertices = ds.mesh()[0][0].double().numpy()
    assert v.shape[0] > 0 and f.shape[0] > 0 and int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    assert bool(((v.double().numpy() >= gt_vertices.min(axis=0)) & (v.double().numpy() <= gt_vertices.max(axis=0))).all())
    print(f"raw {n_vert} vertices {n_face} faces, cropped {v.shape[0]} / {f.shape[0]}, scale {renderer.pred2gt_transformation['scale_pred2gt']:.4f}")
    Evaluator3D(ds, args.dir_prediction, str(tmp_path / "results")).calculate_metrics_3d()
    import pandas as pd

    table = pd.read_csv(str(tmp_path / "results" / "metrics_3d.csv"))
    assert table["mesh"].tolist() == ["mesh_from_nerf"]
    row = table.iloc[0]
    print({k: float(row[k]) for k in ("accuracy", "completion", "precision", "recall", "f1score")})
    assert all(np.isfinite(float(row[k])) for k in ("accuracy", "completion", "precision", "recall", "f1score"))
