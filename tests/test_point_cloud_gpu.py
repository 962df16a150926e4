"""EvaluationRenderer.render_point_cloud on the GPU: the plumbing with an analytic stand-in renderer (deterministic) and the
whole path -- rays, field, k-NN outlier removal, re-orientation, transform, crop, score -- on a trained nerfacto field (no
quality bound: the training is not deterministic)."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HALF_EXTENT = (0.58, 0.45, 0.47)  # of the analytic box, ground-truth coordinates
CAMERA = (0.1, -0.05, 0.08)       # the one camera of the stand-in, inside the box, ground-truth coordinates
METRICS = ("accuracy", "completion", "precision", "recall", "f1score")


def _ply_layout(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    n_vert = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_face = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l]
    return n_vert, n_face, props, len(body)


def _transform_rows(m, p64):
    """transform_mesh's rule in numpy float64: one product or sum per step."""
    return np.stack([((m[r, 0] * p64[:, 0] + m[r, 1] * p64[:, 1]) + m[r, 2] * p64[:, 2]) + m[r, 3] for r in range(3)], axis=1)


class _BoxCloudNerf:
    """A model whose world is the ground truth's moved rigidly and shrunk by 1.25 (as _BoxNerf of
    test_mesh_from_nerf_gpu.py).  ``render_point_cloud`` returns seeded points on the surface of an analytic box given in
    ground-truth coordinates, seen from one camera inside it, with the faces' OUTWARD normals turned by the package's
    re-orientation rule (so they end up inward, towards the camera), all mapped into the model's frame."""

    def __init__(self, dataset, keyframes, pred0):
        self.dataset, self.keyframes, self.pred0 = dataset, keyframes, pred0
        gt0 = np.asarray(dataset.camera_extrinsics[keyframes[0]], dtype=np.float64)
        self.pred2gt = gt0 @ np.diag([1.25, 1.25, 1.25, 1.0]) @ np.linalg.inv(pred0)
        self.calls = []

    def get_camera_extrinsics(self, frame_index):
        assert frame_index == 0
        return self.pred0.copy()

    def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
        return self.dataset.render(self.dataset.camera_extrinsics[self.keyframes[frame_index]])[1] / 1.25

    def render_point_cloud(self, file_point_cloud, lower_bound, upper_bound, num_points, **kwargs):
        from nerf_vo_amd.mapping.renderer import orient_normals_towards_cameras
        from nerf_vo_amd.meshing import write_mesh

        self.calls.append((file_point_cloud, np.asarray(lower_bound), np.asarray(upper_bound), int(num_points), kwargs))
        rng = np.random.default_rng(17)
        half = np.asarray(HALF_EXTENT)
        p = rng.uniform(-half, half, size=(num_points, 3))
        axis, side = rng.integers(0, 3, num_points), rng.integers(0, 2, num_points)
        rows = np.arange(num_points)
        p[rows, axis] = np.where(side == 0, -half[axis], half[axis])
        outward = np.zeros((num_points, 3))
        outward[rows, axis] = np.where(side == 0, -1.0, 1.0)
        view = p - np.asarray(CAMERA)
        view /= np.linalg.norm(view, axis=1, keepdims=True)
        normal_gt = orient_normals_towards_cameras(torch.from_numpy(outward), torch.from_numpy(view)).numpy()
        assert np.array_equal(normal_gt, -outward), "a camera inside the box sees every face from behind its outward normal"
        rot = self.pred2gt[:3, :3] / 1.25
        inv = np.linalg.inv(self.pred2gt)
        p_model = (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        inside = ((p_model > np.asarray(lower_bound)) & (p_model < np.asarray(upper_bound))).all(axis=1)
        self.normal_gt, self.view_gt = normal_gt[inside], view[inside]
        write_mesh(file_point_cloud, torch.from_numpy(p_model[inside]), torch.zeros(0, 3, dtype=torch.int64),
                   colors=torch.from_numpy(rng.integers(0, 256, (num_points, 3)).astype(np.uint8)[inside]),
                   normals=torch.from_numpy((normal_gt @ rot).astype(np.float32)[inside]))  # n_model = R^T n_gt


def _stand_in_scene(device, tmp_path):
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=72, width=96, scene_scale=0.25, device=device,
                                    dir_dataset=str(tmp_path / "dataset" / "room"))
    keyframes = list(range(0, 24, 4))
    a = 0.6
    pred0 = np.eye(4)
    pred0[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ \
        np.asarray(ds.camera_extrinsics[0])[:3, :3]
    pred0[:3, 3] = [0.3, -0.2, 0.15]
    return ds, keyframes, pred0


def test_plumbing_with_an_analytic_renderer(device, tmp_path):
    """The room is [-0.5, 0.5]^3 and the model's frame is turned by 0.6 rad about z: the analytic box sticks out of the
    ground truth's box on x, where the crop has to cut."""
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.meshing import read_mesh

    ds, keyframes, pred0 = _stand_in_scene(device, tmp_path)
    nerf = _BoxCloudNerf(ds, keyframes, pred0)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    t = renderer.pred2gt_transformation
    assert abs(t["scale_pred2gt"] - 1.25) < 1e-9
    path = renderer.render_point_cloud(num_points=6000)
    raw_path = str(tmp_path / "pred" / "pointcloud" / "pointcloud_from_nerf_raw.ply")
    assert path == str(tmp_path / "pred" / "pointcloud" / "pointcloud_from_nerf.ply") and os.path.exists(path) and os.path.exists(raw_path)
    assert not os.path.exists(str(tmp_path / "pred" / "mesh")), "the cloud stays out of mesh/: Evaluator3D reads that folder as meshes"
    (_, lower, upper, n_asked, _), = nerf.calls
    assert n_asked == 6000 and (upper > lower).all()
    for file in (path, raw_path):
        n_vert, n_face, props, n_body = _ply_layout(file)
        assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and n_face == 0 and n_body == 27 * n_vert

    gt_vertices = ds.mesh()[0][0].double().numpy()
    box_lo, box_hi = gt_vertices.min(axis=0), gt_vertices.max(axis=0)
    v, f, c, n = read_mesh(path)
    rv, _, rc, rn = read_mesh(raw_path)
    assert f.shape == (0, 3) and v.shape[0] > 1000
    assert bool(((v.double().numpy() >= box_lo) & (v.double().numpy() <= box_hi)).all()), "a point outside the ground-truth box"
    # the final cloud is the transformed raw cloud restricted to the box (float64 row by row, as transform_mesh)
    m = np.asarray(t["matrix_pred2gt_scaled"], dtype=np.float64)
    moved = _transform_rows(m, rv.double().numpy()).astype(np.float32)
    keep = ((moved.astype(np.float64) >= box_lo) & (moved.astype(np.float64) <= box_hi)).all(axis=1)
    print(f"raw {rv.shape[0]} points, {int(keep.sum())} inside the ground-truth box")
    assert 0 < keep.sum() < keep.shape[0], "the crop cut nothing: the box does not stick out of the ground truth's"
    assert np.array_equal(v.numpy(), moved[keep])
    assert np.array_equal(c.numpy(), rc.numpy()[keep])
    # normals: unit, the analytic ones after the mapping, none facing away from its view direction
    n64 = n.double().numpy()
    unit_err = np.abs(np.linalg.norm(n64, axis=1) - 1.0).max()
    analytic_err = np.abs(n64 - nerf.normal_gt[keep]).max()
    print(f"normals: | |n| - 1 | <= {unit_err:.2e} (bound 1e-6), |n - analytic| <= {analytic_err:.2e} (bound 1e-5)")
    assert unit_err <= 1e-6 and analytic_err <= 1e-5
    assert ((n64 * nerf.view_gt[keep]).sum(axis=1) <= 0).all()
    # and the points lie on the analytic box: float32 positions through two float64 maps
    assert np.abs(np.abs(v.double().numpy()) - np.array(HALF_EXTENT)).min(axis=1).max() < 1e-6


def test_renderer_without_a_point_cloud_is_refused(device, tmp_path):
    from nerf_vo_amd.evaluation import EvaluationRenderer

    ds, keyframes, pred0 = _stand_in_scene(device, tmp_path)
    nerf = _BoxCloudNerf(ds, keyframes, pred0)
    nerf.render_point_cloud = None  # like the occupancy-grid renderer: no such method
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    with pytest.raises(NotImplementedError, match="no normals"):
        renderer.render_point_cloud(num_points=100)


def test_trained_field(device, tmp_path):
    """12 keyframes of 68 x 120 through the Nerfstudio mapper, 400 steps (as tests/test_mapping_gpu.py trains its
    end-to-end runs), then the cloud of 20 000 points and its score."""
    import pandas as pd

    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator3D
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.nerfstudio_mapper import Nerfstudio
    from nerf_vo_amd.mapping.renderer import NerfstudioRenderer
    from nerf_vo_amd.meshing import read_mesh
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    n, H, W, iters, num_points = 12, 68, 120, 400, 20000
    ds = SyntheticEvaluationDataset(num_frames=2 * n, height=H, width=W, device=device, dir_dataset=str(tmp_path / "dataset" / "room"))
    kf = list(range(0, 2 * n, 2))
    args = argparse.Namespace(experiment="pointcloud", dir_prediction=str(tmp_path / "pred"), mapping_snapshot_iterations=iters,
                              mapping_iterations=iters, num_keyframes=n, frame_height=H, frame_width=W, enhancement_module="depth",
                              deterministic=False, dynamic_loss_scale=None, camera_optimizer_mode=None)
    mapper = Nerfstudio(args, device=device)
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
    pipeline = mapper.trainer.pipeline
    assert pipeline.model.config.predict_normals
    nerf = NerfstudioRenderer(mapping_model=mapper)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=kf, dir_prediction=args.dir_prediction)
    state_before = pipeline.datamanager.generator.get_state().clone()
    default_before = torch.cuda.get_rng_state(device).clone()
    path = renderer.render_point_cloud(num_points=num_points)
    assert torch.equal(pipeline.datamanager.generator.get_state(), state_before), "the export advanced the training stream"
    assert torch.equal(torch.cuda.get_rng_state(device), default_before), "the export drew from torch's default generator"
    raw_path = args.dir_prediction + "/pointcloud/pointcloud_from_nerf_raw.ply"
    assert os.path.exists(path) and os.path.exists(raw_path)
    n_raw, n_face, props, n_body = _ply_layout(raw_path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and n_face == 0 and n_body == 27 * n_raw
    assert num_points // 2 <= n_raw <= num_points, "at most num_points and at least half of them survive the outlier removal"
    v, f, c, nrm = read_mesh(path)
    gt_vertices = ds.mesh()[0][0].double().numpy()
    assert 0 < v.shape[0] <= num_points and f.shape[0] == 0 and c.shape == v.shape
    assert bool(((v.double().numpy() >= gt_vertices.min(axis=0)) & (v.double().numpy() <= gt_vertices.max(axis=0))).all())
    assert float((torch.linalg.norm(nrm.double(), dim=1) - 1.0).abs().max()) <= 1e-6
    print(f"raw {n_raw} of {num_points} points after outlier removal, {v.shape[0]} inside the ground-truth box, "
          f"scale {renderer.pred2gt_transformation['scale_pred2gt']:.4f}")

    # the same seed on the same field: the same file, bit for bit; and the re-orientation rule on the cloud itself
    lower, upper = renderer._ground_truth_box_in_model_frame()[3:]
    raw_bytes = open(raw_path, "rb").read()
    again = nerf.render_point_cloud(str(tmp_path / "again.ply"), lower, upper, num_points=num_points)
    assert open(str(tmp_path / "again.ply"), "rb").read() == raw_bytes, "a second export with the same seed differs"
    assert again["kept"] == n_raw and again["generated"] == num_points
    # camera-facing: the file's normals (the same bytes as this export's) against the directions of the rays that saw the
    # points (1e-6: a dot product of exactly opposite sign, summed in another order on the host)
    rv, _, _, rn = read_mesh(raw_path)
    assert torch.equal(rv, again["points"]) and torch.equal(rn, again["normals"])
    assert float((torch.linalg.norm(again["view_directions"].double(), dim=1) - 1.0).abs().max()) <= 1e-6, "unit ray directions"
    assert float((rn * again["view_directions"]).sum(dim=1).max()) <= 1e-6, "a normal that faces away from the ray that saw it"
    assert float((torch.linalg.norm(rn.double(), dim=1) - 1.0).abs().max()) <= 1e-6
    other = nerf.render_point_cloud(str(tmp_path / "other.ply"), lower, upper, num_points=num_points, seed=1, remove_outliers=False)
    assert other["kept"] == other["generated"] == num_points and not torch.equal(other["points"][:100], again["points"][:100])

    Evaluator3D(ds, args.dir_prediction, str(tmp_path / "results")).calculate_metrics_3d_clouds()
    table = pd.read_csv(str(tmp_path / "results" / "metrics_3d_pointcloud.csv"))
    assert list(table.columns) == list(METRICS) + ["mesh"] and table["mesh"].tolist() == ["pointcloud_from_nerf"]
    row = table.iloc[0]
    print({k: float(row[k]) for k in METRICS})
    assert all(np.isfinite(float(row[k])) for k in METRICS)
    assert not os.path.exists(str(tmp_path / "results" / "metrics_3d.csv")), "metrics_3d.csv belongs to calculate_metrics_3d"
