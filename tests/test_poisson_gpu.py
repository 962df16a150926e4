"""Dense-lattice Poisson reconstruction on the GPU (csrc/poisson.hip behind nerf_vo_amd/poisson.py): every operator and the
whole solve bit for bit against the float32 oracle of tests/helpers/poisson_oracle.py; the meshes of the sphere and the
rooms against the bounds of profiles/poisson_parity_margins.json (2 x the oracle's worst vertex); the plumbing through
EvaluationRenderer.render_mesh(source='nerf') with an analytic stand-in renderer; a trained nerfacto field."""
import argparse
import os

import numpy as np
import pytest
import torch

from helpers import poisson_cases as cases
from helpers import poisson_oracle as O

pytestmark = pytest.mark.gpu

METRICS = ("accuracy", "completion", "precision", "recall", "f1score")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got: torch.Tensor, want, what):
    g, w = _bits(got.detach().cpu().numpy()), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ from the float32 oracle, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("case", cases.OPERATOR_CASES, ids=cases.case_id)
def test_operators_bit_for_bit(device, case):
    """Splat (1 and 3 channels), sample, divergence, half-sweeps of both colours, residual + restriction, prolongation +
    correction, the residual norm, and the solve of 8 cycles with the final chi."""
    from nerf_vo_amd import poisson as P

    lat = cases.case_lattice(case)
    ref = cases.case_oracle(case, "f32")
    points, normals = cases.case_cloud(case)
    pts = torch.from_numpy(points).to(device)
    order, cell_start = P.bin_points(pts, lat)
    ref_order, ref_start = O.bin_points(points, lat)
    assert np.array_equal(order.cpu().numpy(), ref_order) and np.array_equal(cell_start.cpu().numpy(), ref_start)
    pts_s = pts[order].contiguous()
    nrm_s = torch.from_numpy(normals).to(device)[order].contiguous()

    W = P.splat(pts_s, cell_start, lat)
    _same_bits(W, ref["W"], "density splat")
    D = P.sample(W, pts_s, lat)
    _same_bits(D[:, 0], ref["D"], "density at the points")
    assert float(D.min()) >= 0.125 * (1 - 1e-5), "a point's own sum of w^2 is at least 1/8"
    V = P.splat(pts_s, cell_start, lat, values=nrm_s, denom=D)
    _same_bits(V, ref["V"], "vector field splat")
    _same_bits(P.sample(V, pts_s, lat), O.sample(ref["V"], ref["points"], lat, np.float32), "3-channel sample")
    # a splat of plain values (the colour pass), C = 3, no denominator
    values = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=points.shape).astype(np.float32)).to(device)
    _same_bits(P.splat(pts_s, cell_start, lat, values=values), O.splat(ref["points"], lat, np.float32, values=values.cpu().numpy()), "colour splat")
    f = P.divergence(V)
    _same_bits(f, ref["f"], "divergence")

    # the stencil operators on a field that is not smooth: a few sweeps into the solve
    chi_ref = np.zeros_like(ref["f"])
    chi = torch.zeros_like(f)
    for color in (0, 1, 0, 1, 1, 0):
        O.sweep(chi_ref, ref["f"], color)
        P.sweep(chi, f, color)
        _same_bits(chi, chi_ref, f"half-sweep of colour {color}")
    coarse = P.restrict(chi, f)
    coarse_ref = O.restrict(chi_ref, ref["f"])
    _same_bits(coarse, coarse_ref, "residual + restriction")
    P.prolong(chi, coarse)  # any coarse field with a zero boundary serves as a correction
    O.prolong(chi_ref, coarse_ref)
    _same_bits(chi, chi_ref, "prolongation + correction")
    assert float(chi[0].abs().max()) == 0 and float(chi[:, 0].abs().max()) == 0 and float(chi[:, :, -1].abs().max()) == 0

    solved, start, norms = P.solve(f, lat["levels"], 8)
    _same_bits(solved, ref["chi"], "chi after 8 V(2,2) cycles")
    assert np.float32(start) == np.float32(ref["start"]) and [np.float32(x) for x in norms] == [np.float32(x) for x in ref["norms"]]
    again, _, norms_again = P.solve(f, lat["levels"], 8)
    assert torch.equal(solved, again) and norms == norms_again, "two runs give the same bytes"
    _same_bits(P.sample(solved, pts_s, lat)[:, 0], O.sample(ref["chi"], ref["points"], lat, np.float32)[:, 0], "chi at the points")


def _reconstruct_scene(device, name, **kwargs):
    from nerf_vo_amd.poisson import poisson_reconstruct

    p, n, face, lower, upper, depth = cases.scene(name)
    colors = None
    if face is not None:
        colors = torch.from_numpy(_FACE_COLORS[face]).to(device)
    out = poisson_reconstruct(torch.from_numpy(p).to(device), torch.from_numpy(n).to(device), colors, lower=lower, upper=upper,
                              depth=depth, **kwargs)
    return out, face


_FACE_COLORS = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [240, 240, 20], [20, 240, 240], [240, 20, 240]], np.uint8)


@pytest.mark.parametrize("name", cases.SCENES)
def test_scene_geometry(device, name):
    recorded = cases.load_margins()["geometry"][name]
    bound = recorded["geometry_bound_voxels"]
    (v, f, c, info), face = _reconstruct_scene(device, name)
    h = info["lattice"]["h"]
    assert list(info["lattice"]["nodes"]) == recorded["nodes"]
    dist = cases.scene_distance(name, v.cpu().numpy(), h)
    print(f"{name}: {info['vertices']} of {info['vertices_before']} vertices kept at density >= {info['density_threshold']:.3f}, worst "
          f"{dist.max():.4f} voxel (bound {bound:.4f} = 2 x the oracle's {recorded['oracle_worst_kept_voxels']:.4f}); residual "
          f"{info['residual'][-1] / info['residual_start']:.2e} of the start")
    assert v.shape[0] > 1000 and f.shape[0] > 1000 and int(f.max()) < v.shape[0] and int(f.min()) >= 0
    assert dist.max() <= bound, "a kept vertex beyond the bound"
    assert info["residual"][-1] <= 1e-4 * info["residual_start"]
    # a second run: the same bytes
    (v2, f2, c2, _), _ = _reconstruct_scene(device, name)
    assert torch.equal(v, v2) and torch.equal(f, f2) and (c is None or torch.equal(c, c2))

    tri = v[f].double()
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    centroid = tri.mean(dim=1)
    if name == "sphere":
        # nothing is trimmed with trim_quantile = 0 (every density is far above the floor): the surface is closed
        (vs, fs, _, info_s), _ = _reconstruct_scene(device, name, trim_quantile=0.0)
        assert info_s["vertices"] == info_s["vertices_before"] and info_s["faces"] == info_s["faces_before"]
        edges = torch.cat([fs[:, [0, 1]], fs[:, [1, 2]], fs[:, [2, 0]]]).sort(dim=1).values
        _, counts = torch.unique(edges, dim=0, return_counts=True)
        assert bool((counts == 2).all()), "every edge of the sphere lies in exactly two faces"
        outward = centroid - torch.tensor(cases.SPHERE_CENTRE, dtype=torch.float64, device=device)
        sign = (normal * outward).sum(dim=1)
        area = torch.linalg.norm(normal, dim=1)
        assert bool((sign[area > 0] > 0).all()), "face normals point out of the sphere, as the points' normals do"
    else:
        # the rooms' normals point inwards: so do the faces' (away from the nearest wall's outside)
        inward = torch.tensor(cases.ROOM_CENTRE, dtype=torch.float64, device=device) - centroid
        big = torch.linalg.norm(normal, dim=1) > 0.25 * h * h
        flat = (centroid - torch.tensor(cases.ROOM_CENTRE, dtype=torch.float64, device=device)).abs().max(dim=1)
        along = normal[torch.arange(normal.shape[0]), flat.indices] * torch.sign(inward[torch.arange(normal.shape[0]), flat.indices])
        middle = big & (flat.values > cases.ROOM_HALF - 1.5 * h) & ((centroid - torch.tensor(cases.ROOM_CENTRE, dtype=torch.float64,
                        device=device)).abs().sort(dim=1).values[:, 1] < cases.ROOM_HALF - 4 * h)
        assert int(middle.sum()) > 1000 and bool((along[middle] > 0).all()), "face normals agree with the walls' inward normals"
        # colours: away from the room's edges a vertex has its wall's colour within one level
        vc = v.double().cpu().numpy() - np.asarray(cases.ROOM_CENTRE)
        wall_axis = np.abs(vc).argmax(axis=1)
        second = np.sort(np.abs(vc), axis=1)[:, 1]
        wall = 2 * wall_axis + (vc[np.arange(vc.shape[0]), wall_axis] > 0)
        inner = (second < cases.ROOM_HALF - 3 * h) & (np.abs(vc).max(axis=1) > cases.ROOM_HALF - 1.5 * h)
        got = c.cpu().numpy().astype(np.int64)[inner]
        off = np.abs(got - _FACE_COLORS[wall[inner]].astype(np.int64)).max()
        print(f"{name}: {int(inner.sum())} vertices away from the edges, colour off by at most {off} level(s)")
        assert inner.sum() > 1000 and off <= 1
    if name == "room_five_faces":
        (v0, _, _, info0), _ = _reconstruct_scene(device, name, min_density=0.0)
        d0 = cases.scene_distance(name, v0.cpu().numpy(), h)
        print(f"{name}: with min_density = 0 the threshold is {info0['density_threshold']:.3f}, {info0['vertices']} vertices, worst "
              f"{d0.max():.2f} voxels from every wall")
        assert d0.max() > 5.0, "without the floor the quantile leaves the sheets in unobserved space"
        assert info["density_threshold"] == 1.0


# ---- plumbing: EvaluationRenderer.render_mesh(source='nerf') over a stand-in renderer ---------------------------------
HALF_EXTENT = (0.58, 0.45, 0.47)  # of the analytic box, ground-truth coordinates


def _ply_layout(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    n_vert = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_face = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l]
    return n_vert, n_face, props, len(body)


class _BoxMeshNerf:
    """A model whose world is the ground truth's moved rigidly and shrunk by 1.25 (as _BoxCloudNerf of
    test_point_cloud_gpu.py).  ``render_mesh`` reconstructs seeded points on the surface of an analytic box given in
    ground-truth coordinates, normals towards the inside (a room seen from within), mapped into the model's frame."""

    def __init__(self, dataset, keyframes, pred0, device):
        self.dataset, self.keyframes, self.pred0, self.device = dataset, keyframes, pred0, device
        gt0 = np.asarray(dataset.camera_extrinsics[keyframes[0]], dtype=np.float64)
        self.pred2gt = gt0 @ np.diag([1.25, 1.25, 1.25, 1.0]) @ np.linalg.inv(pred0)
        self.calls = []

    def get_camera_extrinsics(self, frame_index):
        assert frame_index == 0
        return self.pred0.copy()

    def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
        return self.dataset.render(self.dataset.camera_extrinsics[self.keyframes[frame_index]])[1] / 1.25

    def render_mesh(self, file_mesh, resolution, lower_bound, upper_bound, num_points=40000, depth=5, **kwargs):
        from nerf_vo_amd.meshing import write_mesh
        from nerf_vo_amd.poisson import poisson_reconstruct

        self.calls.append((file_mesh, np.asarray(resolution), np.asarray(lower_bound), np.asarray(upper_bound), num_points, depth, kwargs))
        rng = np.random.default_rng(17)
        half = np.asarray(HALF_EXTENT)
        p = rng.uniform(-half, half, size=(num_points, 3))
        axis, side = rng.integers(0, 3, num_points), rng.integers(0, 2, num_points)
        rows = np.arange(num_points)
        p[rows, axis] = np.where(side == 0, -half[axis], half[axis])
        inward = np.zeros((num_points, 3))
        inward[rows, axis] = np.where(side == 0, 1.0, -1.0)
        rot = self.pred2gt[:3, :3] / 1.25
        inv = np.linalg.inv(self.pred2gt)
        p_model = (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        inside = ((p_model > np.asarray(lower_bound)) & (p_model < np.asarray(upper_bound))).all(axis=1)
        colors = rng.integers(0, 256, (num_points, 3)).astype(np.uint8)
        v, f, c, self.info = poisson_reconstruct(torch.from_numpy(p_model[inside]).to(self.device),
                                                 torch.from_numpy((inward @ rot).astype(np.float32)[inside]).to(self.device),
                                                 torch.from_numpy(colors[inside]).to(self.device), lower=lower_bound,
                                                 upper=upper_bound, depth=depth, **kwargs)
        write_mesh(file_mesh, v, f, colors=c)


def test_plumbing_with_an_analytic_renderer(device, tmp_path):
    import pandas as pd

    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator3D
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
    nerf = _BoxMeshNerf(ds, keyframes, pred0, device)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    path = renderer.render_mesh(source="nerf", num_points=30000, depth=5, cycles=6)
    raw_path = str(tmp_path / "pred" / "mesh" / "mesh_from_nerf_raw.ply")
    assert path == str(tmp_path / "pred" / "mesh" / "mesh_from_nerf.ply") and os.path.exists(path) and os.path.exists(raw_path)
    (_, _, lower, upper, n_asked, depth, kwargs), = nerf.calls
    assert n_asked == 30000 and depth == 5 and kwargs == {"cycles": 6} and (upper > lower).all(), "the arguments reach the renderer"
    assert len(nerf.info["residual"]) == 6
    for file in (path, raw_path):
        n_vert, n_face, props, n_body = _ply_layout(file)
        assert props == ["x", "y", "z", "red", "green", "blue"] and n_face > 0 and n_body == 15 * n_vert + 13 * n_face
    gt_vertices = ds.mesh()[0][0].double().numpy()
    box_lo, box_hi = gt_vertices.min(axis=0), gt_vertices.max(axis=0)
    v, f, c, _ = read_mesh(path)
    rv, rf, rc, _ = read_mesh(raw_path)
    assert v.shape[0] > 1000 and f.shape[0] > 1000 and c.shape == v.shape
    assert bool(((v.double().numpy() >= box_lo) & (v.double().numpy() <= box_hi)).all()), "a vertex outside the ground-truth box"
    assert 0 < v.shape[0] < rv.shape[0], "the analytic box sticks out of the ground truth's: the crop cuts"
    # the colours travel with their vertices through the transform and the crop
    m = np.asarray(renderer.pred2gt_transformation["matrix_pred2gt_scaled"], dtype=np.float64)
    r64 = rv.double().numpy()
    moved = np.stack([((m[r, 0] * r64[:, 0] + m[r, 1] * r64[:, 1]) + m[r, 2] * r64[:, 2]) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)
    keep = ((moved.astype(np.float64) >= box_lo) & (moved.astype(np.float64) <= box_hi)).all(axis=1)
    assert np.array_equal(v.numpy(), moved[keep]) and np.array_equal(c.numpy(), rc.numpy()[keep])
    # the surface is the analytic box: within two of the lattice's voxels, in ground-truth units
    h_gt = nerf.info["lattice"]["h"] * 1.25
    off = np.abs(np.abs(v.double().numpy()) - np.array(HALF_EXTENT)).min(axis=1).max()
    print(f"{v.shape[0]} of {rv.shape[0]} vertices inside the ground-truth box, at most {off / h_gt:.3f} voxel from the analytic box")
    assert off <= 2.0 * h_gt

    Evaluator3D(ds, str(tmp_path / "pred"), str(tmp_path / "results")).calculate_metrics_3d()
    table = pd.read_csv(str(tmp_path / "results" / "metrics_3d.csv")).set_index("mesh")
    assert "mesh_from_nerf" in table.index
    row = table.loc["mesh_from_nerf"]
    print({k: float(row[k]) for k in METRICS})
    assert all(np.isfinite(float(row[k])) for k in METRICS)


def test_trained_field(device, tmp_path):
    """12 keyframes of 68 x 120 through the Nerfstudio mapper, 400 steps (as test_trained_field of
    tests/test_point_cloud_gpu.py), then the mesh of the field itself from 60 000 points at depth 6.  No quality bound: the
    training is not deterministic."""
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.nerfstudio_mapper import Nerfstudio
    from nerf_vo_amd.mapping.renderer import NerfstudioRenderer
    from nerf_vo_amd.meshing import read_mesh
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    n, H, W, iters = 12, 68, 120, 400
    ds = SyntheticEvaluationDataset(num_frames=2 * n, height=H, width=W, device=device, dir_dataset=str(tmp_path / "dataset" / "room"))
    kf = list(range(0, 2 * n, 2))
    args = argparse.Namespace(experiment="poisson", dir_prediction=str(tmp_path / "pred"), mapping_snapshot_iterations=iters,
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
    nerf = NerfstudioRenderer(mapping_model=mapper)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=kf, dir_prediction=args.dir_prediction)
    state_before = pipeline.datamanager.generator.get_state().clone()
    default_before = torch.cuda.get_rng_state(device).clone()
    path = renderer.render_mesh(source="nerf", num_points=60000, depth=6)
    assert torch.equal(pipeline.datamanager.generator.get_state(), state_before), "the export advanced the training stream"
    assert torch.equal(torch.cuda.get_rng_state(device), default_before), "the export drew from torch's default generator"
    raw_path = args.dir_prediction + "/mesh/mesh_from_nerf_raw.ply"
    assert os.path.exists(path) and os.path.exists(raw_path)
    n_vert, n_face, props, n_body = _ply_layout(raw_path)
    assert props == ["x", "y", "z", "red", "green", "blue"] and n_face > 0 and n_vert > 0 and n_body == 15 * n_vert + 13 * n_face
    v, f, c, _ = read_mesh(path)
    assert v.shape[0] > 0 and f.shape[0] > 0 and c.shape == v.shape
    print(f"raw mesh {n_vert} vertices / {n_face} faces, {v.shape[0]} / {f.shape[0]} inside the ground-truth box")
    # the same seed on the same field: the same file, bit for bit
    lower, upper = renderer._ground_truth_box_in_model_frame()[3:]
    info = nerf.render_mesh(str(tmp_path / "again.ply"), None, lower, upper, num_points=60000, depth=6)
    assert open(str(tmp_path / "again.ply"), "rb").read() == open(raw_path, "rb").read(), "a second export with the same seed differs"
    assert info["generated"] == 60000 and info["vertices"] == n_vert and info["faces"] == n_face and len(info["residual"]) == 8
    print(f"lattice {info['lattice']['nodes']}, L = {info['lattice']['levels']}; residual {info['residual'][-1] / info['residual_start']:.2e} "
          f"of the start; {info['vertices']} of {info['vertices_before']} vertices at density >= {info['density_threshold']:.3f}")

    pipeline.model.config.predict_normals = False
    with pytest.raises(RuntimeError, match="predict_normals=False"):
        nerf.render_mesh(str(tmp_path / "none.ply"), None, lower, upper, num_points=100, depth=4)
    pipeline.model.config.predict_normals = True
