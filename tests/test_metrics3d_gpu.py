"""Nearest-neighbour kernel (nerf-vo_amd/csrc/nn.hip) behind pointcloud.NeighbourGrid.query, the ICP built on it and
evaluation.calculate_metrics_3d / Evaluator3D, against the restatements of tests/helpers/nn_oracle.py and the reference's
own kd-tree distances (tests/golden/metrics3d_golden.npz).

Bounds.  The search is compared BITWISE with the float32 brute force.  Against the stored cKDTree distances the bound is
1e-6 relative: the fp32 chain (one rounded subtraction per axis, three squares, two sums, one root) has a relative error
below 5 * 2^-24, about 3e-7.  For the ICP and the end-to-end metrics the bounds come from tests/helpers/nn_tolerances.py,
which measures on the CPU how far the float64 helper moves when only its distance rule is replaced by the kernel's float32
rule (same scenes as here):
  * ICP scene: max |T_fp32rule - T_f64| = 0.0 (5 iterations both; no correspondence flips on this scene).  Ten times
    that is zero, which float64 arithmetic in another summation order cannot meet: the HIP-backed ICP sums its Kabsch
    terms with torch on the device, the helper with numpy.  The bound is therefore the float64 floor, 1e-10: sums of
    about 1100 terms carry a relative error of at most 1100 * 2^-53 = 1.2e-13, the 3x3 SVD of the well-conditioned
    covariance of a box surface amplifies it by less than 10, and five composed updates stay below 1e-11.
  * metrics of the room meshes (clouds of 3768 and 4304 points): |accuracy| 1.6e-13, |completion| 2.4e-12, precision,
    recall and f1score 0.  Bounds: ten times these, 1.6e-12 and 2.4e-11; the three shares must be equal.
"""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import nn_oracle
from helpers.nn_cases import icp_scene, planted_motion, room_meshes, search_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics3d_golden.npz")
ICP_BOUND = 1e-10
METRIC_BOUNDS = {"accuracy": 1.6e-12, "completion": 2.4e-11, "precision": 0.0, "recall": 0.0, "f1score": 0.0}
CASES = search_cases()


@functools.lru_cache(maxsize=None)
def _brute(name):
    c = CASES[name]
    return nn_oracle.nn_brute(c["queries"], c["points"], c.get("max_distance"), c.get("transform"))


def _query(device, c, cell_size=None):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    grid = NeighbourGrid(torch.from_numpy(c["points"]).to(device), c["cell_size"] if cell_size is None else cell_size)
    d2, idx = grid.query(torch.from_numpy(c["queries"]).to(device), max_distance=c.get("max_distance"), transform=c.get("transform"))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64
    return d2.cpu().numpy(), idx.cpu().numpy(), grid


@pytest.mark.parametrize("name", list(CASES))
def test_search_is_bitwise_the_brute_force(device, name):
    c = CASES[name]
    d2, idx, grid = _query(device, c)
    ref_d2, ref_idx = _brute(name)
    misses = int((ref_idx < 0).sum())
    print(f"{name}: grid {grid.dims}, {c['queries'].shape[0]} queries x {c['points'].shape[0]} points, {misses} without a hit, "
          f"{int((d2.view(np.uint32) != ref_d2.view(np.uint32)).sum())} dist2 and {int((idx != ref_idx).sum())} indices differ")
    assert np.array_equal(d2.view(np.uint32), ref_d2.view(np.uint32))
    assert np.array_equal(idx, ref_idx)
    if "max_distance" in c:
        n = c["queries"].shape[0]
        assert 0.25 * n < misses < 0.75 * n or name == "transform_bounded", "about half of the bounded queries have no hit"
        assert np.isposinf(d2[idx < 0]).all() and (idx[d2 == np.inf] == -1).all()
        assert (d2[idx >= 0] <= np.float32(c["max_distance"]) ** 2).all()
    if name == "duplicates_and_exact":
        assert (d2[:4] == 0).all() and idx[:4].tolist() == [5, 120, 110, 49], "ties go to the smallest index"
    if name == "sparse_many_rings":
        assert (np.sqrt(d2) > 10 * c["cell_size"]).sum() > 20, "some queries need more than ten rings"
    if name == "outside":
        assert d2[8] > 90.0 ** 2


def test_cell_size_does_not_change_the_result(device):
    c = CASES["surface_cell_0.0312"]
    ref = _brute("surface_cell_0.0312")
    for cell_size in (1 / 64, 1 / 32, 0.11, 0.3, 5.0):
        d2, idx, grid = _query(device, c, cell_size)
        assert np.array_equal(d2.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(idx, ref[1]), f"cell {cell_size} {grid.dims}"


def test_non_finite_queries_are_refused(device):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    grid = NeighbourGrid(torch.rand(100, 3, device=device), 0.1)
    q = torch.rand(10, 3, device=device)
    q[3, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or infinite"):
        grid.query(q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.query(torch.rand(10, 3))


@pytest.mark.parametrize("pair", [0, 1])
def test_distances_match_the_reference_kdtree(device, pair):
    """Both queries of the reference's calculate_metrics_3d on the stored clouds: |sqrt(dist2) - d_ref| <= 1e-6 d_ref, and the
    point the index names is as near as the reference's nearest point.  No exclusions."""
    from nerf_vo_amd.pointcloud import NeighbourGrid

    g = np.load(GOLDEN)
    for queries, target, key in ((g[f"gt{pair}"], g[f"pred{pair}"], f"pred_to_gt{pair}"), (g[f"pred{pair}"], g[f"gt{pair}"], f"gt_to_pred{pair}")):
        d_ref = g["d_" + key]
        d2, idx = NeighbourGrid(torch.from_numpy(target).to(device)).query(torch.from_numpy(queries).to(device))
        d = np.sqrt(d2.double().cpu().numpy())
        idx = idx.cpu().numpy()
        via_index = np.linalg.norm(queries.astype(np.float64) - target.astype(np.float64)[idx], axis=1)
        print(f"{key}: max relative error of sqrt(dist2) {np.max(np.abs(d - d_ref) / d_ref):.3e}, through the index "
              f"{np.max(np.abs(via_index - d_ref) / d_ref):.3e}, indices equal to cKDTree's {np.mean(idx == g['i_' + key]):.4f}")
        assert (np.abs(d - d_ref) <= 1e-6 * d_ref).all()
        assert (np.abs(via_index - d_ref) <= 1e-6 * d_ref).all()


def test_icp_matches_the_float64_helper(device):
    """Planted motion: 1 degree about a skew axis and 5 mm.  Measured on the CPU: the helper with the float32 distance rule
    equals the float64 helper exactly on this scene; bound 1e-10 (module docstring)."""
    from nerf_vo_amd.pointcloud import icp_point_to_point

    source, target = icp_scene()
    ref_T, ref_fitness, ref_rmse, ref_iterations = nn_oracle.icp(source, target)
    T, fitness, rmse, iterations = icp_point_to_point(torch.from_numpy(source).to(device), torch.from_numpy(target).to(device))
    err = ref_T @ np.linalg.inv(planted_motion())
    print(f"icp: {iterations} iterations (helper {ref_iterations}), fitness {fitness} ({ref_fitness}), rmse {rmse:.9f} ({ref_rmse:.9f}), "
          f"max |T - T_helper| {np.abs(T - ref_T).max():.3e}; helper vs planted: {np.abs(err - np.eye(4)).max():.3e}")
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert np.abs(err - np.eye(4)).max() < 1e-3, "the helper recovers the planted motion"
    assert iterations == ref_iterations and fitness == ref_fitness
    assert abs(rmse - ref_rmse) <= 1e-6 * ref_rmse  # (root of a mean of float32 squares against float64 ones)
    assert np.abs(T - ref_T).max() <= ICP_BOUND


def test_icp_without_correspondences_keeps_the_transform(device):
    from nerf_vo_amd.pointcloud import icp_point_to_point

    src = torch.rand(200, 3, device=device)
    T, fitness, rmse, iterations = icp_point_to_point(src, src + 10.0)
    assert np.array_equal(T, np.eye(4)) and fitness == 0.0 and iterations == 1


@functools.lru_cache(maxsize=None)
def _room_clouds_and_reference():
    from nerf_vo_amd.evaluation import sample_metric_clouds

    mesh_gt, mesh_pred = room_meshes()
    gt, pred = sample_metric_clouds(mesh_gt, mesh_pred, seed=0, device="cpu")
    return gt, pred, nn_oracle.metrics_from_clouds(gt.numpy(), pred.numpy())


def test_metrics_3d_end_to_end(device):
    """The room and the room with every face 1 cm further out, the reference's constants (200 000 samples, voxel 1/64,
    threshold 0.05): the float64 helper pipeline on the same clouds, bounds in the module docstring."""
    from nerf_vo_amd.evaluation import METRICS_3D, calculate_metrics_3d, sample_metric_clouds

    mesh_gt, mesh_pred = room_meshes()
    gt, pred, ref = _room_clouds_and_reference()
    on_gpu = sample_metric_clouds(mesh_gt, mesh_pred, seed=0, device=device)
    # float64 sampling arithmetic may differ in the last bit between devices: float32 positions within an ulp
    assert on_gpu[0].shape == gt.shape and float((on_gpu[0].cpu() - gt).abs().max()) <= 2.0 ** -24
    m = calculate_metrics_3d(mesh_gt, mesh_pred, seed=0, device=device)
    print("metrics", m, "helper", ref, "differences", {k: abs(m[k] - ref[k]) for k in ref})
    assert tuple(m) == METRICS_3D
    assert m["precision"] == 1.0 and m["recall"] == 1.0
    assert 0.009 < m["accuracy"] < 0.013 and 0.009 < m["completion"] < 0.013  # faces 1 cm apart
    for k, bound in METRIC_BOUNDS.items():
        assert abs(m[k] - ref[k]) <= bound, k


def test_evaluator_3d_writes_the_table(device, tmp_path):
    import pandas as pd

    from nerf_vo_amd.evaluation import METRICS_3D, Evaluator3D
    from nerf_vo_amd.meshing import write_mesh

    (gt_v, gt_f), (pred_v, pred_f) = room_meshes()
    mesh_dir = tmp_path / "pred" / "mesh"
    mesh_dir.mkdir(parents=True)
    write_mesh(str(mesh_dir / "mesh_from_evaluation_frames.ply"), torch.from_numpy(pred_v), torch.from_numpy(pred_f))
    write_mesh(str(mesh_dir / "mesh_from_keyframes.ply"), torch.from_numpy(gt_v), torch.from_numpy(gt_f),
               colors=torch.zeros(8, 3, dtype=torch.uint8))
    write_mesh(str(mesh_dir / "mesh_from_nerf_raw.ply"), torch.from_numpy(pred_v) * 3, torch.from_numpy(pred_f))
    write_mesh(str(mesh_dir / "ignored.obj"), torch.from_numpy(pred_v), torch.from_numpy(pred_f))

    class Dataset:
        def mesh(self):
            return (torch.from_numpy(gt_v), torch.from_numpy(gt_f), None, None), "unused"

    out = Evaluator3D(Dataset(), str(tmp_path / "pred"), str(tmp_path / "results"), device=device).calculate_metrics_3d()
    table = pd.read_csv(tmp_path / "results" / "metrics_3d.csv")
    assert list(table.columns) == list(METRICS_3D) + ["mesh"]
    assert table["mesh"].tolist() == ["mesh_from_evaluation_frames", "mesh_from_keyframes"]
    assert set(out) == set(METRICS_3D)
    assert (table["precision"] == 1.0).all() and (table["recall"] == 1.0).all()
    assert 0.009 < table["accuracy"][0] < 0.013 and table["accuracy"][1] < 0.009  # the second mesh IS the ground truth
