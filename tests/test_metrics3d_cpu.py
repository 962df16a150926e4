"""CPU side of the 3-D mesh metrics: the metrics tail against the reference's own numbers
(tests/golden/metrics3d_golden.npz, made by make_golden_metrics3d.py), .ply round trips, voxel down-sampling and surface
sampling against their restatements (tests/helpers/nn_oracle.py), and argument errors.  The search itself needs the GPU:
tests/test_metrics3d_gpu.py."""
import os

import numpy as np
import pytest
import torch

from helpers import nn_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics3d_golden.npz")


def test_metrics_tail_matches_the_reference():
    from nerf_vo_amd.evaluation import METRICS_3D, metrics_3d_from_distances

    g = np.load(GOLDEN)
    names = [str(n) for n in g["metric_names"]]
    assert sorted(METRICS_3D) == names
    strictly_inside = 0
    for i in range(2):
        m = metrics_3d_from_distances(g[f"d_gt_to_pred{i}"], g[f"d_pred_to_gt{i}"])
        np.testing.assert_allclose([m[k] for k in names], g[f"metrics{i}"], rtol=1e-12, atol=0)
        strictly_inside += 0 < m["precision"] < 1 and 0 < m["recall"] < 1
        assert nn_oracle.metrics_tail(g[f"d_gt_to_pred{i}"], g[f"d_pred_to_gt{i}"]) == pytest.approx(m, rel=1e-12)
    assert strictly_inside >= 1


def test_oracle_distances_match_the_reference_kdtree():
    """The brute-force float64 helper against the stored cKDTree results: the helper is a fair reference for the rest."""
    g = np.load(GOLDEN)
    d, i = nn_oracle.nn_brute_f64(g["pred1"], g["gt1"])
    np.testing.assert_allclose(d, g["d_gt_to_pred1"], rtol=1e-12)
    assert (i == g["i_gt_to_pred1"]).mean() > 0.999  # (exact ties may resolve differently)


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_read_mesh_round_trip(tmp_path, with_colors, with_normals):
    from nerf_vo_amd.meshing import read_mesh, write_mesh

    rng = np.random.default_rng(3)
    v = torch.from_numpy(rng.normal(size=(57, 3)).astype(np.float32))
    f = torch.from_numpy(rng.integers(0, 57, (101, 3)))
    c = torch.from_numpy(rng.integers(0, 256, (57, 3)).astype(np.uint8)) if with_colors else None
    n = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(57, 3)).astype(np.float32)), dim=1) if with_normals else None
    path = str(tmp_path / "m.ply")
    write_mesh(path, v, f, colors=c, normals=n)
    rv, rf, rc, rn = read_mesh(path)
    assert rv.dtype == torch.float32 and torch.equal(rv, v)
    assert rf.dtype == torch.int64 and torch.equal(rf, f)
    assert (rc is None) == (c is None) and (c is None or (rc.dtype == torch.uint8 and torch.equal(rc, c)))
    assert (rn is None) == (n is None) and (n is None or torch.equal(rn, n))


def test_read_mesh_rejects_what_it_does_not_read(tmp_path):
    from nerf_vo_amd.meshing import read_mesh, write_mesh

    v, f = torch.rand(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]])
    obj = str(tmp_path / "m.obj")
    write_mesh(obj, v, f)
    with pytest.raises(ValueError, match="not a .ply"):
        read_mesh(obj)
    ascii_ply = tmp_path / "a.ply"
    ascii_ply.write_text("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                         "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError, match="binary_little_endian"):
        read_mesh(str(ascii_ply))
    good = str(tmp_path / "g.ply")
    write_mesh(good, v, f)
    data = open(good, "rb").read()
    cut = tmp_path / "cut.ply"
    cut.write_bytes(data[:-5])
    with pytest.raises(ValueError, match="truncated"):
        read_mesh(str(cut))
    extra = tmp_path / "extra.ply"
    extra.write_bytes(data.replace(b"property float z\n", b"property float z\nproperty float quality\n"))
    with pytest.raises(ValueError, match="vertex properties"):
        read_mesh(str(extra))


def test_voxel_down_sample_matches_the_helper():
    """Empty voxels, voxels with many points, negative coordinates, a point exactly on a lattice plane.  Bound: the result
    is the float32 rounding of a float64 mean (2^-24 relative to the largest coordinate, 1.3) plus float64 summation
    noise: 2^-23 * 1.3."""
    from nerf_vo_amd.pointcloud import voxel_down_sample

    rng = np.random.default_rng(5)
    voxel = 1 / 16
    crowd = (np.array([-0.71, 0.33, -1.2]) + 0.01 * rng.random((300, 3)))  # one voxel, 300 points
    spread = rng.uniform(-1.3, 1.3, (900, 3))                              # mostly one point per voxel, most voxels empty
    on_plane = np.array([[-0.25, 0.5, -1.0], [-0.2501, 0.5001, -1.0001]])
    pts = np.concatenate([spread, crowd, on_plane]).astype(np.float32)
    pts = pts[rng.permutation(pts.shape[0])]
    ref = nn_oracle.voxel_down_sample(pts, voxel)
    out = voxel_down_sample(torch.from_numpy(pts), voxel)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert ref.shape[0] < pts.shape[0] - 250
    err = np.abs(out.double().numpy() - ref).max()
    print(f"voxel_down_sample: {pts.shape[0]} -> {ref.shape[0]} points, max |err| {err:.3e}")
    assert err <= 2.0 ** -23 * 1.3
    # the stated order: ascending voxel index, x most significant
    cells = np.floor(out.double().numpy() / voxel).astype(np.int64)
    keys = [tuple(c) for c in cells]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def _big_small_mesh():
    """Triangle 0 has 100x the area of each of the triangles 1..4 (all in different planes z = k)."""
    v, f = [], []
    for k, s in enumerate([10.0, 1.0, 1.0, 1.0, 1.0]):
        v += [[0, 0, k], [s, 0, k], [0, s, k]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


def test_sample_points_uniformly_lies_on_the_mesh_and_follows_area():
    """n = 40 000 samples; a triangle of area share p receives Binomial(n, p) samples: the 5-sigma band is
    n p +- 5 sqrt(n p (1 - p)), i.e. 38 462 +- 192 for the large triangle (p = 100/104) and 385 +- 98 for each small one."""
    from nerf_vo_amd.pointcloud import sample_points_uniformly

    v, f = _big_small_mesh()
    n = 40000
    pts = sample_points_uniformly(v, f, n, generator=torch.Generator().manual_seed(1))
    assert pts.shape == (n, 3) and pts.dtype == torch.float32
    again = sample_points_uniformly(v, f, n, generator=torch.Generator().manual_seed(1))
    assert torch.equal(pts, again)
    tri = pts[:, 2].round().long()
    assert float((pts[:, 2] - tri).abs().max()) <= 1e-6, "every sample lies in the plane of a triangle"
    size = torch.tensor([10.0, 1.0, 1.0, 1.0, 1.0])[tri]
    x, y = pts[:, 0].double(), pts[:, 1].double()
    assert bool((x >= -1e-6).all() and (y >= -1e-6).all() and (x + y <= size.double() * (1 + 1e-6)).all()), "inside its triangle"
    counts = torch.bincount(tri, minlength=5).double().numpy()
    p = np.array([100.0, 1, 1, 1, 1]) / 104.0
    band = 5 * np.sqrt(n * p * (1 - p))
    print("samples per triangle", counts, "expected", n * p, "+-", band)
    assert (np.abs(counts - n * p) <= band).all()
    # uniform inside the large triangle: the centroid of its samples is (s/3, s/3) within 5 sigma (sigma^2 = s^2 / 18 / count)
    big = tri == 0
    sigma = 10.0 / np.sqrt(18.0 * counts[0])
    assert abs(float(x[big].mean()) - 10 / 3) <= 5 * sigma and abs(float(y[big].mean()) - 10 / 3) <= 5 * sigma


def test_argument_errors():
    from nerf_vo_amd.pointcloud import NeighbourGrid, icp_point_to_point, voxel_down_sample

    pts = torch.rand(50, 3)
    bad = pts.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or infinite"):
        NeighbourGrid(bad, 0.1)
    with pytest.raises(ValueError, match="NaN or infinite"):
        voxel_down_sample(bad, 0.1)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        NeighbourGrid(torch.rand(5, 2), 0.1)
    with pytest.raises(ValueError, match="cell_size of at least"):  # 2000 cells along x
        NeighbourGrid(torch.tensor([[0.0, 0, 0], [20.0, 0.1, 0.1]]), 0.01)
    with pytest.raises(ValueError, match="cell_size of at least"):  # 600^3 cells in all
        NeighbourGrid(torch.tensor([[0.0, 0, 0], [6.0, 6.0, 6.0]]), 0.01)
    grid = NeighbourGrid(pts, 0.1)  # building the grid is plain torch
    assert int(grid.cell_start[-1]) == 50 and sorted(grid.point_index.tolist()) == list(range(50))
    assert bool((grid.cell_start[1:] >= grid.cell_start[:-1]).all())
    assert torch.equal(grid.cells_of(grid.points), torch.sort(grid.cells_of(pts)).values)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.query(torch.rand(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        icp_point_to_point(torch.rand(10, 3), pts)


def test_icp_helper_recovers_the_planted_motion():
    """The scene of the GPU ICP test is sound: the float64 helper alone finds the planted motion (rotation within
    0.05 degrees, translation within 0.5 mm; the clouds are different noisy samples of one surface)."""
    from helpers.nn_cases import icp_scene, planted_motion

    source, target = icp_scene()
    T, fitness, rmse, iterations = nn_oracle.icp(source, target)
    err = T @ np.linalg.inv(planted_motion())
    angle = np.degrees(np.arccos(np.clip((np.trace(err[:3, :3]) - 1) / 2, -1, 1)))
    print(f"helper ICP: {iterations} iterations, fitness {fitness:.4f}, rmse {rmse:.5f}, rotation error {angle:.4f} deg, "
          f"translation error {np.linalg.norm(err[:3, 3]) * 1e3:.3f} mm")
    assert fitness > 0.95 and angle < 0.05 and np.linalg.norm(err[:3, 3]) < 5e-4
