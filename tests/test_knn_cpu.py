"""CPU side of the k-NN search and the point cloud built on it: the brute-force oracle of tests/helpers/knn_oracle.py on
hand-made cases, the outlier rule (oracle and pointcloud.statistical_outlier_mask) on clouds whose answer is known by
construction, the .ply round trip of a face-less cloud, normal re-orientation and normals under a scaled rigid transform,
and the cell-size rule.  The search itself has no CPU form (tests/test_knn_gpu.py)."""
import numpy as np
import pytest
import torch

from helpers import knn_oracle


def test_oracle_five_collinear_points():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [6, 0, 0], [10, 0, 0]], dtype=np.float32)
    d2, idx = knn_oracle.knn_brute(pts, pts, 3)
    assert idx.tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 2, 4], [4, 3, 2]]
    assert d2.tolist() == [[0, 1, 9], [0, 1, 4], [0, 4, 9], [0, 9, 16], [0, 16, 49]]
    mean = knn_oracle.mean_distance(d2, idx)
    assert mean.dtype == np.float32
    assert mean.tolist() == [np.float32(4) / np.float32(3), 1.0, np.float32(5) / np.float32(3), np.float32(7) / np.float32(3),
                             np.float32(11) / np.float32(3)]


def test_oracle_triple_duplicate_ties_go_to_the_smaller_index():
    pts = np.array([[5, 5, 5], [1, 2, 3], [1, 2, 3], [0, 0, 0], [1, 2, 3]], dtype=np.float32)
    d2, idx = knn_oracle.knn_brute(np.array([[1, 2, 3], [1, 2, 4]], dtype=np.float32), pts, 2)
    assert idx.tolist() == [[1, 2], [1, 2]] and d2.tolist() == [[0, 0], [1, 1]]
    d2, idx = knn_oracle.knn_brute(np.array([[1, 2, 3]], dtype=np.float32), pts, 4)
    assert idx.tolist() == [[1, 2, 4, 3]] and d2.tolist() == [[0, 0, 0, 14]]


def test_oracle_pads_when_there_are_fewer_points_than_k():
    pts = np.array([[0, 0, 0], [0, 3, 4]], dtype=np.float32)
    d2, idx = knn_oracle.knn_brute(np.array([[0, 0, 0]], dtype=np.float32), pts, 4)
    assert idx.tolist() == [[0, 1, -1, -1]]
    assert d2[0, :2].tolist() == [0, 25] and np.isposinf(d2[0, 2:]).all()
    assert knn_oracle.mean_distance(d2, idx).tolist() == [2.5], "the mean runs over min(k, M) = 2 entries"


def _line_with_outlier():
    return np.array([[float(x), 0, 0] for x in range(10)] + [[100.0, 0, 0]], dtype=np.float32)


def test_outlier_rule_on_a_cloud_with_a_known_answer():
    """Ten points one unit apart and one 91 units beyond: with 2 neighbours (the point itself and its nearest) every
    average is 0.5 and the far point's is 45.5, so mean = 50.5 / 11 and std = sqrt((10 * (0.5 - mean)^2 + (45.5 - mean)^2) / 10)."""
    from nerf_vo_amd.pointcloud import statistical_outlier_mask

    pts = _line_with_outlier()
    kept, avg, threshold = knn_oracle.remove_statistical_outlier(pts, nb_neighbors=2, std_ratio=1.0)
    assert avg.tolist() == [0.5] * 10 + [45.5]
    mean = 50.5 / 11
    std = np.sqrt((10 * (0.5 - mean) ** 2 + (45.5 - mean) ** 2) / 10)
    assert abs(threshold - (mean + std)) < 1e-12 and 18.0 < threshold < 18.3
    assert kept.tolist() == list(range(10))
    kept10, _, threshold10 = knn_oracle.remove_statistical_outlier(pts, nb_neighbors=2, std_ratio=10.0)
    assert kept10.tolist() == list(range(11)) and abs(threshold10 - (mean + 10 * std)) < 1e-11
    # the package's rule on the same averages
    for ratio, want in ((1.0, kept), (10.0, kept10)):
        keep, thr = statistical_outlier_mask(torch.from_numpy(avg), ratio)
        assert keep.nonzero().flatten().tolist() == want.tolist()
        assert abs(thr - knn_oracle.outlier_rule(avg, ratio)[1]) < 1e-12


def test_outlier_rule_ignores_and_drops_zero_averages():
    from nerf_vo_amd.pointcloud import statistical_outlier_mask

    avg = np.array([0.0, 0.5, 0.5, 0.0, 0.7], dtype=np.float32)  # two points whose neighbours are all duplicates of them
    keep, threshold, mean, std = knn_oracle.outlier_rule(avg, 10.0)
    a = avg.astype(np.float64)
    assert abs(mean - (a[1] + a[2] + a[4]) / 3) < 1e-15 and keep.tolist() == [False, True, True, False, True]
    assert abs(std - np.sqrt(((a[[1, 2, 4]] - mean) ** 2).sum() / 2)) < 1e-15
    got, thr = statistical_outlier_mask(torch.from_numpy(avg), 10.0)
    assert got.tolist() == keep.tolist() and abs(thr - threshold) < 1e-12
    for bad in (np.zeros(4, np.float32), np.array([0, 0, 0.3], np.float32)):
        with pytest.raises(ValueError):
            knn_oracle.outlier_rule(bad, 10.0)
        with pytest.raises(ValueError, match="at least 2"):
            statistical_outlier_mask(torch.from_numpy(bad), 10.0)


def test_outlier_scene_of_the_gpu_test():
    """The cloud tests/test_knn_gpu.py removes outliers from: the oracle drops exactly the 12 planted points at std_ratio 10
    and at 2, with a wide gap between the surface's and the planted points' averages on both sides of the threshold."""
    pts, planted = knn_oracle.outlier_scene()
    assert pts.shape == (3012, 3) and planted.sum() == 12
    d2, idx = knn_oracle.knn_brute(pts, pts, 20)
    avg = knn_oracle.mean_distance(d2, idx)
    for ratio in (10.0, 2.0):
        keep, threshold, _, _ = knn_oracle.outlier_rule(avg, ratio)
        print(f"std_ratio {ratio}: threshold {threshold:.4f}, largest surface average {avg[~planted].max():.4f}, "
              f"smallest planted average {avg[planted].min():.4f}")
        assert np.array_equal(keep, ~planted)
        assert (np.abs(avg.astype(np.float64) - threshold) > 1e-6 * threshold).all()
        assert avg[~planted].max() < 0.6 * threshold and avg[planted].min() > 1.03 * threshold


def test_ply_round_trip_of_a_faceless_cloud(tmp_path):
    from nerf_vo_amd.meshing import read_mesh, write_mesh

    rng = np.random.default_rng(3)
    pts = torch.from_numpy(rng.normal(size=(37, 3)).astype(np.float32))
    nrm = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(37, 3)).astype(np.float32)), dim=1)
    col = torch.from_numpy(rng.integers(0, 256, (37, 3)).astype(np.uint8))
    path = str(tmp_path / "cloud.ply")
    write_mesh(path, pts, torch.zeros(0, 3, dtype=torch.int64), colors=col, normals=nrm)
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert "element vertex 37" in lines and "element face 0" in lines
    assert [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(body) == 27 * 37
    v, f, c, n = read_mesh(path)
    assert torch.equal(v, pts) and torch.equal(n, nrm) and torch.equal(c, col)
    assert f.shape == (0, 3) and f.dtype == torch.int64


def test_normals_are_turned_towards_the_cameras():
    from nerf_vo_amd.mapping.renderer import orient_normals_towards_cameras

    view = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    nrm = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, 0.8, 0.0], [1.0, 0.0, 0.0]])
    out = orient_normals_towards_cameras(nrm, view)
    # facing the camera: kept; along the ray: negated; perpendicular (dot == 0): kept
    want = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [-0.6, -0.8, 0.0], [1.0, 0.0, 0.0]])
    assert torch.equal(out, want)  # (-0.0 == 0.0)
    assert bool(((out * view).sum(dim=1) <= 0).all())


def test_normals_under_a_scaled_rigid_transform():
    from nerf_vo_amd.evaluation import rotate_normals

    a, scale = 0.6, 1.25
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    m = np.eye(4)
    m[:3, :3] = scale * rot
    m[:3, 3] = [3.0, -2.0, 7.0]  # the translation does not move a direction
    rng = np.random.default_rng(1)
    n = rng.normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = rotate_normals(torch.from_numpy(n.astype(np.float32)), m, scale)
    assert out.dtype == torch.float32
    want = n.astype(np.float32).astype(np.float64) @ rot.T
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(out.double().numpy() - want).max() < 1e-7
    assert np.abs(np.linalg.norm(out.double().numpy(), axis=1) - 1).max() < 1e-6
    assert out[0].tolist() != n[0].tolist()


def test_cell_size_rule():
    """sqrt(factor * k * area / n) for a surface-like cloud, raised to keep the grid within its caps."""
    from nerf_vo_amd import _lib
    from nerf_vo_amd.pointcloud import knn_cell_size

    cell = knn_cell_size(200000, (2.0, 1.6, 1.0), 20, factor=1.0)
    area = 2 * (2.0 * 1.6 + 1.6 * 1.0 + 2.0 * 1.0)
    assert abs(cell - np.sqrt(20 * area / 200000)) < 1e-12
    assert knn_cell_size(200000, (2.0, 1.6, 0.0), 20) > 0 and knn_cell_size(5, (0.0, 0.0, 0.0), 20) > 0
    # 34 million points over 20 m: the rule's 7 mm cells would need 2700 per axis
    wide = knn_cell_size(34000000, (20.0, 10.0, 3.0), 20)
    assert 20.0 / wide + 1 <= _lib.NN_MAX_CELLS_PER_AXIS
    small = knn_cell_size(34000000, (20.0, 10.0, 3.0), 20, max_cells=2 ** 20)
    assert (20.0 / small + 1) * (10.0 / small + 1) * (3.0 / small + 1) <= 2 ** 20
