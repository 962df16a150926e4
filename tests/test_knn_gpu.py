"""k-nearest-neighbour kernel (nerf-vo_amd/csrc/knn.hip) behind pointcloud.NeighbourGrid.query_knn and
pointcloud.remove_statistical_outlier, against the brute force of tests/helpers/knn_oracle.py.

Bounds.  Every (dist2, index) table is compared with np.array_equal and every mean distance as BITS: the contract is the
brute force's result, not a tolerance.  The outlier-removal test compares kept indices; the float64 cloud statistics may
differ from numpy's in summation order by a relative 1e-15, so the test first asserts, on the ORACLE's values, that no
average lies within 1e-6 relative of the threshold -- that gap is what makes the masks comparable.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import knn_oracle
from helpers.nn_cases import search_cases, surface_cloud

pytestmark = pytest.mark.gpu

CASES = search_cases()
SURFACES = [n for n in CASES if n.startswith("surface_cell_")]


@functools.lru_cache(maxsize=None)
def _brute(name, k, n_targets=None):
    c = CASES[name]
    return knn_oracle.knn_brute(c["queries"], c["points"][:n_targets], k)


def _query(device, points, queries, cell_size, k, want="table"):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    grid = NeighbourGrid(torch.from_numpy(points).to(device), cell_size)
    out = grid.query_knn(torch.from_numpy(queries).to(device), k, want=want)
    if want == "mean":
        assert out.dtype == torch.float32 and out.shape == (queries.shape[0],)
        return out.cpu().numpy()
    d2, idx = out
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64 and d2.shape == idx.shape == (queries.shape[0], k)
    return d2.cpu().numpy(), idx.cpu().numpy()


def _assert_table(got, ref, what):
    d2, idx = got
    print(f"{what}: {int((d2.view(np.uint32) != ref[0].view(np.uint32)).sum())} dist2 and {int((idx != ref[1]).sum())} indices "
          f"of {idx.size} differ")
    assert np.array_equal(d2.view(np.uint32), ref[0].view(np.uint32)), what
    assert np.array_equal(idx, ref[1]), what


@pytest.mark.parametrize("k", [2, 3])
def test_ties_at_the_cut_go_to_the_smaller_index(device, k):
    c = CASES["duplicates_and_exact"]
    ref = _brute("duplicates_and_exact", k)
    ref3 = _brute("duplicates_and_exact", 3)
    tied = int((ref3[0][:, 1] == ref3[0][:, 2]).sum())
    assert tied >= 90, f"{tied} queries have the 2nd and 3rd neighbour at equal dist2"
    _assert_table(_query(device, c["points"], c["queries"], c["cell_size"], k), ref, f"duplicates k={k}")


def test_termination_is_on_the_kth_entry(device):
    c = CASES["sparse_many_rings"]
    ref = _brute("sparse_many_rings", 32)
    far = np.sqrt(ref[0][:, 31]) > 2 * np.sqrt(ref[0][:, 29])
    assert far.mean() > 0.15, "for many queries the 32nd neighbour is more than twice as far as the 30th"
    _assert_table(_query(device, c["points"], c["queries"], c["cell_size"], 32), ref, "sparse k=32")


def test_same_data_three_cell_sizes(device):
    ref = _brute(SURFACES[0], 20)
    assert CASES[SURFACES[0]]["queries"].shape[0] == 1037 and len(SURFACES) == 3
    for name in SURFACES:
        c = CASES[name]
        _assert_table(_query(device, c["points"], c["queries"], c["cell_size"], 20), ref, f"{name} k=20")


def test_k1_is_the_1nn_kernel(device):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    c = CASES[SURFACES[1]]
    d2, idx = _query(device, c["points"], c["queries"], c["cell_size"], 1)
    one_d2, one_idx = NeighbourGrid(torch.from_numpy(c["points"]).to(device), c["cell_size"]).query(torch.from_numpy(c["queries"]).to(device))
    assert np.array_equal(d2[:, 0].view(np.uint32), one_d2.cpu().numpy().view(np.uint32))
    assert np.array_equal(idx[:, 0], one_idx.cpu().numpy())


def test_padding_single_target(device):
    c = CASES["single_target"]
    d2, idx = _query(device, c["points"], c["queries"], c["cell_size"], 20)
    _assert_table((d2, idx), _brute("single_target", 20), "single target k=20")
    assert (idx[:, 0] == 0).all() and (idx[:, 1:] == -1).all() and np.isposinf(d2[:, 1:]).all()


def test_padding_five_targets(device):
    c = CASES["surface_cell_0.0312"]
    d2, idx = _query(device, c["points"][:5], c["queries"][:130], 1 / 8, 20)
    ref = knn_oracle.knn_brute(c["queries"][:130], c["points"][:5], 20)
    _assert_table((d2, idx), ref, "five targets k=20")
    assert (idx[:, :5] >= 0).all() and (idx[:, 5:] == -1).all() and np.isposinf(d2[:, 5:]).all()
    mean = _query(device, c["points"][:5], c["queries"][:130], 1 / 8, 20, want="mean")
    assert np.array_equal(mean.view(np.uint32), knn_oracle.mean_distance(*ref).view(np.uint32)), "mean over min(k, M) = 5 entries"


def test_one_cell_k32_and_k40_rejected(device):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    c = CASES["one_cell"]
    assert c["points"].shape[0] == 40
    _assert_table(_query(device, c["points"], c["queries"], c["cell_size"], 32), _brute("one_cell", 32), "one cell k=32")
    grid = NeighbourGrid(torch.from_numpy(c["points"]).to(device), c["cell_size"])
    with pytest.raises(ValueError, match="between 1 and 32"):
        grid.query_knn(torch.from_numpy(c["queries"]).to(device), 40)


@pytest.mark.parametrize("k", [8, 24, 32])
def test_m_equals_k(device, k):
    c = CASES["one_cell"]
    d2, idx = _query(device, c["points"][:k], c["queries"], c["cell_size"], k)
    _assert_table((d2, idx), _brute("one_cell", k, k), f"M == k == {k}")
    assert (idx >= 0).all() and (np.sort(idx, axis=1) == np.arange(k)).all()


@pytest.mark.parametrize("name", ["planar", "outside"])
def test_degenerate_grids_and_queries(device, name):
    c = CASES[name]
    _assert_table(_query(device, c["points"], c["queries"], c["cell_size"], 8), _brute(name, 8), f"{name} k=8")


@functools.lru_cache(maxsize=None)
def _self_cloud():
    pts = surface_cloud(np.random.default_rng(5), 3000)
    pts[100:110] = pts[40:50]  # some exact duplicates: entry 0 may then be the lower-indexed twin
    return pts, knn_oracle.knn_brute(pts, pts, 20)


def test_self_query(device):
    pts, ref = _self_cloud()
    d2, idx = _query(device, pts, pts, 1 / 16, 20)
    _assert_table((d2, idx), ref, "self query k=20")
    rows = np.arange(pts.shape[0])
    assert (d2[:, 0] == 0).all()
    assert (idx[:, 0] <= rows).all() and (pts[idx[:, 0]] == pts).all(), "entry 0 is the row itself or a lower-indexed duplicate"
    assert (idx[100:110, 0] == np.arange(40, 50)).all()


def test_mean_against_table(device):
    from nerf_vo_amd.pointcloud import NeighbourGrid

    pts, ref = _self_cloud()
    grid = NeighbourGrid(torch.from_numpy(pts).to(device), 1 / 16)
    q = torch.from_numpy(pts).to(device)
    d2, idx = grid.query_knn(q, 20, want="table")
    mean = grid.query_knn(q, 20, want="mean").cpu().numpy()
    from_table = knn_oracle.mean_distance(d2.cpu().numpy(), idx.cpu().numpy())
    assert np.array_equal(mean.view(np.uint32), from_table.view(np.uint32))
    assert np.array_equal(mean.view(np.uint32), knn_oracle.mean_distance(*ref).view(np.uint32))


def test_both_outputs_in_one_call_and_argument_checks(device):
    """The C entry point directly: table and mean of one launch agree with the two separate ones; k = 0, k = 33 and both
    outputs NULL are errors reported through nvo_last_error."""
    from nerf_vo_amd import _lib
    from nerf_vo_amd.pointcloud import NeighbourGrid

    c = CASES["surface_cell_0.1250"]
    grid = NeighbourGrid(torch.from_numpy(c["points"]).to(device), c["cell_size"])
    q = torch.from_numpy(c["queries"]).to(device).contiguous()
    n, k = q.shape[0], 20
    d2 = torch.empty(n, k, dtype=torch.float32, device=device)
    idx = torch.empty(n, k, dtype=torch.int32, device=device)
    mean = torch.empty(n, dtype=torch.float32, device=device)

    def call(k, table=True, with_mean=True):
        args = _lib.KnnArgs(points=grid.points.data_ptr(), point_index=grid.point_index.data_ptr(),
                            cell_start=grid.cell_start.data_ptr(), queries=q.data_ptr(),
                            out_dist2=d2.data_ptr() if table else None, out_index=idx.data_ptr() if table else None,
                            out_mean_dist=mean.data_ptr() if with_mean else None, N=n, M=grid.n_points, k=k, gx=grid.dims[0],
                            gy=grid.dims[1], gz=grid.dims[2], lower_x=grid.lower[0], lower_y=grid.lower[1], lower_z=grid.lower[2],
                            cell_size=grid.cell_size)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        return _lib.lib().nvo_knn_query(stream, C.byref(args))

    assert call(k) == 0, _lib.lib().nvo_last_error()
    torch.cuda.synchronize()
    ref = _brute("surface_cell_0.1250", 20)  # queries in input order here: the order does not change the result
    _assert_table((d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)), ref, "unsorted queries, both outputs")
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), knn_oracle.mean_distance(*ref).view(np.uint32))
    for bad_k in (0, 33):
        assert call(bad_k) != 0
        assert b"between 1 and NVO_KNN_MAX_K" in _lib.lib().nvo_last_error()
    assert call(k, table=False, with_mean=False) != 0
    assert b"both outputs are NULL" in _lib.lib().nvo_last_error()


@pytest.mark.parametrize("std_ratio", [10.0, 2.0])
def test_remove_statistical_outlier(device, std_ratio):
    from nerf_vo_amd.pointcloud import remove_statistical_outlier

    pts, planted = knn_oracle.outlier_scene()
    ref_index, avg, threshold = _outlier_reference(std_ratio)
    gap = np.abs(avg.astype(np.float64) - threshold) / threshold
    print(f"std_ratio {std_ratio}: threshold {threshold:.4f}, largest surface average {avg[~planted].max():.4f}, smallest planted "
          f"average {avg[planted].min():.4f}, smallest relative gap to the threshold {gap.min():.3e}")
    assert gap.min() > 1e-6
    assert np.array_equal(ref_index, np.nonzero(~planted)[0]), "the oracle removes exactly the 12 planted points"
    kept, index = remove_statistical_outlier(torch.from_numpy(pts).to(device), nb_neighbors=20, std_ratio=std_ratio)
    assert index.dtype == torch.int64 and kept.dtype == torch.float32
    assert np.array_equal(index.cpu().numpy(), ref_index)
    assert np.array_equal(kept.cpu().numpy(), pts[ref_index])
    # the result does not depend on the search grid
    _, index2 = remove_statistical_outlier(torch.from_numpy(pts).to(device), nb_neighbors=20, std_ratio=std_ratio, cell_size=0.2)
    assert torch.equal(index, index2)


@functools.lru_cache(maxsize=None)
def _outlier_reference(std_ratio):
    pts, _ = knn_oracle.outlier_scene()
    return knn_oracle.remove_statistical_outlier(pts, 20, std_ratio)


def test_outlier_removal_needs_two_distinct_points(device):
    from nerf_vo_amd.pointcloud import remove_statistical_outlier

    with pytest.raises(ValueError, match="at least 2"):
        remove_statistical_outlier(torch.ones(50, 3, device=device))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        remove_statistical_outlier(torch.rand(50, 3))
