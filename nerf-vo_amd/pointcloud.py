"""Point-cloud operations behind the 3-D mesh metrics (``evaluation.calculate_metrics_3d``): uniform surface sampling,
voxel down-sampling, exact nearest-neighbour search and point-to-point ICP -- what the reference gets from Open3D
(``sample_points_uniformly``, ``voxel_down_sample``, ``registration.icp``) and scipy (``cKDTree.query``) on the CPU
(evaluation/evaluation_utils.py:447-512 there), without either library.

The hot operation is the nearest-neighbour search between two clouds of up to 200 000 points, once per ICP iteration and
twice more for the metrics: one HIP kernel (csrc/nn.hip: ``nvo_nn_query``, the rule and the termination argument are
stated there and in DESIGN.md "Nearest-neighbour search") over a uniform cell grid that ``NeighbourGrid`` builds with torch
ops.  There is no CPU fallback for the search; everything else is plain torch and works on any device.

What is pinned against what: the search equals a brute-force float32 evaluation bit for bit
(tests/helpers/nn_oracle.py) and agrees with the reference's own kd-tree distances on stored clouds
(tests/golden/metrics3d_golden.npz).  Parity of the sampling, the down-sampling and the ICP with Open3D is UNPINNED: the
library is not available where this project is built and tested.  They follow Open3D's documented behaviour (triangle
drawn by area and square-root barycentrics; mean of the points per voxel of the lattice floor(p / voxel_size);
point-to-point ICP with Kabsch updates and the relative fitness / RMSE criteria) and are tested against this project's
own float64 restatements.

The point cloud of the nerfstudio back-end (mapping/renderer.py: ``render_point_cloud``) adds the k-nearest-neighbour search
on the same grid (csrc/knn.hip: ``nvo_knn_query`` behind ``NeighbourGrid.query_knn``, bit for bit the brute force of
tests/helpers/knn_oracle.py) and ``remove_statistical_outlier`` on it, which follows Open3D's
documented rule; its parity with Open3D is UNPINNED for the same reason.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

# cell size of the search grid in metres: the fastest setting of tools/metrics3d_bench.py at 200 000 x 200 000
# surface-like points (table in EXPERIMENTS.md section 14)
DEFAULT_CELL_SIZE = 3.0 / 64.0
MAX_CELLS = 2 ** 27  # cell_start is 4 bytes per cell: 512 MiB


def _as_points(x, name: str) -> torch.Tensor:
    x = torch.as_tensor(x)
    if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError(f"{name}: points [N, 3] with N >= 1 expected, got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{name}: the points hold NaN or infinite coordinates -- remove them first")
    return x


class NeighbourGrid:
    """Target points binned into a uniform grid of cubic cells over their bounding box, for exact nearest-neighbour
    queries.  Cell of a point: ``floor((p - lower) / cell_size)`` per axis in float32, clamped to the grid; linear id
    ``(iz * gy + iy) * gx + ix``.  ``points`` [M, 3] (kept sorted by cell id, stable), ``point_index`` [M] the index of each
    sorted point in the input, ``cell_start`` [gx*gy*gz + 1] the first sorted row of each cell."""

    def __init__(self, points, cell_size: float = DEFAULT_CELL_SIZE, max_cells: int = MAX_CELLS) -> None:
        pts = _as_points(points, "NeighbourGrid")
        if pts.shape[0] >= 2 ** 31:
            raise ValueError("NeighbourGrid: at most 2^31 - 1 points")
        if not (cell_size > 0 and math.isfinite(cell_size)):
            raise ValueError("NeighbourGrid: cell_size must be positive and finite")
        self.cell_size = float(np.float32(cell_size))
        lo = pts.min(dim=0).values
        hi = pts.max(dim=0).values
        self.lower = tuple(float(v) for v in lo.tolist())
        extent = [float(h) - float(l) for l, h in zip(lo.tolist(), hi.tolist())]
        dims = tuple(int(math.floor(e / self.cell_size)) + 1 for e in extent)
        n_cells = dims[0] * dims[1] * dims[2]
        cap = _lib.NN_MAX_CELLS_PER_AXIS
        if max(dims) > cap or n_cells > min(int(max_cells), 2 ** 31 - 1):
            need = max(max(extent) / (cap - 1), (extent[0] * extent[1] * extent[2] / min(int(max_cells), 2 ** 31 - 1)) ** (1 / 3))
            raise ValueError(
                f"NeighbourGrid: the points span {extent[0]:g} x {extent[1]:g} x {extent[2]:g}, which at cell_size "
                f"{self.cell_size:g} is a grid of {dims[0]} x {dims[1]} x {dims[2]} = {n_cells} cells; the search allows "
                f"{cap} cells per axis (its termination margin is argued for that many) and max_cells = {int(max_cells)} cells "
                f"in all: pass a cell_size of at least {need * 1.01:g}, or remove outlying points")
        self.dims = dims
        lower = torch.tensor(self.lower, dtype=torch.float32, device=pts.device)
        top = torch.tensor([d - 1 for d in dims], dtype=torch.float32, device=pts.device)
        cell = torch.minimum(torch.floor((pts - lower) / self.cell_size).clamp_(min=0.0), top).long()
        cid = (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]
        cid, order = torch.sort(cid, stable=True)
        counts = torch.bincount(cid, minlength=n_cells)
        start = torch.zeros(n_cells + 1, dtype=torch.int64, device=pts.device)
        start[1:] = torch.cumsum(counts, dim=0)
        # (uint32 in the C-ABI: the values are below 2^31, int32 tensors hold the same bits)
        self.cell_start = start.to(torch.int32)
        self.point_index = order.to(torch.int32)
        self.points = pts[order].contiguous()
        self.n_points = int(pts.shape[0])
        self.device = pts.device

    def cells_of(self, queries: torch.Tensor) -> torch.Tensor:
        """Linear cell id of each query, clamped into the grid (what the kernel starts its rings from)."""
        lower = torch.tensor(self.lower, dtype=torch.float32, device=queries.device)
        top = torch.tensor([d - 1 for d in self.dims], dtype=torch.float32, device=queries.device)
        cell = torch.minimum(torch.floor((queries - lower) / self.cell_size).clamp_(min=0.0), top).long()
        return (cell[:, 2] * self.dims[1] + cell[:, 1]) * self.dims[0] + cell[:, 0]

    @torch.no_grad()
    def query(self, queries, max_distance=None, transform=None):
        """Nearest target point of each query: ``(dist2 float32 [N], index int64 [N])``, the squared distance
        ``(dx*dx + dy*dy) + dz*dz`` in float32 and the index into the points the grid was built from (the smallest one among
        equally near points).  ``max_distance``: only points with ``dist2 <= float32(max_distance)^2`` count, a query without
        one gets ``inf`` and ``-1``.  ``transform`` ([4, 4] or [3, 4], rigid): applied to each query in float32 as
        ``((r0*x + r1*y) + r2*z) + t`` before the search."""
        q = torch.as_tensor(queries)
        if not (q.is_cuda and self.points.is_cuda):
            raise RuntimeError("NeighbourGrid.query: the grid and the queries must be on the GPU -- no CPU fallback")
        q = _as_points(q, "NeighbourGrid.query").to(self.device)
        if q.shape[0] >= 2 ** 31:
            raise ValueError("NeighbourGrid.query: at most 2^31 - 1 queries")
        if max_distance is not None and not float(max_distance) > 0:
            raise ValueError("NeighbourGrid.query: max_distance must be positive")
        xf = None
        if transform is not None:
            xf = np.asarray(transform.detach().cpu().numpy() if torch.is_tensor(transform) else transform, dtype=np.float64)
            if xf.shape not in ((4, 4), (3, 4)) or not np.isfinite(xf).all():
                raise ValueError("NeighbourGrid.query: transform must be a finite [4, 4] or [3, 4] matrix")
            xf = xf[:3, :4].astype(np.float32)
        # queries sorted by their own cell: the lanes of a wave then walk the same cells (any order gives the same result)
        if xf is None:
            moved = q
        else:
            m = torch.from_numpy(xf).to(self.device)
            moved = q @ m[:, :3].T + m[:, 3]
        perm = torch.argsort(self.cells_of(moved))
        qs = q[perm].contiguous()
        n = int(q.shape[0])
        d2s = torch.empty(n, dtype=torch.float32, device=self.device)
        idxs = torch.empty(n, dtype=torch.int32, device=self.device)
        args = _lib.NnArgs(
            points=self.points.data_ptr(), point_index=self.point_index.data_ptr(), cell_start=self.cell_start.data_ptr(),
            queries=qs.data_ptr(), out_dist2=d2s.data_ptr(), out_index=idxs.data_ptr(), N=n, M=self.n_points,
            gx=self.dims[0], gy=self.dims[1], gz=self.dims[2], lower_x=self.lower[0], lower_y=self.lower[1],
            lower_z=self.lower[2], cell_size=self.cell_size,
            max_dist=math.inf if max_distance is None else float(max_distance), has_xf=0 if xf is None else 1)
        if xf is not None:
            args.xf = (C.c_float * 12)(*xf.reshape(-1).tolist())
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib().nvo_nn_query(stream, C.byref(args)), "nn_query")
        dist2 = torch.empty_like(d2s)
        index = torch.empty(n, dtype=torch.int64, device=self.device)
        dist2[perm] = d2s
        index[perm] = idxs.long()
        return dist2, index

    @torch.no_grad()
    def query_knn(self, queries, k: int, want: str = "table"):
        """The ``k`` nearest target points of each query (csrc/knn.hip: ``nvo_knn_query``; DESIGN.md "k nearest neighbours
        and the point cloud"), ``1 <= k <= 32``.  ``want='table'`` -> ``(dist2 float32 [N, k], index int64 [N, k])``: the
        k smallest pairs (squared distance ``(dx*dx + dy*dy) + dz*dz`` in float32, index into the points the grid was built
        from) in ascending lexicographic order, ties on the distance going to the smaller index; with fewer than ``k``
        target points the remaining slots hold ``inf`` and ``-1``.  A cloud that queries itself finds each point at distance
        0.  ``want='mean'`` -> float32 [N]: the mean of the ``min(k, M)`` distances (not squared), summed in that order in
        float32, without the table ever being written.  With ``k = 1`` the table is ``query``'s result."""
        if want not in ("table", "mean"):
            raise ValueError(f"NeighbourGrid.query_knn: want must be 'table' or 'mean', got {want!r}")
        k = int(k)
        if not 1 <= k <= _lib.KNN_MAX_K:
            raise ValueError(f"NeighbourGrid.query_knn: k = {k} must be between 1 and {_lib.KNN_MAX_K}")
        q = torch.as_tensor(queries)
        if not (q.is_cuda and self.points.is_cuda):
            raise RuntimeError("NeighbourGrid.query_knn: the grid and the queries must be on the GPU -- no CPU fallback")
        q = _as_points(q, "NeighbourGrid.query_knn").to(self.device)
        if q.shape[0] >= 2 ** 31:
            raise ValueError("NeighbourGrid.query_knn: at most 2^31 - 1 queries")
        # queries sorted by their own cell, as in query (any order gives the same result)
        perm = torch.argsort(self.cells_of(q))
        qs = q[perm].contiguous()
        n = int(q.shape[0])
        d2s = idxs = means = None
        if want == "table":
            d2s = torch.empty(n, k, dtype=torch.float32, device=self.device)
            idxs = torch.empty(n, k, dtype=torch.int32, device=self.device)
        else:
            means = torch.empty(n, dtype=torch.float32, device=self.device)
        args = _lib.KnnArgs(
            points=self.points.data_ptr(), point_index=self.point_index.data_ptr(), cell_start=self.cell_start.data_ptr(),
            queries=qs.data_ptr(), out_dist2=None if d2s is None else d2s.data_ptr(),
            out_index=None if idxs is None else idxs.data_ptr(), out_mean_dist=None if means is None else means.data_ptr(),
            N=n, M=self.n_points, k=k, gx=self.dims[0], gy=self.dims[1], gz=self.dims[2], lower_x=self.lower[0],
            lower_y=self.lower[1], lower_z=self.lower[2], cell_size=self.cell_size)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib().nvo_knn_query(stream, C.byref(args)), "knn_query")
        if want == "mean":
            out = torch.empty_like(means)
            out[perm] = means
            return out
        dist2 = torch.empty_like(d2s)
        index = torch.empty(n, k, dtype=torch.int64, device=self.device)
        dist2[perm] = d2s
        index[perm] = idxs.long()
        return dist2, index


# Cell size of the self-query behind remove_statistical_outlier: cells that hold about KNN_POINTS_PER_CELL_FACTOR * k points
# of a SURFACE-like cloud, whose area is taken as that of its bounding box.  0.25 (five points per cell at k = 20) is the
# fastest setting of tools/knn_bench.py at 2 * 10^5 and 2 * 10^6 surface points (table in EXPERIMENTS.md section 17); at
# 3.4 * 10^7 points over a room the caps of the grid decide the cell size, and the smallest allowed one is the fastest.
KNN_POINTS_PER_CELL_FACTOR = 0.25


def knn_cell_size(n_points: int, extent, k: int, factor: float = KNN_POINTS_PER_CELL_FACTOR, max_cells: int = MAX_CELLS) -> float:
    """``sqrt(factor * k * area / n_points)`` with ``area`` the surface of the ``extent`` box (its two largest sides when
    one side is zero, its longest side squared when two are), raised where needed so that the grid keeps to
    ``NN_MAX_CELLS_PER_AXIS`` cells per axis and ``max_cells`` cells."""
    e = [max(float(v), 0.0) for v in extent]
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    if not area > 0:
        area = max(max(e) ** 2, 1e-12)
    cell = math.sqrt(float(factor) * int(k) * area / max(int(n_points), 1))
    floor_axis = max(e) / (_lib.NN_MAX_CELLS_PER_AXIS - 2)
    floor_cells = (max(e[0], cell) * max(e[1], cell) * max(e[2], cell) / (0.5 * min(int(max_cells), 2 ** 31 - 1))) ** (1 / 3)
    return max(cell, floor_axis, floor_cells, 1e-9)


def statistical_outlier_mask(avg: torch.Tensor, std_ratio: float):
    """The rule of ``remove_statistical_outlier`` on the mean neighbour distances ``avg`` [N] -> ``(keep bool [N],
    threshold)``: with ``a = avg`` as float64 and V the points with ``a > 0``, ``mean = sum_V a / |V|``,
    ``std = sqrt(sum_V (a - mean)^2 / (|V| - 1))``, ``threshold = mean + std_ratio * std``; a point is kept when
    ``0 < a < threshold``.  Any device."""
    a = torch.as_tensor(avg).to(torch.float64)
    valid = a > 0
    n_valid = int(valid.sum())
    if n_valid < 2:
        raise ValueError(f"remove_statistical_outlier: {n_valid} of {a.shape[0]} points have a positive mean neighbour "
                         "distance; the standard deviation needs at least 2 (are all points duplicates of one another?)")
    av = a[valid]
    mean = float(av.sum()) / n_valid
    std = math.sqrt(float(((av - mean) ** 2).sum()) / (n_valid - 1))
    threshold = mean + float(std_ratio) * std
    return valid & (a < threshold), threshold


@torch.no_grad()
def remove_statistical_outlier(points, nb_neighbors: int = 20, std_ratio: float = 10.0, cell_size=None):
    """Open3D's ``PointCloud.remove_statistical_outlier`` as documented (parity with Open3D is UNPINNED: the library is
    not available where this project is built and tested) -> ``(kept_points float32 [K, 3], kept_index int64 [K])`` in
    input order, for points on the GPU (no CPU fallback: the search is ``NeighbourGrid.query_knn(want='mean')``).
    ``avg[i]`` = the float32 mean distance of point i to its ``nb_neighbors`` nearest points of the cloud itself, the
    point included at distance 0; the rule on it is ``statistical_outlier_mask``.  ``cell_size``: of the search grid, by
    default ``knn_cell_size`` of the cloud; the result does not depend on it."""
    pts = torch.as_tensor(points)
    if not pts.is_cuda:
        raise RuntimeError("remove_statistical_outlier: the points must be on the GPU -- no CPU fallback")
    pts = _as_points(pts, "remove_statistical_outlier")
    nb = int(nb_neighbors)
    if not 1 <= nb <= _lib.KNN_MAX_K:
        raise ValueError(f"remove_statistical_outlier: nb_neighbors = {nb} must be between 1 and {_lib.KNN_MAX_K}")
    if not float(std_ratio) > 0:
        raise ValueError("remove_statistical_outlier: std_ratio must be positive")
    if cell_size is None:
        extent = (pts.max(dim=0).values - pts.min(dim=0).values).tolist()
        cell_size = knn_cell_size(pts.shape[0], extent, nb)
    avg = NeighbourGrid(pts, cell_size).query_knn(pts, nb, want="mean")
    keep, _ = statistical_outlier_mask(avg, std_ratio)
    index = keep.nonzero().flatten()
    return pts[index], index


def sample_points_uniformly(vertices, faces, number_of_points: int, generator=None) -> torch.Tensor:
    """``number_of_points`` points spread uniformly over the surface of a triangle mesh (float32 [n, 3] on the vertices'
    device): the triangle is drawn with probability proportional to its area, the point inside it has the barycentric
    coordinates ``(1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2)`` of two uniform numbers.  The random numbers are drawn
    in float64 on ``generator``'s device (a CPU generator gives the same points on every device)."""
    v = torch.as_tensor(vertices)
    f = torch.as_tensor(faces).long().to(v.device)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"sample_points_uniformly: vertices [V, 3] and faces [F >= 1, 3] expected, got {tuple(v.shape)}, {tuple(f.shape)}")
    if int(number_of_points) < 1:
        raise ValueError("sample_points_uniformly: number_of_points must be positive")
    v = v.double()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * torch.linalg.norm(torch.cross(b - a, c - a, dim=1), dim=1)
    total = float(area.sum())
    if not (total > 0 and math.isfinite(total)):
        raise ValueError("sample_points_uniformly: the mesh has no surface area (or non-finite vertices)")
    cdf = torch.cumsum(area, dim=0) / total
    rdev = generator.device if generator is not None else torch.device("cpu")
    r = torch.rand(int(number_of_points), 3, dtype=torch.float64, device=rdev, generator=generator).to(v.device)
    tri = torch.searchsorted(cdf, r[:, 0].contiguous(), right=True).clamp_(max=f.shape[0] - 1)
    s = torch.sqrt(r[:, 1])
    w0, w1, w2 = 1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]
    return (w0[:, None] * a[tri] + w1[:, None] * b[tri] + w2[:, None] * c[tri]).float()


def voxel_down_sample(points, voxel_size: float) -> torch.Tensor:
    """One point per occupied voxel of the lattice ``floor(p / voxel_size)`` (float64): the mean of the voxel's points,
    accumulated in float64, as float32 [K, 3].  Output order: ascending voxel index, x most significant, then y, then z."""
    p = torch.as_tensor(points)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError(f"voxel_down_sample: points [N >= 1, 3] expected, got {tuple(p.shape)}")
    if not (voxel_size > 0 and math.isfinite(voxel_size)):
        raise ValueError("voxel_down_sample: voxel_size must be positive and finite")
    pd = p.double()
    if not bool(torch.isfinite(pd).all()):
        raise ValueError("voxel_down_sample: the points hold NaN or infinite coordinates -- remove them first")
    cell = torch.floor(pd / float(voxel_size)).long()
    cell = cell - cell.min(dim=0).values
    ext = (cell.max(dim=0).values + 1).tolist()
    if ext[0] * ext[1] * ext[2] >= 2 ** 62:
        raise ValueError("voxel_down_sample: the points span too many voxels for a 64-bit key -- pass a larger voxel_size")
    key = (cell[:, 0] * ext[1] + cell[:, 1]) * ext[2] + cell[:, 2]
    key, order = torch.sort(key, stable=True)
    # segment sums in input order within a voxel (sequential per segment on every device: no atomics, same bits each run)
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    seg = torch.cumsum(first.long(), dim=0) - 1
    starts = first.nonzero().flatten()
    counts = torch.diff(torch.cat([starts, starts.new_tensor([key.shape[0]])]))
    sorted_p = pd[order]
    # subtracting the segment's first point keeps the running sums small: the cumulative sum then loses nothing that
    # float32 output could show
    rel = sorted_p - sorted_p[starts][seg]
    run = torch.cumsum(rel, dim=0)
    ends = starts + counts - 1
    before = torch.where((starts > 0)[:, None], run[(starts - 1).clamp(min=0)], torch.zeros_like(run[:1]))
    sums = run[ends] - before
    return (sorted_p[starts] + sums / counts[:, None].double()).float()


def kabsch(source: torch.Tensor, target: torch.Tensor) -> np.ndarray:
    """Rigid transform (no scale) that best maps the float64 points ``source`` [K, 3] onto ``target`` [K, 3] in the least
    squares sense, as a float64 [4, 4] numpy matrix.  Sums in float64 on the points' device, the 3x3 SVD on the host."""
    ps, pt = source.double(), target.double()
    cs, ct = ps.mean(dim=0), pt.mean(dim=0)
    h = ((ps - cs).T @ (pt - ct)).cpu().numpy()
    u, _, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    r = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    out = np.eye(4)
    out[:3, :3] = r
    out[:3, 3] = ct.cpu().numpy() - r @ cs.cpu().numpy()
    return out


@torch.no_grad()
def icp_point_to_point(source, target, max_correspondence_distance: float = 0.02, max_iteration: int = 30,
                       relative_fitness: float = 1e-7, relative_rmse: float = 1e-7, cell_size: float = DEFAULT_CELL_SIZE,
                       init=None):
    """Point-to-point ICP of ``source`` [N, 3] onto ``target`` [M, 3] (both on the GPU), the reference's
    ``get_pcd_alignment_transformation`` settings by default -> ``(T float64 [4, 4] numpy, fitness, inlier_rmse,
    iterations)``.  Per iteration: the nearest target point within ``max_correspondence_distance`` of every source point
    under the current transform (one bounded ``NeighbourGrid.query``; the grid of the target is built once), fitness = the
    share of source points that have one, inlier_rmse = the root of their mean squared distance, then the Kabsch update
    (no scale) of the float64-transformed correspondences, composed onto the transform.  Stops when fitness and inlier_rmse
    both changed by less than the criteria from the iteration before, or after ``max_iteration``.  Without any
    correspondence the transform stays as it is and the iteration ends."""
    src = _as_points(source, "icp_point_to_point source")
    grid = target if isinstance(target, NeighbourGrid) else NeighbourGrid(target, cell_size)
    src = src.to(grid.device)
    tgt = torch.empty_like(grid.points)
    tgt[grid.point_index.long()] = grid.points  # the target in its input order
    tgt64, src64 = tgt.double(), src.double()
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    fitness, rmse, prev, iterations = 0.0, 0.0, None, 0
    for it in range(int(max_iteration)):
        iterations = it + 1
        d2, idx = grid.query(src, max_distance=max_correspondence_distance, transform=T)
        hit = idx >= 0
        k = int(hit.sum())
        if k == 0:
            fitness, rmse = 0.0, 0.0
            break
        fitness = k / src.shape[0]
        rmse = math.sqrt(float(d2[hit].double().sum()) / k)
        Tt = torch.from_numpy(T).to(grid.device)
        moved = src64[hit] @ Tt[:3, :3].T + Tt[:3, 3]
        T = kabsch(moved, tgt64[idx[hit]]) @ T
        if prev is not None and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            break
        prev = (fitness, rmse)
    return T, fitness, rmse, iterations
