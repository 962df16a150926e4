"""Poisson surface reconstruction of an oriented point cloud on a dense lattice: the second half of the nerfstudio
back-end's density mesh (the reference: ``create_from_point_cloud_poisson(depth=9)`` of Open3D, then the vertices below
the 10 % density quantile are dropped; evaluation/nerf_renderer.py:203-207 there).  Open3D is not available where this
project is built and tested, so parity with its octree solver is UNPINNED; what is pinned is this project's own rule,
DESIGN.md section 13, which tests/helpers/poisson_oracle.py restates in numpy and the kernels of csrc/poisson.hip equal
bit for bit.  In short:

  lattice   ``poisson_lattice``: h = max(extent) * scale / 2^depth, two cells of padding per side, cells rounded up to a
            multiple of 2^L so that L coarsenings leave 2..3 cells on the shortest axis
  splat     trilinear, gathered per node in a fixed order: the density W (value 1), then the vector field V (value
            normal / W(point)), optionally the colours
  solve     (sum of six neighbours - 6 chi) = div V with chi = 0 on the boundary, from chi = 0, by V(2,2) multigrid cycles
            (red-black Gauss-Seidel, full weighting, trilinear prolongation)
  surface   the iso-surface of chi at the float64 mean of chi over the points (meshing.extract_isosurface), faces turned
            so that their normals agree with the points' normals
  trim      vertices whose density W is below max(quantile(density, trim_quantile), min_density) are dropped

Not reproduced from Open3D's solver: the screening term (point weight), Neumann boundaries, the
adaptive octree, B-splines above degree 1, a density estimate at a coarser depth.  ``min_density`` is this project's
addition: on a dense lattice unobserved space has density exactly 0 at full resolution and open surfaces grow sheets
there that a quantile does not reach; ``min_density=0`` gives the reference's rule alone.

The kernels have no CPU fallback; ``poisson_lattice`` and ``trim_by_density`` are plain Python / torch and work anywhere.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MIN_DEPTH, MAX_DEPTH = 2, 10


def poisson_lattice(lower, upper, depth: int = 9, scale: float = 1.1) -> dict:
    """The lattice of a reconstruction over the box ``lower..upper`` (float64 arithmetic; ``h`` and ``origin`` are then
    rounded to float32, the values the kernels see).  ``h = max(extent) * scale / 2^depth``; per axis
    ``need = ceil(extent / h) + 4``; ``levels`` = the largest L <= depth with ``min(need) >> L >= 2``;
    ``cells = need`` rounded up to a multiple of 2^L; ``nodes = cells + 1``; ``origin = centre - cells * h / 2``.
    Returns ``h``, ``origin``, ``upper`` (= origin + cells * h), ``cells``, ``nodes``, ``levels``, ``depth``, ``scale``."""
    lo = np.asarray(lower, dtype=np.float64).reshape(3)
    hi = np.asarray(upper, dtype=np.float64).reshape(3)
    if int(depth) != depth or not MIN_DEPTH <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"poisson_lattice: depth = {depth} must be an integer between {MIN_DEPTH} and {MAX_DEPTH} (the "
                         "reference uses 9): pass a depth in that range")
    depth = int(depth)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"poisson_lattice: the box {lo.tolist()} .. {hi.tolist()} is not finite: pass finite bounds")
    extent = hi - lo
    if (extent < 0).any() or not extent.max() > 0:
        raise ValueError(f"poisson_lattice: the box {lo.tolist()} .. {hi.tolist()} needs upper >= lower on every axis and a "
                         "positive extent on at least one: pass the bounds in that order")
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"poisson_lattice: scale = {scale} must be positive and finite (Open3D's default is 1.1)")
    h = float(extent.max()) * float(scale) / 2 ** depth
    need = [int(math.ceil(float(e) / h)) + 4 for e in extent]
    levels = max(l for l in range(depth + 1) if (min(need) >> l) >= 2)
    step = 1 << levels
    cells = tuple(((n + step - 1) // step) * step for n in need)
    nodes = tuple(c + 1 for c in cells)
    if nodes[0] * nodes[1] * nodes[2] >= 2 ** 31 or max(nodes) > _lib.POISSON_MAX_NODES_PER_AXIS:
        raise ValueError(f"poisson_lattice: depth {depth} over a box of extent {extent.tolist()} is a lattice of {nodes[0]} x "
                         f"{nodes[1]} x {nodes[2]} nodes; it must stay below 2^31 nodes and {_lib.POISSON_MAX_NODES_PER_AXIS} per "
                         "axis: lower the depth")
    centre = 0.5 * (lo + hi)
    origin = (centre - 0.5 * h * np.asarray(cells, dtype=np.float64)).astype(np.float32)
    h32 = float(np.float32(h))
    top = origin.astype(np.float64) + h32 * np.asarray(cells, dtype=np.float64)
    return {"h": h32, "origin": tuple(float(v) for v in origin), "upper": tuple(float(v) for v in top), "cells": cells,
            "nodes": nodes, "levels": int(levels), "depth": depth, "scale": float(scale)}


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what}: the data must be on the GPU -- no CPU fallback (tests/helpers/poisson_oracle.py is the "
                           "numpy restatement)")


def _f3(values):
    return (C.c_float * 3)(*[float(v) for v in values])


def bin_points(points: torch.Tensor, lattice: dict):
    """``(order int64 [K], cell_start int32 [cells + 1])``: the points sorted (stable) by the linear index
    ``(cx * cells_y + cy) * cells_z + cz`` of their lattice cell, ``c = clamp(floor((p - origin) / h), 0, cells - 1)`` in
    float32 (the division is a true division: by a tensor, not by a Python number), and the first sorted row of every
    cell (a count per cell and its running sum, as ``NeighbourGrid``).  Any device."""
    dev = points.device
    cells = lattice["cells"]
    origin = torch.tensor(lattice["origin"], dtype=torch.float32, device=dev)
    h = torch.tensor(lattice["h"], dtype=torch.float32, device=dev)
    top = torch.tensor([c - 1 for c in cells], dtype=torch.float32, device=dev)
    cell = torch.minimum(torch.floor((points - origin) / h).clamp_(min=0.0), top).long()
    cid = (cell[:, 0] * cells[1] + cell[:, 1]) * cells[2] + cell[:, 2]
    cid, order = torch.sort(cid, stable=True)
    n_cells = cells[0] * cells[1] * cells[2]
    # (uint32 in the C-ABI: the values are below 2^31, int32 tensors hold the same bits)
    cell_start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    torch.cumsum(torch.bincount(cid, minlength=n_cells), dim=0, dtype=torch.int32, out=cell_start[1:])
    return order, cell_start


@torch.no_grad()
def splat(points_sorted: torch.Tensor, cell_start: torch.Tensor, lattice: dict, values=None, denom=None) -> torch.Tensor:
    """``nvo_poisson_splat``: float32 [C, nx, ny, nz].  ``values`` None: the density W (C = 1); [K, 1] or [K, 3] float32
    in the sorted order otherwise, divided by ``denom`` [K] when given."""
    _need_gpu(points_sorted, "poisson.splat")
    dev = points_sorted.device
    nx, ny, nz = lattice["nodes"]
    channels = 1 if values is None else int(values.shape[1])
    pts = points_sorted.to(torch.float32).contiguous()
    vals = None if values is None else values.to(device=dev, dtype=torch.float32).contiguous()
    den = None if denom is None else denom.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    out = torch.empty(channels, nx, ny, nz, dtype=torch.float32, device=dev)
    args = _lib.PoissonSplatArgs(points=pts.data_ptr(), cell_start=cell_start.data_ptr(),
                                 values=None if vals is None else vals.data_ptr(), denom=None if den is None else den.data_ptr(),
                                 out=out.data_ptr(), K=int(pts.shape[0]), channels=channels, nx=nx, ny=ny, nz=nz,
                                 origin=_f3(lattice["origin"]), h=lattice["h"])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nvo_poisson_splat(_stream(dev), C.byref(args)), "poisson_splat")
    return out


@torch.no_grad()
def sample(field: torch.Tensor, points: torch.Tensor, lattice: dict) -> torch.Tensor:
    """``nvo_poisson_sample``: the planar field [C, nx, ny, nz] (C = 1 or 3; [nx, ny, nz] counts as C = 1) interpolated at
    ``points`` [K, 3] -> float32 [K, C]."""
    _need_gpu(field, "poisson.sample")
    dev = field.device
    nx, ny, nz = lattice["nodes"]
    field = field.to(torch.float32).contiguous().reshape(-1, nx, ny, nz)
    pts = points.to(device=dev, dtype=torch.float32).contiguous()
    channels = int(field.shape[0])
    out = torch.empty(int(pts.shape[0]), channels, dtype=torch.float32, device=dev)
    args = _lib.PoissonSampleArgs(field=field.data_ptr(), points=pts.data_ptr(), out=out.data_ptr(), K=int(pts.shape[0]),
                                  channels=channels, nx=nx, ny=ny, nz=nz, origin=_f3(lattice["origin"]), h=lattice["h"])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nvo_poisson_sample(_stream(dev), C.byref(args)), "poisson_sample")
    return out


def _level_call(name: str, like: torch.Tensor, **fields) -> None:
    nx, ny, nz = like.shape[-3:]
    args = _lib.PoissonLevelArgs(nx=nx, ny=ny, nz=nz, **fields)
    dev = like.device
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), "nvo_poisson_" + name)(_stream(dev), C.byref(args)), "poisson_" + name)


def _lattice_field(t: torch.Tensor, what: str, dims: int = 3) -> torch.Tensor:
    _need_gpu(t, what)
    if t.dim() != dims or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous float32 tensor with {dims} dimensions expected, got {t.dtype} {tuple(t.shape)}")
    return t


@torch.no_grad()
def divergence(field: torch.Tensor) -> torch.Tensor:
    """``nvo_poisson_divergence``: V [3, nx, ny, nz] -> the right-hand side f [nx, ny, nz] (central differences, the factor
    0.5, no h; 0 on the boundary nodes)."""
    field = _lattice_field(field, "poisson.divergence", 4)
    rhs = torch.empty(field.shape[1:], dtype=torch.float32, device=field.device)
    _level_call("divergence", rhs, field=field.data_ptr(), rhs=rhs.data_ptr())
    return rhs


@torch.no_grad()
def sweep(chi: torch.Tensor, rhs: torch.Tensor, color: int) -> None:
    """``nvo_poisson_sweep``: one red-black Gauss-Seidel half-sweep on ``chi`` in place (``color`` 0: red, (i+j+k) even)."""
    _lattice_field(chi, "poisson.sweep"), _lattice_field(rhs, "poisson.sweep")
    _level_call("sweep", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), color=int(color))


@torch.no_grad()
def restrict(chi: torch.Tensor, rhs: torch.Tensor) -> torch.Tensor:
    """``nvo_poisson_restrict``: the coarse right-hand side, 4 * full weighting of the residual."""
    _lattice_field(chi, "poisson.restrict"), _lattice_field(rhs, "poisson.restrict")
    coarse = torch.empty([(n - 1) // 2 + 1 for n in chi.shape], dtype=torch.float32, device=chi.device)
    _level_call("restrict", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), coarse=coarse.data_ptr())
    return coarse


@torch.no_grad()
def prolong(chi: torch.Tensor, coarse: torch.Tensor) -> None:
    """``nvo_poisson_prolong``: ``chi`` += trilinear interpolation of ``coarse``, in place, interior nodes only."""
    _lattice_field(chi, "poisson.prolong"), _lattice_field(coarse, "poisson.prolong")
    if list(coarse.shape) != [(n - 1) // 2 + 1 for n in chi.shape]:
        raise ValueError(f"poisson.prolong: coarse {tuple(coarse.shape)} is not the coarsening of {tuple(chi.shape)}")
    _level_call("prolong", chi, chi=chi.data_ptr(), coarse=coarse.data_ptr())


@torch.no_grad()
def solve(rhs: torch.Tensor, levels: int, cycles: int = 8):
    """``cycles`` V(2,2) cycles (``nvo_poisson_vcycle``) on (sum of six neighbours - 6 chi) = rhs from chi = 0 ->
    ``(chi [nx, ny, nz], residual_start, [residual max-norm after every cycle])``."""
    rhs = _lattice_field(rhs, "poisson.solve")
    dev = rhs.device
    nx, ny, nz = rhs.shape
    lib = _lib.lib()
    n_bytes = int(lib.nvo_poisson_vcycle_scratch_bytes(nx, ny, nz, int(levels)))
    if n_bytes == 0:
        raise ValueError(f"poisson.solve: a lattice of {nx} x {ny} x {nz} nodes cannot be coarsened {levels} times: every axis "
                         "needs a multiple of 2^levels cells and at least 2 cells on the coarsest level")
    scratch = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    chi = torch.zeros_like(rhs)
    norms = torch.zeros(int(cycles) + 1, dtype=torch.int32, device=dev)
    args = _lib.PoissonVcycleArgs(chi=chi.data_ptr(), rhs=rhs.data_ptr(), scratch=scratch.data_ptr(), nx=nx, ny=ny, nz=nz,
                                  levels=int(levels))
    _level_call("residual_norm", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), norm_bits=norms.data_ptr())
    with torch.cuda.device(dev):
        for c in range(int(cycles)):
            _lib.check(lib.nvo_poisson_vcycle(_stream(dev), C.byref(args)), "poisson_vcycle")
            _level_call("residual_norm", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), norm_bits=norms.data_ptr() + 4 * (c + 1))
    values = norms.view(torch.float32).tolist()
    return chi, values[0], values[1:]


def density_quantile(density: torch.Tensor, q: float) -> float:
    """``np.quantile(density as float64, q)`` by its default (linear) rule, on the tensor's device."""
    if not 0.0 <= float(q) <= 1.0:
        raise ValueError(f"trim_quantile = {q} must be between 0 and 1")
    d = torch.sort(torch.as_tensor(density).reshape(-1).to(torch.float64)).values
    n = int(d.shape[0])
    pos = float(q) * (n - 1)
    lo = min(int(math.floor(pos)), n - 1)
    hi = min(lo + 1, n - 1)
    g = pos - lo
    a, b = float(d[lo]), float(d[hi])
    diff = b - a
    return b - diff * (1.0 - g) if g >= 0.5 else a + diff * g  # numpy's _lerp


def trim_by_density(vertices, faces, density, colors=None, trim_quantile: float = 0.1, min_density: float = 1.0):
    """Drop the vertices with ``density < max(quantile(density, trim_quantile), min_density)``, the faces that lose a
    vertex, and re-index the rest in order -> ``(vertices, faces, colors or None, threshold, keep bool [V])``.  Plain
    torch, any device."""
    v, f = torch.as_tensor(vertices), torch.as_tensor(faces).long()
    d = torch.as_tensor(density).reshape(-1)
    if d.shape[0] != v.shape[0]:
        raise ValueError(f"trim_by_density: {d.shape[0]} densities for {v.shape[0]} vertices")
    if v.shape[0] == 0:
        return v, f.reshape(0, 3), colors, float(min_density), torch.zeros(0, dtype=torch.bool, device=v.device)
    threshold = max(density_quantile(d, trim_quantile), float(min_density))
    keep = ~(d.to(torch.float64) < threshold)
    new_index = torch.cumsum(keep.long(), dim=0) - 1
    f = f[keep[f].all(dim=1)] if f.numel() else f.reshape(0, 3)
    return v[keep], new_index[f], None if colors is None else torch.as_tensor(colors)[keep], threshold, keep


@torch.no_grad()
def poisson_reconstruct(points, normals, colors=None, lower=None, upper=None, depth: int = 9, scale: float = 1.1,
                        cycles: int = 8, trim_quantile: float = 0.1, min_density: float = 1.0):
    """Mesh of the oriented cloud ``points`` / ``normals`` ([K, 3] float32 on the GPU; unit normals pointing OUT of the
    solid; ``colors`` uint8 [K, 3] optional) over the box ``lower..upper`` (default: the cloud's own bounding box) ->
    ``(vertices float32 [V, 3], faces int64 [F, 3], colors uint8 [V, 3] or None, info)`` on the GPU.  The rule is in the
    module's docstring and DESIGN.md section 13.  ``info``: ``lattice``, ``iso``, ``residual_start``, ``residual`` (the
    max-norm after every cycle), ``vertices_before`` / ``faces_before`` / ``vertices`` / ``faces``, ``density_threshold``."""
    pts = torch.as_tensor(points)
    _need_gpu(pts, "poisson_reconstruct")
    dev = pts.device
    nrm = torch.as_tensor(normals).to(dev)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1 or tuple(nrm.shape) != tuple(pts.shape):
        raise ValueError(f"poisson_reconstruct: points and normals [K >= 1, 3] expected, got {tuple(pts.shape)} and {tuple(nrm.shape)}")
    if pts.shape[0] >= 2 ** 31:
        raise ValueError("poisson_reconstruct: at most 2^31 - 1 points: reconstruct from fewer points")
    pts, nrm = pts.to(torch.float32).contiguous(), nrm.to(torch.float32).contiguous()
    if not (bool(torch.isfinite(pts).all()) and bool(torch.isfinite(nrm).all())):
        raise ValueError("poisson_reconstruct: the points or normals hold NaN or infinite values -- remove those points first")
    if colors is not None:
        colors = torch.as_tensor(colors).to(dev)
        if tuple(colors.shape) != tuple(pts.shape) or colors.dtype != torch.uint8:
            raise ValueError(f"poisson_reconstruct: colors must be uint8 [K, 3], got {colors.dtype} {tuple(colors.shape)}")
    if int(cycles) < 1:
        raise ValueError("poisson_reconstruct: cycles must be at least 1")
    if (lower is None) != (upper is None):
        raise ValueError("poisson_reconstruct: pass both lower and upper, or neither (the cloud's own bounding box)")
    if lower is None:
        lower, upper = pts.min(dim=0).values.double().cpu().numpy(), pts.max(dim=0).values.double().cpu().numpy()
    lower, upper = np.asarray(lower, dtype=np.float64).reshape(3), np.asarray(upper, dtype=np.float64).reshape(3)
    lattice = poisson_lattice(lower, upper, depth, scale)
    # the box as float32, the precision of the points
    lo32, hi32 = torch.tensor(lower, device=dev).float(), torch.tensor(upper, device=dev).float()
    outside = int(((pts < lo32) | (pts > hi32)).any(dim=1).sum())
    if outside:
        raise ValueError(f"poisson_reconstruct: {outside} of {pts.shape[0]} points lie outside the box {lower.tolist()} .. "
                         f"{upper.tolist()} -- crop the cloud to the box, or pass a box that holds it")

    order, cell_start = bin_points(pts, lattice)
    pts_s, nrm_s = pts[order].contiguous(), nrm[order].contiguous()
    W = splat(pts_s, cell_start, lattice)
    D = sample(W, pts_s, lattice)  # >= the point's own sum of w^2 >= 1/8
    V = splat(pts_s, cell_start, lattice, values=nrm_s, denom=D)
    rhs = divergence(V)
    del V
    chi, r0, residual = solve(rhs, lattice["levels"], cycles)
    del rhs
    iso = float(sample(chi, pts_s, lattice).to(torch.float64).mean())
    from .meshing import extract_isosurface

    vertices, faces = extract_isosurface(chi, lattice["origin"], lattice["upper"], iso)
    del chi
    # extract_isosurface winds its faces so that their normals point from values above the threshold to values below;
    # chi rises along the points' normals (grad chi ~ V), so the agreeing normal points towards HIGHER chi: every face
    # is turned, whatever the mesh
    faces = faces[:, [0, 2, 1]].contiguous()
    info = {"lattice": lattice, "iso": iso, "residual_start": r0, "residual": residual,
            "vertices_before": int(vertices.shape[0]), "faces_before": int(faces.shape[0])}
    if vertices.shape[0] == 0:
        raise RuntimeError(f"poisson_reconstruct: the field has no iso-surface at {iso:g} inside the lattice ({pts.shape[0]} points, "
                           f"depth {lattice['depth']}): are the normals unit vectors that point out of the surface?")
    density = sample(W, vertices, lattice)[:, 0]
    vertex_colors = None
    if colors is not None:
        csum = splat(pts_s, cell_start, lattice, values=colors[order].to(torch.float32))
        seen = W > 0
        node_color = torch.where(seen, csum / W, torch.zeros_like(csum))  # W [1, ...] broadcasts over the channels
        del csum
        # nodes nobody splatted to have no colour: the interpolation is normalised by the weight of those that have one
        # (a kept vertex has density > 0, hence at least one such corner)
        share = sample(seen.to(torch.float32), vertices, lattice)
        vertex_colors = torch.round(sample(node_color, vertices, lattice) / share.clamp_min(1e-30)).clamp_(0.0, 255.0).to(torch.uint8)
        del node_color, seen
    vertices, faces, vertex_colors, threshold, _ = trim_by_density(vertices, faces, density, vertex_colors, trim_quantile, min_density)
    info.update(vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), density_threshold=float(threshold))
    return vertices, faces, vertex_colors, info
