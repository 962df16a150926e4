"""Restatement of the dense-lattice Poisson reconstruction rule in numpy, operator by operator.
Every operator takes ``dtype``: ``np.float32`` follows the kernels of nerf-vo_amd/csrc/poisson.hip operation by operation,
in their order, and is compared with them bit for bit; ``np.float64`` is the same rule in double precision, the yardstick
of the float32 rule's rounding error.  Both see the same lattice (``h`` and ``origin`` are float32 values).  numpy only;
nothing here shares code with the package, and nothing is taken from the reference or from Open3D.

Lattice: nodes [nx, ny, nz], z fastest; a field of C channels is [C, nx, ny, nz].  Every sum starts from 0, as the
kernels' accumulators do.
"""
import math

import numpy as np


def lattice(lower, upper, depth=9, scale=1.1):
    """h = max(extent) * scale / 2^depth; need = ceil(extent / h) + 4; L = largest l <= depth with min(need) >> l >= 2;
    cells = need rounded up to a multiple of 2^L; origin = centre - cells * h / 2 (float64, then rounded to float32)."""
    lo, hi = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    extent = hi - lo
    h = extent.max() * scale / 2.0 ** depth
    need = [int(math.ceil(e / h)) + 4 for e in extent]
    levels = 0
    while levels + 1 <= depth and (min(need) >> (levels + 1)) >= 2:
        levels += 1
    cells = tuple(-(-n // (1 << levels)) * (1 << levels) for n in need)
    origin = ((lo + hi) / 2 - np.asarray(cells) * h / 2).astype(np.float32)
    return {"h": float(np.float32(h)), "origin": tuple(float(v) for v in origin), "cells": cells,
            "nodes": tuple(c + 1 for c in cells), "levels": levels}


def make_lattice(nodes, h=0.125, origin=(-0.25, 0.5, 0.125)):
    """A lattice given by its node counts (operator tests)."""
    return {"h": float(np.float32(h)), "origin": tuple(float(np.float32(v)) for v in origin),
            "cells": tuple(n - 1 for n in nodes), "nodes": tuple(nodes), "levels": 0}


def locate(points, lat, dtype):
    """(c int64 [K, 3], t dtype [K, 3]): g = (p - origin) / h; c = clamp(floor(g), 0, cells - 1); t = g - c."""
    p = np.asarray(points, np.float32).astype(dtype)
    g = (p - np.asarray(lat["origin"], np.float32).astype(dtype)) / dtype(np.float32(lat["h"]))
    fl = np.minimum(np.maximum(np.floor(g), 0), np.asarray(lat["cells"], dtype) - 1)
    assert g.dtype == dtype
    return fl.astype(np.int64), (g - fl).astype(dtype)


def bin_points(points, lat):
    """(order [K], cell_start [cells + 1]): stable sort by the cell index (cx * cells_y + cy) * cells_z + cz of the FLOAT32
    coordinates (the bins are the same for both precisions)."""
    c, _ = locate(points, lat, np.float32)
    cy, cz = lat["cells"][1], lat["cells"][2]
    cid = (c[:, 0] * cy + c[:, 1]) * cz + c[:, 2]
    order = np.argsort(cid, kind="stable")
    n_cells = lat["cells"][0] * cy * cz
    return order, np.searchsorted(cid[order], np.arange(n_cells + 1), side="left")


def _corner_weights(t, dtype):
    """[8][K]: (ax * ay) * az, a = d ? t : 1 - t, corners in the order dx, dy, dz (dz fastest)."""
    one = dtype(1)
    out = []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                ax = t[:, 0] if dx else one - t[:, 0]
                ay = t[:, 1] if dy else one - t[:, 1]
                az = t[:, 2] if dz else one - t[:, 2]
                out.append(((ax * ay) * az).astype(dtype))
    return out


_CORNERS = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]


def splat(points_sorted, lat, dtype, values=None, denom=None):
    """[C, nx, ny, nz]: per node, acc = acc + w * value over the contributions in the order of the sorted points (which is
    the order cells ascending, points of a cell in sorted order).  value = 1 | values[q] | values[q] / denom[q].  The
    fraction t is taken in the precision ``dtype`` against the point's FLOAT32 bin."""
    nx, ny, nz = lat["nodes"]
    c, _ = locate(points_sorted, lat, np.float32)
    p = np.asarray(points_sorted, np.float32).astype(dtype)
    g = (p - np.asarray(lat["origin"], np.float32).astype(dtype)) / dtype(np.float32(lat["h"]))
    t = (g - c.astype(dtype)).astype(dtype)
    k = p.shape[0]
    if values is None:
        val = None
        channels = 1
    else:
        val = np.asarray(values).astype(dtype).reshape(k, -1)
        if denom is not None:
            val = (val / np.asarray(denom).astype(dtype).reshape(k, 1)).astype(dtype)
        channels = val.shape[1]
    weights = _corner_weights(t, dtype)
    node = np.stack([((c[:, 0] + dx) * ny + (c[:, 1] + dy)) * nz + (c[:, 2] + dz) for dx, dy, dz in _CORNERS], axis=1).reshape(-1)
    w = np.stack(weights, axis=1).reshape(-1)  # point-major: a stable sort by node keeps the points' order per node
    contrib = w[:, None] if val is None else (w[:, None] * np.repeat(val, 8, axis=0)).astype(dtype)
    order = np.argsort(node, kind="stable")
    node_s, contrib_s = node[order], contrib[order]
    first = np.ones(node_s.shape[0], bool)
    first[1:] = node_s[1:] != node_s[:-1]
    rank = np.arange(node_s.shape[0]) - np.maximum.accumulate(np.where(first, np.arange(node_s.shape[0]), 0))
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(rank))]
    out = np.zeros((nx * ny * nz, channels), dtype)
    for r in range(len(bounds) - 1):
        rows = by_rank[bounds[r]:bounds[r + 1]]
        out[node_s[rows]] = out[node_s[rows]] + contrib_s[rows]  # one contribution per node in this round
    assert out.dtype == dtype
    return np.ascontiguousarray(out.T).reshape(channels, nx, ny, nz)


def sample(field, points, lat, dtype):
    """[K, C]: acc = acc + w * field[corner] over the 8 corners in the order dx, dy, dz."""
    nx, ny, nz = lat["nodes"]
    f = np.asarray(field).astype(dtype).reshape(-1, nx * ny * nz)
    c, t = locate(points, lat, dtype)
    weights = _corner_weights(t, dtype)
    acc = np.zeros((c.shape[0], f.shape[0]), dtype)
    for w, (dx, dy, dz) in zip(weights, _CORNERS):
        node = ((c[:, 0] + dx) * ny + (c[:, 1] + dy)) * nz + (c[:, 2] + dz)
        acc = acc + w[:, None] * f[:, node].T
    assert acc.dtype == dtype
    return acc


def divergence(v, dtype):
    """f = 0.5 * (((Vx[i+1] - Vx[i-1]) + (Vy[j+1] - Vy[j-1])) + (Vz[k+1] - Vz[k-1])) inside, 0 on the boundary."""
    v = np.asarray(v).astype(dtype)
    f = np.zeros(v.shape[1:], dtype)
    dx = v[0, 2:, 1:-1, 1:-1] - v[0, :-2, 1:-1, 1:-1]
    dy = v[1, 1:-1, 2:, 1:-1] - v[1, 1:-1, :-2, 1:-1]
    dz = v[2, 1:-1, 1:-1, 2:] - v[2, 1:-1, 1:-1, :-2]
    f[1:-1, 1:-1, 1:-1] = dtype(0.5) * ((dx + dy) + dz)
    return f


def _neighbour_sum(chi):
    return ((((chi[:-2, 1:-1, 1:-1] + chi[2:, 1:-1, 1:-1]) + chi[1:-1, :-2, 1:-1]) + chi[1:-1, 2:, 1:-1])
            + chi[1:-1, 1:-1, :-2]) + chi[1:-1, 1:-1, 2:]


def sweep(chi, f, color):
    """Half-sweep in place on the interior nodes with (i + j + k) & 1 == color: chi = (s - f) * dtype(1/6).  (The nodes of
    one colour have only neighbours of the other: the half-sweep is a simultaneous update.)"""
    dtype = chi.dtype.type
    nx, ny, nz = chi.shape
    i, j, k = np.ogrid[1:nx - 1, 1:ny - 1, 1:nz - 1]
    mask = ((i + j + k) & 1) == color
    new = (_neighbour_sum(chi) - f[1:-1, 1:-1, 1:-1]) * (dtype(1) / dtype(6))
    inner = chi[1:-1, 1:-1, 1:-1]
    inner[mask] = new[mask]


def residual(chi, f):
    """r = f - (s - 6 chi) inside, 0 on the boundary."""
    dtype = chi.dtype.type
    r = np.zeros_like(chi)
    r[1:-1, 1:-1, 1:-1] = f[1:-1, 1:-1, 1:-1] - (_neighbour_sum(chi) - dtype(6) * chi[1:-1, 1:-1, 1:-1])
    return r


def restrict(chi, f):
    """Coarse right-hand side: ((m + 2 c) + p) along z, then y, then x around the even nodes, times 0.0625; boundary 0."""
    dtype = chi.dtype.type
    r = residual(chi, f)
    nx, ny, nz = chi.shape
    two = dtype(2)
    z = (r[:, :, 1:nz - 3:2] + two * r[:, :, 2:nz - 2:2]) + r[:, :, 3:nz - 1:2]
    y = (z[:, 1:ny - 3:2] + two * z[:, 2:ny - 2:2]) + z[:, 3:ny - 1:2]
    x = (y[1:nx - 3:2] + two * y[2:nx - 2:2]) + y[3:nx - 1:2]
    coarse = np.zeros(((nx - 1) // 2 + 1, (ny - 1) // 2 + 1, (nz - 1) // 2 + 1), chi.dtype)
    coarse[1:-1, 1:-1, 1:-1] = x * dtype(0.0625)
    return coarse


def prolong(chi, coarse):
    """chi += (sum of the coarse nodes the fine node lies between, x outermost, z fastest, from 0) * 0.5^(odd indices),
    in place, interior nodes."""
    dtype = chi.dtype.type
    shape_c = coarse.shape
    for ox in (0, 1):
        for oy in (0, 1):
            for oz in (0, 1):
                fine, terms = [], []
                for odd, n, nc in zip((ox, oy, oz), chi.shape, shape_c):
                    if odd:
                        fine.append(slice(1, n - 1, 2))
                        terms.append([slice(0, nc - 1), slice(1, nc)])
                    else:
                        fine.append(slice(2, n - 2, 2))
                        terms.append([slice(1, nc - 1)])
                total = None
                for a in terms[0]:
                    for b in terms[1]:
                        for c in terms[2]:
                            total = (np.zeros_like(coarse[a, b, c]) if total is None else total) + coarse[a, b, c]
                w = dtype(0.5 ** (ox + oy + oz))
                chi[fine[0], fine[1], fine[2]] = chi[fine[0], fine[1], fine[2]] + total * w


def smooth(chi, f, sweeps):
    for _ in range(sweeps):
        sweep(chi, f, 0)
        sweep(chi, f, 1)


def vcycle(chi, f, levels, pre=2, post=2, coarse_sweeps=32):
    """One V(2,2) cycle in place."""
    if levels == 0:
        smooth(chi, f, coarse_sweeps)
        return
    smooth(chi, f, pre)
    fc = restrict(chi, f)
    ec = np.zeros_like(fc)
    vcycle(ec, fc, levels - 1, pre, post, coarse_sweeps)
    prolong(chi, ec)
    smooth(chi, f, post)


def residual_norm(chi, f):
    return float(np.abs(residual(chi, f)).max())


def solve(f, levels, cycles=8):
    """(chi, norm at the start, [norm after every cycle])"""
    chi = np.zeros_like(f)
    start = residual_norm(chi, f)
    norms = []
    for _ in range(cycles):
        vcycle(chi, f, levels)
        norms.append(residual_norm(chi, f))
    return chi, start, norms


def reconstruct_field(points, normals, lat, dtype, cycles=8):
    """The whole chain up to the iso value: dict with order, W, D, V, f, chi, norms, iso (float64 mean of chi at the points)."""
    order, _ = bin_points(points, lat)
    ps = np.asarray(points, np.float32)[order]
    ns = np.asarray(normals, np.float32)[order]
    w = splat(ps, lat, dtype)
    d = sample(w, ps, lat, dtype)[:, 0]
    v = splat(ps, lat, dtype, values=ns, denom=d)
    f = divergence(v, dtype)
    chi, start, norms = solve(f, lat["levels"], cycles)
    iso = float(sample(chi, ps, lat, dtype)[:, 0].astype(np.float64).mean())
    return {"order": order, "points": ps, "W": w, "D": d, "V": v, "f": f, "chi": chi, "start": start, "norms": norms, "iso": iso}


def trim(density, faces, trim_quantile=0.1, min_density=1.0):
    """(keep bool [V], faces re-indexed, threshold): drop density < max(np.quantile(density as float64, q), min_density)."""
    d = np.asarray(density).astype(np.float64)
    threshold = max(float(np.quantile(d, trim_quantile)), float(min_density))
    keep = ~(d < threshold)
    new_index = np.cumsum(keep) - 1
    f = np.asarray(faces).reshape(-1, 3)
    f = f[keep[f].all(axis=1)]
    return keep, new_index[f], threshold


# ---- seeded clouds of the tests -------------------------------------------------------------------------------------
def sphere_cloud(n, centre=(0.52, 0.47, 0.55), radius=0.3, seed=3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(centre) + radius * d).astype(np.float32), d.astype(np.float32)


def room_cloud(n, faces=6, half=0.4, centre=(0.5, 0.5, 0.5), seed=5):
    """``n`` points on the six faces of a cube of side 2 * half BEFORE the face selection, inward normals (the solid is the
    outside of the room); then only the first ``faces`` of the faces (-x, +x, -y, +y, -z, +z) are kept: 5 drops the
    ceiling (+z), 3 keeps -x, +x, -y.  -> (points, normals, face id)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-half, half, size=(n, 3))
    face = rng.integers(0, 6, n)
    axis, side = face // 2, face % 2
    rows = np.arange(n)
    p[rows, axis] = np.where(side == 0, -half, half)
    normal = np.zeros((n, 3))
    normal[rows, axis] = np.where(side == 0, 1.0, -1.0)  # inward
    keep = face < faces
    return (p[keep] + np.asarray(centre)).astype(np.float32), normal[keep].astype(np.float32), face[keep]


def distance_to_room(vertices, faces=6, half=0.4, centre=(0.5, 0.5, 0.5)):
    """Distance of each vertex to the nearest of the kept wall squares."""
    v = np.asarray(vertices, np.float64) - np.asarray(centre)
    best = np.full(v.shape[0], np.inf)
    for face in range(faces):
        axis, side = face // 2, face % 2
        plane = -half if side == 0 else half
        q = np.clip(v, -half, half)
        q[:, axis] = plane
        best = np.minimum(best, np.linalg.norm(v - q, axis=1))
    return best
