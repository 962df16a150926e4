"""Seeded inputs and the measurements shared by tests/test_poisson_cpu.py, tests/test_poisson_gpu.py and the writer of
profiles/poisson_parity_margins.json (``python tests/helpers/poisson_cases.py`` rewrites that file from the oracles)."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from helpers import poisson_oracle as O  # noqa: E402

MARGINS_FILE = os.path.join(ROOT, "profiles", "poisson_parity_margins.json")

# (nodes [nx, ny, nz], coarsenings, points).  9^3 has ONE interior coarse node on its coarsest level.  A stencil workgroup is
# 64 lanes along z by 4 rows along y, one x plane per workgroup: 65 x 33 x 33 is several workgroups along x and y but ONE
# along z (nz = 33); 9 x 13 x 137 is the case with more than one along z for every stencil kernel -- the sweep, two nodes
# per lane, needs nz >= 133 for a second workgroup (68 pairs here, the tail ends 4 lanes into it), the prolongation has 135
# lanes (3 workgroups), the restriction 69 coarse nodes (2).  None is a multiple of the tile.
OPERATOR_CASES = [((9, 9, 9), 2, 1), ((9, 9, 9), 2, 2000), ((17, 13, 9), 2, 2000), ((33, 25, 17), 3, 20000), ((65, 33, 33), 4, 20000),
                  ((9, 13, 137), 2, 2000)]
H, ORIGIN = 0.125, (-0.25, 0.5, 0.125)  # dyadic: lattice nodes and planes are exact float32 positions


def case_id(case):
    nodes, _, k = case
    return f"{nodes[0]}x{nodes[1]}x{nodes[2]}-{k}"


def case_lattice(case):
    nodes, levels, _ = case
    lat = O.make_lattice(nodes, H, ORIGIN)
    lat["levels"] = levels
    return lat


@functools.lru_cache(maxsize=None)
def case_cloud(case):
    """(points float32 [K, 3], unit normals float32 [K, 3]) inside the box (two cells of padding on every side): an
    ellipsoid's surface with outward normals -- its inside and the box's corners stay empty -- and, with K >= 2000, 500
    points in one cell, points exactly on nodes, on lattice planes and on the six faces of the box."""
    nodes, _, k = case
    rng = np.random.default_rng(1000 + k + nodes[0])
    cells = np.asarray(nodes) - 1
    lo, hi = np.full(3, 2.0), cells - 2.0  # lattice coordinates of the box
    centre, radii = (lo + hi) / 2 + [0.13, -0.21, 0.08], (hi - lo) / 2 * 0.8

    def ellipsoid(n):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        normal = d / radii
        return centre + radii * d, normal / np.linalg.norm(normal, axis=1, keepdims=True)

    def unit(n):
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    if k == 1:
        g, normal = np.array([[3.3, 4.7, 2.6]]), np.array([[0.6, 0.0, 0.8]])
    else:
        parts = []
        cell = np.floor(centre + [radii[0], 0, 0])  # a cell the surface passes through
        parts.append((cell + rng.uniform(0.01, 0.99, size=(500, 3)), unit(500)))
        on_nodes = np.stack([rng.integers(lo[a], hi[a] + 1, 24) for a in range(3)], axis=1).astype(np.float64)
        parts.append((on_nodes, unit(24)))
        on_planes = rng.uniform(lo, hi, size=(60, 3))
        on_planes[:, 0] = np.round(on_planes[:, 0])
        on_planes[:20, 2] = np.round(on_planes[:20, 2])
        parts.append((np.clip(on_planes, lo, hi), unit(60)))
        on_faces = rng.uniform(lo, hi, size=(60, 3))
        axis, side = rng.integers(0, 3, 60), rng.integers(0, 2, 60)
        on_faces[np.arange(60), axis] = np.where(side == 0, lo[axis], hi[axis])
        parts.append((on_faces, unit(60)))
        parts.insert(0, ellipsoid(k - sum(p.shape[0] for p, _ in parts)))
        g = np.concatenate([p for p, _ in parts])
        normal = np.concatenate([n for _, n in parts])
        perm = rng.permutation(k)
        g, normal = g[perm], normal[perm]
    points = (np.asarray(ORIGIN) + g * H).astype(np.float32)
    assert points.shape == (k, 3)
    return points, normal.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_oracle(case, precision):
    """The whole chain of the oracle for an operator case (computed once per session and shared; treat as read-only)."""
    points, normals = case_cloud(case)
    return O.reconstruct_field(points, normals, case_lattice(case), {"f32": np.float32, "f64": np.float64}[precision])


_KINDS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]  # the extractor's edge kinds


def crossing_difference(chi_a, iso_a, chi_b, iso_b):
    """Largest difference, in voxels along the edge's own axes, between the iso-surface vertices of two fields on the
    lattice edges (the seven edge kinds of the marching-tetrahedra extractor) that BOTH fields cut, and the number of
    edges only one of them cuts."""
    worst, one_sided = 0.0, 0
    nx, ny, nz = chi_a.shape
    for dx, dy, dz in _KINDS:
        lo = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        hi = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        ts, cuts = [], []
        for chi, iso in ((chi_a, iso_a), (chi_b, iso_b)):
            va, vb = chi[lo].astype(np.float64), chi[hi].astype(np.float64)
            cuts.append((va > iso) != (vb > iso))
            with np.errstate(divide="ignore", invalid="ignore"):
                ts.append(np.clip((iso - va) / (vb - va), 0.0, 1.0))
        both = cuts[0] & cuts[1]
        one_sided += int((cuts[0] ^ cuts[1]).sum())
        if both.any():
            worst = max(worst, float(np.abs(ts[0][both] - ts[1][both]).max()))
    return worst, one_sided


def parity_of_case(case):
    """float32 oracle against float64 oracle: relative difference of chi (max |difference| / max |chi|) and the vertex
    difference in voxels."""
    a, b = case_oracle(case, "f32"), case_oracle(case, "f64")
    chi = float(np.abs(a["chi"].astype(np.float64) - b["chi"]).max() / np.abs(b["chi"]).max())
    vertex, one_sided = crossing_difference(a["chi"], np.float32(a["iso"]), b["chi"], b["iso"])
    return {"chi_relative": chi, "vertex_voxels": vertex, "edges_cut_by_one_only": one_sided}


# ---- the prototype's scenes -------------------------------------------------------------------------------------------
SCENES = ("sphere", "room_closed", "room_five_faces")
SPHERE_CENTRE, SPHERE_RADIUS, ROOM_CENTRE, ROOM_HALF = (0.52, 0.47, 0.55), 0.3, (0.5, 0.5, 0.5), 0.4


@functools.lru_cache(maxsize=None)
def scene(name):
    """(points, normals, face id or None, lower, upper, depth): the sphere of 20 000 points at depth 5 in the unit box; the
    rooms of 60 000 points before the face selection at depth 5 over the cloud's own box (the walls lie on the box)."""
    if name == "sphere":
        p, n = O.sphere_cloud(20000, SPHERE_CENTRE, SPHERE_RADIUS)
        return p, n, None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 5
    p, n, face = O.room_cloud(60000, 6 if name == "room_closed" else 5, ROOM_HALF, ROOM_CENTRE)
    return p, n, face, tuple(p.min(axis=0).astype(np.float64)), tuple(p.max(axis=0).astype(np.float64)), 5


def scene_distance(name, vertices, h):
    """Distance of vertices to the scene's true surface, in voxels."""
    v = np.asarray(vertices, np.float64)
    if name == "sphere":
        return np.abs(np.linalg.norm(v - np.asarray(SPHERE_CENTRE), axis=1) - SPHERE_RADIUS) / h
    return O.distance_to_room(v, 6 if name == "room_closed" else 5, ROOM_HALF, ROOM_CENTRE) / h


@functools.lru_cache(maxsize=None)
def scene_oracle_mesh(name):
    """The float32 oracle's field through the package's torch marching_tetrahedra (tetrahedron diagonals included) and the
    oracle's trim -> dict(lattice, vertices, faces, density, keep, keep_without_floor, worst_kept, worst_without_floor)."""
    import torch

    from nerf_vo_amd.meshing import marching_tetrahedra

    p, n, _, lower, upper, depth = scene(name)
    lat = O.lattice(lower, upper, depth)
    res = O.reconstruct_field(p, n, lat, np.float32)
    top = np.asarray(lat["origin"], np.float64) + lat["h"] * np.asarray(lat["cells"], np.float64)
    v, f = marching_tetrahedra(torch.from_numpy(res["chi"]), lat["origin"], top, float(np.float32(res["iso"])))
    v, f = v.numpy(), f.numpy()
    density = O.sample(res["W"], v, lat, np.float32)[:, 0]
    keep, _, threshold = O.trim(density, f)
    keep0, _, _ = O.trim(density, f, min_density=0.0)
    dist = scene_distance(name, v, lat["h"])
    return {"lattice": lat, "vertices": v, "faces": f, "density": density, "keep": keep, "keep_without_floor": keep0,
            "threshold": threshold, "worst_kept": float(dist[keep].max()), "worst_without_floor": float(dist[keep0].max()),
            "zero_density_share": float((density == 0).mean()), "kept_share": float(keep.mean())}


# ---- convergence on the prototype's lattices ------------------------------------------------------------------------
CONVERGENCE_CASES = {"49x49x49": ((1.0, 1.0, 1.0), 5, 20000), "41x33x33": ((1.0, 0.8, 0.8), 5, 20000), "25x25x25": ((1.0, 1.0, 1.0), 4, 4000)}


@functools.lru_cache(maxsize=None)
def convergence(name):
    """float64 oracle: (nodes, worst residual max-norm factor of one cycle over 8 cycles, residual after 8 cycles over the
    start) for a sphere's cloud in the box."""
    upper, depth, k = CONVERGENCE_CASES[name]
    radius = 0.3 * min(upper)
    p, n = O.sphere_cloud(k, tuple(0.5 * u + 0.02 for u in upper), radius)
    lat = O.lattice((0.0, 0.0, 0.0), upper, depth)
    res = O.reconstruct_field(p, n, lat, np.float64)
    norms = [res["start"]] + res["norms"]
    return lat["nodes"], max(b / a for a, b in zip(norms[:-1], norms[1:])), norms[-1] / norms[0]


def measure_all():
    out = {"_comment": "float32 oracle against float64 oracle (tests/helpers/poisson_oracle.py); written by "
                       "`python tests/helpers/poisson_cases.py`; tests assert 2.5 x the parity values, 1.5 x the convergence "
                       "factors, and the GPU meshes against geometry_bound_voxels = 2 x the oracle's worst kept vertex",
           "parity": {case_id(c): parity_of_case(c) for c in OPERATOR_CASES}, "convergence": {}, "geometry": {}}
    for name in CONVERGENCE_CASES:
        nodes, factor, total = convergence(name)
        assert "x".join(map(str, nodes)) == name, (nodes, name)
        out["convergence"][name] = {"worst_factor_per_cycle": factor, "residual_after_8_cycles_over_start": total}
    for name in SCENES:
        m = scene_oracle_mesh(name)
        out["geometry"][name] = {"nodes": list(m["lattice"]["nodes"]), "oracle_worst_kept_voxels": m["worst_kept"],
                                 "geometry_bound_voxels": 2.0 * m["worst_kept"],
                                 "oracle_worst_with_min_density_0_voxels": m["worst_without_floor"],
                                 "zero_density_share": m["zero_density_share"], "kept_share": m["kept_share"],
                                 "density_threshold": m["threshold"]}
    return out


def load_margins():
    with open(MARGINS_FILE) as fh:
        return json.load(fh)


if __name__ == "__main__":
    with open(MARGINS_FILE, "w") as fh:
        json.dump(measure_all(), fh, indent=1)
        fh.write("\n")
    print(open(MARGINS_FILE).read())
