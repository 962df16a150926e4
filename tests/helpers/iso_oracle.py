"""The iso-surface rule of DESIGN.md section 11 (include/nerfvo_hip.h section J) restated in numpy: plain loops for the
order, float32 arithmetic for the positions.  What csrc/iso.hip is pinned against, bit for bit.

    inside(p) = values[p] > threshold                                   (a NaN is outside)
    a cube (named by its minimum corner) is active when it exists and its eight corners are valid
    the edge (a, kind) carries a vertex when b = a + KINDS[kind] is in the lattice, inside(a) != inside(b) and an active
        cube has both a and b among its corners
    vertices in ascending ((i*ny + j)*nz + k, kind);  t = clamp((threshold - va) / (vb - va), 0, 1),
        g = float(a_axis) + (d_axis ? t : 0),  out = lower_axis + g * step_axis
    faces: active cubes ascending, tetrahedra 0..5, triangles 0..1 of meshing._TABLE[case], corners 1 and 2 swapped where
        meshing._WINDING says so
"""
import itertools
import warnings

import numpy as np

from nerf_vo_amd import meshing

KINDS = [tuple(k) for k in meshing._EDGE_KINDS.tolist()]
CORNERS = [tuple(c) for c in meshing._CORNERS.tolist()]
TETS = meshing._TETS.tolist()
TABLE = meshing._TABLE.tolist()
WINDING = meshing._WINDING.tolist()


def lattice_step(lower, upper, shape):
    """float32 step per axis, as marching_tetrahedra computes it"""
    lo, hi = np.asarray(lower, dtype=np.float32), np.asarray(upper, dtype=np.float32)
    return (hi - lo) / np.asarray([n - 1 for n in shape], dtype=np.float32)


def extract(values, lower, step, threshold, valid=None, index_offset=(0, 0, 0)):
    """values float32 [nx, ny, nz]; lower, step float32 [3] -> (vertices float32 [V, 3], faces int64 [F, 3]).
    ``index_offset``: the lattice is the block of a larger one that starts there (positions use the larger one's indices)."""
    values = np.asarray(values, dtype=np.float32)
    nx, ny, nz = values.shape
    lower, step = np.asarray(lower, dtype=np.float32), np.asarray(step, dtype=np.float32)
    thr = np.float32(threshold)
    inside = values > thr
    ok = np.ones(values.shape, bool) if valid is None else np.asarray(valid).astype(bool)
    active = np.zeros((nx, ny, nz), bool)
    active[:nx - 1, :ny - 1, :nz - 1] = True
    for dx, dy, dz in CORNERS:
        active[:nx - 1, :ny - 1, :nz - 1] &= ok[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]

    def cube_is_active(c):
        return all(0 <= c[x] < values.shape[x] for x in range(3)) and bool(active[c])

    vertex_id, vertices = {}, []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, j, k in itertools.product(range(nx), range(ny), range(nz)):
            a = (i, j, k)
            for kind, d in enumerate(KINDS):
                b = (i + d[0], j + d[1], k + d[2])
                if not (b[0] < nx and b[1] < ny and b[2] < nz) or inside[a] == inside[b]:
                    continue
                # cubes with both ends among their corners: minimum corner = a - o with o = 0 on the edge's axes
                cubes = itertools.product(*[(0,) if d[x] else (0, 1) for x in range(3)])
                if not any(cube_is_active((i - o[0], j - o[1], k - o[2])) for o in cubes):
                    continue
                va, vb = values[a], values[b]
                t = np.float32(thr - va) / np.float32(vb - va)
                t = np.fmin(np.fmax(np.float32(t), np.float32(0)), np.float32(1))  # fmaxf / fminf: a NaN gives 0
                pos = []
                for x in range(3):
                    g = np.float32(a[x] + index_offset[x]) + (t if d[x] else np.float32(0))
                    pos.append(lower[x] + np.float32(g * step[x]))
                vertex_id[(a, kind)] = len(vertices)
                vertices.append(pos)
    faces = []
    for i, j, k in itertools.product(range(nx - 1), range(ny - 1), range(nz - 1)):
        if not active[i, j, k]:
            continue
        corner = [(i + c[0], j + c[1], k + c[2]) for c in CORNERS]
        for t, tet in enumerate(TETS):
            case = sum(int(inside[corner[tet[m]]]) << m for m in range(4))
            for r in range(2):
                tri = TABLE[case][r]
                if tri[0][0] < 0:
                    continue
                ids = []
                for ka, kb in tri:
                    pa, pb = corner[tet[ka]], corner[tet[kb]]
                    if pa > pb:  # both ends are ordered on every axis: the tuple order is that order
                        pa, pb = pb, pa
                    ids.append(vertex_id[(pa, KINDS.index((pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2])))])
                if WINDING[t][case][r]:
                    ids = [ids[0], ids[2], ids[1]]
                faces.append(ids)
    return (np.asarray(vertices, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3))


# ---- the fields of the tests: axes are torch.linspace(-1, 1, n) in float32, threshold 0 ----
def axes(shape):
    import torch

    return [torch.linspace(-1.0, 1.0, n, dtype=torch.float32) for n in shape]


def field(name, shape):
    """float32 torch tensor [nx, ny, nz]"""
    import torch

    x, y, z = torch.meshgrid(*axes(shape), indexing="ij")
    if name == "sphere":
        return 0.73 - torch.sqrt((x - 0.03) ** 2 + (y + 0.05) ** 2 + (z - 0.02) ** 2)
    if name == "two":
        a = 0.45 - torch.sqrt((x - 0.4) ** 2 + y ** 2 + z ** 2)
        b = 0.40 - torch.sqrt((x + 0.45) ** 2 + (y - 0.1) ** 2 + z ** 2)
        return torch.maximum(a, b)
    if name == "open":
        return 0.31 - (z + 0.3 * x * y)
    raise KeyError(name)


def valid_mask(spec, shape):
    import torch

    if spec is None:
        return None
    if spec == "rand":
        return torch.rand(shape, generator=torch.Generator().manual_seed(1)) > 0.03
    if spec == "holes":
        v = torch.ones(shape, dtype=torch.bool)
        v[4, 3, :] = False
        v[0, 0, 0] = False
        return v
    raise KeyError(spec)


# (field, lattice, valid, V, F): the inputs on which marching_tetrahedra's counts equal the combinatorial ones
CASES = [
    ("sphere", (23, 19, 17), None, 2600, 5196),
    ("two", (21, 13, 11), None, 952, 1900),
    ("two", (17, 9, 33), None, 1566, 3128),
    ("open", (9, 8, 7), None, 279, 492),
    ("open", (2, 2, 2), None, 9, 8),
    ("open", (65, 3, 2), None, 645, 1024),
    ("open", (2, 3, 67), None, 207, 246),
    ("open", (5, 66, 4), None, 1299, 2316),
    ("sphere", (23, 19, 17), "rand", 2297, 4106),
    ("open", (9, 8, 7), "holes", 270, 458),
]
CRACK = ("open", (3, 2, 130), None, 387, 462)

_CACHE = {}


def reference(case):
    """(values, valid, vertices, faces) of a case, computed once and shared (read-only)"""
    name, shape, spec = case[:3]
    key = (name, shape, spec)
    if key not in _CACHE:
        values, valid = field(name, shape), valid_mask(spec, shape)
        lower, upper = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        v, f = extract(values.numpy(), np.asarray(lower, np.float32), lattice_step(lower, upper, shape), 0.0,
                       None if valid is None else valid.numpy())
        v.setflags(write=False)
        f.setflags(write=False)
        _CACHE[key] = (values, valid, v, f)
    return _CACHE[key]
