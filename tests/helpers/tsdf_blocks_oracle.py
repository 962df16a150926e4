"""numpy restatements of the rules of the block-sparse TSDF volume (DESIGN.md "Block-sparse TSDF volume";
nerf-vo_amd/csrc/tsdf_blocks.hip, iso_blocks.hip), for tests/test_tsdf_blocks_cpu.py and tests/test_tsdf_blocks_gpu.py.

``touch_rule``      which blocks of the table a frame touches, in FLOAT32, operation for operation as k_tsdf_blocks_touch
                    evaluates it (the library is built with -ffp-contract=off; square root and division are correctly
                    rounded on both sides).  The kernel's sets must equal it bit for bit.
``fuse_touched``    the float64 per-voxel rule of tests/helpers/tsdf_oracle.py (same expressions, same ``ambiguous`` flags)
                    with frame f applied only to the voxels of blocks f touched: the reference's rule.
``block_vertices``  the vertices the block-aware extractor emits -- positions and colours in float32 as written, in its
                    order (block in table order, local index, edge kind) -- from dense arrays.

Nothing here is taken from Open3D (parity with it is unpinned, see nerf-vo_amd/tsdf.py)."""
import numpy as np

BLOCK = 8
KINDS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]  # meshing._EDGE_KINDS

f32 = np.float32


def touch_samples(voxel_size, trunc):
    """samples per pixel: n = 0 .. ceil(2 trunc / h) + 1 with h = voxel_size / 2, from the float32 values"""
    return int(np.ceil(2.0 * float(f32(trunc)) / (0.5 * float(f32(voxel_size))))) + 2


def touch_rule(lower, voxel_size, trunc, depth_max, table_dims, camera_to_world, intrinsics, depth, block_range=None):
    """lower [3], table_dims (tbx, tby, tbz), camera_to_world float32 [K, 4, 4] (or [K, 3, 4]), intrinsics (fx, fy, cx, cy)
    or [K, 4], depth [K, H, W] -> bool [K, tbx, tby, tbz]: the blocks each frame touches.  With ``block_range``
    ((b0, b1), (b0, b1), (b0, b1)), half-open, only that part of the table is returned (a very large table never has to be
    built): the arithmetic is that of the whole table."""
    lower = np.asarray(lower, dtype=f32)
    vs, trunc, depth_max = f32(voxel_size), f32(trunc), f32(depth_max)
    h, quarter, block_size = vs * f32(0.5), vs * f32(0.25), vs * f32(8.0)  # exact
    depth = np.asarray(depth, dtype=f32)
    K, H, W = depth.shape
    c2w = np.asarray(camera_to_world, dtype=f32)
    intr = np.broadcast_to(np.asarray(intrinsics, dtype=f32), (K, 4))
    n_samples = touch_samples(vs, trunc)
    rng = tuple((0, t) for t in table_dims) if block_range is None else tuple(block_range)
    out = np.zeros((K,) + tuple(b - a for a, b in rng), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(K):
            fx, fy, cx, cy = intr[f]
            k_pix = f32(0.5 * np.sqrt(1.0 / float(fx) ** 2 + 1.0 / float(fy) ** 2))  # float64 on the host, rounded once
            m = c2w[f]
            vi, ui = np.nonzero((depth[f] > 0) & (depth[f] <= depth_max))  # a NaN fails both
            d = depth[f][vi, ui]
            a = (ui.astype(f32) - cx) / fx
            b = (vi.astype(f32) - cy) / fy
            slant = np.sqrt((a * a + b * b) + f32(1.0))
            z_lo, z_hi = np.maximum(d - trunc, f32(0.0)), d + trunc
            ranges = []
            for n in range(n_samples):
                z = np.minimum(z_lo + f32(n) * h, z_hi)
                xc, yc = a * z, b * z
                p = [m[r, 0] * xc + m[r, 1] * yc + m[r, 2] * z + m[r, 3] for r in range(3)]
                rho = (z * k_pix + quarter * slant) + quarter
                ok = np.ones(z.shape, dtype=bool)
                cols = []
                for x in range(3):
                    lo = np.floor(((p[x] - rho) - lower[x]) / block_size)
                    hi = np.floor(((p[x] + rho) - lower[x]) / block_size)
                    ok &= (hi >= 0) & (lo < f32(table_dims[x]))  # a NaN fails
                    cols += [np.maximum(lo, f32(0.0)), np.minimum(hi, f32(table_dims[x] - 1))]
                ranges.append(np.stack(cols, axis=1)[ok])
            assert all(r.dtype == f32 for r in ranges)
            for x0, x1, y0, y1, z0, z1 in np.unique(np.concatenate(ranges), axis=0).astype(np.int64):
                cut = [slice(max(a - r[0], 0), max(b + 1 - r[0], 0)) for (a, b), r in zip(((x0, x1), (y0, y1), (z0, z1)), rng)]
                out[(f,) + tuple(cut)] = True
    return out


def fuse_touched(lower, voxel_size, trunc, depth_max, index_range, table, depth, rgb, touched, block_origin=(0, 0, 0)):
    """``tsdf_oracle.fuse`` with frame f applied only where ``touched[f]`` (bool [tbx, tby, tbz]) holds the voxel's block;
    same arguments otherwise, same result dict.  ``ambiguous`` is raised by every frame, applied or not.  ``block_origin``:
    the block ``touched[f][0, 0, 0]`` stands for (``touch_rule``'s ``block_range``)."""
    lower = np.asarray(lower, dtype=np.float32).astype(np.float64)
    vs = float(np.float32(voxel_size))
    trunc = float(np.float32(trunc))
    depth_max = float(np.float32(depth_max))
    table = np.asarray(table, dtype=np.float32).astype(np.float64)
    depth = np.asarray(depth, dtype=np.float32)
    K, H, W = depth.shape
    (i0, i1), (j0, j1), (k0, k1) = index_range
    I, J, Kz = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), np.arange(k0, k1), indexing="ij")
    px, py, pz = lower[0] + I * vs, lower[1] + J * vs, lower[2] + Kz * vs
    shape = px.shape
    tsdf, weight, color = np.zeros(shape), np.zeros(shape), np.zeros((3,) + shape)
    ambiguous = np.zeros(shape, dtype=bool)
    for f in range(K):
        c = table[f]
        xc = c[0] * px + c[1] * py + c[2] * pz + c[3]
        yc = c[4] * px + c[5] * py + c[6] * pz + c[7]
        zc = c[8] * px + c[9] * py + c[10] * pz + c[11]
        ambiguous |= np.abs(zc) < 1e-4
        front = zc > 0
        zs = np.where(front, zc, 1.0)
        u = c[12] * xc / zs + c[14]
        v = c[13] * yc / zs + c[15]
        ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
        near = front & (u > -2) & (u < W + 1) & (v > -2) & (v < H + 1)
        edge = (np.abs(u + 0.5 - np.round(u + 0.5)) < 5e-4) | (np.abs(v + 0.5 - np.round(v + 0.5)) < 5e-4)
        ambiguous |= near & edge
        inside = front & (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
        uc, vc = np.clip(ui, 0, W - 1).astype(np.int64), np.clip(vi, 0, H - 1).astype(np.int64)
        d = depth[f][vc, uc].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = inside & (d > 0) & (d <= depth_max)  # a NaN fails both
        sdf = np.where(ok, d, 0.0) - zc
        ambiguous |= ok & (np.abs(sdf + trunc) < 1e-5)
        ok &= ~(sdf < -trunc)
        ok &= np.asarray(touched[f], dtype=bool)[I // BLOCK - block_origin[0], J // BLOCK - block_origin[1], Kz // BLOCK - block_origin[2]]
        s = np.minimum(sdf, trunc) / trunc
        w1 = weight + 1.0
        tsdf = np.where(ok, (weight * tsdf + s) / w1, tsdf)
        for ch in range(3):
            color[ch] = np.where(ok, (weight * color[ch] + rgb[f][vc, uc, ch].astype(np.float64)) / w1, color[ch])
        weight = np.where(ok, w1, weight)
    return {"tsdf": tsdf, "weight": weight, "color": color, "ambiguous": ambiguous}


def block_vertices(values, valid, color, lower, voxel_size):
    """values float32 [nx, ny, nz] (= -tsdf; dimensions multiples of 8), valid bool, color float32 [3, nx, ny, nz], lower [3]
    -> (positions float32 [V, 3], colors uint8 [V, 3]) of the vertices of the edge-owned rule at threshold 0 with
    step = voxel_size, ordered by (table index of the block of the edge's lower end a, local index of a, edge kind)."""
    values = np.asarray(values, dtype=f32)
    color = np.asarray(color, dtype=f32)
    valid = np.asarray(valid).astype(bool)
    lower, vs = np.asarray(lower, dtype=f32), f32(voxel_size)
    nx, ny, nz = values.shape
    inside = values > f32(0.0)
    # act[i + 1, j + 1, k + 1]: the cube with minimum corner (i, j, k) is active; False around the lattice
    act = np.zeros((nx + 1, ny + 1, nz + 1), dtype=bool)
    cube = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cube &= valid[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    act[1:nx, 1:ny, 1:nz] = cube
    I, J, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    tby, tbz = ny // BLOCK, nz // BLOCK
    block = ((I // BLOCK) * tby + J // BLOCK) * tbz + K // BLOCK
    local = ((I % BLOCK) * BLOCK + J % BLOCK) * BLOCK + K % BLOCK
    keys, pos, col = [], [], []
    with np.errstate(all="ignore"):
        for kind, d in enumerate(KINDS):
            sa = tuple(slice(0, n - d[x]) for x, n in enumerate((nx, ny, nz)))
            sb = tuple(slice(d[x], n) for x, n in enumerate((nx, ny, nz)))
            carry = inside[sa] != inside[sb]
            any_cube = np.zeros_like(carry)
            for ox in ((0,) if d[0] else (0, 1)):
                for oy in ((0,) if d[1] else (0, 1)):
                    for oz in ((0,) if d[2] else (0, 1)):
                        o = (ox, oy, oz)  # the cube with minimum corner a - o
                        any_cube |= act[tuple(slice(1 - o[x], 1 - o[x] + n - d[x]) for x, n in enumerate((nx, ny, nz)))]
            carry &= any_cube
            va, vb = values[sa][carry], values[sb][carry]
            t = (f32(0.0) - va) / (vb - va)
            t = np.fmin(np.fmax(t, f32(0.0)), f32(1.0))  # fmaxf / fminf: a NaN gives 0
            idx = [I[sa][carry], J[sa][carry], K[sa][carry]]
            pos.append(np.stack([lower[x] + (idx[x].astype(f32) + (t if d[x] else f32(0.0))) * vs for x in range(3)], axis=1))
            c = np.stack([(f32(1.0) - t) * color[ch][sa][carry] + t * color[ch][sb][carry] for ch in range(3)], axis=1)
            col.append(np.fmin(np.fmax(np.rint(c), f32(0.0)), f32(255.0)).astype(np.uint8))
            keys.append((block[sa][carry].astype(np.int64) * BLOCK ** 3 + local[sa][carry]) * 7 + kind)
    order = np.argsort(np.concatenate(keys), kind="stable")
    pos, col = np.concatenate(pos)[order], np.concatenate(col)[order]
    assert pos.dtype == f32
    return pos, col
