"""float64 restatement of the TSDF integration rule of nerf-vo_amd/csrc/tsdf.hip (DESIGN.md "TSDF fusion"), in numpy, for
tests/test_tsdf_gpu.py.  It evaluates an index range of the volume, so a sub-box of a very large volume can be checked
without building the whole of it, and it flags the voxels whose outcome hangs on a rounding decision.

Inputs are the float32 / uint8 values the kernel receives, promoted to float64; nothing here is taken from Open3D (parity
with it is unpinned, see nerf-vo_amd/tsdf.py)."""
import numpy as np


def fuse(lower, voxel_size, trunc, depth_max, index_range, table, depth, rgb):
    """lower [3], index_range ((i0, i1), (j0, j1), (k0, k1)) half-open, table [K, 16] (world->camera 3x4 row-major, fx fy cx
    cy), depth [K, H, W], rgb [K, H, W, 3] uint8.  Frames are applied in order.  Returns a dict of float64 arrays over the
    range: tsdf, weight, color [3, ...], and bool ``ambiguous``: in some frame u + 0.5 or v + 0.5 lies within 5e-4 of an
    integer (near the image), or sdf within 1e-5 of -trunc, or |zc| < 1e-4."""
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
        s = np.minimum(sdf, trunc) / trunc
        w1 = weight + 1.0
        tsdf = np.where(ok, (weight * tsdf + s) / w1, tsdf)
        for ch in range(3):
            color[ch] = np.where(ok, (weight * color[ch] + rgb[f][vc, uc, ch].astype(np.float64)) / w1, color[ch])
        weight = np.where(ok, w1, weight)
    return {"tsdf": tsdf, "weight": weight, "color": color, "ambiguous": ambiguous}


def room_scene(n_cameras=8, height=72, width=96, half_extent=0.5, translation_scale=0.25):
    """The analytic room [-half_extent, half_extent]^3 seen from an orbit: (depth float32 [n, H, W], rgb uint8 [n, H, W, 3],
    world_to_camera float32 [n, 4, 4], camera_to_world float64 [n, 4, 4], intrinsics (fx, fy, cx, cy)), torch CPU tensors."""
    import torch

    from nerf_vo_amd.synthetic import orbit_poses_opencv, render_room, replica_intrinsics

    intr = replica_intrinsics(height, width)
    c2w = orbit_poses_opencv(n_cameras)
    c2w[:, :3, 3] *= translation_scale
    color, depth, _ = render_room(c2w, height, width, intr, half_extent=half_extent)
    rgb = (color.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()
    w2c = torch.linalg.inv(c2w.double()).float()
    return depth[:, 0].contiguous(), rgb, w2c, c2w.double(), intr


def frame_table(world_to_camera, intrinsics):
    """[K, 16] float32 numpy table of the kernel from world_to_camera [K, 4, 4] and (fx, fy, cx, cy)."""
    w2c = np.asarray(world_to_camera, dtype=np.float32)
    intr = np.tile(np.asarray(intrinsics, dtype=np.float32), (w2c.shape[0], 1))
    return np.concatenate([w2c[:, :3, :4].reshape(-1, 12), intr], axis=1)
