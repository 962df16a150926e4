"""TSDF fusion of rendered frames into a mesh: the reference's ``integrate_mesh`` (evaluation/evaluation_utils.py:160-227
there, called by ``Renderer.render_mesh(source='frames')``) without Open3D.

The reference fuses with Open3D's ``VoxelBlockGrid`` on the CPU (voxel 1/64, depth truncation 5.0, Open3D's default
truncation band of 8 voxels and its default extraction weight of 3).  Here the volume is a DENSE box on the GPU, the
frames are fused by one HIP kernel (csrc/tsdf.hip: ``nvo_tsdf_integrate``, the rule is stated there and in DESIGN.md
"TSDF fusion") and the surface is extracted by ``meshing.marching_tetrahedra`` with a validity mask.  There is no CPU
fallback for the fusion; allocation, bounds and extraction are plain torch and work on any device.

Parity with Open3D is UNPINNED: the library is not available where this project is built and tested.  The integration
rule and the two defaults (8 voxels, weight 3.0) are taken from Open3D's documentation; what the tests pin the kernel
against is this project's own float64 restatement of the rule (tests/helpers/tsdf_oracle.py).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .meshing import marching_tetrahedra, write_mesh

VOXEL_SIZE = 1.0 / 64.0     # the reference's constants (integrate_mesh)
DEPTH_TRUNCATION = 5.0
TRUNC_VOXELS = 8.0          # Open3D's default trunc_voxel_multiplier
WEIGHT_THRESHOLD = 3.0      # Open3D's default extract_triangle_mesh(weight_threshold=3.0)
# frames per kernel launch: the fastest setting of tools/tsdf_bench.py (table in EXPERIMENTS.md section 13)
FRAMES_PER_LAUNCH = 4


def frustum_bounds(depths, camera_to_world, intrinsics, depth_max: float = DEPTH_TRUNCATION):
    """Axis-aligned box of the back-projected valid pixels (0 < depth <= depth_max; pixel centres on integer coordinates)
    of all frames: depths [N, H, W], camera_to_world [N, 4, 4], intrinsics (fx, fy, cx, cy) -> (lower [3], upper [3]),
    float64 tensors on the depths' device.  The caller pads by the truncation distance and snaps to the voxel lattice."""
    depths = torch.as_tensor(depths)
    dev = depths.device
    d = depths.to(torch.float64)
    c2w = torch.as_tensor(camera_to_world).to(device=dev, dtype=torch.float64)
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    n, h, w = d.shape
    vs, us = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64),
                            torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    lower = torch.full((3,), math.inf, dtype=torch.float64, device=dev)
    upper = torch.full((3,), -math.inf, dtype=torch.float64, device=dev)
    for i in range(n):
        ok = (d[i] > 0) & (d[i] <= depth_max)
        if not bool(ok.any()):
            continue
        z = d[i][ok]
        cam = torch.stack([(us[ok] - cx) / fx * z, (vs[ok] - cy) / fy * z, z], dim=1)
        world = cam @ c2w[i, :3, :3].T + c2w[i, :3, 3]
        lower = torch.minimum(lower, world.min(dim=0).values)
        upper = torch.maximum(upper, world.max(dim=0).values)
    if not bool(torch.isfinite(lower).all()):
        raise ValueError("frustum_bounds: no frame has a pixel with 0 < depth <= depth_max")
    return lower, upper


class TSDFVolume:
    """Dense truncated-signed-distance volume over [lower, upper]: voxel (i, j, k) samples ``lower + (i, j, k) * voxel_size``
    (no half-voxel offset).  ``tsdf`` / ``weight`` float32 [nx, ny, nz], ``color`` float32 [3, nx, ny, nz] (0..255)."""

    def __init__(self, lower, upper, voxel_size: float = VOXEL_SIZE, trunc_voxels: float = TRUNC_VOXELS,
                 depth_max: float = DEPTH_TRUNCATION, device="cuda", max_voxels: int = 2 ** 29) -> None:
        lo = np.asarray(lower.detach().cpu().numpy() if torch.is_tensor(lower) else lower, dtype=np.float64).reshape(3)
        hi = np.asarray(upper.detach().cpu().numpy() if torch.is_tensor(upper) else upper, dtype=np.float64).reshape(3)
        if not (voxel_size > 0 and trunc_voxels > 0 and depth_max > 0):
            raise ValueError("TSDFVolume: voxel_size, trunc_voxels and depth_max must be positive")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
            raise ValueError(f"TSDFVolume: bad box {lo.tolist()} .. {hi.tolist()}")
        self.voxel_size = float(voxel_size)
        self.trunc = float(trunc_voxels) * self.voxel_size
        self.depth_max = float(depth_max)
        # samples lower + i * voxel_size up to the first one at or beyond upper
        self.dims = tuple(int(math.ceil((h - l) / self.voxel_size - 1e-6)) + 1 for l, h in zip(lo, hi))
        n = self.dims[0] * self.dims[1] * self.dims[2]
        if n > max_voxels or n >= 2 ** 31:
            raise ValueError(
                f"TSDFVolume: the box {lo.tolist()} .. {hi.tolist()} needs {self.dims[0]} x {self.dims[1]} x {self.dims[2]} = {n} "
                f"voxels of {self.voxel_size:g} ({20 * n / 2 ** 30:.1f} GiB), more than max_voxels = {min(max_voxels, 2 ** 31 - 1)}: "
                "pass a tighter lower / upper, a larger voxel_size or depth values clipped nearer, or raise max_voxels "
                "(the kernel addresses fewer than 2^31 voxels)")
        self.lower = lo
        self.upper_of_grid = lo + (np.asarray(self.dims) - 1) * self.voxel_size
        self.device = torch.device(device)
        # zeroed explicitly: a recycled allocator block holds whatever the last owner left
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3,) + self.dims, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, rgb: torch.Tensor, world_to_camera: torch.Tensor, intrinsics,
                  frames_per_launch: int = FRAMES_PER_LAUNCH) -> None:
        """Fuse N frames in order: depth float32 [N, H, W] metres, rgb uint8 [N, H, W, 3], world_to_camera [N, 4, 4] (or
        [N, 3, 4]), intrinsics (fx, fy, cx, cy) or a tensor [N, 4]; all tensors on the volume's GPU.  The frames are cut
        into launches of at most ``frames_per_launch``; the result does not depend on the cut."""
        if not (self.tsdf.is_cuda and depth.is_cuda and rgb.is_cuda):
            raise RuntimeError("TSDFVolume.integrate: the volume and the frames must be on the GPU -- no CPU fallback")
        if not 1 <= int(frames_per_launch) <= _lib.TSDF_MAX_FRAMES:
            raise ValueError(f"frames_per_launch must be in 1..{_lib.TSDF_MAX_FRAMES}")
        if depth.dim() != 3 or rgb.shape != depth.shape + (3,) or rgb.dtype != torch.uint8:
            raise ValueError(f"integrate: depth [N,H,W] float and rgb [N,H,W,3] uint8 expected, got {tuple(depth.shape)} {depth.dtype} "
                             f"and {tuple(rgb.shape)} {rgb.dtype}")
        dev = self.tsdf.device
        n, h, w = depth.shape
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
        rgb = rgb.to(device=dev).contiguous()
        w2c = torch.as_tensor(world_to_camera).to(device=dev, dtype=torch.float32)
        if w2c.shape[0] != n or tuple(w2c.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"integrate: world_to_camera [N,4,4] expected, got {tuple(w2c.shape)}")
        intr = torch.as_tensor(intrinsics, dtype=torch.float32).to(dev)
        intr = intr.expand(n, 4) if intr.dim() == 1 else intr
        table = torch.cat([w2c[:, :3, :4].reshape(n, 12), intr.reshape(n, 4)], dim=1).contiguous()  # [N, 16]
        lib = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nx, ny, nz = self.dims
        for lo in range(0, n, int(frames_per_launch)):
            k = min(int(frames_per_launch), n - lo)
            args = _lib.TsdfArgs(
                tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(), color=self.color.data_ptr(),
                frames=table[lo:].data_ptr(), depth=depth[lo:].data_ptr(), rgb=rgb[lo:].data_ptr(),
                nx=nx, ny=ny, nz=nz, K=k, H=h, W=w, lower_x=self.lower[0], lower_y=self.lower[1], lower_z=self.lower[2],
                voxel_size=self.voxel_size, trunc=self.trunc, depth_max=self.depth_max)
            _lib.check(lib.nvo_tsdf_integrate(stream, C.byref(args)), "tsdf_integrate")

    @torch.no_grad()
    def extract_mesh(self, weight_threshold: float = WEIGHT_THRESHOLD):
        """(vertices float32 [V, 3], faces int64 [F, 3], colors uint8 [V, 3], normals float32 [V, 3]) of the zero level set
        among voxels observed at least ``weight_threshold`` times.  Faces look into free space (positive distances)."""
        dev = self.tsdf.device
        # -tsdf: "behind the surface" is the inside of marching_tetrahedra, whose faces look away from the inside
        verts, faces = marching_tetrahedra(-self.tsdf, self.lower, self.upper_of_grid, 0.0, valid=self.weight >= weight_threshold)
        if verts.shape[0] == 0:
            return (verts, faces, torch.zeros(0, 3, dtype=torch.uint8, device=dev), torch.zeros(0, 3, device=dev))
        # colours: trilinear interpolation in the cube that holds the vertex.  A vertex lies on an edge or diagonal of a
        # cube whose eight corners are all valid; where it sits on a face shared with another cube, the corners off that
        # face get weight zero.
        lo = torch.as_tensor(self.lower, dtype=torch.float32, device=dev)
        g = (verts - lo) / self.voxel_size
        top = torch.tensor([max(d - 2, 0) for d in self.dims], device=dev)
        base = torch.minimum(g.floor().long().clamp(min=0), top)
        frac = (g - base.float()).clamp(0.0, 1.0)
        dims = torch.tensor(self.dims, device=dev)
        color = torch.zeros(verts.shape[0], 3, device=dev)
        flat = self.color.reshape(3, -1)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    off = torch.tensor([dx, dy, dz], device=dev)
                    c = torch.minimum(base + off, dims - 1)
                    wgt = (torch.where(off.bool(), frac, 1.0 - frac)).prod(dim=1)
                    lin = (c[:, 0] * self.dims[1] + c[:, 1]) * self.dims[2] + c[:, 2]
                    color += wgt[:, None] * flat[:, lin].T
        colors = color.round().clamp(0, 255).to(torch.uint8)
        # normals: area-weighted sum of the face normals around a vertex
        p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
        fn = torch.cross(p1 - p0, p2 - p0, dim=1)  # length = 2 x area
        normals = torch.zeros_like(verts)
        for corner in range(3):
            normals.index_add_(0, faces[:, corner], fn)
        normals = torch.nn.functional.normalize(normals, dim=1)
        return verts, faces, colors, normals


def snap_bounds(lower, upper, voxel_size: float, pad: float):
    """Box padded by ``pad`` and snapped outward to the lattice of integer multiples of ``voxel_size``."""
    lo = np.floor((np.asarray(lower, dtype=np.float64) - pad) / voxel_size) * voxel_size
    hi = np.ceil((np.asarray(upper, dtype=np.float64) + pad) / voxel_size) * voxel_size
    return lo, hi


def integrate_mesh(file_mesh: str, camera_intrinsics: dict, camera_extrinsics, frames_color: list, frames_depth: list,
                   lower=None, upper=None, device="cuda", frames_per_batch: int = 32) -> None:
    """The reference's ``integrate_mesh`` (same arguments; plus optional bounds): ``camera_extrinsics`` [N, 4, 4]
    camera-to-world, ``frames_color`` uint8 [H, W, 3] each, ``frames_depth`` metres [H, W] each.  Depths are quantised as
    the reference does before fusing, ``(depth * depth_scale).astype(uint16) / depth_scale``.  Without bounds the volume is
    the box of the back-projected valid pixels, padded by the truncation distance and snapped to the voxel lattice."""
    depth_scale = float(camera_intrinsics["depth_scale"])
    intr = tuple(float(camera_intrinsics[k]) for k in ("fx", "fy", "cx", "cy"))
    c2w = np.asarray(camera_extrinsics, dtype=np.float64)
    n = min(c2w.shape[0], len(frames_color), len(frames_depth))  # (the reference zips the three)
    if n == 0:
        raise ValueError("integrate_mesh: no frames")
    w2c = np.linalg.inv(c2w[:n])
    depths = np.stack([(np.asarray(d) * depth_scale).astype(np.uint16).astype(np.float32) / np.float32(depth_scale)
                       for d in frames_depth[:n]])
    colors = np.stack([np.ascontiguousarray(c, dtype=np.uint8) for c in frames_color[:n]])
    trunc = TRUNC_VOXELS * VOXEL_SIZE
    if lower is None or upper is None:
        lo, hi = frustum_bounds(torch.from_numpy(depths), c2w[:n], intr, DEPTH_TRUNCATION)
        lo, hi = snap_bounds(lo.numpy(), hi.numpy(), VOXEL_SIZE, trunc)
        lower = lo if lower is None else lower
        upper = hi if upper is None else upper
    dev = torch.device(device)
    volume = TSDFVolume(lower, upper, VOXEL_SIZE, TRUNC_VOXELS, DEPTH_TRUNCATION, device=dev)
    for b in range(0, n, frames_per_batch):
        e = min(n, b + frames_per_batch)
        volume.integrate(torch.from_numpy(depths[b:e]).to(dev), torch.from_numpy(colors[b:e]).to(dev),
                         torch.from_numpy(w2c[b:e]).to(dev), intr)
    verts, faces, vcol, vnrm = volume.extract_mesh(WEIGHT_THRESHOLD)
    write_mesh(file_mesh, verts, faces, colors=vcol, normals=vnrm)
