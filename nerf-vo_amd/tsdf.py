"""TSDF fusion of rendered frames into a mesh: the reference's ``integrate_mesh`` (evaluation/evaluation_utils.py:160-227
there, called by ``Renderer.render_mesh(source='frames')``) without Open3D.

The reference fuses with Open3D's ``VoxelBlockGrid`` on the CPU (voxel 1/64, depth truncation 5.0, Open3D's default
truncation band of 8 voxels and its default extraction weight of 3).  Here the volume is a DENSE box on the GPU, the
frames are fused by one HIP kernel (csrc/tsdf.hip: ``nvo_tsdf_integrate``, the rule is stated there and in DESIGN.md
"TSDF fusion") and the surface is extracted by ``meshing.marching_tetrahedra`` with a validity mask.  There is no CPU
fallback for the fusion; allocation, bounds and extraction are plain torch and work on any device.

``TSDFBlockVolume`` (``integrate_mesh(volume='blocks')``) is the reference's shape instead: blocks of 8^3 voxels behind a
dense block table, allocated where a frame's truncation band touches them and fused and meshed block by block in HIP
(csrc/tsdf_blocks.hip, csrc/iso_blocks.hip; DESIGN.md "Block-sparse TSDF volume").  It has no limit of 2^29 voxels on the
box, a frame updates only the blocks inside its own band, and its mesh is bit-reproducible.  Opt-in: the default is the
dense volume, whose results it does not change.

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


def _parse_box(name, lower, upper, voxel_size, trunc_voxels, depth_max):
    """(lower, upper) of a volume's box as float64 [3]; a ValueError unless the box and the three settings make sense."""
    lo, hi = (np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64).reshape(3) for x in (lower, upper))
    if not (voxel_size > 0 and trunc_voxels > 0 and depth_max > 0):
        raise ValueError(f"{name}: voxel_size, trunc_voxels and depth_max must be positive")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"{name}: bad box {lo.tolist()} .. {hi.tolist()}")
    return lo, hi


def lattice_dims(lo, hi, voxel_size: float) -> tuple:
    """Samples per axis of the lattice over [lo, hi]: ``lo + i * voxel_size`` up to the first one at or beyond hi."""
    return tuple(int(math.ceil((h - l) / voxel_size - 1e-6)) + 1 for l, h in zip(lo, hi))


def _pose(m, name, n, what):
    m = torch.as_tensor(m)
    if m.dim() != 3 or m.shape[0] != n or tuple(m.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"{what}: {name} [N,4,4] expected, got {tuple(m.shape)}")
    return m


def _frame_table(world_to_camera, intrinsics, n, device, what):
    """The kernels' frame table, float32 [N, 16]: world->camera 3x4 row-major, then fx fy cx cy."""
    w2c = _pose(world_to_camera, "world_to_camera", n, what).to(device=device, dtype=torch.float32)
    intr = torch.as_tensor(intrinsics, dtype=torch.float32).to(device)
    intr = intr.expand(n, 4) if intr.dim() == 1 else intr
    if tuple(intr.shape) != (n, 4):
        raise ValueError(f"{what}: intrinsics (fx, fy, cx, cy) or [N,4] expected, got {tuple(intr.shape)}")
    return torch.cat([w2c[:, :3, :4].reshape(n, 12), intr], dim=1).contiguous()


def _check_frames_per_launch(frames_per_launch) -> int:
    if not 1 <= int(frames_per_launch) <= _lib.TSDF_MAX_FRAMES:
        raise ValueError(f"frames_per_launch must be in 1..{_lib.TSDF_MAX_FRAMES}")
    return int(frames_per_launch)


class TSDFVolume:
    """Dense truncated-signed-distance volume over [lower, upper]: voxel (i, j, k) samples ``lower + (i, j, k) * voxel_size``
    (no half-voxel offset).  ``tsdf`` / ``weight`` float32 [nx, ny, nz], ``color`` float32 [3, nx, ny, nz] (0..255)."""

    def __init__(self, lower, upper, voxel_size: float = VOXEL_SIZE, trunc_voxels: float = TRUNC_VOXELS,
                 depth_max: float = DEPTH_TRUNCATION, device="cuda", max_voxels: int = 2 ** 29) -> None:
        lo, hi = _parse_box("TSDFVolume", lower, upper, voxel_size, trunc_voxels, depth_max)
        self.voxel_size = float(voxel_size)
        self.trunc = float(trunc_voxels) * self.voxel_size
        self.depth_max = float(depth_max)
        self.dims = lattice_dims(lo, hi, self.voxel_size)
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
        fpl = _check_frames_per_launch(frames_per_launch)
        if depth.dim() != 3 or rgb.shape != depth.shape + (3,) or rgb.dtype != torch.uint8:
            raise ValueError(f"integrate: depth [N,H,W] float and rgb [N,H,W,3] uint8 expected, got {tuple(depth.shape)} {depth.dtype} "
                             f"and {tuple(rgb.shape)} {rgb.dtype}")
        dev = self.tsdf.device
        n, h, w = depth.shape
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
        rgb = rgb.to(device=dev).contiguous()
        table = _frame_table(world_to_camera, intrinsics, n, dev, "integrate")
        lib = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nx, ny, nz = self.dims
        for lo in range(0, n, fpl):
            k = min(fpl, n - lo)
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


BLOCK = _lib.TSDF_BLOCK                 # voxels per block edge: the reference's BLOCK_RESOLUTION
BLOCK_VOXELS = BLOCK ** 3
BLOCK_COUNT = 100000                    # the reference's BLOCK_COUNT: initial capacity of the pool


def block_table_dims(lower, upper, voxel_size: float = VOXEL_SIZE) -> tuple:
    """Blocks per axis of the table that covers [lower, upper]: the dense volume's sample count per axis (samples
    ``lower + i * voxel_size`` up to the first one at or beyond upper), rounded up to whole blocks.  Raises a ValueError
    beyond 2^26 entries."""
    lo = np.asarray(lower, dtype=np.float64).reshape(3)
    hi = np.asarray(upper, dtype=np.float64).reshape(3)
    tb = tuple(-(-d // BLOCK) for d in lattice_dims(lo, hi, voxel_size))
    n = tb[0] * tb[1] * tb[2]
    if n > _lib.TSDF_BLOCKS_MAX_TABLE:
        raise ValueError(
            f"TSDFBlockVolume: the box {lo.tolist()} .. {hi.tolist()} needs a table of {tb[0]} x {tb[1]} x {tb[2]} = {n} blocks of "
            f"{BLOCK}^3 voxels of {voxel_size:g}, more than {_lib.TSDF_BLOCKS_MAX_TABLE} (2^26) entries: pass a tighter lower / "
            "upper or a larger voxel_size")
    return tb


class TSDFBlockVolume:
    """Block-sparse truncated-signed-distance volume over [lower, upper] (DESIGN.md "Block-sparse TSDF volume"): the
    lattice of ``TSDFVolume`` -- voxel (i, j, k) samples ``lower + (i, j, k) * voxel_size`` -- cut into blocks of 8^3
    voxels, of which only those a frame's truncation band touches are allocated, as in the reference's VoxelBlockGrid.

    ``table`` int32 [tbx, tby, tbz]: -1 or the block's id in the pool.  Pool: ``tsdf`` / ``weight`` float32
    [capacity, 512], ``color`` float32 [capacity, 3, 512] (0..255), local index (li * 8 + lj) * 8 + lk; it starts with
    ``block_count`` blocks and grows by reallocation.  Ids are handed out in ascending table order per launch, so they
    depend on how frames were cut into launches; nothing ``to_dense`` or ``extract_mesh`` returns does."""

    def __init__(self, lower, upper, voxel_size: float = VOXEL_SIZE, trunc_voxels: float = TRUNC_VOXELS,
                 depth_max: float = DEPTH_TRUNCATION, device="cuda", block_count: int = BLOCK_COUNT) -> None:
        lo, hi = _parse_box("TSDFBlockVolume", lower, upper, voxel_size, trunc_voxels, depth_max)
        if not 1 <= int(block_count) <= _lib.TSDF_BLOCKS_MAX_ALLOCATED:
            raise ValueError(f"TSDFBlockVolume: block_count {block_count} not in 1..{_lib.TSDF_BLOCKS_MAX_ALLOCATED} "
                             "(block id * 512 + local index must stay below 2^31)")
        self.voxel_size = float(voxel_size)
        self.trunc = float(trunc_voxels) * self.voxel_size
        self.depth_max = float(depth_max)
        self.table_dims = block_table_dims(lo, hi, self.voxel_size)
        self.dims = tuple(BLOCK * t for t in self.table_dims)  # the lattice: whole blocks
        self.lower = lo
        self.upper_of_grid = lo + (np.asarray(self.dims) - 1) * self.voxel_size
        self.device = torch.device(device)
        self.block_count = int(block_count)
        self.table = torch.full(self.table_dims, -1, dtype=torch.int32, device=self.device)
        self._marks = torch.zeros(self.table_dims, dtype=torch.int32, device=self.device)  # all zero between launches
        self._block_index = torch.zeros(0, dtype=torch.int64, device=self.device)          # table index of block id
        self.tsdf = self.weight = self.color = None                                        # the pool: at the first allocation
        # samples per pixel of the touch rule: n = 0 .. ceil(2 trunc / h) + 1, h = voxel_size / 2, from the float32 values
        # the kernel receives
        self._touch_samples = int(math.ceil(2.0 * float(np.float32(self.trunc)) / (0.5 * float(np.float32(self.voxel_size))))) + 2

    # ---- bookkeeping ----
    @property
    def n_blocks(self) -> int:
        return int(self._block_index.shape[0])

    @property
    def capacity(self) -> int:
        return 0 if self.tsdf is None else int(self.tsdf.shape[0])

    @property
    def block_coords(self) -> torch.Tensor:
        """int64 [n_blocks, 3]: (bi, bj, bk) of every allocated block, in id order."""
        _, tby, tbz = self.table_dims
        t = self._block_index
        return torch.stack([t // (tby * tbz), (t // tbz) % tby, t % tbz], dim=1)

    def _reserve(self, n: int) -> None:
        """Room for ``n`` blocks in the pool: zeroed explicitly (a recycled allocator block holds whatever its last owner
        left), the old blocks copied over."""
        if n > _lib.TSDF_BLOCKS_MAX_ALLOCATED:
            raise ValueError(f"TSDFBlockVolume: {n} blocks needed, more than {_lib.TSDF_BLOCKS_MAX_ALLOCATED}: block id * 512 + "
                             "local index must stay below 2^31 -- fuse a smaller region or use a larger voxel_size")
        if n <= self.capacity:
            return
        cap = min(max(n, 2 * self.capacity, self.block_count), _lib.TSDF_BLOCKS_MAX_ALLOCATED)
        old = (self.tsdf, self.weight, self.color)
        self.tsdf = torch.zeros((cap, BLOCK_VOXELS), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((cap, BLOCK_VOXELS), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((cap, 3, BLOCK_VOXELS), dtype=torch.float32, device=self.device)
        if old[0] is not None:
            for new, prev in zip((self.tsdf, self.weight, self.color), old):
                new[: prev.shape[0]].copy_(prev)

    def _allocate_blocks(self, table_index: torch.Tensor) -> None:
        """Give the unallocated ones of ``table_index`` (int64, ascending) the next ids, in that order."""
        flat = self.table.view(-1)
        new = table_index[flat[table_index] < 0]
        if new.numel() == 0:
            return
        first = self.n_blocks
        self._reserve(first + int(new.numel()))
        flat[new] = torch.arange(first, first + new.numel(), dtype=torch.int32, device=self.device)
        self._block_index = torch.cat([self._block_index, new])

    # ---- frames ----
    def _frames(self, depth, world_to_camera, intrinsics, camera_to_world, what):
        if not (self.table.is_cuda and torch.is_tensor(depth) and depth.is_cuda):
            raise RuntimeError(f"TSDFBlockVolume.{what}: the volume and the frames must be on the GPU -- no CPU fallback")
        if depth.dim() != 3:
            raise ValueError(f"{what}: depth [N,H,W] float expected, got {tuple(depth.shape)}")
        dev = self.device
        n = depth.shape[0]
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()

        def inverse(m):  # of the float32 matrices, in float64, rounded once
            full = torch.eye(4, dtype=torch.float64, device=dev).repeat(n, 1, 1)
            full[:, :3, :4] = m[:, :3, :4].double()
            return torch.linalg.inv(full).float()

        if world_to_camera is None and camera_to_world is None:
            raise ValueError(f"{what}: world_to_camera or camera_to_world is needed")
        if camera_to_world is None:  # the float32 matrix the touch rule maps with
            c2w = inverse(_pose(world_to_camera, "world_to_camera", n, what).to(device=dev, dtype=torch.float32))
        else:
            c2w = _pose(camera_to_world, "camera_to_world", n, what).to(device=dev, dtype=torch.float32)
            if world_to_camera is None:
                world_to_camera = inverse(c2w)
        frames = _frame_table(world_to_camera, intrinsics, n, dev, what)
        k_pix = (0.5 * torch.sqrt(1.0 / frames[:, 12].double() ** 2 + 1.0 / frames[:, 13].double() ** 2)).float()
        touch = torch.cat([c2w[:, :3, :4].reshape(n, 12), k_pix[:, None], torch.zeros(n, 3, device=dev)], dim=1).contiguous()
        return depth, frames, touch

    def _args(self, depth, frames, touch, lo, k, **kw):
        tbx, tby, tbz = self.table_dims
        _, h, w = depth.shape
        return _lib.TsdfBlocksArgs(
            table=self.table.data_ptr(), frames=frames[lo:].data_ptr(), touch_frames=touch[lo:].data_ptr(),
            depth=depth[lo:].data_ptr(), tbx=tbx, tby=tby, tbz=tbz, K=k, H=h, W=w, n_samples=self._touch_samples,
            lower_x=self.lower[0], lower_y=self.lower[1], lower_z=self.lower[2], voxel_size=self.voxel_size, trunc=self.trunc,
            depth_max=self.depth_max, **kw)

    def _touch(self, depth, frames, touch, lo, k):
        """(table indices int64 ascending, frame masks int32) of the blocks the frames lo .. lo + k - 1 touch."""
        args = self._args(depth, frames, touch, lo, k, marks=self._marks.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib().nvo_tsdf_blocks_touch(stream, C.byref(args)), "tsdf_blocks_touch")
        marks = self._marks.view(-1)
        index = torch.nonzero(marks).flatten()
        mask = marks[index]
        marks[index] = 0
        return index, mask

    @torch.no_grad()
    def touched_blocks(self, depth, camera_to_world, intrinsics) -> list:
        """Per frame, the table indices (int64, ascending; index = (bi * tby + bj) * tbz + bk) of the blocks its truncation
        band touches by the touch rule.  Allocates nothing."""
        depth, frames, touch = self._frames(depth, None, intrinsics, camera_to_world, "touched_blocks")
        out = []
        with torch.cuda.device(self.device):
            for lo in range(0, depth.shape[0], _lib.TSDF_MAX_FRAMES):
                k = min(_lib.TSDF_MAX_FRAMES, depth.shape[0] - lo)
                index, mask = self._touch(depth, frames, touch, lo, k)
                out += [index[(mask >> f) & 1 != 0] for f in range(k)]
        return out

    @torch.no_grad()
    def allocate(self, depth, camera_to_world, intrinsics) -> None:
        """Allocate every block the frames touch (depth [N, H, W], camera_to_world [N, 4, 4] float32 as the rule maps with,
        intrinsics as in ``integrate``) without fusing anything."""
        depth, frames, touch = self._frames(depth, None, intrinsics, camera_to_world, "allocate")
        with torch.cuda.device(self.device):
            for lo in range(0, depth.shape[0], _lib.TSDF_MAX_FRAMES):
                index, _ = self._touch(depth, frames, touch, lo, min(_lib.TSDF_MAX_FRAMES, depth.shape[0] - lo))
                self._allocate_blocks(index)

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, rgb: torch.Tensor, world_to_camera: torch.Tensor, intrinsics, camera_to_world=None,
                  frames_per_launch: int = FRAMES_PER_LAUNCH, blocks: str = "touched") -> None:
        """Fuse N frames in order; arguments as ``TSDFVolume.integrate``, plus ``camera_to_world`` [N, 4, 4]: the float32
        matrices the touch rule maps with (default: the float64 inverse of ``world_to_camera``, rounded to float32).

        ``blocks='touched'`` (the reference's rule): per launch the blocks its frames touch are marked, the new ones
        allocated, and frame f goes into a block iff f touched it.  ``blocks='allocated'``: every frame goes into every
        block allocated so far (see ``allocate``), the dense rule restricted to those blocks.  Either way the result does
        not depend on ``frames_per_launch`` or on how the frames are split over calls."""
        fpl = _check_frames_per_launch(frames_per_launch)
        if blocks not in ("touched", "allocated"):
            raise ValueError(f"integrate: blocks must be 'touched' or 'allocated', got {blocks!r}")
        if not (torch.is_tensor(rgb) and torch.is_tensor(depth) and depth.dim() == 3 and rgb.shape == depth.shape + (3,)
                and rgb.dtype == torch.uint8):
            raise ValueError("integrate: depth [N,H,W] float and rgb [N,H,W,3] uint8 expected")
        depth, frames, touch = self._frames(depth, world_to_camera, intrinsics, camera_to_world, "integrate")
        if not rgb.is_cuda:
            raise RuntimeError("TSDFBlockVolume.integrate: the volume and the frames must be on the GPU -- no CPU fallback")
        rgb = rgb.to(device=self.device).contiguous()
        lib = _lib.lib()
        n = depth.shape[0]
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            if blocks == "allocated":
                index = torch.sort(self._block_index).values
            for lo in range(0, n, fpl):
                k = min(fpl, n - lo)
                if blocks == "touched":
                    index, mask = self._touch(depth, frames, touch, lo, k)
                    self._allocate_blocks(index)
                else:
                    mask = torch.full_like(index, (1 << k) - 1, dtype=torch.int32)
                if index.numel() == 0:
                    continue
                block_list = index.to(torch.int32)
                args = self._args(depth, frames, touch, lo, k, tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(),
                                  color=self.color.data_ptr(), rgb=rgb[lo:].data_ptr(), list=block_list.data_ptr(),
                                  list_mask=mask.data_ptr(), n_list=int(block_list.numel()), n_allocated=self.n_blocks)
                _lib.check(lib.nvo_tsdf_blocks_integrate(stream, C.byref(args)), "tsdf_blocks_integrate")

    # ---- reading ----
    @torch.no_grad()
    def to_dense(self, index_range=None):
        """(tsdf, weight, color [3, ...], allocated bool) over the voxel index range ((i0, i1), (j0, j1), (k0, k1)),
        half-open (default: the whole lattice); zeros where the block is not allocated."""
        rng = tuple((0, d) for d in self.dims) if index_range is None else tuple((int(a), int(b)) for a, b in index_range)
        if any(not 0 <= a <= b <= d for (a, b), d in zip(rng, self.dims)):
            raise ValueError(f"to_dense: index range {rng} outside the lattice {self.dims}")
        dev = self.device
        ax = [torch.arange(a, b, device=dev) for a, b in rng]
        _, tby, tbz = self.table_dims
        bi, bj, bk = (x // BLOCK for x in ax)
        li, lj, lk = (x % BLOCK for x in ax)
        index = (bi[:, None, None] * tby + bj[None, :, None]) * tbz + bk[None, None, :]
        local = (li[:, None, None] * BLOCK + lj[None, :, None]) * BLOCK + lk[None, None, :]
        ids = self.table.view(-1)[index].long()
        allocated = ids >= 0
        shape = tuple(allocated.shape)
        if self.tsdf is None:
            zero = torch.zeros(shape, dtype=torch.float32, device=dev)
            return zero, zero.clone(), torch.zeros((3,) + shape, dtype=torch.float32, device=dev), allocated
        ids = ids.clamp(min=0)
        flat = ids * BLOCK_VOXELS + local
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        tsdf = torch.where(allocated, self.tsdf.view(-1)[flat], zero)
        weight = torch.where(allocated, self.weight.view(-1)[flat], zero)
        color = torch.stack([torch.where(allocated, self.color.view(-1)[ids * (3 * BLOCK_VOXELS) + ch * BLOCK_VOXELS + local], zero)
                             for ch in range(3)])
        return tsdf, weight, color, allocated

    @torch.no_grad()
    def extract_mesh(self, weight_threshold: float = WEIGHT_THRESHOLD):
        """(vertices float32 [V, 3], faces int64 [F, 3], colors uint8 [V, 3], normals float32 [V, 3]) of the zero level set
        among voxels of allocated blocks observed at least ``weight_threshold`` times, by the block-aware edge-owned
        extractor (csrc/iso_blocks.hip): the surface ``extract_isosurface(-tsdf, ..., valid)`` gives on ``to_dense``.
        Blocks are walked in ascending table order.  Colours are interpolated along the vertex's edge by the kernel;
        normals are the area-weighted face normals summed per vertex in face order, in float64 (no atomics).  The same
        bits from run to run, whatever the allocation history.  Zero-area triangles are kept."""
        dev = self.device
        n = self.n_blocks
        empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.long, device=dev),
                 torch.zeros(0, 3, dtype=torch.uint8, device=dev), torch.zeros(0, 3, device=dev))
        if n == 0:
            return empty
        if not self.table.is_cuda:
            raise RuntimeError("TSDFBlockVolume.extract_mesh: the volume must be on the GPU -- no CPU fallback")
        lib = _lib.lib()
        tbx, tby, tbz = self.table_dims
        order = torch.sort(self._block_index).values
        ids = self.table.view(-1)[order].long()
        order32 = order.to(torch.int32)
        totals = torch.zeros(2, n, dtype=torch.int64, device=dev)
        vrank = torch.zeros(n * BLOCK_VOXELS, dtype=torch.int32, device=dev)
        mask = torch.zeros(n * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        tcount = torch.zeros(n * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        args = _lib.TsdfBlocksIsoArgs(
            table=self.table.data_ptr(), tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(), color=self.color.data_ptr(),
            order=order32.data_ptr(), totals=totals.data_ptr(), vrank=vrank.data_ptr(), mask=mask.data_ptr(),
            tcount=tcount.data_ptr(), n_blocks=n, n_allocated=n, tbx=tbx, tby=tby, tbz=tbz,
            weight_threshold=float(weight_threshold), lower=(C.c_float * 3)(*[float(x) for x in self.lower]),
            voxel_size=self.voxel_size)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.nvo_tsdf_blocks_iso_count(stream, C.byref(args)), "tsdf_blocks_iso_count")
            in_order = totals[:, ids]
            ends = torch.cumsum(in_order, dim=1)
            bases = torch.empty_like(totals)
            bases[:, ids] = ends - in_order
            n_vert, n_face = (int(x) for x in ends[:, -1].tolist())
            if n_vert >= 2 ** 31 or n_face >= 2 ** 31:
                raise RuntimeError(f"TSDFBlockVolume.extract_mesh: {n_vert} vertices and {n_face} faces -- each must stay below 2^31")
            if n_vert == 0:
                return empty
            vertices = torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
            colors = torch.empty(n_vert, 3, dtype=torch.uint8, device=dev)
            faces = torch.empty(n_face, 3, dtype=torch.int32, device=dev)
            args.vertex_base, args.face_base = bases[0].data_ptr(), bases[1].data_ptr()
            args.vertices, args.colors, args.faces = vertices.data_ptr(), colors.data_ptr(), faces.data_ptr()
            args.n_vertices, args.n_faces = n_vert, n_face
            _lib.check(lib.nvo_tsdf_blocks_iso_emit(stream, C.byref(args)), "tsdf_blocks_iso_emit")
        faces = faces.long()
        return vertices, faces, colors, vertex_normals(vertices, faces)


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Area-weighted face normals (float32 cross products) summed per vertex in face order, in float64, normalised, as
    float32 [V, 3]: a stable sort by vertex, then the r-th face of every vertex is added in round r (a vertex of a
    marching-tetrahedra mesh has a couple of dozen faces at most) -- segment sums without atomics, sequential within a
    vertex, the same bits from run to run.  A vertex without a face gets (0, 0, 0)."""
    n_vert = vertices.shape[0]
    if faces.shape[0] == 0:
        return torch.zeros_like(vertices)
    p0, p1, p2 = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    fn = torch.cross(p1 - p0, p2 - p0, dim=1).double()  # length = 2 x area
    key, order = torch.sort(faces.reshape(-1), stable=True)  # entry 3 f + corner: face order within a vertex
    face_of = order // 3
    counts = torch.bincount(key, minlength=n_vert)
    starts = torch.cumsum(counts, dim=0) - counts
    sums = torch.zeros(n_vert, 3, dtype=torch.float64, device=fn.device)
    for r in range(int(counts.max())):
        has = (counts > r).nonzero().flatten()
        sums[has] += fn[face_of[starts[has] + r]]
    return torch.nn.functional.normalize(sums, dim=1).float()


def snap_bounds(lower, upper, voxel_size: float, pad: float):
    """Box padded by ``pad`` and snapped outward to the lattice of integer multiples of ``voxel_size``."""
    lo = np.floor((np.asarray(lower, dtype=np.float64) - pad) / voxel_size) * voxel_size
    hi = np.ceil((np.asarray(upper, dtype=np.float64) + pad) / voxel_size) * voxel_size
    return lo, hi


def integrate_mesh(file_mesh: str, camera_intrinsics: dict, camera_extrinsics, frames_color: list, frames_depth: list,
                   lower=None, upper=None, device="cuda", frames_per_batch: int = 32, volume: str = "dense") -> None:
    """The reference's ``integrate_mesh`` (same arguments; plus optional bounds and the kind of volume: ``'dense'``, a
    ``TSDFVolume`` over the box, or ``'blocks'``, a ``TSDFBlockVolume`` -- the reference's shape, without the dense
    volume's limit on the box and with another rule of which frames reach a voxel): ``camera_extrinsics`` [N, 4, 4]
    camera-to-world, ``frames_color`` uint8 [H, W, 3] each, ``frames_depth`` metres [H, W] each.  Depths are quantised as
    the reference does before fusing, ``(depth * depth_scale).astype(uint16) / depth_scale``.  Without bounds the volume is
    the box of the back-projected valid pixels, padded by the truncation distance and snapped to the voxel lattice."""
    if volume not in ("dense", "blocks"):
        raise ValueError(f"integrate_mesh: volume must be 'dense' or 'blocks', got {volume!r}")
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
    blocks = volume == "blocks"
    vol = (TSDFBlockVolume if blocks else TSDFVolume)(lower, upper, VOXEL_SIZE, TRUNC_VOXELS, DEPTH_TRUNCATION, device=dev)
    for b in range(0, n, frames_per_batch):
        e = min(n, b + frames_per_batch)
        extra = {"camera_to_world": torch.from_numpy(c2w[b:e]).to(dev)} if blocks else {}
        vol.integrate(torch.from_numpy(depths[b:e]).to(dev), torch.from_numpy(colors[b:e]).to(dev),
                      torch.from_numpy(w2c[b:e]).to(dev), intr, **extra)
    verts, faces, vcol, vnrm = vol.extract_mesh(WEIGHT_THRESHOLD)
    write_mesh(file_mesh, verts, faces, colors=vcol, normals=vnrm)
