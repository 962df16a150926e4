"""CPU side of the block-sparse TSDF volume (nerf_vo_amd/tsdf.py ``TSDFBlockVolume``): the touch rule's coverage of the
per-voxel rule, argument validation in Python and in the launchers, and the extent the block table admits where the dense
volume refuses.  The kernels are tested on the GPU (test_tsdf_blocks_gpu.py).

Scene: ``room_scene()`` of helpers/tsdf_oracle.py (8 frames 72 x 96), voxel 1/64, lower (-0.5625, -0.5625, -0.42), lattice
72 x 72 x 56 = a table of 9 x 9 x 7 blocks."""
import functools

import numpy as np
import pytest
import torch

from helpers.tsdf_blocks_oracle import BLOCK, touch_rule, touch_samples
from helpers.tsdf_oracle import frame_table, fuse, room_scene

VOXEL = 1.0 / 64.0
DEPTH_MAX = 5.0
LOWER = (-0.5625, -0.5625, -0.42)
TABLE = (9, 9, 7)
DIMS = tuple(BLOCK * t for t in TABLE)
UPPER = tuple(l + (d - 1) * VOXEL for l, d in zip(LOWER, DIMS))


@functools.lru_cache(maxsize=None)
def _scene():
    return room_scene()


@pytest.mark.parametrize("trunc_voxels", [8.0, 4.0])
def test_touch_rule_covers_the_per_voxel_rule(trunc_voxels):
    """For every frame, every voxel the float64 oracle updates with tsdf < 1 (inside the band, not merely free space in
    front of it) and does not flag as hanging on a rounding decision lies in a block the float32 touch rule marks."""
    depth, rgb, w2c, c2w, intr = _scene()
    trunc = trunc_voxels * VOXEL
    touched = touch_rule(LOWER, VOXEL, trunc, DEPTH_MAX, TABLE, c2w.float().numpy(), intr, depth.numpy())
    assert touched.shape == (8,) + TABLE and touch_samples(VOXEL, trunc) == int(4 * trunc_voxels) + 2
    table = frame_table(w2c.numpy(), intr)
    I, J, K = np.meshgrid(*[np.arange(d) // BLOCK for d in DIMS], indexing="ij")
    needed_any = np.zeros(TABLE, dtype=bool)
    for f in range(depth.shape[0]):
        ref = fuse(LOWER, VOXEL, trunc, DEPTH_MAX, tuple((0, d) for d in DIMS), table[f:f + 1], depth[f:f + 1].numpy(),
                   rgb[f:f + 1].numpy())
        in_band = (ref["weight"] > 0) & (ref["tsdf"] < 1.0) & ~ref["ambiguous"]
        assert int(in_band.sum()) > 1000
        missed = in_band & ~touched[f][I, J, K]
        assert not missed.any(), f"frame {f}: {int(missed.sum())} in-band voxels lie in blocks the touch rule did not mark"
        needed = np.zeros(TABLE, dtype=bool)
        needed[I[in_band], J[in_band], K[in_band]] = True
        needed_any |= needed
        print(f"trunc {trunc_voxels:g} voxels, frame {f}: {int(touched[f].sum())} blocks touched, {int(needed.sum())} needed "
              f"({touched[f].sum() / needed.sum():.2f} x)")
    total = touched.any(axis=0)
    print(f"trunc {trunc_voxels:g} voxels: {int(total.sum())} of {total.size} blocks allocated, {int(needed_any.sum())} needed")
    assert not (needed_any & ~total).any()


def test_touch_rule_ignores_invalid_depths():
    depth, _, _, c2w, intr = _scene()
    d = depth[:4].clone().numpy()
    d[0], d[1], d[2], d[3] = np.nan, 0.0, np.inf, DEPTH_MAX * 1.2
    assert not touch_rule(LOWER, VOXEL, 8 * VOXEL, DEPTH_MAX, TABLE, c2w[:4].float().numpy(), intr, d).any()


def test_argument_validation():
    from nerf_vo_amd.tsdf import TSDFBlockVolume, integrate_mesh

    good = dict(voxel_size=VOXEL, device="cpu")
    for bad in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(trunc_voxels=0.0), dict(depth_max=-1.0), dict(block_count=0),
                dict(block_count=2 ** 22 + 1)):
        with pytest.raises(ValueError):
            TSDFBlockVolume(LOWER, UPPER, **{**good, **bad})
    with pytest.raises(ValueError, match="bad box"):
        TSDFBlockVolume(UPPER, LOWER, **good)
    with pytest.raises(ValueError, match="bad box"):
        TSDFBlockVolume((0, 0, float("nan")), UPPER, **good)
    vol = TSDFBlockVolume(LOWER, UPPER, **good)
    assert vol.table_dims == TABLE and vol.dims == DIMS and vol.n_blocks == 0 and vol.block_coords.shape == (0, 3)
    assert vol.table.shape == TABLE and bool((vol.table == -1).all())
    np.testing.assert_allclose(vol.upper_of_grid, UPPER, rtol=0, atol=1e-12)
    tsdf, weight, color, allocated = vol.to_dense(((0, 9), (3, 20), (50, 56)))
    assert tsdf.shape == weight.shape == allocated.shape == (9, 17, 6) and color.shape == (3, 9, 17, 6)
    assert not bool(allocated.any()) and float(tsdf.abs().sum() + weight.abs().sum() + color.abs().sum()) == 0.0
    with pytest.raises(ValueError, match="index range"):
        vol.to_dense(((0, 73), (0, 1), (0, 1)))
    assert all(t.shape[0] == 0 for t in vol.extract_mesh())
    depth, rgb, pose, intr = torch.ones(1, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.eye(4)[None], (4.0, 4.0, 2.0, 2.0)
    with pytest.raises(ValueError, match="blocks must be"):
        vol.integrate(depth, rgb, pose, intr, blocks="all")
    for fpl in (0, 17):
        with pytest.raises(ValueError, match="frames_per_launch"):
            vol.integrate(depth, rgb, pose, intr, frames_per_launch=fpl)
    with pytest.raises(ValueError, match="uint8"):
        vol.integrate(depth, rgb.float(), pose, intr)
    for call in (lambda: vol.integrate(depth, rgb, pose, intr), lambda: vol.allocate(depth, pose, intr),
                 lambda: vol.touched_blocks(depth, pose, intr)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="volume must be"):
        integrate_mesh("unused.ply", {"depth_scale": 1000.0, "fx": 1, "fy": 1, "cx": 0, "cy": 0}, np.eye(4)[None], [None], [None],
                       volume="sparse")


def test_launchers_reject_bad_arguments():
    """The four launchers validate before they launch anything (no GPU is touched: every call here is refused)."""
    import ctypes as C

    from nerf_vo_amd import _lib

    lib = _lib.lib()
    good = dict(table=64, tsdf=64, weight=64, color=64, frames=64, touch_frames=64, depth=64, rgb=64, marks=64, list=64,
                list_mask=64, n_list=1, n_allocated=1, tbx=9, tby=9, tbz=7, K=1, H=4, W=4, n_samples=34, lower_x=0.0,
                lower_y=0.0, lower_z=0.0, voxel_size=1 / 64, trunc=8 / 64, depth_max=5.0)
    both = [dict(tbx=0), dict(tbx=1 << 27, tby=1, tbz=1), dict(tbx=512, tby=512, tbz=512), dict(K=0),
            dict(K=_lib.TSDF_MAX_FRAMES + 1), dict(H=0), dict(W=0), dict(voxel_size=0.0), dict(voxel_size=float("nan")),
            dict(trunc=-0.1), dict(frames=None), dict(depth=None)]
    only = {"touch": [dict(marks=None), dict(touch_frames=None), dict(n_samples=0), dict(n_samples=1 << 20)],
            "integrate": [dict(table=None), dict(tsdf=None), dict(weight=None), dict(color=None), dict(rgb=None), dict(list=None),
                          dict(list_mask=None), dict(n_allocated=(1 << 22) + 1), dict(n_list=568)]}
    for name, extra in only.items():
        fn = getattr(lib, f"nvo_tsdf_blocks_{name}")
        for change in both + extra:
            args = _lib.TsdfBlocksArgs(**{**good, **change})
            assert fn(None, C.byref(args)) == 1, (name, change)  # NVO_ERR_INVALID
            assert f"tsdf_blocks_{name}".encode() in lib.nvo_last_error()
        assert fn(None, None) == 1
    good = dict(table=64, tsdf=64, weight=64, color=64, order=64, totals=64, vrank=64, mask=64, tcount=64, vertex_base=64,
                face_base=64, vertices=64, colors=64, faces=64, n_vertices=3, n_faces=1, n_blocks=1, n_allocated=1, tbx=9,
                tby=9, tbz=7, weight_threshold=3.0, voxel_size=1 / 64)
    both = [dict(tbx=0), dict(tbx=512, tby=512, tbz=512), dict(n_blocks=2), dict(n_allocated=(1 << 22) + 1, n_blocks=1),
            dict(voxel_size=0.0), dict(table=None), dict(tsdf=None), dict(weight=None), dict(order=None), dict(totals=None),
            dict(vrank=None), dict(mask=None), dict(tcount=None)]
    only = {"count": [], "emit": [dict(n_vertices=1 << 31), dict(n_faces=1 << 31), dict(color=None), dict(vertex_base=None),
                                  dict(face_base=None), dict(vertices=None), dict(colors=None), dict(faces=None)]}
    for name, extra in only.items():
        fn = getattr(lib, f"nvo_tsdf_blocks_iso_{name}")
        for change in both + extra:
            args = _lib.TsdfBlocksIsoArgs(**{**good, **change})
            assert fn(None, C.byref(args)) == 1, (name, change)
            assert f"tsdf_blocks_iso_{name}".encode() in lib.nvo_last_error()
        assert fn(None, None) == 1


def test_extent_the_dense_volume_refuses():
    """A box of 400 x 400 x 400 blocks (50 m per axis at 1/64; 3.3e10 voxels): the dense volume raises, the block table
    (6.4e7 entries, below 2^26) takes it; 408 blocks per axis are too many and the error names the numbers."""
    from nerf_vo_amd.tsdf import TSDFVolume, block_table_dims

    lower = (0.0, 0.0, 0.0)
    upper = tuple((400 * BLOCK - 1) * VOXEL for _ in range(3))
    with pytest.raises(ValueError, match="max_voxels"):
        TSDFVolume(lower, upper, VOXEL, device="cpu")
    assert block_table_dims(lower, upper, VOXEL) == (400, 400, 400)
    assert block_table_dims(lower, tuple(u + VOXEL for u in upper), VOXEL) == (401, 401, 401)  # one more sample: one more block
    with pytest.raises(ValueError, match=r"408 x 408 x 408 = 67917312 .* 67108864"):
        block_table_dims(lower, tuple((408 * BLOCK - 1) * VOXEL for _ in range(3)), VOXEL)
