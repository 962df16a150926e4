"""The block-sparse TSDF volume on the GPU (nerf-vo_amd/csrc/tsdf_blocks.hip, iso_blocks.hip behind ``TSDFBlockVolume``
and ``render_mesh(source='frames', volume='blocks')``) against the numpy statements of helpers/tsdf_blocks_oracle.py, the
dense volume and the dense extractor.

Scene unless stated: ``room_scene()`` (8 frames 72 x 96, the analytic room [-0.5, 0.5]^3), voxel 1/64, depth_max 5, lower
(-0.5625, -0.5625, -0.42), lattice 72 x 72 x 56 = a table of 9 x 9 x 7 blocks.  The room's walls at z = +-0.5 lie outside
the table, so every frame's band leaves it.

Bounds against the float64 oracle are those of test_tsdf_gpu.py, unchanged (weights equal off the flagged voxels, |tsdf|
2e-5, colour 5e-3, flagged share at most 3 %): the per-voxel arithmetic is the same.  Everything else is bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers.tsdf_blocks_oracle import BLOCK, block_vertices, fuse_touched, touch_rule
from helpers.tsdf_oracle import frame_table, room_scene
from test_tsdf_gpu import _RoomNerf, _compare

pytestmark = pytest.mark.gpu

VOXEL = 1.0 / 64.0
DEPTH_MAX = 5.0
LOWER = (-0.5625, -0.5625, -0.42)
TABLE = (9, 9, 7)
DIMS = tuple(BLOCK * t for t in TABLE)


def _upper(lower, dims=DIMS):
    return tuple(l + (d - 1) * VOXEL for l, d in zip(lower, dims))


@functools.lru_cache(maxsize=None)
def _scene():
    depth, rgb, w2c, c2w, intr = room_scene()
    return depth, rgb, w2c, c2w.float(), intr  # the float32 camera-to-world the touch rule maps with


@functools.lru_cache(maxsize=None)
def _touched(trunc_voxels):
    depth, _, _, c2w, intr = _scene()
    return touch_rule(LOWER, VOXEL, trunc_voxels * VOXEL, DEPTH_MAX, TABLE, c2w.numpy(), intr, depth.numpy())


@functools.lru_cache(maxsize=None)
def _reference():
    depth, rgb, w2c, _, intr = _scene()
    return fuse_touched(LOWER, VOXEL, 8.0 * VOXEL, DEPTH_MAX, tuple((0, d) for d in DIMS), frame_table(w2c.numpy(), intr),
                        depth.numpy(), rgb.numpy(), _touched(8.0))


def _volume(device, lower=LOWER, trunc_voxels=8.0, **kw):
    from nerf_vo_amd.tsdf import TSDFBlockVolume

    vol = TSDFBlockVolume(lower, _upper(lower), VOXEL, trunc_voxels, DEPTH_MAX, device=device, **kw)
    assert vol.table_dims == TABLE and vol.dims == DIMS
    return vol


def _fuse(device, cuts=(8,), **kw):
    depth, rgb, w2c, c2w, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    vol = _volume(device, **kw)
    lo = 0
    for n in cuts:
        vol.integrate(depth[lo:lo + n], rgb[lo:lo + n], w2c[lo:lo + n], intr, camera_to_world=c2w[lo:lo + n], frames_per_launch=n)
        lo += n
    torch.cuda.synchronize()
    return vol


@functools.lru_cache(maxsize=None)
def _fused(device):
    """the scene fused in the default mode, one launch: shared, read only"""
    return _fuse(device)


def _sets(indices):
    return [np.sort(t.cpu().numpy()) for t in indices]


@pytest.mark.parametrize("trunc_voxels", [8.0, 4.0])
def test_touch_sets_equal_the_numpy_statement(device, trunc_voxels):
    depth, _, _, c2w, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    vol = _volume(device, trunc_voxels=trunc_voxels)
    got = _sets(vol.touched_blocks(depth, c2w, intr))
    want = _touched(trunc_voxels)
    assert len(got) == 8 and vol.n_blocks == 0 and not bool(vol._marks.any())
    for f in range(8):
        ref = np.flatnonzero(want[f])
        assert ref.size > 100
        assert np.array_equal(got[f], ref), f"frame {f}: {np.setxor1d(got[f], ref).size} blocks differ"


def test_touch_sets_of_frames_that_touch_nothing_and_of_a_band_that_leaves_the_table(device):
    depth, _, _, c2w, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    vol = _volume(device)
    d = depth[:5].clone()
    d[0], d[1], d[2], d[3] = float("nan"), 0.0, float("inf"), DEPTH_MAX * 1.2
    away = c2w[:5].clone()
    away[4, :3, 3] += 3.0  # frame 4 keeps its depths: its whole band lies beyond the table
    got = _sets(vol.touched_blocks(d, away, intr))
    assert [g.size for g in got] == [0, 0, 0, 0, 0]
    assert not touch_rule(LOWER, VOXEL, 8.0 * VOXEL, DEPTH_MAX, TABLE, away.cpu().numpy(), intr, d.cpu().numpy()).any()
    # a table around a part of the wall x = +0.5 only: the bands of the frames that see it leave the table on four sides (block
    # indices below 0 and beyond the end), the other frames touch nothing
    from nerf_vo_amd.tsdf import TSDFBlockVolume

    lower, dims = (0.25, -0.1875, -0.295), (40, 24, 32)
    part = TSDFBlockVolume(lower, _upper(lower, dims), VOXEL, 8.0, DEPTH_MAX, device=device)
    assert part.table_dims == (5, 3, 4)
    got = _sets(part.touched_blocks(depth, c2w, intr))
    want = touch_rule(lower, VOXEL, 8.0 * VOXEL, DEPTH_MAX, part.table_dims, c2w.cpu().numpy(), intr, depth.cpu().numpy())
    for f in range(8):
        assert np.array_equal(got[f], np.flatnonzero(want[f]))
    assert want.any(axis=(0, 1, 3)).all() and want.any(axis=(0, 1, 2)).all(), \
        "the marks reach the first and the last block of the table along y and z: the wall's band goes on beyond them"


def test_kernel_body_equals_the_dense_volume(device):
    """allocate(all frames) + integrate(blocks='allocated') is the dense fusion restricted to the allocated blocks."""
    from nerf_vo_amd.tsdf import TSDFVolume

    depth, rgb, w2c, c2w, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    dense = TSDFVolume(LOWER, _upper(LOWER), VOXEL, 8.0, DEPTH_MAX, device=device)
    assert dense.dims == DIMS
    dense.integrate(depth, rgb, w2c, intr, frames_per_launch=8)
    vol = _volume(device)
    vol.allocate(depth, c2w, intr)
    assert vol.n_blocks == int(_touched(8.0).any(axis=0).sum())
    vol.integrate(depth, rgb, w2c, intr, frames_per_launch=8, blocks="allocated")
    torch.cuda.synchronize()
    tsdf, weight, color, allocated = vol.to_dense()
    assert int(allocated.sum()) == vol.n_blocks * BLOCK ** 3 and float(weight.max()) >= 3.0
    assert torch.equal(tsdf[allocated], dense.tsdf[allocated])
    assert torch.equal(weight[allocated], dense.weight[allocated])
    assert torch.equal(color[:, allocated], dense.color[:, allocated])
    assert not bool(tsdf[~allocated].any() or weight[~allocated].any() or color[:, ~allocated].any())
    coords = vol.block_coords
    assert torch.equal(vol.table[coords[:, 0], coords[:, 1], coords[:, 2]].long(), torch.arange(vol.n_blocks, device=device))


def test_reference_rule_matches_float64_oracle(device):
    vol = _fused(device)
    ref = _reference()
    tsdf, weight, color, allocated = vol.to_dense()
    assert torch.equal(allocated.cpu(), torch.from_numpy(_touched(8.0).any(axis=0).repeat(8, 0).repeat(8, 1).repeat(8, 2)))
    assert bool(torch.isfinite(tsdf).all() and torch.isfinite(weight).all() and torch.isfinite(color).all())
    _compare((tsdf, weight, color), ref, "touched blocks")


def test_result_does_not_depend_on_batching_or_capacity(device):
    base = _fused(device)
    want = base.to_dense()
    mesh = base.extract_mesh()
    assert mesh[0].shape[0] > 1000
    for cuts, kw in (([1] * 8, {}), ([3, 3, 2], {}), ([8], {"block_count": 16}), ([3, 3, 2], {"block_count": 16})):
        vol = _fuse(device, tuple(cuts), **kw)
        assert vol.n_blocks == base.n_blocks and vol.capacity >= vol.n_blocks
        for a, b, name in zip(vol.to_dense(), want, ("tsdf", "weight", "color", "allocated")):
            assert torch.equal(a, b), f"{name} depends on the cut {cuts} / {kw}"
        for a, b, name in zip(vol.extract_mesh(), mesh, ("vertices", "faces", "colors", "normals")):
            assert torch.equal(a, b), f"mesh {name} depend on the cut {cuts} / {kw}"


def _canonical_triangles(vertices, faces):
    """[F, 9] uint32: the bits of each triangle's three positions, rotated to start at its lexicographically smallest
    vertex, rows sorted."""
    t = vertices.cpu().numpy()[faces.cpu().numpy()]  # [F, 3, 3]
    first = np.lexsort((t[:, :, 2], t[:, :, 1], t[:, :, 0]), axis=1)[:, 0]
    t = t[np.arange(t.shape[0])[:, None], (first[:, None] + np.arange(3)) % 3]
    rows = np.ascontiguousarray(t.reshape(-1, 9)).view(np.uint32)
    return rows[np.lexsort(rows.T[::-1])]


def test_extraction_equals_the_dense_extractor(device):
    from nerf_vo_amd.meshing import extract_isosurface

    vol = _fused(device)
    tsdf, weight, color, allocated = vol.to_dense()
    valid = (weight >= 3.0) & allocated
    v_ref, f_ref = extract_isosurface(-tsdf, vol.lower, vol.upper_of_grid, 0.0, valid)
    v, f, c, n = vol.extract_mesh(3.0)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and c.dtype == torch.uint8 and n.dtype == torch.float32
    assert v.shape[0] == v_ref.shape[0] > 1000 and f.shape == f_ref.shape
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    assert np.array_equal(_canonical_triangles(v, f), _canonical_triangles(v_ref, f_ref))
    again = vol.extract_mesh(3.0)
    for a, b in zip((v, f, c, n), again):
        assert torch.equal(a, b)
    pos, col = block_vertices((-tsdf).cpu().numpy(), valid.cpu().numpy(), color.cpu().numpy(), vol.lower, VOXEL)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(c.cpu().numpy(), col) and col.std(axis=0).min() > 1.0
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    fn = torch.cross(p1 - p0, p2 - p0, dim=1)
    summed = torch.zeros_like(v)
    for corner in range(3):
        summed.index_add_(0, f[:, corner], fn)
    summed = torch.nn.functional.normalize(summed, dim=1)
    assert bool(torch.isfinite(n).all()) and float((n - summed).abs().max()) <= 1e-5
    # another threshold: nothing of the one before is left in the scratch
    v1, f1 = extract_isosurface(-tsdf, vol.lower, vol.upper_of_grid, 0.0, (weight >= 1.0) & allocated)
    w1 = vol.extract_mesh(1.0)
    assert w1[0].shape[0] == v1.shape[0] > v.shape[0]
    assert np.array_equal(_canonical_triangles(w1[0], w1[1]), _canonical_triangles(v1, f1))


def test_extent_beyond_the_dense_volume(device):
    """A table of 400^3 blocks (50 m per axis; the dense volume would need 3.3e10 voxels) with the room around block
    (204, 204, 203): fusion and extraction run, and 3 x 3 x 3 blocks at the wall x = +0.5 match the float64 oracle."""
    from nerf_vo_amd.tsdf import TSDFBlockVolume, TSDFVolume

    depth, rgb, w2c, c2w, intr = _scene()
    lower = tuple(l - 200 * BLOCK * VOXEL for l in LOWER)
    upper = _upper(lower, (3200, 3200, 3200))
    with pytest.raises(ValueError, match="max_voxels"):
        TSDFVolume(lower, upper, VOXEL, 8.0, DEPTH_MAX, device=device)
    vol = TSDFBlockVolume(lower, upper, VOXEL, 8.0, DEPTH_MAX, device=device)
    assert vol.table_dims == (400, 400, 400)
    vol.integrate(depth.to(device), rgb.to(device), w2c.to(device), intr, camera_to_world=c2w.to(device))
    torch.cuda.synchronize()
    coords = vol.block_coords
    # the room spans the blocks 200 .. 208 per axis; a band reaches one block (the truncation distance) beyond a wall, rho less
    assert vol.n_blocks > 100 and int(coords.min()) >= 198 and int(coords.max()) <= 210
    blocks = ((206, 209), (203, 206), (202, 205))
    rng = tuple((a * BLOCK, b * BLOCK) for a, b in blocks)
    touched = touch_rule(lower, VOXEL, 8.0 * VOXEL, DEPTH_MAX, vol.table_dims, c2w.numpy(), intr, depth.numpy(), block_range=blocks)
    ref = fuse_touched(lower, VOXEL, 8.0 * VOXEL, DEPTH_MAX, rng, frame_table(w2c.numpy(), intr), depth.numpy(), rgb.numpy(), touched,
                       block_origin=tuple(a for a, _ in blocks))
    tsdf, weight, color, allocated = vol.to_dense(rng)
    assert torch.equal(allocated.cpu(), torch.from_numpy(touched.any(axis=0).repeat(8, 0).repeat(8, 1).repeat(8, 2)))
    _compare((tsdf, weight, color), ref, "3 x 3 x 3 blocks of the 400^3 table")
    v, f, c, n = vol.extract_mesh()
    assert v.shape[0] > 1000 and f.shape[0] > 1000 and int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    # a zero crossing lies between two observed voxels, and those lie inside the room or within the truncation distance behind a wall
    assert float(v.abs().max()) <= 0.5 + 9 * VOXEL
    assert bool(torch.isfinite(n).all()) and c.shape == v.shape


def test_render_mesh_end_to_end_with_the_block_volume(device, tmp_path):
    """render_frames() then render_mesh(volume='blocks') on the analytic room, as test_tsdf_gpu's end-to-end test."""
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.meshing import read_mesh
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=72, width=96, scene_scale=0.25)
    ds.evaluation_frames = list(range(ds.num_frames))
    keyframes = list(range(0, 24, 4))
    renderer = EvaluationRenderer(dataset=ds, nerf=_RoomNerf(ds, keyframes), keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    renderer.render_frames()
    path = renderer.render_mesh(source="frames", volume="blocks")
    assert path == str(tmp_path / "pred" / "mesh" / "mesh_from_evaluation_frames.ply") and os.path.exists(path)
    v, f, c, n = read_mesh(path)
    assert c is not None and n is not None and c.dtype == torch.uint8
    assert v.shape[0] >= 1000 and f.shape[0] > 0 and int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    to_wall = (v.double().abs() - 0.5).abs().min(dim=1).values / VOXEL
    inward = float(((n.double() * -v.double()).sum(dim=1) > 0).double().mean())
    print(f"{v.shape[0]} vertices, {f.shape[0]} faces, farthest vertex {float(to_wall.max()):.3f} voxel from a wall, normals inward "
          f"{inward:.4f}")
    assert float(to_wall.max()) <= 1.0
    assert inward >= 0.99
    assert float(c.double().std(dim=0).min()) > 1.0, "vertex colours are constant"
    with pytest.raises(ValueError, match="volume must be"):
        renderer.render_mesh(source="frames", volume="octree")
