"""TSDF fusion kernel (nerf-vo_amd/csrc/tsdf.hip) behind TSDFVolume.integrate and EvaluationRenderer.render_mesh, against
the float64 restatement of its rule (tests/helpers/tsdf_oracle.py).

Scene of tests 1-3: the analytic room [-0.5, 0.5]^3, 8 orbit cameras (translations x 0.25), 96 x 72 frames, voxel 1/64,
truncation 8 voxels, depth_max 5, into a volume of 72 x 67 x 53 voxels from (-0.5625, -0.5625, -0.42): no dimension is a
multiple of the kernel's brick, the cameras are inside the volume and bricks straddle the image borders.

Bounds against the oracle, outside the voxels it flags as hanging on a rounding decision: weight equal, |tsdf| within
2e-5, colour within 5e-3 of 255.  A float32 numpy evaluation of the same formulas differs from float64 by at most
8.8e-7 in tsdf and in no weight on this scene; the bound leaves ~20x for another operation order.  The flagged share of
observed voxels is 0.73 % for this box (CPU, oracle alone) and may not exceed 3 %."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers.tsdf_oracle import frame_table, fuse, room_scene
from test_tcnn_gpu import _assert_close

pytestmark = pytest.mark.gpu

VOXEL = 1.0 / 64.0
TRUNC_VOXELS = 8.0
DEPTH_MAX = 5.0
LOWER = (-0.5625, -0.5625, -0.42)
DIMS = (72, 67, 53)
TSDF_BOUND, COLOR_BOUND, MAX_FLAGGED = 2e-5, 5e-3, 0.03


@functools.lru_cache(maxsize=None)
def _scene():
    return room_scene()


@functools.lru_cache(maxsize=None)
def _reference():
    depth, rgb, w2c, _, intr = _scene()
    return fuse(LOWER, VOXEL, TRUNC_VOXELS * VOXEL, DEPTH_MAX, tuple((0, d) for d in DIMS), frame_table(w2c.numpy(), intr),
                depth.numpy(), rgb.numpy())


def _volume(device, lower=LOWER, dims=DIMS, **kw):
    from nerf_vo_amd.tsdf import TSDFVolume

    upper = [l + (d - 1) * VOXEL for l, d in zip(lower, dims)]
    vol = TSDFVolume(lower, upper, VOXEL, TRUNC_VOXELS, DEPTH_MAX, device=device, **kw)
    assert vol.dims == tuple(dims)
    return vol


def _compare(vol_tensors, ref, what):
    """weight exactly, tsdf and colour within the stated bounds, outside the flagged voxels; returns the flagged share."""
    tsdf, weight, color = (t.double().cpu() for t in vol_tensors)
    keep = torch.from_numpy(~ref["ambiguous"])
    r_t, r_w, r_c = (torch.from_numpy(ref[k]) for k in ("tsdf", "weight", "color"))
    observed = r_w > 0
    flagged = float((~keep & observed).sum()) / max(1, int(observed.sum()))
    print(f"{what}: {int(observed.sum())} observed voxels, flagged share {flagged:.4f}, max |tsdf err| "
          f"{float((tsdf - r_t)[keep].abs().max()):.3e}, max |colour err| {float((color - r_c)[:, keep].abs().max()):.3e}, "
          f"weights differing {int((weight != r_w)[keep].sum())}")
    assert flagged <= MAX_FLAGGED
    assert int(observed[keep].sum()) > 1000, "the comparison must cover observed voxels"
    assert torch.equal(weight[keep], r_w[keep]), f"{what}: {int((weight != r_w)[keep].sum())} weights differ"
    _assert_close(tsdf[keep], r_t[keep], 0.0, TSDF_BOUND / float(r_t[keep].abs().max()), f"{what} tsdf")
    _assert_close(color[:, keep], r_c[:, keep], 0.0, COLOR_BOUND / float(r_c[:, keep].abs().max()), f"{what} colour")
    return flagged


# Tests 1-3 record their outcome: the large-index test runs only behind them (it runs them itself when they were not
# selected) and launches nothing when one of them failed.
_OUTCOME = {}


def _run(name, body, device):
    if name in _OUTCOME:
        if not _OUTCOME[name]:
            pytest.fail(f"{name}: failed earlier in this session")
        return
    _OUTCOME[name] = False
    body(device)
    _OUTCOME[name] = True


def _check_oracle(device):
    depth, rgb, w2c, _, intr = _scene()
    vol = _volume(device)
    vol.integrate(depth.to(device), rgb.to(device), w2c.to(device), intr, frames_per_launch=8)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vol.tsdf).all() and torch.isfinite(vol.weight).all() and torch.isfinite(vol.color).all())
    _compare((vol.tsdf, vol.weight, vol.color), _reference(), "ragged box")


def _check_batching(device):
    depth, rgb, w2c, _, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    results = []
    for cuts in ([1] * 8, [8], [3, 3, 2]):
        vol = _volume(device)
        lo = 0
        for n in cuts:
            vol.integrate(depth[lo:lo + n], rgb[lo:lo + n], w2c[lo:lo + n], intr, frames_per_launch=n)
            lo += n
        results.append(vol)
    torch.cuda.synchronize()
    assert float(results[0].weight.max()) >= 3.0
    for other in results[1:]:
        for name in ("tsdf", "weight", "color"):
            assert torch.equal(getattr(results[0], name), getattr(other, name)), f"{name} depends on the cut into launches"


def _check_noop(device):
    depth, rgb, w2c, _, intr = (t.to(device) if torch.is_tensor(t) else t for t in _scene())
    vol = _volume(device)
    vol.integrate(depth[:2], rgb[:2], w2c[:2], intr)
    before = [t.clone() for t in (vol.tsdf, vol.weight, vol.color)]
    assert float(before[1].sum()) > 1000
    away = torch.eye(4, device=device)  # camera above the volume, looking up along +z: every voxel is behind it
    away[2, 3] = -2.0                   # world -> camera: zc = z - 2
    frames = [
        (torch.zeros_like(depth[2]), w2c[2]),
        (depth[3], away),
        (torch.full_like(depth[4], float("nan")), w2c[4]),
        (torch.full_like(depth[5], float("inf")), w2c[5]),
        (torch.full_like(depth[6], DEPTH_MAX * 1.2), w2c[6]),
    ]
    d = torch.stack([f[0] for f in frames])
    m = torch.stack([f[1] for f in frames])
    vol.integrate(d, rgb[2:7], m, intr)                       # one launch
    vol.integrate(d, rgb[2:7], m, intr, frames_per_launch=1)  # and one launch each
    torch.cuda.synchronize()
    for b, a, name in zip(before, (vol.tsdf, vol.weight, vol.color), ("tsdf", "weight", "color")):
        assert bool(torch.isfinite(a).all()), f"{name} is not finite"
        assert torch.equal(a, b), f"{name} changed"


def test_matches_float64_oracle(device):
    _run("oracle", _check_oracle, device)


def test_result_does_not_depend_on_batching(device):
    _run("batching", _check_batching, device)


def test_frames_that_must_do_nothing(device):
    _run("noop", _check_noop, device)


def test_large_index(device):
    """1024 x 1024 x 768 voxels (8.05e8, 16 GB for the five planes): the voxels the camera sees have linear indices near
    8e8, so their third colour value lies beyond 2^31 elements and every byte offset beyond 2^32.

    The volume is placed with its HIGH corner at the world origin, so that the camera and the voxels it sees have
    coordinates below 1 m like those of the small tests and the same bounds apply.  With the low corner at the origin
    instead (coordinates and translation around 16 - 28 m) the float32 evaluation of R p + t the rule prescribes rounds zc
    to some 1e-6 m, and 45 of 32725 tsdf values missed the 2e-5 bound by up to 2.35e-5 (weights equal): the precision of
    the number format at that distance, not an index error."""
    for name, body in (("oracle", _check_oracle), ("batching", _check_batching), ("noop", _check_noop)):
        _run(name, body, device)
    if torch.cuda.mem_get_info()[0] < 24e9:
        pytest.skip("less than 24 GB of device memory free")
    dims = (1024, 1024, 768)
    lower = tuple(-(d - 1) * VOXEL for d in dims)
    corner = np.zeros(3)
    # camera 0.4 m inside the high corner on each axis, looking along the diagonal at it; depth 0.5 m everywhere
    fwd = np.ones(3) / np.sqrt(3.0)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, corner - 0.4
    w2c = torch.from_numpy(np.linalg.inv(c2w)).float()[None]
    H, W = 72, 96
    from nerf_vo_amd.synthetic import replica_intrinsics

    intr = replica_intrinsics(H, W)
    depth = torch.full((1, H, W), 0.5)
    g = torch.Generator().manual_seed(5)
    rgb = torch.randint(0, 256, (1, H, W, 3), generator=g).to(torch.uint8)

    vol = _volume(device, lower, dims, max_voxels=2 ** 30)
    vol.integrate(depth.to(device), rgb.to(device), w2c.to(device), intr)
    torch.cuda.synchronize()
    # everything the frame can touch lies within 0.5 + trunc of z-depth and the image's half widths of the camera:
    # less than 1 m from it, so inside the last 96 voxels (1.5 m) of every axis
    box = tuple(slice(d - 96, d) for d in dims)
    total = float(vol.weight.sum(dtype=torch.float64))
    assert total == float(vol.weight[box].sum(dtype=torch.float64)) and total > 1000
    assert int(torch.count_nonzero(vol.tsdf)) == int(torch.count_nonzero(vol.tsdf[box]))
    for ch in range(3):
        assert int(torch.count_nonzero(vol.color[ch])) == int(torch.count_nonzero(vol.color[ch][box]))
    rng = tuple((d - 32, d) for d in dims)
    ref = fuse(lower, VOXEL, TRUNC_VOXELS * VOXEL, DEPTH_MAX, rng, frame_table(w2c.numpy(), intr), depth.numpy(), rgb.numpy())
    sub = tuple(slice(a, b) for a, b in rng)
    _compare((vol.tsdf[sub], vol.weight[sub], vol.color[(slice(None),) + sub]), ref, "high corner of the large volume")


class _RoomNerf:
    """What a perfect model would render, through the renderer interface: the analytic room at the dataset's own poses."""

    def __init__(self, dataset, keyframes):
        self.dataset, self.keyframes = dataset, keyframes

    def get_camera_extrinsics(self, frame_index):
        return np.array(self.dataset.camera_extrinsics[self.keyframes[frame_index]])

    def render_frame(self, camera_intrinsics, camera_extrinsics):
        return self.dataset.render(camera_extrinsics)

    def render_frame_depth_from_training_frame(self, camera_intrinsics, frame_index):
        return self.render_frame(camera_intrinsics, self.get_camera_extrinsics(frame_index))[1]


def test_render_mesh_end_to_end(device, tmp_path):
    """render_frames() then render_mesh() on the analytic room [-0.5, 0.5]^3.  Every frame is made an evaluation frame:
    with the dataset's default stride the five views lie 72 degrees apart and no surface point is seen three times (in the
    float64 fusion of those five no voxel behind a wall reaches weight 3), so the weight threshold of 3 leaves no surface.
    The zero crossings of the float64 fusion of the 24 frames lie within 0.85 voxel of the walls (CPU, oracle alone)."""
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=72, width=96, scene_scale=0.25)
    ds.evaluation_frames = list(range(ds.num_frames))
    keyframes = list(range(0, 24, 4))
    renderer = EvaluationRenderer(dataset=ds, nerf=_RoomNerf(ds, keyframes), keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    renderer.render_frames()
    renderer.render_mesh()
    path = tmp_path / "pred" / "mesh" / "mesh_from_evaluation_frames.ply"
    assert os.path.exists(path)
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    n_vert = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_face = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    assert [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l] == \
        ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(body) == n_vert * 27 + n_face * 13
    rec = np.frombuffer(body[: n_vert * 27], dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    faces = np.frombuffer(body[n_vert * 27:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert n_vert >= 1000 and n_face > 0 and faces["i"].min() >= 0 and faces["i"].max() < n_vert
    v, nrm = rec["p"].astype(np.float64), rec["n"].astype(np.float64)
    to_wall = np.abs(np.abs(v) - 0.5).min(axis=1) / VOXEL
    inward = float(((nrm * -v).sum(axis=1) > 0).mean())
    print(f"{n_vert} vertices, {n_face} faces, farthest vertex {to_wall.max():.3f} voxel from a wall, normals inward {inward:.4f}")
    assert to_wall.max() <= 1.0
    assert inward >= 0.99
    assert rec["c"].std(axis=0).min() > 1.0, "vertex colours are constant"
    with pytest.raises(NotImplementedError, match="compute_and_save_marching_cubes_mesh"):
        renderer.render_mesh(source="nerf")
