"""Inputs and runs of tests/test_tsdf_bits_gpu.py: the TSDF fusion kernels (csrc/tsdf.hip, tsdf_blocks.hip) and the
edge-owned extractors (csrc/iso.hip, iso_blocks.hip) on the room scene of helpers/tsdf_oracle.py, every output tensor
reduced to a sha256 that tests/golden/tsdf_bits.json records (tests/golden/make_golden_tsdf_bits.py).

Scene: ``room_scene()`` (8 frames of 72 x 96), voxel 1/64, truncation 8 voxels, depth_max 5, lower (-0.5625, -0.5625,
-0.42): the inputs of test_tsdf_gpu.py and test_tsdf_blocks_gpu.py.  The scene is rendered on the CPU and its last bits
depend on the CPU's vector units, so the frames the record was made with are kept next to it
(tests/golden/tsdf_bits_inputs.npz, written by make_golden_tsdf_bits.py from ``scene_inputs()``) and the test reads those.

  dense/8      72 x 67 x 53, the eight frames in one launch: no dimension is a multiple of the 2 x 4 x 32 brick
  dense/16     the same box, the eight frames twice in a row in ONE launch of 16: the brick cull runs a second batch of
               eight and sets bits 8..15 of the live mask
  blocks       table 9 x 9 x 7, blocks='touched', one launch: to_dense(), extract_mesh(3.0), extract_mesh(1.0)
  iso/default  extract_isosurface on the blocks case's to_dense(), (weight >= 3) & allocated, default points_per_workgroup
  iso/1000     the same with points_per_workgroup = 1000: the same digests as iso/default

Importing this module needs no GPU; ``run`` does."""
import hashlib
import json
import os

import numpy as np
import torch

from helpers.tsdf_oracle import room_scene

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
RECORD_PATH = os.path.join(GOLDEN, "tsdf_bits.json")
INPUTS_PATH = os.path.join(GOLDEN, "tsdf_bits_inputs.npz")

VOXEL = 1.0 / 64.0
TRUNC_VOXELS = 8.0
DEPTH_MAX = 5.0
LOWER = (-0.5625, -0.5625, -0.42)
DENSE_DIMS = (72, 67, 53)
TABLE = (9, 9, 7)
BLOCK_DIMS = tuple(8 * t for t in TABLE)
CASES = ("dense/8", "dense/16", "blocks", "iso/default", "iso/1000")


def digest(t):
    """sha256 over a tensor's dtype, shape and contiguous bytes: NaN payloads and the sign of zero count"""
    t = t.detach().cpu().contiguous()
    h = hashlib.sha256(f"{t.dtype}:{tuple(t.shape)};".encode())
    h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def upper(dims, lower=LOWER):
    return tuple(l + (d - 1) * VOXEL for l, d in zip(lower, dims))


def scene_inputs():
    """the scene as the kernels receive it: depth, rgb, world_to_camera float32, camera_to_world float32, intrinsics"""
    depth, rgb, w2c, c2w, intr = room_scene()
    return {"depth": depth, "rgb": rgb, "w2c": w2c, "c2w": c2w.float(), "intr": torch.tensor(intr, dtype=torch.float64)}


def save_inputs(inp, path):
    np.savez_compressed(path, **{name: t.numpy() for name, t in inp.items()})


def inputs(path=INPUTS_PATH):
    """the recorded frames of ``scene_inputs()``"""
    with np.load(path) as z:
        return {name: torch.from_numpy(z[name]) for name in z.files}


def inputs_digest(inp):
    h = hashlib.sha256()
    for name in sorted(inp):
        h.update(f"{name}:{digest(inp[name])};".encode())
    return h.hexdigest()


def load_record():
    with open(RECORD_PATH) as fh:
        return json.load(fh)


def run(inp, device):
    """every case once -> {case: {tensor name: tensor}}"""
    from nerf_vo_amd.meshing import extract_isosurface
    from nerf_vo_amd.tsdf import TSDFBlockVolume, TSDFVolume

    depth, rgb, w2c, c2w = (inp[k].to(device) for k in ("depth", "rgb", "w2c", "c2w"))
    intr = tuple(float(x) for x in inp["intr"])
    out = {}
    for reps in (1, 2):
        vol = TSDFVolume(LOWER, upper(DENSE_DIMS), VOXEL, TRUNC_VOXELS, DEPTH_MAX, device=device)
        assert vol.dims == DENSE_DIMS
        vol.integrate(depth.repeat(reps, 1, 1), rgb.repeat(reps, 1, 1, 1), w2c.repeat(reps, 1, 1), intr, frames_per_launch=8 * reps)
        out[f"dense/{8 * reps}"] = {"tsdf": vol.tsdf, "weight": vol.weight, "color": vol.color}
    blocks = TSDFBlockVolume(LOWER, upper(BLOCK_DIMS), VOXEL, TRUNC_VOXELS, DEPTH_MAX, device=device)
    assert blocks.table_dims == TABLE
    blocks.integrate(depth, rgb, w2c, intr, camera_to_world=c2w, frames_per_launch=8)
    tsdf, weight, color, allocated = blocks.to_dense()
    out["blocks"] = {"tsdf": tsdf, "weight": weight, "color": color, "allocated": allocated}
    for threshold in (3.0, 1.0):
        mesh = blocks.extract_mesh(threshold)
        out["blocks"].update({f"mesh{threshold:g}/{name}": t for name, t in zip(("vertices", "faces", "colors", "normals"), mesh)})
    valid = (weight >= 3.0) & allocated
    for name, ppw in (("default", None), ("1000", 1000)):
        v, f = extract_isosurface(-tsdf, blocks.lower, blocks.upper_of_grid, 0.0, valid, points_per_workgroup=ppw)
        out[f"iso/{name}"] = {"vertices": v, "faces": f}
    torch.cuda.synchronize(device)
    return out
