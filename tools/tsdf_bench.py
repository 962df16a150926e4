#!/usr/bin/env python3
"""TSDF fusion throughput (nerf_vo_amd/tsdf.py, csrc/tsdf.hip): ms per frame of ``TSDFVolume.integrate`` for Replica-sized
frames (1200 x 680) into a 512 x 512 x 192 volume (8 x 8 x 3 m at 1/64), for frames_per_launch in {1, 4, 8, 16}.

Scene: the analytic room [-2, 2]^3 seen from 16 orbit cameras; the volume cuts the room at z = +-1.5, so a part of every
frustum is empty space outside the volume and a part of the volume is outside every frustum.  Timed with HIP events
around the whole ``integrate`` call of the 16 frames, warm-up first, median of ``--repeats`` runs on a zeroed volume.
"volume GB/s" is the traffic of the bricks (2 x 4 x 32 voxels) a launch wrote to -- five float planes read and written
once per launch -- summed over the launches and divided by the time; frame reads are not counted.

    python tools/tsdf_bench.py            # one JSON line per setting, then a markdown table

``--volume blocks``: the same frames and box into a ``TSDFBlockVolume`` (csrc/tsdf_blocks.hip, iso_blocks.hip), see
``run_blocks``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

BRICK = (2, 4, 32)


def _touched_bricks(before: torch.Tensor, after: torch.Tensor) -> int:
    nx, ny, nz = after.shape
    changed = (after != before).view(nx // BRICK[0], BRICK[0], ny // BRICK[1], BRICK[1], nz // BRICK[2], BRICK[2])
    return int(changed.any(dim=5).any(dim=3).any(dim=1).sum())


def run(frames=16, height=680, width=1200, dims=(512, 512, 192), repeats=5, settings=(1, 4, 8, 16), device="cuda:0"):
    entry.build()
    from nerf_vo_amd.synthetic import orbit_poses_opencv, render_room, replica_intrinsics
    from nerf_vo_amd.tsdf import TSDFVolume

    dev = torch.device(device)
    voxel = 1.0 / 64.0
    intr = replica_intrinsics(height, width)
    c2w = orbit_poses_opencv(frames, device=dev)
    color, depth, _ = render_room(c2w, height, width, intr, half_extent=2.0)
    rgb = (color.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()
    depth = depth[:, 0].clamp(0.0, 5.0).contiguous()
    w2c = torch.linalg.inv(c2w.double()).float()
    lower = [-d * voxel / 2 for d in dims]
    upper = [l + (d - 1) * voxel for l, d in zip(lower, dims)]
    vol = TSDFVolume(lower, upper, voxel, device=dev)
    assert vol.dims == tuple(dims) and all(d % b == 0 for d, b in zip(dims, BRICK))
    rows = []
    for fpl in settings:
        # traffic model: bricks written per launch (outside the timing)
        for t in (vol.tsdf, vol.weight, vol.color):
            t.zero_()
        bricks = 0
        for lo in range(0, frames, fpl):
            before = vol.weight.clone()
            vol.integrate(depth[lo:lo + fpl], rgb[lo:lo + fpl], w2c[lo:lo + fpl], intr, frames_per_launch=fpl)
            bricks += _touched_bricks(before, vol.weight)
        del before
        volume_bytes = bricks * BRICK[0] * BRICK[1] * BRICK[2] * 5 * 4 * 2
        times = []
        for r in range(repeats + 1):  # the first run is the warm-up
            for t in (vol.tsdf, vol.weight, vol.color):
                t.zero_()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            vol.integrate(depth, rgb, w2c, intr, frames_per_launch=fpl)
            stop.record()
            torch.cuda.synchronize()
            if r > 0:
                times.append(start.elapsed_time(stop))
        ms = statistics.median(times)
        row = {"frames_per_launch": fpl, "frames": frames, "resolution": [width, height], "volume": list(dims),
               "ms_per_frame": ms / frames, "ms_min": min(times) / frames, "ms_max": max(times) / frames,
               "bricks_written_per_pass": bricks, "volume_GB_per_s": volume_bytes / (ms * 1e-3) / 1e9,
               "observed_voxels": int((vol.weight > 0).sum())}
        print(json.dumps(row), flush=True)
        rows.append(row)
    print("\n| frames per launch | ms / frame (median, min..max) | bricks written per pass | volume GB/s |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['frames_per_launch']} | {r['ms_per_frame']:.3f} ({r['ms_min']:.3f}..{r['ms_max']:.3f}) | "
              f"{r['bricks_written_per_pass']} | {r['volume_GB_per_s']:.0f} |")
    return rows


def _median_ms(body, repeats, setup=None):
    """median, min, max of HIP-event times around ``body(setup())``; the first run is the warm-up"""
    times = []
    for r in range(repeats + 1):
        state = setup() if setup is not None else None
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        body(state)
        stop.record()
        torch.cuda.synchronize()
        if r > 0:
            times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def run_blocks(frames=16, height=680, width=1200, dims=(512, 512, 192), repeats=5, settings=(1, 4, 8, 16), device="cuda:0"):
    """The same scene and box into a ``TSDFBlockVolume`` (csrc/tsdf_blocks.hip): ms per frame of the whole ``integrate`` call
    (touch pass, allocation of the new blocks by torch, fusion) on a fresh volume, of ``allocate`` alone (touch pass and
    allocation, 16 frames per launch), the extraction, the blocks allocated against those that hold an in-band voxel, and
    the bytes."""
    entry.build()
    from nerf_vo_amd.synthetic import orbit_poses_opencv, render_room, replica_intrinsics
    from nerf_vo_amd.tsdf import BLOCK_VOXELS, TSDFBlockVolume

    dev = torch.device(device)
    voxel = 1.0 / 64.0
    intr = replica_intrinsics(height, width)
    c2w = orbit_poses_opencv(frames, device=dev)
    color, depth, _ = render_room(c2w, height, width, intr, half_extent=2.0)
    rgb = (color.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()
    depth = depth[:, 0].clamp(0.0, 5.0).contiguous()
    w2c = torch.linalg.inv(c2w.double()).float()
    c2w = c2w.float()
    lower = [-d * voxel / 2 for d in dims]
    upper = [l + (d - 1) * voxel for l, d in zip(lower, dims)]

    def fresh():
        vol = TSDFBlockVolume(lower, upper, voxel, device=dev)
        vol._reserve(vol.block_count)  # the pool's first allocation (1 GB of zeros) is not what a frame costs
        return vol

    rows, vol = [], None
    # touch pass and allocation alone: ``allocate`` marks the frames in launches of 16
    touch = _median_ms(lambda v: v.allocate(depth, c2w, intr), repeats, fresh)
    print(json.dumps({"volume": "blocks", "allocate_ms_per_frame": touch[0] / frames, "ms_min": touch[1] / frames,
                      "ms_max": touch[2] / frames}), flush=True)
    for fpl in settings:
        ms = _median_ms(lambda v: v.integrate(depth, rgb, w2c, intr, camera_to_world=c2w, frames_per_launch=fpl), repeats, fresh)
        vol = fresh()
        vol.integrate(depth, rgb, w2c, intr, camera_to_world=c2w, frames_per_launch=fpl)
        n = vol.n_blocks
        in_band = ((vol.weight[:n] > 0) & (vol.tsdf[:n] < 1.0)).any(dim=1)
        row = {"volume": "blocks", "frames_per_launch": fpl, "frames": frames, "resolution": [width, height], "lattice": list(vol.dims),
               "ms_per_frame": ms[0] / frames, "ms_min": ms[1] / frames, "ms_max": ms[2] / frames,
               "blocks_allocated": n, "blocks_with_in_band_voxels": int(in_band.sum()),
               "table_entries": vol.table.numel(), "observed_voxels": int((vol.weight[:n] > 0).sum()),
               "pool_bytes_in_use": n * BLOCK_VOXELS * 5 * 4, "pool_bytes_reserved": vol.capacity * BLOCK_VOXELS * 5 * 4,
               "table_and_marks_bytes": 2 * 4 * vol.table.numel(), "dense_bytes": dims[0] * dims[1] * dims[2] * 5 * 4}
        print(json.dumps(row), flush=True)
        rows.append(row)
    mesh = vol.extract_mesh()
    ex = _median_ms(lambda _: vol.extract_mesh(), repeats)
    from nerf_vo_amd.tsdf import vertex_normals

    nrm = _median_ms(lambda _: vertex_normals(mesh[0], mesh[1]), repeats)
    print(json.dumps({"volume": "blocks", "extract_mesh_ms": ex[0], "ms_min": ex[1], "ms_max": ex[2], "of_which_vertex_normals_ms": nrm[0],
                      "vertices": mesh[0].shape[0], "faces": mesh[1].shape[0]}), flush=True)
    print("\n| frames per launch | ms / frame (median, min..max) | blocks allocated / with in-band voxels |")
    print("|---|---|---|")
    for r in rows:
        print(f"| {r['frames_per_launch']} | {r['ms_per_frame']:.3f} ({r['ms_min']:.3f}..{r['ms_max']:.3f}) | "
              f"{r['blocks_allocated']} / {r['blocks_with_in_band_voxels']} |")
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume", default="dense", choices=["dense", "blocks"], help="dense: TSDFVolume; blocks: TSDFBlockVolume")
    a = ap.parse_args()
    (run if a.volume == "dense" else run_blocks)(frames=a.frames, height=a.height, width=a.width, repeats=a.repeats)
