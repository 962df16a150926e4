#!/usr/bin/env python3
"""Iso-surface extraction: the HIP extractor (meshing.extract_isosurface, csrc/iso.hip) beside the torch extractor
(meshing.marching_tetrahedra), and the density mesh of the occupancy-grid back-end end to end.

(a) ``--tsdf``: the volume tools/tsdf_bench.py fuses (512 x 512 x 192 at 1/64, 16 frames of 1200 x 680), extracted as
    ``TSDFVolume.extract_mesh`` does: field -tsdf, threshold 0, valid = weight >= 3.  V and F of both extractors are
    recorded: a larger V of the torch extractor is its count of unmerged duplicate vertices.
(b) ``--field``: an instant-ngp field trained on the synthetic room (``--keyframes`` of 136 x 240, ``--iterations`` steps),
    sampled on a ``--lattice`` (default 512 x 384 x 192, the reference's 1/64 m over a room) spanning the room's box:
    ``NgpEngine.density_lattice`` + ``extract_isosurface`` against the path ``compute_and_save_marching_cubes_mesh`` took
    before (an [n, 3] position grid through ``density_at``, then ``marching_tetrahedra``), restated here.

One warm-up, then the median (min..max) of ``--repeats`` runs.  Whole calls: host clock around a synchronise.  The two
kernels of the HIP extractor: HIP events around each launch.

    python tools/iso_bench.py --tsdf --field     # one JSON line per measurement
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def _timed(fn, repeats):
    """host clock around a synchronise: (median, min, max) in ms and the last result"""
    times, out = [], None
    for r in range(repeats + 1):  # the first run is the warm-up
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r > 0:
            times.append(1e3 * (time.perf_counter() - t0))
    return {"ms": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}, out


def _kernel_times(values, valid, lower, upper, threshold, repeats):
    """HIP events around nvo_iso_count and nvo_iso_emit (the wrapper's steps, restated so that events fit in between)"""
    from nerf_vo_amd import _lib

    lib, dev = _lib.lib(), values.device
    nx, ny, nz = values.shape
    ppw = _lib.ISO_DEFAULT_POINTS_PER_WORKGROUP
    lo, hi = np.asarray(lower, np.float32), np.asarray(upper, np.float32)
    step = (hi - lo) / np.asarray([nx - 1, ny - 1, nz - 1], np.float32)
    groups = int(lib.nvo_iso_workgroups(nx, ny, nz, ppw))
    scratch = torch.empty(int(lib.nvo_iso_scratch_bytes(nx, ny, nz, ppw)), dtype=torch.uint8, device=dev)
    args = _lib.IsoArgs(values=values.data_ptr(), valid=None if valid is None else valid.data_ptr(), scratch=scratch.data_ptr(),
                        nx=nx, ny=ny, nz=nz, points_per_workgroup=ppw, threshold=float(threshold),
                        lower=(C.c_float * 3)(*lo.tolist()), step=(C.c_float * 3)(*step.tolist()))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    count_ms, emit_ms = [], []
    for r in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.check(lib.nvo_iso_count(stream, C.byref(args)), "iso_count")
        ev[1].record()
        totals = scratch[:16 * groups].view(torch.int64).view(2, groups)
        ends = torch.cumsum(totals, dim=1)
        bases = (ends - totals).contiguous()
        n_vert, n_face = (int(x) for x in ends[:, -1].tolist())
        vertices = torch.empty(n_vert, 3, device=dev)
        faces = torch.empty(n_face, 3, dtype=torch.int32, device=dev)
        args.vertex_base, args.face_base = bases[0].data_ptr(), bases[1].data_ptr()
        args.vertices, args.faces, args.n_vertices, args.n_faces = vertices.data_ptr(), faces.data_ptr(), n_vert, n_face
        ev[2].record()
        _lib.check(lib.nvo_iso_emit(stream, C.byref(args)), "iso_emit")
        ev[3].record()
        torch.cuda.synchronize()
        if r > 0:
            count_ms.append(ev[0].elapsed_time(ev[1]))
            emit_ms.append(ev[2].elapsed_time(ev[3]))
    return {"count_ms": statistics.median(count_ms), "count_ms_min": min(count_ms), "count_ms_max": max(count_ms),
            "emit_ms": statistics.median(emit_ms), "emit_ms_min": min(emit_ms), "emit_ms_max": max(emit_ms),
            "scratch_bytes": scratch.numel()}


def _compare(name, values, valid, lower, upper, threshold, repeats, torch_repeats):
    from nerf_vo_amd.meshing import extract_isosurface, marching_tetrahedra

    hip, (v, f) = _timed(lambda: extract_isosurface(values, lower, upper, threshold, valid=valid), repeats)
    row = {"measurement": name, "lattice": list(values.shape), "hip": {**hip, "V": v.shape[0], "F": f.shape[0]},
           "hip_kernels": _kernel_times(values, None if valid is None else valid.to(torch.uint8), lower, upper, threshold, repeats)}
    del v, f
    if torch_repeats > 0:
        ref, (tv, tf) = _timed(lambda: marching_tetrahedra(values, lower, upper, threshold, valid=valid), torch_repeats)
        row["torch"] = {**ref, "V": tv.shape[0], "F": tf.shape[0]}
        row["torch_unmerged_duplicates"] = tv.shape[0] - row["hip"]["V"]
    print(json.dumps(row), flush=True)
    return row


def run_tsdf(repeats=5, torch_repeats=5, device="cuda:0", frames=16, height=680, width=1200, dims=(512, 512, 192)):
    from nerf_vo_amd.synthetic import orbit_poses_opencv, render_room, replica_intrinsics
    from nerf_vo_amd.tsdf import FRAMES_PER_LAUNCH, WEIGHT_THRESHOLD, TSDFVolume

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
    vol.integrate(depth, rgb, w2c, intr, frames_per_launch=FRAMES_PER_LAUNCH)
    del color, depth, rgb
    values, valid = -vol.tsdf, vol.weight >= WEIGHT_THRESHOLD
    return _compare("tsdf_volume", values, valid, vol.lower, vol.upper_of_grid, 0.0, repeats, torch_repeats)


def _previous_density_mesh(eng, lo, hi, res, thresh):
    """what compute_and_save_marching_cubes_mesh did before density_lattice / extract_isosurface (nerf_scale 1, offset 0)"""
    from nerf_vo_amd.meshing import marching_tetrahedra

    axes = [torch.linspace(float(lo[k]), float(hi[k]), res[k], device=eng.device) for k in range(3)]
    gx, gy, gz = torch.meshgrid(*axes, indexing="ij")
    world = torch.stack([gx, gy, gz], dim=-1).reshape(-1, 3)
    dens = eng.density_at(world).view(*res)
    return marching_tetrahedra(dens, lo, hi, float(thresh))


def run_field(repeats=5, torch_repeats=1, device="cuda:0", keyframes=24, iterations=1000, lattice=(512, 384, 192), thresh=2.5):
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGP
    from nerf_vo_amd.meshing import extract_isosurface
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    dev = torch.device(device)
    H, W, scale = 136, 240, 0.5
    ds = SyntheticEvaluationDataset(num_frames=keyframes, height=H, width=W, device=dev, scene_scale=scale)
    import tempfile
    with tempfile.TemporaryDirectory(prefix="nvo_iso_") as tmp:
        args = argparse.Namespace(num_keyframes=keyframes, frame_height=H, frame_width=W, mapping_iterations=iterations,
                                  mapping_snapshot_iterations=iterations, dir_prediction=tmp)
        mapper = InstantNGP(args, device=dev)
        frames = [ds.render(p) for p in ds.camera_extrinsics]
        color = torch.stack([torch.from_numpy(c) for c, _ in frames]).permute(0, 3, 1, 2).float() / 255.0
        depth = torch.stack([torch.from_numpy(d) for _, d in frames])[:, None].float().clamp(0.0, 5.0)
        ci = ds.camera_intrinsics
        intr = torch.tensor([ci["fx"], ci["fy"], ci["cx"], ci["cy"]])
        poses = torch.from_numpy(ds.camera_extrinsics).float()
        mapper(input={"keyframe_indices": torch.arange(keyframes), "camera_intrinsics": intr.repeat(keyframes, 1).to(dev),
                      "camera_extrinsics": opencv_to_opengl(poses.to(dev)), "frames_color": color.to(dev),
                      "frames_depth": depth.to(dev), "last_frame": True})
        while mapper.step < iterations:
            mapper(input=None)
        mapper(input=None)
    eng = mapper.ngp._engine
    half = 2.0 * scale * 1.05
    lo, hi, res = np.full(3, -half), np.full(3, half), [int(r) for r in lattice]
    sample, dens = _timed(lambda: eng.density_lattice(lo, hi, res), repeats)
    ext, (v, f) = _timed(lambda: extract_isosurface(dens, lo, hi, thresh), repeats)
    row = {"measurement": "density_mesh", "lattice": res, "samples": int(np.prod(res)), "keyframes": keyframes, "iterations": iterations,
           "density_lattice": sample, "extract_isosurface": {**ext, "V": v.shape[0], "F": f.shape[0]},
           "hip_kernels": _kernel_times(dens, None, lo, hi, thresh, repeats)}
    del dens, v, f
    if torch_repeats > 0:
        prev, (tv, tf) = _timed(lambda: _previous_density_mesh(eng, lo, hi, res, thresh), torch_repeats)
        row["previous_path"] = {**prev, "V": tv.shape[0], "F": tf.shape[0]}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tsdf", action="store_true", help="(a) extraction of the fused 512 x 512 x 192 volume")
    ap.add_argument("--field", action="store_true", help="(b) density_lattice + extraction on a trained instant-ngp field")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-repeats", type=int, default=None, help="runs of the torch path (0: skip it)")
    ap.add_argument("--keyframes", type=int, default=24)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--lattice", type=int, nargs=3, default=(512, 384, 192))
    a = ap.parse_args()
    entry.build()
    tr = a.repeats if a.torch_repeats is None else a.torch_repeats
    if a.tsdf or not a.field:
        run_tsdf(repeats=a.repeats, torch_repeats=tr)
    if a.field:
        run_field(repeats=a.repeats, torch_repeats=tr, keyframes=a.keyframes, iterations=a.iterations, lattice=a.lattice)
