#!/usr/bin/env python3
"""Times of the occupancy-grid back-end's normals path on the state tools/ngp_bench.py trains (192 keyframes of 360 x 640
of the synthetic room through the pyngp facade): a 1200 x 680 frame with and without normals, the vertex attributes of a
density mesh, points per second of the oriented cloud.  Device time between HIP events around each piece (host copies of
the images included, as tools/ngp_bench.py's frame time has them); the colour-only frame of the same build is printed
beside the others, with its run-to-run spread.  There is no threshold: new ground.
python tools/ngp_normals_bench.py [--steps 600] [--frames 5] [--keyframes 192 --height 360 --width 640]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

entry.build()
from nerf_vo_amd import _lib, pyngp  # noqa: E402
from nerf_vo_amd.mapping.dataset import opencv_to_opengl  # noqa: E402
from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGPRenderer  # noqa: E402
from nerf_vo_amd.synthetic import make_sequence  # noqa: E402


def timed(fn):
    """(result, milliseconds between two events on the current stream around fn)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=192)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--mesh-resolution", type=int, default=128)
    ap.add_argument("--cloud-points", type=int, default=1 << 20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    seq = make_sequence(a.keyframes, H, W, device=dev, scene_scale=0.2)
    poses = seq["camera_extrinsics"].clone()
    poses[:, :3, 3] += 0.5
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf, 0)
    tb.create_empty_nerf_dataset(n_images=a.keyframes, nerf_scale=1.0, nerf_offset=np.zeros(3), aabb_scale=4)
    tb.reload_network_from_file("")
    tb.shall_train = True
    tb.nerf.training.optimize_extrinsics = True
    color = seq["frames_color"].permute(0, 2, 3, 1)
    color = torch.cat([color, torch.ones_like(color[..., :1])], dim=3)
    depth = seq["frames_depth"].permute(0, 2, 3, 1)
    tb.nerf.training.update_training_images(
        frame_ids=list(range(a.keyframes)), poses=opencv_to_opengl(poses)[:, :3], images=color.contiguous(),
        depths=depth.contiguous(), depths_cov=torch.ones_like(depth), resolution=np.array([W, H]),
        principal_point=seq["camera_intrinsics"][0, 2:].cpu().numpy(), focal_length=seq["camera_intrinsics"][0, :2].cpu().numpy())
    for _ in range(a.steps):
        tb.frame()
    torch.cuda.synchronize()
    eng = tb._engine
    fx = float(seq["camera_intrinsics"][0, 0]) * 1200.0 / W
    tb.fov_axis, tb.fov, tb.exposure = 0, 2.0 * math.degrees(math.atan(0.5 * 1200.0 / fx)), 0.0
    tb.nerf.render_min_transmittance = 1e-4

    def set_view(f):
        m = poses[f % a.keyframes].detach().cpu().numpy().astype(np.float64).copy()
        m[0:3, 1:3] *= -1
        tb.set_nerf_camera_matrix(m[[2, 0, 1]])

    def colour_frame():
        tb.render_mode = pyngp.Shade
        tb.render(width=1200, height=680, spp=1, linear=True)
        tb.render_mode = pyngp.Depth
        return tb.render(width=1200, height=680, spp=1, linear=True)

    def normals_frame():
        tb.render_mode = pyngp.Normals
        tb.render(width=1200, height=680, spp=1, linear=True)
        tb.render_mode = pyngp.Shade
        tb.render(width=1200, height=680, spp=1, linear=True)
        tb.render_mode = pyngp.Depth
        return tb.render(width=1200, height=680, spp=1, linear=True)

    res = {"steps": eng.step, "resolution": [1200, 680]}
    for name, fn, first in (("colour_and_depth", colour_frame, 0), ("normals_colour_and_depth", normals_frame, 100),
                            ("colour_and_depth_again", colour_frame, 200)):
        times = []
        for f in range(a.frames + 1):
            set_view(first + f)
            times.append(timed(fn)[1])
        t = times[1:]  # (the first frame of a kind sizes its bundles and allocates)
        res[name] = {"ms_per_frame_mean": round(float(np.mean(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
        print(f"1200x680 {name}: {np.mean(t):.2f} ms per frame (min {min(t):.2f}, max {max(t):.2f}, {len(t)} frames)")
    extra = res["normals_colour_and_depth"]["ms_per_frame_mean"] - res["colour_and_depth"]["ms_per_frame_mean"]
    res["normals_extra_ms"] = round(extra, 3)
    # per-kernel device time of one frame with normals: what the generic chain (seed, fused-MLP backward, streamed grid
    # input backward) and the compositing take of it
    lib = _lib.lib()
    lib.nvo_profile_enable(1)
    set_view(300)
    normals_frame()
    torch.cuda.synchronize()
    need = lib.nvo_profile_summary(None, 0)
    buf = C.create_string_buffer(int(need) + 16)
    lib.nvo_profile_summary(buf, len(buf))
    lib.nvo_profile_enable(0)
    rows = []
    for line in buf.value.decode().strip().splitlines():
        name, cnt, total = line.rsplit(",", 2)
        rows.append((name, int(cnt), float(total)))  # (milliseconds)
    tot = sum(r[2] for r in rows)
    chain = sum(r[2] for r in rows if r[0].startswith(("mlp_bwd", "grid_bwd_input", "ngp_normal_seed")))
    comp = sum(r[2] for r in rows if r[0].startswith("ngp_composite_normals"))
    res["kernel_ms_per_normals_frame"] = {"all": round(tot, 3), "chain_seed_mlp_bwd_grid_input_bwd": round(chain, 3),
                                          "composite_normals": round(comp, 3), "chain_share": round(chain / tot, 3)}
    print(f"kernel time of a frame with normals {tot:.2f} ms: chain {chain:.2f} ms ({100 * chain / tot:.1f} %), "
          f"compositing of the normals {comp:.3f} ms")
    for name, cnt, total in sorted(rows, key=lambda r: -r[2])[:12]:
        print(f"  {name:34s} launches {cnt:4d}  {total:8.3f} ms")

    # vertex attributes of a density mesh over the room
    from nerf_vo_amd.meshing import extract_isosurface

    lo, hi = np.full(3, 0.5 - 0.45), np.full(3, 0.5 + 0.45)
    dens = eng.density_lattice(lo, hi, [a.mesh_resolution] * 3)
    verts, _ = extract_isosurface(dens, lo, hi, 2.5)

    def attributes():
        _, g = eng.density_gradient_at(verts)
        n = -g / (torch.linalg.norm(g, dim=1, keepdim=True) + 1e-10)
        return eng.color_at(verts, -n)

    attributes()
    _, ms = timed(attributes)
    res["mesh_vertex_attributes"] = {"vertices": int(verts.shape[0]), "ms": round(ms, 3),
                                     "vertices_per_sec": round(verts.shape[0] / ms * 1e3)}
    print(f"vertex attributes of {verts.shape[0]} vertices: {ms:.2f} ms")

    nerf = InstantNGPRenderer.__new__(InstantNGPRenderer)
    nerf.ngp = tb
    box = (lo, hi)  # (nerf_scale 1, nerf_offset 0: the dataset's frame is the engine's; the room is centred at 0.5)
    nerf._generate_point_cloud(box[0], box[1], 4096, 0.5, 0)
    cloud, ms = timed(lambda: nerf._generate_point_cloud(box[0], box[1], a.cloud_points, 0.5, 0))
    res["point_cloud"] = {"points": int(cloud["points"].shape[0]), "ms": round(ms, 2),
                          "points_per_sec": round(cloud["points"].shape[0] / ms * 1e3)}
    print(f"oriented cloud (before outlier removal): {cloud['points'].shape[0]} points in {ms:.1f} ms, "
          f"{cloud['points'].shape[0] / ms * 1e3 / 1e6:.2f} M points/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
