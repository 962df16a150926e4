"""The two forms of the ray head (csrc/rays.hip) at the bench's shape, 4096 rays x 256 samples, each ALONE: 50 launches
captured back to back in one graph, 20 replays, median (and minimum) period of a launch in us -- EXPERIMENTS.md 12.6.
Zero plan: none, plain = 1 MB + small ranges, update = plain + 2 x 2.6 MB.  Usage: python tools/probes/ray_head_forms.py"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401,E402
from nerf_vo_amd import _lib  # noqa: E402
from nerf_vo_amd.engine import _call, _stream  # noqa: E402

dev = torch.device("cuda:0")
F, H, W, R, S = 40, 480, 640, 4096, 256
g = torch.Generator().manual_seed(1)
intr = (torch.tensor([[300.0, 300.0, 320.0, 240.0]]).repeat(F, 1)).to(dev)
c2w = torch.eye(4).repeat(F, 1, 1)
c2w[:, :3, 3] = torch.randn(F, 3, generator=g) * 0.3
c2w = c2w.to(dev).contiguous()
images = torch.rand(F, H, W, 3, device=dev)
depths = torch.rand(F, H, W, device=dev)
step_dev = torch.tensor([37.0], device=dev)
extent = torch.tensor([float(F), float(H), float(W)], device=dev)
z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
b = dict(idx=z(R, 3, dt=torch.int64), jit=z(3, R), o=z(R, 3), d=z(R, 3), dn=z(R), pa=z(R), ci=z(R, dt=torch.int32), rgb=z(R, 3),
         dep=z(R), nor=z(R, 3), d01=z(R, 3), sh=z(R, 16, dt=torch.float16), sb=z(R, S + 1), tb=z(R, S + 1), x=z(R * S, 3))
ra = _lib.RayHeadArgs(R=R, S=S, seed=7, n_jitter=3, step_dev=step_dev.data_ptr(), extent_dev=extent.data_ptr(),
                      intrinsics=intr.data_ptr(), c2w=c2w.data_ptr(), c2w_stride=16, corrections=None, H=H, W=W,
                      images=images.data_ptr(), depths=depths.data_ptr(), normals=None, near_plane=0.05, far_plane=1000.0,
                      ray_indices=b["idx"].data_ptr(), jitter=b["jit"].data_ptr(), origins=b["o"].data_ptr(),
                      directions=b["d"].data_ptr(), directions_norm=b["dn"].data_ptr(), pixel_area=b["pa"].data_ptr(),
                      cam_idx=b["ci"].data_ptr(), gt_rgb=b["rgb"].data_ptr(), gt_depth=b["dep"].data_ptr(),
                      gt_normal=b["nor"].data_ptr(), dirs01=b["d01"].data_ptr(), sh=b["sh"].data_ptr(), sh_bf16=0,
                      sbins=b["sb"].data_ptr(), tbins=b["tb"].data_ptr(), x01=b["x"].data_ptr())
zbufs = {"none": [], "plain": [z(1 << 18), z(64), z(4096), z(16)], "update": [z(1 << 18), z(64), z(4096), z(16), z(650000), z(650000)]}


def launch(kind):
    zs = zbufs[kind]
    n = len(zs)
    if n == 0:
        _call("nvo_ray_head", _stream(dev), C.byref(ra))
        return
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in zs])
    sizes = (C.c_uint64 * n)(*[t.numel() * 4 for t in zs])
    _call("nvo_ray_head_zero", _stream(dev), C.byref(ra), n, ptrs, sizes)


def measure(kind, n_in_graph=50, replays=20):
    launch(kind)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(n_in_graph):
            launch(kind)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / n_in_graph)
    times.sort()
    return times[len(times) // 2], times[0]


for rnd in range(2):
    for name, generic in (("k_ray_head (thread per sample)", True), ("k_ray_head_x4", False)):
        os.environ.pop("NVO_RAY_HEAD_GENERIC", None)
        if generic:
            os.environ["NVO_RAY_HEAD_GENERIC"] = "1"  # (read per launch; a captured graph keeps its capture's)
        row = []
        for kind in ("none", "plain", "update"):
            med, mn = measure(kind)
            row.append(f"{kind} {med:6.2f} (min {mn:6.2f})")
        print(f"round {rnd} {name:32s} us/launch: " + " | ".join(row), flush=True)
os.environ.pop("NVO_RAY_HEAD_GENERIC", None)
