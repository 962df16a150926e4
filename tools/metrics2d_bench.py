#!/usr/bin/env python3
"""2-D evaluation metrics: the GPU path (nerf_vo_amd/metrics2d.py, csrc/metrics2d.hip) beside the host functions of
nerf_vo_amd/evaluation.py (``calculate_depth_metrics_2d`` + ``calculate_color_metrics_2d``: numpy float64 over every
pixel, ten depth-wise conv2d passes on CPU tensors, a numpy loop over the channels) on the same frames.

Per frame size (``--sizes``, default 1200x680 and 640x480) and batch (``--batches``, default 1 8 32): seeded uint8 colour
pairs and float64 depth pairs, then
  * ``gpu_resident``  ``color_metrics`` + ``depth_metrics`` of frames already on the device, the table's copy to the host
                      and the host's finishing included: host clock around a synchronise;
  * ``gpu_upload``    the same with the upload of the decoded frames from host memory, which is what
                      ``Evaluator2D(device=cuda)`` does per batch;
  * ``gpu_kernels``   HIP events around the two accumulator launches alone (colour: tile kernel + fold; depth: two passes
                      + fold), with the bytes the launches must read and the HBM time that implies;
  * ``cpu``           the host functions on the first ``--cpu-frames`` frames of the batch, one by one.
One warm-up, then the median (min..max) of ``--repeats`` runs; per-frame figures are the batch's time over its size.
Before timing, the GPU rows are compared with the host rows of the same frames (PSNR equal, the rest to the tests' bounds).

    python tools/metrics2d_bench.py            # one JSON line per (size, batch)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def _timed(fn, repeats, sync=True):
    times, out = [], None
    for r in range(repeats + 1):  # the first run is the warm-up
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        if r > 0:
            times.append(1e3 * (time.perf_counter() - t0))
    return {"ms": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}, out


def _event_timed(fn, repeats):
    times = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            times.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def _frames(batch, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 90 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] * np.array([1.0, 0.7, -0.8])).astype(np.int64)
    c_gt = np.clip(base[None] + rng.integers(-20, 21, (batch, h, w, 3)), 0, 255).astype(np.uint8)
    c_pred = np.clip(c_gt.astype(np.int64) + rng.integers(-8, 9, (batch, h, w, 3)), 0, 255).astype(np.uint8)
    d_gt = 2.5 + 1.8 * np.sin(xx / 91.0) * np.cos(yy / 57.0) + rng.uniform(-0.3, 0.3, (batch, h, w))
    d_pred = d_gt / 1.3 * (1 + 0.05 * rng.normal(size=(batch, h, w)))
    d_gt[:, :7] = 0.0
    return c_gt, c_pred, d_gt, d_pred


def _per_frame(t, batch):
    return {k + "_per_frame": v / batch for k, v in t.items()}


def run(sizes=((680, 1200), (480, 640)), batches=(1, 8, 32), repeats=5, cpu_frames=2, device="cuda:0"):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import calculate_color_metrics_2d, calculate_depth_metrics_2d

    if not torch.cuda.is_available():
        raise SystemExit("metrics2d_bench needs the GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device(device)
    rows = []
    for h, w in sizes:
        for batch in batches:
            c_gt, c_pred, d_gt, d_pred = _frames(batch, h, w, seed=batch)
            on_dev = [torch.from_numpy(x).to(dev) for x in (c_gt, c_pred, d_gt, d_pred)]

            def gpu_rows(tensors):
                color = metrics2d.color_metrics(tensors[0], tensors[1])
                depth = metrics2d.depth_metrics(tensors[2], tensors[3])
                return [{**d, **c} for d, c in zip(depth, color)]

            def cpu_row(k):
                row = dict(calculate_depth_metrics_2d(d_gt[k], d_pred[k]))
                row.update(calculate_color_metrics_2d(c_gt[k], c_pred[k]))
                return row

            n_cpu = min(batch, cpu_frames)
            got = gpu_rows(on_dev)
            for k in range(n_cpu):  # same numbers first, then the clock
                ref = cpu_row(k)
                assert list(got[k]) == list(ref) and got[k]["psnr"] == ref["psnr"], (got[k], ref)
                assert abs(got[k]["mssim"] - ref["mssim"]) <= 2e-6, (got[k]["mssim"], ref["mssim"])
                for name in metrics2d.DEPTH_METRICS:
                    assert abs(got[k][name] - ref[name]) <= 1e-7 * abs(ref[name]), (name, got[k][name], ref[name])

            resident, _ = _timed(lambda: gpu_rows(on_dev), repeats)
            upload, _ = _timed(lambda: gpu_rows([torch.from_numpy(x).to(dev) for x in (c_gt, c_pred, d_gt, d_pred)]), repeats)
            color_k = _event_timed(lambda: metrics2d.color_accumulators(on_dev[0], on_dev[1]), repeats)
            depth_k = _event_timed(lambda: metrics2d.depth_accumulators(on_dev[2], on_dev[3]), repeats)
            cpu, _ = _timed(lambda: [cpu_row(k) for k in range(n_cpu)], max(min(repeats, 3), 1), sync=False)
            color_bytes, depth_bytes = 2 * batch * h * w * 3, 2 * 2 * batch * h * w * 8  # depth: two passes over both maps
            row = {"measurement": "metrics2d", "height": h, "width": w, "batch": batch,
                   "gpu_resident": {**resident, **_per_frame(resident, batch)},
                   "gpu_upload": {**upload, **_per_frame(upload, batch)},
                   "gpu_kernels": {"color": {**color_k, **_per_frame(color_k, batch), "bytes": color_bytes,
                                             "hbm_floor_ms": 1e3 * color_bytes / HBM_BYTES_PER_S},
                                   "depth": {**depth_k, **_per_frame(depth_k, batch), "bytes": depth_bytes,
                                             "hbm_floor_ms": 1e3 * depth_bytes / HBM_BYTES_PER_S}},
                   "cpu": {**cpu, **_per_frame(cpu, n_cpu), "frames": n_cpu, "threads": torch.get_num_threads()},
                   "cpu_over_gpu_resident_per_frame": (cpu["ms"] / n_cpu) / (resident["ms"] / batch),
                   "cpu_over_gpu_upload_per_frame": (cpu["ms"] / n_cpu) / (upload["ms"] / batch)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del on_dev
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1200x680", "640x480"], help="WIDTHxHEIGHT")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=2, help="frames of each batch the host functions are timed on")
    a = ap.parse_args()
    entry.build()
    run(sizes=[tuple(int(v) for v in s.split("x"))[::-1] for s in a.sizes], batches=a.batches, repeats=a.repeats,
        cpu_frames=a.cpu_frames)
