#!/usr/bin/env python3
"""Timing of the k-nearest-neighbour search behind the statistical outlier removal of the point cloud
(nerf_vo_amd/pointcloud.py: NeighbourGrid.query_knn, csrc/knn.hip).

A surface-like cloud (uniform samples of the walls of a 5 x 4 x 2.5 m room, jittered by 2 mm) queries itself with k = 20:

  * ``query_knn(want='mean')`` at each ``--points`` size over a sweep of cell sizes, given as multiples of the rule
    ``pointcloud.knn_cell_size`` (cells that hold about k points): build of the grid, the whole call (sort of the queries,
    kernel, scatter) and the kernel alone (the library's event profiler).  The fastest factor is what
    ``pointcloud.KNN_POINTS_PER_CELL_FACTOR`` should be (EXPERIMENTS.md "k-NN search");
  * the table form (``want='table'``) at the smallest size, rule's cell size;
  * one ``remove_statistical_outlier`` per size;
  * for context only, a chunked ``torch.cdist`` + ``topk`` of the smallest cloud on the same GPU (another distance
    formula: not compared bit for bit, only its mean distances within 1e-4).

    python tools/knn_bench.py [--points 200000 2000000 34000000] [--factors 0.03125 0.0625 0.125 0.25 0.5 1 2] [--repeats 20]
Prints one JSON line.  Needs the GPU: a run without one fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LOWER, UPPER = (-2.5, -2.0, -1.25), (2.5, 2.0, 1.25)
K = 20


def surface_cloud(n, device, seed=0, jitter=0.002):
    """n float32 points on the six walls of the room, area-uniform, jittered (generated on the device from a seed)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    lo = torch.tensor(LOWER, device=device, dtype=torch.float64)
    hi = torch.tensor(UPPER, device=device, dtype=torch.float64)
    e = hi - lo
    area = torch.stack([e[1] * e[2], e[0] * e[2], e[0] * e[1]])  # of a wall with normal x, y, z
    axis = torch.multinomial(area / area.sum(), n, replacement=True, generator=gen)
    p = lo + torch.rand(n, 3, device=device, dtype=torch.float64, generator=gen) * e
    side = torch.rand(n, device=device, generator=gen) < 0.5
    rows = torch.arange(n, device=device)
    p[rows, axis] = torch.where(side, lo[axis], hi[axis])
    return (p + jitter * torch.randn(n, 3, device=device, dtype=torch.float64, generator=gen)).float()


def _timed(fn, repeats):
    """Median / min / max milliseconds of fn() over ``repeats`` runs after one warm-up, host clock around a device synchronise."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def _kernel_ms(lib, fn, repeats):
    lib.nvo_profile_enable(1)
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(int(lib.nvo_profile_summary(None, 0)) + 16)
    lib.nvo_profile_summary(buf, len(buf))
    lib.nvo_profile_enable(0)
    for line in buf.value.decode().strip().splitlines():
        name, cnt, total = line.rsplit(",", 2)
        if name.strip() == "knn_query":
            return float(total) / max(int(cnt), 1)
    return None


def _cdist_topk_mean(points, k, chunk=4096):
    out = torch.empty(points.shape[0], device=points.device)
    for lo in range(0, points.shape[0], chunk):
        d = torch.cdist(points[lo:lo + chunk], points)
        out[lo:lo + chunk] = d.topk(k, dim=1, largest=False).values.mean(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[200000, 2000000, 34000000])
    ap.add_argument("--factors", type=float, nargs="+", default=[1 / 32, 1 / 16, 0.125, 0.25, 0.5, 1.0, 2.0])
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    entry.build()
    from nerf_vo_amd import _lib
    from nerf_vo_amd.pointcloud import KNN_POINTS_PER_CELL_FACTOR, NeighbourGrid, knn_cell_size, remove_statistical_outlier

    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: needs the GPU (there is no CPU fallback for the search)")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    extent = [h - l for l, h in zip(LOWER, UPPER)]
    res = {"k": K, "default_factor": KNN_POINTS_PER_CELL_FACTOR, "sizes": []}
    for n in a.points:
        cloud = surface_cloud(n, dev)
        repeats = a.repeats if n <= 4000000 else min(a.repeats, 5)  # (the large size: tens of milliseconds a call)
        size = {"points": n, "repeats": repeats, "cells": []}
        ref = None
        for factor in a.factors:
            cs = knn_cell_size(n, extent, K, factor=factor)
            if any(row["cell_size"] == cs for row in size["cells"]):
                continue  # (the caps of the grid raised this factor's cell size to one already timed)
            grid = NeighbourGrid(cloud, cs)
            row = {"factor": factor, "cell_size": cs, "grid": list(grid.dims),
                   "build_ms": _timed(lambda: NeighbourGrid(cloud, cs), repeats)[0]}
            row["mean_ms"], row["mean_ms_min"], row["mean_ms_max"] = _timed(lambda: grid.query_knn(cloud, K, want="mean"), repeats)
            row["kernel_ms"] = _kernel_ms(lib, lambda: grid.query_knn(cloud, K, want="mean"), repeats)
            mean = grid.query_knn(cloud, K, want="mean")
            if ref is None:
                ref = mean
            row["same_bits_as_first_cell_size"] = bool(torch.equal(mean.view(torch.int32), ref.view(torch.int32)))
            size["cells"].append(row)
            print(json.dumps({"points": n, **row}), file=sys.stderr, flush=True)
            del grid
        if n == min(a.points):
            cs = knn_cell_size(n, extent, K)
            grid = NeighbourGrid(cloud, cs)
            t = _timed(lambda: grid.query_knn(cloud, K, want="table"), repeats)
            size["table"] = {"cell_size": cs, "ms": t[0], "ms_min": t[1], "ms_max": t[2],
                             "kernel_ms": _kernel_ms(lib, lambda: grid.query_knn(cloud, K, want="table"), repeats)}
            t = _timed(lambda: _cdist_topk_mean(cloud, K), repeats)
            size["torch_cdist_topk"] = {"ms": t[0], "ms_min": t[1], "ms_max": t[2], "chunk": 4096,
                                        "max_abs_diff_of_mean_distance": float((_cdist_topk_mean(cloud, K) - ref).abs().max())}
            del grid
        t = _timed(lambda: remove_statistical_outlier(cloud, nb_neighbors=K, std_ratio=10.0), repeats)
        size["remove_statistical_outlier_ms"] = t[0]
        size["kept"] = int(remove_statistical_outlier(cloud, nb_neighbors=K, std_ratio=10.0)[1].shape[0])
        res["sizes"].append(size)
        del cloud, ref
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
