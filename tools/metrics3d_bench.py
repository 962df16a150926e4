#!/usr/bin/env python3
"""Timing of the nearest-neighbour search behind the 3-D mesh metrics (nerf_vo_amd/pointcloud.py, csrc/nn.hip).

  * the query at 200 000 x 200 000 surface-like points (uniform samples of the walls of a 5 x 4 x 2.5 m room, the
    queries 1 cm off them) for a few cell sizes: build of the grid, unbounded query, and the bounded query of an ICP
    iteration (0.02 m); pointcloud.DEFAULT_CELL_SIZE is the fastest unbounded one (EXPERIMENTS.md section 14);
  * one full evaluation.calculate_metrics_3d of that room against the room with every wall 1 cm further out;
  * if scipy happens to be importable, scipy.spatial.cKDTree (build + query) on the same host, as context only.

    python tools/metrics3d_bench.py [--points 200000] [--cells 0.015625 0.03125 0.0625] [--repeats 5]
Prints one JSON line.
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


def box_mesh(lower, upper):
    lo, hi = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], dtype=np.float32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], dtype=np.int64)
    return torch.from_numpy(v), torch.from_numpy(f)


def _timed(fn, repeats):
    """Median milliseconds of fn() over ``repeats`` runs after one warm-up, host clock around a device synchronise."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--cells", type=float, nargs="+", default=[1 / 64, 3 / 128, 1 / 32, 3 / 64, 1 / 16, 1 / 8])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    entry.build()
    from nerf_vo_amd import _lib
    from nerf_vo_amd.evaluation import calculate_metrics_3d
    from nerf_vo_amd.pointcloud import DEFAULT_CELL_SIZE, NeighbourGrid, sample_points_uniformly

    if not torch.cuda.is_available():
        raise SystemExit("metrics3d_bench: needs the GPU (there is no CPU fallback for the search)")
    dev = torch.device("cuda:0")
    lo, hi = np.array([-2.5, -2.0, -1.25]), np.array([2.5, 2.0, 1.25])
    mesh_gt, mesh_pred = box_mesh(lo, hi), box_mesh(lo - 0.01, hi + 0.01)
    gen = torch.Generator().manual_seed(0)
    target = sample_points_uniformly(mesh_gt[0].to(dev), mesh_gt[1].to(dev), a.points, generator=gen)
    queries = sample_points_uniformly(mesh_pred[0].to(dev), mesh_pred[1].to(dev), a.points, generator=gen)
    lib = _lib.lib()
    res = {"points": a.points, "default_cell_size": DEFAULT_CELL_SIZE, "cells": []}
    ref = None
    for cs in a.cells:
        grid = NeighbourGrid(target, cs)
        row = {"cell_size": cs, "grid": list(grid.dims),
               "build_ms": _timed(lambda: NeighbourGrid(target, cs), a.repeats)[0]}
        row["query_ms"], row["query_ms_min"], row["query_ms_max"] = _timed(lambda: grid.query(queries), a.repeats)
        row["query_bounded_0.02_ms"] = _timed(lambda: grid.query(queries, max_distance=0.02), a.repeats)[0]
        # the kernel alone (the wrapper also sorts the queries by cell and scatters the result back): the library's own
        # event profiler, "name,count,total_ms" lines
        lib.nvo_profile_enable(1)
        for _ in range(a.repeats):
            grid.query(queries)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(int(lib.nvo_profile_summary(None, 0)) + 16)
        lib.nvo_profile_summary(buf, len(buf))
        lib.nvo_profile_enable(0)
        for line in buf.value.decode().strip().splitlines():
            name, cnt, total = line.rsplit(",", 2)
            if name.strip() == "nn_query":
                row["kernel_ms"] = float(total) / max(int(cnt), 1)
        d2, idx = grid.query(queries)
        if ref is None:
            ref = (d2, idx)
        row["same_result_as_first_cell_size"] = bool(torch.equal(d2, ref[0]) and torch.equal(idx, ref[1]))
        res["cells"].append(row)
        del grid
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = calculate_metrics_3d(mesh_gt, mesh_pred, seed=0, device=dev)
    torch.cuda.synchronize()
    res["calculate_metrics_3d"] = {"seconds_first_call": time.perf_counter() - t0, "metrics": m}
    t0 = time.perf_counter()
    calculate_metrics_3d(mesh_gt, mesh_pred, seed=0, device=dev)
    torch.cuda.synchronize()
    res["calculate_metrics_3d"]["seconds_second_call"] = time.perf_counter() - t0
    try:
        import scipy.spatial
    except ImportError:
        res["scipy_cKDTree"] = None
    else:  # context only: the reference's search, on this host's CPU
        t_np, q_np = target.cpu().numpy(), queries.cpu().numpy()
        t0 = time.perf_counter()
        tree = scipy.spatial.cKDTree(t_np)
        t1 = time.perf_counter()
        d_ref, _ = tree.query(q_np)
        t2 = time.perf_counter()
        res["scipy_cKDTree"] = {"build_ms": 1e3 * (t1 - t0), "query_ms": 1e3 * (t2 - t1),
                                "max_rel_diff_to_kernel": float(np.max(np.abs(np.sqrt(ref[0].double().cpu().numpy()) - d_ref) / d_ref))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
