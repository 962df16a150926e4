#!/usr/bin/env python3
"""Timing of the dense-lattice Poisson reconstruction (nerf_vo_amd/poisson.py, csrc/poisson.hip) per phase.

A seeded cloud on the six walls of a 5 x 4 x 2.5 m room (inward normals, 2 mm jitter along the normal is NOT added: the
walls lie on the box) goes through the phases of ``poisson_reconstruct`` one by one, each timed by a host clock around a
device synchronise, after one untimed pass of the two torch phases (bin and trim): bin, splat of the density, density at
the points, splat of the vector field, right-hand side, every V(2,2) cycle (with its residual max-norm), chi at the points, extraction, density at the vertices, trim.  Then the
fine-level half-sweep and the residual + restriction pass alone, ``--repeats`` times, with the bytes per second they
achieve beside the copy rate MI355X_MICROARCH measured (about 6.3 TB/s).  Bytes are counted from the shapes, whole
cache lines: a half-sweep reads chi (4 B per node) and f (4 B) and writes chi (4 B), 12 B per node; the residual pass
reads chi and f (8 B per node) and writes the coarse right-hand side (0.5 B).

    python tools/poisson_bench.py [--depths 7 9] [--points 34000000] [--repeats 10] [--limit 600]
Every depth runs in a fresh child process under its own time limit of ``--limit`` seconds; after a child that fails
or runs out of time nothing more is started.  Prints one JSON line per depth.  Needs the GPU: a run without one fails.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOWER, UPPER = (-2.5, -2.0, -1.25), (2.5, 2.0, 1.25)
COPY_RATE = 6.3e12  # bytes per second, the streaming copy rate measured on the MI355X


def room_cloud(n, device, seed=0):
    """(points, inward unit normals, colours): n float32 points on the six walls, area-uniform, generated on the device."""
    import torch

    gen = torch.Generator(device=device).manual_seed(seed)
    lo = torch.tensor(LOWER, device=device, dtype=torch.float64)
    hi = torch.tensor(UPPER, device=device, dtype=torch.float64)
    e = hi - lo
    area = torch.stack([e[1] * e[2], e[0] * e[2], e[0] * e[1]])
    axis = torch.multinomial(area / area.sum(), n, replacement=True, generator=gen)
    p = lo + torch.rand(n, 3, device=device, dtype=torch.float64, generator=gen) * e
    side = torch.rand(n, device=device, generator=gen) < 0.5
    rows = torch.arange(n, device=device)
    p[rows, axis] = torch.where(side, lo[axis], hi[axis])
    normals = torch.zeros(n, 3, device=device)
    normals[rows, axis] = torch.where(side, 1.0, -1.0)
    colors = (torch.rand(n, 3, device=device, generator=gen) * 255).to(torch.uint8)
    return p.float().clamp(lo.float(), hi.float()), normals, colors


def worker(depth, n_points, repeats, cycles):
    import torch

    import __graft_entry__ as entry

    entry.build()
    from nerf_vo_amd import poisson as P
    from nerf_vo_amd.meshing import extract_isosurface

    if not torch.cuda.is_available():
        raise SystemExit("poisson_bench: needs the GPU (the kernels have no CPU fallback)")
    dev = torch.device("cuda:0")
    phases = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        phases[name] = 1e3 * (time.perf_counter() - t0)
        return out

    points, normals, _ = room_cloud(n_points, dev)
    lattice = P.poisson_lattice(LOWER, UPPER, depth)
    nx, ny, nz = lattice["nodes"]
    nodes = nx * ny * nz
    P.sweep(torch.zeros(5, 5, 5, device=dev), torch.zeros(5, 5, 5, device=dev), 0)  # loads the code object
    # one untimed pass of the two torch phases at the timed sizes' order of magnitude: the first sort, bincount and
    # boolean indexing of a process load and tune their kernels, which is not the phases' cost
    P.bin_points(points, lattice)
    warm = torch.rand(1 << 20, device=dev)
    P.trim_by_density(warm.repeat(3, 1).T.contiguous(), torch.randint(0, 1 << 20, (1 << 21, 3), device=dev), warm)
    del warm
    order, cell_start = timed("bin", lambda: P.bin_points(points, lattice))
    pts_s, nrm_s = points[order].contiguous(), normals[order].contiguous()
    W = timed("splat_density", lambda: P.splat(pts_s, cell_start, lattice))
    D = timed("sample_density_at_points", lambda: P.sample(W, pts_s, lattice))
    V = timed("splat_vector_field", lambda: P.splat(pts_s, cell_start, lattice, values=nrm_s, denom=D))
    rhs = timed("rhs", lambda: P.divergence(V))
    del V
    # the cycles one by one (solve() does the same calls in a loop)
    import ctypes as C

    from nerf_vo_amd import _lib

    lib = _lib.lib()
    scratch = torch.empty(int(lib.nvo_poisson_vcycle_scratch_bytes(nx, ny, nz, lattice["levels"])), dtype=torch.uint8, device=dev)
    chi = torch.zeros_like(rhs)
    norms = torch.zeros(cycles + 1, dtype=torch.int32, device=dev)
    args = _lib.PoissonVcycleArgs(chi=chi.data_ptr(), rhs=rhs.data_ptr(), scratch=scratch.data_ptr(), nx=nx, ny=ny, nz=nz,
                                  levels=lattice["levels"])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P._level_call("residual_norm", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), norm_bits=norms.data_ptr())
    for c in range(cycles):
        timed(f"vcycle_{c + 1}", lambda: _lib.check(lib.nvo_poisson_vcycle(stream, C.byref(args)), "poisson_vcycle"))
        P._level_call("residual_norm", chi, chi=chi.data_ptr(), rhs=rhs.data_ptr(), norm_bits=norms.data_ptr() + 4 * (c + 1))
    residual = norms.view(torch.float32).tolist()
    iso = timed("iso_value", lambda: float(P.sample(chi, pts_s, lattice).to(torch.float64).mean()))
    vertices, faces = timed("extract", lambda: extract_isosurface(chi, lattice["origin"], lattice["upper"], iso))
    density = timed("sample_density_at_vertices", lambda: P.sample(W, vertices, lattice)[:, 0])
    v, f, _, threshold, _ = timed("trim", lambda: P.trim_by_density(vertices, faces, density))

    def repeated(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / repeats

    work = chi.clone()
    sweep_ms = repeated(lambda: (P.sweep(work, rhs, 0), P.sweep(work, rhs, 1))) / 2
    restrict_ms = repeated(lambda: P.restrict(chi, rhs))
    out = {"depth": depth, "points": n_points, "lattice": [nx, ny, nz], "levels": lattice["levels"], "cycles": cycles,
           "phases_ms": {k: round(x, 3) for k, x in phases.items()}, "total_ms": round(sum(phases.values()), 3),
           "residual_over_start": [r / residual[0] for r in residual[1:]], "iso": iso,
           "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "vertices_kept": int(v.shape[0]), "faces_kept": int(f.shape[0]),
           "density_threshold": threshold,
           "half_sweep": {"ms": sweep_ms, "bytes": 12 * nodes, "bytes_per_s": 12 * nodes / (sweep_ms * 1e-3),
                          "share_of_copy_rate": 12 * nodes / (sweep_ms * 1e-3) / COPY_RATE},
           "residual_restrict": {"ms": restrict_ms, "bytes": 8.5 * nodes, "bytes_per_s": 8.5 * nodes / (restrict_ms * 1e-3),
                                 "share_of_copy_rate": 8.5 * nodes / (restrict_ms * 1e-3) / COPY_RATE},
           "copy_rate_bytes_per_s": COPY_RATE}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="+", default=[7, 9])
    ap.add_argument("--points", type=int, default=34000000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--limit", type=float, default=600.0, help="seconds per depth (a fresh process each)")
    ap.add_argument("--worker", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker is not None:
        worker(a.worker, a.points, a.repeats, a.cycles)
        return
    for depth in a.depths:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(depth), "--points", str(a.points), "--repeats",
               str(a.repeats), "--cycles", str(a.cycles)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"poisson_bench: depth {depth} did not finish within {a.limit:g} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"poisson_bench: depth {depth} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
