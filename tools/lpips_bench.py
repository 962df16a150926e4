#!/usr/bin/env python3
"""LPIPS kernels at the evaluation size: 1200 x 680 frames, F = 8 pairs, synthetic weights (tools are not tests: no
acceptance figure comes from here; EXPERIMENTS.md section 24 records a run).

* per launcher, the library's HIP-event profiler (nvo_profile_enable) over ``--steps`` calls after ``--warmup``: mean
  time, and for the convolutions the achieved fp32 rate, 2 * Cout * K * F * Ho * Wo useful operations per launch (the
  zero rows that pad K are not counted), beside the 157.3 TFLOP/s fp32 matrix peak;
* the whole ``lpips_uint8`` call, by a host clock around calls that end in a copy to the host (a synchronise), with
  the profiler off;
* context rows, not gates: the float32 torch restatement of one pair on this host's CPU, and torch's own ``conv2d`` +
  ``max_pool2d`` chain on the device if the build has a convolution back-end.

Usage: python tools/lpips_bench.py [--frames 8] [--height 680] [--width 1200] [--steps 10] [--warmup 3] [--json PATH]
       [--context all|cpu|none]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TFLOPS = 157.3  # fp32 matrix, MI355X


def profile(lib, fn, steps):
    torch.cuda.synchronize()
    lib.nvo_profile_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    need = lib.nvo_profile_summary(None, 0)
    buf = C.create_string_buffer(int(need) + 16)
    lib.nvo_profile_summary(buf, len(buf))
    lib.nvo_profile_enable(0)
    out = {}
    for line in buf.value.decode().strip().splitlines():
        name, cnt, total = line.rsplit(",", 2)
        out[name.split("[")[0]] = (int(cnt), float(total))
    return out


def torch_chain(x, sd, lp):
    """The restatement with torch's own layers (float32): features of one image batch."""
    shift = torch.tensor(lp.DEFAULT_SHIFT, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(lp.DEFAULT_SCALE, device=x.device).view(1, 3, 1, 1)
    x, maps = (x - shift) / scale, []
    for l, ((_, _, _, s, p), pool) in enumerate(zip(lp.LAYERS, lp.POOL_BEFORE)):
        if pool:
            x = TF.max_pool2d(x, 3, 2)
        i = lp.TORCHVISION_INDEX[l]
        x = TF.relu(TF.conv2d(x, sd[f"features.{i}.weight"].to(x.device), sd[f"features.{i}.bias"].to(x.device), stride=s, padding=p))
        maps.append(x)
    return maps


def torch_lpips(x0, x1, sd, lp):
    total = 0
    for l, (a, b) in enumerate(zip(torch_chain(x0, sd, lp), torch_chain(x1, sd, lp))):
        n0 = a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        n1 = b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        total = total + (sd[f"lin{l}.model.1.weight"].to(a.device) * (a / n0 - b / n1) ** 2).sum(1).mean(dim=(1, 2))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--context", default="all", choices=["all", "cpu", "none"], help="which context rows to take")
    a = ap.parse_args()
    entry.build()
    from nerf_vo_amd import _lib
    from nerf_vo_amd import lpips as lp

    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench: needs the GPU -- a time taken anywhere else says nothing")
    dev, lib = torch.device("cuda:0"), _lib.lib()
    F, H, W = a.frames, a.height, a.width
    sd = lp.synthetic_weights(0)
    model = lp.LPIPS(sd, device=dev)
    g = torch.Generator().manual_seed(0)
    gt = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    pred = (gt.int() + torch.randint(-40, 41, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    gt_d, pred_d = gt.to(dev), pred.to(dev)

    for _ in range(a.warmup):
        values = model.lpips_uint8(gt_d, pred_d)
    prof = profile(lib, lambda: model.lpips_uint8(gt_d, pred_d), a.steps)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        model.lpips_uint8(gt_d, pred_d)  # ends in a copy to the host
    call_ms = (time.perf_counter() - t0) / a.steps * 1e3

    sizes = lp.feature_sizes(H, W)
    rows, conv_ms, flop_call = [], 0.0, 0.0
    print(f"LPIPS kernels, {F} pairs of {W} x {H}, {a.steps} calls after {a.warmup}; per launch (a call has two per layer)")
    for l, ((cin, cout, k, _, _), (ho, wo)) in enumerate(zip(lp.LAYERS, sizes)):
        cnt, total = prof[f"lpips_conv_k{k}_c{cin}"]
        ms, flop = total / cnt, 2.0 * cout * cin * k * k * F * ho * wo
        tf = flop / (ms * 1e-3) / 1e12
        conv_ms += 2 * ms
        flop_call += 2 * flop
        rows.append({"kernel": f"conv{l + 1}", "map": [ho, wo], "ms": ms, "gflop": flop / 1e9, "tflops": tf, "of_peak": tf / PEAK_TFLOPS})
        print(f"  conv{l + 1}  {cin:3d}->{cout:3d} {k:2d}x{k:<2d} -> {wo:3d} x {ho:3d}  {ms:8.3f} ms  {flop / 1e9:7.1f} GFLOP  {tf:6.1f} TFLOP/s  "
              f"{100 * tf / PEAK_TFLOPS:5.1f} % of {PEAK_TFLOPS}")
    for name in sorted(prof):
        if not name.startswith("lpips_conv"):
            cnt, total = prof[name]
            rows.append({"kernel": name, "ms": total / cnt, "launches_per_call": cnt / a.steps})
            print(f"  {name:16s} {total / cnt:8.3f} ms x {cnt / a.steps:.0f} per call")
    kernels_ms = sum(total for _, total in prof.values()) / a.steps
    print(f"  all launchers {kernels_ms:.2f} ms per call, convolutions {conv_ms:.2f} ms = {flop_call / 1e9:.0f} GFLOP at "
          f"{flop_call / (conv_ms * 1e-3) / 1e12:.1f} TFLOP/s")
    print(f"lpips_uint8, whole call (host clock, ends in a copy to the host): {call_ms:.2f} ms = {call_ms / F:.2f} ms per pair")
    result = {"frames": F, "height": H, "width": W, "steps": a.steps, "rows": rows, "kernels_ms_per_call": kernels_ms,
              "call_ms": call_ms, "ms_per_pair": call_ms / F, "values": values[:2]}

    def dump():
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as fh:
                json.dump(result, fh, indent=1)

    dump()  # (the context rows below can take long on a build that has to pick convolution algorithms first)
    if a.context == "none":
        print(json.dumps(result))
        return
    # context: torch's own layers
    x0, x1 = ((t[:1].permute(0, 3, 1, 2).float().div(255.0) * 2 - 1) * 2 - 1 for t in (gt, pred))
    with torch.no_grad():
        torch_lpips(x0, x1, sd, lp)
        t0 = time.perf_counter()
        ref = torch_lpips(x0, x1, sd, lp)
        cpu_ms = (time.perf_counter() - t0) * 1e3
    print(f"context: float32 torch restatement on this host's CPU ({torch.get_num_threads()} threads): {cpu_ms:.0f} ms per pair; "
          f"value {float(ref[0]):.6f} against {values[0]:.6f}")
    result.update({"cpu_torch_ms_per_pair": cpu_ms, "cpu_torch_value": float(ref[0])})
    if a.context == "cpu":
        print(json.dumps(result))
        dump()
        return
    try:
        with torch.no_grad():
            y0, y1 = ((t.permute(0, 3, 1, 2).float().div(255.0) * 2 - 1) * 2 - 1 for t in (gt_d, pred_d))
            for _ in range(a.warmup):
                torch_lpips(y0, y1, sd, lp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                got = torch_lpips(y0, y1, sd, lp).cpu()
            dev_ms = (time.perf_counter() - t0) / a.steps * 1e3
        print(f"context: torch's own conv2d chain on the device, float images already there: {dev_ms:.2f} ms per call; value {float(got[0]):.6f}")
        result["device_torch_ms_per_call"] = dev_ms
    except RuntimeError as err:  # a build without a convolution back-end
        print(f"context: torch's own conv2d on the device is not available in this build ({str(err).splitlines()[0]})")
        result["device_torch_ms_per_call"] = None
    print(json.dumps(result))
    dump()


if __name__ == "__main__":
    main()
