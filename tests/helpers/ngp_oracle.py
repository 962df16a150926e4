"""Plain-torch CPU restatements of the occupancy-grid back-end's per-ray and per-sample kernels (csrc/ngp.hip:
nvo_ngp_composite_loss, nvo_ngp_count_alive, nvo_ngp_thickness, nvo_ngp_positions[_live]; csrc/mlp.hip: nvo_ngp_rgb_fwd /
nvo_ngp_rgb_bwd) -- plus the seeded case generators of tests/test_ngp_kernels_gpu.py and tests/test_ngp_oracle_cpu.py.

Every reference function takes ``dtype=``: float64 is the reference, the float32 run of the SAME function on the same
inputs is the yardstick the bounds come from (bound = factor * e32 + 1e-6, profiles/ngp_parity_margins.json, written by
tests/helpers/ngp_tolerances.py).  The kernels evaluate every exponential with __expf, which the device headers define
as exp2(log2e * x) with the product in float32 (log2e = 0x1.715476p+0): the float32 run uses that formulation
(``_exp``), so e32 carries the rounding of the argument, which grows with |x|; the largest |x| fed to an exponential is
recorded per reference call (``max_abs_x``).

Every generator returns, next to the tensors, the class counts the tests assert on (``classes``), so that a test cannot
silently lose a branch.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARGINS_PATH = os.path.join(ROOT, "profiles", "ngp_parity_margins.json")
DEFAULT_FACTOR = 4.0
FLOOR = 1e-6
F64, F32 = torch.float64, torch.float32
LOG2E_F32 = float(np.float32(float.fromhex("0x1.715476p+0")))
SIGMA_GRAD_MAX = float(np.float32(3.2690173e6))  # the kernel's clamp on d exp(x) / dx
DD_CAP = 128.0
TIE_MARGIN = 1e-3  # no sample's transmittance within this (relative) of a threshold a test uses
FP16_MAX = 65504.0


def figure(got, ref) -> float:
    """max|got - ref| / max|ref|; plain max|got - ref| where ref is all zero; inf when got holds a non-finite value."""
    ref = torch.as_tensor(ref).double()
    got = torch.as_tensor(got).double()
    if ref.numel() == 0:
        return 0.0
    err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
    scale = float(ref.abs().max())
    return err / scale if scale > 0 else err


def load_margins(path: str = MARGINS_PATH) -> dict:
    with open(path) as fh:
        return json.load(fh)


def bound_for(key: str, margins: dict) -> float:
    factor = margins.get("factors", {}).get(key, {}).get("factor", DEFAULT_FACTOR)
    return factor * margins["e32"][key] + FLOOR


def half_ulp_fp16(ref):
    """half an fp16 ulp of |ref|, elementwise: 2^-11 |ref| for normal values, 2^-25 absolute in the subnormal range"""
    a = torch.as_tensor(ref).double().abs()
    return torch.where(a >= 2.0 ** -14, a * 2.0 ** -11, torch.full_like(a, 2.0 ** -25))


class _Rec:
    """largest finite |x| fed to an exponential"""

    def __init__(self):
        self.max_abs_x = 0.0

    def see(self, x):
        f = x[torch.isfinite(x)]
        if f.numel():
            self.max_abs_x = max(self.max_abs_x, float(f.abs().max()))


def _exp(x, rec=None):
    """exp as the kernels have it.  float32: __expf = exp2(log2e * x), the product rounded to float32; float64: exp."""
    if rec is not None:
        rec.see(x)
    if x.dtype == F32:
        return torch.exp2(x * torch.tensor(LOG2E_F32, dtype=F32))
    return torch.exp(x)


# ------------------------------------------------------------------------------------------------------------------
# nvo_ngp_composite_loss
# ------------------------------------------------------------------------------------------------------------------
def make_opts(**kw):
    """The scalar side of one nvo_ngp_loss_args: which nullable inputs are passed and the multipliers."""
    o = {"background": True, "depth": "on",  # "on" | "null" (gt_depth NULL) | "mult0" (depth_mult 0)
         "cov": True, "state": False, "thr": 0.0, "R_dev": None, "world_size": 1, "rgb_mult": 1.0, "depth_mult": 0.5,
         "inv_rays": None, "loss_scale": 128.0, "dnorm": True}
    o.update(kw)
    return o


def _ray_pass(pre, y, t, dt, carry_in, dtype, rec):
    sigma = _exp(pre.to(dtype), rec)
    dd = torch.clamp(sigma * dt.to(dtype), max=DD_CAP)
    incl = torch.cumsum(dd, 0) + carry_in
    T = _exp(-(incl - dd), rec)
    w = (1.0 - _exp(-dd, rec)) * T
    rgb = 1.0 / (1.0 + _exp(-y.to(dtype), rec))
    return sigma, dd, incl, T, w, rgb


def composite_reference(case, training, opts=None, dtype=F64, counts=None, offsets=None, carry_in=None):
    """The header contract of nvo_ngp_loss_args.  Forward: sigma = exp(pre), dd = min(sigma dt, 128),
    T_j = exp(-(sum_{i<j} dd_i + carry_in)), w = (1 - exp(-dd)) T, rgb = sigmoid(y), pixel = sum w rgb (+ T_final bg, state 0
    only), depth = sum w t, accumulation = sum w.  Losses: rgb_mult * mean over rays and channels of (pixel - gt)^2;
    depth_mult * mean over rays of [z > 0] (depth - z)^2 / var with z = gt_depth * directions_norm and 1 / var -> 0 for a
    var that is not positive and finite; the mean is inv_rays (as passed, or 1 / (R_dev max(world_size, 1))).  Rays past
    R_dev, dropped rays (count 0 with a kept slot range) and state-2 rays add nothing to the losses.

    Gradients (training): d loss / d pre_i and d loss / d y_i times loss_scale in CLOSED FORM,
        d/dsigma_i = dt_i [T_i exp(-dd_i) (g_pix . rgb_i + g_depth t_i) - sum_{j>i} q_j - T_final g_pix . bg],
        q_j = w_j (g_pix . rgb_j + g_depth t_j),   d/dpre_i = d/dsigma_i * min(sigma_i, 3.2690173e6),
        d/dy_i = w_i g_pix rgb_i (1 - rgb_i),
    with d/dpre_i = 0 on a sample whose optical step is capped (sigma_i dt_i >= 128: the derivative of min(., 128) there),
    then exact zeros in both where T_i < train_min_transmittance.  This is the kernel's rule.  It differs from plain
    autograd of the forward in one place: d exp(x) / dx is clamped at 3.2690173e6 (autograd: sigma) -- which matters only
    where sigma > 3.27e6 on an UNCAPPED sample, and that needs dt < 4e-5; no generator builds one.  On every generated sample
    the two agree to far below float32 resolution (tests/test_ngp_oracle_cpu.py asserts it against
    ``composite_autograd``), except on the ONE sample with pre = fp16 max: sigma = inf, autograd's chain ends in
    0 * inf = NaN, the rule gives the capped sample's exact 0.
    (Why the cap has to be honoured: in exact arithmetic the bracket of a capped sample is below exp(-128), but in float32
    the suffix total_q - incl_q is the rounding noise of two sums of all q, about 1e-7 |total_q|, and min(sigma, 3.27e6)
    turns that into a gradient of up to several per cent of the ray's largest true one -- the float32 run of this very
    function showed 6e-2 of max|d_pre| on the +30..+70 samples before the rule had the zero.)

    Returns per-ray outputs, per-ray loss terms, the per-slot gradients ([capacity], [capacity][3]; zeros outside live
    rays), per-slot T and the ``dead`` / ``live`` masks."""
    o = make_opts(**(opts or {}))
    R, cap = case["R"], case["capacity"]
    counts = case["counts"] if counts is None else counts
    offsets = case["offsets"] if offsets is None else offsets
    rec = _Rec()
    R_use = R if o["R_dev"] is None else min(R, o["R_dev"])
    if o["R_dev"] is not None:
        inv_rays = 1.0 / (o["R_dev"] * max(o["world_size"], 1))
    else:
        inv_rays = o["inv_rays"] if o["inv_rays"] is not None else 1.0 / R
    inv_rays = torch.tensor(float(np.float32(inv_rays)), dtype=dtype)  # (a float32 argument of the kernel)
    out_rgb, out_depth = torch.zeros(R, 3, dtype=dtype), torch.zeros(R, dtype=dtype)
    out_acc, carry = torch.zeros(R, dtype=dtype), torch.zeros(R, dtype=dtype)
    l_rgb, l_depth = torch.zeros(R, dtype=dtype), torch.zeros(R, dtype=dtype)
    d_pre, d_y = torch.zeros(cap, dtype=dtype), torch.zeros(cap, 3, dtype=dtype)
    T_all = torch.full((cap,), float("nan"), dtype=dtype)
    dead = torch.zeros(cap, dtype=torch.bool)
    live = torch.zeros(cap, dtype=torch.bool)
    written = torch.zeros(R, dtype=torch.bool)
    capped_ray = torch.zeros(R, dtype=torch.bool)
    third = torch.tensor(1.0, dtype=dtype) / 3.0
    for r in range(R_use):
        n, base = int(counts[r]), int(offsets[r])
        sl = slice(base, base + n)
        c_in = torch.zeros((), dtype=dtype) if carry_in is None else carry_in[r].to(dtype)
        sigma, dd, incl, T, w, rgb = _ray_pass(case["pre"][sl], case["y"][sl], case["t"][sl], case["dt"][sl], c_in, dtype, rec)
        tt, dts = case["t"][sl].to(dtype), case["dt"][sl].to(dtype)
        total = incl[-1] if n else c_in
        T_final = _exp(-total.reshape(1), rec)[0]
        state = int(case["state"][r]) if (training and o["state"]) else 0
        bg = torch.zeros(3, dtype=dtype)
        if o["background"] and state == 0:
            bg = case["background"][r].to(dtype)
        pix = (w[:, None] * rgb).sum(0) + T_final * bg
        depth, acc = (w * tt).sum(), w.sum()
        out_rgb[r], out_depth[r], out_acc[r], carry[r] = pix, depth, acc, total
        written[r] = True
        capped_ray[r] = bool((~(dd < DD_CAP)).any())
        T_all[sl] = T
        if not training:
            continue
        dropped = n == 0 and int(offsets[r + 1]) != base
        if dropped or state == 2:
            continue
        e = pix - case["gt_rgb"][r].to(dtype)
        l_rgb[r] = (e * e).sum() * inv_rays * third * o["rgb_mult"]
        g_pix = 2.0 * e * inv_rays * third * o["rgb_mult"]
        g_depth = torch.zeros((), dtype=dtype)
        if o["depth"] == "on" and o["depth_mult"] != 0.0:
            z = case["gt_depth"][r].to(dtype) * (case["dnorm"][r].to(dtype) if o["dnorm"] else 1.0)
            wgt = torch.ones((), dtype=dtype)
            if o["cov"]:
                var = case["cov"][r].to(dtype)
                wgt = 1.0 / var if bool(var > 0) and bool(torch.isfinite(var)) else torch.zeros((), dtype=dtype)
            if bool(z > 0):
                ed = depth - z
                l_depth[r] = ed * ed * wgt * inv_rays * o["depth_mult"]
                g_depth = 2.0 * ed * wgt * inv_rays * o["depth_mult"]
        dot = g_depth * tt + (rgb * g_pix).sum(1)
        q = w * dot
        suffix = q.sum() - torch.cumsum(q, 0)
        g_bg = T_final * (g_pix * bg).sum()
        dsigma = dts * (T * _exp(-dd, rec) * dot - suffix - g_bg)
        is_dead = T < o["thr"]
        gp = dsigma * torch.clamp(sigma, max=SIGMA_GRAD_MAX) * o["loss_scale"]
        gy = (w[:, None] * g_pix[None, :]) * rgb * (1.0 - rgb) * o["loss_scale"]
        d_pre[sl] = torch.where(is_dead | ~(dd < DD_CAP), torch.zeros_like(gp), gp)
        d_y[sl] = torch.where(is_dead[:, None], torch.zeros_like(gy), gy)
        dead[sl] = is_dead
        live[sl] = True
    return {"out_rgb": out_rgb, "out_depth": out_depth, "out_acc": out_acc, "carry": carry, "l_rgb": l_rgb,
            "l_depth": l_depth, "loss_rgb": l_rgb.sum().reshape(1), "loss_depth": l_depth.sum().reshape(1), "d_pre": d_pre,
            "d_y": d_y, "T": T_all, "dead": dead, "live": live, "written": written, "capped_ray": capped_ray,
            "max_abs_x": rec.max_abs_x}


def composite_autograd(case, opts=None, pre=None, y=None):
    """loss_scale * (rgb loss + depth loss) of ``composite_reference`` as ONE float64 autograd graph over the
    pre-activations (plain torch.exp, torch.minimum, torch.sigmoid -- no restated derivative, no threshold).
    -> (loss, pre leaf [capacity], y leaf [capacity][3]).  ``pre`` / ``y``: float64 overrides (central differences)."""
    o = make_opts(**(opts or {}))
    R = case["R"]
    pre = (case["pre"].double() if pre is None else pre).clone().requires_grad_(True)
    y = (case["y"].double() if y is None else y).clone().requires_grad_(True)
    R_use = R if o["R_dev"] is None else min(R, o["R_dev"])
    inv_rays = 1.0 / (o["R_dev"] * max(o["world_size"], 1)) if o["R_dev"] is not None else (o["inv_rays"] or 1.0 / R)
    inv_rays = float(np.float32(inv_rays))
    loss = torch.zeros((), dtype=F64)
    for r in range(R_use):
        n, base = int(case["counts"][r]), int(case["offsets"][r])
        state = int(case["state"][r]) if o["state"] else 0
        if (n == 0 and int(case["offsets"][r + 1]) != base) or state == 2:
            continue
        sl = slice(base, base + n)
        tt, dts = case["t"][sl].double(), case["dt"][sl].double()
        dd = torch.minimum(torch.exp(pre[sl]) * dts, torch.tensor(DD_CAP, dtype=F64))
        incl = torch.cumsum(dd, 0)
        w = (1 - torch.exp(-dd)) * torch.exp(-(incl - dd))
        pix = (w[:, None] * torch.sigmoid(y[sl])).sum(0)
        if o["background"] and state == 0:
            pix = pix + torch.exp(-dd.sum()) * case["background"][r].double()
        loss = loss + o["rgb_mult"] * inv_rays * ((pix - case["gt_rgb"][r].double()) ** 2).sum() / 3.0
        if o["depth"] == "on" and o["depth_mult"] != 0.0:
            z = case["gt_depth"][r].double() * (case["dnorm"][r].double() if o["dnorm"] else 1.0)
            var = case["cov"][r].double() if o["cov"] else torch.ones((), dtype=F64)
            if bool(z > 0) and bool(var > 0) and bool(torch.isfinite(var)):
                loss = loss + o["depth_mult"] * inv_rays * ((w * tt).sum() - z) ** 2 / var
    return loss * o["loss_scale"], pre, y


LISTED_COUNTS = ("empty", "dropped", 1, 2, 63, 64, 65, 127, 128, 129, 200)
EXTRA_COUNTS = ("empty2", 5, 17, 33, 70, 96, 12, 3, 40, 64, 65, 20, 9, 130)
COV_CLASSES = ("one", "decades", "zero", "negative", "inf", "nan")
DROPPED_SLOTS = 24


def _f16(x):
    return x.to(torch.float16)


def composite_case(seed=0, listed=LISTED_COUNTS, extra=EXTRA_COUNTS, specials=True, free_slots=20):
    """Packed rays with the listed sample counts in shuffled order, a dropped ray (count 0, DROPPED_SLOTS slots kept, rows
    ray_idx = -1), truly empty rays (one of state 0, one of state 2) and free slots behind the last offset; the inputs of
    slots that belong to no ray are NaN (nothing may read them).  pre (fp16): thin rays (-6..-2), surface-like rays (thin,
    then 2..6 from part-way on; the long ones turn opaque BEHIND sample 64, so that the chunk carries matter), one ray
    with +30..+70 in mid-ray behind thin samples, one sample at fp16 max, one at -inf.  y in +-8 with +-30 on a few
    samples; dt in [0.005, 0.05] with one dt = 0 sample, t increasing."""
    g = torch.Generator().manual_seed(4100 + seed)
    entries = list(listed) + list(extra)
    entries = [entries[i] for i in torch.randperm(len(entries), generator=g).tolist()]
    R = len(entries)
    counts = torch.tensor([e if isinstance(e, int) else 0 for e in entries], dtype=torch.int32)
    spans = torch.tensor([DROPPED_SLOTS if e == "dropped" else (e if isinstance(e, int) else 0) for e in entries])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(spans, 0)]).to(torch.int32)
    total = int(offsets[-1])
    cap = (total + free_slots + 15) // 16 * 16
    nan = float("nan")
    ray_idx = torch.full((cap,), -1, dtype=torch.int32)
    t, dt = torch.full((cap,), nan), torch.full((cap,), nan)
    pre, y = torch.full((cap,), nan), torch.full((cap, 3), nan)
    kind = {}
    cls = {"thin": 0, "surface": 0, "hot": 0, "fp16_max": 0, "neg_inf": 0, "dt0": 0, "y30": 0}
    hot_ray = max((r for r in range(R) if int(counts[r]) >= 129), key=lambda r: int(counts[r])) if specials else -1
    long_seen = 0
    for r in range(R):
        n, base = int(counts[r]), int(offsets[r])
        if n == 0:
            continue
        sl = slice(base, base + n)
        ray_idx[sl] = r
        d = 0.005 + 0.045 * torch.rand(n, generator=g)
        dt[sl] = d
        t[sl] = 0.1 + torch.cumsum(d, 0) - 0.5 * d
        p = -6.0 + 4.0 * torch.rand(n, generator=g)
        yy = (torch.rand(n, 3, generator=g) * 2 - 1) * 8.0
        if r == hot_ray:
            kind[r] = "hot"
            a, b = n // 2, n // 2 + 6
            p[a:b] = 30.0 + 40.0 * torch.rand(b - a, generator=g)
            p[a] = 70.0
            cls["hot"] += b - a
            cls["thin"] += n - (b - a)
        else:
            if n > 64:
                long_seen += 1
                surf = long_seen % 2 == 0
                start = 64 + (n - 64) // 2
            else:
                surf = r % 2 == 0 and n >= 2
                start = n // 2
            if surf:
                kind[r] = "surface"
                p[start:] = 2.0 + 4.0 * torch.rand(n - start, generator=g)
                cls["surface"] += n - start
                cls["thin"] += start
            else:
                kind[r] = "thin"
                cls["thin"] += n
        if n >= 8:
            yy[n // 3, r % 3] = 30.0 if r % 2 else -30.0
            cls["y30"] += 1
        pre[sl], y[sl] = p, yy
    if specials:
        by_n = {int(counts[r]): r for r in range(R) if int(counts[r]) and r != hot_ray}
        r = by_n[127]
        pre[int(offsets[r]) + 60] = FP16_MAX  # (dt > 0 there: sigma dt = inf, capped)
        cls["fp16_max"] += 1
        r = by_n[65]
        pre[int(offsets[r]) + 10] = -float("inf")
        cls["neg_inf"] += 1
        r = by_n[63]
        dt[int(offsets[r]) + 5] = 0.0
        cls["dt0"] += 1
    i = torch.arange(R)
    background, gt_rgb = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    gt_depth = 0.5 + 2.5 * torch.rand(R, generator=g)
    gt_depth[i % 5 == 2] = 0.0
    dnorm = 1.0 + 0.2 * torch.rand(R, generator=g)
    dec = 10.0 ** (torch.rand(R, generator=g) * 3.0 - 1.5)
    cov = torch.ones(R)
    cov_class = [COV_CLASSES[(r + r // 6) % 6] for r in range(R)]  # (decoupled from the period-5 gt_depth = 0 pattern)
    for r, c in enumerate(cov_class):
        cov[r] = {"one": 1.0, "decades": float(dec[r]), "zero": 0.0, "negative": -1.0, "inf": float("inf"), "nan": nan}[c]
    state = torch.zeros(R, dtype=torch.int32)
    for r, e in enumerate(entries):
        if e in ("dropped", "empty2"):
            state[r] = 2
        elif isinstance(e, int) and r % 4 == 1:
            state[r] = 1
    cls.update({f"count_{e}": entries.count(e) for e in set(entries)})
    cls.update({f"cov_{c}": cov_class.count(c) for c in COV_CLASSES})
    for c in COV_CLASSES:  # classes that reach the depth term of a live ray with z > 0
        cls[f"cov_{c}_live"] = sum(1 for r in range(R) if cov_class[r] == c and int(counts[r]) > 0 and float(gt_depth[r]) > 0)
    cls.update({"gt_depth_zero": int((gt_depth == 0).sum()), "state0": int((state == 0).sum()),
                "state1_short": sum(1 for r in range(R) if state[r] == 1 and 0 < counts[r] <= 64),
                "state1_long": sum(1 for r in range(R) if state[r] == 1 and counts[r] > 64),
                "state2": int((state == 2).sum()), "free_slots": cap - total, "dropped_slots": DROPPED_SLOTS,
                "long_surface": sum(1 for r, k in kind.items() if k == "surface" and counts[r] > 64),
                "long_thin": sum(1 for r, k in kind.items() if k == "thin" and counts[r] > 64)})
    return {"R": R, "capacity": cap, "entries": entries, "counts": counts, "offsets": offsets, "ray_idx": ray_idx, "t": t,
            "dt": dt, "pre": _f16(pre), "y": _f16(y), "background": background, "gt_rgb": gt_rgb, "gt_depth": gt_depth,
            "dnorm": dnorm, "cov": cov, "state": state, "kind": kind, "classes": cls}


def threshold_margin(T, thr):
    """min over the finite entries of |T / thr - 1|"""
    T = T[torch.isfinite(T)].double()
    return float((T / thr - 1.0).abs().min()) if T.numel() and thr > 0 else float("inf")


# the training variants of test a (and the keys of their comparisons)
TRAIN_THR = 0.05
COMPOSITE_VARIANTS = {
    "bg-depth-cov-thr0": dict(background=True, depth="on", cov=True, thr=0.0),
    "bg-depth-cov-thr05": dict(background=True, depth="on", cov=True, thr=TRAIN_THR),
    "nobg-depth-cov-thr0": dict(background=False, depth="on", cov=True, thr=0.0),
    "nobg-depth-nocov-thr05": dict(background=False, depth="on", cov=False, thr=TRAIN_THR),
    "bg-depth-nocov-thr0": dict(background=True, depth="on", cov=False, thr=0.0),
    "bg-nodepth-thr05": dict(background=True, depth="null", cov=True, thr=TRAIN_THR),
    "nobg-mult0-thr0": dict(background=False, depth="mult0", cov=True, thr=0.0, depth_mult=0.0),
    "states-thr0": dict(background=True, depth="on", cov=True, thr=0.0, state=True),
    "states-thr05": dict(background=True, depth="on", cov=True, thr=TRAIN_THR, state=True),
}
RAY_OUTPUTS = ("out_rgb", "out_depth", "out_acc")
RAY_LOSSES = ("l_rgb", "l_depth")  # one shard per ray (R <= 64)
LOSS_TOTALS = ("loss_rgb", "loss_depth")
SAMPLE_QUANTITIES = ("d_pre", "d_y") + LOSS_TOTALS
COMPOSITE_QUANTITIES = RAY_OUTPUTS + RAY_LOSSES + tuple(q + "_capped" for q in RAY_OUTPUTS + RAY_LOSSES) + SAMPLE_QUANTITIES
# A ray that holds a capped sample (exp(pre) dt >= 128) is judged under keys of its own (..._capped): the transmittance the
# sample is reached with is read as exp(-((p + 128) - 128)) from the INCLUSIVE scan, p the optical depth in front of it, so
# every add that rounds at the scale of 128 (half an ulp there: 2^-18 = 3.8e-6 below 128, 2^-17 = 7.6e-6 from 128 on)
# lands in the exponent of T, and with it in the ray's outputs and its loss terms, at full size.  The float32 oracle's sequential cumsum
# commits ONE such rounding (the add of the capped step onto p); the kernel's wave scan adds partial sums onto the term
# that holds the 128 in up to six DPP steps and once more for the chunk carry: seven.  Hence 7 x the default factor for the
# ..._capped keys.  (The two loss totals hold those rays' terms too, but stay inside the default factor: not raised.)
CAPPED_FACTOR = 7 * DEFAULT_FACTOR
CAPPED_REASON = ("rays with a capped sample: T is read as exp(-((p + 128) - 128)) from the inclusive scan; the wave scan rounds "
                 "at the scale of 128 (half ulp 7.6e-6) in up to 6 DPP steps + 1 carry add, the float32 oracle's sequential "
                 "cumsum once: 7 x the default factor 4")


def ray_output_figures(got, ref, written, capped_ray, quantities=RAY_OUTPUTS):
    """{quantity or quantity_capped: figure} of per-ray quantities, rays with a capped sample apart"""
    out = {}
    for q in quantities:
        for suffix, rows in (("", written & ~capped_ray), ("_capped", written & capped_ray)):
            out[q + suffix] = figure(torch.as_tensor(got[q])[rows], ref[q][rows])
    return out
LAYOUTS = ("wide", "compact")  # strides 16 / 16 / 16, and density 1 / rgb 4 / d_rgb 3
RDEV_WORLDS = (0, 1, 2)
RDEV_SHORT = 5  # R_dev = R - 5
ROUND_CUTS = (17, 64, 100)


def split_rounds(case, cut):
    """the two launches of an inference in rounds: (counts, offsets) of the first min(n, cut) samples of every ray and of
    the rest (a ray without a rest sits the second round out with count 0)"""
    n = case["counts"].clone()
    first = torch.clamp(n, max=cut)
    off2 = case["offsets"].clone()
    off2[:-1] += first
    return (first, case["offsets"]), (n - first, off2)


def pair_case():
    """rays 2k (64 samples) and 2k + 1 (the same 64 samples and a 65th with dt = 0): the one-pass register form against
    the three-pass chunked form on the same arithmetic"""
    base = composite_case()
    src = [r for r in range(base["R"]) if int(base["counts"][r]) in (64, 70, 96, 128)]
    assert len(src) >= 4 and {base["kind"][r] for r in src} >= {"thin", "surface"}
    counts, chunks = [], {k: [] for k in ("t", "dt", "pre", "y")}
    per_ray = {k: [] for k in ("background", "gt_rgb", "gt_depth", "dnorm", "cov")}
    for r in src:
        o = int(base["offsets"][r])
        # (the surface rays of the shared case turn opaque behind sample 64: take a window that holds the onset)
        a = o + (int(base["counts"][r]) - 64 if base["kind"][r] == "surface" else 0)
        for n in (64, 65):
            for k in chunks:
                v = base[k][a:a + 64]
                extra = v[-1:].clone()
                if k == "dt":
                    extra = torch.zeros(1)
                chunks[k].append(v if n == 64 else torch.cat([v, extra]))
            counts.append(n)
            for k in per_ray:
                per_ray[k].append(base[k][r:r + 1])
    R = len(counts)
    counts = torch.tensor(counts, dtype=torch.int32)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts.long(), 0)]).to(torch.int32)
    total = int(offsets[-1])
    cap = (total + 15) // 16 * 16
    pad = cap - total
    case = {"R": R, "capacity": cap, "counts": counts, "offsets": offsets,
            "ray_idx": torch.cat([torch.repeat_interleave(torch.arange(R, dtype=torch.int32), counts.long()),
                                  torch.full((pad,), -1, dtype=torch.int32)]),
            "state": torch.zeros(R, dtype=torch.int32)}
    for k, v in chunks.items():
        x = torch.cat(v)
        case[k] = torch.cat([x, torch.full((pad,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype)])
    for k, v in per_ray.items():
        case[k] = torch.cat(v)
    case["gt_depth"] = case["gt_depth"].clamp_min(0.7)
    case["cov"] = torch.full((R,), 0.5)
    return case


# ------------------------------------------------------------------------------------------------------------------
# nvo_ngp_count_alive
# ------------------------------------------------------------------------------------------------------------------
ALIVE_THR = 1e-4
ALIVE_SENTINEL = 0x7FFFFFF0


def alive_reference(case, thr=ALIVE_THR, R_dev=None, counts=None, offsets=None, resume_in=None, carry_in=None, kept_base=0,
                    t_next=None, rounds=False, dtype=F64):
    """kept / state / resume_out / carry_out of one launch (header contract of nvo_ngp_alive_args); rows the launch leaves
    alone hold ALIVE_SENTINEL (kept, state) or NaN (resume_out, carry_out).  ``margin``: min |T / thr - 1| over the samples
    looked at.  carry_out of a ray that was cut is whatever the scan held and is returned as NaN (= not compared)."""
    R = case["R"]
    counts = case["counts"] if counts is None else counts
    offsets = case["offsets"] if offsets is None else offsets
    rec = _Rec()
    kept = torch.full((R,), ALIVE_SENTINEL, dtype=torch.int64)
    state = torch.full((R,), ALIVE_SENTINEL, dtype=torch.int64)
    resume_out, carry_out = torch.full((R,), float("nan"), dtype=dtype), torch.full((R,), float("nan"), dtype=dtype)
    margin = float("inf")
    for r in range(R if R_dev is None else min(R, R_dev)):
        if resume_in is not None and not float(resume_in[r]) >= 0.0:
            if rounds:
                resume_out[r] = -1.0
            continue
        n, base = int(counts[r]), int(offsets[r])
        dropped = n == 0 and int(offsets[r + 1]) != base
        sl = slice(base, base + n)
        c_in = torch.zeros((), dtype=dtype) if carry_in is None else carry_in[r].to(dtype)
        dd = torch.clamp(_exp(case["pre"][sl].to(dtype), rec) * case["dt"][sl].to(dtype), max=DD_CAP)
        incl = torch.cumsum(dd, 0) + c_in
        T = _exp(-(incl - dd), rec)
        below = torch.nonzero(T < thr)
        k = int(below[0]) if below.numel() else n
        margin = min(margin, threshold_margin(T[:min(k + 1, n)], thr))
        cut = k < n
        kept[r] = 0 if dropped else kept_base + k
        state[r] = 2 if dropped else (1 if cut else 0)
        if rounds:
            more = (not dropped) and (not cut) and t_next is not None and float(t_next[r]) >= 0.0
            resume_out[r] = float(t_next[r]) if more else -1.0
            if not cut:
                carry_out[r] = incl[-1] if n else c_in
    return {"kept": kept, "state": state, "resume_out": resume_out, "carry_out": carry_out, "margin": margin,
            "max_abs_x": rec.max_abs_x}


# (count, index of the first sample reached below the threshold | None, optical depth handed in)
ALIVE_RAYS = ((100, 63, 0.0), (100, 64, 0.0), (100, 65, 0.0), (130, None, 0.0), ("dropped", None, 0.0), ("empty", None, 0.0),
              (64, None, 0.0), (65, 64, 0.0), (200, 129, 0.0), (1, None, 0.0), (30, 0, 12.0), (64, 63, 0.0), (129, 128, 0.0),
              (40, 7, 0.0), (128, None, 2.0), (70, 1, 0.0))
ALIVE_PAST = 3  # rows behind R_dev


def alive_case(stride=1, seed=0):
    """Rays built to be cut at a stated index: thin samples (pre -8..-5) in front, one opaque sample (pre 6.5..7, dt 0.05:
    optical depth > 30) at index cut - 1, surface-like samples behind it.  ``pre`` is returned per slot; the tests lay it
    out with ``stride``.  The last ALIVE_PAST rays lie past R_dev."""
    g = torch.Generator().manual_seed(5200 + seed)
    rays = list(ALIVE_RAYS) + [(50, 20, 0.0)] * ALIVE_PAST
    R = len(rays)
    counts = torch.tensor([e[0] if isinstance(e[0], int) else 0 for e in rays], dtype=torch.int32)
    spans = torch.tensor([DROPPED_SLOTS if e[0] == "dropped" else (e[0] if isinstance(e[0], int) else 0) for e in rays])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(spans, 0)]).to(torch.int32)
    cap = (int(offsets[-1]) + 20 + 15) // 16 * 16
    pre, dt = torch.full((cap,), float("nan")), torch.full((cap,), float("nan"))
    carry_in = torch.tensor([e[2] for e in rays], dtype=F32)
    expect = torch.zeros(R, dtype=torch.int64)
    for r, (n, cut, _) in enumerate(rays):
        if not isinstance(n, int):
            continue
        base = int(offsets[r])
        p = -8.0 + 3.0 * torch.rand(n, generator=g)
        d = 0.005 + 0.045 * torch.rand(n, generator=g)
        if cut is not None and cut > 0:
            p[cut - 1] = 6.5 + 0.5 * torch.rand(1, generator=g)
            d[cut - 1] = 0.05
            p[cut:] = 2.0 + 4.0 * torch.rand(n - cut, generator=g)
        pre[base:base + n], dt[base:base + n] = p, d
        expect[r] = n if cut is None else cut
    cls = {"cut_at_0": sum(1 for e in rays[:-ALIVE_PAST] if e[1] == 0), "cut_at_63": sum(1 for e in rays if e[1] == 63),
           "cut_at_64": sum(1 for e in rays if e[1] == 64), "cut_at_65": sum(1 for e in rays if e[1] == 65),
           "never": sum(1 for e in rays if isinstance(e[0], int) and e[1] is None),
           "dropped": sum(1 for e in rays if e[0] == "dropped"), "empty": sum(1 for e in rays if e[0] == "empty"),
           "carry_in": int((carry_in > 0).sum())}
    return {"R": R, "R_dev": R - ALIVE_PAST, "capacity": cap, "stride": stride, "counts": counts, "offsets": offsets,
            "pre": _f16(pre), "dt": dt, "carry_in": carry_in, "expect": expect, "classes": cls}


ALIVE_ROUND = 64  # samples a round's march adds per ray


def alive_rounds(case):
    """The two rounds of a march with a budget of ALIVE_ROUND samples per ray and round, on the single-pass case: round
    one looks at the first min(n, 64) samples (t_next >= 0 where the ray has more), round two at the rest.  The ray cut at
    64 is the one whose transmittance falls below the threshold exactly BEHIND round one's last sample."""
    (c1, o1), (c2, o2) = split_rounds(case, ALIVE_ROUND)
    t_next = torch.where(case["counts"] > ALIVE_ROUND, 3.0 + torch.arange(case["R"]).float(), torch.full((case["R"],), -1.0))
    return {"counts": (c1, c2), "offsets": (o1, o2), "t_next": (t_next, torch.full((case["R"],), -1.0))}


# ------------------------------------------------------------------------------------------------------------------
# nvo_ngp_thickness, nvo_ngp_positions[_live]
# ------------------------------------------------------------------------------------------------------------------
THICKNESS_N = 777
THICKNESS_LEVELS = (0, 1, 2, 3, 4)


def thickness_case(seed=0):
    g = torch.Generator().manual_seed(6300 + seed)
    pre = (torch.rand(THICKNESS_N, generator=g) * 2 - 1) * 10.0
    pre[5], pre[300] = -float("inf"), FP16_MAX
    return {"n": THICKNESS_N, "pre": _f16(pre), "classes": {"neg_inf": 1, "fp16_max": 1}}


def thickness_reference(case, level, dtype=F64):
    """exp(pre) * sqrt(3) / 1024 * 2^level (the scale as the float32 constant the kernel holds)"""
    rec = _Rec()
    scale = float(np.float32(np.float32(1.7320508075688772) / np.float32(1024.0))) * 2.0 ** level
    out = _exp(case["pre"].to(dtype), rec) * torch.tensor(scale, dtype=dtype)
    return {"out": out, "max_abs_x": rec.max_abs_x}


POSITIONS_BOX = (-1.5, 2.5)
LIVE_CAPACITY = 12288
LIVE_N = (1, 4096, 4097)


def positions_case(capacity=1000, R=37, seed=0):
    """packed slots with ray_idx in [0, R) and blocks of ray_idx = -1; rays that leave the box on either side (samples
    clamp to exactly 0 and exactly 1); t / origins / directions of empty slots are NaN"""
    g = torch.Generator().manual_seed(7400 + seed)
    lo, hi = POSITIONS_BOX
    ray_idx = torch.randint(0, R, (capacity,), generator=g, dtype=torch.int32)
    ray_idx[capacity // 3: capacity // 3 + 41] = -1
    ray_idx[-7:] = -1
    t = 0.05 + 6.0 * torch.rand(capacity, generator=g)
    t[ray_idx < 0] = float("nan")
    origins = lo + 0.5 + (hi - lo - 1.0) * torch.rand(R, 3, generator=g)
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    inv = float(np.float32(1.0) / (np.float32(hi) - np.float32(lo)))  # what the launcher hands the kernel
    return {"capacity": capacity, "R": R, "ray_idx": ray_idx, "t": t, "origins": origins, "directions": directions,
            "lo": lo, "hi": hi, "inv": inv}


def positions_reference(case, dtype=F64):
    """x01 = clamp((o + d t - lo) * inv, 0, 1) on the float32 inputs (inv = the float32 1 / (hi - lo) of the launcher);
    zeros for ray_idx < 0"""
    ok = case["ray_idx"] >= 0
    r = case["ray_idx"].long().clamp_min(0)
    t = torch.where(ok, case["t"], torch.zeros_like(case["t"])).to(dtype)
    w = case["origins"].to(dtype)[r] + case["directions"].to(dtype)[r] * t[:, None]
    raw = (w - torch.tensor(float(np.float32(case["lo"])), dtype=dtype)) * torch.tensor(case["inv"], dtype=dtype)
    x = torch.where(ok[:, None], raw.clamp(0.0, 1.0), torch.zeros_like(raw))
    return {"x01": x, "raw": raw}


# ------------------------------------------------------------------------------------------------------------------
# nvo_ngp_rgb_fwd / nvo_ngp_rgb_bwd
# ------------------------------------------------------------------------------------------------------------------
HEAD_CAPACITY = 2048
HEAD_RAYS = 30
HEAD_EMPTY = ((100, 108), (1000, 1050))  # ray_idx = -1: inside one 16-row tile, and across tile borders


def rgb_head_case(seed=0):
    from oracle import mlp as M

    g = torch.Generator().manual_seed(8500 + seed)
    cap, R = HEAD_CAPACITY, HEAD_RAYS
    ray_idx = (R - 1 - torch.arange(cap) * R // cap).to(torch.int32)  # runs of slots per ray, as the packed layout has them
    for a, b in HEAD_EMPTY:
        ray_idx[a:b] = -1
    n_w = M.mlp_n_params(32, 3, 64, 2)
    weights = _f16(torch.randn(n_w, generator=g) * (1.5 / math.sqrt(64)))
    sh = _f16(torch.randn(R, 16, generator=g))
    density_out = _f16(torch.randn(cap, 16, generator=g))
    d_rgb = torch.randn(cap, 16, generator=g) * 0.05
    d_rgb[:, 3:] = 0.0  # (what the loss kernel writes)
    d_rgb[ray_idx < 0] = 0.0
    d_pre = torch.randn(cap, generator=g) * 0.3
    d_pre[ray_idx < 0] = 0.0
    return {"capacity": cap, "R": R, "ray_idx": ray_idx, "weights": weights, "sh": sh, "density_out": density_out,
            "d_rgb_out": _f16(d_rgb), "d_density_pre": d_pre, "n_weights": n_w,
            "classes": {"empty_rows": int((ray_idx < 0).sum()), "rays": len(set(ray_idx[ray_idx >= 0].tolist()))}}


def rgb_head_reference(case, with_d_pre=True, gather="ray_idx"):
    """oracle.mlp.mlp_forward (fp16 storage emulated) on [density_out row | SH16 row of ray_idx[row]] with a ZERO SH row
    where ray_idx < 0 (what the kernel's loader substitutes: such a row's output is the head of [density_out | 0], a
    specified value), and its autograd backward for the fp16 d_rgb_out: d_density_out (fp16-rounded sum of the input
    gradient's first 16 columns and, column 0, d_density_pre) and d_weights."""
    from oracle import mlp as M

    ok = case["ray_idx"] >= 0
    sh_rows = case["sh"].double()[case["ray_idx"].long().clamp_min(0)]
    sh_rows = torch.where(ok[:, None], sh_rows, torch.zeros_like(sh_rows))
    x = torch.cat([case["density_out"].double(), sh_rows], dim=1).requires_grad_(True)
    w = case["weights"].double().requires_grad_(True)
    out = M.mlp_forward(x, M.split_weights(w, 32, 3, 64, 2), "ReLU", "None", pad_value=1.0, emulate_fp16=True)
    (out * case["d_rgb_out"].double()).sum().backward()
    d_in = x.grad[:, :16].clone()
    plain = d_in.clone()
    if with_d_pre:
        d_in[:, 0] += case["d_density_pre"].double()
    return {"rgb_out": out.detach(), "d_density_out": d_in, "d_density_out_plain": plain, "d_weights": w.grad.clone()}


# ------------------------------------------------------------------------------------------------------------------
# e32: the float32 run of every reference against its float64 run, one figure per comparison of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def derived_factors(keys):
    """the ``factors`` block: every ..._capped comparison at CAPPED_FACTOR, with the reason"""
    return {k: {"factor": CAPPED_FACTOR, "reason": CAPPED_REASON} for k in keys if k.endswith("_capped")}


def _pair(fn):
    return fn(F64), fn(F32)


def e32_figures(with_x=False):
    """{key: e32}; with_x: also {key: largest |x| fed to an exponential}"""
    out, xs = {}, {}

    def put(key, r64, r32, q, x):
        out[key] = figure(r32[q], r64[q])
        xs[key] = x

    def put_all(prefix, r64, r32):
        for q in SAMPLE_QUANTITIES:
            put(f"{prefix}:{q}", r64, r32, q, r64["max_abs_x"])
        for q, v in ray_output_figures(r32, r64, r64["written"], r64["capped_ray"], RAY_OUTPUTS + RAY_LOSSES).items():
            out[f"{prefix}:{q}"] = v
            xs[f"{prefix}:{q}"] = r64["max_abs_x"]

    case = composite_case()
    for name, kw in COMPOSITE_VARIANTS.items():
        r64, r32 = _pair(lambda dt: composite_reference(case, True, kw, dt))
        put_all(f"composite/{name}", r64, r32)
    for world in RDEV_WORLDS:
        kw = dict(COMPOSITE_VARIANTS["bg-depth-cov-thr0"], R_dev=case["R"] - RDEV_SHORT, world_size=world)
        r64, r32 = _pair(lambda dt: composite_reference(case, True, kw, dt))
        put_all(f"composite/rdev-w{world}", r64, r32)
    kw = dict(background=False)
    r64, r32 = _pair(lambda dt: composite_reference(case, False, kw, dt))
    for cut in ROUND_CUTS:
        (c1, o1), _ = split_rounds(case, cut)
        h64, h32 = _pair(lambda dt: composite_reference(case, False, kw, dt, counts=c1, offsets=o1))
        put(f"rounds/cut{cut}:carry_first", h64, h32, "carry", h64["max_abs_x"])
        put(f"rounds/cut{cut}:carry", r64, r32, "carry", r64["max_abs_x"])
        for q, v in ray_output_figures(r32, r64, r64["written"], r64["capped_ray"]).items():
            out[f"rounds/cut{cut}:{q}"] = v
            xs[f"rounds/cut{cut}:{q}"] = r64["max_abs_x"]
    for stride in (1, 16):
        ac = alive_case(stride)
        a64, a32 = _pair(lambda dt: alive_reference(ac, R_dev=ac["R_dev"], carry_in=ac["carry_in"], rounds=True, dtype=dt))
        out[f"alive/s{stride}:carry_out"] = figure(torch.nan_to_num(a32["carry_out"]), torch.nan_to_num(a64["carry_out"]))
        xs[f"alive/s{stride}:carry_out"] = a64["max_abs_x"]
    ac = alive_case(1)
    rd = alive_rounds(ac)
    prev = {F64: None, F32: None}
    for k in (0, 1):
        res = {}
        for dt in (F64, F32):
            p = prev[dt]
            res[dt] = alive_reference(ac, counts=rd["counts"][k], offsets=rd["offsets"][k], t_next=rd["t_next"][k],
                                      resume_in=None if p is None else p["resume_out"], rounds=True,
                                      carry_in=None if p is None else torch.nan_to_num(p["carry_out"]).float(),
                                      kept_base=k * ALIVE_ROUND, dtype=dt)
        out[f"alive/rounds:carry_out{k + 1}"] = figure(torch.nan_to_num(res[F32]["carry_out"]), torch.nan_to_num(res[F64]["carry_out"]))
        xs[f"alive/rounds:carry_out{k + 1}"] = res[F64]["max_abs_x"]
        prev = res
    tc = thickness_case()
    for level in THICKNESS_LEVELS:
        t64, t32 = _pair(lambda dt: thickness_reference(tc, level, dt))
        fin = torch.isfinite(t64["out"])
        out[f"thickness/L{level}"] = figure(t32["out"][fin], t64["out"][fin])
        xs[f"thickness/L{level}"] = t64["max_abs_x"]
    pc = positions_case()
    p64, p32 = _pair(lambda dt: positions_reference(pc, dt))
    out["positions/x01"] = figure(p32["x01"], p64["x01"])
    lc = positions_case(LIVE_CAPACITY, seed=1)
    l64, l32 = _pair(lambda dt: positions_reference(lc, dt))
    out["positions/live"] = figure(l32["x01"], l64["x01"])
    return (out, xs) if with_x else out
