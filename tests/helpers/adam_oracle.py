"""CPU restatement of the optimiser kernels of csrc/adam.hip (nvo_adam_step, nvo_ema_update, nvo_opt_commit and the casts),
in float64 and in float32, for tests/test_optimizer_kernels_gpu.py and tests/test_adam_oracle_cpu.py.  No GPU needed.

Every hyper-parameter enters as the fp32 value the C ABI carries, widened: beta2 is 0.99900001287..., not 0.999, and
1 - beta is taken in fp32 as the kernel takes it.  The float32 run performs every operation of nvo_adam_one in float32, one
rounding each (the library is built with -ffp-contract=off, so no fused form is needed); the float64 run performs the same
expressions in float64 on the same fp32 inputs.  Bias corrections of a host `step` are the double formula on the fp32 betas,
rounded to fp32 (what nvo_opt_commit writes), in BOTH runs, so that the float32 error holds the chain and nothing else.
"""
import json
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARGINS_PATH = os.path.join(ROOT, "profiles", "adam_parity_margins.json")
FACTOR = 4.0
F32, F64 = np.float32, np.float64


def f32(x) -> float:
    """the fp32 value the ABI carries, as a Python double"""
    return float(np.float32(x))


def figure(got, ref) -> float:
    """max|got - ref| / max|ref|; plain max|got - ref| where ref is all zero; inf when got holds a non-finite value"""
    got, ref = np.asarray(got, F64).ravel(), np.asarray(ref, F64).ravel()
    if ref.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = float(np.abs(got - ref).max())
    top = float(np.abs(ref).max())
    return err / top if top > 0.0 else err


def load_margins(path: str = MARGINS_PATH) -> dict:
    with open(path) as fh:
        return json.load(fh)


def bound_for(key: str, margins: dict) -> float:
    """4 x e32, no floor: a quantity whose e32 is exactly zero is compared for equality"""
    return FACTOR * margins["e32"][key]


# ------------------------------------------------------------------------------------------------------------------
# 16-bit formats (torch's CPU conversions are the reference of every cast)
# ------------------------------------------------------------------------------------------------------------------
def to_words(x32, fmt: int) -> np.ndarray:
    """fp32 -> the raw 16-bit words of fp16 (fmt 1) or bfloat16 (fmt 2), by torch's CPU conversion"""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32))
    t = t.to(torch.bfloat16) if fmt == 2 else t.half()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def from_words(words, fmt: int) -> np.ndarray:
    """raw 16-bit words -> fp32 (exact in both formats)"""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    if fmt == 2:
        return (w.astype(np.uint32) << 16).view(F32)
    return w.view(np.float16).astype(F32)


def working_copy(p32, ranges) -> np.ndarray:
    """the 16-bit working copy of a flat fp32 buffer: bfloat16 inside the [lo, hi) ranges, fp16 elsewhere (raw words)"""
    p32 = np.ascontiguousarray(p32, dtype=F32)
    out = to_words(p32, 1)
    bf = to_words(p32, 2)
    for lo, hi in ranges:
        hi = min(hi, p32.size)
        out[lo:hi] = bf[lo:hi]
    return out


# ------------------------------------------------------------------------------------------------------------------
# nvo_adam_step
# ------------------------------------------------------------------------------------------------------------------
def bias_pair64(beta1, beta2, t):
    """{1 - beta1^t, sqrt(1 - beta2^t)} in double on the fp32 betas"""
    b1, b2 = f32(beta1), f32(beta2)
    return 1.0 - b1 ** float(t), math.sqrt(1.0 - b2 ** float(t))


def bias_pair(beta1, beta2, t):
    """the same, rounded to fp32: what opt_commit_thread writes for an applied step t"""
    a, b = bias_pair64(beta1, beta2, t)
    return F32(a), F32(b)


def group_hyper(group, args):
    """(lr, bias1, bias2_sqrt) of one group as fp32 values: host step < hyper_dev < bias_dev, as k_adam_groups reads them"""
    kind, val = group["bias"]
    lr = F32(group["lr"])
    if kind == "step":
        b1, b2s = bias_pair(args["beta1"], args["beta2"], val)
    elif kind == "hyper":
        lr, b1, b2s = F32(val[0]), F32(val[1]), F32(val[2])
    elif kind == "bias":
        b1, b2s = F32(val[0]), F32(val[1])
    else:
        raise ValueError(kind)
    return lr, b1, b2s


def adam_one(p, m, v, g, h, dtype):
    """nvo_adam_one (csrc/nvo_common.h), expression by expression; h = fp32 scalars, widened to ``dtype``"""
    c = {k: dtype(x) for k, x in h.items()}
    gi = g * c["grad_scale"]
    if h["weight_decay"] != 0.0:
        gi = gi + c["weight_decay"] * p
    m = c["beta1"] * m + c["one_minus_beta1"] * gi
    v = c["beta2"] * v + c["one_minus_beta2"] * gi * gi
    denom = np.sqrt(v) / c["bias2_sqrt"] + c["eps"]
    p = p - (c["lr"] / c["bias1"]) * (m / denom)
    return p, m, v


def grad_scale_of(args) -> np.float32:
    """the factor of the unscale: 1 / *loss_scale_dev (fp32 division) when a device loss scale is given, else grad_scale"""
    if args.get("loss_scale") is not None:
        return F32(1.0) / F32(args["loss_scale"])
    return F32(args.get("grad_scale", 1.0))


def adam_step(state, grads, groups, args, dtype):
    """One nvo_adam_step launch.  state: {"p", "m", "v"} flat arrays (any float type; used as ``dtype``); grads: the flat
    gradient buffer, fp32 values or -- args["grads_fmt"] 1 / 2 -- the raw 16-bit words the kernel reads; groups: dicts
    {offset, n, lr, weight_decay, slot, bias: ("step", t) | ("hyper", (lr, bias1, bias2_sqrt)) | ("bias", (bias1,
    bias2_sqrt))}; args: {beta1, beta2, eps, grad_scale | loss_scale, grads_fmt, flags}.  Returns the new state in
    ``dtype``; a group whose flag word is raised keeps its values."""
    fmt = args.get("grads_fmt", 0)
    g32 = from_words(grads, fmt) if fmt else np.asarray(grads, dtype=F32)
    out = {k: np.array(state[k], dtype=dtype) for k in ("p", "m", "v")}
    flags = args.get("flags")
    b1, b2 = F32(args["beta1"]), F32(args["beta2"])
    for gr in groups:
        o, n = gr["offset"], gr["n"]
        if n == 0 or (flags is not None and flags[gr["slot"]] != 0):
            continue
        lr, bias1, bias2s = group_hyper(gr, args)
        h = {"lr": lr, "beta1": b1, "beta2": b2, "one_minus_beta1": F32(1.0) - b1, "one_minus_beta2": F32(1.0) - b2,
             "eps": F32(args["eps"]), "bias1": bias1, "bias2_sqrt": bias2s, "grad_scale": grad_scale_of(args),
             "weight_decay": F32(gr.get("weight_decay", 0.0))}
        s = slice(o, o + n)
        out["p"][s], out["m"][s], out["v"][s] = adam_one(out["p"][s], out["m"][s], out["v"][s], g32[s].astype(dtype), h,
                                                         dtype)
    return out


# ------------------------------------------------------------------------------------------------------------------
# nvo_ema_update (and the average inside nvo_adam_tail)
# ------------------------------------------------------------------------------------------------------------------
def ema_factors(decay, t):
    """(keep, take, inv_debias) of k_ema_update for the t-th average: keep and inv_debias in double on the fp32 decay,
    take = 1 - decay in fp32"""
    d = f32(decay)
    keep = d * (1.0 - d ** float(t - 1))
    inv = 1.0 / (1.0 - d ** float(t))
    return keep, float(F32(1.0) - F32(decay)), inv


def ema_update(ema, p, decay, t, dtype):
    """ema_t = (ema * keep + p * take) * inv_debias, t = averages applied so far + 1.  The float32 run rounds keep and
    inv_debias to fp32, as the kernel does."""
    keep, take, inv = ema_factors(decay, t)
    if dtype == F32:
        keep, inv = F32(keep), F32(inv)
    e, p = np.asarray(ema, dtype=dtype), np.asarray(p, dtype=dtype)
    return (e * dtype(keep) + p * dtype(take)) * dtype(inv)


# ------------------------------------------------------------------------------------------------------------------
# nvo_opt_commit
# ------------------------------------------------------------------------------------------------------------------
def commit(state, flags, active_mask, scale_mask, schedule):
    """opt_commit_thread.  state: {"applied": [n_groups] ints, "bias": [n_groups][2] fp32, "scale": fp32 | None,
    "tracker": int}; flags: [n_groups] ints or None; schedule: {beta1, beta2, growth, backoff, interval, min_scale,
    max_scale}.  Returns the new state; "bias64" holds the pairs in double before their rounding."""
    n = len(state["applied"])
    out = {"applied": list(state["applied"]), "bias": np.array(state["bias"], dtype=F32).reshape(n, 2).copy(),
           "bias64": np.array(state.get("bias64", state["bias"]), dtype=F64).reshape(n, 2).copy(),
           "scale": state.get("scale"), "tracker": state.get("tracker", 0)}
    any_bad = False
    for i in range(n):
        bad = flags is not None and flags[i] != 0
        if (scale_mask >> i) & 1:
            any_bad = any_bad or bad
        if ((active_mask >> i) & 1) and not bad:
            out["applied"][i] += 1
            pair = bias_pair64(schedule["beta1"], schedule["beta2"], out["applied"][i] + 1)
            out["bias64"][i] = pair
            out["bias"][i] = (F32(pair[0]), F32(pair[1]))
    if out["scale"] is not None:
        sc, tr = F32(out["scale"]), int(out["tracker"])
        if any_bad:
            sc = max(sc * F32(schedule["backoff"]), F32(schedule["min_scale"]))
            tr = 0
        else:
            tr += 1
            if tr >= schedule["interval"]:
                sc = min(sc * F32(schedule["growth"]), F32(schedule["max_scale"]))
                tr = 0
        out["scale"], out["tracker"] = F32(sc), tr
    return out


# ------------------------------------------------------------------------------------------------------------------
# nvo_cast_shards
# ------------------------------------------------------------------------------------------------------------------
FP16_MAX = 65504.0
BF16_WIRE_MAX = 3.0e38


def cast_shards(src, world, pad, fmt):
    """The wire buffer of the sharded exchange: wire[(i / per) * (per + pad) + i % per] = cvt(src[i]), every pad slot
    flag ? 1.0 : 0 in the wire format.  The flag is raised by a non-finite value or, on the fp16 wire, |v| > 65504 / world
    (fp32 division); on the bf16 wire by not |v| <= 3.0e38.  Returns (words, flag)."""
    src = np.ascontiguousarray(src, dtype=F32)
    n = src.size
    per = n // world
    lim = F32(BF16_WIRE_MAX) if fmt == 2 else F32(FP16_MAX) / F32(world)
    with np.errstate(invalid="ignore"):
        flag = int(bool((~(np.abs(src) <= lim)).any()))
    wire = np.zeros(world * (per + pad), dtype=np.uint16)
    i = np.arange(n)
    wire[(i // per) * (per + pad) + i % per] = to_words(src, fmt)
    one = 0x3F80 if fmt == 2 else 0x3C00
    for w in range(world):
        wire[w * (per + pad) + per:(w + 1) * (per + pad)] = one if flag else 0
    return wire, flag
