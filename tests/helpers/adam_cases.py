"""Seeded inputs of the optimiser-kernel parity tests, shared by tests/test_adam_oracle_cpu.py, tests/helpers/
adam_tolerances.py and tests/test_optimizer_kernels_gpu.py so that the CPU figures and the GPU run see the same numbers.
Every input is built on the CPU from one numpy generator per case (seeded with the case's name).

Gradient magnitudes AFTER the unscale are log-uniform, 1e-6 .. 10 where the moments start from seeded non-zero values and
1e-12 .. 10 where they start from zero (eps is 1e-15: any non-zero gradient becomes a full-size step), so that their
squares stay normal fp32 numbers; about 5 % are exact zeros.  Parameters are log-uniform in 1e-4 .. 1 with a random sign
(hash-table entries to MLP weights), so that the fp32 grid of the parameter does not hide the update.
"""
import zlib

import numpy as np

from helpers import adam_oracle as A

F32 = np.float32
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
ZERO_SHARE = 0.05
P16_SENTINEL = 0x1234   # what the 16-bit copies hold before a launch: an element no group covers keeps it


def rng_of(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def log_uniform(rng, n, lo, hi):
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(F32)


def gradients(rng, n, lo, zero_mask=None):
    g = log_uniform(rng, n, lo, 10.0)
    if zero_mask is None:
        zero_mask = rng.random(n) < ZERO_SHARE
    g[zero_mask] = 0.0
    return g


def state(rng, n, zero_moments=False):
    """p, m, v of a flat buffer; non-zero moments are those a history of gradients like the case's own would leave"""
    p = log_uniform(rng, n, 1e-4, 1.0)
    if zero_moments:
        return {"p": p, "m": np.zeros(n, F32), "v": np.zeros(n, F32)}
    prev = log_uniform(rng, n, 1e-6, 10.0)
    m = (prev * rng.uniform(0.05, 0.5, n)).astype(F32)
    v = (prev.astype(np.float64) ** 2 * rng.uniform(5e-4, 5e-3, n)).astype(F32)
    return {"p": p, "m": m, "v": v}


def group(offset, n, lr, wd=0.0, slot=0, bias=None):
    """bias defaults to the engines' source: a bias_dev pair as the commit leaves it (here: of applied step 3)"""
    bias = bias if bias is not None else ("bias", A.bias_pair(BETA1, BETA2, 3))
    return {"offset": offset, "n": n, "lr": lr, "weight_decay": wd, "slot": slot, "bias": bias}


# three groups with 16-byte-aligned starts, a tail of 3 each and one element behind each that no group covers
N_TOTAL = 40012
THREE = ((0, 20003), (20004, 12003), (32008, 8003))
LRS = (1e-2, 5e-3, 2e-2)
RANGES = {
    "none": [],
    "inside": [(1000, 3000)],
    "span": [(20000, 20012)],
    "four": [(8, 16), (20, 40), (20000, 20008), (32008, 33000)],   # fp16 gap of exactly 4 between the first two
    "end": [(39000, N_TOTAL)],
}


def _three(wd=(0.0, 0.0, 0.0), bias=None, slots=(0, 1, 2)):
    return [group(o, n, lr, w, s, bias) for (o, n), lr, w, s in zip(THREE, LRS, wd, slots)]


def _case(name, n=N_TOTAL, groups=None, lo=1e-6, zero_moments=False, **kw):
    rng = rng_of(name)
    c = {"name": name, "n": n, "state": state(rng, n, zero_moments), "groups": groups if groups is not None else _three(),
         "beta1": BETA1, "beta2": BETA2, "eps": EPS, "grad_scale": 1.0, "loss_scale": None, "grads_fmt": 0, "flags": None,
         "ranges": [], "ema": None, "shift": 0}
    c.update(kw)
    g = gradients(rng, n, lo)
    # the buffer holds the gradient times the loss scale the launch divides out again (powers of two: exact)
    scale = c["loss_scale"] if c["loss_scale"] is not None else 1.0 / c["grad_scale"]
    g = (g * F32(scale)).astype(F32)
    c["grads"] = A.to_words(g, c["grads_fmt"]) if c["grads_fmt"] else g
    if c["ema"] is not None:
        c["ema"] = dict(c["ema"], values=log_uniform(rng, n, 1e-4, 1.0))
    return c


def args_of(c):
    return {k: c[k] for k in ("beta1", "beta2", "eps", "grad_scale", "loss_scale", "grads_fmt", "flags")}


def engine_pair(t):
    """the pair engine.py puts into hyper_dev: Python doubles of 0.9 and 0.999, rounded to fp32"""
    import math

    return F32(1.0 - BETA1 ** t), F32(math.sqrt(1.0 - BETA2 ** t))


def _step_cases():
    b = {}
    b["a"] = lambda: _case("a", groups=_three(wd=(0.0, 1e-6, 1e-2)))
    for fmt in (0, 1, 2):
        b[f"b-fmt{fmt}"] = lambda fmt=fmt: _case(f"b-fmt{fmt}", grads_fmt=fmt, groups=_three(wd=(0.0, 1e-2, 0.0)))
    # (with weight decay: it joins the gradient AFTER the unscale, which only a scale other than 1 can show)
    b["c-host"] = lambda: _case("c-host", grad_scale=1.0 / 128.0, groups=_three(wd=(0.0, 1e-2, 1e-6)))
    # the device value must win: the host value next to it is another one
    b["c-dev"] = lambda: _case("c-dev", grad_scale=1.0 / 128.0, loss_scale=65536.0, groups=_three(wd=(0.0, 1e-2, 1e-6)))
    for t in (1, 2, 5, 1000):
        b[f"d-step{t}"] = lambda t=t: _case(f"d-step{t}", groups=_three(wd=(0.0, 1e-2, 0.0), bias=("step", t)))

    def hyper():
        gs = _three(wd=(0.0, 1e-2, 0.0))
        for k, g in enumerate(gs):   # the host lr / step next to the device values are other ones
            pair = A.bias_pair(BETA1, BETA2, 7 + 10 * k)
            g["bias"] = ("hyper", (F32(g["lr"]), pair[0], pair[1]))
            g["host_lr"], g["host_step"] = 0.5, 1
        return _case("d-hyper", groups=gs)

    def bias_dev():
        gs = _three(wd=(0.0, 1e-2, 0.0))
        for k, g in enumerate(gs):
            g["bias"] = ("bias", A.bias_pair(BETA1, BETA2, 2 + 30 * k))
            g["host_step"] = 1
        return _case("d-bias", groups=gs)

    b["d-hyper"], b["d-bias"] = hyper, bias_dev
    # group starts 0, 1, 2 and 3 modulo 4, bf16 ranges across the group boundaries
    b["e"] = lambda: _case("e", n=40011, groups=[group(0, 10001, 1e-2, 0.0, 0), group(10001, 10001, 5e-3, 1e-2, 1),
                                                 group(20002, 10001, 2e-2, 0.0, 2), group(30003, 10008, 1e-2, 1e-6, 3)],
                           ranges=[(9996, 10012), (20000, 20008), (30000, 30004), (40000, 40008)])
    # an empty group in the middle; 1, 3, 4, 5 elements; a second workgroup; every group its own lr / decay / slot
    b["f-1-0-3-2049"] = lambda: _case("f-1-0-3-2049", n=2060, groups=[
        group(0, 1, 1e-2, 0.0, 0), group(4, 0, 0.5, 0.5, 1), group(4, 3, 5e-3, 1e-2, 2), group(8, 2049, 2e-2, 1e-6, 3)])
    b["f-4-0-5-2049"] = lambda: _case("f-4-0-5-2049", n=2064, flags=[0, 0, 1, 0], groups=[
        group(0, 4, 1e-2, 1e-2, 0), group(4, 0, 0.5, 0.5, 1), group(4, 5, 5e-3, 0.0, 2), group(12, 2049, 2e-2, 1e-6, 3)])
    for name, r in RANGES.items():
        b[f"g-{name}"] = lambda name=name, r=r: _case(f"g-{name}", ranges=r, groups=_three(wd=(0.0, 1e-2, 0.0)))
    b["h"] = lambda: _case("h", flags=[0, 1, 0, 0], groups=_three(wd=(0.0, 1e-2, 0.0)), ranges=RANGES["span"],
                           ema={"decay": 0.95, "t0": 3})
    for t in (1, 10, 100, 1000, 10000):
        def eng(t=t):
            gs = [group(0, 4099, 1e-2, 0.0, 0)]
            pair = engine_pair(t)
            gs[0]["bias"] = ("hyper", (F32(1e-2), pair[0], pair[1]))
            return _case(f"engine-bias-{t}", n=4099, groups=gs)
        b[f"engine-bias-{t}"] = eng
    return b


STEP_CASES = _step_cases()
CAP_N = 4096 * 2048 + 3 * 2048 + 5
# name -> (preset of the average's counter, shift of the average's buffer in elements, skip flags)
TAIL_CASES = {"tail-t0": (0, 0, [0, 0, 0, 0]), "tail-t39": (39, 0, [0, 1, 0, 0]), "tail-t39-shifted": (39, 1, [0, 0, 0, 0])}
TAIL_DECAY = 0.95
TAIL_APPLIED = (4, 11, 0)
EMA_N = 4099
EMA_GRID = [(d, t0, s) for d in (0.0, 0.95, 0.99) for t0 in (0, 1, 39, 4999) for s in (0, 1)]


def step_case(name):
    return STEP_CASES[name]()


def cap_case():
    return _case("cap", n=CAP_N, groups=[group(0, CAP_N, 1e-2, 1e-2, 0)])


def tail_case(name):
    """one launch that carries the weight average and both commits: bias through bias_dev of applied counters"""
    t0, shift, flags = TAIL_CASES[name]
    gs = _three(wd=(0.0, 1e-2, 0.0))
    for k, g in enumerate(gs):
        g["bias"] = ("bias", A.bias_pair(BETA1, BETA2, TAIL_APPLIED[k] + 1))
    return _case(name, groups=gs, ema={"decay": TAIL_DECAY, "t0": t0}, shift=shift, flags=flags)


def ema_case(decay, t0, shift):
    rng = rng_of(f"ema-{decay}-{t0}-{shift}")
    return {"p": log_uniform(rng, EMA_N, 1e-4, 1.0), "ema": log_uniform(rng, EMA_N, 1e-4, 1.0)}


def ema_key(decay, t0, shift):
    return f"ema/d{decay}-t{t0}-s{shift}:ema"


# ---- the eight-step trajectory -------------------------------------------------------------------------------------
TRAJ_STEPS, TRAJ_SKIPPED = 8, 5
TRAJ_GROUPS = ((0, 3003, 1e-2), (3004, 2049, 5e-3))
TRAJ_N = 5056


def trajectory_case():
    rng = rng_of("trajectory")
    st = state(rng, TRAJ_N, zero_moments=True)
    zero = rng.random(TRAJ_N) < ZERO_SHARE   # the same elements in every step: they must keep their bits
    grads = [gradients(rng, TRAJ_N, 1e-12, zero) for _ in range(TRAJ_STEPS)]
    return {"state": st, "grads": grads, "zero": zero}


def trajectory_oracle(c, dtype):
    """the oracle's own trajectory: a commit behind every step, step TRAJ_SKIPPED skipped; returns (state, commit state)"""
    st = {k: v.astype(dtype) for k, v in c["state"].items()}
    cs = {"applied": [0, 0], "bias": [A.bias_pair(BETA1, BETA2, 1)] * 2, "scale": None, "tracker": 0}
    sched = {"beta1": BETA1, "beta2": BETA2}
    for s in range(1, TRAJ_STEPS + 1):
        flags = [1, 1, 0, 0] if s == TRAJ_SKIPPED else [0, 0, 0, 0]
        gs = [group(o, n, lr, 0.0, k, ("bias", tuple(cs["bias"][k]))) for k, (o, n, lr) in enumerate(TRAJ_GROUPS)]
        args = {"beta1": BETA1, "beta2": BETA2, "eps": EPS, "grad_scale": 1.0, "grads_fmt": 0, "flags": flags}
        st = A.adam_step(st, c["grads"][s - 1], gs, args, dtype)
        cs = A.commit(cs, flags[:2], 0b11, 0b11, sched)
    return st, cs


# ---- the value sets of the casts -----------------------------------------------------------------------------------
def bf16_values():
    """all 2^16 upper halves x six lower halves: every tie (0x8000), both neighbours of it, the extremes"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (hi[:, None] | lows[None, :]).reshape(-1).view(F32)


def bf16_ties(values):
    u = values.view(np.uint32)
    return np.isfinite(values) & ((u & 0xFFFF) == 0x8000)


def fp16_values():
    """every finite fp16 value as fp32 and its two fp32 neighbours; every midpoint of two adjacent fp16 values and the
    midpoint's two neighbours; the overflow threshold 65520 and values either side; 2^-25 (the tie between 0 and the
    smallest subnormal) and its upper neighbour; both infinities and a NaN"""
    w = np.arange(1 << 16, dtype=np.uint16)
    h = w.view(np.float16)
    fin = h[np.isfinite(h)].astype(F32)
    pos = np.sort(fin[fin >= 0])   # (+0 once more than needed is harmless; -0 stays in fin)
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) * 0.5).astype(F32)   # exact in fp32
    mid = np.concatenate([mid, -mid])

    def around(x):
        return np.concatenate([x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))])

    extra = np.array([65519.99, 65520.0, 65520.01, 2.0 ** -25, np.nextafter(F32(2.0 ** -25), F32(1.0)), np.inf, -np.inf,
                      np.nan], dtype=F32)
    return np.concatenate([around(fin), around(mid), extra]).astype(F32)


SHARD_N = 12 * 1024
SHARD_GRID = [(w, pad) for w in (1, 2, 3) for pad in (4, 8)]


def shard_source(fmt, world, dirty):
    """SHARD_N finite values of the format's set that stay inside the wire's limit; ``dirty``: one value just above it"""
    vals = bf16_values() if fmt == 2 else fp16_values()
    lim = F32(A.BF16_WIRE_MAX) if fmt == 2 else F32(A.FP16_MAX) / F32(world)
    with np.errstate(invalid="ignore"):
        ok = vals[np.abs(vals) <= lim]
    rng = rng_of(f"shards-{fmt}-{world}")
    src = rng.choice(ok, SHARD_N, replace=False).astype(F32)
    src[0], src[SHARD_N - 1] = lim, -lim   # exactly at the limit: clean
    if dirty:
        src[SHARD_N // 2 + 5] = np.nextafter(lim, F32(np.inf))
    return src
