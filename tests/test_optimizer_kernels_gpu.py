"""The optimiser kernels of csrc/adam.hip through the C ABI, on buffers the tests own, against the float64 oracle of
helpers/adam_oracle.py on the inputs of helpers/adam_cases.py: every option of nvo_adam_step (weight decay, gradient
formats, loss scale, the three bias sources, the scalar and the 16-byte form, empty groups, the mixed working copy, skip
flags, the 4096-workgroup cap, the tail's average and commits), nvo_ema_update, nvo_opt_commit and the casts.

Bounds are not written here: a float comparison is bounded by 4 x e32 of its key in profiles/adam_parity_margins.json
(e32 = the oracle's float32 run against its float64 run, tests/helpers/adam_tolerances.py; the CPU suite holds the file to
a fresh computation), a key whose e32 is zero is an equality, the commit's bias pair may sit one fp32 ulp from numpy's
rounding of the double formula, a NaN must stay a NaN through a cast, and everything else is word equality.
NVO_ADAM_MEASURED=<file> records the kernel figures of the session.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from helpers import adam_cases as cases
from helpers import adam_oracle as A
from helpers import adam_tolerances as tol

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MEASURED, RECORDS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _record_measured():
    yield
    path = os.environ.get("NVO_ADAM_MEASURED")
    if path and MEASURED:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"figures": MEASURED, "records": RECORDS}, fh, indent=1)


@pytest.fixture(scope="module")
def margins():
    return A.load_margins()


def _abi():
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call

    return _lib, _call


def _st(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev(a, device):
    """numpy array -> device tensor (uint16 / uint32 words travel as int16 / int32)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(device)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32) if a.dtype == np.int32 else a


def _words(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _judge(key, got, ref, margins, failures):
    fig = A.figure(got, ref)
    bound = A.bound_for(key, margins)
    MEASURED[key] = fig
    print(f"{key:40s} figure {fig:.3e}  bound {bound:.3e}" + (f"  used {fig / bound:.2f}" if bound > 0.0 else "  (equality)"))
    if not fig <= bound:
        failures.append(f"{key}: figure {fig:.3e} > bound {bound:.3e}")


class Launch:
    """The device buffers of one case and one nvo_adam_step launch over them."""

    def __init__(self, c, device, tail=False, commit=None):
        lib, call = _abi()
        self.c, self.device = c, device
        n = c["n"]
        self.p, self.m, self.v = (_dev(c["state"][k], device) for k in ("p", "m", "v"))
        self.p16 = _dev(np.full(n, cases.P16_SENTINEL, np.uint16), device)
        self.g = _dev(c["grads"], device)
        self.flags = None if c["flags"] is None else _dev(np.array(c["flags"], np.uint32), device)
        self.scale = None if c["loss_scale"] is None else _dev(np.array([c["loss_scale"]], F32), device)
        self.keep = []
        k = len(c["ranges"])
        lo = (C.c_uint64 * max(k, 1))(*[r[0] for r in c["ranges"]])
        hi = (C.c_uint64 * max(k, 1))(*[r[1] for r in c["ranges"]])
        self.args = lib.AdamArgs(params=self.p.data_ptr(), params_half=self.p16.data_ptr(), grads=self.g.data_ptr(),
                                 grads_fmt=c["grads_fmt"], exp_avg=self.m.data_ptr(), exp_avg_sq=self.v.data_ptr(),
                                 beta1=c["beta1"], beta2=c["beta2"], eps=c["eps"], grad_scale=c["grad_scale"],
                                 skip_flags=None if self.flags is None else self.flags.data_ptr(),
                                 loss_scale_dev=None if self.scale is None else self.scale.data_ptr(), n_bf16_ranges=k,
                                 bf16_lo=C.cast(lo, C.c_void_p), bf16_hi=C.cast(hi, C.c_void_p))
        self.keep += [lo, hi]
        groups = []
        for g in c["groups"]:
            kind, val = g["bias"]
            hyper = bias = None
            if kind == "hyper":
                hyper = _dev(np.array(val, F32), device)
            elif kind == "bias":
                bias = _dev(np.array(val, F32), device)
            self.keep += [hyper, bias]
            groups.append(lib.AdamGroup(offset=g["offset"], n=g["n"], lr=g.get("host_lr", g["lr"]),
                                        step=val if kind == "step" else g.get("host_step", 1),
                                        hyper_dev=None if hyper is None else hyper.data_ptr(),
                                        bias_dev=None if bias is None else bias.data_ptr(), flag_slot=g["slot"],
                                        weight_decay=g["weight_decay"]))
        self.groups = (lib.AdamGroup * len(groups))(*groups)
        self.tail = None
        if c["ema"] is not None:
            # the average lives `shift` elements into its allocation: shift 1 takes the 16-byte form away from it
            s = c["shift"]
            self.ema_all = _dev(np.concatenate([np.zeros(s, F32), c["ema"]["values"]]), device)
            self.ema16_all = _dev(np.full(n + s, cases.P16_SENTINEL, np.uint16), device)
            self.ema, self.ema16 = self.ema_all[s:], self.ema16_all[s:]
            self.ema_step = _dev(np.array([c["ema"]["t0"]], np.uint32), device)
            self.done = _dev(np.zeros(1, np.uint32), device)
            self.tail = lib.AdamTail(ema=self.ema.data_ptr(), ema_half=self.ema16.data_ptr(), ema_decay=c["ema"]["decay"],
                                     ema_step_dev=self.ema_step.data_ptr(), ema_flag_slot=0, ema_commit=1 if tail else 0,
                                     done_counter=self.done.data_ptr() if tail else None)
            if commit is not None:   # (the commit must name the launch's own flag words)
                commit.skip_flags = self.flags.data_ptr()
                self.tail.commit = commit

    def run(self):
        _, call = _abi()
        call("nvo_adam_step", _st(self.device), C.byref(self.args), len(self.groups), self.groups,
             None if self.tail is None else C.byref(self.tail))
        torch.cuda.synchronize()
        return {"p": _host(self.p), "m": _host(self.m), "v": _host(self.v), "p16": _host(self.p16)}


def _covered(c, skipped=False):
    """mask of the elements the launch steps (or, skipped=True, of the elements of groups whose flag is raised)"""
    mask = np.zeros(c["n"], bool)
    for g in c["groups"]:
        raised = c["flags"] is not None and c["flags"][g["slot"]] != 0
        if raised == skipped:
            mask[g["offset"]:g["offset"] + g["n"]] = True
    return mask


def _check_step(family, device, margins, tail=False, commit=None):
    """one launch of a case against one oracle call: update, m, v (and the average) under the 4 x e32 rule; the working copy
    word for word from the kernel's own fp32 result; what no group steps keeps its bits"""
    c, ref = tol.reference(family)
    launch = Launch(c, device, tail=tail, commit=commit)
    got = launch.run()
    failures = []
    q = tol.quantities(c["state"]["p"], got)
    for name in ("update", "m", "v"):
        _judge(f"{family}:{name}", q[name], ref[name], margins, failures)
    stepped = _covered(c)
    want16 = np.where(stepped, A.working_copy(got["p"], c["ranges"]), np.uint16(cases.P16_SENTINEL))
    bad16 = np.flatnonzero(got["p16"] != want16)
    if bad16.size:
        failures.append(f"{family}: {bad16.size} words of the working copy differ, first at {bad16[0]}")
    for k in ("p", "m", "v"):
        if not np.array_equal(_words(got[k])[~stepped], _words(c["state"][k])[~stepped]):
            failures.append(f"{family}: {k} changed outside the stepped groups")
    if c["ema"] is not None:
        ema, ema16 = _host(launch.ema), _host(launch.ema16)
        _judge(f"{family}:ema", ema, ref["ema"], margins, failures)
        if not np.array_equal(_words(ema)[~stepped], _words(c["ema"]["values"])[~stepped]):
            failures.append(f"{family}: the average changed outside the stepped groups")
        want = np.where(stepped, A.to_words(ema, 1), np.uint16(cases.P16_SENTINEL))
        if not np.array_equal(ema16, want):
            failures.append(f"{family}: the fp16 copy of the average is not .half() of the average")
    assert not failures, "\n".join(failures)
    return c, launch, got


STEP_IDS = [n for n in cases.STEP_CASES if not n.startswith("engine-bias")]


@pytest.mark.parametrize("name", STEP_IDS)
def test_adam_step_options(device, margins, name):
    c, _, got = _check_step(f"step/{name}", device, margins)
    if name == "h":   # the flagged group kept every bit (checked above); the others moved
        moved = _words(got["p"]) != _words(c["state"]["p"])
        assert moved[_covered(c)].mean() > 0.9 and not moved[_covered(c, skipped=True)].any()


@pytest.mark.parametrize("t", (1, 2, 5, 1000))
def test_host_step_equals_committed_bias(device, t):
    """case d, the equality: a step through `step = t` and one through a bias_dev pair that nvo_opt_commit wrote at
    applied = t - 1 give identical words"""
    lib, call = _abi()
    c = cases.step_case(f"d-step{t}")
    host = Launch(c, device).run()
    applied = _dev(np.array([max(t - 2, 0)] * 3, np.uint32), device)
    bias = _dev(np.zeros(6, F32), device)
    args = lib.OptCommitArgs(n_groups=3, active_mask=0b111, scale_mask=0, applied=applied.data_ptr(), skip_flags=None, scale=None,
                             growth_tracker=None, bias=bias.data_ptr(), beta1=c["beta1"], beta2=c["beta2"])
    if t >= 2:
        call("nvo_opt_commit", _st(device), C.byref(args), None)
        torch.cuda.synchronize()
        pair = _host(bias).reshape(3, 2)
        assert list(_host(applied)) == [t - 1] * 3
    else:   # (no commit writes the pair of the first step: the engines initialise it on the host)
        pair = np.array([A.bias_pair(c["beta1"], c["beta2"], 1)] * 3, F32)
    for k, g in enumerate(c["groups"]):
        g["bias"] = ("bias", tuple(pair[k]))
    dev = Launch(c, device).run()
    for k in ("p", "m", "v", "p16"):
        assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), f"step {t}: {k}"


def test_eight_step_trajectory(device, margins):
    lib, call = _abi()
    c, ref, cs_ref = tol.trajectory_reference()
    p, m, v = (_dev(c["state"][k], device) for k in ("p", "m", "v"))
    flags = _dev(np.zeros(4, np.uint32), device)
    applied = _dev(np.zeros(2, np.uint32), device)
    bias = _dev(np.array([A.bias_pair(cases.BETA1, cases.BETA2, 1)] * 2, F32).ravel(), device)
    args = lib.AdamArgs(params=p.data_ptr(), params_half=None, grads=None, grads_fmt=0, exp_avg=m.data_ptr(),
                        exp_avg_sq=v.data_ptr(), beta1=cases.BETA1, beta2=cases.BETA2, eps=cases.EPS, grad_scale=1.0,
                        skip_flags=flags.data_ptr(), loss_scale_dev=None, n_bf16_ranges=0, bf16_lo=None, bf16_hi=None)
    groups = (lib.AdamGroup * 2)(*[lib.AdamGroup(offset=o, n=n, lr=lr, step=0, hyper_dev=None,
                                                 bias_dev=bias.data_ptr() + 8 * k, flag_slot=k, weight_decay=0.0)
                                   for k, (o, n, lr) in enumerate(cases.TRAJ_GROUPS)])
    commit = lib.OptCommitArgs(n_groups=2, active_mask=0b11, scale_mask=0, applied=applied.data_ptr(),
                               skip_flags=flags.data_ptr(), scale=None, growth_tracker=None, bias=bias.data_ptr(),
                               beta1=cases.BETA1, beta2=cases.BETA2)
    for s in range(1, cases.TRAJ_STEPS + 1):
        g = _dev(c["grads"][s - 1], device)
        flags.copy_(_dev(np.array([1, 1, 0, 0] if s == cases.TRAJ_SKIPPED else [0, 0, 0, 0], np.uint32), device))
        args.grads = g.data_ptr()
        call("nvo_adam_step", _st(device), C.byref(args), 2, groups, None)
        call("nvo_opt_commit", _st(device), C.byref(commit), None)
        torch.cuda.synchronize()
    got = {"p": _host(p), "m": _host(m), "v": _host(v)}
    failures = []
    q = tol.quantities(c["state"]["p"], got)
    for name in ("update", "m", "v"):
        _judge(f"trajectory:{name}", q[name], ref[name], margins, failures)
    assert not failures, "\n".join(failures)
    assert list(_host(applied)) == [7, 7] == cs_ref["applied"]
    # zero moments, no weight decay, a gradient that is zero in every step: the element keeps its bits
    stepped = np.zeros(cases.TRAJ_N, bool)
    for o, n, _ in cases.TRAJ_GROUPS:
        stepped[o:o + n] = True
    still = c["zero"] | ~stepped
    assert still[stepped].sum() > 100
    assert np.array_equal(_words(got["p"])[still], _words(c["state"]["p"])[still])
    assert not got["m"][still].any() and not got["v"][still].any()


def test_block_cap(device, margins):
    """one group of 4096 * 2048 + 3 * 2048 + 5 elements: past 4096 workgroups' worth, where the grid is capped and every
    thread strides through the range more than once (the main hash grid's path)"""
    assert -(-cases.CAP_N // 2048) > 4096
    _check_step("cap", device, margins)
    tol._cache.pop("cap", None)


@pytest.mark.parametrize("name", list(cases.TAIL_CASES))
def test_tail_average_and_commits(device, margins, name):
    lib, _ = _abi()
    c, _ = tol.reference(f"tail/{name}")
    flags = c["flags"]
    applied = _dev(np.array(cases.TAIL_APPLIED, np.uint32), device)
    bias_before = np.array([A.bias_pair(c["beta1"], c["beta2"], t + 1) for t in cases.TAIL_APPLIED], F32)
    bias = _dev(bias_before.ravel(), device)
    scale, tracker = _dev(np.array([1024.0], F32), device), _dev(np.array([1], np.uint32), device)
    sched = {"beta1": c["beta1"], "beta2": c["beta2"], "growth": 2.0, "backoff": 0.5, "interval": 2, "min_scale": 512.0,
             "max_scale": 4096.0}
    commit = lib.OptCommitArgs(n_groups=3, active_mask=0b111, scale_mask=0b111, applied=applied.data_ptr(), skip_flags=0,
                               scale=scale.data_ptr(), growth_tracker=tracker.data_ptr(), growth_factor=2.0,
                               backoff_factor=0.5, growth_interval=2, min_scale=512.0, max_scale=4096.0,
                               bias=bias.data_ptr(), beta1=c["beta1"], beta2=c["beta2"])

    _, launch, _ = _check_step(f"tail/{name}", device, margins, tail=True, commit=commit)
    want = A.commit({"applied": list(cases.TAIL_APPLIED), "bias": bias_before, "scale": F32(1024.0), "tracker": 1},
                    flags[:3], 0b111, 0b111, sched)
    assert list(_host(applied)) == want["applied"]
    assert float(_host(scale)[0]) == float(want["scale"]) and int(_host(tracker)[0]) == want["tracker"]
    got_bias = _host(bias).reshape(3, 2)
    ulps = np.abs(got_bias.view(np.int32).astype(np.int64) - want["bias"].view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, (got_bias, want["bias"])
    skipped = [k for k in range(3) if flags[k]]
    assert np.array_equal(got_bias[skipped].view(np.uint32), bias_before[skipped].view(np.uint32))
    assert int(_host(launch.done)[0]) == 0
    assert int(_host(launch.ema_step)[0]) == c["ema"]["t0"] + (0 if flags[0] else 1)


@pytest.mark.parametrize("decay,t0,shift", cases.EMA_GRID, ids=[f"d{d}-t{t}-s{s}" for d, t, s in cases.EMA_GRID])
def test_ema_update_alone(device, margins, decay, t0, shift):
    _, call = _abi()
    c, ref = tol.ema_reference(decay, t0, shift)
    n = cases.EMA_N
    p_all = _dev(np.concatenate([np.zeros(shift, F32), c["p"]]), device)
    e_all = _dev(np.concatenate([np.zeros(shift, F32), c["ema"]]), device)
    h_all = _dev(np.full(n + shift, cases.P16_SENTINEL, np.uint16), device)
    step = _dev(np.array([t0], np.uint32), device)
    p, e, h = p_all[shift:], e_all[shift:], h_all[shift:]
    call("nvo_ema_update", _st(device), n, p.data_ptr(), e.data_ptr(), h.data_ptr(), decay, step.data_ptr(), None, 1)
    torch.cuda.synchronize()
    failures = []
    got = _host(e)
    _judge(cases.ema_key(decay, t0, shift), got, ref, margins, failures)
    assert not failures, failures[0]
    assert np.array_equal(_host(h), A.to_words(got, 1))
    assert int(_host(step)[0]) == t0 + 1
    assert not _host(e_all)[:shift].any() and (_host(h_all)[:shift] == cases.P16_SENTINEL).all()


@pytest.mark.parametrize("preset", (0, 1, 9, 999, 29999))
def test_commit_bias_pair(device, preset):
    """the bias pair of the next applied step after one commit: the oracle's fp32 values, at most one ulp apart (the
    device's double pow need not round as numpy's does); the number of words that differ is recorded"""
    lib, call = _abi()
    applied = _dev(np.array([preset, preset + 1], np.uint32), device)
    bias = _dev(np.zeros(4, F32), device)
    args = lib.OptCommitArgs(n_groups=2, active_mask=0b11, scale_mask=0, applied=applied.data_ptr(), skip_flags=None, scale=None,
                             growth_tracker=None, bias=bias.data_ptr(), beta1=cases.BETA1, beta2=cases.BETA2)
    call("nvo_opt_commit", _st(device), C.byref(args), None)
    torch.cuda.synchronize()
    want = A.commit({"applied": [preset, preset + 1], "bias": np.zeros((2, 2), F32)}, None, 0b11, 0,
                    {"beta1": cases.BETA1, "beta2": cases.BETA2})
    assert list(_host(applied)) == want["applied"] == [preset + 1, preset + 2]
    got = _host(bias).reshape(2, 2)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want["bias"].view(np.int32).astype(np.int64))
    RECORDS[f"commit_bias/applied{preset}:words_differing"] = int((ulps != 0).sum())
    print(f"commit at applied = {preset}: {int((ulps != 0).sum())} of 4 words differ from numpy's rounding, largest {ulps.max()} ulp")
    assert ulps.max() <= 1, (got, want["bias"])


def test_commit_schedule_reaches_both_clamps(device):
    """16 commits from 1024 with min_scale 512, max_scale 4096, growth_interval 2; group 1 is in scale_mask only (its flag
    backs the scale off, its counter stands still), group 2 in active_mask only (its flag stops its counter, not the scale)"""
    lib, call = _abi()
    sched = {"beta1": cases.BETA1, "beta2": cases.BETA2, "growth": 2.0, "backoff": 0.5, "interval": 2, "min_scale": 512.0,
             "max_scale": 4096.0}
    active, in_scale = 0b101, 0b011
    # step -> flags of the three groups
    seq = {1: [1, 0, 0], 2: [0, 1, 0], 3: [1, 1, 0], 5: [0, 0, 1], 12: [0, 1, 1]}
    flags = _dev(np.zeros(4, np.uint32), device)
    applied = _dev(np.array([3, 5, 7], np.uint32), device)
    bias = _dev(np.zeros(6, F32), device)
    scale, tracker = _dev(np.array([1024.0], F32), device), _dev(np.zeros(1, np.uint32), device)
    args = lib.OptCommitArgs(n_groups=3, active_mask=active, scale_mask=in_scale, applied=applied.data_ptr(),
                             skip_flags=flags.data_ptr(), scale=scale.data_ptr(), growth_tracker=tracker.data_ptr(),
                             growth_factor=2.0, backoff_factor=0.5, growth_interval=2, min_scale=512.0, max_scale=4096.0,
                             bias=bias.data_ptr(), beta1=cases.BETA1, beta2=cases.BETA2)
    st = {"applied": [3, 5, 7], "bias": np.zeros((3, 2), F32), "scale": F32(1024.0), "tracker": 0}
    seen = []
    for s in range(1, 17):
        f = seq.get(s, [0, 0, 0])
        flags.copy_(_dev(np.array(f + [0], np.uint32), device))
        call("nvo_opt_commit", _st(device), C.byref(args), None)
        torch.cuda.synchronize()
        st = A.commit(st, f, active, in_scale, sched)
        assert list(_host(applied)) == st["applied"], s
        assert float(_host(scale)[0]) == float(st["scale"]) and int(_host(tracker)[0]) == st["tracker"], s
        seen.append(float(st["scale"]))
    # both clamps were reached by a product that passed them: 512 * 0.5 and 4096 * 2
    assert seen[:3] == [512.0, 512.0, 512.0] and seen[-1] == 4096.0 and seen.count(4096.0) >= 3
    assert st["applied"][1] == 5 and st["applied"][0] == 3 + 16 - 2 and st["applied"][2] == 7 + 16 - 2


# ---- casts ----------------------------------------------------------------------------------------------------------
def _assert_cast(got, src, fmt, what):
    """equality with torch's CPU conversion on every value that is not a NaN; a NaN stays a NaN"""
    want = A.to_words(src, fmt)
    nan = np.isnan(src)
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first src {src[bad[0]]!r} got {got[bad[0]]:#06x} want {want[bad[0]]:#06x}"
    assert np.isnan(A.from_words(got[nan], fmt)).all(), f"{what}: a NaN did not stay one"


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("fmt", (1, 2))
def test_cast_every_value(device, fmt, shift):
    _, call = _abi()
    vals = cases.bf16_values() if fmt == 2 else cases.fp16_values()
    src_all = _dev(np.concatenate([np.zeros(shift, F32), vals]), device)
    dst = _dev(np.full(vals.size, cases.P16_SENTINEL, np.uint16), device)
    call("nvo_cast_bf16" if fmt == 2 else "nvo_cast_half", _st(device), vals.size, src_all[shift:].data_ptr(), dst.data_ptr())
    torch.cuda.synchronize()
    _assert_cast(_host(dst), vals, fmt, f"cast fmt {fmt} shift {shift}")


@pytest.mark.parametrize("name", list(cases.RANGES))
def test_cast_working_copy(device, name):
    _, call = _abi()
    # both value sets, shuffled; the ranges of case g, with the last one moved to this buffer's end
    rng = cases.rng_of(f"wc-{name}")
    vals = rng.permutation(np.concatenate([cases.bf16_values(), cases.fp16_values()]))
    vals = vals[:vals.size // 4 * 4]
    ranges = [(vals.size - 1012, vals.size)] if name == "end" else cases.RANGES[name]
    src = _dev(vals, device)
    dst = _dev(np.full(vals.size, cases.P16_SENTINEL, np.uint16), device)
    k = len(ranges)
    lo, hi = (C.c_uint64 * max(k, 1))(*[r[0] for r in ranges]), (C.c_uint64 * max(k, 1))(*[r[1] for r in ranges])
    call("nvo_cast_working_copy", _st(device), vals.size, src.data_ptr(), dst.data_ptr(), k, C.cast(lo, C.c_void_p),
         C.cast(hi, C.c_void_p))
    torch.cuda.synchronize()
    got = _host(dst)
    bf = np.zeros(vals.size, bool)
    for a, b in ranges:
        bf[a:b] = True
    for fmt, mask in ((2, bf), (1, ~bf)):
        _assert_cast(got[mask], vals[mask], fmt, f"working copy {name} fmt {fmt}")


@pytest.mark.parametrize("dirty", (False, True), ids=("clean", "dirty"))
@pytest.mark.parametrize("world,pad", cases.SHARD_GRID)
@pytest.mark.parametrize("fmt", (1, 2))
def test_cast_shards(device, fmt, world, pad, dirty):
    _, call = _abi()
    src = cases.shard_source(fmt, world, dirty)
    want, want_flag = A.cast_shards(src, world, pad, fmt)
    assert want_flag == int(dirty)
    d_src = _dev(src, device)
    wire = _dev(np.full(want.size, cases.P16_SENTINEL, np.uint16), device)
    flag = _dev(np.zeros(1, np.uint32), device)
    call("nvo_cast_shards", _st(device), src.size, world, pad, d_src.data_ptr(), wire.data_ptr(), fmt, flag.data_ptr())
    torch.cuda.synchronize()
    assert int(_host(flag)[0]) == want_flag
    assert np.array_equal(_host(wire), want)   # (the sources are finite: no NaN allowance is needed)


@pytest.mark.parametrize("t", (1, 10, 100, 1000, 10000))
def test_engine_bias_pair_record(device, margins, t):
    """RECORD: how far a hyper_dev pair computed as engine.py computes it (Python doubles of 0.9 and 0.999) sits from the
    pair the commit writes (fp32 betas).  Asserted: the kernel, given the engine's pair, against the oracle given the same
    pair, under the 4 x e32 rule.  Recorded: the relative distance of the pairs and the update's figure against the oracle
    run with the commit's pair."""
    family = f"step/engine-bias-{t}"
    c, _, got = _check_step(family, device, margins)
    eng, com = cases.engine_pair(t), A.bias_pair(cases.BETA1, cases.BETA2, t)
    c2 = dict(c, groups=[dict(c["groups"][0], bias=("bias", com))])
    ref = tol.run_step(c2, F64)
    fig = A.figure(tol.quantities(c["state"]["p"], got)["update"], ref["update"])
    RECORDS[f"engine_bias/step{t}:bias1_rel"] = abs(float(eng[0]) - float(com[0])) / float(com[0])
    RECORDS[f"engine_bias/step{t}:bias2_sqrt_rel"] = abs(float(eng[1]) - float(com[1])) / float(com[1])
    RECORDS[f"engine_bias/step{t}:update_vs_commit_pair"] = fig
    print(f"engine pair at step {t}: {RECORDS[f'engine_bias/step{t}:bias1_rel']:.2e} / "
          f"{RECORDS[f'engine_bias/step{t}:bias2_sqrt_rel']:.2e} from the commit's; update {fig:.2e} "
          f"(bound of the same-pair comparison {A.bound_for(family + ':update', margins):.2e})")
