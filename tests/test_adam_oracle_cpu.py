"""The optimiser oracle (tests/helpers/adam_oracle.py) against independent statements of the same rules, and the figures
the GPU tests take their bounds from (profiles/adam_parity_margins.json) against a fresh computation.  No GPU."""
import numpy as np
import pytest
import torch

from helpers import adam_cases as cases
from helpers import adam_oracle as A
from helpers import adam_tolerances as tol

F32, F64 = np.float32, np.float64


def test_float64_oracle_matches_torch_adam():
    """Ten steps over two parameter groups with their own lr and weight decay: torch.optim.Adam on float64 CPU tensors,
    given the fp32-rounded hyper-parameters the oracle uses.  Largest relative difference of the parameters measured:
    see the printed figure (expected near 1e-13); asserted 1e-10."""
    rng = cases.rng_of("torch-adam")
    n0, n1 = 1501, 1003
    groups = [cases.group(0, n0, 1e-2, 1e-2, 0), cases.group(n0, n1, 1e-4, 1e-6, 1)]
    st = {k: v.astype(F64) for k, v in cases.state(rng, n0 + n1, zero_moments=True).items()}
    params = [torch.from_numpy(st["p"][:n0].copy()).requires_grad_(True), torch.from_numpy(st["p"][n0:].copy()).requires_grad_(True)]
    # (1.f - beta is exact in fp32 for both betas, so torch's double complement of the fp32 beta is the kernel's value;
    # what torch does not share with the ABI is the ROUNDING of the bias pair to fp32: it gets the unrounded pair here)
    b1, b2 = A.f32(cases.BETA1), A.f32(cases.BETA2)
    opt = torch.optim.Adam([{"params": [params[k]], "lr": A.f32(g["lr"]), "weight_decay": A.f32(g["weight_decay"])}
                            for k, g in enumerate(groups)], betas=(b1, b2), eps=A.f32(cases.EPS))
    args = {"beta1": cases.BETA1, "beta2": cases.BETA2, "eps": cases.EPS, "grad_scale": 1.0, "grads_fmt": 0, "flags": None}
    for step in range(1, 11):
        g = cases.gradients(rng, n0 + n1, 1e-6)
        for gr in groups:
            gr["bias"] = ("bias", A.bias_pair64(cases.BETA1, cases.BETA2, step))   # (unrounded: torch's are doubles too)
        st = _adam_step_unrounded_bias(st, g, groups, args)
        params[0].grad = torch.from_numpy(g[:n0].astype(F64))
        params[1].grad = torch.from_numpy(g[n0:].astype(F64))
        opt.step()
    got = np.concatenate([p.detach().numpy() for p in params])
    rel = float(np.abs(st["p"] - got).max() / np.abs(got).max())
    print(f"float64 oracle against torch.optim.Adam, 10 steps, 2 groups: {rel:.3e}")
    assert rel <= 1e-10


def _adam_step_unrounded_bias(st, g, groups, args):
    """A.adam_step in float64 with the bias pair left in double, as torch keeps it: the expressions are A.adam_one's
    own and the other scalars the ABI's fp32 values."""
    out = {k: v.copy() for k, v in st.items()}
    b1, b2 = A.f32(args["beta1"]), A.f32(args["beta2"])
    for gr in groups:
        s = slice(gr["offset"], gr["offset"] + gr["n"])
        h = {"lr": A.f32(gr["lr"]), "beta1": b1, "beta2": b2, "one_minus_beta1": F32(1.0) - F32(b1),
             "one_minus_beta2": F32(1.0) - F32(b2), "eps": A.f32(args["eps"]), "bias1": gr["bias"][1][0], "bias2_sqrt": gr["bias"][1][1], "grad_scale": 1.0,
             "weight_decay": A.f32(gr["weight_decay"])}
        out["p"][s], out["m"][s], out["v"][s] = A.adam_one(out["p"][s], out["m"][s], out["v"][s], g[s].astype(F64), h, F64)
    return out


def test_abi_complements_are_what_the_kernel_takes():
    """adam_step feeds adam_one the fp32 difference 1.f - beta (0.100000024 and 0.00099998713), not the double one"""
    seen = {}
    real = A.adam_one

    def spy(p, m, v, g, h, dtype):
        seen.update(h)
        return real(p, m, v, g, h, dtype)

    A.adam_one = spy
    try:
        c = cases.step_case("f-1-0-3-2049")
        A.adam_step(c["state"], c["grads"], c["groups"], cases.args_of(c), F64)
    finally:
        A.adam_one = real
    assert seen["one_minus_beta1"] == F32(1.0) - F32(0.9) and seen["one_minus_beta2"] == F32(1.0) - F32(0.999)
    assert float(seen["beta2"]) == A.f32(0.999) != 0.999


def _grad_scaler_update(scale, tracker, found_inf, growth, backoff, interval):
    """torch.cuda.amp.GradScaler.update (torch._amp_update_scale_), restated"""
    if found_inf:
        return scale * backoff, 0
    tracker += 1
    if tracker == interval:
        return scale * growth, 0
    return scale, tracker


def test_schedule_matches_grad_scaler_and_reaches_both_clamps():
    sched = {"beta1": cases.BETA1, "beta2": cases.BETA2, "growth": 2.0, "backoff": 0.5, "interval": 2, "min_scale": 512.0,
             "max_scale": 4096.0}
    bad_steps = {1, 2, 3, 12}   # 1024 -> 512 (clamped twice) ... then eight clean steps: up to 4096 and clamped there
    st = {"applied": [0], "bias": [A.bias_pair(0.9, 0.999, 1)], "scale": F32(1024.0), "tracker": 0}
    scale, tracker, seen = 1024.0, 0, set()
    for s in range(1, 17):
        bad = s in bad_steps
        st = A.commit(st, [int(bad)], 1, 1, sched)
        scale, tracker = _grad_scaler_update(scale, tracker, bad, 2.0, 0.5, 2)
        if scale < 512.0:
            scale = 512.0
            seen.add("min")
        if scale > 4096.0:
            scale = 4096.0
            seen.add("max")
        assert (float(st["scale"]), st["tracker"]) == (scale, tracker), s
    assert seen == {"min", "max"} and st["applied"] == [16 - len(bad_steps)]


def test_recorded_e32_is_what_the_oracle_gives():
    rec = A.load_margins()["e32"]
    now = tol.e32_figures()
    assert set(rec) == set(now)
    for key, v in now.items():
        assert rec[key] == pytest.approx(v, rel=1e-6, abs=0.0), key


def test_every_comparison_has_a_measured_figure():
    m = A.load_margins()
    assert set(m["measured_gfx950"]) == set(m["e32"])


def test_cast_value_sets():
    bf = cases.bf16_values()
    assert bf.size == 393216
    fin = np.isfinite(bf)
    assert int(fin.sum()) >= 390000 and int(cases.bf16_ties(bf).sum()) >= 65000
    # six finite values round to infinity: the class of the source is not the class of the result
    words = A.to_words(bf, 2)
    assert int((fin & ((words & 0x7FFF) == 0x7F80)).sum()) == 6
    h = cases.fp16_values()
    assert 380000 <= h.size <= 383000
    assert np.isnan(h).sum() == 1 and np.isinf(h).sum() == 2
    # the midpoints are ties of the fp16 grid: both neighbours round apart
    w = A.to_words(h, 1)
    assert np.unique(w[np.isfinite(h)]).size >= 63488


def test_cast_shards_layout():
    src = cases.shard_source(1, 3, dirty=False)
    wire, flag = A.cast_shards(src, 3, 8, 1)
    per = cases.SHARD_N // 3
    assert flag == 0 and wire.size == 3 * (per + 8)
    assert np.array_equal(wire[per + 8:per + 8 + per], A.to_words(src[per:2 * per], 1)) and not wire[per:per + 8].any()
    wire, flag = A.cast_shards(cases.shard_source(1, 3, dirty=True), 3, 8, 1)
    assert flag == 1 and (wire[per:per + 8] == 0x3C00).all()
    assert np.isfinite(A.from_words(wire, 1)).all()   # (the dirty value is finite on the wire: only the limit catches it)


def test_working_copy_ranges():
    p = cases.log_uniform(cases.rng_of("wc"), 64, 1e-4, 1.0)
    w = A.working_copy(p, [(8, 16), (20, 40)])
    bf, h = A.to_words(p, 2), A.to_words(p, 1)
    want = h.copy()
    want[8:16], want[20:40] = bf[8:16], bf[20:40]
    assert np.array_equal(w, want) and not np.array_equal(bf[16:20], h[16:20])


def test_cases_stay_inside_their_buffers():
    """what the GPU tests launch: every group inside its buffer, at most four groups, bf16 bounds multiples of 4"""
    built = [cases.step_case(n) for n in cases.STEP_CASES] + [cases.tail_case(n) for n in cases.TAIL_CASES]
    for c in built:
        assert 1 <= len(c["groups"]) <= 4 and c["grads"].size == c["n"] == c["state"]["p"].size
        for g in c["groups"]:
            assert 0 <= g["offset"] and g["offset"] + g["n"] <= c["n"] and g["slot"] < 4
        for lo, hi in c["ranges"]:
            assert lo % 4 == 0 and hi % 4 == 0 and lo <= hi <= c["n"]
        assert len(c["ranges"]) <= 4
    assert max(o + n for o, n, _ in cases.TRAJ_GROUPS) <= cases.TRAJ_N
    # the scalar form, the tail after n >> 2, a second workgroup and a second trip through the grid-stride loop are all there
    e = cases.step_case("e")
    assert sorted(g["offset"] % 4 for g in e["groups"]) == [0, 1, 2, 3]
    a = cases.step_case("a")["groups"]   # ceil(n / 2048) workgroups of 256 threads x 4 elements cover less than n
    assert all(g["n"] > -(-g["n"] // 2048) * 1024 and g["n"] % 4 == 3 and g["offset"] % 4 == 0 for g in a)
