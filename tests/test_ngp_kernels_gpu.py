"""Kernel-level float64 parity of the occupancy-grid back-end's per-ray and per-sample kernels: nvo_ngp_composite_loss
(both training forms, inference, inference in rounds), nvo_ngp_count_alive (single pass and rounds), nvo_ngp_thickness,
nvo_ngp_positions[_live] and the rgb head nvo_ngp_rgb_fwd / nvo_ngp_rgb_bwd, each driven through the C ABI on synthetic
tensors and held to the restatements of tests/helpers/ngp_oracle.py.  No engine, no marcher, no hash grid.

Figure: max|got - ref64| / max|ref64| per comparison.  Bound: factor * e32 + 1e-6 with factor 4 and e32 the same figure of
the float32 run of the SAME oracle function on the same inputs, measured on the CPU with the device's formulation of
__expf (profiles/ngp_parity_margins.json, written by tests/helpers/ngp_tolerances.py, guarded by
tests/test_ngp_oracle_cpu.py).  d_rgb_out is stored as fp16: it is judged elementwise with half an fp16 ulp of the
reference added.  The rgb head keeps the fused MLP's own tolerances (the f16 row of test_tcnn_gpu.test_network_fwd_bwd).
Output buffers are pre-filled: NaN where the contract is "overwritten", a known exact pattern where it is "added to".
NVO_NGP_MEASURED=<file> records the kernel figures of the session.
"""
import ctypes as C
import json
import os

import pytest
import torch

from helpers import ngp_oracle as N

pytestmark = pytest.mark.gpu

MEASURED = {}
_MARGINS = None
NAN = float("nan")
F16 = torch.float16


@pytest.fixture(scope="module", autouse=True)
def _record_measured():
    yield
    path = os.environ.get("NVO_NGP_MEASURED")
    if path and MEASURED:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1)


def _abi():
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call, _ptr, _stream

    return _lib, _call, _ptr, _stream


def _margins():
    global _MARGINS
    if _MARGINS is None:
        _MARGINS = N.load_margins()
    return _MARGINS


def _judge(key, fig):
    bound = N.bound_for(key, _margins())
    MEASURED[key] = max(fig, MEASURED.get(key, 0.0))
    print(f"{key}: figure {fig:.3e} bound {bound:.3e} (e32 {_margins()['e32'][key]:.3e})")
    return [] if fig <= bound else [f"{key}: {fig:.3e} > {bound:.3e}"]


def _hold(key, got, ref):
    """assert figure(got, ref) <= bound of ``key``; every figure is printed and recorded before it is judged."""
    return _judge(key, N.figure(torch.as_tensor(got).detach().cpu(), ref))


def _hold_rays(prefix, got, ref):
    """the per-ray outputs against the oracle; rays that hold a capped sample under keys of their own (N.CAPPED_FACTOR)"""
    assert torch.isfinite(torch.cat([got[q][ref["written"]].reshape(-1) for q in N.RAY_OUTPUTS])).all()
    fails = []
    for q, fig in N.ray_output_figures(got, ref, ref["written"], ref["capped_ray"]).items():
        fails += _judge(f"{prefix}:{q}", fig)
    return fails


def _hold_fp16(key, got, ref):
    """the elementwise rule of an fp16 output: |got - ref| <= bound * max|ref| + half an fp16 ulp of ref"""
    got, ref = got.detach().cpu().double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return _judge(key, float("inf"))
    scale = float(ref.abs().max())
    over = ((got - ref).abs() - N.half_ulp_fp16(ref)).clamp_min(0.0)
    return _judge(key, float(over.max()) / scale if scale > 0 else float(over.max()))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == F16 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_zero_bits(t):
    return not bool(_bits(t).any())


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _pattern(shape, seed=0, unit=2.0 ** -16):
    """a known non-zero pre-fill for outputs that are added to: +-k * unit, k = 1..31 (exact in float32, and small enough
    that the value added on top keeps its own precision)"""
    g = torch.Generator().manual_seed(99 + seed)
    return torch.randint(1, 32, shape, generator=g).float() * unit * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


def _strided(values, stride):
    """fp16 [n][stride] with ``values`` ([n] or [n][k]) in the first columns and NaN in every other one"""
    v = values if values.dim() == 2 else values[:, None]
    out = torch.full((v.shape[0], stride), NAN, dtype=F16)
    out[:, :v.shape[1]] = v[:, :min(v.shape[1], stride)]
    return out


LAYOUT_STRIDES = {"wide": (16, 16, 16), "compact": (1, 4, 3)}  # density_out, rgb_out, d_rgb_out


# ---- nvo_ngp_composite_loss: one launch -------------------------------------------------------------------------------
def _run_loss(device, case, opts, training, layout="wide", counts=None, offsets=None, carry_in=None, want_carry=False,
              accumulate=False, outs=None):
    """-> dict of CPU tensors.  Training: losses [64][8] (pre-fill ``shard_pattern``), d_pre [capacity], d_y
    [capacity][d_rgb_stride]; out_* pre-filled with NaN unless ``outs`` hands in the buffers of an earlier round."""
    _lib, _call, _ptr, _stream = _abi()
    o = N.make_opts(**(opts or {}))
    R, cap = case["R"], case["capacity"]
    ds, rs, gs = LAYOUT_STRIDES[layout]
    dev = lambda t: t.to(device)  # noqa: E731
    keep = {"counts": dev((case["counts"] if counts is None else counts).to(torch.int32)),
            "offsets": dev((case["offsets"] if offsets is None else offsets).to(torch.int32)),
            "ray_idx": dev(case["ray_idx"]), "t": dev(case["t"]), "dt": dev(case["dt"]),
            "den": dev(_strided(case["pre"], ds)), "col": dev(_strided(case["y"], rs)),
            "bg": dev(case["background"]), "gt_rgb": dev(case["gt_rgb"]), "gt_depth": dev(case["gt_depth"]),
            "dnorm": dev(case["dnorm"]), "cov": dev(case["cov"]), "state": dev(case["state"])}
    if outs is None:
        outs = {"out_rgb": torch.full((R, 3), NAN, device=device), "out_depth": torch.full((R,), NAN, device=device),
                "out_acc": torch.full((R,), NAN, device=device)}
    shard_pattern = _pattern((64, 8), 5)
    keep["losses"] = dev(shard_pattern)
    keep["d_pre"] = torch.full((cap,), NAN, device=device)
    keep["d_y"] = torch.full((cap, gs), NAN, dtype=F16, device=device)
    keep["carry_out"] = torch.full((R,), NAN, device=device)
    if carry_in is not None:
        keep["carry_in"] = dev(carry_in.float())
    if o["R_dev"] is not None:
        keep["R_dev"] = torch.tensor([o["R_dev"]], dtype=torch.int32, device=device)
        inv_rays = 123.0  # (must be ignored)
    else:
        inv_rays = o["inv_rays"] if o["inv_rays"] is not None else 1.0 / R
    p = lambda k: keep[k].data_ptr()  # noqa: E731
    la = _lib.NgpLossArgs(
        R=R, capacity=cap, counts=p("counts"), offsets=p("offsets"), ray_idx=p("ray_idx") if training else None, t=p("t"),
        dt=p("dt"), density_out=p("den"), density_stride=ds, rgb_out=p("col"), rgb_stride=rs,
        background=p("bg") if o["background"] else None, gt_rgb=p("gt_rgb") if training else None,
        gt_depth=p("gt_depth") if (training and o["depth"] != "null") else None,
        directions_norm=p("dnorm") if o["dnorm"] else None, rgb_mult=o["rgb_mult"],
        depth_mult=0.0 if o["depth"] == "mult0" else o["depth_mult"], inv_rays=inv_rays, loss_scale=o["loss_scale"],
        out_rgb=outs["out_rgb"].data_ptr(), out_depth=outs["out_depth"].data_ptr(), out_accumulation=outs["out_acc"].data_ptr(),
        losses=p("losses") if training else None, d_rgb_out=p("d_y") if training else None, d_rgb_stride=gs,
        d_density_pre=p("d_pre") if training else None, carry_in=p("carry_in") if carry_in is not None else None,
        carry_out=p("carry_out") if want_carry else None, accumulate_outputs=int(accumulate),
        train_min_transmittance=o["thr"], gt_depth_cov=p("cov") if (training and o["cov"]) else None,
        ray_state=p("state") if (training and o["state"]) else None, R_dev=p("R_dev") if o["R_dev"] is not None else None,
        world_size=o["world_size"])
    _call("nvo_ngp_composite_loss", _stream(device), C.byref(la))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in outs.items()}
    got.update({"losses": keep["losses"].cpu(), "d_pre": keep["d_pre"].cpu(), "d_y": keep["d_y"].cpu(),
                "carry_out": keep["carry_out"].cpu(), "shard_pattern": shard_pattern, "outs_device": outs})
    return got


def _slots_of(case, rays):
    m = torch.zeros(case["capacity"], dtype=torch.bool)
    for r in rays:
        m[int(case["offsets"][r]):int(case["offsets"][r]) + int(case["counts"][r])] = True
    return m


def _check_training(case, opts, got, ref, name, layout):
    """every assertion of a training launch against the oracle's ``ref`` (test a; the states and R_dev tests add theirs)"""
    o = N.make_opts(**opts)
    R, cap = case["R"], case["capacity"]
    gs = LAYOUT_STRIDES[layout][2]
    fails = []
    wr, cr = ref["written"], ref["capped_ray"]
    for q in N.RAY_OUTPUTS:
        assert _all_nan(got[q][~wr]), f"{q}: a row past R_dev was written"
    fails += _hold_rays(f"composite/{name}", got, ref)
    for suffix, rows in (("", wr & ~cr), ("_capped", wr & cr)):  # (rays with a capped sample: keys and a factor of their own)
        acc_bound = N.bound_for(f"composite/{name}:out_acc{suffix}", _margins())
        assert int(rows.sum()) >= 1 and float(got["out_acc"][rows].max()) <= 1.0 + acc_bound, float(got["out_acc"][rows].max())
    # samples: rows of no ray are exact zeros in every column, rows of rays past R_dev keep their pre-fill
    empty = case["ray_idx"] < 0
    past = _slots_of(case, [r for r in range(R) if not bool(wr[r])])
    inside = ~empty & ~past
    assert _all_zero_bits(got["d_pre"][empty]) and _all_zero_bits(got["d_y"][empty]), "ray_idx < 0 rows are not exact zeros"
    assert _all_nan(got["d_pre"][past]) and _all_nan(got["d_y"][past]), "sample rows of a ray past R_dev were written"
    assert bool(torch.isfinite(got["d_pre"][inside]).all()) and bool(torch.isfinite(got["d_y"][inside]).all()), \
        "a NaN pre-fill survived in a live row, or a gradient is not finite"
    if gs > 3:
        assert _all_zero_bits(got["d_y"][inside][:, 3:]), "columns 3.. of a live row are not exact zeros"
    # rays that leave no trace (dropped, state 2) own no sample rows, so ``inside`` is the oracle's ``live``
    assert torch.equal(inside, ref["live"])
    dead = ref["dead"]
    assert (int(dead.sum()) > 0) == (o["thr"] > 0)
    assert _all_zero_bits(got["d_pre"][dead]) and _all_zero_bits(got["d_y"][dead]), "a row with T < threshold is not exact zero"
    # a capped sample (exp(pre) dt >= 128) has an exact zero density gradient: the +30..+70 samples and the fp16-max one
    capped = inside & (torch.exp(case["pre"].double()) * case["dt"].double() >= N.DD_CAP)
    assert int(capped.sum()) >= (7 if bool(wr.all()) else 1)
    assert _all_zero_bits(got["d_pre"][capped]), got["d_pre"][capped]
    fails += _hold(f"composite/{name}:d_pre", got["d_pre"][inside], ref["d_pre"][inside])
    fails += _hold_fp16(f"composite/{name}:d_y", got["d_y"][inside][:, :3], ref["d_y"][inside])
    # losses: the shards were ADDED to (slots 0 and 1), slots 2..7 are untouched bit for bit
    pat = got["shard_pattern"]
    assert _same_bits(got["losses"][:, 2:], pat[:, 2:]), "a shard slot behind 1 was written"
    added = got["losses"].double()[:, :2] - pat.double()[:, :2]
    fails += _hold(f"composite/{name}:loss_rgb", added[:, 0].sum().reshape(1), ref["loss_rgb"])
    fails += _hold(f"composite/{name}:loss_depth", added[:, 1].sum().reshape(1), ref["loss_depth"])
    assert R <= 64  # one ray per shard: each shard against its own ray's loss
    per_ray = {"l_rgb": added[:R, 0], "l_depth": added[:R, 1]}
    for q, fig in N.ray_output_figures(per_ray, ref, wr, cr, N.RAY_LOSSES).items():
        fails += _judge(f"composite/{name}:{q}", fig)
    assert _same_bits(got["losses"][R:], pat[R:]), "a shard without a ray was written"
    silent = [r for r in range(R) if float(ref["l_rgb"][r]) == 0.0 and float(ref["l_depth"][r]) == 0.0]
    assert _same_bits(got["losses"][silent], pat[silent]), "a ray that leaves no trace in the losses reached its shard"
    return fails


_CASE = {}


def _composite_case():
    if "c" not in _CASE:
        _CASE["c"] = N.composite_case()
        cls = _CASE["c"]["classes"]
        assert all(cls[f"count_{e}"] >= 1 for e in N.LISTED_COUNTS), cls
        assert min(cls[k] for k in ("thin", "surface", "hot", "fp16_max", "neg_inf", "dt0", "y30", "free_slots")) >= 1, cls
    return _CASE["c"]


@pytest.mark.parametrize("layout", N.LAYOUTS)
@pytest.mark.parametrize("variant", [v for v in N.COMPOSITE_VARIANTS if not v.startswith("states")])
def test_composite_loss_training(device, variant, layout):
    """Test a.  Rays of 0 (empty), 0 (dropped), 1, 2, 63, 64, 65, 127, 128, 129, 200 samples and more, in one launch: both
    training forms.  Background present / NULL, depth on / gt_depth NULL / depth_mult 0, every class of gt_depth_cov,
    train_min_transmittance 0 and 0.05; strides 16 / 16 / 16 and 1 / 4 / 3 (no column behind 2 to clear).  What the kernel
    does with the fp16-max sample (sigma = inf, dt > 0): its optical step is the cap, 128, everything stays finite, its
    density gradient is an exact zero like every capped sample's."""
    case = _composite_case()
    opts = N.COMPOSITE_VARIANTS[variant]
    got = _run_loss(device, case, opts, True, layout)
    ref = N.composite_reference(case, True, opts)
    fails = _check_training(case, opts, got, ref, variant, layout)
    assert not fails, fails


@pytest.mark.parametrize("thr", ["thr0", "thr05"])
def test_composite_loss_states(device, thr):
    """Test c.  ray_state given: a state-1 ray sees no background (its out_rgb equals, bit for bit, the launch without a
    background), state-2 and dropped rays leave no trace in the shards and render nothing."""
    case = _composite_case()
    cls = case["classes"]
    assert cls["state1_short"] >= 1 and cls["state1_long"] >= 1 and cls["state2"] >= 2 and cls["state0"] >= 1
    name = f"states-{thr}"
    opts = N.COMPOSITE_VARIANTS[name]
    got = _run_loss(device, case, opts, True)
    ref = N.composite_reference(case, True, opts)
    fails = _check_training(case, opts, got, ref, name, "wide")
    nobg = _run_loss(device, case, dict(opts, background=False), True)
    s1, s0 = case["state"] == 1, (case["state"] == 0) & (case["counts"] > 0)
    assert _same_bits(got["out_rgb"][s1], nobg["out_rgb"][s1]), "a state-1 ray saw the background"
    assert int((got["out_rgb"][s0] != nobg["out_rgb"][s0]).any(dim=1).sum()) >= 3, "state-0 rays saw no background"
    s2 = case["state"] == 2
    for q in ("out_rgb", "out_depth", "out_acc"):
        assert _all_zero_bits(got[q][s2]), f"{q} of a state-2 ray"
    assert _same_bits(got["losses"][s2.nonzero().view(-1)], got["shard_pattern"][s2.nonzero().view(-1)])
    # without ray_state the dropped ray is known by its kept slot range: rendered (the background), no trace in the shards
    plain = _run_loss(device, case, dict(opts, state=False), True)
    d = case["entries"].index("dropped")
    assert _same_bits(plain["out_rgb"][d], case["background"][d]) and _same_bits(plain["losses"][d], plain["shard_pattern"][d])
    e = case["entries"].index("empty")  # a truly empty ray of state 0 is a ray: (background - gt)^2 reaches its shard
    assert float(plain["losses"][e, 0]) != float(plain["shard_pattern"][e, 0])
    assert not fails, fails


@pytest.mark.parametrize("world", N.RDEV_WORLDS)
def test_composite_loss_device_ray_count(device, world):
    """Test c.  R_dev < R: rows past it keep their NaN pre-fill (rays and samples), the losses are means over
    R_dev * max(world_size, 1) rays whatever inv_rays says."""
    case = _composite_case()
    opts = dict(N.COMPOSITE_VARIANTS["bg-depth-cov-thr0"], R_dev=case["R"] - N.RDEV_SHORT, world_size=world)
    got = _run_loss(device, case, opts, True)
    ref = N.composite_reference(case, True, opts)
    assert int((~ref["written"]).sum()) == N.RDEV_SHORT
    fails = _check_training(case, opts, got, ref, f"rdev-w{world}", "wide")
    assert not fails, fails


# ---- b. same-bits claims ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, N.TRAIN_THR])
def test_short_form_has_the_chunked_form_bits(device, thr):
    """Test b.  A 65-sample ray whose last sample has dt = 0 takes the chunked form, the 64-sample ray with the same first
    64 samples the register form, in ONE launch: out_* and the first 64 gradient rows are equal (+-0 alike)."""
    case = N.pair_case()
    got = _run_loss(device, case, dict(background=True, depth="on", cov=True, thr=thr), True)
    short, long_ = torch.arange(0, case["R"], 2), torch.arange(1, case["R"], 2)
    for q in ("out_rgb", "out_depth", "out_acc"):
        assert bool(torch.isfinite(got[q]).all())
        assert torch.equal(got[q][short], got[q][long_]), q  # (== on floats: +0 and -0 alike)
    nonzero = 0
    for a, b in zip(short.tolist(), long_.tolist()):
        oa, ob = int(case["offsets"][a]), int(case["offsets"][b])
        for q in ("d_pre", "d_y"):
            x, y = got[q][oa:oa + 64].float(), got[q][ob:ob + 64].float()
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y), (q, a, b, (x != y).nonzero()[:4].tolist())
            nonzero += int((x != 0).sum())
    assert nonzero > 64 * len(short)


def test_inference_launch_has_the_training_launch_bits(device):
    """Test b.  d_rgb_out NULL, no carry, no state: the three out_* buffers of the inference launch equal the training
    launch's bit for bit, for every count of the list (the register form among them)."""
    case = _composite_case()
    opts = dict(background=True, depth="on", cov=True, thr=0.0)
    tr = _run_loss(device, case, opts, True)
    inf = _run_loss(device, case, opts, False)
    for q in ("out_rgb", "out_depth", "out_acc"):
        assert bool(torch.isfinite(inf[q]).all())
        assert _same_bits(tr[q], inf[q]), (q, (tr[q] != inf[q]).nonzero()[:4].tolist())
    assert _all_nan(inf["d_pre"]) and _all_nan(inf["carry_out"]) and _same_bits(inf["losses"], inf["shard_pattern"])


# ---- d. inference in rounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", N.ROUND_CUTS)
def test_composite_inference_in_rounds(device, cut):
    """Test d.  Every ray's samples in two launches, cut inside the first chunk, at exactly 64 and beyond it: round one
    overwrites and leaves carry_out, round two takes it as carry_in and ADDS (a ray without a second part has count 0).
    The sums go against the oracle's single pass, the carries against the float64 optical depth."""
    case = _composite_case()
    opts = dict(background=False)
    (c1, o1), (c2, o2) = N.split_rounds(case, cut)
    assert int((c2 == 0).sum()) >= 3 and int((c2 > 0).sum()) >= 3
    one = _run_loss(device, case, opts, False, counts=c1, offsets=o1, want_carry=True)
    first = N.composite_reference(case, False, opts, counts=c1, offsets=o1)
    fails = _hold(f"rounds/cut{cut}:carry_first", one["carry_out"], first["carry"])
    two = _run_loss(device, case, opts, False, counts=c2, offsets=o2, carry_in=one["carry_out"], want_carry=True,
                    accumulate=True, outs=one["outs_device"])
    ref = N.composite_reference(case, False, opts)
    fails += _hold(f"rounds/cut{cut}:carry", two["carry_out"], ref["carry"])
    fails += _hold_rays(f"rounds/cut{cut}", two, ref)
    sat = c2 == 0  # a ray that sits the second round out: nothing added, its carry handed through
    assert _same_bits(two["out_depth"][sat], one["out_depth"][sat]) and _same_bits(two["carry_out"][sat], one["carry_out"][sat])
    assert not fails, fails


def test_composite_rounds_refuse_a_background(device):
    """Inference in rounds with a background is refused: every round would add T * background, and a ray that sits a later
    round out would add it once more."""
    case = _composite_case()
    (c1, o1), _ = N.split_rounds(case, 17)
    for kw in (dict(want_carry=True), dict(accumulate=True), dict(carry_in=torch.zeros(case["R"]))):
        with pytest.raises(RuntimeError, match="background == NULL"):
            _run_loss(device, case, dict(background=True), False, counts=c1, offsets=o1, **kw)
    got = _run_loss(device, case, dict(background=True), False, counts=c1, offsets=o1)  # (a single pass may have one)
    assert bool(torch.isfinite(got["out_rgb"]).all())


# ---- e. nvo_ngp_count_alive -------------------------------------------------------------------------------------------------
def _run_alive(device, case, stride, R_dev=None, counts=None, offsets=None, resume_in=None, carry_in=None, kept_base=0,
               t_next=None, rounds=False):
    _lib, _call, _ptr, _stream = _abi()
    R = case["R"]
    dev = lambda t: t.to(device)  # noqa: E731
    keep = {"counts": dev((case["counts"] if counts is None else counts).to(torch.int32)),
            "offsets": dev((case["offsets"] if offsets is None else offsets).to(torch.int32)), "dt": dev(case["dt"]),
            "den": dev(_strided(case["pre"], stride)),
            "kept": torch.full((R,), N.ALIVE_SENTINEL, dtype=torch.int32, device=device),
            "state": torch.full((R,), N.ALIVE_SENTINEL, dtype=torch.int32, device=device),
            "resume_out": torch.full((R,), NAN, device=device), "carry_out": torch.full((R,), NAN, device=device)}
    for k, v in (("resume_in", resume_in), ("carry_in", carry_in), ("t_next", t_next)):
        if v is not None:
            keep[k] = dev(v.float())
    if R_dev is not None:
        keep["R_dev"] = torch.tensor([R_dev], dtype=torch.int32, device=device)
    p = lambda k: keep[k].data_ptr() if k in keep else None  # noqa: E731
    aa = _lib.NgpAliveArgs(R=R, counts=p("counts"), offsets=p("offsets"), dt=p("dt"), density_out=p("den"), density_stride=stride,
                           min_transmittance=N.ALIVE_THR, kept=p("kept"), state=p("state"), R_dev=p("R_dev"),
                           resume_in=p("resume_in"), carry_in=p("carry_in"), kept_base=kept_base, t_next=p("t_next"),
                           resume_out=p("resume_out") if rounds else None, carry_out=p("carry_out") if rounds else None)
    _call("nvo_ngp_count_alive", _stream(device), C.byref(aa))
    torch.cuda.synchronize()
    return {k: keep[k].cpu() for k in ("kept", "state", "resume_out", "carry_out")}


def _check_alive(got, ref, key, rounds):
    assert torch.equal(got["kept"].long(), ref["kept"]), (got["kept"].tolist(), ref["kept"].tolist())
    assert torch.equal(got["state"].long(), ref["state"]), (got["state"].tolist(), ref["state"].tolist())
    if not rounds:
        assert _all_nan(got["resume_out"]) and _all_nan(got["carry_out"])
        return []
    same = torch.isnan(ref["resume_out"]) == torch.isnan(got["resume_out"])
    assert bool(same.all()) and torch.equal(torch.nan_to_num(got["resume_out"]).double(), torch.nan_to_num(ref["resume_out"]))
    on = torch.isfinite(ref["carry_out"])
    assert int(on.sum()) >= 2 and _all_nan(got["carry_out"][torch.isnan(ref["resume_out"])])
    return _hold(key, got["carry_out"][on], ref["carry_out"][on])


@pytest.mark.parametrize("stride", [1, 16])
def test_count_alive_single_round(device, stride):
    """Test e.  Rays cut at index 0 (the optical depth handed in is already past the threshold), 63, 64, 65, 128, 129, never;
    one dropped, one empty; R_dev < R leaves the rows past it alone.  No transmittance of any sample lies within 1e-3
    (relative) of the threshold (tests/test_ngp_oracle_cpu.py), so kept and state are exact: no tie allowance."""
    case = N.alive_case(stride)
    cls = case["classes"]
    assert all(cls[k] >= 1 for k in ("cut_at_0", "cut_at_63", "cut_at_64", "cut_at_65", "never", "dropped", "empty")), cls
    ref = N.alive_reference(case, R_dev=case["R_dev"], carry_in=case["carry_in"], rounds=True)
    assert ref["margin"] > N.TIE_MARGIN
    assert torch.equal(ref["kept"][:case["R_dev"]], torch.where(ref["state"][:case["R_dev"]] == 2, 0, case["expect"][:case["R_dev"]]))
    assert bool((ref["kept"][case["R_dev"]:] == N.ALIVE_SENTINEL).all())
    got = _run_alive(device, case, stride, R_dev=case["R_dev"], carry_in=case["carry_in"], rounds=True)
    fails = _check_alive(got, ref, f"alive/s{stride}:carry_out", True)
    assert bool((got["resume_out"][:case["R_dev"]] == -1.0).all())  # (no t_next: nobody goes on)
    # the plain single pass: no carry, no resume / carry outputs
    plain = _run_alive(device, case, stride)
    _check_alive(plain, N.alive_reference(case), "", False)
    assert not fails, fails


def test_count_alive_in_rounds(device):
    """Test e.  Two rounds of 64 samples: kept = kept_base + index; resume_out = t_next only for uncut, undropped rays whose
    march stopped at its budget; rows with resume_in < 0 keep their kept / state and get resume_out = -1; a ray whose
    transmittance falls below the threshold exactly behind round one's last sample is found at index 0 of round two."""
    case = N.alive_case(1)
    rd = N.alive_rounds(case)
    ref1 = N.alive_reference(case, counts=rd["counts"][0], offsets=rd["offsets"][0], t_next=rd["t_next"][0], rounds=True)
    got1 = _run_alive(device, case, 1, counts=rd["counts"][0], offsets=rd["offsets"][0], t_next=rd["t_next"][0], rounds=True)
    fails = _check_alive(got1, ref1, "alive/rounds:carry_out1", True)
    goes_on = ref1["resume_out"] >= 0
    assert 3 <= int(goes_on.sum()) < case["R"]
    ref2 = N.alive_reference(case, counts=rd["counts"][1], offsets=rd["offsets"][1], t_next=rd["t_next"][1], rounds=True,
                             resume_in=got1["resume_out"], carry_in=got1["carry_out"], kept_base=N.ALIVE_ROUND)
    got2 = _run_alive(device, case, 1, counts=rd["counts"][1], offsets=rd["offsets"][1], t_next=rd["t_next"][1], rounds=True,
                      resume_in=got1["resume_out"], carry_in=got1["carry_out"], kept_base=N.ALIVE_ROUND)
    fails += _check_alive(got2, ref2, "alive/rounds:carry_out2", True)
    assert bool((got2["kept"][~goes_on] == N.ALIVE_SENTINEL).all()) and bool((got2["resume_out"][~goes_on] == -1.0).all())
    assert bool((got2["state"][~goes_on] == N.ALIVE_SENTINEL).all()) and _all_nan(got2["carry_out"][~goes_on])
    at0 = (ref2["kept"] == N.ALIVE_ROUND) & (ref2["state"] == 1)
    assert int(at0.sum()) >= 2, "no ray is found at index 0 of the second round"
    # the two rounds together are the single pass
    kept = torch.where(goes_on, got2["kept"].long(), got1["kept"].long())
    assert torch.equal(kept, N.alive_reference(case)["kept"])
    assert not fails, fails


# ---- f. nvo_ngp_thickness, nvo_ngp_positions[_live] ------------------------------------------------------------------------
@pytest.mark.parametrize("level", N.THICKNESS_LEVELS)
@pytest.mark.parametrize("stride", [1, 16])
def test_thickness(device, stride, level):
    """exp(pre) * sqrt(3) / 1024 * 2^level against float64; pre = -inf gives an exact 0, fp16 max gives inf"""
    _lib, _call, _ptr, _stream = _abi()
    case = N.thickness_case()
    n = case["n"]
    den = _strided(case["pre"], stride).to(device)
    out = torch.full((n + 8,), NAN, device=device)
    _call("nvo_ngp_thickness", _stream(device), n, _ptr(den), stride, level, _ptr(out))
    torch.cuda.synchronize()
    out = out.cpu()
    ref = N.thickness_reference(case, level)["out"]
    assert _all_nan(out[n:])
    neg, big = torch.isinf(case["pre"]) & (case["pre"] < 0), case["pre"].float() == N.FP16_MAX
    assert int(neg.sum()) == 1 and int(big.sum()) == 1
    assert _all_zero_bits(out[:n][neg]) and float(out[:n][big]) == float("inf")
    fin = torch.isfinite(ref)
    fails = _hold(f"thickness/L{level}", out[:n][fin], ref[fin])
    assert not fails, fails


def _run_positions(device, case, n_live=None):
    _lib, _call, _ptr, _stream = _abi()
    cap = case["capacity"]
    dev = {k: case[k].to(device) for k in ("ray_idx", "t", "origins", "directions")}
    x01 = torch.full((cap, 3), NAN, device=device)
    args = [_stream(device), cap, _ptr(dev["ray_idx"]), _ptr(dev["t"]), _ptr(dev["origins"]), _ptr(dev["directions"]),
            case["lo"], case["hi"], _ptr(x01)]
    if n_live is None:
        _call("nvo_ngp_positions", *args)
    else:
        live = torch.tensor([n_live], dtype=torch.int32, device=device)
        _call("nvo_ngp_positions_live", *args, _ptr(live))
    torch.cuda.synchronize()
    return x01.cpu()


def test_positions(device):
    """x01 against the float32-input restatement; exact zeros for ray_idx < 0 (whose t is NaN), exact 0 and 1 outside the box"""
    case = N.positions_case()
    ref = N.positions_reference(case)
    got = _run_positions(device, case)
    empty = case["ray_idx"] < 0
    assert int(empty.sum()) >= 48 and _all_zero_bits(got[empty])
    live = ~empty[:, None].expand(-1, 3)
    below, above = live & (ref["raw"] < -1e-5), live & (ref["raw"] > 1.0 + 1e-5)
    assert int(below.sum()) >= 10 and int(above.sum()) >= 10
    assert _all_zero_bits(got[below]) and bool((got[above] == 1.0).all())
    fails = _hold("positions/x01", got, ref["x01"])
    assert not fails, fails


@pytest.mark.parametrize("n_live", N.LIVE_N)
def test_positions_live(device, n_live):
    """slots from the next multiple of 4096 behind n_live on keep their NaN pre-fill; the rows in front are written"""
    case = N.positions_case(N.LIVE_CAPACITY, seed=1)
    ref = N.positions_reference(case)["x01"]
    got = _run_positions(device, case, n_live)
    edge = (n_live + 4095) // 4096 * 4096
    assert edge in (4096, 8192) and _all_nan(got[edge:])
    assert bool(torch.isfinite(got[:edge]).all())
    fails = _hold("positions/live", got[:edge], ref[:edge])
    assert not fails, fails


# ---- g. rgb head ------------------------------------------------------------------------------------------------------------
def _run_head(device, case, hidden, with_d_pre=True, replicas=0, d_rgb=None, flag_value=0):
    _lib, _call, _ptr, _stream = _abi()
    cap, n_w = case["capacity"], case["n_weights"]
    keep = {k: case[k].to(device) for k in ("sh", "density_out", "ray_idx", "weights", "d_density_pre")}
    keep["d_rgb_out"] = (case["d_rgb_out"] if d_rgb is None else d_rgb).to(device)
    keep["rgb_out"] = torch.full((cap, 16), NAN, dtype=F16, device=device)
    keep["d_density_out"] = torch.full((cap, 16), NAN, dtype=F16, device=device)
    pat = _pattern((n_w,), 7, unit=2.0 ** -10)
    keep["d_weights"] = pat.to(device)
    keep["flag"] = torch.tensor([flag_value], dtype=torch.int32, device=device)
    if hidden:
        keep["hidden"] = torch.full((2, cap, 64), NAN, dtype=F16, device=device)
    if replicas:
        keep["rep"] = torch.zeros(replicas * n_w, device=device)
    p = lambda k: keep[k].data_ptr() if k in keep else None  # noqa: E731
    ra = _lib.NgpRgbArgs(capacity=cap, sh=p("sh"), density_out=p("density_out"), ray_idx=p("ray_idx"), weights=p("weights"),
                         rgb_out=p("rgb_out"), hidden=p("hidden"), d_rgb_out=p("d_rgb_out"), d_density_out=p("d_density_out"),
                         d_density_pre=p("d_density_pre") if with_d_pre else None, d_weights=p("d_weights"),
                         nonfinite_flag=p("flag"), dw_replicas=p("rep"), n_dw_replicas=replicas)
    _call("nvo_ngp_rgb_fwd", _stream(device), C.byref(ra))
    _call("nvo_ngp_rgb_bwd", _stream(device), C.byref(ra))
    if replicas:
        torch.cuda.synchronize()
        direct, spread = keep["d_weights"].cpu(), keep["rep"].cpu()
        _call("nvo_fold_replicas", _stream(device), 1, (C.c_void_p * 1)(p("rep")), (C.c_uint32 * 1)(replicas),
              (C.c_uint64 * 1)(n_w), (C.c_void_p * 1)(p("d_weights")))
    torch.cuda.synchronize()
    got = {k: keep[k].cpu() for k in ("rgb_out", "d_density_out", "d_weights", "flag")}
    got["pattern"] = pat
    if replicas:
        got["d_weights_before_fold"], got["rep_before_fold"], got["rep_after_fold"] = direct, spread, keep["rep"].cpu()
    return got


_HEAD = {}


def _head():
    if not _HEAD:
        _HEAD["case"] = N.rgb_head_case()
        _HEAD["ref"] = N.rgb_head_reference(_HEAD["case"])
    return _HEAD["case"], _HEAD["ref"]


def test_rgb_head_forward_and_backward(device):
    """Test g.  32 -> 64 -> 64 -> 16 on [density_out | SH16(ray_idx[row])]; a row with ray_idx < 0 is evaluated on
    [density_out | 0] (the loader substitutes a zero SH row: a specified, finite value -- pinned through the reference).
    With hidden == NULL the backward recomputes both hidden layers: every output bit-identical to the stored form's.
    d_weights accumulates (pre-filled); d_density_pre is added into column 0 before the one fp16 rounding."""
    from test_tcnn_gpu import _assert_close

    case, ref = _head()
    assert case["classes"]["empty_rows"] == 58 and case["classes"]["rays"] == N.HEAD_RAYS
    a, b = N.HEAD_EMPTY
    assert a[0] // 16 == (a[1] - 1) // 16 and b[0] // 16 != (b[1] - 1) // 16  # inside one 16-row tile / across tiles
    stored = _run_head(device, case, hidden=True)
    recomputed = _run_head(device, case, hidden=False)
    for k in ("rgb_out", "d_density_out"):
        assert bool(torch.isfinite(stored[k]).all()), k
        assert _same_bits(stored[k], recomputed[k]), k
    assert int(stored["flag"]) == 0 and int(recomputed["flag"]) == 0, "nonfinite_flag raised on finite inputs"
    _assert_close(stored["rgb_out"], ref["rgb_out"], rtol=1e-3, atol_scale=5e-4, what="ngp rgb head output")
    _assert_close(stored["d_density_out"], ref["d_density_out"], rtol=1.9e-3, atol_scale=9.3e-4, what="ngp rgb head dL/dinput")
    for got in (stored, recomputed):
        dw = got["d_weights"].double() - got["pattern"].double()
        _assert_close(dw, ref["d_weights"], rtol=3.1e-3, atol_scale=1.55e-3, what="ngp rgb head dL/dparams")
    # rows of no ray had zero gradients coming in: exact zeros going out
    empty = case["ray_idx"] < 0
    assert _all_zero_bits(stored["d_density_out"][empty])
    # d_density_pre: NULL against given -- columns 1..15 identical, column 0 the fp16 rounding of the float sum
    plain = _run_head(device, case, hidden=False, with_d_pre=False)
    assert _same_bits(plain["d_density_out"][:, 1:], recomputed["d_density_out"][:, 1:])
    _assert_close(plain["d_density_out"], ref["d_density_out_plain"], rtol=1.9e-3, atol_scale=9.3e-4, what="ngp rgb head dL/dinput (no d_pre)")
    diff = recomputed["d_density_out"][:, 0].double() - plain["d_density_out"][:, 0].double()
    want = case["d_density_pre"].double()
    slack = N.half_ulp_fp16(recomputed["d_density_out"][:, 0]) + N.half_ulp_fp16(plain["d_density_out"][:, 0])
    assert bool(((diff - want).abs() <= slack).all()), float(((diff - want).abs() - slack).max())
    assert float(want.abs().max()) > 100 * float(slack.max())


def test_rgb_head_replicas_and_nonfinite_flag(device):
    """Test g.  The workgroups spread their weight-gradient adds over d_weights and two zeroed replicas; folded by
    nvo_fold_replicas they give the plain form's gradient up to summation order (the replicas come back cleared); nonfinite_flag stays as it was on finite
    inputs and is OR-ed with 1 when one d_rgb_out row holds an inf."""
    from test_tcnn_gpu import _assert_close

    case, ref = _head()
    rep = _run_head(device, case, hidden=False, replicas=2, flag_value=4)
    n_w = case["n_weights"]
    parts = rep["rep_before_fold"].view(2, n_w)
    assert bool((parts[0] != 0).any()) and bool((parts[1] != 0).any()), "a replica received nothing"
    assert not _same_bits(rep["d_weights_before_fold"], rep["d_weights"]), "the fold added nothing"
    assert _all_zero_bits(rep["rep_after_fold"]) and int(rep["flag"]) == 4
    _assert_close(rep["d_weights"].double() - rep["pattern"].double(), ref["d_weights"], rtol=3.1e-3, atol_scale=1.55e-3,
                  what="ngp rgb head dL/dparams (replicas)")
    bad = case["d_rgb_out"].clone()
    bad[777, 1] = float("inf")
    hit = _run_head(device, case, hidden=False, d_rgb=bad, flag_value=4)
    assert int(hit["flag"]) == 5
