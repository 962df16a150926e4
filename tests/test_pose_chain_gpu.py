"""Kernel-level float64 parity of the camera-pose gradient chain: every kernel between dL/dx01 (and dL/dSH) and
dL/dpose_adjustment is fed synthetic float32 inputs through the C ABI and held to the float64 autograd restatements of
tests/helpers/pose_oracle.py -- nvo_positions_bwd, nvo_ngp_positions_bwd[_dev], nvo_sh_bwd_input_f32, the three
per-camera sums (nvo_pose_bwd, nvo_pose_bwd_cams, nvo_pose_bwd_det), nvo_se3_exp_map_bwd_scaled and nvo_pose_exp_map in
both camera modes, and the whole sequence of NerfactoEngine._pose_backward against ONE autograd graph.

Figure: max|got - ref64| / max|ref64| per comparison (per |w| bucket for the exp-map cases).  Bound: factor * e32 + 1e-6
with factor 4 and e32 the same figure of the float32 run of the SAME oracle function on the same inputs, measured on the
CPU (profiles/pose_parity_margins.json, written by tests/helpers/pose_tolerances.py and guarded by
tests/test_pose_oracle_cpu.py).  Factor 4: another summation order (wave tree against sequential) and the device's
sinf / cosf in the cancelling terms just above the Taylor switch; 1e-6 (16 ulp): cases where float32 autograd happens to
be exact.  No element is exempt.  Output buffers are pre-filled: a known pattern where the contract is "accumulates", NaN
where it is "overwrites".  NVO_POSE_MEASURED=<file> records the kernel figures of the session.
"""
import json
import os

import pytest
import torch

from helpers import pose_oracle as P

pytestmark = pytest.mark.gpu

MEASURED = {}
_MARGINS = None
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _record_measured():
    yield
    path = os.environ.get("NVO_POSE_MEASURED")
    if path and MEASURED:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1)


def _abi():
    from nerf_vo_amd.engine import _call, _ptr, _stream

    return _call, _ptr, _stream


def _hold(key, got, ref):
    """assert figure(got, ref) <= bound of ``key``; every figure is printed and recorded before it is judged."""
    global _MARGINS
    if _MARGINS is None:
        _MARGINS = P.load_margins()
    fig, bound = P.figure(got.detach().cpu(), ref), P.bound_for(key, _MARGINS)
    MEASURED[key] = max(fig, MEASURED.get(key, 0.0))
    print(f"{key}: figure {fig:.3e} bound {bound:.3e} (e32 {_MARGINS['e32'][key]:.3e})")
    return [] if fig <= bound else [f"{key}: {fig:.3e} > {bound:.3e}"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pattern(shape, device, seed=0):
    """a known non-zero pre-fill for outputs that are added to (multiples of 1/64 below 1/2: exact in float32)"""
    g = torch.Generator().manual_seed(99 + seed)
    return (torch.randint(1, 32, shape, generator=g).float() / 64.0 * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(device)


# ---- a. nvo_positions_bwd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", P.POSITIONS_S)
@pytest.mark.parametrize("R", P.POSITIONS_R)
def test_positions_bwd(device, R, S):
    """One wave per ray, lanes stride over S samples, 4 rays per workgroup.  The masked set is what nvo_sample_positions
    writes as exact zeros on the same inputs (the inf-edged sample among them); dx01 is NaN there and the outputs must
    come out finite.  Called twice into the same pre-filled outputs, as the engine does once per level: both calls add."""
    _call, _ptr, _stream = _abi()
    c = P.positions_case(R, S)
    o, d, tb = (c[k].to(device) for k in ("origins", "directions", "tbins"))
    x01 = torch.full((R * S, 3), NAN, device=device)
    _call("nvo_sample_positions", _stream(device), R, S, _ptr(o), _ptr(d), _ptr(tb), _ptr(x01))
    x01 = x01.cpu()
    assert bool(torch.isfinite(x01).all())
    mask = (x01 == 0).all(dim=1).view(R, S)
    classes = P.sample_classes(c["origins"], c["directions"], c["tbins"], mask)
    print(classes)
    if R >= 5:
        assert classes["mag_one"] >= 1 and classes["inf_edge"] == 1 and bool(mask[R - 1, S - 1])
    if R == 259 and S >= 48:
        assert all(v > 0 for v in classes.values()), classes
    ref = P.positions_reference(c, mask)
    pre_o, pre_d = _pattern((R, 3), device, 1), _pattern((R, 3), device, 2)
    g_o, g_d = pre_o.clone(), pre_d.clone()
    fails = []
    for call, suffix in enumerate(("", "_twice")):
        dx = c["dx01"][call].clone()
        dx[mask.view(-1)] = NAN
        dx = dx.to(device)
        _call("nvo_positions_bwd", _stream(device), R, S, _ptr(o), _ptr(d), _ptr(tb), _ptr(dx), _ptr(g_o), _ptr(g_d))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g_o).all() and torch.isfinite(g_d).all()), "a masked sample's NaN reached the output"
        fails += _hold(f"positions/R{R}-S{S}:d_origin{suffix}", g_o.double() - pre_o.double(), ref[f"d_origin{suffix}"])
        fails += _hold(f"positions/R{R}-S{S}:d_dir{suffix}", g_d.double() - pre_d.double(), ref[f"d_dir{suffix}"])
    assert not fails, fails


# ---- b. nvo_ngp_positions_bwd[_dev] --------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("box", list(P.NGP_BOXES))
def test_ngp_positions_bwd(device, box, entry):
    """Packed ranges with counts 0, 1, 63, 64, 65, 200, one range that straddles capacity and one that starts beyond it;
    outputs are OVERWRITTEN (NaN pre-fill); with a device R_dev < R the rows past it come back as exact zeros.  In the
    power-of-two box two rays lie exactly in the faces x = lo and x = hi: the clamp passes no gradient there."""
    _call, _ptr, _stream = _abi()
    c = P.ngp_case(box)
    R, cap = c["R"], c["capacity"]
    assert set((0, 1, 63, 64, 65, 200)) <= set(c["counts"].tolist())
    off, cnt = c["offsets"].tolist(), c["counts"].tolist()
    assert off[-2] < cap < off[-2] + cnt[-2] and off[-1] >= cap and cnt[-1] > 0
    assert all(n > 0 for n in c["per_face"]) and c["sides"]["inside"] > 0, c["sides"]
    assert (c["sides"]["on_face"] > 0) == (box == "pow2")
    dev = {k: c[k].to(device) for k in ("counts", "offsets", "t", "origins", "directions", "dx01")}
    g_o, g_d = torch.full((R, 3), NAN, device=device), torch.full((R, 3), NAN, device=device)
    args = [_stream(device), R, cap, _ptr(dev["counts"]), _ptr(dev["offsets"]), _ptr(dev["t"]), _ptr(dev["origins"]),
            _ptr(dev["directions"]), c["lo"], c["hi"], _ptr(dev["dx01"]), _ptr(g_o), _ptr(g_d)]
    if entry == "dev":
        r_dev = torch.tensor([c["R_dev"]], dtype=torch.int32, device=device)
        _call("nvo_ngp_positions_bwd_dev", *args, _ptr(r_dev))
    else:
        _call("nvo_ngp_positions_bwd", *args)
    torch.cuda.synchronize()
    ref = P.ngp_reference(c, entry == "dev")
    assert bool(torch.isfinite(g_o).all() and torch.isfinite(g_d).all()), "an output row was not overwritten"
    if entry == "dev":
        zero = torch.zeros(R - c["R_dev"], 3, dtype=torch.int32)
        assert torch.equal(_bits(g_o[c["R_dev"]:]), zero) and torch.equal(_bits(g_d[c["R_dev"]:]), zero)
    else:
        assert torch.equal(_bits(g_o[-1]), torch.zeros(3, dtype=torch.int32)), "a range beyond capacity contributed"
    fails = _hold(f"ngp/{box}-{entry}:d_origin", g_o, ref["d_origin"]) + _hold(f"ngp/{box}-{entry}:d_dir", g_d, ref["d_dir"])
    assert not fails, fails


# ---- c. nvo_sh_bwd_input_f32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_bwd_input_f32(device, degree):
    """dy has 16 floats per row whatever the degree; the columns >= degree^2 hold NaN and must be ignored.  dd01 is
    overwritten (NaN pre-fill).  N = 257: more than one workgroup."""
    _call, _ptr, _stream = _abi()
    c = P.sh_case(degree)
    N = c["d01"].shape[0]
    d01, dy = c["d01"].to(device), c["dy"].to(device)
    out = torch.full((N, 3), NAN, device=device)
    _call("nvo_sh_bwd_input_f32", _stream(device), N, degree, _ptr(d01), _ptr(dy), _ptr(out))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    fails = _hold(f"sh/deg{degree}:dd01", out, P.sh_reference(c)["dd01"])
    assert not fails, fails


# ---- d. the three per-camera sums -------------------------------------------------------------------------------------
def _pose_run(device, name, c, with_d01):
    """one call of a per-camera sum into a pre-filled [F+1][3][4] buffer (row F is the sentinel) -> (result, pre-fill)"""
    _call, _ptr, _stream = _abi()
    R, F = c["R"], c["F"]
    dev = {k: c[k].to(device) for k in ("idx", "intr", "c2w", "d_origin", "d_dir", "d_dir01")}
    pre = _pattern((F + 1, 3, 4), device, 3)
    acc = pre.clone()
    args = [_stream(device), R, _ptr(dev["idx"]), _ptr(dev["intr"]), _ptr(dev["c2w"]), _ptr(dev["d_origin"]),
            _ptr(dev["d_dir"]), _ptr(dev["d_dir01"]) if with_d01 else None, _ptr(acc)]
    if name == "nvo_pose_bwd_det":
        scratch = torch.full((R, 12), NAN, device=device)
        args += [_ptr(scratch), F]
    elif name == "nvo_pose_bwd_cams":
        args += [F]
    _call(name, *args)
    torch.cuda.synchronize()
    return acc, pre


def _check_pose(device, c, key, with_d01, names):
    F = c["F"]
    ref = P.pose_reference(c, with_d01)["d_corr"]
    cam = c["idx"][:, 0]
    empty = torch.ones(F + 1, dtype=torch.bool)
    empty[cam[(cam >= 0) & (cam < F)]] = False  # cameras without a ray, and the sentinel row
    fails = []
    for name in names:
        acc, pre = _pose_run(device, name, c, with_d01)
        assert torch.equal(_bits(acc[empty]), _bits(pre[empty])), f"{name}: a row without rays (or the sentinel row) changed"
        assert bool(torch.isfinite(acc).all()), name
        fails += [f"{name} {f}" for f in _hold(key, acc[:F].double() - pre[:F].double(), ref)]
        if name == "nvo_pose_bwd_det":
            again, _ = _pose_run(device, name, c, with_d01)
            assert torch.equal(_bits(acc), _bits(again)), "nvo_pose_bwd_det: two runs differ"
    return fails


@pytest.mark.parametrize("with_d01", [True, False], ids=["d01", "nod01"])
@pytest.mark.parametrize("R,F", P.POSE_SHAPES)
def test_pose_bwd_sums(device, R, F, with_d01):
    """nvo_pose_bwd, nvo_pose_bwd_cams (LDS table from 32 rays per camera on, plain atomics below) and nvo_pose_bwd_det
    (per-ray rows into a NaN-pre-filled scratch, then nvo_reduce_by_camera's int64 [R][3] camera form; two runs give the
    same bits) ADD into d_corrections; rows of cameras without rays stay bit-unchanged.  nvo_reduce_by_camera's int32
    camera form is reached from the fused colour-head backward only (mlp_impl.h, the embedding gradient): no C ABI entry
    exposes it with rows a test can set, so it is left to the engine-level tests."""
    c = P.pose_case(R, F)
    assert P.rays_per_camera_path(R, F) == ("plain" if (R, F) in ((4096, 192), (9, 16)) else "table")
    fails = _check_pose(device, c, f"pose/R{R}-F{F}-{'d01' if with_d01 else 'nod01'}:d_corr", with_d01,
                        ("nvo_pose_bwd", "nvo_pose_bwd_cams", "nvo_pose_bwd_det"))
    assert not fails, fails


@pytest.mark.parametrize("with_d01", [True, False], ids=["d01", "nod01"])
@pytest.mark.parametrize("R,F", P.STALE_SHAPES)
def test_pose_bwd_drops_stale_camera_indices(device, R, F, with_d01):
    """A few rays carry camera index -1, F and 2^40: nvo_pose_bwd_cams (table and plain path) and nvo_pose_bwd_det drop
    them.  intrinsics, c2w and d_corrections have F + 1 rows (NaN in the extra input row, a sentinel in the extra output
    row) and n_cameras = F, so a broken guard for index F shows as a wrong value.  (nvo_pose_bwd has no camera count
    and documents no guard: it is not given such indices.)"""
    c = P.pose_case(R, F, stale=True)
    cam = c["idx"][:, 0]
    assert int(((cam < 0) | (cam >= F)).sum()) == 9 and {-1, F, 1 << 40} <= set(cam.tolist())
    fails = _check_pose(device, c, f"pose/R{R}-F{F}-{'d01' if with_d01 else 'nod01'}-stale:d_corr", with_d01,
                        ("nvo_pose_bwd_cams", "nvo_pose_bwd_det"))
    assert not fails, fails


# ---- e. nvo_se3_exp_map_bwd_scaled, nvo_pose_exp_map -----------------------------------------------------------------
MODES = {"SE3": 0, "SO3xR3": 1}


@pytest.mark.parametrize("variant", P.EXP_VARIANTS, ids=[v[0] for v in P.EXP_VARIANTS])
@pytest.mark.parametrize("mode", list(MODES))
def test_exp_map_bwd(device, mode, variant):
    """257 cameras in buckets of |w| from 0 to 6 on both sides of the Taylor switch (SE3, theta < 1e-2) and of the clamp
    (SO3xR3, |w|^2 < 1e-4); some rows have a zero translation.  d_tangent is OVERWRITTEN (NaN pre-fill); penalties zero
    and non-zero; reg_scale from the host alone and times a device factor.  One bound per bucket."""
    _call, _ptr, _stream = _abi()
    name, tp, rp, host, dev_scale = variant
    c = P.exp_case(mode)
    n = c["n"]
    t, dc = c["tangent"].to(device), c["d_corr"].to(device)
    out = torch.full((n, 6), NAN, device=device)
    scale = None if dev_scale is None else torch.tensor([dev_scale], device=device)
    _call("nvo_se3_exp_map_bwd_scaled", _stream(device), n, _ptr(t), _ptr(dc), tp, rp, host, _ptr(out), None, MODES[mode],
          None if scale is None else _ptr(scale))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    ref = P.exp_reference(c, variant)["d_tangent"]
    fails = []
    got = out.cpu()
    for k, w in enumerate(c["buckets"]):
        rows = c["bucket"] == k
        assert int(rows.sum()) >= 16
        fails += _hold(f"exp/{mode}-{name}:w{w:g}", got[rows], ref[rows])
    assert not fails, fails


@pytest.mark.parametrize("n", P.EXP_N)
@pytest.mark.parametrize("mode", list(MODES))
def test_exp_map_bwd_regulariser_value(device, mode, n):
    """The regulariser's value is ADDED into the reg_loss slot (one workgroup strides over the cameras: n = 1, 257, 1000).
    The slot is pre-filled with 2^-10, below the value itself (4e-3 to 7e-3), so that rounding the sum to float32 costs
    under 1e-7 of the value (a pre-fill of 1/8 would cost 7e-7 and say nothing about the kernel)."""
    _call, _ptr, _stream = _abi()
    _, tp, rp, host, _ = variant = P.EXP_VARIANTS[1]
    c = P.exp_case(mode, n)
    t, dc = c["tangent"].to(device), c["d_corr"].to(device)
    out = torch.full((n, 6), NAN, device=device)
    slot = torch.tensor([2.0 ** -10], device=device)
    _call("nvo_se3_exp_map_bwd_scaled", _stream(device), n, _ptr(t), _ptr(dc), tp, rp, host, _ptr(out), _ptr(slot),
          MODES[mode], None)
    torch.cuda.synchronize()
    ref = P.exp_reference(c, variant)["reg"]
    assert float(ref) > 2e-3
    fails = _hold(f"exp/{mode}-n{n}:reg", slot.double().cpu() - 2.0 ** -10, ref.reshape(1))
    assert not fails, fails


@pytest.mark.parametrize("mode", list(MODES))
def test_pose_exp_map_forward(device, mode):
    """nvo_pose_exp_map on the same bucketed tangents, both modes (the golden test covers SE3 at two tangent scales)."""
    _call, _ptr, _stream = _abi()
    c = P.exp_case(mode)
    n = c["n"]
    t = c["tangent"].to(device)
    out = torch.full((n, 3, 4), NAN, device=device)
    _call("nvo_pose_exp_map", _stream(device), n, _ptr(t), _ptr(out), MODES[mode])
    torch.cuda.synchronize()
    ref = P.exp_reference(c, P.EXP_VARIANTS[0])["corr"]
    got, fails = out.cpu(), []
    for k, w in enumerate(c["buckets"]):
        rows = c["bucket"] == k
        fails += _hold(f"expfwd/{mode}:w{w:g}", got[rows], ref[rows])
    assert not fails, fails


# ---- f. the chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_camera", ["cams", "det"])
@pytest.mark.parametrize("mode", list(MODES))
def test_pose_chain(device, mode, per_camera):
    """The kernel sequence of NerfactoEngine._pose_backward on 1501 rays over 7 cameras and levels S = (256, 96, 48):
    nvo_pose_exp_map -> nvo_raygen -> nvo_positions_bwd x 3 -> nvo_sh_bwd_input_f32 -> per-camera sum ->
    nvo_se3_exp_map_bwd_scaled, against ONE float64 autograd graph from the tangent (pose_oracle.whole_chain): a factor or
    a sign lost BETWEEN two kernels shows here and in none of the per-kernel tests."""
    _call, _ptr, _stream = _abi()
    st = _stream(device)
    c = P.chain_case(mode)
    R, F = c["R"], c["F"]
    tp, rp, scale = P.CHAIN_PENALTIES
    t, idx, intr, c2w = (c[k].to(device) for k in ("tangent", "idx", "intr", "c2w"))
    corr = torch.full((F, 3, 4), NAN, device=device)
    _call("nvo_pose_exp_map", st, F, _ptr(t), _ptr(corr), MODES[mode])
    o, d = torch.full((R, 3), NAN, device=device), torch.full((R, 3), NAN, device=device)
    dnorm, cam32 = torch.empty(R, device=device), torch.empty(R, dtype=torch.int32, device=device)
    _call("nvo_raygen", st, R, _ptr(idx), _ptr(intr), _ptr(c2w), _ptr(corr), _ptr(o), _ptr(d), _ptr(dnorm), None, _ptr(cam32))
    g_o, g_d = torch.zeros(R, 3, device=device), torch.zeros(R, 3, device=device)
    masks = []
    for S, tb, dx in zip(P.CHAIN_LEVELS, c["tbins"], c["dx01"]):
        tb, dx = tb.to(device), dx.to(device)
        x01 = torch.full((R * S, 3), NAN, device=device)
        _call("nvo_sample_positions", st, R, S, _ptr(o), _ptr(d), _ptr(tb), _ptr(x01))
        masks.append((x01 == 0).all(dim=1).view(R, S).cpu())
        _call("nvo_positions_bwd", st, R, S, _ptr(o), _ptr(d), _ptr(tb), _ptr(dx), _ptr(g_o), _ptr(g_d))
    dirs01 = ((d + 1.0) * 0.5).contiguous()
    d_sh, g_d01 = c["d_sh"].to(device), torch.full((R, 3), NAN, device=device)
    _call("nvo_sh_bwd_input_f32", st, R, 4, _ptr(dirs01), _ptr(d_sh), _ptr(g_d01))
    d_corr = torch.zeros(F, 3, 4, device=device)
    if per_camera == "det":
        scratch = torch.full((R, 12), NAN, device=device)
        _call("nvo_pose_bwd_det", st, R, _ptr(idx), _ptr(intr), _ptr(c2w), _ptr(g_o), _ptr(g_d), _ptr(g_d01), _ptr(d_corr),
              _ptr(scratch), F)
    else:
        _call("nvo_pose_bwd_cams", st, R, _ptr(idx), _ptr(intr), _ptr(c2w), _ptr(g_o), _ptr(g_d), _ptr(g_d01), _ptr(d_corr), F)
    out = torch.full((F, 6), NAN, device=device)
    _call("nvo_se3_exp_map_bwd_scaled", st, F, _ptr(t), _ptr(d_corr), tp, rp, scale, _ptr(out), None, MODES[mode], None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert sum(int(m.sum()) for m in masks) == 0  # (bins out to t = 100: no sample saturates)
    ref = P.chain_reference(c, masks)["d_tangent"]
    fails = _hold(f"chain/{mode}:d_tangent", out, ref)
    assert not fails, fails
