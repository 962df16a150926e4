"""The slice-owner grid backward (k_grid_bwd_lds) in its instruction-lean form against the form it replaces
(csrc/grid_bwd_legacy.hip, module option grid_bwd_scan = 0): the SAME launcher, item table, L1 scales and live list on the
SAME seeded inputs, driven through the raw C ABI the way the engine drives its proposal networks (_raw_nwie of
test_tcnn_gpu.py), the parameter gradient written into a buffer pre-filled with a sentinel.

The lean scans keep every floating-point expression (operands, order, association) and every index, so:
  * deterministic mode (every slice ONE work item, no live list -- the existing option that makes all items
    single-chunk): the two forms must agree BIT FOR BIT on every level (integer accumulators: the order of the adds is free);
  * default item table (chunked slices meet in float atomics; a live list's append order decides which samples share a
    run of the dense scan): agreement within 1e-6 x max|grad| of the level -- the bound test_grid_bwd_32bit_accumulators
    grants two runs of ONE form -- and the test asserts that two runs of the legacy form stay inside it as well, so the
    inputs are ones for which the reference alone passes.

Batch sizes: nvo_fwd / nvo_bwd take multiples of 16 only, so N real samples are padded to the next multiple of 16 with
rows whose gradient is exactly zero (what the Python modules do with a ragged batch).  The kernel therefore never sees
N % 4 != 0 through this ABI; ragged wave blocks, ragged lane runs and the scalar-load route of the dense scan are reached
through the padding, the chunk boundaries and the live list (whose length is arbitrary).
"""
import numpy as np
import pytest
import torch

from test_tcnn_gpu import MAIN, PROP0, PROP1, _assert_close, _pls, _ray_points, _raw_nwie

pytestmark = pytest.mark.gpu

PAD = 256          # sentinel floats on either side of the gradient buffer
SENTINEL = 7.0
BOUND = 1e-6       # x max|grad| of the level: float-atomic flush order (test_grid_bwd_32bit_accumulators)

GRIDS = {"prop0": (PROP0, 1), "prop1": (PROP1, 1), "main": (MAIN, 1), "main-streamed": (MAIN, 3)}
BATCHES = [8, 1000, 4096, 12328, 12331]
POSITIONS = ["uniform", "rays48", "rays256", "one-cell", "all-0.0", "all-1.0", "z-slab"]
DYS = ["quarter-zero", "all-zero", "nonfinite"]
# Every sample in ONE cell: all chunks of a dense slice add their partial sums to the same 16 accumulators.  The main grid in
# mode 1 has more slices than one round holds, so its item table ignores the batch hint and cuts a dense slice into ~50
# chunks; ~50 float atomics of mixed sign in arbitrary order on one entry leave sqrt(50 / 3) * 2^-24 * sum|partial| ~ 1e-6 x
# the (partly cancelled) total between two runs of ONE form -- the float-atomic bound cannot hold for those levels by the
# reference's own flush: those levels are compared against a bound taken from the legacy form's own run-to-run difference
# (SAME_CELL_BOUND, at the assertion), and bit for bit under the option that makes the items single-chunk (deterministic
# mode, asserted for every case below).  Everywhere else the bound is asserted as it stands: the
# proposal grids and the owner levels of the streamed main grid honour the batch hint (at most 2 chunks for these N:
# a + b = b + a), and the main grid's hashed levels have 2 chunks per slice.  (The streamed main grid's dense level 4 goes
# through the record pass, which cuts a bin into 8 tile-range chunks: lean against legacy, the same record-pass kernel, was
# seen 1.14e-6 x max apart on one-cell input.)  The same holds for a live list on such input: its append order decides
# which samples share a lane's run of 8, every run is rounded to the int32 quantum L1 / 2^29 on its own, and with ~150 runs on
# one entry whose total has largely cancelled two legacy runs were seen 4e-6 x max apart (N = 12328, all-0.0).
SAME_CELL = ("one-cell", "all-0.0", "all-1.0")
SAME_CELL_BOUND = 2e-5


def _levels(cfg):
    from oracle import grid as G

    lv, _ = G.level_table_numpy(cfg["n_levels"], cfg["log2_hashmap_size"], cfg["base_resolution"], _pls(cfg))
    return [(int(o), int(n), bool(h)) for o, n, _, h in lv]


def _positions(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, 3), dtype=np.float32)
    if kind in ("rays48", "rays256"):
        s = 48 if kind == "rays48" else 256
        return _ray_points((n + s - 1) // s, s, seed)[:n]
    if kind == "one-cell":  # (inside one cell of the finest level as well: 2048 cells per axis)
        return (np.float32(0.3) + rng.random((n, 3), dtype=np.float32) * np.float32(1e-4)).astype(np.float32)
    if kind == "all-0.0":
        return np.zeros((n, 3), dtype=np.float32)
    if kind == "all-1.0":  # the upper domain face: the wrap branch of the dense index
        return np.ones((n, 3), dtype=np.float32)
    assert kind == "z-slab"  # every third ray confined to one z slab: whole waves miss a dense level's other slices
    s = 48
    x = _ray_points((n + s - 1) // s, s, seed)[:n].copy()
    ray = np.arange(n) // s
    x[ray % 3 == 0, 2] = np.float32(0.40) + x[ray % 3 == 0, 2] * np.float32(0.05)
    return x


def _douts(kind, n, n_pad, live, seed):
    """dL/doutput of the network, one value per sample (compact output); the padding rows carry none."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n_pad, generator=g)
    if kind == "all-zero":
        d.zero_()
    else:
        d = d * (torch.rand(n_pad, generator=g) > 0.25)
    if live:  # 90 % of the samples dead, in runs of 64 as along trained rays: the listed scan (n_live < 3/4 N)
        d = d * (torch.rand((n_pad + 63) // 64, generator=g) >= 0.9).repeat_interleave(64)[:n_pad]
    d[n:] = 0.0
    if live and kind != "all-zero":
        d[n // 2] = 1.5  # (a short batch may lose every run to the mask: one sample is live whatever it draws)
    if kind == "nonfinite":
        d[0] = float("inf")
        d[n - 1] = float("nan")
    return d


def _module(device, cfg, mode, acc_bits, live, deterministic, scan, flag, batch=0):
    m = _raw_nwie(device, cfg, True, acc_bits=acc_bits, compact_live=live, runs=1)
    m.set_option("grid_bwd_batch", batch)  # (as the engine sets it: the one-round item table where the slices fit one)
    m.set_option("grid_bwd_mode", mode)
    m.set_option("deterministic", int(deterministic))
    m.set_option("grid_bwd_scan", scan)
    m.set_option("nonfinite_flag_ptr", flag.data_ptr())
    return m


def _backward(m, device, x, ph, dout, flag):
    """One forward + backward; returns (gradient view, whole sentinel-padded buffer, flag value)."""
    from nerf_vo_amd.engine import _call, _ptr, _stream

    st = _stream(device)
    n = x.shape[0]
    ctx = torch.empty(m.ctx_bytes(n), dtype=torch.uint8, device=device)
    out = torch.empty(n, dtype=torch.float16, device=device)
    _call("nvo_fwd", m.handle, st, n, _ptr(x), _ptr(ph), _ptr(out), _ptr(ctx))
    dy = (dout * 128).half()
    dx = torch.zeros((n, 3), device=device)
    buf = torch.full((m.n_params + 2 * PAD,), SENTINEL, device=device)
    dp = buf[PAD:PAD + m.n_params]
    flag.zero_()
    _call("nvo_bwd", m.handle, st, n, _ptr(x), _ptr(ph), _ptr(out), _ptr(dy), _ptr(ctx), _ptr(dx), _ptr(dp))
    torch.cuda.synchronize()
    return dp, buf, int(flag[0])


def _sentinel_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def _level_stats(a, b, levels, n_net):
    """Per level: (max |a - b| over the entries finite in both, max |a|, a all finite, b all finite) as one host tensor."""
    rows = []
    for o, cnt, _ in levels:
        u, v = a[n_net + 2 * o:n_net + 2 * (o + cnt)], b[n_net + 2 * o:n_net + 2 * (o + cnt)]
        fu, fv = torch.isfinite(u), torch.isfinite(v)
        both = fu & fv
        z = torch.zeros((), device=a.device)
        rows.append(torch.stack([torch.where(both, (u - v).abs(), z).max(), torch.where(fu, u.abs(), z).max(),
                                 fu.all().float(), fv.all().float()]))
    return torch.stack(rows).cpu()


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("grid", list(GRIDS), ids=list(GRIDS))
def test_lean_scans_give_the_legacy_gradient(device, grid, n):
    cfg, mode = GRIDS[grid]
    levels = _levels(cfg)
    n_pad = (n + 15) & ~15
    flag = torch.zeros(4, dtype=torch.int32, device=device)
    mods = {(live, det, scan): _module(device, cfg, mode, 32, live, det, scan, flag, batch=n_pad)
            for live in (0, 1) for det in (False, True) for scan in (0, 1)}
    n_params = mods[(0, False, 0)].n_params
    n_net = n_params - 2 * (levels[-1][0] + levels[-1][1])
    params = (torch.randn(n_params, generator=torch.Generator().manual_seed(41)) * 0.3).to(device)
    ph = params.half()
    seed = 100
    for pos in POSITIONS:
        xs = np.zeros((n_pad, 3), dtype=np.float32)
        xs[:n] = _positions(pos, n, 7)
        x = torch.from_numpy(xs).to(device)
        for dyk in DYS:
            for live in (0, 1):
                seed += 1
                what = f"{grid} N={n} {pos} dy={dyk} live={live}"
                dout = _douts(dyk, n, n_pad, live, seed).to(device)
                # ---- default item table: both forms inside the bound that two runs of the legacy form keep
                a, buf_a, fl_a = _backward(mods[(live, False, 0)], device, x, ph, dout, flag)
                b, buf_b, fl_b = _backward(mods[(live, False, 0)], device, x, ph, dout, flag)
                c, buf_c, fl_c = _backward(mods[(live, False, 1)], device, x, ph, dout, flag)
                assert _sentinel_intact(buf_a) and _sentinel_intact(buf_b) and _sentinel_intact(buf_c), what
                ref, lean = _level_stats(a, b, levels, n_net), _level_stats(a, c, levels, n_net)
                for l in range(len(levels)):
                    bound = BOUND * float(ref[l, 1])
                    if pos in SAME_CELL and not levels[l][2] and (grid.startswith("main") or live):
                        # (see SAME_CELL) the reference's own run-to-run difference sets the bound here: five times the
                        # largest seen between two legacy runs over all cases of this file (4e-6 x max), or four times
                        # what the two legacy runs of this very case show, whichever is larger
                        bound = max(SAME_CELL_BOUND * float(ref[l, 1]), 4.0 * float(ref[l, 0]))
                    assert float(ref[l, 0]) <= bound, f"{what} level {l}: two legacy runs differ by {float(ref[l, 0])} > {bound}"
                    assert float(lean[l, 0]) <= bound, f"{what} level {l}: lean vs legacy {float(lean[l, 0])} > {bound}"
                    assert float(lean[l, 2]) == float(lean[l, 3]), f"{what} level {l}: finite in one form only"
                if dyk == "nonfinite":
                    assert fl_a and fl_b and fl_c, f"{what}: nf_flag {fl_a} {fl_b} {fl_c}"
                    assert float(lean[:, 2].min()) == 0.0, f"{what}: the planted inf / nan left no trace"
                else:
                    assert not (fl_a or fl_b or fl_c), f"{what}: nf_flag raised without a non-finite gradient"
                    assert float(lean[:, 2].min()) == 1.0 and float(lean[:, 3].min()) == 1.0, what
                if dyk == "all-zero":
                    assert float(c[n_net:].abs().max()) == 0.0 and float(a[n_net:].abs().max()) == 0.0, what
                elif dyk == "quarter-zero":
                    assert float(lean[:, 1].max()) > 0.0, what
                # ---- single-chunk items, no list: the same bits
                d, buf_d, fl_d = _backward(mods[(live, True, 0)], device, x, ph, dout, flag)
                e, buf_e, fl_e = _backward(mods[(live, True, 1)], device, x, ph, dout, flag)
                assert _sentinel_intact(buf_d) and _sentinel_intact(buf_e), what
                assert bool(fl_d) == bool(fl_e) == (dyk == "nonfinite"), f"{what}: nf_flag {fl_d} {fl_e}"
                gd, ge = d[n_net:], e[n_net:]
                assert torch.equal(torch.isfinite(gd), torch.isfinite(ge)), f"{what}: other entries poisoned"
                assert torch.equal(torch.nan_to_num(gd, 0.0, 0.0, 0.0).view(torch.int32),
                                   torch.nan_to_num(ge, 0.0, 0.0, 0.0).view(torch.int32)), \
                    f"{what}: lean and legacy differ in deterministic mode (single-chunk items)"


@pytest.mark.parametrize("pos", ["uniform", "rays48"])
def test_lean_dense_scan_with_64_bit_accumulators(device, pos):
    """grid_acc_bits = 64 (no hit ring: the hashed levels take the generic scan, the dense ones the run-merging scan):
    lean against legacy inside the bound test_run_merged_dense_levels_match_slice_owner grants the run sums."""
    n = 4096
    flag = torch.zeros(4, dtype=torch.int32, device=device)
    x = torch.from_numpy(_positions(pos, n, 9)).to(device)
    dout = _douts("quarter-zero", n, n, 0, 77).to(device)
    res = []
    for scan in (0, 1):
        m = _module(device, PROP0, 1, 64, 0, False, scan, flag)
        if not res:
            params = (torch.randn(m.n_params, generator=torch.Generator().manual_seed(43)) * 0.3).to(device)
        res.append(_backward(m, device, x, params.half(), dout, flag)[0].clone())
    n_net = 16 * 16 + 16 * 16
    assert float(res[0][n_net:].abs().max()) > 0
    _assert_close(res[1][n_net:], res[0][n_net:], rtol=5e-6, atol_scale=5e-7, what="grid gradient, lean vs legacy (64-bit)")


def test_lean_scan_sample_major_gradients(device):
    """The stand-alone encoding hands the backward SAMPLE-major dL/dy ([N][L] pairs, a ragged batch padded inside the
    module).  Deterministic mode: lean and legacy agree bit for bit."""
    import nerf_vo_amd.tinycudann as tcnn
    from test_tcnn_gpu import _enc_cfg

    n = 1000
    g = torch.Generator().manual_seed(19)
    x = torch.from_numpy(_positions("rays48", n, 3)).to(device)
    dy = (torch.randn(n, 2 * PROP0["n_levels"], generator=g) * (torch.rand(n, 1, generator=g) > 0.25)).to(device)
    grads = []
    for scan in (0, 1):
        enc = tcnn.Encoding(3, _enc_cfg(PROP0)).to(device)
        m = enc.native_tcnn_module
        m.set_option("grid_acc_bits", 32)
        m.set_option("grid_bwd_runs", 1)
        m.set_option("deterministic", 1)
        m.set_option("grid_bwd_mode", 1)
        m.set_option("grid_bwd_scan", scan)
        with torch.no_grad():
            enc.params.copy_(torch.linspace(-1, 1, enc.params.numel(), device=device))
        (enc(x).float() * dy).sum().backward()
        grads.append(enc.params.grad.clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default"])
def test_engine_step_with_lean_scans(device, deterministic):
    """64 rays, one plain and one proposal-update step from seeded parameters, eager.
    Deterministic mode (single-chunk items everywhere): the rgb each step's forward rendered is byte-identical between
    grid_bwd_scan 0 and 1, and so are all parameters after the steps.
    Default mode: the proposal grids' gradient of the update step agrees within the float-atomic bound, which two runs of
    the legacy form are asserted to keep as well.  (Parameters are not compared there: Adam's first steps move an entry by
    lr * g / (|g| + 1e-15), so an entry whose chunk sums cancel to 0 in one flush order and to 1e-12 in another moves by
    the whole learning rate in one run and not at all in the other -- in two runs of one form just as well.)"""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 4, 60, 80, 64
    seq = make_sequence(n, H, W, device=device)
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})
    c2w = ds.camera_extrinsics[:, :3, :4].contiguous()

    def run(scan):
        torch.manual_seed(29)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, deterministic=deterministic, dynamic_loss_scale=False,
                                          grid_bwd_scan=scan), device)
        gen = torch.Generator(device=device).manual_seed(6)
        eng.step, eng.steps_since_proposal_update = 100, 1  # (past the first ten steps, which all update: plain, then update)
        rgb, updated = [], []
        for _ in range(2):
            idx = torch.floor(torch.rand(R, 3, device=device, generator=gen) * torch.tensor([n, H, W], device=device)).long()
            jit = tuple(torch.rand(R, device=device, generator=gen) for _ in range(3))
            updated.append(bool(eng.train_step(idx, ds.camera_intrinsics, c2w, ds.frames_color, ds.frames_depth, jitters=jit)))
            torch.cuda.synchronize()
            rgb.append(eng._workspace(R, True)["out_rgb"][:R].clone())
        assert updated == [False, True], updated
        prop = [eng.grads[o:o + s].clone() for o, s, _ in (eng.segments[f"proposal.{k}"] for k in range(2))]
        return rgb, prop, eng.params.clone()

    leg_a, leg_b, lean = run(0), run(0), run(1)
    assert all(float(p.abs().max()) > 0 for p in leg_a[1])
    if deterministic:
        for k in range(2):
            assert torch.equal(leg_a[0][k].view(torch.int32), lean[0][k].view(torch.int32)), f"rgb of step {k} differs"
        assert torch.equal(leg_a[2].view(torch.int32), lean[2].view(torch.int32)), "parameters differ"
        assert torch.equal(leg_a[2].view(torch.int32), leg_b[2].view(torch.int32))
    else:
        assert torch.equal(leg_a[0][0].view(torch.int32), lean[0][0].view(torch.int32)), "rgb of the first step differs"
        for k in range(2):
            bound = BOUND * float(leg_a[1][k].abs().max())
            d_ref, d_lean = float((leg_a[1][k] - leg_b[1][k]).abs().max()), float((leg_a[1][k] - lean[1][k]).abs().max())
            assert d_ref <= bound, f"proposal {k}: two legacy runs differ by {d_ref} > {bound}"
            assert d_lean <= bound, f"proposal {k}: lean vs legacy {d_lean} > {bound}"
