"""Size-independent properties of the hot-path kernels at BASELINE.json's FULL batch sizes (4096 rays;
196 608 main-field samples, 1 048 576 / 393 216 proposal samples), where the CPU oracle would take minutes:

  * hash-grid forward: the 8 trilinear weights form a partition of unity -> a per-level constant table must come
    out as that constant (1 fp16 ulp);
  * hash-grid backward (every scatter form): per (level, feature) the gradient mass equals the dy mass
    ("checksum of checksums"), and the single-owner fixed-point forms are bitwise reproducible run to run;
  * bias-free ReLU MLPs are positively homogeneous and scaling by 2 is exact in fp16/fp32:
    f(2x) == 2 f(x) and dL/dx(2 dy) == 2 dL/dx(dy) BIT FOR BIT (fp16-subnormal values excepted);
  * PDF resampling: bins sorted, inside [0, 1], weights non-negative with sum <= 1;
  * stateless pixel sampler: every index inside the keyframe buffer, all counters distinct streams.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_tcnn_gpu import MAIN, PROP0, PROP1, _enc_cfg, _spec

pytestmark = pytest.mark.gpu

R = 4096
N_MAIN, N_P0, N_P1 = R * 48, R * 256, R * 96


DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}  # bf16 = BASELINE configs[4] (bf16 MFMA MLPs, fp16 hash tables)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("cfg,n", [(MAIN, N_MAIN), (PROP0, N_P0), (PROP1, N_P1)], ids=["main", "prop0", "prop1"])
def test_grid_forward_partition_of_unity(device, cfg, n, dtype):
    import nerf_vo_amd.tinycudann as tcnn

    spec = _spec(cfg)
    enc = tcnn.Encoding(3, _enc_cfg(cfg), dtype=DTYPES[dtype]).to(device)
    consts = torch.zeros(spec.n_levels, 2)
    with torch.no_grad():
        for l in range(spec.n_levels):
            lo, cnt = int(spec.levels[l, 0]), int(spec.levels[l, 1])
            consts[l] = torch.tensor([0.25 + 0.03125 * l, -(0.5 + 0.0625 * l)])  # exactly representable in fp16 and bf16
            enc.params[2 * lo:2 * (lo + cnt)] = consts[l].repeat(cnt).to(device)
    x = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(device)
    x[:4] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.5], [0.5, 0.5, 0.5]], device=device)
    y = enc(x).detach().float().view(n, spec.n_levels, 2)
    ref = consts.to(device)[None]
    # fp32 sum of 8 products w_i*c with sum(w_i) = 1 +- 4 ulp(fp32), rounded once to the output format (1 ulp)
    err = (y - ref).abs()
    ulp = 2.0 ** -10 if dtype == "f16" else 2.0 ** -7
    assert float((err / ref.abs()).max()) <= ulp, float((err / ref.abs()).max())
    assert float((err == 0).float().mean()) > 0.99


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("cfg,n,modes", [(MAIN, N_MAIN, (0, 1, 3)), (PROP0, N_P0, (0, 1)), (PROP1, N_P1, (0, 1))],
                         ids=["main", "prop0", "prop1"])
def test_grid_backward_mass_conservation(device, cfg, n, modes, dtype):
    import nerf_vo_amd.tinycudann as tcnn

    spec = _spec(cfg)
    enc = tcnn.Encoding(3, _enc_cfg(cfg), dtype=DTYPES[dtype]).to(device)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(n, 3, generator=g).to(device)
    dy = torch.randn(n, 2 * spec.n_levels, generator=g).to(device)
    # the kernel consumes dy in the 16-bit format (x128 loss scale inside autograd): the mass it distributes is that
    # of dy16
    dy16 = ((dy * 128).to(DTYPES[dtype]).double() / 128).view(n, spec.n_levels, 2)
    mass = dy16.sum(dim=0).cpu()                      # [L,2]
    l1 = dy16.abs().sum(dim=0).cpu()
    for mode in modes:
        enc.native_tcnn_module.set_option("grid_bwd_mode", mode)
        runs = []
        for _ in range(2):
            enc.params.grad = None
            (enc(x).float() * dy).sum().backward()
            runs.append(enc.params.grad.clone())
        grad = runs[0].double().cpu()
        for l in range(spec.n_levels):
            lo, cnt = int(spec.levels[l, 0]), int(spec.levels[l, 1])
            got = grad[2 * lo:2 * (lo + cnt)].view(cnt, 2).sum(dim=0)
            # fp32 atomics / 2^26 fixed point / 17-bit record mantissas: relative 2^-16 of the level's L1 mass
            assert torch.all((got - mass[l]).abs() <= l1[l] * 2.0 ** -16 + 1e-6), (mode, l, got, mass[l])
        if mode in (2, 3):  # hashed levels: integer accumulation with ONE owner per slice -> order-independent
            # (the slice-owner form, mode 1, splits a slice's samples over several work items whose partial sums meet
            # in fp32 global atomics, so it is reproducible only to rounding)
            hashed = 2 * int(spec.levels[5, 0])
            assert torch.equal(runs[0][hashed:], runs[1][hashed:]), f"mode {mode} is not bitwise reproducible"


MLPS = [  # n_in, n_out, width, hidden layers, batch
    (32, 16, 64, 1, N_MAIN),   # main-field base network
    (16, 16, 64, 2, N_MAIN),   # (colour-head shape without the sigmoid)
    (16, 16, 16, 1, N_P0),     # proposal density network, 1 M samples
]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("shape", MLPS, ids=[f"{s[0]}-{s[2]}x{s[3]}-{s[1]}@{s[4]}" for s in MLPS])
def test_mlp_positive_homogeneity_bit_exact(device, shape, dtype):
    import nerf_vo_amd.tinycudann as tcnn

    n_in, n_out, width, n_hidden, n = shape
    net = tcnn.Network(n_in, n_out, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None",
                                     "n_neurons": width, "n_hidden_layers": n_hidden}, dtype=DTYPES[dtype]).to(device)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        net.params.copy_((torch.randn(net.params.numel(), generator=g) * (1.0 / np.sqrt(width))).to(device))
    x = (torch.randn(n, n_in, generator=g) * 0.5).to(DTYPES[dtype]).float().to(device)
    dy = torch.randn(n, n_out, generator=g).to(device)
    outs = []
    for s in (1.0, 2.0):
        xs = (x * s).requires_grad_(True)
        y = net(xs)
        (y.float() * (dy * s)).sum().backward()
        outs.append((y.float().clone(), xs.grad.clone()))
    torch.cuda.synchronize()
    (y1, g1), (y2, g2) = [(a.detach(), b) for a, b in outs]
    assert torch.isfinite(y2).all() and float(y1.abs().max()) > 0
    # Doubling is exact for every fp16 NORMAL number, so an output whose whole dependency chain stays in the normal
    # range doubles exactly (measured: > 99.98 % of them).  Values below fp16's smallest normal (2^-14) live on the
    # fixed 2^-24 subnormal grid, where round(2a) != 2 round(a): a subnormal output may differ by one grid step, and a
    # subnormal hidden activation perturbs its sample by ~2^-25 * |w|, which can flip the final rounding of an output
    # sitting on a rounding boundary -- never more than ONE fp16 ulp.  (Subnormal operands are NOT flushed: probed.)
    diff = (y2 - 2.0 * y1).abs()
    # (bf16 has fp32's exponent range: nothing here comes near its subnormals, so doubling is exact throughout)
    rel_ulp = 2.0 ** -9 if dtype == "f16" else 2.0 ** -6
    ulp = torch.maximum((2.0 * y1).abs() * rel_ulp, torch.full_like(y1, 2.0 ** -23))  # (x2: binade edges)
    assert bool((diff <= ulp).all()), f"f(2x) differs from 2 f(x) by more than one {dtype} ulp: {float((diff / ulp).max()):.2f}"
    assert int((diff > 0).sum()) <= 1e-3 * y1.numel(), int((diff > 0).sum())
    # The ReLU masks of x and 2x are identical unless a hidden activation underflows for x but not for 2x, which
    # flips that sample's mask: all other rows of the input gradient double exactly.
    bad_rows = (g2 != 2.0 * g1).any(dim=1)
    assert int(bad_rows.sum()) <= max(2, int(1e-4 * n)), f"{int(bad_rows.sum())} rows of dL/dx are not exactly doubled"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("S,S_out", [(256, 96), (96, 48)], ids=["256->96", "96->48"])
def test_pdf_resampling_sorted_at_full_size(device, S, S_out, dtype):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _ptr, _stream

    st = _stream(device)
    g = torch.Generator().manual_seed(6)
    o = ((torch.rand(R, 3, generator=g) - 0.5) * 1.5).to(device)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(device)
    jit = torch.rand(R, generator=g).to(device)
    sb, tb = torch.empty(R, S + 1, device=device), torch.empty(R, S + 1, device=device)
    x = torch.empty(R * S, 3, device=device)
    _call("nvo_lindisp_positions", st, R, S, 0.05, 1000.0, _ptr(jit), _ptr(o), _ptr(d), _ptr(sb), _ptr(tb), _ptr(x))
    pre = (torch.randn(R * S, generator=g) * 3).to(DTYPES[dtype]).to(device)
    pre.view(R, S)[:7] = -30.0   # rays whose density underflows to zero: the padded histogram must still be valid
    pre.view(R, S)[7:9, 100:102] = 11.0  # near-delta densities
    w = torch.empty(R * S, device=device)
    sbo, tbo = torch.empty(R, S_out + 1, device=device), torch.empty(R, S_out + 1, device=device)
    xo = torch.empty(R * S_out, 3, device=device)
    a = _lib.WeightsPdfArgs(
        R=R, S=S, S_out=S_out, pre=pre.data_ptr(), pre_stride=1, x01=x.data_ptr(), sbins=sb.data_ptr(),
        tbins=tb.data_ptr(), density_bias=-1.0, sigma=None, weights=w.data_ptr(), anneal=0.7,
        histogram_padding=0.01, near_plane=0.05, far_plane=1000.0, jitter=jit.data_ptr(),
        sbins_out=sbo.data_ptr(), tbins_out=tbo.data_ptr(), anneal_dev=None, origins=o.data_ptr(),
        directions=d.data_ptr(), x01_out=xo.data_ptr(), act_bf16=int(dtype == "bf16"))
    _call("nvo_weights_pdf", st, C.byref(a))
    torch.cuda.synchronize()
    for bins in (sb, sbo):
        assert torch.isfinite(bins).all() and float(bins.min()) >= 0.0 and float(bins.max()) <= 1.0
        assert bool((bins[:, 1:] >= bins[:, :-1]).all()), "normalised bins are not sorted"
    assert bool((tbo[:, 1:] >= tbo[:, :-1]).all()) and float(tbo.min()) >= 0.05 * (1 - 1e-6)
    w = w.view(R, S)
    assert float(w.min()) >= 0.0 and float(w.sum(dim=1).max()) <= 1.0 + 1e-4  # fp32 sum of S terms
    assert torch.isfinite(xo).all() and float(xo.min()) >= 0.0 and float(xo.max()) <= 1.0


def test_pixel_sampler_ranges_at_full_buffer(device):
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _ptr, _stream

    st = _stream(device)
    extent = torch.tensor([192.0, 480.0, 640.0], device=device)
    step = torch.zeros(1, device=device)
    idx = torch.empty(R, 3, dtype=torch.int64, device=device)
    jit = torch.empty(3, R, device=device)
    seen = []
    for s in (0.0, 1.0, 8191.0):
        step.fill_(s)
        _call("nvo_sample_pixels", st, R, 1234, _ptr(step), _ptr(extent), _ptr(idx), _ptr(jit), 3)
        torch.cuda.synchronize()
        assert int(idx.min()) >= 0 and bool((idx.max(dim=0).values < extent.long()).all())
        assert float(jit.min()) >= 0.0 and float(jit.max()) < 1.0
        # 4096 draws over 192 frames: every frame is hit (P(miss) ~ 192 * e^-21)
        assert idx[:, 0].unique().numel() == 192
        seen.append(idx.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


FULL_SIZE_CONFIGS = {
    # BASELINE.json configs[1]: Replica office0 full mapping loop, fp16, fixed poses (192 keyframes 640x480)
    "configs1-replica-f16-fixed-poses": dict(n=192, H=480, W=640, dtype="f16", normals=False, poses=False),
    # configs[2]: the same with pose-gradient backprop (SE3 camera optimiser)
    "configs2-replica-f16-se3": dict(n=192, H=480, W=640, dtype="f16", normals=False, poses=True),
    # configs[4] (one GPU of it): ScanNet-shaped, depth + normal supervision, bf16 MLPs
    "configs4-scannet-bf16-normals": dict(n=512, H=240, W=320, dtype="bf16", normals=True, poses=False),
}


@pytest.mark.parametrize("name", list(FULL_SIZE_CONFIGS))
def test_graphed_step_at_full_size(device, name):
    """The hipGraph-replayed step bench.py times, at the FULL size of BASELINE configs[1] / [2] (192 keyframes of 640x480,
    fp16 MLPs, fixed poses / SE3 pose refinement: the headline workload) and configs[4] on one GPU (512 keyframes of
    240x320, /root/reference/configs/nerf_vo_scannet.yaml:15-17, depth AND monosdf normal supervision,
    /root/reference/nerf_vo/mapping/nerfstudio.py:68-69,77, bf16 MFMA MLPs + fp16 hash tables with fp32 / fixed-point
    gradient accumulation); 4096 rays.

    Size-independent properties: (1) every drawn pixel lies inside the keyframe buffer and the sampler reaches (nearly)
    all of it; (2) every loss term the configuration enables is present, finite and positive, the per-group skip flags
    stay 0 and all trained parameter groups move; (3) the graph-replayed step IS the eager step: from the same restored
    state the eager launch sequence on the SAME drawn rays and jitters reproduces every loss term to 1e-4 and the
    parameter update to 2e-3 relative L1 (float atomics: an entry whose gradient nearly cancels can flip its Adam
    step); (4) a second replay advances the schedule (anneal, bias corrections) and stays finite."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    c = FULL_SIZE_CONFIGS[name]
    n, H, W = c["n"], c["H"], c["W"]
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=c["normals"])
    seq = make_sequence(n, H, W, device=device)
    for lo in range(0, n, 24):  # tracker-sized ingests, as bench.py does
        hi = min(n, lo + 24)
        ds.update({"keyframe_indices": torch.arange(lo, hi), "camera_intrinsics": seq["camera_intrinsics"][lo:hi],
                   "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"][lo:hi]),
                   "frames_color": seq["frames_color"][lo:hi], "frames_depth": seq["frames_depth"][lo:hi],
                   **({"frames_normal": seq["frames_normal"][lo:hi]} if c["normals"] else {})})
    del seq
    assert ds.num_active_frames == n and ds.frames_color.shape == (n, H, W, 3)
    torch.manual_seed(4)
    eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, mlp_dtype=c["dtype"], expect_normals=c["normals"],
                                      optimize_poses=c["poses"]), device)
    if c["poses"]:  # (zero pose adjustments have a zero regulariser gradient and sit at exp_map's series branch: start off it)
        eng.view("camera_opt.pose_adjustment").copy_(1e-3 * torch.randn(n * 6, generator=torch.Generator().manual_seed(9)).to(device))
    state = [t.clone() for t in (eng.params, eng.params_half, eng.exp_avg, eng.exp_avg_sq)]

    def restore():
        for dst, src in zip((eng.params, eng.params_half, eng.exp_avg, eng.exp_avg_sq), state):
            dst.copy_(src)
        eng.opt_steps = {g: 0 for g in eng.opt_steps}
        eng.step, eng.steps_since_proposal_update = 0, 0

    assert eng.train_step_graphed(ds) is True  # step 0 refreshes the proposal networks
    torch.cuda.synchronize()
    key = next(k for k in eng._graphs if k[1])  # the variant that just ran (with the proposal update)
    assert key[4] is bool(c["normals"]), "the captured step's normal supervision does not follow the configuration"
    if eng._graphs[key].get("pipelined"):
        # the graph already ran the sampling prefix of step 1 beside the optimiser: draw step 0's rays again (the
        # sampler is a stateless function of (seed, step)) so that the eager step below sees the same pixels
        eng._write_sampling_scalars(0)
        eng._graphs[key]["head"].replay()
        eng._pending_head = None
        torch.cuda.synchronize()
    _, drawn, jit, _, _ = eng._graphs[key]["buffers"]
    idx, jit = drawn.clone(), jit.clone()
    assert int(idx.min()) >= 0 and bool((idx.max(dim=0).values < torch.tensor([n, H, W], device=device)).all())
    # 4096 draws over n frames: E[missed] = n e^(-4096 / n) -- 0.17 of 512, 1e-7 of 192
    assert idx[:, 0].unique().numel() >= (500 if n == 512 else n)
    ws = eng._workspace(R, True)
    if c["normals"]:
        gn = ws["gt_normal"]
        assert float(gn.min()) >= 0.0 and float(gn.max()) <= 1.0  # (n + 1) / 2 colour space
        assert float(((gn * 2 - 1).norm(dim=1) - 1).abs().max()) < 1e-3, "gathered normal targets are not unit vectors"
    graph_losses = eng.loss_dict()
    terms = ["rgb_loss", "distortion_loss", "depth_loss", "interlevel_loss"] + (["normal_loss"] if c["normals"] else []) + (
        ["camera_opt_regularizer"] if c["poses"] else [])
    for term in terms:
        assert term in graph_losses and np.isfinite(graph_losses[term]) and graph_losses[term] > 0.0, (term, graph_losses)
    assert int(eng.skip_flag.sum()) == 0
    upd_graph = (eng.params - state[0]).double()
    for g in ("fields", "proposal_networks") + (("camera_opt",) if c["poses"] else ()):
        lo, hi = eng.group_ranges[g]
        assert float(upd_graph[lo:hi].abs().max()) > 0.0, f"group {g} did not move"
    if not c["poses"]:
        lo, hi = eng.group_ranges["camera_opt"]
        assert float(upd_graph[lo:hi].abs().max()) == 0.0, "fixed poses moved"

    restore()
    c2w = ds.camera_extrinsics[:, :3, :4].contiguous()
    eng.train_step(idx, ds.camera_intrinsics, c2w, ds.frames_color, ds.frames_depth, jitters=(jit[0], jit[1], jit[2]),
                   normals=ds.world_normals01() if c["normals"] else None)
    torch.cuda.synchronize()
    eager_losses = eng.loss_dict()
    for term, v in graph_losses.items():
        assert abs(eager_losses[term] - v) <= 1e-4 * abs(v) + 1e-9, (term, v, eager_losses[term])
    upd_eager = (eng.params - state[0]).double()
    rel = float((upd_eager - upd_graph).abs().sum() / upd_graph.abs().sum())
    assert rel < 2e-3, f"graph-replayed and eager step differ by {rel:.3e} (relative L1 of the parameter update)"

    restore()
    eng.train_step_graphed(ds)
    s0 = eng.dev_scalars.clone()
    eng.train_step_graphed(ds)
    torch.cuda.synchronize()
    assert not torch.equal(s0, eng.dev_scalars) and bool(torch.isfinite(eng.params).all())
    assert all(np.isfinite(v) for v in eng.loss_dict().values()) and int(eng.skip_flag.sum()) == 0


def test_bench_dump_outputs_on_the_gpu(device, tmp_path):
    """`bench.py --gpus 1 --dump-outputs DIR` as a caller runs it, twice: the result line still reports the timed steps,
    every dumped array is finite with the step's shape, and the rendered rays of the replayed step are the same bit for
    bit in both runs (the losses to the order of their float-atomic shards)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NVO_BENCH_DRY")}
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--dump-outputs", str(out)], capture_output=True, text=True, env=env, timeout=600, cwd=root)
        assert res.returncode == 0, res.stderr[-3000:]
        line = json.loads(res.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        dumps.append({n[:-4]: np.load(out / n) for n in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == ["accumulation", "depth", "expected_depth", "losses", "rgb"]
    assert a["rgb"].shape == (R, 3) and all(a[n].shape == (R,) for n in ("depth", "expected_depth", "accumulation"))
    for n, v in a.items():
        assert np.isfinite(v).all(), n
    assert a["losses"][0] > 0, "the replayed step carries no colour loss"
    for n in ("rgb", "depth", "expected_depth", "accumulation"):
        assert np.array_equal(a[n], b[n]), f"{n} differs between two runs with the same arguments"
    np.testing.assert_allclose(a["losses"], b["losses"], rtol=1e-5, atol=1e-12)
