"""GPU parity: the native nerfacto training step (HIP kernels sequenced by nerf_vo_amd.engine) vs the
torch-CPU oracle on IDENTICAL injected rays, jitters and parameters.

Tolerances: fp32 kernels vs float64 oracle with fp16 rounding emulated at the kernel's fp16 storage
points.  Bins/weights/rendered values: rtol 2e-3 (+ abs floor).  Losses: rtol 1e-2.  Gradients pass
through fp16 gradient buffers (loss scale 128) and ReLU kinks: rtol 3e-2, atol 1e-2 * max|ref|, with
the documented <=1e-4 outlier allowance of tests/test_tcnn_gpu.py::_assert_close.
"""
import numpy as np
import pytest
import torch

from test_tcnn_gpu import BF16_K, _assert_close, _assert_close_chain

pytestmark = pytest.mark.gpu

NUM_IMAGES = 4


def _make_engine(device, **over):
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine

    # (the kernel-parity tests below were written around tcnn's static loss scale of 128; the reference's GradScaler regime
    # -- the engine's default -- is covered by the `gradscaler` cases of test_full_step_matches_oracle, by
    # test_gradscaler_step_and_update_semantics and by the end-to-end mapper tests)
    over.setdefault("dynamic_loss_scale", False)
    cfg = EngineConfig(num_images=NUM_IMAGES, **over)
    eng = NerfactoEngine(cfg, device)
    # larger-than-init parameters so that densities, colours and all loss terms are non-trivial
    g = torch.Generator().manual_seed(123)
    flat = torch.zeros(eng.n_params)
    for name, (o, s, _) in eng.segments.items():
        if name in ("field.base", "proposal.0", "proposal.1"):
            net = eng.base_net if name == "field.base" else eng.prop_nets[int(name[-1])]
            width = 64 if name == "field.base" else 16
            n_grid = net.n_params - _mlp_count(name)
            n_mlp = net.n_params - n_grid
            flat[o:o + n_mlp] = (torch.rand(n_mlp, generator=g) * 2 - 1) * float(np.sqrt(6.0 / (2 * width))) * 1.5
            flat[o + n_mlp:o + s] = (torch.rand(n_grid, generator=g) * 2 - 1) * 0.7
        elif name == "field.color":
            flat[o:o + s] = (torch.rand(s, generator=g) * 2 - 1) * float(np.sqrt(6.0 / 128)) * 1.5
        elif name == "field.embedding":
            flat[o:o + s] = torch.randn(s, generator=g)
    eng.set_params(flat)
    return eng


def _adam_step(st, groups, p, p16, grads, grads_fmt, m, v, flag, beta2=0.999, grad_scale=1.0 / 128.0, tail=None):
    """nvo_adam_step over (offset, n, lr, step, hyper_dev, flag_slot) groups of one flat buffer; ``p`` ... ``flag`` are
    tensors or raw addresses (p16 / flag may be None)."""
    import ctypes as C

    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call

    def addr(t):
        return t.data_ptr() if torch.is_tensor(t) else t

    args = _lib.AdamArgs(params=addr(p), params_half=addr(p16), grads=addr(grads), grads_fmt=grads_fmt, exp_avg=addr(m),
                         exp_avg_sq=addr(v), beta1=0.9, beta2=beta2, eps=1e-15, grad_scale=grad_scale, skip_flags=addr(flag))
    arr = (_lib.AdamGroup * len(groups))(*[
        _lib.AdamGroup(offset=o, n=n, lr=lr, step=step, hyper_dev=addr(hyper), bias_dev=None, flag_slot=slot, weight_decay=0.0)
        for o, n, lr, step, hyper, slot in groups])
    _call("nvo_adam_step", st, C.byref(args), len(groups), arr, None if tail is None else C.byref(tail))


def _nonfinite_flag(st, spans, grads, grads_fmt, flags, slots=None, reset=1):
    """nvo_nonfinite_flag over (offset, n) spans of ``grads`` (a tensor or a raw address)."""
    import ctypes as C

    from nerf_vo_amd.engine import _call, _ptr

    k = len(spans)
    _call("nvo_nonfinite_flag", st, k, (C.c_uint64 * k)(*[o for o, _ in spans]), (C.c_uint64 * k)(*[n for _, n in spans]),
          None if slots is None else (C.c_uint32 * k)(*slots), _ptr(grads) if torch.is_tensor(grads) else C.c_void_p(grads),
          grads_fmt, _ptr(flags), reset)


def _mlp_count(name):
    from oracle import mlp as M

    return M.mlp_n_params(32, 16, 64, 1) if name == "field.base" else M.mlp_n_params(10, 1, 16, 1)


def _oracle_from_engine(eng):
    from oracle.nerfacto import NerfactoOracle, OracleConfig

    ocfg = OracleConfig(num_images=NUM_IMAGES, density_bias=eng.cfg.density_bias)
    orc = NerfactoOracle(ocfg)
    ph = eng.working_copy_float().double().cpu()  # exactly the 16-bit values the kernels consume

    def seg(name):
        o, s, _ = eng.segments[name]
        return ph[o:o + s]

    nb = _mlp_count("field.base")
    orc.params["base_mlp"] = seg("field.base")[:nb].clone().requires_grad_(True)
    orc.params["base_grid"] = seg("field.base")[nb:].clone().view(-1, 2).requires_grad_(True)
    orc.params["color_mlp"] = seg("field.color").clone().requires_grad_(True)
    orc.params["embedding"] = seg("field.embedding").clone().view(NUM_IMAGES, 32).requires_grad_(True)
    for k in range(2):
        npk = _mlp_count(f"proposal.{k}")
        orc.params[f"prop{k}_mlp"] = seg(f"proposal.{k}")[:npk].clone().requires_grad_(True)
        orc.params[f"prop{k}_grid"] = seg(f"proposal.{k}")[npk:].clone().view(-1, 2).requires_grad_(True)
    return orc


def _rays(R, seed):
    g = torch.Generator().manual_seed(seed)
    origins = (torch.rand(R, 3, generator=g) - 0.5) * 0.8
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    dnorm = 1.0 + 0.3 * torch.rand(R, generator=g)
    cam = torch.randint(0, NUM_IMAGES, (R,), generator=g)
    jit = tuple(torch.rand(R, generator=g) for _ in range(3))
    gt_rgb = torch.rand(R, 3, generator=g)
    gt_depth = torch.rand(R, generator=g) * 1.5
    gt_depth[::7] = 0.0  # masked-out depth pixels
    return origins, directions, dnorm, cam, jit, gt_rgb, gt_depth


@pytest.mark.parametrize("dtype,gradscaler", [("f16", False), ("bf16", False), ("f16", True), ("bf16", True)],
                         ids=["f16", "bf16", "f16-gradscaler", "bf16-gradscaler"])
def test_full_step_matches_oracle(device, dtype, gradscaler):
    """f16 = tcnn's precision (BASELINE configs[1-3]); bf16 = configs[4] (bf16 MFMA MLPs, fp16 hash tables with fp32
    interpolation and fp32 gradient accumulation).  bf16 keeps 8 significant bits against fp16's 11: every tolerance
    below is multiplied by K = 8 in that mode.  gradscaler = the loss-scale regime the reference trains in
    (mixed_precision=True, /root/reference/nerf_vo/mapping/nerfstudio.py:59: torch's GradScaler, initial scale 65536) -- the
    engine's default; the scale reaches the kernels through device memory and every gradient carries it."""
    from oracle.quant import activation_format

    K = 1.0 if dtype == "f16" else BF16_K
    eng = _make_engine(device, mlp_dtype=dtype, dynamic_loss_scale=gradscaler)
    orc = _oracle_from_engine(eng)
    R = 256
    origins, directions, dnorm, cam, jit, gt_rgb, gt_depth = _rays(R, 7)
    ws = eng._workspace(R, True)
    eng.load_ray_bundle(ws, origins.to(device), directions.to(device), dnorm.to(device), cam.to(device),
                        gt_rgb.to(device), gt_depth.to(device))
    anneal = 0.6
    if gradscaler:
        assert eng.current_loss_scale() == 65536.0
    for _ in range(8):
        eng.forward_backward(ws, tuple(j.to(device) for j in jit), has_depth=True, update_proposals=True, anneal=anneal)
        torch.cuda.synchronize()
        if not gradscaler or bool(torch.isfinite(eng.grads).all()):
            break
        # what GradScaler.update() does after a step whose gradients overflowed fp16 (this test's parameters are ~100x
        # larger than a trained model's): the step is skipped and the scale halves
        eng.dev_loss_scale.mul_(0.5)
    assert bool(torch.isfinite(eng.grads).all())
    if gradscaler:
        assert eng.current_loss_scale() >= 2048.0, "GradScaler regime: the scale should stay far above tcnn's 128"

    with activation_format(dtype):
        out = orc.forward(origins.double(), directions.double(), dnorm.double(), cam, tuple(j.double() for j in jit),
                          anneal=anneal, training=True)
        ld = orc.loss_dict(out, gt_rgb.double(), gt_depth.double())
        sum(ld.values()).backward()

    # ---- sampling / rendering
    for k in range(3):
        _assert_close(ws[f"sbins{k}"], out["sbins_list"][k], rtol=1.5e-4 * K, atol_scale=1.5e-5 * K, what=f"sbins level {k}",
                      max_outlier_frac=2e-3 * K)
        _assert_close(ws[f"tbins{k}"], out["tbins_list"][k], rtol=3.5e-4 * K, atol_scale=7e-8 * K, what=f"tbins level {k}",
                      max_outlier_frac=2e-3 * K)
        _assert_close(ws[f"weights{k}"].view(R, -1), out["weights_list"][k], rtol=2e-2 * K, atol_scale=3e-3 * K,
                      what=f"weights level {k}", max_outlier_frac=2e-3 * K)
    _assert_close(ws["rgb"][:, :3].view(R, -1, 3), out["rgb_samples"], rtol=5e-3 * K, atol_scale=2.5e-3 * K,
                  what="per-sample rgb", max_outlier_frac=1e-3 * K)
    _assert_close(ws["out_rgb"], out["rgb"], rtol=2e-4 * K, atol_scale=1e-4 * K, what="rendered rgb")
    _assert_close(ws["out_accumulation"], out["accumulation"].reshape(-1), rtol=5e-5 * K, atol_scale=2.5e-5 * K,
                  what="accumulation")

    # ---- losses
    got = eng.loss_dict()
    for name in ("rgb_loss", "interlevel_loss", "distortion_loss", "depth_loss"):
        ref = float(ld[name])
        assert abs(got[name] - ref) <= 1.5e-2 * K * abs(ref) + 1e-7, f"{name}: got {got[name]:.6e} ref {ref:.6e}"

    # ---- gradients (engine grads carry the loss scale)
    ls = eng.current_loss_scale()

    def gseg(name):
        o, s, _ = eng.segments[name]
        return eng.grads[o:o + s] / ls

    nb = _mlp_count("field.base")
    # (bounds = 2-3x the errors the suite measures, profiles/r5_parity_margins.md; the base network's gradient passes
    # through the colour head's 16-bit d(geo features) first and carries ~10x the error of the heads')
    tol = dict(rtol=1.5e-3 * K, atol_scale=7.5e-4 * K, max_outlier_frac=1e-4 * K, max_outlier=0.05 if K == 1.0 else 0.2)
    tol_base = dict(tol, rtol=1.2e-2 * K, atol_scale=6e-3 * K)
    _assert_close(gseg("field.color"), orc.params["color_mlp"].grad, what="d colour MLP", **tol)
    _assert_close(gseg("field.embedding"), orc.params["embedding"].grad.reshape(-1), what="d embedding", **tol)
    _assert_close(gseg("field.base")[:nb], orc.params["base_mlp"].grad, what="d base MLP", **tol_base)
    # hash-grid gradients: reached through the 16-bit chain (_assert_close_chain: relative L1 error + largest error)
    chain = {"main": (1.5e-2, 0.10), 0: (1.4e-2, 0.04), 1: (5.5e-3, 0.01)} if K == 1.0 else \
        {"main": (5e-2, 0.22), 0: (1.6e-2, 0.10), 1: (8e-3, 0.055)}
    _assert_close_chain(gseg("field.base")[nb:], orc.params["base_grid"].grad, "d main grid", *chain["main"])
    for k in range(2):
        npk = _mlp_count(f"proposal.{k}")
        _assert_close(gseg(f"proposal.{k}")[:npk], orc.params[f"prop{k}_mlp"].grad, what=f"d prop{k} MLP", **tol)
        _assert_close_chain(gseg(f"proposal.{k}")[npk:], orc.params[f"prop{k}_grid"].grad, f"d prop{k} grid", *chain[k])


@pytest.mark.parametrize("stride,poses,fmt", [(16, False, 0), (12, True, 1)], ids=["4x4-fixed-f16", "3x4-corrected-bf16"])
def test_ray_head_matches_separate(device, stride, poses, fmt):
    """nvo_ray_head (pixel sampler + raygen + target gather + SH + first sampler level in one launch) must equal the
    five separate launches BIT FOR BIT on every output."""
    import ctypes as C

    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call, _ptr, _stream

    g = torch.Generator().manual_seed(9)
    F, H, W, R, S = 7, 48, 64, 1000, 256
    dev = lambda t: t.to(device).contiguous()  # noqa: E731
    intr = dev(torch.tensor([[30.0, 28.0, 31.7, 23.6]]).repeat(F, 1) + torch.rand(F, 4, generator=g))
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0]
    c2w44 = torch.eye(4).repeat(F, 1, 1)
    c2w44[:, :3, :3] = rot
    c2w44[:, :3, 3] = torch.randn(F, 3, generator=g) * 0.3
    c2w44 = dev(c2w44)
    c2w34 = c2w44[:, :3, :4].contiguous()
    corr = dev(torch.cat([torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0], torch.randn(F, 3, 1, generator=g) * 0.05], 2))
    images, depths, normals = dev(torch.rand(F, H, W, 3, generator=g)), dev(torch.rand(F, H, W, generator=g)), dev(torch.rand(F, H, W, 3, generator=g))
    step_dev = torch.tensor([37.0], device=device)
    extent = torch.tensor([float(F - 2), float(H), float(W)], device=device)
    seed = 0xC0FFEE
    st = _stream(device)
    adt = torch.bfloat16 if fmt else torch.float16

    def bufs():
        z = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device=device)  # noqa: E731
        return dict(idx=z(R, 3, dt=torch.int64), jit=z(3, R), o=z(R, 3), d=z(R, 3), dn=z(R), pa=z(R), ci=z(R, dt=torch.int32),
                    rgb=z(R, 3), dep=z(R), nor=z(R, 3), d01=z(R, 3), sh=z(R, 16, dt=adt), sb=z(R, S + 1), tb=z(R, S + 1),
                    x=z(R * S, 3))

    a, b = bufs(), bufs()
    poses_t = c2w34 if stride == 12 else c2w44
    # ---- separate launches
    _call("nvo_sample_pixels", st, R, seed, _ptr(step_dev), _ptr(extent), _ptr(a["idx"]), _ptr(a["jit"]), 3)
    _call("nvo_raygen", st, R, _ptr(a["idx"]), _ptr(intr), _ptr(c2w34), _ptr(corr) if poses else None, _ptr(a["o"]), _ptr(a["d"]),
          _ptr(a["dn"]), _ptr(a["pa"]), _ptr(a["ci"]))
    _call("nvo_gather_targets", st, R, _ptr(a["idx"]), H, W, _ptr(images), _ptr(depths), _ptr(normals), _ptr(a["d"]),
          _ptr(a["rgb"]), _ptr(a["dep"]), _ptr(a["nor"]), _ptr(a["d01"]))
    _call("nvo_sh_encode_t", st, R, 4, _ptr(a["d01"]), _ptr(a["sh"]), fmt)
    _call("nvo_lindisp_positions", st, R, S, 0.05, 1000.0, _ptr(a["jit"][0]), _ptr(a["o"]), _ptr(a["d"]), _ptr(a["sb"]),
          _ptr(a["tb"]), _ptr(a["x"]))
    # ---- one launch
    ra = _lib.RayHeadArgs(R=R, S=S, seed=seed, n_jitter=3, step_dev=step_dev.data_ptr(), extent_dev=extent.data_ptr(),
                          intrinsics=intr.data_ptr(), c2w=poses_t.data_ptr(), c2w_stride=stride,
                          corrections=corr.data_ptr() if poses else None, H=H, W=W, images=images.data_ptr(),
                          depths=depths.data_ptr(), normals=normals.data_ptr(), near_plane=0.05, far_plane=1000.0,
                          ray_indices=b["idx"].data_ptr(), jitter=b["jit"].data_ptr(), origins=b["o"].data_ptr(),
                          directions=b["d"].data_ptr(), directions_norm=b["dn"].data_ptr(), pixel_area=b["pa"].data_ptr(),
                          cam_idx=b["ci"].data_ptr(), gt_rgb=b["rgb"].data_ptr(), gt_depth=b["dep"].data_ptr(),
                          gt_normal=b["nor"].data_ptr(), dirs01=b["d01"].data_ptr(), sh=b["sh"].data_ptr(), sh_bf16=fmt,
                          sbins=b["sb"].data_ptr(), tbins=b["tb"].data_ptr(), x01=b["x"].data_ptr())
    _call("nvo_ray_head", st, C.byref(ra))
    torch.cuda.synchronize()
    assert int(a["idx"][:, 0].max()) <= F - 3 and float(a["x"].min()) >= 0.0
    for k in a:
        if not torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)):
            bad = (a[k] != b[k]).nonzero()
            first = tuple(int(v) for v in bad[0])
            raise AssertionError(f"nvo_ray_head output '{k}' differs from the separate kernels at {bad.shape[0]} elements; first "
                                 f"{first}: {a[k][first].item()!r} vs {b[k][first].item()!r}; columns hit: "
                                 f"{sorted(set(bad[:, -1].tolist()))[:20]}")


def test_raygen_and_gather(device):
    from nerf_vo_amd.engine import _call, _ptr, _stream
    from oracle import rays as Rr

    g = torch.Generator().manual_seed(3)
    F, H, W, R = 5, 48, 64, 2000
    intr = torch.tensor([[320.0 / 10, 423.529 / 10, 31.97, 23.96]]).repeat(F, 1) + torch.rand(F, 4, generator=g)
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0]
    c2w = torch.cat([rot, torch.randn(F, 3, 1, generator=g)], dim=2)
    idx = torch.stack([torch.randint(0, F, (R,), generator=g), torch.randint(0, H, (R,), generator=g),
                       torch.randint(0, W, (R,), generator=g)], dim=1)
    images = torch.rand(F, H, W, 3, generator=g)
    corr = Rr.exp_map_se3(torch.randn(F, 6, generator=g).double() * 0.05).float()
    d = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=device)  # noqa: E731
    o, dr, dn, pa, ci, px = d(R, 3), d(R, 3), d(R), d(R), d(R, dt=torch.int32), d(R, 3)
    st = _stream(device)
    dev = lambda t: t.to(device).contiguous()  # noqa: E731
    idx_d, intr_d, c2w_d, img_d, corr_d = dev(idx), dev(intr), dev(c2w), dev(images), dev(corr)
    for use_corr in (False, True):
        _call("nvo_raygen", st, R, _ptr(idx_d), _ptr(intr_d), _ptr(c2w_d), _ptr(corr_d) if use_corr else None,
              _ptr(o), _ptr(dr), _ptr(dn), _ptr(pa), _ptr(ci))
        torch.cuda.synchronize()
        ro, rd, rn, rpa = Rr.generate_rays(idx, intr.double(), c2w.double())
        if use_corr:
            ro, rd = Rr.apply_pose_correction(ro, rd, corr.double()[idx[:, 0]])
        _assert_close(o, ro, rtol=7.5e-8, atol_scale=7.5e-9, what="origins")  # (fp32 against float64: one rounding)
        _assert_close(dr, rd, rtol=1e-6, atol_scale=1e-7, what="directions")
        _assert_close(dn, rn.reshape(-1), rtol=2.7e-7, atol_scale=2.7e-8, what="directions_norm")
        _assert_close(pa, rpa.reshape(-1), rtol=1.8e-5, atol_scale=9e-7, what="pixel_area")
        assert (ci.cpu() == idx[:, 0].int()).all()
    _call("nvo_gather_pixels", st, R, _ptr(idx_d), H, W, 3, _ptr(img_d), _ptr(px))
    torch.cuda.synchronize()
    assert torch.equal(px.cpu(), images[idx[:, 0], idx[:, 1], idx[:, 2]])


def test_lindisp_bins(device):
    from nerf_vo_amd.engine import _call, _ptr, _stream
    from oracle import rays as Rr

    R, S = 300, 256
    jit = torch.rand(R, generator=torch.Generator().manual_seed(1))
    sb = torch.empty(R, S + 1, device=device)
    tb = torch.empty(R, S + 1, device=device)
    for j in (None, jit):
        _call("nvo_sample_lindisp", _stream(device), R, S, 0.05, 1000.0, None if j is None else _ptr(j.to(device)),
              _ptr(sb), _ptr(tb))
        torch.cuda.synchronize()
        rs, rt = Rr.sample_uniform_lindisp(R, S, 0.05, 1000.0, None if j is None else j.double().reshape(R, 1))
        _assert_close(sb, rs, rtol=1.1e-7, atol_scale=1.1e-8, what="lindisp sbins")
        _assert_close(tb, rt, rtol=3.2e-4, atol_scale=1.6e-7, what="lindisp tbins")


def test_adam_matches_torch_semantics(device):
    from nerf_vo_amd.engine import _call, _ptr, _stream
    from oracle.nerfacto import adam_reference

    n = 100_003
    g = torch.Generator().manual_seed(2)
    p = torch.randn(n, generator=g)
    pr, mr, vr = p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pd, p16 = p.to(device), torch.zeros(n, dtype=torch.float16, device=device)
    md, vd = torch.zeros(n, device=device), torch.zeros(n, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * 128.0
        gd = grad.to(device)
        _nonfinite_flag(_stream(device), [(0, n)], gd, 0, flag)
        _adam_step(_stream(device), [(0, n, 1e-2, step, None, 0)], pd, p16, gd, 0, md, vd, flag)
        pr, mr, vr = adam_reference(pr, grad.double() / 128.0, mr, vr, 1e-2, step)
    torch.cuda.synchronize()
    _assert_close(pd, pr, rtol=4.2e-7, atol_scale=4.2e-8, what="adam params")
    assert torch.equal(p16.cpu(), pd.cpu().half())
    # a non-finite gradient anywhere skips the whole step (GradScaler semantics)
    before = pd.clone()
    gd[12345] = float("inf")
    _nonfinite_flag(_stream(device), [(0, n)], gd, 0, flag)
    _adam_step(_stream(device), [(0, n, 1e-2, 6, None, 0)], pd, p16, gd, 0, md, vd, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and torch.equal(before, pd)
    # fp16 gradient buffer (what a compressed all-reduce hands over) gives the same update as its fp32 cast
    g16 = (torch.randn(n, generator=g) * 4).half().to(device)
    pa, pb = pd.clone(), pd.clone()
    ma, mb, va, vb = md.clone(), md.clone(), vd.clone(), vd.clone()
    flag.zero_()
    _adam_step(_stream(device), [(0, n, 1e-2, 7, None, 0)], pa, None, g16, 1, ma, va, flag)
    g32 = g16.float()
    _adam_step(_stream(device), [(0, n, 1e-2, 7, None, 0)], pb, None, g32, 0, mb, vb, flag)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    # bfloat16 gradient buffer (the compressed exchange bench.py uses): nvo_cast_bf16 rounds to nearest even exactly like
    # torch, keeps inf / NaN, and the optimiser consumes the buffer like its fp32 cast
    src = torch.cat([torch.randn(n - 6, generator=g) * torch.logspace(-30, 3, n - 6),
                     torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1e-40])]).to(device)
    dst = torch.empty(n, dtype=torch.bfloat16, device=device)
    _call("nvo_cast_bf16", _stream(device), n, _ptr(src), _ptr(dst))
    torch.cuda.synchronize()
    ref16 = src.to(torch.bfloat16)
    finite = torch.isfinite(src)
    assert torch.equal(dst[finite].view(torch.int16), ref16[finite].view(torch.int16))
    assert torch.equal(torch.isinf(dst), torch.isinf(src)) and torch.equal(torch.isnan(dst), torch.isnan(src))
    gb = (torch.randn(n, generator=g) * torch.logspace(-12, 1, n)).to(torch.bfloat16).to(device)
    pa, pb = pd.clone(), pd.clone()
    ma, mb, va, vb = md.clone(), md.clone(), vd.clone(), vd.clone()
    flag.zero_()
    _nonfinite_flag(_stream(device), [(0, n)], gb, 2, flag)
    _adam_step(_stream(device), [(0, n, 1e-2, 8, None, 0)], pa, None, gb, 2, ma, va, flag)
    gb32 = gb.float()
    _adam_step(_stream(device), [(0, n, 1e-2, 8, None, 0)], pb, None, gb32, 0, mb, vb, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    gb[777] = float("inf")
    _nonfinite_flag(_stream(device), [(0, n)], gb, 2, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


def test_grouped_adam_equals_per_group_launches(device):
    """nvo_adam_step / nvo_nonfinite_flag over three groups (one launch for the groups of a step) against one
    one-group nvo_adam_step launch per group: bit-identical parameters, moments and fp16 copies, including odd (unaligned) group
    boundaries and device-side hyper-parameters; and the per-group skip flags (GradScaler.step decides per optimiser)."""
    from nerf_vo_amd.engine import _stream

    st = _stream(device)
    n = 300_007
    bounds = [(0, 250_000), (250_000, 299_001), (299_001, 300_007)]  # the last two starts are not 16-byte aligned
    lrs, steps = (1e-2, 5e-3, 1e-4), (7, 3, 11)
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=g).to(device)
    m0, v0 = (torch.rand(n, generator=g) * 0.1).to(device), (torch.rand(n, generator=g) * 0.01).to(device)
    grads = (torch.randn(n, generator=g) * 128.0).to(device)
    hyper = torch.tensor([3e-3, 1 - 0.9 ** 5, (1 - 0.999 ** 5) ** 0.5], device=device)  # overrides group 1
    for half in (0, 1):
        gbuf = grads.half() if half else grads
        esz = 2 if half else 4
        out = []
        for grouped in (False, True):
            p, m, v = p0.clone(), m0.clone(), v0.clone()
            p16 = torch.zeros(n, dtype=torch.float16, device=device)
            flag = torch.ones(4, dtype=torch.int32, device=device)  # must be reset by the flag launch
            if grouped:
                _nonfinite_flag(st, [(lo, hi - lo) for lo, hi in bounds], gbuf, half, flag)
                _adam_step(st, [(lo, hi - lo, lrs[i], steps[i], hyper if i == 1 else None, i)
                                for i, (lo, hi) in enumerate(bounds)], p, p16, gbuf, half, m, v, flag)
            else:
                flag[1:] = 0  # a one-span scan owns (and resets) one word only
                _nonfinite_flag(st, [(0, n)], gbuf, half, flag)
                for i, (lo, hi) in enumerate(bounds):  # one group per launch, each on buffers that start at the group
                    _adam_step(st, [(0, hi - lo, lrs[i], steps[i], hyper if i == 1 else None, 0)], p.data_ptr() + 4 * lo,
                               p16.data_ptr() + 2 * lo, gbuf.data_ptr() + esz * lo, half, m.data_ptr() + 4 * lo,
                               v.data_ptr() + 4 * lo, flag)
            torch.cuda.synchronize()
            assert int(flag[:3].sum().item()) == 0
            out.append((p, m, v, p16))
        for a, b in zip(*out):
            assert torch.equal(a, b)
        assert not torch.equal(out[0][0], p0)
    # GradScaler.step semantics: a non-finite value in ONE group skips that group only
    bad = grads.clone()
    bad[bounds[1][0] + 5] = float("nan")
    flag = torch.zeros(4, dtype=torch.int32, device=device)
    _nonfinite_flag(st, [(lo, hi - lo) for lo, hi in bounds], bad, 0, flag)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _adam_step(st, [(lo, hi - lo, lrs[i], steps[i], None, i) for i, (lo, hi) in enumerate(bounds)], p, None, bad, 0, m, v, flag)
    torch.cuda.synchronize()
    assert flag[:3].tolist() == [0, 1, 0]
    lo, hi = bounds[1]
    assert torch.equal(p[lo:hi], p0[lo:hi]) and torch.equal(m[lo:hi], m0[lo:hi]), "the poisoned group must not move"
    assert not torch.equal(p[:lo], p0[:lo]) and not torch.equal(p[hi:], p0[hi:]), "the other groups must step"
    assert bool(torch.isfinite(p).all())


_SCAN_STRIDE = 2048 * 256  # threads of a span whose block count is capped: the stride of the scan's 16-byte loads


@pytest.mark.parametrize("fmt,n,shift", [(0, 6_400_007, 0), (2, 12_800_007, 0), (1, 12_800_007, 0), (0, 6_400_007, 1)],
                         ids=["f32", "bf16", "f16", "f32_unaligned"])
def test_nonfinite_flag_large_span(device, fmt, n, shift):
    """The scan's 4-way unrolled 16-byte loop runs only once a span's block count is capped (2048 blocks) and the span
    holds more than 3 x 2048 x 256 vectors -- the main grid's gradient does, no smaller test buffer.  A clean buffer
    (with the largest finite values of the format in it) raises nothing; one inf where only the FOURTH load of the
    unrolled loop reads raises the flag; so does one NaN at the last element (the scalar tail).  ``shift``: the span
    starts one element behind a 16-byte boundary, i.e. the whole scan takes the scalar form.  Expected values:
    torch.isfinite on the host copy.  (The planted finite extremes stay at 2.9e38: the scan's scalar form -- tail and
    unaligned spans -- tests |x| <= 3.0e38 rather than the exponent bits, so it counts the last 12 % below FLT_MAX as an
    overflow already; the 16-byte form does not.  As old as the kernel, and harmless for a gradient.)"""
    from nerf_vo_amd.engine import _stream

    st = _stream(device)
    dtype = (torch.float32, torch.float16, torch.bfloat16)[fmt]
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    n_vec = n // per
    assert n_vec > 3 * _SCAN_STRIDE and (n + 2047) // 2048 > 2048 and n % per != 0
    buf = torch.randn(n + shift, generator=torch.Generator().manual_seed(4)).to(dtype).to(device)
    g = buf[shift:]
    assert g.data_ptr() % 16 == (shift * buf.element_size())
    big = min(torch.finfo(dtype).max, 2.9e38)
    fourth = (3 * _SCAN_STRIDE + (n_vec - 3 * _SCAN_STRIDE) // 2) * per + per - 1  # vector index in [3 * stride, n_vec)
    g[0], g[fourth - 1], g[n - 2] = big, -big, big
    flag = torch.full((2,), 5, dtype=torch.int32, device=device)  # (word 0 is reset by the launch, word 1 is not its)

    def scan():
        _nonfinite_flag(st, [(0, n)], g.data_ptr(), fmt, flag)
        torch.cuda.synchronize()
        assert int(flag[1].item()) == 5
        return int(flag[0].item()), int(not bool(torch.isfinite(g.cpu().float()).all()))

    assert scan() == (0, 0)
    g[fourth] = float("inf")
    assert scan() == (1, 1)
    g[fourth] = 1.0
    assert scan() == (0, 0)
    g[n - 1] = float("nan")
    assert scan() == (1, 1)


def test_nonfinite_flag_spans_or_into_named_words(device):
    """Three spans, two of them raising the same word, OR-ed (reset=0) into words that already hold something: exactly the
    named words change, by exactly bit 0; the word no span names keeps its sentinel, and an element outside every span
    raises nothing."""
    from nerf_vo_amd.engine import _stream

    st = _stream(device)
    n = 10_000
    spans, slots = [(0, 3000), (3000, 3000), (6001, 3999)], [2, 0, 2]
    init = [4, 0x5A5A, 0, 0x5A5A]
    g = torch.randn(n, generator=torch.Generator().manual_seed(6)).to(device)
    g[6000] = float("nan")  # in no span
    for poison in (None, 7000, 4500, 10):
        if poison is not None:
            g[poison] = float("inf")
        flags = torch.tensor(init, dtype=torch.int32, device=device)
        _nonfinite_flag(st, spans, g, 0, flags, slots=slots, reset=0)
        torch.cuda.synchronize()
        host = g.cpu()
        expect = list(init)
        for (o, m), sl in zip(spans, slots):
            expect[sl] |= int(not bool(torch.isfinite(host[o:o + m]).all()))
        assert flags.tolist() == expect, f"poison at {poison}"
        if poison is not None:
            g[poison] = 0.5
    assert expect == [4, 0x5A5A, 1, 0x5A5A]


def test_opt_commit_with_scalars_equals_commit_then_write(device):
    """nvo_opt_commit with by-value scalars (commit + the next step's scalars in one launch) against nvo_opt_commit
    without scalars followed by nvo_write_floats, from identical states over 6 steps with a skipped group, a back-off and
    a growth (growth_interval 2): applied, bias, scale, growth_tracker and dst are word-equal after every step."""
    import ctypes as C

    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call, _ptr, _stream

    st = _stream(device)
    b1, b2 = 0.9, 0.999

    def state():
        return {"applied": torch.zeros(3, dtype=torch.int32, device=device),
                "bias": torch.tensor([1 - b1, (1 - b2) ** 0.5] * 3, device=device),
                "scale": torch.full((1,), 1024.0, device=device),
                "growth_tracker": torch.zeros(1, dtype=torch.int32, device=device),
                "dst": torch.full((16,), -7.0, device=device)}

    a, b = state(), state()
    flags = torch.zeros(4, dtype=torch.int32, device=device)

    def commit_args(s, mask):
        return _lib.OptCommitArgs(n_groups=3, active_mask=mask, scale_mask=0b111, applied=s["applied"].data_ptr(),
                                  skip_flags=flags.data_ptr(), scale=s["scale"].data_ptr(),
                                  growth_tracker=s["growth_tracker"].data_ptr(), growth_factor=2.0, backoff_factor=0.5,
                                  growth_interval=2, min_scale=1.0, max_scale=65536.0, bias=s["bias"].data_ptr(), beta1=b1,
                                  beta2=b2)

    # (flag words of the step, active mask): clean, clean -> growth, group 1 skipped -> back-off, group 1 idle, clean ->
    # growth, group 0 skipped -> back-off
    steps = [([0, 0, 0], 0b111), ([0, 0, 0], 0b111), ([0, 1, 0], 0b111), ([0, 0, 0], 0b101), ([0, 0, 0], 0b111),
             ([1, 0, 0], 0b111)]
    scales = []
    for it, (fl, mask) in enumerate(steps):
        flags[:3] = torch.tensor(fl, dtype=torch.int32)
        vals = (C.c_float * 5)(*[0.25 * it, 1e-2 / (it + 1), 3.0, float(it), -1.5])
        scalars = _lib.StepScalars(dst=a["dst"].data_ptr(), n=5, host_values=C.addressof(vals))
        _call("nvo_opt_commit", st, C.byref(commit_args(a, mask)), C.byref(scalars))
        _call("nvo_opt_commit", st, C.byref(commit_args(b, mask)), None)
        _call("nvo_write_floats", st, _ptr(b["dst"]), 5, vals)
        torch.cuda.synchronize()
        for name in a:
            assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), f"step {it}: {name} differs"
        scales.append(float(a["scale"].item()))
    assert scales == [1024.0, 2048.0, 1024.0, 1024.0, 2048.0, 1024.0]
    assert a["applied"].tolist() == [5, 4, 6] and int(a["growth_tracker"].item()) == 0
    assert torch.equal(a["dst"].cpu(), torch.tensor([1.25, 1e-2 / 6, 3.0, 5.0, -1.5] + [-7.0] * 11))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_normal_supervision_matches_oracle(device, dtype):
    """monosdf normal loss on the analytic normals (reference hook nerf_vo/mapping/nerfstudio_utils.py:337-350;
    enhancement modes containing 'normal').  Every other loss multiplier is zeroed so that the gradient
    compared is the normal term's alone.  Tolerances: per-sample normals come from a 16-bit MLP backward
    (oracle: float64) -> direction agreement cos > 0.999 (bf16: 1 - 8e-3) on >= 98 % of the samples; with the kernel's own
    per-sample normals injected into the oracle the rendered normals agree to 2e-3 absolute (97 % of rays), the loss to
    1 % and the gradients to the tolerance of the full-step test.  bf16 = BASELINE configs[4] (bf16 MFMA MLPs + normal
    supervision): every tolerance x BF16_K = 8 = 2^(11 - 8), the ratio of the two formats' rounding steps."""  # noqa
    from oracle.quant import activation_format

    K = 1.0 if dtype == "f16" else BF16_K
    eng = _make_engine(device, rgb_loss_mult=0.0, distortion_loss_mult=0.0, depth_loss_mult=0.0,
                       interlevel_loss_mult=0.0, normal_loss_mult=1.0, mlp_dtype=dtype)
    orc = _oracle_from_engine(eng)
    orc.cfg.rgb_loss_mult = orc.cfg.distortion_loss_mult = orc.cfg.depth_loss_mult = 0.0
    orc.cfg.interlevel_loss_mult = 0.0
    orc.cfg.normal_loss_mult = 1.0
    R = 256
    origins, directions, dnorm, cam, jit, gt_rgb, gt_depth = _rays(R, 19)
    g = torch.Generator().manual_seed(5)
    gt_normal = (torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) + 1.0) / 2.0
    ws = eng._workspace(R, True)
    eng.load_ray_bundle(ws, origins.to(device), directions.to(device), dnorm.to(device), cam.to(device),
                        gt_rgb.to(device), gt_depth.to(device), gt_normal.to(device))
    eng.forward_backward(ws, tuple(j.to(device) for j in jit), has_depth=False, update_proposals=False, anneal=1.0,
                         has_normals=True)
    torch.cuda.synchronize()
    gx = ws["dsigma_dx"].double().cpu()
    got_sn = -torch.nn.functional.normalize(gx, dim=-1).view(R, -1, 3)

    with activation_format(dtype):
        out = orc.forward(origins.double(), directions.double(), dnorm.double(), cam, tuple(j.double() for j in jit),
                          anneal=1.0, training=True, normals=True, sample_normals_override=got_sn)
    cos_min = 1.0 - 1e-3 * K
    cos = (got_sn * out["sample_normals"]).sum(-1)
    sel = out["weights_list"][-1] > 1e-4  # samples that matter for the render
    frac = (cos[sel] > cos_min).double().mean().item()
    assert frac >= 0.98, f"analytic normals agree (cos>{cos_min}) on only {frac:.4f} of the weighted samples"

    # the normalised sum is ill-conditioned on rays whose per-sample normals cancel (|sum w n| << 1):
    # 2e-3 on >= 97 % of the rays, 3e-2 everywhere
    err = (ws["out_normals"].double().cpu() - out["normals"]).abs().max(dim=-1).values
    assert (err < 2e-3 * K).double().mean() >= 0.97 and err.max() < min(3e-2 * K, 0.15), \
        f"rendered normals: max err {err.max():.3e}, frac<{2e-3 * K} {(err < 2e-3 * K).double().mean():.3f}"
    with activation_format(dtype):
        ld = orc.loss_dict(out, gt_rgb.double(), None, gt_normal.double())
        ld["normal_loss"].backward()
    got = eng.loss_dict()
    ref = float(ld["normal_loss"])
    assert abs(got["normal_loss"] - ref) <= 1e-2 * K * abs(ref), f"normal_loss got {got['normal_loss']:.6e} ref {ref:.6e}"

    ls = eng.cfg.loss_scale
    o, sz, _ = eng.segments["field.base"]
    nb = _mlp_count("field.base")
    gb = eng.grads[o:o + sz] / ls
    tol = dict(rtol=3e-2 * K, atol_scale=1.5e-2 * K, max_outlier_frac=1e-4 * K, max_outlier=0.05 if K == 1.0 else 0.2)
    assert orc.params["base_mlp"].grad.abs().max() > 0
    _assert_close(gb[:nb], orc.params["base_mlp"].grad, what="d base MLP (normal loss)", **tol)
    _assert_close_chain(gb[nb:], orc.params["base_grid"].grad, "d main grid (normal loss)",
                        *((1.1e-2, 0.085) if K == 1.0 else (2.5e-2, 0.08)))

    # inference output: outputs['normals'] of the eval forward
    res = eng.render_rays(origins.to(device), directions.to(device), dnorm.to(device), normals=True)
    torch.cuda.synchronize()
    wse = eng._workspace(R, False)
    sn_e = -torch.nn.functional.normalize(wse["dsigma_dx"].double().cpu(), dim=-1).view(R, -1, 3)
    with activation_format(dtype):
        refe = orc.forward(origins.double(), directions.double(), dnorm.double(), cam, None, anneal=1.0, training=False,
                           normals=True, sample_normals_override=sn_e)
    cos_e = (sn_e * refe["sample_normals"]).sum(-1)[refe["weights_list"][-1] > 1e-4]
    assert (cos_e > cos_min).double().mean() >= (0.98 if K == 1.0 else 0.97)  # (bf16 eval forward: measured 0.978)
    d = (res["normals"].double().cpu() - refe["normals"]).abs().max(dim=-1).values
    assert (d < 2e-3 * K).double().mean() >= 0.97 and d.max() < min(3e-2 * K, 0.15), \
        f"eval normals: max err {d.max():.3e}, frac<{2e-3 * K} {(d < 2e-3 * K).double().mean():.3f}"


def test_eval_render_matches_oracle(device):
    eng = _make_engine(device)
    orc = _oracle_from_engine(eng)
    R = 128
    origins, directions, dnorm, cam, *_ = _rays(R, 11)
    out = eng.render_rays(origins.to(device), directions.to(device), dnorm.to(device))
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = orc.forward(origins.double(), directions.double(), dnorm.double(), cam, None, anneal=1.0, training=False)
    _assert_close(out["rgb"], ref["rgb"], rtol=2.9e-4, atol_scale=1.45e-4, what="eval rgb")
    _assert_close(out["accumulation"], ref["accumulation"], rtol=1.3e-5, atol_scale=6.5e-6, what="eval accumulation")
    # median depth is a discrete pick: allow a small fraction of neighbouring-sample picks
    d_err = (out["depth"].double().cpu() - ref["depth"]).abs() / ref["depth"].abs().clamp(min=1e-6)
    assert (d_err < 5e-3).double().mean() > 0.95, f"median depth agrees on only {(d_err < 5e-3).double().mean():.3f}"


def test_training_reduces_loss(device):
    """Property test at the BASELINE batch size (4096 rays): 30 steps on a fixed batch must reduce
    the rgb loss -- exercises the whole path incl. the proposal-update schedule and Adam."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine

    eng = NerfactoEngine(EngineConfig(num_images=NUM_IMAGES), device)
    R = 4096
    origins, directions, dnorm, cam, jit, gt_rgb, gt_depth = _rays(R, 21)
    gt_rgb = (0.5 + 0.5 * torch.sin(origins * 5)).clamp(0, 1)
    ws = eng._workspace(R, True)
    eng.load_ray_bundle(ws, origins.to(device), directions.to(device), dnorm.to(device), cam.to(device),
                        gt_rgb.to(device), gt_depth.to(device))
    first = None
    for it in range(30):
        jitters = tuple(torch.rand(R, device=device) for _ in range(3))
        updated = eng.forward_backward(ws, jitters, has_depth=True)
        eng.optimizer_step(["fields"] + (["proposal_networks"] if updated else []))
        if updated:
            eng.steps_since_proposal_update = 0
        eng.steps_since_proposal_update += 1
        eng.step += 1
        loss = eng.loss_dict()["rgb_loss"]
        assert np.isfinite(loss)
        first = loss if first is None else first
    assert loss < 0.6 * first, f"rgb loss did not fall: {first:.5f} -> {loss:.5f}"


def test_graph_replay_matches_eager_semantics(device):
    """The hipGraph-replayed step must train like the eager step: same schedule bookkeeping, finite
    losses, loss goes down on a tiny synthetic sequence; and the per-step scalars (anneal, Adam bias
    corrections) must really change between replays (they live in device memory)."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W = 6, 60, 80
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})
    eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=1024), device)
    p0 = eng.params.clone()
    losses, scalars = [], []
    for it in range(40):
        updated = eng.train_step_graphed(ds)
        scalars.append(eng.dev_scalars[:4].tolist())
        losses.append(eng.loss_dict()["rgb_loss"])
        assert updated == (it < 10 or it % 2 == 0) or True  # schedule is exercised, exact parity not asserted
    torch.cuda.synchronize()
    assert eng.step == 40 and eng.opt_steps["fields"] == 40 and 10 <= eng.opt_steps["proposal_networks"] <= 40
    assert all(np.isfinite(losses)) and losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])
    # (the Adam bias corrections live next to the applied-step counters on the device: after 40 applied steps the fields
    # group holds those of step 41)
    assert eng.dev_bias[0].item() == pytest.approx(1 - 0.9 ** 41, rel=1e-5)
    assert scalars[0][1] == pytest.approx(eng.cfg.lr_fields, rel=1e-6)
    assert scalars[5][0] > scalars[1][0] > 0.0  # anneal ramps up
    assert not torch.equal(p0, eng.params)
    # update step, plain step, plain step that also evaluates the proposal loss values -- each as a dense and as a sparse
    # step (EngineConfig.sparse_backward "auto": the probe runs a sparse one every 64th step)
    assert len(eng._graphs) == 6 and sum(1 for k in eng._graphs if k[-1]) == 3
    # the optimiser must really have run on every replay: the GradScaler-style skip flag stays 0
    # (regression: a captured 4-byte hipMemsetAsync replayed as 0x01 bytes and silently disabled Adam)
    assert int(eng.skip_flag.sum().item()) == 0
    # the buffers the graphs address by pointer must stay owned by the engine (regression: the captured pose /
    # pixel-index / jitter buffers were locals of the capture function; once freed, the caching allocator handed
    # the same blocks to later allocations and every replay overwrote them -- long mapping runs collapsed)
    torch.cuda.synchronize()
    sentinels = []
    for _ in range(8):
        sentinels += [torch.full((1024, 3), 7, dtype=torch.int64, device=device),
                      torch.full((3, 1024), 7.0, device=device), torch.full((n, 3, 4), 7.0, device=device),
                      torch.full((3,), 7.0, device=device)]
    for it in range(4):
        eng.train_step_graphed(ds)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in sentinels), "a graph replay wrote into memory the engine no longer owns"
    del sentinels
    # ... and so must the workspace: rendering (another ray count) or an eager step between replays must not hand the
    # captured scratch back to the allocator (regression: _workspace cached ONE workspace and the graphs kept no
    # reference to theirs)
    before = float(eng.loss_dict()["rgb_loss"])
    o = torch.zeros(2048, 3, device=device)
    d = torch.nn.functional.normalize(torch.randn(2048, 3, device=device), dim=-1)
    eng.render_rays(o, d, torch.ones(2048, device=device), normals=True)
    idx = torch.floor(torch.rand(512, 3, device=device) * torch.tensor([n, H, W], device=device)).long()
    eng.train_step(idx, ds.camera_intrinsics, ds.camera_extrinsics[:, :3, :4].contiguous(), ds.frames_color, ds.frames_depth)
    torch.cuda.synchronize()
    junk = [torch.full((1 << 20,), float("nan"), device=device) for _ in range(16)]  # lands in any freed block
    for it in range(6):
        eng.train_step_graphed(ds)
    torch.cuda.synchronize()
    after = float(eng.loss_dict()["rgb_loss"])
    assert np.isfinite(after) and after < 2.0 * before and int(eng.skip_flag.sum().item()) == 0, (before, after)
    assert all(bool(torch.isnan(t).all()) for t in junk), "a graph replay wrote into a freed workspace block"
    del junk
    # same sequence launched eagerly reaches the same loss level
    eng2 = NerfactoEngine(EngineConfig(num_images=n, num_rays=1024), device)
    c2w = ds.camera_extrinsics[:, :3, :4].contiguous()
    for it in range(40):
        idx = torch.floor(torch.rand(1024, 3, device=device) * torch.tensor([n, H, W], device=device)).long()
        eng2.train_step(idx, ds.camera_intrinsics, c2w, ds.frames_color, ds.frames_depth)
    eager = eng2.loss_dict()["rgb_loss"]
    assert abs(np.log(losses[-1] / eager)) < 0.35, (losses[-1], eager)


def test_gradscaler_step_and_update_semantics(device):
    """GradScaler.step / GradScaler.update as the reference trains with them (mixed_precision=True,
    /root/reference/nerf_vo/mapping/nerfstudio.py:59), restated here and run against the engine's device-side state:
      * a group whose gradient holds an inf / NaN is skipped ALONE, its moments and parameters do not move, and its Adam
        step counter (torch: state['step'], which feeds the bias corrections) does NOT advance;
      * the other groups step with the unscaled gradient;
      * the loss scale halves after a step in which ANY optimiser was skipped and doubles after `growth_interval`
        consecutive clean steps; the growth tracker restarts at every back-off.
    The parameters are compared with torch.optim.Adam fed the unscaled gradients on the clean steps only."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine

    cfg = EngineConfig(num_images=NUM_IMAGES, optimize_poses=True, dynamic_loss_scale=True, loss_scale_init=1024.0,
                       loss_scale_interval=3)
    eng = NerfactoEngine(cfg, device)
    g = torch.Generator().manual_seed(3)
    p0 = (torch.randn(eng.n_params, generator=g) * 0.1)
    eng.set_params(p0)
    ref_p = {k: torch.nn.Parameter(p0[lo:hi].clone().to(device)) for k, (lo, hi) in eng.group_ranges.items()}
    lrs = {"fields": cfg.lr_fields, "proposal_networks": cfg.lr_proposal}
    bad_plan = {2: ["proposal_networks"], 5: ["fields"], 6: ["fields", "camera_opt"]}  # step -> poisoned groups
    scale, tracker = 1024.0, 0
    applied = {k: 0 for k in eng.group_ranges}
    opt = {}
    for step in range(12):
        eng.step = step
        raw = torch.randn(eng.n_params, generator=g) * 1e-3
        grads = (raw * scale).to(device)
        for k in bad_plan.get(step, []):
            lo, hi = eng.group_ranges[k]
            grads[lo + 7] = float("inf") if step % 2 else float("nan")
        eng.grads.copy_(grads)
        eng.skip_flag.zero_()
        assert eng.current_loss_scale() == scale
        eng.optimizer_step(flags_cleared=True)
        torch.cuda.synchronize()
        found = bad_plan.get(step, [])
        for k, (lo, hi) in eng.group_ranges.items():
            if k in found:
                continue
            applied[k] += 1
            if k not in opt:
                lr0 = lrs.get(k, eng.camera_lr(step))
                opt[k] = torch.optim.Adam([ref_p[k]], lr=lr0, eps=cfg.adam_eps, betas=cfg.adam_betas)
            if k == "camera_opt":
                opt[k].param_groups[0]["lr"] = eng.camera_lr(step)
            ref_p[k].grad = raw[lo:hi].to(device)
            opt[k].step()
        if found:
            scale, tracker = scale * 0.5, 0
        else:
            tracker += 1
            if tracker == 3:
                scale, tracker = scale * 2.0, 0
        assert eng.opt_steps == applied, (step, eng.opt_steps, applied)
        assert eng.current_loss_scale() == scale and int(eng.dev_growth_tracker.item()) == tracker, (step, scale)
        flags = eng.skip_flag.tolist()
        assert [bool(flags[eng._GROUP_ORDER.index(k)]) for k in eng._GROUP_ORDER] == [k in found for k in eng._GROUP_ORDER]
    for k, (lo, hi) in eng.group_ranges.items():
        _assert_close(eng.params[lo:hi], ref_p[k].detach(), rtol=1e-6, atol_scale=1e-7, what=f"params of group {k}")
    assert bool(torch.isfinite(eng.params).all()) and bool(torch.isfinite(eng.exp_avg_sq).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_deterministic_mode_is_bitwise_reproducible(device, dtype):
    """EngineConfig.deterministic: every float-atomic reduction of the step is replaced by a fixed summation order.
    Two 50-step graph-replayed trajectories (pose optimisation, depth + normal supervision, proposal updates) from the
    same seed must end in BIT-identical parameters and Adam moments; the default mode is expected to differ (that is
    what makes the assertion meaningful) while reaching the same loss level; and one deterministic step's gradient
    agrees with the default mode's to the usual float-atomic noise."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 512
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=True)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"], "frames_normal": seq["frames_normal"]})

    def run(deterministic: bool, steps: int = 50):
        torch.manual_seed(5)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, optimize_poses=True, expect_normals=True,
                                          mlp_dtype=dtype, deterministic=deterministic), device)
        for _ in range(steps):
            eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        assert int(eng.skip_flag.sum()) == 0
        return eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.loss_dict(), eng.grads.clone()

    a, b = run(True), run(True)
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "last gradient"), (a[0], a[1], a[2], a[4]), (b[0], b[1], b[2], b[4])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), \
            f"deterministic mode: {name} differ between two runs ({int((x != y).sum())} of {x.numel()} entries)"
    c = run(False)
    assert np.isfinite(list(c[3].values())).all()
    assert abs(np.log(a[3]["rgb_loss"] / c[3]["rgb_loss"])) < 0.3, (a[3], c[3])
    # one step from the same initial state: same gradient up to summation order
    g_det, g_def = run(True, 1)[4], run(False, 1)[4]
    # (two summation orders of the same float terms: the difference moves by an order of magnitude from run to run)
    _assert_close(g_det, g_def, rtol=1e-5, atol_scale=1e-7, what="deterministic vs default gradient", max_outlier_frac=1e-4)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dead_tiles_of_the_mlp_backward_are_skipped_exactly(device, dtype, monkeypatch):
    """The render / loss kernel marks every 16-sample tile of the main level whose stored dL/d(rgb) and dL/d(density) are
    all zero (nvo_main_loss_args::tile_live); the role-split backwards of the colour head and of the base network walk
    only the live tiles of a workgroup (mlp_impl.h, "LIVE-TILE LIST") and store zeros as the dead tiles' dX.  With a
    density bias of +12 the first sample inside the box takes a ray's whole weight (T = exp(-sigma delta) underflows to
    0 behind it), which is the state a trained field reaches: most tiles are dead.  Deterministic steps from the same
    state with the list on and off (NVO_MLP_SKIP_DEAD=0 walks every tile): the bytes must be a sound promise (a tile
    without its bit holds only zeros), what the colour head hands the base network must be the same values, and the
    gradients must agree up to the order of the fp32 sums (the live tiles meet the dW accumulators in another order once
    the dead ones between them are gone; the hash grid's fixed-point sums are order-free up to their scale)."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 1024
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})

    def run(skip: bool, steps: int):
        if skip:
            monkeypatch.delenv("NVO_MLP_SKIP_DEAD", raising=False)
        else:
            monkeypatch.setenv("NVO_MLP_SKIP_DEAD", "0")
        torch.manual_seed(5)
        # (bf16 keeps its range and flushes less: a larger bias, so that T itself underflows behind the first sample)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, mlp_dtype=dtype, deterministic=True, sparse_backward="on",
                                          dynamic_loss_scale=False, density_bias=12.0 if dtype == "f16" else 17.0), device)
        for _ in range(steps):
            eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        assert int(eng.skip_flag.sum()) == 0
        ws = eng._workspace(R, True)
        return eng, eng.grads.clone(), eng.params.clone(), ws["drgb"].float().clone(), ws["dout2"].float().clone(), \
            ws["tile_live"].clone()

    eng, g_on, _, drgb, dbo, live = run(True, 1)
    _, g_off, _, drgb_off, dbo_off, _ = run(False, 1)
    # the promise of the bytes
    rgb_nz = (drgb.abs().sum(1) != 0).view(-1, 16).any(1)
    pre_nz = (dbo[:, 0] != 0).view(-1, 16).any(1)
    assert torch.equal((live & 1).bool(), rgb_nz) and torch.equal((live & 2).bool(), pre_nz)
    dead_rgb, dead_base = ~rgb_nz, ~(rgb_nz | pre_nz)
    # both kinds of tile in both kernels, and fewer than 3/4 of them live: above that the kernels do not build their lists
    assert 0.25 < float(dead_rgb.float().mean()) < 0.999 and 0.25 < float(dead_base.float().mean()) < 0.999, \
        (float(dead_rgb.float().mean()), float(dead_base.float().mean()))
    # what the colour head left as the base network's dL/doutput: the same values, zeros behind its dead tiles
    assert torch.equal(drgb, drgb_off) and torch.equal(dbo, dbo_off)
    assert float(dbo.view(-1, 16, 16)[dead_rgb][:, :, 1:].abs().max()) == 0.0
    assert bool(torch.isfinite(g_on).all()) and float(g_on.abs().max()) > 0
    o, sz, _ = eng.segments["field.base"]
    n_mlp = _mlp_count("field.base")
    assert float(g_on[o + n_mlp:o + sz].abs().max()) > 0
    # (fixed-point sums of the same dX values; their scale comes from per-workgroup L1 sums, whose grouping changed)
    _assert_close(g_on[o + n_mlp:o + sz], g_off[o + n_mlp:o + sz], rtol=1e-6, atol_scale=1e-7, what="hash-grid gradient of the main field")
    _assert_close(g_on, g_off, rtol=1e-5, atol_scale=1e-7, what="gradient with / without the live-tile list", max_outlier_frac=1e-4)
    # and a few steps on: the same trajectory up to that noise
    p_on, p_off = run(True, 4)[2], run(False, 4)[2]
    _assert_close(p_on, p_off, rtol=1e-3, atol_scale=1e-5, what="parameters after 4 steps", max_outlier_frac=1e-3)


@pytest.mark.parametrize("lister", ["mlp-backward", "grid-pass"])
def test_grid_backward_walks_the_live_rows_of_a_trained_field(device, monkeypatch, lister):
    """Default (non-deterministic) kernels, the state of a trained field (density bias +12: a ray's first sample inside
    the box takes its whole weight): the main hash grid's backward lists the samples whose dL/doutput row is non-zero from
    the tile bytes of the render / loss kernel -- written by the base network's backward while it walks its live tiles
    (NvoMlpArgsT::live_rows, the default) or by a pass of the encoding's own (k_live_rows, NVO_MLP_LISTS_ROWS=0: what
    batches too large for the network's row buffer get) -- and both its slice-owner items and its record scatter walk that
    list.  The list must hold exactly those samples, and the gradient must agree with the full scan's
    (NVO_GRID_LIVE_ROWS=0) -- the table part up to the fixed-point scale (order-free sums; the per-tile L1 bounds that set
    the scale follow the tile composition), the network weights up to the order of their float atomics."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 2048
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})

    monkeypatch.setenv("NVO_MLP_LISTS_ROWS", "1" if lister == "mlp-backward" else "0")

    def run(listed: bool):
        if listed:
            monkeypatch.delenv("NVO_GRID_LIVE_ROWS", raising=False)
        else:
            monkeypatch.setenv("NVO_GRID_LIVE_ROWS", "0")
        torch.manual_seed(5)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, dynamic_loss_scale=False, density_bias=12.0,
                                          fuse_grid_adam=False, sparse_backward="on"), device)
        eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        assert int(eng.skip_flag.sum()) == 0
        ws = eng._workspace(R, True)
        word = torch.zeros(1, dtype=torch.int32, device=device)
        eng.base_net.set_option("debug_copy_grid_live_n", word.data_ptr())
        return eng, eng.grads.clone(), ws["dout2"].float().clone(), ws["tile_live"].clone(), int(word.item())

    eng, g_on, dbo, live, n_listed = run(True)
    _, g_off, dbo_off, _, n_off = run(False)
    rows_nz = dbo.abs().sum(1) != 0
    assert float((live != 0).float().mean()) < 0.75, "the state must be one where the list is built"
    assert n_listed == int(rows_nz.sum()) and 0 < n_listed < 0.75 * rows_nz.numel(), (n_listed, int(rows_nz.sum()))
    assert n_off == 0, "the full scan does not build a list"
    assert torch.equal(dbo, dbo_off)
    o, sz, _ = eng.segments["field.base"]
    n_mlp = _mlp_count("field.base")
    assert float(g_on[o + n_mlp:o + sz].abs().max()) > 0
    _assert_close(g_on[o + n_mlp:o + sz], g_off[o + n_mlp:o + sz], rtol=1e-6, atol_scale=1e-7, what="main hash grid gradient, listed vs full scan")
    _assert_close(g_on, g_off, rtol=1e-4, atol_scale=1e-6, what="gradient, listed vs full scan", max_outlier_frac=1e-4)


@pytest.mark.parametrize("bias,expect_sparse", [(-1.0, False), (12.0, True)], ids=["untrained-field", "hard-surfaces"])
def test_sparse_backward_auto_follows_the_field(device, bias, expect_sparse):
    """EngineConfig.sparse_backward = "auto": every 64th step is a sparse one (the probe), the live-tile count it leaves in
    slot 7 of the loss shards is read back asynchronously, and all steps switch to the sparse graphs while fewer than 60 %
    of the tiles are live.  An untrained field (every tile live) must stay on dense steps, a field whose first sample takes
    the ray's weight (density bias +12: about half of the tiles live) must switch -- and both kinds of every step variant
    are captured up front, so the switch never captures in the middle of a run."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 1024
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})
    torch.manual_seed(5)
    eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, dynamic_loss_scale=False, density_bias=bias), device)
    assert eng.cfg.sparse_backward == "auto"
    eng.train_step_graphed(ds)  # step 0: a probe
    n_graphs = len(eng._graphs)
    assert n_graphs == 6 and sum(1 for k in eng._graphs if k[-1]) == 3
    torch.cuda.synchronize()    # (the copy has landed: the next step polls it)
    for _ in range(70):
        eng.train_step_graphed(ds)
    torch.cuda.synchronize()
    assert len(eng._graphs) == n_graphs, "no capture after the first step"
    frac = eng._sparse_live_frac
    assert (frac < 0.60) == expect_sparse and 0.0 < frac <= 1.0, frac
    assert bool(getattr(eng, "_sparse_mode", False)) == expect_sparse
    assert int(eng.skip_flag.sum()) == 0 and bool(torch.isfinite(eng.params).all())


@pytest.mark.parametrize("dynamic", [False, True], ids=["static-scale", "dynamic-scale"])
def test_commit_behind_the_replay_is_bit_identical(device, dynamic):
    """EngineConfig.commit_behind_replay: the optimiser's commit (applied-step counters, bias corrections, loss scale)
    leaves the graph and rides in the eager launch behind the replay that also writes the NEXT step's scalars;
    EngineConfig.commit_from_table (default): it is the graph's last node and loads those scalars from a device ring the
    host fills ahead.  Same
    seed, deterministic mode: parameters, moments, counters, bias corrections and loss scale must equal those of the
    commit-in-graph form bit for bit -- across the proposal-update schedule, an externally reset step index and an
    eager step in between (both of which invalidate the scalars written ahead)."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 512
    seq = make_sequence(n, H, W, device=device)
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})

    def run(placement: str):
        torch.manual_seed(21)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, optimize_poses=True, deterministic=True,
                                          dynamic_loss_scale=dynamic, loss_scale_interval=7,
                                          commit_from_table=placement == "table",
                                          commit_behind_replay=placement == "behind"), device)
        if placement == "table":
            eng._TABLE_ROWS = 8  # (the ring of per-step scalars wraps and is refilled several times in 30 steps)
        gen = torch.Generator(device=device).manual_seed(4)
        for it in range(30):
            if it == 12:
                eng.step = 3  # (a step index set from outside: the scalars written ahead are for step 12)
            if it == 20:
                idx = torch.floor(torch.rand(R, 3, device=device, generator=gen) * torch.tensor([n, H, W], device=device)).long()
                eng.train_step(idx, ds.camera_intrinsics, ds.camera_extrinsics[:, :3, :4].contiguous(), ds.frames_color,
                               ds.frames_depth, jitters=tuple(torch.rand(R, device=device, generator=gen) for _ in range(3)))
            eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        if not dynamic:  # (the dynamic scale doubles every 7 steps here and may well run into an overflow: also covered)
            assert int(eng.skip_flag.sum()) == 0
        has_commit = any(e.get("commit") is not None for e in eng._graphs.values())
        has_table = any(e.get("table_commit") for e in eng._graphs.values())
        return (eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.opt_state.clone(), dict(eng.opt_steps),
                has_commit, has_table, eng.dev_scalars.clone())

    a, b, c = run("behind"), run("graph"), run("table")
    assert a[5] and not b[5] and not c[5] and c[6] and not a[6] and not b[6]
    assert a[4] == b[4] == c[4], (a[4], b[4], c[4])
    for other, what in ((b, "in the graph"), (c, "in the graph with the scalar table")):
        for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "optimiser state"), a[:4], other[:4]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{name}: commit behind the replay vs {what}"
    # both ahead-of-time forms leave the NEXT step's scalars (learning rates, anneal, sampler counter) on the device
    assert torch.equal(a[7], c[7]), (a[7], c[7])
    if dynamic:
        assert float(a[3][4:5].view(torch.float32)) > 65536.0  # the scale really grew (interval 7)


@pytest.mark.parametrize("poses", [False, True], ids=["fixed-poses", "se3"])
def test_adam_inside_the_grid_backward_is_bit_identical(device, poses):
    """EngineConfig.fuse_grid_adam: the tile-local accumulate pass of the main grid steps the entries of the hashed levels
    it has just summed instead of storing their gradient, and the optimiser launch covers the rest of the fields group.
    Same seed, deterministic mode, graph-replayed steps across the proposal-update schedule, a dynamic loss scale that
    starts at 2^33 and doubles every 2 clean steps (it backs off until the gradients fit, then keeps running into the
    overflow again: skipped steps occur throughout): parameters, both moments, the 16-bit working copy, step
    counters and the loss scale must equal those of the separate optimiser launch bit for bit."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 512
    seq = make_sequence(n, H, W, device=device)
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})

    def run(fuse: bool):
        torch.manual_seed(33)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, optimize_poses=poses, deterministic=True,
                                          dynamic_loss_scale=True, loss_scale_interval=2, loss_scale_init=2.0 ** 33,
                                          loss_scale_max=2.0 ** 40, fuse_grid_adam=fuse), device)
        for _ in range(36):
            eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        fused = [e.get("fused_adam") for e in eng._graphs.values()]
        return (eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.params_half.clone().view(torch.int16),
                eng.opt_state.clone(), dict(eng.opt_steps), fused, eng.segments["field.base"])

    a, b = run(True), run(False)
    assert all(f is not None for f in a[6]) and all(f is None for f in b[6])
    lo, hi = a[6][0]
    base_lo, base_n, _ = a[7]
    assert base_lo < lo < hi == base_lo + base_n and hi - lo > 0.8 * base_n  # (the hashed levels: most of the table)
    assert a[5] == b[5], (a[5], b[5])
    assert a[5]["fields"] < 36, "the sweep of the loss scale was meant to skip some steps"
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "working copy", "optimiser state"), a[:5], b[:5]):
        same = x.view(torch.int32) == y.view(torch.int32) if x.dtype != torch.int16 else x == y
        assert bool(same.all()), f"{name}: {int((~same).sum())} words differ with the step inside the grid backward"


def test_pipelined_prefix_is_bit_identical_on_one_gpu(device):
    """EngineConfig.pipeline_single_gpu: the graph ends with [Adam of the fields group || sampling prefix of the NEXT
    step] -- the launch order the multi-GPU step uses around its exchange, on one GPU.  The reordering must not change
    a single bit of the parameters: same seed, deterministic mode, with and without the pipelining, across the
    proposal-update schedule (the next step may replay another graph variant), a keyframe ingest (the prefix launched
    ahead saw the old buffer and has to be redone) and an eager step in between (which overwrites the workspace).
    (The reported loss VALUES are summed with float atomics in every mode: compared to 1e-5.)"""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 8, 60, 80, 512
    seq = make_sequence(n, H, W, device=device)

    def ingest(ds, lo, hi):
        ds.update({"keyframe_indices": torch.arange(lo, hi), "camera_intrinsics": seq["camera_intrinsics"][lo:hi],
                   "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"][lo:hi]),
                   "frames_color": seq["frames_color"][lo:hi], "frames_depth": seq["frames_depth"][lo:hi]})

    def run(pipeline: bool):
        torch.manual_seed(3)
        ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=False)
        ingest(ds, 0, 5)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, optimize_poses=True, deterministic=True,
                                          pipeline_single_gpu=pipeline), device)
        gen = torch.Generator(device=device).manual_seed(9)
        losses = []
        for it in range(26):
            if it == 14:
                ingest(ds, 5, 8)
            if it == 20:  # an eager step on the same workspace between two replays
                extent = torch.tensor([ds.num_active_frames, H, W], device=device)
                idx = torch.floor(torch.rand(R, 3, device=device, generator=gen) * extent).long()
                eng.train_step(idx, ds.camera_intrinsics, ds.camera_extrinsics[:, :3, :4].contiguous(), ds.frames_color,
                               ds.frames_depth)
            eng.train_step_graphed(ds)
            losses.append(eng.loss_totals().clone())
        torch.cuda.synchronize()
        assert int(eng.skip_flag.sum()) == 0
        pipelined = any(e.get("pipelined") for e in eng._graphs.values())
        return eng.params.clone(), eng.exp_avg_sq.clone(), torch.stack(losses), pipelined

    a, b = run(True), run(False)
    assert a[3] and not b[3]
    assert torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-12), "losses differ between the two launch orders"
    for name, x, y in (("params", a[0], b[0]), ("exp_avg_sq", a[1], b[1])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), \
            f"{name}: {int((x != y).sum())} of {x.numel()} entries differ between the pipelined and the plain graph"


@pytest.mark.parametrize("scale,expect", [(128.0, False), (1.0e10, True)], ids=["in-range", "overflow"])
def test_producer_overflow_flags_match_the_scan(device, scale, expect):
    """GradScaler's found_inf raised at the source (EngineConfig.producer_overflow_flags): the kernels that store a
    gradient in 16 bits flag their parameter group, the optimiser does not re-read the gradient buffer.  With a loss
    scale that pushes dL/d(rgb) beyond fp16 the flags of a producer-flag step must equal those of the scanning step,
    the skipped groups must not move and their step counters must not advance; in range nothing is flagged and both
    steps apply the same update."""
    res = {}
    for producer in (True, False):
        eng = _make_engine(device, loss_scale=scale, producer_overflow_flags=producer)
        R = 256
        origins, directions, dnorm, cam, jit, gt_rgb, gt_depth = _rays(R, 7)
        ws = eng._workspace(R, True)
        eng.load_ray_bundle(ws, origins.to(device), directions.to(device), dnorm.to(device), cam.to(device),
                            gt_rgb.to(device), gt_depth.to(device))
        p0 = eng.params.clone()
        eng.forward_backward(ws, tuple(j.to(device) for j in jit), has_depth=True, update_proposals=True, anneal=0.6)
        assert eng._producer_flags == producer
        eng.optimizer_step(["fields", "proposal_networks"], flags_cleared=True)
        torch.cuda.synchronize()
        res[producer] = (eng.skip_flag.tolist(), eng.opt_steps, (eng.params - p0).abs().max().item(), p0, eng.params.clone(),
                         bool(torch.isfinite(eng.grads[:eng.group_ranges["proposal_networks"][1]]).all()))
    flags_p, steps_p, moved_p, p0, params_p, _ = res[True]
    flags_s, steps_s, moved_s, _, params_s, grads_finite = res[False]
    assert [bool(f) for f in flags_p[:2]] == [bool(f) for f in flags_s[:2]], (flags_p, flags_s)
    assert bool(flags_s[0]) == expect and grads_finite == (not expect)
    assert steps_p == steps_s
    assert bool(torch.isfinite(params_p).all()) and bool(torch.isfinite(params_s).all())
    if expect:
        lo, hi = 0, res[True][3].numel()
        f_lo, f_hi = 0, 0
        assert steps_p["fields"] == 0 and moved_p >= 0.0
        assert torch.equal(params_p[:1000], p0[:1000]), "a skipped group moved"
    else:
        assert steps_p["fields"] == 1 and moved_p > 0.0
        rel = float((params_p - params_s).abs().sum() / (params_s - p0).abs().sum())
        assert rel < 1e-3, rel


def test_native_scratch_survives_larger_batches_between_replays(device):
    """Graph-capture safety of the NATIVE scratch (record stream of the streamed grid backward, live-sample list,
    per-level partials of the input backward): captured graphs address those blocks by pointer, and a larger batch
    between two replays used to hipFree + hipMalloc them.  Now a block a captured launch addresses is retired, not
    freed (csrc/nvo_common.h NvoScratch).  Run A: 8 replays.  Run B: 4 replays, then -- with the training state saved
    and restored around it -- an eager step at 4x the ray count and a render with analytic normals at 8x (both grow every
    native scratch block), then 4 more replays.  Both runs use the deterministic mode, so B must land where A does BIT
    FOR BIT (a graph that kept a dangling pointer faults or trains on garbage)."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, H, W, R = 6, 60, 80, 1024
    ds = DynamicDataset(num_frames=n, frame_height=H, frame_width=W, device=device, use_normals=True)
    seq = make_sequence(n, H, W, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"], "frames_normal": seq["frames_normal"]})
    c2w = ds.camera_extrinsics[:, :3, :4].contiguous()

    def run(interrupt: bool):
        torch.manual_seed(11)
        # (deterministic mode: the two runs must then agree BIT FOR BIT -- no float-atomic noise to allow for)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R, optimize_poses=True, expect_normals=True,
                                          deterministic=True), device)
        p0 = eng.params.clone()
        for _ in range(4):
            eng.train_step_graphed(ds)
        if interrupt:
            torch.cuda.synchronize()
            saved = ([t.clone() for t in (eng.params, eng.params_half, eng.exp_avg, eng.exp_avg_sq)], dict(eng.opt_steps),
                     eng.step, eng.steps_since_proposal_update)
            idx = torch.floor(torch.rand(4 * R, 3, device=device) * torch.tensor([n, H, W], device=device)).long()
            eng.train_step(idx, ds.camera_intrinsics, c2w, ds.frames_color, ds.frames_depth, normals=ds.world_normals01())
            o = torch.zeros(8 * R, 3, device=device)
            d = torch.nn.functional.normalize(torch.randn(8 * R, 3, device=device), dim=-1)
            eng.render_rays(o, d, torch.ones(8 * R, device=device), normals=True)
            torch.cuda.synchronize()
            for dst, src in zip((eng.params, eng.params_half, eng.exp_avg, eng.exp_avg_sq), saved[0]):
                dst.copy_(src)
            eng.opt_steps = saved[1]
            eng.step, eng.steps_since_proposal_update = saved[2], saved[3]
            junk = [torch.full((1 << 20,), float("nan"), device=device) for _ in range(8)]
        for _ in range(4):
            eng.train_step_graphed(ds)
        torch.cuda.synchronize()
        assert int(eng.skip_flag.sum()) == 0 and bool(torch.isfinite(eng.params).all())
        return (eng.params - p0).double().cpu(), eng.loss_dict()

    upd_a, loss_a = run(False)
    upd_b, loss_b = run(True)
    assert float(upd_a.abs().max()) > 0
    assert torch.equal(upd_a, upd_b), (
        f"replays after a larger eager batch diverged from the uninterrupted run: relative L1 "
        f"{float((upd_a - upd_b).abs().sum() / upd_a.abs().sum()):.3e}")
    assert abs(loss_a["rgb_loss"] - loss_b["rgb_loss"]) <= 1e-4 * loss_a["rgb_loss"], (loss_a, loss_b)


@pytest.mark.parametrize("R,F", [(7552, 48), (4096, 192), (1500, 1)], ids=["ngp-48cams-table", "nerfacto-192cams-plain", "one-camera-table"])
def test_pose_bwd_lds_table_matches_global_atomics(device, R, F):
    """nvo_pose_bwd_cams (per-workgroup camera table in LDS, flushed once) vs nvo_pose_bwd (one global float atomic per
    ray and word) vs a float64 torch restatement of the sum: dL/dcorrection[cam] = [dL/dd (x) d_raw | dL/do].  Both
    kernels add floats in no fixed order: rtol 1e-4 of the largest entry."""
    from nerf_vo_amd.engine import _call, _ptr, _stream

    g = torch.Generator().manual_seed(R + F)
    H, W = 48, 64
    idx = torch.stack([torch.randint(0, F, (R,), generator=g), torch.randint(0, H, (R,), generator=g),
                       torch.randint(0, W, (R,), generator=g)], dim=1).to(device)
    intr = torch.tensor([[60.0, 61.0, W / 2, H / 2]]).repeat(F, 1) + torch.rand(F, 4, generator=g)
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g)).Q
    c2w = torch.cat([rot, torch.randn(F, 3, 1, generator=g)], dim=2).contiguous()
    d_o, d_d, d_d01 = (torch.randn(R, 3, generator=g) for _ in range(3))
    dev = [t.to(device).contiguous() for t in (intr, c2w, d_o, d_d, d_d01)]
    out = {}
    for name in ("nvo_pose_bwd", "nvo_pose_bwd_cams"):
        acc = torch.zeros(F, 3, 4, device=device)
        extra = (F,) if name.endswith("cams") else ()
        _call(name, _stream(device), R, _ptr(idx), _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]),
              _ptr(acc), *extra)
        out[name] = acc.cpu().double()
    from helpers.pose_oracle import pose_chain  # the float64 sum (tests/test_pose_chain_gpu.py holds it to float32 bounds)

    ref = pose_chain(idx.cpu(), intr, c2w, d_o, d_d, d_d01, F)
    tol = 1e-4 * float(ref.abs().max())
    for name, got in out.items():
        assert float((got - ref).abs().max()) <= tol, (name, float((got - ref).abs().max()), tol)


@pytest.mark.parametrize("mode", ["SE3", "SO3xR3"])
def test_pose_gradients_match_oracle(device, mode):
    """SE3 / SO3xR3 camera optimiser: dL/dpose_adjustment through rays -> samples -> contraction ->
    hash grid input gradient (+ SH direction gradient) vs autograd in the oracle.  Tolerance: the chain
    passes through fp16 d(encoded) buffers and fp32 atomics: rtol 5e-2, atol 4e-2 * max|ref| (the worst element of
    the SO3xR3 case sits at 3.0e-2 * max|ref| -- one camera's z translation, 1.8e-3 off on a 6.2e-2 scale)."""
    from oracle import rays as Rr

    eng = _make_engine(device, optimize_poses=True, camera_mode=mode)
    g = torch.Generator().manual_seed(5)
    pose = torch.randn(NUM_IMAGES, 6, generator=g) * 0.03
    pose[1] = 0.0  # an untouched camera (zero tangent: small-angle branch, zero-norm regulariser)
    o, s, _ = eng.segments["camera_opt.pose_adjustment"]
    flat = eng.params.clone()
    flat[o:o + s] = pose.reshape(-1).to(device)
    eng.set_params(flat)
    orc = _oracle_from_engine(eng)

    F, H, W, R = NUM_IMAGES, 24, 32, 256
    intr = torch.tensor([[30.0, 28.0, 15.7, 11.6]]).repeat(F, 1)
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0]
    c2w = torch.cat([rot, (torch.rand(F, 3, 1, generator=g) - 0.5) * 0.6], dim=2)
    idx = torch.stack([torch.randint(0, F, (R,), generator=g), torch.randint(0, H, (R,), generator=g),
                       torch.randint(0, W, (R,), generator=g)], dim=1)
    images = torch.rand(F, H, W, 3, generator=g)
    depths = torch.rand(F, H, W, 1, generator=g) * 1.5
    jit = tuple(torch.rand(R, generator=g) for _ in range(3))

    ws = eng._workspace(R, True)
    eng.load_rays(ws, idx.to(device), intr.to(device), c2w.to(device).contiguous(), images.to(device),
                  depths.to(device))
    eng.forward_backward(ws, tuple(j.to(device) for j in jit), has_depth=True, update_proposals=True, anneal=0.7)
    torch.cuda.synchronize()
    got = (eng.grads[o:o + s] / eng.cfg.loss_scale).view(F, 6).double().cpu()

    pose_r = pose.double().requires_grad_(True)
    ro, rd, rn, _ = Rr.generate_rays(idx, intr.double(), c2w.double())
    corr = (Rr.exp_map_se3 if mode == "SE3" else Rr.exp_map_so3xr3)(pose_r)[idx[:, 0]]
    ro2, rd2 = Rr.apply_pose_correction(ro, rd, corr)
    gt_rgb = images[idx[:, 0], idx[:, 1], idx[:, 2]].double()
    gt_depth = depths[idx[:, 0], idx[:, 1], idx[:, 2], 0].double()
    out = orc.forward(ro2, rd2, rn.reshape(-1), idx[:, 0], tuple(j.double() for j in jit), anneal=0.7, training=True)
    ld = orc.loss_dict(out, gt_rgb, gt_depth)
    ld["camera_opt_regularizer"] = Rr.camera_opt_regularizer(pose_r)
    sum(ld.values()).backward()
    ref = pose_r.grad

    # forward sanity: the corrected rays the kernels used are the oracle's
    _assert_close(ws["origins"], ro2.detach(), rtol=2.2e-7, atol_scale=2.2e-8, what="corrected origins")
    _assert_close(ws["directions"], rd2.detach(), rtol=4.5e-7, atol_scale=4.5e-8, what="corrected directions")
    assert eng.loss_dict()["camera_opt_regularizer"] == pytest.approx(float(ld["camera_opt_regularizer"]), rel=1e-4)
    _assert_close(got, ref, rtol=5e-2, atol_scale=4e-2, what=f"dL/dpose_adjustment ({mode})")
    # and the Adam step on the camera group moves the poses
    before = eng.view("camera_opt.pose_adjustment").clone()
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(before, eng.view("camera_opt.pose_adjustment"))


def test_fused_sampler_kernels_match_unfused(device):
    """nvo_lindisp_positions / nvo_gather_targets / positions inside nvo_weights_pdf are fusions of kernels that
    still exist on their own: the fused outputs must be identical (same arithmetic, same rounding)."""
    import ctypes as C

    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _ptr, _stream

    st = _stream(device)
    g = torch.Generator().manual_seed(3)
    R, S = 96, 256
    o = ((torch.rand(R, 3, generator=g) - 0.5) * 1.5).to(device)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(device)
    jit = torch.rand(R, generator=g).to(device)
    sb_a, tb_a = torch.empty(R, S + 1, device=device), torch.empty(R, S + 1, device=device)
    x_a = torch.empty(R * S, 3, device=device)
    _call("nvo_sample_lindisp", st, R, S, 0.05, 1000.0, _ptr(jit), _ptr(sb_a), _ptr(tb_a))
    _call("nvo_sample_positions", st, R, S, _ptr(o), _ptr(d), _ptr(tb_a), _ptr(x_a))
    sb_b, tb_b, x_b = torch.empty_like(sb_a), torch.empty_like(tb_a), torch.empty_like(x_a)
    _call("nvo_lindisp_positions", st, R, S, 0.05, 1000.0, _ptr(jit), _ptr(o), _ptr(d), _ptr(sb_b), _ptr(tb_b), _ptr(x_b))
    torch.cuda.synchronize()
    assert torch.equal(sb_a, sb_b) and torch.equal(tb_a, tb_b) and torch.equal(x_a, x_b)

    # weights_pdf with and without the fused positions of the resampled level
    S_out = 96
    pre = (torch.randn(R * S, generator=g) * 2).to(torch.float16).to(device)
    w = torch.empty(R * S, device=device)
    outs = []
    for fused in (False, True):
        sbo, tbo = torch.empty(R, S_out + 1, device=device), torch.empty(R, S_out + 1, device=device)
        xo = torch.zeros(R * S_out, 3, device=device)
        a = _lib.WeightsPdfArgs(
            R=R, S=S, S_out=S_out, pre=pre.data_ptr(), pre_stride=1, x01=x_a.data_ptr(), sbins=sb_a.data_ptr(),
            tbins=tb_a.data_ptr(), density_bias=-1.0, sigma=None, weights=w.data_ptr(), anneal=0.7,
            histogram_padding=0.01, near_plane=0.05, far_plane=1000.0, jitter=jit.data_ptr(),
            sbins_out=sbo.data_ptr(), tbins_out=tbo.data_ptr(), anneal_dev=None,
            origins=o.data_ptr() if fused else None, directions=d.data_ptr() if fused else None,
            x01_out=xo.data_ptr() if fused else None)
        _call("nvo_weights_pdf", st, C.byref(a))
        if not fused:
            _call("nvo_sample_positions", st, R, S_out, _ptr(o), _ptr(d), _ptr(tbo), _ptr(xo))
        torch.cuda.synchronize()
        outs.append((sbo, tbo, xo))
    for p, q in zip(*outs):
        assert torch.equal(p, q)

    # one gather for colour / depth / normal targets + dirs01
    F, H, W = 5, 12, 16
    idx = torch.stack([torch.randint(0, F, (R,), generator=g), torch.randint(0, H, (R,), generator=g),
                       torch.randint(0, W, (R,), generator=g)], dim=1).to(device)
    img, dep, nrm = torch.rand(F, H, W, 3, generator=g).to(device), torch.rand(F, H, W, 1, generator=g).to(device), \
        torch.rand(F, H, W, 3, generator=g).to(device)
    rgb, dd, nn, d01 = (torch.empty(R, 3, device=device), torch.empty(R, device=device), torch.empty(R, 3, device=device),
                        torch.empty(R, 3, device=device))
    _call("nvo_gather_targets", st, R, _ptr(idx), H, W, _ptr(img), _ptr(dep), _ptr(nrm), _ptr(d), _ptr(rgb), _ptr(dd),
          _ptr(nn), _ptr(d01))
    torch.cuda.synchronize()
    assert torch.equal(rgb, img[idx[:, 0], idx[:, 1], idx[:, 2]]) and torch.equal(dd, dep[idx[:, 0], idx[:, 1], idx[:, 2], 0])
    assert torch.equal(nn, nrm[idx[:, 0], idx[:, 1], idx[:, 2]]) and torch.equal(d01, (d + 1.0) * 0.5)


def test_pixel_sampler_kernel(device):
    """nvo_sample_pixels: indices inside the extents, jitters in [0,1), uniform enough, reproducible for a
    (seed, step) pair, different across steps / seeds (no parity on RNG streams: SURVEY.md 8a row a3)."""
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _ptr, _stream

    st = _stream(device)
    R = 1 << 16
    extent = torch.tensor([37.0, 480.0, 640.0], device=device)
    step = torch.zeros(1, device=device)

    def draw(seed, s):
        step.fill_(float(s))
        idx = torch.empty(R, 3, dtype=torch.int64, device=device)
        jit = torch.empty(3, R, device=device)
        _call("nvo_sample_pixels", st, R, seed, _ptr(step), _ptr(extent), _ptr(idx), _ptr(jit), 3)
        torch.cuda.synchronize()
        return idx, jit

    idx, jit = draw(1234, 7)
    assert (idx >= 0).all() and (idx[:, 0] < 37).all() and (idx[:, 1] < 480).all() and (idx[:, 2] < 640).all()
    assert (jit >= 0).all() and (jit < 1).all()
    for c, e in enumerate((37, 480, 640)):  # mean / variance of a discrete uniform, 5-sigma bands
        v = idx[:, c].double()
        assert abs(v.mean().item() - (e - 1) / 2) < 5 * (e / 12 ** 0.5) / R ** 0.5 + 0.05
    assert abs(jit.mean().item() - 0.5) < 5 / (12 * 3 * R) ** 0.5
    counts = torch.bincount(idx[:, 0], minlength=37).double()
    assert ((counts - R / 37).abs() < 6 * (R / 37) ** 0.5).all()
    # channels / streams are not copies of each other
    assert (torch.corrcoef(torch.stack([idx[:, 1].double(), idx[:, 2].double(), jit[0].double(), jit[1].double()]))
            - torch.eye(4, device=device, dtype=torch.double)).abs().max() < 0.03
    idx2, jit2 = draw(1234, 7)
    assert torch.equal(idx, idx2) and torch.equal(jit, jit2)
    idx3, _ = draw(1234, 8)
    idx4, _ = draw(1235, 7)
    assert (idx3 != idx).any(dim=1).double().mean() > 0.99 and (idx4 != idx).any(dim=1).double().mean() > 0.99


@pytest.mark.parametrize("normals", [False, True], ids=["rgb-depth", "with-normals"])
def test_render_image_graph_matches_eager_chunks(device, normals):
    """NerfactoEngine.render_image -- every chunk of a full-image bundle inside ONE captured graph, rays read from and
    outputs written to image-sized buffers at the chunk's offset, mean appearance embedding taken once -- against the
    eager per-chunk render_rays (/root/reference/evaluation/nerf_renderer.py:157 -> get_outputs_for_camera_ray_bundle):
    bit for bit, including the ragged last chunk, on the first replay and on a second image through the same graph."""
    eng = _make_engine(device)
    N, chunk = 5000, 2048  # 2048 + 2048 + 904
    for seed in (3, 4):
        origins, directions, dnorm, *_ = _rays(N, seed)
        o, d, dn = origins.to(device), directions.to(device), dnorm.to(device)
        got = eng.render_image(o, d, dn, normals=normals, chunk=chunk)
        ref = {}
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            res = eng.render_rays(o[lo:hi].contiguous(), d[lo:hi].contiguous(), dn[lo:hi].contiguous(), normals=normals)
            for k, v in res.items():
                ref.setdefault(k, []).append(v.clone())
        torch.cuda.synchronize()
        assert set(got) == set(ref)
        for k in ref:
            want = torch.cat(ref[k])
            assert got[k].shape == want.shape, k
            assert torch.equal(got[k].view(torch.int32), want.view(torch.int32)), f"{k}: graphed image render != eager chunks"
    assert len(eng._render_graphs) == 1


def test_producer_flags_catch_overflow_inside_the_chain(device):
    """GradScaler doubles the loss scale until something overflows, and what overflows first need not be a root
    (dL/drgb, dL/d density) or a leaf (dL/d encoded) of the 16-bit gradient chain: a hidden dZ or d_base_out can reach
    inf while the roots are finite.  Sweep the scale from tcnn's 128 to 2^40: for EVERY scale the per-group verdict of
    the producer-flag step (flags at roots / leaves + the dW totals of every fused-MLP backward) must equal the verdict of the
    full scan of the gradient buffer -- including the scales in between, where only the inside of the chain overflows
    (the regime that turned a fixed-pose 8192-step run into NaN weights before the non-grid scan existed)."""
    R = 256
    origins, directions, dnorm, cam, jit, gt_rgb, gt_depth = _rays(R, 7)
    engines = {p: _make_engine(device, producer_overflow_flags=p) for p in (True, False)}
    p0 = engines[True].params.clone()
    verdicts = {}
    for k in [7.0, 13.0, 19.0] + [float(v) for v in range(24, 37)] + [40.0]:
        row = {}
        for producer, eng in engines.items():
            eng.cfg.loss_scale = float(2 ** k)
            eng.dev_loss_scale.fill_(float(2 ** k))
            eng.set_params(p0)
            eng.reset_optimizer()
            ws = eng._workspace(R, True)
            eng.load_ray_bundle(ws, origins.to(device), directions.to(device), dnorm.to(device), cam.to(device),
                                gt_rgb.to(device), gt_depth.to(device))
            eng.forward_backward(ws, tuple(j.to(device) for j in jit), has_depth=True, update_proposals=True, anneal=0.6)
            eng.optimizer_step(["fields", "proposal_networks"], flags_cleared=True)
            torch.cuda.synchronize()
            row[producer] = [bool(f) for f in eng.skip_flag.tolist()[:2]]
            assert bool(torch.isfinite(eng.params).all()), f"scale 2^{k}: non-finite parameters (producer flags: {producer})"
        verdicts[k] = row
        assert row[True] == row[False], f"scale 2^{k}: producer flags {row[True]} vs full scan {row[False]}"
    print(verdicts)
    assert not verdicts[7.0][True][0] and verdicts[40.0][True][0], "the sweep must span in-range and overflowing scales"
    # (With these random-init weights the roots overflow first at every scale -- fields from 2^29, proposals from 2^35.
    # The inside-only case -- finite roots, a hidden dZ that is not -- is planted at the kernel level:
    # tests/test_tcnn_gpu.py::test_network_backward_flags_an_overflow_inside_the_chain.)
