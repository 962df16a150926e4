"""The proposal density network as the epilogue of the small-grid forward (module option fuse_encoding = 2) against the
two-kernel path (fuse_encoding = 0): the fused kernel feeds the SAME 16-bit features through the SAME matrix instructions,
so outputs and stored features must be equal bit for bit -- a condition, not a tolerance.  Driven through the raw C-ABI the
way the engine drives its proposal networks (compact output, recomputed hidden layer)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the engine's two proposal grids (EngineConfig.proposal_grids)
GRIDS = {"prop0": dict(n_levels=5, log2_hashmap_size=17, base_resolution=16, max_res=128),
         "prop1": dict(n_levels=5, log2_hashmap_size=17, base_resolution=16, max_res=256)}
N_NET = 16 * 16 + 16 * 16
# one tile (three quarters of a wave idle) | ragged last wave | more than one pass of a 1024-thread workgroup over
# four-sample runs | several passes of the per-sample form on a small launch
BATCHES = (16, 64 * 17 + 16, 4096 + 16, 3 * 1024 * 4 + 48)


def _enc_cfg(c):
    pls = float(np.exp((np.log(c["max_res"]) - np.log(c["base_resolution"])) / (c["n_levels"] - 1)))
    return {"otype": "HashGrid", "n_levels": c["n_levels"], "n_features_per_level": 2,
            "log2_hashmap_size": c["log2_hashmap_size"], "base_resolution": c["base_resolution"], "per_level_scale": pls}


def _module(grid, dtype, fuse, runs=0, recompute=1):
    from nerf_vo_amd.tinycudann.modules import _create

    net_cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 16,
               "n_hidden_layers": 1}
    m = _create("nvo_create_network_with_input_encoding", 3, 1, json.dumps(_enc_cfg(GRIDS[grid])).encode(),
                json.dumps(net_cfg).encode())
    m.set_option("grid_bwd_mode", 1)
    m.set_option("grid_acc_bits", 32)
    m.set_option("compact_output", 1)
    m.set_option("recompute_hidden", recompute)
    m.set_option("bf16", int(dtype == "bf16"))
    m.set_option("grid_fwd_runs", runs)
    m.set_option("fuse_encoding", fuse)
    return m


_PARAMS = {}


def _params16(m, dtype, device):
    """Seeded parameters as the 16-bit working copy: network weights in the compute type, hash table fp16."""
    key = (m.n_params, dtype)
    if key not in _PARAMS:
        g = torch.Generator().manual_seed(5)
        p = torch.randn(m.n_params, generator=g) * 0.3
        bits = p.half().view(torch.int16).clone()
        if dtype == "bf16":
            bits[:N_NET] = p[:N_NET].bfloat16().view(torch.int16)
        _PARAMS[key] = bits.to(device)
    return _PARAMS[key]


def _inputs(kind, n, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.random((n, 3), dtype=np.float32)
    elif kind == "faces":  # every coordinate exactly on a domain face (dense-index wrap, the generic corner rule)
        x = (rng.random((n, 3)) < 0.5).astype(np.float32)
        x[::3] = rng.random((len(x[::3]), 3), dtype=np.float32)  # ... next to interior samples in the same wave
        x[::3, 0] = 1.0
    else:  # "runs": 8 consecutive samples in one cell of the finest level (the inference form gathers once per cell)
        base = rng.random(((n + 7) // 8, 1, 3), dtype=np.float32) * 0.9 + 0.05
        x = (base + rng.random((1, 8, 3), dtype=np.float32) * 1e-4).reshape(-1, 3)[:n]
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))


SENT16 = 0x7B7B  # sentinel bits of untouched 16-bit outputs
SENT8 = 0x5A


def _forward(m, dtype, x, device, n_live=None, store=None):
    from nerf_vo_amd.engine import _call, _ptr, _stream

    n = x.shape[0]
    ph = _params16(m, dtype, device)
    ctx = torch.full((m.ctx_bytes(n),), SENT8, dtype=torch.uint8, device=device)
    out = torch.full((n,), SENT16, dtype=torch.int16, device=device)
    if store is not None:
        m.set_option("store_encoded", store)
    live = None
    if n_live is not None:
        live = torch.tensor([n_live], dtype=torch.int32, device=device)
        m.set_option("n_live_ptr", live.data_ptr())
    try:
        _call("nvo_fwd", m.handle, _stream(device), n, _ptr(x), _ptr(ph), _ptr(out), _ptr(ctx))
        torch.cuda.synchronize()
    finally:
        if n_live is not None:
            m.set_option("n_live_ptr", 0)
    feats = ctx[:5 * n * 4].view(torch.int32).view(5, n)
    return out, feats, ctx


_REF = {}  # the two-kernel path's outputs, computed once per case and left unchanged


def _reference(grid, dtype, kind, n, device):
    key = (grid, dtype, kind, n)
    if key not in _REF:
        x = _inputs(kind, n).to(device)
        out, feats, _ = _forward(_module(grid, dtype, 0), dtype, x, device)
        assert bool((out != SENT16).all()) and bool((out != 0).any())
        _REF[key] = (x, out.clone(), feats.clone())
    return _REF[key]


@pytest.mark.parametrize("runs", [0, 1], ids=["per-sample", "runs"])
@pytest.mark.parametrize("kind", ["uniform", "faces", "runs"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("grid", ["prop0", "prop1"])
def test_fused_forward_equals_two_kernels(device, grid, dtype, kind, runs):
    m = _module(grid, dtype, 2, runs=runs)
    for n in BATCHES:
        x, ref_out, ref_feats = _reference(grid, dtype, kind, n, device)
        out, feats, _ = _forward(m, dtype, x, device)
        assert torch.equal(out, ref_out), f"B={n}: density output differs from the two-kernel path"
        assert torch.equal(feats, ref_feats), f"B={n}: stored features differ from the two-kernel path"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fused_forward_stores_the_hidden_layer_when_asked(device, dtype):
    """recompute_hidden = 0: the epilogue stores the [B][16] activations k_mlp_fwd stores."""
    n = 64 * 17 + 16
    x = _inputs("uniform", n).to(device)
    res = []
    for fuse in (0, 2):
        m = _module("prop0", dtype, fuse, recompute=0)
        out, feats, ctx = _forward(m, dtype, x, device)
        hid0 = 2 * ((5 * n * 4 + 255) // 256 * 256)
        res.append((out, ctx[hid0:hid0 + n * 16 * 2].clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool((res[1][1] != SENT8).any())


@pytest.mark.parametrize("runs", [0, 1], ids=["per-sample", "runs"])
@pytest.mark.parametrize("grid", ["prop0", "prop1"])
def test_n_live_bounds_the_fused_forward(device, grid, runs):
    n = 4096 + 16
    x, ref_out, ref_feats = _reference(grid, "f16", "uniform", n, device)
    m = _module(grid, "f16", 2, runs=runs)
    for count in (0, 16, n - 16):
        out, feats, _ = _forward(m, "f16", x, device, n_live=count)
        assert torch.equal(out[:count], ref_out[:count]) and torch.equal(feats[:, :count], ref_feats[:, :count])
        assert bool((out[count:] == SENT16).all()), f"n_live={count}: rows past the count were written"


def test_batch_not_a_multiple_of_16_takes_the_two_kernel_path(device):
    """B = 24 through the tcnn surface (the C-ABI itself takes multiples of 16 only; the surface pads): a forward the
    epilogue form does not cover runs the two kernels without a word and gives their bits."""
    import nerf_vo_amd.tinycudann as tcnn

    net_cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 16,
               "n_hidden_layers": 1}
    x = _inputs("uniform", 24).to(device)
    res = []
    for fuse in (0, 2):
        model = tcnn.NetworkWithInputEncoding(3, 1, _enc_cfg(GRIDS["prop0"]), net_cfg).to(device)
        with torch.no_grad():
            g = torch.Generator().manual_seed(5)
            model.params.copy_((torch.randn(model.params.numel(), generator=g) * 0.3).to(device))
            model.native_tcnn_module.set_option("fuse_encoding", fuse)
            res.append(model(x).clone())
    torch.cuda.synchronize()
    assert res[0].shape[0] == 24 and bool((res[0] != 0).any())
    assert torch.equal(res[0].view(torch.int16), res[1].view(torch.int16))


@pytest.mark.parametrize("runs", [0, 1], ids=["per-sample", "runs"])
def test_store_encoded_off_skips_the_features_and_refuses_a_backward(device, runs):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _ptr, _stream

    n = 4096 + 16
    x, ref_out, _ = _reference("prop1", "f16", "uniform", n, device)
    m = _module("prop1", "f16", 2, runs=runs)
    out, feats, ctx = _forward(m, "f16", x, device, store=0)
    assert torch.equal(out, ref_out)
    assert bool((ctx == SENT8).all()), "store_encoded = 0: the forward wrote into ctx"
    dy = torch.ones(n, dtype=torch.float16, device=device)
    dp = torch.zeros(m.n_params, device=device)
    rc = _lib.lib().nvo_bwd(m.handle, _stream(device), n, _ptr(x), _ptr(_params16(m, "f16", device)), _ptr(out), _ptr(dy),
                            _ptr(ctx), None, _ptr(dp))
    torch.cuda.synchronize()
    assert rc != 0 and b"store_encoded" in _lib.lib().nvo_last_error()
    assert float(dp.abs().max()) == 0.0
    # a storing forward on the same ctx makes it usable again
    out, feats, ctx = _forward(m, "f16", x, device, store=1)
    assert bool((feats.view(torch.uint8) != SENT8).any())


@pytest.mark.parametrize("deterministic", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("grid", ["prop0", "prop1"])
def test_backward_after_the_fused_forward(device, grid, deterministic):
    """Gradients behind a storing fused forward equal the two-kernel path's to the spread the two-kernel path shows against
    itself (the slice-owner flush and the weight gradient end in float atomics): the spread is the largest distance between
    any two of four two-kernel runs, measured here.  With the module option `deterministic` that spread is zero and the
    fused path must match exactly."""
    from nerf_vo_amd.engine import _call, _ptr, _stream

    n = 64 * 17 + 16
    x = _inputs("uniform", n).to(device)
    g = torch.Generator().manual_seed(3)
    dy = (torch.randn(n, generator=g) * 64).half().to(device)

    def run(fuse):
        m = _module(grid, "f16", fuse)
        m.set_option("deterministic", deterministic)
        out, feats, ctx = _forward(m, "f16", x, device)
        dx = torch.full((n, 3), 7.0, device=device)
        dp = torch.full((m.n_params,), 7.0, device=device)
        _call("nvo_bwd", m.handle, _stream(device), n, _ptr(x), _ptr(_params16(m, "f16", device)), _ptr(out), _ptr(dy),
              _ptr(ctx), _ptr(dx), _ptr(dp))
        torch.cuda.synchronize()
        return dp, dx

    refs = [run(0) for _ in range(4)]
    f = run(2)
    for k, what in ((0, "dL/dparams"), (1, "dL/dx")):
        spread = max(float((a[k] - b[k]).abs().max()) for a in refs for b in refs)
        err = min(float((f[k] - a[k]).abs().max()) for a in refs)
        print(f"{grid} {what}: two-kernel spread {spread:.3e}, fused vs two-kernel {err:.3e}")
        assert bool((f[k] != 7.0).any())
        assert err <= spread, f"{what}: fused {err:.3e} vs the two-kernel path's own spread {spread:.3e}"
    if deterministic:
        assert torch.equal(f[0], refs[0][0]) and torch.equal(f[1], refs[0][1])


def test_engine_step_is_unchanged_by_the_fusion(device):
    """64 rays through the default (fused) engine and one whose proposal networks run as two kernels: a plain and an
    update step from the same parameters -- proposal bins, weights and the rendered outputs are equal bit for bit."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine

    n_img, R = 4, 64
    g = torch.Generator().manual_seed(0)
    origins = ((torch.rand(R, 3, generator=g) - 0.5) * 0.8).to(device)
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(device)
    dnorm = (1.0 + 0.2 * torch.rand(R, generator=g)).to(device)
    cam = torch.randint(0, n_img, (R,), generator=g).to(device)
    jit = tuple(torch.rand(R, generator=g).to(device) for _ in range(3))
    gt_rgb, gt_depth = torch.rand(R, 3, generator=g).to(device), (torch.rand(R, generator=g) * 1.5).to(device)
    flat = None
    res = []
    for fuse in (2, 0):
        eng = NerfactoEngine(EngineConfig(num_images=n_img, proposal_fuse_encoding=fuse), device)
        if flat is None:
            flat = (torch.rand(eng.n_params, generator=g) * 2 - 1) * 0.3
        eng.set_params(flat)
        ws = eng._workspace(R, True)
        eng.load_ray_bundle(ws, origins, directions, dnorm, cam, gt_rgb, gt_depth)
        got = []
        for update in (False, True):
            eng.forward_backward(ws, jit, has_depth=True, update_proposals=update, anneal=0.5)
            torch.cuda.synchronize()
            names = [f"{n}{k}" for k in range(3) for n in ("sbins", "tbins", "weights")] + ["out0", "out1", "out_rgb", "out_depth",
                                                                                      "out_accumulation"]
            got.append({n: ws[n].clone() for n in names})
        res.append(got)
    for step, (a, b) in enumerate(zip(*res)):
        for name in a:
            assert torch.equal(a[name], b[name]), f"step {step}: {name} differs between the fused and the two-kernel engine"
    assert bool(torch.isfinite(res[0][0]["out_rgb"]).all()) and float(res[0][0]["weights2"].abs().max()) > 0.0
