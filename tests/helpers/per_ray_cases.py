"""Cases, seeded inputs and launches of the per-ray kernels of csrc/render.hip (k_weights_pdf, k_main_render_loss,
k_prop_loss), shared by tests/test_per_ray_forms_gpu.py, tests/test_per_ray_cases_cpu.py and the recorder
tests/golden/make_golden_per_ray_bits.py, so that the record and the test cannot build different inputs.

Inputs of every case: strictly increasing bins; about 10 % of the selectors off (x01[3i] <= 0); ray 1 with all
pre-activations at -60 (all weights zero: pdf padding, isnan(t) path); ray 2 with one pre-activation of +80 (exponent
cap, and at loss scale 65536 the fp16 overflow flag); gt_depth with zeros (depth mask off).  R = 5 is a partial
workgroup, R = 64 sixteen of them.

Every input is built on the CPU from one seeded generator per (family, case, R), in a fixed order of draws, and only
then copied to the device: inputs(family, case, R) needs no GPU, and inputs_digest() of it is part of the record.
run(family, ...) builds the args struct, zeroes fresh outputs, launches once and returns the output tensors by name;
OUTPUTS lists those names.  Loss shards are indexed by r & 63: with R <= 64 every shard slot receives one add per kernel
(two commuting ones in the paired proposal launch), so the sums do not depend on the order of the waves and every
output is a fixed string of bits.
"""
import ctypes as C
import hashlib
import json
import os

import torch

RECORD_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "per_ray_bits.json")

RS = (5, 64)
NEAR, FAR = 0.05, 1000.0
LOSS_SCALE = 65536.0

# (S, S_out, anneal, anneal on the device, jitter, x01_out, pre_stride, bf16, sigma)
PDF_CASES = [
    (256, 96, 1.0, False, True, True, 1, False, False),
    (256, 96, 0.37, True, False, False, 16, True, True),
    (256, 96, 0.37, False, True, True, 16, False, True),
    (256, 96, 1.0, True, True, False, 1, True, False),
    (96, 48, 0.37, False, True, True, 16, False, False),
    (96, 48, 1.0, True, False, True, 1, True, True),
    (65, 7, 0.37, True, True, True, 1, False, True),
    (65, 7, 1.0, False, False, False, 16, True, False),
    (64, 0, 1.0, False, False, False, 1, False, True),
    (64, 0, 0.37, True, True, False, 16, True, False),
    (1, 0, 1.0, False, False, False, 16, True, True),
    (1, 0, 1.0, False, True, False, 1, False, False),
]

# (S, training, gt_depth, distortion_mult, normals, tile_live, drgb_stride, loss_scale on the device, bf16)
MAIN_CASES = [
    (48, True, True, 0.002, False, True, 16, True, False),
    (48, True, False, 0.0, True, False, 3, False, True),
    (48, True, True, 0.002, True, True, 16, True, True),
    (48, False, False, 0.0, False, False, 16, False, False),
    (48, False, False, 0.0, True, False, 16, False, True),
    (16, True, True, 0.0, False, True, 3, True, False),
    (16, True, False, 0.002, True, True, 16, False, False),
    (64, True, True, 0.002, True, True, 16, False, False),
    (64, True, True, 0.0, False, False, 3, True, True),
    (64, False, False, 0.0, False, False, 16, False, True),
    (1, True, True, 0.002, True, False, 16, True, False),
    (1, True, False, 0.0, False, False, 3, False, True),
    (1, False, False, 0.0, True, False, 16, False, False),
]

# (S, S_main, training, dpre_stride, gt_depth, loss_scale on the device, bf16)
PROP_CASES = [
    (256, 48, True, 16, True, True, False),
    (256, 48, True, 1, False, False, True),
    (256, 48, False, 16, True, False, False),
    (96, 48, True, 1, True, True, False),
    (96, 48, True, 16, False, False, True),
    (96, 48, False, 1, True, False, True),
    (65, 7, True, 16, True, False, True),
    (65, 7, True, 1, False, True, False),
    (65, 7, False, 16, True, False, False),
]

# ((S0, S1), S_main, training, dpre_stride, gt_depth, bf16): both proposal levels in one launch, level 0's blocks first
PAIR_CASES = [
    ((256, 96), 48, True, 16, True, False),
    ((256, 96), 48, True, 1, False, True),
    ((256, 96), 48, False, 16, True, True),
    ((65, 65), 7, True, 16, True, False),
]

CASES = {"weights_pdf": PDF_CASES, "main_render_loss": MAIN_CASES, "prop_loss": PROP_CASES,
         "prop_loss_pair": PAIR_CASES}

# the buffers run() returns, per family: every one is in the record, also those whose pointer a case passes as NULL
# (they must stay all-zero)
OUTPUTS = {
    "weights_pdf": ("weights", "sbins_out", "tbins_out", "x01_out", "sigma"),
    "main_render_loss": ("out_rgb", "out_depth", "out_expected_depth", "out_accumulation", "out_normals", "weights",
                         "dpre", "drgb", "tile_live", "losses", "nonfinite_flag"),
    "prop_loss": ("dpre", "losses", "nonfinite_flag"),
    "prop_loss_pair": ("dpre0", "dpre1", "losses", "nonfinite_flag"),
}


def _h16(t, bf16):
    return t.to(torch.bfloat16 if bf16 else torch.float16)


def _bins(g, R, S):
    """strictly increasing spacing bins in [0, 1] and euclidean bins, [R][S+1]"""
    steps = torch.rand(R, S + 1, generator=g) + 0.05
    sb = torch.cumsum(steps, dim=1)
    sb = (sb - sb[:, :1]) / (sb[:, -1:] - sb[:, :1])
    sb = sb * 0.96875 + 0.015625
    assert bool((sb[:, 1:] > sb[:, :-1]).all())
    tb = 0.05 + 6.0 * sb * (1.0 + sb)
    assert bool((tb[:, 1:] > tb[:, :-1]).all())
    return sb.contiguous(), tb.contiguous()


def _level(g, R, S, pre_stride, bf16):
    """inputs of one level: pre-activations, selectors, bins"""
    sb, tb = _bins(g, R, S)
    x01 = torch.rand(R * S, 3, generator=g) * 0.98 + 0.01
    off = torch.rand(R * S, generator=g) < 0.1
    x01[off, 0] = torch.where(torch.rand(int(off.sum()), generator=g) < 0.5, 0.0, -0.25)
    pre = torch.randn(R * S, pre_stride, generator=g) * 2.0
    pre = pre.view(R, S, pre_stride)
    pre[1, :, 0] = -60.0
    pre[2, S // 2, 0] = 80.0
    x01.view(R, S, 3)[2, S // 2, 0] = 0.5  # (the +80 sample is selected)
    return dict(pre=_h16(pre.reshape(R * S, pre_stride), bf16), x01=x01, sb=sb, tb=tb)


def _ray_targets(g, R):
    gt_depth = torch.rand(R, generator=g) * 3.0
    gt_depth[::3] = 0.0
    return dict(gt_rgb=torch.rand(R, 3, generator=g), gt_depth=gt_depth, dnorm=1.0 + 0.1 * torch.rand(R, generator=g),
                gt_normal=torch.rand(R, 3, generator=g))


def _prop_inputs(g, R, S, S_main, pre_stride, bf16):
    lv = _level(g, R, S, pre_stride, bf16)
    sbm, _ = _bins(g, R, S_main)
    wm = torch.rand(R * S_main, generator=g).view(R, S_main)
    wm = wm / wm.sum(dim=1, keepdim=True) * 0.9
    wm[1] = 0.0
    lv.update(sbm=sbm, wm=wm.reshape(-1).contiguous())
    return lv


def inputs(family, case, R):
    """name -> CPU tensor: everything the launch of this (family, case, R) reads"""
    if family == "weights_pdf":
        S, _, anneal, _, _, _, pre_stride, bf16, _ = case
        g = torch.Generator().manual_seed(1000 + 7 * S + R)
        inp = _level(g, R, S, pre_stride, bf16)
        inp["jit"] = torch.rand(R, generator=g)
        inp["o"] = (torch.rand(R, 3, generator=g) - 0.5) * 1.5
        inp["d"] = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        inp["an_dev"] = torch.tensor([anneal])
    elif family == "main_render_loss":
        S, _, _, _, _, _, drgb_stride, _, bf16 = case
        g = torch.Generator().manual_seed(2000 + 7 * S + R)
        inp = _level(g, R, S, 16, bf16)
        inp.update(_ray_targets(g, R))
        inp["rgb"] = _h16(torch.rand(R * S, 16 if drgb_stride == 16 else 3, generator=g), bf16)
        inp["dsig"] = torch.randn(R * S, 3, generator=g) * 40.0
        inp["dsig"][3] = 0.0  # (a zero gradient: the normalisation clamp)
        inp["scale"] = torch.tensor([LOSS_SCALE])
    elif family == "prop_loss":
        S, S_main, _, dpre_stride, _, _, bf16 = case
        g = torch.Generator().manual_seed(3000 + 7 * S + R)
        inp = _prop_inputs(g, R, S, S_main, 1 if dpre_stride == 1 else 16, bf16)
        inp.update(_ray_targets(g, R))
        inp["scale"] = torch.tensor([LOSS_SCALE])
    elif family == "prop_loss_pair":
        Ss, S_main, _, dpre_stride, _, bf16 = case
        g = torch.Generator().manual_seed(4000 + 7 * Ss[0] + R)
        inp = {}
        for k, S in enumerate(Ss):
            lv = _prop_inputs(g, R, S, S_main, 1 if dpre_stride == 1 else 16, bf16)
            inp.update({f"{name}{k}": t for name, t in lv.items()})
        inp.update(_ray_targets(g, R))
        inp["scale"] = torch.tensor([LOSS_SCALE])
    else:
        raise KeyError(family)
    return inp


def digest(t):
    """sha256 of a tensor's raw bytes: NaN payloads and the sign of zero count"""
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def inputs_digest(inp):
    """one sha256 over a case's input tensors (name, dtype, shape and bytes of each, names sorted)"""
    h = hashlib.sha256()
    for name in sorted(inp):
        t = inp[name]
        h.update(f"{name}:{t.dtype}:{tuple(t.shape)}:{digest(t)};".encode())
    return h.hexdigest()


def record_key(family, index, R):
    return f"{family}/{index}/R{R}"


def load_record():
    with open(RECORD_PATH) as fh:
        return json.load(fh)


def _prop_args(_lib, R, S, S_main, lv, tg, gt_depth, out, training, dpre_stride, bf16, scale, scale_dev):
    return _lib.PropLossArgs(
        R=R, S=S, S_main=S_main, pre=lv["pre"].data_ptr(), pre_stride=lv["pre"].shape[1], x01=lv["x01"].data_ptr(),
        sbins=lv["sb"].data_ptr(), tbins=lv["tb"].data_ptr(), sbins_main=lv["sbm"].data_ptr(),
        weights_main=lv["wm"].data_ptr(), density_bias=-1.0, gt_depth=tg["gt_depth"].data_ptr() if gt_depth else None,
        directions_norm=tg["dnorm"].data_ptr(), interlevel_mult=1.0, depth_mult=0.001, depth_sigma=0.01,
        inv_rays=1.0 / R, depth_level_div=1.0 / 3.0, loss_scale=128.0 if scale_dev else LOSS_SCALE,
        losses=out["losses"].data_ptr(), dpre=out["dpre"].data_ptr() if training else None, dpre_stride=dpre_stride,
        act_bf16=int(bf16), loss_scale_dev=scale.data_ptr() if scale_dev else None,
        nonfinite_flag=out["nonfinite_flag"].data_ptr())


def _run_weights_pdf(_lib, _call, st, device, case, R, lv):
    S, S_out, anneal, anneal_dev, jitter, x01_out, pre_stride, bf16, sigma = case
    out = dict(weights=torch.zeros(R * S, device=device),
               sbins_out=torch.zeros(R, S_out + 1, device=device),
               tbins_out=torch.zeros(R, S_out + 1, device=device),
               x01_out=torch.zeros(R * max(S_out, 1), 3, device=device),
               sigma=torch.zeros(R * S, device=device))
    a = _lib.WeightsPdfArgs(
        R=R, S=S, S_out=S_out, pre=lv["pre"].data_ptr(), pre_stride=pre_stride, x01=lv["x01"].data_ptr(),
        sbins=lv["sb"].data_ptr(), tbins=lv["tb"].data_ptr(), density_bias=-1.0,
        sigma=out["sigma"].data_ptr() if sigma else None, weights=out["weights"].data_ptr(),
        anneal=1.0 if anneal_dev else anneal,  # (the device value replaces the field)
        histogram_padding=0.01, near_plane=NEAR, far_plane=FAR, jitter=lv["jit"].data_ptr() if jitter else None,
        sbins_out=out["sbins_out"].data_ptr() if S_out else None,
        tbins_out=out["tbins_out"].data_ptr() if S_out else None,
        anneal_dev=lv["an_dev"].data_ptr() if anneal_dev else None,
        origins=lv["o"].data_ptr() if x01_out else None, directions=lv["d"].data_ptr() if x01_out else None,
        x01_out=out["x01_out"].data_ptr() if x01_out else None, act_bf16=int(bf16))
    _call("nvo_weights_pdf", st, C.byref(a))
    return out


def _run_main_render_loss(_lib, _call, st, device, case, R, lv):
    S, training, gt_depth, distortion_mult, normals, tile_live, drgb_stride, scale_dev, bf16 = case
    pre_stride = dpre_stride = 16
    rgb_stride = 16 if drgb_stride == 16 else 3
    tg = lv
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
    out = dict(out_rgb=z(R, 3), out_depth=z(R), out_expected_depth=z(R), out_accumulation=z(R),
               out_normals=z(R, 3), weights=z(R * S), dpre=z(R * S, dpre_stride, dtype=torch.int16),
               drgb=z(R * S, drgb_stride, dtype=torch.int16), tile_live=z(max(R * S // 16, 1), dtype=torch.uint8),
               losses=z(64, 8), nonfinite_flag=z(1, dtype=torch.int32))
    a = _lib.MainLossArgs(
        R=R, S=S, pre=lv["pre"].data_ptr(), pre_stride=pre_stride, rgb=lv["rgb"].data_ptr(), rgb_stride=rgb_stride,
        x01=lv["x01"].data_ptr(), sbins=lv["sb"].data_ptr(), tbins=lv["tb"].data_ptr(), density_bias=-1.0,
        gt_rgb=tg["gt_rgb"].data_ptr(), gt_depth=tg["gt_depth"].data_ptr() if gt_depth else None,
        directions_norm=tg["dnorm"].data_ptr(), rgb_mult=1.0, distortion_mult=distortion_mult, depth_mult=0.001,
        depth_sigma=0.01, inv_rays=1.0 / R, depth_level_div=1.0 / 3.0,
        loss_scale=128.0 if scale_dev else LOSS_SCALE,  # (the device value replaces the field)
        out_rgb=out["out_rgb"].data_ptr(), out_depth=out["out_depth"].data_ptr(),
        out_expected_depth=out["out_expected_depth"].data_ptr(),
        out_accumulation=out["out_accumulation"].data_ptr(), weights=out["weights"].data_ptr(),
        losses=out["losses"].data_ptr(), dpre=out["dpre"].data_ptr() if training else None,
        dpre_stride=dpre_stride, drgb=out["drgb"].data_ptr(), drgb_stride=drgb_stride,
        dsigma_dx=lv["dsig"].data_ptr() if normals else None, dsigma_inv_scale=1.0 / 128.0,
        gt_normal=tg["gt_normal"].data_ptr() if normals else None, normal_mult=5e-3 if normals else 0.0,
        out_normals=out["out_normals"].data_ptr() if normals else None, act_bf16=int(bf16),
        loss_scale_dev=lv["scale"].data_ptr() if scale_dev else None, nonfinite_flag=out["nonfinite_flag"].data_ptr(),
        tile_live=out["tile_live"].data_ptr() if (tile_live and training) else None)
    _call("nvo_main_render_loss", st, C.byref(a))
    return out


def _run_prop_loss(_lib, _call, st, device, case, R, lv):
    S, S_main, training, dpre_stride, gt_depth, scale_dev, bf16 = case
    out = dict(dpre=torch.zeros(R * S, dpre_stride, dtype=torch.int16, device=device),
               losses=torch.zeros(64, 8, device=device),
               nonfinite_flag=torch.zeros(1, dtype=torch.int32, device=device))
    a = _prop_args(_lib, R, S, S_main, lv, lv, gt_depth, out, training, dpre_stride, bf16, lv["scale"], scale_dev)
    _call("nvo_prop_loss", st, C.byref(a))
    return out


def _run_prop_loss_pair(_lib, _call, st, device, case, R, inp):
    Ss, S_main, training, dpre_stride, gt_depth, bf16 = case
    lvs = [{name: inp[f"{name}{k}"] for name in ("pre", "x01", "sb", "tb", "sbm", "wm")} for k in range(2)]
    losses = torch.zeros(64, 8, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    outs = [dict(dpre=torch.zeros(R * S, dpre_stride, dtype=torch.int16, device=device), losses=losses,
                 nonfinite_flag=flag) for S in Ss]
    args = [_prop_args(_lib, R, S, S_main, lv, inp, gt_depth, out, training, dpre_stride, bf16, inp["scale"], True)
            for S, lv, out in zip(Ss, lvs, outs)]
    _call("nvo_prop_loss_pair", st, C.byref(args[0]), C.byref(args[1]))
    return dict(dpre0=outs[0]["dpre"], dpre1=outs[1]["dpre"], losses=losses, nonfinite_flag=flag)


_RUN = {"weights_pdf": _run_weights_pdf, "main_render_loss": _run_main_render_loss, "prop_loss": _run_prop_loss,
        "prop_loss_pair": _run_prop_loss_pair}


def run(family, case, R, inp, device):
    """one launch of this family's exported entry point on inp (the CPU tensors of inputs(), copied to the device here)
    into freshly zeroed outputs -> name -> output tensor (OUTPUTS[family]), synchronised"""
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _stream

    dev_inp = {name: t.to(device) for name, t in inp.items()}
    out = _RUN[family](_lib, _call, _stream(device), device, case, R, dev_inp)
    torch.cuda.synchronize()
    assert tuple(out) == OUTPUTS[family]
    return out
