"""The per-ray kernels of csrc/render.hip (entry loads up front, backward from registers) against their previous forms in
csrc/render_legacy.hip (NVO_RAY_LEGACY=1): the SAME launcher on the SAME seeded inputs, each into freshly zeroed
outputs, and every output buffer must hold the same bits.  (k_weights_pdf ships in its previous form -- EXPERIMENTS.md
12.4 -- so its cases pin the switch and wait for the next form of that kernel.)

Only the source of an operand changed between the two forms (a register or an LDS row instead of a second load), so
equality is exact.  Loss shards are indexed by r & 63: with R <= 64 every shard slot receives one add per kernel (two
commuting ones in the paired proposal launch), so the sums do not depend on the order of the waves either.  Buffers are
compared as integers: NaN payloads and the sign of zero count.

Inputs of every case: strictly increasing bins; about 10 % of the selectors off (x01[3i] <= 0); ray 1 with all
pre-activations at -60 (all weights zero: pdf padding, isnan(t) path); ray 2 with one pre-activation of +80 (exponent
cap, and at loss scale 65536 the fp16 overflow flag); gt_depth with zeros (depth mask off).  R = 5 is a partial
workgroup, R = 64 sixteen of them.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

RS = (5, 64)
NEAR, FAR = 0.05, 1000.0
LOSS_SCALE = 65536.0


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


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


def _level(g, R, S, pre_stride, bf16, device):
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
    return dict(pre=_h16(pre.reshape(R * S, pre_stride), bf16).to(device), x01=x01.to(device), sb=sb.to(device),
                tb=tb.to(device))


def _ray_targets(g, R, device):
    gt_depth = torch.rand(R, generator=g) * 3.0
    gt_depth[::3] = 0.0
    return dict(gt_rgb=torch.rand(R, 3, generator=g).to(device), gt_depth=gt_depth.to(device),
                dnorm=(1.0 + 0.1 * torch.rand(R, generator=g)).to(device),
                gt_normal=torch.rand(R, 3, generator=g).to(device))


def _both_forms(monkeypatch, run):
    """run() once per form -> two dicts of output tensors, compared bit for bit"""
    outs = []
    for legacy in (True, False):
        if legacy:
            monkeypatch.setenv("NVO_RAY_LEGACY", "1")
        else:
            monkeypatch.delenv("NVO_RAY_LEGACY", raising=False)
        outs.append(run())
        torch.cuda.synchronize()
    monkeypatch.delenv("NVO_RAY_LEGACY", raising=False)
    old, new = outs
    assert old.keys() == new.keys()
    for name in old:
        if old[name] is None:
            continue
        assert torch.equal(_bits(old[name]), _bits(new[name])), name
    return new


# ------------------------------------------------------------------------------------------------
# nvo_weights_pdf
# ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("S,S_out,anneal,anneal_dev,jitter,x01_out,pre_stride,bf16,sigma", PDF_CASES)
def test_weights_pdf_forms_same_bits(device, monkeypatch, S, S_out, anneal, anneal_dev, jitter, x01_out, pre_stride,
                                     bf16, sigma):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _stream

    st = _stream(device)
    for R in RS:
        g = torch.Generator().manual_seed(1000 + 7 * S + R)
        lv = _level(g, R, S, pre_stride, bf16, device)
        jit = torch.rand(R, generator=g).to(device)
        o = ((torch.rand(R, 3, generator=g) - 0.5) * 1.5).to(device)
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(device)
        an_dev = torch.tensor([anneal], device=device)

        def run():
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
                histogram_padding=0.01, near_plane=NEAR, far_plane=FAR, jitter=jit.data_ptr() if jitter else None,
                sbins_out=out["sbins_out"].data_ptr() if S_out else None,
                tbins_out=out["tbins_out"].data_ptr() if S_out else None,
                anneal_dev=an_dev.data_ptr() if anneal_dev else None,
                origins=o.data_ptr() if x01_out else None, directions=d.data_ptr() if x01_out else None,
                x01_out=out["x01_out"].data_ptr() if x01_out else None, act_bf16=int(bf16))
            _call("nvo_weights_pdf", st, C.byref(a))
            return out

        new = _both_forms(monkeypatch, run)
        w = new["weights"].view(R, S)
        assert bool(torch.isfinite(w).all()) and float(w[1].abs().max()) == 0.0
        if S_out:
            sbo = new["sbins_out"]
            assert bool(torch.isfinite(sbo).all()) and bool((sbo[:, 1:] >= sbo[:, :-1]).all())


# ------------------------------------------------------------------------------------------------
# nvo_main_render_loss
# ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("S,training,gt_depth,distortion_mult,normals,tile_live,drgb_stride,scale_dev,bf16", MAIN_CASES)
def test_main_render_loss_forms_same_bits(device, monkeypatch, S, training, gt_depth, distortion_mult, normals,
                                          tile_live, drgb_stride, scale_dev, bf16):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _stream

    st = _stream(device)
    pre_stride = dpre_stride = 16
    rgb_stride = 16 if drgb_stride == 16 else 3
    for R in RS:
        g = torch.Generator().manual_seed(2000 + 7 * S + R)
        lv = _level(g, R, S, pre_stride, bf16, device)
        tg = _ray_targets(g, R, device)
        rgb = _h16(torch.rand(R * S, rgb_stride, generator=g), bf16).to(device)
        dsig = (torch.randn(R * S, 3, generator=g) * 40.0).to(device)
        dsig[3] = 0.0  # (a zero gradient: the normalisation clamp)
        scale = torch.tensor([LOSS_SCALE], device=device)

        def run():
            z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
            out = dict(out_rgb=z(R, 3), out_depth=z(R), out_expected_depth=z(R), out_accumulation=z(R),
                       out_normals=z(R, 3), weights=z(R * S), dpre=z(R * S, dpre_stride, dtype=torch.int16),
                       drgb=z(R * S, drgb_stride, dtype=torch.int16), tile_live=z(max(R * S // 16, 1), dtype=torch.uint8),
                       losses=z(64, 8), nonfinite_flag=z(1, dtype=torch.int32))
            a = _lib.MainLossArgs(
                R=R, S=S, pre=lv["pre"].data_ptr(), pre_stride=pre_stride, rgb=rgb.data_ptr(), rgb_stride=rgb_stride,
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
                dsigma_dx=dsig.data_ptr() if normals else None, dsigma_inv_scale=1.0 / 128.0,
                gt_normal=tg["gt_normal"].data_ptr() if normals else None, normal_mult=5e-3 if normals else 0.0,
                out_normals=out["out_normals"].data_ptr() if normals else None, act_bf16=int(bf16),
                loss_scale_dev=scale.data_ptr() if scale_dev else None, nonfinite_flag=out["nonfinite_flag"].data_ptr(),
                tile_live=out["tile_live"].data_ptr() if (tile_live and training) else None)
            _call("nvo_main_render_loss", st, C.byref(a))
            return out

        new = _both_forms(monkeypatch, run)
        assert bool(torch.isfinite(new["out_rgb"]).all()) and bool(torch.isfinite(new["weights"]).all())
        if training:
            assert float(new["losses"][:, 0].sum()) > 0.0
        else:
            assert not bool(new["dpre"].any()) and not bool(new["losses"].any())


# ------------------------------------------------------------------------------------------------
# nvo_prop_loss / nvo_prop_loss_pair
# ------------------------------------------------------------------------------------------------
def _prop_inputs(g, R, S, S_main, pre_stride, bf16, device):
    lv = _level(g, R, S, pre_stride, bf16, device)
    sbm, _ = _bins(g, R, S_main)
    wm = torch.rand(R * S_main, generator=g).view(R, S_main)
    wm = wm / wm.sum(dim=1, keepdim=True) * 0.9
    wm[1] = 0.0
    lv.update(sbm=sbm.to(device), wm=wm.reshape(-1).contiguous().to(device))
    return lv


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


@pytest.mark.parametrize("S,S_main,training,dpre_stride,gt_depth,scale_dev,bf16", PROP_CASES)
def test_prop_loss_forms_same_bits(device, monkeypatch, S, S_main, training, dpre_stride, gt_depth, scale_dev, bf16):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _stream

    st = _stream(device)
    for R in RS:
        g = torch.Generator().manual_seed(3000 + 7 * S + R)
        lv = _prop_inputs(g, R, S, S_main, 1 if dpre_stride == 1 else 16, bf16, device)
        tg = _ray_targets(g, R, device)
        scale = torch.tensor([LOSS_SCALE], device=device)

        def run():
            out = dict(dpre=torch.zeros(R * S, dpre_stride, dtype=torch.int16, device=device),
                       losses=torch.zeros(64, 8, device=device),
                       nonfinite_flag=torch.zeros(1, dtype=torch.int32, device=device))
            a = _prop_args(_lib, R, S, S_main, lv, tg, gt_depth, out, training, dpre_stride, bf16, scale, scale_dev)
            _call("nvo_prop_loss", st, C.byref(a))
            return out

        new = _both_forms(monkeypatch, run)
        assert bool(torch.isfinite(new["losses"]).all()) and float(new["losses"][:, 0].sum()) > 0.0
        if not training:
            assert not bool(new["dpre"].any())


# ((S0, S1), S_main, training, dpre_stride, gt_depth, bf16): both proposal levels in one launch, level 0's blocks first
PAIR_CASES = [
    ((256, 96), 48, True, 16, True, False),
    ((256, 96), 48, True, 1, False, True),
    ((256, 96), 48, False, 16, True, True),
    ((65, 65), 7, True, 16, True, False),
]


@pytest.mark.parametrize("Ss,S_main,training,dpre_stride,gt_depth,bf16", PAIR_CASES)
def test_prop_loss_pair_forms_same_bits(device, monkeypatch, Ss, S_main, training, dpre_stride, gt_depth, bf16):
    from nerf_vo_amd import _lib
    from nerf_vo_amd.engine import _call
    from nerf_vo_amd.tinycudann.modules import _stream

    st = _stream(device)
    for R in RS:
        g = torch.Generator().manual_seed(4000 + 7 * Ss[0] + R)
        lvs = [_prop_inputs(g, R, S, S_main, 1 if dpre_stride == 1 else 16, bf16, device) for S in Ss]
        tg = _ray_targets(g, R, device)
        scale = torch.tensor([LOSS_SCALE], device=device)

        def run():
            losses = torch.zeros(64, 8, device=device)
            flag = torch.zeros(1, dtype=torch.int32, device=device)
            outs = [dict(dpre=torch.zeros(R * S, dpre_stride, dtype=torch.int16, device=device), losses=losses,
                         nonfinite_flag=flag) for S in Ss]
            args = [_prop_args(_lib, R, S, S_main, lv, tg, gt_depth, out, training, dpre_stride, bf16, scale, True)
                    for S, lv, out in zip(Ss, lvs, outs)]
            _call("nvo_prop_loss_pair", st, C.byref(args[0]), C.byref(args[1]))
            return dict(dpre0=outs[0]["dpre"], dpre1=outs[1]["dpre"], losses=losses, nonfinite_flag=flag)

        new = _both_forms(monkeypatch, run)
        assert bool(torch.isfinite(new["losses"]).all()) and float(new["losses"][:, 0].sum()) > 0.0
