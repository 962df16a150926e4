"""The occupancy-grid back-end's normals path on the GPU: the compositing kernel alone against its float64 reference
(tests/helpers/ngp_normals_oracle.py; bound 4 * e32 + 1e-6, profiles/ngp_normals_parity_margins.json), the density
gradient of the real 16-bit chain against float64 autograd, that the path leaves training and the default render alone,
rounds and halves, and the facade end to end on a trained room (Normals render mode, render_frame_normal,
render_point_cloud, the mesh's vertex attributes).

NVO_NGP_NORMALS_MEASURED=FILE records the figures of the run (tests/helpers/ngp_normals_oracle.py --measured FILE copies
them into the JSON)."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from helpers import ngp_normals_oracle as H
from helpers import ngp_oracle as N
from test_mesh_from_nerf_gpu import _ply_layout

pytestmark = pytest.mark.gpu

_MEASURED = {}

# render_frame_normal against the room's analytic normals, pixels with accumulation > 0.5, 400 training steps: the
# (share within 90 degrees, median angle in degrees) of three seeds measured on gfx950 (EXPERIMENTS.md).  Asserted: the
# worst share minus 0.05, twice the worst median.
FRAME_NORMAL_MEASURED = ((0.6692, 71.15), (0.6942, 69.41), (0.6712, 72.15))  # seeds 0, 1, 2 of train_room, frame 5
FRAME_NORMAL_MIN_SHARE = min((s for s, _ in FRAME_NORMAL_MEASURED), default=float("nan")) - 0.05
FRAME_NORMAL_MAX_MEDIAN_DEG = 2.0 * max((m for _, m in FRAME_NORMAL_MEASURED), default=float("nan"))


def _record(key, value):
    _MEASURED[key] = float(value)
    path = os.environ.get("NVO_NGP_NORMALS_MEASURED")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(_MEASURED, fh, indent=1)


# ------------------------------------------------------------------------------------------------------------------
# the compositing kernel, alone
# ------------------------------------------------------------------------------------------------------------------
class _Kernel:
    """the case's arrays on the device (NaN where no ray owns a slot) and the two launches"""

    def __init__(self, case, device):
        from nerf_vo_amd import _lib
        from nerf_vo_amd.tinycudann.modules import _stream

        self.lib, self.stream, self.case, self.dev = _lib, _stream(device), case, device
        d = lambda x, dt=None: (x if dt is None else x.to(dt)).contiguous().to(device)  # noqa: E731
        cap = case["capacity"]
        den = torch.full((cap, 16), float("nan"), dtype=torch.float16)
        den[:, 0] = case["pre"]
        col = torch.full((cap, 16), float("nan"), dtype=torch.float16)
        col[:, :3] = case["y"]
        self.t, self.dt, self.den, self.col = d(case["t"]), d(case["dt"]), d(den), d(col)
        self.dx01, self.origins, self.directions = d(case["dx01"]), d(case["origins"]), d(case["directions"])

    def normals(self, counts, offsets, out, carry_in=None, accumulate=False):
        case = self.case
        c, o = counts.to(torch.int32).to(self.dev), offsets.to(torch.int32).to(self.dev)
        a = self.lib.NgpNormalArgs(
            R=case["R"], capacity=case["capacity"], counts=c.data_ptr(), offsets=o.data_ptr(), t=self.t.data_ptr(),
            dt=self.dt.data_ptr(), density_out=self.den.data_ptr(), density_stride=16, dx01=self.dx01.data_ptr(),
            origins=self.origins.data_ptr(), directions=self.directions.data_ptr(), aabb_lo=case["lo"], aabb_hi=case["hi"],
            carry_in=None if carry_in is None else carry_in.data_ptr(), accumulate=int(accumulate), out_normal=out.data_ptr())
        self.lib.check(self.lib.lib().nvo_ngp_composite_normals(self.stream, C.byref(a)), "ngp_composite_normals")
        torch.cuda.synchronize()
        return out

    def carry(self, counts, offsets):
        """optical depth of the given ranges, from the colour kernel itself (inference, carry_out)"""
        case = self.case
        R = case["R"]
        c, o = counts.to(torch.int32).to(self.dev), offsets.to(torch.int32).to(self.dev)
        carry = torch.full((R,), float("nan"), device=self.dev)
        rgb, dep, acc = torch.empty(R, 3, device=self.dev), torch.empty(R, device=self.dev), torch.empty(R, device=self.dev)
        a = self.lib.NgpLossArgs(R=R, capacity=case["capacity"], counts=c.data_ptr(), offsets=o.data_ptr(), ray_idx=None,
                                 t=self.t.data_ptr(), dt=self.dt.data_ptr(), density_out=self.den.data_ptr(), density_stride=16,
                                 rgb_out=self.col.data_ptr(), rgb_stride=16, rgb_mult=1.0, depth_mult=0.0, inv_rays=1.0 / R,
                                 loss_scale=1.0, out_rgb=rgb.data_ptr(), out_depth=dep.data_ptr(),
                                 out_accumulation=acc.data_ptr(), carry_out=carry.data_ptr(), d_rgb_stride=16)
        self.lib.check(self.lib.lib().nvo_ngp_composite_loss(self.stream, C.byref(a)), "ngp_composite_loss")
        torch.cuda.synchronize()
        return carry


def _assert_classes(case, specials):
    c = case["classes"]
    for n in ("empty", "dropped", 1, 63, 64, 65, 200):
        assert c[f"count_{n}"] >= 1, n
    assert c["face0"] == 65 and c["face1"] == 64 and c["outside"] >= 20 and c["near_face"] == 0
    assert c["zero_grad"] >= 20 and c["one_axis"] >= 20 and c["dropped_slots"] > 0 and c["free_slots"] > 0
    assert (c["hot"] > 0 and c["fp16_max"] == 1) == specials


def test_composite_normals_kernel(device):
    """the issue's case (no capped sample): one pass against float64, a second launch for the same bits, two rounds with
    carry_in / accumulate at every cut against the uninterrupted pass -- all under 4 * e32 + 1e-6"""
    case = H.normals_case()
    _assert_classes(case, False)
    m = H.load_margins()
    bound = H.bound_for("normals", m)
    ref = H.normals_reference(case)["S"]
    k = _Kernel(case, device)
    R = case["R"]
    out = k.normals(case["counts"], case["offsets"], torch.full((R, 3), float("nan"), device=device))
    fig = N.figure(out.cpu(), ref)
    _record("normals", fig)
    print(f"normals: figure {fig:.3e}  e32 {m['e32']['normals']:.3e}  bound {bound:.3e}")
    assert fig <= bound
    empty = case["counts"] == 0
    assert int(empty.sum()) >= 3 and float(out.cpu()[empty].abs().max()) == 0.0, "rays without samples write zeros"
    again = k.normals(case["counts"], case["offsets"], torch.full((R, 3), float("nan"), device=device))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "a second launch gave other bits"
    for cut in H.ROUND_CUTS:
        (c1, o1), (c2, o2) = N.split_rounds(case, cut)
        acc = k.normals(c1, o1, torch.full((R, 3), float("nan"), device=device))
        carry = k.carry(c1, o1)
        k.normals(c2, o2, acc, carry_in=carry, accumulate=True)
        fig = N.figure(acc.cpu(), ref)
        _record(f"rounds/cut{cut}", fig)
        print(f"rounds cut {cut}: figure {fig:.3e}  bound {bound:.3e}")
        assert fig <= bound, cut


def test_composite_normals_kernel_special_values(device):
    """beyond the issue's case: the generator's special pre-activations (+30..+70, fp16 max, -inf, dt = 0); rays with a
    capped sample judged apart at the project's factor for them (ngp_oracle.CAPPED_FACTOR, with its reason)"""
    case = H.normals_case(specials=True)
    _assert_classes(case, True)
    m = H.load_margins()
    r = H.normals_reference(case)
    k = _Kernel(case, device)
    out = k.normals(case["counts"], case["offsets"], torch.full((case["R"], 3), float("nan"), device=device)).cpu()
    assert bool(torch.isfinite(out).all())
    c = r["capped_ray"]
    assert int(c.sum()) >= 2
    for key, rows in (("specials/normals", ~c), ("specials/normals_capped", c)):
        fig = N.figure(out[rows], r["S"][rows])
        _record(key, fig)
        print(f"{key}: figure {fig:.3e}  bound {H.bound_for(key, m):.3e}")
        assert fig <= H.bound_for(key, m), key


# ------------------------------------------------------------------------------------------------------------------
# the density gradient of the real chain
# ------------------------------------------------------------------------------------------------------------------
def _small_engine(device, **kw):
    from nerf_vo_amd.ngp_engine import NgpConfig, NgpEngine

    kw.setdefault("march_capacity", 1 << 17)
    return NgpEngine(NgpConfig(num_images=4, capacity=1 << 15, **kw), device)


def _engine_with(case, device, rgb_seed=3, **kw):
    eng = _small_engine(device, **kw)
    n_grid = eng.density_net.n_params - eng.n_density_mlp
    assert eng.n_density_mlp == H.N_DENSITY_MLP and n_grid == case["grid"].numel()
    g = torch.Generator().manual_seed(rgb_seed)
    flat = torch.cat([case["mlp"], case["grid"], (torch.rand(eng.n_rgb, generator=g) * 2 - 1) * 0.3])
    eng.set_params(flat)
    return eng


@pytest.fixture(scope="module")
def gradient_setup():
    from oracle.ngp import NgpOracle

    case = H.gradient_case(NgpOracle(aabb_scale=4).spec.n_params)
    dens, grad = H.gradient_reference(case)
    return case, dens, grad


@pytest.mark.parametrize("optimize_extrinsics", [True, False])
def test_density_gradient_matches_float64_autograd(device, gradient_setup, optimize_extrinsics):
    """``optimize_extrinsics``: the module option prepare_input_gradients as the engine finds it, on and off"""
    case, ref_d, ref_g = gradient_setup
    eng = _engine_with(case, device, optimize_extrinsics=optimize_extrinsics)
    pos = case["positions"].to(device)
    kind = case["kind"]
    floor, share = H.gradient_floor(ref_g, kind)
    assert share <= H.GRAD_MAX_BELOW, (floor, share)
    dens, grad = eng.density_gradient_at(pos)
    torch.cuda.synchronize()
    assert torch.equal(dens.view(torch.int32), eng.density_at(pos).view(torch.int32)), "density differs from density_at"
    dens, grad = dens.cpu(), grad.cpu()
    assert float(dens[kind == 2].abs().max()) == 0.0 and float(grad[kind == 2].abs().max()) == 0.0, "outside points"
    assert bool(torch.isfinite(grad).all())
    face = kind == 1
    assert bool(((grad[face] == 0) == (ref_g[face] == 0)).all()), "the face axis' derivative is zero, the others are not"
    sel = (kind != 2) & (ref_g.norm(dim=1) > floor)
    zero_len = int((grad[sel].norm(dim=1) == 0).sum())
    ang = H.angles_deg(grad[sel], ref_g[sel])
    mx, med = float(ang.max()), float(ang.median())
    rel = float(((grad[sel].double().norm(dim=1) / ref_g[sel].norm(dim=1)) - 1.0).abs().median())
    if optimize_extrinsics:
        _record("chain/max_angle_deg", mx)
        _record("chain/median_angle_deg", med)
        _record("chain/share_below_floor", share)
    ch = H.load_margins().get("chain", {})
    print(f"density gradient: {int(sel.sum())} points above the floor {floor:.3e} (share below {share:.4f}), zero-length {zero_len}, "
          f"angle max {mx:.4f} median {med:.4f} degrees (bounds {ch.get('bound_max_angle_deg')} / {ch.get('bound_median_angle_deg')}), "
          f"median relative length error {rel:.3e}")
    assert zero_len == 0, "zero-length gradients: the 16-bit chain under- or overflowed"
    assert mx <= ch["bound_max_angle_deg"] and med <= ch["bound_median_angle_deg"]
    assert eng._pig == int(optimize_extrinsics)


# ------------------------------------------------------------------------------------------------------------------
# the new path disturbs neither training nor the default render
# ------------------------------------------------------------------------------------------------------------------
def _sequence(device, n=8, H_=60, W_=80):
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    seq = make_sequence(n, H_, W_, device=device, scene_scale=0.2)
    c2w = opencv_to_opengl(seq["camera_extrinsics"])
    c2w[:, :3, 3] += 0.5
    return {"n": n, "H": H_, "W": W_, "intr": seq["camera_intrinsics"], "c2w": c2w[:, :3, :4].contiguous(),
            "images": seq["frames_color"].permute(0, 2, 3, 1).contiguous(),
            "depths": seq["frames_depth"].permute(0, 2, 3, 1).contiguous()}


def _bundle(device, R=300, seed=12):
    g = torch.Generator().manual_seed(seed)
    origins = ((torch.rand(R, 3, generator=g) - 0.5) * 0.3 + 0.5).to(device)
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(device)
    return origins, directions, torch.ones(R, device=device)


_STATE = ("params", "grads", "exp_avg", "exp_avg_sq", "params_half", "params_ema", "params_ema_half", "pose_adjustment",
          "pose_grads", "pose_exp_avg", "pose_exp_avg_sq", "density_grid", "bitfield", "_ema_step_dev", "_applied_dev", "_opt_dev",
          "d_corrections", "_cam_dev", "_cam_applied_dev", "losses", "skip_flag", "_tail_done")
_LOCKSTEP = ("params", "exp_avg", "exp_avg_sq", "params_half", "params_ema", "params_ema_half", "pose_adjustment",
             "pose_exp_avg", "pose_exp_avg_sq", "d_corrections", "_ema_step_dev", "_applied_dev", "_opt_dev", "_cam_dev",
             "_cam_applied_dev")


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.float16 else (x.view(torch.int32) if x.dtype == torch.float32 else x)


def test_normals_render_leaves_training_and_default_render_alone(device):
    """Two engines train four steps; one renders with normals = True between the second and the third.  This back-end has
    no deterministic mode -- the two MLPs' weight gradients and the camera gradient are float-atomic sums -- so, as
    tests/test_ngp_gpu.py compares engines, both start every step from the same state and the same generator seed: the
    range whose step is computed in a fixed order (the hash grid's streamed levels: backward, Adam and weight average)
    must agree bit for bit after every step, the float-atomic rest by that file's drift criterion.  What the render
    itself may touch is compared without any such allowance: every parameter, gradient and optimiser buffer, the
    replica buffers, the counters and the training workspace's gradient rows are the same bits before and after it."""
    from nerf_vo_amd.ngp_engine import NgpConfig, NgpEngine

    s = _sequence(device)
    engines = []
    for _ in range(2):
        torch.manual_seed(9)
        engines.append(NgpEngine(NgpConfig(num_images=s["n"], num_rays=512, capacity=1 << 16, density_update_every=2,
                                           optimize_extrinsics=True, extrinsic_update_every=3, render_capacity=1 << 17), device))
    a, b = engines
    lo, hi = a._fused_adam_plan()
    scale = torch.tensor([s["n"], s["H"], s["W"]], device=device)
    o, d, dn = _bundle(device)
    for it in range(4):
        R = b.rays_per_batch
        assert a.rays_per_batch == R
        idx = torch.floor(torch.rand(R, 3, device=device) * scale).long()
        if it > 0:
            for name in _LOCKSTEP:
                getattr(a, name).copy_(getattr(b, name))
        if it == 2:
            for e in (a, b):  # (every cell occupied for the render; the step behind it rebuilds the bitfield in both engines)
                e.bitfield.fill_(255)
            before ={name: getattr(a, name).clone() for name in _STATE if getattr(a, name) is not None}
            rep = a._dw_rep["buf"].clone()
            ws_t = a._wss[True]
            rows = {kk: ws_t[kk].clone() for kk in ("d_density_out", "d_rgb_out", "dx01", "x01", "density_out")}
            plain0 = a.render_rays(o, d, dn)
            plain0 = {kk: v.clone() for kk, v in plain0.items()}
            with_n = a.render_rays(o, d, dn, normals=True)
            with_n = {kk: v.clone() for kk, v in with_n.items()}
            plain1 = a.render_rays(o, d, dn)
            torch.cuda.synchronize()
            assert set(plain0) == set(plain1) == {"rgb", "depth", "accumulation"} and set(with_n) == set(plain0) | {"normals"}
            for kk in plain0:
                assert torch.equal(_bits(plain0[kk]), _bits(plain1[kk])), f"normals=False after normals=True: {kk} moved"
                assert torch.equal(_bits(plain0[kk]), _bits(with_n[kk])), f"normals=True: {kk} differs from the default render"
            assert float(with_n["accumulation"].max()) > 0.0 and bool(torch.isfinite(with_n["normals"]).all())
            for name, v in before.items():
                assert torch.equal(_bits(getattr(a, name)), _bits(v)), f"the render moved {name}"
            assert torch.equal(a._dw_rep["buf"], rep) and a._wss[True] is ws_t
            for kk, v in rows.items():
                assert torch.equal(_bits(ws_t[kk]), _bits(v)), f"the render moved the training workspace's {kk}"
            assert a._pig == 1
        for e in (a, b):
            torch.manual_seed(100 + it)
            e.train_step(idx, s["intr"], s["c2w"], s["images"], s["depths"])
        torch.cuda.synchronize()
        assert not bool(a.skip_flag.item()) and not bool(b.skip_flag.item())
        for name in ("params", "exp_avg", "exp_avg_sq", "params_half", "params_ema", "params_ema_half"):
            x, y = _bits(getattr(a, name)[lo:hi]), _bits(getattr(b, name)[lo:hi])
            assert torch.equal(x, y), f"step {it}: {name} of the hash grid differs ({int((x != y).sum())} words)"
        assert torch.equal(a._opt_dev, b._opt_dev) and torch.equal(a.density_grid, b.density_grid)
        assert torch.equal(a._cam_dev, b._cam_dev) and torch.equal(a._applied_dev, b._applied_dev)
        dd = (a.params[:lo] - b.params[:lo]).abs()
        assert float((dd > 1e-5 + 1e-3 * b.params[:lo].abs()).float().mean()) < 0.02
        dp = (a.pose_adjustment - b.pose_adjustment).abs()
        assert int((dp > 1e-6 + 1e-3 * b.pose_adjustment.abs()).sum()) <= 2
    assert len(a._graphs) >= 1 and a.step == b.step == 4


# ------------------------------------------------------------------------------------------------------------------
# rounds and halves
# ------------------------------------------------------------------------------------------------------------------
def test_rounds_and_halves_match_a_single_round(device):
    """a bundle whose rays need the second round, on an engine whose packed capacity overflows in both rounds (halves of
    the bundle, halves of the second round's range) against a single-round render on an engine that holds it whole"""
    from oracle.ngp import NgpOracle

    case = H.gradient_case(NgpOracle(aabb_scale=4).spec.n_params)
    case = dict(case, mlp=case["mlp"] * 0.1)    # thin medium (density ~ 1): rays stay alive through hundreds of samples
    R = 257
    big = _engine_with(case, device, render_capacity=1 << 19)
    big.bitfield.fill_(255)
    o, d, dn = _bundle(device, R=R, seed=5)
    whole = big.render_rays(o, d, dn, 0.0, normals=True)
    total = big.last_render_samples
    S_whole = big._wss[False]["out_normal"][:R].double().cpu()
    n_whole = (2.0 * whole["normals"] - 1.0).double().cpu()
    assert float(whole["accumulation"].min()) > 0.5
    bound = H.bound_for("normals", H.load_margins())
    # first round of 16 samples per ray: it fits (the sums stay in one workspace and are compared UNNORMALISED), the second
    # overflows and runs over halves of its range; the default first round of 48: the first round overflows too and the
    # bundle is rendered in halves -- only the normalised output exists, so its error is the sums' amplified by at most
    # 2 / |S| per ray (d(S / |S|) <= 2 |dS| / |S|)
    for first in (16, 48):
        small = _engine_with(case, device, render_capacity=1 << 13, render_first_round=first)
        small.bitfield.fill_(255)
        s0 = small.render_shaded_total
        got = small.render_rays(o, d, dn, 1e-30, normals=True)
        torch.cuda.synchronize()
        assert small.cfg.render_capacity * 4 < total <= big.cfg.render_capacity
        assert (R * first > small.cfg.render_capacity) == (first == 48)
        assert small.render_shaded_total - s0 == total, "both rounds, every sample once"
        for kk in ("rgb", "depth", "accumulation"):
            assert torch.allclose(got[kk], whole[kk], rtol=1e-4, atol=2e-5), kk
        if first == 16:
            fig = N.figure(small._wss[False]["out_normal"][:R].double().cpu(), S_whole)
            print(f"rounds, second round in halves: figure {fig:.3e} (bound {bound:.3e}); {total} samples")
            _record("engine/rounds_halves", fig)
            assert fig <= bound
        else:
            err = ((2.0 * got["normals"] - 1.0).double().cpu() - n_whole).abs().max(dim=1).values
            allowed = 2.0 * bound * float(S_whole.abs().max()) / S_whole.norm(dim=1) + 1e-6
            worst = float((err / allowed).max())
            print(f"both rounds in halves: largest error / allowed {worst:.3f}; smallest |S| {float(S_whole.norm(dim=1).min()):.3e}")
            _record("engine/first_round_halves_ratio", worst)
            assert worst <= 1.0
        plain = small.render_rays(o, d, dn, 1e-30)
        for kk in plain:
            assert torch.equal(plain[kk], got[kk]), kk


# ------------------------------------------------------------------------------------------------------------------
# facade, end to end on a trained room
# ------------------------------------------------------------------------------------------------------------------
def train_room(device, root, seed=0, n=12, H_=68, W_=120, iters=400):
    """12 keyframes of 68 x 120 through the occupancy-grid mapper, 400 steps (as tests/test_mesh_from_nerf_gpu.py trains)"""
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGP
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    torch.manual_seed(seed)
    ds = SyntheticEvaluationDataset(num_frames=2 * n, height=H_, width=W_, scene_scale=0.2, device=device,
                                    dir_dataset=os.path.join(root, "dataset", "room"))
    kf = list(range(0, 2 * n, 2))
    args = argparse.Namespace(num_keyframes=n, frame_height=H_, frame_width=W_, mapping_iterations=iters,
                              mapping_snapshot_iterations=iters, dir_prediction=os.path.join(root, "pred"))
    mapper = InstantNGP(args, device=device)
    mapper.ngp._generator.manual_seed(42 + seed)
    frames = [ds.render(ds.camera_extrinsics[i]) for i in kf]
    color = torch.stack([torch.from_numpy(c) for c, _ in frames]).permute(0, 3, 1, 2).float() / 255.0
    depth = torch.stack([torch.from_numpy(dd) for _, dd in frames])[:, None].float().clamp(0.0, 5.0)
    ci = ds.camera_intrinsics
    intr = torch.tensor([ci["fx"], ci["fy"], ci["cx"], ci["cy"]])
    poses = torch.from_numpy(ds.camera_extrinsics[kf]).float()
    mapper(input={"keyframe_indices": torch.arange(n), "camera_intrinsics": intr.repeat(n, 1).to(device),
                  "camera_extrinsics": opencv_to_opengl(poses.to(device)), "frames_color": color.to(device),
                  "frames_depth": depth.to(device), "last_frame": True})
    while mapper.step < iters:
        mapper(input=None)
    mapper(input=None)
    assert mapper.is_shut_down
    return ds, kf, args, mapper


def frame_normal_figures(ds, nerf, frame):
    """(share of the pixels with accumulation > 0.5 whose rendered normal is within 90 degrees of the room's analytic one,
    their median angle in degrees, their number)"""
    from nerf_vo_amd import pyngp
    from nerf_vo_amd.synthetic import render_room

    ci = ds.camera_intrinsics
    pose = np.asarray(ds.camera_extrinsics[frame], dtype=np.float64)
    n = nerf.render_frame_normal(ci, pose.copy())
    nerf.ngp.render_mode = pyngp.Shade
    acc = nerf.ngp.render(width=ci["width"], height=ci["height"], spp=1, linear=True)[..., 3]
    p = torch.as_tensor(pose, dtype=torch.float32)[None]
    n_cam = render_room(p, ci["height"], ci["width"], (ci["fx"], ci["fy"], ci["cx"], ci["cy"]), half_extent=2.0 * ds.scene_scale)[2]
    n_gt = (n_cam[0].permute(1, 2, 0).double() @ p[0, :3, :3].double().T).numpy()
    hit = acc > 0.5
    cos = np.clip((n.astype(np.float64) * n_gt).sum(-1)[hit], -1.0, 1.0)
    return float((cos > 0).mean()), float(np.degrees(np.arccos(np.median(cos)))), int(hit.sum()), n, acc


@pytest.fixture(scope="module")
def room(device, tmp_path_factory):
    from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGPRenderer

    root = str(tmp_path_factory.mktemp("ngp_normals_room"))
    ds, kf, args, mapper = train_room(device, root)
    return {"ds": ds, "kf": kf, "args": args, "mapper": mapper, "nerf": InstantNGPRenderer(mapping_model=mapper), "root": root}


def test_normals_render_mode(device, room):
    from nerf_vo_amd import pyngp

    nerf, ds = room["nerf"], room["ds"]
    ci = ds.camera_intrinsics
    pose = np.asarray(ds.camera_extrinsics[3], dtype=np.float64)
    nerf._set_rendering_defaults(ci)
    nerf._set_camera_extrinsics(pose)
    tb = nerf.ngp
    tb._render_cache = None
    tb.render_mode = pyngp.Shade
    shade0 =tb.render(width=ci["width"], height=ci["height"], spp=1, linear=True)
    assert tb._render_cache[0][-1] is False
    tb.render_mode = pyngp.Normals
    nrm = tb.render(width=ci["width"], height=ci["height"], spp=1, linear=True)
    cache = tb._render_cache
    assert cache[0][-1] is True
    tb.render_mode = pyngp.Shade
    shade1 = tb.render(width=ci["width"], height=ci["height"], spp=1, linear=True)
    tb.render_mode = pyngp.Depth
    tb.render(width=ci["width"], height=ci["height"], spp=1, linear=True)
    assert tb._render_cache is cache, "a pass with normals serves every mode"
    assert nrm.shape == (ci["height"], ci["width"], 4) and nrm.dtype == np.float32
    assert np.array_equal(shade0, shade1) and np.array_equal(nrm[..., 3], shade0[..., 3])
    hit = nrm[..., 3] > 0.5
    assert hit.mean() > 0.5
    v = 2.0 * (nrm[..., :3][hit].astype(np.float64) / nrm[..., 3:][hit]) - 1.0
    err = float(np.abs(np.linalg.norm(v, axis=1) - 1.0).max())
    print(f"Normals mode: {int(hit.sum())} pixels, | |n| - 1 | <= {err:.2e}")
    assert err <= 1e-5  # float32: (n + 1) / 2 * acc / acc keeps 2^-23 relative of values <= 1, doubled by 2 x - 1


def test_render_frame_normal_against_the_analytic_room(device, room):
    """parity with upstream's picture of this mode is unpinned: the check is against the scene's own geometry"""
    share, med, count, n, acc = frame_normal_figures(room["ds"], room["nerf"], 5)
    ci = room["ds"].camera_intrinsics
    assert n.shape == (ci["height"], ci["width"], 3) and n.dtype == np.float32
    length = np.linalg.norm(n.astype(np.float64), axis=-1)
    assert float(np.abs(length[acc > 0] - 1.0).max()) <= 1e-6 and float(np.abs(n[acc == 0]).max(initial=0.0)) == 0.0
    print(f"render_frame_normal: {count} pixels with accumulation > 0.5, within 90 degrees {share:.4f} "
          f"(>= {FRAME_NORMAL_MIN_SHARE:.4f}), median angle {med:.2f} degrees (<= {FRAME_NORMAL_MAX_MEDIAN_DEG:.2f})")
    _record("frame_normal/share_within_90", share)
    _record("frame_normal/median_angle_deg", med)
    assert count > 0.5 * n.shape[0] * n.shape[1]
    assert share >= FRAME_NORMAL_MIN_SHARE and med <= FRAME_NORMAL_MAX_MEDIAN_DEG


def test_render_point_cloud(device, room, tmp_path):
    import pandas as pd

    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator3D
    from nerf_vo_amd.meshing import read_mesh
    from test_point_cloud_gpu import METRICS

    ds, kf, nerf, mapper = room["ds"], room["kf"], room["nerf"], room["mapper"]
    num_points = 20000
    pred = str(tmp_path / "pred")
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=kf, dir_prediction=pred)
    state_before = mapper.ngp._generator.get_state().clone()
    default_before = torch.cuda.get_rng_state(device).clone()
    path = renderer.render_point_cloud(num_points=num_points)
    assert torch.equal(mapper.ngp._generator.get_state(), state_before), "the export advanced the training stream"
    assert torch.equal(torch.cuda.get_rng_state(device), default_before), "the export drew from torch's default generator"
    raw_path = pred + "/pointcloud/pointcloud_from_nerf_raw.ply"
    assert os.path.exists(path) and os.path.exists(raw_path)
    n_raw, n_face, props, n_body = _ply_layout(raw_path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and n_face == 0 and n_body == 27 * n_raw
    assert num_points // 2 <= n_raw <= num_points, "at most num_points and at least half of them survive the outlier removal"
    v, f, c, nrm = read_mesh(path)
    gt_vertices = ds.mesh()[0][0].double().numpy()
    assert 0 < v.shape[0] <= num_points and f.shape[0] == 0 and c.shape == v.shape
    assert bool(((v.double().numpy() >= gt_vertices.min(axis=0)) & (v.double().numpy() <= gt_vertices.max(axis=0))).all())
    assert float((torch.linalg.norm(nrm.double(), dim=1) - 1.0).abs().max()) <= 1e-6
    print(f"raw {n_raw} of {num_points} points after outlier removal, {v.shape[0]} inside the ground-truth box")
    lower, upper = renderer._ground_truth_box_in_model_frame()[3:]
    raw_bytes = open(raw_path, "rb").read()
    again = nerf.render_point_cloud(str(tmp_path / "again.ply"), lower, upper, num_points=num_points)
    assert open(str(tmp_path / "again.ply"), "rb").read() == raw_bytes, "a second export with the same seed differs"
    assert again["kept"] == n_raw and again["generated"] == num_points
    rv, _, _, rn = read_mesh(raw_path)
    assert torch.equal(rv, again["points"]) and torch.equal(rn, again["normals"])
    assert float((torch.linalg.norm(again["view_directions"].double(), dim=1) - 1.0).abs().max()) <= 1e-6, "unit ray directions"
    assert float((rn * again["view_directions"]).sum(dim=1).max()) <= 1e-6, "a normal that faces away from the ray that saw it"
    assert float((torch.linalg.norm(rn.double(), dim=1) - 1.0).abs().max()) <= 1e-6
    other = nerf.render_point_cloud(str(tmp_path / "other.ply"), lower, upper, num_points=num_points, seed=1, remove_outliers=False)
    assert other["kept"] == other["generated"] == num_points and not torch.equal(other["points"][:100], again["points"][:100])
    Evaluator3D(ds, pred, str(tmp_path / "results")).calculate_metrics_3d_clouds()
    table = pd.read_csv(str(tmp_path / "results" / "metrics_3d_pointcloud.csv"))
    assert list(table.columns) == list(METRICS) + ["mesh"] and table["mesh"].tolist() == ["pointcloud_from_nerf"]
    row = table.iloc[0]
    print({kk: float(row[kk]) for kk in METRICS})
    assert all(np.isfinite(float(row[kk])) for kk in METRICS)


def test_mesh_vertex_attributes(device, room, tmp_path):
    from nerf_vo_amd import pyngp
    from nerf_vo_amd.evaluation import EvaluationRenderer
    from nerf_vo_amd.meshing import read_mesh

    ds, kf, nerf = room["ds"], room["kf"], room["nerf"]
    files = {}
    for attrs in (False, True):
        pred = str(tmp_path / ("attrs" if attrs else "plain"))
        renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=kf, dir_prediction=pred)
        final = renderer.render_mesh(source="nerf", **({"vertex_attributes": True} if attrs else {}))
        files[attrs] = (pred + "/mesh/mesh_from_nerf_raw.ply", final)
    # the default: today's file, positions only
    n_vert, n_face, props, n_body = _ply_layout(files[False][0])
    assert props == ["x", "y", "z"] and n_body == 12 * n_vert + 13 * n_face and n_vert > 0
    lower, upper = renderer._ground_truth_box_in_model_frame()[3:]
    resolution = ((upper - lower) * renderer.pred2gt_transformation["scale_pred2gt"] * 64).astype(int)
    direct = str(tmp_path / "direct.ply")
    nerf.ngp.compute_and_save_marching_cubes_mesh(direct, resolution, pyngp.BoundingBox(lower, upper))
    assert open(direct, "rb").read() == open(files[False][0], "rb").read(), "the default call's file changed"
    for which in (0, 1):
        assert _ply_layout(files[False][which])[2] == ["x", "y", "z"]
        nv, nf, props, n_body = _ply_layout(files[True][which])
        assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and n_body == 27 * nv + 13 * nf
        v0, f0 = read_mesh(files[False][which])[:2]
        v1, f1, c1, n1 = read_mesh(files[True][which])
        assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(f0, f1), "positions / faces moved"
        length = torch.linalg.norm(n1.double(), dim=1)
        zero = int((length == 0).sum())
        print(f"{'final' if which else 'raw'} mesh: {nv} vertices, zero-length normals {zero}, colours mean {c1.float().mean():.1f}")
        assert zero == 0 and float((length - 1.0).abs().max()) <= 1e-6
        assert c1.dtype == torch.uint8 and int(c1.max()) > 0
