"""Float64 restatements of the camera-pose gradient chain (pose.hip, ngp.hip's positions backward, sh.hip's float input
gradient), differentiated by torch autograd on the CPU and built on oracle.rays / oracle.sh -- plus the seeded case
generators of tests/test_pose_chain_gpu.py and tests/test_pose_oracle_cpu.py.

Every chain function takes ``dtype=``: float64 is the reference, the float32 run of the SAME function on the same
float32 inputs is the yardstick the bounds come from (bound = factor * e32 + 1e-6, profiles/pose_parity_margins.json;
tests/helpers/pose_tolerances.py writes the e32 figures).  The generators return float32 tensors and stay away from the
places where the chain's derivative jumps (ties of the L-inf contraction's largest component, the SO3xR3 clamp, the box
faces of the occupancy-grid back-end), so that the float32 run itself stays inside its own bound.
"""
from __future__ import annotations

import json
import math
import os

import torch

from oracle import rays as Rr
from oracle import sh as Sh

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARGINS_PATH = os.path.join(ROOT, "profiles", "pose_parity_margins.json")
DEFAULT_FACTOR = 4.0
FLOOR = 1e-6
TIE_MARGIN = 2e-3  # contracted samples keep |p_max| - |p_second| >= this * |p_max| (the issue asks for >= 1e-3)


def figure(got, ref) -> float:
    """max|got - ref| / max|ref| (the atol_scale notion of the suite); plain max|got - ref| where ref is all zero."""
    ref = torch.as_tensor(ref).double()
    got = torch.as_tensor(got).double()
    if ref.numel() == 0:
        return 0.0
    err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
    scale = float(ref.abs().max())
    return err / scale if scale > 0 else err


def load_margins(path: str = MARGINS_PATH) -> dict:
    with open(path) as fh:
        return json.load(fh)


def bound_for(key: str, margins: dict) -> float:
    factor = margins.get("factors", {}).get(key, {}).get("factor", DEFAULT_FACTOR)
    return factor * margins["e32"][key] + FLOOR


# ------------------------------------------------------------------------------------------------------------------
# chain functions
# ------------------------------------------------------------------------------------------------------------------
def _x01_loss(o, d, tbins, dx01, mask):
    """sum dx01 * normalized_positions(sample_positions(o, d, tbins)); samples in ``mask`` [R,S] contribute nothing (a
    bin edge that is not finite may only belong to such samples and is taken out before it reaches the graph)."""
    R, S = tbins.shape[0], tbins.shape[1] - 1
    g = dx01.reshape(R, S, 3)
    if mask is not None:
        bad = ~torch.isfinite(tbins)
        assert not bool(((bad[:, :-1] | bad[:, 1:]) & ~mask).any()), "a sample with a non-finite bin edge is not masked"
        tbins = torch.where(bad, torch.zeros_like(tbins), tbins)
        g = torch.where(mask[:, :, None], torch.zeros_like(g), g)
    x01, _ = Rr.normalized_positions(Rr.sample_positions(o, d, tbins))
    return (g * x01).sum()


def positions_chain(origins, directions, tbins, dx01, mask=None, dtype=torch.float64):
    """L = sum dx01 * x01(o, d, tbins)  ->  (dL/do [R,3], dL/dd [R,3])."""
    o = origins.to(dtype).clone().requires_grad_(True)
    d = directions.to(dtype).clone().requires_grad_(True)
    L = _x01_loss(o, d, tbins.to(dtype), dx01.to(dtype), mask)
    go, gd = torch.autograd.grad(L, (o, d))
    return go, gd


def packed_ranges(counts, offsets, capacity, R_dev=None):
    """(ray, slot) index pairs of the packed samples by the kernel's rules: offset >= capacity -> no samples, a range that
    runs past capacity is cut there, rows >= R_dev have none."""
    rays, slots = [], []
    R = len(counts)
    for r in range(R if R_dev is None else min(R, int(R_dev))):
        off, n = int(offsets[r]), int(counts[r])
        if off >= capacity:
            continue
        n = min(n, capacity - off)
        rays += [r] * n
        slots += list(range(off, off + n))
    return torch.tensor(rays, dtype=torch.long), torch.tensor(slots, dtype=torch.long)


def ngp_positions_chain(counts, offsets, t, origins, directions, aabb_lo, aabb_hi, dx01, capacity, R_dev=None,
                        dtype=torch.float64):
    """x01 = clamp((o + t d - lo) / size, 0, 1) over the packed ranges, L = sum dx01 * x01.  The clamp passes the gradient
    STRICTLY inside the box (a coordinate exactly on a face gets none: the kernel's documented rule; torch.clamp's own
    backward would let it through)."""
    o = origins.to(dtype).clone().requires_grad_(True)
    d = directions.to(dtype).clone().requires_grad_(True)
    ray, slot = packed_ranges(counts, offsets, capacity, R_dev)
    tt = t.to(dtype)[slot]
    x = (o[ray] + tt[:, None] * d[ray] - aabb_lo) / (aabb_hi - aabb_lo)
    inside = (x > 0) & (x < 1)
    x01 = torch.where(inside, x, x.detach().clamp(0, 1))
    L = (dx01.to(dtype)[slot] * x01).sum() + 0.0 * (o.sum() + d.sum())
    go, gd = torch.autograd.grad(L, (o, d))
    return go, gd


def sh_chain(d01, dy, degree, dtype=torch.float64):
    """gradient of sum dy[:, :degree^2] * SH(2 d01 - 1) w.r.t. d01 (oracle.sh.sh_encode maps d01 back itself)."""
    x = d01.to(dtype).clone().requires_grad_(True)
    L = (dy[:, :degree * degree].to(dtype) * Sh.sh_encode(x, degree)).sum() + 0.0 * x.sum()
    return torch.autograd.grad(L, x)[0]


def pose_chain(ray_indices, intrinsics, c2w, d_origin, d_dir, d_dir01, n_cameras, dtype=torch.float64):
    """dL/dcorrection[cam] = sum over the camera's rays of [dL/dd (x) d_raw | dL/do] with dL/dd = d_dir + d_dir01 / 2
    (d_dir01 may be None).  Rays whose camera index is outside [0, n_cameras) are dropped."""
    cam = ray_indices[:, 0]
    keep = (cam >= 0) & (cam < n_cameras)
    cam = cam[keep]
    py = ray_indices[keep, 1].to(dtype) + 0.5
    px = ray_indices[keep, 2].to(dtype) + 0.5
    it = intrinsics.to(dtype)[cam]
    raw = torch.stack([(px - it[:, 2]) / it[:, 0], -(py - it[:, 3]) / it[:, 1], -torch.ones_like(px)], dim=1)
    d0 = torch.einsum("rij,rj->ri", c2w.to(dtype)[cam][:, :, :3], raw)
    d0 = d0 / d0.norm(dim=1, keepdim=True)
    gd = d_dir.to(dtype)[keep]
    if d_dir01 is not None:
        gd = gd + 0.5 * d_dir01.to(dtype)[keep]
    per_ray = torch.cat([gd[:, :, None] * d0[:, None, :], d_origin.to(dtype)[keep][:, :, None]], dim=2)  # [R][3][4]
    return torch.zeros(n_cameras, 3, 4, dtype=dtype).index_add_(0, cam, per_ray)


def exp_map(tangent, mode):
    return (Rr.exp_map_se3 if mode == "SE3" else Rr.exp_map_so3xr3)(tangent)


def exp_chain(tangent, d_corr, mode, trans_penalty, rot_penalty, reg_scale, dtype=torch.float64):
    """gradient of sum d_corr * exp_map(tangent) + reg_scale * camera_opt_regularizer(tangent); also the regulariser's
    value and the forward map.  -> (d_tangent [n,6], reg, corrections [n,3,4])"""
    t = tangent.to(dtype).clone().requires_grad_(True)
    corr = exp_map(t, mode)
    reg = Rr.camera_opt_regularizer(t, trans_penalty, rot_penalty)
    L = (d_corr.to(dtype) * corr).sum() + reg_scale * reg
    return torch.autograd.grad(L, t)[0], reg.detach(), corr.detach()


def corrected_rays(tangent, ray_indices, intrinsics, c2w, mode, dtype=torch.float64):
    ro, rd, _, _ = Rr.generate_rays(ray_indices, intrinsics.to(dtype), c2w.to(dtype))
    return Rr.apply_pose_correction(ro, rd, exp_map(tangent.to(dtype), mode)[ray_indices[:, 0]])


def whole_chain(tangent, ray_indices, intrinsics, c2w, tbins_list, dx01_list, d_sh, mode, trans_penalty, rot_penalty,
                reg_scale, masks=None, dtype=torch.float64):
    """Pose tangent -> dL/dtangent in ONE autograd graph (not a composition of the restatements above): exp_map ->
    apply_pose_correction of the generate_rays output -> sample positions of every level and (d + 1) / 2 ->
    L = sum_k dx01_k * x01_k + sum d_sh * SH4 + reg_scale * regulariser."""
    t = tangent.to(dtype).clone().requires_grad_(True)
    o, d = corrected_rays(t, ray_indices, intrinsics, c2w, mode, dtype)
    L = (d_sh.to(dtype) * Sh.sh_encode((d + 1.0) / 2.0, 4)).sum()
    for k, (tb, dx) in enumerate(zip(tbins_list, dx01_list)):
        L = L + _x01_loss(o, d, tb.to(dtype), dx.to(dtype), None if masks is None else masks[k])
    L = L + reg_scale * Rr.camera_opt_regularizer(t, trans_penalty, rot_penalty)
    return torch.autograd.grad(L, t)[0]


# ------------------------------------------------------------------------------------------------------------------
# case generators (seeded, float32)
# ------------------------------------------------------------------------------------------------------------------
def selector32(origins, directions, tbins):
    """The masked set as float32 arithmetic sees it (rows nvo_sample_positions writes as zeros): used on the CPU, where
    the kernel cannot be asked; the GPU test takes the mask from the kernel itself."""
    with torch.no_grad():
        p = Rr.sample_positions(origins.float(), directions.float(), tbins.float())
        _, sel = Rr.normalized_positions(p)
    return ~sel


def tie_free(origins, directions, tbins):
    """[R] bool: every contracted sample of the ray keeps its largest |component| TIE_MARGIN * mag above the second."""
    tb = tbins.double()
    tb = torch.where(torch.isfinite(tb), tb, torch.zeros_like(tb))
    a = Rr.sample_positions(origins.double(), directions.double(), tb).abs().sort(dim=-1, descending=True).values
    ok = (a[..., 0] < 1.0 - 1e-3) | (a[..., 0] - a[..., 1] >= TIE_MARGIN * a[..., 0])
    return ok.all(dim=1)


def sample_classes(origins, directions, tbins, mask):
    """Counts of the sample classes the positions kernel distinguishes (unmasked samples only)."""
    tb = tbins.double()
    tb = torch.where(torch.isfinite(tb), tb, torch.zeros_like(tb))
    p = Rr.sample_positions(origins.double(), directions.double(), tb)
    mag, m = p.abs().max(dim=-1)
    live = ~mask
    sgn = torch.gather(p, 2, m[..., None])[..., 0] >= 0
    out = {"uncontracted": int((live & (mag < 1)).sum()), "mag_one": int((live & (mag == 1)).sum()),
           "far": int((live & (mag > 500)).sum()), "masked": int(mask.sum()),
           "inf_edge": int((~torch.isfinite(tbins)).sum())}
    for axis in range(3):
        for name, s in (("pos", sgn), ("neg", ~sgn)):
            out[f"contracted_{'xyz'[axis]}_{name}"] = int((live & (mag > 1) & (m == axis) & s).sum())
    return out


POSITIONS_S = (1, 48, 63, 64, 65, 96, 256, 257)
POSITIONS_R = (1, 5, 259)


def _random_rays(n, g, dominant=None):
    """origins in [-0.4, 0.4]^3 and unit directions with one dominant axis (axis and sign cycle over the rays)."""
    o = (torch.rand(n, 3, generator=g) - 0.5) * 0.8
    d = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.6
    k = torch.arange(n) if dominant is None else dominant
    d[torch.arange(n), k % 3] = torch.where((k // 3) % 2 == 0, 1.0, -1.0)
    return o, torch.nn.functional.normalize(d, dim=-1)


def _random_tbins(n, S, g, near=0.05, far=2000.0):
    """sorted bins, uniform in the spacing domain of the samplers (half of them below t = 1, the rest out to ``far``)."""
    s = torch.sort(torch.rand(n, S + 1, generator=g, dtype=torch.float64), dim=1).values
    return Rr.spacing_to_euclidean(s, near, far).float()


def positions_case(R, S, seed=0):
    """origins, directions [R,3], tbins [R,S+1], two dx01 [R*S,3] (the kernel is called once per level into the same
    outputs).  R >= 5: ray 0 is o = (0, 0.25, 0), d = (1, 0, 0) with a bin whose midpoint is exactly 1 (mag == 1), the
    last ray's last bin edge is +inf.  Every other ray is drawn until it is tie-free."""
    g = torch.Generator().manual_seed(1000 * R + S + seed)
    pool = 4 * R + 8
    o, d = _random_rays(pool, g)
    tb = _random_tbins(pool, S, g)
    idx = torch.nonzero(tie_free(o, d, tb))[:, 0]
    # keep the cycle of dominant axes: take the accepted candidates in order
    assert idx.numel() >= R, "positions_case: too few tie-free rays in the pool"
    idx = idx[:R]
    o, d, tb = o[idx].clone(), d[idx].clone(), tb[idx].clone()
    if R >= 5:
        o[0] = torch.tensor([0.0, 0.25, 0.0])
        d[0] = torch.tensor([1.0, 0.0, 0.0])
        edges = 0.75 + 0.5 * torch.arange(S + 1, dtype=torch.float32)  # midpoints 1, 1.5, 2, ...: exact in float32
        tb[0] = edges
        tb[R - 1, S] = float("inf")
    dx_a = torch.randn(R * S, 3, generator=g)
    dx_b = torch.randn(R * S, 3, generator=g)
    return {"origins": o.contiguous(), "directions": d.contiguous(), "tbins": tb.contiguous(), "dx01": (dx_a, dx_b)}


def positions_reference(case, mask, dtype=torch.float64):
    a = positions_chain(case["origins"], case["directions"], case["tbins"], case["dx01"][0], mask, dtype)
    b = positions_chain(case["origins"], case["directions"], case["tbins"], case["dx01"][1], mask, dtype)
    return {"d_origin": a[0], "d_dir": a[1], "d_origin_twice": a[0] + b[0], "d_dir_twice": a[1] + b[1]}


NGP_BOXES = {"pow2": (-1.5, 2.5), "size3": (-1.0, 2.0)}
NGP_COUNTS = (0, 1, 63, 64, 65, 200, 7, 130, 64, 33, 5, 12, 40, 9, 3)


def ngp_case(box, seed=0):
    """Packed samples of R = len(NGP_COUNTS) + on-face rays: counts 0, 1, 63, 64, 65, 200, ...; the range of the ray before
    the last straddles ``capacity``, the last ray's starts beyond it; R_dev = R - 3 (so that both of those and one more lie
    past it in the _dev run).  Samples fall on both sides of every face and keep 1e-3 of the box size from it -- except,
    in the power-of-two box, two rays that lie exactly IN the faces x = lo and x = hi (x01 is exactly 0 or 1 in float32
    and float64 alike: no gradient)."""
    lo, hi = NGP_BOXES[box]
    size = hi - lo
    g = torch.Generator().manual_seed(77 + seed + len(box))
    counts = list(NGP_COUNTS)
    on_face = box == "pow2"
    if on_face:
        counts = counts[:6] + [21, 22] + counts[6:]
    R = len(counts)
    o = lo + size * (0.2 + 0.6 * torch.rand(R, 3, generator=g))
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    if on_face:
        o[6, 0], o[7, 0] = lo, hi
        d[6, 0] = d[7, 0] = 0.0
    offsets, total = [], 0
    for n in counts:
        offsets.append(total)
        total += n + 2  # (gaps: slots no ray owns)
    capacity = offsets[-2] + counts[-2] // 2  # the ray before the last straddles it
    offsets[-1] = capacity + 5                # the last one starts beyond it
    n_slots = offsets[-1] + counts[-1]
    ray, slot = packed_ranges(counts, offsets, n_slots)
    t = torch.zeros(n_slots)
    od, dd = o.double(), d.double()
    todo = torch.ones(ray.numel(), dtype=torch.bool)
    for _ in range(64):  # redraw the t of samples that come within 1e-3 of a face (coordinates lying in a face excepted)
        n = int(todo.sum())
        if n == 0:
            break
        t[slot[todo]] = (torch.rand(n, generator=g) * 1.2 * size).float()
        x = (od[ray] + t[slot].double()[:, None] * dd[ray] - lo) / size
        near = ((x.abs() < 1e-3) | ((x - 1).abs() < 1e-3)) & ~((x == 0) | (x == 1))
        todo = near.any(dim=1)
    assert not bool(todo.any())
    x = (od[ray] + t[slot].double()[:, None] * dd[ray] - lo) / size
    sides = {"below": int((x < 0).sum()), "inside": int(((x > 0) & (x < 1)).sum()), "above": int((x > 1).sum()),
             "on_face": int(((x == 0) | (x == 1)).sum())}
    per_face = [int((x[:, k] < 0).sum()) for k in range(3)] + [int((x[:, k] > 1).sum()) for k in range(3)]
    dx01 = torch.randn(n_slots, 3, generator=g)
    return {"R": R, "capacity": capacity, "R_dev": R - 3, "counts": torch.tensor(counts, dtype=torch.int32),
            "offsets": torch.tensor(offsets, dtype=torch.int32), "t": t, "origins": o.contiguous(),
            "directions": d.contiguous(), "lo": lo, "hi": hi, "dx01": dx01, "sides": sides, "per_face": per_face}


def ngp_reference(case, use_R_dev, dtype=torch.float64):
    go, gd = ngp_positions_chain(case["counts"], case["offsets"], case["t"], case["origins"], case["directions"],
                                 case["lo"], case["hi"], case["dx01"], case["capacity"],
                                 case["R_dev"] if use_R_dev else None, dtype)
    return {"d_origin": go, "d_dir": gd}


def sh_case(degree, N=257, seed=0):
    """d01 [N,3]: the six axes, near-axis directions, random unit directions and non-unit inputs; dy [N,16] with NaN in
    the columns >= degree^2."""
    g = torch.Generator().manual_seed(31 + degree + seed)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    d[:6] = axes
    d[6:12] = torch.nn.functional.normalize(axes + 1e-3 * torch.randn(6, 3, generator=g), dim=-1)
    d[12:18] = torch.nn.functional.normalize(axes + 1e-6 * torch.randn(6, 3, generator=g), dim=-1)
    d[18:60] = d[18:60] * (0.2 + 1.6 * torch.rand(42, 1, generator=g))  # not unit
    dy = torch.randn(N, 16, generator=g)
    dy[:, degree * degree:] = float("nan")
    return {"d01": ((d + 1.0) * 0.5).contiguous(), "dy": dy.contiguous(), "degree": degree}


def sh_reference(case, dtype=torch.float64):
    return {"dd01": sh_chain(case["d01"], case["dy"], case["degree"], dtype)}


POSE_SHAPES = ((1501, 1), (1501, 7), (7552, 48), (4096, 192), (9, 16))
STALE_SHAPES = ((7552, 48), (4096, 192), (1501, 7))  # table path, plain path (of _cams), and an R that is no multiple of 8
STALE_INDICES = (-1, None, 1 << 40)  # None stands for F


def pose_case(R, F, stale=False, seed=0):
    """ray_indices [R,3] int64, intrinsics [F+1,4], c2w [F+1,3,4] (row F holds NaN: n_cameras = F is what the kernels are
    given, so a broken guard reads NaN instead of past the allocation), d_origin / d_dir / d_dir01 [R,3]."""
    g = torch.Generator().manual_seed(R + F + seed)
    H, W = 48, 64
    idx = torch.stack([torch.randint(0, F, (R,), generator=g), torch.randint(0, H, (R,), generator=g),
                       torch.randint(0, W, (R,), generator=g)], dim=1)
    if stale:
        for j, v in enumerate(STALE_INDICES * 3):
            idx[(j * 131 + 17) % R, 0] = F if v is None else v
    intr = torch.tensor([[60.0, 61.0, W / 2, H / 2]]).repeat(F, 1) + torch.rand(F, 4, generator=g)
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g)).Q
    c2w = torch.cat([rot, torch.randn(F, 3, 1, generator=g)], dim=2)
    nan = float("nan")
    intr = torch.cat([intr, torch.full((1, 4), nan)]).contiguous()
    c2w = torch.cat([c2w, torch.full((1, 3, 4), nan)]).contiguous()
    d_o, d_d, d_d01 = (torch.randn(R, 3, generator=g) for _ in range(3))
    return {"R": R, "F": F, "idx": idx.contiguous(), "intr": intr, "c2w": c2w, "d_origin": d_o, "d_dir": d_d,
            "d_dir01": d_d01}


def pose_reference(case, with_d01, dtype=torch.float64):
    F = case["F"]
    return {"d_corr": pose_chain(case["idx"], case["intr"][:F], case["c2w"][:F], case["d_origin"], case["d_dir"],
                                 case["d_dir01"] if with_d01 else None, F, dtype)}


def rays_per_camera_path(R, F):
    """which kernel nvo_pose_bwd_cams takes: the LDS table from 32 rays per camera on (and up to 1024 cameras)."""
    return "table" if (0 < F <= 1024 and R >= 32 * F) else "plain"


EXP_BUCKETS = {"SE3": (0.0, 1e-7, 1e-4, 3e-3, 9.9e-3, 0.0099999, 0.0100001, 1.01e-2, 2e-2, 5e-2, 0.3, 1.0, 2.5, 3.1, 3.2, 6.0),
               "SO3xR3": (0.0, 1e-7, 1e-4, 3e-3, 9.9e-3, 1.01e-2, 2e-2, 5e-2, 0.3, 1.0, 2.5, 3.1, 3.2, 6.0)}
# (name, trans_penalty, rot_penalty, host reg_scale, device scale factor or None)
EXP_VARIANTS = (("pen0", 0.0, 0.0, 1.0, None), ("pen-host", 1e-2, 1e-3, 128.0, None), ("pen-dev", 1e-2, 1e-3, 0.5, 256.0))
EXP_N = (1, 257, 1000)


def exp_case(mode, n=257, seed=0):
    """tangent [n,6]: row i has |w| = bucket[i % n_buckets] about a random axis, translation 0.3 N(0,1) (zero on rows with
    i % 5 == 4: the regulariser's zero-norm branch); d_corr [n,3,4]; bucket [n] the bucket index of every row."""
    buckets = EXP_BUCKETS[mode]
    g = torch.Generator().manual_seed(11 + n + seed + len(mode))
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    b = torch.arange(n) % len(buckets)
    w = (axis * torch.tensor(buckets, dtype=torch.float64)[b][:, None]).float()
    lin = 0.3 * torch.randn(n, 3, generator=g)
    lin[torch.arange(n) % 5 == 4] = 0.0
    w2 = (w.double() ** 2).sum(1)
    if mode == "SO3xR3":
        assert bool(((w2 / 1e-4 - 1).abs() > 1e-5).all()), "a tangent sits on the clamp of exp_map_SO3xR3"
    else:
        assert bool(((w2.sqrt() / 1e-2 - 1).abs() > 5e-6).all()), "a tangent sits on the Taylor switch of exp_map_SE3"
    return {"tangent": torch.cat([lin, w], dim=1).contiguous(), "d_corr": torch.randn(n, 3, 4, generator=g),
            "bucket": b, "buckets": buckets, "mode": mode, "n": n}


def exp_reference(case, variant, dtype=torch.float64):
    _, tp, rp, host, dev = variant
    g, reg, corr = exp_chain(case["tangent"], case["d_corr"], case["mode"], tp, rp, host * (dev or 1.0), dtype)
    return {"d_tangent": g, "reg": reg, "corr": corr}


def bucket_figures(got, ref, case):
    """figure() per |w| bucket -> {bucket label: figure}"""
    return {f"w{w:g}": figure(got[case["bucket"] == k], ref[case["bucket"] == k]) for k, w in enumerate(case["buckets"])}


CHAIN_LEVELS = (256, 96, 48)
CHAIN_W = (0.0, 1e-4, 3e-3, 9.9e-3, 1.01e-2, 5e-2, 0.3)  # both branches of both modes
CHAIN_PENALTIES = (1e-2, 1e-3, 128.0)


def chain_case(mode, R=1501, F=7, seed=0):
    """F cameras on a ring that look at the scene, tangents with |w| = CHAIN_W, R pixels drawn until every corrected ray is
    tie-free at all three levels; bins out to t = 100; dx01 per level and d_sh [R,16] random."""
    g = torch.Generator().manual_seed(5 + seed + len(mode))
    H, W = 48, 64
    axis = torch.nn.functional.normalize(torch.randn(F, 3, generator=g, dtype=torch.float64), dim=-1)
    tangent = torch.cat([0.05 * torch.randn(F, 3, generator=g),
                         (axis * torch.tensor(CHAIN_W, dtype=torch.float64)[:, None]).float()], dim=1)
    tangent[2, :3] = 0.0
    intr = (torch.tensor([[60.0, 61.0, W / 2, H / 2]]).repeat(F, 1) + torch.rand(F, 4, generator=g)).contiguous()
    rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g)).Q
    c2w = torch.cat([rot, (torch.rand(F, 3, 1, generator=g) - 0.5) * 0.6], dim=2).contiguous()
    pool = 6 * R
    idx = torch.stack([torch.arange(pool) % F, torch.randint(0, H, (pool,), generator=g),
                       torch.randint(0, W, (pool,), generator=g)], dim=1)
    tbins = [_random_tbins(pool, S, g, far=100.0) for S in CHAIN_LEVELS]
    with torch.no_grad():
        o, d = corrected_rays(tangent, idx, intr, c2w, mode)
    ok = torch.ones(pool, dtype=torch.bool)
    for tb in tbins:
        ok &= tie_free(o, d, tb)
    keep = torch.nonzero(ok)[:R, 0]
    assert keep.numel() == R, "chain_case: too few tie-free rays in the pool"
    idx = idx[keep].contiguous()
    tbins = [tb[keep].contiguous() for tb in tbins]
    dx01 = [torch.randn(R * S, 3, generator=g) for S in CHAIN_LEVELS]
    d_sh = torch.randn(R, 16, generator=g)
    return {"mode": mode, "R": R, "F": F, "tangent": tangent.contiguous(), "intr": intr, "c2w": c2w, "idx": idx,
            "tbins": tbins, "dx01": dx01, "d_sh": d_sh}


def chain_reference(case, masks=None, dtype=torch.float64):
    tp, rp, scale = CHAIN_PENALTIES
    return {"d_tangent": whole_chain(case["tangent"], case["idx"], case["intr"], case["c2w"], case["tbins"], case["dx01"],
                                     case["d_sh"], case["mode"], tp, rp, scale, masks, dtype)}


# ------------------------------------------------------------------------------------------------------------------
# e32: the float32 run of every reference against its float64 run, per comparison the GPU test makes
# ------------------------------------------------------------------------------------------------------------------
def e32_figures() -> dict:
    out = {}

    def put(prefix, r32, r64, names=None):
        for name in names or r64:
            out[f"{prefix}:{name}"] = figure(r32[name], r64[name])

    for R in POSITIONS_R:
        for S in POSITIONS_S:
            c = positions_case(R, S)
            mask = selector32(c["origins"], c["directions"], c["tbins"])
            put(f"positions/R{R}-S{S}", positions_reference(c, mask, torch.float32), positions_reference(c, mask))
    for box in NGP_BOXES:
        c = ngp_case(box)
        for use_dev in (True, False):
            put(f"ngp/{box}-{'dev' if use_dev else 'host'}", ngp_reference(c, use_dev, torch.float32), ngp_reference(c, use_dev))
    for degree in (1, 2, 3, 4):
        c = sh_case(degree)
        put(f"sh/deg{degree}", sh_reference(c, torch.float32), sh_reference(c))
    for R, F in POSE_SHAPES:
        for stale in (False, True):
            if stale and (R, F) not in STALE_SHAPES:
                continue
            c = pose_case(R, F, stale)
            for with_d01 in (True, False):
                key = f"pose/R{R}-F{F}-{'d01' if with_d01 else 'nod01'}{'-stale' if stale else ''}"
                put(key, pose_reference(c, with_d01, torch.float32), pose_reference(c, with_d01))
    for mode in EXP_BUCKETS:
        c = exp_case(mode)
        for variant in EXP_VARIANTS:
            r32, r64 = exp_reference(c, variant, torch.float32), exp_reference(c, variant)
            for b, v in bucket_figures(r32["d_tangent"], r64["d_tangent"], c).items():
                out[f"exp/{mode}-{variant[0]}:{b}"] = v
        for b, v in bucket_figures(r32["corr"], r64["corr"], c).items():
            out[f"expfwd/{mode}:{b}"] = v
        for n in EXP_N:
            cn = exp_case(mode, n)
            r32, r64 = exp_reference(cn, EXP_VARIANTS[1], torch.float32), exp_reference(cn, EXP_VARIANTS[1])
            out[f"exp/{mode}-n{n}:reg"] = figure(r32["reg"], r64["reg"])
        c = chain_case(mode)
        put(f"chain/{mode}", chain_reference(c, None, torch.float32), chain_reference(c))
    return out
