#!/usr/bin/env python3
"""Time the dense bundle adjustment (nerf_vo_amd/tracking/dense_ba.py) at the reference's size --
45 x 80 pixels, 12 free poses behind 2 fixed ones, 61 edges, itrs = 2, covariance on -- phase by phase, beside the same
step written in torch ops on the device (``torch_step`` below: batched einsum / index_add for the per-edge terms and the
Schur complement, ``torch.linalg`` for the factorisation).  That formulation is the comparison: it is what one would
write without the kernels.  Prints one JSON line; the numbers quoted in EXPERIMENTS.md section 25 are from

    python tools/dense_ba_bench.py --repeats 20 --warmup 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quat_R(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def hat(v):
    o = torch.zeros_like(v[:, 0])
    return torch.stack([o, -v[:, 2], v[:, 1], v[:, 2], o, -v[:, 0], -v[:, 1], v[:, 0], o], -1).view(-1, 3, 3)


def retract(poses, dx):
    """Exp(dx) * poses for [P, 7] float32 poses and [P, 6] float64 steps (theta well away from 0 is not assumed)."""
    tau, phi = dx[:, :3], dx[:, 3:]
    th2 = (phi * phi).sum(-1)
    th = th2.sqrt().clamp_min(1e-12)
    a, b, c = torch.sin(0.5 * th) / th, (1 - torch.cos(th)) / th2.clamp_min(1e-24), (th - torch.sin(th)) / (th2 * th).clamp_min(1e-36)
    q = torch.cat([a[:, None] * phi, torch.cos(0.5 * th)[:, None]], -1)
    W = hat(phi)
    V = torch.eye(3, dtype=dx.dtype, device=dx.device) + b[:, None, None] * W + c[:, None, None] * (W @ W)
    t = (quat_R(q) @ poses[:, :3, None].double())[:, :, 0] + (V @ tau[:, :, None])[:, :, 0]
    ax, ay, az, aw = q.unbind(-1)
    bx, by, bz, bw = poses[:, 3:].double().unbind(-1)
    qn = torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                      aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)
    return torch.cat([t, qn / qn.norm(dim=-1, keepdim=True)], -1).float()


def torch_step(poses, disps, intr, ii, jj, ks, kx, target, weight, eta, t0, t1, covariance):
    """One iteration in torch ops; returns (poses, disps, depth covariance of the kx rows or None)."""
    K, ht, wd = disps.shape
    HW, P, M, Kx = ht * wd, t1 - t0, ii.numel(), kx.numel()
    n = 6 * P
    fx, fy, cx, cy = intr
    dev = disps.device
    R_all, t_all = quat_R(poses[:, 3:]), poses[:, :3]
    R = R_all[jj] @ R_all[ii].transpose(1, 2)
    t = t_all[jj] - (R @ t_all[ii][:, :, None])[:, :, 0]
    vv, uu = torch.meshgrid(torch.arange(ht, device=dev, dtype=torch.float32), torch.arange(wd, device=dev, dtype=torch.float32),
                            indexing="ij")
    X0, Y0 = ((uu.reshape(-1) - cx) / fx)[None], ((vv.reshape(-1) - cy) / fy)[None]
    h = disps.view(K, HW)[ii]
    x, y, z = (R[:, k, 0, None] * X0 + R[:, k, 1, None] * Y0 + R[:, k, 2, None] + t[:, k, None] * h for k in range(3))
    ok = z >= 0.25
    d = torch.where(ok, 1.0 / z, torch.zeros_like(z))
    d2, zero, one = d * d, torch.zeros_like(z), torch.ones_like(z)
    Jj = torch.stack([torch.stack([fx * h * d, zero, -fx * x * h * d2, -fx * x * y * d2, fx * (one + x * x * d2), -fx * y * d], 1),
                      torch.stack([zero, fy * h * d, -fy * y * h * d2, -fy * (one + y * y * d2), fy * x * y * d2, fy * x * d], 1)], 1)
    Jt, Jp = Jj[:, :, :3], Jj[:, :, 3:]
    A = Jp - torch.cross(t[:, None, :, None].expand_as(Jt), Jt, dim=2)
    Ji = -torch.cat([torch.einsum("mrk,mcrp->mckp", R, Jt), torch.einsum("mrk,mcrp->mckp", R, A)], 2)
    Jz = torch.stack([fx * (t[:, 0, None] * d - t[:, 2, None] * x * d2), fy * (t[:, 1, None] * d - t[:, 2, None] * y * d2)], 1)
    res = target.view(M, 2, HW) - torch.stack([fx * d * x + cx, fy * d * y + cy], 1)
    w = torch.where(ok[:, None], 0.001 * weight.view(M, 2, HW), torch.zeros_like(res))
    a, b = ii - t0, jj - t0
    fa, fb = (a >= 0) & (a < P), (b >= 0) & (b < P)
    B = torch.zeros(P, P, 6, 6, dtype=torch.float64, device=dev)
    v = torch.zeros(P, 6, dtype=torch.float64, device=dev)
    wJi, wJj = w[:, :, None] * Ji, w[:, :, None] * Jj
    Hii, Hjj = torch.einsum("mcap,mcbp->mab", wJi, Ji).double(), torch.einsum("mcap,mcbp->mab", wJj, Jj).double()
    Hij = torch.einsum("mcap,mcbp->mab", wJi, Jj).double()
    vi, vj = torch.einsum("mcap,mcp->ma", wJi, res).double(), torch.einsum("mcap,mcp->ma", wJj, res).double()
    B.index_put_((a[fa], a[fa]), Hii[fa], accumulate=True)
    B.index_put_((b[fb], b[fb]), Hjj[fb], accumulate=True)
    both = fa & fb
    B.index_put_((a[both], b[both]), Hij[both], accumulate=True)
    B.index_put_((b[both], a[both]), Hij[both].transpose(1, 2), accumulate=True)
    v.index_put_((a[fa],), vi[fa], accumulate=True)
    v.index_put_((b[fb],), vj[fb], accumulate=True)
    wJz = w * Jz
    C = torch.zeros(Kx, HW, device=dev).index_add_(0, ks, (wJz * Jz).sum(1))
    wz = torch.zeros(Kx, HW, device=dev).index_add_(0, ks, (wJz * res).sum(1))
    Ei_e, Ej = torch.einsum("mcp,mcap->map", wJz, Ji), torch.einsum("mcp,mcap->map", wJz, Jj)
    Eh = torch.zeros(Kx, P, 6, HW, device=dev)
    Eh.index_put_((ks[fa], a[fa]), Ei_e[fa], accumulate=True)
    Eh.index_put_((ks[fb], b[fb]), Ej[fb], accumulate=True)
    Q = 1.0 / (C + eta.view(Kx, HW))
    E2 = Eh.view(Kx, n, HW).double()
    Qd = Q.double()
    S = B.permute(0, 2, 1, 3).reshape(n, n) - torch.einsum("krp,kcp->rc", E2 * Qd[:, None], E2)
    g = v.reshape(n) - torch.einsum("krp,kp->r", E2, Qd * wz.double())
    L = torch.linalg.cholesky(S)
    dx = torch.cholesky_solve(g[:, None], L)[:, 0]
    poses = poses.clone()
    poses[t0:t1] = retract(poses[t0:t1], dx.view(P, 6))
    dz = Q * (wz - torch.einsum("krp,r->kp", Eh.view(Kx, n, HW), dx.float()))
    disps = disps.clone()
    disps.view(K, HW)[kx] = (disps.view(K, HW)[kx] + dz).clamp_min(0.001)
    cov = None
    if covariance:
        Linv = torch.linalg.solve_triangular(L, torch.eye(n, dtype=L.dtype, device=dev), upper=False)
        F = Qd[:, :, None] * torch.einsum("krp,rc->kpc", E2, Linv.t().contiguous())
        cov = ((Qd + (F * F).sum(-1)) / disps.view(K, HW)[kx].double() ** 4).float()
    return poses, disps, cov


def build_case(device, K=14, t0=2, ht=45, wd=80, seed=0):
    from nerf_vo_amd.tracking import dense_ba as ba

    rng = np.random.default_rng(seed)
    ii, jj = [], []
    for i in range(K):
        for j in range(K):
            if i != j and (abs(i - j) <= 2 or j - i == 3):
                ii.append(i)
                jj.append(j)
    ii, jj = torch.tensor(ii), torch.tensor(jj)
    poses = torch.zeros(K, 7)
    poses[:, 6] = 1
    steps = torch.from_numpy(np.concatenate([0.03 * rng.standard_normal((K, 3)), 0.01 * rng.standard_normal((K, 3))], 1))
    poses = retract(poses, steps * torch.arange(K)[:, None] / 4).to(device)
    vv, uu = np.mgrid[0:ht, 0:wd]
    disps = np.stack([1.0 / (1.2 + 0.8 * (1 + np.sin(3.0 * uu / wd + 0.5 * k) * np.cos(2.0 * vv / ht))) for k in range(K)])
    disps = torch.from_numpy(disps).float().to(device)
    intr = [0.8 * wd, 0.8 * wd, 0.5 * wd, 0.5 * ht]
    target, _ = ba.reproject(poses, disps, intr, ii, jj)
    target = (target + 0.3 * torch.from_numpy(rng.standard_normal(tuple(target.shape))).float().to(device)).contiguous()
    weight = torch.from_numpy(0.2 + 0.8 * rng.random(tuple(target.shape))).float().to(device)
    start = poses.clone()
    start[t0:] = retract(poses[t0:], torch.from_numpy(np.concatenate([0.01 * rng.standard_normal((K - t0, 3)),
                                                                      0.005 * rng.standard_normal((K - t0, 3))], 1)).to(device))
    noisy = (disps * (1 + 0.03 * torch.from_numpy(rng.standard_normal(tuple(disps.shape))).float().to(device))).contiguous()
    kx = torch.unique(ii)
    eta = (0.2 * 1e-3 * torch.ones(kx.numel(), ht, wd) + 1e-7).to(device)
    return dict(K=K, t0=t0, t1=K, ht=ht, wd=wd, intr=intr, ii=ii, jj=jj, poses=start.contiguous(), disps=noisy, target=target,
                weight=weight, eta=eta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--itrs", type=int, default=2)
    opt = ap.parse_args()
    import __graft_entry__ as entry

    entry.build()
    from nerf_vo_amd.tracking import DenseWindow
    from nerf_vo_amd.tracking import dense_ba as ba

    dev = torch.device("cuda:0")
    c = build_case(dev)
    win = DenseWindow(c["K"], c["ht"], c["wd"], c["intr"], dev)

    def timed(fn):
        for _ in range(opt.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(opt.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return float(np.median(ms))

    def hip_ba(cov=True):
        win.cam0_T_world.copy_(c["poses"])
        win.cam0_idepths.copy_(c["disps"])
        win.ba(c["target"], c["weight"], c["eta"], c["ii"], c["jj"], kf0=c["t0"], kf1=c["t1"], itrs=opt.itrs, compute_covariances=cov)

    ii_d, jj_d = c["ii"].to(dev), c["jj"].to(dev)
    kx, ks = torch.unique(ii_d, return_inverse=True)

    def torch_ba(cov=True):
        p, d = c["poses"], c["disps"]
        for it in range(opt.itrs):
            p, d, out = torch_step(p, d, c["intr"], ii_d, jj_d, ks, kx, c["target"], c["weight"], c["eta"], c["t0"], c["t1"],
                                   cov and it == opt.itrs - 1)
        return p, d, out

    res = {"size": f"{c['ht']}x{c['wd']}", "free_poses": c["t1"] - c["t0"], "edges": int(c["ii"].numel()), "itrs": opt.itrs}
    res["hip_ba_ms"], res["hip_ba_no_cov_ms"] = timed(hip_ba), timed(lambda: hip_ba(False))
    res["torch_ba_ms"], res["torch_ba_no_cov_ms"] = timed(torch_ba), timed(lambda: torch_ba(False))
    # the two formulations agree (marginal assembly on both sides)
    hip_ba(False)
    p_t, d_t, _ = torch_ba(False)
    res["max_pose_diff"] = float((win.cam0_T_world - p_t).abs().max())
    res["max_disp_diff"] = float((win.cam0_idepths - d_t).abs().max())
    # phases of one linearisation
    plan = ba.Plan(c["ii"], c["jj"], c["K"], c["t0"], c["t1"], c["ht"], c["wd"], dev)
    sy = ba.linearize(plan, c["poses"], c["disps"], c["intr"], c["target"], c["weight"], c["eta"])
    L, Linv, dx, status = ba.solve(sy.S, sy.g)
    args = dict(poses=c["poses"], disps=c["disps"], intrinsics=c["intr"], target=c["target"], weight=c["weight"], eta=c["eta"], B=sy.B,
                v=sy.v, C=sy.C, wz=sy.wz, Q=sy.Q, Ei=sy.Ei, Ej=sy.Ej, Ehat=sy.Ehat)
    res["plan_ms"] = timed(lambda: ba.Plan(c["ii"], c["jj"], c["K"], c["t0"], c["t1"], c["ht"], c["wd"], dev))
    res["accumulate_ms"] = timed(lambda: plan.call("nvo_ba_accumulate", **args))
    res["schur_ms"] = timed(lambda: plan.call("nvo_ba_schur", Ehat=sy.Ehat, Q=sy.Q, wz=sy.wz, B=sy.B, v=sy.v, S=sy.S, g=sy.g))
    res["solve_ms"] = timed(lambda: ba.solve(sy.S, sy.g, check=False))
    scratch_p, scratch_d = c["poses"].clone(), c["disps"].clone()
    res["update_ms"] = timed(lambda: plan.call("nvo_ba_update", poses=scratch_p, disps=scratch_d, Q=sy.Q, wz=sy.wz, Ehat=sy.Ehat, dx=dx))
    cov = torch.ones_like(c["disps"])
    res["covariance_marginal_ms"] = timed(lambda: ba.depth_covariance(sy.Ehat, sy.Q, Linv.t().contiguous(), c["disps"], cov, plan))
    res["covariance_reference_ms"] = timed(lambda: ba.depth_covariance(ba.ehat_from_E(sy.E, plan, "reference"), sy.Q, Linv, c["disps"], cov, plan))
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
