"""The dense bundle adjustment of DESIGN.md section 18, restated in numpy with loops over edges and no cleverness.

Everything takes ``dt``: with ``np.float64`` (the default) this is the oracle the kernels are compared against; with
``np.float32`` the per-pixel terms, the per-pixel sums over edges (C, wz, Ei), Q and the depth step are rounded to
float32 the way csrc/dense_ba.hip rounds them, while the block sums, the Schur complement, the solve, the pose
retraction and the covariance's dot products stay float64 as they are on the device.  The difference of the two
renderings is what float32 alone changes (helpers/dense_ba_tolerances.py).

Conventions: poses are cam_T_world rows [tx ty tz qx qy qz qw]; tangent order (tau, phi); G <- Exp(xi) G.
"""
import numpy as np

Z_MIN = 0.25      # a reprojected point counts from this (scaled) depth on
W_SCALE = 0.001   # residual weight = W_SCALE * confidence
D_MIN = 0.001     # inverse depths are clamped here after every step


# ---------------------------------------------------------------------------------------------------------------
# SE3
# ---------------------------------------------------------------------------------------------------------------
def quat_to_R(q):
    x, y, z, w = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=q.dtype)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float64)


def se3_exp(xi):
    """(tau, phi) float64 -> (t, q): q = exp(phi), t = V(phi) tau."""
    xi = np.asarray(xi, np.float64)
    tau, phi = xi[:3], xi[3:]
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    if th < 1e-6:
        a, b, c = 0.5 - th2 / 48.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
        qw = 1.0 - th2 / 8.0
    else:
        a, b, c = np.sin(0.5 * th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
        qw = np.cos(0.5 * th)
    q = np.array([a * phi[0], a * phi[1], a * phi[2], qw])
    W = hat(phi)
    V = np.eye(3) + b * W + c * (W @ W)
    return V @ tau, q


def retract(pose, xi):
    """Exp(xi) * pose in float64, quaternion renormalised."""
    pose = np.asarray(pose, np.float64)
    t, q = se3_exp(xi)
    R = quat_to_R(q)
    qn = quat_mul(q, pose[3:])
    qn = qn / np.sqrt(qn @ qn)
    return np.concatenate([R @ pose[:3] + t, qn])


def pose_matrix(pose):
    pose = np.asarray(pose, np.float64)
    m = np.eye(4)
    m[:3, :3] = quat_to_R(pose[3:])
    m[:3, 3] = pose[:3]
    return m


def relative(poses, i, j, dt):
    """G_ij = G_j G_i^-1 as (R, t) in dt."""
    pi, pj = poses[i].astype(dt), poses[j].astype(dt)
    Ri, Rj = quat_to_R(pi[3:]), quat_to_R(pj[3:])
    R = (Rj @ Ri.T).astype(dt)
    t = (pj[:3] - R @ pi[:3]).astype(dt)
    return R, t


# ---------------------------------------------------------------------------------------------------------------
# per edge and pixel
# ---------------------------------------------------------------------------------------------------------------
def edge_terms(poses, disps, intrinsics, i, j, target=None, weight=None, dt=np.float64, rel=None):
    """Everything of one edge, per pixel.  Jacobians are [2 (channel), 6, HW], Jz [2, HW]."""
    ht, wd = disps.shape[1:]
    fx, fy, cx, cy = (dt(v) for v in intrinsics)
    R, t = relative(poses, i, j, dt) if rel is None else (rel[0].astype(dt), rel[1].astype(dt))
    vv, uu = np.mgrid[0:ht, 0:wd]
    X0 = (uu.ravel().astype(dt) - cx) / fx
    Y0 = (vv.ravel().astype(dt) - cy) / fy
    h = disps[i].reshape(-1).astype(dt)
    x = R[0, 0] * X0 + R[0, 1] * Y0 + R[0, 2] + t[0] * h
    y = R[1, 0] * X0 + R[1, 1] * Y0 + R[1, 2] + t[1] * h
    z = R[2, 0] * X0 + R[2, 1] * Y0 + R[2, 2] + t[2] * h
    ok = z >= dt(Z_MIN)
    d = np.where(ok, dt(1) / np.where(ok, z, dt(1)), dt(0)).astype(dt)
    d2 = d * d
    coords = np.stack([fx * (d * x) + cx, fy * (d * y) + cy])
    zero, one = np.zeros_like(x), np.ones_like(x)
    Jj = np.stack([
        np.stack([fx * (h * d), zero, fx * (-(x * h) * d2), fx * (-(x * y) * d2), fx * (one + (x * x) * d2), fx * (-(y * d))]),
        np.stack([zero, fy * (h * d), fy * (-(y * h) * d2), fy * (-one - (y * y) * d2), fy * ((x * y) * d2), fy * (x * d)]),
    ]).astype(dt)
    Ji = np.empty_like(Jj)
    for c in range(2):
        Jt, Jp = Jj[c, :3], Jj[c, 3:]
        txJ = np.stack([t[1] * Jt[2] - t[2] * Jt[1], t[2] * Jt[0] - t[0] * Jt[2], t[0] * Jt[1] - t[1] * Jt[0]])
        A = Jp - txJ
        for k in range(3):
            Ji[c, k] = -(R[0, k] * Jt[0] + R[1, k] * Jt[1] + R[2, k] * Jt[2])
            Ji[c, 3 + k] = -(R[0, k] * A[0] + R[1, k] * A[1] + R[2, k] * A[2])
    Jz = np.stack([fx * (t[0] * d - (t[2] * x) * d2), fy * (t[1] * d - (t[2] * y) * d2)]).astype(dt)
    out = {"coords": coords.astype(dt), "ok": ok, "z": z, "Ji": Ji, "Jj": Jj, "Jz": Jz}
    if target is not None:
        out["r"] = (target.reshape(2, -1).astype(dt) - coords).astype(dt)
        out["w"] = np.where(ok, dt(W_SCALE) * weight.reshape(2, -1).astype(dt), dt(0)).astype(dt)
    return out


def reproject(poses, disps, intrinsics, ii, jj, dt=np.float64):
    ht, wd = disps.shape[1:]
    coords = np.empty((len(ii), 2, ht, wd), dt)
    valid = np.empty((len(ii), ht, wd), bool)
    for e, (i, j) in enumerate(zip(ii, jj)):
        T = edge_terms(poses, disps, intrinsics, int(i), int(j), dt=dt)
        coords[e] = T["coords"].reshape(2, ht, wd)
        valid[e] = T["ok"].reshape(ht, wd)
    return coords, valid


def accumulate(poses, disps, intrinsics, ii, jj, target, weight, t0, t1, dt=np.float64):
    """B, v (float64), C, wz [Kx, HW], Ei [P, 6, HW], Ej [M, 6, HW] (dt), kx, ok [M, HW]."""
    ht, wd = disps.shape[1:]
    HW, P, M = ht * wd, t1 - t0, len(ii)
    kx = np.unique(ii)
    row = {int(k): s for s, k in enumerate(kx)}
    B, v = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
    C, wz = np.zeros((len(kx), HW), dt), np.zeros((len(kx), HW), dt)
    Ei, Ej = np.zeros((P, 6, HW), dt), np.zeros((M, 6, HW), dt)
    oks = np.zeros((M, HW), bool)

    def total(a):  # a sum over pixels: float32 terms, added in float64 once their products exist
        return a.astype(np.float64).sum(-1) if dt is np.float64 else a.sum(-1, dtype=dt).astype(np.float64)

    for e in range(M):
        i, j = int(ii[e]), int(jj[e])
        a, b = i - t0, j - t0
        T = edge_terms(poses, disps, intrinsics, i, j, target[e], weight[e], dt)
        oks[e] = T["ok"]
        cz, cwz = np.zeros(HW, dt), np.zeros(HW, dt)
        ei, ej = np.zeros((6, HW), dt), np.zeros((6, HW), dt)
        for c in range(2):
            w, r, Ji, Jj, Jz = T["w"][c], T["r"][c], T["Ji"][c], T["Jj"][c], T["Jz"][c]
            wJi, wJj = w * Ji, w * Jj
            if 0 <= a < P:
                B[6 * a:6 * a + 6, 6 * a:6 * a + 6] += total(wJi[:, None] * Ji[None])
                v[6 * a:6 * a + 6] += total(wJi * r)
            if 0 <= b < P:
                B[6 * b:6 * b + 6, 6 * b:6 * b + 6] += total(wJj[:, None] * Jj[None])
                v[6 * b:6 * b + 6] += total(wJj * r)
            if 0 <= a < P and 0 <= b < P:
                blk = total(wJi[:, None] * Jj[None])
                B[6 * a:6 * a + 6, 6 * b:6 * b + 6] += blk
                B[6 * b:6 * b + 6, 6 * a:6 * a + 6] += blk.T
            wJz = w * Jz
            cz = cz + wJz * Jz
            cwz = cwz + wJz * r
            ei = ei + wJz * Ji
            ej = ej + wJz * Jj
        C[row[i]] += cz
        wz[row[i]] += cwz
        if 0 <= a < P:
            Ei[a] += ei
        Ej[e] = ej
    return {"B": B, "v": v, "C": C, "wz": wz, "Ei": Ei, "Ej": Ej, "kx": kx, "ok": oks}


def ehat_own(Ei, Ej, ii, jj, kx, t0, t1):
    """E^_k [Kx, P, 6, HW]: per source frame and free pose, the rows of the cross block that belong to them."""
    P = t1 - t0
    Eh = np.zeros((len(kx), P) + Ei.shape[1:], Ei.dtype)
    for s, k in enumerate(kx):
        if t0 <= k < t1:
            Eh[s, k - t0] = Ei[k - t0]
        for e in range(len(ii)):
            if ii[e] == k and t0 <= jj[e] < t1:
                Eh[s, jj[e] - t0] += Ej[e]
    return Eh


def ehat_reference(Ei, Ej, ii, jj, kx, t0, t1):
    """What the reference's covariance block indexes out of E = [Ei; Ej] ("what the golden
    showed"): for a free source frame EVERY pose row carries that frame's Ei; for a fixed source frame, pose row a
    carries the Ej of the (last) edge from that frame to pose a."""
    P = t1 - t0
    Eh = np.zeros((len(kx), P) + Ei.shape[1:], Ei.dtype)
    for s, k in enumerate(kx):
        if t0 <= k < t1:
            Eh[s, :] = Ei[k - t0]
        else:
            for e in range(len(ii)):
                if ii[e] == k and t0 <= jj[e] < t1:
                    Eh[s, jj[e] - t0] = Ej[e]
    return Eh


def schur(acc, eta, Eh, dt=np.float64, prior_sigma=None):
    """Q (dt), S and g (float64, prior included)."""
    Q = (dt(1) / (acc["C"] + eta.reshape(acc["C"].shape).astype(dt))).astype(dt)
    S, g = acc["B"].copy(), acc["v"].copy()
    for s in range(Eh.shape[0]):
        E = Eh[s].reshape(-1, Eh.shape[-1]).astype(np.float64)
        q = Q[s].astype(np.float64)
        S -= (E * q) @ E.T
        g -= E @ (q * acc["wz"][s].astype(np.float64))
    if prior_sigma is not None:
        S[:6, :6] += np.eye(6) / float(prior_sigma) ** 2
    return Q, S, g


def depth_step(disps, kx, Q, wz, Eh, dx, dt=np.float64):
    out = disps.copy()
    x = dx.astype(dt)
    for s, k in enumerate(kx):
        E = Eh[s].reshape(-1, Eh.shape[-1])
        acc = np.zeros(E.shape[1], dt)
        for r in range(E.shape[0]):
            acc = acc + E[r] * x[r]
        dz = Q[s] * (wz[s] - acc)
        out[k] = np.maximum(disps[k].reshape(-1).astype(dt) + dz, dt(D_MIN)).reshape(disps.shape[1:])
    return out


def depth_covariance(Eh, Q, Mx, disps_kx):
    """z_cov and depth_cov [Kx, HW] of the general form: Q + sum_c (Q sum_r E^[r] M[r, c])^2, then / d^4."""
    z_cov = np.empty(Q.shape)
    for s in range(Eh.shape[0]):
        E = Eh[s].reshape(-1, Eh.shape[-1]).astype(np.float64)
        q = Q[s].astype(np.float64)
        F = q[:, None] * (E.T @ Mx)
        z_cov[s] = q + (F * F).sum(-1)
    d = disps_kx.reshape(Q.shape).astype(np.float64)
    return z_cov, z_cov / d ** 4


def rms_residual(poses, disps, intrinsics, ii, jj, target):
    """RMS of the reprojection residual over every valid pixel of every edge, both channels."""
    tot, n = 0.0, 0
    for e in range(len(ii)):
        T = edge_terms(poses, disps, intrinsics, int(ii[e]), int(jj[e]), target[e], np.ones_like(target[e]))
        tot += float((T["r"][:, T["ok"]] ** 2).sum())
        n += 2 * int(T["ok"].sum())
    return np.sqrt(tot / max(n, 1))


def ba(poses, disps, intrinsics, ii, jj, target, weight, eta, t0, t1, itrs=2, prior_sigma=None, covariance="reference",
       dt=np.float64):
    """The whole step.  Returns the new state, the covariance rows and every intermediate of every iteration."""
    if t0 == 0 and prior_sigma is None:
        raise ValueError("the first pose is free: pass prior_sigma, or the Hessian is singular")
    store = np.float32 if dt is np.float32 else np.float64
    poses, disps = poses.astype(store).copy(), disps.astype(store).copy()
    P, its = t1 - t0, []
    for _ in range(itrs):
        acc = accumulate(poses, disps, intrinsics, ii, jj, target, weight, t0, t1, dt)
        kx = acc["kx"]
        Eh = ehat_own(acc["Ei"], acc["Ej"], ii, jj, kx, t0, t1)
        Q, S, g = schur(acc, eta, Eh, dt, prior_sigma if t0 == 0 else None)
        L = np.linalg.cholesky(S)
        dx = np.linalg.solve(S, g)
        new = poses.astype(np.float64)
        for a in range(P):
            new[t0 + a] = retract(poses[t0 + a], dx[6 * a:6 * a + 6])
        poses = new.astype(store)
        disps = depth_step(disps, kx, Q, acc["wz"], Eh, dx, dt).astype(store)
        its.append(dict(acc, Q=Q, S=S, g=g, L=L, dx=dx, Eh=Eh, poses=poses.copy(), disps=disps.copy()))
    last = its[-1]
    cov = {}
    Linv = np.linalg.inv(last["L"])
    for name in ("reference", "marginal"):
        E = ehat_reference(last["Ei"], last["Ej"], ii, jj, kx, t0, t1) if name == "reference" else last["Eh"]
        z_cov, d_cov = depth_covariance(E, last["Q"], Linv if name == "reference" else Linv.T, disps[kx])
        cov[name] = d_cov.reshape((len(kx),) + disps.shape[1:])
        cov[name + "_z"] = z_cov
    return {"poses": poses, "disps": disps, "kx": kx, "cov": cov, "its": its}
