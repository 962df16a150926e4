"""Dense bundle adjustment over a window of keyframes (csrc/dense_ba.hip, include/nerfvo_hip.h section P; DESIGN.md
section 18): camera poses, per-pixel inverse depths and the marginal depth variance the occupancy-grid mapper trains on
-- the ``ba`` of the reference's DROID front-end (nerf_vo/tracking/droid_slam.py:573-725) without gtsam, whose
HessianFactor bookkeeping reassembles the same reduced system.

Conventions: poses are cam_T_world rows ``[tx ty tz qx qy qz qw]`` float32; inverse depths ``[K, ht, wd]`` float32; one
intrinsics vector ``(fx, fy, cx, cy)``; edges ``ii[e] -> jj[e]`` int64; ``target`` / ``weight`` ``[M, 2, ht, wd]``; ``eta``
``[Kx, ht, wd]`` for the frames ``kx = unique(ii)``; free poses ``t0 <= k < t1``; tangent order (tau, phi), left
perturbation.  Every stage is a HIP kernel; there is no CPU path.  The one exception is the factorisation of a reduced
system of more than ``BA_MAX_NATIVE_N`` = 192 unknowns (more than 32 free poses), which goes through
``torch.linalg.cholesky_ex`` / ``cholesky_solve`` / ``solve_triangular`` on the same float64 ``S`` on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib

COVARIANCES = ("reference", "marginal")


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need(what: str, t, dtype, shape=None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: the tensor must be on the GPU -- there is no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous {dtype} tensor, got {t.dtype} (contiguous: {t.is_contiguous()})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(shape)} expected, got {tuple(t.shape)}")


class Plan:
    """The frame graph of one call, validated by the library before anything is launched: ``kx``, the edges by source
    frame, and the device memory for those tables and the kernels' scratch."""

    def __init__(self, ii, jj, K: int, t0: int, t1: int, ht: int, wd: int, device):
        self.lib = _lib.lib()
        self.handle = None
        ii_h = np.ascontiguousarray(torch.as_tensor(ii).detach().cpu().numpy().astype(np.int64).reshape(-1))
        jj_h = np.ascontiguousarray(torch.as_tensor(jj).detach().cpu().numpy().astype(np.int64).reshape(-1))
        if ii_h.shape != jj_h.shape:
            raise ValueError(f"dense_ba: ii and jj differ in length ({ii_h.size} and {jj_h.size})")
        for name, val in (("K", K), ("t0", t0), ("t1", t1), ("ht", ht), ("wd", wd)):
            if not 0 <= int(val) < 2 ** 31:
                raise ValueError(f"dense_ba: {name} = {val} is out of range")
        handle = C.c_void_p()
        _lib.check(self.lib.nvo_ba_plan_create(ii_h.ctypes.data_as(C.c_void_p), jj_h.ctypes.data_as(C.c_void_p), ii_h.size, int(K),
                                               int(t0), int(t1), int(ht), int(wd), C.byref(handle)), "nvo_ba_plan_create")
        self.handle = handle
        self.device = torch.device(device)
        self.M, self.K, self.t0, self.t1, self.P, self.ht, self.wd, self.HW = ii_h.size, K, t0, t1, t1 - t0, ht, wd, ht * wd
        self.ii_host, self.jj_host = ii_h, jj_h
        self.Kx = int(self.lib.nvo_ba_plan_kx(handle, None))
        kx = np.zeros(self.Kx, np.int64)
        self.lib.nvo_ba_plan_kx(handle, kx.ctypes.data_as(C.c_void_p))
        self.kx_host = kx
        self.kx = torch.from_numpy(kx).to(self.device)
        nbytes = int(self.lib.nvo_ba_plan_bytes(handle))
        self.memory = torch.empty(nbytes + 16, dtype=torch.uint8, device=self.device)
        base = self.memory.data_ptr()
        self._base = base + (-base) % 16
        _lib.check(self.lib.nvo_ba_plan_bind(_stream(self.device), handle, C.c_void_p(self._base), nbytes), "nvo_ba_plan_bind")

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.nvo_ba_plan_destroy(self.handle)
            self.handle = None

    def call(self, name: str, **fields) -> None:
        args = _lib.BaArgs()
        for key, val in fields.items():
            if isinstance(val, torch.Tensor):
                val = val.data_ptr()
            elif key == "intrinsics":
                val = (C.c_float * 4)(*[float(x) for x in val])
            setattr(args, key, val)
        _lib.check(getattr(self.lib, name)(_stream(self.device), self.handle, C.byref(args)), name)


def _intr(intrinsics):
    vals = [float(x) for x in torch.as_tensor(intrinsics).detach().cpu().reshape(-1)]
    if len(vals) != 4:
        raise ValueError("dense_ba: intrinsics are (fx, fy, cx, cy)")
    return vals


def _check_state(plan: Plan, poses, disps) -> None:
    _need("dense_ba: poses", poses, torch.float32, (plan.K, 7))
    _need("dense_ba: inverse depths", disps, torch.float32, (plan.K, plan.ht, plan.wd))


def reproject(poses, disps, intrinsics, ii, jj, plan: Plan | None = None):
    """Coordinates ``[M, 2, ht, wd]`` of every source pixel in its edge's target frame and the mask ``[M, ht, wd]`` of
    the pixels in front of it (the reference's ``reproject``, :1206-1218, without the Jacobians)."""
    K, ht, wd = (int(v) for v in disps.shape)
    plan = plan or Plan(ii, jj, K, 0, K, ht, wd, disps.device)
    _check_state(plan, poses, disps)
    coords = torch.empty(plan.M, 2, ht, wd, dtype=torch.float32, device=plan.device)
    valid = torch.empty(plan.M, ht, wd, dtype=torch.uint8, device=plan.device)
    plan.call("nvo_ba_reproject", poses=poses, disps=disps, intrinsics=_intr(intrinsics), coords=coords, valid=valid)
    return coords, valid.bool()


class System:
    """Everything ``accumulate`` + ``schur`` leave on the device for one linearisation."""

    def __init__(self, plan: Plan):
        dev, P, M, Kx, HW, n = plan.device, plan.P, plan.M, plan.Kx, plan.HW, 6 * plan.P
        f32, f64 = torch.float32, torch.float64
        self.plan = plan
        self.B, self.v = torch.empty(n, n, dtype=f64, device=dev), torch.empty(n, dtype=f64, device=dev)
        self.S, self.g = torch.empty(n, n, dtype=f64, device=dev), torch.empty(n, dtype=f64, device=dev)
        self.C, self.wz, self.Q = (torch.empty(Kx, HW, dtype=f32, device=dev) for _ in range(3))
        self.E = torch.empty(P + M, 6, HW, dtype=f32, device=dev)  # the upstream layout: Ei rows, then Ej rows
        self.Ei, self.Ej = self.E[:P], self.E[P:]
        self.Ehat = torch.empty(Kx, P, 6, HW, dtype=f32, device=dev)


def linearize(plan: Plan, poses, disps, intrinsics, target, weight, eta, prior_sigma=None) -> System:
    _check_state(plan, poses, disps)
    _need("dense_ba: target", target, torch.float32, (plan.M, 2, plan.ht, plan.wd))
    _need("dense_ba: weight", weight, torch.float32, (plan.M, 2, plan.ht, plan.wd))
    _need("dense_ba: eta", eta, torch.float32, (plan.Kx, plan.ht, plan.wd))
    if plan.t0 == 0 and prior_sigma is None:
        raise ValueError("dense_ba: the first pose is free (t0 == 0): pass prior_sigma (the reference uses 1e-4), or the "
                         "Hessian is ill-conditioned")
    sy = System(plan)
    plan.call("nvo_ba_accumulate", poses=poses, disps=disps, intrinsics=_intr(intrinsics), target=target, weight=weight, eta=eta,
              B=sy.B, v=sy.v, C=sy.C, wz=sy.wz, Q=sy.Q, Ei=sy.Ei, Ej=sy.Ej, Ehat=sy.Ehat)
    prior = 1.0 / float(prior_sigma) ** 2 if (plan.t0 == 0 and prior_sigma is not None) else 0.0
    plan.call("nvo_ba_schur", Ehat=sy.Ehat, Q=sy.Q, wz=sy.wz, B=sy.B, v=sy.v, S=sy.S, g=sy.g, prior_weight=prior)
    return sy


def reduced_camera_matrix(poses, disps, intrinsics, target, weight, eta, ii, jj, t0: int, t1: int, prior_sigma=None):
    """``H, v, Q, E, w`` in the upstream shapes: the reduced system ``H [6P, 6P]`` and ``v [6P]`` (float64, prior
    included), ``Q [Kx, HW]``, ``E = [Ei (P rows); Ej (M rows)]`` each ``[6, HW]``, and ``w [Kx, HW]``."""
    K, ht, wd = (int(v) for v in disps.shape)
    sy = linearize(Plan(ii, jj, K, t0, t1, ht, wd, disps.device), poses, disps, intrinsics, target, weight, eta, prior_sigma)
    return sy.S, sy.g, sy.Q, sy.E, sy.wz


def solve(S: torch.Tensor, g: torch.Tensor, check: bool = True):
    """``L, Linv, dx, status`` of ``S = L L'``, ``dx = S^-1 g`` in float64 on the device: the library's one-workgroup
    Cholesky up to 192 unknowns, ``torch.linalg`` above.  With ``check`` a pivot that is not positive raises."""
    n = int(S.shape[0])
    _need("dense_ba: S", S, torch.float64, (n, n))
    _need("dense_ba: g", g, torch.float64, (n,))
    if n <= _lib.BA_MAX_NATIVE_N:
        L, Linv = torch.empty_like(S), torch.empty_like(S)
        dx = torch.empty_like(g)
        status = torch.empty(1, dtype=torch.int32, device=S.device)
        _lib.check(_lib.lib().nvo_ba_solve(_stream(S.device), n, S.data_ptr(), g.data_ptr(), L.data_ptr(), Linv.data_ptr(),
                                           dx.data_ptr(), status.data_ptr()), "nvo_ba_solve")
    else:
        L, info = torch.linalg.cholesky_ex(S)
        status = info.to(torch.int32).reshape(1)
        dx = torch.cholesky_solve(g[:, None], L)[:, 0].contiguous()
        Linv = torch.linalg.solve_triangular(L, torch.eye(n, dtype=S.dtype, device=S.device), upper=False).contiguous()
        L = L.contiguous()
    if check and int(status.item()) != 0:
        raise RuntimeError(f"dense_ba: the reduced system is not positive definite (pivot {int(status.item())})")
    return L, Linv, dx, status


def _rows_by_source(plan: Plan):
    row = {int(k): s for s, k in enumerate(plan.kx_host)}
    return [row[int(i)] for i in plan.ii_host]


def ehat_from_E(E, plan: Plan, assembly: str = "marginal"):
    """``E^ [Kx, P, 6, HW]`` out of the upstream ``E``.  ``"marginal"``: per source frame and free pose the rows of the
    Hessian's cross block (what ``accumulate`` builds itself).  ``"reference"``: what the reference's covariance block
    indexes out of ``E``: every pose row of a free source frame carries that frame's ``Ei``; a
    fixed source frame's row ``a`` carries the ``Ej`` of its last edge to pose ``a``."""
    if assembly not in COVARIANCES:
        raise ValueError(f"dense_ba: covariance assembly {assembly!r}; one of {COVARIANCES}")
    P, t0 = plan.P, plan.t0
    Ei, Ej = E[:P], E[P:]
    Eh = torch.zeros(plan.Kx, P, 6, plan.HW, dtype=E.dtype, device=E.device)
    ks = _rows_by_source(plan)
    free = [(s, int(k) - t0) for s, k in enumerate(plan.kx_host) if t0 <= k < plan.t1]
    if free:
        rows = torch.tensor([s for s, _ in free], device=E.device)
        own = torch.tensor([a for _, a in free], device=E.device)
        if assembly == "reference":
            Eh[rows] = Ei[own][:, None]
        else:
            Eh[rows, own] = Ei[own]
    for e in range(plan.M):  # edge order: a duplicate adds again ("marginal") or overwrites ("reference")
        i, b = int(plan.ii_host[e]), int(plan.jj_host[e]) - t0
        if not 0 <= b < P:
            continue
        if assembly == "marginal":
            Eh[ks[e], b] += Ej[e]
        elif not t0 <= i < plan.t1:
            Eh[ks[e], b] = Ej[e]
    return Eh


def solve_depth(dx, disps, Q, E, w, ii, jj, t0: int, t1: int):
    """``d <- max(d + Q (w - E^' dx), 0.001)`` in place on the frames ``unique(ii)`` (the upstream ``solve_depth`` with the
    reference's clamp, :672-674)."""
    K, ht, wd = (int(v) for v in disps.shape)
    plan = Plan(ii, jj, K, t0, t1, ht, wd, disps.device)
    _need("dense_ba: inverse depths", disps, torch.float32, (K, ht, wd))
    _need("dense_ba: Q", Q, torch.float32, (plan.Kx, plan.HW))
    _need("dense_ba: w", w, torch.float32, (plan.Kx, plan.HW))
    _need("dense_ba: E", E, torch.float32, (plan.P + plan.M, 6, plan.HW))
    dx = dx.to(torch.float64).reshape(-1).contiguous()
    _need("dense_ba: dx", dx, torch.float64, (6 * plan.P,))
    plan.call("nvo_ba_update", disps=disps, Q=Q, wz=w, Ehat=ehat_from_E(E, plan, "marginal"), dx=dx)
    return disps


def depth_covariance(Ehat, Q, Mx, disps, cov, plan: Plan):
    """The general form: ``cov[kx] = (Q + sum_c (Q sum_r E^[r] Mx[r, c])^2) / d^4``, written into the ``kx`` rows of ``cov``."""
    n = 6 * plan.P
    _need("dense_ba: Ehat", Ehat, torch.float32, (plan.Kx, plan.P, 6, plan.HW))
    _need("dense_ba: Q", Q, torch.float32, (plan.Kx, plan.HW))
    _need("dense_ba: Mx", Mx, torch.float64, (n, n))
    _need("dense_ba: inverse depths", disps, torch.float32, (plan.K, plan.ht, plan.wd))
    _need("dense_ba: covariance", cov, torch.float32, (plan.K, plan.ht, plan.wd))
    plan.call("nvo_ba_covariance", disps=disps, Q=Q, Ehat=Ehat, Mx=Mx, cov=cov)
    return cov


def pose_matrices(poses: torch.Tensor) -> torch.Tensor:
    """``[N, 7]`` rows -> ``[N, 4, 4]`` matrices."""
    t, q = poses[:, :3], poses[:, 3:]
    x, y, z, w = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)
    m = torch.zeros(poses.shape[0], 4, 4, dtype=poses.dtype, device=poses.device)
    m[:, :3, :3], m[:, :3, 3], m[:, 3, 3] = R, t, 1
    return m


def inverse_rigid(m: torch.Tensor) -> torch.Tensor:
    """Inverse of ``[N, 4, 4]`` rigid transforms: ``[R' | -R' t]``."""
    out = torch.zeros_like(m)
    Rt = m[:, :3, :3].transpose(1, 2)
    out[:, :3, :3] = Rt
    out[:, :3, 3] = -(Rt @ m[:, :3, 3:])[:, :, 0]
    out[:, 3, 3] = 1
    return out


class DenseWindow:
    """The keyframe buffers of the reference's DROID front-end that bundle adjustment reads and writes, under its names:
    ``cam0_T_world [K, 7]``, ``cam0_idepths``, ``cam0_depths_cov``, ``damping`` (each ``[K, ht, wd]``).  Where it sits
    relative to ``MappingModule``: INTEGRATION.md."""

    def __init__(self, num_keyframes: int, ht: int, wd: int, intrinsics, device):
        self.device = torch.device(device)  # the buffers and the packet are plain tensors; ba() itself needs the GPU
        self.num_keyframes, self.ht, self.wd = int(num_keyframes), int(ht), int(wd)
        self.cam0_intrinsics = torch.tensor(_intr(intrinsics), dtype=torch.float32, device=self.device)
        self.cam0_T_world = torch.zeros(num_keyframes, 7, dtype=torch.float32, device=self.device)
        self.cam0_T_world[:, 6] = 1.0
        self.cam0_idepths = torch.ones(num_keyframes, ht, wd, dtype=torch.float32, device=self.device)
        self.cam0_depths_cov = torch.ones(num_keyframes, ht, wd, dtype=torch.float32, device=self.device)
        self.damping = 1e-6 * torch.ones(num_keyframes, ht, wd, dtype=torch.float32, device=self.device)
        self.last = None  # the last call's System, L, Linv, dx (for inspection and tests)

    def ba(self, target, weight, damping, ii, jj, kf0: int = 0, kf1=None, itrs: int = 2, lm: float = 1e-4, ep: float = 0.1,
           compute_covariances: bool = True, prior_sigma=None, covariance: str = "reference") -> None:
        """The reference's ``ba`` (:573-725).  ``damping [Kx, ht, wd]`` is the eta of the frames ``unique(ii)``, i.e.
        ``0.2 * self.damping[kx] + 1e-7`` as the reference's callers form it (:402).  ``lm`` and ``ep`` are accepted and
        ignored, as in the reference's body.  ``prior_sigma`` is required when ``kf0 == 0``; the prior's mean is the pose
        itself.  ``covariance``: ``"reference"`` (what the reference's lines compute) or ``"marginal"``.  A reduced system
        that is not positive definite leaves poses and depths as they were and raises."""
        if self.device.type != "cuda":
            raise RuntimeError("DenseWindow.ba: the window must live on the GPU -- there is no CPU fallback")
        if covariance not in COVARIANCES:
            raise ValueError(f"dense_ba: covariance {covariance!r}; one of {COVARIANCES}")
        if kf0 == 0 and prior_sigma is None:
            raise ValueError("dense_ba: kf0 == 0 needs prior_sigma (the reference uses 1e-4 on all six components): without a "
                             "prior on the first pose the Hessian is ill-conditioned")
        if itrs < 1:
            raise ValueError("dense_ba: itrs must be at least 1")
        if kf1 is None:
            kf1 = int(max(int(torch.as_tensor(ii).max()), int(torch.as_tensor(jj).max()))) + 1
        plan = Plan(ii, jj, self.num_keyframes, int(kf0), int(kf1), self.ht, self.wd, self.device)
        poses0, disps0 = self.cam0_T_world.clone(), self.cam0_idepths.clone()
        intr = _intr(self.cam0_intrinsics)
        bad = []
        for _ in range(itrs):
            sy = linearize(plan, self.cam0_T_world, self.cam0_idepths, intr, target, weight, damping, prior_sigma)
            L, Linv, dx, status = solve(sy.S, sy.g, check=False)
            plan.call("nvo_ba_update", poses=self.cam0_T_world, disps=self.cam0_idepths, Q=sy.Q, wz=sy.wz, Ehat=sy.Ehat, dx=dx,
                      status=status)
            bad.append(status)
        if int(torch.cat(bad).abs().max().item()) != 0:  # the one synchronisation of the call
            self.cam0_T_world.copy_(poses0)
            self.cam0_idepths.copy_(disps0)
            raise RuntimeError("dense_ba: the reduced system is not positive definite; poses and depths are unchanged")
        self.last = {"system": sy, "L": L, "Linv": Linv, "dx": dx, "plan": plan}
        if compute_covariances:
            if covariance == "reference":
                Eh, Mx = ehat_from_E(sy.E, plan, "reference"), Linv
            else:
                Eh, Mx = sy.Ehat, Linv.t().contiguous()
            depth_covariance(Eh, sy.Q, Mx, self.cam0_idepths, self.cam0_depths_cov, plan)

    def normalize(self, last_kf: int = -1) -> None:
        """Mean inverse depth 1 over the frames ``[:last_kf]`` (:1225-1229)."""
        s = self.cam0_idepths[:last_kf].mean()
        self.cam0_idepths[:last_kf] /= s
        self.cam0_T_world[:last_kf, :3] *= s

    def output_packet(self, frame_indices, frames_color, last_frame: bool = False) -> dict:
        """The dictionary of :929-952 at ``ht x wd`` with the intrinsics of that resolution;
        ``camera_extrinsics = inv(cam0_T_world)`` as 4 x 4 matrices."""
        idx = torch.as_tensor(frame_indices, dtype=torch.long, device=self.device)
        n = int(idx.numel())
        return {"keyframe_indices": idx,
                "camera_intrinsics": self.cam0_intrinsics[None].expand(n, 4).clone(),
                "camera_extrinsics": inverse_rigid(pose_matrices(self.cam0_T_world[idx])),
                "frames_color": torch.as_tensor(frames_color).to(self.device),
                "droid_slam_inverse_depth": self.cam0_idepths[idx],
                "droid_slam_depth_covariance": self.cam0_depths_cov[idx],
                "last_frame": last_frame}
