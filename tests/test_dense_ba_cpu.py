"""The dense bundle adjustment's rule without a GPU: the oracle of helpers/dense_ba_oracle.py
against central differences, its convergence, the cases' "behind" share, its reading of the reference's covariance
indexing against the golden the reference's own lines produced, and the packet's way through the enhancement stage."""
import os

import numpy as np
import pytest
import torch

from helpers import dense_ba_cases as cases
from helpers import dense_ba_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_ba_cov_golden.npz")

# The golden is float32 torch (the reference factors H and multiplies in float32), the oracle float64: measured gap
# max|oracle / golden - 1| = 6.3e-6 on both cases (z_cov and depth_cov alike), so rtol 1e-6 is out of float32's reach.
# Bound: 4 x the measured gap.
GOLDEN_GAP = 6.3e-6
GOLDEN_RTOL = 4 * GOLDEN_GAP


def _f64(c):
    return c["poses"].astype(np.float64), c["disps"].astype(np.float64), c["intrinsics"].astype(np.float64)


def test_jacobians_against_central_differences():
    c = cases.make(K=5, ht=9, wd=13, t0=2)
    P, D, I = _f64(c)
    eps = 1e-6
    for (i, j) in ((2, 4), (3, 1), (0, 2)):
        T = orc.edge_terms(P, D, I, i, j)
        for which, key in ((i, "Ji"), (j, "Jj")):
            for k in range(6):
                xi = np.zeros(6)
                xi[k] = eps
                Pp, Pm = P.copy(), P.copy()
                Pp[which], Pm[which] = orc.retract(P[which], xi), orc.retract(P[which], -xi)
                fd = (orc.edge_terms(Pp, D, I, i, j)["coords"] - orc.edge_terms(Pm, D, I, i, j)["coords"]) / (2 * eps)
                for ch in range(2):
                    scale = max(np.abs(T[key][ch]).max(), 1.0)
                    assert np.abs(fd[ch] - T[key][ch, k]).max() <= 1e-5 * scale, (i, j, key, k, ch)
        Dp, Dm = D.copy(), D.copy()
        Dp[i] += eps
        Dm[i] -= eps
        fd = (orc.edge_terms(P, Dp, I, i, j)["coords"] - orc.edge_terms(P, Dm, I, i, j)["coords"]) / (2 * eps)
        for ch in range(2):
            assert np.abs(fd[ch] - T["Jz"][ch]).max() <= 1e-5 * max(np.abs(T["Jz"][ch]).max(), 1.0), (i, j, "Jz", ch)


@pytest.mark.parametrize("t0", [2, 0], ids=["two-fixed", "prior"])
def test_oracle_converges(t0):
    """Noise-free targets, five frames of 9 x 13, 2 cm / 1 % tangent noise on the free poses and 5 % on the inverse
    depths: the RMS reprojection residual falls by at least 10 x per iteration over the first three.  (Measured: 38, 74,
    331 with two fixed poses; 49, 19, 1009 with the prior.  10 x is a floor against a wrong sign, not a calibration.)"""
    c = cases.make(K=5, ht=9, wd=13, t0=t0)
    p, d = c["poses"].astype(np.float64), c["disps"].astype(np.float64)
    rms = [orc.rms_residual(p, d, c["intrinsics"], c["ii"], c["jj"], c["target"])]
    for _ in range(3):
        out = orc.ba(p, d, c["intrinsics"], c["ii"], c["jj"], c["target"], c["weight"], c["eta"], c["t0"], c["t1"], itrs=1,
                     prior_sigma=c["prior_sigma"])
        p, d = out["poses"], out["disps"]
        rms.append(orc.rms_residual(p, d, c["intrinsics"], c["ii"], c["jj"], c["target"]))
    ratios = [rms[k] / rms[k + 1] for k in range(3)]
    print("rms", rms, "ratios", ratios)
    assert all(r >= 10.0 for r in ratios), ratios


def test_first_pose_free_needs_a_prior():
    c = cases.make(K=5, ht=5, wd=7, t0=0)
    with pytest.raises(ValueError, match="prior_sigma"):
        orc.ba(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"], c["target"], c["weight"], c["eta"], 0, c["t1"])


@pytest.mark.parametrize("name,kw", [g for g in cases.grid() if g[1]["behind"]], ids=lambda v: v if isinstance(v, str) else "")
def test_behind_share(name, kw):
    """On at least one edge of every "behind" case between 5 % and 50 % of the pixels have z < 0.25."""
    c = cases.make(**kw)
    _, valid = orc.reproject(*_f64(c), c["ii"], c["jj"])
    share = 1.0 - valid.reshape(len(c["ii"]), -1).mean(1)
    assert ((share >= 0.05) & (share <= 0.5)).any(), share


def test_cases_hold_the_special_edges():
    c = cases.make(K=5, ht=5, wd=7, t0=2)
    pairs = list(zip(c["ii"].tolist(), c["jj"].tolist()))
    assert len(pairs) - len(set(pairs)) == 1, "one duplicated edge"
    assert any(i < 2 <= j for i, j in pairs) and any(j < 2 <= i for i, j in pairs), "fixed source, fixed target"
    assert 4 in c["jj"] and 4 not in c["ii"], "the last frame is only ever a target"


@pytest.mark.parametrize("tag", ["prior", "fixed2"])
def test_reference_covariance_against_the_golden(tag):
    g = np.load(GOLDEN)
    H, E, Q, d = (g[f"{tag}_{k}"].astype(np.float64) for k in ("H", "E", "Q", "idepths"))
    ii, jj, t0, t1, kx = g[f"{tag}_ii"], g[f"{tag}_jj"], int(g[f"{tag}_kf0"]), int(g[f"{tag}_kf1"]), g[f"{tag}_kx"]
    P = t1 - t0
    Linv = np.linalg.inv(np.linalg.cholesky(H))
    Eh = orc.ehat_reference(E[:P], E[P:], ii, jj, kx, t0, t1)
    z_cov, d_cov = orc.depth_covariance(Eh, Q, Linv, d[kx])
    ref_z, ref_d = g[f"{tag}_z_cov"].reshape(z_cov.shape), g[f"{tag}_depth_cov"][kx].reshape(d_cov.shape)
    gap = max(np.abs(z_cov / ref_z - 1).max(), np.abs(d_cov / ref_d - 1).max())
    print("gap to the golden", gap)
    assert gap <= GOLDEN_RTOL
    # the marginal assembly is a different quantity: the golden tells the two apart
    z_m, _ = orc.depth_covariance(orc.ehat_own(E[:P], E[P:], ii, jj, kx, t0, t1), Q, Linv.T, d[kx])
    assert np.abs(z_m / ref_z - 1).max() > 0.1


def test_packet_goes_through_the_enhancement_stage():
    from nerf_vo_amd.mapping.enhancement import DpvoDepthEnhancement
    from nerf_vo_amd.tracking import DenseWindow

    K, ht, wd = 4, 6, 8
    c = cases.make(K=K, ht=ht, wd=wd, t0=1)
    win = DenseWindow(K, ht, wd, c["intrinsics"], "cpu")
    win.cam0_T_world[:] = torch.from_numpy(c["poses"])
    win.cam0_idepths[:] = torch.from_numpy(c["disps"])
    win.cam0_depths_cov[:] = 0.01 + torch.rand(K, ht, wd, generator=torch.Generator().manual_seed(0))
    mean_before = win.cam0_idepths.mean().item()
    win.normalize(K)
    assert abs(win.cam0_idepths.mean().item() - 1.0) < 1e-5
    np.testing.assert_allclose(win.cam0_T_world[:, :3].numpy(), c["poses"][:, :3] * mean_before, rtol=1e-5, atol=1e-7)
    packet = win.output_packet(torch.arange(K), torch.randint(0, 255, (K, 3, ht, wd)).float(), last_frame=False)
    for k in range(K):  # camera_extrinsics is the inverse of cam0_T_world
        prod = packet["camera_extrinsics"][k].double().numpy() @ orc.pose_matrix(win.cam0_T_world[k].numpy())
        np.testing.assert_allclose(prod, np.eye(4), atol=1e-5)
    out, skip = DpvoDepthEnhancement(method=None, tracking_module="droid-slam").step(packet)
    assert skip is False
    for key in ("frames_depth", "frames_depth_covariance"):
        assert tuple(out[key].shape) == (K, 1, ht, wd), key
        assert torch.isfinite(out[key]).all() and (out[key] > 0).all(), key
    with pytest.raises(RuntimeError, match="GPU"):
        win.ba(torch.zeros(1, 2, ht, wd), torch.zeros(1, 2, ht, wd), torch.zeros(1, ht, wd), torch.tensor([1]), torch.tensor([2]),
               kf0=1)
