"""Cases of the dense bundle adjustment tests: a small window of cameras a few centimetres and
about a degree apart in front of a smooth surface 1.2 to 2.8 deep, a flow target from the true geometry, confidences in
[0.2, 1], and a frame graph |i - j| <= 2 both ways that also holds a duplicated edge, edges whose source or target is a
fixed pose, and a frame that is only ever a target (the last one).  numpy's PCG64 throughout."""
import numpy as np

from helpers import dense_ba_oracle as orc

SHAPES = ((5, 7), (9, 13), (24, 40))
FRAMES = (5, 7)
PRIOR_SIGMA = 1e-4
# The comparison cases damp the depths at about the size of C (eta ~ 3e-4): with the first pose held by the prior alone
# the scale of the window is fixed by eta only, and at the 1e-6 of the convergence cases float32 rounding of the
# per-pixel terms already moves dx by more than its own size (helpers/dense_ba_tolerances.py measured 1.4), which would
# leave the comparison without content.
GRID_DAMPING = 1e-3
BEHIND_SHARE = 0.3   # "behind" variant: the share of its predecessor's pixels the pushed camera leaves behind Z_MIN


def intrinsics(ht, wd):
    return np.array([0.8 * wd, 0.8 * wd, 0.5 * wd - 0.25, 0.5 * ht + 0.25])


def true_disps(K, ht, wd):
    v, u = np.mgrid[0:ht, 0:wd]
    d = np.empty((K, ht, wd))
    for k in range(K):
        s = 0.5 + 0.5 * np.sin(2.1 * u / wd + 0.7 * k) * np.cos(1.7 * v / ht - 0.4 * k)
        d[k] = 1.0 / (1.2 + 1.6 * s)
    return d


def true_poses(K, behind=None, disps=None):
    poses = np.zeros((K, 7))
    poses[:, 6] = 1.0
    for k in range(1, K):
        xi = np.array([0.035 * k, 0.012 * np.sin(1.3 * k), 0.006 * k, 0.004 * k, -0.017 * k, 0.006 * np.cos(k)])
        poses[k] = orc.retract(poses[0], xi)
    if behind is not None:
        # cam_T_world: a step forward takes the points' z down.  z = 1 + t_z d up to the small rotation, so the step
        # that leaves BEHIND_SHARE of the predecessor's pixels with z < Z_MIN follows from that frame's depths
        push = (1.0 - orc.Z_MIN) / np.quantile(disps[behind - 1], 1.0 - BEHIND_SHARE)
        poses[behind] = orc.retract(poses[behind], np.array([0, 0, -push, 0, 0, 0.0]))
    return poses


def edges(K, t0, chain=False, full=False):
    """|i - j| <= 2 both ways (chain: 1); the last frame has no outgoing edge; one duplicate at the end.  ``full``: every
    frame is a source and no edge is repeated -- the graphs on which the reference's covariance indexing runs."""
    reach = 1 if chain else 2
    ii, jj = [], []
    for i in range(K if full else K - 1):
        for j in range(K):
            if i != j and abs(i - j) <= reach:
                ii.append(i)
                jj.append(j)
    if not full:
        ii.append(min(t0, K - 2))  # the duplicate: first free pose -> its successor
        jj.append(min(t0, K - 2) + 1)
    return np.array(ii, np.int64), np.array(jj, np.int64)


def make(K=5, ht=9, wd=13, t0=2, behind=False, noise=0.0, seed=0, chain=False, perturb=True, damping=1e-6, full=False):
    """A dictionary: intrinsics, ii, jj, t0, t1, target, weight, eta, the true state and the perturbed start."""
    rng = np.random.default_rng(1000 * seed + 31 * K + ht * wd + (7 if behind else 0))
    t1 = K
    intr = intrinsics(ht, wd)
    pushed = K - 2 if behind else None
    disps_true = true_disps(K, ht, wd)
    poses_true = true_poses(K, pushed, disps_true)
    ii, jj = edges(K, t0, chain, full)
    target, _ = orc.reproject(poses_true, disps_true, intr, ii, jj)
    target = target + noise * rng.standard_normal(target.shape)
    weight = 0.2 + 0.8 * rng.random(target.shape)
    kx = np.unique(ii)
    eta = 0.2 * damping * (1.0 + rng.random((len(kx), ht, wd))) + 1e-7  # as the caller of ba() forms it
    poses, disps = poses_true.copy(), disps_true.copy()
    if perturb:
        for k in range(t0, t1):
            xi = np.concatenate([0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)])
            poses[k] = orc.retract(poses_true[k], xi)
        disps = disps_true * (1.0 + 0.05 * rng.standard_normal(disps.shape))
    f32 = np.float32
    return {"K": K, "ht": ht, "wd": wd, "t0": t0, "t1": t1, "intrinsics": intr.astype(f32), "ii": ii, "jj": jj, "kx": kx,
            "target": target.astype(f32), "weight": weight.astype(f32), "eta": eta.astype(f32),
            "poses_true": poses_true, "disps_true": disps_true, "behind": behind, "pushed": pushed,
            "poses": poses.astype(f32), "disps": disps.astype(f32),
            "prior_sigma": PRIOR_SIGMA if t0 == 0 else None}


def grid():
    """(name, keyword arguments) of every case the GPU comparisons and the tolerance figures run on."""
    out = []
    for (ht, wd) in SHAPES:
        for K in FRAMES:
            for prior in (False, True):
                for behind in (False, True):
                    name = f"{ht}x{wd}-K{K}-{'prior' if prior else 'fixed2'}-{'behind' if behind else 'plain'}"
                    out.append((name, dict(K=K, ht=ht, wd=wd, t0=0 if prior else 2, behind=behind, noise=0.05, damping=GRID_DAMPING)))
    return out


LARGE_P = ("5x7-K34-chain", dict(K=34, ht=5, wd=7, t0=1, chain=True, noise=0.05, damping=GRID_DAMPING))

_ORACLE = {}


def oracle(name, kw, dt=np.float64, itrs=2):
    """The oracle's run of a case, computed once per (case, precision) and shared."""
    key = (name, dt is np.float64, itrs)
    if key not in _ORACLE:
        c = make(**kw)
        _ORACLE[key] = (c, orc.ba(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"], c["target"], c["weight"],
                                  c["eta"], c["t0"], c["t1"], itrs=itrs, prior_sigma=c["prior_sigma"], dt=dt))
    return _ORACLE[key]
