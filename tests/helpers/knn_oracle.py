"""Restatement of the k-nearest-neighbour contract of nerf-vo_amd/csrc/knn.hip by brute force, of its mean distance and of
the statistical outlier rule of pointcloud.remove_statistical_outlier.  numpy only; nothing here shares code with the
package."""
import numpy as np


def knn_brute(queries, points, k, chunk=256):
    """(dist2 float32 [N, k], index int64 [N, k]): d2 = (dx*dx + dy*dy) + dz*dz in float32, d = query - point, over all
    points; the k smallest pairs (d2, index) in lexicographic order; slots from M on hold inf / -1."""
    q = np.asarray(queries, dtype=np.float32)
    p = np.asarray(points, dtype=np.float32)
    n, m = q.shape[0], p.shape[0]
    c = min(k, m)
    dist2 = np.full((n, k), np.inf, np.float32)
    index = np.full((n, k), -1, np.int64)
    ids = np.arange(m)
    for lo in range(0, n, chunk):
        b = q[lo:lo + chunk]
        dx = b[:, None, 0] - p[None, :, 0]
        dy = b[:, None, 1] - p[None, :, 1]
        dz = b[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        for r in range(b.shape[0]):
            order = np.lexsort((ids, d2[r]))[:c]  # last key is the primary one: d2, then the index
            dist2[lo + r, :c] = d2[r, order]
            index[lo + r, :c] = order
    return dist2, index


def mean_distance(dist2, index):
    """float32 [N]: (((s_0 + s_1) + ...) + s_{c-1}) / float32(c), s_j = sqrt(d2_j) in float32, over the c filled slots of
    each row (index >= 0), left to right."""
    d2 = np.asarray(dist2, dtype=np.float32)
    filled = np.asarray(index) >= 0
    s = np.sqrt(d2, where=filled, out=np.zeros_like(d2))
    assert s.dtype == np.float32
    total = np.zeros(d2.shape[0], np.float32)
    for j in range(d2.shape[1]):
        total = np.where(filled[:, j], total + s[:, j], total).astype(np.float32)
    return (total / filled.sum(axis=1).astype(np.float32)).astype(np.float32)


def outlier_rule(avg, std_ratio):
    """(keep bool [N], threshold, mean, std) of the float32 mean distances ``avg``: a = avg as float64, V = {a > 0},
    mean = sum_V a / |V|, std = sqrt(sum_V (a - mean)^2 / (|V| - 1)), threshold = mean + std_ratio * std,
    keep = 0 < a < threshold.  Fewer than 2 points in V: ValueError."""
    a = np.asarray(avg).astype(np.float64)
    valid = a > 0
    nv = int(valid.sum())
    if nv < 2:
        raise ValueError("fewer than 2 points with a positive mean distance")
    mean = a[valid].sum() / nv
    std = np.sqrt(((a[valid] - mean) ** 2).sum() / (nv - 1))
    threshold = mean + std_ratio * std
    return valid & (a < threshold), float(threshold), float(mean), float(std)


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=10.0):
    """(kept index int64, avg float32 [N], threshold) by brute force."""
    d2, idx = knn_brute(points, points, nb_neighbors)
    avg = mean_distance(d2, idx)
    keep, threshold, _, _ = outlier_rule(avg, std_ratio)
    return np.nonzero(keep)[0], avg, threshold


def outlier_scene():
    """The cloud of the outlier-removal test: 3000 jittered points on a box surface and 12 planted points at radius
    0.6 .. 0.9 in random directions, shuffled -> (points float32 [3012, 3], planted bool [3012])."""
    from helpers.nn_cases import surface_cloud

    rng = np.random.default_rng(11)
    surface = surface_cloud(rng, 3000, lower=(-0.3, -0.2, -0.15), upper=(0.3, 0.2, 0.15), jitter=0.001)
    direction = rng.normal(size=(12, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    far = (direction * rng.uniform(0.6, 0.9, (12, 1))).astype(np.float32)
    pts = np.concatenate([surface, far])
    planted = np.concatenate([np.zeros(3000, bool), np.ones(12, bool)])
    perm = rng.permutation(pts.shape[0])
    return pts[perm], planted[perm]
