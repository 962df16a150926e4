"""Restatements of nerf_vo_amd/pointcloud.py for the tests: the nearest-neighbour contract of csrc/nn.hip by brute
force in numpy float32 (same operation order, smallest index on ties), and voxel down-sampling, point-to-point ICP and the
3-D metrics pipeline in float64.  Nothing here shares code with the package."""
import numpy as np

THRESHOLD = 0.05


def transform_f32(queries, xf):
    """x' = ((r0*x + r1*y) + r2*z) + t per row, every operation rounded to float32."""
    q = np.asarray(queries, dtype=np.float32)
    m = np.asarray(xf, dtype=np.float64)[:3, :4].astype(np.float32)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)


def nn_brute(queries, points, max_distance=None, transform=None, chunk=512):
    """(dist2 float32 [N], index int64 [N]): min over all points of (dx*dx + dy*dy) + dz*dz in float32, d = query - point;
    the smallest index attaining it; bounded: only dist2 <= float32(max_distance)^2 counts, else inf / -1."""
    q = np.asarray(queries, dtype=np.float32)
    p = np.asarray(points, dtype=np.float32)
    if transform is not None:
        q = transform_f32(q, transform)
    dist2 = np.empty(q.shape[0], np.float32)
    index = np.empty(q.shape[0], np.int64)
    for lo in range(0, q.shape[0], chunk):
        c = q[lo:lo + chunk]
        dx = c[:, None, 0] - p[None, :, 0]
        dy = c[:, None, 1] - p[None, :, 1]
        dz = c[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        index[lo:lo + chunk] = np.argmin(d2, axis=1)  # first occurrence = smallest index
        dist2[lo:lo + chunk] = d2[np.arange(c.shape[0]), index[lo:lo + chunk]]
    if max_distance is not None:
        m = np.float32(max_distance)
        miss = ~(dist2 <= m * m)
        dist2[miss] = np.inf
        index[miss] = -1
    return dist2, index


def nn_brute_f64(queries, points, chunk=512):
    """float64 distances (not squared) and indices."""
    q = np.asarray(queries, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    dist = np.empty(q.shape[0])
    index = np.empty(q.shape[0], np.int64)
    for lo in range(0, q.shape[0], chunk):
        c = q[lo:lo + chunk]
        d2 = (c[:, None, 0] - p[None, :, 0]) ** 2
        d2 += (c[:, None, 1] - p[None, :, 1]) ** 2
        d2 += (c[:, None, 2] - p[None, :, 2]) ** 2
        index[lo:lo + chunk] = np.argmin(d2, axis=1)
        dist[lo:lo + chunk] = np.sqrt(d2[np.arange(d2.shape[0]), index[lo:lo + chunk]])
    return dist, index


def voxel_down_sample(points, voxel_size):
    """float64 mean per occupied voxel of floor(p / voxel_size), ascending (x, y, z) voxel order."""
    p = np.asarray(points, dtype=np.float64)
    cell = np.floor(p / voxel_size).astype(np.int64)
    uniq, inverse = np.unique(cell, axis=0, return_inverse=True)  # rows sorted lexicographically
    inverse = inverse.reshape(-1)
    out = np.zeros((uniq.shape[0], 3))
    np.add.at(out, inverse, p)
    return out / np.bincount(inverse, minlength=uniq.shape[0])[:, None]


def kabsch(src, dst):
    cs, cd = src.mean(0), dst.mean(0)
    u, _, vt = np.linalg.svd((src - cs).T @ (dst - cd))
    d = np.sign(np.linalg.det(vt.T @ u.T))
    r = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    out = np.eye(4)
    out[:3, :3] = r
    out[:3, 3] = cd - r @ cs
    return out


def icp(source, target, max_correspondence_distance=0.02, max_iteration=30, relative_fitness=1e-7, relative_rmse=1e-7,
        fp32_distance_rule=False):
    """Point-to-point ICP in float64 -> (T [4, 4], fitness, inlier_rmse, iterations).  ``fp32_distance_rule``: the
    correspondences come from the float32 contract (nn_brute with the transform applied in float32) instead of float64
    distances -- what the kernel-backed ICP sees; everything else stays float64."""
    src = np.asarray(source, dtype=np.float64)
    tgt = np.asarray(target, dtype=np.float64)
    T = np.eye(4)
    prev, fitness, rmse, iterations = None, 0.0, 0.0, 0
    for it in range(max_iteration):
        iterations = it + 1
        moved = src @ T[:3, :3].T + T[:3, 3]
        if fp32_distance_rule:
            d2, idx = nn_brute(np.asarray(source, np.float32), np.asarray(target, np.float32), max_correspondence_distance, T)
            hit = idx >= 0
            d2 = d2.astype(np.float64)
        else:
            dist, idx = nn_brute_f64(moved, tgt)
            hit = dist <= max_correspondence_distance
            d2 = dist ** 2
        k = int(hit.sum())
        if k == 0:
            fitness, rmse = 0.0, 0.0
            break
        fitness, rmse = k / src.shape[0], float(np.sqrt(d2[hit].sum() / k))
        T = kabsch(moved[hit], tgt[idx[hit]]) @ T
        if prev is not None and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            break
        prev = (fitness, rmse)
    return T, fitness, rmse, iterations


def metrics_tail(d_gt_to_pred, d_pred_to_gt):
    a, b = np.asarray(d_gt_to_pred, np.float64), np.asarray(d_pred_to_gt, np.float64)
    precision, recall = float((a < THRESHOLD).mean()), float((b < THRESHOLD).mean())
    return {"accuracy": float(a.mean()), "completion": float(b.mean()), "precision": precision, "recall": recall,
            "f1score": 2 * precision * recall / (precision + recall)}


def metrics_from_clouds(points_gt, points_pred, fp32_distance_rule=False):
    """ICP of pred onto gt, then nearest-neighbour distances both ways and the five metrics, in float64."""
    T, _, _, _ = icp(points_pred, points_gt, fp32_distance_rule=fp32_distance_rule)
    moved = (np.asarray(points_pred, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    gt = np.asarray(points_gt, np.float32)
    if fp32_distance_rule:
        d_gt_to_pred = np.sqrt(nn_brute(moved, gt)[0].astype(np.float64))
        d_pred_to_gt = np.sqrt(nn_brute(gt, moved)[0].astype(np.float64))
    else:
        d_gt_to_pred, d_pred_to_gt = nn_brute_f64(moved, gt)[0], nn_brute_f64(gt, moved)[0]
    return metrics_tail(d_gt_to_pred, d_pred_to_gt)


def box_mesh(lower, upper):
    """(vertices float32 [8, 3], faces int64 [12, 3]) of an axis-aligned box."""
    lo, hi = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], dtype=np.float32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], dtype=np.int64)
    return v, f
