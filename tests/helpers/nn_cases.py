"""Seeded inputs of tests/test_metrics3d_gpu.py: the smallest cases at which the ring search of csrc/nn.hip can go wrong,
the ICP scene and the two box meshes of the end-to-end test.  numpy only."""
import numpy as np

from helpers.nn_oracle import box_mesh, voxel_down_sample


def surface_cloud(rng, n, lower=(-1.0, -0.8, -0.5), upper=(1.0, 0.8, 0.5), jitter=0.004):
    """n float32 points on the six faces of a box, jittered: a surface with edges and corners."""
    lo, hi = np.asarray(lower), np.asarray(upper)
    p = rng.uniform(lo, hi, size=(n, 3))
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return (p + jitter * rng.normal(size=p.shape)).astype(np.float32)


def search_cases():
    """name -> dict(points, queries, cell_size, [max_distance], [transform])."""
    rng = np.random.default_rng(2024)
    target = surface_cloud(rng, 2500)
    queries = surface_cloud(rng, 1037, jitter=0.01)  # 1037: no multiple of a wave or a workgroup
    cases = {}
    for cs in (1 / 32, 1 / 8, 0.3):  # three cell sizes on the same data: identical output
        cases[f"surface_cell_{cs:.4f}"] = dict(points=target, queries=queries, cell_size=cs)
    cases["single_target"] = dict(points=target[:1], queries=queries[:130], cell_size=1 / 32)
    one_cell = (np.array([0.2, -0.1, 0.05]) + 0.01 * rng.random((40, 3))).astype(np.float32)
    cases["one_cell"] = dict(points=one_cell, queries=queries[:200], cell_size=1 / 16)
    planar = target[:700].copy()
    planar[:, 2] = np.float32(0.25)  # one axis has a single cell
    cases["planar"] = dict(points=planar, queries=queries[:300], cell_size=1 / 16)
    dup = np.concatenate([target[:300], target[100:250], target[:300][::-1]])  # every point two or three times
    # the first queries sit exactly on a target (distance 0), also on duplicated ones
    cases["duplicates_and_exact"] = dict(points=dup, queries=np.concatenate([dup[[5, 120, 310, 700]], queries[:200]]),
                                         cell_size=1 / 16)
    outside = np.array([[-1.5, 0, 0], [1.5, 0, 0], [0, -1.3, 0], [0, 1.3, 0], [0, 0, -0.9], [0, 0, 0.9], [-1.2, -1.0, -0.7],
                        [1.2, 1.0, 0.7], [100.0, 3.0, -2.0], [-1.00001, 0.80001, 0.1]], dtype=np.float32)
    cases["outside"] = dict(points=target, queries=np.concatenate([outside, queries[:54]]), cell_size=1 / 8)
    sparse = np.concatenate([0.02 * rng.random((30, 3)), 1.0 + 0.02 * rng.random((30, 3)),
                             np.array([0.0, 1.0, 0.5]) + 0.02 * rng.random((30, 3))]).astype(np.float32)
    # cells of 1/32 over a unit cube with three small clusters: queries in the void need up to ~16 rings
    cases["sparse_many_rings"] = dict(points=sparse, queries=rng.uniform(0.0, 1.0, (257, 3)).astype(np.float32), cell_size=1 / 32)
    near = (target[rng.integers(0, 2500, 600)] + rng.choice([0.008, 0.03], (600, 1)) * rng.normal(size=(600, 3))).astype(np.float32)
    cases["bounded"] = dict(points=target, queries=near, cell_size=1 / 32, max_distance=0.02)
    cases["bounded_coarse_cells"] = dict(points=target, queries=near, cell_size=1 / 4, max_distance=0.02)
    cases["transform"] = dict(points=target, queries=queries[:500], cell_size=1 / 16, transform=planted_motion())
    cases["transform_bounded"] = dict(points=target, queries=target[:500], cell_size=1 / 32, max_distance=0.02,
                                      transform=planted_motion())
    return cases


def planted_motion(angle_deg=1.0, translation=(0.003, -0.0025, 0.003)):
    """Rotation of about one degree about a skew axis and a translation of 5 mm, float64 [4, 4]."""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(angle_deg)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)
    m[:3, 3] = translation
    return m


def icp_scene():
    """(source, target) float32.  A box surface (edges and corners: no sliding direction) is sampled, jittered by 1 mm
    and voxel down-sampled at 1/32: about 1100 points.  The target holds these points and 2500 further samples of the
    surface, shuffled; the source is the down-sampled cloud with 0.3 mm of noise, moved by the INVERSE of
    planted_motion(), so that ICP has to recover planted_motion() up to that noise."""
    rng = np.random.default_rng(7)
    box = dict(lower=(-0.3, -0.2, -0.15), upper=(0.3, 0.2, 0.15), jitter=0.001)
    cloud = voxel_down_sample(surface_cloud(rng, 20000, **box), 1 / 32)
    target = np.concatenate([cloud.astype(np.float32), surface_cloud(rng, 2500, **box)])
    target = target[rng.permutation(target.shape[0])]
    inv = np.linalg.inv(planted_motion())
    source = (cloud + 3e-4 * rng.normal(size=cloud.shape)) @ inv[:3, :3].T + inv[:3, 3]
    return source.astype(np.float32), target


def room_meshes():
    """A room of 0.5 x 0.4 x 0.3 m and the same room with every face 1 cm further out, as (vertices, faces) pairs: at
    the metrics' voxel size of 1/64 their clouds have about 4000 points, which the brute-force helpers can follow."""
    lo, hi = np.array([-0.25, -0.2, -0.15]), np.array([0.25, 0.2, 0.15])
    return box_mesh(lo, hi), box_mesh(lo - 0.01, hi + 0.01)
