"""Dense-lattice Poisson reconstruction without a GPU: the lattice arithmetic, the float32 oracle against the float64 oracle
(the margins of profiles/poisson_parity_margins.json), the multigrid's convergence, the geometry of the oracle's meshes on
the sphere and the rooms (which fixes the bounds of tests/test_poisson_gpu.py), the trim rule and every refusal."""
import math

import numpy as np
import pytest
import torch

from helpers import poisson_cases as cases
from helpers import poisson_oracle as O

MARGIN = 2.5  # the project's usual margin over a recorded float32-vs-float64 difference


def _padding_and_cells(lat, lower, upper):
    h, origin, cells = lat["h"], np.asarray(lat["origin"], np.float64), np.asarray(lat["cells"])
    below = (np.asarray(lower) - origin) / h
    above = (origin + cells * h - np.asarray(upper)) / h
    return below, above


@pytest.mark.parametrize("lower,upper,depth", [
    ((0.0, 0.0, 0.0), (1.0, 0.8, 0.7), 9),            # the example of the issue: L = 7, 513 x 385 x 385
    ((-1.0, 2.0, 0.5), (3.0, 2.001, 1.5), 7),         # one thin axis
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2),
    ((-0.3, -0.2, -0.1), (0.7, 0.9, 0.6), 10),
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 5),
])
def test_lattice_arithmetic(lower, upper, depth):
    from nerf_vo_amd.poisson import bin_points, poisson_lattice

    lat = poisson_lattice(lower, upper, depth)
    ref = O.lattice(lower, upper, depth)
    assert {k: lat[k] for k in ref} == ref, "the package and the oracle state the same lattice"
    L, cells = lat["levels"], lat["cells"]
    assert 1 <= L <= depth and all(c % (1 << L) == 0 for c in cells) and 2 <= (min(cells) >> L) <= 3
    assert lat["nodes"] == tuple(c + 1 for c in cells)
    below, above = _padding_and_cells(lat, lower, upper)
    assert (below >= 2 - 1e-3).all() and (above >= 2 - 1e-3).all(), "two cells of padding on every side"
    if depth == 9:
        assert L == 7 and lat["nodes"] == (513, 385, 385)
    if depth == 2:
        assert L == 2 and lat["nodes"] == (9, 9, 9)
    # every point of the box, its corners included, falls into an interior cell (not one that touches the boundary)
    rng = np.random.default_rng(0)
    p = rng.uniform(lower, upper, size=(2000, 3))
    p[:8] = [[(lower, upper)[(m >> a) & 1][a] for a in range(3)] for m in range(8)]
    pts = torch.from_numpy(p.astype(np.float32)).clamp(torch.tensor(lower).float(), torch.tensor(upper).float())
    c, _ = O.locate(pts.numpy(), lat, np.float32)
    assert (c >= 1).all() and (c <= np.asarray(cells) - 2).all()
    if lat["nodes"][0] * lat["nodes"][1] * lat["nodes"][2] < 2 ** 24:
        order, start = bin_points(pts, lat)
        ref_order, ref_start = O.bin_points(pts.numpy(), lat)
        assert np.array_equal(order.numpy(), ref_order) and np.array_equal(start.numpy(), ref_start)


@pytest.mark.parametrize("case", cases.OPERATOR_CASES, ids=cases.case_id)
def test_float32_oracle_against_float64_oracle(case):
    recorded = cases.load_margins()["parity"][cases.case_id(case)]
    got = cases.parity_of_case(case)
    print(f"{cases.case_id(case)}: chi relative {got['chi_relative']:.3e} (recorded {recorded['chi_relative']:.3e}), vertices "
          f"{got['vertex_voxels']:.3e} voxel (recorded {recorded['vertex_voxels']:.3e}), edges cut by one field only "
          f"{got['edges_cut_by_one_only']}")
    assert got["chi_relative"] <= MARGIN * recorded["chi_relative"]
    assert got["vertex_voxels"] <= MARGIN * recorded["vertex_voxels"]
    # float32 itself: chi of these sizes is a few thousand sums and products away from its inputs
    assert recorded["chi_relative"] <= 1e-4 and recorded["vertex_voxels"] <= 1e-2
    assert got["edges_cut_by_one_only"] <= recorded["edges_cut_by_one_only"] + 2


@pytest.mark.parametrize("name", list(cases.CONVERGENCE_CASES))
def test_multigrid_convergence_in_float64(name):
    recorded = cases.load_margins()["convergence"][name]
    nodes, factor, total = cases.convergence(name)
    print(f"{name}: worst residual factor of a V(2,2) cycle {factor:.4f} (recorded {recorded['worst_factor_per_cycle']:.4f}), "
          f"after 8 cycles {total:.2e} of the start")
    assert "x".join(map(str, nodes)) == name
    assert recorded["worst_factor_per_cycle"] < 0.2, "a V(2,2) cycle that does not reach 0.2 is a wrong multigrid"
    assert factor <= 1.5 * recorded["worst_factor_per_cycle"] and factor < 0.2
    assert total <= 1e-7


CAPS = {"sphere": 0.5, "room_closed": 1.0, "room_five_faces": 1.0}  # voxels, whatever was measured


@pytest.mark.parametrize("name", cases.SCENES)
def test_geometry_of_the_oracle_mesh(name):
    recorded = cases.load_margins()["geometry"][name]
    m = cases.scene_oracle_mesh(name)
    print(f"{name}: lattice {m['lattice']['nodes']}, {m['vertices'].shape[0]} vertices, {m['kept_share']:.1%} kept at density >= "
          f"{m['threshold']:.3f}; worst kept vertex {m['worst_kept']:.4f} voxel (cap {CAPS[name]}), with min_density = 0 "
          f"{m['worst_without_floor']:.3f}; zero-density share {m['zero_density_share']:.3f}")
    assert m["worst_kept"] <= CAPS[name]
    assert list(m["lattice"]["nodes"]) == recorded["nodes"]
    # the file holds what this oracle gives: the GPU tests' bound is 2 x this figure
    assert math.isclose(m["worst_kept"], recorded["oracle_worst_kept_voxels"], rel_tol=1e-3)
    assert math.isclose(recorded["geometry_bound_voxels"], 2.0 * recorded["oracle_worst_kept_voxels"], rel_tol=1e-12)
    if name == "room_five_faces":
        # the quantile alone trims nothing (more than 10 % of the vertices have density 0) and leaves sheets far from any wall
        assert m["zero_density_share"] > 0.1 and m["worst_without_floor"] > 5.0
        assert m["threshold"] == 1.0


def test_trim_rule_against_numpy_quantile():
    from nerf_vo_amd.poisson import density_quantile, trim_by_density

    rng = np.random.default_rng(4)
    faces = torch.from_numpy(rng.integers(0, 400, size=(900, 3)))
    vertices = torch.from_numpy(rng.normal(size=(400, 3)).astype(np.float32))
    colors = torch.from_numpy(rng.integers(0, 256, size=(400, 3)).astype(np.uint8))
    ties = np.repeat(np.array([0.0, 0.5, 2.0, 2.0, 7.25], np.float32), 80)
    densities = {"ties": rng.permutation(ties), "all_equal": np.full(400, 3.5, np.float32),
                 "random": rng.gamma(2.0, 3.0, 400).astype(np.float32), "zeros": np.where(rng.random(400) < 0.3, 0, 5).astype(np.float32)}
    for label, d in densities.items():
        for q, floor in ((0.1, 1.0), (0.1, 0.0), (0.37, 0.0), (0.9, 1.0), (0.0, 0.0), (1.0, 0.0)):
            assert density_quantile(torch.from_numpy(d), q) == float(np.quantile(d.astype(np.float64), q)), (label, q)
            keep_ref, faces_ref, thr_ref = O.trim(d, faces.numpy(), q, floor)
            v, f, c, thr, keep = trim_by_density(vertices, faces, torch.from_numpy(d), colors, q, floor)
            assert thr == thr_ref and np.array_equal(keep.numpy(), keep_ref), (label, q, floor)
            assert np.array_equal(f.numpy(), faces_ref) and torch.equal(v, vertices[keep]) and torch.equal(c, colors[keep])
            assert f.numel() == 0 or int(f.max()) < v.shape[0]
    # a quantile above the floor decides, a floor above the quantile decides
    d = densities["random"]
    assert trim_by_density(vertices, faces, torch.from_numpy(d), None, 0.9, 1.0)[3] == float(np.quantile(d.astype(np.float64), 0.9)) > 1.0
    assert trim_by_density(vertices, faces, torch.from_numpy(d), None, 0.0, 1.0)[3] == 1.0
    # all-equal densities: nothing is below the quantile, nothing is dropped
    assert trim_by_density(vertices, faces, torch.from_numpy(densities["all_equal"]), None, 0.1, 1.0)[0].shape[0] == 400


def test_refusals_say_what_to_change(monkeypatch):
    from nerf_vo_amd import poisson as P

    for depth in (1, 11, 2.5):
        with pytest.raises(ValueError, match="depth .* between 2 and 10"):
            P.poisson_lattice((0, 0, 0), (1, 1, 1), depth)
    with pytest.raises(ValueError, match="not finite"):
        P.poisson_lattice((0, 0, 0), (1, float("inf"), 1), 5)
    with pytest.raises(ValueError, match="upper >= lower"):
        P.poisson_lattice((0, 0, 0), (1, -1, 1), 5)
    with pytest.raises(ValueError, match="scale"):
        P.poisson_lattice((0, 0, 0), (1, 1, 1), 5, scale=0.0)
    # a lattice of 2^31 nodes or more: depth 10 at a scale that makes the cells small
    with pytest.raises(ValueError, match="lower the depth"):
        P.poisson_lattice((0, 0, 0), (1, 1, 1), 10, scale=0.5)
    points = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.poisson_reconstruct(points, points)
    # the argument checks come before any kernel: run them with the GPU check switched off
    monkeypatch.setattr(P, "_need_gpu", lambda t, what: None)
    normals = torch.nn.functional.normalize(torch.randn(10, 3), dim=1)
    with pytest.raises(ValueError, match=r"\[K >= 1, 3\]"):
        P.poisson_reconstruct(points, normals[:5])
    bad = points.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or infinite .* remove those points"):
        P.poisson_reconstruct(bad, normals)
    with pytest.raises(ValueError, match="NaN or infinite"):
        P.poisson_reconstruct(points, normals * float("inf"))
    with pytest.raises(ValueError, match="3 of 10 points lie outside the box .* crop the cloud"):
        far = points.clone()
        far[:3, 0] = 1.5
        P.poisson_reconstruct(far, normals, lower=(0, 0, 0), upper=(1, 1, 1))
    with pytest.raises(ValueError, match="both lower and upper"):
        P.poisson_reconstruct(points, normals, lower=(0, 0, 0))
    with pytest.raises(ValueError, match="depth .* between 2 and 10"):
        P.poisson_reconstruct(points, normals, depth=12)
    with pytest.raises(ValueError, match="uint8"):
        P.poisson_reconstruct(points, normals, colors=torch.rand(10, 3))
    with pytest.raises(ValueError, match="cycles"):
        P.poisson_reconstruct(points, normals, cycles=0)
    with pytest.raises(ValueError, match="trim_quantile"):
        P.density_quantile(torch.rand(5), 1.5)


def test_protocol_defaults_follow_the_training_pixels():
    """tools/eval_protocol.py: the reference's 33 554 432 points at depth 9 where the frames can carry them, otherwise at most
    a quarter of the training pixels and a depth at which a surface cell holds about four points."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("_eval_protocol", os.path.join(cases.ROOT, "tools", "eval_protocol.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool._mesh_nerf_defaults(None, None, 200 * 680 * 1200) == (33554432, 9)
    assert tool._mesh_nerf_defaults(None, None, 48 * 120 * 160) == (230400, 6)
    assert tool._mesh_nerf_defaults(4000000, None, 1) == (4000000, 8)
    assert tool._mesh_nerf_defaults(None, 7, 10 ** 6) == (250000, 7)
    assert tool._mesh_nerf_defaults(100, None, 10 ** 6) == (100, 2)
