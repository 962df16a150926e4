"""CPU side of the mesh-from-frames path (nerf_vo_amd/tsdf.py, meshing.py): the validity mask of the iso-surface
extractor, colours / normals in the mesh files, the frustum bounds, the volume's size check and the extraction from a
volume filled by hand.  The fusion kernel itself is tested on the GPU (test_tsdf_gpu.py)."""
import numpy as np
import pytest
import torch

from test_meshing_cpu import _sphere


def _edge_counts(f):
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).sort(dim=1).values
    return torch.unique(e, dim=0, return_counts=True)


def test_mask_on_a_masked_sphere():
    from nerf_vo_amd.meshing import marching_tetrahedra

    n = 40
    values = _sphere(n)
    box = ([-1, -1, -1], [1, 1, 1])
    v0, f0 = marching_tetrahedra(values, *box, 0.0, slab=7)
    for valid in (None, torch.ones(n, n, n, dtype=torch.bool)):
        v, f = marching_tetrahedra(values, *box, 0.0, slab=7, valid=valid)
        assert torch.equal(v, v0) and torch.equal(f, f0)

    cut = 22  # samples with x index >= cut are invalid
    valid = torch.ones(n, n, n, dtype=torch.bool)
    valid[cut:] = False
    v, f = marching_tetrahedra(values, *box, 0.0, slab=7, valid=valid)
    assert 100 < f.shape[0] < f0.shape[0]
    step = 2.0 / (n - 1)
    gx = (v[:, 0] + 1.0) / step  # grid coordinate along x
    # a cube with an invalid corner spans x indices [cut - 1, cut] or beyond: no vertex lies past index cut - 1
    assert float(gx[f].max()) <= cut - 1 + 1e-4
    # open edges (used by one triangle) exist only where the mask cut the surface: on the plane x = cut - 1
    u, c = _edge_counts(f)
    assert int(c.max()) == 2
    border = u[c == 1]
    assert border.shape[0] > 0
    assert bool(((gx[border] - (cut - 1)).abs() < 1e-4).all())


def test_write_mesh_round_trips_colors_and_normals(tmp_path):
    from nerf_vo_amd.meshing import marching_tetrahedra, write_mesh

    v, f = marching_tetrahedra(_sphere(20), [-1, -1, -1], [1, 1, 1], 0.0)
    g = torch.Generator().manual_seed(3)
    colors = torch.randint(0, 256, (v.shape[0], 3), generator=g).to(torch.uint8)
    normals = torch.nn.functional.normalize(v, dim=1)
    write_mesh(str(tmp_path / "plain.ply"), v, f)
    write_mesh(str(tmp_path / "full.ply"), v, f, colors=colors, normals=normals)
    write_mesh(str(tmp_path / "plain.obj"), v, f)
    write_mesh(str(tmp_path / "full.obj"), v, f, normals=normals)
    head, body = open(tmp_path / "full.ply", "rb").read().split(b"end_header\n", 1)
    props = [l.split()[-1] for l in head.decode().splitlines() if l.startswith("property") and "list" not in l]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert b"property float nx" in head and b"property uchar red" in head
    assert len(body) == v.shape[0] * 27 + f.shape[0] * 13
    rec = np.frombuffer(body[: v.shape[0] * 27], dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    assert np.array_equal(rec["p"], v.numpy()) and np.array_equal(rec["n"], normals.numpy())
    assert np.array_equal(rec["c"], colors.numpy())
    faces = np.frombuffer(body[v.shape[0] * 27:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert (faces["n"] == 3).all() and np.array_equal(faces["i"], f.numpy())
    # without the extras the file is what it was: positions only
    head, body = open(tmp_path / "plain.ply", "rb").read().split(b"end_header\n", 1)
    assert b"nx" not in head and b"red" not in head and len(body) == v.shape[0] * 12 + f.shape[0] * 13
    plain, full = open(tmp_path / "plain.obj").read().splitlines(), open(tmp_path / "full.obj").read().splitlines()
    assert [l for l in full if not l.startswith("vn ")] == plain
    vn = np.array([[float(x) for x in l.split()[1:]] for l in full if l.startswith("vn ")])
    assert vn.shape == (v.shape[0], 3) and np.allclose(vn, normals.numpy(), atol=1e-6)


def test_frustum_bounds_against_numpy():
    from nerf_vo_amd.tsdf import frustum_bounds

    H, W = 5, 7
    fx, fy, cx, cy = 6.0, 5.0, 3.0, 2.0
    rng = np.random.default_rng(0)
    depths = rng.uniform(0.5, 3.0, size=(2, H, W)).astype(np.float32)
    depths[0, 0, 0] = 0.0        # invalid: not positive
    depths[0, 4, 6] = 7.0        # invalid: beyond depth_max (it would set the upper bound)
    depths[1, 2, 3] = np.nan     # invalid
    depths[1, 1, 1] = 4.0        # valid: exactly depth_max
    a = 0.6
    c2w = np.tile(np.eye(4), (2, 1, 1))
    c2w[1, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    c2w[1, :3, 3] = [0.3, -0.1, 0.2]
    pts = []
    for n in range(2):
        for v in range(H):
            for u in range(W):
                d = float(depths[n, v, u])
                if d > 0 and d <= 4.0:
                    pts.append(c2w[n, :3, :3] @ np.array([(u - cx) / fx * d, (v - cy) / fy * d, d]) + c2w[n, :3, 3])
    pts = np.array(pts)
    assert pts.shape[0] == 2 * H * W - 3
    lower, upper = frustum_bounds(torch.from_numpy(depths), c2w, (fx, fy, cx, cy), 4.0)
    np.testing.assert_allclose(lower.numpy(), pts.min(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(upper.numpy(), pts.max(axis=0), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        frustum_bounds(torch.zeros(1, H, W), c2w[:1], (fx, fy, cx, cy), 4.0)


def test_volume_size_check():
    from nerf_vo_amd.tsdf import TSDFVolume

    with pytest.raises(ValueError, match="max_voxels"):
        TSDFVolume([0, 0, 0], [1, 1, 1], voxel_size=1 / 64, device="cpu", max_voxels=64 ** 3)  # 65^3 samples
    with pytest.raises(ValueError, match="max_voxels"):
        TSDFVolume([-40, -40, -40], [40, 40, 40], device="cpu")  # the default cap, before anything is allocated
    vol = TSDFVolume([0, 0, 0], [1, 0.5, 0.25], voxel_size=1 / 16, device="cpu", max_voxels=17 * 9 * 5)
    assert vol.dims == (17, 9, 5) and vol.tsdf.shape == (17, 9, 5) and vol.color.shape == (3, 17, 9, 5)
    assert float(vol.tsdf.abs().sum() + vol.weight.abs().sum() + vol.color.abs().sum()) == 0.0
    np.testing.assert_allclose(vol.upper_of_grid, [1, 0.5, 0.25])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(torch.ones(1, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.eye(4)[None], (4.0, 4.0, 2.0, 2.0))


def test_extraction_from_a_hand_filled_volume():
    """A plane's TSDF written into the tensors on the CPU, weight 3 on one half of the box and 2 on the other."""
    from nerf_vo_amd.tsdf import TSDFVolume

    vs = 1 / 16
    vol = TSDFVolume([-1, -1, -1], [1, 1, 1], voxel_size=vs, trunc_voxels=4.0, device="cpu")
    n = vol.dims[0]
    assert vol.dims == (33, 33, 33)
    ax = torch.arange(n, dtype=torch.float32) * vs - 1.0
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    normal = torch.nn.functional.normalize(torch.tensor([0.3, -0.2, 1.0]), dim=0)
    offset = 0.11
    sdf = X * normal[0] + Y * normal[1] + Z * normal[2] - offset  # positive on the side the normal points to
    vol.tsdf.copy_((sdf / vol.trunc).clamp(-1, 1))
    half = 16  # x index: samples below it carry weight 3, the others 2
    vol.weight.fill_(2.0)
    vol.weight[:half] = 3.0
    rgb = torch.tensor([200.0, 100.0, 50.0])
    vol.color.copy_(rgb[:, None, None, None].expand_as(vol.color))
    v, f, c, nrm = vol.extract_mesh(weight_threshold=3.0)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and c.dtype == torch.uint8 and nrm.dtype == torch.float32
    assert f.shape[0] > 500 and c.shape == v.shape == nrm.shape
    # only the weight-3 half: cubes need all eight corners valid, so x stops at sample half - 1
    assert float(v[:, 0].max()) <= ax[half - 1] + 1e-6 and float(v[:, 0].min()) == pytest.approx(-1.0, abs=1e-6)
    # the field is linear inside the truncation band, so linear cuts are exact
    assert float(((v * normal).sum(dim=1) - offset).abs().max()) <= 1e-6
    assert float((nrm * normal).sum(dim=1).min()) > 0.999
    assert bool((c == rgb.to(torch.uint8)).all())
    # threshold 2 takes the whole box
    v2, _, _, _ = vol.extract_mesh(weight_threshold=2.0)
    assert float(v2[:, 0].max()) == pytest.approx(1.0, abs=1e-6)


def test_launcher_rejects_bad_arguments():
    """nvo_tsdf_integrate validates before it launches anything (no GPU is touched: every call here is refused)."""
    import ctypes as C

    from nerf_vo_amd import _lib

    lib = _lib.lib()
    good = dict(tsdf=64, weight=64, color=64, frames=64, depth=64, rgb=64, nx=8, ny=8, nz=8, K=1, H=4, W=4,
                lower_x=0.0, lower_y=0.0, lower_z=0.0, voxel_size=1 / 64, trunc=8 / 64, depth_max=5.0)
    bad = [dict(nx=2048, ny=1024, nz=1024), dict(nx=1 << 31, ny=1, nz=1), dict(nx=0), dict(tsdf=None), dict(weight=None),
           dict(color=None), dict(frames=None), dict(depth=None), dict(rgb=None), dict(K=0), dict(K=_lib.TSDF_MAX_FRAMES + 1),
           dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(trunc=0.0), dict(trunc=-0.1),
           dict(H=0), dict(W=0)]
    for change in bad:
        args = _lib.TsdfArgs(**{**good, **change})
        assert lib.nvo_tsdf_integrate(None, C.byref(args)) == 1, change  # NVO_ERR_INVALID
        assert b"tsdf_integrate" in lib.nvo_last_error()
    assert lib.nvo_tsdf_integrate(None, None) == 1
