"""The HIP iso-surface extractor (csrc/iso.hip, meshing.extract_isosurface) against the numpy restatement of its rule
(tests/helpers/iso_oracle.py), BIT FOR BIT -- vertices and faces, their order included -- and NgpEngine.density_lattice
against density_at fed the same float32 positions."""
import numpy as np
import pytest
import torch

from helpers import iso_oracle as O

pytestmark = pytest.mark.gpu

LOWER, UPPER = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
ALL_CASES = O.CASES + [O.CRACK]


def _case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}" + (f"-{case[2]}" if case[2] else "")


def _same_bits(v, f, ref_v, ref_f, what):
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert v.shape == ref_v.shape and f.shape == ref_f.shape, f"{what}: {v.shape} {f.shape} != {ref_v.shape} {ref_f.shape}"
    assert np.array_equal(f, ref_f), f"{what}: faces differ"
    assert np.array_equal(v.view(np.uint32), ref_v.view(np.uint32)), f"{what}: vertices differ in their bits"


@pytest.mark.parametrize("case", ALL_CASES, ids=_case_id)
def test_kernel_matches_oracle_bit_for_bit(device, case):
    """every input of tests/test_iso_cpu.py, the crack case included, at three values of the points-per-workgroup launch
    parameter: the default, one wave, and one that divides neither the lattice nor the 256 threads of a workgroup"""
    from nerf_vo_amd.meshing import extract_isosurface

    values, valid, ref_v, ref_f = O.reference(case)
    assert (ref_v.shape[0], ref_f.shape[0]) == case[3:]
    vd = values.to(device)
    md = None if valid is None else valid.to(device)
    for ppw in (None, 64, 1000):
        v, f = extract_isosurface(vd, LOWER, UPPER, 0.0, valid=md, points_per_workgroup=ppw)
        _same_bits(v, f, ref_v, ref_f, f"{_case_id(case)} points_per_workgroup={ppw}")


def test_mask_that_deactivates_every_cube_and_fields_without_surface(device):
    from nerf_vo_amd.meshing import extract_isosurface

    values = O.field("sphere", (9, 8, 7)).to(device)
    valid = torch.ones(9, 8, 7, dtype=torch.bool, device=device)
    valid[1::2, :, :] = False  # every cube has a corner on an odd x plane
    for v, f in (extract_isosurface(values, LOWER, UPPER, 0.0, valid=valid),
                 extract_isosurface(torch.full((5, 4, 3), -1.0, device=device), LOWER, UPPER, 0.0)):
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64 and v.is_cuda


def test_nan_sample_gives_finite_vertices(device):
    from nerf_vo_amd.meshing import extract_isosurface

    shape = (9, 8, 7)
    values = O.field("sphere", shape).clone()
    values[4, 4, 3] = float("nan")   # deep inside the sphere: its edges are cut, t = NaN -> fmaxf(NaN, 0) = 0
    values[0, 0, 0] = float("nan")   # outside: a NaN is outside, nothing changes there
    assert bool(values[4, 3, 3] > 0)
    step = O.lattice_step(LOWER, UPPER, shape)
    ref_v, ref_f = O.extract(values.numpy(), np.asarray(LOWER, np.float32), step, 0.0)
    v, f = extract_isosurface(values.to(device), LOWER, UPPER, 0.0)
    assert bool(torch.isfinite(v).all()) and np.isfinite(ref_v).all() and v.shape[0] > 0
    _same_bits(v, f, ref_v, ref_f, "NaN sample")


def test_lattice_beyond_2_to_the_30_points(device):
    """1024 x 1024 x 1032 samples (1.08e9: byte offsets of the samples and of the per-point ranks pass 2^32, linear indices
    2^30) filled with -1, the sphere written into the highest 23 x 19 x 17 corner; against the oracle run on that block at
    its index offset.  The sphere's field is negative on the block's faces, so no edge leaves the block."""
    from nerf_vo_amd.meshing import extract_isosurface

    if torch.cuda.mem_get_info()[0] < 16e9:
        pytest.skip("less than 16 GB of device memory free")
    dims, block = (1024, 1024, 1032), (23, 19, 17)
    off = tuple(d - b for d, b in zip(dims, block))
    sphere = O.field("sphere", block)
    lower = np.asarray((-3.0, 0.5, -40.0), dtype=np.float32)
    upper = np.asarray((2.0, 9.25, 1.5), dtype=np.float32)
    step = (upper - lower) / np.asarray([d - 1 for d in dims], dtype=np.float32)
    ref_v, ref_f = O.extract(sphere.numpy(), lower, step, 0.0, index_offset=off)
    assert ref_v.shape[0] == 2600 and ref_f.shape[0] == 5196
    values = torch.full(dims, -1.0, device=device)
    values[off[0]:, off[1]:, off[2]:] = sphere.to(device)
    v, f = extract_isosurface(values, lower, upper, 0.0)
    del values
    _same_bits(v, f, ref_v, ref_f, "high corner of the large lattice")


def _engine(device):
    from nerf_vo_amd.ngp_engine import NgpConfig, NgpEngine

    eng = NgpEngine(NgpConfig(num_images=4, capacity=1 << 15, march_capacity=1 << 17), device)
    g = torch.Generator().manual_seed(9)
    flat = torch.zeros(eng.n_params)
    nd = eng.n_density_mlp
    flat[:nd] = (torch.rand(nd, generator=g) * 2 - 1) * 0.25
    n_grid = eng.density_net.n_params - nd
    flat[nd:nd + n_grid] = (torch.rand(n_grid, generator=g) * 2 - 1) * 0.8
    eng.set_params(flat)
    return eng


def test_density_lattice_matches_density_at(device):
    """33 x 29 x 31 samples over a box that sticks out of the scene box: the bits of density_at at lower + i * step
    (float32, the extractor's step), zeros outside the scene box, whatever the chunk size"""
    eng = _engine(device)
    lo_s, hi_s = eng.cfg.aabb
    res = (33, 29, 31)
    lower = np.asarray((lo_s - 0.4, 0.1, 0.2), dtype=np.float32)
    upper = np.asarray((0.9, hi_s + 0.3, 0.8), dtype=np.float32)
    step = (upper - lower) / np.asarray([r - 1 for r in res], dtype=np.float32)
    axes = [torch.from_numpy(lower[x] + np.arange(res[x], dtype=np.float32) * step[x]) for x in range(3)]
    assert all(a.dtype == torch.float32 for a in axes)
    pos = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).to(device)
    ref = eng.density_at(pos).view(*res)
    outside = ((pos < lo_s) | (pos > hi_s)).any(dim=1).view(*res)
    assert 0 < int(outside.sum()) < outside.numel()
    for chunk in (1 << 20, 4096):
        got = eng.density_lattice(lower, upper, res, chunk=chunk)
        assert got.shape == res and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"chunk {chunk}: density_lattice differs from density_at"
        assert bool((got[outside] == 0).all())
    with pytest.raises(ValueError, match="resolution"):
        eng.density_lattice(lower, upper, (1, 8, 8))
    with pytest.raises(ValueError, match="resolution"):
        eng.density_lattice(lower, upper, (2048, 1024, 1024))
