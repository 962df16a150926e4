"""The TSDF fusion kernels (csrc/tsdf.hip, tsdf_blocks.hip; the per-voxel rule of csrc/tsdf_dev.h) and the edge-owned
extractors (csrc/iso.hip, iso_blocks.hip; the per-point rules of csrc/iso_dev.h) against the recorded bits of
tests/golden/tsdf_bits.json: the cases of tests/helpers/tsdf_bits_cases.py run once, and the sha256 of every output
tensor (dtype, shape, bytes) must be the recorded one.  The frames are read from tests/golden/tsdf_bits_inputs.npz (the
room scene as rendered where the record was made: its last bits depend on the CPU).  The record was made with the
kernels that each held a copy of their own of these rules; it is re-made only by a change that means to alter the rules'
bits and says so (tests/golden/make_golden_tsdf_bits.py).

Why equality is exact: a voxel is owned by one thread that applies the frames in table order in fp32 as written
(-ffp-contract=off), so fusion has no order between threads to depend on; vertices are owned by lattice edges and placed
by prefix sums; vertex normals are summed in face order in float64.  Nothing here uses an atomic on a float.

The dense box 72 x 67 x 53 has no dimension that is a multiple of the 2 x 4 x 32 brick (predicated partial bricks); the
launch of 16 frames is the only one in the suite with more than eight frames, the brick cull's second batch."""
import pytest
import torch

from helpers import tsdf_bits_cases as tbc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    return tbc.load_record()


@pytest.fixture(scope="module")
def outputs(device, record):
    inp = tbc.inputs()
    assert tbc.inputs_digest(inp) == record["inputs"], f"{tbc.INPUTS_PATH} is not the file the record was made with"
    # the recorded frames are room_scene()'s up to the CPU's rounding: depths of at most 2 m through a dozen float32
    # operations (2^-23 relative each), poses through a float64 inverse rounded once
    scene = tbc.scene_inputs()
    assert torch.equal(inp["intr"], scene["intr"]) and inp["rgb"].shape == scene["rgb"].shape
    assert float((inp["depth"] - scene["depth"]).abs().max()) <= 1e-5
    assert float((inp["w2c"] - scene["w2c"]).abs().max()) <= 1e-6 and float((inp["c2w"] - scene["c2w"]).abs().max()) <= 1e-6
    return tbc.run(inp, device)


@pytest.mark.parametrize("case", tbc.CASES)
def test_recorded_bits(outputs, record, case):
    assert case in record["cases"], f"{case}: not in {tbc.RECORD_PATH}"
    assert set(outputs[case]) == set(record["cases"][case])
    for name, t in outputs[case].items():
        assert t.numel() > 0, f"{case}: {name} is empty"
        assert tbc.digest(t) == record["cases"][case][name], f"{case}: {name} differs from the recorded bits"


def test_sixteen_frames_are_the_eight_fused_twice(outputs):
    """every voxel the eight frames observe is observed twice by the sixteen, and no other"""
    w8, w16 = outputs["dense/8"]["weight"], outputs["dense/16"]["weight"]
    assert float(w8.max()) >= 3.0 and bool((w16 == 2.0 * w8).all())


def test_extractor_does_not_depend_on_points_per_workgroup(outputs, record):
    a, b = outputs["iso/default"], outputs["iso/1000"]
    assert a["vertices"].shape[0] > 1000 and a["faces"].shape[0] > 1000
    for name in ("vertices", "faces"):
        assert tbc.digest(a[name]) == tbc.digest(b[name])
        assert record["cases"]["iso/default"][name] == record["cases"]["iso/1000"][name]
