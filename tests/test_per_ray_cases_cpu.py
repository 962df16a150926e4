"""tests/golden/per_ray_bits.json against tests/helpers/per_ray_cases.py, without a GPU: the input builders still give
the recorded inputs (a drifted builder would otherwise show up on the GPU as a kernel that changed), and the record
holds exactly the entries tests/test_per_ray_forms_gpu.py looks up (a stale record)."""
import pytest

from helpers import per_ray_cases as prc


@pytest.fixture(scope="module")
def record():
    return prc.load_record()


@pytest.mark.parametrize("family", list(prc.CASES))
def test_inputs_are_the_recorded_ones(record, family):
    for index, case in enumerate(prc.CASES[family]):
        for R in prc.RS:
            key = prc.record_key(family, index, R)
            assert key in record["cases"], f"{key}: not in the record"
            assert prc.inputs_digest(prc.inputs(family, case, R)) == record["cases"][key]["inputs"], (
                f"{family} case {index} R={R}: the input builders no longer give the recorded inputs")


def test_record_has_exactly_the_looked_up_entries(record):
    want = {(prc.record_key(family, index, R), name) for family, cases in prc.CASES.items()
            for index in range(len(cases)) for R in prc.RS for name in prc.OUTPUTS[family]}
    have = {(key, name) for key, entry in record["cases"].items() for name in entry["outputs"]}
    assert have == want, f"missing {sorted(want - have)[:5]}, stale {sorted(have - want)[:5]}"
    for key, entry in record["cases"].items():
        for value in (entry["inputs"], *entry["outputs"].values()):
            assert len(value) == 64 and int(value, 16) >= 0, key
    assert set(record["header"]) == {"commit", "rocm", "torch", "device"} and all(record["header"].values())
