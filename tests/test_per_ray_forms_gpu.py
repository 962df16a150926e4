"""The per-ray kernels of csrc/render.hip (k_weights_pdf, k_main_render_loss, k_prop_loss) against the recorded bits of
tests/golden/per_ray_bits.json: each exported launcher once on the seeded inputs of tests/helpers/per_ray_cases.py into
freshly zeroed outputs, and the sha256 of every output buffer's bytes must be the recorded one.  The record was made
with the kernels' previous forms (loads where the value is used) and, byte for byte the same file, with the shipped
ones (EXPERIMENTS.md 12.4); it is re-made only by a change that means to alter these kernels' bits and says so
(tests/golden/make_golden_per_ray_bits.py).

Only the source of an operand changed between the two forms (a register or an LDS row instead of a second load), so
equality is exact.  Loss shards are indexed by r & 63: with R <= 64 every shard slot receives one add per kernel (two
commuting ones in the paired proposal launch), so the sums do not depend on the order of the waves either.  Buffers are
compared as bytes: NaN payloads and the sign of zero count, and a buffer whose pointer a case passes as NULL has to stay
all-zero.

Inputs of every case: strictly increasing bins; about 10 % of the selectors off (x01[3i] <= 0); ray 1 with all
pre-activations at -60 (all weights zero: pdf padding, isnan(t) path); ray 2 with one pre-activation of +80 (exponent
cap, and at loss scale 65536 the fp16 overflow flag); gt_depth with zeros (depth mask off).  R = 5 is a partial
workgroup, R = 64 sixteen of them.
"""
import pytest
import torch

from helpers import per_ray_cases as prc
from helpers.per_ray_cases import MAIN_CASES, PAIR_CASES, PDF_CASES, PROP_CASES, RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    return prc.load_record()["cases"]


def _recorded_bits(record, device, family, case, R):
    """one run of the case -> its output tensors, every one holding the recorded bits"""
    index = prc.CASES[family].index(case)
    key = prc.record_key(family, index, R)
    assert key in record, f"{key}: not in {prc.RECORD_PATH}"
    inp = prc.inputs(family, case, R)
    assert prc.inputs_digest(inp) == record[key]["inputs"], (
        f"{family} case {index} R={R}: the INPUTS differ from the recorded ones -- the input builders (or torch's CPU "
        "generator) changed, not the kernel")
    out = prc.run(family, case, R, inp, device)
    for name, t in out.items():
        assert name in record[key]["outputs"], f"{key}: no recorded digest for buffer {name}"
        assert prc.digest(t) == record[key]["outputs"][name], (
            f"{family} case {index} R={R}: buffer {name} differs from the recorded bits")
    return out


# ------------------------------------------------------------------------------------------------
# nvo_weights_pdf
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,S_out,anneal,anneal_dev,jitter,x01_out,pre_stride,bf16,sigma", PDF_CASES)
def test_weights_pdf_forms_same_bits(device, record, S, S_out, anneal, anneal_dev, jitter, x01_out, pre_stride, bf16,
                                   sigma):
    case = (S, S_out, anneal, anneal_dev, jitter, x01_out, pre_stride, bf16, sigma)
    for R in RS:
        new = _recorded_bits(record, device, "weights_pdf", case, R)
        w = new["weights"].view(R, S)
        assert bool(torch.isfinite(w).all()) and float(w[1].abs().max()) == 0.0
        if S_out:
            sbo = new["sbins_out"]
            assert bool(torch.isfinite(sbo).all()) and bool((sbo[:, 1:] >= sbo[:, :-1]).all())


# ------------------------------------------------------------------------------------------------
# nvo_main_render_loss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,training,gt_depth,distortion_mult,normals,tile_live,drgb_stride,scale_dev,bf16", MAIN_CASES)
def test_main_render_loss_forms_same_bits(device, record, S, training, gt_depth, distortion_mult, normals, tile_live,
                                        drgb_stride, scale_dev, bf16):
    case = (S, training, gt_depth, distortion_mult, normals, tile_live, drgb_stride, scale_dev, bf16)
    for R in RS:
        new = _recorded_bits(record, device, "main_render_loss", case, R)
        assert bool(torch.isfinite(new["out_rgb"]).all()) and bool(torch.isfinite(new["weights"]).all())
        if training:
            assert float(new["losses"][:, 0].sum()) > 0.0
        else:
            assert not bool(new["dpre"].any()) and not bool(new["losses"].any())


# ------------------------------------------------------------------------------------------------
# nvo_prop_loss / nvo_prop_loss_pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,S_main,training,dpre_stride,gt_depth,scale_dev,bf16", PROP_CASES)
def test_prop_loss_forms_same_bits(device, record, S, S_main, training, dpre_stride, gt_depth, scale_dev, bf16):
    case = (S, S_main, training, dpre_stride, gt_depth, scale_dev, bf16)
    for R in RS:
        new = _recorded_bits(record, device, "prop_loss", case, R)
        assert bool(torch.isfinite(new["losses"]).all()) and float(new["losses"][:, 0].sum()) > 0.0
        if not training:
            assert not bool(new["dpre"].any())


@pytest.mark.parametrize("Ss,S_main,training,dpre_stride,gt_depth,bf16", PAIR_CASES)
def test_prop_loss_pair_forms_same_bits(device, record, Ss, S_main, training, dpre_stride, gt_depth, bf16):
    case = (Ss, S_main, training, dpre_stride, gt_depth, bf16)
    for R in RS:
        new = _recorded_bits(record, device, "prop_loss_pair", case, R)
        assert bool(torch.isfinite(new["losses"]).all()) and float(new["losses"][:, 0].sum()) > 0.0
