"""LPIPS on the GPU (nerf_vo_amd/lpips.py, csrc/lpips.hip), kernel by kernel and as a whole, against
the float64 restatement of helpers/lpips_oracle.py on the cases of helpers/lpips_cases.py.

Bounds: the convolution on integer data, the max-pool, the uint8 ingest, batch independence and the mean's order are
EQUALITIES.  The float comparisons use 2.5 x the recorded error of the float32 sequential-chain oracle against float64
(profiles/lpips_parity_margins.json; 2.5 x is the margin of test_poisson_cpu.py over such a difference): per layer for
the feature maps and the distance maps, and their sum over the layers for the scalar, since a mean cannot err more than
its worst pixel.  With NVO_LPIPS_MARGINS set, the share of each bound a run used is written to that file.

Shares of the bounds used on an MI355X (profiles/lpips_parity_margins.json, ``gpu_used``): see EXPERIMENTS.md section 24.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from helpers import lpips_cases as cases
from helpers import lpips_oracle as orc

pytestmark = pytest.mark.gpu

USED = {}


@pytest.fixture(scope="module", autouse=True)
def _write_used():
    yield
    path = os.environ.get("NVO_LPIPS_MARGINS")
    if USED and path:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(USED, fh, indent=1, sort_keys=True)
        except OSError:
            pass


@pytest.fixture(scope="module")
def model(device):
    from nerf_vo_amd.lpips import LPIPS

    return LPIPS(cases.weights(), device=device)


@pytest.fixture(scope="module")
def recorded():
    return cases.recorded()["cases"]


def _images(name):
    a, b = cases.frames(name)
    return orc.image_of_uint8(a), orc.image_of_uint8(b)


# ---------------------------------------------------------------------------------------------------------------
# 1. convolution + bias + ReLU: exact on integer data
# ---------------------------------------------------------------------------------------------------------------
def _conv_configs():
    out = []
    for F in (1, 3):
        for H in (31, 32, 33, 34):
            out.append((0, F, H, 35))
        for layer in (1, 2, 3, 4):
            for H, W in ((13, 17), (3, 5), (1, 1)):
                out.append((layer, F, H, W))
    return out


@pytest.mark.parametrize("layer,F,H,W", _conv_configs(), ids=lambda v: str(v))
def test_convolution_is_exact_on_integers(device, layer, F, H, W):
    """Inputs and weights are whole numbers in [-2, 2], biases in [-3, 3]: every partial sum is a whole number of at most
    3456 * 4 + 3 = 13 827 < 2^24, so every summation order gives the float64 result exactly."""
    from nerf_vo_amd import lpips

    cin, cout, k, stride, pad = lpips.LAYERS[layer]
    g = torch.Generator().manual_seed(100 * layer + 10 * F + H)
    x = torch.randint(-2, 3, (F, cin, H, W), generator=g).float()
    w = torch.randint(-2, 3, (cout, cin, k, k), generator=g).float()
    b = torch.randint(-3, 4, (cout,), generator=g).float()
    ref = TF.relu(TF.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))
    got = lpips.conv2d_relu(x.to(device), w.to(device), b.to(device), stride, pad).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    assert float(ref.abs().max()) <= 13827
    assert torch.equal(got.double(), ref)
    assert 0.25 < float((ref > 0).double().mean()) < 0.75, "about half the outputs survive the ReLU"


# ---------------------------------------------------------------------------------------------------------------
# 2. max-pool
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 7), (8, 9), (16, 23)])
def test_maxpool_equals_torchs(device, H, W):
    from nerf_vo_amd import lpips

    x = torch.randn(2, 5, H, W, generator=torch.Generator().manual_seed(H * W))
    x[0, 0] = -x[0, 0].abs() - 1  # a plane of negative values only
    got = lpips.maxpool_3x3_s2(x.to(device)).cpu()
    assert torch.equal(got, TF.max_pool2d(x, 3, 2))


# ---------------------------------------------------------------------------------------------------------------
# 3. head
# ---------------------------------------------------------------------------------------------------------------
HEAD_CASE = "67x95"


@pytest.mark.parametrize("layer", range(5))
def test_head_map_and_mean(device, recorded, layer):
    """The head alone, fed with the float64 oracle's features rounded to float32: the map against the float64 head of
    those same inputs, the mean against the fixed-order float64 mean of the kernel's own map."""
    from nerf_vo_amd import lpips

    ref = cases.reference(HEAD_CASE)
    f0, f1 = (t.float() for t in ref["features"][layer])
    lin = cases.weights()[f"lin{layer}.model.1.weight"]
    expect = orc.head_map(f0, f1, lin, "float64")
    a, b, w = f0.to(device), f1.to(device), lin.to(device)
    dmap = lpips.head(a, b, w, want="map").cpu()
    assert tuple(dmap.shape) == (f0.shape[0], 1, f0.shape[2], f0.shape[3])
    err, bound = float((dmap[:, 0].double() - expect).abs().max()), cases.MARGIN * recorded[HEAD_CASE][layer]["map_err"]
    USED[f"head.{HEAD_CASE}.f{layer + 1}.map"] = {"err": err, "bound": bound, "used": err / bound}
    print(f"head map f{layer + 1}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    mean = lpips.head(a, b, w, want="mean").cpu()
    assert tuple(mean.shape) == (f0.shape[0], 1, 1, 1) and mean.dtype == torch.float32
    for f in range(f0.shape[0]):
        assert mean[f].item() == float(orc.tree_mean(dmap[f].numpy(), lpips._lib.LPIPS_HEAD_BLOCK)), f
    # symmetric bit for bit
    assert torch.equal(lpips.head(b, a, w, want="map").cpu(), dmap)
    assert torch.equal(lpips.head(b, a, w, want="mean").cpu(), mean)


def test_head_zero_cases(device):
    from nerf_vo_amd import lpips

    ref = cases.reference(HEAD_CASE)
    f0, f1 = (t.float().clone() for t in ref["features"][1])  # [3, 192, 7, 11]
    lin = cases.weights()["lin1.model.1.weight"].to(device)
    same = lpips.head(f0.to(device), f0.to(device), lin, want="map")
    assert float(same.abs().max()) == 0 and float(lpips.head(f0.to(device), f0.to(device), lin).abs().max()) == 0
    f0[:, :, 0, 0] = 0  # all channels zero in one image
    f1[:, :, 0, 1] = 0  # ... in the other
    f0[:, :, 0, 2] = 0  # ... in both
    f1[:, :, 0, 2] = 0
    dmap = lpips.head(f0.to(device), f1.to(device), lin, want="map").cpu()
    assert torch.isfinite(dmap).all() and torch.isfinite(lpips.head(f0.to(device), f1.to(device), lin).cpu()).all()
    assert (dmap[:, 0, 0, 2] == 0).all() and (dmap[:, 0, 0, 0] > 0).all() and (dmap[:, 0, 0, 1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. the whole model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_model_against_the_float64_oracle(device, model, recorded, name):
    x0, x1 = _images(name)
    ref = cases.reference(name)
    failures = []
    for image, x in enumerate((x0, x1)):
        maps = model.features(x.to(device))
        assert len(maps) == 5
        for l, m in enumerate(maps):
            expect = ref["features"][l][image]
            assert tuple(m.shape) == tuple(expect.shape) and m.dtype == torch.float32
            err, bound = float((m.cpu().double() - expect).abs().max()), cases.MARGIN * recorded[name][l]["feature_err"]
            key = f"model.{name}.f{l + 1}.features"
            if key not in USED or err > USED[key]["err"]:
                USED[key] = {"err": err, "bound": bound, "used": err / bound}
            print(f"{name} image {image} f{l + 1}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f})")
            if err > bound:
                failures.append((image, l, err, bound))
    value = model(x0.to(device), x1.to(device))
    assert tuple(value.shape) == (x0.shape[0], 1, 1, 1) and value.dtype == torch.float32 and value.device.type == "cuda"
    bound = sum(cases.MARGIN * r["map_err"] for r in recorded[name])
    err = float((value.cpu().view(-1).double() - ref["value"]).abs().max())
    USED[f"model.{name}.value"] = {"err": err, "bound": bound, "used": err / bound, "value": float(ref["value"][0])}
    print(f"{name} value: {float(ref['value'][0]):.6f} err {err:.3e} bound {bound:.3e} ({err / bound:.2f})")
    assert not failures, failures
    assert err <= bound
    # host images: uploaded, computed on the device, returned to the host -- the same bits
    host = model(x0, x1)
    assert host.device.type == "cpu" and torch.equal(host, value.cpu())


# ---------------------------------------------------------------------------------------------------------------
# 5. bitwise properties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_uint8_path_equals_the_float_path(device, model, name):
    a, b = cases.frames(name)
    x0, x1 = _images(name)
    from_float = model(x0.to(device), x1.to(device)).cpu().view(-1).tolist()
    from_u8 = model.lpips_uint8(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
    assert isinstance(from_u8, list) and all(isinstance(v, float) for v in from_u8)
    assert from_u8 == from_float and all(v > 0 for v in from_u8)


def test_frame_alone_equals_its_row_of_a_batch_and_runs_repeat(device, model):
    a, b = (torch.from_numpy(t).to(device) for t in cases.frames("67x95"))
    batch = model.lpips_uint8(a, b)
    assert batch == model.lpips_uint8(a, b)
    for k in range(a.shape[0]):
        assert model.lpips_uint8(a[k:k + 1], b[k:k + 1]) == [batch[k]], k
    x0, x1 = (t.to(device) for t in _images("67x95"))
    maps, again = model.features(x0), model.features(x0)
    alone = model.features(x0[1:2])
    for m, n, s in zip(maps, again, alone):
        assert torch.equal(m, n) and torch.equal(m[1:2], s)


# ---------------------------------------------------------------------------------------------------------------
# 6. Evaluator2D and color_metrics
# ---------------------------------------------------------------------------------------------------------------
def test_evaluator2d_lpips_column(device, model, tmp_path):
    import pandas as pd
    from test_evaluation_cpu import _FakeNerf

    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator2D, read_color
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=60, width=80)
    keyframes = list(range(0, 24, 4))
    rot = np.eye(4)
    rot[:3, :3] = [[np.cos(0.7), -np.sin(0.7), 0], [np.sin(0.7), np.cos(0.7), 0], [0, 0, 1]]
    rot[:3, 3] = [0.3, -0.2, 0.1]
    nerf = _FakeNerf(ds, keyframes, rot, shrink=0.25)
    pred = str(tmp_path / "pred")
    EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=pred).render_frames(mode="evaluation_frames")
    Evaluator2D(ds, keyframes, pred, str(tmp_path / "host"), lpips_loss=model).calculate_metrics_2d("evaluation_frames")
    Evaluator2D(ds, keyframes, pred, str(tmp_path / "gpu"), lpips_loss=model, device=device,
                frames_per_launch=3).calculate_metrics_2d("evaluation_frames")
    Evaluator2D(ds, keyframes, pred, str(tmp_path / "plain"), device=device, frames_per_launch=3).calculate_metrics_2d("evaluation_frames")
    host = pd.read_csv(tmp_path / "host" / "metrics_2d_evaluation_frames.csv")
    gpu = pd.read_csv(tmp_path / "gpu" / "metrics_2d_evaluation_frames.csv")
    plain = pd.read_csv(tmp_path / "plain" / "metrics_2d_evaluation_frames.csv")
    assert list(gpu.columns) == list(host.columns) == list(plain.columns) + ["lpips"] and len(gpu.columns) == 11
    assert len(gpu) == len(host) == len(plain) == len(ds.evaluation_frames) > 3
    assert (gpu["lpips"] == host["lpips"]).all() and (gpu["lpips"] > 0).all()
    for column in plain.columns:  # the other ten columns do not notice the model
        assert (gpu[column] == plain[column]).all(), column
    means = json.load(open(tmp_path / "gpu" / "metrics_2d_evaluation_frames.json"))
    assert "lpips" in means and "lpips" not in json.load(open(tmp_path / "plain" / "metrics_2d_evaluation_frames.json"))
    # ... and equal to the model frame by frame, and to color_metrics(..., lpips=model)
    color_dir = os.path.join(pred, "evaluation_frames", "color")
    colors_pred = [read_color(os.path.join(color_dir, f)) for f in sorted(os.listdir(color_dir)) if f.endswith(".jpg")]
    colors_gt = [np.array(c) for c in ds.frames_color(mode="evaluation_frames", keyframes=keyframes)]
    for k, (c_gt, c_pred) in enumerate(zip(colors_gt, colors_pred)):
        direct = float(model(orc.image_of_uint8(c_gt[None]), orc.image_of_uint8(c_pred[None])))
        assert float(gpu["lpips"][k]) == direct, k
    rows = metrics2d.color_metrics(torch.from_numpy(np.stack(colors_gt)).to(device), torch.from_numpy(np.stack(colors_pred)).to(device),
                                   lpips=model)
    bare = metrics2d.color_metrics(torch.from_numpy(np.stack(colors_gt)).to(device), torch.from_numpy(np.stack(colors_pred)).to(device))
    assert [r["lpips"] for r in rows] == gpu["lpips"].tolist()
    assert [{k: v for k, v in r.items() if k != "lpips"} for r in rows] == bare and list(rows[0]) == ["psnr", "mssim", "lpips"]
    one = metrics2d.color_metrics(torch.from_numpy(colors_gt[0]).to(device), torch.from_numpy(colors_pred[0]).to(device), lpips=model)
    assert one == rows[0]
