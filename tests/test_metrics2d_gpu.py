"""csrc/metrics2d.hip through nerf_vo_amd/metrics2d.py on the GPU: the colour accumulators against the numpy oracle
(helpers/metrics2d_oracle.py) bit for bit, PSNR against the host functions with ==, MSSIM against the reference-made
goldens, the depth table against the goldens and the host function, and ``Evaluator2D(device=cuda)`` against the host
path.

Bounds.  PSNR: equality (integer sums).  MSSIM: 2e-6, the bound test_evaluation_cpu.py states for the separable window.
Depth, float columns: each is a mean (or its root) of n non-negative float64 terms, so another order of summation moves it
by at most n * 2^-53 relative; under ``with_scale`` the scale -- a ratio of two such sums, 2 n 2^-53 -- is amplified by
mean(pred) / mean(|diff|) in the difference columns.  For the golden pairs (n <= 1600, amplification 12 to 50: at most
1.8e-13 * 101) the issue's rtol = 1e-10 covers it; for the 680 x 1200 frame the bound is computed from its own n and
amplification (``_depth_rtol``).  Delta columns: equal, under the precondition (asserted on the host first) that no
pixel's ratio lies within 1e-9 of a threshold.  Measured margins go to the file NVO_M2D_MARGINS names, when it is set
(one run's file is kept as profiles/metrics2d_parity_margins.json)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import metrics2d_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MSSIM_BOUND = 2e-6
DEPTH_RTOL_GOLDEN = 1e-10
FLOAT_COLUMNS = ("absolute_relative", "absolute_difference", "square_relative", "square_difference", "square_log_difference")
DELTA_COLUMNS = ("delta1", "delta2", "delta3")
MARGINS = {}


def _shapes():
    from nerf_vo_amd import _lib

    return [(1, 1), (3, 40), (40, 3), (11, 11), (13, 40), (37, 70), (_lib.M2D_TILE_H + 1, 2 * _lib.M2D_TILE_W + 1)]


SHAPES = _shapes()
BATCH = 5


@pytest.fixture(scope="module")
def gold_eval():
    return np.load(os.path.join(GOLDEN, "evaluation_golden.npz"))


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("NVO_M2D_MARGINS")
    if MARGINS and path:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(MARGINS, fh, indent=1, sort_keys=True)
        except OSError:
            pass


def _u8_frames(shape, seed):
    """BATCH uint8 frame pairs of different content: noise, JPEG-like small differences, a flat frame, 0 against 255."""
    rng = np.random.default_rng(seed)
    h, w = shape
    a = rng.integers(0, 256, (BATCH, h, w, 3), dtype=np.uint8)
    b = a.copy()
    b[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b[1] = np.clip(a[1].astype(int) + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    a[2] = 128
    b[2] = 131
    a[3], b[3] = 0, 255
    # frame 4: identical
    return a, b


def _f32_frames(shape, seed):
    rng = np.random.default_rng(seed)
    h, w = shape
    a = rng.uniform(-1, 1, (BATCH, 3, h, w)).astype(np.float32)
    b = np.clip(a + rng.choice([0.02, 0.3, 1.0], size=(BATCH, 1, 1, 1)) * rng.normal(size=a.shape), -1, 1).astype(np.float32)
    b[4] = a[4]
    return a, b


def _table(device, a, b):
    from nerf_vo_amd import metrics2d

    return metrics2d.color_accumulators(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", ["uint8", "float32"])
def test_color_accumulators_equal_the_oracle(device, shape, form):
    if form == "uint8":
        a, b = _u8_frames(shape, seed=1000 * shape[0] + shape[1])
        expect = np.stack([orc.color_accumulators_u8(x, y) for x, y in zip(a, b)])
    else:
        a, b = _f32_frames(shape, seed=1000 * shape[0] + shape[1] + 500)
        expect = np.stack([orc.color_accumulators_f32(x, y) for x, y in zip(a, b)])
    batch = _table(device, a, b)
    assert batch.shape == (BATCH, 3, 3) and batch.dtype == np.int64
    assert np.array_equal(batch, expect), f"accumulators differ from the oracle at {np.argwhere(batch != expect)[:5].tolist()}"
    assert _table(device, a, b).tobytes() == batch.tobytes(), "two runs differ"
    for k in range(BATCH):  # a frame alone in its launch
        assert _table(device, a[k:k + 1], b[k:k + 1]).tobytes() == batch[k:k + 1].tobytes(), f"frame {k} alone differs"
    if form == "uint8":
        n = shape[0] * shape[1]
        assert (batch[4] == np.array([0, 0, n << 32])).all()        # identical images: every s is exactly 1
        assert (batch[3, :, 0] == n).all() and (batch[3, :, 1] == 65025 * n).all()  # 255^2 = 65025 = 1 mod 256


def test_psnr_equals_the_host_functions(device):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.mapping.renderer import calculate_psnr_float, calculate_psnr_reference

    rng = np.random.default_rng(5)
    h, w = 37, 70
    a = rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)      # differences of 16 and more: the uint8 square wraps
    a[1, :4], b[1, :4] = 0, 255                                  # 0 against 255
    b[2, ..., 1] = a[2, ..., 1]                                  # one identical channel: inf
    b[3] = np.clip(a[3].astype(int) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)  # no wrap at all
    rows = metrics2d.color_metrics(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), float_psnr=True)
    assert [list(r) for r in rows] == [["psnr", "mssim", "psnr_float"]] * 4
    for k, row in enumerate(rows):
        assert row["psnr"] == calculate_psnr_reference(a[k], b[k]), f"frame {k}"
        assert row["psnr_float"] == calculate_psnr_float(a[k], b[k]), f"frame {k}"
    assert rows[2]["psnr"] == float("inf") and rows[2]["psnr_float"] == float("inf")
    assert rows[0]["psnr"] != rows[0]["psnr_float"] and rows[3]["psnr"] == rows[3]["psnr_float"]
    single = metrics2d.color_metrics(torch.from_numpy(a[0]).to(device), torch.from_numpy(b[0]).to(device))
    assert list(single) == ["psnr", "mssim"] and single["psnr"] == rows[0]["psnr"] and single["mssim"] == rows[0]["mssim"]


@pytest.mark.parametrize("i", range(3))
def test_mssim_matches_the_reference_goldens(device, gold_eval, i):
    from nerf_vo_amd import metrics2d

    a, b = gold_eval[f"ssim{i}_a"], gold_eval[f"ssim{i}_b"]
    value = metrics2d.mssim(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
    golden = float(gold_eval[f"ssim{i}_value"])
    print(f"ssim{i}: gpu {value!r} golden {golden!r} |diff| {abs(value - golden):.3e}")
    MARGINS[f"mssim_golden{i}"] = {"abs_err": abs(value - golden), "bound": MSSIM_BOUND}
    assert isinstance(value, float) and abs(value - golden) <= MSSIM_BOUND
    assert value == orc.mssim(a, b)  # the oracle's integer sum, hence its quotient


# ---------------------------------------------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------------------------------------------
def _assert_clear_of_thresholds(gt, pred, with_scale):
    from nerf_vo_amd.evaluation import _valid

    m = _valid(gt, pred)
    g, p = gt[m].astype(np.float64), pred[m].astype(np.float64)
    if with_scale:
        p = p * (g.mean() / p.mean())
    ratio = np.maximum(g / p, p / g)
    for threshold in (1.25, 1.25 ** 2, 1.25 ** 3):
        assert np.abs(ratio - threshold).min() > 1e-9, "precondition: a ratio within 1e-9 of a delta threshold"


def _compare_depth(name, got, expect, rtol):
    assert list(got) == list(expect)
    for k in FLOAT_COLUMNS:
        err = abs(got[k] - expect[k]) / abs(expect[k])
        print(f"{name} {k}: gpu {got[k]!r} host {expect[k]!r} rel {err:.3e} (bound {rtol:.3e})")
        MARGINS[f"{name}.{k}"] = {"rel_err": float(err), "bound": rtol}
        assert err <= rtol, f"{name} {k}"
    for k in DELTA_COLUMNS:
        assert got[k] == expect[k], f"{name} {k}"


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("i", range(3))
def test_depth_metrics_match_the_goldens(device, gold_eval, i, with_scale):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import calculate_depth_metrics_2d

    gt, pred = gold_eval[f"depth{i}_gt"], gold_eval[f"depth{i}_pred"]
    assert gt.size <= 1600
    _assert_clear_of_thresholds(gt, pred, with_scale)
    got = metrics2d.depth_metrics(torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device), with_scale=with_scale)
    host = calculate_depth_metrics_2d(gt, pred, with_scale=with_scale)
    _compare_depth(f"golden{i}_scale{int(with_scale)}", got, host, DEPTH_RTOL_GOLDEN)
    names = [str(n) for n in gold_eval["depth_metric_names"]]
    golden = dict(zip(names, gold_eval[f"depth{i}_metrics_scale{int(with_scale)}"]))
    _compare_depth(f"golden{i}_scale{int(with_scale)}_reference", got, {k: golden[k] for k in got}, DEPTH_RTOL_GOLDEN)


def _special_depths():
    rng = np.random.default_rng(7)
    gt = rng.uniform(0.2, 4.8, (BATCH, 23, 41))
    pred = gt / 1.4 * (1 + 0.1 * rng.normal(size=gt.shape))
    gt[0, 0, :8] = [np.nan, np.inf, -np.inf, -1.0, 0.0, 5.0, 7.5, -0.0]
    pred[0, 1, :8] = [np.nan, np.inf, -np.inf, -1.0, 0.0, 5.0, 7.5, -0.0]
    gt[1] = rng.choice([np.nan, -1.0, 0.0, 5.0, np.inf], size=gt[1].shape)  # no valid pixel
    pred[2, ::2] = -pred[2, ::2]
    return gt, pred


def test_depth_invalid_pixels_and_empty_frames(device):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import calculate_depth_metrics_2d

    gt, pred = _special_depths()
    for with_scale in (True, False):
        rows = metrics2d.depth_metrics(torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device), with_scale=with_scale)
        assert len(rows) == BATCH
        for k in (0, 2, 3, 4):
            _assert_clear_of_thresholds(gt[k], pred[k], with_scale)
            with np.errstate(invalid="ignore"):
                host = calculate_depth_metrics_2d(gt[k], pred[k], with_scale=with_scale)
            _compare_depth(f"special{k}_scale{int(with_scale)}", rows[k], host, DEPTH_RTOL_GOLDEN)
        assert list(rows[1]) == list(metrics2d.DEPTH_METRICS) and all(np.isnan(v) for v in rows[1].values())


def test_depth_float32_input_and_alone_against_batch(device):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import calculate_depth_metrics_2d

    gt, pred = _special_depths()
    gt32, pred32 = gt.astype(np.float32), pred.astype(np.float32)
    g, p = torch.from_numpy(gt32).to(device), torch.from_numpy(pred32).to(device)
    batch = metrics2d.depth_accumulators(g, p).cpu().numpy()
    assert batch.shape == (BATCH, 9)
    assert metrics2d.depth_accumulators(g, p).cpu().numpy().tobytes() == batch.tobytes(), "two runs differ"
    for k in range(BATCH):
        alone = metrics2d.depth_accumulators(g[k:k + 1], p[k:k + 1]).cpu().numpy()
        assert alone.tobytes() == batch[k:k + 1].tobytes(), f"frame {k} alone differs"
    # the float64 copy of the same values on the device gives the same bits: the conversion is per element
    assert metrics2d.depth_accumulators(g.double(), p.double()).cpu().numpy().tobytes() == batch.tobytes()
    assert metrics2d.depth_accumulators(g.double(), p).cpu().numpy().tobytes() == batch.tobytes()
    rows = metrics2d.depth_metrics_of_table(batch)
    for k in (0, 2, 3, 4):
        _assert_clear_of_thresholds(gt32[k].astype(np.float64), pred32[k].astype(np.float64), True)
        with np.errstate(invalid="ignore"):
            host = calculate_depth_metrics_2d(gt32[k].astype(np.float64), pred32[k].astype(np.float64))
        _compare_depth(f"float32_{k}", rows[k], host, DEPTH_RTOL_GOLDEN)
    single = metrics2d.depth_metrics(g[3], p[3])
    assert all(single[k] == rows[3][k] for k in single)


# ---------------------------------------------------------------------------------------------------------------
# one frame of the reference's size
# ---------------------------------------------------------------------------------------------------------------
def _depth_rtol(gt, pred, with_scale):
    """n 2^-53 for another order of the sums, plus (with_scale) the scale's 2 n 2^-53 amplified by mean(pred) / mean(|diff|);
    16 ulp on top for the libraries' log and the handful of operations per pixel."""
    from nerf_vo_amd.evaluation import _valid

    m = _valid(gt, pred)
    g, p = gt[m], pred[m]
    n = int(m.sum())
    bound = n * 2.0 ** -53 + 16 * 2.0 ** -53
    if with_scale:
        p = p * (g.mean() / p.mean())
        bound += 2 * n * 2.0 ** -53 * (p.mean() / np.abs(p - g).mean())
    return bound


def test_full_size_frame_against_the_host_functions(device):
    from nerf_vo_amd import metrics2d
    from nerf_vo_amd.evaluation import calculate_color_metrics_2d, calculate_depth_metrics_2d

    h, w = 680, 1200
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 90 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] * np.array([1.0, 0.7, -0.8])).astype(np.int64)
    a = np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)
    got = metrics2d.color_metrics(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
    host = calculate_color_metrics_2d(a, b)
    print(f"680x1200 psnr gpu {got['psnr']!r} host {host['psnr']!r}; mssim gpu {got['mssim']!r} host {host['mssim']!r} "
          f"|diff| {abs(got['mssim'] - host['mssim']):.3e}")
    MARGINS["full_size.mssim"] = {"abs_err": abs(got["mssim"] - host["mssim"]), "bound": MSSIM_BOUND}
    assert got["psnr"] == host["psnr"]
    assert abs(got["mssim"] - host["mssim"]) <= MSSIM_BOUND

    gt = 2.5 + 1.8 * np.sin(xx / 91.0) * np.cos(yy / 57.0) + rng.uniform(-0.3, 0.3, (h, w))
    pred = gt / 1.3 * (1 + 0.05 * rng.normal(size=(h, w)))
    gt[:7, :] = 0.0
    pred[-5:, :] = 6.0
    for with_scale in (True, False):
        _assert_clear_of_thresholds(gt, pred, with_scale)
        rtol = _depth_rtol(gt, pred, with_scale)
        rows = metrics2d.depth_metrics(torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device), with_scale=with_scale)
        _compare_depth(f"full_size_scale{int(with_scale)}", rows, calculate_depth_metrics_2d(gt, pred, with_scale=with_scale), rtol)


# ---------------------------------------------------------------------------------------------------------------
# Evaluator2D(device=cuda)
# ---------------------------------------------------------------------------------------------------------------
def test_evaluator2d_on_the_device_matches_the_host_path(device, tmp_path):
    import pandas as pd
    from test_evaluation_cpu import _FakeNerf

    from nerf_vo_amd.evaluation import EvaluationRenderer, Evaluator2D, read_depth_png16
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    ds = SyntheticEvaluationDataset(num_frames=24, height=60, width=80)
    keyframes = list(range(0, 24, 4))
    rot = np.eye(4)
    rot[:3, :3] = [[np.cos(0.7), -np.sin(0.7), 0], [np.sin(0.7), np.cos(0.7), 0], [0, 0, 1]]
    rot[:3, 3] = [0.3, -0.2, 0.1]
    nerf = _FakeNerf(ds, keyframes, rot, shrink=0.25)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=keyframes, dir_prediction=str(tmp_path / "pred"))
    renderer.render_frames(mode="evaluation_frames")
    lpips_calls = []

    def fake_lpips(x, y):
        lpips_calls.append(x.device.type)
        return (x - y).abs().mean()

    host_means = Evaluator2D(ds, keyframes, str(tmp_path / "pred"), str(tmp_path / "host"),
                             lpips_loss=fake_lpips).calculate_metrics_2d("evaluation_frames")
    gpu_means = Evaluator2D(ds, keyframes, str(tmp_path / "pred"), str(tmp_path / "gpu"), lpips_loss=fake_lpips, device=device,
                            frames_per_launch=3).calculate_metrics_2d("evaluation_frames")
    assert set(lpips_calls) == {"cpu"}
    host = pd.read_csv(tmp_path / "host" / "metrics_2d_evaluation_frames.csv")
    gpu = pd.read_csv(tmp_path / "gpu" / "metrics_2d_evaluation_frames.csv")
    assert list(gpu.columns) == list(host.columns) and len(gpu) == len(host) == len(ds.evaluation_frames) > 3
    assert list(gpu_means) == list(host_means)
    assert os.path.exists(tmp_path / "gpu" / "metrics_2d_evaluation_frames.json")
    assert (gpu["psnr"] == host["psnr"]).all() and (gpu["lpips"] == host["lpips"]).all()
    assert (gpu["mssim"] - host["mssim"]).abs().max() <= MSSIM_BOUND
    # depth: the bound of each frame from its own n and amplification (a near-perfect prediction: |diff| is the PNG's
    # quantisation step, so the amplification is in the ten thousands)
    depths_gt = ds.frames_depth(mode="evaluation_frames", keyframes=keyframes)
    depth_dir = tmp_path / "pred" / "evaluation_frames" / "depth"
    depths_pred = [read_depth_png16(str(depth_dir / f)) / ds.camera_intrinsics["depth_scale"] for f in sorted(os.listdir(depth_dir))]
    for row, (d_gt, d_pred) in enumerate(zip(depths_gt, depths_pred)):
        _assert_clear_of_thresholds(d_gt, d_pred, True)
        rtol = _depth_rtol(d_gt, d_pred, True)
        for k in FLOAT_COLUMNS:
            err = abs(gpu[k][row] - host[k][row]) / abs(host[k][row])
            MARGINS[f"evaluator2d.frame{row}.{k}"] = {"rel_err": float(err), "bound": rtol}
            assert err <= rtol, (row, k)
    for k in DELTA_COLUMNS:
        assert (gpu[k] == host[k]).all(), k
