"""Host side of the 2-D evaluation tables: the numpy oracle of the colour rule of csrc/metrics2d.hip
(helpers/metrics2d_oracle.py) against the reference-made MSSIM goldens and ``calculate_mssim``, and the trajectory table
(``kabsch_umeyama_alignment``, ``calculate_absolute_trajectory_error``, ``EvaluatorTrajectory``) against
tests/golden/trajectory_golden.npz (made by the reference's functions: make_golden_trajectory.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from helpers import metrics2d_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MSSIM_BOUND = 2e-6  # the bound test_evaluation_cpu.py states for the separable form against the reference's 11 x 11 window


@pytest.fixture(scope="module")
def gold_eval():
    return np.load(os.path.join(GOLDEN, "evaluation_golden.npz"))


@pytest.fixture(scope="module")
def gold_traj():
    return np.load(os.path.join(GOLDEN, "trajectory_golden.npz"))


@pytest.mark.parametrize("i", range(3))
def test_oracle_mssim_matches_the_reference_goldens(gold_eval, i):
    value = orc.mssim(gold_eval[f"ssim{i}_a"], gold_eval[f"ssim{i}_b"])
    err = abs(value - float(gold_eval[f"ssim{i}_value"]))
    print(f"ssim{i}: oracle {value!r} golden {float(gold_eval[f'ssim{i}_value'])!r} |diff| {err:.3e}")
    assert err <= MSSIM_BOUND


def test_oracle_mssim_matches_calculate_mssim_on_uint8_images():
    from nerf_vo_amd.evaluation import calculate_mssim

    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (37, 70, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-20, 20, a.shape), 0, 255).astype(np.uint8)

    def to_tensor(img):
        return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(0).float().div(255.0) * 2 - 1

    ta, tb = to_tensor(a), to_tensor(b)
    # the oracle's uint8 conversion is torch's, bit for bit
    assert np.array_equal(orc.to_signed(a).view(np.uint32), ta[0].numpy().view(np.uint32))
    value, host = orc.mssim(orc.to_signed(a), orc.to_signed(b)), calculate_mssim(ta, tb)
    print(f"oracle {value!r} calculate_mssim {host!r} |diff| {abs(value - host):.3e}")
    assert abs(value - host) <= MSSIM_BOUND


def test_oracle_identical_images_give_exactly_one():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (20, 33, 3), dtype=np.uint8)
    assert orc.mssim(orc.to_signed(a), orc.to_signed(a)) == 1.0
    flat = np.full((12, 9, 3), 128, np.uint8)
    assert orc.mssim(orc.to_signed(flat), orc.to_signed(flat)) == 1.0


def test_oracle_fixed_point_mean_is_the_float64_mean():
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, (3, 19, 23)).astype(np.float32)
    b = np.clip(a + 0.2 * rng.normal(size=a.shape), -1, 1).astype(np.float32)
    s = orc.ssim_map(a, b)
    # every term is rounded to a multiple of 2^-32: the mean moves by at most 2^-33
    assert abs(orc.mssim(a, b) - float(s.astype(np.float64).mean())) <= 2.0 ** -33 + 1e-16


def test_oracle_psnr_of_sums_equals_the_host_functions():
    from nerf_vo_amd.mapping.renderer import calculate_psnr_float, calculate_psnr_reference

    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (13, 21, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (13, 21, 3), dtype=np.uint8)  # differences of 16 and more: the uint8 square wraps
    b[..., 1] = a[..., 1]                                  # one identical channel: inf
    acc = orc.color_accumulators_u8(a, b)
    assert orc.psnr_of_sums(acc[:, 0], 13 * 21) == calculate_psnr_reference(a, b) == float("inf")
    b[0, 0, 1] ^= 0x80
    acc = orc.color_accumulators_u8(a, b)
    assert orc.psnr_of_sums(acc[:, 0], 13 * 21) == calculate_psnr_reference(a, b)
    assert orc.psnr_of_sums(acc[:, 1], 13 * 21) == calculate_psnr_float(a, b)
    assert (acc[:, 0] != acc[:, 1]).any()


def test_launch_shape_queries_refuse_what_the_kernels_cannot_index():
    """Host-only entry points of section N: 0 means 'refused'."""
    from nerf_vo_amd import _lib

    lib = _lib.lib()
    tiles = -(-37 // _lib.M2D_TILE_H) * -(-70 // _lib.M2D_TILE_W)
    assert lib.nvo_m2d_color_scratch_bytes(5, 37, 70) == 5 * 3 * tiles * _lib.M2D_COLOR_WORDS * 8
    assert lib.nvo_m2d_color_scratch_bytes(1, 1 << 15, 1 << 14) == 0     # 3 H W >= 2^30
    assert lib.nvo_m2d_color_scratch_bytes(0, 4, 4) == 0 and lib.nvo_m2d_color_scratch_bytes(21846, 4, 4) == 0
    assert lib.nvo_m2d_depth_chunks(1, 1) == 1 and lib.nvo_m2d_depth_chunks(680, 1200) == 256
    assert lib.nvo_m2d_depth_chunks(40, 52) == 2                          # 2080 pixels: one more than a chunk's 2048
    assert lib.nvo_m2d_depth_chunks(1 << 16, 1 << 15) == 0                # H W >= 2^31
    assert lib.nvo_m2d_depth_scratch_bytes(3, 40, 52) == 3 * 2 * 11 * 8
    args = _lib.M2dColorArgs(F=1, H=4, W=4)
    assert lib.nvo_m2d_color(None, args) != 0 and b"NULL" in lib.nvo_last_error()
    assert lib.nvo_m2d_depth(None, _lib.M2dDepthArgs(F=1, H=4, W=4)) != 0 and b"NULL" in lib.nvo_last_error()


def test_gpu_functions_refuse_host_tensors():
    from nerf_vo_amd import metrics2d

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics2d.depth_metrics(torch.ones(4, 4), torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics2d.color_metrics(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, 3, dtype=torch.uint8))
    assert np.array_equal(metrics2d.gaussian_taps().view(np.uint32), orc.gaussian_taps().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# trajectory table
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3))
def test_ate_functions_match_the_reference(gold_traj, i):
    from nerf_vo_amd.evaluation import ATE_METRICS, calculate_absolute_trajectory_error, kabsch_umeyama_alignment

    assert tuple(gold_traj["ate_names"]) == ATE_METRICS
    gt, pred, with_scale = gold_traj[f"traj{i}_gt"], gold_traj[f"traj{i}_pred"], bool(gold_traj[f"traj{i}_with_scale"])
    assert 5 <= gt.shape[0] <= 40
    rotation, translation, scale = kabsch_umeyama_alignment(gt[:, :3, 3], pred[:, :3, 3], with_scale=with_scale)
    assert translation.shape == (3, 1)
    np.testing.assert_allclose(rotation, gold_traj[f"traj{i}_rotation"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(translation, gold_traj[f"traj{i}_translation"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(scale, gold_traj[f"traj{i}_scale"], rtol=1e-12, atol=0)
    assert np.linalg.det(rotation) == pytest.approx(1.0, abs=1e-12)  # never a reflection
    if not with_scale:
        assert scale == 1.0
    ate = calculate_absolute_trajectory_error(gt, pred, with_scale=with_scale)
    assert tuple(ate) == ATE_METRICS
    np.testing.assert_allclose([ate[k] for k in ATE_METRICS], gold_traj[f"traj{i}_ate"], rtol=1e-12, atol=0)


def test_golden_trajectories_cover_the_reflection_guard(gold_traj):
    """The nearly planar case is one where the SVD's two bases disagree in handedness (the guard flips the last axis)."""
    flips = []
    for i in range(3):
        a, b = gold_traj[f"traj{i}_gt"][:, :3, 3], gold_traj[f"traj{i}_pred"][:, :3, 3]
        u, _, vt = np.linalg.svd(((a - a.mean(0)).T @ (b - b.mean(0))) / len(a))
        flips.append(np.linalg.det(u) * np.linalg.det(vt) < 0)
    assert any(flips)
    assert not all(bool(gold_traj[f"traj{i}_with_scale"]) for i in range(3))


def _write_poses(directory, name, poses):
    os.makedirs(directory / "matrices", exist_ok=True)
    with open(directory / "matrices" / f"matrices_origin2frame_{name}.json", "w") as file:
        json.dump(poses.tolist(), file)


def test_evaluator_trajectory_round_trip(tmp_path, gold_traj):
    import pandas as pd

    from nerf_vo_amd.evaluation import ATE_METRICS, EvaluatorTrajectory, calculate_absolute_trajectory_error

    gt, pred = gold_traj["traj0_gt"], gold_traj["traj0_pred"]
    keyframes = list(range(0, 2 * gt.shape[0], 2))
    extrinsics = np.tile(np.eye(4), (2 * gt.shape[0], 1, 1))
    extrinsics[keyframes] = gt
    dataset = types.SimpleNamespace(camera_extrinsics=extrinsics)
    ev = EvaluatorTrajectory(dataset, keyframes, str(tmp_path / "pred"), str(tmp_path / "res"))
    with pytest.raises(FileNotFoundError, match="neither"):
        ev.calculate_metrics_trajectory()
    assert not os.path.exists(tmp_path / "res" / "metrics_trajectory.csv")

    # the mapping file alone: one row, and the returned dict is that row
    _write_poses(tmp_path / "pred", "keyframes_mapping", pred)
    out = ev.calculate_metrics_trajectory()
    expect = calculate_absolute_trajectory_error(gt, pred, with_scale=True)
    assert list(out) == list(ATE_METRICS) and all(out[k] == expect[k] for k in ATE_METRICS)
    table = pd.read_csv(tmp_path / "res" / "metrics_trajectory.csv")
    assert list(table.columns) == list(ATE_METRICS) + ["trajectory"]
    assert table["trajectory"].tolist() == ["keyframes_mapping"]
    np.testing.assert_allclose(table[list(ATE_METRICS)].to_numpy()[0], gold_traj["traj0_ate"], rtol=1e-12)

    # both files: tracking first, as the reference orders them
    tracked = pred.copy()
    tracked[:, :3, 3] += 0.05 * np.random.default_rng(4).normal(size=(gt.shape[0], 3))
    _write_poses(tmp_path / "pred", "keyframes_tracking", tracked)
    ev.calculate_metrics_trajectory()
    table = pd.read_csv(tmp_path / "res" / "metrics_trajectory.csv")
    assert table["trajectory"].tolist() == ["keyframes_tracking", "keyframes_mapping"]
    assert table["absolute_trajectory_error_rmse"][0] > table["absolute_trajectory_error_rmse"][1]

    # a file whose pose count is not the keyframes' is an error, not a silent broadcast
    _write_poses(tmp_path / "pred", "keyframes_tracking", tracked[:-1])
    with pytest.raises(ValueError, match="shape"):
        ev.calculate_metrics_trajectory()


def test_evaluator2d_rejects_a_host_device(tmp_path):
    from nerf_vo_amd.evaluation import Evaluator2D

    with pytest.raises(ValueError, match="CUDA"):
        Evaluator2D(None, [], str(tmp_path), str(tmp_path), device="cpu")
    assert Evaluator2D(None, [], str(tmp_path), str(tmp_path)).device is None
