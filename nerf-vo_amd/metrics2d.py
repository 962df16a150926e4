"""2-D evaluation metrics on the GPU (csrc/metrics2d.hip, include/nerfvo_hip.h section N): what
``evaluation.calculate_color_metrics_2d`` / ``calculate_mssim`` / ``calculate_depth_metrics_2d`` compute frame by frame on
the host, for batches of frames that already are on the device.  The kernels fill a table of accumulators per frame --
integers for the colour metrics, float64 sums in an order fixed by the frame size for the depth metrics -- which comes to
the host in ONE copy; the means, roots and logarithms are then taken with the expressions of the CPU functions.

``psnr`` (the reference's uint8-wrapping definition) and the float PSNR equal the host functions exactly: their sums are
integers.  ``mssim`` is the mean of the fp32 SSIM map of the separable 11-tap window, summed in fixed point (2^-32), so
it has no summation order; tests/helpers/metrics2d_oracle.py restates it.  No CPU fallback: a host tensor is an error.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

TILE_H, TILE_W = _lib.M2D_TILE_H, _lib.M2D_TILE_W
DEPTH_METRICS = ("absolute_relative", "absolute_difference", "square_relative", "square_difference", "square_log_difference",
                 "delta1", "delta2", "delta3")


def gaussian_taps() -> np.ndarray:
    """The 11 taps of the reference's window (sigma 1.5): float64 on the host, rounded once to float32."""
    x = np.arange(_lib.M2D_TAPS, dtype=np.float64) - _lib.M2D_TAPS // 2
    g = np.exp(-(x ** 2) / 4.5)
    return (g / g.sum()).astype(np.float32)


def _on_gpu(what: str, *tensors) -> torch.device:
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: the images must be tensors on the GPU -- there is no CPU fallback "
                               "(the host functions are in nerf_vo_amd.evaluation)")
    if tensors[0].device != tensors[1].device or tensors[0].shape != tensors[1].shape:
        raise ValueError(f"{what}: the two images must have one shape and one device, got {tuple(tensors[0].shape)} on "
                         f"{tensors[0].device} and {tuple(tensors[1].shape)} on {tensors[1].device}")
    return tensors[0].device


def _stream(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def color_accumulators(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """int64 [F, 3, 3] on the device, per frame and channel: the sum of the wrapping uint8 squared differences, the sum of
    the true squared differences, and the fixed-point sum of the SSIM map.  ``a``, ``b``: uint8 [F, H, W, 3] (as the files
    decode) or float32 [F, 3, H, W] (the contract of ``calculate_mssim``: the first two sums are then 0)."""
    device = _on_gpu("color_accumulators", a, b)
    if a.dtype != b.dtype or a.ndim != 4:
        raise ValueError(f"color_accumulators: two uint8 [F,H,W,3] or two float32 [F,3,H,W] tensors, got {a.dtype} "
                         f"{tuple(a.shape)} and {b.dtype}")
    if a.dtype == torch.uint8 and a.shape[3] == 3:
        is_float, (F, H, W) = 0, (int(a.shape[0]), int(a.shape[1]), int(a.shape[2]))
    elif a.dtype == torch.float32 and a.shape[1] == 3:
        is_float, (F, H, W) = 1, (int(a.shape[0]), int(a.shape[2]), int(a.shape[3]))
    else:
        raise ValueError(f"color_accumulators: two uint8 [F,H,W,3] or two float32 [F,3,H,W] tensors, got {a.dtype} {tuple(a.shape)}")
    if min(F, H, W) < 1 or max(F, H, W) >= 2 ** 32:
        raise ValueError(f"color_accumulators: {F} frames of {W} x {H}")
    a, b = a.contiguous(), b.contiguous()
    lib = _lib.lib()
    need = int(lib.nvo_m2d_color_scratch_bytes(F, H, W))
    if need == 0:
        raise ValueError(f"color_accumulators: {F} frames of {W} x {H} are more than one launch takes (3*H*W < 2^30, 3*F <= 65535, "
                         f"3*F*tiles <= 2^24 with tiles of {TILE_W} x {TILE_H})")
    with torch.cuda.device(device):
        table = torch.empty(F, 3, _lib.M2D_COLOR_WORDS, dtype=torch.int64, device=device)
        scratch = torch.empty(need // 8, dtype=torch.int64, device=device)
        args = _lib.M2dColorArgs(a=a.data_ptr(), b=b.data_ptr(), table=table.data_ptr(), scratch=scratch.data_ptr(), F=F, H=H, W=W,
                                 is_float=is_float, taps=(C.c_float * _lib.M2D_TAPS)(*gaussian_taps().tolist()))
        _lib.check(lib.nvo_m2d_color(_stream(device), C.byref(args)), "m2d_color")
    return table


def _psnr_of_sums(sums, n_pixels: int) -> float:
    """``calculate_psnr_reference`` / ``calculate_psnr_float`` from the three channels' integer sums: numpy's mean of
    integers is their exact sum over the count, which is what ``int / int`` gives."""
    vals = []
    for s in sums:
        mse = int(s) / n_pixels
        vals.append(float("inf") if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse)))
    return sum(vals) / 3.0


def mssim_of_sums(sums, n_pixels: int) -> float:
    """The frame's mean SSIM from the three channels' fixed-point sums (one correctly rounded division of integers)."""
    return sum(int(s) for s in sums) / (4294967296 * 3 * n_pixels)


def color_metrics(gt: torch.Tensor, pred: torch.Tensor, float_psnr: bool = False, lpips=None):
    """``calculate_color_metrics_2d`` of uint8 frames on the device: ``{"psnr", "mssim"}`` for one [H, W, 3] pair, a list
    of such dicts for a batch [F, H, W, 3].  ``float_psnr``: also ``"psnr_float"``, the conventional PSNR of
    ``calculate_psnr_float``.  ``lpips``: a ``nerf_vo_amd.lpips.LPIPS`` model; its ``lpips_uint8`` of the same batch is
    added as ``"lpips"``."""
    single = gt.ndim == 3
    if single:
        gt, pred = gt[None], pred[None]
    if gt.dtype != torch.uint8:
        raise ValueError(f"color_metrics: uint8 [H,W,3] or [F,H,W,3] frames, got {gt.dtype}")
    table = color_accumulators(gt, pred).cpu().tolist()
    n = int(gt.shape[1]) * int(gt.shape[2])
    distances = lpips.lpips_uint8(gt, pred) if lpips is not None else None
    rows = []
    for k, frame in enumerate(table):
        row = {"psnr": _psnr_of_sums([ch[0] for ch in frame], n), "mssim": mssim_of_sums([ch[2] for ch in frame], n)}
        if float_psnr:
            row["psnr_float"] = _psnr_of_sums([ch[1] for ch in frame], n)
        if distances is not None:
            row["lpips"] = distances[k]
        rows.append(row)
    return rows[0] if single else rows


def mssim(image1: torch.Tensor, image2: torch.Tensor):
    """``calculate_mssim`` of float [F, 3, H, W] images on the device: a float for F = 1 (that function's contract), a
    list of floats for a batch."""
    if image1.ndim != 4:
        raise ValueError(f"mssim: [F,3,H,W] images, got {tuple(image1.shape)}")
    table = color_accumulators(image1.float(), image2.float()).cpu().tolist()
    n = int(image1.shape[2]) * int(image1.shape[3])
    vals = [mssim_of_sums([ch[2] for ch in frame], n) for frame in table]
    return vals[0] if len(vals) == 1 else vals


def depth_accumulators(gt: torch.Tensor, pred: torch.Tensor, with_scale: bool = True) -> torch.Tensor:
    """int64 [F, 9] on the device: words 0..4 are the BITS of the float64 sums of diff/pred, diff, diff^2/pred, diff^2 and
    (log pred - log gt)^2 over the valid pixels, word 5 their number, words 6..8 the counts of the three delta thresholds.
    ``gt``, ``pred``: [F, H, W], float32 or float64 each."""
    device = _on_gpu("depth_accumulators", gt, pred)
    if gt.ndim != 3 or gt.dtype not in (torch.float32, torch.float64) or pred.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"depth_accumulators: float32 or float64 [F,H,W] depths, got {gt.dtype} / {pred.dtype} {tuple(gt.shape)}")
    F, H, W = (int(v) for v in gt.shape)
    if min(F, H, W) < 1 or max(F, H, W) >= 2 ** 32:
        raise ValueError(f"depth_accumulators: {F} frames of {W} x {H}")
    gt, pred = gt.contiguous(), pred.contiguous()
    lib = _lib.lib()
    need = int(lib.nvo_m2d_depth_scratch_bytes(F, H, W))
    if need == 0:
        raise ValueError(f"depth_accumulators: {F} frames of {W} x {H}: at most 65535 frames of fewer than 2^31 pixels per launch")
    with torch.cuda.device(device):
        table = torch.empty(F, _lib.M2D_DEPTH_WORDS, dtype=torch.int64, device=device)
        scratch = torch.empty(need // 8, dtype=torch.float64, device=device)
        args = _lib.M2dDepthArgs(gt=gt.data_ptr(), pred=pred.data_ptr(), table=table.data_ptr(), scratch=scratch.data_ptr(), F=F, H=H,
                                 W=W, gt_f64=int(gt.dtype == torch.float64), pred_f64=int(pred.dtype == torch.float64),
                                 with_scale=int(bool(with_scale)))
        _lib.check(lib.nvo_m2d_depth(_stream(device), C.byref(args)), "m2d_depth")
    return table


def depth_metrics_of_table(table: np.ndarray) -> list:
    """The rows of ``calculate_depth_metrics_2d`` from a host copy of ``depth_accumulators``' table (means and roots with
    that function's expressions; no valid pixel: NaN everywhere, numpy's mean of nothing)."""
    table = np.ascontiguousarray(table, dtype=np.int64)
    sums, counts = table[:, :5].copy().view(np.float64), table[:, 5:]
    rows = []
    for s, c in zip(sums, counts):
        n = np.float64(c[0])
        with np.errstate(invalid="ignore", divide="ignore"):
            rows.append({
                "absolute_relative": s[0] / n,
                "absolute_difference": s[1] / n,
                "square_relative": s[2] / n,
                "square_difference": np.sqrt(s[3] / n),
                "square_log_difference": np.sqrt(s[4] / n),
                "delta1": np.float64(c[1]) / n,
                "delta2": np.float64(c[2]) / n,
                "delta3": np.float64(c[3]) / n,
            })
    return rows


def depth_metrics(gt: torch.Tensor, pred: torch.Tensor, with_scale: bool = True):
    """``calculate_depth_metrics_2d`` of depth maps on the device: its dict for one [H, W] pair, a list of dicts for a
    batch [F, H, W]."""
    single = gt.ndim == 2
    if single:
        gt, pred = gt[None], pred[None]
    rows = depth_metrics_of_table(depth_accumulators(gt, pred, with_scale).cpu().numpy())
    return rows[0] if single else rows
