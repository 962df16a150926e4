"""numpy restatement of the colour rule of csrc/metrics2d.hip (include/nerfvo_hip.h section N),
operation for operation: every float32 product, sum, difference and quotient below is ONE numpy float32 operation, in the
kernel's order, so the integers that come out are the kernel's integers.

    x = (float(u) / 255) * 2 - 1                                   (uint8 form)
    planes a, b, a*a, b*b, a*b
    row pass, then column pass: acc = 0; for t = 0..10: acc = acc + g[t] * v[. + t - 5], the image zero outside
        (a tap outside adds g[t] * 0 = +0, which leaves acc as it is: the tap is skipped)
    maa = ma*ma, mbb = mb*mb, mab = ma*mb; va = saa - maa, vb = sbb - mbb, cab = sab - mab
    s = ((2 mab + C1) * (2 cab + C2)) / (((maa + mbb) + C1) * ((va + vb) + C2))
    per channel: sum of rint(float64(s) * 2^32) as int64;  frame: the three sums / (2^32 * 3 H W)
"""
import math

import numpy as np

TAPS = 11
F32 = np.float32


def gaussian_taps() -> np.ndarray:
    x = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-(x ** 2) / 4.5)
    return (g / g.sum()).astype(np.float32)


def to_signed(image_u8: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3] -> float32 [3, H, W] in [-1, 1]: torch's ``.float().div(255.0) * 2 - 1`` bit for bit."""
    x = np.ascontiguousarray(image_u8.transpose(2, 0, 1)).astype(np.float32)
    return (x / F32(255.0)) * F32(2.0) - F32(1.0)


def _pass(p: np.ndarray, g: np.ndarray, axis: int) -> np.ndarray:
    n = p.shape[axis]
    acc = np.zeros_like(p)
    for t in range(TAPS):
        d = t - TAPS // 2
        src = np.zeros_like(p)
        lo, hi = max(0, -d), min(n, n - d)
        if hi > lo:
            dst_sl, src_sl = [slice(None)] * p.ndim, [slice(None)] * p.ndim
            dst_sl[axis], src_sl[axis] = slice(lo, hi), slice(lo + d, hi + d)
            src[tuple(dst_sl)] = p[tuple(src_sl)]
        acc = acc + g[t] * src
    assert acc.dtype == np.float32
    return acc


def blur(p: np.ndarray, g: np.ndarray) -> np.ndarray:
    return _pass(_pass(p, g, axis=2), g, axis=1)


def ssim_map(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float32 [3, H, W] images -> the float32 SSIM map [3, H, W]."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    g = gaussian_taps()
    ma, mb = blur(a, g), blur(b, g)
    saa, sbb, sab = blur(a * a, g), blur(b * b, g), blur(a * b, g)
    maa, mbb, mab = ma * ma, mb * mb, ma * mb
    va, vb, cab = saa - maa, sbb - mbb, sab - mab
    c1, c2 = F32(0.01 ** 2), F32(0.03 ** 2)
    s = ((F32(2.0) * mab + c1) * (F32(2.0) * cab + c2)) / (((maa + mbb) + c1) * ((va + vb) + c2))
    assert s.dtype == np.float32
    return s


def ssim_fixed(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """int64 [3]: per channel, the sum of rint(float64(s) * 2^32)."""
    s = ssim_map(a, b)
    return np.rint(s.astype(np.float64) * 4294967296.0).astype(np.int64).reshape(3, -1).sum(axis=1)


def mssim_of_sums(sums, n_pixels: int) -> float:
    return sum(int(v) for v in sums) / (4294967296 * 3 * n_pixels)


def mssim(a: np.ndarray, b: np.ndarray) -> float:
    """Mean SSIM of two float32 [3, H, W] (or [1, 3, H, W]) images by the kernel's rule."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 4:
        a, b = a[0], b[0]
    return mssim_of_sums(ssim_fixed(a, b), a.shape[1] * a.shape[2])


def color_accumulators_u8(a_u8: np.ndarray, b_u8: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3] pair -> int64 [3, 3]: per channel (wrapping square sum, true square sum, fixed-point SSIM sum)."""
    out = np.zeros((3, 3), dtype=np.int64)
    with np.errstate(over="ignore"):
        d = (a_u8 - b_u8).astype(np.uint8)
        wrap = (d * d).astype(np.uint8)
    true = (a_u8.astype(np.int64) - b_u8.astype(np.int64)) ** 2
    out[:, 0] = wrap.astype(np.int64).reshape(-1, 3).sum(axis=0)
    out[:, 1] = true.reshape(-1, 3).sum(axis=0)
    out[:, 2] = ssim_fixed(to_signed(a_u8), to_signed(b_u8))
    return out


def color_accumulators_f32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float32 [3, H, W] pair -> int64 [3, 3]; the two square sums are not produced in this form (0)."""
    out = np.zeros((3, 3), dtype=np.int64)
    out[:, 2] = ssim_fixed(a, b)
    return out


def psnr_of_sums(sums, n_pixels: int) -> float:
    vals = []
    for s in sums:
        mse = int(s) / n_pixels
        vals.append(float("inf") if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse)))
    return sum(vals) / 3.0
