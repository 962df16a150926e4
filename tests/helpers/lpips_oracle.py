"""The LPIPS rule of DESIGN.md section 17 on the CPU, restated with torch.nn.functional -- the reference the GPU kernels
(csrc/lpips.hip) are held against.  Two modes:

* ``float64``: every stage in float64 from the float32 image and the float32 weights.
* ``chain``: float32 throughout, every convolution accumulating SEQUENTIALLY over k (unfold, then
  ``acc = acc + w[:, k] * col[k]`` in numpy float32, bias last) and the head's sums sequentially over the channels: the
  least favourable common fp32 order.  Its distance from the float64 mode is the yardstick of the GPU bounds
  (helpers/lpips_cases.py records it).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as TF

LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
TORCHVISION_INDEX = (0, 3, 6, 8, 10)
SHIFT = np.float32([-0.030, -0.088, -0.188])
SCALE = np.float32([0.458, 0.448, 0.450])


def image_of_uint8(u8: np.ndarray) -> torch.Tensor:
    """uint8 [F, H, W, 3] -> the float32 [F, 3, H, W] tensor the reference feeds LPIPS: ``float().div(255) * 2 - 1``, then
    ``* 2 - 1`` once more, one float32 rounding per operation."""
    t = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2))).float().div(255.0) * 2 - 1
    return t * 2 - 1


def scaling_layer(x: torch.Tensor, dtype) -> torch.Tensor:
    shift = torch.from_numpy(SHIFT).to(dtype).view(1, 3, 1, 1)
    scale = torch.from_numpy(SCALE).to(dtype).view(1, 3, 1, 1)
    return (x.to(dtype) - shift) / scale


def conv_relu_float64(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    return TF.relu(TF.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))


def conv_relu_chain(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    F, _, H, W = x.shape
    cout, _, k, _ = w.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = TF.unfold(x.float(), k, padding=pad, stride=stride).numpy()  # [F, K, L], k = (ci * k + ky) * k + kx
    wk = w.float().reshape(cout, -1).numpy()
    acc = np.zeros((F, cout, cols.shape[2]), np.float32)
    for kk in range(cols.shape[1]):
        acc = acc + wk[None, :, kk, None] * cols[:, None, kk, :]
    acc = acc + b.float().numpy()[None, :, None]
    return torch.from_numpy(np.maximum(acc, np.float32(0))).view(F, cout, ho, wo)


def features(x: torch.Tensor, sd: dict, mode: str = "float64") -> list:
    """f1..f5 of a float32 [F, 3, H, W] image; ``sd``: a state dict with torchvision's key names."""
    conv = conv_relu_float64 if mode == "float64" else conv_relu_chain
    dtype = torch.float64 if mode == "float64" else torch.float32
    x, maps = scaling_layer(x, dtype), []
    for l, ((_, _, _, stride, pad), pool) in enumerate(zip(LAYERS, POOL_BEFORE)):
        if pool:
            x = TF.max_pool2d(x, 3, 2)
        i = TORCHVISION_INDEX[l]
        x = conv(x, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], stride, pad)
        maps.append(x)
    return maps


def head_map(f0: torch.Tensor, f1: torch.Tensor, lin: torch.Tensor, mode: str = "float64") -> torch.Tensor:
    """The distance map d [F, H, W] of one layer."""
    if mode == "float64":
        a, b, w = f0.double(), f1.double(), lin.double().reshape(1, -1, 1, 1)
        n0 = a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        n1 = b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        return (w * (a / n0 - b / n1) ** 2).sum(1)
    a, b, w = f0.float().numpy(), f1.float().numpy(), lin.float().reshape(-1).numpy()
    s0, s1 = np.zeros_like(a[:, 0]), np.zeros_like(a[:, 0])
    for c in range(a.shape[1]):
        s0 = s0 + a[:, c] * a[:, c]
        s1 = s1 + b[:, c] * b[:, c]
    n0, n1 = np.sqrt(s0) + np.float32(1e-10), np.sqrt(s1) + np.float32(1e-10)
    d = np.zeros_like(s0)
    for c in range(a.shape[1]):
        e = a[:, c] / n0 - b[:, c] / n1
        d = d + w[c] * (e * e)
    return torch.from_numpy(d)


def lpips(x0: torch.Tensor, x1: torch.Tensor, sd: dict, mode: str = "float64") -> dict:
    """``{"features": [(f0_l, f1_l)], "maps": [d_l], "value": [F]}``: the five layers' maps and the sum of their means."""
    f0, f1 = features(x0, sd, mode), features(x1, sd, mode)
    maps = [head_map(a, b, sd[f"lin{l}.model.1.weight"], mode) for l, (a, b) in enumerate(zip(f0, f1))]
    value = sum(m.double().mean(dim=(1, 2)) for m in maps)
    return {"features": list(zip(f0, f1)), "maps": maps, "value": value}


def tree_mean(d: np.ndarray, block: int = 256) -> np.float32:
    """The kernel's fixed-order mean of one frame's distance map: float64, chunks of ``block`` pixels (0 past the end)
    folded as a binary tree (v[t] += v[t + s], s = block / 2 .. 1), the chunks added in ascending order, one division,
    rounded to float32."""
    v = np.asarray(d, np.float32).reshape(-1).astype(np.float64)
    n = v.size
    g = -(-n // block)
    buf = np.zeros(g * block, np.float64)
    buf[:n] = v
    buf = buf.reshape(g, block)
    s = block // 2
    while s >= 1:
        buf[:, :s] = buf[:, :s] + buf[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for k in range(g):
        total = total + buf[k, 0]
    return np.float32(total / np.float64(n))
