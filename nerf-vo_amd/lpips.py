"""LPIPS v0.1 with AlexNet features on the GPU (csrc/lpips.hip, include/nerfvo_hip.h section O):
the ``lpips`` column of the reference's 2-D table, which it takes from ``lpips.LPIPS(net='alex')``.

The network is restated here, not copied: five convolutions of AlexNet with ReLU, two max-pools, and per layer a
channel-normalise / difference / 1x1 head whose spatial means are added.  The weights are NOT shipped and never fetched:
a user who has the two files (torchvision's AlexNet and the package's linear layers) passes them to
``LPIPS.from_files``.  The key names accepted below are written from memory of those two packages -- neither is
installed where this was developed -- so parity with the package on the real weights is unpinned.

Every stage is a HIP kernel with fp32 operands and fp32 accumulation; there is no CPU fallback and no eager-torch path.
A frame's value is bitwise the same alone or in a batch and from run to run.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

# (Cin, Cout, kernel, stride, pad) of conv1..conv5; a max-pool precedes conv2 and conv3
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
TORCHVISION_INDEX = (0, 3, 6, 8, 10)
DEFAULT_SHIFT = (-0.030, -0.088, -0.188)
DEFAULT_SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 31


def conv_out(n: int, ksize: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - ksize) // stride + 1


def pool_out(n: int) -> int:
    return (n - 3) // 2 + 1


def feature_sizes(H: int, W: int) -> list:
    """(Ho, Wo) of f1..f5 for an H x W frame."""
    if min(H, W) < MIN_SIZE:
        raise ValueError(f"LPIPS: a {W} x {H} frame is too small: the second max-pool needs a 3 x 3 map, so width and height "
                         f"must be at least {MIN_SIZE}; pad or resize the frame")
    sizes, h, w = [], H, W
    for (_, _, k, s, p), pool in zip(LAYERS, POOL_BEFORE):
        if pool:
            h, w = pool_out(h), pool_out(w)
        h, w = conv_out(h, k, s, p), conv_out(w, k, s, p)
        sizes.append((h, w))
    return sizes


def check_sizes(F: int, H: int, W: int) -> None:
    """Refuse a batch whose largest launch would pass the launchers' index range."""
    sizes = feature_sizes(H, W)
    if F < 1:
        raise ValueError("LPIPS: an empty batch")
    if F > 65535 or F * sizes[0][0] * sizes[0][1] >= 2 ** 31 or F * 3 * H * W >= 2 ** 40:
        raise ValueError(f"LPIPS: {F} frames of {W} x {H} are more than one launch takes (F <= 65535, F * Ho * Wo < 2^31 for "
                         f"conv1's {sizes[0][1]} x {sizes[0][0]} map); pass fewer frames per call")


def synthetic_weights(seed: int = 0) -> dict:
    """A state dict of the right shapes with random values -- for tests and benchmarks, NOT LPIPS: He-scaled normal
    convolution weights, biases 0.1 * normal, non-negative head weights uniform / C.  (numpy's PCG64, so the values do
    not depend on the torch build.)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        fan_in = cin * k * k
        sd[f"features.{TORCHVISION_INDEX[l]}.weight"] = torch.from_numpy(
            (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / fan_in)).astype(np.float32))
        sd[f"features.{TORCHVISION_INDEX[l]}.bias"] = torch.from_numpy((0.1 * rng.standard_normal(cout)).astype(np.float32))
    for l, (_, cout, _, _, _) in enumerate(LAYERS):
        sd[f"lin{l}.model.1.weight"] = torch.from_numpy((rng.random((1, cout, 1, 1)) / cout).astype(np.float32))
    return sd


def _stream(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_gpu(what: str, *tensors) -> torch.device:
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: the tensors must be on the GPU -- there is no CPU fallback (move them with .cuda(), or "
                               "call the model itself, which uploads host images)")
    for t in tensors[1:]:
        if t.device != tensors[0].device:
            raise ValueError(f"{what}: all tensors must be on one device, got {tensors[0].device} and {t.device}")
    return tensors[0].device


def _need_f32(what: str, t: torch.Tensor, ndim: int, layout: str) -> None:
    if t.dtype != torch.float32 or t.ndim != ndim:
        raise ValueError(f"{what}: a float32 {layout} tensor, got {t.dtype} {tuple(t.shape)}; convert with .float()")


def pack_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, k, k] -> the kernel's k-major [Kpad, Cout] with zero rows past K = Cin * k * k."""
    cout, K = int(weight.shape[0]), int(weight[0].numel())
    kpad = -(-K // _lib.LPIPS_TILE_K) * _lib.LPIPS_TILE_K
    packed = torch.zeros(kpad, cout, dtype=torch.float32, device=weight.device)
    packed[:K] = weight.reshape(cout, K).t()
    return packed


def _conv(x, packed, bias, cin, cout, ksize, stride, pad, ingest=0, shift=DEFAULT_SHIFT, scale=DEFAULT_SCALE):
    device = x.device
    if ingest == 2:
        F, H, W = (int(v) for v in x.shape[:3])
    else:
        F, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    Ho, Wo = conv_out(H, ksize, stride, pad), conv_out(W, ksize, stride, pad)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"conv2d_relu: a {W} x {H} map is smaller than the {ksize}-tap kernel with padding {pad}")
    if F * Ho * Wo >= 2 ** 31:
        raise ValueError(f"conv2d_relu: {F} maps of {Wo} x {Ho} output pixels are more than one launch takes (F * Ho * Wo < 2^31); "
                         "pass fewer frames per call")
    x = x.contiguous()
    lib = _lib.lib()
    with torch.cuda.device(device):
        out = torch.empty(F, cout, Ho, Wo, dtype=torch.float32, device=device)
        args = _lib.LpipsConvArgs(x=x.data_ptr(), weights=packed.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(), F=F, Cin=cin,
                                  H=H, W=W, Cout=cout, ksize=ksize, stride=stride, pad=pad, Kpad=int(packed.shape[0]), ingest=ingest,
                                  shift=(C.c_float * 3)(*shift), scale=(C.c_float * 3)(*scale))
        _lib.check(lib.nvo_lpips_conv(_stream(device), C.byref(args)), "lpips_conv")
    return out


def conv2d_relu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """``relu(conv2d(x, weight, bias, stride, pad))`` of NCHW float32 tensors on the GPU, with AlexNet's three kernels
    (11 x 11 stride 4, 5 x 5 stride 1, 3 x 3 stride 1) and a multiple of 64 output channels."""
    device = _need_gpu("conv2d_relu", x, weight, bias)
    _need_f32("conv2d_relu", x, 4, "[F,C,H,W]")
    _need_f32("conv2d_relu", weight, 4, "[Cout,Cin,k,k]")
    _need_f32("conv2d_relu", bias, 1, "[Cout]")
    cout, cin, k, k2 = (int(v) for v in weight.shape)
    if k != k2 or int(x.shape[1]) != cin or int(bias.shape[0]) != cout:
        raise ValueError(f"conv2d_relu: x {tuple(x.shape)}, weight {tuple(weight.shape)} and bias {tuple(bias.shape)} do not fit together")
    if (k, int(stride)) not in ((11, 4), (5, 1), (3, 1)) or cout % _lib.LPIPS_TILE_M or not 0 <= int(pad) < k:
        raise ValueError(f"conv2d_relu: kernel {k} stride {stride} pad {pad} with {cout} output channels has no kernel instance "
                         f"(11/4, 5/1 or 3/1, pad < kernel, a multiple of {_lib.LPIPS_TILE_M} channels)")
    with torch.cuda.device(device):
        return _conv(x, pack_weight(weight), bias.contiguous(), cin, cout, k, int(stride), int(pad))


def maxpool_3x3_s2(x: torch.Tensor) -> torch.Tensor:
    """``max_pool2d(x, 3, 2)`` of an NCHW float32 tensor on the GPU."""
    device = _need_gpu("maxpool_3x3_s2", x)
    _need_f32("maxpool_3x3_s2", x, 4, "[F,C,H,W]")
    F, Cn, H, W = (int(v) for v in x.shape)
    if min(H, W) < 3 or F * Cn < 1:
        raise ValueError(f"maxpool_3x3_s2: a {W} x {H} map is smaller than the 3 x 3 window")
    if F * Cn >= 2 ** 32 or F * Cn * H * W >= 2 ** 39:
        raise ValueError(f"maxpool_3x3_s2: {F * Cn} planes of {W} x {H} are more than one launch takes; pass fewer frames per call")
    x = x.contiguous()
    with torch.cuda.device(device):
        out = torch.empty(F, Cn, pool_out(H), pool_out(W), dtype=torch.float32, device=device)
        args = _lib.LpipsPoolArgs(x=x.data_ptr(), out=out.data_ptr(), planes=F * Cn, H=H, W=W)
        _lib.check(_lib.lib().nvo_lpips_pool(_stream(device), C.byref(args)), "lpips_pool")
    return out


def _head(f0, f1, lin, out, accumulate, want_map):
    device = f0.device
    F, Cn, HW = int(f0.shape[0]), int(f0.shape[1]), int(f0.shape[2]) * int(f0.shape[3])
    lib = _lib.lib()
    need = int(lib.nvo_lpips_head_scratch_bytes(F, Cn, HW))
    if need == 0:
        raise ValueError(f"head: {F} maps of {Cn} x {HW} values are more than one launch takes (F <= 65535, F * C * H * W < 2^40); "
                         "pass fewer frames per call")
    with torch.cuda.device(device):
        scratch = torch.empty(need // 8, dtype=torch.float64, device=device)
        dmap = torch.empty(F, 1, int(f0.shape[2]), int(f0.shape[3]), dtype=torch.float32, device=device) if want_map else None
        args = _lib.LpipsHeadArgs(f0=f0.data_ptr(), f1=f1.data_ptr(), lin=lin.data_ptr(), map=dmap.data_ptr() if want_map else None,
                                  scratch=scratch.data_ptr(), out=out.data_ptr(), F=F, C=Cn, HW=HW, accumulate=int(accumulate))
        _lib.check(lib.nvo_lpips_head(_stream(device), C.byref(args)), "lpips_head")
    return dmap


def head(f0: torch.Tensor, f1: torch.Tensor, lin: torch.Tensor, want: str = "mean") -> torch.Tensor:
    """One layer of the head on NCHW float32 feature maps on the GPU.  ``lin``: [C] (or the file's [1, C, 1, 1]).
    ``want='map'``: the distance map d, [F, 1, H, W]; ``'mean'``: its spatial mean, [F, 1, 1, 1]."""
    if want not in ("mean", "map"):
        raise ValueError(f"head: want is 'mean' or 'map', got {want!r}")
    device = _need_gpu("head", f0, f1, lin)
    _need_f32("head", f0, 4, "[F,C,H,W]")
    _need_f32("head", f1, 4, "[F,C,H,W]")
    if f0.shape != f1.shape or lin.dtype != torch.float32 or lin.numel() != f0.shape[1] or f0.numel() == 0:
        raise ValueError(f"head: two maps of one shape and C head weights, got {tuple(f0.shape)}, {tuple(f1.shape)} and "
                         f"{lin.dtype} {tuple(lin.shape)}")
    with torch.cuda.device(device):
        out = torch.empty(int(f0.shape[0]), dtype=torch.float32, device=device)
        dmap = _head(f0.contiguous(), f1.contiguous(), lin.reshape(-1).contiguous(), out, False, want == "map")
    return dmap if want == "map" else out.view(-1, 1, 1, 1)


def _resolve(sd: dict) -> tuple:
    """(host tensors by our names, problems) from a state dict of either key set."""
    want, problems = {}, []

    def take(name, candidates, shape):
        found = [k for k in candidates if k in sd]
        if not found:
            problems.append(f"missing {' or '.join(candidates)} {list(shape)}")
            return
        t = sd[found[0]]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or not t.dtype.is_floating_point:
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            problems.append(f"{found[0]}: expected a float tensor {list(shape)}, got {got}")
            return
        want[name] = t.detach().to("cpu", torch.float32).contiguous()

    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        i = TORCHVISION_INDEX[l]
        for part, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            take(f"conv{l}.{part}", (f"features.{i}.{part}", f"net.slice{l + 1}.{i}.{part}"), shape)
        take(f"lin{l}", (f"lin{l}.model.1.weight", f"lins.{l}.model.1.weight"), (1, cout, 1, 1))
    for name in ("shift", "scale"):
        if f"scaling_layer.{name}" in sd:
            take(name, (f"scaling_layer.{name}",), (1, 3, 1, 1))
    return want, problems


class LPIPS:
    """``lpips.LPIPS(net='alex')`` (v0.1, linear layers on, ``spatial=False``, ``normalize=False``) with every stage in HIP.

    ``state_dict`` holds the five convolutions and the five linear layers under either of these key sets (written from
    memory of the two packages, neither of which is installed where this was developed):

    * torchvision's AlexNet: ``features.{0,3,6,8,10}.{weight,bias}``
    * the package's own: ``net.slice1.0.*``, ``net.slice2.3.*``, ``net.slice3.6.*``, ``net.slice4.8.*``, ``net.slice5.10.*``
    * the head: ``lin{0..4}.model.1.weight`` [1, C, 1, 1], also as ``lins.{0..4}.model.1.weight``
    * optionally ``scaling_layer.shift`` / ``scaling_layer.scale`` [1, 3, 1, 1]; otherwise the v0.1 constants

    Other keys (AlexNet's classifier) are ignored.  ``device`` is a CUDA device: host images given to the model are uploaded
    to it; device images are processed where they are."""

    def __init__(self, state_dict: dict, device="cuda") -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"LPIPS: device must be a CUDA device, got {device!r} -- the network has no CPU path")
        host, problems = _resolve(dict(state_dict))
        if problems:
            raise ValueError("LPIPS: the state dict is not AlexNet + LPIPS v0.1 linear layers:\n  " + "\n  ".join(problems))
        self.shift = tuple(float(v) for v in host["shift"].reshape(-1)) if "shift" in host else tuple(np.float32(DEFAULT_SHIFT).tolist())
        self.scale = tuple(float(v) for v in host["scale"].reshape(-1)) if "scale" in host else tuple(np.float32(DEFAULT_SCALE).tolist())
        self.weights = {k: v for k, v in host.items() if k not in ("shift", "scale")}  # host copies, our names
        self._packed = {l: pack_weight(host[f"conv{l}.weight"]) for l in range(len(LAYERS))}  # once per model
        self._on_device = {}

    @classmethod
    def from_files(cls, *paths, device="cuda") -> "LPIPS":
        """The model from one or more weight files (``torch.load(..., weights_only=True, map_location='cpu')``, merged in
        the order given).  Nothing is ever fetched: a missing file is an error."""
        if not paths:
            raise ValueError("LPIPS.from_files: give the AlexNet file and the linear-layer file (or one file that holds both)")
        merged = {}
        for path in paths:
            sd = torch.load(path, weights_only=True, map_location="cpu")
            if not isinstance(sd, dict):
                raise ValueError(f"LPIPS.from_files: {path} holds a {type(sd).__name__}, not a state dict")
            merged.update(sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd)
        return cls(merged, device=device)

    def _params(self, device: torch.device) -> dict:
        if device not in self._on_device:
            p = {}
            for l in range(len(LAYERS)):
                p[f"w{l}"] = self._packed[l].to(device)
                p[f"b{l}"] = self.weights[f"conv{l}.bias"].to(device)
                p[f"lin{l}"] = self.weights[f"lin{l}"].reshape(-1).contiguous().to(device)
            self._on_device[device] = p
        return self._on_device[device]

    def _features(self, x: torch.Tensor, ingest: int) -> list:
        p, maps = self._params(x.device), []
        for l, ((cin, cout, k, s, pad), pool) in enumerate(zip(LAYERS, POOL_BEFORE)):
            if pool:
                x = maxpool_3x3_s2(x)
            x = _conv(x, p[f"w{l}"], p[f"b{l}"], cin, cout, k, s, pad, ingest if l == 0 else 0, self.shift, self.scale)
            maps.append(x)
        return maps

    def features(self, x: torch.Tensor) -> list:
        """f1..f5 of a float32 [F, 3, H, W] image on the GPU (the scaling layer included)."""
        _need_gpu("LPIPS.features", x)
        F, H, W = self._check_float("LPIPS.features", x)
        check_sizes(F, H, W)
        return self._features(x, 1)

    @staticmethod
    def _check_float(what: str, x) -> tuple:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim != 4 or x.shape[1] != 3:
            got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"{what}: a float32 [F,3,H,W] image, got {got}; convert with .float() and add the batch axis")
        return int(x.shape[0]), int(x.shape[2]), int(x.shape[3])

    def _distance(self, x0: torch.Tensor, x1: torch.Tensor, ingest: int) -> torch.Tensor:
        device = x0.device
        f0, f1 = self._features(x0, ingest), self._features(x1, ingest)
        p = self._params(device)
        with torch.cuda.device(device):
            out = torch.empty(int(x0.shape[0]), dtype=torch.float32, device=device)
            for l in range(len(LAYERS)):
                _head(f0[l], f1[l], p[f"lin{l}"], out, l > 0, False)
        return out

    def __call__(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """float32 [F, 3, H, W] images on any device -> float32 [F, 1, 1, 1] on the images' device (the package's contract)."""
        F, H, W = self._check_float("LPIPS", x0)
        self._check_float("LPIPS", x1)
        if x0.shape != x1.shape or x0.device != x1.device:
            raise ValueError(f"LPIPS: the two images must have one shape and one device, got {tuple(x0.shape)} on {x0.device} and "
                             f"{tuple(x1.shape)} on {x1.device}")
        check_sizes(F, H, W)
        home = x0.device
        with torch.no_grad():
            if not x0.is_cuda:
                x0, x1 = x0.to(self.device), x1.to(self.device)
            return self._distance(x0.contiguous(), x1.contiguous(), 1).to(home).view(F, 1, 1, 1)

    def lpips_uint8(self, gt: torch.Tensor, pred: torch.Tensor) -> list:
        """uint8 [F, H, W, 3] frames on the GPU -> a list of Python floats: what the model gives for the tensors the
        reference builds from them, ``((u / 255) * 2 - 1) * 2 - 1``, bit for bit; the conversion happens inside the first
        convolution's load and no float image is made."""
        _need_gpu("LPIPS.lpips_uint8", gt, pred)
        for t in (gt, pred):
            if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3:
                raise ValueError(f"LPIPS.lpips_uint8: uint8 [F,H,W,3] frames, got {t.dtype} {tuple(t.shape)}")
        if gt.shape != pred.shape:
            raise ValueError(f"LPIPS.lpips_uint8: the two frames must have one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
        check_sizes(int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2]))
        with torch.no_grad():
            return self._distance(gt.contiguous(), pred.contiguous(), 2).cpu().tolist()
