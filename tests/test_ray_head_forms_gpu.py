"""The two forms of the ray head (csrc/rays.hip): k_ray_head_x4 -- four samples per thread, 16-byte stores, taken when
S % 4 == 0 and the x01 / SH bases are 16-byte aligned -- and the thread-per-sample k_ray_head for every other shape.  Both
must reproduce the five separate launches (pixel sampler, ray generation, target gather, SH, first sampler level) BIT FOR
BIT on every output, write nothing outside their outputs, and clear exactly the ranges of the zero plan.  Every output
buffer carries 64 sentinel elements behind its last row."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F, H, W = 7, 48, 64
SEED = 0xC0FFEE
PAD = 64  # sentinel elements behind every output
SENT = -7
CONFIGS = {"4x4-fixed-f16": (16, False, 0), "3x4-corrected-bf16": (12, True, 1)}

_SCENE = {}


def _scene(device):
    """Cameras, poses, corrections and frames shared by every test of this file (read-only)."""
    if not _SCENE:
        g = torch.Generator().manual_seed(9)
        dev = lambda t: t.to(device).contiguous()  # noqa: E731
        intr = dev(torch.tensor([[30.0, 28.0, 31.7, 23.6]]).repeat(F, 1) + torch.rand(F, 4, generator=g))
        rot = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0]
        c2w44 = torch.eye(4).repeat(F, 1, 1)
        c2w44[:, :3, :3] = rot
        c2w44[:, :3, 3] = torch.randn(F, 3, generator=g) * 0.3
        c2w44 = dev(c2w44)
        corr = dev(torch.cat([torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0], torch.randn(F, 3, 1, generator=g) * 0.05], 2))
        _SCENE.update(intr=intr, c2w44=c2w44, c2w34=c2w44[:, :3, :4].contiguous(), corr=corr,
                      images=dev(torch.rand(F, H, W, 3, generator=g)), depths=dev(torch.rand(F, H, W, generator=g)),
                      normals=dev(torch.rand(F, H, W, 3, generator=g)), step_dev=torch.tensor([37.0], device=device),
                      extent=torch.tensor([float(F - 2), float(H), float(W)], device=device))
    return _SCENE


SHAPES = dict(idx=(3, torch.int64), jit=(None, torch.float32), o=(3, torch.float32), d=(3, torch.float32), dn=(1, torch.float32),
              pa=(1, torch.float32), ci=(1, torch.int32), rgb=(3, torch.float32), dep=(1, torch.float32), nor=(3, torch.float32),
              d01=(3, torch.float32), sh=(16, None), sb=("S+1", torch.float32), tb=("S+1", torch.float32), x=("3S", torch.float32))


class Bufs:
    """Flat output buffers filled with the sentinel, each with PAD sentinel elements behind its last row (and, for x01,
    ``x_offset`` floats in front of it: a base that is 4-byte but not 16-byte aligned)."""

    def __init__(self, device, R, S, adt, x_offset=0):
        self.n, self.flat, self.off = {}, {}, {}
        for k, (cols, dt) in SHAPES.items():
            dt = adt if dt is None else dt
            n = 3 * R if k == "jit" else R * {"S+1": S + 1, "3S": 3 * S}.get(cols, cols)
            off = x_offset if k == "x" else 0
            self.n[k], self.off[k] = n, off
            self.flat[k] = torch.full((off + n + PAD,), SENT, dtype=dt, device=device)

    def ptr(self, k, skip=0):
        t = self.flat[k]
        return C.c_void_p(t.data_ptr() + (self.off[k] + skip) * t.element_size())

    def addr(self, k):
        return self.ptr(k).value

    def body(self, k):
        return self.flat[k][self.off[k]:self.off[k] + self.n[k]]

    def guards_intact(self, k):
        t = self.flat[k]
        return bool((t[:self.off[k]] == SENT).all()) and bool((t[self.off[k] + self.n[k]:] == SENT).all())


def _separate(device, b, R, S, stride, poses, fmt, null=()):
    """The five separate launches into ``b``."""
    from nerf_vo_amd.engine import _call, _ptr, _stream

    sc, st = _scene(device), _stream(device)
    _call("nvo_sample_pixels", st, R, SEED, _ptr(sc["step_dev"]), _ptr(sc["extent"]), b.ptr("idx"), b.ptr("jit"), 3)
    _call("nvo_raygen", st, R, b.ptr("idx"), _ptr(sc["intr"]), _ptr(sc["c2w34"]), _ptr(sc["corr"]) if poses else None, b.ptr("o"),
          b.ptr("d"), b.ptr("dn"), None if "pixel_area" in null else b.ptr("pa"), b.ptr("ci"))
    _call("nvo_gather_targets", st, R, b.ptr("idx"), H, W, _ptr(sc["images"]), None if "depths" in null else _ptr(sc["depths"]),
          None if "normals" in null else _ptr(sc["normals"]), b.ptr("d"), b.ptr("rgb"), b.ptr("dep"), b.ptr("nor"), b.ptr("d01"))
    if "sh" not in null:
        _call("nvo_sh_encode_t", st, R, 4, b.ptr("d01"), b.ptr("sh"), fmt)
    _call("nvo_lindisp_positions", st, R, S, 0.05, 1000.0, b.ptr("jit"), b.ptr("o"), b.ptr("d"), b.ptr("sb"), b.ptr("tb"), b.ptr("x"))


def _head_args(device, b, R, S, stride, poses, fmt, null=()):
    from nerf_vo_amd import _lib

    sc = _scene(device)
    poses_t = sc["c2w34"] if stride == 12 else sc["c2w44"]
    return _lib.RayHeadArgs(
        R=R, S=S, seed=SEED, n_jitter=3, step_dev=sc["step_dev"].data_ptr(), extent_dev=sc["extent"].data_ptr(),
        intrinsics=sc["intr"].data_ptr(), c2w=poses_t.data_ptr(), c2w_stride=stride,
        corrections=sc["corr"].data_ptr() if poses else None, H=H, W=W, images=sc["images"].data_ptr(),
        depths=None if "depths" in null else sc["depths"].data_ptr(),
        normals=None if "normals" in null else sc["normals"].data_ptr(), near_plane=0.05, far_plane=1000.0,
        ray_indices=b.addr("idx"), jitter=b.addr("jit"), origins=b.addr("o"), directions=b.addr("d"),
        directions_norm=b.addr("dn"), pixel_area=None if "pixel_area" in null else b.addr("pa"), cam_idx=b.addr("ci"),
        gt_rgb=b.addr("rgb"), gt_depth=b.addr("dep"), gt_normal=b.addr("nor"), dirs01=b.addr("d01"),
        sh=None if "sh" in null else b.addr("sh"), sh_bf16=fmt, sbins=b.addr("sb"), tbins=b.addr("tb"), x01=b.addr("x"))


def _assert_same(a, b, R, S, what):
    """Raw bytes of every output, the sentinels around them, the closing edges and the last row of x01."""
    for k in SHAPES:
        assert b.guards_intact(k), f"{what}: output '{k}' has a store outside its {b.n[k]} elements"
        x, y = a.body(k), b.body(k)
        if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            bad = (x != y).nonzero().reshape(-1)
            i = int(bad[0])
            raise AssertionError(f"{what}: output '{k}' differs from the separate kernels at {bad.numel()} of {x.numel()} "
                                 f"elements; first flat index {i}: {x[i].item()!r} vs {y[i].item()!r}")
    for k in ("sb", "tb"):
        rows = b.body(k).view(R, S + 1)
        assert bool((rows[:, S] != SENT).all()) and bool((rows[:, 0] != SENT).all()), f"{what}: '{k}' rows not written to their closing edge"
    assert bool((b.body("x").view(R * S, 3)[R * S - 1] != SENT).all()), f"{what}: row R*S-1 of x01 not written"


def _run_pair(device, R, S, cfg, null=(), x_offset=0):
    from nerf_vo_amd.engine import _call, _stream

    stride, poses, fmt = CONFIGS[cfg]
    adt = torch.bfloat16 if fmt else torch.float16
    a, b = Bufs(device, R, S, adt), Bufs(device, R, S, adt, x_offset=x_offset)
    _separate(device, a, R, S, stride, poses, fmt, null)
    ra = _head_args(device, b, R, S, stride, poses, fmt, null)
    _call("nvo_ray_head", _stream(device), C.byref(ra))
    torch.cuda.synchronize()
    assert int(a.body("idx").view(R, 3)[:, 0].max()) <= F - 3 and float(a.body("x").min()) >= 0.0
    _assert_same(a, b, R, S, f"R={R} S={S} {cfg} null={null} x_offset={x_offset}")
    return a, b


@pytest.mark.parametrize("R", [1, 5, 1000, 4099])
@pytest.mark.parametrize("S", [4, 48, 96, 256, 1, 3, 255, 257])
def test_same_bits_as_separate_launches(device, S, R):
    """S = 4, 48, 96, 256: the 4-samples-per-thread form (one group per ray; more rays per workgroup than the
    thread-per-sample form's table holds; rays that straddle workgroups; a ragged last workgroup).  S = 1, 3, 255, 257: the
    thread-per-sample form.  Both pose layouts, with and without corrections, fp16 and bf16 SH."""
    for cfg in CONFIGS:
        _run_pair(device, R, S, cfg)


@pytest.mark.parametrize("null", ["depths", "normals", "pixel_area", "sh"])
@pytest.mark.parametrize("S", [256, 3])
def test_optional_arguments_null(device, S, null):
    """The optional input / output left out: its output keeps the sentinel in both, everything else matches."""
    a, b = _run_pair(device, 1000, S, "3x4-corrected-bf16", null=(null,))
    out = {"depths": "dep", "normals": "nor", "pixel_area": "pa", "sh": "sh"}[null]
    assert bool((b.body(out) == SENT).all())


@pytest.mark.parametrize("S", [256, 48])
def test_unaligned_x01_base(device, S):
    """x01 at a base that is 4-byte but not 16-byte aligned: no 16-byte stores, same bits."""
    a, b = _run_pair(device, 1000, S, "4x4-fixed-f16", x_offset=1)
    assert b.addr("x") % 16 == 4


@pytest.mark.parametrize("S", [256, 3])
@pytest.mark.parametrize("ranges", ["ranges", "empty"])
def test_zero_plan(device, S, ranges):
    """nvo_ray_head_zero: ranges of 4 B, 20 B at a 4-byte-aligned but not 16-byte-aligned address and 1 MB (or no range at
    all), pre-filled with a sentinel between guard words: the ranges end up zero, the guards intact, and the ray outputs
    are those of nvo_ray_head."""
    from nerf_vo_amd.engine import _call, _stream

    R, cfg = 1000, "3x4-corrected-bf16"
    stride, poses, fmt = CONFIGS[cfg]
    st = _stream(device)
    a = Bufs(device, R, S, torch.bfloat16)
    _call("nvo_ray_head", st, C.byref(_head_args(device, a, R, S, stride, poses, fmt)))
    b = Bufs(device, R, S, torch.bfloat16)
    fill = 0x5A5A5A5A
    big = 1 << 18  # words of the 1 MB range
    zb = torch.full((64 + big + 64,), fill, dtype=torch.int32, device=device)
    spans = [(5, 1), (17, 5), (64, big)] if ranges == "ranges" else []
    assert zb.data_ptr() % 16 == 0  # (so word 17 is 4-byte but not 16-byte aligned)
    n = len(spans)
    ptrs = (C.c_void_p * max(n, 1))(*[zb.data_ptr() + 4 * o for o, _ in spans])
    sizes = (C.c_uint64 * max(n, 1))(*[4 * w for _, w in spans])
    _call("nvo_ray_head_zero", st, C.byref(_head_args(device, b, R, S, stride, poses, fmt)), n, ptrs if n else None,
          sizes if n else None)
    torch.cuda.synchronize()
    expect = torch.full_like(zb, fill)
    for o, w in spans:
        expect[o:o + w] = 0
    wrong = (zb != expect).nonzero().reshape(-1)
    assert wrong.numel() == 0, f"zero plan: {wrong.numel()} words wrong, first at word {int(wrong[0])}"
    _assert_same(a, b, R, S, f"nvo_ray_head_zero S={S} {ranges}")


def test_engine_step_same_with_either_form(device, monkeypatch):
    """Two engines from the same seed at 64 rays, one captured with the thread-per-sample form forced
    (NVO_RAY_HEAD_GENERIC=1; a captured graph keeps the form it was captured with) and one with the 4-samples-per-thread
    form; update steps and a plain step on each; the rendered outputs of the first step must be the same bits."""
    from nerf_vo_amd.engine import EngineConfig, NerfactoEngine
    from nerf_vo_amd.mapping.dataset import DynamicDataset, opencv_to_opengl
    from nerf_vo_amd.synthetic import make_sequence

    n, fh, fw, R = 6, 60, 80, 64
    ds = DynamicDataset(num_frames=n, frame_height=fh, frame_width=fw, device=device, use_normals=False)
    seq = make_sequence(n, fh, fw, device=device)
    ds.update({"keyframe_indices": torch.arange(n), "camera_intrinsics": seq["camera_intrinsics"],
               "camera_extrinsics": opencv_to_opengl(seq["camera_extrinsics"]), "frames_color": seq["frames_color"],
               "frames_depth": seq["frames_depth"]})
    names = ("out_rgb", "out_depth", "out_expected_depth", "out_accumulation")

    def run(generic):
        if generic:
            monkeypatch.setenv("NVO_RAY_HEAD_GENERIC", "1")
        else:
            monkeypatch.delenv("NVO_RAY_HEAD_GENERIC", raising=False)
        torch.manual_seed(5)
        eng = NerfactoEngine(EngineConfig(num_images=n, num_rays=R), device)
        assert eng.levels[0] % 4 == 0
        kinds = [bool(eng.train_step_graphed(ds))]
        torch.cuda.synchronize()
        wss = {id(e["ws"]): e["ws"] for e in eng._graphs.values()}
        assert len(wss) == 1  # (every variant of the step at this ray count works in ONE workspace)
        ws = next(iter(wss.values()))
        first = {k: ws[k].clone() for k in names}
        for _ in range(11):  # (the first ten steps all refresh the proposal networks)
            kinds.append(bool(eng.train_step_graphed(ds)))
        torch.cuda.synchronize()
        assert kinds[0] and not all(kinds), kinds
        assert int(eng.skip_flag.sum()) == 0
        return first, eng.loss_dict()

    old, old_loss = run(True)
    new, new_loss = run(False)
    monkeypatch.delenv("NVO_RAY_HEAD_GENERIC", raising=False)
    for k in names:
        assert bool(torch.isfinite(new[k]).all())
        assert torch.equal(old[k].view(torch.uint8), new[k].view(torch.uint8)), f"first step: {k} differs between the forms"
    assert all(v == v for v in new_loss.values()) and all(v == v for v in old_loss.values())
