"""LPIPS (nerf_vo_amd/lpips.py) without a GPU: weight loading from both key sets, every refusal, the output-size
arithmetic, and the recorded oracle margins (profiles/lpips_parity_margins.json) against what ``--record`` reproduces."""
import pytest
import torch
import torch.nn.functional as TF

from helpers import lpips_cases as cases
from helpers import lpips_oracle as orc


def _lpips():
    from nerf_vo_amd import lpips

    return lpips


def _package_keys(sd):
    """The same tensors under the package's own names."""
    lp = _lpips()
    out = {}
    for l, i in enumerate(lp.TORCHVISION_INDEX):
        for part in ("weight", "bias"):
            out[f"net.slice{l + 1}.{i}.{part}"] = sd[f"features.{i}.{part}"]
        out[f"lins.{l}.model.1.weight"] = sd[f"lin{l}.model.1.weight"]
    return out


def test_weights_load_from_both_key_sets(tmp_path):
    lp = _lpips()
    sd = cases.weights()
    alex = {k: v for k, v in sd.items() if k.startswith("features.")}
    alex["classifier.1.weight"] = torch.zeros(4, 4)  # torchvision's file has more than the features: ignored
    lins = {k: v for k, v in sd.items() if k.startswith("lin")}
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lins, tmp_path / "alex_lin.pth")
    pkg = _package_keys(sd)
    pkg["scaling_layer.shift"] = torch.tensor([-0.03, -0.088, -0.188]).view(1, 3, 1, 1)
    pkg["scaling_layer.scale"] = torch.tensor([0.5, 0.25, 0.125]).view(1, 3, 1, 1)
    torch.save(pkg, tmp_path / "package.pth")
    a = lp.LPIPS.from_files(tmp_path / "alexnet.pth", tmp_path / "alex_lin.pth", device="cuda")
    b = lp.LPIPS.from_files(str(tmp_path / "package.pth"), device="cuda:0")
    assert sorted(a.weights) == sorted(b.weights) and len(a.weights) == 15
    for k in a.weights:
        assert torch.equal(a.weights[k], b.weights[k]), k
    for l, i in enumerate(lp.TORCHVISION_INDEX):
        assert torch.equal(a.weights[f"conv{l}.weight"], sd[f"features.{i}.weight"])
    assert a.shift == tuple(float(v) for v in orc.SHIFT) and a.scale == tuple(float(v) for v in orc.SCALE)
    assert b.scale == (0.5, 0.25, 0.125)
    # the packed form: k-major, zero rows past K
    w = sd["features.0.weight"]
    packed = lp.pack_weight(w)
    assert tuple(packed.shape) == (368, 64) and torch.equal(packed[:363], w.reshape(64, 363).t()) and not packed[363:].any()


def test_state_dicts_that_are_refused(tmp_path):
    lp = _lpips()
    sd = dict(cases.weights())
    with pytest.raises(ValueError, match="CUDA device"):
        lp.LPIPS(sd, device="cpu")
    del sd["features.8.bias"], sd["lin3.model.1.weight"]
    sd["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    sd["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError) as err:
        lp.LPIPS(sd)
    text = str(err.value)
    for piece in ("features.8.bias", "net.slice4.8.bias", "lin3.model.1.weight", "lins.3.model.1.weight", "features.3.weight",
                  "[192, 64, 5, 5]", "[192, 64, 3, 3]", "lin0.model.1.weight", "[1, 64, 1, 1]"):
        assert piece in text, piece
    with pytest.raises(ValueError, match="give the AlexNet file"):
        lp.LPIPS.from_files()
    with pytest.raises(FileNotFoundError):
        lp.LPIPS.from_files(tmp_path / "absent.pth")
    torch.save([1, 2, 3], tmp_path / "list.pth")
    with pytest.raises(ValueError, match="not a state dict"):
        lp.LPIPS.from_files(tmp_path / "list.pth")


def test_inputs_that_are_refused():
    lp = _lpips()
    model = lp.LPIPS(cases.weights())
    ok = torch.zeros(1, 3, 40, 40)
    with pytest.raises(ValueError, match="at least 31"):
        model(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))
    with pytest.raises(ValueError, match="at least 31"):
        model(torch.zeros(1, 3, 64, 30), torch.zeros(1, 3, 64, 30))
    with pytest.raises(ValueError, match=r"float32 \[F,3,H,W\]"):
        model(ok.double(), ok.double())
    with pytest.raises(ValueError, match=r"float32 \[F,3,H,W\]"):
        model(ok[0], ok[0])
    with pytest.raises(ValueError, match=r"float32 \[F,3,H,W\]"):
        model(torch.zeros(1, 4, 40, 40), torch.zeros(1, 4, 40, 40))
    with pytest.raises(ValueError, match=r"float32 \[F,3,H,W\]"):
        model(ok, ok.numpy())
    with pytest.raises(ValueError, match="one shape and one device"):
        model(ok, torch.zeros(1, 3, 40, 41))
    with pytest.raises(ValueError, match="one shape and one device"):
        model(ok, torch.zeros(1, 3, 40, 40, device="meta"))
    u8 = torch.zeros(1, 40, 40, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.lpips_uint8(u8, u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.features(ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lp.conv2d_relu(ok, torch.zeros(64, 3, 11, 11), torch.zeros(64), 4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lp.maxpool_3x3_s2(ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lp.head(ok, ok, torch.zeros(3))
    with pytest.raises(ValueError, match="'mean' or 'map'"):
        lp.head(ok, ok, torch.zeros(3), want="sum")
    # past the launchers' index range: conv1's F * Ho * Wo < 2^31, F <= 65535
    lp.check_sizes(8, 680, 1200)
    with pytest.raises(ValueError, match="fewer frames per call"):
        lp.check_sizes(65536, 31, 31)
    with pytest.raises(ValueError, match="fewer frames per call"):
        lp.check_sizes(43000, 680, 1200)  # 43000 * 169 * 299 > 2^31
    with pytest.raises(ValueError, match="empty batch"):
        lp.check_sizes(0, 40, 40)


@pytest.mark.parametrize("H,W", [(31, 31), (32, 35), (33, 64), (34, 127), (67, 95), (680, 1200)])
def test_output_sizes_are_torchs(H, W):
    """H = 31..34 are the four remainders of the stride-4 layer; sizes against torch's own layers on an empty-channel
    tensor (shape arithmetic only)."""
    lp = _lpips()
    sizes = lp.feature_sizes(H, W)
    x = torch.zeros(1, 1, H, W)
    got = []
    for (_, _, k, s, p), pool in zip(lp.LAYERS, lp.POOL_BEFORE):
        if pool:
            x = TF.max_pool2d(x, 3, 2)
        x = TF.conv2d(x, torch.zeros(1, 1, k, k), stride=s, padding=p)
        got.append(tuple(x.shape[2:]))
    assert sizes == got
    if (H, W) == (31, 31):
        assert sizes == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    if (H, W) == (680, 1200):
        assert sizes[0] == (169, 299)
    assert lp.LAYERS == orc.LAYERS and lp.POOL_BEFORE == orc.POOL_BEFORE and lp.TORCHVISION_INDEX == orc.TORCHVISION_INDEX


def test_synthetic_weights_are_what_they_say():
    lp = _lpips()
    a, b, c = lp.synthetic_weights(3), lp.synthetic_weights(3), lp.synthetic_weights(4)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["features.0.weight"], c["features.0.weight"])
    for l, (cin, cout, k, _, _) in enumerate(lp.LAYERS):
        w = a[f"features.{lp.TORCHVISION_INDEX[l]}.weight"]
        assert tuple(w.shape) == (cout, cin, k, k) and w.dtype == torch.float32
        assert abs(float(w.std()) / (2.0 / (cin * k * k)) ** 0.5 - 1) < 0.05
        lin = a[f"lin{l}.model.1.weight"]
        assert tuple(lin.shape) == (1, cout, 1, 1) and float(lin.min()) >= 0 and float(lin.max()) <= 1.0 / cout


def test_recorded_margins_are_what_record_reproduces():
    rec = cases.recorded()
    assert rec["weight_seed"] == cases.WEIGHT_SEED and sorted(rec["cases"]) == sorted(cases.CASES)
    for name in cases.CASES:
        now = cases.measure(name)
        assert len(rec["cases"][name]) == len(now) == 5
        for l, (old, new) in enumerate(zip(rec["cases"][name], now)):
            for key in ("feature_err", "feature_ref", "map_err", "map_ref"):
                assert abs(old[key] - new[key]) <= 1e-3 * abs(new[key]), (name, l, key, old[key], new[key])
            # a condition on the cases: the float32 chain stays within 1e-5 of the map's scale
            assert 0 < old["feature_err"] <= 1e-5 * old["feature_ref"], (name, l)
            assert 0 < old["map_err"] and old["map_ref"] > 0


def test_oracle_modes_and_ingest():
    """The oracle itself: the uint8 ingest is the reference's two rescalings; a padded tap contributes 0, not
    (0 - shift) / scale; identical images give 0; the tree mean of a constant map is the constant."""
    import numpy as np

    a, b = cases.frames("31x31")
    x = orc.image_of_uint8(a)
    assert x.dtype == torch.float32 and float(x.min()) >= -3 and float(x.max()) <= 1
    u = torch.from_numpy(a[0, 0, 0].astype(np.float32))
    assert torch.equal(x[0, :, 0, 0], ((u / 255) * 2 - 1) * 2 - 1)
    sd = cases.weights()
    f1 = orc.features(x, sd)[0]
    xs = orc.scaling_layer(x, torch.float64)
    direct = TF.relu(TF.conv2d(TF.pad(xs, (2, 2, 2, 2)), sd["features.0.weight"].double(), sd["features.0.bias"].double(), stride=4))
    assert torch.equal(f1, direct)
    same = orc.lpips(x, x, sd)
    assert float(same["value"].abs().max()) == 0
    ref = cases.reference("31x31")
    assert float(ref["value"][0]) > 0 and [tuple(m.shape) for m in ref["maps"]] == [(1, 7, 7), (1, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1)]
    assert orc.tree_mean(np.full(300, 0.25, np.float32)) == np.float32(0.25)
