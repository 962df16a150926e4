"""The occupancy-grid kernel oracle (tests/helpers/ngp_oracle.py) checked against itself on the CPU: its closed-form
gradients against autograd and against central differences in float64 (a typo in a restatement would otherwise become
the GPU tests' truth), the case generators really hold every class they claim to, no transmittance sits near a threshold
a GPU test uses (why those tests need no tie allowance), and the committed float32 figures
(profiles/ngp_parity_margins.json, the e32 the GPU bounds are made of) still hold within a factor of two."""
import torch

from helpers import ngp_oracle as N

F64 = torch.float64


def _small_case():
    return N.composite_case(seed=3, listed=("empty", "dropped", 1, 2, 5), extra=("empty2", 7, 3), specials=False)


def _central(loss, x, eps=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        if keep != keep:  # (slots of no ray hold NaN)
            continue
        flat[i] = keep + eps
        up = float(loss(x))
        flat[i] = keep - eps
        dn = float(loss(x))
        flat[i] = keep
        gf[i] = (up - dn) / (2 * eps)
    return g


def test_closed_form_gradients_match_autograd_on_every_generated_sample():
    """The restated rule (clamped d exp / dx, exact zero on a capped sample) against plain autograd of the forward: equal
    to far below float32 resolution on every sample of the GPU tests' case -- all but the fp16-max one, where autograd
    ends in 0 * inf."""
    case = N.composite_case()
    big = case["pre"].float() == N.FP16_MAX
    assert int(big.sum()) == 1
    for name in ("bg-depth-cov-thr0", "nobg-depth-nocov-thr05", "states-thr0", "bg-nodepth-thr05"):
        opts = dict(N.COMPOSITE_VARIANTS[name], thr=0.0)
        ref = N.composite_reference(case, True, opts)
        loss, pre, y = N.composite_autograd(case, opts)
        g_pre, g_y = torch.autograd.grad(loss, (pre, y))
        live = ref["live"]
        assert bool(torch.isnan(g_pre[big]).all()) and float(ref["d_pre"][big]) == 0.0
        ok = live & ~big
        assert bool(torch.isfinite(g_pre[ok]).all())
        assert N.figure(ref["d_pre"][ok], g_pre[ok]) < 1e-12, (name, N.figure(ref["d_pre"][ok], g_pre[ok]))
        assert N.figure(ref["d_y"][live], g_y[live]) < 1e-12, name
        total = float(loss.detach())
        assert total > 0 and abs(total / 128.0 - float(ref["loss_rgb"] + ref["loss_depth"])) < 1e-12 * total
        # capped samples: autograd passes nothing through min(., 128), the rule has the exact zero
        capped = live & (torch.exp(case["pre"].double()) * case["dt"].double() >= N.DD_CAP) & ~big
        assert int(capped.sum()) >= 6 and float(g_pre[capped].abs().max()) == 0.0 and float(ref["d_pre"][capped].abs().max()) == 0.0


def test_closed_form_gradients_match_central_differences():
    case = _small_case()
    assert case["classes"]["count_dropped"] == 1 and case["R"] == 8
    for opts in (dict(background=True, depth="on", cov=True), dict(background=True, depth="on", cov=True, state=True),
                 dict(background=False, depth="null", R_dev=6, world_size=2)):
        ref = N.composite_reference(case, True, opts)
        pre0, y0 = case["pre"].double(), case["y"].double()
        num_pre = _central(lambda v: N.composite_autograd(case, opts, pre=v)[0].detach(), pre0.clone())
        num_y = _central(lambda v: N.composite_autograd(case, opts, y=v)[0].detach(), y0.clone())
        live = ref["live"]
        assert int(live.sum()) >= 10
        assert N.figure(ref["d_pre"][live], num_pre[live]) < 1e-6, N.figure(ref["d_pre"][live], num_pre[live])
        assert N.figure(ref["d_y"][live], num_y[live]) < 1e-6, N.figure(ref["d_y"][live], num_y[live])
        assert float(ref["d_pre"][~live].abs().max()) == 0.0


def test_threshold_rows_are_exact_zeros_and_nothing_else_changes():
    case = N.composite_case()
    a = N.composite_reference(case, True, N.COMPOSITE_VARIANTS["bg-depth-cov-thr0"])
    b = N.composite_reference(case, True, N.COMPOSITE_VARIANTS["bg-depth-cov-thr05"])
    dead = b["dead"]
    assert 50 < int(dead.sum()) < int(b["live"].sum()) // 2 and not bool(a["dead"].any())
    assert float(b["d_pre"][dead].abs().max()) == 0.0 and float(b["d_y"][dead].abs().max()) == 0.0
    assert torch.equal(a["d_pre"][~dead], b["d_pre"][~dead]) and torch.equal(a["out_rgb"], b["out_rgb"])
    # no sample of the case is reached with a transmittance within 1e-3 (relative) of the threshold the GPU test uses
    assert N.threshold_margin(b["T"], N.TRAIN_THR) > N.TIE_MARGIN
    p = N.pair_case()
    rp = N.composite_reference(p, True, dict(thr=N.TRAIN_THR))
    assert N.threshold_margin(rp["T"], N.TRAIN_THR) > N.TIE_MARGIN and 0 < int(rp["dead"].sum()) < int(rp["live"].sum())


def test_generators_hold_every_class():
    case = N.composite_case()
    cls = case["classes"]
    for e in N.LISTED_COUNTS + N.EXTRA_COUNTS:
        assert cls[f"count_{e}"] >= 1, e
    for k in ("thin", "surface", "hot", "fp16_max", "neg_inf", "dt0", "y30", "gt_depth_zero", "state0", "state1_short",
              "state1_long", "long_surface", "long_thin"):
        assert cls[k] >= 1, (k, cls)
    assert cls["fp16_max"] == 1 and cls["neg_inf"] == 1 and cls["dt0"] == 1 and cls["state2"] == 2
    for c in N.COV_CLASSES:
        assert cls[f"cov_{c}"] >= 1 and cls[f"cov_{c}_live"] >= 1, (c, cls)
    assert case["capacity"] % 16 == 0 and case["capacity"] <= 8192 and case["R"] <= 64
    assert cls["free_slots"] >= 16 and int(case["offsets"][-1]) + cls["free_slots"] == case["capacity"]
    entries = case["entries"]
    assert entries != sorted(entries, key=str)  # shuffled
    d = entries.index("dropped")
    assert int(case["counts"][d]) == 0 and int(case["offsets"][d + 1]) - int(case["offsets"][d]) == N.DROPPED_SLOTS
    assert bool((case["ray_idx"][int(case["offsets"][d]):int(case["offsets"][d + 1])] == -1).all())
    e = entries.index("empty")
    assert int(case["offsets"][e + 1]) == int(case["offsets"][e])
    assert bool((case["state"][case["counts"] > 0] != 2).all())  # state 2 implies count 0
    pre = case["pre"].float()
    live = case["ray_idx"] >= 0
    assert int(((pre >= 30) & (pre <= 70) & live).sum()) >= 6 and float(pre[live & torch.isfinite(pre) & (pre < 100)].max()) == 70.0
    hot = max(range(case["R"]), key=lambda r: int(case["counts"][r]))
    first_hot = int(torch.nonzero(pre[int(case["offsets"][hot]):int(case["offsets"][hot + 1])] >= 30)[0])
    assert first_hot >= 64  # behind thin samples, past the first chunk
    ref = N.composite_reference(case, True, N.COMPOSITE_VARIANTS["bg-depth-cov-thr0"])
    assert float(ref["T"][int(case["offsets"][hot]) + first_hot]) > 0.5
    assert float(ref["out_acc"].max()) <= 1.0 + 1e-12 and bool(torch.isfinite(ref["d_pre"]).all())
    # rays become opaque part-way, and the long surface rays only behind their first chunk
    for r, k in case["kind"].items():
        if k == "surface" and int(case["counts"][r]) > 64:
            o = int(case["offsets"][r])
            assert float(ref["T"][o + 64]) > 0.5 and float(ref["out_acc"][r]) > 0.99
    dt = case["dt"][live]
    assert int((dt == 0).sum()) == 1 and float(dt.min()) == 0.0 and bool(torch.isnan(case["dt"][~live]).all())
    for r in range(case["R"]):
        t = case["t"][int(case["offsets"][r]):int(case["offsets"][r]) + int(case["counts"][r])]
        assert bool((t > 0).all()) and bool((t[1:] > t[:-1]).all())
    assert int((case["y"].float().abs() == 30).sum()) >= 3 and float(case["y"].float()[live].abs().max()) == 30.0
    # the same-bits pairs: both kinds of ray, every 65th sample with dt = 0
    p = N.pair_case()
    assert p["counts"].tolist() == [64, 65] * (p["R"] // 2) and p["R"] >= 8
    for r in range(1, p["R"], 2):
        assert float(p["dt"][int(p["offsets"][r]) + 64]) == 0.0
        a, b = int(p["offsets"][r - 1]), int(p["offsets"][r])
        assert torch.equal(p["pre"][a:a + 64], p["pre"][b:b + 64]) and torch.equal(p["t"][a:a + 64], p["t"][b:b + 64])
    rp = N.composite_reference(p, True, {})
    assert float(rp["out_acc"].min()) < 0.5 and float(rp["out_acc"].max()) > 0.99
    # rounds: every cut leaves rays with and without a second part
    for cut in N.ROUND_CUTS:
        (c1, _), (c2, o2) = N.split_rounds(case, cut)
        assert torch.equal(c1 + c2, case["counts"]) and int((c2 == 0).sum()) >= 3 and int((c2 > 0).sum()) >= 3
        assert int((o2[:-1] + c2).max()) <= case["capacity"]
    hc = N.rgb_head_case()
    assert hc["capacity"] == 2048 and hc["classes"]["empty_rows"] == 58 and hc["classes"]["rays"] == N.HEAD_RAYS
    slot = torch.arange(hc["capacity"])
    assert int((hc["ray_idx"].long() == slot).sum()) <= 1  # gathering by slot index cannot pass for gathering by ray_idx
    tc = N.thickness_case()
    assert int(torch.isinf(tc["pre"]).sum()) == 1 and int((tc["pre"].float() == N.FP16_MAX).sum()) == 1
    for cap, seed in ((1000, 0), (N.LIVE_CAPACITY, 1)):
        pc = N.positions_case(cap, seed=seed)
        raw = N.positions_reference(pc)["raw"][pc["ray_idx"] >= 0]
        assert int((raw < -1e-5).sum()) >= 10 and int((raw > 1 + 1e-5).sum()) >= 10 and int((pc["ray_idx"] < 0).sum()) >= 48


def test_count_alive_cases_have_no_ties():
    """no transmittance of any sample a launch looks at lies within 1e-3 (relative) of the threshold: kept and state of the
    GPU tests are exact, no tie allowance"""
    for stride in (1, 16):
        case = N.alive_case(stride)
        cls = case["classes"]
        assert all(cls[k] >= 1 for k in ("cut_at_0", "cut_at_63", "cut_at_64", "cut_at_65", "never", "dropped", "empty", "carry_in")), cls
        assert case["R_dev"] < case["R"] and case["capacity"] % 16 == 0
        ref = N.alive_reference(case, R_dev=case["R_dev"], carry_in=case["carry_in"], rounds=True)
        assert ref["margin"] > N.TIE_MARGIN, ref["margin"]
        n = case["R_dev"]
        assert torch.equal(ref["kept"][:n], torch.where(ref["state"][:n] == 2, torch.zeros(n, dtype=torch.int64), case["expect"][:n]))
        assert set(ref["state"][:n].tolist()) == {0, 1, 2}
        f32 = N.alive_reference(case, R_dev=case["R_dev"], carry_in=case["carry_in"], rounds=True, dtype=torch.float32)
        assert torch.equal(f32["kept"], ref["kept"]) and torch.equal(f32["state"], ref["state"])
    # against the project's numpy restatement, single pass without a carry
    from oracle.ngp import alive_counts

    case = N.alive_case(1)
    plain = N.alive_reference(case)
    assert plain["margin"] > N.TIE_MARGIN
    pre, dt, cnt = [], [], case["counts"].tolist()
    for r in range(case["R"]):
        o = int(case["offsets"][r])
        pre.append(case["pre"][o:o + cnt[r]].double().numpy())
        dt.append(case["dt"][o:o + cnt[r]].double().numpy())
    kept, margin = alive_counts(cnt, dt, pre, N.ALIVE_THR)
    assert kept.tolist() == plain["kept"].tolist() and float(margin.min()) > N.TIE_MARGIN
    # rounds: the ray cut at 64 is found at index 0 of round two; the two rounds give the single pass
    rd = N.alive_rounds(case)
    one = N.alive_reference(case, counts=rd["counts"][0], offsets=rd["offsets"][0], t_next=rd["t_next"][0], rounds=True)
    two = N.alive_reference(case, counts=rd["counts"][1], offsets=rd["offsets"][1], t_next=rd["t_next"][1], rounds=True,
                            resume_in=one["resume_out"], carry_in=torch.nan_to_num(one["carry_out"]), kept_base=N.ALIVE_ROUND)
    assert min(one["margin"], two["margin"]) > N.TIE_MARGIN
    goes_on = one["resume_out"] >= 0
    assert int(((two["kept"] == N.ALIVE_ROUND) & (two["state"] == 1)).sum()) >= 2
    assert bool((two["kept"][~goes_on] == N.ALIVE_SENTINEL).all()) and bool((two["resume_out"][~goes_on] == -1).all())
    kept = torch.where(goes_on, two["kept"], one["kept"])
    assert kept.tolist() == plain["kept"].tolist()


def test_float32_exponential_is_the_devices_formulation():
    """__expf(x) = exp2(fl32(log2e * x)): the float32 runs carry the rounding of the argument, which grows with |x|"""
    x = torch.tensor([-80.0, -20.0, -1.0, 0.0, 3.0, 11.0], dtype=torch.float32)
    got = N._exp(x)
    assert got.dtype == torch.float32 and float(got[3]) == 1.0
    rel = ((got.double() - torch.exp(x.double())) / torch.exp(x.double())).abs()
    assert bool((rel <= (x.double().abs() * 2.0 ** -24 + 2.0 ** -23)).all()), rel
    assert float(rel[0]) > 2.0 ** -24  # the argument's rounding shows at |x| = 80
    assert float(N._exp(torch.tensor([-float("inf")]))[0]) == 0.0
    assert float(N.half_ulp_fp16(torch.tensor([1.0]))[0]) == 2.0 ** -11 and float(N.half_ulp_fp16(torch.tensor([1e-6]))[0]) == 2.0 ** -25


def test_committed_float32_figures_have_not_drifted():
    """e32 recomputed here against the committed file: more than 2x away fails (with a floor of one float32 ulp, 2^-23:
    figures of a handful of numbers are rounding luck), and so does a comparison the file does not know (or the other way
    round).  Every raised factor carries its reason; every recorded kernel figure lies within its bound."""
    m = N.load_margins()
    now = N.e32_figures()
    assert set(now) == set(m["e32"]), sorted(set(now) ^ set(m["e32"]))
    bad = {k: (m["e32"][k], v) for k, v in now.items()
           if v > 2 * m["e32"][k] + 2.0 ** -23 or m["e32"][k] > 2 * v + 2.0 ** -23}
    assert not bad, bad
    assert "fp16" in m["rule"] and set(m["max_abs_x"]) <= set(m["e32"])
    for key, entry in m.get("factors", {}).items():
        assert key in m["e32"] and entry["factor"] > 0 and entry["reason"]
    for key, got in m.get("measured_gfx950", {}).items():
        assert got <= N.bound_for(key, m), (key, got, N.bound_for(key, m))
