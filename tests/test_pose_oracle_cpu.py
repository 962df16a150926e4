"""The pose-chain oracle (tests/helpers/pose_oracle.py) checked against itself on the CPU: central differences of every
chain function in float64 (a typo in a restatement would otherwise become the GPU tests' truth), the case generators
really reach every branch they claim to, and the committed float32 figures (profiles/pose_parity_margins.json, the e32
the GPU bounds are made of) still hold within a factor of two."""
import torch

from helpers import pose_oracle as P

F64 = torch.float64


def _central(loss, x, eps=1e-6):
    """d loss / d x by central differences (x float64, loss a python function of a tensor shaped like x)"""
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + eps
        up = float(loss(x))
        flat[i] = keep - eps
        dn = float(loss(x))
        flat[i] = keep
        gf[i] = (up - dn) / (2 * eps)
    return g


def _close(got, ref, tol=1e-6):
    assert P.figure(got, ref) <= tol, P.figure(got, ref)


def test_positions_chain_matches_central_differences():
    from oracle import rays as Rr

    c = P.positions_case(5, 48)
    mask = P.selector32(c["origins"], c["directions"], c["tbins"])
    assert bool(mask.any())
    go, gd = P.positions_chain(c["origins"], c["directions"], c["tbins"], c["dx01"][0], mask)
    tb = c["tbins"].double()
    tb = torch.where(torch.isfinite(tb), tb, torch.zeros_like(tb))
    g = torch.where(mask[:, :, None], torch.zeros(5, 48, 3, dtype=F64), c["dx01"][0].double().view(5, 48, 3))

    def loss(o, d):
        return (g * Rr.normalized_positions(Rr.sample_positions(o, d, tb))[0]).sum()

    o, d = c["origins"].double(), c["directions"].double()
    _close(go, _central(lambda v: loss(v, d), o.clone(), 1e-7), 1e-5)
    _close(gd, _central(lambda v: loss(o, v), d.clone(), 1e-7), 1e-5)
    # by hand: an uncontracted sample passes dx01 / 4 to the origin, the mag == 1 sample of ray 0 as well (f = 1, f' = 0)
    one = P.positions_case(5, 1)
    go1, gd1 = P.positions_chain(one["origins"], one["directions"], one["tbins"], one["dx01"][0],
                                 P.selector32(one["origins"], one["directions"], one["tbins"]))
    _close(go1[0], one["dx01"][0][0].double() / 4, 1e-12)
    _close(gd1[0], one["dx01"][0][0].double() / 4, 1e-12)  # (midpoint exactly 1)


def test_ngp_positions_chain_matches_central_differences():
    c = P.ngp_case("size3")
    ray, slot = P.packed_ranges(c["counts"], c["offsets"], c["capacity"], c["R_dev"])
    t, dx = c["t"].double()[slot], c["dx01"].double()[slot]

    def loss(o, d):
        return (dx * ((o[ray] + t[:, None] * d[ray] - c["lo"]) / (c["hi"] - c["lo"])).clamp(0, 1)).sum()

    o, d = c["origins"].double(), c["directions"].double()
    ref = P.ngp_reference(c, True)
    _close(ref["d_origin"], _central(lambda v: loss(v, d), o.clone()))
    _close(ref["d_dir"], _central(lambda v: loss(o, v), d.clone()))
    assert float(ref["d_origin"][c["R_dev"]:].abs().max()) == 0.0
    host = P.ngp_reference(c, False)
    assert float(host["d_origin"][-1].abs().max()) == 0.0 and float(host["d_origin"][-2].abs().max()) > 0.0
    # a coordinate exactly in a face gets no gradient (torch.clamp's own backward would pass it)
    p2 = P.ngp_case("pow2")
    ref2 = P.ngp_reference(p2, False)
    assert float(ref2["d_origin"][6:8, 0].abs().max()) == 0.0 and float(ref2["d_origin"][6:8, 1:].abs().min()) > 0.0


def test_sh_chain_matches_central_differences():
    from oracle import sh as Sh

    for degree in (1, 2, 3, 4):
        c = P.sh_case(degree, N=64)
        dy = c["dy"][:, :degree * degree].double()
        got = P.sh_chain(c["d01"], c["dy"], degree)
        _close(got, _central(lambda v: (dy * Sh.sh_encode(v, degree)).sum(), c["d01"].double().clone()), 1e-7)
    assert float(P.sh_chain(c["d01"], c["dy"], 1).abs().max()) == 0.0


def test_pose_chain_is_the_gradient_of_the_corrected_rays():
    """pose_chain is a written-out sum; autograd through generate_rays / apply_pose_correction must agree with it."""
    from oracle import rays as Rr

    c = P.pose_case(9, 16, stale=False)
    F = c["F"]
    idx, intr, c2w = c["idx"], c["intr"][:F].double(), c["c2w"][:F].double()
    corr = torch.cat([torch.eye(3, dtype=F64), torch.zeros(3, 1, dtype=F64)], dim=1).repeat(F, 1, 1).requires_grad_(True)
    ro, rd, _, _ = Rr.generate_rays(idx, intr, c2w)
    o, d = Rr.apply_pose_correction(ro, rd, corr[idx[:, 0]])
    L = (c["d_origin"].double() * o).sum() + (c["d_dir"].double() * d).sum() + (c["d_dir01"].double() * (d + 1) / 2).sum()
    _close(P.pose_reference(c, True)["d_corr"], torch.autograd.grad(L, corr)[0], 1e-12)
    s = P.pose_case(1501, 7, stale=True)
    kept = P.pose_reference(s, False)["d_corr"]
    assert kept.shape == (7, 3, 4) and bool(torch.isfinite(kept).all())


def test_exp_chain_matches_central_differences():
    for mode in P.EXP_BUCKETS:
        c = P.exp_case(mode, n=32)
        variant = P.EXP_VARIANTS[2]
        _, tp, rp, host, dev = variant
        ref = P.exp_reference(c, variant)
        dc = c["d_corr"].double()

        def loss(t):
            from oracle import rays as Rr

            return (dc * P.exp_map(t, mode)).sum() + host * dev * Rr.camera_opt_regularizer(t, tp, rp)

        num = _central(loss, c["tangent"].double().clone(), 1e-7)
        # (rows at |w| = 0 or with a zero translation sit on the norm's kink: autograd's sub-gradient there is 0; the two
        # SE3 buckets 1e-7 either side of the Taylor switch are closer to it than the difference step: the two branches'
        # VALUES differ by theta^4 / 48 = 2e-10 there, which the step would divide by 2e-7)
        w = c["tangent"][:, 3:].double().norm(dim=1)
        smooth = (c["tangent"][:, :3].abs().sum(1) > 0) & (w > 1e-6) & ((w - 1e-2).abs() > 1e-6)
        assert int(smooth.sum()) >= 16
        _close(ref["d_tangent"][smooth], num[smooth], 2e-5)
        rot = P.exp_map(c["tangent"].double(), mode)[:, :, :3]
        big = c["tangent"][:, 3:].norm(dim=1) > 1.5e-2  # (below it SO3xR3's clamp leaves the rotation slightly non-orthogonal)
        assert float((rot[big] @ rot[big].transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-9


def test_whole_chain_matches_central_differences():
    for mode in P.EXP_BUCKETS:
        c = P.chain_case(mode, R=40, F=7)
        ref = P.chain_reference(c)["d_tangent"]
        tp, rp, scale = P.CHAIN_PENALTIES

        def loss(t):
            from oracle import rays as Rr
            from oracle import sh as Sh

            o, d = P.corrected_rays(t, c["idx"], c["intr"], c["c2w"], mode)
            L = (c["d_sh"].double() * Sh.sh_encode((d + 1) / 2, 4)).sum()
            for tb, dx in zip(c["tbins"], c["dx01"]):
                x01, _ = Rr.normalized_positions(Rr.sample_positions(o, d, tb.double()))
                L = L + (dx.double().view(x01.shape) * x01).sum()
            return L + scale * Rr.camera_opt_regularizer(t, tp, rp)

        num = _central(loss, c["tangent"].double().clone(), 1e-8)
        smooth = torch.ones(7, 6, dtype=torch.bool)
        smooth[0, 3:] = False  # |w| = 0: the rotation norm's kink
        smooth[2, :3] = False  # zero translation: the translation norm's kink
        _close(ref[smooth], num[smooth], 1e-4)


def test_generators_reach_every_branch():
    total = {}
    for R in P.POSITIONS_R:
        for S in P.POSITIONS_S:
            c = P.positions_case(R, S)
            assert bool(P.tie_free(c["origins"][1:], c["directions"][1:], c["tbins"][1:]).all())
            mask = P.selector32(c["origins"], c["directions"], c["tbins"])
            cls = P.sample_classes(c["origins"], c["directions"], c["tbins"], mask)
            if R == 259 and S >= 48:
                assert all(v > 0 for v in cls.values()), (R, S, cls)
            if R >= 5:
                assert cls["mag_one"] >= 1 and cls["inf_edge"] == 1 and bool(mask[R - 1, S - 1])
            assert float(c["tbins"][torch.isfinite(c["tbins"])].max()) <= 2000.0
            for k, v in cls.items():
                total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    for box in P.NGP_BOXES:
        c = P.ngp_case(box)
        assert all(n > 0 for n in c["per_face"]) and c["sides"]["inside"] > 0
        assert (c["sides"]["on_face"] > 0) == (box == "pow2")
        assert c["R_dev"] < c["R"] and int(c["offsets"][-1]) >= c["capacity"]
    for mode, buckets in P.EXP_BUCKETS.items():
        c = P.exp_case(mode)
        w = c["tangent"][:, 3:].double().norm(dim=1)
        for k, target in enumerate(buckets):
            rows = c["bucket"] == k
            assert int(rows.sum()) >= 16
            assert bool(((w[rows] - target).abs() <= 1e-6 * target + 1e-12).all()), (mode, target)
            assert int((c["tangent"][rows, :3].abs().sum(1) == 0).sum()) >= 1, "no zero-translation row in a bucket"
        small = (w < 1e-2) if mode == "SE3" else (w * w < 1e-4)
        assert 0 < int((small & (w > 0)).sum()) < c["n"]
    assert [P.rays_per_camera_path(R, F) for R, F in P.POSE_SHAPES] == ["table", "table", "table", "plain", "plain"]
    assert {P.rays_per_camera_path(R, F) for R, F in P.STALE_SHAPES} == {"table", "plain"}
    assert any(R % 8 for R, _ in P.STALE_SHAPES)
    c = P.pose_case(9, 16)
    assert len(set(c["idx"][:, 0].tolist())) < 16 // 2 + 2  # most cameras without a ray
    for mode in P.EXP_BUCKETS:
        c = P.chain_case(mode)
        assert set(c["idx"][:, 0].tolist()) == set(range(7))


def test_committed_float32_figures_have_not_drifted():
    """e32 recomputed here against the committed file: more than 2x away fails, and so does a comparison of the GPU test
    that the file does not know (or the other way round).  The 2x rule carries a floor of 2^-23, one float32 ulp of the
    largest entry: several figures are the maximum over three numbers (R = 1) or exactly 0, and whether such a figure is
    0.3 or 0.9 ulp is the rounding luck of one summation order, not drift."""
    m = P.load_margins()
    now = P.e32_figures()
    assert set(now) == set(m["e32"]), sorted(set(now) ^ set(m["e32"]))
    bad = {k: (m["e32"][k], v) for k, v in now.items()
           if v > 2 * m["e32"][k] + 2.0 ** -23 or m["e32"][k] > 2 * v + 2.0 ** -23}
    assert not bad, bad
    for key, entry in m.get("factors", {}).items():
        assert key in m["e32"] and entry["factor"] > 0 and entry["reason"]
    for key, got in m.get("measured_gfx950", {}).items():
        assert got <= P.bound_for(key, m), (key, got, P.bound_for(key, m))
