"""conv_halo through cs_op_conv, one case per instantiation the dispatch of canonswap_amd/csrc/conv_halo.hip can launch (tests/conv_cases.py; that the
table reaches every row, and only rows that exist, is tests/test_conv_ref_cpu.py's host-side check), every element of every output against float64
under the bound conv_ref derives from the number formats (tests/conv_ref.py: no tuned constant).

Two operand sets per case: signed (cancellation, the realistic one) and non-negative x, w and bias, where mag equals the value and the bound is
about (K + 2) 2^-24 relative, so that an fp16 rounding anywhere on an fp32 path breaches it at nearly every element.  Operands are multiples of a
power of two that fp16 holds exactly (fp32 for the biases, scales and statistics), so float64 sees what the kernel reads.

Every output sits in a NaN-filled buffer whose positions are 8 channels wider than the launch's Cout, with 64 more elements behind the last
position: the 8 neighbour channels of every position and the tail must still be NaN after the launch; input channel slices have 7.0 in the
neighbouring channels.  Cases inside the coverage of conv_wide, conv_lat or vol32 (conv_cases.py, `other`) run once more through that kernel - the same
operands, the same want and bound, fresh buffers; that kernel refusing the case fails the test.  Every case prints its largest |err| / bound;
DESIGN.md section 3 records them."""
import zlib

import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


OTHER_CFG = {"vol32": 30, "wide": 31, "lat": 32}          # CFG_VOL32, CFG_WIDE, CFG_LAT of common.h


def _cl(t, dtype, hwdc=False):
    """NCDHW float64 -> the logical [N, D, H, W, C] view of dtype on the device; stored in that order, or (hwdc) as [N][H][W][D][C]"""
    if hwdc:
        return t.permute(0, 3, 4, 2, 1).contiguous().to(dtype).to(DEV).permute(0, 3, 1, 2, 4)
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dtype).to(DEV)


def _out(N, D, H, W, C, dtype, hwdc=False):
    """(flat NaN buffer, its [N, D, H, W, C] view): positions of C + 8 channels, 64 elements behind the last.  hwdc: stored [N][H][W][D][C] with no
    channels between the positions (vol32 wants a depth stride of 32): the guard is the tail alone"""
    if hwdc:
        flat = torch.full((N * D * H * W * C + 64,), NAN, dtype=dtype, device=DEV)
        return flat, flat[: N * D * H * W * C].view(N, H, W, D, C).permute(0, 3, 1, 2, 4)
    flat = torch.full((N * D * H * W * (C + 8) + 64,), NAN, dtype=dtype, device=DEV)
    return flat, flat[: N * D * H * W * (C + 8)].view(N, D, H, W, C + 8)[..., :C]


def _untouched(flat, N, D, H, W, C, hwdc=False):
    if hwdc:
        return bool(torch.isnan(flat[N * D * H * W * C:]).all())
    body = flat[: N * D * H * W * (C + 8)].view(N, D, H, W, C + 8)
    return bool(torch.isnan(body[..., C:]).all()) and bool(torch.isnan(flat[N * D * H * W * (C + 8):]).all())


def _ncdhw(view):
    return view.permute(0, 4, 1, 2, 3).double().cpu()


def _check(label, got, want, bound, ratios):
    err = (got - want).abs()
    assert not bool(torch.isnan(got).any()), label + ": NaN left in the output (an element the launch did not write)"
    ratio = float((err / bound).max())
    ratios.append("%s %.4f" % (label, ratio))
    bad = int((err > bound).sum())
    assert bad == 0, "%s: %d of %d elements beyond the bound, largest |err| / bound %.3f, largest |err| %.3e" % (label, bad, err.numel(), ratio, float(err.max()))


def run_case(c, nonneg):
    import hip_ops as ops
    from canonswap_amd import pack
    plan = __import__("conv_plan_host").plans()[c["name"]]
    r = np.random.Generator(np.random.PCG64(zlib.crc32(c["name"].encode()) + int(nonneg)))
    lo = 0.0 if nonneg else -1.0
    hcfg, ck, mode, stv = c["row"]
    form, k = c["form"], c["k"]
    N0, D, H, W = c["dims"]
    rep = c.get("rep", 1)
    N = N0 * rep
    cin, cinr, cout, cpad = c["cin"], c["cin_real"], c["cout"], c["cout_pad"]
    twin = mode in (cc.TBLEND, cc.SPADE)
    rows = cpad // 2 if twin else cpad
    hilo = form.startswith("hilo")
    up = 1 if form == "slice_up" else 0
    hwdc = c.get("layout") == "hwdc"
    K = (32 if hilo else cinr) * int(np.prod(k))
    wstep = 2.0 ** -(6 + int(np.ceil(np.log2(np.sqrt(K)))))
    rw = lambda *s: cr.exact16(r, s, 64 * wstep * lo, 64 * wstep, wstep)
    x = cr.exact16(r, (N0, 32 if hilo else cinr, D, H >> up, W >> up), lo, 1.0)
    bias = torch.zeros(cpad, dtype=torch.float64)
    bias[:cout] = cr.exact32(r, (cout,), 0.5 * lo, 0.5)
    kw, ref = {}, {}
    if hilo:
        whi, wlo = rw(rows, 32, *k), rw(rows, 32, *k) * 2.0 ** -11
        xlo = cr.exact16(r, x.shape, lo, 1.0) * 2.0 ** -11
        wp = ops.packed_weight(torch.cat([whi, wlo, whi], 1), cpad, DEV)
        x = torch.cat([x, xlo], 1)
        ref["hilo"] = (whi[:cout], wlo[:cout])
        w = None
    else:
        w = rw(rows, cinr, *k)
        if twin:
            w2 = rw(rows, cinr, *k)
            wp = torch.from_numpy(pack.pack_conv(pack.interleave16(w.numpy(), w2.numpy()), cpad)).to(DEV)
            ref["w2"] = w2[:cout]
        else:
            wp = ops.packed_weight(w, cpad, DEV)
        if c.get("ragged"):
            ops.pair_ragged(wp, cpad, cin, k)
            kw["ragged"] = True
    # ---- the input: plain, or a channel slice of a 144-wide buffer with 7.0 in the neighbouring channels
    if form in ("slice", "slice_up"):
        buf = torch.full((N, D, H >> up, W >> up, 144), 7.0, dtype=torch.float16, device=DEV)
        buf[..., 32:32 + cin] = 0.0
        buf[..., 32:32 + cinr] = _cl(x, torch.float16).repeat(rep, 1, 1, 1, 1)
        xd = buf[..., 32:]
    else:
        xd = torch.zeros(N, D, H >> up, W >> up, cin if not hilo else 64, dtype=torch.float16, device=DEV)
        if hwdc:
            xd = torch.zeros(N, H, W, D, xd.shape[4], dtype=torch.float16, device=DEV).permute(0, 3, 1, 2, 4)
        xd[..., : x.shape[1]] = _cl(x, torch.float16).repeat(rep, 1, 1, 1, 1)
    kw.update(cin=cin, bias=bias.float().to(DEV), up_shift=up, hilo=hilo, ep_general=bool(c.get("general")), tile=c["tile"], ck=0 if c.get("planned") else ck,
              cfg=-2 if c.get("planned") else hcfg, out_dims=(N, D, H, W))
    ref.update(bias=bias[:cout], up_shift=up)
    per = lambda t: t if rep == 1 else t.repeat(rep, *([1] * (t.dim() - 1)))          # a per-sample device tensor of the N0 distinct samples -> the batch
    o0_f32, has_o0, pool = True, True, False

    def residual(dtype, shift=0):
        t = (cr.exact16 if dtype == torch.float16 else cr.exact32)(r, (N0, cout, D, H >> shift, W >> shift), 2 * lo, 2.0)
        ref["res"] = t
        return per(_cl(t, dtype, hwdc))

    def second(act, slope, affine=True):
        if affine:
            s2, t2 = torch.ones(cpad, dtype=torch.float64), torch.zeros(cpad, dtype=torch.float64)
            s2[:cout], t2[:cout] = cr.exact32(r, (cout,), 0.5, 1.5), cr.exact32(r, (cout,), -0.2, 0.2)
            kw.update(s2=s2.float().to(DEV), t2=t2.float().to(DEV))
            ref.update(s2=s2[:cout], t2=t2[:cout])
        kw.update(act1=act, slope1=slope)
        ref.update(out1=True, act1=act, slope1=slope)

    def stats_in():
        st = torch.stack([cr.exact32(r, (N0, cout), -0.3, 0.3), cr.exact32(r, (N0, cout), 0.5, 1.5)], 2)
        kw["stats"] = per(st.float().to(DEV)).contiguous()
        ref["stats"] = st

    act = ("relu", 0.0)
    if form in ("f16", "slice"):
        act, o0_f32 = ("lrelu", 0.2), False
    elif form == "res16_o1":
        act, o0_f32, kw["res"] = ("none", 0.0), False, residual(torch.float16)
        second("lrelu", 0.01)
    elif form == "res32_o1":
        act, kw["res"] = ("none", 0.0), residual(torch.float32)
        second("relu", 0.0)
    elif form == "res32_inplace":
        act = ("none", 0.0)
        res_dev = residual(torch.float32)
    elif form == "ps":
        ps = cr.exact32(r, (N0, 1, D, H, W), 0.0, 1.0)
        kw.update(pixscale=per(ps.float().to(DEV)).contiguous(), ps_stride=1)
        ref["pixscale"] = ps
    elif form == "pool":
        o0_f32, pool = False, True
        kw["pool_hw"] = True
    elif form in ("gelu", "sigmoid"):
        act = (form, 0.0)
    elif form == "dup":
        o0_f32 = False
        second("none", 0.0, affine=False)
    elif form == "f32o1":
        act = ("none", 0.0)
        second("none", 0.0, affine=False)
    elif form == "o1only":
        act, has_o0, kw["res"] = ("none", 0.0), False, residual(torch.float16)
        second("lrelu", 0.2, affine=False)
    elif form in ("hilo", "hilo_stat"):
        act = ("none", 0.0)
    elif form in ("stat16", "res16"):
        act, o0_f32, kw["res"] = ("none", 0.0), False, residual(torch.float16)
    elif form == "stat16nores":
        o0_f32 = False
    elif form == "lin32":
        act = ("none", 0.0)
    elif form in ("tblend", "tblend16", "tblend_o1"):
        act = ("none", 0.0)
        ps = cr.exact32(r, (N0, 1, D, H, W), 0.0, 1.0)
        m4 = torch.full((N, D, H, W, 4), NAN, dtype=torch.float32, device=DEV)
        m4[..., 0] = per(ps[:, 0].float().to(DEV))
        kw.update(pixscale=m4, ps_stride=4, mode=1)
        ref.update(pixscale=ps, mode="tblend")
        if form == "tblend16":
            o0_f32 = False
        else:
            kw["res"] = residual(torch.float32)
        if form == "tblend_o1":
            second("lrelu", 0.01)
    elif form.startswith("spade") or form.startswith("spmul"):
        sh = int(form[-1])
        o0_f32 = False
        kw.update(res=residual(torch.float16, sh), res_shift=sh)
        stats_in()
        ref["res_shift"] = sh
        if form.startswith("spade"):
            b2 = torch.zeros(cpad, dtype=torch.float64)
            b2[:cout] = cr.exact32(r, (cout,), 0.5 * lo, 0.5)
            act = ("lrelu", 0.2)
            kw.update(bias2=b2.float().to(DEV), mode=2)
            ref.update(bias2=b2[:cout], mode="spade")
        else:
            act = ("none", 0.0)
            kw["mode"] = 5
            ref["mode"] = "spmul"
    elif form == "pixshuf":
        act = ("sigmoid", 0.0)
        kw["mode"] = 3
        ref["mode"] = "pixshuf"
    else:
        assert form in ("f32", "slice_up", "stat32"), form
    kw.update(act0=act[0], slope0=act[1])
    ref.update(act0=act[0], slope0=act[1], out0=has_o0, out0_f32=o0_f32, pool_hw=pool)
    # ---- outputs, the launch, the comparison: once on conv_halo, then once more on every other kernel that has to take this case
    oH, oW = (H // 2, W // 2) if pool else (H, W)
    want = cr.conv_ref(x, None if w is None else w[:cout], **ref)
    tag = "%s[%s]" % (c["name"], "nonneg" if nonneg else "signed")
    ratios = []

    def launch(kernel):
        f0 = v0 = f1 = v1 = fs = None
        k2 = dict(kw)
        lab = tag if kernel == "halo" else "%s via %s" % (tag, kernel)
        if kernel != "halo":
            k2.update(cfg=OTHER_CFG[kernel], ck=0, tile=(0, 0))
        if form == "pixshuf":
            f0 = torch.full((N * 3 * 4 * H * W + 64,), NAN, dtype=torch.float32, device=DEV)
            v0 = f0[: N * 3 * 4 * H * W].view(N, 3, 2 * H, 2 * W)
        elif has_o0:
            f0, v0 = _out(N, D, oH, oW, cout, torch.float32 if o0_f32 else torch.float16, hwdc)
            if form == "res32_inplace":
                v0.copy_(res_dev)
                k2["res"] = v0
        if has_o0:
            k2["out0"] = v0
        if ref.get("out1"):
            f1, v1 = _out(N, D, H, W, cout, torch.float16, hwdc)
            k2["out1"] = v1
        if mode == cc.STDSTAT:
            # vol32 has its own partial-statistics blocks: one per (8 rows, column pair) of the [H][W] plane, each the whole depth
            nblk = ((H + 7) // 8) * (W // 2) if kernel == "vol32" else plan["stat_nblk"]
            fs = torch.full((N * nblk * cout * 2 + 64,), NAN, dtype=torch.float32, device=DEV)
            k2["stat_out"] = fs[: N * nblk * cout * 2].view(N, nblk, cout, 2)
        ops.conv(xd, wp, cpad, cout, k, **k2)
        torch.cuda.synchronize()
        if form == "pixshuf":
            assert bool(torch.isnan(f0[N * 3 * 4 * H * W:]).all()), "wrote behind the image"
            _check(lab + " out0", v0.double().cpu(), *want["out0"], ratios)
        elif has_o0:
            assert _untouched(f0, N, D, oH, oW, cout, hwdc), "out0: wrote outside its channels / positions"
            for i in range(1, rep):
                assert torch.equal(v0[i * N0:(i + 1) * N0], v0[:N0]), "copy %d of the samples differs" % i
            _check(lab + " out0", _ncdhw(v0[:N0]), *want["out0"], ratios)
        if v1 is not None:
            assert _untouched(f1, N, D, H, W, cout, hwdc), "out1: wrote outside its channels / positions"
            _check(lab + " out1", _ncdhw(v1[:N0]), *want["out1"], ratios)
        if fs is not None:
            assert bool(torch.isnan(fs[N * nblk * cout * 2:]).all()), "wrote behind the statistics"
            got = k2["stat_out"].double().cpu()
            if kernel == "vol32":
                # its blocks summed: a partial adds at most the 8 x 2 x 16 = 256 values of its block in some order (g(255)), the float64 sum of the
                # partials here is exact to 2^-53: |sum - want| <= g(256) sum |v| for the values and for their squares
                st = _ncdhw(v0).reshape(N, cout, -1)
                sw = torch.stack([st.sum(-1), (st * st).sum(-1)], -1)
                sb = cr.gamma(256) * torch.stack([st.abs().sum(-1), (st * st).sum(-1)], -1) + cr.TINY32
                _check(lab + " stat", got.sum(1), sw, sb, ratios)
            else:
                sw, sb = cr.stat_ref(_ncdhw(v0), plan["lgT"], plan["wave_px"])
                _check(lab + " stat", got, sw, sb, ratios)

    launch("halo")
    for kernel in c.get("other", ()):
        launch(kernel)
    if form in ("slice", "slice_up"):
        assert bool((buf[..., :32] == 7.0).all())
    print("\n" + "; ".join(ratios))


@pytest.mark.parametrize("nonneg", [False, True], ids=["signed", "nonneg"])
@pytest.mark.parametrize("c", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_conv_bound(c, nonneg):
    run_case(c, nonneg)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["STD", "TBLEND", "SPADE"])
@pytest.mark.parametrize("ck", [64, 32])
def test_128x256_tiles_refuse_dynamic_shapes(mode, ck):
    """The 128x256 tile runs 3x3 convs on 16 x 8 tiles only: its dynamic-shape kernels are not built (hipcc spilled their hand-counted weight ring; the
    weight ring: conv_halo.hip, launch_halo_cfg), and every other shape is refused before anything is launched."""
    import hip_ops as ops
    x = torch.zeros(2, 1, 32, 16, 128, dtype=torch.float16, device=DEV)
    w = torch.zeros(4 * 9, 256, 32, dtype=torch.float16, device=DEV)
    out = torch.zeros(2, 1, 32, 16, 128, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="128x256 tile exists for the static shapes only"):
        ops.conv(x, w, 256, 128, (1, 3, 3), out0=out, mode=mode, cfg=17, ck=ck, tile=(8, 16))
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_extents_that_are_no_whole_tiles_are_refused():
    """halo_plan() has no partial tiles: 24 columns on 16-column tiles would leave the last 8 unwritten, so cs_op_conv refuses the launch"""
    import hip_ops as ops
    x = torch.zeros(1, 1, 16, 24, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(2 * 9, 128, 32, dtype=torch.float16, device=DEV)
    out = torch.zeros(1, 1, 16, 24, 128, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="not a whole number of"):
        ops.conv(x, w, 128, 128, (1, 3, 3), out0=out, cfg=10)
    torch.cuda.synchronize()
    assert not bool(out.any())
