"""tests/conv_ref.py and tests/conv_cases.py without a GPU: the float64 restatement of cs_op_conv agrees with the formulas the other tests use, its
bound is neither too tight for a correct fp32 convolution nor loose enough to let the faults of the issue through, and the case table of
tests/test_gpu_conv_bounds.py reaches exactly the instantiations canonswap_amd/csrc/conv_halo.hip can launch."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import conv_plan_host as ph
import conv_ref as cr
import spade_ref as S
import volume_ref as V

needs_clang = pytest.mark.skipif(not os.path.exists(ph.CLANG), reason="needs ROCm's clang (ext_vector_type, _Float16)")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------------ agreement with the existing formulas
def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_agrees_with_volume_ref():
    """3x3x3 'same' conv + bias (+ residual), the second output through the next block's affine and LeakyReLU: volume_ref.conv / _aff / lrelu"""
    r = _rng(1)
    x, w, b = cr.exact16(r, (2, 32, 4, 8, 8)), cr.exact16(r, (32, 32, 3, 3, 3), -0.1, 0.1, 2.0 ** -12), cr.exact32(r, (32,))
    res, s2, t2 = cr.exact32(r, (2, 32, 4, 8, 8)), cr.exact32(r, (32,), 0.5, 1.5), cr.exact32(r, (32,))
    o = cr.conv_ref(x, w, bias=b, res=res, s2=s2, t2=t2, act1="lrelu", slope1=V.SLOPE, out1=True)
    y = V.conv(x, w, b) + res
    _close(o["out0"][0], y)
    _close(o["out1"][0], V.lrelu(V._aff(y, (s2, t2))))
    _close(cr.conv_ref(x[:, :, :1], w[:, :, 1:2], bias=b, act0="relu")["out0"][0], F.relu(V.conv(x[:, :, 0], w[:, :, 1], b)).unsqueeze(2))


@pytest.mark.parametrize("up", [False, True])
def test_agrees_with_spade_ref(up):
    """SPADE and its gamma-only form (spmul) against spade_ref.spade / normalized / conv3, at the same and at half the resolution"""
    r = _rng(2 + up)
    Cc, Sx = 16, 8 >> up
    actv, x = cr.exact16(r, (1, 32, 8, 8)), cr.exact16(r, (1, Cc, Sx, Sx), -2, 2)
    wg, wb = cr.exact16(r, (Cc, 32, 3, 3), -0.1, 0.1, 2.0 ** -12), cr.exact16(r, (Cc, 32, 3, 3), -0.1, 0.1, 2.0 ** -12)
    bg, bb = cr.exact32(r, (Cc,)), cr.exact32(r, (Cc,))
    stats = torch.stack([cr.exact32(r, (1, Cc), -0.3, 0.3), cr.exact32(r, (1, Cc), 0.5, 1.5)], 2)
    st = (stats[0, :, 0], stats[0, :, 1])
    u5 = lambda t: t.unsqueeze(2)
    kw = dict(res=u5(x), res_shift=int(up), stats=stats, out0_f32=False)
    o = cr.conv_ref(u5(actv), u5(wg), bias=bg, w2=u5(wb), bias2=bb, mode="spade", act0="lrelu", slope0=0.2, **kw)
    _close(o["out0"][0][:, :, 0], S.step_spade(x, st, actv, (wg, bg, wb, bb), up))
    o = cr.conv_ref(u5(actv), u5(wg), bias=bg, mode="spmul", **kw)
    _close(o["out0"][0][:, :, 0], S.normalized(x, st, up) * (1 + S.conv3(actv, wg, bg)))


def test_agrees_with_the_operator_tests_formulas():
    """The forms tests/test_gpu_ops.py states inline (T blend, pixel shuffle, pooled output, folded up-sampling, per-position scale), in float64"""
    r = _rng(4)
    x, w, b = cr.exact16(r, (2, 32, 1, 8, 8)), cr.exact16(r, (16, 32, 1, 3, 3), -0.1, 0.1, 2.0 ** -12), cr.exact32(r, (16,))
    wm, mask, res = cr.exact16(r, (16, 32, 1, 3, 3), -0.1, 0.1, 2.0 ** -12), cr.exact32(r, (2, 1, 1, 8, 8), 0, 1), cr.exact32(r, (2, 16, 1, 8, 8))
    c2 = lambda ww, bb=None: F.conv2d(x[:, :, 0], ww[:, :, 0], bb, padding=1).unsqueeze(2)
    o = cr.conv_ref(x, w, w2=wm, bias=b, mode="tblend", pixscale=mask, res=res)
    _close(o["out0"][0], mask * c2(wm, b) + (1 - mask) * c2(w) + res)
    o = cr.conv_ref(x, w, bias=b, mode="pixshuf", act0="sigmoid")
    _close(o["out0"][0], torch.sigmoid(F.pixel_shuffle(c2(w, b)[:, :12, 0], 2)))
    o = cr.conv_ref(x, w, bias=b, act0="relu", pool_hw=True, out0_f32=False)
    _close(o["out0"][0], F.avg_pool3d(F.relu(c2(w, b)), (1, 2, 2)))
    o = cr.conv_ref(x, w, bias=b, act0="relu", pixscale=mask)
    _close(o["out0"][0], F.relu(c2(w, b)) * mask)
    xs = x[..., :4, :4]
    o = cr.conv_ref(xs, w, bias=b, up_shift=1)
    _close(o["out0"][0], F.conv2d(xs[:, :, 0].repeat_interleave(2, 2).repeat_interleave(2, 3), w[:, :, 0], b, padding=1).unsqueeze(2))
    # even kernel extents pad K / 2 on the leading side only (the per-phase up-sampling convs)
    w22 = w[..., :2, :2]
    o = cr.conv_ref(x, w22, bias=b)
    _close(o["out0"][0], F.conv2d(F.pad(x[:, :, 0], (1, 0, 1, 0)), w22[:, :, 0], b).unsqueeze(2))


def test_hilo_is_the_sum_as_packed():
    r = _rng(5)
    xh, xl = cr.exact16(r, (1, 32, 4, 4, 4)), cr.exact16(r, (1, 32, 4, 4, 4)) * 2.0 ** -11
    wh, wl = cr.exact16(r, (32, 32, 3, 3, 3), -0.1, 0.1, 2.0 ** -12), cr.exact16(r, (32, 32, 3, 3, 3), -0.1, 0.1, 2.0 ** -12) * 2.0 ** -11
    o = cr.conv_ref(torch.cat([xh, xl], 1), None, hilo=(wh, wl))
    _close(o["out0"][0], V.conv(xh, wh + wl) + V.conv(xl, wh))
    # ... which is the product of the unsplit operands but for the W_lo x_lo term
    full = V.conv(xh + xl, wh + wl)
    assert float((o["out0"][0] - full).abs().max()) <= float(V.conv(xl.abs(), wl.abs()).max())


def test_statistics_blocks_partition_the_sample():
    """every position of a sample lies in exactly one block, a block is wave_px positions of one tile"""
    blk = cr.stat_blocks(1, 4, 16, 16, (3, 3, 1), 64)
    assert blk.shape == (16, 64) and sorted(blk.reshape(-1).tolist()) == list(range(4 * 16 * 16))
    first = blk[0].numpy()               # tile (0, 0, 0), its first 64 positions: d = 0, h < 8, w < 8
    assert set(first.tolist()) == {h * 16 + w_ for h in range(8) for w_ in range(8)}
    v = torch.arange(2 * 4 * 4 * 16 * 16, dtype=torch.float64).reshape(2, 4, 4, 16, 16) / 7
    want, bound = cr.stat_ref(v, (3, 3, 1), 64)
    assert want.shape == (2, 16, 4, 2) and abs(float(want[..., 0].sum() - v.sum())) < 1e-6 and abs(float(want[..., 1].sum() - (v * v).sum())) < 1e-3
    assert float((bound[..., 0] / want[..., 0].abs().clamp_min(1e-30)).max()) < 8.1 * cr.U32


# ------------------------------------------------------------------------------------------------ the bound is not vacuous
def _first_case(nonneg):
    """test_gpu_ops.py::test_conv_std's first case: 2 x 64 -> 128 channels, 32 x 32, 3x3, ReLU, fp32 output"""
    r = _rng(7)
    lo = 0.0 if nonneg else -1.0
    x, w, b = cr.exact16(r, (2, 64, 1, 32, 32), lo, 1.0), cr.exact16(r, (128, 64, 1, 3, 3), lo * 2.0 ** -5, 2.0 ** -5, 2.0 ** -11), cr.exact32(r, (128,), 0.5 * lo, 0.5)
    want, bound = cr.conv_ref(x, w, bias=b, act0="relu")["out0"]
    pre = F.conv2d(x[:, :, 0].float(), w[:, :, 0].float(), b.float(), padding=1)
    return want[:, :, 0], bound[:, :, 0], pre, b.float()


def _beyond(got, want, bound):
    return int(((got.double() - want).abs() > bound).sum())


@pytest.mark.parametrize("nonneg", [False, True], ids=["signed", "nonneg"])
def test_bound_holds_for_fp32_and_bites(nonneg):
    """torch's fp32 convolution of the same operands stays inside the bound, far inside; the four faults of the issue, injected into that fp32
    result, breach it: the output rounded through fp16, one sample alone rounded to fp16 before the activation, 5 % of the bias lost on one
    16 x 8 tile of 64 channels, one element 1 % off."""
    want, bound, pre, b = _first_case(nonneg)
    ok = F.relu(pre)
    ratio = float(((ok.double() - want).abs() / bound).max())
    print("largest |err| / bound of the fp32 convolution: %.4f" % ratio)
    assert _beyond(ok, want, bound) == 0 and ratio < 0.1
    assert _beyond(ok.half().float(), want, bound) > 1000
    one = pre.clone()
    one[1] = one[1].half().float()
    assert _beyond(F.relu(one), want, bound) > 500
    lost = pre.clone()
    lost[0, :64, 8:16, 16:32] -= 0.05 * b[:64, None, None]
    n = _beyond(F.relu(lost), want, bound)
    assert n > 1000 and _beyond(F.relu(lost)[0, :64, 8:16, 16:32], want[0, :64, 8:16, 16:32], bound[0, :64, 8:16, 16:32]) == n
    off = ok.clone()
    i = int(torch.argmax(ok.double() / bound))
    off.view(-1)[i] *= 1.01
    assert _beyond(off, want, bound) == 1


# ------------------------------------------------------------------------------------------------ dispatch coverage
@needs_clang
def test_every_case_reaches_its_row():
    """halo_plan() on every case's ConvParams (as cs_op_conv fills them) gives the case's tile configuration and chunk width; the launch meets
    launch_halo_cfg's static-shape condition for the case's static shape and for no other one of its (configuration, chunk, mode), or for none
    where the case names the dynamic kernel; extents are whole tiles, the tile fits, and launches that need it tile within one sample."""
    rows, shapes, plans = ph.dispatch_rows(), ph.static_shapes(), ph.plans()
    for c in cc.CASES:
        p = plans[c["name"]]
        hcfg, ck, mode, stv = c["row"]
        assert (p["hcfg"], p["ck"]) == (hcfg, ck), c["name"]
        assert ph.static_match(c, p, rows, shapes) == ([stv] if stv else []), c["name"]
        N, D, H, W = c["dims"]
        lw, lh, ld = p["lgT"]
        assert (p["nT"][0] << lw, p["nT"][1] << lh, p["nT"][2] << ld) == (W, H, D) and (1 << (lw + lh + ld)) <= p["BM"], c["name"]
        assert p["BM"] == cc.TILES[hcfg][1] and p["BN"] == cc.TILES[hcfg][2] and p["wave_px"] == cc.TILES[hcfg][3] and c["cout_pad"] % p["BN"] == 0
        per_tile = p["BM"] >> (lw + lh + ld)
        if mode in (cc.SPADE, cc.STDSTAT) or c["form"].startswith("spmul") or c["form"] == "pool":
            assert per_tile == 1, c["name"]
        if "tail" in c["name"]:
            assert per_tile > 1 and N * c.get("rep", 1) % per_tile != 0, c["name"]
        assert c["cout"] <= (c["cout_pad"] // 2 if mode in (cc.TBLEND, cc.SPADE) else c["cout_pad"]) and c["cout"] % 4 == 0
        assert (mode == cc.STDSTAT) == ("stat" in c["form"]) and (mode == cc.PIXSHUF) == (c["form"] == "pixshuf")
        assert (mode == cc.TBLEND) == c["form"].startswith("tblend") and (mode == cc.SPADE) == c["form"].startswith("spade")


def test_the_table_covers_the_dispatch():
    """The rows the cases name are exactly the launch_halo_cfg / launch_halo_st call sites of conv_halo.hip (HALO_CASE lines expanded, the
    dynamic form of every row that has one): a row added there without a case here fails this test, and so does a case whose row is gone."""
    rows = ph.dispatch_rows()
    mine = set(cc.rows())
    print("%d dispatch rows, %d cases" % (len(rows), len(cc.CASES)))
    assert mine == rows, "no case for %s; no call site for %s" % (sorted(rows - mine), sorted(mine - rows))
