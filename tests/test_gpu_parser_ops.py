"""The face parser's kernels alone (csrc/parser.hip through cs_op_parser_*; the patch-embedding and sequence-reduction convolutions through
cs_op_id_conv) against float64 on operands that fp16 holds exactly.  Every bound comes from the number formats and is derived in its test's
docstring: u16 = 2^-11 (one fp16 rounding), u32 = 2^-24 (one fp32 rounding)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hip_ops import op

pytestmark = pytest.mark.gpu
U16, U32 = 2.0 ** -11, 2.0 ** -24


def _rand(shape, seed, lo=-1.0, hi=1.0):
    r = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(r.uniform(lo, hi, size=shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ token GEMM
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["f16", "residual", "f32"])
@pytest.mark.parametrize("K,N", [(64, 64), (320, 1280), (1280, 320), (64, 1280), (1280, 64)])
@pytest.mark.parametrize("M", [1, 54, 300])
def test_gemm(M, K, N, mode):
    """fp16 operands are exact in float64; the K products are accumulated in fp32 in one order: |error| <= (K + 2) u32 sum |a w| in the worst
    case, the bias (and residual) additions add u32 |value| each, the fp16 store u16 |value|.  M = 1, 54, 300: a tail tile alone, a tail below
    one tile, two full tiles and a tail; N = 320 and 64 take the 64-column tile, 1280 the 128-column one.  Rows past M must stay untouched."""
    a, w, b = _rand((M, K), 1).half(), _rand((N, K), 2, -0.3, 0.3).half(), _rand((N,), 3)
    res = _rand((M, N), 4, -2, 2)
    pad = 3
    if mode == 0:
        out = torch.full((M + pad, N), float("nan"), dtype=torch.float16, device="cuda")
    else:
        out = torch.full((M + pad, N), float("nan"), dtype=torch.float32, device="cuda")
        if mode == 1:
            out[:M] = res.cuda()
    ad, wd, bd = a.cuda(), w.cuda(), b.cuda()
    op("cs_op_parser_gemm", ad, wd, bd, M, K, N, mode, out, 0, 0)
    want = a.double() @ w.double().T + b.double()
    mag = a.double().abs() @ w.double().abs().T + b.double().abs()
    if mode == 1:
        want, mag = want + res.double(), mag + res.double().abs()
    bound = (K + 4) * U32 * mag + (U16 if mode == 0 else U32) * want.abs() + 2.0 ** -26
    got = out.double().cpu()
    print("max error", float((got[:M] - want).abs().max()), "max bound", float(bound.max()))
    assert bool(((got[:M] - want).abs() <= bound).all())
    assert bool(torch.isnan(got[M:]).all())


@pytest.mark.parametrize("M,P", [(1, 1), (54, 27), (300, 100)])
def test_gemm_classifier_epilogue(M, P):
    """The classifier: 19 real classes in 64 packed rows, written as fp32 NCHW [M / P][19][P] - only the real classes: the 19 x P floats of every
    image are all that is written (the buffer ends there, with a sentinel behind it).  Bound as in test_gemm, K = 320."""
    K, N, L = 320, 64, 19
    a, w, b = _rand((M, K), 5).half(), _rand((N, K), 6, -0.3, 0.3).half(), _rand((N,), 7)
    w[L:] = 0
    out = torch.full((M // P * L * P + 64,), float("nan"), dtype=torch.float32, device="cuda")
    ad, wd, bd = a.cuda(), w.cuda(), b.cuda()
    op("cs_op_parser_gemm", ad, wd, bd, M, K, N, 3, out, P, L)
    want = (a.double() @ w.double().T + b.double())[:, :L].reshape(M // P, P, L).permute(0, 2, 1)
    mag = (a.double().abs() @ w.double().abs().T + b.double().abs())[:, :L].reshape(M // P, P, L).permute(0, 2, 1)
    got = out.double().cpu()
    assert bool(torch.isnan(got[M * L:]).all())
    assert bool(((got[:M * L].reshape(want.shape) - want).abs() <= (K + 4) * U32 * mag + U32 * want.abs()).all())


def test_gemm_refuses_bad_shapes():
    t = torch.zeros(64 * 64, dtype=torch.float16, device="cuda")
    o = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
    for M, K, N, mode, msg in ((0, 64, 64, 0, "bad arguments"), (4, 48, 64, 0, "K = 48"), (4, 64, 96, 0, "N = 96"), (4, 64, 64, 7, "no epilogue"),
                               (4, 64, 64, 3, "NCHW")):
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            op("cs_op_parser_gemm", t, t, None, M, K, N, mode, o, 0, 0)
    with pytest.raises(RuntimeError, match="cs_op_parser_gemm failed"):
        op("cs_op_parser_gemm", None, t, None, 4, 64, 64, 0, o, 0, 0)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C_", [64, 320, 512])
@pytest.mark.parametrize("M", [1, 54])
def test_layernorm(C_, M):
    """Two passes in fp32.  With u = max |x| of a token, n = C / 64 + 8 additions per sum: the mean is within dm = n u32 u; a centred value within
    dm + u32 |d|; the variance within (2 n u32 + dm^2 / var) relative, so 1 / sqrt(var + eps) within half of that plus 2 u32.  Hence
    |y - ref| <= |g| ((dm + 2 u32 |d|) / s + (|d| / s) (n u32 + dm^2 / (2 s^2) + 4 u32)) + 2 u32 (|y| + |b|), s = sqrt(var + eps); the fp16 copy adds
    u16 |y|.  Token 0 is the constant 0.75 (variance 0: the output is b exactly), token 1 is 1e3 times a random token, token 2 a random token
    around 1e3 (where a one-pass variance would lose everything)."""
    eps = 1e-5
    x = _rand((M, C_), 11, -2, 2)
    x[0] = 0.75
    if M > 2:
        x[1] *= 1e3
        x[2] = x[2] * 0.5 + 1e3
    g, b = _rand((C_,), 12, 0.5, 1.5), _rand((C_,), 13, -0.3, 0.3)
    o32 = torch.full((M + 1, C_), float("nan"), dtype=torch.float32, device="cuda")
    o16 = torch.full((M + 1, C_), float("nan"), dtype=torch.float16, device="cuda")
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    op("cs_op_parser_layernorm", xd, gd, bd, C.c_float(eps), M, C_, o32, o16)
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(1, keepdim=True)
    s = torch.sqrt(var + float(np.float32(eps)))
    want = d / s * g.double() + b.double()
    n = C_ // 64 + 8
    dm = n * U32 * x64.abs().amax(1, keepdim=True)
    bound = g.double().abs() * ((dm + 2 * U32 * d.abs()) / s + d.abs() / s * (n * U32 + dm * dm / (2 * s * s) + 4 * U32)) + 2 * U32 * (want.abs() + b.double().abs())
    got32, got16 = o32.double().cpu(), o16.double().cpu()
    print("max error", float((got32[:M] - want).abs().max()), "max bound", float(bound.max()))
    assert bool(((got32[:M] - want).abs() <= bound).all())
    assert bool(((got16[:M] - want).abs() <= bound + U16 * want.abs()).all())
    assert torch.equal(o32[0].cpu(), b)
    assert torch.equal(o16[:M].cpu(), o32[:M].half().cpu())
    assert bool(torch.isnan(got32[M:]).all()) and bool(torch.isnan(got16[M:]).all())


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("Nq,Nk,heads,d", [(54, 6, 5, 64), (300, 40, 2, 64), (256, 256, 8, 64), (54, 6, 2, 32)])
def test_attention(Nq, Nk, heads, d):
    """q and k are normal with standard deviation 1.6, so the scores (d = 64: standard deviation 20) reach about +-60 to 80: a softmax without the
    row maximum overflows.  Error: a score is within es = (d + 2) u32 sum |q k|; a probability within P (u16 + 2 max es + 2^-20 + (Nk + 4) u32)
    + 2^-25 (fp16 rounding, the scores' error through exp twice - numerator and sum -, expf, the sum's own additions, fp16's subnormal step);
    the output adds (Nk + 34) u32 sum P |v| for its accumulation and u16 |out| for the store.  With Nk = 6 the keys 6 .. 31 of the MFMA tile are
    padding: the memory behind each sample's six rows holds the next sample's rows, and NaN behind the last one."""
    B, Cc = 2, heads * d
    g = torch.Generator().manual_seed(100 + Nq + Nk)
    q = (torch.randn(B, Nq, Cc, generator=g) * 1.6).half()
    kv = torch.cat([(torch.randn(B, Nk, Cc, generator=g) * 1.6), torch.rand(B, Nk, Cc, generator=g) * 2 - 1], dim=2).half()
    kvbuf = torch.full((B * Nk + 64, 2 * Cc), float("nan"), dtype=torch.float16, device="cuda")
    kvbuf[:B * Nk] = kv.reshape(B * Nk, 2 * Cc).cuda()
    out = torch.full((B * Nq + 1, Cc), float("nan"), dtype=torch.float16, device="cuda")
    qd = q.cuda()
    op("cs_op_parser_attention", qd, kvbuf, out, B, Nq, Nk, heads, d)
    sp = lambda t: t.double().reshape(B, -1, heads, d).transpose(1, 2)
    qq, kk, vv = sp(q), sp(kv[..., :Cc]), sp(kv[..., Cc:])
    sc = qq @ kk.transpose(-1, -2)
    print("score range", float(sc.min()), float(sc.max()))
    assert float(sc.abs().max()) > (50 if d == 64 else 25)
    pr = torch.softmax(sc, -1)
    want = (pr @ vv).transpose(1, 2).reshape(B, Nq, Cc)
    es = ((d + 2) * U32 * (qq.abs() @ kk.abs().transpose(-1, -2))).amax(-1, keepdim=True)
    rel = U16 + 2 * es + 2.0 ** -20 + (Nk + 4) * U32 + (Nk + 34) * U32
    bound = (rel * (pr @ vv.abs()) + 2.0 ** -25 * vv.abs().sum(-2, keepdim=True)).transpose(1, 2).reshape(B, Nq, Cc) + U16 * want.abs() + 2.0 ** -25
    got = out.double().cpu()
    assert bool(torch.isnan(got[B * Nq:]).all())
    err = (got[:B * Nq].reshape(B, Nq, Cc) - want).abs()
    print("max error", float(err.max()), "max bound", float(bound.max()))
    assert not bool(torch.isnan(err).any())
    assert bool((err <= bound).all())


def test_attention_refuses_what_it_cannot_run():
    t = torch.zeros(1024, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="257 keys"):
        op("cs_op_parser_attention", t, t, t, 1, 4, 257, 1, 64)
    with pytest.raises(RuntimeError, match="head dimension 48"):
        op("cs_op_parser_attention", t, t, t, 1, 4, 4, 1, 48)
    with pytest.raises(RuntimeError, match="cs_op_parser_attention failed"):
        op("cs_op_parser_attention", t, None, t, 1, 4, 4, 1, 64)


# ------------------------------------------------------------------------------------------------ depth-wise conv + GELU
@pytest.mark.parametrize("Cc", [256, 1280])
@pytest.mark.parametrize("H,W", [(2, 3), (16, 24)])
def test_dwconv_gelu(H, W, Cc):
    """fp16 input, fp32 weights (exact in float64), nine fused multiply-adds on the bias in fp32: the sum is within 10 u32 (sum |v w| + |b|);
    GELU's slope is at most 1.13; erff is within 4 ulp (2^-21), the two products of 0.5 v (1 + erf) add 3 u32 |y|, the store u16 |y|.  The 2 x 3
    map is all border; on 16 x 24 the border ring and the interior are asserted one after the other."""
    B = 2
    x = _rand((B, H, W, Cc), 21, -2, 2).half()
    w, b = _rand((9, Cc), 22, -0.6, 0.6), _rand((Cc,), 23, -0.2, 0.2)
    out = torch.full((B * H * W + 1, Cc), float("nan"), dtype=torch.float16, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    op("cs_op_parser_dwgelu", xd, wd, bd, out, B, H, W, Cc)
    x64 = x.double().permute(0, 3, 1, 2)
    w64 = w.double().T.reshape(Cc, 1, 3, 3)
    v = F.conv2d(x64, w64, b.double(), padding=1, groups=Cc)
    mag = F.conv2d(x64.abs(), w64.abs(), b.double().abs(), padding=1, groups=Cc)
    want = F.gelu(v)
    bound = 1.13 * 10 * U32 * mag + 2.0 ** -22 * v.abs() + 3 * U32 * want.abs() + U16 * want.abs() + 2.0 ** -25
    got = out.double().cpu()
    assert bool(torch.isnan(got[B * H * W:]).all())
    ok = (got[:B * H * W].reshape(B, H, W, Cc).permute(0, 3, 1, 2) - want).abs() <= bound
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool(ok[:, :, border].all()), "border"
    assert bool(ok[:, :, ~border].all()), "interior"


# ------------------------------------------------------------------------------------------------ the convolutions (identity.hip's kernel)
@pytest.mark.parametrize("case", ["sr8", "sr4", "sr2", "stem7", "patch3"])
def test_patch_and_sr_convs(case):
    """The sequence-reduction convs (K = stride = 8, 4, 2, no padding) to the 2 x 3 key map of a 64 x 96 input, the 7 x 7 / 4 / 3 stem on 3 real +
    29 zero channels and a 3 x 3 / 2 / 1 patch embedding, through cs_op_id_conv: K^2 Cin products in four partial sums added in order,
    |error| <= (K^2 Cin + 4) u32 sum |a w| + u32 |value| (fp32 output)."""
    from canonswap_amd import pack
    N, IH, IW, Cin, real, Cout, K, stride, padn = {
        "sr8": (2, 16, 24, 64, 64, 64, 8, 8, 0), "sr4": (2, 8, 12, 128, 128, 128, 4, 4, 0), "sr2": (2, 4, 6, 320, 320, 320, 2, 2, 0),
        "stem7": (2, 64, 96, 32, 3, 64, 7, 4, 3), "patch3": (2, 16, 24, 64, 64, 128, 3, 2, 1)}[case]
    x = _rand((N, real, IH, IW), 31).half()
    w = _rand((Cout, real, K, K), 32, -0.2, 0.2)
    b = _rand((Cout,), 33)
    xin = torch.zeros((N, IH, IW, Cin), dtype=torch.float16)
    xin[..., :real] = x.permute(0, 2, 3, 1)
    xin = xin.cuda()
    wp = torch.from_numpy(pack.pack_id_conv(w.numpy())).cuda()
    assert wp.shape == (K * K, Cout, Cin)
    OH, OW = (IH + 2 * padn - K) // stride + 1, (IW + 2 * padn - K) // stride + 1
    out = torch.full((N * OH * OW + 1, Cout), float("nan"), dtype=torch.float32, device="cuda")
    bd = b.cuda()
    op("cs_op_id_conv", xin, 0, N, IH, IW, Cin, K, stride, padn, wp, bd, Cout, None, out, 1)
    x64, w64 = x.double(), w.half().double()
    want = F.conv2d(x64, w64, b.double(), stride=stride, padding=padn)
    mag = F.conv2d(x64.abs(), w64.abs(), b.double().abs(), stride=stride, padding=padn)
    assert want.shape[2:] == (OH, OW)
    got = out.double().cpu()
    assert bool(torch.isnan(got[N * OH * OW:]).all())
    err = (got[:N * OH * OW].reshape(N, OH, OW, Cout).permute(0, 3, 1, 2) - want).abs()
    assert bool((err <= (K * K * Cin + 4) * U32 * mag + U32 * want.abs()).all())


# ------------------------------------------------------------------------------------------------ decode head: up-sample and add
def _upadd(ps, B, H, W, D):
    out = torch.full((B * H * W + 1, D), float("nan"), dtype=torch.float16, device="cuda")
    dev = [p.contiguous().cuda() for p in ps]
    op("cs_op_parser_upadd", dev[0], dev[1], dev[2], dev[3], out, B, H, W, D)
    assert bool(torch.isnan(out[B * H * W:]).all())
    return out[:B * H * W].reshape(B, H, W, D).cpu()


def test_upadd_values():
    """2 x 3 -> 16 x 24 (and 4 x 6, 8 x 12): each bilinear value is three lerps in fp32 (a + f (b - a): 3 roundings each, |intermediate| <= 3 max
    |tap|), the four terms are added in order: |error| <= 40 u32 sum_s max |taps of s| + u16 |y| + 2^-25.  The weights are ATen's fp32 values:
    ratios 1/2, 1/4, 1/8 and the source coordinates are exact in fp32."""
    B, H, W, D = 2, 16, 24, 8
    ps = [_rand((B, H >> s, W >> s, D), 40 + s, -2, 2) for s in range(4)]
    got = _upadd(ps, B, H, W, D).double()
    up = lambda t: F.interpolate(t.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    want = F.relu(sum(up(p) for p in ps))
    amax = lambda t: F.max_pool2d(F.pad(t.double().abs().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate"), 3, 1)
    mag = sum(F.interpolate(amax(p), size=(H, W), mode="nearest").permute(0, 2, 3, 1) for p in ps)
    err = (got - want).abs()
    print("max error", float(err.max()), "max bound", float((40 * U32 * mag + U16 * want.abs()).max()))
    assert bool((err <= 40 * U32 * mag + U16 * want.abs() + 2.0 ** -25).all())


def test_upadd_clamped_taps():
    """Structure at the rim.  With only the coarsest map non-zero (ratio 8, 2 x 3 -> 16 x 24): rows 0 .. 3 have source coordinate max(., 0) = 0, so
    they read row 0 alone with weight exactly 1; rows 12 .. 15 have both taps clamped to row 1; the same for columns 0 .. 3 and 20 .. 23.  So the
    four corners' 4 x 4 blocks equal fp16(relu(corner value)) exactly, the top rows do not change when row 1 changes, the bottom rows do not
    change when row 0 changes."""
    B, H, W, D = 1, 16, 24, 4
    z = [torch.zeros(B, H >> s, W >> s, D) for s in range(3)]
    p3 = _rand((B, 2, 3, D), 50, -2, 2)
    got = _upadd(z + [p3], B, H, W, D)
    for (y, x), (ys, xs) in zip(((0, 0), (0, 2), (1, 0), (1, 2)), ((slice(0, 4), slice(0, 4)), (slice(0, 4), slice(20, 24)), (slice(12, 16), slice(0, 4)),
                                                                    (slice(12, 16), slice(20, 24)))):
        want = F.relu(p3[0, y, x]).half()
        assert torch.equal(got[0, ys, xs], want.expand(4, 4, D)), (y, x)
    other = p3.clone()
    other[:, 1] = _rand((B, 3, D), 51, -2, 2)
    assert torch.equal(_upadd(z + [other], B, H, W, D)[0, :4], got[0, :4])
    other = p3.clone()
    other[:, 0] = _rand((B, 3, D), 52, -2, 2)
    assert torch.equal(_upadd(z + [other], B, H, W, D)[0, 12:], got[0, 12:])
    mid = F.relu(F.interpolate(p3.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1))
    assert bool(((got.double() - mid).abs() <= 40 * U32 * 2 + U16 * mid.abs() + 2.0 ** -25).all())


def test_input_layout():
    """pixel_values fp32 NCHW -> fp16 [B][H][W][32]: the three channels rounded once, 29 zeros."""
    B, H, W = 2, 5, 7
    pv = _rand((B, 3, H, W), 60, -2.5, 2.5)
    out = torch.full((B * H * W + 1, 32), float("nan"), dtype=torch.float16, device="cuda")
    pd = pv.cuda()
    op("cs_op_parser_input", pd, out, B, H, W)
    got = out[:B * H * W].reshape(B, H, W, 32).cpu()
    assert torch.equal(got[..., :3], pv.permute(0, 2, 3, 1).half()) and not bool(got[..., 3:].any())
    assert bool(torch.isnan(out[B * H * W:]).all())
