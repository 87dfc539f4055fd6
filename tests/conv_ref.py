"""cs_op_conv restated in float64, with a bound on the error of every output element.

conv_ref() takes the logical arguments of hip_ops.conv (tensors in NCDHW, values that fp16 / fp32 hold exactly, so float64 sees what the kernel
reads) and returns, per output, `want` (float64) and `bound`: |got - want| <= bound must hold for every element of a correct kernel.  The bound
is a running forward error: every value is a pair (v, e) of the float64 value and a bound on |computed - v|, and every fp32 operation of
conv_halo_kernel.h / conv_epilogue.h maps the pairs of its operands to the pair of its result.  With u = 2^-24 (one fp32 rounding to nearest):

  sum of n terms      A sum of n terms t_i in any order and any grouping - the 32-deep MFMA steps, the chunks, the four K-slices of the split-K
                      tile, the bias, the residual - is within g(n - 1) sum |t_i| of the exact sum, g(m) = m u / (1 - m u) (Higham, Accuracy and
                      Stability of Numerical Algorithms, section 4.2: every term passes through at most n - 1 additions).  The products of two
                      fp16 values are exact in fp32.  The convolution: K = KD KH KW Cin products, so K - 1 additions; the split-K tile
                      (CFG_H_SK128x32: four waves take every fourth K-step, their partial sums meet in LDS and are added in wave order) changes
                      the grouping only.  The issue's form is (K + c) u mag with c the further additions; here c = 1 for the bias
                      (`ep_acc + ep_bias`, conv_epilogue.h) and the sum runs over K + 1 terms, so the accumulator-plus-bias is bounded by g(K + 1) mag,
                      mag = conv(|x|, |w|) + |bias|: one more than needed, which also covers the accumulator's start from 0.f.  The residual is a
                      separate addition below (it comes after the activation).
  a + b               e = (ea + eb) + u |a + b|          (the exact sum of the computed operands is within ea + eb; one rounding of a result
                                                          whose magnitude is at most |a + b| + ea + eb: the u (ea + eb) part is kept, as (1 + u))
  a * b               e = (|a| eb + |b| ea + ea eb)(1 + u) + u |a b|
  fma(a, b, c)        e = (|a| eb + |b| ea + ea eb + ec)(1 + u) + u |a b + c|      (one rounding)
  ReLU, LeakyReLU     lin_act = fma(slope, min(v, 0), max(v, 0)): Lipschitz constant max(1, |slope|) = 1 for the slopes in use; slope 0 and 1 are
                      exact, a leaky slope rounds once: e = ea + u |y|.  (apply_act's `v * slope` of the kernels with sigmoid / GELU: the same.)
  sigmoid             1 / (1 + __expf(-v)).  Slope at most 1/4.  __expf(t) = v_exp_f32(t log2(e)): the product rounds once and the constant is
                      within u of log2(e), each moves the exponent by at most u |t| log2(e), i.e. the result by u |t| relative; v_exp_f32 is good
                      to 1 ulp = 2 u.  So exp(-v) is within (2 |v| + 2) u relative, and through d s / d exp = -s^2, s^2 exp(-v) = s (1 - s):
                      (2 |v| + 2) u s (1 - s).  The addition rounds once (u s relative after the reciprocal), the division is within 2.5 ulp = 5 u:
                      e = ea / 4 + (2 |v| + 2) u s (1 - s) + 6 u s.
  GELU                0.5 v (1 + erff(v / sqrt 2)): slope at most 1.13 (at v = sqrt 2); erff within 4 ulp = 2^-21 absolute on a value below 1, times
                      0.5 |v|: 2^-22 |v| (test_gpu_parser_ops.py::test_dwconv_gelu); the argument's product rounds once and its constant is within u:
                      erf' (z) z <= 0.49, so u |v| covers both; the two products and the addition: 3 u |y|.
                      e = 1.13 ea + 2^-22 |v| + u |v| + 3 u |y|.
  store               fp32: the value is the result of an fp32 operation already; u |y| is added all the same (the issue's form).  fp16:
                      v_cvt_pk_f16_f32 rounds to nearest: 2^-11 (|y| + e) + 2^-25 (half the subnormal spacing 2^-24).  An fp32 result below
                      2^-126 may be flushed: + 2^-126.

The epilogue's forms, in the order of CONV_EPILOGUE_IMPL:
  STD        v = acc + bias; spmul: v = ((res - mean) rstd)(1 + v) (a subtraction, a product, an addition, a product); v = act0(v); v += res (not
             spmul; fp16 or fp32 residual, exact either way); v *= pixscale; pool_hw: ((a + c) + (b + d)) 0.25 or ((a + b) + (c + d)) 0.25 - three
             additions in either grouping, the product with 0.25 is exact; out0 = store(v); out1 = fp16(act1(fma(v, s2, t2))) from the
             unrounded v.
  TBLEND     v = ps (acc_mod + bias) + (1 - ps) acc_std (an addition, 1 - ps, two products and an addition; where hipcc contracts a product
             into the addition there is one rounding less); act0; v += res.
  SPADE      v = fma((res - mean) rstd, 1 + (acc_gamma + bias), acc_beta + bias2); act0.
  PIXSHUF    v = sigmoid(acc + bias), channel 4 c + 2 i + j to out[n][c][2 h + i][2 w + j], fp32.
hilo: activations [hi | lo], weights W_hi, W_lo as packed: acc = conv(x_hi, W_hi + W_lo) + conv(x_lo, W_hi), K = 3 C products.

Statistics (stat_out, MODE_STDSTAT): the kernel sums the values AS STORED (fp16-rounded where out0 is fp16), so stat_ref() takes the output the
launch stored and bounds the partial sums against the float64 sums of exactly those values: a lane adds the wave_px / 16 position blocks of its
segment, then four row shifts add the 16 lanes (ep_row_sum16): n = wave_px / 16 + 4 additions along any path, |sum - want| <= n u sum |v|, and
for the squares (one fma each: the product is not rounded on its own) n u sum v^2.  Block b of a sample (EP_BLK_V) is tile (b / blocks-per-tile, w
fastest, then h, d) and the wave_px consecutive positions (b % blocks-per-tile) wave_px ... of the tile's bit-field order (w, h, d)."""
import numpy as np
import torch
import torch.nn.functional as F

U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY32, HALF_SUB16 = 2.0 ** -126, 2.0 ** -25


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _add(a, b):
    v = a[0] + b[0]
    return v, (a[1] + b[1]) * (1 + U32) + U32 * v.abs()


def _mul(a, b):
    v = a[0] * b[0]
    return v, (a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1]) * (1 + U32) + U32 * v.abs()


def _fma(a, b, c):
    v = a[0] * b[0] + c[0]
    return v, (a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1] + c[1]) * (1 + U32) + U32 * v.abs()


def _exact(t):
    t = t.double()
    return t, torch.zeros_like(t)


def _act(a, act, slope):
    v, e = a
    if act in (None, "none"):
        return a
    if act == "relu":
        return F.relu(v), e
    if act == "lrelu":
        assert abs(slope) <= 1
        y = torch.where(v > 0, v, v * slope)
        return y, e + U32 * y.abs()
    if act == "sigmoid":
        s = torch.sigmoid(v)
        return s, e / 4 + (2 * v.abs() + 2) * U32 * s * (1 - s) + 6 * U32 * s
    if act == "gelu":
        y = F.gelu(v)
        return y, 1.13 * e + 2.0 ** -22 * v.abs() + U32 * v.abs() + 3 * U32 * y.abs()
    raise ValueError(act)


def _store(a, f32):
    v, e = a
    if f32:
        return v, e + U32 * v.abs() + TINY32
    return v, e + U16 * (v.abs() + e) + HALF_SUB16 + TINY32


def _chan(t):
    """[C] -> [1, C, 1, 1, 1]"""
    return t.double().view(1, -1, 1, 1, 1)


def _same_conv(x, w):
    """'same' convolution as the kernel pads it: K / 2 zeros on the leading side of every axis, K - 1 - K / 2 on the trailing one"""
    kd, kh, kw = w.shape[2:]
    pad = (kw // 2, kw - 1 - kw // 2, kh // 2, kh - 1 - kh // 2, kd // 2, kd - 1 - kd // 2)
    return F.conv3d(F.pad(x, pad), w)


def _up(t, shift):
    """the tensor addressed at (h >> shift, w >> shift)"""
    for _ in range(shift):
        t = t.repeat_interleave(2, 3).repeat_interleave(2, 4)
    return t


def _acc(x, w, b, hilo):
    """(conv + bias, its bound): g(K + 1) mag"""
    x, w = x.double(), None if w is None else w.double()
    if hilo is not None:
        whi, wlo = hilo[0].double(), hilo[1].double()
        c = whi.shape[1]
        xhi, xlo = x[:, :c], x[:, c:]
        v = _same_conv(xhi, whi + wlo) + _same_conv(xlo, whi)
        mag = _same_conv(xhi.abs(), whi.abs() + wlo.abs()) + _same_conv(xlo.abs(), whi.abs())
        K = 3 * c * int(np.prod(whi.shape[2:]))
    else:
        v, mag = _same_conv(x, w), _same_conv(x.abs(), w.abs())
        K = int(np.prod(w.shape[1:]))
    if b is not None:
        v, mag = v + _chan(b), mag + _chan(b).abs()
    return v, gamma(K + 1) * mag + TINY32


def conv_ref(x, w, *, bias=None, w2=None, bias2=None, mode="std", act0="none", slope0=0.0, res=None, res_shift=0, pixscale=None, stats=None,
             s2=None, t2=None, act1="none", slope1=0.0, out0=True, out0_f32=True, out1=False, up_shift=0, pool_hw=False, hilo=None):
    """x [N, Cin, D, H, W] (the stored input: up_shift up-samples it); w [Cout, Cin, KD, KH, KW]; mode "std" / "spmul" / "tblend" (w: the shared
    weights, w2: the modulated ones, bias theirs) / "spade" (w, bias: gamma; w2, bias2: beta) / "pixshuf"; res, pixscale [N, 1, D, H, W] and stats
    [N, C, 2] as the launch reads them; hilo = (W_hi, W_lo) with x = [hi | lo].  Returns {"out0": (want, bound), "out1": (want, bound)} in NCDHW
    (pixshuf: [N, 3, 2 H, 2 W]; pool_hw: out0 on the pooled grid)."""
    xs = _up(x.double(), up_shift)
    rr = None if res is None else _exact(_up(res, res_shift if mode in ("spade", "spmul") else 0))
    if stats is not None:
        mean, rstd = _exact(stats[..., 0][:, :, None, None, None]), _exact(stats[..., 1][:, :, None, None, None])
    one = None
    if mode == "tblend":
        ps = _exact(pixscale)
        m = _acc(xs, w2, bias, None)
        a = _acc(xs, w, None, None)
        one = _exact(torch.ones(()))
        v = _add(_mul(ps, m), _mul(_add(one, (-ps[0], ps[1])), a))
    elif mode == "spade":
        gm, bt = _acc(xs, w, bias, None), _acc(xs, w2, bias2, None)
        one = _exact(torch.ones(()))
        v = _fma(_mul(_add(rr, (-mean[0], mean[1])), rstd), _add(one, gm), bt)
    else:
        v = _acc(xs, w, bias, hilo)
        if mode == "spmul":
            one = _exact(torch.ones(()))
            v = _mul(_mul(_add(rr, (-mean[0], mean[1])), rstd), _add(one, v))
    v = _act(v, act0, slope0)
    if mode == "pixshuf":
        y, e = v
        return {"out0": _store((F.pixel_shuffle(y[:, :12, 0], 2), F.pixel_shuffle(e[:, :12, 0], 2)), True)}
    if rr is not None and mode in ("std", "tblend"):
        v = _add(v, rr)
    if pixscale is not None and mode == "std":
        v = _mul(v, _exact(pixscale))
    outs = {}
    if out1:
        a1 = v if s2 is None else _fma(v, _exact(_chan(s2)), _exact(_chan(t2)))
        outs["out1"] = _store(_act(a1, act1, slope1), False)
    if out0:
        if pool_hw:
            q = [(v[0][..., i::2, j::2], v[1][..., i::2, j::2]) for i in (0, 1) for j in (0, 1)]
            v = _add(_add(q[0], q[2]), _add(q[1], q[3]))
            v = (v[0] * 0.25, v[1] * 0.25)
        outs["out0"] = _store(v, out0_f32)
    return outs


def stat_blocks(N, D, H, W, lgT, wave_px):
    """position index [N, nblk, wave_px] -> flat (d, h, w) offset of the positions of every partial-statistics block, in EP_BLK_V's order"""
    lw, lh, ld = lgT
    tw, th, td = 1 << lw, 1 << lh, 1 << ld
    per_tile = (tw * th * td) // wave_px
    idx = []
    for tdi in range(D // td):
        for thi in range(H // th):
            for twi in range(W // tw):
                m = np.arange(tw * th * td)
                w_ = twi * tw + (m & (tw - 1)); h_ = thi * th + ((m >> lw) & (th - 1)); d_ = tdi * td + (m >> (lw + lh))
                idx.append(((d_ * H + h_) * W + w_).reshape(per_tile, wave_px))
    return torch.from_numpy(np.concatenate(idx, 0))


def stat_ref(stored, lgT, wave_px):
    """stored: the launch's out0 [N, C, D, H, W] as stored.  Returns (want, bound) [N, nblk, C, 2] for stat_out."""
    N, C, D, H, W = stored.shape
    blk = stat_blocks(N, D, H, W, lgT, wave_px)                  # [nblk, wave_px]
    v = stored.double().reshape(N, C, -1)[:, :, blk]              # [N, C, nblk, wave_px]
    n = wave_px // 16 + 4
    s, a, q = v.sum(-1), v.abs().sum(-1), (v * v).sum(-1)
    want = torch.stack([s, q], -1).permute(0, 2, 1, 3)
    bound = torch.stack([gamma(n) * a, gamma(n) * q], -1).permute(0, 2, 1, 3) + TINY32
    return want, bound


def exact16(r, shape, lo=-1.0, hi=1.0, step=2.0 ** -8):
    """uniform multiples of `step` in [lo, hi]: exact in fp16 for |values| <= 2^11 step"""
    n0, n1 = int(np.ceil(lo / step)), int(np.floor(hi / step))
    return torch.from_numpy(r.integers(n0, n1 + 1, size=shape).astype(np.float64) * step)


def exact32(r, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(r.uniform(lo, hi, size=shape).astype(np.float32).astype(np.float64))
