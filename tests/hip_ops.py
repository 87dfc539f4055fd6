"""Helpers that drive the operator-level C ABI (cs_op_*) from torch tensors; used by the -m gpu tests."""
import ctypes as C

import numpy as np
import torch

from canonswap_amd import _lib, pack

ACT = {"none": 0, "relu": 1, "lrelu": 2, "sigmoid": 3, "gelu": 4}


def op(name, *args):
    """A handle-less operator hook on torch's current stream (tensors: any GPU tensor, _lib.call)"""
    return _lib.call(name, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def strides_cl(t):
    """t: channels-last tensor [N, D, H, W, C] (possibly a strided view); element strides (sN, sD, sH, sW)."""
    assert t.stride(-1) == 1
    return t.stride(0), t.stride(1), t.stride(2), t.stride(3)


def conv(x, wpacked, cout_pad, cout, k, *, cin=None, bias=None, bias2=None, act0="none", slope0=0.0, res=None, res_shift=0,
         pixscale=None, ps_stride=1, out0=None, s2=None, t2=None, act1="none", slope1=0.0, out1=None, stats=None,
         mode=0, cfg=-1, up_shift=0, tile=(0, 0), out_dims=None, ck=0, xcd_map=None, ragged=False, hilo=False, stat_out=None, xf=None, ep_general=False, pool_hw=False):
    """x: [N, D, H, W, C] fp16 view (C contiguous). out0/out1/res: 5-D channels-last views. k = (KD, KH, KW)."""
    d = _lib.ConvDesc()
    N, D, H, W = out_dims if out_dims is not None else x.shape[:4]
    d.in_ = x.data_ptr()
    d.in_sN, d.in_sD, d.in_sH, d.in_sW = strides_cl(x)
    d.N, d.D, d.H, d.W = N, D, H, W
    d.Cin = cin if cin is not None else x.shape[4]
    d.up_shift = up_shift
    d.KD, d.KH, d.KW = k
    d.wgt = wpacked.data_ptr()
    d.Cout_pad, d.Cout = cout_pad, cout
    d.bias = 0 if bias is None else bias.data_ptr()
    d.bias2 = 0 if bias2 is None else bias2.data_ptr()
    d.act0, d.slope0 = ACT[act0], slope0
    if res is not None:
        d.res = res.data_ptr(); d.res_f32 = int(res.dtype == torch.float32); d.res_shift = res_shift
        d.res_sN, d.res_sD, d.res_sH, d.res_sW = strides_cl(res)
    d.pixscale = 0 if pixscale is None else pixscale.data_ptr()
    d.ps_stride = ps_stride
    if out0 is not None:
        d.out0 = out0.data_ptr(); d.out0_f32 = int(out0.dtype == torch.float32)
        if mode != 3:
            d.out0_sN, d.out0_sD, d.out0_sH, d.out0_sW = strides_cl(out0)
    d.s2 = 0 if s2 is None else s2.data_ptr()
    d.t2 = 0 if t2 is None else t2.data_ptr()
    d.act1, d.slope1 = ACT[act1], slope1
    if out1 is not None:
        d.out1 = out1.data_ptr()
        d.out1_sN, d.out1_sD, d.out1_sH, d.out1_sW = strides_cl(out1)
    d.stats = 0 if stats is None else stats.data_ptr()
    d.mode, d.cfg = mode, cfg
    d.tile_w, d.tile_h = tile
    d.ck = ck
    d.xcd_map = 0 if xcd_map is None else xcd_map + 1
    d.ragged = int(ragged)
    d.hilo = int(hilo)
    d.ep_general = int(ep_general)
    d.pool_hw = int(pool_hw)
    d.stat_out = 0 if stat_out is None else stat_out.data_ptr()
    if xf is not None:      # dict(kind, y, res, out, stats, gamma, beta, slope): fp32 volumes laid out like out0
        d.xf_kind = xf["kind"]
        for k in ("y", "res", "out", "stats", "gamma", "beta"):
            setattr(d, "xf_" + k, 0 if xf.get(k) is None else xf[k].data_ptr())
        d.xf_slope = xf.get("slope", 0.0)
    if -1 <= cfg <= 3:        # the independently written cross-check kernel (tests/csrc/conv_igemm.hip, test-only library)
        tl = _lib.load_test_lib()
        if tl.cs_test_conv_igemm(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
            raise RuntimeError("cs_test_conv_igemm failed: " + tl.cs_test_last_error().decode(errors="replace"))
        return
    op("cs_op_conv", C.byref(d))


def t_mask(x, wpacked, bias):
    """x: [N, H, W, 512] fp16 -> sigmoid(conv3x3(x) + bias[0]) as [N, H, W] fp32 (cs_op_t_mask writes at stride 4)"""
    N, H, W, _ = x.shape
    out = torch.full((N, H, W, 4), -1.0, dtype=torch.float32, device=x.device)
    op("cs_op_t_mask", x, wpacked, bias, out, N, H, W)
    return out


def pair_ragged(wpacked, cout_pad, cin, k):
    """In place: the engine's load-time re-packing of the last chunk of a Cin % 32 == 16 layer (paired taps)."""
    op("cs_op_pair_ragged", wpacked, cout_pad, (cin + 31) // 32, k[0], k[1], k[2])
    return wpacked


def packed_weight(w, cout_pad, device):
    return torch.from_numpy(pack.pack_conv(w.numpy() if isinstance(w, torch.Tensor) else w, cout_pad)).to(device)


def grid_sample(inp_hwdc, grid):
    N, H, W, D, Cc = inp_hwdc.shape
    out32 = torch.empty_like(inp_hwdc)
    out16 = torch.empty(inp_hwdc.shape, dtype=torch.float16, device=inp_hwdc.device)
    op("cs_op_grid_sample3d", inp_hwdc, grid, out32, out16, N, D, H, W)
    return out32, out16


def chan_stats(x, eps=1e-5, with_partials=False):
    """x: [N, P, C] fp16/fp32 contiguous -> [N, C, 2] = (mean, 1/sqrt(var + eps)), biased variance
    (with_partials: also the first pass's partial sums [N, blocks, C, 2])."""
    N, P, Cc = x.shape
    stats = torch.zeros(N, Cc, 2, dtype=torch.float32, device=x.device)
    part = torch.empty(_lib.call("cs_op_chan_stats_partial_floats", N, P, Cc), dtype=torch.float32, device=x.device)
    op("cs_op_chan_stats", x, int(x.dtype == torch.float32), N, P, Cc, eps, part, stats)
    return (stats, part.view(N, -1, Cc, 2)) if with_partials else stats


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- the motion extractor's kernels (cs_op_m_*; csrc/motion.hip).  Split outputs are fp16 [hi | lo] pairs per position.
M_PW1, M_PW2, M_DS = 0, 1, 2


def m_stem(img, w, b, g, be):
    """img fp32 [N, 3, HI, WI] -> x fp32 [N, HI/4, WI/4, 96]"""
    assert img.is_contiguous()
    N, _, HI, WI = img.shape
    x = torch.empty(N, HI // 4, WI // 4, 96, dtype=torch.float32, device=img.device)
    op("cs_op_m_stem", img, w, b, g, be, x, N, HI, WI)
    return x


def m_dwln(x, wt, b, g, be, y):
    """x fp32 [N, H, W, C] -> y (caller's fp16 buffer of N H W 2C values): split(LayerNorm(dwconv7x7(x)))"""
    assert x.is_contiguous() and y.is_contiguous()
    N, H, W, Cc = x.shape
    op("cs_op_m_dwln", x, wt, b, g, be, y, N, H, W, Cc)
    return y


def m_ln_s2d(x, g, be):
    """x fp32 [N, H, W, C] -> split fp16 [N, H/2, W/2, 8C], inner channel (dy*2+dx)*C + c of each half"""
    assert x.is_contiguous()
    N, H, W, Cc = x.shape
    y = torch.empty(N, H // 2, W // 2, 8 * Cc, dtype=torch.float16, device=x.device)
    op("cs_op_m_ln_s2d", x, g, be, y, N, H, W, Cc)
    return y


def m_grn(h, gamma, beta):
    """h fp32 [N, P, C] -> split fp16 [N, P, 2C]"""
    assert h.is_contiguous()
    N, P, Cc = h.shape
    sumsq = torch.empty(N * 16 * Cc, dtype=torch.float32, device=h.device)
    scale = torch.empty(N * Cc, dtype=torch.float32, device=h.device)
    out = torch.empty(N, P, 2 * Cc, dtype=torch.float16, device=h.device)
    op("cs_op_m_grn", h, gamma, beta, sumsq, scale, out, N, P, Cc)
    return out


def m_head(x, g, be, hw, hb):
    """x fp32 [N, P, 768] -> fp32 [N, 328]"""
    assert x.is_contiguous()
    N, P, _ = x.shape
    out = torch.empty(N, 328, dtype=torch.float32, device=x.device)
    op("cs_op_m_head", x, g, be, hw, hb, out, N, P)
    return out


def m_pointwise(engine, form, x, wpacked, bias, out, C_stage):
    """One of M's split-precision 1x1 convs through the engine's routing (cs_op_m_pointwise): x split fp16 [N, H, H, 2 Cin'],
    out fp32 [N, H, H, Cout] (form M_PW2: holds the residual and is updated in place)."""
    assert x.is_contiguous() and out.is_contiguous()
    N, H = x.shape[0], x.shape[1]
    engine._call("cs_op_m_pointwise", form, x, wpacked, bias, out, N, H, C_stage)
    return out


def split16(v):
    """fp32 [..., C] -> the split pair [..., 2C] = [hi | lo] as csrc/motion.hip stores it"""
    hi = v.half()
    return torch.cat([hi, (v - hi.float()).half()], -1)


def unsplit(y):
    """[..., 2C] fp16 pair -> (hi + lo) in float64, hi, lo"""
    c = y.shape[-1] // 2
    hi, lo = y[..., :c], y[..., c:]
    return hi.double() + lo.double(), hi, lo


# ---- the dense-motion kernels of W (cs_op_dm_*, cs_op_occ_finish; csrc/kernels.hip) and the engine's dense-motion buffers (cs_op_dm_read)
DM_COMP, DM_L0, DM_PRED, DM_LOGITS = 0, 1, 7, 8
DM_LW = (144, 128, 256, 512, 1024, 1024)          # concat width of level i (S = 64 >> i)


def dm_compress(f_hwdc, w, b, comp):
    """f fp32 [N, H, W, D, 32] -> comp (caller's fp16 buffer [N, D, H, W, 4])"""
    assert f_hwdc.is_contiguous() and comp.is_contiguous()
    N, Hh, Ww, D, _ = f_hwdc.shape
    op("cs_op_dm_compress", f_hwdc, w, b, comp, N, D, Hh, Ww)
    return comp


def dm_sparse(comp, kp_d, kp_s, out, N, shared_comp=False, shared_kps=False):
    """comp fp16 [1 or N, D, H, W, 4] -> out [N, D, H, W, ostride] fp16 view whose channels [0, 112) receive dm_sparse's output"""
    assert comp.is_contiguous() and kp_d.is_contiguous() and kp_s.is_contiguous()
    _, D, Hh, Ww, _ = comp.shape
    op("cs_op_dm_sparse", comp, int(shared_comp), kp_d, kp_s, int(shared_kps), out, out.stride(3), N, D, Hh, Ww)
    return out


def dm_softmax_warp(part, bias, kp_d, kp_s, inp, N, D, Hh, Ww, shared_kps=False, shared_in=False, out32=None, out16=None, deform=None):
    """part: compact-2 fp32 [N, D, H, W/4, 10, 22]; inp fp32 HWDC [1 or N, H, W, D, 32]"""
    assert part.is_contiguous() and inp.is_contiguous()
    op("cs_op_dm_softmax_warp", part, bias, kp_d, kp_s, int(shared_kps), inp, int(shared_in), out32, out16, deform, N, D, Hh, Ww)


def occ_finish(part, taps, bias, occ):
    """part fp32 [N, H, W, 64 (taps 49) or 16 (taps 7)] -> occ (caller's fp32 buffer [N, H, W])"""
    assert part.is_contiguous() and occ.is_contiguous()
    N, Hh, Ww, _ = part.shape
    op("cs_op_occ_finish", part, taps, float(bias), occ, N, Hh, Ww)
    return occ


def dm_read(engine, which, B):
    """One of the engine's dense-motion buffers as the last call left it (shapes: include/canonswap_hip.h, cs_op_dm_read)"""
    dev = engine.device
    if which == DM_COMP:
        out = torch.empty(B, 16, 64, 64, 4, dtype=torch.float16, device=dev)
    elif DM_L0 <= which < DM_L0 + 6:
        S = 64 >> (which - DM_L0)
        out = torch.empty(B, 16, S, S, DM_LW[which - DM_L0], dtype=torch.float16, device=dev)
    elif which == DM_PRED:
        out = torch.empty(B, 16, 64, 64, 144, dtype=torch.float16, device=dev)
    else:
        out = torch.empty(B, 16, 64, 16, 10, 22, dtype=torch.float32, device=dev)
    engine._call("cs_op_dm_read", which, B, out)
    return out


def compact2(p):
    """The mask conv's (kw, c) partials P [N, D, H, W, 7, 22] (P[.., x, kw, c]: input column x's product with tap kw) -> its compact-2
    hand-over [N, D, H, W/4, 10, 22], as the ST == 9 kw_out epilogue of conv_halo_kernel.h stores it: tile T owns input columns
    4 T .. 4 T + 3 and writes the 10 output columns o = 4 T - 3 + j it reaches, each the sum over its columns w' of P[4 T + w'][w' + 6 - j]
    (the terms with 0 <= kw <= 6), w' ascending.  Computed in p's dtype; sum over the tiles reaching o (T ascending) + bias = logit at o."""
    N, D, Hh, Ww = p.shape[:4]
    q = p.reshape(N, D, Hh, Ww // 4, 4, 7, 22)
    out = torch.zeros(N, D, Hh, Ww // 4, 10, 22, dtype=p.dtype, device=p.device)
    for j in range(10):
        for t in range(4):
            kw = t + 6 - j
            if 0 <= kw <= 6:
                out[:, :, :, :, j] += q[:, :, :, :, t, kw]
    return out


def compact2_logits(part, bias):
    """compact-2 partials [N, D, H, W/4, 10, 22] -> logits [N, D, H, W, 22] = bias + the sum over the (up to three) tiles reaching each column"""
    N, D, Hh, nT = part.shape[:4]
    Ww = 4 * nT
    l = torch.zeros(N, D, Hh, Ww + 6, 22, dtype=part.dtype, device=part.device)     # output column o at index o + 3
    for T in range(nT):
        l[:, :, :, 4 * T:4 * T + 10] += part[:, :, :, T]
    return l[:, :, :, 3:3 + Ww] + bias.to(part.dtype)


# ---- G's workspace (cs_op_g_read / cs_op_g_fill / cs_op_g_stop; layouts: include/canonswap_hip.h)
G_NAMES = ("x0", "x1", "a64", "a128", "a256", "h64", "dx64", "h128", "xs128", "dx128", "h1_128", "o128", "bs", "h256", "xs256", "dx256", "h1_256", "o256")
G_X0, G_X1, G_A64, G_A128, G_A256, G_H64, G_DX64, G_H128, G_XS128, G_DX128, G_H1_128, G_O128, G_BS, G_H256, G_XS256, G_DX256, G_H1_256, G_O256 = range(18)
G_STATS = 18
G_SHAPE = {G_X0: (64, 64, 512), G_X1: (64, 64, 512), G_A64: (64, 64, 1536), G_A128: (128, 128, 384), G_A256: (256, 256, 384), G_H64: (64, 64, 512),
           G_DX64: (64, 64, 512), G_H128: (128, 128, 512), G_XS128: (128, 128, 256), G_DX128: (128, 128, 256), G_H1_128: (128, 128, 256),
           G_O128: (128, 128, 256), G_BS: (256, 256, 64), G_H256: (256, 256, 256), G_XS256: (256, 256, 64), G_DX256: (256, 256, 64),
           G_H1_256: (256, 256, 64), G_O256: (256, 256, 64)}
G_SENTINEL = 0x7E5A


def g_read(engine, which, B, out=None):
    """One of G's buffers as the last cs_spade_decode left it: fp16 [B, H, W, C] (G_BS: as [B, 256, 256, 64]; after up_0's .bs launch view it as
    [B, 128, 128, 256]), G_STATS: fp32 [B, 1024], the slot handed out last ([B][C][2] in its first B C 2 values).  out: a buffer to reuse."""
    shape = (B, 1024) if which == G_STATS else (B,) + G_SHAPE[which]
    if out is None:
        out = torch.empty(shape, dtype=torch.float32 if which == G_STATS else torch.float16, device=engine.device)
    assert out.is_contiguous() and tuple(out.shape) == shape
    engine._call("cs_op_g_read", which, B, out)
    return out


def g_fill(engine, B):
    engine._call("cs_op_g_fill", B)


def g_decode(engine, seg, img, stop=0):
    """cs_spade_decode into the caller's img [B, 3, 512, 512] fp32, returning after its stop-th launch (0: all of it)"""
    assert seg.is_contiguous() and img.is_contiguous() and seg.dtype == img.dtype == torch.float32
    engine._call("cs_op_g_stop", stop)
    engine._call("cs_spade_decode", seg.shape[0], seg, img)
    return img


# ---- the volume workspace of F and R (cs_op_v_read / cs_op_v_fill / cs_op_v_stop; layouts: include/canonswap_hip.h)
V_NAMES = ("t0", "p0", "p1", "s0", "s1", "s2", "a0", "a1", "sp0", "sp1")
V_T0, V_P0, V_P1, V_S0, V_S1, V_S2, V_A0, V_A1, V_SP0, V_SP1 = range(10)
V_STATS = 10
V_SHAPE = {V_T0: (256, 256, 64), V_P0: (128, 128, 128), V_P1: (64, 64, 256), V_A0: (64, 64, 16, 32), V_A1: (64, 64, 16, 32)}
V_F32 = (V_S0, V_S1, V_S2, V_SP0, V_SP1)          # fp32 volumes [64, 64, 16, 32] (SP0 / SP1: as R's transform-staging path uses them)


def v_read(engine, which, B, out=None):
    """One buffer of the volume workspace as the last cs_extract_feature_3d / cs_refine left it: fp16 [B, H, W, C] or [B, 64, 64, 16, 32], the fp32
    volumes (SP0 / SP1 among them) fp32 [B, 64, 64, 16, 32]; V_STATS: fp32 [B, 1024], the slot handed out last ([B][32][2] in its first B 64 values)"""
    if which == V_STATS:
        shape, dt = (B, 1024), torch.float32
    elif which in V_F32:
        shape, dt = (B, 64, 64, 16, 32), torch.float32
    else:
        shape, dt = (B,) + V_SHAPE[which], torch.float16
    if out is None:
        out = torch.empty(shape, dtype=dt, device=engine.device)
    assert out.is_contiguous() and tuple(out.shape) == shape and out.dtype == dt
    engine._call("cs_op_v_read", which, B, out)
    return out


def v_fill(engine, B):
    engine._call("cs_op_v_fill", B)


def v_run(engine, entry, x, out, stop=0):
    """cs_extract_feature_3d (x: images [B, 3, 256, 256]) or cs_refine (x: volumes [B, 32, 16, 64, 64]) into the caller's out [B, 32, 16, 64, 64],
    returning after its stop-th launch (0: all of it)"""
    assert entry in ("cs_extract_feature_3d", "cs_refine") and x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype == torch.float32
    engine._call("cs_op_v_stop", stop)
    engine._call(entry, x.shape[0], x, out)
    return out


def conv_first(img, w, b, out16):
    """img fp32 [N, 3, H, W], w fp32 [64, 27], b fp32 [64] -> out16 (caller's fp16 buffer of N H W 64 values)"""
    assert img.is_contiguous() and w.is_contiguous() and out16.is_contiguous()
    N, _, Hh, Ww = img.shape
    op("cs_op_conv_first", img, w, b, out16, N, Hh, Ww)
    return out16


def norm_act(y, stats, gamma, beta, res=None, slope=0.01, out32=None, out16=None, s2=None, t2=None, period2=512, act2="none", slope2=0.0, split=False,
             per_n=None):
    """y fp32 [N, per_n] (channel = index % 32), stats fp32 [N, 32, 2] -> out32 / out16 (caller's buffers; split: out16 holds 2 N per_n values)"""
    assert y.is_contiguous()
    N = y.shape[0]
    op("cs_op_norm_act", y, stats, gamma, beta, res, slope, out32, out16, s2, t2, period2, ACT[act2], slope2, N, y[0].numel() if per_n is None else per_n,
       int(split))


def split16_op(x, out16):
    """x fp32, n values -> out16 (caller's fp16 buffer of 2 n values): [hi(32) | lo(32)] per voxel"""
    assert x.is_contiguous() and out16.is_contiguous()
    op("cs_op_split16", x, out16, x.numel())
    return out16


# ---- T's identity path (cs_op_t_*; csrc/kernels.hip t_style / t_modulate, the engine's per-slot weight sets and its blend layers)
T_WSET, T_STYLE = 0, 1


def t_style(idv, fc, style, nlayers):
    """idv fp32 [512], fc fp32 nlayers x (2 * (512 * 512 + 512)) -> style (caller's fp32 buffer of nlayers * 512 values)"""
    assert idv.is_contiguous() and fc.is_contiguous() and style.is_contiguous()
    op("cs_op_t_style", idv, fc, style, nlayers)
    return style


def t_modulate(wraw, style, packed):
    """wraw fp32 [512, 9, 512], style fp32 [512] -> the modulated rows of packed (caller's fp16 buffer [144, 1024, 32])"""
    assert wraw.is_contiguous() and style.is_contiguous() and packed.is_contiguous()
    op("cs_op_t_modulate", wraw, style, packed)
    return packed


def t_read(engine, layer, slot, which):
    """The slot's fused weight set fp16 [144, 1024, 32] (T_WSET) or the layer's last style vector fp32 [512] (T_STYLE) of a live engine"""
    out = torch.empty((144, 1024, 32), dtype=torch.float16, device=engine.device) if which == T_WSET else \
        torch.empty(512, dtype=torch.float32, device=engine.device)
    engine._call("cs_op_t_read", layer, slot, which, out)
    return out


def t_layer(engine, layer, slots, x16, res32, tmask, out16, out32):
    """One blend layer of T through the engine's routing (cs_op_t_layer): x16 fp16 [B, 64, 64, 512]; tmask fp32 [B, 64, 64, 4], out16 fp16 and
    (odd layers) res32 / out32 fp32 [B, 64, 64, 512] are the caller's buffers"""
    B = x16.shape[0]
    assert len(slots) == B and all(t is None or t.is_contiguous() for t in (x16, res32, tmask, out16, out32))
    arr = (C.c_int * B)(*[int(s) for s in slots])
    engine._call("cs_op_t_layer", layer, B, arr, x16, res32, tmask, out16, out32)


def t_rows(kind):
    """Row indices, in a fused [W ; w_mod] set of 1024 rows, of the 512 memory out-channels' shared (kind 0) or modulated (kind 1) rows"""
    o = np.arange(512)
    return ((o // 16) * 2 + kind) * 16 + o % 16
