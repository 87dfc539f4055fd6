// The operator-level hooks of the C ABI (cs_op_*): single kernels without an engine, single layers through the engine's routing, and the engine's
// buffers as the last call left them.  The unit parity tests enter here.
#include "engine.h"

// ---- operator level
// The launch is prepared as the engine prepares its own: mk() on a layer built from the descriptor, then - for conv_halo - the engine's launch plan
// (conv_plan.h) under the descriptor's explicit overrides.  Nothing here decides a default.
extern "C" int cs_op_conv(const cs_conv_desc* d, void* stream)
{
    ConvL L;
    L.w = (const half_t*)d->wgt; L.b = d->bias;
    L.Cin = d->Cin; L.Cout_pad = d->Cout_pad; L.Cout = d->Cout; L.KD = d->KD; L.KH = d->KH; L.KW = d->KW;
    ConvCall c = mk(L, d->in, td(nullptr, d->in_sN, d->in_sD, d->in_sH, d->in_sW), d->N, d->D, d->H, d->W, d->up_shift);
    ConvParams& p = c.p;
    p.bias2 = d->bias2; p.act0 = d->act0; p.slope0 = d->slope0;
    p.res = td((void*)d->res, d->res_sN, d->res_sD, d->res_sH, d->res_sW); p.res_f32 = d->res_f32; p.res_shift = d->res_shift;
    p.pixscale = d->pixscale; if (d->ps_stride) p.ps_stride = d->ps_stride;
    p.out0 = td(d->out0, d->out0_sN, d->out0_sD, d->out0_sH, d->out0_sW); p.out0_f32 = d->out0_f32;
    p.s2 = d->s2; p.t2 = d->t2; p.act1 = d->act1; p.slope1 = d->slope1;
    p.out1 = td(d->out1, d->out1_sN, d->out1_sD, d->out1_sH, d->out1_sW);
    p.stats = d->stats;
    p.hilo = d->hilo; p.stat_out = d->stat_out; p.pool_hw = d->pool_hw;
    if (d->xf_kind) {       // transform staging (vol32): the fp32 source volumes share out0's strides
        p.xf_kind = d->xf_kind;
        p.xf_y = td((void*)d->xf_y, d->out0_sN, d->out0_sD, d->out0_sH, d->out0_sW);
        p.xf_res = td((void*)d->xf_res, d->out0_sN, d->out0_sD, d->out0_sH, d->out0_sW);
        p.xf_out = td((void*)d->xf_out, d->out0_sN, d->out0_sD, d->out0_sH, d->out0_sW);
        p.xf_stats = d->xf_stats; p.xf_gamma = d->xf_gamma; p.xf_beta = d->xf_beta; p.xf_slope = d->xf_slope;
    }
    c.mode = d->mode;
    if (d->mode == 5) { c.mode = MODE_STD; p.spmul = 1; }     // out0 = act0(IN(res) (1 + conv + bias)): ConvParams::spmul
    if (d->cfg == CFG_VOL32) return launch_vol32(p, (hipStream_t)stream);
    if (d->cfg == CFG_WIDE) return launch_conv_wide(p, c.mode, (hipStream_t)stream);
    if (d->cfg == CFG_LAT) return launch_conv_lat(p, c.mode, (hipStream_t)stream);
    if (d->cfg >= 10 || d->cfg == -2) {      // conv_halo: the given tile configuration, or the engine's
        const HaloPlan plan = halo_plan(p, c.mode, d->cfg >= 10 ? d->cfg : -1, d->tile_w, d->tile_h, c.cg_ck64);
        // set_tile() takes nT = extent / tile and the kernel stores whole tiles: the remainder of an extent that is no multiple of its tile would
        // stay unwritten (the engine's layers are powers of two; here the caller chooses)
        if ((p.nTW << p.lgTW) != p.W || (p.nTH << p.lgTH) != p.H || (p.nTD << p.lgTD) != p.D) {
            cs_set_error("cs_op_conv: output extent %d x %d x %d is not a whole number of %d x %d x %d tiles", p.D, p.H, p.W, 1 << p.lgTD, 1 << p.lgTH, 1 << p.lgTW);
            return -1;
        }
        if (d->xcd_map > 0) p.xcd_map = d->xcd_map - 1;
        p.ragged = d->ragged; p.ep_general = d->ep_general;
        return launch_conv_halo(p, plan.hcfg, d->ck ? d->ck : plan.ck, c.mode, (hipStream_t)stream);
    }
    cs_set_error("cs_op_conv: cfg %d is not a conv_halo configuration (the conv_igemm cross-check kernel lives in the test-only library)", d->cfg);
    return -1;
}

extern "C" int cs_op_resblock3d(const void* a, const float* x, float* out0, void* out1, int N, int H, int W, const void* w1, const void* w2,
                                const float* b1, const float* b2, const float* s2, const float* t2, int act1, float slope1, void* stream)
{
    ResBlock3dCall c;
    c.a = (const half_t*)a; c.x = x; c.out0 = out0; c.out1 = (half_t*)out1;
    c.sN = (long)H * W * 512; c.sH = (long)W * 512; c.sW = 512;
    c.w1 = (const half_t*)w1; c.w2 = (const half_t*)w2; c.b1 = b1; c.b2 = b2; c.s2 = s2; c.t2 = t2; c.act1 = act1; c.slope1 = slope1;
    c.N = N; c.H = H; c.W = W;
    return launch_vol32_fused(c, (hipStream_t)stream);
}

extern "C" int cs_op_t_mask(const void* x, const void* wpacked, const float* bias, float* tmask, int N, int H, int W, void* stream)
{
    return launch_t_mask((const half_t*)x, (const half_t*)wpacked, bias, tmask, N, H, W, (hipStream_t)stream);
}

// ---- operator level: T's per-identity precompute (csrc/kernels.hip) without an engine, what cs_set_identity left in an engine (cs_op_t_read), and
// one blend layer of T on the caller's buffers through the engine's routing (cs_op_t_layer)
extern "C" int cs_op_t_style(const float* id, const float* fc, float* style, int nlayers, void* stream)
{
    if (!id || !fc || !style || nlayers < 1) { cs_set_error("cs_op_t_style: bad arguments"); return -1; }
    return launch_t_style(id, fc, style, nlayers, (hipStream_t)stream);
}

extern "C" int cs_op_t_modulate(const float* wraw, const float* style, void* packed, void* stream)
{
    if (!wraw || !style || !packed) { cs_set_error("cs_op_t_modulate: bad arguments"); return -1; }
    return launch_t_modulate(wraw, style, (half_t*)packed, 0, (hipStream_t)stream);
}

extern "C" int cs_op_t_read(cs_engine* e, int layer, int slot, int which, void* dst, void* stream)
{
    if (!e || !e->finalized) { cs_set_error("cs_op_t_read: engine not finalized"); return -1; }
    if (!dst) { cs_set_error("cs_op_t_read: null destination"); return -1; }
    if (layer < 0 || layer >= 14) { cs_set_error("cs_op_t_read: layer %d outside [0, 14)", layer); return -1; }
    if (slot < 0 || slot >= MAX_SLOTS) { cs_set_error("cs_op_t_read: identity slot %d outside [0, %d)", slot, MAX_SLOTS); return -1; }
    if (!e->slot_set[slot]) { cs_set_error("cs_op_t_read: cs_set_identity has not been called for slot %d", slot); return -1; }
    DevGuard guard(e->dev);
    if (which == CS_T_WSET) return copy_dd(dst, e->t_l[layer].wset[slot], T_FUSED_ELEMS * sizeof(half_t), (hipStream_t)stream);
    if (which == CS_T_STYLE) return copy_dd(dst, e->style + layer * 512, 512 * sizeof(float), (hipStream_t)stream);
    cs_set_error("cs_op_t_read: no buffer %d", which);
    return -1;
}

extern "C" int cs_op_t_layer(cs_engine* e, int layer, int B, const int* slots, const void* in16, const float* res32, float* tmask_out, void* out16,
                             float* out32, void* stream)
{
    ENTER(e, B);
    if (layer < 0 || layer >= 14) { cs_set_error("cs_op_t_layer: layer %d outside [0, 14)", layer); return -1; }
    const bool conv2 = layer % 2 == 1;
    if (!slots || !in16 || !tmask_out || !out16 || (conv2 && (!res32 || !out32)) || (!conv2 && (res32 || out32))) {
        cs_set_error("cs_op_t_layer: bad arguments (conv2 layers take res32 and out32, conv1 layers neither)");
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    bool mixed = false;
    TRY(t_slots(e, B, slots, &mixed, st));
    return t_layer(e, layer, B, slots, mixed, (const half_t*)in16, res32, tmask_out, (half_t*)out16, out32, st);
}

extern "C" int cs_op_pair_ragged(void* w, int Cout_pad, int nchunks, int KD, int KH, int KW, void* stream)
{
    return launch_pair_ragged((half_t*)w, Cout_pad, nchunks, KD, KH, KW, (hipStream_t)stream);
}

extern "C" int cs_op_grid_sample3d(const float* in_hwdc, const float* grid, float* out32, void* out16, int N, int D, int H, int W,
                                   void* stream)
{
    return launch_grid_sample(in_hwdc, grid, out32, (half_t*)out16, N, D, H, W, (hipStream_t)stream);
}

extern "C" long cs_op_chan_stats_partial_floats(int N, long P, int C) { return chan_stats_partial_floats(N, P, C); }

extern "C" int cs_op_chan_stats(const void* x, int is_f32, int N, long P, int C, float eps, float* partials, float* stats, void* stream)
{
    return launch_chan_stats(x, is_f32, N, P, C, eps, partials, stats, (hipStream_t)stream);
}

// ---- operator level: the motion extractor's kernels (csrc/motion.hip) without an engine, and its 1x1 convs through the engine's routing
extern "C" int cs_op_m_stem(const float* img, const float* w, const float* b, const float* g, const float* be, float* x, int N, int HI, int WI,
                            void* stream)
{
    return launch_m_stem(img, w, b, g, be, x, N, HI, WI, (hipStream_t)stream);
}

extern "C" int cs_op_m_dwln(const float* x, const float* wt, const float* b, const float* g, const float* be, void* y, int N, int H, int W, int C,
                            void* stream)
{
    return launch_m_dwln(x, wt, b, g, be, (half_t*)y, N, H, W, C, (hipStream_t)stream);
}

extern "C" int cs_op_m_ln_s2d(const float* x, const float* g, const float* be, void* y, int N, int H, int W, int C, void* stream)
{
    return launch_m_ln_s2d(x, g, be, (half_t*)y, N, H, W, C, (hipStream_t)stream);
}

extern "C" int cs_op_m_grn(const float* h, const float* gamma, const float* beta, float* sumsq, float* scale, void* out, int N, int P, int C,
                           void* stream)
{
    return launch_m_grn(h, gamma, beta, sumsq, scale, (half_t*)out, N, P, C, (hipStream_t)stream);
}

extern "C" int cs_op_m_head(const float* x, const float* g, const float* be, const float* hw, const float* hb, float* out, int N, int P, void* stream)
{
    return launch_m_head(x, g, be, hw, hb, out, N, P, (hipStream_t)stream);
}

extern "C" int cs_op_m_pointwise(cs_engine* e, int form, const void* in, const void* wpacked, const float* bias, float* out, int N, int H, int C,
                                 void* stream)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    if ((C != 96 && C != 192 && C != 384 && C != 768) || form < M_PW1 || form > M_DS || (form == M_DS && C == 768) || N < 1 || H < 1) {
        cs_set_error("cs_op_m_pointwise: no such layer (form %d, C %d, N %d, H %d)", form, C, N, H);
        return -1;
    }
    DevGuard guard(e->dev);
    ConvL L = m_pointwise_layer(form, C);      // the geometry cs_finalize_weights gives M's layers
    L.w = (const half_t*)wpacked; L.b = bias;
    L.name = form == M_PW1 ? "m_pw1" : form == M_PW2 ? "m_pw2" : "m_ds";
    ConvCall c = m_pointwise(L, form, (const half_t*)in, out, N, H, C);
    return go(e, c, (hipStream_t)stream);
}

// ---- operator level: the dense-motion kernels of W (csrc/kernels.hip) without an engine, and the engine's dense-motion buffers as the last
// call left them (cs_op_dm_read): the tests run W through the public entry points and check each layer on the engine's own input
extern "C" int cs_op_dm_compress(const float* f_hwdc, const float* w, const float* b, void* comp, int N, int D, int H, int W, void* stream)
{
    if (!f_hwdc || !w || !b || !comp || N < 1 || D < 1 || H < 1 || W < 1) { cs_set_error("cs_op_dm_compress: bad arguments"); return -1; }
    return launch_dm_compress(f_hwdc, w, b, (half_t*)comp, N, D, H, W, (hipStream_t)stream);
}

extern "C" int cs_op_dm_sparse(const void* comp, int shared_comp, const float* kp_d, const float* kp_s, int shared_kps, void* out, int ostride,
                               int N, int D, int H, int W, void* stream)
{
    if (!comp || !kp_d || !kp_s || !out || N < 1 || D < 2 || H < 2 || W < 2 || ostride < 112) { cs_set_error("cs_op_dm_sparse: bad arguments"); return -1; }
    return launch_dm_sparse((const half_t*)comp, kp_d, kp_s, (half_t*)out, ostride, N, D, H, W, (hipStream_t)stream, shared_comp != 0, shared_kps != 0);
}

extern "C" int cs_op_dm_softmax_warp(const float* part, const float* bias, const float* kp_d, const float* kp_s, int shared_kps, const float* in_hwdc,
                                     int shared_in, float* out32, void* out16, float* deform, int N, int D, int H, int W, void* stream)
{
    if (!part || !bias || !kp_d || !kp_s || !in_hwdc || N < 1 || H < 2) { cs_set_error("cs_op_dm_softmax_warp: bad arguments"); return -1; }
    if (W & 3) { cs_set_error("cs_op_dm_softmax_warp: compact-2 partials need a width that is a multiple of 4"); return -1; }
    return launch_dm_softmax_warp(part, bias, kp_d, kp_s, in_hwdc, out32, (half_t*)out16, deform, N, D, H, W, (hipStream_t)stream, shared_in != 0, shared_kps != 0);
}

extern "C" int cs_op_occ_finish(const float* part, int taps, float bias, float* occ, int N, int H, int W, void* stream)
{
    if (!part || !occ || N < 1 || H < 1 || W < 1) { cs_set_error("cs_op_occ_finish: bad arguments"); return -1; }
    if (taps == 49) return launch_occ_finish49(part, bias, occ, N, H, W, (hipStream_t)stream);
    if (taps == 7) return launch_occ_finish(part, bias, occ, N, H, W, (hipStream_t)stream);
    cs_set_error("cs_op_occ_finish: taps %d (7 or 49)", taps);
    return -1;
}

extern "C" int cs_op_dm_read(cs_engine* e, int which, int B, void* dst, void* stream)
{
    ENTER(e, B);
    if (!dst) { cs_set_error("cs_op_dm_read: null destination"); return -1; }
    const void* src; size_t bytes;
    if (which == CS_DM_COMP) { src = e->dm_comp; bytes = (size_t)B * DM_COMP_ELEMS * sizeof(half_t); }
    else if (which >= CS_DM_L0 && which <= CS_DM_L0 + 5) { src = e->dm_l[which - CS_DM_L0]; bytes = (size_t)B * dm_level_elems(which - CS_DM_L0) * sizeof(half_t); }
    else if (which == CS_DM_PRED) { src = e->dm_pred; bytes = (size_t)B * DM_PRED_ELEMS * sizeof(half_t); }
    else if (which == CS_DM_LOGITS) { src = e->dm_logits; bytes = (size_t)B * DM_LOGIT_FLOATS * sizeof(float); }
    else { cs_set_error("cs_op_dm_read: no buffer %d", which); return -1; }
    return copy_dd(dst, src, bytes, (hipStream_t)stream);
}

// ---- operator level: G's workspace as the last cs_spade_decode left it (cs_op_g_read), a sentinel over all of it (cs_op_g_fill) and a stop after
// the n-th launch of the next cs_spade_decode (cs_op_g_stop): the tests check every step of run_G on the engine's own input to it
extern "C" int cs_op_g_read(cs_engine* e, int which, int B, void* dst, void* stream)
{
    ENTER(e, B);
    if (!dst) { cs_set_error("cs_op_g_read: null destination"); return -1; }
    if (which == CS_G_STATS) {      // the slot stats_slot() handed out last
        const float* slot = e->stats_pool + ((e->stats_next + e->stats_slots - 1) % e->stats_slots) * e->stats_slot_floats;
        return copy_dd(dst, slot, (size_t)B * 512 * 2 * sizeof(float), (hipStream_t)stream);
    }
    const GBuf b = g_buf(e, which);
    if (!b.p) { cs_set_error("cs_op_g_read: no buffer %d", which); return -1; }
    return copy_dd(dst, *b.p, (size_t)B * b.elems * sizeof(half_t), (hipStream_t)stream);
}

extern "C" int cs_op_g_fill(cs_engine* e, int B, void* stream)
{
    ENTER(e, B);
    for (int which = CS_G_X0; which <= CS_G_O256; ++which) {
        const GBuf b = g_buf(e, which);
        CS_CHECK_HIP(hipMemsetD16Async((hipDeviceptr_t)*b.p, CS_G_SENTINEL, (size_t)B * b.elems, (hipStream_t)stream));
    }
    CS_CHECK_HIP(hipMemsetD16Async((hipDeviceptr_t)e->stats_pool, CS_G_SENTINEL, e->stats_slots * e->stats_slot_floats * 2, (hipStream_t)stream));
    return 0;
}

extern "C" int cs_op_g_stop(cs_engine* e, int n)
{
    if (!e || n < 0) { cs_set_error("cs_op_g_stop: bad arguments"); return -1; }
    e->g_stop = n;
    return 0;
}

// ---- operator level: the volume workspace of F and R as the last cs_extract_feature_3d / cs_refine left it (cs_op_v_read), a sentinel over all of
// it (cs_op_v_fill) and a stop after the n-th launch of the next of the two (cs_op_v_stop): the tests check every step of run_F and run_R on the
// engine's own input to it
extern "C" int cs_op_v_read(cs_engine* e, int which, int B, void* dst, void* stream)
{
    ENTER(e, B);
    if (!dst) { cs_set_error("cs_op_v_read: null destination"); return -1; }
    if (which == CS_V_STATS) {      // the slot stats_slot() handed out last
        const float* slot = e->stats_pool + ((e->stats_next + e->stats_slots - 1) % e->stats_slots) * e->stats_slot_floats;
        return copy_dd(dst, slot, (size_t)B * 512 * 2 * sizeof(float), (hipStream_t)stream);
    }
    const VBuf b = v_buf(e, which);
    if (!b.p) { cs_set_error("cs_op_v_read: no buffer %d", which); return -1; }
    return copy_dd(dst, b.p, (size_t)B * b.bytes, (hipStream_t)stream);
}

extern "C" int cs_op_v_fill(cs_engine* e, int B, void* stream)
{
    ENTER(e, B);
    for (int which = CS_V_T0; which <= CS_V_SP1; ++which) {
        const VBuf b = v_buf(e, which);
        CS_CHECK_HIP(hipMemsetD16Async((hipDeviceptr_t)b.p, CS_G_SENTINEL, (size_t)B * b.bytes / 2, (hipStream_t)stream));
    }
    CS_CHECK_HIP(hipMemsetD16Async((hipDeviceptr_t)e->stats_pool, CS_G_SENTINEL, e->stats_slots * e->stats_slot_floats * 2, (hipStream_t)stream));
    return 0;
}

extern "C" int cs_op_v_stop(cs_engine* e, int n)
{
    if (!e || n < 0) { cs_set_error("cs_op_v_stop: bad arguments"); return -1; }
    e->g_stop = n;
    return 0;
}

// ---- operator level: the three kernels of F and R that run outside the conv kernels (csrc/kernels.hip), without an engine
extern "C" int cs_op_conv_first(const float* img, const float* w, const float* b, void* out16, int N, int H, int W, void* stream)
{
    if (!img || !w || !b || !out16 || N < 1 || H < 1 || W < 1) { cs_set_error("cs_op_conv_first: bad arguments"); return -1; }
    return launch_conv_first(img, w, b, (half_t*)out16, N, H, W, (hipStream_t)stream);
}

extern "C" int cs_op_norm_act(const float* y, const float* stats, const float* gamma, const float* beta, const float* res, float slope, float* out32,
                              void* out16, const float* s2, const float* t2, int period2, int act2, float slope2, int N, long per_n, int split,
                              void* stream)
{
    if (!y || !stats || !gamma || !beta || (!out32 && !out16) || (!s2) != (!t2) || N < 1 || per_n < 1) { cs_set_error("cs_op_norm_act: bad arguments"); return -1; }
    return launch_norm_act(y, stats, gamma, beta, res, slope, out32, (half_t*)out16, s2, t2, period2, act2, slope2, N, per_n, (hipStream_t)stream, split);
}

extern "C" int cs_op_split16(const float* x, void* out16, long n, void* stream)
{
    if (!x || !out16 || n < 32 || n % 32) { cs_set_error("cs_op_split16: bad arguments (n: whole voxels of 32 channels)"); return -1; }
    return launch_split16(x, (half_t*)out16, n, (hipStream_t)stream);
}

// ---- operator level: the identity network's kernels (csrc/identity.hip) without an engine, and the activations the last cs_identity pass left
extern "C" int cs_op_id_conv(const void* in, int in_f32, int N, int IH, int IW, int Cin, int K, int stride, int pad, const void* w, const float* bias,
                             int Cout, const float* slope, void* out, int out_f32, void* stream)
{
    IdConvCall c{};
    c.in = in; c.in_f32 = in_f32; c.N = N; c.IH = IH; c.IW = IW; c.Cin = Cin; c.K = K; c.stride = stride; c.pad = pad;
    if (K < 1 || stride < 1 || IH + 2 * pad < K || IW + 2 * pad < K) { cs_set_error("cs_op_id_conv: bad arguments"); return -1; }
    c.OH = (IH + 2 * pad - K) / stride + 1; c.OW = (IW + 2 * pad - K) / stride + 1;
    c.w = (const half_t*)w; c.bias = bias; c.Cout = Cout; c.slope = slope; c.out = out; c.out_f32 = out_f32;
    return launch_id_conv(c, (hipStream_t)stream);
}

extern "C" int cs_op_id_maxpool(const float* in, const float* s, const float* t, float* x, void* a16, int B, int IH, int IW, int C, void* stream)
{
    return launch_id_maxpool(in, s, t, x, (half_t*)a16, B, IH, IW, C, (hipStream_t)stream);
}

extern "C" int cs_op_id_se_tail(const float* out, long sN, long sH, long sW, int B, int H, int W, int C, const float* w1, const float* b1,
                                const float* w2, const float* b2, const float* slopes, const float* res, const float* s, const float* t, float* se,
                                float* x, void* a16, void* stream)
{
    if (!slopes) { cs_set_error("cs_op_id_se_tail: NULL slopes"); return -1; }
    TRY(launch_id_se(out, sN, sH, sW, B, H, W, C, w1, b1, slopes + 1, w2, b2, se, (hipStream_t)stream));
    return launch_id_tail(out, sN, sH, sW, se, res, slopes, s, t, x, (half_t*)a16, B, H, W, C, (hipStream_t)stream);
}

extern "C" int cs_op_id_embed(const void* a16, const void* w, const float* bias, float* part, float* raw, float* idn, int B, void* stream)
{
    return launch_id_embed((const half_t*)a16, (const half_t*)w, bias, part, raw, idn, B, (hipStream_t)stream);
}

extern "C" int cs_op_identity_read(cs_engine* e, int which, int B, float* dst, void* stream)
{
    if (!e || !e->idn.present) { cs_set_error("cs_op_identity_read: no engine, or no identity network in it"); return -1; }
    const IdNet& A = e->idn;
    if (!dst) { cs_set_error("cs_op_identity_read: null destination"); return -1; }
    if (B < 1 || B > A.lastB) { cs_set_error("cs_op_identity_read: %d samples, the last pass held %d", B, A.lastB); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    if (which == CS_ID_STEM) return launch_id_to_nchw(A.stem_x, 0, dst, B, 64, 55 * 55, st);
    if (which >= CS_ID_LAYER1 && which < CS_ID_LAYER1 + 4) {
        const int l = which - CS_ID_LAYER1;
        return launch_id_to_nchw(A.layer_x[l], 0, dst, B, IDNET_C[l], IDNET_HW[l] * IDNET_HW[l], st);
    }
    if (which == CS_ID_PREFC) return launch_id_to_nchw(A.a16, 1, dst, B, 512, 49, st);
    cs_set_error("cs_op_identity_read: no activation %d", which);
    return -1;
}

// ---- operator level: the face parser's kernels (csrc/parser.hip) without an engine, and the activations the last cs_parser pass left
extern "C" int cs_op_parser_input(const float* pixel_values, void* out16, int B, int H, int W, void* stream)
{
    return launch_p_input(pixel_values, (half_t*)out16, B, H, W, (hipStream_t)stream);
}

extern "C" int cs_op_parser_gemm(const void* a16, const void* w16, const float* bias, int M, int K, int N, int mode, void* out, int P, int L, void* stream)
{
    PGemmCall g{(const half_t*)a16, (const half_t*)w16, bias, out, M, K, N, mode, P, L};
    return launch_p_gemm(g, (hipStream_t)stream);
}

extern "C" int cs_op_parser_layernorm(const float* in, const float* g, const float* b, float eps, long M, int C, float* out32, void* out16, void* stream)
{
    return launch_p_ln(in, g, b, eps, M, C, out32, (half_t*)out16, (hipStream_t)stream);
}

extern "C" int cs_op_parser_attention(const void* q16, const void* kv16, void* ctx16, int B, int Nq, int Nk, int heads, int d, void* stream)
{
    return launch_p_attn((const half_t*)q16, (const half_t*)kv16, (half_t*)ctx16, B, Nq, Nk, heads, d, (hipStream_t)stream);
}

extern "C" int cs_op_parser_dwgelu(const void* in16, const float* w, const float* bias, void* out16, int B, int H, int W, int C, void* stream)
{
    return launch_p_dwgelu((const half_t*)in16, w, bias, (half_t*)out16, B, H, W, C, (hipStream_t)stream);
}

extern "C" int cs_op_parser_upadd(const float* p0, const float* p1, const float* p2, const float* p3, void* out16, int B, int H, int W, int D, void* stream)
{
    return launch_p_upadd(p0, p1, p2, p3, (half_t*)out16, B, H, W, D, (hipStream_t)stream);
}

extern "C" int cs_op_parser_read(cs_engine* e, int which, int B, float* dst, void* stream)
{
    if (!e || !e->psr.present) { cs_set_error("cs_op_parser_read: no engine, or no face parser in it"); return -1; }
    const ParserNet& P = e->psr;
    if (!dst) { cs_set_error("cs_op_parser_read: null destination"); return -1; }
    if (B < 1 || B > P.lastB) { cs_set_error("cs_op_parser_read: %d samples, the last pass held %d", B, P.lastB); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    if (which >= CS_PARSER_STAGE0 && which < CS_PARSER_STAGE0 + 4) {
        const int s = which - CS_PARSER_STAGE0;
        return launch_p_to_nchw(P.st32[s], dst, B, P.st[s].C, (long)(P.lastH >> (s + 2)) * (P.lastW >> (s + 2)), st);
    }
    if (which == CS_PARSER_PRE) return launch_nhwc16_to_nchw(P.pre16, dst, B, P.D, (P.lastH / 4) * (P.lastW / 4), st);
    cs_set_error("cs_op_parser_read: no activation %d", which);
    return -1;
}
