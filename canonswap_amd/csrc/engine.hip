// Host side of the gfx950 CanonSwap engine: weight registry, workspace, per-stage kernel sequencing and
// the C ABI declared in include/canonswap_hip.h.  Stage order and argument wiring follow
// src/can_swap_pipeline_e2e.py:242-263 and src/can_swap_e2e.py:286-312 of the reference.
#include "engine.h"

#include <cstdarg>
#include <initializer_list>

static thread_local char g_err[1024] = "";
void cs_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* cs_last_error(void) { return g_err; }
// 4, unchanged: cs_resize_half_bilinear, cs_motion_keypoints_driven, cs_paste_back_shared (the v2i device-side frame) cs_crop_frames (the crop in front of both chains), cs_face_masks (the parser's logits -> 0/1 masks), cs_parser_input (crops -> the parser's pixel_values) and cs_concat_frames (the side-by-side video frame) were added; new entry points
// alone change no struct, no existing entry point's meaning and no blob format, which is what the header bumps the version for.
// 4, unchanged: cs_identity, cs_identity_u8 (getid on the engine), cs_op_identity_read and cs_op_id_conv / cs_op_id_maxpool / cs_op_id_se_tail /
// cs_op_id_embed (its kernels alone) were added; the optional "A.*" blobs are new names, no existing blob changed.
// 4, unchanged: cs_parser (the SegFormer face parser on the engine), cs_op_parser_read and cs_op_parser_input / cs_op_parser_gemm / cs_op_parser_layernorm /
// cs_op_parser_attention / cs_op_parser_dwgelu / cs_op_parser_upadd (its kernels alone) were added; the optional "P.*" blobs are new names; cs_op_id_conv takes K up to 8.
// 4, unchanged: cs_crop_faces and cs_paste_back_faces (several faces per frame: the crop and the ordered paste-back under a frame index) were added.
// 4, unchanged: cs_det_input and cs_det_decode (the face detector's letterbox + blob and its decode + NMS, around the caller's network) were added.
// 4 (round 6): cs_soft_erosion_frames, cs_paste_back_batch, cs_motion_keypoints.
// 3 (round 4): cs_conv_desc grew (hilo, stat_out, xf_*, ep_general), cs_op_conv takes conv_halo / vol32 / conv_wide configurations only, the
// packed weight blobs of F.down0 / down1 / second carry [W_hi | W_lo], W.occ49 exists; cs_conv_desc::pool_hw.  _lib.load() refuses any other value.
extern "C" int cs_abi_version(void) { return CS_ABI_VERSION; }

static int need(cs_engine* e, const std::string& n, size_t bytes, const void** out)
{
    const Blob* b = e->find(n);
    if (!b) { cs_set_error("weights: blob '%s' was not uploaded", n.c_str()); return -1; }
    if (bytes && b->bytes != bytes) { cs_set_error("weights: blob '%s' has %zu bytes, expected %zu", n.c_str(), b->bytes, bytes); return -1; }
    *out = b->p;
    return 0;
}

static int get_conv(cs_engine* e, const std::string& n, int Cin, int Cout_pad, int Cout, int KD, int KH, int KW, int bias_len,
             double macs, ConvL* L)
{
    const int nch = (Cin + 31) / 32;
    const void* p;
    TRY(need(e, n + ".w", (size_t)nch * KD * KH * KW * Cout_pad * 32 * sizeof(half_t), &p));
    L->w = (const half_t*)p;
    L->b = nullptr;
    if (bias_len > 0) { TRY(need(e, n + ".b", (size_t)bias_len * sizeof(float), &p)); L->b = (const float*)p; }
    L->Cin = Cin; L->Cout_pad = Cout_pad; L->Cout = Cout; L->KD = KD; L->KH = KH; L->KW = KW;
    L->macs_per_pos = macs; L->ragged = false;
    L->name = n;
    return 0;
}

static int get_affine(cs_engine* e, const std::string& n, int len, Affine* a)
{
    const void* p;
    TRY(need(e, n + ".s", (size_t)len * 4, &p)); a->s = (const float*)p;
    TRY(need(e, n + ".t", (size_t)len * 4, &p)); a->t = (const float*)p;
    return 0;
}

static int get_f32(cs_engine* e, const std::string& n, int len, const float** out)
{
    const void* p;
    TRY(need(e, n, (size_t)len * 4, &p));
    *out = (const float*)p;
    return 0;
}

ConvCall mk(const ConvL& L, const void* in, TDesc ind, int N, int D, int H, int W, int up_shift)
{
    ConvCall c;
    memset(&c.p, 0, sizeof(c.p));
    ConvParams& p = c.p;
    p.in = (const half_t*)in;
    p.zero = cs_zero_page();
    p.in_sN = ind.sN; p.in_sD = ind.sD; p.in_sH = ind.sH; p.in_sW = ind.sW;
    p.N = N; p.D = D; p.H = H; p.W = W; p.inD = D;
    p.Cin = L.Cin; p.nchunks = (L.Cin + 31) / 32; p.up_shift = up_shift;
    p.KD = L.KD; p.KH = L.KH; p.KW = L.KW; p.PD = L.KD / 2; p.PH = L.KH / 2; p.PW = L.KW / 2;
    p.wgt = L.w; p.Cout_pad = L.Cout_pad; p.Cout = L.Cout; p.ragged = L.ragged;
    p.bias = L.b;
    p.ps_stride = 1;
    c.macs_per_pos = L.macs_per_pos;
    c.name = L.name.c_str();
    return c;
}

// tile configuration of the 32->32 3x3x3 convs on the [H][W][D][C] volumes: 256 positions (4x4x16) x 32 channels; 128-position
// tiles measured slower (more halo re-reads than the extra occupancy returns)
static int cfg_v32() { return CFG_H_256x32; }

// debug knob CANONSWAP_AMAX=1 (profiled steps only): largest |value| of the fp16 tensors this conv stored
static int amax_after(cs_engine* e, const ConvCall& c, hipStream_t st)
{
    if (!e->knobs.amax || !e->prof || e->recs.empty()) return 0;
    if (!e->amax_dev) { if (e->alloc(&e->amax_dev, (size_t)4096)) return -1; }
    if (e->amax_n >= 4096) return 0;
    const ConvParams& p = c.p;
    const bool o0 = p.out0.p && !p.out0_f32 && c.mode != MODE_PIXSHUF, o1 = p.out1.p != nullptr;
    if (!o0 && !o1) return 0;
    const int slot = e->amax_n++;
    hipError_t r = hipMemsetAsync(e->amax_dev + slot, 0, sizeof(unsigned), st);
    if (r != hipSuccess) { cs_set_error("amax memset: %s", hipGetErrorString(r)); return -1; }
    if (o0) TRY(launch_absmax16((const half_t*)p.out0.p, p.out0, p.N, p.D, p.H, p.W, p.Cout, e->amax_dev + slot, st));
    if (o1) TRY(launch_absmax16((const half_t*)p.out1.p, p.out1, p.N, p.D, p.H, p.W, p.Cout, e->amax_dev + slot, st));
    for (auto it = e->recs.rbegin(); it != e->recs.rend(); ++it) if (it->fam == 0) { it->amax_slot = slot; break; }
    return 0;
}

constexpr int VOL32_MINB = 3;          // below three frames the plain volume convs stay on the halo kernel (see go())

// Launch one convolution on conv_halo (LDS-staged input patch, register-streamed weights).
int go(cs_engine* e, ConvCall& c, hipStream_t st, int prefW, int prefH)
{
    const int nph = c.p.nphase > 0 ? c.p.nphase : 1;      // grouped launch (ConvParams::nphase): macs_per_pos is one phase's
    const double fl = 2.0 * c.macs_per_pos * (double)c.p.N * c.p.D * c.p.H * c.p.W * nph;
    e->flops += fl;
    // MFMA work actually issued: packed (padded) channel counts and the taps this launch really runs
    {
        double ksteps = (double)c.p.nchunks * c.p.KD * c.p.KH * c.p.KW;      // 32-deep K-steps per output element
        if (c.p.ragged) {                                                    // paired taps in the last chunk
            const int NT = c.p.KD * c.p.KH * c.p.KW, PK = c.p.KW > 1 ? c.p.KW : c.p.KH;
            ksteps -= NT - (NT / PK) * (PK / 2 + PK % 2);
        }
        e->flops_exec += 2.0 * (double)c.p.N * c.p.D * c.p.H * c.p.W * c.p.Cout_pad * 32.0 * ksteps * nph;
    }
    // the 3x3x3 32 -> 32 convolutions of the feature volume run on their own kernel (vol32.hip; CANONSWAP_VOL32=0: A/B knob, conv_halo)
    // (below three frames the strips of a launch cover a quarter of the CUs or less: the plain convs - bit-identical on either kernel - stay
    // on the halo kernel there, one frame 6.75 -> 6.5 ms; the statistics / transform-staging convs of R always run vol32: their partial
    // statistics are laid out per kernel, and a frame's bits must not depend on the batch it is part of)
    if (e->knobs.vol32 && vol32_supported(c.p) && (c.p.N >= VOL32_MINB || c.p.stat_out || c.p.xf_kind)) {
        if (e->latency_mode && c.p.stat_out) c.p.v32_srows = 2;      // 2-row segments: 256 items on one frame's 64 x 64 volume (common.h)
        c.stat_nblk = vol32_stat_nblk(c.p);
        TRY(e->run(0, st, [&] { return launch_vol32(c.p, st); }, c.name, fl));
        return amax_after(e, c, st);
    }
    if (c.p.xf_kind) { cs_set_error("%s: transform staging needs the vol32 kernel", c.name); return -1; }
    // the wide 2-D 3x3 convs on the persistent kernel (conv_wide.hip: 256 x 256 workgroup tiles, 8 x 8 fragments per wave, one workgroup per
    // CU) once every workgroup of its grid gets two items or more; the same bits as conv_halo (CANONSWAP_WIDE=0: A/B knob).  The SPADE
    // gamma / beta convs stay on conv_halo's 128 x 256 tiles (CANONSWAP_WIDE=2 moves them too): their K is two chunks (Cin = 128), so a tile
    // is 40 % epilogue, which two resident workgroups overlap and one persistent workgroup per CU cannot: 1.01 - 1.04x the time
    // (profiles/r04_c_ab_wide.txt).
    const int wide_on = e->knobs.wide;
    if (wide_on && !e->latency_mode && c.hcfg < 0 && (c.mode != MODE_SPADE || wide_on >= 2)) {
        if (conv_wide_supported(c.p, c.mode) && (long)c.p.N * (c.p.H / 16) * (c.p.W / 16) * (c.p.Cout_pad / 256) >= 512) {
            c.stat_nblk = (c.p.W / 16) * (c.p.H / 8) * 2;      // partial-statistics blocks per sample: 64 positions each, in the 16 x 8 tiles' order
            TRY(e->run(0, st, [&] { return launch_conv_wide(c.p, c.mode, st); }, c.name, fl));
            return amax_after(e, c, st);
        }
    }
    // single-frame mode: the 512-channel 3x3 layers at 64 x 64 (T blend, G_middle / up_0, R's 2-D pair, W.third) on conv_lat.hip - the 16 x 8 tile
    // with its K loop split over the three kernel rows across 12 waves - while the launch is one workgroup per CU or less.  Another summation
    // order than the batched path: only behind cs_set_latency_mode (conv_halo's four-wave tiles: 4.55 against 4.29 ms per frame, profiles/r05_e_ab_lat_ring.txt)
    if (e->latency_mode && c.hcfg < 0 && conv_lat_supported(c.p, c.mode) &&
        (long)c.p.N * (c.p.H / 8) * (c.p.W / 16) * (c.p.Cout_pad / (c.mode == MODE_TBLEND ? 128 : 64)) <= 256) {
        c.stat_nblk = (c.p.W / 16) * (c.p.H / 8) * 2;      // partial-statistics blocks per sample: 64 positions each, in the 16 x 8 tiles' order
        TRY(e->run(0, st, [&] { return launch_conv_lat(c.p, c.mode, st); }, c.name, fl));
        return amax_after(e, c, st);
    }
    if (c.p.inD == c.p.D) {
        const HaloPlan plan = halo_plan(c.p, c.mode, c.hcfg, prefW, prefH, c.cg_ck64);      // (conv_plan.h: tile, chunk width, statistics blocks)
        const int hcfg = plan.hcfg, ck = plan.ck;
        c.stat_nblk = plan.stat_nblk;
        // cross-workgroup split-K when the launch cannot fill the chip (single-frame latency: the deep hourglass levels run 8-64
        // workgroups that each stream megabytes of weights): plain bias + activation + one output only
        // Split sums are added in another order than one workgroup's sequential accumulation, so results differ in the last
        // bits from the batched path: the engine only does this in latency mode (cs_set_latency_mode), never silently by batch size -
        // frames of a batch stay bit-identical to the same frames run alone.
        const long wgs = (long)c.p.nTW * c.p.nTH * c.p.nTD * c.p.nTN * (c.p.Cout_pad / halo_tile(hcfg).BN);
        const int nck = (c.p.Cin + ck - 1) / ck;
        const long mtot = (long)c.p.N * c.p.D * c.p.H * c.p.W;
        const bool plain = c.mode == MODE_STD && !c.p.res.p && !c.p.pixscale && !c.p.out1.p && !c.p.stat_out && !c.p.s2 &&
                           c.p.act0 <= ACT_SIGMOID && c.p.out0.p && hcfg != CFG_H_SK128x32 && c.p.Cout % 4 == 0 && !c.p.spmul && !c.p.nphase &&
                           (!c.p.pool_hw || (!c.p.out0_f32 && !(c.p.H & 1) && !(c.p.W & 1)));      // (pooled: the finishing launch averages)
        constexpr int sk_maxwg = 64, sk_fill = 512;      // r02 sweep
        if (e->latency_mode && plain && wgs <= sk_maxwg && nck >= 4 && e->sk_buf) {
            int splits = (int)(sk_fill / wgs);
            if (splits > nck) splits = nck;
            if (splits > 16) splits = 16;
            while (splits > 1 && (size_t)splits * mtot * c.p.Cout_pad > e->sk_cap) --splits;
            if (splits >= 2) {
                c.p.sk_out = e->sk_buf; c.p.sk_splits = splits; c.p.xcd_map = 0;
                TRY(e->run(0, st, [&] { return launch_conv_halo(c.p, hcfg, ck, c.mode, st); }, c.name, fl));
                return e->run(1, st, [&] { return launch_splitk_finish(c.p, st); }, "splitk_finish");
            }
        }
        TRY(e->run(0, st, [&] { return launch_conv_halo(c.p, hcfg, ck, c.mode, st); }, c.name, fl));
        return amax_after(e, c, st);
    }
    cs_set_error("%s: no conv_halo launch for this convolution (depth-collapsing convs are not supported)", c.name);
    return -1;
}

static float* stats_slot(cs_engine* e)
{
    float* p = e->stats_pool + (e->stats_next % e->stats_slots) * e->stats_slot_floats;
    e->stats_next++;
    return p;
}

// Convolution whose epilogue also emits the Instance/GroupNorm partial sums of its stored output; returns the finished
// (mean, rstd) slot. P = positions per sample.
static int go_stats(cs_engine* e, ConvCall& c, int C, long P, float** slot, hipStream_t st, int prefW = 0, int prefH = 0)
{
    c.p.stat_out = e->stats_part;
    TRY(go(e, c, st, prefW, prefH));
    float* s = stats_slot(e);
    *slot = s;
    const int nblk = c.stat_nblk, N = c.p.N;
    if ((long)nblk * C * 2 > 262144) { cs_set_error("%s: statistics partials do not fit (%d blocks x %d)", c.name, nblk, C); return -1; }
    return e->run(1, st, [&] { return launch_chan_stats_finish(e->stats_part, nblk, N, C, 1.0 / (double)P, 1e-5f, s, st); }, "chan_stats_finish");
}

// (mean, rstd) per (n, c) of a [N][P][C] tensor into a fresh slot of the stats pool
static int do_stats(cs_engine* e, const void* x, int is_f32, int B, long P, int C, float** out, hipStream_t st)
{
    float* slot = stats_slot(e);
    *out = slot;
    return e->run(1, st, [&] { return launch_chan_stats(x, is_f32, B, P, C, 1e-5f, e->stats_part, slot, st); }, "chan_stats");
}

// ------------------------------------------------------------------------------------------------ F
// AppearanceFeatureExtractor.forward (appearance_feature_extractor.py:38-48); result: fp32 HWDC in vs[*cur]
// whole ResBlock3d per launch (vol32_fused.hip; CANONSWAP_VOL32_FUSED=0: A/B knob, two vol32 / conv_halo launches per block)
static int run_resblocks3d(cs_engine* e, cs_engine::RB3* rb, int B, int* cur, hipStream_t st)
{
    // util.py:94-102; a = relu(bn1(x)) is already in va[0]; x (fp32 residual stream) in vs[*cur]
    if (e->knobs.vol32_fused) {     // at every batch size (one frame: 2-row segments, launch_vol32_fused); the same bits as the two-launch path below
        // block i reads a from va[i & 1] and leaves the next block's a in va[(i + 1) & 1] (a neighbouring workgroup still reads the halo
        // columns of the input while this one stores): six blocks end in va[0] again
        for (int i = 0; i < 6; ++i) {
            const int nxt = (*cur + 1) % 3;
            ResBlock3dCall c;
            c.a = e->va[i & 1]; c.x = e->vs[*cur]; c.out0 = e->vs[nxt]; c.out1 = e->va[(i + 1) & 1];
            c.sN = VOL; c.sH = (long)FW * FD * FC; c.sW = (long)FD * FC;
            c.w1 = rb[i].c1.w; c.w2 = rb[i].c2.w; c.b1 = rb[i].c1.b; c.b2 = rb[i].c2.b;
            c.s2 = nullptr; c.t2 = nullptr; c.act1 = ACT_NONE; c.slope1 = 0.f;
            if (i < 5) { c.s2 = rb[i].post.s; c.t2 = rb[i].post.t; c.act1 = ACT_RELU; }
            c.N = B; c.H = FH; c.W = FW;
            const double fl = 2.0 * (rb[i].c1.macs_per_pos + rb[i].c2.macs_per_pos) * (double)B * VOX;
            e->flops += fl;
            e->flops_exec += 2.0 * 2.0 * (double)B * VOX * 32 * 32.0 * 27;
            TRY(e->run(0, st, [&] { return launch_vol32_fused(c, st); }, (rb[i].c1.name + "+c2").c_str(), fl));
            *cur = nxt;
        }
        return 0;
    }
    for (int i = 0; i < 6; ++i) {
        ConvCall c1 = mk(rb[i].c1, e->va[0], hwdc3(nullptr), B, FD, FH, FW);   // conv1 with norm2 folded, ReLU
        c1.p.act0 = ACT_RELU;
        c1.p.out0 = hwdc3(e->va[1]);
        c1.hcfg = cfg_v32();
        TRY(go(e, c1, st, 4, 4));
        const int nxt = (*cur + 1) % 3;
        ConvCall c2 = mk(rb[i].c2, e->va[1], hwdc3(nullptr), B, FD, FH, FW);   // conv2 + x
        c2.p.res = hwdc3(e->vs[*cur]); c2.p.res_f32 = 1;
        c2.p.out0 = hwdc3(e->vs[nxt]); c2.p.out0_f32 = 1;
        c2.p.out1 = hwdc3(e->va[0]);
        if (i < 5) { c2.p.s2 = rb[i].post.s; c2.p.t2 = rb[i].post.t; c2.p.act1 = ACT_RELU; }
        c2.hcfg = cfg_v32();
        TRY(go(e, c2, st, 4, 4));
        *cur = nxt;
    }
    return 0;
}

// F's three 2-D convs (down_blocks.0 / .1, second: appearance_feature_extractor.py:41-44) with split-precision WEIGHTS: the packed weight holds
// [W_hi | W_lo] along the input channels (pack._pack_F) and the launch reads the same activations for both halves (grouped chunks at group
// stride 0), so out = W_hi x + W_lo x in one fp16 MFMA conv of twice the K.  The fp16 rounding of these three weight tensors alone cost the
// frame more than any other stage's arithmetic except T's (tests/psnr_attrib.py and the CPU emulation in DESIGN section 3: 57.5 dB with only
// these weights rounded, everything else exact); the three launches are 0.7 ms of a 125 ms step.
static void wsplit_in(ConvCall& c, int cin_real)
{
    c.p.cg = cin_real / 32; c.p.cg_cin = cin_real; c.p.in_sG = 0;       // chunk j -> channels (j % cg) * 32 of the one input tensor
}

static int run_F(cs_engine* e, int B, const float* img, int* cur, hipStream_t st)
{
    TRY(e->run(1, st, [&] { return launch_conv_first(img, e->first_w, e->first_b, e->f_t0, B, IMG, IMG, st); }, "conv_first"));
    e->flops += 2.0 * 3 * 64 * 9 * (double)B * IMG * IMG;
    // DownBlock2d (util.py:150-165): conv3x3 + folded BN + ReLU + AvgPool2d(2); the pool runs inside the conv's epilogue (ConvParams::pool_hw:
    // the average of the four fp32 values, one rounding, no full-resolution tensor) where the kernel carries it: the 32-channel-chunk
    // 16 x 8 tiles the [W_hi | W_lo] weights run on (also in latency mode: these launches are 512 / 256 workgroups, never split-K)
    ConvCall d0 = mk(e->f_down0, e->f_t0, nhwc(nullptr, 256, 256, 64), B, 1, 256, 256);
    d0.p.act0 = ACT_RELU; wsplit_in(d0, 64);
    d0.p.pool_hw = 1; d0.p.out0 = nhwc(e->f_p0, 128, 128, 128);
    TRY(go(e, d0, st));
    ConvCall d1 = mk(e->f_down1, e->f_p0, nhwc(nullptr, 128, 128, 128), B, 1, 128, 128);
    d1.p.act0 = ACT_RELU; wsplit_in(d1, 128);
    d1.p.pool_hw = 1; d1.p.out0 = nhwc(e->f_p1, 64, 64, 256);
    TRY(go(e, d1, st));
    *cur = 0;
    ConvCall s = mk(e->f_second, e->f_p1, nhwc(nullptr, 64, 64, 256), B, 1, 64, 64);   // 1x1 -> the 32x16 volume
    s.p.out0 = hwdc2(e->vs[0]); s.p.out0_f32 = 1;
    s.p.out1 = hwdc2(e->va[0]); s.p.s2 = e->f_pre0.s; s.p.t2 = e->f_pre0.t; s.p.act1 = ACT_RELU; wsplit_in(s, 256);
    TRY(go(e, s, st));
    return run_resblocks3d(e, e->f_rb, B, cur, st);
}

// ------------------------------------------------------------------------------------------------ W
// DenseMotionNetwork.forward (dense_motion.py:67-104). feat: fp32 HWDC. Leaves deformation / occlusion in
// e->dm_deform / e->dm_occ (the deformation only when the fused kernel is not used or the caller wants it: in the fused kernel it lives in LDS
// and going through HBM as well would be 0.79 MB per frame and call for nothing - ADVICE r3).
// warp_in / warp_o32 / warp_o16: when given, the feature warp that consumes the deformation (warping_network.py:46-62) is part of the softmax
// kernel (dm_softmax_warp_kernel): the caller launches no grid_sample (CANONSWAP_WARP_FUSED=0: A/B knob, dm_softmax + grid_sample).
// CANONSWAP_DEC_PHASES_DEEP=0: A/B knob (up-blocks 0 - 2 of the hourglass as 27-tap convs on the up-sampled grid, the form of rounds 1-5)
static int run_dense_motion(cs_engine* e, int B, const float* feat, const float* kp_d, const float* kp_s, hipStream_t st,
                     const float* warp_in = nullptr, float* warp_o32 = nullptr, half_t* warp_o16 = nullptr, bool want_deform = false,
                     bool shared_feat = false, bool shared_kps = false)
{
    // shared_feat / shared_kps: `feat` (and warp_in) is ONE volume, kp_s ONE key-point set, used by all B samples (sample stride 0 in the kernels
    // that read them; the compressed volume is computed once) - the v2i body (can_swap_pipeline_v2i.py:311-312)
    TRY(e->run(1, st, [&] { return launch_dm_compress(feat, e->cmp_w, e->cmp_b, e->dm_comp, shared_feat ? 1 : B, FD, FH, FW, st); }, "dm_compress"));
    e->flops += 2.0 * 32 * 4 * VOX * B;
    // hourglass input lands in channels [32,144) of the level-0 concat buffer (util.py:255-264 cat order)
    TRY(e->run(1, st, [&] { return launch_dm_sparse(e->dm_comp, kp_d, kp_s, e->dm_l[0] + 32, 144, B, FD, FH, FW, st, shared_feat, shared_kps); }, "dm_sparse"));
    static const int cout[5] = {64, 128, 256, 512, 1024};
    static const int skip_off[6] = {32, 64, 128, 256, 512, 0};   // channel offset of the skip part
    for (int i = 0; i < 5; ++i) {       // Encoder: DownBlock3d (util.py:185-190)
        const int S = 64 >> i;
        ConvCall c = mk(e->w_enc[i], e->dm_l[i] + skip_off[i], dhwc(nullptr, FD, S, S, DM_LW[i]), B, FD, S, S);
        c.p.act0 = ACT_RELU;
        c.p.out0 = dhwc(e->dm_pre, FD, S, S, cout[i]);
        if (i == 0) c.hcfg = CFG_H_256x64;      // 64 channels at 64x64: 256-position tiles (0.65 -> 0.47 ms per 16 frames)
        TDesc o = dhwc(e->dm_l[i + 1] + skip_off[i + 1], FD, S / 2, S / 2, DM_LW[i + 1]);
        // AvgPool3d((1,2,2)) of the block (util.py:189) inside the conv's epilogue: the average of the four fp32 values, rounded once, goes
        // straight into the next level's concat buffer - no full-resolution tensor, no pooling launch.  In latency mode
        // too: the finishing launch of a split-K conv averages the same way (splitk_finish_pool_kernel).
        c.p.pool_hw = 1; c.p.out0 = o;
        TRY(go(e, c, st));
    }
    for (int i = 0; i < 5; ++i) {       // Decoder: UpBlock3d (util.py:142-147), nearest x(1,2,2) folded into addressing
        const int lv = 5 - i, S = 64 >> (lv - 1), Si = S / 2;
        ConvCall c = mk(e->w_dec[i], e->dm_l[lv], dhwc(nullptr, FD, Si, Si, DM_LW[lv]), B, FD, S, S, 1);
        c.p.act0 = ACT_RELU;
        c.p.out0 = dhwc(e->dm_l[lv - 1], FD, S, S, DM_LW[lv - 1]);
        // Round 6: also up-blocks 0, 1 and 2 (1024 -> 512 from the 4 x 4 grid, 1024 -> 256 from the 8 x 8 one, 512 -> 128 from the 16 x 16 one) in
        // the batched mode - on 128x128 tiles (4x4x8 / 8x8x2 positions, static shapes 17 / 13): 12 of 27 taps, 0.66 -> 0.32 ms per 64-frame launch
        // for up-block 2.  In latency mode these three keep the 27-tap form: their launches are 8 - 64 workgroups there and run split-K, which a
        // grouped launch does not.
        if (i >= 3 || (!e->latency_mode && e->knobs.dec_phases_deep)) {
            // the nearest (1,2,2) up-sampling makes the three row / column taps read two source rows / columns: one 3x2x2 conv per
            // output phase (y, x) = (2i + a, 2j + b) on the source grid, 12 of 27 taps (pack.upsampled_conv3d_phases)
            // The four phases differ in their weights, their leading padding and their offset into the output only: ONE launch, blockIdx.z =
            // phase (ConvParams::nphase).  One frame: 128 / 256 workgroups that run their whole K loop instead of four split-K launches of
            // 32 / 64 tiles each with a finishing launch behind it (8 launches of 14 + 7 us per level: profiles/r05_l_phase_group.txt); the
            // same bits as four launches at every batch size (tests/test_gpu_ops.py).
            const int lwo = DM_LW[lv - 1];
            if (!e->knobs.phase_group) {      // CANONSWAP_PHASE_GROUP=0: four launches (tests: same bits)
                for (int ab = 0; ab < 4; ++ab) {
                    const int a = ab >> 1, b = ab & 1;
                    ConvCall q1 = mk(e->w_dec_p[i][ab], e->dm_l[lv], dhwc(nullptr, FD, Si, Si, DM_LW[lv]), B, FD, Si, Si);
                    q1.p.PH = a == 0; q1.p.PW = b == 0;
                    q1.p.act0 = ACT_RELU;
                    q1.p.out0 = td(e->dm_l[lv - 1] + ((long)a * S + b) * lwo, (long)FD * S * S * lwo, (long)S * S * lwo, 2L * S * lwo, 2L * lwo);
                    if (i == 4) { q1.hcfg = CFG_H_256x32; TRY(go(e, q1, st, 4, 4)); }
                    else TRY(go(e, q1, st));
                }
                continue;
            }
            ConvCall q = mk(e->w_dec_p[i][0], e->dm_l[lv], dhwc(nullptr, FD, Si, Si, DM_LW[lv]), B, FD, Si, Si);
            q.p.act0 = ACT_RELU;
            q.p.out0 = td(e->dm_l[lv - 1], (long)FD * S * S * lwo, (long)S * S * lwo, 2L * S * lwo, 2L * lwo);
            q.p.nphase = 4;
            for (int ab = 0; ab < 4; ++ab) {
                const int a = ab >> 1, b = ab & 1;
                q.p.ph_wofs[ab] = (long)(((intptr_t)e->w_dec_p[i][ab].w - (intptr_t)e->w_dec_p[i][0].w) / (intptr_t)sizeof(half_t));
                q.p.ph_ooff[ab] = (unsigned)(((long)a * S + b) * lwo);
                q.p.ph_PH[ab] = a == 0; q.p.ph_PW[ab] = b == 0;
            }
            q.p.PH = 1; q.p.PW = 1;
            static const char* const pn[5] = {"W.dec0.p", "W.dec1.p", "W.dec2.p", "W.dec3.p", "W.dec4.p"};
            q.name = pn[i];
            if (i == 4) { q.hcfg = CFG_H_256x32; TRY(go(e, q, st, 4, 4)); }     // 32 output channels: 256-position tile
            else TRY(go(e, q, st));
            continue;
        }
        if (i == 4) { c.hcfg = CFG_H_256x32; TRY(go(e, c, st, 4, 4)); continue; }
        TRY(go(e, c, st));
    }
    ConvCall t = mk(e->w_tail, e->dm_l[0], dhwc(nullptr, FD, 64, 64, 144), B, FD, 64, 64);   // util.py:261-263
    t.p.act0 = ACT_RELU; t.p.out0 = dhwc(e->dm_pred, FD, 64, 64, 144);
    // 160-wide tiles: 128 positions (two workgroups per CU) or 256 positions (one per CU, half the weight bytes per MFMA)
    // (tail 1.78 -> 1.29 ms, mask 2.63 -> 2.01 ms per 16 frames, profiles/r02_timeline_*.txt)
    t.hcfg = CFG_H_256x160;
    TRY(go(e, t, st));
    ConvCall m = mk(e->w_mask, e->dm_pred, dhwc(nullptr, FD, 64, 64, 144), B, FD, 64, 64);   // dense_motion.py:88
    // The (kw, c) partials never leave the conv: on its 256-position tiles (4 x 8 x 8) they are summed over kw inside the tile as far as the
    // tile reaches - 10 logit vectors per 4 columns instead of 28 (ConvParams::kw_out): a fixed summation order of the 7 partials of a logit,
    // finished by dm_logits().  Against 2-column tiles (8 vectors per 2 columns) the hand-over to the softmax is 0.92 GB per 64-frame call
    // instead of 1.48 GB, for 27 % more halo (784 voxels per 256 positions instead of 616).
    m.p.kw_out = e->dm_logits;
    m.hcfg = CFG_H_256x160;
    TRY(go(e, m, st, 4, 8));     // no halo along W (KW = 1)
    if (warp_in && e->knobs.warp_fused) {
        TRY(e->run(2, st, [&] { return launch_dm_softmax_warp(e->dm_logits, e->mask_b, kp_d, kp_s, warp_in, warp_o32, warp_o16, want_deform ? e->dm_deform : nullptr, B, FD, FH, FW, st, shared_feat, shared_kps); },
                   "dm_softmax_warp"));
    } else {
        TRY(e->run(1, st, [&] { return launch_dm_softmax(e->dm_logits, e->mask_b, kp_d, kp_s, e->dm_deform, B, FD, FH, FW, st, shared_kps); }, "dm_softmax"));
        if (warp_in) TRY(e->run(2, st, [&] { return launch_grid_sample(warp_in, e->dm_deform, warp_o32, warp_o16, B, FD, FH, FW, st, shared_feat); }, "grid_sample"));
    }
    // occlusion (dense_motion.py:98-102): the (c,d)-flattened 2272-channel 7x7 conv runs as a 2-D (7,1)-tap conv whose
    // input channels are grouped by depth slice (16 groups of 144 channels at stride sD) and whose 7 output channels are the
    // 7 horizontal taps (summed by occ_finish_kernel).
    // Batched path: the taps move into the output channels altogether - a 1x1 conv over the same grouped
    // channels with 49 (ky, kx) output channels (64 packed), finished by occ_finish49_kernel.  The (7,1)-tap form reads every activation
    // from LDS seven times for 7 useful output rows of 32 and was bound by exactly that (0.37 ms per call at 32 frames for 604 MB).
    if (!e->latency_mode) {
        ConvCall oc = mk(e->w_occ49, e->dm_pred, td(nullptr, (long)FD * 4096 * 144, 0, 64L * 144, 144), B, 1, 64, 64);
        oc.p.cg = 5; oc.p.cg_cin = 144; oc.p.in_sG = 4096L * 144;
        oc.p.out0 = nhwc(e->dm_occpart, 64, 64, 64); oc.p.out0_f32 = 1;
        oc.hcfg = CFG_H_128x64;
        TRY(go(e, oc, st));
        TRY(e->run(1, st, [&] { return launch_occ_finish49(e->dm_occpart, e->occ_b, e->dm_occ, B, 64, 64, st); }, "occ_finish"));
        return 0;
    }
    ConvCall oc = mk(e->w_occ, e->dm_pred, td(nullptr, (long)FD * 4096 * 144, 0, 64L * 144, 144), B, 1, 64, 64);
    oc.p.cg = 5; oc.p.cg_cin = 144; oc.p.in_sG = 4096L * 144;
    oc.p.out0 = nhwc(e->dm_occpart, 64, 64, 16); oc.p.out0_f32 = 1;
    // 7 real output channels, 560 K-steps: the four waves split the K-steps (0.27 -> 0.20 ms at B = 16); in latency mode the
    // K-steps are split over workgroups instead (32 tiles cannot fill the chip)
    oc.hcfg = e->latency_mode ? CFG_H_128x32 : CFG_H_SK128x32;
    TRY(go(e, oc, st));
    TRY(e->run(1, st, [&] { return launch_occ_finish(e->dm_occpart, e->occ_b, e->dm_occ, B, 64, 64, st); }, "occ_finish"));
    return 0;
}

// warp_out (warping_network.py:64-71): vol16 = fp16 HWDC volume -> seg16 [B][64][64][256]
static int run_warp_out(cs_engine* e, int B, const half_t* vol16, const float* occ, hipStream_t st)
{
    ConvCall t3 = mk(e->w_third, vol16, hwdc2(nullptr), B, 1, 64, 64);
    t3.p.act0 = ACT_LRELU; t3.p.slope0 = 0.01f;
    t3.p.out0 = nhwc(e->w_t3, 64, 64, 256);
    TRY(go(e, t3, st));
    ConvCall f4 = mk(e->w_fourth, e->w_t3, nhwc(nullptr, 64, 64, 256), B, 1, 64, 64);
    f4.p.pixscale = occ;
    f4.p.out0 = nhwc(e->seg16, 64, 64, 256);
    return go(e, f4, st);
}

// ------------------------------------------------------------------------------------------------ T
// Checks the slots of a batch (B host ints, the identity slot per sample) and, when they differ, uploads the per-sample slot vector; *mixed: the launches read e->slot_dev
int t_slots(cs_engine* e, int B, const int* slots, bool* mixed, hipStream_t st)
{
    *mixed = false;
    for (int b = 0; b < B; ++b) {
        if (slots[b] < 0 || slots[b] >= MAX_SLOTS) { cs_set_error("cs_swap: identity slot %d outside [0, %d)", slots[b], MAX_SLOTS); return -1; }
        if (!e->slot_set[slots[b]]) { cs_set_error("cs_swap: cs_set_identity has not been called for slot %d", slots[b]); return -1; }
        *mixed |= slots[b] != slots[0];
    }
    if (*mixed) {    // upload the per-sample slot vector when it changed (pinned ring: earlier async copies may still be pending)
        if (e->slot_cur.size() != (size_t)B || memcmp(e->slot_cur.data(), slots, sizeof(int) * B) != 0) {
            int* stage = e->slot_pin + (size_t)(e->slot_ring++ % 16) * e->maxB;
            memcpy(stage, slots, sizeof(int) * B);
            hipError_t r = hipMemcpyAsync(e->slot_dev, stage, sizeof(int) * B, hipMemcpyHostToDevice, st);
            if (r != hipSuccess) { cs_set_error("slot upload: %s", hipGetErrorString(r)); return -1; }
            e->slot_cur.assign(slots, slots + B);
        }
    }
    return 0;
}

// One AdaptiveSharedWeightConv2d layer of T (layer = 2 * block + (conv2 ? 1 : 0)) on [B][64][64][512] tensors: the mask conv into tmask, then
// the fused [W ; w_mod] conv with the blend epilogue.  conv1: out16 = relu(blend); conv2: out32 = res32 + blend and out16 its fp16 copy, on the
// last block through resblocks_3d.3dr0's norm1 + ReLU.  run_T and cs_op_t_layer both launch a layer here, so the operator test runs the
// engine's routing.
int t_layer(cs_engine* e, int layer, int B, const int* slots, bool mixed, const half_t* in, const float* res32, float* tmask, half_t* out16,
            float* out32, hipStream_t st)
{
    TLayer& L = e->t_l[layer];
    // mask_conv + sigmoid (:118-121,176): 512 -> 1 channel, a memory-bound dot product - its own VALU kernel (t_mask_kernel: 65 -> 4x us
    // per launch against one row of sixteen on the MFMA kernel)
    {
        const double mfl = 2.0 * L.mask.macs_per_pos * (double)B * 4096;
        e->flops += mfl; e->flops_exec += mfl;
        TRY(e->run(0, st, [&] { return launch_t_mask(in, L.mask.w, L.mask.b, tmask, B, 64, 64, st); }, L.mask.name.c_str(), mfl));
    }
    ConvCall fc = mk(L.fused, in, hwdc2(nullptr), B, 1, 64, 64);      // [W ; w_mod] fused, blend epilogue
    fc.mode = MODE_TBLEND;
    if (mixed) { fc.p.wgt = L.wset[0]; fc.p.wofs = L.wofs; fc.p.wslot = e->slot_dev; }   // per-sample w_mod (groups=N, :157-167)
    else fc.p.wgt = L.wset[slots[0]];
    fc.p.Cout = 512;
    fc.p.bias = L.bias;
    fc.p.pixscale = tmask; fc.p.ps_stride = 4;
    if (layer % 2 == 0) {
        fc.p.act0 = ACT_RELU;
        fc.p.out0 = hwdc2(out16);
    } else {
        fc.p.res = hwdc2((void*)res32); fc.p.res_f32 = 1;
        fc.p.out0 = hwdc2(out32); fc.p.out0_f32 = 1;
        fc.p.out1 = hwdc2(out16);
        if (layer == 13) { fc.p.s2 = e->t_pre0.s; fc.p.t2 = e->t_pre0.t; fc.p.act1 = ACT_RELU; }
    }
    return go(e, fc, st);
}

// transfer_model2.forward (adaptive_modulate.py:522-554). x: fp32 vs[*cur] + fp16 copy va[0].
// On exit: fp32 result in vs[*cur], fp16 copy in va[0].
// slots: B host ints (identity slot per sample)
static int run_T(cs_engine* e, int B, const int* slots, int* cur, hipStream_t st)
{
    bool mixed = false;
    TRY(t_slots(e, B, slots, &mixed, st));
    for (int i = 0; i < 7; ++i) {
        // ResnetBlock_Adaptive2D: conv1 -> ReLU -> conv2, + x (:337-349)
        TRY(t_layer(e, 2 * i, B, slots, mixed, e->va[0], nullptr, e->tmask, e->va[1], nullptr, st));
        const int nxt = (*cur + 1) % 3;
        TRY(t_layer(e, 2 * i + 1, B, slots, mixed, e->va[1], e->vs[*cur], e->tmask, e->va[0], e->vs[nxt], st));
        *cur = nxt;
    }
    return run_resblocks3d(e, e->t_rb, B, cur, st);   // last block leaves the raw fp16 copy in va[0]
}

// ------------------------------------------------------------------------------------------------ R
// G3d.forward (adaptive_modulate.py:721-733). x: fp32 vs[*cur] + fp16 va[0]; result fp32 in vs[*cur].
// Split precision: the two convs of a stage-3 block feed GroupNorms, which divide
// by the std of the conv output - the fp16 rounding of operands there costs 1.5e-3 relative error on the refined volume (every
// other stage: 1-4e-4) and sets the PSNR of the whole frame (50-57 dB depending on the frame).  With activations [hi | lo] and
// weights [W_hi | W_lo | W_hi] (three 32-channel weight chunks, the hi halo staged once: ConvParams::hilo) the same fp16 MFMA kernel
// computes W_hi x_hi + W_lo x_hi + W_hi x_lo, good to about 2^-21.  There is no switch: the plain fp16 form measured 49.5 dB on the worst
// pool frame, below the 50 dB gate (round 6: the CANONSWAP_R_SPLIT knob is gone).
static TDesc hwdc3_split(void* p) { return td(p, VOL * 2, 64, (long)FW * FD * 64, (long)FD * 64); }

// Stage-3 blocks with the GroupNorm apply fused into the consumer convolution (vol32 transform staging, ConvParams::xf_*): per block
//   conv1 reads  a0 = [block 0: x;  later: lrelu(gn2(y2') + x') of the previous block, written back as the new residual stream x]
//   conv2 reads  a1 = lrelu(gn1(y1))
// and one stand-alone norm_act closes the stage.  Five fp32-volume buffers rotate (vs[0..2] and the two split-precision buffers, which
// this path does not use otherwise): a conv never writes a volume that it, or a neighbouring workgroup of the same launch, still reads.
static int run_stage3_xf(cs_engine* e, cs_engine::S3* blk, int B, int* cur, const Affine* last_pre, hipStream_t st)
{
    float* pool[5] = {e->vs[0], e->vs[1], e->vs[2], (float*)e->vsp[0], (float*)e->vsp[1]};
    auto pick = [&](std::initializer_list<const float*> busy) -> float* {
        for (float* b : pool) { bool used = false; for (const float* u : busy) used |= (u == b); if (!used) return b; }
        return nullptr;
    };
    float* X = e->vs[*cur];                 // residual stream
    const float* pend_y = X; const float* pend_stats = nullptr; const float* pend_g = nullptr; const float* pend_b = nullptr;      // conv1's input
    for (int i = 0; i < 3; ++i) {           // ResBlock3D_stage3_leak (util.py:528-544)
        float* Xn = i ? pick({X, pend_y}) : X;                          // where the transformed input of conv1 goes (the new residual stream)
        float* Y1 = pick({X, pend_y, Xn});
        ConvCall c1 = mk(blk[i].c1sp, e->vsp[0], hwdc3_split(nullptr), B, FD, FH, FW);
        c1.p.hilo = 1;
        c1.p.xf_kind = i ? 2 : 1; c1.p.xf_y = hwdc3((void*)pend_y);
        if (i) {
            c1.p.xf_stats = pend_stats; c1.p.xf_gamma = pend_g; c1.p.xf_beta = pend_b; c1.p.xf_slope = 0.01f;
            c1.p.xf_res = hwdc3(X); c1.p.xf_out = hwdc3(Xn);
        }
        c1.p.out0 = hwdc3(Y1); c1.p.out0_f32 = 1;
        float* s1;
        TRY(go_stats(e, c1, 32, VOX, &s1, st, 4, 4));
        X = Xn;
        float* Y2 = pick({X, Y1});
        ConvCall c2 = mk(blk[i].c2sp, e->vsp[0], hwdc3_split(nullptr), B, FD, FH, FW);
        c2.p.hilo = 1;
        c2.p.xf_kind = 2; c2.p.xf_y = hwdc3(Y1); c2.p.xf_stats = s1; c2.p.xf_gamma = blk[i].g1; c2.p.xf_beta = blk[i].b1; c2.p.xf_slope = 0.01f;
        c2.p.out0 = hwdc3(Y2); c2.p.out0_f32 = 1;
        float* s2;
        TRY(go_stats(e, c2, 32, VOX, &s2, st, 4, 4));
        pend_y = Y2; pend_stats = s2; pend_g = blk[i].g2; pend_b = blk[i].b2;
    }
    // out = lrelu(gn2(y2) + x): the stage's result (fp32 stream + fp16 copy for what follows)
    int nxt = 0;
    while (e->vs[nxt] == X || e->vs[nxt] == pend_y) ++nxt;
    TRY(e->run(1, st, [&] { return launch_norm_act(pend_y, pend_stats, pend_g, pend_b, X, 0.01f, e->vs[nxt], e->va[0], last_pre ? last_pre->s : nullptr,
                                                   last_pre ? last_pre->t : nullptr, 512, last_pre ? ACT_LRELU : ACT_NONE, 0.01f, B, VOL, st, 0); },
                "norm_act"));
    *cur = nxt;
    return 0;
}

static int run_stage3(cs_engine* e, cs_engine::S3* blk, int B, int* cur, const Affine* last_pre, hipStream_t st)
{
    // GroupNorm apply / hi-lo split of R's stage-3 blocks inside the consumer conv's staging (vol32 transform staging) instead of stand-alone
    // norm_act / split16 passes (CANONSWAP_VOL32_XF=0: A/B knob)
    if (e->knobs.vol32_xf) return run_stage3_xf(e, blk, B, cur, last_pre, st);
    TRY(e->run(1, st, [&] { return launch_split16(e->vs[*cur], e->vsp[0], (long)B * VOL, st); }, "split16"));
    for (int i = 0; i < 3; ++i) {   // ResBlock3D_stage3_leak (util.py:528-544)
        const int y = (*cur + 1) % 3, nxt = (*cur + 2) % 3;
        ConvCall c1 = mk(blk[i].c1sp, e->vsp[0], hwdc3_split(nullptr), B, FD, FH, FW);
        c1.p.hilo = 1;
        c1.p.out0 = hwdc3(e->vs[y]); c1.p.out0_f32 = 1;
        c1.hcfg = cfg_v32();
        float* s1;
        TRY(go_stats(e, c1, 32, VOX, &s1, st, 4, 4));
        TRY(e->run(1, st, [&] { return launch_norm_act(e->vs[y], s1, blk[i].g1, blk[i].b1, nullptr, 0.01f, nullptr,
                                                       e->vsp[1], nullptr, nullptr, 32, ACT_NONE, 0.f, B, VOL, st, 1); }, "norm_act"));
        ConvCall c2 = mk(blk[i].c2sp, e->vsp[1], hwdc3_split(nullptr), B, FD, FH, FW);
        c2.p.hilo = 1;
        c2.p.out0 = hwdc3(e->vs[y]); c2.p.out0_f32 = 1;
        c2.hcfg = cfg_v32();
        float* s2;
        TRY(go_stats(e, c2, 32, VOX, &s2, st, 4, 4));
        const bool pre = (i == 2 && last_pre);
        const bool sp_out = i < 2;                  // the next stage-3 block reads split precision; everything else plain fp16
        TRY(e->run(1, st, [&] { return launch_norm_act(e->vs[y], s2, blk[i].g2, blk[i].b2, e->vs[*cur], 0.01f,
                                                       e->vs[nxt], sp_out ? e->vsp[0] : e->va[0], pre ? last_pre->s : nullptr,
                                                       pre ? last_pre->t : nullptr, 512, pre ? ACT_LRELU : ACT_NONE, 0.01f, B, VOL, st, sp_out); },
                    "norm_act"));
        *cur = nxt;
    }
    return 0;
}

static int run_R(cs_engine* e, int B, int* cur, hipStream_t st)
{
    TRY(run_stage3(e, e->r_s1, B, cur, &e->r_rb2[0].pre, st));
    for (int i = 0; i < 3; ++i) {   // ResBlock2d on the 512-channel view (util.py:120-128), LeakyReLU(0.01)
        ConvCall c1 = mk(e->r_rb2[i].c1, e->va[0], hwdc2(nullptr), B, 1, 64, 64);
        c1.p.act0 = ACT_LRELU; c1.p.slope0 = 0.01f;
        c1.p.out0 = hwdc2(e->va[1]);
        TRY(go(e, c1, st));
        const int nxt = (*cur + 1) % 3;
        ConvCall c2 = mk(e->r_rb2[i].c2, e->va[1], hwdc2(nullptr), B, 1, 64, 64);
        c2.p.res = hwdc2(e->vs[*cur]); c2.p.res_f32 = 1;
        c2.p.out0 = hwdc2(e->vs[nxt]); c2.p.out0_f32 = 1;
        c2.p.out1 = hwdc2(e->va[0]);
        if (i < 2) { c2.p.s2 = e->r_rb2[i + 1].pre.s; c2.p.t2 = e->r_rb2[i + 1].pre.t; c2.p.act1 = ACT_LRELU; c2.p.slope1 = 0.01f; }
        TRY(go(e, c2, st));
        *cur = nxt;
    }
    return run_stage3(e, e->r_s3, B, cur, nullptr, st);
}

// ------------------------------------------------------------------------------------------------ G
// SPADEDecoder.forward (spade_generator.py:41-59). seg16: [B][64][64][256] fp16 -> img fp32 Bx3x512x512
static int spade_gb(cs_engine* e, const cs_engine::GB& gb, int C, const half_t* actv, int astride, int aoff, int B, int S,
             const half_t* x, int xshift, const float* stats, int act, half_t* out, hipStream_t st)
{
    // SPADE.forward (util.py:295-302): gamma/beta convs fused, modulation applied in the epilogue
    ConvCall c = mk(gb.conv, actv + aoff, nhwc(nullptr, S, S, astride), B, 1, S, S);
    c.mode = MODE_SPADE;
    c.p.Cout = C;
    c.p.bias = gb.bg; c.p.bias2 = gb.bb;
    const int Sx = S >> xshift;
    c.p.res = nhwc((void*)x, Sx, Sx, C); c.p.res_f32 = 0; c.p.res_shift = xshift;
    c.p.stats = stats;
    c.p.act0 = act; c.p.slope0 = 0.2f;
    c.p.out0 = nhwc(out, S, S, C);
    return go(e, c, st);   // 128x128 tiles, three resident workgroups per CU (pick_halo_cfg)
}

// The learned shortcut of a SPADEResnetBlock (util.py:329-344, `x_s = conv_s(norm_s(x, seg))`): no activation sits between SPADE's output
// IN(x)(1 + gamma) + beta and the 1x1 conv_s, so the beta half is a composition of two linear maps,
//     conv_s(beta) = conv3x3(actv; W_s W_beta) + W_s b_beta      (one conv 128 -> fout, weights composed at load time, pack.py),
// and only gamma has to be produced per input channel:  x_s = conv_s(IN(x)(1 + gamma)) + conv_s(beta).  Against the fused gamma/beta launch
// this drops the 128 -> fin beta conv (half of it) for a 128 -> fout one: up_0 512 -> 256, up_1 256 -> 64 channels at 128^2 / 256^2.
static int spade_shortcut(cs_engine* e, const cs_engine::SpadeBlk& K, const half_t* actv, int astride, int aoff, int B, int S, const half_t* x,
                   const float* stats, half_t* h, half_t* xs, hipStream_t st)
{
    if (!e->knobs.shortcut_algebra) {        // CANONSWAP_SHORTCUT_ALGEBRA=0, the reference's order: fused gamma/beta launch, then conv_s
        TRY(spade_gb(e, K.ns, K.fin, actv, astride, aoff, B, S, x, 1, stats, ACT_NONE, h, st));
        ConvCall cs = mk(K.cs, h, nhwc(nullptr, S, S, K.fin), B, 1, S, S);
        cs.p.out0 = nhwc(xs, S, S, K.fout);
        return go(e, cs, st);
    }
    ConvCall bs = mk(K.bs, actv + aoff, nhwc(nullptr, S, S, astride), B, 1, S, S);       // conv_s(beta)
    bs.p.out0 = nhwc(e->g_bs, S, S, K.fout);
    TRY(go(e, bs, st));
    ConvCall ng = mk(K.ng, actv + aoff, nhwc(nullptr, S, S, astride), B, 1, S, S);       // h = IN(x)(1 + gamma): ConvParams::spmul
    ng.p.spmul = 1;
    ng.p.res = nhwc((void*)x, S / 2, S / 2, K.fin); ng.p.res_f32 = 0; ng.p.res_shift = 1;   // nn.Upsample(x2) folded into the addressing
    ng.p.stats = stats;
    // up_1 (256 -> 64 channels): one 128 x 256 tile holds every channel of h for its positions, conv_s runs inside that epilogue and h is never
    // stored (ConvParams::xs_w, conv_halo_kernel.h XSK; CANONSWAP_SHORTCUT_FUSE=0: three launches)
    if (e->knobs.shortcut_fuse && K.fin == 256 && K.fout <= 64 && K.cs.Cout_pad == 64 && pick_halo_cfg(ng.p, MODE_STD) == CFG_H_128x256) {
        ng.p.xs_w = K.cs.w; ng.p.xs_cout = K.fout;
        ng.p.xs_res = nhwc(e->g_bs, S, S, K.fout); ng.p.xs_out = nhwc(xs, S, S, K.fout);
        ng.macs_per_pos += K.cs.macs_per_pos;
        e->flops_exec += 2.0 * (double)B * S * S * K.fin * 64.0;
        return go(e, ng, st);
    }
    ng.p.out0 = nhwc(h, S, S, K.fin);
    TRY(go(e, ng, st));
    ConvCall cs = mk(K.cs, h, nhwc(nullptr, S, S, K.fin), B, 1, S, S);
    cs.p.res = nhwc(e->g_bs, S, S, K.fout);
    cs.p.out0 = nhwc(xs, S, S, K.fout);
    return go(e, cs, st);
}

static int run_G(cs_engine* e, int B, const half_t* seg, float* img, hipStream_t st)
{
    ConvCall fc = mk(e->g_fc, seg, nhwc(nullptr, 64, 64, 256), B, 1, 64, 64);
    fc.p.out0 = nhwc(e->g_x[0], 64, 64, 512);
    float* sx = nullptr;             // (mean, rstd) of the current x, produced by the epilogue of the conv that wrote it
    TRY(go_stats(e, fc, 512, 4096, &sx, st));
    // all 18 mlp_shared convs depend only on seg (util.py:298): run up front, the twelve 64x64 ones as one launch
    ConvCall s64 = mk(e->g_sh64, seg, nhwc(nullptr, 64, 64, 256), B, 1, 64, 64);
    s64.p.act0 = ACT_RELU; s64.p.out0 = nhwc(e->g_a64, 64, 64, 1536);
    TRY(go(e, s64, st));
    // mlp_shared of the up blocks reads seg nearest-resized to 128 / 256 (util.py:297-298): run per output row phase on the 64x64
    // source grid and per group of column phases (pack.upsampled_conv_phases): 16/36 and 36/144 of the taps, same result
    // Phases with the same taps and channel count differ in their weights, their leading padding and their output offset only: up to four
    // of them per launch (ConvParams::nphase) - 16 phase convs in 5 launches (4 | 4 + 2 + 4 + 2); at one frame a phase alone is 96 workgroups.
    const bool sh_grouped = e->knobs.phase_group;      // CANONSWAP_PHASE_GROUP=0: one launch per phase (tests: same bits)
    for (int lv = 0; lv < 2; ++lv) {
        const int sc = lv ? 4 : 2, S = 64 * sc;
        half_t* dst = lv ? e->g_a256 : e->g_a128;
        bool done[16] = {};
        // x4 level: output rows 4i + 1 and 4i + 2 read source row i alone - the same taps, the same summed weights (pack.upsampled_conv_phases),
        // the same values.  The a = 1 launches write both rows (out1 = the row below, through the identity second affine); the a = 2 phases
        // are not launched: 12 phase convs -> 9, same bits (CANONSWAP_SHARED_DEDUP=0: A/B, all twelve)
        const bool dd = e->knobs.shared_dedup && sc == 4;
        for (int k = 0; k < e->g_nshp[lv]; ++k) {
            if (dd && e->g_shp[lv][k].a == 2) done[k] = true;
            if (done[k]) continue;
            const cs_engine::ShPhase& P = e->g_shp[lv][k];
            const bool dup = dd && P.a == 1, dupc = P.dupc;      // (a phase duplicates its row or its pixel, not both: one second output)
            ConvCall c = mk(P.conv, seg, nhwc(nullptr, 64, 64, 256), B, 1, 64, 64);
            if (dup) c.macs_per_pos *= 2;      // (the reference's count: this launch stands for two output rows)
            c.p.PH = P.ph; c.p.PW = P.pw;
            c.p.act0 = ACT_RELU;
            // output pixel (sc*i + a, sc*j + b0 + k), channel c  <-  source position (i, j), channel k*384 + c
            if (!sh_grouped) {
                c.p.out0 = td(dst + ((long)P.a * S + P.b0) * 384, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);
                if (dup) c.p.out1 = td(dst + ((long)(P.a + 1) * S + P.b0) * 384, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);
                if (dupc) c.p.out1 = td(dst + ((long)P.a * S + P.b0 + 1) * 384, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);
                TRY(go(e, c, st));
                continue;
            }
            c.p.out0 = td(dst, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);
            if (dup) c.p.out1 = td(dst + (long)S * 384, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);      // (the phase offset applies to both)
            if (dupc) c.p.out1 = td(dst + 384, (long)S * S * 384, 0, (long)sc * S * 384, (long)sc * 384);
            int n = 0;
            for (int j = k; j < e->g_nshp[lv] && n < 4; ++j) {
                const cs_engine::ShPhase& Q = e->g_shp[lv][j];
                if (done[j] || Q.conv.KH != P.conv.KH || Q.conv.KW != P.conv.KW || Q.conv.Cout_pad != P.conv.Cout_pad || (dd && Q.a == 2) || Q.dupc != P.dupc) continue;
                done[j] = true;
                c.p.ph_wofs[n] = (long)(((intptr_t)Q.conv.w - (intptr_t)P.conv.w) / (intptr_t)sizeof(half_t));
                c.p.ph_ooff[n] = (unsigned)(((long)Q.a * S + Q.b0) * 384);
                c.p.ph_PH[n] = Q.ph; c.p.ph_PW[n] = Q.pw;
                if (Q.conv.macs_per_pos != P.conv.macs_per_pos || Q.conv.Cin != P.conv.Cin || Q.conv.KD != P.conv.KD || Q.conv.ragged != P.conv.ragged) { cs_set_error("G.shared: phases of one group differ in more than weights / padding / offset"); return -1; }
                ++n;
            }
            c.p.nphase = n;
            TRY(go(e, c, st));
        }
    }

    int cx = 0;
    for (int b = 0; b < 6; ++b) {   // SPADEResnetBlock 512->512 @64x64 (util.py:329-344)
        const cs_engine::SpadeBlk& K = e->g_blk[b];
        TRY(spade_gb(e, K.n0, 512, e->g_a64, 1536, (b * 2) * 128, B, 64, e->g_x[cx], 0, sx, ACT_LRELU, e->g_h64, st));
        ConvCall c0 = mk(K.c0, e->g_h64, nhwc(nullptr, 64, 64, 512), B, 1, 64, 64);
        c0.p.out0 = nhwc(e->g_dx64, 64, 64, 512);
        float* st1;
        TRY(go_stats(e, c0, 512, 4096, &st1, st));
        TRY(spade_gb(e, K.n1, 512, e->g_a64, 1536, (b * 2 + 1) * 128, B, 64, e->g_dx64, 0, st1, ACT_LRELU, e->g_h64, st));
        ConvCall c1 = mk(K.c1, e->g_h64, nhwc(nullptr, 64, 64, 512), B, 1, 64, 64);
        c1.p.res = nhwc(e->g_x[cx], 64, 64, 512);
        c1.p.out0 = nhwc(e->g_x[cx ^ 1], 64, 64, 512);
        TRY(go_stats(e, c1, 512, 4096, &sx, st));
        cx ^= 1;
    }
    // up_0: nn.Upsample(x2) folded into addressing; 512 -> 256 @128 (learned shortcut)
    {
        const cs_engine::SpadeBlk& K = e->g_blk[6];
        const half_t* x = e->g_x[cx];   // nearest up-sampling leaves per-channel mean / variance unchanged: sx still applies
        TRY(spade_shortcut(e, K, e->g_a128, 384, 256, B, 128, x, sx, e->g_h128, e->g_xs128, st));
        TRY(spade_gb(e, K.n0, 512, e->g_a128, 384, 0, B, 128, x, 1, sx, ACT_LRELU, e->g_h128, st));
        ConvCall c0 = mk(K.c0, e->g_h128, nhwc(nullptr, 128, 128, 512), B, 1, 128, 128);
        c0.p.out0 = nhwc(e->g_dx128, 128, 128, 256);
        float* s1;
        TRY(go_stats(e, c0, 256, 16384, &s1, st));
        TRY(spade_gb(e, K.n1, 256, e->g_a128, 384, 128, B, 128, e->g_dx128, 0, s1, ACT_LRELU, e->g_h1_128, st));
        ConvCall c1 = mk(K.c1, e->g_h1_128, nhwc(nullptr, 128, 128, 256), B, 1, 128, 128);
        c1.p.res = nhwc(e->g_xs128, 128, 128, 256);
        c1.p.out0 = nhwc(e->g_o128, 128, 128, 256);
        TRY(go_stats(e, c1, 256, 16384, &sx, st));
    }
    // up_1: 256 -> 64 @256
    {
        const cs_engine::SpadeBlk& K = e->g_blk[7];
        const half_t* x = e->g_o128;
        TRY(spade_shortcut(e, K, e->g_a256, 384, 256, B, 256, x, sx, e->g_h256, e->g_xs256, st));
        TRY(spade_gb(e, K.n0, 256, e->g_a256, 384, 0, B, 256, x, 1, sx, ACT_LRELU, e->g_h256, st));
        ConvCall c0 = mk(K.c0, e->g_h256, nhwc(nullptr, 256, 256, 256), B, 1, 256, 256);
        c0.p.out0 = nhwc(e->g_dx256, 256, 256, 64);
        float* s1;
        TRY(go_stats(e, c0, 64, 65536, &s1, st));
        TRY(spade_gb(e, K.n1, 64, e->g_a256, 384, 128, B, 256, e->g_dx256, 0, s1, ACT_LRELU, e->g_h1_256, st));
        ConvCall c1 = mk(K.c1, e->g_h1_256, nhwc(nullptr, 256, 256, 64), B, 1, 256, 256);
        c1.p.res = nhwc(e->g_xs256, 256, 256, 64);
        c1.p.out1 = nhwc(e->g_o256, 256, 256, 64);      // leaky_relu(x, 0.2) feeding conv_img (spade_generator.py:56)
        c1.p.act1 = ACT_LRELU; c1.p.slope1 = 0.2f;
        TRY(go(e, c1, st));
    }
    ConvCall ci = mk(e->g_img, e->g_o256, nhwc(nullptr, 256, 256, 64), B, 1, 256, 256);
    ci.mode = MODE_PIXSHUF;
    ci.p.Cout = 16;
    ci.p.act0 = ACT_SIGMOID;
    ci.p.out0 = td(img, 0, 0, 0, 0); ci.p.out0_f32 = 1;
    return go(e, ci, st);
}

// ------------------------------------------------------------------------------------------------ M
// MotionExtractor.forward (motion_extractor.py:33-35 -> convnextv2.py:110-144): img fp32 NCHW 256x256 -> raw head outputs [B][328]
// M's split-precision GEMMs: the activations are stored once as [hi | lo] (2 x creal channels per position) and read as the 3 x creal-channel
// input [hi | lo | hi] the packed weights [W_hi | W_hi | W_lo] expect: chunk j of the conv fetches channels (j mod 2 creal / 32) * 32
static void msplit_in(ConvCall& c, int creal)
{
    c.p.cg = 2 * creal / 32; c.p.cg_cin = 2 * creal; c.p.in_sG = 0;
    c.cg_ck64 = true;
}

// M's three split-precision 1x1 conv forms (engine.h) on the stage with C channels: Cin = 3 x the real input channels (C for pwconv1, 4 C for
// pwconv2 and, after space-to-depth, for the down-sampling conv).
// (pwconv2 of stage 0: 96 output channels in one 128-channel block - 128x128 tiles stage a position's 1152 input channels once; as three
// 32-channel blocks on 128x32 tiles every block staged them again: 0.25 -> 0.17 ms per 64 frames; stage 1's 192 channels as two blocks instead of three 64-channel ones: 0.15 -> 0.16, not taken)
ConvL m_pointwise_layer(int form, int C)
{
    ConvL L;
    L.Cin = form == M_PW1 ? 3 * C : 12 * C;
    L.Cout = form == M_PW1 ? 4 * C : form == M_PW2 ? C : 2 * C;
    L.Cout_pad = form == M_PW2 && C % 64 ? (C + 127) / 128 * 128 : L.Cout;
    L.macs_per_pos = (double)L.Cout * (L.Cin / 3);
    return L;
}

// ... and their launch on an H x H grid (the conv's own: the downsample's output grid); run_M and cs_op_m_pointwise both build their launches here,
// so the operator test runs the engine's routing
ConvCall m_pointwise(const ConvL& L, int form, const half_t* in, float* out, int B, int H, int C)
{
    const int creal = form == M_PW1 ? C : 4 * C;       // real channels of the split input
    ConvCall c = mk(L, in, nhwc(nullptr, H, H, 2 * creal), B, 1, H, H);
    msplit_in(c, creal);
    c.p.out0 = nhwc(out, H, H, L.Cout); c.p.out0_f32 = 1;
    if (form == M_PW1) c.p.act0 = ACT_GELU;                                           // convnextv2.py:39-40
    if (form == M_PW2) { c.p.res = c.p.out0; c.p.res_f32 = 1; }                       // :42 + residual :45
    return c;
}

static int run_M(cs_engine* e, int B, const float* img, float* out, hipStream_t st)
{
    if (!e->has_m) { cs_set_error("the motion extractor weights (M.*) were not uploaded"); return -1; }
    if (!e->m_x) {   // workspace on first use
        const size_t P0 = (size_t)e->maxB * 64 * 64;
        if (e->alloc(&e->m_x, P0 * 96) || e->alloc(&e->m_y, P0 * 96 * 2) || e->alloc(&e->m_h, P0 * 384 * 2) || e->alloc(&e->m_h32, P0 * 384) ||
            e->alloc(&e->m_sumsq, (size_t)e->maxB * 3072 * 16) || e->alloc(&e->m_scale, (size_t)e->maxB * 3072)) return -1;
    }
    TRY(e->run(1, st, [&] { return launch_m_stem(img, e->m_stem_w, e->m_stem_b, e->m_stem_g, e->m_stem_be, e->m_x, B, 256, 256, st); }, "m_stem"));
    int H = 64;
    for (int i = 0; i < 4; ++i) {
        const cs_engine::MStage& S = e->m_st[i];
        const int C = S.C;
        for (int j = 0; j < S.n; ++j) {
            const cs_engine::MBlk& K = S.blk[j];
            TRY(e->run(1, st, [&] { return launch_m_dwln(e->m_x, K.dw_w, K.dw_b, K.ln_g, K.ln_b, e->m_y, B, H, H, C, st); }, "m_dwln"));
            ConvCall a = m_pointwise(K.pw1, M_PW1, e->m_y, e->m_h32, B, H, C);
            TRY(go(e, a, st));
            TRY(e->run(1, st, [&] { return launch_m_grn(e->m_h32, K.grn_g, K.grn_b, e->m_sumsq, e->m_scale, e->m_h, B, H * H, 4 * C, st); }, "m_grn"));
            ConvCall b = m_pointwise(K.pw2, M_PW2, e->m_h, e->m_x, B, H, C);
            TRY(go(e, b, st));
        }
        if (i < 3) {   // downsample_layers[i+1]: LayerNorm + Conv2d(k=2, s=2) as space-to-depth + 1x1 conv
            TRY(e->run(1, st, [&] { return launch_m_ln_s2d(e->m_x, S.ds_g, S.ds_b, e->m_y, B, H, H, C, st); }, "m_ln_s2d"));
            H /= 2;
            ConvCall d = m_pointwise(S.ds, M_DS, e->m_y, e->m_x, B, H, C);
            TRY(go(e, d, st));
        }
    }
    return e->run(1, st, [&] { return launch_m_head(e->m_x, e->m_norm_g, e->m_norm_b, e->m_head_w, e->m_head_b, out, B, H * H, st); }, "m_head");
}

int copy_dd(void* dst, const void* src, size_t bytes, hipStream_t st)
{
    hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    if (r != hipSuccess) { cs_set_error("memcpy d2d: %s", hipGetErrorString(r)); return -1; }
    return 0;
}

static int to_hwdc(cs_engine* e, int B, const float* f, float* out32, half_t* out16, hipStream_t st)
{
    return e->run(1, st, [&] { return launch_ncdhw_to_hwdc(f, out32, out16, B, FC, FD, FH, FW, st); }, "ncdhw_to_hwdc");
}
static int from_hwdc(cs_engine* e, int B, const float* in, float* out, hipStream_t st)
{
    return e->run(1, st, [&] { return launch_hwdc_to_ncdhw(in, out, B, FC, FD, FH, FW, st); }, "hwdc_to_ncdhw");
}

// =================================================================================================== C ABI
extern "C" int cs_create(int device_id, int max_batch, cs_engine** out)
{
    if (!out || max_batch < 1) { cs_set_error("cs_create: bad arguments"); return -1; }
    // the kernels keep per-tensor element offsets in 32 bits; the largest activation (B x 256 x 256 x 384) reaches 2^31 at B = 85
    if (max_batch > 84) { cs_set_error("cs_create: max_batch %d exceeds 84 (32-bit element offsets inside one tensor)", max_batch); return -1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) {
        cs_set_error("cs_create: HIP device %d not available (%d devices visible)", device_id, ndev);
        return -1;
    }
    DevGuard guard(device_id);
    cs_engine* e = new cs_engine();
    e->dev = device_id; e->maxB = max_batch;
    e->knobs = knobs_from_env();      // the A/B switches are taken here, once per engine; no launch reads the environment
    const size_t B = (size_t)max_batch;
#define A(ptr, n) if (e->alloc(&e->ptr, (size_t)(n)) != 0) { cs_destroy(e); return -1; }
    A(f_t0, B * 65536 * 64); A(f_p0, B * 16384 * 128); A(f_p1, B * 4096 * 256);
    for (int i = 0; i < 3; ++i) A(vs[i], B * VOL);
    for (int i = 0; i < 2; ++i) A(va[i], B * VOL);
    for (int i = 0; i < 2; ++i) A(vsp[i], B * VOL * 2);
    A(dm_comp, B * DM_COMP_ELEMS);
    for (int i = 0; i < 6; ++i) A(dm_l[i], B * dm_level_elems(i));
    A(dm_pre, B * VOX * 64); A(dm_pred, B * DM_PRED_ELEMS);
    A(dm_logits, B * DM_LOGIT_FLOATS); A(dm_deform, B * VOX * 3); A(dm_occ, B * 4096);
    A(kpbuf, B * 21 * 3 * 2);
    A(w_t3, B * 4096 * 256); A(seg16, B * 4096 * 256);
    A(tmask, B * 4096 * 4); A(style, 14 * 512);
    A(slot_dev, B);
    e->sk_cap = (size_t)16 << 20;                       // 64 MB of fp32 partials
    A(sk_buf, e->sk_cap);
    CS_CHECK_HIP(hipHostMalloc((void**)&e->slot_pin, sizeof(int) * 16 * B));
    e->stats_slots = 48; e->stats_slot_floats = B * 512 * 2;
    A(stats_pool, e->stats_slots * e->stats_slot_floats);
    A(stats_part, B * 262144); A(dm_occpart, B * 4096 * 64);
    for (int which = CS_G_X0; which <= CS_G_O256; ++which)      // G's workspace (engine.h)
        if (e->alloc(g_buf(e, which).p, B * g_buf(e, which).elems) != 0) { cs_destroy(e); return -1; }
    A(img_a, B * 3 * 512 * 512); A(img_b, B * 3 * 512 * 512);
#undef A
    // the concat buffers carry zero pad channels that are never written: clear once
    CS_CHECK_HIP(hipMemset(e->dm_l[0], 0, B * dm_level_elems(0) * sizeof(half_t)));
    CS_CHECK_HIP(hipMemset(e->dm_pred, 0, B * DM_PRED_ELEMS * sizeof(half_t)));
    *out = e;
    return 0;
}

extern "C" void cs_destroy(cs_engine* e)
{
    if (!e) return;
    DevGuard guard(e->dev);
    hipDeviceSynchronize();
    for (void* p : e->allocs) hipFree(p);
    if (e->slot_pin) hipHostFree(e->slot_pin);
    for (auto& kv : e->blobs) hipFree(kv.second.p);
    for (hipEvent_t ev : e->evpool) hipEventDestroy(ev);
    delete e;
}

extern "C" int cs_upload(cs_engine* e, const char* name, const void* host_ptr, size_t nbytes)
{
    if (!e || !name || !host_ptr || !nbytes) { cs_set_error("cs_upload: bad arguments"); return -1; }
    DevGuard guard(e->dev);
    Blob& b = e->blobs[name];
    if (b.p) { hipFree(b.p); b.p = nullptr; }
    CS_CHECK_HIP(hipMalloc(&b.p, nbytes));
    b.bytes = nbytes; b.paired = false;
    CS_CHECK_HIP(hipMemcpy(b.p, host_ptr, nbytes, hipMemcpyHostToDevice));
    e->finalized = false;
    return 0;
}

extern "C" int cs_finalize_weights(cs_engine* e)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    DevGuard guard(e->dev);
    char n[96];
    // ---- M (optional)
    e->has_m = e->find("M.stem.w") != nullptr;
    if (e->has_m) {
        static const int dims[4] = {96, 192, 384, 768}, depths[4] = {3, 3, 9, 3};
        auto get_m = [&](const std::string& name, int form, int C, ConvL* L) -> int {      // a split-precision 1x1 conv (m_pointwise_layer)
            const ConvL g = m_pointwise_layer(form, C);
            return get_conv(e, name, g.Cin, g.Cout_pad, g.Cout, 1, 1, 1, g.Cout, g.macs_per_pos, L);
        };
        TRY(get_f32(e, "M.stem.w", 48 * 96, &e->m_stem_w)); TRY(get_f32(e, "M.stem.b", 96, &e->m_stem_b));
        TRY(get_f32(e, "M.stem.ln.g", 96, &e->m_stem_g)); TRY(get_f32(e, "M.stem.ln.b", 96, &e->m_stem_be));
        for (int i = 0; i < 4; ++i) {
            cs_engine::MStage& S = e->m_st[i];
            const int C = dims[i];
            S.C = C; S.n = depths[i];
            for (int j = 0; j < S.n; ++j) {
                cs_engine::MBlk& K = S.blk[j];
                snprintf(n, sizeof n, "M.s%d.%d", i, j);
                const std::string q(n);
                TRY(get_f32(e, q + ".dw.w", 49 * C, &K.dw_w)); TRY(get_f32(e, q + ".dw.b", C, &K.dw_b));
                TRY(get_f32(e, q + ".ln.g", C, &K.ln_g)); TRY(get_f32(e, q + ".ln.b", C, &K.ln_b));
                TRY(get_f32(e, q + ".grn.g", 4 * C, &K.grn_g)); TRY(get_f32(e, q + ".grn.b", 4 * C, &K.grn_b));
                TRY(get_m(q + ".pw1", M_PW1, C, &K.pw1));
                TRY(get_m(q + ".pw2", M_PW2, C, &K.pw2));
            }
            if (i < 3) {
                snprintf(n, sizeof n, "M.ds%d", i);
                const std::string q(n);
                TRY(get_f32(e, q + ".ln.g", C, &S.ds_g)); TRY(get_f32(e, q + ".ln.b", C, &S.ds_b));
                TRY(get_m(q, M_DS, C, &S.ds));
            }
        }
        TRY(get_f32(e, "M.norm.g", 768, &e->m_norm_g)); TRY(get_f32(e, "M.norm.b", 768, &e->m_norm_b));
        TRY(get_f32(e, "M.head.w", 328 * 768, &e->m_head_w)); TRY(get_f32(e, "M.head.b", 328, &e->m_head_b));
    }
    // ---- A (optional): the identity network behind getid (pack.py _pack_A)
    e->idn.present = e->find("A.stem.w") != nullptr;
    if (e->idn.present) {
        IdNet& A = e->idn;
        const void* p;
        TRY(need(e, "A.stem.w", (size_t)9 * 64 * 32 * 2, &p)); A.stem_w = (const half_t*)p;
        TRY(get_f32(e, "A.stem.b", 64, &A.stem_b));
        TRY(get_f32(e, "A.slopes", 49, &A.slopes));
        int bi = 0, cin = 64;
        for (int l = 0; l < 4; ++l)
            for (int k = 0; k < IDNET_DEPTH[l]; ++k, ++bi) {
                IdBlock& K = A.blk[bi];
                const int cout = IDNET_C[l];
                K.cin = cin; K.cout = cout; K.stride = (l > 0 && k == 0) ? 2 : 1;
                snprintf(n, sizeof n, "A.b%d", bi);
                const std::string q(n);
                TRY(get_f32(e, q + ".pre.s", cin, &K.s0)); TRY(get_f32(e, q + ".pre.t", cin, &K.t0));
                TRY(need(e, q + ".c1.w", (size_t)9 * cin * cin * 2, &p)); K.w1 = (const half_t*)p;
                TRY(get_f32(e, q + ".c1.b", cin, &K.b1));
                TRY(need(e, q + ".c2.w", (size_t)9 * cout * cin * 2, &p)); K.w2 = (const half_t*)p;
                TRY(get_f32(e, q + ".c2.b", cout, &K.b2));
                K.wd = nullptr; K.bd = nullptr;
                if (K.stride == 2) {
                    TRY(need(e, q + ".ds.w", (size_t)cout * cin * 2, &p)); K.wd = (const half_t*)p;
                    TRY(get_f32(e, q + ".ds.b", cout, &K.bd));
                }
                TRY(get_f32(e, q + ".se.w1", cout / 16 * cout, &K.se_w1)); TRY(get_f32(e, q + ".se.b1", cout / 16, &K.se_b1));
                TRY(get_f32(e, q + ".se.w2", cout * (cout / 16), &K.se_w2)); TRY(get_f32(e, q + ".se.b2", cout, &K.se_b2));
                cin = cout;
            }
        TRY(get_f32(e, "A.post.s", 512, &A.post_s)); TRY(get_f32(e, "A.post.t", 512, &A.post_t));
        TRY(need(e, "A.fc.w", (size_t)49 * 512 * 512 * 2, &p)); A.fc_w = (const half_t*)p;
        TRY(get_f32(e, "A.fc.b", 512, &A.fc_b));
        if (!A.in16) {
            const int cap = e->maxB < 8 ? e->maxB : 8;
            char* ws = nullptr;
            TRY(e->alloc(&ws, idnet_workspace_bytes(cap)));
            idnet_bind_workspace(A, ws, cap);
        }
        A.lastB = 0;
    }
    // ---- P (optional): the SegFormer face parser (pack.py _pack_P); "P.cfg" holds the geometry
    e->psr.present = e->find("P.cfg") != nullptr;
    if (e->psr.present) {
        ParserNet& P = e->psr;
        const void* p;
        int cfg[20];
        TRY(need(e, "P.cfg", sizeof cfg, &p));
        CS_CHECK_HIP(hipMemcpy(cfg, p, sizeof cfg, hipMemcpyDeviceToHost));
        P.mlp = cfg[16]; P.D = cfg[17]; P.L = cfg[18]; P.Lpad = (P.L + 63) / 64 * 64;
        memcpy(&P.eps, &cfg[19], 4);
        if (P.mlp < 1 || P.mlp > 8 || P.D < 64 || P.D % 64 || P.L < 1 || P.L > 4096 || !(P.eps >= 0.f)) { cs_set_error("weights: 'P.cfg' holds an unsupported decode head"); return -1; }
        int cin = 32;
        for (int s = 0; s < 4; ++s) {
            PStage& S = P.st[s];
            S.depth = cfg[s]; S.C = cfg[4 + s]; S.heads = cfg[8 + s]; S.sr = cfg[12 + s];
            const int Cc = S.C, ksz = s ? 3 : 7;
            if (S.depth < 1 || S.depth > P_MAX_DEPTH || Cc < 64 || Cc > 512 || Cc % 64 || S.heads < 1 || Cc % S.heads || (Cc / S.heads != 32 && Cc / S.heads != 64) ||
                S.sr != (8 >> s)) {
                cs_set_error("weights: 'P.cfg' stage %d (depth %d, width %d, heads %d, sr %d) is not supported", s, S.depth, Cc, S.heads, S.sr); return -1;
            }
            snprintf(n, sizeof n, "P.s%d", s);
            const std::string q(n);
            TRY(need(e, q + ".pe.w", (size_t)ksz * ksz * Cc * cin * 2, &p)); S.pew = (const half_t*)p;
            TRY(get_f32(e, q + ".pe.b", Cc, &S.peb));
            TRY(get_f32(e, q + ".peln.g", Cc, &S.pelng)); TRY(get_f32(e, q + ".peln.b", Cc, &S.pelnb));
            TRY(get_f32(e, q + ".ln.g", Cc, &S.lng)); TRY(get_f32(e, q + ".ln.b", Cc, &S.lnb));
            TRY(need(e, q + ".head.w", (size_t)P.D * Cc * 2, &p)); S.headw = (const half_t*)p;
            for (int k = 0; k < S.depth; ++k) {
                PBlock& K = S.blk[k];
                snprintf(n, sizeof n, "P.s%d.b%d", s, k);
                const std::string b(n);
                const int Hd = P.mlp * Cc;
                TRY(get_f32(e, b + ".ln1.g", Cc, &K.ln1g)); TRY(get_f32(e, b + ".ln1.b", Cc, &K.ln1b));
                TRY(get_f32(e, b + ".ln2.g", Cc, &K.ln2g)); TRY(get_f32(e, b + ".ln2.b", Cc, &K.ln2b));
                TRY(need(e, b + ".q.w", (size_t)Cc * Cc * 2, &p)); K.qw = (const half_t*)p; TRY(get_f32(e, b + ".q.b", Cc, &K.qb));
                TRY(need(e, b + ".kv.w", (size_t)2 * Cc * Cc * 2, &p)); K.kvw = (const half_t*)p; TRY(get_f32(e, b + ".kv.b", 2 * Cc, &K.kvb));
                TRY(need(e, b + ".o.w", (size_t)Cc * Cc * 2, &p)); K.ow = (const half_t*)p; TRY(get_f32(e, b + ".o.b", Cc, &K.ob));
                TRY(need(e, b + ".fc1.w", (size_t)Hd * Cc * 2, &p)); K.fc1w = (const half_t*)p; TRY(get_f32(e, b + ".fc1.b", Hd, &K.fc1b));
                TRY(need(e, b + ".fc2.w", (size_t)Hd * Cc * 2, &p)); K.fc2w = (const half_t*)p; TRY(get_f32(e, b + ".fc2.b", Cc, &K.fc2b));
                TRY(get_f32(e, b + ".dw.w", 9 * Hd, &K.dww)); TRY(get_f32(e, b + ".dw.b", Hd, &K.dwb));
                K.srw = nullptr; K.srb = K.srlng = K.srlnb = nullptr;
                if (S.sr > 1) {
                    TRY(need(e, b + ".sr.w", (size_t)S.sr * S.sr * Cc * Cc * 2, &p)); K.srw = (const half_t*)p; TRY(get_f32(e, b + ".sr.b", Cc, &K.srb));
                    TRY(get_f32(e, b + ".srln.g", Cc, &K.srlng)); TRY(get_f32(e, b + ".srln.b", Cc, &K.srlnb));
                }
            }
            cin = Cc;
        }
        TRY(get_f32(e, "P.head.b", P.D, &P.headb));
        TRY(need(e, "P.cls.w", (size_t)P.Lpad * P.D * 2, &p)); P.clsw = (const half_t*)p;
        TRY(get_f32(e, "P.cls.b", P.Lpad, &P.clsb));
        const int cap = e->maxB < P_CHUNK ? e->maxB : P_CHUNK;
        char* ws = nullptr;          // (a reload with another geometry gets a workspace of its own; the old one lives until cs_destroy)
        TRY(e->alloc(&ws, parser_workspace_bytes(P, cap)));
        parser_bind_workspace(P, ws, cap);
        P.lastB = 0;
    }
    // ---- F
    TRY(get_f32(e, "F.first.w", 64 * 27, &e->first_w)); TRY(get_f32(e, "F.first.b", 64, &e->first_b));
    // packed as [W_hi | W_lo] over twice the input channels (run_F: wsplit_in)
    TRY(get_conv(e, "F.down0", 128, 128, 128, 1, 3, 3, 128, 64.0 * 128 * 9, &e->f_down0));
    TRY(get_conv(e, "F.down1", 256, 256, 256, 1, 3, 3, 256, 128.0 * 256 * 9, &e->f_down1));
    TRY(get_conv(e, "F.second", 512, 512, 512, 1, 1, 1, 512, 256.0 * 512, &e->f_second));
    TRY(get_affine(e, "F.pre0", 512, &e->f_pre0));
    for (int which = 0; which < 2; ++which) {
        cs_engine::RB3* rb = which ? e->t_rb : e->f_rb;
        const char* pre = which ? "T" : "F";
        for (int i = 0; i < 6; ++i) {
            snprintf(n, sizeof n, "%s.rb%d.c1", pre, i); TRY(get_conv(e, n, 32, 32, 32, 3, 3, 3, 32, 32.0 * 32 * 27, &rb[i].c1));
            snprintf(n, sizeof n, "%s.rb%d.c2", pre, i); TRY(get_conv(e, n, 32, 32, 32, 3, 3, 3, 32, 32.0 * 32 * 27, &rb[i].c2));
            if (i < 5) { snprintf(n, sizeof n, "%s.rb%d.post", pre, i); TRY(get_affine(e, n, 32, &rb[i].post)); }
        }
    }
    // ---- W
    TRY(get_f32(e, "W.compress.w", 128, &e->cmp_w)); TRY(get_f32(e, "W.compress.b", 4, &e->cmp_b));
    static const int eci[5] = {112, 64, 128, 256, 512}, eco[5] = {64, 128, 256, 512, 1024};
    static const int ecr[5] = {110, 64, 128, 256, 512};
    static const int dci[5] = {1024, 1024, 512, 256, 128}, dco[5] = {512, 256, 128, 64, 32};
    for (int i = 0; i < 5; ++i) {
        snprintf(n, sizeof n, "W.enc%d", i); TRY(get_conv(e, n, eci[i], eco[i], eco[i], 3, 3, 3, eco[i], (double)ecr[i] * eco[i] * 27, &e->w_enc[i]));
        snprintf(n, sizeof n, "W.dec%d", i); TRY(get_conv(e, n, dci[i], dco[i], dco[i], 3, 3, 3, dco[i], (double)dci[i] * dco[i] * 27, &e->w_dec[i]));
        for (int ab = 0; ab < 4; ++ab) {      // algorithmic MACs per (source) position stay those of the 3x3x3 conv
            snprintf(n, sizeof n, "W.dec%d.p%d%d", i, ab >> 1, ab & 1);
            TRY(get_conv(e, n, dci[i], dco[i], dco[i], 3, 2, 2, 0, (double)dci[i] * dco[i] * 27, &e->w_dec_p[i][ab]));
            e->w_dec_p[i][ab].b = e->w_dec[i].b;
        }
    }
    TRY(get_conv(e, "W.tail", 144, 160, 144, 3, 3, 3, 144, 142.0 * 142 * 27, &e->w_tail));
    TRY(get_conv(e, "W.maskp", 144, 160, 160, 7, 7, 1, 0, 142.0 * 22 * 343, &e->w_mask));
    {      // Cin 144 / 144 / 112: the 16 real channels of the last chunk as paired taps (in place, once per upload)
        auto pair = [&](ConvL& L) -> int {
            Blob& bl = e->blobs[L.name + ".w"];          // exists: get_conv found it
            if (!bl.paired && launch_pair_ragged(const_cast<half_t*>(L.w), L.Cout_pad, (L.Cin + 31) / 32, L.KD, L.KH, L.KW, 0)) return -1;
            bl.paired = true; L.ragged = true;
            return 0;
        };
        TRY(pair(e->w_tail)); TRY(pair(e->w_mask));
        TRY(pair(e->w_enc[0]));
    }
    TRY(get_f32(e, "W.mask.b", 32, &e->mask_b));
    TRY(get_conv(e, "W.occp", 16 * 160, 32, 16, 1, 7, 1, 0, 2272.0 * 49, &e->w_occ));
    TRY(get_conv(e, "W.occ49", 16 * 160, 64, 64, 1, 1, 1, 0, 2272.0 * 49, &e->w_occ49));
    { const Blob* b = e->find("W.occ.b"); if (!b || b->bytes != 4) { cs_set_error("weights: W.occ.b missing"); return -1; }
      CS_CHECK_HIP(hipMemcpy(&e->occ_b, b->p, 4, hipMemcpyDeviceToHost)); }
    TRY(get_conv(e, "W.third", 512, 256, 256, 1, 3, 3, 256, 512.0 * 256 * 9, &e->w_third));
    TRY(get_conv(e, "W.fourth", 256, 256, 256, 1, 1, 1, 256, 256.0 * 256, &e->w_fourth));
    // ---- T
    for (int i = 0; i < 14; ++i) {
        TLayer& L = e->t_l[i];
        snprintf(n, sizeof n, "T.b%d.c%d", i / 2, i % 2 + 1);
        std::string base = n;
        TRY(get_conv(e, base, 512, 1024, 512, 1, 3, 3, 0, 2.0 * 512 * 512 * 9, &L.fused));
        L.wset[0] = (half_t*)L.fused.w;
        if (!L.wofs) { TRY(e->alloc(&L.wofs, (size_t)MAX_SLOTS)); }
        long ofs[MAX_SLOTS];
        for (int sl = 0; sl < MAX_SLOTS; ++sl) ofs[sl] = L.wset[sl] ? (long)(L.wset[sl] - L.wset[0]) : 0;
        CS_CHECK_HIP(hipMemcpy(L.wofs, ofs, sizeof(ofs), hipMemcpyHostToDevice));
        TRY(get_conv(e, base + ".mask", 512, 16, 4, 1, 3, 3, 4, 512.0 * 1 * 9, &L.mask));
        TRY(get_f32(e, base + ".raw", 512 * 9 * 512, &L.raw));
        TRY(get_f32(e, base + ".fc", 2 * (512 * 512 + 512), &L.fc));
        TRY(get_f32(e, base + ".bias", 512, &L.bias));
    }
    TRY(get_affine(e, "T.pre0", 512, &e->t_pre0));
    // ---- R
    for (int which = 0; which < 2; ++which) {
        cs_engine::S3* s = which ? e->r_s3 : e->r_s1;
        for (int i = 0; i < 3; ++i) {
            snprintf(n, sizeof n, "R.s%d.%d", which ? 3 : 1, i);
            std::string b = n;
            TRY(get_conv(e, b + ".c1", 32, 32, 32, 3, 3, 3, 32, 32.0 * 32 * 27, &s[i].c1));
            TRY(get_conv(e, b + ".c2", 32, 32, 32, 3, 3, 3, 32, 32.0 * 32 * 27, &s[i].c2));
            TRY(get_conv(e, b + ".c1.sp", 96, 32, 32, 3, 3, 3, 0, 32.0 * 32 * 27, &s[i].c1sp)); s[i].c1sp.b = s[i].c1.b;
            TRY(get_conv(e, b + ".c2.sp", 96, 32, 32, 3, 3, 3, 0, 32.0 * 32 * 27, &s[i].c2sp)); s[i].c2sp.b = s[i].c2.b;
            TRY(get_f32(e, b + ".gn1.w", 32, &s[i].g1)); TRY(get_f32(e, b + ".gn1.b", 32, &s[i].b1));
            TRY(get_f32(e, b + ".gn2.w", 32, &s[i].g2)); TRY(get_f32(e, b + ".gn2.b", 32, &s[i].b2));
        }
    }
    for (int i = 0; i < 3; ++i) {
        snprintf(n, sizeof n, "R.rb2.%d", i);
        std::string b = n;
        TRY(get_conv(e, b + ".c1", 512, 512, 512, 1, 3, 3, 512, 512.0 * 512 * 9, &e->r_rb2[i].c1));
        TRY(get_conv(e, b + ".c2", 512, 512, 512, 1, 3, 3, 512, 512.0 * 512 * 9, &e->r_rb2[i].c2));
        TRY(get_affine(e, b + ".pre", 512, &e->r_rb2[i].pre));
    }
    // ---- G
    TRY(get_conv(e, "G.fc", 256, 512, 512, 1, 3, 3, 512, 256.0 * 512 * 9, &e->g_fc));
    TRY(get_conv(e, "G.shared64", 256, 1536, 1536, 1, 3, 3, 1536, 256.0 * 1536 * 9, &e->g_sh64));
    TRY(get_conv(e, "G.shared128", 256, 384, 384, 1, 3, 3, 384, 256.0 * 384 * 9, &e->g_sh128));
    TRY(get_conv(e, "G.shared256", 256, 384, 384, 1, 3, 3, 384, 256.0 * 384 * 9, &e->g_sh256));
    for (int lv = 0; lv < 2; ++lv) {      // pack.upsampled_conv_phases: row phase a x groups of column phases with equal source columns
        const int sc = lv ? 4 : 2;
        e->g_nshp[lv] = 0;
        for (int a = 0; a < sc; ++a) {
            const int kh = (a == 0 || a == sc - 1) ? 2 : 1, ph = a == 0 ? 1 : 0;
            for (int b0 = 0; b0 < sc; ) {
                const bool edge = b0 == 0 || b0 == sc - 1;
                const int nb = edge ? 1 : sc - 2, kw = edge ? 2 : 1, pw = b0 == 0 ? 1 : 0;
                cs_engine::ShPhase& P = e->g_shp[lv][e->g_nshp[lv]++];
                P.a = a; P.b0 = b0; P.ph = ph; P.pw = pw;
                // x4 level: the two middle column phases of a two-row phase are the same values - packed once (pack._pack_G), written twice (run_G)
                P.dupc = sc == 4 && nb == 2 && kh == 2;
                const int nbw = P.dupc ? 1 : nb;
                snprintf(n, sizeof n, "G.shared%d.p%d%d", lv ? 256 : 128, a, b0);
                // algorithmic MACs stay those of the 3x3 conv on the up-sampled grid: nb*sc... output pixels per source position
                TRY(get_conv(e, n, 256, nbw * 384, nbw * 384, 1, kh, kw, nbw * 384, 256.0 * 384 * 9 * nb, &P.conv));
                b0 += nb;
            }
        }
        // run_G launches phases of equal tap shape and width as ONE grouped launch that applies the first member's bias to all of them:
        // hold the blobs to that here, once (pack.py replicates mlp_shared's bias per phase)
        for (int i = 0; i < e->g_nshp[lv]; ++i)
            for (int j = i + 1; j < e->g_nshp[lv]; ++j) {
                const ConvL &A = e->g_shp[lv][i].conv, &Bc = e->g_shp[lv][j].conv;
                if (A.KH != Bc.KH || A.KW != Bc.KW || A.Cout_pad != Bc.Cout_pad) continue;
                std::vector<float> ha(A.Cout_pad), hb(A.Cout_pad);
                CS_CHECK_HIP(hipMemcpy(ha.data(), A.b, ha.size() * sizeof(float), hipMemcpyDeviceToHost));
                CS_CHECK_HIP(hipMemcpy(hb.data(), Bc.b, hb.size() * sizeof(float), hipMemcpyDeviceToHost));
                if (memcmp(ha.data(), hb.data(), ha.size() * sizeof(float))) {
                    cs_set_error("weights: '%s.b' and '%s.b' differ; phases of one grouped launch share one bias", A.name.c_str(), Bc.name.c_str());
                    return -1;
                }
            }
    }
    auto get_gb = [&](const std::string& b, int C, cs_engine::GB* gb) -> int {
        const int pad = ((2 * C + 127) / 128) * 128;
        TRY(get_conv(e, b, 128, pad, C, 1, 3, 3, 0, 128.0 * 2 * C * 9, &gb->conv));
        TRY(get_f32(e, b + ".bg", C, &gb->bg)); TRY(get_f32(e, b + ".bb", C, &gb->bb));
        return 0;
    };
    for (int k = 0; k < 8; ++k) {
        cs_engine::SpadeBlk& K = e->g_blk[k];
        std::string b;
        if (k < 6) { snprintf(n, sizeof n, "G.m%d", k); b = n; K.fin = 512; K.fout = 512; }
        else if (k == 6) { b = "G.up0"; K.fin = 512; K.fout = 256; }
        else { b = "G.up1"; K.fin = 256; K.fout = 64; }
        K.fmid = K.fin < K.fout ? K.fin : K.fout;
        K.learned = K.fin != K.fout;
        TRY(get_gb(b + ".n0", K.fin, &K.n0));
        TRY(get_gb(b + ".n1", K.fmid, &K.n1));
        TRY(get_conv(e, b + ".c0", K.fin, K.fmid, K.fmid, 1, 3, 3, K.fmid, (double)K.fin * K.fmid * 9, &K.c0));
        TRY(get_conv(e, b + ".c1", K.fmid, K.fout, K.fout, 1, 3, 3, K.fout, (double)K.fmid * K.fout * 9, &K.c1));
        if (K.learned) {
            // norm_s (pack.py _pack_G): its gamma conv alone, and conv_s o mlp_beta as one 3x3 conv 128 -> fout.  MACs: what the reference executes
            // (gamma + beta convs 128 -> 2 fin) is booked on the first, the composed conv is executed work only
            TRY(get_gb(b + ".ns", K.fin, &K.ns));
            TRY(get_conv(e, b + ".ng", 128, K.fin, K.fin, 1, 3, 3, K.fin, 128.0 * 2 * K.fin * 9, &K.ng));
            TRY(get_conv(e, b + ".bs", 128, K.fout, K.fout, 1, 3, 3, K.fout, 0.0, &K.bs));
            TRY(get_conv(e, b + ".cs", K.fin, K.fout, K.fout, 1, 1, 1, K.fout, (double)K.fin * K.fout, &K.cs));
        }
    }
    TRY(get_conv(e, "G.img", 64, 16, 16, 1, 3, 3, 16, 64.0 * 12 * 9, &e->g_img));
    for (int sl = 0; sl < MAX_SLOTS; ++sl) e->slot_set[sl] = false;      // modulated weights derive from the (new) raw weights
    e->finalized = true;
    return 0;
}

extern "C" int cs_set_identity(cs_engine* e, int slot, const float* id, void* stream)
{
    if (!e || !e->finalized) { cs_set_error("cs_set_identity: engine not finalized"); return -1; }
    if (slot < 0 || slot >= MAX_SLOTS) { cs_set_error("cs_set_identity: slot %d outside [0, %d)", slot, MAX_SLOTS); return -1; }
    hipStream_t st = (hipStream_t)stream;
    DevGuard guard(e->dev);
    for (int i = 0; i < 14; ++i) {
        TLayer& L = e->t_l[i];
        if (!L.wset[slot]) {     // first use of this slot: own buffer for the fused [W; w_mod] rows
            half_t* w = nullptr;
            TRY(e->alloc(&w, T_FUSED_ELEMS));
            L.wset[slot] = w;
            const long ofs = w - L.wset[0];
            CS_CHECK_HIP(hipMemcpy(L.wofs + slot, &ofs, sizeof(long), hipMemcpyHostToDevice));
        }
        // the shared W rows come from slot 0's blob: copied on the slot's first use AND after every cs_finalize_weights (a new
        // checkpoint clears slot_set; an old copy would pair the previous W rows with the new w_mod rows - ADVICE r2)
        if (slot != 0 && !e->slot_set[slot]) TRY(copy_dd(L.wset[slot], L.wset[0], T_FUSED_ELEMS * sizeof(half_t), st));
        TRY(e->run(1, st, [&] { return launch_t_style(id, L.fc, e->style + i * 512, 1, st); }, "t_style"));
        TRY(e->run(1, st, [&] { return launch_t_modulate(L.raw, e->style + i * 512, L.wset[slot], i, st); }, "t_modulate"));
    }
    e->slot_set[slot] = true;
    return 0;
}

extern "C" int cs_extract_feature_3d(cs_engine* e, int B, const float* img, float* f_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    int cur = 0;
    int r = run_F(e, B, img, &cur, st);
    if (r == 0) r = from_hwdc(e, B, e->vs[cur], f_out, st);
    return e->stop_result(r);      // cs_op_v_stop: stopped where the test asked
}

extern "C" int cs_warp(cs_engine* e, int B, const float* f, const float* kp_source, const float* kp_driving, float* f_out,
                       float* occ_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    TRY(to_hwdc(e, B, f, e->vs[0], nullptr, st));
    TRY(run_dense_motion(e, B, e->vs[0], kp_driving, kp_source, st, e->vs[0], e->vs[1], nullptr));      // dense motion + the feature warp it drives
    TRY(from_hwdc(e, B, e->vs[1], f_out, st));
    if (occ_out) TRY(copy_dd(occ_out, e->dm_occ, (size_t)B * 4096 * 4, st));
    return 0;
}

extern "C" int cs_warp_out(cs_engine* e, int B, const float* f, const float* occ, float* seg_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    TRY(to_hwdc(e, B, f, nullptr, e->va[0], st));
    TRY(run_warp_out(e, B, e->va[0], occ, st));
    return e->run(1, st, [&] { return launch_nhwc16_to_nchw(e->seg16, seg_out, B, 256, 4096, st); }, "nhwc16_to_nchw");
}

extern "C" int cs_swap_ids(cs_engine* e, const int* slots, int B, const float* f, float* f_out, void* stream)
{
    ENTER(e, B);
    if (!slots) { cs_set_error("cs_swap_ids: null slot vector"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    int cur = 0;
    TRY(to_hwdc(e, B, f, e->vs[0], e->va[0], st));
    TRY(run_T(e, B, slots, &cur, st));
    return from_hwdc(e, B, e->vs[cur], f_out, st);
}

extern "C" int cs_swap(cs_engine* e, int slot, int B, const float* f, float* f_out, void* stream)
{
    if (B < 1) { cs_set_error("batch %d", B); return -1; }
    std::vector<int> slots((size_t)B, slot);
    return cs_swap_ids(e, slots.data(), B, f, f_out, stream);
}

extern "C" int cs_refine(cs_engine* e, int B, const float* f, float* f_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    int cur = 0;
    int r = to_hwdc(e, B, f, e->vs[0], e->va[0], st);
    if (r == 0) r = run_R(e, B, &cur, st);
    if (r == 0) r = from_hwdc(e, B, e->vs[cur], f_out, st);
    return e->stop_result(r);      // cs_op_v_stop: stopped where the test asked
}

extern "C" int cs_warp_forward(cs_engine* e, int B, const float* f, const float* kp_driving, const float* kp_source,
                               float* occ_out, float* deformation_out, float* seg_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    TRY(to_hwdc(e, B, f, e->vs[0], nullptr, st));
    TRY(run_dense_motion(e, B, e->vs[0], kp_driving, kp_source, st, e->vs[0], nullptr, e->va[0], deformation_out != nullptr));      // dense motion + the feature warp it drives
    TRY(run_warp_out(e, B, e->va[0], e->dm_occ, st));
    if (seg_out) TRY(e->run(1, st, [&] { return launch_nhwc16_to_nchw(e->seg16, seg_out, B, 256, 4096, st); }, "nhwc16_to_nchw"));
    if (occ_out) TRY(copy_dd(occ_out, e->dm_occ, (size_t)B * 4096 * 4, st));
    if (deformation_out) TRY(copy_dd(deformation_out, e->dm_deform, (size_t)B * VOX * 3 * 4, st));
    return 0;
}

extern "C" int cs_spade_decode(cs_engine* e, int B, const float* seg, float* img_out, void* stream)
{
    ENTER(e, B);
    hipStream_t st = (hipStream_t)stream;
    int r = e->run(1, st, [&] { return launch_nchw_to_nhwc16(seg, e->seg16, B, 256, 4096, st); }, "nchw_to_nhwc16");
    if (r == 0) r = run_G(e, B, e->seg16, img_out, st);
    return e->stop_result(r);      // cs_op_g_stop: stopped where the test asked
}

extern "C" int cs_motion_extract(cs_engine* e, int B, const float* img, float* out, void* stream)
{
    ENTER(e, B);
    return run_M(e, B, img, out, (hipStream_t)stream);
}

extern "C" int cs_pack_u8(cs_engine* e, int B, const float* img, uint8_t* out, int H, int W, void* stream)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_pack_u8(img, out, B, 3, H, W, st); }, "pack_u8");
}

extern "C" int cs_unpack_u8(cs_engine* e, int B, const uint8_t* img, float* out, int H, int W, void* stream)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_unpack_u8(img, out, B, 3, H, W, st); }, "unpack_u8");
}

extern "C" int cs_swap_frames(cs_engine* e, int slot, int B, const float* img, const float* x_t, const float* x_can,
                              float* out_f32, uint8_t* out_u8, float* rec_can, float* swap_can, void* stream)
{
    if (B < 1) { cs_set_error("batch %d", B); return -1; }
    std::vector<int> slots((size_t)B, slot);
    return cs_swap_frames_ids(e, slots.data(), B, img, x_t, x_can, out_f32, out_u8, rec_can, swap_can, stream);
}

extern "C" int cs_swap_frames_ids(cs_engine* e, const int* slots, int B, const float* img, const float* x_t, const float* x_can,
                                  float* out_f32, uint8_t* out_u8, float* rec_can, float* swap_can, void* stream)
{
    ENTER(e, B);
    if (!slots) { cs_set_error("cs_swap_frames_ids: null slot vector"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    int cur = 0;
    TRY(run_F(e, B, img, &cur, st));                                                      // :242 f_s
    // :244 warp(f_s, kp_source = x_t, kp_driving = x_can)
    const int nxt = (cur + 1) % 3;
    TRY(run_dense_motion(e, B, e->vs[cur], /*kp_d*/ x_can, /*kp_s*/ x_t, st, e->vs[cur], e->vs[nxt], e->va[0]));      // dense motion + the feature warp it drives
    cur = nxt;
    // the first warp's occlusion map is reused by the debug decodes (:248,:257); keep a copy in tmask-free storage
    float* occ1 = e->img_b;   // B*4096 floats fit easily
    if (rec_can || swap_can) TRY(copy_dd(occ1, e->dm_occ, (size_t)B * 4096 * 4, st));
    if (rec_can) {                                                                          // :248
        TRY(run_warp_out(e, B, e->va[0], occ1, st));
        TRY(run_G(e, B, e->seg16, rec_can, st));
    }
    TRY(run_T(e, B, slots, &cur, st));                                                      // :253
    if (swap_can) {                                                                         // :257
        TRY(run_warp_out(e, B, e->va[0], occ1, st));
        TRY(run_G(e, B, e->seg16, swap_can, st));
    }
    TRY(run_R(e, B, &cur, st));                                                             // :262
    // :263 warp_decode(f, kp_source = x_can, kp_driving = x_t)
    TRY(run_dense_motion(e, B, e->vs[cur], /*kp_d*/ x_t, /*kp_s*/ x_can, st, e->vs[cur], nullptr, e->va[0]));      // dense motion + the feature warp it drives
    TRY(run_warp_out(e, B, e->va[0], e->dm_occ, st));
    float* dst = out_f32 ? out_f32 : e->img_a;
    TRY(run_G(e, B, e->seg16, dst, st));
    if (out_u8) TRY(e->run(1, st, [&] { return launch_pack_u8(dst, out_u8, B, 3, 512, 512, st); }, "pack_u8"));
    return 0;
}

// v2i per-frame body (can_swap_pipeline_v2i.py:311-312: warp_decode of ONE swapped canonical feature volume under per-frame
// driving key-points). nf / ns = 1 (shared by all B frames) or B.
extern "C" int cs_animate_frames(cs_engine* e, int B, const float* f, int nf, const float* kp_source, int ns, const float* kp_driving,
                                 float* out_f32, uint8_t* out_u8, void* stream)
{
    ENTER(e, B);
    if ((nf != 1 && nf != B) || (ns != 1 && ns != B)) { cs_set_error("cs_animate_frames: nf / ns must be 1 or B"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    TRY(to_hwdc(e, nf, f, e->vs[0], nullptr, st));
    // nf == 1 / ns == 1: the one volume / key-point set is broadcast by a zero sample stride in the kernels that read it (round 6; before: B - 1
    // device copies of 8.4 MB and B of 252 bytes per call)
    TRY(run_dense_motion(e, B, e->vs[0], kp_driving, kp_source, st, e->vs[0], nullptr, e->va[0], false, nf == 1 && B > 1, ns == 1 && B > 1));
    TRY(run_warp_out(e, B, e->va[0], e->dm_occ, st));
    float* dst = out_f32 ? out_f32 : e->img_a;
    TRY(run_G(e, B, e->seg16, dst, st));
    if (out_u8) TRY(e->run(1, st, [&] { return launch_pack_u8(dst, out_u8, B, 3, 512, 512, st); }, "pack_u8"));
    return 0;
}

extern "C" int cs_profile_begin(cs_engine* e)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    e->prof = true; e->recs.clear(); e->evnext = 0; e->flops = 0; e->flops_exec = 0; e->amax_n = 0;
    return 0;
}

extern "C" int cs_profile_end(cs_engine* e, double ms[3], long counts[3], double* flops)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    CS_CHECK_HIP(hipDeviceSynchronize());
    ms[0] = ms[1] = ms[2] = 0; counts[0] = counts[1] = counts[2] = 0;
    FILE* csv = nullptr;
    if (const char* path = getenv("CANONSWAP_PROFILE_CSV")) csv = fopen(path, "w");
    std::vector<unsigned> amax((size_t)e->amax_n);
    if (e->amax_n) CS_CHECK_HIP(hipMemcpy(amax.data(), e->amax_dev, sizeof(unsigned) * e->amax_n, hipMemcpyDeviceToHost));
    if (csv) fprintf(csv, e->amax_n ? "family,label,ms,gflop,fp16_amax\n" : "family,label,ms,gflop\n");
    for (auto& r : e->recs) {
        float t = 0;
        CS_CHECK_HIP(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.fam] += t; counts[r.fam]++;
        if (csv && e->amax_n) {
            float am = -1.f;
            if (r.amax_slot >= 0) memcpy(&am, &amax[r.amax_slot], 4);
            if (am >= 0) fprintf(csv, "%d,%s,%.5f,%.4f,%.6g\n", r.fam, r.label.c_str(), t, r.flops / 1e9, am);
            else fprintf(csv, "%d,%s,%.5f,%.4f,\n", r.fam, r.label.c_str(), t, r.flops / 1e9);
        } else if (csv) fprintf(csv, "%d,%s,%.5f,%.4f\n", r.fam, r.label.c_str(), t, r.flops / 1e9);
    }
    if (csv) fclose(csv);
    if (flops) *flops = e->flops;
    e->prof = false; e->recs.clear(); e->evnext = 0;
    return 0;
}

extern "C" int cs_set_latency_mode(cs_engine* e, int on)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    e->latency_mode = on != 0;
    return 0;
}

extern "C" int cs_profile_exec_flops(cs_engine* e, double* flops)
{
    if (!e || !flops) { cs_set_error("cs_profile_exec_flops: bad arguments"); return -1; }
    *flops = e->flops_exec;
    return 0;
}
