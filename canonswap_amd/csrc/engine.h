// Internal header of the engine's host side: what engine.hip (registry, routing, the generator's stages and entry points), engine_image.hip (the
// image-space entry points) and engine_ops.hip (the cs_op_* test hooks) share.  Kernel sources do not include it.
#pragma once
#include "conv_plan.h"
#include "knobs.h"
#include "../../include/canonswap_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define TRY(x) do { if ((x) != 0) return -1; } while (0)

constexpr int FD = 16, FH = 64, FW = 64, FC = 32;            // feature volume 32x16x64x64
constexpr long VOL = (long)FD * FH * FW * FC;                 // 2,097,152 elements
constexpr long VOX = (long)FD * FH * FW;                      // 65,536 voxels
// dense motion's hourglass: level i is a [FD][S][S][DM_LW[i]] fp16 concat buffer per sample, S = 64 >> i (cs_engine::dm_l)
constexpr int DM_LW[6] = {144, 128, 256, 512, 1024, 1024};    // concat widths per level
constexpr long dm_level_elems(int i) { return (long)FD * (64 >> i) * (64 >> i) * DM_LW[i]; }
static_assert(dm_level_elems(0) == 65536L * 144 && dm_level_elems(3) == 16L * 64 * 512 && dm_level_elems(5) == 16L * 4 * 1024, "hourglass level sizes");
constexpr long DM_LOGIT_FLOATS = VOX / 4 * 220;                     // floats per sample of the mask conv's hand-over (ConvParams::kw_out, 4-column tiles)
constexpr long DM_COMP_ELEMS = VOX * 4, DM_PRED_ELEMS = VOX * 144;  // per sample: the compressed volume (cs_engine::dm_comp), the hourglass output (dm_pred)
constexpr int IMG = 256;
constexpr size_t T_FUSED_ELEMS = (size_t)(512 / 32) * 9 * 1024 * 32;     // a fused [W ; w_mod] weight set of T (TLayer::wset): packed [kstep][1024 rows][32]

struct Blob { void* p = nullptr; size_t bytes = 0; bool paired = false; };     // paired: launch_pair_ragged already ran on it

struct ConvL {            // one packed convolution layer
    const half_t* w = nullptr;
    const float* b = nullptr;
    int Cin = 0, Cout_pad = 0, Cout = 0, KD = 1, KH = 1, KW = 1;
    double macs_per_pos = 0;   // logical (reference) Cin*Cout*taps, for FLOP accounting
    bool ragged = false;       // Cin % 32 == 16 and the last chunk's weights re-packed for paired taps (ConvParams::ragged)
    std::string name;
};

struct Affine { const float* s = nullptr; const float* t = nullptr; };

constexpr int MAX_SLOTS = CS_MAX_IDENTITY_SLOTS;
// wset[s]: the fused [W; w_mod] packed weights of identity slot s (slot 0 lives in the uploaded blob, the others are allocated on
// first use); wofs: element offsets wset[s] - wset[0] in device memory for launches that mix identities
struct TLayer { ConvL fused; ConvL mask; const float* raw; const float* fc; const float* bias; half_t* wset[MAX_SLOTS]; long* wofs; };

struct cs_engine {
    int dev = 0, maxB = 1;
    bool finalized = false;
    bool latency_mode = false;             // single-frame latency: cross-workgroup split-K for launches that cannot fill the chip
    Knobs knobs{};                         // the A/B switches this engine runs under (knobs.h): the environment as cs_create found it
    bool slot_set[MAX_SLOTS] = {};
    int* slot_dev = nullptr;               // per-sample identity slot of the current batch (device)
    int* slot_pin = nullptr;               // pinned staging ring for slot_dev uploads
    int slot_ring = 0;
    std::vector<int> slot_cur;             // what slot_dev holds
    std::map<std::string, Blob> blobs;
    std::vector<void*> allocs;

    // ---- layers
    const float *first_w = nullptr, *first_b = nullptr;
    ConvL f_down0, f_down1, f_second;
    Affine f_pre0;
    struct RB3 { ConvL c1, c2; Affine post; } f_rb[6], t_rb[6];
    const float *cmp_w = nullptr, *cmp_b = nullptr;
    ConvL w_enc[5], w_dec[5], w_tail, w_mask, w_occ, w_occ49, w_third, w_fourth;
    ConvL w_dec_p[5][4];                   // the up-blocks per output phase (a, b) on the source grid
    float occ_b = 0.f;
    const float* mask_b = nullptr;
    TLayer t_l[14];
    Affine t_pre0;
    struct S3 { ConvL c1, c2, c1sp, c2sp; const float *g1, *b1, *g2, *b2; } r_s1[3], r_s3[3];   // *sp: split-precision weights (Cin 96)
    struct RB2 { ConvL c1, c2; Affine pre; } r_rb2[3];
    ConvL g_fc, g_sh64, g_sh128, g_sh256, g_img;
    // mlp_shared convs of the up blocks per output phase group on the source grid; dupc: the value also goes to the next pixel (x4 level, middle
    // columns of a two-row phase)
    struct ShPhase { ConvL conv; int a, b0, ph, pw; bool dupc; };
    ShPhase g_shp[2][12]; int g_nshp[2] = {0, 0};
    struct GB { ConvL conv; const float *bg, *bb; };
    struct SpadeBlk { GB n0, n1, ns; ConvL c0, c1, cs, ng, bs; bool learned; int fin, fmid, fout; } g_blk[8];      // ng / bs: the learned shortcut's norm_s, see run_G

    // motion extractor (optional: present when the "M.*" blobs were uploaded)
    bool has_m = false;
    const float *m_stem_w = nullptr, *m_stem_b = nullptr, *m_stem_g = nullptr, *m_stem_be = nullptr;
    struct MBlk { const float *dw_w, *dw_b, *ln_g, *ln_b, *grn_g, *grn_b; ConvL pw1, pw2; };
    struct MStage { int C, n; MBlk blk[9]; const float *ds_g, *ds_b; ConvL ds; } m_st[4];
    const float *m_norm_g = nullptr, *m_norm_b = nullptr, *m_head_w = nullptr, *m_head_b = nullptr;
    float *m_x = nullptr, *m_sumsq = nullptr, *m_scale = nullptr;
    half_t *m_y = nullptr, *m_h = nullptr;   // split-precision GEMM operands [hi | lo]
    float* m_h32 = nullptr;
    // ArcFace identity network (optional: present when the "A.*" blobs were uploaded); its workspace holds min(max_batch, 8) images per pass
    IdNet idn;
    // SegFormer face parser (optional: present when the "P.*" blobs were uploaded); its workspace holds min(max_batch, P_CHUNK) images of 512 x 512 per pass
    ParserNet psr;
    // soft-erosion scratch (allocated on first use for the largest B*H*W seen)
    float *se_a = nullptr, *se_b = nullptr, *se_part = nullptr; size_t se_cap = 0, se_part_cap = 0;      // se_part: 64 maxima per sample

    // ---- workspace
    half_t *f_t0, *f_p0, *f_p1;
    float* vs[3]; half_t* va[2];
    float* sk_buf = nullptr; size_t sk_cap = 0;      // split-K partial sums (floats)
    half_t* vsp[2];                        // split-precision conv inputs of R's GroupNorm blocks: [hi | lo] per voxel
    half_t *dm_comp, *dm_l[6], *dm_pre, *dm_pred;
    float *dm_logits, *dm_deform, *dm_occ;
    float *kpbuf;
    half_t *w_t3, *seg16;
    float* tmask; float* style;
    float* stats_pool; float* stats_part; float* dm_occpart; size_t stats_slots = 0, stats_next = 0; size_t stats_slot_floats = 0;
    half_t *g_x[2], *g_h64, *g_dx64, *g_a64, *g_a128, *g_a256, *g_h128, *g_xs128, *g_dx128, *g_h1_128, *g_o128;
    half_t *g_h256, *g_xs256, *g_dx256, *g_h1_256, *g_o256;
    half_t* g_bs;         // the beta term of a learned shortcut (conv_s o mlp_beta of norm_s)
    int g_stop = 0;       // tests (cs_op_g_stop / cs_op_v_stop): launches the next cs_spade_decode / cs_extract_feature_3d / cs_refine still runs before it returns; 0: all, -1: it stopped
    float *img_a, *img_b;

    // ---- profiling
    bool prof = false;
    struct Rec { int fam; hipEvent_t a, b; std::string label; double flops; int amax_slot; };
    unsigned* amax_dev = nullptr; int amax_n = 0;          // CANONSWAP_AMAX=1: per-launch |max| of the fp16 outputs of a profiled step
    std::vector<Rec> recs;
    std::vector<hipEvent_t> evpool;
    size_t evnext = 0;
    double flops = 0, flops_exec = 0;

    hipEvent_t ev()
    {
        if (evnext == evpool.size()) { hipEvent_t e; hipEventCreate(&e); evpool.push_back(e); }
        return evpool[evnext++];
    }
    template <class F> int run(int fam, hipStream_t st, F f, const char* label = "", double fl = 0)
    {
        if (!prof) return stop_after(f());
        hipEvent_t a = ev(), b = ev();
        hipEventRecord(a, st);
        int r = f();
        hipEventRecord(b, st);
        recs.push_back({fam, a, b, label, fl, -1});
        return stop_after(r);
    }
    // the launch that uses up g_stop ends the call like a failed one (TRY unwinds); the entry point sees g_stop < 0 and reports success (stop_result)
    int stop_after(int r)
    {
        if (r != 0 || g_stop <= 0 || --g_stop > 0) return r;
        g_stop = -1;
        return -1;
    }
    // what an entry point that honours the stop returns for the status r of its launches: a stop is success, and the counter is 0 afterwards
    int stop_result(int r)
    {
        if (g_stop < 0) r = 0;
        g_stop = 0;
        return r;
    }
    template <class T> int alloc(T** p, size_t n)
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) { cs_set_error("hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e)); return -1; }
        allocs.push_back(q);
        *p = (T*)q;
        return 0;
    }
    const Blob* find(const std::string& n) const
    {
        auto it = blobs.find(n);
        return it == blobs.end() ? nullptr : &it->second;
    }
};

inline TDesc td(void* p, long sN, long sD, long sH, long sW) { return TDesc{p, sN, sD, sH, sW}; }
// contiguous [N][H][W][C]
inline TDesc nhwc(void* p, int H, int W, int C) { return td(p, (long)H * W * C, 0, (long)W * C, C); }
// feature volume [N][H][W][D][C] seen as a 3-D tensor (d stride = C) or as the 512-channel 2-D view
inline TDesc hwdc3(void* p) { return td(p, VOL, FC, (long)FW * FD * FC, (long)FD * FC); }
inline TDesc hwdc2(void* p) { return td(p, VOL, 0, (long)FW * FD * FC, (long)FD * FC); }
// dense-motion tensors [N][D][H][W][stride]
inline TDesc dhwc(void* p, int D, int H, int W, int stride) { return td(p, (long)D * H * W * stride, (long)H * W * stride, (long)W * stride, stride); }

struct ConvCall {
    ConvParams p;
    int cfg = -1, mode = MODE_STD;
    int hcfg = -1;            // forced conv_halo configuration (else derived from Cout_pad)
    int stat_nblk = 0;        // set by go(): partial blocks per sample when p.stat_out is used
    bool cg_ck64 = false;     // grouped input channels (ConvParams::cg) on 64-channel chunks where the kernel allows it (1x1 convs, even cg)
    double macs_per_pos = 0;
    const char* name = "";
};

// engine.hip: a layer's launch, its routing to a kernel, and the pieces the operator hooks share with the stages
ConvCall mk(const ConvL& L, const void* in, TDesc ind, int N, int D, int H, int W, int up_shift = 0);
int go(cs_engine* e, ConvCall& c, hipStream_t st, int prefW = 0, int prefH = 0);
int copy_dd(void* dst, const void* src, size_t bytes, hipStream_t st);
int t_slots(cs_engine* e, int B, const int* slots, bool* mixed, hipStream_t st);
int t_layer(cs_engine* e, int layer, int B, const int* slots, bool mixed, const half_t* in, const float* res32, float* tmask, half_t* out16, float* out32, hipStream_t st);
// M's three split-precision 1x1 conv forms on the stage with C channels: the layer's geometry (cs_finalize_weights and cs_op_m_pointwise build
// their ConvL from it) and its launch on an H x H grid
enum { M_PW1 = 0, M_PW2 = 1, M_DS = 2 };
ConvL m_pointwise_layer(int form, int C);      // Cin, Cout, Cout_pad and macs_per_pos; no weights yet
ConvCall m_pointwise(const ConvL& L, int form, const half_t* in, float* out, int B, int H, int C);

// G's workspace: buffer `which` (CS_G_X0 .. CS_G_O256 of canonswap_hip.h) and its fp16 elements per sample.  cs_create allocates from this table,
// cs_op_g_read and cs_op_g_fill copy and fill by it.
struct GBuf { half_t** p; size_t elems; };
inline GBuf g_buf(cs_engine* e, int which)
{
    const GBuf t[] = {      // in the order of CS_G_X0 .. CS_G_O256
        {&e->g_x[0], 4096 * 512}, {&e->g_x[1], 4096 * 512}, {&e->g_a64, 4096 * 1536}, {&e->g_a128, 16384 * 384}, {&e->g_a256, 65536 * 384},
        {&e->g_h64, 4096 * 512}, {&e->g_dx64, 4096 * 512}, {&e->g_h128, 16384 * 512}, {&e->g_xs128, 16384 * 256}, {&e->g_dx128, 16384 * 256},
        {&e->g_h1_128, 16384 * 256}, {&e->g_o128, 16384 * 256}, {&e->g_bs, 65536 * 64}, {&e->g_h256, 65536 * 256}, {&e->g_xs256, 65536 * 64},
        {&e->g_dx256, 65536 * 64}, {&e->g_h1_256, 65536 * 64}, {&e->g_o256, 65536 * 64}};
    static_assert(sizeof t / sizeof *t == CS_G_O256 + 1 && CS_G_X0 == 0 && CS_G_BS == 12, "one row per CS_G_* buffer, in the enum's order");
    return which >= CS_G_X0 && which <= CS_G_O256 ? t[which] : GBuf{nullptr, 0};
}

// The volume workspace of F and R: buffer `which` (CS_V_T0 .. CS_V_SP1 of canonswap_hip.h) and its bytes per sample.  cs_op_v_read and
// cs_op_v_fill copy and fill by it.
struct VBuf { void* p; size_t bytes; };
inline VBuf v_buf(cs_engine* e, int which)
{
    const VBuf t[] = {      // in the order of CS_V_T0 .. CS_V_SP1
        {e->f_t0, (size_t)65536 * 64 * 2}, {e->f_p0, (size_t)16384 * 128 * 2}, {e->f_p1, (size_t)4096 * 256 * 2},
        {e->vs[0], (size_t)VOL * 4}, {e->vs[1], (size_t)VOL * 4}, {e->vs[2], (size_t)VOL * 4}, {e->va[0], (size_t)VOL * 2}, {e->va[1], (size_t)VOL * 2},
        {e->vsp[0], (size_t)VOL * 4}, {e->vsp[1], (size_t)VOL * 4}};
    static_assert(sizeof t / sizeof *t == CS_V_SP1 + 1 && CS_V_T0 == 0 && CS_V_S0 == 3 && CS_V_STATS == CS_V_SP1 + 1, "one row per CS_V_* buffer, in the enum's order");
    return which >= CS_V_T0 && which <= CS_V_SP1 ? t[which] : VBuf{nullptr, 0};
}

// Every entry point runs with the engine's device current and restores the caller's device on exit (the engine may be driven
// from a thread whose current device is another GPU).
struct DevGuard {
    int prev = -1, dev;
    explicit DevGuard(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) hipSetDevice(dev); }
    ~DevGuard() { if (prev >= 0 && prev != dev) hipSetDevice(prev); }
};
#define ENTER(e, B) TRY(check(e, B)); DevGuard dev_guard_((e)->dev)

inline int check(cs_engine* e, int B)
{
    if (!e) { cs_set_error("null engine"); return -1; }
    if (!e->finalized) { cs_set_error("cs_finalize_weights has not been called"); return -1; }
    if (B < 1 || B > e->maxB) { cs_set_error("batch %d outside [1, %d]", B, e->maxB); return -1; }
    return 0;
}
