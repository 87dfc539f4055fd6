// The launch plan of a conv_halo convolution: tile configuration, tile decomposition, chunk width, statistics layout and workgroup mapping as pure
// functions of ConvParams.  go() (engine.hip) and cs_op_conv (engine_ops.hip) both launch what halo_plan() says, so the operator tests run the
// engine's choices; tests/test_conv_plan_cpu.py runs it on the host.  No HIP call in here.
#pragma once
#include "common.h"

// What a CFG_H_* value means as a tile: BM positions x BN packed channels per workgroup, and the positions one wave covers in the epilogue - a
// wave emits one partial-statistics block per wave_px positions (waves that own 128 positions emit two: conv_epilogue.h, EP_SG).  A new tile
// configuration is added here and nowhere else on the host side.
struct HaloTile { int BM, BN, wave_px; };
inline HaloTile halo_tile(int hcfg)
{
    switch (hcfg) {
    case CFG_H_128x128: return {128, 128, 64};
    case CFG_H_128x64: return {128, 64, 64};
    case CFG_H_256x32: return {256, 32, 64};
    case CFG_H_128x32: return {128, 32, 32};
    case CFG_H_128x16: return {128, 16, 32};
    case CFG_H_256x16: return {256, 16, 64};
    case CFG_H_SK128x32: return {128, 32, 32};
    case CFG_H_128x256: return {128, 256, 64};
    case CFG_H_128x160: return {128, 160, 64};
    case CFG_H_256x160: return {256, 160, 64};
    case CFG_H_256x64: return {256, 64, 64};
    }
    return {128, 32, 64};      // no conv_halo configuration: launch_conv_halo refuses it
}

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

inline void set_tile(ConvParams& p, int BM, int prefW, int prefH)
{
    int tw = p.W < prefW ? p.W : prefW;
    int th = p.H < prefH ? p.H : prefH;
    while (tw * th > BM) th >>= 1;
    int tdd = BM / (tw * th);
    if (tdd > p.D) tdd = p.D;
    int tn = BM / (tw * th * tdd);
    p.lgTW = ilog2(tw); p.lgTH = ilog2(th); p.lgTD = ilog2(tdd);
    p.nTW = p.W / tw; p.nTH = p.H / th; p.nTD = p.D / tdd; p.nTN = (p.N + tn - 1) / tn;
}

// The hourglass tail / mask conv (160 packed channels) and the first encoder block (64 channels) run 256-position tiles; the ragged last
// chunk of those layers (Cin 144 / 112) runs paired taps.  (The A/B knobs of rounds 1-4 that selected the older forms are gone:
// profiles/HISTORY.md section 6 keeps their records.)
// SPADE gamma/beta convs with 128 or more modulated channels (Cout_pad % 256 == 0) on 128x256 tiles from three frames up: +0.5 % with the
// conflict-free LDS image (neutral before it).  Those layers keep 64-channel chunks at every batch size (same K order, same bits); the
// 64-channel ones (Cout_pad 128) run 32-channel chunks on 128x128 tiles.
constexpr int HALO_PERSIST = 1;        // ConvParams::persist_total request of every engine launch (persistent tile walk where the kernel has one)
constexpr int XCD_MAP = 2;             // ConvParams::xcd_map of every engine launch (+0.8 % on the step over the plain order, r02 A/B)

inline int pick_halo_cfg(const ConvParams& p, int mode)
{
    const int Cout_pad = p.Cout_pad;
    if (mode == MODE_PIXSHUF) return CFG_H_256x16;
    // 128 positions x 256 channels (64 channels per wave) only exists as the fully unrolled 3x3 / 16x8-tile kernel
    // 2 resident 128x256 workgroups: the T blend convs (N = 1024, 4 channel blocks per tile: +4.7 %).  In round 1 three resident
    // 128x128 workgroups were 4-14 % faster everywhere else (G 3x3 convs, fc, F down-blocks; tools/cmp_layers.py); see below
    // (below 3 frames a 128x256 launch is 128 workgroups or fewer: 128x128 tiles put one on every CU; same K order, same bits)
    // ... and, since the round-2 epilogue / addressing work, for the other 3x3 convs with 256 or more output channels (G 512->512 with
    // and without statistics, R's 512-channel pair, W.third, the SPADE convs above): +0.7 % on the step, the same per-64-position statistics,
    // the same bits.  (Cin: a multiple of 64, of 32 for the T blend convs)
    if ((mode == MODE_TBLEND || mode == MODE_SPADE || mode == MODE_STD || mode == MODE_STDSTAT) && Cout_pad % 256 == 0 && p.KD == 1 && p.KH == 3 &&
        p.KW == 3 && p.W >= 16 && p.H >= 8 && p.Cin % (mode == MODE_TBLEND ? 32 : 64) == 0 && (long)p.N * p.H * p.W >= 3 * 4096) return CFG_H_128x256;
    if (Cout_pad % 128 == 0) {
        // a launch of 128 or fewer 128x128 workgroups leaves half of the 256 CUs idle (one frame: the 512-channel 3x3 convs at 64x64
        // are 32 x 4): 128x64 tiles put a workgroup on every CU.  Same K order per output element, same bits.
        // (the 1x1 convs too - F.second, W.fourth, the learned shortcuts: 64 - 128 workgroups of two or four K-steps per chunk otherwise)
        const long tiles = ((long)p.N * p.D * p.H * p.W + 127) / 128;
        const bool k33 = p.KH == 3 && p.KW == 3, k11 = p.KD == 1 && p.KH == 1 && p.KW == 1 && mode == MODE_STD;
        if ((mode == MODE_STD || mode == MODE_STDSTAT) && (k33 || k11) && tiles * (Cout_pad / 128) <= 128)
            return CFG_H_128x64;
        // ... and the 1x1 convs up to one workgroup per CU: M's stage-3 pwconv2 and last down-sampling conv are 32 x 6 = 192 workgroups of 288 /
        // 144 K-steps each on 128x128 tiles (0.247 -> 0.215 and 0.143 -> 0.118 ms per 64 frames, profiles/r06_q_chain_k11.txt); same bits
        if (k11 && tiles * (Cout_pad / 128) < 256) return CFG_H_128x64;      // (up to 768 - fewer workgroups than resident slots - measured the same)
        return CFG_H_128x128;
    }
    // 64 output channels at 128x128 or more (G's last up block, F's first down block): 256-position tiles (16x16), two position waves x two
    // channel waves - a wave tile of 128 positions halves the weight bytes per MFMA of the 128x64 tile's 64-position wave tiles
    // Same K order per output element; statistics per 16 x 4 positions as on every tile.
    if (Cout_pad == 64 && (mode == MODE_STD || mode == MODE_STDSTAT) && p.KD == 1 && p.KH == 3 && p.KW == 3 && p.Cin % 64 == 0 && p.cg == 0 &&
        p.H % 16 == 0 && p.W % 16 == 0 && p.H >= 128 && !p.sk_out) return CFG_H_256x64;
    if (Cout_pad % 64 == 0) return CFG_H_128x64;
    if (Cout_pad % 32 == 0) return CFG_H_128x32;
    return CFG_H_128x16;
}

struct HaloPlan { int hcfg, ck, stat_nblk; };

// What a conv_halo launch of p runs on.  hcfg: the forced tile configuration, or negative for pick_halo_cfg's; prefW x prefH: the tile's preferred
// footprint, 0 for the default (2-D: 16 x BM / 16, 3-D: 8 x 8); cg_ck64: ConvCall::cg_ck64.  Fills p.lgT* / p.nT*, p.xcd_map and p.persist_total.
inline HaloPlan halo_plan(ConvParams& p, int mode, int hcfg, int prefW, int prefH, bool cg_ck64)
{
    HaloPlan plan;
    plan.hcfg = hcfg >= 0 ? hcfg : pick_halo_cfg(p, mode);
    const HaloTile T = halo_tile(plan.hcfg);
    const bool is3d = p.KD > 1;
    set_tile(p, T.BM, prefW ? prefW : is3d ? 8 : 16, prefH ? prefH : is3d ? 8 : T.BM / 16);
    plan.stat_nblk = p.nTW * p.nTH * p.nTD * (T.BM / T.wave_px);      // partial-statistics blocks per sample: one per wave_px positions
    // SPADE convs run 32-channel chunks: their LDS image is then conflict-free at three workgroups per CU (conv_halo_kernel.h, halo_pad)
    const bool spade_ck32 = mode == MODE_SPADE && p.Cout_pad % 256 != 0;
    // (grouped input channels, ConvParams::cg: 32-channel chunks, except the 1x1 convs that ask for 64 - M's linear layers: a chunk's two
    // halves lie side by side when cg is even; F's [W_hi | W_lo] convs keep their 32-channel chunks and with them their K order)
    const bool k11 = p.KD == 1 && p.KH == 1 && p.KW == 1;
    const bool cg64 = cg_ck64 && k11 && p.cg > 0 && !(p.cg & 1) && p.Cin % 64 == 0 && mode == MODE_STD;
    plan.ck = (!is3d && p.Cin % 64 == 0 && (p.cg == 0 || cg64) && !spade_ck32) ? 64 : 32;
    p.xcd_map = XCD_MAP;
    p.persist_total = HALO_PERSIST;
    return plan;
}
