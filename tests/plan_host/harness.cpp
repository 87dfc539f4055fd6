// The conv_halo launch plan (canonswap_amd/csrc/conv_plan.h) on the host: one line per (convolution of the engine, batch size) with what
// halo_plan() decides for it.  tests/test_conv_plan_cpu.py compares the output with expected.txt.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#define __device__
#define __forceinline__ inline
#include "common_stub.h"
#include "conv_plan.h"

struct Case {
    const char* name;
    int mode, KD, KH, KW, Cin, cg, Cout_pad, D, H, W;
    int hcfg, prefW, prefH;       // forced configuration (-1: none) and tile preference (0: default), as the engine's stage passes them to go()
    bool stat, cg_ck64;
};

static void run(const Case& c, int N)
{
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.N = N; p.D = c.D; p.H = c.H; p.W = c.W; p.inD = c.D;
    p.Cin = c.Cin; p.nchunks = (c.Cin + 31) / 32; p.cg = c.cg;
    p.KD = c.KD; p.KH = c.KH; p.KW = c.KW; p.PD = c.KD / 2; p.PH = c.KH / 2; p.PW = c.KW / 2;
    p.Cout_pad = c.Cout_pad; p.Cout = c.Cout_pad;
    const HaloPlan plan = halo_plan(p, c.mode, c.hcfg, c.prefW, c.prefH, c.cg_ck64);
    char nblk[16] = "-";
    if (c.stat) snprintf(nblk, sizeof nblk, "%d", plan.stat_nblk);
    printf("%s N=%d hcfg=%d lgT=%d,%d,%d nT=%d,%d,%d,%d ck=%d stat_nblk=%s xcd_map=%d persist_total=%d\n", c.name, N, plan.hcfg, p.lgTW, p.lgTH, p.lgTD,
           p.nTW, p.nTH, p.nTD, p.nTN, plan.ck, nblk, p.xcd_map, p.persist_total);
}

int main()
{
    static const Case cases[] = {
        // F: the [W_hi | W_lo] convs (grouped chunks), the ResBlock3d convs as two launches
        {"F.down0", MODE_STD, 1, 3, 3, 128, 2, 128, 1, 256, 256, -1, 0, 0, false, false},
        {"F.down1", MODE_STD, 1, 3, 3, 256, 4, 256, 1, 128, 128, -1, 0, 0, false, false},
        {"F.second", MODE_STD, 1, 1, 1, 512, 8, 512, 1, 64, 64, -1, 0, 0, false, false},
        {"ResBlock3d", MODE_STD, 3, 3, 3, 32, 0, 32, 16, 64, 64, CFG_H_256x32, 4, 4, false, false},
        {"ResBlock3d.stat", MODE_STD, 3, 3, 3, 32, 0, 32, 16, 64, 64, CFG_H_256x32, 4, 4, true, false},
        {"R.s3.sp", MODE_STD, 3, 3, 3, 96, 0, 32, 16, 64, 64, CFG_H_256x32, 4, 4, true, false},
        // W: hourglass (27-tap and per-phase up-blocks), tail, mask conv, occlusion, warp_out
        {"W.enc0", MODE_STD, 3, 3, 3, 112, 0, 64, 16, 64, 64, CFG_H_256x64, 0, 0, false, false},
        {"W.enc1", MODE_STD, 3, 3, 3, 64, 0, 128, 16, 32, 32, -1, 0, 0, false, false},
        {"W.enc2", MODE_STD, 3, 3, 3, 128, 0, 256, 16, 16, 16, -1, 0, 0, false, false},
        {"W.enc3", MODE_STD, 3, 3, 3, 256, 0, 512, 16, 8, 8, -1, 0, 0, false, false},
        {"W.enc4", MODE_STD, 3, 3, 3, 512, 0, 1024, 16, 4, 4, -1, 0, 0, false, false},
        {"W.dec0", MODE_STD, 3, 3, 3, 1024, 0, 512, 16, 4, 4, -1, 0, 0, false, false},
        {"W.dec1", MODE_STD, 3, 3, 3, 1024, 0, 256, 16, 8, 8, -1, 0, 0, false, false},
        {"W.dec2", MODE_STD, 3, 3, 3, 512, 0, 128, 16, 16, 16, -1, 0, 0, false, false},
        {"W.dec3", MODE_STD, 3, 3, 3, 256, 0, 64, 16, 32, 32, -1, 0, 0, false, false},
        {"W.dec4", MODE_STD, 3, 3, 3, 128, 0, 32, 16, 64, 64, CFG_H_256x32, 4, 4, false, false},
        {"W.dec0.p", MODE_STD, 3, 2, 2, 1024, 0, 512, 16, 2, 2, -1, 0, 0, false, false},
        {"W.dec1.p", MODE_STD, 3, 2, 2, 1024, 0, 256, 16, 4, 4, -1, 0, 0, false, false},
        {"W.dec2.p", MODE_STD, 3, 2, 2, 512, 0, 128, 16, 8, 8, -1, 0, 0, false, false},
        {"W.dec3.p", MODE_STD, 3, 2, 2, 256, 0, 64, 16, 16, 16, -1, 0, 0, false, false},
        {"W.dec4.p", MODE_STD, 3, 2, 2, 128, 0, 32, 16, 32, 32, CFG_H_256x32, 4, 4, false, false},
        {"W.tail", MODE_STD, 3, 3, 3, 144, 0, 160, 16, 64, 64, CFG_H_256x160, 0, 0, false, false},
        {"W.mask", MODE_STD, 7, 7, 1, 144, 0, 160, 16, 64, 64, CFG_H_256x160, 4, 8, false, false},
        {"W.occ49", MODE_STD, 1, 1, 1, 2560, 5, 64, 1, 64, 64, CFG_H_128x64, 0, 0, false, false},
        {"W.occ", MODE_STD, 1, 7, 1, 2560, 5, 32, 1, 64, 64, CFG_H_128x32, 0, 0, false, false},
        {"W.occ.sk", MODE_STD, 1, 7, 1, 2560, 5, 32, 1, 64, 64, CFG_H_SK128x32, 0, 0, false, false},
        {"W.third", MODE_STD, 1, 3, 3, 512, 0, 256, 1, 64, 64, -1, 0, 0, false, false},
        {"W.fourth", MODE_STD, 1, 1, 1, 256, 0, 256, 1, 64, 64, -1, 0, 0, false, false},
        // T, R
        {"T.blend", MODE_TBLEND, 1, 3, 3, 512, 0, 1024, 1, 64, 64, -1, 0, 0, false, false},
        {"R.rb2", MODE_STD, 1, 3, 3, 512, 0, 512, 1, 64, 64, -1, 0, 0, false, false},
        // G
        {"G.fc", MODE_STD, 1, 3, 3, 256, 0, 512, 1, 64, 64, -1, 0, 0, true, false},
        {"G.shared64", MODE_STD, 1, 3, 3, 256, 0, 1536, 1, 64, 64, -1, 0, 0, false, false},
        {"G.shared.p22", MODE_STD, 1, 2, 2, 256, 0, 384, 1, 64, 64, -1, 0, 0, false, false},
        {"G.shared.p21", MODE_STD, 1, 2, 1, 256, 0, 384, 1, 64, 64, -1, 0, 0, false, false},
        {"G.shared.p12", MODE_STD, 1, 1, 2, 256, 0, 384, 1, 64, 64, -1, 0, 0, false, false},
        {"G.shared.p11", MODE_STD, 1, 1, 1, 256, 0, 768, 1, 64, 64, -1, 0, 0, false, false},
        {"G.m.spade", MODE_SPADE, 1, 3, 3, 128, 0, 1024, 1, 64, 64, -1, 0, 0, false, false},
        {"G.m.c", MODE_STD, 1, 3, 3, 512, 0, 512, 1, 64, 64, -1, 0, 0, true, false},
        {"G.up0.bs", MODE_STD, 1, 3, 3, 128, 0, 256, 1, 128, 128, -1, 0, 0, false, false},
        {"G.up0.ng", MODE_STD, 1, 3, 3, 128, 0, 512, 1, 128, 128, -1, 0, 0, false, false},
        {"G.up0.cs", MODE_STD, 1, 1, 1, 512, 0, 256, 1, 128, 128, -1, 0, 0, false, false},
        {"G.up0.n0", MODE_SPADE, 1, 3, 3, 128, 0, 1024, 1, 128, 128, -1, 0, 0, false, false},
        {"G.up0.c0", MODE_STD, 1, 3, 3, 512, 0, 256, 1, 128, 128, -1, 0, 0, true, false},
        {"G.up0.n1", MODE_SPADE, 1, 3, 3, 128, 0, 512, 1, 128, 128, -1, 0, 0, false, false},
        {"G.up0.c1", MODE_STD, 1, 3, 3, 256, 0, 256, 1, 128, 128, -1, 0, 0, true, false},
        {"G.up1.bs", MODE_STD, 1, 3, 3, 128, 0, 64, 1, 256, 256, -1, 0, 0, false, false},
        {"G.up1.ng", MODE_STD, 1, 3, 3, 128, 0, 256, 1, 256, 256, -1, 0, 0, false, false},
        {"G.up1.cs", MODE_STD, 1, 1, 1, 256, 0, 64, 1, 256, 256, -1, 0, 0, false, false},
        {"G.up1.n0", MODE_SPADE, 1, 3, 3, 128, 0, 512, 1, 256, 256, -1, 0, 0, false, false},
        {"G.up1.c0", MODE_STD, 1, 3, 3, 256, 0, 64, 1, 256, 256, -1, 0, 0, true, false},
        {"G.up1.n1", MODE_SPADE, 1, 3, 3, 128, 0, 128, 1, 256, 256, -1, 0, 0, false, false},
        {"G.up1.c1", MODE_STD, 1, 3, 3, 64, 0, 64, 1, 256, 256, -1, 0, 0, false, false},
        {"G.img", MODE_PIXSHUF, 1, 3, 3, 64, 0, 16, 1, 256, 256, -1, 0, 0, false, false},
    };
    static const int batches[] = {1, 2, 3, 32, 64};
    for (const Case& c : cases)
        for (int N : batches) run(c, N);
    // M's split-precision 1x1 convs (grouped chunks on 64-channel chunks): stage i has C channels on an H x H grid
    static const int MC[4] = {96, 192, 384, 768};
    for (int i = 0; i < 4; ++i) {
        const int C = MC[i], H = 64 >> i;
        char name[3][16];
        snprintf(name[0], 16, "M.s%d.pw1", i); snprintf(name[1], 16, "M.s%d.pw2", i); snprintf(name[2], 16, "M.ds%d", i);
        const Case pw1 = {name[0], MODE_STD, 1, 1, 1, 3 * C, 2 * C / 32, 4 * C, 1, H, H, -1, 0, 0, false, true};
        const Case pw2 = {name[1], MODE_STD, 1, 1, 1, 12 * C, 8 * C / 32, C % 64 ? (C + 127) / 128 * 128 : C, 1, H, H, -1, 0, 0, false, true};
        const Case ds = {name[2], MODE_STD, 1, 1, 1, 12 * C, 8 * C / 32, 2 * C, 1, H / 2, H / 2, -1, 0, 0, false, true};
        for (int N : batches) {
            run(pw1, N); run(pw2, N);
            if (i < 3) run(ds, N);
        }
    }
    return 0;
}
