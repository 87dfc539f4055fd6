// halo_plan() (canonswap_amd/csrc/conv_plan.h) on the cases of tests/conv_cases.py, as cs_op_conv calls it: one input line per case
//   name mode KD KH KW Cin Cout_pad N D H W cfg tile_w tile_h ck        (cfg < 0: the plan's choice; ck 0: the plan's)
// one output line per case with what the launch runs on.  The ConvParams below are filled as mk() (engine.hip) and cs_op_conv (engine_ops.hip) fill the
// fields halo_plan() reads - extents, taps, Cin, nchunks, Cout_pad, cg = 0 - and not by that code itself (it needs the HIP runtime): a change of
// what those two set before the plan, or of what the plan reads, has to be repeated here.  The GPU test cannot see which instantiation ran.
// tests/conv_plan_host.py builds it like harness.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#define __device__
#define __forceinline__ inline
#include "common_stub.h"
#include "conv_plan.h"

int main()
{
    char name[128];
    int mode, KD, KH, KW, Cin, Cout_pad, N, D, H, W, cfg, tw, th, ck;
    while (scanf("%127s %d %d %d %d %d %d %d %d %d %d %d %d %d %d", name, &mode, &KD, &KH, &KW, &Cin, &Cout_pad, &N, &D, &H, &W, &cfg, &tw, &th, &ck) == 15) {
        ConvParams p;
        memset(&p, 0, sizeof(p));
        p.N = N; p.D = D; p.H = H; p.W = W; p.inD = D;
        p.Cin = Cin; p.nchunks = (Cin + 31) / 32;
        p.KD = KD; p.KH = KH; p.KW = KW; p.PD = KD / 2; p.PH = KH / 2; p.PW = KW / 2;
        p.Cout_pad = Cout_pad; p.Cout = Cout_pad;
        const HaloPlan plan = halo_plan(p, mode == MODE_STDSTAT ? MODE_STD : mode, cfg >= 10 ? cfg : -1, tw, th, false);
        const HaloTile T = halo_tile(plan.hcfg);
        printf("%s hcfg=%d ck=%d lgT=%d,%d,%d nT=%d,%d,%d,%d stat_nblk=%d nchunks=%d BM=%d BN=%d wave_px=%d\n", name, plan.hcfg, ck ? ck : plan.ck, p.lgTW, p.lgTH,
               p.lgTD, p.nTW, p.nTH, p.nTD, p.nTN, plan.stat_nblk, p.nchunks, T.BM, T.BN, T.wave_px);
    }
    return 0;
}
