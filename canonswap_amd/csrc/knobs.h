// The engine's A/B switches: every environment variable that selects another form of the same computation, as one
// struct, one table and one reader.  cs_create fills cs_engine::knobs from the environment once; the stages read e->knobs.* and nothing else
// in csrc reads these names, so a form belongs to the engine that was created under it, not to the process or to whichever launch came first.
// None is needed in production: each is the reference side of a test that holds two forms to each other.  tests/test_knobs_cpu.py runs the
// reader on the host and holds the table to INTEGRATION.md.  Host only: no GPU header, no GPU call in here.
#pragma once
#include <cstdlib>

struct Knobs {
    bool vol32;                 // the 3x3x3 32 -> 32 volume convs on vol32.hip (0: conv_halo)
    bool vol32_xf;              // R's GroupNorm apply / hi-lo split inside the consumer conv's staging (0: norm_act / split16 launches); needs vol32
    bool vol32_fused;           // a whole ResBlock3d of F / T per launch (0: two launches per block); needs vol32
    int wide;                   // the wide 2-D 3x3 convs on conv_wide.hip (0: conv_halo; 2: the SPADE gamma / beta convs too)
    bool warp_fused;            // mask softmax -> deformation -> feature warp in one kernel (0: dm_softmax + grid_sample)
    bool dec_phases_deep;       // the hourglass' up-blocks 0 - 2 per output phase in the batched mode (0: 27-tap convs on the up-sampled grid)
    bool phase_group;           // the phases of an up-sampling conv grouped into one launch, in W's hourglass and G's mlp_shared (0: one launch each)
    bool shortcut_algebra;      // G's learned shortcuts with conv_s(beta) composed at load time (0: the reference's order)
    bool shortcut_fuse;         // up_1's conv_s inside the gamma conv's epilogue (0: its own launch)
    bool shared_dedup;          // mlp_shared at the x4 level without the duplicate row phases (0: all twelve)
    bool amax;                  // debug: largest |value| of the fp16 tensors every conv of a profiled step stored (default off)
};

// (environment name, value when unset, field): a set variable counts as atoi() of its value, so an empty or non-numeric one is 0
struct KnobRow { const char* env; int unset; bool Knobs::*flag; int Knobs::*count; };
constexpr KnobRow KNOB_TABLE[] = {
    {"CANONSWAP_VOL32", 1, &Knobs::vol32, nullptr},
    {"CANONSWAP_VOL32_XF", 1, &Knobs::vol32_xf, nullptr},
    {"CANONSWAP_VOL32_FUSED", 1, &Knobs::vol32_fused, nullptr},
    {"CANONSWAP_WIDE", 1, nullptr, &Knobs::wide},
    {"CANONSWAP_WARP_FUSED", 1, &Knobs::warp_fused, nullptr},
    {"CANONSWAP_DEC_PHASES_DEEP", 1, &Knobs::dec_phases_deep, nullptr},
    {"CANONSWAP_PHASE_GROUP", 1, &Knobs::phase_group, nullptr},
    {"CANONSWAP_SHORTCUT_ALGEBRA", 1, &Knobs::shortcut_algebra, nullptr},
    {"CANONSWAP_SHORTCUT_FUSE", 1, &Knobs::shortcut_fuse, nullptr},
    {"CANONSWAP_SHARED_DEDUP", 1, &Knobs::shared_dedup, nullptr},
    {"CANONSWAP_AMAX", 0, &Knobs::amax, nullptr},
};

inline Knobs knobs_from_env()
{
    Knobs k{};
    for (const KnobRow& r : KNOB_TABLE) {
        const char* s = getenv(r.env);
        const int v = s ? atoi(s) : r.unset;
        if (r.flag) k.*r.flag = v != 0;
        else k.*r.count = v;
    }
    k.vol32_xf = k.vol32_xf && k.vol32;            // both are forms of the vol32 kernel's launches
    k.vol32_fused = k.vol32_fused && k.vol32;
    return k;
}
