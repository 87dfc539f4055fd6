// The reader of the engine's A/B switches (canonswap_amd/csrc/knobs.h) on the host: every case sets the environment, calls knobs_from_env() and
// holds the struct to what the rules of INTEGRATION.md section 4 give, written out here by hand.  One line per case; tests/test_knobs_cpu.py
// runs it and reads the lines.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>
#include "knobs.h"

struct Flag { const char* env; bool Knobs::*field; };
static const Flag DEFAULT_ON[] = {      // (not read from KNOB_TABLE: the table is what is under test)
    {"CANONSWAP_VOL32", &Knobs::vol32}, {"CANONSWAP_VOL32_XF", &Knobs::vol32_xf}, {"CANONSWAP_VOL32_FUSED", &Knobs::vol32_fused},
    {"CANONSWAP_WARP_FUSED", &Knobs::warp_fused}, {"CANONSWAP_DEC_PHASES_DEEP", &Knobs::dec_phases_deep},
    {"CANONSWAP_PHASE_GROUP", &Knobs::phase_group}, {"CANONSWAP_SHORTCUT_ALGEBRA", &Knobs::shortcut_algebra},
    {"CANONSWAP_SHORTCUT_FUSE", &Knobs::shortcut_fuse}, {"CANONSWAP_SHARED_DEDUP", &Knobs::shared_dedup},
};

static Knobs defaults()
{
    Knobs k{};
    for (const Flag& f : DEFAULT_ON) k.*f.field = true;
    k.wide = 1;
    k.amax = false;
    return k;
}

static std::string show(const Knobs& k)
{
    char b[256];
    snprintf(b, sizeof b, "vol32=%d vol32_xf=%d vol32_fused=%d wide=%d warp_fused=%d dec_phases_deep=%d phase_group=%d shortcut_algebra=%d "
             "shortcut_fuse=%d shared_dedup=%d amax=%d", k.vol32, k.vol32_xf, k.vol32_fused, k.wide, k.warp_fused, k.dec_phases_deep, k.phase_group,
             k.shortcut_algebra, k.shortcut_fuse, k.shared_dedup, k.amax);
    return b;
}

static int failed = 0;

static void check(const std::vector<std::pair<const char*, const char*>>& env, const Knobs& want)
{
    for (const Flag& f : DEFAULT_ON) unsetenv(f.env);
    unsetenv("CANONSWAP_WIDE");
    unsetenv("CANONSWAP_AMAX");
    std::string label;
    for (const auto& kv : env) {
        setenv(kv.first, kv.second, 1);
        label += std::string(label.empty() ? "" : " ") + kv.first + "=" + kv.second;
    }
    const std::string got = show(knobs_from_env()), exp = show(want);
    const bool ok = got == exp;
    failed += !ok;
    printf("%s [%s] -> %s", ok ? "ok" : "FAIL", label.c_str(), got.c_str());
    if (!ok) printf("  (expected %s)", exp.c_str());
    printf("\n");
}

int main()
{
    check({}, defaults());
    for (const Flag& f : DEFAULT_ON) {      // each switch off alone: only its field changes (the two forms of the vol32 kernel need the kernel)
        Knobs w = defaults();
        w.*f.field = false;
        if (f.field == &Knobs::vol32) w.vol32_xf = w.vol32_fused = false;
        check({{f.env, "0"}}, w);
    }
    Knobs w = defaults();
    check({{"CANONSWAP_AMAX", "0"}}, w);
    w.wide = 0; check({{"CANONSWAP_WIDE", "0"}}, w);
    w.wide = 2; check({{"CANONSWAP_WIDE", "2"}}, w);
    w = defaults(); w.vol32 = w.vol32_xf = w.vol32_fused = false;
    check({{"CANONSWAP_VOL32", "0"}, {"CANONSWAP_VOL32_XF", "1"}, {"CANONSWAP_VOL32_FUSED", "1"}}, w);
    for (const char* v : {"", "on"}) {      // a value atoi() reads as 0 is off, for a default-on switch as for a default-off one
        for (const Flag& f : DEFAULT_ON) {
            w = defaults();
            w.*f.field = false;
            if (f.field == &Knobs::vol32) w.vol32_xf = w.vol32_fused = false;
            check({{f.env, v}}, w);
        }
        w = defaults(); check({{"CANONSWAP_AMAX", v}}, w);
        w.wide = 0; check({{"CANONSWAP_WIDE", v}}, w);
    }
    w = defaults(); w.amax = true;
    check({{"CANONSWAP_AMAX", "1"}}, w);
    printf("%d cases failed\n", failed);
    return failed != 0;
}
