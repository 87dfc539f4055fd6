// canonswap_amd/csrc/lmk_geometry.h compiled for the host: the text the device runs, with one lane (LmkSerial) walking the points.
// tests/test_landmarks_cpu.py builds this into a shared object (no fp contraction, as the device build) and calls it through ctypes.
#include "lmk_geometry.h"

extern "C" int lmk_geometry_host(const float* pts, int N, cs_lmk_layout layout, int dsize, float scale, float vy_ratio, int flag_do_rot, float* M)
{
    float m[18];
    const int why = lmk_geometry(pts, N, layout, dsize, scale, vy_ratio, flag_do_rot, 0, 1, LmkSerial(), m);
    for (int i = 0; i < 18; ++i) M[i] = m[i];
    return why;
}
