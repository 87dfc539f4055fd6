// Landmarks -> the crop's similarity transform, for the device and for the host: the landmark -> matrix path of canonswap_amd/crop.py (parse_pt2 ->
// parse_rect -> estimate_similar_transform -> M_o2c, M_c2o), which restates src/utils/crop.py:98-300, 381-455.  One text: landmarks.hip runs it
// with the 64 lanes of a wave sharing the N points (LmkWave), tests/landmarks_host/geometry.cpp compiles it for the host with one lane (LmkSerial)
// and tests/test_landmarks_cpu.py holds that build to the reference's own matrices.
//
// Arithmetic (include/canonswap_landmarks.h states the contract):
//   * float32 where the reference holds float32 (landmarks, pt2, the axes, centres, sizes, the scale) - every operation written on its own, the
//     including file compiles without fp contraction, so a float32 line here has numpy's bits;
//   * double where the reference holds Python floats (angle, sine, cosine and the rotated matrix's entries, rounded when the float32 matrix is built);
//   * double, rounded once, where the reference calls float32 BLAS / LAPACK or sums N points: the norm of the axis, np.mean(pts), (pts - c) @ R.T,
//     np.linalg.inv (the closed form of an affine inverse).  That error is the smaller one.
// The N points are walked lane by lane (lane l takes points l, l + lanes, ...) and joined through the reducer: sums in a fixed butterfly order,
// extrema are order free.  No atomics: the result does not depend on the schedule.
#pragma once
#include <math.h>
#include "../../include/canonswap_landmarks.h"

#if defined(__HIPCC__)
#define LMK_HD __host__ __device__
#else
#define LMK_HD
#endif

constexpr float LMK_MAX_ENTRY = 1e6f;      // face_box's bound on a matrix entry (imgops.hip): above it a face is refused

// one lane owns everything: the host build, and the reference order of a serial walk
struct LmkSerial {
    LMK_HD double sum(double v) const { return v; }
    LMK_HD float min(float v) const { return v; }
    LMK_HD float max(float v) const { return v; }
    LMK_HD int any(int v) const { return v; }
};

// Why a face is refused (status stays the caller's mark; the reason is the host test's to read)
enum { LMK_OK = 0, LMK_NOT_FINITE = 1, LMK_EMPTY_BOX = 2, LMK_BAD_SCALE = 3, LMK_BIG_ENTRY = 4 };

LMK_HD inline bool lmk_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN and both infinities

// mean of the first n of idx (np.mean over axis 0 of float32 rows: the rows added in order, then the division)
LMK_HD inline void lmk_mean_of(const float* pts, const int* idx, int n, float& x, float& y)
{
    x = pts[2 * idx[0]]; y = pts[2 * idx[0] + 1];
    for (int i = 1; i < n; ++i) { x = x + pts[2 * idx[i]]; y = y + pts[2 * idx[i] + 1]; }
    x = x / (float)n; y = y / (float)n;
}

// pts: N x 2 float32; M: 18 floats, M_o2c 3 x 3 | M_c2o 3 x 3, written by every lane alike (zeros for a refused face).  Every lane of the team
// calls it with its lane number and returns the same reason.
template <class R>
LMK_HD inline int lmk_geometry(const float* pts, int N, const cs_lmk_layout& L, int dsize, float scale, float vy_ratio, int flag_do_rot, int lane,
                               int lanes, const R& red, float (&M)[18])
{
    for (int i = 0; i < 18; ++i) M[i] = 0.f;
    // ---- guard 1: every landmark finite, before anything is formed from them; the same walk sums them (np.mean(pts, axis=0), crop.py:274)
    int bad = 0;
    double sx = 0., sy = 0.;
    for (int i = lane; i < N; i += lanes) {
        const float x = pts[2 * i], y = pts[2 * i + 1];
        bad |= !(lmk_finite(x) && lmk_finite(y));
        sx += (double)x; sy += (double)y;
    }
    if (red.any(bad)) return LMK_NOT_FINITE;
    const float c0x = (float)(red.sum(sx) / (double)N), c0y = (float)(red.sum(sy) / (double)N);

    // ---- parse_pt2 with use_lip (crop.py:98-241): the centre of the eyes, the centre of the lips
    float elx, ely, erx, ery;
    lmk_mean_of(pts, L.left, L.n_eye, elx, ely);
    lmk_mean_of(pts, L.right, L.n_eye, erx, ery);
    const float p0x = (elx + erx) / 2.f, p0y = (ely + ery) / 2.f;
    const float p1x = (pts[2 * L.lip[0]] + pts[2 * L.lip[1]]) / 2.f, p1y = (pts[2 * L.lip[0] + 1] + pts[2 * L.lip[1] + 1]) / 2.f;

    // ---- parse_rect (crop.py:244-300): the axes
    float uyx = p1x - p0x, uyy = p1y - p0y;
    const float length = (float)sqrt((double)uyx * (double)uyx + (double)uyy * (double)uyy);      // np.linalg.norm
    if ((double)length <= 1e-3) { uyx = 0.f; uyy = 1.f; }                                          // no axis to read: the image's own
    else { uyx = uyx / length; uyy = uyy / length; }
    const float uxx = uyy, uxy = -uyx;
    double angle = acos((double)uxx);
    if (uxy < 0.f) angle = -angle;
    // the box in the turned frame: (pts - centre0) @ R.T, R = [ux, uy]
    float lo0 = INFINITY, lo1 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY;
    for (int i = lane; i < N; i += lanes) {
        const float dx = pts[2 * i] - c0x, dy = pts[2 * i + 1] - c0y;
        const float t0 = (float)((double)dx * (double)uxx + (double)dy * (double)uxy);
        const float t1 = (float)((double)dx * (double)uyx + (double)dy * (double)uyy);
        lo0 = fminf(lo0, t0); hi0 = fmaxf(hi0, t0);
        lo1 = fminf(lo1, t1); hi1 = fmaxf(hi1, t1);
    }
    lo0 = red.min(lo0); lo1 = red.min(lo1); hi0 = red.max(hi0); hi1 = red.max(hi1);
    const float c1x = (lo0 + hi0) / 2.f, c1y = (lo1 + hi1) / 2.f;
    const float side = fmaxf(hi0 - lo0, hi1 - lo1);
    // ---- guard 2: the box has a side (all points equal: 0; differences that overflow: not finite)
    if (!(side > 0.f) || !lmk_finite(side)) return LMK_EMPTY_BOX;
    const float size = side * scale;                                   // need_square: both sides
    float cx = (c0x + uxx * c1x) + uyx * c1y, cy = (c0y + uxy * c1x) + uyy * c1y;
    const float off = vy_ratio * size;
    cx = (cx + uxx * (0.f * size)) + uyx * off;                        // vx_ratio = 0: crop_image never forwards it
    cy = (cy + uxy * (0.f * size)) + uyy * off;

    // ---- estimate_similar_transform (crop.py:381-426)
    const float s = (float)dsize / size;
    // ---- guard 3: the scale
    if (!lmk_finite(s) || !(s > 0.f)) return LMK_BAD_SCALE;
    const float tx = (float)(dsize / 2.0), ty = tx;
    float o[6];
    if (flag_do_rot) {
        const double c = cos(angle), sn = sin(angle), sd = (double)s;
        o[0] = (float)(sd * c); o[1] = (float)(sd * sn); o[2] = (float)((double)tx - sd * (c * (double)cx + sn * (double)cy));
        o[3] = (float)(-sd * sn); o[4] = (float)(sd * c); o[5] = (float)((double)ty - sd * (-sn * (double)cx + c * (double)cy));
    } else {
        o[0] = s; o[1] = 0.f; o[2] = tx - s * cx;
        o[3] = 0.f; o[4] = s; o[5] = ty - s * cy;
    }
    // ---- M_c2o = np.linalg.inv of the float32 3 x 3 (crop.py:445-446): the affine inverse in double, rounded once
    const double a = o[0], b = o[1], c2 = o[2], d = o[3], e = o[4], f = o[5];
    const double D = a * e - b * d;
    float v[6];
    v[0] = (float)(e / D); v[1] = (float)(-b / D); v[2] = (float)((b * f - e * c2) / D);
    v[3] = (float)(-d / D); v[4] = (float)(a / D); v[5] = (float)((d * c2 - a * f) / D);
    // ---- guard 4: every entry of both matrices within face_box's bound (NaN fails the comparison)
    for (int i = 0; i < 6; ++i)
        if (!(fabsf(o[i]) <= LMK_MAX_ENTRY) || !(fabsf(v[i]) <= LMK_MAX_ENTRY)) return LMK_BIG_ENTRY;
    for (int i = 0; i < 6; ++i) { M[i] = o[i]; M[9 + i] = v[i]; }
    M[8] = 1.f; M[17] = 1.f;
    return LMK_OK;
}
