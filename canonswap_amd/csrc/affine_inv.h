// What cv2.warpAffine derives from its matrix, and the paste-back's face box, for the host and for the device: one text.  The host launchers of
// imgops.hip run it on the caller's double matrices (cs_crop_faces, cs_paste_back_faces, ...), the kernels of landmarks.hip and imgops.hip on
// float32 matrices that never left the device, widened to double (cs_lmk_input, cs_crop_lmk, cs_paste_back_faces_dev): the same operations in the
// same order on both sides, every one rounded on its own.  The including file turns fp contraction off (#pragma clang fp contract(off)) BEFORE
// it includes this header; double `/` is correctly rounded on both sides.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define AFFINE_HD __host__ __device__
#else
#define AFFINE_HD
#endif

struct AffineInv { double m[6]; };      // destination -> source map (what warpAffine derives from M)

AFFINE_HD inline AffineInv invert_affine(const double M[6])      // imgwarp.cpp warpAffine, !WARP_INVERSE_MAP
{
    AffineInv A;
    for (int i = 0; i < 6; ++i) A.m[i] = M[i];
    double D = A.m[0] * A.m[4] - A.m[1] * A.m[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = A.m[4] * D, A22 = A.m[0] * D;
    A.m[0] = A11; A.m[1] *= -D; A.m[3] *= -D; A.m[4] = A22;
    const double b1 = -A.m[0] * A.m[2] - A.m[1] * A.m[5];
    const double b2 = -A.m[3] * A.m[2] - A.m[4] * A.m[5];
    A.m[2] = b1; A.m[5] = b2;
    return A;
}

// The box of the paste-back kernels for one face, A its frame -> crop map.  A pixel (x, y) reads the crop (!outside) only if -1 <= sx <= Wc - 1 and
// -1 <= sy <= Hc - 1, where sx = floor(u + 1/64 + e), u = A0 x + A1 y + A2 and |e| <= 1/1024 + the doubles' rounding (affine_coords: two rint at
// 10 bits, + 16, >> 10), so u lies in [-1.017, Wc - 0.014], v likewise: inside R = [-1.0625, Wc + 0.0625] x [-1.0625, Hc + 0.0625] with 0.045 to
// spare.  The pixels with (u, v) in R are the parallelogram A^-1 R; an affine map takes R's hull to the hull of its four corners, so the box
// of the four corners A^-1 c, widened by one pixel on every side, holds them all, given that A^-1 c is off by less than that pixel: with the
// guards below (entries up to 1e6, linear part at least 1e-3 and of condition (max |a|)^2 / |det| up to 1e4) the doubles' error in a corner that
// lies within 1e5 pixels of the frame is below 1e-2 pixel.  Any other matrix (singular, not finite, a crop above the 32767 at which
// affine_coords saturates) gets the whole frame: the box then prunes nothing, and the result is the same.
AFFINE_HD inline void face_box(const AffineInv& A, int Hc, int Wc, int Ho, int Wo, int (&box)[4])
{
    box[0] = 0; box[1] = 0; box[2] = Wo - 1; box[3] = Ho - 1;
    const double* m = A.m;
    double big = 0, lin = 0;
    for (int i = 0; i < 6; ++i) big = fmax(big, fabs(m[i]));
    for (int i = 0; i < 6; ++i) if (i % 3 != 2) lin = fmax(lin, fabs(m[i]));      // the linear part: entries 0, 1, 3, 4
    const double D = m[0] * m[4] - m[1] * m[3];
    if (!(big <= 1e6) || !(lin >= 1e-3) || !(fabs(D) * 1e4 >= lin * lin) || Hc > 32767 || Wc > 32767) return;
    const double us[2] = {-1.0625, (double)Wc + 0.0625}, vs[2] = {-1.0625, (double)Hc + 0.0625};
    double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
    for (int c = 0; c < 4; ++c) {
        const double du = us[c & 1] - m[2], dv = vs[c >> 1] - m[5];
        const double p[2] = {(m[4] * du - m[1] * dv) / D, (m[0] * dv - m[3] * du) / D};
        for (int k = 0; k < 2; ++k) { lo[k] = fmin(lo[k], p[k]); hi[k] = fmax(hi[k], p[k]); }
    }
    const double top[2] = {(double)Wo - 1, (double)Ho - 1};
    for (int k = 0; k < 2; ++k) {
        const double a = fmax(floor(lo[k]) - 1, 0.), b = fmin(ceil(hi[k]) + 1, top[k]);
        if (!(a <= b)) { box[0] = box[1] = 1; box[2] = box[3] = 0; return; }      // the face does not reach the frame
        box[k] = (int)a; box[k + 2] = (int)b;
    }
}
