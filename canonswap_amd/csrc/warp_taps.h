// The bilinear tap of cv2.warpAffine (INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit images and the staging value u8 / 255, shared by the warp, paste and
// crop kernels of imgops.hip and the landmark runner's crop of landmarks.hip: one text, so that a crop cut by either file has the same bits.
// Device code only.  The including file turns fp contraction off (#pragma clang fp contract(off)) BEFORE it includes this header.
#pragma once
#include "affine_inv.h"      // AffineInv, and invert_affine / face_box for the host and the device

// a byte as the networks' fp32 input: / 255, clipped (can_swap_e2e.py:126-163, human_landmark_runner.py:76)
__device__ __forceinline__ float staged_value(int v) { return fminf(fmaxf((float)v / 255.f, 0.f), 1.f); }

// ---------------------------------------------------------------------------------------------- cv2.warpAffine, INTER_LINEAR
// OpenCV's fixed-point source coordinate of destination pixel (x, y): AB_BITS = 10, INTER_BITS = 5 (imgwarp.cpp warpAffine)
__device__ __forceinline__ void affine_coords(const AffineInv& A, int x, int y, int& sx, int& sy, int& fx, int& fy)
{
    const double AB = 1024.0;
    const long adelta = (long)rint(A.m[0] * (double)x * AB);
    const long bdelta = (long)rint(A.m[3] * (double)x * AB);
    const long X0 = (long)rint((A.m[1] * (double)y + A.m[2]) * AB) + 16;     // AB_SCALE / INTER_TAB_SIZE / 2
    const long Y0 = (long)rint((A.m[4] * (double)y + A.m[5]) * AB) + 16;
    const long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    long ix = X >> 5, iy = Y >> 5;
    ix = ix < -32768 ? -32768 : (ix > 32767 ? 32767 : ix);
    iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
    sx = (int)ix; sy = (int)iy; fx = (int)(X & 31); fy = (int)(Y & 31);
}

// The bilinear read of one destination pixel (remapBilinear, BORDER_CONSTANT 0): the taps are the source elements (sy, sx), (sy, sx + 1),
// (sy + 1, sx), (sy + 1, sx + 1) with the 5-bit fractions fx, fy; a tap outside the source reads 0.  Every warp, paste and crop kernel
// of imgops.hip and landmarks.hip forms its taps here and reads them through tap_u8x3 (below) or tap_f32 (imgops.hip).
struct Tap {
    long o00;                   // element offset of tap (sy, sx); dereferenced only where a tap lies inside
    int fx, fy;
    bool y0, y1, x0, x1;        // rows sy, sy + 1 and columns sx, sx + 1 inside the source
    bool outside;               // all four taps outside: an 8-bit read gives 0, a float read 0.f
};

__device__ __forceinline__ Tap tap_at(const AffineInv& A, int x, int y, int Hs, int Ws)
{
    Tap t;
    int sx, sy;
    affine_coords(A, x, y, sx, sy, t.fx, t.fy);
    t.o00 = (long)sy * Ws + sx;
    t.y0 = (unsigned)sy < (unsigned)Hs; t.y1 = (unsigned)(sy + 1) < (unsigned)Hs;
    t.x0 = (unsigned)sx < (unsigned)Ws; t.x1 = (unsigned)(sx + 1) < (unsigned)Ws;
    t.outside = sx < -1 || sy < -1 || sx >= Ws || sy >= Hs;
    return t;
}

// 8-bit image, 3 interleaved channels, rows of Ws pixels: 15-bit weights (sum 1 << 15), rounded to nearest (remapBilinear, uchar)
__device__ __forceinline__ void tap_u8x3(const unsigned char* __restrict__ src, int Ws, const Tap& t, int (&res)[3])
{
    const int w00 = (32 - t.fy) * (32 - t.fx) * 32, w01 = (32 - t.fy) * t.fx * 32, w10 = t.fy * (32 - t.fx) * 32, w11 = t.fy * t.fx * 32;
    const unsigned char* p = src + t.o00 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t00 = (t.y0 && t.x0) ? p[c] : 0;
        const int t01 = (t.y0 && t.x1) ? p[3 + c] : 0;
        const int t10 = (t.y1 && t.x0) ? p[(long)Ws * 3 + c] : 0;
        const int t11 = (t.y1 && t.x1) ? p[(long)Ws * 3 + 3 + c] : 0;
        res[c] = (t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + (1 << 14)) >> 15;
    }
}

// A thread's block of a crop, read from its frame: v[row][pixel][channel] = the pixels (xb .. xb + 3, yb .. yb + ROWS - 1) of the crop under A, a
// pixel whose four taps all lie outside the frame the border value 0.  crop_batch_kernel (imgops.hip) and crop_lmk_kernel (landmarks.hip) both
// read through here and store through crop_store.
template <int ROWS>
__device__ __forceinline__ void crop_read(const unsigned char* __restrict__ frame, int Ho, int Wo, const AffineInv& A, int xb, int yb,
                                          int (&v)[ROWS][4][3])
{
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Tap t = tap_at(A, xb + k, yb + r, Ho, Wo);
            int res[3] = {0, 0, 0};      // a pixel of its own, copied into v: written into v[r][k] in place, two rows take 220 and more VGPRs
            if (!t.outside) tap_u8x3(frame, Wo, t, res);
            v[r][k][0] = res[0]; v[r][k][1] = res[1]; v[r][k][2] = res[2];
        }
}

// A thread's block of crop n - four pixels of a row, of two rows with STAGE != 0 - from its registers (v[row][pixel][channel], 8-bit values): the
// crop's bytes (12 per row = three dwords) and, with STAGE != 0, what prepare_crops_kernel would make of them, so that the crop is not read back:
// STAGE 2 (dsize 512): the two 2 x 2 means (a + b + c + d + 2) >> 2, / 255, one float2 per channel of the NCHW fp32 input; STAGE 1 (dsize 256):
// / 255 only, one float4 per row and channel.  WIDE = false: the same values byte by byte and float by float, for buffers off their boundaries
// (crops: 4 bytes, I: 16).  crop_batch_kernel (imgops.hip) and crop_lmk_kernel (landmarks.hip) both store through here.
template <int STAGE, bool WIDE>
__device__ __forceinline__ void crop_store(const int (&v)[STAGE ? 2 : 1][4][3], long n, int yb, int xb, int dsize, unsigned char* __restrict__ crops,
                                           float* __restrict__ I)
{
    constexpr int ROWS = STAGE ? 2 : 1;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        unsigned char* d = crops + ((n * dsize + yb + r) * dsize + xb) * 3;
        if constexpr (WIDE) {
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 2] |= (unsigned)v[r][j / 3][j % 3] << ((j & 3) * 8);
            unsigned* out = (unsigned*)d;
            out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) d[j] = (unsigned char)v[r][j / 3][j % 3];
        }
    }
    if constexpr (STAGE == 2) {
        const int Wd = dsize >> 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int a = (v[0][0][c] + v[0][1][c] + v[1][0][c] + v[1][1][c] + 2) >> 2;
            const int b = (v[0][2][c] + v[0][3][c] + v[1][2][c] + v[1][3][c] + 2) >> 2;
            float* d = I + ((n * 3 + c) * Wd + (yb >> 1)) * Wd + (xb >> 1);
            if constexpr (WIDE) *(float2*)d = make_float2(staged_value(a), staged_value(b));
            else { d[0] = staged_value(a); d[1] = staged_value(b); }
        }
    } else if constexpr (STAGE == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float* d = I + ((n * 3 + c) * dsize + yb + r) * dsize + xb;
                const float4 q = make_float4(staged_value(v[r][0][c]), staged_value(v[r][1][c]), staged_value(v[r][2][c]), staged_value(v[r][3][c]));
                if constexpr (WIDE) *(float4*)d = q;
                else { d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; }
            }
    }
}
