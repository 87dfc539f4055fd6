// The integer arithmetic of the two 4:2:0 conversions (yuv.hip; include/canonswap_yuv.h), stated once for the host and the device: the host
// builds the coefficients (yuv_coef), the kernels take them as an argument and apply them per pixel and per 2 x 2 block (yuv_decode_px, yuv_encode_luma,
// yuv_encode_chroma).  tests/yuv_ref.py restates all of it in numpy and is the definition; tests/yuv_host/yuv_host.cpp compiles this header for
// the host, so that the CPU suite holds these very lines to the restatement bit for bit.
//
// Real coefficients (BT.601: Kr 0.299, Kb 0.114; BT.709: Kr 0.2126, Kb 0.0722; Kg = 1 - Kr - Kb), in float64:
//     decode   R = sy (Y - y0) + 2 (1 - Kr) sc (V - 128)
//              G = sy (Y - y0) - 2 Kb (1 - Kb) / Kg sc (U - 128) - 2 Kr (1 - Kr) / Kg sc (V - 128)
//              B = sy (Y - y0) + 2 (1 - Kb) sc (U - 128)
//     encode   Y = y0 + (Kr R + Kg G + Kb B) / sy
//              U = 128 + (-Kr R - Kg G + (1 - Kb) B) / (2 (1 - Kb) sc),   V = 128 + ((1 - Kr) R - Kg G - Kb B) / (2 (1 - Kr) sc)
// limited range: sy = 255 / 219, sc = 255 / 224, y0 = 16; full range: sy = sc = 1, y0 = 0.  Each is rounded to nearest (floor(x + 0.5) of the
// magnitude) at 14 fractional bits for decode and 16 for encode; the largest coefficient of U (blue) and of V (red) is then set to minus the sum
// of the other two, so that each chroma triple sums to exactly zero and a grey encodes to U = V = 128 whatever its level.  The chroma
// coefficients are applied to the sums of R, G and B over the block's four pixels: a shift of 18.  Every result is (sum + half) >> shift with
// an arithmetic shift, clamped to 0 .. 255; every intermediate fits an int32 (the largest is below 2^27).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YUV_HD __host__ __device__ __forceinline__
#else
#define YUV_HD inline
#endif

#define YUV_DEC_BITS 14
#define YUV_ENC_BITS 16

struct YuvCoef {
    int y0;
    int cy, crv, cgu, cgv, cbu;                        // decode, 14 fractional bits; cgu and cgv are subtracted
    int ry, gy, by, ur, ug, ub, vr, vg, vb;            // encode, 16 fractional bits; ur + ug + ub = vr + vg + vb = 0
};

#pragma clang fp contract(off)
// matrix 0: BT.601, 1: BT.709; full_range 0 or 1 (checked by the caller).  Every product and quotient below is one rounded float64
// operation in the order written, which is the order of tests/yuv_ref.py coef().
inline YuvCoef yuv_coef(int matrix, int full_range)
{
    const double Kr = matrix ? 0.2126 : 0.299, Kb = matrix ? 0.0722 : 0.114;
    const double Kg = (1.0 - Kr) - Kb;
    const double sy = full_range ? 1.0 : 255.0 / 219.0, sc = full_range ? 1.0 : 255.0 / 224.0;
    const double d = (double)(1 << YUV_DEC_BITS), n = (double)(1 << YUV_ENC_BITS);
    auto rnd = [](double x) { return (int)__builtin_floor(x + 0.5); };
    YuvCoef c;
    c.y0 = full_range ? 0 : 16;
    c.cy = rnd(sy * d);
    c.crv = rnd(((2.0 * (1.0 - Kr)) * sc) * d);
    c.cbu = rnd(((2.0 * (1.0 - Kb)) * sc) * d);
    c.cgu = rnd((((2.0 * Kb) * (1.0 - Kb) / Kg) * sc) * d);
    c.cgv = rnd((((2.0 * Kr) * (1.0 - Kr) / Kg) * sc) * d);
    c.ry = rnd((Kr / sy) * n);
    c.gy = rnd((Kg / sy) * n);
    c.by = rnd((Kb / sy) * n);
    const double du = (2.0 * (1.0 - Kb)) * sc, dv = (2.0 * (1.0 - Kr)) * sc;
    c.ur = -rnd((Kr / du) * n);
    c.ug = -rnd((Kg / du) * n);
    c.ub = -(c.ur + c.ug);
    c.vg = -rnd((Kg / dv) * n);
    c.vb = -rnd((Kb / dv) * n);
    c.vr = -(c.vg + c.vb);
    return c;
}

// (sum >> bits) clamped to 0 .. 255, written as a clamp of the sum followed by the shift: the same value for every int32, in a form that the
// gfx950 back end does not fold into its packed shift-and-saturate instruction (v_ashr_pk_u8_i32), whose result the compiler (ROCm 7.2) ORs into a
// word as if its upper half were zero; on an MI355X bytes 2 and 3 of such chroma words came out with further bits set.
YUV_HD int yuv_shift_clamp8(int sum, int bits)
{
    const int top = (256 << bits) - 1;
    sum = sum < 0 ? 0 : sum > top ? top : sum;
    return sum >> bits;
}

// one pixel: its luma and its block's chroma -> R, G, B
YUV_HD void yuv_decode_px(const YuvCoef& c, int Y, int U, int V, int& R, int& G, int& B)
{
    const int half = 1 << (YUV_DEC_BITS - 1);
    const int l = c.cy * (Y - c.y0) + half, u = U - 128, v = V - 128;
    R = yuv_shift_clamp8(l + c.crv * v, YUV_DEC_BITS);
    G = yuv_shift_clamp8(l - c.cgu * u - c.cgv * v, YUV_DEC_BITS);
    B = yuv_shift_clamp8(l + c.cbu * u, YUV_DEC_BITS);
}

YUV_HD int yuv_encode_luma(const YuvCoef& c, int R, int G, int B)
{
    return yuv_shift_clamp8(c.ry * R + c.gy * G + c.by * B + (c.y0 << YUV_ENC_BITS) + (1 << (YUV_ENC_BITS - 1)), YUV_ENC_BITS);
}

// the block's chroma from the sums of R, G and B over its four pixels
YUV_HD void yuv_encode_chroma(const YuvCoef& c, int sR, int sG, int sB, int& U, int& V)
{
    const int bias = (128 << (YUV_ENC_BITS + 2)) + (1 << (YUV_ENC_BITS + 1));
    U = yuv_shift_clamp8(c.ur * sR + c.ug * sG + c.ub * sB + bias, YUV_ENC_BITS + 2);
    V = yuv_shift_clamp8(c.vr * sR + c.vg * sG + c.vb * sB + bias, YUV_ENC_BITS + 2);
}
