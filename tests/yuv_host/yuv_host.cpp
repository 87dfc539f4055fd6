// canonswap_amd/csrc/yuv_math.h compiled for the host: the coefficient builder and the per-pixel / per-block arithmetic the kernels of yuv.hip
// run.  tests/test_yuv_cpu.py builds this into a shared object (no fp contraction) and holds it to tests/yuv_ref.py through ctypes.
#include "yuv_math.h"

extern "C" void yuv_host_coef(int matrix, int full_range, int* out16)
{
    const YuvCoef c = yuv_coef(matrix, full_range);
    const int v[16] = {c.y0, c.cy, c.crv, c.cgu, c.cgv, c.cbu, c.ry, c.gy, c.by, c.ur, c.ug, c.ub, c.vr, c.vg, c.vb, 0};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
}

// n triples: yuv (n x 3) -> rgb (n x 3)
extern "C" void yuv_host_decode(int matrix, int full_range, long n, const unsigned char* yuv, unsigned char* rgb)
{
    const YuvCoef c = yuv_coef(matrix, full_range);
    for (long i = 0; i < n; ++i) {
        int R, G, B;
        yuv_decode_px(c, yuv[3 * i], yuv[3 * i + 1], yuv[3 * i + 2], R, G, B);
        rgb[3 * i] = (unsigned char)R; rgb[3 * i + 1] = (unsigned char)G; rgb[3 * i + 2] = (unsigned char)B;
    }
}

// n blocks: rgb (n x 4 x 3) -> out (n x 6): the four lumas, U, V
extern "C" void yuv_host_encode(int matrix, int full_range, long n, const unsigned char* rgb, unsigned char* out)
{
    const YuvCoef c = yuv_coef(matrix, full_range);
    for (long i = 0; i < n; ++i) {
        int s[3] = {0, 0, 0}, U, V;
        for (int k = 0; k < 4; ++k) {
            const unsigned char* p = rgb + (i * 4 + k) * 3;
            s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
            out[6 * i + k] = (unsigned char)yuv_encode_luma(c, p[0], p[1], p[2]);
        }
        yuv_encode_chroma(c, s[0], s[1], s[2], U, V);
        out[6 * i + 4] = (unsigned char)U; out[6 * i + 5] = (unsigned char)V;
    }
}
