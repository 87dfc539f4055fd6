// 4:2:0 frames <-> the engine's RGB frames, on the device (include/canonswap_yuv.h): what stands between a codec, which speaks NV12 or I420,
// and the chain, which crops from and pastes into (F, Ho, Wo, 3) uint8.  cs_yuv_to_rgb replicates a block's chroma to its 2 x 2 pixels;
// cs_rgb_to_yuv is the inverse, and with keep = 1 leaves every block whose four RGB pixels still are what its six bytes decode to as it was,
// which makes the part of a frame that nothing wrote lossless.  The arithmetic is integer and stands in yuv_math.h (restated by
// tests/yuv_ref.py, which defines it); this file is the data movement.
//
// Both kernels are pure bandwidth: per 64 frames of 1080 x 1920 the decode reads 199 MB and writes 398 MB, the encode reads 398 MB (and, with
// keep, 199 MB) and writes 199 MB.  A thread owns a tile of 16 x 2 pixels = 8 blocks: two 16-byte runs of Y, 16 bytes of chroma (NV12: one
// interleaved run; I420: 8 of U and 8 of V) and two 48-byte runs of RGB, so that the threads of a wave walk along a row pair and every run of
// a wave is contiguous with its neighbours'.  The fast path moves each run as 8-byte words (as paste_faces_kernel and concat_frames_kernel
// move theirs as dwords); the launcher states when it holds (yuv_frame below).  A thread whose tile is cut by the right edge, and every
// thread of a launch off the fast path, makes element accesses of the same values: a fallback, not an error.  No LDS, no scratch: the tile
// lives in 32 + 12 words of registers, all indices are compile-time after unrolling.
//
// With keep the encode reads the six bytes of a block and writes them back unchanged or re-encoded: one thread owns them, so reading and writing
// the same buffer in one launch needs no ordering.
#include "common.h"
#include "../../include/canonswap_yuv.h"
#include "yuv_math.h"

#define LAUNCH_CHECK(name)                                                                       \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) { cs_set_error(name " launch: %s", hipGetErrorString(_e)); return -1; } \
    } while (0)

extern "C" int cs_yuv_abi_version(void) { return CS_YUV_ABI_VERSION; }

struct YuvFrame {
    YuvCoef c;
    int Ho, Wo, wide;
};

__device__ __forceinline__ int yuv_byte(const unsigned* w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// N bytes at p -> N / 4 words: 8-byte loads (p is 8-byte aligned and all N bytes exist), or the first `valid` bytes one by one, the rest zero
template <int N> __device__ __forceinline__ void yuv_load(const unsigned char* p, bool wide, int valid, unsigned* w)
{
    if (wide) {
#pragma unroll
        for (int k = 0; k < N / 8; ++k) {
            const uint2 q = ((const uint2*)p)[k];
            w[2 * k] = q.x; w[2 * k + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) w[k] = 0u;
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < valid) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    }
}

template <int N> __device__ __forceinline__ void yuv_store(unsigned char* p, bool wide, int valid, const unsigned* w)
{
    if (wide) {
#pragma unroll
        for (int k = 0; k < N / 8; ++k) ((uint2*)p)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < valid) p[k] = (unsigned char)yuv_byte(w, k);
    }
}

// Where the tile of thread t of a frame lies: row pair r, first column x0, npx of its 16 columns inside the frame (even, at least 2).
struct YuvTile {
    int r, x0, npx;
    bool wide;
    long y_off, c_off, v_off, rgb_off;      // byte offsets in a frame: row 2 r of Y; the chroma run (NV12: interleaved; I420: U, and V at v_off); row 2 r of RGB
};

template <bool NV12> __device__ __forceinline__ bool yuv_tile(const YuvFrame& p, YuvTile& t)
{
    const int T = (p.Wo + 15) >> 4;                                      // tiles per row pair
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * (p.Ho >> 1)) return false;
    t.r = (int)(i / T);
    t.x0 = (int)(i % T) * 16;
    t.npx = min(16, p.Wo - t.x0);
    t.wide = p.wide && t.npx == 16;
    const long luma = (long)p.Ho * p.Wo;
    t.y_off = (long)(2 * t.r) * p.Wo + t.x0;
    if (NV12) {
        t.c_off = luma + (long)t.r * p.Wo + t.x0;
        t.v_off = 0;
    } else {
        t.c_off = luma + (long)t.r * (p.Wo >> 1) + (t.x0 >> 1);
        t.v_off = t.c_off + (luma >> 2);
    }
    t.rgb_off = ((long)(2 * t.r) * p.Wo + t.x0) * 3;
    return true;
}

// the tile's YUV bytes: y[row][4 words]; c[4 words]: NV12 the interleaved run, I420 U in words 0-1 and V in words 2-3
template <bool NV12> __device__ __forceinline__ void yuv_load_tile(const unsigned char* f, const YuvFrame& p, const YuvTile& t, unsigned (&y)[2][4],
                                                                    unsigned (&c)[4])
{
    yuv_load<16>(f + t.y_off, t.wide, t.npx, y[0]);
    yuv_load<16>(f + t.y_off + p.Wo, t.wide, t.npx, y[1]);
    if (NV12) {
        yuv_load<16>(f + t.c_off, t.wide, t.npx, c);
    } else {
        yuv_load<8>(f + t.c_off, t.wide, t.npx >> 1, c);
        yuv_load<8>(f + t.v_off, t.wide, t.npx >> 1, c + 2);
    }
}

template <bool NV12> __device__ __forceinline__ void yuv_store_tile(unsigned char* f, const YuvFrame& p, const YuvTile& t, const unsigned (&y)[2][4],
                                                                     const unsigned (&c)[4])
{
    yuv_store<16>(f + t.y_off, t.wide, t.npx, y[0]);
    yuv_store<16>(f + t.y_off + p.Wo, t.wide, t.npx, y[1]);
    if (NV12) {
        yuv_store<16>(f + t.c_off, t.wide, t.npx, c);
    } else {
        yuv_store<8>(f + t.c_off, t.wide, t.npx >> 1, c);
        yuv_store<8>(f + t.v_off, t.wide, t.npx >> 1, c + 2);
    }
}

template <bool NV12> __device__ __forceinline__ int yuv_u_of(const unsigned (&c)[4], int j) { return yuv_byte(c, NV12 ? 2 * j : j); }
template <bool NV12> __device__ __forceinline__ int yuv_v_of(const unsigned (&c)[4], int j) { return yuv_byte(c, NV12 ? 2 * j + 1 : 8 + j); }

// ---------------------------------------------------------------------------------------------- YUV 4:2:0 -> RGB
template <bool NV12>
__global__ void __launch_bounds__(256) yuv_to_rgb_kernel(const unsigned char* __restrict__ yuv, YuvFrame p, unsigned char* __restrict__ rgb)
{
    YuvTile t;
    if (!yuv_tile<NV12>(p, t)) return;
    const long px = (long)p.Ho * p.Wo;
    const unsigned char* f = yuv + (long)blockIdx.y * (px + (px >> 1));
    unsigned y[2][4], c[4], o[2][12];
    yuv_load_tile<NV12>(f, p, t, y, c);
#pragma unroll
    for (int k = 0; k < 12; ++k) o[0][k] = o[1][k] = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int U = yuv_u_of<NV12>(c, j), V = yuv_v_of<NV12>(c, j);
#pragma unroll
        for (int row = 0; row < 2; ++row)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int k = 2 * j + dx;
                int v[3];
                yuv_decode_px(p.c, yuv_byte(y[row], k), U, V, v[0], v[1], v[2]);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) o[row][(3 * k + ch) >> 2] |= (unsigned)v[ch] << (8 * ((3 * k + ch) & 3));
            }
    }
    unsigned char* d = rgb + (long)blockIdx.y * px * 3 + t.rgb_off;
    yuv_store<48>(d, t.wide, 3 * t.npx, o[0]);
    yuv_store<48>(d + (long)p.Wo * 3, t.wide, 3 * t.npx, o[1]);
}

// ---------------------------------------------------------------------------------------------- RGB -> YUV 4:2:0
// KEEP: the block's six bytes are read first; where its four RGB pixels are what they decode to, they are written back as they are.
template <bool NV12, bool KEEP>
__global__ void __launch_bounds__(256) rgb_to_yuv_kernel(const unsigned char* __restrict__ rgb, YuvFrame p, unsigned char* yuv)
{
    YuvTile t;
    if (!yuv_tile<NV12>(p, t)) return;
    const long px = (long)p.Ho * p.Wo;
    unsigned char* f = yuv + (long)blockIdx.y * (px + (px >> 1));
    const unsigned char* s = rgb + (long)blockIdx.y * px * 3 + t.rgb_off;
    unsigned in[2][12], y[2][4], c[4], ny[2][4], nc[4];
    yuv_load<48>(s, t.wide, 3 * t.npx, in[0]);
    yuv_load<48>(s + (long)p.Wo * 3, t.wide, 3 * t.npx, in[1]);
    if (KEEP) yuv_load_tile<NV12>(f, p, t, y, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) ny[0][k] = ny[1][k] = nc[k] = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int Y[2][2], U, V, sum[3] = {0, 0, 0};
        bool kept = KEEP;
        const int U0 = KEEP ? yuv_u_of<NV12>(c, j) : 0, V0 = KEEP ? yuv_v_of<NV12>(c, j) : 0;
#pragma unroll
        for (int row = 0; row < 2; ++row)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int k = 2 * j + dx;
                const int R = yuv_byte(in[row], 3 * k), G = yuv_byte(in[row], 3 * k + 1), B = yuv_byte(in[row], 3 * k + 2);
                sum[0] += R; sum[1] += G; sum[2] += B;
                Y[row][dx] = yuv_encode_luma(p.c, R, G, B);
                if (KEEP) {
                    int r0, g0, b0;
                    yuv_decode_px(p.c, yuv_byte(y[row], k), U0, V0, r0, g0, b0);
                    kept = kept && r0 == R && g0 == G && b0 == B;
                }
            }
        yuv_encode_chroma(p.c, sum[0], sum[1], sum[2], U, V);
        if (kept) {
            U = U0; V = V0;
#pragma unroll
            for (int row = 0; row < 2; ++row)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) Y[row][dx] = yuv_byte(y[row], 2 * j + dx);
        }
#pragma unroll
        for (int row = 0; row < 2; ++row)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) ny[row][(2 * j + dx) >> 2] |= (unsigned)Y[row][dx] << (8 * ((2 * j + dx) & 3));
        const int ku = NV12 ? 2 * j : j, kv = NV12 ? 2 * j + 1 : 8 + j;
        nc[ku >> 2] |= (unsigned)U << (8 * (ku & 3));
        nc[kv >> 2] |= (unsigned)V << (8 * (kv & 3));
    }
    yuv_store_tile<NV12>(f, p, t, ny, nc);
}

// Everything is checked by the caller (cs_yuv_to_rgb, cs_rgb_to_yuv): Ho, Wo even in [2, 16384], F >= 1, no NULL, no overlap.  Frames are grid
// rows, 65535 per launch; every offset is 64-bit.
//
// The fast path: both buffers 8-byte aligned and Wo a multiple of 8 (NV12) or of 16 (I420, whose chroma rows are Wo / 2 long).  Then every
// row of Y, of chroma and of RGB, every plane and every frame (3 Ho Wo / 2 bytes, Ho even) starts on an 8-byte boundary, and so does every
// run of a tile.  Within such a launch the tile cut by the right edge (Wo not a multiple of 16) still takes the element path.
static YuvFrame yuv_frame(int Ho, int Wo, int layout, int matrix, int full_range, const void* yuv, const void* rgb)
{
    YuvFrame p;
    p.c = yuv_coef(matrix, full_range);
    p.Ho = Ho; p.Wo = Wo;
    p.wide = (((uintptr_t)yuv | (uintptr_t)rgb) & 7) == 0 && Wo % (layout == 0 ? 8 : 16) == 0;
    return p;
}

int launch_yuv_to_rgb(const unsigned char* yuv, int F, int Ho, int Wo, int layout, int matrix, int full_range, unsigned char* rgb, hipStream_t st)
{
    const YuvFrame p = yuv_frame(Ho, Wo, layout, matrix, full_range, yuv, rgb);
    const long px = (long)Ho * Wo, tiles = (long)((Wo + 15) >> 4) * (Ho >> 1);
    for (int f0 = 0; f0 < F; f0 += 65535) {
        const dim3 grid((unsigned)((tiles + 255) / 256), (unsigned)(F - f0 < 65535 ? F - f0 : 65535)), block(256);
        const unsigned char* s = yuv + (long)f0 * (px + (px >> 1));
        unsigned char* d = rgb + (long)f0 * px * 3;
        if (layout == 0) hipLaunchKernelGGL(yuv_to_rgb_kernel<true>, grid, block, 0, st, s, p, d);
        else hipLaunchKernelGGL(yuv_to_rgb_kernel<false>, grid, block, 0, st, s, p, d);
        LAUNCH_CHECK("yuv_to_rgb");
    }
    return 0;
}

int launch_rgb_to_yuv(const unsigned char* rgb, int F, int Ho, int Wo, int layout, int matrix, int full_range, int keep, unsigned char* yuv,
                      hipStream_t st)
{
    const YuvFrame p = yuv_frame(Ho, Wo, layout, matrix, full_range, yuv, rgb);
    const long px = (long)Ho * Wo, tiles = (long)((Wo + 15) >> 4) * (Ho >> 1);
    for (int f0 = 0; f0 < F; f0 += 65535) {
        const dim3 grid((unsigned)((tiles + 255) / 256), (unsigned)(F - f0 < 65535 ? F - f0 : 65535)), block(256);
        const unsigned char* s = rgb + (long)f0 * px * 3;
        unsigned char* d = yuv + (long)f0 * (px + (px >> 1));
        if (layout == 0 && keep) hipLaunchKernelGGL((rgb_to_yuv_kernel<true, true>), grid, block, 0, st, s, p, d);
        else if (layout == 0) hipLaunchKernelGGL((rgb_to_yuv_kernel<true, false>), grid, block, 0, st, s, p, d);
        else if (keep) hipLaunchKernelGGL((rgb_to_yuv_kernel<false, true>), grid, block, 0, st, s, p, d);
        else hipLaunchKernelGGL((rgb_to_yuv_kernel<false, false>), grid, block, 0, st, s, p, d);
        LAUNCH_CHECK("rgb_to_yuv");
    }
    return 0;
}
