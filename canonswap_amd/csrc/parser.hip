// The SegFormer face parser (a MiT encoder with an all-MLP decode head) on gfx950: pixel_values -> logits at a quarter of the
// input extent, the tensor cs_face_masks takes.  Tokens are contiguous channels-last [B][H_s][W_s][C_s] tensors at their real extents, the
// residual stream is fp32, every matmul operand is fp16 and accumulates in fp32.  As in identity.hip there are no float atomics and every sum has
// one fixed order: a sample's bits do not depend on the batch it is part of.  The patch-embedding and sequence-reduction convolutions go
// through identity.hip's direct convolution (launch_id_conv); everything else is here.
#include "common.h"

namespace {

constexpr int P_CIN0 = 32;      // the first patch embedding reads 3 real + 29 zero channels (one 32-deep K-step per tap)

// ---- input: pixel_values fp32 NCHW [B][3][H][W] -> fp16 [B][H][W][32]
__global__ void p_input_kernel(const float* __restrict__ pv, half_t* __restrict__ out, long total, long HW)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / HW, p = i - n * HW;
    h8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 3; ++c) v[c] = (half_t)pv[(n * 3 + c) * HW + p];
    h8_t* o = (h8_t*)(out + i * P_CIN0);
    const h8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
    o[0] = v; o[1] = z; o[2] = z; o[3] = z;
}

// ---- token GEMM: out[M][N] = a[M][K] w[N][K]^T (+ bias), a and w fp16, K % 32 == 0, N % BN == 0, any M (rows past M are loaded as zero and
// not stored).  One workgroup = 128 rows x BN columns; its four waves sit 2 x 2, each owns 64 rows x BN / 2 columns as 4 x BN / 32 fragments of
// v_mfma_f32_16x16x32_f16 (lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k][col l & 15], 16 bytes each; result register r of lane l is
// row 4 (l >> 4) + r, column l & 15).  A 32-deep K-step of both operands is staged in LDS, double-buffered: the next step's global loads are
// in flight while this step's MFMAs run.  A fragment read is 64 lanes x 16 bytes over one contiguous KB of LDS: no bank conflicts, no padding.
// One wave adds the whole K range of its outputs in K order.
template <int BN>
__global__ void __launch_bounds__(256) p_gemm_kernel(PGemmCall g)
{
    constexpr int NJ = BN / 32, NB = BN / 64;
    __shared__ __attribute__((aligned(16))) half_t sA[2][128 * 32];
    __shared__ __attribute__((aligned(16))) half_t sB[2][BN * 32];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int wm = wv & 1, wn = wv >> 1;
    const int m0 = blockIdx.x * 128, n0 = blockIdx.y * BN;
    const int lrow = tid >> 2, lch = (tid & 3) * 8;
    h8_t ra[2], rb[NB];
#define P_GLOAD(k0)                                                                                              \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                              \
        const int gm = m0 + lrow + 64 * i;                                                                       \
        ra[i] = h8_t{0, 0, 0, 0, 0, 0, 0, 0};                                                                    \
        if (gm < g.M) ra[i] = *(const h8_t*)(g.a + (long)gm * g.K + (k0) + lch);                                 \
    }                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) rb[i] = *(const h8_t*)(g.w + (long)(n0 + lrow + 64 * i) * g.K + (k0) + lch);
#define P_SSTORE(buf)                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) *(h8_t*)&sA[buf][(lrow + 64 * i) * 32 + lch] = ra[i];          \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) *(h8_t*)&sB[buf][(lrow + 64 * i) * 32 + lch] = rb[i];
    f4_t acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};
    const int nk = g.K >> 5;
    P_GLOAD(0)
    P_SSTORE(0)
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk) { P_GLOAD((ks + 1) * 32) }
        h8_t af[4], bf[NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = *(const h8_t*)&sA[buf][(wm * 64 + i * 16 + lr) * 32 + lk * 8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[j] = *(const h8_t*)&sB[buf][(wn * (BN / 2) + j * 16 + lr) * 32 + lk * 8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        if (ks + 1 < nk) { P_SSTORE(buf ^ 1) }      // the other buffer: its last readers passed the barrier that ended the previous step
        __syncthreads();
    }
#undef P_GLOAD
#undef P_SSTORE
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = n0 + wn * (BN / 2) + j * 16 + lr;
        const float bias = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + lk * 4 + r;
                if (row >= g.M) continue;
                const float v = acc[i][j][r] + bias;
                const long o = (long)row * g.N + col;
                if (g.mode == P_GEMM_F16) ((half_t*)g.out)[o] = (half_t)v;
                else if (g.mode == P_GEMM_RES) ((float*)g.out)[o] += v;          // the fp32 residual stream, in place
                else if (g.mode == P_GEMM_F32) ((float*)g.out)[o] = v;
                else if (col < g.L) ((float*)g.out)[((long)(row / g.P) * g.L + col) * g.P + row % g.P] = v;      // P_GEMM_NCHW: the real classes only
            }
    }
}

// ---- LayerNorm over the channels of one token, one wave per token: fp32 in -> fp32 and / or fp16 out.  Two passes in fp32 (mean, then the
// variance of the centred values, biased as nn.LayerNorm's), each a per-lane sum in channel order followed by a butterfly over the 64 lanes.
__global__ void __launch_bounds__(256) p_ln_kernel(const float* __restrict__ in, const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                   long M, int C, float* __restrict__ out32, half_t* __restrict__ out16)
{
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= M) return;
    const int n = C >> 6;          // C % 64 == 0, C <= 512
    const float* x = in + t * C;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = j < n ? x[lane + 64 * j] : 0.f; s += v[j]; }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = j < n ? v[j] - mean : 0.f; q = fmaf(d, d, q); }
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float rstd = 1.f / sqrtf(q / (float)C + eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j >= n) continue;
        const int c = lane + 64 * j;
        const float y = fmaf((v[j] - mean) * rstd, g[c], b[c]);
        if (out32) out32[t * C + c] = y;
        if (out16) out16[t * C + c] = (half_t)y;
    }
}

// ---- attention: one workgroup per (sample, head, tile of 64 queries); wave w owns queries 16 w .. 16 w + 15.  q [B][Nq][C] (the d^-1/2 scale is
// folded into q_proj), kv [B][Nk][2 C] (keys in the first C columns, values in the last), head h = channels h D .. h D + D - 1; ctx [B][Nq][C].
// The head's keys [Nkp][D] and values, transposed to [D][Nkp], live in LDS (Nkp = Nk rounded up to 32, the padding zero; rows are 8 halves
// longer than their content so that 16 rows do not share a bank).  S = q k^T on MFMA with the keys as the B operand; keys past Nk get -inf
// before the row maximum; softmax in fp32, normalised, then rounded to fp16 into the wave's rows of sP; ctx = P v on MFMA with P as the A
// operand and the transposed values as B.  Nk <= 256: the 16 score fragments of a wave stay in registers.
template <int D>
__global__ void __launch_bounds__(256) p_attn_kernel(const half_t* __restrict__ q, const half_t* __restrict__ kv, half_t* __restrict__ ctx,
                                                     int Nq, int Nk, int heads)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int C = heads * D, Nkp = (Nk + 31) & ~31, KS = D + 8, VS = Nkp + 8;
    half_t* sK = (half_t*)smem;          // [Nkp][KS]
    half_t* sV = sK + Nkp * KS;          // [D][VS]
    half_t* sP = sV + D * VS;            // [64][VS]
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64;
    for (int p = tid; p < Nkp * (D / 8); p += 256) {
        const int key = p / (D / 8), c8 = (p % (D / 8)) * 8;
        h8_t kk = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (key < Nk) {
            const half_t* src = kv + ((long)b * Nk + key) * 2 * C + h * D + c8;
            kk = *(const h8_t*)src;
            vv = *(const h8_t*)(src + C);
        }
        *(h8_t*)(sK + key * KS + c8) = kk;
        for (int j = 0; j < 8; ++j) sV[(c8 + j) * VS + key] = vv[j];
    }
    __syncthreads();
    const int qrow = q0 + wv * 16 + lr;
    h8_t qf[D / 32];
    for (int c = 0; c < D / 32; ++c) {
        qf[c] = h8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (qrow < Nq) qf[c] = *(const h8_t*)(q + ((long)b * Nq + qrow) * C + h * D + c * 32 + lk * 8);
    }
    const int nt = Nkp >> 4;
    f4_t s[16];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        s[t] = f4_t{0.f, 0.f, 0.f, 0.f};
        if (t < nt) {
            for (int c = 0; c < D / 32; ++c)
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[c], *(const h8_t*)(sK + (t * 16 + lr) * KS + c * 32 + lk * 8), s[t], 0, 0, 0);
            if (t * 16 + lr >= Nk) s[t] = f4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], s[t][r]);
        }
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 4; ++r)
        for (int off = 8; off > 0; off >>= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off));      // the 16 lanes of a row
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (t < nt)
            for (int r = 0; r < 4; ++r) { s[t][r] = expf(s[t][r] - mx[r]); sum[r] += s[t][r]; }
    for (int r = 0; r < 4; ++r) {
        for (int off = 8; off > 0; off >>= 1) sum[r] += __shfl_xor(sum[r], off);
        sum[r] = 1.f / sum[r];
    }
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (t < nt)
            for (int r = 0; r < 4; ++r) sP[(wv * 16 + lk * 4 + r) * VS + t * 16 + lr] = (half_t)(s[t][r] * sum[r]);
    __syncthreads();
    f4_t o[D / 16];
    for (int n = 0; n < D / 16; ++n) o[n] = f4_t{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < (Nkp >> 5); ++kc) {
        const h8_t pf = *(const h8_t*)(sP + (wv * 16 + lr) * VS + kc * 32 + lk * 8);
        for (int n = 0; n < D / 16; ++n)
            o[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, *(const h8_t*)(sV + (n * 16 + lr) * VS + kc * 32 + lk * 8), o[n], 0, 0, 0);
    }
    for (int n = 0; n < D / 16; ++n)
        for (int r = 0; r < 4; ++r) {
            const int row = q0 + wv * 16 + lk * 4 + r;
            if (row < Nq) ctx[((long)b * Nq + row) * C + h * D + n * 16 + lr] = (half_t)o[n][r];
        }
}

// ---- Mix-FFN middle: GELU(depth-wise 3 x 3 conv + bias), zero padding 1, fp16 [B][H][W][C] -> fp16; w fp32 [9][C] tap-major.  One thread = one
// position x 8 channels; taps are added in (ky, kx) order in fp32.  GELU is the erf form.
__global__ void p_dwgelu_kernel(const half_t* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, half_t* __restrict__ out,
                                int B, int H, int W, int C)
{
    const int C8 = C >> 3;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * H * W * C8) return;
    const int c = (int)(i % C8) * 8;
    const long p = i / C8;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long n = p / ((long)W * H);
    float acc[8];
    for (int k = 0; k < 8; ++k) acc[k] = bias[c + k];
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x + kx - 1;
            if (ix < 0 || ix >= W) continue;
            const h8_t v = *(const h8_t*)(in + ((n * H + iy) * W + ix) * C + c);
            const float* wt = w + (ky * 3 + kx) * C + c;
            for (int k = 0; k < 8; ++k) acc[k] = fmaf((float)v[k], wt[k], acc[k]);
        }
    }
    h8_t o;
    for (int k = 0; k < 8; ++k) o[k] = (half_t)(0.5f * acc[k] * (1.f + erff(acc[k] * 0.70710678118654752f)));
    *(h8_t*)(out + p * C + c) = o;
}

// ---- decode head: out = fp16(relu(p0 + up2(p1) + up4(p2) + up8(p3))), up = bilinear, align_corners = False; p_s fp32 [B][H >> s][W >> s][D]
// (the composed per-stage projections; every bias is already in p0).  A tap pair along one axis for output o at ratio R:
// src = max((o + 0.5) / R - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), weight of i1 = src - i0 (ATen's arithmetic in fp32).
__device__ __forceinline__ void p_tap(int o, float inv, int n, int& i0, int& i1, float& f)
{
    const float src = fmaxf(((float)o + 0.5f) * inv - 0.5f, 0.f);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    f = src - (float)i0;
}

__global__ void p_upadd_kernel(const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ p2, const float* __restrict__ p3,
                               half_t* __restrict__ out, int B, int H, int W, int D)
{
    const int D4 = D >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * H * W * D4) return;
    const int c = (int)(i % D4) * 4;
    const long p = i / D4;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long n = p / ((long)W * H);
    f4_t v = *(const f4_t*)(p0 + p * D + c);
    const float* ps[3] = {p1, p2, p3};
    for (int s = 0; s < 3; ++s) {
        const int hs = H >> (s + 1), ws = W >> (s + 1);
        const float inv = 1.f / (float)(2 << s);
        int y0, y1, x0, x1; float fy, fx;
        p_tap(y, inv, hs, y0, y1, fy);
        p_tap(x, inv, ws, x0, x1, fx);
        const float* base = ps[s] + n * hs * ws * D + c;
        const f4_t a = *(const f4_t*)(base + ((long)y0 * ws + x0) * D), bq = *(const f4_t*)(base + ((long)y0 * ws + x1) * D);
        const f4_t cq = *(const f4_t*)(base + ((long)y1 * ws + x0) * D), d = *(const f4_t*)(base + ((long)y1 * ws + x1) * D);
        for (int k = 0; k < 4; ++k) {
            const float top = a[k] + fx * (bq[k] - a[k]), bot = cq[k] + fx * (d[k] - cq[k]);
            v[k] += top + fy * (bot - top);
        }
    }
    h4_t o;
    for (int k = 0; k < 4; ++k) o[k] = (half_t)fmaxf(v[k], 0.f);
    *(h4_t*)(out + p * D + c) = o;
}

// ---- tests (cs_op_parser_read): channels-last fp32 [N][P][C] -> fp32 NCHW [N][C][P]
__global__ void p_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, long total, int C, long P)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long p = i % P, c = (i / P) % C, n = i / (P * C);
    out[i] = in[(n * P + p) * C + c];
}

}  // namespace

#define P_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { cs_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); return -1; } } while (0)

int launch_p_input(const float* pv, half_t* out, int B, int H, int W, hipStream_t st)
{
    if (!pv || !out || B < 1 || H < 1 || W < 1) { cs_set_error("parser_input16: bad arguments"); return -1; }
    const long total = (long)B * H * W;
    p_input_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(pv, out, total, (long)H * W);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_gemm(const PGemmCall& g, hipStream_t st)
{
    if (!g.a || !g.w || !g.out || g.M < 1) { cs_set_error("parser_gemm: bad arguments"); return -1; }
    if (g.K < 32 || g.K % 32) { cs_set_error("parser_gemm: K = %d (a multiple of 32)", g.K); return -1; }
    if (g.N < 64 || g.N % 64) { cs_set_error("parser_gemm: N = %d (a multiple of 64)", g.N); return -1; }
    if (g.mode < P_GEMM_F16 || g.mode > P_GEMM_NCHW) { cs_set_error("parser_gemm: no epilogue %d", g.mode); return -1; }
    if (g.mode == P_GEMM_NCHW && (g.P < 1 || g.L < 1 || g.L > g.N || g.M % g.P)) { cs_set_error("parser_gemm: bad NCHW epilogue (P = %d, L = %d)", g.P, g.L); return -1; }
    if ((long)g.M * g.N >= (1L << 31) || (long)g.M * g.K >= (1L << 31)) { cs_set_error("parser_gemm: tensor above 2^31 elements"); return -1; }
    const unsigned gm = (unsigned)((g.M + 127) / 128);
    if (g.N % 128 == 0) p_gemm_kernel<128><<<dim3(gm, g.N / 128), 256, 0, st>>>(g);
    else p_gemm_kernel<64><<<dim3(gm, g.N / 64), 256, 0, st>>>(g);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_ln(const float* in, const float* g, const float* b, float eps, long M, int C, float* out32, half_t* out16, hipStream_t st)
{
    if (!in || !g || !b || (!out32 && !out16) || M < 1 || !(eps >= 0.f)) { cs_set_error("parser_layernorm: bad arguments"); return -1; }
    if (C < 64 || C > 512 || C % 64) { cs_set_error("parser_layernorm: %d channels (a multiple of 64 up to 512)", C); return -1; }
    if ((M + 3) / 4 >= (1L << 31)) { cs_set_error("parser_layernorm: too many tokens"); return -1; }
    p_ln_kernel<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(in, g, b, eps, M, C, out32, out16);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_attn(const half_t* q, const half_t* kv, half_t* ctx, int B, int Nq, int Nk, int heads, int d, hipStream_t st)
{
    if (!q || !kv || !ctx || B < 1 || Nq < 1 || Nk < 1 || heads < 1 || B > 65535 || heads > 65535) { cs_set_error("parser_attention: bad arguments"); return -1; }
    if (d != 32 && d != 64) { cs_set_error("parser_attention: head dimension %d (32 or 64)", d); return -1; }
    if (Nk > 256) { cs_set_error("parser_attention: %d keys (at most 256 in one pass: inputs up to 512 x 512)", Nk); return -1; }
    const int Nkp = (Nk + 31) & ~31;
    const size_t lds = 2 * ((size_t)Nkp * (d + 8) + (size_t)(d + 64) * (Nkp + 8));
    const dim3 grid((unsigned)((Nq + 63) / 64), (unsigned)heads, (unsigned)B);
    const void* k = d == 64 ? (const void*)p_attn_kernel<64> : (const void*)p_attn_kernel<32>;
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);      // per launch: the attribute belongs to the current device
    if (e != hipSuccess) { cs_set_error("parser_attention: %zu bytes of LDS: %s", lds, hipGetErrorString(e)); return -1; }
    if (d == 64) p_attn_kernel<64><<<grid, 256, lds, st>>>(q, kv, ctx, Nq, Nk, heads);
    else p_attn_kernel<32><<<grid, 256, lds, st>>>(q, kv, ctx, Nq, Nk, heads);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_dwgelu(const half_t* in, const float* w, const float* bias, half_t* out, int B, int H, int W, int C, hipStream_t st)
{
    if (!in || !w || !bias || !out || B < 1 || H < 1 || W < 1 || C < 8 || C % 8) { cs_set_error("parser_dwgelu: bad arguments"); return -1; }
    const long n = (long)B * H * W * (C / 8);
    if ((n + 255) / 256 >= (1L << 31)) { cs_set_error("parser_dwgelu: tensor too large"); return -1; }
    p_dwgelu_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, w, bias, out, B, H, W, C);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_upadd(const float* p0, const float* p1, const float* p2, const float* p3, half_t* out, int B, int H, int W, int D, hipStream_t st)
{
    if (!p0 || !p1 || !p2 || !p3 || !out || B < 1 || H < 8 || W < 8 || H % 8 || W % 8 || D < 4 || D % 4) { cs_set_error("parser_upadd: bad arguments"); return -1; }
    const long n = (long)B * H * W * (D / 4);
    if ((n + 255) / 256 >= (1L << 31)) { cs_set_error("parser_upadd: tensor too large"); return -1; }
    p_upadd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p0, p1, p2, p3, out, B, H, W, D);
    P_LAUNCH_CHECK();
    return 0;
}

int launch_p_to_nchw(const float* in, float* out, int N, int C, long P, hipStream_t st)
{
    if (!in || !out || N < 1 || C < 1 || P < 1) { cs_set_error("parser_to_nchw: bad arguments"); return -1; }
    const long total = (long)N * C * P;
    p_to_nchw_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(in, out, total, C, P);
    P_LAUNCH_CHECK();
    return 0;
}

// ---- the network
namespace {
struct PSizes { size_t in16, nc, kvin, kv, st[4], p32[4], pre; };
PSizes p_sizes(const ParserNet& n)
{
    PSizes z{};
    const long H = n.maxH, W = n.maxW, nk = (H / 32) * (W / 32);
    z.in16 = (size_t)H * W * P_CIN0;
    for (int s = 0; s < 4; ++s) {
        const size_t tok = (size_t)(H >> (s + 2)) * (W >> (s + 2));
        z.st[s] = tok * n.st[s].C;
        z.p32[s] = tok * n.D;
        if (z.st[s] > z.nc) z.nc = z.st[s];
        if ((size_t)nk * n.st[s].C > z.kvin) z.kvin = (size_t)nk * n.st[s].C;
    }
    z.kv = 2 * z.kvin;
    z.pre = (size_t)(H / 4) * (W / 4) * n.D;
    return z;
}
}  // namespace

size_t parser_workspace_bytes(const ParserNet& n, int cap)
{
    const PSizes z = p_sizes(n);
    size_t per = z.in16 * 2 + z.nc * 4 * 2 + z.nc * 2 * 3 + z.kvin * 4 + z.kvin * 2 + z.kv * 2 + (size_t)n.mlp * z.nc * 2 * 2 + z.pre * 2;
    for (int s = 0; s < 4; ++s) per += z.st[s] * 4 + z.st[s] * 2 + z.p32[s] * 4;
    return per * cap + 40 * 256;          // every buffer starts on a 256-byte boundary
}

void parser_bind_workspace(ParserNet& n, void* ws, int cap)
{
    const PSizes z = p_sizes(n);
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { void* q = p; p += (bytes * cap + 255) / 256 * 256; return q; };
    n.cap = cap;
    n.in16 = (half_t*)take(z.in16 * 2);
    n.x32 = (float*)take(z.nc * 4); n.s32 = (float*)take(z.nc * 4);
    n.a16 = (half_t*)take(z.nc * 2); n.q16 = (half_t*)take(z.nc * 2); n.c16 = (half_t*)take(z.nc * 2);
    n.sr32 = (float*)take(z.kvin * 4); n.kvin16 = (half_t*)take(z.kvin * 2); n.kv16 = (half_t*)take(z.kv * 2);
    n.h16 = (half_t*)take((size_t)n.mlp * z.nc * 2); n.g16 = (half_t*)take((size_t)n.mlp * z.nc * 2);
    for (int s = 0; s < 4; ++s) { n.st32[s] = (float*)take(z.st[s] * 4); n.st16[s] = (half_t*)take(z.st[s] * 2); n.p32[s] = (float*)take(z.p32[s] * 4); }
    n.pre16 = (half_t*)take(z.pre * 2);
}

// in16 holds B <= cap images of H x W (multiples of 32 within the workspace's extent); leaves the stage outputs and the pre-classifier map in the
// net's buffers and writes logits fp32 [B][L][H / 4][W / 4]
int parser_forward(ParserNet& n, int B, int H, int W, float* logits, hipStream_t st)
{
    if (B < 1 || B > n.cap) { cs_set_error("parser_forward: batch %d outside [1, %d]", B, n.cap); return -1; }
    if (H < 32 || W < 32 || H % 32 || W % 32 || (long)H * W > (long)n.maxH * n.maxW) { cs_set_error("parser_forward: bad extent %d x %d", H, W); return -1; }
    const int nk = (H / 32) * (W / 32);
    const void* in = n.in16;
    int ih = H, iw = W, cin = P_CIN0;
    auto gemm = [&](const half_t* a, const half_t* w, const float* bias, long M, int K, int N, int mode, void* out, int P = 0, int L = 0) {
        PGemmCall g{a, w, bias, out, (int)M, K, N, mode, P, L};
        return launch_p_gemm(g, st);
    };
    for (int s = 0; s < 4; ++s) {
        const PStage& S = n.st[s];
        const int C = S.C, oh = H >> (s + 2), ow = W >> (s + 2), d = C / S.heads;
        const long M = (long)B * oh * ow;
        IdConvCall c{};
        c.in = in; c.in_f32 = 0; c.N = B; c.IH = ih; c.IW = iw; c.Cin = cin; c.OH = oh; c.OW = ow; c.K = s ? 3 : 7; c.stride = s ? 2 : 4; c.pad = s ? 1 : 3;
        c.w = S.pew; c.bias = S.peb; c.Cout = C; c.slope = nullptr; c.out = n.s32; c.out_f32 = 1;
        if (launch_id_conv(c, st)) return -1;
        if (launch_p_ln(n.s32, S.pelng, S.pelnb, n.eps, M, C, n.x32, nullptr, st)) return -1;
        for (int k = 0; k < S.depth; ++k) {
            const PBlock& K = S.blk[k];
            if (launch_p_ln(n.x32, K.ln1g, K.ln1b, n.eps, M, C, nullptr, n.a16, st)) return -1;
            if (gemm(n.a16, K.qw, K.qb, M, C, C, P_GEMM_F16, n.q16)) return -1;
            const half_t* kvin = n.a16;
            if (S.sr > 1) {
                c = IdConvCall{};
                c.in = n.a16; c.N = B; c.IH = oh; c.IW = ow; c.Cin = C; c.OH = oh / S.sr; c.OW = ow / S.sr; c.K = S.sr; c.stride = S.sr; c.pad = 0;
                c.w = K.srw; c.bias = K.srb; c.Cout = C; c.out = n.sr32; c.out_f32 = 1;
                if (launch_id_conv(c, st)) return -1;
                if (launch_p_ln(n.sr32, K.srlng, K.srlnb, n.eps, (long)B * nk, C, nullptr, n.kvin16, st)) return -1;
                kvin = n.kvin16;
            }
            if (gemm(kvin, K.kvw, K.kvb, (long)B * nk, C, 2 * C, P_GEMM_F16, n.kv16)) return -1;
            if (launch_p_attn(n.q16, n.kv16, n.c16, B, oh * ow, nk, S.heads, d, st)) return -1;
            if (gemm(n.c16, K.ow, K.ob, M, C, C, P_GEMM_RES, n.x32)) return -1;
            if (launch_p_ln(n.x32, K.ln2g, K.ln2b, n.eps, M, C, nullptr, n.a16, st)) return -1;
            if (gemm(n.a16, K.fc1w, K.fc1b, M, C, n.mlp * C, P_GEMM_F16, n.h16)) return -1;
            if (launch_p_dwgelu(n.h16, K.dww, K.dwb, n.g16, B, oh, ow, n.mlp * C, st)) return -1;
            if (gemm(n.g16, K.fc2w, K.fc2b, M, n.mlp * C, C, P_GEMM_RES, n.x32)) return -1;
        }
        if (launch_p_ln(n.x32, S.lng, S.lnb, n.eps, M, C, n.st32[s], n.st16[s], st)) return -1;
        if (gemm(n.st16[s], S.headw, s == 0 ? n.headb : nullptr, M, C, n.D, P_GEMM_F32, n.p32[s])) return -1;
        in = n.st16[s]; ih = oh; iw = ow; cin = C;
    }
    const int h0 = H / 4, w0 = W / 4;
    if (launch_p_upadd(n.p32[0], n.p32[1], n.p32[2], n.p32[3], n.pre16, B, h0, w0, n.D, st)) return -1;
    n.lastB = B; n.lastH = H; n.lastW = W;
    return gemm(n.pre16, n.clsw, n.clsb, (long)B * h0 * w0, n.D, n.Lpad, P_GEMM_NCHW, logits, h0 * w0, n.L);
}
