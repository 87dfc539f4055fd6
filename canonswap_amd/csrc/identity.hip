// The ArcFace identity network behind can_swapper.getid (can_swap_e2e.py:102-107; models/arcface_models.py:10-136,
// ResNet(IRBlock, [3, 4, 14, 3], use_se=True)) on gfx950: nearest resize to 112 x 112, stem, 24 IRBlocks with squeeze-excitation,
// bn2 -> fc -> bn3, L2 normalisation.  It runs once per identity, so every kernel here is the plain form: activations are contiguous
// channels-last [B][H][W][C] tensors at their real extents (110, 55, 28, 14, 7), the convolution is a direct implicit GEMM that reads its
// MFMA fragments straight from global memory (zero for padding, any stride), and every sum has one fixed order - no float atomics, a row's
// bits do not depend on the batch it is part of.  BatchNorms are folded at load time (pack.py _pack_A).
#include "common.h"

namespace {

constexpr int ID_IN = 112, ID_CIN0 = 32;      // the stem reads 3 real + 29 zero channels (one 32-deep K-step per tap)

__device__ __forceinline__ float prelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---- input: F.interpolate(img, size=(112, 112)) in nearest mode (src = min(floor(dst * (float)in / 112), in - 1), ATen's float arithmetic)
// fp32 NCHW images, or uint8 HWC crops through a [3][256] table -> fp16 [B][112][112][32]
__global__ void id_input_kernel(const float* __restrict__ img, const unsigned char* __restrict__ u8, const float* __restrict__ lut,
                                half_t* __restrict__ out, int B, int H, int W)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * ID_IN * ID_IN) return;
    const int ox = i % ID_IN, oy = (i / ID_IN) % ID_IN, n = i / (ID_IN * ID_IN);
    const float sh = (float)H / (float)ID_IN, sw = (float)W / (float)ID_IN;
    const int sy = min((int)floorf(oy * sh), H - 1), sx = min((int)floorf(ox * sw), W - 1);
    h8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        float f;
        if (u8) f = lut[c * 256 + u8[(((long)n * H + sy) * W + sx) * 3 + c]];
        else f = img[(((long)n * 3 + c) * H + sy) * W + sx];
        v[c] = (half_t)f;
    }
    h8_t* o = (h8_t*)(out + (long)i * ID_CIN0);
    const h8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
    o[0] = v; o[1] = z; o[2] = z; o[3] = z;
}

// ---- convolution: M = N * OH * OW output positions x Cout, K = taps x Cin.  One workgroup = 32 positions x 64 channels; its four waves
// split the K-steps (tap, 32-channel chunk) into four contiguous ranges and wave 0 adds the partial tiles through LDS in wave order.
// v_mfma_f32_16x16x32_f16: lane l holds A[row l & 15][k = 8 (l >> 4) + j] (positions) and B[k][col l & 15] (output channels), 16 bytes each;
// result register r of lane l is row 4 (l >> 4) + r, column l & 15.
template <bool IN_F32>
__global__ void __launch_bounds__(256) id_conv_kernel(IdConvCall c)
{
    __shared__ float red[3][32][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int M = c.N * c.OH * c.OW, NC = c.Cin >> 5, S = c.K * c.K * NC;
    const int p0 = blockIdx.x * 32, co0 = blockIdx.y * 64;
    int pn[2], py[2], px[2]; bool pv[2];
    for (int m = 0; m < 2; ++m) {
        const int p = p0 + m * 16 + lr;
        pv[m] = p < M;
        const int q = pv[m] ? p : 0;
        pn[m] = q / (c.OH * c.OW);
        const int r = q - pn[m] * (c.OH * c.OW);
        py[m] = (r / c.OW) * c.stride - c.pad;
        px[m] = (r % c.OW) * c.stride - c.pad;
    }
    f4_t acc[2][4];
    for (int m = 0; m < 2; ++m) for (int j = 0; j < 4; ++j) acc[m][j] = f4_t{0.f, 0.f, 0.f, 0.f};
    const int s0 = S * wv / 4, s1 = S * (wv + 1) / 4;
    for (int s = s0; s < s1; ++s) {
        const int tap = s / NC, ch = s - tap * NC;
        const int kh = tap / c.K, kw = tap - kh * c.K;
        const int cofs = ch * 32 + lk * 8;
        h8_t a[2], b[4];
        for (int m = 0; m < 2; ++m) {
            const int iy = py[m] + kh, ix = px[m] + kw;
            const bool ok = pv[m] && iy >= 0 && iy < c.IH && ix >= 0 && ix < c.IW;
            a[m] = h8_t{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) {
                const long o = (((long)pn[m] * c.IH + iy) * c.IW + ix) * c.Cin + cofs;
                if (IN_F32) {
                    const f4_t u = *(const f4_t*)((const float*)c.in + o), v = *(const f4_t*)((const float*)c.in + o + 4);
                    a[m] = h8_t{(half_t)u[0], (half_t)u[1], (half_t)u[2], (half_t)u[3], (half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                } else {
                    a[m] = *(const h8_t*)((const half_t*)c.in + o);
                }
            }
        }
        for (int j = 0; j < 4; ++j)
            b[j] = *(const h8_t*)(c.w + ((long)tap * c.Cout + co0 + j * 16 + lr) * c.Cin + cofs);
        for (int m = 0; m < 2; ++m)
            for (int j = 0; j < 4; ++j)
                acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], b[j], acc[m][j], 0, 0, 0);
    }
    if (wv > 0)
        for (int m = 0; m < 2; ++m) for (int j = 0; j < 4; ++j) for (int r = 0; r < 4; ++r) red[wv - 1][(m * 4 + j) * 4 + r][lane] = acc[m][j][r];
    __syncthreads();
    if (wv > 0) return;
    const float slope = c.slope ? *c.slope : 1.f;
    for (int m = 0; m < 2; ++m)
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + j * 16 + lr;
            const float bias = c.bias ? c.bias[co] : 0.f;
            for (int r = 0; r < 4; ++r) {
                const int p = p0 + m * 16 + lk * 4 + r;
                if (p >= M) continue;
                const int i = (m * 4 + j) * 4 + r;
                float v = acc[m][j][r];
                v += red[0][i][lane]; v += red[1][i][lane]; v += red[2][i][lane];
                v = prelu(v + bias, slope);
                if (c.out_f32) ((float*)c.out)[(long)p * c.Cout + co] = v;
                else ((half_t*)c.out)[(long)p * c.Cout + co] = (half_t)v;
            }
        }
}

// ---- MaxPool2d(2, 2) of the stem (fp32 [B][IH][IW][C] -> [B][IH/2][IW/2][C]): the residual stream x and the first block's bn0 copy a = fp16(x s + t)
__global__ void id_maxpool_kernel(const float* __restrict__ in, const float* __restrict__ s, const float* __restrict__ t, float* __restrict__ x,
                                  half_t* __restrict__ a, int B, int IH, int IW, int C)
{
    const int OH = IH / 2, OW = IW / 2, C4 = C / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * OH * OW * C4) return;
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int ox = (int)(p % OW), oy = (int)((p / OW) % OH), n = (int)(p / ((long)OW * OH));
    const float* q = in + (((long)n * IH + 2 * oy) * IW + 2 * ox) * C + c;
    const f4_t v00 = *(const f4_t*)q, v01 = *(const f4_t*)(q + C), v10 = *(const f4_t*)(q + (long)IW * C), v11 = *(const f4_t*)(q + (long)IW * C + C);
    f4_t v; h4_t h;
    for (int k = 0; k < 4; ++k) {
        v[k] = fmaxf(fmaxf(v00[k], v01[k]), fmaxf(v10[k], v11[k]));
        h[k] = (half_t)fmaf(v[k], s[c + k], t[c + k]);
    }
    *(f4_t*)(x + p * C + c) = v;
    *(h4_t*)(a + p * C + c) = h;
}

// ---- squeeze-excitation gate (arcface_models.py:10-25): se[n][c] = sigmoid(W2 prelu(W1 mean_hw(out[n]) + b1) + b2); one workgroup per sample.
// out: fp32, position (h, w) of sample n at n sN + h sH + w sW (so a map can be read at its even positions).  The mean is summed in a fixed
// order: NG = 1024 / C threads share a channel, thread g of them adds positions g, g + NG, ...; the NG partial sums are then added in g order.
__global__ void __launch_bounds__(1024) id_se_kernel(const float* __restrict__ out, long sN, long sH, long sW, int H, int W, int C,
                                                     const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ slope,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ se)
{
    __shared__ float part[1024];
    __shared__ float mean[512];
    __shared__ float hid[32];
    const int tid = threadIdx.x, n = blockIdx.x, P = H * W, R = C / 16;
    const int NG = 1024 / C, g = tid / C, c = tid % C;          // C in {64, 128, 256, 512}: NG = 16, 8, 4, 2
    const float* o = out + n * sN + c;
    float s = 0.f;
#pragma unroll 4
    for (int p = g; p < P; p += NG) s += o[(p / W) * sH + (p % W) * sW];
    part[g * C + c] = s;
    __syncthreads();
    if (tid < C) {
        float m = 0.f;
        for (int k = 0; k < NG; ++k) m += part[k * C + tid];
        mean[tid] = m / (float)P;
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    for (int j = wv; j < R; j += 16) {
        float d = 0.f;
        for (int k = lane; k < C; k += 64) d = fmaf(w1[j * C + k], mean[k], d);
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
        if (lane == 0) hid[j] = prelu(d + b1[j], *slope);
    }
    __syncthreads();
    if (tid < C) {
        float d = b2[tid];
        for (int j = 0; j < R; ++j) d = fmaf(w2[tid * R + j], hid[j], d);
        se[n * C + tid] = 1.f / (1.f + expf(-d));
    }
}

// ---- block tail (arcface_models.py:54-63): x = prelu(out * se + res); a = fp16(x s + t), the next block's bn0 (or the net's bn2) copy
__global__ void id_tail_kernel(const float* __restrict__ out, long sN, long sH, long sW, const float* __restrict__ se, const float* __restrict__ res,
                               const float* __restrict__ slope, const float* __restrict__ s, const float* __restrict__ t, float* __restrict__ x,
                               half_t* __restrict__ a, int B, int H, int W, int C)
{
    const int C4 = C / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * H * W * C4) return;
    const int c = (int)(i % C4) * 4;
    const long p = i / C4;
    const int w = (int)(p % W), h = (int)((p / W) % H), n = (int)(p / ((long)W * H));
    const f4_t o = *(const f4_t*)(out + n * sN + h * sH + w * sW + c), r = *(const f4_t*)(res + p * C + c), g = *(const f4_t*)(se + n * C + c);
    const float sl = *slope;
    f4_t v; h4_t hh;
    for (int k = 0; k < 4; ++k) {
        v[k] = prelu(fmaf(o[k], g[k], r[k]), sl);
        hh[k] = (half_t)fmaf(v[k], s[c + k], t[c + k]);
    }
    *(f4_t*)(x + p * C + c) = v;
    *(h4_t*)(a + p * C + c) = hh;
}

// ---- embedding (arcface_models.py:129-134): a = fp16 bn2(x) [B][49][512]; fc as 49 position slices of [512 out][512 in] fp16 (bn3's scale folded
// into the rows, columns in the engine's (h, w, c) order).  Workgroup (pos, channel block of 64) writes the slice's partial product
// part[pos][b][o]; id_embed_finish adds the 49 slices in position order, the bias, and normalises.
__global__ void __launch_bounds__(256) id_embed_kernel(const half_t* __restrict__ a, const half_t* __restrict__ w, float* __restrict__ part, int B)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int pos = blockIdx.x, co = blockIdx.y * 64 + wv * 16 + lr;
    const half_t* wr = w + ((long)pos * 512 + co) * 512 + lk * 8;
    for (int b0 = 0; b0 < B; b0 += 16) {
        const int b = b0 + lr;
        const half_t* ar = a + ((long)(b < B ? b : 0) * 49 + pos) * 512 + lk * 8;
        f4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ch = 0; ch < 16; ++ch) {
            h8_t av = *(const h8_t*)(ar + ch * 32);
            if (b >= B) av = h8_t{0, 0, 0, 0, 0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, *(const h8_t*)(wr + ch * 32), acc, 0, 0, 0);
        }
        for (int r = 0; r < 4; ++r) {
            const int bo = b0 + lk * 4 + r;
            if (bo < B) part[((long)pos * B + bo) * 512 + co] = acc[r];
        }
    }
}

__global__ void __launch_bounds__(512) id_embed_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ raw,
                                                              float* __restrict__ idn, int B)
{
    __shared__ float sq[512];
    const int c = threadIdx.x, b = blockIdx.x;
    float v = 0.f;
    for (int pos = 0; pos < 49; ++pos) v += part[((long)pos * B + b) * 512 + c];
    v += bias[c];
    if (raw) raw[b * 512 + c] = v;
    if (!idn) return;
    sq[c] = v * v;
    __syncthreads();
    for (int k = 256; k > 0; k >>= 1) {          // fixed tree: the norm does not depend on scheduling
        if (c < k) sq[c] += sq[c + k];
        __syncthreads();
    }
    idn[b * 512 + c] = v / fmaxf(sqrtf(sq[0]), 1e-12f);      // F.normalize(p=2, dim=1, eps=1e-12)
}

// ---- tests (cs_op_identity_read): channels-last fp32 / fp16 [N][P][C] -> fp32 NCHW [N][C][P]
__global__ void id_to_nchw_kernel(const void* __restrict__ in, int is_f16, float* __restrict__ out, long total, int C, int P)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i % P), c = (int)((i / P) % C);
    const long n = i / ((long)P * C), src = (n * P + p) * C + c;
    out[i] = is_f16 ? (float)((const half_t*)in)[src] : ((const float*)in)[src];
}

}  // namespace

#define ID_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { cs_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); return -1; } } while (0)

int launch_id_input(const float* img, const unsigned char* u8, const float* lut, half_t* out, int B, int H, int W, hipStream_t st)
{
    if ((!img && !u8) || (u8 && !lut) || !out || B < 1 || H < 1 || W < 1) { cs_set_error("id_input: bad arguments"); return -1; }
    const int n = B * ID_IN * ID_IN;
    id_input_kernel<<<(n + 255) / 256, 256, 0, st>>>(img, u8, lut, out, B, H, W);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_conv(const IdConvCall& c, hipStream_t st)
{
    if (!c.in || !c.w || !c.out || c.N < 1 || c.IH < 1 || c.IW < 1 || c.Cin < 32 || c.Cin % 32 || c.Cout < 64 || c.Cout % 64 ||
        c.K < 1 || c.K > 8 || c.stride < 1 || c.pad < 0 || c.pad >= c.K) { cs_set_error("id_conv: bad arguments"); return -1; }
    if (c.IH + 2 * c.pad < c.K || c.IW + 2 * c.pad < c.K) { cs_set_error("id_conv: input smaller than the kernel"); return -1; }
    if (c.OH != (c.IH + 2 * c.pad - c.K) / c.stride + 1 || c.OW != (c.IW + 2 * c.pad - c.K) / c.stride + 1) { cs_set_error("id_conv: output extent does not match"); return -1; }
    const long M = (long)c.N * c.OH * c.OW;
    if (M * c.Cout >= (1L << 31) || (long)c.N * c.IH * c.IW * c.Cin >= (1L << 31)) { cs_set_error("id_conv: tensor above 2^31 elements"); return -1; }
    const dim3 grid((unsigned)((M + 31) / 32), (unsigned)(c.Cout / 64));
    if (c.in_f32) id_conv_kernel<true><<<grid, 256, 0, st>>>(c);
    else id_conv_kernel<false><<<grid, 256, 0, st>>>(c);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_maxpool(const float* in, const float* s, const float* t, float* x, half_t* a, int B, int IH, int IW, int C, hipStream_t st)
{
    if (!in || !s || !t || !x || !a || B < 1 || IH < 2 || IW < 2 || C < 4 || C % 4) { cs_set_error("id_maxpool: bad arguments"); return -1; }
    const long n = (long)B * (IH / 2) * (IW / 2) * (C / 4);
    id_maxpool_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, s, t, x, a, B, IH, IW, C);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_se(const float* out, long sN, long sH, long sW, int B, int H, int W, int C, const float* w1, const float* b1, const float* slope,
                 const float* w2, const float* b2, float* se, hipStream_t st)
{
    if (!out || !w1 || !b1 || !slope || !w2 || !b2 || !se || B < 1 || H < 1 || W < 1) { cs_set_error("id_se: bad arguments"); return -1; }
    if (C != 64 && C != 128 && C != 256 && C != 512) { cs_set_error("id_se: %d channels (64, 128, 256 or 512)", C); return -1; }
    id_se_kernel<<<B, 1024, 0, st>>>(out, sN, sH, sW, H, W, C, w1, b1, slope, w2, b2, se);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_tail(const float* out, long sN, long sH, long sW, const float* se, const float* res, const float* slope, const float* s, const float* t,
                   float* x, half_t* a, int B, int H, int W, int C, hipStream_t st)
{
    if (!out || !se || !res || !slope || !s || !t || !x || !a || B < 1 || H < 1 || W < 1 || C < 4 || C % 4 || (sN | sH | sW) % 4) {
        cs_set_error("id_tail: bad arguments"); return -1;
    }
    const long n = (long)B * H * W * (C / 4);
    id_tail_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(out, sN, sH, sW, se, res, slope, s, t, x, a, B, H, W, C);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_embed(const half_t* a, const half_t* w, const float* bias, float* part, float* raw, float* idn, int B, hipStream_t st)
{
    if (!a || !w || !bias || !part || (!raw && !idn) || B < 1) { cs_set_error("id_embed: bad arguments"); return -1; }
    id_embed_kernel<<<dim3(49, 8), 256, 0, st>>>(a, w, part, B);
    ID_LAUNCH_CHECK();
    id_embed_finish_kernel<<<B, 512, 0, st>>>(part, bias, raw, idn, B);
    ID_LAUNCH_CHECK();
    return 0;
}

int launch_id_to_nchw(const void* in, int is_f16, float* out, int N, int C, int P, hipStream_t st)
{
    if (!in || !out || N < 1 || C < 1 || P < 1) { cs_set_error("id_to_nchw: bad arguments"); return -1; }
    const long total = (long)N * C * P;
    id_to_nchw_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(in, is_f16, out, total, C, P);
    ID_LAUNCH_CHECK();
    return 0;
}

// ---- the network
size_t idnet_workspace_bytes(int cap)
{
    size_t per = 0;
    per += (size_t)ID_IN * ID_IN * ID_CIN0 * 2;            // in16
    per += (size_t)110 * 110 * 64 * 4 + (size_t)55 * 55 * 64 * 4;      // stem32, stem_x
    for (int l = 0; l < 4; ++l) per += 2 * (size_t)IDNET_HW[l] * IDNET_HW[l] * IDNET_C[l] * 4;      // xs
    per += 2 * (size_t)55 * 55 * 64 * 2;                   // a16, h16
    per += (size_t)55 * 55 * 64 * 4 + (size_t)28 * 28 * 128 * 4;      // o32, ds32
    per += 512 * 4 + (size_t)49 * 512 * 4;                 // se, part
    return per * cap + 32 * 256;          // every buffer starts on a 256-byte boundary
}

void idnet_bind_workspace(IdNet& n, void* ws, int cap)
{
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { void* q = p; p += (bytes * cap + 255) / 256 * 256; return q; };
    n.cap = cap;
    n.in16 = (half_t*)take((size_t)ID_IN * ID_IN * ID_CIN0 * 2);
    n.stem32 = (float*)take((size_t)110 * 110 * 64 * 4);
    n.stem_x = (float*)take((size_t)55 * 55 * 64 * 4);
    for (int l = 0; l < 4; ++l) for (int k = 0; k < 2; ++k) n.xs[l][k] = (float*)take((size_t)IDNET_HW[l] * IDNET_HW[l] * IDNET_C[l] * 4);
    n.a16 = (half_t*)take((size_t)55 * 55 * 64 * 2);
    n.h16 = (half_t*)take((size_t)55 * 55 * 64 * 2);
    n.o32 = (float*)take((size_t)55 * 55 * 64 * 4);
    n.ds32 = (float*)take((size_t)28 * 28 * 128 * 4);
    n.se = (float*)take(512 * 4);
    n.part = (float*)take((size_t)49 * 512 * 4);
}

// in16 holds B <= cap resized images; leaves the stage activations in the net's buffers and writes the embeddings
int idnet_forward(IdNet& n, int B, float* idn, float* raw, hipStream_t st)
{
    if (B < 1 || B > n.cap) { cs_set_error("idnet_forward: batch %d outside [1, %d]", B, n.cap); return -1; }
    IdConvCall c{};
    c.in = n.in16; c.in_f32 = 0; c.N = B; c.IH = c.IW = ID_IN; c.Cin = ID_CIN0; c.OH = c.OW = 110; c.stride = 1; c.pad = 0; c.K = 3;
    c.w = n.stem_w; c.bias = n.stem_b; c.Cout = 64; c.slope = n.slopes; c.out = n.stem32; c.out_f32 = 1;
    if (launch_id_conv(c, st)) return -1;
    if (launch_id_maxpool(n.stem32, n.blk[0].s0, n.blk[0].t0, n.stem_x, n.a16, B, 110, 110, 64, st)) return -1;
    const float* x = n.stem_x;
    int bi = 0;
    for (int l = 0; l < 4; ++l) {
        for (int k = 0; k < IDNET_DEPTH[l]; ++k, ++bi) {
            const IdBlock& K = n.blk[bi];
            const int ih = (l > 0 && k == 0) ? IDNET_HW[l - 1] : IDNET_HW[l], oh = IDNET_HW[l];
            c = IdConvCall{};
            c.in = n.a16; c.N = B; c.IH = c.IW = ih; c.Cin = K.cin; c.OH = c.OW = ih; c.stride = 1; c.pad = 1; c.K = 3;
            c.w = K.w1; c.bias = K.b1; c.Cout = K.cin; c.slope = n.slopes + 1 + 2 * bi; c.out = n.h16; c.out_f32 = 0;
            if (launch_id_conv(c, st)) return -1;
            c.in = n.h16; c.OH = c.OW = oh; c.stride = K.stride; c.w = K.w2; c.bias = K.b2; c.Cout = K.cout; c.slope = nullptr;
            c.out = n.o32; c.out_f32 = 1;
            if (launch_id_conv(c, st)) return -1;
            const float* res = x;
            if (K.wd) {
                c.in = x; c.in_f32 = 1; c.pad = 0; c.K = 1; c.w = K.wd; c.bias = K.bd; c.out = n.ds32;
                if (launch_id_conv(c, st)) return -1;
                res = n.ds32;
            }
            const long sW = K.cout, sH = sW * oh, sN = sH * oh;
            if (launch_id_se(n.o32, sN, sH, sW, B, oh, oh, K.cout, K.se_w1, K.se_b1, n.slopes + 2 + 2 * bi, K.se_w2, K.se_b2, n.se, st)) return -1;
            const bool last = bi == 23;
            float* xo = n.xs[l][k & 1];          // the layer's stream alternates between its two buffers
            if (launch_id_tail(n.o32, sN, sH, sW, n.se, res, n.slopes + 1 + 2 * bi, last ? n.post_s : n.blk[bi + 1].s0, last ? n.post_t : n.blk[bi + 1].t0,
                               xo, n.a16, B, oh, oh, K.cout, st)) return -1;
            x = xo;
        }
        n.layer_x[l] = x;
    }
    n.lastB = B;
    return launch_id_embed(n.a16, n.fc_w, n.fc_b, n.part, raw, idn, B, st);
}
