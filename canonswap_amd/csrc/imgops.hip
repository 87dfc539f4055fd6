// Image-space steps on either side of the generator, on the device:
//   * SoftErosion of the face-parsing mask (src/utils/crop.py:21-47),
//   * paste-back of the generated crop into the original frame: cv2.warpAffine of crop and mask + blend
//     (src/utils/crop.py:49-63, 515-529, driven from can_swap_pipeline_e2e.py:267-283),
//   * input staging: cv2.resize(crop, (256,256), INTER_AREA) + /255 + HWC->CHW (src/utils/cropper.py:209, can_swap_e2e.py:126-163),
//   * the crop itself: cv2.warpAffine of the frame into the crop's frame (src/utils/crop.py:429-455, src/utils/cropper.py:196-209).
//   * the face parser's input: cv2.resize to one half + SegformerImageProcessor (PIL resize x 2, rescale, normalize) of a crop
//     (src/can_swap_pipeline_e2e.py:171, 180, src/can_swap_pipeline_v2i.py:73).
//   * the side-by-side video frame: concat_frames (src/utils/video.py:84-109; src/can_swap_pipeline_e2e.py:290, src/can_swap_pipeline_v2i.py:328).
// All of them are HBM-bound byte / float work: one thread per output pixel, coalesced along the row.  The OpenCV steps follow
// OpenCV's published fixed-point algorithm (restated in oracle/cv_ref.py, which the tests compare against bit for bit).
#include "common.h"

// Bit-exact restatements of CPU arithmetic (numpy / OpenCV evaluate a * b + c with two roundings): no FMA contraction in this file.
// Plain operators on purpose: the __fmul_rn / __fadd_rn intrinsics are header functions compiled with contraction allowed, and
// once inlined their multiply and add fuse again.  The fp32 convolution of SoftErosion asks for fmaf explicitly.
#pragma clang fp contract(off)

#include "warp_taps.h"      // staged_value, affine_coords, Tap, tap_at, tap_u8x3 (shared with landmarks.hip); AffineInv, invert_affine, face_box (affine_inv.h)

#define LAUNCH_CHECK(name)                                                                       \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) { cs_set_error(name " launch: %s", hipGetErrorString(_e)); return -1; } \
    } while (0)

// ---------------------------------------------------------------------------------------------- SoftErosion
// one pass: out = conv2d(in, w, padding = r) [zero padding], optionally out = min(in, out)  (crop.py:38-41)
// Round 6: register tiled.  A workgroup owns 64 x 32 outputs, a thread 8 consecutive outputs of one row: per kernel row it reads the
// 8 + KS - 1 inputs it needs ONCE from LDS (seven ds_read_b128; the lane -> address map (row stride 84 floats, 32 B between lanes) is
// conflict free for that instruction: the 16 lanes of a group cover the 64 banks) and issues KS x 8 FMAs on them, the weights are
// wave-uniform scalar loads, the FMAs packed two per instruction (v_pk_fma_f32).  One LDS read per six FMAs instead of two per FMA: the pass is VALU-bound (0.69 GFLOP per frame and
// three passes, crop.py:29-35 - the kernel is a cone, not separable).  An output's products are added in the order (ky, kx) ascending.
// IN: float (0/1 masks as the reference's .float() makes them, or the previous pass) or uint8 (0/1 labels straight from the parser).
template <int KS, typename IN>
__global__ void __launch_bounds__(256) se_conv_kernel(const IN* __restrict__ in, const float* __restrict__ w, float* __restrict__ out,
                                                      int H, int W, int take_min)
{
    constexpr int R = KS / 2, NX = 8, TW = 64, TH = 32, LW = 84, LH = TH + 2 * R, NV = (NX + 2 * R + 3) / 4;
    static_assert(TW + 2 * R <= LW && LW % 8 == 4, "row stride: 16 B aligned and an odd multiple of 16 B");
    __shared__ __attribute__((aligned(16))) float tile[LH * LW + 4];
    const int n = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const IN* src = in + (long)n * H * W;
    {   // staging: thread -> (column lx, rows ly0, ly0 + 3, ...): one division per thread, not per element (252 of the 256 threads; LW = 84)
        const int lx = threadIdx.x % LW, ly0 = threadIdx.x / LW, x = x0 + lx - R;
        const bool xin = (unsigned)x < (unsigned)W;
        if (ly0 < 3) {
#pragma unroll 6
            for (int ly = ly0; ly < LH; ly += 3) {
                const int y = y0 + ly - R;
                tile[ly * LW + lx] = (xin && (unsigned)y < (unsigned)H) ? (float)src[(long)y * W + x] : 0.f;
            }
        }
    }
    __syncthreads();
    const int g = threadIdx.x & 7, r = threadIdx.x >> 3;
    // packed fp32 FMAs (v_pk_fma_f32: two lanes' worth of FMA per instruction slot): outputs in pairs (2p, 2p + 1); an even tap reads the
    // aligned input pairs E[j] = (v[2j], v[2j + 1]), an odd tap the shifted pairs O[j] = (v[2j + 1], v[2j + 2]) (one v_pk_mov_b32 each per
    // kernel row).  84 packed FMAs + 13 moves per kernel row instead of 168 FMAs; every output still adds its products in (ky, kx) order.
    typedef float f2_t __attribute__((ext_vector_type(2)));
    constexpr int NP = NX / 2, NE = NV * 2;
    f2_t acc2[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc2[p] = (f2_t){0.f, 0.f};
#pragma unroll 1
    for (int ky = 0; ky < KS; ++ky) {
        const float4* rp = (const float4*)(tile + (r + ky) * LW + g * NX);
        f2_t E[NE], O[NE - 1];
#pragma unroll
        for (int j = 0; j < NV; ++j) { const float4 q = rp[j]; E[2 * j] = (f2_t){q.x, q.y}; E[2 * j + 1] = (f2_t){q.z, q.w}; }
#pragma unroll
        for (int j = 0; j < NE - 1; ++j) O[j] = (f2_t){E[j].y, E[j + 1].x};
        const float* wr = w + ky * KS;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const float wv = wr[kx];
            const f2_t w2 = (f2_t){wv, wv};
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const f2_t in2 = (kx & 1) ? O[p + (kx - 1) / 2] : E[p + kx / 2];
                acc2[p] = __builtin_elementwise_fma(in2, w2, acc2[p]);
            }
        }
    }
    float acc[NX];
#pragma unroll
    for (int p = 0; p < NP; ++p) { acc[2 * p] = acc2[p].x; acc[2 * p + 1] = acc2[p].y; }
    const int y = y0 + r, xb = x0 + g * NX;
    if (y >= H) return;
    float res[NX];
#pragma unroll
    for (int o = 0; o < NX; ++o) {
        const float c = tile[(r + R) * LW + g * NX + R + o];
        res[o] = take_min ? fminf(c, acc[o]) : acc[o];
    }
    float* dst = out + (long)n * H * W + (long)y * W + xb;
    if (xb + NX <= W && (W & 3) == 0) {
        ((float4*)dst)[0] = make_float4(res[0], res[1], res[2], res[3]);
        ((float4*)dst)[1] = make_float4(res[4], res[5], res[6], res[7]);
    } else {
#pragma unroll
        for (int o = 0; o < NX; ++o) if (xb + o < W) dst[o] = res[o];
    }
}

// max over the pixels below the threshold (crop.py:45: `x[~mask].max()` runs over the WHOLE (N,1,H,W) tensor, not per sample -
// ADVICE r2); two deterministic stages (max is order independent): per-(sample, block) partials, then every workgroup of the final
// pass reduces all N x nparts of them once
__global__ void __launch_bounds__(256) se_max_kernel(const float* __restrict__ x, long P, float thr, float* __restrict__ part)
{
    const int n = blockIdx.y;
    float m = -INFINITY;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float v = x[(long)n * P + i];
        if (!(v >= thr)) m = fmaxf(m, v);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

__global__ void __launch_bounds__(256) se_final_kernel(float* __restrict__ x, long P, float thr, const float* __restrict__ part, int nparts,
                                                       unsigned char* __restrict__ hard, int per_sample)
{
    const int n = blockIdx.y;
    if (per_sample) part += (long)n * nparts;      // B independent calls of the module (the pipeline's loop): the maximum of this sample only
    // nparts = blocks x samples: the maximum over the whole batch.  One cooperative pass per workgroup (threads stride over the partials,
    // wave butterfly, four wave results through LDS) instead of every thread looping over all of them (4096 broadcast loads per thread at
    // 64 frames: ADVICE r3); max is order independent, so the value is the same.
    __shared__ float sm[4];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += 256) m = fmaxf(m, part[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float v = x[(long)n * P + i];
    const bool hi = v >= thr;
    x[(long)n * P + i] = hi ? 1.f : v / m;          // x[mask] = 1; x[~mask] /= x[~mask].max()
    if (hard) hard[(long)n * P + i] = hi ? 1 : 0;
}

int launch_soft_erosion(const void* mask, int mask_u8, float* tmp_a, float* tmp_b, const float* w, float* part, float* soft, unsigned char* hard,
                        int B, int H, int W, int ksize, float thr, int iters, int per_sample, hipStream_t st)
{
    if (ksize != 21 && ksize != 15) { cs_set_error("soft_erosion: kernel size %d (21 and 15 are built)", ksize); return -1; }
    if (iters < 1) { cs_set_error("soft_erosion: iterations %d", iters); return -1; }
    const dim3 grid((W + 63) / 64, (H + 31) / 32, B);
    const float* src = nullptr;
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        float* dst = last ? soft : (it % 2 == 0 ? tmp_a : tmp_b);
        const int tm = last ? 0 : 1;
        if (it == 0 && mask_u8) {
            if (ksize == 21) hipLaunchKernelGGL((se_conv_kernel<21, unsigned char>), grid, dim3(256), 0, st, (const unsigned char*)mask, w, dst, H, W, tm);
            else hipLaunchKernelGGL((se_conv_kernel<15, unsigned char>), grid, dim3(256), 0, st, (const unsigned char*)mask, w, dst, H, W, tm);
        } else {
            const float* s_ = it == 0 ? (const float*)mask : src;
            if (ksize == 21) hipLaunchKernelGGL((se_conv_kernel<21, float>), grid, dim3(256), 0, st, s_, w, dst, H, W, tm);
            else hipLaunchKernelGGL((se_conv_kernel<15, float>), grid, dim3(256), 0, st, s_, w, dst, H, W, tm);
        }
        LAUNCH_CHECK("se_conv");
        src = dst;
    }
    const long P = (long)H * W;
    const int nparts = 64;
    hipLaunchKernelGGL(se_max_kernel, dim3(nparts, B), dim3(256), 0, st, soft, P, thr, part);
    LAUNCH_CHECK("se_max");
    hipLaunchKernelGGL(se_final_kernel, dim3((unsigned)((P + 255) / 256), B), dim3(256), 0, st, soft, P, thr, part, per_sample ? nparts : nparts * B, hard,
                       per_sample);
    LAUNCH_CHECK("se_final");
    return 0;
}

// ---------------------------------------------------------------------------------------------- input staging
// cv2.resize(INTER_AREA) by exactly 2 in both directions for 8-bit images: (a + b + c + d + 2) >> 2; then / 255, clip, CHW

__global__ void __launch_bounds__(256) prepare_crops_kernel(const unsigned char* __restrict__ in, float* __restrict__ out, int B, int Hd, int Wd,
                                                            int factor)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long P = (long)Hd * Wd;
    if (i >= (long)B * P) return;
    const int n = (int)(i / P), y = (int)((i % P) / Wd), x = (int)(i % Wd);
    const int Ws = Wd * factor;
    const unsigned char* s = in + ((long)n * Hd * factor + (long)y * factor) * Ws * 3 + (long)x * factor * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v;
        if (factor == 2) v = (s[c] + s[3 + c] + s[(long)Ws * 3 + c] + s[(long)Ws * 3 + 3 + c] + 2) >> 2;
        else v = s[c];
        out[((long)n * 3 + c) * P + (long)y * Wd + x] = staged_value(v);
    }
}

int launch_prepare_crops(const unsigned char* in, float* out, int B, int Hc, int Wc, int factor, hipStream_t st)
{
    const long n = (long)B * (Hc / factor) * (Wc / factor);
    hipLaunchKernelGGL(prepare_crops_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, B, Hc / factor, Wc / factor, factor);
    LAUNCH_CHECK("prepare_crops");
    return 0;
}

// ---------------------------------------------------------------------------------------------- cv2.warpAffine, INTER_LINEAR
// paste_shared_kernel keeps a tap per pixel across its frames as two ints (its launcher bounds the offset): the offset, and
// fx | fy << 5 | (y0, y1, x0, x1) << 10 | !outside << 14.  The word 0 is a pixel that reads nothing.
__device__ __forceinline__ int tap_pack(const Tap& t)
{
    return t.fx | t.fy << 5 | t.y0 << 10 | t.y1 << 11 | t.x0 << 12 | t.x1 << 13 | !t.outside << 14;
}

__device__ __forceinline__ Tap tap_unpack(int o00, int w)
{
    return Tap{o00, w & 31, (w >> 5) & 31, (bool)(w & 1 << 10), (bool)(w & 1 << 11), (bool)(w & 1 << 12), (bool)(w & 1 << 13), !(w >> 14)};
}

// float image, one channel: table weights (1 - a)(1 - b) ... in float, left-to-right sum without contraction (remapBilinear, float)
__device__ __forceinline__ float tap_f32(const float* __restrict__ src, int Ws, const Tap& t)
{
    const float ax = (float)t.fx * 0.03125f, ay = (float)t.fy * 0.03125f;
    const float f00 = (1.f - ay) * (1.f - ax), f01 = (1.f - ay) * ax;
    const float f10 = ay * (1.f - ax), f11 = ay * ax;
    const float* p = src + t.o00;
    const float t00 = (t.y0 && t.x0) ? p[0] : 0.f, t01 = (t.y0 && t.x1) ? p[1] : 0.f;
    const float t10 = (t.y1 && t.x0) ? p[Ws] : 0.f, t11 = (t.y1 && t.x1) ? p[(long)Ws + 1] : 0.f;
    return ((t00 * f00 + t01 * f01) + t10 * f10) + t11 * f11;
}

// out = clip(m * warped + (1 - m) * ori, 0, 255) truncated (crop.py:523-529; np.clip(...).astype(np.uint8)), `rest` = (1 - m) * ori.
// The blend rounds both products and the sum (this file compiles with fp contraction off), so the second product, which in
// paste_shared_kernel does not depend on the frame, may be formed apart (tests/test_gpu_v2i_chain.py holds the kernels bit-equal).
__device__ __forceinline__ unsigned blend_u8(float m, int res, float rest)
{
    return (unsigned)(unsigned char)fminf(fmaxf(m * (float)res + rest, 0.f), 255.f);
}

// crop (u8, 3 channels) warped into the destination frame; with the original image: blended into it under a mask, warped from the
// crop frame here (mask_crop) or given in the destination frame (mask_ori)
__global__ void __launch_bounds__(256) paste_kernel(const unsigned char* __restrict__ crop, const float* __restrict__ mask_crop,
                                                    const float* __restrict__ mask_ori, int Hc, int Wc, AffineInv A,
                                                    const unsigned char* ori, unsigned char* out, int Ho, int Wo)
{
    // ori and out may be ONE buffer: a thread reads and writes its own pixel only
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Ho * Wo) return;
    const int y = (int)(i / Wo), x = (int)(i % Wo);
    const Tap t = tap_at(A, x, y, Hc, Wc);
    int res[3];
    tap_u8x3(crop, Wc, t, res);
    if (!ori) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = (unsigned char)res[c];
        return;
    }
    const float m = mask_ori ? mask_ori[i] : tap_f32(mask_crop, Wc, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = blend_u8(m, res[c], (1.f - m) * (float)ori[i * 3 + c]);
}

// ---- the paste-back step of B frames in one launch (can_swap_pipeline_e2e.py:273-283 per frame: SoftErosion mask -> prepare_paste_back ->
// paste_back).  blockIdx.y = frame; a thread owns PX consecutive pixels of a row, loads them once and stores them once.  PX = 4: 12 bytes = three
// dwords of the original and of the result (the single-frame kernel above moves them byte by byte); PX = 1: one pixel, byte by byte - widths that are
// no multiple of 4 and buffers off a 4-byte boundary.  A pixel whose source position lies outside the crop has mask 0 and warped value 0:
// v = 0 * 0 + (1 - 0) * ori = ori exactly, so it is copied - most of a 1080p frame - and paste_kernel, which blends it, leaves the same byte.
// Same arithmetic per pixel as paste_kernel with mask_crop (tests/test_gpu_chain.py holds the two bit-equal).
struct AffineBatch { AffineInv a[64]; };      // 3 KB of kernel arguments: no device-side staging buffer, nothing to race with

// A thread's group q of PX pixels of a frame as dwords, loaded and stored once: PX = 8: 24 bytes, 8-byte aligned (three 8-byte accesses); PX = 4:
// three dwords; PX = 1: three single bytes, in the low bytes of w[0].  The launchers choose PX by the row width and the buffers' alignment.
template <int PX> constexpr int PX_WORDS = (PX * 3 + 3) / 4;

template <int PX>
__device__ __forceinline__ void load_px(const unsigned char* frame, long q, unsigned (&w)[PX_WORDS<PX>])
{
    if constexpr (PX == 8) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint2 v = ((const uint2*)frame)[q * 3 + j];
            w[2 * j] = v.x; w[2 * j + 1] = v.y;
        }
    } else if constexpr (PX == 1) {
        const unsigned char* in = frame + q * 3;
        w[0] = in[0] | in[1] << 8 | in[2] << 16;
    } else {
#pragma unroll
        for (int j = 0; j < PX_WORDS<PX>; ++j) w[j] = ((const unsigned*)frame)[q * PX_WORDS<PX> + j];
    }
}

template <int PX>
__device__ __forceinline__ void store_px(unsigned char* frame, long q, const unsigned (&w)[PX_WORDS<PX>])
{
    if constexpr (PX == 8) {
        uint2* out = (uint2*)frame + q * 3;
        out[0] = make_uint2(w[0], w[1]); out[1] = make_uint2(w[2], w[3]); out[2] = make_uint2(w[4], w[5]);
    } else if constexpr (PX == 1) {
        unsigned char* out = frame + q * 3;
        out[0] = (unsigned char)w[0]; out[1] = (unsigned char)(w[0] >> 8); out[2] = (unsigned char)(w[0] >> 16);
    } else {
        unsigned* out = (unsigned*)frame + q * PX_WORDS<PX>;
#pragma unroll
        for (int j = 0; j < PX_WORDS<PX>; ++j) out[j] = w[j];
    }
}

// one face into a thread's PX pixels (xb .. xb + PX - 1, y), px their 3 PX bytes: the pixel is truncated to 8 bits, as paste_back's astype(np.uint8)
template <int PX>
__device__ __forceinline__ void paste_px(const unsigned char* __restrict__ crop, const float* __restrict__ mask_crop, int Hc, int Wc,
                                         const AffineInv& A, int xb, int y, unsigned char* px)
{
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const Tap t = tap_at(A, xb + k, y, Hc, Wc);
        if (t.outside) continue;                                           // the original pixel
        const float m = tap_f32(mask_crop, Wc, t);
        int res[3];
        tap_u8x3(crop, Wc, t, res);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k * 3 + c] = blend_u8(m, res[c], (1.f - m) * (float)px[k * 3 + c]);
    }
}

template <int PX>
__global__ void __launch_bounds__(256) paste_batch_kernel(const unsigned char* __restrict__ crops, const float* __restrict__ masks, int Hc, int Wc,
                                                          AffineBatch AB, const unsigned char* __restrict__ oris,
                                                          unsigned char* __restrict__ outs, int Ho, int Wo)
{
    const int n = blockIdx.y;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;          // group of PX pixels
    const long P = (long)Ho * Wo;
    if (q * PX >= P) return;
    const AffineInv& A = AB.a[n];
    const unsigned char* crop = crops + (long)n * Hc * Wc * 3;
    const float* mask_crop = masks + (long)n * Hc * Wc;
    unsigned wv[PX_WORDS<PX>];
    load_px<PX>(oris + (long)n * P * 3, q, wv);
    const int y = (int)((q * PX) / Wo), xb = (int)((q * PX) % Wo);
    paste_px<PX>(crop, mask_crop, Hc, Wc, A, xb, y, (unsigned char*)wv);
    store_px<PX>(outs + (long)n * P * 3, q, wv);
}

// ---- several faces per frame: prepare_paste_back + paste_back (crop.py:515-529) applied once per face of a frame, in the faces' order, each on
// the result of the one before, in ONE pass over the frame.  blockIdx.y = frame of the launch; a thread owns the PX pixels of
// paste_batch_kernel, loads them once, walks its frame's faces (paste_faces_px: paste_batch_kernel's arithmetic per face, the pixel
// truncated to 8 bits after every face, as sequential paste_back calls leave it) and stores them once: the frames between two faces
// never exist in memory.  A frame without a face is copied (in place: left alone).  Matrices, boxes and face ranges are kernel arguments:
// FACES_PER_LAUNCH = 48 faces and at most as many frames per launch, 48 x (48 B matrix + 16 B box) + 49 x 4 B ranges = 3272 B beside ~70 B of
// scalars, under HIP's 4 KB argument block with the room AffineBatch leaves (64 matrices alone are 3 KB; with box and range 64 faces would be 4356 B).
// box: a conservative integer rectangle (x0, y0, x1, y1, inclusive, clipped to the frame; x0 > x1: empty) that holds every pixel of the frame
// for which !tap_at(...).outside, so a group of pixels outside it skips the face before any double-precision coordinate is formed - most of
// a 1080p frame, for every face.  It prunes only: inside it every pixel still decides by tap_at (face_box, affine_inv.h, for why it cannot cut a pixel).
// oris / outs may be ONE buffer, and a launch may continue a frame that an earlier launch began (resume: frame 0 of this launch is read from
// outs): a thread reads and writes its own bytes only, so neither is a race.  crops and masks must not overlap outs.
constexpr int FACES_PER_LAUNCH = 48;
struct FaceBatch {
    AffineInv a[FACES_PER_LAUNCH];
    int box[FACES_PER_LAUNCH][4];
    int first[FACES_PER_LAUNCH + 1];      // frame j of the launch owns the launch's faces first[j] .. first[j + 1] - 1
};
static_assert(sizeof(FaceBatch) <= 3328, "FaceBatch and the scalars beside it must fit HIP's 4 KB of kernel arguments");

// The walk over n faces of a frame, in order, into a thread's PX pixels: the box test, then paste_px.  crops / masks / a / box: face 0 of the
// walk; a and box are read where they lie, paste_faces_kernel's kernel arguments (scalar loads).
template <int PX>
__device__ __forceinline__ void paste_faces_px(const unsigned char* __restrict__ crops, const float* __restrict__ masks, int Hc, int Wc,
                                               const AffineInv* a, const int (*box)[4], int n, int xb, int y, unsigned char* px)
{
    for (int i = 0; i < n; ++i) {
        if (y < box[i][1] || y > box[i][3] || xb + PX - 1 < box[i][0] || xb > box[i][2]) continue;
        paste_px<PX>(crops + (long)i * Hc * Wc * 3, masks + (long)i * Hc * Wc, Hc, Wc, a[i], xb, y, px);
    }
}

template <int PX>
__global__ void __launch_bounds__(256) paste_faces_kernel(const unsigned char* __restrict__ crops, const float* __restrict__ masks, int Hc, int Wc,
                                                          FaceBatch FB, const unsigned char* oris, unsigned char* outs, int Ho, int Wo, int resume)
{
    const int j = blockIdx.y;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;          // group of PX pixels
    const long P = (long)Ho * Wo;
    if (q * PX >= P) return;
    const int i0 = FB.first[j], i1 = FB.first[j + 1];
    const unsigned char* in = (j == 0 && resume ? outs : oris) + (long)j * P * 3;
    unsigned char* out = outs + (long)j * P * 3;
    if (i0 == i1 && in == out) return;                             // in place, no face: nothing to do
    unsigned wv[PX_WORDS<PX>];
    load_px<PX>(in, q, wv);
    const int y = (int)((q * PX) / Wo), xb = (int)((q * PX) % Wo);
    paste_faces_px<PX>(crops + (long)i0 * Hc * Wc * 3, masks + (long)i0 * Hc * Wc, Hc, Wc, FB.a + i0, FB.box + i0, i1 - i0, xb, y, (unsigned char*)wv);
    store_px<PX>(out, q, wv);
}

// ---- paste-back of B generated frames into ONE image under ONE mask and ONE matrix (can_swap_pipeline_v2i.py:317-321: every frame is
// pasted into a fresh copy of the source image with the same mask_ori_float and source_M_c2o).  Per pixel the arithmetic of paste_kernel with
// mask_ori given.  Everything that does not depend on the frame is formed once per thread - the fixed-point coordinates, the tap weights (kept
// as fx, fy), the mask value, the image's pixels - and the thread then walks its group of frames (blockIdx.y), reading that frame's four crop
// taps only.  A pixel with mask 0 (v = 0 * res + 1 * ori = ori) or with all four taps outside the crop (res = 0: v = m * 0 + (1 - m) * ori,
// the same for every frame) never touches the crop; most of a 1080p frame is such pixels and is stored from registers, frame after frame.
// PX pixels of a row per thread: 8 (24 bytes, 8-byte aligned: one 16-byte and one 8-byte store) or 4 (12 bytes, as paste_batch_kernel); it
// loads the image beside the mask itself and stores through store_px.
template <int PX>
__global__ void __launch_bounds__(256) paste_shared_kernel(const unsigned char* __restrict__ crops, int Hc, int Wc, AffineInv A,
                                                           const float* __restrict__ mask_ori, const unsigned char* __restrict__ ori,
                                                           unsigned char* __restrict__ outs, int Ho, int Wo, int B, int frames_per_block)
{
    constexpr int NW = PX * 3 / 4;                                   // dwords of PX pixels
    const long q = (long)blockIdx.x * 256 + threadIdx.x;             // group of PX pixels of one row
    const long P = (long)Ho * Wo;
    if (q * PX >= P) return;
    const int f0 = blockIdx.y * frames_per_block, f1 = min(B, f0 + frames_per_block);
    unsigned base[NW];                                               // the image's bytes; for pixels that never read the crop: the result
    float m[PX];
    if constexpr (PX == 8) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint2 v = ((const uint2*)ori)[q * 3 + j];
            base[2 * j] = v.x; base[2 * j + 1] = v.y;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float4 v = ((const float4*)mask_ori)[q * 2 + j];
            m[4 * j] = v.x; m[4 * j + 1] = v.y; m[4 * j + 2] = v.z; m[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NW; ++j) base[j] = ((const unsigned*)ori)[q * NW + j];
#pragma unroll
        for (int k = 0; k < PX; ++k) m[k] = mask_ori[q * PX + k];
    }
    const int y = (int)((q * PX) / Wo), xb = (int)((q * PX) % Wo);
    int o00[PX], info[PX];      // the pixel's tap, packed (tap_pack)
    bool any = false;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        o00[k] = 0; info[k] = 0;
        if (m[k] == 0.f) continue;                                   // the original pixel
        const Tap t = tap_at(A, xb + k, y, Hc, Wc);
        if (t.outside) {                                             // res = 0 for every frame
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int by = k * 3 + c, sh = (by & 3) * 8;
                const float o = (float)((base[by >> 2] >> sh) & 0xffu);
                base[by >> 2] = (base[by >> 2] & ~(0xffu << sh)) | (blend_u8(m[k], 0, (1.f - m[k]) * o) << sh);
            }
            continue;
        }
        o00[k] = (int)t.o00;                                         // sx, sy >= -1 and inside the crop otherwise: fits (the launcher bounds Hc * Wc)
        info[k] = tap_pack(t);
        any = true;
    }
    if (!any) {                                                      // nothing of this group depends on the frame
        for (int f = f0; f < f1; ++f) store_px<PX>(outs + (long)f * P * 3, q, base);
        return;
    }
    for (int f = f0; f < f1; ++f) {
        const unsigned char* crop = crops + (long)f * Hc * Wc * 3;
        unsigned wv[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) wv[j] = base[j];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const Tap t = tap_unpack(o00[k], info[k]);
            if (t.outside) continue;
            int res[3];
            tap_u8x3(crop, Wc, t, res);
            const float mk = m[k], om = 1.f - mk;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int by = k * 3 + c, sh = (by & 3) * 8;
                const float o = (float)((base[by >> 2] >> sh) & 0xffu);
                wv[by >> 2] = (wv[by >> 2] & ~(0xffu << sh)) | (blend_u8(mk, res[c], om * o) << sh);
            }
        }
        store_px<PX>(outs + (long)f * P * 3, q, wv);
    }
}

// ---- F.interpolate(x, size=(H/2, W/2), mode="bilinear", align_corners=False) at exactly one half (can_swap_pipeline_v2i.py:294): the
// source coordinate of output i is 2 i + 0.5, so every weight is 1/2 * 1/2 and the result is the mean of a 2x2 block.  The order of the three
// additions is the one of the GPU kernel the reference runs, 0.25f * ((a + b) + (c + d)) (rows first); the products by 1/2 are exact.
__global__ void __launch_bounds__(256) resize_half_vec_kernel(const float* __restrict__ in, float* __restrict__ out, long planes, int Hd, int Wd)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;          // four output columns
    const int W4 = Wd / 4;
    if (i >= planes * Hd * W4) return;
    const long row = i / W4;                                       // plane * Hd + y
    const int x4 = (int)(i % W4);
    const float4* u = (const float4*)(in + row * 2 * (Wd * 2L)) + x4 * 2;
    const float4* l = (const float4*)(in + (row * 2 + 1) * (Wd * 2L)) + x4 * 2;
    const float4 u0 = u[0], u1 = u[1], l0 = l[0], l1 = l[1];
    float4 r;
    r.x = 0.25f * ((u0.x + u0.y) + (l0.x + l0.y)); r.y = 0.25f * ((u0.z + u0.w) + (l0.z + l0.w));
    r.z = 0.25f * ((u1.x + u1.y) + (l1.x + l1.y)); r.w = 0.25f * ((u1.z + u1.w) + (l1.z + l1.w));
    ((float4*)out)[i] = r;
}

__global__ void __launch_bounds__(256) resize_half_kernel(const float* __restrict__ in, float* __restrict__ out, long planes, int Hd, int Wd)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * Hd * Wd) return;
    const long row = i / Wd;
    const int x = (int)(i % Wd);
    const float* u = in + row * 2 * (Wd * 2L) + x * 2;
    const float* l = u + Wd * 2L;
    out[i] = 0.25f * ((u[0] + u[1]) + (l[0] + l[1]));
}

// float image (one channel) warped into the destination frame (prepare_paste_back, crop.py:515-521)
__global__ void __launch_bounds__(256) warp_f32_kernel(const float* __restrict__ src, int Hs, int Ws, AffineInv A, float* __restrict__ dst,
                                                       int Hd, int Wd)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Hd * Wd) return;
    const int y = (int)(i / Wd), x = (int)(i % Wd);
    dst[i] = tap_f32(src, Ws, tap_at(A, x, y, Hs, Ws));
}

// B matrices, inverted, in chunks of the 64 that one launch takes as kernel arguments: launch(first frame, frames, matrices) per chunk
template <typename F>
static int for_affine_batches(const double* M, int B, F launch)
{
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int nb = B - b0 < 64 ? B - b0 : 64;
        AffineBatch AB;
        for (int i = 0; i < nb; ++i) AB.a[i] = invert_affine(M + (long)(b0 + i) * 6);
        if (launch(b0, nb, AB)) return -1;
    }
    return 0;
}

int launch_paste(const unsigned char* crop, const float* mask_crop, const float* mask_ori, int Hc, int Wc, const double M[6],
                 const unsigned char* ori, unsigned char* out, int Ho, int Wo, hipStream_t st)
{
    const long n = (long)Ho * Wo;
    hipLaunchKernelGGL(paste_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, crop, mask_crop, mask_ori, Hc, Wc, invert_affine(M),
                       ori, out, Ho, Wo);
    LAUNCH_CHECK("paste");
    return 0;
}

int launch_warp_f32(const float* src, int Hs, int Ws, const double M[6], float* dst, int Hd, int Wd, hipStream_t st)
{
    const long n = (long)Hd * Wd;
    hipLaunchKernelGGL(warp_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, Hs, Ws, invert_affine(M), dst, Hd, Wd);
    LAUNCH_CHECK("warp_f32");
    return 0;
}

int launch_resize_half(const float* in, float* out, long planes, int H, int W, hipStream_t st)
{
    const int Hd = H / 2, Wd = W / 2;
    if (Wd % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0) {
        const long n = planes * Hd * (Wd / 4);
        hipLaunchKernelGGL(resize_half_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, planes, Hd, Wd);
    } else {
        const long n = planes * Hd * Wd;
        hipLaunchKernelGGL(resize_half_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, planes, Hd, Wd);
    }
    LAUNCH_CHECK("resize_half");
    return 0;
}

// B frames into one image: eight pixels per thread where rows and buffers allow 8-byte accesses, four pixels (dwords) otherwise; widths that are
// no multiple of 4 / buffers off a 4-byte boundary: the single-frame kernel per frame (same arithmetic; the kernel's packed-dword bookkeeping has
// no byte form).  The frame groups are grid rows, so B is not bound by a chunk size.
int launch_paste_shared(const unsigned char* crops, int Hc, int Wc, const float* mask_ori, const double M[6], const unsigned char* ori,
                        unsigned char* outs, int B, int Ho, int Wo, hipStream_t st)
{
    const long P = (long)Ho * Wo;
    const uintptr_t al = (uintptr_t)ori | (uintptr_t)outs;
    const int FPB = 8;                                               // frames a thread walks with its per-pixel state
    const dim3 groups(1, (unsigned)((B + FPB - 1) / FPB));
    if (Wo % 8 == 0 && (al & 7) == 0 && ((uintptr_t)mask_ori & 15) == 0) {
        hipLaunchKernelGGL(paste_shared_kernel<8>, dim3((unsigned)((P / 8 + 255) / 256), groups.y), dim3(256), 0, st, crops, Hc, Wc, invert_affine(M),
                           mask_ori, ori, outs, Ho, Wo, B, FPB);
        LAUNCH_CHECK("paste_shared");
    } else if (Wo % 4 == 0 && (al & 3) == 0) {
        hipLaunchKernelGGL(paste_shared_kernel<4>, dim3((unsigned)((P / 4 + 255) / 256), groups.y), dim3(256), 0, st, crops, Hc, Wc, invert_affine(M),
                           mask_ori, ori, outs, Ho, Wo, B, FPB);
        LAUNCH_CHECK("paste_shared");
    } else {
        for (int i = 0; i < B; ++i)
            if (launch_paste(crops + (long)i * Hc * Wc * 3, nullptr, mask_ori, Hc, Wc, M, ori, outs + (long)i * P * 3, Ho, Wo, st)) return -1;
    }
    return 0;
}

// Whether the batched paste kernels may move a thread's four pixels as three dwords (PX = 4): rows of a multiple of four pixels in buffers on a
// 4-byte boundary.  Otherwise PX = 1: one pixel per thread, byte by byte, the same values.
static bool wide_px(const unsigned char* oris, const unsigned char* outs, int Wo)
{
    return Wo % 4 == 0 && ((uintptr_t)oris & 3) == 0 && ((uintptr_t)outs & 3) == 0;
}

int launch_paste_batch(const unsigned char* crops, const float* masks, int Hc, int Wc, const double* M, const unsigned char* oris,
                       unsigned char* outs, int B, int Ho, int Wo, hipStream_t st)
{
    const long P = (long)Ho * Wo;
    const bool wide = wide_px(oris, outs, Wo);
    const dim3 grid((unsigned)(((wide ? P / 4 : P) + 255) / 256));
    return for_affine_batches(M, B, [&](int b0, int nb, const AffineBatch& AB) {
        const unsigned char *c = crops + (long)b0 * Hc * Wc * 3, *from = oris + (long)b0 * P * 3;
        const float* m = masks + (long)b0 * Hc * Wc;
        unsigned char* to = outs + (long)b0 * P * 3;
        if (wide) hipLaunchKernelGGL(paste_batch_kernel<4>, dim3(grid.x, nb), dim3(256), 0, st, c, m, Hc, Wc, AB, from, to, Ho, Wo);
        else hipLaunchKernelGGL(paste_batch_kernel<1>, dim3(grid.x, nb), dim3(256), 0, st, c, m, Hc, Wc, AB, from, to, Ho, Wo);
        LAUNCH_CHECK("paste_batch");
        return 0;
    });
}

// B faces into F frames, face b into frame frame_index[b] (non-decreasing, in [0, F): the caller checks), in the faces' order.  A launch takes up
// to FACES_PER_LAUNCH faces and as many frames; a frame whose faces do not fit is finished by the next launch, which reads what this one wrote
// (stream order).  outs == oris pastes in place.  The same launches at PX = 1 where wide_px refuses the dwords.
int launch_paste_faces(const unsigned char* crops, const float* masks, int Hc, int Wc, const double* M, const int* frame_index,
                       const unsigned char* oris, unsigned char* outs, int B, int F, int Ho, int Wo, hipStream_t st)
{
    const long P = (long)Ho * Wo, C = (long)Hc * Wc;
    const bool wide = wide_px(oris, outs, Wo);
    const unsigned blocks = (unsigned)(((wide ? P / 4 : P) + 255) / 256);
    constexpr int N = FACES_PER_LAUNCH;
    int b = 0, f = 0, resume = 0;
    while (f < F) {
        FaceBatch FB = {};
        const int b0 = b, f0 = f;
        int nb = 0, nf = 0, split = 0;
        while (nf < N && f0 + nf < F && !split) {
            int cnt = 0;                                              // faces of this frame not pasted yet
            while (b + cnt < B && frame_index[b + cnt] == f0 + nf) ++cnt;
            if (cnt && nb == N) break;                                // the launch is full: the frame goes to the next one as a whole
            const int take = cnt < N - nb ? cnt : N - nb;
            for (int i = 0; i < take; ++i, ++nb, ++b) {
                FB.a[nb] = invert_affine(M + (long)b * 6);
                face_box(FB.a[nb], Hc, Wc, Ho, Wo, FB.box[nb]);
            }
            FB.first[++nf] = nb;
            split = take < cnt;
        }
        if (nb || oris != outs) {
            const unsigned char* from = oris + (long)f0 * P * 3;
            unsigned char* to = outs + (long)f0 * P * 3;
            if (wide) hipLaunchKernelGGL(paste_faces_kernel<4>, dim3(blocks, nf), dim3(256), 0, st, crops + b0 * C * 3, masks + b0 * C, Hc, Wc, FB, from, to, Ho, Wo, resume);
            else hipLaunchKernelGGL(paste_faces_kernel<1>, dim3(blocks, nf), dim3(256), 0, st, crops + b0 * C * 3, masks + b0 * C, Hc, Wc, FB, from, to, Ho, Wo, resume);
            LAUNCH_CHECK("paste_faces");
        }
        f = f0 + nf - split;                                          // a split frame is frame 0 of the next launch, read from outs
        resume = split;
    }
    return 0;
}

// ---- the same with the matrices in device memory (cs_paste_back_faces_dev, include/canonswap_device_crop.h): M is B x 18 fp32 as cs_crop_lmk and
// cs_lmk_input write it, M_c2o = M + 18 b + 9.  What paste_faces_kernel gets as kernel arguments - a face's inverted matrix and its box - a
// workgroup forms itself: the faces of its frame in chunks of DEV_FACE_CHUNK, thread i of the chunk widens face i's six floats to double and runs
// invert_affine and face_box (affine_inv.h: the text launch_paste_faces runs on the host, so the AffineInv has the host form's bits) into LDS,
// once per workgroup; after the barrier every thread walks the chunk as paste_faces_kernel walks its range.  Nothing is staged in device
// memory, so two calls on two streams share nothing.  A face with status != 0 gets the empty box and is skipped like a face that does not
// reach the frame.  The faces come from device memory, so a frame's faces never have to be split over launches: only the frames' ranges are
// kernel arguments, DEV_FRAMES_PER_LAUNCH of them (absolute face numbers).  PX as in the host form: 4, or 1 where wide_px refuses the dwords.
// The pixel group and the face walk are written out here, not taken from load_px / store_px / paste_faces_px: through them this kernel measured
// 1.3 % (PX = 4) to 10 % (PX = 1) slower than this text on the same inputs.
constexpr int DEV_FRAMES_PER_LAUNCH = 48, DEV_FACE_CHUNK = 16;
struct FrameFaces { int first[DEV_FRAMES_PER_LAUNCH + 1]; };      // frame j of the launch owns faces first[j] .. first[j + 1] - 1

template <int PX>
__global__ void __launch_bounds__(256) paste_faces_dev_kernel(const unsigned char* __restrict__ crops, const float* __restrict__ masks, int Hc, int Wc,
                                                              const float* __restrict__ M, const int* __restrict__ status, FrameFaces FF,
                                                              const unsigned char* oris, unsigned char* outs, int Ho, int Wo)
{
    __shared__ AffineInv s_a[DEV_FACE_CHUNK];
    __shared__ int s_box[DEV_FACE_CHUNK][4];
    const int j = blockIdx.y, tid = threadIdx.x;
    const int i0 = FF.first[j], i1 = FF.first[j + 1];
    if (i0 == i1 && oris == outs) return;                          // in place, no face: nothing to do (the whole workgroup leaves)
    const long q = (long)blockIdx.x * 256 + tid;                   // group of PX pixels
    const long P = (long)Ho * Wo;
    const bool live = q * PX < P;                                  // the others only help to form the matrices and keep the barriers
    const unsigned char* in = oris + ((long)j * P + q * PX) * 3;
    unsigned char* out = outs + ((long)j * P + q * PX) * 3;
    unsigned wv[3] = {0u, 0u, 0u};
    unsigned char* px = (unsigned char*)wv;
    if (live) {
        if constexpr (PX == 4) { wv[0] = ((const unsigned*)in)[0]; wv[1] = ((const unsigned*)in)[1]; wv[2] = ((const unsigned*)in)[2]; }
        else { px[0] = in[0]; px[1] = in[1]; px[2] = in[2]; }
    }
    const int y = (int)((q * PX) / Wo), xb = (int)((q * PX) % Wo);
    for (int c0 = i0; c0 < i1; c0 += DEV_FACE_CHUNK) {
        const int nc = min(DEV_FACE_CHUNK, i1 - c0);
        __syncthreads();                                           // the chunk before has been read by everyone
        if (tid < nc) {
            const int b = c0 + tid;
            AffineInv A = {};
            int box[4] = {1, 1, 0, 0};                             // empty: a face that is not pasted
            if (!status || status[b] == 0) {
                const float* m = M + (long)b * 18 + 9;
                const double Md[6] = {(double)m[0], (double)m[1], (double)m[2], (double)m[3], (double)m[4], (double)m[5]};
                A = invert_affine(Md);
                face_box(A, Hc, Wc, Ho, Wo, box);
            }
            s_a[tid] = A;
#pragma unroll
            for (int k = 0; k < 4; ++k) s_box[tid][k] = box[k];
        }
        __syncthreads();
        if (!live) continue;
        for (int i = 0; i < nc; ++i) {
            if (y < s_box[i][1] || y > s_box[i][3] || xb + PX - 1 < s_box[i][0] || xb > s_box[i][2]) continue;
            paste_px<PX>(crops + (long)(c0 + i) * Hc * Wc * 3, masks + (long)(c0 + i) * Hc * Wc, Hc, Wc, s_a[i], xb, y, px);
        }
    }
    if (!live) return;
    if constexpr (PX == 4) { ((unsigned*)out)[0] = wv[0]; ((unsigned*)out)[1] = wv[1]; ((unsigned*)out)[2] = wv[2]; }
    else { out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; }
}

// frame_index is checked by the caller (non-decreasing, in [0, F)); B = 0: it is not read.  outs == oris pastes in place.
int launch_paste_faces_dev(const unsigned char* crops, const float* masks, int Hc, int Wc, const float* M, const int* status, const int* frame_index,
                           const unsigned char* oris, unsigned char* outs, int B, int F, int Ho, int Wo, hipStream_t st)
{
    const long P = (long)Ho * Wo;
    const bool wide = wide_px(oris, outs, Wo);
    const unsigned blocks = (unsigned)(((wide ? P / 4 : P) + 255) / 256);
    int b = 0;
    for (int f0 = 0; f0 < F; f0 += DEV_FRAMES_PER_LAUNCH) {
        const int nf = F - f0 < DEV_FRAMES_PER_LAUNCH ? F - f0 : DEV_FRAMES_PER_LAUNCH, b0 = b;
        FrameFaces FF = {};
        FF.first[0] = b;
        for (int j = 0; j < nf; ++j) {
            while (b < B && frame_index[b] == f0 + j) ++b;
            FF.first[j + 1] = b;
        }
        if (b == b0 && oris == outs) continue;                        // in place, no face in these frames
        const unsigned char* from = oris + (long)f0 * P * 3;
        unsigned char* to = outs + (long)f0 * P * 3;
        if (wide) hipLaunchKernelGGL(paste_faces_dev_kernel<4>, dim3(blocks, nf), dim3(256), 0, st, crops, masks, Hc, Wc, M, status, FF, from, to, Ho, Wo);
        else hipLaunchKernelGGL(paste_faces_dev_kernel<1>, dim3(blocks, nf), dim3(256), 0, st, crops, masks, Hc, Wc, M, status, FF, from, to, Ho, Wo);
        LAUNCH_CHECK("paste_faces_dev");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the crop itself
// crop_image's image step (src/utils/crop.py:429-455 as src/utils/cropper.py:196-209 calls it per frame): cv2.warpAffine(frame, M_o2c[:2],
// (dsize, dsize), INTER_LINEAR), BORDER_CONSTANT 0, for B frames in one launch; blockIdx.y = frame, the matrices are kernel arguments as in
// paste_batch_kernel.  Per pixel the arithmetic of paste_kernel without an original image.  The reads are a rotated gather of bytes that the L2
// serves (a crop row walks a slanted line through the frame, 4 x 3 bytes per pixel, neighbouring lanes on neighbouring pixels); what can be
// made wide is the store: a thread owns four consecutive crop pixels of a row = 12 bytes = three dwords, a wave's stores of one row are contiguous.
// STAGE != 0: the thread owns a 4 x 2 block and also writes what prepare_crops_kernel would make of it, from its registers - the crop is not
// read back: STAGE 2 (dsize 512): the two 2 x 2 means (a + b + c + d + 2) >> 2, / 255, as one float2 per channel of the NCHW fp32 input;
// STAGE 1 (dsize 256): / 255 only, one float4 per row and channel.  WIDE: crops on a 4-byte and I on a 16-byte boundary; otherwise the same
// values byte by byte and float by float (crop_store<STAGE, false>).  A template parameter, not crop_lmk_kernel's launch-uniform flag: with both
// stores in one body STAGE 1 takes 72 VGPRs, seven waves per SIMD, where the wide store alone takes 48 and runs eight.
struct CropSource { int frame[64]; };         // crop n of a launch is cut from frame[n] of `frames` (several faces of one frame: the same entry)

template <int STAGE, bool WIDE>
__global__ void __launch_bounds__(256) crop_batch_kernel(const unsigned char* __restrict__ frames, int Ho, int Wo, AffineBatch AB, CropSource CS,
                                                         int dsize, unsigned char* __restrict__ crops, float* __restrict__ I)
{
    constexpr int ROWS = STAGE ? 2 : 1;
    const int n = blockIdx.y;
    const int gw = dsize >> 2;                                        // groups of four pixels in a row
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= gw * (dsize / ROWS)) return;
    const int yb = (g / gw) * ROWS, xb = (g % gw) * 4;
    const AffineInv& A = AB.a[n];
    int v[ROWS][4][3];
    crop_read<ROWS>(frames + (long)CS.frame[n] * Ho * Wo * 3, Ho, Wo, A, xb, yb, v);      // warp_taps.h, as crop_store
    crop_store<STAGE, WIDE>(v, n, yb, xb, dsize, crops, I);          // the crop's bytes and, with STAGE, the staged input
}

// dsize: a multiple of 4 (the caller checks); I != nullptr: dsize 256 or 512.  B is chunked by the 64 matrices of a launch, so it is not bound
// by anything.  frame_index: crop b is cut from frame frame_index[b] (cs_crop_faces); nullptr: from frame b (cs_crop_frames).  Buffers that do
// not allow the wide stores (a crop buffer off a 4-byte, an I off a 16-byte boundary): the same launches, storing narrow.
int launch_crop_batch(const unsigned char* frames, int Ho, int Wo, const double* M, const int* frame_index, int dsize, unsigned char* crops, float* I,
                      int B, hipStream_t st)
{
    const long C = (long)dsize * dsize * 3;
    const bool wide = ((uintptr_t)crops & 3) == 0 && ((uintptr_t)I & 15) == 0;      // rows are multiples of four pixels: aligned with the base
    const int stage = I ? dsize / 256 : 0, rows = stage ? 2 : 1;
    const dim3 grid((unsigned)(((long)(dsize / 4) * (dsize / rows) + 255) / 256));
    const auto kernel = stage == 2 ? (wide ? crop_batch_kernel<2, true> : crop_batch_kernel<2, false>)
                      : stage == 1 ? (wide ? crop_batch_kernel<1, true> : crop_batch_kernel<1, false>)
                                   : (wide ? crop_batch_kernel<0, true> : crop_batch_kernel<0, false>);
    return for_affine_batches(M, B, [&](int b0, int nb, const AffineBatch& AB) {
        CropSource CS;
        for (int i = 0; i < 64; ++i) CS.frame[i] = i < nb ? (frame_index ? frame_index[b0 + i] : b0 + i) : 0;
        unsigned char* c = crops + b0 * C;
        float* Ib = I ? I + (long)b0 * 3 * 256 * 256 : nullptr;
        hipLaunchKernelGGL(kernel, dim3(grid.x, nb), dim3(256), 0, st, frames, Ho, Wo, AB, CS, dsize, c, Ib);
        LAUNCH_CHECK("crop_batch");
        return 0;
    });
}

// ---------------------------------------------------------------------------------------------- face mask from the parser's logits
// The torch lines between SegFormer and SoftErosion (can_swap_pipeline_e2e.py:183-190, can_swap_pipeline_v2i.py:76-83) in one launch for B frames:
//   up = F.interpolate(logits, size=(S h, S w), mode="bilinear", align_corners=False);  labels = up.argmax(1);  mask = isin(labels, valid)
// The up-sampled logits exist in registers only.  A thread owns the S x S output pixels of ONE source cell (yc, xc), aligned to it, and walks the
// classes with S x S running maxima and labels.  Output column S xc + k has the source coordinate src = (S xc + k + 0.5) / S - 0.5 clamped below at 0,
// i0 = floor(src), i1 = min(i0 + 1, w - 1), l1 = src - i0, l0 = 1 - l1 (exact in fp32 for S = 1, 2, 4): i0 is xc - 1 for k < S / 2 and xc otherwise,
// so per class the block reads the 3 x 3 cells about (yc, xc), indices clamped to the plane, and takes taps (TAP0(k), TAP0(k) + 1) of them.
// At the low border the clamp of src gives i0 = 0 with l1 = 0, where this reads cell 0 for both taps: l0 a + 0 b is a either way (finite logits).
// The value is formed in the expression order of torch's GPU kernel (upsample_bilinear2d_out_frame), every product and sum rounded (no
// contraction in this file):   v = hl0 * (wl0 * a + wl1 * b) + hl1 * (wl0 * c + wl1 * d)
// so the two parentheses, which depend on the tap row and the column only, are formed once per row (3 S of them) and shared by the S output rows.
// argmax: classes in order, strict >: the first maximum, as torch.  NaN logits are outside the contract.
// Lanes of a wave are 64 consecutive cells of a row: every load is contiguous along w, the three columns and three rows of neighbouring threads
// and waves (a workgroup is 64 x 4 cells) come from the L1 / L2, so HBM sees each logit about once.  The next class's nine cells are fetched
// while this one's are used.  Per output row the block's S bytes go out as one S-byte store (S = 4: aligned dwords, 256 contiguous bytes per wave),
// byte by byte where a buffer is not S-byte aligned.
template <int S>
__device__ __forceinline__ void store_packed(unsigned char* p, unsigned v, int wide)
{
    if (S == 4 && wide) *(unsigned*)p = v;
    else if (S == 2 && wide) *(unsigned short*)p = (unsigned short)v;
    else {
#pragma unroll
        for (int k = 0; k < S; ++k) p[k] = (unsigned char)(v >> (8 * k));
    }
}

// the 3 x 3 cells of one class about the thread's cell: cls is the class's plane, off the cells' offsets inside a plane, already clamped to
// it (32-bit: the launcher bounds h * w)
__device__ __forceinline__ void face_taps(const float* __restrict__ cls, const unsigned (&off)[3][3], float (&t)[3][3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) t[r][q] = cls[off[r][q]];
}

// class c's S x S up-sampled values from its cells, in the expression order stated above, into the running first maximum
template <int S>
__device__ __forceinline__ void face_class(const float (&t)[3][3], int c, const float (&wl0)[S], const float (&wl1)[S], const float (&hl0)[S],
                                           const float (&hl1)[S], float (&best)[S][S], int (&lab)[S][S])
{
    float hx[3][S];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int q = k < S / 2 ? 0 : 1;                            // TAP0(k)
            hx[r][k] = wl0[k] * t[r][q] + wl1[k] * t[r][q + 1];
        }
#pragma unroll
    for (int ky = 0; ky < S; ++ky) {
        const int r = ky < S / 2 ? 0 : 1;
#pragma unroll
        for (int kx = 0; kx < S; ++kx) {
            const float v = hl0[ky] * hx[r][kx] + hl1[ky] * hx[r + 1][kx];
            if (v > best[ky][kx]) { best[ky][kx] = v; lab[ky][kx] = c; }
        }
    }
}

// grid: (tiles of 64 x 4 cells, frames)
template <int S>
__global__ void __launch_bounds__(256) face_mask_kernel(const float* __restrict__ logits, int C, int h, int w, int tiles_x, unsigned valid_bits,
                                                        unsigned char* __restrict__ masks, unsigned char* __restrict__ labels, int wide)
{
    const long n = blockIdx.y;
    const int xc = (int)(blockIdx.x % tiles_x) * 64 + (threadIdx.x & 63), yc = (int)(blockIdx.x / tiles_x) * 4 + (threadIdx.x >> 6);
    if (xc >= w || yc >= h) return;
    float wl0[S], wl1[S], hl0[S], hl1[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const float sx = fmaxf(((float)(xc * S + k) + 0.5f) / (float)S - 0.5f, 0.f), sy = fmaxf(((float)(yc * S + k) + 0.5f) / (float)S - 0.5f, 0.f);
        wl1[k] = sx - floorf(sx); wl0[k] = 1.f - wl1[k];
        hl1[k] = sy - floorf(sy); hl0[k] = 1.f - hl1[k];
    }
    const long plane = (long)h * w;
    const int xo[3] = {max(xc - 1, 0), xc, min(xc + 1, w - 1)}, yo[3] = {max(yc - 1, 0), yc, min(yc + 1, h - 1)};
    unsigned off[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) off[i / 3][i % 3] = (unsigned)yo[i / 3] * (unsigned)w + (unsigned)xo[i % 3];
    const float* src = logits + n * C * plane;
    float best[S][S], ta[3][3], tb[3][3];
    int lab[S][S];
#pragma unroll
    for (int i = 0; i < S * S; ++i) { best[i / S][i % S] = -INFINITY; lab[i / S][i % S] = 0; }
    // two classes per trip, their cells in two register sets that are fetched one class ahead of their use; a fetch past the last class reads
    // the last class again (no branch, nothing out of bounds)
    face_taps(src, off, ta);
    for (int c = 0; c < C; c += 2) {
        face_taps(src + min(c + 1, C - 1) * plane, off, tb);
        face_class<S>(ta, c, wl0, wl1, hl0, hl1, best, lab);
        face_taps(src + min(c + 2, C - 1) * plane, off, ta);
        if (c + 1 < C) face_class<S>(tb, c + 1, wl0, wl1, hl0, hl1, best, lab);
    }
    const int W = w * S;
#pragma unroll
    for (int ky = 0; ky < S; ++ky) {
        unsigned lw = 0, mw = 0;
#pragma unroll
        for (int kx = 0; kx < S; ++kx) {
            lw |= (unsigned)lab[ky][kx] << (8 * kx);
            mw |= ((valid_bits >> lab[ky][kx]) & 1u) << (8 * kx);
        }
        const long o = ((n * h + yc) * S + ky) * W + (long)xc * S;
        if (masks) store_packed<S>(masks + o, mw, wide);
        if (labels) store_packed<S>(labels + o, lw, wide);
    }
}

// scale 1, 2 or 4, 1 <= C <= 32, B, h, w >= 1 and an output given: the caller checks (cs_face_masks).  Frame, class and output offsets are 64-bit,
// a cell's offset inside its class plane is 32-bit: h * w < 2^30, which also bounds a frame's tiles.  Frames are grid rows,
// 65535 of them per launch, so B is not bound by anything.
int launch_face_masks(const float* logits, int B, int C, int h, int w, int scale, unsigned valid_bits, unsigned char* masks, unsigned char* labels,
                      hipStream_t st)
{
    const int tiles_x = (w + 63) / 64;
    const long tiles = (long)tiles_x * ((h + 3) / 4);
    if ((long)h * w >= (1L << 30)) { cs_set_error("face_masks: %dx%d logits: a class plane must hold fewer than 2^30 cells", h, w); return -1; }
    const int wide = (((uintptr_t)masks | (uintptr_t)labels) & (uintptr_t)(scale - 1)) == 0;
    const long in_frame = (long)C * h * w, out_frame = (long)h * scale * w * scale;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const dim3 grid((unsigned)tiles, (unsigned)(B - b0 < 65535 ? B - b0 : 65535)), block(256);
        const float* lg = logits + b0 * in_frame;
        unsigned char* m = masks ? masks + b0 * out_frame : nullptr;
        unsigned char* l = labels ? labels + b0 * out_frame : nullptr;
        if (scale == 4) hipLaunchKernelGGL(face_mask_kernel<4>, grid, block, 0, st, lg, C, h, w, tiles_x, valid_bits, m, l, wide);
        else if (scale == 2) hipLaunchKernelGGL(face_mask_kernel<2>, grid, block, 0, st, lg, C, h, w, tiles_x, valid_bits, m, l, wide);
        else hipLaunchKernelGGL(face_mask_kernel<1>, grid, block, 0, st, lg, C, h, w, tiles_x, valid_bits, m, l, wide);
        LAUNCH_CHECK("face_masks");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the parser's input
// What both pipelines do to a crop before SegFormer sees it (can_swap_pipeline_e2e.py:171 + :180, can_swap_pipeline_v2i.py:73: cv2.resize to
// 256 x 256, then SegformerImageProcessor of transformers 4.38: PIL resize to 512 x 512 BILINEAR, rescale, normalize, HWC -> CHW) in one launch
// for B crops, in integers:
//   HALVE: x = (a + b + c + d + 2) >> 2 of each 2 x 2 block of the crop (cv2.resize by exactly one half, as prepare_crops_kernel), else x = the crop;
//   PIL's Resample.c by exactly 2 (coefficients 0.75 / 0.25, 1.0 at both ends, exact in its 22-bit fixed point), the horizontal pass FIRST and
//   its result rounded to uint8, the vertical pass on that; one axis pass n -> 2 n:
//     out[2 j] = (3 in[j] + in[max(j - 1, 0)] + 2) >> 2,   out[2 j + 1] = (3 in[j] + in[min(j + 1, n - 1)] + 2) >> 2;
//   pixel_values[c][y][x] = lut[c][byte]: rescale + normalize are a function of one byte per channel, tabulated on the host with the
//   processor's own numpy lines (tail.parser_lut).  Nothing is computed in float here.
// A workgroup owns 128 x 32 output pixels = 64 x 16 source pixels.  It stages those with a one-sample halo, indices clamped to the image (the
// clamp is the filter's own border rule: a clamped neighbour equals the sample, (3 a + a + 2) >> 2 = a), filters every staged row horizontally
// ONCE into LDS as bytes, one plane per channel (18 rows: the two output rows of a source row and its neighbours' share them), and then a
// thread owns four consecutive output pixels of four output rows: per row and channel one dword of each of the two filtered rows it blends,
// four table reads from LDS and one 16-byte store - the 32 lanes of a half-wave store 512 contiguous bytes of a plane's row.  The uint8
// image goes out as three dwords per thread and row.  No intermediate in global memory.
template <bool HALVE>
__global__ void __launch_bounds__(256) parser_input_kernel(const unsigned char* __restrict__ crops, int Hc, int Wc, const float* __restrict__ lut,
                                                           float* __restrict__ pv, unsigned char* __restrict__ u8, int tiles_x, int wide_f, int wide_u)
{
    constexpr int SX = 64, SY = 16, LR = SY + 2, SROW = (SX + 2) * 3, NS = LR * SROW, HW = SX * 2 / 4;
    __shared__ float tab[3 * 256];
    __shared__ unsigned char src[NS];
    __shared__ unsigned hf[3][LR][HW];
    const long n = blockIdx.y;
    const int h = HALVE ? Hc >> 1 : Hc, w = HALVE ? Wc >> 1 : Wc, Ho = 2 * h, Wo = 2 * w;
    const int sx0 = (int)(blockIdx.x % tiles_x) * SX, sy0 = (int)(blockIdx.x / tiles_x) * SY;
    const unsigned char* in = crops + n * Hc * Wc * 3;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = lut[i];
    for (int i = threadIdx.x; i < NS; i += 256) {                       // source tile + halo, interleaved as in memory
        const int row = i / SROW, b = i % SROW, col = b / 3, c = b % 3;
        const int gy = min(max(sy0 - 1 + row, 0), h - 1), gx = min(max(sx0 - 1 + col, 0), w - 1);
        int v;
        if (HALVE) {
            const unsigned char* p = in + ((long)(2 * gy) * Wc + 2 * gx) * 3 + c;
            v = (p[0] + p[3] + p[(long)Wc * 3] + p[(long)Wc * 3 + 3] + 2) >> 2;
        } else {
            v = in[((long)gy * Wc + gx) * 3 + c];
        }
        src[i] = (unsigned char)v;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 3 * LR * HW; q += 256) {              // horizontal pass: four output columns = two source columns per dword
        const int t = q % HW, row = (q / HW) % LR, c = q / (HW * LR);
        const unsigned char* p = src + row * SROW + 2 * t * 3 + c;       // staged columns 2 t .. 2 t + 3 = source columns 2 t - 1 .. 2 t + 2 of the tile
        const unsigned p0 = p[0], p1 = p[3], p2 = p[6], p3 = p[9];
        hf[c][row][t] = ((3 * p1 + p0 + 2) >> 2) | ((3 * p1 + p2 + 2) >> 2) << 8 | ((3 * p2 + p1 + 2) >> 2) << 16 | ((3 * p2 + p3 + 2) >> 2) << 24;
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = 2 * sx0 + 4 * tx;
    if (x >= Wo) return;
    const int nx = min(4, Wo - x);
    unsigned R[4][3];                                                   // filtered rows of source rows 2 ty - 1 .. 2 ty + 2 of the tile
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = hf[c][2 * ty + r][tx];
    const long plane = (long)Ho * Wo;
#pragma unroll
    for (int o = 0; o < 4; ++o) {                                       // output row 2 j + (o & 1) of source row j = 2 ty + (o >> 1): 3 j's row + its neighbour's
        const int y = 2 * (sy0 + 2 * ty) + o;
        if (y >= Ho) break;
        const int ra = (o >> 1) + 1, rb = (o & 1) ? ra + 1 : ra - 1;
        unsigned v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = (3 * ((R[ra][c] >> (8 * k)) & 255u) + ((R[rb][c] >> (8 * k)) & 255u) + 2) >> 2;
        if (pv) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* d = pv + (n * 3 + c) * plane + (long)y * Wo + x;
                const float4 f = make_float4(tab[c * 256 + v[c][0]], tab[c * 256 + v[c][1]], tab[c * 256 + v[c][2]], tab[c * 256 + v[c][3]]);
                if (wide_f) *(float4*)d = f;                            // Wo % 4 == 0: the group is whole
                else {
                    d[0] = f.x;
                    if (nx > 1) d[1] = f.y;
                    if (nx > 2) d[2] = f.z;
                    if (nx > 3) d[3] = f.w;
                }
            }
        }
        if (u8) {
            unsigned char* d = u8 + ((n * Ho + y) * Wo + x) * 3;
            if (wide_u) {
                unsigned wv[3] = {0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 12; ++j) wv[j >> 2] |= v[j % 3][j / 3] << ((j & 3) * 8);
                unsigned* dw = (unsigned*)d;
                dw[0] = wv[0]; dw[1] = wv[1]; dw[2] = wv[2];
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) if (j / 3 < nx) d[j] = (unsigned char)v[j % 3][j / 3];
            }
        }
    }
}

// B, Hc, Wc >= 1, even with halve, an output given, output sides <= 16384: the caller checks (cs_parser_input).  Frame and plane offsets are
// 64-bit; frames are grid rows, 65535 of them per launch, so B is not bound by anything.  The wide stores need whole groups of four
// pixels (Wo % 4 == 0) and aligned buffers; everything else takes element stores with the same values.
int launch_parser_input(const unsigned char* crops, int B, int Hc, int Wc, int halve, const float* lut, float* pv, unsigned char* u8, hipStream_t st)
{
    const int h = halve ? Hc / 2 : Hc, w = halve ? Wc / 2 : Wc, Ho = 2 * h, Wo = 2 * w;
    const int tiles_x = (w + 63) / 64, tiles = tiles_x * ((h + 15) / 16);
    const int wide_f = Wo % 4 == 0 && ((uintptr_t)pv & 15) == 0, wide_u = Wo % 4 == 0 && ((uintptr_t)u8 & 3) == 0;
    const long in_frame = (long)Hc * Wc * 3, out_frame = (long)Ho * Wo * 3;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const dim3 grid((unsigned)tiles, (unsigned)(B - b0 < 65535 ? B - b0 : 65535)), block(256);
        const unsigned char* c = crops + b0 * in_frame;
        float* p = pv ? pv + b0 * out_frame : nullptr;
        unsigned char* u = u8 ? u8 + b0 * out_frame : nullptr;
        if (halve) hipLaunchKernelGGL(parser_input_kernel<true>, grid, block, 0, st, c, Hc, Wc, lut, p, u, tiles_x, wide_f, wide_u);
        else hipLaunchKernelGGL(parser_input_kernel<false>, grid, block, 0, st, c, Hc, Wc, lut, p, u, tiles_x, wide_f, wide_u);
        LAUNCH_CHECK("parser_input");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the side-by-side ("concat") frame
// concat_frames of src/utils/video.py:84-109 (src/can_swap_pipeline_e2e.py:290: driving | rec_can | I_can | I_p; src/can_swap_pipeline_v2i.py:328:
// driving | I_can | I_p) for B frames in one launch: P panels, each brought to S x S uint8, side by side in out (B, S, P S, 3).  Panel kinds:
//   0  u8 HWC S x S: copied (cv2.resize to the size the image has is the identity);
//   1  u8 HWC S/2 x S/2: cv2.resize(img, (S, S)), INTER_LINEAR, OpenCV's 8-bit path (11-bit coefficients: at exactly x2 the weights are 512 and
//      1536 of 2048).  Horizontal pass into int32: H[2j] = 512 s[j-1] + 1536 s[j], H[2j+1] = 1536 s[j] + 512 s[j+1], a tap beyond either border
//      replaced by the border sample (2048 s[0], 2048 s[w-1]).  Vertical pass: row 2i from rows (max(i-1, 0), i) with (b0, b1) = (512, 1536),
//      row 2i+1 from rows (i, min(i+1, h-1)) with (1536, 512); dst = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2, truncations and all.
//   2  u8 HWC S x S: cv2.resize to one half first, (a + b + c + d + 2) >> 2 per 2 x 2 block (can_swap_pipeline_e2e.py:171: the pipeline's driving
//      crop is the halved 512 crop; parser_input_kernel's HALVE), then kind 1, with no half-size image in memory;
//   3  fp32 CHW 3 x S x S: parse_output (can_swap_e2e.py:314-322), pack_u8_kernel's expression: clip(x, 0, 1) * 255, clip(., 0, 255), truncate.
// PARITY UNPINNED: kinds 1 and 2 restate OpenCV's published arithmetic (tests/concat_ref.py is the same restatement in numpy); no vectors of
// cv2's own were at hand.
// A thread owns four consecutive pixels of one panel row: 12 output bytes, three dword stores, consecutive threads consecutive addresses (the
// output row runs through the panels, so thread t of a frame writes bytes 12 t ... 12 t + 11 of it).  At S = 512 a panel row is two waves: no
// wave straddles two panels, the branch on the kind is uniform.  Kind 3 reads one float4 per channel plane, the uint8 kinds aligned dwords.
// Purely bandwidth bound (e2e arrangement at B = 64: 0.65 GB read, 0.2 GB written); no LDS, no scratch.
struct ConcatPanels {
    const unsigned char* ptr[4];      // the panel's first image
    long step[4];                     // bytes from one frame's image to the next; 0: one image shared by all frames
    uintptr_t lo[4], hi[4];           // the aligned dwords that hold the first and the last byte of the panel's buffer: uint8 loads stay between them
    int kind[4];
    int vec[4];                       // kind 3: the planes are 16-byte aligned, float4 loads
};

// N bytes from address a as N / 4 dwords: aligned dword loads, funnel-shifted.  The dword addresses are clamped to [lo, hi], so a neighbour
// column beyond the image's border - whose value the caller replaces by the border sample - never reads outside the panel's buffer.
template <int N> __device__ __forceinline__ void load_bytes(uintptr_t a, uintptr_t lo, uintptr_t hi, unsigned (&d)[N / 4])
{
    const unsigned sh = 8u * (unsigned)(a & 3);
    const uintptr_t q = a & ~(uintptr_t)3;
    unsigned w[N / 4 + 1];
#pragma unroll
    for (int k = 0; k < N / 4; ++k) w[k] = *(const unsigned*)min(max(q + 4 * k, lo), hi);
    w[N / 4] = sh ? *(const unsigned*)min(max(q + N, lo), hi) : 0u;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) d[k] = sh ? (w[k] >> sh) | (w[k + 1] << (32u - sh)) : w[k];
}

__device__ __forceinline__ int byte_of(const unsigned* d, int k) { return (int)((d[k >> 2] >> (8 * (k & 3))) & 255u); }

// (H >> 4) of the horizontal pass for the thread's four output pixels (x 3 channels, in output byte order) of half-size row r: source
// columns 2g - 1 .. 2g + 2, the first / last replaced by its neighbour at the image's border.  HALVE: the half-size row is the 2 x 2 mean of
// rows 2r, 2r + 1 of the S x S image.
template <bool HALVE>
__device__ __forceinline__ void concat_hrow(const unsigned char* img, int r, int g, int S, uintptr_t lo, uintptr_t hi, int (&hq)[12])
{
    int s[4][3];
    if (HALVE) {
        unsigned a[6], b[6];
        const uintptr_t p = (uintptr_t)img + ((long)(2 * r) * S + 4 * g - 2) * 3;
        load_bytes<24>(p, lo, hi, a);
        load_bytes<24>(p + (long)S * 3, lo, hi, b);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[k][c] = (byte_of(a, 6 * k + c) + byte_of(a, 6 * k + 3 + c) + byte_of(b, 6 * k + c) + byte_of(b, 6 * k + 3 + c) + 2) >> 2;
    } else {
        unsigned a[3];
        load_bytes<12>((uintptr_t)img + ((long)r * (S >> 1) + 2 * g - 1) * 3, lo, hi, a);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[k][c] = byte_of(a, 3 * k + c);
    }
    const bool first = g == 0, last = g == (S >> 2) - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s0 = first ? s[1][c] : s[0][c], s1 = s[1][c], s2 = s[2][c], s3 = last ? s[2][c] : s[3][c];
        hq[c] = (512 * s0 + 1536 * s1) >> 4;
        hq[3 + c] = (1536 * s1 + 512 * s2) >> 4;
        hq[6 + c] = (512 * s1 + 1536 * s2) >> 4;
        hq[9 + c] = (1536 * s2 + 512 * s3) >> 4;
    }
}

__device__ __forceinline__ unsigned pack_byte(float v)      // pack_u8_kernel's expression (kernels.hip)
{
    v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (unsigned)(uint8_t)v;
}

__global__ void __launch_bounds__(256) concat_frames_kernel(ConcatPanels pn, int P, int S, unsigned char* __restrict__ out, int wide_out)
{
    const int G = S >> 2, PG = P * G;                                   // groups of four pixels per panel row, per output row
    const long per_frame = (long)S * PG;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= per_frame) return;
    const long n = blockIdx.y;
    const int y = (int)(t / PG), gr = (int)(t % PG), p = gr / G, g = gr % G;
    const unsigned char* img = pn.ptr[0] + n * pn.step[0];
    uintptr_t lo = pn.lo[0], hi = pn.hi[0];
    int kind = pn.kind[0], vec = pn.vec[0];
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (p == q) { img = pn.ptr[q] + n * pn.step[q]; lo = pn.lo[q]; hi = pn.hi[q]; kind = pn.kind[q]; vec = pn.vec[q]; }
    unsigned o[3];
    if (kind == 0) {
        load_bytes<12>((uintptr_t)img + ((long)y * S + 4 * g) * 3, lo, hi, o);
    } else if (kind == 3) {
        const float* f = (const float*)img + (long)y * S + 4 * g;
        const long plane = (long)S * S;
        unsigned v[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 x;
            if (vec) x = *(const float4*)(f + c * plane);
            else x = make_float4(f[c * plane], f[c * plane + 1], f[c * plane + 2], f[c * plane + 3]);
            v[c] = pack_byte(x.x); v[3 + c] = pack_byte(x.y); v[6 + c] = pack_byte(x.z); v[9 + c] = pack_byte(x.w);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = v[4 * k] | v[4 * k + 1] << 8 | v[4 * k + 2] << 16 | v[4 * k + 3] << 24;
    } else {
        const int h = S >> 1, i = y >> 1, odd = y & 1;
        const int r0 = odd ? i : max(i - 1, 0), r1 = odd ? min(i + 1, h - 1) : i, b0 = odd ? 1536 : 512, b1 = 2048 - b0;
        int h0[12], h1[12];
        if (kind == 2) { concat_hrow<true>(img, r0, g, S, lo, hi, h0); concat_hrow<true>(img, r1, g, S, lo, hi, h1); }
        else { concat_hrow<false>(img, r0, g, S, lo, hi, h0); concat_hrow<false>(img, r1, g, S, lo, hi, h1); }
        o[0] = o[1] = o[2] = 0u;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k >> 2] |= (unsigned)((((b0 * h0[k]) >> 16) + ((b1 * h1[k]) >> 16) + 2) >> 2) << (8 * (k & 3));
    }
    unsigned char* d = out + (n * per_frame + t) * 12;
    if (wide_out) {
        unsigned* dw = (unsigned*)d;
        dw[0] = o[0]; dw[1] = o[1]; dw[2] = o[2];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) d[k] = (unsigned char)byte_of(o, k);
    }
}

// B >= 1, 1 <= P <= 4, S a multiple of 4 in [4, 16384], kinds in 0..3, no NULL pointer: the caller checks (cs_concat_frames).  Frames are
// grid rows, 65535 of them per launch; every offset is 64-bit.  Buffers at any address: unaligned uint8 panels are read through the
// funnel shift, an fp32 panel off 16 bytes or an out off 4 bytes takes element accesses with the same values.
int launch_concat_frames(const void* const* panels, const int* kinds, const int* shared, int B, int P, int S, unsigned char* out, hipStream_t st)
{
    ConcatPanels pn = {};
    const long px = (long)S * S;
    long img[4] = {0, 0, 0, 0};
    for (int p = 0; p < P; ++p) {
        img[p] = kinds[p] == 1 ? px * 3 / 4 : kinds[p] == 3 ? px * 12 : px * 3;
        const uintptr_t a = (uintptr_t)panels[p];
        pn.step[p] = shared[p] ? 0 : img[p];
        pn.lo[p] = a & ~(uintptr_t)3;
        pn.hi[p] = (a + (uintptr_t)(shared[p] ? img[p] : (long)B * img[p]) - 1) & ~(uintptr_t)3;
        pn.kind[p] = kinds[p];
        pn.vec[p] = (a & 15) == 0;
    }
    const long per_frame = px / 4 * P;
    const int wide_out = ((uintptr_t)out & 3) == 0;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        for (int p = 0; p < P; ++p) pn.ptr[p] = (const unsigned char*)panels[p] + (long)b0 * pn.step[p];
        const dim3 grid((unsigned)((per_frame + 255) / 256), (unsigned)(B - b0 < 65535 ? B - b0 : 65535)), block(256);
        hipLaunchKernelGGL(concat_frames_kernel, grid, block, 0, st, pn, P, S, out + (long)b0 * per_frame * 12, wide_out);
        LAUNCH_CHECK("concat_frames");
    }
    return 0;
}
