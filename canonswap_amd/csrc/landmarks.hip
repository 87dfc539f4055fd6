// The two sides of the landmark network (src/utils/human_landmark_runner.py:60-85), on the device: tracked landmarks -> the crop's matrices, the crop
// and the network's input (cs_lmk_input, lines 62 and 76) and the network's points -> landmarks in the frame (cs_lmk_decode, lines 82-83).  The
// network itself stays the caller's.  With both on the device the cropper's per-frame loop (src/utils/cropper.py:186-193: frame k is cropped around
// the landmarks of frame k - 1) needs nothing from the host, and the steps of a batch of frames are enqueued in one go.  The third kernel here
// is the chains' crop from the same landmarks (cs_crop_lmk, include/canonswap_device_crop.h): the same head, crop_image's parameters, the chains'
// staging.
//
// Both kernels restate numpy / OpenCV lines whose every operation is rounded on its own: no FMA contraction in this translation unit (the pragma
// below, as in detect.hip and imgops.hip), and no fmaf / __fma_rn anywhere in it or in the headers it includes.  fp32 and fp64 `/` and sqrt are
// correctly rounded by default; the file is not compiled with any fast-math flag (_build.HIPCC_FLAGS).
#include "common.h"
#include "../../include/canonswap_landmarks.h"

#pragma clang fp contract(off)

#include "warp_taps.h"
#include "lmk_geometry.h"

#define LAUNCH_CHECK(name)                                                                       \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) { cs_set_error(name " launch: %s", hipGetErrorString(_e)); return -1; } \
    } while (0)

extern "C" int cs_lmk_abi_version(void) { return CS_LMK_ABI_VERSION; }

// ---------------------------------------------------------------------------------------------- landmarks -> matrices, crop, network input
// ONE kernel, not a geometry kernel and a crop kernel: the loop this serves is serial over the frames and launch bound (a step is this launch,
// the network, the decode), so a second launch per step costs more than what it would save - the geometry is 2 N floats (1.6 KB at 203 points,
// from the L2 after the first workgroup) and a few hundred flops, which wave 0 of every tile's workgroup recomputes while the other three wait
// at one barrier.  The 64 lanes of that wave share the N points (lmk_geometry with LmkWave): lane l walks points l, l + 64, ..., sums are joined by
// a butterfly in the fixed order 32, 16, 8, 4, 2, 1, extrema are order free - no atomics, the same bits whatever the schedule, and the same bits
// in every workgroup of a face.  M is written by tile 0's workgroup only.
//
// status is read on entry by every workgroup of the face and written by tile 0's, only where the geometry refuses the face and the entry value
// was 0.  Both are relaxed atomic accesses of one int (a plain vector load and store on this hardware), so a reader sees the old or the new value
// whole; a workgroup that reads the new one finds the face refused either way - it would have recomputed the same refusal itself - so what it
// does is the same on both sides of the store.
//
// A thread owns four consecutive crop pixels of a row, as crop_batch_kernel does: per channel one float4 of inp, and 12 bytes = three dwords of
// the optional uint8 crop.  A refused face writes zeros and forms no tap at all: no coordinate, no address, no read of the frame.
struct LmkWave {
    __device__ double sum(double v) const
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
        return v;
    }
    __device__ float min(float v) const
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
        return v;
    }
    __device__ float max(float v) const
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        return v;
    }
    __device__ int any(int v) const { return __any(v); }
};

struct LmkInput {
    int frame[64];                     // face n of the launch is cut from frame[n] (checked on the host: in [0, F))
    cs_lmk_layout L;
    int Ho, Wo, N, dsize, flag_do_rot, status_mark, wide_inp, wide_crops;      // (crop_lmk_kernel reads wide_crops alone: crops and I_out both)
    float scale, vy_ratio;
};

// What a workgroup knows of its face (blockIdx.y) once lmk_face has run: the float32 matrices, and the crop's destination -> source map, which is
// affine_inv.h's invert_affine of the float32 M_o2c widened to double - the AffineInv cs_crop_faces derives from the same doubles on the host.
struct LmkFace {
    float M[18];
    double A[6];
    int ok, refused;
};

// The head of lmk_input_kernel and crop_lmk_kernel, every thread of the workgroup: wave 0 forms the face's geometry (or finds it refused) into
// `s` (LDS), one barrier, tile 0's workgroup writes M and marks a face refused here.  Returns whether the face is cut.
__device__ __forceinline__ bool lmk_face(const float* __restrict__ lmk, const LmkInput& p, float* __restrict__ M_out, int* status, LmkFace& s)
{
    const int n = blockIdx.y, tid = threadIdx.x;
    if (tid < 64) {
        const int held = __hip_atomic_load(status + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // sticky: a face refused before is not looked at
        float M[18];
        int why = LMK_OK;
        if (held == 0) why = lmk_geometry(lmk + (long)n * p.N * 2, p.N, p.L, p.dsize, p.scale, p.vy_ratio, p.flag_do_rot, tid, 64, LmkWave(), M);
        else for (int i = 0; i < 18; ++i) M[i] = 0.f;
        if (tid == 0) {
            for (int i = 0; i < 18; ++i) s.M[i] = M[i];
            s.ok = held == 0 && why == LMK_OK;
            s.refused = held == 0 && why != LMK_OK;
            const double Md[6] = {(double)M[0], (double)M[1], (double)M[2], (double)M[3], (double)M[4], (double)M[5]};
            const AffineInv A = invert_affine(Md);
            for (int i = 0; i < 6; ++i) s.A[i] = A.m[i];
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (tid < 18) M_out[(long)n * 18 + tid] = s.M[tid];
        if (tid == 0 && s.refused) __hip_atomic_store(status + n, p.status_mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return s.ok != 0;
}

__global__ void __launch_bounds__(256) lmk_input_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ lmk, LmkInput p,
                                                        float* __restrict__ M_out, float* __restrict__ inp, unsigned char* __restrict__ crops,
                                                        int* status)
{
    __shared__ LmkFace s;
    const int n = blockIdx.y, tid = threadIdx.x;
    const bool ok = lmk_face(lmk, p, M_out, status, s);
    const int dsize = p.dsize, gw = dsize >> 2;
    const int g = blockIdx.x * 256 + tid;
    if (g >= gw * dsize) return;
    const int y = g / gw, xb = (g % gw) * 4;
    int v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 0;
    if (ok) {
        AffineInv A;
#pragma unroll
        for (int i = 0; i < 6; ++i) A.m[i] = s.A[i];
        const unsigned char* frame = frames + (long)p.frame[n] * p.Ho * p.Wo * 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Tap t = tap_at(A, xb + k, y, p.Ho, p.Wo);
            if (!t.outside) tap_u8x3(frame, p.Wo, t, v[k]);            // all four taps outside the frame: the border value 0
        }
    }
    const long plane = (long)dsize * dsize;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = inp + ((long)n * 3 + c) * plane + (long)y * dsize + xb;
        const float4 q = make_float4(staged_value(v[0][c]), staged_value(v[1][c]), staged_value(v[2][c]), staged_value(v[3][c]));
        if (p.wide_inp) *(float4*)d = q;
        else { d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; }
    }
    if (crops) {
        unsigned char* d = crops + (((long)n * dsize + y) * dsize + xb) * 3;
        if (p.wide_crops) {
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 2] |= (unsigned)v[j / 3][j % 3] << ((j & 3) * 8);
            ((unsigned*)d)[0] = w[0]; ((unsigned*)d)[1] = w[1]; ((unsigned*)d)[2] = w[2];
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) d[j] = (unsigned char)v[j / 3][j % 3];
        }
    }
}

// Everything is checked by the caller (cs_lmk_input).  Faces are grid rows, 64 per launch (their frame numbers are kernel arguments, as
// cs_crop_faces passes them), so B is not bound by anything; face, frame and plane offsets are 64-bit.
int launch_lmk_input(const unsigned char* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N, const cs_lmk_layout& L,
                            int dsize, float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M, float* inp, unsigned char* crops,
                            int* status, int B, hipStream_t st)
{
    LmkInput p = {};
    p.L = L; p.Ho = Ho; p.Wo = Wo; p.N = N; p.dsize = dsize; p.flag_do_rot = flag_do_rot; p.status_mark = status_mark;
    p.scale = scale; p.vy_ratio = vy_ratio;
    p.wide_inp = ((uintptr_t)inp & 15) == 0;                            // rows are multiples of four floats: every float4 is aligned with the base
    p.wide_crops = ((uintptr_t)crops & 3) == 0;
    const long plane = (long)dsize * dsize;
    const unsigned tiles = (unsigned)(((long)(dsize / 4) * dsize + 255) / 256);
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int nb = B - b0 < 64 ? B - b0 : 64;
        for (int i = 0; i < 64; ++i) p.frame[i] = i < nb ? frame_index[b0 + i] : 0;
        hipLaunchKernelGGL(lmk_input_kernel, dim3(tiles, (unsigned)nb), dim3(256), 0, st, frames, lmk + (long)b0 * N * 2, p, M + (long)b0 * 18,
                           inp + (long)b0 * 3 * plane, crops ? crops + (long)b0 * plane * 3 : nullptr, status + b0);
        LAUNCH_CHECK("lmk_input");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- landmarks -> matrices, the chains' crop, staged input
// cs_crop_lmk (include/canonswap_device_crop.h): crop_image for the chains from landmarks that stay on the device.  lmk_input_kernel's head
// (lmk_face: the geometry, the guard, the sticky status, M) in front of crop_batch_kernel's body (imgops.hip): a thread owns four crop pixels of
// a row, of two rows with STAGE != 0, forms their taps under the AffineInv of the float32 M_o2c and stores through crop_store (warp_taps.h), the
// crop's bytes and the fp32 staging cs_crop_faces writes from the same launch.  Tile 0's workgroup also writes the landmarks in the crop's
// frame, _transform_pts(lmk, M_o2c) (crop.py:66-72) in fp32, lmk_decode_kernel's order with the other matrix.  A refused face: zeros everywhere.
template <int STAGE>
__global__ void __launch_bounds__(256) crop_lmk_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ lmk, LmkInput p,
                                                       float* __restrict__ M_out, unsigned char* __restrict__ crops, float* __restrict__ I,
                                                       float* __restrict__ lmk_crop, int* status)
{
    constexpr int ROWS = STAGE ? 2 : 1;
    __shared__ LmkFace s;
    const int n = blockIdx.y, tid = threadIdx.x;
    const bool ok = lmk_face(lmk, p, M_out, status, s);
    if (lmk_crop && blockIdx.x == 0) {
        const float* src = lmk + (long)n * p.N * 2;
        float* d = lmk_crop + (long)n * p.N * 2;
        for (int i = tid; i < p.N; i += 256) {
            float cx = 0.f, cy = 0.f;
            if (ok) {
                const float x = src[2 * i], y = src[2 * i + 1];
                cx = (x * s.M[0] + y * s.M[1]) + s.M[2];
                cy = (x * s.M[3] + y * s.M[4]) + s.M[5];
            }
            d[2 * i] = cx; d[2 * i + 1] = cy;
        }
    }
    const int dsize = p.dsize, gw = dsize >> 2;
    const int g = blockIdx.x * 256 + tid;
    if (g >= gw * (dsize / ROWS)) return;
    const int yb = (g / gw) * ROWS, xb = (g % gw) * 4;
    int v[ROWS][4][3] = {};                                          // a refused face: zeros
    if (ok) {
        AffineInv A;
#pragma unroll
        for (int i = 0; i < 6; ++i) A.m[i] = s.A[i];
        crop_read<ROWS>(frames + (long)p.frame[n] * p.Ho * p.Wo * 3, p.Ho, p.Wo, A, xb, yb, v);
    }
    if (p.wide_crops) crop_store<STAGE, true>(v, n, yb, xb, dsize, crops, I);
    else crop_store<STAGE, false>(v, n, yb, xb, dsize, crops, I);
}

// Everything is checked by the caller (cs_crop_lmk): I != nullptr goes with dsize 256 or 512.  64 faces per launch, as launch_lmk_input.
int launch_crop_lmk(const unsigned char* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N, const cs_lmk_layout& L, int dsize,
                    float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M, unsigned char* crops, float* I, float* lmk_crop,
                    int* status, int B, hipStream_t st)
{
    LmkInput p = {};
    p.L = L; p.Ho = Ho; p.Wo = Wo; p.N = N; p.dsize = dsize; p.flag_do_rot = flag_do_rot; p.status_mark = status_mark;
    p.scale = scale; p.vy_ratio = vy_ratio;
    p.wide_crops = ((uintptr_t)crops & 3) == 0 && ((uintptr_t)I & 15) == 0;      // rows are multiples of four pixels: aligned with the base
    const long plane = (long)dsize * dsize;
    const int stage = I ? dsize / 256 : 0, rows = stage ? 2 : 1;
    const dim3 grid((unsigned)(((long)(dsize / 4) * (dsize / rows) + 255) / 256));
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int nb = B - b0 < 64 ? B - b0 : 64;
        for (int i = 0; i < 64; ++i) p.frame[i] = i < nb ? frame_index[b0 + i] : 0;
        const float* l = lmk + (long)b0 * N * 2;
        float* m = M + (long)b0 * 18;
        unsigned char* c = crops + (long)b0 * plane * 3;
        float* Ib = I ? I + (long)b0 * 3 * 256 * 256 : nullptr;
        float* lc = lmk_crop ? lmk_crop + (long)b0 * N * 2 : nullptr;
        if (stage == 2) hipLaunchKernelGGL(crop_lmk_kernel<2>, dim3(grid.x, nb), dim3(256), 0, st, frames, l, p, m, c, Ib, lc, status + b0);
        else if (stage == 1) hipLaunchKernelGGL(crop_lmk_kernel<1>, dim3(grid.x, nb), dim3(256), 0, st, frames, l, p, m, c, Ib, lc, status + b0);
        else hipLaunchKernelGGL(crop_lmk_kernel<0>, dim3(grid.x, nb), dim3(256), 0, st, frames, l, p, m, c, Ib, lc, status + b0);
        LAUNCH_CHECK("crop_lmk");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the network's points -> landmarks in the frame
// lmk = out_pts[2].reshape(-1, 2) * dsize (human_landmark_runner.py:82), then _transform_pts(lmk, M_c2o) = pts @ M[:2, :2].T + M[:2, 2]
// (crop.py:66-72): four products and four sums per point in fp32, each rounded, in the order written.  One thread per point; a refused face's
// points are left as they are.
__global__ void __launch_bounds__(256) lmk_decode_kernel(const float* __restrict__ out_pts, const float* __restrict__ M, const int* __restrict__ status,
                                                         float* __restrict__ lmk, int Np, float dsize)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Np || status[b] != 0) return;
    const float* m = M + (long)b * 18 + 9;
    const float x = out_pts[((long)b * Np + i) * 2] * dsize, y = out_pts[((long)b * Np + i) * 2 + 1] * dsize;
    float* d = lmk + ((long)b * Np + i) * 2;
    d[0] = (x * m[0] + y * m[1]) + m[2];
    d[1] = (x * m[3] + y * m[4]) + m[5];
}

int launch_lmk_decode(const float* out_pts, int Np, const float* M, int dsize, const int* status, float* lmk, int B, hipStream_t st)
{
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(lmk_decode_kernel, dim3((unsigned)((Np + 255) / 256), (unsigned)nb), dim3(256), 0, st, out_pts + (long)b0 * Np * 2,
                           M + (long)b0 * 18, status + b0, lmk + (long)b0 * Np * 2, Np, (float)dsize);
        LAUNCH_CHECK("lmk_decode");
    }
    return 0;
}
