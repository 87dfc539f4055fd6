// The two sides of the face detector's network (SCRFD; src/utils/dependencies/insightface/model_zoo/scrfd.py), on the device: frames -> the
// network's blob (cs_det_input) and the network's outputs -> faces (cs_det_decode).  The network itself stays the caller's.
//
// Both kernels restate numpy / OpenCV lines whose every operation is rounded on its own.  hipcc contracts a * b + c into one fma by default,
// which rounds once and gives other bits; the pragma below turns contraction off for this whole translation unit, and no fmaf / __fma_rn
// is written anywhere in it.  Division: hipcc's fp32 `/` is correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt), as
// numpy's is; the file is not compiled with any fast-math flag (_lib.HIPCC_FLAGS).
#include "common.h"
#include "../../include/canonswap_hip.h"

#pragma clang fp contract(off)

#define LAUNCH_CHECK(name)                                                                       \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) { cs_set_error(name " launch: %s", hipGetErrorString(_e)); return -1; } \
    } while (0)

// ---------------------------------------------------------------------------------------------- frames -> the detector's blob
// SCRFD.detect's letterbox (scrfd.py:224-235) and forward's blobFromImage (:154) for F frames in one launch, no intermediate in memory:
//   resized = cv2.resize(frame, (nw, nh))            default INTER_LINEAR, OpenCV's 8-bit arithmetic at a general ratio (below)
//   det_img = zeros(Hd, Wd, 3); det_img[:nh, :nw] = resized
//   blob    = (float(det_img) - mean) * (1 / std), channels first, swapRB      as a table of the byte: lut[c][v], c the OUTPUT plane
// One axis of cv2.resize src -> dst (resize.cpp, resizeGeneric_ with the fixed-point linear kernels):
//   scale = 1.0 / (double(dst) / src);  f = float((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s;
//   columns: s < 0 -> s = 0, f = 0;  s >= src - 1 -> s = src - 1, f = 0;  taps s and s + 1 (the second never read where f was zeroed)
//   rows:    the two rows s and s + 1 are clamped to [0, src - 1], their weights KEPT (at x2 row 0 is row 0 twice under 512 and 1536, the
//            arithmetic of cs_concat_frames kind 1; the truncating shifts make that differ from one tap of 2048)
//   coefficients short(rint((1.f - f) * 2048)) and short(rint(f * 2048)), rint = round half to even (cvRound)
//   horizontal pass into int32: H = a0 S[s] + a1 S[s + 1];  vertical: (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2, saturated
//   src = 2 dst on BOTH axes: OpenCV takes INTER_AREA's 2 x 2 mean, (a + b + c + d + 2) >> 2;  equal sizes: the arithmetic is the identity.
// PARITY UNPINNED: restated from OpenCV's published algorithm (tests/detect_ref.py is the same restatement in numpy), no cv2 vectors at hand.
// A thread owns one pixel of the blob: its two column taps and two row taps are computed in place (two double multiplications each), four
// bytes per channel are read, three floats written - a wave writes 256 contiguous bytes of each plane's row.  The table sits in LDS.
struct DetInput {
    int Ho, Wo, Hd, Wd, nh, nw, swap_rb, area;      // area: the 2 x 2 mean (Ho == 2 nh and Wo == 2 nw)
    double sx, sy;                                   // 1.0 / (double(nw) / Wo), 1.0 / (double(nh) / Ho)
};

__device__ __forceinline__ void cv_linear_tap(int d, double scale, int& s, float& f)
{
    f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    f -= fl;
}

__device__ __forceinline__ void cv_coeffs(float f, int& c0, int& c1)
{
    c0 = (int)(short)rintf((1.f - f) * 2048.f);
    c1 = (int)(short)rintf(f * 2048.f);
}

__global__ void __launch_bounds__(256) det_input_kernel(const unsigned char* __restrict__ frames, DetInput p, const float* __restrict__ lut,
                                                        float* __restrict__ blob)
{
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = lut[i];
    __syncthreads();
    const long plane = (long)p.Hd * p.Wd;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= plane) return;
    const long n = blockIdx.y;
    const int y = (int)(t / p.Wd), x = (int)(t % p.Wd);
    int v[3] = {0, 0, 0};                                               // the letterbox's zeros go through the blob arithmetic too
    if (y < p.nh && x < p.nw) {
        const unsigned char* in = frames + n * ((long)p.Ho * p.Wo * 3);
        if (p.area) {
            const unsigned char* q = in + ((long)(2 * y) * p.Wo + 2 * x) * 3;
            const long row = (long)p.Wo * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (q[c] + q[3 + c] + q[row + c] + q[row + 3 + c] + 2) >> 2;
        } else {
            int s0, r0, a0, a1, b0, b1;
            float fx, fy;
            cv_linear_tap(x, p.sx, s0, fx);
            if (s0 < 0) { s0 = 0; fx = 0.f; }
            if (s0 >= p.Wo - 1) { s0 = p.Wo - 1; fx = 0.f; }
            const int s1 = min(s0 + 1, p.Wo - 1);                        // read only under a zero coefficient where it is clamped
            cv_linear_tap(y, p.sy, r0, fy);
            const int y0 = min(max(r0, 0), p.Ho - 1), y1 = min(max(r0 + 1, 0), p.Ho - 1);
            cv_coeffs(fx, a0, a1);
            cv_coeffs(fy, b0, b1);
            const unsigned char* q0 = in + (long)y0 * p.Wo * 3;
            const unsigned char* q1 = in + (long)y1 * p.Wo * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h0 = a0 * q0[s0 * 3 + c] + a1 * q0[s1 * 3 + c], h1 = a0 * q1[s0 * 3 + c] + a1 * q1[s1 * 3 + c];
                v[c] = min(max((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0), 255);
            }
        }
    }
    float* d = blob + n * 3 * plane + t;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * plane] = tab[c * 256 + v[p.swap_rb ? 2 - c : c]];
}

// scrfd.py:224-231 with its truncating int(): the resized size inside the Hd x Wd letterbox.  Host doubles, as Python's floats.
void det_letterbox(int Ho, int Wo, int Hd, int Wd, int* nh, int* nw)
{
    const double im_ratio = (double)Ho / (double)Wo, model_ratio = (double)Hd / (double)Wd;
    if (im_ratio > model_ratio) {
        *nh = Hd;
        *nw = (int)((double)*nh / im_ratio);
    } else {
        *nw = Wd;
        *nh = (int)((double)*nw * im_ratio);
    }
}

// F, Ho, Wo >= 1, 1 <= Hd, Wd <= 16384, a resized size of at least 1 x 1, no NULL pointer: the caller checks (cs_det_input).  Frames are grid
// rows, 65535 of them per launch; frame and plane offsets are 64-bit.
int launch_det_input(const unsigned char* frames, int F, int Ho, int Wo, int Hd, int Wd, int swap_rb, const float* lut, float* blob, hipStream_t st)
{
    DetInput p = {};
    p.Ho = Ho; p.Wo = Wo; p.Hd = Hd; p.Wd = Wd; p.swap_rb = swap_rb;
    det_letterbox(Ho, Wo, Hd, Wd, &p.nh, &p.nw);
    p.area = Ho == 2 * p.nh && Wo == 2 * p.nw;
    p.sx = 1.0 / ((double)p.nw / (double)Wo);
    p.sy = 1.0 / ((double)p.nh / (double)Ho);
    const long plane = (long)Hd * Wd, in_frame = (long)Ho * Wo * 3;
    for (int f0 = 0; f0 < F; f0 += 65535) {
        const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)(F - f0 < 65535 ? F - f0 : 65535)), block(256);
        hipLaunchKernelGGL(det_input_kernel, grid, block, 0, st, frames + f0 * in_frame, p, lut, blob + f0 * 3 * plane);
        LAUNCH_CHECK("det_input");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the network's outputs -> faces
// SCRFD.forward's decode (scrfd.py:160-218) and detect's sort, NMS and max_num pick (:239-273, :275-303) for F frames in one launch, one
// workgroup per frame, everything between the network's tensors and the result in LDS.  fp32 throughout, every operation rounded on its own
// (see the head of the file).  Per frame:
//   1. candidates: the anchors with score >= det_thresh, levels in order, anchors in order - compacted in exactly that order with a prefix
//      scan over the waves' 64-bit ballots (no atomics: position k of the list is candidate k of the reference's vstack, whatever the schedule);
//   2. centre = ((cell % width) * stride, (cell / width) * stride), cell = anchor / num_anchors; box = centre -/+ pred * stride, / det_scale;
//   3. the order NMS visits them in: descending score; the reference sorts twice with argsort()[::-1] (:241, :284), a stable argsort
//      reversed both times by this project's contract - the first puts the LATER of two equal scores first, the second reverses that again, so
//      NMS visits equal scores in anchor order.  A rank sort over LDS (every candidate counts the ones in front of it);
//   4. greedy NMS (:275-303): areas with + 1, ovr = inter / (area_i + area_j - inter), survives on ovr <= nms_thresh.  Only a kept box costs a
//      barrier: a suppressed one is skipped by every thread alike;
//   5. max_num > 0 and more survivors: the max_num largest by area - 2 offset^2 (metric_max: area), area without + 1, stable argsort reversed;
//   6. det (x1, y1, x2, y2, score) and kps (five points, decoded like the box's corners) of the result.
// count: the faces written; -1: more than DET_MAX_CAND candidates; -2: max_num == 0 and more than max_faces survivors (nothing else of the
// frame is written then).  Scores and predictions are assumed finite: how a NaN orders is not part of the contract.
constexpr int DET_MAX_CAND = 1024, DET_NT = 1024, DET_WAVES = DET_NT / 64, DET_LEVELS = 5;
static_assert(DET_MAX_CAND == CS_DET_MAX_CAND && CS_DET_MAX_FACES <= DET_MAX_CAND, "the header's CS_DET_MAX_CAND / CS_DET_MAX_FACES");

struct DetDecode {
    const float* score[DET_LEVELS];
    const float* bbox[DET_LEVELS];
    const float* kps[DET_LEVELS];      // all NULL without key points
    int stride[DET_LEVELS], width[DET_LEVELS], anchors[DET_LEVELS];      // anchors: A_l per frame
    int n_levels, num_anchors, max_num, metric_max, max_faces;
    float det_scale, det_thresh, nms_thresh, cx, cy;      // (cx, cy) = (Wo / 2, Ho / 2), integer division, as floats
};

__global__ void __launch_bounds__(DET_NT) det_decode_kernel(DetDecode p, float* __restrict__ det, float* __restrict__ kps_out, int* __restrict__ count)
{
    __shared__ float s_score[DET_MAX_CAND];
    __shared__ float s_box[DET_MAX_CAND][4];
    __shared__ float s_val[DET_MAX_CAND];
    __shared__ int s_src[DET_MAX_CAND];       // level << 24 | anchor (an anchor index stays below 2^24 at 16384 a side)
    __shared__ int s_ord[DET_MAX_CAND];       // visiting position -> candidate
    __shared__ int s_sup[DET_MAX_CAND];       // by visiting position
    __shared__ int s_keep[DET_MAX_CAND];      // kept candidates in the order NMS kept them
    __shared__ int s_out[DET_MAX_CAND];       // output slot -> index into s_keep
    __shared__ int s_wave[2][DET_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long f = blockIdx.x;

    // 1. compaction in anchor order
    int n = 0, it = 0;                                                  // n: candidates so far, the same in every thread
    for (int l = 0; l < p.n_levels; ++l) {
        const int A = p.anchors[l];
        const float* sc = p.score[l] + f * A;
        for (int a0 = 0; a0 < A; a0 += DET_NT, ++it) {
            const int a = a0 + tid;
            const float s = a < A ? sc[a] : 0.f;
            const bool c = a < A && s >= p.det_thresh;
            const unsigned long long m = __ballot(c);
            if (lane == 0) s_wave[it & 1][wave] = __popcll(m);
            __syncthreads();                                            // (the other half of s_wave is rewritten only behind the next barrier)
            int off = n, total = 0;
#pragma unroll
            for (int k = 0; k < DET_WAVES; ++k) {
                const int cnt = s_wave[it & 1][k];
                if (k < wave) off += cnt;
                total += cnt;
            }
            if (c) {
                const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < DET_MAX_CAND) { s_score[pos] = s; s_src[pos] = l << 24 | a; }
            }
            n += total;
        }
    }
    if (n > DET_MAX_CAND) {
        if (tid == 0) count[f] = -1;
        return;
    }
    if (n == 0) {
        if (tid == 0) count[f] = 0;
        return;
    }
    __syncthreads();

    // 2. boxes
    for (int i = tid; i < n; i += DET_NT) {
        const int l = s_src[i] >> 24, a = s_src[i] & 0xffffff, cell = a / p.num_anchors;
        const float st = (float)p.stride[l];
        const float px = (float)(cell % p.width[l]) * st, py = (float)(cell / p.width[l]) * st;
        const float* b = p.bbox[l] + (f * p.anchors[l] + a) * 4;
        s_box[i][0] = (px - b[0] * st) / p.det_scale;
        s_box[i][1] = (py - b[1] * st) / p.det_scale;
        s_box[i][2] = (px + b[2] * st) / p.det_scale;
        s_box[i][3] = (py + b[3] * st) / p.det_scale;
        s_sup[i] = 0;
    }
    // 3. the visiting order: descending score, equal scores in anchor order
    for (int i = tid; i < n; i += DET_NT) {
        const float si = s_score[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = s_score[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        s_ord[r] = i;
    }
    __syncthreads();

    // 4. greedy NMS
    int nk = 0;
    const bool capped = p.max_num == 0;
    for (int q = 0; q < n; ++q) {
        if (s_sup[q]) continue;                                         // uniform: written before the last barrier
        const int i = s_ord[q];
        if (capped && nk == p.max_faces) {                              // one survivor more than the result holds
            if (tid == 0) count[f] = -2;
            return;
        }
        if (tid == 0) s_keep[nk] = i;
        ++nk;
        const float x1 = s_box[i][0], y1 = s_box[i][1], x2 = s_box[i][2], y2 = s_box[i][3];
        const float area_i = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
        for (int r = q + 1 + tid; r < n; r += DET_NT) {
            if (s_sup[r]) continue;
            const int j = s_ord[r];
            const float u1 = s_box[j][0], v1 = s_box[j][1], u2 = s_box[j][2], v2 = s_box[j][3];
            const float area_j = (u2 - u1 + 1.f) * (v2 - v1 + 1.f);
            const float w = fmaxf(0.f, fminf(x2, u2) - fmaxf(x1, u1) + 1.f), h = fmaxf(0.f, fminf(y2, v2) - fmaxf(y1, v1) + 1.f);
            const float inter = w * h;
            const float ovr = inter / (area_i + area_j - inter);
            if (!(ovr <= p.nms_thresh)) s_sup[r] = 1;
        }
        __syncthreads();
    }
    __syncthreads();                                                    // s_keep

    // 5. the max_num pick
    int nout = nk;
    if (p.max_num > 0 && nk > p.max_num) {
        nout = p.max_num;
        for (int k = tid; k < nk; k += DET_NT) {
            const int i = s_keep[k];
            const float x1 = s_box[i][0], y1 = s_box[i][1], x2 = s_box[i][2], y2 = s_box[i][3];
            const float area = (x2 - x1) * (y2 - y1);
            const float ox = (x1 + x2) / 2.f - p.cx, oy = (y1 + y2) / 2.f - p.cy;
            const float d2 = ox * ox + oy * oy;
            s_val[k] = p.metric_max ? area : area - d2 * 2.f;
        }
        __syncthreads();
        for (int k = tid; k < nk; k += DET_NT) {
            const float vk = s_val[k];
            int r = 0;
            for (int j = 0; j < nk; ++j) {
                const float vj = s_val[j];
                r += (vj > vk || (vj == vk && j > k)) ? 1 : 0;          // a stable argsort reversed: the later of two equal values first
            }
            if (r < nout) s_out[r] = k;
        }
    } else {
        for (int k = tid; k < nk; k += DET_NT) s_out[k] = k;
    }
    __syncthreads();

    // 6. the result
    for (int o = tid; o < nout; o += DET_NT) {
        const int i = s_keep[s_out[o]];
        float* d = det + (f * p.max_faces + o) * 5;
        d[0] = s_box[i][0]; d[1] = s_box[i][1]; d[2] = s_box[i][2]; d[3] = s_box[i][3]; d[4] = s_score[i];
    }
    if (kps_out) {
        for (int o = tid; o < nout * 10; o += DET_NT) {
            const int i = s_keep[s_out[o / 10]], e = o % 10;
            const int l = s_src[i] >> 24, a = s_src[i] & 0xffffff, cell = a / p.num_anchors;
            const float st = (float)p.stride[l];
            const float c = (e & 1) ? (float)(cell / p.width[l]) * st : (float)(cell % p.width[l]) * st;
            kps_out[(f * p.max_faces) * 10 + o] = (c + p.kps[l][(f * p.anchors[l] + a) * 10 + e] * st) / p.det_scale;
        }
    }
    if (tid == 0) count[f] = nout;
}

// Everything is checked by the caller (cs_det_decode): a supported layout, sizes in range, no NULL pointer but the optional ones.
int launch_det_decode(int F, int n_levels, const int* strides, int num_anchors, const void* const* outs, int Hd, int Wd, float det_scale,
                      float det_thresh, float nms_thresh, int max_num, int metric_max, int Ho, int Wo, int max_faces, float* det, float* kps,
                      int* count, hipStream_t st)
{
    DetDecode p = {};
    for (int l = 0; l < n_levels; ++l) {
        p.score[l] = (const float*)outs[l];
        p.bbox[l] = (const float*)outs[n_levels + l];
        p.kps[l] = (const float*)outs[2 * n_levels + l];
        p.stride[l] = strides[l];
        p.width[l] = Wd / strides[l];
        p.anchors[l] = (Hd / strides[l]) * (Wd / strides[l]) * num_anchors;
    }
    p.n_levels = n_levels; p.num_anchors = num_anchors; p.max_num = max_num; p.metric_max = metric_max; p.max_faces = max_faces;
    p.det_scale = det_scale; p.det_thresh = det_thresh; p.nms_thresh = nms_thresh;
    p.cx = (float)(Wo / 2); p.cy = (float)(Ho / 2);
    hipLaunchKernelGGL(det_decode_kernel, dim3((unsigned)F), dim3(DET_NT), 0, st, p, det, kps, count);
    LAUNCH_CHECK("det_decode");
    return 0;
}
