/* canonswap_landmarks.h -- the landmark runner's two sides on the device: the per-frame loop of the cropper without the host.
 *
 * Why a header of its own: include/canonswap_hip.h is version 4 of the C ABI and is recorded line for line (tests/golden/abi_v4.txt, with the
 * binding table canonswap_amd/_lib.py ABI pinned entry by entry).  These entry points are an addition beside it, not a change of it: they live in
 * the same library, take the same cs_engine, follow the same conventions (0 or non-zero with cs_last_error(), caller-owned contiguous device
 * buffers, everything enqueued on the caller's stream, last parameter `void* stream`), and carry a version of their own, cs_lmk_abi_version().
 * Their binding is canonswap_amd/_lib.py ABI_LANDMARKS.
 *
 * The reference tracks landmarks frame by frame: Cropper.crop_source_video (src/utils/cropper.py:167-222) crops frame k around the landmarks of
 * frame k - 1 (cropper.py:186-193) and LandmarkRunner.run (src/utils/human_landmark_runner.py:60-85) does, per frame,
 *     crop_image(img, lmk, dsize=224, scale=1.5, vy_ratio=-0.1)      human_landmark_runner.py:62   (src/utils/crop.py:429-455)
 *     inp = (img_crop / 255).transpose(2, 0, 1)[None]                human_landmark_runner.py:76
 *     out_pts = the ONNX network(inp)                                human_landmark_runner.py:78   (the caller's, as the detector's is)
 *     lmk = out_pts[2].reshape(-1, 2) * dsize                        human_landmark_runner.py:82
 *     lmk = _transform_pts(lmk, M=M_c2o)                             human_landmark_runner.py:83   (src/utils/crop.py:66-72)
 * cs_lmk_input is everything in front of the network, cs_lmk_decode everything behind it; the landmarks, the matrices and the crop stay on the
 * device, so the steps of a batch of frames can be enqueued without a host wait.
 */
#ifndef CANONSWAP_LANDMARKS_H
#define CANONSWAP_LANDMARKS_H
#include <stdint.h>
#include "canonswap_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CS_LMK_ABI_VERSION 1   /* bumped whenever cs_lmk_layout or an entry point's meaning changes */
int cs_lmk_abi_version(void);

/* Which landmarks span the eye-lip axis (parse_pt2_from_pt_x and the per-layout parsers it dispatches to, src/utils/crop.py:98-241, with
 * use_lip=True as parse_rect_from_landmark calls it): each eye is the mean of n_eye points (4: the 101 / 106 / 203 layouts, crop.py:103-142;
 * 2: 68 and 9 points, crop.py:153-171, 190-214; 1: 5 points, crop.py:173-188), the lips the mean of two.  canonswap_amd/landmarks.py layout_of(N)
 * builds it from crop.EYE_LIP_POINTS and the 68 / 9 / 5 rules; "more than 101 points reads the first 101" is the 101 layout's indices, which the
 * struct states as they are.  Every index lies in [0, N). */
typedef struct cs_lmk_layout {
    int n_eye;                 /* points per eye, 1 to 4 */
    int left[4], right[4];     /* the first n_eye of each are read */
    int lip[2];
} cs_lmk_layout;

/* human_landmark_runner.py:62 + :76 for B faces in F frames, one launch per 64 faces.  Face b, from its landmarks lmk[b] (N x 2 fp32 on the
 * device, frame coordinates):
 *   geometry   crop_image's matrices (crop.py:429-455 through _estimate_similar_transform_from_pts, crop.py:381-426, and
 *              parse_rect_from_landmark, crop.py:244-300): M_o2c, and M_c2o = its inverse, both stored as float32.  float32 landmarks and
 *              constants, the angle, its sine and cosine doubles, as the reference holds them; where the reference calls float32 BLAS / LAPACK
 *              ((pts - c) @ R.T, np.linalg.inv) and where it sums N points the value is formed in double and rounded once.  Every branch is
 *              mirrored: an eye-lip distance <= 1e-3 takes the axis (0, 1); the sign of the angle; flag_do_rot = 0; vx_ratio is never
 *              forwarded by crop_image and does not exist here.  The sums and extrema over the N points run in a fixed order.
 *   crop       cv2.warpAffine(frames[frame_index[b]], M_o2c[b][:2], (dsize, dsize), INTER_LINEAR), border 0: the arithmetic of cs_crop_faces on
 *              the float32 M_o2c widened to double, bit for bit.
 *   outputs    M[b]: 18 fp32 = M_o2c 3 x 3 | M_c2o 3 x 3;  inp[b]: 3 x dsize x dsize fp32 = crop / 255, channels first (the network's input);
 *              crops[b]: dsize x dsize x 3 uint8, optional (NULL: not written);  status[b]: int32.
 *   guard      before any coordinate is formed a face is refused when a landmark is not finite, the box side is not > 0, the scale is not
 *              finite, or an entry of either matrix is above 1e6 in magnitude (the bound of the paste-back's face box): status[b] = status_mark,
 *              inp[b], crops[b] and M[b] are zeros and no byte of any frame is read for it.  status is sticky: a face whose status[b] is
 *              non-zero on entry is refused without a look at its landmarks and keeps its value.  The caller zeroes status once.
 * frame_index: B host ints in [0, F), any order, repeats allowed (all faces of a step may name one frame).  dsize: a multiple of 4 from 4 to
 * 16384.  B, F >= 1, not bound by max_batch.  status_mark: non-zero (a tracker passes the step's number + 1 and reads which step froze a face).
 * No engine scratch is used and nothing synchronises; every argument is checked before anything is launched. */
int cs_lmk_input(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N,
                 cs_lmk_layout layout, int dsize, float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M, float* inp,
                 uint8_t* crops, int* status, void* stream);

/* human_landmark_runner.py:82-83 for B faces: out_pts (B x 2 Np fp32, the network's third output) -> lmk (B x Np x 2 fp32, frame coordinates):
 *   x = out_pts[2 i] * dsize, y = out_pts[2 i + 1] * dsize;  lmk = (x m00 + y m01) + m02, (x m10 + y m11) + m12
 * with M_c2o = M[b] + 9 in fp32, every product and sum rounded, in that order.  A face with status[b] != 0 keeps what lmk[b] holds: its
 * trajectory is frozen, not poisoned by a matrix of zeros.  lmk may be the buffer the next cs_lmk_input reads (stream order); out_pts and lmk
 * must not overlap.  B, Np >= 1.  No engine scratch, nothing synchronises, every argument is checked before the launch. */
int cs_lmk_decode(cs_engine* e, int B, const float* out_pts, int Np, const float* M, int dsize, const int* status, float* lmk, void* stream);

#ifdef __cplusplus
}
#endif
#endif
