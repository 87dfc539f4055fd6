/* canonswap_device_crop.h -- the crop and the paste-back from landmarks and matrices that never leave the device.
 *
 * Why a header of its own: as include/canonswap_landmarks.h and include/canonswap_yuv.h, these entry points are an addition beside version 4 of
 * the C ABI (include/canonswap_hip.h, recorded line for line), not a change of it.  They live in the same library, take the same cs_engine, follow
 * the same conventions (0 or non-zero with cs_last_error(), caller-owned contiguous device buffers, everything enqueued on the caller's stream,
 * last parameter `void* stream`, every argument checked before anything is launched) and carry a version of their own, cs_dcrop_abi_version().
 * Their binding is canonswap_amd/_lib.py ABI_DEVICE_CROP; the recorded text is tests/golden/abi_device_crop_v1.txt.
 *
 * cs_crop_faces and cs_paste_back_faces take their matrices as host doubles: a caller whose landmarks come from cs_lmk_decode has to download
 * them, form the matrices and only then enqueue the crop.  Here the landmarks (cs_crop_lmk) and the matrices (cs_paste_back_faces_dev) are read
 * from device memory by the kernels themselves, so a batch's crop, generator and paste-back are enqueued behind the tracker without a host wait.
 * Neither call uses engine scratch and neither synchronises: both may run beside a prefetch on another stream.  The struct cs_lmk_layout is the
 * one of canonswap_landmarks.h, taken by pointer (a host pointer, read before the call returns); this header defines no struct.
 */
#ifndef CANONSWAP_DEVICE_CROP_H
#define CANONSWAP_DEVICE_CROP_H
#include <stdint.h>
#include "canonswap_landmarks.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CS_DCROP_ABI_VERSION 1   /* bumped whenever an entry point's meaning changes */
int cs_dcrop_abi_version(void);

/* crop_image (src/utils/crop.py:429-455) for B faces in F frames from landmarks on the device, one launch per 64 faces.  Face b, from lmk[b]
 * (N x 2 fp32 on the device, frame coordinates):
 *   geometry   cs_lmk_input's, the same text (csrc/lmk_geometry.h): M[b] = 18 fp32 = M_o2c 3 x 3 | M_c2o 3 x 3 has the bits cs_lmk_input writes
 *              for the same lmk, N, layout, dsize, scale, vy_ratio and flag_do_rot.
 *   guard      cs_lmk_input's, and its sticky status: a face whose status[b] is non-zero on entry is refused without a look at its landmarks and
 *              keeps its value; a face the geometry refuses (a landmark not finite, an empty box, a scale that is not finite, a matrix entry above
 *              1e6) gets status[b] = status_mark.  A refused face's M, crop, I_out and lmk_crop are zeros and no byte of any frame is read for it.
 *   crop       crops[b] = cv2.warpAffine(frames[frame_index[b]], M_o2c[:2], (dsize, dsize), INTER_LINEAR), border 0: the arithmetic of
 *              cs_crop_faces on the float32 M_o2c widened to double, bit for bit.
 *   I_out      optional (NULL: not written; dsize 256 or 512 only): B x 3 x 256 x 256 fp32, what cs_crop_faces writes from the same launch, i.e.
 *              cs_prepare_crops of the crop (dsize 512: INTER_AREA to one half; / 255; channels first).
 *   lmk_crop   optional (NULL: not written): B x N x 2 fp32, the landmarks in the crop's frame, _transform_pts(lmk, M_o2c) (crop.py:66-72) in fp32:
 *              (x m00 + y m01) + m02, (x m10 + y m11) + m12, every product and sum rounded, in that order (cs_lmk_decode's, with the other matrix).
 * frame_index: B host ints in [0, F), any order, repeats allowed.  layout: a host pointer; every index it reads lies in [0, N).  dsize: a multiple
 * of 4 from 4 to 16384.  B, F >= 1, not bound by max_batch.  status_mark: non-zero.  status: B int32 on the device, read and written; the caller
 * zeroes it once.  lmk must not overlap any output. */
int cs_crop_lmk(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N,
                const cs_lmk_layout* layout, int dsize, float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M, uint8_t* crops,
                float* I_out, float* lmk_crop, int* status, void* stream);

/* cs_paste_back_faces with the matrices read from device memory: face b (crops[b] Hc x Wc x 3 u8 under masks_crop[b] Hc x Wc fp32) is pasted into
 * frame frame_index[b] under M_c2o = M[b] + 9 (M: B x 18 fp32 on the device, what cs_crop_lmk and cs_lmk_input write), the faces of a frame in
 * their order, each on the result of the one before, in one pass over every frame.  Per face the float32 M_c2o is widened to double and
 * inverted as cv2.warpAffine inverts it (once per workgroup, not per pixel), from the text cs_paste_back_faces runs on the host; then
 * cs_paste_back_faces' arithmetic per pixel, bit for bit.  status: B int32 on the device or NULL; a face with status[b] != 0 is skipped as if
 * it were not listed (its M is zeros).  frame_index: B host ints, non-decreasing, in [0, F).  What cs_paste_back_faces allows, this allows:
 * out == imgs_ori (in place), a frame without a face (copied; in place: left alone), B = 0 (the frames are copied; crops, masks_crop, frame_index,
 * M and status are not read and may be NULL), any B and F, any Ho and Wo and any alignment of imgs_ori and out (Wo not a multiple of 4 or a buffer
 * off a 4-byte boundary: a per-pixel kernel with the same values).  crops and masks_crop must not overlap out. */
int cs_paste_back_faces_dev(cs_engine* e, int B, int F, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const int* frame_index,
                            const float* M, const int* status, const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream);

#ifdef __cplusplus
}
#endif
#endif
