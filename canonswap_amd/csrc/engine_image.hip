// The image-space entry points of the C ABI around the generator: soft erosion, crops, warps, paste-back, key-points, resize, face masks, parser
// input, concat, the detector's input and decode, the landmark runner's input and decode, the identity network and the face parser.  Argument checks
// and one launch each.
#include "engine.h"
#include "../../include/canonswap_landmarks.h"
#include "../../include/canonswap_yuv.h"
#include "../../include/canonswap_device_crop.h"

// ---- image-space steps around the generator
static int soft_erosion_impl(cs_engine* e, int B, int H, int W, const void* mask, int mask_u8, const float* w, int ksize, float thr, int iters,
                             float* soft_out, uint8_t* hard_out, int per_sample, void* stream, const char* who)
{
    if (!e || !mask || !w || !soft_out || B < 1 || H < 1 || W < 1) { cs_set_error("%s: bad arguments", who); return -1; }
    if (B > 65535 || H > 65535 * 32) { cs_set_error("%s: %d x %d x %d exceeds the launch grid", who, B, H, W); return -1; }      // grid (W/64, H/32, B)
    DevGuard guard(e->dev);
    const size_t need = (size_t)B * H * W, need_part = (size_t)64 * B;      // launch_soft_erosion: 64 partial maxima per sample
    // grow-only scratch; buffers of earlier sizes stay owned by the engine until cs_destroy
    if (need > e->se_cap) {
        if (e->alloc(&e->se_a, need) || e->alloc(&e->se_b, need)) return -1;
        e->se_cap = need;
    }
    if (need_part > e->se_part_cap) {
        if (e->alloc(&e->se_part, need_part)) return -1;
        e->se_part_cap = need_part;
    }
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_soft_erosion(mask, mask_u8, e->se_a, e->se_b, w, e->se_part, soft_out, hard_out, B, H, W, ksize, thr, iters,
                                                          per_sample, st); }, "soft_erosion");
}

extern "C" int cs_soft_erosion(cs_engine* e, int B, int H, int W, const float* mask, const float* w, int ksize, float thr, int iters,
                               float* soft_out, uint8_t* hard_out, void* stream)
{
    return soft_erosion_impl(e, B, H, W, mask, 0, w, ksize, thr, iters, soft_out, hard_out, 0, stream, "cs_soft_erosion");
}

extern "C" int cs_soft_erosion_frames(cs_engine* e, int B, int H, int W, const void* masks, int masks_u8, const float* w, int ksize, float thr,
                                      int iters, float* soft_out, uint8_t* hard_out, void* stream)
{
    return soft_erosion_impl(e, B, H, W, masks, masks_u8 != 0, w, ksize, thr, iters, soft_out, hard_out, 1, stream, "cs_soft_erosion_frames");
}

extern "C" int cs_prepare_crops(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, float* out, void* stream)
{
    if (!e || !crops || !out || B < 1) { cs_set_error("cs_prepare_crops: bad arguments"); return -1; }
    if (!((Hc == 256 && Wc == 256) || (Hc == 512 && Wc == 512))) {
        cs_set_error("cs_prepare_crops: crops must be 256x256 or 512x512 (got %dx%d)", Hc, Wc);
        return -1;
    }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_prepare_crops(crops, out, B, Hc, Wc, Hc / 256, st); }, "prepare_crops");
}

extern "C" int cs_warp_affine_u8(cs_engine* e, const uint8_t* src, int Hs, int Ws, const double M[6], uint8_t* dst, int Hd, int Wd, void* stream)
{
    if (!e || !src || !dst || !M || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) { cs_set_error("cs_warp_affine_u8: bad arguments"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste(src, nullptr, nullptr, Hs, Ws, M, nullptr, dst, Hd, Wd, st); }, "warp_affine_u8");
}

extern "C" int cs_warp_affine_f32(cs_engine* e, const float* src, int Hs, int Ws, const double M[6], float* dst, int Hd, int Wd, void* stream)
{
    if (!e || !src || !dst || !M || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) { cs_set_error("cs_warp_affine_f32: bad arguments"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_warp_f32(src, Hs, Ws, M, dst, Hd, Wd, st); }, "warp_affine_f32");
}

extern "C" int cs_paste_back(cs_engine* e, const uint8_t* crop, const float* mask_crop, const float* mask_ori, int Hc, int Wc,
                             const double M_c2o[6], const uint8_t* img_ori, uint8_t* out, int Ho, int Wo, void* stream)
{
    if (!e || !crop || !M_c2o || !img_ori || !out || Hc < 1 || Wc < 1 || Ho < 1 || Wo < 1) { cs_set_error("cs_paste_back: bad arguments"); return -1; }
    if ((mask_crop != nullptr) == (mask_ori != nullptr)) { cs_set_error("cs_paste_back: pass exactly one of mask_crop / mask_ori"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste(crop, mask_crop, mask_ori, Hc, Wc, M_c2o, img_ori, out, Ho, Wo, st); }, "paste_back");
}

extern "C" int cs_paste_back_batch(cs_engine* e, int B, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const double* M_c2o,
                                   const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream)
{
    if (!e || !crops || !masks_crop || !M_c2o || !imgs_ori || !out || B < 1 || Hc < 1 || Wc < 1 || Ho < 1 || Wo < 1) {
        cs_set_error("cs_paste_back_batch: bad arguments");
        return -1;
    }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste_batch(crops, masks_crop, Hc, Wc, M_c2o, imgs_ori, out, B, Ho, Wo, st); }, "paste_back_batch");
}

extern "C" int cs_motion_keypoints(cs_engine* e, int B, const float* raw, float* x_t, float* x_can, float* rot, void* stream)
{
    if (!e || !raw || !x_t || !x_can || B < 1) { cs_set_error("cs_motion_keypoints: bad arguments"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_m_keypoints(raw, x_t, x_can, rot, B, st); }, "m_keypoints");
}

// ---- the device-side frame of the video-to-image pipeline around cs_animate_frames (can_swap_pipeline_v2i.py:285-321)
extern "C" int cs_resize_half_bilinear(cs_engine* e, int B, int C, const float* img, int H, int W, float* out, void* stream)
{
    if (!e || !img || !out || B < 1 || C < 1 || H < 2 || W < 2) { cs_set_error("cs_resize_half_bilinear: bad arguments"); return -1; }
    if (H % 2 || W % 2) { cs_set_error("cs_resize_half_bilinear: H and W must be even (got %dx%d)", H, W); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_resize_half(img, out, (long)B * C, H, W, st); }, "resize_half");
}

extern "C" int cs_motion_keypoints_driven(cs_engine* e, int B, const float* raw_driving, const float* raw_pose, const float* kp, float* x_t,
                                          void* stream)
{
    if (!e || !raw_driving || !raw_pose || !kp || !x_t || B < 1) { cs_set_error("cs_motion_keypoints_driven: bad arguments"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_m_keypoints_driven(raw_driving, raw_pose, kp, x_t, B, st); }, "m_keypoints_driven");
}

extern "C" int cs_paste_back_shared(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, const float* mask_ori, const double M_c2o[6],
                                    const uint8_t* img_ori, uint8_t* out, int Ho, int Wo, void* stream)
{
    if (!e || !crops || !mask_ori || !M_c2o || !img_ori || !out || B < 1 || Hc < 1 || Wc < 1 || Ho < 1 || Wo < 1) {
        cs_set_error("cs_paste_back_shared: bad arguments");
        return -1;
    }
    // 32-bit byte offsets inside one crop; eight frames per grid row
    if ((long)Hc * Wc * 3 >= (1L << 31) || B > 65535 * 8) { cs_set_error("cs_paste_back_shared: crop %dx%d or B = %d exceeds the kernel's limits", Hc, Wc, B); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste_shared(crops, Hc, Wc, mask_ori, M_c2o, img_ori, out, B, Ho, Wo, st); }, "paste_back_shared");
}

// The crop size of every crop entry point: a multiple of 4 (a thread owns four pixels of a row); the fp32 staging I_out exists for 256 and 512.
// Sets the error and returns nonzero otherwise.
static int check_dsize(const char* who, int dsize, const void* I_out)
{
    if (dsize < 4 || dsize % 4 || dsize > 16384) { cs_set_error("%s: dsize %d (a multiple of 4 from 4 to 16384)", who, dsize); return -1; }
    if (I_out && dsize != 256 && dsize != 512) { cs_set_error("%s: I_out goes with dsize 256 or 512 (got %d)", who, dsize); return -1; }
    return 0;
}

// ---- the crop in front of both chains (crop.py:429-455 per frame, cropper.py:196-209)
extern "C" int cs_crop_frames(cs_engine* e, int B, const uint8_t* frames, int Ho, int Wo, const double* M_o2c, int dsize, uint8_t* crops, float* I_out,
                              void* stream)
{
    if (!e || !frames || !M_o2c || !crops || B < 1 || Ho < 1 || Wo < 1) { cs_set_error("cs_crop_frames: bad arguments"); return -1; }
    if (check_dsize("cs_crop_frames", dsize, I_out)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_crop_batch(frames, Ho, Wo, M_o2c, nullptr, dsize, crops, I_out, B, st); }, "crop_frames");
}

// ---- several faces per frame: face b is cut from, and pasted into, frame frame_index[b]
// frame_index: B host ints, non-decreasing, in [0, F).  Sets the error and returns nonzero otherwise; nothing has been launched then.
static int check_frame_index(const char* who, const int* frame_index, int B, int F)
{
    for (int b = 0; b < B; ++b) {
        if (frame_index[b] < 0 || frame_index[b] >= F) {
            cs_set_error("%s: frame_index[%d] = %d outside [0, %d)", who, b, frame_index[b], F);
            return -1;
        }
        if (b && frame_index[b] < frame_index[b - 1]) {
            cs_set_error("%s: frame_index decreases at %d (%d after %d): the faces of a frame are contiguous, frames in order", who, b, frame_index[b],
                         frame_index[b - 1]);
            return -1;
        }
    }
    return 0;
}

extern "C" int cs_crop_faces(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const double* M_o2c,
                             int dsize, uint8_t* crops, float* I_out, void* stream)
{
    if (!e || !frames || !frame_index || !M_o2c || !crops || B < 1 || F < 1 || Ho < 1 || Wo < 1) {
        cs_set_error("cs_crop_faces: bad arguments (B = %d faces, F = %d frames)", B, F);
        return -1;
    }
    if (check_dsize("cs_crop_faces", dsize, I_out)) return -1;
    if (check_frame_index("cs_crop_faces", frame_index, B, F)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_crop_batch(frames, Ho, Wo, M_o2c, frame_index, dsize, crops, I_out, B, st); }, "crop_faces");
}

extern "C" int cs_paste_back_faces(cs_engine* e, int B, int F, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const int* frame_index,
                                   const double* M_c2o, const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream)
{
    // B == 0: no face at all, the frames are copied; crops, masks, index and matrices are then not read and may be NULL
    if (!e || !imgs_ori || !out || B < 0 || F < 1 || Ho < 1 || Wo < 1 || (B > 0 && (!crops || !masks_crop || !frame_index || !M_c2o || Hc < 1 || Wc < 1))) {
        cs_set_error("cs_paste_back_faces: bad arguments (B = %d faces, F = %d frames)", B, F);
        return -1;
    }
    if (check_frame_index("cs_paste_back_faces", frame_index, B, F)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste_faces(crops, masks_crop, Hc, Wc, M_c2o, frame_index, imgs_ori, out, B, F, Ho, Wo, st); },
                  "paste_back_faces");
}

// ---- the face mask from the parser's logits (can_swap_pipeline_e2e.py:183-190, can_swap_pipeline_v2i.py:76-83)
extern "C" int cs_face_masks(cs_engine* e, int B, int C, const float* logits, int h, int w, int scale, uint32_t valid_bits, uint8_t* masks,
                             uint8_t* labels, void* stream)
{
    if (!e || !logits) { cs_set_error("cs_face_masks: bad arguments"); return -1; }
    if (scale != 1 && scale != 2 && scale != 4) { cs_set_error("cs_face_masks: scale %d (1, 2 and 4 are built)", scale); return -1; }
    if (C < 1 || C > 32) { cs_set_error("cs_face_masks: %d classes outside [1, 32]", C); return -1; }
    if (B < 1 || h < 1 || w < 1) { cs_set_error("cs_face_masks: B = %d, h = %d, w = %d (each at least 1)", B, h, w); return -1; }
    if (!masks && !labels) { cs_set_error("cs_face_masks: both outputs are NULL"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_face_masks(logits, B, C, h, w, scale, valid_bits, masks, labels, st); }, "face_masks");
}

// ---- the parser's input (can_swap_pipeline_e2e.py:171 + :180, can_swap_pipeline_v2i.py:73): everything is refused before any launch
extern "C" int cs_parser_input(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, int halve, const float* lut, float* pixel_values,
                               uint8_t* resized_u8, void* stream)
{
    if (!e || !crops || !lut) { cs_set_error("cs_parser_input: NULL %s", !e ? "engine" : !crops ? "crops" : "lut"); return -1; }
    if (!pixel_values && !resized_u8) { cs_set_error("cs_parser_input: both outputs are NULL"); return -1; }
    if (B < 1 || Hc < 1 || Wc < 1) { cs_set_error("cs_parser_input: B = %d, Hc = %d, Wc = %d (each at least 1)", B, Hc, Wc); return -1; }
    if (halve != 0 && halve != 1) { cs_set_error("cs_parser_input: halve %d (0 or 1)", halve); return -1; }
    if (halve && ((Hc | Wc) & 1)) { cs_set_error("cs_parser_input: %dx%d crops cannot be halved (odd size)", Hc, Wc); return -1; }
    const long Ho = halve ? Hc : 2L * Hc, Wo = halve ? Wc : 2L * Wc;
    if (Ho > 16384 || Wo > 16384) { cs_set_error("cs_parser_input: output %ldx%ld above 16384 a side", Ho, Wo); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_parser_input(crops, B, Hc, Wc, halve, lut, pixel_values, resized_u8, st); }, "parser_input");
}

// ---- the side-by-side video frame (src/utils/video.py:84-109; can_swap_pipeline_e2e.py:290, can_swap_pipeline_v2i.py:328): everything is refused
// before any launch
extern "C" int cs_concat_frames(cs_engine* e, int B, int P, int S, const void* const* panels, const int* kinds, const int* shared, uint8_t* out,
                                void* stream)
{
    if (!e || !out || !panels || !kinds || !shared) {
        cs_set_error("cs_concat_frames: NULL %s", !e ? "engine" : !out ? "out" : !panels ? "panels" : !kinds ? "kinds" : "shared");
        return -1;
    }
    if (B < 1) { cs_set_error("cs_concat_frames: B = %d (at least 1)", B); return -1; }
    if (P < 1 || P > 4) { cs_set_error("cs_concat_frames: P = %d (1 to 4 panels)", P); return -1; }
    if (S < 4 || S % 4 || S > 16384) { cs_set_error("cs_concat_frames: S = %d (a multiple of 4 from 4 to 16384)", S); return -1; }
    for (int p = 0; p < P; ++p) {
        if (kinds[p] < 0 || kinds[p] > 3) { cs_set_error("cs_concat_frames: kind %d of panel %d (0 to 3)", kinds[p], p); return -1; }
        if (!panels[p]) { cs_set_error("cs_concat_frames: NULL panel %d", p); return -1; }
    }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_concat_frames(panels, kinds, shared, B, P, S, out, st); }, "concat_frames");
}

// ---- the face detector's input (scrfd.py:224-235, :154) and decode (scrfd.py:160-218, :239-303): everything is refused before any launch
extern "C" int cs_det_input(cs_engine* e, int F, const uint8_t* frames, int Ho, int Wo, int Hd, int Wd, int swap_rb, const float* lut, float* blob,
                            void* stream)
{
    if (!e || !frames || !lut || !blob) {
        cs_set_error("cs_det_input: NULL %s", !e ? "engine" : !frames ? "frames" : !lut ? "lut" : "blob");
        return -1;
    }
    if (F < 1 || Ho < 1 || Wo < 1) { cs_set_error("cs_det_input: F = %d, Ho = %d, Wo = %d (each at least 1)", F, Ho, Wo); return -1; }
    if (Hd < 1 || Wd < 1 || Hd > 16384 || Wd > 16384) { cs_set_error("cs_det_input: det size %dx%d (Hd x Wd) outside [1, 16384] a side", Hd, Wd); return -1; }
    int nh, nw;
    det_letterbox(Ho, Wo, Hd, Wd, &nh, &nw);
    if (nh < 1 || nw < 1) { cs_set_error("cs_det_input: a %dx%d frame resizes to %dx%d inside %dx%d (empty)", Ho, Wo, nh, nw, Hd, Wd); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_det_input(frames, F, Ho, Wo, Hd, Wd, swap_rb != 0, lut, blob, st); }, "det_input");
}

extern "C" int cs_det_decode(cs_engine* e, int F, int n_levels, const int* strides, int num_anchors, const void* const* outs, int Hd, int Wd,
                             float det_scale, float det_thresh, float nms_thresh, int max_num, int metric_max, int Ho, int Wo, int max_faces,
                             float* det, float* kps, int* count, void* stream)
{
    if (!e || !strides || !outs || !det || !count) {
        cs_set_error("cs_det_decode: NULL %s", !e ? "engine" : !strides ? "strides" : !outs ? "outs" : !det ? "det" : "count");
        return -1;
    }
    static const int S5[5] = {8, 16, 32, 64, 128};
    bool layout = (n_levels == 3 && num_anchors == 2) || (n_levels == 5 && num_anchors == 1);
    for (int l = 0; layout && l < n_levels; ++l) layout = strides[l] == S5[l];
    if (!layout) {
        cs_set_error("cs_det_decode: layout of %d levels with %d anchors is not 3 levels (8, 16, 32) x 2 or 5 levels (8 .. 128) x 1", n_levels, num_anchors);
        return -1;
    }
    if (F < 1 || Ho < 1 || Wo < 1) { cs_set_error("cs_det_decode: F = %d, Ho = %d, Wo = %d (each at least 1)", F, Ho, Wo); return -1; }
    if (Hd < 1 || Wd < 1 || Hd > 16384 || Wd > 16384) { cs_set_error("cs_det_decode: det size %dx%d (Hd x Wd) outside [1, 16384] a side", Hd, Wd); return -1; }
    if (max_faces < 1 || max_faces > CS_DET_MAX_FACES) { cs_set_error("cs_det_decode: max_faces %d outside [1, %d]", max_faces, CS_DET_MAX_FACES); return -1; }
    if (max_num < 0 || max_num > max_faces) { cs_set_error("cs_det_decode: max_num %d outside [0, max_faces = %d]", max_num, max_faces); return -1; }
    if (!(det_scale > 0.f) || det_scale > 3.0e38f) { cs_set_error("cs_det_decode: det_scale %g is not a positive finite number", (double)det_scale); return -1; }
    if (det_thresh != det_thresh || nms_thresh != nms_thresh) { cs_set_error("cs_det_decode: a threshold is NaN"); return -1; }
    int nk = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!outs[l] || !outs[n_levels + l]) { cs_set_error("cs_det_decode: NULL %s pointer of level %d", !outs[l] ? "score" : "bbox", l); return -1; }
        nk += outs[2 * n_levels + l] != nullptr;
    }
    if (nk != 0 && nk != n_levels) { cs_set_error("cs_det_decode: %d of %d kps pointers are NULL (all or none)", n_levels - nk, n_levels); return -1; }
    if (kps && !nk) { cs_set_error("cs_det_decode: kps output given without kps pointers in outs"); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] {
        return launch_det_decode(F, n_levels, strides, num_anchors, outs, Hd, Wd, det_scale, det_thresh, nms_thresh, max_num, metric_max != 0, Ho, Wo,
                                 max_faces, det, kps, count, st);
    }, "det_decode");
}

// What cs_lmk_input and cs_crop_lmk check alike, behind their NULL checks: sizes, the layout's indices, the crop's parameters, frame_index (B host
// ints in [0, F), any order).  Sets the error and returns nonzero; nothing has been launched then.
static int check_lmk_args(const char* who, int B, int F, int Ho, int Wo, const int* frame_index, int N, const cs_lmk_layout& layout, int dsize,
                          float scale, float vy_ratio, int status_mark)
{
    if (B < 1 || F < 1 || Ho < 1 || Wo < 1) { cs_set_error("%s: B = %d, F = %d, Ho = %d, Wo = %d (each at least 1)", who, B, F, Ho, Wo); return -1; }
    if (check_dsize(who, dsize, nullptr)) return -1;
    if (N < 1 || N > (1 << 20)) { cs_set_error("%s: N = %d landmarks outside [1, 2^20]", who, N); return -1; }
    if (layout.n_eye < 1 || layout.n_eye > 4) { cs_set_error("%s: layout.n_eye %d outside [1, 4]", who, layout.n_eye); return -1; }
    for (int i = 0; i < layout.n_eye; ++i)
        if (layout.left[i] < 0 || layout.left[i] >= N || layout.right[i] < 0 || layout.right[i] >= N) {
            cs_set_error("%s: layout eye index %d (%d, %d) outside [0, N = %d)", who, i, layout.left[i], layout.right[i], N);
            return -1;
        }
    if (layout.lip[0] < 0 || layout.lip[0] >= N || layout.lip[1] < 0 || layout.lip[1] >= N) {
        cs_set_error("%s: layout lip indices (%d, %d) outside [0, N = %d)", who, layout.lip[0], layout.lip[1], N);
        return -1;
    }
    if (!(scale > 0.f) || scale > 3.0e38f) { cs_set_error("%s: scale %g is not a positive finite number", who, (double)scale); return -1; }
    if (!(fabsf(vy_ratio) <= 3.0e38f)) { cs_set_error("%s: vy_ratio %g is not finite", who, (double)vy_ratio); return -1; }
    if (status_mark == 0) { cs_set_error("%s: status_mark 0 (a refused face is marked with a non-zero value)", who); return -1; }
    for (int b = 0; b < B; ++b)
        if (frame_index[b] < 0 || frame_index[b] >= F) {
            cs_set_error("%s: frame_index[%d] = %d outside [0, %d)", who, b, frame_index[b], F);
            return -1;
        }
    return 0;
}

// ---- the landmark runner's input (human_landmark_runner.py:62, :76) and decode (:82-83): everything is refused before any launch; neither call
// uses engine scratch or synchronises, B and F are not bound by max_batch
extern "C" int cs_lmk_input(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N,
                            cs_lmk_layout layout, int dsize, float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M, float* inp,
                            uint8_t* crops, int* status, void* stream)
{
    if (!e || !frames || !frame_index || !lmk || !M || !inp || !status) {
        cs_set_error("cs_lmk_input: NULL %s", !e ? "engine" : !frames ? "frames" : !frame_index ? "frame_index" : !lmk ? "lmk" : !M ? "M" : !inp ? "inp" : "status");
        return -1;
    }
    if (check_lmk_args("cs_lmk_input", B, F, Ho, Wo, frame_index, N, layout, dsize, scale, vy_ratio, status_mark)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] {
        return launch_lmk_input(frames, Ho, Wo, frame_index, lmk, N, layout, dsize, scale, vy_ratio, flag_do_rot != 0, status_mark, M, inp, crops, status,
                                B, st);
    }, "lmk_input");
}

extern "C" int cs_lmk_decode(cs_engine* e, int B, const float* out_pts, int Np, const float* M, int dsize, const int* status, float* lmk, void* stream)
{
    if (!e || !out_pts || !M || !status || !lmk) {
        cs_set_error("cs_lmk_decode: NULL %s", !e ? "engine" : !out_pts ? "out_pts" : !M ? "M" : !status ? "status" : "lmk");
        return -1;
    }
    if (B < 1 || Np < 1 || Np > (1 << 20)) { cs_set_error("cs_lmk_decode: B = %d, Np = %d (B at least 1, Np in [1, 2^20])", B, Np); return -1; }
    if (check_dsize("cs_lmk_decode", dsize, nullptr)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_lmk_decode(out_pts, Np, M, dsize, status, lmk, B, st); }, "lmk_decode");
}

// ---- 4:2:0 frames <-> RGB frames (include/canonswap_yuv.h): everything is refused before any launch; neither call uses engine scratch or
// synchronises, F is not bound by max_batch
static int yuv_check(const char* who, cs_engine* e, int F, const uint8_t* yuv, const uint8_t* rgb, int Ho, int Wo, int layout, int matrix, int full_range)
{
    if (!e || !yuv || !rgb) { cs_set_error("%s: NULL %s", who, !e ? "engine" : !yuv ? "yuv" : "rgb"); return -1; }
    if (F < 1) { cs_set_error("%s: F = %d (at least 1)", who, F); return -1; }
    if (Ho < 2 || Ho % 2 || Ho > 16384) { cs_set_error("%s: Ho = %d (an even number from 2 to 16384)", who, Ho); return -1; }
    if (Wo < 2 || Wo % 2 || Wo > 16384) { cs_set_error("%s: Wo = %d (an even number from 2 to 16384)", who, Wo); return -1; }
    if (layout != 0 && layout != 1) { cs_set_error("%s: layout %d (0: NV12, 1: I420)", who, layout); return -1; }
    if (matrix != 0 && matrix != 1) { cs_set_error("%s: matrix %d (0: BT.601, 1: BT.709)", who, matrix); return -1; }
    if (full_range != 0 && full_range != 1) { cs_set_error("%s: full_range %d (0 or 1)", who, full_range); return -1; }
    const uintptr_t px = (uintptr_t)F * Ho * Wo, y0 = (uintptr_t)yuv, r0 = (uintptr_t)rgb;
    if (y0 < r0 + px * 3 && r0 < y0 + px + px / 2) { cs_set_error("%s: rgb and yuv overlap", who); return -1; }
    return 0;
}

extern "C" int cs_yuv_to_rgb(cs_engine* e, int F, const uint8_t* yuv, int Ho, int Wo, int layout, int matrix, int full_range, uint8_t* rgb, void* stream)
{
    if (yuv_check("cs_yuv_to_rgb", e, F, yuv, rgb, Ho, Wo, layout, matrix, full_range)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_yuv_to_rgb(yuv, F, Ho, Wo, layout, matrix, full_range, rgb, st); }, "yuv_to_rgb");
}

extern "C" int cs_rgb_to_yuv(cs_engine* e, int F, const uint8_t* rgb, int Ho, int Wo, int layout, int matrix, int full_range, int keep, uint8_t* yuv,
                             void* stream)
{
    if (yuv_check("cs_rgb_to_yuv", e, F, yuv, rgb, Ho, Wo, layout, matrix, full_range)) return -1;
    if (keep != 0 && keep != 1) { cs_set_error("cs_rgb_to_yuv: keep %d (0 or 1)", keep); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_rgb_to_yuv(rgb, F, Ho, Wo, layout, matrix, full_range, keep, yuv, st); }, "rgb_to_yuv");
}

// ---- getid on the engine (can_swap_e2e.py:102-107): nearest resize to 112 x 112, the ArcFace network, L2 normalisation.  Everything is refused
// before any launch; more than the workspace's images run as several passes.
static int identity_impl(cs_engine* e, const char* who, int B, const float* img, const uint8_t* u8, const float* lut, int H, int W, float* id_out,
                         float* raw_out, void* stream)
{
    if (!e) { cs_set_error("%s: NULL engine", who); return -1; }
    if (!e->finalized) { cs_set_error("%s: cs_finalize_weights has not been called", who); return -1; }
    if (!e->idn.present) { cs_set_error("%s: the engine holds no identity network (no 'A.*' blobs: pass the 'arcface' state-dict)", who); return -1; }
    if (B < 1 || B > e->maxB) { cs_set_error("%s: batch %d outside [1, %d]", who, B, e->maxB); return -1; }
    if (!img && !u8) { cs_set_error("%s: NULL input", who); return -1; }
    if (u8 && !lut) { cs_set_error("%s: NULL lut", who); return -1; }
    if (H < 1 || W < 1 || H > 16384 || W > 16384) { cs_set_error("%s: H = %d, W = %d (each from 1 to 16384)", who, H, W); return -1; }
    if (!id_out && !raw_out) { cs_set_error("%s: both outputs are NULL", who); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    IdNet& A = e->idn;
    for (int b0 = 0; b0 < B; b0 += A.cap) {
        const int nb = B - b0 < A.cap ? B - b0 : A.cap;
        const size_t ofs = (size_t)b0 * 3 * H * W;
        TRY(e->run(1, st, [&] { return launch_id_input(img ? img + ofs : nullptr, u8 ? u8 + ofs : nullptr, lut, A.in16, nb, H, W, st); }, "id_input"));
        TRY(e->run(1, st, [&] { return idnet_forward(A, nb, id_out ? id_out + (size_t)b0 * 512 : nullptr, raw_out ? raw_out + (size_t)b0 * 512 : nullptr, st); },
                   "identity"));
    }
    return 0;
}

extern "C" int cs_identity(cs_engine* e, int B, const float* img, int H, int W, float* id_out, float* raw_out, void* stream)
{
    return identity_impl(e, "cs_identity", B, img, nullptr, nullptr, H, W, id_out, raw_out, stream);
}

extern "C" int cs_identity_u8(cs_engine* e, int B, const uint8_t* crops, int H, int W, const float* lut, float* id_out, float* raw_out, void* stream)
{
    return identity_impl(e, "cs_identity_u8", B, nullptr, crops, lut, H, W, id_out, raw_out, stream);
}

// ---- the SegFormer face parser on the engine (can_swap_pipeline_e2e.py:178-182: model(pixel_values).logits): pixel_values fp32 NCHW -> logits fp32
// [B][L][H / 4][W / 4].  Everything is refused before any launch; more than the workspace's images run as several passes.
extern "C" int cs_parser(cs_engine* e, int B, const float* pixel_values, int H, int W, float* logits_out, void* stream)
{
    if (!e) { cs_set_error("cs_parser: NULL engine"); return -1; }
    if (!e->finalized) { cs_set_error("cs_parser: cs_finalize_weights has not been called"); return -1; }
    if (!e->psr.present) { cs_set_error("cs_parser: the engine holds no face parser (no 'P.*' blobs: pass the 'parser' state-dict)"); return -1; }
    if (B < 1 || B > e->maxB) { cs_set_error("cs_parser: batch %d outside [1, %d]", B, e->maxB); return -1; }
    if (!pixel_values || !logits_out) { cs_set_error("cs_parser: NULL pointer"); return -1; }
    ParserNet& P = e->psr;
    if (H < 32 || W < 32 || H % 32 || W % 32) { cs_set_error("cs_parser: H = %d, W = %d (each a multiple of 32)", H, W); return -1; }
    if ((long)H * W > (long)P.maxH * P.maxW) { cs_set_error("cs_parser: %d x %d exceeds the workspace's %d x %d", H, W, P.maxH, P.maxW); return -1; }
    if ((H / 32) * (W / 32) > 256) { cs_set_error("cs_parser: %d keys per stage (at most 256: inputs up to 512 x 512)", (H / 32) * (W / 32)); return -1; }
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += P.cap) {
        const int nb = B - b0 < P.cap ? B - b0 : P.cap;
        TRY(e->run(1, st, [&] { return launch_p_input(pixel_values + (size_t)b0 * 3 * H * W, P.in16, nb, H, W, st); }, "parser_input16"));
        TRY(e->run(1, st, [&] { return parser_forward(P, nb, H, W, logits_out + (size_t)b0 * P.L * (H / 4) * (W / 4), st); }, "parser"));
    }
    return 0;
}

// ---- the crop and the paste-back from landmarks and matrices on the device (include/canonswap_device_crop.h): everything is refused before any
// launch; neither call uses engine scratch or synchronises
extern "C" int cs_dcrop_abi_version(void) { return CS_DCROP_ABI_VERSION; }

extern "C" int cs_crop_lmk(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const float* lmk, int N,
                           const cs_lmk_layout* layout, int dsize, float scale, float vy_ratio, int flag_do_rot, int status_mark, float* M,
                           uint8_t* crops, float* I_out, float* lmk_crop, int* status, void* stream)
{
    if (!e || !frames || !frame_index || !lmk || !layout || !M || !crops || !status) {
        cs_set_error("cs_crop_lmk: NULL %s", !e ? "engine" : !frames ? "frames" : !frame_index ? "frame_index" : !lmk ? "lmk" : !layout ? "layout" :
                     !M ? "M" : !crops ? "crops" : "status");
        return -1;
    }
    if (check_lmk_args("cs_crop_lmk", B, F, Ho, Wo, frame_index, N, *layout, dsize, scale, vy_ratio, status_mark)) return -1;
    if (check_dsize("cs_crop_lmk", dsize, I_out)) return -1;      // behind the other checks, as before: dsize itself has passed
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] {
        return launch_crop_lmk(frames, Ho, Wo, frame_index, lmk, N, *layout, dsize, scale, vy_ratio, flag_do_rot != 0, status_mark, M, crops, I_out,
                               lmk_crop, status, B, st);
    }, "crop_lmk");
}

extern "C" int cs_paste_back_faces_dev(cs_engine* e, int B, int F, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const int* frame_index,
                                       const float* M, const int* status, const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream)
{
    // B == 0: no face at all, the frames are copied; crops, masks, index, matrices and status are then not read and may be NULL
    if (!e || !imgs_ori || !out) { cs_set_error("cs_paste_back_faces_dev: NULL %s", !e ? "engine" : !imgs_ori ? "imgs_ori" : "out"); return -1; }
    if (B > 0 && (!crops || !masks_crop || !frame_index || !M)) {
        cs_set_error("cs_paste_back_faces_dev: NULL %s", !crops ? "crops" : !masks_crop ? "masks_crop" : !frame_index ? "frame_index" : "M");
        return -1;
    }
    if (B < 0 || F < 1 || Ho < 1 || Wo < 1 || (B > 0 && (Hc < 1 || Wc < 1))) {
        cs_set_error("cs_paste_back_faces_dev: B = %d faces, F = %d frames, Hc = %d, Wc = %d, Ho = %d, Wo = %d", B, F, Hc, Wc, Ho, Wo);
        return -1;
    }
    if (check_frame_index("cs_paste_back_faces_dev", frame_index, B, F)) return -1;
    DevGuard guard(e->dev);
    hipStream_t st = (hipStream_t)stream;
    return e->run(1, st, [&] { return launch_paste_faces_dev(crops, masks_crop, Hc, Wc, M, status, frame_index, imgs_ori, out, B, F, Ho, Wo, st); },
                  "paste_back_faces_dev");
}
