/* canonswap_hip.h -- C ABI of the MI355X (gfx950) CanonSwap generator engine.
 *
 * The reference has no FFI: its boundary for this path is the Python class `can_swapper`
 * (src/can_swap_e2e.py:39) whose stage methods/attributes the pipeline calls once per frame
 * (src/can_swap_pipeline_e2e.py:242-263).  Every entry point below replaces one of those calls and keeps
 * its tensor signature: all tensors are caller-owned, contiguous fp32 device buffers in the reference's
 * NCHW / NCDHW layouts, passed as raw pointers (`tensor.data_ptr()`), and all work is enqueued on the
 * caller's HIP stream (`torch.cuda.current_stream().cuda_stream`).  The engine owns its packed weights,
 * per-identity modulated weights and workspace; nothing it allocates is returned.
 *
 * Error convention: every function returns 0 on success, non-zero on failure with a message available
 * from cs_last_error() (thread local).  No C++ exception crosses this boundary.
 * Threading: an engine is bound to one device and is not thread-safe.
 */
#ifndef CANONSWAP_HIP_H
#define CANONSWAP_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cs_engine cs_engine;

/* ---- life cycle (replaces can_swapper.__init__ / load_cpk, src/can_swap_e2e.py:44-100) */
int cs_create(int device_id, int max_batch, cs_engine** out);   /* 1 <= max_batch <= 84 (32-bit element offsets inside one tensor); workspace ~0.37 GB per frame of batch; 64 is the fastest launch size (profiles/r05_b_batch_sweep.txt) */
void cs_destroy(cs_engine* e);
const char* cs_last_error(void);
#define CS_ABI_VERSION 4       /* bumped whenever a struct of this header, an entry point's meaning or the weight blob format changes */
int cs_abi_version(void);
/* Upload one packed weight blob (host pointer).  Names/layouts are produced by canonswap_amd/pack.py from
 * the reference's state-dict keys (BatchNorm / spectral norm folded, channels-last, fp16 MFMA order). */
int cs_upload(cs_engine* e, const char* name, const void* host_ptr, size_t nbytes);
int cs_finalize_weights(cs_engine* e);
/* Per-identity precompute of the 14 modulated+demodulated conv weights of T
 * (AdaptiveSharedWeightConv2d.forward, src/modules/adaptive_modulate.py:148-155).  id: device, 512 fp32. */
#define CS_MAX_IDENTITY_SLOTS 8
/* slot in [0, CS_MAX_IDENTITY_SLOTS): each slot keeps its own 14 modulated weight sets (about 132 MB), so several source
 * identities stay resident (concurrent streams, BASELINE configs[4]) and may be mixed inside one batch (cs_swap_ids). */
int cs_set_identity(cs_engine* e, int slot, const float* id, void* stream);

/* can_swapper.getid (can_swap_e2e.py:102-107; the network: models/arcface_models.py:66-136, ResNet(IRBlock, [3, 4, 14, 3], use_se=True)):
 * img fp32 Bx3xHxW (any H, W >= 1; the pipeline passes ID_transform's values, can_swap_pipeline_e2e.py:43-46,97-98) -> F.interpolate(size=(112, 112)),
 * nearest -> the network -> id_out Bx512 = F.normalize(raw, p=2, dim=1), raw_out Bx512 = the network's first output (its second, the pooled layer-3
 * map, is never computed).  Either output may be NULL, not both.  B <= max_batch; needs the optional "A.*" blobs (pack.py: the "arcface"
 * state-dict) and fails without them.  Deterministic, and a row's bits do not depend on the batch it is part of.  id_out can be handed to
 * cs_set_identity on the same stream.  The calls use a workspace of their own (allocated by cs_finalize_weights when the blobs are there, for
 * min(max_batch, 8) images per pass; larger batches run as several passes), not the generator's scratch: they may be enqueued beside any other
 * entry point of the engine, but two identity calls on one engine must be ordered with each other. */
int cs_identity(cs_engine* e, int B, const float* img, int H, int W, float* id_out, float* raw_out, void* stream);
/* The same from aligned uint8 crops BxHxWx3 (can_swap_pipeline_e2e.py:97: ID_transform = ToTensor + Normalize, then getid): lut fp32 [3][256] on the
 * device holds what the transform makes of byte v in channel c (canonswap_amd/tail.py id_lut); bit-equal to cs_identity on the table's values. */
int cs_identity_u8(cs_engine* e, int B, const uint8_t* crops, int H, int W, const float* lut, float* id_out, float* raw_out, void* stream);

/* The SegFormer face parser on the engine (can_swap_pipeline_e2e.py:178-182, can_swap_pipeline_v2i.py:73-76: model(pixel_values).logits): needs the
 * optional "P.*" blobs (pack.py _pack_P, from the "parser" state-dict).  pixel_values fp32 Bx3xHxW on the device (what cs_parser_input writes), H and W
 * multiples of 32 up to 512 x 512 -> logits_out fp32 BxLx(H/4)x(W/4), the tensor cs_face_masks takes.  Everything is checked before any launch.  The
 * call uses a workspace of its own (allocated by cs_finalize_weights when the blobs are there, for min(max_batch, 8) images of 512 x 512 per pass;
 * larger batches run as several passes), not the generator's scratch: it may be enqueued beside any other entry point of the engine, but two parser
 * calls on one engine must be ordered with each other. */
int cs_parser(cs_engine* e, int B, const float* pixel_values, int H, int W, float* logits_out, void* stream);

/* Single-frame latency mode (BASELINE configs[1]): launches that cannot fill the 256 CUs at one or two frames per call take forms that
 * add an output element's products in another (fixed) order than the batched path - the 512-channel 3x3 convs split their K loop over twelve waves
 * of a workgroup (conv_lat.hip), the deep hourglass levels over workgroups (split-K), R's volume convs emit 2-row statistics blocks.  Deterministic,
 * the same tolerance against the reference (>= 50 dB), not bit-identical with the default mode - which is why it is opt-in: the DEFAULT mode never
 * picks a summation order by batch size, so there a frame's bits do not depend on the batch it is part of.  That guarantee does NOT hold inside
 * latency mode: conv_lat and the split-K forms are taken per launch by its workgroup count (N x tiles <= 256), so a frame run at B = 2 in this mode
 * may differ in its last bits from the same frame at B = 1 (both deterministic, both inside the tolerance). */
int cs_set_latency_mode(cs_engine* e, int on);

/* ---- stage calls; B frames per call, B <= max_batch --------------------------------------------------- */
/* can_swapper.extract_feature_3d (can_swap_e2e.py:165-172): img Bx3x256x256 -> f Bx32x16x64x64 */
int cs_extract_feature_3d(cs_engine* e, int B, const float* img, float* f_out, void* stream);
/* WarpingNetwork.warp(feature_3d, kp_source, kp_driving) (warping_network.py:49-62):
 * f Bx32x16x64x64, kp Bx21x3 -> f_out Bx32x16x64x64, occ_out Bx1x64x64 */
int cs_warp(cs_engine* e, int B, const float* f, const float* kp_source, const float* kp_driving, float* f_out,
            float* occ_out, void* stream);
/* WarpingNetwork.warp_out(out, occlusion_map) (warping_network.py:64-71): -> seg Bx256x64x64; occ may be NULL */
int cs_warp_out(cs_engine* e, int B, const float* f, const float* occ, float* seg_out, void* stream);
/* transfer_model2.forward(x, dlatents) == can_swapper.swap (adaptive_modulate.py:522-554), identity from slot */
int cs_swap(cs_engine* e, int slot, int B, const float* f, float* f_out, void* stream);
/* the same with one identity slot per sample (slots: B host ints): the reference's per-sample dlatents, i.e. the groups=N
 * modulated convolution of AdaptiveSharedWeightConv2d.forward (adaptive_modulate.py:157-167) */
int cs_swap_ids(cs_engine* e, const int* slots, int B, const float* f, float* f_out, void* stream);
/* G3d.forward (adaptive_modulate.py:721-733) */
int cs_refine(cs_engine* e, int B, const float* f, float* f_out, void* stream);
/* WarpingNetwork.forward(feature_3d, kp_driving=, kp_source=) (warping_network.py:83-111):
 * any of occ_out (Bx1x64x64), deformation_out (Bx16x64x64x3), seg_out (Bx256x64x64) may be NULL */
int cs_warp_forward(cs_engine* e, int B, const float* f, const float* kp_driving, const float* kp_source,
                    float* occ_out, float* deformation_out, float* seg_out, void* stream);
/* SPADEDecoder.forward (spade_generator.py:41-59): seg Bx256x64x64 -> img Bx3x512x512 in (0,1) */
int cs_spade_decode(cs_engine* e, int B, const float* seg, float* img_out, void* stream);
/* MotionExtractor.forward (motion_extractor.py:33-35 -> convnextv2.py:110-144), as called by can_swapper.get_kp_info
 * (can_swap_e2e.py:174-199): img Bx3x256x256 fp32 in [0,1] -> out Bx328 fp32, the raw head outputs concatenated in the order
 * kp(63) scale(1) pitch(66) yaw(66) roll(66) t(3) exp(63).  Needs the "M.*" blobs. */
int cs_motion_extract(cs_engine* e, int B, const float* img, float* out, void* stream);
/* can_swapper.parse_output on device (can_swap_e2e.py:314-322): Bx3xHxW fp32 -> BxHxWx3 u8 (truncation) */
int cs_pack_u8(cs_engine* e, int B, const float* img, uint8_t* out, int H, int W, void* stream);
/* can_swapper.prepare_source / prepare_videos on device (can_swap_e2e.py:126-163): BxHxWx3 u8 -> Bx3xHxW fp32 = u8 / 255 */
int cs_unpack_u8(cs_engine* e, int B, const uint8_t* img, float* out, int H, int W, void* stream);
/* The whole per-frame loop body (can_swap_pipeline_e2e.py:242-263) for B frames without leaving the device:
 * img Bx3x256x256, x_t / x_can Bx21x3.  out_f32 (Bx3x512x512), out_u8 (Bx512x512x3), rec_can, swap_can
 * (debug decodes of lines 248 / 257, Bx3x512x512) may each be NULL. */
int cs_swap_frames(cs_engine* e, int slot, int B, const float* img, const float* x_t, const float* x_can,
                   float* out_f32, uint8_t* out_u8, float* rec_can, float* swap_can, void* stream);
/* cs_swap_frames with one identity slot per frame (slots: B host ints) */
int cs_swap_frames_ids(cs_engine* e, const int* slots, int B, const float* img, const float* x_t, const float* x_can,
                       float* out_f32, uint8_t* out_u8, float* rec_can, float* swap_can, void* stream);
/* The per-frame body of the video-to-image pipeline (can_swap_pipeline_v2i.py:311-312):
 * warp_decode(f, kp_source, kp_driving) -> 3x512x512 for B driving frames.  f: nf x 32x16x64x64 feature volumes and
 * kp_source: ns x 21x3, with nf / ns = 1 (one swapped canonical volume / key-point set shared by all frames) or B;
 * kp_driving Bx21x3.  out_f32 (Bx3x512x512) and out_u8 (Bx512x512x3) may each be NULL. */
int cs_animate_frames(cs_engine* e, int B, const float* f, int nf, const float* kp_source, int ns, const float* kp_driving,
                      float* out_f32, uint8_t* out_u8, void* stream);

/* ---- image-space steps on either side of the generator; all buffers on the device ---- */
/* SoftErosion.forward (src/utils/crop.py:21-47; the pipeline builds it with kernel_size 21, threshold 0.9, iterations 3 / 2,
 * can_swap_pipeline_e2e.py:42, _v2i.py:43): mask BxHxW fp32 (0/1) -> soft_out BxHxW fp32, hard_out BxHxW u8 (may be NULL).
 * w: the ksize x ksize fp32 kernel (crop.py:29-35), built by the caller exactly as the reference builds it.  ksize 21 or 15, iters >= 1,
 * any H, W >= 1; B from 1 to 65535 (the maximum is taken over the whole BxHxW tensor, as the module does); the engine's scratch grows to
 * the largest B x H x W seen, independently of cs_create's max_batch. */
int cs_soft_erosion(cs_engine* e, int B, int H, int W, const float* mask, const float* w, int ksize, float thr, int iters,
                    float* soft_out, uint8_t* hard_out, void* stream);
/* Input staging (src/utils/cropper.py:209 + can_swap_e2e.py:126-163): uint8 crops BxHcxWcx3, 512x512 (cv2.resize to 256x256 with
 * INTER_AREA = 2x2 means, (a+b+c+d+2)>>2) or 256x256 -> Bx3x256x256 fp32 = u8 / 255 */
int cs_prepare_crops(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, float* out, void* stream);
/* cv2.warpAffine(src, M, dsize=(Wd, Hd), flags=INTER_LINEAR), BORDER_CONSTANT 0 (src/utils/crop.py:49-63 _transform_img):
 * M: host, 2x3 row major, source -> destination.  8-bit 3-channel and float 1-channel images. */
int cs_warp_affine_u8(cs_engine* e, const uint8_t* src, int Hs, int Ws, const double M[6], uint8_t* dst, int Hd, int Wd, void* stream);
int cs_warp_affine_f32(cs_engine* e, const float* src, int Hs, int Ws, const double M[6], float* dst, int Hd, int Wd, void* stream);
/* paste_back (src/utils/crop.py:523-529) fused with the mask warp of prepare_paste_back (:515-521): crop HcxWcx3 u8, the soft mask
 * either in the crop frame (mask_crop HcxWc, warped here) or already in the frame of the original image (mask_ori HoxWo) - exactly
 * one of the two -, M_c2o 2x3 (crop -> original), img_ori / out HoxWox3 u8:
 * out = clip(mask * warp(crop) + (1 - mask) * img_ori, 0, 255) truncated to 8 bits */
int cs_paste_back(cs_engine* e, const uint8_t* crop, const float* mask_crop, const float* mask_ori, int Hc, int Wc,
                  const double M_c2o[6], const uint8_t* img_ori, uint8_t* out, int Ho, int Wo, void* stream);

/* The same steps for the B frames of one launch of the per-frame loop (can_swap_pipeline_e2e.py:273-283 runs them frame by frame):
 * cs_soft_erosion_frames = B independent SoftErosion calls on (1,1,H,W) masks - the maximum of crop.py:45 is taken per frame, as in the
 * pipeline's loop, not over the batch; masks: BxHxW, fp32 or (masks_u8 != 0) uint8 0/1 labels (`torch.isin(labels, valid).to(int)`,
 * can_swap_pipeline_e2e.py:192); the limits of cs_soft_erosion (B up to 65535, not bound to max_batch).  cs_paste_back_batch = prepare_paste_back + paste_back of B frames in one launch: crops BxHcxWcx3 u8
 * (the generator's frames), masks_crop BxHcxWc fp32 (the soft masks, in the crop frame), M_c2o: HOST, B x 6 doubles (2x3 row major, crop ->
 * original, target_M_c2o_lst[i]), imgs_ori / out BxHoxWox3 u8. */
int cs_soft_erosion_frames(cs_engine* e, int B, int H, int W, const void* masks, int masks_u8, const float* w, int ksize, float thr, int iters,
                           float* soft_out, uint8_t* hard_out, void* stream);
int cs_paste_back_batch(cs_engine* e, int B, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const double* M_c2o,
                        const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream);
/* Key-points of B frames from cs_motion_extract's raw head outputs, on the device: get_kp_info's refinement (can_swap_e2e.py:192-197,
 * camera.py:14-28), get_rotation_matrix (camera.py:31-73) and transform_keypoint (can_swap_e2e.py:228-256) -> x_t Bx21x3
 * = scale (kp R + exp) + t_xy, and x_can = scale kp Bx21x3 (can_swap_pipeline_e2e.py:243); rot (Bx3x3, may be NULL) = R.
 * Replaces make_motion_template's per-frame D2H of seven tensors (can_swap_pipeline_e2e.py:111-125). */
int cs_motion_keypoints(cs_engine* e, int B, const float* raw, float* x_t, float* x_can, float* rot, void* stream);

/* ---- the device-side frame of the video-to-image pipeline around cs_animate_frames (can_swap_pipeline_v2i.py; chain.py AnimateChain) ---- */
/* F.interpolate(img, size=(H/2, W/2), mode="bilinear", align_corners=False) at exactly one half (can_swap_pipeline_v2i.py:294, swap_can
 * 512 -> 256): img BxCxHxW fp32 -> out BxCx(H/2)x(W/2) fp32, H and W even.  The source coordinate of output i is 2i + 0.5, all four weights are
 * 1/4; the summation order is the one of the GPU kernel the reference executes: out = 0.25f * ((a + b) + (c + d)), a b the upper row's
 * two pixels, c d the lower row's. */
int cs_resize_half_bilinear(cs_engine* e, int B, int C, const float* img, int H, int W, float* out, void* stream);
/* The driven key-points of B driving frames (can_swap_pipeline_v2i.py:301-305): raw_driving Bx328 (cs_motion_extract's raw heads of the
 * driving frames; only their exp is read), raw_pose 1x328 (the raw heads of the SOURCE crop: its scale, its three 66-bin pose logits, its
 * t), kp 21x3 (x_swap_info['kp'], the canonical key-points of the swapped canonical image) -> x_t Bx21x3:
 * x_t[b] = scale_pose * (kp @ R_pose + exp[b]) + (t_x, t_y, 0)   (t_swap[..., 2].fill_(0), :303), R_pose formed as in cs_motion_keypoints. */
int cs_motion_keypoints_driven(cs_engine* e, int B, const float* raw_driving, const float* raw_pose, const float* kp, float* x_t, void* stream);
/* paste_back of B generated frames into ONE source image (src/utils/crop.py:523-529 as the loop of can_swap_pipeline_v2i.py:317-321 calls
 * it, on a fresh copy of the image per frame): crops BxHcxWcx3 u8, mask_ori HoxWo fp32 (the soft mask already in the image's frame:
 * cs_warp_affine_f32 = prepare_paste_back, can_swap_pipeline_v2i.py:255-258), M_c2o 2x3 (host), img_ori HoxWox3 u8 -> out BxHoxWox3 u8,
 * out[b] bit-equal to cs_paste_back of crops[b] with mask_ori given.  Coordinates, tap weights, the mask value and the image's pixels are
 * formed once per pixel group and reused for every frame; any B >= 1 (not bound to max_batch). */
int cs_paste_back_shared(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, const float* mask_ori, const double M_c2o[6],
                         const uint8_t* img_ori, uint8_t* out, int Ho, int Wo, void* stream);

/* ---- the crop in front of both chains ---- */
/* crop_image's image step (src/utils/crop.py:429-455, called per frame by src/utils/cropper.py:196-209; the landmark runner's 224x224 crop,
 * human_landmark_runner.py:62, is the same call) for B frames in one launch: crops[b] = cv2.warpAffine(frames[b], M_o2c[b], (dsize, dsize),
 * INTER_LINEAR), BORDER_CONSTANT 0, bit-equal to cs_warp_affine_u8 of that frame.  frames BxHoxWox3 u8; M_o2c: HOST, B x 6 doubles (2x3 row
 * major, original -> crop: the matrices of canonswap_amd/crop.py crop_matrices, or a caller's own = crop_image_mo2c); crops B x dsize x dsize x 3 u8,
 * dsize a multiple of 4 from 4 to 16384.  I_out (NULL, or Bx3x256x256 fp32; dsize 256 or 512 only): what cs_prepare_crops makes of the crops
 * (cropper.py:209 + can_swap_e2e.py:126-163), bit-equal, written from the same registers instead of a second pass.  Any B >= 1 (not bound to
 * max_batch). */
int cs_crop_frames(cs_engine* e, int B, const uint8_t* frames, int Ho, int Wo, const double* M_o2c, int dsize, uint8_t* crops, float* I_out,
                   void* stream);

/* ---- several faces per frame: the crop and the paste-back under a frame index ---- */
/* B faces in F frames.  frame_index: HOST, B ints, non-decreasing, each in [0, F): face b is cut from, and pasted into, frame frame_index[b]; the
 * faces of one frame are contiguous and their order is the paste order; a frame may own no face (F > B is fine).  The reference ships the
 * detector wrapper that returns every face of a frame (insightface_func/face_detect_crop_multi.py:63-99); its pipelines run the steps below once
 * per frame with one face.
 * cs_crop_faces = cs_crop_frames with the source frame named per crop (src/utils/crop.py:429-455 per face): crops[b] = cv2.warpAffine(
 * frames[frame_index[b]], M_o2c[b], (dsize, dsize), INTER_LINEAR), bit-equal to cs_crop_frames on the gathered frames and to cs_warp_affine_u8;
 * frames FxHoxWox3 u8, M_o2c HOST B x 6 doubles, crops B x dsize x dsize x 3 u8, I_out NULL or Bx3x256x256 fp32 (= cs_prepare_crops of the crops;
 * dsize 256 or 512 only); dsize a multiple of 4 from 4 to 16384.  B >= 1.
 * cs_paste_back_faces = prepare_paste_back + paste_back (src/utils/crop.py:515-529) applied once per face, in order, each on the result of the
 * one before: out = imgs_ori; for b: out[f] = paste_back(crops[b], M_c2o[b], out[f], prepare_paste_back(masks_crop[b], M_c2o[b])), f =
 * frame_index[b] - bit-equal to that sequence of cs_paste_back calls (the frame is truncated to 8 bits after every face), and for frame_index =
 * 0 .. B-1 to cs_paste_back_batch - in one pass over every frame: the frames between two faces never exist in memory.  crops BxHcxWcx3 u8, masks_crop
 * BxHcxWc fp32, M_c2o HOST B x 6 doubles, imgs_ori / out FxHoxWox3 u8.  A frame without a face is copied.  out may BE imgs_ori (in place: a frame
 * without a face is then not touched); any other overlap of out with an input is not allowed.  B == 0 with F >= 1 copies the frames (crops,
 * masks_crop, frame_index and M_c2o are then not read).  One launch takes 48 faces and as many frames; neither B nor F is bound to that or to
 * max_batch (more are further launches on the stream, a frame's faces may span two of them).
 * Both return nonzero with cs_last_error() set, before anything is launched, for a NULL pointer, F < 1, B < 1 (cs_paste_back_faces: B < 0), an
 * index outside [0, F), a decreasing index, and cs_crop_frames' rules for dsize and I_out. */
int cs_crop_faces(cs_engine* e, int B, int F, const uint8_t* frames, int Ho, int Wo, const int* frame_index, const double* M_o2c,
                  int dsize, uint8_t* crops, float* I_out, void* stream);
int cs_paste_back_faces(cs_engine* e, int B, int F, const uint8_t* crops, const float* masks_crop, int Hc, int Wc, const int* frame_index,
                        const double* M_c2o, const uint8_t* imgs_ori, uint8_t* out, int Ho, int Wo, void* stream);

/* ---- the face mask from the parser's logits, in front of cs_soft_erosion_frames ---- */
/* What both pipelines do between SegFormer and SoftErosion (can_swap_pipeline_e2e.py:183-190 per frame, can_swap_pipeline_v2i.py:76-83 per
 * source image) for B frames in one launch, without materialising the up-sampled logits:
 *   up = F.interpolate(logits, size=(scale*h, scale*w), mode="bilinear", align_corners=False); labels = up.argmax(dim=1);
 *   mask = torch.isin(labels, valid_list)
 * logits BxCxhxw fp32 (NCHW, contiguous), 1 <= C <= 32, scale 1, 2 or 4 on both axes; masks and labels B x scale*h x scale*w uint8, either may
 * be NULL but not both: labels = the class id, masks = bit `label` of valid_bits (0/1; the pipelines' valid_list [1, 2, 4, 5, 6, 7, 10, 11, 12]
 * is 0x1cf6).  Per pixel: src = (dst + 0.5) / scale - 0.5 clamped below at 0, i0 = floor(src), i1 = min(i0 + 1, n - 1), l1 = src - i0, l0 = 1 - l1,
 * v = hl0 * (wl0 * a + wl1 * b) + hl1 * (wl0 * c + wl1 * d) with every product and sum rounded to fp32 (the expression of the GPU kernel
 * the reference executes); the label is the FIRST maximum over the classes (strict >, classes in order), as torch.argmax.  Logits are assumed
 * finite: how a NaN orders is not part of the contract.  Asynchronous on the stream, allocates nothing, any B >= 1 (not bound to max_batch).
 * Returns nonzero and sets cs_last_error() for scale outside {1, 2, 4}, C outside [1, 32], B, h or w below 1, or both outputs NULL. */
int cs_face_masks(cs_engine* e, int B, int C, const float* logits, int h, int w, int scale, uint32_t valid_bits, uint8_t* masks, uint8_t* labels,
                  void* stream);

/* ---- the parser's input, in front of the caller's SegFormer network ---- */
/* What both pipelines do to a crop before the face parser sees it (can_swap_pipeline_e2e.py:171 and :180 per frame, can_swap_pipeline_v2i.py:73
 * per source image; SegformerImageProcessor of transformers 4.38: resize -> rescale -> normalize -> channels first) for B crops in one launch,
 * without an intermediate in memory.  crops BxHcxWcx3 u8.
 *   1. halve = 1: x = cv2.resize(crop, (Wc/2, Hc/2)) = (a + b + c + d + 2) >> 2 per 2x2 block and channel (INTER_LINEAR and INTER_AREA agree at
 *      exactly one half: :171, cropper.py:209); halve = 0: x = the crop.  x is h x w.
 *   2. PIL's image.resize((2w, 2h), BILINEAR) (Resample.c, PRECISION_BITS 22; at exactly x2 every coefficient is 0.75 / 0.25, 1.0 at both
 *      ends, exact in fixed point): the HORIZONTAL pass first, its result rounded to uint8, the vertical pass on that.  One axis pass n -> 2n:
 *        out[2j] = (3 in[j] + in[max(j - 1, 0)] + 2) >> 2,  out[2j + 1] = (3 in[j] + in[min(j + 1, n - 1)] + 2) >> 2.
 *   3. rescale + normalize (image_transforms.py: (u8 * rescale).astype(float32), then (r - mean) / std in float32) as a table look-up:
 *      lut: DEVICE, 3 x 256 fp32, lut[c][v] built on the host with exactly those numpy lines (canonswap_amd/tail.py parser_lut; the class defaults
 *      are mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225), rescale 1/255).  The device computes nothing in float.
 *   4. pixel_values Bx3xHoxWo fp32 (NCHW), resized_u8 BxHoxWox3 (step 2's image); (Ho, Wo) = halve ? (Hc, Wc) : (2 Hc, 2 Wc).  Either output may be
 *      NULL, not both.
 * Any Hc, Wc >= 1 (even with halve), any B >= 1 (not bound to max_batch); asynchronous on the stream, no engine scratch, allocates nothing.
 * Returns nonzero and sets cs_last_error() before any launch for a NULL e, crops or lut, both outputs NULL, B, Hc or Wc below 1, odd sizes with
 * halve, halve outside {0, 1}, or an output side above 16384. */
int cs_parser_input(cs_engine* e, int B, const uint8_t* crops, int Hc, int Wc, int halve, const float* lut, float* pixel_values,
                    uint8_t* resized_u8, void* stream);

/* ---- the side-by-side ("concat") video frame, behind both chains ---- */
/* concat_frames of src/utils/video.py:84-109, the video both pipelines write unconditionally (can_swap_pipeline_e2e.py:290: driving crop | rec_can
 * (:248-250) | I_can (:257-259) | I_p; can_swap_pipeline_v2i.py:328: driving crop | I_can | I_p), for B frames in one launch: P panels per frame,
 * each brought to S x S uint8, left to right in out BxSx(P S)x3 u8 (np.hstack).  panels, kinds, shared: HOST arrays of P entries; panels[p]: DEVICE
 * pointer to B images of the panel, or to ONE image shown in every frame where shared[p] != 0 (v2i's single I_can).  kinds[p]:
 *   0  u8 HWC SxS: copied (cv2.resize to the size the image has is the identity);
 *   1  u8 HWC (S/2)x(S/2): cv2.resize(img, (S, S)), default INTER_LINEAR, OpenCV's 8-bit arithmetic with 11-bit coefficients, at exactly x2
 *      (weights 512 and 1536 of 2048).  Horizontal pass into int32: H[2j] = 512 s[j-1] + 1536 s[j], H[2j+1] = 1536 s[j] + 512 s[j+1], at the
 *      borders H[0] = 2048 s[0], H[2w-1] = 2048 s[w-1].  Vertical pass: row 2i from rows (max(i-1, 0), i) with (b0, b1) = (512, 1536), row
 *      2i+1 from rows (i, min(i+1, h-1)) with (1536, 512): dst = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2;
 *   2  u8 HWC SxS: cv2.resize to one half first, (a + b + c + d + 2) >> 2 per 2x2 block (can_swap_pipeline_e2e.py:171: the pipeline's driving
 *      crop is the halved 512 crop, and the concat resizes that back up), then kind 1, without the half-size image in memory;
 *   3  fp32 CHW 3xSxS: parse_output (can_swap_e2e.py:314-322; cs_pack_u8's arithmetic): clip(x, 0, 1) * 255, clip(., 0, 255), truncated.
 * PARITY UNPINNED for kinds 1 and 2: the arithmetic is OpenCV's as published, not checked against vectors of cv2's own.
 * Any B >= 1 (not bound to max_batch); asynchronous on the stream, no engine scratch, allocates nothing: it may run beside a prefetch on
 * another stream.  Returns nonzero and sets cs_last_error() before any launch for a NULL e, out, array or panel pointer, B < 1, P outside
 * 1..4, a kind outside 0..3, or S below 4, above 16384 or no multiple of 4 (a thread owns four pixels). */
int cs_concat_frames(cs_engine* e, int B, int P, int S, const void* const* panels, const int* kinds, const int* shared, uint8_t* out,
                     void* stream);

/* ---- the face detector's input and decode: what stands around the caller's SCRFD network ---- */
/* The detector network (SCRFD, src/utils/dependencies/insightface/model_zoo/scrfd.py; the pipelines reach it through Face_detect_crop.get,
 * insightface_func/face_detect_crop_single.py:63-82 and _multi.py:63-100, at can_swap_pipeline_e2e.py:93-98 and can_swap_pipeline_v2i.py:113-118,
 * 136-145) stays the caller's; cs_det_input is everything in front of it, cs_det_decode everything behind it, so a frame never leaves the device.
 * cs_det_input = SCRFD.detect's letterbox (scrfd.py:224-235) and forward's blobFromImage (scrfd.py:154) for F frames in one launch, no
 * intermediate in memory.  frames FxHoxWox3 u8, blob Fx3xHdxWd fp32 (NCHW), (Wd, Hd) = the detector's input_size.
 *   1. the resized size exactly as :224-231, truncating int() included: im_ratio = Ho / Wo, model_ratio = Hd / Wd (doubles);
 *      im_ratio > model_ratio ? (nh = Hd, nw = int(nh / im_ratio)) : (nw = Wd, nh = int(nw * im_ratio)); det_scale = double(nh) / Ho is the
 *      caller's to keep (canonswap_amd/detect.py det_geometry) for cs_det_decode.
 *   2. cv2.resize(frame, (nw, nh)), default INTER_LINEAR, OpenCV's 8-bit arithmetic at a general ratio.  One axis src -> dst:
 *        scale = 1.0 / (double(dst) / src); f = float((d + 0.5) * scale - 0.5); s = floor(f); f -= s;
 *        coefficients short(round_half_even((1 - f) * 2048)) for tap s and short(round_half_even(f * 2048)) for tap s + 1, in fp32.
 *      Columns: s < 0 gives s = 0, f = 0; s >= src - 1 gives s = src - 1, f = 0.  Rows: the row numbers s and s + 1 are clamped to
 *      [0, src - 1] and the weights kept, as resize.cpp does it and as cs_concat_frames kind 1 states it at x2.  Horizontal pass into int32,
 *      vertical pass dst = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2.  At exactly one half on BOTH axes OpenCV takes the
 *      2 x 2 mean, (a + b + c + d + 2) >> 2; equal sizes copy.  At x2 and x1/2 the bits are those of cs_concat_frames kind 1 and of
 *      cs_parser_input step 1.
 *   3. rows and columns outside the resized image hold lut[c][0]: np.zeros goes through the blob arithmetic too.
 *   4. blobFromImage(det_img, 1 / std, size, (mean,) * 3, swapRB=True) = (float(u8) - mean) * scalefactor, channels first, as a table look-up:
 *      lut: DEVICE, 3 x 256 fp32, lut[c][v] for OUTPUT plane c, built on the host (canonswap_amd/detect.py det_lut; mean 127.5, std 128.0:
 *      scrfd.py:107-108).  The device computes nothing in float.  swap_rb != 0: output plane c holds source channel 2 - c.  swap_rb = 1 is what
 *      BOTH of the reference's calls do: forward passes swapRB=True whatever it is handed, BGR frames of cv2.imread at
 *      can_swap_pipeline_e2e.py:93 and RGB crops at can_swap_pipeline_v2i.py:230 alike - the quirk is mirrored, not mended; swap_rb = 0 is for
 *      callers who want the planes in the frame's own channel order.
 * PARITY UNPINNED for step 2: the arithmetic is OpenCV's as published, not checked against vectors of cv2's own.
 * Any F >= 1 (not bound to max_batch), any Ho, Wo >= 1, 1 <= Hd, Wd <= 16384; asynchronous on the stream, no engine scratch, allocates nothing;
 * a frame's bits do not depend on its batch.  Returns nonzero and sets cs_last_error() before any launch for a NULL e, frames, lut or blob, F,
 * Ho or Wo below 1, Hd or Wd outside [1, 16384], or a resized size that truncates to 0 (cv2.resize raises there). */
int cs_det_input(cs_engine* e, int F, const uint8_t* frames, int Ho, int Wo, int Hd, int Wd, int swap_rb, const float* lut, float* blob,
                 void* stream);
/* cs_det_decode = SCRFD.forward's decode (scrfd.py:160-218) and detect's sort, NMS and max_num pick (scrfd.py:239-273 with :275-303) for F
 * frames in one launch.  outs: HOST array of 3 * n_levels DEVICE pointers in the reference's output order - scores per level, then bbox per
 * level, then kps per level (net_outs[idx], [idx + fmc], [idx + 2 fmc]) - each F x A_l x {1, 4, 10} fp32 contiguous, A_l = (Hd / s_l) * (Wd / s_l) *
 * num_anchors; the kps pointers may ALL be NULL (a model without key points; kps must be NULL then).  strides: HOST, n_levels ints.  Supported
 * layouts (scrfd.py:114-131): 3 levels (8, 16, 32) with 2 anchors, 5 levels (8, 16, 32, 64, 128) with 1 anchor.  Outputs on the device: det F x
 * max_faces x 5 (x1, y1, x2, y2, score), kps F x max_faces x 5 x 2 or NULL, count F int32.  Per frame:
 *   1. candidates: the anchors with score >= det_thresh, levels in order, anchors in order (np.where, vstack);
 *   2. anchor centre ((cell % width) * stride, (cell / width) * stride) as fp32, cell = a / num_anchors, width = Wd / stride;
 *   3. pred * stride in fp32, centre - / + distance (distance2bbox, distance2kps), then division by float32(det_scale);
 *   4. descending score over the concatenation of the levels (:241) and again inside nms (:284);
 *   5. greedy NMS: areas (x2 - x1 + 1) * (y2 - y1 + 1), ovr = inter / (area_i + area_j - inter), a box survives on ovr <= nms_thresh;
 *   6. max_num > 0 and more than max_num survivors: the max_num largest by area - 2 * offset^2 (metric_max != 0: by area) come first, in that
 *      order; area here without the + 1, offset from the image centre (Wo / 2, Ho / 2), integer division.
 * All of it fp32 with every product, sum and quotient rounded on its own (numpy's arithmetic: the kernel is compiled with fp contraction off,
 * its division is correctly rounded): the result is bit-equal to the numpy lines.  Where the reference's argsort()[::-1] leaves the order of
 * equal keys open, the contract is a STABLE argsort reversed, at each of the three places: of two equal scores the candidate later in the
 * concatenated list comes first in :241's order; nms' own sort (:284) reverses that once more, so NMS visits - and the result lists - equal
 * scores in anchor order; of two equal max_num values the later survivor comes first.  Inputs are assumed finite.
 * One workgroup per frame; the candidates are compacted in anchor order by a prefix scan over wave ballots, not with atomics; sort and NMS
 * run in LDS: a frame's result depends neither on scheduling nor on its batch.  Caps, which are conditions and not errors of the call: a
 * frame with more than CS_DET_MAX_CAND candidates reports count = -1; a frame with more than max_faces NMS survivors and max_num == 0 reports
 * count = -2; nothing else of such a frame is defined.  A frame without a candidate reports 0.  Slots beyond count are not written.
 * Any F >= 1 (not bound to max_batch); asynchronous on the stream, no engine scratch, allocates nothing.  Returns nonzero and sets
 * cs_last_error() before any launch for a NULL e, outs, strides, det, count, score or bbox pointer, kps pointers partly NULL, kps given without
 * kps pointers, an unsupported layout, F < 1, Hd or Wd outside [1, 16384], Ho or Wo below 1, max_faces outside [1, CS_DET_MAX_FACES], max_num
 * below 0 or above max_faces, det_scale not a positive finite number, or a threshold that is NaN. */
#define CS_DET_MAX_CAND 1024
#define CS_DET_MAX_FACES 256
int cs_det_decode(cs_engine* e, int F, int n_levels, const int* strides, int num_anchors, const void* const* outs, int Hd, int Wd,
                  float det_scale, float det_thresh, float nms_thresh, int max_num, int metric_max, int Ho, int Wo, int max_faces, float* det,
                  float* kps, int* count, void* stream);

/* ---- measurement: per-kernel-family HIP-event timing on the launch stream */
int cs_profile_begin(cs_engine* e);
/* ms[0] = convolution kernels (conv_halo / conv_igemm), ms[1] = all other kernels except ms[2] = the feature warp
 * (grid_sample_kernel); counts likewise; flops = algorithmic conv FLOPs (2*MAC over the reference's logical channel
 * counts) enqueued since cs_profile_begin. CANONSWAP_PROFILE_CSV=<path> additionally dumps one line per launch. */
int cs_profile_end(cs_engine* e, double ms[3], long counts[3], double* flops);
/* MFMA FLOPs actually issued by the convolution launches since cs_profile_begin (padded channel counts, the taps the
 * phase-decomposed up-sampling convs really run): matrix-pipe utilisation, next to the algorithmic figure above */
int cs_profile_exec_flops(cs_engine* e, double* flops);

/* ---- operator level (unit parity tests) ---------------------------------------------------------------- */
typedef struct cs_conv_desc {
    const void* in;           /* fp16 channels-last */
    long in_sN, in_sD, in_sH, in_sW;
    int N, D, H, W, Cin, up_shift;
    int KD, KH, KW;
    const void* wgt;          /* packed fp16 (pack.py pack_conv) */
    int Cout_pad, Cout;
    const float* bias; const float* bias2;
    int act0; float slope0;
    const void* res; int res_f32; int res_shift; long res_sN, res_sD, res_sH, res_sW;
    const float* pixscale; int ps_stride;
    void* out0; int out0_f32; long out0_sN, out0_sD, out0_sH, out0_sW;
    const float* s2; const float* t2; int act1; float slope1;
    void* out1; long out1_sN, out1_sD, out1_sH, out1_sW;
    const float* stats;       /* SPADE: [N][C][2] = (mean, 1/sqrt(var+eps)) from cs_op_chan_stats */
    int mode;                 /* 0 std, 1 T blend, 2 SPADE, 3 pixel-shuffle + sigmoid, 5 std with out0 = act0(IN(res) * (1 + conv + bias)): SPADE's
                                 modulation without the beta half (res fp16, stats as for SPADE; /root/reference/src/modules/util.py:295-302) */
    int cfg;                  /* -2 conv_halo on the engine's tile cfg for this convolution, 10..20 conv_halo tile cfg, 30 the vol32 kernel (3x3x3 32 -> 32 on [N][H][W][16][32]), 31 conv_wide, 32 conv_lat
                               * (both: 3x3, 2-D, the engine's tensor combinations; conv_lat: Cin = 512, another summation order); -1, 0..3: test-only library */
    int tile_w, tile_h;       /* 0: the engine's choice */
    int ck;                   /* conv_halo channel chunk: 0: the engine's choice (its launch plan for this convolution and mode), 32 or 64 force it */
    int xcd_map;              /* conv_halo workgroup -> tile mapping: 0 engine default, k > 0 forces mapping k - 1 (common.h) */
    int ragged;               /* Cin % 32 == 16 and wgt went through cs_op_pair_ragged: paired taps in the last chunk (cfg 19 / 20 only) */
    int hilo;                 /* split-precision conv (util.py:528-544 convs of R): in = [hi | lo] per voxel, wgt = chunks W_hi | W_lo | W_hi, Cin = 96 */
    float* stat_out;          /* optional per-block partial (sum, sum of squares) of the stored fp32 out0 (cfg 30: [N][ceil(H/8) * W/2][32][2]) */
    /* cfg 30 with hilo: transform staging - the conv input is computed from fp32 volumes (strides of out0) while it is staged instead of read
     * from `in`: kind 1: xf_y; kind 2: lrelu((xf_y - mean) * rstd * gamma + beta [+ xf_res]) with (mean, rstd) = xf_stats[n][c][2], written back to
     * xf_out when given (util.py:531-540 fused into the consumer conv) */
    int xf_kind;
    const float* xf_y; const float* xf_res; float* xf_out;
    const float* xf_stats; const float* xf_gamma; const float* xf_beta;
    float xf_slope;
    int ep_general;           /* tests / A/B: 1 forces the general epilogue where a kernel also carries branch-free copies of it (same bits) */
    int pool_hw;              /* 1: out0 = AvgPool(1,2,2) of the activated conv output, computed in the epilogue; out0's strides address the pooled grid
                                 (DownBlock3d, /root/reference/src/modules/util.py:185-190) */
} cs_conv_desc;
int cs_op_conv(const cs_conv_desc* d, void* stream);
/* in place: re-pack the last 32-channel chunk of a packed conv weight [chunks * taps][Cout_pad][32] (Cin % 32 == 16) so that two
 * taps that are neighbours along the row share one 32-deep K-step (what the engine does for the hourglass tail, the mask conv and the
 * first encoder block at load time; dense_motion.py:88, util.py:185-190,261-263) */
int cs_op_pair_ragged(void* w, int Cout_pad, int nchunks, int KD, int KH, int KW, void* stream);
/* T's mask conv + sigmoid (adaptive_modulate.py:118-121,176: Conv2d(512, 1, 3, padding 1)) as a memory-bound VALU kernel: x fp16 [N][H][W][512],
 * w the layer's packed conv weight [16 chunks * 9 taps][16][32] (row 0 is the output channel), tmask[(n H W + h W + w) * 4] = sigmoid(conv + bias[0]) */
int cs_op_t_mask(const void* x, const void* wpacked, const float* bias, float* tmask, int N, int H, int W, void* stream);
/* T's per-identity precompute one kernel at a time (csrc/kernels.hip; blobs as pack._pack_T lays them out).
 * style: id 512 fp32, fc = nlayers x [W1 512x512][b1 512][W2 512x512][b2 512] fp32 (the ".fc" blobs back to back) -> style fp32 [nlayers][512]
 * = W2 lrelu(W1 id + b1, 0.2) + b2; the ".fc" blob carries W2 / b2 in memory channel order, so style does too.
 * modulate: wraw fp32 [512 o][9 taps][512 i] (the ".raw" blob, memory channel order), style 512 fp32 -> the 512 x 4608 values
 * wraw[o][t][i] style[i] / sqrt(sum_{t,i} (wraw[o][t][i] style[i])^2 + 1e-8) as fp16 into packed [144 = (i / 32) * 9 + t][1024][32 = i % 32] at
 * row ((o / 16) * 2 + 1) * 16 + o % 16; the rows ((o / 16) * 2) * 16 + o % 16 (the shared weight W) are not written. */
int cs_op_t_style(const float* id, const float* fc, float* style, int nlayers, void* stream);
int cs_op_t_modulate(const float* wraw, const float* style, void* packed, void* stream);
/* Copies to dst on `stream` what cs_set_identity left in the engine for layer 0 .. 13 (2 * block + conv - 1) and an identity slot that has been set:
 *   CS_T_WSET:   fp16 [144][1024][32], the slot's fused [W ; w_mod] set of the layer (rows as cs_op_t_modulate describes them)
 *   CS_T_STYLE:  fp32 [512], the style vector the LAST cs_set_identity call (whatever its slot) computed for the layer, memory channel order */
enum { CS_T_WSET = 0, CS_T_STYLE = 1 };
int cs_op_t_read(cs_engine* e, int layer, int slot, int which, void* dst, void* stream);
/* One AdaptiveSharedWeightConv2d layer of T (adaptive_modulate.py:128-193) on caller buffers, launched as cs_swap_ids launches it on this engine
 * (tile configuration by batch, the wide kernel, latency mode's conv_lat, per-sample weight sets): slots: B host ints; in16 fp16 [B][64][64][512]
 * (channel d * 32 + c); tmask_out fp32 [B][64][64][4], element 0 of each group receives sigmoid(mask_conv), the others are not written;
 * blend = mask * (conv(in, w_mod[slot]) + bias) + (1 - mask) * conv(in, W).
 * Even layers (conv1): out16 fp16 [B][64][64][512] = relu(blend); res32 and out32 must be NULL.
 * Odd layers (conv2): res32 fp32 [B][64][64][512] -> out32 fp32 = res32 + blend, out16 = fp16(out32), for layer 13 out16 = relu(out32 * s + t)
 * with the "T.pre0" affine (resblocks_3d.3dr0.norm1 folded). */
int cs_op_t_layer(cs_engine* e, int layer, int B, const int* slots, const void* in16, const float* res32, float* tmask_out, void* out16,
                  float* out32, void* stream);
/* one ResBlock3d of a feature volume (util.py:80-102, BatchNorms folded): contiguous [N][H][W][16][32] volumes a (fp16), x (fp32) ->
 * out0 (fp32) = conv2(relu(conv1(a) + b1)) + b2 + x, out1 (fp16) = act1(out0 * s2 + t2); w1 / w2 packed like every 3x3x3 32 -> 32 weight */
int cs_op_resblock3d(const void* a, const float* x, float* out0, void* out1, int N, int H, int W, const void* w1, const void* w2,
                     const float* b1, const float* b2, const float* s2, const float* t2, int act1, float slope1, void* stream);
int cs_op_grid_sample3d(const float* in_hwdc, const float* grid, float* out32, void* out16, int N, int D, int H, int W,
                        void* stream);
/* per-(n,c) mean and 1/sqrt(var+eps) of a [N][P][C] tensor; partials: scratch of cs_op_chan_stats_partial_floats floats */
long cs_op_chan_stats_partial_floats(int N, long P, int C);
int cs_op_chan_stats(const void* x, int is_f32, int N, long P, int C, float eps, float* partials, float* stats, void* stream);

/* The motion extractor's kernels one at a time (csrc/motion.hip; weights as pack._pack_M lays them out).  A split output is the fp16 pair
 * [hi | lo] per position (hi = fp16(v), lo = fp16(v - hi)), 2 C values.
 * stem: img fp32 [N][3][HI][256] -> x fp32 [N][HI/4][64][96], Conv2d(3, 96, 4, s 4) + LayerNorm (w: [48][96]) */
int cs_op_m_stem(const float* img, const float* w, const float* b, const float* g, const float* be, float* x, int N, int HI, int WI, void* stream);
/* depth-wise 7x7 + LayerNorm: x fp32 [N][H][W][C] -> y split [N][H][W][2C] (wt: [49][C], C = 96, 192, 384 or 768) */
int cs_op_m_dwln(const float* x, const float* wt, const float* b, const float* g, const float* be, void* y, int N, int H, int W, int C, void* stream);
/* LayerNorm + space-to-depth: x fp32 [N][H][W][C] -> y split [N][H/2][W/2][2 x 4C], inner channel (dy*2+dx)*C + c */
int cs_op_m_ln_s2d(const float* x, const float* g, const float* be, void* y, int N, int H, int W, int C, void* stream);
/* GRN: h fp32 [N][P][C] -> out split [N][P][2C]; scratch sumsq (N x 16 x C floats) and scale (N x C floats) */
int cs_op_m_grn(const float* h, const float* gamma, const float* beta, float* sumsq, float* scale, void* out, int N, int P, int C, void* stream);
/* average pool + LayerNorm + the 7 heads: x fp32 [N][P][768] -> out fp32 [N][328] (hw: [328][768]) */
int cs_op_m_head(const float* x, const float* g, const float* be, const float* hw, const float* hb, float* out, int N, int P, void* stream);
/* One of M's split-precision 1x1 convs, routed as run_M routes it on this engine (latency mode included).  C: the stage's channels (96, 192, 384,
 * 768); wpacked / bias: the layer's pack._pack_M blobs.  form 0 (pwconv1): in split [N][H][H][2C] -> out fp32 [N][H][H][4C] = GELU(conv);
 * form 1 (pwconv2): in split [N][H][H][8C], out fp32 [N][H][H][C] holds the residual and receives out + conv; form 2 (downsample, C < 768):
 * in split [N][H][H][8C] from cs_op_m_ln_s2d (H: the output grid) -> out fp32 [N][H][H][2C]. */
int cs_op_m_pointwise(cs_engine* e, int form, const void* in, const void* wpacked, const float* bias, float* out, int N, int H, int C, void* stream);

/* The dense-motion kernels of W one at a time (csrc/kernels.hip; weights as pack._pack_W lays them out).  Volumes are [N][D][H][W] voxels.
 * compress: f fp32 HWDC [N][H][W][D][32] -> comp fp16 [N][D][H][W][4] = ReLU(conv1x1 + BN folded) (w: [4][32], b: [4]) */
int cs_op_dm_compress(const float* f_hwdc, const float* w, const float* b, void* comp, int N, int D, int H, int W, void* stream);
/* sparse motions + heat maps: comp fp16 [N][D][H][W][4] (shared_comp: one volume [1][D][H][W][4] for all N), kp_d [N][21][3], kp_s [N][21][3]
 * (shared_kps: [1][21][3]) -> 112 fp16 channels per voxel at voxel stride ostride (a multiple of 8, 16-byte aligned): channel 5 k = heat map of
 * slot k (0 for k = 0), 5 k + 1 .. 5 k + 4 = comp sampled at slot k's sparse motion, 110 / 111 = zero.  D, H >= 2, 2 <= W <= 64. */
int cs_op_dm_sparse(const void* comp, int shared_comp, const float* kp_d, const float* kp_s, int shared_kps, void* out, int ostride,
                    int N, int D, int H, int W, void* stream);
/* mask softmax + deformation + feature warp: part = the mask conv's compact-2 partials fp32 [N][D][H][W/4][10][22] (tile T, j <-> output column
 * 4 T - 3 + j, see cs_op_dm_read), bias [22]; in fp32 HWDC [N][H][W][D][32] (shared_in: one volume) -> out32 fp32 / out16 fp16 HWDC (either may
 * be null), deform fp32 [N][D][H][W][3] (may be null).  D = 16, W a multiple of 16. */
int cs_op_dm_softmax_warp(const float* part, const float* bias, const float* kp_d, const float* kp_s, int shared_kps, const float* in_hwdc,
                          int shared_in, float* out32, void* out16, float* deform, int N, int D, int H, int W, void* stream);
/* occlusion finish: occ fp32 [N][H][W] = sigmoid(bias + the shifted partial sums, zero padding).  taps 49: part [N][H][W][64] with channel
 * ky * 7 + kx (the batched path's 1x1 conv); taps 7: part [N][H][W][16] with channel kx (latency mode's (7,1)-tap conv). */
int cs_op_occ_finish(const float* part, int taps, float bias, float* occ, int N, int H, int W, void* stream);
/* Copies one of the engine's dense-motion buffers, as the last call (cs_warp, cs_warp_forward, cs_animate_frames) left it, to dst on `stream`;
 * B: samples to copy (<= max_batch).
 *   CS_DM_COMP:    fp16 [B][16][64][64][4] (after a shared-volume call only sample 0 is valid)
 *   CS_DM_L0 + i:  fp16 [B][16][S][S][lw], S = 64 >> i, lw = 144, 128, 256, 512, 1024, 1024 (i = 0 .. 5): channels [0, skip_off) the up-block
 *                  output, [skip_off, skip_off + cin) the down-block input, skip_off = 32, 64, 128, 256, 512, 0, cin = 112, 64, 128, 256, 512,
 *                  1024; in level 0 channels [32, 144) are the output of dm_sparse
 *   CS_DM_PRED:    fp16 [B][16][64][64][144] (the hourglass output; channels 142, 143 zero)
 *   CS_DM_LOGITS:  fp32 [B][16][64][16][10][22]: the mask conv's compact-2 partials (cs_op_dm_softmax_warp) */
enum { CS_DM_COMP = 0, CS_DM_L0 = 1, CS_DM_PRED = 7, CS_DM_LOGITS = 8 };
int cs_op_dm_read(cs_engine* e, int which, int B, void* dst, void* stream);

/* The SPADE decoder's workspace, for tests that check G launch by launch on the engine's own tensors.
 * cs_op_g_read copies one buffer, as the last cs_spade_decode left it, to dst on `stream`; B: samples to copy (<= max_batch).  All fp16, channels last:
 *   CS_G_X0, CS_G_X1:  [B][64][64][512]    x of the middle blocks: fc writes X0, block b reads X(b & 1) and writes X(~b & 1); up_0 reads X0
 *   CS_G_A64:          [B][64][64][1536]   relu(mlp_shared) of G_middle_b.norm_k in channels [(2 b + k) 128, +128)
 *   CS_G_A128 / A256:  [B][S][S][384]      relu(mlp_shared) of up_0 / up_1 (S = 128 / 256): norm_0 in [0, 128), norm_1 in [128, 256), norm_s in [256, 384)
 *   CS_G_H64:          [B][64][64][512]    lrelu(SPADE) of a middle block's norm_0, then of its norm_1
 *   CS_G_DX64:         [B][64][64][512]    conv_0 of a middle block
 *   CS_G_H128:         [B][128][128][512]  up_0: IN(x)(1 + gamma_s) (the shortcut's .ng launch), then lrelu(SPADE norm_0)
 *   CS_G_XS128:        [B][128][128][256]  up_0's learned shortcut x_s
 *   CS_G_DX128, CS_G_H1_128, CS_G_O128: [B][128][128][256]  up_0's conv_0, lrelu(SPADE norm_1), block output x_s + conv_1
 *   CS_G_BS:           B x 4194304 values: conv_s(beta) of the shortcut, [B][128][128][256] after up_0's .bs launch, [B][256][256][64] after up_1's
 *   CS_G_H256:         [B][256][256][256]  up_1: lrelu(SPADE norm_0) (and IN(x)(1 + gamma_s) before it where the shortcut runs as three launches)
 *   CS_G_XS256, CS_G_DX256, CS_G_H1_256: [B][256][256][64]  up_1's x_s, conv_0, lrelu(SPADE norm_1)
 *   CS_G_O256:         [B][256][256][64]   lrelu(x_s + conv_1, 0.2): conv_img's input
 *   CS_G_STATS:        fp32 B x 1024 values: the (mean, rstd) slot handed out last, [B][C][2] in its first B C 2 values (C: the channels of the
 *                      tensor whose statistics-emitting conv ran last)
 * cs_op_g_fill writes the fp16 NaN pattern CS_G_SENTINEL over the first B samples of every buffer above and over the whole statistics pool (an
 * fp32 there reads 0x7E5A7E5A).
 * cs_op_g_stop(e, n): the next cs_spade_decode returns (with 0) after its n-th launch, counted as the profile CSV lists them (nchw_to_nhwc16
 * is the first; chan_stats_finish and splitk_finish count); n = 0: all of it.  That call clears the stop. */
enum { CS_G_X0 = 0, CS_G_X1, CS_G_A64, CS_G_A128, CS_G_A256, CS_G_H64, CS_G_DX64, CS_G_H128, CS_G_XS128, CS_G_DX128, CS_G_H1_128, CS_G_O128, CS_G_BS,
       CS_G_H256, CS_G_XS256, CS_G_DX256, CS_G_H1_256, CS_G_O256, CS_G_STATS };
#define CS_G_SENTINEL 0x7E5A
int cs_op_g_read(cs_engine* e, int which, int B, void* dst, void* stream);
int cs_op_g_fill(cs_engine* e, int B, void* stream);
int cs_op_g_stop(cs_engine* e, int n);

/* The volume workspace of F (cs_extract_feature_3d) and R (cs_refine), for tests that check both launch by launch on the engine's own tensors.
 * cs_op_v_read copies one buffer, as the last call left it, to dst on `stream`; B: samples to copy (<= max_batch).  Volumes are HWDC,
 * [B][64][64][16][32] (the 512-channel 2-D view: channel d * 32 + c):
 *   CS_V_T0:             fp16 [B][256][256][64]   F: conv_first
 *   CS_V_P0:             fp16 [B][128][128][128]  F: down_blocks.0 (pooled)
 *   CS_V_P1:             fp16 [B][64][64][256]    F: down_blocks.1 (pooled)
 *   CS_V_S0 .. CS_V_S2:  fp32 volumes: the residual stream and the conv outputs that rotate through them
 *   CS_V_A0, CS_V_A1:    fp16 volumes: the pre-activated copies the fp16 convs read
 *   CS_V_SP0, CS_V_SP1:  B x 4194304 fp16 values, the split-precision [hi | lo] inputs of R's stage-3 convs; in the default (transform-staging)
 *                        path R uses each as one more fp32 volume [B][64][64][16][32] at the sample stride of an fp32 volume
 *   CS_V_STATS:          fp32 B x 1024 values: the (mean, rstd) slot handed out last, [B][32][2] in its first B 64 values (as CS_G_STATS)
 * cs_op_v_fill writes the 16-bit pattern CS_G_SENTINEL over the first B samples of every buffer above and over the whole statistics pool.
 * cs_op_v_stop(e, n): the next cs_extract_feature_3d or cs_refine returns (with 0) after its n-th launch, counted as the profile CSV lists them
 * (the layout launches ncdhw_to_hwdc / hwdc_to_ncdhw and chan_stats_finish count); stopped before its last launch the call leaves f_out
 * untouched; n = 0: all of it.  That call clears the stop.  (One counter serves cs_op_g_stop and cs_op_v_stop: the next of the three entry
 * points uses it up.) */
enum { CS_V_T0 = 0, CS_V_P0, CS_V_P1, CS_V_S0, CS_V_S1, CS_V_S2, CS_V_A0, CS_V_A1, CS_V_SP0, CS_V_SP1, CS_V_STATS };
int cs_op_v_read(cs_engine* e, int which, int B, void* dst, void* stream);
int cs_op_v_fill(cs_engine* e, int B, void* stream);
int cs_op_v_stop(cs_engine* e, int n);
/* Three kernels of these stages alone (csrc/kernels.hip), on the caller's buffers.
 * conv_first: img fp32 [N][3][H][W] -> out16 fp16 [N][H][W][64] = relu(conv3x3(img; w [64][27] fp32, input channel major) + b [64]), zero padding
 * (first.conv with first.norm folded, appearance_feature_extractor.py:22,39)
 * norm_act: GroupNorm(32, 32) apply + residual + LeakyReLU on N samples of per_n fp32 values, channel = index % 32 (util.py:531-540):
 *   v = lrelu((y - mean) rstd gamma + beta [+ res], slope), (mean, rstd) = stats [N][32][2]; out32 = v; out16 = fp16(act2(v s2[i % period2] +
 *   t2[i % period2])) (s2 NULL: fp16(v)); split != 0: out16 receives the pair [hi(32) | lo(32)] per voxel, hi = fp16(v), lo = fp16(v - hi).
 *   res, out32, out16, s2 / t2 may be NULL.  Refused: per_n no multiple of 32 or (with s2) of period2, split with s2.
 * split16: x fp32, n values (a multiple of 32) -> out16 fp16, 2 n values: [hi(32) | lo(32)] per voxel of 32 channels */
int cs_op_conv_first(const float* img, const float* w, const float* b, void* out16, int N, int H, int W, void* stream);
int cs_op_norm_act(const float* y, const float* stats, const float* gamma, const float* beta, const float* res, float slope, float* out32,
                   void* out16, const float* s2, const float* t2, int period2, int act2, float slope2, int N, long per_n, int split, void* stream);
int cs_op_split16(const float* x, void* out16, long n, void* stream);

/* The identity network's kernels one at a time (csrc/identity.hip; weights as pack._pack_A lays them out; models/arcface_models.py:10-136).
 * conv: in fp16 (in_f32: fp32, rounded to fp16 on load) contiguous [N][IH][IW][Cin] -> out fp32 / fp16 [N][OH][OW][Cout] = prelu(conv + bias), K x K
 * taps (K from 1 to 8), stride >= 1, zero padding pad < K, OH = (IH + 2 pad - K) / stride + 1; w fp16 [K * K][Cout][Cin] (pack.pack_id_conv); Cin % 32 == 0,
 * Cout % 64 == 0; slope: device pointer to the PReLU's one slope, NULL = no activation; bias may be NULL */
int cs_op_id_conv(const void* in, int in_f32, int N, int IH, int IW, int Cin, int K, int stride, int pad, const void* w, const float* bias,
                  int Cout, const float* slope, void* out, int out_f32, void* stream);
/* MaxPool2d(2, 2) (arcface_models.py:116): in fp32 [B][IH][IW][C] -> x fp32 [B][IH/2][IW/2][C], a16 fp16 = x s + t (the first block's bn0); C % 4 == 0 */
int cs_op_id_maxpool(const float* in, const float* s, const float* t, float* x, void* a16, int B, int IH, int IW, int C, void* stream);
/* SE gate + block tail (arcface_models.py:21-25,54-63): out fp32, position (h, w) of sample n at n sN + h sH + w sW (a stride-1 map read at its even
 * positions: doubled sH / sW), channels contiguous; se [B][C] = sigmoid(W2 prelu(W1 mean_hw(out) + b1, slopes[1]) + b2) (w1 [C/16][C], w2 [C][C/16]);
 * x fp32 [B][H][W][C] = prelu(out se + res, slopes[0]), res fp32 [B][H][W][C]; a16 fp16 = x s + t.  C = 64, 128, 256 or 512; strides multiples of 4. */
int cs_op_id_se_tail(const float* out, long sN, long sH, long sW, int B, int H, int W, int C, const float* w1, const float* b1,
                     const float* w2, const float* b2, const float* slopes, const float* res, const float* s, const float* t, float* se,
                     float* x, void* a16, void* stream);
/* bn2 -> flatten -> fc -> bn3 [-> F.normalize] (arcface_models.py:129-134; can_swap_e2e.py:106): a16 fp16 [B][49][512] = bn2(x) in (h, w, c) order,
 * w fp16 [49][512][512] and bias [512] (the "A.fc" blobs), part: scratch of 49 x B x 512 floats -> raw [B][512], idn [B][512] (either may be NULL) */
int cs_op_id_embed(const void* a16, const void* w, const float* bias, float* part, float* raw, float* idn, int B, void* stream);
/* Copies to dst on `stream`, as fp32 NCHW at its valid extent, an activation the LAST pass of cs_identity / cs_identity_u8 left (B <= the images of
 * that pass, at most min(max_batch, 8); arcface_models.py:116-129): CS_ID_STEM Bx64x55x55 (after the max-pool), CS_ID_LAYER1 + i: Bx64x55x55, Bx128x28x28, Bx256x14x14,
 * Bx512x7x7 (i = 0 .. 3), CS_ID_PREFC Bx512x7x7 (bn2's output as the fc reads it, fp16 values) */
enum { CS_ID_STEM = 0, CS_ID_LAYER1 = 1, CS_ID_PREFC = 5 };
int cs_op_identity_read(cs_engine* e, int which, int B, float* dst, void* stream);

/* ---- operator level: the face parser's kernels alone (csrc/parser.hip; all tensors contiguous, channels-last, on the device).
 * input: pixel_values fp32 [B][3][H][W] -> fp16 [B][H][W][32] (3 real + 29 zero channels) */
int cs_op_parser_input(const float* pixel_values, void* out16, int B, int H, int W, void* stream);
/* token GEMM: a16 fp16 [M][K] x w16 fp16 [N][K]^T + bias (may be NULL), fp32 accumulation; K % 32 == 0, N % 64 == 0, any M >= 1.  mode 0: out fp16
 * [M][N]; 1: out fp32 [M][N] += result (the residual stream, in place); 2: out fp32 [M][N]; 3: out fp32 [M / P][L][P], the first L columns only */
int cs_op_parser_gemm(const void* a16, const void* w16, const float* bias, int M, int K, int N, int mode, void* out, int P, int L, void* stream);
/* LayerNorm over C channels (a multiple of 64 up to 512) of M tokens: in fp32 [M][C] -> out32 fp32 and / or out16 fp16 (either may be NULL) */
int cs_op_parser_layernorm(const float* in, const float* g, const float* b, float eps, long M, int C, float* out32, void* out16, void* stream);
/* attention: q16 fp16 [B][Nq][heads d] (scale folded in), kv16 fp16 [B][Nk][2 heads d] (keys | values) -> ctx16 fp16 [B][Nq][heads d] =
 * softmax(q k^T) v per head (contiguous channel slices); d = 32 or 64, Nk <= 256 (more is refused) */
int cs_op_parser_attention(const void* q16, const void* kv16, void* ctx16, int B, int Nq, int Nk, int heads, int d, void* stream);
/* GELU(depth-wise 3 x 3 conv + bias), zero padding 1: in16 fp16 [B][H][W][C] -> out16; w fp32 [9][C] tap-major, bias fp32 [C]; C % 8 == 0 */
int cs_op_parser_dwgelu(const void* in16, const float* w, const float* bias, void* out16, int B, int H, int W, int C, void* stream);
/* decode head: out16 fp16 [B][H][W][D] = relu(p0 + up2(p1) + up4(p2) + up8(p3)), bilinear with align_corners = False; p_s fp32 [B][H >> s][W >> s][D];
 * H, W multiples of 8, D % 4 == 0 */
int cs_op_parser_upadd(const float* p0, const float* p1, const float* p2, const float* p3, void* out16, int B, int H, int W, int D, void* stream);
/* Copies to dst on `stream`, as fp32 NCHW, an activation the LAST pass of cs_parser left (B <= the images of that pass): CS_PARSER_STAGE0 + s: the
 * output of encoder stage s after its final LayerNorm, BxC_sx(H >> (s + 2))x(W >> (s + 2)); CS_PARSER_PRE: the decode head's map in front of the
 * classifier, BxDx(H/4)x(W/4) (fp16 values) */
enum { CS_PARSER_STAGE0 = 0, CS_PARSER_PRE = 4 };
int cs_op_parser_read(cs_engine* e, int which, int B, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
