"""Image-space steps on either side of the generator, on the device.

Counterparts of the reference's host-side helpers, same names and argument meaning, operating on device tensors so the
per-frame loop (src/can_swap_pipeline_e2e.py:223-283) no longer leaves the GPU between the generator and the final frame:

* ``face_masks``             src/can_swap_pipeline_e2e.py:183-190, src/can_swap_pipeline_v2i.py:76-83: the parser's logits -> 0/1 masks
                             (F.interpolate to 512 x 512, argmax, isin) of B frames in one launch, nothing up-sampled in memory
* ``parser_input``           src/can_swap_pipeline_e2e.py:171 + :180, src/can_swap_pipeline_v2i.py:73: crops -> the face parser's pixel_values
                             (cv2.resize to one half, SegformerImageProcessor's PIL resize x 2, rescale, normalize, CHW) of B crops in one launch
* ``concat_frames``          src/utils/video.py:84-109 (called at src/can_swap_pipeline_e2e.py:290, src/can_swap_pipeline_v2i.py:328): the side-by-side
                             video frame, up to four panels resized / packed to S x S uint8 and stacked left to right, B frames in one launch
* ``yuv_to_rgb``, ``rgb_to_yuv``   no counterpart: the reference lets swscale convert on the host (imageio-ffmpeg's rgb24, images2video).  NV12 / I420
                             frames as the codec has them -> the chain's RGB frames and back, the blocks nothing wrote byte for byte (csrc/yuv.hip)
* ``SoftErosion``            src/utils/crop.py:21-47           (the reference runs it with .cuda() too: pure torch)
* ``prepare_paste_back``     src/utils/crop.py:515-521          (cv2.warpAffine of the float mask)
* ``paste_back``             src/utils/crop.py:523-529          (cv2.warpAffine of the crop + blend)
* ``paste_back_fused``       both of the above in one kernel launch per frame
* ``paste_back_shared``      paste_back of B frames into one image under one mask (can_swap_pipeline_v2i.py:317-321)
* ``crop_frames``            src/utils/crop.py:429-455 per frame (cropper.py:196-209): landmark geometry on the host (crop.py of this
                             package), cv2.warpAffine of B frames in one launch; ``crop_frames_M``: the same with the caller's matrices
* ``crop_faces``, ``paste_back_faces``   several faces per frame: face b is cut from, and pasted into, frame frame_index[b]; the paste is
                             paste_back once per face of a frame, in order, in one pass over the frame (``crop_faces_M``: the caller's matrices)
* ``crop_lmk``, ``paste_back_faces_dev``   the same two from landmarks and matrices that never leave the device (cs_crop_lmk,
                             cs_paste_back_faces_dev): the geometry of csrc/lmk_geometry.h in front of the crop, the matrices inverted
                             by the paste kernel itself - nothing is downloaded between the tracker and the paste-back
* ``prepare_crops``          src/utils/cropper.py:209 + src/can_swap_e2e.py:126-163 (INTER_AREA 512 -> 256, /255, HWC -> CHW)
* ``FrameStreamer``          streamed upload of the uint8 crops instead of the whole-video residency of prepare_videos

Every operation is a HIP kernel of libcanonswap_hip.so (csrc/imgops.hip; crop_lmk: csrc/landmarks.hip); there is no torch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import crop as crop_geometry
from .engine import Engine, u8_images


def _m6(M, B=None):
    """One host matrix, 2x3 or 3x3 (its top rows) -> (six doubles, their pointer); with B: B matrices -> (B, 6)."""
    a = np.asarray(M, dtype=np.float64)
    m = np.ascontiguousarray(a.reshape(-1)[:6] if B is None else a.reshape(B, -1)[:, :6])
    return m, m.ctypes.data_as(C.POINTER(C.c_double))


def _m6_of(M, B, name, who):
    """B host matrices, (B,2,3) or (B,3,3), B >= 1 -> _m6's pair; ValueError names the argument."""
    if B < 1 or tuple(np.shape(M)) not in ((B, 2, 3), (B, 3, 3)):
        raise ValueError(f"{who}: {name} must be (B,2,3) or (B,3,3) host matrices, B = {B if B >= 0 else '?'} >= 1, got shape {tuple(np.shape(M))}")
    return _m6(M, B)


def _masks_of(masks_crop, crops, who):
    """The soft masks of B crops (B,Hc,Wc,3), host or device -> the (B,Hc,Wc) tensor where it lies (the caller converts and uploads)."""
    mc = torch.as_tensor(masks_crop)
    if tuple(mc.shape) != tuple(crops.shape[:3]):
        raise ValueError(f"{who}: masks_crop must be (B, Hc, Wc), one mask per crop, got {tuple(mc.shape)} for crops {tuple(crops.shape)}")
    return mc


def _mask_hw(e: Engine, mask):
    """A float mask, HxW or HxWx3 (the reference stacks three identical channels), host or device -> contiguous fp32 HxW on the device."""
    m = torch.as_tensor(mask)
    if m.dim() == 3:
        m = m[..., 0]
    return m.to(e.device).float().contiguous()


FACE_VALID = (1, 2, 4, 5, 6, 7, 10, 11, 12)      # valid_list of can_swap_pipeline_e2e.py:189 / can_swap_pipeline_v2i.py:82: the face's classes


def valid_bits(valid) -> int:
    """Class ids -> the 32-bit set cs_face_masks takes (bit c: class c is part of the mask)."""
    ids = [int(c) for c in valid]
    if any(c != v for c, v in zip(ids, valid)) or any(not 0 <= c < 32 for c in ids):
        raise ValueError(f"valid: class ids must be integers in [0, 32), got {tuple(valid)}")
    bits = 0
    for c in ids:
        bits |= 1 << c
    return bits


def face_masks(e: Engine, logits, valid=FACE_VALID, size=(512, 512), out=None, want_labels=False, out_labels=None):
    """The lines between the parser and SoftErosion (can_swap_pipeline_e2e.py:183-190, can_swap_pipeline_v2i.py:76-83) of B frames in one launch:
    logits (B,C,h,w), or (C,h,w) for one frame, the parser's output (anything but contiguous fp32 is converted with .float().contiguous()) ->
    (B,H,W) uint8 0/1 on the device = isin(argmax(F.interpolate(logits, size, mode="bilinear", align_corners=False), 1), valid); with want_labels
    (or out_labels) {"masks", "labels"}, labels (B,H,W) uint8 class ids.  size = s * (h, w), s 1, 2 or 4; C <= 32; valid: class ids in [0, 32)."""
    t = torch.as_tensor(logits)
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError("face_masks expects (B, C, h, w) logits")
    B, Cn, h, w = t.shape
    if Cn > 32:
        raise ValueError(f"face_masks: {Cn} classes (at most 32: the valid set is a 32-bit word)")
    H, W = int(size[0]), int(size[1])
    s = H // h
    if s not in (1, 2, 4) or (H, W) != (s * h, s * w):
        raise ValueError(f"face_masks: size {(H, W)} is not s * {(h, w)} with s in (1, 2, 4)")
    bits = valid_bits(valid)
    t = t.to(e.device).float().contiguous()
    want_labels = want_labels or out_labels is not None
    masks = e._out(out, (B, H, W), torch.uint8)
    labels = e._out(out_labels, (B, H, W), torch.uint8) if want_labels else None
    e._call("cs_face_masks", B, Cn, t, h, w, s, bits, masks, labels)
    return {"masks": masks, "labels": labels} if want_labels else masks


# SegformerImageProcessor's class defaults (transformers 4.38: IMAGENET_DEFAULT_MEAN / _STD, rescale_factor 1 / 255, size 512 x 512); a checkpoint's
# preprocessor_config.json may name others, hence parameters
PARSER_MEAN = (0.485, 0.456, 0.406)
PARSER_STD = (0.229, 0.224, 0.225)
PARSER_RESCALE = 1 / 255


def parser_lut(mean=PARSER_MEAN, std=PARSER_STD, rescale=PARSER_RESCALE) -> np.ndarray:
    """(3, 256) fp32: what the processor's rescale and normalize make of byte v in channel c, by its own numpy lines (transformers 4.38
    image_transforms.py): rescale = (image * scale).astype(np.float32), the product of a uint8 array and a Python float taken in float64;
    normalize = (image - mean) / std with mean and std cast to the image's float32.  cs_parser_input looks this up and computes nothing in float
    (a folded v * scale + bias differs from it in most entries)."""
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError("parser_lut: mean and std are three numbers each, std nonzero")
    image = np.arange(256, dtype=np.uint8)
    r = (image * float(rescale)).astype(np.float32)
    m, s = np.array(mean, dtype=r.dtype), np.array(std, dtype=r.dtype)
    lut = (r[None, :] - m[:, None]) / s[:, None]
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    return np.ascontiguousarray(lut)


def _parser_lut_on(e: Engine, mean, std, rescale):
    """The table on the engine's device, uploaded once per engine and set of constants."""
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std), float(rescale))
    return e.device_table(("parser_lut",) + key, lambda: parser_lut(*key))


ID_MEAN, ID_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # ID_transform's Normalize (can_swap_pipeline_e2e.py:43-46, can_swap_pipeline_v2i.py:44-47)


def id_lut(mean=ID_MEAN, std=ID_STD) -> np.ndarray:
    """(3, 256) fp32: what ID_transform makes of byte v in channel c, by torchvision's own arithmetic: ToTensor = byte.float().div(255),
    Normalize = (x - mean) / std with mean and std as float32 tensors (the kind of table parser_lut builds by the image processor's numpy
    lines).  cs_identity_u8 looks this up."""
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError("id_lut: mean and std are three numbers each, std nonzero")
    x = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return np.ascontiguousarray(((x[None, :] - m[:, None]) / s[:, None]).numpy())


def id_lut_on(e: Engine, mean=ID_MEAN, std=ID_STD):
    """The table on the engine's device, uploaded once per engine and set of constants."""
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std))
    return e.device_table(("id_lut",) + key, lambda: id_lut(*key))


def parser_input(e: Engine, crops_u8, halve=None, mean=PARSER_MEAN, std=PARSER_STD, rescale=PARSER_RESCALE, out=None, want_u8=False, out_u8=None):
    """What both pipelines feed the face parser (can_swap_pipeline_e2e.py:171 + :180, can_swap_pipeline_v2i.py:73) for B crops in one launch:
    crops_u8 (B,H,W,3), or (H,W,3) for one crop, uint8, host or device -> pixel_values (B,3,Ho,Wo) fp32 on the device =
    SegformerImageProcessor(size 2h x 2w)(x), x = cv2.resize(crop, (W/2, H/2)) with halve, the crop itself without; (Ho, Wo) = (H, W) with
    halve, (2H, 2W) without.  halve=None: halve iff the crop is 512 x 512 (the pipelines' 256 x 256 parser crop, 512 x 512 pixel_values, from
    either crop size).  Bit-equal to PIL's two-pass fixed-point bilinear resize and the processor's numpy lines (parser_lut).  With want_u8 (or
    out_u8) {"pixel_values", "resized_u8"}, resized_u8 (B,Ho,Wo,3) uint8: the resized image before rescale / normalize."""
    t = torch.as_tensor(crops_u8)
    t = u8_images(t[None] if t.dim() == 3 else t, True, 1, "crops_u8", "parser_input")
    B, H, W, _ = t.shape
    if halve is None:
        halve = (H, W) == (512, 512)
    halve = bool(halve)
    if halve and (H % 2 or W % 2):
        raise ValueError(f"parser_input: {H}x{W} crops cannot be halved (odd size)")
    Ho, Wo = (H, W) if halve else (2 * H, 2 * W)
    if max(Ho, Wo) > 16384:
        raise ValueError(f"parser_input: output {Ho}x{Wo} above 16384 a side")
    t = t.to(e.device).contiguous()
    want_u8 = want_u8 or out_u8 is not None
    pv = e._out(out, (B, 3, Ho, Wo), torch.float32)
    u8 = e._out(out_u8, (B, Ho, Wo, 3), torch.uint8) if want_u8 else None
    lut = _parser_lut_on(e, mean, std, rescale)
    e._call("cs_parser_input", B, t, H, W, int(halve), lut, pv, u8)
    return {"pixel_values": pv, "resized_u8": u8} if want_u8 else pv


CONCAT_KINDS = (0, 1, 2, 3)      # cs_concat_frames: u8 S x S as it is; u8 S/2 x S/2, cv2.resize x 2; u8 S x S halved, then x 2; fp32 3 x S x S, parse_output


def concat_frames(e: Engine, panels, kinds=None, shared=None, out=None):
    """concat_frames of src/utils/video.py:84-109 (can_swap_pipeline_e2e.py:290: driving | rec_can | I_can | I_p; can_swap_pipeline_v2i.py:328:
    driving | I_can | I_p) for B frames in one launch: panels, 1 to 4 images per frame, left to right -> (B, S, P * S, 3) uint8 on the device.
    A panel is (n,H,W,3) / (H,W,3) uint8 or (n,3,H,W) / (3,H,W) fp32, host or device, square; its kind (CONCAT_KINDS; cs_concat_frames in
    include/canonswap_hip.h) is by default 3 for fp32 (parse_output), and for uint8 0 where its side is S (a copy) and 1 where it is S / 2
    (cv2.resize(img, (S, S)), INTER_LINEAR, OpenCV's 8-bit arithmetic), S being the largest side among the panels; kind 2 (S x S uint8: cv2.resize to
    one half first, can_swap_pipeline_e2e.py:171, then kind 1) is the caller's to name in kinds=.  B is the largest n; a panel with n = 1 beside
    others with more is shared by all frames (shared=: one flag per panel, to say so explicitly).  No engine scratch, no allocation but the
    result: it may run on the caller's stream while a prefetch is in flight."""
    ts = [torch.as_tensor(p) for p in panels]
    P = len(ts)
    if not 1 <= P <= 4:
        raise ValueError(f"concat_frames: {P} panels (1 to 4)")
    if kinds is not None and (len(kinds) != P or any(k not in CONCAT_KINDS for k in kinds)):
        raise ValueError(f"concat_frames: kinds {tuple(kinds)}: one of {CONCAT_KINDS} per panel")
    if shared is not None and len(shared) != P:
        raise ValueError("concat_frames: shared holds one flag per panel")
    sides = []
    for i, t in enumerate(ts):
        if t.dtype not in (torch.uint8, torch.float32) or t.dim() not in (3, 4):
            raise ValueError(f"concat_frames: panel {i} is neither uint8 (n,H,W,3) nor fp32 (n,3,H,W)")
        if t.dim() == 3:
            t = ts[i] = t[None]
        side, ch = (t.shape[1:3], t.shape[3]) if t.dtype == torch.uint8 else (t.shape[2:4], t.shape[1])
        if ch != 3 or side[0] != side[1] or side[0] < 1 or t.shape[0] < 1:
            raise ValueError(f"concat_frames: panel {i} has shape {tuple(t.shape)}, not B square three-channel images")
        if kinds is not None and (kinds[i] == 3) != (t.dtype == torch.float32):
            raise ValueError(f"concat_frames: panel {i} is {t.dtype}, its kind {kinds[i]}")
        sides.append(int(side[0]))
    if kinds is None:
        S = max(sides)
        kinds = [3 if t.dtype == torch.float32 else 0 if n == S else 1 for t, n in zip(ts, sides)]
    else:
        kinds = [int(k) for k in kinds]
        S = sides[0] * (2 if kinds[0] == 1 else 1)
    if any(n * (2 if k == 1 else 1) != S for n, k in zip(sides, kinds)):
        raise ValueError(f"concat_frames: panels of sides {sides} and kinds {kinds} do not come to one size")
    if S < 4 or S % 4 or S > 16384:
        raise ValueError(f"concat_frames: panel size {S} (a multiple of 4 from 4 to 16384)")
    B = max(t.shape[0] for t in ts)
    if shared is None:
        shared = [t.shape[0] == 1 and B > 1 for t in ts]
    shared = [int(bool(f)) for f in shared]
    if any(t.shape[0] != (1 if f else B) for t, f in zip(ts, shared)):
        raise ValueError(f"concat_frames: panels hold {[t.shape[0] for t in ts]} images: B = {B}, or one where shared")
    ts = [t.to(e.device).contiguous() for t in ts]
    out = e._out(out, (B, S, P * S, 3), torch.uint8)
    ptrs = (C.c_void_p * P)(*[t.data_ptr() for t in ts])
    e._call("cs_concat_frames", B, P, S, ptrs, (C.c_int * P)(*kinds), (C.c_int * P)(*shared), out)
    return out


YUV_LAYOUTS = {"nv12": 0, "i420": 1}          # cs_yuv_to_rgb / cs_rgb_to_yuv: layout (i420 is ffmpeg's yuv420p)
YUV_MATRICES = {"bt601": 0, "bt709": 1}       # matrix


def yuv_format(who, layout, matrix, full_range):
    """The three format arguments of the 4:2:0 calls -> the C ABI's integers; ValueError names the argument."""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f"{who}: layout {layout!r} is none of {sorted(YUV_LAYOUTS)}")
    if matrix not in YUV_MATRICES:
        raise ValueError(f"{who}: matrix {matrix!r} is none of {sorted(YUV_MATRICES)}")
    if not isinstance(full_range, (bool, np.bool_)) and full_range not in (0, 1):
        raise ValueError(f"{who}: full_range {full_range!r} is neither True nor False")
    return YUV_LAYOUTS[layout], YUV_MATRICES[matrix], int(bool(full_range))


def yuv_frame_hw(who, shape, what="yuv"):
    """(F, 3 Ho / 2, Wo) -> (Ho, Wo), both even and in 2 .. 16384; ValueError names `what`."""
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 3 or shape[1] % 3 or shape[2] < 2 or shape[2] % 2 or max(shape[1] // 3 * 2, shape[2]) > 16384:
        raise ValueError(f"{who}: {what}: expected (F, 3 Ho / 2, Wo) uint8 4:2:0 frames with Ho and Wo even, 2 to 16384, got shape {tuple(shape)}")
    return int(shape[1]) // 3 * 2, int(shape[2])


def _disjoint(who, a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    if a0 < b0 + b.numel() and b0 < a0 + a.numel():
        raise ValueError(f"{who}: rgb and yuv overlap in memory")


def yuv_to_rgb(e: Engine, yuv, layout="nv12", matrix="bt601", full_range=False, out=None):
    """cs_yuv_to_rgb (include/canonswap_yuv.h): yuv (F, 3 Ho / 2, Wo) uint8, host or device - F frames of NV12 (the Y plane, then interleaved
    U V rows) or I420 (Y, U plane, V plane), the memory of ffmpeg's rawvideo nv12 / yuv420p - -> (F, Ho, Wo, 3) uint8 RGB on the device, the
    block's chroma replicated to its 2 x 2 pixels.  matrix "bt601" or "bt709"; full_range False: Y 16 - 235, chroma 16 - 240.  Integer
    arithmetic, bit-equal to tests/yuv_ref.py.  No engine scratch, no allocation but the result, no host wait for device frames."""
    who = "yuv_to_rgb"
    fmt = yuv_format(who, layout, matrix, full_range)
    t = torch.as_tensor(yuv)
    if t.dtype != torch.uint8:
        raise ValueError(f"{who}: yuv: expected uint8, got {t.dtype}")
    Ho, Wo = yuv_frame_hw(who, t.shape)
    t = t.to(e.device).contiguous()
    try:
        rgb = e._out(out, (t.shape[0], Ho, Wo, 3), torch.uint8)
    except ValueError as err:
        raise ValueError(f"{who}: out: {err}") from None
    _disjoint(who, rgb, t)
    e._call("cs_yuv_to_rgb", int(t.shape[0]), t, Ho, Wo, *fmt, rgb)
    return rgb


def rgb_to_yuv(e: Engine, rgb, layout="nv12", matrix="bt601", full_range=False, keep=None, out=None):
    """cs_rgb_to_yuv: rgb (F, Ho, Wo, 3) uint8, host or device, Ho and Wo even -> (F, 3 Ho / 2, Wo) uint8 on the device in `layout`: Y per
    pixel, U and V from the sums of R, G and B over the 2 x 2 block.  keep: the device YUV tensor the frames came from (contiguous, of the
    result's shape); it is updated in place and returned: a block whose four RGB pixels still are what its six bytes decode to keeps those
    bytes, every other block is re-encoded, so what nothing wrote since yuv_to_rgb comes back as it went in.  Pass keep or out, not both."""
    who = "rgb_to_yuv"
    fmt = yuv_format(who, layout, matrix, full_range)
    t = u8_images(rgb, True, 1, "rgb", who)
    F, Ho, Wo = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    if Ho < 2 or Wo < 2 or Ho % 2 or Wo % 2 or max(Ho, Wo) > 16384:
        raise ValueError(f"{who}: rgb: 4:2:0 needs an even Ho and Wo from 2 to 16384, got {Ho} x {Wo}")
    if keep is not None and out is not None:
        raise ValueError(f"{who}: keep / out: keep is the output as well; pass one of the two")
    t = t.to(e.device).contiguous()
    try:
        yuv = e._out(keep if keep is not None else out, (F, Ho * 3 // 2, Wo), torch.uint8)
    except ValueError as err:
        raise ValueError(f"{who}: {'keep' if keep is not None else 'out'}: {err}") from None
    _disjoint(who, t, yuv)
    e._call("cs_rgb_to_yuv", F, t, Ho, Wo, *fmt, int(keep is not None), yuv)
    return yuv


class SoftErosion:
    """SoftErosion(kernel_size, threshold, iterations) of crop.py:21-47; call -> (soft mask, hard mask), inputs (N,1,H,W)."""

    def __init__(self, engine: Engine, kernel_size=15, threshold=0.6, iterations=1):
        self.e, self.kernel_size, self.threshold, self.iterations = engine, kernel_size, threshold, iterations
        r = kernel_size // 2
        # the kernel exactly as the reference builds it (crop.py:29-35), in fp32 on the host
        y, x = torch.meshgrid(torch.arange(0., kernel_size), torch.arange(0., kernel_size), indexing="ij")
        dist = torch.sqrt((x - r) ** 2 + (y - r) ** 2)
        k = dist.max() - dist
        k /= k.sum()
        self.weight = k.view(1, 1, kernel_size, kernel_size).to(engine.device)

    def __call__(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError("SoftErosion expects (N, 1, H, W)")
        e = self.e
        m = x.to(e.device).float().contiguous()
        N, _, H, W = m.shape
        soft = torch.empty_like(m)
        hard = torch.empty((N, 1, H, W), dtype=torch.uint8, device=e.device)
        e._call("cs_soft_erosion", N, H, W, m, self.weight, self.kernel_size, float(self.threshold), self.iterations, soft, hard)
        return soft, hard.bool()

    forward = __call__


def soft_erosion_frames(e: Engine, masks, weight, kernel_size=21, threshold=0.9, iterations=3, out=None):
    """B independent SoftErosion calls (the pipeline's loop calls the module once per frame, can_swap_pipeline_e2e.py:274: the maximum of
    crop.py:45 is that frame's) in one launch sequence.  masks: (B,H,W) uint8 0/1 labels or fp32, on the device -> soft masks (B,H,W) fp32."""
    m = torch.as_tensor(masks)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3:
        raise ValueError("soft_erosion_frames expects (B, H, W) masks")
    if m.dtype not in (torch.uint8, torch.float32):
        m = m.to(torch.uint8) if not m.dtype.is_floating_point else m.float()
    m = m.to(e.device).contiguous()
    B, H, W = m.shape
    out = e._out(out, (B, H, W), torch.float32)
    if weight.dtype != torch.float32 or weight.numel() != kernel_size * kernel_size or not weight.is_contiguous() or weight.device != e.device:
        raise ValueError("weight must be the contiguous kernel_size x kernel_size fp32 kernel on the engine's device")
    e._call("cs_soft_erosion_frames", B, H, W, m, int(m.dtype == torch.uint8), weight, kernel_size, float(threshold), iterations, out, None)
    return out


def paste_back_batch(e: Engine, crops, masks_crop, M_c2o, imgs_ori, out=None):
    """prepare_paste_back + paste_back (crop.py:515-529) of B frames in one launch: crops (B,Hc,Wc,3) u8, masks_crop (B,Hc,Wc) fp32 soft masks
    in the crop frame, M_c2o (B,2,3) or (B,3,3) host matrices crop -> original, imgs_ori (B,Ho,Wo,3) u8 -> (B,Ho,Wo,3) u8."""
    who = "paste_back_batch"
    crops, ori = u8_images(crops, True, 1, "crops", who), u8_images(imgs_ori, True, 1, "imgs_ori", who)
    crops, ori = crops.to(e.device).contiguous(), ori.to(e.device).contiguous()
    B = crops.shape[0]
    mc = _masks_of(masks_crop, crops, who).to(e.device).float().contiguous()
    if ori.shape[0] != B:
        raise ValueError(f"{who}: imgs_ori must hold the {B} frames of the crops, got {ori.shape[0]}")
    mm, mp = _m6_of(M_c2o, B, "M_c2o", who)
    out = e._out(out, ori.shape, torch.uint8)
    e._call("cs_paste_back_batch", B, crops, mc, crops.shape[1], crops.shape[2], mp, ori, out, ori.shape[1], ori.shape[2])
    return out


def paste_back_shared(e: Engine, crops, M_c2o, img_ori, mask_ori, out=None):
    """paste_back (crop.py:523-529) of B generated frames into ONE image, as the loop of can_swap_pipeline_v2i.py:317-321 does on a fresh copy
    of the source image per frame: crops (B,Hc,Wc,3) u8, M_c2o 2x3 / 3x3 host, img_ori (Ho,Wo,3) u8, mask_ori (Ho,Wo) fp32 (prepare_paste_back's
    result, :255-258) -> (B,Ho,Wo,3) u8, frame b bit-equal to paste_back(crops[b], M_c2o, img_ori, mask_ori)."""
    crops, ori = u8_images(crops, True, 1, "crops", "paste_back_shared"), u8_images(img_ori, False, 1, "img_ori", "paste_back_shared")
    crops, ori = crops.to(e.device).contiguous(), ori.to(e.device).contiguous()
    mo = _mask_hw(e, mask_ori)
    if tuple(mo.shape) != tuple(ori.shape[:2]):
        raise ValueError("mask_ori must have the size of img_ori")
    B = crops.shape[0]
    out = e._out(out, (B,) + tuple(ori.shape), torch.uint8)
    mm, mp = _m6(M_c2o)
    e._call("cs_paste_back_shared", B, crops, crops.shape[1], crops.shape[2], mo, mp, ori, out, ori.shape[0], ori.shape[1])
    return out


def _u8_hwc(e: Engine, img, name, who):
    return u8_images(img, False, 1, name, who).to(e.device).contiguous()


def warp_affine_u8(e: Engine, img, M, dsize):
    """cv2.warpAffine(img, M[:2], dsize=(W, H), flags=cv2.INTER_LINEAR) for HxWx3 uint8 (crop.py:49-63 _transform_img)."""
    src = _u8_hwc(e, img, "img", "warp_affine_u8")
    Wd, Hd = int(dsize[0]), int(dsize[1])
    dst = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device=e.device)
    m, mp = _m6(M)
    e._call("cs_warp_affine_u8", src, src.shape[0], src.shape[1], mp, dst, Hd, Wd)
    return dst


def prepare_paste_back(e: Engine, mask_crop, crop_M_c2o, dsize):
    """crop.py:515-521 with if_float=True (the call of can_swap_pipeline_e2e.py:279): float mask -> frame of the original image.
    mask_crop: HxW or HxWx3 (the reference stacks three identical channels); returns HoxWo float32 on the device."""
    m = _mask_hw(e, mask_crop)
    Wd, Hd = int(dsize[0]), int(dsize[1])
    dst = torch.empty((Hd, Wd), dtype=torch.float32, device=e.device)
    mm, mp = _m6(crop_M_c2o)
    e._call("cs_warp_affine_f32", m, m.shape[0], m.shape[1], mp, dst, Hd, Wd)
    return dst


def paste_back(e: Engine, img_crop, M_c2o, img_ori, mask_ori):
    """crop.py:523-529: result = warp(img_crop); clip(mask_ori * result + (1 - mask_ori) * img_ori, 0, 255) as uint8."""
    crop, ori = _u8_hwc(e, img_crop, "img_crop", "paste_back"), _u8_hwc(e, img_ori, "img_ori", "paste_back")
    mo = _mask_hw(e, mask_ori)
    if tuple(mo.shape) != tuple(ori.shape[:2]):
        raise ValueError("mask_ori must have the size of img_ori")
    out = torch.empty_like(ori)
    mm, mp = _m6(M_c2o)
    e._call("cs_paste_back", crop, None, mo, crop.shape[0], crop.shape[1], mp, ori, out, ori.shape[0], ori.shape[1])
    return out


def paste_back_fused(e: Engine, img_crop, mask_crop, M_c2o, img_ori):
    """prepare_paste_back + paste_back in one launch: the soft mask stays in the crop frame (HcxWc float32)."""
    crop, ori = _u8_hwc(e, img_crop, "img_crop", "paste_back_fused"), _u8_hwc(e, img_ori, "img_ori", "paste_back_fused")
    mc = _mask_hw(e, mask_crop)
    if tuple(mc.shape) != tuple(crop.shape[:2]):
        raise ValueError("mask_crop must have the size of img_crop")
    out = torch.empty_like(ori)
    mm, mp = _m6(M_c2o)
    e._call("cs_paste_back", crop, mc, None, crop.shape[0], crop.shape[1], mp, ori, out, ori.shape[0], ori.shape[1])
    return out


def prepare_crops(e: Engine, crops_u8, out=None) -> torch.Tensor:
    """uint8 crops (B,512,512,3) or (B,256,256,3), host or device -> (B,3,256,256) fp32 in [0,1] on the device: the cropper's
    cv2.resize(..., (256, 256), INTER_AREA) (cropper.py:209) fused with prepare_source / prepare_videos (can_swap_e2e.py:126-163)."""
    t = torch.as_tensor(crops_u8)
    t = u8_images(t[None] if t.dim() == 3 else t, True, 0, "crops_u8", "prepare_crops").to(e.device).contiguous()
    B, H, W, _ = t.shape
    out = e._out(out, (B, 3, 256, 256), torch.float32)
    e._call("cs_prepare_crops", B, t, H, W, out)
    return out


def _crop_M(e: Engine, who, frames, M_o2c, frame_index, dsize, out, want_I, out_I):
    """crop_frames_M (frame_index None: crop b from frame b, cs_crop_frames) and crop_faces_M (B matrices, crop b from frame frame_index[b],
    cs_crop_faces)."""
    fr = u8_images(frames, True, 1, "frames", who).to(e.device).contiguous()
    F, dsize = fr.shape[0], int(dsize)
    B = F if frame_index is None else int(np.shape(M_o2c)[0]) if np.ndim(M_o2c) == 3 else -1
    mm, mp = _m6_of(M_o2c, B, "M_o2c", who)
    idx = None if frame_index is None else frame_index_of(frame_index, B, F)
    want_I = want_I or out_I is not None
    crops = e._out(out, (B, dsize, dsize, 3), torch.uint8)
    I = e._out(out_I, (B, 3, 256, 256), torch.float32) if want_I else None
    if idx is None:
        e._call("cs_crop_frames", B, fr, fr.shape[1], fr.shape[2], mp, dsize, crops, I)
    else:
        e._call("cs_crop_faces", B, F, fr, fr.shape[1], fr.shape[2], _index_ptr(idx), mp, dsize, crops, I)
    return {"crops": crops, "I": I} if want_I else {"crops": crops}


def crop_frames_M(e: Engine, frames, M_o2c, dsize, out=None, want_I=False, out_I=None):
    """crop_image_mo2c's image step (crop.py:457-461) of B frames in one launch: frames (B,Ho,Wo,3) u8, M_o2c (B,2,3) or (B,3,3) host matrices original ->
    crop, dsize a multiple of 4 -> {"crops": (B,dsize,dsize,3) u8 on the device, crops[b] = cv2.warpAffine(frames[b], M_o2c[b][:2], (dsize, dsize),
    INTER_LINEAR)[, "I": (B,3,256,256) fp32 = prepare_crops(crops), from the same launch; dsize 256 or 512 only]}."""
    return _crop_M(e, "crop_frames_M", frames, M_o2c, None, dsize, out, want_I, out_I)


def crop_frames(e: Engine, frames, lmk, dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True, out=None, want_I=False, out_I=None):
    """crop_image (crop.py:429-455) of B frames, as the cropper runs it per frame (cropper.py:196-204; defaults: CropConfig's): frames
    (B,Ho,Wo,3) u8, lmk (B,N,2) tracked landmarks in the frame (host; (N,2) for one frame) -> {"crops" (B,dsize,dsize,3) u8 on the device,
    "M_o2c", "M_c2o" (B,3,3) float32 on the host, "lmk_crop" (B,N,2) on the host[, "I" (B,3,256,256) fp32 with want_I]}.  The matrices come from
    crop.crop_matrices on the host (a few hundred flops per frame), the image step is one launch."""
    M_o2c, M_c2o, lmk_crop = crop_geometry.crop_matrices(lmk, dsize=dsize, scale=scale, vy_ratio=vy_ratio, flag_do_rot=flag_do_rot)
    if M_o2c.shape[0] != np.shape(frames)[0]:
        raise ValueError(f"{M_o2c.shape[0]} landmark sets for {np.shape(frames)[0]} frames")
    res = crop_frames_M(e, frames, M_o2c, dsize, out=out, want_I=want_I, out_I=out_I)
    res.update(M_o2c=M_o2c, M_c2o=M_c2o, lmk_crop=lmk_crop)
    return res


def frame_index_of(frame_index, B, F, who="frame_index"):
    """The frame of each face -> B contiguous int32 on the host: B integers, non-decreasing (the faces of a frame are contiguous, in paste
    order), each in [0, F).  Raises ValueError naming the argument otherwise."""
    a = np.asarray(frame_index.cpu() if isinstance(frame_index, torch.Tensor) else frame_index)
    if a.ndim != 1 or a.shape[0] != B:
        raise ValueError(f"{who}: expected {B} frame numbers, one per face, got shape {tuple(a.shape)}")
    if B and a.dtype.kind not in "iu":
        raise ValueError(f"{who}: expected integers, got {a.dtype}")
    a = a.astype(np.int64)
    if B and (a.min() < 0 or a.max() >= F):
        raise ValueError(f"{who}: frame numbers must lie in [0, {F}), got {int(a.min())} .. {int(a.max())}")
    if B > 1 and (np.diff(a) < 0).any():
        raise ValueError(f"{who}: must not decrease (decreases at face {int(np.argmax(np.diff(a) < 0)) + 1}): the faces of a frame are contiguous")
    return np.ascontiguousarray(a, dtype=np.int32)


def _index_ptr(idx):
    return idx.ctypes.data_as(C.POINTER(C.c_int))


def crop_faces_M(e: Engine, frames, M_o2c, frame_index, dsize, out=None, want_I=False, out_I=None):
    """crop_frames_M for B faces in F frames: frames (F,Ho,Wo,3) u8, M_o2c (B,2,3) or (B,3,3) host matrices, frame_index B host ints (non-decreasing,
    in [0, F); a frame may own several faces or none) -> {"crops": (B,dsize,dsize,3) u8, crops[b] = cv2.warpAffine(frames[frame_index[b]], M_o2c[b][:2],
    (dsize, dsize), INTER_LINEAR)[, "I": (B,3,256,256) fp32 = prepare_crops(crops)]}: the bits of crop_frames_M on frames[frame_index], no frame
    gathered.  B >= 1."""
    return _crop_M(e, "crop_faces_M", frames, M_o2c, frame_index, dsize, out, want_I, out_I)


def crop_faces(e: Engine, frames, lmk, frame_index, dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True, out=None, want_I=False, out_I=None):
    """crop_frames for B faces in F frames: frames (F,Ho,Wo,3) u8, lmk (B,N,2) landmarks of the B faces in their frames (host), frame_index as in
    crop_faces_M -> crop_frames' dict, per face: {"crops" (B,dsize,dsize,3) u8, "M_o2c", "M_c2o" (B,3,3), "lmk_crop" (B,N,2)[, "I"]}."""
    M_o2c, M_c2o, lmk_crop = crop_geometry.crop_matrices(lmk, dsize=dsize, scale=scale, vy_ratio=vy_ratio, flag_do_rot=flag_do_rot)
    frame_index_of(frame_index, M_o2c.shape[0], np.shape(frames)[0])      # one frame number per landmark set: the error names frame_index
    res = crop_faces_M(e, frames, M_o2c, frame_index, dsize, out=out, want_I=want_I, out_I=out_I)
    res.update(M_o2c=M_o2c, M_c2o=M_c2o, lmk_crop=lmk_crop)
    return res


def paste_back_faces(e: Engine, crops, masks_crop, M_c2o, frame_index, imgs_ori, out=None):
    """prepare_paste_back + paste_back (crop.py:515-529) of B faces into F frames, face b into frame frame_index[b], the faces of a frame in their
    order and each on the result of the one before, in one pass over every frame: crops (B,Hc,Wc,3) u8, masks_crop (B,Hc,Wc) fp32 soft masks in the
    crop frame, M_c2o (B,2,3) or (B,3,3) host, frame_index B host ints (non-decreasing, in [0, F)), imgs_ori (F,Ho,Wo,3) u8 -> (F,Ho,Wo,3) u8; a frame
    without a face is copied.  out may be the imgs_ori tensor itself (in place).  B = 0 (crops (0,Hc,Wc,3)) copies the frames.  Bit-equal to
    paste_back_fused face by face, and with frame_index = arange(B) to paste_back_batch."""
    who = "paste_back_faces"
    crops, ori = u8_images(crops, True, 0, "crops", who), u8_images(imgs_ori, True, 1, "imgs_ori", who)
    crops, ori = crops.to(e.device).contiguous(), ori.to(e.device).contiguous()
    B, F = crops.shape[0], ori.shape[0]
    mc = _masks_of(masks_crop, crops, who).to(e.device).float().contiguous()
    idx = frame_index_of(frame_index, B, F)
    mm, mp = _m6_of(M_c2o, B, "M_c2o", who) if B else (None, None)
    out = e._out(out, ori.shape, torch.uint8)
    e._call("cs_paste_back_faces", B, F, crops if B else None, mc if B else None, crops.shape[1], crops.shape[2],
            _index_ptr(idx) if B else None, mp, ori, out, ori.shape[1], ori.shape[2])
    return out


def _device_tensor(e: Engine, t, shape, dtype, name, who):
    """A caller's tensor exactly as a kernel reads or writes it - dtype, shape, on the engine's device, contiguous - or ValueError naming the
    argument; checked in that order, so the message says what is wrong first.  shape: None where any is wanted (-1: any size of that axis)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if len(shape) != t.dim() or any(want not in (-1, have) for want, have in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} must have shape {tuple(shape)} (-1: any), got {tuple(t.shape)}")
    if t.device != e.device:
        raise ValueError(f"{who}: {name} must be on {e.device}, it is on {t.device}: it is read where it is, not uploaded")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    return t


def crop_lmk(e: Engine, frames, lmk, frame_index=None, dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True, status=None, status_mark=1, out=None,
             want_I=False, want_lmk_crop=False):
    """crop_faces from landmarks that never leave the device (cs_crop_lmk, one launch per 64 faces): frames (F,Ho,Wo,3) u8; lmk (B,N,2) float32 ON
    THE DEVICE, the landmarks of the B faces in their frames (landmarks.layout_of(N) says which span the eye-lip axis); frame_index as in crop_faces
    (None: face b in frame b) -> {"crops": (B,dsize,dsize,3) u8, "M": (B,18) fp32 = M_o2c 3x3 | M_c2o 3x3 with the bits lmk_input writes,
    "status": (B,) int32[, "I": (B,3,256,256) fp32 = prepare_crops(crops) with want_I (dsize 256 or 512)][, "lmk_crop": (B,N,2) fp32, the
    landmarks in the crop's frame, with want_lmk_crop]}, all on the device; nothing is downloaded and nothing waits for the device.  crops equals
    crop_faces_M on M[:, :9] downloaded and widened.  A face the guard refuses (a landmark not finite, an empty box, a matrix entry above 1e6) gets
    status_mark in status and zeros everywhere else; status is sticky (a non-zero entry on entry: refused, kept): pass the tracker's, or None to
    start at zero.  out: a dict with any of "crops", "M", "I", "lmk_crop" as the caller's buffers.
    LandmarkTracker.track's (N,S,Np,2) output reshaped to (N S,Np,2) with frame_index = repeat(arange(N), S) is a valid lmk: the tracker, this
    crop, the generator and paste_back_faces_dev are then enqueued one behind the other without a host wait."""
    from .landmarks import layout_of      # (landmarks imports this module)
    who = "crop_lmk"
    fr = u8_images(frames, True, 1, "frames", who)
    F = int(fr.shape[0])
    pts = _device_tensor(e, lmk, (-1, -1, 2), torch.float32, "lmk", who)
    B, N = int(pts.shape[0]), int(pts.shape[1])
    if B < 1 or N < 1:
        raise ValueError(f"{who}: lmk must hold at least one face and one landmark, got {tuple(pts.shape)}")
    if frame_index is None and B != F:
        raise ValueError(f"{who}: frame_index: {B} landmark sets for {F} frames and no frame_index")
    idx = frame_index_of(np.arange(B) if frame_index is None else frame_index, B, F, f"{who}: frame_index")
    layout = layout_of(N)
    dsize = int(dsize)
    if not 4 <= dsize <= 16384 or dsize % 4:
        raise ValueError(f"{who}: dsize {dsize} (a multiple of 4 from 4 to 16384)")
    if int(status_mark) == 0:
        raise ValueError(f"{who}: status_mark must not be 0")
    out = dict(out or {})
    unknown = set(out) - {"crops", "M", "I", "lmk_crop"}
    if unknown:
        raise ValueError(f"{who}: out has no buffer named {sorted(unknown)}")
    want = {"crops": True, "M": True, "I": want_I or out.get("I") is not None, "lmk_crop": want_lmk_crop or out.get("lmk_crop") is not None}
    if want["I"] and dsize not in (256, 512):
        raise ValueError(f"{who}: want_I goes with dsize 256 or 512 (got {dsize})")
    shapes = {"crops": ((B, dsize, dsize, 3), torch.uint8), "M": ((B, 18), torch.float32), "I": ((B, 3, 256, 256), torch.float32),
              "lmk_crop": ((B, N, 2), torch.float32)}
    for k, t in out.items():
        if t is not None:
            _device_tensor(e, t, *shapes[k], f"out[{k!r}]", who)
    if status is not None:
        _device_tensor(e, status, (B,), torch.int32, "status", who)
    buf = {k: (out[k] if out.get(k) is not None else torch.empty(shapes[k][0], dtype=shapes[k][1], device=e.device)) if want[k] else None for k in shapes}
    status = status if status is not None else torch.zeros((B,), dtype=torch.int32, device=e.device)
    fr = fr.to(e.device).contiguous()
    e._call("cs_crop_lmk", B, F, fr, fr.shape[1], fr.shape[2], _index_ptr(idx), pts, N, C.byref(layout), dsize, float(scale), float(vy_ratio),
            int(bool(flag_do_rot)), int(status_mark), buf["M"], buf["crops"], buf["I"], buf["lmk_crop"], status)
    res = {"crops": buf["crops"], "M": buf["M"], "status": status}
    res.update({k: buf[k] for k in ("I", "lmk_crop") if want[k]})
    return res


def paste_back_faces_dev(e: Engine, crops, masks_crop, M, frame_index, imgs_ori, status=None, out=None):
    """paste_back_faces with the matrices read from device memory (cs_paste_back_faces_dev): M (B,18) float32 ON THE DEVICE, crop_lmk's or
    lmk_input's (M_c2o = M[:, 9:]); status (B,) int32 on the device or None: a face with a non-zero entry is skipped as if it were not listed;
    everything else as paste_back_faces takes it -> (F,Ho,Wo,3) u8, the bytes of paste_back_faces on M[:, 9:] downloaded and widened.  out may be
    imgs_ori itself (in place); B = 0 copies the frames (M is not read and may be None).  Nothing is downloaded and nothing waits for the device."""
    who = "paste_back_faces_dev"
    crops, ori = u8_images(crops, True, 0, "crops", who), u8_images(imgs_ori, True, 1, "imgs_ori", who)
    B, F = int(crops.shape[0]), int(ori.shape[0])
    mc = _masks_of(masks_crop, crops, who)
    idx = frame_index_of(frame_index, B, F, f"{who}: frame_index")
    if B:
        _device_tensor(e, M, (B, 18), torch.float32, "M", who)
    if B and status is not None:
        _device_tensor(e, status, (B,), torch.int32, "status", who)
    if out is not None:
        _device_tensor(e, out, tuple(ori.shape), torch.uint8, "out", who)
    crops, ori, mc = crops.to(e.device).contiguous(), ori.to(e.device).contiguous(), mc.to(e.device).float().contiguous()
    out = out if out is not None else torch.empty_like(ori)
    e._call("cs_paste_back_faces_dev", B, F, crops if B else None, mc if B else None, crops.shape[1], crops.shape[2], _index_ptr(idx) if B else None,
            M if B else None, status if B else None, ori, out, ori.shape[1], ori.shape[2])
    return out


class FrameStreamer:
    """Streams the uint8 crops of a video to the device in batches (N3): batch k+1 is copied from pinned host memory on a side
    stream while batch k is being processed, instead of prepare_videos' whole-video upload as fp32 (can_swap_e2e.py:147-163,
    786 KB per frame; a uint8 512x512 crop is the same 786 KB but is converted on the device, a 256x256 one is 196 KB).

        for I_batch, (start, stop) in FrameStreamer(engine, crops_u8, batch=32): ...   # I_batch: (n, 3, 256, 256) fp32
    """

    def __init__(self, engine: Engine, crops_u8, batch: int = 32):
        self.e, self.batch = engine, batch
        self.frames = crops_u8
        self.n = len(crops_u8)
        f0 = np.asarray(crops_u8[0])
        if f0.dtype != np.uint8 or f0.ndim != 3 or f0.shape[2] != 3 or f0.shape[0] not in (256, 512) or f0.shape[0] != f0.shape[1]:
            raise ValueError("expected 256x256x3 or 512x512x3 uint8 crops")
        self.shape = f0.shape
        self.copy_stream = torch.cuda.Stream(device=engine.device)
        self.pinned = [torch.empty((batch,) + tuple(self.shape), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty((batch,) + tuple(self.shape), dtype=torch.uint8, device=engine.device) for _ in range(2)]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [torch.cuda.Event(), torch.cuda.Event()]

    def _stage(self, k):
        a, b = k * self.batch, min(self.n, (k + 1) * self.batch)
        s = k % 2
        self.consumed[s].synchronize()                       # the pinned slot is free again (first use: event never recorded)
        for j in range(a, b):
            self.pinned[s][j - a].copy_(torch.from_numpy(np.ascontiguousarray(self.frames[j])))
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(self.consumed[s])
            self.dev[s][: b - a].copy_(self.pinned[s][: b - a], non_blocking=True)
            self.ready[s].record(self.copy_stream)
        return a, b

    def __iter__(self):
        nb = (self.n + self.batch - 1) // self.batch
        if nb == 0:
            return
        span = self._stage(0)
        for k in range(nb):
            nxt = self._stage(k + 1) if k + 1 < nb else None          # upload of the next batch overlaps this batch's work
            s = k % 2
            cur = torch.cuda.current_stream(self.e.device)
            cur.wait_event(self.ready[s])
            out = prepare_crops(self.e, self.dev[s][: span[1] - span[0]])
            self.consumed[s].record(cur)
            yield out, span
            span = nxt
