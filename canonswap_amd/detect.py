"""The face detector's two sides on the device: frames -> the network's blob, the network's outputs -> faces.

The reference detects with SCRFD (src/utils/dependencies/insightface/model_zoo/scrfd.py), reached through ``Face_detect_crop.get``
(insightface_func/face_detect_crop_single.py:63-82, _multi.py:63-100; can_swap_pipeline_e2e.py:93-98, can_swap_pipeline_v2i.py:113-118, 136-145).
The network is an ONNX file the reference downloads and stays the caller's (MIGraphX, ONNX Runtime's ROCm provider, a torch port): one call
between two of ours.

* ``det_geometry``   scrfd.py:224-232: the resized size inside the letterbox and det_scale, truncating int() included
* ``det_lut``        scrfd.py:154 blobFromImage's (u8 - mean) * (1 / std) as a (3, 256) table
* ``det_input``      scrfd.py:224-235 + :154 of F frames in one launch (cs_det_input)
* ``det_decode``     scrfd.py:160-218 + :239-303 of F frames in one launch (cs_det_decode): threshold, distance decode, sort, NMS, max_num
* ``FaceDetector``   SCRFD.detect and Face_detect_crop.get around the caller's ``net``: faces, key points and ``frame_index`` for
                     ``chain.crop(frames, kps, frame_index=)``, aligned crops for ``getid_crops``

Both kernels live in csrc/detect.hip; there is no torch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, align
from .engine import Engine, u8_images

DET_MEAN, DET_STD = 127.5, 128.0                    # SCRFD.input_mean / input_std (scrfd.py:107-108)
LAYOUTS = {3: ((8, 16, 32), 2), 5: ((8, 16, 32, 64, 128), 1)}      # levels -> (strides, anchors per cell) (scrfd.py:114-131)
SWAP_RB = True                                      # forward's blobFromImage(..., swapRB=True) (scrfd.py:154), whatever image it is handed


def _size2(det_size):
    try:
        w, h = (int(v) for v in det_size)
    except (TypeError, ValueError):
        raise ValueError(f"det_size: expected (width, height), got {det_size!r}") from None
    if (w, h) != tuple(det_size) or not (1 <= w <= 16384 and 1 <= h <= 16384):
        raise ValueError(f"det_size: (width, height) integers in [1, 16384], got {det_size!r}")
    return w, h


def det_geometry(Ho, Wo, det_size=(640, 640)):
    """scrfd.py:224-232 for an Ho x Wo frame and input_size = det_size = (width, height), as the reference passes it: -> (new_height, new_width,
    det_scale), the resized image's size inside the letterbox with the reference's truncating int(), det_scale = float(new_height) / Ho."""
    Ho, Wo = int(Ho), int(Wo)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"det_geometry: frame {Ho}x{Wo}")
    input_size = _size2(det_size)
    im_ratio = float(Ho) / Wo
    model_ratio = float(input_size[1]) / input_size[0]
    if im_ratio > model_ratio:
        new_height = input_size[1]
        new_width = int(new_height / im_ratio)
    else:
        new_width = input_size[0]
        new_height = int(new_width * im_ratio)
    return new_height, new_width, float(new_height) / Ho


def det_lut(mean=DET_MEAN, std=DET_STD) -> np.ndarray:
    """(3, 256) fp32: what cv2.dnn.blobFromImage(img, 1.0 / std, size, (mean, mean, mean), swapRB=True) (scrfd.py:154) makes of byte v in OUTPUT plane
    c: the image as float32, minus the mean, times the scale factor, every step in float32.  mean: one number or three (per output plane).  With
    the detector's constants (127.5, 128.0) every entry is exact.  cs_det_input looks this up and computes nothing in float."""
    m = [float(mean)] * 3 if np.ndim(mean) == 0 else [float(v) for v in mean]
    std = float(std)
    if len(m) != 3 or std == 0 or not np.isfinite(std):
        raise ValueError("det_lut: mean is one number or three, std a nonzero number")
    image = np.arange(256, dtype=np.uint8).astype(np.float32)
    scalefactor = np.float32(1.0 / std)
    lut = (image[None, :] - np.array(m, dtype=np.float32)[:, None]) * scalefactor
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    return np.ascontiguousarray(lut)


def _det_lut_on(e: Engine, mean, std):
    """The table on the engine's device, uploaded once per engine and set of constants."""
    key = (tuple([float(mean)] * 3 if np.ndim(mean) == 0 else [float(v) for v in mean]), float(std))
    return e.device_table(("det_lut",) + key, lambda: det_lut(*key))


def _frames(frames, who):
    t = torch.as_tensor(frames)
    return u8_images(t[None] if t.dim() == 3 else t, True, 1, "frames", who)


def det_input(e: Engine, frames, det_size=(640, 640), swap_rb=SWAP_RB, mean=DET_MEAN, std=DET_STD, out=None):
    """SCRFD.detect's letterbox and forward's blob (scrfd.py:224-235, :154) of F frames in one launch: frames (F,Ho,Wo,3) or (Ho,Wo,3) uint8, host or
    device -> blob (F,3,Hd,Wd) fp32 on the device, (Wd, Hd) = det_size: cv2.resize to det_geometry's size (OpenCV's 8-bit INTER_LINEAR, PARITY
    UNPINNED), zeros below and to the right, (u8 - mean) / std as a table, channels first.  swap_rb=True is the reference's swapRB=True - the flag
    of BOTH of its calls, on cv2.imread's BGR frames (can_swap_pipeline_e2e.py:93) and on RGB crops (can_swap_pipeline_v2i.py:230) alike: plane c of
    the blob is channel 2 - c of the frame.  out: the caller's (F,3,Hd,Wd) fp32 buffer."""
    t = _frames(frames, "det_input")
    F, Ho, Wo, _ = t.shape
    Wd, Hd = _size2(det_size)
    nh, nw, _ = det_geometry(Ho, Wo, (Wd, Hd))
    if nh < 1 or nw < 1:
        raise ValueError(f"det_input: a {Ho}x{Wo} frame resizes to {nh}x{nw} inside {Hd}x{Wd}")
    t = t.to(e.device).contiguous()
    blob = e._out(out, (F, 3, Hd, Wd), torch.float32)
    lut = _det_lut_on(e, mean, std)
    e._call("cs_det_input", F, t, Ho, Wo, Hd, Wd, int(bool(swap_rb)), lut, blob)
    return blob


def _net_outs(e: Engine, outs, det_size):
    """The network's 6, 9, 10 or 15 outputs -> (n_levels, strides, num_anchors, F, contiguous fp32 device tensors scores + bbox [+ kps])."""
    outs = list(outs)
    if len(outs) not in (6, 9, 10, 15):
        raise ValueError(f"det_decode: {len(outs)} network outputs (6 or 9: three levels without / with key points; 10 or 15: five levels)")
    n_levels = 3 if len(outs) in (6, 9) else 5
    strides, na = LAYOUTS[n_levels]
    Wd, Hd = _size2(det_size)
    ts, F = [], None
    for k, o in enumerate(outs):
        if not isinstance(o, torch.Tensor):
            raise ValueError(f"det_decode: output {k} is not a torch.Tensor on the engine's device")
        if o.device != e.device:
            raise ValueError(f"det_decode: output {k} lives on {o.device}, the engine on {e.device}")
        if o.dtype != torch.float32:
            raise ValueError(f"det_decode: output {k} is {o.dtype}, expected float32")
        l, width = k % n_levels, (1, 4, 10)[k // n_levels]
        A = (Hd // strides[l]) * (Wd // strides[l]) * na
        if o.dim() == 2:                                   # the unbatched model's (A, width): one frame
            o = o[None]
        if o.dim() != 3 or tuple(o.shape[1:]) != (A, width) or o.shape[0] < 1 or (F is not None and o.shape[0] != F):
            raise ValueError(f"det_decode: output {k} has shape {tuple(o.shape)}, expected (F, {A}, {width}) for level {l} (stride {strides[l]}) of "
                             f"a {Hd}x{Wd} input")
        F = o.shape[0]
        ts.append(o.contiguous())
    return n_levels, strides, na, F, ts


def det_decode(e: Engine, outs, det_size, det_scale, frame_hw, det_thresh=0.5, nms_thresh=0.4, max_num=0, metric="default", max_faces=32,
               want_device=False):
    """SCRFD.forward's decode and detect's sort, NMS and max_num pick (scrfd.py:160-218, :239-303) of F frames in one launch.  outs: the network's
    tensors in its output order (scores per level, bbox per level[, kps per level]), each (F, A_l, 1 | 4 | 10) fp32 on the engine's device ((A_l, .)
    for one frame); det_size = (width, height) of the blob; det_scale: det_geometry's; frame_hw = (Ho, Wo) of the frames (the max_num pick's centre).
    -> (dets, kpss, frame_index): per frame a (n, 5) fp32 array (x1, y1, x2, y2, score) and a (n, 5, 2) fp32 array (None without key points) on the
    host - one small D2H of det / kps / count - and frame_index, the int32 frame number of every face over all frames, in order, the form
    tail.frame_index_of accepts.  Raises ValueError naming the frame for more than _lib.DET_MAX_CAND candidates in a frame, or more than
    max_faces NMS survivors with max_num = 0.  want_device: also the raw device tensors, as a fourth element {"det", "kps", "count"}."""
    n_levels, strides, na, F, ts = _net_outs(e, outs, det_size)
    Wd, Hd = _size2(det_size)
    Ho, Wo = int(frame_hw[0]), int(frame_hw[1])
    if metric not in ("default", "max"):
        raise ValueError(f"det_decode: metric {metric!r} ('default' or 'max')")
    max_num, max_faces = int(max_num), int(max_faces)
    if not 1 <= max_faces <= _lib.DET_MAX_FACES or not 0 <= max_num <= max_faces:
        raise ValueError(f"det_decode: max_faces {max_faces} in [1, {_lib.DET_MAX_FACES}] and max_num {max_num} in [0, max_faces]")
    has_kps = len(ts) == 3 * n_levels
    det = torch.empty((F, max_faces, 5), dtype=torch.float32, device=e.device)
    kps = torch.empty((F, max_faces, 5, 2), dtype=torch.float32, device=e.device) if has_kps else None
    count = torch.empty((F,), dtype=torch.int32, device=e.device)
    ptrs = (C.c_void_p * (3 * n_levels))(*([t.data_ptr() for t in ts] + [None] * (3 * n_levels - len(ts))))
    e._call("cs_det_decode", F, n_levels, (C.c_int * n_levels)(*strides), na, ptrs, Hd, Wd, float(det_scale), float(det_thresh),
            float(nms_thresh), max_num, int(metric == "max"), Ho, Wo, max_faces, det, kps, count)
    cnt = count.cpu().numpy()
    for f, c in enumerate(cnt):
        if c == -1:
            raise ValueError(f"det_decode: frame {f} has more than {_lib.DET_MAX_CAND} candidates above det_thresh = {det_thresh} (raise the threshold)")
        if c == -2:
            raise ValueError(f"det_decode: frame {f} keeps more than max_faces = {max_faces} faces after NMS (raise max_faces or set max_num)")
    d, k = det.cpu().numpy(), kps.cpu().numpy() if has_kps else None
    dets = [d[f, :c].copy() for f, c in enumerate(cnt)]
    kpss = [k[f, :c].copy() for f, c in enumerate(cnt)] if has_kps else None
    frame_index = np.repeat(np.arange(F, dtype=np.int32), cnt)
    if want_device:
        return dets, kpss, frame_index, {"det": det, "kps": kps, "count": count}
    return dets, kpss, frame_index


class FaceDetector:
    """SCRFD.detect (scrfd.py:220-273) and Face_detect_crop.get (face_detect_crop_multi.py:63-100, _single.py:63-82) for F frames, around the caller's
    network: net(blob) takes the (F,3,Hd,Wd) fp32 device blob and returns the model's 6 / 9 (three levels) or 10 / 15 (five levels) output tensors on
    the device, in the model's output order.  det_size = (width, height), det_thresh, nms_thresh: Face_detect_crop.prepare's and SCRFD's."""

    def __init__(self, swapper, net, det_size=(640, 640), det_thresh=0.5, nms_thresh=0.4, max_faces=32, swap_rb=SWAP_RB):
        self.swapper = swapper
        self.e = swapper.engine if hasattr(swapper, "engine") else swapper
        if not callable(net):
            raise ValueError("FaceDetector: net must be callable: blob (F,3,Hd,Wd) -> the detector's output tensors")
        self.net, self.det_size = net, _size2(det_size)
        self.det_thresh, self.nms_thresh, self.max_faces, self.swap_rb = float(det_thresh), float(nms_thresh), int(max_faces), bool(swap_rb)

    def detect(self, frames, max_num=0, metric="default", best=False):
        """frames (F,Ho,Wo,3) u8 -> {"dets": per frame (n,5), "kpss": per frame (n,5,2) or None, "frame_index": int32 per face, "kps": (B,5,2) fp32 all
        faces in order (what chain.crop(frames, kps, frame_index=) takes; None without key points)}.  best=True: per frame only the face with the
        highest score (face_detect_crop_single.py:71-80: argmax of det_score; NMS lists the survivors by descending score, so it is the first)."""
        t = _frames(frames, "FaceDetector.detect").to(self.e.device)
        F, Ho, Wo, _ = t.shape
        _, _, det_scale = det_geometry(Ho, Wo, self.det_size)
        blob = det_input(self.e, t, self.det_size, swap_rb=self.swap_rb)
        outs = self.net(blob)
        dets, kpss, fi = det_decode(self.e, outs, self.det_size, det_scale, (Ho, Wo), det_thresh=self.det_thresh, nms_thresh=self.nms_thresh,
                                    max_num=max_num, metric=metric, max_faces=self.max_faces)
        if best:
            pick = [int(np.argmax(d[:, 4])) if len(d) else None for d in dets]
            dets = [d[p:p + 1] if p is not None else d for d, p in zip(dets, pick)]
            if kpss is not None:
                kpss = [k[p:p + 1] if p is not None else k for k, p in zip(kpss, pick)]
            fi = np.repeat(np.arange(F, dtype=np.int32), [len(d) for d in dets])
        kps = np.concatenate(kpss, axis=0) if kpss is not None else None
        return {"dets": dets, "kpss": kpss, "frame_index": fi, "kps": kps}

    def get(self, frames, crop_size, max_num=0, mode="None", best=False, out=None):
        """Face_detect_crop.get for F frames: detect, estimate_norm per face (align.estimate_norm), cv2.warpAffine(frame, M, (crop_size, crop_size),
        borderValue=0) of every face in one launch (tail.crop_faces_M) -> {"crops": (B,crop_size,crop_size,3) u8 on the device, "M": (B,2,3) float64,
        "frame_index", "dets", "kpss", "kps"}, or None when no frame holds a face (the reference returns None per image)."""
        from . import tail
        res = self.detect(frames, max_num=max_num, metric="default", best=best)      # get always detects with metric="default" (_multi.py:64-67)
        if res["kps"] is None:
            raise ValueError("FaceDetector.get: the detector returns no key points (a 6- or 10-output model); alignment needs them")
        if len(res["frame_index"]) == 0:
            return None
        M, _ = align.norm_matrices(res["kps"], crop_size, mode)
        crops = tail.crop_faces_M(self.e, frames, M, res["frame_index"], crop_size, out=out)["crops"]
        res.update(crops=crops, M=M)
        return res

