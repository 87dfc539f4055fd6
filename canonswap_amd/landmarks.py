"""Landmark tracking on the device: the cropper's per-frame loop without the host.

The reference gets the landmarks of a video from ``Cropper.crop_source_video`` (src/utils/cropper.py:167-222): serial over the frames, frame k
cropped around the landmarks of frame k - 1 (cropper.py:186-193), each step ``LandmarkRunner.run`` (src/utils/human_landmark_runner.py:60-85).
The landmark network is an ONNX file and stays the caller's, as the detector's does: one call between two of ours.

* ``layout_of``        which points span the eye-lip axis for N landmarks (crop.EYE_LIP_POINTS and the 68 / 9 / 5 rules) as cs_lmk_layout
* ``lmk_input``        human_landmark_runner.py:62 + :76 of B faces in F frames, one launch (cs_lmk_input): landmarks on the device -> matrices,
                       crop, the network's input, a status per face
* ``lmk_decode``       human_landmark_runner.py:82-83 (cs_lmk_decode): the network's points -> landmarks in the frame
* ``LandmarkTracker``  LandmarkRunner.run, the loop of cropper.py:186-193 for S trajectories enqueued without a host wait, and the pre-pass
                       over a host video that hands ``VideoSwapper.run`` its ``lmk``
* ``Landmark106``      the seed of a trajectory: insightface's 106-point model on a detected box (model_zoo/landmark.py:80-105)

Both kernels live in csrc/landmarks.hip; there is no torch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, crop as crop_geometry, tail, video
from .engine import Engine, u8_images

RUNNER_DSIZE, RUNNER_SCALE, RUNNER_VY_RATIO = 224, 1.5, -0.1      # crop_image's defaults, which human_landmark_runner.py:62 leaves as they are


def layout_of(n) -> _lib.LmkLayout:
    """cs_lmk_layout for n landmarks: crop.parse_pt2's dispatch (crop.py:216-241) with use_lip=True.  Exact counts first; any other n above 101 is
    read as its first 101 points."""
    n = int(n)
    if n in crop_geometry.EYE_LIP_POINTS:
        left, right, lips = crop_geometry.EYE_LIP_POINTS[n]
    elif n == 68:
        left, right, lips = crop_geometry._PT68_LEFT_EYE, crop_geometry._PT68_RIGHT_EYE, crop_geometry._PT68_LIPS
    elif n == 5:                                            # eyes, nose, lip corners
        left, right, lips = (0,), (1,), (3, 4)
    elif n > 101:
        left, right, lips = crop_geometry.EYE_LIP_POINTS[101]
    elif n == 9:                                            # right eye (2), left eye (2), nose tip, lip corners (2), upper lip, lower lip
        left, right, lips = (2, 3), (0, 1), (5, 6)
    else:
        raise ValueError(f"no landmark layout with {n} points (101, 106, 203, 68, 9, 5, or more than 101)")
    pad = lambda idx: (C.c_int * 4)(*(tuple(idx) + (0,) * (4 - len(idx))))
    return _lib.LmkLayout(len(left), pad(left), pad(right), (C.c_int * 2)(*lips))


def _engine_of(swapper) -> Engine:
    return swapper.engine if hasattr(swapper, "engine") else swapper


def _frames(e, frames, who):
    t = torch.as_tensor(frames)
    return u8_images(t[None] if t.dim() == 3 else t, True, 1, "frames", who).to(e.device).contiguous()


def _dsize(dsize, who):
    if int(dsize) != dsize or not 4 <= int(dsize) <= 16384 or int(dsize) % 4:
        raise ValueError(f"{who}: dsize {dsize!r} (a multiple of 4 from 4 to 16384)")
    return int(dsize)


def lmk_input(e: Engine, frames, lmk, frame_index=None, dsize=RUNNER_DSIZE, scale=RUNNER_SCALE, vy_ratio=RUNNER_VY_RATIO, flag_do_rot=True, out=None,
              want_crops=False, status_mark=1):
    """human_landmark_runner.py:62 + :76 for B faces in F frames, one launch: frames (F,Ho,Wo,3) u8; lmk (B,N,2) fp32 landmarks in frame coordinates,
    on the device as they are (host landmarks are uploaded); frame_index: B host ints in [0, F), any order (None: face b in frame b)
    -> {"inp": (B,3,dsize,dsize) fp32 = crop / 255, "M": (B,18) fp32 = M_o2c | M_c2o, "status": (B,) int32[, "crops": (B,dsize,dsize,3) u8]}, all on the
    device.  A face the guard refuses (a landmark not finite, an empty box, a matrix entry above 1e6) gets status_mark in status, zeros elsewhere, and
    stays refused: hand the same status on through out=.  out: a dict with any of "inp", "M", "status", "crops" as the caller's buffers; a status
    given here is read (sticky), one made here starts at zero."""
    e = _engine_of(e)
    fr = _frames(e, frames, "lmk_input")
    F, Ho, Wo, _ = fr.shape
    pts = torch.as_tensor(lmk)
    if pts.dim() == 2:
        pts = pts[None]
    if pts.dim() != 3 or pts.shape[2] != 2 or pts.shape[0] < 1 or not pts.dtype.is_floating_point:
        raise ValueError(f"lmk_input: expected landmarks (B,N,2) floating point, got {tuple(pts.shape)} {pts.dtype}")
    pts = pts.to(e.device, torch.float32).contiguous()
    B, N = int(pts.shape[0]), int(pts.shape[1])
    layout = layout_of(N)
    dsize = _dsize(dsize, "lmk_input")
    if frame_index is None:
        if B != F:
            raise ValueError(f"lmk_input: {B} landmark sets for {F} frames and no frame_index")
        idx = np.arange(B, dtype=np.int32)
    else:
        idx = np.ascontiguousarray(np.asarray(frame_index), dtype=np.int32)
        if idx.shape != (B,) or np.asarray(frame_index).dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= F:
            raise ValueError(f"lmk_input: frame_index must be {B} integers in [0, {F})")
    status_mark = int(status_mark)
    if status_mark == 0:
        raise ValueError("lmk_input: status_mark must not be 0")
    out = dict(out or {})
    unknown = set(out) - {"inp", "M", "status", "crops"}
    if unknown:
        raise ValueError(f"lmk_input: out has no buffer named {sorted(unknown)}")
    inp = e._out(out.get("inp"), (B, 3, dsize, dsize), torch.float32)
    M = e._out(out.get("M"), (B, 18), torch.float32)
    status = e._out(out["status"], (B,), torch.int32) if out.get("status") is not None else torch.zeros((B,), dtype=torch.int32, device=e.device)
    crops = e._out(out.get("crops"), (B, dsize, dsize, 3), torch.uint8) if (want_crops or out.get("crops") is not None) else None
    e._call("cs_lmk_input", B, F, fr, Ho, Wo, idx.ctypes.data_as(C.POINTER(C.c_int)), pts, N, layout, dsize, float(scale), float(vy_ratio),
            int(bool(flag_do_rot)), status_mark, M, inp, crops, status)
    res = {"inp": inp, "M": M, "status": status}
    if crops is not None:
        res["crops"] = crops
    return res


def lmk_decode(e: Engine, out_pts, M, dsize=RUNNER_DSIZE, status=None, out=None):
    """human_landmark_runner.py:82-83 for B faces: out_pts (B, 2 Np) or (B,Np,2) fp32 on the device, the network's third output; M (B,18) fp32,
    lmk_input's -> lmk (B,Np,2) fp32 on the device, frame coordinates: (out_pts * dsize) under M_c2o, in fp32.  status: lmk_input's; a face with a
    non-zero entry keeps what `out` holds for it (None: every face is decoded).  out: the caller's (B,Np,2) buffer - it may be the tensor the next
    lmk_input reads - a new one starts as zeros."""
    e = _engine_of(e)
    if not isinstance(out_pts, torch.Tensor) or out_pts.device != e.device or out_pts.dtype != torch.float32:
        raise ValueError(f"lmk_decode: out_pts must be a float32 tensor on {e.device}")
    B = int(out_pts.shape[0]) if out_pts.dim() in (2, 3) else 0
    flat = out_pts.reshape(B, -1).contiguous() if B else out_pts
    if B < 1 or flat.shape[1] < 2 or flat.shape[1] % 2 or (out_pts.dim() == 3 and out_pts.shape[2] != 2):
        raise ValueError(f"lmk_decode: out_pts must be (B, 2 Np) or (B, Np, 2), got {tuple(out_pts.shape)}")
    Np = flat.shape[1] // 2
    M = e._out(M, (B, 18), torch.float32)
    dsize = _dsize(dsize, "lmk_decode")
    status = e._out(status, (B,), torch.int32) if status is not None else torch.zeros((B,), dtype=torch.int32, device=e.device)
    lmk = e._out(out, (B, Np, 2), torch.float32) if out is not None else torch.zeros((B, Np, 2), dtype=torch.float32, device=e.device)
    if lmk.data_ptr() == flat.data_ptr():
        raise ValueError("lmk_decode: out_pts and out must not be the same buffer")
    e._call("cs_lmk_decode", B, flat, Np, M, dsize, status, lmk)
    return lmk


def plan_track_batches(n_frames, batch):
    """The batches of the pre-pass: video.plan_batches' (f0, f1) for one face per frame slot, `batch` frames at a time."""
    return [(f0, f1) for f0, f1, _, _ in video.plan_batches(n_frames, None, batch=batch, max_faces=batch)]


class LandmarkTracker:
    """LandmarkRunner.run (human_landmark_runner.py:60-85) and the cropper's loop over a video (cropper.py:186-193) around the caller's network:
    net(inp) takes the (B,3,dsize,dsize) fp32 device tensor and returns the points tensor (B, 2 Np) on the device - output [2] of the reference's
    ONNX model, (B, 406) for its 203 points."""

    def __init__(self, swapper, net, dsize=RUNNER_DSIZE):
        self.swapper, self.e = swapper, _engine_of(swapper)
        if not callable(net):
            raise ValueError("LandmarkTracker: net must be callable: inp (B,3,dsize,dsize) -> the points (B, 2 Np)")
        self.net, self.dsize = net, _dsize(dsize, "LandmarkTracker")

    def _points(self, inp):
        pts = self.net(inp)
        if not isinstance(pts, torch.Tensor) or pts.device != self.e.device or pts.dtype != torch.float32 or pts.shape[0] != inp.shape[0]:
            raise ValueError(f"LandmarkTracker: net must return a float32 tensor ({inp.shape[0]}, 2 Np) on {self.e.device}")
        return pts

    def run(self, frames, lmk, frame_index=None, status=None, out=None, status_mark=1):
        """LandmarkRunner.run for B faces: frames (F,Ho,Wo,3) u8, lmk (B,n,2) landmarks of the faces in their frames -> {"lmk": (B,Np,2) fp32 on the
        device, the network's landmarks in the frame, "status": (B,) int32, "M": (B,18)}.  status / out: see lmk_input / lmk_decode."""
        step = lmk_input(self.e, frames, lmk, frame_index, dsize=self.dsize, out={"status": status}, status_mark=status_mark)
        new = lmk_decode(self.e, self._points(step["inp"]), step["M"], self.dsize, status=step["status"], out=out)
        return {"lmk": new, "status": step["status"], "M": step["M"]}

    def track(self, frames, lmk_prev, status=None):
        """The loop of cropper.py:186-193 for S trajectories: frames (N,Ho,Wo,3) u8 on the device, lmk_prev (S,n,2) host or device, the landmarks of
        the frame before frames[0] (the seed for the first batch) -> (lmk (N,S,Np,2) fp32, status (S,) int32), both on the device:
        lmk[k] = run(frames[k], lmk[k - 1]), lmk[-1] = lmk_prev.  The N steps are enqueued on the current stream without a host wait (device
        inputs given).  status: a trajectory the guard refuses at step k gets k + 1 and is frozen - its later landmarks repeat the last good ones
        (zeros where it froze at step 0 of a seed with another layout than the network's); pass the previous batch's status to continue it."""
        e = self.e
        fr = _frames(e, frames, "LandmarkTracker.track")
        N = int(fr.shape[0])
        prev = torch.as_tensor(lmk_prev)
        if prev.dim() != 3 or prev.shape[2] != 2 or prev.shape[0] < 1:
            raise ValueError(f"LandmarkTracker.track: lmk_prev must be (S,n,2), got {tuple(prev.shape)}")
        prev = prev.to(e.device, torch.float32).contiguous()
        S = int(prev.shape[0])
        status = e._out(status, (S,), torch.int32) if status is not None else torch.zeros((S,), dtype=torch.int32, device=e.device)
        buf = {"inp": torch.empty((S, 3, self.dsize, self.dsize), dtype=torch.float32, device=e.device),
               "M": torch.empty((S, 18), dtype=torch.float32, device=e.device), "status": status}
        out = None
        for k in range(N):
            step = lmk_input(e, fr, prev, [k] * S, dsize=self.dsize, out=buf, status_mark=k + 1)
            pts = self._points(step["inp"])
            if out is None:                                  # the network says how many points it tracks
                Np = pts.reshape(S, -1).shape[1] // 2
                out = torch.zeros((N, S, Np, 2), dtype=torch.float32, device=e.device)
            if tuple(prev.shape) == tuple(out[k].shape):
                out[k].copy_(prev)                           # what a frozen trajectory keeps
            lmk_decode(e, pts, step["M"], self.dsize, status=status, out=out[k])
            prev = out[k]
        return out, status

    def _device_batches(self, frames_host, plan):
        """The plan's batches as device frames, batch i + 1 uploaded (video.HostFrames, its own stream) while batch i is tracked: yields
        (i, frames on the device, done) - call done() once the batch's work is enqueued."""
        src = video._Source(frames_host, "LandmarkTracker.track_video")
        if src.n == 0:
            return
        hf = video.HostFrames(self.e.device, max(f1 - f0 for f0, f1 in plan))
        hf.reserve(*src.hw)
        cur = torch.cuda.current_stream(self.e.device)
        up = hf.upload(src, plan[0][0], plan[0][1], 0)
        for i, (f0, f1) in enumerate(plan):
            s, dev = i & 1, up
            cur.wait_event(hf.copied[s])
            if i + 1 < len(plan):
                up = hf.upload(src, plan[i + 1][0], plan[i + 1][1], s ^ 1)
            yield i, dev, (lambda s=s: hf.consumed[s].record(cur))

    def track_video(self, frames_host, lmk0, batch=None):
        """The pre-pass the reference runs before its swap loop (cropper.py:167-222): frames_host (N,Ho,Wo,3) u8 on the host (what VideoSwapper
        takes), lmk0 (S,n,2) the seed landmarks of frame 0's faces (frame 0 is run from them too, cropper.py:185-186)
        -> (N,S,Np,2) float32 on the host: for one face, lmk[:, 0] is the `lmk` VideoSwapper.run takes.  Batches of video.plan_batches go through
        video.HostFrames; `track` runs per batch, continued on the device from the previous batch's last landmarks and status; one download of
        landmarks and status per batch.  A trajectory the guard froze raises ValueError naming its first frozen frame."""
        batch = int(batch) if batch is not None else 64
        n = len(frames_host)
        plan = plan_track_batches(n, batch)
        prev, status, parts = lmk0, None, []
        for i, dev, done in self._device_batches(frames_host, plan):
            f0, f1 = plan[i]
            lmk, status = self.track(dev, prev, status)
            done()
            host, st = lmk.cpu().numpy(), status.cpu().numpy()
            if st.any():
                t = int(np.argmax(st != 0))
                raise ValueError(f"track_video: trajectory {t} froze at frame {f0 + int(st[t]) - 1}: the guard refused its landmarks "
                                 "(not finite, an empty box, or a crop matrix above 1e6)")
            parts.append(host)
            prev = lmk[-1]
        if not parts:
            raise ValueError("track_video: no frames")
        return np.concatenate(parts, axis=0)


class Landmark106:
    """The seed of a trajectory: insightface's Landmark.get (src/utils/dependencies/insightface/model_zoo/landmark.py:80-105) for B detected
    boxes, around the caller's network: net(blob (B,3,size,size) fp32 on the device) -> (B, 2 * 106) (or (B, 3 * 68) for the 3-d models: x, y are
    kept).  mean / std: the model's input_mean / input_std, which the reference reads off the ONNX graph (landmark.py:30-47: 0.0 / 1.0 where the graph
    normalises itself, else 127.5 / 128.0); explicit here.  Runs once per trajectory: the box -> matrix is host float64, the crop is
    tail.crop_faces_M, the rest torch lines on the device.
    PARITY UNPINNED: the matrix is face_align.transform at rotation 0 written out, [[s, 0, size/2 - cx s], [0, s, size/2 - cy s]] with
    s = size / (1.5 max(w, h)); no skimage SimilarityTransform output at hand to hold it to."""

    def __init__(self, swapper, net, input_size=192, mean=0.0, std=1.0, lmk_dim=2, lmk_num=106):
        self.swapper, self.e = swapper, _engine_of(swapper)
        if not callable(net):
            raise ValueError("Landmark106: net must be callable: blob (B,3,size,size) -> the points")
        self.net, self.size = net, _dsize(input_size, "Landmark106")
        self.mean, self.std, self.lmk_dim, self.lmk_num = float(mean), float(std), int(lmk_dim), int(lmk_num)

    def matrices(self, bbox):
        """landmark.py:82-87: boxes (B,4) x1, y1, x2, y2 -> M (B,2,3) float64, frame -> crop."""
        b = np.asarray(bbox, dtype=np.float64).reshape(-1, 4)
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cx, cy = (b[:, 2] + b[:, 0]) / 2, (b[:, 3] + b[:, 1]) / 2
        s = self.size / (np.maximum(w, h) * 1.5)
        M = np.zeros((b.shape[0], 2, 3), dtype=np.float64)
        M[:, 0, 0] = M[:, 1, 1] = s
        M[:, 0, 2], M[:, 1, 2] = self.size / 2 - cx * s, self.size / 2 - cy * s
        return M

    def get(self, frames, bbox, frame_index=None):
        """frames (F,Ho,Wo,3) u8, bbox (B,4) the detector's boxes (host), frame_index B host ints (non-decreasing; None: box b in frame b)
        -> {"lmk": (B,106,2) fp32 on the device, frame coordinates - a seed for LandmarkTracker, "crops": (B,size,size,3) u8, "M": (B,2,3)}."""
        M = self.matrices(bbox)
        B = M.shape[0]
        idx = np.arange(B, dtype=np.int32) if frame_index is None else frame_index
        crops = tail.crop_faces_M(self.e, frames, M, idx, self.size)["crops"]
        # cv2.dnn.blobFromImage(aimg, 1 / std, size, (mean, mean, mean), swapRB=True) (landmark.py:91)
        blob = (crops.permute(0, 3, 1, 2).flip(1).to(torch.float32) - self.mean) * np.float32(1.0 / self.std)
        pred = self.net(blob.contiguous())
        if not isinstance(pred, torch.Tensor) or pred.device != self.e.device or pred.shape[0] != B:
            raise ValueError(f"Landmark106: net must return a tensor ({B}, points) on {self.e.device}")
        pred = pred.to(torch.float32).reshape(B, -1, self.lmk_dim)
        if self.lmk_num < pred.shape[1]:
            pred = pred[:, -self.lmk_num:, :]                                    # landmark.py:96-97
        half = float(self.size // 2)
        xy = (pred[:, :, :2] + 1.0) * half                                       # landmark.py:98-100
        IM = np.stack([np.linalg.inv(np.vstack([m, [0, 0, 1]]))[:2] for m in M]).astype(np.float32)      # cv2.invertAffineTransform (:102)
        IMt = torch.from_numpy(IM).to(self.e.device)
        lmk = (xy[:, :, 0:1] * IMt[:, None, :, 0] + xy[:, :, 1:2] * IMt[:, None, :, 1]) + IMt[:, None, :, 2]      # trans_points2d (:103)
        return {"lmk": lmk.contiguous(), "crops": crops, "M": M}
