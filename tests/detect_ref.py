"""Yardstick of the detector tests (test_detect_cpu.py, test_gpu_detect.py; not collected): what the reference executes around the SCRFD
network (src/utils/dependencies/insightface/model_zoo/scrfd.py) and for the identity crops (insightface_func/utils/face_align_ffhqandnewarc.py),
restated in numpy from the description of those lines:

  resize_linear_cv   cv2.resize(img, (w, h)), default INTER_LINEAR, OpenCV's 8-bit arithmetic at a general ratio (scrfd.py:233)
  letterbox_blob     scrfd.py:224-235 + :154: resize, zero letterbox, blobFromImage as a table of the byte
  decode_faces       scrfd.py:160-218 + :239-273 + :275-303: threshold -> distance decode -> sort -> greedy NMS -> max_num
  estimate_norm_ref  face_align_ffhqandnewarc.py:55-78 by an independent derivation: the least-squares similarity as ONE complex number
                     (w = a z + b), which equals Umeyama's solution wherever no reflection is involved

PARITY UNPINNED: resize_linear_cv restates OpenCV's published algorithm (resize.cpp), no cv2 at hand; decode_faces is pinned to the reference's
own code by tests/golden/detect.npz (tools/make_golden_detect.py).  Where the reference's argsort()[::-1] leaves ties open the contract is a
stable argsort reversed, at each of its three places.

It also builds the synthetic network outputs the tests feed: a scene places boxes with five points; every anchor whose centre lies in a box gets
a score falling with its distance from the box centre and the distances of the true box plus seeded jitter, so each face is a cluster of
overlapping candidates that NMS must thin.  Scores are tie-free unless a test says otherwise."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect.npz")
LAYOUTS = {3: ((8, 16, 32), 2), 5: ((8, 16, 32, 64, 128), 1)}      # scrfd.py:114-131
MEAN, STD = 127.5, 128.0                                         # scrfd.py:107-108
F32 = np.float32


# ------------------------------------------------------------------------------------------------ cv2.resize, INTER_LINEAR, 8 bit
def _axis(dst, src):
    """One axis src -> dst: (tap s as cvFloor gives it, coefficient of tap s, coefficient of tap s + 1), before any clamp."""
    scale = 1.0 / (float(dst) / src)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f)
    f = f - s.astype(F32)
    return s.astype(np.int64), f


def _coeffs(f):
    c0 = np.rint((F32(1) - f) * F32(2048)).astype(np.int16).astype(np.int64)      # np.rint: half to even, as cvRound
    c1 = np.rint(f * F32(2048)).astype(np.int16).astype(np.int64)
    return c0, c1


def resize_linear_cv(u8, dst_h, dst_w):
    """(..., h, w, C) uint8 -> (..., dst_h, dst_w, C) uint8.  Columns: a tap beyond either border is pulled in and its fraction zeroed (s < 0:
    s = 0, f = 0; s >= w - 1: s = w - 1, f = 0).  Rows: the row numbers s, s + 1 are clamped, the weights kept (resize.cpp clips the row index where
    it fetches the row).  Horizontal pass into integers, vertical pass (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2, saturated.  Exactly
    one half on both axes: the 2 x 2 mean (OpenCV switches to INTER_AREA there); equal sizes: a copy."""
    a = np.asarray(u8)
    assert a.dtype == np.uint8 and a.ndim >= 3
    h, w = a.shape[-3], a.shape[-2]
    if (h, w) == (dst_h, dst_w):
        return a.copy()
    x = a.astype(np.int64)
    if h == 2 * dst_h and w == 2 * dst_w:
        s = x[..., 0::2, 0::2, :] + x[..., 0::2, 1::2, :] + x[..., 1::2, 0::2, :] + x[..., 1::2, 1::2, :]
        return ((s + 2) >> 2).astype(np.uint8)
    sx, fx = _axis(dst_w, w)
    lo, hi = sx < 0, sx >= w - 1
    fx = np.where(lo | hi, F32(0), fx)
    sx = np.where(lo, 0, np.where(hi, w - 1, sx))
    a0, a1 = _coeffs(fx)
    sx1 = np.minimum(sx + 1, w - 1)                                                 # under a zero coefficient where clamped
    H = x[..., :, sx, :] * a0[:, None] + x[..., :, sx1, :] * a1[:, None]            # (..., h, dst_w, C)
    sy, fy = _axis(dst_h, h)
    b0, b1 = _coeffs(fy)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    H = np.moveaxis(H, -3, 0) >> 4
    shape = (dst_h,) + (1,) * (H.ndim - 1)
    out = (((b0.reshape(shape) * H[y0]) >> 16) + ((b1.reshape(shape) * H[y1]) >> 16) + 2) >> 2
    return np.ascontiguousarray(np.moveaxis(np.clip(out, 0, 255), 0, -3).astype(np.uint8))


def geometry(Ho, Wo, det_size):
    """scrfd.py:224-232: (new_height, new_width, det_scale) with the reference's truncations; det_size = (width, height)."""
    im_ratio = float(Ho) / Wo
    model_ratio = float(det_size[1]) / det_size[0]
    if im_ratio > model_ratio:
        new_height = det_size[1]
        new_width = int(new_height / im_ratio)
    else:
        new_width = det_size[0]
        new_height = int(new_width * im_ratio)
    return new_height, new_width, float(new_height) / Ho


def table(mean=MEAN, std=STD):
    """(3, 256) fp32: blobFromImage's (float(u8) - mean) * (1 / std) per output plane."""
    m = np.array([mean] * 3 if np.ndim(mean) == 0 else mean, dtype=F32)
    v = np.arange(256, dtype=np.uint8).astype(F32)
    return np.ascontiguousarray((v[None, :] - m[:, None]) * F32(1.0 / std))


def letterbox_blob(frames, det_size, swap_rb=True, lut=None):
    """frames (F, Ho, Wo, 3) uint8 -> blob (F, 3, Hd, Wd) fp32: scrfd.py:224-235 then :154."""
    frames = np.asarray(frames)
    F, Ho, Wo, _ = frames.shape
    Wd, Hd = det_size
    nh, nw, _ = geometry(Ho, Wo, det_size)
    det_img = np.zeros((F, Hd, Wd, 3), dtype=np.uint8)
    det_img[:, :nh, :nw, :] = resize_linear_cv(frames, nh, nw)
    lut = table() if lut is None else lut
    src = det_img[..., ::-1] if swap_rb else det_img                                 # output plane c holds source channel 2 - c
    return np.ascontiguousarray(np.stack([lut[c][src[..., c]] for c in range(3)], axis=1))


# ------------------------------------------------------------------------------------------------ the network's outputs -> faces
def levels_of(n_outs):
    n_levels = 3 if n_outs in (6, 9) else 5
    assert n_outs in (6, 9, 10, 15)
    return n_levels, n_outs == 3 * n_levels


def stable_desc(v):
    """argsort()[::-1] under the tie contract: a stable argsort, reversed."""
    return np.argsort(v, kind="stable")[::-1]


def decode_faces(outs, det_size, det_scale, frame_hw, det_thresh=0.5, nms_thresh=0.4, max_num=0, metric="default"):
    """One frame: outs = the network's arrays in its output order, (A_l, 1), (A_l, 4)[, (A_l, 10)] fp32 per level -> (det (n, 5) fp32, kps (n, 5, 2)
    fp32 or None).  Everything float32, one rounding per operation."""
    n_levels, use_kps = levels_of(len(outs))
    strides, na = LAYOUTS[n_levels]
    Wd, Hd = det_size
    thr, scale = F32(det_thresh), F32(det_scale)
    S, B, K = [], [], []
    for l, stride in enumerate(strides):
        height, width = Hd // stride, Wd // stride
        cell = np.arange(height * width * na) // na
        cx = (cell % width).astype(F32) * F32(stride)
        cy = (cell // width).astype(F32) * F32(stride)
        score = np.asarray(outs[l], dtype=F32).reshape(-1)
        bb = np.asarray(outs[n_levels + l], dtype=F32) * F32(stride)
        assert score.shape[0] == cell.shape[0] and bb.shape == (cell.shape[0], 4)
        pos = np.nonzero(score >= thr)[0]                                            # scrfd.py:206
        S.append(score[pos])
        B.append(np.stack([cx - bb[:, 0], cy - bb[:, 1], cx + bb[:, 2], cy + bb[:, 3]], axis=-1)[pos])      # distance2bbox
        if use_kps:
            kp = np.asarray(outs[2 * n_levels + l], dtype=F32) * F32(stride)
            pts = np.stack([(cx if i % 2 == 0 else cy) + kp[:, i] for i in range(10)], axis=-1)             # distance2kps
            K.append(pts[pos].reshape(-1, 5, 2))
    score = np.concatenate(S)
    boxes = np.concatenate(B) / scale                                                # scrfd.py:242: float32 array / Python float
    kpss = np.concatenate(K) / scale if use_kps else None
    assert boxes.dtype == F32 and score.dtype == F32
    order = stable_desc(score)                                                       # :241
    pre = np.concatenate([boxes, score[:, None]], axis=1)[order]
    if use_kps:
        kpss = kpss[order]
    keep = nms(pre, nms_thresh)
    det = pre[keep]
    if use_kps:
        kpss = kpss[keep]
    if max_num > 0 and det.shape[0] > max_num:                                       # :254-272
        area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
        cy0, cx0 = frame_hw[0] // 2, frame_hw[1] // 2
        ox = (det[:, 0] + det[:, 2]) / F32(2) - F32(cx0)
        oy = (det[:, 1] + det[:, 3]) / F32(2) - F32(cy0)
        d2 = ox * ox + oy * oy
        values = area if metric == "max" else area - d2 * F32(2)
        assert values.dtype == F32
        pick = stable_desc(values)[:max_num]
        det = det[pick]
        if use_kps:
            kpss = kpss[pick]
    return np.ascontiguousarray(det), (np.ascontiguousarray(kpss) if use_kps else None)


def nms(dets, thresh):
    """scrfd.py:275-303 as flags over the visiting order: a visited box that is still alive is kept and kills every later box with
    ovr > thresh (not ovr <= thresh)."""
    thr = F32(thresh)
    x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
    areas = (x2 - x1 + F32(1)) * (y2 - y1 + F32(1))
    visit = stable_desc(dets[:, 4])                                                  # :284
    alive = np.ones(len(visit), dtype=bool)
    keep = []
    for p, i in enumerate(visit):
        if not alive[p]:
            continue
        keep.append(int(i))
        rest = visit[p + 1:]
        w = np.maximum(F32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + F32(1))
        h = np.maximum(F32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + F32(1))
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[rest] - inter)
        assert ovr.dtype == F32
        alive[p + 1:] &= ovr <= thr
    return keep


def decode_frames(outs, det_size, det_scale, frame_hw, **kw):
    """outs: arrays (F, A_l, .) -> per-frame lists (dets, kpss or None, frame_index int32)."""
    F = outs[0].shape[0]
    res = [decode_faces([o[f] for o in outs], det_size, det_scale, frame_hw, **kw) for f in range(F)]
    dets = [d for d, _ in res]
    kpss = [k for _, k in res] if res[0][1] is not None else None
    return dets, kpss, np.repeat(np.arange(F, dtype=np.int32), [len(d) for d in dets])


# ------------------------------------------------------------------------------------------------ alignment, independently derived
def similarity_complex(src, dst):
    """Least squares w = a z + b over complex a, b (points as x + iy): a = sum (w - mw) conj(z - mz) / sum |z - mz|^2, b = mw - a mz -> 2 x 3."""
    z = np.asarray(src, np.float64) @ np.array([1, 1j])
    w = np.asarray(dst, np.float64) @ np.array([1, 1j])
    mz, mw = z.mean(), w.mean()
    a = np.sum((w - mw) * np.conj(z - mz)) / np.sum(np.abs(z - mz) ** 2)
    b = mw - a * mz
    return np.array([[a.real, -a.imag, b.real], [a.imag, a.real, b.imag]])


def estimate_norm_ref(kps5, templates):
    """templates (T, 5, 2) as the reference scales them -> (M 2 x 3, index): the template with the smallest summed point distance."""
    kps5 = np.asarray(kps5, np.float64)
    best = None
    for i, t in enumerate(np.asarray(templates, np.float64)):
        M = similarity_complex(kps5, t)
        err = np.sum(np.linalg.norm(kps5 @ M[:, :2].T + M[:, 2] - t, axis=1))
        if best is None or err < best[2]:
            best = (M, i, err)
    return best[0], best[1]


# ------------------------------------------------------------------------------------------------ synthetic network outputs
KPS_REL = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])      # eyes, nose, mouth corners inside a box


def anchors(det_size, n_levels):
    """Per level (stride, centres (A, 2) float64) in the network's anchor order."""
    strides, na = LAYOUTS[n_levels]
    Wd, Hd = det_size
    out = []
    for s in strides:
        h, w = Hd // s, Wd // s
        cell = np.arange(h * w * na) // na
        out.append((s, np.stack([(cell % w) * s, (cell // w) * s], axis=-1).astype(np.float64)))
    return out


def box_kps(box):
    x1, y1, x2, y2 = box
    return np.array([x1, y1]) + KPS_REL * np.array([x2 - x1, y2 - y1])


def synth_outputs(det_size, n_levels, faces, seed, use_kps=True, single=False, background=0.3):
    """One frame's network outputs: faces = [(box (x1, y1, x2, y2) in the det image, base score)].  Every anchor whose centre lies in a box
    (single: only the one nearest the box centre, on the finest level that has one) scores base - 0.2 * distance / half diagonal + jitter and
    predicts the box and its five points plus jitter, in units of the stride; the others score below `background`.  All float32; the candidate
    scores are checked to be tie-free."""
    r = np.random.Generator(np.random.PCG64([5100, det_size[0], det_size[1], n_levels, seed]))
    S, B, K = [], [], []
    taken = set()
    for s, c in anchors(det_size, n_levels):
        A = c.shape[0]
        score = r.uniform(0.0, background, A)
        bb = r.uniform(0.0, 2.0, (A, 4))
        kp = r.uniform(-2.0, 2.0, (A, 10))
        for g, (box, base) in enumerate(faces):
            x1, y1, x2, y2 = box
            mid = np.array([(x1 + x2) / 2, (y1 + y2) / 2])
            inside = (c[:, 0] >= x1) & (c[:, 0] <= x2) & (c[:, 1] >= y1) & (c[:, 1] <= y2)
            dist = np.hypot(*(c - mid).T)
            if single:
                if g in taken or not inside.any():
                    continue
                taken.add(g)
                k = int(np.argmin(np.where(inside, dist, np.inf)))
                inside = np.zeros(A, bool)
                inside[k] = True
            new = base - 0.2 * dist / (np.hypot(x2 - x1, y2 - y1) / 2) + r.uniform(0, 1e-3, A)
            use = inside & (new > score)
            score = np.where(use, new, score)
            true = np.stack([c[:, 0] - x1, c[:, 1] - y1, x2 - c[:, 0], y2 - c[:, 1]], axis=-1) / s
            bb = np.where(use[:, None], true + r.uniform(-0.02, 0.02, (A, 4)), bb)
            pts = (box_kps(box)[None] - c[:, None, :]).reshape(A, 10) / s
            kp = np.where(use[:, None], pts + r.uniform(-0.02, 0.02, (A, 10)), kp)
        S.append(score.astype(F32).reshape(A, 1))
        B.append(bb.astype(F32))
        K.append(kp.astype(F32))
    seen = set()                                                                     # tie-free: a repeated candidate score moves up by single ulps
    for x in S:
        for k in np.nonzero(x[:, 0] >= F32(0.5))[0]:
            v = x[k, 0]
            while float(v) in seen:
                v = np.nextafter(v, F32(2))
            x[k, 0] = v
            seen.add(float(v))
    cand = np.concatenate([x[x >= F32(0.5)] for x in S])
    assert len(np.unique(cand)) == len(cand), "the scene's candidate scores tie"
    return S + B + (K if use_kps else [])


def stack_frames(per_frame):
    """[[arrays of frame 0], [arrays of frame 1], ...] -> arrays (F, A_l, .)."""
    return [np.ascontiguousarray(np.stack(x)) for x in zip(*per_frame)]


# the scenes, in det-image coordinates of a 64 x 64 input fed by 100 x 100 frames (det_scale 0.64, image centre (50, 50) = det (32, 32))
FRAME_64 = (100, 100)
TWO = [((6, 6, 30, 30), 0.9), ((34, 30, 58, 54), 0.8)]
OVERLAP = [((8, 8, 36, 36), 0.9), ((14, 12, 42, 40), 0.8)]                              # IoU about 0.5: the weaker one goes
CHAIN = [((4, 20, 28, 44), 0.95), ((13, 20, 37, 44), 0.85), ((22, 20, 46, 44), 0.75)]   # A-B and B-C above 0.4, A-C below: A and C stay
# the highest score, the largest area and the most central box are three different faces
PICK3 = [((44, 6, 58, 20), 0.95), ((2, 2, 28, 28), 0.85), ((26, 26, 38, 38), 0.75)]
FIVE = [((10, 10, 60, 70), 0.9), ((70, 60, 120, 118), 0.8)]                             # at 128 x 128, five levels


def scene_64(faces, seed, **kw):
    return synth_outputs((64, 64), 3, faces, seed, **kw)


def det_scale_64():
    return geometry(FRAME_64[0], FRAME_64[1], (64, 64))[2]


# what tools/make_golden_detect.py records with the reference's own detect(): name -> (det_size, frame_hw, levels, faces, seed, use_kps, max_num, metric)
GOLDEN_SCENES = {
    "two": ((64, 64), FRAME_64, 3, TWO, 1, True, 0, "default"),
    "overlap": ((64, 64), FRAME_64, 3, OVERLAP, 2, True, 0, "default"),
    "chain": ((64, 64), FRAME_64, 3, CHAIN, 3, True, 0, "default"),
    "empty": ((64, 64), FRAME_64, 3, [], 4, True, 0, "default"),
    "nokps": ((64, 64), FRAME_64, 3, TWO, 5, False, 0, "default"),
    "pick1": ((64, 64), FRAME_64, 3, PICK3, 6, True, 1, "default"),
    "pick1max": ((64, 64), FRAME_64, 3, PICK3, 6, True, 1, "max"),
    "pick2": ((64, 64), FRAME_64, 3, PICK3, 6, True, 2, "default"),
    "pick2max": ((64, 64), FRAME_64, 3, PICK3, 6, True, 2, "max"),
    "pick0": ((64, 64), FRAME_64, 3, PICK3, 6, True, 0, "default"),
    "five": ((128, 128), (150, 200), 5, FIVE, 7, True, 0, "default"),
    "five1": ((128, 128), (150, 200), 5, FIVE, 7, True, 1, "max"),
    "landscape": ((64, 64), (90, 160), 3, TWO, 8, True, 0, "default"),
}


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """The scene's inputs and the restatement's answer, computed once and shared (read-only arrays)."""
    det_size, frame_hw, levels, faces, seed, use_kps, max_num, metric = GOLDEN_SCENES[name]
    outs = synth_outputs(det_size, levels, faces, seed, use_kps=use_kps)
    det_scale = geometry(frame_hw[0], frame_hw[1], det_size)[2]
    det, kps = decode_faces(outs, det_size, det_scale, frame_hw, max_num=max_num, metric=metric)
    for a in outs + [det] + ([kps] if kps is not None else []):
        a.setflags(write=False)
    return dict(outs=outs, det_size=det_size, det_scale=det_scale, frame_hw=frame_hw, max_num=max_num, metric=metric, det=det, kps=kps)


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def frames_u8(F, Ho, Wo, seed):
    """F seeded frames that hold every byte value and both extremes next to each other."""
    r = np.random.Generator(np.random.PCG64([5200, F, Ho, Wo, seed]))
    x = r.integers(0, 256, size=(F, Ho, Wo, 3)).astype(np.uint8)
    flat = x.reshape(F, -1)
    flat[:, 0::7] = 255
    flat[:, 1::7] = 0
    return x
