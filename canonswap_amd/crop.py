"""The cropper's geometry on the host: tracked landmarks -> the similarity transform of the crop (src/utils/crop.py:98-300, 381-455 as
src/utils/cropper.py:196-204 and human_landmark_runner.py:62 call it).  The image step that goes with it, cv2.warpAffine of the frame,
is cs_crop_frames on the device (tail.crop_frames).

A restatement of the reference's landmark -> matrix path that keeps its dtypes and its order of operations, so that the matrices
come out as the reference's do (tests/golden/crop_geometry.npz holds the reference's own results, tools/make_golden_crop.py):

* every constant array is float32 (`DTYPE = np.float32`, crop.py:15);
* the angle, its sine and cosine are Python floats from `math` (crop.py:272, 406) and are rounded when the 2x3 matrix is built as float32;
* M_c2o is np.linalg.inv of the float32 3x3 matrix (crop.py:445-446).

A quirk that is mirrored, not mended: crop_image (crop.py:429-440) never forwards `vx_ratio`, so the offset along the eye axis is always
0 whatever CropConfig.vx_ratio says (cropper.py:201 passes it, crop_image drops it).  There is no vx_ratio parameter here.
"""
from __future__ import annotations

from math import acos, cos, sin

import numpy as np

DTYPE = np.float32      # crop.py:15

# landmark layouts with four points around each eye and two lip corners (crop.py:103-109, 120-126, 137-142):
# number of points -> (left eye, right eye, lip corners)
EYE_LIP_POINTS = {
    101: ((39, 42, 45, 48), (51, 54, 57, 60), (75, 81)),
    106: ((33, 35, 40, 39), (87, 89, 94, 93), (52, 61)),
    203: ((0, 6, 12, 18), (24, 30, 36, 42), (48, 66)),
}
# 68 points (crop.py:153-171): eye corners, lip corners (the reference's 1-based list minus one)
_PT68_LEFT_EYE, _PT68_RIGHT_EYE, _PT68_LIPS = (36, 39), (42, 45), (48, 54)


def _pt2_eye_lip(pts, layout, use_lip):
    left, right, lips = layout
    eye_l = np.mean(pts[list(left)], axis=0)
    eye_r = np.mean(pts[list(right)], axis=0)
    if not use_lip:
        return np.stack([eye_l, eye_r], axis=0)
    return np.stack([(eye_l + eye_r) / 2, (pts[lips[0]] + pts[lips[1]]) / 2], axis=0)


def parse_pt2(pts, use_lip=True):
    """parse_pt2_from_pt_x (crop.py:216-241) with the per-layout parsers it dispatches to (crop.py:98-214): landmarks (N,2) -> two points,
    the centre of the eyes and the centre of the lips.  N in 101, 106, 68, 5, 203, 9; any other N above 101 is read as its first 101
    points.  use_lip=False: the two eyes, the second point then turned a quarter clockwise about the first, so that the pair spans the
    same axis as (eyes, lips) would."""
    n = pts.shape[0]
    if n in EYE_LIP_POINTS:                                # (exact counts first: 106 and 203 are not "more than 101")
        pt2 = _pt2_eye_lip(pts, EYE_LIP_POINTS[n], use_lip)
    elif n == 68:
        eye_l = np.mean(pts[list(_PT68_LEFT_EYE), :], 0)
        eye_r = np.mean(pts[list(_PT68_RIGHT_EYE), :], 0)
        if use_lip:
            pt2 = np.stack([(eye_l + eye_r) / 2, (pts[_PT68_LIPS[0], :] + pts[_PT68_LIPS[1], :]) / 2], axis=0)
        else:
            pt2 = np.stack([eye_l, eye_r], axis=0)
    elif n == 5:                                           # eyes, nose, lip corners
        pt2 = np.stack([(pts[0] + pts[1]) / 2, (pts[3] + pts[4]) / 2] if use_lip else [pts[0], pts[1]], axis=0)
    elif n > 101:
        pt2 = _pt2_eye_lip(pts[:101], EYE_LIP_POINTS[101], use_lip)
    elif n == 9:                                           # right eye (2), left eye (2), nose tip, lip corners (2), upper lip, lower lip
        eye_l, eye_r = (pts[2] + pts[3]) / 2, (pts[0] + pts[1]) / 2
        pt2 = np.stack([(eye_l + eye_r) / 2, (pts[5] + pts[6]) / 2] if use_lip else [eye_l, eye_r], axis=0)
    else:
        raise ValueError(f"no landmark layout with {n} points (101, 106, 203, 68, 9, 5, or more than 101)")
    if not use_lip:
        v = pt2[1] - pt2[0]
        pt2[1, 0] = pt2[0, 0] - v[1]
        pt2[1, 1] = pt2[0, 1] + v[0]
    return pt2


def parse_rect(pts, scale=1.5, vy_ratio=0, use_lip=True):
    """parse_rect_from_landmark (crop.py:244-300) with need_square=True, vx_ratio=0 and the angle in radians, as
    _estimate_similar_transform_from_pts calls it: landmarks (N,2) -> centre (2,), size (2,) (a square: both equal), angle (Python float)
    of the box that holds the landmarks, upright along the eye-lip axis, enlarged by `scale` and moved by vy_ratio * size along that axis."""
    pt2 = parse_pt2(pts, use_lip=use_lip)
    uy = pt2[1] - pt2[0]
    length = np.linalg.norm(uy)
    if length <= 1e-3:                                     # eyes and lips coincide: no axis to read, the image's own
        uy = np.array([0, 1], dtype=DTYPE)
    else:
        uy /= length
    ux = np.array((uy[1], -uy[0]), dtype=DTYPE)
    angle = acos(ux[0])                                    # of the x axis; clockwise positive in image coordinates
    if ux[1] < 0:
        angle = -angle
    R = np.array([ux, uy])
    centre0 = np.mean(pts, axis=0)
    turned = (pts - centre0) @ R.T
    lo = np.min(turned, axis=0)
    hi = np.max(turned, axis=0)
    centre1 = (lo + hi) / 2
    size = hi - lo
    side = max(size[0], size[1])
    size[0] = side
    size[1] = side
    size *= scale
    centre = centre0 + ux * centre1[0] + uy * centre1[1]
    centre = centre + ux * (0 * size) + uy * (vy_ratio * size)      # vx_ratio = 0: see the module's docstring
    return centre, size, angle


def estimate_similar_transform(pts, dsize, scale=1.5, vy_ratio=-0.1, flag_do_rot=True):
    """_estimate_similar_transform_from_pts (crop.py:381-426) -> M_INV, the 2x3 float32 matrix original image -> crop."""
    centre, size, angle = parse_rect(pts, scale=scale, vy_ratio=vy_ratio)
    s = dsize / size[0]
    target = np.array([dsize / 2, dsize / 2], dtype=DTYPE)
    if flag_do_rot:
        c, sn = cos(angle), sin(angle)
        cx, cy = centre[0], centre[1]
        tx, ty = target[0], target[1]
        return np.array([[s * c, s * sn, tx - s * (c * cx + sn * cy)],
                         [-s * sn, s * c, ty - s * (-sn * cx + c * cy)]], dtype=DTYPE)
    return np.array([[s, 0, target[0] - s * centre[0]],
                     [0, s, target[1] - s * centre[1]]], dtype=DTYPE)


def _transform_one(pts, M):
    return pts @ M[:2, :2].T + M[:2, 2]                   # crop.py:66-72


def transform_pts(pts, M):
    """_transform_pts (crop.py:66-72): points (N,2) under a 2x3 / 3x3 matrix, or (B,N,2) under B matrices (B,2,3) / (B,3,3)."""
    pts, M = np.asarray(pts), np.asarray(M)
    if pts.ndim == 2 and M.ndim == 2 and pts.shape[1] == 2 and M.shape in ((2, 3), (3, 3)):
        return _transform_one(pts, M)
    if pts.ndim == 3 and M.ndim == 3 and pts.shape[2] == 2 and M.shape[0] == pts.shape[0] and M.shape[1:] in ((2, 3), (3, 3)):
        return np.stack([_transform_one(p, m) for p, m in zip(pts, M)])
    raise ValueError(f"transform_pts: points {pts.shape} and matrices {M.shape} do not go together ((N,2) with 2x3 / 3x3, or (B,N,2) with B of them)")


def crop_matrices(lmk, dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True):
    """What crop_image (crop.py:429-455) builds besides the image: landmarks (N,2) or (B,N,2) in the original frame ->
    M_o2c (B,3,3) float32, original -> crop; M_c2o (B,3,3) float32, its np.linalg.inv; lmk_crop (B,N,2), the landmarks in the crop.
    The defaults are CropConfig's (src/config/crop_config.py:21-26); the landmark runner crops with (224, 1.5, -0.1)
    (human_landmark_runner.py:62, the defaults of crop_image).  vx_ratio: never forwarded by crop_image, see the module's docstring."""
    pts = np.asarray(lmk)
    if pts.ndim == 2:
        pts = pts[None]
    if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[0] < 1:
        raise ValueError(f"crop_matrices: expected landmarks (N,2) or (B,N,2), got {np.asarray(lmk).shape}")
    if pts.dtype.kind != "f":
        raise ValueError(f"crop_matrices: landmarks must be floating point (the tracker's are float32), got {pts.dtype}")
    if int(dsize) != dsize or dsize < 1:
        raise ValueError(f"crop_matrices: dsize {dsize!r}")
    dsize, scale, vy_ratio = int(dsize), float(scale), float(vy_ratio)      # Python numbers, as CropConfig holds them: a numpy float64 scalar
    last_row = np.array([0, 0, 1], dtype=DTYPE)                             # would lift the float32 arithmetic below to float64
    M_o2c, M_c2o, lmk_crop = [], [], []
    for p in pts:
        M_INV = estimate_similar_transform(p, dsize, scale=scale, vy_ratio=vy_ratio, flag_do_rot=flag_do_rot)
        lmk_crop.append(_transform_one(p, M_INV))
        M = np.vstack([M_INV, last_row])
        M_o2c.append(M)
        M_c2o.append(np.linalg.inv(M))
    return np.stack(M_o2c), np.stack(M_c2o), np.stack(lmk_crop)
