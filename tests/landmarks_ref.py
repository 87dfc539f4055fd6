"""LandmarkRunner.run (src/utils/human_landmark_runner.py:60-85) restated in numpy on top of canonswap_amd.crop.crop_matrices, and a float64
evaluation of the same formulas: the yardsticks of tests/test_landmarks_cpu.py and tests/test_gpu_landmarks.py.

* ``matrices64``   the landmark -> matrix path of crop.py (parse_pt2 -> parse_rect -> estimate_similar_transform -> inverse) with every value a
                   float64: what the formulas give on the landmarks as they are, to which both the reference's float32 route and the device's
                   are held (err below)
* ``err``          the largest distance in pixels between X p and F p over a set of points p
* ``decode`` / ``decode64``   human_landmark_runner.py:82-83 in float32 (numpy, operation by operation) and in float64
* ``standin_net``  a deterministic torch-only stand-in for the landmark network; ``synthetic_face``, ``shape203``, ``loop_shape``: its shapes
"""
from math import acos, cos, sin

import numpy as np

from canonswap_amd import crop


def matrices64(pts, dsize, scale, vy_ratio, flag_do_rot):
    """(M_o2c, M_c2o) 3 x 3 float64 for landmarks (N,2): crop.py's formulas, nothing rounded below double."""
    pts = np.asarray(pts, dtype=np.float64)
    pt2 = crop.parse_pt2(pts, use_lip=True).astype(np.float64)      # means and midpoints of float64 points: float64
    uy = pt2[1] - pt2[0]
    length = np.linalg.norm(uy)
    uy = np.array([0.0, 1.0]) if length <= 1e-3 else uy / length
    ux = np.array([uy[1], -uy[0]])
    angle = acos(min(1.0, max(-1.0, ux[0])))
    if ux[1] < 0:
        angle = -angle
    c0 = pts.mean(axis=0)
    turned = (pts - c0) @ np.array([ux, uy]).T
    lo, hi = turned.min(axis=0), turned.max(axis=0)
    c1 = (lo + hi) / 2
    size = max(hi - lo) * float(scale)
    centre = c0 + ux * c1[0] + uy * c1[1] + uy * (float(vy_ratio) * size)
    s = dsize / size
    t = dsize / 2
    if flag_do_rot:
        c, sn = cos(angle), sin(angle)
        M = np.array([[s * c, s * sn, t - s * (c * centre[0] + sn * centre[1])],
                      [-s * sn, s * c, t - s * (-sn * centre[0] + c * centre[1])], [0, 0, 1]])
    else:
        M = np.array([[s, 0, t - s * centre[0]], [0, s, t - s * centre[1]], [0, 0, 1]])
    return M, np.linalg.inv(M)


def corners(dsize):
    return np.array([[0, 0], [dsize, 0], [0, dsize], [dsize, dsize]], dtype=np.float64)


def err(X, F, p):
    """The largest distance in pixels between X p and F p; X, F 3 x 3 (any float type), p (K,2)."""
    X, F, p = np.asarray(X, np.float64), np.asarray(F, np.float64), np.asarray(p, np.float64)
    a = p @ X[:2, :2].T + X[:2, 2]
    b = p @ F[:2, :2].T + F[:2, 2]
    return float(np.sqrt(((a - b) ** 2).sum(axis=1)).max())


def geometry_errors(M_o2c, M_c2o, lmk, dsize, scale, vy_ratio, flag_do_rot):
    """(err of M_o2c over the landmarks and the crop's corners taken back to the frame, err of M_c2o over the crop's corners) against matrices64."""
    F_o2c, F_c2o = matrices64(lmk, dsize, scale, vy_ratio, flag_do_rot)
    frame_corners = corners(dsize) @ F_c2o[:2, :2].T + F_c2o[:2, 2]      # the four crop corners, as points of the frame
    p = np.concatenate([np.asarray(lmk, np.float64), frame_corners])
    return err(M_o2c, F_o2c, p), err(M_c2o, F_c2o, corners(dsize))


def decode(out_pts, M_c2o, dsize):
    """human_landmark_runner.py:82-83 in float32, operation by operation: out_pts (2 Np,) float32, M_c2o 3 x 3 float32 -> (Np,2) float32."""
    q = np.asarray(out_pts, np.float32).reshape(-1, 2) * np.float32(dsize)
    m = np.asarray(M_c2o, np.float32)
    x = (q[:, 0] * m[0, 0] + q[:, 1] * m[0, 1]) + m[0, 2]
    y = (q[:, 0] * m[1, 0] + q[:, 1] * m[1, 1]) + m[1, 2]
    return np.stack([x, y], axis=1)


def decode64(out_pts, M_c2o, dsize):
    """The same on the same float32 inputs in float64 -> ((Np,2) values, (Np,2) bound terms |x m00| + |y m01| + |m02| per coordinate)."""
    q = np.asarray(out_pts, np.float32).astype(np.float64).reshape(-1, 2) * float(dsize)
    m = np.asarray(M_c2o, np.float32).astype(np.float64)
    val = q @ m[:2, :2].T + m[:2, 2]
    mag = np.abs(q) @ np.abs(m[:2, :2]).T + np.abs(m[:2, 2])
    return val, mag


DECODE_ULPS = 4 * 2.0 ** -24      # a term of a coordinate passes through four roundings at most: x dsize, the product, the two sums


def shape203(seed=0):
    """A fixed face-like 203-point shape in the unit square (the stand-in network's answer before its image term), float32 (203,2)."""
    rng = np.random.default_rng(seed)
    pts = 0.5 + 0.18 * rng.standard_normal((203, 2))
    pts[[0, 6, 12, 18]] = [0.33, 0.40] + 0.02 * rng.standard_normal((4, 2))      # left eye
    pts[[24, 30, 36, 42]] = [0.67, 0.40] + 0.02 * rng.standard_normal((4, 2))    # right eye
    pts[[48, 66]] = [[0.40, 0.72], [0.60, 0.72]]                                # lip corners
    return np.clip(pts, 0.05, 0.95).astype(np.float32)


def loop_shape():
    """The stand-in's fixed answer for a loop: the 203-point shape drawn in so that a trajectory keeps its size (span 0.63 x scale 1.5) and moved
    down by the crop's vy_ratio, so that it keeps its place from step to step."""
    return ((shape203() - np.float32(0.5)) * np.float32(0.7) + np.array([0.5, 0.6], np.float32)).astype(np.float32)


def standin_net(shape, device):
    """A deterministic, torch-only stand-in for the landmark network: the fixed shape + 0.05 x (mean of the crop's right half - left half,
    top - bottom), the same for every point.  inp (B,3,d,d) -> (B, 2 Np).  The shape is uploaded here, once: a call waits for nothing."""
    import torch
    base = torch.from_numpy(np.ascontiguousarray(shape, dtype=np.float32)).to(device)
    torch.cuda.synchronize(device)

    def net(inp):
        d = inp.shape[-1]
        dx = inp[:, :, :, d // 2:].mean(dim=(1, 2, 3)) - inp[:, :, :, :d // 2].mean(dim=(1, 2, 3))
        dy = inp[:, :, :d // 2, :].mean(dim=(1, 2, 3)) - inp[:, :, d // 2:, :].mean(dim=(1, 2, 3))
        return (base[None] + (0.05 * torch.stack([dx, dy], dim=1))[:, None, :]).reshape(inp.shape[0], -1).contiguous()
    return net


def synthetic_face(cx, cy, width, angle_deg, seed=0):
    """A 203-point face of `width` pixels centred at (cx, cy), turned by angle_deg, float32 (203,2)."""
    pts = (shape203(seed).astype(np.float64) - 0.5) * width
    a = np.deg2rad(angle_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (pts @ R.T + [cx, cy]).astype(np.float32)
