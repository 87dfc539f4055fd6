"""Alignment of a detected face for the identity network, on the host (insightface_func/utils/face_align_ffhqandnewarc.py:14-42, :55-78).

``estimate_norm(kps5, image_size, mode)`` restates the reference's function of the same name: the similarity transform that brings the
detector's five points (eyes, nose, mouth corners) onto one of the templates, the template with the smallest summed point error taken.
The image step that follows it in the reference, ``cv2.warpAffine(img, M, (size, size), borderValue=0)`` (:85-91; face_detect_crop_multi.py:86),
needs no code of its own: it is ``tail.crop_faces_M(engine, frames, M, frame_index, size)``, which takes source -> destination matrices and a
frame index.

PARITY UNPINNED: the reference calls skimage's ``SimilarityTransform.estimate``; skimage is not at hand and its working dtype depends on
its version.  What is restated is the published closed form it implements (S. Umeyama, "Least-squares estimation of transformation
parameters between two point patterns", PAMI 13(4), 1991, eqs. 34-43), computed in float64.  A few hundred flops per face.
"""
from __future__ import annotations

import numpy as np

# the five templates of :14-37 at 112 x 112 (profile left, left, frontal, right, profile right) and the FFHQ one of :40-42 at 512 x 512: data
SRC_MAP = np.array([
    [[51.642, 50.115], [57.617, 49.990], [35.740, 69.007], [51.157, 89.050], [57.025, 89.702]],
    [[45.031, 50.118], [65.568, 50.872], [39.677, 68.111], [45.177, 86.190], [64.246, 86.758]],
    [[39.730, 51.138], [72.270, 51.138], [56.000, 68.493], [42.463, 87.010], [69.537, 87.010]],
    [[46.845, 50.872], [67.382, 50.118], [72.737, 68.111], [48.167, 86.758], [67.236, 86.190]],
    [[54.796, 49.990], [60.771, 50.115], [76.673, 69.007], [55.388, 89.702], [61.257, 89.050]],
], dtype=np.float32)
FFHQ_SRC = np.array([[[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043], [313.08905, 371.15118]]],
                    dtype=np.float64)


def templates(image_size=112, mode="None") -> np.ndarray:
    """The templates estimate_norm tries, scaled as :62-66 scales them: mode "ffhq": the one FFHQ template * image_size / 512; any other mode
    (the pipelines pass "None"): the five of src_map * image_size / 112 (float32 data times a Python int over a Python int: float32 under
    numpy 2's promotion, lifted to float64 here without changing a value)."""
    if mode == "ffhq":
        return FFHQ_SRC * image_size / 512
    return (SRC_MAP * image_size / 112).astype(np.float64)


def umeyama(src, dst) -> np.ndarray:
    """The 3 x 3 similarity (rotation, one scale, translation; no reflection) that maps src (N,2) onto dst (N,2) with the least summed squared
    error: Umeyama's closed form, float64."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n, dim = src.shape
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    sd, dd = src - ms, dst - md
    A = dd.T @ sd / n                                      # eq. 38
    d = np.ones(dim)
    if np.linalg.det(A) < 0:                               # eq. 39
        d[dim - 1] = -1
    T = np.eye(dim + 1)
    U, S, Vt = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.full((dim + 1, dim + 1), np.nan)
    if rank == dim - 1:                                    # eq. 43
        if np.linalg.det(U) * np.linalg.det(Vt) > 0:
            T[:dim, :dim] = U @ Vt
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ Vt
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ Vt                # eq. 40
    scale = 1.0 / sd.var(axis=0).sum() * (S @ d)           # eqs. 41, 42
    T[:dim, dim] = md - scale * (T[:dim, :dim] @ ms)
    T[:dim, :dim] *= scale
    return T


def estimate_norm(kps5, image_size=112, mode="None"):
    """face_align_ffhqandnewarc.py:55-78: kps5 (5,2), the detector's points in the frame -> (M (2,3) float64 frame -> aligned crop, index of the
    template taken): per template the similarity onto it, the error sum_i |M p_i - t_i| (:72), the first smallest wins (:74, strict <)."""
    lmk = np.asarray(kps5, dtype=np.float64)
    if lmk.shape != (5, 2):
        raise ValueError(f"estimate_norm: expected five points (5, 2), got {lmk.shape}")
    lmk_h = np.concatenate([lmk, np.ones((5, 1))], axis=1)
    best_M, best_i, best_err = None, -1, float("inf")
    for i, t in enumerate(templates(image_size, mode)):
        M = umeyama(lmk, t)[0:2, :]
        err = float(np.sum(np.sqrt(np.sum((lmk_h @ M.T - t) ** 2, axis=1))))
        if err < best_err:
            best_M, best_i, best_err = M, i, err
    if best_M is None:
        raise ValueError("estimate_norm: no template fits (degenerate or non-finite points)")
    return best_M, best_i


def norm_matrices(kps, image_size=112, mode="None"):
    """estimate_norm for B faces: kps (B,5,2) -> (M (B,2,3) float64, template indices (B,) int64)."""
    k = np.asarray(kps, dtype=np.float64)
    if k.ndim == 2:
        k = k[None]
    if k.ndim != 3 or k.shape[1:] != (5, 2) or k.shape[0] < 1:
        raise ValueError(f"norm_matrices: expected key points (B, 5, 2), B >= 1, got {np.shape(kps)}")
    res = [estimate_norm(p, image_size, mode) for p in k]
    return np.stack([m for m, _ in res]), np.array([i for _, i in res], dtype=np.int64)
