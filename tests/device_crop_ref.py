"""What the device-crop tests share (test_device_crop_cpu.py, test_gpu_device_crop.py): the numpy restatement of cs_crop_lmk's lmk_crop, the float64
evaluation it is held to, and the small scenes of the paste tests.  The images' references are the host-matrix kernels themselves
(tail.crop_faces_M, tail.paste_back_faces), which tests/test_gpu_multi_face.py holds to oracle/cv_ref.py."""
import numpy as np

import multi_face_ref as MF

LMK_CROP_ULPS = 3 * 2.0 ** -24      # a term of a coordinate passes through three roundings at most: the product and the two sums


def lmk_crop(lmk, M_o2c):
    """_transform_pts(lmk, M_o2c) (src/utils/crop.py:66-72) as cs_crop_lmk forms it: lmk (N,2), M_o2c 3x3 or 2x3, both taken as float32;
    (x m00 + y m01) + m02, (x m10 + y m11) + m12, every product and sum rounded to float32, in that order.  -> (N,2) float32."""
    p, m = np.asarray(lmk, np.float32), np.asarray(M_o2c, np.float32)
    x, y = p[:, 0], p[:, 1]
    cx = (x * m[0, 0] + y * m[0, 1]) + m[0, 2]
    cy = (x * m[1, 0] + y * m[1, 1]) + m[1, 2]
    assert cx.dtype == np.float32 and cy.dtype == np.float32
    return np.stack([cx, cy], axis=1)


def lmk_crop64(lmk, M_o2c):
    """The same in float64 on the same float32 inputs -> (values (N,2), magnitudes (N,2): |x m0| + |y m1| + |m2| per coordinate)."""
    p, m = np.asarray(lmk, np.float32).astype(np.float64), np.asarray(M_o2c, np.float32).astype(np.float64)
    val = p @ m[:2, :2].T + m[:2, 2]
    mag = np.abs(p) @ np.abs(m[:2, :2]).T + np.abs(m[:2, 2])
    return val, mag


def face5(cx, cy, width, angle_deg):
    """Five points - the eyes, the nose, the lip corners (landmarks.layout_of(5)) - of a face `width` pixels wide, float32 (5,2)."""
    pts = np.array([[-0.2, -0.15], [0.2, -0.15], [0.0, 0.05], [-0.13, 0.27], [0.13, 0.27]]) * width
    a = np.deg2rad(angle_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (pts @ R.T + [cx, cy]).astype(np.float32)


def m18(M_c2o):
    """(B,3,3) float64 crop -> frame matrices -> (B,18) float32 as the device holds them: M_o2c (the inverse) | M_c2o; and the float32 M_c2o
    widened back to float64, (B,3,3): what the host-matrix reference of the same paste takes."""
    M_c2o = np.asarray(M_c2o, np.float64).reshape(-1, 3, 3)
    both = np.concatenate([np.linalg.inv(M_c2o).reshape(-1, 9), M_c2o.reshape(-1, 9)], axis=1).astype(np.float32)
    return both, both[:, 9:].astype(np.float64).reshape(-1, 3, 3)


def paste_scene(seed=21, Wo=48):
    """F = 3 frames of 36 x Wo, crops 16 x 16, faces per frame [2, 0, 1]: frame 0's two faces overlap, frame 1 has none, frame 2's face is turned
    and reaches over the border.  Masks in [0, 1] with exact 0 and exact 1.  -> crops, masks, M_c2o (B,3,3) float64, frame_index, imgs_ori."""
    r = np.random.Generator(np.random.PCG64(seed))
    M = np.stack([MF.similarity(1.1, 0.1, 8.2, 6.4), MF.similarity(1.3, -0.25, 12.7, 9.1), MF.similarity(1.2, np.pi / 4 + 0.03, 40.3, 12.6)])
    fi = np.array([0, 0, 2], np.int32)
    return MF._bytes(r, (3, 16, 16, 3)), MF._masks(r, 3, 16, 16), M, fi, MF._bytes(r, (3, 36, Wo, 3))


def many_scene(faces_per_frame, Ho, Wo, seed):
    """len(faces_per_frame) frames of Ho x Wo with that many 8 x 8 faces each, placed at random about the frame."""
    r = np.random.Generator(np.random.PCG64(seed))
    fi = np.repeat(np.arange(len(faces_per_frame)), faces_per_frame).astype(np.int32)
    B = len(fi)
    M = np.stack([MF.similarity(r.uniform(0.6, 1.6), r.uniform(-0.8, 0.8), r.uniform(-3, Wo - 6), r.uniform(-3, Ho - 6)) for _ in range(B)])
    return MF._bytes(r, (B, 8, 8, 3)), MF._masks(r, B, 8, 8), M, fi, MF._bytes(r, (len(faces_per_frame), Ho, Wo, 3))
