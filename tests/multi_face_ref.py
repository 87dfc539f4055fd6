"""Several faces per frame, in numpy on top of oracle/cv_ref.py: the reference's paste_back (src/utils/crop.py:515-529) applied once per face, in
the faces' order, each on the result of the one before; the crop of face b from frame frame_index[b] (src/utils/crop.py:429-455).  And the
small scenes that tests/test_multi_face_cpu.py and tests/test_gpu_multi_face.py share."""
import numpy as np

from oracle import cv_ref as R


def paste_faces(crops, masks, M_c2o, frame_index, imgs_ori):
    """out = imgs_ori; for b in order: out[f] = paste_back(crops[b], M_c2o[b], out[f], prepare_paste_back(masks[b], M_c2o[b], (Wo, Ho))), f = frame_index[b]."""
    out = imgs_ori.copy()
    Ho, Wo = out.shape[1:3]
    for b in range(len(crops)):
        f = frame_index[b]
        out[f] = R.paste_back(crops[b], M_c2o[b], out[f], R.prepare_paste_back(masks[b], M_c2o[b], (Wo, Ho))[..., None])
    return out


def crop_faces(frames, M_o2c, frame_index, dsize):
    return np.stack([R.warp_affine_u8(frames[frame_index[b]], M_o2c[b], (dsize, dsize)) for b in range(len(M_o2c))])


def similarity(scale, angle, tx, ty):
    """crop -> frame: scale, rotation by `angle` (radians), then translation, as a 3x3 float64 matrix."""
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    return np.array([[c, -s, tx], [s, c, ty], [0, 0, 1]], np.float64)


def _bytes(r, shape):
    """Seeded bytes that certainly hold 0 and 255."""
    a = r.integers(0, 256, size=shape, dtype=np.uint8)
    a.reshape(-1)[:4] = (0, 255, 255, 0)
    a[..., -1, -1, :] = (255, 0, 255)
    return a


def _masks(r, B, Hc, Wc):
    """fp32 in [0, 1]: exact 0 in a band at the top, exact 1 in a block in the middle, anything between elsewhere."""
    m = r.uniform(0, 1, size=(B, Hc, Wc)).astype(np.float32)
    m[:, : max(1, Hc // 8)] = 0
    m[:, Hc // 3: Hc // 3 * 2, Wc // 3: Wc // 3 * 2] = 1
    return m


FACES = (2, 0, 3, 1)          # faces per frame of scene()


def scene(seed=3):
    """F = 4 frames of 24 x 36, crops 16 x 16, faces per frame [2, 0, 3, 1]: frame 0's two faces overlap (heavily: their centres are 3 pixels
    apart); frame 2 holds a face turned by about 45 degrees that reaches over the frame's border, a face wholly outside the frame, and a small
    upright one; frame 3's face covers the whole frame (a crop pixel is three frame pixels).  -> crops, masks, M_c2o, frame_index, imgs_ori."""
    r = np.random.Generator(np.random.PCG64(seed))
    F, Ho, Wo, Hc, Wc = 4, 24, 36, 16, 16
    frame_index = np.repeat(np.arange(F), FACES).astype(np.int32)
    M = np.stack([
        similarity(0.9, 0.1, 8.2, 3.4), similarity(1.0, -0.2, 10.7, 5.1),                    # frame 0: overlapping
        similarity(1.1, np.pi / 4 + 0.03, 30.3, 4.6),                                        # frame 2: turned, over the right and lower border
        similarity(0.8, 0.3, -40.5, 60.25),                                                  # frame 2: wholly outside
        similarity(0.5, 0.0, 3.25, 12.5),                                                    # frame 2: small, upright, inside
        similarity(3.0, 0.0, -5.5, -12.25),                                                  # frame 3: covers the frame (48 x 48 from (-5.5, -12.25))
    ])
    B = len(M)
    assert B == sum(FACES)
    return _bytes(r, (B, Hc, Wc, 3)), _masks(r, B, Hc, Wc), M, frame_index, _bytes(r, (F, Ho, Wo, 3))


def footprint(M_c2o, Hc, Wc, Ho, Wo):
    """Boolean (Ho, Wo): the frame's pixels that read the crop under M_c2o - those where a mask of ones, warped, is not zero."""
    return R.prepare_paste_back(np.ones((Hc, Wc), np.float32), M_c2o, (Wo, Ho)) > 0


def chunk_scene(seed=5):
    """F = 3 frames of 16 x 16, crops 8 x 8, faces [40, 0, 30]: more faces than one launch takes, a frame's faces in two launches."""
    r = np.random.Generator(np.random.PCG64(seed))
    F, Ho, Wo, Hc, Wc = 3, 16, 16, 8, 8
    frame_index = np.repeat(np.arange(F), (40, 0, 30)).astype(np.int32)
    B = len(frame_index)
    M = np.stack([similarity(r.uniform(0.6, 1.6), r.uniform(-0.8, 0.8), r.uniform(-3, 9), r.uniform(-3, 9)) for _ in range(B)])
    return _bytes(r, (B, Hc, Wc, 3)), _masks(r, B, Hc, Wc), M, frame_index, _bytes(r, (F, Ho, Wo, 3))
