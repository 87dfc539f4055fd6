"""The 4:2:0 conversions of include/canonswap_yuv.h restated in numpy: this file DEFINES their integer arithmetic, the kernels
(canonswap_amd/csrc/yuv.hip with yuv_math.h) equal it bit for bit (tests/test_gpu_yuv.py; tests/test_yuv_cpu.py holds yuv_math.h compiled for
the host to it).  It is itself held to the standards' float64 formula (formula_decode, formula_encode below) within 1 LSB.

A frame is (3 Ho / 2, Wo) uint8: rows 0 .. Ho - 1 the Y plane, the rest NV12's interleaved U V rows or I420's U plane followed by its V plane,
i.e. the frame's bytes in ffmpeg's rawvideo order seen Wo bytes per row."""
import numpy as np

LAYOUTS = ("nv12", "i420")
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SETS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]      # the four coefficient sets
DEC_BITS, ENC_BITS = 14, 16


def real(matrix, full_range):
    """Kr, Kg, Kb, sy, sc, y0 in float64."""
    Kr, Kb = MATRICES[matrix]
    Kg = (1.0 - Kr) - Kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return Kr, Kg, Kb, sy, sc, 0 if full_range else 16


def coef(matrix, full_range):
    """The integers, by the float64 operations of yuv_math.h yuv_coef in the same order."""
    Kr, Kg, Kb, sy, sc, y0 = real(matrix, full_range)
    d, n = float(1 << DEC_BITS), float(1 << ENC_BITS)
    rnd = lambda x: int(np.floor(x + 0.5))
    c = {"y0": y0}
    c["cy"] = rnd(sy * d)
    c["crv"] = rnd(((2.0 * (1.0 - Kr)) * sc) * d)
    c["cbu"] = rnd(((2.0 * (1.0 - Kb)) * sc) * d)
    c["cgu"] = rnd((((2.0 * Kb) * (1.0 - Kb) / Kg) * sc) * d)
    c["cgv"] = rnd((((2.0 * Kr) * (1.0 - Kr) / Kg) * sc) * d)
    c["ry"], c["gy"], c["by"] = rnd((Kr / sy) * n), rnd((Kg / sy) * n), rnd((Kb / sy) * n)
    du, dv = (2.0 * (1.0 - Kb)) * sc, (2.0 * (1.0 - Kr)) * sc
    c["ur"], c["ug"] = -rnd((Kr / du) * n), -rnd((Kg / du) * n)
    c["ub"] = -(c["ur"] + c["ug"])
    c["vg"], c["vb"] = -rnd((Kg / dv) * n), -rnd((Kb / dv) * n)
    c["vr"] = -(c["vg"] + c["vb"])
    return c


def _clamp(v):
    return np.clip(v, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ per value
def decode_values(Y, U, V, matrix="bt601", full_range=False):
    """Y, U, V integer arrays of one shape -> R, G, B uint8."""
    c = coef(matrix, full_range)
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    l = c["cy"] * (Y - c["y0"]) + (1 << (DEC_BITS - 1))
    u, v = U - 128, V - 128
    return _clamp((l + c["crv"] * v) >> DEC_BITS), _clamp((l - c["cgu"] * u - c["cgv"] * v) >> DEC_BITS), _clamp((l + c["cbu"] * u) >> DEC_BITS)


def encode_blocks(rgb, matrix="bt601", full_range=False):
    """rgb (..., 2, 2, 3) uint8 blocks -> Y (..., 2, 2), U (...), V (...) uint8."""
    c = coef(matrix, full_range)
    p = np.asarray(rgb).astype(np.int32)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = _clamp((c["ry"] * R + c["gy"] * G + c["by"] * B + (c["y0"] << ENC_BITS) + (1 << (ENC_BITS - 1))) >> ENC_BITS)
    sR, sG, sB = R.sum(axis=(-2, -1)), G.sum(axis=(-2, -1)), B.sum(axis=(-2, -1))
    bias = (128 << (ENC_BITS + 2)) + (1 << (ENC_BITS + 1))
    U = _clamp((c["ur"] * sR + c["ug"] * sG + c["ub"] * sB + bias) >> (ENC_BITS + 2))
    V = _clamp((c["vr"] * sR + c["vg"] * sG + c["vb"] * sB + bias) >> (ENC_BITS + 2))
    return Y, U, V


# ------------------------------------------------------------------------------------------------ frames
def _hw(yuv):
    yuv = np.asarray(yuv)
    if yuv.ndim != 3 or yuv.dtype != np.uint8 or yuv.shape[1] % 3 or yuv.shape[2] % 2 or (yuv.shape[1] // 3 * 2) % 2:
        raise ValueError(f"expected (F, 3 Ho / 2, Wo) uint8 with Ho and Wo even, got {yuv.shape} {yuv.dtype}")
    return yuv.shape[1] // 3 * 2, yuv.shape[2]


def split(yuv, layout):
    """(F, 3 Ho / 2, Wo) -> Y (F, Ho, Wo), U, V (F, Ho / 2, Wo / 2): copies."""
    Ho, Wo = _hw(yuv)
    F = yuv.shape[0]
    Y = yuv[:, :Ho].copy()
    if layout == "nv12":
        uv = yuv[:, Ho:].reshape(F, Ho // 2, Wo // 2, 2)
        return Y, uv[..., 0].copy(), uv[..., 1].copy()
    if layout != "i420":
        raise ValueError(f"layout {layout!r}")
    planes = yuv[:, Ho:].reshape(F, 2, Ho // 2, Wo // 2)
    return Y, planes[:, 0].copy(), planes[:, 1].copy()


def merge(Y, U, V, layout):
    F, Ho, Wo = Y.shape
    out = np.empty((F, Ho * 3 // 2, Wo), np.uint8)
    out[:, :Ho] = Y
    if layout == "nv12":
        out[:, Ho:] = np.stack([U, V], axis=-1).reshape(F, Ho // 2, Wo)
    elif layout == "i420":
        out[:, Ho:] = np.stack([U, V], axis=1).reshape(F, Ho // 2, Wo)
    else:
        raise ValueError(f"layout {layout!r}")
    return out


def decode_ref(yuv, layout="nv12", matrix="bt601", full_range=False):
    """(F, 3 Ho / 2, Wo) uint8 -> (F, Ho, Wo, 3) uint8: cs_yuv_to_rgb."""
    Y, U, V = split(yuv, layout)
    up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    return np.stack(decode_values(Y, up(U), up(V), matrix, full_range), axis=-1)


def rgb_to_yuv_ref(rgb, layout="nv12", matrix="bt601", full_range=False, keep=None):
    """(F, Ho, Wo, 3) uint8 -> (F, 3 Ho / 2, Wo) uint8: cs_rgb_to_yuv; keep: the YUV frames to update (not written: a new array is returned)."""
    rgb = np.asarray(rgb)
    F, Ho, Wo, _ = rgb.shape
    blocks = rgb.reshape(F, Ho // 2, 2, Wo // 2, 2, 3).transpose(0, 1, 3, 2, 4, 5)              # (F, Ho/2, Wo/2, 2, 2, 3)
    Yb, U, V = encode_blocks(blocks, matrix, full_range)
    Y = Yb.transpose(0, 1, 3, 2, 4).reshape(F, Ho, Wo)
    if keep is not None:
        Y0, U0, V0 = split(keep, layout)
        same = (decode_ref(keep, layout, matrix, full_range) == rgb).all(axis=-1)                # per pixel
        same = same.reshape(F, Ho // 2, 2, Wo // 2, 2).all(axis=(2, 4))                          # per block
        U, V = np.where(same, U0, U), np.where(same, V0, V)
        Y = np.where(np.repeat(np.repeat(same, 2, axis=1), 2, axis=2), Y0, Y)
    return merge(Y, U, V, layout)


# ------------------------------------------------------------------------------------------------ the standards' formula, float64
def formula_decode(Y, U, V, matrix, full_range):
    """-> R, G, B float64, unrounded and unclamped."""
    Kr, Kg, Kb, sy, sc, y0 = real(matrix, full_range)
    Y, U, V = (np.asarray(a, dtype=np.float64) for a in (Y, U, V))
    l = sy * (Y - y0)
    return (l + 2 * (1 - Kr) * sc * (V - 128), l - 2 * Kb * (1 - Kb) / Kg * sc * (U - 128) - 2 * Kr * (1 - Kr) / Kg * sc * (V - 128),
            l + 2 * (1 - Kb) * sc * (U - 128))


def formula_encode(rgb, matrix, full_range):
    """rgb (..., 2, 2, 3) -> Y (..., 2, 2), U, V (...) float64, unrounded: luma per pixel, chroma of the block's mean colour."""
    Kr, Kg, Kb, sy, sc, y0 = real(matrix, full_range)
    p = np.asarray(rgb, dtype=np.float64)
    luma = Kr * p[..., 0] + Kg * p[..., 1] + Kb * p[..., 2]
    m = p.mean(axis=(-3, -2))
    lm = Kr * m[..., 0] + Kg * m[..., 1] + Kb * m[..., 2]
    return y0 + luma / sy, 128 + (m[..., 2] - lm) / (2 * (1 - Kb) * sc), 128 + (m[..., 0] - lm) / (2 * (1 - Kr) * sc)


def exhaustive_nv12():
    """One 4096 x 4096 NV12 frame (1, 6144, 4096) that holds every (Y, U, V) triple once: the 2048 x 2048 blocks are numbered row by row,
    block b has (U, V) = (b >> 6) >> 8, (b >> 6) & 255 - 64 blocks per pair - and its four pixels the luma 4 (b & 63) + (0, 1, 2, 3)."""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair, base = b >> 6, (b & 63) * 4
    Y = np.empty((4096, 4096), np.uint8)
    Y[0::2, 0::2], Y[0::2, 1::2], Y[1::2, 0::2], Y[1::2, 1::2] = base, base + 1, base + 2, base + 3
    return merge(Y[None], (pair >> 8).astype(np.uint8)[None], (pair & 255).astype(np.uint8)[None], "nv12")
