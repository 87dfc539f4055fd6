"""Yardstick of the parser-input tests (test_parser_input_cpu.py, test_gpu_parser_input.py; not collected): what the reference executes on a
crop before SegFormer sees it (src/can_swap_pipeline_e2e.py:171 + :180, src/can_swap_pipeline_v2i.py:73), restated in numpy int64:

  1. cv2.resize(crop, one half) = (a + b + c + d + 2) >> 2 per 2 x 2 block (INTER_LINEAR and INTER_AREA agree at exactly one half);
  2. PIL's image.resize((2w, 2h), BILINEAR) (Resample.c, 22-bit fixed point; at exactly x2 the coefficients 0.75 / 0.25, 1.0 at both ends, are
     exact): per axis  out[2j] = (3 in[j] + in[max(j-1, 0)] + 2) >> 2,  out[2j+1] = (3 in[j] + in[min(j+1, n-1)] + 2) >> 2,  the horizontal
     pass first, its result stored as uint8, the vertical pass on that;
  3. rescale + normalize of transformers 4.38 (image_transforms.py) as a table of the byte, written here on a channels-last image as the
     processor holds it;
  4. HWC -> CHW.

tests/golden/parser_input.npz (tools/make_golden_parser_input.py) holds what PIL itself made of the small inputs, and the table."""
import functools
import os

import numpy as np

MEAN, STD, RESCALE = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 1 / 255      # SegformerImageProcessor's class defaults
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parser_input.npz")

# (B, h, w) of the image the two passes run on (after any halving); every case also runs with halve=1 from (B, 2h, 2w) crops.  1 x 1, single rows
# and columns: both clamps on one sample; odd widths: a last group of two output pixels, element stores; 33 x 65: more than one tile along either
# axis (a tile is 64 x 16 source pixels) with a partial last tile; 256 x 256: the pipelines' size, all stores wide.
CASES = {
    "one": (1, 1, 1), "row5": (2, 1, 5), "r2x3": (2, 2, 3), "r5x7": (3, 5, 7), "r16x4": (1, 16, 4), "r33x65": (2, 33, 65), "full": (2, 256, 256),
}
SMALL = [n for n in CASES if n != "full"]
FIXTURE_ONLY = {"sq64": (1, 64, 64)}                                            # in the fixture beside the small cases
KINDS = ("random", "sat", "edge")        # uniform bytes; 0 / 255 only (the + 2 >> 2 must never pass 255); draws from {0, 1, 2, 253, 254, 255}


def shape_of(name):
    return CASES.get(name) or FIXTURE_ONLY[name]


def crops_of(name, kind, halve=0):
    """The case's input: (B, h, w, 3) uint8, or (B, 2h, 2w, 3) with halve; seeded."""
    B, h, w = shape_of(name)
    names = list(CASES) + list(FIXTURE_ONLY)
    r = np.random.Generator(np.random.PCG64([4100, names.index(name), KINDS.index(kind), int(halve)]))
    shape = (B, h * (2 if halve else 1), w * (2 if halve else 1), 3)
    if kind == "random":
        x = r.integers(0, 256, size=shape)
    elif kind == "sat":
        x = r.integers(0, 2, size=shape) * 255
    else:
        x = np.array([0, 1, 2, 253, 254, 255])[r.integers(0, 6, size=shape)]
    return x.astype(np.uint8)


def halve_u8(x):
    """(..., 2h, 2w, 3) uint8 -> (..., h, w, 3) uint8: cv2.resize by exactly one half."""
    x = x.astype(np.int64)
    s = x[..., 0::2, 0::2, :] + x[..., 0::2, 1::2, :] + x[..., 1::2, 0::2, :] + x[..., 1::2, 1::2, :]
    return ((s + 2) >> 2).astype(np.uint8)


def _pass_x2(a, axis):
    """One axis pass n -> 2n of PIL's bilinear resize by exactly 2, in int64, rounded to uint8 as ImagingResample stores it."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    n = a.shape[0]
    j = np.arange(n)
    out = np.empty((2 * n,) + a.shape[1:], np.int64)
    out[0::2] = (3 * a + a[np.maximum(j - 1, 0)] + 2) >> 2
    out[1::2] = (3 * a + a[np.minimum(j + 1, n - 1)] + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize_x2(x, vertical_first=False):
    """(..., h, w, 3) uint8 -> (..., 2h, 2w, 3) uint8; PIL's order is horizontal, then vertical."""
    for axis in ((-3, -2) if vertical_first else (-2, -3)):
        x = _pass_x2(x, axis)
    return x


def table(mean=MEAN, std=STD, rescale=RESCALE):
    """(3, 256) fp32: rescale() and normalize() of the processor applied to a channels-last image that holds every byte in every channel."""
    image = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    rescaled = (image * rescale).astype(np.float32)                             # rescale(): uint8 array * Python float is float64
    m, s = np.array(mean, dtype=rescaled.dtype), np.array(std, dtype=rescaled.dtype)
    normalized = (rescaled - m) / s                                             # normalize(), channels last
    assert normalized.dtype == np.float32
    return np.ascontiguousarray(normalized.reshape(256, 3).T)


def pixel_values(u8, lut):
    """(B, H, W, 3) uint8 -> (B, 3, H, W) fp32 through the table."""
    return np.ascontiguousarray(np.stack([lut[c][u8[..., c]] for c in range(3)], axis=1))


def restate(crops, halve, lut=None):
    """-> {"resized_u8" (B,Ho,Wo,3) uint8, "pixel_values" (B,3,Ho,Wo) fp32}: steps 1 to 4."""
    x = halve_u8(crops) if halve else crops
    u8 = resize_x2(x)
    return {"resized_u8": u8, "pixel_values": pixel_values(u8, table() if lut is None else lut)}


@functools.lru_cache(maxsize=None)
def reference(name, kind, halve):
    """The case's input and yardstick, computed once and shared (read-only arrays)."""
    crops = crops_of(name, kind, halve)
    ref = dict(restate(crops, halve), crops=crops)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/parser_input.npz: {"lut": (3,256) fp32, "<case>/<kind>/in": (B,h,w,3) u8, "<case>/<kind>/pil": (B,2h,2w,3) u8}."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_items():
    """[(case, kind)] of the fixture, without reading it."""
    return [(n, k) for n in SMALL for k in KINDS] + [("sq64", "edge")]      # (the 64 x 64 input in one kind: the file stays under 200 KB)
