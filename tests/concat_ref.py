"""Yardstick of the concat tests (test_concat_cpu.py, test_gpu_concat.py; not collected): the pipelines' side-by-side video frame
(src/utils/video.py:84-109 concat_frames, called at src/can_swap_pipeline_e2e.py:290 and src/can_swap_pipeline_v2i.py:328), restated in numpy:
every panel is brought to S x S uint8 and the panels are stacked left to right (np.hstack).  A panel is one of four kinds:

  0  uint8 HWC S x S: the image itself (cv2.resize to the size it has is the identity);
  1  uint8 HWC S/2 x S/2: cv2.resize(img, (S, S)), default INTER_LINEAR, at exactly x2 (resize_x2_cv below);
  2  uint8 HWC S x S: cv2.resize to one half first (can_swap_pipeline_e2e.py:171, parser_input_ref.halve_u8), then kind 1;
  3  fp32 CHW 3 x S x S: parse_output (can_swap_e2e.py:314-322, oracle.canonswap_ref.parse_output).

PARITY UNPINNED: resize_x2_cv restates OpenCV's published 8-bit INTER_LINEAR arithmetic (11-bit coefficients, the vertical pass's
truncating shifts) from its description; no OpenCV was at hand to produce reference-owned vectors for it, so nothing here is pinned to
cv2's own output.  A x2 resize has only the weights 512 and 1536 (of 2048); a tap clamped at the left or right border takes 2048."""
import functools

import numpy as np
import torch

import parser_input_ref as PR
from oracle import canonswap_ref as O


def resize_x2_cv(u8):
    """(..., h, w, C) uint8 -> (..., 2h, 2w, C) uint8: cv2.resize(img, (2w, 2h)), INTER_LINEAR, 8-bit.
    Horizontal pass into int32: H[0] = 2048 s[0], H[2j] = 512 s[j-1] + 1536 s[j], H[2j+1] = 1536 s[j] + 512 s[j+1], H[2w-1] = 2048 s[w-1].
    Vertical pass: row 2i from rows (max(i-1, 0), i) with (512, 1536), row 2i+1 from rows (i, min(i+1, h-1)) with (1536, 512) - the row
    indices are clamped, the weights kept - dst = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2."""
    s = np.asarray(u8)
    assert s.dtype == np.uint8 and s.ndim >= 3
    s = s.astype(np.int64)
    h, w = s.shape[-3], s.shape[-2]
    H = np.empty(s.shape[:-2] + (2 * w, s.shape[-1]), np.int64)
    H[..., 0, :] = 2048 * s[..., 0, :]
    H[..., 2::2, :] = 512 * s[..., :-1, :] + 1536 * s[..., 1:, :]
    H[..., 1:-1:2, :] = 1536 * s[..., :-1, :] + 512 * s[..., 1:, :]
    H[..., 2 * w - 1, :] = 2048 * s[..., w - 1, :]
    H = np.moveaxis(H, -3, 0) >> 4                                              # rows first: (h, ..., 2w, C)
    i = np.arange(h)
    out = np.empty((2 * h,) + H.shape[1:], np.int64)
    out[0::2] = (((512 * H[np.maximum(i - 1, 0)]) >> 16) + ((1536 * H) >> 16) + 2) >> 2
    out[1::2] = (((1536 * H) >> 16) + ((512 * H[np.minimum(i + 1, h - 1)]) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(np.moveaxis(out, 0, -3).astype(np.uint8))


def panel_u8(x, kind):
    """One panel of B (or one shared) image(s) -> (n, S, S, 3) uint8."""
    x = np.asarray(x)
    if kind == 0:
        return x
    if kind == 1:
        return resize_x2_cv(x)
    if kind == 2:
        return resize_x2_cv(PR.halve_u8(x))
    if kind == 3:
        return O.parse_output(torch.from_numpy(np.array(x, dtype=np.float32)))              # a copy: the cases' arrays are read-only
    raise ValueError(kind)


def concat(panels, kinds, shared=None):
    """panels: P arrays, (B, ...) each or (1, ...) where shared -> (B, S, P * S, 3) uint8, the panels left to right."""
    shared = [0] * len(panels) if shared is None else shared
    B = max(np.asarray(p).shape[0] for p, sh in zip(panels, shared) if not sh) if not all(shared) else 1
    cols = []
    for p, k, sh in zip(panels, kinds, shared):
        u = panel_u8(p, k)
        assert u.dtype == np.uint8 and u.shape[0] == (1 if sh else B)
        cols.append(np.broadcast_to(u, (B,) + u.shape[1:]) if sh else u)
    return np.ascontiguousarray(np.concatenate(cols, axis=2))


# ------------------------------------------------------------------------------------------------ the operator tests' inputs
def _f32_values():
    """What parse_output can get wrong: negatives, -0.0, values above 1, every exact k / 255 and its two fp32 neighbours (k / 255 * 255 in fp32
    lands on either side of k, and the truncation shows it).  No NaN: the reference's cast of it is undefined."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    near = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))])
    other = np.array([-0.0, -1.5, -1e-8, 1e-8, 0.5, 1.0000001, 1.5, 2.0, 255.0, 1e30, -1e30, np.inf, -np.inf], np.float32)
    return np.concatenate([near, other]).astype(np.float32)


def panel_data(kind, n, S, seed):
    """n images of a panel of the given kind for panel size S, seeded: uint8 panels draw from all bytes and hold 0 and 255 in every image, fp32
    panels draw from _f32_values()."""
    r = np.random.Generator(np.random.PCG64([4300, kind, n, S, seed]))
    if kind == 3:
        v = _f32_values()
        return v[r.integers(0, len(v), size=(n, 3, S, S))]
    s = S // 2 if kind == 1 else S
    x = r.integers(0, 256, size=(n, s, s, 3)).astype(np.uint8)
    flat = x.reshape(n, -1)
    flat[:, 0::5] = 255
    flat[:, 1::5] = 0
    return x


def arrangements(P):
    """Four arrangements of P panels: with rot = 0..3 every kind stands in every position once; the shared flags alternate, never all set."""
    out = []
    for rot in range(4):
        kinds = [(rot + i) % 4 for i in range(P)]
        shared = [(rot + i) % 2 for i in range(P)]
        if all(shared):
            shared[0] = 0
        out.append((tuple(kinds), tuple(shared)))
    return out


@functools.lru_cache(maxsize=None)
def case(B, S, kinds, shared):
    """The case's panels and yardstick, computed once and shared (read-only arrays)."""
    panels = [panel_data(k, 1 if sh else B, S, i) for i, (k, sh) in enumerate(zip(kinds, shared))]
    want = concat(panels, kinds, shared)
    for a in panels + [want]:
        a.setflags(write=False)
    return panels, want
