"""What the face-mask tests share (test_face_mask_cpu.py, test_gpu_face_mask.py): the three torch lines between the parser and SoftErosion
(src/can_swap_pipeline_e2e.py:183-190, src/can_swap_pipeline_v2i.py:76-83) as the yardstick, the seeded inputs, and the comparison rule.

    up = F.interpolate(logits, size=size, mode="bilinear", align_corners=False);  labels = up.argmax(dim=1);  mask = torch.isin(labels, valid)

The reference of every comparison is these lines in float64.  A pixel is DECIDED when the float64 margin between its two largest up-sampled
logits is at least MARGIN * max|logit| of the input: the fp32 expression v = hl0 (wl0 a + wl1 b) + hl1 (wl0 c + wl1 d) has exact weights
(scale 1, 2, 4) and seven roundings of values no larger than max|logit|, so it errs by a few ulp of the largest operand, below
5e-7 max|logit| on the difference of two classes; 1e-5 leaves twenty times that.  Labels and mask must be equal on every decided pixel,
and at most CAP of an input's pixels may be undecided."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

FACE_VALID = (1, 2, 4, 5, 6, 7, 10, 11, 12)
MARGIN = 1e-5
CAP = 1e-3

# name -> (logits shape, output size): the shapes of the GPU parity tests
CASES = {
    "one_cell": ((1, 19, 1, 1), (4, 4)),                 # every tap is clamped
    "borders": ((3, 19, 5, 7), (20, 28)),                # borders on all sides, the width no multiple of 16, an odd batch
    "pipeline": ((2, 19, 128, 128), (512, 512)),         # the pipelines' own shape: more than one workgroup per frame
    "s1": ((2, 19, 6, 10), (6, 10)),
    "s2": ((2, 19, 6, 10), (12, 20)),
    "c1": ((1, 1, 5, 7), (20, 28)),
    "c32": ((1, 32, 5, 7), (20, 28)),
}


def face_field(B, C=19, n=128, seed=0):
    """Parser-like logits (B,C,n,n): smooth per-class fields a few units high, class 0 (background) winning outside an ellipse and class 1
    (skin) inside, the other classes in blobs; its masks are face-sized regions with ragged rims."""
    r = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64) / n
    out = np.empty((B, C, n, n), np.float32)
    for b in range(B):
        cx, cy, a, bb = r.uniform(0.42, 0.58), r.uniform(0.42, 0.58), r.uniform(0.24, 0.36), r.uniform(0.3, 0.42)
        d = np.sqrt(((xx - cx) / a) ** 2 + ((yy - cy) / bb) ** 2)
        for c in range(C):
            px, py, s = r.uniform(0.2, 0.8), r.uniform(0.2, 0.8), r.uniform(0.05, 0.2)
            blob = 5.0 * np.exp(-((xx - px) ** 2 + (yy - py) ** 2) / (2 * s * s)) - 2.0
            f = 6.0 * (d - 1) if c == 0 else (6.0 * (1 - d) if c == 1 else blob)
            out[b, c] = f + 0.3 * r.normal(0, 1, (n, n))
    return out


@functools.lru_cache(maxsize=None)
def logits_of(name):
    """The seeded input of a case, fp32 on the host (do not modify: shared)."""
    shape, _ = CASES[name]
    r = np.random.Generator(np.random.PCG64(1000 + sorted(CASES).index(name)))
    x = r.normal(0, 1, shape).astype(np.float32)
    if name == "pipeline":
        x[1] = face_field(1, shape[1], shape[2], seed=7)[0]          # frame 0: N(0,1) noise, frame 1: a smooth, scaled field
    t = torch.from_numpy(x)
    return t


def torch_lines(logits, size, valid=FACE_VALID):
    """The reference's lines as they stand, in the dtype and on the device of `logits` -> (labels int64, mask bool), (B,H,W)."""
    up = F.interpolate(logits, size=tuple(size), mode="bilinear", align_corners=False)
    labels = up.argmax(dim=1)
    return labels, torch.isin(labels, torch.tensor(list(valid), dtype=labels.dtype, device=labels.device))


def reference_of(logits, size, valid=FACE_VALID):
    """float64 yardstick of one input -> dict(labels (B,H,W) uint8, mask (B,H,W) uint8, margin (B,H,W) float64, decided (B,H,W) bool)."""
    lg = torch.as_tensor(logits).detach().cpu().double()
    up = F.interpolate(lg, size=tuple(size), mode="bilinear", align_corners=False)
    labels = up.argmax(dim=1)
    mask = torch.isin(labels, torch.tensor(list(valid), dtype=labels.dtype))
    if lg.shape[1] > 1:
        top = up.topk(2, dim=1).values
        margin = top[:, 0] - top[:, 1]
    else:
        margin = torch.full(labels.shape, float("inf"), dtype=torch.float64)
    decided = margin >= MARGIN * lg.abs().max()
    return dict(labels=labels.to(torch.uint8), mask=mask.to(torch.uint8), margin=margin, decided=decided)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The yardstick of a case, computed once (do not modify: shared)."""
    return reference_of(logits_of(name), CASES[name][1])


def undecided_fraction(ref):
    return float((~ref["decided"]).double().mean())


def assert_agrees(ref, labels=None, mask=None, what=""):
    """Equality with the float64 yardstick on every decided pixel, and the cap on undecided pixels."""
    frac = undecided_fraction(ref)
    assert frac <= CAP, f"{what}: {frac:.3g} of the pixels are undecided (cap {CAP})"
    dec = ref["decided"]
    for name, got, want in (("labels", labels, ref["labels"]), ("mask", mask, ref["mask"])):
        if got is None:
            continue
        got = torch.as_tensor(got).detach().cpu()
        assert tuple(got.shape) == tuple(want.shape), f"{what}: {name} shape {tuple(got.shape)}, expected {tuple(want.shape)}"
        bad = (got.to(torch.int64) != want.to(torch.int64)) & dec
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} decided pixels with the wrong {name} (first at {bad.nonzero()[0].tolist()})"
