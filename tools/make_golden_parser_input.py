"""Writes tests/golden/parser_input.npz: what PIL's Image.resize(..., BILINEAR) makes of the small inputs of tests/parser_input_ref.py (and of one
64 x 64 input), and the (3, 256) table of SegformerImageProcessor's rescale + normalize as its numpy lines produce it.  Arrays only: the inputs,
PIL's uint8 outputs, the table.  Needs Pillow (the fixture was written with the version the script prints).

    python tools/make_golden_parser_input.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parser_input_ref as PR


def pil_resize_x2(x):
    """(B, h, w, 3) uint8 -> (B, 2h, 2w, 3) uint8, image by image, as the processor calls it (image_transforms.resize: PIL, size (2w, 2h))."""
    out = [np.asarray(Image.fromarray(np.ascontiguousarray(im)).resize((2 * im.shape[1], 2 * im.shape[0]), resample=Image.BILINEAR)) for im in x]
    return np.stack(out).astype(np.uint8)


def main():
    arrays = {}
    # the table by the processor's lines, written out flat (parser_input_ref.table and tail.parser_lut restate them in two other shapes)
    lut = np.empty((3, 256), np.float32)
    for c in range(3):
        image = np.arange(256, dtype=np.uint8)
        rescaled = (image * PR.RESCALE).astype(np.float32)
        lut[c] = (rescaled - np.array(PR.MEAN[c], dtype=np.float32)) / np.array(PR.STD[c], dtype=np.float32)
    arrays["lut"] = lut
    for name, kind in PR.fixture_items():
        x = PR.crops_of(name, kind, 0)
        arrays[f"{name}/{kind}/in"] = x
        arrays[f"{name}/{kind}/pil"] = pil_resize_x2(x)
    os.makedirs(os.path.dirname(PR.GOLDEN), exist_ok=True)
    np.savez_compressed(PR.GOLDEN, **arrays)
    print(f"Pillow {PIL.__version__}: {len(arrays)} arrays, {os.path.getsize(PR.GOLDEN)} bytes -> {PR.GOLDEN}")


if __name__ == "__main__":
    main()
