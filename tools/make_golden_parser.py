"""tests/golden/parser_b2.npz: the installed transformers SegformerForSemanticSegmentation in float64 on synthetic weights (synth._segformer, seed 0,
geometry synth.PARSER_A), two 64 x 96 inputs.  The weights go into the class with strict=True after pack's rename table (which proves the table
complete); they come from the seed and are not stored.  Stored: the inputs as the uint8 images
the pixel_values are made of (synth.parser_pixel_values), the logits, and of each stage output every 16th element and the norm per image
(fp32: kilobytes; the float64 restatement is compared at fp32 resolution).  Run where transformers is installed:  python tools/make_golden_parser.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from canonswap_amd import synth  # noqa: E402
import parser_ref as R  # noqa: E402


STRIDE = 16


def main():
    cfg = dict(synth.PARSER_A)
    sd = synth._segformer(0, cfg)
    u8 = synth.make_parser_images(2, seed=4000, H=64, W=96)
    pv = synth.parser_pixel_values(u8)
    model = R.hf_model(sd, cfg, torch.float64)
    with torch.no_grad():
        o = model(pixel_values=torch.from_numpy(pv).double(), output_hidden_states=True)
    out = {"image_u8": u8, "logits": o.logits.numpy().astype(np.float32)}
    for s in range(4):          # every STRIDE-th element of the flattened stage output, and its norm per image
        h = o.hidden_states[s].numpy()
        out[f"stage{s}"] = h.reshape(2, -1)[:, ::STRIDE].astype(np.float32)
        out[f"stage{s}_norm"] = np.linalg.norm(h.reshape(2, -1), axis=1)
    path = os.path.join(ROOT, "tests", "golden", "parser_b2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
