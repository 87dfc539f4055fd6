"""Writes tests/golden/identity_b3.npz: what the reference's own identity network class makes of three synthetic inputs under the synthetic
weights synth._arcface(0).  Build machine only (imports the reference checkout, CPU, about a second per image); the fixture holds the seeds,
the 3 x 512 raw embeddings, mean |.| and max |.| per stage and the class's state-dict key names and shapes - no weights.

The reference file calls conv3x3 without defining it (the pickled checkpoint never needs the source); it is supplied here as the upstream
definition: 3x3, the given stride, padding 1, no bias.

    python tools/make_golden_identity.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from canonswap_amd import synth
from ref_import import REF

GOLDEN = os.path.join(ROOT, "tests", "golden", "identity_b3.npz")
WEIGHT_SEED, INPUT_SEED, N = 0, 3000, 3


def golden_inputs():
    """The fixture's inputs (tests/test_identity_cpu.py builds the same): image 1 is the constant 0.5."""
    img = synth.make_identity_inputs(N, seed=INPUT_SEED, size=112)
    img[1] = 0.5
    return img


def main():
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import models.arcface_models as AM
    AM.conv3x3 = lambda cin, cout, stride=1: torch.nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)
    net = AM.ResNet(AM.IRBlock, [3, 4, 14, 3], use_se=True).eval()
    own = net.state_dict()
    sd = synth.to_torch({"arcface": synth._arcface(WEIGHT_SEED)})["arcface"]
    net.load_state_dict(sd, strict=True)
    stages = {}
    hooks = [net.maxpool.register_forward_hook(lambda m, i, o: stages.__setitem__("stem", o)),
             net.bn2.register_forward_hook(lambda m, i, o: stages.__setitem__("prefc", o))]
    for l in range(1, 5):
        hooks.append(getattr(net, f"layer{l}").register_forward_hook(lambda m, i, o, l=l: stages.__setitem__(f"layer{l}", o)))
    with torch.no_grad():
        raw, _ = net(torch.from_numpy(golden_inputs()))
    names = ("stem", "layer1", "layer2", "layer3", "layer4", "prefc")
    arrays = {
        "weight_seed": np.array(WEIGHT_SEED), "input_seed": np.array(INPUT_SEED),
        "raw": raw.numpy().astype(np.float32),
        "stage_names": np.array(names),
        "stage_mean_abs": np.array([[stages[k][b].abs().mean().item() for k in names] for b in range(N)], np.float64),
        "stage_max_abs": np.array([[stages[k][b].abs().max().item() for k in names] for b in range(N)], np.float64),
        "keys": np.array(list(own.keys())),
        "shapes": np.array([",".join(map(str, v.shape)) for v in own.values()]),
    }
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **arrays)
    print(f"{len(own)} keys, {sum(v.numel() for k, v in own.items() if 'num_batches' not in k) / 1e6:.1f} M parameters; raw |.| max "
          f"{np.abs(arrays['raw']).max():.3f}; stage max |.| {arrays['stage_max_abs'].max(0)}; {os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    main()
