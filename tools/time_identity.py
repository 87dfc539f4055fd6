"""Timing of getid on the engine (cs_identity; csrc/identity.hip) on one MI355X beside the same network as a plain fp32 torch module on the same
device (tests/identity_ref.py TorchNet, the restatement the tests use); prints one JSON line.

    python tools/time_identity.py [--reps 30] [--out profiles/identity_b8.json]

Per batch size (1 and 8): 112 x 112 inputs resident in HBM, both candidates warmed, profiler off, all in ONE process; the two candidates alternate
repetition by repetition, each repetition is 4 calls inside a host clock that ends in a synchronise, the MEDIAN of the repetitions is reported with
the spread.  No ratio is fixed in advance: the record holds what was measured.  Needs a GPU: the engine raises without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

from canonswap_amd import synth
from canonswap_amd.can_swap_e2e import can_swapper
import identity_ref as R

FLOP_PER_IMAGE = 2 * 3.16e9      # multiply-adds of the convolutions and the fc at 112 x 112, times two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions per candidate and batch size (>= 20), 4 calls each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("arcface",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=8)
    e = sw.engine
    dev = e.device
    net = R.TorchNet(synth._arcface(0), torch.float32, dev)
    NP, res = 4, {}
    for B in (1, 8):
        x = torch.from_numpy(synth.make_identity_inputs(B, seed=3100, size=112)).to(dev)
        out = torch.empty((B, 512), dtype=torch.float32, device=dev)
        cand = {"engine": lambda: e.identity(x, out=out), "torch_fp32": lambda: net(x)}
        with torch.cuda.device(dev):
            err = float(R.rel_l2(cand["engine"](), cand["torch_fp32"]()).max())
            for f in cand.values():
                for _ in range(3):
                    f()
            torch.cuda.synchronize(dev)
            t = {k: [] for k in cand}
            for _ in range(max(20, a.reps)):
                for k, f in cand.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(NP):
                        f()
                    torch.cuda.synchronize(dev)
                    t[k].append((time.perf_counter() - t0) / NP * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        res[f"b{B}"] = {
            "engine_ms": round(med["engine"], 4), "torch_fp32_ms": round(med["torch_fp32"], 4),
            "engine_min_max_ms": [round(min(t["engine"]), 4), round(max(t["engine"]), 4)],
            "torch_fp32_min_max_ms": [round(min(t["torch_fp32"]), 4), round(max(t["torch_fp32"]), 4)],
            "torch_over_engine": round(med["torch_fp32"] / med["engine"], 3),
            "engine_TFLOPs": round(FLOP_PER_IMAGE * B / med["engine"] / 1e9, 3),
            "max_rel_l2_engine_vs_torch_fp32": err,
        }
    line = {
        "workload": "getid (can_swap_e2e.py:102-107) of B 112x112 fp32 images resident in HBM: cs_identity beside the same network as an eager fp32 "
                    "torch module (tests/identity_ref.py) on the same device",
        "repetitions": max(20, a.reps), "calls_per_repetition": NP, "statistic": "median", "flop_per_image": FLOP_PER_IMAGE,
        **res, "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
