"""Timing of the side-by-side video frame on the device (cs_concat_frames; tail.concat_frames, FrameChain's concat=True) on one MI355X; prints
one JSON line.

    python tools/time_concat.py [--batch 64] [--reps 24] [--chain-reps 20] [--out FILE]

Everything resident in HBM, every shape warmed, profiler off, all in ONE process:
  * the launch alone in the e2e arrangement (can_swap_pipeline_e2e.py:290: driving crop u8, halved and resized back | rec_can fp32 | I_can fp32 |
    I_p u8, 512 x 512 each) for B frames into a resident (B,512,2048,3) output: repetitions of 4 calls, a host clock around calls that end in
    a synchronise, the MEDIAN of the repetitions; TB/s over the algorithmic bytes - every panel read once, the output written once;
  * FrameChain's step with concat=True beside the step without, alternating repetition by repetition on the same box: the difference is the
    price of the generator's two extra decodes (rec_can, swap_can) plus the launch.
No ratio is fixed in advance: the record holds what was measured.  Needs a GPU: the engine raises without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from canonswap_amd import synth, tail
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from chain_helpers import _masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions of the launch (>= 20), 4 calls each")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, Ho, Wo = a.batch, 1080, 1920
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    smooth = synth.make_smooth_images(B, seed=2100, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
    rec = torch.from_numpy(synth.make_smooth_images(B, seed=2200, size=512)).to(dev).float().contiguous()
    swp = torch.from_numpy(synth.make_smooth_images(B, seed=2300, size=512)).to(dev).float().contiguous()
    gen = crops.flip(0).contiguous()
    cat = torch.empty((B, 512, 2048, 3), dtype=torch.uint8, device=dev)
    kinds = [2, 3, 3, 0]

    def launch():
        tail.concat_frames(e, [crops, rec, swp, gen], kinds=kinds, out=cat)

    NP = 4
    with torch.cuda.device(dev):
        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        t_launch = []
        for _ in range(max(20, a.reps)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(NP):
                launch()
            torch.cuda.synchronize(dev)
            t_launch.append((time.perf_counter() - t0) / NP * 1e3)
    med = statistics.median(t_launch)

    # FrameChain's step without and with concat=True
    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = FrameChain(sw)
    masks = torch.from_numpy(_masks(8)).repeat((B + 7) // 8, 1, 1)[:B].contiguous().to(dev)
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    th, sc = 0.1, 0.9
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), 0.35 * Wo], [sc * np.sin(th), sc * np.cos(th), 0.2 * Ho], [0, 0, 1]], np.float64)
    M_c2o = np.stack([M] * B)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)

    def chain_alone():
        chain(crops, masks, M_c2o, frames, idv, out=outf)

    def chain_concat():
        chain(crops, masks, M_c2o, frames, idv, out=outf, concat=True, concat_out=cat)

    ch = {"chain_alone": chain_alone, "chain_with_concat": chain_concat}
    with torch.cuda.device(dev):
        for f in ch.values():
            f(); f()
        torch.cuda.synchronize(dev)
        tc = {k: [] for k in ch}
        for _ in range(max(20, a.chain_reps)):
            for k, f in ch.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(dev)
                tc[k].append((time.perf_counter() - t0) * 1e3)
    medc = {k: statistics.median(v) for k, v in tc.items()}

    px = B * 512 * 512
    nbytes = {"driving_u8_read": px * 3, "rec_can_f32_read": px * 12, "swap_can_f32_read": px * 12, "I_p_u8_read": px * 3, "concat_u8_written": px * 12}
    total = sum(nbytes.values())
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    line = {
        "workload": f"concat_frames (video.py:84-109 as called at can_swap_pipeline_e2e.py:290): driving crop (halved, resized x2) | rec_can | I_can | I_p "
                    f"of {B} frames, 512x512 panels resident in HBM -> ({B},512,2048,3) uint8",
        "batch": B, "kinds": kinds, "repetitions": len(t_launch), "calls_per_repetition": NP, "statistic": "median",
        "launch_ms": round(med, 4), "launch_min_max_ms": spread(t_launch),
        "algorithmic_bytes": nbytes, "algorithmic_bytes_total": total,
        "launch_TBps": round(total / med / 1e9, 3),
        "chain": {"repetitions": len(tc["chain_alone"]), "chain_alone_ms_per_step": round(medc["chain_alone"], 3),
                  "chain_with_concat_ms_per_step": round(medc["chain_with_concat"], 3),
                  "chain_alone_frames_per_s": round(B / medc["chain_alone"] * 1e3, 2),
                  "chain_with_concat_frames_per_s": round(B / medc["chain_with_concat"] * 1e3, 2),
                  "extra_ms_per_step": round(medc["chain_with_concat"] - medc["chain_alone"], 3),
                  "ratio": round(medc["chain_alone"] / medc["chain_with_concat"], 4), "min_max_ms": {k: spread(v) for k, v in tc.items()}},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
