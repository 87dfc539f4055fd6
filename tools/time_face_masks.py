"""Timing of the face mask from the parser's logits (cs_face_masks; tail.face_masks, the chains' logits=) on one MI355X; prints one JSON line.

    python tools/time_face_masks.py [--batch 64] [--reps 24] [--chain-reps 20] [--out FILE]

B frames of (19,128,128) fp32 logits resident in HBM (seeded and parser-like: smooth class fields with a face-sized region, face_field of
tests/face_mask_ref.py, which the tests' chains use too), masks at 512 x 512, every shape warmed, profiler off.  In ONE process, the
candidates alternating repetition by repetition (so that clock and temperature drift hits them alike), each repetition a host clock around
calls that end in a synchronise; the figure of a candidate is the MEDIAN of its repetitions:
  * the fused launch (tail.face_masks into a resident output);
  * the reference's torch lines on the same device (can_swap_pipeline_e2e.py:183-190): F.interpolate -> argmax -> isin -> .to(int), for the
    whole batch at once and frame by frame as the pipeline's loop runs them; with each the peak of torch.cuda.max_memory_allocated above
    what was allocated before the call;
  * FrameChain fed with the logits beside FrameChain fed with masks made beforehand (the chain's own work is the same).
The bandwidth figure is the algorithmic bytes - logits read once, masks written once - over the median time.  Needs a GPU: the engine
raises without one."""
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
import torch.nn.functional as F

from canonswap_amd import synth, tail
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from face_mask_ref import face_field


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions per kernel candidate (>= 20), 4 calls each")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, C, n, size = a.batch, 19, 128, (512, 512)
    Ho, Wo = 1080, 1920
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    few = torch.from_numpy(face_field(8, C, n, seed=2024))
    logits = few.repeat((B + 7) // 8, 1, 1, 1)[:B].contiguous().to(dev)
    logits += 0.01 * torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).to(dev)      # no two frames alike
    valid = torch.tensor(tail.FACE_VALID, device=dev)
    masks = torch.empty((B,) + size, dtype=torch.uint8, device=dev)

    def fused():
        tail.face_masks(e, logits, out=masks)

    def lines(lg):
        up = F.interpolate(lg, size=size, mode="bilinear", align_corners=False)
        labels = up.argmax(dim=1)
        return torch.isin(labels, valid).to(dtype=torch.int)

    def torch_batch():
        return lines(logits)

    def torch_frames():
        return [lines(logits[b:b + 1]) for b in range(B)]

    def peak_of(f):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        r = f()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - before
        del r
        return peak

    NP = 4                                                              # calls per repetition (sub-millisecond kernels)
    kern = {"fused": fused, "torch_batch": torch_batch, "torch_frames": torch_frames}
    with torch.cuda.device(dev):
        for f in kern.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize(dev)
        ref = torch_batch()
        differ = int((masks.to(torch.int) != ref).sum())
        del ref
        peaks = {k: peak_of(f) for k, f in kern.items()}
        t = {k: [] for k in kern}
        for _ in range(max(20, a.reps)):
            for k, f in kern.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(NP):
                    f()
                torch.cuda.synchronize(dev)
                t[k].append((time.perf_counter() - t0) / NP * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}

    # FrameChain: fed with masks made beforehand, and fed with the logits
    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = FrameChain(sw)
    smooth = synth.make_smooth_images(B, seed=2100, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    th, sc = 0.1, 0.9
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), 0.35 * Wo], [sc * np.sin(th), sc * np.cos(th), 0.2 * Ho], [0, 0, 1]], np.float64)
    M_c2o = np.stack([M] * B)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    ready = masks.clone()
    ch = {"chain_masks": lambda: chain(crops, ready, M_c2o, frames, idv, out=outf),
          "chain_logits": lambda: chain(crops, None, M_c2o, frames, idv, out=outf, logits=logits)}
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

    bytes_in, bytes_out = B * C * n * n * 4, B * size[0] * size[1]
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    line = {
        "workload": f"the torch lines between the parser and SoftErosion (can_swap_pipeline_e2e.py:183-190) for {B} frames of ({C},{n},{n}) fp32 logits "
                    f"resident in HBM -> {size[0]}x{size[1]} uint8 0/1 masks (F.interpolate bilinear, argmax, isin of the nine face classes)",
        "batch": B, "logits": [C, n, n], "size": list(size), "repetitions": len(t["fused"]), "calls_per_repetition": NP, "statistic": "median",
        "fused_ms": round(med["fused"], 4), "torch_lines_batch_ms": round(med["torch_batch"], 4), "torch_lines_per_frame_ms": round(med["torch_frames"], 4),
        "torch_batch_over_fused": round(med["torch_batch"] / med["fused"], 2), "torch_per_frame_over_fused": round(med["torch_frames"] / med["fused"], 2),
        "min_max_ms": {k: spread(v) for k, v in t.items()},
        "peak_bytes_allocated_during_call": peaks,
        "algorithmic_bytes": {"logits_read": bytes_in, "masks_written": bytes_out},
        "fused_GBps": round((bytes_in + bytes_out) / med["fused"] / 1e6, 1),
        "pixels_differing_from_torch_on_the_device": differ, "pixels": B * size[0] * size[1],
        "chain": {"repetitions": len(tc["chain_masks"]), "chain_with_masks_ms_per_step": round(medc["chain_masks"], 3),
                  "chain_with_logits_ms_per_step": round(medc["chain_logits"], 3),
                  "chain_with_masks_frames_per_s": round(B / medc["chain_masks"] * 1e3, 2), "chain_with_logits_frames_per_s": round(B / medc["chain_logits"] * 1e3, 2),
                  "ratio": round(medc["chain_masks"] / medc["chain_logits"], 4), "min_max_ms": {k: spread(v) for k, v in tc.items()}},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
