"""Timing of the parser's input on the device (cs_parser_input; tail.parser_input, the chains' parser_input) on one MI355X; prints one JSON line.

    python tools/time_parser_input.py [--batch 64] [--reps 24] [--host-reps 5] [--chain-reps 20] [--out FILE]

B uint8 crops of 512 x 512 resident in HBM (seeded, smooth images), pixel_values (B,3,512,512) fp32 into a resident output, every shape warmed,
profiler off, all in ONE process:
  * the launch alone: repetitions of 4 calls, a host clock around calls that end in a synchronise, the MEDIAN of the repetitions; GB/s over the
    algorithmic bytes - crops read once, pixel_values written once;
  * the host route it replaces (can_swap_pipeline_e2e.py:171 + :180 per frame): D2H of the crops, then per frame the 2 x 2 mean of cv2.resize in
    numpy, PIL's resize to 512 x 512 BILINEAR and the processor's numpy lines (rescale, normalize, HWC -> CHW) on one thread, then H2D of the
    fp32 batch and a synchronise; its three parts timed apart.  Without Pillow the PIL part is skipped and the record says so;
  * FrameChain's step with parser_input of the same crops in front of it, beside the step alone, alternating repetition by repetition.
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

try:
    from PIL import Image
except ImportError:
    Image = None


def host_processor(frames_u8, mean, std, rescale):
    """The reference's lines on the host for crops already there: (B,512,512,3) uint8 -> (B,3,512,512) fp32 (needs Pillow)."""
    out = np.empty((len(frames_u8), 3, 512, 512), np.float32)
    m, s = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32)
    for i, f in enumerate(frames_u8):
        a = f.astype(np.uint16)
        x = ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)      # cv2.resize(f, (256, 256))
        r = np.asarray(Image.fromarray(x).resize((512, 512), resample=Image.BILINEAR))                # resize()
        r = (r * rescale).astype(np.float32)                                                                  # rescale()
        r = (r - m) / s                                                                                       # normalize()
        out[i] = r.transpose(2, 0, 1)                                                                         # to channels first
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions of the launch (>= 20), 4 calls each")
    ap.add_argument("--host-reps", type=int, default=5, help="timed repetitions of the host route")
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
    pv = torch.empty((B, 3, 512, 512), dtype=torch.float32, device=dev)

    def fused():
        tail.parser_input(e, crops, out=pv)

    NP = 4
    with torch.cuda.device(dev):
        for _ in range(3):
            fused()
        torch.cuda.synchronize(dev)
        t_fused = []
        for _ in range(max(20, a.reps)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(NP):
                fused()
            torch.cuda.synchronize(dev)
            t_fused.append((time.perf_counter() - t0) / NP * 1e3)
    med_fused = statistics.median(t_fused)

    # the host route, in the same process
    host = {"d2h_ms": [], "processor_ms": [], "h2d_ms": []}
    differ = None
    pinned_in = torch.empty(crops.shape, dtype=torch.uint8).pin_memory()
    pinned_out = torch.empty(pv.shape, dtype=torch.float32).pin_memory()
    back = torch.empty_like(pv)
    torch.set_num_threads(1)
    for rep in range(a.host_reps + 1):                                   # the first repetition warms and is dropped
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pinned_in.copy_(crops, non_blocking=True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if Image is not None:
            res = host_processor(pinned_in.numpy(), tail.PARSER_MEAN, tail.PARSER_STD, tail.PARSER_RESCALE)
            pinned_out.copy_(torch.from_numpy(res))
        t2 = time.perf_counter()
        back.copy_(pinned_out, non_blocking=True)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        if rep:
            host["d2h_ms"].append((t1 - t0) * 1e3); host["processor_ms"].append((t2 - t1) * 1e3); host["h2d_ms"].append((t3 - t2) * 1e3)
    if Image is not None:
        differ = int((back.view(torch.int32) != pv.view(torch.int32)).sum())
    med_host = {k: statistics.median(v) for k, v in host.items()}

    # FrameChain alone, and with parser_input of the same crops in front of it
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

    def chain_with():
        chain.parser_input(crops, out=pv)
        chain(crops, masks, M_c2o, frames, idv, out=outf)

    ch = {"chain_alone": chain_alone, "chain_with_parser_input": chain_with}
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

    bytes_in, bytes_out = B * 512 * 512 * 3, B * 3 * 512 * 512 * 4
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    host_total = sum(med_host.values())
    line = {
        "workload": f"cv2.resize to 256x256 + SegformerImageProcessor (PIL resize to 512x512 BILINEAR, rescale, normalize, CHW; can_swap_pipeline_e2e.py:171, 180) "
                    f"for {B} uint8 crops of 512x512 resident in HBM -> pixel_values ({B},3,512,512) fp32",
        "batch": B, "repetitions": len(t_fused), "calls_per_repetition": NP, "statistic": "median",
        "launch_ms": round(med_fused, 4), "launch_min_max_ms": spread(t_fused),
        "algorithmic_bytes": {"crops_read": bytes_in, "pixel_values_written": bytes_out},
        "launch_GBps": round((bytes_in + bytes_out) / med_fused / 1e6, 1),
        "host_route": {"repetitions": len(host["d2h_ms"]), "threads": 1,
                       "d2h_ms": round(med_host["d2h_ms"], 3), "h2d_ms": round(med_host["h2d_ms"], 3),
                       "processor_ms": round(med_host["processor_ms"], 3) if Image is not None else None,
                       "total_ms": round(host_total, 3) if Image is not None else None,
                       "total_over_launch": round(host_total / med_fused, 1) if Image is not None else None,
                       "note": None if Image is not None else "Pillow is not installed here: the PIL resize and the numpy lines were skipped, only the copies were timed",
                       "min_max_ms": {k: spread(v) for k, v in host.items()},
                       "values_differing_from_the_launch": differ},
        "chain": {"repetitions": len(tc["chain_alone"]), "chain_alone_ms_per_step": round(medc["chain_alone"], 3),
                  "chain_with_parser_input_ms_per_step": round(medc["chain_with_parser_input"], 3),
                  "chain_alone_frames_per_s": round(B / medc["chain_alone"] * 1e3, 2),
                  "chain_with_parser_input_frames_per_s": round(B / medc["chain_with_parser_input"] * 1e3, 2),
                  "ratio": round(medc["chain_alone"] / medc["chain_with_parser_input"], 4), "min_max_ms": {k: spread(v) for k, v in tc.items()}},
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
