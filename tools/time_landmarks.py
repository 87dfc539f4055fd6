"""Timing of landmark tracking on the device (cs_lmk_input, cs_lmk_decode; canonswap_amd/landmarks.py LandmarkTracker.track) on one MI355X; prints
one JSON line.

    python tools/time_landmarks.py [--batch 64] [--reps 24] [--chain-reps 20] [--out profiles/landmarks_b64.json]

B uint8 frames of 1080 x 1920 resident in HBM, one trajectory of 203 points, a stand-in network of negligible cost (tests/landmarks_ref.py's: two
half-image means and an add), every shape warmed, profiler off, all in ONE process:
  * `track` over the B frames: a host clock around a call that ends in a synchronise, the MEDIAN of the repetitions, in ms per tracked frame;
  * beside the host route the device route replaces, per frame: crop.crop_matrices in numpy, cs_crop_frames at 224, / 255 in torch, the network, a
    download of the 203 points, the decode in numpy, the next frame's crop from those landmarks;
  * FrameChain's B-face step alone, and with `track` of the next batch enqueued on a side stream beside it (the host
    enqueuing the chain first, or the tracker first), alternating repetition by repetition.
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

import landmarks_ref as LR
from canonswap_amd import crop, landmarks, synth, tail
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from chain_helpers import _masks


def timed(fn, reps, dev):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions of a pass over the batch (>= 20)")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, Ho, Wo = a.batch, 1080, 1920
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e, dev = sw.engine, sw.engine.device
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    net = LR.standin_net(LR.loop_shape(), dev)          # keeps the trajectory's size and place
    seed_np = LR.synthetic_face(960, 540, 400, 8)[None]
    seed = torch.from_numpy(seed_np).to(dev)
    tracker = landmarks.LandmarkTracker(sw, net)

    def device_route():
        return tracker.track(frames, seed)

    def host_route():
        lmk = seed_np[0]
        for k in range(B):
            M_o2c, M_c2o, _ = crop.crop_matrices(lmk[None], dsize=224, scale=1.5, vy_ratio=-0.1)
            crops = tail.crop_frames_M(e, frames[k:k + 1], M_o2c, 224)["crops"]
            pts = net(crops.permute(0, 3, 1, 2).float() / 255).cpu().numpy()
            lmk = LR.decode(pts[0], M_c2o[0], 224)
        return lmk

    reps = max(20, a.reps)
    t = {}
    with torch.cuda.device(dev):
        for k, fn in (("device", device_route), ("host", host_route)):
            fn(); fn()
            t[k] = timed(fn, reps, dev)
    med = {k: statistics.median(v) for k, v in t.items()}
    last_dev = device_route()[0][-1, 0].cpu().numpy()
    apart = float(np.abs(last_dev - host_route()).max())          # the two routes after B steps, in pixels of the frame

    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = FrameChain(sw)
    smooth = synth.make_smooth_images(B, seed=2100, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
    masks = torch.from_numpy(_masks(8)).repeat((B + 7) // 8, 1, 1)[:B].contiguous().to(dev)
    th, sc = 0.1, 0.9
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), 0.35 * Wo], [sc * np.sin(th), sc * np.cos(th), 0.2 * Ho], [0, 0, 1]], np.float64)
    M_c2o = np.stack([M] * B)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)

    def chain_alone():
        chain(crops, masks, M_c2o, frames, idv, out=outf)

    def chain_with_track(chain_first):
        cur = torch.cuda.current_stream(dev)
        side.wait_stream(cur)                        # the side stream waits for what came before this step, not for the step
        if chain_first:                              # the host enqueues the generator, then the tracker's steps while the generator runs
            chain(crops, masks, M_c2o, frames, idv, out=outf)
        with torch.cuda.stream(side):
            tracker.track(frames, seed)              # the next batch's landmarks, beside this batch's generator
        if not chain_first:                          # the host enqueues the tracker's steps first: the generator starts after that host time
            chain(crops, masks, M_c2o, frames, idv, out=outf)
        cur.wait_stream(side)

    ch = {"chain_alone": chain_alone, "chain_then_track": lambda: chain_with_track(True), "track_then_chain": lambda: chain_with_track(False)}
    with torch.cuda.device(dev):
        for fn in ch.values():
            fn(); fn()
        tc = {k: [] for k in ch}
        for _ in range(max(20, a.chain_reps)):
            for k, fn in ch.items():
                tc[k] += timed(fn, 1, dev)
    medc = {k: statistics.median(v) for k, v in tc.items()}

    spread = lambda v, n=1: [round(min(v) / n, 4), round(max(v) / n, 4)]
    line = {
        "workload": f"LandmarkRunner.run (human_landmark_runner.py:60-85) over {B} uint8 frames of {Ho}x{Wo} resident in HBM, one trajectory of 203 points, "
                    "frame k cropped around the landmarks of frame k - 1 (cropper.py:186-193), a stand-in network of two half-image means",
        "batch": B, "statistic": "median", "repetitions": reps,
        "track": {"ms_per_frame": round(med["device"] / B, 4), "min_max_ms_per_frame": spread(t["device"], B), "launches_per_frame": "cs_lmk_input, the network, a copy, cs_lmk_decode"},
        "host_route": {"ms_per_frame": round(med["host"] / B, 4), "min_max_ms_per_frame": spread(t["host"], B),
                       "per_frame": "crop.crop_matrices (numpy), cs_crop_frames at 224, / 255 (torch), the network, D2H of 203 points, decode (numpy)",
                       "over_track": round(med["host"] / med["device"], 2)},
        "routes_apart_after_batch_px": round(apart, 4),
        "chain": {"repetitions": len(tc["chain_alone"]), "chain_alone_ms_per_step": round(medc["chain_alone"], 3),
                  "chain_then_track_ms_per_step": round(medc["chain_then_track"], 3),
                  "track_then_chain_ms_per_step": round(medc["track_then_chain"], 3),
                  "ratio_chain_then_track": round(medc["chain_alone"] / medc["chain_then_track"], 4),
                  "ratio_track_then_chain": round(medc["chain_alone"] / medc["track_then_chain"], 4), "min_max_ms": {k: spread(v) for k, v in tc.items()}},
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
