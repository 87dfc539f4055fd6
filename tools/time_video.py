"""Timing of the video driver (canonswap_amd/video.py) on one MI355X: host frames through FrameChain and back; prints one JSON line.

    python tools/time_video.py [--frames 640] [--batch 64] [--size 1080x1920] [--reps 10] [--out profiles/video_b64.json]
    python tools/time_video.py --pixel-format nv12 --out profiles/video_yuv_b64.json

One process, every shape warmed, profiler off.  Per repetition, in alternation on the same box, one pass over the same video each (a host
clock around a pass that ends with its last frame on the host, or in a device synchronise):
  a. VideoSwapper.swap_video, masks on the device, identity slots: from a pageable ndarray to a pageable ndarray, from a pinned tensor to a
     pageable ndarray, and from a pinned tensor to a pinned tensor (no staging memcpy either way);
  b. the synchronous loop of tests/test_gpu_video.py per batch: torch.from_numpy(...).to(device), chain.crop, chain(...), .cpu();
  c. FrameChain on device-resident crops and frames, stage A prefetched, as bench.py --full times its `chain` (no crop step, no copy).
The MEDIAN of the repetitions with min and max, the ratios a/c and a/b in frames per second, the bytes moved per step, the host-side staging
time per batch, and - from one further traced pass per source kind, timing events at every stage boundary of the driver - where a step's time
goes: the copies, the caller's stream waiting for an upload, the sink waiting for the paste-back.  Nothing is fixed in advance: the record
holds what was measured.  Needs a GPU: the engine raises without one.

--pixel-format nv12 (or i420) adds, in the same alternation, the driver on 4:2:0 frames of the same size (random bytes, pageable to pageable
and pinned to pinned; checked against the synchronous device loop yuv_to_rgb, crop, chain, rgb_to_yuv(keep=) per batch), its traced pass,
the bytes over the link in either format, and the two conversion launches on one step's frames timed on their own (events around each,
median of 20, with the bytes they move and the rate that makes)."""
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

from canonswap_amd import synth
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from canonswap_amd.video import VideoSwapper, plan_batches
from chain_helpers import _masks
from test_gpu_crop import _face


def _stage_times(trace, nb):
    """Medians over the steady-state batches (2 .. nb-2) of the driver's trace -> ms per step, by stage."""
    ev = {(k, name): e for k, name, e in trace}
    ks = [k for k in range(2, nb - 1) if all((k, n) in ev for n in ("h2d_begin", "h2d_end", "crop_queued", "crop_begin", "crop_end", "chain_begin",
                                                                      "chain_end", "d2h_begin", "d2h_end"))]
    span = lambda a, b: round(statistics.median(ev[(k, a)].elapsed_time(ev[(k, b)]) for k in ks), 3)
    step = round(statistics.median(ev[(k, "chain_end")].elapsed_time(ev[(k + 1, "chain_end")]) for k in ks[:-1]), 3)
    yuv = {}
    if ks and all((k, n) in ev for k in ks for n in ("rgb_ready", "paste_end")):          # a 4:2:0 pass: the two conversions, inside `crop` and `generator...`
        yuv = {"yuv_to_rgb_incl_in_crop": span("crop_begin", "rgb_ready"), "rgb_to_yuv_keep_incl_in_generator_and_paste": span("paste_end", "chain_end")}
    return {**yuv, "batches": len(ks), "step_chain_end_to_chain_end": step, "h2d_copy": span("h2d_begin", "h2d_end"), "d2h_copy": span("d2h_begin", "d2h_end"),
            "caller_stream_waits_for_upload": span("crop_queued", "crop_begin"), "crop": span("crop_begin", "crop_end"),
            "generator_and_paste_incl_wait_for_stage_a": span("chain_begin", "chain_end"), "sink_waits_after_paste": span("chain_end", "d2h_begin"),
            "paste_end_to_frames_on_host": span("chain_end", "d2h_end")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--reps", type=int, default=10, help="timed repetitions per candidate (>= 10), one pass over the video each")
    ap.add_argument("--pixel-format", default="rgb24", choices=["rgb24", "nv12", "i420"], help="also time the driver on 4:2:0 frames of this format")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, B = a.frames, a.batch
    Ho, Wo = (int(v) for v in a.size.lower().split("x"))
    reps = max(10, a.reps)
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    chain = FrameChain(sw)
    e.set_identity(torch.from_numpy(synth.make_identity(7)).to(dev), 0)
    r = np.random.Generator(np.random.PCG64(3))
    base = r.integers(0, 256, size=(min(N, B), Ho, Wo, 3), dtype=np.uint8)
    frames = np.concatenate([base] * ((N + len(base) - 1) // len(base)))[:N]      # pageable, N * Ho * Wo * 3 bytes of its own
    del base
    pinned = torch.from_numpy(frames).pin_memory()
    out_np = np.empty_like(frames)
    out_pin = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    lmk = np.stack([_face(r, (r.uniform(0.3, 0.7) * Wo, r.uniform(0.35, 0.65) * Ho), r.uniform(0.14, 0.2) * Wo, r.uniform(-0.3, 0.3)) for _ in range(N)])
    masks = torch.from_numpy(_masks(8)).repeat((N + 7) // 8, 1, 1)[:N].contiguous().to(dev)
    slots = [0] * N
    plan = plan_batches(N, None, B, B)
    drv = VideoSwapper(sw, batch=B, chain=chain)

    def a_pageable():
        drv.swap_video(frames, lmk, slots=slots, masks=masks, out=out_np)

    def a_pinned():
        drv.swap_video(pinned, lmk, slots=slots, masks=masks, out=out_np)

    def a_pinned_to_pinned():
        drv.swap_video(pinned, lmk, slots=slots, masks=masks, out=out_pin)

    def b_loop():
        for f0, f1, b0, b1 in plan:
            fr = torch.from_numpy(frames[f0:f1]).to(dev)
            c = chain.crop(fr, lmk[b0:b1])
            res = chain(c["crops"], masks[b0:b1], c["M_c2o"], fr, slots=slots[b0:b1])
            out_np[f0:f1] = res["frames"].cpu().numpy()

    fr0 = torch.from_numpy(frames[:B]).to(dev)
    c0 = chain.crop(fr0, lmk[:B])
    crops, crops_b, M0, m0, outf = c0["crops"], c0["crops"].clone(), c0["M_c2o"], masks[:B], torch.empty_like(fr0)

    def c_resident():
        cur, nxt = crops, crops_b
        chain.prefetch(cur, m0)
        for _ in range(len(plan)):
            chain.prefetch(nxt, m0)
            chain(cur, m0, M0, fr0, slots=slots[:B], out=outf)
            cur, nxt = nxt, cur
        chain.drop_prefetches()
        torch.cuda.synchronize(dev)

    cands = {"a_pageable_to_pageable": a_pageable, "a_pinned_to_pageable": a_pinned, "a_pinned_to_pinned": a_pinned_to_pinned,
             "b_synchronous_loop": b_loop, "c_chain_device_resident_prefetched": c_resident}
    fmt = a.pixel_format
    if fmt != "rgb24":
        from canonswap_amd import tail
        ybase = r.integers(0, 256, size=(min(N, B), Ho * 3 // 2, Wo), dtype=np.uint8)
        yuv = np.concatenate([ybase] * ((N + len(ybase) - 1) // len(ybase)))[:N]
        del ybase
        yuv_pin = torch.from_numpy(yuv).pin_memory()
        yout_np, yout_pin, yloop = np.empty_like(yuv), torch.empty(yuv.shape, dtype=torch.uint8).pin_memory(), np.empty_like(yuv)

        def y_pageable():
            drv.swap_video(yuv, lmk, slots=slots, masks=masks, out=yout_np, pixel_format=fmt)

        def y_pinned_to_pinned():
            drv.swap_video(yuv_pin, lmk, slots=slots, masks=masks, out=yout_pin, pixel_format=fmt)

        def y_loop():
            for f0, f1, b0, b1 in plan:
                y = torch.from_numpy(yuv[f0:f1]).to(dev)
                fr = tail.yuv_to_rgb(e, y, fmt)
                c = chain.crop(fr, lmk[b0:b1])
                chain(c["crops"], masks[b0:b1], c["M_c2o"], fr, slots=slots[b0:b1], out=fr)
                yloop[f0:f1] = tail.rgb_to_yuv(e, fr, fmt, keep=y).cpu().numpy()

        cands.update({f"a_{fmt}_pageable_to_pageable": y_pageable, f"a_{fmt}_pinned_to_pinned": y_pinned_to_pinned, f"b_{fmt}_synchronous_loop": y_loop})
    t = {k: [] for k in cands}
    staging = {k: [] for k in cands if k.startswith("a_")}
    with torch.cuda.device(dev):
        for f in cands.values():
            f()
        torch.cuda.synchronize(dev)
        b_loop()
        a_pinned_to_pinned()
        same = bool(np.array_equal(out_pin.numpy(), out_np))                     # the driver's bytes against the loop's, at the timed size
        if fmt != "rgb24":
            y_loop()
            y_pinned_to_pinned()
            same = same and bool(np.array_equal(yout_pin.numpy(), yloop))
            kept_blocks = float(((yloop[:B] == yuv[:B])[:, :Ho].reshape(B, Ho // 2, 2, Wo // 2, 2).all(axis=(2, 4))).mean())
        for i in range(reps):
            print(f"repetition {i + 1} of {reps}", file=sys.stderr, flush=True)
            for k, f in cands.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k in staging:
                    staging[k].append(statistics.median(drv.staging_ms))
        stages = {}
        for k in [k for k in cands if k.startswith("a_") and k != "a_pinned_to_pageable"]:
            drv.trace = []
            cands[k]()
            torch.cuda.synchronize(dev)
            stages[k] = _stage_times(drv.trace, len(plan))
            drv.trace = None

        launches = None
        if fmt != "rgb24":                                                       # the two conversions of one step's frames, on their own
            y64 = torch.from_numpy(yuv[:B]).to(dev)
            rgb64 = tail.yuv_to_rgb(e, y64, fmt)
            c = chain.crop(rgb64, lmk[:B])
            chain(c["crops"], masks[:B], c["M_c2o"], rgb64, slots=slots[:B], out=rgb64)      # pasted: what the encode meets in the driver
            back = y64.clone()
            scratch_rgb = torch.empty_like(rgb64)

            def timed(f):
                ms = []
                for _ in range(20):
                    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a0.record()
                    f()
                    a1.record()
                    a1.synchronize()
                    ms.append(a0.elapsed_time(a1))
                return statistics.median(ms), min(ms), max(ms)

            px = B * Ho * Wo
            d_ms, k_ms = timed(lambda: tail.yuv_to_rgb(e, y64, fmt, out=scratch_rgb)), timed(lambda: tail.rgb_to_yuv(e, rgb64, fmt, keep=back))
            launches = {"frames": B, "yuv_to_rgb": {"ms": round(d_ms[0], 4), "min_max_ms": [round(d_ms[1], 4), round(d_ms[2], 4)], "bytes": px * 9 // 2,
                                                     "TBps": round(px * 4.5 / d_ms[0] / 1e9, 3)},
                        "rgb_to_yuv_keep": {"ms": round(k_ms[0], 4), "min_max_ms": [round(k_ms[1], 4), round(k_ms[2], 4)], "bytes": px * 6,
                                            "TBps": round(px * 6 / k_ms[0] / 1e9, 3)},
                        "share_of_blocks_kept_in_the_first_step": round(kept_blocks, 4)}

    med = {k: statistics.median(v) for k, v in t.items()}
    fps = {k: N / med[k] * 1e3 for k in med}
    step_bytes = B * Ho * Wo * 3
    line = {
        "workload": f"{N} host frames of {Ho}x{Wo}, one face each, {B} per step, masks on the device, identity slots: upload -> crop -> stage A -> "
                    "generator -> SoftErosion -> in-place paste-back -> download",
        "frames": N, "batch": B, "steps_per_pass": len(plan), "repetitions": reps, "statistic": "median of passes, alternated on the same box",
        "pass_ms": {k: round(v, 2) for k, v in med.items()}, "pass_min_max_ms": {k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
        "step_ms": {k: round(v / len(plan), 3) for k, v in med.items()}, "frames_per_s": {k: round(v, 2) for k, v in fps.items()},
        "ratio_a_over_c": {k: round(fps[k] / fps["c_chain_device_resident_prefetched"], 4) for k in staging},
        "ratio_a_over_b": {k: round(fps[k] / fps["b_synchronous_loop"], 4) for k in staging},
        "bytes_per_step": {"frames_up": step_bytes, "frames_down": step_bytes, "masks_up": 0, "total": 2 * step_bytes},
        "link_GBps_at_the_measured_rate": {k: round((1 if fmt in k else 2) * step_bytes / (med[k] / len(plan)) / 1e6, 2) for k in staging},
        "host_staging_ms_per_batch": {k: round(statistics.median(v), 3) for k, v in staging.items()},
        "stage_ms_per_step_traced_pass": stages,
        "driver_equals_loop_bytes": same,
        **({} if fmt == "rgb24" else {"pixel_format": fmt, "bytes_per_step_" + fmt: {"frames_up": step_bytes // 2, "frames_down": step_bytes // 2,
                                                                                      "total": step_bytes},
                                      "conversion_launches_one_step": launches}),
        "torch_intra_op_threads": torch.get_num_threads(),
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    if not same:
        raise SystemExit("the driver's frames differ from the synchronous loop's")


if __name__ == "__main__":
    main()
