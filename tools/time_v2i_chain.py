"""Timing of the v2i device-side frame (canonswap_amd/chain.py AnimateChain) on one MI355X; prints one JSON line.

    python tools/time_v2i_chain.py [--batch 64] [--size 1080x1920] [--rounds 4] [--steps 5] [--out FILE]

B driving crops of 512 x 512 resident in HBM into one source image, every shape warmed, profiler off, each timed block ended by a
synchronise.  In ONE process, alternating round by round (so that clock and temperature drift hits every candidate alike):
  * AnimateChain in-line and with prefetch(), and cs_animate_frames alone on the same key-points (bench.py's v2i_body workload);
  * cs_paste_back_shared against cs_paste_back_batch on B materialised copies of the image and of the soft mask (what a caller had to do
    before), same crops, same matrix.
Per-stage milliseconds of one in-line step come from the engine's HIP-event profile, taken after the timed rounds.  Needs a GPU: the
engine raises without one."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from canonswap_amd import synth, tail
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import AnimateChain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round and candidate (rounds x steps >= 20)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, R, K = a.batch, a.rounds, a.steps
    Ho, Wo = (int(v) for v in a.size.lower().split("x"))
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device

    def u8_crops(n, seed):
        smooth = synth.make_smooth_images(n, seed=seed, size=512)
        return torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)

    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    mask = torch.from_numpy((((xx - 256) / 170) ** 2 + ((yy - 250) / 200) ** 2 <= 1).astype(np.uint8)).to(dev)
    sc, th = 0.45 * Ho / 512.0, 0.1                                     # crop -> image: a face 0.45 of the image height
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), 0.35 * Wo], [sc * np.sin(th), sc * np.cos(th), 0.2 * Ho]])
    ori = torch.randint(0, 256, (Ho, Wo, 3), dtype=torch.uint8, device=dev)
    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = AnimateChain(sw)
    chain.set_source(u8_crops(1, 2000)[0], mask, M, ori, idv)
    st = chain.source_state()
    crops = u8_crops(B, 2100)
    crops_b = crops.clone()                                             # the "next" batch: another tensor object (prefetch matches by identity)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)

    def inline(n):
        for _ in range(n):
            chain(crops, out=outf)

    def piped(n):
        cur, nxt = crops, crops_b
        chain.prefetch(cur)
        for _ in range(n):
            chain.prefetch(nxt)
            chain(cur, out=outf)
            cur, nxt = nxt, cur
        chain.drop_prefetches()

    r0 = chain(crops, out=outf, keep=True)
    x_t, gen = r0["x_t"].clone(), r0["crops_out"].clone()
    gen_u8 = torch.empty(B, 512, 512, 3, dtype=torch.uint8, device=dev)

    def body(n):
        for _ in range(n):
            e.animate_frames(st["f_swap_can_2"], st["x_swap"], x_t, want_f32=False, want_u8=True, out_u8=gen_u8)

    # the parent's way of the same paste: B copies of the image, B copies of the soft mask (in the crop's frame), B matrices
    soft = tail.soft_erosion_frames(e, mask[None], chain.se.weight, chain.se.kernel_size, chain.se.threshold, chain.se.iterations)
    soft_b = soft.expand(B, -1, -1).contiguous()
    ori_b = ori[None].expand(B, -1, -1, -1).contiguous()
    Ms = np.repeat(M[None], B, 0)
    outb = torch.empty_like(outf)
    NP = 4                                                              # paste calls per timed step (sub-millisecond kernels)

    def paste_shared(n):
        for _ in range(n * NP):
            tail.paste_back_shared(e, gen, M, ori, st["mask_ori"], out=outf)

    def paste_batch(n):
        for _ in range(n * NP):
            tail.paste_back_batch(e, gen, soft_b, Ms, ori_b, out=outb)

    cands = {"inline": inline, "prefetch": piped, "body": body, "paste_shared": paste_shared, "paste_batch": paste_batch}
    for f in cands.values():                                            # warm every shape
        f(2)
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(outf, outb))                                # mask warped once vs per frame: the same bytes
    total = {k: 0.0 for k in cands}
    per_round = {k: [] for k in cands}
    for _ in range(R):
        for k, f in cands.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f(K)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            total[k] += dt
            per_round[k].append(dt)
    n = R * K
    # per-stage device time of one in-line step: HIP events around every launch, summed by stage
    tmp = tempfile.NamedTemporaryFile(suffix=".csv", delete=False); tmp.close()
    os.environ["CANONSWAP_PROFILE_CSV"] = tmp.name
    e.profile_begin()
    chain(crops, out=outf)
    e.profile_end()
    del os.environ["CANONSWAP_PROFILE_CSV"]
    stage = {"staging": 0.0, "motion_extractor": 0.0, "keypoints": 0.0, "body": 0.0, "paste": 0.0}
    with open(tmp.name) as f:
        for row in csv.DictReader(f):
            lab, ms = row["label"], float(row["ms"])
            key = ("staging" if lab == "prepare_crops" else "keypoints" if lab == "m_keypoints_driven" else "paste" if lab == "paste_back_shared" else
                   "motion_extractor" if (lab.startswith("M.") or lab.startswith("m_")) else "body")
            stage[key] += ms
    os.remove(tmp.name)
    ms_shared, ms_batch = total["paste_shared"] / (n * NP) * 1e3, total["paste_batch"] / (n * NP) * 1e3
    line = {
        "workload": f"v2i device-side frame, {B} driving frames per launch: uint8 512x512 crops in HBM -> INTER_AREA 256x256 + /255 -> motion extractor M -> "
                    f"driven key-points -> warp_decode of one swapped canonical volume -> paste-back into ONE {Ho}x{Wo} uint8 image "
                    "(can_swap_pipeline_v2i.py:223-238, 260-321 without its host round trips)",
        "batch": B, "size": f"{Ho}x{Wo}", "timed_steps": n, "frames": n * B,
        "value": round(n * B / total["inline"], 3), "unit": "frames/s", "ms_per_step": round(total["inline"] / n * 1e3, 3),
        "value_prefetch": round(n * B / total["prefetch"], 3), "ms_per_step_prefetch": round(total["prefetch"] / n * 1e3, 3),
        "body_alone_same_keypoints": round(n * B / total["body"], 3), "ms_per_step_body": round(total["body"] / n * 1e3, 3),
        "ratio_to_body": round(total["body"] / total["inline"], 4), "ratio_to_body_prefetch": round(total["body"] / total["prefetch"], 4),
        "stage_ms_per_step": {k: round(v, 3) for k, v in stage.items()},
        "paste": {"shared_ms": round(ms_shared, 4), "batch_on_B_copies_ms": round(ms_batch, 4), "shared_over_batch": round(ms_shared / ms_batch, 4),
                  "same_bytes": same, "calls_timed_each": n * NP,
                  "shared_GBps_written": round(B * Ho * Wo * 3 / ms_shared / 1e6, 1),
                  "copies_not_allocated_MB": round((B * Ho * Wo * 3 + B * 512 * 512 * 4) / 1e6, 1),
                  "per_round_ms": {k: [round(v / (K * NP) * 1e3, 4) for v in per_round[k]] for k in ("paste_shared", "paste_batch")}},
        "per_round_ms_per_step": {k: [round(v / K * 1e3, 3) for v in per_round[k]] for k in ("inline", "prefetch", "body")},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
