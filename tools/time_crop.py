"""Timing of the crop on the device (cs_crop_frames; tail.crop_frames, chain.crop) on one MI355X; prints one JSON line.

    python tools/time_crop.py [--batch 64] [--size 1080x1920] [--reps 24] [--chain-reps 20] [--out FILE]

B frames of the given size resident in HBM, 512 x 512 crops about seeded face-like landmarks (rolled, CropConfig's parameters), every shape
warmed, profiler off.  In ONE process, the candidates alternating repetition by repetition (so that clock and temperature drift hits them
alike), each repetition a host clock around calls that end in a synchronise; the figure of a candidate is the MEDIAN of its repetitions:
  * cs_crop_frames without and with I_out (the fused staging);
  * what the library offered before for the same bytes on the device: B calls of cs_warp_affine_u8 (one per frame) without and with one
    cs_prepare_crops behind them, through the C entry points with every argument prepared ahead (no tensor is allocated in the timed loop);
  * FrameChain with the crop in front (chain.crop on the frames, then the chain on its crops and matrices: the landmark geometry on the host
    is inside the timing) beside the chain alone on resident crops.
The bandwidth figure is the algorithmic bytes - crop (and I) written, the source footprint (dsize / s)^2 x 3 read once, s the matrix's
scale - over the median time.  Needs a GPU: the engine raises without one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from canonswap_amd import crop, synth, tail
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from canonswap_amd.engine import _ptr


def face(r, centre, width, roll):
    """106 float32 landmarks of a face `width` pixels wide about `centre`: a cloud in the face's ellipse, eyes and lips where the layout reads them."""
    rad, ang = np.sqrt(r.uniform(0, 1, 106)), r.uniform(0, 2 * np.pi, 106)
    p = np.stack([0.5 * width * rad * np.cos(ang), 0.65 * width * rad * np.sin(ang)], axis=1)
    left, right, lips = crop.EYE_LIP_POINTS[106]
    for idx, (x, y) in ((left, (-0.22, -0.2)), (right, (0.22, -0.2)), (lips[:1], (-0.17, 0.35)), (lips[1:], (0.17, 0.35))):
        for i in idx:
            p[i] = np.array([x, y]) * width + r.uniform(-0.03, 0.03, 2) * width
    c, s = np.cos(roll), np.sin(roll)
    return (p @ np.array([[c, s], [-s, c]]) + np.asarray(centre)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions per kernel candidate (>= 20), 4 calls each")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, dsize = a.batch, 512
    Ho, Wo = (int(v) for v in a.size.lower().split("x"))
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    r = np.random.Generator(np.random.PCG64(2024))
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    lmk = np.stack([face(r, (r.uniform(0.3, 0.7) * Wo, r.uniform(0.35, 0.65) * Ho), r.uniform(0.1, 0.16) * Wo, r.uniform(-0.5, 0.5)) for _ in range(B)])
    M_o2c, M_c2o, _ = crop.crop_matrices(lmk)
    scales = np.hypot(M_o2c[:, 0, 0], M_o2c[:, 0, 1]).astype(np.float64)
    crops, crops_p = (torch.empty((B, dsize, dsize, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    I, I_p = (torch.empty((B, 3, 256, 256), dtype=torch.float32, device=dev) for _ in range(2))

    # the parent's calls, every argument prepared ahead
    m6 = np.ascontiguousarray(M_o2c.astype(np.float64).reshape(B, 9)[:, :6])
    d6 = C.POINTER(C.c_double)
    rows = [(C.c_void_p(frames[b].data_ptr()), C.cast(m6[b].ctypes.data, d6), C.c_void_p(crops_p[b].data_ptr())) for b in range(B)]

    def parent(with_I):
        st = e._stream().cuda_stream
        for f, m, c in rows:
            if e.lib.cs_warp_affine_u8(e.h, f, Ho, Wo, m, c, dsize, dsize, st):
                raise RuntimeError("cs_warp_affine_u8")
        if with_I and e.lib.cs_prepare_crops(e.h, B, _ptr(crops_p), dsize, dsize, _ptr(I_p), st):
            raise RuntimeError("cs_prepare_crops")

    NP = 4                                                              # calls per repetition (sub-millisecond kernels)
    kern = {
        "crop": lambda: tail.crop_frames_M(e, frames, M_o2c, dsize, out=crops),
        "crop_I": lambda: tail.crop_frames_M(e, frames, M_o2c, dsize, out=crops, out_I=I),
        "parent": lambda: parent(False),
        "parent_I": lambda: parent(True),
    }
    with torch.cuda.device(dev):
        for f in kern.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(crops, crops_p)) and bool(torch.equal(I, I_p))
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

    # FrameChain: alone on resident crops, and with the crop in front
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    masks = torch.from_numpy((((xx - 256) / 170) ** 2 + ((yy - 250) / 200) ** 2 <= 1).astype(np.uint8)).to(dev)[None].expand(B, -1, -1).contiguous()
    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = FrameChain(sw)
    smooth = synth.make_smooth_images(B, seed=2100, size=512)
    res_crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)

    def chain_alone():
        chain(res_crops, masks, M_c2o, frames, idv, out=outf)

    def chain_with_crop():
        c = chain.crop(frames, lmk, out=crops)
        chain(c["crops"], masks, c["M_c2o"], frames, idv, out=outf)

    ch = {"chain": chain_alone, "crop_chain": chain_with_crop}
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
    t0 = time.perf_counter()
    for _ in range(20):
        crop.crop_matrices(lmk)
    host_ms = (time.perf_counter() - t0) / 20 * 1e3

    bytes_crop = B * dsize * dsize * 3
    bytes_I = B * 3 * 256 * 256 * 4
    bytes_src = float(((dsize / scales) ** 2 * 3).sum())
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    line = {
        "workload": f"crop_image's image step (crop.py:429-455 per frame, cropper.py:196-209) for {B} uint8 {Ho}x{Wo} frames resident in HBM -> "
                    f"{dsize}x{dsize} uint8 crops about seeded 106-point landmarks (scale 2.3, vy_ratio -0.125, rolled), optionally the "
                    "256x256 fp32 NCHW input of the motion extractor from the same launch",
        "batch": B, "size": f"{Ho}x{Wo}", "dsize": dsize, "repetitions": len(t["crop"]), "calls_per_repetition": NP, "statistic": "median",
        "matrix_scale_min_max": [round(float(scales.min()), 4), round(float(scales.max()), 4)],
        "crop_ms": round(med["crop"], 4), "crop_I_ms": round(med["crop_I"], 4),
        "parent_64_warps_ms": round(med["parent"], 4), "parent_64_warps_plus_prepare_ms": round(med["parent_I"], 4),
        "crop_over_parent": round(med["crop"] / med["parent"], 4), "crop_I_over_parent_plus_prepare": round(med["crop_I"] / med["parent_I"], 4),
        "same_bytes_as_parent": same,
        "min_max_ms": {k: spread(v) for k, v in t.items()},
        "algorithmic_bytes": {"crops_written": bytes_crop, "I_written": bytes_I, "source_footprint_read": round(bytes_src)},
        "crop_GBps": round((bytes_crop + bytes_src) / med["crop"] / 1e6, 1),
        "crop_I_GBps": round((bytes_crop + bytes_I + bytes_src) / med["crop_I"] / 1e6, 1),
        "chain": {"repetitions": len(tc["chain"]), "chain_alone_ms_per_step": round(medc["chain"], 3), "crop_then_chain_ms_per_step": round(medc["crop_chain"], 3),
                  "chain_alone_frames_per_s": round(B / medc["chain"] * 1e3, 2), "crop_then_chain_frames_per_s": round(B / medc["crop_chain"] * 1e3, 2),
                  "ratio": round(medc["chain"] / medc["crop_chain"], 4), "host_crop_matrices_ms_per_batch": round(host_ms, 3),
                  "min_max_ms": {k: spread(v) for k, v in tc.items()}},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
