"""Timing of the crop and the paste-back from landmarks and matrices on the device (cs_crop_lmk, cs_paste_back_faces_dev; FrameChain's device
route) beside the host-matrix route they replace, on one MI355X; prints one JSON line.

    python tools/time_device_crop.py [--frames 64] [--size 1080x1920] [--reps 24] [--chain-reps 20] [--out profiles/device_crop_b64.json]

F frames of the given size resident in HBM with one face each (B = F faces, 512 x 512 crops, seeded 106-point landmarks ON THE DEVICE, as a
tracker leaves them; CropConfig's parameters, rolled), every shape warmed, profiler off.  In ONE process, the candidates of a comparison
alternating repetition by repetition, each repetition a host clock around calls that end in a synchronise; a candidate's figure is the MEDIAN
of its repetitions (tools/time_multi_face.py's scheme).  Every call goes through Engine._call, the package's one call path, for both candidates.
  * crop: cs_crop_lmk with I_out against the route it replaces: the landmarks downloaded, crop.crop_matrices on the host, cs_crop_faces with
    I_out; the host route's figure includes the download's wait and the numpy geometry, which is the point;
  * paste: cs_paste_back_faces_dev against cs_paste_back_faces on the same matrices (the device's float32 M_c2o widened to double);
  * FrameChain's step of B faces by both routes: chain.crop(frames, lmk on the device) -> chain(crops, masks, M, ..., status=) against the
    landmarks downloaded, chain.crop(frames, lmk on the host) -> chain(crops, masks, M_c2o, ...).
Needs a GPU: the engine raises without one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from canonswap_amd import crop, landmarks, synth
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from time_crop import face
from time_multi_face import alternate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames, one face each")
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions per kernel candidate (>= 20), 4 calls each")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = F = a.frames
    dsize, cfg = 512, dict(scale=2.3, vy_ratio=-0.125, flag_do_rot=True)
    Ho, Wo = (int(v) for v in a.size.lower().split("x"))
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    r = np.random.Generator(np.random.PCG64(2026))
    frames = torch.randint(0, 256, (F, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    lmk_np = np.stack([face(r, (r.uniform(0.3, 0.7) * Wo, r.uniform(0.35, 0.65) * Ho), r.uniform(0.1, 0.16) * Wo, r.uniform(-0.5, 0.5)) for _ in range(B)])
    lmk = torch.from_numpy(lmk_np.astype(np.float32)).to(dev)
    N = int(lmk.shape[1])
    layout = landmarks.layout_of(N)
    fi = np.arange(B, dtype=np.int32)
    ip, d6 = fi.ctypes.data_as(C.POINTER(C.c_int)), C.POINTER(C.c_double)
    m6 = lambda M: np.ascontiguousarray(np.asarray(M, np.float64).reshape(len(M), 9)[:, :6])

    # ---- the crop: landmarks on the device -> M, crops, I
    M = torch.empty((B, 18), dtype=torch.float32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    cut_d, cut_h = (torch.empty((B, dsize, dsize, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    I_d, I_h = (torch.empty((B, 3, 256, 256), dtype=torch.float32, device=dev) for _ in range(2))

    def crop_lmk():
        e._call("cs_crop_lmk", B, F, frames, Ho, Wo, ip, lmk, N, C.byref(layout), dsize, cfg["scale"], cfg["vy_ratio"], 1, 1, M, cut_d, I_d, None, status)

    def download_matrices_crop_faces():
        host = lmk.cpu().numpy()                                                            # waits for the device: the landmarks' producer
        M_o2c, _, _ = crop.crop_matrices(host, dsize=dsize, **cfg)
        mo = m6(M_o2c)
        e._call("cs_crop_faces", B, F, frames, Ho, Wo, ip, mo.ctypes.data_as(d6), dsize, cut_h, I_h)

    # ---- the paste: the same faces back into the frames
    crops = torch.randint(0, 256, (B, dsize, dsize, 3), dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:dsize, 0:dsize].astype(np.float32)
    soft = np.clip(1.25 - np.sqrt(((xx - 256) / 170) ** 2 + ((yy - 250) / 200) ** 2), 0, 1).astype(np.float32)      # 1 inside, a ramp to 0 at the rim
    masks = torch.from_numpy(soft).to(dev)[None].expand(B, -1, -1).contiguous()
    out_d, out_h = (torch.empty((F, Ho, Wo, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    with torch.cuda.device(dev):
        crop_lmk()
        torch.cuda.synchronize(dev)
    refused = int((status != 0).sum())
    mc = m6(M.cpu().numpy()[:, 9:].astype(np.float64).reshape(B, 3, 3))

    def paste_dev():
        e._call("cs_paste_back_faces_dev", B, F, crops, masks, dsize, dsize, ip, M, status, frames, out_d, Ho, Wo)

    def paste_host():
        e._call("cs_paste_back_faces", B, F, crops, masks, dsize, dsize, ip, mc.ctypes.data_as(d6), frames, out_h, Ho, Wo)

    NP = 4
    with torch.cuda.device(dev):
        tcut = alternate(dev, {"crop_lmk": crop_lmk, "host_route": download_matrices_crop_faces}, a.reps, NP)
        # the host route's float32 matrices come from numpy's BLAS / LAPACK, the device's from csrc/lmk_geometry.h: the crops may differ in a few bytes
        crop_bytes_differ = int((cut_d != cut_h).sum())
        tp = alternate(dev, {"dev": paste_dev, "host": paste_host}, a.reps, NP)
        same_paste = bool(torch.equal(out_d, out_h))

        # ---- FrameChain's step by both routes
        hard = torch.from_numpy((soft > 0.5).astype(np.uint8)).to(dev)[None].expand(B, -1, -1).contiguous()
        e.set_identity(torch.from_numpy(synth.make_identity(7)).reshape(1, 512).to(dev), 0)
        slots = [0] * B
        chain = FrameChain(sw)

        def step_dev():
            c = chain.crop(frames, lmk)
            chain(c["crops"], hard, c["M"], frames, slots=slots, out=out_d, status=c["status"])

        def step_host():
            c = chain.crop(frames, lmk.cpu().numpy())
            chain(c["crops"], hard, c["M_c2o"], frames, slots=slots, out=out_h)

        tch = alternate(dev, {"device_route": step_dev, "host_route": step_host}, a.chain_reps, 1)

    med = lambda t: {k: statistics.median(v) for k, v in t.items()}
    spread = lambda t: {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    mcut, mp, mch = med(tcut), med(tp), med(tch)
    paste_bytes = 2 * F * Ho * Wo * 3 + B * dsize * dsize * (3 + 4)
    line = {
        "workload": f"crop and paste-back of {B} faces, one in each of {F} uint8 {Ho}x{Wo} frames resident in HBM, 512x512 crops about seeded "
                    f"{N}-point landmarks on the device (scale 2.3, vy_ratio -0.125, rolled)",
        "faces": B, "frames": F, "size": f"{Ho}x{Wo}", "dsize": dsize, "statistic": "median", "calls_per_repetition": NP,
        "repetitions": len(tcut["crop_lmk"]), "faces_refused_by_the_guard": refused,
        "crop": {
            "crop_lmk_with_I_ms": round(mcut["crop_lmk"], 4), "download_crop_matrices_crop_faces_with_I_ms": round(mcut["host_route"], 4),
            "crop_lmk_over_host_route": round(mcut["crop_lmk"] / mcut["host_route"], 4), "crop_bytes_that_differ": crop_bytes_differ,
            "crop_bytes": int(cut_d.numel()), "min_max_ms": spread(tcut)},
        "paste": {
            "paste_back_faces_dev_ms": round(mp["dev"], 4), "paste_back_faces_ms": round(mp["host"], 4),
            "dev_over_host": round(mp["dev"] / mp["host"], 4), "same_bytes": same_paste, "algorithmic_bytes": paste_bytes,
            "paste_back_faces_dev_GBps": round(paste_bytes / mp["dev"] / 1e6, 1), "paste_back_faces_GBps": round(paste_bytes / mp["host"] / 1e6, 1),
            "min_max_ms": spread(tp)},
        "chain": {
            "repetitions": len(tch["device_route"]), "faces_per_step": B,
            "device_route_ms_per_step": round(mch["device_route"], 3), "host_route_ms_per_step": round(mch["host_route"], 3),
            "device_over_host": round(mch["device_route"] / mch["host_route"], 4), "min_max_ms": spread(tch)},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
