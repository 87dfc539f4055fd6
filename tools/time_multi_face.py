"""Timing of several faces per frame (cs_crop_faces, cs_paste_back_faces; FrameChain with frame_index) on one MI355X; prints one JSON line.

    python tools/time_multi_face.py [--frames 32] [--size 1080x1920] [--reps 24] [--chain-reps 20] [--out FILE]

F frames of the given size resident in HBM with TWO faces each (B = 2 F faces, 512 x 512 crops, seeded face-like landmarks left and right of
the middle, CropConfig's parameters, rolled), every shape warmed, profiler off.  In ONE process, the candidates of a comparison alternating
repetition by repetition (clock and temperature drift hits them alike), each repetition a host clock around calls that end in a synchronise;
a candidate's figure is the MEDIAN of its repetitions.  Every C call has its arguments prepared ahead: no tensor is allocated in a timed loop.
  * two faces per frame: cs_paste_back_faces (one pass) against the route there was before: two cs_paste_back_batch calls over the F frames,
    the second face pasted into the first call's output;
  * one face per frame (B = F = 2 x frames): cs_paste_back_faces against cs_paste_back_batch;
  * cs_crop_faces against gathering the frames with index_select and cs_crop_frames on the copies;
  * FrameChain's step with frame_index (B faces into F frames) and without (B faces into B frames).
The bandwidth figure is the algorithmic bytes - every frame read once and written once, every crop byte and mask float read once - over the
median time.  Needs a GPU: the engine raises without one."""
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
from time_crop import face


def alternate(dev, cands, reps, calls):
    """{name: [ms per call]}: the candidates in turn, repetition by repetition, `calls` calls per repetition between two synchronises."""
    for f in cands.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in cands}
    for _ in range(max(20, reps)):
        for k, f in cands.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize(dev)
            t[k].append((time.perf_counter() - t0) / calls * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32, help="frames with two faces each")
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions per kernel candidate (>= 20), 4 calls each")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, dsize = a.frames, 512
    B = 2 * F
    Ho, Wo = (int(v) for v in a.size.lower().split("x"))
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e = sw.engine
    dev = e.device
    r = np.random.Generator(np.random.PCG64(2025))
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)          # the first F: the two-face frames; all B: one face each
    # face 2f left of the middle of frame f, face 2f + 1 right of it: their crops (2.3 face widths) overlap in some frames
    lmk = np.stack([face(r, (r.uniform(0.3, 0.45) * Wo if b % 2 == 0 else r.uniform(0.55, 0.7) * Wo, r.uniform(0.35, 0.65) * Ho), r.uniform(0.1, 0.16) * Wo,
                         r.uniform(-0.5, 0.5)) for b in range(B)])
    M_o2c, M_c2o, _ = crop.crop_matrices(lmk)
    fi2 = np.repeat(np.arange(F), 2).astype(np.int32)                                       # two faces per frame
    fi1 = np.arange(B, dtype=np.int32)                                                      # one face per frame
    crops = torch.randint(0, 256, (B, dsize, dsize, 3), dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:dsize, 0:dsize].astype(np.float32)
    soft = np.clip(1.25 - np.sqrt(((xx - 256) / 170) ** 2 + ((yy - 250) / 200) ** 2), 0, 1).astype(np.float32)      # 1 inside, a ramp to 0 at the rim
    masks = torch.from_numpy(soft).to(dev)[None].expand(B, -1, -1).contiguous()
    d6, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    m6 = lambda M: np.ascontiguousarray(np.asarray(M, np.float64).reshape(len(M), 9)[:, :6])
    st = lambda: e._stream().cuda_stream

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {e.lib.cs_last_error().decode()}")

    # ---- two faces per frame: one pass against two batched passes (first faces, then second faces into the first pass's output)
    first, second = np.arange(0, B, 2), np.arange(1, B, 2)
    cr_a, cr_b = crops[first].contiguous(), crops[second].contiguous()
    mk_a, mk_b = masks[first].contiguous(), masks[second].contiguous()
    mc_all, mc_a, mc_b = m6(M_c2o), m6(M_c2o[first]), m6(M_c2o[second])
    out_f, tmp, out_p = (torch.empty((F, Ho, Wo, 3), dtype=torch.uint8, device=dev) for _ in range(3))

    def faces2():
        ok(e.lib.cs_paste_back_faces(e.h, B, F, _ptr(crops), _ptr(masks), dsize, dsize, fi2.ctypes.data_as(ip), mc_all.ctypes.data_as(d6), _ptr(frames),
                                     _ptr(out_f), Ho, Wo, st()), "cs_paste_back_faces")

    def batches2():
        ok(e.lib.cs_paste_back_batch(e.h, F, _ptr(cr_a), _ptr(mk_a), dsize, dsize, mc_a.ctypes.data_as(d6), _ptr(frames), _ptr(tmp), Ho, Wo, st()),
           "cs_paste_back_batch")
        ok(e.lib.cs_paste_back_batch(e.h, F, _ptr(cr_b), _ptr(mk_b), dsize, dsize, mc_b.ctypes.data_as(d6), _ptr(tmp), _ptr(out_p), Ho, Wo, st()),
           "cs_paste_back_batch")

    # ---- one face per frame
    out1_f, out1_p = (torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev) for _ in range(2))

    def faces1():
        ok(e.lib.cs_paste_back_faces(e.h, B, B, _ptr(crops), _ptr(masks), dsize, dsize, fi1.ctypes.data_as(ip), mc_all.ctypes.data_as(d6), _ptr(frames),
                                     _ptr(out1_f), Ho, Wo, st()), "cs_paste_back_faces")

    def batch1():
        ok(e.lib.cs_paste_back_batch(e.h, B, _ptr(crops), _ptr(masks), dsize, dsize, mc_all.ctypes.data_as(d6), _ptr(frames), _ptr(out1_p), Ho, Wo, st()),
           "cs_paste_back_batch")

    # ---- the crop: the frame named per face against a gather of the frames
    mo_all = m6(M_o2c)
    cut_f, cut_p = (torch.empty((B, dsize, dsize, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    gathered = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    gi = torch.from_numpy(fi2).long().to(dev)

    def crop_faces():
        ok(e.lib.cs_crop_faces(e.h, B, F, _ptr(frames), Ho, Wo, fi2.ctypes.data_as(ip), mo_all.ctypes.data_as(d6), dsize, _ptr(cut_f), None, st()),
           "cs_crop_faces")

    def gather_crop():
        torch.index_select(frames[:F], 0, gi, out=gathered)
        ok(e.lib.cs_crop_frames(e.h, B, _ptr(gathered), Ho, Wo, mo_all.ctypes.data_as(d6), dsize, _ptr(cut_p), None, st()), "cs_crop_frames")

    NP = 4
    with torch.cuda.device(dev):
        t2 = alternate(dev, {"faces": faces2, "two_batches": batches2}, a.reps, NP)
        same2 = bool(torch.equal(out_f, out_p))
        t1 = alternate(dev, {"faces": faces1, "batch": batch1}, a.reps, NP)
        same1 = bool(torch.equal(out1_f, out1_p))
        tcut = alternate(dev, {"crop_faces": crop_faces, "gather_crop_frames": gather_crop}, a.reps, NP)
        same_cut = bool(torch.equal(cut_f, cut_p))

        # ---- FrameChain's step: B faces into F frames (frame_index) beside B faces into B frames
        hard = torch.from_numpy((soft > 0.5).astype(np.uint8)).to(dev)[None].expand(B, -1, -1).contiguous()
        idv = torch.from_numpy(synth.make_identity(7)).to(dev)
        chain = FrameChain(sw)
        smooth = synth.make_smooth_images(B, seed=2100, size=512)
        res_crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
        ch = {"frame_index": lambda: chain(res_crops, hard, M_c2o, frames[:F], idv, out=out_f, frame_index=fi2),
              "one_face_per_frame": lambda: chain(res_crops, hard, M_c2o, frames, idv, out=out1_f)}
        tch = alternate(dev, ch, a.chain_reps, 1)

    med = lambda t: {k: statistics.median(v) for k, v in t.items()}
    spread = lambda t: {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    m2, m1, mcut, mch = med(t2), med(t1), med(tcut), med(tch)
    face_bytes = B * dsize * dsize * (3 + 4)                                                # crop bytes and mask floats, read once
    frame_bytes = Ho * Wo * 3
    one_pass2, two_pass2, one_pass1 = 2 * F * frame_bytes + face_bytes, 4 * F * frame_bytes + face_bytes, 2 * B * frame_bytes + face_bytes
    line = {
        "workload": f"paste-back and crop of {B} faces, 512x512 crops about seeded 106-point landmarks (scale 2.3, vy_ratio -0.125, rolled), uint8 {Ho}x{Wo} "
                    f"frames resident in HBM: two faces in each of {F} frames, and one face in each of {B} frames",
        "faces": B, "frames_two_faces_each": F, "size": f"{Ho}x{Wo}", "dsize": dsize, "statistic": "median", "calls_per_repetition": NP,
        "repetitions": len(t2["faces"]),
        "two_faces_per_frame": {
            "paste_back_faces_ms": round(m2["faces"], 4), "two_paste_back_batch_ms": round(m2["two_batches"], 4),
            "faces_over_two_batches": round(m2["faces"] / m2["two_batches"], 4), "same_bytes": same2,
            "algorithmic_bytes": {"one_pass": one_pass2, "two_passes": two_pass2},
            "paste_back_faces_GBps": round(one_pass2 / m2["faces"] / 1e6, 1), "two_paste_back_batch_GBps": round(two_pass2 / m2["two_batches"] / 1e6, 1),
            "min_max_ms": spread(t2)},
        "one_face_per_frame": {
            "paste_back_faces_ms": round(m1["faces"], 4), "paste_back_batch_ms": round(m1["batch"], 4),
            "faces_over_batch": round(m1["faces"] / m1["batch"], 4), "same_bytes": same1, "algorithmic_bytes": one_pass1,
            "paste_back_faces_GBps": round(one_pass1 / m1["faces"] / 1e6, 1), "paste_back_batch_GBps": round(one_pass1 / m1["batch"] / 1e6, 1),
            "min_max_ms": spread(t1)},
        "crop": {
            "crop_faces_ms": round(mcut["crop_faces"], 4), "index_select_plus_crop_frames_ms": round(mcut["gather_crop_frames"], 4),
            "crop_faces_over_gather": round(mcut["crop_faces"] / mcut["gather_crop_frames"], 4), "same_bytes": same_cut,
            "gathered_frame_bytes_written_and_read_by_the_gather": 2 * B * frame_bytes, "min_max_ms": spread(tcut)},
        "chain": {
            "repetitions": len(tch["frame_index"]), "faces_per_step": B,
            "with_frame_index_ms_per_step": round(mch["frame_index"], 3), "one_face_per_frame_ms_per_step": round(mch["one_face_per_frame"], 3),
            "with_frame_index_faces_per_s": round(B / mch["frame_index"] * 1e3, 2), "one_face_per_frame_faces_per_s": round(B / mch["one_face_per_frame"] * 1e3, 2),
            "ratio": round(mch["frame_index"] / mch["one_face_per_frame"], 4), "min_max_ms": spread(tch)},
        "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
