"""Timing of the face detector's input and decode on the device (cs_det_input, cs_det_decode; canonswap_amd/detect.py) on one MI355X; prints one
JSON line.

    python tools/time_detect.py [--batch 64] [--reps 24] [--host-reps 2] [--chain-reps 20] [--out profiles/detect_b64.json]

B uint8 frames of 1080 x 1920 resident in HBM -> the 640 x 640 blob, and B frames of 16 800 anchors (three levels, two anchors; a few faces of
some dozens of candidates each, tests/detect_ref.py's synthetic outputs) -> faces; every shape warmed, profiler off, all in ONE process:
  * each launch alone: repetitions of 4 calls, a host clock around calls that end in a synchronise, the MEDIAN of the repetitions; cs_det_input also
    in TB/s over the bytes read plus written (frames once, blob once);
  * beside the numpy restatement (tests/detect_ref.py: the reference's lines) on one host thread, on data already on the host;
  * beside the same lines written with torch ops on the same device: F.interpolate (bilinear, antialias off) + pad + normalize for the input
    - the nearest torch has, not bit-equal to cv2 - and threshold, gather, sort and the reference's greedy NMS loop per frame for the decode;
  * FrameChain's B-face step with and without the two launches in front, alternating repetition by repetition.
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
import torch.nn.functional as F

import detect_ref as DR
from canonswap_amd import detect, synth
from canonswap_amd.can_swap_e2e import can_swapper
from canonswap_amd.chain import FrameChain
from chain_helpers import _masks

FACES = [((60, 80, 130, 170), 0.95), ((300, 90, 360, 160), 0.9), ((420, 200, 500, 300), 0.85), ((150, 250, 200, 310), 0.8)]
STRIDES, NA = (8, 16, 32), 2


def torch_input(frames, nh, nw, Hd, Wd):
    x = frames.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False).round_().clamp_(0, 255)
    x = F.pad(x, (0, Wd - nw, 0, Hd - nh))
    return ((x - 127.5) * (1.0 / 128.0)).flip(1).contiguous()


def torch_decode(outs, centres, scale, thr=0.5, nms_thr=0.4):
    """scrfd.py:160-218, :239-253, :275-303 in torch ops on the device, frame by frame as the reference runs them."""
    res = []
    for f in range(outs[0].shape[0]):
        S, B = [], []
        for l, s in enumerate(STRIDES):
            score = outs[l][f, :, 0]
            pos = torch.nonzero(score >= thr)[:, 0]
            bb = outs[3 + l][f] * s
            c = centres[l]
            box = torch.stack([c[:, 0] - bb[:, 0], c[:, 1] - bb[:, 1], c[:, 0] + bb[:, 2], c[:, 1] + bb[:, 3]], dim=-1)
            S.append(score[pos]); B.append(box[pos])
        score, box = torch.cat(S), torch.cat(B) / scale
        order = torch.argsort(score, descending=True)
        box, score = box[order], score[order]
        areas = (box[:, 2] - box[:, 0] + 1) * (box[:, 3] - box[:, 1] + 1)
        idx = torch.arange(len(score), device=score.device)
        keep = []
        while idx.numel() > 0:
            i = idx[0]
            keep.append(i)
            r = idx[1:]
            w = (torch.minimum(box[i, 2], box[r, 2]) - torch.maximum(box[i, 0], box[r, 0]) + 1).clamp_(min=0)
            h = (torch.minimum(box[i, 3], box[r, 3]) - torch.maximum(box[i, 1], box[r, 1]) + 1).clamp_(min=0)
            inter = w * h
            idx = r[inter / (areas[i] + areas[r] - inter) <= nms_thr]
        k = torch.stack(keep) if keep else idx
        res.append(torch.cat([box[k], score[k, None]], dim=1))
    return res


def timed(fn, reps, calls, dev):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        t.append((time.perf_counter() - t0) / calls * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24, help="timed repetitions of a launch (>= 20), 4 calls each")
    ap.add_argument("--host-reps", type=int, default=2, help="timed repetitions of the numpy restatement")
    ap.add_argument("--chain-reps", type=int, default=20, help="timed repetitions per chain candidate (>= 20), one step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, Ho, Wo, size = a.batch, 1080, 1920, (640, 640)
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=B)
    e, dev = sw.engine, sw.engine.device
    nh, nw, scale = detect.det_geometry(Ho, Wo, size)
    frames = torch.randint(0, 256, (B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    blob = torch.empty((B, 3, size[1], size[0]), dtype=torch.float32, device=dev)
    per_frame = [DR.synth_outputs(size, 3, FACES[: 1 + f % len(FACES)], 6000 + f) for f in range(min(B, 8))]
    outs_np = DR.stack_frames([per_frame[f % len(per_frame)] for f in range(B)])
    outs = [torch.from_numpy(o).to(dev) for o in outs_np]
    cand = [sum(int((o[f] >= np.float32(0.5)).sum()) for o in outs_np[:3]) for f in range(B)]
    centres = [torch.from_numpy(c.astype(np.float32)).to(dev) for _, c in DR.anchors(size, 3)]
    reps = max(20, a.reps)

    cand_fn = {
        "det_input": lambda: detect.det_input(e, frames, size, out=blob),
        "det_input_torch": lambda: torch_input(frames, nh, nw, size[1], size[0]),
        "det_decode": lambda: detect.det_decode(e, outs, size, scale, (Ho, Wo)),
        "det_decode_torch": lambda: torch_decode(outs, centres, scale),
    }
    t = {}
    with torch.cuda.device(dev):
        for k, fn in cand_fn.items():
            fn(); fn()
            t[k] = timed(fn, reps if "torch" not in k or "input" in k else 5, 4 if "decode_torch" not in k else 1, dev)
    med = {k: statistics.median(v) for k, v in t.items()}
    faces = [len(d) for d in detect.det_decode(e, outs, size, scale, (Ho, Wo))[0]]

    host = {"det_input_numpy": [], "det_decode_numpy": []}
    frames_np = frames.cpu().numpy()
    torch.set_num_threads(1)
    for _ in range(max(1, a.host_reps)):
        t0 = time.perf_counter()
        want_blob = DR.letterbox_blob(frames_np, size)
        t1 = time.perf_counter()
        want = DR.decode_frames(outs_np, size, scale, (Ho, Wo))
        t2 = time.perf_counter()
        host["det_input_numpy"].append((t1 - t0) * 1e3); host["det_decode_numpy"].append((t2 - t1) * 1e3)
    medh = {k: statistics.median(v) for k, v in host.items()}
    detect.det_input(e, frames, size, out=blob)
    blob_differs = int((blob.cpu().numpy().view(np.uint32) != want_blob.view(np.uint32)).sum())
    got = detect.det_decode(e, outs, size, scale, (Ho, Wo))
    det_differs = sum(int(not np.array_equal(g.view(np.uint32), w.view(np.uint32))) for g, w in zip(got[0], want[0]))

    idv = torch.from_numpy(synth.make_identity(7)).to(dev)
    chain = FrameChain(sw)
    smooth = synth.make_smooth_images(B, seed=2100, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
    masks = torch.from_numpy(_masks(8)).repeat((B + 7) // 8, 1, 1)[:B].contiguous().to(dev)
    th, sc = 0.1, 0.9
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), 0.35 * Wo], [sc * np.sin(th), sc * np.cos(th), 0.2 * Ho], [0, 0, 1]], np.float64)
    M_c2o = np.stack([M] * B)
    outf = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)

    def chain_alone():
        chain(crops, masks, M_c2o, frames, idv, out=outf)

    def chain_with():
        detect.det_input(e, frames, size, out=blob)
        detect.det_decode(e, outs, size, scale, (Ho, Wo))
        chain(crops, masks, M_c2o, frames, idv, out=outf)

    ch = {"chain_alone": chain_alone, "chain_with_detect": chain_with}
    with torch.cuda.device(dev):
        for fn in ch.values():
            fn(); fn()
        tc = {k: [] for k in ch}
        for _ in range(max(20, a.chain_reps)):
            for k, fn in ch.items():
                tc[k] += timed(fn, 1, 1, dev)
    medc = {k: statistics.median(v) for k, v in tc.items()}

    nbytes = B * Ho * Wo * 3 + B * 3 * size[0] * size[1] * 4
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    line = {
        "workload": f"SCRFD's letterbox + blob (scrfd.py:224-235, 154) of {B} uint8 frames of {Ho}x{Wo} -> ({B},3,{size[1]},{size[0]}) fp32, and its decode + NMS "
                    f"(scrfd.py:160-218, 239-303) of {B} frames of 16800 anchors, all resident in HBM",
        "batch": B, "statistic": "median", "calls_per_repetition": 4,
        "det_input": {"ms": round(med["det_input"], 4), "min_max_ms": spread(t["det_input"]), "repetitions": len(t["det_input"]),
                      "bytes_read_plus_written": nbytes, "TBps": round(nbytes / med["det_input"] / 1e9, 3),
                      "torch_ops_ms": round(med["det_input_torch"], 4), "torch_over_launch": round(med["det_input_torch"] / med["det_input"], 2),
                      "numpy_one_thread_ms": round(medh["det_input_numpy"], 1), "numpy_over_launch": round(medh["det_input_numpy"] / med["det_input"], 1),
                      "values_differing_from_numpy": blob_differs},
        "det_decode": {"ms": round(med["det_decode"], 4), "min_max_ms": spread(t["det_decode"]), "repetitions": len(t["det_decode"]),
                       "includes": "the wrapper's D2H of det / kps / count", "candidates_per_frame_min_max": [min(cand), max(cand)],
                       "faces_per_frame_min_max": [min(faces), max(faces)],
                       "torch_ops_ms": round(med["det_decode_torch"], 3), "torch_repetitions": len(t["det_decode_torch"]),
                       "torch_over_launch": round(med["det_decode_torch"] / med["det_decode"], 1),
                       "numpy_one_thread_ms": round(medh["det_decode_numpy"], 1), "numpy_over_launch": round(medh["det_decode_numpy"] / med["det_decode"], 1),
                       "frames_differing_from_numpy": det_differs},
        "chain": {"repetitions": len(tc["chain_alone"]), "chain_alone_ms_per_step": round(medc["chain_alone"], 3),
                  "chain_with_detect_ms_per_step": round(medc["chain_with_detect"], 3),
                  "ratio": round(medc["chain_alone"] / medc["chain_with_detect"], 4), "min_max_ms": {k: spread(v) for k, v in tc.items()}},
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
