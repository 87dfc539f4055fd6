"""Timing of the SegFormer face parser on the engine (cs_parser; csrc/parser.hip) on one MI355X beside the installed transformers class on the same
device, eager fp32 (what the reference runs) and fp16; prints one JSON line.

    python tools/time_parser.py [--reps 20] [--out profiles/parser_b64.json] [--no-chain]

Full MiT-b5 geometry (synth.MIT_B5) with synthetic weights, 512 x 512 pixel_values resident in HBM, B = 1 and B = 64.  All candidates warmed, in ONE
process; they alternate repetition by repetition, each repetition is a few calls inside a host clock that ends in a synchronise; the MEDIAN is
reported with the spread.  Per kernel family: device time of one cs_parser call from torch.profiler's kernel records (a separate, profiled call;
"not measured" where the profiler does not see the library's launches), and the token GEMM's achieved TFLOP/s from its share.  Then FrameChain's
64-frame step fed with ready logits, with parse=True in-line, and with parse=True and prefetch.  No ratio is fixed in advance."""
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
import parser_ref as R

FAMILIES = (("gemm", "p_gemm_kernel"), ("attention", "p_attn_kernel"), ("layernorm", "p_ln_kernel"), ("dwconv_gelu", "p_dwgelu_kernel"),
            ("conv", "id_conv_kernel"), ("head_upadd", "p_upadd_kernel"), ("input", "p_input_kernel"))


def gemm_macs(cfg, H, W):
    """Multiply-adds of the token GEMMs of one image (executed form: composed head, classifier padded to 64 rows)."""
    nk, n = (H // 32) * (W // 32), 0
    for s, (d, c) in enumerate(zip(cfg["depths"], cfg["widths"])):
        t = (H >> (s + 2)) * (W >> (s + 2))
        n += d * (t * c * c * 2 + nk * c * 2 * c + 2 * t * c * cfg["mlp"] * c) + t * c * cfg["D"]
    return n + (H // 4) * (W // 4) * cfg["D"] * 64


def median_ms(cands, reps, calls, dev):
    for f in cands.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in cands}
    for _ in range(reps):
        for k, f in cands.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize(dev)
            t[k].append((time.perf_counter() - t0) / calls * 1e3)
    return {k: {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]} for k, v in t.items()}


def families(fn, dev):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn(); torch.cuda.synchronize(dev)
        out = {k: 0.0 for k, _ in FAMILIES}
        for ev in prof.events():
            if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
                for k, pat in FAMILIES:
                    if pat in ev.name:
                        out[k] += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
        if sum(out.values()) <= 0:
            return "not measured (the profiler saw no kernel of the library)"
        return {k: round(v / 1e3, 4) for k, v in out.items()}
    except Exception as ex:          # a measurement aid: never the reason a timing run fails
        return f"not measured ({type(ex).__name__}: {ex})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    cfg = dict(synth.MIT_B5)
    psd = synth._segformer(0, cfg)
    heads = {"num_attention_heads": list(cfg["heads"])}
    sds = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
    sw = can_swapper(None, state_dicts=sds, max_batch=64, parser=(synth.to_torch({"p": psd})["p"], heads))
    e = sw.engine
    dev = e.device
    hf32 = R.hf_model(psd, cfg, torch.float32).to(dev)
    hf16 = R.hf_model(psd, cfg, torch.float16).to(dev)
    res = {}
    for B in (1, 64):
        x = torch.from_numpy(synth.make_parser_inputs(B, seed=4700)).to(dev)
        x16 = x.half()
        out = torch.empty((B, cfg["L"], 128, 128), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), torch.no_grad():
            cand = {"engine": lambda: e.parser(x, out=out), "torch_fp32": lambda: hf32(pixel_values=x).logits, "torch_fp16": lambda: hf16(pixel_values=x16).logits}
            err = float(R.rel_l2(cand["engine"](), cand["torch_fp32"]()).max())
            r = median_ms(cand, max(5, a.reps if B == 1 else a.reps // 2), 4 if B == 1 else 1, dev)
            fam = families(cand["engine"], dev)
        rec = {k: v for k, v in r.items()}
        rec["max_rel_l2_engine_vs_torch_fp32"] = err
        rec["kernel_family_ms"] = fam
        fl = 2.0 * gemm_macs(cfg, 512, 512) * B
        rec["gemm_flop"] = fl
        if isinstance(fam, dict) and fam["gemm"] > 0:
            rec["gemm_TFLOPs"] = round(fl / fam["gemm"] / 1e9, 2)
        rec["engine_TFLOPs_all_gemm_flop_over_whole_call"] = round(fl / r["engine"]["ms"] / 1e9, 2)
        res[f"b{B}"] = rec
    if not a.no_chain:
        from canonswap_amd.chain import FrameChain
        B = 64
        rng = np.random.Generator(np.random.PCG64(1))
        crops = [torch.from_numpy(np.ascontiguousarray((synth.make_smooth_images(B, seed=4800 + k, size=512).transpose(0, 2, 3, 1) * 255).astype(np.uint8))).to(dev)
                 for k in range(2)]
        ori = torch.from_numpy(rng.integers(0, 256, size=(B, 720, 1280, 3), dtype=np.uint8)).to(dev)
        M = np.tile(np.array([[0.5, 0, 300.0], [0, 0.5, 100.0], [0, 0, 1]], np.float64), (B, 1, 1))
        sid = torch.from_numpy(synth.make_identity(7)).to(dev)
        chain = FrameChain(sw)
        with torch.cuda.device(dev):
            lg = [e.parser(chain.parser_input(c)).clone() for c in crops]
            state = {"k": 0}

            def ready():
                chain(crops[0], None, M, ori, sid, logits=lg[0])

            def inline():
                chain(crops[0], None, M, ori, sid, parse=True)

            def prefetched():          # steady state: the next batch is staged on the side stream while this one runs
                k = state["k"]
                if not chain._pending:
                    chain.prefetch(crops[k], parse=True)
                chain.prefetch(crops[1 - k], parse=True)
                chain(crops[k], None, M, ori, sid, parse=True)
                state["k"] = 1 - k

            res["chain_b64_step"] = median_ms({"ready_logits": ready, "parse_inline": inline}, max(5, a.reps // 2), 1, dev)
            res["chain_b64_step"].update(median_ms({"parse_prefetch": prefetched}, max(5, a.reps // 2), 1, dev))
            chain.drop_prefetches()
    line = {
        "workload": "SegFormer face parser (MiT-b5 geometry, synthetic weights) on B 512x512 pixel_values resident in HBM: cs_parser beside transformers' "
                    "SegformerForSemanticSegmentation on the same device (eager fp32, fp16); FrameChain's 64-frame step with and without the parser",
        "repetitions": a.reps, "statistic": "median", **res, "device": torch.cuda.get_device_name(dev),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
