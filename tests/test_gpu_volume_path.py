"""F (engine.hip run_F / run_resblocks3d, pack._pack_F / _resblocks3d) and R (run_R / run_stage3_xf, pack._pack_R) launch by launch against float64,
on the engine's own routing, in both modes: what test_gpu_spade_decoder.py is for G.

cs_op_v_fill writes a 16-bit sentinel over the volume workspace and the statistics pool, cs_op_v_stop makes cs_extract_feature_3d / cs_refine return
after its n-th launch, cs_op_v_read copies a buffer out.  For every launch n the test fills, runs to n and looks at all ten buffers, the slot and
f_out: what launches 1 .. n write (plan_F / plan_R: a reading of run_F and of run_stage3_xf's pick() rotation, not the engine's) holds no sentinel on
any sample, everything else is still all sentinel, and against the run stopped at n - 1 only launch n's outputs have changed a bit.  The tensors
launch n wrote (sample 1 of the B = 3 call, sample 0 of the latency call: the same frame) are brought to the reference's layout and compared with
tests/volume_ref.py's float64 restatement of that step, computed from the tensors and the (mean, rstd) slot the engine's launch read and from the
unpacked state dicts - so pack._pack_F, _pack_R and _resblocks3d are checked too (test_volume_ref_cpu.py ties the restatement to the oracle).

Gates.  A conv launch, per output tensor, elementwise: half an fp16 spacing at |R| where it stores fp16, plus 4 x max |E32 - R|, E32 the same step
in torch fp32 on the CPU from the same operands (spade_ref.gate).  The elementwise GroupNorm launches - the xf_out write-back of conv1 of blocks 1
and 2 and the norm_act that closes a stage - by rounding counts (volume_ref.gn_gate: 6 x 2^-24 (|y sc| + |mean sc| + |beta| + |res|), 8 with the
second affine, half a spacing for the fp16 copy).  The layout launches and f_out: equal to the permutation, bit for bit.  Nothing is pinned from a
GPU run.

The geometry is compiled in (256 x 256 image, 64 x 64 x 16 x 32 volume).  B = 3 is the smallest batch on the batched routes (vol32 for the plain
volume convs: VOL32_MINB; 8-row statistics blocks), B = 1 the latency batch (v32_srows = 2, conv_lat for the 512-channel pair).  R's input is the
batched engine's own swap(warp(F(img))) of the frames: GroupNorm needs realistic magnitudes.

Rows: F stores 18 tensors (conv_first, two down blocks, two of F.second, two per fused ResBlock3d, f_out), R 32 (two of ncdhw_to_hwdc; per stage
conv1 and conv2 of three blocks, the xf_out of blocks 1 and 2, two of norm_act; three per 2-D block; f_out) and 12 statistics slots: 50 rows and 12
slots per mode (block 0 of a stage has no write-back; the closing norm_act has two outputs).

Measured 2026-10-20 on an MI355X (no gate; the table is in DESIGN.md section 5.10).  The largest fraction of its gate any step used is 1.00 in both
modes - every fp16 tensor has elements on a rounding tie, which use up the half spacing.  Beyond the half spacing (_row's "beyond"): batched F 0.38,
R 0.99 (R.rb2.0.c2's fp32 stream, 2.01e-06 against 2.03e-06: conv_halo's sequential fp32 accumulation over K = 4608 against an allowance of two
spacings of an fp32 near 10; the next is 0.66); latency F 0.38, R 0.48.  Slots: mean within 1.2e-7, rstd within 6.1e-8 relative.  f_out against the
chained float64 steps / the oracle, relative L2: F 2.46e-4 / 2.74e-4, R 1.52e-4 / 1.98e-4, in both modes."""
import os
import tempfile

import numpy as np
import pytest
import torch

import hip_ops as H
import spade_ref as S
import volume_ref as V

pytestmark = pytest.mark.gpu

MODES = ("batched", "latency")
ENTRIES = {"F": "cs_extract_feature_3d", "R": "cs_refine"}
SENT16 = H.G_SENTINEL
SENT32 = (SENT16 << 16) | SENT16
VS = (H.V_S0, H.V_S1, H.V_S2)
VA = (H.V_A0, H.V_A1)
FIN = "chan_stats_finish"


# ------------------------------------------------------------------------------------------------ a reading of run_F and run_R
def plan_F():
    """[(label, {key of volume_ref: buffer})] per launch of cs_extract_feature_3d, the same in both modes: the down blocks are 512 / 256
    workgroups and F.second has two outputs (never split-K), the fused ResBlock3d runs at every batch size.  Block i reads va[i & 1] and vs[cur] and
    writes vs[(cur + 1) % 3] and va[(i + 1) & 1]."""
    P = [("conv_first", {"t0": H.V_T0}), ("F.down0", {"p0": H.V_P0}), ("F.down1", {"p1": H.V_P1}), ("F.second", {"x.0": VS[0], "a.0": VA[0]})]
    for i in range(6):
        P.append((f"F.rb{i}.c1+c2", {f"x.{i + 1}": VS[(i + 1) % 3], f"a.{i + 1}": VA[(i + 1) & 1]}))
    return P + [("hwdc_to_ncdhw", {"f_out": "out"})]


def plan_R():
    """The same for cs_refine.  run_stage3_xf rotates five fp32 volumes, pool = (vs[0], vs[1], vs[2], vsp[0], vsp[1]), pick(busy) = the first not in
    busy: per block Xn = pick(X, pend_y) (block 0: X itself), Y1 = pick(X, pend_y, Xn), conv1 reads pend_y (and X) and writes Y1 (and Xn); X = Xn;
    Y2 = pick(X, Y1), conv2 reads Y1 and writes Y2 = the next pend_y.  norm_act writes the first vs that is neither X nor pend_y, and va[0].  The
    2-D pair: conv1 va[0] -> va[1], conv2 -> vs[(cur + 1) % 3] and va[0].  In latency mode conv_lat keeps the layer's label and no launch is
    split-K (conv1 of the pair is 256 workgroups of conv_lat; everything else has statistics, a residual or two outputs)."""
    P = [("ncdhw_to_hwdc", {"x.in": VS[0], "a.in": VA[0]})]
    pool = VS + (H.V_SP0, H.V_SP1)
    pick = lambda *busy: next(b for b in pool if b not in busy)

    def stage(s, cur):
        X = pend = VS[cur]
        for i in range(3):
            Xn = pick(X, pend) if i else X
            Y1 = pick(X, pend, Xn)
            w = {f"{s}.y1.{i}": Y1}
            if i:
                w[f"{s}.x.{i}"] = Xn
            P.extend([(f"R.{s}.{i}.c1.sp", w), (FIN, {f"{s}.st1.{i}": H.V_STATS})])
            X = Xn
            Y2 = pick(X, Y1)
            P.extend([(f"R.{s}.{i}.c2.sp", {f"{s}.y2.{i}": Y2}), (FIN, {f"{s}.st2.{i}": H.V_STATS})])
            pend = Y2
        nxt = next(k for k in range(3) if VS[k] not in (X, pend))
        P.append(("norm_act", {f"{s}.out": VS[nxt], f"{s}.a": VA[0]}))
        return nxt

    cur = stage("s1", 0)
    for i in range(3):
        P.append((f"R.rb2.{i}.c1", {f"rb2.h.{i}": VA[1]}))
        cur = (cur + 1) % 3
        P.append((f"R.rb2.{i}.c2", {f"rb2.x.{i + 1}": VS[cur], f"rb2.a.{i + 1}": VA[0]}))
    stage("s3", cur)
    return P + [("hwdc_to_ncdhw", {"f_out": "out"})]


PLANS = {"F": plan_F, "R": plan_R}


def test_the_rotation_never_writes_what_the_launch_reads():
    """plan_R's reading of pick(): the buffers are the ones worked out by hand for stage 1 (vs[0] in: y1 vs[1], y2 vs[2]; block 1 writes the stream
    to vs[1] and y1 to vsp[0], y2 to vs[0]; block 2 the stream to vs[2]; norm_act vs[1]), and only vsp[0] of the two split buffers is ever used"""
    P = dict(kv for _, w in plan_R() for kv in w.items())
    assert [P[k] for k in ("s1.y1.0", "s1.y2.0", "s1.x.1", "s1.y1.1", "s1.y2.1", "s1.x.2", "s1.y1.2", "s1.y2.2", "s1.out")] == \
        [H.V_S1, H.V_S2, H.V_S1, H.V_SP0, H.V_S0, H.V_S2, H.V_SP0, H.V_S0, H.V_S1]
    assert P["rb2.x.3"] == H.V_S1 and P["s3.y1.0"] == H.V_S0 and P["s3.out"] == H.V_S1 and H.V_SP1 not in P.values()
    assert len(plan_F()) == 11 and len(plan_R()) == 34
    assert sum(len(w) for _, w in plan_F()) == 18 and sum(len(w) for _, w in plan_R()) == 32 + 12


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def engines(state_dicts):
    from canonswap_amd import pack
    from canonswap_amd.engine import Engine
    blobs = pack.build_blobs(state_dicts)
    es = {"batched": Engine(0, max_batch=3), "latency": Engine(0, max_batch=1, latency_mode=True)}
    for e in es.values():
        e.load_blobs(blobs)
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def inputs(engines):
    """F's input: three synthetic frames; R's: the batched engine's swap(warp(F(img))) of them"""
    from canonswap_amd import synth
    e = engines["batched"]
    inp = synth.make_frame_inputs(3, seed=2300, size=256)
    img = torch.from_numpy(inp["img"]).cuda().contiguous()
    e.set_identity(torch.from_numpy(synth.make_identity(7)))
    f_can, _ = e.warp(e.extract_feature_3d(img), torch.from_numpy(inp["x_t"]).cuda(), torch.from_numpy(inp["x_can"]).cuda())
    return {"F": img, "R": e.swap(f_can).contiguous()}


def _labels(e, entry, x, out):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "launches.csv")
        old = os.environ.get("CANONSWAP_PROFILE_CSV")
        os.environ["CANONSWAP_PROFILE_CSV"] = path
        try:
            e.profile_begin()
            H.v_run(e, entry, x, out)
            e.profile_end()
        finally:
            if old is None:
                del os.environ["CANONSWAP_PROFILE_CSV"]
            else:
                os.environ["CANONSWAP_PROFILE_CSV"] = old
        return [l.split(",")[1] for l in open(path).read().splitlines()[1:]]


def _to_ref(t):
    """one sample of a buffer on the device, channels last ([H, W, C] or the HWDC volume [H, W, D, C]) -> the reference's [1, C, (D,) H, W] on the host"""
    t = t.permute(2, 0, 1) if t.dim() == 3 else t.permute(3, 2, 0, 1)
    return t.unsqueeze(0).contiguous().cpu()


def _sentinels(t):
    """where a buffer still holds the fill: per 16-bit value for fp16, per 32-bit value for fp32 (the lower half of a genuine fp32 may be anything)"""
    return t.view(torch.int16) == SENT16 if t.dtype == torch.float16 else t.view(torch.int32) == SENT32


def _trace(e, which, x, s):
    """Runs the entry point to each of its launches in turn.  Returns the launch list, per key what its launch wrote (sample s, the reference's
    layout; statistics as (mean, rstd)), the full run's f_out and the violations of the accounting."""
    B = x.shape[0]
    entry, plan = ENTRIES[which], PLANS[which]()
    out = torch.empty(B, 32, 16, 64, 64, device=x.device)
    labels = _labels(e, entry, x, out)
    full = out[s:s + 1].cpu()
    bufs = [{w: H.v_read(e, w, B) for w in range(11)} for _ in range(2)]
    written, cap, bad = set(), {}, []
    if labels != [l for l, _ in plan]:
        return dict(labels=labels, cap=cap, bad=[("the launch list is not the plan's",)], full=full)
    for n, (label, outs) in enumerate(plan, 1):
        scratch, prev = bufs[n & 1], bufs[~n & 1]
        H.v_fill(e, B)
        out.fill_(float("nan"))
        H.v_run(e, entry, x, out, stop=n)
        written |= set(outs.values())
        for w in range(11):
            cur = H.v_read(e, w, B, out=scratch[w])
            sent = _sentinels(cur)
            if w == H.V_STATS:      # [B][32][2] at the head of the slot handed out last, the rest of what is read as the fill left it
                head = sent.reshape(-1)[:B * 64]
                ok = bool(sent.all()) if w not in written else not bool(head.any()) and bool(sent.reshape(-1)[B * 64:].all())
            else:
                ok = bool(sent.all()) if w not in written else not bool(sent.any())
            if not ok:
                bad.append((n, label, H.V_NAMES[w] if w < 10 else "stats", "written" if w not in written else "sentinel left"))
            # the runs are deterministic: against the run that stopped one launch earlier, launch n changed its own outputs and nothing else
            if n > 1 and w not in outs.values() and not torch.equal(cur.view(torch.int16), prev[w].view(torch.int16)):
                bad.append((n, label, H.V_NAMES[w] if w < 10 else "stats", "changed by a launch that does not write it"))
        isn = torch.isnan(out)
        if not bool(~isn.any() if "f_out" in outs else isn.all()):
            bad.append((n, label, "f_out", "sentinel left" if "f_out" in outs else "written"))
        for key, w in outs.items():
            if w == "out":
                cap[key] = out[s:s + 1].cpu()
            elif w == H.V_STATS:
                v = scratch[w].reshape(-1)[:B * 64].view(B, 32, 2)[s].cpu()
                cap[key] = (v[:, 0].clone(), v[:, 1].clone())
            else:
                cap[key] = _to_ref(scratch[w][s])
    return dict(labels=labels, cap=cap, bad=bad, full=full)


@pytest.fixture(scope="module")
def traces(engines, inputs):
    out = {}
    for which, x in inputs.items():
        out[which, "batched"] = _trace(engines["batched"], which, x, 1)
        out[which, "latency"] = _trace(engines["latency"], which, x[1:2].contiguous(), 0)
    return out


@pytest.fixture(scope="module")
def vw(state_dicts):
    return V.VWeights(state_dicts["appearance_feature_extractor"], state_dicts["refine"])


class _Reads(dict):
    """a dict that notes the keys a step reads"""

    def __init__(self, *a):
        super().__init__(*a)
        self.seen = []

    def __getitem__(self, k):
        self.seen.append(k)
        return super().__getitem__(k)


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)


def _row(label, key, got, R, g, f16):
    """a row of the table; "beyond": the largest share of the gate's fp32 part an element needs once its half fp16 spacing is spent (among millions
    of fp16 values some sit on a rounding tie, so the whole gate of an fp16 tensor is always used up: this is the figure with headroom)"""
    fr, d, gt = S.used(got, R, g)
    flat = lambda t: t.reshape(1, -1, *t.shape[-2:])
    bd = S.breakdown(flat(got), flat(R), flat(g))
    h = 0.5 * S.spacing16(R) if f16 else torch.zeros_like(R)
    bd["beyond"] = (((got.double() - R).abs() - h) / (g - h)).clamp_min(0).max().item()
    return (label, key, fr, d, gt, bd)


def _exact(label, key, got, want):
    eq = got.dtype == want.dtype and torch.equal(got, want)
    return (label, key, 0.0 if eq else float("inf"), 0.0 if eq else float("nan"), 0.0,
            {"note": "equal to the permutation" if eq else "NOT the permutation", "beyond": 0.0 if eq else float("inf")})


@pytest.fixture(scope="module")
def reports(traces, vw, inputs):
    """Per (network, mode): a row per stored tensor (label, key, largest fraction of its gate used, |d| and gate there, the breakdown) and per
    statistics slot.  The float64 and fp32 references of a step are computed once where both modes hand it the same operands."""
    out, memo = {}, {}
    for which in ENTRIES:
        steps = V.step_list_F(vw) if which == "F" else V.step_list_R(vw)
        x = inputs[which][1:2].cpu()
        for mode in MODES:
            cap = traces[which, mode]["cap"]
            rows, stats = [], []
            missing = lambda label, key: (label, key, float("inf"), float("nan"), float("nan"), {"note": "not captured", "beyond": float("inf")})
            T = _Reads({"img": x} if which == "F" else {})
            if which == "R":
                for key, want in (("x.in", x), ("a.in", x.half())):
                    rows.append(_exact("ncdhw_to_hwdc", key, cap[key], want) if key in cap else missing("ncdhw_to_hwdc", key))
                    T[key] = cap.get(key)
            for i, e in enumerate(steps):
                if any(k not in cap for k in e["outs"]) or (e["st"] and e["st"] not in cap):
                    rows += [missing(e["label"], k) for k in e["outs"]]
                    continue
                if e["kind"] == "gn":
                    _, refs, gates = V.gn_step(e, T)
                    f16s = (False, True)[:len(refs)]
                else:
                    hit = memo.get((which, i))
                    if hit and all(_same(T[k], v) for k, v in hit[0].items()):
                        Rs, Es = hit[1], hit[2]
                    else:
                        T.seen = []
                        Rs, Es = e["fn"](T, torch.float64), e["fn"](T, torch.float32)
                        memo[which, i] = ({k: dict.__getitem__(T, k) for k in set(T.seen)}, Rs, Es)
                    refs, gates, f16s = Rs, [S.gate(r, x32, f) for r, x32, f in zip(Rs, Es, e["f16"])], e["f16"]
                for k, r, g, f in zip(e["outs"], refs, gates, f16s):
                    rows.append(_row(e["label"], k, cap[k], r, g, f))
                    T[k] = cap[k]
                if e["st"]:
                    T[e["st"]] = cap[e["st"]]
                    stats.append((e["label"], cap[e["st"]], V.vol_stats(cap[e["outs"][0]].double())))
            last = "x.6" if which == "F" else "s3.out"
            rows.append(_exact("hwdc_to_ncdhw", "f_out", cap["f_out"], cap[last]) if "f_out" in cap and last in cap else missing("hwdc_to_ncdhw", "f_out"))
            out[which, mode] = dict(rows=rows, stats=stats)
    return out


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(ENTRIES))
def test_launch_list(traces, which, mode):
    """The profile CSV's labels of the entry point equal the list read off run_F / run_resblocks3d or run_R / run_stage3_xf, layout launches
    included, in both modes; no split-K; no norm_act or split16 beyond the two norm_act launches that close R's stages; every stage-3 conv is
    followed by chan_stats_finish"""
    labels = traces[which, mode]["labels"]
    print("\n" + which + " " + mode + ": " + " ".join(labels))
    assert labels == [l for l, _ in PLANS[which]()]
    assert "splitk_finish" not in labels and "split16" not in labels and "chan_stats" not in labels
    na = [i for i, l in enumerate(labels) if l == "norm_act"]
    assert na == ([] if which == "F" else [13, 32])
    sp = [i for i, l in enumerate(labels) if l.endswith(".sp")]
    assert len(sp) == (0 if which == "F" else 12) and all(labels[i + 1] == FIN for i in sp) and labels.count(FIN) == len(sp)
    assert labels[-1] == "hwdc_to_ncdhw" and (which == "F" or labels[0] == "ncdhw_to_hwdc")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(ENTRIES))
def test_every_launch_writes_its_outputs_and_nothing_else(traces, which, mode):
    """After launch n: no sentinel in what launches 1 .. n write (all samples), everything else all sentinel - vsp[1] to the end, f_out until the
    last launch - and, against the run that stopped at launch n - 1, no buffer but launch n's outputs has changed a bit"""
    tr = traces[which, mode]
    assert not tr["bad"], tr["bad"][:8]
    assert len(tr["cap"]) == (18 if which == "F" else 32 + 12), sorted(tr["cap"])
    assert torch.equal(tr["cap"]["f_out"], tr["full"]), "f_out of the stop at the last launch is not the full run's"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(ENTRIES))
def test_steps_against_float64(reports, which, mode):
    """Every stored tensor of every launch against its float64 restatement on the engine's own operands, under the gate rules of the module
    docstring; the table is printed (error and gate at the element that uses most of its gate, the fraction used there, the 4-pixel border bands
    and the interior, the worst channel: c 16 + d of a volume; _row's "beyond")"""
    rows = reports[which, mode]["rows"]
    print(f"\n{which} step by step, {mode}: |d| and gate at the element that uses most of its gate")
    print(f"  {'launch':14s} {'tensor':9s} {'|d|':>9s} {'gate':>9s} {'used':>6s} {'border':>6s} {'inter.':>6s} {'chan':>4s} {'beyond':>6s}")
    for label, key, fr, d, gt, bd in rows:
        if "note" in bd:
            print(f"  {label:14s} {key:9s} {bd['note']}")
            continue
        border = max(bd["top"], bd["bottom"], bd["left"], bd["right"])
        print(f"  {label:14s} {key:9s} {d:9.2e} {gt:9.2e} {fr:6.2f} {border:6.2f} {bd['interior']:6.2f} {bd['channel']:4d} {bd['beyond']:6.2f}")
    print(f"  the largest fraction of its gate any step used: {max(r[2] for r in rows):.2f}; beyond the half fp16 spacing: {max(r[5]['beyond'] for r in rows):.2f}")
    assert len(rows) == (18 if which == "F" else 32)
    over = [(label, key, round(fr, 3)) for label, key, fr, _, _, _ in rows if not fr <= 1.0]
    assert not over, over


@pytest.mark.parametrize("mode", MODES)
def test_statistics_slots(reports, mode):
    """After each chan_stats_finish the slot holds no sentinel (the accounting test) and equals the float64 mean and 1 / sqrt(var + 1e-5) of the
    volume the conv stored, under test_chan_stats's tolerances: 12 slots per mode"""
    assert reports["F", mode]["stats"] == []
    stats = reports["R", mode]["stats"]
    assert len(stats) == 12
    for label, slot, (m64, r64) in stats:
        em, er = (slot[0].double() - m64).abs().max().item(), ((slot[1].double() - r64).abs() / r64).max().item()
        print(f"\n{mode} {label}: mean |d| {em:.2e}, rstd rel {er:.2e}")
        assert V.stats_close(slot, m64, r64), (label, em, er)


@pytest.mark.parametrize("which", list(ENTRIES))
def test_batch_independence(engines, inputs, which):
    """Every buffer cs_op_v_read returns after a B = 3 run equals, bit for bit, the same sample run alone at B = 1 on the batched engine; so does f_out"""
    e, x = engines["batched"], inputs[which]

    def run(xb):
        B = xb.shape[0]
        H.v_fill(e, B)
        out = H.v_run(e, ENTRIES[which], xb, torch.empty(B, 32, 16, 64, 64, device="cuda")).cpu()
        got = {w: H.v_read(e, w, B).view(torch.int16).cpu() for w in range(10)}
        got["stats"] = H.v_read(e, H.V_STATS, B).reshape(-1)[:B * 64].view(B, 64).view(torch.int16).cpu()
        return out, got

    out3, all3 = run(x)
    for i in range(3):
        out1, one = run(x[i:i + 1].contiguous())
        assert torch.equal(out1[0], out3[i]), i
        for k, v in one.items():
            assert torch.equal(v[0], all3[k][i]), (i, k)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_whole_stages(traces, vw, inputs, state_dicts):
    """f_out of the full runs (both modes) against the chained float64 steps and against the oracle: the stage gates of test_extract_feature_3d
    (1e-3) and test_refine_module (6e-4), in latency mode too"""
    from oracle import canonswap_ref as O
    for which, gate, chain, oracle, sd in (("F", 1e-3, V.chain_F, O.appearance_feature_extractor, "appearance_feature_extractor"),
                                          ("R", 6e-4, V.chain_R, O.refine, "refine")):
        x = inputs[which][1:2].cpu()
        chained, ref = chain(x.double(), vw), oracle(state_dicts[sd], x)
        for mode in MODES:
            full = traces[which, mode]["full"]
            rc, ro = _rel(full, chained), _rel(full, ref)
            print(f"\n{which} {mode}: relative L2 {rc:.2e} against the chained float64 steps, {ro:.2e} against the oracle")
            assert rc < gate and ro < gate


# ------------------------------------------------------------------------------------------------ the three kernels alone, at their edges
GUARD = 256


def _guarded(n, dtype):
    """(whole int buffer filled with the sentinel, view of the n payload elements in dtype) with GUARD elements on either side"""
    it, sent = (torch.int16, SENT16) if dtype == torch.float16 else (torch.int32, SENT32)
    buf = torch.full((n + 2 * GUARD,), sent, dtype=it, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _guards_intact(buf, n):
    s = int(buf[0])
    return bool(torch.all(buf[:GUARD] == s)) and bool(torch.all(buf[GUARD + n:] == s))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _randn(r, *shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


@pytest.mark.parametrize("N,Hh,Ww", [(2, 5, 7), (1, 16, 16)])
def test_conv_first(N, Hh, Ww):
    """conv_first_kernel against the float64 conv + bias + ReLU of its fp32 operands.  70 pixels: the second workgroup is mostly past the end.
    Gate: 27 fused multiply-adds from the bias, each rounding a partial sum no larger than |b| + sum |in| |w|, and the bias itself: 28 x 2^-24 of
    that magnitude, plus half an fp16 spacing for the store.  The guards around the output stay intact."""
    r = _rng(31)
    img, w, b = _randn(r, N, 3, Hh, Ww), _randn(r, 64, 27, scale=0.2), _randn(r, 64, scale=0.1)
    n = N * Hh * Ww * 64
    buf, out = _guarded(n, torch.float16)
    H.conv_first(img.cuda(), w.cuda(), b.cuda(), out)
    torch.cuda.synchronize()
    assert _guards_intact(buf, n) and not bool((out.view(torch.int16) == SENT16).any())
    got = out.view(N, Hh, Ww, 64).permute(0, 3, 1, 2).cpu().double()
    w64 = w.double().view(64, 3, 3, 3)
    R = torch.relu(torch.nn.functional.conv2d(img.double(), w64, b.double(), padding=1))
    mag = torch.nn.functional.conv2d(img.double().abs(), w64.abs(), b.double().abs(), padding=1)
    g = 28 * 2.0 ** -24 * mag + 0.5 * S.spacing16(R)
    fr = ((got - R).abs() / g).max().item()
    print(f"\nconv_first {N}x{Hh}x{Ww}: {fr:.2f} of the gate")
    assert fr <= 1.0


def _norm_act_case(r, N=2, per_n=4608):
    P = per_n // 32
    y, res = _randn(r, N, per_n, scale=2.0) + 0.5, _randn(r, N, per_n)
    stats = torch.stack([_randn(r, N, 32, scale=0.5) + 0.5, torch.from_numpy(r.uniform(0.3, 3.0, (N, 32)).astype(np.float32))], -1).contiguous()
    gamma, beta = _randn(r, 32) + 1.0, _randn(r, 32, scale=0.3)
    s2, t2 = _randn(r, 512) + 1.0, _randn(r, 512, scale=0.3)
    vol = lambda t: t.view(N, P, 32).permute(0, 2, 1).reshape(N, 1, 32, 1, 1, P)      # sample n as a "volume" [1, 32, 1, 1, P] of volume_ref
    per = lambda t: t[(torch.arange(per_n) % 512)].view(P, 32).t().reshape(1, 32, 1, 1, P)      # the 512-periodic affine in that view
    return dict(N=N, per_n=per_n, y=y, res=res, stats=stats, gamma=gamma, beta=beta, s2=s2, t2=t2, vol=vol, per=per)


@pytest.mark.parametrize("variant", ["split", "affine", "plain"])
@pytest.mark.parametrize("with_out32", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_norm_act(with_res, with_out32, variant):
    """norm_act_kernel on 2 samples of 4608 values (one full 4096-element block and a 512-element tail; a multiple of the period 512) against
    float64 under volume_ref.gn_gate; split mode: hi = fp16(v), lo = fp16(v - hi) bit for bit from the kernel's own out32 (without out32: the same
    bits as with it).  The guards around both outputs stay intact."""
    c = _norm_act_case(_rng(32))
    N, per_n = c["N"], c["per_n"]
    dev = lambda t: t.cuda().contiguous()
    kw = dict(res=dev(c["res"]) if with_res else None, split=variant == "split")
    if variant == "affine":
        kw.update(s2=dev(c["s2"]), t2=dev(c["t2"]), period2=512, act2="lrelu", slope2=0.01)
    n16 = N * per_n * (2 if variant == "split" else 1)
    b32, o32 = _guarded(N * per_n, torch.float32)
    b16, o16 = _guarded(n16, torch.float16)
    H.norm_act(dev(c["y"]), dev(c["stats"]), dev(c["gamma"]), dev(c["beta"]), out32=o32, out16=o16, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(b32, N * per_n) and _guards_intact(b16, n16)
    assert not bool((o32.view(torch.int32) == SENT32).any()) and not bool((o16.view(torch.int16) == SENT16).any())
    if not with_out32:      # the same bits without the fp32 output
        b16b, o16b = _guarded(n16, torch.float16)
        H.norm_act(dev(c["y"]), dev(c["stats"]), dev(c["gamma"]), dev(c["beta"]), out32=None, out16=o16b, **kw)
        torch.cuda.synchronize()
        assert _guards_intact(b16b, n16) and torch.equal(o16b.view(torch.int16), o16.view(torch.int16))
    got32, got16 = o32.view(N, per_n).cpu(), o16.view(N, -1).cpu()
    worst = 0.0
    for n in range(N):
        st = (c["stats"][n, :, 0], c["stats"][n, :, 1])
        R, M = V.gn_ref(c["vol"](c["y"])[n], st, c["gamma"], c["beta"], c["vol"](c["res"])[n] if with_res else None)
        worst = max(worst, ((c["vol"](got32)[n].double() - R).abs() / V.gn_gate(R, M)).max().item())
        if variant == "split":
            assert torch.equal(got16[n].view(-1, 64).view(torch.int16), H.split16(got32[n].view(-1, 32)).view(torch.int16))
            continue
        if variant == "affine":
            s2, t2 = c["per"](c["s2"]).double(), c["per"](c["t2"]).double()
            R2 = V.lrelu(R * s2 + t2)
            g = V.gn_gate(R2, M, True, (s2.abs(), t2.abs()))
        else:
            R2, g = R, V.gn_gate(R, M, True)
        worst = max(worst, ((c["vol"](got16.float())[n].double() - R2).abs() / g).max().item())
    print(f"\nnorm_act res {with_res} out32 {with_out32} {variant}: {worst:.2f} of the gate")
    assert worst <= 1.0


def test_norm_act_refusals():
    """the launcher refuses, with an error: values per sample that are no whole voxels, no multiple of the second affine's period, and the split
    output together with a second affine"""
    c = _norm_act_case(_rng(33))
    dev = lambda t: t.cuda().contiguous()
    y, st, g, b, s2, t2 = (dev(c[k]) for k in ("y", "stats", "gamma", "beta", "s2", "t2"))
    o32, o16 = torch.empty(2 * 4608, device="cuda"), torch.empty(4 * 4608, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="norm_act"):
        H.norm_act(y, st, g, b, out32=o32, out16=o16, per_n=4600)
    with pytest.raises(RuntimeError, match="norm_act"):
        H.norm_act(y, st, g, b, out32=o32, out16=o16, s2=s2, t2=t2, period2=1000, act2="lrelu", slope2=0.01)
    with pytest.raises(RuntimeError, match="norm_act"):
        H.norm_act(y, st, g, b, out32=o32, out16=o16, s2=s2, t2=t2, period2=512, split=True)
    H.norm_act(y, st, g, b, out32=o32, out16=o16)      # and launches what it does not refuse
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [32 * 5, 32 * 300])
def test_split16(n):
    """split16_kernel: [hi(32) | lo(32)] per voxel, hi = fp16(x), lo = fp16(x - hi), bit for bit (40 threads of one workgroup; ten workgroups, the last
    one partly past the end); the guards stay intact"""
    x = _randn(_rng(34), n, scale=3.0)
    buf, out = _guarded(2 * n, torch.float16)
    H.split16_op(x.cuda(), out)
    torch.cuda.synchronize()
    assert _guards_intact(buf, 2 * n)
    assert torch.equal(out.cpu().view(-1, 64).view(torch.int16), H.split16(x.view(-1, 32)).view(torch.int16))
