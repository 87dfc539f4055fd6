"""The SPADE decoder G (engine.hip run_G / spade_shortcut, pack._pack_G) launch by launch against float64, on the engine's own routing, in both modes.

cs_op_g_fill writes an fp16 NaN sentinel over G's workspace, cs_op_g_stop makes cs_spade_decode return after its n-th launch, cs_op_g_read copies
a buffer out.  For every launch n the test fills, runs to n and looks at all 18 buffers: what the launches so far must have written holds no
sentinel, everything else is still all sentinel (per output phase while mlp_shared's phase launches of an up block are under way).  The tensor launch
n wrote (sample 1 of the B = 3 call, sample 0 of the latency call: the same seg) is compared with tests/spade_ref.py's float64 restatement of
that step, computed from the fp16 tensors and the (mean, rstd) slot the engine's launch read and from the unpacked state dict - so pack._pack_G is
checked too.  The restatement is in the reference's form (mlp_shared as a 3x3 conv on the resized seg, SPADE on the up-sampled x, test_spade_ref_cpu.py
ties it to the oracle); the weights are rounded where pack rounds them, which for the learned shortcut is the composed W_s W_beta.

Gate of a step with float64 result R, elementwise: half an fp16 spacing at |R| where the launch stores fp16, plus 4 x max |E32 - R|, E32 the same
step in torch fp32 on the CPU from the same operands (spade_ref.gate).  Nothing is pinned from a GPU run.  The one launch whose arithmetic has a
rounding the step's operands do not show is up_1's fused .ng: the kernel packs h = IN(x)(1 + gamma) to fp16 for conv_s's MFMAs without storing it
(conv_halo_kernel.h, XSK); R and E32 round h there too (spade_ref.step_ng_cs), as the three-launch form would by storing it.

B = 3 is the smallest batch with the batched tile policy (128 x 256 tiles from 3 x 4096 positions, pick_halo_cfg); the B >= 8 / 16 conv_wide route
is tied to the halo route bit for bit by test_gpu_wide.py and test_gpu_batch32.py and is not run again here."""
import os
import tempfile

import numpy as np
import pytest
import torch

import hip_ops as H
import spade_ref as S

pytestmark = pytest.mark.gpu

MODES = ("batched", "latency")
SENT = H.G_SENTINEL
SENT32 = np.array([0x7E5A7E5A], np.uint32).view(np.float32)[0]      # what cs_op_g_fill leaves in an fp32 of the statistics pool


# ------------------------------------------------------------------------------------------------ a reading of run_G
def expected_labels():
    """cs_spade_decode's launches as engine.hip lists them, the same in both modes: conv_lat (latency: the 512 -> 512 convs at 64 x 64) keeps the
    layer's label, and no launch of G is `plain` with 64 workgroups or fewer (go(): G.fc, c0 and c1 carry statistics or a residual, the phase
    launches are grouped, the 64 x 64 mlp_shared is 384 workgroups, the 1x1 conv_s has a residual), so none is followed by splitk_finish.
    mlp_shared of the up blocks: x2 - all four phases are 2x2 taps, one grouped launch (p00); x4 - p00 (the four corner phases, 2x2 taps), p01
    (a = 0, 3 x the middle columns, 2x1, written to both pixels), p10 (a = 1 x b = 0, 3, 1x2, written to rows 1 and 2), p11 (a = 1 x the middle
    columns, 1x1, rows 1 and 2); no a = 2 phase.  up_1's conv_s runs inside its .ng launch (256 -> 64 channels on a 128 x 256 tile), up_0's apart."""
    L = ["nchw_to_nhwc16", "G.fc", "chan_stats_finish", "G.shared64", "G.shared128.p00", "G.shared256.p00", "G.shared256.p01", "G.shared256.p10",
         "G.shared256.p11"]
    for b in range(6):
        L += [f"G.m{b}.n0", f"G.m{b}.c0", "chan_stats_finish", f"G.m{b}.n1", f"G.m{b}.c1", "chan_stats_finish"]
    L += ["G.up0.bs", "G.up0.ng", "G.up0.cs", "G.up0.n0", "G.up0.c0", "chan_stats_finish", "G.up0.n1", "G.up0.c1", "chan_stats_finish"]
    L += ["G.up1.bs", "G.up1.ng", "G.up1.n0", "G.up1.c0", "chan_stats_finish", "G.up1.n1", "G.up1.c1", "G.img"]
    return L


def phase_cover(label):
    """(buffer, s, the output phases (y mod s, x mod s) a phase launch of mlp_shared writes): the phases of its tap shape, at x4 without row
    phase 2 as a launch of its own - the a = 1 launches write it"""
    grp, ph = label.rsplit(".p", 1)
    s = {"G.shared128": 2, "G.shared256": 4}[grp]
    a0, b0 = int(ph[0]), int(ph[1])
    edge = lambda v: v in (0, s - 1)
    rows = [a for a in range(s) if edge(a) == edge(a0) and not (s == 4 and a == 2)]
    if s == 4 and 1 in rows:
        rows.append(2)
    return (H.G_A128 if s == 2 else H.G_A256), s, {(a, b) for a in rows for b in range(s) if edge(b) == edge(b0)}


def buffer_of(key):
    k, _, i = key.partition(".")
    i = int(i) if i else -1
    if k == "x":
        return H.G_O256 if i == 8 else H.G_O128 if i == 7 else H.G_X0 + (i & 1)
    if k in ("a64", "a128", "a256"):
        return {"a64": H.G_A64, "a128": H.G_A128, "a256": H.G_A256}[k]
    lv = 0 if i < 6 else i - 5
    return {"bs": (None, H.G_BS, H.G_BS), "hs": (None, H.G_H128, H.G_H256), "xs": (None, H.G_XS128, H.G_XS256), "h0": (H.G_H64, H.G_H128, H.G_H256),
            "dx": (H.G_DX64, H.G_DX128, H.G_DX256), "h1": (H.G_H64, H.G_H1_128, H.G_H1_256)}[k][lv]


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
def seg3(engines):
    """[3, 256, 64, 64] fp32 on the device: cs_warp_out of the synthetic frames' appearance features under a smooth occlusion map"""
    from canonswap_amd import synth
    e = engines["batched"]
    img = torch.from_numpy(synth.make_frame_inputs(3, seed=2100, size=256)["img"]).cuda()
    f = e.extract_feature_3d(img)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 64), torch.linspace(-1, 1, 64), indexing="ij")
    occ = torch.stack([torch.sigmoid(3.0 * torch.sin(2.5 * xx + i) * torch.cos(1.7 * yy - i) + 0.5) for i in range(3)])[:, None]
    return e.warp_out(f, occ.cuda()).contiguous()


def _labels(e, seg, img):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "launches.csv")
        old = os.environ.get("CANONSWAP_PROFILE_CSV")
        os.environ["CANONSWAP_PROFILE_CSV"] = path
        try:
            e.profile_begin()
            H.g_decode(e, seg, img)
            e.profile_end()
        finally:
            if old is None:
                del os.environ["CANONSWAP_PROFILE_CSV"]
            else:
                os.environ["CANONSWAP_PROFILE_CSV"] = old
        return [l.split(",")[1] for l in open(path).read().splitlines()[1:]]


def _nchw(t):
    """one sample [H, W, C] fp16 on the device -> [1, C, H, W] on the host"""
    return t.permute(2, 0, 1).unsqueeze(0).contiguous().cpu()


def _trace(e, seg, s):
    """Runs cs_spade_decode to each of its launches in turn.  Returns the launch list, per launch what it wrote (sample s), the statistics slot
    read at every stop (all samples) and the violations of the accounting: a sentinel in what launches 1 .. n write, anything but the sentinel
    elsewhere, a buffer other than launch n's output that differs from the run that stopped at launch n - 1."""
    B = seg.shape[0]
    img = torch.empty(B, 3, 512, 512, device=seg.device)
    labels = _labels(e, seg, img)
    full_img = img[s:s + 1].cpu()
    steps = {l: (out, st) for l, out, _, _, _, st in S.step_list(None, fused_up1="G.up1.cs" not in labels)}
    bufs = [{w: torch.empty((B,) + H.G_SHAPE[w], dtype=torch.float16, device=seg.device) for w in range(18)} for _ in range(2)]
    written, cap, slots, bad = {}, {}, [], []
    for n, label in enumerate(labels, 1):
        scratch, prev = bufs[n & 1], bufs[~n & 1]
        H.g_fill(e, B)
        img.fill_(float("nan"))
        H.g_decode(e, seg, img, stop=n)
        out, wout, cover = None, None, None      # the step's key, the buffer launch n writes, the output phases it writes (None: all)
        if label.startswith(("G.shared128.p", "G.shared256.p")):
            wout, sc, cover = phase_cover(label)
            written[wout] = (sc, (written[wout][1] if wout in written else set()) | cover)
            if len(written[wout][1]) == sc * sc:
                written[wout] = "all"
                out = "a128" if sc == 2 else "a256"
        elif label in steps and label != "G.img":
            out = steps[label][0]
            wout = buffer_of(out)
            written[wout] = "all"
        for w in range(18):
            cur = H.g_read(e, w, B, out=scratch[w]).view(torch.int16)
            sent = cur == SENT
            if w not in written:
                ok = bool(sent.all())
            elif written[w] == "all":
                ok = not bool(sent.any())
            else:
                sc, cov = written[w]
                ok = all(not bool(sent[:, a::sc, b::sc].any()) if (a, b) in cov else bool(sent[:, a::sc, b::sc].all())
                         for a in range(sc) for b in range(sc))
            if not ok:
                bad.append((n, label, H.G_NAMES[w], "untouched" if w not in written else written[w]))
            # the runs are deterministic: against the run that stopped one launch earlier, launch n changed its own output and nothing else
            if n > 1:
                old = prev[w].view(torch.int16)
                if w != wout:
                    same = torch.equal(cur, old)
                else:
                    same = cover is None or all(torch.equal(cur[:, a::sc, b::sc], old[:, a::sc, b::sc])
                                                for a in range(sc) for b in range(sc) if (a, b) not in cover)
                if not same:
                    bad.append((n, label, H.G_NAMES[w], "changed by a launch that does not write it"))
        isn = torch.isnan(img)
        if not bool(isn.all() if label != "G.img" else ~isn.any()):
            bad.append((n, label, "img", "written" if label != "G.img" else "sentinel left"))
        if out is not None:
            w = buffer_of(out)
            t = scratch[w][s]
            if out == "bs.6":
                t = t.reshape(128, 128, 256)
            cap[out] = _nchw(t)
        if label == "G.img":
            cap["img"] = img[s:s + 1].cpu()
        slots.append(H.g_read(e, H.G_STATS, B).cpu())
    return dict(labels=labels, cap=cap, slots=slots, bad=bad, full_img=full_img, B=B, s=s)


@pytest.fixture(scope="module")
def traces(engines, seg3):
    return {"batched": _trace(engines["batched"], seg3, 1), "latency": _trace(engines["latency"], seg3[1:2].contiguous(), 0)}


def _slot(tr, n, C):
    """the (mean, rstd) of sample s in the slot read after launch n (1-based), as fp32 [C] tensors"""
    v = tr["slots"][n - 1][:, :].reshape(-1)[:tr["B"] * C * 2].view(tr["B"], C, 2)[tr["s"]]
    return v[:, 0].clone(), v[:, 1].clone()


@pytest.fixture(scope="module")
def gw(state_dicts):
    return S.GWeights(state_dicts["spade_generator"])


@pytest.fixture(scope="module")
def seg_only(gw, seg3):
    """(R, E32) of the launches that read seg alone: the same in both modes"""
    T = {"seg": seg3[1:2].half().cpu()}
    return {l: (fn(T, torch.float64), fn(T, torch.float32)) for l, _, fn, _, _, _ in S.step_list(gw)[:4]}


@pytest.fixture(scope="module")
def reports(traces, gw, seg3, seg_only):
    """Per mode: a row per step (label, largest fraction of its gate used, |d| and gate there, the breakdown) and per statistics slot"""
    out = {}
    for mode in MODES:
        tr = traces[mode]
        labels, cap = tr["labels"], tr["cap"]
        T = {"seg": seg3[1:2].half().cpu()}
        rows, stats = [], []
        for label, okey, fn, sc, f16, st in S.step_list(gw, fused_up1="G.up1.cs" not in labels):
            if okey not in cap:
                rows.append((label, float("inf"), float("nan"), float("nan"), {"note": "not captured"}))
                continue
            R, E32 = seg_only[label] if label in seg_only else (fn(T, torch.float64), fn(T, torch.float32))
            got = cap[okey]
            if label == "G.img":
                g = S.gate(R, E32, False) + _sigmoid_term(S.img_logits(T["x.8"].double(), gw))
            else:
                g = S.gate(R, E32, f16)
            fr, d, gt = S.used(got, R, g)
            bd = S.breakdown(got, R, g, sc)
            bd["allow"], bd["allow_used"] = S.allowance(R, E32), S.allowance_used(got, R, g, S.allowance(R, E32))
            rows.append((label, fr, d, gt, bd))
            T[okey] = got
            if st:
                last = max(i for i, l in enumerate(labels, 1) if l.startswith(label))
                assert labels[last] == "chan_stats_finish", (label, labels[last])
                T[st] = _slot(tr, last + 1, got.shape[1])
                m, r = S.chan_stats(got.double())
                stats.append((label, T[st][0].double(), T[st][1].double(), m, r))
        out[mode] = dict(rows=rows, stats=stats, T=T)
    return out


def _sigmoid_term(z):
    """The engine's sigmoid is 1.f / (1.f + __expf(-z)) (conv_epilogue.h).  __expf(x) = exp2(x log2 e): the product's rounding and the constant's
    shift the exponent by at most |x| log2 e 2^-23, a relative ln 2 |x| log2 e 2^-23 = |x| 2^-23 of the result; the hardware exp2 is good to one
    ulp, 2^-23: e = exp(-z) carries (|z| + 1) 2^-23.  d sigma / d e = -sigma^2, so e's error moves sigma by sigma (1 - sigma) <= 1/4 of that;
    the sum 1 + e and the division round once each, 2^-24 sigma <= 2^-24 apiece.  (The error of z itself goes through the same slope <= 1/4 and is
    in the E32 allowance, which is measured on the image.)"""
    return 2.0 ** -23 * (1.0 + (z.abs() + 1.0) / 4.0)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("mode", MODES)
def test_launch_list(traces, mode):
    """The profile CSV's labels of cs_spade_decode equal the list read off run_G (expected_labels), in both modes"""
    labels = traces[mode]["labels"]
    print("\n" + mode + ": " + " ".join(labels))
    assert labels == expected_labels()
    assert not any(l.startswith(("G.shared128.p", "G.shared256.p")) and l[-2] == "2" for l in labels), "an a = 2 phase was launched"
    assert "splitk_finish" not in labels
    follows = [labels[i - 1] for i, l in enumerate(labels) if l == "chan_stats_finish"]
    assert follows == ["G.fc"] + [f"G.m{b}.c{k}" for b in range(6) for k in (0, 1)] + ["G.up0.c0", "G.up0.c1", "G.up1.c0"]


@pytest.mark.parametrize("mode", MODES)
def test_every_launch_writes_its_output_and_nothing_else(traces, mode):
    """After launch n: no sentinel in what launches 1 .. n write (all samples; per output phase inside mlp_shared's phase launches), everything else
    all sentinel - g_h256 after up_1's fused .ng, the other g_x of the first middle block, the image before conv_img - and, against the run that
    stopped at launch n - 1, no buffer but launch n's output has changed a bit (the other g_x of every block, the phases of g_a256 written before)"""
    tr = traces[mode]
    assert not tr["bad"], tr["bad"][:8]
    assert len(tr["cap"]) == 42, sorted(tr["cap"])


@pytest.mark.parametrize("mode", MODES)
def test_steps_against_float64(reports, mode):
    """Every launch of G against its float64 restatement on the engine's own operands, under the gate rule of the module docstring; the table is
    printed (error, gate at the worst element, fraction of the gate used there, border bands / interior, worst output phase, worst channel, the fp32
    allowance 4 x max |E32 - R| and the largest fraction of it an element needs beyond its spacing term)"""
    rows = reports[mode]["rows"]
    print(f"\nG step by step, {mode}: |d| and gate at the element that uses most of its gate")
    print(f"  {'step':12s} {'|d|':>9s} {'gate':>9s} {'used':>6s} {'border':>6s} {'inter.':>6s} {'phase':>7s} {'chan':>4s} {'fp32 allow.':>11s} {'used':>6s}")
    for label, fr, d, gt, bd in rows:
        if "note" in bd:
            print(f"  {label:12s} {bd['note']}")
            continue
        border = max(bd["top"], bd["bottom"], bd["left"], bd["right"])
        print(f"  {label:12s} {d:9.2e} {gt:9.2e} {fr:6.2f} {border:6.2f} {bd['interior']:6.2f} {str(bd.get('phase', '-')):>7s} {bd['channel']:4d} {bd['allow']:11.2e} {bd['allow_used']:6.2f}")
    assert len(rows) == 42
    over = [(label, round(fr, 3)) for label, fr, _, _, _ in rows if not fr <= 1.0]
    assert not over, over


@pytest.mark.parametrize("mode", MODES)
def test_statistics_slots(reports, mode):
    """After each go_stats the slot holds the mean and 1 / sqrt(var + 1e-5) of the tensor the conv stored (test_chan_stats's tolerances)"""
    stats = reports[mode]["stats"]
    assert len(stats) == 16
    for label, mean, rstd, m64, r64 in stats:
        em, er = (mean - m64).abs().max().item(), ((rstd - r64).abs() / r64).max().item()
        print(f"\n{mode} {label}: mean |d| {em:.2e}, rstd rel {er:.2e}")
        assert not (mean == float(SENT32)).any() and not (rstd == float(SENT32)).any(), label
        assert torch.allclose(mean, m64, rtol=1e-5, atol=1e-6), (label, em)
        assert torch.allclose(rstd, r64, rtol=1e-4, atol=0), (label, er)


@pytest.mark.parametrize("mode", MODES)
def test_sx_survives_the_upsampling(traces, reports, mode):
    """The SPADE launches of an up block (.ng, .n0) normalise the up-sampled x with the statistics of the half-size x: the slot read at every stop
    from the chan_stats_finish of the previous block to the block's conv_0 is the same bits, and float64 statistics of the nearest-up-sampled tensor
    agree with it"""
    from oracle import canonswap_ref as O
    tr, T = traces[mode], reports[mode]["T"]
    labels = tr["labels"]
    for first, last, xk, sk in (("G.up0.bs", "G.up0.c0", "x.6", "sx.6"), ("G.up1.bs", "G.up1.c0", "x.7", "sx.7")):
        i0, i1 = labels.index(first), labels.index(last)
        assert labels[i0 - 1] == "chan_stats_finish"
        for i in range(i0, i1 + 1):
            assert torch.equal(tr["slots"][i], tr["slots"][i0 - 1]), labels[i]
        m, r = S.chan_stats(O.nearest_up(T[xk].double(), 1, 2, 2))
        assert torch.allclose(T[sk][0].double(), m, rtol=1e-5, atol=1e-6) and torch.allclose(T[sk][1].double(), r, rtol=1e-4, atol=0)


def _read_all(e, B):
    out = {H.G_NAMES[w]: H.g_read(e, w, B).view(torch.int16).cpu() for w in range(18)}
    out["stats"] = H.g_read(e, H.G_STATS, B)[:, :].reshape(-1)[:B * 128].view(B, 128).cpu()      # the last go_stats: up_1's conv_0, 64 channels
    return out


def test_batch_independence(engines, seg3):
    """Every buffer cs_op_g_read returns after a full B = 3 run equals, bit for bit, the same sample run alone at B = 1; so does the image"""
    e = engines["batched"]
    img3 = H.g_decode(e, seg3, torch.empty(3, 3, 512, 512, device="cuda")).cpu()
    all3 = _read_all(e, 3)
    for i in range(3):
        img1 = H.g_decode(e, seg3[i:i + 1].contiguous(), torch.empty(1, 3, 512, 512, device="cuda")).cpu()
        one = _read_all(e, 1)
        assert torch.equal(img1[0], img3[i]), i
        for k, v in one.items():
            assert torch.equal(v[0], all3[k][i]), (i, k)


def test_whole_decoder(traces, gw, seg3, state_dicts):
    """The image of the full run (both modes) against the chained float64 steps and against oracle.canonswap_ref.spade_decoder: the PSNR gate of
    test_conv_decode"""
    from oracle import canonswap_ref as O
    seg = seg3[1:2].cpu()
    chained, _ = S.chain(seg.half().double(), gw)
    oracle = O.spade_decoder(state_dicts["spade_generator"], seg)
    for mode in MODES:
        tr = traces[mode]
        assert torch.equal(tr["cap"]["img"], tr["full_img"]), "the image of the stop at the last launch is not the full run's"
        pc, po = O.psnr(tr["full_img"].double(), chained), O.psnr(tr["full_img"], oracle)
        print(f"\n{mode}: PSNR {pc:.1f} dB against the chained float64 steps, {po:.1f} dB against the oracle")
        assert pc >= 50.0 and po >= 50.0
