"""The motion extractor M kernel by kernel (csrc/motion.hip and M's split-precision 1x1 convs) against float64 restatements.

Weights: M's synthetic weights (synth) packed by pack._pack_M, the references read the unpacked state dict, so the packing layouts are
checked too.  A split output [hi | lo] is checked twice: hi + lo (float64) against the reference, and as a pair: hi is a nearest fp16 of
hi + lo (ties either way) and |lo| <= ulp(hi) / 2.  Errors are max |got - ref| / max |ref| per tensor; every gate records the value
measured on the MI355X and sits within 4x of it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hip_ops as H

pytestmark = pytest.mark.gpu

DIMS, DEPTHS = (96, 192, 384, 768), (3, 3, 9, 3)
GRID = (64, 32, 16, 8)
SENT = 0x7E5A          # fp16 NaN payload: the sentinel of the guard regions


@pytest.fixture(scope="module")
def msd():
    from canonswap_amd import synth
    return synth.to_torch(synth.make_state_dicts(0, modules=("motion_extractor",)))["motion_extractor"]


@pytest.fixture(scope="module")
def sdd(msd):
    return {k: v.double() for k, v in msd.items()}


@pytest.fixture(scope="module")
def mb(msd):
    """pack._pack_M's blobs on the device"""
    from canonswap_amd import pack
    out = {}
    pack._pack_M(out, pack._np_sd(msd))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in out.items()}


@pytest.fixture(scope="module")
def engines():
    from canonswap_amd.engine import Engine
    es = {"batched": Engine(0, max_batch=3), "latency": Engine(0, max_batch=1, latency_mode=True)}
    yield es
    for e in es.values():
        e.close()


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def _err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return (got - ref).abs().max().item() / ref.abs().max().item()


def _gate(what, err, gate):
    print(f"\n{what}: {err:.3e} (gate {gate:.0e})")
    assert err <= gate, (what, err, gate)


def _check_split(what, y, ref, gate):
    """y: fp16 [..., 2C] = [hi | lo]; ref float64 [..., C]"""
    v, hi, lo = H.unsplit(y)
    _gate(what, _err(v, ref), gate)
    s = v.cpu().numpy()
    h = hi.cpu().numpy()
    r = s.astype(np.float16).astype(np.float64)         # numpy rounds float64 -> fp16 once
    assert np.all(np.abs(s - h) <= np.abs(s - r)), f"{what}: hi is not a nearest fp16 of hi + lo"
    assert np.all(np.abs(lo.cpu().numpy().astype(np.float64)) <= np.spacing(np.abs(h)).astype(np.float64) / 2), f"{what}: |lo| > ulp(hi) / 2"


def _ln(x, g, b, eps=1e-6):
    u = x.mean(-1, keepdim=True)
    v = ((x - u) ** 2).mean(-1, keepdim=True)
    return (x - u) / torch.sqrt(v + eps) * g + b


def _guarded16(n, guard):
    buf = torch.full((guard + n + guard,), SENT, dtype=torch.int16, device="cuda")
    return buf, buf[guard:guard + n].view(torch.float16)


# ------------------------------------------------------------------------------------------------ stem
def _stem_ref(img, w, b, g, be):
    x = F.conv2d(img.double(), w.double(), b.double(), stride=4).permute(0, 2, 3, 1)
    return _ln(x, g.double(), be.double())


@pytest.mark.parametrize("N", [1, 3, 64])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_stem(mb, sdd, N, kind):
    from canonswap_amd import synth
    img = (torch.from_numpy(synth.make_smooth_images(N, seed=3100 + N, size=256)) if kind == "smooth"
           else torch.rand(N, 3, 256, 256, generator=_rng(N)))
    got = H.m_stem(img.cuda(), mb["M.stem.w"], mb["M.stem.b"], mb["M.stem.ln.g"], mb["M.stem.ln.b"])
    p = "detector.downsample_layers.0."
    ref = _stem_ref(img, sdd[p + "0.weight"], sdd[p + "0.bias"], sdd[p + "1.weight"], sdd[p + "1.bias"])
    # 48-term fp32 dot products, LayerNorm over 96 with rsqrtf: measured <= 4.9e-7 (smooth) / 3.6e-7 (noise)
    _gate(f"stem N={N} {kind}", _err(got, ref), 1.4e-6)


def test_stem_zero_variance_gives_beta(mb):
    """96 equal output rows: every position's variance is exactly 0, so the normalised value is 0 and the output is `be` bit for bit.
    (Dyadic image and weights keep the conv sums exact, the mean of equal values exact.)"""
    r = _rng(7)
    img = torch.floor(torch.rand(3, 3, 256, 256, generator=r) * 256) / 256
    wk = torch.randint(-8, 9, (48, 1), generator=r).float() / 64
    w = wk.expand(48, 96).contiguous().cuda()
    b = torch.full((96,), 0.25).cuda()
    be = mb["M.stem.ln.b"]
    got = H.m_stem(img.cuda(), w, b, mb["M.stem.ln.g"], be)
    assert torch.equal(got, be.expand_as(got))


def test_stem_rejects_other_widths(mb):
    img = torch.zeros(1, 3, 256, 128, device="cuda")
    with pytest.raises(RuntimeError, match="256 input columns"):
        H.m_stem(img, mb["M.stem.w"], mb["M.stem.b"], mb["M.stem.ln.g"], mb["M.stem.ln.b"])


# ------------------------------------------------------------------------------------------------ dwln
def _dwln_ref(x, sdd, q, bias):
    C = x.shape[-1]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), sdd[q + ".dwconv.weight"], bias, padding=3, groups=C).permute(0, 2, 3, 1)
    return _ln(y, sdd[q + ".norm.weight"], sdd[q + ".norm.bias"])


DWLN_CASES = [(0, 1), (0, 3), (0, 64), (1, 1), (1, 3), (2, 1), (2, 3), (3, 1), (3, 3)]


@pytest.mark.parametrize("stage,N", DWLN_CASES)
@pytest.mark.parametrize("data", ["normal", "offset"])
def test_dwln(mb, sdd, stage, N, data):
    """Every template instance (K = 2 with half-masked lanes, 3, 6, 12), every stage's grid (the 8 x 8 one: every run touches both borders).
    offset: the conv outputs of a position share an offset of 100 (bias + 100) with a spread of 1e-2 (LayerNorm cancellation: a one-pass
    variance would lose every bit).  Guard regions around the output keep their sentinel."""
    C, Hs = DIMS[stage], GRID[stage]
    q, o = f"detector.stages.{stage}.0", f"M.s{stage}.0"
    x = torch.randn(N, Hs, Hs, C, generator=_rng(100 * stage + N))
    b = mb[o + ".dw.b"]
    if data == "offset":
        b = b + 100.0
        # x scaled so that the conv's own spread is 1e-2 (the LayerNorm output is scale-free)
        x = x * (1e-2 / F.conv2d(x[:1].double().permute(0, 3, 1, 2), sdd[q + ".dwconv.weight"], None, padding=3, groups=C).std().item())
    n = N * Hs * Hs * 2 * C
    guard = 4 * C
    buf, y = _guarded16(n, guard)
    H.m_dwln(x.cuda(), mb[o + ".dw.w"], b, mb[o + ".ln.g"], mb[o + ".ln.b"], y)
    ref = _dwln_ref(x, sdd, q, b.double().cpu())
    # normal: 49-tap fp32 sums + LayerNorm, measured <= 3.7e-7.  offset: every fp32 partial sum near 100 rounds at ulp(100) / 2 = 3.8e-6,
    # against a spread of 1e-2 (inherent to fp32), measured <= 5.6e-4
    _check_split(f"dwln stage {stage} N={N} {data}", y.view(N, Hs, Hs, 2 * C), ref, 1.2e-6 if data == "normal" else 2e-3)
    assert torch.all(buf[:guard] == SENT) and torch.all(buf[guard + n:] == SENT), "m_dwln wrote outside its output"


# ------------------------------------------------------------------------------------------------ ln_s2d
@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("data", ["normal", "offset"])
def test_ln_s2d_channel_order(mb, sdd, stage, data):
    """LayerNorm then the 2x2 space-to-depth in (dy, dx, c) order - the order pack._pack_M's downsample weights assume."""
    C, Hs, N = DIMS[stage], GRID[stage], 3
    x = torch.randn(N, Hs, Hs, C, generator=_rng(200 + stage))
    if data == "offset":      # per-row offset 100, spread 1e-2
        x = 100.0 + torch.randn(N, Hs, Hs, 1, generator=_rng(300 + stage)) + 1e-2 * x
    q = f"detector.downsample_layers.{stage + 1}.0"
    y = H.m_ln_s2d(x.cuda(), mb[f"M.ds{stage}.ln.g"], mb[f"M.ds{stage}.ln.b"])
    ln = _ln(x.double(), sdd[q + ".weight"], sdd[q + ".bias"])
    ref = ln.view(N, Hs // 2, 2, Hs // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Hs // 2, Hs // 2, 4 * C)
    # normal: measured <= 2.0e-7; offset: the fp32 row sums near C x 100 round at ulp / 2, against a spread of 1e-2, measured <= 4.4e-4
    _check_split(f"ln_s2d stage {stage} {data}", y, ref, 6e-7 if data == "normal" else 1.5e-3)


# ------------------------------------------------------------------------------------------------ grn
def _grn_ref(h, gamma, beta):
    h = h.double()
    gx = torch.sqrt((h * h).sum(1, keepdim=True))                 # util.py:365-368
    nx = gx / (gx.mean(-1, keepdim=True) + 1e-6)
    return gamma * (h * nx) + beta + h


GRN_CASES = [(4096, 384, 0), (1024, 768, 1), (256, 1536, 2), (64, 3072, 3),     # the engine's four shapes (16 / 8 / 4 / 1 slices)
             (4100, 384, 0), (1000, 768, 1), (300, 1536, 2)]                     # slices of unequal length, the tail loop


@pytest.mark.parametrize("P,C,stage", GRN_CASES)
def test_grn(mb, sdd, P, C, stage):
    """N = 3 with sample 1 all zero and channel 5 zero in every sample; bit-equal when repeated."""
    N = 3
    h = F.gelu(torch.randn(N, P, C, generator=_rng(P + C)) * 2)
    h[1] = 0
    h[:, :, 5] = 0
    o = f"M.s{stage}.0.grn"
    hd = h.cuda()
    y = H.m_grn(hd, mb[o + ".g"], mb[o + ".b"])
    q = f"detector.stages.{stage}.0.grn"
    ref = _grn_ref(h, sdd[q + ".gamma"].reshape(-1), sdd[q + ".beta"].reshape(-1))
    # fp32 sum of squares over P (16 position lanes per slice), sqrtf, and one fp32 multiply-add per element: measured <= 1.7e-7
    _check_split(f"grn P={P} C={C}", y, ref, 5e-7)
    assert torch.equal(H.m_grn(hd, mb[o + ".g"], mb[o + ".b"]), y)


def test_grn_sample_of_a_batch_is_the_sample_alone(mb):
    N, P, C = 64, 4096, 384
    h = F.gelu(torch.randn(N, P, C, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) * 2)
    g, b = mb["M.s0.0.grn.g"], mb["M.s0.0.grn.b"]
    y = H.m_grn(h, g, b)
    for i in (0, 31, 63):
        assert torch.equal(H.m_grn(h[i:i + 1].contiguous(), g, b), y[i:i + 1]), i


# ------------------------------------------------------------------------------------------------ head
def _head_ref(x, sdd):
    p = "detector."
    f = _ln(x.double().mean(1), sdd[p + "norm.weight"], sdd[p + "norm.bias"])
    from oracle.canonswap_ref import M_HEADS
    w = torch.cat([sdd[f"{p}fc_{k}.weight"] for k, _ in M_HEADS], 0)
    b = torch.cat([sdd[f"{p}fc_{k}.bias"] for k, _ in M_HEADS], 0)
    return f @ w.t() + b


@pytest.mark.parametrize("N", [1, 3, 64])
def test_head(mb, sdd, N):
    x = torch.randn(N, 64, 768, generator=_rng(400 + N))
    got = H.m_head(x.cuda(), mb["M.norm.g"], mb["M.norm.b"], mb["M.head.w"], mb["M.head.b"])
    # 64-term pool, LayerNorm over 768, 768-term fp32 dot products: measured 6.7e-7 (N = 1, 3) / 1.1e-6 (N = 64)
    _gate(f"head N={N}", _err(got, _head_ref(x, sdd)), 2.6e-6)


# ------------------------------------------------------------------------------------------------ split-precision 1x1 convs
def _pw_case(form, stage, N, seed):
    """(input split fp16, out buffer (guarded, fp32), float64 reference builder inputs)"""
    C, Hs = DIMS[stage], GRID[stage]
    r = _rng(seed)
    if form == H.M_PW1:
        v = torch.randn(N, Hs, Hs, C, generator=r)
        return v, H.split16(v), None, Hs, 4 * C
    if form == H.M_PW2:
        v = F.gelu(torch.randn(N, Hs, Hs, 4 * C, generator=r))
        return v, H.split16(v), torch.randn(N, Hs, Hs, C, generator=r), Hs, C
    x = torch.randn(N, Hs, Hs, C, generator=r)                     # the downsample's input grid; the conv runs on Hs / 2
    s2d = x.view(N, Hs // 2, 2, Hs // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Hs // 2, Hs // 2, 4 * C)
    return x, H.split16(s2d), None, Hs // 2, 2 * C


def _pw_ref(form, stage, sdd, v, res):
    C = DIMS[stage]
    if form == H.M_PW1:
        q = f"detector.stages.{stage}.0.pwconv1"
        return F.gelu(v.double() @ sdd[q + ".weight"].t() + sdd[q + ".bias"])
    if form == H.M_PW2:
        q = f"detector.stages.{stage}.0.pwconv2"
        return res.double() + v.double() @ sdd[q + ".weight"].t() + sdd[q + ".bias"]
    q = f"detector.downsample_layers.{stage + 1}.1"
    return F.conv2d(v.double().permute(0, 3, 1, 2), sdd[q + ".weight"], sdd[q + ".bias"], stride=2).permute(0, 2, 3, 1)


PW_CASES = [(f, s) for s in range(4) for f in (H.M_PW1, H.M_PW2, H.M_DS) if not (f == H.M_DS and s == 3)]
# max |d| / max |ref| measured on the MI355X (batched engine, latency engine); the gate is 2.5x the mode's value
PW_MEASURED = {(H.M_PW1, 0): (4.2e-7, 3.9e-7), (H.M_PW1, 1): (6.1e-7, 6.2e-7), (H.M_PW1, 2): (8.3e-7, 8.7e-7), (H.M_PW1, 3): (9.8e-7, 9.8e-7),
               (H.M_PW2, 0): (2.8e-7, 2.9e-7), (H.M_PW2, 1): (4.0e-7, 3.5e-7), (H.M_PW2, 2): (6.0e-7, 6.2e-7), (H.M_PW2, 3): (8.7e-7, 9.3e-7),
               (H.M_DS, 0): (7.4e-7, 4.3e-7), (H.M_DS, 1): (9.6e-7, 5.6e-7), (H.M_DS, 2): (1.5e-6, 6.1e-7)}



@pytest.mark.parametrize("mode", ["batched", "latency"])
@pytest.mark.parametrize("form,stage", PW_CASES)
def test_pointwise(mb, sdd, engines, tmp_path, monkeypatch, mode, form, stage):
    """pwconv1 (GELU), pwconv2 (fp32 residual in place; stage 0: Cout 96 on a 128-wide block) and the downsample conv (space-to-depth
    input) on the engine's routing, against the float64 matmul / conv2d(k=2, s=2) of the un-split fp32 input.  The latency-mode engine at
    B = 1 sends the downsample convs through cross-workgroup split-K (a splitk_finish launch), never the others; the batched engine never."""
    e = engines[mode]
    N = 3 if mode == "batched" else 1
    v, xin, res, Ho, Cout = _pw_case(form, stage, N, 500 + 10 * stage + form)
    name = {H.M_PW1: "pw1", H.M_PW2: "pw2", H.M_DS: "ds"}[form]
    if form == H.M_DS:
        w, b = mb[f"M.ds{stage}.w"], mb[f"M.ds{stage}.b"]
    else:
        w, b = mb[f"M.s{stage}.0.{name}.w"], mb[f"M.s{stage}.0.{name}.b"]
    n = N * Ho * Ho * Cout
    guard = 2 * Cout
    buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:n].view(N, Ho, Ho, Cout)
    if res is not None:
        out.copy_(res)
    monkeypatch.setenv("CANONSWAP_PROFILE_CSV", str(tmp_path / "launches.csv"))
    e.profile_begin()
    H.m_pointwise(e, form, xin.cuda(), w, b, out, DIMS[stage])
    prof = e.profile_end()
    labels = [l.split(",")[1] for l in (tmp_path / "launches.csv").read_text().splitlines()[1:]]
    splitk = mode == "latency" and form == H.M_DS
    assert prof["conv_launches"] == 1 and labels[0] == f"m_{name}"
    assert labels[1:] == (["splitk_finish"] if splitk else []), labels
    # 2^-22 from the split operands and the dropped W_lo v_lo, fp32 sums of 3 Cin terms (288 - 9216), growing with Cin; split-K adds the
    # same products in 16 partial sums
    _gate(f"{name} stage {stage} {mode}", _err(out, _pw_ref(form, stage, sdd, v, res)), 2.5 * PW_MEASURED[form, stage][mode == "latency"])
    assert torch.all(torch.isnan(buf[n:])), "the conv wrote past its output"


# ------------------------------------------------------------------------------------------------ one block at a time
def test_blocks_one_at_a_time(mb, sdd, engines):
    """Each of the 18 ConvNeXtV2 blocks, the three downsample layers, the stem and the head on the float64 oracle's own input to that
    layer, composed from the operators the engine runs (dwln -> pw1 -> grn -> pw2; ln_s2d -> ds).  Localises a precision regression to
    one layer.  Gate: the relative error of the layer's output, measured 4.2e-7 (stem) - 1.5e-6 (ds2)."""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    e = engines["batched"]
    img = torch.from_numpy(synth.make_smooth_images(1, seed=2000, size=256))
    p = "detector."
    x = _stem_ref(img, sdd[p + "downsample_layers.0.0.weight"], sdd[p + "downsample_layers.0.0.bias"],
                  sdd[p + "downsample_layers.0.1.weight"], sdd[p + "downsample_layers.0.1.bias"])
    errs = []
    got = H.m_stem(img.cuda(), mb["M.stem.w"], mb["M.stem.b"], mb["M.stem.ln.g"], mb["M.stem.ln.b"])
    errs.append(("stem", _err(got, x)))
    for i in range(4):
        C, Hs = DIMS[i], GRID[i]
        if i > 0:
            xin = x
            x = O._ln_last(x, sdd, p + f"downsample_layers.{i}.0")
            x = F.conv2d(x.permute(0, 3, 1, 2), sdd[p + f"downsample_layers.{i}.1.weight"], sdd[p + f"downsample_layers.{i}.1.bias"],
                         stride=2).permute(0, 2, 3, 1)
            y = H.m_ln_s2d(xin.float().contiguous().cuda(), mb[f"M.ds{i - 1}.ln.g"], mb[f"M.ds{i - 1}.ln.b"])
            out = torch.empty(1, Hs, Hs, C, device="cuda")
            H.m_pointwise(e, H.M_DS, y, mb[f"M.ds{i - 1}.w"], mb[f"M.ds{i - 1}.b"], out, DIMS[i - 1])
            errs.append((f"ds{i - 1}", _err(out, x)))
        for j in range(DEPTHS[i]):
            xin, o = x, f"M.s{i}.{j}"
            x = O.convnext_block(x, sdd, p + f"stages.{i}.{j}")
            y = torch.empty(1, Hs, Hs, 2 * C, dtype=torch.float16, device="cuda")
            H.m_dwln(xin.float().contiguous().cuda(), mb[o + ".dw.w"], mb[o + ".dw.b"], mb[o + ".ln.g"], mb[o + ".ln.b"], y)
            h32 = torch.empty(1, Hs, Hs, 4 * C, device="cuda")
            H.m_pointwise(e, H.M_PW1, y, mb[o + ".pw1.w"], mb[o + ".pw1.b"], h32, C)
            hs = H.m_grn(h32.view(1, Hs * Hs, 4 * C), mb[o + ".grn.g"], mb[o + ".grn.b"]).view(1, Hs, Hs, 8 * C)
            out = xin.float().contiguous().cuda()
            H.m_pointwise(e, H.M_PW2, hs, mb[o + ".pw2.w"], mb[o + ".pw2.b"], out, C)
            errs.append((f"s{i}.{j}", _err(out, x)))
    heads = _head_ref(x.reshape(1, 64, 768), sdd)
    got = H.m_head(x.reshape(1, 64, 768).float().contiguous().cuda(), mb["M.norm.g"], mb["M.norm.b"], mb["M.head.w"], mb["M.head.b"])
    errs.append(("head", _err(got, heads)))
    print("\nM layer by layer on the float64 oracle's inputs (max |d| / max |ref|):")
    for k, v in errs:
        print(f"  {k:6s} {v:.3e}")
    worst = max(errs, key=lambda kv: kv[1])
    assert len(errs) == 1 + 3 + 18 + 1
    assert worst[1] <= 3e-6, worst
