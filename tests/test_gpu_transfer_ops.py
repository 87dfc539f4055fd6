"""T's identity path kernel by kernel against float64: t_style, t_modulate, what cs_set_identity leaves in an engine, and each of the fourteen
AdaptiveSharedWeightConv2d layers through the engine's own routing (cs_op_t_layer), in the default mode and in latency mode.

References are float64 restatements that read the unpacked synthetic state dict (oracle.canonswap_ref.style_vector / modulated_weight on a
.double() state dict, permuted to memory channel order with pack.MEM2REF), so pack._pack_T's blob layouts are checked too.  The gates of the two
precompute kernels are derived (fp32 rounding counts, written out below) and computed in float64 inside the tests; only the MFMA accumulation of
the blend convs is measured (4x the largest value seen on the MI355X over layers and modes, as in test_gpu_dense_motion.py).  Output buffers
carry a sentinel and guard regions; what a kernel must not write is asserted untouched.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hip_ops as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24               # unit roundoff of fp32
SENT16 = 0x7E5A              # fp16 NaN payload: the sentinel of fp16 buffers
SENT32 = 0x7FC5A5A5          # fp32 NaN payload
GUARD = 256
LAYERS = [f"T.b{i}.c{j}" for i in range(7) for j in (1, 2)]


def _key(layer):
    return f"BottleNeck_2d.{layer // 2}.conv{layer % 2 + 1}"


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def tsd(state_dicts):
    return state_dicts["transfer"]


@pytest.fixture(scope="module")
def sdd(tsd):
    return {k: v.double() for k, v in tsd.items()}


@pytest.fixture(scope="module")
def tb(state_dicts_np):
    """pack._pack_T's blobs (numpy)"""
    from canonswap_amd import pack
    out = {}
    pack._pack_T(out, state_dicts_np["transfer"])
    return out


def _ident(seed):
    from canonswap_amd import synth
    return torch.from_numpy(synth.make_identity(seed))[0]


def _guarded(n, dtype):
    """(whole int buffer filled with the sentinel, view of the n payload elements in dtype) with GUARD elements on either side"""
    it, sent = (torch.int16, SENT16) if dtype == torch.float16 else (torch.int32, SENT32)
    buf = torch.full((n + 2 * GUARD,), sent if sent < 2 ** 31 else sent - 2 ** 32, dtype=it, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _guards_intact(buf, n):
    s = int(buf[0])
    return bool(torch.all(buf[:GUARD] == s)) and bool(torch.all(buf[GUARD + n:] == s))


def _spacing16(ref):
    """fp16 spacing in the binade of |ref| (float64 array): 2^(e - 10), 2^-24 below 2^-14"""
    a = np.abs(np.asarray(ref, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(np.maximum(e, -14) - 10)


# ------------------------------------------------------------------------------------------------ t_style
def _style_ref_and_bound(w1, b1, w2, b2, idv, slope=0.2):
    """float64 style = W2 lrelu(W1 id + b1) + b2 of the fp32 operands, and the bound of t_style_kernel's error on it.

    A sequential fp32 fma dot of length n that starts from the bias makes n roundings: |err| <= (n + 1) u (sum |a_i b_i| + |bias|), u = 2^-24
    (n u would do; n + 1 covers the second-order terms).  The leaky ReLU is 1-Lipschitz, so the first layer's bound e1 passes through it
    unchanged; the product with 0.2f adds one rounding and the distance of 0.2f from 0.2 (2^-26 relative): 2 u |h| covers both.  The second layer
    multiplies by the computed hidden values: |err| <= |W2| e_h + (n + 1) u (|W2| (|h| + e_h) + |b2|)."""
    w1, b1, w2, b2, idv = (np.asarray(a, np.float64) for a in (w1, b1, w2, b2, idv))
    pre = w1 @ idv + b1
    e1 = 513 * U * (np.abs(w1) @ np.abs(idv) + np.abs(b1))
    h = np.where(pre > 0, pre, slope * pre)
    eh = e1 + 2 * U * np.abs(h)
    style = w2 @ h + b2
    bound = np.abs(w2) @ eh + 513 * U * (np.abs(w2) @ (np.abs(h) + eh) + np.abs(b2))
    return style, bound, pre


def _fc_parts(fc):
    n = 512 * 512
    return fc[:n].reshape(512, 512), fc[n:n + 512], fc[n + 512:2 * n + 512].reshape(512, 512), fc[2 * n + 512:]


def _run_t_style(idv, fc, nlayers):
    buf, style = _guarded(nlayers * 512, torch.float32)
    H.t_style(idv.cuda().contiguous(), torch.from_numpy(np.ascontiguousarray(fc)).cuda(), style, nlayers)
    torch.cuda.synchronize()
    assert _guards_intact(buf, nlayers * 512), "t_style wrote outside its output"
    out = style.cpu().numpy().astype(np.float64).reshape(nlayers, 512)
    assert np.all(np.isfinite(out)), "t_style left an output unwritten (sentinel) or wrote a non-finite value"
    return out


@pytest.mark.parametrize("nlayers", [1, 14])
@pytest.mark.parametrize("ident", ["unit", "zero", "x100"])
def test_t_style_against_float64(tb, sdd, nlayers, ident):
    """style = fc2(lrelu(fc0(id), 0.2)) per layer within the derived fp32 bound of the float64 oracle (memory channel order); with a zero identity
    the result is fc2(lrelu(b1)) + b2.  Asserted in float64: a slope of 0.01 instead of 0.2 would leave the bound on this input."""
    from canonswap_amd import pack
    from oracle import canonswap_ref as O
    idv = {"unit": _ident(7), "zero": torch.zeros(512), "x100": _ident(11) * 100}[ident]
    names = LAYERS[:nlayers] if nlayers == 14 else [LAYERS[5]]
    got = _run_t_style(idv, np.concatenate([tb[n + ".fc"] for n in names]), nlayers)
    for k, n in enumerate(names):
        layer = LAYERS.index(n)
        ref, bound, pre = _style_ref_and_bound(*_fc_parts(tb[n + ".fc"]), idv.numpy())
        orc = O.style_vector(sdd, _key(layer), idv.double()[None])[0].numpy()[pack.MEM2REF]
        assert np.abs(orc - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), "the blob's float64 restatement is not the oracle's style"
        err = np.abs(got[k] - orc)
        print(f"\nt_style {n} {ident}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}, max |style| {np.abs(orc).max():.3f}")
        assert np.all(err <= bound), (n, float(np.max(err / bound)))
        if ident == "zero":
            b1 = np.asarray(_fc_parts(tb[n + ".fc"])[1], np.float64)
            assert np.array_equal(pre, b1)
        wrong = _style_ref_and_bound(*_fc_parts(tb[n + ".fc"]), idv.numpy(), slope=0.01)[0]
        assert np.mean(np.abs(wrong - orc) > bound) > 0.9, "this input would not notice a wrong LeakyReLU slope"


def test_t_style_zero_hidden_units_and_both_signs(tb):
    """A layer whose first 64 hidden units are exactly 0 (zero rows of W1, zero b1) next to well populated positive and negative ones: the zeros
    contribute nothing whatever the slope, the negative half carries the factor 0.2."""
    fc = tb[LAYERS[8] + ".fc"].copy()
    w1, b1, w2, b2 = _fc_parts(fc)
    w1[:64] = 0
    b1[:64] = 0
    idv = _ident(23) * 3
    ref, bound, pre = _style_ref_and_bound(w1, b1, w2, b2, idv.numpy())
    assert np.all(pre[:64] == 0) and np.mean(pre > 0) > 0.25 and np.mean(pre < 0) > 0.25
    got = _run_t_style(idv, fc, 1)[0]
    err = np.abs(got - ref)
    print(f"\nt_style zero hidden units: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    for slope in (0.01, 0.0, 1.0):
        wrong = _style_ref_and_bound(w1, b1, w2, b2, idv.numpy(), slope=slope)[0]
        assert np.mean(np.abs(wrong - ref) > bound) > 0.9, slope


# ------------------------------------------------------------------------------------------------ t_modulate
RHO = 20 * U


def _modulate_ref(raw, style, eps=1e-8):
    """float64 w[o][t][i] s[i] / sqrt(sum_{t, i} (w s)^2 + eps) of the fp32 operands; also the row sums of squares"""
    m = np.asarray(raw, np.float64) * np.asarray(style, np.float64)[None, None, :]
    ss = (m * m).reshape(512, -1).sum(1)
    return m / np.sqrt(ss + eps)[:, None, None], ss


def _modulate_gate(ref):
    """|got - ref| <= 1/2 spacing16(ref) + RHO |ref|, RHO = 20 u, first-order rounding count of t_modulate_kernel (u = 2^-24):
      the product m = fl(w s)                                              1 u   on m, 2 u on m^2
      18 sequential fma of non-negative terms per thread                  18 u   on the row's sum of squares
      8 levels of the workgroup's tree, each one rounded add               8 u
      the add of the epsilon: one rounding, and 1e-8f is within u of 1e-8  2 u   -> 30 u on (ss + eps)
      the square root halves it                                           15 u
      rsqrtf: 1 ulp of the result (HIP math API accuracy table) <= 2^-23   2 u   -> 17 u on the demodulation factor
      the final product fl(m demod): m's own rounding and one more         2 u   -> 19 u, rounded up to 20 u for the second-order terms.
    The computed fp32 value v = ref (1 + d), |d| <= RHO, is then rounded to fp16: half a spacing of v's binade, which is ref's (when v crosses into
    the next binade it rounds onto the power of two, |got - ref| <= RHO |ref|)."""
    return 0.5 * _spacing16(ref) + RHO * np.abs(ref)


def _unpack_rows(packed, kind):
    """fp16 [144, 1024, 32] (numpy) -> [512 o][9 taps][512 i] of the kind-0 (W) or kind-1 (w_mod) rows"""
    v = packed[:, H.t_rows(kind), :].reshape(16, 9, 512, 32)           # [chunk][tap][o][kk]
    return np.ascontiguousarray(v.transpose(2, 1, 0, 3)).reshape(512, 9, 512)


def _run_t_modulate(raw, style):
    """-> (modulated rows as float64 [512, 9, 512], their bit patterns uint16); checks the sentinel on every row the kernel must not write"""
    n = 144 * 1024 * 32
    buf, packed = _guarded(n, torch.float16)
    H.t_modulate(torch.from_numpy(np.ascontiguousarray(raw, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(style, np.float32)).cuda(),
                 packed.view(144, 1024, 32))
    torch.cuda.synchronize()
    assert _guards_intact(buf, n), "t_modulate wrote outside the packed set"
    bits = buf[GUARD:GUARD + n].cpu().numpy().view(np.uint16).reshape(144, 1024, 32)
    assert np.all(_unpack_rows(bits, 0) == SENT16), "t_modulate wrote a shared-W row (kind 0)"
    mb = _unpack_rows(bits, 1)
    assert not np.any(mb == SENT16), "t_modulate left a modulated element unwritten"
    return mb.view(np.float16).astype(np.float64), mb


def _check_modulate(what, raw, style):
    got, bits = _run_t_modulate(raw, style)
    ref, ss = _modulate_ref(raw, style)
    assert np.all(np.isfinite(got))
    ex = np.abs(got - ref) - 0.5 * _spacing16(ref)
    nz = np.abs(ref) > 0
    rel = float(np.max(ex[nz] / np.abs(ref[nz]))) / U if nz.any() else 0.0
    ulp = float(np.max(np.abs(got - ref) / _spacing16(ref)))
    print(f"\nt_modulate {what}: max err {ulp:.4f} fp16 spacings; max (|d| - spacing / 2) / |ref| = {rel:.2f} u (gate {RHO / U:.0f} u); "
          f"row sums of squares {ss.min():.3e} .. {ss.max():.3e}")
    assert np.all(np.abs(got - ref) <= _modulate_gate(ref)), (what, rel)
    return got, ref, ss, bits


@pytest.fixture(scope="module")
def kernel_styles(tb):
    """the fp32 styles t_style_kernel computes for identity 7, per layer [14, 512]"""
    return _run_t_style(_ident(7), np.concatenate([tb[n + ".fc"] for n in LAYERS]), 14).astype(np.float32)


@pytest.mark.parametrize("layer", [0, 7, 13])
def test_t_modulate_real_layers(tb, kernel_styles, layer):
    _check_modulate(LAYERS[layer], tb[LAYERS[layer] + ".raw"], kernel_styles[layer])


def test_t_modulate_zero_style(tb):
    """style == 0: every product is a zero, the sum 0, the factor rsqrt(1e-8) = 1e4: every output the bit pattern of +0, none a NaN"""
    raw = tb[LAYERS[2] + ".raw"]
    got, bits = _run_t_modulate(raw, np.zeros(512, np.float32))
    assert np.all(got == 0) and not np.any(np.isnan(got))
    assert np.all(bits == 0)


def test_t_modulate_epsilon_decides(tb, kernel_styles):
    """The style scaled so that a row's sum of squares is about 1e-8: the epsilon is half of the denominator.  Asserted in float64: 1e-5 or 0 in its
    place leaves the gate on this input."""
    raw = tb[LAYERS[4] + ".raw"]
    s0 = kernel_styles[4].astype(np.float64)
    ss0 = _modulate_ref(raw, s0)[1]
    style = (s0 * np.sqrt(1e-8 / np.median(ss0))).astype(np.float32)
    got, ref, ss, _ = _check_modulate("epsilon", raw, style)
    assert 0.2e-8 < ss.min() and ss.max() < 5e-8
    for eps in (1e-5, 0.0):
        assert np.mean(np.abs(_modulate_ref(raw, style, eps)[0] - ref) > _modulate_gate(ref)) > 0.5, eps


def test_t_modulate_huge_style(tb, kernel_styles):
    """|style| = 1e10 (signs of the real style): the sums of squares are about 1e18, finite in fp32"""
    raw = tb[LAYERS[9] + ".raw"]
    style = (np.where(kernel_styles[9] < 0, -1.0, 1.0) * 1e10).astype(np.float32)
    _, _, ss, _ = _check_modulate("1e10", raw, style)
    assert 1e17 < ss.min() and ss.max() < 1e20


def test_t_modulate_one_channel(tb):
    raw = tb[LAYERS[11] + ".raw"]
    style = np.zeros(512, np.float32)
    style[37] = 0.7
    got, ref, _, _ = _check_modulate("one channel", raw, style)
    live = np.zeros((9, 512), bool)
    live[:, 37] = True
    assert np.all(got[:, ~live] == 0) and np.mean(got[:, live] != 0) > 0.99


def test_t_modulate_row_scales_and_subnormals():
    """Random weights whose rows carry the scales 2^(o mod 16 - 32): for the small rows the epsilon is the whole denominator and the outputs are fp16
    subnormals, the large ones are normalised; every row, tap and channel has its own value, so no permutation of them can hide."""
    r = np.random.Generator(np.random.PCG64(515))
    raw = (r.standard_normal((512, 9, 512)) * np.exp2(np.arange(512) % 16 - 32.0)[:, None, None]).astype(np.float32)
    style = r.standard_normal(512).astype(np.float32)
    got, ref, _, _ = _check_modulate("row scales", raw, style)
    sub = (np.abs(ref) < 2.0 ** -14) & (np.abs(ref) >= 2.0 ** -25)
    assert sub.mean() > 0.2 and np.mean(got[sub] != 0) > 0.9
    assert np.abs(ref).max() > 2e-2


# ------------------------------------------------------------------------------------------------ cs_set_identity on the engine
SLOTS = {0: 7, 3: 8, 7: 9}          # identity slot -> identity seed


def _read_sets(eng, slot):
    return [H.t_read(eng, l, slot, H.T_WSET) for l in range(14)]


def _read_styles(eng, slot):
    return torch.stack([H.t_read(eng, l, slot, H.T_STYLE) for l in range(14)]).cpu().numpy()


@pytest.fixture(scope="module")
def eng(state_dicts):
    """An engine with identities in slots 0, 3 and 7; records what each cs_set_identity call left behind"""
    from canonswap_amd.engine import Engine
    e = Engine(0, max_batch=8)
    e.load_state_dicts(state_dicts)
    rec = {"unset_error": None, "styles": {}, "sets0_before": None}
    try:
        H.t_read(e, 0, 0, H.T_WSET)
    except RuntimeError as ex:
        rec["unset_error"] = str(ex)
    for slot, seed in SLOTS.items():
        if slot == 3:
            rec["sets0_before"] = _read_sets(e, 0)
        e.set_identity(_ident(seed), slot)
        rec["styles"][slot] = _read_styles(e, slot)
    torch.cuda.synchronize()
    e.rec = rec
    yield e
    e.close()


def test_unset_slot_is_an_error(eng):
    assert eng.rec["unset_error"] and "slot 0" in eng.rec["unset_error"]
    for slot in (1, 2, 4, 6):
        with pytest.raises(RuntimeError, match=f"slot {slot}"):
            H.t_read(eng, 3, slot, H.T_WSET)
        with pytest.raises(RuntimeError, match=f"slot {slot}"):
            H.t_read(eng, 3, slot, H.T_STYLE)
    with pytest.raises(RuntimeError):
        H.t_read(eng, 14, 0, H.T_WSET)
    x = torch.zeros(1, 64, 64, 512, dtype=torch.float16, device="cuda")
    tm = torch.zeros(1, 64, 64, 4, device="cuda")
    with pytest.raises(RuntimeError, match="slot 6"):
        H.t_layer(eng, 0, [6], x, None, tm, torch.empty_like(x), None)


@pytest.mark.parametrize("slot", list(SLOTS))
def test_set_identity_all_layers(eng, tb, sdd, slot):
    """Per layer: the style read back within t_style's bound of the oracle; the modulated rows within t_modulate's gate of float64 applied to that
    style; the W rows the bits of pack's shared weights; and against the oracle's modulated_weight directly the t_modulate gate plus the style
    bound pushed through the quotient (first order: |W| demod ds_i + |ref| sum |m W| ds / (ss + eps), times 1.01 for the higher orders).
    Measured on the MI355X: at most 1.007 fp16 spacings from the oracle over the three identities and fourteen layers
    (0.70 for an fp32 numpy restatement, whose pairwise sums leave a smaller error in the style)."""
    from canonswap_amd import pack
    from oracle import canonswap_ref as O
    idv = _ident(SLOTS[slot])
    worst = 0.0
    for l, n in enumerate(LAYERS):
        style = eng.rec["styles"][slot][l]
        sref, sbound, _ = _style_ref_and_bound(*_fc_parts(tb[n + ".fc"]), idv.numpy())
        orc_s = O.style_vector(sdd, _key(l), idv.double()[None])[0].numpy()[pack.MEM2REF]
        assert np.abs(orc_s - sref).max() <= 1e-12 * max(1.0, np.abs(sref).max())
        assert np.all(np.abs(style.astype(np.float64) - orc_s) <= sbound), (n, "style")
        bits = H.t_read(eng, l, slot, H.T_WSET).cpu().numpy().view(np.uint16)
        assert np.array_equal(_unpack_rows(bits, 0), _unpack_rows(tb[n + ".w"].view(np.uint16), 0)), (n, "shared W rows")
        got = _unpack_rows(bits, 1).view(np.float16).astype(np.float64)
        raw = tb[n + ".raw"]
        ref, ss = _modulate_ref(raw, style)
        assert np.all(np.abs(got - ref) <= _modulate_gate(ref)), (n, "modulated rows against float64 of the read-back style")
        orc = O.modulated_weight(sdd, _key(l), idv.double()[None])[0].numpy()[pack.MEM2REF][:, pack.MEM2REF].transpose(0, 2, 3, 1).reshape(512, 9, 512)
        w = np.abs(raw.astype(np.float64))
        dem = 1.0 / np.sqrt(ss + 1e-8)
        m = w * np.abs(orc_s)[None, None, :]
        push = w * dem[:, None, None] * sbound[None, None, :] + np.abs(orc) * (((m * w).sum(1) @ sbound) / (ss + 1e-8))[:, None, None]
        err = np.abs(got - orc)
        ulp = float(np.max(err / _spacing16(orc)))
        worst = max(worst, ulp)
        assert np.all(err <= _modulate_gate(orc) + 1.01 * push), (n, "modulated rows against the oracle", ulp)
    print(f"\ncs_set_identity slot {slot}: modulated rows at most {worst:.3f} fp16 spacings from the oracle's modulated_weight")


def test_slots_do_not_disturb_each_other(eng):
    """Setting slot 3 (and 7) left slot 0's fourteen sets as they were; the same identity set into another slot gives the same bits"""
    now = _read_sets(eng, 0)
    for l in range(14):
        assert torch.equal(now[l].view(torch.int16), eng.rec["sets0_before"][l].view(torch.int16)), l
    eng.set_identity(_ident(SLOTS[3]), 5)
    try:
        for l in range(14):
            a, b = H.t_read(eng, l, 3, H.T_WSET), H.t_read(eng, l, 5, H.T_WSET)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), l
            assert not torch.equal(a.view(torch.int16), now[l].view(torch.int16))
        assert np.array_equal(_read_styles(eng, 5), eng.rec["styles"][3])
    finally:
        eng.set_identity(_ident(SLOTS[7]), 7)          # the style buffer holds slot 7's again, as the other tests found it


# ------------------------------------------------------------------------------------------------ the fourteen blend layers
# max |got - ref| / max |ref| per output tensor, measured on the MI355X over the 14 layers, every configuration and sample (the largest per
# mode; the layers lie within 1.3x of one another):
#   mask (fp32, the same kernel in both modes)                             1.21e-07
#   fp32 stream of the conv2 layers                 default 3.43e-07,  latency 1.38e-07 (conv_lat adds twelve shorter partial sums)
#   fp16 outputs, beyond half a spacing of float64  default 4.86e-07,  latency 2.59e-07
# gates: 4 x the largest of each line - seed and layer variation, and still two orders of magnitude under the 3e-4 the whole stage is held to
GATE_MASK = 4.9e-7
GATE_F32 = 1.4e-6
GATE_F16X = 2.0e-6


@pytest.fixture(scope="module")
def captured(tsd):
    """The inputs of the 14 layers as the oracle's own T computes them for two samples and two identities, through its q hook:
    -> x0 [2, 512, 64, 64] and the hooked tensors [relu(y_0), x_1, relu(y_1), x_2, ...] (reference channel order, fp32)"""
    from oracle import canonswap_ref as O
    r = np.random.Generator(np.random.PCG64(4242))
    x = torch.from_numpy((0.08 * r.standard_normal((2, 32, 16, 64, 64))).astype(np.float32))
    ids = torch.stack([_ident(SLOTS[0]), _ident(SLOTS[3])])
    seen = []

    def q(t):
        if len(seen) < 14:
            seen.append(t.detach().clone())
        return t
    with torch.no_grad():
        O.transfer(tsd, x, ids, q=q)
    return x.reshape(2, 512, 64, 64), seen


def _mem(t):
    """[B, 512 (reference order), 64, 64] -> [B, 64, 64, 512 (memory order)] contiguous"""
    from canonswap_amd import pack
    return t[:, torch.from_numpy(pack.MEM2REF)].permute(0, 2, 3, 1).contiguous()


def _layer_io(captured, layer):
    """(fp16 input, fp32 residual or None) of a layer in the engine's layout, on the device"""
    x0, seen = captured
    blk = layer // 2
    xin = x0 if blk == 0 else seen[2 * blk - 1]
    if layer % 2 == 0:
        return _mem(xin).half().cuda(), None
    return _mem(seen[2 * blk]).half().cuda(), _mem(xin).cuda()


def _conv64(x, w):
    """float64 3x3 'same' conv on the device as one GEMM: x [64, 64, 512] , w [O, 9, 512] -> [64, 64, O]"""
    xp = F.pad(x.permute(2, 0, 1), (1, 1, 1, 1))                                       # [512, 66, 66]
    cols = torch.stack([xp[:, ky:ky + 64, kx:kx + 64] for ky in range(3) for kx in range(3)])      # [9, 512, 64, 64]
    return (w.reshape(w.shape[0], 9 * 512) @ cols.reshape(9 * 512, 4096)).t().reshape(64, 64, -1)


class LayerRef:
    """float64 reference of one layer for one sample: the fp16 input, the W / w_mod rows read back from the engine, the fp16 mask weights"""

    def __init__(self, eng, tb, layer, slot, x16, res32):
        n = LAYERS[layer]
        st = H.t_read(eng, layer, slot, H.T_WSET).cpu().numpy()
        wf = torch.from_numpy(np.concatenate([_unpack_rows(st, 0), _unpack_rows(st, 1)]).astype(np.float64)).cuda()      # [1024][9][512]
        from canonswap_amd import pack
        wm = pack.unpack_conv(tb[n + ".mask.w"], 1, 512, 1, 3, 3)[0, :, 0]                  # [512][3][3]
        wm = torch.from_numpy(wm.astype(np.float64)).permute(1, 2, 0).reshape(1, 9, 512).cuda()
        x = x16.double()
        y = _conv64(x, wf)
        bias = torch.from_numpy(tb[n + ".bias"].astype(np.float64)).cuda()
        self.mask = torch.sigmoid(_conv64(x, wm)[..., 0] + float(tb[n + ".mask.b"][0]))
        m = self.mask[..., None]
        self.blend = m * (y[..., 512:] + bias) + (1 - m) * y[..., :512]
        if layer % 2 == 0:
            self.out32 = None
            self.out16 = F.relu(self.blend)
        else:
            self.out32 = res32.double() + self.blend
            self.out16 = self.out32
            if layer == 13:
                s, t = (torch.from_numpy(a.astype(np.float64)).cuda() for a in (tb["T.pre0.s"], tb["T.pre0.t"]))
                self.pre_s = s
                self.out16 = F.relu(self.out32 * s + t)


def _run_layer(eng, layer, slots, x16, res32):
    """cs_op_t_layer with sentinel-filled, guarded outputs -> (mask [B, 64, 64], out16, out32 or None)"""
    B = x16.shape[0]
    n = B * 4096 * 512
    mbuf, tm = _guarded(B * 4096 * 4, torch.float32)
    obuf, o16 = _guarded(n, torch.float16)
    fbuf, o32 = _guarded(n, torch.float32) if res32 is not None else (None, None)
    tm4 = tm.view(B, 64, 64, 4)
    H.t_layer(eng, layer, slots, x16, res32, tm4, o16.view(B, 64, 64, 512), None if o32 is None else o32.view(B, 64, 64, 512))
    torch.cuda.synchronize()
    assert _guards_intact(mbuf, B * 4096 * 4) and _guards_intact(obuf, n) and (fbuf is None or _guards_intact(fbuf, n)), "a T layer wrote outside its outputs"
    raw = mbuf[GUARD:GUARD + B * 4096 * 4].view(B, 64, 64, 4)
    assert torch.all(raw[..., 1:] == raw[0, 0, 0, 1]) and int(raw[0, 0, 0, 1]) == int(mbuf[0]), "t_mask wrote elements 1 .. 3 of a group"
    assert not torch.any(obuf[GUARD:GUARD + n] == SENT16) and not torch.any(torch.isnan(tm4[..., 0]))
    if o32 is not None:
        assert not torch.any(torch.isnan(o32))
    return tm4, o16.view(B, 64, 64, 512), None if o32 is None else o32.view(B, 64, 64, 512)


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _f16_excess(got, ref):
    """max (|got - ref| - half an fp16 spacing of ref) / max |ref|"""
    a = ref.abs().clamp_min(2.0 ** -14)
    half = torch.exp2(torch.floor(torch.log2(a)) - 11)
    return float(((got.double() - ref).abs() - half).max() / ref.abs().max())


def _explicit(eng, tb, layer, slot, x16, res32, tm4, cfg):
    """The same layer for one sample as one cs_op_conv launch of the named kernel on the slot's read-back set -> (out16, out32)"""
    n = LAYERS[layer]
    wset = H.t_read(eng, layer, slot, H.T_WSET)
    bias = torch.from_numpy(tb[n + ".bias"]).cuda()
    o16 = torch.zeros(1, 1, 64, 64, 512, dtype=torch.float16, device="cuda")
    xin = x16.view(1, 1, 64, 64, 512)
    if layer % 2 == 0:
        H.conv(xin, wset, 1024, 512, (1, 3, 3), bias=bias, pixscale=tm4, ps_stride=4, act0="relu", out0=o16, mode=1, cfg=cfg)
        o32 = None
    else:
        o32 = torch.zeros(1, 1, 64, 64, 512, dtype=torch.float32, device="cuda")
        kw = {}
        if layer == 13:
            kw = dict(s2=torch.from_numpy(tb["T.pre0.s"]).cuda(), t2=torch.from_numpy(tb["T.pre0.t"]).cuda(), act1="relu")
        H.conv(xin, wset, 1024, 512, (1, 3, 3), bias=bias, pixscale=tm4, ps_stride=4, res=res32.view(1, 1, 64, 64, 512), out0=o32, out1=o16,
               mode=1, cfg=cfg, **kw)
    torch.cuda.synchronize()
    return o16[0, 0], None if o32 is None else o32[0, 0]


def _bits_equal(a, b):
    if a is None and b is None:
        return True
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _check_sample(what, ref, mask, o16, o32, layer, measured):
    assert float(ref.blend.abs().max()) > 1e-2 and float(ref.mask.max() - ref.mask.min()) > 1e-2, (what, "a trivial input")
    em = _rel(mask, ref.mask)
    ex = _f16_excess(o16, ref.out16)
    measured["mask"].append(em); measured["f16x"].append(ex)
    line = f"\n{what}: mask {em:.3e}, fp16 excess {ex:.3e}"
    if o32 is not None:
        e32 = _rel(o32, ref.out32)
        measured["f32"].append(e32)
        line += f", fp32 {e32:.3e}"
    print(line, end="")
    assert em <= GATE_MASK, (what, "mask", em)
    assert ex <= GATE_F16X, (what, "fp16 output", ex)
    if o32 is not None:
        assert e32 <= GATE_F32, (what, "fp32 output", e32)
        if layer != 13:      # the fp16 copy is the rounding of the fp32 value the kernel stored
            assert _bits_equal(o16, o32.half())
    if layer % 2 == 0 or layer == 13:
        assert bool(torch.all(o16 >= 0)) and float((o16 == 0).double().mean()) > 0.05, (what, "ReLU")


@pytest.mark.parametrize("layer", range(14))
def test_blend_layer_default_mode(eng, tb, captured, layer):
    """One layer on the oracle's own input at B = 2 with mixed slots (0, 3), at B = 8 (conv_wide; samples repeated, slots mixed) and at B = 1:
    mask, fp32 stream and fp16 output of every sample at every position (borders included) against float64; B = 2 is the bits of conv_halo's
    128 x 128 tiles on the read-back set, of the same samples run one slot per call, and B = 8 the bits of B = 1 per sample."""
    x16, res32 = _layer_io(captured, layer)
    measured = {"mask": [], "f32": [], "f16x": []}
    slots = [0, 3]
    refs = [LayerRef(eng, tb, layer, slots[b], x16[b], None if res32 is None else res32[b]) for b in range(2)]
    tm, o16, o32 = _run_layer(eng, layer, slots, x16, res32)
    one = []
    for b in range(2):
        _check_sample(f"{LAYERS[layer]} B=2 sample {b} slot {slots[b]}", refs[b], tm[b, ..., 0], o16[b], None if o32 is None else o32[b], layer, measured)
        r = None if res32 is None else res32[b:b + 1].contiguous()
        t1, a16, a32 = _run_layer(eng, layer, [slots[b]], x16[b:b + 1].contiguous(), r)
        assert _bits_equal(t1[0], tm[b]) and _bits_equal(a16[0], o16[b]) and _bits_equal(None if a32 is None else a32[0], None if o32 is None else o32[b]), \
            (b, "a sample of a mixed batch differs from the sample run alone with its slot")
        e16, e32 = _explicit(eng, tb, layer, slots[b], x16[b], None if res32 is None else res32[b], tm[b:b + 1].contiguous(), 10)
        assert _bits_equal(e16, o16[b]) and _bits_equal(e32, None if o32 is None else o32[b]), (b, "not the bits of conv_halo's 128 x 128 tiles")
        one.append((t1[0], a16[0], None if a32 is None else a32[0]))
    # swapped slots are another result (the per-sample slot is really read)
    _, s16, _ = _run_layer(eng, layer, [3, 0], x16, res32)
    assert not _bits_equal(s16[0], o16[0]) and not _bits_equal(s16[1], o16[1])
    # B = 8: sample k is input k % 2 with slot pattern (0, 3, 3, 0, 7, 0, 3, 7)
    pat = [0, 3, 3, 0, 7, 0, 3, 7]
    x8 = x16.repeat(4, 1, 1, 1)
    r8 = None if res32 is None else res32.repeat(4, 1, 1, 1)
    tm8, p16, p32 = _run_layer(eng, layer, pat, x8, r8)
    for k in (0, 1):                  # slots as at B = 2: the same bits
        assert _bits_equal(tm8[k], one[k][0]) and _bits_equal(p16[k], one[k][1]) and _bits_equal(None if p32 is None else p32[k], one[k][2]), \
            (k, "B = 8 differs from B = 1")
    for k in (2, 4, 5, 7):
        rk = None if res32 is None else res32[k % 2:k % 2 + 1].contiguous()
        t1, a16, a32 = _run_layer(eng, layer, [pat[k]], x16[k % 2:k % 2 + 1].contiguous(), rk)
        assert _bits_equal(tm8[k], t1[0]) and _bits_equal(p16[k], a16[0]) and _bits_equal(None if p32 is None else p32[k], None if a32 is None else a32[0]), \
            (k, "B = 8 differs from B = 1")
    ref7 = LayerRef(eng, tb, layer, 7, x16[0], None if res32 is None else res32[0])
    _check_sample(f"{LAYERS[layer]} B=8 sample 4 slot 7", ref7, tm8[4, ..., 0], p16[4], None if p32 is None else p32[4], layer, measured)
    print(f"\n{LAYERS[layer]} default: worst mask {max(measured['mask']):.3e} fp32 {max(measured['f32'] or [0]):.3e} fp16x {max(measured['f16x']):.3e}")


@pytest.mark.parametrize("layer", range(14))
def test_blend_layer_latency_mode(eng, tb, captured, layer):
    """The same layer at B = 1 in latency mode (conv_lat: another summation order): both samples against float64, and the bits of the explicit
    conv_lat launch on the read-back set."""
    x16, res32 = _layer_io(captured, layer)
    measured = {"mask": [], "f32": [], "f16x": []}
    eng._call("cs_set_latency_mode", 1)
    try:
        for b, slot in ((0, 0), (1, 3)):
            r = None if res32 is None else res32[b:b + 1].contiguous()
            tm, o16, o32 = _run_layer(eng, layer, [slot], x16[b:b + 1].contiguous(), r)
            ref = LayerRef(eng, tb, layer, slot, x16[b], None if res32 is None else res32[b])
            _check_sample(f"{LAYERS[layer]} latency sample {b} slot {slot}", ref, tm[0, ..., 0], o16[0], None if o32 is None else o32[0], layer, measured)
            e16, e32 = _explicit(eng, tb, layer, slot, x16[b], None if res32 is None else res32[b], tm, 32)
            assert _bits_equal(e16, o16[0]) and _bits_equal(e32, None if o32 is None else o32[0]), (b, "not the bits of conv_lat")
    finally:
        eng._call("cs_set_latency_mode", 0)
    print(f"\n{LAYERS[layer]} latency: worst mask {max(measured['mask']):.3e} fp32 {max(measured['f32'] or [0]):.3e} fp16x {max(measured['f16x']):.3e}")
