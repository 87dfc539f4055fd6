"""Pins tests/volume_ref.py - the float64 restatement test_gpu_volume_path.py measures the engine's F and R against - and shows that the gates of
that test bite.  No GPU.  Most tests run a 32 x 32 image (an 8 x 8 x 16 volume): the stand-in for the engine is the same step in torch fp32, for
the elementwise GroupNorm steps the kernel's own fp32 operation sequence (volume_ref.gn_engine).  One test runs one 256 x 256 frame:

test_chains_against_the_fp32_oracle_on_one_frame: the float64 chains with unrounded weights against oracle.canonswap_ref in fp32, the distance
being the oracle's own fp32 error.  Computed once (frame synth.make_frame_inputs(1, seed=2200), R on the oracle's F of it): relative L2
2.40e-7 for F and 2.18e-6 for R, largest element 4.65e-7 (of 1.28) and 3.25e-5 (of 10.25); the test asserts four times the relative L2 figures."""
import pytest
import torch

import spade_ref as S
import volume_ref as V
from canonswap_amd import synth
from oracle import canonswap_ref as O

ORACLE_FP32_REL = {"F": 2.40e-7, "R": 2.18e-6}      # the module docstring's figures


@pytest.fixture(scope="module")
def sds(state_dicts):
    return state_dicts["appearance_feature_extractor"], state_dicts["refine"]


@pytest.fixture(scope="module")
def W(sds):
    return V.VWeights(*sds)


@pytest.fixture(scope="module")
def img():
    return torch.from_numpy(synth.make_frame_inputs(1, seed=2200, size=256)["img"])[:, :, 96:128, 96:128].contiguous()


@pytest.fixture(scope="module")
def stand_in(W, img):
    """F on the 32 x 32 image, R on F's result: {(label, key): (R, E32, stored, fp16, gate)} and the operands T of each"""
    TF = {"img": img}
    rf = V.run_steps(V.step_list_F(W), TF)
    TR = {"x.in": TF["x.6"], "a.in": TF["x.6"].half()}
    rr = V.run_steps(V.step_list_R(W), TR)
    return rf, TF, rr, TR


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_chains_equal_the_oracle_in_float64(sds, img):
    """float64, unrounded weights: the chained steps (BatchNorm folded into the convs, the next block's norm1 on conv2's epilogue, GroupNorm as
    scale and shift, the 2-D pair on the reshaped volume) are oracle.canonswap_ref.appearance_feature_extractor and .refine"""
    W0 = V.VWeights(*sds, rounded=False)
    sf, sr = ({k: v.double() for k, v in sd.items()} for sd in sds)
    f = O.appearance_feature_extractor(sf, img.double())
    got = V.chain_F(img.double(), W0)
    assert got.shape == f.shape == (1, 32, 16, 8, 8)
    assert (got - f).abs().max().item() < 1e-11 * f.abs().max().item()
    want = O.refine(sr, f)
    assert (V.chain_R(f, W0) - want).abs().max().item() < 1e-11 * want.abs().max().item()


def test_chains_against_the_fp32_oracle_on_one_frame(sds):
    W0 = V.VWeights(*sds, rounded=False)
    frame = torch.from_numpy(synth.make_frame_inputs(1, seed=2200, size=256)["img"])
    f32 = O.appearance_feature_extractor(sds[0], frame)
    f64 = V.chain_F(frame.double(), W0)
    r32 = O.refine(sds[1], f32)
    r64 = V.chain_R(f32.double(), W0)
    for name, a, b in (("F", f32, f64), ("R", r32, r64)):
        rel, mx = _rel(a, b), (a.double() - b).abs().max().item()
        print(f"\n{name}: the fp32 oracle against the float64 chain: relative L2 {rel:.2e}, largest element {mx:.2e} of {b.abs().max().item():.2f}")
        assert rel < 4 * ORACLE_FP32_REL[name]


def test_stand_in_passes_every_gate(stand_in):
    rf, _, rr, _ = stand_in
    assert len(rf) == 17 and len(rr) == 29      # one per stored tensor; the three layout launches are no steps
    for res in (rf, rr):
        for (label, key), (R, E32, stored, f16, g) in res.items():
            if g is None:
                g = S.gate(R, E32, f16)
            assert S.used(stored, R, g)[0] <= 1.0, (label, key)


def test_step_list_order_and_statistics(W):
    """run_R's order: per stage-3 block conv1 (behind block 0 with its write-back entry in front), conv2, each with a statistics key; one
    norm_act per stage; the 2-D pair in between"""
    L = V.step_list_R(W)
    assert [e["label"] for e in L if e["kind"] == "gn"] == ["R.s1.1.c1.sp", "R.s1.2.c1.sp", "norm_act", "R.s3.1.c1.sp", "R.s3.2.c1.sp", "norm_act"]
    assert len([e for e in L if e["st"]]) == 12 and all(e["label"].endswith(".sp") for e in L if e["st"])
    assert [e["label"] for e in L[9:15]] == [f"R.rb2.{i}.c{c}" for i in range(3) for c in (1, 2)]
    assert [e["label"] for e in V.step_list_F(W)] == ["conv_first", "F.down0", "F.down1", "F.second"] + [f"F.rb{i}.c1+c2" for i in range(6)]


@pytest.mark.parametrize("mutation", V.MUTATIONS)
@pytest.mark.parametrize("label,blk,c", [("R.s1.0.c1.sp", "resblocks1", 1), ("R.s3.2.c2.sp", "resblocks3", 2)])
def test_mutation_split_terms(W, stand_in, mutation, label, blk, c):
    """A stage-3 conv without W_lo a_hi, without W_hi a_lo, or on plain fp16 operands exceeds the step's gate"""
    _, _, rr, T = stand_in
    i = int(label.split(".")[2])
    s = label.split(".")[1]
    key = f"{s}.y{c}.{i}"
    R, E32, _, f16, _ = rr[(label, key)]
    if c == 1:
        a = T["x.in"] if (s, i) == ("s1", 0) else T[f"{s}.x.{i}"]
    else:
        w1 = W.s3(blk, i, 1)
        a = V.gn_engine(T[f"{s}.y1.{i}"], T[f"{s}.st1.{i}"], w1[3], w1[4])
    bad = V.s3_conv(a, W.s3(blk, i, c), torch.float32, mutation)
    g = S.gate(R, E32, f16)
    fr = ((bad.double() - R).abs() / g)
    print(f"\n{label} {mutation}: {fr.max().item():.0f} x the gate at the worst element, {100 * (fr > 1).double().mean().item():.0f} % of the elements over")
    assert fr.max().item() > 10.0 and (fr > 1).double().mean().item() > 0.5
    assert S.used(V.s3_conv(a, W.s3(blk, i, c), torch.float32), R, g)[0] <= 1.0


def test_mutation_own_norm1_as_post(W, stand_in):
    """conv2's second output under block i's own norm1 instead of block i + 1's exceeds its gate; the fp32 stream does not change"""
    rf, T, _, _ = stand_in
    for i in (0, 4):
        y, a = V.step_rb3(T[f"a.{i}"].float(), T[f"x.{i}"].float(), W, i, own_post=True)
        label = f"F.rb{i}.c1+c2"
        R, E32, _, f16, _ = rf[(label, f"a.{i + 1}")]
        assert S.used(a.half(), R, S.gate(R, E32, f16))[0] > 1.0
        R, E32, _, f16, _ = rf[(label, f"x.{i + 1}")]
        assert S.used(y, R, S.gate(R, E32, f16))[0] <= 1.0


def test_mutation_second_without_mem2ref(W, stand_in):
    rf, T, _, _ = stand_in
    y, a = V.step_second(T["p1"].float(), W, mem2ref=False)
    for key, bad in (("x.0", y), ("a.0", a.half())):
        R, E32, _, f16, _ = rf[("F.second", key)]
        assert S.used(bad, R, S.gate(R, E32, f16))[0] > 1.0


def test_mutation_unbiased_variance(stand_in):
    """A slot with the unbiased variance misses the statistics tolerances (those of test_chan_stats) on this volume's 1024 positions per channel.
    On the engine's 65536 positions the two rstd differ by 7.6e-6 relative, inside the 1e-4 tolerance: there the slot's divisor is held by the
    float64 statistics only to that tolerance."""
    _, _, _, T = stand_in
    y = T["s1.y1.0"].double()
    m64, r64 = V.vol_stats(y)
    assert V.stats_close(T["s1.st1.0"], m64, r64)
    bad = 1.0 / torch.sqrt(y.var((0, 2, 3, 4), unbiased=True) + V.EPS)
    assert not V.stats_close((m64.float(), bad.float()), m64, r64)


def test_split_bound(sds, W, stand_in):
    """The three-term float64 result lies within the derived bound (volume_ref.split_bound) of the float64 conv of the unrounded operands; every
    synthetic weight is below 2^-3, so W_lo is an fp16 subnormal: the case pack._hi_lo's docstring describes"""
    _, _, _, T = stand_in
    W0 = V.VWeights(*sds, rounded=False)
    a = T["x.in"]
    w0 = W0.s3("resblocks1", 0, 1)
    assert w0[0].abs().max().item() < 2.0 ** -3
    lo = W.s3("resblocks1", 0, 1)[1]
    assert (lo.abs() < 2.0 ** -14).all() and (lo != 0).any()
    d = (V.s3_conv(a, W.s3("resblocks1", 0, 1), torch.float64) - V.s3_conv(a, w0, torch.float64)).abs()
    bound = V.split_bound(a, w0[0])
    print(f"\nresblocks1.0.conv1: the split's error uses at most {(d / bound).max().item():.2f} of its bound")
    assert (d <= bound).all()
    for m in V.MUTATIONS:
        dm = (V.s3_conv(a, W.s3("resblocks1", 0, 1), torch.float64, m) - V.s3_conv(a, w0, torch.float64)).abs()
        assert (dm > bound).any(), m


def test_gn_gate_holds_for_other_fp32_orders(stand_in, W):
    """the rounding-count gate of the elementwise steps also covers the plain fp32 form without fused multiply-adds, and rejects a wrong slope"""
    _, _, _, T = stand_in
    w = W.s3("resblocks1", 0, 2)
    y, st, res = T["s1.y2.0"], T["s1.st2.0"], T["x.in"]
    R, M = V.gn_ref(y, st, w[3], w[4], res)
    g = V.gn_gate(R, M)
    v = (y - st[0].view(1, -1, 1, 1, 1)) * st[1].view(1, -1, 1, 1, 1) * w[3].float().view(1, -1, 1, 1, 1) + w[4].float().view(1, -1, 1, 1, 1) + res
    assert ((V.lrelu(v).double() - R).abs() <= g).all()
    assert ((V.gn_engine(y, st, w[3], w[4], res).double() - R).abs() <= g).all()
    assert not ((torch.nn.functional.leaky_relu(v, 0.2).double() - R).abs() <= g).all()
