"""Pins tests/spade_ref.py - the float64 restatement test_gpu_spade_decoder.py measures the engine's SPADE decoder against - and shows that the
gates of that test bite.  No GPU: an 8 x 8 seg (up blocks at 16 x 16 and 32 x 32), the stand-in for the engine is the same step in torch fp32."""
import numpy as np
import pytest
import torch

import spade_ref as S
from canonswap_amd import pack
from oracle import canonswap_ref as O


@pytest.fixture(scope="module")
def gsd(state_dicts):
    return state_dicts["spade_generator"]


@pytest.fixture(scope="module")
def seg():
    r = np.random.Generator(np.random.PCG64(77))
    return torch.from_numpy((0.5 * r.standard_normal((1, 256, 8, 8))).astype(np.float16).astype(np.float64))


@pytest.fixture(scope="module")
def blobs(gsd):
    out = {}
    pack._pack_G(out, pack._np_sd(gsd))
    return out


@pytest.fixture(scope="module")
def stand_in(gsd, seg):
    return S.run_steps(S.GWeights(gsd), seg)


def test_chained_steps_equal_the_oracle(gsd, seg):
    """float64, unrounded weights: the chain of steps (strided phase form of mlp_shared, composed .bs / .ng / .cs shortcut, SPADE on the up-sampled
    x with the half-size statistics) is oracle.canonswap_ref.spade_decoder"""
    sd64 = {k: v.double() for k, v in gsd.items()}
    want = O.spade_decoder(sd64, seg)
    got, t = S.chain(seg, S.GWeights(gsd, rounded=False))
    assert got.shape == want.shape == (1, 3, 64, 64)
    assert (got - want).abs().max().item() < 1e-12
    # ... and step by step where the forms differ: mlp_shared on the resized seg, the shortcut in the reference's order
    W = S.GWeights(gsd, rounded=False)
    for grp, s in (("G.shared128", 2), ("G.shared256", 4)):
        w, b = W.shared(grp)
        plain = torch.relu(torch.nn.functional.conv2d(O.nearest_up(seg, 1, s, s), w, b, padding=1))
        assert (S.step_shared(seg, W, grp, s) - plain).abs().max().item() < 1e-12
    x, sx, a = t["G_middle_5.c1"], S.chan_stats(t["G_middle_5.c1"]), t["shared128"][:, 256:384]
    assert (t["up_0.cs"] - S.shortcut_reference(x, sx, a, W, "up_0")).abs().max().item() < 1e-12
    # nearest up-sampling leaves the statistics as they are
    for u, v in zip(S.chan_stats(O.nearest_up(x, 1, 2, 2)), sx):
        assert (u - v).abs().max().item() < 1e-12


@pytest.mark.parametrize("grp,s", [("G.shared128", 2), ("G.shared256", 4)])
def test_phase_replay_equals_the_resized_conv(gsd, seg, blobs, grp, s):
    """run_G's bookkeeping replayed from _pack_G's blobs (rounded phase sums; no a = 2 phase at x4, its row written by a = 1; the duplicated middle
    pixel) writes every element, and what it writes is the 3x3 conv on the resized seg with the same rounded sums"""
    got = S.shared_replay(seg[0].numpy(), blobs, grp, s)
    assert not np.isnan(got).any()
    want = S.step_shared(seg, S.GWeights(gsd), grp, s)[0].numpy()
    assert np.abs(got - want).max() < 1e-12
    if s == 4:
        assert np.array_equal(got[:, 1::4], got[:, 2::4])


def _frac(got, label, stand_in):
    R, E32, _, _, f16 = stand_in[0][label]
    return S.used(got, R, S.gate(R, E32, f16))[0]


def test_stand_in_passes_every_gate(stand_in):
    res, _ = stand_in
    assert len(res) == 4 + 6 * 4 + 7 + 6 + 1
    for label, (R, E32, stored, s, f16) in res.items():
        fr = S.used(stored, R, S.gate(R, E32, f16))[0]
        assert fr <= 1.0, (label, fr)
        if s > 1:      # (the 64 x 64 maps are 8 x 8 here: all border)
            bd = S.breakdown(stored, R, S.gate(R, E32, f16), s)
            assert max(bd["interior"], bd["top"], bd["bottom"], bd["left"], bd["right"], *bd["phases"].values()) == fr


def test_mutation_dropped_chunk(gsd, stand_in):
    _, T = stand_in
    W = S.GWeights(gsd)
    bad = S.step_conv(T["h0.0"].float(), W.spectral("G_middle_0.conv_0"), drop_chunk=5)
    assert _frac(bad.half(), "G.m0.c0", stand_in) > 1.0


def test_mutation_phase_padding(seg, blobs, stand_in):
    bad = S.shared_replay(seg[0].numpy(), blobs, "G.shared256", 4, pad_shift=(0, 3))
    assert _frac(torch.from_numpy(bad)[None].half(), "G.shared256", stand_in) > 1.0
    good = S.shared_replay(seg[0].numpy(), blobs, "G.shared256", 4)
    assert _frac(torch.from_numpy(good)[None].half(), "G.shared256", stand_in) <= 1.0


def test_mutation_duplicate_row(seg, blobs, stand_in):
    """the x4 duplicate of row 4 i + 1 written to 4 i + 3: row 4 i + 2 is never written (the sentinel stays), the gate is exceeded there"""
    bad = torch.from_numpy(S.shared_replay(seg[0].numpy(), blobs, "G.shared256", 4, dup_row=3))[None]
    assert torch.isnan(bad[:, :, 2::4]).all() and not torch.isnan(bad[:, :, 3::4]).any()
    R, E32, _, s, f16 = stand_in[0]["G.shared256"]
    g = S.gate(R, E32, f16)
    assert S.used(bad, R, g)[0] > 1.0
    assert S.breakdown(bad, R, g, s)["phase"][0] == 2


def test_mutation_statistics_of_the_previous_block(gsd, stand_in):
    _, T = stand_in
    W = S.GWeights(gsd)
    bad = S.step_spade(T["x.1"].float(), T["sx.0"], T["a64"][:, 256:384].float(), W.gb("G_middle_1.norm_0"))
    assert _frac(bad.half(), "G.m1.n0", stand_in) > 1.0


def test_mutation_bias_composed_without_ws(gsd, stand_in):
    _, T = stand_in
    W = S.GWeights(gsd)
    for i, p, n, ak in ((6, "up_0", "G.up0.bs", "a128"), (7, "up_1", "G.up1.bs", "a256")):
        bad = S.step_bs(T[ak][:, 256:384].float(), W.shortcut(p, bias_through_ws=False))
        assert _frac(bad.half(), n, stand_in) > 1.0


def test_gate_rule():
    """half an fp16 spacing at |R| plus four times the reference-side fp32 error, elementwise"""
    R = torch.tensor([[[[1.0, 1000.0, 3e-6, -0.75]]]], dtype=torch.float64)
    E = R + torch.tensor([1e-7, -2e-7, 0.0, 0.0], dtype=torch.float64)
    g = S.gate(R, E)
    assert torch.allclose(g, 8e-7 + 0.5 * torch.tensor([2.0 ** -10, 2.0 ** -1, 2.0 ** -24, 2.0 ** -11], dtype=torch.float64), rtol=1e-5, atol=0)
    assert torch.allclose(S.gate(R, E, fp16_out=False), torch.full_like(R, 8e-7), rtol=1e-5, atol=0)
