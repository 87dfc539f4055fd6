"""The SegFormer face parser, without a GPU: the restatement (tests/parser_ref.py) against the transformers class's recorded outputs
(tests/golden/parser_b2.npz, tools/make_golden_parser.py) and, where the package imports, against the class itself; the packer's spellings,
folds and composed decode head; the C ABI's declarations; and that the GPU tests' tolerance and label check can fail."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parser_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cs_parser", "cs_op_parser_read", "cs_op_parser_input", "cs_op_parser_gemm", "cs_op_parser_layernorm", "cs_op_parser_attention",
                "cs_op_parser_dwgelu", "cs_op_parser_upadd")
GPU_FACTOR = 4.0          # tests/test_gpu_parser.py: the engine may be 4 x the fp16-operand emulation's distance from float64
HEADS = {"num_attention_heads": [1, 2, 5, 8]}


@pytest.fixture(scope="module")
def gold(golden):
    return golden("parser_b2.npz")


@pytest.fixture(scope="module")
def cfg():
    from canonswap_amd import synth
    return dict(synth.PARSER_A)


@pytest.fixture(scope="module")
def sd_np(cfg):
    from canonswap_amd import synth
    return synth._segformer(0, cfg)


@pytest.fixture(scope="module")
def pv(gold):
    from canonswap_amd import synth
    return torch.from_numpy(synth.parser_pixel_values(gold["image_u8"])).double()


@pytest.fixture(scope="module")
def f64(sd_np, cfg, pv):
    with torch.no_grad():
        return R.forward(R.to_tensors(sd_np), cfg, pv)


@pytest.fixture(scope="module")
def emu(sd_np, cfg, pv):
    with torch.no_grad():
        return R.forward(R.to_tensors(sd_np), cfg, pv, emulate=True)


@pytest.fixture(scope="module")
def blobs(sd_np):
    from canonswap_amd import pack
    out = {}
    pack._pack_P(out, sd_np, HEADS)
    return out


def test_restatement_matches_the_recorded_class(gold, f64):
    """The golden holds the class's float64 outputs rounded to fp32 (2^-24 relative per element): measured 2.7e-8 relative L2 at worst, asserted
    at 2e-7.  The stage outputs are recorded as every 16th element plus the norm per image."""
    worst = float(R.rel_l2(f64["logits"], torch.from_numpy(gold["logits"])).max())
    for s in range(4):
        got = f64[f"stage{s}"].reshape(2, -1)
        want = torch.from_numpy(gold[f"stage{s}"]).double()
        worst = max(worst, float(((got[:, ::16] - want).norm(dim=1) / want.norm(dim=1)).max()))
        assert np.allclose(got.norm(dim=1).numpy(), gold[f"stage{s}_norm"], rtol=1e-12)
    print("restatement vs golden, worst relative L2:", worst)
    assert worst <= 2e-7


def test_restatement_matches_the_class_live(sd_np, cfg, pv, f64):
    """Against the installed class in float64 (sdpa attention: the eager path rounds its softmax to fp32): float64 noise, measured 1.4e-15 of the
    largest logit; asserted at 1e-12.  Loading is strict, through pack's rename table: the table is complete."""
    pytest.importorskip("transformers")
    m = R.hf_model(sd_np, cfg)
    with torch.no_grad():
        o = m(pixel_values=pv, output_hidden_states=True)
    err = float((f64["logits"] - o.logits).abs().max() / o.logits.abs().max())
    print("restatement vs transformers, max abs / max |logit|:", err)
    assert err <= 1e-12
    for s in range(4):
        assert float((f64[f"stage{s}"] - o.hidden_states[s]).abs().max()) <= 1e-12 * float(o.hidden_states[s].abs().max()) + 1e-13


def test_both_spellings_pack_to_the_same_blobs(sd_np, blobs):
    from canonswap_amd import pack
    new = pack.parser_rename(sd_np)
    assert set(new) != set(sd_np) and all(k.startswith(("segformer.stages.", "decode_head.")) for k in new)
    out = {}
    pack._pack_P(out, new, HEADS)
    assert set(out) == set(blobs)
    for k in out:
        assert out[k].dtype == blobs[k].dtype and np.array_equal(out[k], blobs[k]), k
    assert blobs["P.cfg"].dtype == np.int32 and blobs["P.cfg"].tolist()[:19] == [1, 1, 2, 1, 64, 128, 320, 512, 1, 2, 5, 8, 8, 4, 2, 1, 4, 768, 19]
    assert float(blobs["P.cfg"][19:].view(np.float32)[0]) == np.float32(1e-5)


def test_missing_and_extra_keys_are_named(sd_np):
    from canonswap_amd import pack
    sd = dict(sd_np)
    del sd["segformer.encoder.block.2.1.mlp.dense2.bias"]
    with pytest.raises(ValueError, match=r"segformer\.stages\.2\.blocks\.1\.mlp\.fc2\.bias"):
        pack._pack_P({}, sd, HEADS)
    sd = dict(sd_np, **{"decode_head.extra.weight": np.zeros(3, np.float32)})
    with pytest.raises(ValueError, match=r"unexpected key 'decode_head\.extra\.weight'"):
        pack._pack_P({}, sd, HEADS)


def test_refused_configs_name_their_reason(sd_np):
    from canonswap_amd import pack
    with pytest.raises(ValueError, match="head dimension 160"):
        pack._pack_P({}, sd_np, {"num_attention_heads": [1, 2, 2, 8]})
    with pytest.raises(ValueError, match="head dimension 16"):
        pack._pack_P({}, sd_np, {"num_attention_heads": [4, 2, 5, 8]})
    # without a config the heads default to C / 64: 1, 2, 5, 8
    out = {}
    assert pack._pack_P(out, sd_np)["heads"] == [1, 2, 5, 8]


def test_scale_is_folded_into_q_and_kv_is_stacked(sd_np, blobs):
    """fp16(W_q d^-1/2) to one rounding; k and v stacked; the depth-wise weights tap-major; the classifier's padded rows are zero."""
    for s, (C, h) in enumerate(((64, 1), (128, 2), (320, 5), (512, 8))):
        b = f"segformer.encoder.block.{s}.0"
        w = sd_np[b + ".attention.self.query.weight"].astype(np.float64) * (C // h) ** -0.5
        got = blobs[f"P.s{s}.b0.q.w"].astype(np.float64)
        assert got.shape == (C, C) and np.all(np.abs(got - w) <= 2.0 ** -11 * np.abs(w) + 2.0 ** -25)
        assert np.allclose(blobs[f"P.s{s}.b0.q.b"], sd_np[b + ".attention.self.query.bias"] * (C // h) ** -0.5, rtol=1e-6)
        kv = blobs[f"P.s{s}.b0.kv.w"]
        assert kv.shape == (2 * C, C)
        assert np.array_equal(kv[:C], sd_np[b + ".attention.self.key.weight"].astype(np.float16))
        assert np.array_equal(kv[C:], sd_np[b + ".attention.self.value.weight"].astype(np.float16))
        dw = blobs[f"P.s{s}.b0.dw.w"]
        assert dw.shape == (9, 4 * C) and np.array_equal(dw[5], sd_np[b + ".mlp.dwconv.dwconv.weight"][:, 0, 1, 2])
        assert (f"P.s{s}.b0.sr.w" in blobs) == (s < 3)
    assert blobs["P.cls.w"].shape == (64, 768) and not blobs["P.cls.w"][19:].any() and not blobs["P.cls.b"][19:].any()
    assert np.array_equal(blobs["P.cls.w"][:19], sd_np["decode_head.classifier.weight"].reshape(19, 768).astype(np.float16))


def test_composed_head_equals_the_uncomposed_one():
    """sum_s up(W'_s x_s) + b' against BN(linear_fuse(cat(up(linear_c[s](x_s)))[::-1])) on random stage maps, geometry B (D = 256), float64:
    measured 6e-16 of the largest value; asserted at 1e-12.  The fp16 blobs are W'_s to one rounding."""
    from canonswap_amd import pack, synth
    cfg = dict(synth.PARSER_B)
    sd_np = synth._segformer(3, cfg)
    sd = R.to_tensors(sd_np)
    D = cfg["D"]
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, c, 16 >> s, 24 >> s, generator=g, dtype=torch.float64) for s, c in enumerate(cfg["widths"])]
    up = lambda t: F.interpolate(t, size=(16, 24), mode="bilinear", align_corners=False)
    maps = [up(F.conv2d(x, sd[f"decode_head.linear_c.{s}.proj.weight"][:, :, None, None], sd[f"decode_head.linear_c.{s}.proj.bias"])) for s, x in enumerate(xs)]
    y = F.conv2d(torch.cat(maps[::-1], 1), sd["decode_head.linear_fuse.weight"])
    want = F.batch_norm(y, sd["decode_head.batch_norm.running_mean"], sd["decode_head.batch_norm.running_var"], sd["decode_head.batch_norm.weight"],
                        sd["decode_head.batch_norm.bias"], False, 0.0, 1e-5)
    ws, bp = pack.parser_compose_head(pack.parser_rename(sd_np), cfg)
    got = torch.as_tensor(bp).reshape(1, -1, 1, 1) + sum(up(F.conv2d(x, torch.as_tensor(w)[:, :, None, None])) for x, w in zip(xs, ws))
    err = float((got - want).abs().max() / want.abs().max())
    print("composed vs uncomposed head:", err)
    assert err <= 1e-12
    out = {}
    pack._pack_P(out, sd_np, HEADS)
    for s in range(4):
        w = out[f"P.s{s}.head.w"].astype(np.float64)
        assert w.shape == (D, cfg["widths"][s]) and np.all(np.abs(w - ws[s]) <= 2.0 ** -11 * np.abs(ws[s]) + 2.0 ** -25)
    assert np.allclose(out["P.head.b"], bp, rtol=1e-6)


def test_build_blobs_takes_the_optional_parser(sd_np, blobs):
    from canonswap_amd import pack
    seen = {}

    def stub(out, sd):
        pass
    import unittest.mock as um
    with um.patch.multiple(pack, _pack_F=stub, _pack_W=stub, _pack_T=stub, _pack_R=stub, _pack_G=stub):
        base = {k: {} for k in ("appearance_feature_extractor", "warping_module", "transfer", "refine", "spade_generator")}
        assert not any(k.startswith("P.") for k in pack.build_blobs(base))
        seen = pack.build_blobs(dict(base, parser=sd_np, parser_config=HEADS))
    assert set(seen) == set(blobs)


def test_abi_declares_the_parser_entry_points():
    from canonswap_amd import _build
    hdr = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    for name in ENTRY_POINTS:          # (their types, arity and export: test_abi_cpu.py)
        assert re.search(r"\*/\s*(?:enum[^;]*;\s*)?int " + name + r"\(", hdr, re.S), f"{name}: no declaration with a comment above it"
    eng = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    head = eng[:eng.index('extern "C" int cs_abi_version')]
    for name in ENTRY_POINTS[:2]:
        assert name in head, f"{name}: not in the entry-point list at the top of engine.hip"
    assert any(s.endswith("parser.hip") for s in _build.SOURCES)


def test_synthetic_weights_are_not_degenerate(sd_np, cfg, pv, f64):
    """LayerNorm affines are not (1, 0); attention rows are neither uniform nor one-hot; activations stay far below the fp16 range; the logits
    spread over several labels."""
    for k, v in sd_np.items():
        if "layer_norm" in k and k.endswith(".weight"):
            assert float(np.abs(v - 1).max()) > 0.05 and float(np.abs(sd_np[k[:-6] + "bias"]).max()) > 0.02, k
    sd = R.to_tensors(sd_np)
    x = f64["stage1"].flatten(2).transpose(1, 2)                     # a plausible token tensor for stage 2's first block
    p = "segformer.encoder.patch_embeddings.2"
    t = F.conv2d(f64["stage1"], sd[p + ".proj.weight"], sd[p + ".proj.bias"], stride=2, padding=1).flatten(2).transpose(1, 2)
    t = F.layer_norm(t, (320,), sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"], 1e-5)
    b = "segformer.encoder.block.2.0"
    a = F.layer_norm(t, (320,), sd[b + ".layer_norm_1.weight"], sd[b + ".layer_norm_1.bias"], 1e-5)
    q = F.linear(a, sd[b + ".attention.self.query.weight"], sd[b + ".attention.self.query.bias"]).reshape(2, -1, 5, 64).transpose(1, 2)
    r = F.conv2d(a.transpose(1, 2).reshape(2, 320, 4, 6), sd[b + ".attention.self.sr.weight"], sd[b + ".attention.self.sr.bias"], stride=2).flatten(2).transpose(1, 2)
    r = F.layer_norm(r, (320,), sd[b + ".attention.self.layer_norm.weight"], sd[b + ".attention.self.layer_norm.bias"], 1e-5)
    k = F.linear(r, sd[b + ".attention.self.key.weight"], sd[b + ".attention.self.key.bias"]).reshape(2, -1, 5, 64).transpose(1, 2)
    pr = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    nk = pr.shape[-1]
    print("attention rows: mean max probability", float(pr.amax(-1).mean()), "of", nk, "keys")
    assert 1.5 / nk < float(pr.amax(-1).mean()) < 0.9
    for k_ in R.STAGES + ("pre", "logits"):
        assert float(f64[k_].abs().max()) < 100, k_
    assert len(f64["logits"].argmax(1).unique()) >= 6
    del x


def test_label_margins_are_usable(f64, emu):
    """The GPU label check skips pixels whose float64 margin is under 2 x the max-abs bound (4 x the emulation's max-abs distance); at most 10 %
    of the pixels may be skipped (measured: 2.3 %), and the emulation itself passes the check."""
    lg = f64["logits"]
    bound = GPU_FACTOR * R.max_abs(emu["logits"], lg) * lg.reshape(2, -1).abs().amax(1)
    sure = R.margins(lg) > 2 * bound[:, None, None]
    frac = 1 - sure.double().mean(dim=(1, 2))
    print("pixels under the margin:", frac.tolist())
    assert bool((frac <= 0.10).all())
    assert bool((emu["logits"].argmax(1) == lg.argmax(1))[sure].all())


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_the_gpu_tolerance_can_fail(sd_np, cfg, pv, f64, emu, mistake):
    """Each deliberate mistake, made in the restatement, moves every image's logits by at least 10 x the GPU tests' bound (4 x the emulation's
    distance from float64), in relative L2 and in max-abs (measured: 30 x for the skipped LN_sr, the smallest; 450 x for unreversed slices)."""
    with torch.no_grad():
        wrong = R.forward(R.to_tensors(sd_np), cfg, pv, mistake=mistake)["logits"]
    r2 = R.rel_l2(wrong, f64["logits"]) / (GPU_FACTOR * R.rel_l2(emu["logits"], f64["logits"]))
    ma = R.max_abs(wrong, f64["logits"]) / (GPU_FACTOR * R.max_abs(emu["logits"], f64["logits"]))
    print(mistake, "x the bound:", r2.tolist(), ma.tolist())
    assert bool((r2 >= 10).all()) and bool((ma >= 10).all())
