"""The identity network behind getid, without a GPU: the restatement (tests/identity_ref.py) against the reference class's recorded outputs
(tests/golden/identity_b3.npz, tools/make_golden_identity.py), the packer's folds, the C ABI's declarations, and that the GPU tests'
tolerance can fail."""
import os
import re

import numpy as np
import pytest
import torch

import identity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cs_identity", "cs_identity_u8", "cs_op_identity_read", "cs_op_id_conv", "cs_op_id_maxpool", "cs_op_id_se_tail", "cs_op_id_embed")
GPU_FACTOR = 4.0          # tests/test_gpu_getid.py: the engine may be 4 x the fp16-operand emulation's error away from float64


@pytest.fixture(scope="module")
def gold(golden):
    return golden("identity_b3.npz")


@pytest.fixture(scope="module")
def sd_np(gold):
    from canonswap_amd import synth
    return synth._arcface(int(gold["weight_seed"]))


@pytest.fixture(scope="module")
def imgs(gold):
    from canonswap_amd import synth
    img = synth.make_identity_inputs(3, seed=int(gold["input_seed"]), size=112)
    img[1] = 0.5
    return torch.from_numpy(img)


@pytest.fixture(scope="module")
def f64(sd_np, imgs):
    with torch.no_grad():
        return R.forward(R.to_tensors(sd_np), imgs.double())


@pytest.fixture(scope="module")
def emu_err(sd_np, imgs, f64):
    """Per-row relative L2 error of the fp16-operand emulation's raw embedding: a measurement of the restatement alone."""
    with torch.no_grad():
        return R.rel_l2(R.forward(R.to_tensors(sd_np), imgs.double(), emulate=True)["raw"], f64["raw"])


@pytest.fixture(scope="module")
def blobs(sd_np):
    from canonswap_amd import pack
    out = {}
    pack._pack_A(out, sd_np)
    return out


def test_restatement_matches_the_reference_class(gold, sd_np, imgs, f64):
    """float32 restatement: 1e-5 relative against the reference class's float32 embeddings.  float64 restatement: the same bound - what is
    left between it and the golden is the float32 reference's own rounding, which a float32 evaluation of the same network bounds."""
    ref = torch.from_numpy(gold["raw"])
    with torch.no_grad():
        e32 = R.rel_l2(R.forward(R.to_tensors(sd_np, torch.float32), imgs)["raw"], ref)
    e64 = R.rel_l2(f64["raw"], ref)
    print("float32 restatement vs golden", e32.tolist(), "float64", e64.tolist())
    assert float(e32.max()) <= 1e-5 and float(e64.max()) <= 1e-5
    names = [str(s) for s in gold["stage_names"]]
    assert tuple(names) == R.STAGES
    for j, k in enumerate(names):
        for b in range(3):
            assert abs(float(f64[k][b].abs().mean()) / gold["stage_mean_abs"][b, j] - 1) <= 1e-5, (k, b)
            assert abs(float(f64[k][b].abs().max()) / gold["stage_max_abs"][b, j] - 1) <= 1e-5, (k, b)


def test_state_dict_keys_are_the_reference_class_s(gold, sd_np):
    assert len(sd_np) == 589
    assert list(sd_np.keys()) == [str(k) for k in gold["keys"]]
    assert [",".join(map(str, v.shape)) for v in sd_np.values()] == [str(s) for s in gold["shapes"]]
    from canonswap_amd import synth
    assert "arcface" not in synth.MODULES and set(synth.make_state_dicts(0, modules=("arcface",))) == {"arcface"}
    slopes = [float(v[0]) for k, v in sd_np.items() if k.endswith("prelu.weight") or k.endswith("se.fc.1.weight")]
    assert len(slopes) == 49 and all(0.1 <= s <= 0.4 for s in slopes) and len(set(slopes)) == 49


def test_activations_stay_far_below_the_fp16_range(f64):
    for k in R.STAGES + ("raw",):
        assert float(f64[k].abs().max()) < 100, k


def test_inputs_have_the_normalised_range():
    from canonswap_amd import synth
    x = synth.make_identity_inputs(2, seed=11, size=64)
    assert x.shape == (2, 3, 64, 64) and x.dtype == np.float32
    assert -2.2 <= x.min() < -1.5 and 2.0 < x.max() <= 2.7
    assert np.array_equal(x, synth.make_identity_inputs(2, seed=11, size=64))


def test_packer_folds_unpack_to_the_scaled_weights(sd_np, blobs):
    """Every folded conv un-packs to W * scale within one fp16 rounding (2^-11 relative, 2^-25 absolute below the normal range); the bias is the
    BatchNorm's shift; the bn0 pairs, the net's bn2 pair and the fc re-ordering are what the docstring of pack._pack_A says."""
    from canonswap_amd import pack

    def check(blob, w, bn, cin, k):
        s, t = pack.bn_affine(sd_np, bn)
        want = sd_np[w].astype(np.float64) * s[:, None, None, None]
        got = pack.unpack_id_conv(blobs[blob + ".w"], cin, k, k).astype(np.float64)
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 2.0 ** -11 * np.abs(want) + 2.0 ** -25), blob
        assert np.array_equal(blobs[blob + ".b"], t.astype(np.float32)), blob
        assert not blobs[blob + ".w"][:, :, cin:].any(), blob

    check("A.stem", "conv1.weight", "bn1", 3, 3)
    assert blobs["A.stem.w"].shape == (9, 64, 32)
    nds = 0
    for n, p, cin, cout, stride in pack.id_blocks():
        check(n + ".c1", p + ".conv1.weight", p + ".bn1", cin, 3)
        check(n + ".c2", p + ".conv2.weight", p + ".bn2", cin, 3)
        assert blobs[n + ".c2.w"].shape == (9, cout, cin)
        if stride == 2:
            check(n + ".ds", p + ".downsample.0.weight", p + ".downsample.1", cin, 1)
            nds += 1
        else:
            assert n + ".ds.w" not in blobs
        s, t = pack.bn_affine(sd_np, p + ".bn0")
        assert np.array_equal(blobs[n + ".pre.s"], s.astype(np.float32)) and np.array_equal(blobs[n + ".pre.t"], t.astype(np.float32))
    assert nds == 3 and len(pack.id_blocks()) == 24
    s3, t3 = pack.bn_affine(sd_np, "bn3")
    want = (sd_np["fc.weight"].astype(np.float64) * s3[:, None]).reshape(512, 512, 7, 7)            # [o][c][h][w]
    got = blobs["A.fc.w"].astype(np.float64).reshape(7, 7, 512, 512).transpose(2, 3, 0, 1)           # [h][w][o][c] -> [o][c][h][w]
    assert np.all(np.abs(got - want) <= 2.0 ** -11 * np.abs(want) + 2.0 ** -25)
    assert np.allclose(blobs["A.fc.b"], sd_np["fc.bias"].astype(np.float64) * s3 + t3, rtol=1e-6, atol=1e-7)
    assert blobs["A.slopes"].shape == (49,) and blobs["A.slopes"][0] == sd_np["prelu.weight"][0]
    assert blobs["A.slopes"][1] == sd_np["layer1.0.prelu.weight"][0] and blobs["A.slopes"][2] == sd_np["layer1.0.se.fc.1.weight"][0]
    assert all(k.startswith("A.") for k in blobs)


def test_build_blobs_takes_the_optional_arcface(monkeypatch, sd_np, blobs):
    """build_blobs handles "arcface" as it handles "motion_extractor": there when given, absent otherwise."""
    from canonswap_amd import pack
    for f in ("_pack_F", "_pack_W", "_pack_T", "_pack_R", "_pack_G"):
        monkeypatch.setattr(pack, f, lambda out, sd: None)
    five = {k: {} for k in ("appearance_feature_extractor", "warping_module", "spade_generator", "transfer", "refine")}
    assert pack.build_blobs(five) == {}
    got = pack.build_blobs(dict(five, arcface=sd_np))
    assert set(got) == set(blobs) and all(np.array_equal(got[k], blobs[k]) for k in blobs)


def test_packed_constants_reproduce_the_restatement(blobs, imgs, f64, emu_err):
    """The engine's constants in the engine's data flow, evaluated on the CPU in float64 with fp16 activations where the engine stores them: the
    emulation's roundings plus the BatchNorm scale rounded with the weight - two error sets of the emulation's size, so twice its error bounds it."""
    with torch.no_grad():
        err = R.rel_l2(R.forward_blobs(blobs, imgs), f64["raw"])
    print("packed constants vs float64", err.tolist(), "emulation", emu_err.tolist())
    assert bool((err <= 2 * emu_err).all())


def test_abi_declares_the_identity_entry_points():
    from canonswap_amd import _build
    hdr = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    for name in ENTRY_POINTS:          # (their types, arity and export: test_abi_cpu.py)
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:enum[^;]*;\s*)?int " + name + r"\(", hdr, re.S)
        assert m, f"{name}: no declaration with a comment above it"
        assert re.search(r"(arcface_models|can_swap_e2e|can_swap_pipeline_e2e)\.py:\d+", m.group(1)), f"{name}: the comment names no reference file:line"
    eng = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    head = eng[:eng.index('extern "C" int cs_abi_version')]
    for name in ENTRY_POINTS[:3]:
        assert name in head, f"{name}: not in the entry-point list at the top of engine.hip"
    assert any(s.endswith("identity.hip") for s in _build.SOURCES)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_the_gpu_tolerance_can_fail(sd_np, imgs, f64, emu_err, mistake):
    """Each of these mistakes, made in the restatement, moves every raw embedding by more than 10 x the GPU tests' tolerance (4 x the emulation's
    error).  One SE gate forced to 1 is one block's (block 5); the others are made where an engine would make them, in every block."""
    with torch.no_grad():
        bad = R.forward(R.to_tensors(sd_np), imgs.double(), mistake=mistake, mistake_block=5 if mistake == "se_one" else None)
    err = R.rel_l2(bad["raw"], f64["raw"])
    print(mistake, err.tolist(), "tolerance", (GPU_FACTOR * emu_err).tolist())
    assert bool((err > 10 * GPU_FACTOR * emu_err).all())
