"""The parser's input (cs_parser_input; tail.parser_input; the chains' parser_input) without a GPU: the yardstick of test_gpu_parser_input.py
(tests/parser_input_ref.py) against what PIL itself computes (tests/golden/parser_input.npz, and PIL live where it imports), the table of
rescale + normalize, the pass order, and the C ABI of the entry point (src/can_swap_pipeline_e2e.py:171, :180, src/can_swap_pipeline_v2i.py:73)."""
import inspect
import os
import re

import numpy as np
import pytest

import parser_input_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name,kind", PR.fixture_items())
def test_restatement_equals_pil_in_the_fixture(name, kind):
    fx = PR.fixture()
    x, pil = fx[f"{name}/{kind}/in"], fx[f"{name}/{kind}/pil"]
    B, h, w = PR.shape_of(name)
    assert x.dtype == np.uint8 and x.shape == (B, h, w, 3) and pil.dtype == np.uint8 and pil.shape == (B, 2 * h, 2 * w, 3)
    assert np.array_equal(x, PR.crops_of(name, kind, 0))                          # the fixture's inputs are the tests' inputs
    assert np.array_equal(PR.resize_x2(x), pil)
    if name in PR.CASES:
        assert np.array_equal(PR.reference(name, kind, 0)["resized_u8"], pil)


def test_fixture_holds_arrays_only_and_stays_small():
    assert os.path.getsize(PR.GOLDEN) < 200_000
    with np.load(PR.GOLDEN, allow_pickle=False) as z:                            # a pickled object would raise here
        keys = set(z.files)
        assert all(z[k].dtype in (np.uint8, np.float32) for k in keys)
    want = {"lut"} | {f"{n}/{k}/{io}" for n, k in PR.fixture_items() for io in ("in", "pil")}
    assert keys == want


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_restatement_equals_pil_live(name):
    Image = pytest.importorskip("PIL.Image")
    for kind in PR.KINDS:
        ref = PR.reference(name, kind, 0)
        for x, want in zip(ref["crops"], ref["resized_u8"]):
            h, w = x.shape[:2]
            got = np.asarray(Image.fromarray(np.ascontiguousarray(x)).resize((2 * w, 2 * h), resample=Image.BILINEAR))
            assert np.array_equal(got, want), (name, kind)


def test_saturated_inputs_stay_saturated():
    """0 / 255 inputs: (3 * 255 + 255 + 2) >> 2 is 255, never more; the restatement asserts the range in every pass."""
    for name in PR.CASES:
        for halve in (0, 1):
            u8 = PR.reference(name, "sat", halve)["resized_u8"]
            assert u8.dtype == np.uint8 and int(u8.max()) <= 255
    assert int(PR.reference("full", "sat", 0)["resized_u8"].max()) == 255 and int(PR.reference("full", "sat", 0)["resized_u8"].min()) == 0


def test_the_halving_is_the_staging_kernels_mean():
    """Step 1 is what cs_prepare_crops documents for the same cv2.resize: (a + b + c + d + 2) >> 2."""
    x = PR.crops_of("r5x7", "random", 1)
    a = x.astype(np.int64)
    want = (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2] + 2) // 4
    assert np.array_equal(PR.halve_u8(x), want.astype(np.uint8)) and PR.halve_u8(x).shape == (3, 5, 7, 3)


def test_table_equals_the_fixture_bit_for_bit():
    from canonswap_amd import tail
    lut = PR.fixture()["lut"]
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    got = tail.parser_lut()
    assert got.dtype == np.float32 and got.shape == (3, 256) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(_bits(got), _bits(lut))
    assert np.array_equal(_bits(PR.table()), _bits(lut))
    assert (tail.PARSER_MEAN, tail.PARSER_STD, tail.PARSER_RESCALE) == (PR.MEAN, PR.STD, PR.RESCALE) == ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 1 / 255)
    # the folded form u8 * scale + bias is another function: most entries differ, which is why the device looks the value up
    v = np.arange(256, dtype=np.float32)
    folded = np.stack([v * np.float32(1 / 255 / s) + np.float32(-m / s) for m, s in zip(PR.MEAN, PR.STD)])
    assert int((_bits(folded) != _bits(lut)).sum()) > 384
    # other constants change the table, by the same lines
    other = tail.parser_lut(mean=(0.5, 0.25, 0.125), std=(0.5, 0.25, 2.0), rescale=1 / 128)
    assert np.array_equal(_bits(other), _bits(PR.table((0.5, 0.25, 0.125), (0.5, 0.25, 2.0), 1 / 128))) and not np.array_equal(_bits(other), _bits(lut))
    for bad in ({"mean": (0.5, 0.5)}, {"std": (1.0, 0.0, 1.0)}):
        with pytest.raises(ValueError):
            tail.parser_lut(**bad)


def test_horizontal_pass_first_is_pinned():
    """PIL filters rows first and rounds to uint8 between the passes: the other order gives other bytes on the random 33 x 65 input."""
    fx = PR.fixture()
    x, pil = fx["r33x65/random/in"], fx["r33x65/random/pil"]
    assert np.array_equal(PR.resize_x2(x), pil)
    other = PR.resize_x2(x, vertical_first=True)
    frac = float((other != pil).mean())
    print(f"vertical-first differs from PIL in {frac:.3f} of the samples")
    assert frac > 0.05 and int(np.abs(other.astype(int) - pil.astype(int)).max()) == 1


def test_header_comment_cites_the_reference_and_the_engine_lists_the_entry_point():
    """(The entry point's types, arity and export: test_abi_cpu.py.)"""
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int cs_parser_input", header, flags=re.S)      # the comment right above the declaration
    assert comment and "can_swap_pipeline_e2e.py:171" in comment[0] and ":180" in comment[0] and "can_swap_pipeline_v2i.py:73" in comment[0]
    assert ">> 2" in comment[0] and "HORIZONTAL" in comment[0]
    engine = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    assert "cs_parser_input" in engine.split("extern \"C\" int cs_abi_version")[0]          # the entry-point list at the top


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain, FrameChain, _StagedChain
    sig = inspect.signature(tail.parser_input).parameters
    assert list(sig)[:3] == ["e", "crops_u8", "halve"] and sig["halve"].default is None
    assert sig["mean"].default == tail.PARSER_MEAN and sig["std"].default == tail.PARSER_STD and sig["rescale"].default == tail.PARSER_RESCALE
    assert sig["out"].default is None and sig["want_u8"].default is False and sig["out_u8"].default is None
    assert callable(can_swapper.parser_input)
    assert FrameChain.parser_input is _StagedChain.parser_input is AnimateChain.parser_input
    doc = _StagedChain.parser_input.__doc__
    assert "no engine scratch" in doc and "prefetch" in doc
