"""The side-by-side video frame (cs_concat_frames; tail.concat_frames; the chains' concat=True) without a GPU: the yardstick of
test_gpu_concat.py (tests/concat_ref.py: src/utils/video.py:84-109 with OpenCV's 8-bit x2 INTER_LINEAR restated in integers - PARITY UNPINNED, no
cv2 output is at hand) against the hand check, the constants and the float formula; the C ABI of the entry point; the argument checks of
tail.concat_frames that run before anything touches the device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import concat_ref as CR
import parser_input_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_comment_cites_the_reference_and_the_engine_lists_the_entry_point():
    """(The entry point's types, arity and export: test_abi_cpu.py.)"""
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int cs_concat_frames", header, flags=re.S)      # the comment right above the declaration
    assert comment and "video.py:84-109" in comment[0] and "can_swap_pipeline_e2e.py:290" in comment[0] and "can_swap_pipeline_v2i.py:328" in comment[0]
    assert ">> 16" in comment[0] and "PARITY UNPINNED" in comment[0] and "no engine scratch" in comment[0]
    engine = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    assert "cs_concat_frames" in engine.split("extern \"C\" int cs_abi_version")[0]          # the entry-point list at the top


def test_resize_x2_hand_check():
    """A source whose rows are all [0, 255] gives rows [0, 64, 191, 255]; a single pixel stays itself."""
    for h in (1, 2, 3):
        s = np.tile(np.array([0, 255], np.uint8)[None, :, None], (h, 1, 3))
        got = CR.resize_x2_cv(s)
        assert got.shape == (2 * h, 4, 3) and got.dtype == np.uint8
        assert np.array_equal(got, np.tile(np.array([0, 64, 191, 255], np.uint8)[None, :, None], (2 * h, 1, 3)))
    assert np.array_equal(CR.resize_x2_cv(np.full((1, 1, 3), 77, np.uint8)), np.full((2, 2, 3), 77, np.uint8))


def test_resize_x2_keeps_every_constant():
    for v in range(256):
        assert np.array_equal(CR.resize_x2_cv(np.full((3, 5, 3), v, np.uint8)), np.full((6, 10, 3), v, np.uint8)), v


def test_resize_x2_stays_within_one_lsb_of_the_float_formula():
    """The horizontal pass is exact; the vertical pass truncates each of its two products by less than 3/4 of the final quarter-units before the
    rounding shift: the result is floor(v + 1/2 - d / 4) with 0 <= d <= 3/2, so |result - v| <= 1/2 + 3/8 < 1 of the exact bilinear value v."""
    r = np.random.Generator(np.random.PCG64(4310))
    x = r.integers(0, 256, size=(2, 13, 9, 3), dtype=np.uint8)
    got = CR.resize_x2_cv(x).astype(np.float64)
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    want = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    err = np.abs(got - want).max()
    print(f"resize_x2_cv vs float bilinear: max |diff| {err:.4f} LSB, differs from round() in {(got != np.floor(want + 0.5)).mean():.3f} of the samples")
    assert err < 1.0


def test_concat_stacks_the_panels_left_to_right():
    r = np.random.Generator(np.random.PCG64(4311))
    a = r.integers(0, 256, size=(2, 8, 8, 3), dtype=np.uint8)
    b = r.integers(0, 256, size=(1, 4, 4, 3), dtype=np.uint8)
    f = r.uniform(-0.2, 1.2, size=(2, 3, 8, 8)).astype(np.float32)
    got = CR.concat([a, b, a, f], [0, 1, 2, 3], [0, 1, 0, 0])
    assert got.shape == (2, 8, 32, 3) and got.dtype == np.uint8
    for n in range(2):
        assert np.array_equal(got[n, :, 0:8], a[n]) and np.array_equal(got[n, :, 8:16], CR.resize_x2_cv(b[0]))
        assert np.array_equal(got[n, :, 16:24], CR.resize_x2_cv(PR.halve_u8(a[n])))
        assert np.array_equal(got[n, :, 24:32], np.clip(np.clip(f[n].transpose(1, 2, 0), 0, 1) * 255, 0, 255).astype(np.uint8))
    for P in (1, 2, 3, 4):
        arr = CR.arrangements(P)
        assert all({k[i] for k, _ in arr} == {0, 1, 2, 3} for i in range(P)) and not any(all(sh) for _, sh in arr)


def test_argument_checks_run_before_the_device():
    """Every refusal of tail.concat_frames comes before the engine is touched: None stands in for it."""
    from canonswap_amd import tail
    u8 = lambda n, s: torch.zeros((n, s, s, 3), dtype=torch.uint8)
    f32 = lambda n, s: torch.zeros((n, 3, s, s), dtype=torch.float32)
    bad = [
        dict(panels=[]), dict(panels=[u8(1, 8)] * 5),                                               # 1 to 4 panels
        dict(panels=[u8(1, 8)], kinds=[4]), dict(panels=[u8(1, 8)], kinds=[0, 0]),                  # kinds: 0..3, one per panel
        dict(panels=[u8(1, 8)], shared=[0, 0]),
        dict(panels=[u8(1, 8).to(torch.int32)]), dict(panels=[f32(1, 8).double()]), dict(panels=[torch.zeros((8, 8), dtype=torch.uint8)]),
        dict(panels=[torch.zeros((1, 8, 12, 3), dtype=torch.uint8)]), dict(panels=[torch.zeros((1, 8, 8, 4), dtype=torch.uint8)]),
        dict(panels=[torch.zeros((1, 4, 8, 8), dtype=torch.float32)]), dict(panels=[torch.zeros((0, 8, 8, 3), dtype=torch.uint8)]),
        dict(panels=[u8(1, 8)], kinds=[3]), dict(panels=[f32(1, 8)], kinds=[0]),                    # the kind and the dtype disagree
        dict(panels=[u8(1, 8), u8(1, 12)]), dict(panels=[u8(1, 8), u8(1, 8)], kinds=[0, 1]), dict(panels=[u8(1, 8), f32(1, 8)], kinds=[1, 3]),      # not one size
        dict(panels=[u8(1, 6)]), dict(panels=[u8(1, 2)]), dict(panels=[u8(1, 3)], kinds=[1]),       # S: a multiple of 4, at least 4
        dict(panels=[u8(2, 8), u8(3, 8)]), dict(panels=[u8(2, 8), u8(2, 8)], shared=[0, 1]), dict(panels=[u8(2, 8), u8(1, 8)], shared=[0, 0]),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="concat_frames"):
            tail.concat_frames(None, **kw)
    with pytest.raises(ValueError, match="16384"):
        tail.concat_frames(None, [torch.zeros((1, 3, 16388, 1), dtype=torch.float32).expand(1, 3, 16388, 16388)])      # a view: nothing that large is allocated


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain, FrameChain
    from canonswap_amd.engine import Engine
    sig = inspect.signature(tail.concat_frames).parameters
    assert list(sig) == ["e", "panels", "kinds", "shared", "out"] and all(sig[k].default is None for k in ("kinds", "shared", "out"))
    assert "no engine scratch" in tail.concat_frames.__doc__.lower() and "prefetch" in tail.concat_frames.__doc__
    assert callable(can_swapper.concat_frames)
    sw = inspect.signature(Engine.swap_frames).parameters
    assert sw["out_rec"].default is None and sw["out_swap"].default is None and list(sw)[-2:] == ["out_rec", "out_swap"]
    fc = inspect.signature(FrameChain.__call__).parameters
    assert fc["concat"].default is False and fc["concat_out"].default is None and list(fc)[1:5] == ["crops_u8", "masks", "M_c2o", "frames_ori"]
    ac = inspect.signature(AnimateChain.__call__).parameters
    assert list(ac)[1:4] == ["crops_u8", "out", "keep"] and ac["concat"].default is False and ac["I_can"].default is None and ac["concat_out"].default is None
