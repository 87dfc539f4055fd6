"""Several faces per frame, checked without a GPU: the C ABI of cs_crop_faces / cs_paste_back_faces (declared, bound, exported; the version
stays 4), the reference composition tests/multi_face_ref.py itself (it must see order, or the GPU's order test shows nothing), the scenes the
GPU tests run, and tail's validation of the frame index."""
import os
import re

import numpy as np
import pytest

import multi_face_ref as MF
from oracle import cv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_cites_the_reference_and_both_entry_points_take_a_frame_index():
    """(The entry points' types, arity and export: test_abi_cpu.py.)"""
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(cs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))}
    assert re.search(r"face_detect_crop_multi\.py:63-99.*?crop\.py:515-529.*?int cs_crop_faces", header, flags=re.S)      # the comment cites the reference
    for name in ("cs_crop_faces", "cs_paste_back_faces"):
        assert "frame_index" in decl[name]


def test_python_names_import():
    import inspect
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain, FrameChain
    for f in (tail.crop_faces, tail.crop_faces_M, tail.paste_back_faces, can_swapper.crop_faces, can_swapper.paste_back_faces):
        assert callable(f) and "frame_index" in inspect.signature(f).parameters
    assert inspect.signature(FrameChain.__call__).parameters["frame_index"].default is None
    assert inspect.signature(FrameChain.crop).parameters["frame_index"].default is None
    assert "frame_index" not in inspect.signature(AnimateChain.__call__).parameters


# ---- the reference composition
def test_one_face_per_frame_is_single_paste_back():
    crops, masks, M, _, ori = MF.scene()
    B = 4
    got = MF.paste_faces(crops[:B], masks[:B], M[:B], np.arange(B), ori)
    for b in range(B):
        want = R.paste_back(crops[b], M[b], ori[b], R.prepare_paste_back(masks[b], M[b], (ori.shape[2], ori.shape[1]))[..., None])
        assert np.array_equal(got[b], want)
    assert not np.array_equal(got[0], ori[0])


def test_faceless_frames_stay_and_the_scene_is_what_it_says():
    crops, masks, M, fi, ori = MF.scene()
    F, Ho, Wo = ori.shape[:3]
    assert list(fi) == [0, 0, 2, 2, 2, 3] and np.bincount(fi, minlength=F).tolist() == list(MF.FACES)
    assert masks.min() == 0 and masks.max() == 1 and 0 < np.median(masks) < 1 and masks.dtype == np.float32
    assert crops.min() == 0 and crops.max() == 255 and ori.min() == 0 and ori.max() == 255
    got = MF.paste_faces(crops, masks, M, fi, ori)
    assert np.array_equal(got[1], ori[1])                                               # the frame without a face
    for f in (0, 2, 3):
        assert not np.array_equal(got[f], ori[f])
    fp = [MF.footprint(M[b], 16, 16, Ho, Wo) for b in range(len(M))]
    assert (fp[0] & fp[1]).sum() > 100                                                  # frame 0: the two faces overlap
    assert abs(np.arctan2(M[2][1, 0], M[2][0, 0]) - np.pi / 4) < 0.1                    # frame 2: turned by about 45 degrees
    assert fp[2].any() and not fp[2].all() and fp[2][:, -1].any() and fp[2][-1, :].any()      # ... and cut by the right and the lower border
    assert not fp[3].any()                                                              # wholly outside its frame
    assert fp[4].any() and not fp[4][0].any() and not fp[4][:, 0].any()                 # inside
    assert fp[5].all()                                                                  # covers its whole frame
    without = MF.paste_faces(np.delete(crops, 3, 0), np.delete(masks, 3, 0), np.delete(M, 3, 0), np.delete(fi, 3), ori)
    assert np.array_equal(without, got)                                                 # the face outside pastes nothing


def test_order_of_two_overlapping_faces_matters():
    """Guards the GPU's order test: on frame 0's two faces the composition differs when they swap places - in the overlap, and only there."""
    crops, masks, M, fi, ori = MF.scene()
    ab = MF.paste_faces(crops[:2], masks[:2], M[:2], fi[:2], ori)
    ba = MF.paste_faces(crops[1::-1], masks[1::-1], M[1::-1], fi[:2], ori)
    differs = (ab[0] != ba[0]).any(-1)
    both = MF.footprint(M[0], 16, 16, 24, 36) & MF.footprint(M[1], 16, 16, 24, 36)
    assert differs.sum() > 50 and not (differs & ~both).any()
    assert np.array_equal(ab[1:], ba[1:])


def test_chunk_scene_crosses_every_launch_size():
    crops, masks, M, fi, ori = MF.chunk_scene()
    counts = np.bincount(fi, minlength=3).tolist()
    assert counts == [40, 0, 30] and len(crops) == 70 > 64


def test_reference_crop_reads_the_indexed_frame():
    r = np.random.Generator(np.random.PCG64(1))
    frames = r.integers(0, 256, size=(2, 20, 28, 3), dtype=np.uint8)
    M = np.stack([np.linalg.inv(MF.similarity(1.5, 0.2 * b, 3.0 + b, 2.0)) for b in range(3)])
    got = MF.crop_faces(frames, M, [0, 1, 1], 8)
    assert got.shape == (3, 8, 8, 3)
    assert np.array_equal(got[2], R.warp_affine_u8(frames[1], M[2], (8, 8))) and not np.array_equal(got[2], R.warp_affine_u8(frames[0], M[2], (8, 8)))


# ---- tail's validation of the index: no engine is needed to be refused
def test_frame_index_of_accepts_and_normalises():
    from canonswap_amd import tail
    for fi in ([0, 0, 2, 2], np.array([0, 0, 2, 2], np.int64), np.array([0, 0, 2, 2], np.uint8), (0, 0, 2, 2)):
        a = tail.frame_index_of(fi, 4, 3)
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.tolist() == [0, 0, 2, 2]
    assert tail.frame_index_of([], 0, 2).shape == (0,)
    assert tail.frame_index_of(np.arange(0, 8, 2)[::1], 4, 7).tolist() == [0, 2, 4, 6]


@pytest.mark.parametrize("fi,B,F,word", [
    ([0, 1, 0], 3, 2, "decrease"), ([1, 0], 2, 2, "decrease"),
    ([0, 2], 2, 2, r"\[0, 2\)"), ([-1, 0], 2, 2, r"\[0, 2\)"), ([0, 0, 5], 3, 5, r"\[0, 5\)"),
    ([0, 0], 3, 2, "3 frame numbers"), ([0, 0, 1, 1], 3, 2, "3 frame numbers"), ([[0, 1]], 2, 2, "frame numbers"), (0, 1, 1, "frame numbers"),
    ([0.0, 1.0], 2, 2, "integers"), ([0], 0, 1, "0 frame numbers"),
], ids=["decreasing", "decreasing-2", "too-large", "negative", "equal-F", "too-short", "too-long", "two-dim", "scalar", "floats", "index-without-faces"])
def test_frame_index_of_refuses(fi, B, F, word):
    from canonswap_amd import tail
    with pytest.raises(ValueError, match="frame_index.*" + word):
        tail.frame_index_of(fi, B, F)


def test_tail_refuses_a_bad_index_before_it_needs_an_engine():
    """paste_back_faces / crop_faces_M check shapes and the index on the host first: with host inputs and no engine (None) the refusal of the
    index is what comes out, not an attribute error - nothing of the engine has been touched."""
    from canonswap_amd import tail

    class NoEngine:
        device = "cpu"

    crops, masks, M, fi, ori = MF.scene()
    for bad in ([0, 0, 2, 1, 2, 3], [0, 0, 2, 2, 2, 4], [0, 0, 2, 2, 2]):
        with pytest.raises(ValueError, match="frame_index"):
            tail.paste_back_faces(NoEngine(), crops, masks, M, bad, ori)
        with pytest.raises(ValueError, match="frame_index"):
            tail.crop_faces_M(NoEngine(), ori, M, bad, 8)
