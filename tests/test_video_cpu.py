"""video.plan_batches, checked without a GPU: which frames and which faces go into which step of the video driver (canonswap_amd/video.py).
A pure function of the frame count and the frame index; the module imports without torch."""
import subprocess
import sys

import numpy as np
import pytest

from canonswap_amd.video import plan_batches


def _check_plan(plan, n_frames, frame_index, batch, max_faces):
    """Coverage, order and both caps: the spans [f0, f1) tile [0, n_frames) in order, the spans [b0, b1) tile the faces in order, [b0, b1)
    holds exactly the faces of the frames [f0, f1), no step holds more than `batch` frames or `max_faces` faces, and none is empty."""
    fi = np.arange(n_frames) if frame_index is None else np.asarray(frame_index, np.int64)
    f, b = 0, 0
    for f0, f1, b0, b1 in plan:
        assert (f0, b0) == (f, b) and f1 > f0 and b1 >= b0
        assert f1 - f0 <= batch and b1 - b0 <= max_faces
        assert np.array_equal(np.nonzero((fi >= f0) & (fi < f1))[0], np.arange(b0, b1))      # a frame's faces stay together, in this step
        f, b = f1, b1
    assert (f, b) == (n_frames, len(fi))


def test_one_face_per_frame():
    assert plan_batches(7, batch=3) == [(0, 3, 0, 3), (3, 6, 3, 6), (6, 7, 6, 7)]
    assert plan_batches(0) == [] and plan_batches(0, [], 4, 4) == []
    assert plan_batches(1) == [(0, 1, 0, 1)]
    assert plan_batches(5, batch=64) == [(0, 5, 0, 5)]                          # batch larger than n_frames
    assert plan_batches(64) == [(0, 64, 0, 64)] and plan_batches(65) == [(0, 64, 0, 64), (64, 65, 64, 65)]      # the defaults: 64 frames, 84 faces
    assert plan_batches(10, batch=8, max_faces=4) == [(0, 4, 0, 4), (4, 8, 4, 8), (8, 10, 8, 10)]               # the face cap binds: min(batch, max_faces)
    for n, batch, mf in ((7, 3, 84), (10, 8, 4), (1, 1, 1), (9, 2, 5)):
        _check_plan(plan_batches(n, None, batch, mf), n, None, batch, mf)
    assert isinstance(plan_batches(3)[0], tuple) and all(type(v) is int for v in plan_batches(3)[0])


def test_frame_index_takes_whole_frames_under_both_caps():
    # seven frames, six faces: frame 0 none, 1 one, 2 one, 3 and 4 none, 5 two, 6 two
    fi = [1, 2, 5, 5, 6, 6]
    plan = plan_batches(7, fi, batch=3, max_faces=4)
    assert plan == [(0, 3, 0, 2), (3, 6, 2, 4), (6, 7, 4, 6)]
    _check_plan(plan, 7, fi, 3, 4)
    # the face cap closes a step before the frame cap does: frame 2's two faces do not fit behind three, and open the next step
    fi = [0, 0, 1, 2, 2, 3]
    plan = plan_batches(4, fi, batch=4, max_faces=4)
    assert plan == [(0, 2, 0, 3), (2, 4, 3, 6)]
    _check_plan(plan, 4, fi, 4, 4)
    # the same index under the frame cap alone
    assert plan_batches(4, fi, batch=3, max_faces=84) == [(0, 3, 0, 5), (3, 4, 5, 6)]
    # a frame with exactly max_faces faces is a step of its own between its neighbours
    fi = [0, 1, 1, 1, 2]
    assert plan_batches(3, fi, batch=8, max_faces=3) == [(0, 1, 0, 1), (1, 2, 1, 4), (2, 3, 4, 5)]


def test_frames_without_faces_at_the_start_in_the_middle_and_at_the_end():
    fi = [2, 2, 5]                                                              # frames 0, 1 (start), 3, 4 (middle), 6, 7, 8 (end) hold nobody
    for batch, mf in ((2, 2), (3, 2), (4, 3), (9, 84), (1, 2)):
        plan = plan_batches(9, fi, batch, mf)
        _check_plan(plan, 9, fi, batch, mf)
    assert plan_batches(9, fi, 2, 2) == [(0, 2, 0, 0), (2, 4, 0, 2), (4, 6, 2, 3), (6, 8, 3, 3), (8, 9, 3, 3)]      # steps without any face
    assert plan_batches(9, fi, 9, 84) == [(0, 9, 0, 3)]
    assert plan_batches(3, [], 2, 4) == [(0, 2, 0, 0), (2, 3, 0, 0)]            # a video in which nobody was found
    assert plan_batches(1, [0, 0], 5, 2) == [(0, 1, 0, 2)]
    assert plan_batches(4, np.array([], np.int32), 64) == [(0, 4, 0, 0)]


def test_random_indices_keep_every_property():
    r = np.random.Generator(np.random.PCG64(7))
    for _ in range(200):
        n = int(r.integers(1, 30))
        mf = int(r.integers(1, 7))
        per = r.integers(0, mf + 1, size=n)
        fi = np.repeat(np.arange(n), per)
        batch = int(r.integers(1, 9))
        _check_plan(plan_batches(n, fi, batch, mf), n, fi, batch, mf)
        _check_plan(plan_batches(n, fi.tolist(), batch, mf), n, fi, batch, mf)


def test_refusals_name_the_argument():
    with pytest.raises(ValueError, match=r"frame 3 .*5 faces.*max_faces = 4"):
        plan_batches(6, [0, 3, 3, 3, 3, 3, 5], batch=8, max_faces=4)           # max_faces + 1 faces in frame 3
    with pytest.raises(ValueError, match="batch"):
        plan_batches(6, None, batch=0)
    with pytest.raises(ValueError, match="batch"):
        plan_batches(6, [0, 1], batch=-2)
    with pytest.raises(ValueError, match="frame_index.*decrease"):
        plan_batches(6, [0, 2, 1, 3])
    for bad in ([0, 6], [-1, 0]):
        with pytest.raises(ValueError, match="frame_index.*lie in"):
            plan_batches(6, bad)
    with pytest.raises(ValueError, match="frame_index.*lie in"):
        plan_batches(0, [0])
    with pytest.raises(ValueError, match="frame_index.*integers"):
        plan_batches(6, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="frame_index"):
        plan_batches(6, [[0, 1], [2, 3]])


def test_the_same_index_rules_as_tail_frame_index_of():
    """plan_batches validates a frame index as tail.frame_index_of does: what one refuses, the other refuses."""
    from canonswap_amd import tail
    for fi, ok in (([0, 0, 2], True), ([], True), ([2, 1], False), ([0, 4], False), ([-1], False), (np.array([0.5]), False)):
        for f in (lambda: plan_batches(4, fi, 2, 4), lambda: tail.frame_index_of(fi, len(fi), 4)):
            if ok:
                f()
            else:
                with pytest.raises(ValueError, match="frame_index"):
                    f()


def test_planning_needs_no_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from canonswap_amd.video import plan_batches\n"
            "assert plan_batches(5, [0, 0, 4], 2, 2) == [(0, 2, 0, 2), (2, 4, 2, 2), (4, 5, 2, 3)]\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=__import__("os").path.dirname(__import__("os").path.dirname(__file__)))


def test_the_driver_is_reachable_from_the_swapper():
    import inspect
    from canonswap_amd import video
    from canonswap_amd.can_swap_e2e import can_swapper
    assert "driver" in inspect.signature(can_swapper.swap_video).parameters
    run = inspect.signature(video.VideoSwapper.run).parameters
    for name in ("frames", "lmk", "source_id", "slots", "frame_index", "masks", "parse", "logits_fn"):
        assert name in run
    for rule in "abcdef":
        assert f"\n    {rule}. " in video.__doc__                               # each ordering rule stated once, in the module docstring
