"""The landmark runner's two sides (cs_lmk_input, cs_lmk_decode; canonswap_amd/landmarks.py) without a GPU: what the C ABI of
include/canonswap_landmarks.h states beyond its types (those: test_abi_cpu.py), the geometry function of csrc/lmk_geometry.h compiled for the host and held to the
reference's own matrices (tests/golden/crop_geometry.npz) and to its guard on landmarks that must be refused, and track_video's batch planning
with a stub engine.

Bounds of the geometry (from the reference's own error, not from what the code gives): err(X) is the largest distance in pixels between X p and
the float64 evaluation's F p (tests/landmarks_ref.py), p the landmarks and the crop's corners for M_o2c, the crop's corners for M_c2o; the
function must stay within 4 x the error of the reference's golden matrices, the maximum taken over all sets and configurations - the project's
parity margin.  Non-finite landmarks are exercised here only, never on a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import landmarks_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "canonswap_landmarks.h")
CSRC = os.path.join(ROOT, "canonswap_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "crop_geometry.npz"))
CASES = [(str(k), str(c)) for k in GOLD["sets"] for c in GOLD["configs"]]


def _cfg(c):
    dsize, scale, vy, rot = GOLD[f"{c}_cfg"]
    return dict(dsize=int(dsize), scale=float(scale), vy_ratio=float(vy), flag_do_rot=bool(rot))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound():
    """(The entry points' types, arity and export, the header against its record and its recorded text: test_abi_cpu.py.)"""
    from canonswap_amd import _lib
    assert _lib.load().cs_lmk_abi_version() == 1
    assert "cs_lmk_abi_version" not in _lib.STATUS and {"cs_lmk_input", "cs_lmk_decode"} <= _lib.STATUS
    with pytest.raises(TypeError, match="cs_lmk_decode takes 9 arguments"):             # the same checks as any other entry point (_lib.call)
        _lib.call("cs_lmk_decode", None)


def test_header_cites_the_reference_and_states_why_it_stands_alone():
    header = open(HEADER).read()
    assert re.search(r"human_landmark_runner\.py:62.*?human_landmark_runner\.py:76.*?int cs_lmk_input", header, flags=re.S)
    assert re.search(r"human_landmark_runner\.py:82-83.*?int cs_lmk_decode", header, flags=re.S)
    assert "abi_v4.txt" in header and "cropper.py:186-193" in header


def test_source_is_built_under_the_contract_pragma():
    from canonswap_amd import _build
    src = os.path.join(CSRC, "landmarks.hip")
    assert src in _build.SOURCES
    text = open(src).read()
    assert "#pragma clang fp contract(off)" in text
    assert text.index("#pragma clang fp contract(off)") < text.index('#include "warp_taps.h"') < text.index('#include "lmk_geometry.h"')
    for h in ("lmk_geometry.h", "warp_taps.h"):
        assert os.path.join(CSRC, h) in _build.HEADERS
    code = re.sub(r"//[^\n]*", " ", text + open(os.path.join(CSRC, "lmk_geometry.h")).read() + open(os.path.join(CSRC, "warp_taps.h")).read())
    assert not re.search(r"\bfmaf?\s*\(|__fma", code)          # nothing asks for a fused multiply-add
    assert re.search(r"#define LMK_HD __host__ __device__", open(os.path.join(CSRC, "lmk_geometry.h")).read())


def test_python_names_import():
    from canonswap_amd import landmarks
    from canonswap_amd.can_swap_e2e import can_swapper
    assert callable(can_swapper.lmk_input) and callable(can_swapper.lmk_decode)
    assert callable(landmarks.LandmarkTracker.track_video) and callable(landmarks.Landmark106.get)
    for n, eyes in ((203, 4), (106, 4), (101, 4), (120, 4), (68, 2), (9, 2), (5, 1)):
        L = landmarks.layout_of(n)
        assert L.n_eye == eyes and max(list(L.left) + list(L.right) + list(L.lip)) < n
    assert list(landmarks.layout_of(120).left) == list(landmarks.layout_of(101).left)
    with pytest.raises(ValueError):
        landmarks.layout_of(100)


# ------------------------------------------------------------------------------------------------ the geometry function on the host
@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("needs ROCm's clang")
    from canonswap_amd import _lib, landmarks
    so = str(tmp_path_factory.mktemp("lmk_host") / "liblmk_geometry.so")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "landmarks_host", "geometry.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.lmk_geometry_host.restype = C.c_int
    lib.lmk_geometry_host.argtypes = [C.c_void_p, C.c_int, _lib.LmkLayout, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]

    def run(lmk, dsize, scale, vy_ratio, flag_do_rot):
        pts = np.ascontiguousarray(lmk, dtype=np.float32)
        M = np.full(18, np.nan, dtype=np.float32)
        why = lib.lmk_geometry_host(pts.ctypes.data, pts.shape[0], landmarks.layout_of(pts.shape[0]), dsize, scale, vy_ratio, int(flag_do_rot), M.ctypes.data)
        return why, M[:9].reshape(3, 3), M[9:].reshape(3, 3)
    return run


def test_geometry_stays_within_four_times_the_references_error(geometry):
    worst = {"dev_o2c": 0.0, "dev_c2o": 0.0, "ref_o2c": 0.0, "ref_c2o": 0.0}
    for k, c in CASES:
        lmk, cfg = GOLD[f"{k}_lmk"], _cfg(c)
        why, M_o2c, M_c2o = geometry(lmk, **cfg)
        assert why == 0, (k, c, why)
        assert np.array_equal(M_o2c[2], [0, 0, 1]) and np.array_equal(M_c2o[2], [0, 0, 1])
        d = LR.geometry_errors(M_o2c, M_c2o, lmk, **cfg)
        r = LR.geometry_errors(GOLD[f"{k}_{c}_M_o2c"], GOLD[f"{k}_{c}_M_c2o"], lmk, **cfg)
        print(f"{k} {c}: host build {d[0]:.3e} {d[1]:.3e} px, reference {r[0]:.3e} {r[1]:.3e} px")
        worst["dev_o2c"], worst["dev_c2o"] = max(worst["dev_o2c"], d[0]), max(worst["dev_c2o"], d[1])
        worst["ref_o2c"], worst["ref_c2o"] = max(worst["ref_o2c"], r[0]), max(worst["ref_c2o"], r[1])
    print(worst)
    assert worst["dev_o2c"] <= 4 * worst["ref_o2c"] and worst["dev_c2o"] <= 4 * worst["ref_c2o"], worst


def test_degenerate_axis_takes_the_images_own(geometry):
    why, M_o2c, _ = geometry(GOLD["pt5_degenerate_lmk"], 224, 1.5, -0.1, True)
    assert why == 0 and M_o2c[0, 1] == 0 and M_o2c[1, 0] == 0 and M_o2c[0, 0] == M_o2c[1, 1] > 0


@pytest.mark.parametrize("name", ["nan", "inf", "minus_inf", "huge", "all_equal", "far_apart"])
def test_guard_refuses_what_must_not_reach_a_coordinate(geometry, name):
    lmk = LR.synthetic_face(300, 200, 120, 10)
    want = None
    if name == "nan":
        lmk[77, 1] = np.nan; want = 1
    elif name == "inf":
        lmk[202, 0] = np.inf; want = 1
    elif name == "minus_inf":
        lmk[0, 0] = -np.inf; want = 1
    elif name == "huge":                      # finite, but the box overflows or the matrices leave face_box's range
        lmk[5] = [1e30, -1e30]
    elif name == "all_equal":
        lmk[:] = [123.25, 77.5]; want = 2
    elif name == "far_apart":                 # a finite box 1e12 wide: the scale is fine, M_c2o is not
        lmk = lmk * np.float32(1e10)
    for rot in (True, False):
        why, M_o2c, M_c2o = geometry(lmk, 224, 1.5, -0.1, rot)
        assert why != 0 and (want is None or why == want), (name, why)
        assert not M_o2c.any() and not M_c2o.any()                                      # zeros, and no NaN among them


def test_guard_passes_a_plain_face_and_is_deterministic(geometry):
    lmk = LR.synthetic_face(960, 540, 400, -170)
    a, b = geometry(lmk, 224, 1.5, -0.1, True), geometry(lmk, 224, 1.5, -0.1, True)
    assert a[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.abs(a[2].astype(np.float64) @ a[1].astype(np.float64) - np.eye(3)).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ track_video's batch planning
class _StubTracker:
    """LandmarkTracker.track_video over host stand-ins: batches come from the plan as plain arrays, track records what it was handed."""

    def __init__(self, freeze_at=None):
        from canonswap_amd import landmarks
        self.calls, self.freeze_at = [], freeze_at
        self.track_video = landmarks.LandmarkTracker.track_video.__get__(self)

    def _device_batches(self, frames_host, plan):
        for i, (f0, f1) in enumerate(plan):
            yield i, frames_host[f0:f1], lambda: None

    def track(self, frames, prev, status):
        import torch
        prev = torch.as_tensor(prev)
        first = int(frames[0, 0, 0, 0])
        self.calls.append((first, len(frames), prev.clone(), status))
        S = prev.shape[0]
        lmk = torch.stack([torch.full((S, 3, 2), float(first + k)) for k in range(len(frames))])      # lmk[k] names its frame
        st = torch.zeros(S, dtype=torch.int32)
        if self.freeze_at is not None and first <= self.freeze_at < first + len(frames):
            st[1] = self.freeze_at - first + 1
        return lmk, st


def test_track_video_plans_batches_and_continues_from_the_last_landmarks():
    from canonswap_amd import landmarks
    assert landmarks.plan_track_batches(7, 3) == [(0, 3), (3, 6), (6, 7)] and landmarks.plan_track_batches(4, 64) == [(0, 4)]
    frames = np.zeros((7, 2, 2, 3), np.uint8)
    frames[:, 0, 0, 0] = np.arange(7)
    seed = np.full((2, 5, 2), -1.0, np.float32)
    t = _StubTracker()
    out = t.track_video(frames, seed, batch=3)
    assert out.shape == (7, 2, 3, 2) and out.dtype == np.float32 and np.array_equal(out[:, 0, 0, 0], np.arange(7))
    assert [(c[0], c[1]) for c in t.calls] == [(0, 3), (3, 3), (6, 1)]
    assert np.array_equal(t.calls[0][2].numpy(), seed) and t.calls[0][3] is None
    assert float(t.calls[1][2][0, 0, 0]) == 2.0 and float(t.calls[2][2][0, 0, 0]) == 5.0          # the previous batch's last landmarks
    with pytest.raises(ValueError, match="trajectory 1 froze at frame 4"):
        _StubTracker(freeze_at=4).track_video(frames, seed, batch=3)
    with pytest.raises(ValueError):
        t.track_video(frames, seed, batch=0)
