"""The 4:2:0 conversions (cs_yuv_to_rgb, cs_rgb_to_yuv; include/canonswap_yuv.h) without a GPU: the numpy restatement tests/yuv_ref.py, which
defines their integer arithmetic, against the standards' float64 formula; csrc/yuv_math.h compiled for the host against the restatement, bit for
bit; the keep rule; the C ABI beyond its types (those: test_abi_cpu.py); and what the Python wrappers and the video driver refuse before they touch a GPU.

Bounds.  Decode: the coefficients carry 14 fractional bits, so each of at most three products is off by at most 2^-15 of its factor, which is
below 255: |integer result before the shift - float64 formula| < 3 x 2^-15 x 255 < 0.03.  Rounding two numbers 0.03 apart gives integers at
most 1 apart: every channel within 1 LSB of the rounded (and clamped) float64 value.  Encode: 16 fractional bits and sums of four pixels
give < 3 x 2^-17 x 255 per pixel, far below 0.03: the same 1 LSB, for luma and for chroma."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import yuv_ref as YR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "canonswap_yuv.h")
CSRC = os.path.join(ROOT, "canonswap_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SET_IDS = [f"{m}-{'full' if fr else 'limited'}" for m, fr in YR.SETS]


def _round8(x):
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the restatement against float64
@pytest.mark.parametrize("matrix,full_range", YR.SETS, ids=SET_IDS)
def test_decode_of_every_triple_is_within_one_lsb_of_float64(matrix, full_range):
    worst = 0
    for y0 in range(0, 256, 64):                      # 2^24 triples, a quarter at a time
        Y, U, V = np.meshgrid(np.arange(y0, y0 + 64, dtype=np.int32), np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
        got = YR.decode_values(Y, U, V, matrix, full_range)
        want = YR.formula_decode(Y, U, V, matrix, full_range)
        for g, w in zip(got, want):
            worst = max(worst, int(np.abs(g.astype(np.int32) - _round8(w)).max()))
    print(f"{matrix} full_range={full_range}: largest |restatement - rounded float64| over 2^24 triples: {worst} LSB")
    assert worst <= 1


def _encode_inputs():
    r = np.random.Generator(np.random.PCG64(11))
    rand = r.integers(0, 256, size=(1 << 20, 2, 2, 3), dtype=np.uint8)
    greys = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 2, 2, 3))
    corners = np.array([[r_, g, b] for r_ in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    return np.concatenate([rand, greys, np.broadcast_to(corners[:, None, None, :], (8, 2, 2, 3))])


@pytest.mark.parametrize("matrix,full_range", YR.SETS, ids=SET_IDS)
def test_encode_is_within_one_lsb_of_float64(matrix, full_range):
    blocks = _encode_inputs()
    assert blocks.shape[0] == (1 << 20) + 256 + 8
    got = YR.encode_blocks(blocks, matrix, full_range)
    want = YR.formula_encode(blocks, matrix, full_range)
    worst = [int(np.abs(g.astype(np.int32) - _round8(w)).max()) for g, w in zip(got, want)]
    print(f"{matrix} full_range={full_range}: largest |restatement - rounded float64|: Y {worst[0]}, U {worst[1]}, V {worst[2]} LSB")
    assert max(worst) <= 1
    c = YR.coef(matrix, full_range)
    assert c["ur"] + c["ug"] + c["ub"] == 0 and c["vr"] + c["vg"] + c["vb"] == 0
    Y, U, V = YR.encode_blocks(blocks[1 << 20: (1 << 20) + 256], matrix, full_range)
    assert (U == 128).all() and (V == 128).all()                  # greys are neutral under every set


def test_hand_checks_bt601_limited():
    dec = lambda y, u, v: tuple(int(a) for a in YR.decode_values(y, u, v))
    assert dec(16, 128, 128) == (0, 0, 0) and dec(235, 128, 128) == (255, 255, 255)
    grey = lambda g: np.full((2, 2, 3), g, np.uint8)
    for g in range(256):
        Y, U, V = YR.encode_blocks(grey(g))
        assert int(U) == 128 and int(V) == 128, g
    Y, U, V = YR.encode_blocks(grey(255))
    assert (Y == 235).all() and (int(U), int(V)) == (128, 128)
    Y, U, V = YR.encode_blocks(grey(0))
    assert (Y == 16).all() and (int(U), int(V)) == (128, 128)
    red = np.zeros((2, 2, 3), np.uint8); red[..., 0] = 255       # BT.601 limited red: (81, 90, 240) in every table of the standard's values
    Y, U, V = YR.encode_blocks(red)
    assert abs(int(Y[0, 0]) - 81) <= 1 and abs(int(U) - 90) <= 1 and int(V) == 240


# ------------------------------------------------------------------------------------------------ the keep rule
@pytest.mark.parametrize("layout", YR.LAYOUTS)
def test_keep_returns_what_came_in_and_rewrites_one_block(layout):
    r = np.random.Generator(np.random.PCG64(21))
    yuv = r.integers(0, 256, size=(3, 18, 20), dtype=np.uint8)      # Ho 12, Wo 20; the full byte range: most triples clamp in RGB
    for matrix, fr in YR.SETS:
        rgb = YR.decode_ref(yuv, layout, matrix, fr)
        assert ((rgb == 0) | (rgb == 255)).any()                    # values outside the nominal range did clamp
        assert np.array_equal(YR.rgb_to_yuv_ref(rgb, layout, matrix, fr, keep=yuv), yuv)
        assert not np.array_equal(YR.rgb_to_yuv_ref(rgb, layout, matrix, fr), yuv)      # without keep the round trip is lossy
    rgb = YR.decode_ref(yuv, layout)
    rgb[1, 7, 9, 1] ^= 0x40                                          # one pixel of block (3, 4) of frame 1
    got = YR.rgb_to_yuv_ref(rgb, layout, keep=yuv)
    fresh = YR.rgb_to_yuv_ref(rgb, layout)
    Yg, Ug, Vg = YR.split(got, layout)
    Y0, U0, V0 = YR.split(yuv, layout)
    Yf, Uf, Vf = YR.split(fresh, layout)
    block = np.zeros((3, 6, 10), bool); block[1, 3, 4] = True
    px = np.repeat(np.repeat(block, 2, axis=1), 2, axis=2)
    assert np.array_equal(Yg, np.where(px, Yf, Y0)) and np.array_equal(Ug, np.where(block, Uf, U0)) and np.array_equal(Vg, np.where(block, Vf, V0))
    assert (got != yuv).sum() <= 6 and (got != yuv).any()           # its six bytes, no other
    assert np.array_equal(YR.merge(*YR.split(yuv, layout), layout), yuv)


def test_exhaustive_image_holds_every_triple_once():
    img = YR.exhaustive_nv12()
    assert img.shape == (1, 6144, 4096)
    Y, U, V = YR.split(img, "nv12")
    code = (Y[0].astype(np.int64) << 16) | (np.repeat(np.repeat(U[0], 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(V[0], 2, 0), 2, 1)
    assert np.array_equal(np.sort(code.ravel()), np.arange(1 << 24))


# ------------------------------------------------------------------------------------------------ yuv_math.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("needs ROCm's clang")
    so = str(tmp_path_factory.mktemp("yuv_host") / "libyuv_host.so")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "yuv_host", "yuv_host.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.yuv_host_coef.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.yuv_host_decode.argtypes = [C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    lib.yuv_host_encode.argtypes = [C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("matrix,full_range", YR.SETS, ids=SET_IDS)
def test_the_kernels_arithmetic_equals_the_restatement(host, matrix, full_range):
    m, fr = ("bt601", "bt709").index(matrix), int(full_range)
    got = np.zeros(16, np.int32)
    host.yuv_host_coef(m, fr, got.ctypes.data)
    c = YR.coef(matrix, full_range)
    names = ["y0", "cy", "crv", "cgu", "cgv", "cbu", "ry", "gy", "by", "ur", "ug", "ub", "vr", "vg", "vb"]
    assert dict(zip(names, got.tolist())) == c
    Y, U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    triples = np.ascontiguousarray(np.stack([Y, U, V], axis=-1).reshape(-1, 3))
    rgb = np.empty_like(triples)
    host.yuv_host_decode(m, fr, triples.shape[0], triples.ctypes.data, rgb.ctypes.data)
    assert np.array_equal(rgb, np.stack(YR.decode_values(triples[:, 0], triples[:, 1], triples[:, 2], matrix, full_range), axis=-1))
    blocks = np.ascontiguousarray(_encode_inputs())
    out = np.empty((blocks.shape[0], 6), np.uint8)
    host.yuv_host_encode(m, fr, blocks.shape[0], blocks.ctypes.data, out.ctypes.data)
    Yb, Ub, Vb = YR.encode_blocks(blocks, matrix, full_range)
    assert np.array_equal(out[:, :4], Yb.reshape(-1, 4)) and np.array_equal(out[:, 4], Ub) and np.array_equal(out[:, 5], Vb)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound():
    """(The entry points' types, arity and export, the header against its record and its recorded text: test_abi_cpu.py.)"""
    from canonswap_amd import _build, _lib
    assert _lib.load().cs_yuv_abi_version() == 1
    assert "cs_yuv_abi_version" not in _lib.STATUS and {"cs_yuv_to_rgb", "cs_rgb_to_yuv"} <= _lib.STATUS
    with pytest.raises(TypeError, match="cs_rgb_to_yuv takes 11 arguments"):
        _lib.call("cs_rgb_to_yuv", None)
    assert os.path.join(CSRC, "yuv.hip") in _build.SOURCES and os.path.join(CSRC, "yuv_math.h") in _build.HEADERS and HEADER in _build.HEADERS
    # the version-4 header and its binding are as they were
    assert _lib.ABI_VERSION == 4 and "cs_yuv" not in open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()


def test_every_argument_is_refused_by_the_library_before_a_device_is_touched():
    """A NULL engine comes first in the C checks; the rest of the argument checks are exercised with a real engine in tests/test_gpu_yuv.py."""
    from canonswap_amd import _lib
    lib = _lib.load()
    assert lib.cs_yuv_to_rgb(None, 1, None, 2, 2, 0, 0, 0, None, None) != 0 and b"cs_yuv_to_rgb: NULL engine" in lib.cs_last_error()
    assert lib.cs_rgb_to_yuv(None, 1, None, 2, 2, 0, 0, 0, 0, None, None) != 0 and b"cs_rgb_to_yuv: NULL engine" in lib.cs_last_error()


# ------------------------------------------------------------------------------------------------ Python: names and refusals that need no GPU
def test_python_names_import():
    import inspect
    from canonswap_amd import tail, video
    from canonswap_amd.can_swap_e2e import can_swapper
    assert callable(can_swapper.yuv_to_rgb) and callable(can_swapper.rgb_to_yuv)
    assert list(inspect.signature(tail.yuv_to_rgb).parameters) == ["e", "yuv", "layout", "matrix", "full_range", "out"]
    assert list(inspect.signature(tail.rgb_to_yuv).parameters) == ["e", "rgb", "layout", "matrix", "full_range", "keep", "out"]
    for f in (video.VideoSwapper.run, video.VideoSwapper.swap_video):
        assert f is video.VideoSwapper.swap_video or inspect.signature(f).parameters["pixel_format"].default == "rgb24"
    assert video.PIXEL_FORMATS == ("rgb24", "nv12", "i420")


class _NoEngine:
    """Stands where the engine would: the wrappers must refuse before they ask it for anything."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine's {name} was touched before the arguments were checked")


def test_wrappers_refuse_by_argument_name():
    import torch
    from canonswap_amd import tail
    e = _NoEngine()
    yuv, rgb = np.zeros((1, 6, 8), np.uint8), np.zeros((1, 4, 8, 3), np.uint8)
    cases = [
        ("layout", lambda: tail.yuv_to_rgb(e, yuv, layout="yuyv")),
        ("matrix", lambda: tail.yuv_to_rgb(e, yuv, matrix="bt2020")),
        ("full_range", lambda: tail.yuv_to_rgb(e, yuv, full_range="tv")),
        ("yuv", lambda: tail.yuv_to_rgb(e, yuv.astype(np.int16))),
        ("yuv", lambda: tail.yuv_to_rgb(e, yuv[0])),                                           # rank
        ("yuv", lambda: tail.yuv_to_rgb(e, np.zeros((1, 7, 8), np.uint8))),                    # 7 rows: Ho = 14 / 3
        ("yuv", lambda: tail.yuv_to_rgb(e, np.zeros((1, 6, 7), np.uint8))),                    # odd Wo
        ("layout", lambda: tail.rgb_to_yuv(e, rgb, layout="rgb24")),
        ("rgb", lambda: tail.rgb_to_yuv(e, np.zeros((1, 5, 8, 3), np.uint8))),                 # odd Ho
        ("rgb", lambda: tail.rgb_to_yuv(e, np.zeros((1, 4, 7, 3), np.uint8))),                 # odd Wo
        ("rgb", lambda: tail.rgb_to_yuv(e, rgb[..., :2])),
        ("rgb", lambda: tail.rgb_to_yuv(e, rgb.astype(np.float32))),
        ("keep / out", lambda: tail.rgb_to_yuv(e, rgb, keep=torch.zeros(1), out=torch.zeros(1))),
    ]
    for who, call in cases:
        with pytest.raises(ValueError, match=who):
            call()


class _StubChain:
    class e:
        max_batch, latency_mode, device, has_parser, _ids = 4, False, "cpu", False, [0]
    _side = None


@pytest.fixture
def driver(monkeypatch):
    """A VideoSwapper over stand-ins: its checks run before anything is enqueued, so they need neither an engine nor a stream."""
    from canonswap_amd import video
    monkeypatch.setattr(video, "HostFrames", lambda device, batch: None)
    monkeypatch.setattr(video, "FrameSink", lambda device, batch: None)
    return video.VideoSwapper(None, batch=2, chain=_StubChain())


def test_driver_refusals_name_the_argument(driver):
    lmk, masks = np.zeros((3, 5, 2), np.float32), np.zeros((3, 512, 512), np.uint8)
    ok = dict(slots=[0, 0, 0], masks=masks)
    good = np.zeros((3, 18, 16), np.uint8)                                                      # Ho 12, Wo 16
    cases = [
        ("frames", lambda fmt: driver.run(np.zeros((3, 17, 16), np.uint8), lmk, pixel_format=fmt, **ok)),       # 17 rows: Ho would be 11 1/3
        ("frames", lambda fmt: driver.run(np.zeros((3, 18, 15), np.uint8), lmk, pixel_format=fmt, **ok)),       # odd Wo
        ("frames", lambda fmt: driver.run(np.zeros((3, 12, 16, 3), np.uint8), lmk, pixel_format=fmt, **ok)),    # RGB frames: the wrong rank
        ("frames", lambda fmt: driver.run([good[0], good[1][:12]], lmk[:2], pixel_format=fmt, slots=[0, 0], masks=masks[:2])),
        ("frames", lambda fmt: driver.run(good.astype(np.uint16), lmk, pixel_format=fmt, **ok)),
        ("matrix", lambda fmt: driver.run(good, lmk, pixel_format=fmt, matrix="smpte240m", **ok)),
        ("full_range", lambda fmt: driver.run(good, lmk, pixel_format=fmt, full_range="pc", **ok)),
        ("out", lambda fmt: driver.swap_video(good, lmk, pixel_format=fmt, out=np.empty((3, 12, 16, 3), np.uint8), **ok)),
        ("lmk", lambda fmt: driver.run(good, lmk[:2], pixel_format=fmt, **ok)),
    ]
    for fmt in ("nv12", "i420"):
        for who, call in cases:
            with pytest.raises(ValueError, match=who):
                call(fmt)
    for bad in ("yuv420p", "rgb", None):
        with pytest.raises(ValueError, match="pixel_format"):
            driver.run(good, lmk, pixel_format=bad, **ok)
        with pytest.raises(ValueError, match="pixel_format"):
            driver.swap_video(good, lmk, pixel_format=bad, **ok)
    with pytest.raises(ValueError, match="frames"):                                             # and rgb24 does not take 4:2:0 frames
        driver.run(good, lmk, **ok)
