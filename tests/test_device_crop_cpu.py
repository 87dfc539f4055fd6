"""include/canonswap_device_crop.h without a GPU: the header, its record of canonswap_amd/_lib.py HEADERS_BESIDE and the recorded
tests/golden/abi_device_crop_v1.txt rendered to the same text (tests/abi_text.py, as tests/test_abi_cpu.py does for the three records of HEADERS);
how the record is bound (load(), beside bind()); the numpy restatement of lmk_crop; and what tail.crop_lmk / tail.paste_back_faces_dev refuse
before the library is touched.

`python tests/test_device_crop_cpu.py` prints the header's rendering, first line included: that is the recorded file."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import device_crop_ref as DR
from abi_text import mismatches, render_binding, render_header, stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = "abi_device_crop_v1.txt"
CALLS = {"cs_crop_lmk", "cs_paste_back_faces_dev"}


def record():
    """(the record, its header's text, the first line of its recorded file)."""
    from canonswap_amd import _lib
    (h,) = _lib.HEADERS_BESIDE
    rule = (f"# C ABI version {h.version} as include/{h.file} declares it (python tests/test_device_crop_cpu.py). A changed line "
            f"is a changed meaning of version {h.version}: bump {h.version_define} and record a new file. A new entry point adds a line.")
    return h, open(os.path.join(ROOT, "include", h.file)).read(), rule


def recorded():
    return open(os.path.join(ROOT, "tests", "golden", RECORDED)).read().split("\n")


# ------------------------------------------------------------------------------------------------ the header, the record, the recorded text
def test_the_record():
    from canonswap_amd import _lib
    h, _, _ = record()
    assert (h.file, h.version, h.version_define, h.version_call, h.ab_may_lack) == (
        "canonswap_device_crop.h", 1, "CS_DCROP_ABI_VERSION", "cs_dcrop_abi_version", True)
    assert h.table is _lib.ABI_DEVICE_CROP and set(h.table) == CALLS | {"cs_dcrop_abi_version"} and h.structs == {} and h.constants == {}
    assert type(h) is type(_lib.HEADERS[0])


def test_header_equals_binding_and_the_recorded_abi():
    h, header, rule = record()
    assert mismatches(render_header(header, h), render_binding(h), "canonswap_amd/_lib.py") == []
    assert render_header(header, h) == render_binding(h)
    lines = recorded()
    assert lines[0] == rule and lines[-1] == ""
    assert mismatches(render_header(header, h), lines[1:-1], "tests/golden/" + RECORDED) == []
    assert render_header(header, h) == lines[1:-1]
    assert "typedef" not in header and '#include "canonswap_landmarks.h"' in header          # cs_lmk_layout by pointer: no struct of its own


def test_the_check_can_fail():
    h, header, _ = record()
    bad = render_header(header.replace("const float* lmk, int N", "const float* lmk, long N"), h)
    for other, what in ((render_binding(h), "canonswap_amd/_lib.py"), (recorded()[1:-1], "tests/golden/" + RECORDED)):
        found = mismatches(bad, other, what)
        assert found and any(m.startswith("cs_crop_lmk:") for m in found)


def test_the_stream_parameters_the_status_and_no_scratch():
    from canonswap_amd import _lib
    h, header, _ = record()
    assert stream_entries(header) == CALLS == _lib.TAKES_STREAM & set(h.table)
    assert all(h.table[name][1][-1] is C.c_void_p for name in CALLS)
    assert CALLS <= _lib.STATUS and "cs_dcrop_abi_version" not in _lib.STATUS
    assert not (set(h.table) & set(_lib.SCRATCH))                                    # no engine scratch: both may run beside a prefetch
    assert all(name in _lib._TABLES and name in _lib._PTR_SLOTS for name in h.table)
    assert _lib._PTR_SLOTS["cs_crop_lmk"][9] and h.table["cs_crop_lmk"][1][9] is C.POINTER(_lib.LmkLayout)      # the layout: a pointer slot


def test_the_symbols_are_exported_and_bound():
    from canonswap_amd import _lib
    h, _, _ = record()
    lib = _lib.load()
    for name, (ret, args) in h.table.items():
        assert hasattr(lib, name), f"{name}: not exported"
        assert list(getattr(lib, name).argtypes) == list(args) and getattr(lib, name).restype is ret, name
    assert lib.cs_dcrop_abi_version() == h.version == _lib.call("cs_dcrop_abi_version")


# ------------------------------------------------------------------------------------------------ two tuples
def _fake(version=1, with_beside=True):
    from canonswap_amd import _lib
    lib = types.SimpleNamespace()
    for h in _lib.HEADERS + (_lib.HEADERS_BESIDE if with_beside else ()):
        for name in h.table:
            value = 0 if name != h.version_call else version if h in _lib.HEADERS_BESIDE else h.version
            setattr(lib, name, lambda *args, value=value: value)
    return lib


def test_headers_still_is_the_three_records_and_bind_does_not_ask_for_the_new_names():
    from canonswap_amd import _lib
    assert [h.file for h in _lib.HEADERS] == ["canonswap_hip.h", "canonswap_landmarks.h", "canonswap_yuv.h"]
    assert [len(h.table) for h in _lib.HEADERS] == [90, 3, 3]
    lib = _fake(with_beside=False)
    assert _lib.bind(lib) is lib and not hasattr(lib, "cs_crop_lmk")
    with pytest.raises(AttributeError, match="cs_dcrop_abi_version"):                # the in-tree library must carry the header
        _lib.bind_beside(lib)
    assert _lib.bind_beside(lib, ab=True) is lib                                     # an A/B library of an older tree may lack it
    full = _lib.bind_beside(_lib.bind(_fake()))
    for name, (ret, args) in _lib.ABI_DEVICE_CROP.items():
        assert getattr(full, name).restype is ret and getattr(full, name).argtypes == args, name


def test_a_wrong_version_fails_the_load_time_binding_naming_the_header(monkeypatch):
    from canonswap_amd import _lib
    assert os.path.exists(_lib.LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: _fake(version=2))
    with pytest.raises(RuntimeError, match="version 2 of include/canonswap_device_crop.h"):
        _lib.load()
    assert _lib._lib is None


# ------------------------------------------------------------------------------------------------ lmk_crop's restatement
def test_the_restatement_of_lmk_crop_is_float32_line_by_line_and_within_three_roundings_of_float64():
    from canonswap_amd import crop
    import landmarks_ref as LR
    faces = np.stack([LR.synthetic_face(960, 540, 400, 170), LR.synthetic_face(500.3, 500.7, 3, 12), LR.synthetic_face(-2500, 3000, 250, 33)])
    M_o2c, _, host = crop.crop_matrices(faces, dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True)
    worst = 0.0
    for b in range(3):
        got = DR.lmk_crop(faces[b], M_o2c[b])
        assert got.dtype == np.float32 and got.shape == (203, 2)
        val, mag = DR.lmk_crop64(faces[b], M_o2c[b])
        worst = max(worst, float((np.abs(got.astype(np.float64) - val) / (DR.LMK_CROP_ULPS * mag)).max()))
        assert np.abs(got - host[b]).max() <= 2 * DR.LMK_CROP_ULPS * mag.max()          # and the package's own host route, which calls BLAS
    print(f"lmk_crop restatement: largest |d| / bound = {worst:.3f}")
    assert worst <= 1.0
    one = DR.lmk_crop(np.array([[3.0, 5.0]], np.float32), np.array([[2, 0.5, 1], [0, 4, -2], [0, 0, 1]], np.float32))
    assert one.tolist() == [[9.5, 18.0]]


# ------------------------------------------------------------------------------------------------ what the wrappers refuse
class NoLibrary:
    def __getattr__(self, name):
        pytest.fail(f"the library was asked for {name}")


@pytest.fixture
def stub(monkeypatch):
    """An engine that must not be reached: its device is torch's `meta`, so tensors `on the device` exist without a GPU; the library fails the
    test when touched."""
    from canonswap_amd import _lib
    monkeypatch.setattr(_lib, "_lib", NoLibrary())

    class Stub:
        device = torch.device("meta")

        def _call(self, name, *args, **kw):
            pytest.fail(f"{name} was called")
    return Stub()


def _meta(shape, dtype):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_crop_lmk_refuses_before_the_library_is_touched(stub):
    from canonswap_amd import tail
    frames = torch.zeros((3, 8, 12, 3), dtype=torch.uint8)
    good = _meta((4, 203, 2), torch.float32)
    fi = [0, 0, 1, 2]
    for lmk, word in ((torch.zeros((4, 203, 2)), "lmk must be on"), (np.zeros((4, 203, 2), np.float32), "lmk must be a"),
                      (_meta((4, 203, 2), torch.float64), "lmk must be a"), (_meta((4, 203, 3), torch.float32), "lmk must have shape"),
                      (_meta((4, 406), torch.float32), "lmk must have shape"), (_meta((8, 203, 2), torch.float32)[::2], "lmk must be contiguous")):
        with pytest.raises(ValueError, match="crop_lmk: " + word):
            tail.crop_lmk(stub, frames, lmk, fi, dsize=8)
    for bad in ([0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 1], np.array(fi, np.float32)):
        with pytest.raises(ValueError, match="crop_lmk: frame_index"):
            tail.crop_lmk(stub, frames, good, bad, dsize=8)
    with pytest.raises(ValueError, match="crop_lmk: frame_index"):
        tail.crop_lmk(stub, frames, good, None, dsize=8)                                # four faces, three frames, no index
    for out, word in (({"crops": torch.zeros((4, 8, 8, 3), dtype=torch.uint8)}, r"out\['crops'\] must be on"),
                      ({"M": _meta((4, 9), torch.float32)}, r"out\['M'\] must have shape"),
                      ({"lmk_crop": _meta((4, 203, 2), torch.float64)}, r"out\['lmk_crop'\] must be a"),
                      ({"inp": _meta((4, 3, 8, 8), torch.float32)}, "out has no buffer named")):
        with pytest.raises(ValueError, match="crop_lmk: " + word):
            tail.crop_lmk(stub, frames, good, fi, dsize=8, out=out)
    with pytest.raises(ValueError, match="crop_lmk: status must be on"):
        tail.crop_lmk(stub, frames, good, fi, dsize=8, status=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="crop_lmk: status must be a"):
        tail.crop_lmk(stub, frames, good, fi, dsize=8, status=_meta((4,), torch.int64))
    with pytest.raises(ValueError, match="crop_lmk: want_I"):
        tail.crop_lmk(stub, frames, good, fi, dsize=8, want_I=True)
    with pytest.raises(ValueError, match="crop_lmk: dsize 6"):
        tail.crop_lmk(stub, frames, good, fi, dsize=6)
    with pytest.raises(ValueError, match="crop_lmk: frames"):
        tail.crop_lmk(stub, frames.float(), good, fi, dsize=8)
    with pytest.raises(ValueError, match="no landmark layout"):
        tail.crop_lmk(stub, frames, _meta((4, 7, 2), torch.float32), fi, dsize=8)


def test_paste_back_faces_dev_refuses_before_the_library_is_touched(stub):
    from canonswap_amd import tail
    crops, masks = torch.zeros((3, 8, 8, 3), dtype=torch.uint8), torch.zeros((3, 8, 8))
    ori, fi = torch.zeros((2, 12, 16, 3), dtype=torch.uint8), [0, 0, 1]
    M = _meta((3, 18), torch.float32)
    for bad, word in ((torch.zeros((3, 18)), "M must be on"), (np.zeros((3, 18), np.float32), "M must be a"), (_meta((3, 18), torch.float64), "M must be a"),
                      (_meta((3, 3, 3), torch.float32), "M must have shape"), (_meta((2, 18), torch.float32), "M must have shape")):
        with pytest.raises(ValueError, match="paste_back_faces_dev: " + word):
            tail.paste_back_faces_dev(stub, crops, masks, bad, fi, ori)
    for bad in ([0, 1, 0], [0, 0, 2], [0, 0], np.array(fi, np.float32)):
        with pytest.raises(ValueError, match="paste_back_faces_dev: frame_index"):
            tail.paste_back_faces_dev(stub, crops, masks, M, bad, ori)
    with pytest.raises(ValueError, match="paste_back_faces_dev: out must be on"):
        tail.paste_back_faces_dev(stub, crops, masks, M, fi, ori, out=torch.zeros_like(ori))
    with pytest.raises(ValueError, match="paste_back_faces_dev: out must have shape"):
        tail.paste_back_faces_dev(stub, crops, masks, M, fi, ori, out=_meta((3, 12, 16, 3), torch.uint8))
    with pytest.raises(ValueError, match="paste_back_faces_dev: status must be on"):
        tail.paste_back_faces_dev(stub, crops, masks, M, fi, ori, status=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="paste_back_faces_dev: masks_crop"):
        tail.paste_back_faces_dev(stub, crops, masks[:2], M, fi, ori)
    with pytest.raises(ValueError, match="paste_back_faces_dev: crops"):
        tail.paste_back_faces_dev(stub, crops.float(), masks, M, fi, ori)
    with pytest.raises(ValueError, match="paste_back_faces_dev: imgs_ori"):
        tail.paste_back_faces_dev(stub, crops, masks, M, fi, ori[0])


def test_paste_back_batch_names_a_wrong_matrix_count_before_the_library_is_touched(stub):
    from canonswap_amd import tail
    crops, masks = torch.zeros((3, 8, 8, 3), dtype=torch.uint8), torch.zeros((3, 8, 8))
    ori = torch.zeros((3, 12, 16, 3), dtype=torch.uint8)
    for bad in (np.zeros((2, 3, 3)), np.zeros((3, 9)), np.zeros((3, 3, 2))):
        with pytest.raises(ValueError, match="paste_back_batch: M_c2o"):
            tail.paste_back_batch(stub, crops, masks, bad, ori)
    for bad in (np.zeros((2, 3, 3)), np.zeros((3, 6))):
        with pytest.raises(ValueError, match="crop_frames_M: M_o2c"):
            tail.crop_frames_M(stub, ori, bad, 8)
        with pytest.raises(ValueError, match="paste_back_faces: M_c2o"):
            tail.paste_back_faces(stub, crops, masks, bad, [0, 0, 1], ori)
    for bad in (np.zeros((3, 6)), np.zeros((3, 3, 2)), np.zeros((0, 3, 3))):
        with pytest.raises(ValueError, match="crop_faces_M: M_o2c"):
            tail.crop_faces_M(stub, ori[:2], bad, [0, 1, 1][:len(bad)], 8)


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


# every public wrapper that takes 8-bit RGB images: (its name in the message, the argument, a call with that argument as `x`, and what it takes:
# "batch", "one" image, or "either" - a batch, or one image that it makes a batch of)
def _image_wrappers():
    from canonswap_amd import chain, detect, landmarks, tail
    from canonswap_amd.engine import Engine
    M, M3 = np.eye(3), np.stack([np.eye(3)] * 3)
    crops, masks, frames = _u8(3, 8, 8, 3), torch.zeros((3, 8, 8)), _u8(3, 12, 16, 3)
    return [
        ("parser_input", "crops_u8", lambda e, x: tail.parser_input(e, x), "either"),
        ("prepare_crops", "crops_u8", lambda e, x: tail.prepare_crops(e, x), "either"),
        ("rgb_to_yuv", "rgb", lambda e, x: tail.rgb_to_yuv(e, x), "batch"),
        ("paste_back_batch", "crops", lambda e, x: tail.paste_back_batch(e, x, masks, M3, frames), "batch"),
        ("paste_back_batch", "imgs_ori", lambda e, x: tail.paste_back_batch(e, crops, masks, M3, x), "batch"),
        ("paste_back_shared", "crops", lambda e, x: tail.paste_back_shared(e, x, M, frames[0], torch.zeros((12, 16))), "batch"),
        ("paste_back_shared", "img_ori", lambda e, x: tail.paste_back_shared(e, crops, M, x, torch.zeros((12, 16))), "one"),
        ("warp_affine_u8", "img", lambda e, x: tail.warp_affine_u8(e, x, M, (8, 8)), "one"),
        ("paste_back", "img_crop", lambda e, x: tail.paste_back(e, x, M, frames[0], torch.zeros((12, 16))), "one"),
        ("paste_back", "img_ori", lambda e, x: tail.paste_back(e, crops[0], M, x, torch.zeros((12, 16))), "one"),
        ("paste_back_fused", "img_crop", lambda e, x: tail.paste_back_fused(e, x, masks[0], M, frames[0]), "one"),
        ("paste_back_fused", "img_ori", lambda e, x: tail.paste_back_fused(e, crops[0], masks[0], M, x), "one"),
        ("crop_frames_M", "frames", lambda e, x: tail.crop_frames_M(e, x, M3, 8), "batch"),
        ("crop_faces_M", "frames", lambda e, x: tail.crop_faces_M(e, x, M3, [0, 0, 0], 8), "batch"),
        ("paste_back_faces", "imgs_ori", lambda e, x: tail.paste_back_faces(e, crops, masks, M3, [0, 0, 0], x), "batch"),
        ("crop_lmk", "frames", lambda e, x: tail.crop_lmk(e, x, _meta((3, 203, 2), torch.float32), dsize=8), "batch"),
        ("paste_back_faces_dev", "imgs_ori", lambda e, x: tail.paste_back_faces_dev(e, crops, masks, _meta((3, 18), torch.float32), [0, 0, 0], x), "batch"),
        ("unpack_u8", "img_u8", lambda e, x: Engine.unpack_u8(e, x), "batch"),
        ("identity_u8", "crops_u8", lambda e, x: Engine.identity_u8(e, x), "either"),
        ("det_input", "frames", lambda e, x: detect.det_input(e, x), "either"),
        ("lmk_input", "frames", lambda e, x: landmarks.lmk_input(e, x, np.zeros((3, 203, 2), np.float32)), "either"),
        ("FrameChain", "frames_ori", lambda e, x: chain.FrameChain._no_faces(types.SimpleNamespace(e=e), x, [], None), "batch"),
        ("load_source_state", "img_ori", lambda e, x: chain.AnimateChain.load_source_state(
            types.SimpleNamespace(e=e), {"f_swap_can_2": torch.zeros((1, 32, 16, 64, 64)), "x_swap": torch.zeros((1, 21, 3)), "kp_swap": torch.zeros((21, 3)),
                                         "raw_pose": torch.zeros((1, 328)), "img_ori": x}), "one"),
    ]


def test_every_wrapper_refuses_what_is_not_8_bit_rgb_under_its_own_name(stub):
    """The shared check (engine.u8_images): a float tensor, a channel-first tensor and an empty batch are refused with a ValueError that names the
    wrapper and the argument, before the library is touched.  unpack_u8 and prepare_crops alone take an empty batch as far as the library."""
    from canonswap_amd.engine import u8_images
    for who, name, call, takes in _image_wrappers():
        good = _u8(12, 16, 3) if takes == "one" else _u8(3, 12, 16, 3)
        bads = [good.float(), good.movedim(-1, -3).contiguous(), good[..., :0, :], good[0, 0] if takes == "either" else good[0] if takes == "batch" else good[None]]
        if takes != "one" and who not in ("unpack_u8", "prepare_crops"):
            bads.append(good[:0])
        for bad in bads:
            with pytest.raises(ValueError, match=f"{who}: {name} must be"):
                call(stub, bad)
    assert u8_images(np.zeros((2, 4, 4, 3), np.uint8), True, 1, "a", "f").shape == (2, 4, 4, 3)      # an array comes back as a tensor
    assert u8_images(_u8(0, 4, 4, 3), True, 0, "a", "f").shape[0] == 0 and u8_images(_u8(4, 4, 3), False, 1, "a", "f").dim() == 3


def test_the_chain_and_the_swapper_reach_the_wrappers():
    import inspect
    from canonswap_amd import can_swap_e2e, chain
    assert "status" in inspect.signature(chain.FrameChain.__call__).parameters
    assert chain.FrameChain.crop is not chain._StagedChain.crop and chain.AnimateChain.crop is chain._StagedChain.crop
    assert {"crop_lmk", "paste_back_faces_dev"} <= set(vars(can_swap_e2e.can_swapper))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    h, header, rule = record()
    print("\n".join([rule] + render_header(header, h)))
