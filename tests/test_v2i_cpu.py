"""The C-ABI and Python surface of the v2i device-side frame (AnimateChain), checked without a GPU: the three entry points
are declared in the header with their documented argument counts, listed in _lib.ABI_SYMBOLS, bound with as many argtypes and exported by
the built library; the ABI version did not move; the Python names import."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments of the declaration in include/canonswap_hip.h
NEW = {
    "cs_resize_half_bilinear": 8,         # e, B, C, img, H, W, out, stream
    "cs_motion_keypoints_driven": 7,      # e, B, raw_driving, raw_pose, kp, x_t, stream
    "cs_paste_back_shared": 12,           # e, B, crops, Hc, Wc, mask_ori, M_c2o, img_ori, out, Ho, Wo, stream
}


def _declarations():
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(cs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header)}


def test_new_entry_points_are_declared_with_their_argument_counts():
    decl = _declarations()
    for name, nargs in NEW.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == nargs, (name, decl[name])


def test_new_entry_points_are_bound_and_exported_and_the_abi_version_stays():
    from canonswap_amd import _lib
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    assert re.search(r"#define\s+CS_ABI_VERSION\s+4\b", header)
    assert _lib.ABI_VERSION == 4
    lib = _lib.load()
    assert lib.cs_abi_version() == 4
    for name, nargs in NEW.items():
        assert name in _lib.ABI_SYMBOLS, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.chain import AnimateChain, FrameChain
    from canonswap_amd.engine import Engine
    assert callable(tail.paste_back_shared)
    assert callable(Engine.resize_half_bilinear) and callable(Engine.motion_keypoints_driven)
    for name in ("set_source", "source_state", "load_source_state", "prefetch", "drop_prefetches", "__call__"):
        assert callable(getattr(AnimateChain, name)), name
    assert AnimateChain is not FrameChain
