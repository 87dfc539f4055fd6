"""The C ABI by type, without a GPU, once per record of canonswap_amd/_lib.py HEADERS: the header under include/, the record (its ctypes table, its
structs and constants) and the recorded file under tests/golden/ are rendered to the same text (tests/abi_text.py) and compared line for line; the
loaded library carries exactly the tables; bind() applies the records to whatever library it is given.

`python tests/test_abi_cpu.py [landmarks | yuv]` prints a header's rendering, first line included: that is its file of RECORDED."""
import ctypes as C
import os
import re
import sys
import types

import pytest

from abi_text import mismatches, render_binding, render_header, stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = {"v4": "abi_v4.txt", "landmarks": "abi_landmarks_v1.txt", "yuv": "abi_yuv_v1.txt"}      # in the order of _lib.HEADERS
STREAMS = {"v4": 77, "landmarks": {"cs_lmk_input", "cs_lmk_decode"}, "yuv": {"cs_yuv_to_rgb", "cs_rgb_to_yuv"}}      # how many, or which


def record(key):
    """(key, the record, its header's text, the first line of its recorded file)."""
    from canonswap_amd import _lib
    h = _lib.HEADERS[list(RECORDED).index(key)]
    rule = (f"# C ABI version {h.version} as include/{h.file} declares it (python tests/test_abi_cpu.py{'' if key == 'v4' else ' ' + key}). A changed line "
            f"is a changed meaning of version {h.version}: bump {h.version_define} and record a new file. A new entry point adds a line.")
    return key, h, open(os.path.join(ROOT, "include", h.file)).read(), rule


def recorded(key):
    return open(os.path.join(ROOT, "tests", "golden", RECORDED[key])).read().split("\n")


@pytest.fixture(params=list(RECORDED))
def rec(request):
    return record(request.param)


def test_the_records_are_the_three_headers():
    from canonswap_amd import _lib
    assert [(h.file, h.version, len(h.table), h.ab_may_lack) for h in _lib.HEADERS] == [
        ("canonswap_hip.h", 4, 90, False), ("canonswap_landmarks.h", 1, 3, True), ("canonswap_yuv.h", 1, 3, True)]
    assert [h.table for h in _lib.HEADERS] == [_lib.ABI, _lib.ABI_LANDMARKS, _lib.ABI_YUV]
    assert _lib.ABI_SYMBOLS == list(_lib.ABI) and len(_lib.ConvDesc._fields_) == 65 and _lib.ABI_VERSION == 4
    names = [name for h in _lib.HEADERS for name in h.table]
    assert len(names) == len(set(names)) == 96          # no name stands in two tables


def test_header_equals_binding(rec):
    from canonswap_amd import _lib
    _, h, header, _ = rec
    assert mismatches(render_header(header, h), render_binding(h), "canonswap_amd/_lib.py") == []
    assert render_header(header, h) == render_binding(h)
    assert getattr(_lib.load(), h.version_call)() == h.version


def test_the_table_is_what_got_bound(rec):
    from canonswap_amd import _lib
    lib = _lib.load()
    assert set(_lib.ABI_OPTIONAL) <= set(_lib.ABI)
    for name, (ret, args) in rec[1].table.items():
        assert hasattr(lib, name), f"{name}: not exported"
        assert list(getattr(lib, name).argtypes) == list(args) and getattr(lib, name).restype is ret, name


def test_header_equals_the_recorded_abi(rec):
    key, h, header, rule = rec
    lines = recorded(key)
    assert lines[0] == rule and lines[-1] == ""
    assert mismatches(render_header(header, h), lines[1:-1], "tests/golden/" + RECORDED[key]) == []
    assert render_header(header, h) == lines[1:-1]


def _sub(pattern, repl, text):
    out, n = re.subn(pattern, repl, text, flags=re.S)
    assert n == 1, pattern
    return out


DOCTORED = {      # name that must be reported -> (header, pattern, replacement), applied once to the header's text
    "cs_crop_faces": ("v4", r"(int cs_crop_faces\(cs_engine\* e, )int B", r"\1long B"),
    "cs_face_masks": ("v4", r"(int cs_face_masks\([^)]*uint8_t\* labels),\s*void\* stream\)", r"\1)"),
    "cs_op_id_se_tail": ("v4", r"(int cs_op_id_se_tail\(const float\* out, )long sN, long sH, long sW", r"\1int sN, int sH, int sW"),
    "slope0": ("v4", r"int act0; float slope0;", r"float slope0; int act0;"),      # (both keep their class: only the order tells)
    "ps_stride": ("v4", r" int ps_stride;", r""),
    "cs_pack_u8": ("v4", r"(int cs_pack_u8\([^)]*void\* )stream\)", r"\1st)"),      # (every class stays: only the stream comparison tells)
    "cs_lmk_input": ("landmarks", r"(const float\* lmk, )int N", r"\1long N"),
    "left": ("landmarks", r"int left\[4\]", r"int left[3]"),
    "cs_rgb_to_yuv": ("yuv", r"(int full_range, )int keep", r"\1long keep"),
}
RENAMED_STREAM = "cs_pack_u8"


def test_the_marked_entries_are_the_headers_stream_parameters(rec):
    from canonswap_amd import _lib
    key, h, header, _ = rec
    marked = _lib.TAKES_STREAM & set(h.table)
    assert stream_entries(header) == marked and STREAMS[key] in (len(marked), marked)
    assert all(h.table[name][1][-1] is C.c_void_p for name in marked)


def test_a_renamed_stream_parameter_is_found_by_the_stream_comparison_only():
    from canonswap_amd import _lib
    key, h, header, _ = record(DOCTORED[RENAMED_STREAM][0])
    bad = _sub(*DOCTORED[RENAMED_STREAM][1:], header)
    assert render_header(bad, h) == render_header(header, h)
    marked = _lib.TAKES_STREAM & set(h.table)
    assert marked - stream_entries(bad) == {RENAMED_STREAM} and not stream_entries(bad) - marked


@pytest.mark.parametrize("name", [n for n in DOCTORED if n != RENAMED_STREAM])
def test_the_check_can_fail(name):
    key, h, header, _ = record(DOCTORED[name][0])
    bad = render_header(_sub(*DOCTORED[name][1:], header), h)
    for other, what in ((render_binding(h), "canonswap_amd/_lib.py"), (recorded(key)[1:-1], "tests/golden/" + RECORDED[key])):
        found = mismatches(bad, other, what)
        print(found)
        assert found and any(m.startswith(name + ":") for m in found) and bad != other


def test_an_unknown_type_is_an_error_that_names_its_owner():
    _, h, header, _ = record("v4")
    with pytest.raises(ValueError, match="cs_face_masks.*extend C_CLASS"):
        render_header(header.replace("uint32_t valid_bits", "uint64_t valid_bits"), h)
    with pytest.raises(ValueError, match="cs_conv_desc.hilo.*extend C_CLASS"):
        render_header(header.replace("int hilo;", "short hilo;"), h)


@pytest.mark.parametrize("lacks,ab,lmk_version,error", [      # lacks: canonswap_yuv.h and the ABI_OPTIONAL names; ab: bind()'s A/B flag
    (False, False, 1, None), (True, True, 1, None), (True, False, 1, AttributeError), (False, False, 2, RuntimeError),
], ids=["complete", "ab_library_lacks_a_side_header", "in_tree_library_lacks_a_side_header", "side_header_of_another_version"])
def test_bind_applies_the_records_to_a_fake_library(lacks, ab, lmk_version, error):
    from canonswap_amd import _lib
    gone = set(_lib.ABI_YUV) | set(_lib.ABI_OPTIONAL) if lacks else set()
    lib = types.SimpleNamespace()
    for h in _lib.HEADERS:
        for name in set(h.table) - gone:
            value = 0 if name != h.version_call else lmk_version if h.table is _lib.ABI_LANDMARKS else h.version
            setattr(lib, name, lambda *args, value=value: value)
    if error:
        with pytest.raises(error, match="version 2 of include/canonswap_landmarks.h" if error is RuntimeError else "cs_yuv_abi_version"):
            _lib.bind(lib, ab)
        return
    assert _lib.bind(lib, ab) is lib
    for h in _lib.HEADERS:
        for name, (ret, args) in h.table.items():
            if name in gone:
                with pytest.raises(AttributeError):
                    getattr(lib, name)
            else:
                assert getattr(lib, name).restype is ret and getattr(lib, name).argtypes == args, name


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    key, h, header, rule = record(sys.argv[1] if len(sys.argv) > 1 else "v4")
    print("\n".join([rule] + render_header(header, h)))
