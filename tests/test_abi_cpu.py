"""The C ABI by type, without a GPU: include/canonswap_hip.h, the ctypes table canonswap_amd/_lib.py ABI (with ConvDesc and the constants) and
the recorded tests/golden/abi_v4.txt are rendered to the same text and compared line for line; the loaded library carries exactly the table.

`python tests/test_abi_cpu.py` prints the header's rendering, first line included: that is tests/golden/abi_v4.txt."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "canonswap_hip.h")
RECORD = os.path.join(ROOT, "tests", "golden", "abi_v4.txt")
RULE = ("# C ABI version 4 as include/canonswap_hip.h declares it (python tests/test_abi_cpu.py). A changed line is a changed meaning of version 4: "
        "bump CS_ABI_VERSION and record a new file. A new entry point adds a line.")
CONSTANTS = {"CS_ABI_VERSION": "ABI_VERSION", "CS_MAX_IDENTITY_SLOTS": "MAX_IDENTITY_SLOTS", "CS_DET_MAX_CAND": "DET_MAX_CAND",
             "CS_DET_MAX_FACES": "DET_MAX_FACES"}
C_CLASS = {"int": "int", "uint32_t": "int", "long": "long", "size_t": "long", "float": "float", "double": "double", "void": "void"}
CTYPES_CLASS = {None: "void", C.c_int: "int", C.c_uint32: "int", C.c_long: "long", C.c_size_t: "long", C.c_float: "float", C.c_double: "double",
                C.c_void_p: "ptr", C.c_char_p: "ptr"}


def _c_class(decl, owner, named):
    """Class of one C declaration (`const float* x`, `long sN`, `const double M[6]`; named=False: a bare type such as a return type)."""
    if "*" in decl or "[" in decl:
        return "ptr"
    tokens = [t for t in decl.split() if t != "const"]
    if named and len(tokens) > 1:
        tokens = tokens[:-1]
    if len(tokens) != 1 or tokens[0] not in C_CLASS:
        raise ValueError(f"{owner}: `{decl.strip()}` has a type this test does not know: extend C_CLASS")
    return C_CLASS[tokens[0]]


def render_header(text):
    """The header as lines: `name: ret(class, ...)` per prototype, `name class` per cs_conv_desc field, `NAME value` per constant."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\w+)", text, flags=re.M))
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    struct = re.search(r"typedef\s+struct\s+cs_conv_desc\s*\{(.*?)\}\s*cs_conv_desc\s*;", text, flags=re.S)
    if not struct:
        raise ValueError("cs_conv_desc: no such struct in the header")
    text = text[:struct.start()] + text[struct.end():]
    text = re.sub(r"\benum\s*\{[^}]*\}\s*;", " ", text)
    text = re.sub(r"\btypedef\s+struct\s+cs_engine\s+cs_engine\s*;", " ", text)
    *statements, rest = text.split(";")
    if rest.strip() != "}":
        raise ValueError(f"the header ends in `{rest.strip()}`, not in the brace that closes extern \"C\"")
    lines = []
    for s in statements:
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(cs_\w+)\s*\((.*)\)\s*", s, flags=re.S)
        if not m:
            raise ValueError(f"`{' '.join(s.split())}` is neither a prototype nor anything else this test knows")
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        lines.append(f"{name}: {_c_class(ret, name, False)}({', '.join(_c_class(p, name, True) for p in params)})")
    for s in struct.group(1).split(";"):
        if not s.strip():
            continue
        first, *more = s.split(",")
        name = re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", first).group(1)
        lines.append(f"{name} {_c_class(first, 'cs_conv_desc.' + name, True)}")
        base = first[:first.rindex(name)].replace("*", " ")
        for d in more:          # `long in_sN, in_sD`: the further declarators share the base type, not the first one's `*`
            name = re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", d).group(1)
            lines.append(f"{name} {_c_class(base + d, 'cs_conv_desc.' + name, True)}")
    for name in CONSTANTS:
        if name not in defines:
            raise ValueError(f"{name}: not #defined in the header")
        lines.append(f"{name} {defines[name]}")
    return lines


def stream_entries(text):
    """The header's prototypes whose last parameter is named `stream`."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    return {name for name, params in re.findall(r"\b(cs_\w+)\s*\(([^)]*)\)\s*;", text) if re.search(r"\bstream\s*$", params)}


def _ctypes_class(t, owner):
    if t in CTYPES_CLASS:
        return CTYPES_CLASS[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    raise ValueError(f"{owner}: ctypes type {t!r} has no class in this test: extend CTYPES_CLASS")


def render_binding(_lib):
    lines = [f"{name}: {_ctypes_class(ret, name)}({', '.join(_ctypes_class(a, name) for a in args)})" for name, (ret, args) in _lib.ABI.items()]
    lines += [f"{'in' if name == 'in_' else name} {_ctypes_class(t, 'ConvDesc.' + name)}" for name, t in _lib.ConvDesc._fields_]
    return lines + [f"{c} {getattr(_lib, py)}" for c, py in CONSTANTS.items()]


def mismatches(header, other, what):
    """One message per name on which the two renderings disagree ([] when they are equal line for line), each beginning with the name."""
    key = lambda line: line.split()[0].rstrip(":")
    a, b = {key(l): l for l in header}, {key(l): l for l in other}
    out = [f"{n}: in the header, not in {what}" for n in a if n not in b] + [f"{n}: in {what}, not in the header" for n in b if n not in a]
    out += [f"{n}: the header says `{a[n]}`, {what} `{b[n]}`" for n in a if n in b and a[n] != b[n]]
    if len(a) != len(header) or len(b) != len(other):
        out.append(f"a name stands twice in the header or in {what}")
    if not out and header != other:
        i = next(i for i, (x, y) in enumerate(zip(header, other)) if x != y)
        out.append(f"{key(header[i])}: line {i + 1} of the header's order, where {what} has {key(other[i])}")
    return out


@pytest.fixture(scope="module")
def header():
    return open(HEADER).read()


def test_header_equals_binding(header):
    from canonswap_amd import _lib
    assert _lib.ABI_SYMBOLS == list(_lib.ABI) and len(_lib.ABI) == 90 and len(_lib.ConvDesc._fields_) == 65
    assert mismatches(render_header(header), render_binding(_lib), "canonswap_amd/_lib.py") == []
    assert render_header(header) == render_binding(_lib)
    assert _lib.load().cs_abi_version() == _lib.ABI_VERSION == 4


def test_the_table_is_what_got_bound():
    from canonswap_amd import _lib
    lib = _lib.load()
    assert set(_lib.ABI_OPTIONAL) <= set(_lib.ABI)
    for name, (ret, args) in _lib.ABI.items():
        assert hasattr(lib, name), f"{name}: not exported"
        f = getattr(lib, name)
        assert list(f.argtypes) == list(args), name
        assert f.restype is ret, name


def test_header_equals_the_recorded_abi(header):
    recorded = open(RECORD).read().split("\n")
    assert recorded[0] == RULE and recorded[-1] == ""
    assert mismatches(render_header(header), recorded[1:-1], "tests/golden/abi_v4.txt") == []
    assert render_header(header) == recorded[1:-1]


def _sub(pattern, repl, text):
    out, n = re.subn(pattern, repl, text, flags=re.S)
    assert n == 1, pattern
    return out


DOCTORED = {      # name that must be reported -> (pattern, replacement) applied once to the header text
    "cs_crop_faces": (r"(int cs_crop_faces\(cs_engine\* e, )int B", r"\1long B"),
    "cs_face_masks": (r"(int cs_face_masks\([^)]*uint8_t\* labels),\s*void\* stream\)", r"\1)"),
    "cs_op_id_se_tail": (r"(int cs_op_id_se_tail\(const float\* out, )long sN, long sH, long sW", r"\1int sN, int sH, int sW"),
    "slope0": (r"int act0; float slope0;", r"float slope0; int act0;"),      # (both keep their class: only the order tells)
    "ps_stride": (r" int ps_stride;", r""),
    "cs_pack_u8": (r"(int cs_pack_u8\([^)]*void\* )stream\)", r"\1st)"),      # (every class stays: only the stream comparison tells)
}
RENAMED_STREAM = "cs_pack_u8"


def test_the_marked_entries_are_the_headers_stream_parameters(header):
    from canonswap_amd import _lib
    assert stream_entries(header) == set(_lib.TAKES_STREAM) and len(_lib.TAKES_STREAM) == 77
    assert all(_lib.ABI[name][1][-1] is C.c_void_p for name in _lib.TAKES_STREAM)
    bad = _sub(*DOCTORED[RENAMED_STREAM], header)
    assert render_header(bad) == render_header(header)
    assert set(_lib.TAKES_STREAM) - stream_entries(bad) == {RENAMED_STREAM} and not stream_entries(bad) - set(_lib.TAKES_STREAM)


@pytest.mark.parametrize("name", [n for n in DOCTORED if n != RENAMED_STREAM])
def test_the_check_can_fail(header, name):
    from canonswap_amd import _lib
    pattern, repl = DOCTORED[name]
    bad = render_header(_sub(pattern, repl, header))
    for other, what in ((render_binding(_lib), "canonswap_amd/_lib.py"), (open(RECORD).read().split("\n")[1:-1], "tests/golden/abi_v4.txt")):
        found = mismatches(bad, other, what)
        print(found)
        assert found and any(m.startswith(name + ":") for m in found) and bad != other


def test_an_unknown_type_is_an_error_that_names_its_owner(header):
    with pytest.raises(ValueError, match="cs_face_masks.*extend C_CLASS"):
        render_header(header.replace("uint32_t valid_bits", "uint64_t valid_bits"))
    with pytest.raises(ValueError, match="cs_conv_desc.hilo.*extend C_CLASS"):
        render_header(header.replace("int hilo;", "short hilo;"))


if __name__ == "__main__":
    print("\n".join([RULE] + render_header(open(HEADER).read())))
