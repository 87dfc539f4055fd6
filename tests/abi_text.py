"""A C header of include/ and its record of canonswap_amd/_lib.py HEADERS, rendered to the same text: `name: ret(class, ...)` per prototype,
`name class` per field of the record's structs (`class[n]` for an array), `NAME value` for the version and per constant.  The classes are ptr,
int, long, float, double, void, and a struct passed by value is its C name.  tests/test_abi_cpu.py compares the renderings."""
import ctypes as C
import re

C_CLASS = {"int": "int", "uint32_t": "int", "long": "long", "size_t": "long", "float": "float", "double": "double", "void": "void"}
CTYPES_CLASS = {None: "void", C.c_int: "int", C.c_uint32: "int", C.c_long: "long", C.c_size_t: "long", C.c_float: "float", C.c_double: "double",
                C.c_void_p: "ptr", C.c_char_p: "ptr"}


def _c_class(decl, owner, named, structs=()):
    """Class of one C declaration (`const float* x`, `long sN`, `const double M[6]`; named=False: a bare type such as a return type)."""
    if "*" in decl or "[" in decl:
        return "ptr"
    tokens = [t for t in decl.split() if t != "const"]
    if named and len(tokens) > 1:
        tokens = tokens[:-1]
    classes = {**C_CLASS, **{c_name: c_name for c_name in structs}}          # a struct by value: its C name
    if len(tokens) != 1 or tokens[0] not in classes:
        raise ValueError(f"{owner}: `{decl.strip()}` has a type this test does not know: extend C_CLASS")
    return classes[tokens[0]]


def _ctypes_class(t, owner, structs={}):
    classes = {**CTYPES_CLASS, **{cls: c_name for c_name, cls in structs.items()}}
    if t in classes:
        return classes[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    raise ValueError(f"{owner}: ctypes type {t!r} has no class in this test: extend CTYPES_CLASS")


def _uncommented(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def render_header(text, record):
    """The header as lines; raises ValueError for anything in it that is neither a prototype nor named by the record."""
    text = _uncommented(text)
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\w+)", text, flags=re.M))
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    bodies = {}
    for struct in record.structs:
        m = re.search(rf"typedef\s+struct\s+{struct}\s*\{{(.*?)\}}\s*{struct}\s*;", text, flags=re.S)
        if not m:
            raise ValueError(f"{struct}: no such struct in the header")
        bodies[struct], text = m.group(1), text[:m.start()] + text[m.end():]
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
        lines.append(f"{name}: {_c_class(ret, name, False)}({', '.join(_c_class(p, name, True, record.structs) for p in params)})")
    for struct, body in bodies.items():
        for s in filter(str.strip, body.split(";")):
            first, *more = s.split(",")
            base = first[:re.search(r"\w+\s*(\[\d+\])?\s*$", first).start()].replace("*", " ")
            for decl in [first] + [base + d for d in more]:          # `long in_sN, in_sD`: the further declarators share the base type, not the first one's `*`
                decl, name, dim = re.fullmatch(r"(.*?(\w+))\s*(?:\[(\d+)\])?\s*", decl, flags=re.S).groups()
                lines.append(f"{name} {_c_class(decl, f'{struct}.{name}', True)}" + (f"[{dim}]" if dim else ""))
    for name in (record.version_define, *record.constants):
        if name not in defines:
            raise ValueError(f"{name}: not #defined in the header")
        lines.append(f"{name} {defines[name]}")
    return lines


def render_binding(record):
    cls = lambda t, owner: _ctypes_class(t, owner, record.structs)
    lines = [f"{name}: {cls(ret, name)}({', '.join(cls(a, name) for a in args)})" for name, (ret, args) in record.table.items()]
    for struct in record.structs.values():
        for name, t in struct._fields_:          # (`in_` is the field `in`)
            dim, t = (f"[{t._length_}]", t._type_) if issubclass(t, C.Array) else ("", t)
            lines.append(f"{name.rstrip('_')} {_ctypes_class(t, f'{struct.__name__}.{name}')}{dim}")
    return lines + [f"{record.version_define} {record.version}"] + [f"{name} {value}" for name, value in record.constants.items()]


def stream_entries(text):
    """The header's prototypes whose last parameter is named `stream`."""
    return {name for name, params in re.findall(r"\b(cs_\w+)\s*\(([^)]*)\)\s*;", _uncommented(text)) if re.search(r"\bstream\s*$", params)}


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
