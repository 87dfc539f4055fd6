"""Every preprocessor name the kernel sources test can be defined by something in the tree (no GPU).

A fork behind `#ifdef X` that no build, tool or test can take is dead text in the files where changes go wrong most often
(INTEGRATION.md lists the switches that exist and who defines each).  No allow-list: a new fork passes exactly when
something can build it."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = (".py", ".sh", ".hip", ".h", ".hpp", ".c", ".cpp", ".txt", ".cmake")


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def undefinable_switches(root):
    """{name: [file:line, ...]} of the names tested by the sources under `root` that nothing there defines."""
    srcs = sorted(glob.glob(os.path.join(root, "canonswap_amd", "csrc", "*.h")) + glob.glob(os.path.join(root, "canonswap_amd", "csrc", "*.hip")))
    srcs.append(os.path.join(root, "include", "canonswap_hip.h"))
    tested, defined = {}, set()
    for path in srcs:
        no = 1
        for line in re.split(r"(?<!\\)\n", _read(path)):          # logical lines: a continued directive is one directive
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif|define)\b(.*)", line, re.S)
            if m and m.group(1) == "define":
                defined.add(re.match(r"\s*(\w+)", m.group(2)).group(1))
            elif m:
                pat = r"^\s*(\w+)" if m.group(1) in ("ifdef", "ifndef") else r"\bdefined\s*\(?\s*(\w+)"
                for name in re.findall(pat, m.group(2)):
                    if not name.startswith("__"):
                        tested.setdefault(name, []).append(f"{os.path.relpath(path, root)}:{no}")
            no += line.count("\n") + 1
    users = [os.path.join(root, "canonswap_amd", "_build.py")]
    for sub in ("tools", "tests"):
        for d, dirs, files in os.walk(os.path.join(root, sub)):
            dirs[:] = [x for x in dirs if x not in ("golden", "__pycache__")]
            users += [os.path.join(d, f) for f in files if f.endswith(TEXT)]
    flags = set()
    for path in users:
        flags.update(re.findall(r"-D(\w+)", _read(path)))
    return {n: where for n, where in tested.items() if n not in defined and n not in flags}


def test_every_tested_switch_can_be_defined():
    dead = undefinable_switches(ROOT)
    assert not dead, "preprocessor names that no source #defines and no build, tool or test passes as a flag: " + \
        "; ".join(f"{n} ({', '.join(w)})" for n, w in sorted(dead.items()))
