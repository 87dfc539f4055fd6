"""The engine's A/B switches (canonswap_amd/csrc/knobs.h: one struct, one table of environment names and defaults, one reader that cs_create
calls) on the HOST: tests/knobs_host/harness.cpp sets the environment case by case and holds knobs_from_env() to the parsing rules - a default-on
switch is off for any value atoi() reads as 0, CANONSWAP_WIDE is a number, CANONSWAP_AMAX is off unless set to one, the two forms of the vol32
kernel need the kernel.  The header is the one list of the switches: its names are those of INTEGRATION.md section 4, and no other line of csrc
reads a CANONSWAP_* variable except the CSV path of a profiled step."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "canonswap_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FIELDS = ("vol32", "vol32_xf", "vol32_fused", "wide", "warp_fused", "dec_phases_deep", "phase_group", "shortcut_algebra", "shortcut_fuse",
          "shared_dedup", "amax")


def _line(env, **changed):
    v = dict({f: 1 for f in FIELDS}, amax=0)
    v.update(changed)
    return "ok [%s] -> %s" % (env, " ".join(f"{f}={v[f]}" for f in FIELDS))


# derived by hand from the rules above; each must be among the harness' lines
ROWS = [
    _line(""),
    _line("CANONSWAP_PHASE_GROUP=0", phase_group=0),
    _line("CANONSWAP_VOL32_XF=0", vol32_xf=0),
    _line("CANONSWAP_VOL32=0", vol32=0, vol32_xf=0, vol32_fused=0),
    _line("CANONSWAP_VOL32=0 CANONSWAP_VOL32_XF=1 CANONSWAP_VOL32_FUSED=1", vol32=0, vol32_xf=0, vol32_fused=0),
    _line("CANONSWAP_WIDE=2", wide=2),
    _line("CANONSWAP_WIDE=0", wide=0),
    _line("CANONSWAP_WARP_FUSED=", warp_fused=0),
    _line("CANONSWAP_SHARED_DEDUP=on", shared_dedup=0),
    _line("CANONSWAP_AMAX="),
    _line("CANONSWAP_AMAX=on"),
    _line("CANONSWAP_AMAX=1", amax=1),
]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang")
def test_knobs_from_env_on_host(tmp_path):
    exe = str(tmp_path / "h")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "knobs_host", "harness.cpp"), "-o", exe],
                   check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CANONSWAP_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 cases failed" and all(l.startswith("ok [") for l in lines[:-1])
    assert len(lines) - 1 == 1 + 9 + 3 + 1 + 2 * 11 + 1      # defaults, each =0, AMAX / WIDE, the vol32 triple, "" and "on" for all eleven, AMAX=1
    for row in ROWS:
        assert row in lines, row


def test_header_is_host_only_and_the_one_list():
    hdr = open(os.path.join(CSRC, "knobs.h")).read()
    assert "#include <hip" not in hdr and not re.search(r"\bhip[A-Z]\w*", hdr)
    table = re.findall(r'\{"(CANONSWAP_\w+)",', hdr)
    assert len(table) == 11 and len(set(table)) == 11
    # every CANONSWAP_* name of the table's rows, less the three that are not engine switches
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 4. Environment knobs"):].split("\n## ")[0]
    assert "knobs.h" in sec
    rows = [l for l in sec.splitlines() if l.startswith("| ")]
    named = {n for l in rows for n in re.findall(r"CANONSWAP_\w+", l.split("|")[1])}
    assert named - {"CANONSWAP_PROFILE_CSV", "CANONSWAP_LIB", "CANONSWAP_BENCH_BATCH"} == set(table)
    # nothing else in csrc reads the environment for a switch
    calls = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path):
            calls += re.findall(r"getenv\(([^)]*)\)", open(path).read())
    assert sorted(calls) == ['"CANONSWAP_PROFILE_CSV"', "r.env"]      # the CSV path of cs_profile_end, and the reader's one call
