"""The conv_halo launch plan (canonswap_amd/csrc/conv_plan.h: tile configuration, tile decomposition, chunk width, statistics blocks, workgroup
mapping) executed on the HOST: tests/plan_host/harness.cpp runs halo_plan() on the engine's convolutions at 1, 2, 3, 32 and 64 frames and prints one
line per case.  tests/plan_host/expected.txt was recorded from the rules as engine.hip held them before they moved into conv_plan.h (four ternary
chains over the CFG_H_* values, three 128x256 clauses), so a later edit of the plan that changes a tile, a chunk width or a statistics layout shows
up here without a GPU.  ROWS are derived by hand from those rules and must be among the lines."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "plan_host")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

CFG = {"128x128": 10, "128x64": 11, "256x32": 12, "256x16": 15, "128x256": 17, "256x160": 19, "256x64": 20}      # CFG_H_* of common.h
# (harness case, N, tile configuration, lgT (W, H, D), nT (W, H, D, N), ck, statistics blocks per sample or None)
ROWS = [
    ("T.blend", 3, "128x256", (4, 3, 0), (4, 8, 1, 3), 64, None),
    ("T.blend", 2, "128x128", (4, 3, 0), (4, 8, 1, 2), 64, None),
    ("G.m.c", 1, "128x64", (4, 3, 0), (4, 8, 1, 1), 64, 64),
    ("G.up1.n1", 1, "128x128", (4, 3, 0), (16, 32, 1, 1), 32, None),
    ("G.m.spade", 3, "128x256", (4, 3, 0), (4, 8, 1, 3), 64, None),
    ("G.m.spade", 2, "128x128", (4, 3, 0), (4, 8, 1, 2), 64, None),
    ("G.img", 1, "256x16", (4, 4, 0), (16, 16, 1, 1), 64, None),
    ("G.up1.c0", 1, "256x64", (4, 4, 0), (16, 16, 1, 1), 64, 1024),
    ("F.second", 1, "128x64", (4, 3, 0), (4, 8, 1, 1), 32, None),
    ("M.s3.pw2", 64, "128x64", (3, 3, 0), (1, 1, 1, 32), 64, None),
    ("ResBlock3d.stat", 2, "256x32", (2, 2, 4), (16, 16, 1, 2), 32, 1024),
    ("W.enc0", 1, "256x64", (3, 3, 2), (8, 8, 4, 1), 32, None),
    ("W.mask", 1, "256x160", (2, 3, 3), (16, 8, 2, 1), 32, None),
]


def _line(name, N, cfg, lg, nt, ck, nblk):
    return "%s N=%d hcfg=%d lgT=%d,%d,%d nT=%d,%d,%d,%d ck=%d stat_nblk=%s xcd_map=2 persist_total=1" % (
        name, N, CFG[cfg], *lg, *nt, ck, "-" if nblk is None else nblk)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang (ext_vector_type, _Float16)")
def test_halo_plan_on_host(tmp_path):
    csrc = os.path.join(ROOT, "canonswap_amd", "csrc")
    common = open(os.path.join(csrc, "common.h")).read().replace("#include <hip/hip_runtime.h>", "")
    (tmp_path / "common_stub.h").write_text(common[: common.index("#define CS_CHECK_HIP")])
    plan = open(os.path.join(csrc, "conv_plan.h")).read()
    assert plan.count("#include") == 1 and not re.search(r"\bhip[A-Z]\w*", plan)      # common.h only, no HIP call
    (tmp_path / "conv_plan.h").write_text(plan.replace('#include "common.h"', ""))
    shutil.copy(os.path.join(HERE, "harness.cpp"), tmp_path / "h.cpp")
    exe = str(tmp_path / "h")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-Wno-everything", "h.cpp", "-o", exe], cwd=tmp_path, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(HERE, "expected.txt")).read()
    lines = out.splitlines()
    for row in ROWS:
        assert _line(*row) in lines, row
