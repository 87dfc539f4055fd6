"""The launch plan and the dispatch table of conv_halo for the cases of tests/conv_cases.py, without a GPU: halo_plan() executed on the host
(tests/plan_host/rows.cpp, built like tests/plan_host/harness.cpp) and the call sites of canonswap_amd/csrc/conv_halo.hip read from its text."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import conv_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "canonswap_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
MODES = {"MODE_STD": cc.STD, "MODE_TBLEND": cc.TBLEND, "MODE_SPADE": cc.SPADE, "MODE_PIXSHUF": cc.PIXSHUF, "MODE_STDSTAT": cc.STDSTAT}


@functools.lru_cache(None)
def plans():
    """case name -> dict(hcfg, ck, lgT, nT, stat_nblk, nchunks, BM, BN, wave_px): what halo_plan() answers for the case as cs_op_conv asks"""
    with tempfile.TemporaryDirectory() as tmp:
        common = open(os.path.join(CSRC, "common.h")).read().replace("#include <hip/hip_runtime.h>", "")
        open(os.path.join(tmp, "common_stub.h"), "w").write(common[: common.index("#define CS_CHECK_HIP")])
        open(os.path.join(tmp, "conv_plan.h"), "w").write(open(os.path.join(CSRC, "conv_plan.h")).read().replace('#include "common.h"', ""))
        shutil.copy(os.path.join(ROOT, "tests", "plan_host", "rows.cpp"), os.path.join(tmp, "rows.cpp"))
        subprocess.run([CLANG, "-std=c++17", "-O1", "-Wno-everything", "rows.cpp", "-o", "rows"], cwd=tmp, check=True)
        lines = []
        for c in cc.CASES:
            N, D, H, W = c["dims"]
            N *= c.get("rep", 1)
            hcfg, ck, mode, _ = c["row"]
            lines.append("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (c["name"], mode, *c["k"], c["cin"], c["cout_pad"], N, D, H, W,
                                                                    -1 if c.get("planned") else hcfg, *c["tile"], 0 if c.get("planned") else ck))
        out = subprocess.run([os.path.join(tmp, "rows")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    res = {}
    for line in out.splitlines():
        name, rest = line.split(" ", 1)
        kv = dict(f.split("=") for f in rest.split())
        res[name] = dict(hcfg=int(kv["hcfg"]), ck=int(kv["ck"]), lgT=tuple(int(v) for v in kv["lgT"].split(",")),
                         nT=tuple(int(v) for v in kv["nT"].split(",")), stat_nblk=int(kv["stat_nblk"]), nchunks=int(kv["nchunks"]), BM=int(kv["BM"]),
                         BN=int(kv["BN"]), wave_px=int(kv["wave_px"]))
    assert len(res) == len(cc.CASES)
    return res


def static_shapes():
    """StaticShape<ST> of conv_halo_kernel.h: ST -> (KD, KH, KW, LW, LH, LD)"""
    text = open(os.path.join(CSRC, "conv_halo_kernel.h")).read()
    pat = r"template <> struct StaticShape<(\d+)> \{ static constexpr int KD = (\d+), KH = (\d+), KW = (\d+), LW = (\d+), LH = (\d+), LD = (\d+); \};"
    shapes = {int(m[0]): tuple(int(v) for v in m[1:]) for m in re.findall(pat, text)}
    assert len(shapes) == text.count("struct StaticShape<") and len(shapes) >= 17
    return shapes


def _hcfg(wpx, wch, wvp, wvc, sk):
    bm, bn = wpx * 16 * (1 if sk else wvp), wch * 16 * wvc
    if sk:
        assert (bm, bn) == (128, 32)
        return 16
    (h,) = [k for k, v in cc.TILES.items() if v[1:3] == (bm, bn) and k != 16]
    return h


def dispatch_rows():
    """The rows conv_halo.hip can launch, from its text: every launch_halo_st<...> call site is one row; every launch_halo_cfg<..., STV> call
    site is the static row STV (when STV != 0) and its dynamic form, except on the 128x256 tiles (WCH == 4), which have none (launch_halo_cfg);
    every HALO_CASE line is the four launch_halo_cfg arms of the macro."""
    text = open(os.path.join(CSRC, "conv_halo.hip")).read()
    macro = text[text.index("#define HALO_CASE"):text.index("#define GROUP_FN")]
    arms = re.findall(r"launch_halo_cfg<(\d+), WPX, WCH, WVP, WVC, MODE, SK, ([^>]+)>", macro)
    assert arms == [("64", "ST2D"), ("32", "ST2D"), ("32", "(ST3D == 2 ? 5 : 0)"), ("32", "ST3D")], "HALO_CASE changed: update dispatch_rows()"
    assert "if constexpr (WCH == 4) {" in text[:text.index("#define HALO_CASE")], "launch_halo_cfg changed: update dispatch_rows()"
    tmpl = r"<(\d+), (\d+), (\d+), (\d+), (\d+), (MODE_\w+), (true|false), (\d+)>"
    rows = set()

    def cfg_site(ck, wpx, wch, wvp, wvc, mode, sk, stv):
        h = _hcfg(wpx, wch, wvp, wvc, sk)
        if stv:
            rows.add((h, ck, mode, stv))
        if wch != 4:
            rows.add((h, ck, mode, 0))

    for kind, *a in re.findall(r"launch_halo_(cfg|st)" + tmpl, text):
        ck, wpx, wch, wvp, wvc, mode, sk, stv = int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(a[4]), MODES[a[5]], a[6] == "true", int(a[7])
        if kind == "st":
            rows.add((_hcfg(wpx, wch, wvp, wvc, sk), ck, mode, stv))
        else:
            cfg_site(ck, wpx, wch, wvp, wvc, mode, sk, stv)
    cases = re.findall(r"^\s*HALO_CASE\((CFG_H_\w+), (\d+), (\d+), (\d+), (\d+), (MODE_\w+), (true|false), (\d+), (\d+)\)", text, re.M)
    assert len(cases) == len(re.findall(r"^\s*HALO_CASE\(", text, re.M))
    for name, wpx, wch, wvp, wvc, mode, sk, st2, st3 in cases:
        wpx, wch, wvp, wvc, st2, st3, sk = int(wpx), int(wch), int(wvp), int(wvc), int(st2), int(st3), sk == "true"
        assert "CFG_H_" + ("SK" if sk else "") + cc.TILES[_hcfg(wpx, wch, wvp, wvc, sk)][0].replace("SK", "") == name, name
        for ck, stv in ((64, st2), (32, st2), (32, 5 if st3 == 2 else 0), (32, st3)):
            cfg_site(ck, wpx, wch, wvp, wvc, MODES[mode], sk, stv)
    return rows


def static_match(case, plan, rows, shapes):
    """the static shapes among the rows of the case's (tile configuration, chunk width, mode) whose launch_halo_cfg condition the launch meets"""
    hcfg, ck, mode, _ = case["row"]
    out = []
    for (h, c, m, stv) in rows:
        if (h, c, m) == (hcfg, ck, mode) and stv and shapes[stv] == tuple(case["k"]) + plan["lgT"] and plan["nchunks"] % (ck // 32) == 0:
            out.append(stv)
    return sorted(out)
