"""The in-tree build of libcanonswap_hip.so and of the test-only cross-check library (hipcc cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = [os.path.join(CSRC, f) for f in ("conv_halo.hip", "conv_wide.hip", "conv_lat.hip", "vol32.hip", "vol32_fused.hip", "kernels.hip", "motion.hip", "imgops.hip", "detect.hip", "landmarks.hip", "yuv.hip", "identity.hip", "parser.hip", "engine.hip", "engine_image.hip", "engine_ops.hip")]
# test-only cross-check kernel (the first-generation implicit-GEMM conv): its own library, never linked into the product
TEST_SRC = os.path.join(os.path.dirname(HERE), "tests", "csrc", "test_igemm.hip")
TEST_LIB_PATH = os.path.join(os.path.dirname(HERE), "tests", "libcanonswap_test.so")
HEADERS = [os.path.join(CSRC, f) for f in ("common.h", "conv_epilogue.h", "conv_halo_kernel.h", "conv_plan.h", "engine.h", "affine_inv.h", "knobs.h", "lmk_geometry.h", "warp_taps.h", "yuv_math.h")] + \
          [os.path.join(os.path.dirname(HERE), "include", f) for f in ("canonswap_hip.h", "canonswap_landmarks.h", "canonswap_yuv.h", "canonswap_device_crop.h")]
HALO_NGROUPS = 8          # conv_halo.hip is compiled once per -DHALO_GROUP=k (slices of its instantiation table)
OBJ_DIR = os.path.join(HERE, "build")
LIB_PATH = os.environ.get("CANONSWAP_LIB") or os.path.join(HERE, "libcanonswap_hip.so")      # CANONSWAP_LIB: A/B builds (tools/)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]


def _units():
    """(source, object name, extra flags) of every translation unit."""
    units = []
    for src in SOURCES:
        base = os.path.splitext(os.path.basename(src))[0]
        if base == "conv_halo":
            units += [(src, f"conv_halo_g{g}.o", [f"-DHALO_GROUP={g}"]) for g in range(HALO_NGROUPS)]
        else:
            units.append((src, base + ".o", []))
    return units


def build(force: bool = False, lib_path: str | None = None, extra_flags=(), obj_dir: str | None = None, jobs: int | None = None) -> str:
    """Compile the HIP sources for gfx950 into canonswap_amd/libcanonswap_hip.so (hipcc cross-compiles without a GPU).

    Objects are cached under canonswap_amd/build/ and rebuilt when their source, any header or the flags changed; the
    translation units compile in parallel."""
    from concurrent.futures import ThreadPoolExecutor
    lib_path = lib_path or LIB_PATH
    obj_dir = obj_dir or OBJ_DIR
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = HIPCC_FLAGS + list(extra_flags)
    stamp = " ".join([hipcc] + flags)
    hdr_time = max(os.path.getmtime(p) for p in HEADERS)
    todo, objs = [], []
    for src, oname, extra in _units():
        obj = os.path.join(obj_dir, oname)
        objs.append(obj)
        tag = obj + ".flags"
        fresh = (not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(hdr_time, os.path.getmtime(src))
                 and os.path.exists(tag) and open(tag).read() == stamp + " " + " ".join(extra))
        if not fresh:
            todo.append((src, obj, extra, tag))

    def compile_one(job):
        src, obj, extra, tag = job
        subprocess.run([hipcc, *flags, *extra, "-c", src, "-o", obj], check=True)
        with open(tag, "w") as f:
            f.write(stamp + " " + " ".join(extra))

    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(len(todo), os.cpu_count() or 4)) as ex:
            list(ex.map(compile_one, todo))
    if todo or not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(os.path.getmtime(o) for o in objs):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib_path], check=True)
    return lib_path


def build_test_lib(force: bool = False) -> str:
    """tests/libcanonswap_test.so = tests/csrc/test_igemm.hip (+ conv_igemm.hip): used by tests/hip_ops.py only."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = [TEST_SRC, os.path.join(os.path.dirname(TEST_SRC), "conv_igemm.hip")] + HEADERS
    if force or not os.path.exists(TEST_LIB_PATH) or os.path.getmtime(TEST_LIB_PATH) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([hipcc, *HIPCC_FLAGS, "-shared", "-Wl,-Bsymbolic", TEST_SRC, "-o", TEST_LIB_PATH], check=True)
    return TEST_LIB_PATH


def toolchain() -> str:
    """hipcc version string (recorded by build(): the dynamic-shape conv kernels rely on hand-counted waits, see conv_halo_kernel.h)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return " | ".join(l.strip() for l in out.splitlines() if "version" in l.lower())[:200]
