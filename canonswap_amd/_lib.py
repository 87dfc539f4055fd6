"""ctypes binding of libcanonswap_hip.so (C ABI: include/canonswap_hip.h, and include/canonswap_landmarks.h, include/canonswap_yuv.h and
include/canonswap_device_crop.h beside it).

The library is the product: if it cannot be loaded, every entry point raises -- there is no CPU or
PyTorch fallback (the CPU restatement under oracle/ is test infrastructure only).  The in-tree build is _build.py,
the disassembly checks of the built objects are _isa.py.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import torch          # before the library is loaded, see load()

from ._build import LIB_PATH, TEST_LIB_PATH

ABI_VERSION = 4          # CS_ABI_VERSION of include/canonswap_hip.h
MAX_IDENTITY_SLOTS = 8      # CS_MAX_IDENTITY_SLOTS (include/canonswap_hip.h)
DET_MAX_CAND = 1024         # CS_DET_MAX_CAND: candidates per frame cs_det_decode takes
DET_MAX_FACES = 256         # CS_DET_MAX_FACES: the largest max_faces of cs_det_decode


class ConvDesc(C.Structure):
    """Mirror of cs_conv_desc (include/canonswap_hip.h)."""
    _fields_ = [
        ("in_", C.c_void_p), ("in_sN", C.c_long), ("in_sD", C.c_long), ("in_sH", C.c_long), ("in_sW", C.c_long),
        ("N", C.c_int), ("D", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("up_shift", C.c_int),
        ("KD", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
        ("wgt", C.c_void_p), ("Cout_pad", C.c_int), ("Cout", C.c_int),
        ("bias", C.c_void_p), ("bias2", C.c_void_p),
        ("act0", C.c_int), ("slope0", C.c_float),
        ("res", C.c_void_p), ("res_f32", C.c_int), ("res_shift", C.c_int),
        ("res_sN", C.c_long), ("res_sD", C.c_long), ("res_sH", C.c_long), ("res_sW", C.c_long),
        ("pixscale", C.c_void_p), ("ps_stride", C.c_int),
        ("out0", C.c_void_p), ("out0_f32", C.c_int),
        ("out0_sN", C.c_long), ("out0_sD", C.c_long), ("out0_sH", C.c_long), ("out0_sW", C.c_long),
        ("s2", C.c_void_p), ("t2", C.c_void_p), ("act1", C.c_int), ("slope1", C.c_float),
        ("out1", C.c_void_p), ("out1_sN", C.c_long), ("out1_sD", C.c_long), ("out1_sH", C.c_long), ("out1_sW", C.c_long),
        ("stats", C.c_void_p),
        ("mode", C.c_int), ("cfg", C.c_int), ("tile_w", C.c_int), ("tile_h", C.c_int), ("ck", C.c_int), ("xcd_map", C.c_int), ("ragged", C.c_int),
        ("hilo", C.c_int), ("stat_out", C.c_void_p),
        ("xf_kind", C.c_int), ("xf_y", C.c_void_p), ("xf_res", C.c_void_p), ("xf_out", C.c_void_p),
        ("xf_stats", C.c_void_p), ("xf_gamma", C.c_void_p), ("xf_beta", C.c_void_p), ("xf_slope", C.c_float),
        ("ep_general", C.c_int), ("pool_hw", C.c_int),
    ]


class LmkLayout(C.Structure):
    """Mirror of cs_lmk_layout (include/canonswap_landmarks.h); passed by value."""
    _fields_ = [("n_eye", C.c_int), ("left", C.c_int * 4), ("right", C.c_int * 4), ("lip", C.c_int * 2)]


vp, ci, cf, cl, cd = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_double
pi, pd, pvp = C.POINTER(ci), C.POINTER(cd), C.POINTER(vp)
# The binding, stated once: entry point -> (restype, argtypes), in the order of include/canonswap_hip.h.  tests/test_abi_cpu.py compares it with the
# header class by class (pointer / int / long / float / double), and the header with the recorded tests/golden/abi_v4.txt (HEADERS below).
ABI = {
    "cs_create": (ci, [ci, ci, pvp]),
    "cs_destroy": (None, [vp]),
    "cs_last_error": (C.c_char_p, []),
    "cs_abi_version": (ci, []),          # the one c_int that is a value, not a status (STATUS below)
    "cs_upload": (ci, [vp, C.c_char_p, vp, C.c_size_t]),
    "cs_finalize_weights": (ci, [vp]),
    "cs_set_identity": (ci, [vp, ci, vp, vp]),
    "cs_identity": (ci, [vp, ci, vp, ci, ci, vp, vp, vp]),
    "cs_identity_u8": (ci, [vp, ci, vp, ci, ci, vp, vp, vp, vp]),
    "cs_parser": (ci, [vp, ci, vp, ci, ci, vp, vp]),
    "cs_set_latency_mode": (ci, [vp, ci]),
    "cs_extract_feature_3d": (ci, [vp, ci, vp, vp, vp]),
    "cs_warp": (ci, [vp, ci, vp, vp, vp, vp, vp, vp]),
    "cs_warp_out": (ci, [vp, ci, vp, vp, vp, vp]),
    "cs_swap": (ci, [vp, ci, ci, vp, vp, vp]),
    "cs_swap_ids": (ci, [vp, pi, ci, vp, vp, vp]),
    "cs_refine": (ci, [vp, ci, vp, vp, vp]),
    "cs_warp_forward": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp]),
    "cs_spade_decode": (ci, [vp, ci, vp, vp, vp]),
    "cs_motion_extract": (ci, [vp, ci, vp, vp, vp]),
    "cs_pack_u8": (ci, [vp, ci, vp, vp, ci, ci, vp]),
    "cs_unpack_u8": (ci, [vp, ci, vp, vp, ci, ci, vp]),
    "cs_swap_frames": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "cs_swap_frames_ids": (ci, [vp, pi, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "cs_animate_frames": (ci, [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp]),
    "cs_soft_erosion": (ci, [vp, ci, ci, ci, vp, vp, ci, cf, ci, vp, vp, vp]),
    "cs_prepare_crops": (ci, [vp, ci, vp, ci, ci, vp, vp]),
    "cs_warp_affine_u8": (ci, [vp, vp, ci, ci, pd, vp, ci, ci, vp]),
    "cs_warp_affine_f32": (ci, [vp, vp, ci, ci, pd, vp, ci, ci, vp]),
    "cs_paste_back": (ci, [vp, vp, vp, vp, ci, ci, pd, vp, vp, ci, ci, vp]),
    "cs_soft_erosion_frames": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, cf, ci, vp, vp, vp]),
    "cs_paste_back_batch": (ci, [vp, ci, vp, vp, ci, ci, pd, vp, vp, ci, ci, vp]),
    "cs_motion_keypoints": (ci, [vp, ci, vp, vp, vp, vp, vp]),
    "cs_resize_half_bilinear": (ci, [vp, ci, ci, vp, ci, ci, vp, vp]),
    "cs_motion_keypoints_driven": (ci, [vp, ci, vp, vp, vp, vp, vp]),
    "cs_paste_back_shared": (ci, [vp, ci, vp, ci, ci, vp, pd, vp, vp, ci, ci, vp]),
    "cs_crop_frames": (ci, [vp, ci, vp, ci, ci, pd, ci, vp, vp, vp]),
    "cs_crop_faces": (ci, [vp, ci, ci, vp, ci, ci, pi, pd, ci, vp, vp, vp]),
    "cs_paste_back_faces": (ci, [vp, ci, ci, vp, vp, ci, ci, pi, pd, vp, vp, ci, ci, vp]),
    "cs_face_masks": (ci, [vp, ci, ci, vp, ci, ci, ci, C.c_uint32, vp, vp, vp]),
    "cs_parser_input": (ci, [vp, ci, vp, ci, ci, ci, vp, vp, vp, vp]),
    "cs_concat_frames": (ci, [vp, ci, ci, ci, pvp, pi, pi, vp, vp]),
    "cs_det_input": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "cs_det_decode": (ci, [vp, ci, ci, pi, ci, pvp, ci, ci, cf, cf, cf, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "cs_profile_begin": (ci, [vp]),
    "cs_profile_end": (ci, [vp, pd, C.POINTER(cl), pd]),
    "cs_profile_exec_flops": (ci, [vp, pd]),
    "cs_op_conv": (ci, [C.POINTER(ConvDesc), vp]),
    "cs_op_pair_ragged": (ci, [vp, ci, ci, ci, ci, ci, vp]),
    "cs_op_t_mask": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "cs_op_t_style": (ci, [vp, vp, vp, ci, vp]),
    "cs_op_t_modulate": (ci, [vp, vp, vp, vp]),
    "cs_op_t_read": (ci, [vp, ci, ci, ci, vp, vp]),
    "cs_op_t_layer": (ci, [vp, ci, ci, pi, vp, vp, vp, vp, vp, vp]),
    "cs_op_resblock3d": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, cf, vp]),
    "cs_op_grid_sample3d": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_chan_stats_partial_floats": (cl, [ci, cl, ci]),
    "cs_op_chan_stats": (ci, [vp, ci, ci, cl, ci, cf, vp, vp, vp]),
    "cs_op_m_stem": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "cs_op_m_dwln": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_m_ln_s2d": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_m_grn": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "cs_op_m_head": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "cs_op_m_pointwise": (ci, [vp, ci, vp, vp, vp, vp, ci, ci, ci, vp]),
    "cs_op_dm_compress": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_dm_sparse": (ci, [vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp]),
    "cs_op_dm_softmax_warp": (ci, [vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_occ_finish": (ci, [vp, ci, cf, vp, ci, ci, ci, vp]),
    "cs_op_dm_read": (ci, [vp, ci, ci, vp, vp]),
    "cs_op_g_read": (ci, [vp, ci, ci, vp, vp]),
    "cs_op_g_fill": (ci, [vp, ci, vp]),
    "cs_op_g_stop": (ci, [vp, ci]),
    "cs_op_v_read": (ci, [vp, ci, ci, vp, vp]),
    "cs_op_v_fill": (ci, [vp, ci, vp]),
    "cs_op_v_stop": (ci, [vp, ci]),
    "cs_op_conv_first": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "cs_op_norm_act": (ci, [vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, ci, ci, cf, ci, cl, ci, vp]),
    "cs_op_split16": (ci, [vp, vp, cl, vp]),
    "cs_op_id_conv": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp, ci, vp]),
    "cs_op_id_maxpool": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_id_se_tail": (ci, [vp, cl, cl, cl, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "cs_op_id_embed": (ci, [vp, vp, vp, vp, vp, vp, ci, vp]),
    "cs_op_identity_read": (ci, [vp, ci, ci, vp, vp]),
    "cs_op_parser_input": (ci, [vp, vp, ci, ci, ci, vp]),
    "cs_op_parser_gemm": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, ci, ci, vp]),
    "cs_op_parser_layernorm": (ci, [vp, vp, vp, cf, cl, ci, vp, vp, vp]),
    "cs_op_parser_attention": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "cs_op_parser_dwgelu": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_parser_upadd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "cs_op_parser_read": (ci, [vp, ci, ci, vp, vp]),
}
# The landmark runner's entry points: a table of their own beside ABI, as their header stands beside canonswap_hip.h (the reason is stated there).
ABI_LANDMARKS = {
    "cs_lmk_abi_version": (ci, []),
    "cs_lmk_input": (ci, [vp, ci, ci, vp, ci, ci, pi, vp, ci, LmkLayout, ci, cf, cf, ci, ci, vp, vp, vp, vp, vp]),
    "cs_lmk_decode": (ci, [vp, ci, vp, ci, vp, ci, vp, vp, vp]),
}
# The 4:2:0 conversions, the third table: include/canonswap_yuv.h.
ABI_YUV = {
    "cs_yuv_abi_version": (ci, []),
    "cs_yuv_to_rgb": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp]),
    "cs_rgb_to_yuv": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
}
# The crop and the paste-back from device landmarks and matrices, the fourth table: include/canonswap_device_crop.h (cs_lmk_layout by pointer).
ABI_DEVICE_CROP = {
    "cs_dcrop_abi_version": (ci, []),
    "cs_crop_lmk": (ci, [vp, ci, ci, vp, ci, ci, pi, vp, ci, C.POINTER(LmkLayout), ci, cf, cf, ci, ci, vp, vp, vp, vp, vp, vp]),
    "cs_paste_back_faces_dev": (ci, [vp, ci, ci, vp, vp, ci, ci, pi, vp, vp, vp, vp, ci, ci, vp]),
}


class Header(NamedTuple):
    """One header under include/ as the package binds it; tests/test_abi_cpu.py compares it with the header and the header's recorded text."""
    file: str
    table: dict             # entry point -> (restype, argtypes), in the header's order
    version_define: str
    version: int
    version_call: str       # returns `version`: a value, not a status
    structs: dict           # C name -> ctypes class
    constants: dict         # the header's other #defines: C name -> value
    ab_may_lack: bool       # an A/B library of an older tree (CANONSWAP_LIB, tools/cmp_libs.py) may lack the whole header


def _header(file, table, version_define, version, structs, constants, ab_may_lack):
    (version_call,) = (name for name, sig in table.items() if sig == (C.c_int, []))          # the table's one `int f(void)`
    return Header(file, table, version_define, version, version_call, structs, constants, ab_may_lack)


# A further header is a further record: everything below follows from these.
HEADERS = (
    _header("canonswap_hip.h", ABI, "CS_ABI_VERSION", ABI_VERSION, {"cs_conv_desc": ConvDesc},
            {"CS_MAX_IDENTITY_SLOTS": MAX_IDENTITY_SLOTS, "CS_DET_MAX_CAND": DET_MAX_CAND, "CS_DET_MAX_FACES": DET_MAX_FACES}, False),
    _header("canonswap_landmarks.h", ABI_LANDMARKS, "CS_LMK_ABI_VERSION", 1, {"cs_lmk_layout": LmkLayout}, {}, True),
    _header("canonswap_yuv.h", ABI_YUV, "CS_YUV_ABI_VERSION", 1, {}, {}, True),
)
# Why a second tuple: tests/test_abi_cpu.py states HEADERS as exactly the three records above and hands bind() a fake library that has only their
# names, so a header added since stands here and is bound by load() (bind_header, the body bind() applies to HEADERS: the same version check, the
# same A/B rule).  Everything else - call(), STATUS, TAKES_STREAM, the pointer slots - is formed over both tuples and does not tell them apart.
# Merging the tuples is for a change that may edit that test.
HEADERS_BESIDE = (
    _header("canonswap_device_crop.h", ABI_DEVICE_CROP, "CS_DCROP_ABI_VERSION", 1, {}, {}, True),
)
_ALL_HEADERS = HEADERS + HEADERS_BESIDE
_TABLES = {name: sig for h in _ALL_HEADERS for name, sig in h.table.items()}
if len(_TABLES) != sum(len(h.table) for h in _ALL_HEADERS):
    raise ImportError("canonswap_amd/_lib.py: an entry point stands in two headers' tables")
_VERSION_CALLS = frozenset(h.version_call for h in _ALL_HEADERS)
STATUS = frozenset(name for name, (restype, _) in _TABLES.items() if restype is ci) - _VERSION_CALLS      # 0, or the text is in cs_last_error()
# The headers' stream parameters are all the last one, `void* stream`; every entry has one but the version calls and these (tests/test_abi_cpu.py).
TAKES_STREAM = frozenset(_TABLES) - _VERSION_CALLS - {
    "cs_create", "cs_destroy", "cs_last_error", "cs_upload", "cs_finalize_weights", "cs_set_latency_mode", "cs_profile_begin", "cs_profile_end",
    "cs_profile_exec_flops", "cs_op_chan_stats_partial_floats", "cs_op_g_stop", "cs_op_v_stop"}
# The engine's device memory that more than one stream can reach, by group, and the entry points that read or write it.  Engine._call orders two
# calls of one group that come on different streams; the C side orders nothing.  An entry point without a row writes only what the caller passes
# and may run beside anything.  One case stays outside: on a latency-mode engine M's small convs go split-K on sk_buf, which is G's; the chains'
# prefetch refuses such an engine (chain._StagedChain._stage_ahead), so M never runs beside the generator there.
_SCRATCH_GROUPS = {
    "M": ("cs_motion_extract",),                                                       # m_x, m_y, m_h, m_h32, m_sumsq, m_scale
    "SE": ("cs_soft_erosion", "cs_soft_erosion_frames"),                               # se_a, se_b, se_part
    "P": ("cs_parser", "cs_op_parser_read"),                                           # psr
    "A": ("cs_identity", "cs_identity_u8", "cs_op_identity_read"),                     # idn
    "G": ("cs_set_identity", "cs_extract_feature_3d", "cs_warp", "cs_warp_out", "cs_swap", "cs_swap_ids", "cs_refine", "cs_warp_forward",
          "cs_spade_decode", "cs_swap_frames", "cs_swap_frames_ids", "cs_animate_frames", "cs_op_t_layer", "cs_op_t_read", "cs_op_m_pointwise",
          "cs_op_dm_read", "cs_op_g_read", "cs_op_g_fill", "cs_op_v_read", "cs_op_v_fill"),      # vs, va, vsp, dm_*, g_*, seg16, w_t3, tmask, style,
}                                                                                      # the statistics pool, sk_buf, slot_dev, img_a/b
SCRATCH = {name: group for group, names in _SCRATCH_GROUPS.items() for name in names}      # entry point -> its group
_PTR_SLOTS = {name: tuple(t in (vp, C.c_char_p) or issubclass(t, C._Pointer) for t in argtypes) for name, (_, argtypes) in _TABLES.items()}      # or a number
del vp, ci, cf, cl, cd, pi, pd, pvp
ABI_SYMBOLS = list(ABI)
# tests only; an A/B build of an older tree - CANONSWAP_LIB, tools/cmp_libs.py - has none of these: bind() binds them where they exist
ABI_OPTIONAL = ("cs_op_g_read", "cs_op_g_fill", "cs_op_g_stop", "cs_op_v_read", "cs_op_v_fill", "cs_op_v_stop", "cs_op_conv_first", "cs_op_norm_act",
                "cs_op_split16")
_lib = None


def bind_header(lib, h, ab=False):
    """One record on `lib`: its version checked, its entry points given their restype and argtypes.  A missing entry point raises AttributeError,
    but for the ABI_OPTIONAL ones and, with `ab`, for a whole header that an A/B library may lack: it is skipped where its version call is
    missing, and a call of one of its names raises AttributeError then."""
    if ab and h.ab_may_lack and not hasattr(lib, h.version_call):
        return
    speaks = getattr(lib, h.version_call)()          # (ctypes' default restype is the int it returns)
    if speaks != h.version:
        what, binds = ((f"C-ABI version {speaks}", f"{h.version} (include/{h.file}: {h.version_define})") if h is HEADERS[0] else
                       (f"version {speaks} of include/{h.file}", h.version))
        raise RuntimeError(f"{LIB_PATH} speaks {what}, this package binds version {binds}: rebuild with __graft_entry__.build()")
    for name, (restype, argtypes) in h.table.items():
        if name in ABI_OPTIONAL and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes


def bind(lib, ab=False):
    """bind_header for every record of HEADERS on `lib` (a CDLL, or anything with the entry points as attributes); load() goes on with
    HEADERS_BESIDE (bind_beside)."""
    for h in HEADERS:
        bind_header(lib, h, ab)
    return lib


def bind_beside(lib, ab=False):
    """The records of HEADERS_BESIDE on a library bind() has seen: the load-time binding of the headers added beside the recorded three."""
    for h in HEADERS_BESIDE:
        bind_header(lib, h, ab)
    return lib


def load():
    """Load the shared library; raises RuntimeError if it is missing (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP engine has not been built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(needs hipcc); canonswap_amd has no CPU fallback.")
        # The process must hold ONE HIP runtime.  This package's callers pass torch tensors and torch's stream, and torch carries its own
        # libamdhip64 / libhsa-runtime64: imported first, its copies satisfy this library's NEEDED entries too.  Loaded the other way round (this
        # library first - `python __graft_entry__.py smoke`, whose build() checks the ABI before anything imports torch) the system runtime and
        # torch's both initialise and cs_create sees 0 devices.  Hence the import of torch at the top of this module.
        ab = bool(os.environ.get("CANONSWAP_LIB"))                                       # the in-tree library must carry every header
        _lib = bind_beside(bind(C.CDLL(LIB_PATH), ab), ab)
    return _lib


_test_lib = None


def load_test_lib():
    global _test_lib
    if _test_lib is None:
        if not os.path.exists(TEST_LIB_PATH):
            raise RuntimeError(f"{TEST_LIB_PATH} is missing: run __graft_entry__.build()")
        lib = C.CDLL(TEST_LIB_PATH)
        lib.cs_test_last_error.restype = C.c_char_p
        lib.cs_test_conv_igemm.argtypes = [C.POINTER(ConvDesc), C.c_void_p]
        _test_lib = lib
    return _test_lib


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {load().cs_last_error().decode(errors='replace')}")


def call(name, *args, what=None, device=None):
    """The one way into the library: entry point `name` of any of HEADERS and HEADERS_BESIDE with exactly its arguments, checked before the library is touched.  A torch tensor
    stands for its address: in a pointer slot only, and only from a GPU (device=: from that one); None is NULL; the rest goes to ctypes as it is
    (contiguity and dtype are the caller's).  A nonzero status raises RuntimeError("<what or name> failed: <cs_last_error>"); values are returned."""
    argtypes = _TABLES[name][1]
    if len(args) != len(argtypes):
        raise TypeError(f"{name} takes {len(argtypes)} arguments, {len(args)} given")
    args = list(args)
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            if not _PTR_SLOTS[name][i]:
                raise TypeError(f"{name}: argument {i} is a tensor where the entry point takes a number")
            if not a.is_cuda or (device is not None and a.device != device):
                raise TypeError(f"{name}: argument {i} is a tensor on {a.device}, not on {device or 'a GPU'}: its address means nothing to the kernels")
            args[i] = C.c_void_p(a.data_ptr())
    r = getattr(load(), name)(*args)
    if r != 0 and name in STATUS:
        check(r, what or name)
    return r
