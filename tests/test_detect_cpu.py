"""The face detector's input and decode (cs_det_input, cs_det_decode; canonswap_amd/detect.py, align.py) without a GPU: the yardstick of
test_gpu_detect.py (tests/detect_ref.py) against the reference's own detect() (tests/golden/detect.npz), against the x2 and x1/2 restatements
the repository already holds, and against an independent derivation of the alignment; the host geometry; the C ABI of the two entry points;
detect.py's validation (src/utils/dependencies/insightface/model_zoo/scrfd.py:154-303, insightface_func/utils/face_align_ffhqandnewarc.py:55-78)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import concat_ref
import detect_ref as DR
import parser_input_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_comments_cite_the_reference_and_the_caps_and_the_kernel_file_are_in_place():
    """(The entry points' types, arity and export: test_abi_cpu.py.)"""
    from canonswap_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    engine = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    for name in ("cs_det_input", "cs_det_decode"):
        assert name in engine.split("extern \"C\" int cs_abi_version")[0]                # the entry-point list at the top
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int cs_det_input", header, flags=re.S)[0]
    assert "scrfd.py:224-235" in comment and "scrfd.py:154" in comment and "PARITY UNPINNED" in comment and ">> 16" in comment
    assert "can_swap_pipeline_e2e.py:93" in comment and "can_swap_pipeline_v2i.py:230" in comment and "no engine scratch" in comment
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*#define CS_DET_MAX_CAND", header, flags=re.S)[0]
    assert "scrfd.py:160-218" in comment and "scrfd.py:239-273" in comment and ":275-303" in comment and "STABLE argsort reversed" in comment
    assert int(re.search(r"#define\s+CS_DET_MAX_CAND\s+(\d+)", header).group(1)) == _lib.DET_MAX_CAND >= 1024
    assert int(re.search(r"#define\s+CS_DET_MAX_FACES\s+(\d+)", header).group(1)) == _lib.DET_MAX_FACES == 256
    kernel = open(os.path.join(ROOT, "canonswap_amd", "csrc", "detect.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "fmaf" not in kernel.split("#include")[1]      # how contraction is prevented is said and done
    assert os.path.join(_build.CSRC, "detect.hip") in _build.SOURCES


def test_python_names_import():
    from canonswap_amd import align, detect
    from canonswap_amd.can_swap_e2e import can_swapper
    for name in ("det_geometry", "det_lut", "det_input", "det_decode", "FaceDetector"):
        assert hasattr(detect, name)
    for name in ("det_input", "det_decode", "getid_faces"):
        assert hasattr(can_swapper, name)
    assert hasattr(align, "estimate_norm") and detect.SWAP_RB is True


# ------------------------------------------------------------------------------------------------ the restatement against the reference's code
def test_fixture_holds_arrays_only_and_stays_small():
    assert os.path.getsize(DR.GOLDEN) < 50_000
    with np.load(DR.GOLDEN, allow_pickle=False) as z:
        assert all(z[k].dtype == np.float32 for k in z.files)
        want = {f"{n}/det" for n in DR.GOLDEN_SCENES} | {f"{n}/kps" for n, s in DR.GOLDEN_SCENES.items() if s[5]}
        assert set(z.files) == want


@pytest.mark.parametrize("name", sorted(DR.GOLDEN_SCENES))
def test_decode_faces_equals_the_references_detect(name):
    fx, c = DR.fixture(), DR.golden_case(name)
    assert c["det"].dtype == np.float32 and c["det"].shape == fx[f"{name}/det"].shape
    assert np.array_equal(_bits(c["det"]), _bits(fx[f"{name}/det"]))
    if c["kps"] is None:
        assert f"{name}/kps" not in fx
    else:
        assert c["kps"].shape == (len(c["det"]), 5, 2) and np.array_equal(_bits(c["kps"]), _bits(fx[f"{name}/kps"]))


def test_golden_scenes_cover_what_they_should():
    n = {k: len(DR.golden_case(k)["det"]) for k in DR.GOLDEN_SCENES}
    assert n["empty"] == 0 and n["two"] == 2 and n["overlap"] == 1 and n["chain"] == 2 and n["pick0"] == 3 and n["pick1"] == 1 and n["pick2"] == 2
    assert n["five"] == 2 and n["five1"] == 1 and DR.golden_case("nokps")["kps"] is None
    for k in ("two", "chain", "five"):                                                   # clusters: NMS had candidates to thin
        c = DR.golden_case(k)
        nl = DR.levels_of(len(c["outs"]))[0]
        assert sum(int((s >= np.float32(0.5)).sum()) for s in c["outs"][:nl]) >= 5 * n[k]


# ------------------------------------------------------------------------------------------------ order and suppression are seen
def test_chain_scene_keeps_the_first_and_the_third():
    """A > B > C with A-B and B-C above the threshold and A-C below: greedy NMS in score order keeps A and C; any other order keeps B."""
    outs = DR.scene_64(DR.CHAIN, 11, single=True)
    scale = DR.det_scale_64()
    raw, _ = DR.decode_faces(outs, (64, 64), scale, DR.FRAME_64, nms_thresh=1.0)          # nothing suppressed: the three boxes by score
    assert raw.shape == (3, 5) and (np.diff(raw[:, 4]) < 0).all()

    def iou(a, b):
        w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
        h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
        return w * h / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - w * h)
    assert iou(raw[0], raw[1]) > 0.4 and iou(raw[1], raw[2]) > 0.4 and iou(raw[0], raw[2]) < 0.4
    det, _ = DR.decode_faces(outs, (64, 64), scale, DR.FRAME_64)
    assert np.array_equal(det, raw[[0, 2]])
    flipped = [o.copy() for o in outs]                                                   # B the strongest: it alone remains
    for s in flipped[:3]:
        s[np.isclose(s, raw[1, 4])] = 0.99
    only_b, _ = DR.decode_faces(flipped, (64, 64), scale, DR.FRAME_64)
    assert only_b.shape == (1, 5) and np.array_equal(only_b[0, :4], raw[1, :4])


def test_highest_score_largest_area_and_most_central_are_three_answers():
    outs = DR.scene_64(DR.PICK3, 6)
    scale = DR.det_scale_64()
    every, _ = DR.decode_faces(outs, (64, 64), scale, DR.FRAME_64)
    assert every.shape == (3, 5)
    best = every[int(np.argmax(every[:, 4]))]                                            # face_detect_crop_single.py:71-80
    by_area, _ = DR.decode_faces(outs, (64, 64), scale, DR.FRAME_64, max_num=1, metric="max")
    central, _ = DR.decode_faces(outs, (64, 64), scale, DR.FRAME_64, max_num=1)
    rows = [tuple(best), tuple(by_area[0]), tuple(central[0])]
    assert len(set(rows)) == 3 and all(r in [tuple(e) for e in every] for r in rows)
    area = (every[:, 2] - every[:, 0]) * (every[:, 3] - every[:, 1])
    assert tuple(every[int(np.argmax(area))]) == rows[1]
    mid = np.stack([(every[:, 0] + every[:, 2]) / 2 - 50, (every[:, 1] + every[:, 3]) / 2 - 50])
    assert tuple(every[int(np.argmin((mid ** 2).sum(0)))]) == rows[2]


def test_tie_contract_of_the_restatement():
    """Two disjoint boxes of equal score: :241's order lists the later first, nms' own sort reverses it once more - the result is in anchor order;
    two equal max_num values: the later survivor first."""
    outs = [o.copy() for o in DR.scene_64(DR.TWO, 12, single=True)]
    top = sorted(float(s.max()) for s in outs[:3])[-1]
    for s in outs[:3]:
        s[s >= np.float32(0.5)] = np.float32(top)
    det, _ = DR.decode_faces(outs, (64, 64), DR.det_scale_64(), DR.FRAME_64)
    assert det.shape == (2, 5) and det[0, 4] == det[1, 4] and det[0, 0] < det[1, 0]       # TWO's first face is the earlier anchor
    assert list(DR.stable_desc(np.array([1.0, 2.0, 2.0, 0.5], np.float32))) == [2, 1, 0, 3]


# ------------------------------------------------------------------------------------------------ geometry, table, resize
def test_det_geometry_reproduces_the_references_truncations():
    from canonswap_amd import detect
    cases = {(1080, 1920, (640, 640)): (360, 640), (1920, 1080, (640, 640)): (640, 360), (512, 512, (640, 640)): (640, 640),
             (45, 80, (64, 64)): (36, 64), (80, 45, (64, 64)): (64, 36), (50, 70, (96, 64)): (64, 89), (20, 30, (64, 64)): (42, 64),
             (720, 1279, (640, 640)): (360, 640), (1279, 720, (640, 640)): (640, 360), (100, 333, (320, 256)): (96, 320)}
    for (Ho, Wo, size), (nh, nw) in cases.items():
        got = detect.det_geometry(Ho, Wo, size)
        assert got[:2] == (nh, nw) and got == DR.geometry(Ho, Wo, size), (Ho, Wo, size, got)
        assert got[2] == float(nh) / Ho and isinstance(got[2], float)
        assert nh <= size[1] and nw <= size[0]
    assert detect.det_geometry(720, 1279, (640, 640))[0] == int(640 * (720.0 / 1279))      # truncated, not rounded: 360.28
    assert int(64 / (80.0 / 45)) == 36 and detect.det_geometry(50, 70, (96, 64))[1] == int(64 / (50.0 / 70))
    for bad in ((0, 5, (64, 64)), (5, 5, (64,)), (5, 5, (0, 64)), (5, 5, (64.5, 64))):
        with pytest.raises(ValueError):
            detect.det_geometry(*bad)


def test_table_is_exact_for_the_detectors_constants():
    from canonswap_amd import detect
    lut = detect.det_lut()
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and lut.flags["C_CONTIGUOUS"]
    want = (np.arange(256, dtype=np.float64) - 127.5) / 128.0
    assert np.array_equal(lut.astype(np.float64), np.stack([want] * 3))                  # exact: no rounding anywhere
    assert np.array_equal(_bits(lut), _bits(DR.table()))
    other = detect.det_lut(mean=(104.0, 117.0, 123.0), std=57.0)
    assert np.array_equal(_bits(other), _bits(DR.table((104.0, 117.0, 123.0), 57.0))) and not np.array_equal(other[0], other[2])
    for bad in ({"mean": (1.0, 2.0)}, {"std": 0.0}):
        with pytest.raises(ValueError):
            detect.det_lut(**bad)


def test_resize_agrees_with_the_repositorys_restatements_at_x2_half_and_x1():
    for shape, seed in (((2, 5, 7, 3), 1), ((1, 16, 16, 3), 2), ((1, 1, 1, 3), 3), ((1, 33, 2, 3), 4)):
        x = DR.frames_u8(shape[0], shape[1], shape[2], seed)
        assert np.array_equal(DR.resize_linear_cv(x, 2 * shape[1], 2 * shape[2]), concat_ref.resize_x2_cv(x))
        assert np.array_equal(DR.resize_linear_cv(x, shape[1], shape[2]), x)
        big = DR.frames_u8(shape[0], 2 * shape[1], 2 * shape[2], seed)
        assert np.array_equal(DR.resize_linear_cv(big, shape[1], shape[2]), PR.halve_u8(big))
    sat = np.where(DR.frames_u8(1, 9, 11, 5) > 127, 255, 0).astype(np.uint8)
    assert np.array_equal(DR.resize_linear_cv(sat, 18, 22), concat_ref.resize_x2_cv(sat))


def test_resize_general_ratio_by_hand_and_against_the_float_formula():
    """A 1 x 4 row to width 3: scale 4/3; d = 0: f = 1/6, d = 1: s = 1, f = .5, d = 2: s = 2, f = 5/6 -> coefficients (1707, 341), (1024, 1024),
    (341, 1707); a single row: both row taps are row 0 under (2048, 0)."""
    row = np.array([[[10], [50], [200], [255]]], np.uint8)
    got = DR.resize_linear_cv(row, 1, 3)[0, :, 0]
    want = []
    for (s, a0, a1) in ((0, 1707, 341), (1, 1024, 1024), (2, 341, 1707)):
        h = a0 * int(row[0, s, 0]) + a1 * int(row[0, s + 1, 0])
        want.append((((2048 * (h >> 4)) >> 16) + 2) >> 2)
    assert list(got) == want
    x = DR.frames_u8(1, 45, 80, 6)
    for dh, dw in ((36, 64), (64, 113), (45, 64), (7, 80)):
        got = DR.resize_linear_cv(x, dh, dw).astype(np.float64)
        assert got.shape == (1, dh, dw, 3)
        sx = (np.arange(dw) + 0.5) * (80 / dw) - 0.5
        sy = (np.arange(dh) + 0.5) * (45 / dh) - 0.5
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = (sx - x0)[None, :, None], (sy - y0)[:, None, None]
        g = lambda yy, xx: x[0][np.clip(yy, 0, 44)][:, np.clip(xx, 0, 79)].astype(np.float64)
        ideal = (g(y0, x0) * (1 - fx) + g(y0, x0 + 1) * fx) * (1 - fy) + (g(y0 + 1, x0) * (1 - fx) + g(y0 + 1, x0 + 1) * fx) * fy
        assert np.abs(got[0] - ideal).max() <= 1.0                                      # the fixed-point path stays within one count of bilinear


def test_letterbox_pads_with_the_tables_zero_and_swaps_channels():
    x = DR.frames_u8(2, 45, 80, 7)
    blob = DR.letterbox_blob(x, (64, 64))
    assert blob.shape == (2, 3, 64, 64) and blob.dtype == np.float32
    assert (blob[:, :, 36:, :] == np.float32(-127.5 / 128)).all() and not (blob[:, :, :36, :] == np.float32(-127.5 / 128)).all()
    plain = DR.letterbox_blob(x, (64, 64), swap_rb=False)
    assert np.array_equal(blob[:, ::-1], plain) and not np.array_equal(blob, plain)
    tall = DR.letterbox_blob(DR.frames_u8(1, 80, 45, 8), (64, 64))
    assert (tall[:, :, :, 36:] == np.float32(-127.5 / 128)).all()
    wide = DR.letterbox_blob(DR.frames_u8(1, 50, 70, 9), (96, 64))                       # det_size is (width, height)
    assert wide.shape == (1, 3, 64, 96) and (wide[:, :, :, 89:] == np.float32(-127.5 / 128)).all()


# ------------------------------------------------------------------------------------------------ alignment
def _similar(points, angle, scale, t):
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    return points @ np.array([[c, s], [-s, c]]) + np.asarray(t)


@pytest.mark.parametrize("size,mode", [(112, "None"), (224, "None"), (512, "ffhq"), (112, "ffhq")])
def test_estimate_norm_agrees_with_the_independent_derivation(size, mode):
    from canonswap_amd import align
    T = align.templates(size, mode)
    assert T.dtype == np.float64 and T.shape == ((1, 5, 2) if mode == "ffhq" else (5, 5, 2))
    r = np.random.Generator(np.random.PCG64([5300, size]))
    for k in range(6):
        kps = _similar(T[k % len(T)], r.uniform(-0.6, 0.6), r.uniform(0.5, 3.0), r.uniform(-200, 800, 2)) + r.normal(0, 1.5, (5, 2))
        M, i = align.estimate_norm(kps.astype(np.float32), size, mode)
        Mr, ir = DR.estimate_norm_ref(kps.astype(np.float32), T)
        assert M.dtype == np.float64 and M.shape == (2, 3) and i == ir
        assert np.abs(M - Mr).max() <= 1e-9 * np.abs(Mr).max()


def test_estimate_norm_picks_the_generating_template_and_recovers_the_similarity():
    from canonswap_amd import align
    T = align.templates(112, "None")
    assert np.array_equal(T.astype(np.float32), align.SRC_MAP)                           # at 112 the templates are the data itself
    assert np.array_equal(align.templates(224, "None"), (align.SRC_MAP * 224 / 112).astype(np.float64))
    assert np.allclose(align.templates(112, "ffhq"), align.FFHQ_SRC * 112 / 512, rtol=0, atol=0)
    for i in range(5):
        angle, scale, t = 0.3 - 0.1 * i, 1.7 + 0.2 * i, (300.0 + 10 * i, 150.0 - 7 * i)
        kps = _similar(T[i], angle, scale, t)                                            # template -> frame; estimate_norm finds frame -> template
        M, idx = align.estimate_norm(kps, 112, "None")
        assert idx == i
        back = kps @ M[:, :2].T + M[:, 2]
        assert np.abs(back - T[i]).max() < 1e-9
        assert abs(np.hypot(M[0, 0], M[1, 0]) - 1 / scale) < 1e-12 and abs(np.arctan2(M[1, 0], M[0, 0]) + angle) < 1e-12      # the inverse turns back
    Ms, idxs = align.norm_matrices(np.stack([_similar(T[2], 0.1, 2.0, (50, 60)), _similar(T[4], -0.2, 1.5, (5, 6))]), 112)
    assert Ms.shape == (2, 2, 3) and list(idxs) == [2, 4]
    for bad in (np.zeros((4, 2)), np.zeros((5, 3))):
        with pytest.raises(ValueError):
            align.estimate_norm(bad)


# ------------------------------------------------------------------------------------------------ detect.py's validation (no device needed)
def test_det_decode_validates_shapes_dtypes_and_devices():
    from canonswap_amd import detect
    e = types.SimpleNamespace(device=torch.device("cuda:0"))
    outs = [torch.from_numpy(o) for o in DR.scene_64(DR.TWO, 1)]
    args = ((64, 64), 0.64, (100, 100))
    with pytest.raises(ValueError, match="lives on cpu"):
        detect.det_decode(e, outs, *args)
    cpu = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="8 network outputs"):
        detect.det_decode(cpu, outs[:8], *args)
    with pytest.raises(ValueError, match="float64"):
        detect.det_decode(cpu, [outs[0].double()] + outs[1:], *args)
    with pytest.raises(ValueError, match=r"output 4 has shape .*expected \(F, 32, 4\)"):
        detect.det_decode(cpu, outs[:4] + [outs[4][:-1]] + outs[5:], *args)
    with pytest.raises(ValueError, match="expected"):
        detect.det_decode(cpu, outs, (128, 64), 0.64, (100, 100))                       # another det_size: other anchor counts
    with pytest.raises(ValueError, match="output 1"):
        detect.det_decode(cpu, [outs[0][None].repeat(2, 1, 1)] + outs[1:], *args)      # frames disagree
    with pytest.raises(ValueError, match="not a torch.Tensor"):
        detect.det_decode(cpu, [o.numpy() for o in outs], *args)
    with pytest.raises(ValueError, match="metric"):
        detect.det_decode(cpu, outs, *args, metric="area")
    for kw in ({"max_faces": 0}, {"max_faces": 257}, {"max_num": 33}, {"max_num": -1}):
        with pytest.raises(ValueError, match="max_faces"):
            detect.det_decode(cpu, outs, *args, **kw)
    with pytest.raises(ValueError, match="uint8 frames"):
        detect.det_input(cpu, np.zeros((2, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="uint8 frames"):
        detect.det_input(cpu, np.zeros((2, 8, 8, 4), np.uint8))
    with pytest.raises(ValueError, match="det_size"):
        detect.det_input(cpu, np.zeros((2, 8, 8, 3), np.uint8), det_size=(64, 20000))
    with pytest.raises(ValueError, match="resizes to"):
        detect.det_input(cpu, np.zeros((1, 1, 200, 3), np.uint8), det_size=(64, 64))
    with pytest.raises(ValueError, match="callable"):
        detect.FaceDetector(cpu, None)
