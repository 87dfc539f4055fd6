"""Golden vectors for the cropper's geometry (src/utils/crop.py:98-300, 381-455) produced by the reference's OWN functions.

crop.py cannot be imported (its first statements import cv2, which is not installed), so the function definitions are cut out of the
reference source with `ast` at generation time and executed as they are, with numpy and `math` in their namespace - the reference's
code runs, nothing of it is copied into this repository.  crop_image's one image call, _transform_img (cv2.warpAffine), is replaced by a
stub that returns None: the fixture holds the geometry only.  Only the resulting arrays are committed (tests/golden/crop_geometry.npz).

    python tools/make_golden_crop.py <reference checkout>        # build container only; or CANONSWAP_REFERENCE=<reference checkout>

Per landmark set `k` (names in `sets`) the file holds `<k>_lmk` and, per configuration `c` (names in `configs`, values in `<c>_cfg` =
dsize, scale, vy_ratio, flag_do_rot), the reference's `<k>_<c>_M_INV` (2x3), `_M_o2c`, `_M_c2o` (3x3) and `_pt_crop`; and
`<k>_pt2_nolip`, parse_pt2_from_pt_x(lmk, use_lip=False), which no caller of crop_image reaches.
"""
import ast
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WANTED = ("parse_pt2_from_pt101", "parse_pt2_from_pt106", "parse_pt2_from_pt203", "parse_pt2_from_pt68", "parse_pt2_from_pt5",
          "parse_pt2_from_pt9", "parse_pt2_from_pt_x", "parse_rect_from_landmark", "_estimate_similar_transform_from_pts", "_transform_pts",
          "crop_image")
# (dsize, scale, vy_ratio): CropConfig (src/config/crop_config.py:21-26) and crop_image's defaults, which the landmark runner crops with
# (human_landmark_runner.py:62)
CONFIGS = {"cropper_rot": (512, 2.3, -0.125, True), "cropper_norot": (512, 2.3, -0.125, False),
           "runner_rot": (224, 1.5, -0.1, True), "runner_norot": (224, 1.5, -0.1, False)}


def reference_functions(src):
    tree = ast.parse(open(src).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    if sorted(n.name for n in nodes) != sorted(WANTED):
        raise RuntimeError(f"{src}: expected the functions {WANTED}")
    ns = {"np": np, "DTYPE": np.float32, "sin": math.sin, "cos": math.cos, "acos": math.acos, "degrees": math.degrees,
          "_transform_img": lambda img, M, dsize: None}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), src, "exec"), ns)
    return ns


def face_landmarks(n, seed, dtype=np.float32, degenerate=False):
    """n points at face-like scale and position in a 1920x1080 frame: a cloud inside the face's ellipse, the points the layout reads as eyes
    and lips put where eyes and lips are, the whole rolled by up to half a radian.  These are inputs only; which indices are eyes and lips
    is the layouts' own knowledge (canonswap_amd.crop.EYE_LIP_POINTS for 101 / 106 / 203 points)."""
    from canonswap_amd.crop import EYE_LIP_POINTS
    r = np.random.Generator(np.random.PCG64(seed))
    w = r.uniform(140, 320)
    centre = np.array([r.uniform(500, 1400), r.uniform(300, 750)])
    roll = r.uniform(-0.5, 0.5)
    rad, ang = np.sqrt(r.uniform(0, 1, n)), r.uniform(0, 2 * np.pi, n)
    p = np.stack([0.5 * w * rad * np.cos(ang), 0.65 * w * rad * np.sin(ang)], axis=1)
    layout = {68: ((36, 39), (42, 45), (48, 54)), 5: ((0,), (1,), (3, 4)), 9: ((2, 3), (0, 1), (5, 6))}
    left, right, lips = (EYE_LIP_POINTS[n] if n in EYE_LIP_POINTS else EYE_LIP_POINTS[101] if n > 101 else layout[n])
    for idx, (x, y) in ((left, (-0.22, -0.2)), (right, (0.22, -0.2)), (lips[:1], (-0.17, 0.35)), (lips[1:], (0.17, 0.35))):
        for i in idx:
            p[i] = np.array([x, y]) * w + r.uniform(-0.03, 0.03, 2) * w
    if degenerate:                                          # the lips' centre falls on the eyes' centre: the `l <= 1e-3` branch
        assert n == 5
        p[3], p[4] = p[0], p[1]
    c, s = np.cos(roll), np.sin(roll)
    return (p @ np.array([[c, s], [-s, c]]) + centre).astype(dtype)


SETS = {"pt203": (203, 1), "pt106": (106, 2), "pt101": (101, 3), "pt68": (68, 4), "pt9": (9, 5), "pt5": (5, 6), "pt120": (120, 7),
        "pt106_f64": (106, 8), "pt5_degenerate": (5, 9)}


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CANONSWAP_REFERENCE")
    if not src:
        raise SystemExit(__doc__)
    ref = reference_functions(os.path.join(src, "src", "utils", "crop.py"))
    out = {"sets": np.array(sorted(SETS)), "configs": np.array(sorted(CONFIGS))}
    for c, cfg in CONFIGS.items():
        out[f"{c}_cfg"] = np.array(cfg, dtype=np.float64)
    for k, (n, seed) in SETS.items():
        lmk = face_landmarks(n, seed, np.float64 if k.endswith("f64") else np.float32, degenerate=k.endswith("degenerate"))
        out[f"{k}_lmk"] = lmk
        out[f"{k}_pt2_nolip"] = ref["parse_pt2_from_pt_x"](lmk.copy(), use_lip=False)
        for c, (dsize, scale, vy, rot) in CONFIGS.items():
            M_INV, _ = ref["_estimate_similar_transform_from_pts"](lmk.copy(), dsize=dsize, scale=scale, vy_ratio=vy, flag_do_rot=rot)
            d = ref["crop_image"](None, lmk.copy(), dsize=dsize, scale=scale, vy_ratio=vy, flag_do_rot=rot)
            assert np.array_equal(M_INV, d["M_o2c"][:2])
            out[f"{k}_{c}_M_INV"] = M_INV
            out[f"{k}_{c}_M_o2c"] = d["M_o2c"]
            out[f"{k}_{c}_M_c2o"] = d["M_c2o"]
            out[f"{k}_{c}_pt_crop"] = d["pt_crop"]
    path = os.path.join(ROOT, "tests", "golden", "crop_geometry.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(SETS), "landmark sets x", len(CONFIGS), "configurations")


if __name__ == "__main__":
    main()
