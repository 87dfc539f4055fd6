"""The cropper's geometry on the host (canonswap_amd/crop.py) against the reference's own vectors, and the C ABI of cs_crop_frames,
checked without a GPU.

tests/golden/crop_geometry.npz was written by tools/make_golden_crop.py, which executes the reference's functions (src/utils/crop.py:98-300,
381-455) on seeded face-like landmark sets: 203, 106, 101, 68, 9 and 5 points, 120 points (more than 101: the first 101), float64 landmarks,
one set whose eye-lip axis is degenerate; each with the cropper's parameters (512, 2.3, -0.125) and the landmark runner's (224, 1.5, -0.1),
flag_do_rot on and off.

Bounds (from the number formats, not from what the code gives): the restatement makes the same numpy / `math` calls in the same order and
dtype, so M_o2c and pt_crop may differ from the reference's by the last bit of a libm result at most: one ulp (np.spacing) of the reference's
value per entry.  M_c2o comes out of LAPACK's inverse, whose last bits depend on the BLAS build: 8 float32 ulps of the matrix's largest entry.
On the machine that wrote the fixture all three were bit-equal for every case; the test prints whether they are where it runs."""
import os
import re

import numpy as np
import pytest

from canonswap_amd import crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "crop_geometry.npz"))
CASES = [(str(k), str(c)) for k in GOLD["sets"] for c in GOLD["configs"]]


def _cfg(c):
    dsize, scale, vy, rot = GOLD[f"{c}_cfg"]
    return dict(dsize=int(dsize), scale=float(scale), vy_ratio=float(vy), flag_do_rot=bool(rot))


def test_fixture_covers_what_it_should():
    n = {GOLD[f"{k}_lmk"].shape[0] for k in GOLD["sets"]}
    assert {203, 106, 101, 68, 9, 5} <= n and any(m > 101 and m not in (106, 203) for m in n)
    cfgs = {tuple(GOLD[f"{c}_cfg"]) for c in GOLD["configs"]}
    assert cfgs == {(512, 2.3, -0.125, 1), (512, 2.3, -0.125, 0), (224, 1.5, -0.1, 1), (224, 1.5, -0.1, 0)}
    deg = GOLD["pt5_degenerate_lmk"]
    assert np.linalg.norm((deg[3] + deg[4]) / 2 - (deg[0] + deg[1]) / 2) <= 1e-3          # the `l <= 1e-3` branch
    assert len(CASES) == 36


@pytest.mark.parametrize("k,c", CASES)
def test_matrices_and_landmarks_equal_the_references(k, c):
    lmk = GOLD[f"{k}_lmk"]
    M_o2c, M_c2o, lmk_crop = crop.crop_matrices(lmk, **_cfg(c))
    assert M_o2c.shape == (1, 3, 3) and M_o2c.dtype == np.float32
    assert M_c2o.shape == (1, 3, 3) and M_c2o.dtype == np.float32
    assert lmk_crop.shape == (1,) + lmk.shape
    ref_o2c, ref_c2o, ref_pts = GOLD[f"{k}_{c}_M_o2c"], GOLD[f"{k}_{c}_M_c2o"], GOLD[f"{k}_{c}_pt_crop"]
    assert ref_o2c.dtype == np.float32 and ref_c2o.dtype == np.float32 and lmk_crop.dtype == ref_pts.dtype
    assert np.array_equal(GOLD[f"{k}_{c}_M_INV"], ref_o2c[:2])
    print(f"{k} {c}: bit-equal M_o2c {np.array_equal(M_o2c[0], ref_o2c)}, M_c2o {np.array_equal(M_c2o[0], ref_c2o)}, "
          f"pt_crop {np.array_equal(lmk_crop[0], ref_pts)}")
    assert np.all(np.abs(M_o2c[0].astype(np.float64) - ref_o2c) <= np.spacing(np.abs(ref_o2c)))
    assert np.all(np.abs(lmk_crop[0].astype(np.float64) - ref_pts) <= np.spacing(np.abs(ref_pts)))
    assert np.all(np.abs(M_c2o[0].astype(np.float64) - ref_c2o) <= 8 * np.spacing(np.float32(np.abs(ref_c2o).max())))


@pytest.mark.parametrize("k", [str(k) for k in GOLD["sets"]])
def test_two_points_without_the_lips(k):
    got = crop.parse_pt2(GOLD[f"{k}_lmk"].copy(), use_lip=False)
    ref = GOLD[f"{k}_pt2_nolip"]
    assert got.dtype == ref.dtype
    assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref)))


@pytest.mark.parametrize("k,c", CASES)
def test_inverse_property_and_landmark_transform(k, c):
    lmk = GOLD[f"{k}_lmk"]
    M_o2c, M_c2o, lmk_crop = crop.crop_matrices(lmk, **_cfg(c))
    assert np.abs(M_c2o[0].astype(np.float64) @ M_o2c[0].astype(np.float64) - np.eye(3)).max() <= 1e-4
    assert np.array_equal(lmk_crop, crop.transform_pts(lmk[None], M_o2c))
    assert np.array_equal(lmk_crop[0], crop.transform_pts(lmk, M_o2c[0]))
    assert np.array_equal(lmk_crop[0], crop.transform_pts(lmk, M_o2c[0, :2]))
    back = crop.transform_pts(lmk_crop, M_c2o)                                            # and back: a pixel's fraction at 1080p
    assert np.abs(back[0].astype(np.float64) - lmk).max() <= 1e-2


def test_a_batch_is_its_frames_one_by_one():
    lmk = np.stack([GOLD["pt106_lmk"], GOLD["pt106_lmk"] + np.float32(17.5), GOLD["pt106_lmk"][::-1].copy()])
    M_o2c, M_c2o, lmk_crop = crop.crop_matrices(lmk)
    assert M_o2c.shape == (3, 3, 3) and M_c2o.shape == (3, 3, 3) and lmk_crop.shape == lmk.shape
    for b in range(3):
        one = crop.crop_matrices(lmk[b])
        assert np.array_equal(M_o2c[b], one[0][0]) and np.array_equal(M_c2o[b], one[1][0]) and np.array_equal(lmk_crop[b], one[2][0])
    assert np.array_equal(M_o2c[0], GOLD["pt106_cropper_rot_M_o2c"])                     # the defaults are CropConfig's


def test_degenerate_axis_is_the_images_own():
    M_o2c, _, _ = crop.crop_matrices(GOLD["pt5_degenerate_lmk"])
    assert M_o2c[0, 0, 1] == 0 and M_o2c[0, 1, 0] == 0 and M_o2c[0, 0, 0] == M_o2c[0, 1, 1] > 0


def test_no_vx_ratio_parameter():
    import inspect
    assert "vx_ratio" not in inspect.signature(crop.crop_matrices).parameters
    assert "vx_ratio" in crop.__doc__ and "vx_ratio" in crop.crop_matrices.__doc__


@pytest.mark.parametrize("shape", [(106,), (106, 3), (2, 106, 3), (1, 2, 106, 2), (0, 106, 2), (7, 2), (100, 2), (2, 33, 2)])
def test_wrong_landmark_shapes_raise(shape):
    with pytest.raises(ValueError):
        crop.crop_matrices(np.zeros(shape, np.float32))


def test_wrong_arguments_raise():
    lmk = GOLD["pt106_lmk"]
    with pytest.raises(ValueError):
        crop.crop_matrices(lmk.astype(np.int32))
    with pytest.raises(ValueError):
        crop.crop_matrices(lmk, dsize=0)
    with pytest.raises(ValueError):
        crop.crop_matrices(lmk, dsize=224.5)
    M = crop.crop_matrices(lmk)[0]
    for pts, m in ((lmk, M), (lmk[None], M[0]), (lmk[:, :1], M[0]), (lmk, M[0, :1]), (np.stack([lmk, lmk]), M)):
        with pytest.raises(ValueError):
            crop.transform_pts(pts, m)


# ---- the C ABI of the device step (its types, arity and export: test_abi_cpu.py)
def test_header_comment_of_the_entry_point_cites_the_reference():
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    assert re.search(r"crop\.py:429-455.*?cropper\.py:196-209.*?int cs_crop_frames", header, flags=re.S)


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain, FrameChain
    assert callable(tail.crop_frames) and callable(tail.crop_frames_M) and callable(can_swapper.crop_frames)
    assert callable(FrameChain.crop) and callable(AnimateChain.crop)
