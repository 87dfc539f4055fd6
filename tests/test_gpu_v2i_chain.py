"""The device-side frame of the video-to-image pipeline (canonswap_amd/chain.py AnimateChain): the three kernels behind
cs_resize_half_bilinear, cs_motion_keypoints_driven and cs_paste_back_shared against their yardsticks, the chain against the oracle's
composition of CanSwapPipeline.execute of src/can_swap_pipeline_v2i.py (each step below cites its line there), the chain against its own
stages, and the stream rules of prefetch()."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import chain_helpers
from chain_helpers import _affine, _masks, _occupy, _timed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


def _crops(n, seed):
    from canonswap_amd import synth
    smooth = synth.make_smooth_images(n, seed=seed, size=512)                       # (n,3,512,512) in [0,1]
    return np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))


def _small_affine(k, Ho, Wo):
    return _affine(k, Ho, Wo) * np.array([[0.5], [0.5], [1]]) + np.array([[0, 0, 100.], [0, 0, 20.], [0, 0, 0]])


# ------------------------------------------------------------------------------------------------ kernel (a): the half-size resize
def _rows_first(x):
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    return 0.25 * ((a + b) + (c + d))


@pytest.mark.parametrize("shape", [(2, 3, 512, 512), (1, 1, 6, 10)])
def test_resize_half_is_the_rows_first_mean(swapper_m, shape):
    """0.25f * ((a + b) + (c + d)), a b the upper row: element by element the same bits as that expression in torch on the CPU
    (512 x 512 takes the float4 path, 6 x 10 the scalar one)."""
    r = np.random.Generator(np.random.PCG64(101))
    x = torch.from_numpy(r.uniform(0, 1, size=shape).astype(np.float32))
    got = swapper_m.engine.resize_half_bilinear(x.cuda()).cpu()
    assert got.shape == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    assert torch.equal(got, _rows_first(x))


def test_resize_half_vs_interpolate(swapper_m):
    """F.interpolate(bilinear, align_corners=False) on the CPU sums the four quarter-weighted pixels in an order that depends on its thread
    count, so it is no bit-level yardstick.  Each form rounds three partial sums below 4, each rounding <= 2^-23 before the x 1/4: two forms
    differ by <= 6 * 2^-25 = 1.8e-7 on inputs in [0, 1]."""
    r = np.random.Generator(np.random.PCG64(102))
    x = torch.from_numpy(r.uniform(0, 1, size=(2, 3, 512, 512)).astype(np.float32))
    got = swapper_m.engine.resize_half_bilinear(x.cuda()).cpu()
    want = F.interpolate(x, size=(256, 256), mode="bilinear", align_corners=False)
    err = (got - want).abs().max().item()
    print(f"resize_half vs F.interpolate: max |diff| {err:.3e}")
    assert err <= 2e-7


def test_resize_half_refuses_odd_sizes_and_bad_out(swapper_m):
    e = swapper_m.engine
    with pytest.raises(ValueError):
        e.resize_half_bilinear(torch.zeros(1, 3, 7, 8).cuda())
    with pytest.raises(ValueError):
        e.resize_half_bilinear(torch.zeros(1, 3, 8, 8).cuda(), out=torch.zeros(1, 3, 4, 4, dtype=torch.float16).cuda())
    with pytest.raises(ValueError):
        e.resize_half_bilinear(torch.zeros(1, 3, 8, 8).cuda(), out=torch.zeros(1, 3, 4, 4))


# ------------------------------------------------------------------------------------------------ kernel (b): the driven key-points
def _raw_heads(B, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    raw = r.normal(0, 1, size=(B, 328)).astype(np.float32)
    raw[:, :63] *= 0.3; raw[:, 63] = r.uniform(0.9, 1.3, B); raw[:, 262:265] *= 0.1; raw[:, 265:] *= 0.02
    raw[:, 64:262] *= 3.0                                   # peaked 66-bin pose logits
    return torch.from_numpy(raw)


def _split(t):
    from oracle import canonswap_ref as O
    info, o = {}, 0
    for k, n in O.M_HEADS:
        info[k] = t[:, o:o + n].clone(); o += n
    return info


def test_driven_keypoints_vs_oracle(swapper_m):
    """x_t[b] = scale_pose * (kp @ R_pose + exp[b]) + (t_x, t_y, 0) for B = 4 driving rows and ONE pose row, on random raw heads shaped as
    in test_gpu_chain.py::test_keypoints_kernel_vs_oracle and with that test's bound."""
    from oracle import canonswap_ref as O
    B = 4
    raw_d, raw_p = _raw_heads(B, 3), _raw_heads(1, 4)
    kp = _raw_heads(1, 5)[:, :63].reshape(21, 3).contiguous()
    pose_info, drv = _split(raw_p), _split(raw_d)
    R_pose = O.get_rotation_matrix(*[O.headpose_pred_to_degree(pose_info[k]) for k in ("pitch", "yaw", "roll")])      # :301
    t_pose = pose_info["t"].clone()                                                                                   # :302
    t_pose[..., 2].fill_(0)                                                                                           # :303
    want = pose_info["scale"] * (kp[None] @ R_pose + drv["exp"].reshape(B, 21, 3)) + t_pose                           # :304-305
    got = swapper_m.engine.motion_keypoints_driven(raw_d.cuda(), raw_p.cuda(), kp.cuda()).cpu()
    bound = 2e-6 * max(1.0, want.abs().max().item()) * 4
    err = (got - want).abs().max().item()
    print(f"driven key-points vs oracle: max |diff| {err:.3e} (bound {bound:.3e})")
    assert got.shape == (B, 21, 3) and err <= bound
    assert (got[:, :, 2] - (pose_info["scale"] * (kp[None] @ R_pose + drv["exp"].reshape(B, 21, 3)))[:, :, 2]).abs().max().item() <= bound   # no t_z


def test_driven_keypoints_reduce_to_cs_motion_keypoints(swapper_m):
    """With raw_pose = raw_driving[b] and kp = that row's kp the driven key-points are that row's x_t of cs_motion_keypoints."""
    e = swapper_m.engine
    B = 4
    raw = _raw_heads(B, 7).cuda()
    x_t, _ = e.motion_keypoints(raw)
    for b in range(B):
        got = e.motion_keypoints_driven(raw[b:b + 1], raw[b:b + 1], raw[b, :63].reshape(21, 3))
        assert (got[0] - x_t[b]).abs().max().item() <= 2e-6 * max(1.0, x_t.abs().max().item()) * 4, b


def test_driven_keypoints_beyond_one_wavefronts_frames(swapper_m):
    """A wavefront walks 16 frames.  37 rows in one call of the C entry point (which, like cs_motion_keypoints, is not bound to the engine's
    max_batch) == the rows through the Python binding four at a time, bit for bit; and the binding checks its buffers."""
    e = swapper_m.engine
    N = 37
    raw, pose = _raw_heads(N, 8).cuda(), _raw_heads(1, 9).cuda()
    kp = _raw_heads(1, 10)[:, :63].reshape(21, 3).cuda()
    got = torch.full((N + 1, 21, 3), -7.0, device=e.device)
    e._call("cs_motion_keypoints_driven", N, raw, pose, kp, got)
    for b in range(0, N, 4):
        assert torch.equal(got[b:min(b + 4, N)], e.motion_keypoints_driven(raw[b:b + 4], pose, kp)), b
    assert (got[N] == -7.0).all()                           # nothing behind the last row
    assert not torch.equal(got[0], got[36])
    with pytest.raises(ValueError):
        e.motion_keypoints_driven(raw[:4], pose[:, :100], kp)
    with pytest.raises(ValueError):
        e.motion_keypoints_driven(raw[:4], pose, kp, out=torch.empty((4, 21, 3), dtype=torch.float64, device=e.device))
    with pytest.raises(ValueError):
        e.motion_keypoints_driven(raw, pose, kp)           # 37 rows on an engine created for 4


# ------------------------------------------------------------------------------------------------ kernel (c): the shared paste
def _paste_case(B, Ho, Wo, seed, outside=False):
    from oracle import cv_ref as R
    r = np.random.Generator(np.random.PCG64(seed))
    crops = r.integers(0, 256, size=(B, 512, 512, 3), dtype=np.uint8)
    ori = r.integers(0, 256, size=(Ho, Wo, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    mask = np.clip(1.2 - np.hypot(xx - 256, yy - 256) / 190, 0, 1).astype(np.float32)
    M = _affine(1, Ho, Wo) * np.array([[min(1.0, Ho / 700)], [min(1.0, Ho / 700)], [1]])
    if outside:
        M[0, 2] = -150.5 * min(1.0, Ho / 700)              # partly outside the frame
    mo = R.prepare_paste_back(np.stack([mask] * 3, -1), M, (Wo, Ho))[..., 0].copy()      # can_swap_pipeline_v2i.py:255-258
    return crops, ori, M, mo


@pytest.mark.parametrize("size,outside", [((720, 1280), False), ((720, 1280), True), ((301, 403), False), ((302, 404), True)],
                         ids=["720x1280", "720x1280-outside", "301x403-odd", "302x404-dwords"])
def test_paste_back_shared_equals_single_frames(swapper_m, size, outside):
    """B = 3 frames into one image under one mask == three calls of the single-frame kernel with mask_ori given, and == cv_ref.paste_back.
    1280 columns take the eight-pixel path, 404 the four-pixel one, 403 the per-frame fallback."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    Ho, Wo = size
    e = swapper_m.engine
    B = 3
    crops, ori, M, mo = _paste_case(B, Ho, Wo, 17, outside)
    got = tail.paste_back_shared(e, crops, M, ori, mo).cpu().numpy()
    assert got.shape == (B, Ho, Wo, 3)
    assert (mo > 0).any() and (mo == 0).any()
    for k in range(B):
        one = tail.paste_back(e, crops[k], M, ori, mo).cpu().numpy()
        assert np.array_equal(got[k], one), k
        assert np.array_equal(got[k], R.paste_back(crops[k], M, ori, np.stack([mo] * 3, -1))), k
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("size", [(96, 128), (90, 132)], ids=["96x128", "90x132-dwords"])
def test_paste_back_shared_beyond_64_frames(swapper_m, size):
    """B = 70: more than one 64-frame chunk of the batch kernel and several frame groups of this one."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    Ho, Wo = size
    e = swapper_m.engine
    B = 70
    crops, ori, M, mo = _paste_case(B, Ho, Wo, 19)
    M = np.array([[0.2, -0.02, 10.25], [0.02, 0.2, -8.5], [0, 0, 1]], np.float64)          # the crop covers most of the small frame
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    mask = np.clip(1.2 - np.hypot(xx - 256, yy - 256) / 190, 0, 1).astype(np.float32)
    mo = R.prepare_paste_back(np.stack([mask] * 3, -1), M, (Wo, Ho))[..., 0].copy()
    assert (mo > 0).sum() > 1000
    got = tail.paste_back_shared(e, crops, M, ori, mo).cpu().numpy()
    for k in range(B):
        assert np.array_equal(got[k], R.paste_back(crops[k], M, ori, np.stack([mo] * 3, -1))), k
    assert np.array_equal(got[69], tail.paste_back(e, crops[69], M, ori, mo).cpu().numpy())
    assert not np.array_equal(got[63], got[64])


def test_paste_back_shared_with_a_mask_beyond_the_crop(swapper_m):
    """The entry point takes any mask_ori: where all four taps lie outside the crop the warped value is 0 and the result (1 - m) * ori, the
    same for every frame and formed without reading the crop; still bit-equal to the single-frame kernel and to cv_ref."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    e = swapper_m.engine
    B, Ho, Wo = 3, 200, 320
    crops, ori, M, _ = _paste_case(B, Ho, Wo, 23, outside=True)
    r = np.random.Generator(np.random.PCG64(24))
    mo = r.uniform(0, 1, size=(Ho, Wo)).astype(np.float32)
    mo[r.uniform(size=(Ho, Wo)) < 0.3] = 0
    got = tail.paste_back_shared(e, crops, M, ori, mo).cpu().numpy()
    for k in range(B):
        assert np.array_equal(got[k], tail.paste_back(e, crops[k], M, ori, mo).cpu().numpy()), k
        assert np.array_equal(got[k], R.paste_back(crops[k], M, ori, np.stack([mo] * 3, -1))), k


def test_paste_back_shared_validates_its_buffers(swapper_m):
    from canonswap_amd import tail
    e = swapper_m.engine
    crops, ori, M, mo = _paste_case(2, 64, 96, 29)
    good = torch.empty((2, 64, 96, 3), dtype=torch.uint8, device=e.device)
    assert tail.paste_back_shared(e, crops, M, ori, mo, out=good) is good
    for bad in (torch.empty((1, 64, 96, 3), dtype=torch.uint8, device=e.device), torch.empty((2, 64, 96, 3), dtype=torch.float32, device=e.device),
                torch.empty((2, 64, 96, 3), dtype=torch.uint8), torch.empty((2, 64, 192, 3), dtype=torch.uint8, device=e.device)[:, :, ::2]):
        with pytest.raises(ValueError):
            tail.paste_back_shared(e, crops, M, ori, mo, out=bad)
    with pytest.raises(ValueError):
        tail.paste_back_shared(e, crops, M, np.stack([ori, ori]), mo)                   # one image, not B
    with pytest.raises(ValueError):
        tail.paste_back_shared(e, crops, M, ori, mo[:, :50])


# ------------------------------------------------------------------------------------------------ the chain against the oracle
B_DRV, HO, WO = 2, 540, 960


@pytest.fixture(scope="module")
def case(sds_m):
    """Inputs of one v2i run and the ORACLE's composition of can_swap_pipeline_v2i.py on them: the set-up (execute_face_canonical :61-106,
    the i == 0 branch :285-304, the mask :255-258) and the loop (:260-321) for B_DRV driving frames."""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    from oracle import cv_ref as R
    src_crop = _crops(1, 3100)[0]
    drv_crops = _crops(B_DRV, 3200)
    mask = _masks(1, seed=33)[0]
    r = np.random.Generator(np.random.PCG64(35))
    ori = r.integers(0, 256, size=(HO, WO, 3), dtype=np.uint8)
    M = _small_affine(1, HO, WO)
    idv = torch.from_numpy(synth.make_identity(7))
    Fsd, Wsd, Msd = sds_m["appearance_feature_extractor"], sds_m["warping_module"], sds_m["motion_extractor"]
    with torch.no_grad():
        I_s = O.prepare_source(R.resize_area_2x_u8(src_crop))                               # cropper.py:155, :86
        x_s_info = O.get_kp_info(Msd, I_s)                                                  # :87
        f_s = O.appearance_feature_extractor(Fsd, I_s)                                      # :89
        x_s = O.transform_keypoint(x_s_info)                                                # :90
        x_d_i_new = x_s_info["scale"][..., None] * x_s_info["kp"]                           # :92-94
        f_s_can, occ_map, _ = O.warp(Wsd, f_s, kp_source=x_s, kp_driving=x_d_i_new)         # :97
        f_can_swap = O.transfer(sds_m["transfer"], f_s_can, idv)                            # :286
        swap_can = O.conv_decode(sds_m, f_can_swap, occ_map)                                # :289
        swap_can_256 = F.interpolate(swap_can, size=(256, 256), mode="bilinear", align_corners=False)      # :294
        x_swap_info = O.get_kp_info(Msd, swap_can_256)                                      # :297
        x_swap = O.transform_keypoint(x_swap_info)                                          # :298
        R_swap = O.get_rotation_matrix(x_s_info["pitch"], x_s_info["yaw"], x_s_info["roll"])      # :301
        t_swap = x_s_info["t"].clone()                                                      # :302
        t_swap[..., 2].fill_(0)                                                             # :303
        scale_swap = x_s_info["scale"]                                                      # :304
        f_swap_can_2 = O.appearance_feature_extractor(Fsd, swap_can_256)                    # :308 (the same every frame)
        soft, _ = R.soft_erosion(torch.from_numpy(mask[None, None].astype(np.float32)), 21, 0.9, 2)       # :43, :255
        mask_ori = R.prepare_paste_back(np.stack([soft.numpy()[0, 0]] * 3, -1), M, (WO, HO))             # :257-258
        raw_pose = torch.cat([O.motion_extractor(Msd, I_s)[k] for k, _ in O.M_HEADS], 1)    # the raw heads x_s_info was refined from
        x_t_2, crops_out, frames = [], [], []
        for k in range(B_DRV):
            I_d = O.prepare_source(R.resize_area_2x_u8(drv_crops[k]))                       # :223, :235
            x_t_info = O.get_kp_info(Msd, I_d)                                              # :161
            delta_t = x_t_info["exp"]                                                       # :269
            x_t = scale_swap * (x_swap_info["kp"] @ R_swap + delta_t) + t_swap              # :305
            out = O.spade_decoder(sds_m["spade_generator"],
                                  O.warping_forward(Wsd, f_swap_can_2, kp_driving=x_t, kp_source=x_swap)["out"])      # :309
            I_p = O.parse_output(out)[0]                                                    # :312
            x_t_2.append(x_t[0]); crops_out.append(I_p)
            frames.append(R.paste_back(I_p, M, ori, mask_ori))                              # :317-320
    return dict(src_crop=src_crop, drv_crops=drv_crops, mask=mask, ori=ori, M=M, idv=idv, x_s=x_s, swap_can=swap_can, x_swap=x_swap,
                kp_swap=x_swap_info["kp"][0].contiguous(), f_swap_can_2=f_swap_can_2, mask_ori=mask_ori[..., 0].copy(), raw_pose=raw_pose,
                x_t_2=torch.stack(x_t_2), frames=np.stack(frames), region=mask_ori[..., 0] > 0)


def _set_source(chain, case):
    return chain.set_source(torch.from_numpy(case["src_crop"]).cuda(), torch.from_numpy(case["mask"]).cuda(), case["M"],
                            torch.from_numpy(case["ori"]).cuda(), case["idv"].cuda())


def _frame_figures(got, case, k):
    region = case["region"]
    want = case["frames"][k]
    d = got[region].astype(np.float64) - want[region].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max((d ** 2).mean(), 1e-12)), np.abs(d).mean()


def test_set_source_products_vs_oracle(swapper_m, case):
    """The engine's set-up against the oracle's, both fed the same uint8 crop and both on their own M: swap_can >= 50 dB (the gate
    test_frame_with_hip_keypoints puts on the whole loop body, of which F -> W.warp -> T -> decode is a part), x_s <= 1e-4 (the bound
    test_chain_vs_oracle_loop uses for x_t)."""
    from canonswap_amd.chain import AnimateChain
    from oracle import canonswap_ref as O
    chain = AnimateChain(swapper_m)
    info = _set_source(chain, case)
    p = O.psnr(info["swap_can"].cpu(), case["swap_can"])
    ex = (info["x_s"].cpu() - case["x_s"]).abs().max().item()
    print(f"set_source: swap_can PSNR {p:.2f} dB, |x_s - oracle|max {ex:.3e}")
    assert p >= 50.0
    assert ex <= 1e-4
    assert np.array_equal(info["I_can"].cpu().numpy(), swapper_m.engine.pack_u8(info["swap_can"])[0].cpu().numpy())
    st = chain.source_state()
    assert set(st) == {"f_swap_can_2", "x_swap", "kp_swap", "raw_pose", "mask_ori", "img_ori", "M_c2o"}
    assert st["mask_ori"].shape == (HO, WO) and st["f_swap_can_2"].shape == (1, 32, 16, 64, 64) and st["kp_swap"].shape == (21, 3)


def test_per_frame_chain_on_the_oracles_setup(swapper_m, case):
    """The per-frame path alone: the engine is handed the ORACLE's set-up products through load_source_state and runs B = 2 driving frames
    into a 540 x 960 image; the gates of test_gpu_chain.py::test_chain_vs_oracle_loop."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    chain.load_source_state({"f_swap_can_2": case["f_swap_can_2"], "x_swap": case["x_swap"], "kp_swap": case["kp_swap"],
                             "raw_pose": case["raw_pose"], "mask_ori": torch.from_numpy(case["mask_ori"]),
                             "img_ori": torch.from_numpy(case["ori"]), "M_c2o": case["M"]})
    res = chain(torch.from_numpy(case["drv_crops"]).cuda(), keep=True)
    got = res["frames"].cpu().numpy()
    ex = (res["x_t"].cpu() - case["x_t_2"]).abs().max().item()
    print(f"per-frame chain: |x_t - oracle|max {ex:.3e}")
    assert ex <= 1e-4
    worst = 1e9
    for k in range(B_DRV):
        assert np.array_equal(got[k][~case["region"]], case["ori"][~case["region"]])          # mask_ori == 0: the source image
        p, md = _frame_figures(got[k], case, k)
        print(f"per-frame chain, frame {k}: pasted region {int(case['region'].sum())} px, PSNR {p:.2f} dB, mean |diff| {md:.3f} LSB")
        worst = min(worst, p)
        assert md < 0.6
    assert worst >= 48.0


def test_end_to_end_vs_oracle(swapper_m, case):
    """Engine set-up + engine loop against oracle set-up + oracle loop on the same inputs.  The two sides run M and F on their own swap_can,
    which differ at the 50-60 dB level, so this also measures M's sensitivity to its input: the bounds are measured, 4 x the
    measured value for the two error norms and the project's 48 dB / 0.6 LSB gate for the frames (the measured worst frame clears 49 dB)."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    info = _set_source(chain, case)
    st = chain.source_state()
    ex = (info["x_swap"].cpu() - case["x_swap"]).abs().max().item()
    fo = case["f_swap_can_2"].double()
    ef = ((st["f_swap_can_2"].cpu().double() - fo).norm() / fo.norm()).item()
    em = np.abs(st["mask_ori"].cpu().numpy() - case["mask_ori"]).max()
    print(f"end to end: |x_swap - oracle|max {ex:.3e}, f_swap_can_2 relative L2 {ef:.3e}, |mask_ori - oracle|max {em:.3e}")
    got = chain(torch.from_numpy(case["drv_crops"]).cuda())["frames"].cpu().numpy()
    figs = [_frame_figures(got[k], case, k) for k in range(B_DRV)]
    for k, (p, md) in enumerate(figs):
        print(f"end to end, frame {k}: PSNR {p:.2f} dB, mean |diff| {md:.3f} LSB")
    assert ex <= X_SWAP_BOUND
    assert ef <= F_SWAP_BOUND
    for k, (p, md) in enumerate(figs):
        assert p >= E2E_PSNR_DB and md < E2E_MEAN_LSB, k


X_SWAP_BOUND = 2.8e-4      # measured 6.9e-5 (|x_swap - oracle|max: M on the engine's swap_can_256 against M on the oracle's)
F_SWAP_BOUND = 1.7e-3      # measured 4.2e-4 (f_swap_can_2, relative L2)
E2E_PSNR_DB, E2E_MEAN_LSB = 48.0, 0.6      # measured 55.46 / 55.40 dB, 0.185 / 0.187 LSB: the worst frame clears 49 dB, so the project's u8 gate


# ------------------------------------------------------------------------------------------------ the chain == its stages
def test_chain_equals_its_stages(swapper_m, case):
    from canonswap_amd import tail
    from canonswap_amd.chain import AnimateChain
    e = swapper_m.engine
    chain = AnimateChain(swapper_m)
    _set_source(chain, case)
    st = chain.source_state()
    crops = torch.from_numpy(case["drv_crops"]).cuda()
    res = chain(crops, keep=True)
    frames = res["frames"].clone()
    I = tail.prepare_crops(e, crops)
    assert torch.equal(I, res["I"])
    x_t = e.motion_keypoints_driven(e.motion_extract_raw(I), st["raw_pose"], st["kp_swap"])
    assert torch.equal(x_t, res["x_t"])
    gen = e.animate_frames(st["f_swap_can_2"], st["x_swap"], x_t, want_f32=False, want_u8=True)["out_u8"]
    assert torch.equal(gen, res["crops_out"])
    for k in range(B_DRV):
        one = tail.paste_back(e, gen[k], st["M_c2o"], st["img_ori"], st["mask_ori"])
        assert torch.equal(one, frames[k]), k
    # the set-up == its stages: the soft mask of the module, warped once
    soft, _ = chain.se(torch.from_numpy(case["mask"][None, None]).cuda().float())
    assert torch.equal(tail.prepare_paste_back(e, soft[0, 0], case["M"], (WO, HO)), st["mask_ori"])
    out = torch.empty_like(frames)
    assert chain(crops, out=out)["frames"] is out and torch.equal(out, frames)


# ------------------------------------------------------------------------------------------------ stream rules
def _drv(seed, B=2):
    return torch.from_numpy(_crops(B, seed)).cuda()


def test_call_before_set_source_raises(swapper_m):
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    with pytest.raises(RuntimeError, match="no source"):
        chain(_drv(3300))
    with pytest.raises(RuntimeError, match="no source"):
        chain.prefetch(_drv(3300))
    with pytest.raises(RuntimeError, match="no source"):
        chain.source_state()
    assert not chain._pending


def test_prefetched_batches_give_the_same_frames(swapper_m, case):
    """prefetch-then-hit over three batches == the in-line chain, byte for byte; a third prefetch raises."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    _set_source(chain, case)
    batches = [_drv(3400 + k) for k in range(3)]
    want = [chain(b)["frames"].clone() for b in batches]
    assert not torch.equal(want[0], want[1])
    chain.prefetch(batches[0])
    got = []
    for k, b in enumerate(batches):
        if k + 1 < len(batches):
            chain.prefetch(batches[k + 1])
        got.append(chain(b)["frames"].clone())
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
    assert not chain._pending
    chain.prefetch(batches[0]); chain.prefetch(batches[1])
    with pytest.raises(RuntimeError, match="double buffer"):
        chain.prefetch(batches[2])
    # staged batches run in any order
    assert torch.equal(chain(batches[1])["frames"], want[1])
    chain.prefetch(batches[2])
    assert torch.equal(chain(batches[0])["frames"], want[0]) and torch.equal(chain(batches[2])["frames"], want[2])
    assert not chain._pending


@pytest.mark.parametrize("dropped", [False, True], ids=["pending", "dropped"])
def test_inline_stage_a_waits_for_a_prefetch_in_flight(swapper_m, case, dropped):
    """prefetch(b1), then chain(b0) with b0 never prefetched (or after drop_prefetches()): the in-line stage A uses the engine's one M
    scratch and must run behind the side stream's.  The side stream is held busy before the prefetch is queued, so without that ordering
    the in-line call would end first."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    _set_source(chain, case)
    b0, b1 = _drv(3500), _drv(3501)
    want = [chain(b)["frames"].clone() for b in (b0, b1)]
    assert not torch.equal(want[0], want[1])
    chain.prefetch(b1)                                    # a first prefetch / hit pair creates the side stream
    assert torch.equal(chain(b1)["frames"], want[1])
    a, z = _timed(), _timed()
    a.record(); chain(b0); z.record(); z.synchronize()
    dt = a.elapsed_time(z)
    _occupy(chain._side, max(40.0, 8 * dt))
    chain.prefetch(b1)
    staged = _timed()
    staged.record(chain._side)
    if dropped:
        chain.drop_prefetches()
    got0 = chain(b0)["frames"]
    end0 = _timed()
    end0.record()
    got1 = chain(b1)["frames"]
    torch.cuda.synchronize()
    print(f"in-line call {dt:.2f} ms; its end {staged.elapsed_time(end0):.2f} ms after the prefetch's")
    assert staged.elapsed_time(end0) > 0
    assert torch.equal(got0, want[0]) and torch.equal(got1, want[1])
    assert not chain._pending


def test_set_source_with_a_batch_staged_drops_it(swapper_m, case):
    """A staged batch's key-points were formed with the old kp_swap / pose: set_source and load_source_state forget it (and wait for the
    side stream, whose M shares the engine's scratch with the set-up's), and the batch then runs in-line under the new source."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    _set_source(chain, case)
    first = chain.source_state()
    b = _drv(3600)
    want_first = chain(b)["frames"].clone()
    other_crop = torch.from_numpy(_crops(1, 3700)[0]).cuda()
    args = (other_crop, torch.from_numpy(_masks(1, seed=37)[0]).cuda(), _small_affine(0, HO, WO), torch.from_numpy(case["ori"]).cuda(), case["idv"].cuda())
    fresh = AnimateChain(swapper_m)
    fresh.set_source(*args)
    want_other = fresh(b)["frames"].clone()
    assert not torch.equal(want_first, want_other)
    chain.prefetch(b)
    assert len(chain._pending) == 1
    _occupy(chain._side, 20.0)
    chain.prefetch(_drv(3601))
    chain.set_source(*args)
    assert not chain._pending
    assert torch.equal(chain(b)["frames"], want_other)
    chain.prefetch(b)
    chain.load_source_state(first)
    assert not chain._pending
    assert torch.equal(chain(b)["frames"], want_first)


def test_latency_mode_chain_refuses_prefetch_and_runs_in_line(sds_m, swapper_m, case):
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain
    sw = can_swapper(None, state_dicts=sds_m, max_batch=1, latency_mode=True)
    chain = AnimateChain(sw)
    _set_source(chain, case)
    b = _drv(3800, B=1)
    with pytest.raises(RuntimeError, match="latency"):
        chain.prefetch(b)
    assert chain._side is None and not chain._pending
    got = chain(b)["frames"].cpu().numpy()
    assert got.shape == (1, HO, WO, 3)
    assert np.array_equal(got[0][~case["region"]], case["ori"][~case["region"]])
    del sw, chain
    torch.cuda.empty_cache()
