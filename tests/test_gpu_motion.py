"""Motion extractor M on the HIP engine against the oracle and the reference's own vectors.

M's GEMMs run in split precision (hi/lo fp16 operand pairs, fp32 accumulate; csrc/motion.hip), LayerNorm / GRN / GELU and
the residual stream in fp32: plain fp16 operands gave 1e-3 on the key-points and only 41 dB on the generated frame, the
split form measures 2.5e-6.  Gates: |d kp|, |d exp|, |d t|, |d scale| <= 1e-4, head-pose <= 0.01 degree, transformed
key-points <= 1e-4, and >= 50 dB on the generated frame when the key-points come from the HIP M instead of the oracle's.
"""
import numpy as np
import pytest
import torch

import chain_helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


@pytest.fixture(scope="module")
def imgs():
    from canonswap_amd import synth
    return torch.from_numpy(synth.make_smooth_images(3, seed=2000, size=256))


def _chk(out, ref):
    for k in ("kp", "exp", "t", "scale"):
        d = (out[k].float().cpu().reshape(-1) - ref[k].reshape(-1)).abs().max().item()
        print(f"\n  |d {k}| = {d:.2e}", end="")
        assert d <= 1e-4, (k, d)


def test_raw_heads_vs_oracle(swapper_m, sds_m, imgs):
    from oracle import canonswap_ref as O
    with torch.no_grad():
        ref = O.motion_extractor(sds_m["motion_extractor"], imgs)
    out = swapper_m.motion_extractor(imgs.cuda())
    assert set(out) == set(ref)
    for k, n in O.M_HEADS:
        assert out[k].shape == (3, n) and out[k].dtype == torch.float32
    _chk(out, ref)
    for k in ("pitch", "yaw", "roll"):     # 66-bin logits -> expected degrees (camera.py:14-28)
        dd = (O.headpose_pred_to_degree(out[k].cpu()) - O.headpose_pred_to_degree(ref[k])).abs().max().item()
        assert dd <= 0.01, (k, dd)


def test_raw_heads_vs_reference_vectors(swapper_m, golden, imgs):
    g = golden("motion_b3.npz")            # written by tools/make_golden.py from the reference's MotionExtractor
    out = swapper_m.motion_extractor(imgs.cuda())
    _chk(out, {k: torch.from_numpy(g[k]) for k in ("kp", "exp", "t", "scale")})


def test_get_kp_info_and_transform(swapper_m, sds_m, imgs):
    from oracle import canonswap_ref as O
    with torch.no_grad():
        ref = O.get_kp_info(sds_m["motion_extractor"], imgs)
        xr = O.transform_keypoint(ref)
    info = swapper_m.get_kp_info(imgs.cuda())
    assert info["kp"].shape == (3, 21, 3) and info["exp"].shape == (3, 21, 3) and info["pitch"].shape == (3, 1)
    x = swapper_m.transform_keypoint(info)
    assert x.shape == (3, 21, 3)
    assert (x.cpu() - xr).abs().max().item() <= 1e-4
    raw = swapper_m.get_kp_info(imgs.cuda(), flag_refine_info=False)
    assert raw["pitch"].shape == (3, 66) and raw["kp"].shape == (3, 63)


def test_batch_independence(swapper_m, imgs):
    a = swapper_m.motion_extractor(imgs.cuda())
    b = swapper_m.motion_extractor(imgs[1:2].cuda())
    for k in a:
        assert torch.equal(a[k][1:2], b[k]), k


def test_frame_with_hip_keypoints(swapper_m, sds_m, imgs):
    """M feeding the generator: x_t from the driving frame, x_can = scale * kp (can_swap_pipeline_e2e.py:236-241)."""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    idv = torch.from_numpy(synth.make_identity(7))
    frame = imgs[:1]
    info = swapper_m.get_kp_info(frame.cuda())
    x_t = swapper_m.transform_keypoint(info)
    x_can = info["scale"][..., None] * info["kp"]
    with torch.no_grad():
        rinfo = O.get_kp_info(sds_m["motion_extractor"], frame)
        rx_t, rx_can = O.transform_keypoint(rinfo), rinfo["scale"][..., None] * rinfo["kp"]
        ref = O.swap_frame(sds_m, frame, rx_t, rx_can, idv)
    out = swapper_m.swap_frames(frame.cuda(), x_t, x_can, idv.cuda())["out"]
    assert O.psnr(out.cpu(), ref["out"]) >= 50.0


def test_missing_motion_weights(state_dicts):
    from canonswap_amd.can_swap_e2e import can_swapper
    sw = can_swapper(None, state_dicts=state_dicts, max_batch=1)
    with pytest.raises(RuntimeError):
        sw.get_kp_info(torch.zeros(1, 3, 256, 256, device="cuda"))


def test_pose_and_source_helpers(swapper_m, sds_m, imgs):
    """get_pose_dct / get_fs_and_kp_info / calc_ratio (can_swap_e2e.py:201-226, 324-331) on the engine."""
    from oracle import canonswap_ref as O
    raw = swapper_m.get_kp_info(imgs[:1].cuda(), flag_refine_info=False)
    pose = swapper_m.get_pose_dct(raw)
    with torch.no_grad():
        ref = O.motion_extractor(sds_m["motion_extractor"], imgs[:1])
    for k in ("pitch", "yaw", "roll"):
        assert abs(pose[k] - O.headpose_pred_to_degree(ref[k]).item()) <= 0.01
    s_info, s_rot, f_s, d_info, d_rot = swapper_m.get_fs_and_kp_info(imgs[:1].cuda(), imgs[1:2].cuda())
    assert f_s.shape == (1, 32, 16, 64, 64) and s_rot.shape == (1, 3, 3) and d_info["kp"].shape == (1, 21, 3)
    lmk = [np.random.default_rng(0).uniform(0, 256, size=(106, 2)).astype(np.float32) for _ in range(2)]
    eyes, lips = swapper_m.calc_ratio(lmk)
    assert len(eyes) == 2 and eyes[0].shape == (1, 2) and lips[0].shape == (1, 1)
    assert swapper_m.calc_combined_eye_ratio(eyes[0], lmk[1]).shape == (1, 3)
    assert swapper_m.calc_combined_lip_ratio(lips[0], lmk[1]).shape == (1, 2)


# ---- M where the chain runs it: one frame per call in latency mode (split-K downsample convs), 64 / 84 frames per launch
@pytest.fixture(scope="module")
def swapper_lat(sds_m):
    from canonswap_amd.can_swap_e2e import can_swapper
    sw = can_swapper(None, state_dicts=sds_m, max_batch=1, latency_mode=True)
    yield sw
    sw.engine.close()


def test_latency_mode_raw_heads_vs_oracle_and_reference_vectors(swapper_lat, sds_m, golden, imgs):
    from oracle import canonswap_ref as O
    with torch.no_grad():
        ref = O.motion_extractor(sds_m["motion_extractor"], imgs)
    g = golden("motion_b3.npz")
    outs = [swapper_lat.motion_extractor(imgs[i:i + 1].cuda()) for i in range(3)]
    out = {k: torch.cat([o[k] for o in outs]) for k in outs[0]}
    _chk(out, ref)
    _chk(out, {k: torch.from_numpy(g[k]) for k in ("kp", "exp", "t", "scale")})
    for k in ("pitch", "yaw", "roll"):
        dd = (O.headpose_pred_to_degree(out[k].cpu()) - O.headpose_pred_to_degree(ref[k])).abs().max().item()
        print(f"\n  |d {k}| = {dd:.2e} degree", end="")
        assert dd <= 0.01, (k, dd)


@pytest.mark.parametrize("B", [64, 84])
def test_chain_batch_frames_equal_b1_and_oracle(sds_m, B):
    """Conv tiles are chosen by B: frames 0, 31, 63 (and 83) of a B-frame launch equal the same frame alone, bit for bit, and the oracle."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    from oracle import canonswap_ref as O
    frames = [0, 31, 63] + ([83] if B == 84 else [])
    im = torch.from_numpy(synth.make_smooth_images(B, seed=2100, size=256))
    sw = can_swapper(None, state_dicts=sds_m, max_batch=B)
    try:
        out = sw.motion_extractor(im.cuda())
        for f in frames:
            one = sw.motion_extractor(im[f:f + 1].cuda())
            for k in out:
                assert torch.equal(out[k][f:f + 1], one[k]), (f, k)
    finally:
        sw.engine.close()
    with torch.no_grad():
        ref = O.motion_extractor(sds_m["motion_extractor"], im[frames])
    _chk({k: v[frames] for k, v in out.items()}, ref)


def _kp_ref(raw):
    """float64 restatement of cs_motion_keypoints: softmax-expected degrees, R = (Rz Ry Rx)^T, x_t = s (kp R + exp) + t_xy, x_can = s kp"""
    r = raw.double()
    idx = torch.arange(66, dtype=torch.float64)
    deg = [(torch.softmax(r[:, a:a + 66], 1) * idx).sum(1) * 3 - 97.5 for a in (64, 130, 196)]
    x, y, z = [d * np.pi / 180 for d in deg]
    o, n = torch.ones_like(x), torch.zeros_like(x)
    rx = torch.stack([o, n, n, n, x.cos(), -x.sin(), n, x.sin(), x.cos()], 1).view(-1, 3, 3)
    ry = torch.stack([y.cos(), n, y.sin(), n, o, n, -y.sin(), n, y.cos()], 1).view(-1, 3, 3)
    rz = torch.stack([z.cos(), -z.sin(), n, z.sin(), z.cos(), n, n, n, o], 1).view(-1, 3, 3)
    R = (rz @ ry @ rx).transpose(1, 2)
    kp, s = r[:, :63].view(-1, 21, 3), r[:, 63].view(-1, 1, 1)
    x_t = s * (kp @ R + r[:, 265:].view(-1, 21, 3))
    x_t[:, :, :2] += r[:, None, 262:264]
    return deg, R, x_t, s * kp


def test_keypoints_with_peaked_logits(swapper_m):
    """Pose logits peaked by >= 80 at bins 0, 33, 65 (-97.5, 1.5, +97.5 degrees), on a common offset of 1000, and with two equal maxima."""
    gen = np.random.Generator(np.random.PCG64(11))
    raw = gen.normal(0, 1, size=(4, 328))
    raw[:, :63] *= 0.3; raw[:, 63] = gen.uniform(0.9, 1.3, 4); raw[:, 262:265] *= 0.1; raw[:, 265:] *= 0.02
    cases = [(0, 65, 33), (65, 0, 0), (33, 33, 65)]            # peak bins of (pitch, yaw, roll) for frames 0 - 2
    for f, bins in enumerate(cases):
        for a, b in zip((64, 130, 196), bins):
            raw[f, a + b] = raw[f, a:a + 66].max() + 80 + f
    raw[2, 130:196] += 1000.0                                    # common offset: only the max subtraction keeps exp() finite
    for a, (b0, b1) in zip((64, 130, 196), ((10, 50), (64, 65), (0, 65))):   # frame 3: two equal maxima
        raw[3, a + b0] = raw[3, a + b1] = raw[3, a:a + 66].max() + 90
    t = torch.from_numpy(raw.astype(np.float32))
    deg, R_ref, xt_ref, xc_ref = _kp_ref(t)
    assert abs(deg[0][0] + 97.5) < 1e-9 and abs(deg[1][0] - 97.5) < 1e-9 and abs(deg[2][0] - 1.5) < 1e-9
    assert abs(deg[0][3] + 7.5) < 1e-9 and abs(deg[1][3] - 96.0) < 1e-9 and abs(deg[2][3]) < 1e-9
    x_t, x_can, R = swapper_m.engine.motion_keypoints(t.cuda(), want_rot=True)
    # fp32 softmax / sincos / 3-term products: measured 1.7e-7 (R), 1.9e-7 (x_t, relative to its largest value)
    dr = (R.cpu().double() - R_ref).abs().max().item()
    dx = (x_t.cpu().double() - xt_ref).abs().max().item() / xt_ref.abs().max().item()
    print(f"\nkeypoints, peaked logits: |dR| {dr:.3e}, |dx_t| / max {dx:.3e}")
    assert dr <= 6e-7 and dx <= 7e-7, (dr, dx)
    assert (x_can.cpu().double() - xc_ref).abs().max().item() <= 2 ** -24 * xc_ref.abs().max().item()      # one fp32 product
