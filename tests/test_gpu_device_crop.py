"""The crop and the paste-back from landmarks and matrices that stay on the device (cs_crop_lmk, cs_paste_back_faces_dev; tail.crop_lmk /
paste_back_faces_dev; FrameChain's device route).  Every comparison is bit for bit, none has a tolerance:
* M against cs_lmk_input's M for the same arguments (the same geometry text);
* the crop against cs_crop_faces on the device's own M_o2c read back and widened to double; I against cs_prepare_crops of that crop;
* lmk_crop against tests/device_crop_ref.py, numpy float32 operation by operation;
* the paste against cs_paste_back_faces on the float32 M_c2o widened to double;
* the chain's device route against the same chain fed host matrices taken from the device's M.
Shapes are the smallest that take every path: N = 203 and 5, dsize 8 and 16 (no staging) and 256 / 512 (both staged forms), a face over the frame's
border, a frame without a face, more faces than a workgroup's chunk and more frames than a launch, an odd width, a buffer off the dword grid."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_helpers
import device_crop_ref as DR
import landmarks_ref as LR

pytestmark = pytest.mark.gpu
CFG = dict(scale=2.3, vy_ratio=-0.125)


@pytest.fixture(scope="module")
def swapper_m():
    return chain_helpers.swapper_b4(chain_helpers.motion_state_dicts())


@pytest.fixture(scope="module")
def engine(swapper_m):
    return swapper_m.engine


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).view(np.uint32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _frames(F, Ho, Wo, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (F, Ho, Wo, 3), dtype=np.uint8)).cuda()


FI5 = np.array([0, 0, 1, 2, 2], np.int32)


def _faces(N):
    """Five faces in frames of 40 x 56; the fourth sits on the lower right corner, most of its crop over the border."""
    make = LR.synthetic_face if N == 203 else DR.face5
    return np.stack([make(20, 16, 11, 10), make(36, 24, 9, -25), make(28, 20, 14, 170), make(56, 40, 12, 40), make(14, 26, 8, -90)])


def _o2c64(M):
    return M.cpu().numpy()[:, :9].astype(np.float64).reshape(-1, 3, 3)


def _c2o64(M):
    return M.cpu().numpy()[:, 9:].astype(np.float64).reshape(-1, 3, 3)


# ------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("dsize", [8, 16])
@pytest.mark.parametrize("N", [203, 5])
def test_crop_equals_lmk_input_crop_faces_and_the_restatement(engine, N, dsize, rot):
    from canonswap_amd import landmarks, tail
    frames, faces = _frames(3, 40, 56), _faces(N)
    lmk = torch.from_numpy(faces).cuda()
    got = tail.crop_lmk(engine, frames, lmk, FI5, dsize=dsize, flag_do_rot=rot, want_lmk_crop=True, **CFG)
    assert set(got) == {"crops", "M", "status", "lmk_crop"} and got["status"].cpu().tolist() == [0] * 5
    want = landmarks.lmk_input(engine, frames, lmk, FI5, dsize=dsize, flag_do_rot=rot, **CFG)
    assert np.array_equal(_bits(got["M"]), _bits(want["M"])) and got["M"].any(dim=1).all()
    ref = tail.crop_faces_M(engine, frames, _o2c64(got["M"]), FI5, dsize)["crops"]
    assert torch.equal(got["crops"], ref), int((got["crops"] != ref).sum())
    assert got["crops"].any(dim=3).any(dim=2).any(dim=1).all()                       # every face reads pixels
    border = got["crops"][3].cpu().numpy()
    assert (border == 0).all(axis=2).any() and border.any()                          # the face over the border: the zero border, and pixels
    M_o2c = got["M"].cpu().numpy()[:, :9].reshape(-1, 3, 3)
    for b in range(5):
        assert np.array_equal(_bits(got["lmk_crop"][b]), _bits(DR.lmk_crop(faces[b], M_o2c[b]))), b
    plain = tail.crop_lmk(engine, frames, lmk, FI5, dsize=dsize, flag_do_rot=rot, **CFG)      # lmk_crop = NULL: the same crop
    assert set(plain) == {"crops", "M", "status"} and torch.equal(plain["crops"], got["crops"]) and torch.equal(plain["M"], got["M"])


@pytest.mark.parametrize("dsize", [256, 512])
def test_the_staged_input_is_prepare_crops_of_the_crop(engine, dsize):
    from canonswap_amd import tail
    frames = _frames(2, 40, 56, seed=4)
    lmk = torch.from_numpy(_faces(203)[[0, 3]]).cuda()
    got = tail.crop_lmk(engine, frames, lmk, dsize=dsize, want_I=True, **CFG)           # frame_index None: face b in frame b
    assert tuple(got["I"].shape) == (2, 3, 256, 256) and got["status"].cpu().tolist() == [0, 0]
    assert np.array_equal(_bits(got["I"]), _bits(tail.prepare_crops(engine, got["crops"])))
    ref = tail.crop_faces_M(engine, frames, _o2c64(got["M"]), [0, 1], dsize)["crops"]
    assert torch.equal(got["crops"], ref) and got["I"].any()
    off = torch.zeros(2 * dsize * dsize * 3 + 1, dtype=torch.uint8, device="cuda")[1:].view(2, dsize, dsize, 3)      # a crop buffer off the dword grid
    assert off.data_ptr() % 4 == 1
    odd = tail.crop_lmk(engine, frames, lmk, dsize=dsize, want_I=True, out={"crops": off}, **CFG)
    assert odd["crops"] is off and torch.equal(off, got["crops"]) and torch.equal(odd["I"], got["I"])


def test_more_faces_than_one_launch_takes(engine):
    from canonswap_amd import tail
    frames = _frames(3, 40, 56)
    faces = np.concatenate([_faces(203)] * 14)[:66]                                  # 66 faces: 64 + 2
    fi = np.sort(np.tile(FI5, 14)[:66]).astype(np.int32)
    lmk = torch.from_numpy(faces).cuda()
    got = tail.crop_lmk(engine, frames, lmk, fi, dsize=8, want_lmk_crop=True, **CFG)
    for b0 in (0, 64):
        part = tail.crop_lmk(engine, frames, lmk[b0:b0 + 2], fi[b0:b0 + 2], dsize=8, want_lmk_crop=True, **CFG)
        for k in ("crops", "M", "lmk_crop", "status"):
            assert torch.equal(got[k][b0:b0 + 2], part[k]), (b0, k)


# ------------------------------------------------------------------------------------------------ guard
def test_a_refused_face_is_zeros_and_the_mark_and_leaves_its_neighbours_alone(engine):
    from canonswap_amd import tail
    frames, faces = _frames(3, 40, 56), _faces(203)
    good = tail.crop_lmk(engine, frames, torch.from_numpy(faces).cuda(), FI5, dsize=16, want_lmk_crop=True, **CFG)
    others = [0, 1, 3, 4]
    nan, flat = faces.copy(), faces.copy()
    nan[2, 77, 1] = np.nan
    flat[2] = [21.5, 9.25]
    for name, lmk, held in (("nan", nan, 0), ("all points equal", flat, 0), ("status on entry", faces, 9)):
        status = torch.tensor([0, 0, held, 0, 0], dtype=torch.int32, device="cuda")
        out = {k: torch.full_like(good[k], 1) for k in ("crops", "M", "lmk_crop")}    # what was there is overwritten by zeros
        got = tail.crop_lmk(engine, frames, torch.from_numpy(lmk).cuda(), FI5, dsize=16, status=status, status_mark=7, out=out, **CFG)
        assert got["status"] is status and status.cpu().tolist() == [0, 0, held or 7, 0, 0], name
        for k in ("crops", "M", "lmk_crop"):
            assert got[k] is out[k] and not got[k][2].any(), (name, k)
            assert torch.equal(got[k][others], good[k][others]), (name, k)
    big = tail.crop_lmk(engine, frames[:2], torch.from_numpy(nan[[2, 0]]).cuda(), dsize=256, want_I=True, **CFG)      # the staged form too
    assert big["status"].cpu().tolist() == [1, 0] and not big["I"][0].any() and not big["crops"][0].any() and big["I"][1].any()


# ------------------------------------------------------------------------------------------------ paste
def _paste_both(engine, scene, status=None, out=None, ori=None, inplace=False):
    """(the device-matrix paste, the host-matrix paste of the same float32 matrices widened to double)."""
    from canonswap_amd import tail
    crops_np, masks_np, M, fi, ori_np = scene
    crops, masks = _dev(crops_np, masks_np)
    ori = _dev(ori_np)[0] if ori is None else ori
    m18, M64 = DR.m18(M)
    want = tail.paste_back_faces(engine, crops, masks, M64, fi, ori)
    if inplace:
        out = ori = ori.clone()
    got = tail.paste_back_faces_dev(engine, crops, masks, torch.from_numpy(m18).cuda(), fi, ori, status=status, out=out)
    return got, want


def test_paste_equals_paste_back_faces_out_of_place_and_in_place(engine):
    scene = DR.paste_scene()
    got, want = _paste_both(engine, scene)
    assert got.dtype == torch.uint8 and torch.equal(got, want), int((got != want).sum())
    ori = _dev(scene[4])[0]
    assert torch.equal(got[1], ori[1]) and not torch.equal(got[0], ori[0]) and not torch.equal(got[2], ori[2])
    one = list(scene)
    one[0], one[1], one[2], one[3] = scene[0][[1, 2]], scene[1][[1, 2]], scene[2][[1, 2]], scene[3][[1, 2]]
    assert not torch.equal(_paste_both(engine, one)[1][0], want[0])                  # the two faces of frame 0 overlap: the first one shows
    same, _ = _paste_both(engine, scene, inplace=True)
    assert torch.equal(same, want)


def test_no_face_at_all_copies_the_frames(engine):
    from canonswap_amd import tail
    ori = _dev(DR.paste_scene()[4])[0]
    none = torch.empty((0, 16, 16, 3), dtype=torch.uint8, device="cuda")
    out = torch.full_like(ori, 7)
    assert tail.paste_back_faces_dev(engine, none, none[..., 0].float(), None, [], ori, out=out) is out and torch.equal(out, ori)
    keep = ori.clone()
    assert tail.paste_back_faces_dev(engine, none, none[..., 0].float(), None, [], ori, out=ori) is ori and torch.equal(ori, keep)


@pytest.mark.parametrize("skip", [0, 1, 2])
def test_a_face_with_a_status_is_skipped_as_if_it_were_not_listed(engine, skip):
    scene = DR.paste_scene()
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    status[skip] = 5
    got, _ = _paste_both(engine, scene, status=status)
    keep = [b for b in range(3) if b != skip]
    without = [a[keep] for a in scene[:4]] + [scene[4]]
    assert torch.equal(got, _paste_both(engine, without)[1])
    everything = torch.ones(3, dtype=torch.int32, device="cuda")
    assert torch.equal(_paste_both(engine, scene, status=everything)[0], _dev(scene[4])[0])


def _off_by_one(t):
    raw = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=t.device)
    odd = raw[1:].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    return odd


def test_an_odd_width_and_a_buffer_off_the_dword_grid_take_the_per_pixel_path_with_the_same_bytes(engine):
    wide = DR.paste_scene(Wo=50)
    got, want = _paste_both(engine, wide)
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(_paste_both(engine, wide, inplace=True)[0], want)
    scene = DR.paste_scene()
    ori = _dev(scene[4])[0]
    _, want = _paste_both(engine, scene)
    for src, dst in ((_off_by_one(ori), None), (ori, _off_by_one(torch.zeros_like(ori)))):
        got, _ = _paste_both(engine, scene, ori=src, out=dst)
        assert (dst is None or got is dst) and torch.equal(got, want)
    buf = _off_by_one(ori)
    got, _ = _paste_both(engine, scene, ori=buf, out=buf)
    assert got is buf and torch.equal(buf, want)


@pytest.mark.parametrize("faces_per_frame,hw", [((33, 17), (24, 32)), ((1,) * 50, (8, 12))], ids=["50_faces_in_2_frames", "50_frames_of_one_face"])
def test_more_faces_than_a_chunk_and_more_frames_than_a_launch(engine, faces_per_frame, hw):
    scene = DR.many_scene(faces_per_frame, *hw, seed=7)
    got, want = _paste_both(engine, scene)
    assert torch.equal(got, want), int((got != want).sum())
    assert not torch.equal(got, _dev(scene[4])[0])
    assert torch.equal(_paste_both(engine, scene, inplace=True)[0], want)


# ------------------------------------------------------------------------------------------------ arguments through the C ABI
def test_arguments_are_refused_before_any_launch_naming_the_entry_point_and_the_argument(engine):
    from canonswap_amd import _lib, landmarks
    frames = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    lmk = torch.from_numpy(LR.synthetic_face(8, 8, 6, 0)[None]).cuda()
    M, crops = torch.full((1, 18), 3.0, device="cuda"), torch.full((1, 8, 8, 3), 0x5a, dtype=torch.uint8, device="cuda")
    I, crops16 = torch.full((1, 3, 256, 256), -3.0, device="cuda"), torch.full((1, 16, 16, 3), 0x5a, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    fi = lambda v: (C.c_int * 1)(v)
    L = landmarks.layout_of(203)
    bad = _lib.LmkLayout(4, L.left, L.right, (C.c_int * 2)(48, 203))
    ref = C.byref
    for word, args in (("NULL lmk", (1, 2, frames, 16, 16, fi(0), None, 203, ref(L), 8, 2.3, -0.125, 1, 1, M, crops, None, None, status)),
                       ("NULL M", (1, 2, frames, 16, 16, fi(0), lmk, 203, ref(L), 8, 2.3, -0.125, 1, 1, None, crops, None, None, status)),
                       ("NULL status", (1, 2, frames, 16, 16, fi(0), lmk, 203, ref(L), 8, 2.3, -0.125, 1, 1, M, crops, None, None, None)),
                       ("NULL layout", (1, 2, frames, 16, 16, fi(0), lmk, 203, None, 8, 2.3, -0.125, 1, 1, M, crops, None, None, status)),
                       ("dsize 6", (1, 2, frames, 16, 16, fi(0), lmk, 203, ref(L), 6, 2.3, -0.125, 1, 1, M, crops, None, None, status)),
                       ("I_out.*16", (1, 2, frames, 16, 16, fi(0), lmk, 203, ref(L), 16, 2.3, -0.125, 1, 1, M, crops16, I, None, status)),
                       (r"frame_index\[0\] = 2", (1, 2, frames, 16, 16, fi(2), lmk, 203, ref(L), 8, 2.3, -0.125, 1, 1, M, crops, None, None, status)),
                       ("layout lip.*203", (1, 2, frames, 16, 16, fi(0), lmk, 203, ref(bad), 8, 2.3, -0.125, 1, 1, M, crops, None, None, status))):
        with pytest.raises(RuntimeError, match=f"cs_crop_lmk: {word}"):
            engine._call("cs_crop_lmk", *args)
    out = torch.full((2, 16, 16, 3), 0x5a, dtype=torch.uint8, device="cuda")
    masks = torch.zeros((1, 8, 8), device="cuda")
    for word, args in (("NULL M", (1, 2, crops, masks, 8, 8, fi(0), None, None, frames, out, 16, 16)),
                       ("NULL out", (1, 2, crops, masks, 8, 8, fi(0), M, None, frames, None, 16, 16)),
                       (r"frame_index\[0\] = 2", (1, 2, crops, masks, 8, 8, fi(2), M, None, frames, out, 16, 16))):
        with pytest.raises(RuntimeError, match=f"cs_paste_back_faces_dev: {word}"):
            engine._call("cs_paste_back_faces_dev", *args)
    torch.cuda.synchronize()
    assert (M == 3.0).all() and (crops == 0x5a).all() and (crops16 == 0x5a).all() and (I == -3.0).all() and (out == 0x5a).all()
    assert not status.any()                                                              # nothing was launched


# ------------------------------------------------------------------------------------------------ the route through the chain
def test_frame_chain_from_device_landmarks_equals_the_chain_fed_host_matrices(swapper_m):
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import FrameChain
    from test_gpu_crop import _face
    e = swapper_m.engine
    r = np.random.Generator(np.random.PCG64(83))
    fr = _frames(2, 96, 128, seed=8)
    lmk_np = np.stack([_face(r, c, 26.0, r.uniform(-0.4, 0.4)) for c in [(40, 44), (84, 50), (60, 48)]]).astype(np.float32)
    fi = np.array([0, 0, 1], np.int32)
    masks = torch.from_numpy(chain_helpers._masks(3, seed=84)).cuda()
    for slot, seed in ((0, 7), (1, 9)):
        e.set_identity(torch.from_numpy(synth.make_identity(seed)).reshape(1, 512).cuda(), slot)
    slots = [0, 1, 0]
    chain = FrameChain(swapper_m)
    c = chain.crop(fr, torch.from_numpy(lmk_np).cuda(), fi)
    assert set(c) == {"crops", "M", "status"} and c["crops"].shape == (3, 512, 512, 3) and c["status"].cpu().tolist() == [0, 0, 0]
    assert torch.equal(c["crops"], swapper_m.crop_lmk(fr, torch.from_numpy(lmk_np).cuda(), fi)["crops"])
    got = chain(c["crops"], masks, c["M"], fr, slots=slots, frame_index=fi, status=c["status"])["frames"].clone()
    cm = tail.crop_faces_M(e, fr, _o2c64(c["M"]), fi, 512)                               # the host route, matrices taken from the device's M
    assert torch.equal(cm["crops"], c["crops"])
    want = chain(cm["crops"], masks, _c2o64(c["M"]), fr, slots=slots, frame_index=fi)["frames"]
    assert torch.equal(got, want), int((got != want).sum())
    assert not torch.equal(got[0], fr[0]) and not torch.equal(got[1], fr[1])
    per_frame = chain(c["crops"][[0, 2]], masks[[0, 2]], c["M"][[0, 2]].contiguous(), fr, slots=[0, 0])["frames"]      # frame_index None: arange(B)
    assert torch.equal(per_frame, chain(c["crops"][[0, 2]], masks[[0, 2]], _c2o64(c["M"])[[0, 2]], fr, slots=[0, 0])["frames"])
    with pytest.raises(ValueError, match="status"):
        chain(cm["crops"], masks, _c2o64(c["M"]), fr, slots=slots, frame_index=fi, status=c["status"])
    host_lmk = chain.crop(fr, lmk_np, fi)                                                # host landmarks: today's dict
    assert {"M_c2o", "M_o2c", "lmk_crop", "crops"} <= set(host_lmk) and "M" not in host_lmk


# ------------------------------------------------------------------------------------------------ no host wait
def _sync_error_mode():
    if not hasattr(torch.cuda, "set_sync_debug_mode") or not hasattr(torch._C, "_cuda_set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    torch.cuda.set_sync_debug_mode("error")


def test_tracker_crop_and_paste_are_enqueued_without_a_host_wait(engine):
    from canonswap_amd import landmarks, tail
    from test_gpu_landmarks import _gradient_frames, _seed106
    frames = torch.from_numpy(_gradient_frames(3, 135, 240)).cuda()
    tracker = landmarks.LandmarkTracker(engine, LR.standin_net(LR.loop_shape(), "cuda"))
    seed = torch.from_numpy(_seed106()).cuda()
    fi = np.repeat(np.arange(3), 2).astype(np.int32)                                     # N = 3 frames, S = 2 trajectories: frame_index of (N S)
    masks = torch.from_numpy(DR.MF._masks(np.random.Generator(np.random.PCG64(5)), 6, 16, 16)).cuda()

    def step():
        lmk, status = tracker.track(frames, seed)                                        # (N,S,Np,2), (S,)
        c = tail.crop_lmk(engine, frames, lmk.reshape(6, -1, 2), fi, dsize=16, **CFG)
        return lmk, c, tail.paste_back_faces_dev(engine, c["crops"], masks, c["M"], fi, frames, status=c["status"])

    _, _, warm = step()                                                                  # allocator and kernels are loaded
    torch.cuda.synchronize()
    _sync_error_mode()
    try:
        lmk, c, got = step()                                                             # any synchronising call raises here
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, warm) and c["status"].cpu().tolist() == [0] * 6 and not torch.equal(got, frames)
    want = tail.paste_back_faces(engine, c["crops"], masks, _c2o64(c["M"]), fi, frames)
    assert torch.equal(got, want)


def test_the_chains_step_by_the_device_route_is_enqueued_without_a_host_wait(swapper_m):
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    e = swapper_m.engine
    fr = _frames(2, 96, 128, seed=8)
    lmk = torch.from_numpy(np.stack([LR.synthetic_face(44, 44, 30, 5), LR.synthetic_face(80, 50, 28, -12)])).cuda()
    masks = torch.from_numpy(chain_helpers._masks(2, seed=85)).cuda()
    e.set_identity(torch.from_numpy(synth.make_identity(7)).reshape(1, 512).cuda(), 0)
    chain = FrameChain(swapper_m)

    def step():
        c = chain.crop(fr, lmk)
        return chain(c["crops"], masks, c["M"], fr, slots=[0, 0], status=c["status"])["frames"].clone()

    warm = step()
    torch.cuda.synchronize()
    _sync_error_mode()
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, warm) and not torch.equal(got, fr)
