"""The landmark runner's two sides on the device (cs_lmk_input, cs_lmk_decode; landmarks.lmk_input / lmk_decode / LandmarkTracker / Landmark106).

Bounds, none taken from what the code gives:
* geometry: err(X) = the largest distance in pixels between X p and the float64 evaluation's F p (tests/landmarks_ref.py), p over the landmarks and
  the crop's four corners for M_o2c, over the crop's corners for M_c2o.  err(device) <= 4 x err(reference) per matrix kind, the maximum over the
  set: the project's parity margin.  The reference is the golden matrices on the golden sets, crop.crop_matrices on the synthetic.
* image: with the device's own M_o2c read back and widened to double, inp and crops are bit-equal to cs_crop_faces' crop (/ 255 in IEEE float32).
* decode: against float64 on the same fp32 inputs, |d| <= 4 x 2^-24 x (|x m00| + |y m01| + |m02|) per coordinate: a term passes through four
  roundings at most.
Non-finite landmarks are exercised on the host build only (tests/test_landmarks_cpu.py), never here.  Shapes are the smallest that still take
every path: N not a multiple of 64, B = 1, 3 and 65 (two launches of 64 faces), frames of odd size, dsize 224, 8 and 12."""
import os

import numpy as np
import pytest
import torch

import landmarks_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "crop_geometry.npz"))
RUNNER = dict(dsize=224, scale=1.5, vy_ratio=-0.1, flag_do_rot=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cfg(c):
    dsize, scale, vy, rot = GOLD[f"{c}_cfg"]
    return dict(dsize=int(dsize), scale=float(scale), vy_ratio=float(vy), flag_do_rot=bool(rot))


@pytest.fixture(scope="module")
def engine():
    from canonswap_amd.engine import Engine
    e = Engine(0, max_batch=1)           # neither call needs weights, scratch or a batch limit
    yield e
    e.close()


def _gradient_frames(F, Ho, Wo):
    """Distinct smooth frames (a slope below one grey level per pixel, no wrap): a step that reads the wrong frame shows."""
    y, x = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    out = np.empty((F, Ho, Wo, 3), np.uint8)
    for f in range(F):
        for c in range(3):
            out[f, :, :, c] = np.clip(20 + 10 * f + 5 * c + x * (0.2 + 0.1 * f) + y * (0.5 - 0.08 * f), 0, 255).astype(np.uint8)
    return out


def _noise_frames(F, Ho, Wo, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (F, Ho, Wo, 3), dtype=np.uint8)


def _split(M):
    M = M.cpu().numpy()
    return M[:, :9].reshape(-1, 3, 3), M[:, 9:].reshape(-1, 3, 3)


# ------------------------------------------------------------------------------------------------ geometry
def test_geometry_on_the_references_own_vectors(engine):
    from canonswap_amd import landmarks
    frames = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    worst = np.zeros(4)          # device o2c, c2o; reference o2c, c2o
    for k in map(str, GOLD["sets"]):
        for c in map(str, GOLD["configs"]):
            lmk, cfg = GOLD[f"{k}_lmk"], _cfg(c)
            res = landmarks.lmk_input(engine, frames, lmk[None].astype(np.float32), **cfg)
            assert int(res["status"][0]) == 0, (k, c)
            M_o2c, M_c2o = _split(res["M"])
            assert np.array_equal(M_o2c[0, 2], [0, 0, 1]) and np.array_equal(M_c2o[0, 2], [0, 0, 1])
            d = LR.geometry_errors(M_o2c[0], M_c2o[0], lmk, **cfg)
            r = LR.geometry_errors(GOLD[f"{k}_{c}_M_o2c"], GOLD[f"{k}_{c}_M_c2o"], lmk, **cfg)
            worst = np.maximum(worst, [d[0], d[1], r[0], r[1]])
    print(f"golden sets: device M_o2c {worst[0]:.3e} px, M_c2o {worst[1]:.3e} px; reference M_o2c {worst[2]:.3e} px, M_c2o {worst[3]:.3e} px")
    assert worst[0] <= 4 * worst[2] and worst[1] <= 4 * worst[3], worst


def _synthetic_faces():
    """65 faces of 203 points in a 1080p frame: the named hard ones first, then a seeded spread."""
    faces = [LR.synthetic_face(960, 540, 400, 170), LR.synthetic_face(700, 300, 400, -170), LR.synthetic_face(500.3, 500.7, 3, 12),
             LR.synthetic_face(960, 540, 3000, -7), LR.synthetic_face(-2500, 3000, 250, 33)]
    rng = np.random.default_rng(11)
    while len(faces) < 65:
        faces.append(LR.synthetic_face(rng.uniform(0, 1920), rng.uniform(0, 1080), rng.uniform(20, 900), rng.uniform(-180, 180), seed=len(faces)))
    return np.stack(faces)


def test_geometry_on_synthetic_faces_at_one_three_and_sixtyfive(engine):
    from canonswap_amd import crop, landmarks
    faces = _synthetic_faces()
    frames = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    worst = np.zeros(4)
    for c in map(str, GOLD["configs"]):
        cfg = _cfg(c)
        ref_o2c, ref_c2o, _ = crop.crop_matrices(faces, **cfg)
        per_B = {}
        for B in (1, 3, 65):
            res = landmarks.lmk_input(engine, frames, faces[:B], [0] * B, **cfg)
            assert not res["status"].cpu().numpy().any(), (c, B)
            per_B[B] = _split(res["M"])
            for b in range(B):
                d = LR.geometry_errors(per_B[B][0][b], per_B[B][1][b], faces[b], **cfg)
                worst[:2] = np.maximum(worst[:2], d)
        for b in range(65):
            worst[2:] = np.maximum(worst[2:], LR.geometry_errors(ref_o2c[b], ref_c2o[b], faces[b], **cfg))
        for B in (1, 3):             # a face's matrices do not depend on the batch it is part of
            assert np.array_equal(_bits(per_B[B][0]), _bits(per_B[65][0][:B])) and np.array_equal(_bits(per_B[B][1]), _bits(per_B[65][1][:B]))
    print(f"synthetic faces: device M_o2c {worst[0]:.3e} px, M_c2o {worst[1]:.3e} px; reference M_o2c {worst[2]:.3e} px, M_c2o {worst[3]:.3e} px")
    assert worst[0] <= 4 * worst[2] and worst[1] <= 4 * worst[3], worst


# ------------------------------------------------------------------------------------------------ image
@pytest.mark.parametrize("hw", [(270, 480), (271, 479)])
@pytest.mark.parametrize("dsize", [224, 8, 12])
def test_input_and_crop_equal_cs_crop_faces_on_the_devices_own_matrix(engine, hw, dsize):
    from canonswap_amd import landmarks, tail
    Ho, Wo = hw
    frames = torch.from_numpy(_noise_frames(3, Ho, Wo)).cuda()
    faces = np.stack([LR.synthetic_face(240, 135, 120, 15), LR.synthetic_face(5, 130, 90, -40), LR.synthetic_face(470, 265, 150, 100),
                      LR.synthetic_face(-2000, -2000, 100, 0), LR.synthetic_face(240, 2, 60, 179), LR.synthetic_face(100, 200, 30, -90, seed=4)])
    fi = np.array([2, 0, 0, 1, 2, 0], dtype=np.int32)                     # repeats, and goes backwards
    res = landmarks.lmk_input(engine, frames, faces, fi, dsize=dsize, want_crops=True)
    assert not res["status"].cpu().numpy().any()
    M_o2c, _ = _split(res["M"])
    order = np.argsort(fi, kind="stable")                                   # cs_crop_faces takes the faces of a frame together, frames in order
    want = tail.crop_faces_M(engine, frames, M_o2c[order, :2].astype(np.float64), fi[order], dsize)["crops"].cpu().numpy()
    got_crops, got_inp = res["crops"].cpu().numpy()[order], res["inp"].cpu().numpy()[order]
    assert np.array_equal(got_crops, want), int((got_crops != want).sum())
    want_inp = want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)
    assert np.array_equal(_bits(got_inp), _bits(want_inp)), int((_bits(got_inp) != _bits(want_inp)).sum())
    outside = int(np.where(order == 3)[0][0])
    assert not want[outside].any() and want[[i for i in range(6) if i != outside]].any(axis=(1, 2, 3)).all()      # wholly outside: zeros; the others read pixels
    only_inp = landmarks.lmk_input(engine, frames, faces, fi, dsize=dsize)                                        # crops = NULL: the same inp
    assert "crops" not in only_inp and torch.equal(only_inp["inp"], res["inp"])


def test_arguments_are_refused_before_any_launch(engine):
    from canonswap_amd import _lib, landmarks
    frames = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    lmk = torch.from_numpy(LR.synthetic_face(8, 8, 6, 0)[None]).cuda()
    M, inp = torch.zeros((1, 18), device="cuda"), torch.zeros((1, 3, 8, 8), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    import ctypes as C
    fi = lambda v: (C.c_int * 1)(v)
    L = landmarks.layout_of(203)
    bad = _lib.LmkLayout(4, L.left, L.right, (C.c_int * 2)(48, 203))
    for word, args in (("dsize", (1, 2, frames, 16, 16, fi(0), lmk, 203, L, 10, 1.5, -0.1, 1, 1, M, inp, None, status)),
                       ("frame_index", (1, 2, frames, 16, 16, fi(2), lmk, 203, L, 8, 1.5, -0.1, 1, 1, M, inp, None, status)),
                       ("lip", (1, 2, frames, 16, 16, fi(0), lmk, 203, bad, 8, 1.5, -0.1, 1, 1, M, inp, None, status)),
                       ("scale", (1, 2, frames, 16, 16, fi(0), lmk, 203, L, 8, 0.0, -0.1, 1, 1, M, inp, None, status)),
                       ("status_mark", (1, 2, frames, 16, 16, fi(0), lmk, 203, L, 8, 1.5, -0.1, 1, 0, M, inp, None, status)),
                       ("NULL inp", (1, 2, frames, 16, 16, fi(0), lmk, 203, L, 8, 1.5, -0.1, 1, 1, M, None, None, status))):
        with pytest.raises(RuntimeError, match=f"cs_lmk_input.*{word}"):
            engine._call("cs_lmk_input", *args)
    with pytest.raises(RuntimeError, match="cs_lmk_decode.*Np"):
        engine._call("cs_lmk_decode", 1, inp, 0, M, 8, status, lmk)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("Np", [203, 1])
def test_decode_is_within_four_roundings_of_float64(engine, Np):
    from canonswap_amd import landmarks
    frames = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    faces = np.stack([LR.synthetic_face(960, 540, 400, 170), LR.synthetic_face(500.3, 500.7, 3, 12), LR.synthetic_face(960, 540, 3000, -7)])
    step = landmarks.lmk_input(engine, frames, faces, [0, 0, 0])
    _, M_c2o = _split(step["M"])
    pts = np.random.default_rng(5).uniform(-0.2, 1.2, (3, 2 * Np)).astype(np.float32)
    got = landmarks.lmk_decode(engine, torch.from_numpy(pts).cuda(), step["M"], status=step["status"]).cpu().numpy()
    assert got.shape == (3, Np, 2)
    worst = 0.0
    for b in range(3):
        val, mag = LR.decode64(pts[b], M_c2o[b], 224)
        ratio = np.abs(got[b].astype(np.float64) - val) / (LR.DECODE_ULPS * mag)
        worst = max(worst, float(ratio.max()))
        assert np.array_equal(_bits(got[b]), _bits(LR.decode(pts[b], M_c2o[b], 224)))       # and the bits of numpy's float32, operation by operation
    print(f"decode Np = {Np}: largest |d| / bound = {worst:.3f}")
    assert worst <= 1.0
    if Np == 203:                    # in place over the buffer the input read its landmarks from
        buf = torch.from_numpy(faces).cuda()
        step2 = landmarks.lmk_input(engine, frames, buf, [0, 0, 0])
        same = landmarks.lmk_decode(engine, torch.from_numpy(pts).cuda(), step2["M"], status=step2["status"], out=buf)
        assert same.data_ptr() == buf.data_ptr() and np.array_equal(_bits(buf.cpu().numpy()), _bits(got))


# ------------------------------------------------------------------------------------------------ guard
def test_a_refused_face_is_zeros_frozen_sticky_and_leaves_its_neighbours_alone(engine):
    from canonswap_amd import landmarks
    frames = torch.from_numpy(_noise_frames(1, 135, 240)).cuda()
    faces = np.stack([LR.synthetic_face(100, 60, 80, 20), LR.synthetic_face(120, 70, 50, 0), LR.synthetic_face(180, 90, 70, -30)])
    broken = faces.copy()
    broken[1] = [77.5, 31.25]                                              # all points equal (finite): no box
    res = landmarks.lmk_input(engine, frames, broken, [0, 0, 0], want_crops=True)
    assert res["status"].cpu().tolist() == [0, 1, 0]
    assert not res["inp"][1].any() and not res["crops"][1].any() and not res["M"][1].any()
    pair = landmarks.lmk_input(engine, frames, faces[[0, 2]], [0, 0], want_crops=True)          # a run without it
    for key in ("inp", "crops", "M"):
        assert torch.equal(res[key][[0, 2]], pair[key])
    pts = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (3, 406)).astype(np.float32)).cuda()
    lmk = torch.from_numpy(broken).cuda()
    landmarks.lmk_decode(engine, pts, res["M"], status=res["status"], out=lmk)
    out = lmk.cpu().numpy()
    assert np.array_equal(_bits(out[1]), _bits(broken[1]))                                     # frozen: what the buffer held
    assert not np.array_equal(out[0], broken[0]) and not np.array_equal(out[2], broken[2])
    # sticky: good landmarks for face 1 in a second step, under the status of the first
    again = landmarks.lmk_input(engine, frames, faces, [0, 0, 0], out={"status": res["status"]}, status_mark=2)
    assert again["status"].cpu().tolist() == [0, 1, 0] and not again["inp"][1].any() and not again["M"][1].any()
    assert torch.equal(again["inp"][[0, 2]], pair["inp"])
    fresh = landmarks.lmk_input(engine, frames, faces, [0, 0, 0])                                # without that status the face is fine
    assert fresh["status"].cpu().tolist() == [0, 0, 0] and fresh["inp"][1].any()


# ------------------------------------------------------------------------------------------------ the loop
def _seed106():
    pts = GOLD["pt106_lmk"].astype(np.float64)
    unit = (pts - pts.min(axis=0)) / (pts.max(axis=0) - pts.min(axis=0)).max()
    return np.stack([unit * 60 + [60, 35], unit * 45 + [150, 45]]).astype(np.float32)      # well inside the 240 x 135 frames


@pytest.fixture(scope="module")
def loop(engine):
    """Five hand-made steps for two trajectories, shared by the loop's tests: per step the landmarks going in, inp, M, the points, the landmarks out."""
    from canonswap_amd import landmarks
    frames = torch.from_numpy(_gradient_frames(5, 135, 240)).cuda()
    net = LR.standin_net(LR.loop_shape(), "cuda")
    prev, steps = torch.from_numpy(_seed106()).cuda(), []
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    for k in range(5):
        step = landmarks.lmk_input(engine, frames, prev, [k, k], out={"status": status}, want_crops=True)
        pts = net(step["inp"])
        new = landmarks.lmk_decode(engine, pts, step["M"], status=status)
        steps.append({"prev": prev.cpu().numpy(), "inp": step["inp"].cpu().numpy(), "crops": step["crops"].cpu().numpy(), "M": step["M"].cpu().numpy(),
                      "pts": pts.cpu().numpy(), "lmk": new.cpu().numpy()})
        prev = new
    assert status.cpu().tolist() == [0, 0]
    return {"frames": frames, "net": net, "steps": steps, "lmk": np.stack([s["lmk"] for s in steps])}


def test_track_equals_the_hand_made_steps(engine, loop):
    from canonswap_amd import landmarks
    tracker = landmarks.LandmarkTracker(engine, loop["net"])
    seed = torch.from_numpy(_seed106()).cuda()
    lmk, status = tracker.track(loop["frames"], seed)
    assert tuple(lmk.shape) == (5, 2, 203, 2) and status.cpu().tolist() == [0, 0]       # 106 points in, the network's 203 from the first step on
    assert np.array_equal(_bits(lmk.cpu().numpy()), _bits(loop["lmk"]))
    assert len({loop["lmk"][k].tobytes() for k in range(5)}) == 5                        # the frames differ, so do the steps
    a, st = tracker.track(loop["frames"][:2], seed)                                      # 2 + 3, continued from device landmarks and status
    b, st = tracker.track(loop["frames"][2:], a[-1], st)
    assert np.array_equal(_bits(torch.cat([a, b]).cpu().numpy()), _bits(loop["lmk"])) and st.cpu().tolist() == [0, 0]
    one = tracker.run(loop["frames"], seed, [0, 0])                                      # LandmarkRunner.run alone
    assert np.array_equal(_bits(one["lmk"].cpu().numpy()), _bits(loop["lmk"][0]))


def test_track_video_from_host_frames_equals_track(engine, loop):
    from canonswap_amd import landmarks
    tracker = landmarks.LandmarkTracker(engine, loop["net"])
    got = tracker.track_video(loop["frames"].cpu().numpy(), _seed106(), batch=2)        # batches of 2 + 2 + 1 through HostFrames
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(loop["lmk"]))


def test_track_enqueues_without_a_host_wait(engine, loop):
    from canonswap_amd import landmarks
    tracker = landmarks.LandmarkTracker(engine, loop["net"])
    seed = torch.from_numpy(_seed106()).cuda()
    tracker.track(loop["frames"][:1], seed)                                              # warm: allocator and kernels are loaded
    torch.cuda.synchronize()
    if not hasattr(torch.cuda, "set_sync_debug_mode") or not hasattr(torch._C, "_cuda_set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    torch.cuda.set_sync_debug_mode("error")
    try:
        lmk, status = tracker.track(loop["frames"], seed)                                # any synchronising call raises here
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(_bits(lmk.cpu().numpy()), _bits(loop["lmk"]))


def test_each_step_agrees_with_the_host_route(engine, loop):
    """Step by step from the same landmarks, so nothing accumulates: the host route is crop.crop_matrices + cs_crop_frames + numpy decode."""
    from canonswap_amd import crop, tail
    worst, routes = np.zeros(4), []
    for k, s in enumerate(loop["steps"]):
        ref_o2c, ref_c2o, _ = crop.crop_matrices(s["prev"], **RUNNER)
        M_o2c, M_c2o = s["M"][:, :9].reshape(2, 3, 3), s["M"][:, 9:].reshape(2, 3, 3)
        for b in range(2):
            worst[:2] = np.maximum(worst[:2], LR.geometry_errors(M_o2c[b], M_c2o[b], s["prev"][b], **RUNNER))
            worst[2:] = np.maximum(worst[2:], LR.geometry_errors(ref_o2c[b], ref_c2o[b], s["prev"][b], **RUNNER))
            val, mag = LR.decode64(s["pts"][b], M_c2o[b], 224)
            assert (np.abs(s["lmk"][b].astype(np.float64) - val) <= LR.DECODE_ULPS * mag).all(), (k, b)
        # the host route's image: the same frame under the host's matrices.  The two matrices agree to the geometry bound (about 1e-3 px), the
        # frames slope by less than one grey level per pixel and OpenCV's coordinates step by 1/32 px: a pixel differs by one level at most
        host = tail.crop_frames_M(engine, loop["frames"][[k, k]], ref_o2c, 224)["crops"].cpu().numpy()
        assert np.abs(host.astype(np.int32) - s["crops"].astype(np.int32)).max() <= 1, k
        host_inp = torch.from_numpy(host.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).cuda()
        host_lmk = np.stack([LR.decode(p, m, 224) for p, m in zip(loop["net"](host_inp).cpu().numpy(), ref_c2o)])
        routes.append((k, host_lmk, ref_c2o))
    print(f"loop steps: device M_o2c {worst[0]:.3e} px, M_c2o {worst[1]:.3e} px; host route M_o2c {worst[2]:.3e} px, M_c2o {worst[3]:.3e} px")
    assert worst[0] <= 4 * worst[2] and worst[1] <= 4 * worst[3], worst
    # Where the two routes' landmarks may differ: (1) one grey level in every pixel moves the stand-in's image term by 0.05 x 2 / 255 of the crop
    # at most, times the scale back to the frame; (2) on the crop's corners the host's M_c2o is within worst[3] of the float64 evaluation and the
    # device's within 4 x that (the gate just passed), so the two are at most 5 x worst[3] apart anywhere in the crop, where the points lie;
    # (3) each route's decode rounds within DECODE_ULPS x mag.  (The fp32 rounding of the stand-in's means is not allowed for.)
    for k, host_lmk, ref_c2o in routes:
        for b in range(2):
            back = np.abs(ref_c2o[b, :2, :2]).sum(axis=1).max()
            _, mag = LR.decode64(loop["steps"][k]["pts"][b], ref_c2o[b], 224)
            allowed = 224 * 0.05 * 2 / 255 * back + 5 * worst[3] + 2 * LR.DECODE_ULPS * mag.max()
            assert np.abs(host_lmk[b] - loop["steps"][k]["lmk"][b]).max() <= allowed, (k, b)


# ------------------------------------------------------------------------------------------------ the seed
def test_landmark106_seed_against_its_restatement(engine):
    from canonswap_amd import landmarks, tail
    frames = torch.from_numpy(_noise_frames(2, 135, 240, seed=9)).cuda()
    bbox = np.array([[60.5, 20.25, 140.0, 110.0], [100.0, 40.0, 230.0, 100.5]])
    size = 192
    pred = (np.random.default_rng(4).integers(-1024, 1025, (2, 212)) / 1024.0).astype(np.float32)      # on a grid: (pred + 1) * 96 is exact in fp32
    seen = {}

    def net(blob):
        seen["blob"] = blob
        return torch.from_numpy(pred).cuda()
    res = landmarks.Landmark106(engine, net, input_size=size, mean=127.5, std=128.0).get(frames, bbox, [0, 1])
    # the restatement (landmark.py:80-105), float64
    w, h = bbox[:, 2] - bbox[:, 0], bbox[:, 3] - bbox[:, 1]
    cx, cy = (bbox[:, 2] + bbox[:, 0]) / 2, (bbox[:, 3] + bbox[:, 1]) / 2
    s = size / (np.maximum(w, h) * 1.5)
    M = np.array([[[s[b], 0, size / 2 - cx[b] * s[b]], [0, s[b], size / 2 - cy[b] * s[b]]] for b in range(2)])
    assert np.array_equal(res["M"], M)
    want = tail.crop_faces_M(engine, frames, M, [0, 1], size)["crops"]
    assert torch.equal(res["crops"], want)
    blob = (want.cpu().numpy()[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) - np.float32(127.5)) * np.float32(1 / 128.0)
    assert np.array_equal(_bits(seen["blob"].cpu().numpy()), _bits(blob))
    got = res["lmk"].cpu().numpy()
    assert got.shape == (2, 106, 2)
    for b in range(2):
        IM = np.linalg.inv(np.vstack([M[b], [0, 0, 1]]))[:2].astype(np.float32).astype(np.float64)      # the fp32 matrix the device multiplies by
        xy = (pred[b].astype(np.float64).reshape(106, 2) + 1) * (size // 2)
        val = xy @ IM[:, :2].T + IM[:, 2]
        mag = np.abs(xy) @ np.abs(IM[:, :2]).T + np.abs(IM[:, 2])
        assert (np.abs(got[b].astype(np.float64) - val) <= LR.DECODE_ULPS * mag).all(), b
