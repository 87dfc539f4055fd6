"""The crop on the device (cs_crop_frames; tail.crop_frames / crop_frames_M; chain.crop): crop_image's image step (src/utils/crop.py:429-455,
called per frame by src/utils/cropper.py:196-204) for B frames in one launch.  Integer arithmetic throughout, so every comparison is bit
for bit: against oracle/cv_ref.py's restatement of cv2.warpAffine, against cs_prepare_crops for the fused staging, and through both chains."""
import numpy as np
import pytest
import torch

import chain_helpers
from chain_helpers import _masks

pytestmark = pytest.mark.gpu

CROPPER = dict(dsize=512, scale=2.3, vy_ratio=-0.125)          # CropConfig (src/config/crop_config.py:21-26)
RUNNER = dict(dsize=224, scale=1.5, vy_ratio=-0.1)             # crop_image's defaults = the landmark runner's crop (human_landmark_runner.py:62)


@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


@pytest.fixture(scope="module")
def engine(swapper_m):
    return swapper_m.engine


def _face(r, centre, width, roll):
    """106 float32 landmarks of a face of `width` pixels about `centre`, rolled by `roll`: a cloud in the face's ellipse, eyes and lips where
    the 106-point layout reads them."""
    from canonswap_amd.crop import EYE_LIP_POINTS
    rad, ang = np.sqrt(r.uniform(0, 1, 106)), r.uniform(0, 2 * np.pi, 106)
    p = np.stack([0.5 * width * rad * np.cos(ang), 0.65 * width * rad * np.sin(ang)], axis=1)
    left, right, lips = EYE_LIP_POINTS[106]
    for idx, (x, y) in ((left, (-0.22, -0.2)), (right, (0.22, -0.2)), (lips[:1], (-0.17, 0.35)), (lips[1:], (0.17, 0.35))):
        for i in idx:
            p[i] = np.array([x, y]) * width + r.uniform(-0.03, 0.03, 2) * width
    c, s = np.cos(roll), np.sin(roll)
    return (p @ np.array([[c, s], [-s, c]]) + np.asarray(centre)).astype(np.float32)


def _faces(B, Ho, Wo, seed):
    """Frame 0: a face well inside; frame 1 (if any): its box leaves the frame at the top and at the left; frame 2: a box entirely outside
    the frame; the rest: anywhere inside, any roll."""
    r = np.random.Generator(np.random.PCG64(seed))
    out = []
    for b in range(B):
        w = r.uniform(0.12, 0.2) * Wo
        if b == 1:
            out.append(_face(r, (0.03 * Wo, 0.05 * Ho), w, 0.3))
        elif b == 2:
            out.append(_face(r, (-1.5 * Wo, 2.5 * Ho), w, -0.2))
        else:
            out.append(_face(r, (r.uniform(0.25, 0.75) * Wo, r.uniform(0.3, 0.7) * Ho), w, r.uniform(-0.6, 0.6)))
    return np.stack(out)


def _frames(B, Ho, Wo, seed):
    """Seeded noise frames; the first one smooth (slopes and waves, as a decoded picture is)."""
    r = np.random.Generator(np.random.PCG64(seed))
    f = r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    for c in range(3):
        f[0, :, :, c] = (127.5 + 90 * np.sin(xx / (37 + 11 * c) + c) * np.cos(yy / (29 + 7 * c)) + 37 * (xx / Wo - yy / Ho)).clip(0, 255).astype(np.uint8)
    return f


def _check_against_oracle(res, frames, dsize):
    from oracle import cv_ref as R
    got = res["crops"].cpu().numpy()
    assert got.shape == (frames.shape[0], dsize, dsize, 3) and got.dtype == np.uint8
    for b in range(frames.shape[0]):
        want = R.warp_affine_u8(frames[b], res["M_o2c"][b], (dsize, dsize))
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    return got


@pytest.mark.parametrize("size,B,cfg,rot", [
    ((1080, 1920), 3, CROPPER, True), ((1080, 1920), 3, CROPPER, False), ((1080, 1920), 1, RUNNER, True), ((1080, 1920), 3, RUNNER, False),
    ((719, 1279), 3, CROPPER, True), ((719, 1279), 1, CROPPER, False), ((719, 1279), 3, RUNNER, True),
], ids=["1080p-3-512-rot", "1080p-3-512", "1080p-1-224-rot", "1080p-3-224", "odd-3-512-rot", "odd-1-512", "odd-3-224-rot"])
def test_crops_equal_the_oracle(engine, size, B, cfg, rot):
    """crops[b] == cv_ref.warp_affine_u8(frame[b], M_o2c[b], (dsize, dsize)): a face inside, a box that leaves the frame on two sides (zero
    border), a box entirely outside (all zeros); the matrices are crop.crop_matrices'."""
    from canonswap_amd import crop, tail
    Ho, Wo = size
    frames, lmk = _frames(B, Ho, Wo, 51), _faces(B, Ho, Wo, 52)
    res = tail.crop_frames(engine, torch.from_numpy(frames).cuda(), lmk, flag_do_rot=rot, **cfg)
    M_o2c, M_c2o, lmk_crop = crop.crop_matrices(lmk, flag_do_rot=rot, **cfg)
    assert np.array_equal(res["M_o2c"], M_o2c) and np.array_equal(res["M_c2o"], M_c2o) and np.array_equal(res["lmk_crop"], lmk_crop)
    assert res["M_o2c"].shape == (B, 3, 3) and res["M_c2o"].shape == (B, 3, 3) and res["lmk_crop"].shape == (B, 106, 2) and "I" not in res
    if rot:
        assert abs(res["M_o2c"][0, 0, 1]) > 1e-3                                       # a turned crop indeed
    got = _check_against_oracle(res, frames, cfg["dsize"])
    assert got[0].min() < got[0].max()
    if B == 3:
        border = got[1] == 0
        assert border[:8, :8].all() and not border[-64:, -64:].all()                    # the corner outside the frame is the border value
        assert not got[2].any()                                                         # nothing of the frame under this box


def test_seventy_frames_cross_the_chunk_of_64(engine):
    """B = 70 > the 64 matrices of one launch (and > the engine's max_batch of 4, which does not bind this call): every frame its own face and
    its own noise, all against the oracle."""
    from canonswap_amd import tail
    B, Ho, Wo = 70, 719, 1279
    frames, lmk = _frames(B, Ho, Wo, 53), _faces(B, Ho, Wo, 54)
    res = tail.crop_frames(engine, torch.from_numpy(frames).cuda(), lmk)
    got = _check_against_oracle(res, frames, 512)
    assert len({got[b].tobytes() for b in range(B)}) == B                                # every frame its own crop (one of them all zeros)
    one = tail.crop_frames(engine, torch.from_numpy(frames[66:67]).cuda(), lmk[66])      # (N,2) landmarks for one frame
    assert np.array_equal(one["crops"].cpu().numpy()[0], got[66])


def test_seventy_frames_at_1080p(engine):
    """The same at the size the pipeline runs, 224-pixel crops of 70 1080p frames (two seeded noise frames, repeated)."""
    from canonswap_amd import tail
    B, Ho, Wo = 70, 1080, 1920
    two = _frames(2, Ho, Wo, 55)
    frames = np.ascontiguousarray(two[np.arange(B) % 2])
    res = tail.crop_frames(engine, torch.from_numpy(frames).cuda(), _faces(B, Ho, Wo, 56), **RUNNER)
    _check_against_oracle(res, frames, 224)


@pytest.mark.parametrize("dsize", [512, 256])
def test_fused_staging_is_prepare_crops(engine, dsize):
    """want_I: I == prepare_crops(crops), bit for bit (2x2 means then / 255 from 512, / 255 from 256), and the crops are those of a launch without I."""
    from canonswap_amd import tail
    B, Ho, Wo = 3, 1080, 1920
    frames = torch.from_numpy(_frames(B, Ho, Wo, 57)).cuda()
    lmk = _faces(B, Ho, Wo, 58)
    res = tail.crop_frames(engine, frames, lmk, dsize=dsize, want_I=True)
    plain = tail.crop_frames(engine, frames, lmk, dsize=dsize)
    assert torch.equal(res["crops"], plain["crops"])
    assert res["I"].shape == (B, 3, 256, 256) and res["I"].dtype == torch.float32
    assert torch.equal(res["I"], tail.prepare_crops(engine, res["crops"]))
    assert 0 < res["I"][0].mean().item() < 1 and res["I"][2].abs().max().item() == 0
    buf = torch.full((B, 3, 256, 256), -1.0, device=engine.device)
    assert tail.crop_frames(engine, frames, lmk, dsize=dsize, out_I=buf)["I"] is buf and torch.equal(buf, res["I"])


def test_crop_frames_M_and_caller_buffers(engine):
    """A caller's own matrices (crop_image_mo2c): (B,3,3) and (B,2,3), float32 or float64, give crop_frames' crops; `out` is written in place;
    a crop buffer off a 4-byte boundary / an I buffer off a 16-byte one are stored byte by byte and float by float from the same launch, at
    dsize 512 (two rows per thread, the 2 x 2 means) and 256: the same bytes."""
    from canonswap_amd import tail
    B, Ho, Wo = 3, 1080, 1920
    frames = torch.from_numpy(_frames(B, Ho, Wo, 59)).cuda()
    lmk = _faces(B, Ho, Wo, 60)
    want = tail.crop_frames(engine, frames, lmk, want_I=True)
    M = want["M_o2c"]
    for m in (M, M[:, :2], M.astype(np.float64), torch.from_numpy(M)):
        got = tail.crop_frames_M(engine, frames, m, 512)
        assert set(got) == {"crops"} and torch.equal(got["crops"], want["crops"])
    out = torch.zeros((B, 512, 512, 3), dtype=torch.uint8, device=engine.device)
    assert tail.crop_frames_M(engine, frames, M, 512, out=out)["crops"] is out and torch.equal(out, want["crops"])
    for dsize, w in ((512, want), (256, tail.crop_frames(engine, frames, lmk, dsize=256, want_I=True))):
        raw = torch.zeros(B * dsize * dsize * 3 + 1, dtype=torch.uint8, device=engine.device)
        odd = raw[1:].view(B, dsize, dsize, 3)
        assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
        got = tail.crop_frames_M(engine, frames, w["M_o2c"], dsize, out=odd, want_I=True)
        assert torch.equal(odd, w["crops"]) and torch.equal(got["I"], w["I"])
        rawI = torch.zeros(B * 3 * 256 * 256 + 1, dtype=torch.float32, device=engine.device)
        oddI = rawI[1:].view(B, 3, 256, 256)
        assert oddI.data_ptr() % 16 == 4
        got = tail.crop_frames_M(engine, frames, w["M_o2c"], dsize, out_I=oddI)
        assert torch.equal(got["crops"], w["crops"]) and torch.equal(oddI, w["I"])
    host = tail.crop_frames_M(engine, frames.cpu().numpy(), M, 512)                     # host frames are uploaded, as paste_back_batch's are
    assert torch.equal(host["crops"], want["crops"])


def test_refused_arguments_launch_nothing(engine):
    from canonswap_amd import tail
    B, Ho, Wo = 2, 360, 640
    frames = torch.from_numpy(_frames(B, Ho, Wo, 61)).cuda()
    lmk = _faces(B, Ho, Wo, 62)
    M = tail.crop_frames(engine, frames, lmk)["M_o2c"]
    sentinel = lambda *shape, dtype=torch.uint8: torch.full(shape, 7, dtype=dtype, device=engine.device)
    out6 = sentinel(B, 6, 6, 3)
    with pytest.raises(RuntimeError, match="dsize 6"):                                  # not a multiple of 4
        tail.crop_frames_M(engine, frames, M, 6, out=out6)
    with pytest.raises(RuntimeError, match="dsize 10"):
        tail.crop_frames_M(engine, frames, M, 10)
    out224, I = sentinel(B, 224, 224, 3), sentinel(B, 3, 256, 256, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="256 or 512"):                               # no staging from a 224-pixel crop
        tail.crop_frames_M(engine, frames, M, 224, out=out224, out_I=I)
    with pytest.raises(RuntimeError, match="256 or 512"):
        tail.crop_frames(engine, frames, lmk, want_I=True, **RUNNER)
    torch.cuda.synchronize()
    assert (out6 == 7).all() and (out224 == 7).all() and (I == 7).all()                 # nothing was launched
    with pytest.raises(ValueError):
        tail.crop_frames(engine, frames.float(), lmk)                                   # non-uint8 frames
    with pytest.raises(ValueError):
        tail.crop_frames(engine, frames[0], lmk[0])                                     # one HxWx3 frame: pass frames[None]
    with pytest.raises(ValueError):
        tail.crop_frames(engine, frames[..., :2], lmk)
    for bad in (sentinel(B, 512, 512, 4), sentinel(B, 256, 512, 3), sentinel(B + 1, 512, 512, 3), sentinel(B, 512, 512, 3).cpu(),
                sentinel(B, 512, 512, 3, dtype=torch.int8), sentinel(B, 512, 1024, 3)[:, :, ::2]):
        with pytest.raises(ValueError):
            tail.crop_frames(engine, frames, lmk, out=bad)                              # a wrongly shaped / typed / placed / strided `out`
    with pytest.raises(ValueError):
        tail.crop_frames(engine, frames, lmk, out_I=sentinel(B, 3, 256, 256, dtype=torch.float16))
    with pytest.raises(ValueError):
        tail.crop_frames(engine, frames, lmk[:1])                                       # one landmark set for two frames
    with pytest.raises(ValueError):
        tail.crop_frames_M(engine, frames, M[:1], 512)
    with pytest.raises(ValueError):
        tail.crop_frames_M(engine, frames, M.reshape(B, 9), 512)


# ------------------------------------------------------------------------------------------------ through the chains
def _scene(B, Ho, Wo, seed):
    """Smooth frames (the motion extractor sees a picture, not noise) with a face-sized box well inside."""
    r = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    frames = np.empty((B, Ho, Wo, 3), np.uint8)
    for b in range(B):
        for c in range(3):
            frames[b, :, :, c] = (127.5 + 80 * np.sin(xx / (23 + 9 * c + 5 * b) + b) * np.cos(yy / (19 + 6 * c) + c)
                                  + 40 * np.sin((xx + yy) / (61 + 13 * b))).clip(0, 255).astype(np.uint8)
    lmk = np.stack([_face(r, (r.uniform(0.4, 0.6) * Wo, r.uniform(0.4, 0.6) * Ho), 0.16 * Wo, r.uniform(-0.4, 0.4)) for _ in range(B)])
    return frames, lmk


def _host_crops(frames, M_o2c, dsize=512):
    from oracle import cv_ref as R
    return np.stack([R.warp_affine_u8(frames[b], M_o2c[b], (dsize, dsize)) for b in range(frames.shape[0])])


def test_frame_chain_with_the_crop_in_front(swapper_m):
    """c = chain.crop(frames, lmk); chain(c["crops"], masks, c["M_c2o"], frames, id): the same bytes as the chain fed with crops cut on the
    host by the oracle under the same matrices; swapper.crop_frames is the same call."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    B, Ho, Wo = 2, 540, 960
    frames, lmk = _scene(B, Ho, Wo, 71)
    fr = torch.from_numpy(frames).cuda()
    masks = torch.from_numpy(_masks(B, seed=72)).cuda()
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    chain = FrameChain(swapper_m)
    c = chain.crop(fr, lmk)
    assert c["crops"].is_cuda and c["crops"].shape == (B, 512, 512, 3) and c["M_c2o"].shape == (B, 3, 3)
    host = _host_crops(frames, c["M_o2c"])
    assert np.array_equal(c["crops"].cpu().numpy(), host)
    again = swapper_m.crop_frames(fr, lmk)
    assert torch.equal(again["crops"], c["crops"]) and np.array_equal(again["M_c2o"], c["M_c2o"])
    got = chain(c["crops"], masks, c["M_c2o"], fr, idv)["frames"].clone()
    want = chain(torch.from_numpy(host), masks, c["M_c2o"], fr, idv)["frames"]
    assert torch.equal(got, want)
    assert not torch.equal(got, fr)                                                     # the faces were pasted in


def test_prefetch_picks_up_the_cropped_batch(swapper_m):
    """A batch prefetched from c["crops"] is found by _resolve through the tensor's identity, and gives the in-line frames."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    B, Ho, Wo = 2, 360, 640
    frames, lmk = _scene(B, Ho, Wo, 73)
    fr = torch.from_numpy(frames).cuda()
    masks = torch.from_numpy(_masks(B, seed=74)).cuda()
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    chain = FrameChain(swapper_m)
    c = chain.crop(fr, lmk)
    want = chain(c["crops"], masks, c["M_c2o"], fr, idv)["frames"].clone()
    c2 = chain.crop(fr, lmk)
    assert c2["crops"] is not c["crops"]                                                # a new tensor per call: batches may overlap
    chain.prefetch(c2["crops"], masks)
    assert len(chain._pending) == 1 and chain._pending[0][0] is c2["crops"]
    slot, staged = chain._resolve(c2["crops"], masks)
    assert slot == 0 and not chain._pending                                             # the staged batch, not an in-line stage A
    chain._release(slot)
    chain.prefetch(c2["crops"], masks)
    got = chain(c2["crops"], masks, c2["M_c2o"], fr, idv)["frames"]
    assert not chain._pending
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_animate_chain_with_the_crop_in_front(swapper_m):
    """v2i: chain.crop(img[None], lmk) -> set_source, chain.crop(driving frames) -> one batch: the same bytes as with the oracle's host crops."""
    from canonswap_amd import synth
    from canonswap_amd.chain import AnimateChain
    B, Ho, Wo = 2, 540, 960
    img, lmk_s = _scene(1, Ho, Wo, 75)
    drv, lmk_d = _scene(B, 360, 640, 76)
    mask = torch.from_numpy(_masks(1, seed=77)[0]).cuda()
    idv = torch.from_numpy(synth.make_identity(9)).cuda()
    chain = AnimateChain(swapper_m)
    s = chain.crop(torch.from_numpy(img).cuda(), lmk_s)
    d = chain.crop(torch.from_numpy(drv).cuda(), lmk_d)
    host_s, host_d = _host_crops(img, s["M_o2c"]), _host_crops(drv, d["M_o2c"])
    assert np.array_equal(s["crops"].cpu().numpy(), host_s) and np.array_equal(d["crops"].cpu().numpy(), host_d)
    chain.set_source(s["crops"][0], mask, s["M_c2o"][0], torch.from_numpy(img[0]).cuda(), idv)
    got = chain(d["crops"])["frames"].clone()
    chain.prefetch(d["crops"])
    assert chain._pending[0][0] is d["crops"]
    assert torch.equal(chain(d["crops"])["frames"], got) and not chain._pending
    chain.set_source(torch.from_numpy(host_s[0]), mask, s["M_c2o"][0], torch.from_numpy(img[0]).cuda(), idv)
    want = chain(torch.from_numpy(host_d))["frames"]
    assert got.shape == (B, Ho, Wo, 3) and torch.equal(got, want)
    assert not torch.equal(got[0], torch.from_numpy(img[0]).cuda())
