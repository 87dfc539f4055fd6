"""Several faces per frame on the device (cs_crop_faces, cs_paste_back_faces; tail.crop_faces / crop_faces_M / paste_back_faces; chain.crop and
FrameChain with frame_index).  Face b is cut from, and pasted into, frame frame_index[b]; the paste is the reference's paste_back
(src/utils/crop.py:515-529) once per face of a frame, in order, each on the result of the one before.  Integer and fixed-order float
arithmetic, so every comparison is bit for bit: against tests/multi_face_ref.py (numpy on oracle/cv_ref.py), against sequential calls of the
single-frame kernels, and through the chain.  The scenes are small (a few hundred pixels per frame): what can go wrong - order, a frame
without a face, a face outside or over the border or over the whole frame, the launch's 48 faces, in place, odd widths - does so at any size."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_helpers
import multi_face_ref as MF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def swapper_m():
    return chain_helpers.swapper_b4(chain_helpers.motion_state_dicts())


@pytest.fixture(scope="module")
def engine(swapper_m):
    return swapper_m.engine


@pytest.fixture(scope="module")
def scene():
    """The shared scene and its reference result, computed once; nobody writes into them."""
    crops, masks, M, fi, ori = MF.scene()
    return dict(crops=crops, masks=masks, M=M, fi=fi, ori=ori, want=MF.paste_faces(crops, masks, M, fi, ori))


@pytest.fixture(scope="module")
def chunks():
    crops, masks, M, fi, ori = MF.chunk_scene()
    return dict(crops=crops, masks=masks, M=M, fi=fi, ori=ori, want=MF.paste_faces(crops, masks, M, fi, ori))


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _paste(engine, s, **kw):
    from canonswap_amd import tail
    crops, masks, ori = _dev(s["crops"], s["masks"], s["ori"])
    return tail.paste_back_faces(engine, crops, masks, s["M"], s["fi"], ori, **kw)


def _off_by_one(t):
    """The same bytes in a buffer that starts one byte off the dword grid."""
    raw = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=t.device)
    odd = raw[1:].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    return odd


# ------------------------------------------------------------------------------------------------ paste
def test_paste_equals_the_reference_and_sequential_single_frame_calls(engine, scene):
    from canonswap_amd import tail
    got = _paste(engine, scene)
    assert got.dtype == torch.uint8 and tuple(got.shape) == scene["ori"].shape
    g = got.cpu().numpy()
    for f in range(4):
        assert np.array_equal(g[f], scene["want"][f]), (f, int((g[f] != scene["want"][f]).sum()))
    assert np.array_equal(g[1], scene["ori"][1])                                        # the frame without a face: copied
    crops, masks, ori = _dev(scene["crops"], scene["masks"], scene["ori"])
    seq = [ori[f] for f in range(4)]
    for b, f in enumerate(scene["fi"]):
        seq[f] = tail.paste_back_fused(engine, crops[b], masks[b], scene["M"][b], seq[f])
    assert torch.equal(got, torch.stack(seq))
    again = tail.paste_back_faces(engine, scene["crops"], scene["masks"], scene["M"][:, :2], torch.from_numpy(scene["fi"]), scene["ori"])
    assert torch.equal(again, got)                                                      # host inputs, 2x3 matrices, a tensor for the index


def test_swapping_two_overlapping_faces_changes_the_result_as_it_changes_the_references(engine, scene):
    s = dict(scene)
    swap = np.array([1, 0, 2, 3, 4, 5])
    s.update(crops=scene["crops"][swap], masks=scene["masks"][swap], M=scene["M"][swap])
    want = MF.paste_faces(s["crops"], s["masks"], s["M"], s["fi"], s["ori"])
    got = _paste(engine, s).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[0] != scene["want"][0]).any() and np.array_equal(want[1:], scene["want"][1:])
    assert np.array_equal(got != scene["want"], want != scene["want"])


def test_more_faces_than_a_launch_takes_and_a_frame_in_two_launches(engine, chunks):
    got = _paste(engine, chunks).cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f], chunks["want"][f]), (f, int((got[f] != chunks["want"][f]).sum()))
    assert np.array_equal(got[1], chunks["ori"][1]) and not np.array_equal(got[0], chunks["ori"][0])


@pytest.mark.parametrize("which", ["scene", "chunks"])
def test_in_place(engine, scene, chunks, which):
    from canonswap_amd import tail
    s = {"scene": scene, "chunks": chunks}[which]
    crops, masks, buf = _dev(s["crops"], s["masks"], s["ori"])
    got = tail.paste_back_faces(engine, crops, masks, s["M"], s["fi"], buf, out=buf)
    assert got is buf and np.array_equal(buf.cpu().numpy(), s["want"])


def test_no_face_at_all_copies_the_frames(engine, scene):
    from canonswap_amd import tail
    ori = _dev(scene["ori"][:2])[0]
    none = torch.empty((0, 16, 16, 3), dtype=torch.uint8, device=ori.device)
    out = torch.full_like(ori, 7)
    got = tail.paste_back_faces(engine, none, none[..., 0].float(), np.zeros((0, 3, 3)), [], ori, out=out)
    assert got is out and torch.equal(out, ori)
    assert torch.equal(tail.paste_back_faces(engine, none, none[..., 0].float(), None, np.zeros(0, np.int32), ori), ori)
    keep = ori.clone()
    assert tail.paste_back_faces(engine, none, none[..., 0].float(), None, [], ori, out=ori) is ori and torch.equal(ori, keep)      # in place: untouched


def test_one_face_per_frame_is_paste_back_batch(engine, scene):
    from canonswap_amd import tail
    pick = [0, 2, 3, 5]                                                                  # a face inside, the turned one, the one outside, the one over the frame
    crops, masks, ori = _dev(scene["crops"][pick], scene["masks"][pick], scene["ori"])
    M = scene["M"][pick]
    got = tail.paste_back_faces(engine, crops, masks, M, np.arange(4), ori)
    assert torch.equal(got, tail.paste_back_batch(engine, crops, masks, M, ori))
    assert np.array_equal(got.cpu().numpy(), MF.paste_faces(scene["crops"][pick], scene["masks"][pick], M, np.arange(4), scene["ori"]))


def test_odd_width_and_buffers_off_the_dword_grid_give_the_same_bits(engine, scene):
    """Wo % 4 != 0, or imgs_ori / out one byte off a 4-byte boundary: the same launches, one pixel per thread (paste_faces_kernel<1>)."""
    from canonswap_amd import tail
    r = np.random.Generator(np.random.PCG64(9))
    ori_np = r.integers(0, 256, size=(4, 23, 37, 3), dtype=np.uint8)
    want = MF.paste_faces(scene["crops"], scene["masks"], scene["M"], scene["fi"], ori_np)
    crops, masks, ori = _dev(scene["crops"], scene["masks"], ori_np)
    got = tail.paste_back_faces(engine, crops, masks, scene["M"], scene["fi"], ori)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want[1], ori_np[1])
    buf = ori.clone()
    assert tail.paste_back_faces(engine, crops, masks, scene["M"], scene["fi"], buf, out=buf) is buf and np.array_equal(buf.cpu().numpy(), want)
    ori36 = _dev(scene["ori"])[0]
    for src, dst in ((_off_by_one(ori36), None), (ori36, _off_by_one(torch.zeros_like(ori36))), (_off_by_one(ori36), "same")):
        out = src if dst == "same" else dst
        got = tail.paste_back_faces(engine, crops, masks, scene["M"], scene["fi"], src, out=out)
        assert (out is None or got is out) and np.array_equal(got.cpu().numpy(), scene["want"])


def test_a_frame_in_two_launches_off_the_dword_grid(engine, chunks):
    """paste_faces_kernel<1> across a launch boundary with resume: the 70 faces of `chunks`, imgs_ori and out one byte off the dword grid, out of
    place and in place."""
    from canonswap_amd import tail
    crops, masks, ori = _dev(chunks["crops"], chunks["masks"], chunks["ori"])
    src, out = _off_by_one(ori), _off_by_one(torch.zeros_like(ori))
    assert tail.paste_back_faces(engine, crops, masks, chunks["M"], chunks["fi"], src, out=out) is out
    assert np.array_equal(out.cpu().numpy(), chunks["want"]) and torch.equal(src, ori)
    assert tail.paste_back_faces(engine, crops, masks, chunks["M"], chunks["fi"], src, out=src) is src
    assert np.array_equal(src.cpu().numpy(), chunks["want"])


def test_paste_back_batch_of_an_odd_width_over_two_chunks_of_matrices(engine):
    """paste_batch_kernel<1> across the 64 matrices of a launch: 66 frames of 10 x 13 (Wo % 4 = 1), 8 x 8 crops, one face per frame."""
    from canonswap_amd import tail
    r = np.random.Generator(np.random.PCG64(17))
    B, Ho, Wo, Hc, Wc = 66, 10, 13, 8, 8
    M = np.stack([MF.similarity(r.uniform(0.6, 1.6), r.uniform(-0.8, 0.8), r.uniform(-3, 6), r.uniform(-3, 4)) for _ in range(B)])
    crops, masks, ori = MF._bytes(r, (B, Hc, Wc, 3)), MF._masks(r, B, Hc, Wc), MF._bytes(r, (B, Ho, Wo, 3))
    want = MF.paste_faces(crops, masks, M, np.arange(B), ori)
    got = tail.paste_back_batch(engine, *_dev(crops, masks), M, _dev(ori)[0]).cpu().numpy()
    assert np.array_equal(got, want), [b for b in range(B) if not np.array_equal(got[b], want[b])]
    assert (want[0] != ori[0]).any() and (want[65] != ori[65]).any()


# ------------------------------------------------------------------------------------------------ crop
def _crop_case(B_index, Ho=20, Wo=28, zoom=1.0, seed=11):
    r = np.random.Generator(np.random.PCG64(seed))
    F = max(B_index) + 1
    frames = r.integers(0, 256, size=(F, Ho, Wo, 3), dtype=np.uint8)
    # frame -> crop: the inverse of a crop -> frame placement; the last face looks over the frame's corner (zero border)
    M = np.stack([np.linalg.inv(MF.similarity(r.uniform(0.8, 1.4) / zoom, r.uniform(-0.7, 0.7), r.uniform(2, 12), r.uniform(1, 8))) for _ in B_index])
    M[-1] = np.linalg.inv(MF.similarity(1.2 / zoom, 0.4, -3.5, -2.25))
    return frames, M, np.asarray(B_index, np.int32)


@pytest.mark.parametrize("dsize", [8, 12])
def test_crops_equal_the_reference_and_crop_frames_on_the_gathered_frames(engine, dsize):
    from canonswap_amd import tail
    frames, M, fi = _crop_case([0, 0, 1, 1, 1])
    fr = torch.from_numpy(frames).cuda()
    got = tail.crop_faces_M(engine, fr, M, fi, dsize)
    assert set(got) == {"crops"} and tuple(got["crops"].shape) == (5, dsize, dsize, 3)
    want = MF.crop_faces(frames, M, fi, dsize)
    assert np.array_equal(got["crops"].cpu().numpy(), want)
    assert torch.equal(got["crops"], tail.crop_frames_M(engine, fr[torch.from_numpy(fi).long().cuda()], M, dsize)["crops"])
    assert not np.array_equal(want[1], want[2]) and (want[4] == 0).any() and want[4].any()
    odd = _off_by_one(torch.zeros_like(got["crops"]))                                   # a crop buffer off the dword grid: the same launch, narrow stores
    assert tail.crop_faces_M(engine, fr, M, fi, dsize, out=odd)["crops"] is odd and torch.equal(odd, got["crops"])


def test_narrow_stores_over_two_chunks_of_matrices(engine):
    """66 faces at dsize 8 into a crop buffer one byte off the dword grid: crop_store<0, false> across the 64 matrices of a launch."""
    from canonswap_amd import tail
    frames, M, fi = _crop_case(sorted(list(range(5)) * 13 + [4]))
    assert len(fi) == 66
    fr = torch.from_numpy(frames).cuda()
    want = tail.crop_faces_M(engine, fr, M, fi, 8)["crops"]
    odd = _off_by_one(torch.zeros_like(want))
    assert tail.crop_faces_M(engine, fr, M, fi, 8, out=odd)["crops"] is odd and torch.equal(odd, want)
    assert np.array_equal(odd.cpu().numpy(), MF.crop_faces(frames, M, fi, 8))
    assert not torch.equal(odd[63], odd[64]) and odd[65].any()


@pytest.mark.parametrize("dsize", [256, 512])
def test_fused_staging_under_the_index(engine, dsize):
    """want_I with two crops of one frame - the first frame's, then the second's: I == prepare_crops(crops), the crops those of a launch without I."""
    from canonswap_amd import tail
    for index in ([0, 0], [1, 1]):
        frames, M, fi = _crop_case(index, zoom=dsize / 16.0, seed=13 + index[0])
        fr = torch.from_numpy(frames).cuda()
        got = tail.crop_faces_M(engine, fr, M, fi, dsize, want_I=True)
        assert tuple(got["I"].shape) == (2, 3, 256, 256) and got["I"].dtype == torch.float32
        assert torch.equal(got["I"], tail.prepare_crops(engine, got["crops"]))
        assert torch.equal(got["crops"], tail.crop_faces_M(engine, fr, M, fi, dsize)["crops"])
        assert torch.equal(got["crops"], tail.crop_frames_M(engine, fr[torch.tensor(index).cuda()], M, dsize)["crops"])
        assert got["crops"].float().std().item() > 10 and not torch.equal(got["crops"][0], got["crops"][1])
        odd = _off_by_one(torch.zeros_like(got["crops"]))
        res = tail.crop_faces_M(engine, fr, M, fi, dsize, out=odd, want_I=True)
        assert torch.equal(odd, got["crops"]) and torch.equal(res["I"], got["I"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_arguments_launch_nothing(engine, scene):
    """The C entry points refuse before any launch: nonzero, cs_last_error set, the output (pre-filled with a pattern) unchanged; tail refuses
    the same on the host, naming the argument."""
    from canonswap_amd import _lib, tail
    from canonswap_amd.engine import _ptr
    e, lib = engine, engine.lib
    crops, masks, ori = _dev(scene["crops"], scene["masks"], scene["ori"])
    B, F, (Ho, Wo) = 6, 4, ori.shape[1:3]
    out = torch.full_like(ori, 0x5a)
    M, mp = tail._m6(scene["M"], B)
    ip = lambda idx: (C.c_int * len(idx))(*idx)
    good = ip(scene["fi"].tolist())

    def paste(B=B, F=F, crops=crops, masks=masks, index=good, mp=mp, ori=ori, out=out):
        return lib.cs_paste_back_faces(e.h, B, F, _ptr(crops), _ptr(masks), 16, 16, index, mp, _ptr(ori), _ptr(out), Ho, Wo, e._stream().cuda_stream)

    cases = [dict(crops=None), dict(masks=None), dict(index=None), dict(mp=None), dict(ori=None), dict(F=0), dict(B=-1),
             dict(index=ip([0, 0, 2, 2, 2, 4])), dict(index=ip([0, 0, 2, 2, 2, -1])), dict(index=ip([0, 0, 2, 1, 2, 3])), dict(F=3)]
    for kw in cases:
        assert paste(**kw) != 0, kw
        assert b"cs_paste_back_faces" in lib.cs_last_error(), kw
    assert paste(out=None) != 0
    assert paste(index=ip([0, 0, 2, 1, 2, 3])) != 0 and b"decreases" in lib.cs_last_error()
    assert paste(index=ip([0, 0, 2, 2, 2, 4])) != 0 and b"outside [0, 4)" in lib.cs_last_error()

    frames = ori
    co = torch.full((B, 8, 8, 3), 0x5a, dtype=torch.uint8, device=ori.device)
    Io = torch.full((B, 3, 256, 256), -3.0, device=ori.device)

    def crop(B=B, F=F, frames=frames, index=good, mp=mp, dsize=8, out=co, I=None):
        return lib.cs_crop_faces(e.h, B, F, _ptr(frames), Ho, Wo, index, mp, dsize, _ptr(out), _ptr(I), e._stream().cuda_stream)

    for kw in [dict(frames=None), dict(index=None), dict(mp=None), dict(out=None), dict(F=0), dict(B=0), dict(B=-2), dict(F=3),
               dict(index=ip([0, 0, 2, 2, 2, 4])), dict(index=ip([1, 0, 2, 2, 2, 3])), dict(dsize=6), dict(dsize=0), dict(dsize=16388), dict(I=Io)]:
        assert crop(**kw) != 0, kw
        assert b"cs_crop_faces" in lib.cs_last_error(), kw
    assert crop(I=Io) != 0 and b"256 or 512" in lib.cs_last_error()
    torch.cuda.synchronize()
    assert (out == 0x5a).all() and (co == 0x5a).all() and (Io == -3.0).all()            # nothing was launched

    for bad in ([0, 0, 2, 1, 2, 3], [0, 0, 2, 2, 2, 4], [0, 0, 2, 2, 2], np.array(scene["fi"], np.float32)):
        with pytest.raises(ValueError, match="frame_index"):
            tail.paste_back_faces(e, crops, masks, scene["M"], bad, ori, out=out)
        with pytest.raises(ValueError, match="frame_index"):
            tail.crop_faces_M(e, frames, scene["M"], bad, 8, out=co)
    with pytest.raises(ValueError):
        tail.paste_back_faces(e, crops, masks[:5], scene["M"], scene["fi"], ori)
    with pytest.raises(ValueError):
        tail.paste_back_faces(e, crops, masks, scene["M"][:5], scene["fi"], ori)
    with pytest.raises(ValueError):
        tail.paste_back_faces(e, crops, masks, scene["M"], scene["fi"], ori, out=out[:3])
    with pytest.raises(ValueError):
        tail.paste_back_faces(e, crops.float(), masks, scene["M"], scene["fi"], ori)
    with pytest.raises(ValueError):
        tail.crop_faces_M(e, frames, scene["M"].reshape(B, 9), scene["fi"], 8)
    with pytest.raises(RuntimeError, match="dsize 6"):
        tail.crop_faces_M(e, frames, scene["M"], scene["fi"], 6, out=torch.full((B, 6, 6, 3), 0x5a, dtype=torch.uint8, device=ori.device))
    torch.cuda.synchronize()
    assert (out == 0x5a).all() and (co == 0x5a).all()
    assert paste() == 0                                                                 # and the accepted call still runs
    assert np.array_equal(out.cpu().numpy(), scene["want"])


# ------------------------------------------------------------------------------------------------ through the chain
def _chain_scene():
    """F = 3 frames of 96 x 128, four faces: two in frame 0, none in frame 1, two in frame 2."""
    from test_gpu_crop import _face
    r = np.random.Generator(np.random.PCG64(81))
    F, Ho, Wo = 3, 96, 128
    yy, xx = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    frames = np.empty((F, Ho, Wo, 3), np.uint8)
    for f in range(F):
        for c in range(3):
            frames[f, :, :, c] = (127.5 + 80 * np.sin(xx / (9 + 3 * c + 2 * f) + f) * np.cos(yy / (7 + 2 * c) + c) + 40 * np.sin((xx + yy) / (21 + 5 * f))).clip(0, 255)
    centres = [(40, 44), (84, 50), (46, 52), (90, 40)]
    lmk = np.stack([_face(r, c, 26.0, r.uniform(-0.4, 0.4)) for c in centres])
    return frames, lmk, np.array([0, 0, 2, 2], np.int32)


def test_frame_chain_with_a_frame_index(swapper_m):
    """chain.crop(frames, lmk, frame_index=) feeds chain(..., frame_index=): the generator does not see the index (crops_out is that of the same
    call on four duplicated frames), "frames" is paste_back_faces of the kept stages, the frame without a face is its original - in line and with
    prefetch; without frame_index the chain still pastes with paste_back_batch; no face at all gives the frames back."""
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import FrameChain
    e = swapper_m.engine
    frames, lmk, fi = _chain_scene()
    fr = torch.from_numpy(frames).cuda()
    gather = torch.from_numpy(fi).long().cuda()
    masks = torch.from_numpy(chain_helpers._masks(4, seed=82)).cuda()
    a, b = torch.from_numpy(synth.make_identity(7)).reshape(1, 512), torch.from_numpy(synth.make_identity(9)).reshape(1, 512)
    ids = torch.cat([a, b, b, a]).cuda()                                                # two identities, two slots, one launch
    chain = FrameChain(swapper_m)
    c = chain.crop(fr, lmk, frame_index=fi)
    plain = chain.crop(fr[gather], lmk)
    assert torch.equal(c["crops"], plain["crops"]) and np.array_equal(c["M_c2o"], plain["M_c2o"]) and c["crops"].shape == (4, 512, 512, 3)
    assert torch.equal(swapper_m.crop_faces(fr, lmk, fi)["crops"], c["crops"])

    res = chain(c["crops"], masks, c["M_c2o"], fr, ids, keep=True, frame_index=fi)
    got, gen, soft = res["frames"].clone(), res["crops_out"].clone(), res["soft_mask"].clone()
    assert got.shape == fr.shape
    dup = chain(c["crops"], masks, c["M_c2o"], fr[gather], ids, keep=True)              # frame_index=None: what it returned before
    assert dup["frames"].shape == (4, 96, 128, 3)
    assert torch.equal(dup["crops_out"], gen) and torch.equal(dup["soft_mask"], soft)
    assert torch.equal(dup["frames"], tail.paste_back_batch(e, dup["crops_out"], dup["soft_mask"], c["M_c2o"], fr[gather]))
    assert not torch.equal(gen[0], gen[3])
    assert torch.equal(got, tail.paste_back_faces(e, gen, soft, c["M_c2o"], fi, fr))
    assert torch.equal(got, swapper_m.paste_back_faces(gen, soft, c["M_c2o"], fi, fr))
    assert torch.equal(got[1], fr[1]) and not torch.equal(got[0], fr[0]) and not torch.equal(got[2], fr[2])

    chain.prefetch(c["crops"], masks)
    out = torch.zeros_like(fr)
    pre = chain(c["crops"], masks, c["M_c2o"], fr, ids, keep=True, frame_index=fi, out=out)
    assert not chain._pending and pre["frames"] is out
    torch.cuda.synchronize()
    assert torch.equal(out, got) and torch.equal(pre["crops_out"], gen)

    with pytest.raises(ValueError, match="frame_index"):
        chain(c["crops"], masks, c["M_c2o"], fr, ids, frame_index=[0, 2, 0, 2])
    nobody = torch.empty((0, 512, 512, 3), dtype=torch.uint8, device=fr.device)
    assert torch.equal(chain(nobody, None, None, fr, frame_index=[])["frames"], fr)
    out.fill_(3)
    assert chain(nobody, None, None, fr, frame_index=[], out=out)["frames"] is out and torch.equal(out, fr)
