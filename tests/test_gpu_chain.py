"""The whole device-side frame (canonswap_amd/chain.py; SURVEY 8f rows N1-N3 around the generator): uint8 crops ->
cs_prepare_crops -> cs_motion_extract + cs_motion_keypoints -> cs_swap_frames_ids -> cs_soft_erosion_frames -> cs_paste_back_batch -> uint8
frames.  Each batched step against the single-frame form it replaces (bit-equal) and against the oracle; the chain against the oracle's
composition of the reference's per-frame loop (can_swap_pipeline_e2e.py:223-283)."""
import numpy as np
import pytest
import torch

import chain_helpers
from chain_helpers import _affine, _masks, _occupy, _timed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


def test_keypoints_kernel_vs_oracle(swapper_m):
    """cs_motion_keypoints on raw head outputs the oracle also sees: x_t = s (kp R + exp) + t_xy, x_can = s kp, R = (Rz Ry Rx)^T."""
    from oracle import canonswap_ref as O
    r = np.random.Generator(np.random.PCG64(3))
    B = 4
    raw = r.normal(0, 1, size=(B, 328)).astype(np.float32)
    raw[:, :63] *= 0.3; raw[:, 63] = r.uniform(0.9, 1.3, B); raw[:, 262:265] *= 0.1; raw[:, 265:] *= 0.02
    raw[:, 64:262] *= 3.0                                   # peaked 66-bin pose logits
    t = torch.from_numpy(raw)
    info, o = {}, 0
    for k, n in O.M_HEADS:
        info[k] = t[:, o:o + n].clone(); o += n
    pose = [O.headpose_pred_to_degree(info[k]) for k in ("pitch", "yaw", "roll")]
    want_t = O.transform_keypoint(info)
    want_can = info["scale"][..., None] * info["kp"].reshape(B, 21, 3)
    want_R = O.get_rotation_matrix(*pose)
    x_t, x_can, R = swapper_m.engine.motion_keypoints(t.cuda(), want_rot=True)
    assert (x_t.cpu() - want_t).abs().max().item() <= 2e-6 * max(1.0, want_t.abs().max().item()) * 4
    assert torch.equal(x_can.cpu(), want_can)               # one fp32 product per element
    assert (R.cpu() - want_R).abs().max().item() <= 1e-6


def test_chain_keypoints_equal_the_torch_path(swapper_m):
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    imgs = torch.from_numpy(synth.make_smooth_images(3, seed=2000, size=256)).cuda()
    info = swapper_m.get_kp_info(imgs)
    x_t = swapper_m.transform_keypoint(info)
    x_can = info["scale"][..., None] * info["kp"]
    got_t, got_can = FrameChain(swapper_m).keypoints(imgs)
    assert (got_t - x_t).abs().max().item() <= 2e-6 and (got_can - x_can).abs().max().item() <= 1e-7


def test_soft_erosion_frames_is_b_single_calls(swapper_m):
    """Per-frame maximum (the pipeline calls the module once per frame), uint8 labels == their float copy, and equal to the batch entry
    point run one sample at a time."""
    from canonswap_amd import tail
    e = swapper_m.engine
    m = torch.from_numpy(_masks(3)).cuda()
    m[1] = 0; m[1, 250:262, 250:262] = 1                    # a tiny mask: its own maximum is far below the others'
    se = swapper_m.soft_mask(21, 0.9, 3)
    got = tail.soft_erosion_frames(e, m, se.weight, 21, 0.9, 3)
    gotf = tail.soft_erosion_frames(e, m.float(), se.weight, 21, 0.9, 3)
    assert torch.equal(got, gotf)
    for k in range(3):
        one, _ = se(m[k:k + 1, None].float())
        assert torch.equal(got[k], one[0, 0]), k
    both, _ = se(m[:, None].float())                        # the module's own batch semantics: one maximum for the whole tensor
    assert not torch.equal(both[1, 0], got[1])


def test_soft_erosion_frames_vs_oracle(swapper_m):
    from canonswap_amd import tail
    from oracle import cv_ref as R
    m = _masks(2, seed=9)
    se = swapper_m.soft_mask(21, 0.9, 3)
    got = tail.soft_erosion_frames(swapper_m.engine, torch.from_numpy(m).cuda(), se.weight, 21, 0.9, 3).cpu().numpy()
    for k in range(2):
        want, hard = R.soft_erosion(torch.from_numpy(m[k:k + 1, None].astype(np.float32)), 21, 0.9, 3)
        want, hard = want.numpy()[0, 0], hard.numpy()[0, 0]
        flips = (got[k] >= 1.0) != hard
        assert flips.sum() <= 4
        assert np.abs(got[k] - want)[~flips].max() < 2e-6


@pytest.mark.parametrize("size", [(720, 1280), (301, 403)])
def test_paste_back_batch_equals_single_frames(swapper_m, size):
    """One launch for B frames (four pixels per thread, copies outside the crop) == the single-frame kernel, which is bit-exact against
    oracle/cv_ref.py (test_gpu_tail.py); the odd width takes the same launch at one pixel per thread (paste_batch_kernel<1>)."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    Ho, Wo = size
    e = swapper_m.engine
    r = np.random.Generator(np.random.PCG64(17))
    B = 3
    crops = r.integers(0, 256, size=(B, 512, 512, 3), dtype=np.uint8)
    ori = r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    masks = np.stack([np.clip(1.2 - np.hypot(xx - 256, yy - 256) / (160 + 30 * k), 0, 1) for k in range(B)]).astype(np.float32)
    Ms = np.stack([_affine(k, Ho, Wo) for k in range(B)])
    Ms[2, 0, 2] = -150.5                                   # partly outside the frame
    got = tail.paste_back_batch(e, crops, masks, Ms, ori).cpu().numpy()
    for k in range(B):
        one = tail.paste_back_fused(e, crops[k], masks[k], Ms[k], ori[k]).cpu().numpy()
        assert np.array_equal(got[k], one), k
    mo = R.prepare_paste_back(np.stack([masks[0]] * 3, -1), Ms[0], (Wo, Ho))
    assert np.array_equal(got[0], R.paste_back(crops[0], Ms[0], ori[0], mo))


def test_chain_vs_oracle_loop(swapper_m, sds_m):
    """The chain for B = 2 frames against the oracle's composition of the reference's per-frame loop, and bit-equal to its own stages
    called one by one."""
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import FrameChain
    from oracle import canonswap_ref as O
    from oracle import cv_ref as R
    B, Ho, Wo = 2, 540, 960
    smooth = synth.make_smooth_images(B, seed=2100, size=512)                       # (B,3,512,512) in [0,1]
    crops = np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))
    masks = _masks(B, seed=21)
    r = np.random.Generator(np.random.PCG64(23))
    ori = r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)
    Ms = np.stack([_affine(k, Ho, Wo) * np.array([[0.5], [0.5], [1]]) + np.array([[0, 0, 100.], [0, 0, 20.], [0, 0, 0]]) for k in range(B)])
    idv = torch.from_numpy(synth.make_identity(7))
    chain = FrameChain(swapper_m)
    res = chain(torch.from_numpy(crops).cuda(), torch.from_numpy(masks).cuda(), Ms, torch.from_numpy(ori).cuda(), idv.cuda(), keep=True)
    got = res["frames"].cpu().numpy()
    # ---- the stages one by one: the same bits
    e = swapper_m.engine
    I = tail.prepare_crops(e, crops)
    assert torch.equal(I, res["I"])
    gen = e.swap_frames(I, res["x_t"], res["x_can"], idv.cuda(), want_f32=False, want_u8=True)["out_u8"]
    assert torch.equal(gen, res["crops_out"])
    for k in range(B):
        soft, _ = chain.se(torch.from_numpy(masks[k:k + 1, None]).cuda().float())
        one = tail.paste_back_fused(e, gen[k], soft[0, 0], Ms[k], ori[k])
        assert np.array_equal(one.cpu().numpy(), got[k]), k
    # ---- the oracle's loop
    worst = 1e9
    for k in range(B):
        with torch.no_grad():
            Ik = O.prepare_source(R.resize_area_2x_u8(crops[k]))
            info = O.get_kp_info(sds_m["motion_extractor"], Ik)
            x_t = O.transform_keypoint(info)
            x_can = info["scale"][..., None] * info["kp"]
            assert (res["x_t"][k].cpu() - x_t[0]).abs().max().item() <= 1e-4
            out = O.swap_frame(sds_m, Ik, x_t, x_can, idv)["out"]
        crop_o = O.parse_output(out)[0]
        soft, _ = R.soft_erosion(torch.from_numpy(masks[k:k + 1, None].astype(np.float32)), 21, 0.9, 3)
        soft = soft.numpy()[0, 0]
        mo = R.prepare_paste_back(np.stack([soft] * 3, -1), Ms[k], (Wo, Ho))
        want = R.paste_back(crop_o, Ms[k], ori[k], mo)
        region = mo[..., 0] > 0
        assert np.array_equal(got[k][~region], want[~region])                       # untouched pixels are the original frame
        d = got[k][region].astype(np.float64) - want[region].astype(np.float64)
        p = 10 * np.log10(255.0 ** 2 / max((d ** 2).mean(), 1e-12))
        print(f"frame {k}: pasted region {int(region.sum())} px, PSNR {p:.2f} dB, mean |diff| {np.abs(d).mean():.3f} LSB")
        worst = min(worst, p)
        assert np.abs(d).mean() < 0.6
    assert worst >= 48.0                                                           # uint8 frames: the gate of the generator's u8 output


def test_prefetched_stage_a_gives_the_same_frames(swapper_m):
    """FrameChain.prefetch: staging + M + key-points + soft masks of the next batch on a side stream (double-buffered) beside the current batch's
    generator - the same bytes as the in-line chain, batch after batch."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    B, Ho, Wo = 2, 360, 640
    r = np.random.Generator(np.random.PCG64(29))
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    batches = []
    for k in range(3):
        smooth = synth.make_smooth_images(B, seed=2200 + k, size=512)
        crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda()
        masks = torch.from_numpy(_masks(B, seed=31 + k)).cuda()
        ori = torch.from_numpy(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
        Ms = np.stack([_affine(j, Ho, Wo) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(B)])
        batches.append((crops, masks, Ms, ori))
    chain = FrameChain(swapper_m)
    want = [chain(c, m, M, o, idv)["frames"].clone() for c, m, M, o in batches]
    chain.prefetch(batches[0][0], batches[0][1])
    got = []
    for k, (c, m, M, o) in enumerate(batches):
        if k + 1 < len(batches):
            chain.prefetch(batches[k + 1][0], batches[k + 1][1])
        got.append(chain(c, m, M, o, idv)["frames"].clone())
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(want[0], want[1])
    with pytest.raises(RuntimeError):
        chain.prefetch(batches[0][0], batches[0][1]); chain.prefetch(batches[1][0], batches[1][1]); chain.prefetch(batches[2][0], batches[2][1])
    chain.drop_prefetches()


# ---- FrameChain call patterns beyond prefetch-then-hit: every result is compared byte for byte with the plain in-line chain
# on the same inputs (itself held to the oracle by test_chain_vs_oracle_loop)
def _batch(B, seed, Ho=360, Wo=640):
    from canonswap_amd import synth
    r = np.random.Generator(np.random.PCG64(seed))
    smooth = synth.make_smooth_images(B, seed=2300 + seed, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda()
    masks = torch.from_numpy(_masks(B, seed=seed)).cuda()
    ori = torch.from_numpy(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
    Ms = np.stack([_affine(j % 4, Ho, Wo) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(B)])
    return crops, masks, Ms, ori


def _inline_ms(chain, b, idv):
    a, z = _timed(), _timed()
    a.record()
    chain(*b, idv)
    z.record()
    z.synchronize()
    return a.elapsed_time(z)


@pytest.mark.parametrize("dropped", [False, True], ids=["pending", "dropped"])
def test_inline_stage_a_waits_for_a_prefetch_in_flight(swapper_m, dropped):
    """prefetch(b1), then chain(b0) with b0 never prefetched (or after drop_prefetches()): the in-line stage A uses the engine's one M and
    SoftErosion scratch, so it must run after the side stream's stage A.  The side stream is held busy (a spin of several times the
    in-line call's duration) before the prefetch is queued, so without that ordering the in-line call would end first: the end of the
    in-line call on the caller's stream must come after the prefetch's completion, and both batches must come out as in the in-line chain."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    b0, b1 = _batch(2, 41), _batch(2, 42)
    chain = FrameChain(swapper_m)
    want = [chain(*b, idv)["frames"].clone() for b in (b0, b1)]
    assert not torch.equal(want[0], want[1])
    chain.prefetch(b1[0], b1[1])                          # a first prefetch / hit pair creates the side stream
    assert torch.equal(chain(*b1, idv)["frames"], want[1])
    dt = _inline_ms(chain, b0, idv)
    _occupy(chain._side, max(40.0, 8 * dt))
    chain.prefetch(b1[0], b1[1])
    staged = _timed()
    staged.record(chain._side)                            # right behind the prefetch's `ready` event on the side stream
    if dropped:
        chain.drop_prefetches()
    got0 = chain(*b0, idv)["frames"]
    end0 = _timed()
    end0.record()
    got1 = chain(*b1, idv)["frames"]
    torch.cuda.synchronize()
    print(f"in-line call {dt:.2f} ms; its end {staged.elapsed_time(end0):.2f} ms after the prefetch's")
    assert staged.elapsed_time(end0) > 0
    assert torch.equal(got0, want[0]) and torch.equal(got1, want[1])
    assert not chain._pending


def test_prefetches_consumed_out_of_order(swapper_m):
    """prefetch(A), prefetch(B), chain(B), prefetch(C), chain(A), chain(C): C must not land in the half of the double buffer A still holds."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    A, Bt, Cc = _batch(2, 51), _batch(2, 52), _batch(2, 53)
    chain = FrameChain(swapper_m)
    want = [chain(*b, idv)["frames"].clone() for b in (A, Bt, Cc)]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(want[i], want[j]), (i, j)
    chain.prefetch(A[0], A[1])
    chain.prefetch(Bt[0], Bt[1])
    got_b = chain(*Bt, idv)["frames"]
    chain.prefetch(Cc[0], Cc[1])
    got_a = chain(*A, idv)["frames"]
    got_c = chain(*Cc, idv)["frames"]
    torch.cuda.synchronize()
    assert torch.equal(got_b, want[1])
    assert torch.equal(got_a, want[0])
    assert torch.equal(got_c, want[2])
    assert not chain._pending


def _oracle_frame(sds, crops, mask, M, ori, idv):
    """The reference's per-frame loop for one frame (can_swap_pipeline_e2e.py:223-283) composed from the oracle, as in
    test_chain_vs_oracle_loop: -> (frame, pasted region)."""
    from oracle import canonswap_ref as O
    from oracle import cv_ref as R
    Ho, Wo = ori.shape[:2]
    with torch.no_grad():
        Ik = O.prepare_source(R.resize_area_2x_u8(crops))
        info = O.get_kp_info(sds["motion_extractor"], Ik)
        x_t = O.transform_keypoint(info)
        x_can = info["scale"][..., None] * info["kp"]
        out = O.swap_frame(sds, Ik, x_t, x_can, idv)["out"]
    soft, _ = R.soft_erosion(torch.from_numpy(mask[None, None].astype(np.float32)), 21, 0.9, 3)
    mo = R.prepare_paste_back(np.stack([soft.numpy()[0, 0]] * 3, -1), M, (Wo, Ho))
    return R.paste_back(O.parse_output(out)[0], M, ori, mo), mo[..., 0] > 0


def test_latency_mode_chain_refuses_prefetch_and_runs_in_line(sds_m):
    """On a latency-mode engine every small plain conv goes through split-K on the engine's one partial-sum buffer, so M on a side stream
    beside the generator would share it: prefetch refuses before it queues anything.  The in-line chain still works there: two batches
    against the oracle's loop (the gate of test_chain_vs_oracle_loop) and equal to a fresh latency-mode chain byte for byte."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import FrameChain
    sw = can_swapper(None, state_dicts=sds_m, max_batch=1, latency_mode=True)
    idv = torch.from_numpy(synth.make_identity(7))
    b = [_batch(1, 61, 540, 960), _batch(1, 62, 540, 960)]
    chain = FrameChain(sw)
    with pytest.raises(RuntimeError, match="latency"):
        chain.prefetch(b[1][0], b[1][1])
    assert chain._side is None and not chain._pending
    got = [chain(*x, idv.cuda())["frames"].clone() for x in b]
    again = FrameChain(sw)
    for k in (1, 0):
        assert torch.equal(again(*b[k], idv.cuda())["frames"], got[k]), k
    for k, (crops, masks, Ms, ori) in enumerate(b):
        want, region = _oracle_frame(sds_m, crops[0].cpu().numpy(), masks[0].cpu().numpy(), Ms[0], ori[0].cpu().numpy(), idv)
        g = got[k][0].cpu().numpy()
        assert np.array_equal(g[~region], want[~region])
        d = g[region].astype(np.float64) - want[region].astype(np.float64)
        p = 10 * np.log10(255.0 ** 2 / max((d ** 2).mean(), 1e-12))
        print(f"latency-mode batch {k}: PSNR {p:.2f} dB, mean |diff| {np.abs(d).mean():.3f} LSB")
        assert np.abs(d).mean() < 0.6 and p >= 48.0


def test_soft_erosion_frames_beyond_64(swapper_m):
    """cs_create, cs_swap_frames and cs_paste_back_batch take up to 84 frames; so does SoftErosion (its per-(sample, block) maxima are
    sized by the batch).  84 frames in one call == 84 single-sample calls, bit for bit, and a few of them against the oracle."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    from test_gpu_tail import _compare
    e = swapper_m.engine
    m = _masks(84, seed=71)
    m[5] = 0; m[5, 250:262, 250:262] = 1                    # a tiny mask: its own maximum is far below the others'
    se = swapper_m.soft_mask(21, 0.9, 3)
    md = torch.from_numpy(m).cuda()
    got = tail.soft_erosion_frames(e, md, se.weight, 21, 0.9, 3)
    for k in range(84):
        one = tail.soft_erosion_frames(e, md[k:k + 1], se.weight, 21, 0.9, 3)
        assert torch.equal(got[k], one[0]), k
    got = got.cpu().numpy()
    for k in (0, 5, 64, 83):
        want, hard = R.soft_erosion(torch.from_numpy(m[k:k + 1, None].astype(np.float32)), 21, 0.9, 3)
        want, hard = want.numpy()[0, 0], hard.numpy()[0, 0]
        hard_got = np.where(hard, got[k] >= 1.0, (got[k] >= 1.0) & (np.abs(want - 1.0) > 1e-5))     # 1.0: above the threshold or the maximum
        _compare(got[k], want, hard_got, hard, m[k:k + 1], k)


def test_soft_erosion_module_beyond_64(swapper_m):
    """The module path (one maximum over the whole (N,1,H,W) tensor, crop.py:45) at N = 70 against the oracle's whole-batch result."""
    from oracle import cv_ref as R
    from test_gpu_tail import _compare
    m = torch.from_numpy(_masks(70, seed=73).astype(np.float32))[:, None]
    se = swapper_m.soft_mask(21, 0.9, 3)
    soft, hard = se(m)
    want, wmask = R.soft_erosion(m, 21, 0.9, 3)
    _compare(soft.cpu().numpy()[:, 0], want.numpy()[:, 0], hard.cpu().numpy()[:, 0], wmask.numpy()[:, 0], m.numpy()[:, 0], "N = 70")


def test_chain_of_84_frames_is_64_plus_20(sds_m):
    """A FrameChain call of 84 frames (the engine's largest batch) == a 64-frame call followed by a 20-frame call, byte for byte."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import FrameChain
    sw = can_swapper(None, state_dicts=sds_m, max_batch=84)
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    crops, masks, Ms, ori = _batch(84, 81)
    chain = FrameChain(sw)
    got = chain(crops, masks, Ms, ori, idv)["frames"].clone()
    lo = chain(crops[:64], masks[:64], Ms[:64], ori[:64], idv)["frames"].clone()
    hi = chain(crops[64:], masks[64:], Ms[64:], ori[64:], idv)["frames"]
    torch.cuda.synchronize()
    assert torch.equal(got, torch.cat([lo, hi]))
    assert not torch.equal(got[0], got[64])
    del sw, chain
    torch.cuda.empty_cache()


class _NoLaunch:
    """Stands in for the engine's library: any call of cs_soft_erosion_frames is a test failure (nothing reaches the device)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name == "cs_soft_erosion_frames":
            def refuse(*a):
                self.calls.append(a)
                raise AssertionError("cs_soft_erosion_frames launched on a buffer that should have been refused")
            return refuse
        return getattr(self._lib, name)


def test_soft_erosion_frames_validates_its_buffers(swapper_m, monkeypatch):
    """A caller's `out` of the wrong dtype, shape, layout or device, a kernel of another size or on the host, and masks that are not (B,H,W)
    raise ValueError before any launch: the library is replaced by a stub that fails the test if it is called."""
    from canonswap_amd import tail
    e = swapper_m.engine
    se = swapper_m.soft_mask(21, 0.9, 3)
    m = torch.from_numpy(_masks(2, seed=91)[:, :300, :200]).cuda().contiguous()
    want = tail.soft_erosion_frames(e, m, se.weight, 21, 0.9, 3)
    good = torch.empty((2, 300, 200), dtype=torch.float32, device=e.device)
    assert tail.soft_erosion_frames(e, m, se.weight, 21, 0.9, 3, out=good) is good and torch.equal(good, want)
    bad_out = {
        "fp16": torch.empty((2, 300, 200), dtype=torch.float16, device=e.device),
        "fp64": torch.empty((2, 300, 200), dtype=torch.float64, device=e.device),
        "fewer frames": torch.empty((1, 300, 200), dtype=torch.float32, device=e.device),
        "transposed shape": torch.empty((2, 200, 300), dtype=torch.float32, device=e.device),
        "flat": torch.empty((2 * 300 * 200,), dtype=torch.float32, device=e.device),
        "non-contiguous": torch.empty((2, 300, 400), dtype=torch.float32, device=e.device)[..., ::2],
        "host": torch.empty((2, 300, 200), dtype=torch.float32),
    }
    bad_masks = {"2-d": m[0], "(B,2,H,W)": torch.stack([m, m], 1), "5-d": m[None, :, None]}
    stub = _NoLaunch(e.lib)
    monkeypatch.setattr(e, "lib", stub)
    for name, out in bad_out.items():
        with pytest.raises(ValueError):
            tail.soft_erosion_frames(e, m, se.weight, 21, 0.9, 3, out=out)
        assert not stub.calls, name
    for name, w in {"15 x 15 kernel": swapper_m.soft_mask(15, 0.9, 3).weight, "host kernel": se.weight.cpu()}.items():
        with pytest.raises(ValueError):
            tail.soft_erosion_frames(e, m, w, 21, 0.9, 3)
        assert not stub.calls, name
    for name, x in bad_masks.items():
        with pytest.raises(ValueError):
            tail.soft_erosion_frames(e, x, se.weight, 21, 0.9, 3)
        assert not stub.calls, name
