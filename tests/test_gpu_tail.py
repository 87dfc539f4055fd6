"""N2 / N3 on the device (csrc/imgops.hip) against oracle/cv_ref.py: integer / byte work bit-exact; SoftErosion (fp32 conv with
another summation order than torch) to 2e-6 with at most a handful of threshold flips."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def swapper(state_dicts):
    from canonswap_amd.can_swap_e2e import can_swapper
    return can_swapper(None, state_dicts=state_dicts, max_batch=4)


def test_soft_erosion_vs_reference_vectors(swapper, golden):
    g = golden("soft_erosion.npz")
    for name, (ks, thr, it) in {"e2e": (21, 0.9, 3), "v2i": (21, 0.9, 2)}.items():
        se = swapper.soft_mask(ks, thr, it)
        # built on this host with the reference's formula: the fp32 sum that normalises it may differ in the last bit between CPUs
        assert np.allclose(se.weight.cpu().numpy(), g[name + "_weight"], rtol=1e-6, atol=0)
        for k in (0, 1):          # the vectors were made one sample per call, as the pipeline calls it (the max of crop.py:45 is over the call's tensor)
            x = torch.from_numpy(g[f"{name}_{k}_in"].astype(np.int32))[None, None]
            soft, hard = se(x)
            soft, hard = {k: soft.cpu().numpy()[0, 0]}, {k: hard.cpu().numpy()[0, 0]}
            flips = hard[k] != g[f"{name}_{k}_hard"]
            d = np.abs(soft[k] - g[f"{name}_{k}_soft"])[~flips]
            print(name, k, "hard-mask flips", int(flips.sum()), "max |soft diff| elsewhere", float(d.max()))
            assert flips.sum() <= 4, (name, k, int(flips.sum()))          # pixels whose conv value sits within rounding of 0.9
            assert d.max() < 2e-6, (name, k, float(d.max()))


def test_soft_erosion_batch_normalises_by_the_max_of_the_whole_batch(swapper, golden):
    """`x[~mask] /= x[~mask].max()` (crop.py:45) takes the maximum over the whole (N,1,H,W) tensor.  A batch of two
    different masks against the oracle (pinned to the reference class for N = 1, same code for N = 2)."""
    from oracle import cv_ref as R
    g = golden("soft_erosion.npz")
    x = torch.from_numpy(np.stack([g["e2e_0_in"], (g["e2e_1_in"] * 0.5)]).astype(np.float32))[:, None]
    se = swapper.soft_mask(21, 0.9, 3)
    soft, hard = se(x)
    want, wmask = R.soft_erosion(x, 21, 0.9, 3)
    flips = hard.cpu().numpy().astype(bool) != wmask.numpy()
    assert flips.sum() <= 8
    d = np.abs(soft.cpu().numpy() - want.numpy())[~flips]
    assert d.max() < 2e-6, float(d.max())
    # ... and it differs from normalising each sample by its own maximum
    own, _ = R.soft_erosion(x[1:2], 21, 0.9, 3)
    assert float((own - want[1:2]).abs().max()) > 1e-3


def test_prepare_crops_bit_exact(swapper):
    from oracle import cv_ref as R
    from oracle import canonswap_ref as O
    r = np.random.Generator(np.random.PCG64(7))
    crops = r.integers(0, 256, size=(3, 512, 512, 3), dtype=np.uint8)
    got = swapper.prepare_source(crops).cpu().numpy()
    want = np.concatenate([O.prepare_source(R.resize_area_2x_u8(c)).numpy() for c in crops])
    assert got.shape == (3, 3, 256, 256) and np.array_equal(got, want)
    small = r.integers(0, 256, size=(2, 256, 256, 3), dtype=np.uint8)
    from canonswap_amd import tail
    assert np.array_equal(tail.prepare_crops(swapper.engine, small).cpu().numpy(),
                          np.concatenate([O.prepare_source(c).numpy() for c in small]))


@pytest.mark.parametrize("case", ["upscale_rot", "downscale", "partly_outside"])
def test_paste_back_bit_exact(swapper, case):
    from oracle import cv_ref as R
    r = np.random.Generator(np.random.PCG64(11))
    crop = r.integers(0, 256, size=(512, 512, 3), dtype=np.uint8)
    Ho, Wo = (720, 1280) if case != "downscale" else (300, 400)
    ori = r.integers(0, 256, size=(Ho, Wo, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    mask = np.clip(1.2 - np.hypot(xx - 256, yy - 256) / 200, 0, 1).astype(np.float32)
    th = {"upscale_rot": 0.3, "downscale": -0.1, "partly_outside": 0.05}[case]
    sc = {"upscale_rot": 1.13, "downscale": 0.37, "partly_outside": 0.9}[case]
    tx, ty = {"upscale_rot": (333.25, 41.6), "downscale": (60.1, 20.9), "partly_outside": (-200.5, 500.3)}[case]
    M = np.array([[sc * np.cos(th), -sc * np.sin(th), tx], [sc * np.sin(th), sc * np.cos(th), ty], [0, 0, 1]], np.float64)
    mask_ori = R.prepare_paste_back(np.stack([mask] * 3, -1), M, (Wo, Ho))
    want = R.paste_back(crop, M, ori, mask_ori)
    got_mask = swapper.prepare_paste_back(mask, M, (Wo, Ho)).cpu().numpy()
    assert np.array_equal(got_mask, mask_ori[..., 0])
    from canonswap_amd import tail

    def same(a, b, what):
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert d.max() == 0, (what, int((d > 0).sum()), int(d.max()), np.argwhere(d > 0)[:3].tolist())

    same(tail.warp_affine_u8(swapper.engine, crop, M, (Wo, Ho)).cpu().numpy(), R.warp_affine_u8(crop, M[:2], (Wo, Ho)), "warp_u8")
    same(swapper.paste_back(crop, M, ori, torch.from_numpy(mask_ori)).cpu().numpy(), want, "paste_back")
    same(swapper.paste_back_fused(crop, mask, M, ori).cpu().numpy(), want, "fused")


def test_frame_streamer_equals_whole_video_upload(swapper):
    from oracle import cv_ref as R
    from oracle import canonswap_ref as O
    r = np.random.Generator(np.random.PCG64(13))
    frames = [r.integers(0, 256, size=(512, 512, 3), dtype=np.uint8) for _ in range(10)]
    seen = []
    for I, (a, b) in swapper.stream_videos(frames, batch=4):
        assert I.shape == (b - a, 3, 256, 256)
        seen.append((a, b, I.cpu().numpy()))
    assert [(a, b) for a, b, _ in seen] == [(0, 4), (4, 8), (8, 10)]
    got = np.concatenate([x for _, _, x in seen])
    want = np.concatenate([O.prepare_source(R.resize_area_2x_u8(f)).numpy() for f in frames])
    assert np.array_equal(got, want)


# ---- SoftErosion at its edges: se_conv_kernel's two instantiations (KS = 21 for the pipeline, 15 for the module's defaults, crop.py:21),
# the scalar tail store (W % 4 != 0, a partial 8-wide group), partial 64 x 32 tiles, images smaller than a tile or than the kernel, one row
def _edge_masks(H, W, seed):
    """Four masks with real edges: two ellipses scaled to the image with random blobs toggled in, an all-ones mask (only the zero padding
    pulls pixels below the threshold: the maximum comes from the border) and a tiny one (its maximum is far below the others')."""
    r = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for _ in range(2):
        cx, cy, a, b = r.uniform(0.4, 0.6) * W, r.uniform(0.4, 0.6) * H, r.uniform(0.25, 0.4) * W, r.uniform(0.3, 0.45) * H
        m = ((xx - cx) / max(a, 0.5)) ** 2 + ((yy - cy) / max(b, 0.5)) ** 2 <= 1
        for _ in range(6):
            bx, by, rad = r.uniform(0, W), r.uniform(0, H), r.uniform(1, max(2, min(H, W) / 6))
            m ^= np.hypot(xx - bx, yy - by) <= rad
        m[H // 2, W // 2] = True                              # never empty (an all-zero mask divides 0 by 0)
        out.append(m)
    out.append(np.ones((H, W), bool))
    tiny = np.zeros((H, W), bool)
    tiny[H // 2:H // 2 + 2, W // 3:W // 3 + 2] = True
    out.append(tiny)
    return np.stack(out).astype(np.uint8)


def _edge_pixels(masks):
    """Value changes between neighbouring pixels of the zero-padded masks: the pixels near which a conv value can sit at the threshold."""
    p = np.pad(np.asarray(masks, dtype=np.int8), ((0, 0), (1, 1), (1, 1)))
    return int((p[:, 1:] != p[:, :-1]).sum() + (p[:, :, 1:] != p[:, :, :-1]).sum())


def _compare(got, want, hard_got, hard_want, masks, what):
    """Hard-mask flips (conv values within fp32 rounding of the threshold) at most 4 + one per 1000 edge pixels; elsewhere |soft - oracle|
    < 2e-6.  That bound holds for a tiny mask too, whose normalising maximum is far below 1: the soft value is a ratio of two sums of
    non-negative fp32 terms, whose rounding is relative, so dividing by a small maximum does not scale the error up (a float64 run of
    the same operation against the oracle: at most 1.4e-6 at every shape and setting here, 1.2e-7 for the tiny masks)."""
    flips = hard_got != hard_want
    limit = 4 + _edge_pixels(masks) // 1000
    d = np.abs(got - want)[~flips]
    print(what, "flips", int(flips.sum()), "of at most", limit, "max |soft diff| elsewhere", float(d.max()) if d.size else 0.0)
    assert flips.sum() <= limit, (what, int(flips.sum()), limit)
    assert d.size == 0 or d.max() < 2e-6, (what, float(d.max()))


@pytest.mark.parametrize("ks", [21, 15])
@pytest.mark.parametrize("size", [(512, 512), (301, 403), (256, 256), (33, 68), (17, 45), (1, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_soft_erosion_edges_vs_oracle(swapper, size, ks):
    """tail.soft_erosion_frames (per-sample maximum; uint8 labels and their fp32 copy give the same bits) and the module path (one maximum
    for the whole tensor) against oracle/cv_ref.py, for iterations 1 / 2 / 3 and thresholds 0.9 / 0.6."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    H, W = size
    e = swapper.engine
    m = _edge_masks(H, W, seed=H * 1000 + W)
    mf = torch.from_numpy(m.astype(np.float32))
    md = torch.from_numpy(m).cuda()
    for iters in (1, 2, 3):
        for thr in (0.9, 0.6):
            se = swapper.soft_mask(ks, thr, iters)
            what = (H, W, ks, iters, thr)
            got = tail.soft_erosion_frames(e, md, se.weight, ks, thr, iters)
            assert torch.equal(got, tail.soft_erosion_frames(e, md.float(), se.weight, ks, thr, iters)), what
            got = got.cpu().numpy()
            for k in range(len(m)):
                want, hard = R.soft_erosion(mf[k:k + 1, None], ks, thr, iters)
                want, hard = want.numpy()[0, 0], hard.numpy()[0, 0]
                # the frames entry point returns no hard mask: a pixel at 1.0 is above the threshold or the maximum itself
                hard_got = np.where(hard, got[k] >= 1.0, (got[k] >= 1.0) & (np.abs(want - 1.0) > 1e-5))
                _compare(got[k], want, hard_got, hard, m[k:k + 1], what + (k,))
            soft, hard_got = se(mf[:, None])
            want, hard = R.soft_erosion(mf[:, None], ks, thr, iters)
            _compare(soft.cpu().numpy()[:, 0], want.numpy()[:, 0], hard_got.cpu().numpy()[:, 0], hard.numpy()[:, 0], m, what + ("module",))
