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


# ---- the shared bilinear tap of imgops.hip (tap_at / tap_u8x3 / tap_f32) on shapes so small that every class of tap occurs: every entry
# point that reads through it, straight against oracle/cv_ref.py
_TAP_SRC = (6, 10)            # source H x W
_TAP_THETAS = (0.3, -0.5)


def _tap_matrix(theta, Hd, Wd, s=2.0):
    """Scale 2 and a rotation about the source's centre (5, 3), which lands (0.3, -0.2) off the destination's centre."""
    c, sn = np.cos(theta), np.sin(theta)
    tx = Wd / 2 - s * (5 * c - 3 * sn) + 0.3
    ty = Hd / 2 - s * (5 * sn + 3 * c) - 0.2
    return np.array([[s * c, -s * sn, tx], [s * sn, s * c, ty]], np.float64)


def _tap_classes(M, Hd, Wd):
    """From the oracle's fixed-point coordinates: (counts of the nine classes (rows both in / only the lower in / only the upper in) x
    (columns likewise) among the pixels with fx > 0 and fy > 0, the map of pixels whose four taps are all outside)."""
    from oracle import cv_ref as R
    Hs, Ws = _TAP_SRC
    sx, sy, fx, fy = R._coords(R.invert_affine(M), Hd, Wd)
    rows = [(sy >= 0) & (sy + 1 < Hs), sy == -1, sy == Hs - 1]
    cols = [(sx >= 0) & (sx + 1 < Ws), sx == -1, sx == Ws - 1]
    frac = (fx > 0) & (fy > 0)
    counts = np.array([[int((rw & cl & frac).sum()) for cl in cols] for rw in rows])
    outside = (sx < -1) | (sy < -1) | (sx >= Ws) | (sy >= Hs)
    return counts, outside


@pytest.mark.parametrize("dest", ["24x32", "24x28", "23x29", "crop24"])
def test_shared_tap_every_class_vs_oracle(swapper, dest):
    """Destinations: 24x32 (paste_shared's 8-pixel path, paste_batch's dword path), 24x28 (the 4-pixel path), 23x29 (paste_shared's single-frame
    fallback, paste_batch's one-pixel path), and cs_crop_frames at dsize 24.  Bit for bit against the cv_ref composition; the inputs are checked to hold every tap class."""
    from canonswap_amd import tail
    from oracle import cv_ref as R
    e = swapper.engine
    Hs, Ws = _TAP_SRC
    r = np.random.Generator(np.random.PCG64(2718))
    crops = r.integers(0, 256, size=(3, Hs, Ws, 3), dtype=np.uint8)          # crops[0] is "the source"
    masks = r.random(size=(3, Hs, Ws), dtype=np.float32)

    def same(got, want, what):
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
        d = got != want
        assert not d.any(), (dest, what, int(d.sum()), np.argwhere(d)[:3].tolist())

    def covered(M, Hd, Wd):
        counts, outside = _tap_classes(M, Hd, Wd)
        print(dest, "tap classes with fx, fy > 0 (rows: both / lower / upper x columns likewise)", counts.tolist(), "all outside", int(outside.sum()))
        assert counts.min() >= 1 and outside.sum() >= 1, (dest, counts.tolist(), int(outside.sum()))
        return outside

    if dest == "crop24":
        Ms = np.stack([_tap_matrix(th, 24, 24) for th in _TAP_THETAS])
        for M in Ms:
            covered(M, 24, 24)
        got = tail.crop_frames_M(e, crops[:2], Ms, 24)["crops"]
        same(got, np.stack([R.warp_affine_u8(crops[b], Ms[b], (24, 24)) for b in range(2)]), "crop_frames_M")
        return

    Hd, Wd = (int(v) for v in dest.split("x"))
    oris = r.integers(0, 256, size=(3, Hd, Wd, 3), dtype=np.uint8)
    mask_ori = r.random(size=(Hd, Wd), dtype=np.float32)
    mask_ori[1, 1] = 1.0                                                      # seeded values in [0, 1], both ends included
    mask_ori[10:14, 12:18] = 0.0                                              # exact zeros over pixels that would read the crop
    mask_ori[0:2, 0:4] = 1.0                                                  # ones over pixels whose taps are all outside (asserted below)
    want_fused = {}
    for th in _TAP_THETAS:
        M = _tap_matrix(th, Hd, Wd)
        outside = covered(M, Hd, Wd)
        assert outside[0:2, 0:4].all() and not outside[10:14, 12:18].any(), (dest, th)
        same(tail.warp_affine_u8(e, crops[0], M, (Wd, Hd)), R.warp_affine_u8(crops[0], M, (Wd, Hd)), ("warp_affine_u8", th))
        for b in range(3):
            want_fused[th, b] = R.paste_back(crops[b], M, oris[b], R.prepare_paste_back(masks[b], M, (Wd, Hd))[..., None])
        same(tail.prepare_paste_back(e, masks[0], M, (Wd, Hd)), R.prepare_paste_back(masks[0], M, (Wd, Hd)), ("prepare_paste_back", th))
        same(tail.paste_back(e, crops[0], M, oris[0], mask_ori), R.paste_back(crops[0], M, oris[0], mask_ori[..., None]), ("paste_back", th))
        same(tail.paste_back_fused(e, crops[0], masks[0], M, oris[0]), want_fused[th, 0], ("paste_back_fused", th))
        same(tail.paste_back_shared(e, crops, M, oris[0], mask_ori),
             np.stack([R.paste_back(crops[b], M, oris[0], mask_ori[..., None]) for b in range(3)]), ("paste_back_shared", th))
    ths = (_TAP_THETAS[0], _TAP_THETAS[1], _TAP_THETAS[0])                    # both matrices and one repeated
    same(tail.paste_back_batch(e, crops, masks, np.stack([_tap_matrix(th, Hd, Wd) for th in ths]), oris),
         np.stack([want_fused[ths[b], b] for b in range(3)]), "paste_back_batch")
