"""cs_yuv_to_rgb and cs_rgb_to_yuv (include/canonswap_yuv.h; canonswap_amd/csrc/yuv.hip) on the GPU, and the video driver in the 4:2:0
pixel formats.  Every comparison is bit-equal to the numpy restatement tests/yuv_ref.py, which tests/test_yuv_cpu.py holds to the standards'
float64 formula.  A thread of either kernel owns 16 x 2 pixels; the fast path needs 8-byte aligned buffers and Wo a multiple of 8 (NV12) or
16 (I420), the tile cut by the right edge and everything else takes byte accesses: the sizes below walk through one block, one cut tile, one
whole tile, whole tiles with a cut one behind them, a width off the fast path, and the driver tests' frame.  The driver's expected bytes are
made of existing pieces: decode_ref, the synchronous RGB loop of tests/test_gpu_video.py, rgb_to_yuv_ref(keep=)."""
import numpy as np
import pytest
import torch

import chain_helpers
import yuv_ref as YR
from chain_helpers import _masks, _occupy
from test_gpu_video import HO, WO, N, _ident, _idle, _lmk, _loop

pytestmark = pytest.mark.gpu

F = 3
SIZES = [(2, 2), (2, 8), (4, 16), (6, 40), (6, 10), (96, 128)]
SET_IDS = [f"{m}-{'full' if fr else 'limited'}" for m, fr in YR.SETS]


@pytest.fixture(scope="module")
def engine():
    from canonswap_amd.engine import Engine
    e = Engine(0, max_batch=1)           # neither call needs weights, scratch or a batch limit
    yield e
    e.close()


def _rand_yuv(f, Ho, Wo, seed):
    """Bytes over the full 0 .. 255, the extremes certainly among them."""
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(f, Ho * 3 // 2, Wo), dtype=np.uint8)
    a[0, 0, 0], a[0, 0, 1], a[-1, -1, -1], a[-1, -1, -2] = 0, 255, 0, 255
    return a


def _rand_rgb(f, Ho, Wo, seed):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(f, Ho, Wo, 3), dtype=np.uint8)
    a[0, 0, 0], a[0, 0, 1], a[-1, -1, -1], a[-1, -1, -2] = 0, 255, (255, 0, 255), (0, 255, 0)
    return a


def _dev(a, offset=0):
    """The array on the device; offset: as a view that starts that many bytes into its buffer."""
    buf = torch.zeros(a.size + offset, dtype=torch.uint8, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a)))
    assert t.is_contiguous() and t.data_ptr() % 8 == offset % 8
    return t


def _both(engine, yuv, layout, matrix="bt601", full_range=False, offset=0):
    """Both kernels on one set of frames against the restatement: the decode; the encode of other RGB frames with keep=None; the encode of the
    decoded frames, one pixel changed in about a third of the blocks, with keep=."""
    from canonswap_amd import tail
    fmt = dict(layout=layout, matrix=matrix, full_range=full_range)
    f, rows, Wo = yuv.shape
    Ho = rows // 3 * 2
    want_rgb = YR.decode_ref(yuv, **fmt)
    d_yuv = _dev(yuv, offset)
    out = _dev(np.full(want_rgb.shape, 7, np.uint8), offset)
    assert tail.yuv_to_rgb(engine, d_yuv, out=out, **fmt) is out
    assert np.array_equal(out.cpu().numpy(), want_rgb), "decode"
    assert np.array_equal(d_yuv.cpu().numpy(), yuv)

    rgb = _rand_rgb(f, Ho, Wo, 1000 + Ho * Wo)
    got = tail.rgb_to_yuv(engine, _dev(rgb, offset), out=_dev(np.full(yuv.shape, 7, np.uint8), offset), **fmt)
    assert np.array_equal(got.cpu().numpy(), YR.rgb_to_yuv_ref(rgb, **fmt)), "encode"

    r = np.random.Generator(np.random.PCG64(2000 + Ho * Wo))
    hit = r.random((f, Ho // 2, Wo // 2)) < 0.3
    hit[0, 0, 0] = True
    px = np.repeat(np.repeat(hit, 2, axis=1), 2, axis=2) & (r.integers(0, 4, size=(f, Ho, Wo)) == 0)
    px[0, 0, 0] = True
    changed = want_rgb.copy()
    changed[px] ^= 0x55
    want = YR.rgb_to_yuv_ref(changed, keep=yuv, **fmt)
    keep = _dev(yuv, offset)
    assert tail.rgb_to_yuv(engine, _dev(changed, offset), keep=keep, **fmt) is keep
    assert np.array_equal(keep.cpu().numpy(), want), "encode with keep"


# ---------------------------------------------------------------------------------------------------------------- both kernels, small sizes
@pytest.mark.parametrize("layout", YR.LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_both_kernels_equal_the_restatement(engine, layout, size):
    _both(engine, _rand_yuv(F, *size, seed=size[0] * 100 + size[1]), layout)


@pytest.mark.parametrize("layout", YR.LAYOUTS)
def test_a_buffer_one_byte_off_takes_the_element_path_with_the_same_values(engine, layout):
    _both(engine, _rand_yuv(F, 96, 128, seed=31), layout, offset=1)


@pytest.mark.parametrize("layout", YR.LAYOUTS)
@pytest.mark.parametrize("matrix,full_range", YR.SETS, ids=SET_IDS)
def test_all_four_coefficient_sets(engine, layout, matrix, full_range):
    _both(engine, _rand_yuv(F, 4, 16, seed=41), layout, matrix, full_range)


def test_host_frames_and_the_swappers_forwards(engine):
    """Host arrays are uploaded; can_swapper.yuv_to_rgb / rgb_to_yuv forward to tail's."""
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper

    class _Holder:
        pass
    h = _Holder()
    h.engine = engine
    yuv = _rand_yuv(2, 4, 16, seed=51)
    rgb = can_swapper.yuv_to_rgb(h, yuv, layout="i420", matrix="bt709")
    assert rgb.is_cuda and np.array_equal(rgb.cpu().numpy(), YR.decode_ref(yuv, "i420", "bt709"))
    back = can_swapper.rgb_to_yuv(h, rgb.cpu().numpy(), layout="i420", matrix="bt709")
    assert np.array_equal(back.cpu().numpy(), YR.rgb_to_yuv_ref(rgb.cpu().numpy(), "i420", "bt709"))
    assert np.array_equal(tail.yuv_to_rgb(engine, torch.from_numpy(yuv)).cpu().numpy(), YR.decode_ref(yuv))


# ---------------------------------------------------------------------------------------------------------------- every triple
@pytest.fixture(scope="module")
def every_triple():
    img = YR.exhaustive_nv12()
    img.setflags(write=False)
    return img, _dev(img)


@pytest.mark.parametrize("matrix,full_range", YR.SETS, ids=SET_IDS)
def test_exhaustive_decode_and_keep(engine, every_triple, matrix, full_range):
    """One 4096 x 4096 NV12 image with every (Y, U, V) once: the decode equals the restatement, and the decoded image through
    cs_rgb_to_yuv(keep=1) leaves all 25 MB as they were."""
    from canonswap_amd import tail
    img, d_img = every_triple
    rgb = tail.yuv_to_rgb(engine, d_img, matrix=matrix, full_range=full_range)
    Y, U, V = YR.split(img, "nv12")
    up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    want = np.stack(YR.decode_values(Y, up(U), up(V), matrix, full_range), axis=-1)
    assert np.array_equal(rgb.cpu().numpy(), want)
    keep = d_img.clone()
    assert tail.rgb_to_yuv(engine, rgb, matrix=matrix, full_range=full_range, keep=keep) is keep
    assert torch.equal(keep, d_img)
    assert np.array_equal(d_img.cpu().numpy(), img)


def test_exhaustive_re_encode_without_keep(engine, every_triple):
    """keep=0 on the same image equals the restatement's re-encode; the round trip's largest differences are printed: a number
    to report, not a gate - most triples lie outside the RGB cube and clamp."""
    from canonswap_amd import tail
    img, d_img = every_triple
    rgb = tail.yuv_to_rgb(engine, d_img)
    got = tail.rgb_to_yuv(engine, rgb).cpu().numpy()
    assert np.array_equal(got, YR.rgb_to_yuv_ref(rgb.cpu().numpy()))
    a, b = YR.split(got, "nv12"), YR.split(img, "nv12")
    dY, dU, dV = (int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max()) for x, y in zip(a, b))
    up = lambda x: np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    inside = np.stack(YR.formula_decode(b[0], up(b[1]), up(b[2]), "bt601", False), axis=-1)
    ok = ((inside >= 0) & (inside <= 255)).all(axis=-1).reshape(1, 2048, 2, 2048, 2).all(axis=(2, 4))
    iY = int(np.abs(a[0].astype(np.int32) - b[0].astype(np.int32))[up(ok)].max())
    iU, iV = (int(np.abs(x.astype(np.int32) - y.astype(np.int32))[ok].max()) for x, y in zip(a[1:], b[1:]))
    print(f"round trip without keep, bt601 limited, every triple: max |dY| {dY}, |dU| {dU}, |dV| {dV}; "
          f"over the {int(ok.sum())} blocks whose four pixels lie inside the RGB cube: |dY| {iY}, |dU| {iU}, |dV| {iV}")


# ---------------------------------------------------------------------------------------------------------------- keep, chosen blocks
@pytest.mark.parametrize("layout,size", [("nv12", (8, 40)), ("i420", (8, 40)), ("i420", (8, 48))], ids=["nv12-8x40", "i420-8x40", "i420-8x48"])
def test_keep_rewrites_exactly_the_changed_blocks(engine, layout, size):
    """One pixel changed in each of: the four corner blocks, an interior block of a whole tile (the fast path in nv12-8x40 and i420-8x48) and
    a block of the last columns (in 8x40 the tile cut by the edge: the element path beside a fast one)."""
    from canonswap_amd import tail
    Ho, Wo = size
    yuv = _rand_yuv(F, Ho, Wo, seed=61)
    rgb = YR.decode_ref(yuv, layout)
    blocks = [(0, 0, 0), (0, 0, Wo // 2 - 1), (0, Ho // 2 - 1, 0), (2, Ho // 2 - 1, Wo // 2 - 1), (1, 1, 5), (1, 2, Wo // 2 - 3)]
    for k, (f, by, bx) in enumerate(blocks):
        rgb[f, 2 * by + (k & 1), 2 * bx + ((k >> 1) & 1), k % 3] ^= 0x80
    keep = _dev(yuv)
    tail.rgb_to_yuv(engine, _dev(rgb), layout=layout, keep=keep)
    got = keep.cpu().numpy()
    want = YR.rgb_to_yuv_ref(rgb, layout, keep=yuv)
    assert np.array_equal(got, want)
    hit = np.zeros((F, Ho // 2, Wo // 2), bool)
    for b in blocks:
        hit[b] = True
    g, o, fresh = YR.split(got, layout), YR.split(yuv, layout), YR.split(YR.rgb_to_yuv_ref(rgb, layout), layout)
    px = np.repeat(np.repeat(hit, 2, axis=1), 2, axis=2)
    assert np.array_equal(g[0], np.where(px, fresh[0], o[0]))
    assert np.array_equal(g[1], np.where(hit, fresh[1], o[1])) and np.array_equal(g[2], np.where(hit, fresh[2], o[2]))
    assert all((g[0][f, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2] != o[0][f, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2]).any() for f, by, bx in blocks)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_refused_argument_is_refused_before_any_launch(engine):
    """Through the one call path into the C ABI: the status names the argument, nothing was enqueued, and the buffers hold what they held."""
    from canonswap_amd import tail
    yuv, rgb = _dev(np.full((2, 6, 8), 3, np.uint8)), _dev(np.full((2, 4, 8, 3), 5, np.uint8))
    both = torch.zeros(2 * 4 * 8 * 3 + 16, dtype=torch.uint8, device="cuda")
    four_channels, on_the_host = torch.zeros((2, 4, 8, 4), dtype=torch.uint8, device="cuda"), yuv.cpu()
    torch.cuda.synchronize()                          # from here on nothing but a launch of the library's could occupy the stream
    dec = lambda F_=2, y=yuv, Ho=4, Wo=8, lay=0, m=0, fr=0, out=rgb: engine._call("cs_yuv_to_rgb", F_, y, Ho, Wo, lay, m, fr, out)
    enc = lambda F_=2, r=rgb, Ho=4, Wo=8, lay=0, m=0, fr=0, keep=0, out=yuv: engine._call("cs_rgb_to_yuv", F_, r, Ho, Wo, lay, m, fr, keep, out)
    cases = [("F = 0", dict(F_=0)), ("Ho = 5", dict(Ho=5)), ("Ho = 0", dict(Ho=0)), ("Ho = 16386", dict(Ho=16386)), ("Wo = 7", dict(Wo=7)),
             ("Wo = 16386", dict(Wo=16386)), ("layout 2", dict(lay=2)), ("layout -1", dict(lay=-1)), ("matrix 2", dict(m=2)),
             ("full_range 2", dict(fr=2))]
    for f, name in ((dec, "cs_yuv_to_rgb"), (enc, "cs_rgb_to_yuv")):
        for text, kw in cases:
            with pytest.raises(RuntimeError, match=f"{name}: {text}"):
                f(**kw)
    with pytest.raises(RuntimeError, match="cs_rgb_to_yuv: keep 2"):
        enc(keep=2)
    with pytest.raises(RuntimeError, match="cs_yuv_to_rgb: NULL yuv"):
        dec(y=None)
    with pytest.raises(RuntimeError, match="cs_yuv_to_rgb: NULL rgb"):
        dec(out=None)
    with pytest.raises(RuntimeError, match="cs_rgb_to_yuv: NULL rgb"):
        enc(r=None)
    with pytest.raises(RuntimeError, match="cs_yuv_to_rgb: rgb and yuv overlap"):
        dec(y=both[8:], out=both)
    with pytest.raises(RuntimeError, match="cs_rgb_to_yuv: rgb and yuv overlap"):
        enc(r=both, out=both[2 * 4 * 8 * 3 - 1:])
    with pytest.raises(ValueError, match="overlap"):
        tail.rgb_to_yuv(engine, both[: 2 * 4 * 8 * 3].view(2, 4, 8, 3), out=both[16: 16 + 96].view(2, 6, 8))
    with pytest.raises(ValueError, match="keep"):
        tail.rgb_to_yuv(engine, rgb, keep=yuv[:, :, ::2])
    with pytest.raises(ValueError, match="keep"):
        tail.rgb_to_yuv(engine, rgb, keep=on_the_host)
    with pytest.raises(ValueError, match="out"):
        tail.yuv_to_rgb(engine, yuv, out=four_channels)
    assert torch.cuda.current_stream().query()
    assert (yuv == 3).all() and (rgb == 5).all() and not both.any()


# ---------------------------------------------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


@pytest.fixture(scope="module")
def chain(swapper_m):
    from canonswap_amd.chain import FrameChain
    return FrameChain(swapper_m)


def _want(chain, yuv, lmk, plan, layout, idv, masks, fi=None, **fmt):
    """decode_ref, the synchronous RGB loop, rgb_to_yuv_ref(keep=)."""
    rgb = YR.decode_ref(yuv, layout, **fmt)
    return YR.rgb_to_yuv_ref(_loop(chain, rgb, lmk, plan, idv, masks=masks, fi=fi), layout, keep=yuv, **fmt)


@pytest.fixture(scope="module")
def scene(chain):
    """Two 4:2:0 videos of N frames (the same bytes read as NV12 and as I420), one face each, and the expected frames in batches of 2,
    computed once and never written."""
    from canonswap_amd.video import plan_batches
    s = {"A": _rand_yuv(N, HO, WO, 201), "B": _rand_yuv(N, HO, WO, 202), "lmkA": _lmk(N, 103), "lmkB": _lmk(N, 104), "masks": _masks(N, seed=105),
         "id": _ident(7), "plan": plan_batches(N, None, 2, 4)}
    for v in "AB":
        for layout in YR.LAYOUTS:
            w = s[f"want{v}_{layout}"] = _want(chain, s[v], s["lmk" + v], s["plan"], layout, s["id"], s["masks"])
            w.setflags(write=False)
            changed = (w != s[v]).any(axis=(1, 2))
            Y0, U0, V0 = YR.split(s[v], layout)
            Y1, U1, V1 = YR.split(w, layout)
            kept = ((Y0 == Y1).reshape(N, HO // 2, 2, WO // 2, 2).all(axis=(2, 4)) & (U0 == U1) & (V0 == V1)).any(axis=(1, 2))
            assert changed.all() and kept.all()               # every frame got its paste, and in every frame a block kept its input bytes
        s[v].setflags(write=False)
    return s


@pytest.mark.parametrize("source", ["ndarray", "list", "pinned"])
def test_nv12_video_from_every_kind_of_source(swapper_m, chain, scene, source):
    from canonswap_amd.video import VideoSwapper
    keep = np.array(scene["A"])
    frames = {"ndarray": lambda: keep.copy(), "list": lambda: [f.copy() for f in keep], "pinned": lambda: torch.from_numpy(keep.copy()).pin_memory()}[source]()
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    got, spans = np.zeros_like(keep), []
    for f0, f1, view in drv.run(frames, scene["lmkA"], scene["id"], masks=scene["masks"], pixel_format="nv12"):
        assert isinstance(view, np.ndarray) and view.shape == (f1 - f0, HO * 3 // 2, WO) and view.dtype == np.uint8
        spans.append((f0, f1))
        got[f0:f1] = view
    assert spans == [p[:2] for p in scene["plan"]] and np.array_equal(got, scene["wantA_nv12"])
    assert np.array_equal(np.stack([np.asarray(f) for f in frames]), keep)       # the caller's frames were not written
    out = swapper_m.swap_video(frames, scene["lmkA"], scene["id"], masks=scene["masks"], pixel_format="nv12", driver=drv)
    assert out.shape == keep.shape and np.array_equal(out, scene["wantA_nv12"])
    pinned_out = torch.full(keep.shape, 9, dtype=torch.uint8).pin_memory()
    assert drv.swap_video(frames, scene["lmkA"], scene["id"], masks=scene["masks"], pixel_format="nv12", out=pinned_out) is pinned_out
    assert np.array_equal(pinned_out.numpy(), scene["wantA_nv12"])
    assert not chain._pending and _idle(drv)


def test_i420_video_and_another_matrix(swapper_m, chain, scene):
    from canonswap_amd.video import VideoSwapper
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    got = drv.swap_video(scene["B"], scene["lmkB"], scene["id"], masks=scene["masks"], pixel_format="i420")
    assert np.array_equal(got, scene["wantB_i420"]) and not np.array_equal(got, scene["wantB_nv12"])
    fmt = dict(matrix="bt709", full_range=True)
    want = _want(chain, scene["B"], scene["lmkB"], scene["plan"], "i420", scene["id"], scene["masks"], **fmt)
    assert not np.array_equal(want, scene["wantB_i420"])
    assert np.array_equal(drv.swap_video(scene["B"], scene["lmkB"], scene["id"], masks=scene["masks"], pixel_format="i420", **fmt), want)


def test_frames_without_a_face_come_back_byte_for_byte(swapper_m, chain, scene):
    """Seven frames, five faces: frames 4 and 5 hold none (a whole step of the plan), frame 1 two."""
    from canonswap_amd.video import VideoSwapper, plan_batches
    fi = np.array([0, 1, 1, 2, 3, 6], np.int32)
    plan = plan_batches(N, fi, 2, 2)
    lmk = _lmk(6, 111, centres=[(60, 48), (56, 46), (68, 50), (45, 44), (85, 52), (64, 47)])
    masks = _masks(6, seed=112)
    want = _want(chain, scene["A"], lmk, plan, "nv12", scene["id"], masks, fi=fi)
    drv = VideoSwapper(swapper_m, batch=2, max_faces=2, chain=chain)
    got = drv.swap_video(scene["A"], lmk, scene["id"], frame_index=fi, masks=masks, pixel_format="nv12")
    assert np.array_equal(got, want)
    assert np.array_equal(got[4:6], scene["A"][4:6]) and all((got[f] != scene["A"][f]).any() for f in (0, 1, 2, 3, 6))


def _without_host_waits(run):
    """run() with torch's sync debug mode at "error" -> (result, True), or, where this torch build has no such mode, (run(), False)."""
    if not hasattr(torch.cuda, "set_sync_debug_mode") or not hasattr(torch._C, "_cuda_set_sync_debug_mode"):
        return run(), False
    torch.cuda.set_sync_debug_mode("error")
    try:
        return run(), True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("late", ["upload", "sink", "caller"])
def test_two_videos_on_one_driver_under_a_late_stream(swapper_m, chain, scene, late):
    """As test_gpu_video's test_slot_reuse_under_a_late_stream: four batches of two frames, so every YUV and every RGB slot is used twice per
    video, video A and then video B on the same driver with one stream held busy before B.  Identity slots, masks on the device and pinned
    frames both ways, so that nothing makes the host wait for the caller's stream: where the rgb24 path runs under torch's sync debug mode
    "error", so does the 4:2:0 one."""
    from canonswap_amd.video import VideoSwapper
    e = swapper_m.engine
    e.set_identity(scene["id"].cuda(), 0)
    masks = torch.from_numpy(scene["masks"]).cuda()
    slots = [0] * N
    main = torch.cuda.current_stream()
    _occupy(main, 1)
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    pin = {v: torch.from_numpy(np.array(scene[v])).pin_memory() for v in "AB"}
    out = torch.zeros(pin["A"].shape, dtype=torch.uint8).pin_memory()
    rgb_in = torch.from_numpy(YR.decode_ref(scene["A"])).pin_memory()
    rgb_out = torch.zeros(rgb_in.shape, dtype=torch.uint8).pin_memory()
    drv.swap_video(pin["A"], scene["lmkA"], slots=slots, masks=masks, pixel_format="nv12", out=out)      # warm: buffers and kernels
    drv.swap_video(rgb_in, scene["lmkA"], slots=slots, masks=masks, out=rgb_out)
    torch.cuda.synchronize()
    try:
        _, strict = _without_host_waits(lambda: drv.swap_video(rgb_in, scene["lmkA"], slots=slots, masks=masks, out=rgb_out))
    except RuntimeError as err:
        print(f"the rgb24 path does not run under sync debug mode 'error' here ({str(err)[:80]}): the 4:2:0 path is run without it")
        strict = False
    torch.cuda.synchronize()
    run = _without_host_waits if strict else (lambda f: (f(), False))
    run(lambda: drv.swap_video(pin["A"], scene["lmkA"], slots=slots, masks=masks, pixel_format="nv12", out=out))
    assert np.array_equal(out.numpy(), scene["wantA_nv12"])
    torch.cuda.synchronize()
    _occupy({"upload": drv.upload.stream, "sink": drv.sink.stream, "caller": main}[late], 60)
    run(lambda: drv.swap_video(pin["B"], scene["lmkB"], slots=slots, masks=masks, pixel_format="nv12", out=out))
    assert np.array_equal(out.numpy(), scene["wantB_nv12"])
    print(f"late {late}: under sync debug mode 'error': {strict}")
    assert not chain._pending and _idle(drv)


def test_early_break_and_a_change_of_format_leave_the_driver_usable(swapper_m, chain, scene):
    """After `break` the driver is idle and runs either format; an rgb24 run before and after a 4:2:0 run gives the synchronous loop's frames."""
    from canonswap_amd.video import VideoSwapper
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    rgb = YR.decode_ref(scene["A"])
    kw = dict(masks=scene["masks"])
    want_rgb = _loop(chain, rgb, scene["lmkA"], scene["plan"], scene["id"], masks=scene["masks"])
    assert np.array_equal(drv.swap_video(rgb, scene["lmkA"], scene["id"], **kw), want_rgb)
    gen = drv.run(scene["A"], scene["lmkA"], scene["id"], pixel_format="nv12", **kw)
    for f0, f1, view in gen:
        assert (f0, f1) == (0, 2) and np.array_equal(view, scene["wantA_nv12"][:2])
        break
    gen.close()
    assert not chain._pending and _idle(drv)
    assert np.array_equal(drv.swap_video(rgb, scene["lmkA"], scene["id"], **kw), want_rgb)
    assert np.array_equal(drv.swap_video(scene["B"], scene["lmkB"], scene["id"], pixel_format="i420", **kw), scene["wantB_i420"])
    gen = drv.run(rgb, scene["lmkA"], scene["id"], **kw)
    next(gen)
    gen.close()
    assert not chain._pending and _idle(drv)
    assert np.array_equal(drv.swap_video(scene["A"], scene["lmkA"], scene["id"], pixel_format="nv12", **kw), scene["wantA_nv12"])
    assert np.array_equal(drv.swap_video(rgb, scene["lmkA"], scene["id"], **kw), want_rgb)
