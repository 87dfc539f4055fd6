"""The video driver (canonswap_amd/video.py: VideoSwapper over HostFrames, FrameChain and FrameSink): host frames in, pasted-back host frames
out, the copies of a batch beside the generator of its neighbours.  The reference result is always the plain synchronous loop, written here
per planned batch (upload, chain.crop, chain(...), .cpu()), and every comparison is byte for byte.  Frames are 96 x 128 random uint8,
landmarks synthetic as the crop tests build them, one module-scope engine of max_batch 4.  Every wait in here is an event or stream wait on
work already queued."""
import numpy as np
import pytest
import torch

import chain_helpers
from chain_helpers import _logits, _masks, _occupy

pytestmark = pytest.mark.gpu

HO, WO, N = 96, 128, 7


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


def _frames(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(n, HO, WO, 3), dtype=np.uint8)


def _lmk(n, seed, centres=None):
    from test_gpu_crop import _face
    r = np.random.Generator(np.random.PCG64(seed))
    centres = centres or [(r.uniform(40, 90), r.uniform(40, 55)) for _ in range(n)]
    return np.stack([_face(r, c, 26.0, r.uniform(-0.4, 0.4)) for c in centres])


def _ident(seed):
    from canonswap_amd import synth
    return torch.from_numpy(synth.make_identity(seed)).reshape(1, 512)


def _loop(chain, frames, lmk, plan, source_id=None, slots=None, masks=None, logits=None, fi=None):
    """The synchronous loop: per planned batch, frames to the device, crop, chain, frames back."""
    dev = chain.e.device
    out = np.empty_like(frames)
    for f0, f1, b0, b1 in plan:
        fr = torch.from_numpy(frames[f0:f1]).to(dev)
        sid = None if source_id is None else (source_id if source_id.shape[0] == 1 else source_id[b0:b1]).to(dev)
        kw = dict(slots=None if slots is None else slots[b0:b1], logits=None if logits is None else logits[b0:b1])
        m = None if masks is None else torch.as_tensor(masks[b0:b1]).to(dev)
        if fi is None:
            c = chain.crop(fr, lmk[b0:b1])
            res = chain(c["crops"], m, c["M_c2o"], fr, sid, **kw)
        elif b1 == b0:
            res = chain(torch.empty((0, 512, 512, 3), dtype=torch.uint8, device=dev), None, None, fr, frame_index=[])
        else:
            idx = np.asarray(fi[b0:b1]) - f0
            c = chain.crop(fr, lmk[b0:b1], frame_index=idx)
            res = chain(c["crops"], m, c["M_c2o"], fr, sid, frame_index=idx, **kw)
        out[f0:f1] = res["frames"].cpu().numpy()
    return out


@pytest.fixture(scope="module")
def scene(chain):
    """Two videos of N frames with one face each, their masks, and the loop's result for each in batches of 2 (computed once, never written)."""
    from canonswap_amd.video import plan_batches
    s = {"A": _frames(N, 101), "B": _frames(N, 102), "lmkA": _lmk(N, 103), "lmkB": _lmk(N, 104), "masks": _masks(N, seed=105), "id": _ident(7)}
    plan = plan_batches(N, None, 2, 4)
    for v in "AB":
        s["want" + v] = _loop(chain, s[v], s["lmk" + v], plan, s["id"], masks=s["masks"])
        s["want" + v].setflags(write=False)
        assert (s["want" + v] != s[v]).any(axis=(1, 2, 3)).all()                # every frame got its paste
    assert not np.array_equal(s["wantA"], s["wantB"])
    return s


def _idle(drv):
    """After a wait for the CALLER's stream alone, the driver's three streams have nothing left: they were joined to it."""
    torch.cuda.current_stream().synchronize()
    return all(st.query() for st in drv.streams())


# ---------------------------------------------------------------------------------------------------------------- 1, 2: sources, sinks, batch sizes
@pytest.mark.parametrize("source", ["ndarray", "list", "pinned"])
def test_three_batches_from_every_kind_of_source(swapper_m, chain, scene, source):
    """N = 7 in batches of 3, 3 and 1, through run() and through swap_video(out=), from an ndarray, a list of arrays and a pinned tensor: the
    loop's bytes (in batches of 3; the scene's, in batches of 2, are the same: case 2), and the caller's frames as they were."""
    from canonswap_amd.video import VideoSwapper, plan_batches
    plan = plan_batches(N, None, 3, 4)
    assert [(p[0], p[1]) for p in plan] == [(0, 3), (3, 6), (6, 7)]
    want = _loop(chain, scene["A"], scene["lmkA"], plan, scene["id"], masks=scene["masks"])
    assert np.array_equal(want, scene["wantA"])
    keep = scene["A"].copy()
    frames = {"ndarray": lambda: keep.copy(), "list": lambda: [f.copy() for f in keep], "pinned": lambda: torch.from_numpy(keep.copy()).pin_memory()}[source]()
    drv = VideoSwapper(swapper_m, batch=3, chain=chain)
    got, spans = np.zeros_like(keep), []
    for f0, f1, view in drv.run(frames, scene["lmkA"], scene["id"], masks=scene["masks"]):
        assert isinstance(view, np.ndarray) and view.shape == (f1 - f0, HO, WO, 3) and view.dtype == np.uint8
        spans.append((f0, f1))
        got[f0:f1] = view
    assert spans == [(0, 3), (3, 6), (6, 7)] and np.array_equal(got, want)
    assert np.array_equal(np.stack([np.asarray(f) for f in frames]), keep)       # the caller's frames were not written
    assert not chain._pending

    out = np.full_like(keep, 9)
    assert drv.swap_video(frames, scene["lmkA"], scene["id"], masks=torch.from_numpy(scene["masks"]).cuda(), out=out) is out
    assert np.array_equal(out, want)
    pinned_out = torch.full((N, HO, WO, 3), 9, dtype=torch.uint8).pin_memory()
    assert drv.swap_video(frames, scene["lmkA"], scene["id"], masks=scene["masks"], out=pinned_out) is pinned_out
    assert np.array_equal(pinned_out.numpy(), want)
    made = swapper_m.swap_video(frames, scene["lmkA"], scene["id"], masks=scene["masks"], driver=drv)
    assert isinstance(made, np.ndarray) and np.array_equal(made, want)
    assert np.array_equal(np.stack([np.asarray(f) for f in frames]), keep)
    assert drv.swap_video(keep[:0], scene["lmkA"][:0], scene["id"], masks=scene["masks"][:0]).shape == (0, HO, WO, 3)


def test_the_batch_size_does_not_change_the_bytes(swapper_m, chain, scene):
    """batch=2, batch=4 and the swapper's default driver (batch = max_batch = 4): default-mode bits do not depend on the batch."""
    from canonswap_amd.video import VideoSwapper
    for batch in (2, 4):
        got = VideoSwapper(swapper_m, batch=batch, chain=chain).swap_video(scene["B"], scene["lmkB"], scene["id"], masks=scene["masks"])
        assert np.array_equal(got, scene["wantB"]), batch
    assert np.array_equal(swapper_m.swap_video(scene["B"], scene["lmkB"], scene["id"], masks=scene["masks"]), scene["wantB"])
    assert swapper_m._video.batch == 4


# ---------------------------------------------------------------------------------------------------------------- 3: faces per frame
def test_frame_index_with_frames_and_a_batch_without_a_face(swapper_m, chain, scene):
    """Seven frames, six faces: frame 1 holds two overlapping faces, frames 4 and 5 none.  In steps of two frames and two faces, frame 1 does
    not fit behind frame 0's face and opens the next step, and frames 4, 5 make a step without any face.  Two identities, per face."""
    from canonswap_amd.video import VideoSwapper, plan_batches
    fi = np.array([0, 1, 1, 2, 3, 6], np.int32)
    plan = plan_batches(N, fi, 2, 2)
    assert plan == [(0, 1, 0, 1), (1, 2, 1, 3), (2, 4, 3, 5), (4, 6, 5, 5), (6, 7, 5, 6)]
    lmk = _lmk(6, 111, centres=[(60, 48), (56, 46), (68, 50), (45, 44), (85, 52), (64, 47)])      # faces 1 and 2 overlap in frame 1
    masks = _masks(6, seed=112)
    a, b = _ident(7), _ident(9)
    ids = torch.cat([a, b, a, b, b, a])
    want = _loop(chain, scene["A"], lmk, plan, ids, masks=masks, fi=fi)
    assert np.array_equal(want[4:6], scene["A"][4:6]) and all((want[f] != scene["A"][f]).any() for f in (0, 1, 2, 3, 6))
    one = _loop(chain, scene["A"], lmk, plan, a, masks=masks, fi=fi)
    assert not np.array_equal(one[1], want[1])                                  # the second identity shows
    drv = VideoSwapper(swapper_m, batch=2, max_faces=2, chain=chain)
    spans = []
    got = np.zeros_like(want)
    for f0, f1, view in drv.run(scene["A"], lmk, ids, frame_index=fi, masks=masks):
        spans.append((f0, f1))
        got[f0:f1] = view
    assert spans == [p[:2] for p in plan] and np.array_equal(got, want)
    assert np.array_equal(drv.swap_video(list(scene["A"]), lmk, ids.cuda(), frame_index=fi.tolist(), masks=torch.from_numpy(masks).cuda()), want)
    with pytest.raises(ValueError, match="frame_index.*frame 1 "):
        VideoSwapper(swapper_m, batch=2, max_faces=1, chain=chain).run(scene["A"], lmk, ids, frame_index=fi, masks=masks)


# ---------------------------------------------------------------------------------------------------------------- 4: slot reuse and the waits
def _beside(busy, other, kind):
    """Does work queued on `other` run while `busy` is held?  Streams are software; the runtime spreads them, kernels and copies, over a few
    hardware queues, and two streams that share one run in order whatever their events say.  A short bounded spin on `busy` (with a
    download queued behind it, when `other` is to upload past it), then on `other` the kind of work the driver puts there - a kernel, an
    upload from pinned memory, a download into it - and the two end times."""
    d = torch.zeros(HO * WO * 6, dtype=torch.uint8, device="cuda")
    h, h2 = torch.zeros(HO * WO * 6, dtype=torch.uint8).pin_memory(), torch.zeros(HO * WO * 6, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    _occupy(busy, 20)
    end_busy, end_other = chain_helpers._timed(), chain_helpers._timed()
    with torch.cuda.stream(busy):
        if kind == "upload":
            h2.copy_(d, non_blocking=True)
        end_busy.record(busy)
    with torch.cuda.stream(other):
        if kind == "kernel":
            d.add_(1)
        elif kind == "upload":
            d.copy_(h, non_blocking=True)
        else:
            h.copy_(d, non_blocking=True)
        end_other.record(other)
    torch.cuda.synchronize()
    return end_other.elapsed_time(end_busy) > 5.0                               # `other` was done well inside the 20 ms of the spin


def _driver_with_streams_side_by_side(swapper, chain, rule, skip):
    """A driver whose wait of `rule` is a wait that matters: the stream that waits and the stream it waits for (b: caller's and upload; c: upload
    and sink; d: sink and caller's) do not share a hardware queue, so that without the wait the later work really overtakes the earlier.  (Rule
    a is a host wait: any driver.)  A new driver takes the next two streams, and one more is taken between two tries, so that the pairs do not
    all fall on the queues alike; one of the first few has them apart.  None if none of them has: a box that maps its streams otherwise."""
    from canonswap_amd.video import VideoSwapper
    main = torch.cuda.current_stream()
    tried = []
    for _ in range(8):
        drv = VideoSwapper(swapper, batch=2, chain=chain, _skip_waits=skip)
        busy, other, kind = {"a": (None, None, None), "b": (drv.upload.stream, main, "kernel"), "c": (drv.sink.stream, drv.upload.stream, "upload"),
                             "d": (main, drv.sink.stream, "download")}[rule]
        if busy is None or _beside(busy, other, kind):
            print(f"rule {rule}: driver {len(tried) + 1} has the two streams side by side")
            return drv
        tried.append((drv, torch.cuda.Stream()))
    print(f"rule {rule}: no driver of {len(tried)} got two streams that run side by side")
    return None


@pytest.mark.parametrize("rule,late", [("a", "upload"), ("b", "upload"), ("c", "sink"), ("d", "caller")])
def test_slot_reuse_under_a_late_stream(swapper_m, chain, scene, rule, late):
    """Four batches of two frames, so every slot is used twice per video, and the same driver runs video A and then video B: what a slot
    holds from before is real pixels.  One stream is held busy (a bounded spin, chain_helpers._occupy) before video B is run, so that the
    work queued on it is certainly late: the upload stream for rules a and b, the sink's for rule c (and d, which then holds trivially), the
    caller's - on which the paste-back runs - for rule d.  With every wait in place the bytes are the loop's.  That each check can fail is
    shown by a driver built with the one wait left out (a constructor argument of this test's only): its bytes differ.  Both drivers are
    chosen so that the two streams of the rule run side by side (_driver_with_streams_side_by_side): on one hardware queue the order would
    hold without the wait.  Identity slots and masks on the device, so that no step of the loop makes the host wait for the caller's stream.
    Rule c is shown in time, not in bytes.  Without its wait the upload stream reaches the copy of batch 2 into slot 0 while the download of
    batch 0 from that slot is still held (measured on an MI355X: reached at 3.0 ms, the download ended at 71.9 ms), but the runtime there
    puts the two copies on one in-order copy queue, where the upload then stands behind the held download (it ended at 71.9 ms too) and the
    bytes come out right by the queue's order, not by the driver's.  Stream semantics promise no such order, so the wait stays, and what is
    asserted is the order of two events: with the wait the upload stream is let go after the download's end (`early <= 0`), without it before."""
    e = swapper_m.engine
    e.set_identity(scene["id"].cuda(), 0)
    masks = torch.from_numpy(scene["masks"]).cuda()
    slots = [0] * N
    main = torch.cuda.current_stream()
    _occupy(main, 1)                                                            # the spin's first launch in a process loads its code: calibrate after it
    torch.cuda.synchronize()

    def a_then_b(drv):
        assert np.array_equal(drv.swap_video(scene["A"], scene["lmkA"], slots=slots, masks=masks), scene["wantA"]) or drv._skip
        torch.cuda.synchronize()
        _occupy({"upload": drv.upload.stream, "sink": drv.sink.stream, "caller": main}[late], 60)
        drv.trace = []
        got = drv.swap_video(scene["B"], scene["lmkB"], slots=slots, masks=masks)
        torch.cuda.synchronize()
        ev, drv.trace = {(k, name): t for k, name, t in drv.trace}, None
        # rule c in time: how long before the download of batch 0 ended did the upload stream reach the copy of batch 2 into the same slot
        return got, ev[(2, "h2d_begin")].elapsed_time(ev[(0, "d2h_end")])

    from canonswap_amd.video import VideoSwapper
    good = _driver_with_streams_side_by_side(swapper_m, chain, rule, ()) or VideoSwapper(swapper_m, batch=2, chain=chain)
    got, early = a_then_b(good)
    assert np.array_equal(got, scene["wantB"])
    assert early <= 0, f"the upload into slot 0 was let go {early:.3f} ms before the download that read it had ended"
    if late == "sink":
        torch.cuda.synchronize()
        _occupy(main, 60)                                                       # rule d with the paste-back late as well
        assert np.array_equal(good.swap_video(scene["A"], scene["lmkA"], slots=slots, masks=masks), scene["wantA"])
    bad = _driver_with_streams_side_by_side(swapper_m, chain, rule, rule)
    if bad is None:                                                             # everything above holds; only the negative control cannot be shown
        pytest.skip(f"rule {rule}: the two streams of the rule share a hardware queue on this box, where a missing wait shows nothing")
    got, early = a_then_b(bad)
    differs = not np.array_equal(got, scene["wantB"])
    print(f"rule {rule} left out: bytes differ: {differs}; upload of batch 2 let go {early:.2f} ms before the download of batch 0 ended")
    if rule == "c":
        assert early > 0, "leaving out the wait of rule c changed nothing: the upload was not let go before the download had ended"
    else:
        assert differs, f"leaving out the wait of rule {rule} changed nothing"
    assert not chain._pending and _idle(bad)
    assert np.array_equal(good.swap_video(scene["B"], scene["lmkB"], slots=slots, masks=masks), scene["wantB"])      # and the chain is as it was


# ---------------------------------------------------------------------------------------------------------------- 5: the view's lifetime
def test_a_consumer_may_scribble_on_a_view_until_the_next_item(swapper_m, chain, scene):
    """Rule e: the consumer reads a view, zeroes it and keeps it across one next(); the later batches come out as in the loop."""
    from canonswap_amd.video import VideoSwapper
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    got, held = np.zeros_like(scene["wantA"]), []
    for f0, f1, view in drv.run(scene["A"], scene["lmkA"], scene["id"], masks=scene["masks"]):
        got[f0:f1] = view
        view[...] = 0
        held = [view] + held[:1]                                                # this view and the one before stay referenced
    assert np.array_equal(got, scene["wantA"])


# ---------------------------------------------------------------------------------------------------------------- 6, 7: early exit, logits_fn
def test_early_exit_leaves_the_driver_usable(swapper_m, chain, scene):
    """Rule f: `break` after the first batch, and a logits_fn that raises on its second call; each time the same driver then runs the whole
    video and matches the loop, and nothing stays staged in the chain."""
    from canonswap_amd.video import VideoSwapper
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    gen = drv.run(scene["A"], scene["lmkA"], scene["id"], masks=scene["masks"])
    for f0, f1, view in gen:
        assert (f0, f1) == (0, 2) and np.array_equal(view, scene["wantA"][:2])
        break
    gen.close()
    assert not chain._pending and _idle(drv)
    assert np.array_equal(drv.swap_video(scene["B"], scene["lmkB"], scene["id"], masks=scene["masks"]), scene["wantB"])

    calls = []

    def failing(pv):
        calls.append(tuple(pv.shape))
        if len(calls) == 2:
            raise KeyError("the caller's parser failed")
        return _logits(pv.shape[0], 5)

    with pytest.raises(KeyError, match="parser failed"):
        drv.swap_video(scene["A"], scene["lmkA"], scene["id"], logits_fn=failing)
    assert calls == [(2, 3, 512, 512)] * 2
    assert not chain._pending and _idle(drv)
    assert np.array_equal(drv.swap_video(scene["A"], scene["lmkA"], scene["id"], masks=scene["masks"]), scene["wantA"])
    drv.close()
    assert _idle(drv)


def test_logits_fn_is_called_per_batch_in_order(swapper_m, chain, scene):
    """The caller's parser network, here a stand-in that returns fixed logits: called once per batch, in order, on chain.parser_input of
    that batch's crops; the frames are those of the loop fed the same logits."""
    from canonswap_amd.video import VideoSwapper, plan_batches
    lg = _logits(N, 6)
    plan = plan_batches(N, None, 3, 4)
    want = _loop(chain, scene["B"], scene["lmkB"], plan, scene["id"], logits=lg)
    assert (want != scene["B"]).any(axis=(1, 2, 3)).all() and not np.array_equal(want, scene["wantB"])
    seen, pos = [], [0]

    def parser(pv):
        assert pv.is_cuda and pv.dtype == torch.float32 and tuple(pv.shape[1:]) == (3, 512, 512)
        seen.append(pv.clone())
        pos[0] += pv.shape[0]
        return lg[pos[0] - pv.shape[0]: pos[0]]

    drv = VideoSwapper(swapper_m, batch=3, chain=chain)
    assert np.array_equal(drv.swap_video(scene["B"], scene["lmkB"], scene["id"], logits_fn=parser), want)
    assert [int(p.shape[0]) for p in seen] == [3, 3, 1]
    fr = torch.from_numpy(scene["B"][3:6]).cuda()
    assert torch.equal(seen[1], chain.parser_input(chain.crop(fr, scene["lmkB"][3:6])["crops"]))


# ---------------------------------------------------------------------------------------------------------------- 8: latency mode
def test_latency_mode_engine_runs_in_line(sds_m, scene):
    """A latency-mode engine (max_batch 1): FrameChain.prefetch refuses there, the driver does not call it and does not raise; two frames,
    equal to the same engine's own in-line loop."""
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import FrameChain
    from canonswap_amd.video import VideoSwapper, plan_batches
    sw = can_swapper(None, state_dicts=sds_m, max_batch=1, latency_mode=True)
    ch = FrameChain(sw)
    frames, lmk, masks = scene["A"][:2], scene["lmkA"][:2], scene["masks"][:2]
    want = _loop(ch, frames, lmk, plan_batches(2, None, 1, 1), scene["id"], masks=masks)
    assert (want != frames).any(axis=(1, 2, 3)).all()
    drv = VideoSwapper(sw, chain=ch)
    assert drv.batch == 1 and not drv.prefetch
    spans = []
    got = np.zeros_like(want)
    for f0, f1, view in drv.run(frames, lmk, scene["id"], masks=masks):
        spans.append((f0, f1))
        got[f0:f1] = view
    assert spans == [(0, 1), (1, 2)] and np.array_equal(got, want)
    assert ch._side is None and not ch._pending


# ---------------------------------------------------------------------------------------------------------------- 9: refusals
def test_refusals_name_the_argument_and_enqueue_nothing(swapper_m, chain, scene):
    from canonswap_amd.video import VideoSwapper
    drv = VideoSwapper(swapper_m, batch=2, chain=chain)
    A, lmk, masks, idv = scene["A"], scene["lmkA"], scene["masks"], scene["id"]
    swapper_m.engine.set_identity(idv.cuda(), 0)
    assert _idle(drv)
    ok = dict(masks=masks)
    cases = [
        ("frames", lambda: drv.run([A[0], A[1][:, :100], A[2]], lmk[:3], idv, **ok)),                     # unequal sizes
        ("frames", lambda: drv.run(A.astype(np.float32), lmk, idv, **ok)),                                 # wrong dtype
        ("frames", lambda: drv.run([A[0], A[1].astype(np.int16)], lmk[:2], idv, **ok)),
        ("frames", lambda: drv.run(A[..., :2], lmk, idv, **ok)),
        ("frames", lambda: drv.run(torch.from_numpy(A).cuda(), lmk, idv, **ok)),                           # device frames are FrameChain's
        ("lmk", lambda: drv.run(A, lmk[:6], idv, **ok)),
        ("lmk", lambda: drv.run(A, lmk, idv, frame_index=[0, 1, 2], masks=masks[:3])),
        ("masks", lambda: drv.run(A, lmk, idv, masks=masks[:6])),
        ("masks", lambda: drv.run(A, lmk, idv, masks=torch.from_numpy(masks[:5]).cuda())),
        ("masks", lambda: drv.run(A, lmk, idv, masks=masks[:, ::2, ::2])),                                 # (B, 256, 256)
        ("masks", lambda: drv.run(A, lmk, idv, masks=masks.astype(np.float32))),
        ("slots", lambda: drv.run(A, lmk, slots=[0] * 6, **ok)),
        ("slots", lambda: drv.run(A, lmk, idv, slots=[0] * N, **ok)),                                      # slots and source_id
        ("source_id", lambda: drv.run(A, lmk, torch.zeros(3, 512), **ok)),
        ("source_id", lambda: drv.run(A, lmk, torch.zeros(1, 256), **ok)),
        ("masks / parse / logits_fn", lambda: drv.run(A, lmk, idv)),                                       # no mask source
        ("masks / parse / logits_fn", lambda: drv.run(A, lmk, idv, masks=masks, parse=True)),              # more than one
        ("masks / parse / logits_fn", lambda: drv.run(A, lmk, idv, masks=masks, logits_fn=lambda pv: pv)),
        ("masks / parse / logits_fn", lambda: drv.run(A, lmk, idv, parse=True, logits_fn=lambda pv: pv)),
        ("frame_index", lambda: drv.run(A, lmk, idv, frame_index=[0, 1, 2, 3, 4, 6, 5], **ok)),
        ("frame_index", lambda: drv.run(A, lmk, idv, frame_index=[0, 1, 2, 3, 4, 5, 7], **ok)),
        ("frame_index.*frame 2 ", lambda: drv.run(A, lmk, idv, frame_index=[0, 2, 2, 2, 2, 2, 6], **ok)),  # five faces in frame 2, max_batch 4
        ("out", lambda: drv.swap_video(A, lmk, idv, out=np.empty((N, HO, WO + 1, 3), np.uint8), **ok)),
        ("out", lambda: drv.swap_video(A, lmk, idv, out=np.empty((N - 1, HO, WO, 3), np.uint8), **ok)),
        ("out", lambda: drv.swap_video(A, lmk, idv, out=np.empty((N, HO, WO, 3), np.float32), **ok)),
        ("out", lambda: drv.swap_video(A, lmk, idv, out=torch.empty((N, HO, WO, 3), dtype=torch.int8), **ok)),
    ]
    for who, call in cases:
        with pytest.raises(ValueError, match=who):
            call()
        assert all(st.query() for st in drv.streams() + [torch.cuda.current_stream()]), who
    with pytest.raises(RuntimeError, match="parse"):                            # no parser among this engine's weights
        drv.run(A, lmk, idv, parse=True)
    with pytest.raises(ValueError, match="batch"):
        VideoSwapper(swapper_m, batch=0, chain=chain)
    with pytest.raises(ValueError, match="chain"):
        VideoSwapper(swapper_m, chain=chain, iterations=2)
    assert drv.upload.pinned is None and drv.upload.dev is None and drv.sink.pinned is None      # not a buffer was made
    assert not chain._pending and _idle(drv)
    assert np.array_equal(drv.swap_video(A, lmk, idv, **ok), scene["wantA"])     # and the accepted call runs
