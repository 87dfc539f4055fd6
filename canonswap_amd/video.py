"""The video driver: a user's frames start in host memory and have to end there (video decode and encode stay on the host), and
between the two stands chain.FrameChain.  The reference loads the whole video into Python lists (can_swap_pipeline_e2e.py:155, io.py:19-29),
loops frame by frame (:223-283) and hands the lists to images2video (:319).  Here the same walk is made in batches, with the two copies of a
batch beside the generator of its neighbours instead of around its own:

    drv = VideoSwapper(swapper)                                               # batch = the engine's max_batch
    for f0, f1, view in drv.run(frames, lmk, source_id, masks=masks): ...     # view: pinned (f1 - f0, Ho, Wo, 3) u8, valid until the next next()
    out = drv.swap_video(frames, lmk, source_id, parse=True)                  # or drained into one (N, Ho, Wo, 3) array

Host Python over chain.FrameChain, tail, torch streams and events.  In the default pixel_format "rgb24" the driver has no kernel
of its own.  In "nv12" and "i420" it has two, cs_yuv_to_rgb and cs_rgb_to_yuv (include/canonswap_yuv.h, tail.yuv_to_rgb / rgb_to_yuv; DESIGN
8.13): the frames cross the link as the codec has them, 1.5 bytes per pixel each way instead of 3, and are converted on the device.

The schedule is one batch ahead.  Iteration k of the loop, all of it enqueued from the calling thread (the engine is not thread-safe):
    1. upload batch k + 1: host frames -> pinned slot -> device slot (k + 1) % 2, on the upload stream
    2. chain.crop and chain.prefetch of batch k + 1 (crop on the caller's stream, stage A on the chain's side stream)
    3. chain(...) of batch k with out= the device slot that holds its frames: the paste-back is in place (cs_paste_back_faces allows it; the
       driver therefore always passes a frame index, 0 .. n-1 when every frame holds one face: bit-equal to cs_paste_back_batch)
    4. download that slot into pinned slot k % 2 on the sink's stream
    5. yield batch k - 1
Two device slots and two pinned slots each way, allocated once per (batch, Ho, Wo) and kept for the life of the driver.  Per step of B frames
of Ho x Wo the link carries B * Ho * Wo * 3 bytes up and as many down (64 frames of 1080 x 1920: 398 MB each way) plus the masks, when they
come from the host (B * 256 KB).

The ordering rules.  Three streams beside the caller's: HostFrames.stream (upload), FrameSink.stream (download), the chain's side stream.
    a. A pinned upload slot is rewritten by the host only after the H2D copy that read it has completed (host wait on `copied`).
    b. The crop of a batch waits for that batch's upload (the caller's stream waits for `copied`).
    c. A device slot is uploaded into only after the download that read it has completed (the upload stream waits for `consumed`).
    d. The download of a slot waits for the paste-back that wrote it (the sink's stream waits for `pasted`, recorded on the caller's stream).
    e. A view is yielded only after its D2H event is synchronised (`done`); its pinned slot is the target of a download again only after the
       consumer has asked for the next item - the generator does not run between two next() calls.
    f. On close(), break, or an exception (the caller's logits_fn included), chain.drop_prefetches() runs and the caller's stream waits for
       the upload and the sink's stream (drop_prefetches joins the chain's side stream): the driver and its chain are usable again.
The 4:2:0 formats (pixel_format="nv12" / "i420", with matrix= and full_range=).  frames, out= and the yielded views are (N, 3 Ho / 2, Wo)
uint8, the memory of ffmpeg's rawvideo; the slots above hold YUV, and two further device slots (batch, Ho, Wo, 3) hold the RGB frames the
chain works on.  Per slot: 1. the upload as above, into the device YUV slot; 2. on the caller's stream, behind the wait of rule b,
cs_yuv_to_rgb writes the RGB slot; 3. crop, prefetch, chain and in-place paste-back as above, on the RGB slot; 4. cs_rgb_to_yuv(keep=1)
converts the RGB slot back into the YUV slot it came from; 5. `pasted` is recorded behind it; 6. the YUV slot is downloaded.  The RGB slots
are read and written on the caller's stream only, so stream order is all they need; rules a - f, their events and their waits are the same
lines in both formats, and there is no further stream.  A batch without a face is not converted at all.  Because of keep, a frame without a
face and every 2 x 2 block outside what the paste-back changed come back with the bytes they came in with; the blocks the paste changed are
re-encoded (Y per pixel, U and V from the block's sums).  Per step the link carries B * Ho * Wo * 3 / 2 bytes each way (64 frames of 1080 x
1920: 199 MB), the two launches move 597 MB and 796 MB of device memory.

What the chain orders itself (stage A against the generator, the double buffer) stands in chain._StagedChain and is not restated here.
On a latency-mode engine FrameChain.prefetch refuses; the driver runs stage A in-line there and keeps the rest of the schedule.  Stage A
is prefetched only when the masks come finished (masks=): where it makes them of logits (logits_fn, parse=True) it runs in-line.
"""
from __future__ import annotations

import numpy as np

def _no_mark(name):
    """The trace switched off (VideoSwapper.trace is None)."""


_RULES = frozenset("abcd")      # the waits VideoSwapper(_skip_waits=) can leave out, by rule letter (tests/test_gpu_video.py only)


# ---------------------------------------------------------------------------------------------------------------- planning (no torch)
def _frame_index(frame_index, n_frames):
    """tail.frame_index_of without its face count: 1-D integers, non-decreasing, in [0, n_frames)."""
    a = np.asarray(frame_index)
    if a.ndim != 1:
        raise ValueError(f"frame_index: expected one frame number per face, got shape {tuple(a.shape)}")
    if a.shape[0] and a.dtype.kind not in "iu":
        raise ValueError(f"frame_index: expected integers, got {a.dtype}")
    a = a.astype(np.int64)
    if a.shape[0] and (a.min() < 0 or a.max() >= n_frames):
        raise ValueError(f"frame_index: frame numbers must lie in [0, {n_frames}), got {int(a.min())} .. {int(a.max())}")
    if a.shape[0] > 1 and (np.diff(a) < 0).any():
        raise ValueError(f"frame_index: must not decrease (decreases at face {int(np.argmax(np.diff(a) < 0)) + 1}): the faces of a frame are contiguous")
    return a


def plan_batches(n_frames, frame_index=None, batch=64, max_faces=84):
    """-> [(f0, f1, b0, b1)]: frames [f0, f1) and their faces [b0, b1), in order, every frame and every face once.  Without frame_index
    frame f holds face f and a batch holds at most min(batch, max_faces) frames.  With it (the frame of each face, as tail.frame_index_of
    takes it) a batch takes whole frames only - at most `batch` of them, at most `max_faces` faces - and may hold frames without a face, or
    no face at all.  ValueError before any work for batch < 1 and for a frame that alone holds more than max_faces faces."""
    n_frames, batch, max_faces = int(n_frames), int(batch), int(max_faces)
    if batch < 1:
        raise ValueError(f"batch: must be at least 1, got {batch}")
    if max_faces < 1:
        raise ValueError(f"max_faces: must be at least 1, got {max_faces}")
    if n_frames < 0:
        raise ValueError(f"n_frames: must not be negative, got {n_frames}")
    if frame_index is None:
        step = min(batch, max_faces)
        return [(f, min(f + step, n_frames), f, min(f + step, n_frames)) for f in range(0, n_frames, step)]
    fi = _frame_index(frame_index, n_frames)
    first = np.searchsorted(fi, np.arange(n_frames + 1), side="left")      # frame f owns faces first[f] .. first[f + 1] - 1
    per_frame = np.diff(first)
    if n_frames and per_frame.max() > max_faces:
        f = int(np.argmax(per_frame > max_faces))
        raise ValueError(f"frame_index: frame {f} alone holds {int(per_frame[f])} faces, more than max_faces = {max_faces}")
    plan, f0 = [], 0
    while f0 < n_frames:
        f1 = f0 + 1
        while f1 < n_frames and f1 - f0 < batch and first[f1 + 1] - first[f0] <= max_faces:
            f1 += 1
        plan.append((f0, f1, int(first[f0]), int(first[f1])))
        f0 = f1
    return plan


# ---------------------------------------------------------------------------------------------------------------- host frames
def _host_copy(dst, src):
    """dst: a CPU uint8 tensor; src: an ndarray of its shape.  torch's copy where torch can alias src (it spreads a large copy over its
    intra-op threads), numpy's otherwise (read-only or negatively strided arrays)."""
    import torch
    if src.flags.writeable and all(s >= 0 for s in src.strides):
        dst.copy_(torch.from_numpy(src))
    else:
        np.copyto(dst.numpy(), src)


PIXEL_FORMATS = ("rgb24", "nv12", "i420")


def _yuv_hw(shape, what):
    """A 4:2:0 frame's (3 Ho / 2, Wo) -> (Ho, Wo); both must be even, which for Ho means a row count that is a multiple of 3."""
    rows, Wo = int(shape[0]), int(shape[1])
    if rows % 3 or Wo % 2:
        raise ValueError(f"{what}: a 4:2:0 frame is (3 Ho / 2, Wo) uint8 with Ho and Wo even, got {rows} x {Wo} (Ho = {rows * 2 / 3:g})")
    return rows // 3 * 2, Wo


class _Source:
    """The caller's frames, validated once and never written: `n` frames of `hw`, each of shape `frame` ((Ho, Wo, 3), or (3 Ho / 2, Wo) with
    yuv=True); `pinned` is the (n, *frame) pinned tensor they already are, or None; fill(dst, f0, f1) copies frames [f0, f1) into the first
    rows of the pinned tensor dst."""

    def __init__(self, frames, who="frames", yuv=False):
        import torch
        self.pinned, self._arr, self._seq = None, None, None
        self.yuv = bool(yuv)
        one, ok = ("(3 Ho / 2, Wo)", lambda sh: len(sh) == 2) if yuv else ("(Ho, Wo, 3)", lambda sh: len(sh) == 3 and sh[2] == 3)
        many = "(N, " + one[1:]
        if isinstance(frames, torch.Tensor):
            if frames.device.type != "cpu":
                raise ValueError(f"{who}: expected host frames, got a tensor on {frames.device} (FrameChain takes device frames as they are)")
            if frames.dtype != torch.uint8 or frames.dim() < 1 or not ok(frames.shape[1:]):
                raise ValueError(f"{who}: expected {many} uint8, got {tuple(frames.shape)} {frames.dtype}")
            if frames.is_pinned() and frames.is_contiguous():
                self.pinned = frames
            else:
                self._arr = frames.detach().numpy()
            self.n, self.frame = int(frames.shape[0]), tuple(int(v) for v in frames.shape[1:])
        elif isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or frames.ndim < 1 or not ok(frames.shape[1:]):
                raise ValueError(f"{who}: expected {many} uint8, got {tuple(frames.shape)} {frames.dtype}")
            self._arr = frames
            self.n, self.frame = int(frames.shape[0]), tuple(int(v) for v in frames.shape[1:])
        else:
            try:
                seq = [f.detach().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
            except TypeError:
                raise ValueError(f"{who}: expected an {many} uint8 array, a CPU tensor or a sequence of {one} uint8 arrays") from None
            for j, f in enumerate(seq):
                if f.dtype != np.uint8 or not ok(f.shape):
                    raise ValueError(f"{who}: frame {j}: expected {one} uint8, got {tuple(f.shape)} {f.dtype}")
                if f.shape != seq[0].shape:
                    raise ValueError(f"{who}: frame {j} is {f.shape[0]} x {f.shape[1]}, frame 0 is {seq[0].shape[0]} x {seq[0].shape[1]}: one size per video")
            self._seq = seq
            self.n, self.frame = len(seq), (tuple(int(v) for v in seq[0].shape) if seq else ((0, 0) if yuv else (0, 0, 3)))
        self.hw = _yuv_hw(self.frame, who) if yuv else self.frame[:2]

    def fill(self, dst, f0, f1):
        if self._arr is not None:
            _host_copy(dst[: f1 - f0], self._arr[f0:f1])
        else:
            for j in range(f0, f1):
                _host_copy(dst[j - f0], self._seq[j])


class _Slots:
    """What HostFrames and FrameSink share: a stream of their own and two pinned host buffers u8, (batch, Ho, Wo, 3) or for 4:2:0 frames
    (batch, 3 Ho / 2, Wo), allocated at the first reserve() of a size and format and kept."""

    def __init__(self, device, batch):
        import torch
        self.device, self.batch = torch.device(device), int(batch)
        self.stream = torch.cuda.Stream(device=self.device)
        self.hw, self.yuv, self.pinned = None, False, None

    def reserve(self, Ho, Wo, yuv=False):
        import torch
        if (self.hw, self.yuv) != ((Ho, Wo), bool(yuv)):
            frame = (Ho * 3 // 2, Wo) if yuv else (Ho, Wo, 3)
            self.pinned = None
            self.pinned = [torch.empty((self.batch,) + frame, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._reserve_device(frame)
            self.hw, self.yuv = (Ho, Wo), bool(yuv)

    def _reserve_device(self, frame):
        pass


class HostFrames(_Slots):
    """Upload: host frames -> pinned slot -> device slot, on `stream`.  Two slots, each a pinned and a device buffer (batch, Ho, Wo, 3) u8 with
    two events: `copied[s]` (the H2D copy into device slot s is done) and `consumed[s]` (what read device slot s last - the download of the
    batch pasted there - is done; the driver records it on the sink's stream).  A source that is a pinned tensor is copied from its own memory."""

    def __init__(self, device, batch):
        import torch
        super().__init__(device, batch)
        self.dev = None
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [torch.cuda.Event(), torch.cuda.Event()]

    def _reserve_device(self, frame):
        import torch
        self.dev = None                                   # the old pair goes before the new one comes
        self.dev = [torch.empty((self.batch,) + frame, dtype=torch.uint8, device=self.device) for _ in range(2)]

    def upload(self, src: _Source, f0, f1, s, skip=(), mark=_no_mark):
        """Frames [f0, f1) of src into device slot s -> that slot's first f1 - f0 frames (a view).  Rules a and c.  mark: the driver's
        trace (VideoSwapper.trace), called with a name on the stream where the event belongs."""
        import torch
        n = f1 - f0
        if src.pinned is not None:
            host = src.pinned[f0:f1]
        else:
            if "a" not in skip:
                self.copied[s].synchronize()              # rule a (an event never recorded counts as complete)
            src.fill(self.pinned[s], f0, f1)
            host = self.pinned[s][:n]
        with torch.cuda.stream(self.stream):
            if "c" not in skip:
                self.stream.wait_event(self.consumed[s])  # rule c
            mark("h2d_begin")
            self.dev[s][:n].copy_(host, non_blocking=True)
            self.copied[s].record(self.stream)
            mark("h2d_end")
        return self.dev[s][:n]


class FrameSink(_Slots):
    """Download: device frames -> pinned slot (or the caller's own pinned memory), on `stream`.  Two pinned slots (batch, Ho, Wo, 3) u8 with
    two events each: `pasted[s]` (recorded by the driver on the caller's stream behind the paste-back whose frames go to slot s) and
    `done[s]` (the D2H copy into slot s is done).  The device side of a slot is HostFrames' device slot: the paste-back is in place, so the
    sink reads where the upload wrote and owns no device memory."""

    def __init__(self, device, batch):
        import torch
        super().__init__(device, batch)
        self.pasted = [torch.cuda.Event(), torch.cuda.Event()]
        self.done = [torch.cuda.Event(), torch.cuda.Event()]

    def download(self, frames_dev, s, into=None, skip=(), mark=_no_mark):
        """frames_dev (n, Ho, Wo, 3) on the device -> the host tensor that receives them: the first n rows of pinned slot s, or `into` (pinned,
        (n, Ho, Wo, 3)).  Rule d."""
        import torch
        host = self.pinned[s][: frames_dev.shape[0]] if into is None else into
        with torch.cuda.stream(self.stream):
            if "d" not in skip:
                self.stream.wait_event(self.pasted[s])    # rule d
            mark("d2h_begin")
            host.copy_(frames_dev, non_blocking=True)
            self.done[s].record(self.stream)
            mark("d2h_end")
        return host


# ---------------------------------------------------------------------------------------------------------------- the driver
class VideoSwapper:
    """drv = VideoSwapper(swapper, batch=None, chain=None, prefetch=True, max_faces=None, **chain_kw)

    batch: frames per step, the engine's max_batch by default; max_faces: faces per step, the engine's max_batch by default and at most.
    chain: a FrameChain to drive; otherwise one is built from chain_kw (kernel_size, threshold, iterations, valid).  prefetch=False, or a
    latency-mode engine: stage A runs in-line.  `upload` (HostFrames) and `sink` (FrameSink) hold the slots and the two streams."""

    def __init__(self, swapper, batch=None, chain=None, prefetch=True, max_faces=None, _skip_waits=(), **chain_kw):
        from .chain import FrameChain
        if chain is not None and chain_kw:
            raise ValueError(f"chain: an existing chain takes no {sorted(chain_kw)}; they are FrameChain's constructor arguments")
        self.chain = FrameChain(swapper, **chain_kw) if chain is None else chain
        self.e = self.chain.e
        self.batch = int(self.e.max_batch if batch is None else batch)
        if self.batch < 1:
            raise ValueError(f"batch: must be at least 1, got {self.batch}")
        self.max_faces = int(self.e.max_batch if max_faces is None else max_faces)
        if not 1 <= self.max_faces <= self.e.max_batch:
            raise ValueError(f"max_faces: must lie in [1, {self.e.max_batch}] (the engine's max_batch), got {self.max_faces}")
        self.prefetch = bool(prefetch) and not self.e.latency_mode
        self._skip = frozenset(_skip_waits)
        if not self._skip <= _RULES:
            raise ValueError(f"_skip_waits: rule letters among {sorted(_RULES)}")
        self.upload = HostFrames(self.e.device, self.batch)
        self.sink = FrameSink(self.e.device, self.batch)
        self._rgb, self._rgb_key = None, None      # the two RGB device slots of the 4:2:0 formats, made at the first such run of a size
        self.staging_ms = []              # host time of each batch's staging memcpy + H2D enqueue in the last run (tools/time_video.py reads it)
        self.trace = None                 # a list: the run appends (batch, name, timing event) at every stage boundary (tools/time_video.py)

    def streams(self):
        """The streams beside the caller's: upload, sink, and the chain's side stream once a prefetch has made it."""
        return [s for s in (self.upload.stream, self.sink.stream, self.chain._side) if s is not None]

    # ---- everything that can be refused, before anything is enqueued
    @staticmethod
    def _format(pixel_format, matrix, full_range):
        """-> None for rgb24, else the (layout, matrix, full_range) names tail.yuv_to_rgb takes, checked."""
        from . import tail
        if pixel_format not in PIXEL_FORMATS:
            raise ValueError(f"pixel_format: {pixel_format!r} is none of {PIXEL_FORMATS}")
        if pixel_format == "rgb24":
            return None
        tail.yuv_format("swap_video", pixel_format, matrix, full_range)
        return pixel_format, matrix, bool(full_range)

    def _check(self, frames, lmk, source_id, slots, frame_index, masks, parse, logits_fn, fmt=None):
        import torch
        src = frames if isinstance(frames, _Source) else _Source(frames, yuv=fmt is not None)
        if src.n and fmt is not None and max(src.hw) > 16384:
            raise ValueError(f"frames: 4:2:0 frames of {src.hw[0]} x {src.hw[1]} are above 16384 a side")
        if src.n and min(src.hw) < 1:
            raise ValueError(f"frames: empty frames ({src.hw[0]} x {src.hw[1]})")
        given = [k for k, v in (("masks", masks is not None), ("parse", bool(parse)), ("logits_fn", logits_fn is not None)) if v]
        if len(given) != 1:
            raise ValueError("masks / parse / logits_fn: pass exactly one mask source, got " + (" and ".join(given) if given else "none"))
        if parse and not self.e.has_parser:
            raise RuntimeError("parse: parse=True, but the engine holds no face parser (pass parser= to can_swapper or the 'parser' state-dict)")
        if logits_fn is not None and not callable(logits_fn):
            raise ValueError("logits_fn: expected a callable pixel_values -> logits")
        fi = None if frame_index is None else _frame_index(frame_index.cpu() if isinstance(frame_index, torch.Tensor) else frame_index, src.n)
        B = src.n if fi is None else int(fi.shape[0])
        lmk = np.asarray(lmk)
        if lmk.ndim != 3 or lmk.shape[0] != B or lmk.shape[2] != 2:
            raise ValueError(f"lmk: expected ({B}, n_points, 2) landmarks, one set per face, got {tuple(lmk.shape)}")
        if masks is not None:
            if not hasattr(masks, "shape"):
                masks = np.asarray(masks)
            if tuple(masks.shape) != (B, 512, 512) or str(masks.dtype).split(".")[-1] != "uint8":
                raise ValueError(f"masks: expected ({B}, 512, 512) uint8 0/1 masks, one per face, got {tuple(masks.shape)} {masks.dtype}")
        if slots is not None:
            if source_id is not None:
                raise ValueError("slots: identity slots take the place of source_id; pass one of the two")
            slots = [int(k) for k in slots]
            if len(slots) != B:
                raise ValueError(f"slots: expected {B} identity slots, one per face, got {len(slots)}")
        elif source_id is None:
            if not self.e._ids:
                raise ValueError("source_id: no identity has been set on the engine; pass source_id or slots")
        else:
            if not isinstance(source_id, torch.Tensor):
                source_id = torch.as_tensor(np.asarray(source_id))
            if source_id.numel() % 512 or source_id.numel() // 512 not in (1, B):
                raise ValueError(f"source_id: expected (1, 512) or ({B}, 512), got {tuple(source_id.shape)}")
        plan = plan_batches(src.n, fi, self.batch, self.max_faces)
        return src, lmk, source_id, slots, fi, masks, plan

    def run(self, frames, lmk, source_id=None, *, slots=None, frame_index=None, masks=None, parse=False, logits_fn=None, pixel_format="rgb24",
            matrix="bt601", full_range=False, _into=None, **crop_cfg):
        """-> a generator of (f0, f1, view) in frame order: view the pinned (f1 - f0, Ho, Wo, 3) u8 array of the pasted-back frames [f0, f1),
        valid until the next next().
        pixel_format "nv12" or "i420" (ffmpeg's yuv420p), with matrix "bt601" / "bt709" and full_range: frames and the views are 4:2:0,
        (N, 3 Ho / 2, Wo) uint8 - an array, a CPU tensor or a sequence of (3 Ho / 2, Wo) arrays - converted on the device both ways; what the
        paste-back did not change comes back byte for byte (the module's text).
        frames: (N, Ho, Wo, 3) uint8 ndarray, a sequence of N (Ho, Wo, 3) uint8 arrays, or a CPU tensor (a pinned one is uploaded from its own
        memory); never written.  lmk (B, n_points, 2): the landmarks of each face, host.  frame_index: the frame of each of the B faces
        (non-decreasing; a frame may hold several faces or none), None: one face per frame.  source_id (1, 512) for all faces or (B, 512), or
        slots (B identity slots set with set_identity).  The masks come from exactly one of masks ((B, 512, 512) u8 0/1, host or device),
        parse=True (the engine's parser) and logits_fn (the caller's parser network: logits_fn(chain.parser_input(crops)) -> logits
        (n, C, 128, 128), called on the caller's stream once per batch with a face, in order).  crop_cfg: chain.crop's dsize, scale, vy_ratio,
        flag_do_rot.  Every argument is checked here, before anything is enqueued and before the first next()."""
        for k in crop_cfg:
            if k not in ("dsize", "scale", "vy_ratio", "flag_do_rot"):
                raise TypeError(f"run() got an unexpected keyword argument {k!r}")
        fmt = self._format(pixel_format, matrix, full_range)
        checked = self._check(frames, lmk, source_id, slots, frame_index, masks, parse, logits_fn, fmt)
        return self._run(*checked, bool(parse), logits_fn, _into, crop_cfg, fmt)

    def swap_video(self, frames, lmk, source_id=None, *, out=None, **kw):
        """run() drained into out, an (N, Ho, Wo, 3) uint8 ndarray or CPU tensor - (N, 3 Ho / 2, Wo) in a 4:2:0 pixel_format - (allocated when
        None) -> out.  A pinned contiguous tensor is downloaded into directly."""
        import torch
        src = _Source(frames, yuv=self._format(kw.get("pixel_format", "rgb24"), kw.get("matrix", "bt601"), kw.get("full_range", False)) is not None)
        shape = (src.n,) + src.frame
        direct = None
        if out is None:
            out = np.empty(shape, np.uint8)
        if isinstance(out, torch.Tensor):
            if out.device.type != "cpu" or out.dtype != torch.uint8 or tuple(out.shape) != shape:
                raise ValueError(f"out: expected a CPU uint8 tensor of shape {shape}, got {tuple(out.shape)} {out.dtype} on {out.device}")
            if out.is_pinned() and out.is_contiguous():
                direct = out
            dst = out
        elif isinstance(out, np.ndarray):
            if out.dtype != np.uint8 or out.shape != shape or not out.flags.writeable:
                raise ValueError(f"out: expected a writeable uint8 array of shape {shape}, got {out.shape} {out.dtype}")
            dst = torch.from_numpy(out) if all(s >= 0 for s in out.strides) else None
        else:
            raise ValueError(f"out: expected an ndarray or a CPU tensor of shape {shape}, got {type(out).__name__}")
        for f0, f1, view in self.run(src, lmk, source_id, _into=direct, **kw):
            if direct is not None:
                continue
            if dst is not None:
                dst[f0:f1].copy_(torch.from_numpy(view))
            else:
                np.copyto(out[f0:f1], view)
        return out

    # ---- the loop
    def _run(self, src, lmk, source_id, slots, fi, masks, plan, parse, logits_fn, into, crop_cfg, fmt=None):
        import time
        import torch
        from . import tail
        if not plan:
            return
        e, chain, up, sink, skip = self.e, self.chain, self.upload, self.sink, self._skip
        main = torch.cuda.current_stream(e.device)
        self.staging_ms = []
        try:
            up.reserve(*src.hw, yuv=src.yuv)
            if into is None:
                sink.reserve(*src.hw, yuv=src.yuv)
            if fmt is not None and self._rgb_key != (src.hw, self.batch):                     # the RGB slots of the 4:2:0 formats: the caller's stream only
                self._rgb = None
                self._rgb = [torch.empty((self.batch,) + src.hw + (3,), dtype=torch.uint8, device=e.device) for _ in range(2)]
                self._rgb_key = (src.hw, self.batch)
            if source_id is not None:
                source_id = source_id.detach().to(e.device).float().reshape(-1, 512)
            if masks is not None and not isinstance(masks, torch.Tensor):
                masks = torch.from_numpy(masks) if masks.flags.writeable else torch.from_numpy(masks.copy())

            def marker(k):
                if self.trace is None:
                    return _no_mark

                def mark(name):
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(torch.cuda.current_stream(e.device))
                    self.trace.append((k, name, ev))
                return mark

            def stage(k):
                """Steps 1 and 2 for batch k."""
                f0, f1, b0, b1 = plan[k]
                s, mark = k % 2, marker(k)
                t0 = time.perf_counter()
                dev = up.upload(src, f0, f1, s, skip, mark)
                self.staging_ms.append((time.perf_counter() - t0) * 1e3)
                mark("crop_queued")
                if "b" not in skip:
                    main.wait_event(up.copied[s])                                             # rule b
                mark("crop_begin")
                st = {"k": k, "span": (f0, f1), "slot": s, "dev": dev, "faces": b1 - b0}
                if fmt is not None and b1 > b0:                                               # a batch without a face stays as it was uploaded
                    st["yuv"], dev = dev, tail.yuv_to_rgb(e, dev, *fmt, out=self._rgb[s][: f1 - f0])
                    st["dev"] = dev
                    mark("rgb_ready")
                if b1 > b0:
                    idx = np.arange(f1 - f0, dtype=np.int32) if fi is None else (fi[b0:b1] - f0).astype(np.int32)
                    c = chain.crop(dev, lmk[b0:b1], frame_index=idx, **crop_cfg)
                    m = lg = None
                    if masks is not None:
                        m = masks[b0:b1].to(e.device, non_blocking=True)
                    elif logits_fn is not None:
                        lg = logits_fn(chain.parser_input(c["crops"]))
                    mark("crop_end")
                    if self.prefetch and m is not None:   # finished masks only: with logits (logits_fn, parse) stage A runs in-line
                        chain.prefetch(c["crops"], m, lg, parse)
                    sid = None if source_id is None else (source_id if source_id.shape[0] == 1 else source_id[b0:b1])
                    st.update(crops=c["crops"], M_c2o=c["M_c2o"], masks=m, logits=lg, index=idx, source_id=sid,
                              slots=None if slots is None else slots[b0:b1])
                return st

            def swap(st):
                """Steps 3 and 4 for a staged batch."""
                s, dev, mark = st["slot"], st["dev"], marker(st["k"])
                mark("chain_begin")
                if st["faces"]:
                    chain(st["crops"], st["masks"], st["M_c2o"], dev, st["source_id"], slots=st["slots"], out=dev, logits=st["logits"],
                          parse=parse, frame_index=st["index"])
                    if fmt is not None:
                        mark("paste_end")
                        dev = tail.rgb_to_yuv(e, dev, *fmt, keep=st["yuv"])                   # back into the YUV slot the batch came in
                sink.pasted[s].record(main)
                mark("chain_end")
                f0, f1 = st["span"]
                st["host"] = sink.download(dev, s, None if into is None else into[f0:f1], skip, mark)
                up.consumed[s].record(sink.stream)

            def finish(st):
                """Step 5: rule e."""
                sink.done[st["slot"]].synchronize()
                return st["span"][0], st["span"][1], st["host"].numpy()

            nxt, waiting = stage(0), None
            for k in range(len(plan)):
                cur, nxt = nxt, (stage(k + 1) if k + 1 < len(plan) else None)
                swap(cur)
                if waiting is not None:
                    yield finish(waiting)
                waiting = cur
            yield finish(waiting)
        finally:                                                                              # rule f
            self.close()

    def close(self):
        """Rule f: staged batches are dropped, the three streams joined to the caller's stream, and both device slots marked as consumed
        there - a batch that was cropped, or pasted, but never downloaded left work on the caller's stream that reads or writes its slot, and
        the next upload into that slot waits for it.  Runs at the end of every run, also after break or an exception."""
        import torch
        main = torch.cuda.current_stream(self.e.device)
        self.chain.drop_prefetches()
        main.wait_stream(self.upload.stream)
        main.wait_stream(self.sink.stream)
        for ev in self.upload.consumed:
            ev.record(main)
