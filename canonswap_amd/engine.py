"""Thin Python handle over the C ABI (include/canonswap_hip.h).

PyTorch is plumbing here: it owns the caller-visible device tensors and the HIP stream; every operation on
the generator path is a HIP kernel launched by libcanonswap_hip.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, pack


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def u8_images(x, batch, least, name, who):
    """Argument `name` of `who` as 8-bit RGB images, tensor or array, host or device: with batch (B,H,W,3) uint8, B >= least, without ONE
    (H,W,3) uint8 image, H and W at least 1 -> the tensor where it lies (the caller uploads), or ValueError.  The one text of this check
    for every wrapper of the package."""
    t = torch.as_tensor(x)
    if t.dtype != torch.uint8 or t.dim() != (4 if batch else 3) or t.shape[-1] != 3 or min(t.shape[-3:]) < 1 or (batch and t.shape[0] < least):
        want = f"(B,H,W,3) uint8 frames or crops, B >= {least}" if batch else "ONE (H,W,3) uint8 image"
        raise ValueError(f"{who}: {name} must be {want}, got {tuple(t.shape)} {t.dtype}")
    return t


class Engine:
    """One engine per device; not thread-safe (same contract as the C ABI)."""

    def __init__(self, device_id: int = 0, max_batch: int = 8, latency_mode: bool = False):
        if not torch.cuda.is_available():
            raise RuntimeError("canonswap_amd.Engine needs a ROCm device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(f"cuda:{device_id}")
        self.max_batch = max_batch
        self.h = C.c_void_p()
        _lib.call("cs_create", device_id, max_batch, C.byref(self.h))
        self.latency_mode = bool(latency_mode)
        if latency_mode:         # BASELINE configs[1]: the one-frame forms (conv_lat, split-K, 2-row volume segments; see cs_set_latency_mode)
            self._call("cs_set_latency_mode", 1)
        self._ids = []            # resident identities: [slot, device copy (512,), last tensor seen, its _version, use tick]
        self._tick = 0
        self.parser_cfg = None    # geometry of the face parser the loaded blobs hold ("P.cfg"), or None
        self._scratch_last = {}   # scratch group (_lib.SCRATCH) -> the torch stream that used it last (_call)
        self._tables = {}         # device_table()

    def close(self):
        if getattr(self, "h", None):
            _lib.call("cs_destroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- weights
    def load_state_dicts(self, state_dicts: dict):
        """Ingest the reference's six state-dicts (src/can_swap_e2e.py:87-100 key layout)."""
        self.load_blobs(pack.build_blobs(state_dicts))

    def load_blobs(self, blobs: dict):
        """Upload packed weight blobs (pack.build_blobs): the load-time transform runs once; N ranks of one node can share its result
        (bench.py packs on rank 0 and hands the blobs over through /dev/shm)."""
        for name, arr in blobs.items():
            arr = np.ascontiguousarray(arr)
            self._call("cs_upload", name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes, what=f"cs_upload({name})")
        self._call("cs_finalize_weights")
        self._ids = []
        if "P.cfg" in blobs:
            c = [int(v) for v in np.asarray(blobs["P.cfg"]).reshape(-1)]
            self.parser_cfg = {"depths": c[0:4], "widths": c[4:8], "heads": c[8:12], "sr": c[12:16], "mlp": c[16], "D": c[17], "L": c[18]}

    def _stream(self):
        return torch.cuda.current_stream(self.device)

    def _call(self, name, *args, what=None):
        """Entry point `name` on this engine: the handle first, torch's current stream of the engine's device last where the entry point takes
        one, tensors from that device only (_lib.call), under the package's one device guard (the C side keeps its own).  An entry point that
        uses a scratch group of the engine (_lib.SCRATCH) first makes its stream wait for the stream that used the group last, where that is
        another one: every cross-stream ordering of engine-owned memory is made here, and no call site places a wait."""
        if name in _lib.TAKES_STREAM:
            cur = self._stream()
            group = _lib.SCRATCH.get(name)
            if group is not None:
                last = self._scratch_last.get(group)
                if last is not None and last != cur:
                    cur.wait_stream(last)
                self._scratch_last[group] = cur
            args += (cur.cuda_stream,)
        with torch.cuda.device(self.device):
            return _lib.call(name, self.h, *args, what=what, device=self.device)

    def _in(self, t, shape_tail=None):
        if not isinstance(t, torch.Tensor):
            raise TypeError("expected a torch.Tensor")
        if t.device != self.device:
            t = t.to(self.device)
        t = t.contiguous().float()
        if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
            raise ValueError(f"expected shape (B, {', '.join(map(str, shape_tail))}), got {tuple(t.shape)}")
        if t.shape[0] < 1 or t.shape[0] > self.max_batch:
            raise ValueError(f"batch {t.shape[0]} outside [1, {self.max_batch}]")
        return t

    @staticmethod
    def _same_batch(*ts):
        n = {int(t.shape[0]) for t in ts if t is not None}
        if len(n) != 1:
            raise ValueError(f"inputs disagree on the batch size: {sorted(n)}")

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _out(self, t, shape, dtype):
        """A caller-provided output buffer must be exactly what the C ABI will write: device, dtype, shape, contiguous."""
        if t is None:
            return self._new(*shape, dtype=dtype)
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous():
            raise ValueError(f"output buffer must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}")
        return t

    def device_table(self, key, build):
        """The small constant table `key` on the engine's device: build() -> a numpy array, made and uploaded once per engine."""
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = torch.from_numpy(build()).to(self.device)
            torch.cuda.current_stream(self.device).synchronize()      # once: later calls may come from any stream
        return t

    def set_identity(self, source_id: torch.Tensor, slot: int = 0):
        """Per-identity precompute of T's modulated weights (adaptive_modulate.py:148-155) into an identity slot.
        source_id: (1,512) or (512,)."""
        sid = source_id.detach().to(self.device).float().reshape(-1, 512)
        if sid.shape[0] != 1:
            raise ValueError("set_identity takes one identity; pass several rows to swap()/swap_frames() instead")
        sid = sid[0].contiguous().clone()
        self._call("cs_set_identity", slot, sid)
        self._ids = [r for r in self._ids if r[0] != slot]
        self._multi = None
        self._tick += 1
        self._ids.append([slot, sid, None, None, self._tick])
        return slot

    def _slot_of_row(self, row: torch.Tensor, src=None):
        """Slot that holds identity `row` (512 floats on the device), computing it into the least recently used slot if needed.
        Identities are compared by VALUE (2 KB), never by address: the allocator reuses addresses of freed tensors."""
        self._tick += 1
        for r in self._ids:
            if torch.equal(r[1], row):
                r[4] = self._tick
                return r[0]
        used = {r[0] for r in self._ids}
        free = [k for k in range(_lib.MAX_IDENTITY_SLOTS) if k not in used]
        slot = free[0] if free else min(self._ids, key=lambda r: r[4])[0]
        return self.set_identity(row, slot)

    def identity_slots(self, source_id: torch.Tensor, B: int):
        """Per-sample identity slots for a (1,512), (512,) or (B,512) source_id (the reference's per-sample dlatents)."""
        # fast path of the per-frame loop: the very same tensor object, unmodified since it was resolved (a strong reference
        # is kept, so its address cannot have been recycled)
        for r in self._ids:
            if r[2] is source_id and r[3] == source_id._version and source_id.numel() == 512:
                self._tick += 1
                r[4] = self._tick
                return [r[0]] * B
        mc = getattr(self, "_multi", None)          # the same (B, 512) tensor object as last time, unmodified: slots are known
        if mc is not None and mc[0] is source_id and mc[1] == source_id._version and len(mc[2]) >= B and \
                all(any(r[0] == k for r in self._ids) for k in set(mc[2][:B])):
            return mc[2][:B]
        sid = source_id.detach().to(self.device).float().reshape(-1, 512)
        if sid.shape[0] not in (1, B):
            raise ValueError(f"source_id holds {sid.shape[0]} identities for a batch of {B}")
        uniq, inv = torch.unique(sid, dim=0, return_inverse=True)
        if uniq.shape[0] > _lib.MAX_IDENTITY_SLOTS:
            raise ValueError(f"{uniq.shape[0]} distinct identities in one batch exceed the {_lib.MAX_IDENTITY_SLOTS} identity slots")
        slot_of = [self._slot_of_row(uniq[k].contiguous()) for k in range(uniq.shape[0])]
        if len(set(slot_of)) != len(slot_of):       # an eviction inside this very batch: cannot happen with <= MAX slots
            raise RuntimeError("identity slot assignment collided")
        slots = [slot_of[int(k)] for k in inv.tolist()]
        if sid.shape[0] == B and B > 1:
            self._multi = (source_id, source_id._version, slots)
        if sid.shape[0] == 1:
            slots = slots * B
            for r in self._ids:
                if r[0] == slots[0]:
                    r[2], r[3] = source_id, source_id._version
        return slots

    def ensure_identity(self, source_id: torch.Tensor):
        return self.identity_slots(source_id, 1)[0]

    def _default_slots(self, B):
        if not self._ids:
            raise RuntimeError("no identity has been set (cs_set_identity): pass source_id or call set_identity first")
        return [max(self._ids, key=lambda r: r[4])[0]] * B

    @staticmethod
    def _slot_array(slots):
        return (C.c_int * len(slots))(*slots)

    # ---------------------------------------------------------------- stages
    def extract_feature_3d(self, img):
        img = self._in(img, (3, 256, 256))
        out = self._new(img.shape[0], 32, 16, 64, 64)
        self._call("cs_extract_feature_3d", img.shape[0], img, out)
        return out

    def warp(self, f, kp_source, kp_driving):
        f = self._in(f, (32, 16, 64, 64)); ks = self._in(kp_source, (21, 3)); kd = self._in(kp_driving, (21, 3))
        self._same_batch(f, ks, kd)
        B = f.shape[0]
        out, occ = self._new(B, 32, 16, 64, 64), self._new(B, 1, 64, 64)
        self._call("cs_warp", B, f, ks, kd, out, occ)
        return out, occ

    def warp_out(self, f, occ=None):
        f = self._in(f, (32, 16, 64, 64))
        B = f.shape[0]
        occ = None if occ is None else self._in(occ, (1, 64, 64))
        self._same_batch(f, occ)
        seg = self._new(B, 256, 64, 64)
        self._call("cs_warp_out", B, f, occ, seg)
        return seg

    def swap(self, f, source_id=None):
        """transfer_model2.forward(x, dlatents): source_id (1,512) or one row per sample (adaptive_modulate.py:157-167)."""
        f = self._in(f, (32, 16, 64, 64))
        B = f.shape[0]
        slots = self.identity_slots(source_id, B) if source_id is not None else self._default_slots(B)
        out = self._new(*f.shape)
        self._call("cs_swap_ids", self._slot_array(slots), B, f, out)
        return out

    def refine(self, f):
        f = self._in(f, (32, 16, 64, 64))
        out = self._new(*f.shape)
        self._call("cs_refine", f.shape[0], f, out)
        return out

    def warp_forward(self, f, kp_driving, kp_source):
        f = self._in(f, (32, 16, 64, 64)); kd = self._in(kp_driving, (21, 3)); ks = self._in(kp_source, (21, 3))
        self._same_batch(f, ks, kd)
        B = f.shape[0]
        occ, deform, seg = self._new(B, 1, 64, 64), self._new(B, 16, 64, 64, 3), self._new(B, 256, 64, 64)
        self._call("cs_warp_forward", B, f, kd, ks, occ, deform, seg)
        return {"occlusion_map": occ, "deformation": deform, "out": seg}

    def spade_decode(self, seg):
        seg = self._in(seg, (256, 64, 64))
        img = self._new(seg.shape[0], 3, 512, 512)
        self._call("cs_spade_decode", seg.shape[0], seg, img)
        return img

    def motion_extract(self, img):
        """MotionExtractor.forward (motion_extractor.py:33-35): Bx3x256x256 in [0,1] -> dict of raw head outputs."""
        out = self.motion_extract_raw(img)
        res, o = {}, 0
        for k, n in pack.M_HEADS:
            res[k] = out[:, o:o + n].contiguous()
            o += n
        return res

    def motion_keypoints(self, raw, want_rot=False, out=None):
        """Key-points from motion_extract's raw head outputs (B, 328), on the device: get_kp_info's refinement + get_rotation_matrix +
        transform_keypoint (can_swap_e2e.py:192-197, 228-256; camera.py:14-73) -> x_t (B,21,3), x_can = scale * kp (B,21,3)
        (can_swap_pipeline_e2e.py:243)[, R (B,3,3)]."""
        raw = self._in(raw, (328,))
        B = raw.shape[0]
        x_t, x_can = (self._out(o, (B, 21, 3), torch.float32) for o in (out if out is not None else (None, None)))
        rot = self._new(B, 3, 3) if want_rot else None
        self._call("cs_motion_keypoints", B, raw, x_t, x_can, rot)
        return (x_t, x_can, rot) if want_rot else (x_t, x_can)

    def motion_extract_raw(self, img, out=None):
        """cs_motion_extract without the per-head split: (B, 328) fp32."""
        img = self._in(img, (3, 256, 256))
        out = self._out(out, (img.shape[0], 328), torch.float32)
        self._call("cs_motion_extract", img.shape[0], img, out)
        return out

    def pack_u8(self, img):
        img = self._in(img)
        B, _, H, W = img.shape
        out = self._new(B, H, W, 3, dtype=torch.uint8)
        self._call("cs_pack_u8", B, img, out, H, W)
        return out

    def unpack_u8(self, img_u8):
        """BxHxWx3 uint8 (host or device) -> Bx3xHxW fp32 in [0,1] on the device (prepare_source / prepare_videos arithmetic)."""
        t = u8_images(img_u8, True, 0, "img_u8", "unpack_u8").to(self.device).contiguous()
        B, H, W, _ = t.shape
        out = self._new(B, 3, H, W)
        self._call("cs_unpack_u8", B, t, out, H, W)
        return out

    def swap_frames(self, img, x_t, x_can, source_id=None, want_f32=True, want_u8=False, debug=False,
                    out_f32=None, out_u8=None, slots=None, out_rec=None, out_swap=None):
        """Whole loop body of can_swap_pipeline_e2e.py:242-263 for B frames, on device.
        slots: identity slot per frame (ints, set with set_identity) instead of `source_id` rows - no identity lookup at all
        (multi-stream callers that placed their identities themselves).
        debug: also the two canonical-space decodes of :248-250 and :257-259, "rec_can" and "swap_can" (B,3,512,512) fp32; out_rec / out_swap:
        the caller's buffers for them (either one asks for its decode, with or without debug)."""
        img = self._in(img, (3, 256, 256)); x_t = self._in(x_t, (21, 3)); x_can = self._in(x_can, (21, 3))
        self._same_batch(img, x_t, x_can)
        B = img.shape[0]
        if slots is not None:
            slots = [int(k) for k in slots]
            if len(slots) != B or source_id is not None:
                raise ValueError("slots: one identity slot per frame, and no source_id")
        else:
            slots = self.identity_slots(source_id, B) if source_id is not None else self._default_slots(B)
        out_f32 = self._out(out_f32, (B, 3, 512, 512), torch.float32) if (want_f32 or out_f32 is not None) else None
        out_u8 = self._out(out_u8, (B, 512, 512, 3), torch.uint8) if (want_u8 or out_u8 is not None) else None
        rec = self._out(out_rec, (B, 3, 512, 512), torch.float32) if (debug or out_rec is not None) else None
        swp = self._out(out_swap, (B, 3, 512, 512), torch.float32) if (debug or out_swap is not None) else None
        self._call("cs_swap_frames_ids", self._slot_array(slots), B, img, x_t, x_can, out_f32, out_u8, rec, swp)
        res = {"out": out_f32, "out_u8": out_u8}
        if debug or rec is not None or swp is not None:
            res.update(rec_can=rec, swap_can=swp)
        return res

    def animate_frames(self, f, kp_source, kp_driving, want_f32=True, want_u8=False, out_f32=None, out_u8=None):
        """Per-frame body of can_swap_pipeline_v2i.py:311-312 for B driving frames: one (or B) feature volume(s) f and source
        key-point set(s), B driving key-point sets -> Bx3x512x512."""
        kp_driving = self._in(kp_driving, (21, 3))
        B = kp_driving.shape[0]
        f = self._in(f, (32, 16, 64, 64)); kp_source = self._in(kp_source, (21, 3))
        if f.shape[0] not in (1, B) or kp_source.shape[0] not in (1, B):
            raise ValueError("f and kp_source must hold 1 or B entries")
        out_f32 = self._out(out_f32, (B, 3, 512, 512), torch.float32) if (want_f32 or out_f32 is not None) else None
        out_u8 = self._out(out_u8, (B, 512, 512, 3), torch.uint8) if (want_u8 or out_u8 is not None) else None
        self._call("cs_animate_frames", B, f, f.shape[0], kp_source, kp_source.shape[0], kp_driving, out_f32, out_u8)
        return {"out": out_f32, "out_u8": out_u8}

    def resize_half_bilinear(self, img, out=None):
        """F.interpolate(img, size=(H/2, W/2), mode="bilinear", align_corners=False) at exactly one half (can_swap_pipeline_v2i.py:294):
        (B,C,H,W) fp32, H and W even -> (B,C,H/2,W/2); the 2x2 mean summed rows first, 0.25 * ((a + b) + (c + d))."""
        if not isinstance(img, torch.Tensor) or img.dim() != 4:
            raise ValueError("expected a (B, C, H, W) tensor")
        img = img.to(self.device).contiguous().float()
        B, Cc, H, W = img.shape
        if B < 1 or Cc < 1 or H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError(f"resize_half_bilinear: H and W must be even and the tensor not empty, got {tuple(img.shape)}")
        out = self._out(out, (B, Cc, H // 2, W // 2), torch.float32)
        self._call("cs_resize_half_bilinear", B, Cc, img, H, W, out)
        return out

    def motion_keypoints_driven(self, raw_driving, raw_pose, kp, out=None):
        """The driven key-points of can_swap_pipeline_v2i.py:301-305 on the device: raw_driving (B,328) raw heads of the driving frames,
        raw_pose (1,328) raw heads of the source crop (scale, pose, t), kp (21,3) or (1,21,3) canonical key-points of the swapped canonical
        image -> x_t (B,21,3) = scale_pose * (kp @ R_pose + exp[b]) + (t_x, t_y, 0)."""
        raw_driving = self._in(raw_driving, (328,))
        B = raw_driving.shape[0]
        for name, t, n in (("raw_pose", raw_pose, 328), ("kp", kp, 63)):
            if not isinstance(t, torch.Tensor) or t.numel() != n:
                raise ValueError(f"{name} must hold {n} values (one row)")
        raw_pose = raw_pose.to(self.device).contiguous().float()
        kp = kp.to(self.device).contiguous().float()
        x_t = self._out(out, (B, 21, 3), torch.float32)
        self._call("cs_motion_keypoints_driven", B, raw_driving, raw_pose, kp, x_t)
        return x_t

    # ---------------------------------------------------------------- identity network (getid)
    def identity(self, img, normalize=True, want_raw=False, out=None):
        """can_swapper.getid on the engine (can_swap_e2e.py:102-107): img (B,3,H,W) fp32, any H, W -> nearest resize to 112 x 112 -> the ArcFace
        network -> (B,512), L2-normalised rows with normalize, the network's raw output without; want_raw: (normalised, raw).  Needs the
        "arcface" state-dict among the loaded weights.  The result lives on the device and feeds set_identity / swap_frames as it is."""
        if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.shape[1] != 3 or min(img.shape) < 1:
            raise ValueError("identity expects a (B, 3, H, W) tensor")
        img = self._in(img)
        return self._identity(img.shape[0], img, None, None, img.shape[2], img.shape[3], normalize, want_raw, out)

    def identity_u8(self, crops_u8, lut=None, normalize=True, want_raw=False, out=None):
        """identity() from aligned uint8 crops (B,H,W,3) or (H,W,3), host or device: ID_transform (ToTensor + Normalize,
        can_swap_pipeline_e2e.py:43-46) as a (3,256) table, then getid; lut: another table (tail.id_lut builds them)."""
        from . import tail
        t = torch.as_tensor(crops_u8)
        t = u8_images(t[None] if t.dim() == 3 else t, True, 1, "crops_u8", "identity_u8")
        if t.shape[0] > self.max_batch:
            raise ValueError(f"batch {t.shape[0]} outside [1, {self.max_batch}]")
        t = t.to(self.device).contiguous()
        if lut is None:
            lut = tail.id_lut_on(self)
        else:
            lut = torch.as_tensor(lut, dtype=torch.float32).to(self.device).contiguous()
            if tuple(lut.shape) != (3, 256):
                raise ValueError("lut must be a (3, 256) table")
        return self._identity(t.shape[0], None, t, lut, t.shape[1], t.shape[2], normalize, want_raw, out)

    def _identity(self, B, img, u8, lut, H, W, normalize, want_raw, out):
        idn = self._out(out, (B, 512), torch.float32) if normalize else None
        raw = (self._out(None if normalize else out, (B, 512), torch.float32)) if (want_raw or not normalize) else None
        if u8 is None:
            self._call("cs_identity", B, img, H, W, idn, raw)
        else:
            self._call("cs_identity_u8", B, u8, H, W, lut, idn, raw)
        if normalize:
            return (idn, raw) if want_raw else idn
        return raw

    def identity_read(self, which: int, B: int):
        """cs_op_identity_read: activation `which` (0 stem, 1-4 layer1-4, 5 pre-fc) of the last identity pass as fp32 NCHW (tests)."""
        shape = [(64, 55, 55), (64, 55, 55), (128, 28, 28), (256, 14, 14), (512, 7, 7), (512, 7, 7)][which]
        dst = self._new(B, *shape)
        self._call("cs_op_identity_read", which, B, dst)
        return dst

    # ---------------------------------------------------------------- face parser (SegFormer)
    @property
    def has_parser(self):
        return self.parser_cfg is not None

    def parser(self, pixel_values, out=None):
        """The SegFormer face parser on the engine (can_swap_pipeline_e2e.py:178-182: model(pixel_values).logits): pixel_values (B,3,H,W) fp32, H and W
        multiples of 32 up to 512 x 512 (what parser_input makes of the crops) -> logits (B,L,H/4,W/4) fp32 on the device, the tensor face_masks
        takes.  Needs the "parser" state-dict among the loaded weights.  A workspace of its own: it may be enqueued beside the generator."""
        if not self.has_parser:
            raise RuntimeError("parser: the engine holds no face parser (pass the 'parser' state-dict with the weights)")
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or min(pixel_values.shape) < 1:
            raise ValueError("parser expects a (B, 3, H, W) tensor")
        pv = self._in(pixel_values)
        B, _, H, W = pv.shape
        if H % 32 or W % 32:
            raise ValueError(f"parser: H = {H}, W = {W} (each a multiple of 32)")
        logits = self._out(out, (B, self.parser_cfg["L"], H // 4, W // 4), torch.float32)
        self._call("cs_parser", B, pv, H, W, logits)
        return logits

    def parser_read(self, which: int, B: int, H: int, W: int):
        """cs_op_parser_read: activation `which` (0-3: the encoder stages' outputs, 4: the decode head's map in front of the classifier) of the
        last parser pass, whose input was H x W, as fp32 NCHW (tests)."""
        if not self.has_parser:
            raise RuntimeError("parser_read: the engine holds no face parser")
        c = self.parser_cfg
        shape = (c["D"], H // 4, W // 4) if which == 4 else (c["widths"][which], H >> (which + 2), W >> (which + 2))
        dst = self._new(B, *shape)
        self._call("cs_op_parser_read", which, B, dst)
        return dst

    # ---------------------------------------------------------------- measurement
    def profile_begin(self):
        self._call("cs_profile_begin")

    def profile_end(self):
        ms, cnt, fl, ex = (C.c_double * 3)(), (C.c_long * 3)(), C.c_double(), C.c_double()
        self._call("cs_profile_end", ms, cnt, C.byref(fl))
        self._call("cs_profile_exec_flops", C.byref(ex))
        return {"exec_flops": ex.value,"conv_ms": ms[0], "other_ms": ms[1], "warp_ms": ms[2], "conv_launches": cnt[0], "other_launches": cnt[1],
                "warp_launches": cnt[2], "conv_flops": fl.value}
