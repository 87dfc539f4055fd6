"""The whole device-side frame: the per-frame work of CanSwapPipeline.execute (src/can_swap_pipeline_e2e.py) for B frames per call
without leaving the GPU between the decoded uint8 frame and the pasted-back uint8 frame (SURVEY.md section 8f rows N1-N3 around
the generator).

    reference (per frame, host round trips in brackets)                       here (B frames per launch, all on the device)
    cropper.py:196-204  crop_image: landmarks -> M_o2c, cv2.warpAffine        chain.crop: crop.crop_matrices (host, no image) +
                              of the 1080p frame [host, then upload]           cs_crop_frames
    cropper.py:209  cv2.resize(crop 512 -> 256, INTER_AREA) [host]            cs_prepare_crops
    can_swap_e2e.py:147-163  prepare_videos -> fp32 NCHW [upload]               "
    can_swap_pipeline_e2e.py:111-125  get_kp_info + transform_keypoint         cs_motion_extract + cs_motion_keypoints
                              [seven tensors to the host and back per frame]
    :242-263  F -> warp -> T -> R -> warp_decode                               cs_swap_frames_ids
    :267      parse_output [sync + D2H]                                        (pack_u8 inside cs_swap_frames_ids)
    :171, :180  cv2.resize(crop, 256 x 256) + SegformerImageProcessor          chain.parser_input: cs_parser_input (PIL's two integer passes,
                              [D2H, PIL resize, three numpy passes, upload]     rescale + normalize as a table, fp32 NCHW)
    :183-190  F.interpolate(logits, 512 x 512) -> argmax -> isin               cs_face_masks (with logits=: the parser's logits go in as they
                              [19.9 MB of up-sampled logits per frame]          are; with masks: the caller has run these lines)
    :274      soft_mask(masks[i]) [D2H]                                        cs_soft_erosion_frames
    :279-282  prepare_paste_back + paste_back (two cv2.warpAffine) [host]      cs_paste_back_batch
    (one face per frame; face_detect_crop_multi.py:63-99 finds them all)       chain.crop(frames, lmk, frame_index=) / chain(..., frame_index=):
                                                                               cs_crop_faces, cs_paste_back_faces - B faces in F frames
    :248-250, :257-259, :290  rec_can, I_can, concat_frames (video.py:84-109)  chain(..., concat=True): the two debug decodes of
                              [three images per frame D2H, cv2.resize, hstack]  cs_swap_frames_ids + cs_concat_frames

The loop of a caller:  c = chain.crop(frames, lmk);  frames_out = chain(c["crops"], None, c["M_c2o"], frames, source_id, parse=True)["frames"]
with the face parser among the engine's weights (cs_parser_input + cs_parser + cs_face_masks in stage A, no torch module in the process).  A
caller who runs the parser himself:  logits = model(pixel_values=chain.parser_input(c["crops"])).logits, (B,19,128,128);
chain(c["crops"], None, c["M_c2o"], frames, source_id, logits=logits)  (or, with 0/1 masks made of them: chain(c["crops"], masks, ...)).

Several faces per frame, or none (frame_index: the frame of each face, non-decreasing):  c = chain.crop(frames, lmk, frame_index=fi);
frames_out = chain(c["crops"], None, c["M_c2o"], frames, slots=slot_of_face, parse=True, frame_index=fi)["frames"] - F frames in, F frames out,
every face of a frame pasted in order in one pass, a frame without a face returned as it came.

Frames that start and end in host memory - a whole video: video.VideoSwapper drives this loop in batches, with the upload of the next batch and
the download of the last one beside the generator (video.py).

AnimateChain below is the same for the second program, inference_v2i.py (src/can_swap_pipeline_v2i.py: one source image animated by a
driving video, the driving identity swapped in); its table stands in the class's docstring.

What stays outside (out of scope): face detection and the landmark network (they produce the landmarks), video decode /
encode.  The SegFormer face parser runs on the engine when its weights are loaded (parse=True: cs_parser between cs_parser_input and cs_face_masks).
"""
from __future__ import annotations

import torch

from . import tail
from .engine import Engine, u8_images


class _StagedChain:
    """What the two chains share: engine, SoftErosion module, named buffers and the staging pipeline.  Stage A of a batch (`_stage_a`, the
    subclass's own: everything the generator needs from the crops) runs in-line on the caller's stream, or ahead of time on a side stream
    into one half of a double buffer.  Every stream-ordering rule for the memory FrameChain and AnimateChain own stands here, once; the
    engine's scratch (M, SoftErosion, parser) is ordered between streams by the call path itself, Engine._call."""

    def __init__(self, swapper, kernel_size, threshold, iterations, valid):
        self.sw = swapper
        tail.valid_bits(valid)                                        # raises on a class id the mask word cannot hold
        self.valid = tuple(valid)
        self.e: Engine = swapper.engine
        if swapper.motion_extractor is None:
            raise RuntimeError(f"{type(self).__name__}: the loaded weights hold no 'motion_extractor' state-dict")
        self.se = tail.SoftErosion(self.e, kernel_size, threshold, iterations)
        self._buf = {}
        self._side, self._free, self._pending = None, None, []        # _stage_ahead(): side stream, double buffer

    def _get(self, key, shape, dtype):
        t = self._buf.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.e.device)
            self._buf[key] = t
        return t

    def crop(self, frames_ori, lmk, frame_index=None, **cfg):
        """The cropper's step in front of the chain (cropper.py:196-204, crop.py:429-455): frames_ori (B,Ho,Wo,3) u8 on the device, lmk (B,N,2)
        tracked landmarks (host) -> {"crops" (B,512,512,3) u8 on the device, "M_c2o", "M_o2c" (B,3,3) host, "lmk_crop"}: tail.crop_frames with
        CropConfig's defaults (cfg: dsize, scale, vy_ratio, flag_do_rot, out, want_I).  A new crops tensor per call, so a batch may be cropped
        and prefetched while the one before it runs; stage A reads the crops as it would a caller's.
        frame_index (B host ints, non-decreasing, in [0, F)): B faces in F frames, frames_ori (F,Ho,Wo,3), face b cut from frame frame_index[b]
        (tail.crop_faces); the dict is per face."""
        if frame_index is None:
            return tail.crop_frames(self.e, frames_ori, lmk, **cfg)
        return tail.crop_faces(self.e, frames_ori, lmk, frame_index, **cfg)

    def parser_input(self, crops_u8, **kw):
        """What the caller's face parsing network takes (can_swap_pipeline_e2e.py:171 + :180, can_swap_pipeline_v2i.py:73): crops_u8 (B,512,512,3) or
        (B,256,256,3) u8 -> pixel_values (B,3,512,512) fp32 on the device, tail.parser_input (kw: halve, mean, std, rescale, out, want_u8,
        out_u8).  One launch on the caller's stream that reads the crops and a 3 KB table and writes its own output: it uses no engine scratch,
        so it may run on the caller's stream while a prefetch is in flight on the side stream."""
        return tail.parser_input(self.e, crops_u8, **kw)

    def _concat(self, crops_u8, middle, gen, out):
        """The pipelines' side-by-side frame (video.py:84-109): driving crop | middle panels | gen, tail.concat_frames.  The driving panel is
        the reference's driving_rgb_crop_256x256_lst resized back to 512 (can_swap_pipeline_e2e.py:171 then video.py:99): kind 2 for 512 x 512
        crops (halved, then x 2), kind 1 for 256 x 256 crops (x 2).  middle: [(panel, kind, shared)].  One launch on the caller's stream behind the
        generator; no engine scratch."""
        drv = torch.as_tensor(crops_u8)
        drv = drv[None] if drv.dim() == 3 else drv
        panels = [(drv, 2 if drv.shape[1] == 512 else 1, 0)] + list(middle) + [(gen, 0, 0)]
        return tail.concat_frames(self.e, [p for p, _, _ in panels], kinds=[k for _, k, _ in panels], shared=[f for _, _, f in panels], out=out)

    def _check_stageable(self):
        """Raises where stage A cannot run yet (AnimateChain: no source)."""

    def _mask_or_logits(self, masks, logits, who, parse=False):
        """The parser's result comes as 0/1 masks or as logits (tail.face_masks makes the masks of them), never both, never neither; or, with
        parse=True, from the engine's own parser: then neither is passed, and the engine must hold the network (checked before anything is enqueued)."""
        if parse:
            if masks is not None or logits is not None:
                raise ValueError(f"{who}: parse=True takes the place of masks and logits=; pass neither")
            if not self.e.has_parser:
                raise RuntimeError(f"{who}: parse=True, but the engine holds no face parser (pass parser= to can_swapper or the 'parser' state-dict)")
            return
        if (masks is None) == (logits is None):
            raise ValueError(f"{who}: pass either masks or logits=" + (", not both" if masks is not None else " (got neither)"))

    def _stage_ahead(self, crops_u8, *args):
        """prefetch() of both chains: _stage_a(crops_u8, *args, slot) on the side stream, into the half of the double buffer no staged
        batch holds; the call with the same crops tensor picks the result up (_resolve)."""
        e, name = self.e, type(self).__name__
        if e.latency_mode:
            raise RuntimeError(f"{name}.prefetch: the engine is in latency mode (split-K scratch shared by M and the generator); "
                               "run the chain in-line")
        self._check_stageable()
        if len(self._pending) >= 2:
            raise RuntimeError(f"{name}.prefetch: two batches are already staged (double buffer); run one of them first")
        if self._side is None:
            self._side = torch.cuda.Stream(device=e.device)      # (a high-priority side stream measured the same: 0.933 either way)
            self._free = [torch.cuda.Event(), torch.cuda.Event()]
        slot = 1 - self._pending[0][1] if self._pending else 0      # the half no staged batch holds (they may be run out of order)
        main = torch.cuda.current_stream(e.device)
        self._side.wait_stream(main)                      # the crops (and AnimateChain's source state) were produced on the caller's stream
        self._side.wait_event(self._free[slot])           # the generator that read this half of the double buffer is done
        with torch.cuda.stream(self._side):
            res = self._stage_a(crops_u8, *args, slot)
            ready = torch.cuda.Event()
            ready.record(self._side)
        self._pending.append((crops_u8, slot, res, ready))

    def drop_prefetches(self):
        """Forget staged batches that will not be run (their buffers are reused by the next prefetch).  Their stage A may still be running
        on the side stream, reading the caller's crops and writing the chain's double buffer: the caller's stream waits for it."""
        self._pending = []
        if self._side is not None:
            torch.cuda.current_stream(self.e.device).wait_stream(self._side)

    def _resolve(self, crops_u8, *args):
        """Head of __call__ -> (slot, stage A's result): the staged batch whose crops tensor is this one (slot = its half of the double
        buffer), else stage A in-line (slot None)."""
        main = torch.cuda.current_stream(self.e.device)
        hit = [k for k, q in enumerate(self._pending) if q[0] is crops_u8]
        if hit:
            _, slot, res, ready = self._pending.pop(hit[0])
            main.wait_event(ready)
            return slot, res
        return None, self._stage_a(crops_u8, *args, "inline")

    def _release(self, slot):
        """End of __call__, the generator queued: the next prefetch into this half of the double buffer waits for it."""
        if slot is not None:
            self._free[slot].record(torch.cuda.current_stream(self.e.device))


class FrameChain(_StagedChain):
    """chain = FrameChain(swapper);  frames = chain(crops_u8, masks, M_c2o, frames_ori, source_id)["frames"]"""

    def __init__(self, swapper, kernel_size: int = 21, threshold: float = 0.9, iterations: int = 3, valid=tail.FACE_VALID):
        super().__init__(swapper, kernel_size, threshold, iterations, valid)      # SoftErosion(21, 0.9, 3): can_swap_pipeline_e2e.py:42; valid_list :189

    def crop(self, frames_ori, lmk, frame_index=None, **cfg):
        """_StagedChain.crop for host landmarks, as it is.  lmk a (B,N,2) float32 DEVICE tensor (the tracker's landmarks as they lie): the device
        route, tail.crop_lmk (cfg: dsize, scale, vy_ratio, flag_do_rot, status, status_mark, out, want_I, want_lmk_crop) -> {"crops", "M" (B,18)
        fp32 = M_o2c | M_c2o, "status" (B,) int32[, "I", "lmk_crop"]}, all on the device, in place of the host "M_c2o" / "M_o2c": hand "M" to
        __call__ as M_c2o and "status" as status=, and nothing between the tracker and the paste-back waits for the device."""
        if isinstance(lmk, torch.Tensor) and lmk.is_cuda:
            return tail.crop_lmk(self.e, frames_ori, lmk, frame_index, **cfg)
        return super().crop(frames_ori, lmk, frame_index, **cfg)

    def keypoints(self, I, slot=0):
        """(B,3,256,256) fp32 -> x_t, x_can (B,21,3): make_motion_template's get_kp_info + transform_keypoint and the loop's
        x_can = scale * kp (can_swap_pipeline_e2e.py:111-125, 236-243)."""
        B = I.shape[0]
        raw = self.e.motion_extract_raw(I, out=self._get(("raw", slot), (B, 328), torch.float32))
        return self.e.motion_keypoints(raw, out=(self._get(("x_t", slot), (B, 21, 3), torch.float32), self._get(("x_can", slot), (B, 21, 3), torch.float32)))

    # ---- stage A: everything the generator needs from a batch of crops (input staging + motion extractor).  The reference runs it as a
    # pre-pass over the whole video (prepare_videos + make_motion_template, can_swap_pipeline_e2e.py:196-197) before the swapping loop
    # ... and the soft mask, which depends on the parser's labels only (:274); given the logits, the labels' mask first (:183-190)
    def _stage_a(self, crops_u8, masks, logits, parse, slot):
        t = torch.as_tensor(crops_u8)
        B = t.shape[0] if t.dim() == 4 else 1
        if parse:                                                                                         # :171-182 on the engine
            pv = tail.parser_input(self.e, t, out=self._get(("pv", slot), (B, 3, 512, 512), torch.float32))
            logits = self.e.parser(pv, out=self._get(("logits", slot), (B, self.e.parser_cfg["L"], 128, 128), torch.float32))
        I = tail.prepare_crops(self.e, t, out=self._get(("I", slot), (B, 3, 256, 256), torch.float32))      # cropper.py:209 + can_swap_e2e.py:147-163
        x_t, x_can = self.keypoints(I, slot)                                                              # can_swap_pipeline_e2e.py:111-125, 243
        made = None
        if logits is not None:
            m = made = tail.face_masks(self.e, logits, self.valid, out=self._get(("mask", slot), (B, 512, 512), torch.uint8))
        else:
            m = torch.as_tensor(masks)
        soft = tail.soft_erosion_frames(self.e, m, self.se.weight, self.se.kernel_size, self.se.threshold, self.se.iterations,
                                        out=self._get(("soft", slot), (B,) + tuple(m.shape[-2:]), torch.float32))      # :274
        return I, x_t, x_can, soft, made                      # made: the u8 mask stage A made (logits=, parse=True), None for the caller's masks

    def prefetch(self, crops_u8, masks=None, logits=None, parse=False):
        """Stage A of the NEXT batch on a side stream (masks, logits= or parse=True as in __call__; the engine's parser then runs there too, beside the generator: its workspace is its own), so that it runs beside the generator of the current one
        (M and the staging are bandwidth / latency bound, the generator is matrix-pipe bound): call it before __call__ of the current batch; the next __call__ with
        the same crops tensor picks the result up (the soft masks of that batch included: they depend on the parser's labels only).  M's workspace is its own, the batch's inputs land in the other half of a double buffer.
        Staged batches may be run in any order.  Not on a latency-mode engine: there every small plain conv (M's and the generator's
        alike) runs split-K on the engine's one partial-sum buffer, which M on the side stream and the generator would share.
        NOT YET SAFE with logits= or parse=True beside the generator: the mask stage A makes then came out with a few isolated bytes flipped
        (and the soft mask and frame pixels with them) in about half of the batches staged while the host ran ahead of the device; the cause
        is not found.  With masks= the bytes are the in-line chain's.  video.VideoSwapper stages such batches in-line."""
        self._mask_or_logits(masks, logits, "FrameChain.prefetch", parse)
        self._stage_ahead(crops_u8, masks, logits, parse)

    def __call__(self, crops_u8, masks, M_c2o, frames_ori, source_id=None, slots=None, out=None, keep=False, logits=None, concat=False,
                 concat_out=None, parse=False, frame_index=None, status=None):
        """parse=True (masks None, no logits=): the engine's own face parser makes the logits of the crops in stage A (parser_input -> parser).
        crops_u8 (B,512,512,3) or (B,256,256,3) u8; masks (B,512,512) u8 0/1 or fp32 (the parser's `torch.isin(labels, valid)`), or None
        with logits= (B,C,128,128), (B,C,256,256) or (B,C,512,512) fp32: the parser's logits, masked here (tail.face_masks with the chain's valid);
        M_c2o (B,2,3)/(B,3,3) host; frames_ori (B,Ho,Wo,3) u8; source_id (1,512)/(B,512) or identity slots.
        concat=True: also the frames of the pipeline's side-by-side video (:290, video.py:84-109), "concat" (B,512,2048,3) u8 (into concat_out):
        driving crop | rec_can (:248-250) | I_can (:257-259) | I_p.  The generator then runs its two debug decodes, into chain-owned buffers; without
        concat it runs neither.
        -> {"frames": (B,Ho,Wo,3) u8[, "concat"][, "crops_out", "x_t", "x_can", "I", "soft_mask", "mask" with keep=True, and "rec_can", "swap_can"
        (B,3,512,512) fp32 with keep and concat]}.  "mask": the (B,512,512) u8 0/1 mask stage A made of the logits (logits=, parse=True), None where
        the caller passed masks.  The kept stages are the chain's own buffers, not copies (no launch is added): "mask", "soft_mask", "I", "x_t" and
        "x_can" of a prefetched batch are rewritten by the prefetch after the next one, "crops_out" by the next call.
        frame_index (B host ints, non-decreasing, in [0, F)): B faces in F frames.  Everything above stays per face (B up to the engine's
        max_batch; crops, masks / logits, M_c2o, source_id / slots, "concat", the kept stages); frames_ori, out and "frames" are (F,Ho,Wo,3): face b
        is pasted into frame frame_index[b], the faces of a frame in their order (tail.paste_back_faces), a frame without a face comes back as
        it is.  B = 0 (crops (0,512,512,3), F >= 1): no generator runs, "frames" is frames_ori (copied into out, if given).
        M_c2o a (B,18) float32 DEVICE tensor (chain.crop's "M" of device landmarks, M_c2o = M[:, 9:]): the paste-back reads the matrices where
        they lie (tail.paste_back_faces_dev; frame_index None: arange(B)), status= (B,) int32 on the device, optional: crop's "status", a face
        with a non-zero entry is not pasted.  Host matrices go the way they went."""
        e = self.e
        if frame_index is not None and torch.as_tensor(crops_u8).shape[0] == 0:
            return self._no_faces(frames_ori, frame_index, out)
        self._mask_or_logits(masks, logits, "FrameChain", parse)
        on_device = isinstance(M_c2o, torch.Tensor) and M_c2o.is_cuda      # the (B,18) matrices of chain.crop's device route
        if status is not None and not on_device:
            raise ValueError("FrameChain: status= goes with a (B,18) device M_c2o (chain.crop of device landmarks)")
        if on_device and frame_index is None:
            frame_index = range(len(crops_u8))
        if frame_index is not None:                                   # before anything is enqueued: the error names the argument
            frame_index = tail.frame_index_of(frame_index, len(crops_u8), len(frames_ori))
        slot, (I, x_t, x_can, soft, made) = self._resolve(crops_u8, masks, logits, parse)
        B = I.shape[0]
        rec = self._get("rec_can", (B, 3, 512, 512), torch.float32) if concat else None
        swp = self._get("swap_can", (B, 3, 512, 512), torch.float32) if concat else None
        gen = e.swap_frames(I, x_t, x_can, source_id, want_f32=False, want_u8=True, slots=slots,
                            out_u8=self._get("gen", (B, 512, 512, 3), torch.uint8), out_rec=rec, out_swap=swp)["out_u8"]   # :242-267
        if on_device:                                                                           # :279-282, the matrices read where they lie
            frames = tail.paste_back_faces_dev(e, gen, soft, M_c2o, frame_index, frames_ori, status=status, out=out)
        elif frame_index is None:
            frames = tail.paste_back_batch(e, gen, soft, M_c2o, frames_ori, out=out)            # :279-282
        else:
            frames = tail.paste_back_faces(e, gen, soft, M_c2o, frame_index, frames_ori, out=out)      # :279-282 once per face of a frame
        self._release(slot)
        res = {"frames": frames}
        if concat:
            res["concat"] = self._concat(crops_u8, [(rec, 3, 0), (swp, 3, 0)], gen, concat_out)  # :290
        if keep:
            res.update(crops_out=gen, x_t=x_t, x_can=x_can, soft_mask=soft, I=I, mask=made)
            if concat:
                res.update(rec_can=rec, swap_can=swp)
        return res


    def _no_faces(self, frames_ori, frame_index, out):
        """A batch of frames in which nobody was found: nothing to generate.  The frames come back as they are, copied into `out` if given
        (cs_paste_back_faces with B = 0)."""
        fr = u8_images(frames_ori, True, 1, "frames_ori", "FrameChain")
        tail.frame_index_of(frame_index, 0, fr.shape[0])
        if out is None:
            return {"frames": fr.to(self.e.device)}
        none = torch.empty((0, 512, 512, 3), dtype=torch.uint8, device=self.e.device)
        return {"frames": tail.paste_back_faces(self.e, none, none[..., 0].float(), None, frame_index, fr, out=out)}


class AnimateChain(_StagedChain):
    """chain = AnimateChain(swapper);  chain.set_source(crop_u8, mask, M_c2o, img_ori, driving_id);  frames = chain(driving_crops_u8)["frames"]

    The device-side frame of CanSwapPipeline.execute of src/can_swap_pipeline_v2i.py, B driving frames per call:

        reference (host round trips in brackets)                                   here
        once per source image and driving identity                                 set_source
        :86-90    prepare_source, get_kp_info, extract_feature_3d, transform_keypoint   cs_prepare_crops, cs_motion_extract, cs_motion_keypoints,
                                                                                   cs_extract_feature_3d
        :92-97    warp(f_s, x_s, scale * kp)                                       cs_warp
        :286-289  swap_module + conv_decode                                        cs_swap_ids, cs_warp_out + cs_spade_decode
        :294      F.interpolate(swap_can, (256, 256), bilinear)                    cs_resize_half_bilinear
        :297-298  get_kp_info + transform_keypoint of swap_can_256                 cs_motion_extract + cs_motion_keypoints
        :308      extract_feature_3d(swap_can_256), there once per frame           cs_extract_feature_3d, once (loop-invariant)
        :73       image_processor(img_crop_256x256) [host: PIL, numpy, upload]     cs_parser_input (chain.parser_input(crop): the parser's pixel_values)
        :76-83    F.interpolate(logits, 512 x 512) -> argmax -> isin               cs_face_masks (set_source(..., logits=))
        :255-258  soft_mask + prepare_paste_back [D2H, cv2.warpAffine]             cs_soft_erosion_frames + cs_warp_affine_f32
        per driving frame                                                          __call__
        :223-238  cv2.resize + prepare_videos + make_motion_template [seven tensors D2H]   cs_prepare_crops + cs_motion_extract
        :301-305  x_t_2 = scale_swap * (kp_swap @ R_swap + delta_t) + t_swap        cs_motion_keypoints_driven
        :309      warp_decode(f_swap_can_2, x_swap, x_t_2)                         cs_animate_frames
        :312-321  parse_output [sync + D2H] + paste_back into a copy of the image   (pack_u8 inside cs_animate_frames) cs_paste_back_shared
        :328      concat_frames (video.py:84-109) [cv2.resize, hstack on the host]  chain(..., concat=True): cs_concat_frames, the one I_can shared

    There is no refine module in this pipeline.  The crops, the source's and the driving frames', come from chain.crop (cropper.py:144-152,
    196-204): `c = chain.crop(img[None], lmk)`, then `set_source(c["crops"][0], mask, c["M_c2o"][0], img, driving_id)`.  Outside: everything
    FrameChain leaves outside and getid (the driving identity is passed in).  With the face parser among the engine's weights,
    set_source(crop, None, M_c2o, img, driving_id, parse=True) runs it on the crop."""

    def __init__(self, swapper, kernel_size: int = 21, threshold: float = 0.9, iterations: int = 2, valid=tail.FACE_VALID):
        super().__init__(swapper, kernel_size, threshold, iterations, valid)      # SoftErosion(21, 0.9, 2): can_swap_pipeline_v2i.py:43; valid_list :82
        self._src = None                                              # source_state()
        self._I_can = None                                            # set_source's I_can, the middle panel of concat=True; beside _src, not in it

    # ---- once per (source image, driving identity)
    def set_source(self, crop_u8, mask, M_c2o, img_ori, driving_id, logits=None, parse=False):
        """crop_u8 (512,512,3) or (256,256,3) u8: the cropper's crop of the source image; mask (Hm,Wm) u8 0/1 or fp32: the parser's
        `torch.isin(labels, valid)` of that crop, or None with logits= (C,h,w) / (1,C,h,w): the parser's logits of that crop (:76-83 run
        here), or None with parse=True: the engine's own face parser makes them of the crop (:73-76); M_c2o 2x3 / 3x3 host, crop -> image; img_ori (Ho,Wo,3) u8; driving_id (1,512).
        Everything on the device, on the caller's stream.  -> {"I_can" (512,512,3) u8, "swap_can" (1,3,512,512), "x_swap", "x_s" (1,21,3)}"""
        e = self.e
        self.drop_prefetches()                                                       # staged key-points were formed with the old kp_swap / pose
        ori = u8_images(img_ori, False, 1, "img_ori", "AnimateChain.set_source").to(e.device).contiguous()
        self._mask_or_logits(mask, logits, "AnimateChain.set_source", parse)
        if parse:
            c1 = torch.as_tensor(crop_u8)
            logits = e.parser(tail.parser_input(e, c1[None] if c1.dim() == 3 else c1))      # :73-76
        if logits is not None:
            lg = torch.as_tensor(logits)
            if lg.dim() not in (3, 4) or (lg.dim() == 4 and lg.shape[0] != 1):
                raise ValueError("logits: expected ONE (C, h, w) set of logits of the crop")
            m = tail.face_masks(e, lg, self.valid)[0]                                # :76-83
        else:
            m = torch.as_tensor(mask)
        if m.dim() != 2:
            raise ValueError("mask: expected ONE (H, W) mask in the crop's frame")
        M = tail._m6(M_c2o)[0].copy()                                                # not the caller's array
        I_s = tail.prepare_crops(e, crop_u8)                                         # cropper.py:155 + :86
        if I_s.shape[0] != 1:
            raise ValueError("crop_u8: expected ONE crop")
        raw_pose = e.motion_extract_raw(I_s)                                         # :87
        x_s, x_d = e.motion_keypoints(raw_pose)                                      # :90, :92-94 (x_d_i_new = scale * kp)
        f_s = e.extract_feature_3d(I_s)                                              # :89
        f_s_can, occ = e.warp(f_s, x_s, x_d)                                         # :97
        f_can_swap = e.swap(f_s_can, driving_id)                                     # :286
        swap_can = e.spade_decode(e.warp_out(f_can_swap, occ))                       # :289 conv_decode
        swap_can_256 = e.resize_half_bilinear(swap_can)                              # :294
        raw_swap = e.motion_extract_raw(swap_can_256)                                # :297
        x_swap, _ = e.motion_keypoints(raw_swap)                                     # :298
        f_swap_can_2 = e.extract_feature_3d(swap_can_256)                            # :308, hoisted out of the loop
        soft = tail.soft_erosion_frames(e, m[None], self.se.weight, self.se.kernel_size, self.se.threshold, self.se.iterations)      # :255
        mask_ori = tail.prepare_paste_back(e, soft[0], M, (ori.shape[1], ori.shape[0]))      # :258
        self._src = {"f_swap_can_2": f_swap_can_2, "x_swap": x_swap, "kp_swap": raw_swap[0, :63].view(21, 3), "raw_pose": raw_pose,
                     "mask_ori": mask_ori, "img_ori": ori, "M_c2o": M}
        self._I_can = e.pack_u8(swap_can)[0]                                         # :290 parse_output
        return {"I_can": self._I_can, "swap_can": swap_can, "x_swap": x_swap, "x_s": x_s}

    def _check_stageable(self):
        if self._src is None:
            raise RuntimeError("AnimateChain: no source has been set (set_source / load_source_state)")

    def source_state(self):
        """What the per-frame path reads: device tensors f_swap_can_2 (1,32,16,64,64), x_swap (1,21,3), kp_swap (21,3), raw_pose (1,328),
        mask_ori (Ho,Wo) fp32, img_ori (Ho,Wo,3) u8, and the host matrix M_c2o (6 doubles).  A caller with several source images keeps one
        dict per image and switches with load_source_state()."""
        self._check_stageable()
        return dict(self._src)

    def load_source_state(self, d):
        e = self.e
        want = {"f_swap_can_2": ((1, 32, 16, 64, 64), torch.float32), "x_swap": ((1, 21, 3), torch.float32), "kp_swap": ((21, 3), torch.float32),
                "raw_pose": ((1, 328), torch.float32)}
        src = {}
        for k, (shape, dt) in want.items():
            t = d[k]
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape:
                raise ValueError(f"load_source_state: {k} must be a {dt} tensor of shape {shape}")
            src[k] = t.to(e.device).contiguous()
        ori, mo = u8_images(d["img_ori"], False, 1, "img_ori", "load_source_state"), d["mask_ori"]
        if not isinstance(mo, torch.Tensor) or mo.dtype != torch.float32 or tuple(mo.shape) != tuple(ori.shape[:2]):
            raise ValueError("load_source_state: mask_ori must be an fp32 tensor of the size of img_ori")
        src["img_ori"], src["mask_ori"] = ori.to(e.device).contiguous(), mo.to(e.device).contiguous()
        src["M_c2o"] = tail._m6(d["M_c2o"])[0].copy()
        self.drop_prefetches()
        self._src = src
        self._I_can = None                                            # the state holds no picture of its source: concat=True needs I_can= from here on

    # ---- stage A: what the generator needs from a batch of driving crops.  The reference runs it as a pre-pass over the whole driving video
    # (prepare_videos + make_motion_template, can_swap_pipeline_v2i.py:235-238) and forms x_t_2 in the loop (:305)
    def _stage_a(self, crops_u8, slot):
        self._check_stageable()
        t = torch.as_tensor(crops_u8)
        B = t.shape[0] if t.dim() == 4 else 1
        I = tail.prepare_crops(self.e, t, out=self._get(("I", slot), (B, 3, 256, 256), torch.float32))      # :223 + :235
        raw = self.e.motion_extract_raw(I, out=self._get(("raw", slot), (B, 328), torch.float32))           # :161
        x_t = self.e.motion_keypoints_driven(raw, self._src["raw_pose"], self._src["kp_swap"],
                                             out=self._get(("x_t", slot), (B, 21, 3), torch.float32))       # :301-305
        return I, x_t

    def prefetch(self, crops_u8):
        """Stage A of the NEXT batch on a side stream beside the generator of the current one; the next __call__ with the same crops tensor
        picks it up.  The rules of FrameChain.prefetch, for the same reasons: a double buffer, at most two batches staged, any
        order; not on a latency-mode engine (split-K scratch shared by M and the generator)."""
        self._stage_ahead(crops_u8)

    def __call__(self, crops_u8, out=None, keep=False, concat=False, I_can=None, concat_out=None):
        """crops_u8 (B,512,512,3) or (B,256,256,3) u8: the cropper's crops of B driving frames
        concat=True: also the frames of the pipeline's side-by-side video (:328, video.py:84-109), "concat" (B,512,1536,3) u8 (into concat_out):
        driving crop | I_can | I_p, the one I_can (512,512,3) u8 shown in every frame: set_source's by default, I_can= otherwise (after
        load_source_state, which carries no picture, it has to be given).
        -> {"frames": (B,Ho,Wo,3) u8[, "concat"][, "crops_out" (B,512,512,3) u8, "x_t" (B,21,3), "I" (B,3,256,256) with keep=True]}"""
        e = self.e
        if concat:
            self._check_stageable()
            ic = self._I_can if I_can is None else torch.as_tensor(I_can)
            if ic is None:
                raise RuntimeError("AnimateChain: concat=True after load_source_state needs I_can= (the state holds no picture of its source)")
            ic = ic[None] if ic.dim() == 3 else ic
            if ic.dtype != torch.uint8 or tuple(ic.shape) != (1, 512, 512, 3):
                raise ValueError("I_can: expected ONE (512, 512, 3) uint8 image")
        slot, (I, x_t) = self._resolve(crops_u8)
        src = self._src
        B = I.shape[0]
        gen = e.animate_frames(src["f_swap_can_2"], src["x_swap"], x_t, want_f32=False, want_u8=True,
                               out_u8=self._get("gen", (B, 512, 512, 3), torch.uint8))["out_u8"]        # :309-312
        frames = tail.paste_back_shared(e, gen, src["M_c2o"], src["img_ori"], src["mask_ori"], out=out)  # :317-321
        self._release(slot)
        res = {"frames": frames}
        if concat:
            res["concat"] = self._concat(crops_u8, [(ic, 0, 1)], gen, concat_out)                       # :328
        if keep:
            res.update(crops_out=gen, x_t=x_t, I=I)
        return res
