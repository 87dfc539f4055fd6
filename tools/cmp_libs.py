"""GPU box: the same frames through two builds of the library, compared bit for bit (stage outputs of the whole loop body, default and latency mode,
cs_spade_decode's image and launch list, W's own entry points - warp, warp_forward, animate_frames on one shared volume -, the motion extractor's raw head outputs, and the crop / warp /
paste-back entry points on 1080p frames); the environment (an A/B knob such as CANONSWAP_WARP_FUSED=0) reaches both children:
    python tools/cmp_libs.py tools/bin/base.so ""        ("" = the shipped library)
Each build runs in its own process (the library is chosen at import: CANONSWAP_LIB)."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, tempfile, torch
sys.path.insert(0, %r)
from canonswap_amd import synth
from canonswap_amd.can_swap_e2e import can_swapper
B = 6
sds = synth.to_torch(synth.make_state_dicts(0))
out = {}
for lat in (False, True):
    sw = can_swapper(None, state_dicts=sds, max_batch=B, latency_mode=lat)
    inp = synth.make_frame_inputs(B, seed=1000, size=256)
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    args = [torch.from_numpy(inp[k]).cuda() for k in ("img", "x_t", "x_can")]
    nb = 1 if lat else B
    r = sw.swap_frames(*(a[:nb] for a in args), idv, debug=True)
    for k, v in r.items():
        if torch.is_tensor(v):
            out[("lat." if lat else "") + k] = v.cpu()
    # cs_spade_decode on its own (default and latency mode): the image and the launch list of the profile CSV (its labels, as bytes)
    e = sw.engine
    seg = e.warp_out(e.extract_feature_3d(args[0][:nb]))
    out[("lat." if lat else "") + "engine.spade_decode"] = e.spade_decode(seg).cpu()
    with tempfile.TemporaryDirectory() as td:
        os.environ["CANONSWAP_PROFILE_CSV"] = os.path.join(td, "l.csv")
        e.profile_begin(); e.spade_decode(seg); e.profile_end()
        labels = " ".join(l.split(",")[1] for l in open(os.environ.pop("CANONSWAP_PROFILE_CSV")).read().splitlines()[1:])
    out[("lat." if lat else "") + "engine.spade_decode.launches"] = torch.tensor(list(labels.encode()), dtype=torch.uint8)
    if not lat:
        # W's entry points beyond the loop body, on the same engine: cs_warp (f_out and occ), cs_warp_forward (the fused kernel also stores its
        # deformation), cs_animate_frames with ONE volume and ONE source key-point set for 3 frames (sample stride 0 in dm_sparse and in the
        # softmax / warp kernels)
        e, (img, kd, ks) = sw.engine, (a[:3] for a in args)
        f = e.extract_feature_3d(img)
        out["engine.warp.f_out"], out["engine.warp.occ"] = (t.cpu() for t in e.warp(f, ks, kd))
        for k, v in e.warp_forward(f, kd, ks).items():
            out["engine.warp_forward." + k] = v.cpu()
        out["engine.animate_frames.shared"] = e.animate_frames(f[:1], ks[:1], kd)["out"].cpu()
sdm = synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))
swm = can_swapper(None, state_dicts=sdm, max_batch=5)
out["M.raw"] = swm.engine.motion_extract_raw(torch.from_numpy(synth.make_smooth_images(5, seed=77, size=256)).cuda()).cpu()
# the image-space tail (csrc/imgops.hip) at the sizes tools/time_crop.py and tools/time_v2i_chain.py time: 1080 x 1920 frames, 512 x 512 crops
import numpy as np
from canonswap_amd import tail
e = swm.engine
r = np.random.Generator(np.random.PCG64(4242))
Bt, Ho, Wo = 4, 1080, 1920
frames = torch.from_numpy(r.integers(0, 256, size=(Bt, Ho, Wo, 3), dtype=np.uint8)).cuda()
crops = torch.from_numpy(r.integers(0, 256, size=(Bt, 512, 512, 3), dtype=np.uint8)).cuda()
masks = torch.from_numpy(r.random(size=(Bt, 512, 512), dtype=np.float32)).cuda()
# crop -> frame: inside the frame, rotated and enlarged, hanging over the left and over the right edge
M_c2o = np.stack([[[sc * np.cos(th), -sc * np.sin(th), tx], [sc * np.sin(th), sc * np.cos(th), ty], [0, 0, 1]] for sc, th, tx, ty in
                  ((0.45 * Ho / 512, 0.1, 0.35 * Wo, 0.2 * Ho), (1.3, -0.3, 900.0, 300.0), (0.6, 0.25, -150.5, 700.3), (1.0, 0.0, 1500.25, 600.75))])
c = tail.crop_frames_M(e, frames, np.linalg.inv(M_c2o), 512, want_I=True)
out["tail.crop_frames_M"], out["tail.crop_frames_M.I"] = c["crops"].cpu(), c["I"].cpu()
out["tail.paste_back_batch"] = tail.paste_back_batch(e, crops, masks, M_c2o, frames).cpu()
mask_ori = tail.prepare_paste_back(e, masks[0], M_c2o[0], (Wo, Ho))
out["tail.prepare_paste_back"] = mask_ori.cpu()
out["tail.paste_back_shared"] = tail.paste_back_shared(e, crops, M_c2o[0], frames[0], mask_ori).cpu()
out["tail.paste_back"] = tail.paste_back(e, crops[0], M_c2o[0], frames[0], mask_ori).cpu()
out["tail.paste_back_fused"] = tail.paste_back_fused(e, crops[0], masks[0], M_c2o[0], frames[0]).cpu()
out["tail.warp_affine_u8"] = tail.warp_affine_u8(e, crops[0], M_c2o[0], (Wo, Ho)).cpu()
torch.save(out, sys.argv[1])
''' % ROOT


def run(lib, path):
    env = dict(os.environ)
    if lib:
        env["CANONSWAP_LIB"] = lib
    else:
        env.pop("CANONSWAP_LIB", None)
    subprocess.run([sys.executable, "-c", CHILD, path], check=True, env=env, cwd=ROOT)


def main():
    import torch
    a, b = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        pa, pb = os.path.join(d, "a.pt"), os.path.join(d, "b.pt")
        run(a, pa); run(b, pb)
        A, Bv = torch.load(pa), torch.load(pb)
    bad = 0
    for k in A:
        same = torch.equal(A[k], Bv[k])
        bad += not same
        print("%-24s %s %s" % (k, tuple(A[k].shape), "same bits" if same else "DIFFERS: max abs %g" % float((A[k].float() - Bv[k].float()).abs().max())))
    print("libs [%s] vs [%s]: %s" % (a, b, "identical outputs" if not bad else "%d outputs differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
