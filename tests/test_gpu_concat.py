"""The side-by-side video frame on the device (cs_concat_frames; tail.concat_frames; can_swapper.concat_frames; both chains' concat=True):
concat_frames of src/utils/video.py:84-109 as the pipelines call it (src/can_swap_pipeline_e2e.py:290, src/can_swap_pipeline_v2i.py:328) in one
kernel.  The yardstick is tests/concat_ref.py (test_concat_cpu.py holds it to the hand check and the float formula; PARITY UNPINNED: no cv2
output is at hand); the tolerance is bit equality: the arithmetic is integer, or parse_output's clip / scale / truncate in fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_helpers
import concat_ref as CR
from chain_helpers import _affine, _masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sds_m():
    return chain_helpers.motion_state_dicts()


@pytest.fixture(scope="module")
def swapper_m(sds_m):
    return chain_helpers.swapper_b4(sds_m)


@pytest.fixture(scope="module")
def eng(swapper_m):
    return swapper_m.engine


def _t(a):
    """numpy -> torch through a copy: the yardstick's arrays are shared between the tests and read-only."""
    return torch.from_numpy(np.array(a))


def _run_case(eng, B, S, kinds, shared):
    from canonswap_amd import tail
    panels, want = CR.case(B, S, kinds, shared)
    got = tail.concat_frames(eng, [_t(p).cuda() for p in panels], kinds=kinds, shared=shared)
    assert got.device == eng.device and got.dtype == torch.uint8 and tuple(got.shape) == (B, S, len(kinds) * S, 3)
    diff = int((got.cpu() != _t(want)).sum())
    assert diff == 0, (B, S, kinds, shared, f"{diff} bytes differ")


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("S", [4, 8, 12])
def test_every_kind_in_every_position_equals_the_restatement(eng, S):
    """B = 3, P = 1 .. 4, every kind in every panel position, mixed shared flags.  S = 4: a 2-pixel source row, both border taps in one thread;
    S = 8, 12: two and three threads per panel row (first, interior, last), 12 with a ragged last block and source rows off the dword grid."""
    for P in (1, 2, 3, 4):
        for kinds, shared in CR.arrangements(P):
            _run_case(eng, 3, S, kinds, shared)


@pytest.mark.parametrize("kinds,shared", [((2, 3, 3, 0), (0, 0, 0, 0)), ((1, 0, 0), (0, 1, 0))], ids=["e2e", "v2i"])
def test_full_size_arrangements(eng, kinds, shared):
    """S = 512, B = 2 as the chains call it: driving | rec_can | I_can | I_p, and driving (256 x 256 crops) | the one I_can | I_p."""
    _run_case(eng, 2, 512, kinds, shared)


def test_input_forms_defaults_and_output_buffers(eng, swapper_m):
    from canonswap_amd import tail
    kinds, shared = (1, 3, 0), (0, 1, 0)
    panels, want = CR.case(3, 8, kinds, shared)
    dev = [_t(p).cuda() for p in panels]
    assert torch.equal(tail.concat_frames(eng, dev).cpu(), _t(want))                      # kinds and shared inferred: 4 x 4 u8, fp32, 8 x 8 u8; n = 1 beside 3
    assert torch.equal(tail.concat_frames(eng, [np.array(p) for p in panels]).cpu(), _t(want))      # host arrays are uploaded
    assert torch.equal(swapper_m.concat_frames(dev, kinds=kinds).cpu(), _t(want))
    one = tail.concat_frames(eng, [dev[0][1], dev[1][0], dev[2][1]])                      # (H,W,3) / (3,H,W): one frame
    assert tuple(one.shape) == (1, 8, 24, 3) and torch.equal(one.cpu()[0], _t(want)[1])
    out = torch.empty((3, 8, 24, 3), dtype=torch.uint8, device=eng.device)
    assert tail.concat_frames(eng, dev, out=out) is out and torch.equal(out.cpu(), _t(want))
    for bad in (torch.empty((3, 8, 24, 3), dtype=torch.uint8), torch.empty((3, 8, 24, 3), dtype=torch.float32, device=eng.device),
                torch.empty((2, 8, 24, 3), dtype=torch.uint8, device=eng.device), torch.empty((3, 8, 48, 3), dtype=torch.uint8, device=eng.device)[:, :, ::2]):
        with pytest.raises(ValueError):
            tail.concat_frames(eng, dev, out=bad)
    # buffers off the dword / 16-byte grid take the element accesses: the same bytes, nothing before or beyond
    n, pad = want.size, 64
    ob = torch.full((pad + n + pad,), 0xAB, dtype=torch.uint8, device=eng.device)
    o1 = ob[pad + 1:pad + 1 + n].view(want.shape)
    fb = torch.zeros((panels[1].size + 1,), dtype=torch.float32, device=eng.device)
    fb[1:] = dev[1].reshape(-1)
    ub = torch.zeros((panels[0].size + 3,), dtype=torch.uint8, device=eng.device)
    ub[3:] = dev[0].reshape(-1)
    f1, u1 = fb[1:].view(panels[1].shape), ub[3:].view(panels[0].shape)
    assert o1.data_ptr() % 4 == 1 and f1.data_ptr() % 16 == 4 and u1.data_ptr() % 4 == 3
    assert tail.concat_frames(eng, [u1, f1, dev[2]], kinds=kinds, shared=shared, out=o1) is o1
    assert torch.equal(o1.cpu(), _t(want))
    assert bool((ob[:pad + 1] == 0xAB).all()) and bool((ob[pad + 1 + n:] == 0xAB).all())


def test_c_side_refusals_name_the_entry_point_and_launch_nothing(eng):
    from canonswap_amd.engine import _ptr
    panels, _ = CR.case(3, 8, (1, 3, 0), (0, 1, 0))
    dev = [_t(p).cuda() for p in panels]
    out = torch.full((3, 8, 24, 3), 7, dtype=torch.uint8, device=eng.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = eng.lib
    vp3, i3 = C.c_void_p * 3, C.c_int * 3
    base = dict(e=eng.h, B=3, P=3, S=8, panels=vp3(*[t.data_ptr() for t in dev]), kinds=i3(1, 3, 0), shared=i3(0, 1, 0), out=_ptr(out))

    def call(**kw):
        a = dict(base, **kw)
        rc = lib.cs_concat_frames(a["e"], a["B"], a["P"], a["S"], a["panels"], a["kinds"], a["shared"], a["out"], st)
        return rc, lib.cs_last_error().decode()

    five = (C.c_void_p * 5)(*[dev[2].data_ptr()] * 5), (C.c_int * 5)(0, 0, 0, 0, 0)
    refused = [({"e": None}, "NULL engine"), ({"out": None}, "NULL out"), ({"panels": None}, "NULL panels"), ({"kinds": None}, "NULL kinds"),
               ({"shared": None}, "NULL shared"), ({"panels": vp3(dev[0].data_ptr(), None, dev[2].data_ptr())}, "NULL panel 1"),
               ({"B": 0}, "B = 0"), ({"B": -2}, "B = -2"), ({"P": 0}, "P = 0"), ({"P": 5, "panels": five[0], "kinds": five[1], "shared": five[1]}, "P = 5"),
               ({"kinds": i3(1, 4, 0)}, "kind 4 of panel 1"), ({"kinds": i3(-1, 3, 0)}, "kind -1 of panel 0"),
               ({"S": 6}, "S = 6"), ({"S": 0}, "S = 0"), ({"S": 2}, "S = 2"), ({"S": -8}, "S = -8"), ({"S": 16388}, "S = 16388"), ({"S": 2 ** 30}, "16384")]
    for kw, word in refused:
        rc, err = call(**kw)
        assert rc != 0 and "cs_concat_frames" in err and word in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                 # a refused call launches nothing
    rc, _ = call()
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _t(CR.case(3, 8, (1, 3, 0), (0, 1, 0))[1]))


# ------------------------------------------------------------------------------------------------ the chains
def _crops(n, seed):
    from canonswap_amd import synth
    smooth = synth.make_smooth_images(n, seed=seed, size=512)
    return np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))


def _chain_batch(B, seed, Ho=360, Wo=640):
    r = np.random.Generator(np.random.PCG64(seed))
    crops = _t(_crops(B, 2700 + seed)).cuda()
    masks = _t(_masks(B, seed=seed)).cuda()
    ori = _t(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
    Ms = np.stack([_affine(j % 4, Ho, Wo) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(B)])
    return crops, masks, Ms, ori


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("size", [512, 256])
def test_frame_chain_concat(swapper_m, size):
    """B = 2, concat=True, keep=True: the frames are those of the call without concat, rec_can / swap_can are the engine's debug decodes on the
    kept I, x_t, x_can, and "concat" is the restatement of driving | rec_can | I_can | I_p on the crops and the kept tensors; a caller's
    concat_out is written; the call without concat carries none of it."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    idv = _t(synth.make_identity(7)).cuda()
    crops, masks, Ms, ori = _chain_batch(2, 121)
    if size == 256:
        crops = crops[:, ::2, ::2].contiguous()
    chain = FrameChain(swapper_m)
    plain = chain(crops, masks, Ms, ori, idv, keep=True)
    assert "concat" not in plain and "rec_can" not in plain and "rec_can" not in chain._buf      # no extra decode, no buffer for one
    frames0 = plain["frames"].clone()
    res = chain(crops, masks, Ms, ori, idv, concat=True, keep=True)
    assert torch.equal(res["frames"], frames0)
    cat = res["concat"]
    assert cat.dtype == torch.uint8 and tuple(cat.shape) == (2, 512, 2048, 3) and cat.device == swapper_m.engine.device
    dbg = swapper_m.engine.swap_frames(res["I"], res["x_t"], res["x_can"], idv, want_f32=False, want_u8=True, debug=True)
    assert torch.equal(dbg["rec_can"], res["rec_can"]) and torch.equal(dbg["swap_can"], res["swap_can"]) and torch.equal(dbg["out_u8"], res["crops_out"])
    want = CR.concat([_np(crops), _np(res["rec_can"]), _np(res["swap_can"]), _np(res["crops_out"])], [2 if size == 512 else 1, 3, 3, 0])
    assert np.array_equal(_np(cat), want)
    assert np.array_equal(_np(cat)[:, :, 1536:], _np(res["crops_out"]))            # the last panel is I_p
    out = torch.empty((2, 512, 2048, 3), dtype=torch.uint8, device=cat.device)
    again = chain(crops, masks, Ms, ori, idv, concat=True, concat_out=out)
    assert again["concat"] is out and torch.equal(out, cat) and "rec_can" not in again


def test_frame_chain_concat_of_a_prefetched_batch(swapper_m):
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    idv = _t(synth.make_identity(7)).cuda()
    cur, nxt = _chain_batch(2, 131), _chain_batch(2, 132)
    chain = FrameChain(swapper_m)
    want = [{k: v.clone() for k, v in chain(b[0], b[1], b[2], b[3], idv, concat=True).items()} for b in (cur, nxt)]
    chain.prefetch(cur[0], cur[1])
    chain.prefetch(nxt[0], nxt[1])
    got = [{k: v.clone() for k, v in chain(b[0], b[1], b[2], b[3], idv, concat=True).items()} for b in (cur, nxt)]
    torch.cuda.synchronize()
    assert not chain._pending and not torch.equal(want[0]["concat"], want[1]["concat"])
    for w, g in zip(want, got):
        assert torch.equal(g["frames"], w["frames"]) and torch.equal(g["concat"], w["concat"])


def _source(chain, seed=3100, Ho=540, Wo=960):
    from canonswap_amd import synth
    r = np.random.Generator(np.random.PCG64(seed))
    M = _affine(1, Ho, Wo) * np.array([[0.5], [0.5], [1]]) + np.array([[0, 0, 100.], [0, 0, 20.], [0, 0, 0]])
    return chain.set_source(_t(_crops(1, seed)[0]).cuda(), _t(_masks(1, seed=33)[0]).cuda(), M,
                            _t(r.integers(0, 256, size=(Ho, Wo, 3), dtype=np.uint8)).cuda(), _t(synth.make_identity(7)).cuda())


def test_animate_chain_concat(swapper_m):
    """driving | the one I_can | I_p: the restatement on the driving crops, set_source's I_can and crops_out; the frames do not change; after
    load_source_state the chain has no picture of the source and asks for one."""
    from canonswap_amd.chain import AnimateChain
    chain = AnimateChain(swapper_m)
    with pytest.raises(RuntimeError, match="no source"):
        chain(_t(_crops(2, 3200)).cuda(), concat=True)
    info = _source(chain)
    drv = _t(_crops(2, 3200)).cuda()
    frames0 = chain(drv)["frames"].clone()
    res = chain(drv, concat=True, keep=True)
    assert torch.equal(res["frames"], frames0)
    cat = res["concat"]
    assert cat.dtype == torch.uint8 and tuple(cat.shape) == (2, 512, 1536, 3)
    want = CR.concat([_np(drv), _np(info["I_can"])[None], _np(res["crops_out"])], [2, 0, 0], [0, 1, 0])
    assert np.array_equal(_np(cat), want)
    small = drv[:, ::2, ::2].contiguous()                                          # 256 x 256 driving crops: resized x 2
    res = chain(small, concat=True, keep=True)
    assert np.array_equal(_np(res["concat"]), CR.concat([_np(small), _np(info["I_can"])[None], _np(res["crops_out"])], [1, 0, 0], [0, 1, 0]))
    st = chain.source_state()
    assert set(st) == {"f_swap_can_2", "x_swap", "kp_swap", "raw_pose", "mask_ori", "img_ori", "M_c2o"}
    # another source's state, loaded: no picture comes with it
    other = AnimateChain(swapper_m)
    other_info = _source(other, seed=3150)
    assert not torch.equal(other_info["I_can"], info["I_can"])
    chain.load_source_state(other.source_state())
    with pytest.raises(RuntimeError, match="I_can"):
        chain(drv, concat=True)
    assert not chain._pending
    with pytest.raises(ValueError, match="I_can"):
        chain(drv, concat=True, I_can=other_info["I_can"][:256])
    out = torch.empty((2, 512, 1536, 3), dtype=torch.uint8, device=cat.device)
    res = chain(drv, concat=True, I_can=other_info["I_can"], concat_out=out, keep=True)
    assert res["concat"] is out
    assert torch.equal(res["frames"], other(drv)["frames"])
    assert np.array_equal(_np(out), CR.concat([_np(drv), _np(other_info["I_can"])[None], _np(res["crops_out"])], [2, 0, 0], [0, 1, 0]))
    assert set(chain.source_state()) == set(st)
    _source(chain)                                                                 # set_source remembers its own again
    assert torch.equal(chain(drv, concat=True)["concat"], cat)
