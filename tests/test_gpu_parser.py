"""The SegFormer face parser on the engine (cs_parser; csrc/parser.hip): the whole network and its stages against the float64 restatement of
tests/parser_ref.py, batching, determinism, refusals, and the wiring into can_swapper and the two chains.

Tolerance of every comparison with the network in it: at most 4 x the distance of the restatement's fp16-operand emulation from float64 on the
same input (measured here on the CPU; a property of the restatement, never of the engine) - relative L2 per image for the logits and the
stage outputs, and max-abs over max |logit| for the logits.  The emulation rounds only the operands of the matmuls; the engine also stores
activations in fp16 and sums in another order.  tests/test_parser_cpu.py shows that real mistakes are more than 10 x above this bound."""
import numpy as np
import pytest
import torch

import chain_helpers
import parser_ref as R
from chain_helpers import _affine
from hip_ops import op

pytestmark = pytest.mark.gpu
FACTOR = 4.0
HEADS = {"num_attention_heads": [1, 2, 5, 8]}
H0, W0 = 64, 96


@pytest.fixture(scope="module")
def cfg():
    from canonswap_amd import synth
    return dict(synth.PARSER_A)


@pytest.fixture(scope="module")
def sd_np(cfg):
    from canonswap_amd import synth
    return synth._segformer(0, cfg)


@pytest.fixture(scope="module")
def swapper(sd_np):
    """The generator, the motion extractor and the parser in one engine of 9 images (one more than the parser's workspace chunk of 8)."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    sds = chain_helpers.motion_state_dicts()
    return can_swapper(None, state_dicts=sds, max_batch=9, parser=(synth.to_torch({"p": sd_np})["p"], HEADS))


@pytest.fixture(scope="module")
def pv():
    """Three 64 x 96 inputs: two smooth images and one that is constant except for one bright pixel in each corner (padding of the stem and of
    the depth-wise convs, clamped taps of the head)."""
    from canonswap_amd import synth
    u8 = synth.make_parser_images(3, seed=4100, H=H0, W=W0)
    u8[2] = 128
    for (h, w), v in zip(((0, 0), (0, W0 - 1), (H0 - 1, 0), (H0 - 1, W0 - 1)), (255, 0, 200, 30)):
        u8[2, :, h, w] = v
    return torch.from_numpy(synth.parser_pixel_values(u8))


def _refs(sd_np, cfg, x):
    sd = R.to_tensors(sd_np)
    with torch.no_grad():
        f64 = R.forward(sd, cfg, x.double())
        emu = R.forward(sd, cfg, x.double(), emulate=True)
    keys = R.STAGES + ("pre", "logits")
    err = {k: R.rel_l2(emu[k], f64[k]) for k in keys}
    err["maxabs"] = R.max_abs(emu["logits"], f64["logits"])
    print("emulation vs float64:", {k: [f"{v:.2e}" for v in e.tolist()] for k, e in err.items()})
    return {"f64": f64, "err": err}


@pytest.fixture(scope="module")
def ref(sd_np, cfg, pv):
    return _refs(sd_np, cfg, pv)


def _check(got, ref, rows, what=""):
    want = ref["f64"]["logits"][rows]
    e2, ema = R.rel_l2(got, want), R.max_abs(got, want)
    b2, bma = FACTOR * ref["err"]["logits"][rows], FACTOR * ref["err"]["maxabs"][rows]
    print(what, "logits, engine vs float64: rel L2", [f"{v:.2e}" for v in e2.tolist()], "bound", [f"{v:.2e}" for v in b2.tolist()],
          "max-abs", [f"{v:.2e}" for v in ema.tolist()], "bound", [f"{v:.2e}" for v in bma.tolist()])
    assert got.shape == want.shape
    assert bool((e2 <= b2).all()) and bool((ema <= bma).all())
    # labels: wherever the float64 margin exceeds twice the max-abs bound, the engine's argmax is the float64 one; at most 10 % of pixels are unsure
    bound = bma * want.reshape(len(rows), -1).abs().amax(1)
    sure = R.margins(want) > 2 * bound[:, None, None]
    assert bool((1 - sure.double().mean(dim=(1, 2)) <= 0.10).all())
    assert bool((got.cpu().argmax(1) == want.argmax(1))[sure].all())


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("rows", [(0,), (0, 1, 2)], ids=["b1", "b3"])
def test_whole_network_against_float64(swapper, pv, ref, rows):
    rows = list(rows)
    e = swapper.engine
    logits = e.parser(pv[rows].cuda())
    _check(logits, ref, rows)
    for which, k in enumerate(R.STAGES + ("pre",)):
        got = e.parser_read(which, len(rows), H0, W0)
        want = ref["f64"][k][rows]
        assert got.shape == want.shape, k
        err, tol = R.rel_l2(got, want), FACTOR * ref["err"][k][rows]
        print(k, "engine vs float64:", [f"{v:.2e}" for v in err.tolist()], "bound:", [f"{v:.2e}" for v in tol.tolist()])
        assert bool((err <= tol).all()), k
    with pytest.raises(RuntimeError, match=f"last pass held {len(rows)}"):
        e.parser_read(0, len(rows) + 1, H0, W0)


def test_rows_do_not_depend_on_their_batch_and_calls_repeat(swapper, pv):
    e = swapper.engine
    x = pv.cuda()
    three = e.parser(x).clone()
    assert torch.equal(e.parser(x), three)
    for k in range(3):
        assert torch.equal(e.parser(x[k:k + 1])[0], three[k]), k
    assert swapper.parse(x).shape == (3, 19, H0 // 4, W0 // 4)


def test_more_images_than_the_workspace_chunk(swapper, pv):
    """Nine images run as a pass of eight and a pass of one: every row has the bits of its own single-image call."""
    e = swapper.engine
    x = torch.cat([pv, pv.flip(3), pv.flip(2)]).cuda()
    nine = e.parser(x)
    for k in (0, 4, 7, 8):
        assert torch.equal(e.parser(x[k:k + 1])[0], nine[k]), k
    with pytest.raises(RuntimeError, match="last pass held 1"):
        e.parser_read(0, 2, H0, W0)


def test_product_extent(swapper, sd_np, cfg):
    """512 x 512, two images: 256 keys in every stage (the attention kernel's full LDS tile), 16384 tokens in stage 0."""
    from canonswap_amd import synth
    x = torch.from_numpy(synth.make_parser_inputs(2, seed=4200, H=512, W=512))
    ref = _refs(sd_np, cfg, x)
    _check(swapper.engine.parser(x.cuda()), ref, [0, 1], "512 x 512")


# ------------------------------------------------------------------------------------------------ refusals, each before any launch
def test_refusals(swapper, state_dicts):
    from canonswap_amd.engine import Engine
    e = swapper.engine
    x = torch.zeros(1, 3, 96, 96, device="cuda")
    out = torch.full((1, 19, 24, 24), 7.0, device="cuda")

    def refused(word, *args):
        with pytest.raises(RuntimeError, match=word):
            op(*args)
    refused("multiple of 32", "cs_parser", e.h, 1, x, 72, 96, out)
    refused("batch 0", "cs_parser", e.h, 0, x, 96, 96, out)
    refused("batch 10", "cs_parser", e.h, 10, x, 96, 96, out)
    refused("NULL", "cs_parser", e.h, 1, None, 96, 96, out)
    refused("NULL", "cs_parser", e.h, 1, x, 96, 96, None)
    refused("exceeds", "cs_parser", e.h, 1, x, 544, 512, out)
    refused("cs_parser failed", "cs_parser", None, 1, x, 96, 96, out)
    with pytest.raises(ValueError, match="multiple of 32"):
        e.parser(torch.zeros(1, 3, 72, 96))
    bare = Engine(0, max_batch=1)
    refused("cs_finalize_weights has not been called", "cs_parser", bare.h, 1, x, 96, 96, out)
    with pytest.raises(RuntimeError, match="no face parser"):
        bare.parser(x)
    bare.load_state_dicts(state_dicts)
    assert not bare.has_parser
    refused("holds no face parser", "cs_parser", bare.h, 1, x, 96, 96, out)
    refused("cs_op_parser_read failed", "cs_op_parser_read", bare.h, 0, 1, out)
    bare.close()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ wiring
def _frames(B, seed=4300, Ho=360, Wo=640):
    from canonswap_amd import synth
    smooth = synth.make_smooth_images(B, seed=seed, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda()
    r = np.random.Generator(np.random.PCG64(seed))
    ori = torch.from_numpy(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
    Ms = np.stack([_affine(k, Ho, Wo) * np.array([[0.5], [0.5], [1]]) for k in range(B)])
    return crops, Ms, ori


def test_face_masks_from_crops(swapper):
    from canonswap_amd import tail
    crops, _, _ = _frames(2)
    e = swapper.engine
    want = tail.face_masks(e, e.parser(tail.parser_input(e, crops)))
    got = swapper.face_masks_from_crops(crops)
    assert got.shape == (2, 512, 512) and got.dtype == torch.uint8 and torch.equal(got, want)
    assert 0 < int(got.sum()) < got.numel()


def test_frame_chain_parse_equals_logits_path(swapper):
    """parse=True frames are the frames of logits=engine.parser(chain.parser_input(crops)): in-line, prefetched, and staged out of order."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    e = swapper.engine
    sid = torch.from_numpy(synth.make_identity(7)).cuda()
    chain = FrameChain(swapper)
    a, Ma, oa = _frames(2, seed=4300)
    b, Mb, ob = _frames(2, seed=4400)
    want_a = chain(a, None, Ma, oa, sid, logits=e.parser(chain.parser_input(a)))["frames"].clone()
    want_b = chain(b, None, Mb, ob, sid, logits=e.parser(chain.parser_input(b)))["frames"].clone()
    assert not torch.equal(want_a, oa)
    assert torch.equal(chain(a, None, Ma, oa, sid, parse=True)["frames"], want_a)
    chain.prefetch(a, parse=True)
    assert torch.equal(chain(a, None, Ma, oa, sid, parse=True)["frames"], want_a)
    chain.prefetch(a, parse=True)
    chain.prefetch(b, parse=True)
    assert torch.equal(chain(b, None, Mb, ob, sid, parse=True)["frames"], want_b)
    assert torch.equal(chain(a, None, Ma, oa, sid, parse=True)["frames"], want_a)


def test_parse_arguments(swapper, state_dicts):
    from canonswap_amd.chain import FrameChain
    chain = FrameChain(swapper)
    a, Ma, oa = _frames(1)
    with pytest.raises(ValueError, match="pass neither"):
        chain(a, None, Ma, oa, logits=torch.zeros(1, 19, 128, 128, device="cuda"), parse=True)
    with pytest.raises(ValueError, match="pass neither"):
        chain.prefetch(a, masks=torch.zeros(1, 512, 512, dtype=torch.uint8, device="cuda"), parse=True)
    with pytest.raises(ValueError, match=r"got neither"):
        chain(a, None, Ma, oa)
    # an engine without the network: a RuntimeError before anything is enqueued
    import types
    lame = types.SimpleNamespace(has_parser=False)
    real, chain.e = chain.e, lame
    try:
        with pytest.raises(RuntimeError, match="holds no face parser"):
            chain(a, None, Ma, oa, parse=True)
        with pytest.raises(RuntimeError, match="holds no face parser"):
            chain.prefetch(a, parse=True)
    finally:
        chain.e = real
    assert not chain._pending


def test_animate_chain_set_source_parse(swapper):
    from canonswap_amd import synth
    from canonswap_amd.chain import AnimateChain
    e = swapper.engine
    did = torch.from_numpy(synth.make_identity(9)).cuda()
    crops, Ms, ori = _frames(2, seed=4500)
    one = AnimateChain(swapper)
    one.set_source(crops[0], None, Ms[0], ori[0], did, logits=e.parser(one.parser_input(crops[:1])))
    want_mask = one.source_state()["mask_ori"].clone()
    want = one(crops)["frames"].clone()
    two = AnimateChain(swapper)
    two.set_source(crops[0], None, Ms[0], ori[0], did, parse=True)
    assert torch.equal(two.source_state()["mask_ori"], want_mask) and 0 < float(want_mask.sum())
    assert torch.equal(two(crops)["frames"], want)
    with pytest.raises(ValueError, match="pass neither"):
        two.set_source(crops[0], torch.zeros(512, 512, dtype=torch.uint8), Ms[0], ori[0], did, parse=True)


def test_parser_call_between_prefetch_and_call_leaves_the_generator_alone(swapper, pv):
    """The parser's workspace is its own: a parser call enqueued on the caller's stream while a batch is staged on the side stream changes
    nothing in the frames, and is not changed by them."""
    from canonswap_amd import synth
    from canonswap_amd.chain import FrameChain
    e = swapper.engine
    sid = torch.from_numpy(synth.make_identity(7)).cuda()
    chain = FrameChain(swapper)
    a, Ma, oa = _frames(2, seed=4600)
    lg = e.parser(chain.parser_input(a)).clone()
    want = chain(a, None, Ma, oa, sid, logits=lg)["frames"].clone()
    other = e.parser(pv.cuda()).clone()
    chain.prefetch(a, logits=lg)
    again = e.parser(pv.cuda())
    got = chain(a, None, Ma, oa, sid, logits=lg)["frames"]
    assert torch.equal(got, want) and torch.equal(again, other)
