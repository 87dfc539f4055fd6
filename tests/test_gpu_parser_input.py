"""The parser's input on the device (cs_parser_input; tail.parser_input; can_swapper.parser_input; the chains' parser_input): what the
reference runs on the host on a crop before SegFormer sees it (src/can_swap_pipeline_e2e.py:171 + :180, src/can_swap_pipeline_v2i.py:73) in one
kernel.  The yardstick is tests/parser_input_ref.py, the integer restatement that test_parser_input_cpu.py holds equal to PIL; the tolerance
is bit equality: the arithmetic is integer and the floats are table entries."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_helpers
import parser_input_ref as PR
from chain_helpers import _affine

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


def _same_bits(got, want):
    """fp32 tensors equal bit for bit (torch.equal on the int32 view: -0.0 and 0.0 would differ, NaN would compare)."""
    return torch.equal(got.cpu().contiguous().view(torch.int32), _t(want).view(torch.int32))


def _check(got, ref, what):
    B, Ho, Wo, _ = ref["resized_u8"].shape
    pv, u8 = got["pixel_values"], got["resized_u8"]
    assert pv.dtype == torch.float32 and tuple(pv.shape) == (B, 3, Ho, Wo) and u8.dtype == torch.uint8 and tuple(u8.shape) == (B, Ho, Wo, 3), what
    assert torch.equal(u8.cpu(), _t(ref["resized_u8"])), what
    assert torch.equal(pv.cpu(), _t(ref["pixel_values"])) and _same_bits(pv, ref["pixel_values"]), what


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("halve", [0, 1])
@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("name", list(PR.CASES))
def test_both_outputs_equal_the_restatement(eng, name, kind, halve):
    from canonswap_amd import tail
    ref = PR.reference(name, kind, halve)
    crops = _t(ref["crops"]).cuda()
    got = tail.parser_input(eng, crops, halve=halve, want_u8=True)
    assert got["pixel_values"].device == eng.device and got["resized_u8"].device == eng.device
    _check(got, ref, (name, kind, halve))


@pytest.mark.parametrize("name,kind", PR.fixture_items())
def test_pils_own_outputs(eng, name, kind):
    """The fixture's inputs through the kernel against what PIL made of them (tools/make_golden_parser_input.py) and the fixture's table."""
    from canonswap_amd import tail
    fx = PR.fixture()
    x, pil = fx[f"{name}/{kind}/in"], fx[f"{name}/{kind}/pil"]
    got = tail.parser_input(eng, _t(x).cuda(), halve=0, want_u8=True)
    _check(got, {"resized_u8": pil, "pixel_values": PR.pixel_values(pil, fx["lut"])}, (name, kind))


@pytest.mark.parametrize("name,halve", [("r5x7", 0), ("r33x65", 1), ("r16x4", 0), ("full", 1)])
def test_either_output_alone_gives_the_same_bits(eng, name, halve):
    """Straight through the C entry point: pixel_values alone, resized_u8 alone; sentinel-filled buffers longer than needed stay untouched
    outside the output."""
    from canonswap_amd import tail
    ref = PR.reference(name, "random", halve)
    crops = _t(ref["crops"]).cuda()
    B, Hc, Wc, _ = crops.shape
    n, pad = ref["resized_u8"].size, 1024
    lut = _t(tail.parser_lut()).cuda()
    pv = torch.full((pad + n + pad,), -7.0, dtype=torch.float32, device=eng.device)
    u8 = torch.full((pad + n + pad,), 0xAB, dtype=torch.uint8, device=eng.device)
    eng._call("cs_parser_input", B, crops, Hc, Wc, halve, lut, pv[pad:], None)
    eng._call("cs_parser_input", B, crops, Hc, Wc, halve, lut, None, u8[pad:])
    _check({"pixel_values": pv[pad:pad + n].view(ref["pixel_values"].shape), "resized_u8": u8[pad:pad + n].view(ref["resized_u8"].shape)}, ref, name)
    assert bool((pv[:pad] == -7.0).all()) and bool((pv[pad + n:] == -7.0).all())
    assert bool((u8[:pad] == 0xAB).all()) and bool((u8[pad + n:] == 0xAB).all())


@pytest.mark.parametrize("name,halve", [("r5x7", 0), ("r2x3", 1), ("r16x4", 1)])
def test_unaligned_buffers_take_the_element_stores(eng, name, halve):
    """Outputs at addresses off the 16-byte / 4-byte boundaries of the wide stores: the same bits, nothing before or beyond."""
    from canonswap_amd import tail
    ref = PR.reference(name, "random", halve)
    n, pad = ref["resized_u8"].size, 64
    pvb = torch.full((pad + n + pad,), -7.0, dtype=torch.float32, device=eng.device)
    u8b = torch.full((pad + n + pad,), 0xAB, dtype=torch.uint8, device=eng.device)
    pv, u8 = pvb[pad + 1:pad + 1 + n].view(ref["pixel_values"].shape), u8b[pad + 1:pad + 1 + n].view(ref["resized_u8"].shape)
    assert pv.data_ptr() % 16 == 4 and u8.data_ptr() % 4 == 1
    got = tail.parser_input(eng, _t(ref["crops"]).cuda(), halve=halve, out=pv, out_u8=u8)
    assert got["pixel_values"] is pv and got["resized_u8"] is u8
    _check(got, ref, name)
    assert bool((pvb[:pad + 1] == -7.0).all()) and bool((pvb[pad + 1 + n:] == -7.0).all())
    assert bool((u8b[:pad + 1] == 0xAB).all()) and bool((u8b[pad + 1 + n:] == 0xAB).all())


# ------------------------------------------------------------------------------------------------ inputs, outputs, constants
def test_input_forms_and_output_buffers(eng, swapper_m):
    from canonswap_amd import tail
    ref = PR.reference("r33x65", "random", 0)
    crops = _t(ref["crops"]).cuda()
    want = tail.parser_input(eng, crops, want_u8=True)
    _check(want, ref, "device input")
    one = tail.parser_input(eng, crops[1], want_u8=True)                          # (H,W,3): one frame
    assert tuple(one["pixel_values"].shape) == (1, 3, 66, 130)
    assert torch.equal(one["pixel_values"], want["pixel_values"][1:2]) and torch.equal(one["resized_u8"], want["resized_u8"][1:2])
    host = tail.parser_input(eng, _t(ref["crops"].copy()))          # host input is uploaded; without want_u8: the tensor
    assert isinstance(host, torch.Tensor) and host.device == eng.device and torch.equal(host, want["pixel_values"])
    assert torch.equal(tail.parser_input(eng, ref["crops"].copy()), want["pixel_values"])      # a numpy array as well
    nc = crops.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not nc.is_contiguous() and torch.equal(tail.parser_input(eng, nc), want["pixel_values"])
    out = torch.empty((2, 3, 66, 130), dtype=torch.float32, device=eng.device)
    out_u8 = torch.empty((2, 66, 130, 3), dtype=torch.uint8, device=eng.device)
    got = tail.parser_input(eng, crops, out=out, out_u8=out_u8)
    assert got["pixel_values"] is out and got["resized_u8"] is out_u8
    assert torch.equal(out, want["pixel_values"]) and torch.equal(out_u8, want["resized_u8"])
    assert tail.parser_input(eng, crops, out=out) is out
    assert torch.equal(swapper_m.parser_input(crops), want["pixel_values"])
    for bad in (crops.float(), crops[..., :2], crops[0, 0], torch.zeros((0, 4, 4, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            tail.parser_input(eng, bad)
    with pytest.raises(ValueError):
        tail.parser_input(eng, crops, halve=True)                                 # 33 x 65 cannot be halved
    with pytest.raises(ValueError):
        tail.parser_input(eng, crops, out=torch.empty((2, 3, 66, 130), dtype=torch.float64, device=eng.device))
    with pytest.raises(ValueError):
        tail.parser_input(eng, crops, out_u8=torch.empty((2, 3, 66, 130), dtype=torch.uint8, device=eng.device))


def test_custom_constants_change_only_the_table(eng):
    from canonswap_amd import tail
    ref = PR.reference("r5x7", "random", 0)
    crops = _t(ref["crops"]).cuda()
    mean, std, rescale = (0.5, 0.25, 0.125), (0.5, 0.25, 2.0), 1 / 128
    got = tail.parser_input(eng, crops, mean=mean, std=std, rescale=rescale, want_u8=True)
    _check(got, PR.restate(ref["crops"], 0, PR.table(mean, std, rescale)), "custom constants")
    assert torch.equal(got["resized_u8"].cpu(), _t(ref["resized_u8"]))
    again = tail.parser_input(eng, crops)                                         # the defaults' table is still the defaults'
    assert _same_bits(again, ref["pixel_values"])
    n = len(eng._tables)
    assert n >= 2
    tail.parser_input(eng, crops, mean=mean, std=std, rescale=rescale)
    tail.parser_input(eng, crops, mean=list(mean), std=np.array(std), rescale=rescale)
    assert len(eng._tables) == n                                             # cached per engine and constants


def test_default_halving_and_the_staged_intermediate(eng):
    """halve=None halves 512 x 512 crops and nothing else; with halve=1 the halved image is what cs_prepare_crops stages (times 255)."""
    from canonswap_amd import tail
    r = np.random.Generator(np.random.PCG64(4201))
    big = _t(r.integers(0, 256, size=(2, 512, 512, 3), dtype=np.uint8)).cuda()
    got = tail.parser_input(eng, big, want_u8=True)
    assert tuple(got["pixel_values"].shape) == (2, 3, 512, 512)
    h1 = tail.parser_input(eng, big, halve=1, want_u8=True)
    assert torch.equal(got["pixel_values"], h1["pixel_values"]) and torch.equal(got["resized_u8"], h1["resized_u8"])
    small = _t(PR.reference("full", "random", 0)["crops"]).cuda()
    got = tail.parser_input(eng, small, want_u8=True)
    assert tuple(got["pixel_values"].shape) == (2, 3, 512, 512)
    h0 = tail.parser_input(eng, small, halve=0, want_u8=True)
    assert torch.equal(got["pixel_values"], h0["pixel_values"]) and torch.equal(got["resized_u8"], h0["resized_u8"])
    I = tail.prepare_crops(eng, big)                                              # (2,3,256,256) fp32 = halved byte / 255
    staged = torch.round(I * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert float((I * 255 - torch.round(I * 255)).abs().max()) < 1e-3             # the staging is a byte over 255
    assert torch.equal(staged.cpu(), _t(PR.halve_u8(big.cpu().numpy())))
    from_staged = tail.parser_input(eng, staged, halve=0, want_u8=True)
    assert torch.equal(from_staged["pixel_values"], h1["pixel_values"]) and torch.equal(from_staged["resized_u8"], h1["resized_u8"])


# ------------------------------------------------------------------------------------------------ argument checks
def test_c_side_refusals_name_the_entry_point_and_launch_nothing(eng):
    from canonswap_amd import tail
    from canonswap_amd.engine import _ptr
    crops = _t(PR.reference("r5x7", "random", 1)["crops"]).cuda()   # (3,10,14,3)
    lut = _t(tail.parser_lut()).cuda()
    pv = torch.full((3, 3, 20, 28), -7.0, dtype=torch.float32, device=eng.device)
    u8 = torch.full((3, 20, 28, 3), 7, dtype=torch.uint8, device=eng.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = eng.lib
    base = dict(e=eng.h, B=3, crops=_ptr(crops), Hc=10, Wc=14, halve=0, lut=_ptr(lut), pv=_ptr(pv), u8=_ptr(u8))

    def call(**kw):
        a = dict(base, **kw)
        rc = lib.cs_parser_input(a["e"], a["B"], a["crops"], a["Hc"], a["Wc"], a["halve"], a["lut"], a["pv"], a["u8"], st)
        return rc, lib.cs_last_error().decode()

    refused = [({"e": None}, "NULL engine"), ({"crops": None}, "NULL crops"), ({"lut": None}, "NULL lut"), ({"pv": None, "u8": None}, "both outputs"),
               ({"B": 0}, "B = 0"), ({"B": -2}, "B = -2"), ({"Hc": 0}, "Hc = 0"), ({"Wc": -1}, "Wc = -1"),
               ({"halve": 1, "Hc": 9}, "odd"), ({"halve": 1, "Wc": 13}, "odd"), ({"halve": 2}, "halve 2"), ({"halve": -1}, "halve -1"),
               ({"Hc": 8193}, "16384"), ({"Wc": 8193}, "16384"), ({"halve": 1, "Hc": 16386}, "16384"), ({"Wc": 2 ** 30 + 1}, "16384")]
    for kw, word in refused:
        rc, err = call(**kw)
        assert rc != 0 and "cs_parser_input" in err and word in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((pv == -7.0).all()) and bool((u8 == 7).all())                     # a refused call launches nothing
    rc, _ = call()
    assert rc == 0
    rc, _ = call(halve=1, pv=None, u8=_ptr(u8))                                   # the same crops halved: (3,10,14,3) -> (3,10,14,3)
    assert rc == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        tail.parser_input(eng, torch.zeros((1, 8193, 2, 3), dtype=torch.uint8))   # refused before anything is uploaded


# ------------------------------------------------------------------------------------------------ the chains
def _chain_batch(B, seed, Ho=360, Wo=640):
    from canonswap_amd import synth
    r = np.random.Generator(np.random.PCG64(seed))
    smooth = synth.make_smooth_images(B, seed=2500 + seed, size=512)
    crops = _t(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda()
    masks = _t(chain_helpers._masks(B, seed=seed)).cuda()
    ori = _t(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
    Ms = np.stack([_affine(j % 4, Ho, Wo) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(B)])
    return crops, masks, Ms, ori


def test_both_chains_return_the_bits_of_tail_parser_input(swapper_m):
    from canonswap_amd import tail
    from canonswap_amd.chain import AnimateChain, FrameChain
    crops = _chain_batch(2, 101)[0]
    want = tail.parser_input(swapper_m.engine, crops, want_u8=True)
    assert tuple(want["pixel_values"].shape) == (2, 3, 512, 512)
    _check(want, PR.restate(crops.cpu().numpy(), 1), "chain crops")
    for chain in (FrameChain(swapper_m), AnimateChain(swapper_m)):                # AnimateChain needs no source for it
        got = chain.parser_input(crops, want_u8=True)
        assert torch.equal(got["pixel_values"], want["pixel_values"]) and torch.equal(got["resized_u8"], want["resized_u8"])
        assert torch.equal(chain.parser_input(crops), want["pixel_values"])
        small = chain.parser_input(crops[:, ::2, ::2].contiguous(), halve=0)      # kw reach tail.parser_input
        assert tuple(small.shape) == (2, 3, 512, 512)


def test_parser_input_between_prefetch_and_call_leaves_the_chain_alone(swapper_m):
    """B = 2: prefetch(next), parser_input(next) on the caller's stream while stage A runs on the side stream, then __call__(current) and
    __call__(next): frames bit-equal to the same run without parser_input, and parser_input's own result right."""
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import FrameChain
    idv = _t(synth.make_identity(7)).cuda()
    cur, nxt = _chain_batch(2, 111), _chain_batch(2, 112)
    chain = FrameChain(swapper_m)

    def run(with_parser):
        chain.prefetch(nxt[0], nxt[1])
        pv = chain.parser_input(nxt[0]).clone() if with_parser else None
        a = chain(cur[0], cur[1], cur[2], cur[3], idv)["frames"].clone()
        b = chain(nxt[0], nxt[1], nxt[2], nxt[3], idv)["frames"].clone()
        torch.cuda.synchronize()
        assert not chain._pending
        return a, b, pv

    a0, b0, _ = run(False)
    a1, b1, pv = run(True)
    assert not torch.equal(a0, b0)
    assert torch.equal(a1, a0) and torch.equal(b1, b0)
    assert torch.equal(pv, tail.parser_input(swapper_m.engine, nxt[0]))
    assert _same_bits(pv, PR.restate(nxt[0].cpu().numpy(), 1)["pixel_values"])
