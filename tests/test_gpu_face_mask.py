"""The face mask from the parser's logits on the device (cs_face_masks; tail.face_masks; FrameChain / AnimateChain with logits=): the
lines between SegFormer and SoftErosion (src/can_swap_pipeline_e2e.py:183-190, src/can_swap_pipeline_v2i.py:76-83) in one kernel.  The
yardstick is those torch lines in float64 on the host (tests/face_mask_ref.py): labels and mask equal on every decided pixel (margin
>= 1e-5 max|logit|), at most 1e-3 of an input's pixels undecided; the same rule against the fp32 lines run on the device."""
import numpy as np
import pytest
import torch

import chain_helpers
import face_mask_ref as FR
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


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_parity_with_the_float64_lines(eng, name):
    from canonswap_amd import tail
    size = FR.CASES[name][1]
    got = tail.face_masks(eng, FR.logits_of(name).cuda(), size=size, want_labels=True)
    B = FR.CASES[name][0][0]
    for k in ("masks", "labels"):
        assert got[k].dtype == torch.uint8 and tuple(got[k].shape) == (B,) + size and got[k].device == eng.device
    ref = FR.reference(name)
    wrong = int(((got["labels"].cpu() != ref["labels"]) & ~ref["decided"]).sum())
    print(f"{name}: undecided {FR.undecided_fraction(ref):.3g} of the pixels, {wrong} of them labelled otherwise than float64")
    FR.assert_agrees(ref, got["labels"], got["masks"], name)
    assert torch.equal(got["masks"].cpu(), torch.isin(got["labels"].cpu().long(), torch.tensor(FR.FACE_VALID)).to(torch.uint8))


@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_parity_with_the_fp32_lines_on_the_device(eng, name):
    """The reference's own lines on the same device in fp32: under the same rule (both sides are fp32 evaluations of the float64 value)."""
    from canonswap_amd import tail
    size = FR.CASES[name][1]
    lg = FR.logits_of(name).cuda()
    got = tail.face_masks(eng, lg, size=size, want_labels=True)
    labels, mask = FR.torch_lines(lg, size)
    ref = FR.reference(name)
    dec = ref["decided"]
    differ = got["labels"].cpu().long() != labels.cpu()
    print(f"{name}: {int(differ.sum())} pixels differ from the device's fp32 lines, {int((differ & dec).sum())} of them decided")
    FR.assert_agrees(ref, labels, mask, name + " (torch on the device)")
    assert not bool((differ & dec).any())
    assert not bool(((got["masks"].cpu() != mask.cpu().to(torch.uint8)) & dec).any())


def test_one_frame_and_other_dtypes_and_layouts(eng, swapper_m):
    """(C,h,w) is one frame; fp64 / fp16-representable / non-contiguous logits are converted with .float().contiguous(); the swapper's method."""
    from canonswap_amd import tail
    lg = FR.logits_of("borders").cuda()
    want = tail.face_masks(eng, lg, size=(20, 28))
    assert torch.equal(tail.face_masks(eng, lg[1], size=(20, 28)), want[1:2])
    assert torch.equal(tail.face_masks(eng, lg.double(), size=(20, 28)), want)
    nc = lg.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and torch.equal(tail.face_masks(eng, nc, size=(20, 28)), want)
    assert torch.equal(swapper_m.face_masks(lg, size=(20, 28)), want)
    assert torch.equal(tail.face_masks(eng, FR.logits_of("borders"), size=(20, 28)), want)          # host logits are uploaded


# ------------------------------------------------------------------------------------------------ first maximum
def _integer_planes(h=6, w=9, C=19):
    r = np.random.Generator(np.random.PCG64(61))
    return torch.from_numpy(r.integers(-8, 0, size=(2, C, h, w)).astype(np.float32))          # integers interpolate exactly in any order


def test_equal_maxima_give_the_first_class(eng):
    from canonswap_amd import tail
    lg = _integer_planes()
    top = torch.from_numpy(np.random.Generator(np.random.PCG64(62)).integers(1, 9, size=(2, 6, 9)).astype(np.float32))
    lg[:, 3] = top
    lg[:, 5] = top                                                                # classes 3 and 5 equal and largest everywhere
    for s in (1, 2, 4):
        got = tail.face_masks(eng, lg.cuda(), size=(6 * s, 9 * s), want_labels=True)
        assert bool((got["labels"] == 3).all()) and bool((got["masks"] == 0).all()), s      # 3 is not a face class, 5 is
        labels, _ = FR.torch_lines(lg, (6 * s, 9 * s))
        assert bool((labels == 3).all())


def test_a_later_class_wins_only_where_it_is_larger(eng):
    from canonswap_amd import tail
    lg = _integer_planes(h=6, w=8)
    ramp = torch.arange(8, dtype=torch.float32).expand(2, 6, 8)                   # class 5: 0 .. 7 along x; class 3: constant 3.5 (exact at every scale)
    lg[:, 5] = ramp
    lg[:, 3] = 3.5
    for s in (1, 2, 4):
        got = tail.face_masks(eng, lg.cuda(), size=(6 * s, 8 * s), want_labels=True)
        labels, mask = FR.torch_lines(lg.double(), (6 * s, 8 * s))
        assert set(labels.unique().tolist()) == {3, 5}
        assert torch.equal(got["labels"].cpu().long(), labels), s
        assert torch.equal(got["masks"].cpu(), mask.to(torch.uint8)), s
        right = got["labels"][:, :, 4 * s + s // 2:]                              # source coordinate >= 4: class 5 >= 4 > 3.5
        assert bool((right == 5).all()) and bool((got["masks"][:, :, 4 * s + s // 2:] == 1).all())
        assert bool((got["labels"][:, :, :3 * s] == 3).all()) and bool((got["masks"][:, :, :3 * s] == 0).all())


# ------------------------------------------------------------------------------------------------ valid set, outputs
def test_valid_sets(eng):
    from canonswap_amd import tail
    lg = FR.logits_of("borders").cuda()
    size = (20, 28)
    both = tail.face_masks(eng, lg, size=size, want_labels=True)
    labels = both["labels"].cpu().long()
    assert len(labels.unique()) > 8
    assert bool((tail.face_masks(eng, lg, valid=(), size=size) == 0).all())
    assert bool((tail.face_masks(eng, lg, valid=range(32), size=size) == 1).all())
    assert torch.equal(both["masks"].cpu(), torch.isin(labels, torch.tensor(tail.FACE_VALID)).to(torch.uint8))
    odd = (0, 3, 18)
    assert torch.equal(tail.face_masks(eng, lg, valid=odd, size=size).cpu(), torch.isin(labels, torch.tensor(odd)).to(torch.uint8))
    assert torch.equal(tail.face_masks(eng, lg, valid=odd + (19, 25, 31), size=size), tail.face_masks(eng, lg, valid=odd, size=size))      # bits >= C
    # masks alone, labels alone (straight through the C entry point: the Python wrapper always asks for masks) and both: the same bytes
    only_l = torch.full((3, 20, 28), 99, dtype=torch.uint8, device=eng.device)
    only_m = torch.full((3, 20, 28), 99, dtype=torch.uint8, device=eng.device)
    eng._call("cs_face_masks", 3, 19, lg, 5, 7, 4, tail.valid_bits(tail.FACE_VALID), None, only_l)
    eng._call("cs_face_masks", 3, 19, lg, 5, 7, 4, tail.valid_bits(tail.FACE_VALID), only_m, None)
    assert torch.equal(only_l, both["labels"]) and torch.equal(only_m, both["masks"])


@pytest.mark.parametrize("name,shift", [("borders", 0), ("borders", 1), ("s2", 0), ("s2", 1), ("s1", 3), ("pipeline", 0)])
def test_exactly_the_outputs_bytes_are_written(eng, name, shift):
    """Outputs inside sentinel-filled buffers longer than needed, at an aligned and at an odd address (the byte-wise stores): the right
    bytes inside, nothing before or beyond."""
    from canonswap_amd import tail
    (B, _, _, _), (H, W) = FR.CASES[name]
    n, pad = B * H * W, 4096
    lg = FR.logits_of(name).cuda()
    want = tail.face_masks(eng, lg, size=(H, W), want_labels=True)
    bm = torch.full((pad + n + pad,), 0xAB, dtype=torch.uint8, device=eng.device)
    bl = torch.full((pad + n + pad,), 0xCD, dtype=torch.uint8, device=eng.device)
    a = pad + shift
    om, ol = bm[a:a + n].view(B, H, W), bl[a:a + n].view(B, H, W)
    assert om.data_ptr() % 4 == shift % 4
    got = tail.face_masks(eng, lg, size=(H, W), out=om, out_labels=ol)
    assert got["masks"] is om and got["labels"] is ol
    assert torch.equal(om, want["masks"]) and torch.equal(ol, want["labels"])
    assert bool((bm[:a] == 0xAB).all()) and bool((bm[a + n:] == 0xAB).all())
    assert bool((bl[:a] == 0xCD).all()) and bool((bl[a + n:] == 0xCD).all())


def test_stream_order_and_reuse(eng):
    from canonswap_amd import tail
    a, b = FR.logits_of("s2").cuda(), FR.logits_of("s2").flip(1).contiguous().cuda()
    size = (12, 20)
    wa, wb = tail.face_masks(eng, a, size=size).clone(), tail.face_masks(eng, b, size=size).clone()
    assert not torch.equal(wa, wb)
    out = torch.empty((2, 12, 20), dtype=torch.uint8, device=eng.device)
    tail.face_masks(eng, a, size=size, out=out)
    tail.face_masks(eng, b, size=size, out=out)
    assert torch.equal(out, wb)                                                   # the second call's result, in launch order
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = tail.face_masks(eng, a, size=size)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, wa)


# ------------------------------------------------------------------------------------------------ the chains
def _chain_batch(B, seed, Ho=360, Wo=640):
    from canonswap_amd import synth
    r = np.random.Generator(np.random.PCG64(seed))
    smooth = synth.make_smooth_images(B, seed=2400 + seed, size=512)
    crops = torch.from_numpy(np.ascontiguousarray((smooth.transpose(0, 2, 3, 1) * 255).astype(np.uint8))).cuda()
    logits = torch.from_numpy(FR.face_field(B, seed=seed)).cuda()
    ori = torch.from_numpy(r.integers(0, 256, size=(B, Ho, Wo, 3), dtype=np.uint8)).cuda()
    Ms = np.stack([_affine(j % 4, Ho, Wo) * np.array([[0.4], [0.4], [1]]) + np.array([[0, 0, 60.], [0, 0, 10.], [0, 0, 0]]) for j in range(B)])
    return crops, logits, Ms, ori


def test_frame_chain_with_logits_equals_the_chain_with_their_masks(swapper_m):
    """In-line, through prefetch, and with two batches staged and run out of order: bit-equal frames (and soft masks) to the same call fed
    with masks=face_masks(logits)."""
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import FrameChain
    e = swapper_m.engine
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    batches = [_chain_batch(2, 71), _chain_batch(2, 72)]
    chain = FrameChain(swapper_m)
    want = []
    for crops, logits, Ms, ori in batches:
        masks = tail.face_masks(e, logits)
        frac = float(masks.float().mean())
        assert 0.05 < frac < 0.7, frac                                             # a face-sized region
        res = chain(crops, masks, Ms, ori, idv, keep=True)
        want.append((res["frames"].clone(), res["soft_mask"].clone()))
    assert not torch.equal(want[0][0], want[1][0])
    for k, (crops, logits, Ms, ori) in enumerate(batches):                        # in-line
        res = chain(crops, None, Ms, ori, idv, keep=True, logits=logits)
        assert torch.equal(res["frames"], want[k][0]) and torch.equal(res["soft_mask"], want[k][1]), k
    crops, logits, Ms, ori = batches[0]                                           # prefetch, then the hit
    chain.prefetch(crops, logits=logits)
    res = chain(crops, None, Ms, ori, idv, keep=True, logits=logits)
    assert torch.equal(res["frames"], want[0][0]) and torch.equal(res["soft_mask"], want[0][1])
    chain.prefetch(batches[0][0], logits=batches[0][1])                           # two staged, run out of order
    chain.prefetch(batches[1][0], logits=batches[1][1])
    r1 = chain(batches[1][0], None, batches[1][2], batches[1][3], idv, keep=True, logits=batches[1][1])
    f1, s1 = r1["frames"].clone(), r1["soft_mask"].clone()
    r0 = chain(batches[0][0], None, batches[0][2], batches[0][3], idv, keep=True, logits=batches[0][1])
    torch.cuda.synchronize()
    assert torch.equal(f1, want[1][0]) and torch.equal(s1, want[1][1])
    assert torch.equal(r0["frames"], want[0][0]) and torch.equal(r0["soft_mask"], want[0][1])
    assert not chain._pending
    other = FrameChain(swapper_m, valid=(1,))                                     # the constructor's valid set is the one used
    res = other(crops, None, Ms, ori, idv, keep=True, logits=logits)
    alone = chain(crops, tail.face_masks(e, logits, valid=(1,)), Ms, ori, idv, keep=True)
    assert torch.equal(res["soft_mask"], alone["soft_mask"]) and not torch.equal(res["soft_mask"], want[0][1])


def test_animate_chain_source_from_logits_equals_the_one_from_their_mask(swapper_m):
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import AnimateChain
    e = swapper_m.engine
    crops, logits, Ms, ori = _chain_batch(1, 81, Ho=300, Wo=420)
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    mask = tail.face_masks(e, logits)[0]
    a, b = AnimateChain(swapper_m), AnimateChain(swapper_m)
    a.set_source(crops[0], mask, Ms[0], ori[0], idv)
    b.set_source(crops[0], None, Ms[0], ori[0], idv, logits=logits[0])
    sa, sb = a.source_state(), b.source_state()
    assert set(sa) == set(sb)
    for k in sa:
        same = torch.equal(sa[k], sb[k]) if isinstance(sa[k], torch.Tensor) else np.array_equal(sa[k], sb[k])
        assert same, k
    assert float(sa["mask_ori"].max()) > 0.5
    b.set_source(crops[0], None, Ms[0], ori[0], idv, logits=logits)               # (1,C,h,w) as well
    assert torch.equal(b.source_state()["mask_ori"], sa["mask_ori"])


# ------------------------------------------------------------------------------------------------ argument checks
def test_python_argument_checks(eng, swapper_m):
    from canonswap_amd import synth, tail
    from canonswap_amd.chain import AnimateChain, FrameChain
    lg = FR.logits_of("borders").cuda()
    for size in ((15, 21), (40, 56), (20, 27), (20, 14), (5, 28), (0, 0)):          # not s * (5, 7) with s in {1, 2, 4}
        with pytest.raises(ValueError):
            tail.face_masks(eng, lg, size=size)
    with pytest.raises(ValueError):
        tail.face_masks(eng, torch.zeros((1, 33, 5, 7), device=eng.device), size=(20, 28))
    for bad in ((32,), (-1,), (1, 40)):
        with pytest.raises(ValueError):
            tail.face_masks(eng, lg, valid=bad, size=(20, 28))
        with pytest.raises(ValueError):
            FrameChain(swapper_m, valid=bad)
        with pytest.raises(ValueError):
            AnimateChain(swapper_m, valid=bad)
    with pytest.raises(ValueError):
        tail.face_masks(eng, lg[0, 0], size=(20, 28))                             # (h,w): no class axis
    with pytest.raises(ValueError):
        tail.face_masks(eng, lg, size=(20, 28), out=torch.empty((3, 20, 28), dtype=torch.float32, device=eng.device))
    crops, logits, Ms, ori = _chain_batch(2, 91)
    masks = tail.face_masks(eng, logits)
    idv = torch.from_numpy(synth.make_identity(7)).cuda()
    chain = FrameChain(swapper_m)
    with pytest.raises(ValueError):
        chain(crops, masks, Ms, ori, idv, logits=logits)
    with pytest.raises(ValueError):
        chain(crops, None, Ms, ori, idv)
    with pytest.raises(ValueError):
        chain.prefetch(crops, masks, logits=logits)
    with pytest.raises(ValueError):
        chain.prefetch(crops)
    assert not chain._pending
    an = AnimateChain(swapper_m)
    with pytest.raises(ValueError):
        an.set_source(crops[0], masks[0], Ms[0], ori[0], idv, logits=logits[0])
    with pytest.raises(ValueError):
        an.set_source(crops[0], None, Ms[0], ori[0], idv)
    with pytest.raises(ValueError):
        an.set_source(crops[0], None, Ms[0], ori[0], idv, logits=logits)          # two frames' logits for one source


def test_c_side_refusals_name_their_reason(eng):
    import ctypes as C
    from canonswap_amd.engine import _ptr
    lg = FR.logits_of("borders").cuda()
    out = torch.full((3, 20, 28), 7, dtype=torch.uint8, device=eng.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, h = eng.lib, eng.h

    def call(B=3, Cn=19, hh=5, ww=7, scale=4, masks=out, labels=None):
        return lib.cs_face_masks(h, B, Cn, _ptr(lg), hh, ww, scale, 0x1cf6, _ptr(masks), _ptr(labels), st), lib.cs_last_error().decode()

    for kw, word in (({"scale": 3}, "scale 3"), ({"scale": 0}, "scale 0"), ({"scale": 8}, "scale 8"), ({"Cn": 0}, "0 classes"), ({"Cn": 33}, "33 classes"),
                     ({"B": 0}, "B = 0"), ({"hh": 0}, "h = 0"), ({"ww": -1}, "w = -1"), ({"masks": None}, "both outputs")):
        rc, err = call(**kw)
        assert rc != 0 and "cs_face_masks" in err and word in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                 # a refused call launches nothing
    rc, _ = call()
    assert rc == 0
