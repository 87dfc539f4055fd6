"""getid on the engine (cs_identity, cs_identity_u8; csrc/identity.hip): the whole network, its stages and its kernels against the float64
restatement of tests/identity_ref.py, the input forms, batching, determinism, stream order and the wiring into can_swapper.

Tolerance of every comparison with the network in it: relative L2 error per row <= 4 x the error of the restatement's fp16-operand emulation
(measured here on the CPU; a property of the restatement, never of the engine).  The emulation rounds only the operands of the convolutions
and linear layers; the engine also stores activations and the folded BatchNorm scales in fp16 - about one more rounding of that size per
layer - and sums in another order.  tests/test_identity_cpu.py shows that real mistakes are more than 10 x above this bound.
The kernels alone have bounds from their number formats, stated where they are used."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import identity_ref as R
from chain_helpers import _occupy
from hip_ops import op

pytestmark = pytest.mark.gpu
FACTOR = 4.0


# ------------------------------------------------------------------------------------------------ shared inputs and references (computed once)
@pytest.fixture(scope="module")
def sd_np():
    from canonswap_amd import synth
    return synth._arcface(0)


@pytest.fixture(scope="module")
def blobs(state_dicts, sd_np):
    from canonswap_amd import pack, synth
    return pack.build_blobs(dict(state_dicts, arcface=synth.to_torch({"a": sd_np})["a"]))


@pytest.fixture(scope="module")
def swapper(blobs):
    from canonswap_amd.can_swap_e2e import can_swapper
    return can_swapper(None, packed_blobs=blobs, max_batch=4)


@pytest.fixture(scope="module")
def imgs():
    """Four 112 x 112 inputs: two synthetic faces' worth of smooth images, the constant 0.5, and an image that is zero except for one pixel
    in each corner (where the unpadded stem, the 110 -> 55 pool, stride 2 on an odd extent and bn0-then-zero-padding go wrong)."""
    from canonswap_amd import synth
    x = synth.make_identity_inputs(4, seed=3000, size=112)
    x[2] = 0.5
    x[3] = 0
    for (h, w), v in zip(((0, 0), (0, 111), (111, 0), (111, 111)), (2.5, -2.0, 1.5, -1.0)):
        x[3, :, h, w] = v
    return torch.from_numpy(x)


@pytest.fixture(scope="module")
def ref(sd_np, imgs):
    """float64 restatement and its fp16-operand emulation for the four inputs, on the CPU; per stage and row the emulation's error."""
    sd = R.to_tensors(sd_np)
    with torch.no_grad():
        f64 = R.forward(sd, imgs.double())
        emu = R.forward(sd, imgs.double(), emulate=True)
    err = {k: R.rel_l2(emu[k], f64[k]) for k in R.STAGES + ("raw",)}
    d = lambda a: (a["raw"][0] - a["raw"][1])[None]
    err["diff"] = R.rel_l2(d(emu), d(f64))
    print("emulation vs float64, relative L2 per row:", {k: [f"{v:.2e}" for v in e.tolist()] for k, e in err.items()})
    print("1 - cos of the emulation's embeddings:", (1 - F.cosine_similarity(emu["raw"], f64["raw"], dim=1)).tolist(),
          "cos(row 0, row 1):", float(F.cosine_similarity(f64["raw"][0], f64["raw"][1], dim=0)))
    return {"f64": f64, "err": err}


# ------------------------------------------------------------------------------------------------ 1-5: the network
@pytest.mark.parametrize("rows", [(0,), (0, 2, 3)], ids=["b1", "b3"])
def test_whole_network_against_float64(swapper, imgs, ref, rows):
    rows = list(rows)
    idn, raw = swapper.engine.identity(imgs[rows].cuda(), want_raw=True)
    err = R.rel_l2(raw, ref["f64"]["raw"][rows])
    tol = FACTOR * ref["err"]["raw"][rows]
    print("engine vs float64:", err.tolist(), "bound:", tol.tolist(), "1 - cos:", (1 - F.cosine_similarity(raw.double().cpu(), ref["f64"]["raw"][rows], dim=1)).tolist())
    assert bool((err <= tol).all())
    # 4: the normalised output is F.normalize of the raw one to fp32 rounding, with unit norm
    want = F.normalize(raw.double(), p=2, dim=1)
    assert float((idn.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert float((idn.double().norm(dim=1) - 1).abs().max()) <= 2e-6


def test_difference_of_two_embeddings(swapper, imgs, ref):
    """Two embeddings share most of their value; an error in the common part hides in each row's own comparison, not in their difference."""
    raw = swapper.engine.identity(imgs[:2].cuda(), normalize=False).double().cpu()
    want = ref["f64"]["raw"]
    err = R.rel_l2((raw[0] - raw[1])[None], (want[0] - want[1])[None])
    print("difference of rows 0 and 1, engine vs float64:", err.tolist(), "bound:", (FACTOR * ref["err"]["diff"]).tolist())
    assert bool((err <= FACTOR * ref["err"]["diff"]).all())


def test_stage_by_stage(swapper, imgs, ref):
    """The activations the pass left, at their valid extents (the engine's tensors have no other: nothing lies outside them)."""
    rows = [0, 2, 3]
    swapper.engine.identity(imgs[rows].cuda())
    for which, k in enumerate(R.STAGES):
        got = swapper.engine.identity_read(which, 3)
        want = ref["f64"][k][rows]
        assert got.shape == want.shape
        err = R.rel_l2(got, want)
        print(k, "engine vs float64:", [f"{v:.2e}" for v in err.tolist()], "bound:", [f"{v:.2e}" for v in (FACTOR * ref["err"][k][rows]).tolist()])
        assert bool((err <= FACTOR * ref["err"][k][rows]).all()), k
    with pytest.raises(RuntimeError, match="last pass held 3"):
        swapper.engine.identity_read(0, 4)


# ------------------------------------------------------------------------------------------------ 6: the kernels alone
def _rand(shape, seed, lo=-1.0, hi=1.0):
    r = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(r.uniform(lo, hi, size=shape).astype(np.float32))


@pytest.mark.parametrize("case", ["3x3_s2_odd", "1x1_s2_f32", "stem_unpadded", "3x3_s1_batch"])
def test_conv_alone(case):
    """fp16 operands, fp32 accumulation of K = taps x Cin products (four partial sums, added in order): |error| <= (K + 4) 2^-24 sum |a w| in
    the worst case, plus the output's own rounding (fp32: 2^-24, fp16: 2^-11).  Odd extents, stride 2, more than one workgroup along both axes."""
    from canonswap_amd import pack
    N, IH, IW, Cin, Cout, K, stride, pad, in_f32, out_f32, act = {
        "3x3_s2_odd": (2, 9, 7, 64, 128, 3, 2, 1, 0, 1, False),
        "1x1_s2_f32": (1, 13, 13, 64, 128, 1, 2, 0, 1, 1, False),
        "stem_unpadded": (1, 12, 11, 32, 64, 3, 1, 0, 0, 1, True),
        "3x3_s1_batch": (3, 7, 7, 96, 64, 3, 1, 1, 0, 0, True),
    }[case]
    x = _rand((N, Cin, IH, IW), 1)
    w = _rand((Cout, Cin, K, K), 2, -0.2, 0.2)
    b = _rand((Cout,), 3)
    slope = torch.tensor([0.25], dtype=torch.float32)
    xq = x if in_f32 else x.half().float()
    xin = (xq if in_f32 else xq.half()).permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.from_numpy(pack.pack_id_conv(w.numpy())).cuda()
    OH, OW = (IH + 2 * pad - K) // stride + 1, (IW + 2 * pad - K) // stride + 1
    out = torch.full((N, OH, OW, Cout), float("nan"), dtype=torch.float32 if out_f32 else torch.float16, device="cuda")
    bd, sd = b.cuda(), slope.cuda()          # named: a temporary's block would be handed to the next allocation while the pointer is still in use
    op("cs_op_id_conv", xin, in_f32, N, IH, IW, Cin, K, stride, pad, wp, bd, Cout, sd if act else None, out, out_f32)
    x64, w64 = x.half().double(), w.half().double()
    want = F.conv2d(x64, w64, b.double(), stride=stride, padding=pad)
    mag = F.conv2d(x64.abs(), w64.abs(), stride=stride, padding=pad) + b.double().abs()[None, :, None, None]
    if act:
        want = torch.where(want > 0, want, want * 0.25)
    got = out.double().cpu().permute(0, 3, 1, 2)
    bound = (K * K * Cin + 4) * 2.0 ** -24 * mag + (2.0 ** -24 if out_f32 else 2.0 ** -11) * want.abs() + 2.0 ** -24
    print(case, "max error", float((got - want).abs().max()), "max bound", float(bound.max()), "max |value|", float(want.abs().max()))
    assert bool(((got - want).abs() <= bound).all())


def test_maxpool_alone():
    """110 -> 55: the maximum is exact; the fp16 copy is fp16(fma(x, s, t))."""
    B, IH, IW, Cc = 2, 110, 110, 64
    x = _rand((B, IH, IW, Cc), 5, -3, 3)
    s, t = _rand((Cc,), 6, 0.5, 1.5), _rand((Cc,), 7)
    xo = torch.empty((B, 55, 55, Cc), dtype=torch.float32, device="cuda")
    ao = torch.empty((B, 55, 55, Cc), dtype=torch.float16, device="cuda")
    xd, sd, td = x.cuda(), s.cuda(), t.cuda()
    op("cs_op_id_maxpool", xd, sd, td, xo, ao, B, IH, IW, Cc)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(xo.cpu(), want)
    a64 = want.double() * s.double() + t.double()
    assert bool(((ao.double().cpu() - a64).abs() <= 2.0 ** -11 * a64.abs() + 2.0 ** -23 * (want.double().abs() * s.double() + t.double().abs()) + 2.0 ** -25).all())


@pytest.mark.parametrize("Cc,E", [(64, 55), (512, 7)])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "even_positions"])
def test_se_and_block_tail_alone(Cc, E, strided):
    """SE gate + tail on a dense map, and on the even positions of a stride-1 map of odd extent 2E - 1.  Bounds: the fp32 mean of P values is
    within P 2^-24 mean|v| of the exact one in the worst case (P <= 3025: 1.8e-4); two unit-gain linear layers and the sigmoid (slope <= 1/4)
    carry at most that into the gate: |se - ref| <= 1e-4.  x = prelu(out se + res): 1e-4 |out| + 2^-22 (|out| + |res|); the fp16 copy adds 2^-11."""
    B, R_ = 2, Cc // 16
    full = 2 * E - 1 if strided else E
    step = 2 if strided else 1
    big = _rand((B, full, full, Cc), 10, -2, 2) + _rand((1, 1, 1, Cc), 11, -0.5, 0.5)
    res = _rand((B, E, E, Cc), 12, -2, 2)
    w1, b1 = _rand((R_, Cc), 13, -(3.0 / Cc) ** 0.5, (3.0 / Cc) ** 0.5), _rand((R_,), 14, -0.1, 0.1)
    w2, b2 = _rand((Cc, R_), 15, -(3.0 / R_) ** 0.5, (3.0 / R_) ** 0.5), _rand((Cc,), 16, -0.1, 0.1)
    slopes = torch.tensor([0.3, 0.15], dtype=torch.float32)          # block PReLU, SE PReLU
    s, t = _rand((Cc,), 17, 0.5, 1.5), _rand((Cc,), 18)
    se = torch.empty((B, Cc), dtype=torch.float32, device="cuda")
    xo = torch.empty((B, E, E, Cc), dtype=torch.float32, device="cuda")
    ao = torch.empty((B, E, E, Cc), dtype=torch.float16, device="cuda")
    g = [v.cuda() for v in (big, w1, b1, w2, b2, slopes, res, s, t)]
    sW = Cc * step
    sH = full * Cc * step
    op("cs_op_id_se_tail", g[0], full * full * Cc, sH, sW, B, E, E, Cc, g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], se, xo, ao)
    o = big[:, ::step, ::step].double()
    assert o.shape[1] == E
    y = F.linear(o.mean(dim=(1, 2)), w1.double(), b1.double())
    y = torch.where(y > 0, y, y * 0.15)
    gate = torch.sigmoid(F.linear(y, w2.double(), b2.double()))
    v = o * gate[:, None, None, :] + res.double()
    want = torch.where(v > 0, v, v * 0.3)
    e_se = float((se.double().cpu() - gate).abs().max())
    print(f"C {Cc} extent {E} strided {strided}: max |se error| {e_se:.2e}, max |x error| {float((xo.double().cpu() - want).abs().max()):.2e}")
    assert e_se <= 1e-4
    bx = 1e-4 * o.abs() + 2.0 ** -22 * (o.abs() + res.double().abs())
    assert bool(((xo.double().cpu() - want).abs() <= bx).all())
    a64 = want * s.double() + t.double()
    assert bool(((ao.double().cpu() - a64).abs() <= 2.0 ** -11 * a64.abs() + bx * s.double() + 2.0 ** -22 * (a64.abs() + t.double().abs()) + 2.0 ** -25).all())


@pytest.mark.parametrize("B", [1, 3])
def test_embedding_alone(B):
    """fc over 49 slices of 512 products each, fp32: |error| <= (512 + 49 + 1) 2^-24 sum |a w| in the worst case; the normalised rows equal
    F.normalize of the raw ones to fp32 rounding (512-term sum of squares: 2^-15 relative is generous by 100 x)."""
    a = _rand((B, 49, 512), 20, -3, 3).half()
    w = _rand((49, 512, 512), 21, -0.011, 0.011).half()
    bias = _rand((512,), 22)
    part = torch.empty((49, B, 512), dtype=torch.float32, device="cuda")
    raw = torch.empty((B, 512), dtype=torch.float32, device="cuda")
    idn = torch.empty((B, 512), dtype=torch.float32, device="cuda")
    ad, wd, bd = a.cuda(), w.cuda(), bias.cuda()
    op("cs_op_id_embed", ad, wd, bd, part, raw, idn, B)
    want = torch.einsum("bpc,poc->bo", a.double(), w.double()) + bias.double()
    mag = torch.einsum("bpc,poc->bo", a.double().abs(), w.double().abs()) + bias.double().abs()
    err = (raw.double().cpu() - want).abs()
    print(f"B {B}: max |error| {float(err.max()):.2e}, max bound {float((562 * 2.0 ** -24 * mag).max()):.2e}, max |value| {float(want.abs().max()):.2f}")
    assert bool((err <= 562 * 2.0 ** -24 * mag).all())
    n = F.normalize(raw.double(), p=2, dim=1).cpu()
    assert float((idn.double().cpu() - n).abs().max()) <= 2.0 ** -15 * float(n.abs().max())
    raw2 = torch.empty_like(raw)
    op("cs_op_id_embed", ad, wd, bd, part, raw2, None, B)
    assert torch.equal(raw, raw2)


# ------------------------------------------------------------------------------------------------ 7-9: input forms, batching, order
@pytest.mark.parametrize("H,W", [(224, 224), (100, 130), (37, 61)])
def test_nearest_resize_is_torch_s(swapper, H, W):
    from canonswap_amd import synth
    x = torch.from_numpy(synth.make_identity_inputs(2, seed=77, size=max(H, W))[:, :, :H, :W].copy()).cuda()
    got = swapper.engine.identity(x, normalize=False)
    want = swapper.engine.identity(F.interpolate(x, size=(112, 112)), normalize=False)
    assert torch.equal(got, want)
    assert float(got.abs().max()) > 0.1


def test_uint8_crops_equal_the_table_s_values(swapper):
    from canonswap_amd import tail
    r = np.random.Generator(np.random.PCG64(9))
    crops = torch.from_numpy(r.integers(0, 256, size=(2, 120, 96, 3), dtype=np.uint8))
    lut = torch.from_numpy(tail.id_lut())
    x = torch.stack([lut[c][crops[..., c].long()] for c in range(3)], dim=1)          # (2, 3, 120, 96)
    # the table is ID_transform: ToTensor (v / 255) then Normalize, in float32
    m, s = torch.tensor(tail.ID_MEAN).view(1, 3, 1, 1), torch.tensor(tail.ID_STD).view(1, 3, 1, 1)
    assert torch.equal(x, (crops.permute(0, 3, 1, 2).float().div(255) - m) / s)
    got = swapper.engine.identity_u8(crops, want_raw=True)
    want = swapper.engine.identity(x.cuda(), want_raw=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(swapper.getid_crops(crops.numpy()), want[0])
    assert torch.equal(swapper.engine.identity_u8(crops[0].cuda()), want[0][:1])


def test_batching_determinism_and_stream_order(swapper, imgs):
    eng = swapper.engine
    x = imgs[[0, 2, 3]].cuda()
    a = eng.identity(x, want_raw=True)
    b = eng.identity(x, want_raw=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in range(3):
        one = eng.identity(x[i:i + 1], want_raw=True)
        assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), i
    out = torch.empty((3, 512), dtype=torch.float32, device="cuda")
    assert eng.identity(x, out=out) is out and torch.equal(out, a[0])
    # a call on a side stream runs on that stream: its input is written there, behind a spin, and the default stream holds nothing it could wait for
    side = torch.cuda.Stream()
    buf = torch.zeros_like(x)
    torch.cuda.synchronize()
    _occupy(side, 20.0)
    with torch.cuda.stream(side):
        buf.copy_(x)
        got = eng.identity(buf)
        done = torch.cuda.Event()
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    assert torch.equal(got, a[0])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 10: wiring
class _TorchArc(torch.nn.Module):
    """A torch identity network with the reference class's state-dict and its (x, x2) return."""

    def __init__(self, sd_np):
        super().__init__()
        from canonswap_amd import synth
        self._sd = synth.to_torch({"a": sd_np})["a"]
        self._t = R.to_tensors(sd_np, torch.float32, "cuda")
        self.calls = 0

    def state_dict(self, *a, **k):
        return self._sd

    def forward(self, x):
        self.calls += 1
        assert tuple(x.shape[2:]) == (112, 112)
        return R.forward(self._t, x)["raw"], None


def test_getid_runs_on_the_engine_and_feeds_the_swap(swapper, imgs):
    from canonswap_amd import synth
    assert swapper.netArc is None and swapper.id_on_engine
    x = imgs[:2].cuda()
    idv = swapper.getid(x)
    assert idv.shape == (2, 512) and idv.is_cuda and torch.equal(idv, swapper.engine.identity(x))
    assert float((idv.double().norm(dim=1) - 1).abs().max()) <= 2e-6
    # the composition: the device tensor goes into the identity slots as it is, and gives the frames the same identity gives as a host-made tensor
    inp = synth.make_frame_inputs(1, seed=1000, size=256)
    args = [torch.from_numpy(inp[k]).cuda() for k in ("img", "x_t", "x_can")]
    one = swapper.getid(x[:1])
    a = swapper.swap_frames(*args, one)["out"].clone()
    host = torch.from_numpy(one.cpu().numpy().copy())
    b = swapper.swap_frames(*args, host.cuda())["out"]
    assert torch.equal(a, b)
    slot = swapper.engine.set_identity(one)
    c = swapper.engine.swap_frames(*args, slots=[slot])["out"]
    assert torch.equal(a, c)


def test_an_injected_module_keeps_precedence_and_can_move_onto_the_engine(swapper, blobs, sd_np, imgs):
    from canonswap_amd.can_swap_e2e import can_swapper
    x = imgs[:2].cuda()
    on_engine = swapper.getid(x)
    plain = {k: v for k, v in blobs.items() if not k.startswith("A.")}
    net = _TorchArc(sd_np)
    sw = can_swapper(None, packed_blobs=blobs, max_batch=2, id_net=net)          # the weights are there too: the module still wins
    got = sw.getid(x)
    assert net.calls == 1 and sw.netArc is net
    with torch.no_grad():
        want = F.normalize(net(F.interpolate(x, size=(112, 112)))[0], p=2, dim=1)
    assert float(R.rel_l2(got, want).max()) < 1e-5 and not torch.equal(got, on_engine)      # torch's fp32 network, not the engine's fp16 one
    assert float(R.rel_l2(got, on_engine).max()) < 5e-3
    del sw
    moved = can_swapper(None, packed_blobs=plain, max_batch=2, id_net=_TorchArc(sd_np), id_on_engine=True)
    assert moved.netArc is None and moved.id_on_engine
    assert torch.equal(moved.getid(x), on_engine)
    del moved
    bare = can_swapper(None, packed_blobs=plain, max_batch=2)
    assert not bare.id_on_engine
    with pytest.raises(RuntimeError, match="no identity network"):
        bare.getid(x)
    with pytest.raises(RuntimeError, match="no identity network"):
        bare.engine.identity(x)


def test_bad_arguments_are_refused_before_any_launch(swapper, imgs):
    eng = swapper.engine
    x = imgs[:1].cuda()
    out = torch.full((4, 512), 7.0, device="cuda")
    lut = torch.zeros((3, 256), device="cuda")
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    bad = [
        ("cs_identity", eng.h, 0, x, 112, 112, out, None),
        ("cs_identity", eng.h, 5, x, 112, 112, out, None),
        ("cs_identity", eng.h, 1, x, 0, 112, out, None),
        ("cs_identity", eng.h, 1, x, 112, -3, out, None),
        ("cs_identity", eng.h, 1, None, 112, 112, out, None),
        ("cs_identity", eng.h, 1, x, 112, 112, None, None),
        ("cs_identity", None, 1, x, 112, 112, out, None),
        ("cs_identity_u8", eng.h, 1, u8, 8, 8, None, out, None),
        ("cs_identity_u8", eng.h, 1, None, 8, 8, lut, out, None),
        ("cs_op_identity_read", eng.h, 9, 1, out),
    ]
    eng.identity(x)
    for name, *args in bad:
        with pytest.raises(RuntimeError, match=rf"(?s){name} failed: .{{11}}"):      # a message of more than 10 characters
            op(name, *args)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        eng.identity(torch.zeros((1, 4, 112, 112)))
    with pytest.raises(ValueError):
        eng.identity_u8(torch.zeros((1, 8, 8, 3)))
