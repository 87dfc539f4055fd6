"""W's dense-motion network kernel by kernel (csrc/kernels.hip and the hourglass / mask / occlusion convs) against float64 restatements.

References read the unpacked synthetic state dict, so pack._pack_W (BN folding, the (kw, c) mask layout, W.occ49 / W.occp, the up-block phase
weights) is checked too.  They multiply the weights the kernels multiply: folded with pack.fold_conv_bn and rounded to fp16 (the phase-form
up-blocks: the fp16 rounding of pack.upsampled_conv3d_phases' tap sums), biases in fp32.  Errors are max |got - ref| / max |ref| per tensor,
broken down where the kernel has structure (key-point slot, border columns / rows / slices, depth slice); every gate records the value measured
on the MI355X and sits within 4x of it.  Output buffers are filled with a sentinel first; what a kernel must not write is asserted untouched.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hip_ops as H

pytestmark = pytest.mark.gpu

SENT16 = 0x7E5A          # fp16 NaN payload: the sentinel of fp16 buffers
CIN = (112, 64, 128, 256, 512)
COUT = (64, 128, 256, 512, 1024)
SKIP = (32, 64, 128, 256, 512, 0)
DEC_OUT = (512, 256, 128, 64, 32)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def wsd():
    from canonswap_amd import synth
    return synth.to_torch(synth.make_state_dicts(0, modules=("warping_module",)))["warping_module"]


@pytest.fixture(scope="module")
def sdd(wsd):
    return {k: v.double() for k, v in wsd.items()}


@pytest.fixture(scope="module")
def wb(wsd):
    """pack._pack_W's blobs on the device"""
    from canonswap_amd import pack
    out = {}
    pack._pack_W(out, pack._np_sd(wsd))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in out.items()}


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def _err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    m = ref.abs().max().item()
    return (got - ref).abs().max().item() / (m if m > 0 else 1.0)         # (an all-zero reference: the absolute error)


def _gate(what, err, gate):
    print(f"\n{what}: {err:.3e} (gate {gate:.1e})")
    assert err <= gate, (what, err, gate)


def _w16(w):
    return torch.from_numpy(np.asarray(w, np.float64).astype(np.float16).astype(np.float64))


def _b32(b):
    return torch.from_numpy(np.asarray(b, np.float64).astype(np.float32).astype(np.float64))


def _folded(wsd, p):
    """(fp16 weight, fp32 bias) of conv p.conv + BN p.norm as float64 tensors"""
    from canonswap_amd import pack
    sd = pack._np_sd(wsd)
    s, t = pack.bn_affine(sd, p + ".norm")
    w, b = pack.fold_conv_bn(sd[p + ".conv.weight"], sd[p + ".conv.bias"], s, t)
    return w, b


def _kps(N, seed):
    from canonswap_amd import synth
    inp = synth.make_frame_inputs(N, seed=seed, size=8)
    return torch.from_numpy(inp["x_t"]), torch.from_numpy(inp["x_can"])      # (driving, source)


def _features(N, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((0.08 * r.standard_normal((N, 32, 16, 64, 64))).astype(np.float32))


# ------------------------------------------------------------------------------------------------ float64 references
def _compress_ref(f, sdd):
    """f [N, 32, D, H, W] -> [N, D, H, W, 4]"""
    from oracle import canonswap_ref as O
    p = "dense_motion_network"
    return F.relu(O.bn_eval(O.conv(f.double(), sdd, p + ".compress", 0), sdd, p + ".norm")).permute(0, 2, 3, 4, 1)


def _sparse_motions(kp_d, kp_s, D, Hh, Ww):
    """[N, 22, D, H, W, 3] float64: slot 0 the identity grid, slot k grid - kp_d[k - 1] + kp_s[k - 1] (dense_motion.py:29-43)"""
    from oracle import canonswap_ref as O
    g = O.make_coordinate_grid(D, Hh, Ww, torch.float64)
    N = kp_d.shape[0]
    d2s = g.view(1, 1, D, Hh, Ww, 3) - kp_d.double().view(N, 21, 1, 1, 1, 3) + kp_s.double().view(N, 21, 1, 1, 1, 3)
    return torch.cat([g.view(1, 1, D, Hh, Ww, 3).expand(N, 1, -1, -1, -1, -1), d2s], 1)


def _sparse_ref(comp, kp_d, kp_s):
    """comp float64 [N, D, H, W, 4] (the kernel's fp16 input) -> [N, D, H, W, 112]: per slot (heat, 4 sampled channels), 2 zero channels"""
    from oracle import canonswap_ref as O
    N, D, Hh, Ww, _ = comp.shape
    sp = _sparse_motions(kp_d, kp_s, D, Hh, Ww)
    rep = comp.permute(0, 4, 1, 2, 3).unsqueeze(1).expand(-1, 22, -1, -1, -1, -1).reshape(N * 22, 4, D, Hh, Ww)
    deformed = O.grid_sample_3d_explicit(rep, sp.reshape(N * 22, D, Hh, Ww, 3)).view(N, 22, 4, D, Hh, Ww)
    heat = O.kp2gaussian(kp_d.double(), D, Hh, Ww) - O.kp2gaussian(kp_s.double(), D, Hh, Ww)
    heat = torch.cat([torch.zeros(N, 1, D, Hh, Ww, dtype=torch.float64), heat], 1).unsqueeze(2)
    out = torch.cat([heat, deformed], 2).permute(0, 3, 4, 5, 1, 2).reshape(N, D, Hh, Ww, 110)
    return torch.cat([out, torch.zeros(N, D, Hh, Ww, 2, dtype=torch.float64)], -1)


def _deform_ref(logits, kp_d, kp_s):
    """logits float64 [N, D, H, W, 22] -> deformation [N, D, H, W, 3] (dense_motion.py:88-94)"""
    N, D, Hh, Ww, _ = logits.shape
    m = torch.softmax(logits, -1)
    sp = _sparse_motions(kp_d, kp_s, D, Hh, Ww)                             # [N, 22, D, H, W, 3]
    return (sp * m.permute(0, 4, 1, 2, 3).unsqueeze(-1)).sum(1)


def _warp_ref(inp_hwdc, deform):
    """inp fp32 HWDC [N, H, W, D, 32], deformation [N, D, H, W, 3] -> float64 HWDC"""
    from oracle import canonswap_ref as O
    x = inp_hwdc.double().permute(0, 4, 3, 1, 2)                             # [N, 32, D, H, W]
    return O.grid_sample_3d_explicit(x, deform.double()).permute(0, 3, 4, 2, 1)


def _occ_ref(part, taps, bias):
    """part [N, H, W, 64 | 16] -> float64 sigmoid(bias + shifted sums), zero padding"""
    p = part.double().cpu()
    N, Hh, Ww, _ = p.shape
    s = torch.full((N, Hh, Ww), float(bias), dtype=torch.float64)
    pp = F.pad(p, (0, 0, 3, 3, 3, 3))                                        # [N, H + 6, W + 6, C]
    for ky in range(7) if taps == 49 else (3,):
        for kx in range(7):
            c = ky * 7 + kx if taps == 49 else kx
            s += pp[:, ky:ky + Hh, kx:kx + Ww, c]
    return torch.sigmoid(s)


def _ulp16(ref):
    r = ref.double().cpu().numpy().astype(np.float16)
    return torch.from_numpy(np.spacing(np.abs(r)).astype(np.float64))


def _within_ulp(what, got, ref, abs_term):
    """every element within one fp16 ulp of the float64 value plus abs_term; prints the worst excess over the ulp"""
    got, ref = got.double().cpu(), ref.double().cpu()
    ex = ((got - ref).abs() - _ulp16(ref)).max().item()
    print(f"\n{what}: max(|d| - ulp16) {ex:.3e} (allowed {abs_term:.1e})")
    assert ex <= abs_term, (what, ex, abs_term)


# ------------------------------------------------------------------------------------------------ dm_compress
@pytest.mark.parametrize("N", [1, 3])
def test_dm_compress(wb, sdd, N):
    """1x1x1 conv 32 -> 4 + folded BN + ReLU, fp16 out: within one fp16 ulp of float64 everywhere; the inputs push some channels below 0."""
    f = _features(N, 900 + N) * 4
    f[:, :, :, :8] -= 0.5                                                    # ReLU clips where the inputs shift
    comp = torch.full((N * 16 * 64 * 64 * 4 + 64,), SENT16, dtype=torch.int16, device="cuda")
    hw = f.permute(0, 3, 4, 2, 1).contiguous().cuda()
    H.dm_compress(hw, wb["W.compress.w"], wb["W.compress.b"], comp[:N * 65536 * 4].view(torch.float16).view(N, 16, 64, 64, 4))
    got = comp[:N * 65536 * 4].view(torch.float16).view(N, 16, 64, 64, 4)
    assert torch.all(comp[N * 65536 * 4:] == SENT16), "dm_compress wrote past its output"
    ref = _compress_ref(f, sdd)
    assert (ref == 0).double().mean() > 0.05 and (ref > 0).double().mean() > 0.05
    assert torch.all(got.cpu()[ref == 0] == 0)
    _within_ulp(f"dm_compress N={N}", got, ref, 1e-6)          # the fp32 sum of 32 products: measured 2.5e-7
    # measured 2.7e-4 (fp16 storage)
    _gate(f"dm_compress N={N}", _err(got, ref), 1.1e-3)


# ------------------------------------------------------------------------------------------------ dm_sparse
def _slot_deltas(kind, N, rng, D, Hh, Ww):
    """kp_d, kp_s [N, 21, 3] for the key-point set `kind`"""
    kd, ks = _kps(N, 4000 + rng)
    if kind == "synthetic":
        return kd, ks
    if kind == "equal":
        return kd, kd.clone()
    if kind == "outside":
        ks = ks.clone()
        ks[:, 7] = kd[:, 7] + torch.tensor([3.0, 0.0, 0.0])                  # slot 8 samples at x >= 2 everywhere
        return kd, ks
    if kind == "edges":
        # sampling points on voxel centres (a shift of a whole number of voxels at W / (W - 1) scale is not one: use half-voxel shifts of
        # the align_corners=False lattice), on the +-1 borders and just past them, along each axis
        dx, dy, dz = 2.0 / Ww, 2.0 / Hh, 2.0 / D
        shifts = [(0, 0, 0), (dx / 2, 0, 0), (-dx / 2, 0, 0), (0, dy / 2, 0), (0, -dy / 2, 0), (0, 0, dz / 2), (0, 0, -dz / 2),
                  (1e-3, 0, 0), (-1e-3, 0, 0), (0, 1e-3, 0), (0, -1e-3, 0), (0, 0, 1e-3), (0, 0, -1e-3),
                  (dx, dy, dz), (-dx, -dy, -dz), (2 - dx, 0, 0), (0, -(2 - dy), 0), (0, 0, 2 - dz), (1.0, 1.0, 1.0), (-1.0, 0.5, -0.5),
                  (2.0, 2.0, 2.0)]
        ks = kd + torch.tensor(shifts, dtype=torch.float32).view(1, 21, 3)
        return kd, ks
    if kind == "grid_node":
        # key-points on grid nodes: the heat map peaks at exactly 1 (driving) / -1 (source) there
        from oracle import canonswap_ref as O
        g = O.make_coordinate_grid(D, Hh, Ww)
        kd, ks = kd.clone(), ks.clone()
        for k in range(21):
            kd[:, k] = g[(3 * k) % D, (5 * k) % Hh, (7 * k) % Ww]
            ks[:, k] = g[(3 * k + 1) % D, (5 * k + 2) % Hh, (7 * k + 3) % Ww]
        return kd, ks
    raise ValueError(kind)


def _run_sparse(comp16, kd, ks, N, shared_comp=False, shared_kps=False, ostride=128):
    D, Hh, Ww = comp16.shape[1:4]
    buf = torch.full((N, D, Hh, Ww, ostride), SENT16, dtype=torch.int16, device="cuda")
    out = buf.view(torch.float16)[..., 8:]                                  # 16-byte aligned rows, 8 guard channels on each side
    H.dm_sparse(comp16.cuda(), kd.cuda().contiguous(), ks.cuda().contiguous(), out, N, shared_comp, shared_kps)
    assert torch.all(buf[..., :8] == SENT16) and torch.all(buf[..., 120:] == SENT16), "dm_sparse wrote outside its 112 channels"
    return out[..., :112].cpu()


def _comp_input(N, D, Hh, Ww, seed):
    r = _rng(seed)
    return (torch.rand(N, D, Hh, Ww, 4, generator=r) * 3).half()


SPARSE_SHAPES = [(1, 16, 64, 64), (2, 8, 24, 40), (2, 5, 9, 17)]


@pytest.mark.parametrize("shape", SPARSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["synthetic", "equal", "outside", "edges", "grid_node"])
def test_dm_sparse(shape, kind):
    """Heat maps and deformed channels of every slot, one fp16 ulp of float64 plus the fp32 exponential / sampling point; borders apart."""
    N, D, Hh, Ww = shape
    comp = _comp_input(N, D, Hh, Ww, 50 + Ww)
    kd, ks = _slot_deltas(kind, N, Ww, D, Hh, Ww)
    got = _run_sparse(comp, kd, ks, N)
    ref = _sparse_ref(comp.double(), kd, ks)
    assert torch.all(got[..., 110:] == 0), "pad channels 110 / 111 are not zero"
    assert torch.all(got[..., 0] == 0), "slot 0 carries no heat map"
    if kind == "equal":
        assert torch.all(got[..., 0:110:5] == 0), "kp_d == kp_s: every heat map must be exactly 0"
    if kind == "outside":
        assert torch.all(got[..., 8 * 5 + 1:8 * 5 + 5] == 0), "a slot sampled wholly outside the volume must be exactly 0"
        base = _run_sparse(comp, *_slot_deltas("synthetic", N, Ww, D, Hh, Ww), N)
        keep = [c for c in range(112) if not 40 <= c < 45]
        assert torch.equal(got[..., keep], base[..., keep]), "moving slot 8 changed other slots"
    # beyond the ulp: the fp32 exponentials (__expf; measured 6.8e-8) and the fp32 sampling points (ix rounded at 2^-24 x W times the step
    # between neighbouring comp values; measured 5.1e-6)
    heat_abs, def_abs = 2.7e-7, 2e-5
    ch_heat = list(range(0, 110, 5))
    ch_def = [c for c in range(110) if c % 5]
    _within_ulp(f"dm_sparse {shape} {kind} heat", got[..., ch_heat], ref[..., ch_heat], heat_abs)
    _within_ulp(f"dm_sparse {shape} {kind} deformed", got[..., ch_def], ref[..., ch_def], def_abs)
    worst = 0.0
    for k in range(22):
        for c in range(5 * k + (k == 0), 5 * k + 5):
            r = ref[..., c]
            if r.abs().max() > 0:
                worst = max(worst, _err(got[..., c], r))
            else:
                assert torch.all(got[..., c] == 0), (k, c)
    for name, sl in (("x0", (..., slice(0, 1), slice(None))), ("x-1", (..., slice(Ww - 1, Ww), slice(None))),
                     ("y0", (slice(None), slice(None), slice(0, 1))), ("y-1", (slice(None), slice(None), slice(Hh - 1, Hh))),
                     ("z0", (slice(None), slice(0, 1))), ("z-1", (slice(None), slice(D - 1, D)))):
        worst = max(worst, _err(got[sl], ref[sl]))
    # per channel and per border face: measured 4.7e-4 (fp16 storage)
    _gate(f"dm_sparse {shape} {kind} worst channel / border", worst, 1.8e-3)


@pytest.mark.parametrize("shared", ["comp", "kps", "both"])
def test_dm_sparse_shared_inputs_equal_copies(shared):
    N, D, Hh, Ww = 3, 8, 24, 40
    comp = _comp_input(1, D, Hh, Ww, 77)
    kd, ks = _kps(N, 4100)
    ks1 = ks[:1]
    sc, sk = shared in ("comp", "both"), shared in ("kps", "both")
    got = _run_sparse(comp if sc else comp.expand(N, -1, -1, -1, -1).contiguous(), kd, ks1 if sk else ks1.expand(N, -1, -1).contiguous(), N,
                      shared_comp=sc, shared_kps=sk)
    want = _run_sparse(comp.expand(N, -1, -1, -1, -1).contiguous(), kd, ks1.expand(N, -1, -1).contiguous(), N)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_dm_sparse_rejects_wide_rows():
    comp = torch.zeros(1, 2, 2, 65, 4, dtype=torch.float16, device="cuda")
    kd = torch.zeros(1, 21, 3, device="cuda")
    out = torch.zeros(1, 2, 2, 65, 120, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="64"):
        H.dm_sparse(comp, kd, kd, out, 1)


# ------------------------------------------------------------------------------------------------ dm_softmax_warp
def _logit_case(pattern, N, D, Hh, Ww, seed):
    """(P [N, D, H, W, 7, 22] float64 (kw, c) partials, bias [22], kp_d, kp_s)"""
    r = _rng(seed)
    kd, ks = _kps(N, 4200 + seed)
    P = torch.randn(N, D, Hh, Ww, 7, 22, generator=r, dtype=torch.float64) * 0.6
    bias = torch.randn(22, generator=r).float() * 0.3
    if pattern == "dominant":
        # slot (x + y) % 22 is 60 above the rest: the deformation is that slot's sparse motion; slots 5 / 9 / 13 leave the volume along x / y / z
        k = (torch.arange(Ww).view(1, 1, 1, Ww) + torch.arange(Hh).view(1, 1, Hh, 1)) % 22
        P[..., 3, :] += 60.0 * F.one_hot(k.expand(N, D, Hh, Ww), 22).double()
        ks = ks.clone()
        ks[:, 4] += torch.tensor([1.5, 0.0, 0.0]); ks[:, 8] += torch.tensor([0.0, -1.5, 0.0]); ks[:, 12] += torch.tensor([0.0, 0.0, 1.7])
    elif pattern == "equal":
        P.zero_()
        bias = torch.full((22,), 0.75)
    elif pattern == "negative":
        P = P * 0.2 - 400.0 / 7
    return P, bias, kd, ks


def _run_softmax_warp(part, bias, kd, ks, inp, N, D, Hh, Ww, shared_kps=False, shared_in=False):
    n = N * Hh * Ww * D * 32
    o32 = torch.full((n + 64,), float("nan"), device="cuda")
    o16 = torch.full((n + 64,), SENT16, dtype=torch.int16, device="cuda")
    de = torch.full((N * D * Hh * Ww * 3 + 64,), float("nan"), device="cuda")
    H.dm_softmax_warp(part.cuda(), bias.cuda(), kd.cuda().contiguous(), ks.cuda().contiguous(), inp.cuda(), N, D, Hh, Ww, shared_kps, shared_in,
                      o32[:n], o16[:n].view(torch.float16), de[:-64])
    assert torch.all(torch.isnan(o32[n:])) and torch.all(o16[n:] == SENT16) and torch.all(torch.isnan(de[-64:])), "wrote past an output"
    return (o32[:n].view(N, Hh, Ww, D, 32).cpu(), o16[:n].view(torch.float16).view(N, Hh, Ww, D, 32).cpu(),
            de[:-64].view(N, D, Hh, Ww, 3).cpu())


def _column_classes(Ww):
    cls = {f"x%4={m}": [x for x in range(Ww) if x % 4 == m] for m in range(4)}
    cls.update({f"x={x}": [x] for x in (0, 1, 2, Ww - 3, Ww - 2, Ww - 1)})
    return cls


@pytest.mark.parametrize("shape", [(1, 16, 64, 64), (2, 16, 24, 48), (1, 16, 3, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pattern", ["ordinary", "dominant", "equal", "negative"])
def test_dm_softmax_warp(shape, pattern):
    """compact-2 hand-over -> softmax -> deformation -> warp, per column class (x mod 4 and the three border columns on each side).
    (1, 16, 3, 16) is 3 workgroups: the block walk of a grid that is no multiple of 8 (the other shapes' grids are).  The stand-alone
    gather (grid_sample_kernel) fed the kernel's own deformation gives the fused kernel's bits: one function behind both."""
    N, D, Hh, Ww = shape
    P, bias, kd, ks = _logit_case(pattern, N, D, Hh, Ww, 10 + Ww)
    part = H.compact2(P).float()
    logits = H.compact2_logits(part.double(), bias.double())
    inp = (torch.randn(N, Hh, Ww, D, 32, generator=_rng(3)) * 0.5).float()
    o32, o16, de = _run_softmax_warp(part, bias, kd, ks, inp, N, D, Hh, Ww)
    dref = _deform_ref(logits, kd, ks)
    if pattern == "dominant":
        sp = _sparse_motions(kd, ks, D, Hh, Ww)
        k = (torch.arange(Ww).view(1, Ww) + torch.arange(Hh).view(Hh, 1)) % 22
        pick = sp.permute(0, 2, 3, 4, 1, 5).gather(4, k.view(1, 1, Hh, Ww, 1, 1).expand(N, D, -1, -1, 1, 3)).squeeze(4)
        assert (dref - pick).abs().max() < 1e-12
        assert (de.double().abs() > 1).any(), "no deformation left the volume"
    if pattern == "equal":
        assert (dref - _sparse_motions(kd, ks, D, Hh, Ww).mean(1)).abs().max() < 1e-12
    wref32 = _warp_ref(inp, de)                                              # the gather, driven by the kernel's own deformation
    errs = {}
    for name, xs in _column_classes(Ww).items():
        errs[name] = (_err(de[:, :, :, xs], dref[:, :, :, xs]), _err(o32[:, :, xs], wref32[:, :, xs]), _err(o16[:, :, xs], wref32[:, :, xs]))
    for i, what in enumerate(("deformation", "warp fp32", "warp fp16")):
        w = max(errs, key=lambda n: errs[n][i])
        # measured: deformation 1.1e-6 (all logits near -400), warp fp32 5.5e-6 (the fp32 sampling point), fp16 4.2e-4 (storage)
        _gate(f"dm_softmax_warp {shape} {pattern} {what} (worst class {w})", errs[w][i], (4e-6, 2e-5, 1.8e-3)[i])
    assert torch.equal(o16, o32.half())
    g32, g16 = H.grid_sample(inp.cuda(), de.cuda())
    assert torch.equal(g32.cpu(), o32) and torch.equal(g16.cpu(), o16)


@pytest.mark.parametrize("shared", ["in", "kps", "both"])
def test_dm_softmax_warp_shared_inputs_equal_copies(shared):
    N, D, Hh, Ww = 3, 16, 24, 48
    P, bias, kd, ks = _logit_case("ordinary", N, D, Hh, Ww, 5)
    part = H.compact2(P).float()
    inp = (torch.randn(1, Hh, Ww, D, 32, generator=_rng(4)) * 0.5).float()
    si, sk = shared in ("in", "both"), shared in ("kps", "both")
    ks1 = ks[:1]
    got = _run_softmax_warp(part, bias, kd, ks1 if sk else ks1.expand(N, -1, -1), inp if si else inp.expand(N, -1, -1, -1, -1).contiguous(),
                            N, D, Hh, Ww, shared_kps=sk, shared_in=si)
    want = _run_softmax_warp(part, bias, kd, ks1.expand(N, -1, -1), inp.expand(N, -1, -1, -1, -1).contiguous(), N, D, Hh, Ww)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ occ_finish
@pytest.mark.parametrize("taps", [49, 7])
@pytest.mark.parametrize("shape", [(1, 64, 64), (2, 24, 40)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sat", [False, True])
def test_occ_finish(taps, shape, sat):
    """sigmoid(bias + the shifted partials), zero padding: each of the four border bands apart; partials of +-40 saturate the sigmoid."""
    N, Hh, Ww = shape
    r = _rng(taps + Ww)
    part = torch.randn(N, Hh, Ww, 64 if taps == 49 else 16, generator=r) * (0.4 if taps == 49 else 1.0)
    if sat:
        part[:, : Hh // 3] = 40.0 / taps * 7
        part[:, -(Hh // 3):] = -40.0 / taps * 7
    occ = torch.full((N * Hh * Ww + 64,), float("nan"), device="cuda")
    H.occ_finish(part.cuda(), taps, 0.3, occ[:N * Hh * Ww].view(N, Hh, Ww))
    assert torch.all(torch.isnan(occ[N * Hh * Ww:]))
    got = occ[:N * Hh * Ww].view(N, Hh, Ww).cpu()
    ref = _occ_ref(part, taps, 0.3)
    bands = {"top": got[:, :3], "bottom": got[:, -3:], "left": got[:, :, :3], "right": got[:, :, -3:], "interior": got[:, 3:-3, 3:-3]}
    rb = {"top": ref[:, :3], "bottom": ref[:, -3:], "left": ref[:, :, :3], "right": ref[:, :, -3:], "interior": ref[:, 3:-3, 3:-3]}
    for k in bands:
        # max |d| measured <= 2.6e-7 (fp32 sums of 7 / 49 terms, __expf)
        _gate(f"occ_finish taps={taps} {shape} sat={sat} {k}", (bands[k].double() - rb[k]).abs().max().item(), 1e-6)
    if sat:
        assert got[:, 0].min() > 0.999 and got[:, -1].max() < 1e-3


# ------------------------------------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def engines(state_dicts):
    from canonswap_amd import pack
    from canonswap_amd.engine import Engine
    blobs = pack.build_blobs(state_dicts)
    es = {"batched": Engine(0, max_batch=3), "latency": Engine(0, max_batch=1, latency_mode=True)}
    for e in es.values():
        e.load_blobs(blobs)
    yield es
    for e in es.values():
        e.close()


def _read_all(e, B):
    return {w: H.dm_read(e, w, B).cpu() for w in [H.DM_COMP] + [H.DM_L0 + i for i in range(6)] + [H.DM_PRED, H.DM_LOGITS]}


@pytest.fixture(scope="module")
def engine_runs(engines):
    """Per mode: cs_warp_forward on B = 3 (batched) / 1 (latency) with the launch list recorded, the buffers it left, and cs_warp's output."""
    import tempfile
    out = {}
    for mode, e in engines.items():
        B = 3 if mode == "batched" else 1
        f = _features(B, 31)
        kd, ks = _kps(B, 4300)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "launches.csv")
            old = os.environ.get("CANONSWAP_PROFILE_CSV")
            os.environ["CANONSWAP_PROFILE_CSV"] = path
            try:
                e.profile_begin()
                fwd = e.warp_forward(f.cuda(), kd.cuda(), ks.cuda())
                e.profile_end()
            finally:
                if old is None:
                    del os.environ["CANONSWAP_PROFILE_CSV"]
                else:
                    os.environ["CANONSWAP_PROFILE_CSV"] = old
            labels = [l.split(",")[1] for l in open(path).read().splitlines()[1:]]
        bufs = _read_all(e, B)
        warped, occ2 = e.warp(f.cuda(), ks.cuda(), kd.cuda())
        out[mode] = dict(B=B, f=f, kd=kd, ks=ks, labels=labels, bufs=bufs, deform=fwd["deformation"].cpu(), occ=fwd["occlusion_map"].cpu(),
                         warped=warped.cpu(), occ2=occ2.cpu())
    return out


@pytest.mark.parametrize("mode", ["batched", "latency"])
def test_engine_launch_list(engine_runs, mode):
    """Pins the forms the layer test covers: grouped up-block phases, the 49-tap occlusion conv + finish (batched); the 7-tap W.occp conv and
    cross-workgroup split-K (latency)."""
    labels = engine_runs[mode]["labels"]
    print("\n" + mode + ": " + " ".join(labels))
    w = labels[labels.index("dm_compress"):labels.index("occ_finish") + 1]
    enc = [f"W.enc{i}" for i in range(5)]
    if mode == "batched":
        assert w == ["dm_compress", "dm_sparse"] + enc + [f"W.dec{i}.p" for i in range(5)] + ["W.tail", "W.maskp", "dm_softmax_warp", "W.occ49",
                                                                                               "occ_finish"], w
    else:
        sk = [w[j - 1] for j in range(1, len(w)) if w[j] == "splitk_finish"]
        assert sk == ["W.enc3", "W.enc4", "W.dec0", "W.dec1", "W.dec2", "W.occp"], sk
        assert [l for l in w if l != "splitk_finish"] == (["dm_compress", "dm_sparse"] + enc + ["W.dec0", "W.dec1", "W.dec2", "W.dec3.p", "W.dec4.p",
                                                          "W.tail", "W.maskp", "dm_softmax_warp", "W.occp", "occ_finish"]), w


def _conv3d(x, w, b, pad=1):
    """x [D, H, W, C] float64 -> [D, H, W, Co]"""
    y = F.conv3d(x.permute(3, 0, 1, 2).unsqueeze(0), w, b, padding=pad)
    return y[0].permute(1, 2, 3, 0)


def _upblock(x, w, b, phased):
    """UpBlock3d conv on x [D, S/2, S/2, C] (fp16 weights: w or its phase sums) + ReLU -> [D, S, S, Co]"""
    from canonswap_amd import pack
    from oracle import canonswap_ref as O
    xt = x.permute(3, 0, 1, 2).unsqueeze(0)
    if not phased:
        y = F.conv3d(O.nearest_up(xt, 1, 2, 2), _w16(w), _b32(b), padding=1)
    else:
        D, Si = x.shape[0], x.shape[1]
        y = torch.zeros(1, w.shape[0], D, 2 * Si, 2 * Si, dtype=torch.float64)
        for (a, bb), (ph, pw, wab) in pack.upsampled_conv3d_phases(w).items():
            y[:, :, :, a::2, bb::2] = F.conv3d(F.pad(xt, (pw, 1 - pw, ph, 1 - ph, 1, 1)), _w16(wab), _b32(b))
    return F.relu(y)[0].permute(1, 2, 3, 0)


# measured max |d| / max |ref| per layer on the MI355X (batched, latency); gate 4x
LAYER_MEASURED = {}


@pytest.mark.parametrize("mode", ["batched", "latency"])
def test_engine_layer_by_layer(engine_runs, wsd, sdd, mode):
    """Each layer of W's dense-motion network on the engine's own input to it (one sample: 1 of the B = 3 call, 0 of the latency call)."""
    from canonswap_amd import pack
    r = engine_runs[mode]
    s = 1 if mode == "batched" else 0
    bufs = {k: v[s].double() for k, v in r["bufs"].items()}
    kd, ks = r["kd"][s:s + 1], r["ks"][s:s + 1]
    errs = []
    # compress + sparse / heat
    errs.append(("compress", _err(bufs[H.DM_COMP], _compress_ref(r["f"][s:s + 1], sdd)[0])))
    l0 = bufs[H.DM_L0]
    sref = _sparse_ref(bufs[H.DM_COMP].unsqueeze(0), kd, ks)[0]
    errs.append(("sparse", _err(l0[..., 32:144], sref)))
    assert torch.all(l0[..., 142:144] == 0), "pad channels 142 / 143 of level 0"
    p = "dense_motion_network.hourglass"
    for i in range(5):
        w, b = _folded(wsd, f"{p}.encoder.down_blocks.{i}")
        x = bufs[H.DM_L0 + i][..., SKIP[i]:SKIP[i] + (110 if i == 0 else CIN[i])]
        y = F.relu(_conv3d(x, _w16(w), _b32(b)))
        y = F.avg_pool3d(y.permute(3, 0, 1, 2).unsqueeze(0), (1, 2, 2))[0].permute(1, 2, 3, 0)
        errs.append((f"enc{i}", _err(bufs[H.DM_L0 + i + 1][..., SKIP[i + 1]:SKIP[i + 1] + COUT[i]], y)))
    for i in range(5):
        lv = 5 - i
        w, b = _folded(wsd, f"{p}.decoder.up_blocks.{i}")
        x = bufs[H.DM_L0 + lv][..., :w.shape[1]]
        phased = mode == "batched" or i >= 3
        y = _upblock(x, w, b, phased)
        errs.append((f"dec{i}{'.p' if phased else ''}", _err(bufs[H.DM_L0 + lv - 1][..., :DEC_OUT[i]], y)))
    w, b = _folded(wsd, "dense_motion_network.hourglass.decoder")
    pred = F.relu(_conv3d(l0[..., :142], _w16(w), _b32(b)))
    got_pred = bufs[H.DM_PRED]
    assert torch.all(got_pred[..., 142:144] == 0), "pad channels 142 / 143 of dm_pred"
    errs.append(("tail", _err(got_pred[..., :142], pred)))
    # mask conv on the engine's pred: the compact-2 partials sum to the float64 logits, the softmax gives the deformation
    xp = got_pred[..., :142]
    logits = _conv3d(xp, _w16(sdd["dense_motion_network.mask.weight"].numpy()), _b32(sdd["dense_motion_network.mask.bias"].numpy()), pad=3)
    lg = H.compact2_logits(bufs[H.DM_LOGITS].unsqueeze(0), _b32(sdd["dense_motion_network.mask.bias"].numpy()))[0]
    errs.append(("mask logits", _err(lg, logits)))
    dref = _deform_ref(logits.unsqueeze(0), kd, ks)[0]
    errs.append(("deformation", _err(r["deform"][s], dref)))
    # occlusion on the engine's pred
    wo = _w16(sdd["dense_motion_network.occlusion.weight"].numpy())
    xo = xp.permute(3, 0, 1, 2).reshape(1, 142 * 16, 64, 64)
    occ = torch.sigmoid(F.conv2d(xo, wo, _b32(sdd["dense_motion_network.occlusion.bias"].numpy()), padding=3))
    errs.append(("occlusion", _err(r["occ"][s], occ[0])))
    assert torch.equal(r["occ"], r["occ2"])
    # the warp: cs_warp's output against float64 grid_sample driven by the engine's deformation
    wref = _warp_ref(r["f"][s:s + 1].permute(0, 3, 4, 2, 1), r["deform"][s:s + 1])[0]      # HWDC
    errs.append(("warp", _err(r["warped"][s].permute(2, 3, 1, 0), wref)))
    print(f"\nW layer by layer, {mode} (max |d| / max |ref|):")
    for k, v in errs:
        print(f"  {k:12s} {v:.3e}")
    # measured (batched / latency): compress 2.7e-4 / 3.0e-4, sparse 3.4e-4 / 3.2e-4, hourglass convs 2.6e-4 - 4.4e-4 (fp16 storage), mask
    # logits 7.5e-7 / 9.1e-7, deformation 4.2e-7 / 3.8e-7, occlusion 1.7e-7 / 1.5e-7, warp 3.5e-6 / 4.7e-6
    gates = {"compress": 1.2e-3, "sparse": 1.4e-3, "mask logits": 3.6e-6, "deformation": 1.7e-6, "occlusion": 7e-7, "warp": 1.9e-5}
    for k, v in errs:
        g = gates.get(k, 1.8e-3)
        assert v <= g, (k, v, g)


def test_engine_batch_independence(engines, engine_runs):
    """Sample i of the batched B = 3 call equals the same sample run at B = 1, bit for bit, in every buffer cs_op_dm_read returns."""
    e, r = engines["batched"], engine_runs["batched"]
    for i in range(3):
        e.warp_forward(r["f"][i:i + 1].cuda(), r["kd"][i:i + 1].cuda(), r["ks"][i:i + 1].cuda())
        one = _read_all(e, 1)
        for w, v in one.items():
            assert torch.equal(v[0].view(torch.int16) if v.dtype == torch.float16 else v[0],
                               r["bufs"][w][i].view(torch.int16) if v.dtype == torch.float16 else r["bufs"][w][i]), (i, w)


def test_animate_frames_mixed_sharing(engines, sdd):
    """cs_animate_frames at B = 3 with nf = 1, ns = 3 and with nf = 3, ns = 1: each equals the call with expanded copies, bit for bit; the
    shared-volume call's level-0 buffer against the float64 sparse-motion reference."""
    e = engines["batched"]
    f = _features(1, 32)
    kd, ks = _kps(3, 4400)
    f3 = f.expand(3, -1, -1, -1, -1).contiguous()
    ks1 = ks[:1]
    ks3 = ks1.expand(3, -1, -1).contiguous()
    a = e.animate_frames(f.cuda(), ks.cuda(), kd.cuda())["out"].cpu()           # nf = 1, ns = 3
    l0 = H.dm_read(e, H.DM_L0, 3).cpu().double()
    comp0 = H.dm_read(e, H.DM_COMP, 1).cpu().double()
    a3 = e.animate_frames(f3.cuda(), ks.cuda(), kd.cuda())["out"].cpu()
    assert torch.equal(a, a3)
    sref = _sparse_ref(comp0.expand(3, -1, -1, -1, -1), kd, ks)
    _gate("v2i shared volume: level-0 sparse channels", _err(l0[..., 32:144], sref), 1.3e-3)      # measured 3.2e-4
    b = e.animate_frames(f3.cuda(), ks1.cuda(), kd.cuda())["out"].cpu()         # nf = 3, ns = 1
    b3 = e.animate_frames(f3.cuda(), ks3.cuda(), kd.cuda())["out"].cpu()
    assert torch.equal(b, b3)
