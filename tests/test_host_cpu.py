"""CPU-side checks: weight packer, C-ABI surface, host helpers (no GPU compute)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from canonswap_amd import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_conv_roundtrip_and_kstep_order():
    r = np.random.Generator(np.random.PCG64(3))
    w = r.standard_normal((22, 142, 7, 7, 7)).astype(np.float32)
    p = pack.pack_conv(w, 32)
    assert p.shape == (5 * 343, 32, 32) and p.dtype == np.float16
    assert np.array_equal(pack.unpack_conv(p, 22, 142, 7, 7, 7), w.astype(np.float16).astype(np.float32))
    # kstep = ((chunk*KD+kd)*KH+kh)*KW+kw, in-channel = chunk*32 + kk
    chunk, kd, kh, kw, row, kk = 3, 2, 5, 1, 7, 9
    assert p[((chunk * 7 + kd) * 7 + kh) * 7 + kw, row, kk] == np.float16(w[row, chunk * 32 + kk, kd, kh, kw])
    assert np.all(p[:, 22:, :] == 0) and np.all(p[4 * 343:, :, 14:] == 0)      # padded rows / channels are zero


def test_interleave16():
    a = np.arange(32)[:, None] * np.ones((1, 3)); b = -a
    z = pack.interleave16(a, b)
    assert z.shape == (64, 3)
    assert np.array_equal(z[:16], a[:16]) and np.array_equal(z[16:32], b[:16]) and np.array_equal(z[32:48], a[16:])


def test_bn_and_spectral_folding_match_oracle(state_dicts_np, state_dicts):
    from oracle import canonswap_ref as O
    sd, sdt = state_dicts_np["appearance_feature_extractor"], state_dicts["appearance_feature_extractor"]
    s, t = pack.bn_affine(sd, "down_blocks.0.norm")
    w, b = pack.fold_conv_bn(sd["down_blocks.0.conv.weight"], sd["down_blocks.0.conv.bias"], s, t)
    x = torch.randn(1, 64, 8, 8)
    ref = O.bn_eval(O.conv(x, sdt, "down_blocks.0.conv", 1), sdt, "down_blocks.0.norm")
    got = F.conv2d(x, torch.from_numpy(w).float(), torch.from_numpy(b).float(), padding=1)
    assert (ref - got).abs().max() < 1e-4
    g, gt = state_dicts_np["spade_generator"], state_dicts["spade_generator"]
    assert np.abs(pack.spectral_weight(g, "up_1.conv_1") - O.spectral_weight(gt, "up_1.conv_1").numpy()).max() < 1e-5


def test_view_permutation_is_the_reference_view():
    """Memory channel jm = d*32 + c of the [H][W][D][C] volume is reference channel c*16 + d of view(bs, c*d, h, w)."""
    v = torch.arange(32 * 16).view(32, 16)                       # value = reference flat channel index c*16+d
    mem = v.t().reshape(-1)                                      # [d][c] order
    assert np.array_equal(mem.numpy(), pack.MEM2REF)


def test_build_blobs_names_and_sizes(state_dicts_np):
    blobs = pack.build_blobs(state_dicts_np)
    assert blobs["T.b6.c2.w"].shape == (144, 1024, 32) and blobs["T.b0.c1.raw"].shape == (512, 9, 512)
    assert blobs["W.maskp.w"].shape == (5 * 49, 160, 32) and blobs["W.occp.w"].shape == (80 * 7, 32, 32) and blobs["W.occ49.w"].shape == (80, 64, 32)
    assert blobs["G.shared64.w"].shape == (72, 1536, 32) and blobs["G.up1.n1.w"].shape == (36, 128, 32)
    assert all(b.flags["C_CONTIGUOUS"] for b in blobs.values())
    # every blob the engine asks for by literal name exists (names built with snprintf are covered on the GPU)
    src = open(os.path.join(ROOT, "canonswap_amd", "csrc", "engine.hip")).read()
    for name in re.findall(r'"((?:F|W|T|R|G)\.[A-Za-z0-9_.]+\.(?:w|b))"', src):
        assert name in blobs, name


def test_isa_check_of_the_hand_counted_weight_rings():
    """The objects the shipped library was linked from (canonswap_amd/build/): every untracked ring load is covered by a counted wait that
    is deep enough for it before an MFMA reads it (the check marks a register waited only when its load is older than the
    N youngest VMEM ops of `s_waitcnt vmcnt(N)`)."""
    from canonswap_amd import _build, _isa
    if not os.path.isdir(_build.OBJ_DIR) or not os.path.exists(os.path.join(_build.OBJ_DIR, "conv_wide.o")):
        pytest.skip("no object files next to the library (prebuilt .so only)")
    seen = _isa.isa_check()
    assert len(seen) >= 70 and any("conv_wide_kernel" in k for k in seen)


def test_isa_check_rejects_a_wait_that_is_too_shallow(tmp_path, monkeypatch):
    """A counted wait whose immediate leaves the consumed load among the outstanding ones must fail the check."""
    from canonswap_amd import _isa
    asm = """0000000000001000 <conv_wide_kernel_fake>:
	global_load_dwordx4 v[10:13], v[0:1], off
	global_load_dwordx4 v[14:17], v[0:1], off
	s_waitcnt vmcnt(%d)
	v_mfma_f32_16x16x32_f16 a[0:3], v[10:13], v[20:23], a[0:3]
	v_mfma_f32_16x16x32_f16 a[0:3], v[14:17], v[20:23], a[0:3]
	s_endpgm
"""
    import subprocess as sp

    def fake_run_factory(n):
        def fake_run(cmd, **kw):
            class R:
                stdout = asm % n
            return R()
        return fake_run

    (tmp_path / "fake.o").write_bytes(b"")
    monkeypatch.setattr(_isa.subprocess, "run", fake_run_factory(0))
    assert _isa._isa_check_ring(str(tmp_path), "objdump", "fake.o", r"conv_wide_kernel_fake", 2) == {"conv_wide_kernel_fake": 2}
    monkeypatch.setattr(_isa.subprocess, "run", fake_run_factory(1))       # vmcnt(1): the second load may still be in flight
    with pytest.raises(RuntimeError, match="no vmcnt wait"):
        _isa._isa_check_ring(str(tmp_path), "objdump", "fake.o", r"conv_wide_kernel_fake", 2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_engine_fails_loudly_without_gpu():
    from canonswap_amd.engine import Engine
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine(0)


def test_keypoint_helpers_match_golden(golden):
    from canonswap_amd.can_swap_e2e import get_rotation_matrix, headpose_pred_to_degree
    g = golden("unit_vectors.npz")
    pyr = torch.from_numpy(g["pyr"])
    assert np.abs(get_rotation_matrix(pyr[:, 0], pyr[:, 1], pyr[:, 2]).numpy() - g["rot"]).max() < 1e-6
    assert np.abs(headpose_pred_to_degree(torch.from_numpy(g["bins"])).numpy() - g["deg"]).max() < 1e-4


def test_landmark_ratios_match_reference_vectors(golden):
    """calc_ratio's helpers (can_swap_e2e.py:324-348) against values computed by the reference's retargeting_utils."""
    from canonswap_amd import can_swap_e2e as H
    g = golden("unit_vectors.npz")
    assert np.allclose(H.eye_close_ratio(g["lmk"]), g["eye_ratio"], rtol=0, atol=1e-6)
    assert np.allclose(H.lip_close_ratio(g["lmk"]), g["lip_ratio"], rtol=0, atol=1e-6)
    assert H.eye_close_ratio(g["lmk"][:1]).shape == (1, 2) and H.lip_close_ratio(g["lmk"][:1]).shape == (1, 1)


@pytest.mark.parametrize("s", [2, 4])
def test_upsampled_conv_phase_decomposition(s):
    """pack.upsampled_conv_phases: a 3x3 conv on a nearest-up-sampled map == per-row-phase convs on the source grid."""
    r = np.random.Generator(np.random.PCG64(s))
    w, x = r.standard_normal((5, 3, 3, 3)), r.standard_normal((2, 3, 8, 8))
    ref = F.conv2d(F.interpolate(torch.from_numpy(x), scale_factor=s, mode="nearest"), torch.from_numpy(w), padding=1).numpy()
    out = np.zeros_like(ref)
    phases = pack.upsampled_conv_phases(w, s)
    assert len(phases) == (4 if s == 2 else 12)
    for a, b0, nb, kh, ph, kw, pw, wg in phases:
        assert wg.shape == (nb * 5, 3, kh, kw)
        y = F.conv2d(F.pad(torch.from_numpy(x), (pw, kw - 1 - pw, ph, kh - 1 - ph)), torch.from_numpy(wg)).numpy()
        for k in range(nb):
            out[:, :, a::s, b0 + k::s] = y[:, k * 5:(k + 1) * 5]
    assert np.abs(out - ref).max() < 1e-12
    if s == 4:      # what run_G's de-duplication rests on: rows 4i+1 / 4i+2 and the two middle columns carry the same weights, bit for bit
        by = {(a, b0): wg for a, b0, nb, kh, ph, kw, pw, wg in phases}
        for b0 in (0, 1, 3):
            assert np.array_equal(by[(1, b0)], by[(2, b0)])
        for a in range(4):
            assert np.array_equal(by[(a, 1)][:5], by[(a, 1)][5:])


def test_upsampled_conv3d_phase_decomposition():
    """pack.upsampled_conv3d_phases: 3x3x3 conv after a nearest (1,2,2) up-sampling == four 3x2x2 convs on the source grid."""
    r = np.random.Generator(np.random.PCG64(9))
    w, x = r.standard_normal((5, 3, 3, 3, 3)), r.standard_normal((1, 3, 4, 6, 6))
    ref = F.conv3d(F.interpolate(torch.from_numpy(x), scale_factor=(1, 2, 2), mode="nearest"), torch.from_numpy(w), padding=1).numpy()
    out = np.zeros_like(ref)
    for (a, b), (ph, pw, wab) in pack.upsampled_conv3d_phases(w).items():
        assert (ph, pw) == (int(a == 0), int(b == 0)) and wab.shape == (5, 3, 3, 2, 2)
        xp = F.pad(torch.from_numpy(x), (pw, 1 - pw, ph, 1 - ph, 1, 1))
        out[:, :, :, a::2, b::2] = F.conv3d(xp, torch.from_numpy(wab)).numpy()
    assert np.abs(out - ref).max() < 1e-12


@pytest.fixture(scope="module")
def w_blobs():
    """pack._pack_W's blobs of the synthetic warping module and its state dict (numpy)"""
    from canonswap_amd import synth
    sd = synth.make_state_dicts(0, modules=("warping_module",))["warping_module"]
    out = {}
    pack._pack_W(out, pack._np_sd(sd))
    return out, pack._np_sd(sd)


def _f16(w):
    return torch.from_numpy(np.asarray(w, np.float64).astype(np.float16).astype(np.float64))


def test_mask_conv_kw_split_decomposition(w_blobs):
    """W.maskp, the (7,7,1)-tap conv with (kw, c) output channels, shifted by kw - 3 along W and summed over kw == the 7x7x7 mask conv."""
    out, sd = w_blobs
    w = _f16(sd["dense_motion_network.mask.weight"])                                          # [22][142][7][7][7]
    wp = torch.from_numpy(pack.unpack_conv(out["W.maskp.w"], 154, 142, 7, 7, 1).astype(np.float64))
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).standard_normal((1, 142, 5, 6, 9)))
    ref = F.conv3d(x, w, padding=3)
    part = F.conv3d(x, wp, padding=(3, 3, 0)).view(1, 7, 22, 5, 6, 9)                        # [.., kw, c, d, h, xin]
    got = torch.zeros_like(ref)
    for kw in range(7):
        lo, hi = max(0, 3 - kw), min(9, 12 - kw)                                              # output x takes input x + kw - 3
        got[..., lo:hi] += part[:, kw, :, :, :, lo + kw - 3:hi + kw - 3]
    assert (got - ref).abs().max() < 1e-10 * ref.abs().max()


def test_compact2_regrouping_sums_back_to_the_logits():
    """tests/hip_ops.compact2 (the ST == 9 kw_out epilogue's layout) and compact2_logits == bias + sum_kw P[x + kw - 3][kw], zero padding."""
    import hip_ops
    r = np.random.Generator(np.random.PCG64(4))
    for Wd in (4, 8, 24):
        P = torch.from_numpy(r.standard_normal((2, 3, 5, Wd, 7, 22)))
        bias = torch.from_numpy(r.standard_normal(22))
        part = hip_ops.compact2(P)
        assert part.shape == (2, 3, 5, Wd // 4, 10, 22)
        ref = bias.expand(2, 3, 5, Wd, 22).clone()
        for x in range(Wd):
            for kw in range(7):
                if 0 <= x + kw - 3 < Wd:
                    ref[:, :, :, x] += P[:, :, :, x + kw - 3, kw]
        assert (hip_ops.compact2_logits(part, bias) - ref).abs().max() < 1e-12


def test_occlusion_conv_decompositions(w_blobs):
    """W.occ49 (a 1x1 conv with the 49 taps as output channels, shifted and summed) and W.occp (7 vertical taps, the 7 horizontal taps as
    output channels) == the 7x7 occlusion conv over the (c * 16 + d)-flattened prediction; input channel d * 160 + c of the grouped form."""
    out, sd = w_blobs
    w = _f16(sd["dense_motion_network.occlusion.weight"])                                     # [1][2272][7][7]
    Hh, Ww = 9, 11
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((1, 142, 16, Hh, Ww)))
    ref = F.conv2d(x.reshape(1, 2272, Hh, Ww), w, padding=3)[0, 0]
    xg = torch.zeros(1, 16, 160, Hh, Ww, dtype=torch.float64)
    xg[:, :, :142] = x.permute(0, 2, 1, 3, 4)
    xg = xg.reshape(1, 2560, Hh, Ww)
    w49 = torch.from_numpy(pack.unpack_conv(out["W.occ49.w"], 49, 2560, 1, 1, 1).astype(np.float64)).view(49, 2560, 1, 1)
    p49 = F.pad(F.conv2d(xg, w49)[0], (3, 3, 3, 3))                                            # [49][H + 6][W + 6]
    got49 = sum(p49[ky * 7 + kx, ky:ky + Hh, kx:kx + Ww] for ky in range(7) for kx in range(7))
    w7 = torch.from_numpy(pack.unpack_conv(out["W.occp.w"], 7, 2560, 1, 7, 1).astype(np.float64)).view(7, 2560, 7, 1)
    p7 = F.pad(F.conv2d(xg, w7, padding=(3, 0))[0], (3, 3))                                    # [7][H][W + 6]
    got7 = sum(p7[kx, :, kx:kx + Ww] for kx in range(7))
    for got in (got49, got7):
        assert (got - ref).abs().max() < 1e-10 * ref.abs().max()


def test_getid_arithmetic_with_injected_network():
    """can_swap_e2e.py:102-107: nearest resize to 112x112 -> identity network -> L2 normalisation; the network is injected."""
    from canonswap_amd.can_swap_e2e import can_swapper

    class Net(torch.nn.Module):
        def forward(self, x):
            assert x.shape[-2:] == (112, 112)
            return x.mean(dim=(2, 3)).repeat(1, 171)[:, :512] + 0.25, None      # (id, aux) like the reference's ArcFace module

    host = type("H", (), {"netArc": Net()})()
    img = torch.rand(2, 3, 160, 160)
    got = can_swapper.getid(host, img)
    want, _ = Net()(F.interpolate(img, size=(112, 112)))
    want = F.normalize(want, p=2, dim=1)
    assert got.shape == (2, 512) and torch.allclose(got, want) and torch.allclose(got.norm(dim=1), torch.ones(2))
    host.netArc = None
    with pytest.raises(RuntimeError, match="identity network"):
        can_swapper.getid(host, img)


def test_unpack_conv_deinterleaves_the_fused_t_rows():
    """unpack_conv(pack_conv(interleave16(a, b))) gives a and b back at rows ((o / 16) * 2 + kind) * 16 + o % 16: the row formula of
    t_modulate_kernel (csrc/kernels.hip) for the fused [W ; w_mod] set"""
    r = np.random.Generator(np.random.PCG64(31))
    a = r.standard_normal((64, 96, 3, 3)).astype(np.float16).astype(np.float32)
    b = r.standard_normal((64, 96, 3, 3)).astype(np.float16).astype(np.float32)
    p = pack.pack_conv(pack.interleave16(a, b), 128)
    assert p.shape == (3 * 9, 128, 32)
    u = pack.unpack_conv(p, 128, 96, 1, 3, 3)[:, :, 0]
    o = np.arange(64)
    assert np.array_equal(u[((o // 16) * 2) * 16 + o % 16], a) and np.array_equal(u[((o // 16) * 2 + 1) * 16 + o % 16], b)
    v = u.reshape(4, 2, 16, 96, 3, 3)
    assert np.array_equal(v[:, 0].reshape(64, 96, 3, 3), a) and np.array_equal(v[:, 1].reshape(64, 96, 3, 3), b)


def t_precompute_f32(fc, raw, idv):
    """fp32 numpy restatement of t_style_kernel + t_modulate_kernel on pack._pack_T's ".fc" / ".raw" blobs -> (style [512], w_mod [512, 9, 512])"""
    f = np.float32
    n = 512 * 512
    w1, b1, w2, b2 = fc[:n].reshape(512, 512), fc[n:n + 512], fc[n + 512:2 * n + 512].reshape(512, 512), fc[2 * n + 512:]
    h = w1 @ idv.astype(f) + b1
    h = np.where(h > 0, h, f(0.2) * h).astype(f)
    style = (w2 @ h + b2).astype(f)
    m = raw * style[None, None, :]
    ss = (m * m).reshape(512, -1).sum(1, dtype=f)
    return style, m * (f(1) / np.sqrt(ss + f(1e-8)))[:, None, None]


@pytest.mark.parametrize("layer", ["T.b0.c1", "T.b0.c2", "T.b3.c2", "T.b6.c1", "T.b6.c2"])
def test_t_blobs_restated_in_fp32_match_the_oracles_modulated_weight(state_dicts_np, state_dicts, layer):
    """The ".fc" blob is [W1][b1][W2][b2] with fc.2 (rows and bias) in memory channel order and fc.0 untouched, ".raw" is [o][tap][i] in memory
    order: an fp32 restatement of the two kernels on them lands within one fp16 ulp of the oracle's float64 modulated_weight, its style within
    1e-6 of the oracle's style (|style| is O(1))."""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    blobs = {}
    pack._pack_T(blobs, state_dicts_np["transfer"])
    sdd = {k: v.double() for k, v in state_dicts["transfer"].items()}
    idv = synth.make_identity(7)
    p = "BottleNeck_2d.%s.conv%s" % (layer[3], layer[6])
    style, wm = t_precompute_f32(blobs[layer + ".fc"], blobs[layer + ".raw"], idv[0])
    lat = torch.from_numpy(idv).double()
    ref_s = O.style_vector(sdd, p, lat)[0].numpy()[pack.MEM2REF]
    assert np.abs(style - ref_s).max() < 1e-6
    assert np.abs(style - O.style_vector(sdd, p, lat)[0].numpy()).max() > 1e-2      # (the permutation is not the identity on this vector)
    ref = O.modulated_weight(sdd, p, lat)[0].numpy()[pack.MEM2REF][:, pack.MEM2REF].transpose(0, 2, 3, 1).reshape(512, 9, 512)
    ulp = np.abs(np.spacing(np.abs(ref).astype(np.float16))).astype(np.float64)
    err = np.abs(wm.astype(np.float16).astype(np.float64) - ref) / ulp
    print(f"\n{layer}: max error {err.max():.3f} fp16 ulp, style {np.abs(style - ref_s).max():.2e}")
    assert err.max() <= 1.0


def test_isa_check_rejects_a_spilled_dynamic_ring(monkeypatch):
    """The ring of a dynamic-shape conv_halo kernel (ST = 0) on made-up disassembly, two fragments per slot: accepted as the kernels have it;
    refused when two fragments share registers, and when a fragment of a slot is no MFMA's weight operand (the MFMA reads a copy instead)."""
    from canonswap_amd import _isa
    name = "_Z16conv_halo_kernelILi32ELi8ELi2ELi1ELi4ELi0ELb0ELb0ELi0EEv10ConvParams"

    def text(regs, operand=lambda r: r):
        lines = ["\tglobal_load_dwordx4 v[%d:%d], v[60:61], off" % (r, r + 3) for r in regs]
        for k in range(4):
            slot = regs[2 * k:2 * k + 2]
            lines.append("\ts_waitcnt vmcnt(6)")
            lines += ["\tv_mfma_f32_16x16x32_f16 v[100:103], v[%d:%d], v[50:53], v[100:103]" % (operand(r), operand(r) + 3) for r in slot]
            lines += ["\tglobal_load_dwordx4 v[%d:%d], v[60:61], off" % (r, r + 3) for r in slot]
        lines += ["\tv_mfma_f32_16x16x32_f16 v[100:103], v[0:3], v[50:53], v[100:103]", "\ts_waitcnt vmcnt(0)", "\ts_endpgm"]
        return "0000000000001000 <%s>:\n%s\n" % (name, "\n".join(lines))

    monkeypatch.setattr(_isa, "_isa_check_wide", lambda *a: {})
    monkeypatch.setattr(_isa, "_isa_check_lat", lambda *a: {})
    monkeypatch.setattr(_isa.os.path, "exists", lambda p: True)
    good = list(range(0, 32, 4))

    def run(txt):
        monkeypatch.setattr(_isa, "_disassemble", lambda d, o, oname: txt if oname == "conv_halo_g0.o" else "")
        return _isa.isa_check("nowhere")

    assert run(text(good)) == {name: 4}
    with pytest.raises(RuntimeError, match="overlap"):
        run(text([0, 4, 8, 12, 16, 20, 26, 24]))
    with pytest.raises(RuntimeError, match="no MFMA takes v\\[28:31\\]"):
        run(text(good, operand=lambda r: 24 if r == 28 else r))
