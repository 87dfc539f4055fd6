"""Single-frame latency mode (BASELINE configs[1]): forms that only pay when a launch cannot fill the chip and that add an output
element's products in another order than the batched path - conv_lat (the K loop of the 512-channel 3x3 convs split over twelve waves of a workgroup),
cross-workgroup split-K for the deep hourglass levels, 2-row statistics blocks in R's volume convs.  Same tolerance as the batched path (PSNR >= 50 dB
vs the oracle), deterministic, and close to - not bit-identical with - the batched path, which is why it is a mode."""
import numpy as np
import pytest
import torch

from chain_helpers import swapper_with_env

pytestmark = pytest.mark.gpu


def test_latency_mode_frame(state_dicts):
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    from oracle import canonswap_ref as O
    inp = synth.make_frame_inputs(1, seed=1000, size=256)
    args = [torch.from_numpy(inp[k]) for k in ("img", "x_t", "x_can")]
    idv = torch.from_numpy(synth.make_identity(7))
    with torch.no_grad():
        ref = O.swap_frame(state_dicts, *args, idv)
    lat = can_swapper(None, state_dicts=state_dicts, max_batch=1, latency_mode=True)
    std = can_swapper(None, state_dicts=state_dicts, max_batch=1)
    try:
        g = [a.cuda() for a in args]
        a1 = lat.swap_frames(*g, idv.cuda(), want_u8=True)
        a2 = lat.swap_frames(*g, idv.cuda(), want_u8=True)
        b = std.swap_frames(*g, idv.cuda(), want_u8=True)
        assert torch.equal(a1["out"], a2["out"])                                  # deterministic (fixed split order)
        p = O.psnr(a1["out"].cpu(), ref["out"])
        assert p >= 50.0, p
        assert O.psnr(a1["out"].cpu(), b["out"].cpu()) > 60.0                     # the two modes agree far inside the tolerance
        wd_l = lat.warp_decode(ref["f_ref"].cuda(), args[2].cuda(), args[1].cuda())
        wd_s = std.warp_decode(ref["f_ref"].cuda(), args[2].cuda(), args[1].cuda())
        for k in ("deformation", "occlusion_map"):                               # the split layers sit in the dense-motion hourglass
            d = float((wd_l[k] - wd_s[k]).abs().max())
            assert d < 2e-3, (k, d)
        assert float((wd_l["deformation"] - ref["deformation"].cuda()).norm() / ref["deformation"].norm()) < 2e-3
    finally:
        lat.engine.close(); std.engine.close()


def _phase_group_inputs(state_dicts, B):
    """(f_ref repeated B times, x_can, x_t): what test_grouped_phase_launch_equals_four_launches puts through warp_decode"""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    inp = synth.make_frame_inputs(B, seed=1234, size=256)
    args = [torch.from_numpy(inp[k]) for k in ("img", "x_t", "x_can")]
    idv = torch.from_numpy(synth.make_identity(7))
    with torch.no_grad():
        ref = O.swap_frame(state_dicts, *[a[:1] for a in args], idv)
    return ref["f_ref"].repeat(B, 1, 1, 1, 1), args[2], args[1]


def _warp_decode(sw, f_ref, x_can, x_t):
    wd = sw.warp_decode(f_ref.cuda(), x_can.cuda(), x_t.cuda())
    return {k: wd[k].cpu() for k in ("deformation", "occlusion_map", "out")}


@pytest.mark.parametrize("B,lat", [(2, False), (1, True)])
def test_grouped_phase_launch_equals_four_launches(state_dicts, B, lat, monkeypatch):
    """The four output phases of the hourglass' two last up-sampling convs (util.py:142-147 on the source grid) run as ONE conv_halo launch
    (ConvParams::nphase, blockIdx.z = phase: weights, leading padding and output offset per phase); an engine created under
    CANONSWAP_PHASE_GROUP=0 launches them one by one - in latency mode as split-K convs with their finishing launches.  Batched path: the
    same bits.  Latency mode: the grouped launch runs the whole K loop in one workgroup where the four launches split it: agreement to 2e-3 on the
    deformation / occlusion map and beyond 60 dB on the image, as between the two modes."""
    from oracle import canonswap_ref as O
    wd_in = _phase_group_inputs(state_dicts, B)
    with swapper_with_env(monkeypatch, state_dicts, {}, max_batch=B, latency_mode=lat) as sw:
        got = _warp_decode(sw, *wd_in)
    with swapper_with_env(monkeypatch, state_dicts, {"CANONSWAP_PHASE_GROUP": "0"}, max_batch=B, latency_mode=lat) as off:
        want = _warp_decode(off, *wd_in)
    for k in got:
        if lat and k == "out":
            assert O.psnr(got[k], want[k]) > 60.0
        elif lat:
            assert float((got[k] - want[k]).abs().max()) < 2e-3, k
        else:
            assert torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def test_switches_belong_to_the_engine(state_dicts, monkeypatch):
    """A switch is a property of the engine that was created under it (cs_create reads them, csrc/knobs.h), not of the process or of whichever
    launch comes first: A default, B created under CANONSWAP_PHASE_GROUP=0 - the environment is back before any launch -, C default and created
    after B.  A, B, A again, C through warp_decode: the same bits four times (the forms agree bit for bit in the batched path, test above); B
    launches more convs (four per grouped hourglass level, one per mlp_shared phase), A both times and C the same number."""
    wd_in = _phase_group_inputs(state_dicts, 2)

    def profiled(sw):
        sw.engine.profile_begin()
        out = _warp_decode(sw, *wd_in)
        return out, sw.engine.profile_end()["conv_launches"]

    with swapper_with_env(monkeypatch, state_dicts, {}, max_batch=2) as a, \
            swapper_with_env(monkeypatch, state_dicts, {"CANONSWAP_PHASE_GROUP": "0"}, max_batch=2) as b, \
            swapper_with_env(monkeypatch, state_dicts, {}, max_batch=2) as c:
        runs = [profiled(sw) for sw in (a, b, a, c)]
    for out, _ in runs[1:]:
        for k in out:
            assert torch.equal(out[k], runs[0][0][k]), k
    n_a, n_b, n_a2, n_c = (n for _, n in runs)
    assert n_b > n_a, (n_a, n_b)
    assert n_a == n_a2 == n_c, (n_a, n_a2, n_c)


@pytest.fixture(scope="module")
def pool_modes(state_dicts):
    """One engine per mode, one frame per call, and the bench's pool inputs (seed 1000, identity 7)."""
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    inp = synth.make_frame_inputs(256, seed=1000, size=256)
    idv = torch.from_numpy(synth.make_identity(7))
    lat = can_swapper(None, state_dicts=state_dicts, max_batch=1, latency_mode=True)
    std = can_swapper(None, state_dicts=state_dicts, max_batch=1)
    yield inp, idv, lat, std
    lat.engine.close(); std.engine.close()


# 63, 255, 134, 163 and 3 are the five worst of the 256 pool frames in the default mode (profiles/psnr_worst_frame.json: 53.01 / 53.41 / 53.42 / 53.73 /
# 54.44 dB); VERDICT r5 "what's weak" 4: the latency mode re-orders every 512-channel K loop and R's statistics blocks and was held to the oracle on
# the easiest kind of frame only
@pytest.mark.parametrize("frame", [3, 63, 134, 255])
def test_latency_mode_worst_pool_frames(state_dicts, pool_modes, frame):
    from oracle import canonswap_ref as O
    inp, idv, lat, std = pool_modes
    a = [torch.from_numpy(inp[k][frame:frame + 1]) for k in ("img", "x_t", "x_can")]
    with torch.no_grad():
        ref = O.swap_frame(state_dicts, *a, idv)["out"]
    g = [t.cuda() for t in a]
    o1 = lat.swap_frames(*g, idv.cuda())["out"]
    o2 = lat.swap_frames(*g, idv.cuda())["out"]
    assert torch.equal(o1, o2)
    pl = O.psnr(o1.cpu(), ref)
    ps = O.psnr(std.swap_frames(*g, idv.cuda())["out"].cpu(), ref)
    print(f"pool frame {frame}: latency mode {pl:.2f} dB, default mode {ps:.2f} dB")
    assert pl >= 50.0 and ps >= 50.0, (frame, pl, ps)
    assert pl >= ps - 0.5, (frame, pl, ps)            # the mode costs no margin: within half a dB of the default mode's value on the same frame


@pytest.mark.parametrize("knob,lat", [("CANONSWAP_VOL32_XF=0", 0), ("CANONSWAP_WIDE=2", 0), ("CANONSWAP_WIDE=0", 0),
                                      ("CANONSWAP_SHARED_DEDUP=0", 0), ("CANONSWAP_DEC_PHASES_DEEP=0", 0)])
def test_knob_product_paths_through_swap_frames(state_dicts, knob, lat, monkeypatch):
    """The knobs that select another PRODUCT path (R's GroupNorm apply as its own launch instead of inside the consumer conv's staging; SPADE
    gamma / beta on conv_wide: the same bits) and the one that takes conv_wide out, through swap_frames of an engine created under them, on pool
    frames 0 and 63 (seed 1000, identity 7: the bench's pool), one frame per call, against an engine created with the variable removed;
    mlp_shared with every row phase launched (the same bits as the de-duplicated form) and the hourglass' up-blocks 0 - 2 as 27-tap convs.
    (CANONSWAP_R_SPLIT=0 - R without its split-precision passes - measured 49.5 dB on frame 63 here and was removed: round 6.)"""
    from canonswap_amd import synth
    from oracle import canonswap_ref as O
    k, v = knob.split("=")
    inp = synth.make_frame_inputs(64, seed=1000, size=256)
    idv = torch.from_numpy(synth.make_identity(7))
    outs = {}
    for tag, env in (("knob", {k: v}), ("base", {k: None})):
        with swapper_with_env(monkeypatch, state_dicts, env, max_batch=1, latency_mode=bool(lat)) as sw:
            outs[tag] = {}
            for j in (0, 63):
                g = [torch.from_numpy(inp[kk][j:j + 1]).cuda() for kk in ("img", "x_t", "x_can")]
                outs[tag][j] = sw.swap_frames(*g, idv.cuda())["out"].cpu()
    for j in (0, 63):
        a = [torch.from_numpy(inp[kk][j:j + 1]) for kk in ("img", "x_t", "x_can")]
        with torch.no_grad():
            ref = O.swap_frame(state_dicts, *a, idv)["out"]
        p = O.psnr(outs["knob"][j], ref)
        print(f"{knob} latency={lat} pool frame {j}: {p:.2f} dB (default build {O.psnr(outs['base'][j], ref):.2f})")
        assert p >= 50.0, (knob, j, p)
        if k in ("CANONSWAP_WIDE", "CANONSWAP_SHARED_DEDUP") and not lat:
            assert torch.equal(outs["knob"][j], outs["base"][j]), (knob, j)       # conv_wide and conv_halo add in the same order
