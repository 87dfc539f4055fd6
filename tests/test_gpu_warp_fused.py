"""dm_softmax_warp_kernel: softmax over the 22 mask logits -> deformation -> trilinear feature warp in one kernel (dense_motion.py:88-94 ->
warping_network.py:46-62), the sampling grid never going through HBM.  Same per-voxel operation sequence as dm_softmax_kernel followed by
grid_sample_kernel: identical bits (second engine created under CANONSWAP_WARP_FUSED=0); parity against the oracle is covered by
tests/test_gpu_stages.py (test_warp / test_warp_decode run the fused kernel by default)."""
import numpy as np
import pytest
import torch

from chain_helpers import swapper_with_env

pytestmark = pytest.mark.gpu


def _four(sw, f, x_t, x_can):
    out, occ = sw.warping_module.warp(f.cuda(), kp_source=x_t.cuda(), kp_driving=x_can.cuda())
    fwd = sw.warping_module(f.cuda(), kp_source=x_can.cuda(), kp_driving=x_t.cuda())
    return [out.cpu(), occ.cpu(), fwd["out"].cpu(), fwd["deformation"].cpu()]


def test_fused_softmax_warp_equals_two_kernels(state_dicts, monkeypatch):
    from canonswap_amd import synth
    from canonswap_amd.can_swap_e2e import can_swapper
    r = np.random.Generator(np.random.PCG64(17))
    f = torch.from_numpy((0.08 * r.standard_normal((3, 32, 16, 64, 64))).astype(np.float32))
    inp = synth.make_frame_inputs(3, seed=77, size=256)
    x_t, x_can = torch.from_numpy(inp["x_t"]), torch.from_numpy(inp["x_can"])
    sw = can_swapper(None, state_dicts=state_dicts, max_batch=3)
    got = _four(sw, f, x_t, x_can)
    with swapper_with_env(monkeypatch, state_dicts, {"CANONSWAP_WARP_FUSED": "0"}, max_batch=3) as off:
        want = _four(off, f, x_t, x_can)
    for a, b in zip(got, want):
        assert torch.equal(a, b), float((a - b).abs().max())
