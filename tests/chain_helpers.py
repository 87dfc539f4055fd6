"""What the chain and motion tests share (test_gpu_chain.py, test_gpu_v2i_chain.py, test_gpu_motion.py): the weights with M, the swapper
their module-scope fixtures hand out, synthetic geometry and masks, and the two stream helpers of the ordering tests; and the swapper of the
tests that hold two forms of a stage to each other (an engine created under CANONSWAP_* switches)."""
import contextlib

import numpy as np
import torch


def motion_state_dicts():
    from canonswap_amd import synth
    return synth.to_torch(synth.make_state_dicts(0, modules=synth.MODULES + ("motion_extractor",)))


def swapper_b4(sds):
    from canonswap_amd.can_swap_e2e import can_swapper
    return can_swapper(None, state_dicts=sds, max_batch=4)


@contextlib.contextmanager
def swapper_with_env(monkeypatch, sds, env, **kw):
    """can_swapper(None, state_dicts=sds, **kw) created with the variables of `env` set (value None: removed).  The environment is put back right
    after construction, before the first launch: an engine takes its switches at cs_create (csrc/knobs.h), so every comparison on this helper
    also holds the other form to having been chosen there.  The engine is closed on exit."""
    from canonswap_amd.can_swap_e2e import can_swapper
    with monkeypatch.context() as m:
        for k, v in env.items():
            if v is None:
                m.delenv(k, raising=False)
            else:
                m.setenv(k, v)
        sw = can_swapper(None, state_dicts=sds, **kw)
    try:
        yield sw
    finally:
        sw.engine.close()


def _affine(k, Ho, Wo):
    th, sc = 0.1 * k - 0.15, 0.8 + 0.12 * k
    tx, ty = 0.3 * Wo - 40.5 * k, 0.1 * Ho + 33.25 * k
    return np.array([[sc * np.cos(th), -sc * np.sin(th), tx], [sc * np.sin(th), sc * np.cos(th), ty], [0, 0, 1]], np.float64)


def _masks(n, seed=5):
    r = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    out = []
    for k in range(n):
        cx, cy, a, b = r.uniform(200, 312), r.uniform(200, 312), r.uniform(120, 200), r.uniform(150, 220)
        out.append((((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1).astype(np.uint8))
    return np.stack(out)


def _logits(n, seed):
    """Fixed stand-in logits (n, 19, 128, 128): noise, with the skin class (1, a valid one) raised in a block about the middle.  Noise is rich
    in near-ties of the arg-max: one changed logit flips a label."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((n, 19, 128, 128), generator=g)
    lg[:, 1, 30:100, 36:92] += 8.0
    return lg.cuda()


def _timed():
    return torch.cuda.Event(enable_timing=True)


def _occupy(stream, ms):
    """Keep `stream` busy for about `ms` milliseconds with one bounded spin kernel (torch.cuda._sleep counts GPU clock cycles: calibrated
    here first), so that work queued behind it on that stream is certainly still pending while the caller's stream runs."""
    a, b = _timed(), _timed()
    with torch.cuda.stream(stream):
        a.record()
        torch.cuda._sleep(1_000_000)
        b.record()
    b.synchronize()
    per_ms = 1e6 / max(a.elapsed_time(b), 1e-3)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(min(min(ms, 200.0) * per_ms, 1e9)))
