"""Restatement of the identity network behind can_swapper.getid for the tests (written from the description of the network, driven by the
state-dict of the pickled class; nothing here comes from the reference's program text).

getid = F.interpolate(img, (112, 112)) [nearest] -> ResNet(IRBlock, [3, 4, 14, 3], use_se=True) -> F.normalize(p=2, dim=1):
  stem     conv1 3 -> 64, 3x3, no padding, no bias (112 -> 110) -> bn1 -> PReLU (one slope) -> MaxPool2d(2, 2) (-> 55)
  IRBlock  bn0 -> conv3x3 -> bn1 -> PReLU -> conv3x3(stride) -> bn2 -> SE -> + residual -> PReLU (the same slope); conv3x3 = 3x3, padding 1, no bias;
           the first block of layers 2-4 has stride 2 and a downsample (1x1 stride-2 conv + BN) on the residual
  SE       mean over (h, w) -> Linear(C, C/16) -> PReLU -> Linear(C/16, C) -> sigmoid -> scale
  tail     bn2 -> flatten in NCHW order -> fc 25088 -> 512 -> bn3 (BatchNorm1d); dropout is the identity in eval

forward(..., emulate=True) rounds the two operands of every convolution and linear layer to fp16 and accumulates wide: the arithmetic of an
fp16-operand / fp32-accumulate engine with nothing else rounded.  `mistake` makes one deliberate error (the discrimination test)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

DEPTHS, DIMS = (3, 4, 14, 3), (64, 128, 256, 512)
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4", "prefc")
MISTAKES = ("se_one", "bn0_into_padding", "second_prelu_skipped", "flatten_hwc")
EPS = 1e-5


def to_tensors(sd, dtype=torch.float64, device="cpu"):
    return {k: torch.as_tensor(np.asarray(v)).to(device=device, dtype=dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def _bn(sd, p, x):
    s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + EPS)
    t = sd[p + ".bias"] - sd[p + ".running_mean"] * s
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return x * s.reshape(shape) + t.reshape(shape)


def _prelu(x, slope):
    return torch.where(x > 0, x, x * slope.reshape(()))


def forward(sd, img, emulate=False, mistake=None, mistake_block=None):
    """sd: to_tensors(state-dict); img (B, 3, H, W) in sd's dtype -> {"raw": (B, 512), "id": (B, 512), stage name: activation (NCHW)}.
    mistake: None or one of MISTAKES; the per-block ones are made in block `mistake_block` (0 .. 23), or in every block with None."""
    assert mistake is None or mistake in MISTAKES
    dt = img.dtype
    q = (lambda t: t.half().to(dt)) if emulate else (lambda t: t)
    conv = lambda x, w, **kw: F.conv2d(q(x), q(w), **kw)
    lin = lambda x, w, b: F.linear(q(x), q(w), b)
    st = {}
    x = F.interpolate(img, size=(112, 112))                     # nearest
    x = _prelu(_bn(sd, "bn1", conv(x, sd["conv1.weight"])), sd["prelu.weight"])
    x = F.max_pool2d(x, 2, 2)
    st["stem"] = x
    bi = 0
    for l, n in enumerate(DEPTHS):
        for k in range(n):
            p = f"layer{l + 1}.{k}"
            stride = 2 if (l > 0 and k == 0) else 1
            wrong = mistake if mistake_block in (None, bi) else None
            res = x
            if wrong == "bn0_into_padding":                     # the affine applied to the zero border too
                out = conv(_bn(sd, p + ".bn0", F.pad(x, (1, 1, 1, 1))), sd[p + ".conv1.weight"])
            else:
                out = conv(_bn(sd, p + ".bn0", x), sd[p + ".conv1.weight"], padding=1)
            out = _prelu(_bn(sd, p + ".bn1", out), sd[p + ".prelu.weight"])
            out = _bn(sd, p + ".bn2", conv(out, sd[p + ".conv2.weight"], stride=stride, padding=1))
            y = out.mean(dim=(2, 3))
            y = _prelu(lin(y, sd[p + ".se.fc.0.weight"], sd[p + ".se.fc.0.bias"]), sd[p + ".se.fc.1.weight"])
            y = torch.sigmoid(lin(y, sd[p + ".se.fc.2.weight"], sd[p + ".se.fc.2.bias"]))
            if wrong == "se_one":
                y = torch.ones_like(y)
            out = out * y[:, :, None, None]
            if p + ".downsample.0.weight" in sd:
                res = _bn(sd, p + ".downsample.1", conv(x, sd[p + ".downsample.0.weight"], stride=stride))
            out = out + res
            x = out if wrong == "second_prelu_skipped" else _prelu(out, sd[p + ".prelu.weight"])
            bi += 1
        st[f"layer{l + 1}"] = x
    x = _bn(sd, "bn2", x)
    st["prefc"] = x
    flat = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1) if mistake == "flatten_hwc" else x.reshape(x.shape[0], -1)
    raw = _bn(sd, "bn3", lin(flat, sd["fc.weight"], sd["fc.bias"]))
    st["raw"] = raw
    st["id"] = F.normalize(raw, p=2, dim=1)
    return st


def rel_l2(a, b):
    """Per-row relative L2 error of a against b, rows = the leading dimension."""
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


class TorchNet(torch.nn.Module):
    """The same network as a plain torch module (fp32 by default) - what tools/time_identity.py times the engine against."""

    def __init__(self, sd, dtype=torch.float32, device="cpu"):
        super().__init__()
        self.sd = to_tensors(sd, dtype, device)

    def forward(self, img):
        with torch.no_grad():
            return forward(self.sd, img.to(next(iter(self.sd.values())).dtype))["id"]


def forward_blobs(blobs, img, emulate=True):
    """CPU evaluation of what pack._pack_A produced (the engine's constants, in the engine's data flow): folded fp16 conv weights + fp32 biases, the
    bn0 pairs applied before zero padding, fc in (h, w, c) slices.  float64; with emulate the activations a conv / the fc read are rounded to fp16
    as the engine stores them."""
    from canonswap_amd import pack
    dt = torch.float64
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    q = (lambda t: t.half().to(dt)) if emulate else (lambda t: t)
    sl = T(blobs["A.slopes"])
    aff = lambda x, n: x * T(blobs[n + ".s"]).reshape(1, -1, 1, 1) + T(blobs[n + ".t"]).reshape(1, -1, 1, 1)
    x = F.interpolate(img.to(dt), size=(112, 112))
    w = T(pack.unpack_id_conv(blobs["A.stem.w"], 3, 3, 3))
    x = _prelu(F.conv2d(q(x), w) + T(blobs["A.stem.b"]).reshape(1, -1, 1, 1), sl[0])
    x = F.max_pool2d(x, 2, 2)
    blocks = pack.id_blocks()
    for i, (n, _, cin, cout, stride) in enumerate(blocks):
        a = q(aff(x, n + ".pre"))
        h = F.conv2d(a, T(pack.unpack_id_conv(blobs[n + ".c1.w"], cin, 3, 3)), padding=1) + T(blobs[n + ".c1.b"]).reshape(1, -1, 1, 1)
        h = q(_prelu(h, sl[1 + 2 * i]))
        o = F.conv2d(h, T(pack.unpack_id_conv(blobs[n + ".c2.w"], cin, 3, 3)), stride=stride, padding=1) + T(blobs[n + ".c2.b"]).reshape(1, -1, 1, 1)
        y = _prelu(F.linear(o.mean(dim=(2, 3)), T(blobs[n + ".se.w1"]), T(blobs[n + ".se.b1"])), sl[2 + 2 * i])
        y = torch.sigmoid(F.linear(y, T(blobs[n + ".se.w2"]), T(blobs[n + ".se.b2"])))
        res = x
        if n + ".ds.w" in blobs:
            res = F.conv2d(q(x), T(pack.unpack_id_conv(blobs[n + ".ds.w"], cin, 1, 1)), stride=stride) + T(blobs[n + ".ds.b"]).reshape(1, -1, 1, 1)
        x = _prelu(o * y[:, :, None, None] + res, sl[1 + 2 * i])
    a = q(aff(x, "A.post")).permute(0, 2, 3, 1).reshape(x.shape[0], 49, 512)                 # [b][h * 7 + w][c]
    return torch.einsum("bpc,poc->bo", a, T(blobs["A.fc.w"])) + T(blobs["A.fc.b"])
