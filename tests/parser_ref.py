"""Restatement of the SegFormer face parser for the tests (written from the description of the network in DESIGN section 8.8, driven by the
state-dict in the published checkpoint's spelling; nothing here is the engine's code).

  stage s    patch embedding (conv 7x7 / 4 / 3, then 3x3 / 2 / 1, with bias) -> LayerNorm over channels -> blocks -> LayerNorm
  block      x += o_proj(attn(LN1 x));  x += fc2(GELU(dwconv3x3(fc1(LN2 x))))          (pre-norm; GELU in its erf form)
  attention  q = q_proj(LN1 x); keys and values from LN_sr(conv_{sr x sr, stride sr}(LN1 x)) when sr > 1, else from LN1 x;
             softmax(q k^T d^-1/2) v per head, heads = contiguous channel slices of width d = C / heads
             every LayerNorm has eps = 1e-5 (nn.LayerNorm's default: the class never passes config.layer_norm_eps)
  head       linear_c[s] -> bilinear up-sampling to stage 0's extent (align_corners=False) -> cat(...[::-1]) -> linear_fuse (1x1, no bias) ->
             BatchNorm -> ReLU -> classifier

forward(..., emulate=True) rounds the two operands of every convolution, linear layer and attention matmul to fp16 and accumulates wide, and
sends the decode head through the composed fp16 matrices W'_s of pack.parser_compose_head: the arithmetic of an fp16-operand / wide-accumulate
engine with nothing else rounded (it prices the head's re-association too).  `mistake` makes one deliberate error (the discrimination test)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MISTAKES = ("scale_dropped", "ln_sr_skipped", "slices_not_reversed", "gelu_before_dwconv", "heads_interleaved", "align_corners")
STAGES = ("stage0", "stage1", "stage2", "stage3")
BN_EPS = 1e-5


def to_tensors(sd, dtype=torch.float64):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def _ln(sd, p, x, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def forward(sd, cfg, pv, emulate=False, mistake=None):
    """sd: to_tensors(4.x state-dict); cfg: geometry (synth.MIT_B5's keys; "eps" optional); pv (B, 3, H, W) -> {"logits": (B, L, H/4, W/4),
    "stage0" .. "stage3": the stages' outputs (NCHW), "pre": the map in front of the classifier}."""
    assert mistake is None or mistake in MISTAKES
    dt = pv.dtype
    eps = cfg.get("eps", 1e-5)          # nn.LayerNorm's default: the class does not read config.layer_norm_eps
    q = (lambda t: t.half().to(dt)) if emulate else (lambda t: t)
    lin = lambda x, p: F.linear(q(x), q(sd[p + ".weight"]), sd[p + ".bias"])
    out = {}
    x = pv
    B = pv.shape[0]
    for s in range(4):
        C, heads, sr = cfg["widths"][s], cfg["heads"][s], cfg["sr"][s]
        d = C // heads
        p = f"segformer.encoder.patch_embeddings.{s}"
        k, st, pad = (7, 4, 3) if s == 0 else (3, 2, 1)
        x = F.conv2d(q(x), q(sd[p + ".proj.weight"]), sd[p + ".proj.bias"], stride=st, padding=pad)
        h, w = x.shape[2:]
        x = _ln(sd, p + ".layer_norm", x.flatten(2).transpose(1, 2), eps)                    # (B, N, C)
        for i in range(cfg["depths"][s]):
            b = f"segformer.encoder.block.{s}.{i}"
            a = _ln(sd, b + ".layer_norm_1", x, eps)
            qq = lin(a, b + ".attention.self.query")
            kvin = a
            if sr > 1:
                r = F.conv2d(q(a.transpose(1, 2).reshape(B, C, h, w)), q(sd[b + ".attention.self.sr.weight"]), sd[b + ".attention.self.sr.bias"], stride=sr)
                kvin = r.flatten(2).transpose(1, 2)
                if mistake != "ln_sr_skipped":
                    kvin = _ln(sd, b + ".attention.self.layer_norm", kvin, eps)
            kk, vv = lin(kvin, b + ".attention.self.key"), lin(kvin, b + ".attention.self.value")
            if mistake == "heads_interleaved":
                split = lambda t: t.reshape(B, -1, d, heads).permute(0, 3, 1, 2)
            else:
                split = lambda t: t.reshape(B, -1, heads, d).transpose(1, 2)              # (B, heads, N, d)
            scale = 1.0 if mistake == "scale_dropped" else float(d) ** -0.5
            sc = torch.matmul(q(split(qq) * scale), q(split(kk)).transpose(-1, -2))
            pr = torch.softmax(sc, dim=-1)
            ctx = torch.matmul(q(pr), q(split(vv)))
            if mistake == "heads_interleaved":
                ctx = ctx.permute(0, 2, 3, 1).reshape(B, -1, C)
            else:
                ctx = ctx.transpose(1, 2).reshape(B, -1, C)
            x = x + lin(ctx, b + ".attention.output.dense")
            a = _ln(sd, b + ".layer_norm_2", x, eps)
            hdn = lin(a, b + ".mlp.dense1")
            Hd = hdn.shape[-1]
            g = hdn.transpose(1, 2).reshape(B, Hd, h, w)
            dw = lambda t: F.conv2d(q(t), q(sd[b + ".mlp.dwconv.dwconv.weight"]), sd[b + ".mlp.dwconv.dwconv.bias"], padding=1, groups=Hd)
            g = dw(F.gelu(g)) if mistake == "gelu_before_dwconv" else F.gelu(dw(g))
            x = x + lin(g.flatten(2).transpose(1, 2), b + ".mlp.dense2")
        x = _ln(sd, f"segformer.encoder.layer_norm.{s}", x, eps)
        x = x.transpose(1, 2).reshape(B, C, h, w)
        out[f"stage{s}"] = x
    h0, w0 = out["stage0"].shape[2:]
    D = cfg["D"]
    up = lambda t: F.interpolate(t, size=(h0, w0), mode="bilinear", align_corners=(mistake == "align_corners"))
    if emulate:
        from canonswap_amd import pack
        ws, bp = pack.parser_compose_head({k: v.numpy() for k, v in pack.parser_rename(sd).items()}, cfg)
        y = torch.as_tensor(bp).to(dt).reshape(1, -1, 1, 1)
        for s in range(4):
            w16 = q(torch.as_tensor(ws[s]).to(dt))
            y = y + up(F.conv2d(q(out[f"stage{s}"]), w16[:, :, None, None]))
    else:
        maps = []
        for s in range(4):
            t = out[f"stage{s}"]
            t = F.linear(t.flatten(2).transpose(1, 2), sd[f"decode_head.linear_c.{s}.proj.weight"], sd[f"decode_head.linear_c.{s}.proj.bias"])
            maps.append(up(t.transpose(1, 2).reshape(B, D, *out[f"stage{s}"].shape[2:])))
        cat = torch.cat(maps if mistake == "slices_not_reversed" else maps[::-1], dim=1)
        y = F.conv2d(cat, sd["decode_head.linear_fuse.weight"])
        p = "decode_head.batch_norm"
        sc = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + BN_EPS)
        y = y * sc.reshape(1, -1, 1, 1) + (sd[p + ".bias"] - sd[p + ".running_mean"] * sc).reshape(1, -1, 1, 1)
    y = F.relu(y)
    out["pre"] = y
    out["logits"] = F.conv2d(q(y), q(sd["decode_head.classifier.weight"]), sd["decode_head.classifier.bias"])
    return out


def rel_l2(a, b):
    """Per-image relative L2 error of a against b."""
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def max_abs(a, b):
    """Per-image max |a - b| over max |b|."""
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return (a - b).abs().amax(dim=1) / b.abs().amax(dim=1)


def margins(logits):
    """Per pixel: the float64 margin between the two largest logits, (B, h, w)."""
    top = logits.double().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def hf_model(sd_np, cfg, dtype=torch.float64):
    """The installed transformers class loaded (strict) with a 4.x state-dict through pack's rename table."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from canonswap_amd import pack
    c = SegformerConfig(depths=list(cfg["depths"]), hidden_sizes=list(cfg["widths"]), num_attention_heads=list(cfg["heads"]), sr_ratios=list(cfg["sr"]),
                        mlp_ratios=[cfg["mlp"]] * 4, decoder_hidden_size=cfg["D"], num_labels=cfg["L"])
    c._attn_implementation = "sdpa"          # the eager path rounds its softmax to fp32 whatever the module's dtype; sdpa stays in the module's dtype
    m = SegformerForSemanticSegmentation(c).eval().to(dtype)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype if np.asarray(v).dtype.kind == "f" else torch.int64)
                       for k, v in pack.parser_rename(sd_np).items()}, strict=True)
    return m
