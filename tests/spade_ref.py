"""The SPADE decoder G launch by launch, restated in the reference's form (spade_generator.py:41-59, util.py:282-344) for the tests of run_G.

Every step is a function of the tensors the engine's launch of that name reads, [1, C, H, W] in the dtype of its first argument: float64 gives the
reference value R of a step, float32 (torch on the CPU) the stand-in E32 whose distance from R sizes the fp32 allowance of the gates.  Weights
come from the unpacked state dict through GWeights: spectral weights by oracle.canonswap_ref.spectral_weight; `rounded` rounds to fp16 what
pack._pack_G rounds (every conv weight; the composed W_s W_beta of a learned shortcut after the float64 product; mlp_shared's summed taps per
output phase) and to fp32 its biases.  Where the engine runs another form the step is written in the reference's:
  mlp_shared of the up blocks   a 3x3 conv on the nearest-resized seg, evaluated per output phase with stride s (the taps of a phase that read the
                                same source pixel carry their summed weight on the first of them: with unrounded weights the plain conv);
  SPADE of an up block          on the nearest-up-sampled x, with the statistics the caller passes;
  the learned shortcut          conv_s(IN(x)(1 + gamma) + beta) (shortcut_reference), next to the three launches .bs / .ng / .cs the engine runs.
shared_replay replays run_G's phase bookkeeping (grouped phases, the de-duplicated row 4 i + 2, the duplicated middle pixel) in numpy from
pack._pack_G's blobs; the CPU test ties all forms to oracle.canonswap_ref.spade_decoder and shows that the gates bite."""
import numpy as np
import torch
import torch.nn.functional as F

from canonswap_amd import pack
from oracle import canonswap_ref as O

BLOCKS = [f"G_middle_{b}" for b in range(6)] + ["up_0", "up_1"]
SHARED = {
    "G.shared64": [f"G_middle_{b}.norm_{k}" for b in range(6) for k in (0, 1)],
    "G.shared128": ["up_0.norm_0", "up_0.norm_1", "up_0.norm_s"],
    "G.shared256": ["up_1.norm_0", "up_1.norm_1", "up_1.norm_s"],
}
EPS = 1e-5


def r16(t):
    """through fp16 (round to nearest even, ONE rounding: numpy's conversion, as pack.py's), back in t's dtype"""
    return torch.from_numpy(t.numpy().astype(np.float16)).to(t.dtype)


def r32(t):
    return t.to(torch.float32).to(t.dtype)


def spacing16(ref):
    """fp16 spacing in the binade of |ref|: 2^(e - 10), 2^-24 below 2^-14"""
    a = ref.abs().double().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


class GWeights:
    """The weights of G's steps as float64 tensors from the state dict sd (torch tensors); rounded: as the engine multiplies them"""

    def __init__(self, sd, rounded=True):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.rounded = rounded

    def _w(self, w):
        return r16(w) if self.rounded else w

    def _b(self, b):
        return r32(b) if self.rounded else b

    def plain(self, p):
        return self._w(self.sd[p + ".weight"]), self._b(self.sd[p + ".bias"])

    def spectral(self, p):
        return self._w(O.spectral_weight(self.sd, p)), self._b(self.sd[p + ".bias"])

    def shared(self, group):
        """mlp_shared of the norms of one resolution, concatenated as pack._pack_G concatenates them (UNROUNDED weight: shared_step rounds)"""
        w = torch.cat([self.sd[q + ".mlp_shared.0.weight"] for q in SHARED[group]], 0)
        return w, self._b(torch.cat([self.sd[q + ".mlp_shared.0.bias"] for q in SHARED[group]]))

    def gb(self, p):
        """(W_gamma, b_gamma, W_beta, b_beta) of SPADE p"""
        return self.plain(p + ".mlp_gamma") + self.plain(p + ".mlp_beta")

    def shortcut(self, p, bias_through_ws=True):
        """The learned shortcut of block p as the engine composes it at load time: .ng = (W_gamma, b_gamma), .bs = (W_s W_beta, W_s b_beta),
        .cs = W_s.  bias_through_ws=False: the wrong composition that leaves b_beta as it is (a mutation of the CPU test)."""
        ws = O.spectral_weight(self.sd, p + ".conv_s")[:, :, 0, 0]
        wb, bb = self.sd[p + ".norm_s.mlp_beta.weight"], self.sd[p + ".norm_s.mlp_beta.bias"]
        wbs = torch.einsum("oc,cjhw->ojhw", ws, wb)
        bbs = ws @ bb if bias_through_ws else bb[:ws.shape[0]]
        return {"ng": self.plain(p + ".norm_s.mlp_gamma"), "bs": (self._w(wbs), self._b(bbs)), "cs": self._w(ws)[:, :, None, None]}


def _to(x, *ts):
    return [None if t is None else t.to(x.dtype) for t in ts]


def conv3(x, w, b=None, drop_chunk=None):
    """3x3 'same' conv; drop_chunk = k: without input channels [32 k, 32 k + 32) (a mutation of the CPU test)"""
    w, b = _to(x, w, b)
    if drop_chunk is not None:
        w = w.clone()
        w[:, 32 * drop_chunk:32 * drop_chunk + 32] = 0
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


def chan_stats(x):
    """(mean, 1 / sqrt(var + 1e-5)) per channel of x [1, C, H, W] as [C] tensors: InstanceNorm2d's statistics (util.py:286), biased variance"""
    return x.mean((0, 2, 3)), 1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + EPS)


def step_fc(seg, W, **kw):
    return conv3(seg, *W.plain("fc"), **kw)


def phase_weight(w, s, a, b, rounded):
    """The 3x3 weight that output phase (a, b) of the x`s` nearest-resized map sees: taps that read the same source pixel carry their float64 sum
    (rounded to fp16 as pack does) on the first of them, the others are zero"""
    off = lambda ph, d: (ph + d - 1) // s
    out = torch.zeros_like(w)
    first = {}
    for dy in range(3):
        for dx in range(3):
            key = (off(a, dy), off(b, dx))
            ty, tx = first.setdefault(key, (dy, dx))
            out[:, :, ty, tx] += w[:, :, dy, dx]
    return r16(out) if rounded else out


def step_shared(seg, W, group, s):
    """relu(mlp_shared(nearest_resize(seg, x s))) of every norm of one resolution: [1, 128 n, 64 s, 64 s]"""
    w, b = W.shared(group)
    if s == 1:
        return F.relu(conv3(seg, W._w(w), b))
    up = F.pad(O.nearest_up(seg, 1, s, s), (1, 1, 1, 1))
    Hs = seg.shape[2]
    out = seg.new_zeros(1, w.shape[0], Hs * s, Hs * s)
    for a in range(s):
        for bb in range(s):
            wp, bp = _to(seg, phase_weight(w, s, a, bb, W.rounded), b)
            out[:, :, a::s, bb::s] = F.conv2d(up[:, :, a:, bb:], wp, bp, stride=s)[:, :, :Hs, :Hs]
    return F.relu(out)


def normalized(x, stats, up):
    """IN(x) with the statistics passed in, on the nearest-up-sampled x where up"""
    mean, rstd = _to(x, *stats)
    if up:
        x = O.nearest_up(x, 1, 2, 2)
    return (x - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)


def spade(x, stats, actv, gbw, up=False, **kw):
    """util.py:295-302 with actv = relu(mlp_shared(seg)) given: IN(x)(1 + gamma) + beta"""
    wg, bg, wb, bb = gbw
    return normalized(x, stats, up) * (1 + conv3(actv, wg, bg, **kw)) + conv3(actv, wb, bb, **kw)


def step_spade(x, stats, actv, gbw, up=False, **kw):
    return F.leaky_relu(spade(x, stats, actv, gbw, up, **kw), 0.2)


def step_conv(h, wb, res=None, **kw):
    y = conv3(h, *wb, **kw)
    return y if res is None else y + res


def step_bs(actv_s, sc):
    return conv3(actv_s, *sc["bs"])


def step_ng(x, stats, actv_s, sc):
    return normalized(x, stats, True) * (1 + conv3(actv_s, *sc["ng"]))


def step_cs(h, bs, sc):
    return conv3(h, sc["cs"]) + bs


def step_ng_cs(x, stats, actv_s, bs, sc):
    """the fused launch of up_1: h is rounded to fp16 where the kernel packs it for conv_s's MFMAs and never stored"""
    return step_cs(r16(step_ng(x, stats, actv_s, sc)), bs, sc)


def shortcut_reference(x, stats, actv_s, W, p):
    """x_s = conv_s(norm_s(x, seg)) as util.py:329-344 writes it (x: before the up-sampling)"""
    ws = W._w(O.spectral_weight(W.sd, p + ".conv_s"))
    return conv3(spade(x, stats, actv_s, W.gb(p + ".norm_s"), up=True), ws)


def step_img(o256, W):
    """conv_img + PixelShuffle(2) + sigmoid on o256 = lrelu(x, 0.2): [1, 3, 512, 512]"""
    return torch.sigmoid(O.pixel_shuffle2(conv3(o256, *W.plain("conv_img.0"))))


def img_logits(o256, W):
    return O.pixel_shuffle2(conv3(o256, *W.plain("conv_img.0")))


def chain(seg, W, stats_from=None, bias_through_ws=True, drop_chunk=None):
    """All of G as the chain of the steps above, each on the previous one's result, statistics from the tensors themselves.
    stats_from = (b, b2): block b's norm_0 takes the statistics of block b2's input (a mutation).  Returns the image and every step's result."""
    t = {}
    t["fc"] = x = step_fc(seg, W)
    a = {1: step_shared(seg, W, "G.shared64", 1), 2: step_shared(seg, W, "G.shared128", 2), 4: step_shared(seg, W, "G.shared256", 4)}
    t["shared64"], t["shared128"], t["shared256"] = a[1], a[2], a[4]
    xs_in = []
    for i, p in enumerate(BLOCKS):
        learned = i >= 6
        s = (1, 1, 1, 1, 1, 1, 2, 4)[i]
        act = a[s]
        k0 = 2 * i * 128 if not learned else 0
        xs_in.append(x)
        sx = chan_stats(x if stats_from is None or stats_from[0] != i else xs_in[stats_from[1]])
        if learned:
            sc = W.shortcut(p, bias_through_ws)
            t[p + ".bs"] = bs = step_bs(act[:, 256:384], sc)
            t[p + ".ng"] = h = step_ng(x, sx, act[:, 256:384], sc)
            t[p + ".cs"] = x_s = step_cs(h, bs, sc)
        else:
            x_s = x
        t[p + ".n0"] = h0 = step_spade(x, sx, act[:, k0:k0 + 128], W.gb(p + ".norm_0"), up=learned)
        t[p + ".c0"] = dx = step_conv(h0, W.spectral(p + ".conv_0"), drop_chunk=drop_chunk if i == 0 else None)
        t[p + ".n1"] = h1 = step_spade(dx, chan_stats(dx), act[:, k0 + 128:k0 + 256], W.gb(p + ".norm_1"))
        t[p + ".c1"] = x = step_conv(h1, W.spectral(p + ".conv_1"), res=x_s)
    t["o256"] = o = F.leaky_relu(x, 0.2)
    t["img"] = step_img(o, W)
    return t["img"], t


# ------------------------------------------------------------------------------------------------ the steps by the engine's launch labels
def step_list(W, fused_up1=True):
    """[(label, out key, fn(T, dtype), phase scale s, stored as fp16, key of the statistics the launch emits or None)] in run_G's order.  T maps keys
    to the tensors a launch reads - fp16 [1, C, H, W] as the engine stored them, statistics as (mean, rstd) fp32 [C] pairs: "seg", "a64" / "a128" /
    "a256", per block i "x.i" (its input; "x.8": lrelu(x, 0.2) feeding conv_img), "sx.i", "bs.i", "hs.i", "xs.i", "h0.i", "dx.i", "s1.i", "h1.i".
    Labels "G.shared128" / "G.shared256" stand for all phase launches of that map.  fused_up1: conv_s inside up_1's .ng launch (h not stored)."""
    L = []

    def add(label, out, fn, s=1, f16=True, st=None):
        L.append((label, out, fn, s, f16, st))

    add("G.fc", "x.0", lambda T, dt: step_fc(T["seg"].to(dt), W), st="sx.0")
    add("G.shared64", "a64", lambda T, dt: step_shared(T["seg"].to(dt), W, "G.shared64", 1))
    add("G.shared128", "a128", lambda T, dt: step_shared(T["seg"].to(dt), W, "G.shared128", 2), 2)
    add("G.shared256", "a256", lambda T, dt: step_shared(T["seg"].to(dt), W, "G.shared256", 4), 4)
    for i, p in enumerate(BLOCKS):
        n = f"G.m{i}" if i < 6 else f"G.up{i - 6}"
        up = i >= 6
        s = (1, 1, 1, 1, 1, 1, 2, 4)[i]
        ak = {1: "a64", 2: "a128", 4: "a256"}[s]
        k0 = 2 * i * 128 if not up else 0

        def A(T, dt, lo, ak=ak):
            return T[ak][:, lo:lo + 128].to(dt)

        if up:
            def sc(p=p):
                return W.shortcut(p)
            add(n + ".bs", f"bs.{i}", lambda T, dt, A=A, sc=sc: step_bs(A(T, dt, 256), sc()), s)
            if i == 7 and fused_up1:
                add(n + ".ng", f"xs.{i}", lambda T, dt, A=A, sc=sc, i=i: step_ng_cs(T[f"x.{i}"].to(dt), T[f"sx.{i}"], A(T, dt, 256), T[f"bs.{i}"].to(dt), sc()), s)
            else:
                add(n + ".ng", f"hs.{i}", lambda T, dt, A=A, sc=sc, i=i: step_ng(T[f"x.{i}"].to(dt), T[f"sx.{i}"], A(T, dt, 256), sc()), s)
                add(n + ".cs", f"xs.{i}", lambda T, dt, sc=sc, i=i: step_cs(T[f"hs.{i}"].to(dt), T[f"bs.{i}"].to(dt), sc()), s)
        add(n + ".n0", f"h0.{i}", lambda T, dt, A=A, i=i, p=p, k0=k0, up=up: step_spade(T[f"x.{i}"].to(dt), T[f"sx.{i}"], A(T, dt, k0), W.gb(p + ".norm_0"), up=up), s)
        add(n + ".c0", f"dx.{i}", lambda T, dt, i=i, p=p: step_conv(T[f"h0.{i}"].to(dt), W.spectral(p + ".conv_0")), s, st=f"s1.{i}")
        add(n + ".n1", f"h1.{i}", lambda T, dt, A=A, i=i, p=p, k0=k0: step_spade(T[f"dx.{i}"].to(dt), T[f"s1.{i}"], A(T, dt, k0 + 128), W.gb(p + ".norm_1")), s)

        def c1(T, dt, i=i, p=p, up=up):
            y = step_conv(T[f"h1.{i}"].to(dt), W.spectral(p + ".conv_1"), res=T[f"xs.{i}" if up else f"x.{i}"].to(dt))
            return F.leaky_relu(y, 0.2) if i == 7 else y
        add(n + ".c1", f"x.{i + 1}", c1, s, st=None if i == 7 else f"sx.{i + 1}")
    add("G.img", "img", lambda T, dt: step_img(T["x.8"].to(dt), W), 2, f16=False)
    return L


def run_steps(W, seg16, fused_up1=True):
    """The step list on a stand-in engine (the CPU test): each step in float64 (R) and in fp32 (E32) from the same stored operands; what the next
    step reads is E32 rounded to fp16, the statistics those of the stored tensor in fp32.  Returns {label: (R, E32, stored, s, fp16)} and T."""
    T = {"seg": seg16.half()}
    res = {}
    for label, out, fn, s, f16, st in step_list(W, fused_up1):
        R, E = fn(T, torch.float64), fn(T, torch.float32)
        T[out] = E.half() if f16 else E
        if st:
            T[st] = chan_stats(T[out].float())
        res[label] = (R, E, T[out], s, f16)
    return res, T


# ------------------------------------------------------------------------------------------------ run_G's phase bookkeeping, replayed
def shared_replay(seg, blobs, group, s, pad_shift=None, dup_row=None):
    """g_a128 / g_a256 as run_G writes them, from pack._pack_G's blobs (numpy, float64; seg [256, 64, 64]): phase p{a}{b0} is a conv on the
    source grid with leading padding (a == 0, b0 == 0) whose output channel k 384 + c goes to pixel (s i + a, s j + b0 + k); at x4 the a = 2
    blobs are not used - the a = 1 phases write rows 4 i + 1 and 4 i + 2 - and the one-block middle phase of a = 0, 3 writes pixels b0 and b0 + 1.
    pad_shift = (a, b0): that phase's leading row padding off by one; dup_row: the row offset the a = 1 duplicate goes to (default 2).
    Returns [384, 64 s, 64 s] with NaN where nothing was written."""
    Hs = seg.shape[1]
    out = np.full((384, Hs * s, Hs * s), np.nan)
    x = torch.from_numpy(np.asarray(seg, np.float64))[None]
    for a in range(s):
        if s == 4 and a == 2:
            continue
        b0 = 0
        while b0 < s:
            edge = b0 in (0, s - 1)
            nb = 1 if edge else s - 2
            kh, kw = (2 if a in (0, s - 1) else 1), (2 if edge else 1)
            ph, pw = int(a == 0), int(b0 == 0)
            dupc = s == 4 and nb == 2 and kh == 2
            nbw = 1 if dupc else nb
            name = f"{group}.p{a}{b0}"
            w = torch.from_numpy(pack.unpack_conv(blobs[name + ".w"], nbw * 384, 256, 1, kh, kw)[:, :, 0].astype(np.float64))
            bias = torch.from_numpy(blobs[name + ".b"].astype(np.float64))
            if pad_shift == (a, b0):
                ph += 1
            y = F.relu(F.conv2d(F.pad(x, (pw, kw - 1 - pw, ph, kh - 1 - ph)), w, bias))[0].numpy()[:, :Hs, :Hs]
            for k in range(nbw):
                out[:, a::s, b0 + k::s] = y[k * 384:(k + 1) * 384]
                if s == 4 and a == 1:
                    out[:, (2 if dup_row is None else dup_row)::s, b0 + k::s] = y[k * 384:(k + 1) * 384]
            if dupc:
                out[:, a::s, b0 + 1::s] = y[:384]
            b0 += nb
    return out


# ------------------------------------------------------------------------------------------------ the gate of a step
def allowance(R, E32):
    return 4.0 * (E32.double() - R).abs().max().item()


def allowance_used(got, R, g, allow):
    """The largest fraction of the fp32 allowance an element needs once the rest of its gate (the fp16 spacing term, the image's sigmoid term) is
    spent.  Among millions of fp16 values some sit on a rounding tie, so the spacing term is always used up: this is the figure with headroom."""
    return (((got.double() - R).abs() - (g - allow)) / allow).clamp_min(0).max().item()


def gate(R, E32, fp16_out=True):
    """Elementwise bound on |engine - R| for a step whose float64 result is R: half the fp16 spacing at |R| where the engine stores fp16, plus
    4 x max |E32 - R| for the fp32 accumulation and the epilogue's fp32 roundings (E32: the same step in fp32 from the same operands)."""
    allow = allowance(R, E32)
    g = torch.full_like(R, allow)
    return g + 0.5 * spacing16(R) if fp16_out else g


def used(got, R, g):
    """the largest fraction of the gate an element uses, the absolute error there and the gate there"""
    fr = (got.double() - R).abs() / g
    fr = torch.nan_to_num(fr, nan=float("inf"))
    i = int(fr.argmax())
    return fr.flatten()[i].item(), (got.double() - R).abs().flatten()[i].item(), g.flatten()[i].item()


def breakdown(got, R, g, s=1):
    """fraction of the gate used in the 4-pixel border bands and in the interior, per output phase (y mod s, x mod s), and the worst channel"""
    fr = torch.nan_to_num((got.double() - R).abs() / g, nan=float("inf"))[0]
    out = {"top": fr[:, :4].max().item(), "bottom": fr[:, -4:].max().item(), "left": fr[:, :, :4].max().item(), "right": fr[:, :, -4:].max().item(),
           "interior": fr[:, 4:-4, 4:-4].max().item(), "channel": int(fr.amax((1, 2)).argmax())}
    if s > 1:
        ph = {(a, b): fr[:, a::s, b::s].max().item() for a in range(s) for b in range(s)}
        out["phase"] = max(ph, key=ph.get)
        out["phases"] = ph
    return out
