"""F (appearance_feature_extractor.py:38-48) and R (adaptive_modulate.py:721-733) launch by launch, restated in the reference's form for the tests of
run_F / run_resblocks3d and run_R / run_stage3_xf: what tests/spade_ref.py is for G.

Every step is a function of the tensors the engine's launch of that label reads, in the reference's layout (images [1, C, H, W], volumes
[1, 32, 16, 64, 64]; the 512-channel 2-D view is reshape(1, 512, H, W), channel c 16 + d) and in the dtype asked for: float64 gives the reference
value R of a step, float32 (torch on the CPU) the stand-in E32 whose distance from R sizes the fp32 allowance of the gates (spade_ref.gate).
Weights come from the unpacked state dicts through VWeights, in the reference's form and rounded where pack rounds them:
  BatchNorm folded in float64 as pack.fold_conv_bn does, then rounded to fp16 (fp32 for conv_first, whose kernel multiplies in fp32);
  F's three 2-D layers as the exact sum W_hi + W_lo of pack._hi_lo;
  R's stage-3 convs as the kernel's three terms W_hi a_hi + W_lo a_hi + W_hi a_lo, a_hi = fp16(a), a_lo = fp16(a - a_hi): one conv3d over
  three stacked input groups (s3_conv).
No channel of a weight is reordered here: the tests bring the engine's HWDC memory to the reference's channel order, so a packer that forgets
pack.MEM2REF on F.second or on R's 2-D pair shows.  Operands:
  the down blocks               ReLU, then the mean of the four values, then ONE fp16 rounding (ConvParams::pool_hw);
  the fused ResBlock3d          h = fp16(relu(conv1(a) + b1)) is rounded in R and in E32 alike - the kernel never stores it (G's fused .ng step
                                is treated the same way);
  a transform-staged conv       block 0's conv1 reads the fp32 stream itself; conv2 reads a = lrelu(gn1(y1)), recomputed here from (y1, the slot,
                                gamma, beta) in the kernel's own fp32 operation sequence (gn_engine: common.h gn_scale / gn_shift / gn_lrelu);
                                conv1 of blocks 1 and 2 reads the xf_out volume the same launch stored, which is checked on its own as an
                                elementwise step (kind "gn") under a gate from rounding counts (gn_gate).
chain_F / chain_R chain the steps unrounded; tests/test_volume_ref_cpu.py ties them to oracle.canonswap_ref and shows that the gates bite."""
import numpy as np
import torch
import torch.nn.functional as F

from canonswap_amd import pack
from oracle import canonswap_ref as O
from spade_ref import r16, r32, spacing16

EPS = 1e-5
SLOPE = 0.01
STAGES = (("s1", "resblocks1"), ("s3", "resblocks3"))
MUTATIONS = ("no_wlo", "no_alo", "fp16")      # of s3_conv: without W_lo a_hi, without W_hi a_lo, W_hi a_hi alone


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


class VWeights:
    """The weights of F's and R's steps as float64 tensors from the two state dicts (torch or numpy); rounded: as the engine multiplies them"""

    def __init__(self, sd_f, sd_r, rounded=True):
        self.f = {k: np.asarray(v, np.float64) for k, v in sd_f.items()}
        self.r = {k: np.asarray(v, np.float64) for k, v in sd_r.items()}
        self.rounded = rounded

    def _w(self, w):
        return r16(_t(w)) if self.rounded else _t(w)

    def _b(self, b):
        return r32(_t(b)) if self.rounded else _t(b)

    def _folded(self, sd, p, q):
        """conv p with the BatchNorm q behind it, folded in float64 (pack.fold_conv_bn)"""
        return pack.fold_conv_bn(sd[p + ".weight"], sd[p + ".bias"], *pack.bn_affine(sd, q))

    def first(self):
        w, b = self._folded(self.f, "first.conv", "first.norm")
        return self._b(w), self._b(b)      # an fp32 kernel: the weight is rounded to fp32

    def _hilo(self, w):
        """W_hi + W_lo of pack._hi_lo, exactly"""
        if not self.rounded:
            return _t(w)
        hl = pack._hi_lo(w)
        n = w.shape[1]
        return _t(hl[:, :n] + hl[:, n:])

    def down(self, i):
        w, b = self._folded(self.f, f"down_blocks.{i}.conv", f"down_blocks.{i}.norm")
        return self._hilo(w), self._b(b)

    def second(self):
        return self._hilo(self.f["second.weight"]), self._b(self.f["second.bias"])

    def affine(self, sd, p):
        s, t = pack.bn_affine(sd, p)
        return self._b(s), self._b(t)

    def rb3(self, i, own_post=False):
        """ResBlock3d i of F: (w1, b1) with norm2 folded, (w2, b2), post = the NEXT block's norm1 (None behind the last block).
        own_post: block i's own norm1 instead (a mutation of the CPU test)"""
        p = f"resblocks_3d.3dr{i}"
        w1, b1 = self._folded(self.f, p + ".conv1", p + ".norm2")
        post = None
        if i < 5 or own_post:
            post = self.affine(self.f, f"resblocks_3d.3dr{i if own_post else i + 1}.norm1")
        return (self._w(w1), self._b(b1)), (self._w(self.f[p + ".conv2.weight"]), self._b(self.f[p + ".conv2.bias"])), post

    def s3(self, blk, i, c):
        """(W_hi, W_lo, bias, gamma, beta) of conv c / gn c of stage-3 block blk.i; unrounded: (W, None, ...)"""
        p = f"{blk}.{i}"
        w = self.r[f"{p}.conv{c}.weight"]
        g, b = self._b(self.r[f"{p}.gn{c}.weight"]), self._b(self.r[f"{p}.gn{c}.bias"])
        bias = self._b(self.r[f"{p}.conv{c}.bias"])
        if not self.rounded:
            return _t(w), None, bias, g, b
        hi = w.astype(np.float16).astype(np.float64)
        return _t(hi), _t((w - hi).astype(np.float16)), bias, g, b

    def rb2(self, i):
        """ResBlock2d i of R: (w1, b1) with norm2 folded, (w2, b2), pre = its norm1"""
        p = f"resblocks2.{i}"
        w1, b1 = self._folded(self.r, p + ".conv1", p + ".norm2")
        return (self._w(w1), self._b(b1)), (self._w(self.r[p + ".conv2.weight"]), self._b(self.r[p + ".conv2.bias"])), self.affine(self.r, p + ".norm1")


def conv(x, w, b=None):
    """'same' conv2d / conv3d of x in x's dtype"""
    w = w.to(x.dtype)
    b = None if b is None else b.to(x.dtype)
    return (F.conv3d if w.dim() == 5 else F.conv2d)(x, w, b, padding=w.shape[-1] // 2)


def _aff(x, st):
    s, t = st
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return x * s.to(x.dtype).view(shape) + t.to(x.dtype).view(shape)


def lrelu(x):
    return F.leaky_relu(x, SLOPE)


def vol_stats(x):
    """(mean, 1 / sqrt(var + 1e-5)) per channel of a volume [1, 32, D, H, W] as [32] tensors: GroupNorm(32, 32), biased variance (util.py:521-523)"""
    return x.mean((0, 2, 3, 4)), 1.0 / torch.sqrt(x.var((0, 2, 3, 4), unbiased=False) + EPS)


def stats_close(slot, m64, r64):
    """a (mean, rstd) slot against float64 statistics under test_chan_stats's tolerances: mean rtol 1e-5 / atol 1e-6, rstd rtol 1e-4"""
    return bool(torch.allclose(slot[0].double(), m64, rtol=1e-5, atol=1e-6) and torch.allclose(slot[1].double(), r64, rtol=1e-4, atol=0))


# ------------------------------------------------------------------------------------------------ F
def step_first(img, W):
    return F.relu(conv(img, *W.first()))


def step_down(x, W, i):
    return F.avg_pool2d(F.relu(conv(x, *W.down(i))), 2)


def step_second(p1, W, mem2ref=True):
    """(the 1x1 conv as the volume [1, 32, 16, H, W], relu(norm1 of block 0)).  mem2ref=False: what the engine's memory would hold, brought to the
    reference's order, had pack._pack_F not reordered the rows of second.weight (a mutation of the CPU test)"""
    y = conv(p1, *W.second())
    if not mem2ref:      # memory channel jm would hold reference channel jm; the tests read memory channel jm as reference channel MEM2REF[jm]
        bad = torch.empty_like(y)
        bad[:, torch.from_numpy(pack.MEM2REF)] = y
        y = bad
    y = y.view(1, 32, 16, *y.shape[2:])
    return y, F.relu(_aff(y, W.affine(W.f, "resblocks_3d.3dr0.norm1")))


def step_rb3(a, x, W, i, own_post=False):
    """One ResBlock3d as vol32_fused runs it: (x + conv2(h) + b2, the next block's relu(norm1(.)) or the plain copy), h = relu(conv1(a) + b1)
    rounded to fp16 where the weights are"""
    c1, c2, post = W.rb3(i, own_post)
    h = F.relu(conv(a, *c1))
    if W.rounded:
        h = r16(h)
    y = conv(h, *c2) + x
    return y, (y if post is None else F.relu(_aff(y, post)))


def chain_F(img, W):
    """All of F as the chain of the steps, each on the previous one's result"""
    x = step_down(step_down(step_first(img, W), W, 0), W, 1)
    x, a = step_second(x, W)
    for i in range(6):
        x, a = step_rb3(a, x, W, i)
    return x


# ------------------------------------------------------------------------------------------------ R
def gn_engine(y, stats, gamma, beta, res=None):
    """lrelu(gn(y) [+ res]) in fp32 with the operation sequence of common.h (gn_scale, gn_shift, gn_lrelu: sc = rstd gamma,
    sh = fma(-mean, sc, beta), a = fma(y, sc, sh), a += res, max(a, a * slope)); the fused multiply-adds through float64, whose 53 bits hold the
    product exactly.  y, res: fp32 volumes; returns fp32."""
    mean, rstd = (s.float() for s in stats)
    sc = rstd * gamma.float()
    sh = (-mean.double() * sc.double() + beta.double()).float()
    v = (y.double() * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)).float()
    if res is not None:
        v = v + res.float()
    return torch.maximum(v, v * torch.tensor(SLOPE, dtype=torch.float32))


def gn_ref(y, stats, gamma, beta, res=None):
    """The same in float64 from the same inputs, and the magnitude M = |y sc| + |mean sc| + |beta| + |res| its fp32 roundings scale with"""
    mean, rstd = (s.double().view(1, -1, 1, 1, 1) for s in stats)
    g, b = gamma.double().view(1, -1, 1, 1, 1), beta.double().view(1, -1, 1, 1, 1)
    sc = rstd * g
    v = (y.double() - mean) * sc + b
    M = (y.double() * sc).abs() + (mean * sc).abs() + b.abs()
    if res is not None:
        v = v + res.double()
        M = M + res.double().abs()
    return lrelu(v), M


def gn_gate(R, M, fp16_out=False, second=None):
    """Elementwise bound on |engine - R| of an elementwise GroupNorm launch, from its rounding counts.  gn_scale rounds sc (2^-24 of |y sc| and
    of |mean sc|), gn_shift's fma rounds sh (2^-24 |sh| <= 2^-24 (|mean sc| + |beta|)), gn_lrelu's fma, its sum with the residual and its product
    with the slope round once each (2^-24 of a magnitude <= M): five roundings of at most 2^-24 M, a sixth for their second order.
    second = (|s2|, |t2|): the second affine and its activation add a product, a sum and the slope product (2.01 roundings of at most
    2^-24 (|v s2| + |t2|)) - with the sixth above, 8 2^-24 (M |s2| + |t2|) covers them.  fp16_out: half an fp16 spacing at |R|."""
    if second is None:
        g = 6 * 2.0 ** -24 * M
    else:
        g = 8 * 2.0 ** -24 * (M * second[0] + second[1])
    return g + 0.5 * spacing16(R) if fp16_out else g


def split(a):
    """(a_hi, a_lo) of an fp32 operand as the transform staging splits it: a_hi = fp16(a), a_lo = fp16(a - a_hi), both as fp32"""
    a = a.float()
    hi = r16(a)
    return hi, r16(a - hi)


def s3_conv(a, w, dtype, mutation=None):
    """A stage-3 conv on the operand a.  Rounded weights w = (W_hi, W_lo, bias, ..): the kernel's three terms from a's split, computed in dtype
    as one conv3d over the stacked groups [a_hi | a_hi | a_lo] x [W_hi | W_lo | W_hi]; mutation: one of MUTATIONS.  Unrounded (W, None, bias, ..):
    the plain conv."""
    whi, wlo, bias = w[:3]
    if wlo is None:
        return conv(a.to(dtype), whi, bias)
    hi, lo = split(a)
    xs, ws = [hi], [whi]
    if mutation not in ("no_wlo", "fp16"):
        xs.append(hi); ws.append(wlo)
    if mutation not in ("no_alo", "fp16"):
        xs.append(lo); ws.append(whi)
    return conv(torch.cat(xs, 1).to(dtype), torch.cat(ws, 1), bias)


def split_bound(a, w):
    """Elementwise bound on |three-term float64 result - float64 conv of the unrounded operands|, w the UNROUNDED weight, a the fp32 operand.
    W = W_hi + W_lo + dW with |dW| <= 2^-22 |W| (W_lo a normal fp16) or 2^-25 (W_lo an fp16 subnormal, quantised at 2^-24: every |w| below 2^-3,
    pack._hi_lo's docstring), a = a_hi + a_lo + da likewise, and the term the kernel leaves out is |W_lo a_lo| <= 2^-11 |W| 2^-11 |a|:
    |dW| |a| + |W| |da| + |W_lo a_lo| <= 3 2^-22 |W| |a| + 2^-25 (|a| + |W|), summed over the taps."""
    a, w = a.double().abs(), w.double().abs()
    return 3 * 2.0 ** -22 * conv(a, w) + 2.0 ** -25 * (conv(a, torch.ones_like(w)) + conv(torch.ones_like(a), w))


def step_rb2_c1(a, W, i):
    """conv1 (norm2 folded) + LeakyReLU of ResBlock2d i on the pre-activated volume a, as a volume"""
    return lrelu(conv(a.reshape(1, 512, *a.shape[3:]), *W.rb2(i)[0])).view(a.shape)


def step_rb2_c2(h, x, W, i):
    """(x + conv2(h), lrelu(norm1 of block i + 1) of it, or the plain copy behind the last block)"""
    y = conv(h.reshape(1, 512, *h.shape[3:]), *W.rb2(i)[1]) + x.reshape(1, 512, *x.shape[3:])
    a = lrelu(_aff(y, W.rb2(i + 1)[2])) if i < 2 else y
    return y.view(x.shape), a.view(x.shape)


def chain_R(x, W):
    """All of R as the chain of the steps, statistics from the tensors themselves"""
    def stage(x, blk):
        for i in range(3):
            w1, w2 = W.s3(blk, i, 1), W.s3(blk, i, 2)
            y1 = s3_conv(x, w1, x.dtype)
            a = gn_ref(y1, vol_stats(y1), w1[3], w1[4])[0]
            y2 = s3_conv(a, w2, x.dtype)
            x = gn_ref(y2, vol_stats(y2), w2[3], w2[4], x)[0]
        return x
    x = stage(x, "resblocks1")
    a = lrelu(_aff(x.reshape(1, 512, *x.shape[3:]), W.rb2(0)[2])).view(x.shape)
    for i in range(3):
        x, a = step_rb2_c2(step_rb2_c1(a, W, i), x, W, i)
    return stage(x, "resblocks3")


# ------------------------------------------------------------------------------------------------ the steps by the engine's launch labels
def _step(label, outs, fn, f16, st=None, kind="conv"):
    return dict(label=label, outs=outs, fn=fn, f16=f16, st=st, kind=kind)


def step_list_F(W):
    """One entry per launch of run_F, in its order: label (the profile CSV's), outs (keys of the tensors it stores), fn(T, dtype) -> those tensors,
    f16 (per output: stored as fp16), st (None: F emits no statistics), kind "conv".  T maps keys to the tensors the launch reads, as the engine
    stored them: "img"; "t0", "p0", "p1" (fp16); per block i its input "x.i" (fp32) and "a.i" (fp16).  The closing hwdc_to_ncdhw is a permutation
    and no step."""
    L = [_step("conv_first", ("t0",), lambda T, dt: (step_first(T["img"].to(dt), W),), (True,)),
         _step("F.down0", ("p0",), lambda T, dt: (step_down(T["t0"].to(dt), W, 0),), (True,)),
         _step("F.down1", ("p1",), lambda T, dt: (step_down(T["p0"].to(dt), W, 1),), (True,)),
         _step("F.second", ("x.0", "a.0"), lambda T, dt: step_second(T["p1"].to(dt), W), (False, True))]
    for i in range(6):
        L.append(_step(f"F.rb{i}.c1+c2", (f"x.{i + 1}", f"a.{i + 1}"), lambda T, dt, i=i: step_rb3(T[f"a.{i}"].to(dt), T[f"x.{i}"].to(dt), W, i),
                       (False, True)))
    return L


def step_list_R(W):
    """One entry per stored tensor group of run_R's launches, in its order; T holds "x.in" / "a.in" (ncdhw_to_hwdc's two copies of the input).
    kind "conv": as in step_list_F, st the key of the statistics the launch's chan_stats_finish emits.  kind "gn": an elementwise GroupNorm step -
    the xf_out write-back of conv1 of blocks 1 and 2 (the entry in front of that launch's conv entry, same label) and the norm_act that closes a
    stage; fn(T) -> dict(y, stats, gamma, beta, res[, second = (s2, t2)]) from which gn_engine / gn_ref / gn_gate give the stand-in, R and the
    gate; outs: (the fp32 result[, the fp16 copy]).
    Keys per stage s in ("s1", "s3") and block i: "s.x.i" (residual stream), "s.y1.i", "s.st1.i", "s.y2.i", "s.st2.i"; "s.out", "s.a" (the
    stage's result and its fp16 copy: lrelu(norm1 of resblocks2.0) behind stage 1, plain behind stage 3); "rb2.h.i", "rb2.x.i", "rb2.a.i"."""
    L = []

    def stage(s, blk, xin, last_pre):
        for i in range(3):
            xk = xin if i == 0 else f"{s}.x.{i}"
            if i:      # conv1's transform staging writes the new residual stream: lrelu(gn2(y2) + x) of the previous block
                L.append(_step(f"R.{s}.{i}.c1.sp", (xk,), lambda T, i=i, s=s: dict(
                    y=T[f"{s}.y2.{i - 1}"], stats=T[f"{s}.st2.{i - 1}"], gamma=W.s3(blk, i - 1, 2)[3], beta=W.s3(blk, i - 1, 2)[4],
                    res=T[xin if i == 1 else f"{s}.x.{i - 1}"]), (False,), kind="gn"))
            L.append(_step(f"R.{s}.{i}.c1.sp", (f"{s}.y1.{i}",), lambda T, dt, i=i, xk=xk: (s3_conv(T[xk], W.s3(blk, i, 1), dt),), (False,),
                           st=f"{s}.st1.{i}"))

            def c2(T, dt, i=i, s=s):
                w1 = W.s3(blk, i, 1)
                return (s3_conv(gn_engine(T[f"{s}.y1.{i}"], T[f"{s}.st1.{i}"], w1[3], w1[4]), W.s3(blk, i, 2), dt),)
            L.append(_step(f"R.{s}.{i}.c2.sp", (f"{s}.y2.{i}",), c2, (False,), st=f"{s}.st2.{i}"))
        L.append(_step("norm_act", (f"{s}.out", f"{s}.a"), lambda T, s=s: dict(
            y=T[f"{s}.y2.2"], stats=T[f"{s}.st2.2"], gamma=W.s3(blk, 2, 2)[3], beta=W.s3(blk, 2, 2)[4], res=T[f"{s}.x.2"], second=last_pre),
            (False, True), kind="gn"))

    stage("s1", "resblocks1", "x.in", W.rb2(0)[2])
    for i in range(3):
        ak, xk = ("s1.a", "s1.out") if i == 0 else (f"rb2.a.{i}", f"rb2.x.{i}")
        L.append(_step(f"R.rb2.{i}.c1", (f"rb2.h.{i}",), lambda T, dt, i=i, ak=ak: (step_rb2_c1(T[ak].to(dt), W, i),), (True,)))
        L.append(_step(f"R.rb2.{i}.c2", (f"rb2.x.{i + 1}", f"rb2.a.{i + 1}"),
                       lambda T, dt, i=i, xk=xk: step_rb2_c2(T[f"rb2.h.{i}"].to(dt), T[xk].to(dt), W, i), (False, True)))
    stage("s3", "resblocks3", "rb2.x.3", None)
    return L


def gn_step(entry, T):
    """An elementwise entry on the operands in T: (stand-in outputs, float64 references, gates), one of each per output.  The second affine is
    512-periodic over the memory index d 32 + c in the engine and per channel c 16 + d of the 2-D view here."""
    q = entry["fn"](T)
    v32 = gn_engine(q["y"], q["stats"], q["gamma"], q["beta"], q["res"])
    R, M = gn_ref(q["y"], q["stats"], q["gamma"], q["beta"], q["res"])
    outs, refs, gates = [v32], [R], [gn_gate(R, M)]
    if len(entry["outs"]) == 2:
        sec = q.get("second")
        if sec is None:
            outs.append(r16(v32)); refs.append(R); gates.append(gn_gate(R, M, True))
        else:
            s2, t2 = (t.view(1, 32, 16, 1, 1) for t in sec)
            outs.append(r16(lrelu(v32 * s2.float() + t2.float())))
            R2 = lrelu(R * s2 + t2)
            refs.append(R2); gates.append(gn_gate(R2, M, True, (s2.abs(), t2.abs())))
    return outs, refs, gates


def run_steps(steps, T, stats_of=vol_stats):
    """The step list on a stand-in engine (the CPU test): each conv step in float64 (R) and in fp32 (E32) from the same stored operands, each
    elementwise step by gn_engine; what the next step reads is the stand-in's result as the engine would store it, the statistics those of the
    stored tensor (stats_of) in fp32.  Fills T; returns {(label, out key): (R, E32, stored, fp16, gate)}."""
    res = {}
    for e in steps:
        if e["kind"] == "gn":
            outs, refs, gates = gn_step(e, T)
            for k, o, r, g in zip(e["outs"], outs, refs, gates):
                T[k] = o
                res[(e["label"], k)] = (r, o, o, k == e["outs"][-1] and len(e["outs"]) == 2, g)
            continue
        Rs, Es = e["fn"](T, torch.float64), e["fn"](T, torch.float32)
        for k, r, x, f16 in zip(e["outs"], Rs, Es, e["f16"]):
            T[k] = x.half() if f16 else x
            res[(e["label"], k)] = (r, x, T[k], f16, None)
        if e["st"]:
            T[e["st"]] = tuple(s.float() for s in stats_of(T[e["outs"][0]].double()))
    return res
