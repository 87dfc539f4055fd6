"""The case table of tests/test_gpu_conv_bounds.py: one case (at least) per instantiation of conv_halo's kernel template that
canonswap_amd/csrc/conv_halo.hip can launch.  A dispatch row is (tile configuration, chunk width, mode, static shape or 0); every case names the
row it is meant to reach, tests/test_conv_ref_cpu.py checks on the host that it does (halo_plan() on the case's ConvParams, then the static-shape
condition of launch_halo_cfg) and that the rows of this table are exactly the call sites of conv_halo.hip.  No torch in here.

Shapes: two tiles along every tiled axis (interior halo edges), tiles within one sample except the `tail` cases, whose 128-position tiles hold two
8 x 8 samples of a batch of three (nTN rounds up).  halo_plan() has no partial tiles along W, H or D - set_tile() takes nT = extent / tile and
the epilogue stores whole tiles - so every extent is a multiple of its tile; the batch is the one axis with a tail.  Cin: two chunks or more.
Cout < Cout_pad (8 packed rows without an output channel) wherever the case is not about a branch-free epilogue copy, and two channel blocks per tile where the tile is narrower than 160."""

STD, TBLEND, SPADE, PIXSHUF, STDSTAT = 0, 1, 2, 3, 4
MODE_NAME = {STD: "STD", TBLEND: "TBLEND", SPADE: "SPADE", PIXSHUF: "PIXSHUF", STDSTAT: "STDSTAT"}
# CFG_H_* of common.h -> (name, BM, BN, wave_px) of conv_plan.h's halo_tile()
TILES = {10: ("128x128", 128, 128, 64), 11: ("128x64", 128, 64, 64), 12: ("256x32", 256, 32, 64), 13: ("128x32", 128, 32, 32),
         14: ("128x16", 128, 16, 32), 15: ("256x16", 256, 16, 64), 16: ("SK128x32", 128, 32, 32), 17: ("128x256", 128, 256, 64),
         18: ("128x160", 128, 160, 64), 19: ("256x160", 256, 160, 64), 20: ("256x64", 256, 64, 64)}

CASES = []


def case(hcfg, ck, mode, stv, k, dims, cin, form="f32", tile=(0, 0), cout_pad=None, cout=None, cin_real=None, tag="", **kw):
    """dims = (N, D, H, W) of the output; form: the epilogue form (test_gpu_conv_bounds.py FORMS); kw: ragged, rep (the batch is `rep` copies of
    dims[0] distinct samples), general (ep_general), layout (hwdc: tensors stored [N][H][W][D][C]), other (see the end of the table)"""
    bn = TILES[hcfg][2]
    if cout_pad is None:
        cout_pad = bn if bn >= 160 else 2 * bn
    if cout is None:
        cout = (cout_pad // 2 if mode in (TBLEND, SPADE) else cout_pad) - 8
    name = "%s-ck%d-%s-st%d-%s%s" % (TILES[hcfg][0], ck, MODE_NAME[mode], stv, form, "-" + tag if tag else "")
    assert name not in [c["name"] for c in CASES], name
    CASES.append(dict(name=name, row=(hcfg, ck, mode, stv), k=k, dims=dims, cin=cin, cin_real=cin_real or cin, cout_pad=cout_pad, cout=cout,
                      tile=tile, form=form, **kw))


K33, K333, K322, K771, K11 = (1, 3, 3), (3, 3, 3), (3, 2, 2), (7, 7, 1), (1, 1, 1)
S2 = dict(k=K33, dims=(2, 1, 16, 32))                           # static shape 1: 16 x 8 tiles, 2 x 2 of them
D2 = dict(k=K33, dims=(2, 1, 32, 16), tile=(8, 16))             # 128 positions as 8 x 16: no static shape has it
D2T = dict(k=K33, dims=(3, 1, 16, 16), tile=(8, 8))             # 8 x 8: two samples per 128-position tile, the batch of three leaves a tail
D2B = dict(k=K33, dims=(2, 1, 32, 32))                          # 256-position tiles: 16 x 16
V2 = dict(k=K333, dims=(2, 4, 16, 16))                          # static shape 2: 8 x 8 x 2
V5 = dict(k=K333, dims=(2, 16, 8, 8), tile=(4, 4))              # static shape 5: 4 x 4 x 8
V3 = dict(k=K333, dims=(2, 32, 8, 8), tile=(4, 4))              # static shape 3 (256 positions): 4 x 4 x 16
V7 = dict(k=K333, dims=(2, 8, 16, 16))                          # static shape 7 (256 positions): 8 x 8 x 4
DV = dict(k=K333, dims=(2, 8, 8, 16), tile=(8, 4))              # 8 x 4 x 4: dynamic, 128 positions
DVB = dict(k=K333, dims=(2, 16, 8, 16), tile=(8, 4))            # 8 x 4 x 8: dynamic, 256 positions

# ---- 128 x 128 (CFG_H_128x128)
case(10, 64, STD, 1, cin=128, form="f32", **S2)
case(10, 64, STD, 1, cin=128, form="res16_o1", tag="full", cout=256, **S2)
case(10, 32, STD, 1, cin=96, form="f16", **S2)
case(10, 32, STD, 1, cin=64, form="pool", cout=256, **S2)
case(10, 32, STD, 2, cin=64, form="res32_o1", **V2)
case(10, 32, STD, 2, cin=64, form="pool", cout=256, tag="vol", **V2)
case(10, 32, STD, 5, cin=64, form="f16", **V5)
case(10, 32, STD, 13, cin=64, form="f32", k=K322, dims=(2, 4, 16, 16))
case(10, 32, STD, 17, cin=64, form="f16", k=K322, dims=(2, 16, 8, 8), tile=(4, 4))
case(10, 32, STD, 15, cin=96, form="gelu", k=K11, dims=(2, 1, 16, 32))
case(10, 64, STD, 15, cin=128, form="res32_inplace", k=K11, dims=(2, 1, 16, 32), cout=256)
case(10, 64, STD, 10, cin=128, form="f16", k=(1, 2, 2), dims=(2, 1, 16, 32))
case(10, 64, STD, 11, cin=128, form="dup", k=(1, 2, 1), dims=(2, 1, 16, 32), cout=256)
case(10, 64, STD, 14, cin=128, form="f32", k=(1, 1, 2), dims=(2, 1, 16, 32))
case(10, 64, STD, 0, cin=128, form="ps", **D2)
case(10, 64, STD, 0, cin=128, form="f32", tag="tail", **D2T)
case(10, 32, STD, 0, cin=64, form="sigmoid", **DV)
case(10, 32, STD, 0, cin=112, cin_real=110, form="slice_up", k=K333, dims=(2, 8, 8, 16), tile=(8, 4))
for ck, st, sh in ((64, 1, S2), (32, 1, S2), (64, 0, D2), (32, 0, D2)):
    case(10, ck, STDSTAT, st, cin=128 if ck == 64 else 64, form="stat16" if ck == 64 else "stat32", **sh)
    case(10, ck, TBLEND, st, cin=128 if ck == 64 else 64, form="tblend", **sh)
    case(10, ck, SPADE, st, cin=128 if ck == 64 else 64, form="spade%d" % (ck == 32), **sh)
case(10, 32, SPADE, 1, cin=64, form="spade0", tag="general", general=True, cout=128, **S2)

# ---- 128 x 64
case(11, 64, STD, 1, cin=128, form="f16", **S2)
case(11, 32, STD, 1, cin=64, form="res16_o1", **S2)
case(11, 32, STD, 2, cin=64, form="f32", **V2)
case(11, 32, STD, 5, cin=64, form="res32_o1", **V5)
case(11, 32, STD, 13, cin=64, form="f16", k=K322, dims=(2, 4, 16, 16))
case(11, 64, STD, 15, cin=128, form="gelu", k=K11, dims=(2, 1, 16, 32), cout=128)
case(11, 32, STD, 15, cin=96, form="f32o1", k=K11, dims=(2, 1, 16, 32), cout=128)
case(11, 64, STD, 0, cin=128, form="f32", **D2)
case(11, 32, STD, 0, cin=64, form="gelu", **DV)
for ck, st, sh in ((64, 1, S2), (32, 1, S2), (64, 0, D2), (32, 0, D2)):
    case(11, ck, STDSTAT, st, cin=128 if ck == 64 else 64, form="stat32" if ck == 64 else "stat16", **sh)

# ---- 256 x 32
case(12, 32, STD, 3, cin=64, form="res32_o1", **V3)
case(12, 32, STD, 3, cin=96, form="hilo", cout_pad=32, cout=32, **V3)
case(12, 32, STD, 12, cin=64, form="f16", k=K322, dims=(2, 32, 8, 8), tile=(4, 4))
case(12, 32, STD, 0, cin=64, form="f32", **DVB)
case(12, 64, STD, 0, cin=128, form="f16", **D2B)
case(12, 32, STDSTAT, 3, cin=64, form="stat32", **V3)
case(12, 32, STDSTAT, 3, cin=96, form="hilo_stat", cout_pad=32, cout=32, **V3)
case(12, 32, STDSTAT, 0, cin=64, form="stat16", **DVB)
case(12, 64, STDSTAT, 0, cin=128, form="stat32", **D2B)

# ---- 128 x 32, 128 x 16, the pixel shuffle, split K
case(13, 32, STD, 2, cin=64, form="f16", **V2)
case(13, 32, STD, 5, cin=64, form="f32", **V5)
case(13, 64, STD, 15, cin=128, form="res32_inplace", k=K11, dims=(2, 1, 16, 32), cout=64)
case(13, 32, STD, 15, cin=96, form="sigmoid", k=K11, dims=(2, 1, 16, 32))
case(13, 64, STD, 0, cin=128, form="ps", **D2)
case(13, 32, STD, 0, cin=64, form="f32", k=(1, 7, 1), dims=(3, 1, 16, 16), tile=(8, 8), tag="tail")
case(14, 64, STD, 1, cin=128, form="sigmoid", cout_pad=16, cout=4, **S2)
case(14, 32, STD, 1, cin=64, form="f16", **S2)
case(14, 64, STD, 0, cin=128, form="f32", **D2)
case(14, 32, STD, 0, cin=64, form="gelu", **D2T)
case(15, 64, PIXSHUF, 0, cin=128, form="pixshuf", cout_pad=16, cout=16, **D2B)
case(15, 32, PIXSHUF, 0, cin=64, form="pixshuf", cout_pad=16, cout=16, **D2B)
case(16, 64, STD, 0, cin=256, form="f32", **D2)
case(16, 32, STD, 0, cin=96, form="f16", k=K333, dims=(2, 8, 8, 16), tile=(8, 4))
case(16, 32, STD, 0, cin=32, form="f32", k=K11, dims=(3, 1, 16, 16), tile=(8, 8), tag="fewsteps")

# ---- 128 x 256
case(17, 64, STD, 1, cin=128, form="f16", **S2)
case(17, 64, STD, 1, cin=64, form="f16", tag="planned", k=K33, dims=(3, 1, 64, 64), cout_pad=256, cout=256, planned=True)
case(17, 64, STD, 1, cin=128, form="res32_o1", tag="full", cout=256, **S2)
case(17, 64, STD, 1, cin=128, form="spmul0", cout=256, **S2)
case(17, 64, STD, 1, cin=128, form="spmul1", tag="general", general=True, **S2)
case(17, 32, STD, 1, cin=96, form="res16_o1", **S2)
for ck, st, sh in ((64, 1, S2), (32, 1, S2)):             # (no dynamic 128x256 kernel: launch_halo_cfg refuses, test_gpu_conv_bounds.py checks that it does)
    case(17, ck, TBLEND, st, cin=128 if ck == 64 else 64, form="tblend", **sh)
    case(17, ck, SPADE, st, cin=128 if ck == 64 else 64, form="spade%d" % (ck == 64), **sh)
case(17, 64, STDSTAT, 1, cin=128, form="stat16", **S2)
case(17, 32, STDSTAT, 1, cin=64, form="stat32", **S2)

# ---- 256 x 64, 256 x 160, 128 x 160
case(20, 32, STD, 7, cin=112, cin_real=110, form="slice", cout_pad=64, cout=64, **V7)
case(20, 32, STD, 7, cin=64, form="pool", cout_pad=64, cout=64, tag="vol", **V7)
case(20, 32, STD, 0, cin=64, form="f32", **D2B)
case(20, 64, STD, 16, cin=128, form="o1only", cout_pad=64, cout=64, tile=(16, 16), k=K33, dims=(2, 1, 32, 32))
case(20, 64, STD, 16, cin=128, form="f16", tile=(16, 16), k=K33, dims=(2, 1, 32, 32))
case(20, 64, STDSTAT, 16, cin=128, form="stat16", tile=(16, 16), k=K33, dims=(2, 1, 32, 32))
case(19, 32, STD, 7, cin=144, cin_real=142, form="f32", ragged=True, rep=17, tag="walk", **V7)
case(19, 32, STD, 7, cin=128, form="f16", **V7)
case(19, 32, STD, 8, cin=144, cin_real=142, form="f32", ragged=True, k=K771, dims=(2, 32, 16, 4), tile=(2, 8))
case(19, 32, STD, 9, cin=144, form="f16", k=K771, dims=(2, 16, 16, 8), tile=(4, 8))
case(19, 32, STD, 0, cin=64, form="f32", **D2B)
case(18, 32, STD, 2, cin=144, cin_real=142, form="f32", **V2)
case(18, 32, STD, 4, cin=144, form="f16", k=K771, dims=(2, 4, 16, 16))
case(18, 32, STD, 6, cin=64, form="f32", k=K771, dims=(2, 16, 16, 4), tile=(2, 8))
case(18, 32, STD, 0, cin=64, form="f16", k=K33, dims=(2, 1, 16, 32))


# ---- epilogue forms on the other kind of row than above (static <-> dynamic) and, for every branch-free copy of the epilogue (conv_epilogue.h,
# CONV_EPILOGUE: every channel real, so Cout = Cout_pad), the same case through the general one (tag general).  Not possible: hilo on a dynamic
# row and pool_hw through the general epilogue - launch_halo_st refuses both.
case(10, 64, STD, 0, cin=128, form="res16_o1", **D2)
case(11, 32, STD, 0, cin=64, form="res32_o1", **DV)
case(11, 64, STD, 0, cin=128, form="f32o1", **D2)
case(13, 32, STD, 0, cin=64, form="res16", **DV)
case(10, 64, STD, 1, cin=128, form="ps", **S2)
case(11, 32, STD, 2, cin=112, cin_real=110, form="slice_up", **V2)
for g in (False, True):
    t = dict(tag="general", general=True) if g else dict(tag="fast")
    case(10, 64, STD, 1, cin=128, form="res16", cout=256, **S2, **t)
    case(17, 64, STD, 1, cin=128, form="res16", cout=256, **S2, **t)
    case(10, 32, STD, 15, cin=96, form="lin32", k=K11, dims=(2, 1, 16, 32), cout=256, **t)
    case(17, 64, STDSTAT, 1, cin=128, form="stat16", cout=256, **S2, **t)
    case(10, 64, STDSTAT, 1, cin=128, form="stat16nores", cout=256, **S2, **t)
    if g:
        case(10, 64, STD, 11, cin=128, form="dup", k=(1, 2, 1), dims=(2, 1, 16, 32), cout=256, **t)
        case(20, 64, STD, 16, cin=128, form="o1only", cout_pad=64, cout=64, tile=(16, 16), k=K33, dims=(2, 1, 32, 32), **t)
        case(11, 32, STD, 15, cin=96, form="f32o1", k=K11, dims=(2, 1, 16, 32), cout=128, **t)
        case(10, 64, STD, 15, cin=128, form="res32_inplace", k=K11, dims=(2, 1, 16, 32), cout=256, **t)
        case(11, 64, STD, 15, cin=128, form="gelu", k=K11, dims=(2, 1, 16, 32), cout=128, **t)
        case(17, 64, STD, 1, cin=128, form="res32_o1", cout=256, **S2, **t)
        case(19, 32, STD, 7, cin=128, form="f16", **V7, **t)
        case(10, 64, STD, 1, cin=128, form="res16_o1", cout=256, **S2, **t)

# ---- cases inside the coverage of the kernels that are otherwise only held bit-equal to conv_halo: conv_wide and conv_lat (3x3, Cin 512, every
# packed channel real; one case per tensor combination they are built for) and vol32 (3x3x3, 32 -> 32, [N][H][W][16][32] volumes: layout hwdc).
# OTHER: which of those kernels must accept the case (test_gpu_conv_bounds.py runs it through them under the same bound).
WL = dict(k=K33, dims=(2, 1, 32, 32), cin=512, cout_pad=256, tag="wl")
case(17, 64, STD, 1, form="f16", cout=256, other=("wide", "lat"), **WL)
case(17, 64, STD, 1, form="res32_o1", cout=256, other=("wide", "lat"), **WL)
case(17, 64, STDSTAT, 1, form="stat16nores", cout=256, other=("wide", "lat"), **WL)
case(17, 64, STDSTAT, 1, form="stat16", cout=256, other=("wide", "lat"), **WL)
case(17, 64, TBLEND, 1, form="tblend16", cout=128, other=("wide", "lat"), **WL)
case(17, 64, TBLEND, 1, form="tblend_o1", cout=128, other=("wide", "lat"), **WL)
case(17, 64, SPADE, 1, form="spade0", cout=128, other=("wide",), **WL)
case(17, 64, SPADE, 1, form="spade1", cout=128, other=("wide",), **WL)
VV = dict(k=K333, dims=(2, 16, 8, 8), tile=(4, 4), cout_pad=32, cout=32, layout="hwdc", tag="vol", other=("vol32",))
case(12, 32, STD, 3, cin=32, form="f16", **VV)
case(12, 32, STD, 3, cin=32, form="res32_o1", **VV)
case(12, 32, STDSTAT, 3, cin=32, form="stat32", **VV)
case(12, 32, STDSTAT, 3, cin=96, form="hilo_stat", **VV)


def rows():
    return sorted({c["row"] for c in CASES})
