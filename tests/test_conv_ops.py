"""Op-level tests of the conv kernels the dispatcher (csrc/conv_plan.cpp) can choose, except the
stride-1 3x3 family and the fused ResBlock, which tests/test_conv3x3_ops.py covers with this file's
helpers and method: the 1x1 GEMM family (conv2_kernel: forced tile configurations, minimal /
general / swapped / GEGLU epilogues, ring depths, partial M and N tiles, two sources), 1x1 and 3x3
split-K with conv_part_reduce, conv_down (4x4 stride 2), conv7 and conv3n (conv_edge.hip, plain and
split-precision weights), their generic fallbacks (v2 row-tap 7x7, v2 kh = 4, conv1, the 256x16 v4
tile), fp32 instantiations, and the plain up = 1 3x3 conv -- each as ONE launch through the C ABI
hook dac_op_conv, against a torch float64 reference written from the definition in kernels.h:

    y[m, n] = epi(sum_k A[m, k] W[n, k]),  m = (b, oh, ow),  k = (kh, kw, ci)
    A: zero padding, nearest 2x for up; channels [0, C1) from x1, the rest from x2
    epi: +bias -> *(1 + scale) + shift -> act -> +res1 -> +res2 -> +bbias;  GEGLU: x * gelu_erf(gate)

The reference works on the exactly representable operands (inputs, weights and residuals rounded
to T first; split-precision weights are hi + lo). The weight packers of csrc/pack.h (plain
[O][kh][kw][Cin], the 7x7 row-tap layout, conv_dual's two layouts, geglu's two row orders) are
re-implemented here; CPU tests unpack each, and check that the literal packed-K GEMM over the
arrays handed to the hook (pitches, packed weights, ConvArgs fields) equals the reference.

Tolerances are not taken from the kernel. err = max|y - ref64| / max|ref64| per image. The rounding
model is the same operation in torch float32 with the epilogue in fp32, rounded to T once at the
output. 16-bit bound: 4 x the model's err, floor 2 ulp of T at max|ref|. fp32 bound: 4 x the float32
model's own err. GELU / GEGLU cases add gelu_fast's documented bound (common.h: |erf error| <=
1.5e-7, i.e. 0.75e-7 |u|). Split-precision cases also bound the mean signed (y - ref) / max|ref|
(inputs positive, every weight's rounding error positive, so a dropped lo part is systematic):
4 x the model's value, floor 4 ulp / sqrt(12 N) for N outputs per image.

The CPU precondition test covers every case: each applicable reference-level mutant (a padding
column replicated, the last K tile dropped, a split-K partial dropped, x2 shifted by one 8-channel
vector, GEGLU gate shifted by 16 channels, lo weights dropped, res2 omitted, another image's
scale / shift / bbias, output rows shifted by one row width) must move the metric by more than
10 x the case's bound; borders are loud (outer pixel ring x 4, last K tile scaled up). The CPU
coverage test asserts through the hook's plan-only mode (no GPU) the kernel kind, tile, ring depth
and epilogue every case selects. Every GPU case runs with 256 guard columns and 256 guard rows of
a sentinel around y (and slack rows after every input) that must come back bit-unchanged, and
asserts that the executed plan is the planned one.

Measured on an MI355X (the largest over a family's cases and images; kernel/bound is the largest ratio of a
case's error to its own bound, 1.0 = at the bound; every test prints its case's figures). No case exceeded
its bound, no guard band was touched and no kernel needed a change; the hook's refusal tests made conv_plan
refuse 7x7 row-tap layouts (K = 7 x 8 x Cin or cwrap = 1) that neither conv7 nor the v2 row-tap tile takes,
which it used to plan onto generic kernels that read K as [7][7][Cin]. Model and kernel agree to three
digits in 16 bits: the largest error is then the final rounding of y to T near max|ref|, which both share.
_fb: the generic fallbacks; 1x1_two: two sources (the signed columns: split-precision over both).
Arithmetic-only mutants of the kernels, built aside and run once against these tests, failed exactly the
cases that reach them and no other: conv_part_reduce leaving out the last partial (every split1 / split3
case), conv7 and conv3n dropping the lo weights (every split-precision case of each, through the signed
bound), conv_down's tap 3 reading tap 1's pixel (every conv_down case), the swapped GEGLU epilogue pairing x
with the next channel's gate (the eight w_gs cases on swapped tiles of each dtype).

family     type cases |    model   kernel kernel/bound | signed:    model   kernel kernel/bound
down       bf16    48 |  3.4e-03  3.4e-03         0.25 |                -        -            -
down_fb    bf16     1 |  3.0e-03  3.0e-03         0.25 |                -        -            -
conv7      bf16    32 |  3.4e-03  3.4e-03         0.25 |          5.6e-05  5.6e-05         0.18
conv7_fb   bf16     1 |  3.3e-03  3.3e-03         0.25 |                -        -            -
conv3n     bf16    36 |  3.1e-03  3.1e-03         0.25 |          2.1e-05  2.1e-05         0.09
conv3n_fb  bf16     2 |  3.1e-03  3.1e-03         0.23 |                -        -            -
1x1_forced bf16    40 |  3.1e-03  3.1e-03         0.25 |                -        -            -
1x1        bf16    27 |  3.6e-03  3.6e-03         0.25 |                -        -            -
1x1_two    bf16     4 |  3.7e-03  3.7e-03         0.25 |          1.1e-06  1.1e-06         0.02
geglu      bf16    13 |  3.3e-03  3.3e-03         0.25 |                -        -            -
split1     bf16    12 |  3.5e-03  3.5e-03         0.25 |                -        -            -
split3     bf16     9 |  3.5e-03  3.5e-03         0.25 |                -        -            -
up3        bf16     8 |  3.7e-03  3.7e-03         0.25 |                -        -            -
down       fp16    48 |  4.5e-04  4.5e-04         0.25 |                -        -            -
down_fb    fp16     1 |  3.7e-04  3.7e-04         0.24 |                -        -            -
conv7      fp16    32 |  4.5e-04  4.5e-04         0.25 |          1.4e-06  1.4e-06         0.07
conv7_fb   fp16     1 |  4.1e-04  4.1e-04         0.24 |                -        -            -
conv3n     fp16    36 |  3.8e-04  3.8e-04         0.25 |          5.9e-06  5.9e-06         0.15
conv3n_fb  fp16     2 |  3.0e-04  3.0e-04         0.25 |                -        -            -
1x1_forced fp16    40 |  3.9e-04  3.9e-04         0.25 |                -        -            -
1x1        fp16    27 |  4.6e-04  4.6e-04         0.25 |                -        -            -
1x1_two    fp16     4 |  4.2e-04  4.2e-04         0.25 |          5.1e-07  5.2e-07         0.11
geglu      fp16    13 |  3.7e-04  3.7e-04         0.25 |                -        -            -
split1     fp16    12 |  4.7e-04  4.7e-04         0.25 |                -        -            -
split3     fp16     9 |  3.7e-04  3.7e-04         0.25 |                -        -            -
up3        fp16     8 |  4.7e-04  4.7e-04         0.25 |                -        -            -
down_fb    fp32     1 |  5.3e-07  6.2e-07         0.29 |                -        -            -
conv7_fb   fp32     1 |  2.2e-07  2.0e-07         0.22 |                -        -            -
conv3n_fb  fp32     1 |  3.5e-07  5.2e-07         0.37 |                -        -            -
1x1        fp32     3 |  2.5e-07  2.6e-07         0.31 |                -        -            -
"""
import ctypes
import functools
import math
import zlib
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MANT = {"bf16": 7, "fp16": 10, "fp32": 23}
H16 = ("bf16", "fp16")
KINDS = ["none", "conv7", "conv3n", "conv_down", "conv3r", "conv3w", "conv3i", "conv3", "conv3_split", "conv2",
         "conv2_split", "conv1"]
MIN, ALL, GEGLU_LDS, SWAP, PART = 0, 15, 2, 32, 256        # conv_plan.h EPI_* values
NONE, SILU, GELU, GEGLU = 0, 1, 2, 3
STRIDE = {1: 1, 3: 1, 4: 2, 7: 1}
PAD = {1: 0, 3: 1, 4: 1, 7: 3}
GUARD = 256


# ------------------------------------------------------------------ cases
def mk(fam, dt, kh, B, H, W, C, Cout, want, **kw):
    """One launch. C: logical input channels; C1 < C: two sources; dual: split-precision weights;
    rowtap: the 7x7 layout with kw padded to 8; gs: GEGLU (None: not one; False: only the
    interleaved order exists; True: w_gs / b_gs too); ks: split-K; f3 / f2 / f32: the knobs."""
    c = SimpleNamespace(fam=fam, dt=dt, kh=kh, B=B, H=H, W=W, C=C, Cout=Cout, want=want, up=0, C1=C, dual=False,
                        rowtap=False, act=NONE, bias=False, ss=False, res1=False, res2=False, bbias=False, ks=0,
                        f3=-1, f2=0, f32=18, gs=None)
    c.__dict__.update(kw)
    c.key = (f"{fam}-k{kh}-B{B}-{H}x{W}{'^' if c.up else ''}-C{C}{'+' if c.C1 < C else ''}{'d' if c.dual else ''}"
             f"-O{Cout}-a{c.act}{'b' if c.bias else ''}{'s' if c.ss else ''}{'r' if c.res1 else ''}"
             f"{'R' if c.res2 else ''}{'p' if c.bbias else ''}-ks{c.ks}-f{c.f3}.{c.f2}.{c.f32}"
             f"{'' if c.gs is None else '-gs' + str(int(c.gs))}")
    c.id = f"{dt}-{c.key}"
    return c


EPI4 = [dict(), dict(bias=True, act=SILU), dict(ss=True, res1=True), dict(res1=True, res2=True)]
EPI5 = [dict(bias=True), dict(bias=True, act=GELU), dict(ss=True, act=SILU), dict(res1=True, res2=True),
        dict(bbias=True)]
F2 = {1: (256, 128, 3), 2: (128, 128, 2), 3: (256, 128, 2), 4: (128, 128, 3), 5: (256, 256, 2), 6: (128, 256, 2),
      7: (128, 64, 2), 8: (64, 128, 2), 9: (64, 64, 3), 10: (128, 64, 3), 11: (64, 128, 3), 12: (64, 128, 4),
      13: (64, 128, 3)}
F2SW = {14: (128, 128, 2), 15: (128, 128, 3), 16: (64, 128, 4), 17: (64, 128, 6), 18: (128, 128, 4), 19: (128, 128, 5)}
R77, R64, R256, R50 = (7, 11), (8, 8), (16, 16), (5, 10)


def build_cases():
    cs = []
    own = lambda k: (k, 0, 0, 0, 0)
    for dt in H16:
        # conv_down: row tiles of 4 / 2 / 1 output rows, two segments per row; one, even, odd chunk counts.
        n = 0
        for (H, W) in ((8, 64), (4, 128), (2, 256), (2, 512)):
            for C in (32, 64, 96):
                for e in EPI4:
                    cs.append(mk("down", dt, 4, 2, H, W, C, (64, 128)[(n // 4 + n) % 2], own("conv_down"), **e))
                    n += 1
        cs.append(mk("down_fb", dt, 4, 2, 32, 32, 64, 64, ("conv2", 256, 64, 3, MIN), bias=True, act=SILU))
        # conv7: one tile in total, 18 tiles, a second segment 8 wide, a ragged segment.
        n = 0
        for (H, W) in ((1, 8), (9, 256), (3, 264), (2, 300)):
            for B in (1, 2):
                for dual in (False, True):
                    for bias in (False, True):
                        cs.append(mk("conv7", dt, 7, B, H, W, 8, 64, own("conv7"), dual=dual, rowtap=True, bias=bias))
        cs.append(mk("conv7_fb", dt, 7, 2, 3, 264, 8, 64, ("conv2", 256, 64, 3, ALL), rowtap=True, res1=True))
        # conv3n: 1 / 3 / 6 / 8 tiles (fewer than ring slots and than XCD bands, and exactly 8).
        for (H, W) in ((4, 64), (8, 128), (12, 64)):
            for B in (1, 2):
                for Cout in (1, 3, 4):
                    for dual in (False, True):
                        cs.append(mk("conv3n", dt, 3, B, H, W, 64, Cout, own("conv3n"), dual=dual, bias=n % 2 == 0))
                        n += 1
        cs.append(mk("conv3n_fb", dt, 3, 2, 8, 32, 64, 3, ("conv1", 256, 16, 1, ALL), bias=True))
        cs.append(mk("conv3n_fb", dt, 3, 2, 4, 64, 64, 3, ("conv3i", 256, 16, 2, ALL), bias=True, res1=True))
        # 1x1: every forced configuration at an aligned shape (through conv2_force32, K loop of 2
        # tiles) and at a ragged one (through conv2_force: tiles straddle images, partial M and N).
        for k in range(20):
            al = (F2[k] + (MIN,)) if 1 <= k <= 12 else (64, 128, 3, SWAP) if k == 13 else \
                 (F2SW[k] + (SWAP,)) if k >= 14 else (64, 128, 2, SWAP)
            rg = (F2[k] + (MIN if k == 5 else ALL,)) if 1 <= k <= 13 else (64, 128, 2, ALL)
            cs.append(mk("1x1_forced", dt, 1, 2, *R256, 128, 128, ("conv2",) + al, ss=True, act=SILU, f32=k))
            cs.append(mk("1x1_forced", dt, 1, 2, *R77, 192, 192, ("conv2",) + rg, bias=True, res1=True, f2=k, f32=0))
        for e in EPI5:
            mn = e.get("act", NONE) != GELU
            cs.append(mk("1x1", dt, 1, 2, *R77, 128, 192, ("conv2", 64, 128, 2, ALL), **e))
            cs.append(mk("1x1", dt, 1, 2, *R77, 128, 128, ("conv2", 64, 128, 2, ALL), **e))
            cs.append(mk("1x1", dt, 1, 2, *R64, 128, 192, ("conv2", 64, 128, 2, MIN if mn else ALL), **e))
            cs.append(mk("1x1", dt, 1, 2, *R64, 128, 128, ("conv2", 64, 128, 2, SWAP if mn else ALL), **e))
        cs.append(mk("1x1", dt, 1, 2, *R77, 64, 128, ("conv2", 128, 64, 1, ALL), bias=True))
        cs.append(mk("1x1", dt, 1, 2, *R256, 64, 64, ("conv2", 128, 64, 1, MIN), ss=True, act=SILU, f32=0))
        cs.append(mk("1x1", dt, 1, 2, *R77, 2048, 64, ("conv2", 128, 64, 2, ALL), bias=True, act=GELU))
        cs.append(mk("1x1", dt, 1, 2, *R256, 2048, 1152, ("conv2", 256, 256, 2, MIN), res1=True, res2=True, f32=0))
        cs.append(mk("1x1", dt, 1, 2, *R256, 128, 384, ("conv2", 128, 128, 4, SWAP), bias=True))
        cs.append(mk("1x1", dt, 1, 2, *R256, 128, 192, ("conv2", 64, 128, 2, MIN), bbias=True))
        cs.append(mk("1x1", dt, 1, 2, *R64, 192, 1152, ("conv2", 64, 128, 2, SWAP), bias=True))
        cs.append(mk("1x1_two", dt, 1, 2, *R77, 128, 128, ("conv2", 64, 128, 2, ALL), C1=64, bias=True))
        cs.append(mk("1x1_two", dt, 1, 2, *R64, 128, 128, ("conv2", 64, 128, 2, SWAP), C1=64, ss=True, act=SILU))
        # ... and with split-precision weights over both sources (cwrap = C: [x1 | x2 | x1 | x2]).
        cs.append(mk("1x1_two", dt, 1, 2, *R77, 128, 64, ("conv2", 128, 64, 2, ALL), C1=64, dual=True, bias=True))
        cs.append(mk("1x1_two", dt, 1, 2, *R256, 128, 64, ("conv2", 64, 128, 2, MIN), C1=64, dual=True))
        # GEGLU: interleaved order on the LDS-epilogue tiles, w_gs order on the four swapped sizes.
        for (I, Fo) in ((256, 256), (128, 128)):
            g = dict(act=GEGLU, bias=True)
            cs.append(mk("geglu", dt, 1, 2, *R256, I, 2 * Fo, ("conv2", 256, 256, 2, GEGLU_LDS), gs=False, **g))
            cs.append(mk("geglu", dt, 1, 2, *R256, I, 2 * Fo, ("conv2", 128, 256, 2, ALL), gs=False, f2=6, **g))
            for f, (BM, BN) in ((20, (256, 256)), (21, (128, 256)), (22, (256, 128)), (23, (128, 128))):
                cs.append(mk("geglu", dt, 1, 2, *R256, I, 2 * Fo, ("conv2", BM, BN, 2, SWAP | GEGLU_LDS), gs=True, f2=f, **g))
        cs.append(mk("geglu", dt, 1, 2, *R77, 128, 256, ("conv2", 128, 256, 2, ALL), gs=True, act=GEGLU, bias=True))
        # 1x1 split-K: 8 / 16 K tiles over 2, 3 (uneven) and 8 splits.
        n = 0
        for ks in (2, 3, 8):
            for K in (512, 1024):
                for (B, R) in ((2, R77), (1, R50)):
                    e = (dict(bias=True, act=GELU), dict(res1=True, res2=True))[n % 2]
                    cs.append(mk("split1", dt, 1, B, *R, K, (128, 192)[(n // 2) % 2], ("conv2_split", 64, 128, 2, PART),
                                 ks=ks, **e))
                    n += 1
        # 3x3 split-K over Cin ranges (4 chunks of 64 channels: two per split, one per split).
        for (H, W) in ((16, 16), (32, 32)):
            for ks in (2, 4):
                for e in (dict(ss=True, act=SILU), dict(res1=True)):
                    cs.append(mk("split3", dt, 3, 2, H, W, 256, 128, ("conv3_split", 128, 128, 2, MIN), ks=ks, **e))
        cs.append(mk("split3", dt, 3, 2, 16, 16, 256, 128, ("conv3_split", 128, 128, 2, MIN), ks=2, C1=128, bias=True))
        # Plain up = 1 3x3: the built-in choice and v3.
        for (H, W) in ((8, 8), (16, 16)):
            for C in (64, 128):
                built = ("conv3", 128, 64, 2, MIN) if W == 8 else ("conv3i", 128, 64, 3, MIN)
                cs.append(mk("up3", dt, 3, 2, H, W, C, 64, built, up=1, bias=True))
                cs.append(mk("up3", dt, 3, 2, H, W, C, 64, ("conv3", 128, 64, 2, MIN), up=1, bias=True, f3=0))
    # fp32 instantiations.
    cs.append(mk("down_fb", "fp32", 4, 2, 8, 64, 32, 64, ("conv2", 256, 64, 3, ALL), bias=True, act=SILU))
    cs.append(mk("conv7_fb", "fp32", 7, 2, 3, 264, 8, 64, ("conv1", 256, 64, 1, ALL), bias=True))
    cs.append(mk("conv3n_fb", "fp32", 3, 2, 4, 64, 64, 3, ("conv3i", 256, 16, 2, ALL), bias=True))
    cs.append(mk("1x1", "fp32", 1, 2, *R77, 32, 128, ("conv2", 128, 64, 1, ALL), bias=True, act=GELU))
    cs.append(mk("1x1", "fp32", 1, 2, *R77, 96, 192, ("conv2", 64, 128, 2, ALL), ss=True, act=SILU, res1=True))
    cs.append(mk("1x1", "fp32", 1, 2, *R77, 96, 64, ("conv2", 128, 64, 2, ALL), res1=True, res2=True))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = build_cases()
FAMILIES = sorted({c.fam for c in CASES})


# ------------------------------------------------------------------ packers (csrc/pack.h; pinned to it by test_pack.py)
def pack_plain(W):
    """[O][C][kh][kw] -> [O][kh][kw][C] as [O, K]."""
    return W.permute(0, 2, 3, 1).reshape(W.shape[0], -1)


def unpack_plain(P, C, kh):
    return P.reshape(P.shape[0], kh, kh, C).permute(0, 3, 1, 2)


def pack_rowtap(parts):
    """7x7, C = 8: each part [O][8][7][7] -> [O][7 rows][8 taps][8 ch] with a zero tap 7; parts side by side
    ([hi rows | lo rows])."""
    out = []
    for W in parts:
        P = torch.zeros(W.shape[0], 7, 8, 8, dtype=W.dtype)
        P[:, :, :7, :] = W.permute(0, 2, 3, 1)
        out.append(P.reshape(W.shape[0], 448))
    return torch.cat(out, 1)


def unpack_rowtap(P, nparts):
    return [P[:, 448 * i:448 * (i + 1)].reshape(-1, 7, 8, 8)[:, :, :7, :].permute(0, 3, 1, 2) for i in range(nparts)]


def pack_dual_tap(hi, lo):
    """[O][tap][hi C | lo C] (conv_dual without a padded kernel row)."""
    O, C, kh, kw = hi.shape
    return torch.cat([hi.permute(0, 2, 3, 1), lo.permute(0, 2, 3, 1)], -1).reshape(O, kh * kw * 2 * C)


def unpack_dual_tap(P, C, kh):
    t = P.reshape(P.shape[0], kh, kh, 2, C)
    return t[:, :, :, 0].permute(0, 3, 1, 2), t[:, :, :, 1].permute(0, 3, 1, 2)


def geglu_rows(Fo):
    """Source row of each packed row r: 32-row groups of 16 x rows then their 16 gate rows."""
    r = torch.arange(2 * Fo)
    g, s = r // 32, r % 32
    return torch.where(s < 16, 16 * g + s, Fo + 16 * g + (s - 16))


def geglu_gs_rows(Fo):
    """The swapped-tile order: row L of 64-row group G, lane group lg, e = L % 16 is x (e < 8) or gate of
    output channel 32 G + 8 lg + (e & 7)."""
    L = torch.arange(2 * Fo)
    G, lg, e = L // 64, (L % 64) // 16, L % 16
    return torch.where(e < 8, 0, Fo) + 32 * G + 8 * lg + (e & 7)


def test_packers_round_trip():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(5, 16, 3, 3, generator=g, dtype=torch.float64)
    P = pack_plain(W)
    assert P[2, (1 * 3 + 2) * 16 + 7] == W[2, 7, 1, 2] and torch.equal(unpack_plain(P, 16, 3), W)
    hi, lo = torch.randn(4, 8, 7, 7, generator=g), torch.randn(4, 8, 7, 7, generator=g)
    P = pack_rowtap([hi, lo])
    assert P.shape == (4, 896) and P[1, 448 + (3 * 8 + 5) * 8 + 2] == lo[1, 2, 3, 5]
    assert (P.reshape(4, 2, 7, 8, 8)[:, :, :, 7] == 0).all()
    u = unpack_rowtap(P, 2)
    assert torch.equal(u[0], hi) and torch.equal(u[1], lo)
    hi, lo = torch.randn(3, 64, 3, 3, generator=g), torch.randn(3, 64, 3, 3, generator=g)
    P = pack_dual_tap(hi, lo)
    assert P[2, (2 * 3 + 1) * 128 + 64 + 9] == lo[2, 9, 2, 1] and P[2, (2 * 3 + 1) * 128 + 9] == hi[2, 9, 2, 1]
    u = unpack_dual_tap(P, 64, 3)
    assert torch.equal(u[0], hi) and torch.equal(u[1], lo)
    for Fo in (128, 256):
        for rows in (geglu_rows(Fo), geglu_gs_rows(Fo)):
            assert sorted(rows.tolist()) == list(range(2 * Fo))            # a permutation
        r = geglu_rows(Fo)
        assert r[0] == 0 and r[15] == 15 and r[16] == Fo and r[31] == Fo + 15 and r[32] == 16
        q = geglu_gs_rows(Fo)
        assert q[0] == 0 and q[7] == 7 and q[8] == Fo and q[15] == Fo + 7 and q[16] == 8 and q[64] == 32
        Wl = torch.randn(2 * Fo, 4, generator=g)
        for rows in (r, q):
            back = torch.empty_like(Wl)
            back[rows] = Wl[rows]
            assert torch.equal(back, Wl)


# ------------------------------------------------------------------ data, reference, model
def bke(c):
    return 32 if c.dt == "fp32" else 64


def out_hw(c):
    s, p = STRIDE[c.kh], PAD[c.kh]
    Hin, Win = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    return (Hin + 2 * p - c.kh) // s + 1, (Win + 2 * p - c.kh) // s + 1


def last_tile(c):
    """[start, end) of the "last K tile" in the flat [kh][kw][C] order: the bke(c) entries ending with the last
    tap that reads a real pixel (a one-row image never reaches the bottom kernel rows)."""
    Hin, Win = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    r, t = min(c.kh - 1, Hin - 1 + PAD[c.kh]), min(c.kh - 1, Win - 1 + PAD[c.kh])
    end = ((r * c.kh + t) + 1) * c.C
    return max(0, end - bke(c)), end


def conv_acc(c, X, W, mut=None):
    """X [B, H, W, C], W [O, C, kh, kw] (one dtype) -> [B, Ho * Wo, O]; mut 'pad': the padding line next to
    the image's longer edge (the row above it, or the column left of a tall image) repeats the image's
    first line instead of zero."""
    x = X.permute(0, 3, 1, 2)
    if c.up:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    p = PAD[c.kh]
    x = F.pad(x, (p, p, p, p))
    if mut == "pad" and out_hw(c)[1] >= out_hw(c)[0]:
        x[..., p - 1, :] = x[..., p, :]
    elif mut == "pad":
        x[..., :, p - 1] = x[..., :, p]
    y = F.conv2d(x, W, stride=STRIDE[c.kh])
    return y.permute(0, 2, 3, 1).reshape(X.shape[0], -1, W.shape[0])


def gelu_erf(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def epilogue(c, d, acc, dtype, mut=None):
    """acc [B, HW, O] -> [B, HW, Cy] in `dtype` arithmetic, the order of kernels.h."""
    B = acc.shape[0]
    cv = lambda t: t.to(dtype)
    v = acc
    if c.bias:
        v = v + cv(d.bias)
    if c.act == GEGLU:
        Fo = c.Cout // 2
        gate = v[..., Fo:]
        if mut == "geglu16":
            gate = torch.roll(gate, 16, -1)
        return v[..., :Fo] * gelu_erf(gate)
    roll = (lambda t: torch.roll(t, 1, 0)) if mut == "imgterm" else (lambda t: t)
    if c.ss:
        ss = roll(cv(d.ss))
        v = v * (1.0 + ss[:, None, :c.Cout]) + ss[:, None, c.Cout:]
    if c.act == SILU:
        v = v * torch.sigmoid(v)
    elif c.act == GELU:
        v = gelu_erf(v)
    if c.res1:
        v = v + cv(d.res1).reshape(B, -1, c.Cout)
    if c.res2 and mut != "res2":
        v = v + cv(d.res2).reshape(B, -1, c.Cout)
    if c.bbias:
        v = v + roll(cv(d.bbias))[:, None, :]
    return v


def row_width(c):
    Ho, Wo = out_hw(c)
    rw = Wo if c.kh > 1 else 16
    M = c.B * Ho * Wo
    return rw if rw < M else M // 2


def mutated(c, d, mut):
    """X, W of a reference-level mutant (the others act in conv_acc / epilogue / on the result)."""
    X, W = d.Xq, d.Wq
    if mut == "ktile":
        Wk = pack_plain(W).clone()
        Wk[:, slice(*last_tile(c))] = 0
        W = unpack_plain(Wk, c.C, c.kh)
    elif mut == "split":
        nch = c.C // bke(c)
        W = W.clone()
        W[:, (c.ks - 1) * nch // c.ks * bke(c):] = 0
    elif mut == "x2shift":
        X = torch.cat([X[..., :c.C1], torch.roll(X[..., c.C1:], 8, -1)], -1)
    elif mut == "lo":
        W = d.hi
    return X, W


def reference(c, d, mut=None):
    X, W = mutated(c, d, mut)
    y = epilogue(c, d, conv_acc(c, X, W, mut), torch.float64, mut)
    if mut == "rowshift":
        y = torch.roll(y.reshape(-1, y.shape[-1]), row_width(c), 0).reshape(y.shape)
    return y


def mutants(c):
    m = ["ktile", "rowshift"]
    if c.kh > 1:
        m.append("pad")
    if c.ks > 1:
        m.append("split")
    if c.C1 < c.C:
        m.append("x2shift")
    if c.act == GEGLU:
        m.append("geglu16")
    if c.res2:
        m.append("res2")
    if (c.ss or c.bbias) and c.B > 1:
        m.append("imgterm")
    return m


def rel_err(a, ref):
    B = ref.shape[0]
    d = (a.double() - ref).abs().reshape(B, -1).max(dim=1).values
    return (d / ref.abs().reshape(B, -1).max(dim=1).values).tolist()


def mean_signed(a, ref):
    B = ref.shape[0]
    return ((a.double() - ref).reshape(B, -1).mean(dim=1) / ref.abs().reshape(B, -1).max(dim=1).values).tolist()


def ulp_rel(dt, m):
    return 2.0 ** (math.floor(math.log2(m)) - MANT[dt]) / m


def layout(c):
    """Sizes, pitches and which operands exist (1 / None placeholders; make() puts the tensors there)."""
    Ho, Wo = out_hw(c)
    Cy = c.Cout // 2 if c.act == GEGLU else c.Cout
    on = lambda f: 1 if f else None
    return SimpleNamespace(Ho=Ho, Wo=Wo, M=c.B * Ho * Wo, Cy=Cy, ld1=c.C1, ld2=(c.C - c.C1 + 8 if c.C1 < c.C else 0),
                           ldr1=Cy + 8, ldr2=Cy + 16, ss_ld=2 * c.Cout, bb_ld=Cy + 4, ldy=Cy + GUARD, x1=1,
                           x2=on(c.C1 < c.C), wp=1, bp=on(c.bias), ss=on(c.ss), res1=on(c.res1), res2=on(c.res2),
                           bbias=on(c.bbias), w_gs=on(c.gs), b_gs=on(c.gs))


@functools.lru_cache(maxsize=8)
def make(c_id):
    """Operands of a case in T (as fp64 values and as the packed / pitched arrays the hook gets), the fp64
    reference, the rounding model's errors and the bounds. The random draws do not depend on the dtype."""
    c = BY_ID[c_id]
    T = TDT[c.dt]
    g = torch.Generator().manual_seed(zlib.crc32(c.key.encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q = lambda t: t.to(T).double()
    B, H, W, C, O, kh = c.B, c.H, c.W, c.C, c.Cout, c.kh
    Ho, Wo = out_hw(c)
    d = layout(c)
    M, Cy = d.M, d.Cy
    X = rn(B, H, W, C)
    if c.dual:
        X = X.abs() + 0.25
    if kh > 1:                                            # loud outermost pixel ring
        ring = torch.zeros(H, W, dtype=torch.float64)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = 1, 1, 1, 1
        X = X * (1.0 + 3.0 * ring)[None, :, :, None]
    K = kh * kh * C
    Wk = rn(O, K) / math.sqrt(K)
    nk = (K + bke(c) - 1) // bke(c)
    Wk[:, slice(*last_tile(c))] *= 2.0 * math.sqrt(max(nk - 1, 1))     # loud last K tile (and last channel chunk)
    Wf = unpack_plain(Wk, C, kh).contiguous()
    d.Xq = q(X)
    if c.dual:
        # hi = RNE(w), lo = RNE(w - hi) with w = hi + 3/8 ulp(hi): every rounding error positive.
        Wf = torch.where(Wf.abs() < 2.0 ** -8, torch.copysign(torch.full_like(Wf, 2.0 ** -8), Wf), Wf)
        d.hi = q(Wf)
        pw = torch.exp2(torch.floor(torch.log2(d.hi.abs())))
        # (a negative power of two has the finer spacing on the side the error moves it to)
        d.lo = 0.375 * pw * 2.0 ** -MANT[c.dt] * torch.where((d.hi < 0) & (d.hi.abs() == pw), 0.5, 1.0)
        d.Wq = d.hi + d.lo
        assert torch.equal(q(d.Wq), d.hi) and torch.equal(q(d.lo), d.lo)
    else:
        d.Wq = q(Wf)
        d.hi = d.Wq
    acc = conv_acc(c, d.Xq, d.Wq)
    s0 = acc.std().item()
    r_bias, r_ss, r_r1, r_r2, r_bb = rn(O), rn(B, 2 * O), rn(M, Cy), rn(M, Cy), rn(B, Cy)
    d.bias = (0.5 * s0 * r_bias).float() if c.bias else None
    d.ss = torch.cat([0.5 * r_ss[:, :O], s0 * r_ss[:, O:]], 1).float() if c.ss else None
    sr = s0 * (1.0 if c.act != SILU else 0.5)
    d.res1 = q(sr * r_r1).to(T) if c.res1 else None
    d.res2 = q(sr * r_r2).to(T) if c.res2 else None
    d.bbias = (sr * r_bb).float() if c.bbias else None
    d.ref = epilogue(c, d, acc, torch.float64)
    assert torch.isfinite(d.ref).all()
    # The rounding model: float32 throughout, rounded to T once.
    model = epilogue(c, d, conv_acc(c, d.Xq.float(), d.Wq.float()), torch.float32).to(T)
    d.model_err = rel_err(model, d.ref)
    mx = d.ref.abs().reshape(B, -1).max(dim=1).values.tolist()
    gel = [0.0] * B
    if c.act in (GELU, GEGLU):
        u = acc + (d.bias.double() if c.bias else 0.0)
        if c.act == GEGLU:
            gterm = (u[..., :Cy].abs() * u[..., Cy:].abs()).reshape(B, -1).max(dim=1).values
        else:
            gterm = u.abs().reshape(B, -1).max(dim=1).values
        gel = [0.75e-7 * t / m for t, m in zip(gterm.tolist(), mx)]
    if c.dt == "fp32":
        d.tol = [4.0 * e + ge for e, ge in zip(d.model_err, gel)]
    else:
        d.tol = [max(4.0 * e, 2.0 * ulp_rel(c.dt, m)) + ge for e, m, ge in zip(d.model_err, mx, gel)]
    if c.dual:
        d.model_sys = mean_signed(model, d.ref)
        n_out = Ho * Wo * Cy
        d.tol_sys = [max(4.0 * abs(s), 4.0 * ulp_rel(c.dt, m) / math.sqrt(12.0 * n_out)) for s, m in zip(d.model_sys, mx)]
    # What the hook gets.
    if c.rowtap and c.dt != "fp32":
        d.wp = pack_rowtap([d.hi, d.lo] if c.dual else [d.Wq]).to(T)
    elif c.dual:
        d.wp = pack_dual_tap(d.hi, d.lo).to(T)
    else:
        d.wp = pack_plain(d.Wq).to(T)
    d.bp, d.w_gs, d.b_gs = d.bias, None, None
    if c.act == GEGLU:
        r = geglu_rows(Cy)
        d.wp, d.bp = d.wp[r].contiguous(), d.bias[r].contiguous()
        if c.gs:
            r = geglu_gs_rows(Cy)
            d.w_gs, d.b_gs = pack_plain(d.Wq).to(T)[r].contiguous(), d.bias[r].contiguous()
    C1 = c.C1
    d.x1 = d.Xq[..., :C1].reshape(-1, C1).to(T)
    d.x2 = None
    if C1 < C:
        d.x2 = torch.full((B * H * W, d.ld2), 1000.0, dtype=T)
        d.x2[:, :C - C1] = d.Xq[..., C1:].reshape(-1, C - C1).to(T)
    return d


def descriptor(c, d):
    from daclip_amd import _lib
    Cin, C1, ld2, K, cwrap = c.C, c.C1, d.ld2, c.kh * c.kh * c.C, 0
    if c.rowtap and c.dt != "fp32":
        K, cwrap = (896, 1) if c.dual else (448, 0)
    elif c.dual and c.C1 < c.C:                           # two sources read twice: channel ci >= cwrap wraps
        Cin, K, cwrap = 2 * c.C, 2 * K, c.C
    elif c.dual:                                          # the input read twice through x2 = x1
        Cin, ld2, K = 2 * c.C, d.ld1, 2 * K
    code = {"bf16": _lib.DAC_BF16, "fp16": _lib.DAC_F16, "fp32": _lib.DAC_F32}[c.dt]
    return _lib.DacConvDesc(dtype=code, kh=c.kh, B=c.B, Hs=c.H, Ws=c.W, up=c.up, C1=C1, Cin=Cin, ld1=d.ld1, ld2=ld2,
                            Cout=c.Cout, K=K, ldy=d.ldy, act=c.act, cwrap=cwrap, ksplit=c.ks, ss_ld=d.ss_ld,
                            ldr1=d.ldr1, ldr2=d.ldr2, bb_ld=d.bb_ld, conv3_force=c.f3, conv2_force=c.f2,
                            conv2_force32=c.f32)


BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------ CPU: the definition, literally
def definition(c, d):
    """The packed-K GEMM of kernels.h over the arrays the hook gets: A gathered tap by tap from x1 / x2 with
    their pitches, W = the packed rows, the epilogue in the packed GEGLU order."""
    ds = descriptor(c, d)
    B, H, W = c.B, c.H, c.W
    x1 = d.x1.double().reshape(B, H, W, ds.ld1)
    x2 = d.x2.double().reshape(B, H, W, ds.ld2) if d.x2 is not None else x1 if (c.dual and not c.rowtap) else None
    chans = []
    for ci in range(ds.Cin):
        ci = ci - ds.cwrap if (ds.cwrap > 1 and ci >= ds.cwrap) else ci
        chans.append(x1[..., ci] if ci < ds.C1 else x2[..., ci - ds.C1])
    X = torch.stack(chans, -1)
    if c.up:
        X = X.repeat_interleave(2, 1).repeat_interleave(2, 2)
    p, s = PAD[c.kh], STRIDE[c.kh]
    Xp = F.pad(X, (0, 0, p, p + 1, p, p))                  # one more column on the right: the zero-weight tap 7
    rowtap = c.rowtap and c.dt != "fp32"
    kws = 8 if rowtap else c.kh
    cols = []
    for part in range(2 if (rowtap and c.dual) else 1):
        for r in range(c.kh):
            for t in range(kws):
                cols.append(Xp[:, r:r + s * (d.Ho - 1) + 1:s, t:t + s * (d.Wo - 1) + 1:s, :])
    A = torch.cat(cols, -1).reshape(B, d.Ho * d.Wo, -1)
    assert A.shape[-1] == ds.K
    outs = []
    for wp, bp, rows in ((d.wp, d.bp, geglu_rows), (d.w_gs, d.b_gs, geglu_gs_rows)):
        if wp is None:
            continue
        acc = A @ wp.double().t()
        if c.act == GEGLU:                                 # back to [x | gate] through the row order
            u = acc + bp.double()
            nat = torch.empty_like(u)
            nat[..., rows(d.Cy)] = u
            outs.append(nat[..., :d.Cy] * gelu_erf(nat[..., d.Cy:]))
        else:
            outs.append(epilogue(c, d, acc, torch.float64))
    return outs


def one_per_variant():
    seen, out = set(), []
    for c in CASES:
        k = (c.fam, c.dt == "fp32", c.dual, c.C1 < c.C, c.gs, c.up, c.ks > 1, c.ss, c.bbias)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def test_reference_matches_definition():
    """The logical reference equals the literal packed-K GEMM over what the hook is handed, for one case of
    every family / layout / feature (so a GPU mismatch is the kernel's, not the test's packing)."""
    for c in one_per_variant():
        d = make(c.id)
        for out in definition(c, d):
            e = max(rel_err(out, d.ref))
            assert e < 1e-12, (c.id, e)


# ------------------------------------------------------------------ CPU: preconditions and sensitivity
@pytest.mark.parametrize("fam", FAMILIES)
def test_preconditions_and_sensitivity(fam):
    """Every case: a finite reference, a sane rounding model, and every reference-level mutant moves the
    metric by more than 10 x the case's bound (in every image)."""
    for c in [c for c in CASES if c.fam == fam]:
        d = make(c.id)
        lim = {"bf16": 0.05, "fp16": 0.01, "fp32": 1e-5}[c.dt]
        assert all(0 < t < lim for t in d.tol), (c.id, d.tol)
        moved = {}
        for mut in mutants(c):
            mv = rel_err(reference(c, d, mut), d.ref)
            moved[mut] = min(mv)
            assert all(m > 10.0 * t for m, t in zip(mv, d.tol)), (c.id, mut, mv, d.tol)
        if c.dual:
            sy = mean_signed(reference(c, d, "lo"), d.ref)
            moved["lo"] = min(abs(s) for s in sy)
            assert all(s < -10.0 * t for s, t in zip(sy, d.tol_sys)), (c.id, "lo", sy, d.tol_sys)
        print(f"{c.id}: model {max(d.model_err):.2e} tol {max(d.tol):.2e} " +
              " ".join(f"{n} {v:.2e}" for n, v in moved.items()))


# ------------------------------------------------------------------ CPU: plan coverage (plan-only mode)
def _have_lib():
    import os
    from daclip_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


def hook(c, d, ptr, y):
    """dac_op_conv with ptr(tensor) for every operand the case has; -> (rc, plan)."""
    from daclip_amd import _lib
    ds = descriptor(c, d)
    plan = (ctypes.c_int * _lib.DAC_CONV_PLAN_N)()
    x2 = d.x1 if (c.dual and not c.rowtap and c.C1 == c.C) else d.x2
    rc = _lib.lib().dac_op_conv(ctypes.byref(ds), ptr(d.x1), ptr(x2), ptr(d.wp), ptr(d.bp), ptr(d.ss), ptr(d.res1),
                                ptr(d.res2), ptr(d.bbias), ptr(d.w_gs), ptr(d.b_gs), y, plan, None)
    return rc, list(plan)


def plan_only(c, d):
    dummy = lambda t: None if t is None else ctypes.c_void_p(1 << 20)
    return hook(c, d, dummy, None)


def plan_key(plan):
    return (KINDS[plan[0]],) + tuple(plan[1:5])


def test_plan_coverage():
    """Which kernel every case selects, proved without a GPU; and every listed family occurs."""
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    bad, seen = [], set()
    for c in CASES:
        rc, plan = plan_only(c, layout(c))
        if rc != 0 or plan_key(plan) != c.want:
            bad.append((c.id, rc, plan_key(plan) if rc == 0 else None, c.want))
            continue
        kind, epi = KINDS[plan[0]], plan[4]
        seen.add((kind, epi) if kind == "conv2" else (kind, plan[1], plan[2]) if kind == "conv3i" else kind)
    assert not bad, bad[:10]
    need = {"conv7", "conv3n", "conv_down", ("conv2", MIN), ("conv2", ALL), ("conv2", SWAP), ("conv2", GEGLU_LDS),
            ("conv2", SWAP | GEGLU_LDS), "conv2_split", "conv3_split", "conv1", ("conv3i", 256, 16)}
    assert need <= seen, need - seen


def test_bad_arguments_are_refused_before_any_device_work():
    """Runs without a GPU: DAC_E_ARG comes from the checks (or from a plan of kind none), ahead of the first
    HIP call; afterwards the process's knobs are what they were."""
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    from daclip_amd import _lib
    L, E = _lib.lib(), _lib.DAC_E_ARG
    p = ctypes.c_void_p(1 << 20)
    plan = (ctypes.c_int * 8)()

    def call(x1=p, x2=None, w=p, y=p, **kw):
        f = dict(dtype=_lib.DAC_BF16, kh=1, B=2, Hs=8, Ws=8, up=0, C1=64, Cin=64, ld1=64, ld2=0, Cout=128, K=64, ldy=128,
                 act=0, cwrap=0, ksplit=0, ss_ld=0, ldr1=0, ldr2=0, bb_ld=0, conv3_force=_lib.DAC_CONV_KEEP,
                 conv2_force=_lib.DAC_CONV_KEEP, conv2_force32=_lib.DAC_CONV_KEEP)
        f.update(kw)
        ds = _lib.DacConvDesc(**f)
        return L.dac_op_conv(ctypes.byref(ds), x1, x2, w, None, None, None, None, None, None, None, y, plan, None)
    assert L.dac_op_conv(None, p, None, p, None, None, None, None, None, None, None, p, plan, None) == E
    assert call(x1=None) == E and call(w=None) == E
    assert call(y=None) == 0 and plan_key(list(plan)) == ("conv2", 128, 64, 1, ALL)
    before = list(plan)
    assert call(y=None, conv2_force=3) == 0 and plan_key(list(plan))[1:4] == (256, 128, 2)
    assert call(y=None) == 0 and list(plan) == before                    # the override did not stick
    for kw in (dict(dtype=_lib.DAC_FP8), dict(dtype=99), dict(kh=2), dict(kh=5), dict(B=0), dict(Hs=0), dict(Ws=-1),
               dict(up=2), dict(up=1), dict(Cout=0), dict(Cin=60, K=60), dict(Cin=0, K=0), dict(K=128), dict(ldy=127),
               dict(act=4), dict(act=-1), dict(act=3, Cout=48), dict(ksplit=-1), dict(C1=32), dict(ld1=63), dict(cwrap=-1),
               dict(C1=32, ld1=32, ld2=16, x2=p), dict(ksplit=2, act=3), dict(kh=4, Hs=7, K=1024),
               dict(kh=7, C1=8, Cin=8, ld1=8, K=896, cwrap=1, dtype=_lib.DAC_F32),
               dict(kh=7, C1=8, Cin=8, ld1=8, K=448, dtype=_lib.DAC_F32)):
        assert call(**kw) == E, kw


# ------------------------------------------------------------------ GPU
def run_gpu(c, d):
    """-> (y [B, HW, Cy] on the CPU, executed plan). Guard rows / columns of y are checked here."""
    from daclip_amd import _lib
    T = TDT[c.dt]
    dev = {}

    def up(t, rows_slack):
        if t is None:
            return None
        if id(t) not in dev:
            t2 = t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t
            if rows_slack and t2.dim() == 2:
                t2 = torch.cat([t2, torch.full((GUARD, t2.shape[1]), 1000.0, dtype=t2.dtype)], 0)
            dev[id(t)] = t2.contiguous().cuda()
        return dev[id(t)]

    def pitched(t, ld):
        if t is None:
            return None
        out = torch.full((t.shape[0], ld), 1000.0, dtype=t.dtype)
        out[:, :t.shape[1]] = t
        return out
    g = SimpleNamespace(**d.__dict__)
    g.res1, g.res2 = pitched(d.res1, d.ldr1), pitched(d.res2, d.ldr2)
    g.bbias = pitched(d.bbias, d.bb_ld)
    slack = {id(t) for t in (g.x1, g.x2, g.res1, g.res2)}
    sentinel = torch.full((d.M + GUARD, d.ldy), -1234.0, dtype=T)
    y = sentinel.cuda()
    ptr = lambda t: None if t is None else ctypes.c_void_p(up(t, id(t) in slack).data_ptr())
    rc, plan = hook(c, g, ptr, ctypes.c_void_p(y.data_ptr()))
    if rc == -5:      # DAC_E_HIP: the context is gone; nothing more may run on this GPU from this process
        pytest.exit(f"{c.id}: HIP error in dac_op_conv", returncode=3)
    assert rc == 0, (c.id, rc)
    torch.cuda.synchronize()
    out = y.cpu()
    keep = torch.ones(d.M + GUARD, d.ldy, dtype=torch.bool)
    # Narrow-output kernels write whole 4-channel groups.
    keep[:d.M, :(d.Cy + 3) // 4 * 4 if d.Cy <= 4 else d.Cy] = False
    bits = lambda t: t.view(torch.int16 if T != torch.float32 else torch.int32)
    assert torch.equal(bits(out)[keep], bits(sentinel)[keep]), (c.id, "guard band written")
    return out[:d.M, :d.Cy].reshape(c.B, -1, d.Cy), plan


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_conv_matches_fp64_reference(cid):
    c = BY_ID[cid]
    d = make(cid)
    rc, planned = plan_only(c, layout(c))
    assert rc == 0 and plan_key(planned) == c.want, (planned, c.want)
    y, executed = run_gpu(c, d)
    assert executed == planned, (executed, planned)
    assert torch.isfinite(y).all()
    err = rel_err(y, d.ref)
    ratio = max(e / t for e, t in zip(err, d.tol))
    line = f"CONV {c.fam} {c.id}: model {max(d.model_err):.2e} kernel {max(err):.2e} kernel/bound {ratio:.2f}"
    ok = all(e <= t for e, t in zip(err, d.tol))
    if c.dual:
        sy = mean_signed(y, d.ref)
        rs = max(abs(s) / t for s, t in zip(sy, d.tol_sys))
        line += f" | signed: model {max(map(abs, d.model_sys)):.2e} kernel {max(map(abs, sy)):.2e} kernel/bound {rs:.2f}"
        ok = ok and all(abs(s) <= t for s, t in zip(sy, d.tol_sys))
    print(line)
    assert ok, line
