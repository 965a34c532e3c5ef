"""Op-level tests of the stride-1 3x3 conv family and the fused ResBlock, by the method of
tests/test_conv_ops.py (whose helpers this file imports): conv3r (register-stationary, csrc/conv3r.hip),
conv3w (weight-stationary), the conv3i v4 row-halo tiles (every forced configuration, the default
selection's branches, the C3I_RES fused second output, the row- and row+column-phase upsample tiles), the
v3 conv3 tiles, and rbfuse (csrc/rbfuse.hip) -- each as ONE launch through the C ABI hooks dac_op_conv_ex /
dac_op_rbfuse, against a torch float64 reference written from the definition in csrc/kernels.h:

    y[m, n]  = epi(sum_k A[m, k] W[n, k]),  m = (b, oh, ow),  k = (kh, kw, ci)      (test_conv_ops.py)
    y2[m, n] = sum_c x[m, c] w2[n, c]                       the fused 1x1 res_conv: centre tap, no epilogue
    uph = 1: output row 2i + a reads source rows i - 1 + a + s (s = 0, 1) with weight row set 2a + s of
             w [Cout][4][3][Cin]; the three column taps run over the upsampled columns
    uph = 2: the columns fold the same way: output column 2j + b reads source columns j - 1 + b + t with
             column set 2b + t of w [Cout][4][4][Cin]
    rbfuse:  h = SiLU(conv(x, w1) (1 + scale) + shift), y = SiLU(conv(h, w2)) + res, res = x (Cin 64) or
             x wr^T (Cin 128); both convs zero-pad, so h is ZERO outside the image

The phase references use the folded weights exactly as packed: dac_op_pack's DAC_PACK_UPH_ROW / _COL output
in T, decoded. A CPU test shows that with unrounded (DAC_F32) packing the phase definition equals the plain
nearest-2x + 3x3 conv to 1e-12, which separates "folded weights rounded once" from kernel error.

Tolerances follow test_conv_ops.py's rule and are never taken from the kernel: err = max|y - ref64| /
max|ref64| per image; the rounding model is the same operation in torch float32, rounded to T once at the
output (rbfuse: block1 in fp32 -> h rounded to T; res_conv in fp32 -> rounded to T; block2 in fp32 +
residual -> rounded once). 16-bit bound: 4 x the model's err, floor 2 ulp of T at max|ref|; fp32 bound:
4 x the float32 model's own err. y and y2 are checked separately, each with its own bound. rbfuse is also
compared bit for bit with the pair of conv launches it replaces (two dac_op_conv_ex calls).

Shapes are the smallest that reach each launcher branch: H in {1, 2, 3, 5} (top and bottom halo in one
band), 2 and 3 strips (Cin 64: 128 columns, Cin 128: 64 columns per strip), one / two sources with
ld2 == ld1 (buffer-descriptor DMA) and ld2 != ld1 (flat addresses), persistent grids with fewer segments
than waves, tiles ending at image seams (B = 2), and five large cases for the band-height formulas
(conv3r_rb / rbfuse_rb: the largest divisor of H not above B H (W / SW) / 512 resp. / 256) and the
ring-depth-2 branch of conv3i (more than 256 blocks).

The CPU precondition test covers every case: test_conv_ops.py's mutants (padding line replicated, last K
tile dropped, x2 shifted by one vector, another image's scale / shift, output rows shifted) plus: the top
and the bottom padding ROW replicated; a strip's first column taken from the column before it (an
off-by-one at every multiple of the strip / segment / tile width); h outside the image computed from
zero-padded x instead of being zero (rbfuse and the pair); res_conv read at a non-centre tap (y2, rbfuse);
the two row parities' weight sets swapped and the unfolded middle kernel row dropped (uph). Each must move
the metric by more than 10 x the case's bound in every image (rbfuse's data make block2 eight times louder
than unit variance, so that what reaches y only through h shows beside the residual, which carries the loud
pixel ring; its padding-column mutant replicates both columns). The CPU coverage test asserts through the
hooks' plan-only / served-query modes (no GPU) the kind, tile, ring depth, FL bits, DMA form and class every
case selects, and that the reached set holds conv3r at both Cin, conv3w, conv3i in each (BM, BN) with and
without SWAP, RES, BUF, UPH and UPC, and both v3 CK forms. Every GPU case runs with 256 guard rows and
columns of a sentinel around y and y2 and slack rows after every input, all of which must come back
bit-unchanged, and asserts that the executed plan (rbfuse: band height and strip width) is the planned one.

Measured on an MI355X (the largest over a family's cases and images; kernel/bound is the largest ratio of a
case's error to its own bound, 1.0 = at the bound; every test prints its case's figures). No case exceeded
its bound, no guard band was touched and no kernel or launcher needed a change. Model and kernel agree to
three digits in 16 bits: the largest error is then the final rounding to T near max|ref|, which both share.
One statement of the sources turned out narrower than it reads: rbfuse equals the pair bit for bit where both
launches of the pair are conv3r (every case with W % 128 == 0); at Cin 128 and W = 320 the dispatcher gives
the pair's block2 to conv3w, which sums in another order, so there the fused block and the pair differ in
last bits (H > 1) and the test holds the pair to the fused block's bound against fp64 instead.
c3i_forced: the kC3IForce configurations; c3i: the default selection; large: the band-height and
ring-depth-2 cases; the y2 columns: the fused second output of the cases that have one.
Arithmetic-only mutants of the kernels, built aside and run once against these tests, failed exactly the
cases that reach them and no other: rbfuse dropping block2's residual (all 38 rbfuse cases); rbfuse taking
the h rows outside the image from block1 instead of zero (all 38); conv3r's fused y2 summing only the first
64 input channels (the 14 conv3r y2 cases, through y2's own bound, and the 20 Cin 128 rbfuse cases, through
the pair); conv3w skipping the shift of scale / shift (its 4 scale / shift cases); the C3I_RES tiles reading
w2 of the next output channel (the 8 conv3i y2 cases); the uph = 2 tiles swapping the column parities' weight
sets (the 16 uph = 2 cases).

family     type cases |    model   kernel kernel/bound | y2: cases    model   kernel kernel/bound
conv3r     bf16    34 |  3.6e-03  3.6e-03         0.25 |         7  3.4e-03  3.4e-03         0.25
conv3w     bf16    10 |  3.0e-03  3.0e-03         0.25 |         -        -        -            -
c3i_forced bf16    20 |  3.8e-03  3.8e-03         0.25 |         -        -        -            -
c3i        bf16    14 |  3.1e-03  3.1e-03         0.25 |         4  3.0e-03  3.0e-03         0.25
v3         bf16     4 |  2.4e-03  2.4e-03         0.25 |         -        -        -            -
uph        bf16    12 |  3.5e-03  3.5e-03         0.25 |         -        -        -            -
large      bf16     2 |  2.4e-03  2.4e-03         0.25 |         1  3.4e-03  3.4e-03         0.25
rbfuse     bf16    19 |  4.0e-03  4.0e-03         0.25 |         -        -        -            -
conv3r     fp16    34 |  4.6e-04  4.6e-04         0.25 |         6  4.3e-04  4.3e-04         0.25
conv3w     fp16    10 |  4.6e-04  4.6e-04         0.25 |         -        -        -            -
c3i_forced fp16    20 |  4.3e-04  4.3e-04         0.25 |         -        -        -            -
c3i        fp16    14 |  4.5e-04  4.5e-04         0.25 |         4  4.1e-04  4.1e-04         0.25
v3         fp16     4 |  3.4e-04  3.4e-04         0.25 |         -        -        -            -
uph        fp16    12 |  4.3e-04  4.3e-04         0.25 |         -        -        -            -
large      fp16     1 |  4.0e-04  4.0e-04         0.25 |         -        -        -            -
rbfuse     fp16    19 |  4.8e-04  4.8e-04         0.25 |         -        -        -            -
c3i_forced fp32    16 |  4.5e-07  7.0e-07         0.90 |         -        -        -            -
c3i        fp32     2 |  4.0e-07  6.0e-07         0.46 |         -        -        -            -
v3         fp32     3 |  2.7e-07  5.2e-07         0.48 |         -        -        -            -
"""
import ctypes
import functools
import math
import zlib
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import test_conv_ops as co  # noqa: E402

TDT, H16, MIN, ALL, NONE, SILU, GUARD = co.TDT, co.H16, co.MIN, co.ALL, co.NONE, co.SILU, co.GUARD
C3I_SWAP, C3I_RES, C3I_BUF, C3I_UPH, C3I_UPC = 8, 16, 1024, 8192, 16384     # conv_plan.h
# conv_plan.cpp kC3IForce: code -> (BM, BN, ST, FL)
C3I_FORCE = {2: (256, 64, 2, 0), 4: (128, 128, 2, 0), 11: (256, 64, 2, 1), 12: (256, 64, 2, 2), 13: (256, 64, 2, 3),
             14: (256, 128, 2, 1), 15: (256, 128, 2, 3), 16: (256, 64, 3, 1), 17: (256, 64, 2, 5), 19: (64, 128, 2, 4),
             20: (128, 64, 2, 4), 22: (64, 64, 2, 4), 18: (256, 64, 2, 4), 8: (128, 128, 3, 3), 9: (128, 128, 2, 3),
             10: (128, 64, 2, 3), 40: (256, 64, 2, 12), 41: (128, 64, 2, 12), 48: (256, 64, 2, 12 | C3I_BUF),
             49: (128, 64, 2, 12 | C3I_BUF)}


# ------------------------------------------------------------------ cases
def mk3(fam, dt, B, H, W, C, Cout, want, fl=None, buf=None, label=None, sw=0, **kw):
    """One 3x3 launch (test_conv_ops.mk) plus: y2 (fused second output), uph, ld1 / ld2 (pitches; None: the
    defaults of test_conv_ops.layout), and what the plan must say besides `want`: FL bits, DMA form, class.
    sw: the width at whose multiples the kernel's column blocks meet (strip / segment / tile)."""
    c = co.mk(fam, dt, 3, B, H, W, C, Cout, want, **dict(dict(y2=False, uph=0, ld1=None, ld2=None), fl=fl, buf=buf,
                                                          label=label, sw=sw, **kw))
    c.key += f"-y{int(c.y2)}u{c.uph}-l{c.ld1}.{c.ld2}"
    c.id = f"{dt}-{c.key}"
    return c


EPI4 = co.EPI4
EPI_R = [dict(), dict(bias=True, act=SILU), dict(ss=True, act=SILU), dict(res1=True, act=SILU), dict(ss=True, res1=True),
         dict(bias=True, res1=True)]                                                  # what conv3r takes
EPI_W = [dict(), dict(bias=True, act=SILU), dict(ss=True, act=SILU), dict(res1=True, act=SILU), dict(bias=True, res1=True)]
OWN = lambda k: (k, 0, 0, 0, 0)


def build_cases():
    cs = []
    for di, dt in enumerate(H16):
        # conv3r, Cin 64: strips of 128 columns -> W = 256 / 384 are 2 / 3 strips; every H puts the top and the
        # bottom halo row in one band (rb = 1: B H (W / 128) < 512). Default selection and conv3_force = 70.
        n = di
        for W in (256, 384):
            for H in (1, 2, 3, 5):
                for B in (1, 2):
                    cs.append(mk3("conv3r", dt, B, H, W, 64, 64, OWN("conv3r"), sw=128, f3=(-1, 70)[n % 2],
                                  **EPI_R[n % len(EPI_R)]))
                    n += 1
        # conv3r, Cin 128: strips of 64 columns -> W = 256 / 320 are 4 / 5 strips. Sources: one 128-channel
        # tensor, or 64 | 64 with ld2 = 64 and 96; the fused y2 (no res1 with it).
        SRC = [dict(), dict(C1=64, ld2=64), dict(C1=64, ld2=96), dict(ld1=136)]
        EPI_R2 = EPI_R + [dict(y2=True), dict(y2=True, ss=True, act=SILU), dict(y2=True, bias=True, act=SILU)]
        for W in (256, 320):
            for H in (1, 2, 3, 5):
                for B in (1, 2):
                    e = EPI_R2[n % len(EPI_R2)]                      # (the selection fuses y2 only when nothing is forced)
                    cs.append(mk3("conv3r", dt, B, H, W, 128, 64, OWN("conv3r"), sw=64,
                                  f3=-1 if e.get("y2") else (-1, 70)[(n // 3) % 2], **SRC[n % 4], **e))
                    n += 1
        for s in SRC[1:3]:              # y2 over two sources at both pitches, whatever the cycles above paired
            cs.append(mk3("conv3r", dt, 2, 4, 320, 128, 64, OWN("conv3r"), sw=64, y2=True, ss=True, act=SILU, **s))
        # conv3w: 64-pixel segments, 8 waves per block: W x H = 64 x 1 is one segment in total, 128 x 3 with
        # B = 1 six (fewer than a block's waves), the others more than one block's worth. One source, or
        # 32 | 32 with ld2 = ld1 (buffer-descriptor form) and ld2 = 40 (flat form).
        n = di
        for W in (64, 128, 192):
            for H in (1, 3, 8):
                B = 1 if (W, H) in ((64, 1), (128, 3)) else 2
                src = [dict(), dict(C1=32, ld2=32), dict(C1=32, ld2=40)][n % 3]
                buf = 0 if src.get("ld2") == 40 else 1
                cs.append(mk3("conv3w", dt, B, H, W, 64, 64, OWN("conv3w"), buf=buf, sw=64, f3=(-1, 30, 35)[(n // 3) % 3],
                              **src, **EPI_W[n % len(EPI_W)]))
                n += 1
        # ... and over a 2x nearest-upsampled input (the kernel halves the row and column indices).
        cs.append(mk3("conv3w", dt, 2, 4, 32, 64, 64, OWN("conv3w"), buf=1, sw=64, up=1, bias=True))
        # conv3i: every forced configuration at an aligned small shape (B = 2, 8 x 64: row width 64 for every BM).
        for n, (code, (BM, BN, ST, fl)) in enumerate(sorted(C3I_FORCE.items())):
            cs.append(mk3("c3i_forced", dt, 2, 8, 64, 64, 128, ("conv3i", BM, BN, ST, MIN), fl=fl, buf=int(fl >= 1024),
                          sw=64, f3=code, **EPI4[(n + di) % 4]))
        # conv3i, default selection. Grids of at most 256 blocks take ring depth 3 (with BUF), else 2.
        D = lambda BM, ST, fl: dict(want=("conv3i", BM, 64, ST, MIN), fl=fl, buf=int(fl >= 1024))
        sel = [
            # 256 x 64 swapped with BUF, and without it (ld2 != ld1)
            (2, 8, 64, 128, 128, D(256, 3, 12 | C3I_BUF), dict()),
            (2, 8, 64, 128, 128, D(256, 2, 12), dict(C1=64, ld2=72)),
            (2, 8, 64, 64, 128, D(256, 3, 12 | C3I_BUF), dict(C1=32, ld1=40, ld2=40)),
            (2, 4, 64, 256, 64, D(256, 2, 12), dict(C1=128)),
            # 128 x 64 at W = 32 (4 rows per tile; the selection asks H % 8 of every v4 / v3 shape this narrow)
            (2, 8, 32, 64, 128, D(128, 3, 12 | C3I_BUF), dict()),
            (2, 8, 32, 128, 256, D(128, 2, 12), dict(C1=64)),
            # row widths 128, 256, 512 (two tiles per row) and 768 (not a power of two: three tiles per row)
            (2, 2, 128, 64, 128, D(256, 3, 12 | C3I_BUF), dict()),
            (2, 3, 256, 64, 128, D(256, 3, 12 | C3I_BUF), dict()),
            (2, 1, 512, 64, 128, D(256, 3, 12 | C3I_BUF), dict()),
            (2, 2, 768, 64, 128, D(256, 3, 12 | C3I_BUF), dict()),
            # C3I_RES fused y2 at BM = 256 and BM = 128 (a 64 | 128 -> 128 concat), with and without BUF
            (2, 8, 64, 128, 64, D(256, 2, 12 | C3I_RES | C3I_BUF), dict(y2=True)),
            (2, 8, 64, 128, 128, D(256, 2, 12 | C3I_RES), dict(y2=True, C1=64, ld2=72)),
            (2, 8, 32, 192, 128, D(128, 2, 12 | C3I_RES), dict(y2=True, C1=64)),
            (2, 8, 32, 192, 128, D(128, 2, 12 | C3I_RES | C3I_BUF), dict(y2=True, C1=64, ld1=136, ld2=136)),
        ]
        for n, (B, H, W, C, O, d, kw) in enumerate(sel):
            e = [dict(bias=True, act=SILU), dict(ss=True, act=SILU), dict()][n % 3] if kw.get("y2") else EPI4[(n + di) % 4]
            cs.append(mk3("c3i", dt, B, H, W, C, O, sw=min(W, d["want"][1]), **d, **kw, **e))
        # v3 (conv3_force = 0): 128 x 64 tiles (Cout <= 64), 128 x 128 with CK = 128 (fewer than 64 tiles per
        # image: class 11) and with CK = 64 (64 x 128 pixels x 128 channels = 64 tiles: class 7).
        cs.append(mk3("v3", dt, 2, 16, 16, 64, 64, ("conv3", 128, 64, 2, MIN), label=6, sw=16, f3=0, **EPI4[di]))
        cs.append(mk3("v3", dt, 2, 16, 16, 128, 128, ("conv3", 128, 128, 2, MIN), label=11, sw=16, f3=0, **EPI4[1 + di]))
        cs.append(mk3("v3", dt, 2, 8, 32, 128, 192, ("conv3", 128, 128, 2, MIN), label=11, sw=32, f3=0, C1=64, **EPI4[2 + di]))
        cs.append(mk3("v3", dt, 1, 64, 128, 64, 128, ("conv3", 128, 128, 2, MIN), label=7, sw=128, f3=0, **EPI4[3 - di]))
        # Row- and row+column-phase upsample tiles (256 x 64, one row parity per tile, BUF).
        n = di
        for (uph, H, W) in ((1, 8, 32), (2, 4, 64), (2, 8, 128)):
            for C in (64, 128):
                for O in (64, 128):
                    fl = 12 | C3I_UPH | (C3I_UPC if uph == 2 else 0) | C3I_BUF
                    e = [dict(bias=True), dict(bias=True, act=SILU), dict(ss=True, res1=True), dict()][n % 4]
                    cs.append(mk3("uph", dt, 2, H, W, C, O, ("conv3i", 256, 64, 2, MIN), fl=fl, buf=1, sw=min(2 * W, 256),
                                  up=1, uph=uph, **e))
                    n += 1
    # fp32: the non-swapped conv3i tiles and v3.
    for n, (code, (BM, BN, ST, fl)) in enumerate(sorted(C3I_FORCE.items())):
        if not fl & C3I_SWAP:
            cs.append(mk3("c3i_forced", "fp32", 2, 8, 64, 64, 128, ("conv3i", BM, BN, ST, MIN), fl=fl, buf=0, sw=64, f3=code,
                          **EPI4[n % 4]))
    cs.append(mk3("c3i", "fp32", 2, 8, 64, 64, 128, ("conv3i", 256, 64, 2, MIN), fl=4, buf=0, sw=64, bias=True, act=SILU))
    cs.append(mk3("c3i", "fp32", 2, 8, 32, 64, 128, ("conv3i", 128, 64, 2, MIN), fl=4, buf=0, sw=32, C1=32, ss=True, res1=True))
    cs.append(mk3("v3", "fp32", 2, 16, 16, 64, 64, ("conv3", 128, 64, 2, MIN), label=6, sw=16, f3=0, bias=True, act=SILU))
    cs.append(mk3("v3", "fp32", 2, 16, 16, 64, 128, ("conv3", 128, 128, 2, MIN), label=11, sw=16, f3=0, ss=True, res1=True))
    cs.append(mk3("v3", "fp32", 1, 64, 128, 32, 128, ("conv3", 128, 128, 2, MIN), label=7, sw=128, f3=0, res1=True, res2=True))
    # The large cases (one dtype each). conv3r_rb: rb = B H (W / 64) / 512 = 2 * 64 * 8 / 512 = 2; and
    # 2 * 27 * 38 / 512 = 4, which does not divide 27 -> 3. conv3i: 2 * 128 * 128 / 256 tiles x 4 channel
    # tiles = 512 blocks > 256 -> ring depth 2.
    cs.append(mk3("large", "bf16", 2, 64, 512, 128, 64, OWN("conv3r"), sw=64, C1=64, ld2=96, y2=True, ss=True, act=SILU))
    cs.append(mk3("large", "fp16", 2, 27, 2432, 128, 64, OWN("conv3r"), sw=64, res1=True, act=SILU))
    cs.append(mk3("large", "bf16", 2, 128, 128, 64, 256, ("conv3i", 256, 64, 2, MIN), fl=12 | C3I_BUF, buf=1, sw=128,
                  ss=True, res1=True))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = build_cases()
FAMILIES = sorted({c.fam for c in CASES})
BY_ID = {c.id: c for c in CASES}
co.BY_ID.update(BY_ID)                                    # test_conv_ops.make() looks its cases up there


def mkrb(dt, B, H, W, C, rb, **kw):
    """One fused ResBlock launch; rb: the band height the shape was designed for (strip width from Cin)."""
    c = SimpleNamespace(fam="rbfuse", dt=dt, B=B, H=H, W=W, C=C, C1=C, ld1=None, ld2=None, rb=rb, sw=128 if C == 64 else 64)
    c.__dict__.update(kw)
    c.key = f"rbfuse-B{B}-{H}x{W}-C{C}{'+' if c.C1 < C else ''}-l{c.ld1}.{c.ld2}"
    c.id = f"{dt}-{c.key}"
    return c


def build_rb_cases():
    cs = []
    for di, dt in enumerate(H16):
        n = di
        for (C, Ws) in ((64, (256, 384)), (128, (256, 320))):
            for W in Ws:
                for H in (1, 2, 3, 5):
                    B = 1 + (n % 2)
                    src = dict() if C == 64 else [dict(), dict(C1=64, ld2=64), dict(C1=64, ld2=96), dict(ld1=136)][n % 4]
                    cs.append(mkrb(dt, B, H, W, C, 1, **src))
                    n += 1
        for s in (dict(C1=64, ld2=64), dict(C1=64, ld2=96)):
            cs.append(mkrb(dt, 2, 4, 320, 128, 1, **s))
    # rbfuse_rb: rb = B H (W / 128) / 256 = 2 * 64 * 4 / 256 = 2; and 2 * 27 * 19 / 256 = 4 -> 3 (27 % 4 != 0).
    cs.append(mkrb("fp16", 2, 64, 512, 64, 2))
    cs.append(mkrb("bf16", 2, 27, 2432, 64, 3))
    assert len({c.id for c in cs}) == len(cs)
    return cs


RB_CASES = build_rb_cases()
RB_BY_ID = {c.id: c for c in RB_CASES}


# ------------------------------------------------------------------ data, reference, model
def silu(v):
    return v * torch.sigmoid(v)


def bound(dt, model, ref):
    """test_conv_ops.py's rule -> (model err, tol) per image."""
    me = co.rel_err(model, ref)
    mx = ref.abs().reshape(ref.shape[0], -1).max(dim=1).values.tolist()
    if dt == "fp32":
        return me, [4.0 * e for e in me]
    return me, [max(4.0 * e, 2.0 * co.ulp_rel(dt, m)) for e, m in zip(me, mx)]


def layout3(c):
    d = co.layout(c)
    if c.ld1 is not None:
        d.ld1 = c.ld1
    if c.ld2 is not None:
        d.ld2 = c.ld2
    d.ldy2 = c.Cout + GUARD + 8
    d.w2 = d.y2 = 1 if c.y2 else None
    return d


def pitched(t, ld, rows=None):
    """t [..., n] -> [rows, ld] with 1000 in the columns beyond n."""
    t = t.reshape(-1, t.shape[-1])
    out = torch.full((t.shape[0], ld), 1000.0, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def pack_uph(c, W, dtype_code):
    """dac_op_pack (csrc/pack.h fold_row_phase / fold_rowcol_phase) of W [O][C][3][3] fp32 -> the folded rows as
    stored: [O, 4, 3 or 4, C] (16-bit codes decoded; DAC_F32: the fp32 sums), as float64."""
    from daclip_amd import _lib
    O, C = W.shape[:2]
    nt = 3 if c.uph == 1 else 4
    ds = _lib.DacPackDesc(layout=_lib.DAC_PACK_UPH_ROW if c.uph == 1 else _lib.DAC_PACK_UPH_COL, dtype=dtype_code, round=0,
                          O=O, C=C, kh=3, kw=3, kwp=0, F=0, I=0, K=0, flag=0, scale=1.0)
    w = W.float().contiguous()
    es = 4 if dtype_code == _lib.DAC_F32 else 2
    out = torch.zeros(O * 4 * nt * C, dtype=torch.float32 if es == 4 else torch.int16)
    need = (ctypes.c_size_t * 3)()
    outs = (ctypes.c_void_p * 3)(out.data_ptr(), None, None)
    cap = (ctypes.c_size_t * 3)(out.numel() * es, 0, 0)
    rc = _lib.lib().dac_op_pack(ctypes.byref(ds), ctypes.c_void_p(w.data_ptr()), None, None, None, outs, cap, need)
    assert rc == 0 and need[0] == out.numel() * es, (rc, need[0])
    if es == 2:
        out = out.view(TDT[c.dt])
    return out, out.double().reshape(O, 4, nt, C)


def phase_acc(c, X, Wf):
    """The phase definition. X [B, H, W, C], Wf [O, 4, nt, C] (one dtype) -> [B, 2H * 2W, O]."""
    B, H, W, _ = X.shape
    x = X.permute(0, 3, 1, 2)
    if c.uph == 1:
        x = x.repeat_interleave(2, 3)
    xp = F.pad(x, (1, 1, 1, 1))                            # xp row p = source row p - 1
    out = torch.zeros(B, Wf.shape[0], 2 * H, 2 * W, dtype=X.dtype)
    for a in (0, 1):                                       # conv row j reads xp rows j, j + 1: j = i + a
        if c.uph == 1:
            r = F.conv2d(xp, Wf[:, 2 * a:2 * a + 2].permute(0, 3, 1, 2))
            out[:, :, a::2, :] = r[:, :, a:a + H, :]
        else:
            for b in (0, 1):
                r = F.conv2d(xp, Wf[:, 2 * a:2 * a + 2, 2 * b:2 * b + 2].permute(0, 3, 1, 2))
                out[:, :, a::2, b::2] = r[:, :, a:a + H, b:b + W]
    return out.permute(0, 2, 3, 1).reshape(B, -1, Wf.shape[0])


def fold_rows64(W, mut=None):
    """The row (and column) fold in float64 from W [O][C][3][3], for the weight-level mutants."""
    w = W.permute(0, 2, 3, 1)                              # [O][kh][kw][C]
    mid = 0.0 if mut == "midrow" else 1.0
    rows = torch.stack([w[:, 0], mid * w[:, 1] + w[:, 2], w[:, 0] + mid * w[:, 1], w[:, 2]], 1)
    if mut == "parity":
        rows = torch.cat([rows[:, 2:], rows[:, :2]], 1)
    return rows


def fold_cols64(rows):
    return torch.stack([rows[:, :, 0], rows[:, :, 1] + rows[:, :, 2], rows[:, :, 0] + rows[:, :, 1], rows[:, :, 2]], 2)


def strip_mut(c, y):
    """Every column block's first column repeats the column before it. y [B, Ho * Wo, O]."""
    Ho, Wo = co.out_hw(c)
    v = y.reshape(y.shape[0], Ho, Wo, -1).clone()
    for x0 in range(c.sw, Wo, c.sw):
        v[:, :, x0] = v[:, :, x0 - 1]
    return v.reshape(y.shape)


def acc3(c, d, mut=None, dtype=torch.float64):
    if c.uph:
        X, Wf = d.Xq, d.Wfold
        if mut == "x2shift":
            X, _ = co.mutated(c, d, mut)
        elif mut == "ktile":
            Wf = Wf.clone().reshape(Wf.shape[0], -1)
            Wf[:, -co.bke(c):] = 0
            Wf = Wf.reshape(d.Wfold.shape)
        elif mut in ("parity", "midrow"):
            Wf = fold_rows64(d.Wq, mut)
            Wf = fold_cols64(Wf) if c.uph == 2 else Wf
        Xp = X
        if mut in ("padtop", "padbot"):                    # the missing source row repeats the edge row
            Xp = torch.cat([X[:, :1], X] if mut == "padtop" else [X, X[:, -1:]], 1)
        y = phase_acc(c, Xp.to(dtype), Wf.to(dtype))
        if mut in ("padtop", "padbot"):
            Wo = 2 * c.W
            y = y.reshape(c.B, 2 * c.H + 2, Wo, -1)
            # rows of the extended image; its padding row is still zero, the image's is not
            y = (y[:, 2:] if mut == "padtop" else y[:, :-2]).reshape(c.B, -1, y.shape[-1])
        return y
    X, W = co.mutated(c, d, mut)
    if mut in ("padtop", "padbot"):
        x = X.permute(0, 3, 1, 2)
        if c.up:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        x = F.pad(x, (1, 1, 1, 1))
        if mut == "padtop":
            x[..., 0, :] = x[..., 1, :]
        else:
            x[..., -1, :] = x[..., -2, :]
        return F.conv2d(x.to(dtype), W.to(dtype)).permute(0, 2, 3, 1).reshape(c.B, -1, c.Cout)
    return co.conv_acc(c, X.to(dtype), W.to(dtype), mut)


def reference3(c, d, mut=None):
    y = co.epilogue(c, d, acc3(c, d, mut), torch.float64, mut)
    if mut == "rowshift":
        y = torch.roll(y.reshape(-1, y.shape[-1]), co.row_width(c), 0).reshape(y.shape)
    if mut == "strip":
        y = strip_mut(c, y)
    return y


def y2_acc(c, d, dtype, mut=None):
    X = d.Xq
    if mut == "restap":                                    # the tap left of the centre
        X = F.pad(X, (0, 0, 1, 0))[:, :, :-1]
    elif mut == "x2shift":
        X, _ = co.mutated(c, d, mut)
    return (X.to(dtype).reshape(c.B, -1, c.C) @ d.w2q.to(dtype).t())


def mutants3(c):
    m = [x for x in co.mutants(c) if x != "pad"] + ([] if c.uph else ["pad"]) + ["padtop", "padbot"]
    if co.out_hw(c)[1] > c.sw > 0:
        m.append("strip")
    if c.uph:
        m += ["parity", "midrow"]
    return m


@functools.lru_cache(maxsize=4)
def make3(c_id):
    c = BY_ID[c_id]
    T = TDT[c.dt]
    base = co.make(c_id)
    d = SimpleNamespace(**base.__dict__)
    d.__dict__.update({k: v for k, v in layout3(c).__dict__.items() if k in ("ld1", "ld2", "ldy2")})
    q = lambda t: t.to(T).double()
    if c.uph:
        from daclip_amd import _lib
        code = {"bf16": _lib.DAC_BF16, "fp16": _lib.DAC_F16}[c.dt]
        d.wp, d.Wfold = pack_uph(c, d.Wq, code)
        d.wp = d.wp.reshape(c.Cout, -1)
        d.ref = co.epilogue(c, d, acc3(c, d), torch.float64)
        model = co.epilogue(c, d, acc3(c, d, dtype=torch.float32), torch.float32).to(T)
        d.model_err, d.tol = bound(c.dt, model, d.ref)
    d.x1 = pitched(d.Xq[..., :c.C1].to(T), d.ld1)
    d.x2 = pitched(d.Xq[..., c.C1:].to(T), d.ld2) if c.C1 < c.C else None
    d.w2 = d.w2q = d.ref2 = None
    if c.y2:
        g = torch.Generator().manual_seed(zlib.crc32(("w2" + c.key).encode()))
        d.w2q = q(torch.randn(c.Cout, c.C, generator=g, dtype=torch.float64) / math.sqrt(c.C))
        d.w2 = d.w2q.to(T)
        d.ref2 = y2_acc(c, d, torch.float64)
        d.model_err2, d.tol2 = bound(c.dt, y2_acc(c, d, torch.float32).to(T), d.ref2)
    return d


def descriptor3(c, d):
    from daclip_amd import _lib
    ds = co.descriptor(c, d)
    if c.uph:
        ds.K = (12 if c.uph == 1 else 16) * c.C
    return ds, _lib.DacConvExt(uph=c.uph, ldy2=d.ldy2)


def hook3(c, d, ptr, y, y2):
    """dac_op_conv_ex with ptr(tensor) for every operand the case has; -> (rc, plan)."""
    from daclip_amd import _lib
    ds, ex = descriptor3(c, d)
    plan = (ctypes.c_int * _lib.DAC_CONV_PLAN_N)()
    rc = _lib.lib().dac_op_conv_ex(ctypes.byref(ds), ctypes.byref(ex), ptr(d.x1), ptr(d.x2), ptr(d.wp), ptr(d.bp), ptr(d.ss),
                                   ptr(d.res1), ptr(d.res2), ptr(d.bbias), None, None, y, ptr(d.w2), y2, plan, None)
    return rc, list(plan)


DUMMY = ctypes.c_void_p(1 << 20)


def plan_only3(c):
    d = layout3(c)
    return hook3(c, d, lambda t: None if t is None else DUMMY, None, DUMMY if c.y2 else None)


def plan_ok(c, plan):
    """The plan says what the case names."""
    return (co.plan_key(plan) == c.want and (c.fl is None or plan[5] == c.fl) and (c.buf is None or plan[6] == c.buf) and
            (c.label is None or plan[7] == c.label))


# ---- rbfuse
def rb_forward(c, d, dtype, mut=None, rounded=None):
    """The ResBlock on d's operands in `dtype`; rounded: the storage type T for the rounding model (h and the
    res_conv output rounded to T, the output once at the end), or None. -> [B, H * W, 64]."""
    rnd = (lambda t: t.to(rounded).to(dtype)) if rounded is not None else (lambda t: t)
    X = d.Xq
    if mut == "x2shift":
        X = torch.cat([X[..., :c.C1], torch.roll(X[..., c.C1:], 8, -1)], -1)
    x = X.to(dtype).permute(0, 3, 1, 2)
    W1, W2 = d.W1q.to(dtype), d.W2q.to(dtype)
    ss = d.ss.to(dtype)
    if mut == "imgterm":
        ss = torch.roll(ss, 1, 0)
    sc, sh = (1.0 + ss[:, :64])[:, :, None, None], ss[:, 64:][:, :, None, None]
    block1 = lambda xpad: silu(F.conv2d(xpad, W1) * sc + sh)
    if mut == "hpad":                                      # h outside the image: block1 over zero-padded x
        a2 = F.conv2d(rnd(block1(F.pad(x, (2, 2, 2, 2)))), W2)
    else:
        xp = F.pad(x, (1, 1, 1, 1))
        if mut == "padtop":
            xp[..., 0, :] = xp[..., 1, :]
        elif mut == "padbot":
            xp[..., -1, :] = xp[..., -2, :]
        elif mut == "pad":                                 # both padding columns
            xp[..., :, 0], xp[..., :, -1] = xp[..., :, 1], xp[..., :, -2]
        hp = F.pad(rnd(block1(xp)), (1, 1, 1, 1))
        if mut == "hpadrep":
            hp[..., 0, :] = hp[..., 1, :]
        a2 = F.conv2d(hp, W2)
    xr = F.pad(x, (1, 0))[..., :-1] if mut == "restap" else x
    res = xr if c.C == 64 else rnd(F.conv2d(xr, d.wrq.to(dtype)[:, :, None, None]))
    y = (silu(a2) + res).permute(0, 2, 3, 1).reshape(c.B, -1, 64)
    if mut == "rowshift":
        y = torch.roll(y.reshape(-1, 64), c.W if c.B * c.H > 1 else c.W // 2, 0).reshape(y.shape)
    if mut == "strip":
        y = strip_mut(SimpleNamespace(kh=3, H=c.H, W=c.W, up=0, sw=c.sw), y)
    return rnd(y)


def rb_mutants(c):
    m = ["pad", "padtop", "padbot", "hpad", "hpadrep", "restap", "rowshift", "strip"]
    if c.C1 < c.C:
        m.append("x2shift")
    if c.B > 1:
        m.append("imgterm")
    return m


def rb_layout(c):
    ld1 = c.ld1 if c.ld1 is not None else c.C1
    return SimpleNamespace(ld1=ld1, ld2=(c.ld2 if c.ld2 is not None else 0), ss_ld=132, ldy=64 + GUARD, M=c.B * c.H * c.W)


@functools.lru_cache(maxsize=4)
def make_rb(c_id):
    c = RB_BY_ID[c_id]
    T = TDT[c.dt]
    g = torch.Generator().manual_seed(zlib.crc32(c.key.encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q = lambda t: t.to(T).double()
    d = rb_layout(c)
    X = rn(c.B, c.H, c.W, c.C)
    ring = torch.zeros(c.H, c.W, dtype=torch.float64)      # loud outermost pixel ring
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = 1, 1, 1, 1
    d.Xq = q(X * (1.0 + 3.0 * ring)[None, :, :, None])
    d.W1q = q(rn(64, c.C, 3, 3) / math.sqrt(9 * c.C))
    # (block2 eight times louder than unit variance: the residual carries the loud pixel ring, and what only
    # reaches y through h must not vanish beside it)
    d.W2q = q(8.0 * rn(64, 64, 3, 3) / math.sqrt(576.0))
    d.wrq = q(rn(64, c.C) / math.sqrt(c.C)) if c.C == 128 else None
    r = rn(c.B, 128)
    d.ss = torch.cat([0.5 * r[:, :64], r[:, 64:]], 1).float()
    d.ref = rb_forward(c, d, torch.float64)
    assert torch.isfinite(d.ref).all()
    d.model_err, d.tol = bound(c.dt, rb_forward(c, d, torch.float32, rounded=T), d.ref)
    d.x1 = pitched(d.Xq[..., :c.C1].to(T), d.ld1)
    d.x2 = pitched(d.Xq[..., c.C1:].to(T), d.ld2) if c.C1 < c.C else None
    d.w1, d.w2 = co.pack_plain(d.W1q).to(T), co.pack_plain(d.W2q).to(T)
    d.wr = d.wrq.to(T) if c.C == 128 else None
    d.ssp = pitched(d.ss, d.ss_ld)
    return d


def rb_hook(c, d, ptr, y, **over):
    """dac_op_rbfuse; over: descriptor fields to replace. -> (rc, [band height, strip width])."""
    from daclip_amd import _lib
    f = dict(dtype={"bf16": _lib.DAC_BF16, "fp16": _lib.DAC_F16}[c.dt], B=c.B, H=c.H, W=c.W, C1=c.C1, Cin=c.C, ld1=d.ld1,
             ld2=d.ld2, ss_ld=d.ss_ld, ldy=d.ldy)
    f.update(over)
    ds = _lib.DacRbDesc(**f)
    geom = (ctypes.c_int * 2)(-1, -1)
    rc = _lib.lib().dac_op_rbfuse(ctypes.byref(ds), ptr("x1"), ptr("x2"), ptr("w1"), ptr("w2"), ptr("wr"), ptr("ssp"), y, geom,
                                  None)
    return rc, list(geom)


def rb_query(c, wr=True, **over):
    have = lambda n: (n != "x2" or c.C1 < c.C) and (n != "wr" or (c.C == 128 and wr))
    return rb_hook(c, rb_layout(c), lambda n: DUMMY if have(n) else None, None, **over)


# ------------------------------------------------------------------ CPU: the definitions, literally
def gather(d, c, b, row, col):
    """Input pixel (row, col) of image b from the pitched arrays the hook gets: [C], zero outside the image."""
    if not (0 <= row < c.H and 0 <= col < c.W):
        return torch.zeros(c.C, dtype=torch.float64)
    m = (b * c.H + row) * c.W + col
    v = d.x1[m, :c.C1].double()
    return v if d.x2 is None else torch.cat([v, d.x2[m, :c.C - c.C1].double()])


def test_reference_matches_definition():
    """For one case of each new layout (y2, uph row, uph column) the literal packed-K GEMM over the arrays handed
    to the hook -- A gathered pixel by pixel from x1 | x2 with their pitches, W the packed rows with K read as
    the descriptor says -- equals the logical reference to 1e-12."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    pick = {}
    for c in CASES:
        k = "y2" if c.y2 else f"uph{c.uph}"
        if c.fam != "large" and c.dt == "bf16" and (c.y2 or c.uph) and (k not in pick or (c.C1 < c.C and c.y2)):
            pick[k] = c
    assert sorted(pick) == ["uph1", "uph2", "y2"]
    for c in pick.values():
        d = make3(c.id)
        ds, ex = descriptor3(c, d)
        if c.y2:
            A = torch.stack([gather(d, c, b, r, x) for b in range(c.B) for r in range(c.H) for x in range(c.W)])
            out = (A @ d.w2.double().t()).reshape(c.B, -1, c.Cout)
            e = max(co.rel_err(out, d.ref2))
            assert e < 1e-12, (c.id, e)
            continue
        nt = 3 if c.uph == 1 else 4
        assert ds.K == 4 * nt * c.C and tuple(d.wp.shape) == (c.Cout, ds.K)
        wp = d.wp.double().reshape(c.Cout, 4, nt, c.C)
        Ho, Wo = 2 * c.H, 2 * c.W
        g = torch.Generator().manual_seed(1)
        rows = torch.randint(0, c.B * Ho * Wo, (192,), generator=g).tolist() + [0, Wo - 1, (Ho - 1) * Wo, c.B * Ho * Wo - 1]
        acc = torch.zeros(len(rows), c.Cout, dtype=torch.float64)
        for j, m in enumerate(rows):
            b, oh, ow = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
            i, a = oh // 2, oh % 2
            for s in (0, 1):
                if c.uph == 1:                             # taps over the upsampled columns ow - 1 .. ow + 1
                    for t in range(3):
                        u = ow + t - 1
                        px = gather(d, c, b, i - 1 + a + s, u // 2 if 0 <= u < Wo else -1)
                        acc[j] += wp[:, 2 * a + s, t] @ px
                else:
                    jj, bb = ow // 2, ow % 2
                    for t in (0, 1):
                        acc[j] += wp[:, 2 * a + s, 2 * bb + t] @ gather(d, c, b, i - 1 + a + s, jj - 1 + bb + t)
        accfull = phase_acc(c, d.Xq, d.Wfold).reshape(-1, c.Cout)
        e = ((accfull[rows] - acc).abs().max() / accfull.abs().max()).item()
        assert e < 1e-12, (c.id, e)
        assert torch.equal(co.epilogue(c, d, accfull.reshape(c.B, -1, c.Cout), torch.float64), d.ref)


@pytest.mark.parametrize("uph", [1, 2])
def test_phase_definition_equals_the_plain_upsampled_conv(uph):
    """With unrounded (DAC_F32) packing the phase definition is the plain nearest-2x + 3x3 conv (to 1e-12; the
    weights sit on a 2^-10 grid so that the packer's fp32 sums are exact)."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    from daclip_amd import _lib
    g = torch.Generator().manual_seed(7 + uph)
    c = SimpleNamespace(uph=uph, dt="fp32")
    W = torch.round(torch.randn(24, 16, 3, 3, generator=g, dtype=torch.float64) * 64.0) / 1024.0
    X = torch.randn(2, 5, 7, 16, generator=g, dtype=torch.float64)
    _, Wf = pack_uph(c, W, _lib.DAC_F32)
    rows = fold_rows64(W)
    assert torch.equal(Wf, rows if uph == 1 else fold_cols64(rows))
    x = X.permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    plain = F.conv2d(x, W, padding=1).permute(0, 2, 3, 1).reshape(2, -1, 24)
    e = max(co.rel_err(phase_acc(c, X, Wf), plain))
    assert e < 1e-12, e


# ------------------------------------------------------------------ CPU: preconditions and sensitivity
@pytest.mark.parametrize("fam", FAMILIES)
def test_preconditions_and_sensitivity(fam):
    """Every case: a finite reference, a sane rounding model, and every reference-level mutant moves the
    metric by more than 10 x the case's bound (in every image)."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    for c in [c for c in CASES if c.fam == fam]:
        d = make3(c.id)
        lim = {"bf16": 0.05, "fp16": 0.01, "fp32": 1e-5}[c.dt]
        assert all(0 < t < lim for t in d.tol), (c.id, d.tol)
        moved = {}
        for mut in mutants3(c):
            mv = co.rel_err(reference3(c, d, mut), d.ref)
            moved[mut] = min(mv)
            assert all(m > 10.0 * t for m, t in zip(mv, d.tol)), (c.id, mut, mv, d.tol)
        if c.y2:
            assert all(0 < t < lim for t in d.tol2), (c.id, d.tol2)
            for mut in ["restap"] + (["x2shift"] if c.C1 < c.C else []):
                mv = co.rel_err(y2_acc(c, d, torch.float64, mut), d.ref2)
                moved["y2_" + mut] = min(mv)
                assert all(m > 10.0 * t for m, t in zip(mv, d.tol2)), (c.id, "y2", mut, mv, d.tol2)
        print(f"{c.id}: model {max(d.model_err):.2e} tol {max(d.tol):.2e} " +
              " ".join(f"{n} {v:.2e}" for n, v in moved.items()))


def test_rbfuse_preconditions_and_sensitivity():
    for c in RB_CASES:
        d = make_rb(c.id)
        assert all(0 < t < {"bf16": 0.05, "fp16": 0.01}[c.dt] for t in d.tol), (c.id, d.tol)
        moved = {}
        for mut in rb_mutants(c):
            mv = co.rel_err(rb_forward(c, d, torch.float64, mut), d.ref)
            moved[mut] = min(mv)
            assert all(m > 10.0 * t for m, t in zip(mv, d.tol)), (c.id, mut, mv, d.tol)
        print(f"{c.id}: model {max(d.model_err):.2e} tol {max(d.tol):.2e} " +
              " ".join(f"{n} {v:.2e}" for n, v in moved.items()))


# ------------------------------------------------------------------ CPU: plan coverage (plan-only mode)
def test_plan_coverage():
    """Which kernel, tile, ring depth, FL bits, DMA form and class every case selects, proved without a GPU;
    and the reached set holds every selection the family has."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    bad, seen = [], set()
    for c in CASES:
        rc, plan = plan_only3(c)
        if rc != 0 or not plan_ok(c, plan):
            bad.append((c.id, rc, plan, c.want, c.fl, c.buf, c.label))
            continue
        kind, fl = co.KINDS[plan[0]], plan[5]
        if kind == "conv3i":
            seen.add(("conv3i", plan[1], plan[2]))
            seen.add(("st", plan[3]))
            for name, bit in (("SWAP", C3I_SWAP), ("RES", C3I_RES), ("BUF", C3I_BUF), ("UPH", C3I_UPH), ("UPC", C3I_UPC)):
                seen.add((name, bool(fl & bit)))
            if fl & C3I_RES:
                seen.add(("RES", plan[1]))
        elif kind == "conv3":
            seen.add(("conv3", plan[7]))
        else:
            seen.add((kind, c.C))
            seen.add((kind, "buf", plan[6]))
    assert not bad, bad[:10]
    need = {("conv3r", 64), ("conv3r", 128), ("conv3w", 64), ("conv3w", "buf", 0), ("conv3w", "buf", 1), ("conv3", 6),
            ("conv3", 7), ("conv3", 11), ("st", 2), ("st", 3), ("RES", 256), ("RES", 128)}
    need |= {("conv3i", BM, BN) for (BM, BN, _, _) in C3I_FORCE.values()}
    need |= {(n, v) for n in ("SWAP", "RES", "BUF", "UPH", "UPC") for v in (False, True)}
    assert need <= seen, need - seen


def test_rbfuse_served_query():
    """The served-query answers true, with the designed band height and strip width, for every rbfuse case; false
    for W = 192, W = 320 at Cin 64, and wr missing at Cin 128."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    for c in RB_CASES:
        assert rb_query(c) == (1, [c.rb, c.sw]), (c.id, rb_query(c))
    c64, c128 = mkrb("bf16", 2, 3, 256, 64, 1), mkrb("bf16", 2, 3, 320, 128, 1)
    assert rb_query(c64) == (1, [1, 128]) and rb_query(c128) == (1, [1, 64])
    assert rb_query(c64, W=192)[0] == 0 and rb_query(c128, W=192)[0] == 0
    assert rb_query(c64, W=320)[0] == 0
    assert rb_query(c128, wr=False)[0] == 0
    assert set(c.rb for c in RB_CASES) == {1, 2, 3}


def test_bad_arguments_are_refused_before_any_device_work():
    """Runs without a GPU: both hooks answer DAC_E_ARG from their checks (or from a plan of kind none), ahead of
    the first HIP call; afterwards the process's knobs are what they were."""
    if not co._have_lib():
        pytest.skip("libdaclip_hip.so not built")
    from daclip_amd import _lib
    L, E, p = _lib.lib(), _lib.DAC_E_ARG, DUMMY
    plan = (ctypes.c_int * 8)()

    def call(e=(0, 72), x2=None, w=p, y=p, w2=None, y2=None, **kw):
        f = dict(dtype=_lib.DAC_BF16, kh=3, B=2, Hs=4, Ws=256, up=0, C1=128, Cin=128, ld1=128, ld2=0, Cout=64, K=1152, ldy=64,
                 act=0, cwrap=0, ksplit=0, ss_ld=0, ldr1=0, ldr2=0, bb_ld=0, conv3_force=_lib.DAC_CONV_KEEP,
                 conv2_force=_lib.DAC_CONV_KEEP, conv2_force32=_lib.DAC_CONV_KEEP)
        f.update(kw)
        ds = _lib.DacConvDesc(**f)
        ex = None if e is None else ctypes.byref(_lib.DacConvExt(uph=e[0], ldy2=e[1]))
        return L.dac_op_conv_ex(ctypes.byref(ds), ex, p, x2, w, None, None, None, None, None, None, None, y, w2, y2, plan, None)
    assert L.dac_op_conv_ex(None, None, p, None, p, None, None, None, None, None, None, None, p, None, None, plan, None) == E
    assert call(y=None) == 0 and co.plan_key(list(plan)) == OWN("conv3r")
    assert call(e=None, y=None) == 0 and co.plan_key(list(plan)) == OWN("conv3r")       # e == NULL: dac_op_conv
    assert call(y=None, w2=p, y2=p) == 0 and co.plan_key(list(plan)) == OWN("conv3r")
    before = list(plan)
    assert call(y=None, conv3_force=40) == 0 and co.plan_key(list(plan)) == ("conv3i", 256, 64, 2, MIN)
    assert call(y=None, w2=p, y2=p) == 0 and list(plan) == before                       # the override did not stick
    up = dict(Hs=8, Ws=64, up=1, C1=64, Cin=64, ld1=64)
    assert call(e=(1, 0), y=None, K=768, **up) == 0 and plan[5] & C3I_UPH and not plan[5] & C3I_UPC
    assert call(e=(2, 0), y=None, K=1024, **up) == 0 and plan[5] & C3I_UPC
    for kw in (dict(w=None), dict(y2=p), dict(w2=p), dict(e=None, w2=p, y2=p), dict(e=(0, 63), w2=p, y2=p),
               dict(e=(0, 68), w2=p, y2=p),                                             # y2 rows not 16-byte
               dict(w2=p, y2=p, conv3_force=0), dict(w2=p, y2=p, conv3_force=40), dict(w2=p, y2=p, dtype=_lib.DAC_F32),
               dict(w2=p, y2=p, kh=1, K=128), dict(w2=p, y2=p, Ws=192),                 # no fusing kernel at 192 columns
               dict(w2=p, y2=p, Cout=48, ldy=48), dict(e=(3, 0)), dict(e=(-1, 0)), dict(e=(1, 0)), dict(e=(2, 0)),
               dict(e=(1, 0), K=768, **dict(up, up=0)), dict(e=(1, 0), K=1024, **up), dict(e=(2, 0), K=768, **up),
               dict(e=(0, 0), K=768, **up), dict(e=(1, 0), K=768, dtype=_lib.DAC_F32, **up),
               dict(e=(1, 0), K=768, conv3_force=0, **up), dict(e=(2, 0), K=1024, **dict(up, Ws=32)),
               dict(e=(1, 0), K=768, **dict(up, Hs=1)),                                 # 2 output rows: half a parity tile pair
               dict(e=(1, 0), K=768, ksplit=2, **up), dict(e=(1, 0), K=768, cwrap=32, **up),
               dict(e=(1, 0), K=768, w2=p, y2=p, **up), dict(e=(1, 0), K=768, Cout=48, ldy=48, **up)):
        assert call(**kw) == E, kw
    # dac_op_rbfuse
    c = mkrb("bf16", 2, 3, 256, 64, 1)
    d = rb_layout(c)
    all_ = lambda n: DUMMY if n != "x2" else None
    assert rb_hook(c, d, all_, None) == (0, [-1, -1])                                   # wr with Cin 64: not served
    assert rb_hook(c, d, all_, DUMMY)[0] == E
    ok = lambda n: DUMMY if n not in ("x2", "wr") else None
    assert rb_hook(c, d, ok, None) == (1, [1, 128])
    for miss in ("x1", "w1", "w2", "ssp"):
        assert rb_hook(c, d, lambda n: None if n == miss else ok(n), DUMMY)[0] == E, miss
    assert rb_hook(c, d, lambda n: ctypes.c_void_p((1 << 20) + 4) if n == "ssp" else ok(n), DUMMY)[0] == E
    for kw in (dict(dtype=_lib.DAC_F32), dict(dtype=_lib.DAC_FP8), dict(B=0), dict(H=0), dict(W=-256), dict(W=192), dict(W=320),
               dict(W=128), dict(Cin=96, C1=96, ld1=96), dict(Cin=128), dict(ld1=56), dict(ld1=68), dict(ldy=63), dict(ldy=68),
               dict(ss_ld=-4), dict(ss_ld=130), dict(C1=0), dict(B=1 << 20, H=1 << 10, W=1 << 10)):
        assert rb_hook(c, d, ok, DUMMY, **kw)[0] == E, kw
    two = lambda n: DUMMY
    for kw in (dict(Cin=128, W=320, ld2=56), dict(Cin=128, W=320, ld2=68), dict(Cin=128, W=320, ld2=64, C1=32, ld1=32),
               dict(Cin=128, W=288, ld2=64)):
        assert rb_hook(c, d, two, DUMMY, **kw)[0] == E, kw
    assert rb_hook(c, d, two, None, Cin=128, W=320, ld2=96) == (1, [1, 64])
    assert rb_hook(c, d, lambda n: None if n == "wr" else DUMMY, DUMMY, Cin=128, W=320, ld2=96)[0] == E


# ------------------------------------------------------------------ GPU
class Device:
    """Uploads with slack rows after every activation; guarded outputs."""

    def __init__(self, T):
        self.T, self.keep = T, []

    def up(self, t, slack=False):
        if t is None:
            return None
        t2 = t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t
        if slack:
            t2 = torch.cat([t2, torch.full((GUARD, t2.shape[1]), 1000.0, dtype=t2.dtype)], 0)
        g = t2.contiguous().cuda()
        self.keep.append(g)
        return ctypes.c_void_p(g.data_ptr())

    def out(self, M, ld):
        sentinel = torch.full((M + GUARD, ld), -1234.0, dtype=self.T)
        return sentinel, sentinel.cuda()

    def check(self, what, sentinel, y, M, n):
        """The guard band of y [M + GUARD, ld] is bit-unchanged; -> the [M, n] payload on the CPU."""
        out = y.cpu()
        keep = torch.ones_like(sentinel, dtype=torch.bool)
        keep[:M, :n] = False
        bits = lambda t: t.view(torch.int16 if self.T != torch.float32 else torch.int32)
        assert torch.equal(bits(out)[keep], bits(sentinel)[keep]), (what, "guard band written")
        return out[:M, :n]


def hip_error(what):
    # DAC_E_HIP: the context is gone; nothing more may run on this GPU from this process
    pytest.exit(f"{what}: HIP error", returncode=3)


def run_gpu3(c, d):
    """-> (y [B, HW, Cout], y2 or None, executed plan)."""
    dev = Device(TDT[c.dt])
    g = SimpleNamespace(**d.__dict__)
    g.res1, g.res2 = co_pitched(d.res1, d.ldr1), co_pitched(d.res2, d.ldr2)
    g.bbias = co_pitched(d.bbias, d.bb_ld)
    slack = {id(t) for t in (g.x1, g.x2, g.res1, g.res2)}
    sy, y = dev.out(d.M, d.ldy)
    sy2, y2 = dev.out(d.M, d.ldy2) if c.y2 else (None, None)
    rc, plan = hook3(c, g, lambda t: dev.up(t, id(t) in slack), ctypes.c_void_p(y.data_ptr()),
                     ctypes.c_void_p(y2.data_ptr()) if c.y2 else None)
    if rc == -5:
        hip_error(c.id)
    assert rc == 0, (c.id, rc)
    torch.cuda.synchronize()
    out = dev.check(c.id, sy, y, d.M, c.Cout).reshape(c.B, -1, c.Cout)
    out2 = dev.check(c.id + " y2", sy2, y2, d.M, c.Cout).reshape(c.B, -1, c.Cout) if c.y2 else None
    return out, out2, plan


def co_pitched(t, ld):
    return None if t is None else pitched(t, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_conv3x3_matches_fp64_reference(cid):
    c = BY_ID[cid]
    d = make3(cid)
    rc, planned = plan_only3(c)
    assert rc == 0 and plan_ok(c, planned), (planned, c.want, c.fl, c.buf, c.label)
    y, y2, executed = run_gpu3(c, d)
    assert executed == planned, (executed, planned)
    assert torch.isfinite(y).all()
    err = co.rel_err(y, d.ref)
    ratio = max(e / t for e, t in zip(err, d.tol))
    line = f"CONV3 {c.fam} {c.id}: model {max(d.model_err):.2e} kernel {max(err):.2e} kernel/bound {ratio:.2f}"
    ok = all(e <= t for e, t in zip(err, d.tol))
    if c.y2:
        assert torch.isfinite(y2).all()
        err2 = co.rel_err(y2, d.ref2)
        r2 = max(e / t for e, t in zip(err2, d.tol2))
        line += f" | y2: model {max(d.model_err2):.2e} kernel {max(err2):.2e} kernel/bound {r2:.2f}"
        ok = ok and all(e <= t for e, t in zip(err2, d.tol2))
    print(line)
    assert ok, line


def launch(dev, dt, B, H, W, x1, x2, C1, Cin, ld1, ld2, w, ss, ss_ld, res1, ldr1, y, ldy, w2=None, y2=None, ldy2=0):
    """One plain 64-output 3x3 SiLU launch of the pair rbfuse replaces (device pointers)."""
    from daclip_amd import _lib
    ds = _lib.DacConvDesc(dtype={"bf16": _lib.DAC_BF16, "fp16": _lib.DAC_F16}[dt], kh=3, B=B, Hs=H, Ws=W, up=0, C1=C1, Cin=Cin,
                          ld1=ld1, ld2=ld2, Cout=64, K=9 * Cin, ldy=ldy, act=SILU, cwrap=0, ksplit=0, ss_ld=ss_ld, ldr1=ldr1,
                          ldr2=0, bb_ld=0, conv3_force=-1, conv2_force=_lib.DAC_CONV_KEEP, conv2_force32=_lib.DAC_CONV_KEEP)
    ex = _lib.DacConvExt(uph=0, ldy2=ldy2)
    plan = (ctypes.c_int * _lib.DAC_CONV_PLAN_N)()
    rc = _lib.lib().dac_op_conv_ex(ctypes.byref(ds), ctypes.byref(ex), x1, x2, w, None, ss, res1, None, None, None, None, y, w2,
                                   y2, plan, None)
    if rc == -5:
        hip_error("rbfuse pair")
    # (block2 at a width conv3r's 128-column strips do not divide goes to conv3w, as in the network)
    assert rc == 0 and co.KINDS[plan[0]] == ("conv3r" if Cin == 128 or W % 128 == 0 else "conv3w"), (rc, list(plan))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in RB_CASES])
def test_rbfuse_matches_fp64_reference_and_the_pair(cid):
    c = RB_BY_ID[cid]
    d = make_rb(cid)
    T = TDT[c.dt]
    assert rb_query(c) == (1, [c.rb, c.sw])
    dev = Device(T)
    ptrs = {n: dev.up(getattr(d, n), n in ("x1", "x2")) for n in ("x1", "x2", "w1", "w2", "wr", "ssp")}
    sy, y = dev.out(d.M, d.ldy)
    rc, geom = rb_hook(c, d, lambda n: ptrs[n], ctypes.c_void_p(y.data_ptr()))
    if rc == -5:
        hip_error(c.id)
    assert rc == 0, (c.id, rc)
    assert geom == [c.rb, c.sw], (geom, c.rb, c.sw)
    torch.cuda.synchronize()
    out = dev.check(c.id, sy, y, d.M, 64)
    # The pair: block1 (with the fused res_conv at Cin 128) into h, block2 + residual.
    sh, h = dev.out(d.M, 64)
    sp, yp = dev.out(d.M, d.ldy)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    if c.C == 128:
        sr, r = dev.out(d.M, 72)
        launch(dev, c.dt, c.B, c.H, c.W, ptrs["x1"], ptrs["x2"], c.C1, c.C, d.ld1, d.ld2, ptrs["w1"], ptrs["ssp"], d.ss_ld, None, 0,
               P(h), 64, ptrs["wr"], P(r), 72)
        launch(dev, c.dt, c.B, c.H, c.W, P(h), None, 64, 64, 64, 0, ptrs["w2"], None, 0, P(r), 72, P(yp), d.ldy)
        dev.check(c.id + " pair res", sr, r, d.M, 64)
    else:
        launch(dev, c.dt, c.B, c.H, c.W, ptrs["x1"], None, 64, 64, d.ld1, 0, ptrs["w1"], ptrs["ssp"], d.ss_ld, None, 0, P(h), 64)
        launch(dev, c.dt, c.B, c.H, c.W, P(h), None, 64, 64, 64, 0, ptrs["w2"], None, 0, ptrs["x1"], d.ld1, P(yp), d.ldy)
    torch.cuda.synchronize()
    pair = dev.check(c.id + " pair", sp, yp, d.M, 64)
    # rbfuse repeats conv3r's ordered sums, so it equals a pair of conv3r launches bit for bit. Where block2 of
    # the pair is conv3w (W % 128 != 0: another summation order) the pair has to meet the fused block's bound.
    if c.W % 128 == 0:
        assert torch.equal(out.view(torch.int16), pair.view(torch.int16)), (c.id, "the fused block differs from the pair")
    else:
        perr = co.rel_err(pair.reshape(c.B, -1, 64), d.ref)
        assert all(e <= t for e, t in zip(perr, d.tol)), (c.id, "pair", perr, d.tol)
    yv = out.reshape(c.B, -1, 64)
    assert torch.isfinite(yv).all()
    err = co.rel_err(yv, d.ref)
    ratio = max(e / t for e, t in zip(err, d.tol))
    line = f"CONV3 rbfuse {c.id}: model {max(d.model_err):.2e} kernel {max(err):.2e} kernel/bound {ratio:.2f}"
    print(line)
    assert all(e <= t for e, t in zip(err, d.tol)), line
