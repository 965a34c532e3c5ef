"""CPU tests of the weight packing the engine ships (csrc/pack.h) through the host-only C ABI hook
dac_op_pack: no GPU is touched. The Python packers of test_conv_ops (which build the operands of
the op-level conv tests) are pinned to the product bit for bit; the codecs are compared with
torch's casts on every 16-bit pattern and every midpoint; the sum-keeping rounding, the phase
folds, the MX e4m3 packers, the LayerNorm fold and the LinearAttention fold are checked against
their definitions, written here independently in torch.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from test_conv_ops import geglu_gs_rows, geglu_rows, pack_dual_tap, pack_plain, pack_rowtap  # noqa: E402

T16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
TDT = dict(T16, fp32=torch.float32)


def _lib():
    from daclip_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdaclip_hip.so not built")
    return _lib


def _code(dt):
    L = _lib()
    return {"bf16": L.DAC_BF16, "fp16": L.DAC_F16, "fp32": L.DAC_F32, "e4m3": L.DAC_FP8}[dt]


def raw_pack(layout, dt, w, gain=None, beta=None, bias=None, out=True, shrink=None, **kw):
    """(rc, [three uint8 tensors of exactly the queried sizes]). out=False: the size query only.
    shrink=i: output i is offered one byte less than needed."""
    L = _lib()
    f = dict(layout=layout, dtype=dt if isinstance(dt, int) else _code(dt), round=0, O=0, C=0, kh=0, kw=0, kwp=0,
             F=0, I=0, K=0, flag=0, scale=1.0)
    f.update(kw)
    d = L.DacPackDesc(**f)
    need = (ctypes.c_size_t * 3)()
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = L.lib().dac_op_pack(ctypes.byref(d), None, None, None, None, None, None, need)
    if rc != 0 or not out:
        return rc, list(need)
    keep = [t if t is None else t.contiguous().float() for t in (w, gain, beta, bias)]
    cap = [n - 1 if shrink == i else n for i, n in enumerate(need)]
    bufs = [torch.full((max(c, 0),), 0xA5, dtype=torch.uint8) for c in cap]
    outs = (ctypes.c_void_p * 3)(*[b.data_ptr() if b.numel() else None for b in bufs])
    rc = L.lib().dac_op_pack(ctypes.byref(d), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), outs,
                             (ctypes.c_size_t * 3)(*cap), need)
    return rc, bufs


def pack(layout, dt, w, **kw):
    rc, bufs = raw_pack(layout, dt, w, **kw)
    assert rc == 0, (layout, dt, kw, rc)
    return bufs


def bits(t, dt):
    """The stored bits of a float tensor cast (RNE) to dt, flat."""
    return t.to(TDT[dt]).contiguous().view(torch.int32 if dt == "fp32" else torch.int16).reshape(-1)


def stored(buf, dt):
    return buf.view(torch.int32 if dt == "fp32" else torch.int16)


def pad_c(W, cin):
    P = torch.zeros(W.shape[0], cin, *W.shape[2:], dtype=W.dtype)
    P[:, :W.shape[1]] = W
    return P


# ------------------------------------------------------------------ Python packers vs the product
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_plain_layouts_match_product(dt):
    L = _lib()
    g = torch.Generator().manual_seed(11)
    ve = 4 if dt == "fp32" else 8
    # 3x3 with C = 12 (pads to 16 in 16 bit, stays 12 in fp32) and a 1x1; operands already in T.
    for (O, C, k) in ((5, 12, 3), (3, 20, 1)):
        W = torch.randn(O, C, k, k, generator=g).to(TDT[dt]).float()
        cin = (C + ve - 1) // ve * ve
        got = stored(pack(L.DAC_PACK_CONV, dt, W, O=O, C=C, kh=k, kw=k)[0], dt)
        assert torch.equal(got, bits(pack_plain(pad_c(W, cin)), dt))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_rowtap_and_dual_layouts_match_product(dt):
    L = _lib()
    T = T16[dt]
    g = torch.Generator().manual_seed(12)
    split = lambda W: (W.to(T).float(), (W - W.to(T).float()).to(T).float())     # cast, cast of the remainder
    # 7x7, C = 6 -> 8, kernel rows padded to 8 taps: plain (operands in T) and split precision.
    W = torch.randn(4, 6, 7, 7, generator=g)
    Wt = W.to(T).float()
    got = stored(pack(L.DAC_PACK_CONV, dt, Wt, O=4, C=6, kh=7, kw=7, kwp=8)[0], dt)
    assert torch.equal(got, bits(pack_rowtap([pad_c(Wt, 8)]), dt))
    hi, lo = split(W)
    assert lo.abs().max() > 0
    got = stored(pack(L.DAC_PACK_DUAL, dt, W, O=4, C=6, kh=7, kw=7, kwp=8)[0], dt)
    assert torch.equal(got, bits(pack_rowtap([pad_c(hi, 8), pad_c(lo, 8)]), dt))
    # [hi C | lo C] per tap: 3x3 C = 64 O = 3, and 1x1.
    for (O, C, k) in ((3, 64, 3), (5, 16, 1)):
        W = torch.randn(O, C, k, k, generator=g)
        hi, lo = split(W)
        got = stored(pack(L.DAC_PACK_DUAL, dt, W, O=O, C=C, kh=k, kw=k)[0], dt)
        assert torch.equal(got, bits(pack_dual_tap(hi, lo), dt))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("Fo", [64, 96])
def test_geglu_orders_match_product(dt, Fo):
    L = _lib()
    g = torch.Generator().manual_seed(13)
    I = 8
    W = torch.randn(2 * Fo, I, generator=g).to(TDT[dt]).float()
    b = torch.randn(2 * Fo, generator=g)
    for layout, rows in ((L.DAC_PACK_GEGLU, geglu_rows(Fo)), (L.DAC_PACK_GEGLU_GS, geglu_gs_rows(Fo))):
        w_o, b_o, r_o = pack(layout, dt, W, bias=b, F=Fo, I=I)
        assert torch.equal(r_o.view(torch.int32).long(), rows)
        assert torch.equal(stored(w_o, dt), bits(W[rows], dt))
        assert torch.equal(b_o.view(torch.float32), b[rows])


def test_concat_transpose_and_emulation():
    L = _lib()
    g = torch.Generator().manual_seed(14)
    W = torch.randn(3, 4, 8, generator=g)                       # q | k | v, each [4][8]
    s = 0.2550348616841918
    want = W.clone()
    want[0] *= torch.tensor(s, dtype=torch.float32)
    for dt in ("bf16", "fp16", "fp32"):
        got = stored(pack(L.DAC_PACK_CONCAT, dt, W, K=3, O=4, I=8, scale=s)[0], dt)
        assert torch.equal(got, bits(want, dt))
    M = torch.randn(5, 7, generator=g)
    assert torch.equal(pack(L.DAC_PACK_TRANSPOSE, "fp32", M, I=5, O=7)[0].view(torch.float32).reshape(7, 5), M.t())
    # The fp32 handles' f16 probe: 11 significant bits = the f16 cast for values in f16's normal range.
    x = torch.randn(4096, generator=g) * 3
    x = x[x.abs() > 1e-3]
    got = pack(L.DAC_PACK_EMU_FP16, "fp32", x, O=x.numel())[0].view(torch.float32)
    assert torch.equal(got, x.half().float())


# ------------------------------------------------------------------ codecs
def _patterns16(dt):
    p = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = p.view(T16[dt]).float()
    ok = torch.isfinite(v)
    return p[ok], v[ok]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_codec16_equals_torch_cast(dt):
    L = _lib()
    p, v = _patterns16(dt)
    enc = lambda x: pack(L.DAC_PACK_CODEC, dt, x, O=x.numel())[0].view(torch.int16)
    # Every finite pattern (+-0 and the f16 subnormals among them) encodes to itself and decodes back.
    assert torch.equal(enc(v), p)
    dec = pack(L.DAC_PACK_CODEC, dt, v, O=v.numel(), flag=1)[0].view(torch.float32)
    assert torch.equal(dec.view(torch.int32), v.view(torch.int32))
    # Every midpoint of adjacent finite values (exact in fp32: one more significant bit), and the one
    # above the largest finite value, which rounds to infinity.
    pos = torch.sort(v[v >= 0].double()).values
    step = pos[-1] - pos[-2]
    mid = torch.cat([(pos[1:] + pos[:-1]) / 2, (pos[-1:] + step / 2)]).float()
    assert torch.equal(mid.double(), torch.cat([(pos[1:] + pos[:-1]) / 2, (pos[-1:] + step / 2)]))
    for x in (mid, -mid, torch.nextafter(mid, torch.zeros(())), torch.nextafter(mid, torch.full((), float("inf")))):
        assert torch.equal(enc(x), bits(x, dt))
    edge = torch.tensor([0.0, -0.0, 65519.99, 65520.0, -65519.99, -65520.0, 6e-8, 2.9e-8, 3.0e-8, 1e-9, 3.3e38, -3.4e38])
    assert torch.equal(enc(edge), bits(edge, dt))
    g = torch.Generator().manual_seed(15)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-30, 20, (1 << 16,), generator=g).float())
    assert torch.equal(enc(x), bits(x, dt))


def _e4m3_value(c):
    E, q = (c >> 3) & 15, c & 7
    v = (1 + q / 8) * 2.0 ** (E - 7) if E else q / 8 * 2.0 ** -6
    return -v if c & 0x80 else v


def test_codec_e4m3():
    L = _lib()
    enc = lambda x: pack(L.DAC_PACK_CODEC, "e4m3", x, O=x.numel())[0]
    codes = [c for c in range(256) if c & 0x7f != 0x7f]                    # all but the two NaNs
    vals = torch.tensor([_e4m3_value(c) for c in codes], dtype=torch.float32)
    assert vals.abs().max() == 448
    assert enc(vals).tolist() == codes                                      # every code round-trips
    dec = pack(L.DAC_PACK_CODEC, "e4m3", vals, O=vals.numel(), flag=1)[0].view(torch.float32)
    assert torch.equal(dec.view(torch.int32), vals.view(torch.int32))
    # Midpoints of adjacent codes tie to the even code; just beside them the nearer code wins.
    pc = [c for c in codes if c < 0x7f]
    pv = torch.tensor([_e4m3_value(c) for c in pc], dtype=torch.float64)
    mid = ((pv[1:] + pv[:-1]) / 2).float()
    even = [a if a % 2 == 0 else b for a, b in zip(pc[:-1], pc[1:])]
    assert enc(mid).tolist() == even and enc(-mid).tolist() == [c | 0x80 for c in even]
    assert enc(torch.nextafter(mid, torch.zeros(()))).tolist() == pc[:-1]
    assert enc(torch.nextafter(mid, torch.full((), 1e9))).tolist() == pc[1:]
    # Saturation: [448, 464) rounds to 448, everything from 464 up (infinities too) saturates to it.
    x = torch.tensor([448.0, 455.9, 463.99, 464.0, 465.0, 1e6, 3e38, float("inf")])
    assert enc(x).tolist() == [0x7e] * 8 and enc(-x).tolist() == [0xfe] * 8
    if hasattr(torch, "float8_e4m3fn"):
        g = torch.Generator().manual_seed(16)
        x = torch.cat([vals, mid, -mid, torch.randn(1 << 14, generator=g) * torch.exp2(
            torch.randint(-12, 8, (1 << 14,), generator=g).float())])
        x = x[x.abs() <= 448]
        assert torch.equal(enc(x), x.to(torch.float8_e4m3fn).view(torch.uint8))
    # (A torch without float8_e4m3fn leaves the integer checks above, which define the format.)


# ------------------------------------------------------------------ sum-keeping rounding
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("k", [3, 7])
def test_sum_keeping_rounding(dt, k):
    L = _lib()
    T = T16[dt]
    g = torch.Generator().manual_seed(17)
    O, C, taps = 4, 8, k * k
    W = torch.randn(O, C, k, k, generator=g) * 0.1
    P = pack_plain(W).reshape(O, taps, C)                                   # [O][taps][cin]: no padding at C = 8
    q = pack(L.DAC_PACK_CONV, dt, W, O=O, C=C, kh=k, kw=k, round=1)[0].view(torch.int16).reshape(O, taps, C)
    rne = P.to(T)
    rb = rne.view(torch.int16).int() & 0xffff
    # The neighbour of RNE(w) on w's side: sign-magnitude formats, so one step on the magnitude bits.
    away = (rne.float() > 0) == (P > rne.float())
    other = torch.where(away, rb + 1, rb - 1)
    qb = q.int() & 0xffff
    exact = P == rne.float()
    assert (rne.float() != 0).all()
    assert ((qb == rb) | ((qb == other) & ~exact)).all()
    qv = q.view(T).double()
    e_q = (P.double() - qv).sum(1).abs()
    e_r = (P.double() - rne.double()).sum(1).abs()
    assert (e_q <= e_r).all()
    changed = (qb != rb).any(1)
    frac = changed.float().mean().item()
    print(f"sum-keeping {dt} taps {taps}: groups changed {frac:.2f}, mean |sum err| {e_q.mean():.2e} vs RNE {e_r.mean():.2e}")
    assert frac >= 0.25
    # One tap per group: nothing to trade, plain RNE.
    W1 = torch.randn(O, C, 1, 1, generator=g) * 0.1
    q1 = pack(L.DAC_PACK_CONV, dt, W1, O=O, C=C, kh=1, kw=1, round=1)[0].view(torch.int16)
    assert torch.equal(q1, bits(pack_plain(W1), dt))


# ------------------------------------------------------------------ phase folds
def test_phase_folds():
    L = _lib()
    g = torch.Generator().manual_seed(18)
    O, C = 3, 8
    W = torch.randn(O, C, 3, 3, generator=g) * 0.1
    P = W.permute(0, 2, 3, 1).contiguous()                                  # [O][kh][kw][C]
    row = pack(L.DAC_PACK_UPH_ROW, "fp32", W, O=O, C=C, kh=3, kw=3)[0].view(torch.float32).reshape(O, 4, 3, C)
    col = pack(L.DAC_PACK_UPH_COL, "fp32", W, O=O, C=C, kh=3, kw=3)[0].view(torch.float32).reshape(O, 4, 4, C)
    # Bit-equal to the same float32 sums in the same order.
    want = torch.stack([P[:, 0], P[:, 1] + P[:, 2], P[:, 0] + P[:, 1], P[:, 2]], 1)
    assert torch.equal(row, want)
    sets = ((0,), (1, 2), (0, 1), (2,))
    for rs in range(4):
        for cs in range(4):
            v = torch.zeros(O, C)
            for kh in sets[rs]:
                for kw in sets[cs]:
                    v = v + P[:, kh, kw]
            assert torch.equal(col[:, rs, cs], v), (rs, cs)
    # ... and in 16 bits they are those sums rounded once.
    for dt in ("bf16", "fp16"):
        assert torch.equal(pack(L.DAC_PACK_UPH_ROW, dt, W, O=O, C=C, kh=3, kw=3)[0].view(torch.int16), bits(want, dt))
    # Semantics (fp64): the 3x3 conv over the nearest-2x image = the phase convs over the source, with
    # weights on a 2^-12 grid below 1 so that the folds' fp32 sums of up to four taps are exact.
    W = torch.round(torch.randn(O, C, 3, 3, generator=g) * 0.1 * 4096) / 4096
    row = pack(L.DAC_PACK_UPH_ROW, "fp32", W, O=O, C=C, kh=3, kw=3)[0].view(torch.float32).reshape(O, 4, 3, C)
    col = pack(L.DAC_PACK_UPH_COL, "fp32", W, O=O, C=C, kh=3, kw=3)[0].view(torch.float32).reshape(O, 4, 4, C)
    H, Wd = 4, 5
    x = torch.randn(1, C, H, Wd, generator=g, dtype=torch.float64)
    up = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    ref = F.conv2d(up, W.double(), padding=1)
    rk = row.double().permute(0, 3, 1, 2)                                   # [O][C][4][3]
    xw = x.repeat_interleave(2, 3)                                          # columns still upsampled
    y = torch.empty_like(ref)
    y[:, :, 0::2] = F.conv2d(F.pad(xw, (1, 1, 1, 0)), rk[:, :, 0:2])        # rows (i-1, i)
    y[:, :, 1::2] = F.conv2d(F.pad(xw, (1, 1, 0, 1)), rk[:, :, 2:4])        # rows (i, i+1)
    assert (y - ref).abs().max() <= 1e-12
    ck = col.double().permute(0, 3, 1, 2)                                   # [O][C][4][4]
    y2 = torch.empty_like(ref)
    for pr in (0, 1):
        for pc in (0, 1):
            pad = ((1, 0) if pc == 0 else (0, 1)) + ((1, 0) if pr == 0 else (0, 1))
            y2[:, :, pr::2, pc::2] = F.conv2d(F.pad(x, pad), ck[:, :, 2 * pr:2 * pr + 2, 2 * pc:2 * pc + 2])
    assert (y2 - ref).abs().max() <= 1e-12


# ------------------------------------------------------------------ MX e4m3 packers
def _check_mx_blocks(w_blocks, codes, expo):
    """w_blocks [n][len] fp32, codes [n][len] uint8, expo [n] uint8: the exponent rule and the bytes."""
    L = _lib()
    e = expo.int() - 127
    mx = w_blocks.abs().max(1).values.double()
    zero = mx == 0
    assert (e[zero] == 0).all() and zero.any()
    free = ~zero & (e > -126) & (e < 126)                                   # not clamped
    assert torch.equal(free, ~zero)                                         # (none is, at these magnitudes)
    assert (mx[free] / torch.exp2(e[free].double()) <= 448).all()
    assert (mx[free] / torch.exp2(e[free].double() - 1) > 448).all()
    scaled = (w_blocks * torch.exp2(-e.float())[:, None]).reshape(-1)       # exact: a power of two
    want = pack(L.DAC_PACK_CODEC, "e4m3", scaled, O=scaled.numel())[0]
    assert torch.equal(codes.reshape(-1), want)


def test_make_fp8():
    L = _lib()
    g = torch.Generator().manual_seed(19)
    O, K = 3, 192
    W = torch.randn(O, K, generator=g) * torch.exp2(torch.randint(-12, 6, (O, K // 64, 1), generator=g).float()).expand(
        O, K // 64, 64).reshape(O, K)
    W[1, 64:128] = 0                                                        # an all-zero block
    W[2, 0] = 448 * 8.0                                                     # a block maximum exactly at 448 * 2^e
    w8, s8, kp = pack(L.DAC_PACK_FP8, "e4m3", W, O=O, K=K)
    assert kp.view(torch.int32).item() == 256
    w8, s8 = w8.reshape(O, 256), s8.reshape(O, 4)
    assert (w8[:, K:] == 0).all() and (s8[:, 3] == 127).all()               # K padded to 128s: zero bytes, e = 0
    assert s8[2, 0] == 127 + 3
    _check_mx_blocks(W.reshape(O * 3, 64), w8[:, :K].reshape(O * 3, 64), s8[:, :3].reshape(-1))


def test_make_q8c3():
    L = _lib()
    g = torch.Generator().manual_seed(20)
    W = torch.randn(64, 64, 3, 3, generator=g) * torch.exp2(torch.randint(-10, 4, (64, 1, 3, 3), generator=g).float())
    W[5, 32:, 1, 2] = 0                                                     # (n = 5, tap 5, upper half): all zero
    w8, s8, _ = pack(L.DAC_PACK_Q8C3, "e4m3", W, O=64, C=64, kh=3, kw=3)
    P = pack_plain(W).reshape(64 * 9 * 2, 32)                               # [n][tap][half][32]
    assert s8.numel() == 64 * 18 and s8.reshape(64, 9, 2)[5, 5, 1] == 127
    _check_mx_blocks(P, w8.reshape(-1, 32), s8)


# ------------------------------------------------------------------ LayerNorm fold
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("with_beta,with_pb", [(True, True), (False, False), (True, False)])
def test_fold_ln(dt, with_beta, with_pb):
    L = _lib()
    T = T16[dt]
    g = torch.Generator().manual_seed(21)
    O, K = 6, 32
    # |p g| in [0.24, 1.08]: every stored w' is a multiple of 2^-13 (f16's ulp in [0.125, 0.25)) and a row's sum
    # is below 64, so cs is exact in fp32 and the identity below holds to fp64 rounding.
    sgn = torch.where(torch.rand(O, K, generator=g) < 0.5, -1.0, 1.0)
    p = sgn * (0.3 + 0.6 * torch.rand(O, K, generator=g))
    gain = 0.8 + 0.4 * torch.rand(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g) if with_beta else None
    pb = 0.1 * torch.randn(O, generator=g) if with_pb else None
    w_o, cs_o, b_o = pack(L.DAC_PACK_FOLD_LN, dt, p, gain=gain, beta=beta, bias=pb, O=O, K=K)
    wq = w_o.view(torch.int16).reshape(O, K)
    assert torch.equal(wq.reshape(-1), bits(p * gain, dt))                  # dec(w') = RNE(p g)
    wd = wq.view(T).double()
    cs, bias = torch.zeros(O, dtype=torch.float64), (pb.double() if with_pb else torch.zeros(O, dtype=torch.float64))
    for k in range(K):                                                      # the sums in fp64, in k order
        cs = cs + wd[:, k]
        if with_beta:
            bias = bias + p[:, k].double() * beta[k].double()
    assert torch.equal(cs_o.view(torch.float32), cs.float())
    assert torch.equal(cs_o.view(torch.float32).double(), cs)               # exact by the construction above
    assert torch.equal(b_o.view(torch.float32), bias.float())
    # LN(x) p^T + pb = rstd (x w'^T - mean cs) + bias', with LN0 the LayerNorm without gain; rows 50 sigma off zero.
    x = 50.0 + torch.randn(16, K, generator=g, dtype=torch.float64)
    mu = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    bf = b_o.view(torch.float32).double()
    lhs = rstd * (x @ wd.t() - mu * cs_o.view(torch.float32).double()) + bf
    rhs = ((x - mu) * rstd) @ wd.t() + bf
    assert (lhs - rhs).abs().max() <= 1e-9


# ------------------------------------------------------------------ LinearAttention gain fold
def test_la_gain_fold():
    L = _lib()
    g = torch.Generator().manual_seed(22)
    O, C = 12, 16
    W = torch.randn(O, C, generator=g) * 0.2
    gain = 1 + 0.3 * torch.randn(C, generator=g)
    W[7] *= 50                                                              # a large k row: not in the bound

    def fold(Wx, flag, dt="fp32"):
        w_o, s_o, _ = pack(L.DAC_PACK_LA_FOLD, dt, Wx, gain=gain, O=O, C=C, flag=flag)
        return w_o, s_o.view(torch.float32).item()

    def bound(Wx):
        wg = (Wx * gain).double()                                           # the fp32 products
        return 1.01 * wg[:O // 3].norm(dim=1).max().item() * C ** 0.5 + 0.05

    w_o, s = fold(W, 1)
    assert torch.equal(w_o.view(torch.float32).reshape(O, C), W * gain)
    b = bound(W)
    assert 0.05 < b < 40 and s == torch.tensor(b, dtype=torch.float64).float().item()
    assert abs(s - b) <= 2e-7 * b
    assert fold(W, 0)[1] == 0.0                                             # knob off
    big = W * (41 / b)
    assert bound(big) > 40 and fold(big, 1)[1] == 0.0                       # past e^-80's range: no shift
    for dt in ("bf16", "fp16"):
        assert torch.equal(fold(W, 1, dt)[0].view(torch.int16), bits(W * gain, dt))


# ------------------------------------------------------------------ refusals
def test_refusals():
    L = _lib()
    E = L.DAC_E_ARG
    lib = L.lib()
    W = torch.randn(64 * 64 * 9)
    need = (ctypes.c_size_t * 3)()
    ok = dict(layout=L.DAC_PACK_CONV, dt="bf16", w=W, O=4, C=8, kh=3, kw=3)
    assert raw_pack(**ok)[0] == 0
    d = L.DacPackDesc(layout=L.DAC_PACK_CONV, dtype=L.DAC_BF16, O=4, C=8, kh=3, kw=3, scale=1.0)
    # Null descriptor / size array / weights / outputs / capacities.
    assert lib.dac_op_pack(None, None, None, None, None, None, None, need) == E
    assert lib.dac_op_pack(ctypes.byref(d), None, None, None, None, None, None, None) == E
    buf = torch.zeros(4 * 9 * 8 * 2, dtype=torch.uint8)
    outs = (ctypes.c_void_p * 3)(buf.data_ptr(), None, None)
    cap = (ctypes.c_size_t * 3)(buf.numel(), 0, 0)
    wp = ctypes.c_void_p(W.data_ptr())
    assert lib.dac_op_pack(ctypes.byref(d), wp, None, None, None, outs, cap, need) == 0 and need[0] == buf.numel()
    assert lib.dac_op_pack(ctypes.byref(d), None, None, None, None, outs, cap, need) == E
    assert lib.dac_op_pack(ctypes.byref(d), wp, None, None, None, outs, None, need) == E
    assert lib.dac_op_pack(ctypes.byref(d), wp, None, None, None, (ctypes.c_void_p * 3)(None, None, None), cap, need) == E
    # Unknown layout / dtype / rounding; a dtype the layout does not store.
    for kw in (dict(layout=99), dict(layout=-1), dict(dt=99), dict(dt="e4m3"), dict(round=2), dict(round=-1)):
        assert raw_pack(**dict(ok, **kw))[0] == E, kw
    assert raw_pack(L.DAC_PACK_CODEC, "fp32", W, O=8)[0] == E
    assert raw_pack(L.DAC_PACK_DUAL, "fp32", W, O=4, C=8, kh=3, kw=3)[0] == E
    assert raw_pack(L.DAC_PACK_FOLD_LN, "fp32", W, gain=W, O=4, K=8)[0] == E
    assert raw_pack(L.DAC_PACK_FP8, "bf16", W, O=4, K=64)[0] == E
    assert raw_pack(L.DAC_PACK_TRANSPOSE, "bf16", W, O=4, I=8)[0] == E
    # Non-positive dimensions.
    for kw in (dict(O=0), dict(C=0), dict(kh=0), dict(kw=-3), dict(kwp=-1), dict(O=-4)):
        assert raw_pack(**dict(ok, **kw))[0] == E, kw
    assert raw_pack(L.DAC_PACK_CODEC, "bf16", W, O=0)[0] == E
    assert raw_pack(L.DAC_PACK_GEGLU, "bf16", W, bias=W, F=0, I=8)[0] == E
    assert raw_pack(L.DAC_PACK_GEGLU, "bf16", W, bias=W, F=32, I=0)[0] == E
    assert raw_pack(L.DAC_PACK_FP8, "e4m3", W, O=4, K=0)[0] == E
    assert raw_pack(L.DAC_PACK_CONCAT, "bf16", W, K=0, O=4, I=8)[0] == E
    assert raw_pack(L.DAC_PACK_FOLD_LN, "bf16", W, gain=W, O=4, K=0)[0] == E
    assert raw_pack(L.DAC_PACK_LA_FOLD, "bf16", W, gain=W, O=6, C=0)[0] == E
    # Each layout's own precondition.
    q8 = dict(layout=L.DAC_PACK_Q8C3, dt="e4m3", w=W, O=64, C=64, kh=3, kw=3)
    assert raw_pack(**q8)[0] == 0
    for kw in (dict(O=32), dict(C=32), dict(kh=1, kw=1), dict(kwp=8)):
        assert raw_pack(**dict(q8, **kw))[0] == E, kw
    for lay in (L.DAC_PACK_UPH_ROW, L.DAC_PACK_UPH_COL):
        assert raw_pack(lay, "bf16", W, O=4, C=8, kh=3, kw=3)[0] == 0
        assert raw_pack(lay, "bf16", W, O=4, C=8, kh=1, kw=1)[0] == E
        assert raw_pack(lay, "bf16", W, O=4, C=8, kh=3, kw=3, kwp=8)[0] == E
    assert raw_pack(L.DAC_PACK_GEGLU_GS, "bf16", W, bias=W, F=64, I=8)[0] == 0
    assert raw_pack(L.DAC_PACK_GEGLU_GS, "bf16", W, bias=W, F=48, I=8)[0] == E      # F % 32
    assert raw_pack(L.DAC_PACK_GEGLU, "bf16", W, bias=W, F=48, I=8)[0] == 0
    assert raw_pack(L.DAC_PACK_GEGLU, "bf16", W, bias=W, F=40, I=8)[0] == E         # F % 16
    assert raw_pack(L.DAC_PACK_LA_FOLD, "bf16", W, gain=W, O=8, C=8)[0] == E        # q | k | v rows
    # A required operand that is missing.
    assert raw_pack(L.DAC_PACK_GEGLU, "bf16", W, F=32, I=8)[0] == E
    assert raw_pack(L.DAC_PACK_FOLD_LN, "bf16", W, O=4, K=8)[0] == E
    assert raw_pack(L.DAC_PACK_LA_FOLD, "bf16", W, O=6, C=8)[0] == E
    # A capacity below the queried size, for each output: refused, and nothing is written.
    for i in range(3):
        rc, bufs = raw_pack(L.DAC_PACK_GEGLU, "bf16", W, bias=W, F=32, I=8, shrink=i)
        assert rc == E and all((b == 0xA5).all() for b in bufs)
