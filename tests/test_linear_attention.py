"""Op-level tests of the LinearAttention kernels (csrc/linattn.hip) through the C ABI hooks
dac_op_linear_attention (the fused block, as Engine::linattn_fused launches it) and
dac_op_linear_attention_weff (the unfused context chain), against a plain torch float64
reference written from the model's definition (module_util.py LayerNorm, PreNorm,
LinearAttention; eps 1e-5 in both LayerNorms):

    xn = LN(x);  q|k|v = xn wqkv^T;  q = softmax_d(q) 32^-0.5;  k = softmax_n(k)
    ctx = k v^T / HW;  t = Wout (ctx^T q) + bout;  y = x + LN(t) gout
    W_eff[b][c][h*32+d] = sum_e Wout[c][h*32+e] ctx[b][h][d][e]

Tolerances are not taken from the kernel. A second reference, the "rounding model", is the same
computation in float32 rounded to T where the fused path stores 16 bits (xn, P = exp(k - max)
and V as MFMA operands, W_eff, the softmaxed q, y). With err = max|y - ref64| / max|ref64| per
image, the 16-bit bound is 4 x the model's err (floor: 2 ulp of T at max|ref|); fp32: 1e-5.

Shapes (B = 2 unless noted): HW = 7 (one partial 16-pixel tile), 36 (one partial 64-pixel
tile), 1000 (16 chunks, the last 40 pixels, HW % 16 = 8), 1024 (16 one-tile chunks), 5184
(72x72: 23 empty chunks at C <= 128, 5 at C = 256) and 16384 (B = 1: 4 / 8 tiles per chunk).
Regimes, each defined by a property of the reference's k or q that the CPU precondition test
asserts (together with the sensitivity of y to W_eff x 2, to one extra k = 0 pixel, and to one
dropped chunk partial -- each must move y by more than 10 x the case's tolerance):
  random    independent x entries + per-pixel offset, k spread 2..4           all shapes
  rising    per-channel k rises by >= 20 along the pixels; inside the chunk
            that carries the softmax's weight by < 5.5 per tile on some
            (head, 16-channel) groups and by > 5.5 on others                  16384, 5184
  falling   the mirror image: the first tile holds every channel's max        16384, 5184
  negk      >= 32 k channels with every real k <= -8 (ragged tiles)           7, 36, 1000, 5184
  dominant  in >= 32 k channels one pixel (last tile of a middle chunk)
            exceeds all others by 12..16                                      16384, 1024
  qbound    the engine's q bound lands in 30..40 and pixels reach 0.8 of it   36, 1000
random and qbound run with qshift = 0 and with the bound.

Measured on an MI355X (err as above; the largest over C, the shapes, the images and both
qshift settings of a regime; kernel/bound is the largest ratio of a case's error to its own
bound, 1.0 = at the bound; every test prints the figures of its case). No case exceeded its
bound and no kernel needed a change. Model and kernel often agree to three digits: the largest
error is then the final rounding of y (or W_eff) to T near max|ref|, which both share.
Arithmetic-only mutants of linattn.hip, built aside and run once against these tests, each
failed cases here: padding pixels left in la_proj_ctx's exp sums (random / negk / qbound at
HW = 7, 36, 1000) or in its max (fp16 negk), exp sums not rescaled when the stale max moves
(rising and the 5184 / 16384 shapes, every dtype), a mover factor exp(0.9 d) (fp32, some fp16),
chunk weights exp(0.97 d) in la_combine_weff (rising / falling / random), fp16 wscale off by 2 %.

regime    dtype | fused y: model   kernel  kernel/bound | W_eff chain: model   kernel  kernel/bound
random    bf16  |         7.2e-03  6.5e-03     0.27     |             3.5e-03  3.5e-03     0.25
random    fp16  |         8.5e-04  8.9e-04     0.32     |             4.6e-04  4.6e-04     0.25
random    fp32  |               -  1.2e-06     0.12     |                   -  3.4e-07     0.03
rising    bf16  |         6.2e-03  5.5e-03     0.26     |             3.8e-03  3.8e-03     0.25
rising    fp16  |         8.2e-04  7.4e-04     0.25     |             4.5e-04  4.5e-04     0.25
rising    fp32  |               -  1.8e-06     0.18     |                   -  4.9e-07     0.05
falling   bf16  |         6.2e-03  6.2e-03     0.25     |             3.7e-03  3.7e-03     0.25
falling   fp16  |         7.2e-04  7.0e-04     0.27     |             5.0e-04  5.0e-04     0.25
falling   fp32  |               -  1.3e-06     0.13     |                   -  5.9e-07     0.06
negk      bf16  |         5.5e-03  5.5e-03     0.27     |             3.9e-03  3.9e-03     0.25
negk      fp16  |         7.0e-04  6.9e-04     0.26     |             5.1e-04  5.1e-04     0.25
negk      fp32  |               -  1.1e-06     0.11     |                   -  3.2e-07     0.03
dominant  bf16  |         1.0e-02  1.0e-02     0.26     |             3.0e-03  3.0e-03     0.25
dominant  fp16  |         1.1e-03  1.1e-03     0.28     |             3.8e-04  3.8e-04     0.25
dominant  fp32  |               -  1.9e-06     0.19     |                   -  4.3e-07     0.04
qbound    bf16  |         7.2e-03  7.2e-03     0.27     |                   -        -        -
qbound    fp16  |         7.8e-04  7.1e-04     0.25     |                   -        -        -
qbound    fp32  |               -  1.4e-06     0.14     |                   -        -        -
"""
import ctypes
import functools
import math
import os

import pytest

torch = pytest.importorskip("torch")

EPS = 1e-5
TAU = 5.5                      # la_tau(): the stale-max slack of la_proj_ctx
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MANT = {"bf16": 7, "fp16": 10}
DTC = [(dt, C) for dt in ("bf16", "fp16") for C in (64, 128, 256)] + [("fp32", 64), ("fp32", 128)]
SHAPES = {"random": (7, 36, 1000, 1024, 5184, 16384), "rising": (16384, 5184), "falling": (16384, 5184),
          "negk": (7, 36, 1000, 5184), "dominant": (16384, 1024), "qbound": (36, 1000)}
SR = [(HW, reg) for reg, hws in SHAPES.items() for HW in hws]
CASES = [(dt, C, HW, reg) for (HW, reg) in SR for (dt, C) in DTC]
IDS = [f"{dt}-C{C}-HW{HW}-{reg}" for (dt, C, HW, reg) in CASES]


def _batch(HW):
    return 1 if HW == 16384 else 2


# ------------------------------------------------------------------ chunking (copied from
# linattn.hip la_fused_chunks / la_chunk_px; a change there must show up here).
def fused_chunking(HW, C):
    nc = 32 if C >= 256 else 128 if HW >= 131072 else 64
    nc = min(nc, (HW + 63) // 64, 128)
    ch = ((HW + nc - 1) // nc + 63) // 64 * 64
    used = (HW + ch - 1) // ch
    return nc, ch, nc - used


# ------------------------------------------------------------------ the fp64 reference
def _ln(x):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS)


def ref_qkv(x, wqkv):
    """x [B, HW, C], wqkv [384, C] (any dtype) -> q, k, v [B, HW, 128] float64 (raw projections)."""
    qkv = _ln(x.double()) @ wqkv.double().t()
    return qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]


def ref_context(k, v, extra_zero_pixel=False, drop=None):
    """ctx [B, 4, 32, 32] = softmax_n(k) v^T / HW. extra_zero_pixel: one more pixel with k = 0,
    v = 0 in the softmax (a leaked padding pixel); drop = (p0, p1): those pixels' partial (their
    context and exp sums) left out of the merge."""
    B, HW, _ = k.shape
    if drop is not None:
        keep = torch.ones(HW, dtype=torch.bool, device=k.device)
        keep[drop[0]:drop[1]] = False
        k, v = k[:, keep], v[:, keep]
    m = k.max(dim=1, keepdim=True).values
    if extra_zero_pixel:
        m = m.clamp(min=0.0)
    p = torch.exp(k - m)
    s = p.sum(dim=1, keepdim=True)
    if extra_zero_pixel:
        s = s + torch.exp(-m)
    p = (p / s).view(B, -1, 4, 32)
    return torch.einsum("bnhd,bnhe->bhde", p, v.view(B, -1, 4, 32)) / HW


def ref_weff(ctx, wout):
    B, C = ctx.shape[0], wout.shape[0]
    return torch.einsum("che,bhde->bchd", wout.double().view(C, 4, 32), ctx).reshape(B, C, 128)


def ref_apply(x, q, weff, bout, gout):
    B, HW, _ = q.shape
    qs = torch.softmax(q.view(B, HW, 4, 32), dim=-1).reshape(B, HW, 128) * 32 ** -0.5
    t = qs @ weff.transpose(1, 2) + bout.double()
    return x.double() + _ln(t) * gout.double()


def reference(x, wqkv, wout, bout, gout, weff_scale=1.0, extra_zero_pixel=False, drop=None):
    q, k, v = ref_qkv(x, wqkv)
    weff = ref_weff(ref_context(k, v, extra_zero_pixel, drop), wout)
    return dict(q=q, k=k, v=v, weff=weff, y=ref_apply(x, q, weff * weff_scale, bout, gout))


# ------------------------------------------------------------------ the rounding model
def model_context(k, v, wout, dt, hw_scale):
    """float32; P = exp(k - max) and V rounded to T (the MFMA operands), exp sums unrounded,
    W_eff * hw_scale rounded to T."""
    T = TDT[dt]
    r = lambda a: a.to(T).float()
    B, HW, _ = k.shape
    p = torch.exp(k - k.max(dim=1, keepdim=True).values)
    s = p.sum(dim=1)
    ctx = torch.einsum("bnhd,bnhe->bhde", r(p).view(B, HW, 4, 32), r(v).view(B, HW, 4, 32))
    ctx = ctx / s.view(B, 4, 32, 1)
    C = wout.shape[0]
    weff = torch.einsum("che,bhde->bchd", wout.float().view(C, 4, 32), ctx).reshape(B, C, 128)
    return r(weff * hw_scale)


def rounding_model(x, wqkv, wout, bout, gout, dt):
    T = TDT[dt]
    r = lambda a: a.to(T).float()
    B, HW, _ = x.shape
    xf = x.float()
    qkv = r(_ln(xf)) @ wqkv.float().t()
    q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
    late = dt == "fp16"                      # fp16: 1/HW applied to the accumulators (hw_late)
    weff = model_context(k, v, wout, dt, 1.0 if late else 1.0 / HW)
    qs = r(torch.softmax(q.view(B, HW, 4, 32), dim=-1).reshape(B, HW, 128) * 32 ** -0.5)
    t = (qs @ weff.transpose(1, 2)) * (1.0 / HW if late else 1.0) + bout.float()
    return r(xf + _ln(t) * gout.float())


def rel_err(a, ref):
    """max|a - ref| / max|ref| per image -> list of floats."""
    B = ref.shape[0]
    d = (a.double() - ref).abs().reshape(B, -1).max(dim=1).values
    return (d / ref.abs().reshape(B, -1).max(dim=1).values).tolist()


def two_ulp(dt, ref):
    """2 ulp of T at max|ref|, relative to max|ref|, per image."""
    B = ref.shape[0]
    out = []
    for m in ref.abs().reshape(B, -1).max(dim=1).values.tolist():
        out.append(2.0 * 2.0 ** (math.floor(math.log2(m)) - MANT[dt]) / m)
    return out


def bounds(dt, model_err, ref):
    if dt == "fp32":
        return [1e-5] * ref.shape[0]
    return [max(4.0 * e, f) for e, f in zip(model_err, two_ulp(dt, ref))]


# ------------------------------------------------------------------ data
def _zero_mean_unit(v):
    v = v - v.mean(-1, keepdim=True)
    return v / v.norm(dim=-1, keepdim=True) * math.sqrt(v.shape[-1])


def _profile(HW, C, reg, g):
    """cos(theta) per pixel [HW] for the steered regimes."""
    nc, ch, empty = fused_chunking(HW, C)
    if reg in ("rising", "falling"):
        # Monotone from -1 to 1: 0.1 per 64-pixel tile inside the steep chunk (k channels of
        # gain a move by 0.1 a per tile there), the rest spread evenly over the other pixels.
        p0 = steep_chunk(HW, C, reg) * ch
        p1 = min(HW, p0 + ch)
        steep = 0.1 / 64
        rest = (2.0 - steep * (p1 - p0)) / (HW - (p1 - p0))
        slope = torch.full((HW,), rest, dtype=torch.float64)
        slope[p0:p1] = steep
        c = -1.0 + torch.cumsum(slope, 0) - slope[0]
        c = c.clamp(-1.0, 1.0)
        return (c if reg == "rising" else -c).float()              # falling: the mirror image
    if reg == "negk":
        return -1.0 + 0.4 * torch.rand(HW, generator=g)
    if reg == "dominant":
        c = -0.6 + 0.2 * torch.rand(HW, generator=g)
        c[dominant_pixel(HW, C)] = 1.0
        return c
    raise ValueError(reg)


def steep_chunk(HW, C, reg):
    """The chunk in which the rising / falling k moves fastest: the one that carries the
    softmax's weight (rising: the last chunk with at least two tiles; falling: the first), so
    what the stale max and the within-chunk rescale do there shows in the output."""
    nc, ch, empty = fused_chunking(HW, C)
    used = nc - empty
    if reg == "falling":
        return 0
    return used - 1 if HW - (used - 1) * ch >= 128 else used - 2


def dominant_pixel(HW, C):
    nc, ch, empty = fused_chunking(HW, C)
    return ((nc - empty) // 2) * ch + min(ch, HW) - 10          # last tile of a middle chunk


SLOW, FAST = 14.0, 68.0        # k gains of the rising / falling regimes (before LN's 1/std)


def _k_gains(reg):
    """Gain of k channel h*32+d along u1 (0: a random row instead)."""
    a = torch.zeros(4, 32)
    if reg in ("rising", "falling"):
        a[:] = SLOW                      # heads 0, 1 and head 2's channels 16..31: slow groups
        a[2, :16] = FAST                 # head 2, channels 0..15 and head 3: fast groups
        a[3, :] = FAST
        a[3, ::2] = 0.6 * FAST           # (mixed: the group moves, these channels need not)
    elif reg == "negk":
        a[:, :16] = torch.linspace(24.0, 40.0, 16)
    elif reg == "dominant":
        a[:, :8] = 11.2
    return a.reshape(128)


@functools.lru_cache(maxsize=4)
def master(HW, C, reg, B):
    """fp32 inputs of a case (the same for every dtype, which then rounds x and wqkv to T):
    x [B, HW, C], wqkv [384, C], wout [C, 128], bout, gout [C], qbound (the engine's formula)."""
    g = torch.Generator().manual_seed(1000003 * HW + 101 * C + sum(map(ord, reg)))
    rn = lambda *s: torch.randn(*s, generator=g)
    sc = 1.0 / math.sqrt(C)
    wq, wk, wv = rn(128, C) * 1.5 * sc, rn(128, C) * 4.0 * sc, rn(128, C) * sc
    if reg in ("random", "qbound"):
        x = rn(1, 1, C) + rn(B, HW, C) + 3.0 * rn(B, HW, 1)
        if reg == "qbound":
            z = _zero_mean_unit(rn(2, C)) * sc                    # unit vectors
            norm = (38.0 - 0.05) / 1.01 / math.sqrt(C)
            wq[5], wq[70] = z[0] * norm, z[1] * norm
            sel = torch.rand(B, HW, generator=g)
            for lo, hi, d in ((0.0, 0.1, z[0]), (0.1, 0.2, -z[0]), (0.2, 0.3, z[1])):
                m = (sel >= lo) & (sel < hi)
                m[:, int(lo * 10 + 0.5)] = True                   # every image has each kind of pixel
                al = d * math.sqrt(C) * 2.0 + 0.6 * rn(B, HW, C) + rn(B, HW, 1)
                x = torch.where(m.unsqueeze(-1), al, x)
    else:
        # x = (cos u1 + sin u2 + 0.5 n) * scale + offset per pixel, with u1, u2, n zero-mean,
        # mutually orthogonal and of norm sqrt(C): LN(x) = (cos u1 + sin u2 + 0.5 n) / sqrt(1.25)
        # whatever the scale and offset, so a k row a u1 / C gives k = a cos / sqrt(1.25). n
        # carries a third direction u3 whose sign alternates from chunk to chunk, and v rows see
        # it: the context then depends on which chunks hold the softmax's weight.
        u = rn(3, C)
        u1 = _zero_mean_unit(u[0])
        u2 = u[1] - u[1].mean()
        u2 = _zero_mean_unit(u2 - (u2 @ u1) / C * u1)
        u3 = u[2] - u[2].mean()
        u3 = _zero_mean_unit(u3 - (u3 @ u1) / C * u1 - (u3 @ u2) / C * u2)
        sign = 1.0 - 2.0 * ((torch.arange(HW) // fused_chunking(HW, C)[1]) % 2).float()
        n = rn(B, HW, C) + 1.5 * sign.view(1, HW, 1) * u3
        n = n - n.mean(-1, keepdim=True)
        n = n - (n @ u1 / C).unsqueeze(-1) * u1 - (n @ u2 / C).unsqueeze(-1) * u2
        n = _zero_mean_unit(n)
        wv = wv + 2.0 * rn(128, 1) * u3 / C
        c = _profile(HW, C, reg, g)
        s = torch.sqrt((1 - c * c).clamp(min=0)) * torch.where(torch.rand(HW, generator=g) < 0.5, -1.0, 1.0)
        x = c.view(1, HW, 1) * u1 + s.view(1, HW, 1) * u2 + 0.5 * n
        x = x * (0.7 + 0.7 * torch.rand(B, HW, 1, generator=g)) + 0.5 * rn(B, HW, 1)
        a = _k_gains(reg)
        steer = a.view(128, 1) * u1 / C + 0.02 * sc * rn(128, C)
        wk = torch.where((a > 0).view(128, 1), steer, wk)
    wqkv = torch.cat([wq, wk, wv], 0)
    bound = 1.01 * wq.double().norm(dim=1).max().item() * math.sqrt(C) + 0.05
    # to_out: scaled so the channel variance of W_eff q is a few times the LayerNorm's eps, and
    # a bias that cancels its mean over the pixels: t is then the pixel-dependent part of
    # W_eff q, and a scale error in W_eff changes the direction of t, not only its size (which
    # the LayerNorm would hide). gout is of the size of x.
    wout = rn(C, 128) / math.sqrt(128.0)
    q, k, v = ref_qkv(x, wqkv)
    weff = ref_weff(ref_context(k, v), wout)
    t0 = torch.softmax(q.view(B, HW, 4, 32), dim=-1).reshape(B, HW, 128) * 32 ** -0.5 @ weff.transpose(1, 2)
    target = 2.0 * math.sqrt(EPS)
    scale = target / t0.std(dim=-1).median().item()
    wout = wout * scale
    bout = (-scale * t0.mean(dim=(0, 1)) + 0.3 * target * rn(C)).float()
    gout = (1.0 + 0.25 * rn(C)) * 1.5 * x.square().mean().sqrt() * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return dict(x=x, wqkv=wqkv, wout=wout.float(), bout=bout, gout=gout, qbound=float(bound))


@functools.lru_cache(maxsize=4)
def case(dt, C, HW, reg, B=None):
    """Inputs in T, the fp64 reference on them, the rounding model's error and the bounds."""
    B = B or _batch(HW)
    m = master(HW, C, reg, B)
    T = TDT[dt]
    d = dict(m, x=m["x"].to(T), wqkv=m["wqkv"].to(T), B=B)
    ref = reference(d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"])
    d["ref"] = ref
    if dt == "fp32":
        d["model_err"] = [float("nan")] * B
    else:
        d["model_err"] = rel_err(rounding_model(d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"], dt), ref["y"])
    d["tol"] = bounds(dt, d["model_err"], ref["y"])
    return d


def weff_case(dt, d):
    """The unfused chain's inputs and references for a case: qkv in T, the fp64 W_eff of that
    rounded qkv times hw_scale * HW, the model's error, the bounds."""
    T = TDT[dt]
    B, HW = d["B"], d["x"].shape[1]
    r = d["ref"]
    qkv = torch.cat([r["q"], r["k"], r["v"]], -1).to(T)
    S = 2.0 ** math.ceil(math.log2(HW)) if dt == "fp16" else 0.0   # Engine::linattn: S = 2^k >= HW
    mul = S if dt == "fp16" else 1.0
    k, v = qkv[..., 128:256].double(), qkv[..., 256:].double()
    ref = ref_weff(ref_context(k, v), d["wout"]) * mul
    if dt == "fp32":
        merr = [float("nan")] * B
    else:
        merr = rel_err(model_context(k.float(), v.float(), d["wout"], dt, mul / HW), ref)
    return dict(qkv=qkv, hw_scale=S / HW, ref=ref, model_err=merr, tol=bounds(dt, merr, ref))


# ------------------------------------------------------------------ preconditions (CPU)
def _tile_max(k, ch0, ch1):
    """k [HW, 128] -> per 64-pixel tile maxima [ntiles, 128] of pixels ch0..ch1."""
    seg = k[ch0:ch1]
    return torch.stack([seg[i:i + 64].max(dim=0).values for i in range(0, seg.shape[0], 64)])


def check_regime(dt, C, HW, reg, d):
    nc, ch, empty = fused_chunking(HW, C)
    used = nc - empty
    K, Q = d["ref"]["k"], d["ref"]["q"]
    for b in range(d["B"]):
        k = K[b]
        if reg == "random":
            sp = k.std(dim=0)
            assert 2.0 < sp.median().item() < 4.0, sp.median().item()
        elif reg in ("rising", "falling"):
            sgn = 1.0 if reg == "rising" else -1.0
            cm = torch.stack([k[c * ch:min(HW, (c + 1) * ch)].max(dim=0).values for c in range(used)])
            assert (sgn * (cm[1:] - cm[:-1]) > 0).all()               # every chunk's max beyond the last one's
            assert (sgn * (cm[-1] - cm[0])).min().item() >= 20.0      # by >= 20 over the image, per channel
            if reg == "falling":                                      # the first tile holds every channel's max
                assert torch.equal(k[:64].max(dim=0).values, k.max(dim=0).values)
            # the steep chunk: per-tile moves of the tile maxima, by (head, 16-channel) group --
            # the granularity at which la_proj_ctx decides to move its reference max
            p0 = steep_chunk(HW, C, reg) * ch
            tm = _tile_max(k, p0, min(HW, p0 + ch))
            assert tm.shape[0] >= 2
            step = (tm[1:] - tm[:-1]).abs().view(-1, 8, 16)           # [tile steps, group, channel]
            gs = step.amax(dim=2)                                     # the group's fastest channel
            assert (gs.amax(dim=0) < TAU).sum().item() >= 2, gs      # groups that never pass tau per tile
            assert (gs.amin(dim=0) > TAU).sum().item() >= 2, gs      # groups that pass it on every tile
        elif reg == "negk":
            assert ((k.max(dim=0).values <= -8.0).sum().item()) >= 32
        elif reg == "dominant":
            top = k.topk(2, dim=0)
            gap = top.values[0] - top.values[1]
            hit = (gap >= 12.0) & (gap <= 16.0) & (top.indices[0] == dominant_pixel(HW, C))
            assert hit.sum().item() >= 32, gap
            ps = dominant_pixel(HW, C)
            c0 = ps // ch * ch
            assert 0 < ps // ch < used - 1 and ps >= min(HW, c0 + ch) - 64     # last tile, middle chunk
        elif reg == "qbound":
            assert 30.0 <= d["qbound"] <= 40.0
            q = Q[b].view(HW, 4, 32)
            big = q.abs() >= 0.8 * d["qbound"]
            assert big.any()
            px, h, j = big.nonzero()[0].tolist()
            others = torch.cat([q[px, h, :j], q[px, h, j + 1:]])
            assert others.abs().max().item() < 0.25 * d["qbound"]
            assert (q <= -0.8 * d["qbound"]).any()                    # exp(q - qshift) down to e^-70
        assert Q[b].abs().max().item() <= d["qbound"]                 # the shift really bounds q
    if dt == "fp16":       # fp16 stores W_eff without the 1/HW: the case must stay in range
        assert (d["ref"]["weff"].abs().max().item() * HW) < 3.0e4


def check_sensitivity(dt, C, HW, reg, d):
    """Each perturbation of the reference must move y by more than 10 x the case's tolerance."""
    nc, ch, empty = fused_chunking(HW, C)
    args = (d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"])
    pert = {"weff_x2": dict(weff_scale=2.0)}
    if reg == "negk":
        pert["extra_zero_pixel"] = dict(extra_zero_pixel=True)
    if reg in ("rising", "falling"):
        c = nc - empty - 1 if reg == "rising" else 0                 # the chunk that carries the max
        pert["dropped_chunk"] = dict(drop=(c * ch, min(HW, (c + 1) * ch)))
    out = {}
    for name, kw in pert.items():
        moved = rel_err(reference(*args, **kw)["y"], d["ref"]["y"])
        out[name] = moved
        for mv, tol in zip(moved, d["tol"]):
            assert mv > 10.0 * tol, (name, mv, tol)
    return out


def test_empty_chunk_counts():
    """72x72: the chunk length rounds up to 64 pixels and leaves trailing chunks empty."""
    assert fused_chunking(5184, 64) == (64, 128, 23)
    assert fused_chunking(5184, 128) == (64, 128, 23)
    assert fused_chunking(5184, 256) == (32, 192, 5)
    assert fused_chunking(16384, 64)[:2] == (64, 256) and fused_chunking(16384, 256)[:2] == (32, 512)
    assert fused_chunking(1000, 128) == (16, 64, 0) and fused_chunking(1024, 256) == (16, 64, 0)
    assert fused_chunking(7, 64) == (1, 64, 0) and fused_chunking(36, 256) == (1, 64, 0)


def test_reference_matches_module_definition():
    """The reference against a literal transcription of module_util.py's LinearAttention
    (NCHW, to_qkv / to_out as channel matmuls, the PreNorm gain applied instead of folded)."""
    g = torch.Generator().manual_seed(5)
    B, H, W, C = 2, 5, 7, 64
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gain = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    wqkv = torch.randn(384, C, generator=g, dtype=torch.float64) * 0.3
    wout = torch.randn(C, 128, generator=g, dtype=torch.float64) * 0.5
    bout = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    gout = torch.randn(C, generator=g, dtype=torch.float64)

    def ln(t, gn):
        var = t.var(dim=1, unbiased=False, keepdim=True)
        return (t - t.mean(dim=1, keepdim=True)) * (var + EPS).rsqrt() * gn.view(1, -1, 1, 1)
    qkv = torch.einsum("oc,bchw->bohw", wqkv, ln(x, gain)).chunk(3, dim=1)
    q, k, v = (t.reshape(B, 4, 32, H * W) for t in qkv)
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    v = v / (H * W)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, 128, H, W)
    t = torch.einsum("oc,bchw->bohw", wout, out) + bout.view(1, -1, 1, 1)
    want = (ln(t, gout) + x).permute(0, 2, 3, 1).reshape(B, H * W, C)
    got = reference(x.permute(0, 2, 3, 1).reshape(B, H * W, C), wqkv * gain, wout, bout, gout)["y"]
    assert (got - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("HW,reg", SR, ids=[f"HW{h}-{r}" for h, r in SR])
def test_preconditions_and_sensitivity(HW, reg):
    """CPU: every (dtype, C) of a (shape, regime) has the regime's property, a rounding model
    within sane limits, and a reference that every perturbation moves by > 10 x the tolerance."""
    for dt, C in DTC:
        d = case(dt, C, HW, reg)
        assert torch.isfinite(d["ref"]["y"]).all()
        check_regime(dt, C, HW, reg, d)
        moved = check_sensitivity(dt, C, HW, reg, d)
        print(f"{dt} C={C} HW={HW} {reg}: model {max(d['model_err']):.2e} tol {max(d['tol']):.2e} "
              + " ".join(f"{n} {min(v):.2e}" for n, v in moved.items()))


# ------------------------------------------------------------------ the ABI's argument checks
def _have_lib():
    from daclip_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


def test_bad_arguments_are_refused_before_any_device_work():
    """Runs without a GPU: DAC_E_ARG must come from the checks, ahead of the first HIP call."""
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    from daclip_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E = _lib.DAC_E_ARG
    for hole in range(6):
        ptrs = [p] * 6
        ptrs[hole] = None
        assert L.dac_op_linear_attention(*ptrs, 1, 64, 64, _lib.DAC_BF16, 0.0, None) == E, hole
    for hole in range(3):
        ptrs = [p] * 3
        ptrs[hole] = None
        assert L.dac_op_linear_attention_weff(*ptrs, 1, 64, 64, _lib.DAC_BF16, 0.0, None) == E, hole
    bad = [(0, 64, 64, _lib.DAC_BF16), (-1, 64, 64, _lib.DAC_F16), (1, 0, 64, _lib.DAC_BF16),
           (1, -5, 128, _lib.DAC_F32), (1, 64, 0, _lib.DAC_BF16), (1, 64, 32, _lib.DAC_BF16),
           (1, 64, 96, _lib.DAC_F16), (1, 64, 512, _lib.DAC_BF16), (1, 64, 256, _lib.DAC_F32),
           (1, 64, 64, _lib.DAC_FP8), (1, 64, 64, 99)]
    for (B, HW, C, code) in bad:
        assert L.dac_op_linear_attention(p, p, p, p, p, p, B, HW, C, code, 0.0, None) == E, (B, HW, C, code)
        assert L.dac_op_linear_attention_weff(p, p, p, B, HW, C, code, 0.0, None) == E, (B, HW, C, code)
    assert L.dac_op_linear_attention(p, p, p, p, p, p, 1, 64, 64, _lib.DAC_BF16, -1.0, None) == E
    assert L.dac_op_linear_attention(p, p, p, p, p, p, 1, 64, 64, _lib.DAC_BF16, float("nan"), None) == E
    assert L.dac_op_linear_attention_weff(p, p, p, 1, 64, 64, _lib.DAC_F16, -0.5, None) == E


# ------------------------------------------------------------------ GPU
def _code(dt):
    from daclip_amd import _lib
    return {"bf16": _lib.DAC_BF16, "fp16": _lib.DAC_F16, "fp32": _lib.DAC_F32}[dt]


def run_fused(dt, x, wqkv, wout, bout, gout, qshift):
    """x [B, HW, C] in T (any device) -> y on the GPU."""
    from daclip_amd import _lib
    B, HW, C = x.shape
    dev = [t.cuda().contiguous() for t in (x, wqkv, wout.float(), bout.float(), gout.float())]
    y = torch.empty_like(dev[0])
    rc = _lib.lib().dac_op_linear_attention(*[_lib._ptr(t) for t in dev], _lib._ptr(y), B, HW, C, _code(dt),
                                            float(qshift), _lib._stream(y.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y


def run_weff(dt, qkv, wout, hw_scale):
    from daclip_amd import _lib
    B, HW, _ = qkv.shape
    C = wout.shape[0]
    qd, wd = qkv.cuda().contiguous(), wout.float().cuda().contiguous()
    weff = torch.empty(B, C, 128, device="cuda", dtype=qd.dtype)
    rc = _lib.lib().dac_op_linear_attention_weff(_lib._ptr(qd), _lib._ptr(wd), _lib._ptr(weff), B, HW, C,
                                                 _code(dt), float(hw_scale), _lib._stream(weff.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return weff


@pytest.mark.gpu
@pytest.mark.parametrize("dt,C,HW,reg", CASES, ids=IDS)
def test_fused_matches_fp64_reference(dt, C, HW, reg):
    d = case(dt, C, HW, reg)
    check_regime(dt, C, HW, reg, d)
    shifts = (0.0, d["qbound"]) if reg in ("random", "qbound") else (d["qbound"] if d["qbound"] <= 40.0 else 0.0,)
    fails = []
    for qs in shifts:
        y = run_fused(dt, d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"], qs)
        assert torch.isfinite(y).all()
        err = rel_err(y.cpu(), d["ref"]["y"])
        print(f"LA {dt} C={C} HW={HW} {reg} qshift={qs:.2f}: model {max(d['model_err']):.2e} "
              f"kernel {max(err):.2e} bound {max(d['tol']):.2e}")
        fails += [(qs, e, t) for e, t in zip(err, d["tol"]) if not e <= t]
        again = run_fused(dt, d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"], qs)
        assert torch.equal(y.view(torch.uint8), again.view(torch.uint8))      # deterministic
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("dt,C,HW,reg", [c for c in CASES if c[3] != "qbound"],
                         ids=[i for i, c in zip(IDS, CASES) if c[3] != "qbound"])
def test_weff_chain_matches_fp64_reference(dt, C, HW, reg):
    d = case(dt, C, HW, reg)
    w = weff_case(dt, d)
    out = run_weff(dt, w["qkv"], d["wout"], w["hw_scale"])
    assert torch.isfinite(out).all()
    err = rel_err(out.cpu(), w["ref"])
    print(f"LAW {dt} C={C} HW={HW} {reg}: model {max(w['model_err']):.2e} kernel {max(err):.2e} "
          f"bound {max(w['tol']):.2e}")
    assert torch.equal(out.view(torch.uint8), run_weff(dt, w["qkv"], d["wout"], w["hw_scale"]).view(torch.uint8))
    assert all(e <= t for e, t in zip(err, w["tol"])), (err, w["tol"])


@pytest.mark.gpu
@pytest.mark.parametrize("HW", [1000, 5184])
@pytest.mark.parametrize("dt,C", DTC, ids=[f"{dt}-C{C}" for dt, C in DTC])
def test_batch_invariance_is_bit_exact(dt, C, HW):
    """An image gives the same bits alone and as image 0, 1 or 2 of a batch of three different
    images: the chunking depends on (HW, C) only, and la_apply's split of the tiles over a block
    count that depends on B must not matter. Likewise the unfused chain."""
    d = case(dt, C, HW, "random", 3)
    w = weff_case(dt, d)
    bits = lambda t: t.view(torch.uint8)
    for qs in (0.0, d["qbound"]):
        y3 = run_fused(dt, d["x"], d["wqkv"], d["wout"], d["bout"], d["gout"], qs)
        assert not torch.equal(bits(y3[0]), bits(y3[1]))
        for b in range(3):
            y1 = run_fused(dt, d["x"][b:b + 1], d["wqkv"], d["wout"], d["bout"], d["gout"], qs)
            assert torch.equal(bits(y1[0]), bits(y3[b])), (qs, b)
    w3 = run_weff(dt, w["qkv"], d["wout"], w["hw_scale"])
    for b in range(3):
        w1 = run_weff(dt, w["qkv"][b:b + 1], d["wout"], w["hw_scale"])
        assert torch.equal(bits(w1[0]), bits(w3[b])), b
