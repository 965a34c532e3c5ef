"""Tiled restoration (dac_sde_reverse_tiled, dac_op_tile_blend, IRSDE(..., tile=...)).

The feature has no reference counterpart; it is defined in include/daclip_hip.h / DESIGN.md §10
and restated here in torch. Bars:
  * the blend op is bit-identical to the torch restatement (fixed tile order, separate multiply
    and add, one division; single-covered pixels copied);
  * a one-tile plan is bit-identical to the untiled loop; the result is bit-identical for every
    tiles_per_forward, for the captured and the eagerly enqueued loop, and for an image restored
    alone or in a batch (context routing);
  * fp32: the native tiled loop against the Python tiled loop (the same algorithm, stepwise,
    through a plain callable) within the project's fp32 bar, max|d| / max|ref| < 1e-4
    (tests/test_hip_parity.py), next to the untiled graph-versus-stepwise floor.
Standard synthetic UNet, T = 100 cosine schedule run for 3 steps.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 3
FP32_BAR = 1e-4


# ----------------------------------------------------------------------------- helpers
def build_model(unet_sd, dtype):
    from daclip_amd.unet import ConditionalUNet
    m = ConditionalUNet(3, 3, 64, [1, 2, 4, 8], 512, True, True, dtype=dtype)
    m.load_state_dict(unet_sd)
    return m


@pytest.fixture(scope="module")
def models(unet_sd):
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = build_model(unet_sd, dtype)
        return cache[dtype]
    return get


def make_sde(model):
    from daclip_amd.sde import IRSDE
    sde = IRSDE(max_sigma=50, T=100, schedule="cosine", eps=0.005)
    sde.set_model(model)
    return sde


def inputs(B, H, W, seed=0):
    """mu in about [0, 1], the noisy state, STEPS step noises and per-image contexts."""
    from daclip_amd import synth
    T = lambda a: torch.from_numpy(a).cuda()
    mu = T(0.5 + 0.15 * synth.synth_noise((B, 3, H, W), seed, "tiled_mu")).clamp(0, 1)
    x = mu + T(synth.synth_noise((B, 3, H, W), seed, "tiled_x0")) * (50 / 255)
    z = T(synth.synth_noise((STEPS, B, 3, H, W), seed, "tiled_steps"))
    tc = T(synth.synth_noise((B, 512), seed, "tiled_tc"))
    ic = T(synth.synth_noise((B, 512), seed, "tiled_ic"))
    return x, mu, z, tc, ic


def run(sde, mode, x, mu, z, tc, ic, seed=None, **kw):
    sde.set_mu(mu)
    if seed is not None:
        sde.seed = seed               # the loop pre-increments it: equal seeds, equal draws
    f = sde.reverse_posterior if mode == "posterior" else sde.reverse_sde
    out = f(x, T=STEPS, noises=z, text_context=tc, image_context=ic, **kw)
    torch.cuda.synchronize()
    return out


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def torch_blend(tiles, B, H, W, th, tw, ov, ys, xs):
    """The blend restated on the host: tiles in ascending k = (b*ny + iy)*nx + ix, the product
    and the sum separate fp32 roundings, one division; a single-covered pixel is a copy."""
    tiles = tiles.cpu()
    ramp = lambda l: torch.tensor([min(i + 1, l - i, ov + 1) for i in range(l)], dtype=torch.float32)
    w = ramp(th)[:, None] * ramp(tw)[None, :]
    acc = torch.zeros(B, 3, H, W)
    copy = torch.zeros(B, 3, H, W)
    ws = torch.zeros(H, W)
    cnt = torch.zeros(H, W, dtype=torch.int64)
    for iy, y0 in enumerate(ys):
        for ix, x0 in enumerate(xs):
            cnt[y0:y0 + th, x0:x0 + tw] += 1
            ws[y0:y0 + th, x0:x0 + tw] = ws[y0:y0 + th, x0:x0 + tw] + w
            for b in range(B):
                t = tiles[(b * len(ys) + iy) * len(xs) + ix]
                prod = w * t
                acc[b, :, y0:y0 + th, x0:x0 + tw] = acc[b, :, y0:y0 + th, x0:x0 + tw] + prod
                copy[b, :, y0:y0 + th, x0:x0 + tw] = t
    assert int(cnt.min()) >= 1
    return torch.where(cnt == 1, copy, acc / ws), cnt


# ----------------------------------------------------------------------------- 1, 7: the blend op
@pytest.mark.parametrize("B,H,W,tile,ov,grid", [
    (2, 48, 40, 32, 16, ([0, 16], [0, 8])),        # clamped last column: overlap 24, 16-byte path
    (2, 64, 64, 32, 0, ([0, 32], [0, 32])),        # overlap 0: every pixel single-covered
    (1, 45, 39, 32, 16, ([0, 13], [0, 7])),        # odd sizes: the per-pixel path
    (1, 40, 70, 16, 15, None),                     # stride 1: up to 16 x 16 tiles cover a pixel
])
def test_blend_op_bit_exact(B, H, W, tile, ov, grid):
    from daclip_amd import synth, tiling
    from daclip_amd.sde import tile_blend
    th, tw, ys, xs = tiling.plan(H, W, tile, ov)
    if grid is not None:
        assert (ys, xs) == grid
    tiles = torch.from_numpy(synth.synth_noise((B * len(ys) * len(xs), 3, th, tw), 3, "blend_tiles")).cuda()
    out = tile_blend(tiles, B, H, W, th, tw, ov, ys, xs)
    ref, cnt = torch_blend(tiles, B, H, W, th, tw, ov, ys, xs)
    assert torch.equal(out.cpu(), ref)
    if ov == 0:
        assert int(cnt.max()) == 1                 # a pure copy


def test_blend_op_distinct_constants():
    """Seam guard: tile k holds the constant 2k + 1. Pixel (5, 20) of the 48 x 40 plan lies in
    tiles 0 and 1 (values 1 and 3) with weights 6 * 12 and 6 * 13."""
    from daclip_amd import tiling
    from daclip_amd.sde import tile_blend
    th, tw, ys, xs = tiling.plan(48, 40, 32, 16)
    vals = torch.arange(4, dtype=torch.float32) * 2 + 1
    tiles = vals[:, None, None, None].expand(4, 3, th, tw).contiguous().cuda()
    out = tile_blend(tiles, 1, 48, 40, th, tw, 16, ys, xs).cpu()
    wa, wb = np.float32(6 * 12), np.float32(6 * 13)
    want = (wa * np.float32(1) + wb * np.float32(3)) / (wa + wb)
    assert out[0, 0, 5, 20].item() == want
    assert out[0, 0, 5, 20].item() != 1.0          # not the first tile's value
    assert out[0, 1, 2, 3].item() == 1.0           # single-covered: tile 0 unchanged
    assert out[0, 2, 47, 39].item() == 7.0
    ref, _ = torch_blend(tiles, 1, 48, 40, th, tw, 16, ys, xs)
    assert torch.equal(out, ref)


# ----------------------------------------------------------------------------- 2: one tile
@pytest.mark.parametrize("mode", ["posterior", "sde"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_one_tile_equals_untiled(models, dtype, mode):
    sde = make_sde(models(dtype))
    x, mu, z, tc, ic = inputs(2, 32, 32)
    a = run(sde, mode, x, mu, z, tc, ic)
    b = run(sde, mode, x, mu, z, tc, ic, tile=32, tile_overlap=16)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    a = run(sde, mode, x, mu, None, tc, ic, seed=11)             # device Philox noise
    b = run(sde, mode, x, mu, None, tc, ic, seed=11, tile=32, tile_overlap=16)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, run(sde, mode, x, mu, None, tc, ic, seed=12, tile=32, tile_overlap=16))


# ----------------------------------------------------------------------------- 3, 7: chunking
@pytest.fixture(scope="module")
def tiled_fp16(models):
    sde = make_sde(models("fp16"))
    args = inputs(2, 48, 40)
    return sde, args, run(sde, "posterior", *args, tile=32, tile_overlap=16, tiles_per_forward=8)


@pytest.mark.parametrize("tpf", [1, 3])
def test_chunking_invariance(tiled_fp16, tpf):
    sde, args, full = tiled_fp16
    assert torch.equal(run(sde, "posterior", *args, tile=32, tile_overlap=16, tiles_per_forward=tpf), full)


def test_eager_loop_equals_graph(tiled_fp16, monkeypatch):
    """Above the node limit the loop is enqueued eagerly instead of instantiated; same result."""
    sde, args, full = tiled_fp16
    monkeypatch.setenv("DAC_TILED_MAX_NODES", "0")
    assert torch.equal(run(sde, "posterior", *args, tile=32, tile_overlap=16, tiles_per_forward=4), full)


def test_seams_finite_and_blended(tiled_fp16, models):
    sde, (x, mu, z, tc, ic), full = tiled_fp16
    assert torch.isfinite(full).all()
    assert full.shape == x.shape
    # Rows 16..31 x columns 8..31 are covered by all four tiles: there the result differs from
    # the restore of tile 0 alone (its own trajectory), so the blend is not "first tile wins".
    alone = run(sde, "posterior", x[:, :, :32, :32].contiguous(), mu[:, :, :32, :32].contiguous(),
                z[:, :, :, :32, :32].contiguous(), tc, ic)
    assert not torch.equal(full[:, :, 16:32, 8:32], alone[:, :, 16:32, 8:32])


# ----------------------------------------------------------------------------- 4, 5: restatement
def python_loop(model):
    """The same model as a plain callable: IRSDE then runs its Python loops."""
    return lambda x, mu, t, **kw: model(x, mu, t, **kw)


@pytest.mark.parametrize("H,W,grid", [(48, 40, (32, 32, [0, 16], [0, 8])),
                                      (30, 34, (30, 32, [0], [0, 2]))])     # reflect-padded tiles
def test_native_tiled_matches_python_tiled_fp32(models, H, W, grid):
    """Measured (MI355X, fp32, 3 steps): see DESIGN.md §10."""
    from daclip_amd import tiling
    assert tiling.plan(H, W, 32, 16) == grid
    m = models("fp32")
    native, stepwise = make_sde(m), make_sde(python_loop(m))
    assert stepwise._native() is None
    args = inputs(2, H, W, seed=1)
    a = run(native, "posterior", *args, tile=32, tile_overlap=16)
    b = run(stepwise, "posterior", *args, tile=32, tile_overlap=16)
    small = inputs(2, 32, 32, seed=1)
    floor = rel(run(native, "posterior", *small), run(stepwise, "posterior", *small))
    d = rel(a, b)
    print(f"tiled native vs python loop {H}x{W}: rel {d:.3e}; untiled graph vs stepwise floor 32x32: rel {floor:.3e}")
    assert torch.isfinite(a).all()
    assert floor < FP32_BAR
    assert d < FP32_BAR


# ----------------------------------------------------------------------------- 6: context routing
@pytest.mark.parametrize("device_noise", [False, True])
def test_context_routing(models, device_noise):
    sde = make_sde(models("fp16"))
    x, mu, z, tc, ic = inputs(2, 48, 40, seed=2)
    assert not torch.equal(tc[0], tc[1]) and not torch.equal(ic[0], ic[1])
    kw = dict(tile=32, tile_overlap=16)
    if device_noise:
        both = run(sde, "posterior", x, mu, None, tc, ic, seed=5, **kw)
        sde.image_offset = 1
        one = run(sde, "posterior", x[1:], mu[1:], None, tc[1:], ic[1:], seed=5, **kw)
    else:
        both = run(sde, "posterior", x, mu, z, tc, ic, **kw)
        one = run(sde, "posterior", x[1:], mu[1:], z[:, 1:], tc[1:], ic[1:], **kw)
    assert torch.equal(both[1:], one)
    swapped = run(sde, "posterior", x[1:], mu[1:], z[:, 1:] if not device_noise else None, tc[:1], ic[:1],
                  seed=5 if device_noise else None, **kw)
    assert not torch.equal(swapped, one)           # the contexts do reach the tiles


# ----------------------------------------------------------------------------- 8: refusals
def test_refusals(models):
    from daclip_amd import _lib
    m = models("fp32")
    sde = make_sde(m)
    h = m._h
    x, mu, z, tc, ic = inputs(1, 48, 40)
    x0 = x.clone()
    L = _lib.lib()
    I32 = ctypes.c_int32
    arr = lambda v: None if v is None else (I32 * max(1, len(v)))(*v)

    def call(th=32, tw=32, ov=16, ys=(0, 16), xs=(0, 8), ny=None, nx=None, tpf=16):
        with torch.cuda.device(m.device):
            return L.dac_sde_reverse_tiled(h.h, 0, _lib._ptr(x), _lib._ptr(mu), _lib._ptr(tc), _lib._ptr(ic),
                                           1, 48, 40, th, tw, ov, arr(ys), len(ys) if ny is None else ny,
                                           arr(xs), len(xs) if nx is None else nx, tpf, STEPS, _lib._ptr(z), 1,
                                           h.stream())
    with torch.cuda.device(m.device):
        sde._sync_schedule(h)
    cases = {"null ys": dict(ys=None, ny=2), "null xs": dict(xs=None, nx=2), "empty ys": dict(ny=0),
             "empty xs": dict(nx=0), "th < 2": dict(th=1, ys=(0,)), "tw < 2": dict(tw=1, xs=(0,)),
             "th > H": dict(th=64, ys=(0,)), "tw > W": dict(tw=48, xs=(0,)), "overlap < 0": dict(ov=-1),
             "overlap >= tile": dict(ov=32), "overlap >= min": dict(tw=24, xs=(0, 16), ov=24),
             "ys out of bounds": dict(ys=(0, 20)), "xs negative": dict(xs=(-8, 8)),
             "ys descending": dict(ys=(16, 0)), "xs repeated": dict(xs=(0, 0, 8)),
             "row gap": dict(th=16, ys=(0, 32), ov=4), "first row uncovered": dict(ys=(8, 16)),
             "last column uncovered": dict(xs=(0, 4)), "tiles_per_forward < 1": dict(tpf=0)}
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc == _lib.DAC_E_ARG, (name, rc)
        assert L.dac_last_error(h.h).decode(), name
    torch.cuda.synchronize()
    assert torch.equal(x, x0)                      # nothing ran
    assert L.dac_profile_enable(h.h, 0) == 0
    try:
        rc = call()
        assert rc == _lib.DAC_E_STATE, rc
        assert "profil" in L.dac_last_error(h.h).decode()
    finally:
        L.dac_profile_enable(h.h, -1)
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
    assert call() == 0                             # the same call, valid and unprofiled, runs
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and not torch.equal(x, x0)
    # the op hook refuses the same grids, handle-less
    t = torch.zeros(4, 3, 32, 32, device="cuda")
    o = torch.zeros(1, 3, 48, 40, device="cuda")
    for ys, xs, ov in (((0, 20), (0, 8), 16), ((0, 16), (0, 4), 16), ((0, 16), (0, 8), 32)):
        assert L.dac_op_tile_blend(_lib._ptr(t), _lib._ptr(o), 1, 48, 40, 32, 32, ov, arr(ys), 2, arr(xs), 2,
                                   None) == _lib.DAC_E_ARG


# ----------------------------------------------------------------------------- 9: API plumbing
OPT = {"model": "denoising",
       "sde": {"max_sigma": 50, "T": STEPS, "schedule": "cosine", "eps": 0.005, "sampling_mode": "posterior"},
       "network_G": {"which_model_G": "ConditionalUNet",
                     "setting": {"in_nc": 3, "out_nc": 3, "nf": 64, "ch_mult": [1, 2, 4, 8],
                                 "context_dim": 512, "use_degra_context": True, "use_image_context": True}},
       "path": {"pretrain_model_G": None}}


def test_predictor_tiled():
    from daclip_amd import synth
    from daclip_amd.predict import Predictor
    from daclip_amd.preprocess import tensor2img
    p = Predictor()
    p.setup(OPT, dtype="fp16", synthetic=True)
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (48, 40, 3), dtype=np.uint8) for _ in range(2)]
    n0 = torch.from_numpy(synth.synth_noise((2, 3, 48, 40), 6, "pred_n0"))
    nz = torch.from_numpy(synth.synth_noise((STEPS, 2, 3, 48, 40), 6, "pred_steps"))
    outs = p.predict_batch(imgs, noise=n0, noises=nz, tile=32, tile_overlap=16)
    assert len(outs) == 2 and all(o.shape == (48, 40, 3) and o.dtype == np.uint8 for o in outs)
    rgb = [im[:, :, [2, 1, 0]] / 255.0 for im in imgs]
    ic, dc = p._contexts(rgb)
    lq = torch.stack([torch.tensor(im, dtype=torch.float32).permute(2, 0, 1) for im in rgb])
    p.sde.set_mu(lq.to(p.device))
    x = p.sde.reverse_posterior(p.sde.noise_state(lq, noise=n0), noises=nz, text_context=dc, image_context=ic,
                                tile=32, tile_overlap=16).float().cpu()
    for o, r in zip(outs, x):
        assert np.array_equal(o, tensor2img(r))
    untiled = p.predict_batch(imgs, noise=n0, noises=nz)
    assert any(not np.array_equal(a, b) for a, b in zip(outs, untiled))    # the option is not ignored
    one = p.predict(imgs[1], noise=n0[1:], noises=nz[:, 1:], tile=32, tile_overlap=16)
    assert np.array_equal(one, outs[1])


def test_evaluate_tiled(tmp_path):
    from PIL import Image
    from daclip_amd.evaluate import evaluate
    rng = np.random.default_rng(8)
    lq = tmp_path / "lq"
    lq.mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)).save(lq / f"img{i}.png")
    res = evaluate(OPT, str(lq), None, str(tmp_path / "out"), batch=2, dtype="fp16", synthetic=True, tile=32,
                   tile_overlap=16)
    assert res["summary"]["images"] == 2
    for i in range(2):
        assert Image.open(tmp_path / "out" / f"img{i}.png").size == (48, 40)


# ----------------------------------------------------------------------------- 10: shape-cache eviction
# The engine keeps the loop buffers and captured graphs of at most 8 untiled shapes (kMaxShapes)
# and 4 tiled keys (kMaxTiledShapes); one more drops every buffer and graph of that kind. Each
# test takes a handle of its own (the same model as `models`), so the cache starts empty and the
# last new key is the one that evicts. T = 100 cosine schedule, 2 steps, explicit noises.
EVICT_STEPS = 2


def test_untiled_shape_cache_eviction(unet_sd):
    sde = make_sde(build_model(unet_sd, "fp16"))
    shapes = [(H, W) for H in (16, 32, 64) for W in (16, 32, 64)]

    def restore(H, W):
        x, mu, z, tc, ic = inputs(1, H, W, seed=3)
        sde.set_mu(mu)
        out = sde.reverse_posterior(x, T=EVICT_STEPS, noises=z[:EVICT_STEPS], text_context=tc, image_context=ic)
        torch.cuda.synchronize()
        assert out.shape == x.shape and torch.isfinite(out).all(), (H, W)
        return out
    first = [restore(H, W) for H, W in shapes]      # the ninth (B, H, W, T) key evicts the other eight
    assert torch.equal(restore(*shapes[0]), first[0])            # rebuilt after the eviction
    assert torch.equal(restore(*shapes[-1]), first[-1])          # the graph captured right after it, replayed


def test_tiled_shape_cache_eviction(unet_sd):
    from daclip_amd import _lib
    m = build_model(unet_sd, "fp16")
    sde = make_sde(m)
    h, L = m._h, _lib.lib()
    H = W = 48
    x0, mu, z, tc, ic = inputs(1, H, W, seed=4)
    z = z[:EVICT_STEPS].contiguous()
    I32 = ctypes.c_int32
    ys = [0, 16]
    grids = [[0, 16], [0, 8, 16], [0, 4, 16], [0, 12, 16], [0, 8, 12, 16]]      # five TKeys

    def restore(xs):
        x = x0.clone()
        with torch.cuda.device(m.device):
            sde._sync_schedule(h)
            h.check(L.dac_sde_set_time_scale(h.h, float(sde.sample_scale)), "time_scale")
            h.check(L.dac_set_noise_offset(h.h, 0), "noise_offset")
            h.check(L.dac_sde_reverse_tiled(h.h, _lib.DAC_POSTERIOR, _lib._ptr(x), _lib._ptr(mu), _lib._ptr(tc),
                                            _lib._ptr(ic), 1, H, W, 32, 32, 16, (I32 * len(ys))(*ys), len(ys),
                                            (I32 * len(xs))(*xs), len(xs), 16, EVICT_STEPS, _lib._ptr(z), 1,
                                            h.stream()), "sde_reverse_tiled")
        torch.cuda.synchronize()
        assert torch.isfinite(x).all() and not torch.equal(x, x0), xs
        return x
    first = [restore(xs) for xs in grids]           # the fifth key evicts the other four
    assert torch.equal(restore(grids[0]), first[0])
