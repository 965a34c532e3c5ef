"""Device-side evaluation metrics (csrc/metrics.hip, dac_image_metrics, metrics.image_metrics_device,
evaluate(metrics="device")) against the host code they restate: preprocess.tensor2img and
metrics.image_metrics.

Bars: uint8 images bit-identical; PSNR / PSNR_Y within 1e-10 dB; SSIM / SSIM_Y within 1e-10 (the
bar tests/test_metrics.py holds the host SSIM to against its direct window sum; a separable fp64
restatement of the host code stays within 6.2e-13 of it on these shape and content families).

The SSIM-map tile is 16 rows x 32 columns (metrics.hip IM_TH, IM_TW), so a cropped window of
27 x 43 is one row and one column past a tile; 43 x 75 crosses two tile boundaries each way with
an odd width (unaligned byte loads)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from daclip_amd import _lib, metrics
from daclip_amd.preprocess import tensor2img

PSNR_TOL = 1e-10
SSIM_TOL = 1e-10
CONTENTS = ("perturbed", "unrelated", "flat", "binary", "identical")
# (H, W, crop_border): cropped 11x11 (one window); 12x43 (ragged, narrower than a tile); 27x43 and
# 43x75 (one past a tile boundary, odd W); 64x64 crop 4; a crop that leaves an odd offset.
SHAPES = ((11, 11, 0), (12, 43, 0), (27, 43, 0), (43, 75, 0), (64, 64, 4), (21, 53, 5))


def _have_lib():
    return os.path.exists(_lib.LIB_PATH)


# ---------------------------------------------------------------------------------- CPU tests
def test_symbols_exported():
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    got = _lib.exports_present(["dac_image_metrics_workspace", "dac_image_metrics"])
    assert got == {"dac_image_metrics_workspace": True, "dac_image_metrics": True}
    assert "dac_image_metrics" in _lib.EXPORTS and "dac_image_metrics_workspace" in _lib.EXPORTS


BAD_SHAPES = ((1, 3, 10, 11, 0), (1, 3, 11, 10, 0), (1, 2, 11, 11, 0), (1, 3, 16, 16, 3), (0, 3, 11, 11, 0),
              (1, 3, 16, 16, -1), (1, 4, 32, 32, 0), (1, 3, 32, 20, 5))


def test_workspace_size():
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    L = _lib.lib()
    assert L.dac_image_metrics_workspace(1, 3, 11, 11, 0) > 0
    assert L.dac_image_metrics_workspace(1, 1, 11, 11, 0) > 0
    assert L.dac_image_metrics_workspace(1, 3, 16, 16, 2) > 0            # cropped 12x12
    assert L.dac_image_metrics_workspace(1, 3, 10, 16, 0) == 0           # H = 10
    assert L.dac_image_metrics_workspace(1, 2, 16, 16, 0) == 0           # C = 2
    assert L.dac_image_metrics_workspace(1, 3, 16, 16, 3) == 0           # crop 3 on H = 16: 10 rows
    for s in BAD_SHAPES:
        assert L.dac_image_metrics_workspace(*s) == 0, s
    # grows with the batch and the image
    assert L.dac_image_metrics_workspace(2, 3, 64, 64, 0) > L.dac_image_metrics_workspace(1, 3, 64, 64, 0)
    assert L.dac_image_metrics_workspace(1, 3, 128, 128, 0) > L.dac_image_metrics_workspace(1, 3, 64, 64, 0)


def test_bad_arguments_are_refused_before_any_device_work():
    """Runs without a GPU: DAC_E_ARG must come from the checks, ahead of the first HIP call."""
    if not _have_lib():
        pytest.skip("libdaclip_hip.so not built")
    L = _lib.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.dac_image_metrics(None, None, 1, 3, 11, 11, 0, None, None, None, None, None) == _lib.DAC_E_ARG
    for hole in range(6):
        ptrs = [p] * 6
        ptrs[hole] = None
        o, g, o8, g8, res, ws = ptrs
        assert L.dac_image_metrics(o, g, 1, 3, 11, 11, 0, o8, g8, res, ws, None) == _lib.DAC_E_ARG, hole
    for (B, C, H, W, cb) in BAD_SHAPES:
        assert L.dac_image_metrics(p, p, B, C, H, W, cb, p, p, p, p, None) == _lib.DAC_E_ARG, (B, C, H, W, cb)


def test_evaluate_rejects_unknown_metrics_mode(tmp_path):
    from daclip_amd.evaluate import evaluate
    with pytest.raises(ValueError, match="metrics"):
        evaluate({}, str(tmp_path / "missing_lq"), None, str(tmp_path / "out"), metrics="bogus")
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------- GPU tests
def _pairs(C, H, W, seed):
    """The five content cases as uint8 [5, C, H, W] (out, gt), RGB planes."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (C, H, W), dtype=np.uint8)
    out = {"perturbed": np.clip(base.astype(int) + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8),
           "unrelated": rng.integers(0, 256, base.shape, dtype=np.uint8),
           "flat": np.full(base.shape, 255, np.uint8),
           "binary": (rng.integers(0, 2, base.shape) * 255).astype(np.uint8),
           "identical": base.copy()}
    gt = {"perturbed": base, "unrelated": base, "flat": np.full(base.shape, 254, np.uint8),
          "binary": (rng.integers(0, 2, base.shape) * 255).astype(np.uint8), "identical": base.copy()}
    return np.stack([out[k] for k in CONTENTS]), np.stack([gt[k] for k in CONTENTS])


def _as_float(u8):
    return torch.from_numpy(u8.astype(np.float32) / np.float32(255.0))


def _check_against_host(out_f, gt_f, cb, label):
    """out_f, gt_f: float32 CPU tensors [B,C,H,W]. Prints every figure, then asserts."""
    rows, out_u8 = metrics.image_metrics_device(out_f.cuda(), gt_f.cuda(), cb)
    B, C = out_f.shape[:2]
    assert out_u8.shape == (B, out_f.shape[2], out_f.shape[3], C) and out_u8.dtype == np.uint8
    failures = []
    for i in range(B):
        ho, hg = tensor2img(out_f[i]), tensor2img(gt_f[i])
        dev_img = out_u8[i] if C == 3 else out_u8[i, :, :, 0]
        assert np.array_equal(dev_img, ho), f"{label}[{i}]: uint8 image differs from tensor2img"
        ref = metrics.image_metrics(ho, hg, cb)
        assert sorted(rows[i]) == sorted(ref), (rows[i], ref)
        for k, want in ref.items():
            got = rows[i][k]
            tol = PSNR_TOL if k.startswith("psnr") else SSIM_TOL
            if math.isinf(want):
                ok, d = got == want, 0.0
            else:
                d = abs(got - want)
                ok = math.isfinite(got) and d <= tol
            print(f"{label}[{i}] {k}: device {got!r} host {want!r} |diff| {d:.3e}")
            if not ok:
                failures.append((label, i, k, got, want))
    assert not failures, failures
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_crop%d" % s)
def test_matches_host_metrics(shape, C):
    """All five content cases of one shape as one batch of 5 (flat 255 / 254, binary noise and
    identical images included); identical images must give infinite PSNR."""
    H, W, cb = shape
    o, g = _pairs(C, H, W, seed=H * 1000 + W + C)
    rows = _check_against_host(_as_float(o), _as_float(g), cb, f"{H}x{W}c{cb}C{C}")
    ident = rows[CONTENTS.index("identical")]
    assert ident["psnr"] == float("inf") and abs(ident["ssim"] - 1.0) <= SSIM_TOL
    if C == 3:
        assert ident["psnr_y"] == float("inf") and abs(ident["ssim_y"] - 1.0) <= SSIM_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 3))
def test_quantiser_ties_and_out_of_range(C):
    """Float images with exact .5 ties (k/255 + 0.5/255), values outside [0, 1], signed zeros and
    tiny values: bytes bit-identical to tensor2img, metrics of those bytes equal to the host's."""
    H, W = 27, 43
    rng = np.random.default_rng(7)
    k = rng.integers(0, 256, (2, C, H, W)).astype(np.float32)
    ties = k / np.float32(255.0) + np.float32(0.5) / np.float32(255.0)
    wild = rng.uniform(-0.5, 1.5, (2, C, H, W)).astype(np.float32)
    wild.reshape(-1)[:8] = [-0.0, 0.0, 1.0, 1e-30, -3.0, 7.5, np.float32(0.5 / 255.0), np.float32(254.5 / 255.0)]
    out = torch.from_numpy(np.stack([ties[0], wild[0], (k[0] + 0.5) / 255.0]).astype(np.float32))
    gt = torch.from_numpy(np.stack([ties[1], wild[1], (k[1] - 0.5) / 255.0]).astype(np.float32))
    _check_against_host(out, gt, 0, f"ties_C{C}")
    none_rows, only_u8 = metrics.image_metrics_device(out.cuda())             # no GT: bytes only
    assert none_rows is None
    for i in range(3):
        ref = tensor2img(out[i])
        assert np.array_equal(only_u8[i] if C == 3 else only_u8[i, :, :, 0], ref)


@pytest.mark.gpu
def test_batch_invariance_and_repeatability():
    """Image k alone and as element k of B = 3 (three different pairs): bit-identical records and
    bytes; a second call repeats the first bit for bit."""
    H, W, cb = 43, 75, 0
    o, g = _pairs(3, H, W, seed=11)
    pick = [CONTENTS.index(n) for n in ("perturbed", "unrelated", "binary")]
    of, gf = _as_float(o[pick]).cuda(), _as_float(g[pick]).cuda()
    rec3, u3 = metrics.image_metrics_records(of, gf, cb)
    again, u3b = metrics.image_metrics_records(of, gf, cb)
    assert rec3.tobytes() == again.tobytes() and np.array_equal(u3, u3b)
    assert len({rec3[i].tobytes() for i in range(3)}) == 3                   # three different pairs
    for k in range(3):
        rec1, u1 = metrics.image_metrics_records(of[k:k + 1], gf[k:k + 1], cb)
        assert rec1[0].tobytes() == rec3[k].tobytes(), (k, rec1[0], rec3[k])
        assert np.array_equal(u1[0], u3[k])
    # the record's bookkeeping fields
    assert np.all(rec3[:, 1] == 3 * H * W) and np.all(rec3[:, 4] == H * W) and np.all(rec3[:, 6:] == 0)
    sse = ((tensor2img(of[0].cpu()).astype(np.int64) - tensor2img(gf[0].cpu()).astype(np.int64)) ** 2).sum()
    assert rec3[0, 0] == float(sse)                                           # exact integer SSE


@pytest.mark.gpu
def test_nonfinite_input_raises():
    o, g = _pairs(3, 27, 43, seed=3)
    of, gf = _as_float(o[:2]).cuda(), _as_float(g[:2]).cuda()
    of[1, 2, 5, 7] = float("nan")
    gf[1, 0, 0, 0] = float("inf")
    rec, u8 = metrics.image_metrics_records(of, gf, 0)
    assert rec[0, 6] == 0 and rec[1, 6] == 2
    assert u8[1, 5, 7, 0] == 0                                                # RGB plane 2 -> BGR byte 0
    with pytest.raises(RuntimeError, match="non-finite"):
        metrics.image_metrics_device(of, gf, 0)
    with pytest.raises(ValueError):
        metrics.image_metrics_device(of[:, :, :10], gf[:, :, :10], 0)        # H = 10


def _write_pair(root, n=3, sizes=((32, 32), (32, 32), (40, 48))):
    lq, gt = root / "LQ", root / "GT"
    lq.mkdir(), gt.mkdir()
    rng = np.random.default_rng(0)
    for i in range(n):
        h, w = sizes[i]
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(lq / f"img{i}.png")
        Image.fromarray(np.clip(a.astype(int) + 7, 0, 255).astype(np.uint8)).save(gt / f"img{i}.png")
    return str(lq), str(gt)


@pytest.mark.gpu
def test_evaluate_device_matches_host(tmp_path):
    from daclip_amd.evaluate import evaluate
    opt = {"model": "denoising",
           "sde": {"max_sigma": 50, "T": 3, "schedule": "cosine", "eps": 0.005, "sampling_mode": "posterior"},
           "network_G": {"which_model_G": "ConditionalUNet",
                         "setting": {"in_nc": 3, "out_nc": 3, "nf": 64, "ch_mult": [1, 2, 4, 8],
                                     "context_dim": 512, "use_degra_context": True, "use_image_context": True}},
           "path": {"pretrain_model_G": None}}
    lq, gt = _write_pair(tmp_path)
    res = {}
    for mode in ("host", "device"):
        torch.manual_seed(0)
        res[mode] = evaluate(opt, lq, gt, str(tmp_path / mode), batch=2, synthetic=True, crop_border=4,
                             metrics=mode)
    for name in ("img0.png", "img1.png", "img2.png"):
        assert (tmp_path / "host" / name).read_bytes() == (tmp_path / "device" / name).read_bytes(), name
    hs, ds = res["host"]["summary"], res["device"]["summary"]
    assert ds["images"] == 3
    for k in ("psnr", "ssim", "psnr_y", "ssim_y"):
        print(f"summary {k}: device {ds[k]!r} host {hs[k]!r} |diff| {abs(ds[k] - hs[k]):.3e}")
        assert abs(ds[k] - hs[k]) <= 1e-10, (k, ds[k], hs[k])
    for name, hrec in res["host"]["per_image"].items():
        drec = res["device"]["per_image"][name]
        for k in ("psnr", "ssim", "psnr_y", "ssim_y"):
            assert abs(drec[k] - hrec[k]) <= 1e-10, (name, k, drec[k], hrec[k])
        assert drec["lpips"] is None
