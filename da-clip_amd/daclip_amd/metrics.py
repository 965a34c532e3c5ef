"""Image-quality metrics of the reference evaluation: host-side numpy like the reference
(`image_metrics`, the yardstick), and the same numbers from the fp64 HIP kernels of
csrc/metrics.hip for a batch that is still on the GPU (`image_metrics_device`).

* calculate_psnr: utils/img_utils.py:182-189 (float64 MSE over all pixels, inf if equal).
* ssim / calculate_ssim: utils/img_utils.py:192-234. Gaussian window 11x11, sigma 1.5 (the
  normalised cv2.getGaussianKernel(11, 1.5) outer product), per-channel 'valid' filtering
  (cv2.filter2D followed by the [5:-5, 5:-5] crop, so the border mode never matters), C1/C2
  of the 8-bit range. For 3-channel images the reference evaluates ssim on the whole HxWx3
  array (three times) -- i.e. the mean over all channels' SSIM maps; restated as such.
  Parity with cv2 is UNPINNED (cv2 is absent offline); tests check an independent direct
  window sum and SSIM identities.
* bgr2ycbcr: data/util.py:189-210 (BT.601, MATLAB-compatible); pinned by
  tests/golden/img_metrics.npz. Unlike the reference it does not scale a float input in place.
"""
from __future__ import annotations

import math

import numpy as np

from .preprocess import calculate_psnr  # noqa: F401  (utils/img_utils.py:182-189)


def gaussian_window(size: int = 11, sigma: float = 1.5) -> np.ndarray:
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g)


def _filter_valid(img: np.ndarray, win: np.ndarray) -> np.ndarray:
    """Correlation of each channel with `win`, 'valid' region only (== filter2D + crop)."""
    k = win.shape[0]
    v = np.lib.stride_tricks.sliding_window_view(img, (k, k), axis=(0, 1))
    return np.einsum("ij...kl,kl->ij...", v, win) if img.ndim == 2 else np.einsum("ijckl,kl->ijc", v, win)


def ssim(img1: np.ndarray, img2: np.ndarray) -> float:
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    w = gaussian_window()
    mu1, mu2 = _filter_valid(a, w), _filter_valid(b, w)
    s1 = _filter_valid(a * a, w) - mu1 * mu1
    s2 = _filter_valid(b * b, w) - mu2 * mu2
    s12 = _filter_valid(a * b, w) - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return float(m.mean())


def calculate_ssim(img1: np.ndarray, img2: np.ndarray) -> float:
    if img1.shape != img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if img1.ndim == 2:
        return ssim(img1, img2)
    if img1.ndim == 3:
        if img1.shape[2] == 3:
            return ssim(img1, img2)        # the reference's 3 identical calls, averaged
        if img1.shape[2] == 1:
            return ssim(np.squeeze(img1), np.squeeze(img2))
    raise ValueError("Wrong input image dimensions.")


def bgr2ycbcr(img: np.ndarray, only_y: bool = True) -> np.ndarray:
    in_type = img.dtype
    x = img.astype(np.float64) * (1.0 if in_type == np.uint8 else 255.0)
    if only_y:
        r = np.dot(x, [24.966, 128.553, 65.481]) / 255.0 + 16.0
    else:
        r = np.matmul(x, [[24.966, 112.0, -18.214], [128.553, -74.203, -93.786],
                          [65.481, -37.797, 112.0]]) / 255.0 + [16, 128, 128]
    r = r.round() if in_type == np.uint8 else r / 255.0
    return r.astype(in_type)


def crop(img: np.ndarray, border: int) -> np.ndarray:
    return img if border == 0 else img[border:-border, border:-border]


def image_metrics(out_u8: np.ndarray, gt_u8: np.ndarray, crop_border: int = 0) -> dict:
    """test.py:146-196 for one image: PSNR / SSIM on BGR uint8 (as [0,1] floats * 255) and
    PSNR_Y / SSIM_Y on the Y channel. LPIPS needs its pretrained net (absent): not computed."""
    sr, gt = out_u8 / 255.0, gt_u8 / 255.0
    res = {"psnr": calculate_psnr(crop(sr, crop_border) * 255, crop(gt, crop_border) * 255),
           "ssim": calculate_ssim(crop(sr, crop_border) * 255, crop(gt, crop_border) * 255)}
    if gt.ndim == 3 and gt.shape[2] == 3:
        sy, gy = bgr2ycbcr(sr, True), bgr2ycbcr(gt, True)
        res["psnr_y"] = calculate_psnr(crop(sy, crop_border) * 255, crop(gy, crop_border) * 255)
        res["ssim_y"] = calculate_ssim(crop(sy, crop_border) * 255, crop(gy, crop_border) * 255)
    return res


def image_metrics_records(out, gt, crop_border: int = 0):
    """One dac_image_metrics call: (records, out_u8) for out, gt [B,C,H,W] float tensors on one
    GPU. records is the [B, 8] float64 array {sse, n, ssim, sse_y, n_y, ssim_y, nonfinite, 0}
    of include/daclip_hip.h, out_u8 the [B,H,W,C] uint8 BGR array. Scratch and results are
    torch allocations on the inputs' device, the kernels run on its current stream."""
    import torch

    from . import _lib
    if out.dim() != 4 or tuple(out.shape) != tuple(gt.shape):
        raise ValueError(f"out and gt must be [B,C,H,W] of one shape, got {tuple(out.shape)} and {tuple(gt.shape)}")
    B, C, H, W = (int(v) for v in out.shape)
    L = _lib.lib()
    ws_bytes = L.dac_image_metrics_workspace(B, C, H, W, int(crop_border))
    if ws_bytes == 0:
        raise ValueError(f"image metrics on the device: unsupported B={B} C={C} H={H} W={W} "
                         f"crop_border={crop_border} (C in {{1, 3}}, cropped window >= 11x11)")
    if not (out.is_cuda and gt.is_cuda and out.device == gt.device):
        raise RuntimeError("image metrics on the device need out and gt on one GPU")
    dev = out.device
    with torch.cuda.device(dev):
        o = out.detach().float().contiguous()
        g = o if gt is out else gt.detach().float().contiguous()
        o8 = torch.empty((B, H, W, C), dtype=torch.uint8, device=dev)
        g8 = torch.empty((B, H, W, C), dtype=torch.uint8, device=dev)
        res = torch.empty((B, 8), dtype=torch.float64, device=dev)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
        rc = L.dac_image_metrics(_lib._ptr(o), _lib._ptr(g), B, C, H, W, int(crop_border), _lib._ptr(o8),
                                 _lib._ptr(g8), _lib._ptr(res), _lib._ptr(ws), _lib._stream(dev))
        if rc == _lib.DAC_E_ARG:
            raise ValueError(f"dac_image_metrics refused B={B} C={C} H={H} W={W} crop_border={crop_border}")
        if rc != 0:
            raise RuntimeError(f"dac_image_metrics failed ({rc})")
        return res.cpu().numpy(), o8.cpu().numpy()


def image_metrics_device(out, gt=None, crop_border: int = 0):
    """`image_metrics` and `tensor2img` for a whole batch on the GPU (csrc/metrics.hip).

    out, gt: [B,C,H,W] float tensors on one GPU, RGB, C in {1, 3}. Returns (rows, out_u8):
    rows[i] has the keys of `image_metrics` for image i (psnr, ssim, and for C = 3 psnr_y,
    ssim_y); out_u8 is the [B,H,W,C] uint8 numpy array, BGR, that `tensor2img` would give
    per image. gt=None: only the uint8 images are wanted (out stands in as its own gt, with no
    crop, and rows is None). ValueError: a shape the kernels refuse (unlike the host path, a
    cropped window smaller than the 11x11 filter is an error, not NaN). RuntimeError: non-finite
    inputs."""
    score = gt is not None
    r, out_u8 = image_metrics_records(out, gt if score else out, crop_border if score else 0)
    if (r[:, 6] > 0).any():
        bad = {i: int(r[i, 6]) for i in range(len(r)) if r[i, 6] > 0}
        raise RuntimeError(f"non-finite values in the images to score (image: count) {bad}")
    if not score:
        return None, out_u8

    def psnr(sse, n):
        return float("inf") if sse == 0 else 20 * math.log10(255.0 / math.sqrt(sse / n))
    rows = []
    for rec in r:
        row = {"psnr": psnr(rec[0], rec[1]), "ssim": float(rec[2])}
        if out.shape[1] == 3:
            row["psnr_y"] = psnr(rec[3], rec[4])
            row["ssim_y"] = float(rec[5])
        rows.append(row)
    return rows, out_u8
