"""Host against device evaluation metrics at the bench shape (256x256x3, crop_border 4):

  (a) metrics.image_metrics (host numpy) per image;
  (b) metrics.image_metrics_device per image at B images per call, wall time of the whole call
      (allocations, three kernels, read-back of the records and the uint8 images), plus the
      kernels alone from device events;
  (c) (b) as a fraction of the restore time per image (encode + T-step posterior loop on
      synthetic weights) measured in this process.

    python tools/metrics_bench.py [--batch 8] [--size 256] [--crop 4] [--reps 30] [--host-reps 5]
                                  [--dtype bf16] [--T 100] [--no-restore]

Prints one JSON line: medians with min / max over the repetitions, after warm-up.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "da-clip_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from daclip_amd import metrics  # noqa: E402
from daclip_amd.preprocess import tensor2img  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--crop", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--no-restore", action="store_true")
    a = ap.parse_args(argv)
    B, S, cb = a.batch, a.size, a.crop
    rng = np.random.default_rng(0)
    gt_u8 = rng.integers(0, 256, (B, 3, S, S), dtype=np.uint8)
    out_u8 = np.clip(gt_u8.astype(int) + rng.integers(-6, 7, gt_u8.shape), 0, 255).astype(np.uint8)
    out = torch.from_numpy(out_u8.astype(np.float32) / np.float32(255.0))
    gt = torch.from_numpy(gt_u8.astype(np.float32) / np.float32(255.0))
    res = {"shape": [B, 3, S, S], "crop_border": cb}

    # (a) host: quantise + score one image, as evaluate(metrics="host") does per image
    ho, hg = tensor2img(out[0]), tensor2img(gt[0])
    metrics.image_metrics(ho, hg, cb)                                         # warm-up
    host, host_q = [], []
    for i in range(a.host_reps):
        k = i % B
        t0 = time.perf_counter()
        ho, hg = tensor2img(out[k]), tensor2img(gt[k])
        t1 = time.perf_counter()
        ref = metrics.image_metrics(ho, hg, cb)
        host.append(time.perf_counter() - t1)
        host_q.append(t1 - t0)
    res["host_image_metrics_s_per_image"] = spread(host)
    res["host_tensor2img_pair_s_per_image"] = spread(host_q)

    # (b) device
    od, gd = out.cuda(), gt.cuda()
    for _ in range(5):
        rows, _u8 = metrics.image_metrics_device(od, gd, cb)
    k = (a.host_reps - 1) % B
    res["max_abs_diff_vs_host"] = max(abs(rows[k][key] - ref[key]) for key in ref)
    wall, kern = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics.image_metrics_device(od, gd, cb)
        wall.append((time.perf_counter() - t0) / B)
    from daclip_amd import _lib
    L = _lib.lib()
    ws = torch.empty(L.dac_image_metrics_workspace(B, 3, S, S, cb) // 8 + 1, dtype=torch.float64, device="cuda")
    o8, g8 = (torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    rec = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    for _ in range(a.reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.dac_image_metrics(_lib._ptr(od), _lib._ptr(gd), B, 3, S, S, cb, _lib._ptr(o8), _lib._ptr(g8),
                                 _lib._ptr(rec), _lib._ptr(ws), _lib._stream(od.device))
        e1.record()
        assert rc == 0, rc
        e1.synchronize()
        kern.append(e0.elapsed_time(e1) * 1e-3 / B)
    res["device_call_s_per_image"] = spread(wall)
    res["device_kernels_s_per_image"] = spread(kern[5:])
    res["host_over_device"] = res["host_image_metrics_s_per_image"]["median"] / res["device_call_s_per_image"]["median"]

    # (c) restore time per image in this process
    if not a.no_restore:
        from daclip_amd.evaluate import _setup
        opt = {"model": "denoising",
               "sde": {"max_sigma": 50, "T": a.T, "schedule": "cosine", "eps": 0.005, "sampling_mode": "posterior"},
               "network_G": {"which_model_G": "ConditionalUNet",
                             "setting": {"in_nc": 3, "out_nc": 3, "nf": 64, "ch_mult": [1, 2, 4, 8],
                                         "context_dim": 512, "use_degra_context": True,
                                         "use_image_context": True}},
               "path": {"pretrain_model_G": None}}
        model, clip, sde, mode = _setup(opt, "cuda", a.dtype, True, "daclip_ViT-B-32")
        img4clip = torch.rand(B, 3, 224, 224, device=model.device)
        restore = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                ic, dc = clip.encode_image(img4clip, control=True)
            model.feed_data(sde.noise_state(out), out, gt, text_context=dc.float(), image_context=ic.float())
            model.test(sde, mode=mode, save_states=False)
            torch.cuda.synchronize()
            if i:                                                             # first pass: capture + warm-up
                restore.append((time.perf_counter() - t0) / B)
        res["restore_s_per_image"] = dict(spread(restore), dtype=a.dtype, T=a.T)
        res["device_metrics_over_restore"] = res["device_call_s_per_image"]["median"] / res["restore_s_per_image"]["median"]
        res["host_metrics_over_restore"] = res["host_image_metrics_s_per_image"]["median"] / res["restore_s_per_image"]["median"]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
