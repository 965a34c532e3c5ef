"""Tiled against untiled restore of one large synthetic image (recorded in DESIGN.md §10, not asserted):

  (a) IRSDE.reverse_posterior(tile=256, tile_overlap=32, tiles_per_forward=16): tiles blended at
      every sampler step (dac_sde_reverse_tiled);
  (b) IRSDE.reverse_posterior over the whole image (dac_sde_reverse), the only path before.

    python tools/tiled_bench.py [--size 1024] [--tile 256] [--overlap 32] [--tpf 16] [--dtype fp16]
                                [--T 100] [--reps 2] [--only tiled|untiled]

One process, synthetic weights, device noise. Prints one JSON line: seconds per image (median over
the repetitions after one warm-up call, which also captures the loop) and megapixels/s for each.
Run it under `timeout`; (b) may be taken on its own with --only untiled.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "da-clip_amd"))

import torch  # noqa: E402

from daclip_amd import synth, tiling  # noqa: E402
from daclip_amd.sde import IRSDE  # noqa: E402
from daclip_amd.unet import ConditionalUNet  # noqa: E402


def timed(fn, reps):
    fn()                                     # warm-up: allocations, capture, instantiation
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--tpf", type=int, default=16)
    ap.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default=None, choices=["tiled", "untiled"])
    a = ap.parse_args(argv)
    S = a.size
    m = ConditionalUNet(3, 3, 64, [1, 2, 4, 8], 512, True, True, dtype=a.dtype)
    m.load_synthetic(0)
    sde = IRSDE(max_sigma=50, T=100, sample_T=a.T, schedule="cosine", eps=0.005)
    sde.set_model(m)
    T = lambda arr: torch.from_numpy(arr).cuda()
    mu = T(0.5 + 0.15 * synth.synth_noise((1, 3, S, S), 0, "tb_mu")).clamp(0, 1)
    sde.set_mu(mu)
    x = sde.noise_state(mu, noise=T(synth.synth_noise((1, 3, S, S), 0, "tb_x0")))
    kw = dict(text_context=T(synth.synth_noise((1, 512), 0, "tb_tc")),
              image_context=T(synth.synth_noise((1, 512), 0, "tb_ic")))
    th, tw, ys, xs = tiling.plan(S, S, a.tile, a.overlap)
    res = {"size": S, "dtype": a.dtype, "T": a.T, "tile": [th, tw], "overlap": a.overlap,
           "tiles": len(ys) * len(xs), "tiles_per_forward": a.tpf}
    mp = S * S / 1e6
    runs = {"tiled": lambda: sde.reverse_posterior(x, tile=a.tile, tile_overlap=a.overlap,
                                                   tiles_per_forward=a.tpf, **kw),
            "untiled": lambda: sde.reverse_posterior(x, **kw)}
    for name, fn in runs.items():
        if a.only and a.only != name:
            continue
        ts, out = timed(fn, a.reps)
        s = statistics.median(ts)
        res[name] = {"s_per_image": s, "mpix_per_s": mp / s, "min_s": min(ts), "max_s": max(ts),
                     "finite": bool(torch.isfinite(out).all())}
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
