"""The conv kernel selection (csrc/conv_plan.h) on the CPU: `tools/convbench plan FILE` prints the
plan for each conv call of FILE before any HIP call.

Pinned rows (tests/golden/conv_plan_rows.txt): every distinct conv call of the headline UNet
restore (nf 64, 256x256, B = 8 and the half batch of the split levels; fp16, bf16, fp8, fp32),
the Wild-IR restore at 512x512, and the ViT-B/32, ViT-L/14 and text tower linears, as the engine
made them at the commit before the selection moved into conv_plan (fused res_conv, fp8 output,
row-phase upsample, LN fold, GroupNorm in A, GEGLU with w_gs, 3x3 and 1x1 split-K included; the
engine never asks for the row-LayerNorm epilogue, so no row has it). The expected kernel, tile,
stages, DMA form, grid and block of a row are the launch that commit's kernel trace shows for
it, the class the number its conv_variant returned.

Consistency sweep: a few thousand synthetic calls; the plan is a kernel whose own fit function
accepts the arguments or "none" with a reason, serves every request, agrees with the engine's
predicates, and its grid covers the output."""
import itertools
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "convbench")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_rows.txt")


def plan(rows, tmp_path):
    assert os.path.exists(BIN), "tools/convbench missing: run __graft_entry__.build()"
    f = tmp_path / "rows.txt"
    f.write_text("\n".join(rows) + "\n")
    out = subprocess.run([BIN, "plan", str(f)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    return lines


def fields(line):
    head, why = line.split(" why=")
    d = dict(x.split("=", 1) for x in head.split())
    d["why"] = why
    return d


def test_pinned_workload_rows(tmp_path):
    gold = [l.split(" | ") for l in open(GOLDEN).read().splitlines() if not l.startswith("#")]
    assert len(gold) >= 150
    seen = set(",".join(g[0] for g in gold).split(","))
    assert seen == {"restore256-fp16", "restore256-bf16", "restore256-fp8", "restore256-fp32", "wild512-fp16",
                    "vit-b32", "vit-l14", "text"}
    got = plan([g[1] for g in gold], tmp_path)
    bad = [f"{g[0]}: {g[1]}\n  expected {g[2]}\n  planned  {l}" for g, l in zip(gold, got)
           if l.split(" serves=")[0] != g[2]]
    assert not bad, "\n".join(bad)
    # The feature requests the engine makes are all among the rows.
    rows = " ".join(g[1] for g in gold)
    for req in (" y2=1", " ys8=1", " uph=1", " lnf=1", " gna=1", " gs=1", " ks=2", " ks=8"):
        assert req + " " in rows + " ", req
    # The plain small-image 1x1 GEMMs on the 128x128 4-stage tile keep class 17 (bench.py's roofline key).
    f32 = [g for g in gold if "tile=128x128" in g[2] and "st=4" in g[2] and "epi=32" in g[2]]
    assert f32 and all(g[2].endswith("label=17") for g in f32)


SIZES = [4, 8, 16, 30, 32, 48, 64, 128, 256]
CINS = [8, 32, 64, 96, 128, 192, 512]
COUTS = [3, 16, 64, 128, 192, 256, 1024]
FEATURES = ["none", "y2", "ys8", "ys8+y2", "uph", "lnf", "gna", "ln", "ks"]


def synth_row(rng, kh, es, feat, buf):
    Ho, Wo = rng.choice(SIZES), rng.choice(SIZES)
    Cin, Cout, B = rng.choice(CINS), rng.choice(COUTS), rng.choice([1, 8])
    if rng.random() < 0.5:      # the shapes the kernels are built for, so every family is exercised
        Ho = Wo = rng.choice([16, 32, 64, 128, 256])
        Cin, Cout = rng.choice([64, 128, 192, 512]), rng.choice([64, 128, 256, 1024])
    if "ys8" in feat and rng.random() < 0.6:   # the fp8-output kernels are 64 channels wide
        Cout = 64
        if feat == "ys8":
            Cin, Wo = 64, rng.choice([64, 128, 256])
    s, p = {3: (1, 1), 1: (1, 0), 4: (2, 1), 7: (1, 3)}[kh]
    up = 1 if feat == "uph" or (kh == 3 and rng.random() < 0.05) else 0
    Hs, Ws = (Ho // 2, Wo // 2) if up else (Ho * s, Wo * s)
    two = rng.random() < 0.4 and Cin % 2 == 0
    C1 = Cin // 2 if two else Cin
    ld1 = C1
    ld2 = (ld1 if rng.random() < 0.5 else ld1 + 8) if two else 0
    r = dict(kh=kh, kw=kh, s=s, p=p, es=es, B=B, Hs=Hs, Ws=Ws, up=up, Ho=Ho, Wo=Wo, Cin=Cin, C1=C1, x2=int(two),
             ld1=ld1, ld2=ld2, Cout=Cout, K=kh * kh * Cin, ldy=Cout if Cout >= 8 else 4, act=rng.choice([0, 0, 1, 1, 2, 3]),
             buf=buf)
    if r["act"] == 3:
        r["ldy"] = Cout // 2
        r["gs"] = rng.choice([0, 1])
    if rng.random() < 0.4:
        r.update(ss=1, ss_ld=2 * Cout + rng.choice([0, 0, 0, 1]), ssmis=rng.choice([0, 0, 0, 1]))
    if rng.random() < 0.3:
        r.update(res1=1, ldr1=Cout)
    if rng.random() < 0.1:
        r.update(res2=1, ldr2=Cout)
    if rng.random() < 0.1:
        r.update(bbias=1)
    if rng.random() < 0.05:
        r.update(wb=1)
    if "y2" in feat:
        r.update(y2=1, w2=1, ldy2=Cout)
    if "ys8" in feat:
        r.update(ys8=1, ldy=64 if rng.random() < 0.8 else Cout)
    if feat == "uph":
        r.update(uph=1, K=12 * Cin)
    if feat == "lnf":
        r.update(lnf=1)
    if feat == "gna":
        r.update(gna=1, groups=rng.choice([32, 32, 2, 64]))
    if feat == "ln":
        r.update(ln=1)
    if feat == "ks":
        r.update(ks=rng.choice([2, 4]))
    return r


def test_consistency_sweep(tmp_path):
    rng = random.Random(1234)
    cases = []
    for kh, es, feat, buf in itertools.product([3, 1, 4, 7], [2, 4], FEATURES, [0, 1]):
        n = 40 if kh in (3, 1) else 6
        cases += [synth_row(rng, kh, es, feat, buf) for _ in range(n)]
    assert 3000 <= len(cases) <= 8000
    rows = [" ".join(f"{k}={v}" for k, v in c.items()) for c in cases]
    kinds, served_by = set(), {}
    bad = []
    for c, row, line in zip(cases, rows, plan(rows, tmp_path)):
        d = fields(line)
        kind = d["kind"]
        kinds.add(kind)
        req = (1 if c.get("y2") else 0) | (2 if c.get("ys8") else 0) | (4 if c.get("lnf") else 0) | \
              (8 if c.get("gna") else 0) | (16 if c.get("uph") else 0) | (32 if c.get("ln") else 0) | \
              (64 if c.get("ks", 0) > 1 else 0)
        err = []
        if kind == "none":
            if d["why"] in ("-", ""):
                err.append("none without a reason")
        else:
            if d["fit"] != "1":
                err.append("the kernel's fit function rejects the arguments")
            if req & ~int(d["serves"]):
                err.append(f"request {req} on a kernel serving {d['serves']}")
            BM, BN = map(int, d["tile"].split("x"))
            gx, gy, gz = map(int, d["grid"].split(","))
            M = c["B"] * c["Ho"] * c["Wo"]
            if BM:          # tiled kernels (the others size a persistent grid in their own launcher)
                per_image = bool(c.get("wb")) and kind in ("conv2", "conv1")
                rows_z = c["Ho"] * c["Wo"] if per_image else M
                if gx * BM < rows_z or gy * BN < c["Cout"] or gz != (c["B"] if per_image else max(1, c.get("ks", 0) if "split" in kind else 1)):
                    err.append("grid does not cover M x Cout")
                if int(d["thr"]) != 64 * int(d["wg"].split("x")[0]) * int(d["wg"].split("x")[1]):
                    err.append("block size")
            elif kind == "conv3w" and (gx <= 0 or gx % 8 or d["thr"] != "512"):
                err.append("conv3w grid")
        served = kind != "none"
        served_by.setdefault(req, set()).add(served)
        for key, want in (("res", served and bool(c.get("y2"))), ("q8", served), ("uph", served), ("lnf", served),
                          ("gna", served), ("sp", kind == "conv3_split")):
            if key in d and d[key] != str(int(want)):
                err.append(f"predicate {key}={d[key]} but the plan is {kind}")
        if err:
            bad.append(f"{row}\n  {line}\n  " + "; ".join(err))
    assert not bad, f"{len(bad)} inconsistent cases, first:\n" + "\n".join(bad[:5])
    # Every request (alone, and fp8 output with the fused res_conv) is both served and refused somewhere.
    for req in (0, 1, 2, 3, 4, 8, 16, 32, 64):
        assert served_by.get(req) == ({True} if req == 0 else {True, False}), (req, served_by.get(req))
    # The sweep reaches every kernel family (conv7 / conv3n / conv_down need their exact layer shapes:
    # the pinned rows cover them).
    assert {"none", "conv3r", "conv3w", "conv3i", "conv3", "conv3_split", "conv2", "conv2_split", "conv1"} <= kinds, kinds
