"""The in-engine profiler (csrc/profiler.*, the dac_profile_* entry points).

CPU: tools/profiler_check.cpp drives the HIP-free part (stamp reduction, summary, report, bounds,
pass state, symbol-owner table) under host ASan + UBSan.

GPU: the standard synthetic UNet in fp16 on a 2 x 3 x 8 x 256 input, 2 steps of the T = 100 cosine
schedule with injected noise: the smallest input that has fused-ResBlock launches (class 350:
64 channels need W >= 256, W % 128 == 0), launches inside the split section's concurrent branches
(B = 2) and ordinary conv launches. tests/golden/profile_launches.json holds, for the stamped and
the eager pass with class 999, every launch's (class, label, flops, bytes, in_branch, symbol base
names), recorded with `python tests/test_profiler.py --record` before the profiler became a unit
of its own. A symbol's base names are its `+`-separated parts reduced to the kernel's own name
(the last name of a mangled symbol's scope, or the text before the first `<`), so the table
survives a change of tile choice but not of kernel family.

The eager pass runs the split section as full-batch launches; its restored x was bit-identical
to the captured loop's when the table was recorded (results do not depend on the batch split),
so both passes are held to bit-identity with the unprofiled call.
"""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "profile_launches.json")
B, H, W, STEPS, DTYPE = 2, 8, 256, 2, "fp16"
ALL = 999


# ----------------------------------------------------------------------------- CPU
def test_profiler_host_check():
    exe = os.path.join(ROOT, "tools", "profiler_check")
    if not os.path.exists(exe):
        if not any(shutil.which(c) for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")):
            pytest.skip("no host C++ compiler")
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "da-clip_amd"), "profcheck"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


# ----------------------------------------------------------------------------- GPU helpers
def base_names(symbol):
    out = []
    for part in symbol.split("+") if symbol else []:
        if part.startswith("_ZN"):                  # _ZN <len><name>... : the last name of the scope
            i, name = 3, ""
            while (m := re.match(r"\d+", part[i:])):
                n = int(m.group())
                name = part[i + len(m.group()):i + len(m.group()) + n]
                i += len(m.group()) + n
            out.append(name)
        else:
            out.append(part.split("<")[0])
    return out


class Session:
    """One fp16 handle and one set of inputs; every call restores the same x."""

    def __init__(self, unet_sd):
        import torch
        from daclip_amd import _lib, synth
        from daclip_amd.sde import IRSDE
        from daclip_amd.unet import ConditionalUNet
        self.torch, self.L = torch, _lib.lib()
        m = ConditionalUNet(3, 3, 64, [1, 2, 4, 8], 512, True, True, dtype=DTYPE)
        m.load_state_dict(unet_sd)
        self.h = m._h
        self.sde = IRSDE(max_sigma=50, T=100, schedule="cosine", eps=0.005)
        self.sde.set_model(m)
        T = lambda a: torch.from_numpy(a).cuda()
        self.mu = T(0.5 + 0.15 * synth.synth_noise((B, 3, H, W), 0, "prof_mu")).clamp(0, 1)
        self.x = self.mu + T(synth.synth_noise((B, 3, H, W), 0, "prof_x0")) * (50 / 255)
        self.z = T(synth.synth_noise((STEPS, B, 3, H, W), 0, "prof_steps"))
        self.tc = T(synth.synth_noise((B, 512), 0, "prof_tc"))
        self.ic = T(synth.synth_noise((B, 512), 0, "prof_ic"))

    def restore(self):
        self.sde.set_mu(self.mu)
        out = self.sde.reverse_posterior(self.x, T=STEPS, noises=self.z, text_context=self.tc, image_context=self.ic)
        self.torch.cuda.synchronize()
        return out

    def read(self):
        """(rc of dac_profile_read, mean ms, flops / launch, bytes / launch)."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = self.L.dac_profile_read(self.h.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return n, a.value, b.value, c.value

    def launch(self, i):
        """(rc, row): row = dict of the eight fields of launch i."""
        c = ctypes
        ms, fl, by, cls, t0, br = c.c_double(), c.c_double(), c.c_double(), c.c_int(), c.c_double(), c.c_int()
        lab, sym = c.create_string_buffer(200), c.create_string_buffer(400)
        rc = self.L.dac_profile_launch(self.h.h, i, c.byref(ms), c.byref(fl), c.byref(by), c.byref(cls),
                                       c.byref(t0), c.byref(br), lab, 200, sym, 400)
        return rc, dict(ms=ms.value, flops=fl.value, bytes=by.value, cls=cls.value, t0=t0.value, in_branch=br.value,
                        label=lab.value.decode(), symbol=sym.value.decode())

    def rows(self, n):
        out = []
        for i in range(max(n, 0)):
            rc, row = self.launch(i)
            assert rc == 0, (i, rc)
            out.append(row)
        return out

    def graph_ms(self):
        g = ctypes.c_double()
        self.h.check(self.L.dac_profile_graph_ms(self.h.h, ctypes.byref(g)), "profile_graph_ms")
        return g.value

    def profiled(self, mode, cls):
        """One profiled restore: dict(x, read, rows, graph_ms). Leaves profiling enabled."""
        self.h.check(self.L.dac_profile_mode(self.h.h, mode), "profile_mode")
        self.h.check(self.L.dac_profile_enable(self.h.h, cls), "profile_enable")
        x = self.restore()
        rd = self.read()
        return dict(x=x, read=rd, rows=self.rows(rd[0]), graph_ms=self.graph_ms())

    def off(self):
        self.L.dac_profile_enable(self.h.h, -1)
        self.L.dac_profile_mode(self.h.h, 0)


def golden_row(r):
    return [r["cls"], r["label"], r["flops"], r["bytes"], r["in_branch"], base_names(r["symbol"])]


def other_class(golden):
    """The lowest class other than 350 that both golden tables contain."""
    both = {r[0] for r in golden["stamped"]} & {r[0] for r in golden["eager"]}
    return min(both - {350})


# ----------------------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope="module")
def golden_table():
    with open(GOLDEN_FILE) as f:
        g = json.load(f)
    assert g["input"] == [B, 3, H, W] and g["steps"] == STEPS and g["dtype"] == DTYPE
    return g


@pytest.fixture(scope="module")
def runs(unet_sd, golden_table):
    """Every GPU call of this module, made once, in the order the bit-identity check needs: the
    stamped pass comes first on a fresh handle, so the first unprofiled call after it captures
    the loop graph and the second replays it."""
    s = Session(unet_sd)
    r = {"s": s}
    try:
        r["stamped"] = s.profiled(1, ALL)
        s.h.check(s.L.dac_profile_mode(s.h.h, 0), "profile_mode")         # the flip: the next pass would be eager
        rd = s.read()
        r["flipped"] = dict(read=rd, rows=s.rows(rd[0]), graph_ms=s.graph_ms())
        r["bounds"] = [(s.launch(i)[0], s.L.dac_last_error(s.h.h).decode()) for i in (-1, rd[0])]
        s.off()
        r["plain"] = [s.restore(), s.restore()]
        r["eager"] = s.profiled(0, ALL)
        for cls in (350, other_class(golden_table)):
            for mode, name in ((1, "stamped"), (0, "eager")):
                r[name, cls] = s.profiled(mode, cls)
    finally:
        s.off()
    return r


def check_ms(rows):
    assert all(math.isfinite(r["ms"]) and r["ms"] > 0 for r in rows)


# ----------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
def test_stamped_pass(runs, golden_table):
    p, want = runs["stamped"], golden_table["stamped"]
    assert p["read"][0] == len(want)
    assert [golden_row(r) for r in p["rows"]] == want
    check_ms(p["rows"])
    assert min(r["t0"] for r in p["rows"]) == 0
    assert p["graph_ms"] > 0
    assert any(r["cls"] == 350 for r in p["rows"]) and any(r["in_branch"] == 1 for r in p["rows"])
    assert all(r["symbol"] for r in p["rows"])


@pytest.mark.gpu
def test_eager_pass(runs, golden_table):
    p, want = runs["eager"], golden_table["eager"]
    n, mean_ms, fl, by = p["read"]
    assert n == len(want)
    assert [golden_row(r) for r in p["rows"]] == want
    assert all(r["in_branch"] == 0 and r["symbol"] == "" for r in p["rows"])
    check_ms(p["rows"])
    assert fl == sum(w[2] for w in want) / n and by == sum(w[3] for w in want) / n
    assert mean_ms == pytest.approx(sum(r["ms"] for r in p["rows"]) / n, rel=1e-12, abs=0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fused ResBlock", "other"])
def test_one_class(runs, golden_table, which):
    cls = 350 if which == "fused ResBlock" else other_class(golden_table)
    for name in ("stamped", "eager"):
        want = [w for w in golden_table[name] if w[0] == cls]
        p = runs[name, cls]
        assert want and p["read"][0] == len(want), (name, cls)
        assert [golden_row(r) for r in p["rows"]] == want, (name, cls)
        check_ms(p["rows"])


@pytest.mark.gpu
def test_read_after_mode_flip(runs):
    """dac_profile_mode only chooses the next pass: the last pass reads as it ran."""
    a, b = runs["stamped"], runs["flipped"]
    assert b["read"] == a["read"] and b["rows"] == a["rows"] and b["graph_ms"] == a["graph_ms"]


@pytest.mark.gpu
def test_profiling_leaves_result_alone(runs):
    torch = runs["s"].torch
    x = runs["stamped"]["x"]
    assert torch.isfinite(x).all()
    assert torch.equal(x, runs["plain"][0])          # captures the loop graph
    assert torch.equal(x, runs["plain"][1])          # replays it
    assert torch.equal(x, runs["eager"]["x"])         # full-batch launches in the split section
    assert torch.equal(x, runs["stamped", 350]["x"]) and torch.equal(x, runs["eager", 350]["x"])


@pytest.mark.gpu
def test_launch_index_bounds(runs):
    from daclip_amd import _lib
    for rc, msg in runs["bounds"]:
        assert rc == _lib.DAC_E_ARG and msg


# ----------------------------------------------------------------------------- recorder
def record(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "da-clip_amd")]
    from daclip_amd import arch, synth
    s = Session(synth.synth_state_dict(arch.unet_state_spec(arch.UNetConfig()), seed=0))
    try:
        st = s.profiled(1, ALL)
        s.off()
        plain = s.restore()
        eg = s.profiled(0, ALL)
    finally:
        s.off()
    out = {"input": [B, 3, H, W], "steps": STEPS, "dtype": DTYPE,
           "stamped": [golden_row(r) for r in st["rows"]], "eager": [golden_row(r) for r in eg["rows"]]}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            f' "{k}": ' + (json.dumps(v) if not isinstance(v, list) or not v or not isinstance(v[0], list)
                           else "[\n  " + ",\n  ".join(json.dumps(r) for r in v) + "\n ]")
            for k, v in out.items()) + "\n}\n")
    n350 = sum(r["cls"] == 350 for r in st["rows"])
    nbr = sum(r["in_branch"] for r in st["rows"])
    print(f"recorded {len(st['rows'])} stamped / {len(eg['rows'])} eager rows to {path}: {n350} class-350 rows, "
          f"{nbr} in_branch rows, classes {sorted({r['cls'] for r in st['rows']})} / "
          f"{sorted({r['cls'] for r in eg['rows']})}")
    print(f"stamped x == unprofiled x: {s.torch.equal(st['x'], plain)}; eager x == unprofiled x: "
          f"{s.torch.equal(eg['x'], plain)}")
    print("symbols:", sorted({r["symbol"] for r in st["rows"]})[:6])


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_profiler.py --record [FILE]")
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN_FILE)
