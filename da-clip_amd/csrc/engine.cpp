// engine.cpp — network executors of libdaclip_hip (host C++, launches the gfx950 kernels).
//
// ConditionalUNet forward: DenoisingUNet_arch.py:118-174 (blocks: module_util.py:100-185,
//   attention.py:152-261). DaCLIP.encode_image(control=True): daclip_model.py:46-53,
//   transformer.py:288-369, 507-555. IR-SDE: utils/sde_utils.py:91-313.
// All activations are NHWC in the compute dtype T; every conv/linear goes through conv_call
// (MFMA implicit GEMM) with its elementwise tail fused into the epilogue.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dac {

// ============================================================================= precision probe
// Debug aid for locating where bf16 storage costs accuracy, fp32 handles only (off by default):
// DAC_EMU_W (PackKnobs::emu_w) / DAC_EMU_A are bit masks of UNet roles whose weights (at packing)
// / outputs (after each kernel) are rounded to bf16, emulating the bf16 engine one part at a time.
enum Role : int { R_INIT = 1, R_RB = 2, R_SAMP = 4, R_LA = 8, R_ST = 16, R_FINAL = 32, R_FIN_RB = 64,
                  R_MID = 128, R_OTHER = 256 };
// Per-image split-K count for the 3x3 convs (and split-K for the 1x1 GEMMs) of the UNet levels of
// at most 1024 pixels per image (the 32x32 level at 256^2), set by UNetNet::forward from the
// handle's policy: Wild-IR (scale-0.5) handles, whose configs[3] slice is 2 images per GPU, use 4;
// the universal handles none (DAC_SPLITK32=k overrides both; 0 = off). A function of the
// network, never of the batch: an image's summation order is the same in every batch / shard.
static thread_local int g_splitk = 0;
struct SplitKScope {
  int prev;
  explicit SplitKScope(int k) : prev(g_splitk) { g_splitk = k; }
  ~SplitKScope() { g_splitk = prev; }
};
static thread_local int g_role = R_OTHER;
struct RoleScope {
  int prev;
  explicit RoleScope(int r) : prev(g_role) { g_role = r; }
  ~RoleScope() { g_role = prev; }
};
// UNet weight key -> role (DenoisingUNet_arch.py module names).
static int key_role(const std::string& k) {
  auto has = [&](const char* s) { return k.find(s) != std::string::npos; };
  if (k.rfind("init_conv", 0) == 0) return R_INIT;
  if (k.rfind("final_conv", 0) == 0) return R_FINAL;
  if (k.rfind("final_res_block", 0) == 0) return R_FIN_RB;
  if (k.rfind("mid_", 0) == 0) return R_MID;
  if (has(".fn.fn.to_qkv") || has(".fn.fn.to_out")) return R_LA;
  if (has(".fn.fn.")) return R_ST;
  if (has("block1") || has("block2") || has("res_conv") || has(".mlp.")) return R_RB;
  if ((k.rfind("downs.", 0) == 0 && has(".3.")) || (k.rfind("ups.", 0) == 0 && has(".3."))) return R_SAMP;
  return R_OTHER;
}
template <typename T>
static void emu_round(const Run& r, void* y, int ld, size_t rows, int C);
// ============================================================================= runtime switches
// Every environment variable this file reads: one accessor each, with its read time. (The packing
// switches are PackKnobs in pack.h, the kernel-selection ones ConvKnobs in conv_plan.h.)
static bool env_on(const char* v, bool dflt) { return v ? atoi(v) != 0 : dflt; }
static long long env_num(const char* v, long long dflt) { return v ? atoll(v) : dflt; }
static bool env_is1(const char* v) { return v && v[0] == '1'; }
static bool env_is(const char* v, const char* want) { return v && !strcmp(v, want); }
static int env_mask(const char* v) { return v ? (int)strtol(v, nullptr, 0) : 0; }

// ---- read once per process
// DAC_EMU_A: the precision probe's activation role mask (above; any strtol base).
static int emu_a() { static const int m = env_mask(getenv("DAC_EMU_A")); return m; }
// DAC_Q8=0: fp8 handles keep the 16-bit ResBlock pairs (A/B switch for the e4m3 block2 path).
static bool q8_on() { static const bool on = env_on(getenv("DAC_Q8"), true); return on; }
// DAC_NO_RES_FUSE=1: run each ResBlock res_conv as its own launch (A/B switch).
static bool no_res_fuse() { static const bool on = env_on(getenv("DAC_NO_RES_FUSE"), false); return on; }
// DAC_LA256=0: the C = 256 LinearAttention (the 64x64 level) on the unfused chain, for A/B.
static bool la256_on() { static const bool on = env_on(getenv("DAC_LA256"), true); return on; }
// DAC_F16_EDGES=1: f16 handles take the bf16 handles' split-precision edge weights (precision
// probe, tools/gpu_probe16.sh).
static bool f16_edges() { static const bool on = env_on(getenv("DAC_F16_EDGES"), false); return on; }
// DAC_DUP1X1=1 (diagnostic): the 32x32-level 1x1 GEMMs run twice back to back (idempotent: the
// output never aliases an input), to separate a launch's cold-input cost in the trace.
static bool dup1x1() { static const bool on = env_on(getenv("DAC_DUP1X1"), false); return on; }
// DAC_SPLITK_PX: the largest level, in pixels per image, whose 3x3 convs split K under g_splitk.
static long splitk_px() { static const long n = (long)env_num(getenv("DAC_SPLITK_PX"), 1024); return n; }
// DAC_SPLITK32_1X1=0: the UNet's 1x1 GEMMs stay unsplit under g_splitk.
static bool splitk32_1x1() { static const bool on = env_on(getenv("DAC_SPLITK32_1X1"), true); return on; }
// DAC_SPLITK32=k: g_splitk for every handle (0 = off); unset (-1): the handle's policy.
static int splitk32() { static const int k = (int)env_num(getenv("DAC_SPLITK32"), -1); return k; }
// DAC_SPLIT_LVL: first level, counted from the bottom, of the UNet section that runs as concurrent
// branches (0 = off); DAC_SPLIT_N: how many branches.
static int split_lvl() { static const int n = (int)env_num(getenv("DAC_SPLIT_LVL"), 3); return n; }
static int split_n() { static const int n = (int)env_num(getenv("DAC_SPLIT_N"), 2); return n; }
// DAC_POISON=1: fill fresh workspace with 0xFF bytes (NaN in f32/bf16) so any read-before-write
// shows up as a NaN in the outputs (debug aid).
static bool poison() { static const bool on = env_is1(getenv("DAC_POISON")); return on; }
// DAC_NO_GRAPH=1: the sampler loops are enqueued eagerly instead of captured and replayed.
static bool no_graph() { static const bool on = env_is1(getenv("DAC_NO_GRAPH")); return on; }
// DAC_FP8_BASE=f16: fp8 handles run every non-e4m3 layer in IEEE half instead of bf16.
static bool fp8_base_f16() { static const bool on = env_is(getenv("DAC_FP8_BASE"), "f16"); return on; }

// ---- read at every use
// Norm folding switches (DAC_FOLD, a bit mask read when weights are packed and per forward):
//   1 norm1 LayerNorm folded into the SpatialTransformer's q|k|v GEMM
//   2 (unused: norm3 folded into the GEGLU proj measured slower and, in fp16 handles, not
//      batch-invariant on the restoration fixture; its kernel was deleted in round 4)
//   4 the C = 256 LinearAttention PreNorm folded into to_qkv
//   8 GroupNorm applied in proj_in's A path
//  16 ... with its statistics taken by the PreNorm LayerNorm kernel (needs 8)
// The default is the set measured faster in the network.
constexpr int kFoldDefault = 1 | 4 | 8 | 16;
static bool fold_on(int bit) { return ((int)env_num(getenv("DAC_FOLD"), kFoldDefault) & bit) != 0; }
// DAC_VIT_GEMM=0 (when weights are packed): the ViT patch stem stays the direct conv.
static bool vit_gemm_on() { return env_on(getenv("DAC_VIT_GEMM"), true); }
// DAC_FUSE_PREP=0 (per recording): every step keeps its own unet_prep launch.
static bool fuse_prep_on() { return env_on(getenv("DAC_FUSE_PREP"), true); }
// DAC_TILED_MAX_NODES (per tiled call that captures): the largest captured loop still instantiated
// as a graph (tests compare the two forms).
static size_t tiled_max_nodes(size_t dflt) { return (size_t)env_num(getenv("DAC_TILED_MAX_NODES"), (long long)dflt); }

// ============================================================================= weights
const HostW* WStore::get(const std::string& key, std::vector<int64_t> shape) {
  auto it = m.find(key);
  if (it == m.end()) {
    missing.push_back(key);
    return nullptr;
  }
  if (it->second.shape != shape) {
    std::string a, b;
    for (auto s : shape) a += std::to_string(s) + ",";
    for (auto s : it->second.shape) b += std::to_string(s) + ",";
    throw Error(DAC_E_KEY, "size mismatch for " + key + ": expected [" + a + "] got [" + b + "]");
  }
  it->second.used = true;
  return &it->second;
}

DevPool::~DevPool() {
  for (void* p : ptrs) (void)hipFree(p);
}
void* DevPool::alloc(size_t bytes) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
  ptrs.push_back(p);
  return p;
}
void* DevPool::upload(const void* host, size_t bytes) {
  void* p = alloc(bytes);
  HIP_OK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  return p;
}

// Packs a handle's weights: WStore lookups (strict-load bookkeeping), which forms a layer gets
// (ConvW fields) and the uploads. Every value comes from pack.h; no arithmetic on weights here.
template <typename T>
struct Packer {
  DevPool& pool;
  WStore& ws;
  const PackKnobs kn;                  // the environment's packing switches, read once per handle
  bool fp8 = false;                    // also build the e4m3 weights of every eligible layer
  bool q8 = false;                     // fp8 handles' UNet: e4m3 64 -> 64 ResBlock block2 weights
  static constexpr int VE = sizeof(T) == 2 ? 8 : 4;
  static constexpr Store ST = sizeof(T) == 4 ? Store::f32 : std::is_same<T, f16>::value ? Store::f16 : Store::bf16;

  template <class X> const X* up(const std::vector<X>& v) { return (const X*)pool.upload(v.data(), v.size() * sizeof(X)); }
  // fp32 handles: is `key` a weight the DAC_EMU_W probe rounds as a 16-bit handle would.
  bool emu_key(const std::string& key) const { return (kn.emu_w & key_role(key)) && !kn.emu_skips(key); }

  // Row-phase weights of a 3x3 conv applied after a 2x nearest upsample (ConvArgs::uph), rounded
  // to T once: 16-bit 3x3 without a padded kernel row.
  void make_uph(ConvW& cw, const std::vector<float>& p, const std::string& key) {
    if (sizeof(T) != 2 || cw.kh != 3 || cw.kw != 3 || cw.kwp || p.size() != (size_t)cw.cout * 9 * cw.cin) return;
    if (kn.uph == 0) return;
    cw.wph = upload_T(fold_row_phase(p, cw.cout, cw.cin), key, 12, cw.cin);
    // The row- and column-phase form is opt-in (DAC_UPH=2): measured +0.1-0.4 % in the network over
    // the row form (upsample convs 62 -> 54 and 53 -> 44 us at 256^2 / 128^2), with the restoration
    // fixture's fp16 dPSNR at -8.3e-4 dB against -2.4e-4 for the row form (RMS error unchanged,
    // 2.2e-4): too close to the 1e-3 dB bar for the default.
    if (kn.uph == 2) cw.wpc = upload_T(fold_rowcol_phase(p, cw.cout, cw.cin), key, 16, cw.cin);
  }

  // conv3q weights of a 3x3 64 -> 64 conv from its packed [64][3][3][64] fp32 values.
  void make_q8c3(ConvW& cw, const std::vector<float>& p) {
    if (!q8 || sizeof(T) != 2 || cw.kh != 3 || cw.kw != 3 || cw.cin != 64 || cw.cout != 64 || cw.kwp ||
        p.size() != (size_t)64 * 576)
      return;
    const Mx8 m = dac::make_q8c3(p);
    cw.q8w = up(m.w8);
    cw.q8s = up(m.s8);
  }

  // fp8 copy of a packed [O][K] weight (conv8.hip).
  void make_fp8(ConvW& cw, const std::vector<float>& p, int O, int K) {
    if (!fp8 || sizeof(T) != 2 || cw.cin % 64) return;
    const Mx8 m = dac::make_fp8(p, O, K);
    cw.w8 = up(m.w8);
    cw.ws8 = up(m.s8);
    cw.kp8 = m.Kp;
  }

  // v: packed [rows][taps][cin] weights, stored in T.
  const void* upload_T(const std::vector<float>& v, const std::string& key = "", int taps = 1, int cin = 1) {
    if (cin <= 1) cin = (int)v.size(), taps = 1;
    if (ST == Store::f32) {
      if (!emu_key(key)) return up(v);
      return up(emulate16(v, taps, cin, kn.emu_fp16, kn.round(Store::bf16, "")));
    }
    return up(quantize16(v, taps, cin, ST, kn.round(ST, key)));
  }
  const float* f32(const std::string& key, std::vector<int64_t> shape) {
    const HostW* w = ws.get(key, shape);
    return w ? up(w->v) : nullptr;
  }
  // [I][O] -> [O][I] fp32 (for `pooled @ proj`).
  const float* f32_t(const std::string& key, int I, int O) {
    const HostW* w = ws.get(key, {I, O});
    return w ? up(transpose_io(w->v.data(), I, O)) : nullptr;
  }
  static int pad_to(int c, int v) { return (c + v - 1) / v * v; }
  // conv weight [O][C][kh][kw] (4-D key) or linear [O][C] (2-D key, kh = kw = 1).
  // kwp > kw: each kernel row is padded to kwp taps (zero weights), so one K tile of
  // kwp * cin elements is one kernel row (the bf16 7x7 init conv: 8 taps x 8 channels).
  ConvW conv(const std::string& key, int O, int C, int kh, int kw, const std::string& bkey = "",
             bool linear2d = false, int kwp = 0, std::vector<float>* keep = nullptr) {
    ConvW cw;
    cw.cout = O; cw.cin_real = C; cw.cin = pad_to(C, VE); cw.kh = kh; cw.kw = kw;
    cw.kwp = kwp > kw ? kwp : 0;
    const int kws = cw.kwp ? cw.kwp : kw;
    const HostW* w = linear2d ? ws.get(key, {O, C}) : ws.get(key, {O, C, kh, kw});
    if (!bkey.empty()) cw.b = f32(bkey, {O});
    if (!w) return cw;
    std::vector<float> p = pack_ohwi(w->v.data(), O, C, kh, kw, kws, cw.cin);
    cw.w = upload_T(p, key, kh * kws, cw.cin);
    make_fp8(cw, p, O, kh * kws * cw.cin);
    if (keep) *keep = std::move(p);
    return cw;
  }
  ConvW linear(const std::string& key, int O, int I, const std::string& bkey = "") {
    return conv(key, O, I, 1, 1, bkey, true);
  }
  // Split-precision weights (16-bit handles; fp32 handles keep plain fp32 weights), pack_dual's
  // [hi | lo] layouts. The layer then computes A.hi + A.lo in one fp32 accumulator: weight error
  // ~2^-17 (bf16) / 2^-23 (f16) relative instead of 2^-9 / 2^-12.
  ConvW conv_dual(const std::string& key, int O, int C, int kh, int kw, const std::string& bkey = "",
                  int kwp = 0) {
    if (sizeof(T) == 4) return conv(key, O, C, kh, kw, bkey, false, kwp);
    ConvW cw;
    cw.cout = O; cw.cin_real = C; cw.cin = pad_to(C, VE); cw.kh = kh; cw.kw = kw;
    cw.kwp = kwp > kw ? kwp : 0;
    cw.dual = 1;
    const HostW* w = ws.get(key, {O, C, kh, kw});
    if (!bkey.empty()) cw.b = f32(bkey, {O});
    if (!w) return cw;
    cw.w = up(pack_dual(w->v.data(), O, C, kh, kw, cw.kwp, cw.cin, ST));
    return cw;
  }
  // Input-LayerNorm fold of a packed [O][K] 1x1 weight p (ConvArgs::lnf_cs; 16-bit handles only).
  struct Folded { ConvW cw; const float* cs = nullptr; };
  // bkey empty: a gain-only LayerNorm (module_util.py:77-86); gshape: the gain's stored shape.
  Folded fold_ln(const ConvW& base, const std::vector<float>& p, int O, int K, const std::string& gkey,
                 const std::string& bkey, const std::vector<float>* pb, std::vector<int64_t> gshape = {}) {
    Folded f;
    f.cw = base;
    f.cw.w8 = nullptr; f.cw.ws8 = nullptr; f.cw.kp8 = 0;
    if constexpr (sizeof(T) != 2) return f;
    if (gshape.empty()) gshape = {K};
    const HostW* g = ws.get(gkey, gshape);
    const HostW* be = bkey.empty() ? nullptr : ws.get(bkey, {K});
    if (!g || (!bkey.empty() && !be) || p.size() != (size_t)O * K || base.cin != K) return f;
    const FoldedLN fl = dac::fold_ln(p, O, K, g->v.data(), be ? be->v.data() : nullptr, pb ? pb->data() : nullptr, ST);
    f.cw.w = up(fl.w);
    f.cw.b = up(fl.bias);
    f.cs = up(fl.cs);
    return f;
  }
  // Row-concatenation of several [Oi][I] linears (q | k | v) into one GEMM, the first block's
  // rows times `scale0` before rounding.
  ConvW concat(const std::vector<std::string>& keys, int O, int I, std::vector<float>* keep = nullptr,
               float scale0 = 1.f) {
    ConvW cw;
    cw.cout = O * (int)keys.size(); cw.cin = cw.cin_real = I;
    std::vector<const float*> parts;
    for (auto& k : keys)
      if (const HostW* w = ws.get(k, {O, I})) parts.push_back(w->v.data());
    if (parts.size() != keys.size()) return cw;
    std::vector<float> p = concat_rows(parts.data(), (int)parts.size(), O, I, scale0);
    cw.w = upload_T(p, keys[0]);
    make_fp8(cw, p, cw.cout, I);
    if (keep) *keep = std::move(p);
    return cw;
  }
  // GEGLU proj [2F][I] (+bias) in the geglu_rows order and, for 16-bit handles with F % 32 == 0,
  // again in the swapped-tile order (ConvArgs::w_gs).
  ConvW geglu(const std::string& key, const std::string& bkey, int F, int I) {
    ConvW cw;
    cw.cout = 2 * F; cw.cin = cw.cin_real = I;
    const HostW* w = ws.get(key, {2 * F, I});
    const HostW* b = ws.get(bkey, {2 * F});
    if (!w || !b) return cw;
    const std::vector<int> rows = geglu_rows(F);
    const std::vector<float> p = gather_rows(w->v.data(), rows, I);
    cw.w = upload_T(p, key);
    make_fp8(cw, p, 2 * F, I);
    cw.b = up(gather_rows(b->v.data(), rows, 1));
    if (sizeof(T) == 2 && F % 32 == 0) {
      const std::vector<int> gs = geglu_gs_rows(F);
      cw.w_gs = upload_T(gather_rows(w->v.data(), gs, I), key);
      cw.b_gs = up(gather_rows(b->v.data(), gs, 1));
    }
    return cw;
  }
};

// ============================================================================= launches
// One launch of conv class `cls`, timed when the Run's profiler wants that class: launch(stamp)
// enqueues it (stamp: the launch's stamp block in a stamped pass, else null). A dry run launches
// nothing and counts the launches a live one will time; the label is only built for those.
template <class Label, class Launcher>
static void timed(Run& r, int cls, double flops, double bytes, Label&& make_label, Launcher&& launch) {
  Profiler* p = r.prof && r.prof->wants(cls) ? r.prof : nullptr;
  if (r.dry) {
    if (p) p->counted++;
    return;
  }
  launch(p ? p->begin(r.st) : nullptr);
  if (p) p->end(r.st, Launch{cls, flops, bytes, 0.0, -1.0, r.in_branch, make_label(), std::string()});
}

// The kernel arguments of a conv_call (the fused res_conv's fields included when requested).
static ConvArgs conv_args(const Run& r, const ConvW& cw, const void* x1, int ld1, int C1, const void* x2, int ld2,
                          int B, int Hs, int Ws, int up, int stride, int pad, void* y, int ldy, const Epi& e) {
  ConvArgs a{};
  a.x1 = x1; a.x2 = x2; a.ld1 = ld1; a.ld2 = ld2; a.C1 = C1; a.Cin = cw.cin;
  a.Hs = Hs; a.Ws = Ws; a.up = up; a.B = B;
  const int Hin = up ? 2 * Hs : Hs, Win = up ? 2 * Ws : Ws;
  a.Ho = (Hin + 2 * pad - cw.kh) / stride + 1;
  a.Wo = (Win + 2 * pad - cw.kw) / stride + 1;
  a.Cout = cw.cout; a.K = cw.kh * (cw.kwp ? cw.kwp : cw.kw) * cw.cin; a.w = cw.w; a.bias = cw.b;
  a.cwrap = 0;
  if (cw.dual) {
    // [hi | lo] along K: the input is read twice (ConvArgs::cwrap).
    a.K *= 2;
    if (cw.kwp) {
      a.cwrap = 1;                                   // 7x7 row-tap layout: kernel rows wrap
    } else if (x2 == nullptr) {
      a.Cin = 2 * cw.cin; a.x2 = x1; a.ld2 = ld1; a.C1 = cw.cin;   // second copy via x2
    } else {
      a.Cin = 2 * cw.cin; a.cwrap = cw.cin;          // [x1 | x2 | x1 | x2]
    }
  }
  a.ss = e.ss; a.ss_ld = e.ss_ld; a.res1 = e.res1; a.ldr1 = e.ldr1; a.res2 = e.res2;
  a.ldr2 = e.ldr2; a.bbias = e.bbias; a.bb_ld = e.bb_ld; a.y = y; a.ldy = ldy; a.act = e.act;
  a.amode = e.amode; a.w_bstride = e.w_bstride; a.zero = r.zero; a.ln_g = e.ln_g; a.ln_eps = e.ln_eps;
  a.lnf_cs = e.lnf_cs; a.lnf_n = e.lnf_n; a.lnf_eps = e.lnf_eps;
  a.gna_stats = e.gna_stats; a.gna_g = e.gna_g; a.gna_b = e.gna_b; a.gna_groups = e.gna_groups;
  a.gna_nb = e.gna_nb; a.gna_eps = e.gna_eps;
  a.ys8 = e.ys8; a.xs8 = e.xs8;
  if (e.act == ACT_GEGLU) { a.w_gs = cw.w_gs; a.b_gs = cw.b_gs; }
  if (e.fuse1x1) {
    a.w2 = e.fuse1x1->w; a.w2_dual = e.fuse1x1->dual; a.bias2 = e.fuse1x1->b; a.y2 = e.y2; a.ldy2 = e.ldy2;
  }
  return a;
}

template <typename T>
void conv_call(Run& r, const ConvW& cw, const void* x1, int ld1, int C1, const void* x2, int ld2,
               int B, int Hs, int Ws, int up, int stride, int pad, void* y, int ldy,
               const Epi& e) {
  ConvArgs a = conv_args(r, cw, x1, ld1, C1, x2, ld2, B, Hs, Ws, up, stride, pad, y, ldy, e);
  const double M = (double)B * a.Ho * a.Wo;
  double fl = 2.0 * M * cw.cout * cw.kh * cw.kw * cw.cin_real;
  if (cw.wph && up && stride == 1 && pad == 1 && !cw.dual && !e.fuse1x1) {
    // Phase forms (ConvArgs::uph): rows and columns folded (4 of the 9 taps' work per output
    // pixel), or rows only (6 of 9) where the column form does not apply.
    for (int u = cw.wpc ? 2 : 1; u >= 1; --u) {
      ConvArgs q = a;
      q.w = u == 2 ? cw.wpc : cw.wph; q.K = (u == 2 ? 16 : 12) * cw.cin; q.uph = u;
      if (conv_uph_ok(q, (int)sizeof(T))) {
        a.w = q.w; a.K = q.K; a.uph = u;
        fl = 2.0 * M * cw.cout * (u == 2 ? 4 : 6) * cw.cin_real;
        break;
      }
    }
  }
  const bool use8 = sizeof(T) == 2 && cw.w8 && conv8_ok(a, cw.kh, cw.kw, stride, pad);
  // Per-image split-K at the small levels (g_splitk, UNetNet::forward): 3x3 convs over ks Cin
  // ranges; the count depends on one image's shape and the handle's policy, never on B.
  int ks3 = 0;
  if (g_splitk > 1 && cw.kh == 3 && cw.kw == 3 && stride == 1 && pad == 1 && !up && !use8 && !a.uph &&
      (long)a.Ho * a.Wo <= splitk_px() && a.Ho > 1) {
    ConvArgs q = a;
    q.w2 = nullptr; q.bias2 = nullptr; q.y2 = nullptr; q.w2_dual = 0; q.ldy2 = 0;
    ks3 = conv3_split_k(q, (int)sizeof(T), g_splitk);
  }
  bool fused = false;
  if (e.fuse1x1) {
    fused = sizeof(T) == 2 && !use8 && !ks3 && a.w2 && cw.kh == 3 && stride == 1 && pad == 1 && !up &&
            e.fuse1x1->cout == cw.cout && e.fuse1x1->cin == cw.cin && conv_res_fusable(a);
    if (!fused) {
      a.w2 = nullptr; a.bias2 = nullptr; a.y2 = nullptr; a.w2_dual = 0; a.ldy2 = 0;
      // Not fusable here: the 1x1 conv runs as its own launch (it only reads the same input).
      conv_call<T>(r, *e.fuse1x1, x1, ld1, C1, x2, ld2, B, Hs, Ws, 0, 1, 0, e.y2, e.ldy2, Epi());
    } else {
      fl += 2.0 * M * cw.cout * e.fuse1x1->cin_real;
    }
  }
  if (ks3 > 1) {
    a.ksplit = ks3;
    a.part = r.alloc<float>((size_t)ks3 * (size_t)M * cw.cout);
  }
  // Split-K (the small-M 1x1 GEMMs: ViT / text tower linears, and the UNet's small levels under
  // g_splitk): fp32 partials from the arena; the count follows one image's rows.
  const long srows = e.split_rows > 0 ? e.split_rows
                     : (splitk32_1x1() && g_splitk > 1 && a.Ho > 1 && a.Wo > 1 && (long)a.Ho * a.Wo <= 1024) ? (long)a.Ho * a.Wo : 0;
  if (srows > 0 && cw.kh == 1 && cw.kw == 1 && stride == 1 && pad == 0 && !use8 && !e.fuse1x1) {
    const int ks = conv_split_k(a, (int)sizeof(T), srows);
    if (ks > 1) {
      a.ksplit = ks;
      a.part = r.alloc<float>((size_t)ks * (size_t)M * cw.cout);
    }
  }
  r.flops += fl;
  // Class 340: the fp8 ResBlock block2 (conv3q); an fp8-output block1 keeps its kernel's class.
  // Class 326: the row-phase upsample conv on v4 tiles (kept out of class 312's roofline).
  const int cls = cw.kh * 100 + (a.xs8 ? 40 : use8 ? 30 : a.uph ? 26 : conv_variant(a, cw.kh, (int)sizeof(T)));
  // Algorithmic HBM bytes: every operand touched once (input, weights, output, residuals).
  // (e4m3 tensors: 1 byte per value + 2 exponent bytes per pixel; e4m3 weights 1 byte.)
  const double es = sizeof(T), ei = a.xs8 ? 1 + 2.0 / 64 : es, eo = a.ys8 ? 1 + 2.0 / 64 : es;
  const double bytes = ei * B * Hs * Ws * cw.cin_real + (a.xs8 ? 1 : es) * cw.cout * cw.kh * cw.kw * cw.cin +
                       M * cw.cout * (eo + es * ((e.res1 ? 1 : 0) + (e.res2 ? 1 : 0) + (fused ? 1 : 0)));
  auto label = [&] {
    char lab[160];
    snprintf(lab, sizeof lab, "c%d %3dx%-3d%s B%d s%d %4d->%-4d%s%s%s%s%s", cls, Hs, Ws, up ? "^" : " ", B,
             stride, cw.cin_real, cw.cout, e.res1 ? " +r" : "", e.res2 ? " +r2" : "",
             e.ss ? " ss" : "", e.w_bstride ? " perimg" : "", fused ? " +1x1" : "");
    return std::string(lab);
  };
  timed(r, cls, fl, bytes, label, [&](unsigned long long* stamp) {
    if (!cw.w) throw Error(DAC_E_STATE, "conv weight not loaded");
    if (a.lnf_cs && !conv_lnf_ok(a, (int)sizeof(T))) throw Error(DAC_E_STATE, "conv: LN fold requested on a shape without a folding kernel");
    if (a.gna_stats && !conv_gna_ok(a, (int)sizeof(T))) throw Error(DAC_E_STATE, "conv: GroupNorm A path requested on a shape without such a kernel");
    if (a.ys8 && !conv_q8out_ok(a)) throw Error(DAC_E_STATE, "conv: fp8 output requested on a shape without such a kernel");
    if (a.xs8 && !(sizeof(T) == 2 && cw.q8w && conv3q_ok(a))) throw Error(DAC_E_STATE, "conv: fp8 input on a layer without fp8 weights / kernel");
    if (a.Cin % (16 / (int)sizeof(T)) || (a.x2 == nullptr && a.C1 < a.Cin))
      throw Error(DAC_E_ARG, "conv: bad channel layout");
    a.stamp = stamp;
    if (a.xs8) {
      if constexpr (sizeof(T) == 2) conv3q<T>(a, cw.q8w, cw.q8s, r.st);
    } else if (use8) {
      if constexpr (sizeof(T) == 2) conv8<T>(a, cw.kh, cw.kw, stride, pad, cw.w8, cw.ws8, cw.kp8, r.st);
    } else {
      conv<T>(a, cw.kh, cw.kw, stride, pad, r.st);
      if (dup1x1() && cw.kh == 1 && a.Ho * a.Wo <= 1024 && a.Ho * a.Wo >= 256 && a.ksplit <= 1) conv<T>(a, cw.kh, cw.kw, stride, pad, r.st);
    }
    emu_round<T>(r, y, ldy, (size_t)M, cw.cout);
    if (fused) emu_round<T>(r, e.y2, e.ldy2, (size_t)M, cw.cout);
  });
}

template <typename T>
static void emu_round(const Run& r, void* y, int ld, size_t rows, int C) {
  if (sizeof(T) == 4 && !r.dry && (emu_a() & g_role))
    round_bf16_rows(reinterpret_cast<float*>(y), ld, rows, C, r.st);
}

template <typename T>
static void ln(Run& r, const void* x, int ldx, void* y, int ldy, const void* res, int ldr,
               const float* g, const float* b, int rows, int C, float eps) {
  if (r.dry) return;
  layernorm<T>(x, ldx, y, ldy, res, ldr, g, b, rows, C, eps, r.st);
  emu_round<T>(r, y, ldy, (size_t)rows, C);
}

// ============================================================================= schedule
TileGrid check_tile_grid(int B, int H, int W, int th, int tw, int overlap, const int32_t* ys, int ny,
                         const int32_t* xs, int nx) {
  auto bad = [](const std::string& m) { throw Error(DAC_E_ARG, "tile grid: " + m); };
  if (B < 1 || H < 2 || W < 2) bad("needs B >= 1 and an image of at least 2 x 2");
  if (!ys || !xs || ny < 1 || nx < 1) bad("null or empty offset list");
  if (th < 2 || tw < 2) bad("tile sides must be >= 2");
  if (th > H || tw > W) bad("tile larger than the image (clamp it to the image size)");
  if (overlap < 0 || overlap >= std::min(th, tw)) bad("overlap must be in [0, min(th, tw))");
  auto axis = [&](const int32_t* o, int n, int l, int L, const char* name) {
    for (int i = 0; i < n; ++i) {
      if (o[i] < 0 || o[i] > L - l) bad(std::string(name) + " offset out of bounds");
      if (i && o[i] <= o[i - 1]) bad(std::string(name) + " offsets must ascend");
      if (i && o[i] > o[i - 1] + l) bad(std::string(name) + " axis has a gap between tiles");
    }
    if (o[0] != 0 || o[n - 1] != L - l) bad(std::string(name) + " axis is not covered to its ends");
  };
  axis(ys, ny, th, H, "row");
  axis(xs, nx, tw, W, "column");
  if ((long long)B * ny * nx > (1 << 20) || (long long)B * H * W > INT32_MAX / 4)
    bad("too many tiles or pixels for one call");
  TileGrid g;
  g.th = th; g.tw = tw; g.ov = overlap;
  g.ys.assign(ys, ys + ny);
  g.xs.assign(xs, xs + nx);
  return g;
}

void compute_schedule(SdeSchedule& s, float max_sigma, int T, int schedule, float eps) {
  // sde_utils.py:84-154 in fp32 (torch 0-dim / 1-D float32 semantics).
  const double ms = max_sigma >= 1 ? max_sigma / 255.0 : max_sigma;
  s.T = T;
  s.max_sigma = (float)ms;
  const int n = T + 1;
  s.thetas.assign(n, 0.f);
  if (schedule == DAC_COSINE) {
    const int ts = T + 2;
    std::vector<float> ac(ts + 1);
    const float c1 = (float)0.008, c2 = (float)(1 + 0.008), c3 = (float)(M_PI * 0.5);
    for (int i = 0; i <= ts; ++i) {
      const float x = (float)i;
      const float c = std::cos(((x / (float)ts) + c1) / c2 * c3);
      ac[i] = c * c;
    }
    const float a0 = ac[0];
    for (int i = 0; i <= ts; ++i) ac[i] = ac[i] / a0;
    for (int i = 0; i < n; ++i) s.thetas[i] = 1.f - ac[i + 1];
  } else if (schedule == DAC_LINEAR) {
    const double scale = 1000.0 / n;
    const float b0 = (float)(scale * 0.0001), b1 = (float)(scale * 0.02);
    for (int i = 0; i < n; ++i)
      s.thetas[i] = n == 1 ? b0 : b0 + (b1 - b0) * (float)i / (float)(n - 1);
  } else {
    for (int i = 0; i < n; ++i) s.thetas[i] = 1.f;
  }
  s.sigmas.resize(n);
  s.tcum.resize(n);
  s.sbar.resize(n);
  const float ms2x2 = (float)(ms * ms * 2), ms2 = (float)(ms * ms);
  float acc = 0.f;
  for (int i = 0; i < n; ++i) {
    s.sigmas[i] = std::sqrt(ms2x2 * s.thetas[i]);
    acc += s.thetas[i];
    s.tcum[i] = acc - s.thetas[0];
  }
  s.dt = (-1.f / s.tcum[n - 1]) * (float)std::log((double)eps);
  for (int i = 0; i < n; ++i) s.sbar[i] = std::sqrt(ms2 * (1.f - std::exp(-2.f * s.tcum[i] * s.dt)));
}

StepCoef SdeSchedule::coef(int t, int mode) const {
  (void)mode;
  StepCoef c{};
  const float th = thetas[t], tc = tcum[t], tc1 = tcum[t - 1];
  c.sbar = sbar[t];
  c.ea = std::exp(tc * dt);                                  // sde_utils.py:246
  const float A = std::exp(-th * dt), B = std::exp(-tc * dt), C = std::exp(-tc1 * dt);
  c.t1 = A * (1.f - C * C) / (1.f - B * B);                  // :210
  c.t2 = C * (1.f - A * A) / (1.f - B * B);                  // :211
  const float A2 = std::exp(-2.f * th * dt), B2 = std::exp(-2.f * tc * dt),
              C2 = std::exp(-2.f * tc1 * dt);
  const float var = (1.f - A2) * (1.f - C2) / (1.f - B2);    // :220
  const float lv = std::log(std::max(var, 1e-20f * dt));     // :223-224
  c.std = std::exp(0.5f * lv) * max_sigma;                   // :225
  c.theta = th;
  c.sigma2 = sigmas[t] * sigmas[t];
  c.dt = dt;
  c.sigma_sqrt_dt = sigmas[t] * (float)std::sqrt((double)dt);
  return c;
}

// ============================================================================= UNet
template <typename T>
struct UNetNet {
  struct RB { ConvW c1, c2, res; bool has_res = false; int din = 0, dout = 0;
              const float* mw = nullptr; const float* mb = nullptr; int ss_off = 0; };
  struct LA { const float* gpre = nullptr; ConvW qkv; const float* wout = nullptr;
              const float* bout = nullptr; const float* gout = nullptr;
              ConvW qkv_f; const float* qkv_cs = nullptr;     // PreNorm folded into to_qkv (C = 256)
              const void* wqkv_g = nullptr;   // fused kernels: to_qkv diag(g) (the PreNorm gain)
              float qshift = 0.f; };          // bound on |q| for la_apply's softmax (0: per-pixel max)
  struct ST { const float* gpre = nullptr; const float *gnw = nullptr, *gnb = nullptr;
              ConvW pin; const float *n1w = nullptr, *n1b = nullptr, *n3w = nullptr, *n3b = nullptr;
              ConvW qkv, o, ff1, ff2, pout; const float *a2v = nullptr, *a2o = nullptr, *a2ob = nullptr;
              // attn2 without a context is self-attention over norm2(x) (attention.py:174);
              // it needs context_dim == C, as in the reference (to_k / to_v take C inputs).
              bool self_ok = false; ConvW qkv2, o2; const float *n2w = nullptr, *n2b = nullptr;
              int cc_off = 0;
              // norm1 folded into q|k|v (16-bit handles, not fp8).
              ConvW qkv_f; const float* qkv_cs = nullptr;
              bool q_pre = false; };   // q rows of qkv / qkv_f prescaled (see load_attn)
  struct Attn { bool st = false; LA la; ST s; };
  struct Level { RB b1, b2; Attn at; ConvW samp; };

  dac_config cfg;
  int nf, depth, tdim, ctx;
  bool degra, imgctx;
  std::vector<std::pair<int, int>> levels;
  ConvW init_conv, final_conv;
  const float *tm1w, *tm1b, *tm3w, *tm3b, *prompt = nullptr, *t0w = nullptr, *t0b = nullptr,
              *t2w = nullptr, *t2b = nullptr, *pmw = nullptr, *pmb = nullptr;
  std::vector<Level> downs, ups;
  ConvW half_down, half_up;            // Wild-IR scale 0.5 wrap (downsample / upsample.1)
  bool half = false;
  int st_from = 3;
  RB mid1, mid2, fin;
  Attn mid_attn;
  int ss_total = 0, cc_total = 0, n_st = 0;

  explicit UNetNet(const dac_config& c) : cfg(c) {
    nf = c.nf; depth = c.depth; tdim = nf * 4; ctx = c.context_dim;
    degra = ctx > 0 && c.use_degra_context;
    imgctx = ctx > 0 && c.use_image_context;
    half = c.unet_scale_half != 0;
    st_from = c.unet_st_from > 0 ? c.unet_st_from : 3;
    std::vector<int> m = {1};
    for (int i = 0; i < depth; ++i) m.push_back(c.ch_mult[i]);
    for (int i = 0; i < depth; ++i) levels.push_back({nf * m[i], nf * m[i + 1]});
  }

  RB load_rb(Packer<T>& P, const std::string& p, int din, int dout, bool dual_res = false) {
    RB rb;
    rb.din = din; rb.dout = dout;
    rb.mw = P.f32(p + "mlp.1.weight", {2 * dout, tdim});
    rb.mb = P.f32(p + "mlp.1.bias", {2 * dout});
    rb.c1 = P.conv(p + "block1.proj.weight", dout, din, 3, 3);
    std::vector<float> p2;
    rb.c2 = P.conv(p + "block2.proj.weight", dout, dout, 3, 3, "", false, 0, P.q8 ? &p2 : nullptr);
    if (P.q8 && dout == 64) P.make_q8c3(rb.c2, p2);
    if (din != dout) {
      rb.has_res = true;
      rb.res = dual_res ? P.conv_dual(p + "res_conv.weight", dout, din, 1, 1)
                        : P.conv(p + "res_conv.weight", dout, din, 1, 1);
    }
    rb.ss_off = ss_total;
    ss_total += 2 * dout;
    return rb;
  }
  Attn load_attn(Packer<T>& P, const std::string& p, int C, bool st) {
    Attn a;
    a.st = st;
    const std::string f = p + "fn.fn.";
    if (!st) {
      a.la.gpre = P.f32(p + "fn.norm.g", {1, C, 1, 1});
      std::vector<float> pq;
      a.la.qkv = P.conv(f + "to_qkv.weight", 384, C, 1, 1, "", false, 0, &pq);
      if (sizeof(T) == 2 && !P.fp8 && fold_on(4) && C != 64 && C != 128) {
        // The unfused LinearAttention path (C = 256): its channel LayerNorm (gain only) is
        // folded into to_qkv like the SpatialTransformer's norm1.
        auto fq = P.fold_ln(a.la.qkv, pq, 384, C, p + "fn.norm.g", "", nullptr, {1, C, 1, 1});
        if (fq.cs) { a.la.qkv_f = fq.cw; a.la.qkv_cs = fq.cs; }
      }
      if (const HostW* g = P.ws.get(p + "fn.norm.g", {1, C, 1, 1}); g && pq.size() == (size_t)384 * C) {
        // The fused kernels take the PreNorm gain inside to_qkv, and la_apply its softmax shift
        // from the bound on the 128 q rows (fold_la_gain).
        const LaFold lf = fold_la_gain(pq, 384, C, 128, g->v.data(), P.kn.la_qshift);
        a.la.wqkv_g = P.upload_T(lf.wg, f + "to_qkv.weight", 1, C);
        a.la.qshift = lf.qshift;
      }
      a.la.wout = P.f32(f + "to_out.0.weight", {C, 128, 1, 1});
      a.la.bout = P.f32(f + "to_out.0.bias", {C});
      a.la.gout = P.f32(f + "to_out.1.g", {1, C, 1, 1});
      return a;
    }
    ST& s = a.s;
    s.gpre = P.f32(p + "fn.norm.g", {1, C, 1, 1});
    s.gnw = P.f32(f + "norm.weight", {C});
    s.gnb = P.f32(f + "norm.bias", {C});
    s.pin = P.conv(f + "proj_in.weight", C, C, 1, 1, f + "proj_in.bias");
    const std::string b = f + "transformer_blocks.0.";
    std::vector<float> pq;
    // 16-bit handles: q comes out of its GEMM already times 32^-0.5 * log2(e) (one rounding, as
    // for q itself), so the attention kernel's scores are in log2 units (flash_kv PRE).
    s.q_pre = sizeof(T) == 2;
    s.qkv = P.concat({b + "attn1.to_q.weight", b + "attn1.to_k.weight", b + "attn1.to_v.weight"}, C, C, &pq,
                     s.q_pre ? (float)(1.4426950408889634 / std::sqrt(32.0)) : 1.f);
    s.o = P.linear(b + "attn1.to_out.0.weight", C, C, b + "attn1.to_out.0.bias");
    s.ff1 = P.geglu(b + "ff.net.0.proj.weight", b + "ff.net.0.proj.bias", 4 * C, C);
    if (sizeof(T) == 2 && !P.fp8 && fold_on(1)) {
      auto fq = P.fold_ln(s.qkv, pq, 3 * C, C, b + "norm1.weight", b + "norm1.bias", nullptr);
      if (fq.cs) { s.qkv_f = fq.cw; s.qkv_cs = fq.cs; }
    }
    s.ff2 = P.linear(b + "ff.net.2.weight", C, 4 * C, b + "ff.net.2.bias");
    // attn2 attends to ONE context token: softmax over a single key is exactly 1, so its
    // output is to_out(to_v(ctx)) for every query; to_q / to_k / norm2 cannot affect it
    // (attention.py:170-193 with context [B,1,ctx]). They are still required keys.
    (void)P.f32(b + "attn2.to_q.weight", {C, C});
    (void)P.f32(b + "attn2.to_k.weight", {C, ctx});
    s.a2v = P.f32(b + "attn2.to_v.weight", {C, ctx});
    s.a2o = P.f32(b + "attn2.to_out.0.weight", {C, C});
    s.a2ob = P.f32(b + "attn2.to_out.0.bias", {C});
    s.n1w = P.f32(b + "norm1.weight", {C});
    s.n1b = P.f32(b + "norm1.bias", {C});
    s.n2w = P.f32(b + "norm2.weight", {C});
    s.n2b = P.f32(b + "norm2.bias", {C});
    if (ctx == C) {              // image_context=None falls back to self-attention
      s.self_ok = true;
      s.qkv2 = P.concat({b + "attn2.to_q.weight", b + "attn2.to_k.weight", b + "attn2.to_v.weight"}, C, C);
      s.o2 = P.linear(b + "attn2.to_out.0.weight", C, C, b + "attn2.to_out.0.bias");
    }
    s.n3w = P.f32(b + "norm3.weight", {C});
    s.n3b = P.f32(b + "norm3.bias", {C});
    s.pout = P.conv(f + "proj_out.weight", C, C, 1, 1, f + "proj_out.bias");
    s.cc_off = cc_total;
    cc_total += C;
    n_st++;
    return a;
  }

  // Split-precision (hi | lo) edge weights: bf16 handles (and fp8, whose activations are bf16),
  // and f16 handles under f16_edges().
  static bool split_edges_f() { return std::is_same<T, bf16>::value || (sizeof(T) == 2 && f16_edges()); }
  void load(Packer<T>& P) {
    ss_total = cc_total = n_st = 0;
    if (degra) prompt = P.f32("prompt", {1, tdim});
    // bf16: [xt | mu] has 6 (-> 8) channels = one 16-byte vector per pixel, so a K tile of 64
    // elements is 8 neighbouring pixels of one input row (kernel row padded to 8 taps).
    // init_conv, final_conv and final_res_block.res_conv keep split-precision weights in bf16
    // handles: their bf16 rounding error alone moved the T=100 restore by up to ~1e-3 dB
    // (measured with the DAC_EMU_* probe); together they are ~1.4 % of the FLOPs.
    // f16 handles keep plain weights there: f16's own weight rounding (2^-12 relative) is that of
    // the activations it produces, and the split doubles the init conv's MFMAs.
    const int kwp7 = sizeof(T) == 2 && Packer<T>::pad_to(cfg.in_nc * 2, 8) == 8 ? 8 : 0;
    const bool split_edges = split_edges_f();
    init_conv = split_edges ? P.conv_dual("init_conv.weight", nf, cfg.in_nc * 2, 7, 7, "", kwp7)
                            : P.conv("init_conv.weight", nf, cfg.in_nc * 2, 7, 7, "", false, kwp7);
    if (half) {
      half_down = P.conv("downsample.weight", nf, nf, 4, 4, "downsample.bias");
      std::vector<float> pk;
      half_up = P.conv("upsample.1.weight", nf, nf, 3, 3, "upsample.1.bias", false, 0, &pk);
      P.make_uph(half_up, pk, "upsample.1.weight");
    }
    tm1w = P.f32("time_mlp.1.weight", {tdim, nf});
    tm1b = P.f32("time_mlp.1.bias", {tdim});
    tm3w = P.f32("time_mlp.3.weight", {tdim, tdim});
    tm3b = P.f32("time_mlp.3.bias", {tdim});
    if (degra) {
      t0w = P.f32("text_mlp.0.weight", {tdim, ctx});
      t0b = P.f32("text_mlp.0.bias", {tdim});
      t2w = P.f32("text_mlp.2.weight", {tdim, tdim});
      t2b = P.f32("text_mlp.2.bias", {tdim});
      pmw = P.f32("prompt_mlp.weight", {tdim, tdim});
      pmb = P.f32("prompt_mlp.bias", {tdim});
    }
    downs.assign(depth, Level());
    ups.assign(depth, Level());
    for (int i = 0; i < depth; ++i) {
      const auto [din, dout] = levels[i];
      const std::string p = "downs." + std::to_string(i) + ".";
      Level& L = downs[i];
      L.b1 = load_rb(P, p + "0.", din, din);
      L.b2 = load_rb(P, p + "1.", din, din);
      L.at = load_attn(P, p + "2.", din, imgctx && i >= st_from);
      L.samp = i != depth - 1 ? P.conv(p + "3.weight", dout, din, 4, 4, p + "3.bias")
                              : P.conv(p + "3.weight", dout, din, 3, 3);
    }
    for (int j = 0; j < depth; ++j) {
      const int i = depth - 1 - j;
      const auto [din, dout] = levels[i];
      const std::string p = "ups." + std::to_string(j) + ".";
      Level& L = ups[j];
      L.b1 = load_rb(P, p + "0.", dout + din, dout);
      L.b2 = load_rb(P, p + "1.", dout + din, dout);
      L.at = load_attn(P, p + "2.", dout, imgctx && i >= st_from);
      if (i != 0) {                                  // Upsample: nearest 2x, then this 3x3
        std::vector<float> pk;
        L.samp = P.conv(p + "3.1.weight", din, dout, 3, 3, p + "3.1.bias", false, 0, &pk);
        P.make_uph(L.samp, pk, p + "3.1.weight");
      } else {
        L.samp = P.conv(p + "3.weight", din, dout, 3, 3);
      }
    }
    const int mid = levels.back().second;
    mid1 = load_rb(P, "mid_block1.", mid, mid);
    mid_attn = load_attn(P, "mid_attn.", mid, imgctx);
    mid2 = load_rb(P, "mid_block2.", mid, mid);
    fin = load_rb(P, "final_res_block.", 2 * nf, nf, /*dual_res=*/split_edges);
    final_conv = P.conv_dual("final_conv.weight", cfg.out_nc, nf, 3, 3, "final_conv.bias");
    // Every ResBlock's time MLP (SiLU, Linear(tdim, 2 dout)) reads the same embedding, so the
    // per-call tables take them as ONE small_linear over the weights concatenated in ss_off
    // order (each output is the same per-output dot product as a separate call's).
    mw_all = mb_all = nullptr;
    std::vector<const RB*> rbs;
    for (auto& L : downs) { rbs.push_back(&L.b1); rbs.push_back(&L.b2); }
    for (auto& L : ups) { rbs.push_back(&L.b1); rbs.push_back(&L.b2); }
    rbs.push_back(&mid1); rbs.push_back(&mid2); rbs.push_back(&fin);
    bool all = ss_total > 0;
    for (const RB* rb : rbs) all = all && rb->mw && rb->mb;
    if (all) {
      float* W = (float*)P.pool.alloc((size_t)ss_total * tdim * 4);
      float* bb = (float*)P.pool.alloc((size_t)ss_total * 4);
      for (const RB* rb : rbs) {
        HIP_OK(hipMemcpy(W + (size_t)rb->ss_off * tdim, rb->mw, (size_t)2 * rb->dout * tdim * 4, hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(bb + rb->ss_off, rb->mb, (size_t)2 * rb->dout * 4, hipMemcpyDeviceToDevice));
      }
      mw_all = W;
      mb_all = bb;
    }
  }
  const float* mw_all = nullptr;       // [ss_total][tdim]: all ResBlock time-MLP weights
  const float* mb_all = nullptr;

  // ----------------------------------------------------------------- per-call tables
  // ss_all[(i*B + b)*ss_total + off ...]: ResBlock (scale, shift) for step i, image b, whose
  // time is t0 + dt * i. sin_tab: [nT*B][nf] device scratch for the sinusoidal embeddings.
  // Step i's time is (t0 + dt * i) * scale (IRSDE.sample_scale); tc / icx may be null (no
  // prompt embedding / no cross-attention constants, DenoisingUNet_arch.py:133-140).
  void tables(Run& r, float* sin_tab, int nT, double t0, double dt, double scale, const float* tc,
              const float* icx, int B, float* ss_all, float* cc) {
    const int R = nT * B;
    if (!r.dry) sinus_embedding(sin_tab, R, B, nf, t0, dt, scale, r.st);
    float* h1 = r.alloc<float>((size_t)R * tdim);
    float* temb = r.alloc<float>((size_t)R * tdim);
    float* pe = nullptr;
    if (degra && tc) {
      float* p0 = r.alloc<float>((size_t)B * tdim);
      float* p1 = r.alloc<float>((size_t)B * tdim);
      float* p2 = r.alloc<float>((size_t)B * tdim);
      pe = r.alloc<float>((size_t)B * tdim);
      if (!r.dry) {
        small_linear(tc, ctx, t0w, t0b, p0, tdim, B, ctx, tdim, ACT_NONE, ACT_SILU, nullptr, 0, 1, r.st);
        small_linear(p0, tdim, t2w, t2b, p1, tdim, B, tdim, tdim, ACT_NONE, ACT_NONE, nullptr, 0, 1, r.st);
        softmax_mul(p1, prompt, p2, B, tdim, r.st);
        small_linear(p2, tdim, pmw, pmb, pe, tdim, B, tdim, tdim, ACT_NONE, ACT_NONE, nullptr, 0, 1, r.st);
      }
    }
    if (!r.dry) {
      small_linear(sin_tab, nf, tm1w, tm1b, h1, tdim, R, nf, tdim, ACT_NONE, ACT_GELU, nullptr, 0, 1, r.st);
      small_linear(h1, tdim, tm3w, tm3b, temb, tdim, R, tdim, tdim, ACT_NONE, ACT_NONE, pe, tdim, B, r.st);
    }
    auto rbt = [&](const RB& rb) {
      if (!r.dry)
        small_linear(temb, tdim, rb.mw, rb.mb, ss_all + rb.ss_off, ss_total, R, tdim,
                     2 * rb.dout, ACT_SILU, ACT_NONE, nullptr, 0, 1, r.st);
    };
    if (mw_all) {
      if (!r.dry)
        small_linear(temb, tdim, mw_all, mb_all, ss_all, ss_total, R, tdim, ss_total, ACT_SILU, ACT_NONE, nullptr, 0, 1,
                     r.st);
    } else {
      for (auto& L : downs) { rbt(L.b1); rbt(L.b2); }
      for (auto& L : ups) { rbt(L.b1); rbt(L.b2); }
      rbt(mid1); rbt(mid2); rbt(fin);
    }
    auto stc = [&](const Attn& a) {
      if (!a.st) return;
      const int C = a.s.pin.cout;
      float* v = r.alloc<float>((size_t)B * C);
      if (!r.dry) {
        small_linear(icx, ctx, a.s.a2v, nullptr, v, C, B, ctx, C, ACT_NONE, ACT_NONE, nullptr, 0, 1, r.st);
        small_linear(v, C, a.s.a2o, a.s.a2ob, cc + a.s.cc_off, cc_total, B, C, C, ACT_NONE,
                     ACT_NONE, nullptr, 0, 1, r.st);
      }
    };
    if (!icx) return;
    for (auto& L : downs) stc(L.at);
    stc(mid_attn);
    for (auto& L : ups) stc(L.at);
  }

  // ----------------------------------------------------------------- blocks
  const void* resblock(Run& r, const RB& rb, const void* xa, int Ca, const void* xb, int Cb,
                       int B, int H, int W, const float* ss) {
    const size_t M = (size_t)B * H * W;
    if constexpr (sizeof(T) == 2) {
      // The whole ResBlock as one launch (rbfuse.hip) where it applies: h and the res_conv output
      // stay in LDS. (fp8 handles keep their e4m3 pair below.)
      const bool q8pair = rb.c2.q8w && q8_on();
      RbArgs ra{};
      ra.x1 = xa; ra.ld1 = Ca; ra.C1 = Ca; ra.x2 = xb; ra.ld2 = Cb; ra.Cin = rb.c1.cin;
      ra.B = B; ra.H = H; ra.W = W; ra.w1 = rb.c1.w; ra.w2 = rb.c2.w;
      ra.wr = rb.has_res ? rb.res.w : nullptr; ra.ss = ss + rb.ss_off; ra.ss_ld = ss_total; ra.ldy = rb.dout;
      const bool shapes = !q8pair && rb.dout == 64 && rb.c2.cin == 64 && rb.c1.kh == 3 && rb.c2.kh == 3 &&
                          !rb.c1.dual && !rb.c2.dual && !rb.c1.kwp && !rb.c2.kwp && rb.c1.cin_real == Ca + Cb &&
                          (!rb.has_res || (!rb.res.dual && !rb.res.b && rb.res.cin == rb.c1.cin)) &&
                          !rb.c1.b && !rb.c2.b && rb.ss_off % 4 == 0 && ss_total % 4 == 0 && !no_res_fuse();
      if (shapes && rbfuse_ok(ra) && rbfuse_pays(ra)) {
        T* o = r.alloc<T>(M * rb.dout);
        ra.y = o;
        const double fl = 2.0 * M * 64 * 9 * (rb.c1.cin_real + 64) + (rb.has_res ? 2.0 * M * 64 * rb.c1.cin_real : 0.0);
        r.flops += fl;
        auto label = [&] {
          char lab[160];
          snprintf(lab, sizeof lab, "c350 %3dx%-3d  B%d ResBlock %4d->%-4d fused", H, W, B, rb.c1.cin_real, rb.dout);
          return std::string(lab);
        };
        // Algorithmic HBM bytes: x in, y out.
        timed(r, 350, fl, sizeof(T) * (double)M * (rb.c1.cin_real + rb.dout), label, [&](unsigned long long* stamp) {
          if (!rb.c1.w || !rb.c2.w || (rb.has_res && !rb.res.w)) throw Error(DAC_E_STATE, "conv weight not loaded");
          ra.stamp = stamp;
          rbfuse<T>(ra, r.st);
        });
        return o;
      }
    }
    T* h1 = r.alloc<T>(M * rb.dout);
    Epi e1;
    e1.ss = ss + rb.ss_off; e1.ss_ld = ss_total; e1.act = ACT_SILU;
    const void* res = xa;
    int ldr = Ca;
    T* rr = rb.has_res ? r.alloc<T>(M * rb.dout) : nullptr;
    if (rb.has_res && !no_res_fuse()) {
      // res_conv rides along in block1's conv kernel (same input; conv_call falls back to a
      // separate launch when the kernel cannot take it).
      e1.fuse1x1 = &rb.res; e1.y2 = rr; e1.ldy2 = rb.dout;
    }
    if (rb.c2.q8w && q8_on()) {
      // fp8 handles: h = block1's output lives only as block2's input, so block1's epilogue
      // writes it as e4m3 + per-(pixel, 32-channel) exponents and block2 runs on the block-scaled
      // MFMA (conv3q.hip). Shapes without both kernels keep the 16-bit pair.
      ConvArgs q = conv_args(r, rb.c1, xa, Ca, Ca, xb, Cb, B, H, W, 0, 1, 1, h1, 64, e1);
      ConvArgs q2 = q;
      q2.x1 = h1; q2.x2 = nullptr; q2.xs8 = reinterpret_cast<const uint8_t*>(&q); q2.ld1 = q2.C1 = q2.Cin = 64;
      q2.K = 576; q2.ss = nullptr; q2.res1 = res; q2.ldr1 = rb.has_res ? rb.dout : Ca; q2.y2 = nullptr; q2.w2 = nullptr;
      q2.ys8 = nullptr;
      if (conv_q8out_ok(q) && conv3q_ok(q2)) {
        uint8_t* h8 = r.alloc<uint8_t>(M * 64);
        uint8_t* hs = r.alloc<uint8_t>(M * 2);
        e1.ys8 = hs;
        conv_call<T>(r, rb.c1, xa, Ca, Ca, xb, Cb, B, H, W, 0, 1, 1, h8, 64, e1);
        if (rb.has_res) {
          if (no_res_fuse()) conv_call<T>(r, rb.res, xa, Ca, Ca, xb, Cb, B, H, W, 0, 1, 0, rr, rb.dout, Epi());
          res = rr;
          ldr = rb.dout;
        }
        T* o = r.alloc<T>(M * rb.dout);
        Epi e2;
        e2.act = ACT_SILU; e2.res1 = res; e2.ldr1 = ldr; e2.xs8 = hs;
        conv_call<T>(r, rb.c2, h8, 64, 64, nullptr, 0, B, H, W, 0, 1, 1, o, rb.dout, e2);
        return o;
      }
    }
    conv_call<T>(r, rb.c1, xa, Ca, Ca, xb, Cb, B, H, W, 0, 1, 1, h1, rb.dout, e1);
    if (rb.has_res) {
      if (no_res_fuse()) conv_call<T>(r, rb.res, xa, Ca, Ca, xb, Cb, B, H, W, 0, 1, 0, rr, rb.dout, Epi());
      res = rr;
      ldr = rb.dout;
    }
    T* o = r.alloc<T>(M * rb.dout);
    Epi e2;
    e2.act = ACT_SILU; e2.res1 = res; e2.ldr1 = ldr;
    conv_call<T>(r, rb.c2, h1, rb.dout, rb.dout, nullptr, 0, B, H, W, 0, 1, 1, o, rb.dout, e2);
    return o;
  }

  // Runs fn(run, first image, images) for nbr contiguous parts of the batch as concurrent
  // branches: part 0 on r.st, part k on r.side[k - 1], forked from and joined back into r.st
  // (recorded into the graph when r.st is capturing).
  template <class F> void branches(Run& r, int B, int nbr, F&& fn) {
    if (r.in_branch) throw Error(DAC_E_STATE, "nested branch fork");
    if (!r.dry) {
      HIP_OK(hipEventRecord(r.evf, r.st));
      for (int k = 0; k + 1 < nbr; ++k) HIP_OK(hipStreamWaitEvent(r.side[k], r.evf, 0));
    }
    // Every side stream is joined back into r.st on every exit, also when a branch throws
    // (HIP error, arena overflow, missing weight): a capture left with a forked stream could
    // not be ended, and the side streams would stay in capture mode for later calls.
    auto join = [&]() {
      if (r.dry) return;
      for (int k = 0; k + 1 < nbr; ++k) {
        HIP_OK(hipEventRecord(r.evj[k], r.side[k]));
        HIP_OK(hipStreamWaitEvent(r.st, r.evj[k], 0));
      }
    };
    double fl = 0;
    try {
      for (int k = 0; k < nbr; ++k) {
        const int b0 = (int)((long)B * k / nbr), b1 = (int)((long)B * (k + 1) / nbr);
        Run rk = r;
        rk.st = k ? r.side[k - 1] : r.st;
        rk.flops = 0;
        rk.in_branch = true;
        fn(rk, b0, b1 - b0);
        fl += rk.flops;
      }
    } catch (...) {
      try { join(); } catch (...) {}             // the branch's error is the one reported
      throw;
    }
    r.flops += fl;
    join();
  }
  bool la_fused(const LA& la, int C) const {
    // C = 256 (the 64x64 level) takes the fused pair too on 16-bit handles (la256_on()).
    return la.wqkv_g && (C == 64 || C == 128 || (C == 256 && sizeof(T) == 2 && la256_on()));
  }
  // Fused (linattn.hip): context pass over x, then one apply pass x -> y (LN, q projection and
  // softmax, per-image to_out, its LayerNorm and the Residual).
  void linattn_fused(Run& r, const LA& la, const void* x, int C, int B, int H, int W, T* y) {
    const size_t M = (size_t)B * H * W;
    T* weff = r.alloc<T>((size_t)B * C * 128);
    float* ws = r.alloc<float>(linear_attention_fused_ws_floats(B, H * W));
    r.flops += 2.0 * M * 384 * C + 2.0 * M * 4 * 32 * 32 + 2.0 * B * C * 128 * 32 + 2.0 * M * 128 * C;
    if (!r.dry)
      linear_attention_fused<T>(x, la.wqkv_g, la.wout, la.bout, la.gout, weff, y, B, H * W, C, ws, r.st, la.qshift);
    emu_round<T>(r, y, C, M, C);
  }
  const void* linattn(Run& r, const LA& la, const void* x, int C, int B, int H, int W) {
    RoleScope rs(g_role == R_MID ? R_MID : R_LA);
    const size_t M = (size_t)B * H * W;
    if (la_fused(la, C)) {
      T* y = r.alloc<T>(M * C);
      linattn_fused(r, la, x, C, B, H, W, y);
      return y;
    }
    T* qkv = r.alloc<T>(M * 384);
    if (la.qkv_cs && lnf_fits(C, 384, ACT_NONE, H * W)) {
      Epi ef;                                       // PreNorm folded into to_qkv
      ef.lnf_cs = la.qkv_cs; ef.lnf_n = C;
      conv_call<T>(r, la.qkv_f, x, C, C, nullptr, 0, B, H, W, 0, 1, 0, qkv, 384, ef);
    } else {
      T* xn = r.alloc<T>(M * C);
      ln<T>(r, x, C, xn, C, nullptr, 0, la.gpre, nullptr, (int)M, C, 1e-5f);
      conv_call<T>(r, la.qkv, xn, C, C, nullptr, 0, B, H, W, 0, 1, 0, qkv, 384, Epi());
    }
    // Context k v^T (MFMA) folded into per-image to_out weights (linattn.hip).
    T* weff = r.alloc<T>((size_t)B * C * 128);
    float* ws = r.alloc<float>(linear_attention_ws_floats(B, H * W));
    r.flops += 2.0 * M * 4 * 32 * 32 + 2.0 * B * C * 128 * 32;
    // f16: W_eff / HW is subnormal, so W_eff is stored times S / HW (S = 2^k >= HW) and the GEMM
    // epilogue takes 1/S out exactly: (acc + 0) * (1 + (2^-k - 1)) + bout, from one shared
    // scale/shift row (ss_ld = 0).
    constexpr bool hw_late = std::is_same<T, f16>::value;
    float* ssr = hw_late ? r.alloc<float>(2 * (size_t)C) : nullptr;
    if (!r.dry) {
      int k = 0;
      while ((1 << k) < H * W) ++k;
      const float S = std::ldexp(1.f, k);
      linear_attention_weff<T>(qkv, la.wout, weff, B, H * W, C, ws, r.st, hw_late ? S / (float)(H * W) : 0.f);
      if (hw_late) ss_fill(ssr, C, 1.f / S - 1.f, la.bout, r.st);
    }
    ConvW wo;
    wo.w = weff; wo.b = hw_late ? nullptr : la.bout; wo.cout = C; wo.cin = wo.cin_real = 128;
    T* t = r.alloc<T>(M * C);
    Epi eo;
    eo.amode = 1; eo.w_bstride = (long long)C * 128;
    if (hw_late) { eo.ss = ssr; eo.ss_ld = 0; }
    conv_call<T>(r, wo, qkv, 384, 128, nullptr, 0, B, H, W, 0, 1, 0, t, C, eo);
    T* y = r.alloc<T>(M * C);
    ln<T>(r, t, C, y, C, x, C, la.gout, nullptr, (int)M, C, 1e-5f);
    return y;
  }

  // The dispatcher has an LN-folding kernel for this 1x1 GEMM shape (conv_lnf_ok).
  static bool gna_fits(int C, int Cout, int HW) {
    ConvArgs a{};
    a.Cin = a.C1 = a.K = C; a.Cout = a.ldy = Cout; a.gna_groups = 32; a.Ho = HW; a.Wo = 1;
    return fold_on(8) && conv_gna_ok(a, (int)sizeof(T));
  }
  static bool lnf_fits(int Cin, int Cout, int act, int HW) {
    ConvArgs a{};
    a.Cin = a.C1 = Cin; a.Cout = Cout; a.act = act; a.ldy = act == ACT_GEGLU ? Cout / 2 : Cout;
    a.Ho = HW; a.Wo = 1;
    return conv_lnf_ok(a, (int)sizeof(T));
  }
  const void* sptrans(Run& r, const ST& s, const void* x, int C, int B, int H, int W,
                      const float* cc) {
    RoleScope rs(g_role == R_MID ? R_MID : R_ST);
    const int L = H * W;
    const size_t M = (size_t)B * L;
    T* xn = r.alloc<T>(M * C);
    // GroupNorm workspace: partial moments [B][32 groups][GN_CHUNKS = 32][3], then the merged
    // (mean, rstd) [B][32][2]; or the PreNorm LN's per-block group sums + the table.
    float* stats = r.alloc<float>(std::max((size_t)B * 32 * (32 * 3 + 2), layernorm_gnstats_ws_floats(B, L, 32)));
    T* hh = r.alloc<T>(M * C);
    if (gna_fits(C, C, L)) {
      // proj_in reads xn and applies the GroupNorm to its A fragments (no normalised copy); the
      // GroupNorm statistics come out of the PreNorm LayerNorm's own pass when it can take them
      // (per-block group sums, merged by proj_in's table fill).
      Epi ep;
      const int nb = fold_on(16) ? layernorm_gnstats<T>(x, C, xn, C, s.gpre, nullptr, (int)M, C, 1e-5f, L, 32,
                                                        stats, !r.dry, r.st)
                                 : 0;
      if (nb > 0) {
        ep.gna_stats = stats; ep.gna_nb = nb;
      } else {
        ln<T>(r, x, C, xn, C, nullptr, 0, s.gpre, nullptr, (int)M, C, 1e-5f);
        ep.gna_stats = stats + (size_t)B * 32 * 32 * 3;
        if (!r.dry) groupnorm_stats<T>(xn, B, L, C, 32, 1e-6f, stats, r.st);
      }
      ep.gna_g = s.gnw; ep.gna_b = s.gnb; ep.gna_groups = 32; ep.gna_eps = 1e-6f;
      conv_call<T>(r, s.pin, xn, C, C, nullptr, 0, B, H, W, 0, 1, 0, hh, C, ep);
    } else {
      ln<T>(r, x, C, xn, C, nullptr, 0, s.gpre, nullptr, (int)M, C, 1e-5f);
      T* gn = r.alloc<T>(M * C);
      if (!r.dry) groupnorm<T>(xn, gn, s.gnw, s.gnb, B, L, C, 32, 1e-6f, stats, r.st);
      emu_round<T>(r, gn, C, M, C);
      conv_call<T>(r, s.pin, gn, C, C, nullptr, 0, B, H, W, 0, 1, 0, hh, C, Epi());
    }
    T* qkv = r.alloc<T>(M * 3 * C);
    if (s.qkv_cs && lnf_fits(C, 3 * C, ACT_NONE, L)) {
      // norm1 folded into q|k|v: the GEMM reads hh and takes its row moments itself.
      Epi ef;
      ef.lnf_cs = s.qkv_cs; ef.lnf_n = C;
      conv_call<T>(r, s.qkv_f, hh, C, C, nullptr, 0, B, H, W, 0, 1, 0, qkv, 3 * C, ef);
    } else {
      T* a = r.alloc<T>(M * C);
      ln<T>(r, hh, C, a, C, nullptr, 0, s.n1w, s.n1b, (int)M, C, 1e-5f);
      conv_call<T>(r, s.qkv, a, C, C, nullptr, 0, B, H, W, 0, 1, 0, qkv, 3 * C, Epi());
    }
    T* o = r.alloc<T>(M * C);
    r.flops += 4.0 * B * (double)L * L * C;     // QK^T and PV
    if (!r.dry) flash_attn_d32<T>(qkv, o, B, L, C / 32, s.q_pre ? 0.f : 0.17677669529663687f, r.st);
    emu_round<T>(r, o, C, M, C);
    T* h2 = r.alloc<T>(M * C);
    Epi e;
    e.res1 = hh; e.ldr1 = C;
    if (cc) {
      // attn2 over the single context token folded in as a per-image bias (see load_attn).
      e.bbias = cc + s.cc_off; e.bb_ld = cc_total;
    }
    conv_call<T>(r, s.o, o, C, C, nullptr, 0, B, H, W, 0, 1, 0, h2, C, e);
    if (!cc) {
      // No image context: attn2 is self-attention over norm2(x) (attention.py:174, 212).
      if (!s.self_ok)
        throw Error(DAC_E_ARG, "image_context is None: cross-attention falls back to self-attention, which "
                               "needs context_dim == channels (the reference fails with 'mat1 and mat2 "
                               "shapes cannot be multiplied')");
      T* a2 = r.alloc<T>(M * C);
      ln<T>(r, h2, C, a2, C, nullptr, 0, s.n2w, s.n2b, (int)M, C, 1e-5f);
      T* qkv2 = r.alloc<T>(M * 3 * C);
      conv_call<T>(r, s.qkv2, a2, C, C, nullptr, 0, B, H, W, 0, 1, 0, qkv2, 3 * C, Epi());
      T* o2 = r.alloc<T>(M * C);
      r.flops += 4.0 * B * (double)L * L * C;
      if (!r.dry) flash_attn_d32<T>(qkv2, o2, B, L, C / 32, 0.17677669529663687f, r.st);
      T* h3 = r.alloc<T>(M * C);
      Epi e3;
      e3.res1 = h2; e3.ldr1 = C;
      conv_call<T>(r, s.o2, o2, C, C, nullptr, 0, B, H, W, 0, 1, 0, h3, C, e3);
      h2 = h3;
    }
    T* g = r.alloc<T>(M * 4 * C);
    Epi eg;
    eg.act = ACT_GEGLU;
    T* f = r.alloc<T>(M * C);
    ln<T>(r, h2, C, f, C, nullptr, 0, s.n3w, s.n3b, (int)M, C, 1e-5f);
    conv_call<T>(r, s.ff1, f, C, C, nullptr, 0, B, H, W, 0, 1, 0, g, 4 * C, eg);
    T* h4 = r.alloc<T>(M * C);
    Epi e4;
    e4.res1 = h2; e4.ldr1 = C;
    conv_call<T>(r, s.ff2, g, 4 * C, 4 * C, nullptr, 0, B, H, W, 0, 1, 0, h4, C, e4);
    T* y = r.alloc<T>(M * C);
    Epi e5;
    e5.res1 = xn; e5.ldr1 = C; e5.res2 = x; e5.ldr2 = C;
    conv_call<T>(r, s.pout, h4, C, C, nullptr, 0, B, H, W, 0, 1, 0, y, C, e5);
    return y;
  }

  const void* attn(Run& r, const Attn& a, const void* x, int C, int B, int H, int W,
                   const float* cc) {
    return a.st ? sptrans(r, a.s, x, C, B, H, W, cc) : linattn(r, a.la, x, C, B, H, W);
  }

  int pad_of(int n) const {
    const int s = 1 << depth;
    return n + (s - n % s) % s;
  }

  // The level walk's state: the current activation of B images at h x w, this step's tables and
  // the skip stack the down levels push and the up levels pop.
  struct Walk {
    const void* cur; int B, h, w; const float *ss, *cc;
    std::vector<std::pair<const void*, int>> hs;
  };
  // downs[i0, i1).
  void down(Run& r, Walk& k, int i0, int i1) {
    for (int i = i0; i < i1; ++i) {
      const auto [din, dout] = levels[i];
      Level& L = downs[i];
      g_role = R_RB;
      k.cur = resblock(r, L.b1, k.cur, din, nullptr, 0, k.B, k.h, k.w, k.ss);
      k.hs.push_back({k.cur, din});
      k.cur = resblock(r, L.b2, k.cur, din, nullptr, 0, k.B, k.h, k.w, k.ss);
      k.cur = attn(r, L.at, k.cur, din, k.B, k.h, k.w, k.cc);
      g_role = R_SAMP;
      k.hs.push_back({k.cur, din});
      if (i != depth - 1) {
        T* y = r.alloc<T>((size_t)k.B * (k.h / 2) * (k.w / 2) * dout);
        conv_call<T>(r, L.samp, k.cur, din, din, nullptr, 0, k.B, k.h, k.w, 0, 2, 1, y, dout, Epi());
        k.h /= 2; k.w /= 2;
        k.cur = y;
      } else {
        T* y = r.alloc<T>((size_t)k.B * k.h * k.w * dout);
        conv_call<T>(r, L.samp, k.cur, din, din, nullptr, 0, k.B, k.h, k.w, 0, 1, 1, y, dout, Epi());
        k.cur = y;
      }
    }
  }
  void middle(Run& r, Walk& k) {
    const int mid = levels.back().second;
    g_role = R_MID;
    k.cur = resblock(r, mid1, k.cur, mid, nullptr, 0, k.B, k.h, k.w, k.ss);
    k.cur = attn(r, mid_attn, k.cur, mid, k.B, k.h, k.w, k.cc);
    k.cur = resblock(r, mid2, k.cur, mid, nullptr, 0, k.B, k.h, k.w, k.ss);
  }
  // ups[j0, j1); yout: where the last sampling conv writes instead of a fresh arena buffer.
  void up(Run& r, Walk& k, int j0, int j1, T* yout = nullptr) {
    for (int j = j0; j < j1; ++j) {
      const int i = depth - 1 - j;
      const auto [din, dout] = levels[i];
      Level& L = ups[j];
      auto sk = k.hs.back(); k.hs.pop_back();
      g_role = R_RB;
      k.cur = resblock(r, L.b1, k.cur, dout, sk.first, sk.second, k.B, k.h, k.w, k.ss);
      sk = k.hs.back(); k.hs.pop_back();
      k.cur = resblock(r, L.b2, k.cur, dout, sk.first, sk.second, k.B, k.h, k.w, k.ss);
      k.cur = attn(r, L.at, k.cur, dout, k.B, k.h, k.w, k.cc);
      g_role = R_SAMP;
      const int u = i != 0;                           // Upsample: nearest 2x, then the 3x3
      T* y = yout && j == j1 - 1 ? yout : r.alloc<T>((size_t)k.B * (k.h << u) * (k.w << u) * din);
      conv_call<T>(r, L.samp, k.cur, dout, dout, nullptr, 0, k.B, k.h, k.w, u, 1, 1, y, din, Epi());
      k.h <<= u; k.w <<= u;
      k.cur = y;
    }
  }

  // Levels sl .. depth-1 for images [0, B) of the pointers given: downs[sl..] (their skips stay
  // inside), the middle blocks, ups[..depth-1-sl], the last sampling conv writing yout
  // (B x (2h x 2w) x Cin of level sl; same resolution when sl == 0).
  void section(Run& r, int sl, const void* cur, int B, int h, int w, const float* ss, const float* cc, T* yout) {
    Walk k{cur, B, h, w, ss, cc, {}};
    down(r, k, sl, depth);
    middle(r, k);
    up(r, k, 0, depth - sl, yout);
  }

  // One forward. ss: [B][ss_total] of this step; out: [B*Hp*Wp][ldo] (channels < out_nc).
  // prepped: the input rows are already in place (the previous loop step's sde_step wrote them
  // at the same arena address, the first allocation after the reset); *xin_at receives it.
  void forward(Run& r, const float* xt, const float* mu, int B, int H, int W, const float* ss,
               const float* cc, void* out, int ldo, bool prepped = false, void** xin_at = nullptr) {
    const int Hp = pad_of(H), Wp = pad_of(W);
    const size_t M0 = (size_t)B * Hp * Wp;
    T* xin = r.alloc<T>(M0 * 8);
    if (xin_at) *xin_at = xin;
    if (!r.dry && !prepped) unet_prep<T>(xt, mu, xin, B, H, W, Hp, Wp, r.st);
    T* x0 = r.alloc<T>(M0 * nf);
    // Roles are assigned per section below; this scope restores the caller's role when the
    // forward returns (ViT / encoder calls on the thread are unaffected).
    RoleScope rs_init(R_INIT);
    SplitKScope sks(splitk32() >= 0 ? splitk32() : (half ? 4 : 0));
    conv_call<T>(r, init_conv, xin, 8, 8, nullptr, 0, B, Hp, Wp, 0, 1, 3, x0, nf, Epi());
    Walk k{x0, B, Hp, Wp, ss, cc, {}};
    if (half) {                                   // Wild-IR: levels run at half resolution
      T* xd = r.alloc<T>((size_t)B * (Hp / 2) * (Wp / 2) * nf);
      conv_call<T>(r, half_down, x0, nf, nf, nullptr, 0, B, Hp, Wp, 0, 2, 1, xd, nf, Epi());
      k.cur = xd;
      k.h = Hp / 2; k.w = Wp / 2;
    }
    // Section split: split_lvl() is the first level of the section, split_n() its branches.
    const int nbr = std::min({split_n(), B, 1 + Run::kSide});
    const bool split = split_lvl() > 0 && nbr >= 2 && r.side[nbr - 2];
    const int sl = split ? std::max(0, depth - split_lvl()) : depth;
    down(r, k, 0, sl);
    if (!split) {
      middle(r, k);
    } else {
      // The lowest split_lvl levels (by default three: the 128x128, 64x64 and 32x32 levels at
      // 256^2, i.e. downs[1..3], the middle blocks, ups[0..2]) have small, latency-bound kernels
      // (DESIGN.md §9), so with B >= 2 they run as nbr concurrent branches of B / nbr images
      // (streams r.st + r.side) whose prologues, epilogues and tails overlap. The 256^2 level
      // stays one branch: its one-block-per-CU kernels (rbfuse, conv3w) would displace each
      // other. Every kernel is per-image (batch-invariant): the outputs are bit-identical to one
      // full-batch branch. Output: the section's last sampling conv, all images.
      const int C0 = levels[sl].first;
      const int h0 = k.h, w0 = k.w;
      const size_t px = (size_t)h0 * w0;
      if (sl != 0) { k.h *= 2; k.w *= 2; }
      const size_t pxo = (size_t)k.h * k.w;
      T* y = r.alloc<T>((size_t)B * pxo * C0);
      branches(r, B, nbr, [&](Run& rk, int b0, int nb) {
        section(rk, sl, static_cast<const T*>(k.cur) + b0 * px * C0, nb, h0, w0,
                ss ? ss + (size_t)b0 * ss_total : nullptr, cc ? cc + (size_t)b0 * cc_total : nullptr,
                y + b0 * pxo * C0);
      });
      k.cur = y;
    }
    up(r, k, depth - sl, depth);
    if (half) {
      T* xu = r.alloc<T>((size_t)B * Hp * Wp * nf);
      conv_call<T>(r, half_up, k.cur, nf, nf, nullptr, 0, B, k.h, k.w, 1, 1, 1, xu, nf, Epi());
      k.cur = xu;
      k.h = Hp; k.w = Wp;
    }
    g_role = R_FIN_RB;
    k.cur = resblock(r, fin, k.cur, nf, x0, nf, B, k.h, k.w, ss);
    g_role = R_FINAL;
    conv_call<T>(r, final_conv, k.cur, nf, nf, nullptr, 0, B, k.h, k.w, 0, 1, 1, out, ldo, Epi());
  }
};

// ============================================================================= ViT
template <typename T>
struct VitNet {
  struct Block { const float *l1w, *l1b, *l2w, *l2b; ConvW qkv, out, fc, proj; };
  // conv1g: the patch conv as a GEMM over im2col rows (K = 3 P P, stride == kernel), when K
  // fits the GEMM tiles; conv1 the direct conv otherwise.
  struct Tower { ConvW conv1, conv1g; const float *cls, *pos, *prew, *preb, *postw, *postb, *projT;
                 std::vector<Block> blocks; std::vector<ConvW> zero; };
  // CLIP text tower (model.py:203-211, 237-249): token / positional embeddings (fp32 tables),
  // causal ResidualAttentionBlocks, ln_final, text_projection (transposed, fp32).
  struct TextTower { const float *tok = nullptr, *pos = nullptr, *lnw = nullptr, *lnb = nullptr,
                     *projT = nullptr; std::vector<Block> blocks; };
  dac_config cfg;
  int S, P, D, layers, heads, hd, mlp, E, G, L;
  int Lt = 0, Vt = 0, Dt = 0, Ht = 0, layers_t = 0;
  Tower main, ctl;
  TextTower txt;
  explicit VitNet(const dac_config& c) : cfg(c) {
    S = c.image_size; P = c.patch_size; D = c.width; layers = c.layers; hd = c.head_width;
    heads = D / hd; mlp = c.mlp_width; E = c.embed_dim; G = S / P; L = G * G + 1;
    if (c.text) {
      Lt = c.context_length; Vt = c.vocab_size; Dt = c.text_width; Ht = c.text_heads;
      layers_t = c.text_layers;
    }
  }
  Block load_block(Packer<T>& Pk, const std::string& q, int Dm, int mlpw) {
    Block b;
    b.l1w = Pk.f32(q + "ln_1.weight", {Dm});
    b.l1b = Pk.f32(q + "ln_1.bias", {Dm});
    b.qkv = Pk.linear(q + "attn.in_proj_weight", 3 * Dm, Dm, q + "attn.in_proj_bias");
    b.out = Pk.linear(q + "attn.out_proj.weight", Dm, Dm, q + "attn.out_proj.bias");
    b.l2w = Pk.f32(q + "ln_2.weight", {Dm});
    b.l2b = Pk.f32(q + "ln_2.bias", {Dm});
    b.fc = Pk.linear(q + "mlp.c_fc.weight", mlpw, Dm, q + "mlp.c_fc.bias");
    b.proj = Pk.linear(q + "mlp.c_proj.weight", Dm, mlpw, q + "mlp.c_proj.bias");
    return b;
  }
  // ResidualAttentionBlock.forward (transformer.py:232-244) on Mt = Bs * Ls token rows:
  // x += attn(ln_1(x)); x += mlp(ln_2(x)) [+ res2, the controlled tower's control.pop()].
  T* block(Run& r, const Block& b, const void* x, int Bs, int Ls, int Dm, int Hm, int mlpw, int causal,
           const void* res2) {
    const size_t Mt = (size_t)Bs * Ls;
    T* a = r.alloc<T>(Mt * Dm);
    ln<T>(r, x, Dm, a, Dm, nullptr, 0, b.l1w, b.l1b, (int)Mt, Dm, 1e-5f);
    T* qkv = r.alloc<T>(Mt * 3 * Dm);
    Epi eq;
    eq.split_rows = Ls;
    conv_call<T>(r, b.qkv, a, Dm, Dm, nullptr, 0, 1, 1, (int)Mt, 0, 1, 0, qkv, 3 * Dm, eq);
    T* o = r.alloc<T>(Mt * Dm);
    r.flops += 4.0 * Bs * (double)Ls * Ls * Dm;
    if (!r.dry) small_mha<T>(qkv, o, Bs, Ls, Hm, Dm / Hm, causal, r.st);
    T* x2 = r.alloc<T>(Mt * Dm);
    Epi e1;
    e1.res1 = x; e1.ldr1 = Dm;
    e1.split_rows = Ls;
    conv_call<T>(r, b.out, o, Dm, Dm, nullptr, 0, 1, 1, (int)Mt, 0, 1, 0, x2, Dm, e1);
    T* a2 = r.alloc<T>(Mt * Dm);
    ln<T>(r, x2, Dm, a2, Dm, nullptr, 0, b.l2w, b.l2b, (int)Mt, Dm, 1e-5f);
    T* f = r.alloc<T>(Mt * mlpw);
    Epi eg;
    eg.act = ACT_GELU;
    eg.split_rows = Ls;
    conv_call<T>(r, b.fc, a2, Dm, Dm, nullptr, 0, 1, 1, (int)Mt, 0, 1, 0, f, mlpw, eg);
    T* x3 = r.alloc<T>(Mt * Dm);
    Epi e3;
    e3.res1 = x2; e3.ldr1 = Dm;
    if (res2) { e3.res2 = res2; e3.ldr2 = Dm; }
    e3.split_rows = Ls;
    conv_call<T>(r, b.proj, f, mlpw, mlpw, nullptr, 0, 1, 1, (int)Mt, 0, 1, 0, x3, Dm, e3);
    return x3;
  }
  Tower load_tower(Packer<T>& Pk, const std::string& p, bool control) {
    Tower t;
    t.conv1 = Pk.conv(p + "conv1.weight", D, 3, P, P);
    const int K = 3 * P * P;
    const HostW* w1 = t.conv1.w ? Pk.ws.get(p + "conv1.weight", {D, 3, P, P}) : nullptr;
    if (K % 64 == 0 && w1 && vit_gemm_on()) {
      // [D][P][P][3]: the same weights without the padding channels, as one GEMM operand.
      const std::vector<float> q = pack_ohwi(w1->v.data(), D, 3, P, P, P, 3);
      ConvW& g = t.conv1g;
      g.cout = D; g.cin = g.cin_real = K; g.kh = g.kw = 1;
      g.w = Pk.upload_T(q, p + "conv1.weight", P * P, 3);
      Pk.make_fp8(g, q, D, K);
    }
    t.cls = Pk.f32(p + "class_embedding", {D});
    t.pos = Pk.f32(p + "positional_embedding", {L, D});
    t.prew = Pk.f32(p + "ln_pre.weight", {D});
    t.preb = Pk.f32(p + "ln_pre.bias", {D});
    t.postw = Pk.f32(p + "ln_post.weight", {D});
    t.postb = Pk.f32(p + "ln_post.bias", {D});
    t.projT = Pk.f32_t(p + "proj", D, E);
    const std::string rb = p + (control ? "transformer.transformer.resblocks." : "transformer.resblocks.");
    for (int l = 0; l < layers; ++l) {
      t.blocks.push_back(load_block(Pk, rb + std::to_string(l) + ".", D, mlp));
      if (control)
        t.zero.push_back(Pk.linear(p + "transformer.zero_modules." + std::to_string(l) + ".weight",
                                   D, D, p + "transformer.zero_modules." + std::to_string(l) + ".bias"));
    }
    return t;
  }
  void load(Packer<T>& Pk, WStore& ws) {
    // `visual.*` aliases `clip.visual.*` (daclip_model.py:21): accept either spelling.
    std::vector<std::string> alias;
    for (auto& kv : ws.m)
      if (kv.first.rfind("visual.", 0) == 0) alias.push_back(kv.first);
    for (auto& k : alias) {
      const std::string c = "clip." + k;
      if (!ws.m.count(c)) ws.m[c] = ws.m[k];
      ws.m[k].used = true;
    }
    main = load_tower(Pk, "clip.visual.", false);
    ctl = load_tower(Pk, "visual_control.", true);
    if (cfg.text) {
      txt.tok = Pk.f32("clip.token_embedding.weight", {Vt, Dt});
      txt.pos = Pk.f32("clip.positional_embedding", {Lt, Dt});
      for (int l = 0; l < layers_t; ++l)
        txt.blocks.push_back(load_block(Pk, "clip.transformer.resblocks." + std::to_string(l) + ".", Dt, 4 * Dt));
      txt.lnw = Pk.f32("clip.ln_final.weight", {Dt});
      txt.lnb = Pk.f32("clip.ln_final.bias", {Dt});
      txt.projT = Pk.f32_t("clip.text_projection", Dt, E);
    }
  }
  // CLIP.encode_text (model.py:237-249): the EOT row is gathered before ln_final (a per-row
  // op), then projected.
  void encode_text(Run& r, const int64_t* tokens, int N, float* out) {
    const size_t Mt = (size_t)N * Lt;
    T* x = r.alloc<T>(Mt * Dt);
    if (!r.dry) text_embed<T>(tokens, txt.tok, txt.pos, x, N, Lt, Dt, Vt, r.st);
    const void* cur = x;
    for (int l = 0; l < layers_t; ++l) cur = block(r, txt.blocks[l], cur, N, Lt, Dt, Ht, 4 * Dt, 1, nullptr);
    T* pooled = r.alloc<T>((size_t)N * Dt);
    if (!r.dry) eot_gather<T>(tokens, cur, pooled, N, Lt, Dt, r.st);
    T* pn = r.alloc<T>((size_t)N * Dt);
    ln<T>(r, pooled, Dt, pn, Dt, nullptr, 0, txt.lnw, txt.lnb, N, Dt, 1e-5f);
    float* pf = r.alloc<float>((size_t)N * Dt);
    r.flops += 2.0 * N * Dt * E;
    if (!r.dry) {
      rows_to_f32<T>(pn, Dt, pf, N, Dt, r.st);
      small_linear(pf, Dt, txt.projT, nullptr, out, E, N, Dt, E, ACT_NONE, ACT_NONE, nullptr, 0, 1, r.st);
    }
  }
  void tower(Run& r, const Tower& tw, const void* xin, int B, bool control,
             std::vector<const void*>* hid_out, const std::vector<const void*>* hid_in,
             float* out, bool gemm) {
    constexpr int VE = sizeof(T) == 2 ? 8 : 4;
    const size_t Mt = (size_t)B * L;
    T* patch = r.alloc<T>((size_t)B * G * G * D);
    if (gemm) {
      // xin holds the im2col rows (encode): one GEMM over B * G^2 rows, K = 3 P P.
      const int K = 3 * P * P;
      Epi es;
      es.split_rows = G * G;
      conv_call<T>(r, tw.conv1g, xin, K, K, nullptr, 0, B, G * G, 1, 0, 1, 0, patch, D, es);
    } else {
      conv_call<T>(r, tw.conv1, xin, VE, VE, nullptr, 0, B, S, S, 0, P, 0, patch, D, Epi());
    }
    T* tok = r.alloc<T>(Mt * D);
    if (!r.dry) vit_embed<T>(patch, tw.cls, tw.pos, tok, B, L, D, r.st);
    T* x = r.alloc<T>(Mt * D);
    ln<T>(r, tok, D, x, D, nullptr, 0, tw.prew, tw.preb, (int)Mt, D, 1e-5f);
    for (int l = 0; l < layers; ++l) {
      T* x3 = block(r, tw.blocks[l], x, B, L, D, heads, mlp, 0,
                    hid_in ? (*hid_in)[layers - 1 - l] : nullptr);        // control.pop()
      if (control) {
        T* hz = r.alloc<T>(Mt * D);
        Epi ez;
        ez.split_rows = L;
        conv_call<T>(r, tw.zero[l], x3, D, D, nullptr, 0, 1, 1, (int)Mt, 0, 1, 0, hz, D, ez);
        hid_out->push_back(hz);
      }
      x = x3;
    }
    T* pooled = r.alloc<T>((size_t)B * D);
    ln<T>(r, x, L * D, pooled, D, nullptr, 0, tw.postw, tw.postb, B, D, 1e-5f);
    float* pf = r.alloc<float>((size_t)B * D);
    r.flops += 2.0 * B * D * E;
    if (!r.dry) {
      rows_to_f32<T>(pooled, D, pf, B, D, r.st);
      small_linear(pf, D, tw.projT, nullptr, out, E, B, D, E, ACT_NONE, ACT_NONE, nullptr, 0, 1, r.st);
    }
  }
  // control: DaCLIP.encode_image(control=True) (daclip_model.py:46-53), the controller tower
  // and then the clip tower with its hiddens; otherwise CLIP.encode_image (daclip_model.py:54-55
  // -> model.py:233-235), the clip tower alone.
  void encode(Run& r, const float* img, int B, float* ic, float* dc, bool control) {
    constexpr int VE = sizeof(T) == 2 ? 8 : 4;
    const bool gemm = main.conv1g.w && (!control || ctl.conv1g.w);
    T* xin = r.alloc<T>(gemm ? (size_t)B * S * S * 3 : (size_t)B * S * S * VE);
    if (!r.dry) {
      if (gemm) vit_patches<T>(img, xin, B, S, P, r.st);
      else vit_prep<T>(img, xin, B, S, r.st);
    }
    std::vector<const void*> hid;
    if (control) tower(r, ctl, xin, B, true, &hid, nullptr, dc, gemm);
    tower(r, main, xin, B, false, nullptr, control ? &hid : nullptr, ic, gemm);
  }
};

// ============================================================================= engine
template <typename T>
class EngineT : public Engine {
 public:
  EngineT(int device, const dac_config& c, bool fp8w = false) : dev(device), cfg(c), fp8(fp8w) {
    HIP_OK(hipSetDevice(dev));
    HIP_OK(hipStreamCreateWithFlags(&priv, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    for (int k = 0; k < Run::kSide; ++k) {
      HIP_OK(hipStreamCreateWithFlags(&side[k], hipStreamNonBlocking));
      HIP_OK(hipEventCreateWithFlags(&ev_join[k], hipEventDisableTiming));
    }
    HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    zero_page = pool.alloc(256);
    HIP_OK(hipMemset(zero_page, 0, 256));
    if (c.unet) unet = std::make_unique<UNetNet<T>>(c);
    if (c.vit) {
      if (c.image_size % c.patch_size || c.width % c.head_width || (c.head_width != 64 && c.head_width != 32) ||
          (c.image_size / c.patch_size) * (c.image_size / c.patch_size) + 1 > 320)
        throw Error(DAC_E_ARG, "unsupported vision config (needs <= 320 tokens, head_width 32 or 64)");
      if (c.text && (c.text_heads < 1 || c.text_width % c.text_heads || c.context_length < 1 ||
                     c.context_length > 320 || c.vocab_size < 1 || c.text_layers < 1 ||
                     (c.text_width / c.text_heads != 64 && c.text_width / c.text_heads != 32)))
        throw Error(DAC_E_ARG, "unsupported text config (head width 32 or 64, context <= 320)");
      vit = std::make_unique<VitNet<T>>(c);
    }
  }
  ~EngineT() override {
    clear_graphs();
    if (arena.base) (void)hipFree(arena.base);
    for (auto& kv : bufs) release(kv.second);
    for (auto& kv : tloops) release(kv.second);
    (void)hipEventDestroy(ev_in);
    (void)hipEventDestroy(ev_out);
    (void)hipEventDestroy(ev_fork);
    for (int k = 0; k < Run::kSide; ++k) {
      (void)hipEventDestroy(ev_join[k]);
      (void)hipStreamDestroy(side[k]);
    }
    (void)hipStreamDestroy(priv);
  }

  void finalize(WStore& ws) override {
    HIP_OK(hipSetDevice(dev));
    Packer<T> P{pool, ws, pack_knobs_from_env()};
    // fp8 handles: the UNet runs the 16-bit kernels with its 64 -> 64 ResBlock block2 convs on
    // e4m3 (q8: conv3q.hip, fed by e4m3 block1 epilogues); the ViT's GEMMs take e4m3 MX weights
    // (conv8.hip). (conv8 on the UNet's layers measured 1.2-3.5x slower than their 16-bit
    // kernels: it quantizes activations in its A loader.)
    P.q8 = fp8;
    if (unet) unet->load(P);
    P.q8 = false;
    P.fp8 = fp8;
    if (vit) vit->load(P, ws);
    if (!ws.missing.empty()) {
      std::string m = "Missing key(s) in state_dict: ";
      for (size_t i = 0; i < ws.missing.size(); ++i) m += (i ? ", \"" : "\"") + ws.missing[i] + "\"";
      throw Error(DAC_E_MISSING, m);
    }
    ready = true;
  }

  // ------------------------------------------------------------------ workspace
  void ensure_arena(size_t bytes) {
    if (arena.cap >= bytes) return;
    if (arena.base) HIP_OK(hipFree(arena.base));
    clear_graphs();
    arena.base = nullptr;
    HIP_OK(hipMalloc(&arena.base, bytes));
    arena.cap = bytes;
    if (poison()) HIP_OK(hipMemset(arena.base, 0xFF, bytes));
  }
  // Device buffers of one cached loop shape. Every dalloc registers its pointer with the struct it
  // allocates for, and release() walks that list: no field is named twice.
  struct Bufs {
    float *xs = nullptr, *mus = nullptr, *tcs = nullptr, *ics = nullptr, *ss = nullptr,
          *cc = nullptr, *sin = nullptr;
    float* noise = nullptr;       // owned copy of injected noise [nT,B,3,H,W] (lazily allocated)
    void* out = nullptr;
    uint64_t* seed = nullptr;     // [seed, element offset of image 0]
    int ldo = 0;
    std::vector<void*> owned;
  };
  template <class X> X* dalloc(Bufs& o, size_t n) {
    const size_t bytes = std::max<size_t>(n * sizeof(X), 16);
    o.owned.push_back(nullptr);
    HIP_OK(hipMalloc(&o.owned.back(), bytes));
    if (poison()) HIP_OK(hipMemset(o.owned.back(), 0xFF, bytes));
    return (X*)o.owned.back();
  }
  void release(Bufs& b) {
    for (void* p : b.owned) (void)hipFree(p);
    b.owned.clear();
  }
  // The fields both loops share: B images of n floats in all, nT steps, a UNet output of out_px
  // padded pixels.
  void alloc_loop(Bufs& b, int B, size_t n, int nT, size_t out_px) {
    b.xs = dalloc<float>(b, n);
    b.mus = dalloc<float>(b, n);
    b.tcs = dalloc<float>(b, (size_t)B * std::max(1, unet->ctx));
    b.ics = dalloc<float>(b, (size_t)B * std::max(1, unet->ctx));
    b.ss = dalloc<float>(b, (size_t)nT * B * unet->ss_total);
    b.cc = dalloc<float>(b, (size_t)B * std::max(1, unet->cc_total));
    b.sin = dalloc<float>(b, (size_t)nT * B * unet->nf);
    b.ldo = 4;
    b.out = dalloc<char>(b, out_px * b.ldo * sizeof(T));
    b.seed = dalloc<uint64_t>(b, 2);
  }
  // The entry of a shape cache, filled by fill(entry) on a miss. Graphs bake the buffers' addresses
  // in, so a cache that is full (max entries) drops every graph together with all its buffers. A
  // fill that throws releases what the entry holds and leaves no entry.
  template <class M, class F>
  typename M::mapped_type& cache_entry(M& m, const typename M::key_type& key, size_t max, F&& fill) {
    auto it = m.find(key);
    if (it != m.end()) return it->second;
    if (m.size() >= max) {
      HIP_OK(hipDeviceSynchronize());
      clear_graphs();
      for (auto& kv : m) release(kv.second);
      m.clear();
    }
    auto& e = m[key];
    try {
      fill(e);
    } catch (...) {
      release(e);
      m.erase(key);
      throw;
    }
    return e;
  }
  std::map<std::tuple<int, int, int, int>, Bufs> bufs;    // (B, H, W, nT)
  static constexpr size_t kMaxShapes = 8;
  Bufs& get_bufs(int B, int H, int W, int nT) {
    return cache_entry(bufs, std::make_tuple(B, H, W, nT), kMaxShapes, [&](Bufs& b) {
      alloc_loop(b, B, (size_t)B * 3 * H * W, nT, (size_t)B * unet->pad_of(H) * unet->pad_of(W));
    });
  }
  void set_side(Run& r) {
    for (int k = 0; k < Run::kSide; ++k) { r.side[k] = side[k]; r.evj[k] = ev_join[k]; }
    r.evf = ev_fork;
  }
  Run live(hipStream_t st) {
    Run r;
    r.st = st;
    r.zero = zero_page;
    r.dry = false;
    arena.dry = false;
    r.ar = &arena;
    set_side(r);
    return r;
  }
  // A dry Run over `a`: the same launch sequence with nothing launched, for arena sizes, argument
  // checks, FLOP counts and the profiler's slot counts. sides: fork the split section as the live
  // recording does (same allocation sequence).
  Run dry(Arena& a, bool sides = false, Profiler* p = nullptr, const void* zero = nullptr) {
    Run r;
    r.dry = true;
    r.ar = &a;
    r.prof = p;
    r.zero = zero;
    if (sides) set_side(r);
    return r;
  }
  // Arena bytes of a UNet call or loop: dry runs of the tables for (B, nT, has_ic) and of one
  // forward per listed (images, h, w), the arena reset before each (they also carry the argument
  // checks, e.g. the self-attention fallback, before anything is launched or captured).
  struct Fwd { int nb, h, w; };
  size_t plan(int B, int nT, bool has_ic, std::initializer_list<Fwd> fwds) {
    Arena a;
    Run r = dry(a, true);
    const float* dummy = (const float*)1;
    unet->tables(r, nullptr, nT, 0.0, 0.0, 1.0, dummy, has_ic ? dummy : nullptr, B, nullptr, nullptr);
    for (const Fwd& f : fwds) {
      if (f.nb < 1) continue;
      a.reset();
      unet->forward(r, nullptr, nullptr, f.nb, f.h, f.w, nullptr, has_ic ? dummy : nullptr, nullptr, 4);
    }
    return a.peak + (1 << 20);
  }

  // ------------------------------------------------------------------ encode
  void encode(const float* img, int B, float* ic, float* dc, hipStream_t st) override {
    need(vit != nullptr, "handle has no vision towers");
    HIP_OK(hipSetDevice(dev));
    Arena a;
    Run d = dry(a);
    vit->encode(d, nullptr, B, nullptr, nullptr, dc != nullptr);
    ensure_arena(a.peak + (1 << 20));
    Run r = live(st);
    arena.reset();
    vit->encode(r, img, B, ic, dc, dc != nullptr);
    HIP_OK(hipGetLastError());
  }

  // ------------------------------------------------------------------ text
  void encode_text(const int64_t* tokens, int N, float* out, hipStream_t st) override {
    need(vit != nullptr && cfg.text, "handle has no text tower");
    HIP_OK(hipSetDevice(dev));
    Arena a;
    Run d = dry(a);
    vit->encode_text(d, nullptr, N, nullptr);
    ensure_arena(a.peak + (1 << 20));
    Run r = live(st);
    arena.reset();
    vit->encode_text(r, tokens, N, out);
    HIP_OK(hipGetLastError());
  }

  // ------------------------------------------------------------------ one UNet call
  void unet_forward(const float* xt, const float* mu, float t, const float* tc, const float* icx,
                    int B, int H, int W, float* eps, hipStream_t st) override {
    need(unet != nullptr, "handle has no UNet");
    HIP_OK(hipSetDevice(dev));
    const float* tcu = unet->degra ? tc : nullptr;
    const float* icu = unet->imgctx ? icx : nullptr;
    ensure_arena(plan(B, 1, icu != nullptr, {{B, H, W}}));
    Bufs& b = get_bufs(B, H, W, 1);
    Run r = live(st);
    arena.reset();
    unet->tables(r, b.sin, 1, (double)t, 0.0, 1.0, tcu, icu, B, b.ss, b.cc);
    arena.reset();
    unet->forward(r, xt, mu, B, H, W, b.ss, icu ? b.cc : nullptr, b.out, b.ldo);
    unet_out<T>(b.out, b.ldo, eps, B, H, W, unet->pad_of(H), unet->pad_of(W), st);
    HIP_OK(hipGetLastError());
  }

  void posterior_step(int mode, float* x, const float* eps, const float* mu, const float* z, int t,
                      int n, hipStream_t st) override {
    need(sched.T > 0, "schedule not set");
    need(t >= 1 && t <= sched.T, "t out of range");
    need(z != nullptr, "posterior_step needs explicit noise");
    need(n > 0 && n % 3 == 0, "posterior_step: n must be B*3*H*W");
    // eps is NCHW here (ld = 0 selects flat indexing in the kernel); the kernel covers
    // B*3*H*W elements, so the flat view is B = H = 1, W = n / 3.
    sde_step<float>(mode, x, mu, eps, 0, 1, 1, z, nullptr, 0, sched.coef(t, mode), 1, 1, n / 3, st);
    HIP_OK(hipGetLastError());
  }

  // ------------------------------------------------------------------ full loop
  // One captured loop per (mode | feature bits, shape). Feature bits: 2 = no text context
  // (no prompt embedding), 4 = no image context (self-attention attn2), 8 = injected noise
  // (read from the handle-owned copy, so the caller's pointer is not part of the key).
  struct GKey {
    int mode, B, H, W, nT;
    bool operator<(const GKey& o) const {
      return std::tie(mode, B, H, W, nT) < std::tie(o.mode, o.B, o.H, o.W, o.nT);
    }
  };
  std::map<GKey, hipGraphExec_t> graphs;
  void clear_graphs() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
    for (auto& kv : tloops) {
      for (auto& g : kv.second.graphs)
        if (g.second) (void)hipGraphExecDestroy(g.second);
      kv.second.graphs.clear();
    }
  }
  // One loop call: its arguments and what both entry points derive from them (n = B*3*H*W floats;
  // mkey = mode | feature bits).
  struct LoopCall {
    int mode; float* x; const float *mu, *tc, *icx; int B, H, W, nT; const float* noise; uint64_t seed;
    hipStream_t st;
    bool has_tc, has_ic, has_noise; int mkey; size_t n;
  };
  LoopCall loop_call(int mode, float* x, const float* mu, const float* tc, const float* icx, int B, int H, int W,
                     int nT, const float* noise, uint64_t seed, hipStream_t st, int tpf = 1) {
    need(unet != nullptr, "handle has no UNet");
    need(tpf >= 1, "tiles_per_forward must be >= 1");
    need(sched.T > 0, "call dac_sde_schedule first");
    need(nT >= 1 && nT <= sched.T, "T exceeds the schedule length");
    LoopCall c{mode, x, mu, tc, icx, B, H, W, nT, noise, seed, st};
    c.has_tc = tc != nullptr && unet->degra;
    c.has_ic = icx != nullptr && unet->imgctx;
    c.has_noise = noise != nullptr;
    c.mkey = mode | (c.has_tc ? 0 : 2) | (c.has_ic ? 0 : 4) | (c.has_noise ? 8 : 0);
    c.n = (size_t)B * 3 * H * W;
    return c;
  }
  // Prologue of a loop call: the caller's stream hands over to the private one, which copies the
  // inputs into the loop's buffers and writes the noise key.
  void stage(Bufs& b, const LoopCall& c) {
    if (c.has_noise && !b.noise) b.noise = dalloc<float>(b, (size_t)c.nT * c.n);
    HIP_OK(hipEventRecord(ev_in, c.st));
    HIP_OK(hipStreamWaitEvent(priv, ev_in, 0));
    HIP_OK(hipMemcpyAsync(b.xs, c.x, c.n * 4, hipMemcpyDeviceToDevice, priv));
    HIP_OK(hipMemcpyAsync(b.mus, c.mu, c.n * 4, hipMemcpyDeviceToDevice, priv));
    if (c.has_tc) HIP_OK(hipMemcpyAsync(b.tcs, c.tc, (size_t)c.B * unet->ctx * 4, hipMemcpyDeviceToDevice, priv));
    if (c.has_ic) HIP_OK(hipMemcpyAsync(b.ics, c.icx, (size_t)c.B * unet->ctx * 4, hipMemcpyDeviceToDevice, priv));
    if (c.has_noise) HIP_OK(hipMemcpyAsync(b.noise, c.noise, (size_t)c.nT * c.n * 4, hipMemcpyDeviceToDevice, priv));
    // Noise key [seed, element offset of image 0], written in stream order by a kernel. Tiled or
    // not, a pixel's draw depends on the full image alone.
    set_u64x2(b.seed, c.seed, noise_offset * (uint64_t)(3 * c.H * c.W), priv);
  }
  // Epilogue: the state back to the caller, and the caller's stream waits for it.
  void finish(Bufs& b, const LoopCall& c) {
    HIP_OK(hipMemcpyAsync(c.x, b.xs, c.n * 4, hipMemcpyDeviceToDevice, priv));
    HIP_OK(hipEventRecord(ev_out, priv));
    HIP_OK(hipStreamWaitEvent(c.st, ev_out, 0));
  }
  // Captures what rec() enqueues on the private stream (and the side streams it forks) into a
  // graph. A throwing rec() still ends the capture; its dead graph is destroyed.
  template <class F> hipGraph_t capture(F&& rec) {
    hipGraph_t g = nullptr;
    HIP_OK(hipStreamBeginCapture(priv, hipStreamCaptureModeThreadLocal));
    try {
      rec();
    } catch (...) {
      hipGraph_t dead = nullptr;
      (void)hipStreamEndCapture(priv, &dead);
      if (dead) (void)hipGraphDestroy(dead);
      throw;
    }
    HIP_OK(hipStreamEndCapture(priv, &g));
    return g;
  }

  void record_loop(Run& r, Bufs& b, const LoopCall& c) {
    const int B = c.B, H = c.H, W = c.W, nT = c.nT;
    const int Hp = unet->pad_of(H), Wp = unet->pad_of(W);
    r.ar->reset();
    // Step i runs the model at time (T - i) * sample_scale (sde_utils.py:302).
    unet->tables(r, b.sin, nT, (double)nT, -1.0, sched.time_scale, c.has_tc ? b.tcs : nullptr,
                 c.has_ic ? b.ics : nullptr, B, b.ss, b.cc);
    // Unpadded images: each step's sampler update also writes the next step's UNet input rows
    // (same values unet_prep computes from the new x), one launch less per step.
    const bool fuse = fuse_prep_on() && sde_step_fuses(b.ldo, H, W, Hp, Wp);
    for (int i = 0; i < nT; ++i) {
      const int t = nT - i;
      r.ar->reset();
      void* xin = nullptr;
      unet->forward(r, b.xs, b.mus, B, H, W, b.ss + (size_t)i * B * unet->ss_total, c.has_ic ? b.cc : nullptr,
                    b.out, b.ldo, fuse && i > 0, &xin);
      if (!r.dry)
        sde_step<T>(c.mode, b.xs, b.mus, b.out, b.ldo, Hp, Wp, c.has_noise ? b.noise + (size_t)i * c.n : nullptr,
                    b.seed, (uint32_t)t, sched.coef(t, c.mode), B, H, W, r.st, fuse && i + 1 < nT ? xin : nullptr);
    }
  }
  void sde_reverse(int mode, float* x, const float* mu, const float* tc, const float* icx, int B,
                   int H, int W, int nT, const float* noise, uint64_t seed, hipStream_t st) override {
    const LoopCall c = loop_call(mode, x, mu, tc, icx, B, H, W, nT, noise, seed, st);
    HIP_OK(hipSetDevice(dev));
    ensure_arena(plan(B, nT, c.has_ic, {{B, H, W}}));
    Bufs& b = get_bufs(B, H, W, nT);
    stage(b, c);
    if (prof.on()) {
      profile_pass(b, c);
    } else if (no_graph()) {
      Run r = live(priv);
      record_loop(r, b, c);
    } else {
      const GKey key{c.mkey, B, H, W, nT};
      auto it = graphs.find(key);
      if (it == graphs.end()) {
        Run r = live(priv);
        hipGraph_t g = capture([&] { record_loop(r, b, c); });
        hipGraphExec_t ex;
        HIP_OK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
        HIP_OK(hipGraphDestroy(g));
        it = graphs.emplace(key, ex).first;
      }
      HIP_OK(hipGraphLaunch(it->second, priv));
    }
    finish(b, c);
  }

  // ------------------------------------------------------------------ tiled loop
  // One full-image state; every step gathers its tiles, runs the UNet on them C at a time,
  // blends the per-tile eps back to a full-image eps (tile.hip) and applies the flat fp32 sampler
  // update to the whole image, so the noise and the trajectory do not depend on the tiling.
  // Buffers and graphs are cached per (shape, grid contents, chunk, T); the buffers live outside
  // the arena (the arena only holds one forward's activations).
  struct TKey {
    int B, H, W, th, tw, ov, C, nT;
    std::vector<int32_t> ys, xs;
    bool operator<(const TKey& o) const {
      return std::tie(B, H, W, th, tw, ov, C, nT, ys, xs) <
             std::tie(o.B, o.H, o.W, o.th, o.tw, o.ov, o.C, o.nT, o.ys, o.xs);
    }
  };
  struct TBufs : Bufs {
    float *xt = nullptr;          // [C, 3, th, tw] tiles of the current state (one chunk)
    float *mut = nullptr;         // [NT, 3, th, tw] tiles of mu, gathered once per call
    float *epst = nullptr;        // [NT, 3, th, tw] per-tile eps
    float *eps = nullptr;         // [B, 3, H, W] blended eps
    float *ssc = nullptr;         // [C, ss_total] the chunk's (scale, shift) rows
    float *cct = nullptr;         // [NT, cc_total] cross-attention constants per tile
    int32_t *ysd = nullptr, *xsd = nullptr;
  };
  struct TLoop : TBufs {
    std::map<int, hipGraphExec_t> graphs;     // by mode | feature bits; null = runs eagerly
  };
  std::map<TKey, TLoop> tloops;
  static constexpr size_t kMaxTiledShapes = 4;
  // A captured loop with more nodes than this is not instantiated: the loop is enqueued eagerly
  // on the private stream instead (the same launch sequence, so the same result).
  static constexpr size_t kMaxGraphNodes = 65536;
  TLoop& get_tloop(const TKey& key) {
    return cache_entry(tloops, key, kMaxTiledShapes, [&](TLoop& b) {
      const int ny = (int)key.ys.size(), nx = (int)key.xs.size(), NT = key.B * ny * nx;
      const size_t n = (size_t)key.B * 3 * key.H * key.W, tn = (size_t)3 * key.th * key.tw;
      alloc_loop(b, key.B, n, key.nT, (size_t)key.C * unet->pad_of(key.th) * unet->pad_of(key.tw));
      b.eps = dalloc<float>(b, n);
      b.xt = dalloc<float>(b, (size_t)key.C * tn);
      b.mut = dalloc<float>(b, (size_t)NT * tn);
      b.epst = dalloc<float>(b, (size_t)NT * tn);
      b.ssc = dalloc<float>(b, (size_t)key.C * unet->ss_total);
      b.cct = dalloc<float>(b, (size_t)NT * std::max(1, unet->cc_total));
      b.ysd = dalloc<int32_t>(b, ny);
      b.xsd = dalloc<int32_t>(b, nx);
      HIP_OK(hipMemcpy(b.ysd, key.ys.data(), ny * sizeof(int32_t), hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(b.xsd, key.xs.data(), nx * sizeof(int32_t), hipMemcpyHostToDevice));
    });
  }
  void record_tiled(Run& r, TBufs& b, const TKey& k, const LoopCall& c) {
    const int ny = (int)k.ys.size(), nx = (int)k.xs.size(), per = ny * nx, NT = k.B * per;
    const int Hp = unet->pad_of(k.th), Wp = unet->pad_of(k.tw);
    const size_t tn = (size_t)3 * k.th * k.tw;
    r.ar->reset();
    // Per-image tables (step i runs the model at (T - i) * sample_scale); a chunk's rows are
    // copies of its tiles' images' rows.
    unet->tables(r, b.sin, k.nT, (double)k.nT, -1.0, sched.time_scale, c.has_tc ? b.tcs : nullptr,
                 c.has_ic ? b.ics : nullptr, k.B, b.ss, b.cc);
    if (!r.dry) {
      tile_gather(b.mus, b.mut, b.ysd, b.xsd, k.xs.data(), ny, nx, k.H, k.W, k.th, k.tw, 0, NT, r.st);
      if (c.has_ic) rows_gather(b.cc, b.cct, NT, unet->cc_total, 0, per, r.st);
    }
    for (int i = 0; i < k.nT; ++i) {
      const int t = k.nT - i;
      for (int k0 = 0; k0 < NT; k0 += k.C) {
        const int nb = std::min(k.C, NT - k0);
        r.ar->reset();
        if (!r.dry) {
          tile_gather(b.xs, b.xt, b.ysd, b.xsd, k.xs.data(), ny, nx, k.H, k.W, k.th, k.tw, k0, nb, r.st);
          rows_gather(b.ss + (size_t)i * k.B * unet->ss_total, b.ssc, nb, unet->ss_total, k0, per, r.st);
        }
        unet->forward(r, b.xt, b.mut + (size_t)k0 * tn, nb, k.th, k.tw, b.ssc,
                      c.has_ic ? b.cct + (size_t)k0 * unet->cc_total : nullptr, b.out, b.ldo);
        if (!r.dry) unet_out<T>(b.out, b.ldo, b.epst + (size_t)k0 * tn, nb, k.th, k.tw, Hp, Wp, r.st);
      }
      if (!r.dry) {
        tile_blend(b.epst, b.eps, b.ysd, b.xsd, k.xs.data(), k.B, ny, nx, k.H, k.W, k.th, k.tw, k.ov, r.st);
        // The flat fp32 sampler update on the full image (eps is NCHW: ld = 0).
        sde_step<float>(c.mode, b.xs, b.mus, b.eps, 0, 1, 1, c.has_noise ? b.noise + (size_t)i * c.n : nullptr,
                        b.seed, (uint32_t)t, sched.coef(t, c.mode), 1, 1, (int)(c.n / 3), r.st);
      }
    }
  }
  void sde_reverse_tiled(int mode, float* x, const float* mu, const float* tc, const float* icx, int B,
                         int H, int W, const TileGrid& g, int tpf, int nT, const float* noise,
                         uint64_t seed, hipStream_t st) override {
    const LoopCall c = loop_call(mode, x, mu, tc, icx, B, H, W, nT, noise, seed, st, tpf);
    if (prof.on())
      throw Error(DAC_E_STATE, "the tiled loop has no profiling mode (disable profiling first)");
    HIP_OK(hipSetDevice(dev));
    const int NT = B * (int)g.ys.size() * (int)g.xs.size();
    const int C = std::min(tpf, NT);
    // One forward of a full chunk and one of the ragged last chunk.
    ensure_arena(plan(B, nT, c.has_ic, {{C, g.th, g.tw}, {NT % C, g.th, g.tw}}));
    const TKey key{B, H, W, g.th, g.tw, g.ov, C, nT, g.ys, g.xs};
    TLoop& L = get_tloop(key);
    stage(L, c);
    auto it = L.graphs.find(c.mkey);
    if (it == L.graphs.end() && !no_graph()) {
      Run r = live(priv);
      hipGraph_t gr = capture([&] { record_tiled(r, L, key, c); });
      size_t nn = 0;
      hipError_t e = hipGraphGetNodes(gr, nullptr, &nn);
      hipGraphExec_t ex = nullptr;
      if (e == hipSuccess && nn <= tiled_max_nodes(kMaxGraphNodes)) e = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
      (void)hipGraphDestroy(gr);
      HIP_OK(e);
      it = L.graphs.emplace(c.mkey, ex).first;
    }
    if (it != L.graphs.end() && it->second) {
      HIP_OK(hipGraphLaunch(it->second, priv));
    } else {
      Run r = live(priv);
      record_tiled(r, L, key, c);
    }
    finish(L, c);
  }

  // One profiled restore (profiler.h): a dry count of the launches of the profiled class(es),
  // events or stamp slots for them, then the live recording.
  // Eager pass: HIP cannot report elapsed time between events recorded by graph nodes
  // (hipEventElapsedTime -> invalid handle), so the launch sequence runs eagerly on the loop's
  // stream with an event pair around every timed launch; event pairs time one stream, so there
  // are no side streams (nor in the dry count).
  // Stamped pass: the loop is recorded and captured exactly as the timed graph (same arena,
  // side-stream branches, kernels and grids), every timed launch writing its own wall-clock
  // stamps; one replay, bracketed by HIP events on the loop's stream, gives every launch's
  // in-graph duration, and the captured graph's kernel nodes name each launch's kernel symbol.
  void profile_pass(Bufs& b, const LoopCall& c) {
    const bool graph = prof.stamps;
    Arena da;
    Run d = dry(da, graph, &prof, zero_page);
    prof.begin_pass(Pass::counting);
    record_loop(d, b, c);
    prof.prepare(priv);
    Run r = live(priv);
    r.prof = &prof;
    if (graph) return profile_graph(r, b, c);
    for (int k = 0; k < Run::kSide; ++k) r.side[k] = nullptr;
    record_loop(r, b, c);
    prof.check_complete();
  }
  void profile_graph(Run& r, Bufs& b, const LoopCall& c) {
    hipGraph_t g = capture([&] { record_loop(r, b, c); });
    hipGraphExec_t ex = nullptr;
    try {
      prof.check_complete();
      prof.name_symbols(g, priv);
      HIP_OK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
      prof.finish_stamps(ex, priv, dev);
    } catch (...) {
      (void)hipGraphDestroy(g);
      if (ex) (void)hipGraphExecDestroy(ex);
      throw;
    }
    (void)hipGraphDestroy(g);
    HIP_OK(hipGraphExecDestroy(ex));
  }

  void invalidate_graphs() override { clear_graphs(); }
  void set_noise_offset(uint64_t first_image) override { noise_offset = first_image; }

  double unet_flops(int B, int H, int W) override {
    Arena a;
    Run r = dry(a);
    unet->forward(r, nullptr, nullptr, B, H, W, nullptr, (const float*)1, nullptr, 4);
    return r.flops;
  }
  double encode_flops(int B) override {
    Arena a;
    Run r = dry(a);
    vit->encode(r, nullptr, B, nullptr, nullptr, true);
    return r.flops;
  }

  static void need(bool c, const char* m) {
    if (!c) throw Error(DAC_E_ARG, m);
  }

  int dev;
  dac_config cfg;
  bool fp8 = false;              // DAC_FP8 handle: e4m3 weights + conv8 for eligible layers
  bool ready = false;
  DevPool pool;
  std::unique_ptr<UNetNet<T>> unet;
  std::unique_ptr<VitNet<T>> vit;
  Arena arena;
  hipStream_t priv;
  hipStream_t side[Run::kSide];  // the other branches of the UNet's split section
  hipEvent_t ev_in, ev_out, ev_fork, ev_join[Run::kSide];
  uint64_t noise_offset = 0;     // global index of image 0 (sharded runs)
  void* zero_page = nullptr;
};

std::unique_ptr<Engine> make_engine(int device, int dtype, const dac_config& cfg) {
  if (dtype == DAC_F32) return std::make_unique<EngineT<float>>(device, cfg);
  if (dtype == DAC_BF16) return std::make_unique<EngineT<bf16>>(device, cfg);
  // fp8 handles: the e4m3 layers inside bf16 networks (measured 2.5 % faster than the same
  // handles on an fp16 base, B = 16: 30.08 / 29.83 against 29.17 / 29.32 images/s);
  // DAC_FP8_BASE=f16 runs every non-e4m3 layer in IEEE half instead.
  if (dtype == DAC_FP8) {
    if (fp8_base_f16()) return std::make_unique<EngineT<f16>>(device, cfg, true);
    return std::make_unique<EngineT<bf16>>(device, cfg, true);
  }
  if (dtype == DAC_F16) return std::make_unique<EngineT<f16>>(device, cfg);
  throw Error(DAC_E_ARG, "dtype must be DAC_F32, DAC_BF16, DAC_FP8 or DAC_F16");
}

template void conv_call<float>(Run&, const ConvW&, const void*, int, int, const void*, int, int,
                               int, int, int, int, int, void*, int, const Epi&);
template void conv_call<bf16>(Run&, const ConvW&, const void*, int, int, const void*, int, int,
                              int, int, int, int, int, void*, int, const Epi&);
template void conv_call<f16>(Run&, const ConvW&, const void*, int, int, const void*, int, int,
                             int, int, int, int, int, void*, int, const Epi&);

}  // namespace dac
