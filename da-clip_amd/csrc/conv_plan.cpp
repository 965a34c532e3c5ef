// conv_plan.cpp — the conv kernel selection (conv_plan.h). Host code only.
#include "conv_plan.h"

#include <cstdlib>

namespace dac {

ConvKnobs conv_knobs_from_env() {
  ConvKnobs k;
  auto env = [](const char* n, int& v) { if (const char* e = getenv(n)) v = atoi(e); };
  env("DAC_CONV2_FORCE32", k.conv2_force32);
  env("DAC_CONV3_BUF", k.conv3_buf);
  env("DAC_C3I_ST", k.c3i_st);
  env("DAC_GEGLU_SW", k.geglu_sw);
  env("DAC_C3W_BUF", k.c3w_buf);
  env("DAC_SPLITK", k.splitk);
  return k;
}
ConvKnobs& conv_knobs() {
  static ConvKnobs k = conv_knobs_from_env();
  return k;
}
extern "C" void dac_c3i_st(int v) { conv_knobs().c3i_st = v; }
extern "C" void dac_conv3_force(int v) { conv_knobs().conv3_force = v; }
extern "C" void dac_conv2_force(int v) { conv_knobs().conv2_force = v; }

const char* conv_kind_name(ConvKind k) {
  static const char* const n[] = {"none", "conv7", "conv3n", "conv_down", "conv3r", "conv3w", "conv3i", "conv3",
                                  "conv3_split", "conv2", "conv2_split", "conv1"};
  return n[k];
}

int conv3_rw(const ConvArgs& a, int BM) {
  const int Wo = a.Wo, Ho = a.Ho;
  if (Wo <= 0 || (Wo & (Wo - 1))) return Wo % BM == 0 ? BM : 0;
  const int RW = Wo < BM ? Wo : BM;
  if (RW < 16 || Ho % (BM / RW)) return 0;
  return RW;
}

static bool one_pitch(const ConvArgs& a) { return a.C1 >= a.Cin || !a.x2 || a.ld2 == a.ld1; }
static size_t src_bytes(const ConvArgs& a, int ld, int es) { return (size_t)a.B * a.Hs * a.Ws * ld * es; }
bool conv3_buf_fit(const ConvArgs& a, int es) {
  const size_t LIM = (size_t)1 << 30;
  return one_pitch(a) && src_bytes(a, a.ld1, es) < LIM && (size_t)a.Cout * a.K * es < LIM;
}
bool conv3w_buf_fit(const ConvArgs& a) {
  return one_pitch(a) && src_bytes(a, a.ld1, 2) + a.ld1 * 2 < ((size_t)1 << 31);
}
bool conv2_buf_fit(const ConvArgs& a, int es) {
  const size_t LIM = (size_t)1 << 31;
  return one_pitch(a) && !a.up && src_bytes(a, a.ld1, es) < LIM && (!a.x2 || src_bytes(a, a.ld2, es) < LIM) &&
         (size_t)a.Cout * a.K * es < LIM;
}

// Swapped tiles DMA the scale / shift / bias rows in 16-byte pieces.
static bool terms16(const ConvArgs& a) {
  return !((a.ss && (a.ss_ld % 4 || a.Cout % 4 || ((uintptr_t)a.ss & 15))) || ((uintptr_t)a.bias & 15));
}
static bool act_min(const ConvArgs& a) { return a.act == ACT_NONE || a.act == ACT_SILU; }
// 16-byte output / residual rows (the register and EPI_MIN epilogues).
static bool rows16(const ConvArgs& a, int es) {
  const int VE = 16 / es;
  return a.Cout % VE == 0 && a.ldy % VE == 0 && (!a.res1 || a.ldr1 % VE == 0) && (!a.res2 || a.ldr2 % VE == 0);
}

bool conv3i_fit(const ConvArgs& a, int es, int BM, int WGM, int CK, int fl) {
  const int WTM = BM / WGM, BKE = CK / es;
  const int RW = conv3_rw(a, BM);
  if (RW <= 0 || RW % WTM || a.Cin % BKE || (a.C1 < a.Cin && a.C1 % BKE)) return false;
  if ((fl & C3I_BUF) && !conv3_buf_fit(a, es)) return false;
  if ((fl & C3I_RES) && (!a.y2 || !a.w2)) return false;    // fused res_conv writes y2 from w2
  if (fl & C3I_UPH) {                                       // row-phase upsample tiles: one parity per tile
    if (!a.up || !a.uph || a.Ho % (2 * (BM / RW))) return false;
    // column-phase too: uph == 2, K = 16 Cin, rows of >= 128 output pixels
    if (((fl & C3I_UPC) != 0) != (a.uph == 2)) return false;
    if ((fl & C3I_UPC) && RW < 128) return false;
  } else if (a.uph) {
    return false;
  }
  return !(fl & C3I_SWAP) || terms16(a);
}

// 1x1, 16-bit, whole 16-byte rows, 64x128 swapped tiles inside one image; no GEGLU (the tile
// that folded it is gone).
bool conv2_lnf_fit(const ConvArgs& a) {
  if (a.cwrap || a.up || (a.x2 && a.C1 < a.Cin)) return false;
  return a.act != ACT_GEGLU && act_min(a) && rows16(a, 2) && (a.w_bstride > 0 || (a.Ho * a.Wo) % 64 == 0) &&
         a.Cout % 128 == 0;
}
// 1x1, 16-bit, 64x128 swapped tiles inside one image, groups of whole 16-byte vectors (the
// groupnorm_stats layout), Cin <= 512.
bool conv2_gna_fit(const ConvArgs& a) {
  if (a.cwrap || a.up || a.x2 || a.w_bstride || a.Cin > 512 || a.Cin != a.K) return false;
  // gna_groups >= 4: the statistics merge reduces tpg = 256 / groups lanes with an xor tree
  // inside one wave (conv_impl.h), so a group may not span two waves.
  if (a.gna_groups < 4 || a.gna_groups > 64 || (a.gna_groups & (a.gna_groups - 1))) return false;
  if (a.Cin % a.gna_groups || (a.Cin / a.gna_groups) % 8 || 256 % (a.Cin / 8)) return false;
  return act_min(a) && rows16(a, 2) && (a.Ho * a.Wo) % 64 == 0 && a.Cout % 128 == 0;
}
// 3x3 split-K on v3's 128x128 form: plain epilogues (bias, scale/shift, SiLU, residuals).
static bool conv3_split_fit(const ConvArgs& a, int es) {
  const int BKE = 128 / es;
  if (a.w2 || a.up || a.cwrap || a.w_bstride || a.amode || !act_min(a)) return false;
  if (a.Cin % BKE || !rows16(a, es) || a.Cout <= 16) return false;
  if (a.Ho != a.Hs || a.Wo != a.Ws || a.K != 9 * a.Cin || (a.x2 && a.C1 % BKE)) return false;
  return conv3_rw(a, 128) > 0 && conv3_rw(a, 256) > 0;
}

int conv_requests(const ConvArgs& a) {
  return (a.y2 ? ASK_Y2 : 0) | (a.ys8 ? ASK_YS8 : 0) | (a.lnf_cs ? ASK_LNF : 0) | (a.gna_stats ? ASK_GNA : 0) |
         (a.uph ? 16 : 0) | (a.ln_g ? 32 : 0) | (a.ksplit > 1 ? 64 : 0);
}
int conv_plan_serves(const ConvPlan& p) {
  switch (p.kind) {
    case CONV_3R: return ASK_Y2;
    case CONV_3W: return p.epi == C3I_Q8 ? ASK_YS8 : 0;
    case CONV_3I: return ((p.fl & C3I_RES) ? ASK_Y2 : 0) | ((p.fl & C3I_Q8) ? ASK_YS8 : 0) | ((p.fl & C3I_UPH) ? 16 : 0);
    case CONV_2: return ((p.epi & EPI_LNF) ? ASK_LNF : 0) | ((p.epi & EPI_GNA) ? ASK_GNA : 0) | ((p.epi & EPI_LN) ? 32 : 0);
    case CONV_3_SPLIT: case CONV_2_SPLIT: return 64;
    default: return 0;
  }
}

namespace {

ConvPlan none(const char* why) {
  ConvPlan p;
  p.why_not = why;
  return p;
}
ConvPlan tile(ConvKind kind, int BM, int BN, int WGM, int WGN, int CK, int ST, int epi, unsigned gx, unsigned gy,
              unsigned gz) {
  ConvPlan p;
  p.kind = kind; p.BM = BM; p.BN = BN; p.WGM = WGM; p.WGN = WGN; p.CK = CK; p.ST = ST; p.epi = epi;
  p.gx = gx; p.gy = gy; p.gz = gz; p.threads = 64 * WGM * WGN;
  return p;
}
ConvPlan own(ConvKind kind) {       // kernels whose launcher sizes its own (persistent) grid
  ConvPlan p;
  p.kind = kind;
  return p;
}

// conv3i configurations of the convbench force codes (ConvKnobs::conv3_force): BM BN WGM WGN ST FL;
// those with swapped operands (FL bit 3) are 16-bit only and need whole 64-channel N tiles.
struct C3ICfg { int code, BM, BN, WGM, WGN, ST, fl; };
constexpr C3ICfg kC3IForce[] = {
    {2, 256, 64, 4, 1, 2, 0},    {4, 128, 128, 2, 2, 2, 0},   {11, 256, 64, 4, 1, 2, 1},   {12, 256, 64, 4, 1, 2, 2},
    {13, 256, 64, 4, 1, 2, 3},   {14, 256, 128, 4, 2, 2, 1},  {15, 256, 128, 4, 2, 2, 3},  {16, 256, 64, 4, 1, 3, 1},
    {17, 256, 64, 4, 1, 2, 5},   {19, 64, 128, 2, 2, 2, 4},   {20, 128, 64, 4, 1, 2, 4},   {22, 64, 64, 2, 1, 2, 4},
    {18, 256, 64, 4, 1, 2, 4},   {8, 128, 128, 4, 2, 3, 3},   {9, 128, 128, 4, 2, 2, 3},   {10, 128, 64, 4, 1, 2, 3},
    {40, 256, 64, 4, 1, 2, 12},  {41, 128, 64, 4, 1, 2, 12},  {48, 256, 64, 4, 1, 2, 12 | C3I_BUF},
    {49, 128, 64, 4, 1, 2, 12 | C3I_BUF},
};

struct Sel {
  const ConvArgs& a;
  const int kh, es, req;
  const ConvKnobs& k;
  const bool h;                 // 16-bit element type
  const int M, Mg;
  const unsigned gz;
  const bool batched;

  bool c3i(ConvPlan& out, int BM, int BN, int WGM, int WGN, int ST, int fl, int epi = EPI_MIN) const {
    if ((fl & C3I_SWAP) && (!h || a.Cout % 64)) return false;
    if (!conv3i_fit(a, es, BM, WGM, 64, fl)) return false;
    out = tile(CONV_3I, BM, BN, WGM, WGN, 64, ST, epi, M / BM, (a.Cout + BN - 1) / BN, 1);
    out.fl = fl;
    out.buffer_dma = (fl & C3I_BUF) != 0;
    out.RW = conv3_rw(a, BM);
    return true;
  }
  ConvPlan c3(int BM, int BN, int WGM, int WGN, int CK, unsigned gzz = 1, ConvKind kind = CONV_3) const {
    ConvPlan p = tile(kind, BM, BN, WGM, WGN, CK, 2, EPI_MIN, M / BM, (a.Cout + BN - 1) / BN, gzz);
    p.RW = conv3_rw(a, BM);
    p.buffer_dma = k.conv3_buf && conv3_buf_fit(a, es);
    return p;
  }
  // Minimal epilogue when every tile lies inside one image (tile rows divide H*W, or the
  // per-image grid) and the tail is SiLU / none on 16-byte rows.
  bool minimal(int BM) const { return rows16(a, es) && act_min(a) && (batched || (a.Ho * a.Wo) % BM == 0); }
  ConvPlan c2(int BM, int BN, int WGM, int WGN, int ST, int epi) const {   // whole-N-tile kernels
    return tile(CONV_2, BM, BN, WGM, WGN, 128, ST, epi, (Mg + BM - 1) / BM, (a.Cout + BN - 1) / BN, gz);
  }
  ConvPlan c2any(int BM, int BN, int WGM, int WGN, int ST) const {
    return c2(BM, BN, WGM, WGN, ST, minimal(BM) ? EPI_MIN : EPI_ALL);
  }

  ConvPlan conv3x3() const;     // the v4 / v3 row-halo forms; kind NONE without a reason = not taken
  ConvPlan conv1x1_features(bool& taken) const;
  ConvPlan conv1x1_forced(int f2, bool& taken) const;
  ConvPlan v2() const;
  ConvPlan select() const;
};

ConvPlan Sel::conv3x3() const {
  ConvPlan p;
  if (k.conv3_force > 0) {
    for (const C3ICfg& c : kC3IForce)
      if (c.code == k.conv3_force && c3i(p, c.BM, c.BN, c.WGM, c.WGN, c.ST, c.fl)) return p;
  } else if (k.conv3_force < 0) {
    // v4: 256 x 64 tiles, 4 waves of 64x64, interleaved rows (measured 3-15 % faster than v3 at
    // every 3x3 shape of the UNet whose row width is a multiple of 64). 16-bit with whole
    // 64-channel tiles: swapped operands + register epilogue (FL bit 3), 4-9 % faster than the
    // LDS-staged epilogue at every v4 shape of the UNet. Buffer-resource DMA (FL bit 10) first;
    // the flat-address form takes what it rejects.
    const int bufs[2] = {C3I_BUF, 0};
    const int b0 = k.conv3_buf ? 0 : 1;
    if (h) {
      if (a.uph) {                                // row- (and column-) phase upsample conv
        const int f = 12 | C3I_UPH | (a.uph == 2 ? C3I_UPC : 0);
        if (a.K == (a.uph == 2 ? 16 : 12) * a.Cin && a.Cout % 64 == 0)
          for (int b = b0; b < 2; ++b) if (c3i(p, 256, 64, 4, 1, 2, f | bufs[b])) return p;
        return none("row-phase upsample conv without a matching v4 tile");
      }
      if (req & ASK_YS8) {                        // fp8 output: fused-res 256x64 tiles only
        if (a.y2 && a.Cout == 64)
          for (int b = b0; b < 2; ++b) if (c3i(p, 256, 64, 4, 1, 2, 12 | C3I_RES | C3I_Q8 | bufs[b])) return p;
        return none("fp8 output without a matching fused v4 tile");
      }
      if (a.y2) {
        for (int BM = 256; BM >= 128; BM -= 128)
          for (int b = b0; b < 2; ++b) if (c3i(p, BM, 64, 4, 1, 2, 12 | C3I_RES | bufs[b])) return p;
        return none("fused second output requested on a shape without a fusing kernel");
      }
    }
    // Rows of 32 (the 32x32 level), Cout <= 256: 128x64 tiles of 32-pixel wave tiles (TM = 2),
    // 8 % faster than v3 in the UNet; the 512-wide convs stay on v3 (v4 128x64 swapped tiles
    // measured 11 % faster in convbench but 3 % slower in the network).
    for (int BM = 256; BM >= 128; BM -= 128) {
      if (BM == 128 && a.Cout > 256) break;
      // Ring depth of the plain swapped tiles when the grid is at most one block per CU.
      const int st = (long)M / BM * ((a.Cout + 63) / 64) <= 256 ? k.c3i_st : 2;
      if (k.conv3_buf && (st == 3 || st == 4) && c3i(p, BM, 64, 4, 1, st, 12 | C3I_BUF)) return p;
      for (int b = b0; b < 2; ++b) if (c3i(p, BM, 64, 4, 1, 2, 12 | bufs[b])) return p;
      if (c3i(p, BM, 64, 4, 1, 2, 4)) return p;
    }
  }
  // v3. 64-byte K rows, 4 waves of 64x64 (or 64x32) wave tiles: two 24-36 KB stages, so 2-3
  // blocks share a CU and one block's LDS-DMA latency hides behind another's MFMAs (measured
  // 10-24 % faster than one 8-wave block with 128-byte rows). Small grids (< 2 blocks per CU,
  // the 32x32 level) keep the 8-wave block.
  const bool rw128 = conv3_rw(a, 128) > 0;
  if (a.Cout <= 64) return rw128 ? c3(128, 64, 2, 2, 64) : c3(256, 64, 4, 2, 128);
  if (rw128) {
    // Chosen from ONE image's tile count (64 = the batch-8 grid's 512): the two forms walk the
    // channels in different chunk orders (CK), so a batch-size-driven choice made an image's
    // result depend on its batch (B = 16 vs 1 at the 32x32 level). The 8-wave form as 4 x 2
    // waves of 32 x 64 (round 5: +0.3 % in the network against 2 x 4 waves of 64 x 32).
    return (long)(a.Ho * a.Wo / 128) * ((a.Cout + 127) / 128) >= 64 ? c3(128, 128, 2, 2, 64) : c3(128, 128, 4, 2, 128);
  }
  return p;
}

// Row LayerNorm / input GroupNorm / input LayerNorm fold: one kernel each, or none.
ConvPlan Sel::conv1x1_features(bool& taken) const {
  taken = true;
  if (a.ln_g) {   // one N tile must cover Cout exactly
    // One wave owns all 64 channels of its rows: the LN runs in registers.
    if (h && minimal(256) && a.Cout == 64 && !a.ss && a.act == ACT_NONE && !a.res2 && !a.bbias)
      return c2(256, 64, 4, 1, 2, EPI_SWAP | EPI_LN);
    if (minimal(256) && a.Cout == 64) return c2(256, 64, 4, 2, 3, EPI_LN);
    if (minimal(128) && a.Cout == 128) return c2(128, 128, 2, 2, 2, EPI_LN);
    return none("row LayerNorm epilogue on a shape without its kernel");
  }
  if (req & ASK_GNA)
    return h && conv2_gna_fit(a) ? c2(64, 128, 2, 2, 2, EPI_SWAP | EPI_GNA)
                                 : none("GroupNorm A path requested on a shape without such a kernel");
  if (req & ASK_LNF)
    return h && conv2_lnf_fit(a) ? c2(64, 128, 2, 2, 2, EPI_SWAP | EPI_LNF)
                                 : none("LN fold requested on a shape without a folding kernel");
  taken = false;
  return ConvPlan();
}

// The 1x1 configuration table (ConvKnobs::conv2_force / conv2_force32).
ConvPlan Sel::conv1x1_forced(int f2, bool& taken) const {
  taken = true;
  const bool sw = h && minimal(128) && a.Cout % 128 == 0;
  switch (f2) {
    case 1: return c2any(256, 128, 4, 2, 3);
    case 2: return c2any(128, 128, 2, 2, 2);
    case 3: return c2any(256, 128, 4, 2, 2);
    case 4: return c2any(128, 128, 2, 2, 3);
    case 5: return c2(256, 256, 4, 2, 2, EPI_MIN);
    case 6: return c2any(128, 256, 2, 4, 2);
    case 7: return c2any(128, 64, 2, 2, 2);
    case 8: return c2any(64, 128, 2, 2, 2);
    case 9: return c2any(64, 64, 2, 2, 3);
    case 10: return c2any(128, 64, 2, 2, 3);
    case 11: return c2any(64, 128, 2, 2, 3);
    case 12: return c2any(64, 128, 2, 2, 4);
    case 13: return h && minimal(64) && a.Cout % 128 == 0 ? c2(64, 128, 2, 2, 3, EPI_SWAP) : c2any(64, 128, 2, 2, 3);
    // Swapped tiles; 17-19 deep rings (in-flight depth probe): 64x128 x 6 stages, 128x128 x 4 / 5.
    case 14: return sw ? c2(128, 128, 2, 2, 2, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    case 15: return sw ? c2(128, 128, 2, 2, 3, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    case 16: return sw ? c2(64, 128, 2, 2, 4, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    case 17: return sw ? c2(64, 128, 2, 2, 6, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    case 18: return sw ? c2(128, 128, 2, 2, 4, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    case 19: return sw ? c2(128, 128, 2, 2, 5, EPI_SWAP) : c2any(64, 128, 2, 2, 2);
    default: taken = false; return ConvPlan();
  }
}

ConvPlan Sel::v2() const {
  const int BKE = 128 / es, HWo = a.Ho * a.Wo;
  if (kh == 1) {
    bool taken;
    ConvPlan p = conv1x1_features(taken);
    if (taken) return p;
    const int f2 = k.conv2_force32 > 0 && a.Ho > 1 && a.Wo > 1 && HWo <= 1024 && HWo >= 256 && a.ksplit <= 1 &&
                           a.act != ACT_GEGLU ? k.conv2_force32 : k.conv2_force;
    p = conv1x1_forced(f2, taken);
    if (taken) return p;
    if (a.ksplit > 1) {
      // Split-K: 64x128 tiles, grid z = ksplit, then the reduce + epilogue pass.
      if (batched || a.act == ACT_GEGLU || a.cwrap || a.up || a.Cin != a.K || a.Cout < 64)
        return none("1x1 split-K on a shape without it (plain GEMMs, Cout >= 64, shared weights)");
      return tile(CONV_2_SPLIT, 64, 128, 2, 2, 128, 2, EPI_PART, (Mg + 63) / 64, (a.Cout + 127) / 128, a.ksplit);
    }
    // One K tile (1x1 over 64 bf16 channels): no pipeline to fill, so a single small stage
    // (128x64, 4 waves) keeps several blocks resident per CU and their load latencies overlap
    // (measured best of 256x128 x {1,2,3} stages, 128x128, 128x64).
    if (a.K <= BKE) return c2any(128, 64, 2, 2, 1);
    // Measured (tools/convbench 1x1 sweep): Cout <= 64 (K > 64) 128x64 with 2 stages; GEGLU
    // projections below; wide plain outputs 256x256 (8 waves of 64x128, 2 stages, minimal
    // epilogue only: the general one spills at this tile); the rest 64x128 with 2 stages (4 waves
    // of 32x64), which doubles the blocks of the small 32x32-level GEMMs over 128x128.
    if (a.Cout <= 64) return c2any(128, 64, 2, 2, 2);
    if (a.act == ACT_GEGLU) {
      const bool bare = rows16(a, es) && !a.res1 && !a.res2 && !a.bbias;
      // Swapped tiles with the register GEGLU epilogue (weights in the w_gs order): no LDS
      // staging of the fp32 tile, 16-byte stores straight from the accumulators.
      if (h && a.w_gs && a.b_gs && bare && !a.ss && k.geglu_sw > 0) {
        const int cfg = k.conv2_force >= 20 && k.conv2_force <= 23 ? k.conv2_force - 19 : k.geglu_sw;
        const int BM = cfg == 1 || cfg == 3 ? 256 : 128, BN = cfg <= 2 ? 256 : 128;
        if (cfg >= 1 && cfg <= 4 && (batched || HWo % BM == 0) && a.Cout % BN == 0) {
          p = c2(BM, BN, BM / 64, BN / 64, 2, EPI_SWAP | EPI_GEGLU);
          p.w_gs = true;
          return p;
        }
      }
      // 256x256 tiles when they stay inside one image: half the LDS-DMA bytes per MFMA of the
      // 128x256 tiles, whose per-stage refill the MFMAs could not cover.
      if (h && bare && (batched || HWo % 256 == 0) && a.Cout % 256 == 0 && k.conv2_force == 0)
        return c2(256, 256, 4, 2, 2, EPI_GEGLU);
      return c2any(128, 256, 2, 4, 2);
    }
    if (a.Cout >= 1024 && minimal(256)) return c2(256, 256, 4, 2, 2, EPI_MIN);
    // 16-bit, whole tiles in one image, Cout a multiple of the tile: swapped operands + register
    // epilogue (no LDS round trip).
    if (h && minimal(64) && a.Cout % 128 == 0 && k.conv2_force == 0) return c2(64, 128, 2, 2, 2, EPI_SWAP);
    return c2any(64, 128, 2, 2, 2);
  }
  if (a.Cout <= 64) return c2any(256, 64, 4, 2, 3);
  if ((long)((Mg + 255) / 256) * ((a.Cout + 127) / 128) * gz >= 256) return c2any(256, 128, 4, 2, 3);
  return c2any(128, 128, 2, 2, 3);
}

ConvPlan Sel::select() const {
  const int BKE = 128 / es, f3 = k.conv3_force;
  if (a.xs8) return none("e4m3 inputs are conv3q-only");
  // A fused second output rides on conv3r or the 16-bit v4 swapped tiles only; an fp8 output on
  // conv3w or the fused 256x64 v4 tiles, 64 channels wide, nothing added after the activation.
  if (a.y2 && !(kh == 3 && h && f3 < 0 && a.w2 && a.ldy2 % 8 == 0 && !a.bias2 && a.Cout % 64 == 0 && !a.cwrap && terms16(a)))
    return none("fused second output requested on a shape without a fusing kernel");
  if ((req & ASK_YS8) && !(kh == 3 && h && f3 < 0 && a.Cout == 64 && a.ldy == 64 && !a.res1 && !a.res2 && !a.bbias))
    return none("fp8 output requested on a shape without such a kernel");
  // Tap shapes whose Cin is always a multiple of the K tile use v2; v1 serves the rest
  // (init conv Cin=8, patch embed, final conv Cout=3, LinearAttention to_out amode=1).
  const bool v2ok = (kh == 1 || kh == 3 || kh == 4) && a.Cin % BKE == 0 && a.amode == 0 && a.Cout > 16;
  if (kh == 3) {
    if (a.ksplit > 1) {
      if (!conv3_split_fit(a, es)) return none("3x3 split-K on a shape without it");
      return c3(128, 128, 4, 2, 128, a.ksplit, CONV_3_SPLIT);
    }
    if (h && f3 < 0 && conv3n_ok(a)) return own(CONV_3N);
    // Narrow output (the final conv, Cout = 3): v4 row-halo tiles with 16 output channels and
    // the general (scalar-capable) epilogue; the A operand dominates, and v4 reads each input
    // pixel once per kernel row instead of 9 times.
    ConvPlan p;
    if (a.Cout <= 16 && a.amode == 0 && a.w_bstride == 0 && f3 < 0 && act_min(a) && a.Cin % (64 / es) == 0 &&
        c3i(p, 256, 16, 4, 1, 2, 3, EPI_ALL))
      return p;
    if (h && (f3 < 0 || f3 == 70) && !(req & ASK_YS8) && conv3r_ok(a)) return own(CONV_3R);
    if (h && (f3 < 0 || (f3 >= 30 && f3 < 40)) && conv3w_ok(a)) {
      p = own(CONV_3W);
      p.delay = f3 >= 30 ? (f3 - 30) * 2 : 6;   // swept: 4-10 best
      p.buffer_dma = k.c3w_buf && conv3w_buf_fit(a);
      if (req & ASK_YS8) {
        if (!p.buffer_dma) return none("fp8 output needs conv3w's buffer-descriptor DMA form");
        p.epi = C3I_Q8;
      }
      p.gx = conv3w_blocks(a.B * a.Ho * (a.Wo >> 6), 8, k.ncu);   // 8 waves walking 64-pixel segments
      p.gy = p.gz = 1; p.threads = 512;
      return p;
    }
    // v4 / v3: the fast epilogue only (SiLU / none, 16-byte rows).
    if (v2ok && conv3_rw(a) > 0 && a.w_bstride == 0 && act_min(a) && rows16(a, es) && a.cwrap == 0) {
      p = conv3x3();
      if (p.kind != CONV_NONE || p.why_not) return p;
    }
  }
  if (kh == 4 && h && f3 < 0 && conv_down_ok(a)) return own(CONV_DOWN);
  if (kh == 7 && h) {
    if (conv7_ok(a)) return own(CONV_7);
    if (a.Cin == 8 && a.K == (a.cwrap ? 2 : 1) * 7 * 8 * 8 && a.amode == 0 && a.w_bstride == 0 && !a.x2)
      return tile(CONV_2, 256, 64, 4, 2, 128, 3, EPI_ALL, (M + 255) / 256, (a.Cout + 63) / 64, 1);
  }
  // cwrap = 1 here means the row-tap dual layout (kernel rows wrap), and K = 7 x 8 x Cin its
  // padded kernel rows; the generic loaders read a nonzero cwrap as a channel wrap and K as
  // [7][7][Cin], so no other kernel (of any element type) may take either.
  if (kh == 7 && (a.cwrap || a.K != 49 * a.Cin)) return none("7x7 row-tap layout without its kernel");
  if (v2ok) return v2();
  if (a.Cout <= 16 && a.act != ACT_GEGLU) return tile(CONV_1, 256, 16, 4, 1, 128, 1, EPI_ALL, (Mg + 255) / 256, (a.Cout + 15) / 16, gz);
  if (a.Cout <= 64) return tile(CONV_1, 256, 64, 4, 1, 128, 1, EPI_ALL, (Mg + 255) / 256, (a.Cout + 63) / 64, gz);
  return tile(CONV_1, 128, 128, 2, 2, 128, 1, EPI_ALL, (Mg + 127) / 128, (a.Cout + 127) / 128, gz);
}

// Profiler class (the numbers of conv_variant's comment in conv.hip). The 1x1 GEMMs are classed
// by shape, not by tile: the roofline keys on the class, and the tile of a shape class is tunable.
int label_of(const Sel& s, const ConvPlan& p) {
  const ConvArgs& a = s.a;
  switch (p.kind) {
    case CONV_7: return 22;
    case CONV_3N: return 23;
    case CONV_DOWN: return 24;
    case CONV_3R: return 27;
    case CONV_3W: return 21;
    case CONV_3I: return p.BN == 16 ? 14 : p.BM == 256 ? 12 : 20;
    case CONV_3: return p.CK == 64 ? (p.BN == 64 ? 6 : 7) : (p.BN == 64 ? 10 : 11);
    case CONV_1: return p.BN == 16 ? 0 : p.BN == 64 ? 1 : 2;
    case CONV_2: case CONV_2_SPLIT:
      if (s.kh == 7) return 13;
      if (s.kh != 1) return p.BN == 64 ? 3 : p.BM == 256 ? 4 : 5;
      if (a.K <= 128 / s.es) return 8;
      if (a.Cout <= 64) return 18;
      if (a.act == ACT_GEGLU) return 15;
      return a.Cout >= 1024 && s.minimal(256) ? 16 : 17;
    default: return -1;
  }
}

}  // namespace

ConvPlan conv_plan(const ConvArgs& a, int kh, int kw, int stride, int pad, int es, const ConvKnobs& k, int ask) {
  const int shapes[6][4] = {{3, 3, 1, 1}, {1, 1, 1, 0}, {4, 4, 2, 1}, {7, 7, 1, 3}, {32, 32, 32, 0}, {14, 14, 14, 0}};
  bool known = false;
  for (const auto& s : shapes) known |= kh == s[0] && kw == s[1] && stride == s[2] && pad == s[3];
  if (!known) return none("unsupported kernel/stride/padding");
  const bool batched = a.w_bstride > 0;
  const int M = a.B * a.Ho * a.Wo;
  const Sel s{a, kh, es, ask | conv_requests(a), k, es == 2, M, batched ? a.Ho * a.Wo : M, batched ? (unsigned)a.B : 1u, batched};
  ConvPlan p = s.select();
  if (p.kind == CONV_NONE) return p;
  // A request the chosen kernel would ignore is not served.
  if (s.req & ~conv_plan_serves(p)) return none("a requested output / fold / split is not served by the kernel for this shape");
  if (kh == 1) p.buffer_dma = k.conv3_buf && conv2_buf_fit(a, es);
  p.label = label_of(s, p);
  // A launch that carries an extra output or a K split keeps the class of the plain launch.
  if (p.kind == CONV_3_SPLIT || (p.kind == CONV_3I && (p.fl & C3I_RES) && p.BM == 128)) {
    ConvArgs q = a;
    q.ksplit = 0; q.y2 = nullptr; q.w2 = nullptr;
    p.label = conv_plan(q, kh, kw, stride, pad, es, k, ask).label;
  }
  return p;
}

}  // namespace dac
