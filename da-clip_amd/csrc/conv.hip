// conv.hip — tap-shape switch of the implicit-GEMM conv; kernels live in conv_impl.h and are
// instantiated in conv_k3.hip / conv_k1.hip / conv_kx.hip.
#include "common.h"
#include "kernels.h"
#include "conv_epi.h"

namespace dac {

const ConvKnobs& conv_launch_knobs() {
  static const bool asked = [] {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu >= 8)
      conv_knobs().ncu = ncu;
    return true;
  }();
  (void)asked;
  return conv_knobs();
}

template <typename T, int KH, int KW, int S, int P>
void conv_dispatch(const ConvArgs& a, hipStream_t st);

// The engine's questions, each one look at the plan (conv_plan.h) for the hypothetical arguments.
static ConvPlan plan_of(const ConvArgs& a, int kh, int elem_bytes, int ask = 0) {
  const int s = kh == 4 ? 2 : kh > 7 ? kh : 1, p = kh == 3 || kh == 4 ? 1 : kh == 7 ? 3 : 0;
  return conv_plan(a, kh, kh, s, p, elem_bytes, conv_knobs(), ask);
}
// Profiler class of the launch conv<T>() would make; used to label timed launches:
// 0/1/2 = v1 256x16 / 256x64 / 128x128, 3/4/5 = v2 256x64 / 256x128 / 128x128,
// 6/7 = v3 (row-halo 3x3, 64-byte rows, 4 waves) 128x64 / 128x128, 10/11 = v3 (128-byte rows,
// 8 waves) 256x64 / 128x128, 12 = v4 (3x3 interleaved-row tiles) 256-pixel tiles, 13 = v2 7x7
// row-tap layout (Cin = 8), 14 = v4 256x16 (narrow Cout), 20 = v4 128-pixel tiles, 21 = v5
// weight-stationary 3x3 (64 -> 64), 22 / 23 = conv_edge.hip init_conv / final_conv, 24 =
// conv_down.hip, 26 = v4 row-phase upsample conv (ConvArgs::uph; labelled by the engine), 27 =
// conv3r. The 1x1 GEMMs are classed by shape, whichever tile the knobs give it: 8 = one K tile,
// 18 = Cout <= 64, 15 = GEGLU, 16 = Cout >= 1024 with the minimal epilogue, 17 = the rest. A fused
// res_conv on 128-pixel tiles and a split-K launch keep the class of the plain launch. -1: none.
int conv_variant(const ConvArgs& a, int kh, int elem_bytes) { return plan_of(a, kh, elem_bytes).label; }
bool conv_res_fusable(const ConvArgs& a) { return a.y2 && plan_of(a, 3, 2).kind != CONV_NONE; }
bool conv_lnf_ok(const ConvArgs& a, int elem_bytes) { return plan_of(a, 1, elem_bytes, ASK_LNF).kind != CONV_NONE; }
bool conv_gna_ok(const ConvArgs& a, int elem_bytes) { return plan_of(a, 1, elem_bytes, ASK_GNA).kind != CONV_NONE; }
bool conv_q8out_ok(const ConvArgs& a) { return plan_of(a, 3, 2, ASK_YS8).kind != CONV_NONE; }
bool conv_uph_ok(const ConvArgs& a, int elem_bytes) { return a.uph && plan_of(a, 3, elem_bytes).kind != CONV_NONE; }

// Split-K for 1x1 GEMMs whose 64x128 tile grid covers under half the CUs (the ViT and text
// tower linears at M = B x L rows): enough K splits to fill the chip, each with >= 4 K tiles.
// The split count is a function of `rows` = ONE image's rows (L), never of the batch: the
// partial sums' order then does not depend on what else is in the batch, so an image's result
// is bit-identical in any batch / shard. 0 = no split. Plain epilogues only (no row LayerNorm,
// folds, GEGLU or per-image weights).
int conv_split_k(const ConvArgs& a, int elem_bytes, long rows) {
  ConvArgs q = a;
  q.ksplit = 2;
  if (!conv_knobs().splitk || rows <= 0 || plan_of(q, 1, elem_bytes).kind != CONV_2_SPLIT) return 0;
  const long tiles = ((rows + 63) / 64) * ((a.Cout + 127) / 128);
  const int nk = a.K / (128 / elem_bytes);
  if (tiles >= 128 || nk < 8) return 0;
  int s = (int)((256 + tiles - 1) / tiles);
  s = s > nk / 4 ? nk / 4 : s;
  s = s > 8 ? 8 : s;
  return s >= 2 ? s : 0;
}

bool conv3_split_ok(const ConvArgs& a, int elem_bytes) {
  ConvArgs q = a;
  q.ksplit = 2;
  return plan_of(q, 3, elem_bytes).kind == CONV_3_SPLIT;
}
int conv3_split_k(const ConvArgs& a, int elem_bytes, int ks) {
  if (ks < 2 || !conv3_split_ok(a, elem_bytes)) return 0;
  const int nchunk = a.Cin / (128 / elem_bytes);
  while (ks > 1 && nchunk / ks < 2) --ks;
  return ks >= 2 ? ks : 0;
}

template <typename T>
__global__ void __launch_bounds__(256) conv_part_reduce_kernel(ConvArgs a, int M, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % a.Cout);
  const int m = (int)(i / a.Cout);
  float v = 0.f;
  for (int z = 0; z < a.ksplit; ++z) v += a.part[((size_t)z * M + m) * a.Cout + c];
  const int HWo = a.Ho * a.Wo, b = m / HWo;
  // The register epilogues' fast path: bias folded into the shift, SiLU in the log2 domain.
  float s = 1.f, h = 0.f;
  if (a.ss) { s += a.ss[(size_t)b * a.ss_ld + c]; h = a.ss[(size_t)b * a.ss_ld + a.Cout + c]; }
  const bool silu = a.act == ACT_SILU;
  epi_fold(a.bias ? a.bias[c] : 0.f, s, h, silu);
  v = fmaf(v, s, h);
  if (silu) v = silu_log2(v);
  else if (a.act == ACT_GELU) v = gelu_fast(v);
  if (a.res1) v += to_f(reinterpret_cast<const T*>(a.res1)[(size_t)m * a.ldr1 + c]);
  if (a.res2) v += to_f(reinterpret_cast<const T*>(a.res2)[(size_t)m * a.ldr2 + c]);
  if (a.bbias) v += a.bbias[(size_t)b * a.bb_ld + c];
  reinterpret_cast<T*>(a.y)[(size_t)m * a.ldy + c] = from_f<T>(v);
}

template <typename T>
void conv_part_reduce(const ConvArgs& a, hipStream_t st) {
  const int M = a.B * a.Ho * a.Wo;
  const size_t n = (size_t)M * a.Cout;
  conv_part_reduce_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(a, M, n);
}
template void conv_part_reduce<float>(const ConvArgs&, hipStream_t);
template void conv_part_reduce<bf16>(const ConvArgs&, hipStream_t);
template void conv_part_reduce<f16>(const ConvArgs&, hipStream_t);

template <typename T>
void conv(const ConvArgs& a, int kh, int kw, int s, int p, hipStream_t st) {
  if (a.xs8) throw std::invalid_argument("conv: e4m3 inputs are conv3q-only");
  if (kh == 3 && kw == 3 && s == 1 && p == 1) conv_dispatch<T, 3, 3, 1, 1>(a, st);
  else if (kh == 1 && kw == 1 && s == 1 && p == 0) conv_dispatch<T, 1, 1, 1, 0>(a, st);
  else if (kh == 4 && kw == 4 && s == 2 && p == 1) conv_dispatch<T, 4, 4, 2, 1>(a, st);
  else if (kh == 7 && kw == 7 && s == 1 && p == 3) conv_dispatch<T, 7, 7, 1, 3>(a, st);
  else if (kh == 32 && kw == 32 && s == 32 && p == 0) conv_dispatch<T, 32, 32, 32, 0>(a, st);
  else if (kh == 14 && kw == 14 && s == 14 && p == 0) conv_dispatch<T, 14, 14, 14, 0>(a, st);
  else throw std::invalid_argument("conv: unsupported kernel/stride/padding");
}

template void conv<float>(const ConvArgs&, int, int, int, int, hipStream_t);
template void conv<bf16>(const ConvArgs&, int, int, int, int, hipStream_t);
template void conv<f16>(const ConvArgs&, int, int, int, int, hipStream_t);

}  // namespace dac
