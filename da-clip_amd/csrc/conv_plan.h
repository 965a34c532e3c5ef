// conv_plan.h — which conv kernel runs for a ConvArgs: one pure host function. conv_dispatch
// (conv_impl.h) executes the plan; the engine's predicates (conv.hip) and tools/convbench's
// `plan` mode ask it. No HIP call, no static state: everything tunable comes in as ConvKnobs.
#pragma once
#include "kernels.h"

namespace dac {

// Epilogue feature set compiled into a kernel (EPK bits). A kernel that can only meet the
// fast case (tile inside one image, SiLU / none, 16-byte aligned rows) compiles EPI_MIN and
// stays small: the epilogue runs once per block, and every path compiled into it costs
// instruction-cache fetches on that one pass.
enum : int { EPI_GENERAL = 1, EPI_GEGLU = 2, EPI_GELU = 4, EPI_SCALAR = 8, EPI_MIN = 0, EPI_ALL = 15,
             EPI_LN = 16, EPI_SWAP = 32,   // EPI_SWAP: swapped operands + epi_regs16 (conv_impl.h)
             EPI_LNF = 64,                 // input LayerNorm folded into a 1x1 GEMM (ConvArgs::lnf_cs)
             EPI_GNA = 128,                // input GroupNorm applied in the A path (ConvArgs::gna_stats)
             EPI_PART = 256 };             // split-K partial sums to ConvArgs::part (no epilogue)

// conv3i_kernel FL bits the selection reads (the kernel's own comment lists all of them).
enum : int { C3I_SWAP = 8, C3I_RES = 16, C3I_BUF = 1024, C3I_Q8 = 4096, C3I_UPH = 8192, C3I_UPC = 16384 };

// What is tunable about the selection (INTEGRATION.md lists the environment names).
struct ConvKnobs {
  int conv3_force = -1;   // convbench: -1 built-in choice, 0 v3 only, k > 0 conv3i configuration k,
                          // 30..39 conv3w with issue delay 2 (k - 30), 70 conv3r
  int conv2_force = 0;    // 1x1 configuration override (convbench; 20..23 = GEGLU forms 1..4), 0 = built-in
  // DAC_CONV2_FORCE32=k: 1x1 configuration k for the small-image plain GEMMs (256 <= Ho*Wo <= 1024:
  // the SpatialTransformer level; GEGLU projections and the LN / GroupNorm folds keep their tiles).
  // Default 18, swapped 128x128 tiles with a 4-stage ring: with the lowest levels split into two
  // half-batch branches it measured +0.6-0.8 % over the 64x128 tiles (four interleaved pairs,
  // DESIGN.md §9); 0 = the general dispatch.
  int conv2_force32 = 18;
  int conv3_buf = 1;      // DAC_CONV3_BUF: buffer-descriptor DMA of conv3i / conv3 / the 1x1 GEMMs
  // DAC_C3I_ST: ring depth (2 / 3 / 4) of the plain conv3i swapped tiles when the grid is at most
  // one block per CU (the 64x64 / 32x32 levels at B = 8): with no co-resident block to cover a
  // stage's DMA, deeper rings keep more of it in flight (3 measured best: 32x32 256->256 21.6 ->
  // 18.9 us, 64x64 128->128 18.2 -> 17.6 us in the network, +0.45 % images/s). The stage count only
  // buffers: every output is the same ordered sum, so the choice leaves results bit-identical.
  int c3i_st = 3;
  // DAC_GEGLU_SW: GEGLU projections on swapped tiles with the register epilogue: 0 off (the
  // 256x256 LDS-epilogue tile), 1 256x256 (16 waves), 2 128x256, 3 256x128, 4 128x128.
  int geglu_sw = 1;
  int c3w_buf = 1;        // DAC_C3W_BUF: buffer-descriptor DMA of conv3w
  int splitk = 1;         // DAC_SPLITK=0: no 1x1 split-K
  int ncu = 256;          // compute units (conv3w's persistent grid); conv_knobs() asks the device once
};
ConvKnobs conv_knobs_from_env();
// The process's instance: built from the environment at load, written by dac_conv3_force /
// dac_conv2_force / dac_c3i_st, CU count filled in at the first launch.
ConvKnobs& conv_knobs();
const ConvKnobs& conv_launch_knobs();   // conv.hip: conv_knobs() with this device's CU count
// Blocks of a persistent kernel whose waves each walk 1 / nwv of ntiles: at most one per CU, in
// whole XCD bands (conv3w, conv3q).
inline int conv3w_blocks(int ntiles, int nwv, int ncu) {
  int nb = (ntiles + nwv - 1) / nwv;
  if (nb > ncu) nb = ncu;
  return (nb + 7) / 8 * 8;
}

enum ConvKind : int {
  CONV_NONE = 0,      // no kernel serves these arguments: ConvPlan::why_not says why
  CONV_7,             // conv_edge.hip init_conv
  CONV_3N,            // conv_edge.hip final_conv
  CONV_DOWN,          // conv_down.hip
  CONV_3R,            // conv3r.hip register-stationary 64 -> 64
  CONV_3W,            // v5 weight-stationary 64 -> 64 (epi: 0, or C3I_Q8 for the fp8-output form)
  CONV_3I,            // v4 interleaved-row tiles (fl = FL bits, epi = EPK)
  CONV_3,             // v3 row-halo tiles
  CONV_3_SPLIT,       // v3 128x128 over ksplit Cin ranges + conv_part_reduce
  CONV_2,             // v2 (epi = EPK)
  CONV_2_SPLIT,       // v2 64x128 EPI_PART + conv_part_reduce
  CONV_1,             // v1 conv_kernel
};
const char* conv_kind_name(ConvKind k);

struct ConvPlan {
  ConvKind kind = CONV_NONE;
  int BM = 0, BN = 0, WGM = 0, WGN = 0, CK = 0, ST = 0;   // tile (conv3i / conv3 / conv2 / conv1)
  int fl = 0, epi = 0;        // conv3i FL bits; epilogue kind
  bool buffer_dma = false;    // buffer-descriptor LDS-DMA form (ConvArgs::dbuf for the 1x1 GEMMs)
  bool w_gs = false;          // conv2 GEGLU register epilogue: weights / bias in the w_gs order
  int RW = 0;                 // row width of a conv3i / conv3 tile
  unsigned gx = 0, gy = 0, gz = 0;
  int threads = 0;
  int delay = 0;              // conv3w issue delay
  int label = -1;             // profiler class (conv_variant)
  const char* why_not = nullptr;
};

// Requests beyond the ConvArgs fields that exist when the engine asks (a tensor it would only
// allocate on a yes): or-ed with the ones conv_requests() reads off the non-null pointers.
enum : int { ASK_Y2 = 1, ASK_YS8 = 2, ASK_LNF = 4, ASK_GNA = 8 };
int conv_requests(const ConvArgs& a);
// Which of the requests (ASK_*, plus uph / ln_g / ksplit as bits 16 / 32 / 64) the planned kernel serves.
int conv_plan_serves(const ConvPlan& p);

ConvPlan conv_plan(const ConvArgs& a, int kh, int kw, int stride, int pad, int elem_bytes, const ConvKnobs& k,
                   int ask = 0);

// Row width of a row-halo tile of BM pixels (conv3 / conv3i) for this output, or 0 if the shape
// does not tile: RW = min(Wo, BM) for power-of-two Wo >= 16 with Ho a multiple of BM / RW rows.
int conv3_rw(const ConvArgs& a, int BM = 256);

// Fit functions: the arguments one kernel family accepts (the plan calls them, the launcher
// asserts them).
bool conv3i_fit(const ConvArgs& a, int elem_bytes, int BM, int WGM, int CK, int fl);
bool conv2_lnf_fit(const ConvArgs& a);
bool conv2_gna_fit(const ConvArgs& a);
// Buffer-descriptor DMA limits, one per kernel family, each with its kernel's own bound.
bool conv3_buf_fit(const ConvArgs& a, int elem_bytes);    // conv3i and conv3: input and weights under 2^30 bytes
bool conv3w_buf_fit(const ConvArgs& a);                   // input + one pixel under 2^31 bytes
bool conv2_buf_fit(const ConvArgs& a, int elem_bytes);    // each source and the weights under 2^31 bytes

}  // namespace dac
