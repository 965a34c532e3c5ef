// pack.h — weight packing of libdaclip_hip: the number codecs, the 16-bit rounding and every
// layout the kernels read, as pure host functions from host arrays to host arrays. No HIP, no
// environment, no state: the storage type and the rounding mode are arguments. engine.cpp's
// Packer looks weights up, decides which forms a layer gets and uploads what these return;
// tools/convbench.cpp and the C ABI hook dac_op_pack (CPU tests) call the same functions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace dac {

// ----------------------------------------------------------------------------- codecs
// f32 -> bf16 / IEEE half: round to nearest even (half: subnormals kept, overflow to +-inf).
uint16_t f2bf_host(float f);
float bf2f_host(uint16_t h);
uint16_t f2h_host(float f);
float h2f_host(uint16_t h);
// f32 -> OCP e4m3 (e4m3fn: bias 7, max 448, no infinities): round to nearest even, saturating
// to +-448; NaN -> 0x7f.
uint8_t f2e4m3_host(float f);
float e4m3f_host(uint8_t b);

// Storage type of a packed weight.
enum class Store { f32, bf16, f16 };
uint16_t enc16(Store t, float f);      // t: bf16 or f16
float dec16(Store t, uint16_t h);

// ----------------------------------------------------------------------------- 16-bit rounding
// bf16 round-to-nearest leaves a per-layer systematic error (the same every step and pixel).
// keep_sums rounds each (output row, input channel) group of `taps` kernel taps so that its
// sum is kept (greedy flips of the taps closest to the rounding midpoint, each to its other
// 16-bit neighbour), which removes the error's response to smooth inputs.
enum class Round { rne, keep_sums };
// v: [rows][taps][cin]. taps < 2 is plain RNE.
std::vector<uint16_t> quantize16(const std::vector<float>& v, int taps, int cin, Store t, Round r);
// fp32 handles' precision probe: the values a 16-bit handle would store, kept in fp32. fp16:
// rounded to 11 significant bits (normals) instead of bf16 with rounding r.
std::vector<float> emulate16(const std::vector<float>& v, int taps, int cin, bool fp16, Round r);

// ----------------------------------------------------------------------------- knobs
// The packing switches of the environment, read once per handle:
//   DAC_WROUND      0 RNE, 1 (default) sum-keeping for bf16 only, 2 sum-keeping for bf16 and f16.
//                   fp16 keeps plain RNE by default: with an 11-bit significand the flips (up to
//                   1 ulp per tap) cost more texture-response accuracy than the DC error they
//                   remove (restoration fixture: dPSNR -1.3e-3 dB with sum-keeping, -1.2e-4 RNE).
//   DAC_WROUND_KEY  sum-keeping for the conv weights whose state-dict key contains this
//                   substring, whatever DAC_WROUND says for the rest (a per-layer probe).
//   DAC_UPH         upsample convs: 0 plain, 1 (default) row-phase weights, 2 also the row- and
//                   column-phase weights.
//   DAC_EMU_W, DAC_EMU_WSKIP, DAC_EMU_FP16   fp32 handles: role mask of the layers whose weights
//                   are rounded as a 16-bit handle's, key substrings (comma-separated) exempt
//                   from it, and f16 instead of bf16 rounding.
//   DAC_LA_QSHIFT   0: no softmax shift for the fused LinearAttention kernels.
struct PackKnobs {
  int wround = 1;
  std::string wround_key;
  int uph = 1;
  int emu_w = 0;
  std::string emu_wskip;
  bool emu_fp16 = false;
  bool la_qshift = true;
  // The 16-bit rounding of the weight stored under `key` in type t.
  Round round(Store t, const std::string& key) const;
  // key contains one of emu_wskip's substrings.
  bool emu_skips(const std::string& key) const;
};
PackKnobs pack_knobs_from_env();

// ----------------------------------------------------------------------------- layouts
// Conv weight [O][C][kh][kw] -> [O][kh][kws][cin] fp32, kws >= kw and cin >= C zero-filled (kws >
// kw: a kernel row padded to kws taps, so one K tile of kws * cin elements is one kernel row).
std::vector<float> pack_ohwi(const float* w, int O, int C, int kh, int kw, int kws, int cin);
// Split-precision weights: hi = enc(w), lo = enc(w - dec(hi)), packed [O][kh][kw][hi cin | lo cin]
// or, for the row-tap layout (kwp > kw), [O][hi rows | lo rows] of [kh][kwp][cin].
std::vector<uint16_t> pack_dual(const float* w, int O, int C, int kh, int kw, int kwp, int cin, Store t);
// Row-phase weights of a 3x3 conv applied after a 2x nearest upsample: output row 2i reads
// source rows (i-1 | i, i) and row 2i+1 (i, i | i+1), so the kernel rows of p [O][3][3][cin] fold
// to [O][4][3][cin] = (W0, W1+W2 | W0+W1, W2), summed in fp32.
std::vector<float> fold_row_phase(const std::vector<float>& p, int O, int cin);
// Columns fold the same way: [O][4 row sets][4 column sets][cin], set (b, t) of row set r = the
// sum of the kernel taps (kh, kw) with kh in rows(r), kw in cols(b, t); rows / cols: (0 | 1,2)
// for parity 0, (0,1 | 2) for parity 1.
std::vector<float> fold_rowcol_phase(const std::vector<float>& p, int O, int cin);
// GEGLU proj [2F][I]: the source row of each packed row. geglu_rows: each 32-row group holds 16
// "x" rows then their 16 "gate" rows (the conv epilogue pairs accumulator tiles j, j+1).
// geglu_gs_rows, the swapped-tile order (F % 32 == 0): row L of 64-row group G = L / 64, lane
// group lg = (L % 64) / 16, e = L % 16 is x (e < 8) or gate (e >= 8) of output channel
// 32 G + 8 lg + (e & 7).
std::vector<int> geglu_rows(int F);
std::vector<int> geglu_gs_rows(int F);
// out[r][:] = w[rows[r]][:] for rows of I values (I = 1: a bias).
std::vector<float> gather_rows(const float* w, const std::vector<int>& rows, int I);
// Row-concatenation of `parts` [O][I] blocks (q | k | v) stored back to back in w; the first
// block is multiplied by scale0 (q prescaled for the attention kernel's log2-domain softmax).
std::vector<float> concat_rows(const float* const* parts, int nparts, int O, int I, float scale0);
// [I][O] -> [O][I].
std::vector<float> transpose_io(const float* w, int I, int O);

// MX block-scaled e4m3 copies: bytes = e4m3(w / 2^e), one E8M0 exponent byte 127 + e per block,
// e the smallest with max |w| / 2^e <= 448 (0 for an all-zero block, clamped to +-126).
struct Mx8 {
  std::vector<uint8_t> w8, s8;
  int Kp = 0;
};
// p [O][K] -> w8 [O][Kp] (Kp = K up to a multiple of 128, zero-filled), s8 [O][Kp / 64] over
// 64-k blocks (127 for a block of padding only). conv8.hip.
Mx8 make_fp8(const std::vector<float>& p, int O, int K);
// p [64][3][3][64] -> w8 [64][9][64], s8 [64][9][2] (per output channel, tap, 32-channel half).
// conv3q.hip.
Mx8 make_q8c3(const std::vector<float>& p);
// The values make_fp8's operands stand for: [O][K] of e4m3f(w8) * 2^e.
std::vector<float> fp8_dequant(const Mx8& m, int O, int K);

// Input-LayerNorm fold of a packed [O][K] 1x1 weight p: w = p diag(g) stored in t (RNE), cs[n] =
// sum_k w[n][k] over the STORED (rounded) values, bias = pb + p beta (beta, pb may be null).
// LN(x) p^T + pb = rstd (x w^T - mean cs) + bias.
struct FoldedLN {
  std::vector<uint16_t> w;
  std::vector<float> cs, bias;
};
FoldedLN fold_ln(const std::vector<float>& p, int O, int K, const float* g, const float* beta, const float* pb,
                 Store t);
// LinearAttention's PreNorm gain folded into to_qkv: wg = pq diag(g) for pq [O][C], and the softmax
// shift of the fused kernels. |q_j| = |(Wq_j . g) . LN(x)| <= ||Wq_j . g|| sqrt(C) (||LN(x)|| <=
// sqrt(C)): with margin for the 16-bit operands, the largest over the first nq rows (q) is the
// shift when <= 40 (e^-80 is normal), else (or with qshift_on false) 0.
struct LaFold {
  std::vector<float> wg;
  float qshift = 0.f;
};
LaFold fold_la_gain(const std::vector<float>& pq, int O, int C, int nq, const float* g, bool qshift_on);

}  // namespace dac
