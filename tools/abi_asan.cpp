// abi_asan.cpp — argument-validation paths of the C ABI (include/daclip_hip.h) under a host
// AddressSanitizer build (SURVEY.md §5 "Race detection / sanitizers": a debug build with
// -fsanitize=address for host code). Built by `make -C da-clip_amd asan`: capi.cpp, pack.cpp and
// engine.cpp compiled with `-Xarch_host -fsanitize=address` (device code is not sanitized),
// linked with the normal kernel objects into this executable, so the ASan runtime comes with
// the binary (no preload). Every call below must return its documented DAC_E* code without a
// heap error or leak; with a GPU present it also walks a handle through the state machine
// (set_weight / finalize / forward errors) before destroying it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/daclip_hip.h"

static int g_fail = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

static dac_config small_unet() {
  dac_config c;
  std::memset(&c, 0, sizeof c);
  c.unet = 1;
  c.in_nc = 3;
  c.out_nc = 3;
  c.nf = 32;
  c.depth = 2;
  c.ch_mult[0] = 1;
  c.ch_mult[1] = 2;
  c.context_dim = 0;
  return c;
}

int main() {
  // Null handles and pointers: every entry point rejects them before touching memory.
  EXPECT(dac_create(0, DAC_F32, nullptr, nullptr) == DAC_E_ARG);
  dac_handle* h = reinterpret_cast<dac_handle*>(0x1);
  dac_config c = small_unet();
  EXPECT(dac_create(0, DAC_F32, &c, nullptr) == DAC_E_ARG);
  EXPECT(dac_set_weight(nullptr, "k", &c, nullptr, 0, DAC_SRC_F32) == DAC_E_ARG);
  EXPECT(dac_finalize_weights(nullptr) == DAC_E_ARG);
  EXPECT(dac_encode_image(nullptr, nullptr, 1, nullptr, nullptr, nullptr) == DAC_E_ARG);
  EXPECT(dac_unet_forward(nullptr, nullptr, nullptr, 1.f, nullptr, nullptr, 1, 8, 8, nullptr, nullptr) == DAC_E_ARG);
  EXPECT(dac_sde_reverse(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 1, 8, 8, 1, nullptr, 0, nullptr) == DAC_E_ARG);
  EXPECT(dac_profile_enable(nullptr, 0) == DAC_E_ARG);
  EXPECT(dac_unet_flops(nullptr, 1, 8, 8) < 0);
  EXPECT(std::strcmp(dac_last_error(nullptr), "null handle") == 0);
  EXPECT(dac_op_attention(nullptr, nullptr, 1, 64, 1, DAC_F32, 0, nullptr) == DAC_E_ARG);
  float dummy[4] = {0, 0, 0, 0};
  EXPECT(dac_op_attention(dummy, dummy, 1, 64, 1, 99, 0, nullptr) == DAC_E_ARG);      // bad dtype
  EXPECT(dac_op_attention(dummy, dummy, 1, 100, 1, DAC_F32, 2, nullptr) == DAC_E_ARG); // variant 2: fp32
  EXPECT(dac_op_attention(dummy, dummy, 1, 2048, 1, DAC_BF16, 3, nullptr) == DAC_E_ARG); // L > 1024
  // LinearAttention op hooks: null pointers, sizes, widths, dtypes, fp32 at C = 256 and negative
  // shifts / scales are refused before any device work.
  EXPECT(dac_op_linear_attention(nullptr, dummy, dummy, dummy, dummy, dummy, 1, 64, 64, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, nullptr, 1, 64, 64, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 0, 64, 64, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 1, 0, 64, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 1, 64, 96, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 1, 64, 256, DAC_F32, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 1, 64, 64, DAC_FP8, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention(dummy, dummy, dummy, dummy, dummy, dummy, 1, 64, 64, DAC_F16, -1.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention_weff(nullptr, dummy, dummy, 1, 64, 64, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention_weff(dummy, dummy, dummy, 1, 64, 32, DAC_BF16, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention_weff(dummy, dummy, dummy, 1, 64, 256, DAC_F32, 0.f, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_linear_attention_weff(dummy, dummy, dummy, 1, 64, 64, DAC_F16, -0.5f, nullptr) == DAC_E_ARG);
  // dac_op_conv: a null descriptor / input / weight, bad dtypes, windows and dimensions, a second
  // source that is missing, and arguments no kernel serves are refused before any device work;
  // with y == NULL a valid call only plans (no HIP call), so it runs here too.
  {
    dac_conv_desc cd;
    std::memset(&cd, 0, sizeof cd);
    cd.dtype = DAC_BF16; cd.kh = 1; cd.B = 2; cd.Hs = 8; cd.Ws = 8; cd.C1 = cd.Cin = cd.ld1 = 64;
    cd.Cout = cd.ldy = 128; cd.K = 64;
    cd.conv3_force = cd.conv2_force = cd.conv2_force32 = DAC_CONV_KEEP;
    int plan[DAC_CONV_PLAN_N] = {0};
    auto call = [&](const dac_conv_desc& q, const void* x1, const void* x2, const void* w, void* y) {
      return dac_op_conv(&q, x1, x2, w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, y, plan, nullptr);
    };
    EXPECT(dac_op_conv(nullptr, dummy, nullptr, dummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       dummy, plan, nullptr) == DAC_E_ARG);
    EXPECT(call(cd, nullptr, nullptr, dummy, dummy) == DAC_E_ARG);
    EXPECT(call(cd, dummy, nullptr, nullptr, dummy) == DAC_E_ARG);
    EXPECT(call(cd, dummy, nullptr, dummy, nullptr) == DAC_OK && plan[0] > 0 && plan[1] > 0);   // plan-only
    dac_conv_desc q = cd;
    q.dtype = DAC_FP8; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.dtype = 99; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.kh = 5; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.B = 0; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.Ws = -3; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.Cout = 0; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.Cin = 60; q.K = 60; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);   // not whole vectors
    q = cd; q.K = 128; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);              // K != kh kw Cin
    q = cd; q.ldy = 64; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);             // ldy < Cout
    q = cd; q.act = 7; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.ksplit = -1; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);
    q = cd; q.up = 1; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);               // up: 3x3 only
    q = cd; q.C1 = 32; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);              // C1 < Cin, no x2
    q = cd; q.C1 = 32; q.ld1 = 32; q.ld2 = 40; EXPECT(call(q, dummy, dummy, dummy, nullptr) == DAC_OK);
    q = cd; q.ksplit = 2; q.act = 3; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);  // no such kernel
    q = cd; q.kh = 7; q.C1 = q.Cin = q.ld1 = 8; q.K = 896; q.cwrap = 1; q.dtype = DAC_F32;
    EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);                                  // row-tap dual in fp32
    q = cd; q.kh = 4; q.Hs = 7; q.K = 16 * 64; EXPECT(call(q, dummy, nullptr, dummy, dummy) == DAC_E_ARG);   // odd input
    // dac_op_conv_ex: the fused second output and the phase forms; refusals before any device work,
    // plan-only calls (y == NULL) on valid arguments.
    dac_conv_desc c3 = cd;
    c3.kh = 3; c3.Hs = 4; c3.Ws = 256; c3.C1 = c3.Cin = c3.ld1 = 128; c3.Cout = c3.ldy = 64; c3.K = 9 * 128;
    dac_conv_ext ex = {0, 64};
    auto callx = [&](const dac_conv_desc& q, const dac_conv_ext* e, const void* w2, void* y2, void* y) {
      return dac_op_conv_ex(&q, e, dummy, nullptr, dummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            y, w2, y2, plan, nullptr);
    };
    EXPECT(dac_op_conv_ex(nullptr, &ex, dummy, nullptr, dummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, dummy, nullptr, nullptr, plan, nullptr) == DAC_E_ARG);
    EXPECT(callx(c3, nullptr, nullptr, nullptr, nullptr) == DAC_OK && plan[0] == 4);      // e == NULL: dac_op_conv (conv3r)
    EXPECT(callx(c3, &ex, dummy, dummy, nullptr) == DAC_OK && plan[0] == 4);              // conv3r with y2
    EXPECT(callx(c3, &ex, nullptr, dummy, dummy) == DAC_E_ARG);                           // y2 without w2
    EXPECT(callx(c3, &ex, dummy, nullptr, dummy) == DAC_E_ARG);                           // w2 without y2
    EXPECT(callx(c3, nullptr, dummy, dummy, dummy) == DAC_E_ARG);                         // y2 without its pitch
    ex.ldy2 = 63; EXPECT(callx(c3, &ex, dummy, dummy, dummy) == DAC_E_ARG);               // ldy2 < Cout
    ex.ldy2 = 64;
    q = c3; q.conv3_force = 0; EXPECT(callx(q, &ex, dummy, dummy, dummy) == DAC_E_ARG);   // v3 fuses nothing
    q = c3; q.dtype = DAC_F32; EXPECT(callx(q, &ex, dummy, dummy, dummy) == DAC_E_ARG);   // 16-bit only
    q = c3; q.kh = 1; q.K = 128; EXPECT(callx(q, &ex, dummy, dummy, dummy) == DAC_E_ARG); // 3x3 only
    q = c3; q.Hs = 8; q.Ws = 64; q.C1 = q.Cin = q.ld1 = 64; q.up = 1; q.K = 12 * 64;
    ex.uph = 1; EXPECT(callx(q, &ex, nullptr, nullptr, nullptr) == DAC_OK && plan[0] == 6 && (plan[5] & 8192));
    ex.uph = 2; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);              // K is the row layout's
    q.K = 16 * 64; EXPECT(callx(q, &ex, nullptr, nullptr, nullptr) == DAC_OK && (plan[5] & 16384));
    ex.uph = 3; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);
    ex.uph = -1; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);
    ex.uph = 0; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);              // K = 16 Cin without uph
    ex.uph = 2; q.up = 0; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);    // uph without up
    q.up = 1; q.dtype = DAC_F32; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG);   // no fp32 phase tile
    q.dtype = DAC_BF16; q.Ws = 32; EXPECT(callx(q, &ex, nullptr, nullptr, dummy) == DAC_E_ARG); // uph = 2: rows >= 128
    q.Ws = 64; EXPECT(callx(q, &ex, dummy, dummy, dummy) == DAC_E_ARG);                   // no phase tile fuses y2
  }
  // dac_op_rbfuse: the served-query (y == NULL) and the refusals, all before any device work.
  {
    alignas(16) static float ssb[4];
    dac_rb_desc rd = {DAC_BF16, 2, 3, 256, 64, 64, 64, 0, 128, 64};
    int geom[2] = {0, 0};
    auto rb = [&](const dac_rb_desc& q, const void* x1, const void* x2, const void* w1, const void* w2, const void* wr,
                  const float* ss, void* y) { return dac_op_rbfuse(&q, x1, x2, w1, w2, wr, ss, y, geom, nullptr); };
    EXPECT(rb(rd, dummy, nullptr, dummy, dummy, nullptr, ssb, nullptr) == 1 && geom[0] == 1 && geom[1] == 128);
    EXPECT(dac_op_rbfuse(nullptr, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy, geom, nullptr) == DAC_E_ARG);
    EXPECT(rb(rd, nullptr, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    EXPECT(rb(rd, dummy, nullptr, nullptr, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    EXPECT(rb(rd, dummy, nullptr, dummy, nullptr, nullptr, ssb, dummy) == DAC_E_ARG);
    EXPECT(rb(rd, dummy, nullptr, dummy, dummy, nullptr, nullptr, dummy) == DAC_E_ARG);
    EXPECT(rb(rd, dummy, nullptr, dummy, dummy, nullptr, ssb + 1, dummy) == DAC_E_ARG);   // ss alignment
    EXPECT(rb(rd, dummy, nullptr, dummy, dummy, dummy, ssb, dummy) == DAC_E_ARG);         // wr with Cin 64
    EXPECT(rb(rd, dummy, nullptr, dummy, dummy, dummy, ssb, nullptr) == 0);               // ... as a query
    dac_rb_desc q = rd;
    q.dtype = DAC_F32; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.B = 0; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.H = -1; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.W = 192; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, nullptr) == 0);
    q = rd; q.W = 320; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);   // strips of 128
    q = rd; q.ldy = 63; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.ldy = 68; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.ld1 = 56; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.ss_ld = -4; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.ss_ld = 130; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
    q = rd; q.Cin = 128; q.W = 320;
    EXPECT(rb(q, dummy, nullptr, dummy, dummy, dummy, ssb, dummy) == DAC_E_ARG);          // C1 < Cin, no x2
    q.ld2 = 56; EXPECT(rb(q, dummy, dummy, dummy, dummy, dummy, ssb, dummy) == DAC_E_ARG);
    q.ld2 = 96; EXPECT(rb(q, dummy, dummy, dummy, dummy, dummy, ssb, nullptr) == 1 && geom[0] == 1 && geom[1] == 64);
    EXPECT(rb(q, dummy, dummy, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);          // wr missing at Cin 128
    q.C1 = 32; q.ld1 = 32; EXPECT(rb(q, dummy, dummy, dummy, dummy, dummy, ssb, dummy) == DAC_E_ARG);   // 32 | 96
    q = rd; q.Cin = q.C1 = q.ld1 = 96; EXPECT(rb(q, dummy, nullptr, dummy, dummy, nullptr, ssb, dummy) == DAC_E_ARG);
  }
  // dac_op_pack (host only): every layout family writes into heap buffers of exactly the queried
  // sizes, and the refusals come before any buffer is touched.
  {
    std::vector<float> w(64 * 64 * 9), g(64, 1.25f), b(192, 0.5f);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 0.001f * (float)((int)(i * 37 % 1001) - 500);
    auto run = [&](dac_pack_desc d, const float* gain, const float* beta, const float* bias, int shrink = -1) {
      size_t need[3] = {0, 0, 0};
      int rc = dac_op_pack(&d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, need);
      if (rc != DAC_OK) return rc;
      std::vector<std::vector<unsigned char>> buf(3);
      void* out[3];
      size_t cap[3];
      for (int i = 0; i < 3; ++i) {
        cap[i] = need[i] - (i == shrink ? 1 : 0);
        buf[i].resize(cap[i]);
        out[i] = cap[i] ? buf[i].data() : nullptr;
      }
      return dac_op_pack(&d, w.data(), gain, beta, bias, out, cap, need);
    };
    dac_pack_desc d;
    auto desc = [&](int layout, int dtype) {
      std::memset(&d, 0, sizeof d);
      d.layout = layout; d.dtype = dtype; d.scale = 1.f;
    };
    desc(DAC_PACK_CODEC, DAC_FP8); d.O = 100; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_CODEC, DAC_F16); d.O = 100; d.flag = 1; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_EMU_FP16, DAC_F32); d.O = 100; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_CONV, DAC_BF16); d.O = 5; d.C = 6; d.kh = d.kw = 7; d.kwp = 8; d.round = 1;
    EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    EXPECT(run(d, nullptr, nullptr, nullptr, 0) == DAC_E_ARG);                         // capacity one byte short
    d.C = 0; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);
    desc(DAC_PACK_CONV, DAC_F32); d.O = 5; d.C = 13; d.kh = d.kw = 3; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_DUAL, DAC_F16); d.O = 5; d.C = 6; d.kh = d.kw = 7; d.kwp = 8; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_DUAL, DAC_BF16); d.O = 3; d.C = 64; d.kh = d.kw = 3; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    d.dtype = DAC_F32; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);         // 16-bit only
    desc(DAC_PACK_UPH_ROW, DAC_BF16); d.O = 3; d.C = 12; d.kh = d.kw = 3; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_UPH_COL, DAC_F16); d.O = 3; d.C = 12; d.kh = d.kw = 3; d.round = 1; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    d.kh = d.kw = 1; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);           // 3x3 only
    desc(DAC_PACK_Q8C3, DAC_FP8); d.O = d.C = 64; d.kh = d.kw = 3; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    d.C = 32; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);
    desc(DAC_PACK_GEGLU, DAC_BF16); d.F = 48; d.I = 8; EXPECT(run(d, nullptr, nullptr, b.data()) == DAC_OK);
    EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);                            // bias required
    EXPECT(run(d, nullptr, nullptr, b.data(), 2) == DAC_E_ARG);
    desc(DAC_PACK_GEGLU_GS, DAC_F16); d.F = 96; d.I = 8; EXPECT(run(d, nullptr, nullptr, b.data()) == DAC_OK);
    d.F = 48; EXPECT(run(d, nullptr, nullptr, b.data()) == DAC_E_ARG);                 // F % 32
    desc(DAC_PACK_CONCAT, DAC_BF16); d.K = 3; d.O = 4; d.I = 8; d.scale = 0.25f; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_TRANSPOSE, DAC_F32); d.I = 5; d.O = 7; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_FP8, DAC_FP8); d.O = 3; d.K = 192; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_OK);
    desc(DAC_PACK_FOLD_LN, DAC_BF16); d.O = 6; d.K = 32; EXPECT(run(d, g.data(), b.data(), b.data()) == DAC_OK);
    EXPECT(run(d, g.data(), nullptr, nullptr) == DAC_OK);
    EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);                            // gain required
    desc(DAC_PACK_LA_FOLD, DAC_F16); d.O = 12; d.C = 16; d.flag = 1; EXPECT(run(d, g.data(), nullptr, nullptr) == DAC_OK);
    d.O = 8; EXPECT(run(d, g.data(), nullptr, nullptr) == DAC_E_ARG);
    desc(99, DAC_BF16); d.O = 4; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);
    desc(DAC_PACK_CONV, 99); d.O = 4; d.C = 8; d.kh = d.kw = 3; EXPECT(run(d, nullptr, nullptr, nullptr) == DAC_E_ARG);
    size_t need[3];
    EXPECT(dac_op_pack(nullptr, w.data(), nullptr, nullptr, nullptr, nullptr, nullptr, need) == DAC_E_ARG);
    desc(DAC_PACK_CONV, DAC_BF16); d.O = 4; d.C = 8; d.kh = d.kw = 3;
    EXPECT(dac_op_pack(&d, w.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DAC_E_ARG);
  }
  // dac_image_metrics: null pointers and unsupported shapes are refused before any device work.
  unsigned char bytes[4] = {0, 0, 0, 0};
  double rec[8];
  EXPECT(dac_image_metrics(nullptr, nullptr, 1, 3, 11, 11, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == DAC_E_ARG);
  EXPECT(dac_image_metrics(dummy, dummy, 1, 3, 11, 11, 0, bytes, bytes, rec, nullptr, nullptr) == DAC_E_ARG);
  EXPECT(dac_image_metrics(dummy, dummy, 0, 3, 11, 11, 0, bytes, bytes, rec, rec, nullptr) == DAC_E_ARG);   // B
  EXPECT(dac_image_metrics(dummy, dummy, 1, 2, 11, 11, 0, bytes, bytes, rec, rec, nullptr) == DAC_E_ARG);   // C
  EXPECT(dac_image_metrics(dummy, dummy, 1, 3, 10, 11, 0, bytes, bytes, rec, rec, nullptr) == DAC_E_ARG);   // H < 11
  EXPECT(dac_image_metrics(dummy, dummy, 1, 3, 16, 16, 3, bytes, bytes, rec, rec, nullptr) == DAC_E_ARG);   // cropped 10
  EXPECT(dac_image_metrics(dummy, dummy, 1, 3, 16, 16, -1, bytes, bytes, rec, rec, nullptr) == DAC_E_ARG);
  EXPECT(dac_image_metrics_workspace(1, 3, 11, 11, 0) > 0 && dac_image_metrics_workspace(1, 3, 10, 11, 0) == 0);
  // Tiled loop: a null handle, and the grid checks (shared with dac_sde_reverse_tiled) through the
  // handle-less blend hook; every refusal comes before any device work.
  const int32_t ys2[2] = {0, 16}, xs2[2] = {0, 8}, oob[2] = {0, 20}, desc[2] = {16, 0}, rep[2] = {0, 0},
                gap[2] = {0, 40}, late[2] = {8, 16}, brief[2] = {0, 4};
  EXPECT(dac_sde_reverse_tiled(nullptr, 0, dummy, dummy, nullptr, nullptr, 1, 48, 40, 32, 32, 16, ys2, 2, xs2, 2,
                               16, 1, nullptr, 0, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(nullptr, nullptr, 1, 48, 40, 32, 32, 16, ys2, 2, xs2, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, nullptr, 2, xs2, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, ys2, 2, xs2, 0, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 0, 48, 40, 32, 32, 16, ys2, 2, xs2, 2, nullptr) == DAC_E_ARG);     // B
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 1, 32, 0, ys2, 1, xs2, 2, nullptr) == DAC_E_ARG);       // th < 2
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 48, 16, ys2, 2, xs2, 1, nullptr) == DAC_E_ARG);     // tw > W
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, -1, ys2, 2, xs2, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 32, ys2, 2, xs2, 2, nullptr) == DAC_E_ARG);     // overlap
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, oob, 2, xs2, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, desc, 2, xs2, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, ys2, 2, rep, 2, nullptr) == DAC_E_ARG);
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 8, 32, 4, gap, 2, xs2, 2, nullptr) == DAC_E_ARG);       // rows 8..39
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, late, 2, xs2, 2, nullptr) == DAC_E_ARG);    // row 0
  EXPECT(dac_op_tile_blend(dummy, dummy, 1, 48, 40, 32, 32, 16, ys2, 2, brief, 2, nullptr) == DAC_E_ARG);   // last columns
  std::printf("build: %s\n", dac_build_id());

  // Unsupported UNet configurations fail in dac_create, and the half-built handle is freed.
  dac_config bad = small_unet();
  bad.nf = 30;
  h = nullptr;
  EXPECT(dac_create(0, DAC_F32, &bad, &h) == DAC_E_ARG && h == nullptr);
  bad = small_unet();
  bad.depth = 9;
  EXPECT(dac_create(0, DAC_F32, &bad, &h) == DAC_E_ARG && h == nullptr);
  bad = small_unet();
  bad.out_nc = 4;
  EXPECT(dac_create(0, DAC_F32, &bad, &h) == DAC_E_ARG && h == nullptr);

  // A valid configuration: without a GPU the engine's device setup fails (DAC_E_HIP or
  // DAC_E_ARG for a missing device) and nothing leaks; with one, walk the handle's states.
  const int rc = dac_create(0, DAC_F32, &c, &h);
  if (rc != DAC_OK) {
    EXPECT(h == nullptr && rc < 0);
    std::printf("no device: dac_create -> %d (expected without a GPU)\n", rc);
  } else {
    const int64_t shp[4] = {32, 6, 7, 7};
    std::vector<float> w(32 * 6 * 7 * 7, 0.01f);
    EXPECT(dac_set_weight(h, nullptr, w.data(), shp, 4, DAC_SRC_F32) == DAC_E_ARG);
    EXPECT(dac_set_weight(h, "init_conv.weight", nullptr, shp, 4, DAC_SRC_F32) == DAC_E_ARG);
    EXPECT(dac_set_weight(h, "init_conv.weight", w.data(), shp, -1, DAC_SRC_F32) == DAC_E_ARG);
    EXPECT(dac_set_weight(h, "init_conv.weight", w.data(), nullptr, 4, DAC_SRC_F32) == DAC_E_ARG);
    EXPECT(dac_set_weight(h, "init_conv.weight", w.data(), shp, 4, 7) == DAC_E_ARG);   // src dtype
    EXPECT(dac_set_weight(h, "init_conv.weight", w.data(), shp, 4, DAC_SRC_F32) == DAC_OK);
    // Forward before finalize: a state error, not a fault.
    EXPECT(dac_unet_forward(h, dummy, dummy, 1.f, nullptr, nullptr, 1, 8, 8, dummy, nullptr) == DAC_E_STATE);
    EXPECT(dac_sde_schedule(h, 50.f, 0, DAC_COSINE, 0.005f, nullptr, 0.f) == DAC_E_ARG);    // T < 1
    EXPECT(dac_sde_set_time_scale(h, -1.0) == DAC_E_ARG);
    // Strict load: almost every key is missing.
    const int fr = dac_finalize_weights(h);
    EXPECT(fr == DAC_E_MISSING || fr == DAC_E_KEY);
    EXPECT(std::strlen(dac_last_error(h)) > 0);
    std::printf("finalize with missing keys -> %d: %.80s...\n", fr, dac_last_error(h));
    dac_destroy(h);
  }
  if (g_fail) {
    std::fprintf(stderr, "abi_asan: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("abi_asan: all checks passed\n");
  return 0;
}
