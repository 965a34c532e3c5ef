// capi.cpp — extern "C" boundary of libdaclip_hip.so (declared in include/daclip_hip.h).
// Every entry point converts exceptions into a negative DAC_E* code + dac_last_error().
#include <cstdio>
#include <algorithm>
#include <cmath>

#include "engine.h"
#include "conv_plan.h"

struct dac_handle {
  int device = 0;
  int dtype = 0;
  dac_config cfg{};
  std::string err;
  dac::WStore ws;
  std::unique_ptr<dac::Engine> eng;
  bool finalized = false;
};

namespace {

template <class F>
int guard(dac_handle* h, F&& f) {
  if (!h) return DAC_E_ARG;
  try {
    h->err.clear();
    return f();
  } catch (const dac::Error& e) {
    h->err = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    h->err = "out of host memory";
    return DAC_E_NOMEM;
  } catch (const std::exception& e) {
    h->err = e.what();
    return DAC_E_ARG;
  }
}

// Keys of a DaCLIP checkpoint that the image path never reads (text tower, logit scales);
// open_clip/model.py:203-213, daclip_model.py:24.
bool ignorable(const dac_handle* h, const std::string& k) {
  if (!h->cfg.vit) return false;
  if (h->cfg.text) return k == "clip.logit_scale" || k == "logit_scale";
  static const char* pre[] = {"clip.transformer.", "clip.token_embedding.", "clip.ln_final.",
                              "clip.positional_embedding", "clip.text_projection",
                              "clip.logit_scale", "logit_scale"};
  for (auto p : pre)
    if (k.rfind(p, 0) == 0) return true;
  return false;
}

}  // namespace

extern "C" {

int dac_create(int device, int dtype, const dac_config* cfg, dac_handle** out) {
  if (!cfg || !out) return DAC_E_ARG;
  *out = nullptr;
  auto* h = new dac_handle();
  h->device = device;
  h->dtype = dtype;
  h->cfg = *cfg;
  int rc = guard(h, [&]() -> int {
    // in_nc = out_nc = 3: the sampler consumes the noise prediction as an image-shaped
    // tensor (sde_utils.py:245-247), and the output / step kernels are laid out for 3 channels.
    if (cfg->unet && (cfg->depth < 1 || cfg->depth > 8 || cfg->nf % 32 || cfg->in_nc != 3 ||
                      cfg->out_nc != 3))
      throw dac::Error(DAC_E_ARG, "unsupported UNet config (needs in_nc = out_nc = 3, nf % 32 == 0, "
                                  "1 <= depth <= 8)");
    h->eng = dac::make_engine(device, dtype, *cfg);
    return DAC_OK;
  });
  if (rc != DAC_OK) {
    delete h;
    return rc;
  }
  *out = h;
  return DAC_OK;
}

void dac_destroy(dac_handle* h) { delete h; }

int dac_set_weight(dac_handle* h, const char* key, const void* data, const int64_t* shape,
                   int ndim, int src_dtype) {
  return guard(h, [&]() -> int {
    if (!key || !data || ndim < 0 || ndim > 8 || (ndim > 0 && !shape))
      throw dac::Error(DAC_E_ARG, "bad argument");
    if (h->finalized) throw dac::Error(DAC_E_STATE, "weights already finalized");
    const std::string k(key);
    if (ignorable(h, k)) return 1;
    dac::HostW w;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      w.shape.push_back(shape[i]);
      n *= (size_t)shape[i];
    }
    const size_t es = src_dtype == DAC_SRC_F32 ? 4 : 2;
    std::vector<char> raw(n * es);
    hipPointerAttribute_t attr{};
    const bool dev = hipPointerGetAttributes(&attr, data) == hipSuccess &&
                     attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    if (dev) HIP_OK(hipMemcpy(raw.data(), data, n * es, hipMemcpyDeviceToHost));
    else std::memcpy(raw.data(), data, n * es);
    w.v.resize(n);
    if (src_dtype == DAC_SRC_F32) {
      std::memcpy(w.v.data(), raw.data(), n * 4);
    } else if (src_dtype == DAC_SRC_BF16) {
      const uint16_t* s = (const uint16_t*)raw.data();
      for (size_t i = 0; i < n; ++i) w.v[i] = dac::bf2f_host(s[i]);
    } else if (src_dtype == DAC_SRC_F16) {
      const uint16_t* s = (const uint16_t*)raw.data();
      for (size_t i = 0; i < n; ++i) w.v[i] = dac::h2f_host(s[i]);
    } else {
      throw dac::Error(DAC_E_ARG, "unknown src_dtype");
    }
    h->ws.m[k] = std::move(w);
    return DAC_OK;
  });
}

int dac_finalize_weights(dac_handle* h) {
  return guard(h, [&]() -> int {
    if (h->finalized) return DAC_OK;
    h->ws.missing.clear();
    h->eng->finalize(h->ws);
    std::string unexpected;
    for (auto& kv : h->ws.m)
      if (!kv.second.used) unexpected += (unexpected.empty() ? "\"" : ", \"") + kv.first + "\"";
    if (!unexpected.empty())
      throw dac::Error(DAC_E_KEY, "Unexpected key(s) in state_dict: " + unexpected);
    h->ws.m.clear();     // host copies no longer needed
    h->finalized = true;
    return DAC_OK;
  });
}

static void need_ready(dac_handle* h) {
  if (!h->finalized) throw dac::Error(DAC_E_STATE, "dac_finalize_weights not called");
}

int dac_encode_image(dac_handle* h, const float* img, int B, float* image_ctx, float* degra_ctx,
                     void* stream) {
  return guard(h, [&]() -> int {
    need_ready(h);
    if (!img || !image_ctx || B < 1) throw dac::Error(DAC_E_ARG, "bad argument");
    h->eng->encode(img, B, image_ctx, degra_ctx, (hipStream_t)stream);
    return DAC_OK;
  });
}

int dac_encode_text(dac_handle* h, const int64_t* tokens, int N, float* text_features, void* stream) {
  return guard(h, [&]() -> int {
    need_ready(h);
    if (!tokens || !text_features || N < 1) throw dac::Error(DAC_E_ARG, "bad argument");
    h->eng->encode_text(tokens, N, text_features, (hipStream_t)stream);
    return DAC_OK;
  });
}

int dac_degradation_probs(dac_handle* h, const float* degra, const float* text_features, int B, int K,
                          int E, float* probs, int32_t* argmax, void* stream) {
  return guard(h, [&]() -> int {
    if (!degra || !text_features || !probs || !argmax || B < 1 || K < 1 || K > 64 || E < 1)
      throw dac::Error(DAC_E_ARG, "bad argument (1 <= K <= 64)");
    dac::degradation_probs(degra, text_features, B, K, E, probs, argmax, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return DAC_OK;
  });
}

int dac_unet_forward(dac_handle* h, const float* xt, const float* mu, float t,
                     const float* text_ctx, const float* image_ctx, int B, int H, int W,
                     float* eps_out, void* stream) {
  return guard(h, [&]() -> int {
    need_ready(h);
    if (!xt || !mu || !eps_out || B < 1 || H < 2 || W < 2) throw dac::Error(DAC_E_ARG, "bad argument");
    h->eng->unet_forward(xt, mu, t, text_ctx, image_ctx, B, H, W, eps_out, (hipStream_t)stream);
    return DAC_OK;
  });
}

int dac_sde_schedule(dac_handle* h, float max_sigma, int T, int schedule, float eps,
                     const float* tables, float dt) {
  return guard(h, [&]() -> int {
    if (T < 1) throw dac::Error(DAC_E_ARG, "T must be >= 1");
    auto& s = h->eng->sched;
    const dac::SdeSchedule old = s;
    dac::compute_schedule(s, max_sigma, T, schedule, eps);
    if (tables) {
      const int n = T + 1;
      s.thetas.assign(tables, tables + n);
      s.sigmas.assign(tables + n, tables + 2 * n);
      s.tcum.assign(tables + 2 * n, tables + 3 * n);
      s.sbar.assign(tables + 3 * n, tables + 4 * n);
      s.dt = dt;
    }
    if (s.T != old.T || s.dt != old.dt || s.max_sigma != old.max_sigma || s.thetas != old.thetas ||
        s.sigmas != old.sigmas || s.tcum != old.tcum || s.sbar != old.sbar)
      h->eng->invalidate_graphs();
    return DAC_OK;
  });
}

int dac_sde_set_time_scale(dac_handle* h, double scale) {
  return guard(h, [&]() -> int {
    if (!(scale > 0.0) || !std::isfinite(scale)) throw dac::Error(DAC_E_ARG, "time scale must be > 0");
    auto& s = h->eng->sched;
    if (s.time_scale != scale) {
      s.time_scale = scale;
      h->eng->invalidate_graphs();
    }
    return DAC_OK;
  });
}

int dac_sde_reverse(dac_handle* h, int mode, float* x_inout, const float* mu, const float* text_ctx,
                    const float* image_ctx, int B, int H, int W, int T, const float* noise,
                    uint64_t seed, void* stream) {
  return guard(h, [&]() -> int {
    need_ready(h);
    if (!x_inout || !mu || B < 1 || H < 2 || W < 2 || (mode != DAC_POSTERIOR && mode != DAC_SDE))
      throw dac::Error(DAC_E_ARG, "bad argument");
    h->eng->sde_reverse(mode, x_inout, mu, text_ctx, image_ctx, B, H, W, T, noise, seed,
                        (hipStream_t)stream);
    return DAC_OK;
  });
}

int dac_sde_reverse_tiled(dac_handle* h, int mode, float* x_inout, const float* mu,
                          const float* text_ctx, const float* image_ctx, int B, int H, int W, int th,
                          int tw, int overlap, const int32_t* ys, int ny, const int32_t* xs, int nx,
                          int tiles_per_forward, int T, const float* noise, uint64_t seed,
                          void* stream) {
  return guard(h, [&]() -> int {
    // Every argument check comes before the first device call.
    if (!x_inout || !mu || (mode != DAC_POSTERIOR && mode != DAC_SDE))
      throw dac::Error(DAC_E_ARG, "bad argument");
    const dac::TileGrid g = dac::check_tile_grid(B, H, W, th, tw, overlap, ys, ny, xs, nx);
    if (tiles_per_forward < 1) throw dac::Error(DAC_E_ARG, "tiles_per_forward must be >= 1");
    need_ready(h);
    h->eng->sde_reverse_tiled(mode, x_inout, mu, text_ctx, image_ctx, B, H, W, g, tiles_per_forward, T,
                              noise, seed, (hipStream_t)stream);
    return DAC_OK;
  });
}

int dac_op_tile_blend(const float* eps_tiles, float* eps_full, int B, int H, int W, int th, int tw,
                      int overlap, const int32_t* ys, int ny, const int32_t* xs, int nx,
                      void* stream) {
  if (!eps_tiles || !eps_full) return DAC_E_ARG;
  try {
    (void)dac::check_tile_grid(B, H, W, th, tw, overlap, ys, ny, xs, nx);
  } catch (const std::exception&) {
    return DAC_E_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  int32_t* dev = nullptr;
  if (hipMalloc(&dev, (size_t)(ny + nx) * sizeof(int32_t)) != hipSuccess) return DAC_E_NOMEM;
  hipError_t e = hipMemcpyAsync(dev, ys, ny * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dev + ny, xs, nx * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    dac::tile_blend(eps_tiles, eps_full, dev, dev + ny, xs, B, ny, nx, H, W, th, tw, overlap, st);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(st);
  (void)hipFree(dev);
  return e == hipSuccess && es == hipSuccess ? DAC_OK : DAC_E_HIP;
}

int dac_set_noise_offset(dac_handle* h, uint64_t first_image) {
  return guard(h, [&]() -> int {
    h->eng->set_noise_offset(first_image);
    return DAC_OK;
  });
}

int dac_posterior_step(dac_handle* h, int mode, float* x_inout, const float* eps, const float* mu,
                       const float* z, int t, int n, void* stream) {
  return guard(h, [&]() -> int {
    if (!x_inout || !eps || !mu || n < 1) throw dac::Error(DAC_E_ARG, "bad argument");
    h->eng->posterior_step(mode, x_inout, eps, mu, z, t, n, (hipStream_t)stream);
    return DAC_OK;
  });
}

double dac_unet_flops(dac_handle* h, int B, int H, int W) {
  double f = -1;
  guard(h, [&]() -> int {
    if (!h->cfg.unet) throw dac::Error(DAC_E_ARG, "no UNet");
    f = h->eng->unet_flops(B, H, W);
    return DAC_OK;
  });
  return f;
}

double dac_encode_flops(dac_handle* h, int B) {
  double f = -1;
  guard(h, [&]() -> int {
    if (!h->cfg.vit) throw dac::Error(DAC_E_ARG, "no vision tower");
    f = h->eng->encode_flops(B);
    return DAC_OK;
  });
  return f;
}

int dac_op_attention(const void* qkv, void* out, int B, int L, int H, int dtype, int variant,
                     void* stream) {
  const bool pre = (variant & DAC_ATTN_Q_PRESCALED) != 0;
  variant &= ~DAC_ATTN_Q_PRESCALED;
  if (!qkv || !out || B <= 0 || L <= 0 || H <= 0 ||
      (dtype != DAC_F32 && dtype != DAC_BF16 && dtype != DAC_F16) || variant < 0 || variant > 4 ||
      (variant == 2 && (dtype == DAC_F32 || L % 64)) ||
      (variant >= 3 && (dtype == DAC_F32 || L % 256 || L > 1024)))
    return DAC_E_ARG;
  const float scale = pre ? 0.f : 1.f / std::sqrt(32.f);
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == DAC_BF16) dac::flash_attn_d32_v<__bf16>(qkv, out, B, L, H, scale, variant, st);
  else if (dtype == DAC_F16) dac::flash_attn_d32_v<_Float16>(qkv, out, B, L, H, scale, variant, st);
  else dac::flash_attn_d32_v<float>(qkv, out, B, L, H, scale, variant, st);
  return hipGetLastError() == hipSuccess ? DAC_OK : DAC_E_HIP;
}

namespace {

// Argument checks shared by the two LinearAttention hooks: everything the launchers would throw
// on (or index out of bounds with) is refused here, before the first device call.
bool la_op_args_ok(int B, int HW, int C, int dtype) {
  if (B < 1 || HW < 1 || (C != 64 && C != 128 && C != 256)) return false;
  if (dtype != DAC_F32 && dtype != DAC_BF16 && dtype != DAC_F16) return false;
  return !(dtype == DAC_F32 && C == 256);
}

// Scratch of an op hook: freed on every path.
struct DevBuf {
  void* p = nullptr;
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
  ~DevBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

int dac_op_linear_attention(const void* x, const void* wqkv, const float* wout, const float* bout,
                            const float* gout, void* y, int B, int HW, int C, int dtype,
                            float qshift, void* stream) {
  if (!x || !wqkv || !wout || !bout || !gout || !y || !la_op_args_ok(B, HW, C, dtype) ||
      !(qshift >= 0.f))
    return DAC_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const size_t es = dtype == DAC_F32 ? 4 : 2;
  DevBuf weff, ws;
  if (!weff.alloc((size_t)B * C * 128 * es) ||
      !ws.alloc(dac::linear_attention_fused_ws_floats(B, HW) * sizeof(float)))
    return DAC_E_NOMEM;
  hipError_t e = hipSuccess;
  try {
    if (dtype == DAC_BF16)
      dac::linear_attention_fused<__bf16>(x, wqkv, wout, bout, gout, weff.p, y, B, HW, C, (float*)ws.p, st, qshift);
    else if (dtype == DAC_F16)
      dac::linear_attention_fused<_Float16>(x, wqkv, wout, bout, gout, weff.p, y, B, HW, C, (float*)ws.p, st, qshift);
    else
      dac::linear_attention_fused<float>(x, wqkv, wout, bout, gout, weff.p, y, B, HW, C, (float*)ws.p, st, qshift);
    e = hipGetLastError();
  } catch (const std::exception&) {
    (void)hipStreamSynchronize(st);
    return DAC_E_ARG;
  }
  const hipError_t es2 = hipStreamSynchronize(st);
  return e == hipSuccess && es2 == hipSuccess ? DAC_OK : DAC_E_HIP;
}

int dac_op_linear_attention_weff(const void* qkv, const float* wout, void* weff, int B, int HW, int C,
                                 int dtype, float hw_scale, void* stream) {
  if (!qkv || !wout || !weff || !la_op_args_ok(B, HW, C, dtype) || !(hw_scale >= 0.f))
    return DAC_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  DevBuf ws;
  if (!ws.alloc(dac::linear_attention_ws_floats(B, HW) * sizeof(float))) return DAC_E_NOMEM;
  if (dtype == DAC_BF16)
    dac::linear_attention_weff<__bf16>(qkv, wout, weff, B, HW, C, (float*)ws.p, st, hw_scale);
  else if (dtype == DAC_F16)
    dac::linear_attention_weff<_Float16>(qkv, wout, weff, B, HW, C, (float*)ws.p, st, hw_scale);
  else
    dac::linear_attention_weff<float>(qkv, wout, weff, B, HW, C, (float*)ws.p, st, hw_scale);
  const hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(st);
  return e == hipSuccess && es == hipSuccess ? DAC_OK : DAC_E_HIP;
}

namespace {

// The three selection knobs dac_op_conv may override for one call (the CU count stays).
struct KnobOverride {
  dac::ConvKnobs& k = dac::conv_knobs();
  const int s3 = k.conv3_force, s2 = k.conv2_force, s32 = k.conv2_force32;
  explicit KnobOverride(const dac_conv_desc& d) {
    if (d.conv3_force != DAC_CONV_KEEP) k.conv3_force = d.conv3_force;
    if (d.conv2_force != DAC_CONV_KEEP) k.conv2_force = d.conv2_force;
    if (d.conv2_force32 != DAC_CONV_KEEP) k.conv2_force32 = d.conv2_force32;
  }
  ~KnobOverride() { k.conv3_force = s3; k.conv2_force = s2; k.conv2_force32 = s32; }
};

// Descriptor + pointers -> ConvArgs (y, zero and part are filled in by the caller). False: an
// argument the kernels would index out of bounds with, or that no layer has.
bool conv_op_args(const dac_conv_desc& d, const void* x1, const void* x2, const void* w, const float* bias,
                  const float* ss, const void* res1, const void* res2, const float* bbias, const void* w_gs,
                  const float* b_gs, dac::ConvArgs& a, int& stride, int& pad) {
  if (d.dtype != DAC_F32 && d.dtype != DAC_BF16 && d.dtype != DAC_F16) return false;
  if (d.kh != 1 && d.kh != 3 && d.kh != 4 && d.kh != 7) return false;
  if (!x1 || !w) return false;
  const int es = d.dtype == DAC_F32 ? 4 : 2, VE = 16 / es;
  stride = d.kh == 4 ? 2 : 1;
  pad = d.kh == 3 || d.kh == 4 ? 1 : d.kh == 7 ? 3 : 0;
  const long LIM = 1 << 24;
  if (d.B < 1 || d.Hs < 1 || d.Ws < 1 || d.B > LIM || d.Hs > LIM || d.Ws > LIM || (d.up != 0 && d.up != 1) ||
      (d.up && d.kh != 3))
    return false;
  const int Hin = d.up ? 2 * d.Hs : d.Hs, Win = d.up ? 2 * d.Ws : d.Ws;
  if (Hin + 2 * pad < d.kh || Win + 2 * pad < d.kh || (d.kh == 4 && ((Hin | Win) & 1))) return false;
  const int Ho = (Hin + 2 * pad - d.kh) / stride + 1, Wo = (Win + 2 * pad - d.kh) / stride + 1;
  if ((long)d.B * Ho * Wo > ((long)1 << 30)) return false;
  if (d.Cin < VE || d.Cin % VE || d.Cin > LIM || d.C1 < 1 || d.Cout < 1 || d.Cout > LIM || d.cwrap < 0 || d.ksplit < 0 ||
      d.ksplit > 64)
    return false;
  if (d.act < dac::ACT_NONE || d.act > dac::ACT_GEGLU || (d.act == dac::ACT_GEGLU && (d.kh != 1 || d.Cout % 32)))
    return false;
  // K: [kh][kw][Cin], or the 7x7 row-tap layout (kw padded to 8; cwrap = 1: [hi rows | lo rows]).
  const bool rowtap = d.kh == 7 && d.Cin == 8 && d.K == (d.cwrap ? 2 : 1) * 7 * 8 * 8 && d.cwrap <= 1;
  if (!rowtap && (d.K != d.kh * d.kh * d.Cin || d.cwrap >= d.Cin || (d.cwrap && d.cwrap * 2 != d.Cin))) return false;
  // Channels [0, C1) from x1, the rest (up to the wrap) from x2.
  const int Cread = d.cwrap > 1 ? d.cwrap : d.Cin;
  if (d.C1 < Cread && (!x2 || d.ld2 < Cread - d.C1)) return false;
  if (d.ld1 < (d.C1 < Cread ? d.C1 : Cread)) return false;
  const int Cy = d.act == dac::ACT_GEGLU ? d.Cout / 2 : d.Cout;
  if (d.ldy < Cy || (res1 && d.ldr1 < Cy) || (res2 && d.ldr2 < Cy) || (ss && d.ss_ld < 0) || (bbias && d.bb_ld < 0))
    return false;
  a = dac::ConvArgs{};
  a.x1 = x1; a.x2 = x2; a.ld1 = d.ld1; a.ld2 = d.ld2; a.C1 = d.C1; a.Cin = d.Cin;
  a.Hs = d.Hs; a.Ws = d.Ws; a.up = d.up; a.B = d.B; a.Ho = Ho; a.Wo = Wo; a.Cout = d.Cout; a.K = d.K;
  a.w = w; a.bias = bias; a.ss = ss; a.ss_ld = d.ss_ld; a.res1 = res1; a.ldr1 = d.ldr1; a.res2 = res2;
  a.ldr2 = d.ldr2; a.bbias = bbias; a.bb_ld = d.bb_ld; a.ldy = d.ldy; a.act = d.act; a.cwrap = d.cwrap;
  a.ksplit = d.ksplit > 1 ? d.ksplit : 0;
  if (d.act == dac::ACT_GEGLU) { a.w_gs = w_gs; a.b_gs = b_gs; }
  return true;
}

}  // namespace

namespace {

// dac_op_conv / dac_op_conv_ex: e (may be null), w2 and y2 are the extension.
int conv_op(const dac_conv_desc* d, const dac_conv_ext* e, const void* x1, const void* x2, const void* w,
            const float* bias, const float* ss, const void* res1, const void* res2, const float* bbias,
            const void* w_gs, const float* b_gs, void* y, const void* w2, void* y2, int* plan_out, void* stream) {
  if (!d) return DAC_E_ARG;
  const int uph = e ? e->uph : 0;
  if (uph < 0 || uph > 2 || (!w2) != (!y2) || (y2 && !e)) return DAC_E_ARG;
  // The phase layouts keep [rows][taps][Cin] with 12 / 16 (row set, tap) pairs instead of 9.
  dac_conv_desc dd = *d;
  if (uph) {
    if (d->kh != 3 || d->up != 1 || d->cwrap || d->ksplit > 1 || d->Cin < 1 || d->Cin > (1 << 24) ||
        d->K != (uph == 2 ? 16 : 12) * d->Cin)
      return DAC_E_ARG;
    dd.K = 9 * d->Cin;
  }
  dac::ConvArgs a;
  int stride = 1, pad = 0;
  if (!conv_op_args(dd, x1, x2, w, bias, ss, res1, res2, bbias, w_gs, b_gs, a, stride, pad)) return DAC_E_ARG;
  a.K = d->K;
  a.uph = uph;
  if (y2) {
    if (e->ldy2 < d->Cout) return DAC_E_ARG;
    a.w2 = w2; a.y2 = y2; a.ldy2 = e->ldy2;
  }
  const int es = d->dtype == DAC_F32 ? 4 : 2;
  KnobOverride knobs(*d);
  // Planning never touches HIP (plan-only calls and every refusal stay off the device); a launch
  // then plans again with the device's CU count, as conv_dispatch does.
  dac::ConvPlan p = dac::conv_plan(a, d->kh, d->kh, stride, pad, es, dac::conv_knobs());
  if (p.kind == dac::CONV_NONE) return DAC_E_ARG;
  if (y) p = dac::conv_plan(a, d->kh, d->kh, stride, pad, es, dac::conv_launch_knobs());
  if (plan_out) {
    const int v[DAC_CONV_PLAN_N] = {(int)p.kind, p.BM, p.BN, p.ST, p.epi, p.fl, p.buffer_dma ? 1 : 0, p.label};
    std::copy(v, v + DAC_CONV_PLAN_N, plan_out);
  }
  if (!y) return DAC_OK;
  const hipStream_t st = (hipStream_t)stream;
  DevBuf zero, part;
  if (!zero.alloc(256)) return DAC_E_NOMEM;
  if (a.ksplit > 1 && !part.alloc((size_t)a.ksplit * a.B * a.Ho * a.Wo * a.Cout * sizeof(float))) return DAC_E_NOMEM;
  hipError_t err = hipMemsetAsync(zero.p, 0, 256, st);
  a.y = y; a.zero = zero.p; a.part = (float*)part.p;
  if (err == hipSuccess) {
    try {
      if (d->dtype == DAC_BF16) dac::conv<__bf16>(a, d->kh, d->kh, stride, pad, st);
      else if (d->dtype == DAC_F16) dac::conv<_Float16>(a, d->kh, d->kh, stride, pad, st);
      else dac::conv<float>(a, d->kh, d->kh, stride, pad, st);
      err = hipGetLastError();
    } catch (const std::exception&) {
      (void)hipStreamSynchronize(st);
      return DAC_E_ARG;
    }
  }
  const hipError_t es2 = hipStreamSynchronize(st);
  return err == hipSuccess && es2 == hipSuccess ? DAC_OK : DAC_E_HIP;
}

}  // namespace

int dac_op_conv(const dac_conv_desc* d, const void* x1, const void* x2, const void* w, const float* bias,
                const float* ss, const void* res1, const void* res2, const float* bbias, const void* w_gs,
                const float* b_gs, void* y, int* plan_out, void* stream) {
  return conv_op(d, nullptr, x1, x2, w, bias, ss, res1, res2, bbias, w_gs, b_gs, y, nullptr, nullptr, plan_out, stream);
}

int dac_op_conv_ex(const dac_conv_desc* d, const dac_conv_ext* e, const void* x1, const void* x2, const void* w,
                   const float* bias, const float* ss, const void* res1, const void* res2, const float* bbias,
                   const void* w_gs, const float* b_gs, void* y, const void* w2, void* y2, int* plan_out,
                   void* stream) {
  return conv_op(d, e, x1, x2, w, bias, ss, res1, res2, bbias, w_gs, b_gs, y, w2, y2, plan_out, stream);
}

int dac_op_rbfuse(const dac_rb_desc* d, const void* x1, const void* x2, const void* w1, const void* w2,
                  const void* wr, const float* ss, void* y, int* geom_out, void* stream) {
  if (!d || !x1 || !w1 || !w2 || !ss || ((uintptr_t)ss & 15)) return DAC_E_ARG;
  if (d->dtype != DAC_BF16 && d->dtype != DAC_F16) return DAC_E_ARG;
  const int LIM = 1 << 24;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->C1 < 1 || d->Cin < 1 || d->B > LIM || d->H > LIM || d->W > LIM ||
      d->C1 > LIM || d->Cin > LIM || (long)d->B * d->H * d->W > ((long)1 << 30))
    return DAC_E_ARG;
  if (d->C1 < d->Cin && (!x2 || d->ld2 < d->Cin - d->C1)) return DAC_E_ARG;
  if (d->ld1 < (d->C1 < d->Cin ? d->C1 : d->Cin) || d->ldy < 64 || d->ss_ld < 0) return DAC_E_ARG;
  dac::RbArgs a{};
  a.x1 = x1; a.x2 = x2; a.ld1 = d->ld1; a.ld2 = d->ld2; a.C1 = d->C1; a.Cin = d->Cin;
  a.B = d->B; a.H = d->H; a.W = d->W; a.w1 = w1; a.w2 = w2; a.wr = wr; a.ss = ss; a.ss_ld = d->ss_ld;
  a.y = y; a.ldy = d->ldy;
  const bool served = dac::rbfuse_ok(a);
  if (served && geom_out) dac::rbfuse_geometry(a, geom_out[0], geom_out[1]);
  if (!y) return served ? 1 : 0;
  if (!served) return DAC_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  hipError_t err = hipSuccess;
  try {
    if (d->dtype == DAC_BF16) dac::rbfuse<__bf16>(a, st);
    else dac::rbfuse<_Float16>(a, st);
    err = hipGetLastError();
  } catch (const std::exception&) {
    (void)hipStreamSynchronize(st);
    return DAC_E_ARG;
  }
  const hipError_t es2 = hipStreamSynchronize(st);
  return err == hipSuccess && es2 == hipSuccess ? DAC_OK : DAC_E_HIP;
}

namespace {

// What one dac_op_pack call is: the dimensions it uses, its element types and output sizes.
// False: an argument outside the layout's domain.
struct PackSpec {
  dac::Store st = dac::Store::f32;
  int es = 4, cin = 0, kws = 0;
  size_t need[3] = {0, 0, 0};
};
bool pack_spec(const dac_pack_desc& d, PackSpec& s) {
  const int LIM = 1 << 16;
  auto dims = [&](std::initializer_list<int> v) {
    size_t n = 1;
    for (int x : v) {
      if (x < 1 || x > LIM) return false;
      n *= (size_t)x;
      if (n > ((size_t)1 << 28)) return false;
    }
    return true;
  };
  const bool f32 = d.dtype == DAC_F32, h16 = d.dtype == DAC_BF16 || d.dtype == DAC_F16, e4 = d.dtype == DAC_FP8;
  if (!f32 && !h16 && !e4) return false;
  if (d.round != 0 && d.round != 1) return false;
  s.st = d.dtype == DAC_BF16 ? dac::Store::bf16 : d.dtype == DAC_F16 ? dac::Store::f16 : dac::Store::f32;
  s.es = h16 ? 2 : 4;
  const size_t es = s.es;
  switch (d.layout) {
    case DAC_PACK_CODEC:
      if (f32 || !dims({d.O})) return false;
      s.need[0] = (size_t)d.O * (d.flag ? 4 : e4 ? 1 : 2);
      return true;
    case DAC_PACK_EMU_FP16:
      if (!f32 || !dims({d.O})) return false;
      s.need[0] = (size_t)d.O * 4;
      return true;
    case DAC_PACK_CONV:
    case DAC_PACK_DUAL:
    case DAC_PACK_UPH_ROW:
    case DAC_PACK_UPH_COL:
    case DAC_PACK_Q8C3: {
      if (!dims({d.O, d.C, d.kh, d.kw}) || d.kwp < 0 || d.kwp > LIM) return false;
      const int VE = h16 ? 8 : 4;
      s.cin = (d.C + VE - 1) / VE * VE;
      s.kws = d.kwp > d.kw ? d.kwp : d.kw;
      if (!dims({d.O, d.kh, s.kws, s.cin, 2})) return false;
      const size_t n = (size_t)d.O * d.kh * s.kws * s.cin;
      if (d.layout == DAC_PACK_CONV) {
        if (e4) return false;
        s.need[0] = n * es;
      } else if (d.layout == DAC_PACK_DUAL) {
        if (!h16) return false;
        s.need[0] = 2 * n * 2;
      } else if (d.layout == DAC_PACK_Q8C3) {
        if (!e4 || d.O != 64 || d.C != 64 || d.kh != 3 || d.kw != 3 || d.kwp) return false;
        s.cin = 64;
        s.need[0] = (size_t)64 * 576;
        s.need[1] = (size_t)64 * 18;
      } else {
        if (e4 || d.kh != 3 || d.kw != 3 || d.kwp) return false;
        s.need[0] = (size_t)d.O * (d.layout == DAC_PACK_UPH_ROW ? 12 : 16) * s.cin * es;
      }
      return true;
    }
    case DAC_PACK_GEGLU:
    case DAC_PACK_GEGLU_GS:
      if (e4 || !dims({d.F, d.I, 2}) || d.F % (d.layout == DAC_PACK_GEGLU_GS ? 32 : 16)) return false;
      s.need[0] = (size_t)2 * d.F * d.I * es;
      s.need[1] = s.need[2] = (size_t)2 * d.F * 4;
      return true;
    case DAC_PACK_CONCAT:
      if (e4 || !dims({d.K, d.O, d.I})) return false;
      s.need[0] = (size_t)d.K * d.O * d.I * es;
      return true;
    case DAC_PACK_TRANSPOSE:
      if (!f32 || !dims({d.I, d.O})) return false;
      s.need[0] = (size_t)d.I * d.O * 4;
      return true;
    case DAC_PACK_FP8: {
      if (!e4 || !dims({d.O, d.K}) || !dims({d.O, d.K + 127})) return false;
      const size_t Kp = (size_t)(d.K + 127) / 128 * 128;
      s.need[0] = d.O * Kp;
      s.need[1] = d.O * (Kp / 64);
      s.need[2] = 4;
      return true;
    }
    case DAC_PACK_FOLD_LN:
      if (!h16 || !dims({d.O, d.K})) return false;
      s.need[0] = (size_t)d.O * d.K * 2;
      s.need[1] = s.need[2] = (size_t)d.O * 4;
      return true;
    case DAC_PACK_LA_FOLD:
      if (e4 || !dims({d.O, d.C}) || d.O % 3) return false;
      s.need[0] = (size_t)d.O * d.C * es;
      s.need[1] = 4;
      return true;
    default:
      return false;
  }
}

}  // namespace

int dac_op_pack(const dac_pack_desc* d, const float* w, const float* gain, const float* beta, const float* bias,
                void* const* out, const size_t* cap, size_t* need) {
  if (!d || !need) return DAC_E_ARG;
  PackSpec s;
  if (!pack_spec(*d, s)) return DAC_E_ARG;
  std::copy(s.need, s.need + 3, need);
  if (!out) return DAC_OK;                               // size query
  const bool geglu = d->layout == DAC_PACK_GEGLU || d->layout == DAC_PACK_GEGLU_GS;
  const bool gained = d->layout == DAC_PACK_FOLD_LN || d->layout == DAC_PACK_LA_FOLD;
  if (!w || !cap || (geglu && !bias) || (gained && !gain)) return DAC_E_ARG;
  for (int i = 0; i < 3; ++i)
    if (s.need[i] && (!out[i] || cap[i] < s.need[i])) return DAC_E_ARG;
  try {
    const dac::Round rm = d->round ? dac::Round::keep_sums : dac::Round::rne;
    auto put = [](void* dst, const auto& v) { std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    // v [rows][taps][cin] stored in the descriptor's dtype.
    auto store =[&](void* dst, const std::vector<float>& v, int taps, int cin) {
      if (s.es == 4) put(dst, v);
      else put(dst, dac::quantize16(v, taps, cin, s.st, rm));
    };
    switch (d->layout) {
      case DAC_PACK_CODEC:
        for (int i = 0; i < d->O; ++i) {
          if (d->dtype == DAC_FP8) {
            const uint8_t q = dac::f2e4m3_host(w[i]);
            if (d->flag) ((float*)out[0])[i] = dac::e4m3f_host(q);
            else ((uint8_t*)out[0])[i] = q;
          } else {
            const uint16_t q = dac::enc16(s.st, w[i]);
            if (d->flag) ((float*)out[0])[i] = dac::dec16(s.st, q);
            else ((uint16_t*)out[0])[i] = q;
          }
        }
        break;
      case DAC_PACK_EMU_FP16:
        put(out[0], dac::emulate16(std::vector<float>(w, w + d->O), 1, d->O, true, rm));
        break;
      case DAC_PACK_CONV:
        store(out[0], dac::pack_ohwi(w, d->O, d->C, d->kh, d->kw, s.kws, s.cin), d->kh * s.kws, s.cin);
        break;
      case DAC_PACK_DUAL:
        put(out[0], dac::pack_dual(w, d->O, d->C, d->kh, d->kw, d->kwp, s.cin, s.st));
        break;
      case DAC_PACK_UPH_ROW:
        store(out[0], dac::fold_row_phase(dac::pack_ohwi(w, d->O, d->C, 3, 3, 3, s.cin), d->O, s.cin), 12, s.cin);
        break;
      case DAC_PACK_UPH_COL:
        store(out[0], dac::fold_rowcol_phase(dac::pack_ohwi(w, d->O, d->C, 3, 3, 3, s.cin), d->O, s.cin), 16, s.cin);
        break;
      case DAC_PACK_Q8C3: {
        const dac::Mx8 m = dac::make_q8c3(dac::pack_ohwi(w, 64, 64, 3, 3, 3, 64));
        put(out[0], m.w8);
        put(out[1], m.s8);
        break;
      }
      case DAC_PACK_GEGLU:
      case DAC_PACK_GEGLU_GS: {
        const std::vector<int> rows = d->layout == DAC_PACK_GEGLU ? dac::geglu_rows(d->F) : dac::geglu_gs_rows(d->F);
        store(out[0], dac::gather_rows(w, rows, d->I), 1, d->I);
        put(out[1], dac::gather_rows(bias, rows, 1));
        put(out[2], rows);
        break;
      }
      case DAC_PACK_CONCAT: {
        std::vector<const float*> parts;
        for (int k = 0; k < d->K; ++k) parts.push_back(w + (size_t)k * d->O * d->I);
        store(out[0], dac::concat_rows(parts.data(), d->K, d->O, d->I, d->scale), 1, d->I);
        break;
      }
      case DAC_PACK_TRANSPOSE:
        put(out[0], dac::transpose_io(w, d->I, d->O));
        break;
      case DAC_PACK_FP8: {
        const dac::Mx8 m = dac::make_fp8(std::vector<float>(w, w + (size_t)d->O * d->K), d->O, d->K);
        put(out[0], m.w8);
        put(out[1], m.s8);
        *(int*)out[2] = m.Kp;
        break;
      }
      case DAC_PACK_FOLD_LN: {
        const dac::FoldedLN f =
            dac::fold_ln(std::vector<float>(w, w + (size_t)d->O * d->K), d->O, d->K, gain, beta, bias, s.st);
        put(out[0], f.w);
        put(out[1], f.cs);
        put(out[2], f.bias);
        break;
      }
      case DAC_PACK_LA_FOLD: {
        const dac::LaFold f = dac::fold_la_gain(std::vector<float>(w, w + (size_t)d->O * d->C), d->O, d->C, d->O / 3,
                                                gain, d->flag != 0);
        store(out[0], f.wg, 1, d->C);
        *(float*)out[1] = f.qshift;
        break;
      }
    }
  } catch (const std::bad_alloc&) {
    return DAC_E_NOMEM;
  }
  return DAC_OK;
}

size_t dac_image_metrics_workspace(int B, int C, int H, int W, int crop_border) {
  return dac::image_metrics_ws_bytes(B, C, H, W, crop_border);
}

int dac_image_metrics(const float* out, const float* gt, int B, int C, int H, int W, int crop_border,
                      unsigned char* out_bytes, unsigned char* gt_bytes, double* results,
                      void* workspace, void* stream) {
  if (!out || !gt || !out_bytes || !gt_bytes || !results || !workspace ||
      !dac::image_metrics_ok(B, C, H, W, crop_border))
    return DAC_E_ARG;
  dac::image_metrics(out, gt, B, C, H, W, crop_border, out_bytes, gt_bytes, results, workspace,
                     (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? DAC_OK : DAC_E_HIP;
}

int dac_profile_enable(dac_handle* h, int kernel_id) {
  return guard(h, [&]() -> int {
    h->eng->prof.enable(kernel_id);
    return DAC_OK;
  });
}

int dac_profile_read(dac_handle* h, double* mean_ms, double* flops_per_launch,
                     double* bytes_per_launch) {
  int n = 0;
  int rc = guard(h, [&]() -> int {
    auto& p = h->eng->prof;
    if (p.pass == dac::Pass::events) p.finish_events();
    const auto s = p.summary();
    if (p.kernel_id == dac::Profiler::ALL && getenv("DAC_PROFILE_PRINT")) p.report(stderr);   // per-shape report
    n = s.n;
    if (mean_ms) *mean_ms = s.mean_ms;
    if (flops_per_launch) *flops_per_launch = s.flops_per_launch;
    if (bytes_per_launch) *bytes_per_launch = s.bytes_per_launch;
    return DAC_OK;
  });
  return rc < 0 ? rc : n;
}

int dac_profile_mode(dac_handle* h, int graph_stamps) {
  return guard(h, [&]() -> int {
    h->eng->prof.stamps = graph_stamps != 0;
    return DAC_OK;
  });
}

int dac_profile_launch(dac_handle* h, int i, double* ms, double* flops, double* bytes, int* kernel_class,
                       double* start_ms, int* in_branch, char* label, int label_len, char* symbol,
                       int symbol_len) {
  return guard(h, [&]() -> int {
    const dac::Launch& l = h->eng->prof.at(i);
    if (ms) *ms = l.ms;
    if (flops) *flops = l.flops;
    if (bytes) *bytes = l.bytes;
    if (kernel_class) *kernel_class = l.cls;
    if (start_ms) *start_ms = l.t0_ms;
    if (in_branch) *in_branch = l.in_branch ? 1 : 0;
    if (label && label_len > 0) snprintf(label, label_len, "%s", l.label.c_str());
    if (symbol && symbol_len > 0) snprintf(symbol, symbol_len, "%s", l.symbol.c_str());
    return DAC_OK;
  });
}

int dac_profile_graph_ms(dac_handle* h, double* ms) {
  return guard(h, [&]() -> int {
    if (!ms) throw dac::Error(DAC_E_ARG, "null output");
    *ms = h->eng->prof.graph_ms;
    return DAC_OK;
  });
}

const char* dac_last_error(dac_handle* h) { return h ? h->err.c_str() : "null handle"; }

#ifndef DAC_BUILD_ID
#define DAC_BUILD_ID "unknown"
#endif
const char* dac_build_id(void) { return DAC_BUILD_ID; }

}  // extern "C"
