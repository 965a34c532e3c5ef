// pack.cpp — host-only weight packing (pack.h): codecs, 16-bit rounding, kernel layouts.
#include "pack.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace dac {

// ============================================================================= codecs
uint16_t f2bf_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf2f_host(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
uint16_t f2h_host(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
  if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (ax > 0x7f800000u ? 0x200u : 0u));
  if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);          // >= 65520 -> inf
  if (ax < 0x38800000u) {                                             // |f| < 2^-14: subnormal
    float a;
    std::memcpy(&a, &ax, 4);
    return (uint16_t)(sign | (uint32_t)std::nearbyint(a * 16777216.f));   // a * 2^24 is exact
  }
  uint32_t h = (((ax >> 23) - 112u) << 10) | ((ax & 0x7fffffu) >> 13);
  const uint32_t rem = ax & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}
float h2f_host(uint16_t h) {
  const int e = (h >> 10) & 0x1f;
  const uint32_t m = h & 0x3ffu;
  float v = e == 0 ? std::ldexp((float)m, -24)
                   : e == 31 ? (m ? NAN : INFINITY) : std::ldexp((float)(m | 0x400u), e - 25);
  return (h & 0x8000u) ? -v : v;
}
uint8_t f2e4m3_host(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  const float a = std::fabs(f);
  if (std::isnan(a)) return 0x7f;
  if (a >= 464.f) return sign | 0x7e;
  if (a < std::ldexp(1.f, -6)) {                       // subnormal: q * 2^-9
    const int q = (int)std::nearbyint(a * 512.f);
    return sign | (uint8_t)(q >= 8 ? 0x08 : q);
  }
  int e;
  std::frexp(a, &e);                                   // a = m * 2^e, m in [0.5, 1)
  int E = e - 1 + 7;
  int q = (int)std::nearbyint((a / std::ldexp(1.f, e - 1) - 1.f) * 8.f);
  if (q == 8) { q = 0; ++E; }
  if (E > 15 || (E == 15 && q == 7)) return sign | 0x7e;
  return sign | (uint8_t)(E << 3) | (uint8_t)q;
}
float e4m3f_host(uint8_t b) {
  const int s = b >> 7, E = (b >> 3) & 15, q = b & 7;
  if (E == 15 && q == 7) return NAN;
  const float v = E ? std::ldexp(1.f + q / 8.f, E - 7) : std::ldexp(q / 8.f, -6);
  return s ? -v : v;
}
uint16_t enc16(Store t, float f) { return t == Store::f16 ? f2h_host(f) : f2bf_host(f); }
float dec16(Store t, uint16_t h) { return t == Store::f16 ? h2f_host(h) : bf2f_host(h); }

// ============================================================================= 16-bit rounding
namespace {

template <Store S> uint16_t enc(float f) { return S == Store::f16 ? f2h_host(f) : f2bf_host(f); }
template <Store S> float dec(uint16_t h) { return S == Store::f16 ? h2f_host(h) : bf2f_host(h); }

// The 16-bit neighbour of h one step toward f (h != f, both finite); both formats are
// sign-magnitude, so a magnitude step is +-1 on the bits.
template <Store S>
uint16_t step_toward(uint16_t h, float f) {
  const float v = dec<S>(h);
  const bool up = f > v;
  if (v == 0.f) return up ? 0x0001 : 0x8001;
  return (uint16_t)(((v > 0.f) == up) ? h + 1 : h - 1);
}

template <Store S>
std::vector<uint16_t> quantize16_t(const std::vector<float>& v, int taps, int cin, Round rm) {
  std::vector<uint16_t> h(v.size());
  for (size_t i = 0; i < v.size(); ++i) h[i] = enc<S>(v[i]);
  if (taps < 2 || rm == Round::rne) return h;
  const size_t rows = v.size() / ((size_t)taps * cin);
  std::vector<size_t> idx(taps);
  std::vector<char> used(taps);
  for (size_t o = 0; o < rows; ++o)
    for (int c = 0; c < cin; ++c) {
      double r = 0;
      for (int t = 0; t < taps; ++t) {
        idx[t] = (o * taps + t) * cin + c;
        used[t] = 0;
        r += (double)v[idx[t]] - dec<S>(h[idx[t]]);
      }
      for (int it = 0; it < taps; ++it) {
        int best = -1;
        double br = std::fabs(r);
        for (int t = 0; t < taps; ++t) {
          const float w = v[idx[t]];
          const uint16_t q = h[idx[t]];
          if (used[t] || dec<S>(q) == w || !std::isfinite(w)) continue;
          const double nr = r + (double)dec<S>(q) - dec<S>(step_toward<S>(q, w));
          if (std::fabs(nr) < br) { br = std::fabs(nr); best = t; }
        }
        if (best < 0) break;
        const uint16_t q = h[idx[best]], q2 = step_toward<S>(q, v[idx[best]]);
        r += (double)dec<S>(q) - dec<S>(q2);
        h[idx[best]] = q2;
        used[best] = 1;
      }
    }
  return h;
}

}  // namespace

std::vector<uint16_t> quantize16(const std::vector<float>& v, int taps, int cin, Store t, Round r) {
  return t == Store::f16 ? quantize16_t<Store::f16>(v, taps, cin, r) : quantize16_t<Store::bf16>(v, taps, cin, r);
}

std::vector<float> emulate16(const std::vector<float>& v, int taps, int cin, bool fp16, Round r) {
  std::vector<float> q(v.size());
  if (fp16) {
    for (size_t i = 0; i < v.size(); ++i) {            // round to 11 significant bits (normals)
      int e;
      const double m = std::frexp((double)v[i], &e);
      q[i] = (float)std::ldexp(std::nearbyint(std::ldexp(m, 11)), e - 11);
    }
    return q;
  }
  const std::vector<uint16_t> h = quantize16(v, taps, cin, Store::bf16, r);
  for (size_t i = 0; i < v.size(); ++i) q[i] = bf2f_host(h[i]);
  return q;
}

// ============================================================================= knobs
Round PackKnobs::round(Store t, const std::string& key) const {
  const bool by_key = !wround_key.empty() && !key.empty() && key.find(wround_key) != std::string::npos;
  const bool rne = wround == 0 || (wround == 1 && t == Store::f16);
  return by_key || !rne ? Round::keep_sums : Round::rne;
}
bool PackKnobs::emu_skips(const std::string& key) const {
  size_t a = 0;
  while (a < emu_wskip.size()) {
    size_t b = emu_wskip.find(',', a);
    if (b == std::string::npos) b = emu_wskip.size();
    if (b > a && key.find(emu_wskip.substr(a, b - a)) != std::string::npos) return true;
    a = b + 1;
  }
  return false;
}
PackKnobs pack_knobs_from_env() {
  PackKnobs k;
  auto str = [](const char* n) { const char* v = getenv(n); return std::string(v ? v : ""); };
  if (const char* v = getenv("DAC_WROUND")) k.wround = (int)strtol(v, nullptr, 0);
  k.wround_key = str("DAC_WROUND_KEY");
  if (const char* v = getenv("DAC_UPH")) k.uph = atoi(v);
  if (const char* v = getenv("DAC_EMU_W")) k.emu_w = (int)strtol(v, nullptr, 0);
  k.emu_wskip = str("DAC_EMU_WSKIP");
  if (const char* v = getenv("DAC_EMU_FP16")) k.emu_fp16 = atoi(v) != 0;
  if (const char* v = getenv("DAC_LA_QSHIFT")) k.la_qshift = atoi(v) != 0;
  return k;
}

// ============================================================================= layouts
std::vector<float> pack_ohwi(const float* w, int O, int C, int kh, int kw, int kws, int cin) {
  std::vector<float> p((size_t)O * kh * kws * cin, 0.f);
  for (int o = 0; o < O; ++o)
    for (int c = 0; c < C; ++c)
      for (int y = 0; y < kh; ++y)
        for (int x = 0; x < kw; ++x)
          p[(((size_t)o * kh + y) * kws + x) * cin + c] = w[(((size_t)o * C + c) * kh + y) * kw + x];
  return p;
}

std::vector<uint16_t> pack_dual(const float* w, int O, int C, int kh, int kw, int kwp, int cin, Store t) {
  const bool rowtap = kwp > kw;
  const int kws = rowtap ? kwp : kw;
  const size_t per = (size_t)kh * kws * cin;                   // one precision part of a row
  std::vector<uint16_t> h((size_t)O * 2 * per, 0);
  for (int o = 0; o < O; ++o)
    for (int c = 0; c < C; ++c)
      for (int y = 0; y < kh; ++y)
        for (int x = 0; x < kw; ++x) {
          const float v = w[(((size_t)o * C + c) * kh + y) * kw + x];
          const uint16_t hi = enc16(t, v), lo = enc16(t, v - dec16(t, hi));
          const size_t tap = (size_t)y * kws + x;
          if (rowtap) {
            h[(size_t)o * 2 * per + tap * cin + c] = hi;
            h[(size_t)o * 2 * per + per + tap * cin + c] = lo;
          } else {
            h[(size_t)o * 2 * per + tap * 2 * cin + c] = hi;
            h[(size_t)o * 2 * per + tap * 2 * cin + cin + c] = lo;
          }
        }
  return h;
}

std::vector<float> fold_row_phase(const std::vector<float>& p, int O, int cin) {
  const size_t R = (size_t)3 * cin;                    // one kernel row [3][cin]
  std::vector<float> q((size_t)O * 4 * R);
  for (int o = 0; o < O; ++o) {
    const float* w = &p[(size_t)o * 3 * R];
    float* d = &q[(size_t)o * 4 * R];
    for (size_t k = 0; k < R; ++k) {
      d[k] = w[k];
      d[R + k] = w[R + k] + w[2 * R + k];
      d[2 * R + k] = w[k] + w[R + k];
      d[3 * R + k] = w[2 * R + k];
    }
  }
  return q;
}

std::vector<float> fold_rowcol_phase(const std::vector<float>& p, int O, int cin) {
  static const int lo[4] = {0, 1, 0, 2}, hi[4] = {0, 2, 1, 2};   // index ranges of the 4 sets
  const size_t C = cin;
  std::vector<float> q((size_t)O * 16 * C);
  for (int o = 0; o < O; ++o)
    for (int rs = 0; rs < 4; ++rs)
      for (int cs = 0; cs < 4; ++cs)
        for (size_t c = 0; c < C; ++c) {
          float v = 0.f;
          for (int kh = lo[rs]; kh <= hi[rs]; ++kh)
            for (int kw = lo[cs]; kw <= hi[cs]; ++kw) v += p[(((size_t)o * 3 + kh) * 3 + kw) * C + c];
          q[(((size_t)o * 4 + rs) * 4 + cs) * C + c] = v;
        }
  return q;
}

std::vector<int> geglu_rows(int F) {
  std::vector<int> src(2 * F);
  for (int r = 0; r < 2 * F; ++r) {
    const int g = r / 32, s = r % 32;
    src[r] = s < 16 ? 16 * g + s : F + 16 * g + (s - 16);
  }
  return src;
}
std::vector<int> geglu_gs_rows(int F) {
  std::vector<int> src(2 * F);
  for (int L = 0; L < 2 * F; ++L) {
    const int G = L / 64, lg = (L % 64) / 16, e = L % 16;
    src[L] = (e < 8 ? 0 : F) + 32 * G + 8 * lg + (e & 7);
  }
  return src;
}
std::vector<float> gather_rows(const float* w, const std::vector<int>& rows, int I) {
  std::vector<float> p(rows.size() * (size_t)I);
  for (size_t r = 0; r < rows.size(); ++r) std::copy(w + (size_t)rows[r] * I, w + (size_t)(rows[r] + 1) * I, p.begin() + r * I);
  return p;
}
std::vector<float> concat_rows(const float* const* parts, int nparts, int O, int I, float scale0) {
  std::vector<float> p;
  p.reserve((size_t)nparts * O * I);
  for (int k = 0; k < nparts; ++k) p.insert(p.end(), parts[k], parts[k] + (size_t)O * I);
  if (scale0 != 1.f)
    for (size_t i = 0; i < (size_t)O * I; ++i) p[i] *= scale0;
  return p;
}
std::vector<float> transpose_io(const float* w, int I, int O) {
  std::vector<float> t((size_t)I * O);
  for (int i = 0; i < I; ++i)
    for (int o = 0; o < O; ++o) t[(size_t)o * I + i] = w[(size_t)i * O + o];
  return t;
}

// ============================================================================= MX e4m3
// The block exponent: the smallest e with mx / 2^e <= 448. make_q8c3 takes the logarithm in
// double; make_fp8 in float, where the sum k + log2(1 + d) rounds to k for mx within a few ulp above
// 448 * 2^k, so such a block keeps e = k and its largest value saturates to 448. The packed bytes
// of both are those their kernels were validated with.
static int mx_exponent(float mx, bool wide) {
  if (!(mx > 0.f)) return 0;
  const int e = (int)std::ceil(wide ? std::log2((double)mx / 448.0) : (double)std::log2(mx / 448.f));
  return std::min(126, std::max(-126, e));
}

Mx8 make_fp8(const std::vector<float>& p, int O, int K) {
  Mx8 m;
  const int Kp = m.Kp = (K + 127) / 128 * 128;
  m.w8.assign((size_t)O * Kp, 0);
  m.s8.assign((size_t)O * (Kp / 64), 127);
  for (int o = 0; o < O; ++o)
    for (int b = 0; b < Kp / 64; ++b) {
      const int k1 = std::min(64 * b + 64, K);
      float mx = 0.f;
      for (int k = 64 * b; k < k1; ++k) mx = std::max(mx, std::fabs(p[(size_t)o * K + k]));
      const int e = mx_exponent(mx, false);
      m.s8[(size_t)o * (Kp / 64) + b] = (uint8_t)(127 + e);
      const float inv = std::ldexp(1.f, -e);
      for (int k = 64 * b; k < k1; ++k) m.w8[(size_t)o * Kp + k] = f2e4m3_host(p[(size_t)o * K + k] * inv);
    }
  return m;
}

Mx8 make_q8c3(const std::vector<float>& p) {
  Mx8 m;
  m.Kp = 576;
  m.w8.assign((size_t)64 * 576, 0);
  m.s8.assign((size_t)64 * 18, 127);
  for (int n = 0; n < 64; ++n)
    for (int t = 0; t < 9; ++t)
      for (int h = 0; h < 2; ++h) {
        const size_t o = (size_t)n * 576 + t * 64 + 32 * h;
        float mx = 0.f;
        for (int c = 0; c < 32; ++c) mx = std::max(mx, std::fabs(p[o + c]));
        const int e = mx_exponent(mx, true);
        m.s8[(size_t)n * 18 + t * 2 + h] = (uint8_t)(127 + e);
        for (int c = 0; c < 32; ++c) m.w8[o + c] = f2e4m3_host(std::ldexp(p[o + c], -e));
      }
  return m;
}

std::vector<float> fp8_dequant(const Mx8& m, int O, int K) {
  std::vector<float> d((size_t)O * K);
  for (int o = 0; o < O; ++o)
    for (int k = 0; k < K; ++k)
      d[(size_t)o * K + k] =
          e4m3f_host(m.w8[(size_t)o * m.Kp + k]) * std::ldexp(1.f, (int)m.s8[(size_t)o * (m.Kp / 64) + k / 64] - 127);
  return d;
}

// ============================================================================= folds
FoldedLN fold_ln(const std::vector<float>& p, int O, int K, const float* g, const float* beta, const float* pb,
                 Store t) {
  FoldedLN f;
  f.w.resize((size_t)O * K);
  f.cs.resize(O);
  f.bias.resize(O);
  for (int o = 0; o < O; ++o) {
    double c = 0, b = pb ? pb[o] : 0.0;
    for (int k = 0; k < K; ++k) {
      const uint16_t h = enc16(t, p[(size_t)o * K + k] * g[k]);
      f.w[(size_t)o * K + k] = h;
      c += dec16(t, h);
      if (beta) b += (double)p[(size_t)o * K + k] * beta[k];
    }
    f.cs[o] = (float)c;
    f.bias[o] = (float)b;
  }
  return f;
}

LaFold fold_la_gain(const std::vector<float>& pq, int O, int C, int nq, const float* g, bool qshift_on) {
  LaFold f;
  f.wg.resize(pq.size());
  double mx = 0;
  for (int o = 0; o < O; ++o) {
    double n2 = 0;
    for (int k = 0; k < C; ++k) {
      f.wg[(size_t)o * C + k] = pq[(size_t)o * C + k] * g[k];
      n2 += (double)f.wg[(size_t)o * C + k] * f.wg[(size_t)o * C + k];
    }
    if (o < nq) mx = std::max(mx, std::sqrt(n2));
  }
  const double bound = 1.01 * mx * std::sqrt((double)C) + 0.05;
  f.qshift = (qshift_on && bound <= 40.0) ? (float)bound : 0.f;
  return f;
}

}  // namespace dac
