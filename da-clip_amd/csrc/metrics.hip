// metrics.hip — evaluation metrics of config/daclip-sde/test.py:131-196 on the device, fp64:
//  * im_quantise : util.tensor2img (utils/img_utils.py:126-163) for a batch: fp32 [B,C,H,W] RGB
//    -> uint8 [B,H,W,C] BGR, clamp to [0,1], * 255 in fp32, round half to even; counts the
//    non-finite inputs per block.
//  * im_tile     : per (image, plane, 16x32 tile of the SSIM map): the SSE of the pixels the
//    tile owns and the sum of its SSIM map values (utils/img_utils.py:182-234: 11x11 Gaussian
//    window, sigma 1.5, 'valid' region), the window applied in its separable form. Planes are
//    the C stored channels and, for C = 3, Y = (24.966 B + 128.553 G + 65.481 R) / 255 + 16
//    (data/util.py:189-210 on a float input, not rounded).
//  * im_finish   : per image, the block partials summed in a fixed order into the 8-double
//    result record.
// No atomics: every partial has one writer and every sum one fixed order, so a record depends
// on neither the batch size, the image's place in the batch, nor the run.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace dac {

constexpr int IM_TH = 16, IM_TW = 32;                  // SSIM-map tile (rows x columns)
constexpr int IM_K = 11, IM_HALO = IM_K - 1;           // window taps, halo of a tile
constexpr int IM_IH = IM_TH + IM_HALO, IM_IW = IM_TW + IM_HALO;   // staged pixels: 26 x 42
constexpr int IM_QB = 256;                             // pixels per quantise block

struct ImWin { double g[IM_K]; };                      // normalised 11-tap Gaussian

struct ImShape {
  int B, C, H, W, cb;
  int Hc, Wc, Ho, Wo;       // cropped window, SSIM map ('valid' region of the window)
  int tx, ty, planes, nq;   // tiles per map, planes per image, quantise blocks per image
};

static ImShape im_shape(int B, int C, int H, int W, int cb) {
  ImShape s;
  s.B = B, s.C = C, s.H = H, s.W = W, s.cb = cb;
  s.Hc = H - 2 * cb, s.Wc = W - 2 * cb;
  s.Ho = s.Hc - IM_HALO, s.Wo = s.Wc - IM_HALO;
  s.tx = (s.Wo + IM_TW - 1) / IM_TW, s.ty = (s.Ho + IM_TH - 1) / IM_TH;
  s.planes = C == 3 ? 4 : 1;
  s.nq = (int)(((size_t)H * W + IM_QB - 1) / IM_QB);
  return s;
}

// Workspace: double ssim[B][planes][tiles] | 8-byte sse[B][planes][tiles] (int64 for the stored
// channels, double for Y) | unsigned nonfinite[B][2][nq].
static size_t im_tiles(const ImShape& s) { return (size_t)s.B * s.planes * s.tx * s.ty; }

bool image_metrics_ok(int B, int C, int H, int W, int cb) {
  // grid.z carries B * planes (<= 65535); H * W stays an int so pixel indices fit 32 bits.
  return B >= 1 && B <= 16383 && (C == 1 || C == 3) && cb >= 0 && H >= IM_K && W >= IM_K &&
         cb <= (H - IM_K) / 2 && cb <= (W - IM_K) / 2 && (long long)H * W <= 0x7fffffffLL;
}

size_t image_metrics_ws_bytes(int B, int C, int H, int W, int cb) {
  if (!image_metrics_ok(B, C, H, W, cb)) return 0;
  const ImShape s = im_shape(B, C, H, W, cb);
  const size_t nf = ((size_t)B * 2 * s.nq * sizeof(unsigned) + 7) & ~(size_t)7;
  return im_tiles(s) * 16 + nf;
}

__global__ void __launch_bounds__(IM_QB) im_quantise_kernel(const float* __restrict__ out,
                                                            const float* __restrict__ gt,
                                                            unsigned char* __restrict__ out_u8,
                                                            unsigned char* __restrict__ gt_u8,
                                                            unsigned* __restrict__ nf_part, int C,
                                                            int HW, int nq) {
  const int b = blockIdx.y, which = blockIdx.z;
  const float* src = (which ? gt : out) + (size_t)b * C * HW;
  unsigned char* dst = (which ? gt_u8 : out_u8) + (size_t)b * C * HW;
  const int p = blockIdx.x * IM_QB + threadIdx.x;
  int bad = 0;
  if (p < HW) {
    for (int c = 0; c < C; ++c) {
      const float v = src[(size_t)c * HW + p];
      unsigned char q = 0;
      if (isfinite(v)) q = (unsigned char)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
      else ++bad;
      dst[(size_t)p * C + (C - 1 - c)] = q;            // RGB planes -> BGR bytes
    }
  }
  __shared__ int red[IM_QB / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < IM_QB / 64; ++w) t += red[w];
    nf_part[((size_t)b * 2 + which) * nq + blockIdx.x] = (unsigned)t;
  }
}

// One block per (tile, image x plane). 256 threads = 8 rows x 32 columns of the tile; LDS rows
// are read by 32 consecutive lanes at consecutive doubles, which an 8-byte LDS read serves
// without bank conflicts (64 banks of 4 bytes per 32-lane half).
__global__ void __launch_bounds__(256) im_tile_kernel(const unsigned char* __restrict__ out_u8,
                                                      const unsigned char* __restrict__ gt_u8,
                                                      double* __restrict__ ws_ssim,
                                                      long long* __restrict__ ws_sse, ImShape s,
                                                      ImWin win) {
  __shared__ double sa[IM_IH][IM_IW], sb[IM_IH][IM_IW];   // the tile + halo of both images
  __shared__ double hm[5][IM_IH][IM_TW];                   // row-filtered a, b, aa, bb, ab
  __shared__ double red_f[4][2];
  __shared__ long long red_i[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.z / s.planes, p = blockIdx.z - b * s.planes;
  const int x0 = blockIdx.x * IM_TW, y0 = blockIdx.y * IM_TH;
  const bool isY = p >= s.C;
  const size_t img = (size_t)b * s.H * s.W * s.C;
  const unsigned char* A = out_u8 + img;
  const unsigned char* G = gt_u8 + img;

  long long sse_i = 0;
  double sse_f = 0.0;
  for (int k = tid; k < IM_IH * IM_IW; k += 256) {
    const int ly = k / IM_IW, lx = k - ly * IM_IW;
    const int py = y0 + ly, px = x0 + lx;                  // in the cropped window
    double a = 0.0, g = 0.0;
    if (py < s.Hc && px < s.Wc) {
      const size_t at = ((size_t)(s.cb + py) * s.W + (s.cb + px)) * s.C;
      // The tile whose SSIM rows / columns hold the window centred here owns the pixel's SSE
      // (the 5-pixel rim of the cropped window goes to the nearest tile).
      const int cy = min(max(py - IM_HALO / 2, 0), s.Ho - 1), cx = min(max(px - IM_HALO / 2, 0), s.Wo - 1);
      const bool own = cy / IM_TH == (int)blockIdx.y && cx / IM_TW == (int)blockIdx.x;
      if (!isY) {
        const int ai = A[at + p], gi = G[at + p];
        a = (double)ai, g = (double)gi;
        if (own) sse_i += (long long)((ai - gi) * (ai - gi));
      } else {
        a = (24.966 * (double)A[at] + 128.553 * (double)A[at + 1] + 65.481 * (double)A[at + 2]) / 255.0 + 16.0;
        g = (24.966 * (double)G[at] + 128.553 * (double)G[at + 1] + 65.481 * (double)G[at + 2]) / 255.0 + 16.0;
        if (own) sse_f += (a - g) * (a - g);
      }
    }
    sa[ly][lx] = a;
    sb[ly][lx] = g;
  }
  __syncthreads();

  for (int k = tid; k < IM_IH * IM_TW; k += 256) {
    const int ly = k / IM_TW, ox = k - ly * IM_TW;
    double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
    for (int t = 0; t < IM_K; ++t) {
      const double a = sa[ly][ox + t], g = sb[ly][ox + t], w = win.g[t];
      ha += w * a;
      hb += w * g;
      haa += w * (a * a);
      hbb += w * (g * g);
      hab += w * (a * g);
    }
    hm[0][ly][ox] = ha;
    hm[1][ly][ox] = hb;
    hm[2][ly][ox] = haa;
    hm[3][ly][ox] = hbb;
    hm[4][ly][ox] = hab;
  }
  __syncthreads();

  const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
  const int ox = tid & 31;
  double ssum = 0.0;
#pragma unroll
  for (int r = 0; r < IM_TH / 8; ++r) {
    const int oy = (tid >> 5) + 8 * r;
    double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int t = 0; t < IM_K; ++t) {
      const double w = win.g[t];
      m1 += w * hm[0][oy + t][ox];
      m2 += w * hm[1][oy + t][ox];
      e11 += w * hm[2][oy + t][ox];
      e22 += w * hm[3][oy + t][ox];
      e12 += w * hm[4][oy + t][ox];
    }
    const double s1 = e11 - m1 * m1, s2 = e22 - m2 * m2, s12 = e12 - m1 * m2;
    const double v = ((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2));
    if (y0 + oy < s.Ho && x0 + ox < s.Wo) ssum += v;
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ssum += __shfl_down(ssum, o);
    sse_f += __shfl_down(sse_f, o);
    sse_i += __shfl_down(sse_i, o);
  }
  if ((tid & 63) == 0) {
    red_f[tid >> 6][0] = ssum;
    red_f[tid >> 6][1] = sse_f;
    red_i[tid >> 6] = sse_i;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t slot = ((size_t)blockIdx.z * s.ty + blockIdx.y) * s.tx + blockIdx.x;
    ws_ssim[slot] = (red_f[0][0] + red_f[1][0]) + (red_f[2][0] + red_f[3][0]);
    const double f = (red_f[0][1] + red_f[1][1]) + (red_f[2][1] + red_f[3][1]);
    const long long i = red_i[0] + red_i[1] + red_i[2] + red_i[3];
    ws_sse[slot] = isY ? __double_as_longlong(f) : i;
  }
}

// One block per image: thread t sums partials t, t + 256, ... of each quantity, then the 256
// thread sums are combined by a fixed tree.
__global__ void __launch_bounds__(256) im_finish_kernel(const double* __restrict__ ws_ssim,
                                                        const long long* __restrict__ ws_sse,
                                                        const unsigned* __restrict__ nf_part,
                                                        double* __restrict__ results, ImShape s) {
  __shared__ double rf[3][256];
  __shared__ long long ri[2][256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int nt = s.tx * s.ty;
  double ssim = 0.0, ssim_y = 0.0, sse_y = 0.0;
  long long sse = 0, nf = 0;
  for (int p = 0; p < s.planes; ++p) {
    const size_t base = ((size_t)b * s.planes + p) * nt;
    for (int i = tid; i < nt; i += 256) {
      if (p < s.C) {
        ssim += ws_ssim[base + i];
        sse += ws_sse[base + i];
      } else {
        ssim_y += ws_ssim[base + i];
        sse_y += __longlong_as_double(ws_sse[base + i]);
      }
    }
  }
  for (int i = tid; i < 2 * s.nq; i += 256) nf += nf_part[(size_t)b * 2 * s.nq + i];
  rf[0][tid] = ssim, rf[1][tid] = ssim_y, rf[2][tid] = sse_y;
  ri[0][tid] = sse, ri[1][tid] = nf;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      for (int q = 0; q < 3; ++q) rf[q][tid] += rf[q][tid + o];
      for (int q = 0; q < 2; ++q) ri[q][tid] += ri[q][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* r = results + (size_t)b * 8;
    const double npx = (double)s.Hc * s.Wc, nmap = (double)s.Ho * s.Wo;
    r[0] = (double)ri[0][0];
    r[1] = npx * s.C;
    r[2] = rf[0][0] / (nmap * s.C);
    r[3] = s.C == 3 ? rf[2][0] : 0.0;
    r[4] = s.C == 3 ? npx : 0.0;
    r[5] = s.C == 3 ? rf[1][0] / nmap : 0.0;
    r[6] = (double)ri[1][0];
    r[7] = 0.0;
  }
}

void image_metrics(const float* out, const float* gt, int B, int C, int H, int W, int cb,
                   unsigned char* out_u8, unsigned char* gt_u8, double* results, void* ws,
                   hipStream_t st) {
  const ImShape s = im_shape(B, C, H, W, cb);
  double* ws_ssim = (double*)ws;
  long long* ws_sse = (long long*)(ws_ssim + im_tiles(s));
  unsigned* nf_part = (unsigned*)(ws_sse + im_tiles(s));
  // metrics.gaussian_window(): exp(-x^2 / (2 sigma^2)) / sum, sigma = 1.5.
  ImWin win;
  double sum = 0.0;
  for (int t = 0; t < IM_K; ++t) {
    const double x = t - (IM_K - 1) / 2.0;
    win.g[t] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
    sum += win.g[t];
  }
  for (int t = 0; t < IM_K; ++t) win.g[t] /= sum;
  im_quantise_kernel<<<dim3(s.nq, B, 2), IM_QB, 0, st>>>(out, gt, out_u8, gt_u8, nf_part, C, H * W, s.nq);
  im_tile_kernel<<<dim3(s.tx, s.ty, B * s.planes), 256, 0, st>>>(out_u8, gt_u8, ws_ssim, ws_sse, s, win);
  im_finish_kernel<<<B, 256, 0, st>>>(ws_ssim, ws_sse, nf_part, results, s);
}

}  // namespace dac
