// tile.hip — tiled restoration of large images: the streaming kernels around the
// per-tile UNet forwards of dac_sde_reverse_tiled.
//  * tile_gather : windows of a full NCHW fp32 image -> the NCHW fp32 tile batch unet_prep reads.
//  * tile_blend  : per-tile fp32 eps -> full-image eps, weighted by the separable integer ramp
//                  w1(i) = min(i + 1, l - i, overlap + 1), fixed tile order, no atomics.
//  * rows_gather : per-image table rows (ResBlock scale/shift, cross-attention constants)
//                  repeated for the tiles of a chunk.
// Tile k of the batch is (image b, grid row iy, grid column ix) with k = (b*ny + iy)*nx + ix.
// All three are bandwidth-bound: one thread per 16 bytes along W where the image width, the
// tile width and every column offset are multiples of 4 (so a 4-pixel group never straddles a
// tile border), one thread per pixel otherwise.
#include "common.h"
#include "kernels.h"

namespace dac {

template <int V>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          const int* __restrict__ ys, const int* __restrict__ xs,
                                                          int ny, int nx, int H, int W, int th, int tw, int k0,
                                                          size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int twv = tw / V;
  const int xv = (int)(i % twv);
  const int y = (int)((i / twv) % th);
  const int c = (int)((i / ((size_t)twv * th)) % 3);
  const int k = k0 + (int)(i / ((size_t)twv * th * 3));
  const int ix = k % nx, iy = (k / nx) % ny, b = k / (nx * ny);
  const float* s = src + (((size_t)b * 3 + c) * H + ys[iy] + y) * W + xs[ix] + xv * V;
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + i * 4) = *reinterpret_cast<const f32x4*>(s);
  else dst[i] = *s;
}

static bool grid_vec4(const int32_t* xs, int nx, int W, int tw) {
  bool v = W % 4 == 0 && tw % 4 == 0;
  for (int i = 0; i < nx; ++i) v = v && xs[i] % 4 == 0;
  return v;
}

void tile_gather(const float* src, float* dst, const int32_t* ys_dev, const int32_t* xs_dev,
                 const int32_t* xs_host, int ny, int nx, int H, int W, int th, int tw, int k0, int nk,
                 hipStream_t st) {
  if (nk <= 0) return;
  const bool v4 = grid_vec4(xs_host, nx, W, tw) && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const size_t n = (size_t)nk * 3 * th * (v4 ? tw / 4 : tw);
  const unsigned g = (unsigned)((n + 255) / 256);
  if (v4) tile_gather_kernel<4><<<g, 256, 0, st>>>(src, dst, ys_dev, xs_dev, ny, nx, H, W, th, tw, k0, n);
  else tile_gather_kernel<1><<<g, 256, 0, st>>>(src, dst, ys_dev, xs_dev, ny, nx, H, W, th, tw, k0, n);
}

// Ramp weight of position i in a tile side of length l: 1 at the border, rising by 1 a pixel to
// overlap + 1 (an exact small integer).
__device__ __forceinline__ int ramp_w(int i, int l, int ov) { return min(min(i + 1, l - i), ov + 1); }

// The offsets ascend, so the tiles covering a position are one contiguous index range [i0, i1).
__device__ __forceinline__ void cover(const int* __restrict__ off, int n, int l, int p, int& i0, int& i1) {
  i0 = 0;
  while (i0 < n && off[i0] + l <= p) ++i0;
  i1 = i0;
  while (i1 < n && off[i1] <= p) ++i1;
}

// One thread per V pixels of a row of the full image. A pixel inside exactly one tile is copied;
// otherwise eps = (sum_k w_k * eps_k) / (sum_k w_k) over the covering tiles in ascending k, in
// fp32 with the multiply and the add rounded separately (no fma contraction) and one division,
// which makes the result reproducible by a plain elementwise restatement.
template <int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ out,
                                                         const int* __restrict__ ys, const int* __restrict__ xs,
                                                         int ny, int nx, int H, int W, int th, int tw, int ov,
                                                         size_t n) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Wv = W / V;
  const int x0 = (int)(i % Wv) * V;
  const int y = (int)((i / Wv) % H);
  const int c = (int)((i / ((size_t)Wv * H)) % 3);
  const int b = (int)(i / ((size_t)Wv * H * 3));
  int iy0, iy1, ix0, ix1;
  cover(ys, ny, th, y, iy0, iy1);
  cover(xs, nx, tw, x0, ix0, ix1);          // V == 4: the same tiles cover all four pixels
  const size_t tp = (size_t)th * tw;
  float acc[V], ws[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = ws[e] = 0.f;
  const bool single = (iy1 - iy0) * (ix1 - ix0) == 1;
  for (int iy = iy0; iy < iy1; ++iy) {
    const int ty = y - ys[iy];
    const int wy = ramp_w(ty, th, ov);
    for (int ix = ix0; ix < ix1; ++ix) {
      const int tx = x0 - xs[ix];
      const float* p = tiles + ((((size_t)b * ny + iy) * nx + ix) * 3 + c) * tp + (size_t)ty * tw + tx;
      float v[V];
      if constexpr (V == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
        v[0] = *p;
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (single) {
          acc[e] = v[e];
        } else {
          const float w = (float)(wy * ramp_w(tx + e, tw, ov));
          const float prod = w * v[e];
          acc[e] = acc[e] + prod;
          ws[e] = ws[e] + w;
        }
      }
    }
  }
  float o[V];
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = single ? acc[e] : acc[e] / ws[e];
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(out + i * 4) = f32x4{o[0], o[1], o[2], o[3]};
  else out[i] = o[0];
}

void tile_blend(const float* tiles, float* out, const int32_t* ys_dev, const int32_t* xs_dev,
                const int32_t* xs_host, int B, int ny, int nx, int H, int W, int th, int tw, int ov,
                hipStream_t st) {
  const bool v4 = grid_vec4(xs_host, nx, W, tw) && ((uintptr_t)tiles & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const size_t n = (size_t)B * 3 * H * (v4 ? W / 4 : W);
  const unsigned g = (unsigned)((n + 255) / 256);
  if (v4) tile_blend_kernel<4><<<g, 256, 0, st>>>(tiles, out, ys_dev, xs_dev, ny, nx, H, W, th, tw, ov, n);
  else tile_blend_kernel<1><<<g, 256, 0, st>>>(tiles, out, ys_dev, xs_dev, ny, nx, H, W, th, tw, ov, n);
}

__global__ void __launch_bounds__(256) rows_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          int ld, int k0, int per, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i / ld), c = (int)(i % ld);
  dst[i] = src[(size_t)((k0 + j) / per) * ld + c];
}

void rows_gather(const float* src, float* dst, int rows, int ld, int k0, int per, hipStream_t st) {
  const size_t n = (size_t)rows * ld;
  if (n) rows_gather_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, dst, ld, k0, per, n);
}

}  // namespace dac
