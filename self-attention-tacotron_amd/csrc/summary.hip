// Training-summary images (sat_amd/summary.py): float sources -> 8-bit grayscale canvases.
//
// Every plotted source is contiguous along what becomes the image's ROW axis (alignment history
// A[t][b][n], self-attention P[b][h][q][k], mel X[b][t][m]): element (r, c) of image i sits at
// src[base[i] + c * col_stride + r].  Two launches per source, each over all its images:
//   sat_image_minmax  per-image min / max of the finite pixels of the crop + a non-finite count
//   sat_image_render  quantise, transpose through a padded LDS tile, write the row-flipped crop
// The crop lengths are device arrays; the kernels clamp them to the canvas and keep every read
// inside src[0, src_n), so no device value can move an access out of bounds.
#include "sat_common.h"

namespace sat {
namespace {

constexpr int kTile = 32;       // tile edge; 256 threads move one 32 x 32 tile
constexpr int kThreads = 256;

struct ImageSrc {
  const float* src;
  int64_t src_n;
  const int64_t* base;
  const int32_t* rows;
  const int32_t* cols;
  int64_t col_stride;
  int32_t Rmax, Cmax;
};

__device__ __forceinline__ bool finite_bits(float x) {
  return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 16-byte lanes need every column start of the image on a 16-byte boundary
__device__ __forceinline__ bool image_vec(const ImageSrc& s, int64_t base) {
  return ((reinterpret_cast<uintptr_t>(s.src + base) & 15) == 0) && ((s.col_stride & 3) == 0);
}

// v[0..n) = src[off .. off+n), n <= 4: one 16-byte load where it is whole and aligned, else the
// scalar tail; elements outside src[0, src_n) read as 0
__device__ __forceinline__ void load_quad(const ImageSrc& s, int64_t off, int n, bool vec,
                                          float v[4]) {
  if (vec && n == 4 && off >= 0 && off + 4 <= s.src_n) {
    const float4 q = *reinterpret_cast<const float4*>(s.src + off);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t o = off + j;
    v[j] = (j < n && o >= 0 && o < s.src_n) ? s.src[o] : 0.f;
  }
}

// one workgroup per image: threads walk the crop in quads along the contiguous row axis
__global__ __launch_bounds__(kThreads) void image_minmax_kernel(ImageSrc s,
                                                                float* __restrict__ minmax,
                                                                int32_t* __restrict__ nonfinite) {
  __shared__ float s_lo[kThreads / kWave], s_hi[kThreads / kWave];
  __shared__ int s_bad[kThreads / kWave];
  const int i = blockIdx.x;
  const int rows = clampi(s.rows[i], s.Rmax), cols = clampi(s.cols[i], s.Cmax);
  const int64_t base = s.base[i];
  const bool vec = image_vec(s, base);
  const int nq = (rows + 3) / 4;
  const int64_t total = (int64_t)cols * nq;
  float lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  for (int64_t e = threadIdx.x; e < total; e += kThreads) {
    const int c = (int)(e / nq), r = 4 * (int)(e - (int64_t)c * nq);
    const int n = min(4, rows - r);
    float v[4];
    load_quad(s, base + c * s.col_stride + r, n, vec, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        if (finite_bits(v[j])) {
          lo = fminf(lo, v[j]);
          hi = fmaxf(hi, v[j]);
        } else {
          ++bad;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    bad += __shfl_xor(bad, o, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_lo[w] = lo;
    s_hi[w] = hi;
    s_bad[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / kWave; ++k) {
      lo = fminf(lo, s_lo[k]);
      hi = fmaxf(hi, s_hi[k]);
      bad += s_bad[k];
    }
    if (!(lo <= hi)) lo = hi = 0.f;      // no finite pixel (or an empty crop)
    minmax[2 * i] = lo;
    minmax[2 * i + 1] = hi;
    nonfinite[i] = bad;
  }
}

// q = floor(255 * (x - lo) / (hi - lo) + 0.5) clamped to 0..255, each operation rounded to fp32
// on its own (no contraction), so the host statement of the formula reproduces it
__device__ __forceinline__ unsigned quantise(float x, float lo, float hi) {
  if (!finite_bits(x) || !(hi > lo)) return 0u;
  const float t = __fadd_rn(__fdiv_rn(__fmul_rn(255.f, __fsub_rn(x, lo)), __fsub_rn(hi, lo)), 0.5f);
  if (!(t > 0.f)) return 0u;             // also a NaN from an overflowing range
  return t >= 255.f ? 255u : (unsigned)floorf(t);
}

// grid (column tiles, row tiles, images).  Load: 8 threads take one source column's 32 rows as
// 16-byte quads (contiguous along r); store: 8 threads take one canvas line's 32 columns as
// packed 4-byte words (contiguous along c).  The tile is [column][row] with 33-word lines: in
// both phases a 32-lane half touches 32 different banks of the 32-bank ds_write_b32 /
// ds_read_b32 (bank = (col + row) mod 32 with col over 4 values and row over multiples of 4, or
// the transpose of that).
__global__ __launch_bounds__(kThreads) void image_render_kernel(ImageSrc s,
                                                                const float* __restrict__ minmax,
                                                                uint8_t* __restrict__ canvas) {
  __shared__ float tile[kTile][kTile + 1];
  const int i = blockIdx.z;
  const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
  const int rows = clampi(s.rows[i], s.Rmax), cols = clampi(s.cols[i], s.Cmax);
  const float lo = minmax[2 * i], hi = minmax[2 * i + 1];
  const int64_t base = s.base[i];
  {
    const int cl = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int c = c0 + cl, r = r0 + 4 * q;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < cols && r < rows)
      load_quad(s, base + c * s.col_stride + r, min(4, rows - r), image_vec(s, base), v);
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[cl][4 * q + j] = v[j];
  }
  __syncthreads();
  const int rl = threadIdx.x >> 3, cq = threadIdx.x & 7;
  const int r = r0 + rl, c = c0 + 4 * cq;
  if (r >= s.Rmax || c >= s.Cmax) return;
  // source row 0 is the crop's bottom line; lines below the crop keep their place (all zero)
  const int line = r < rows ? rows - 1 - r : r;
  unsigned px[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    px[j] = (r < rows && c + j < cols) ? quantise(tile[4 * cq + j][rl], lo, hi) : 0u;
  uint8_t* out = canvas + ((int64_t)i * s.Rmax + line) * s.Cmax + c;
  if (c + 4 <= s.Cmax && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(out) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
    for (int j = 0; j < 4 && c + j < s.Cmax; ++j) out[j] = (uint8_t)px[j];
  }
}

int check_images(const char* what, const float* src, int64_t src_n, const int64_t* base,
                 const int32_t* rows, const int32_t* cols, int64_t col_stride, int32_t n_images,
                 int32_t Rmax, int32_t Cmax, const int32_t* rows_host, const int32_t* cols_host) {
  SAT_CHECK_ARG(src && base && rows && cols, "%s: null pointer", what);
  SAT_CHECK_ARG(src_n >= 0 && col_stride >= 0 && n_images >= 0 && Rmax >= 0 && Cmax >= 0,
                "%s: negative size", what);
  SAT_CHECK_ARG(n_images <= 65535, "%s: at most 65535 images per launch", what);
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & 3) == 0, "%s: src not 4-byte aligned", what);
  for (int i = 0; i < n_images; ++i) {
    if (rows_host)
      SAT_CHECK_ARG(rows_host[i] >= 0 && rows_host[i] <= Rmax,
                    "%s: rows[%d] = %d outside the canvas (Rmax %d)", what, i, rows_host[i], Rmax);
    if (cols_host)
      SAT_CHECK_ARG(cols_host[i] >= 0 && cols_host[i] <= Cmax,
                    "%s: cols[%d] = %d outside the canvas (Cmax %d)", what, i, cols_host[i], Cmax);
  }
  return SAT_OK;
}

}  // namespace
}  // namespace sat

using namespace sat;

extern "C" int sat_image_minmax(const float* src, int64_t src_n, const int64_t* base,
                                const int32_t* rows, const int32_t* cols, int64_t col_stride,
                                int32_t n_images, int32_t Rmax, int32_t Cmax,
                                const int32_t* rows_host, const int32_t* cols_host, float* minmax,
                                int32_t* nonfinite, void* stream) {
  const int rc = check_images("sat_image_minmax", src, src_n, base, rows, cols, col_stride,
                              n_images, Rmax, Cmax, rows_host, cols_host);
  if (rc != SAT_OK) return rc;
  SAT_CHECK_ARG(minmax && nonfinite, "sat_image_minmax: null output");
  if (n_images == 0) return SAT_OK;
  const ImageSrc s{src, src_n, base, rows, cols, col_stride, Rmax, Cmax};
  hipLaunchKernelGGL(image_minmax_kernel, dim3(n_images), dim3(kThreads), 0, as_stream(stream), s,
                     minmax, nonfinite);
  SAT_LAUNCH_CHECK("sat_image_minmax");
  return SAT_OK;
}

extern "C" int sat_image_render(const float* src, int64_t src_n, const int64_t* base,
                                const int32_t* rows, const int32_t* cols, int64_t col_stride,
                                int32_t n_images, int32_t Rmax, int32_t Cmax,
                                const int32_t* rows_host, const int32_t* cols_host,
                                const float* minmax, uint8_t* canvas, void* stream) {
  const int rc = check_images("sat_image_render", src, src_n, base, rows, cols, col_stride,
                              n_images, Rmax, Cmax, rows_host, cols_host);
  if (rc != SAT_OK) return rc;
  SAT_CHECK_ARG(minmax && canvas, "sat_image_render: null pointer");
  SAT_CHECK_ARG(ceil_div(Rmax, kTile) <= 65535, "sat_image_render: Rmax too large");
  if (n_images == 0 || Rmax == 0 || Cmax == 0) return SAT_OK;
  const ImageSrc s{src, src_n, base, rows, cols, col_stride, Rmax, Cmax};
  hipLaunchKernelGGL(image_render_kernel,
                     dim3(ceil_div(Cmax, kTile), ceil_div(Rmax, kTile), n_images), dim3(kThreads),
                     0, as_stream(stream), s, minmax, canvas);
  SAT_LAUNCH_CHECK("sat_image_render");
  return SAT_OK;
}
