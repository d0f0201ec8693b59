// Synthesis figures (sat_amd/plots.py): one colour canvas per utterance, composed in one launch.
//
// A figure is n_panel boxes of Hp x Wp pixels stacked top to bottom, each a nearest-neighbour
// resampling of one crop (addressed as summary.hip addresses an image: element (r, c) at
// src[base + c * col_stride + r]) through a colour table, with a colour bar strip at its right
// and margins of a background colour; include/sat_abi.h states every formula.
//
// Mapping.  The canvas [n_fig][Hfig][Wfig][3] is one contiguous byte string whose base may sit at
// any byte address, and a pixel is 3 bytes, so neither a line nor a pixel starts on a word in
// general.  The kernel therefore ignores lines when it stores: the string is cut at the first
// 4-byte boundary into `head` (< 4) bytes, nfull chunks of 12 bytes, and a tail (< 12 bytes).  One
// thread forms one chunk -- three whole words in registers -- and stores it with one 12-byte
// store; lane l of a wave writes bytes [12 l, 12 l + 12) of a 768-byte run, so a wave's store
// instruction covers whole, consecutive words and no word is touched by two lanes.  12 is a
// multiple of 3, so every chunk starts at the same byte of a pixel (phase = head mod 3, a launch
// constant and a template argument): a chunk is 4 pixels at phase 0, parts of 5 otherwise.  One
// more thread writes the head and the tail with byte stores (at most 14).  Every byte has exactly
// one writer; nothing is cleared first.  The grid depends on the geometry alone.
//
// The reads are gathers: neighbouring pixels of a line are neighbouring source COLUMNS, col_stride
// floats apart.  A source is small beside the canvas (a [T'][B][N] history against Hp x Wp x 3
// bytes per panel) and every 64-byte line of it is read again by the lanes of the next canvas
// lines, so these come from L2; the canvas stores are the traffic that reaches memory.
#include "sat_common.h"

namespace sat {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxTables = 8;

struct FigArgs {
  const SatFigurePanel* panels;
  const uint8_t* lut;
  uint8_t* canvas;
  int64_t total;       // canvas bytes
  int64_t nfull;       // 12-byte chunks after the head
  int32_t head;        // bytes before the first 4-byte boundary
  int32_t n_panel, Hp, Wp, m, cb, n_tables;
  int32_t Hfig, Wfig;
  uint32_t rows32, cols32;   // crops up to these keep the index arithmetic in 32 bits
  uint32_t background;
};

__device__ __forceinline__ bool finite_bits(float x) {
  return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u;
}

// sat_image_render's q (summary.hip): every operation rounded to fp32 on its own, no contraction
__device__ __forceinline__ unsigned quantise(float x, float lo, float hi) {
  if (!finite_bits(x) || !(hi > lo)) return 0u;
  const float t = __fadd_rn(__fdiv_rn(__fmul_rn(255.f, __fsub_rn(x, lo)), __fsub_rn(hi, lo)), 0.5f);
  if (!(t > 0.f)) return 0u;
  return t >= 255.f ? 255u : (unsigned)floorf(t);
}

// ((2 i + 1) * n) / (2 * L) for 0 <= i < L, n > 0
__device__ __forceinline__ int64_t resample(int i, int n, int L, uint32_t n32) {
  if ((uint32_t)n <= n32) return ((2u * (uint32_t)i + 1u) * (uint32_t)n) / (2u * (uint32_t)L);
  return (int64_t)(((uint64_t)(2 * (int64_t)i + 1) * (uint64_t)n) / (uint64_t)(2 * (int64_t)L));
}

// what one canvas line needs of its panel; panel < 0: a margin line
struct Line {
  int fig, y;
  int panel;
  const float* src;
  int64_t src_n, off_r, col_stride;   // off_r = base + r
  float lo, hi;
  int cols;
  bool empty;
  const uint32_t* table;              // LDS: 256 packed colours
  uint32_t bar;                       // the colour bar's colour on this line
};

__device__ __forceinline__ void load_line(const FigArgs& a, const uint32_t* s_lut, int fig, int y,
                                          Line& L) {
  L.fig = fig;
  L.y = y;
  L.panel = -1;
  const int yy = y - a.m;
  if (yy < 0) return;
  const int k = yy / (a.Hp + a.m), py = yy - k * (a.Hp + a.m);
  if (k >= a.n_panel || py >= a.Hp) return;
  L.panel = k;
  const SatFigurePanel p = a.panels[(int64_t)fig * a.n_panel + k];
  const int t = p.table < 0 ? 0 : (p.table >= a.n_tables ? a.n_tables - 1 : p.table);
  L.table = s_lut + 256 * t;
  L.bar = L.table[a.Hp == 1 ? 0 : 255 - (255 * py) / (a.Hp - 1)];
  L.empty = p.rows <= 0 || p.cols <= 0;
  if (L.empty) return;
  L.src = p.src;
  L.src_n = p.src_n;
  L.col_stride = p.col_stride;
  L.cols = p.cols;
  L.off_r = p.base + resample(a.Hp - 1 - py, p.rows, a.Hp, a.rows32);
  L.lo = p.minmax[0];
  L.hi = p.minmax[1];
}

// packed colour (R | G << 8 | B << 16) of pixel x of the line
__device__ __forceinline__ uint32_t pixel(const FigArgs& a, const Line& L, int x) {
  if (L.panel < 0) return a.background;
  const int bx = x - a.m;
  if (bx < 0) return a.background;
  if (bx < a.Wp) {
    if (L.empty) return L.table[0];
    const int64_t off = L.off_r + resample(bx, L.cols, a.Wp, a.cols32) * L.col_stride;
    const float v = (off >= 0 && off < L.src_n) ? L.src[off] : 0.f;
    return L.table[quantise(v, L.lo, L.hi)];
  }
  const int sx = bx - a.Wp - a.m;
  return (sx >= 0 && sx < a.cb) ? L.bar : a.background;
}

// pixel index -> (fig, y, x)
__device__ __forceinline__ void locate(const FigArgs& a, int64_t P, int& fig, int& y, int& x) {
  const uint32_t HW = (uint32_t)a.Hfig * (uint32_t)a.Wfig;
  uint32_t rem;
  if (P <= 0xFFFFFFFFll) {
    fig = (int)((uint32_t)P / HW);
    rem = (uint32_t)P - (uint32_t)fig * HW;
  } else {
    fig = (int)(P / HW);
    rem = (uint32_t)(P - (int64_t)fig * HW);
  }
  y = (int)(rem / (uint32_t)a.Wfig);
  x = (int)(rem - (uint32_t)y * (uint32_t)a.Wfig);
}

struct alignas(4) Chunk {
  uint32_t w[3];
};

template <int PHASE>
__global__ __launch_bounds__(kThreads) void figure_kernel(FigArgs a) {
  __shared__ uint32_t s_lut[kMaxTables * 256];
  for (int e = threadIdx.x; e < a.n_tables * 256; e += kThreads)
    s_lut[e] = a.lut[3 * e] | ((uint32_t)a.lut[3 * e + 1] << 8) | ((uint32_t)a.lut[3 * e + 2] << 16);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t > a.nfull) return;
  Line L;
  int fig, y, x;
  if (t < a.nfull) {
    constexpr int kPix = PHASE ? 5 : 4;
    const int64_t k0 = a.head + 12 * t;          // canvas + k0 is 4-byte aligned; k0 % 3 == PHASE
    locate(a, (k0 - PHASE) / 3, fig, y, x);
    load_line(a, s_lut, fig, y, L);
    uint32_t col[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      col[j] = pixel(a, L, x);
      if (j + 1 < kPix && ++x == a.Wfig) {
        x = 0;
        if (++y == a.Hfig) {
          y = 0;
          ++fig;
        }
        load_line(a, s_lut, fig, y, L);
      }
    }
    Chunk c;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = PHASE + 4 * w + j;         // byte b of the pixel run: pixel b / 3, channel b % 3
        word |= ((col[b / 3] >> (8 * (b % 3))) & 255u) << (8 * j);
      }
      c.w[w] = word;
    }
    *reinterpret_cast<Chunk*>(a.canvas + k0) = c;
    return;
  }
  // the edges: bytes [0, head) and [head + 12 nfull, total)
  const int64_t tail0 = a.head + 12 * a.nfull;
  const int n_edge = a.head + (int)(a.total - tail0);
  L.fig = -1;
  L.y = -1;
  for (int e = 0; e < n_edge; ++e) {
    const int64_t k = e < a.head ? e : tail0 + (e - a.head);
    const int64_t P = k / 3;
    locate(a, P, fig, y, x);
    if (fig != L.fig || y != L.y) load_line(a, s_lut, fig, y, L);
    a.canvas[k] = (uint8_t)(pixel(a, L, x) >> (8 * (int)(k - 3 * P)));
  }
}

}  // namespace
}  // namespace sat

using namespace sat;

extern "C" int sat_figure_render(const SatFigure* d, void* stream) {
  SAT_CHECK_ARG(d, "sat_figure_render: null descriptor");
  SAT_CHECK_ARG(d->panels && d->lut && d->canvas, "sat_figure_render: null pointer");
  SAT_CHECK_ARG(d->n_fig >= 0 && d->n_panel >= 0 && d->margin >= 0 && d->cbar >= 0,
                "sat_figure_render: negative size");
  SAT_CHECK_ARG(d->Hp >= 1 && d->Wp >= 1, "sat_figure_render: Hp and Wp must be at least 1");
  SAT_CHECK_ARG((int64_t)d->n_fig * d->n_panel <= 65535,
                "sat_figure_render: at most 65535 panels per launch");
  SAT_CHECK_ARG(d->n_tables >= 1 && d->n_tables <= kMaxTables,
                "sat_figure_render: n_tables %d outside 1..%d", d->n_tables, kMaxTables);
  SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->lut) & 3) == 0,
                "sat_figure_render: lut not 4-byte aligned");
  const int64_t Hfig = (int64_t)d->n_panel * d->Hp + ((int64_t)d->n_panel + 1) * d->margin;
  const int64_t Wfig = (int64_t)d->Wp + d->cbar + 3 * (int64_t)d->margin;
  SAT_CHECK_ARG(Hfig < (1ll << 31) && Wfig < (1ll << 31) && Hfig * Wfig < (1ll << 31),
                "sat_figure_render: a figure of %lld x %lld pixels is too large", (long long)Hfig,
                (long long)Wfig);
  if (d->panels_host) {
    for (int i = 0; i < d->n_fig * d->n_panel; ++i) {
      const SatFigurePanel& p = d->panels_host[i];
      SAT_CHECK_ARG(p.src && p.minmax, "sat_figure_render: panel %d: null pointer", i);
      SAT_CHECK_ARG((reinterpret_cast<uintptr_t>(p.src) & 3) == 0 &&
                        (reinterpret_cast<uintptr_t>(p.minmax) & 3) == 0,
                    "sat_figure_render: panel %d: src or minmax not 4-byte aligned", i);
      SAT_CHECK_ARG(p.src_n >= 0 && p.col_stride >= 0, "sat_figure_render: panel %d: negative size",
                    i);
      SAT_CHECK_ARG(p.table >= 0 && p.table < d->n_tables,
                    "sat_figure_render: panel %d: table %d outside 0..%d", i, p.table,
                    d->n_tables - 1);
    }
  }
  const int64_t total = (int64_t)d->n_fig * Hfig * Wfig * 3;
  if (total == 0) return SAT_OK;
  FigArgs a{};
  a.panels = d->panels;
  a.lut = d->lut;
  a.canvas = d->canvas;
  a.total = total;
  a.head = (int32_t)std::min<int64_t>((4 - (reinterpret_cast<uintptr_t>(d->canvas) & 3)) & 3, total);
  a.nfull = (total - a.head) / 12;
  a.n_panel = d->n_panel;
  a.Hp = d->Hp;
  a.Wp = d->Wp;
  a.m = d->margin;
  a.cb = d->cbar;
  a.n_tables = d->n_tables;
  a.Hfig = (int32_t)Hfig;
  a.Wfig = (int32_t)Wfig;
  a.rows32 = 0xFFFFFFFFu / (2u * (uint32_t)d->Hp);
  a.cols32 = 0xFFFFFFFFu / (2u * (uint32_t)d->Wp);
  a.background = d->background & 0xFFFFFFu;
  // one thread per 12-byte chunk and one for the edges; total / 12 >= nfull whatever the base's
  // alignment, so the grid is a function of the geometry alone
  const int64_t blocks = (total / 12 + 1 + kThreads - 1) / kThreads;
  SAT_CHECK_ARG(blocks <= 0x7FFFFFFFll, "sat_figure_render: canvas too large");
  const dim3 grid((unsigned)blocks), block(kThreads);
  switch (a.head % 3) {
    case 0: hipLaunchKernelGGL(figure_kernel<0>, grid, block, 0, as_stream(stream), a); break;
    case 1: hipLaunchKernelGGL(figure_kernel<1>, grid, block, 0, as_stream(stream), a); break;
    default: hipLaunchKernelGGL(figure_kernel<2>, grid, block, 0, as_stream(stream), a); break;
  }
  SAT_LAUNCH_CHECK("sat_figure_render");
  return SAT_OK;
}
