// Speaker vector into the decoder (models/models.py:72-83: speaker_embedding_projection_out_dim,
// speaker_embedd_to_decoder).  The reference tiles s [B][S] over the N encoder positions and
// concatenates it to both memories; the appended columns are constant over n, so every consumer
// sees either a per-utterance bias row (sat_rows_bias_fwd / _bwd) or s itself in the tail columns
// of a wider context row (sat_ctx_tail_fill) -- DESIGN.md "Speaker vector to the decoder".
// These run once per step or once per decode, outside every recurrence: plain one-pass kernels,
// 16 bytes per lane.
#include "sat_common.h"

using namespace sat;

namespace {

struct RowsBiasP {
  float* y; int64_t y_sb, y_sn;
  const float* bias; int64_t bias_sb;
  const int64_t* len;
  int B, N, C4;
};

// one float4 of Y per thread: Y[b][n][c4] += bias[b][c4] for n < len[b]
__global__ void __launch_bounds__(256) rows_bias_fwd_kernel(RowsBiasP p) {
  const int64_t total = (int64_t)p.B * p.N * p.C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % p.C4);
    const int64_t r = i / p.C4;
    const int n = (int)(r % p.N), b = (int)(r / p.N);
    if (p.len && n >= p.len[b]) continue;
    float4* y = reinterpret_cast<float4*>(p.y + b * p.y_sb + n * p.y_sn) + c4;
    const float4 v = reinterpret_cast<const float4*>(p.bias + b * p.bias_sb)[c4];
    float4 o = *y;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *y = o;
  }
}

struct RowsSumP {
  const float* dy; int64_t dy_sb, dy_sn;
  float* dbias; int64_t dbias_sb;
  const int64_t* len;
  int B, N, C4;
};

// One block per (utterance, 16 float4 columns): 16 row slices x 16 column groups.  Each slice
// sums its rows n = slice, slice + 16, .. in fp64, the 16 slices are then added in a fixed order
// by one thread per column group: no atomics, the same bits on every run.
__global__ void __launch_bounds__(256) rows_bias_bwd_kernel(RowsSumP p) {
  __shared__ double part[16][16][4];
  const int b = blockIdx.y;
  const int cg = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int c4 = blockIdx.x * 16 + cg;
  int rows = p.N;
  if (p.len) {
    const int64_t l = p.len[b];
    rows = l < 0 ? 0 : (l < p.N ? (int)l : p.N);
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c4 < p.C4) {
    const float* base = p.dy + b * p.dy_sb;
    for (int n = slice; n < rows; n += 16) {
      const float4 v = reinterpret_cast<const float4*>(base + n * p.dy_sn)[c4];
      a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
  }
  part[slice][cg][0] = a0; part[slice][cg][1] = a1;
  part[slice][cg][2] = a2; part[slice][cg][3] = a3;
  __syncthreads();
  if (slice == 0 && c4 < p.C4) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += part[k][cg][j];
    reinterpret_cast<float4*>(p.dbias + b * p.dbias_sb)[c4] =
        make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
  }
}

struct TailFillP {
  float* ctx; int64_t ctx_st, ctx_sb;
  const float* s; int64_t s_sb;
  int t0, t1, B, S4;
};

// ctx[t][b][col0 + j] = s[b][j] for t0 <= t < t1 (ctx already points at column col0)
__global__ void __launch_bounds__(256) ctx_tail_fill_kernel(TailFillP p) {
  const int64_t total = (int64_t)(p.t1 - p.t0) * p.B * p.S4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % p.S4);
    const int64_t r = i / p.S4;
    const int b = (int)(r % p.B);
    const int64_t t = p.t0 + r / p.B;
    reinterpret_cast<float4*>(p.ctx + t * p.ctx_st + b * p.ctx_sb)[j] =
        reinterpret_cast<const float4*>(p.s + b * p.s_sb)[j];
  }
}

inline unsigned grid_of(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

}  // namespace

extern "C" int sat_rows_bias_fwd(float* y, int64_t y_sb, int64_t y_sn, const float* bias,
                                 int64_t bias_sb, int32_t B, int32_t N, int32_t C,
                                 const int64_t* lengths, void* stream) {
  SAT_CHECK_ARG(B >= 0 && N >= 0 && C > 0, "sat_rows_bias_fwd: bad sizes");
  if (B == 0 || N == 0) return SAT_OK;
  SAT_CHECK_ARG(y && bias, "sat_rows_bias_fwd: null pointer");
  SAT_CHECK_ARG(aligned16(y) && aligned16(bias), "sat_rows_bias_fwd: operands must be 16-byte aligned");
  SAT_CHECK_ARG(C % 4 == 0 && y_sb % 4 == 0 && y_sn % 4 == 0 && bias_sb % 4 == 0,
                "sat_rows_bias_fwd: C and every stride must be multiples of 4");
  SAT_CHECK_ARG(y_sn >= C && bias_sb >= C, "sat_rows_bias_fwd: rows overlap");
  RowsBiasP p{y, y_sb, y_sn, bias, bias_sb, lengths, B, N, C / 4};
  hipLaunchKernelGGL(rows_bias_fwd_kernel, dim3(grid_of((int64_t)B * N * p.C4)), dim3(256), 0,
                     as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_rows_bias_fwd");
  return SAT_OK;
}

extern "C" int sat_rows_bias_bwd(const float* dy, int64_t dy_sb, int64_t dy_sn, float* dbias,
                                 int64_t dbias_sb, int32_t B, int32_t N, int32_t C,
                                 const int64_t* lengths, void* stream) {
  SAT_CHECK_ARG(B >= 0 && N >= 0 && C > 0, "sat_rows_bias_bwd: bad sizes");
  if (B == 0) return SAT_OK;
  SAT_CHECK_ARG(dbias && (dy || N == 0), "sat_rows_bias_bwd: null pointer");
  SAT_CHECK_ARG(aligned16(dy) && aligned16(dbias), "sat_rows_bias_bwd: operands must be 16-byte aligned");
  SAT_CHECK_ARG(C % 4 == 0 && dy_sb % 4 == 0 && dy_sn % 4 == 0 && dbias_sb % 4 == 0,
                "sat_rows_bias_bwd: C and every stride must be multiples of 4");
  SAT_CHECK_ARG(dbias_sb >= C, "sat_rows_bias_bwd: rows overlap");
  SAT_CHECK_ARG(B <= 65535, "sat_rows_bias_bwd: B <= 65535");
  RowsSumP p{dy, dy_sb, dy_sn, dbias, dbias_sb, lengths, B, N, C / 4};
  hipLaunchKernelGGL(rows_bias_bwd_kernel, dim3((p.C4 + 15) / 16, B), dim3(256), 0,
                     as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_rows_bias_bwd");
  return SAT_OK;
}

extern "C" int sat_ctx_tail_fill(float* ctx, int64_t ctx_st, int64_t ctx_sb, int32_t col0,
                                 const float* s, int64_t s_sb, int32_t t0, int32_t t1, int32_t B,
                                 int32_t S, void* stream) {
  SAT_CHECK_ARG(B >= 0 && S > 0 && col0 >= 0 && t0 >= 0 && t1 >= t0, "sat_ctx_tail_fill: bad sizes");
  if (B == 0 || t1 == t0) return SAT_OK;
  SAT_CHECK_ARG(ctx && s, "sat_ctx_tail_fill: null pointer");
  SAT_CHECK_ARG(aligned16(ctx) && aligned16(s), "sat_ctx_tail_fill: operands must be 16-byte aligned");
  SAT_CHECK_ARG(S % 4 == 0 && col0 % 4 == 0 && ctx_st % 4 == 0 && ctx_sb % 4 == 0 && s_sb % 4 == 0,
                "sat_ctx_tail_fill: S, col0 and every stride must be multiples of 4");
  SAT_CHECK_ARG(ctx_sb >= (int64_t)col0 + S && s_sb >= S, "sat_ctx_tail_fill: tail outside the row");
  TailFillP p{ctx + col0, ctx_st, ctx_sb, s, s_sb, t0, t1, B, S / 4};
  hipLaunchKernelGGL(ctx_tail_fill_kernel, dim3(grid_of((int64_t)(t1 - t0) * B * p.S4)), dim3(256),
                     0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_ctx_tail_fill");
  return SAT_OK;
}
