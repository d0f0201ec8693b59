// Objective scores of a free-running decode (include/sat_abi.h "synthesis scores"): the edit
// distance between predicted and true code sequences and the distortion along the dynamic-time-
// warping path between predicted and true mel frames.  Both are one dynamic programme over a
// Ta x Tb grid, D(i, j) = cost(i, j) (+) min of three predecessors, so both are ONE kernel template:
//
//   score_kernel<DTW>, grid = pairs, 256 threads.  One workgroup owns one pair and never looks at
//   another: no atomics, no flags, no spin loops; the only synchronisation is __syncthreads.
//
//   Rows (sequence a, the prediction) are taken in strips of kS = 256, one thread per row.  Inside
//   a strip the threads sweep the columns skewed: at sweep step s thread i is at column s - i.
//     D(i, j-1)    is the thread's own value of the step before (a register);
//     D(i-1, j)    is the value the lane above computed in the step before: one __shfl_up, or, for
//                  lane 0 of waves 1..3, the seam word lane 63 of the wave above left in LDS
//                  (double-buffered on the parity of s: one barrier per step);
//     D(i-1, j-1)  is what arrived as D(i-1, j) one step earlier (kept in a register).
//   Thread 0's "lane above" is the last row of the strip before: thread 255 of a strip that is not
//   the last stores its row to the pair's scratch row as it goes, and the next strip reads it back
//   kCT columns at a time.  One row is enough: column j is read at step <= j and overwritten at
//   step j + 255.  The first strip's row -1 is the recurrence's boundary (j + 1 for the edit
//   distance; +inf for DTW with D(-1, -1) = 0, which makes D(0, 0) = c(0, 0)).
//
//   The sweep runs in blocks of kCT = 32 steps.  Before each block every thread forms the 32 cell
//   costs it is about to use -- columns s0 - i .. s0 - i + 31 of its own row -- in registers:
//     codes  the window b[s0 - 255 .. s0 + 31] is staged in LDS; cost = (a_i != b_j);
//     DTW    c(i, j) = sqrt(sum_k (p_ik - t_jk)^2) in fp32 by direct differences.  The frames are
//            walked in chunks of kKC = 16 features: the thread holds its own frame's chunk in 16
//            registers, the same chunk of the 287 true frames of the window is staged in LDS, rows
//            kKP = 20 floats apart.  Lane i reads row (q - i + 255) as four ds_read_b128; a b128
//            read is served in groups of 16 lanes whose 16-byte slots must differ modulo 16: rows
//            80 bytes apart put lane i on slot (5 i + c) mod 16, a permutation of every group (a
//            16- or 80-float row, 64 or 320 bytes, puts lane i on slot 4 i mod 16: 4-way).  The
//            LDS cost does not depend on the frame width: 23 KB for any width up to 256.
//   D and the path length travel together (fp64 + int32): the minimum is taken in the order
//   diagonal, (i-1, j), (i, j-1) with strict <, so no back-trace and no Ta x Tb matrix exists.
//
//   A pair whose offsets are negative, decreasing, longer than max_len, past the end of the array
//   (or, for DTW, empty) is refused by its own workgroup before it reads anything else: -1 / NaN
//   for that pair, the error word set to 1 by a plain store (every refusing workgroup stores the
//   same value).
#include <type_traits>

#include "sat_common.h"

using namespace sat;

namespace {

constexpr int kS = 256;             // strip height = threads per workgroup
constexpr int kCT = 32;             // sweep steps per block
constexpr int kKC = 16;             // features per staged chunk
constexpr int kKP = 20;             // floats between window rows in LDS (80 B: see above)
constexpr int kWin = kS + kCT;      // window rows staged (kS + kCT - 1 are read)
constexpr int kMaxLen = 16384;
constexpr int kMaxWidth = 256;

struct ScoreP {
  const void* a; const void* b;
  const int64_t* aoff; const int64_t* boff;
  int64_t na, nb;                   // symbols / frames the arrays hold
  void* out; int32_t* out_len; int32_t* err;
  char* scratch; int64_t stride;    // bytes of scratch per pair
  int width, max_len;
};

inline int64_t pair_stride(int max_len) { return ((int64_t)max_len * 12 + 255) / 256 * 256; }

template <bool DTW>
__global__ void __launch_bounds__(kS) score_kernel(ScoreP p) {
  using V = std::conditional_t<DTW, double, int>;
  using C = std::conditional_t<DTW, float, int>;
  __shared__ V seam_v[2][kS / 64];
  __shared__ int seam_n[2][kS / 64];
  __shared__ V bnd_v[kCT];
  __shared__ int bnd_n[kCT];
  __shared__ __align__(16) int32_t win_raw[DTW ? kWin * kKP : kWin];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pair = blockIdx.x;
  const int64_t oa = p.aoff[pair], ea = p.aoff[pair + 1];
  const int64_t ob = p.boff[pair], eb = p.boff[pair + 1];
  const int64_t least = DTW ? 1 : 0;
  const bool ok = oa >= 0 && ea >= oa && ea - oa <= p.max_len && ea <= p.na && ea - oa >= least &&
                  ob >= 0 && eb >= ob && eb - ob <= p.max_len && eb <= p.nb && eb - ob >= least;
  if (!ok) {                                            // uniform over the workgroup
    if (tid == 0) {
      if (DTW) {
        reinterpret_cast<double*>(p.out)[pair] = __longlong_as_double(0x7FF8000000000000LL);
        p.out_len[pair] = -1;
      } else {
        reinterpret_cast<int32_t*>(p.out)[pair] = -1;
      }
      *p.err = 1;
    }
    return;
  }
  const int Ta = (int)(ea - oa), Tb = (int)(eb - ob);
  if (!DTW && (Ta == 0 || Tb == 0)) {
    if (tid == 0) reinterpret_cast<int32_t*>(p.out)[pair] = Ta + Tb;
    return;
  }
  V kFar = 0;                                           // DTW's boundary value
  if constexpr (DTW) kFar = INFINITY;
  V* row_v = reinterpret_cast<V*>(p.scratch + pair * p.stride);
  int* row_n = reinterpret_cast<int*>(p.scratch + pair * p.stride + (int64_t)p.max_len * 8);

  for (int r0 = 0; r0 < Ta; r0 += kS) {
    const int rows = min(kS, Ta - r0);
    const bool last = r0 + kS >= Ta;
    const int r = r0 + tid;
    const bool live = tid < rows;
    // D(r, -1), and for thread 0 D(r0 - 1, -1); the other threads' diagonal arrives from the
    // lane above while they are still waiting for their first column
    V cur = DTW ? kFar : (V)(r + 1), diag = DTW ? ((r == 0) ? (V)0 : kFar) : (V)r0;
    int curn = 0, diagn = 0;
    int av = 0;
    if (!DTW && live) av = reinterpret_cast<const int32_t*>(p.a)[oa + r];
    if (lane == 63) { seam_v[1][wave] = cur; seam_n[1][wave] = 0; }

    const int nsteps = Tb + rows - 1;
    for (int s0 = 0; s0 < nsteps; s0 += kCT) {
      // row r0 - 1 at columns s0 .. s0 + kCT - 1 (thread 0's lane above)
      if (tid < kCT) {
        const int j = s0 + tid;
        V v = DTW ? kFar : (V)(j + 1);
        int n = 0;
        if (r0 > 0 && j < Tb) {
          v = row_v[j];
          if (DTW) n = row_n[j];
        }
        bnd_v[tid] = v;
        bnd_n[tid] = n;
      }
      C cost[kCT];
      if (!DTW) {
        const int32_t* b = reinterpret_cast<const int32_t*>(p.b);
        for (int w = tid; w < kWin; w += kS) {
          const int j = s0 - (kS - 1) + w;
          win_raw[w] = (j >= 0 && j < Tb) ? b[ob + j] : -1;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kCT; ++q) cost[q] = (C)(av != win_raw[q - tid + kS - 1] ? 1 : 0);
      } else {
        const float* pa = reinterpret_cast<const float*>(p.a);
        const float* tb = reinterpret_cast<const float*>(p.b);
        float* win = reinterpret_cast<float*>(win_raw);
        float acc[kCT];
#pragma unroll
        for (int q = 0; q < kCT; ++q) acc[q] = 0.f;
        for (int k0 = 0; k0 < p.width; k0 += kKC) {
          if (k0 > 0) __syncthreads();                  // the chunk before has been read
          for (int e = tid; e < kWin * kKC; e += kS) {
            const int w = e / kKC, k = e % kKC;
            const int j = s0 - (kS - 1) + w, kk = k0 + k;
            float v = 0.f;
            if (j >= 0 && j < Tb && kk < p.width) v = tb[(ob + j) * p.width + kk];
            win[w * kKP + k] = v;
          }
          float pr[kKC];
#pragma unroll
          for (int k = 0; k < kKC; ++k) {
            const int kk = k0 + k;
            pr[k] = (live && kk < p.width) ? pa[(oa + r) * p.width + kk] : 0.f;
          }
          __syncthreads();
          if (live) {
#pragma unroll
            for (int q = 0; q < kCT; ++q) {
              const float4* t4 = reinterpret_cast<const float4*>(win + (q - tid + kS - 1) * kKP);
#pragma unroll
              for (int c = 0; c < kKC / 4; ++c) {
                const float4 t = t4[c];
                const float d0 = pr[4 * c] - t.x, d1 = pr[4 * c + 1] - t.y;
                const float d2 = pr[4 * c + 2] - t.z, d3 = pr[4 * c + 3] - t.w;
                acc[q] = fmaf(d0, d0, acc[q]);
                acc[q] = fmaf(d1, d1, acc[q]);
                acc[q] = fmaf(d2, d2, acc[q]);
                acc[q] = fmaf(d3, d3, acc[q]);
              }
            }
          }
        }
#pragma unroll
        for (int q = 0; q < kCT; ++q) cost[q] = (C)sqrtf(acc[q]);
      }

#pragma unroll
      for (int q = 0; q < kCT; ++q) {
        const int s = s0 + q, j = s - tid;
        V up = __shfl_up(cur, 1, 64);
        int upn = DTW ? __shfl_up(curn, 1, 64) : 0;
        if (lane == 0) {
          if (tid == 0) {
            up = bnd_v[q];
            upn = bnd_n[q];
          } else {
            up = seam_v[(s & 1) ^ 1][wave - 1];
            upn = seam_n[(s & 1) ^ 1][wave - 1];
          }
        }
        if (live && j >= 0 && j < Tb) {
          if (DTW) {
            V best = diag;
            int bn = diagn;
            if (up < best) { best = up; bn = upn; }
            if (cur < best) { best = cur; bn = curn; }
            cur = (V)cost[q] + best;
            curn = bn + 1;
          } else {
            cur = (V)min((int)diag + (int)cost[q], min((int)up, (int)cur) + 1);
          }
          if (!last && tid == kS - 1) {
            row_v[j] = cur;
            if (DTW) row_n[j] = curn;
          }
        }
        diag = up;
        diagn = upn;
        if (lane == 63) {
          seam_v[s & 1][wave] = cur;
          seam_n[s & 1][wave] = curn;
        }
        __syncthreads();
      }
    }
    if (last && tid == rows - 1) {
      if (DTW) {
        reinterpret_cast<double*>(p.out)[pair] = (double)cur;
        p.out_len[pair] = curn;
      } else {
        reinterpret_cast<int32_t*>(p.out)[pair] = (int32_t)cur;
      }
    }
  }
}

inline bool aligned_to(const void* ptr, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0;
}

}  // namespace

extern "C" int64_t sat_score_scratch_bytes(int32_t pairs, int32_t max_len) {
  if (pairs < 1 || max_len < 1 || max_len > kMaxLen) return SAT_ERR_ARGUMENT;
  return (int64_t)pairs * pair_stride(max_len);
}

#define SAT_SCORE_COMMON(name, a, na, aoff, b, nb, boff, out)                                    \
  SAT_CHECK_ARG(pairs >= 1, name ": pairs %d < 1", pairs);                                       \
  SAT_CHECK_ARG(max_len >= 1 && max_len <= kMaxLen, name ": max_len %d outside 1..%d", max_len,  \
                kMaxLen);                                                                        \
  SAT_CHECK_ARG(a && aoff && b && boff && out && err && scratch, name ": null pointer");         \
  SAT_CHECK_ARG(na >= 0 && nb >= 0, name ": a negative array size");                             \
  SAT_CHECK_ARG(scratch_bytes >= (int64_t)pairs * pair_stride(max_len),                          \
                name ": scratch of %lld bytes, %lld needed", (long long)scratch_bytes,           \
                (long long)((int64_t)pairs * pair_stride(max_len)));                             \
  SAT_CHECK_ARG(aligned_to(a, 4) && aligned_to(b, 4) && aligned_to(err, 4),                      \
                name ": an array or err is not 4-byte aligned");                                 \
  SAT_CHECK_ARG(aligned_to(aoff, 8) && aligned_to(boff, 8) && aligned_to(scratch, 8),            \
                name ": offsets or scratch are not 8-byte aligned")

extern "C" int sat_edit_distance(const int32_t* a, int64_t n_a, const int64_t* a_off,
                                 const int32_t* b, int64_t n_b, const int64_t* b_off,
                                 int32_t pairs, int32_t max_len, int32_t* distance, int32_t* err,
                                 void* scratch, int64_t scratch_bytes, void* stream) {
  SAT_SCORE_COMMON("sat_edit_distance", a, n_a, a_off, b, n_b, b_off, distance);
  SAT_CHECK_ARG(aligned_to(distance, 4), "sat_edit_distance: distance is not 4-byte aligned");
  ScoreP p{};
  p.a = a; p.b = b; p.aoff = a_off; p.boff = b_off; p.na = n_a; p.nb = n_b;
  p.out = distance; p.err = err; p.scratch = static_cast<char*>(scratch);
  p.stride = pair_stride(max_len); p.width = 1; p.max_len = max_len;
  hipLaunchKernelGGL(score_kernel<false>, dim3(pairs), dim3(kS), 0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_edit_distance");
  return SAT_OK;
}

extern "C" int sat_dtw_distortion(const float* p_frames, int64_t n_p, const int64_t* p_off,
                                  const float* t_frames, int64_t n_t, const int64_t* t_off,
                                  int32_t width, int32_t pairs, int32_t max_len, double* cost,
                                  int32_t* path_len, int32_t* err, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  SAT_CHECK_ARG(width >= 1 && width <= kMaxWidth, "sat_dtw_distortion: width %d outside 1..%d",
                width, kMaxWidth);
  SAT_SCORE_COMMON("sat_dtw_distortion", p_frames, n_p, p_off, t_frames, n_t, t_off, cost);
  SAT_CHECK_ARG(path_len, "sat_dtw_distortion: null pointer");
  SAT_CHECK_ARG(aligned_to(cost, 8) && aligned_to(path_len, 4),
                "sat_dtw_distortion: cost is not 8-byte or path_len not 4-byte aligned");
  ScoreP p{};
  p.a = p_frames; p.b = t_frames; p.aoff = p_off; p.boff = t_off; p.na = n_p; p.nb = n_t;
  p.out = cost; p.out_len = path_len; p.err = err; p.scratch = static_cast<char*>(scratch);
  p.stride = pair_stride(max_len); p.width = width; p.max_len = max_len;
  hipLaunchKernelGGL(score_kernel<true>, dim3(pairs), dim3(kS), 0, as_stream(stream), p);
  SAT_LAUNCH_CHECK("sat_dtw_distortion");
  return SAT_OK;
}
