// Rate control for the VBR quantizer: bits of a clip as a function of the level, and the level
// that meets a bit budget, from the importance map alone (codes and latents do not depend on the
// level). Every total is an integer, so the results do not depend on the reduction order.
//
// Frame count, the expression of the RVQ kernels (rvq.hip, mask of (imp * level) * nq):
//   s = fl(fl(imp * level) * (float)nq)
//   n(imp, level) = s >= 0 ? (int)floorf(fminf(s, nq - 1)) + 1 : 0        (NaN -> 0)
// Bits of a frame: cum[n], the prefix sum of bits[nq].
#include "common.h"

namespace {

constexpr int RATE_THREADS = 256;
constexpr int RATE_WAVES = RATE_THREADS / 64;
constexpr int RATE_MAX_NQ = 32;
constexpr int RATE_LV = 4;  // levels per workgroup of the curve kernel
// The solver keeps a group's importance values in registers when the group has at most
// RATE_KEEP * 256 = 4096 elements (16 VGPRs per thread; 47 one-second clips of 87 frames). A
// larger group is read again from global memory in every iteration (<= 33 passes over data
// that stays in L2), 4096 elements at a time through the same number of registers.
constexpr int RATE_KEEP = 16;

__device__ __forceinline__ int frame_count(float imp, float level, int nq) {
  const float s = (imp * level) * (float)nq;  // two roundings (-ffp-contract=off)
  return s >= 0.0f ? (int)floorf(fminf(s, (float)(nq - 1))) + 1 : 0;
}

// cum[0..nq] in LDS from bits[nq]; the caller's next barrier publishes it.
__device__ __forceinline__ void fill_cum(const int* __restrict__ bits, int nq, long long* cum) {
  if (threadIdx.x == 0) {
    long long c = 0;
    cum[0] = 0;
    for (int i = 0; i < nq; ++i) {
      c += bits[i];
      cum[i + 1] = c;
    }
  }
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Sum over the workgroup, returned to every thread. part is one of two alternating
// [RATE_WAVES] buffers: a buffer is written again only two calls later, after the barrier of
// the call between them, which no thread passes before all have read this call's sums. One
// barrier per call, reached by all 256 threads.
__device__ __forceinline__ long long block_sum(long long v, long long* part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int w = 0; w < RATE_WAVES; ++w) t += part[w];
  return t;
}

// total_bits[b][l] for RATE_LV levels of one row per workgroup.
__global__ __launch_bounds__(RATE_THREADS) void rate_curve_kernel(
    const float* __restrict__ imp, int T, int nq, const int* __restrict__ bits,
    const float* __restrict__ levels, int L, long long* __restrict__ total_bits) {
  __shared__ long long cum[RATE_MAX_NQ + 1];
  __shared__ long long part[2][RATE_WAVES];
  const int b = blockIdx.x, l0 = blockIdx.y * RATE_LV;
  fill_cum(bits, nq, cum);
  float lv[RATE_LV];
#pragma unroll
  for (int j = 0; j < RATE_LV; ++j) lv[j] = levels[min(l0 + j, L - 1)];
  __syncthreads();
  const float* row = imp + (size_t)b * T;
  long long acc[RATE_LV] = {0, 0, 0, 0};
  for (int t = threadIdx.x; t < T; t += RATE_THREADS) {
    const float v = row[t];
#pragma unroll
    for (int j = 0; j < RATE_LV; ++j) acc[j] += cum[frame_count(v, lv[j], nq)];
  }
#pragma unroll
  for (int j = 0; j < RATE_LV; ++j) {
    const long long tot = block_sum(acc[j], part[j & 1]);
    if (threadIdx.x == 0 && l0 + j < L) total_bits[(size_t)b * L + l0 + j] = tot;
  }
}

// Bits of the group at one level, in every thread. KEEP: the values are in v[], else in global
// memory at x[0..n).
template <bool KEEP>
__device__ __forceinline__ long long group_bits(const float (&v)[RATE_KEEP],
                                                const float* __restrict__ x, long long n,
                                                float level, int nq, const long long* cum,
                                                long long* part) {
  long long acc = 0;
  if (KEEP) {
    // slots past the group hold NaN (0 bits); the uniform test skips them
#pragma unroll
    for (int k = 0; k < RATE_KEEP; ++k)
      if ((long long)k * RATE_THREADS < n) acc += cum[frame_count(v[k], level, nq)];
  } else {
    // RATE_KEEP independent loads in flight per thread (the pass is bound by load latency: one
    // wave per SIMD). Addresses are clamped and the value replaced afterwards, so no load sits
    // under a branch.
    for (long long base = 0; base < n; base += (long long)RATE_KEEP * RATE_THREADS) {
      float w[RATE_KEEP];
#pragma unroll
      for (int k = 0; k < RATE_KEEP; ++k) {
        const long long e = base + k * RATE_THREADS + (long long)threadIdx.x;
        const float val = x[e < n ? e : n - 1];
        w[k] = e < n ? val : __uint_as_float(0x7fc00000u);  // NaN: 0 bits
      }
#pragma unroll
      for (int k = 0; k < RATE_KEEP; ++k) acc += cum[frame_count(w[k], level, nq)];
    }
  }
  return block_sum(acc, part);
}

// The largest level in [lo, hi] whose bits are <= budget: bisection on the bit patterns of the
// two positive floats (they order like their uint32 patterns). Every thread computes the same
// totals, so every decision is uniform and each thread runs the same number of barriers. The
// interval [lo_u, hi_u] at least halves per pass and is narrower than 2^31, so the loop ends
// within 31 passes for any input (its bound of 32 is never the reason it ends).
template <bool KEEP>
__device__ __forceinline__ void solve_group(const float (&v)[RATE_KEEP],
                                            const float* __restrict__ x, long long n, int nq,
                                            const long long* cum, long long (*part)[RATE_WAVES],
                                            long long budget, float level_lo, float level_hi,
                                            float* level_out, long long* total_out, int* status) {
  int call = 0;
  const long long t_lo = group_bits<KEEP>(v, x, n, level_lo, nq, cum, part[call++ & 1]);
  int st;
  float lvl;
  long long tot;
  if (t_lo > budget) {  // every frame costs at least one code
    st = 1;
    lvl = level_lo;
    tot = t_lo;
  } else {
    const long long t_hi = group_bits<KEEP>(v, x, n, level_hi, nq, cum, part[call++ & 1]);
    if (t_hi <= budget) {
      st = 2;
      lvl = level_hi;
      tot = t_hi;
    } else {
      unsigned lo_u = __float_as_uint(level_lo), hi_u = __float_as_uint(level_hi);
      tot = t_lo;
      for (int it = 0; it < 32 && hi_u - lo_u > 1u; ++it) {
        const unsigned mid = lo_u + ((hi_u - lo_u) >> 1);
        const long long t_mid =
            group_bits<KEEP>(v, x, n, __uint_as_float(mid), nq, cum, part[call++ & 1]);
        if (t_mid <= budget) {
          lo_u = mid;
          tot = t_mid;
        } else {
          hi_u = mid;
        }
      }
      st = 0;
      lvl = __uint_as_float(lo_u);
    }
  }
  if (threadIdx.x == 0) {
    *level_out = lvl;
    *total_out = tot;
    *status = st;
  }
}

// One workgroup per group of rows group_off[g] .. group_off[g + 1].
__global__ __launch_bounds__(RATE_THREADS) void rate_solve_kernel(
    const float* __restrict__ imp, int B, int T, int nq, const int* __restrict__ bits,
    const int* __restrict__ group_off, const long long* __restrict__ budget, float level_lo,
    float level_hi, float* __restrict__ level_out, long long* __restrict__ total_out,
    int* __restrict__ status) {
  __shared__ long long cum[RATE_MAX_NQ + 1];
  __shared__ long long part[2][RATE_WAVES];
  const int g = blockIdx.x;
  const int r0 = group_off[g], r1 = group_off[g + 1];
  // r0, r1 are uniform over the workgroup: both early returns are taken by all threads or none,
  // before the first barrier.
  if (r0 < 0 || r1 < r0 || r1 > B) {  // not monotone / outside the map: nothing is read
    if (threadIdx.x == 0) {
      level_out[g] = level_lo;
      total_out[g] = 0;
      status[g] = -1;
    }
    return;
  }
  if (r0 == r1) {  // empty group: any level fits
    if (threadIdx.x == 0) {
      level_out[g] = level_hi;
      total_out[g] = 0;
      status[g] = 2;
    }
    return;
  }
  fill_cum(bits, nq, cum);
  const long long n = (long long)(r1 - r0) * T;  // [r0 T, r1 T) lies inside [0, B T)
  const float* x = imp + (size_t)r0 * T;
  float v[RATE_KEEP];
  const bool keep = n <= (long long)RATE_KEEP * RATE_THREADS;
#pragma unroll
  for (int k = 0; k < RATE_KEEP; ++k) {
    const int e = k * RATE_THREADS + (int)threadIdx.x;
    v[k] = keep && e < n ? x[e] : __uint_as_float(0x7fc00000u);  // NaN: no codes, cum[0] = 0 bits
  }
  __syncthreads();  // cum
  if (keep)
    solve_group<true>(v, x, n, nq, cum, part, budget[g], level_lo, level_hi, level_out + g,
                      total_out + g, status + g);
  else
    solve_group<false>(v, x, n, nq, cum, part, budget[g], level_lo, level_hi, level_out + g,
                       total_out + g, status + g);
}

__global__ __launch_bounds__(256) void scale_imp_rows_kernel(const float* __restrict__ imp,
                                                             long long n, int T,
                                                             const float* __restrict__ levels,
                                                             float* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n;
       e += (long long)gridDim.x * 256)
    out[e] = imp[e] * levels[e / T];
}

bool level_range_ok(float lo, float hi) {
  return lo > 0.0f && lo <= hi && hi <= 3.402823466e+38f;  // finite, positive, ordered (no NaN)
}

}  // namespace

extern "C" int vrvq_rate_curve(const float* imp, int batch, int frames, int nq, const int* bits,
                               const float* levels, int n_levels, long long* total_bits,
                               vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(imp && bits && levels && total_bits && batch > 0 && frames > 0 && n_levels > 0);
  VRVQ_CHECK_ARG(nq > 0 && nq <= RATE_MAX_NQ);
  const int ly = (n_levels + RATE_LV - 1) / RATE_LV;
  VRVQ_CHECK_ARG(ly <= 65535);
  hipLaunchKernelGGL(rate_curve_kernel, dim3(batch, ly), dim3(RATE_THREADS), 0, as_stream(stream),
                     imp, frames, nq, bits, levels, n_levels, total_bits);
  return vrvq_launch_status();
}

extern "C" int vrvq_rate_solve(const float* imp, int batch, int frames, int nq, const int* bits,
                               const int* group_off, int n_groups, const long long* budget,
                               float level_lo, float level_hi, float* level_out,
                               long long* total_out, int* status, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(imp && bits && group_off && budget && level_out && total_out && status);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && n_groups > 0 && nq > 0 && nq <= RATE_MAX_NQ);
  VRVQ_CHECK_ARG(level_range_ok(level_lo, level_hi));
  hipLaunchKernelGGL(rate_solve_kernel, dim3(n_groups), dim3(RATE_THREADS), 0, as_stream(stream),
                     imp, batch, frames, nq, bits, group_off, budget, level_lo, level_hi,
                     level_out, total_out, status);
  return vrvq_launch_status();
}

extern "C" int vrvq_scale_imp_rows(const float* imp, int batch, int frames, const float* levels,
                                   float* out, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(imp && levels && out && batch > 0 && frames > 0);
  const long long n = (long long)batch * frames;
  long long g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(scale_imp_rows_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream),
                     imp, n, frames, levels, out);
  return vrvq_launch_status();
}
