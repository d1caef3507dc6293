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

// ---------------------------------------------------------------------------------------------
// Capped rate control: a packet is a run of P frames of one row (NP = ceil(T / P) per row, the
// last one short). Launch 1 solves every packet on its own against packet_budget[p] (its cap);
// launch 2 solves each group's level lambda over bits(min(lambda, cap)) and writes the packets'
// levels, totals and states. The caps travel from launch 1 to launch 2 in packet_level itself.

// solve_group's bisection over any total: the largest level in [lo, hi] with bits_at(level) <=
// budget. solve_group keeps its own loop: built on this one, rate_solve_kernel compiles to other
// code (6 more VGPRs), and a commit that adds a path leaves the existing one as it was.
// bits_at(level) returns the same total in every thread that shares its barriers or shuffles, so
// every decision is uniform over them and each runs the same number of calls. The interval
// [lo_u, hi_u] at least halves per pass and is narrower than 2^31, so the loop ends within 31
// passes for any input (its bound of 32 is never the reason it ends).
template <class F>
__device__ __forceinline__ void bisect_level(F&& bits_at, long long budget, float level_lo,
                                             float level_hi, float& lvl, long long& tot, int& st) {
  const long long t_lo = bits_at(level_lo);
  if (t_lo > budget) {  // every frame costs at least one code
    st = 1;
    lvl = level_lo;
    tot = t_lo;
  } else {
    const long long t_hi = bits_at(level_hi);
    if (t_hi <= budget) {
      st = 2;
      lvl = level_hi;
      tot = t_hi;
    } else {
      unsigned lo_u = __float_as_uint(level_lo), hi_u = __float_as_uint(level_hi);
      tot = t_lo;
      for (int it = 0; it < 32 && hi_u - lo_u > 1u; ++it) {
        const unsigned mid = lo_u + ((hi_u - lo_u) >> 1);
        const long long t_mid = bits_at(__uint_as_float(mid));
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
}

// A wave holds a packet of up to CAP_KEEP * 64 = 256 frames in registers; a longer one is read
// again in every pass, 256 frames at a time.
constexpr int CAP_KEEP = 4;

// Bits of frames x[0..nf) at one level, in every lane of the wave (no barrier). KEEP: the frames
// are in v[] (NaN past nf).
template <bool KEEP>
__device__ __forceinline__ long long packet_bits(const float (&v)[CAP_KEEP],
                                                 const float* __restrict__ x, int nf, float level,
                                                 int nq, const long long* cum) {
  const int lane = threadIdx.x & 63;
  long long acc = 0;
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < CAP_KEEP; ++k)
      if (k * 64 < nf) acc += cum[frame_count(v[k], level, nq)];
  } else {
    // as group_bits: clamped addresses, the value replaced afterwards, no load under a branch
    for (long long base = 0; base < nf; base += CAP_KEEP * 64) {
      float w[CAP_KEEP];
#pragma unroll
      for (int k = 0; k < CAP_KEEP; ++k) {
        const long long f = base + k * 64 + lane;
        const float val = x[f < nf ? f : nf - 1];
        w[k] = f < nf ? val : __uint_as_float(0x7fc00000u);  // NaN: 0 bits
      }
#pragma unroll
      for (int k = 0; k < CAP_KEEP; ++k) acc += cum[frame_count(w[k], level, nq)];
    }
  }
  return wave_sum(acc);
}

// Launch 1: one wave per packet, RATE_WAVES packets per workgroup. Writes the packet's cap, its
// total at the cap and state 1 (infeasible) or 2: what a row that belongs to no valid group keeps.
__global__ __launch_bounds__(RATE_THREADS) void rate_caps_kernel(
    const float* __restrict__ imp, int B, int T, int P, int NP, int nq,
    const int* __restrict__ bits, const long long* __restrict__ packet_budget, float level_lo,
    float level_hi, float* __restrict__ packet_level, long long* __restrict__ packet_total,
    int* __restrict__ packet_status) {
  __shared__ long long cum[RATE_MAX_NQ + 1];
  fill_cum(bits, nq, cum);
  __syncthreads();  // the only barrier: everything below is per wave
  const long long pk = (long long)blockIdx.x * RATE_WAVES + (threadIdx.x >> 6);
  if (pk >= (long long)B * NP) return;  // uniform over the wave
  const long long row = pk / NP;
  const int p = (int)(pk - row * NP);
  const int f0 = p * P;  // < T
  const int nf = min(P, T - f0);
  const float* x = imp + (size_t)row * T + f0;
  const int lane = threadIdx.x & 63;
  const bool keep = nf <= CAP_KEEP * 64;
  float v[CAP_KEEP];
#pragma unroll
  for (int k = 0; k < CAP_KEEP; ++k) {
    const int f = k * 64 + lane;
    v[k] = keep && f < nf ? x[f] : __uint_as_float(0x7fc00000u);
  }
  const long long budget = packet_budget[p];
  float lvl;
  long long tot;
  int st;
  if (keep)
    bisect_level([&](float level) { return packet_bits<true>(v, x, nf, level, nq, cum); }, budget,
                 level_lo, level_hi, lvl, tot, st);
  else
    bisect_level([&](float level) { return packet_bits<false>(v, x, nf, level, nq, cum); },
                 budget, level_lo, level_hi, lvl, tot, st);
  if (lane == 0) {
    packet_level[pk] = lvl;
    packet_total[pk] = tot;
    packet_status[pk] = st == 1 ? 1 : 2;
  }
}

// Bits of the group with every element at min(level, the cap of its packet), in every thread.
// KEEP: values and caps are in v[] and c[]; else the values are at x[0..n) (rows of T frames) and
// the caps at cap[row * NP + t / P], both read again.
template <bool KEEP>
__device__ __forceinline__ long long group_bits_capped(const float (&v)[RATE_KEEP],
                                                       const float (&c)[RATE_KEEP],
                                                       const float* __restrict__ x,
                                                       const float* cap, long long n, int T, int P,
                                                       int NP, float level, int nq,
                                                       const long long* cum, long long* part) {
  long long acc = 0;
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < RATE_KEEP; ++k)
      if ((long long)k * RATE_THREADS < n)
        acc += cum[frame_count(v[k], fminf(level, c[k]), nq)];
  } else {
    // (row, t) of the thread's element moves on by 256 elements per slot without a division
    // (unsigned: t + 256 stays below 2^32 for any T)
    const unsigned uT = T, uP = P, dq = RATE_THREADS / uT, dr = RATE_THREADS % uT;
    long long row = threadIdx.x / uT;
    unsigned t = threadIdx.x % uT;
    for (long long base = 0; base < n; base += (long long)RATE_KEEP * RATE_THREADS) {
      float w[RATE_KEEP], cw[RATE_KEEP];
#pragma unroll
      for (int k = 0; k < RATE_KEEP; ++k) {
        const long long e = base + k * RATE_THREADS + (long long)threadIdx.x;
        const float val = x[e < n ? e : n - 1];
        cw[k] = cap[e < n ? row * NP + t / uP : 0];
        w[k] = e < n ? val : __uint_as_float(0x7fc00000u);  // NaN: 0 bits
        row += dq;
        t += dr;
        if (t >= uT) {
          t -= uT;
          ++row;
        }
      }
#pragma unroll
      for (int k = 0; k < RATE_KEEP; ++k)
        acc += cum[frame_count(w[k], fminf(level, cw[k]), nq)];
    }
  }
  return block_sum(acc, part);
}

// Launch 2: one workgroup per group, as rate_solve_kernel, then one wave per packet of the
// group's rows for the packet outputs. Groups that share rows leave those rows' packet outputs
// to whichever workgroup writes last.
__global__ __launch_bounds__(RATE_THREADS) void rate_solve_capped_kernel(
    const float* __restrict__ imp, int B, int T, int P, int NP, int nq,
    const int* __restrict__ bits, const int* __restrict__ group_off,
    const long long* __restrict__ budget, float level_lo, float level_hi,
    float* __restrict__ level_out, long long* __restrict__ total_out, int* __restrict__ status,
    float* packet_level, long long* packet_total, int* packet_status) {
  __shared__ long long cum[RATE_MAX_NQ + 1];
  __shared__ long long part[2][RATE_WAVES];
  const int g = blockIdx.x;
  const int r0 = group_off[g], r1 = group_off[g + 1];
  // uniform over the workgroup and before the first barrier, as in rate_solve_kernel
  if (r0 < 0 || r1 < r0 || r1 > B) {
    if (threadIdx.x == 0) {
      level_out[g] = level_lo;
      total_out[g] = 0;
      status[g] = -1;
    }
    return;
  }
  if (r0 == r1) {
    if (threadIdx.x == 0) {
      level_out[g] = level_hi;
      total_out[g] = 0;
      status[g] = 2;
    }
    return;
  }
  fill_cum(bits, nq, cum);
  const long long n = (long long)(r1 - r0) * T;
  const float* x = imp + (size_t)r0 * T;
  float* cap = packet_level + (size_t)r0 * NP;  // launch 1 left the caps here
  float v[RATE_KEEP], c[RATE_KEEP];
  const bool keep = n <= (long long)RATE_KEEP * RATE_THREADS;
#pragma unroll
  for (int k = 0; k < RATE_KEEP; ++k) {
    const int e = k * RATE_THREADS + (int)threadIdx.x;  // < 4096
    const bool in = keep && e < n;
    v[k] = in ? x[e] : __uint_as_float(0x7fc00000u);  // NaN: no codes, cum[0] = 0 bits
    c[k] = in ? cap[(long long)(e / T) * NP + (e % T) / P] : level_lo;
  }
  __syncthreads();  // cum
  int call = 0, st;
  float lvl;
  long long tot;
  if (keep)
    bisect_level(
        [&](float level) {
          return group_bits_capped<true>(v, c, x, cap, n, T, P, NP, level, nq, cum,
                                         part[call++ & 1]);
        },
        budget[g], level_lo, level_hi, lvl, tot, st);
  else
    bisect_level(
        [&](float level) {
          return group_bits_capped<false>(v, c, x, cap, n, T, P, NP, level, nq, cum,
                                          part[call++ & 1]);
        },
        budget[g], level_lo, level_hi, lvl, tot, st);
  if (threadIdx.x == 0) {
    level_out[g] = lvl;
    total_out[g] = tot;
    status[g] = st;
  }
  // Packet outputs. Every thread passed the barrier of the last block_sum after its last read of
  // a cap, so the caps may be overwritten now; each packet is read and written by one wave. The
  // wave's (row, p) moves on by RATE_WAVES packets without a division.
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long npk = (long long)(r1 - r0) * NP;
  const int dq = RATE_WAVES / NP, dr = RATE_WAVES % NP;
  long long row = wave / NP;
  int p = wave % NP;
  const float none[CAP_KEEP] = {};  // packet_bits<false> reads the frames, not this
  for (long long k = wave; k < npk; k += RATE_WAVES) {
    const int f0 = p * P;
    const float cp = cap[k];
    const int st0 = packet_status[(size_t)r0 * NP + k];
    const float l = fminf(lvl, cp);
    const long long t_p =
        packet_bits<false>(none, x + (size_t)row * T + f0, min(P, T - f0), l, nq, cum);
    if (lane == 0) {
      cap[k] = l;
      packet_total[(size_t)r0 * NP + k] = t_p;
      packet_status[(size_t)r0 * NP + k] = st0 == 1 ? 1 : (cp < lvl ? 2 : 0);
    }
    row += dq;
    p += dr;
    if (p >= NP) {
      p -= NP;
      ++row;
    }
  }
}

__global__ __launch_bounds__(256) void scale_imp_packets_kernel(
    const float* __restrict__ imp, long long n, int T, int P, int NP,
    const float* __restrict__ packet_level, float* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n;
       e += (long long)gridDim.x * 256) {
    const long long row = e / T;
    out[e] = imp[e] * packet_level[row * NP + (int)(e - row * T) / P];
  }
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

extern "C" int vrvq_rate_solve_capped(const float* imp, int batch, int frames, int nq,
                                      const int* bits, const int* group_off, int n_groups,
                                      const long long* budget, const long long* packet_budget,
                                      int packet_frames, float level_lo, float level_hi,
                                      float* level_out, long long* total_out, int* status,
                                      float* packet_level, long long* packet_total,
                                      int* packet_status, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(imp && bits && group_off && budget && level_out && total_out && status);
  VRVQ_CHECK_ARG(packet_budget && packet_level && packet_total && packet_status);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && n_groups > 0 && nq > 0 && nq <= RATE_MAX_NQ);
  VRVQ_CHECK_ARG(packet_frames >= 1);
  VRVQ_CHECK_ARG(level_range_ok(level_lo, level_hi));
  const int np = (frames - 1) / packet_frames + 1;
  const long long wgs = ((long long)batch * np + RATE_WAVES - 1) / RATE_WAVES;
  VRVQ_CHECK_ARG(wgs <= 0x7fffffffLL);
  hipLaunchKernelGGL(rate_caps_kernel, dim3((unsigned)wgs), dim3(RATE_THREADS), 0,
                     as_stream(stream), imp, batch, frames, packet_frames, np, nq, bits,
                     packet_budget, level_lo, level_hi, packet_level, packet_total, packet_status);
  const int rc = vrvq_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(rate_solve_capped_kernel, dim3(n_groups), dim3(RATE_THREADS), 0,
                     as_stream(stream), imp, batch, frames, packet_frames, np, nq, bits, group_off,
                     budget, level_lo, level_hi, level_out, total_out, status, packet_level,
                     packet_total, packet_status);
  return vrvq_launch_status();
}

extern "C" int vrvq_scale_imp_packets(const float* imp, int batch, int frames,
                                      const float* packet_level, int packet_frames, float* out,
                                      vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(imp && packet_level && out && batch > 0 && frames > 0 && packet_frames >= 1);
  const long long n = (long long)batch * frames;
  long long g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(scale_imp_packets_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream),
                     imp, n, frames, packet_frames, (frames - 1) / packet_frames + 1, packet_level,
                     out);
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
