// Distortion metrics of reconstructions against their inputs (include/vrvq.h "Distortion
// metrics"): SI-SDR, SI-SNR, SNR and L1 per row, the numbers of models/utils.py:91-129
// cal_metrics (torchmetrics' formulas for fp32 input), from seven fp64 sums per row.
//
// Two launches, no atomics. The first streams both rows once in fixed chunks of
// VRVQ_METRICS_CHUNK samples, one 256-thread workgroup per (chunk, row), and stores the chunk's
// seven partial sums; the second adds a row's chunk partials and evaluates the formulas. Which
// thread adds which sample, and in which order, is a function of the sample's index in its row
// alone: not of the row's address (loads are 16 bytes wide at 4-byte alignment, so no row needs
// a head of its own), not of the other rows, the batch or the device. A row's bits therefore do
// not depend on what else is in the launch.
//
// Summation chains (the accuracy bound of DESIGN.md §4 rests on none exceeding 4096 terms):
//   per thread   MET_GROUPS * 4 = 64 terms in sequence            (chunk_kernel, the k / j loops)
//   lanes        a 6-level xor tree                                (wave_tree)
//   waves        MET_WAVES = 4 terms in sequence                   (chunk_kernel, after the barrier)
//   chunks       per lane ceil(chunks / 64) terms in sequence, then the 6-level tree
//                (finish_kernel); chunks <= 64 * 4096 is checked by the entry point, which is
//                samples <= MET_MAX_SAMPLES = 2^32
#include "common.h"

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_WAVES = MET_THREADS / 64;
constexpr int MET_CHUNK = VRVQ_METRICS_CHUNK;
constexpr int MET_GROUPS = MET_CHUNK / (MET_THREADS * 4);  // float4 groups per thread: 16
constexpr int MET_BATCH = 8;                               // groups loaded ahead of their use
constexpr int MET_SUMS = 7;
constexpr long long MET_MAX_CHUNKS = 64LL * 4096;
constexpr long long MET_MAX_SAMPLES = MET_MAX_CHUNKS * MET_CHUNK;  // 2^32
static_assert(MET_CHUNK % (MET_THREADS * 4 * MET_BATCH) == 0, "whole batches per chunk");
static_assert(MET_GROUPS * 4 <= 4096 && MET_WAVES <= 4096, "summation-chain condition");

// Four floats at 4-byte alignment: one global_load_dwordx4 (the hardware asks dword alignment of
// a multi-dword global load), whatever (row * samples) % 4 is.
typedef float met_f4 __attribute__((ext_vector_type(4), aligned(4)));

struct Sums {
  double v[MET_SUMS];  // sum p, t, p t, p^2, t^2, |p - t|, (p - t)^2
};

// One sample. p t, p^2 and t^2 of fp32 values are exact in fp64, so fma(p, t, acc) is
// acc + p * t with the one rounding of the add; d * d is not exact and takes the fma's single
// rounding. All of it in fp64.
__device__ __forceinline__ void add_sample(Sums& s, float pf, float tf) {
  const double p = (double)pf, t = (double)tf, d = p - t;
  s.v[0] += p;
  s.v[1] += t;
  s.v[2] = fma(p, t, s.v[2]);
  s.v[3] = fma(p, p, s.v[3]);
  s.v[4] = fma(t, t, s.v[4]);
  s.v[5] += fabs(d);
  s.v[6] = fma(d, d, s.v[6]);
}

__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ long long row_length(const long long* __restrict__ lengths, int ref_row,
                                                long long samples) {
  if (!lengths) return samples;
  const long long n = lengths[ref_row];
  return n < 0 ? 0 : (n > samples ? samples : n);
}

// workspace[row][chunk][7]: the sums over samples [chunk * MET_CHUNK, ...) of the row, below its
// length. Thread x owns samples k * 1024 + 4 x + j of the chunk (k < 16, j < 4) and adds them in
// (k, j) order.
__global__ __launch_bounds__(MET_THREADS) void metrics_chunk_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, int ref_rows, long long samples,
    const long long* __restrict__ lengths, double* __restrict__ ws) {
  __shared__ double part[MET_WAVES][MET_SUMS];
  const int row = blockIdx.y, rrow = row % ref_rows;
  const long long chunk = blockIdx.x, chunks = gridDim.x;
  const long long n = row_length(lengths, rrow, samples);
  const long long base = chunk * MET_CHUNK;
  // samples of this chunk that count: uniform over the workgroup
  const int nv = (int)(n - base < 0 ? 0 : (n - base > MET_CHUNK ? MET_CHUNK : n - base));
  const float* __restrict__ p = est + (size_t)row * samples + base;
  const float* __restrict__ t = ref + (size_t)rrow * samples + base;
  Sums s = {};
  if (nv == MET_CHUNK) {
    // Full chunk: MET_BATCH independent 16-byte loads of each row in flight per thread before
    // the first is used (2 x 8 x 16 B; a grid of a few hundred workgroups leaves about one wave
    // per SIMD, so the loads in flight per wave are what hides the latency).
#pragma unroll
    for (int k0 = 0; k0 < MET_GROUPS; k0 += MET_BATCH) {
      met_f4 a[MET_BATCH], b[MET_BATCH];
#pragma unroll
      for (int k = 0; k < MET_BATCH; ++k) {
        const int e = (k0 + k) * (MET_THREADS * 4) + (int)threadIdx.x * 4;
        a[k] = *reinterpret_cast<const met_f4*>(p + e);
        b[k] = *reinterpret_cast<const met_f4*>(t + e);
      }
      // keep the batch's loads ahead of its arithmetic (the scheduler otherwise sinks them to
      // save registers and leaves about half as many in flight)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < MET_BATCH; ++k) {  // chain: 4 of the thread's 64 terms per group
        add_sample(s, a[k].x, b[k].x);
        add_sample(s, a[k].y, b[k].y);
        add_sample(s, a[k].z, b[k].z);
        add_sample(s, a[k].w, b[k].w);
      }
    }
  } else if (nv > 0) {
    // The row's last chunk: the same samples per thread in the same order, each behind its own
    // bound (nothing at or past the length is read).
    for (int k = 0; k < MET_GROUPS; ++k) {
      const int e = k * (MET_THREADS * 4) + (int)threadIdx.x * 4;
      if (e >= nv) break;
      if (e + 4 <= nv) {
        const met_f4 a = *reinterpret_cast<const met_f4*>(p + e);
        const met_f4 b = *reinterpret_cast<const met_f4*>(t + e);
        add_sample(s, a.x, b.x);
        add_sample(s, a.y, b.y);
        add_sample(s, a.z, b.z);
        add_sample(s, a.w, b.w);
      } else {
        for (int j = 0; e + j < nv; ++j) add_sample(s, p[e + j], t[e + j]);
      }
    }
  }
  // lanes: xor tree; waves: 4 terms in wave order. Every thread reaches the barrier.
#pragma unroll
  for (int i = 0; i < MET_SUMS; ++i) s.v[i] = wave_tree(s.v[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < MET_SUMS; ++i) part[threadIdx.x >> 6][i] = s.v[i];
  }
  __syncthreads();
  if (threadIdx.x < MET_SUMS) {
    double tot = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < MET_WAVES; ++w) tot += part[w][threadIdx.x];
    ws[((size_t)row * chunks + chunk) * MET_SUMS + threadIdx.x] = tot;
  }
}

// max(x, 0) that keeps NaN (fmax would return 0)
__device__ __forceinline__ double clamp0(double x) { return x < 0.0 ? 0.0 : x; }

// 10 log10((S + eps) / (N + eps)), S = alpha^2 tt, N = max(S - 2 alpha pt + pp, 0),
// alpha = (pt + eps) / (tt + eps)
__device__ __forceinline__ double si_ratio_db(double pt, double pp, double tt, double eps) {
  const double alpha = (pt + eps) / (tt + eps);
  const double S = (alpha * alpha) * tt;
  const double N = clamp0((S - (2.0 * alpha) * pt) + pp);
  return 10.0 * log10((S + eps) / (N + eps));
}

// One wave per row: lane l adds chunks l, l + 64, ... in sequence (<= 4096 terms, see the entry
// point), then the xor tree over the lanes; lane 0 evaluates the formulas.
__global__ __launch_bounds__(64) void metrics_finish_kernel(
    const double* __restrict__ ws, long long chunks, int ref_rows, long long samples,
    const long long* __restrict__ lengths, double* __restrict__ metrics,
    double* __restrict__ moments) {
  const int row = blockIdx.x;
  const double* __restrict__ w = ws + (size_t)row * chunks * MET_SUMS;
  double s[MET_SUMS] = {};
  for (long long c = threadIdx.x; c < chunks; c += 64) {
#pragma unroll
    for (int i = 0; i < MET_SUMS; ++i) s[i] += w[c * MET_SUMS + i];
  }
#pragma unroll
  for (int i = 0; i < MET_SUMS; ++i) s[i] = wave_tree(s[i]);
  if (threadIdx.x != 0) return;
  const long long n = row_length(lengths, row % ref_rows, samples);
  const double nd = (double)n, eps = 0x1p-23;  // float32 eps, torchmetrics' for fp32 input
  const double sp = s[0], st = s[1], pt = s[2], pp = s[3], tt = s[4];
  if (moments) {
#pragma unroll
    for (int i = 0; i < MET_SUMS; ++i) moments[(size_t)row * 8 + i] = s[i];
    moments[(size_t)row * 8 + 7] = nd;
  }
  // the centred moments of SI-SNR (zero_mean); n = 0 has nothing to centre
  const double cpt = n > 0 ? pt - sp * st / nd : pt;
  const double cpp = n > 0 ? clamp0(pp - sp * sp / nd) : pp;
  const double ctt = n > 0 ? clamp0(tt - st * st / nd) : tt;
  double* m = metrics + (size_t)row * 4;
  m[0] = si_ratio_db(pt, pp, tt, eps);
  m[1] = si_ratio_db(cpt, cpp, ctt, eps);
  m[2] = 10.0 * log10((tt + eps) / (s[6] + eps));
  m[3] = s[5] / nd;  // NaN for n = 0
}

long long chunks_of(long long samples) { return (samples + MET_CHUNK - 1) / MET_CHUNK; }

bool shape_ok(int rows, long long samples) {
  // grid.y carries the rows; the chunk sum's chain bounds the samples (file header)
  return rows > 0 && rows <= 65535 && samples > 0 && samples <= MET_MAX_SAMPLES;
}

}  // namespace

extern "C" int vrvq_signal_metrics_workspace(int rows, long long samples, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && shape_ok(rows, samples));
  *bytes = (long long)rows * chunks_of(samples) * MET_SUMS * (long long)sizeof(double);
  return VRVQ_OK;
}

extern "C" int vrvq_signal_metrics(const float* est, const float* ref, int rows, int ref_rows,
                                   long long samples, const long long* lengths, double* metrics,
                                   double* moments, void* workspace, long long workspace_bytes,
                                   vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(est && ref && metrics && workspace);
  VRVQ_CHECK_ARG(shape_ok(rows, samples) && ref_rows > 0 && rows % ref_rows == 0);
  const long long chunks = chunks_of(samples);
  VRVQ_CHECK_ARG(workspace_bytes >= (long long)rows * chunks * MET_SUMS * (long long)sizeof(double));
  VRVQ_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  double* ws = static_cast<double*>(workspace);
  hipLaunchKernelGGL(metrics_chunk_kernel, dim3((unsigned)chunks, (unsigned)rows),
                     dim3(MET_THREADS), 0, as_stream(stream), est, ref, ref_rows, samples, lengths,
                     ws);
  int rc = vrvq_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)rows), dim3(64), 0, as_stream(stream),
                     ws, chunks, ref_rows, samples, lengths, metrics, moments);
  return vrvq_launch_status();
}
