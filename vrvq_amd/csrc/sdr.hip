// BSS-eval SDR (include/vrvq.h "BSS SDR"): torchmetrics' signal_distortion_ratio, the "SDR" of
// models/utils.py:91-143 cal_metrics, per row and without a host sync. The estimate is projected
// onto the span of the F delayed copies of the reference; the ratio is the energy inside that
// span over the energy outside it. Everything in fp64.
//
// Three launches (four with zero_mean), no atomics:
//   mean     (zero_mean only) one workgroup per row: the row's mean over its length
//   corr     one workgroup per (row, chunk of VRVQ_SDR_CHUNK samples): the chunk's partial sums
//            of b[l] = sum t[i] p[i+l], l < F, of p^2 and of t p; the same for r[l] and sum t^2,
//            once per reference row (the reference against itself), not once per estimate
//   reduce   one workgroup per row: the chunk partials added in a fixed order, divided by the
//            clamped norms, load_diag added to r[0], NaN for the special rows
//   solve    one wave per (reference row, group of SDR_LT estimates): Levinson-Durbin on r with
//            the group's right-hand sides carried through the same recursion, then coh and the dB
//
// Which thread adds which (sample, lag) product, and in which order, is a function of the
// sample's index in its row and the lag alone; an estimate's recursion state is its own. A row's
// bits therefore do not depend on the other rows of the call, on how many estimates share its
// reference, or on the row's address.
//
// Summation chains (fp64, sequential terms): corr 128 samples per accumulator, 4 accumulators
// per wave, 4 waves; reduce 16 chunks per group, then the groups; solve 8 terms per lane, a
// 4-level tree over 16 lanes and 4 rows of lanes.
#include "common.h"

namespace {

constexpr int SDR_CHUNK = VRVQ_SDR_CHUNK;
constexpr int SDR_FMAX = 512;
constexpr int SDR_THREADS = 256;
constexpr int SDR_WAVES = SDR_THREADS / 64;
constexpr int SDR_J = 8;                                  // consecutive lags per lane: 64 * 8 = 512
constexpr int SDR_WAVE_SAMPLES = SDR_CHUNK / SDR_WAVES;   // 512 samples of the chunk per wave
constexpr int SDR_SEG = 128;                              // samples per accumulator chain
constexpr int SDR_PLOG = SDR_CHUNK + SDR_FMAX;            // p window: the chunk and its halo
constexpr int SDR_PPHYS = SDR_PLOG / 8 * 9;               // one pad double per 8: lane stride 9
constexpr int SDR_LT = 4;                                 // estimates per solve wave
constexpr int SDR_GROUP = 16;                             // chunks per reduce group
constexpr long long SDR_MAX_SAMPLES = 1LL << 32;
static_assert(SDR_J * 64 == SDR_FMAX && SDR_J == 8, "the lag tile covers filter_length <= 512");
static_assert(SDR_WAVE_SAMPLES % SDR_SEG == 0 && SDR_SEG % 8 == 0, "whole 8-sample blocks");
static_assert(SDR_WAVES * SDR_FMAX <= SDR_PPHYS, "the wave partials reuse the p window");

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double read_lane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// The sum over the 64 lanes, the same bits in every lane; all 64 lanes must be active. Four DPP
// levels inside each row of 16 lanes (lane ^ 1, lane ^ 2, the mirror of each half row, the mirror
// of the row: both partners of a level add the same two values), then the four rows in order.
// No LDS round trip: the solve's latency is this, 511 times over.
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return ((read_lane_f64(v, 0) + read_lane_f64(v, 16)) + read_lane_f64(v, 32)) +
         read_lane_f64(v, 48);
}

__device__ __forceinline__ long long row_length(const long long* __restrict__ lengths, int ref_row,
                                                long long samples) {
  if (!lengths) return samples;
  const long long n = lengths[ref_row];
  return n < 0 ? 0 : (n > samples ? samples : n);
}

// means[row] of the rows + ref_rows rows (the estimates, then the references) over their
// lengths; n = 0 gives 0. Thread x adds samples x + 256 k in runs of 64, the runs in order.
__global__ __launch_bounds__(SDR_THREADS) void sdr_mean_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, int rows, int ref_rows,
    long long samples, const long long* __restrict__ lengths, double* __restrict__ means) {
  __shared__ double part[SDR_WAVES];
  const int row = blockIdx.x;
  const bool is_ref = row >= rows;
  const int rrow = is_ref ? row - rows : row % ref_rows;
  const long long n = row_length(lengths, rrow, samples);
  const float* __restrict__ x = is_ref ? ref + (size_t)rrow * samples : est + (size_t)row * samples;
  double tot = 0.0;
  for (long long i0 = threadIdx.x; i0 < n; i0 += (long long)SDR_THREADS * 64) {
    double s = 0.0;
    for (int k = 0; k < 64; ++k) {
      const long long i = i0 + (long long)k * SDR_THREADS;
      if (i < n) s += (double)x[i];
    }
    tot += s;
  }
  tot = wave_sum(tot);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = ((part[0] + part[1]) + part[2]) + part[3];
    means[row] = n > 0 ? s / (double)n : 0.0;
  }
}

// part[row][chunk][F + 2]: for l < F the sum over the chunk's samples i (below the length) of
// t[i] p[i + l] (p[i + l] = 0 at and past the length), then the chunk's sums of p^2 and t p. Rows
// blockIdx.z = 0 are the estimates against their references, blockIdx.z = 1 the references
// against themselves (stored after the estimates' rows).
//
// Lane x of each wave owns the 8 lags 8 x .. 8 x + 7, wave w the chunk's samples 512 w .. 512 w
// + 511. Per sample one t (an LDS broadcast) and one new p enter a sliding window of 8 p values
// held in registers, and 8 FMAs use them: the loop is bound by the fp64 FMA rate, not by LDS.
// The p window is stored with one pad double after every 8, so the lanes' reads (8 doubles
// apart) fall 9 apart and on different banks. The other form, the plane tiled into
// v_mfma_f64_16x16x4_f64 products, was measured next to this one and is slower even before its
// diagonals are collected (tools/micro/sdr_corr_forms.hip, DESIGN.md "BSS SDR").
__global__ __launch_bounds__(SDR_THREADS) void sdr_corr_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, int rows, int ref_rows,
    long long samples, const long long* __restrict__ lengths, int F,
    const double* __restrict__ means, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double tl[SDR_CHUNK];
  __shared__ __attribute__((aligned(16))) double pl[SDR_PPHYS];
  __shared__ double sq[SDR_WAVES], tp[SDR_WAVES];
  const bool is_ref = blockIdx.z != 0;
  if (is_ref && (int)blockIdx.y >= ref_rows) return;
  const int rrow = is_ref ? (int)blockIdx.y : (int)blockIdx.y % ref_rows;
  const int row = is_ref ? rows + rrow : (int)blockIdx.y;
  const long long chunk = blockIdx.x, chunks = gridDim.x;
  const long long n = row_length(lengths, rrow, samples);
  const long long base = chunk * SDR_CHUNK;
  if (base >= n) return;  // uniform; the reduction adds only the chunks below the length
  const float* __restrict__ t = ref + (size_t)rrow * samples;
  const float* __restrict__ p = is_ref ? t : est + (size_t)row * samples;
  const double mt = means ? means[rows + rrow] : 0.0;
  const double mp = means ? means[row] : 0.0;
  const int tid = threadIdx.x;
  for (int i = tid; i < SDR_CHUNK; i += SDR_THREADS)
    tl[i] = base + i < n ? (double)t[base + i] - mt : 0.0;
  for (int i = tid; i < SDR_PLOG; i += SDR_THREADS)
    pl[i + (i >> 3)] = base + i < n ? (double)p[base + i] - mp : 0.0;
  __syncthreads();

  // the chunk's sums of p^2 and of t p (lag 0 once more, in the order of the energies: see
  // sdr_reduce_kernel): thread x adds samples x + 256 k in k order
  double ss = 0.0, st = 0.0;
#pragma unroll
  for (int k = 0; k < SDR_CHUNK / SDR_THREADS; ++k) {
    const int i = tid + k * SDR_THREADS;
    const double v = pl[i + (i >> 3)];
    ss = fma(v, v, ss);
    st = fma(tl[i], v, st);
  }
  ss = wave_sum(ss);
  st = wave_sum(st);

  const int wave = tid >> 6, lane = tid & 63;
  double tot[SDR_J];
#pragma unroll
  for (int j = 0; j < SDR_J; ++j) tot[j] = 0.0;
  for (int seg = 0; seg < SDR_WAVE_SAMPLES / SDR_SEG; ++seg) {
    const int ib = wave * SDR_WAVE_SAMPLES + seg * SDR_SEG;  // a multiple of 8
    // logical index ib + 8 lane of the p window, a multiple of 8: physical + (that / 8)
    const double* __restrict__ pb = pl + (ib + SDR_J * lane) + (ib >> 3) + lane;
    const double* __restrict__ tb = tl + ib;
    double acc[SDR_J], w[SDR_J];
#pragma unroll
    for (int j = 0; j < SDR_J; ++j) acc[j] = 0.0;
#pragma unroll
    for (int j = 0; j < SDR_J - 1; ++j) w[j] = pb[j];
    for (int blk = 0; blk < SDR_SEG / 8; ++blk) {
      const double* __restrict__ pq = pb + blk * 9;
      const double* __restrict__ tq = tb + blk * 8;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        // sample ib + 8 blk + s: its lag j needs p at window offset s + j, held in slot
        // (s + j) % 8; offset s + 7 is new (physical: + 1 past the first 8)
        w[(s + 7) & 7] = pq[(s + 7) + ((s + 7) >> 3)];
        const double tv = tq[s];
#pragma unroll
        for (int j = 0; j < SDR_J; ++j) acc[j] = fma(tv, w[(s + j) & 7], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < SDR_J; ++j) tot[j] += acc[j];
  }
  __syncthreads();  // every wave is done with the p window: it now holds the waves' partials
  double* wsum = pl;
#pragma unroll
  for (int j = 0; j < SDR_J; ++j) wsum[wave * SDR_FMAX + SDR_J * lane + j] = tot[j];
  if (lane == 0) {
    sq[wave] = ss;
    tp[wave] = st;
  }
  __syncthreads();
  double* __restrict__ dst = part + ((size_t)row * chunks + chunk) * (size_t)(F + 2);
  for (int l = tid; l < F; l += SDR_THREADS)
    dst[l] = ((wsum[l] + wsum[SDR_FMAX + l]) + wsum[2 * SDR_FMAX + l]) + wsum[3 * SDR_FMAX + l];
  if (tid == 0) dst[F] = ((sq[0] + sq[1]) + sq[2]) + sq[3];
  if (tid == 1) dst[F + 1] = ((tp[0] + tp[1]) + tp[2]) + tp[3];
}

// chunk partials v[c * stride], c < nch, in groups of SDR_GROUP: each group in order, then the
// groups in order
__device__ __forceinline__ double sum_chunks(const double* __restrict__ v, long long nch,
                                             size_t stride) {
  double tot = 0.0;
  for (long long c0 = 0; c0 < nch; c0 += SDR_GROUP) {
    double s = 0.0;
    const long long c1 = c0 + SDR_GROUP < nch ? c0 + SDR_GROUP : nch;
    for (long long c = c0; c < c1; ++c) s += v[(size_t)c * stride];
    tot += s;
  }
  return tot;
}

// max(sqrt(x), 1e-6) that keeps NaN
__device__ __forceinline__ double clamped_norm(double x) {
  const double s = sqrt(x);
  return s < 1e-6 ? 1e-6 : s;
}

// vec[row][F]: b of the estimates' rows, then r of the references' rows, divided by the clamped
// norms. A row with n = 0, sum t^2 = 0, sum p^2 = 0 or a NaN in either sum gets b = NaN.
// Lag 0 is taken from the sum of t p that was formed in the order of the two energies, not from
// the lag loop: for a row against itself the three are then the same bits, r[0] is exactly 1,
// and est == ref gives b = r, s = (1, 0, ...) and coh = 1 exactly.
__global__ __launch_bounds__(SDR_THREADS) void sdr_reduce_kernel(
    const double* __restrict__ part, long long chunks, int rows, int ref_rows, long long samples,
    const long long* __restrict__ lengths, int F, double load_diag, double* __restrict__ vec) {
  const int row = blockIdx.x;
  const bool is_ref = row >= rows;
  const int rrow = is_ref ? row - rows : row % ref_rows;
  const long long n = row_length(lengths, rrow, samples);
  const long long nch = (n + SDR_CHUNK - 1) / SDR_CHUNK;
  const size_t stride = (size_t)(F + 2);
  const double* __restrict__ mine = part + (size_t)row * chunks * stride;
  const double* __restrict__ refp = part + (size_t)(rows + rrow) * chunks * stride;
  const double tt = sum_chunks(refp + F, nch, stride);
  const double pp = is_ref ? tt : sum_chunks(mine + F, nch, stride);
  // both norms above the clamp: sqrt(tt pp), which is tt itself for a reference against itself
  // (r[0] = 1 exactly, and est == ref gives coh = 1 exactly)
  const double scale = (tt >= 1e-12 && pp >= 1e-12) ? sqrt(tt * pp)
                                                    : clamped_norm(tt) * clamped_norm(pp);
  const bool special = !is_ref && (!(tt > 0.0) || !(pp > 0.0));
  for (int l = threadIdx.x; l < F; l += SDR_THREADS) {
    double v = sum_chunks(mine + (l == 0 ? F + 1 : l), nch, stride) / scale;
    if (is_ref && l == 0 && load_diag == load_diag) v += load_diag;
    if (special) v = __builtin_nan("");
    vec[(size_t)row * F + l] = v;
  }
}

// Levinson-Durbin on r, one wave: lane x holds elements x + 64 i (i < 8) of the prediction
// polynomial a and of each estimate's solution s, so a step of order m touches the blocks
// i <= m / 64 only. Per step: the dot products a . r and s . r against the reversed r (LDS, the
// lanes' reads consecutive), their wave sums, the reflection coefficient and the error once, the
// polynomial's update against its own reverse (LDS, two buffers: one barrier per step, which a
// one-wave workgroup does not wait at), and one AXPY per estimate. F - 1 steps whatever the data.
__global__ __launch_bounds__(64) void sdr_solve_kernel(const double* __restrict__ vec, int rows,
                                                       int ref_rows, int F,
                                                       double* __restrict__ out) {
  __shared__ double rl[SDR_FMAX];
  __shared__ double al[2][SDR_FMAX];
  __shared__ double bl[SDR_LT][SDR_FMAX];
  const int rrow = blockIdx.x, lane = threadIdx.x;
  const int levels = rows / ref_rows;
  int erow[SDR_LT];
  bool valid[SDR_LT];
#pragma unroll
  for (int e = 0; e < SDR_LT; ++e) {
    const int lev = (int)blockIdx.y * SDR_LT + e;
    valid[e] = lev < levels;
    erow[e] = valid[e] ? lev * ref_rows + rrow : rrow;
  }
  double a[8], x[SDR_LT][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = lane + 64 * i;
    rl[j] = j < F ? vec[(size_t)(rows + rrow) * F + j] : 0.0;
    al[0][j] = j == 0 ? 1.0 : 0.0;
    al[1][j] = 0.0;
    a[i] = j == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int e = 0; e < SDR_LT; ++e) {
      bl[e][j] = (valid[e] && j < F) ? vec[(size_t)erow[e] * F + j] : 0.0;
      x[e][i] = 0.0;
    }
  }
  __syncthreads();
  double E = rl[0];
  bool singular = !(E > 0.0 && E < __builtin_inf());
#pragma unroll
  for (int e = 0; e < SDR_LT; ++e)
    if (lane == 0) x[e][0] = bl[e][0] / E;

  for (int m = 1; m < F; ++m) {
    const double* __restrict__ old = al[(m - 1) & 1];
    double* __restrict__ nw = al[m & 1];
    double pa = 0.0, pe[SDR_LT];
#pragma unroll
    for (int e = 0; e < SDR_LT; ++e) pe[e] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (64 * i < m) {  // uniform: the block holds an element below m
        const int idx = m - (lane + 64 * i);
        const double rv = idx > 0 ? rl[idx] : 0.0;
        pa = fma(a[i], rv, pa);
#pragma unroll
        for (int e = 0; e < SDR_LT; ++e) pe[e] = fma(x[e][i], rv, pe[e]);
      }
    }
    const double k = -wave_sum(pa) / E;
    E = E * (1.0 - k * k);
    singular = singular || !(E > 0.0 && E < __builtin_inf());
    double q[SDR_LT];
#pragma unroll
    for (int e = 0; e < SDR_LT; ++e) q[e] = (bl[e][m] - wave_sum(pe[e])) / E;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (64 * i <= m) {
        const int j = lane + 64 * i, idx = m - j;
        const double ar = idx >= 0 ? old[idx] : 0.0;
        a[i] = fma(k, ar, a[i]);
        nw[j] = a[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (64 * i <= m) {
        const int idx = m - (lane + 64 * i);
        const double an = idx >= 0 ? nw[idx] : 0.0;
#pragma unroll
        for (int e = 0; e < SDR_LT; ++e) x[e][i] = fma(q[e], an, x[e][i]);
      }
    }
  }

#pragma unroll
  for (int e = 0; e < SDR_LT; ++e) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = fma(bl[e][lane + 64 * i], x[e][i], c);
    const double coh = wave_sum(c);
    if (lane == 0 && valid[e])
      out[erow[e]] = singular ? __builtin_nan("") : 10.0 * log10(coh / (1.0 - coh));
  }
}

long long chunks_of(long long samples) { return (samples + SDR_CHUNK - 1) / SDR_CHUNK; }

bool shape_ok(int rows, int ref_rows, long long samples, int filter_length) {
  // grid.y carries the rows (rows <= 65535 as for vrvq_signal_metrics)
  return rows > 0 && rows <= 65535 && ref_rows > 0 && rows % ref_rows == 0 && samples > 0 &&
         samples <= SDR_MAX_SAMPLES && filter_length >= 1 && filter_length <= SDR_FMAX;
}

long long workspace_doubles(int rows, int ref_rows, long long samples, int F) {
  const long long all = (long long)rows + ref_rows;
  return all * (1 + chunks_of(samples) * (F + 2) + F);
}

}  // namespace

extern "C" int vrvq_bss_sdr_workspace(int rows, int ref_rows, long long samples,
                                      int filter_length, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && shape_ok(rows, ref_rows, samples, filter_length));
  *bytes = workspace_doubles(rows, ref_rows, samples, filter_length) * (long long)sizeof(double);
  return VRVQ_OK;
}

extern "C" int vrvq_bss_sdr(const float* est, const float* ref, int rows, int ref_rows,
                            long long samples, const long long* lengths, int filter_length,
                            int zero_mean, double load_diag, double* out, void* workspace,
                            long long workspace_bytes, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(est && ref && out && workspace);
  VRVQ_CHECK_ARG(shape_ok(rows, ref_rows, samples, filter_length));
  const int F = filter_length;
  const long long chunks = chunks_of(samples), all = (long long)rows + ref_rows;
  VRVQ_CHECK_ARG(workspace_bytes >=
                 workspace_doubles(rows, ref_rows, samples, F) * (long long)sizeof(double));
  VRVQ_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  double* means = static_cast<double*>(workspace);  // [all]
  double* part = means + all;                        // [all][chunks][F + 2]
  double* vec = part + all * chunks * (F + 2);       // [all][F]
  int rc;
  if (zero_mean) {
    hipLaunchKernelGGL(sdr_mean_kernel, dim3((unsigned)all), dim3(SDR_THREADS), 0,
                       as_stream(stream), est, ref, rows, ref_rows, samples, lengths, means);
    if ((rc = vrvq_launch_status())) return rc;
  }
  hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)chunks, (unsigned)rows, 2),
                     dim3(SDR_THREADS), 0, as_stream(stream), est, ref, rows, ref_rows, samples,
                     lengths, F, zero_mean ? means : (const double*)nullptr, part);
  if ((rc = vrvq_launch_status())) return rc;
  hipLaunchKernelGGL(sdr_reduce_kernel, dim3((unsigned)all), dim3(SDR_THREADS), 0,
                     as_stream(stream), part, chunks, rows, ref_rows, samples, lengths, F,
                     load_diag, vec);
  if ((rc = vrvq_launch_status())) return rc;
  const int levels = rows / ref_rows;
  hipLaunchKernelGGL(sdr_solve_kernel,
                     dim3((unsigned)ref_rows, (unsigned)((levels + SDR_LT - 1) / SDR_LT)), dim3(64),
                     0, as_stream(stream), vec, rows, ref_rows, F, out);
  return vrvq_launch_status();
}
