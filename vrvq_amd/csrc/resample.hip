// Sample-rate conversion (include/vrvq.h "Sample-rate conversion"): the polyphase windowed-sinc
// FIR of julius.resample_frac as audiotools.AudioSignal.resample calls it, forward and adjoint.
//
// julius runs it as a dense strided conv1d over `new` output channels with K = 2 W + old taps
// each; about three quarters of those taps carry the window's zero for the common ratios. Here the
// host builds the kept taps only ([new][ntaps] + first[new], fp64 rounded once to fp32) and
//
//   forward   one 256-thread workgroup owns RS_TILE consecutive outputs of one row. The input
//             window those outputs read, x[f0 old - W .. f1 old + K - 1 - W] for the tile's first
//             and last frame, is staged in LDS RS_SEG samples at a time with the replicate clamp
//             applied at staging (one segment for every ratio between the usual audio rates; an
//             extreme down-ratio walks several). Each lane owns RS_TILE / 256 outputs and adds
//             their taps in ascending j as one fp32 fma chain, whatever the segmentation: the
//             bits of an output are a function of (ratio, n, the row's samples) alone.
//             The tap rows are read through L1 / L2 (441:80 needs 90 KB for the table, which does
//             not fit beside the window), four taps per 16-byte load at 4-byte alignment.
//             LDS index p lives at p + p / 32: a down-ratio makes neighbouring lanes read `old`
//             samples apart, and a stride of 2 or 4 words would otherwise put 2 or 4 lanes of a
//             32-lane group on one bank.
//   adjoint   gather form, one thread per input sample m: for every frame f whose K-window covers
//             m the tap index j = m + W - f old is fixed, and the phases whose row holds j are a
//             contiguous range because first[] is non-decreasing (two binary searches). Frames,
//             then phases, ascending: one fma chain, no atomics. The gradient of the replicated
//             edges (the taps whose index fell below 0 or past L - 1) is summed by one workgroup per
//             row in a fixed order (threads stride over (frame, phase) pairs, then an LDS tree) and
//             added to dx[0] and dx[L - 1] by one thread after the gather has written them.
//
// 64-bit sample indices throughout (an hour of 48 kHz audio is 1.7e8 samples per channel).
#include <math.h>
#include <stdio.h>

#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = VRVQ_RESAMPLE_TILE;
constexpr int RS_PER = RS_TILE / RS_THREADS;  // outputs per lane
constexpr int RS_SEG = 8192;                  // window samples staged at once (32 KiB + skew)
constexpr int RS_MAX_RATE = 1024;
constexpr int RS_MAX_ZEROS = 1024;
constexpr long long RS_MAX_LENGTH = 1LL << 40;
static_assert(RS_TILE % RS_THREADS == 0, "whole outputs per lane");

typedef float rs_f4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int rs_skew(int p) { return p + (p >> 5); }

__device__ __forceinline__ int rs_first(const int* __restrict__ first, int i, int K, int ntaps) {
  // the table's own invariant (0 <= first[i] <= K - ntaps), enforced: every LDS index below
  // stays inside the staged window whatever the caller's buffer holds
  const int f = first[i];
  return f < 0 ? 0 : (f > K - ntaps ? K - ntaps : f);
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const float* __restrict__ x, long long L, int old, int nw, int W, int K, int ntaps,
    const float* __restrict__ taps, const int* __restrict__ first, float* __restrict__ y,
    long long out_len) {
  __shared__ float win[RS_SEG + RS_SEG / 32 + 1];
  const int tid = threadIdx.x;
  const int row = blockIdx.y;
  const long long n0 = (long long)blockIdx.x * RS_TILE;
  const long long nend = n0 + RS_TILE < out_len ? n0 + RS_TILE : out_len;
  const long long f0 = n0 / nw, f1 = (nend - 1) / nw;
  const long long gbase = f0 * old - W;                // input index of window position 0
  const int wlen = (int)(f1 - f0) * old + K;           // <= (RS_TILE / new + 1) old + K
  const float* __restrict__ xr = x + (size_t)row * L;

  float acc[RS_PER];
  int q0[RS_PER];  // window position of the lane's first tap; -1: no output
  const float* tp[RS_PER];
#pragma unroll
  for (int r = 0; r < RS_PER; ++r) {
    const long long n = n0 + tid + r * RS_THREADS;
    acc[r] = 0.0f;
    q0[r] = -1;
    tp[r] = taps;
    if (n < nend) {
      const long long f = n / nw;
      const int i = (int)(n - f * nw);
      q0[r] = (int)(f - f0) * old + rs_first(first, i, K, ntaps);
      tp[r] = taps + (size_t)i * ntaps;
    }
  }

  for (int s0 = 0; s0 < wlen; s0 += RS_SEG) {  // uniform over the workgroup
    const int slen = wlen - s0 < RS_SEG ? wlen - s0 : RS_SEG;
    if (s0) __syncthreads();
    for (int p = tid; p < slen; p += RS_THREADS) {
      long long g = gbase + s0 + p;
      g = g < 0 ? 0 : (g > L - 1 ? L - 1 : g);
      win[rs_skew(p)] = xr[g];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
      if (q0[r] < 0) continue;
      // the lane's taps inside this segment, ascending: one chain across the segments
      const int jlo = s0 - q0[r] > 0 ? s0 - q0[r] : 0;
      const int jhi = s0 + slen - q0[r] < ntaps ? s0 + slen - q0[r] : ntaps;
      const float* __restrict__ t = tp[r];
      const int pb = q0[r] - s0;
      float a = acc[r];
      int jj = jlo;
      for (; jj + 4 <= jhi; jj += 4) {
        const rs_f4 k = *reinterpret_cast<const rs_f4*>(t + jj);
        a = fmaf(k.x, win[rs_skew(pb + jj)], a);
        a = fmaf(k.y, win[rs_skew(pb + jj + 1)], a);
        a = fmaf(k.z, win[rs_skew(pb + jj + 2)], a);
        a = fmaf(k.w, win[rs_skew(pb + jj + 3)], a);
      }
      for (; jj < jhi; ++jj) a = fmaf(t[jj], win[rs_skew(pb + jj)], a);
      acc[r] = a;
    }
  }
  float* __restrict__ yr = y + (size_t)row * out_len;
#pragma unroll
  for (int r = 0; r < RS_PER; ++r) {
    const long long n = n0 + tid + r * RS_THREADS;
    if (n < nend) yr[n] = acc[r];
  }
}

// floor(a / b) for b > 0
__device__ __forceinline__ long long rs_floor_div(long long a, long long b) {
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// first index i in [0, n) with first[i] > v (n if none); first is non-decreasing
__device__ __forceinline__ int rs_upper(const int* __restrict__ first, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] > v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(RS_THREADS) void resample_adjoint_kernel(
    const float* __restrict__ dy, long long out_len, int old, int nw, int W, int K, int ntaps,
    const float* __restrict__ taps, const int* __restrict__ first, float* __restrict__ dx,
    long long L) {
  const long long m = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (m >= L) return;
  const int row = blockIdx.y;
  const float* __restrict__ dyr = dy + (size_t)row * out_len;
  const long long fmax = (out_len - 1) / nw;
  // frames with 0 <= m + W - f old <= K - 1
  long long flo = -rs_floor_div(-(m + W - K + 1), old);  // ceil
  if (flo < 0) flo = 0;
  long long fhi = (m + W) / old;
  if (fhi > fmax) fhi = fmax;
  float acc = 0.0f;
  for (long long f = flo; f <= fhi; ++f) {
    const int j = (int)(m + W - f * old);
    // phases with first[i] <= j < first[i] + ntaps
    int ilo = rs_upper(first, nw, j - ntaps);
    int ihi = rs_upper(first, nw, j) - 1;
    const long long left = out_len - 1 - f * nw;  // outputs of this frame that exist
    if (ihi > left) ihi = (int)left;
    const float* __restrict__ d = dyr + f * nw;
    for (int i = ilo; i <= ihi; ++i) {
      const int jj = j - first[i];
      if ((unsigned)jj < (unsigned)ntaps) acc = fmaf(taps[(size_t)i * ntaps + jj], d[i], acc);
    }
  }
  dx[(size_t)row * L + m] = acc;
}

// Gradient of the replicated edges: every product k_i[j] dy[n] whose input index f old + j - W is
// below 0 goes to dx[0], above L - 1 to dx[L - 1]. One workgroup per row.
__global__ __launch_bounds__(RS_THREADS) void resample_adjoint_edge_kernel(
    const float* __restrict__ dy, long long out_len, int old, int nw, int W, int K, int ntaps,
    const float* __restrict__ taps, const int* __restrict__ first, float* __restrict__ dx,
    long long L) {
  __shared__ float red[2][RS_THREADS];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const float* __restrict__ dyr = dy + (size_t)row * out_len;
  const long long fmax = (out_len - 1) / nw;
  float left = 0.0f, right = 0.0f;
  // left: frames whose first tap index f old - W is negative
  {
    long long fl = (W - 1) / old;
    if (fl > fmax) fl = fmax;
    const long long pairs = (fl + 1) * nw;
    for (long long p = tid; p < pairs; p += RS_THREADS) {
      const long long f = p / nw;
      const int i = (int)(p - f * nw);
      if (f * nw + i >= out_len) continue;
      const float d = dyr[f * nw + i];
      const long long base = f * old + rs_first(first, i, K, ntaps) - W;
      const float* __restrict__ t = taps + (size_t)i * ntaps;
      for (int jj = 0; jj < ntaps && base + jj < 0; ++jj) left = fmaf(t[jj], d, left);
    }
  }
  // right: frames whose last tap index f old + K - 1 - W is past L - 1
  {
    long long fr = -rs_floor_div(-(L + W - K + 1), old);  // ceil
    if (fr < 0) fr = 0;
    const long long pairs = fr <= fmax ? (fmax - fr + 1) * nw : 0;
    for (long long p = tid; p < pairs; p += RS_THREADS) {
      const long long f = fr + p / nw;
      const int i = (int)(p % nw);
      if (f * nw + i >= out_len) continue;
      const float d = dyr[f * nw + i];
      const long long base = f * old + rs_first(first, i, K, ntaps) - W;
      const float* __restrict__ t = taps + (size_t)i * ntaps;
      long long js = L - base;  // first jj with base + jj > L - 1
      if (js < 0) js = 0;
      for (int jj = (int)(js < ntaps ? js : ntaps); jj < ntaps; ++jj) right = fmaf(t[jj], d, right);
    }
  }
  red[0][tid] = left;
  red[1][tid] = right;
  __syncthreads();
  for (int s = RS_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {  // in this order: with L == 1 both edges are the one sample
    float* __restrict__ dxr = dx + (size_t)row * L;
    dxr[0] += red[0][0];
    dxr[L - 1] += red[1][0];
  }
}

// ------------------------------------------------------------------------------- host side
thread_local char rs_error[192] = "";

struct Plan {
  int old, nw, W, K, ntaps;
  double sr;
};

int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// u of the specification: the tap's position in units of the zero crossings
double rs_u(const Plan& p, int i, int j) {
  return (-(double)i / (double)p.nw + (double)(j - p.W) / (double)p.old) * p.sr;
}

// kept taps of phase i: j in [*lo, *hi) (u is increasing in j)
void rs_kept(const Plan& p, int zeros, int i, int* lo, int* hi) {
  int a = 0, b = p.K;
  while (a < p.K && !(fabs(rs_u(p, i, a)) < (double)zeros)) ++a;
  while (b > a && !(fabs(rs_u(p, i, b - 1)) < (double)zeros)) --b;
  *lo = a;
  *hi = b;
}

int rs_plan(int old_sr, int new_sr, int zeros, double rolloff, Plan* p) {
  rs_error[0] = 0;
  if (old_sr <= 0 || new_sr <= 0) {
    snprintf(rs_error, sizeof rs_error, "resample: sample rates must be positive (%d -> %d)",
             old_sr, new_sr);
    return VRVQ_ERR_ARG;
  }
  if (zeros <= 0 || zeros > RS_MAX_ZEROS || !(rolloff > 0.0 && rolloff <= 1.0)) {
    snprintf(rs_error, sizeof rs_error,
             "resample: zeros must be in [1, %d] and rolloff in (0, 1] (got %d, %g)",
             RS_MAX_ZEROS, zeros, rolloff);
    return VRVQ_ERR_ARG;
  }
  const int g = rs_gcd(old_sr, new_sr);
  p->old = old_sr / g;
  p->nw = new_sr / g;
  if (p->old > RS_MAX_RATE || p->nw > RS_MAX_RATE) {
    snprintf(rs_error, sizeof rs_error,
             "resample: %d -> %d Hz reduces to the ratio %d:%d, beyond the supported %d:%d",
             old_sr, new_sr, p->old, p->nw, RS_MAX_RATE, RS_MAX_RATE);
    return VRVQ_ERR_ARG;
  }
  p->sr = (double)(p->old < p->nw ? p->old : p->nw) * rolloff;
  const double w = ceil((double)zeros * (double)p->old / p->sr);
  if (!(w <= 2.0 * RS_MAX_ZEROS * RS_MAX_RATE)) {
    snprintf(rs_error, sizeof rs_error,
             "resample: ratio %d:%d with zeros %d and rolloff %g needs a half-width of %g taps, "
             "beyond the supported %d", p->old, p->nw, zeros, rolloff, w,
             2 * RS_MAX_ZEROS * RS_MAX_RATE);
    return VRVQ_ERR_ARG;
  }
  p->W = (int)w;
  p->K = 2 * p->W + p->old;
  int nt = 1;
  for (int i = 0; i < p->nw; ++i) {
    int lo, hi;
    rs_kept(*p, zeros, i, &lo, &hi);
    if (hi - lo > nt) nt = hi - lo;
  }
  p->ntaps = nt;
  return VRVQ_OK;
}

// what the launchers accept: a plan's numbers (their consistency, not their origin)
bool rs_shape_ok(int rows, long long length, int old, int nw, int W, int ntaps,
                 long long out_length) {
  if (rows <= 0 || rows > 65535 || length <= 0 || length > RS_MAX_LENGTH) return false;
  if (old <= 0 || old > RS_MAX_RATE || nw <= 0 || nw > RS_MAX_RATE) return false;
  if (W <= 0 || W > 2 * RS_MAX_ZEROS * RS_MAX_RATE || ntaps <= 0 || ntaps > 2 * W + old)
    return false;
  const long long out_max = ((long long)nw * length + old - 1) / old;
  return out_length > 0 && out_length <= out_max;
}

}  // namespace

extern "C" const char* vrvq_resample_error(void) { return rs_error; }

extern "C" int vrvq_resample_plan(int old_sr, int new_sr, int zeros, double rolloff,
                                  long long length, long long out[8]) {
  Plan p;
  const int rc = rs_plan(old_sr, new_sr, zeros, rolloff, &p);
  if (rc) return rc;
  if (!out || length < 0 || length > RS_MAX_LENGTH) {
    snprintf(rs_error, sizeof rs_error, "resample: null output or a length outside [0, 2^40]");
    return VRVQ_ERR_ARG;
  }
  out[0] = p.old;
  out[1] = p.nw;
  out[2] = p.W;
  out[3] = p.K;
  out[4] = p.ntaps;
  out[5] = (long long)p.nw * length / p.old;
  out[6] = ((long long)p.nw * length + p.old - 1) / p.old;
  out[7] = (long long)p.nw * p.ntaps;
  return VRVQ_OK;
}

extern "C" int vrvq_resample_taps(int old_sr, int new_sr, int zeros, double rolloff, float* taps,
                                  long long taps_len, int* first, long long first_len) {
  Plan p;
  const int rc = rs_plan(old_sr, new_sr, zeros, rolloff, &p);
  if (rc) return rc;
  if (!taps || !first || taps_len < (long long)p.nw * p.ntaps || first_len < p.nw) {
    snprintf(rs_error, sizeof rs_error, "resample: tap buffers are null or too small");
    return VRVQ_ERR_ARG;
  }
  const double pi = 3.14159265358979323846;
  double* k = new double[p.K];
  for (int i = 0; i < p.nw; ++i) {
    double sum = 0.0;
    for (int j = 0; j < p.K; ++j) {
      double u = rs_u(p, i, j);
      u = u < -(double)zeros ? -(double)zeros : (u > (double)zeros ? (double)zeros : u);
      const double t = u * pi;
      const double c = cos(t / (double)zeros / 2.0);
      k[j] = (t == 0.0 ? 1.0 : sin(t) / t) * (c * c);
      sum += k[j];
    }
    int lo, hi;
    rs_kept(p, zeros, i, &lo, &hi);
    // the row's window [fi, fi + ntaps) holds the kept taps and ends inside K
    const int fi = lo < p.K - p.ntaps ? lo : p.K - p.ntaps;
    first[i] = fi;
    for (int jj = 0; jj < p.ntaps; ++jj) {
      const int j = fi + jj;
      taps[(size_t)i * p.ntaps + jj] = (j >= lo && j < hi) ? (float)(k[j] / sum) : 0.0f;
    }
  }
  delete[] k;
  return VRVQ_OK;
}

extern "C" int vrvq_resample(const float* x, int rows, long long length, int old_rate,
                             int new_rate, int width, int ntaps, const float* taps,
                             const int* first, float* y, long long out_length,
                             vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(x && y && taps && first);
  VRVQ_CHECK_ARG(rs_shape_ok(rows, length, old_rate, new_rate, width, ntaps, out_length));
  const long long tiles = (out_length + RS_TILE - 1) / RS_TILE;
  VRVQ_CHECK_ARG(tiles <= (1LL << 23));  // grid.x * 256 threads stays below 2^32
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(RS_THREADS), 0,
                     as_stream(stream), x, length, old_rate, new_rate, width,
                     2 * width + old_rate, ntaps, taps, first, y, out_length);
  return vrvq_launch_status();
}

extern "C" int vrvq_resample_adjoint(const float* dy, int rows, long long out_length,
                                     int old_rate, int new_rate, int width, int ntaps,
                                     const float* taps, const int* first, float* dx,
                                     long long length, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(dy && dx && taps && first);
  VRVQ_CHECK_ARG(rs_shape_ok(rows, length, old_rate, new_rate, width, ntaps, out_length));
  const long long blocks = (length + RS_THREADS - 1) / RS_THREADS;
  VRVQ_CHECK_ARG(blocks <= (1LL << 23));
  const int K = 2 * width + old_rate;
  hipLaunchKernelGGL(resample_adjoint_kernel, dim3((unsigned)blocks, (unsigned)rows),
                     dim3(RS_THREADS), 0, as_stream(stream), dy, out_length, old_rate, new_rate,
                     width, K, ntaps, taps, first, dx, length);
  int rc = vrvq_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(resample_adjoint_edge_kernel, dim3((unsigned)rows), dim3(RS_THREADS), 0,
                     as_stream(stream), dy, out_length, old_rate, new_rate, width, K, ntaps, taps,
                     first, dx, length);
  return vrvq_launch_status();
}
