// Integrated loudness (include/vrvq.h "Integrated loudness"): ITU-R BS.1770-4 as audiotools'
// Meter.integrated_loudness computes it, in the arithmetic of vrvq_amd.codec.loudness.
//
// The K-weighting is a fourth-order IIR (two biquads in cascade) and is run exactly, as a chunked
// scan over each (item, channel) row:
//
//   pass 1   one lane owns LD_C consecutive samples. It runs the cascade from zero state in fp64
//            (transposed direct form II, the form of scipy's lfilter) and stores its four final
//            state values.
//   carry    one wave per row turns the finals into every chunk's entry state. Over a chunk of
//            zero input the state (s, t) of the two stages moves by s' = M1 s, t' = M2 t + K s (the
//            blocks of the 4 x 4 power, built on the host in long double and rounded once), so
//            entry[k + 1] = M entry[k] + final[k]. Lane l owns the G = ceil(chunks / 64)
//            consecutive chunks [l G, (l + 1) G): it scans them from zero and, beside that, moves
//            the four unit states through G chunks (the columns of M^G); lane 0 chains the 64
//            groups; every lane then rescans its chunks from its group's entry state, in place.
//   pass 2   every lane reruns its chunk from its entry state and adds y^2 in fp64, in sample
//            order. The sum is cut wherever a block begins or ends and at the chunk's end: with
//            win = q step + rem the cuts are the multiples of step and, where rem > 0, those plus
//            rem ("segments": one or two per step, nothing assumes win = 4 step). The piece that
//            starts at sample p of chunk k and segment s is stored at index k + s of the row.
//   finish   one workgroup per item: a thread per (channel, segment) adds the segment's pieces in
//            sample order; a thread per block adds its segments in order, divides by win and
//            evaluates the block loudness; the gated means are sums over the blocks j = thread,
//            thread + 256, ... in sequence, then an LDS tree over the 256 threads.
//
// The filtered signal is never stored. No atomics. Which lane adds which sample in which order is
// a function of (sample_rate, length) alone: LD_C is a constant, so a row's bits do not depend on
// the batch. Samples at or past `length` read as zeros (the short-input rule), nothing is padded
// in memory.
//
// Global loads: a lane that walked its own chunk would read at a stride of LD_C floats. The
// workgroup instead stages LD_SUB samples of each of its 256 chunks at a time, 32 consecutive
// threads reading one chunk's 128 contiguous bytes, into LDS rows of LD_SUB + 1 dwords: lane l
// then reads dword 33 l + o, bank (l + o) % 32, which differs for the 32 lanes of a half-wave.
//
// 64-bit sample indices throughout.
#include <math.h>
#include <stdio.h>

#include "common.h"

namespace {

constexpr int LD_C = VRVQ_LOUDNESS_CHUNK;  // samples per lane
constexpr int LD_THREADS = 256;            // lanes (chunks) per workgroup
constexpr int LD_SUB = 32;                 // samples of every chunk staged at once
constexpr int LD_ROW = LD_SUB + 1;         // LDS row stride in dwords (odd: see the file header)
constexpr int LD_MAX_CH = 5;
constexpr long long LD_MAX_LENGTH = 1LL << 40;
static_assert(LD_C % LD_SUB == 0 && LD_SUB == 32, "whole sub-tiles; a staging row is 32 threads");

struct Coef {  // [0] high shelf, [1] high pass; a0 = 1
  double b0[2], b1[2], b2[2], a1[2], a2[2];
};

struct Trans {  // chunk transition, row-major 2 x 2 each: s' = M1 s, t' = M2 t + K s
  double M1[4], M2[4], K[4];
};

struct State {
  double s0, s1, t0, t1;
};

struct Geom {
  long long length, eff, chunks, pieces, segs, blocks;
  int win, step, q, rem, channels;
};

// One sample through the cascade; returns the K-weighted sample.
__device__ __forceinline__ double ld_step(const Coef& c, State& v, double x) {
  const double y1 = fma(c.b0[0], x, v.s0);
  v.s0 = fma(-c.a1[0], y1, fma(c.b1[0], x, v.s1));
  v.s1 = fma(-c.a2[0], y1, c.b2[0] * x);
  const double y2 = fma(c.b0[1], y1, v.t0);
  v.t0 = fma(-c.a1[1], y2, fma(c.b1[1], y1, v.t1));
  v.t1 = fma(-c.a2[1], y2, c.b2[1] * y1);
  return y2;
}

// index of the segment that holds sample p
__device__ __forceinline__ long long ld_seg(long long p, int step, int rem) {
  const long long m = p / step;
  if (!rem) return m;
  return 2 * m + ((p - m * step) >= rem ? 1 : 0);
}

// the first segment edge after sample p
__device__ __forceinline__ long long ld_next(long long p, int step, int rem) {
  const long long m = p / step;
  return (rem && (p - m * step) < rem) ? m * step + rem : (m + 1) * step;
}

// state [row][chunk][4]: pass 1 writes the finals, pass 2 reads the entry states the carry left
// there. part [row][pieces] (pass 2).
template <bool SECOND>
__global__ __launch_bounds__(LD_THREADS) void loudness_pass_kernel(
    const float* __restrict__ x, Geom g, Coef cf, double* __restrict__ state,
    double* __restrict__ part) {
  __shared__ float tile[LD_THREADS * LD_ROW];
  const int tid = threadIdx.x;
  const int row = blockIdx.y;
  const long long k0 = (long long)blockIdx.x * LD_THREADS;  // the workgroup's first chunk
  const long long k = k0 + tid;
  const bool live = k < g.chunks;
  const float* __restrict__ xr = x + (size_t)row * g.length;
  double* __restrict__ st = state + ((size_t)row * g.chunks + (live ? k : 0)) * 4;
  double* __restrict__ pr = part + (size_t)row * g.pieces;

  State v = {0.0, 0.0, 0.0, 0.0};
  const long long p0 = k * LD_C;
  const long long pend = p0 + LD_C < g.eff ? p0 + LD_C : g.eff;  // <= p0 for a lane past the row
  long long idx = 0, nb = 0;
  double acc = 0.0;
  bool open = false;  // acc holds samples not yet stored
  if (SECOND && live) {
    v.s0 = st[0];
    v.s1 = st[1];
    v.t0 = st[2];
    v.t1 = st[3];
    idx = k + ld_seg(p0, g.step, g.rem);
    nb = ld_next(p0, g.step, g.rem);
  }

  for (int t = 0; t < LD_C / LD_SUB; ++t) {
    if (t) __syncthreads();
#pragma unroll 8
    for (int i = tid; i < LD_THREADS * LD_SUB; i += LD_THREADS) {
      const int l = i >> 5, o = i & 31;
      const long long gi = (k0 + l) * LD_C + t * LD_SUB + o;
      tile[l * LD_ROW + o] = gi < g.length ? xr[gi] : 0.0f;
    }
    __syncthreads();
    if (!live) continue;  // no barrier depends on it: every lane reaches the two above
    const float* __restrict__ mine = tile + tid * LD_ROW;
    if (!SECOND) {
#pragma unroll
      for (int o = 0; o < LD_SUB; ++o) ld_step(cf, v, (double)mine[o]);
    } else {
      const long long pb = p0 + t * LD_SUB;
      const int n = (int)(pend - pb < 0 ? 0 : (pend - pb > LD_SUB ? LD_SUB : pend - pb));
      for (int o = 0; o < n; ++o) {
        const double y = ld_step(cf, v, (double)mine[o]);
        acc = fma(y, y, acc);
        open = true;
        if (pb + o + 1 == nb) {
          if (idx < g.pieces) pr[idx] = acc;
          acc = 0.0;
          open = false;
          ++idx;
          nb = ld_next(nb, g.step, g.rem);
        }
      }
    }
  }
  if (!live) return;
  if (!SECOND) {
    st[0] = v.s0;
    st[1] = v.s1;
    st[2] = v.t0;
    st[3] = v.t1;
  } else if (open && idx < g.pieces) {
    pr[idx] = acc;
  }
}

// M v + f, in this order
__device__ __forceinline__ State ld_apply(const Trans& m, const State& v, const State& f) {
  State r;
  r.s0 = fma(m.M1[0], v.s0, fma(m.M1[1], v.s1, f.s0));
  r.s1 = fma(m.M1[2], v.s0, fma(m.M1[3], v.s1, f.s1));
  r.t0 = fma(m.M2[0], v.t0, fma(m.M2[1], v.t1, fma(m.K[0], v.s0, fma(m.K[1], v.s1, f.t0))));
  r.t1 = fma(m.M2[2], v.t0, fma(m.M2[3], v.t1, fma(m.K[2], v.s0, fma(m.K[3], v.s1, f.t1))));
  return r;
}

// One wave per row (file header, "carry"). In place: state[k] is final[k] on entry and
// entry[k] on return.
__global__ __launch_bounds__(64) void loudness_carry_kernel(double* __restrict__ state,
                                                            long long chunks, Trans m) {
  __shared__ State fin[64];
  __shared__ State ent[64];
  const int lane = threadIdx.x;
  double* __restrict__ st = state + (size_t)blockIdx.x * chunks * 4;
  const long long G = (chunks + 63) / 64;
  const long long lo = lane * G < chunks ? lane * G : chunks;
  const long long hi = lo + G < chunks ? lo + G : chunks;
  const State zero = {0.0, 0.0, 0.0, 0.0};

  // the lane's chunks from zero state, and the unit states through G chunks (uniform trip count)
  State cur = zero;
  State col[4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0},
                  {0.0, 0.0, 0.0, 1.0}};
  for (long long i = 0; i < G; ++i) {
    if (lo + i < hi) {
      const double* __restrict__ f = st + (lo + i) * 4;
      const State fv = {f[0], f[1], f[2], f[3]};
      cur = ld_apply(m, cur, fv);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) col[c] = ld_apply(m, col[c], zero);
  }
  fin[lane] = cur;
  __syncthreads();
  if (lane == 0) {  // groups in order: entry of group l + 1 = M^G entry of group l + its final
    State e = zero;
    for (int l = 0; l < 64; ++l) {
      ent[l] = e;
      const State f = fin[l];
      State r;
      r.s0 = fma(col[0].s0, e.s0, fma(col[1].s0, e.s1, f.s0));
      r.s1 = fma(col[0].s1, e.s0, fma(col[1].s1, e.s1, f.s1));
      r.t0 = fma(col[2].t0, e.t0, fma(col[3].t0, e.t1,
                                      fma(col[0].t0, e.s0, fma(col[1].t0, e.s1, f.t0))));
      r.t1 = fma(col[2].t1, e.t0, fma(col[3].t1, e.t1,
                                      fma(col[0].t1, e.s0, fma(col[1].t1, e.s1, f.t1))));
      e = r;
    }
  }
  __syncthreads();
  cur = ent[lane];
  for (long long kk = lo; kk < hi; ++kk) {
    double* __restrict__ f = st + kk * 4;
    const State fv = {f[0], f[1], f[2], f[3]};
    f[0] = cur.s0;
    f[1] = cur.s1;
    f[2] = cur.t0;
    f[3] = cur.t1;
    cur = ld_apply(m, cur, fv);
  }
}

__device__ __forceinline__ double ld_lufs(double power) { return -0.691 + 10.0 * log10(power); }

// sums v[0 .. n) of every thread over the workgroup: red[i][thread], a tree in a fixed order.
// Returns the totals to every thread.
template <int N>
__device__ __forceinline__ void ld_tree(double (&v)[N], double (*red)[LD_THREADS]) {
  const int tid = threadIdx.x;
  __syncthreads();  // red may still be read from the call before
#pragma unroll
  for (int i = 0; i < N; ++i) red[i][tid] = v[i];
  __syncthreads();
  for (int s = LD_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int i = 0; i < N; ++i) red[i][tid] += red[i][tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i][0];
}

// One workgroup per item. part [row][pieces] from pass 2; segsum [row][segs], z [row][blocks] and
// lj [item][blocks] are scratch of this launch.
__global__ __launch_bounds__(LD_THREADS) void loudness_finish_kernel(
    const double* __restrict__ part, Geom g, double* __restrict__ segsum, double* __restrict__ z,
    double* __restrict__ lj, double* __restrict__ out) {
  __shared__ double red[LD_MAX_CH + 1][LD_THREADS];
  const int tid = threadIdx.x;
  const int item = blockIdx.x;
  const int nch = g.channels;
  const size_t row0 = (size_t)item * nch;
  const double gain[LD_MAX_CH] = {1.0, 1.0, 1.0, 1.41, 1.41};

  // segments from their pieces, in sample order
  for (long long e = tid; e < g.segs * nch; e += LD_THREADS) {
    const int c = (int)(e / g.segs);
    const long long s = e - c * g.segs;
    long long a, b;
    if (!g.rem) {
      a = s * g.step;
      b = a + g.step;
    } else {
      const long long m = s >> 1;
      a = (s & 1) ? m * g.step + g.rem : m * g.step;
      b = (s & 1) ? (m + 1) * g.step : a + g.rem;
    }
    const double* __restrict__ pr = part + (row0 + c) * g.pieces;
    double sum = 0.0;
    for (long long p = a; p < b;) {
      const long long kk = p / LD_C;
      const long long idx = kk + s;
      if (idx < g.pieces) sum += pr[idx];
      const long long ce = (kk + 1) * LD_C;
      p = ce < b ? ce : b;
    }
    segsum[(row0 + c) * g.segs + s] = sum;
  }
  __syncthreads();  // segsum is read back by other threads of this workgroup

  // blocks from their segments; block loudness
  for (long long j = tid; j < g.blocks; j += LD_THREADS) {
    const long long s_lo = g.rem ? 2 * j : j;
    const long long s_hi = g.rem ? 2 * (j + g.q) + 1 : j + g.q;
    double w = 0.0;
    for (int c = 0; c < nch; ++c) {
      const double* __restrict__ sr = segsum + (row0 + c) * g.segs;
      double sum = 0.0;
      for (long long s = s_lo; s < s_hi && s < g.segs; ++s) sum += sr[s];
      const double zc = sum / (double)g.win;
      z[(row0 + c) * g.blocks + j] = zc;
      w += gain[c] * zc;
    }
    lj[(size_t)item * g.blocks + j] = ld_lufs(w);
  }
  __syncthreads();

  // the two gates: channel means over the blocks that pass, blocks j = tid, tid + 256, ... in
  // sequence, then the tree
  double gamma = -70.0;  // the first round's gate is the absolute one alone
  double result = -70.0;
  for (int round = 0; round < 2; ++round) {
    double v[LD_MAX_CH + 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // channel sums, count
    for (long long j = tid; j < g.blocks; j += LD_THREADS) {
      const double l = lj[(size_t)item * g.blocks + j];
      if (l > -70.0 && l > gamma) {
        for (int c = 0; c < nch; ++c) v[c] += z[(row0 + c) * g.blocks + j];
        v[LD_MAX_CH] += 1.0;
      }
    }
    ld_tree<LD_MAX_CH + 1>(v, red);
    if (!(v[LD_MAX_CH] > 0.0)) break;  // uniform: no block passes, -70
    double w = 0.0;
    for (int c = 0; c < nch; ++c) w += gain[c] * (v[c] / v[LD_MAX_CH]);
    const double l = ld_lufs(w);
    if (round == 0) {
      gamma = l - 10.0;
    } else {
      result = l > -70.0 ? l : -70.0;  // NaN and -inf read -70 too
    }
  }
  if (tid == 0) out[item] = result;
}

// ------------------------------------------------------------------------------- host side
thread_local char ld_error[192] = "";

// RBJ cookbook biquad in the operation order of vrvq_amd.codec._biquad, normalised by a0.
void ld_biquad(bool shelf, double gain_db, double q, double fc, double rate, int i, Coef* cf) {
  const double pi = 3.141592653589793;
  const double A = pow(10.0, gain_db / 40.0);
  const double w0 = 2.0 * pi * fc / rate;
  const double al = sin(w0) / (2.0 * q);
  const double c = cos(w0);
  double b[3], a[3];
  if (shelf) {
    b[0] = A * ((A + 1) + (A - 1) * c + 2 * sqrt(A) * al);
    b[1] = -2 * A * ((A - 1) + (A + 1) * c);
    b[2] = A * ((A + 1) + (A - 1) * c - 2 * sqrt(A) * al);
    a[0] = (A + 1) - (A - 1) * c + 2 * sqrt(A) * al;
    a[1] = 2 * ((A - 1) - (A + 1) * c);
    a[2] = (A + 1) - (A - 1) * c - 2 * sqrt(A) * al;
  } else {
    b[0] = (1 + c) / 2;
    b[1] = -(1 + c);
    b[2] = (1 + c) / 2;
    a[0] = 1 + al;
    a[1] = -2 * c;
    a[2] = 1 - al;
  }
  cf->b0[i] = b[0] / a[0];
  cf->b1[i] = b[1] / a[0];
  cf->b2[i] = b[2] / a[0];
  cf->a1[i] = a[1] / a[0];
  cf->a2[i] = a[2] / a[0];
}

// The zero-input cascade moves (s0, s1, t0, t1) by the 4 x 4 matrix below per sample (y1 = s0
// feeds the second stage); its LD_C-th power by repeated squaring in long double, rounded once.
void ld_transition(const Coef& cf, Trans* tr) {
  static_assert((LD_C & (LD_C - 1)) == 0, "LD_C is a power of two: squarings only");
  long double m[4][4] = {};
  const long double b0 = cf.b0[1], b1 = cf.b1[1], b2 = cf.b2[1], a1 = cf.a1[1], a2 = cf.a2[1];
  m[0][0] = -(long double)cf.a1[0];
  m[0][1] = 1.0L;
  m[1][0] = -(long double)cf.a2[0];
  m[2][0] = b1 - a1 * b0;
  m[2][2] = -a1;
  m[2][3] = 1.0L;
  m[3][0] = b2 - a2 * b0;
  m[3][2] = -a2;
  for (int n = 1; n < LD_C; n *= 2) {
    long double r[4][4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        long double s = 0.0L;
        for (int k = 0; k < 4; ++k) s += m[i][k] * m[k][j];
        r[i][j] = s;
      }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) m[i][j] = r[i][j];
  }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      tr->M1[i * 2 + j] = (double)m[i][j];
      tr->M2[i * 2 + j] = (double)m[2 + i][2 + j];
      tr->K[i * 2 + j] = (double)m[2 + i][j];
    }
}

int ld_plan(int sample_rate, int channels, long long length, Geom* g, Coef* cf, Trans* tr) {
  ld_error[0] = 0;
  if (sample_rate <= 0) {
    snprintf(ld_error, sizeof ld_error, "loudness: the sample rate must be positive (got %d)",
             sample_rate);
    return VRVQ_ERR_ARG;
  }
  if (channels < 1 || channels > LD_MAX_CH) {
    snprintf(ld_error, sizeof ld_error,
             "loudness: 1 to %d channels have a BS.1770 gain (got %d)", LD_MAX_CH, channels);
    return VRVQ_ERR_ARG;
  }
  if (length < 1 || length > LD_MAX_LENGTH) {
    snprintf(ld_error, sizeof ld_error, "loudness: the length must be in [1, 2^40] (got %lld)",
             length);
    return VRVQ_ERR_ARG;
  }
  const double sr = (double)sample_rate;
  g->win = (int)(0.4 * sr);
  g->step = (int)(0.4 * sr * 0.25);
  if (g->step < 1) {
    snprintf(ld_error, sizeof ld_error,
             "loudness: at %d Hz the 100 ms block step is shorter than one sample", sample_rate);
    return VRVQ_ERR_ARG;
  }
  const double dur = (double)length / sr;
  g->length = length;
  g->eff = dur < 0.5 ? length + (long long)((0.5 - dur) * sr) : length;
  g->channels = channels;
  g->q = g->win / g->step;
  g->rem = g->win % g->step;
  g->blocks = g->eff >= g->win ? (g->eff - g->win) / g->step + 1 : 0;
  if (g->blocks < 1) {  // int(0.5 sr) - 1 < int(0.4 sr): rates below 10 Hz only, kept as a guard
    snprintf(ld_error, sizeof ld_error, "loudness: %lld samples at %d Hz hold no 400 ms block",
             g->eff, sample_rate);
    return VRVQ_ERR_ARG;
  }
  g->chunks = (g->eff + LD_C - 1) / LD_C;
  const long long last = g->eff - 1, m = last / g->step;
  g->pieces = g->chunks + (g->rem ? 2 * m + ((last - m * g->step) >= g->rem ? 1 : 0) : m) + 1;
  g->segs = g->rem ? 2 * (g->blocks - 1 + g->q) + 1 : g->blocks - 1 + g->q;
  ld_biquad(true, 4.0, 1.0 / sqrt(2.0), 1500.0, sr, 0, cf);
  ld_biquad(false, 0.0, 0.5, 38.0, sr, 1, cf);
  ld_transition(*cf, tr);
  return VRVQ_OK;
}

// doubles of workspace per item: state, pieces, segment sums and block means per row; block
// loudness per item
long long ld_item_doubles(const Geom& g) {
  return (long long)g.channels * (g.chunks * 4 + g.pieces + g.segs + g.blocks) + g.blocks;
}

}  // namespace

extern "C" const char* vrvq_loudness_error(void) { return ld_error; }

extern "C" int vrvq_loudness_plan(int sample_rate, int channels, long long length, double* out) {
  Geom g;
  Coef cf;
  Trans tr;
  const int rc = ld_plan(sample_rate, channels, length, &g, &cf, &tr);
  if (rc) return rc;
  if (!out) {
    snprintf(ld_error, sizeof ld_error, "loudness: null plan output");
    return VRVQ_ERR_ARG;
  }
  out[0] = (double)g.eff;
  out[1] = (double)g.win;
  out[2] = (double)g.step;
  out[3] = (double)g.blocks;
  out[4] = (double)LD_C;
  out[5] = (double)g.chunks;
  out[6] = (double)(ld_item_doubles(g) * (long long)sizeof(double));
  out[7] = (double)g.pieces;
  for (int i = 0; i < 2; ++i) {
    out[8 + 5 * i] = cf.b0[i];
    out[9 + 5 * i] = cf.b1[i];
    out[10 + 5 * i] = cf.b2[i];
    out[11 + 5 * i] = cf.a1[i];
    out[12 + 5 * i] = cf.a2[i];
  }
  for (int i = 0; i < 4; ++i) {
    out[18 + i] = tr.M1[i];
    out[22 + i] = tr.M2[i];
    out[26 + i] = tr.K[i];
  }
  static_assert(VRVQ_LOUDNESS_PLAN_LEN == 30, "the plan's layout");
  return VRVQ_OK;
}

extern "C" int vrvq_loudness(const float* x, int items, int channels, long long length,
                             int sample_rate, void* workspace, double* out_lufs,
                             vrvq_stream_t stream) {
  Geom g;
  Coef cf;
  Trans tr;
  const int rc = ld_plan(sample_rate, channels, length, &g, &cf, &tr);
  if (rc) return rc;
  VRVQ_CHECK_ARG(x && workspace && out_lufs && items > 0);
  VRVQ_CHECK_ARG((long long)items * channels <= 65535);  // grid.y carries the rows
  VRVQ_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  const long long rows = (long long)items * channels;
  const long long groups = (g.chunks + LD_THREADS - 1) / LD_THREADS;  // <= 2^24
  double* ws = static_cast<double*>(workspace);
  double* state = ws;
  double* part = state + rows * g.chunks * 4;
  double* segsum = part + rows * g.pieces;
  double* z = segsum + rows * g.segs;
  double* lj = z + rows * g.blocks;
  const dim3 grid((unsigned)groups, (unsigned)rows);
  hipLaunchKernelGGL(loudness_pass_kernel<false>, grid, dim3(LD_THREADS), 0, as_stream(stream), x,
                     g, cf, state, part);
  int st = vrvq_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(loudness_carry_kernel, dim3((unsigned)rows), dim3(64), 0, as_stream(stream),
                     state, g.chunks, tr);
  st = vrvq_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(loudness_pass_kernel<true>, grid, dim3(LD_THREADS), 0, as_stream(stream), x,
                     g, cf, state, part);
  st = vrvq_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(loudness_finish_kernel, dim3((unsigned)items), dim3(LD_THREADS), 0,
                     as_stream(stream), part, g, segsum, z, lj, out_lufs);
  return vrvq_launch_status();
}
