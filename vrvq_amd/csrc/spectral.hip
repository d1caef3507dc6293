// Spectral distances of reconstructions against their inputs (include/vrvq.h "Spectral
// distance"): per row and per scale the two terms of models/loss.py:168-401 (MultiScaleSTFTLoss /
// MelSpectrogramLoss), mean |pow log10 max(E, eps) - pow log10 max(R, eps)| and mean |E - R| over
// the (mel or bin, frame) elements of the row's magnitude spectrograms. No spectrogram reaches
// memory: frames -> window -> FFT in LDS -> |.| -> banded mel projection -> the two differences
// -> fp64 sums.
//
// One launch per scale plus one. A 256-thread workgroup owns a tile of
// F = VRVQ_SPECTRAL_TILE_FRAMES(W) consecutive frames of one (row, scale): it stages the tile's
// sample span of both signals once (reflection applied at the load), then works through the tile
// in SP_BATCHES batches of G = F / SP_BATCHES frames. A batch holds 2 G real transforms of length
// W (estimate and reference of G frames, never packed into one complex transform: each signal's
// spectrum is computed from that signal alone), each run as a complex Stockham transform of
// length W / 2 over (even, odd) sample pairs -- radix-4 passes and one radix-2 pass when
// log2(W / 2) is odd -- plus the unpack step, 2 G * W / 2 = 2048 complex points whatever W is.
// The workgroup stores the tile's two fp64 partial sums; the finish kernel adds a (row, scale)'s
// tiles and divides by the element count.
//
// Which thread adds which element, and in what order, is a function of (scale, frame, bin)
// alone: not of the row's address (scalar loads), of the other rows or of their lengths. The
// estimate and the reference of a frame go through the same instructions, so equal signals give
// exactly 0. Twiddles and window are the caller's fp64-built tables; no fast-math intrinsic.
//
// Summation chains (fp64):
//   per thread   the thread's elements of the tile: item = frame_in_batch * n_items + element,
//                items tid, tid + 256, ... of batch 0, then batch 1, ...  (<= 5 per batch, 20 terms)
//   lanes        a 6-level xor tree;  waves  4 terms in sequence
//   tiles        per lane ceil(tiles / 64) terms in sequence, then the 6-level tree (finish)
//
// The gradient with respect to the estimate (include/vrvq.h "Gradient of the spectral distance")
// runs on the same tiles with the same transform functions: spectral_grad_tile_kernel recomputes
// a tile's spectra, forms the per-pair gradient, takes it back through bands, magnitude, inverse
// transform (the same passes on the conjugate) and window, and overlap-adds its frames into its
// span in LDS; spectral_grad_gather_kernel joins the overlapping spans, the reflection folds and
// the scales in a fixed order. No spectrogram reaches memory and no float atomics are used.
#include "common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_POINTS = 2048;  // complex points of a batch: G frames x 2 signals x W / 2
constexpr int SP_BATCHES = 4;    // batches per tile
constexpr int SP_MAX_SCALES = 16;
constexpr int SP_REFINE_CAP = 32;  // fp64 re-summed bins per batch of the gradient kernel, at most
constexpr long long SP_MAX_SAMPLES = 1LL << 32;
static_assert(SP_BATCHES * SP_POINTS == VRVQ_SPECTRAL_TILE_SAMPLES, "tile frames of the header");

struct SpScales {
  int n;
  int window[SP_MAX_SCALES];
  int n_items[SP_MAX_SCALES];    // n_mels, or W / 2 + 1 linear bins
  int tiles[SP_MAX_SCALES];
  long long ws_off[SP_MAX_SCALES];  // in doubles
};

__device__ __forceinline__ double sp_wave_tree(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ long long sp_row_length(const long long* __restrict__ lengths,
                                                   int ref_row, long long samples) {
  if (!lengths) return samples;
  const long long n = lengths[ref_row];
  return n < 0 ? 0 : (n > samples ? samples : n);
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * w: each component one product and one fma
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x));
}
// i * a
__device__ __forceinline__ float2 cmul_i(float2 a) { return make_float2(-a.y, a.x); }

// One radix-4 Stockham butterfly (decimation in frequency, forward): inputs a, b, c, d are
// elements p, p + n/4, p + n/2, p + 3n/4 of a length-n sub-transform; outputs go to 4p + k.
__device__ __forceinline__ void radix4(float2 a, float2 b, float2 c, float2 d, float2 w1,
                                       float2 w2, float2 w3, float2& y0, float2& y1, float2& y2,
                                       float2& y3) {
  const float2 apc = cadd(a, c), amc = csub(a, c), bpd = cadd(b, d), jbmd = cmul_i(csub(b, d));
  y0 = cadd(apc, bpd);
  y1 = cmul(csub(amc, jbmd), w1);
  y2 = cmul(csub(apc, bpd), w2);
  y3 = cmul(cadd(amc, jbmd), w3);
}

constexpr int sp_ilog2(int v) { return v <= 1 ? 0 : 1 + sp_ilog2(v >> 1); }

// The Stockham passes of SLOTS length-N transforms held in buf[cur] from sub-transform length NN0
// on (stride N / NN0): radix-4 passes, then one radix-2 pass when a factor 2 is left. Returns the
// buffer that holds the result, in natural order. Ends on a barrier.
template <int N, int SLOTS, int NN0>
__device__ __forceinline__ int sp_passes(float2 (*buf)[SP_POINTS], const float2* tw, int tid,
                                         int cur) {
  constexpr int W = 2 * N, Q = N / 4;
  static_assert(SLOTS * Q % SP_THREADS == 0, "whole butterflies per thread");
  int nn = NN0, s = N / NN0, ls = sp_ilog2(N / NN0);
#pragma unroll
  for (; nn >= 4; nn >>= 2, s <<= 2, ls += 2) {
    const float2* __restrict__ xb = buf[cur];
    float2* __restrict__ yb = buf[cur ^ 1];
#pragma unroll
    for (int i = 0; i < SLOTS * Q / SP_THREADS; ++i) {
      const int b = tid + i * SP_THREADS, slot = b / Q, t = b % Q, p = t >> ls, q = t & (s - 1);
      const float2* __restrict__ x = xb + slot * N + t;
      const int ti = p * 2 * s;  // exp(-2 pi i p / nn) = tw[p * W / nn], W / nn = 2 s
      float2 y0, y1, y2, y3;
      radix4(x[0], x[Q], x[2 * Q], x[3 * Q], tw[ti], tw[2 * ti], tw[3 * ti], y0, y1, y2, y3);
      float2* __restrict__ y = yb + slot * N + q + 4 * s * p;
      y[0] = y0;
      y[s] = y1;
      y[2 * s] = y2;
      y[3 * s] = y3;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (nn == 2) {  // log2(N) odd: one radix-2 pass, s = N / 2, twiddle 1
    const float2* __restrict__ xb = buf[cur];
    float2* __restrict__ yb = buf[cur ^ 1];
#pragma unroll
    for (int i = 0; i < SLOTS * (N / 2) / SP_THREADS; ++i) {
      const int b = tid + i * SP_THREADS, slot = b / (N / 2), q = b % (N / 2);
      const float2 a = xb[slot * N + q], c = xb[slot * N + q + N / 2];
      yb[slot * N + q] = cadd(a, c);
      yb[slot * N + q + N / 2] = csub(a, c);
    }
    __syncthreads();
    cur ^= 1;
  }
  (void)W;
  return cur;
}

// Batch fb of a tile: the 2 G transforms (estimate and reference of G frames) of the staged
// spans, Z of slot 2 g + signal in the returned buffer. span is [2][SPAN].
template <int W>
__device__ __forceinline__ int sp_batch_transform(const float* __restrict__ span, int fb,
                                                  const float2* tw,
                                                  const float* __restrict__ win_g,
                                                  float2 (*buf)[SP_POINTS], int tid) {
  constexpr int N = W / 2, HOP = W / 4, Q = N / 4;
  constexpr int G = SP_POINTS / W, F = SP_BATCHES * G, SLOTS = 2 * G;
  constexpr int SPAN = W + (F - 1) * HOP;
  static_assert(SLOTS * Q % SP_THREADS == 0, "whole butterflies per thread");
  // first pass (n = N, s = 1): windowed (even, odd) sample pairs straight from the span
#pragma unroll
  for (int i = 0; i < SLOTS * Q / SP_THREADS; ++i) {
    const int b = tid + i * SP_THREADS, slot = b / Q, t = b % Q;
    const float* __restrict__ x = span + (slot & 1) * SPAN + (fb * G + (slot >> 1)) * HOP;
    float2 in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = t + j * Q;
      const float2 v = *reinterpret_cast<const float2*>(x + 2 * c);
      const float2 h = *reinterpret_cast<const float2*>(win_g + 2 * c);
      in[j] = make_float2(v.x * h.x, v.y * h.y);
    }
    float2 y0, y1, y2, y3;
    radix4(in[0], in[1], in[2], in[3], tw[2 * t], tw[4 * t], tw[6 * t], y0, y1, y2, y3);
    float2* __restrict__ y = &buf[0][slot * N + 4 * t];
    y[0] = y0;
    y[1] = y1;
    y[2] = y2;
    y[3] = y3;
  }
  __syncthreads();
  return sp_passes<N, SLOTS, N / 4>(buf, tw, tid, 0);
}

// Twice bin k of the real transform from Z = zs (one slot, N points):
// 2 X[k] = (Z[k] + conj Z[N-k]) - i w_k (Z[k] - conj Z[N-k]), w_k = exp(-2 pi i k / W)
template <int N>
__device__ __forceinline__ float2 sp_unpack_bin(const float2* __restrict__ zs, int k,
                                                const float2* tw) {
  const float2 zk = zs[k & (N - 1)];
  float2 zc = zs[(N - k) & (N - 1)];
  zc.y = -zc.y;
  const float2 a = cadd(zk, zc), wb = cmul(csub(zk, zc), tw[k]);
  return make_float2(a.x + wb.y, a.y - wb.x);
}

// |X| of bins 0..N of every slot of zb -> mags[slot][NB]
template <int N, int SLOTS>
__device__ __forceinline__ void sp_magnitudes(const float2* __restrict__ zb, const float2* tw,
                                              float* __restrict__ mags, int tid) {
  constexpr int NB = N + 1;
  for (int i = tid; i < SLOTS * NB; i += SP_THREADS) {
    const int slot = i / NB, k = i % NB;
    const float2 x2 = sp_unpack_bin<N>(zb + slot * N, k, tw);
    mags[i] = 0.5f * sqrtf(fmaf(x2.x, x2.x, x2.y * x2.y));
  }
}

// E and R of element m of frame g from the batch's magnitudes (the banded mel projection in
// ascending bins, or bin m itself)
template <int NB>
__device__ __forceinline__ void sp_project(const float* __restrict__ mags, int g, int m,
                                           int n_mels, const int* __restrict__ bands,
                                           const float* __restrict__ bw, float& E, float& R) {
  const float* __restrict__ me = mags + (2 * g) * NB;
  const float* __restrict__ mr = me + NB;
  if (n_mels > 0) {
    int st = bands[m], ln = bands[n_mels + m];
    const int off = bands[2 * n_mels + m];
    st = st < 0 ? 0 : (st > NB ? NB : st);  // a band never leaves the bins
    ln = ln > NB - st ? NB - st : ln;
    E = 0.0f;
    R = 0.0f;
    for (int j = 0; j < ln; ++j) {  // ascending bins
      const float wgt = bw[off + j];
      E = fmaf(wgt, me[st + j], E);
      R = fmaf(wgt, mr[st + j], R);
    }
  } else {
    E = me[m];
    R = mr[m];
  }
}

// Both signals' sample f0 * HOP - W / 2 + i, i < SPAN, reflected at 0 and at n without repeating
// the edge; positions past the row's last frame are clamped (their frames are not counted)
template <int SPAN>
__device__ __forceinline__ void sp_stage_spans(const float* __restrict__ e,
                                               const float* __restrict__ r, long long base,
                                               long long n, float* __restrict__ span, int tid) {
  for (int i = tid; i < SPAN; i += SP_THREADS) {
    long long idx = base + i;
    if (idx < 0) idx = -idx;
    if (idx >= n) idx = 2 * (n - 1) - idx;
    idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
    span[i] = e[idx];
    span[SPAN + i] = r[idx];
  }
}

// ws[row][tile][2]: the sums of the two terms over the tile's frames and all elements.
template <int W>
__global__ __launch_bounds__(SP_THREADS) void spectral_tile_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, int ref_rows, long long samples,
    const long long* __restrict__ lengths, const float2* __restrict__ tw_g,
    const float* __restrict__ win_g, int n_mels, const int* __restrict__ bands,
    const float* __restrict__ bw, double eps, double pw, double* __restrict__ ws) {
  constexpr int N = W / 2, NB = N + 1, HOP = W / 4, Q = N / 4;
  constexpr int G = SP_POINTS / W, F = SP_BATCHES * G, SLOTS = 2 * G;
  constexpr int SPAN = W + (F - 1) * HOP;
  static_assert(SLOTS * Q % SP_THREADS == 0, "whole butterflies per thread");
  static_assert(SLOTS * NB <= 2 * SP_POINTS, "magnitudes fit the idle transform buffer");
  __shared__ float2 tw[W];                // exp(-2 pi i k / W)
  __shared__ __attribute__((aligned(8))) float span[2][SPAN];
  __shared__ float2 buf[2][SP_POINTS];
  __shared__ double part[SP_WAVES][2];

  const int tid = threadIdx.x;
  const int row = blockIdx.y, rrow = row % ref_rows;
  const int tile = blockIdx.x, tiles = gridDim.x;
  double* __restrict__ out = ws + ((size_t)row * tiles + tile) * 2;
  const long long n = sp_row_length(lengths, rrow, samples);
  const long long frames = n > N ? 1 + n / HOP : 0;  // n <= W / 2: the finish kernel writes NaN
  const long long f0 = (long long)tile * F;
  const int valid = (int)(frames - f0 < 0 ? 0 : (frames - f0 > F ? F : frames - f0));
  if (valid == 0) {  // uniform over the workgroup
    if (tid < 2) out[tid] = 0.0;
    return;
  }

  for (int k = tid; k < W; k += SP_THREADS) tw[k] = tw_g[k];
  sp_stage_spans<SPAN>(est + (size_t)row * samples, ref + (size_t)rrow * samples, f0 * HOP - N, n,
                       &span[0][0], tid);
  __syncthreads();

  const int n_items = n_mels > 0 ? n_mels : NB;
  double acc_log = 0.0, acc_mag = 0.0;
  for (int fb = 0; fb < SP_BATCHES; ++fb) {
    const int gv = valid - fb * G < G ? valid - fb * G : G;  // frames of this batch that count
    if (gv <= 0) break;                                      // uniform

    const int cur = sp_batch_transform<W>(&span[0][0], fb, tw, win_g, buf, tid);

    // unpack the real transform's bins 0..N from Z = buf[cur] and take magnitudes
    float* __restrict__ mags = reinterpret_cast<float*>(buf[cur ^ 1]);
    sp_magnitudes<N, SLOTS>(buf[cur], tw, mags, tid);
    __syncthreads();

    // projection and the two differences; item = frame * n_items + element
    for (int item = tid; item < gv * n_items; item += SP_THREADS) {
      const int g = item / n_items, m = item - g * n_items;
      float E, R;
      sp_project<NB>(mags, g, m, n_mels, bands, bw, E, R);
      const double dE = (double)E, dR = (double)R;
      const double cE = dE < eps ? eps : dE, cR = dR < eps ? eps : dR;  // keeps NaN
      acc_log += fabs(pw * log10(cE) - pw * log10(cR));
      acc_mag += fabs(dE - dR);
    }
    __syncthreads();  // the next batch overwrites both buffers
  }

  acc_log = sp_wave_tree(acc_log);
  acc_mag = sp_wave_tree(acc_mag);
  if ((tid & 63) == 0) {
    part[tid >> 6][0] = acc_log;
    part[tid >> 6][1] = acc_mag;
  }
  __syncthreads();
  if (tid < 2) {
    double tot = part[0][tid];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) tot += part[w][tid];
    out[tid] = tot;
  }
}

// One wave per row: for each scale in turn, lane l adds tiles l, l + 64, ... in sequence, then
// the xor tree; terms[row][scale][2] = sums / (n_items * frames), NaN for a row no longer than
// W / 2. distance[row] = sum over the scales, in their order, of log_weight * terms[..][0] +
// mag_weight * terms[..][1].
__global__ __launch_bounds__(64) void spectral_finish_kernel(
    const double* __restrict__ ws, SpScales sc, int ref_rows, long long samples,
    const long long* __restrict__ lengths, double log_weight, double mag_weight,
    double* __restrict__ terms, double* __restrict__ distance) {
  const int row = blockIdx.x;
  const long long n = sp_row_length(lengths, row % ref_rows, samples);
  double dist = 0.0;
  for (int scale = 0; scale < sc.n; ++scale) {
    const int tiles = sc.tiles[scale], W = sc.window[scale];
    const double* __restrict__ w = ws + sc.ws_off[scale] + (size_t)row * tiles * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) {
      s0 += w[2 * t];
      s1 += w[2 * t + 1];
    }
    s0 = sp_wave_tree(s0);
    s1 = sp_wave_tree(s1);
    if (n > W / 2) {
      const double count = (double)(1 + n / (W / 4)) * (double)sc.n_items[scale];
      s0 = s0 / count;
      s1 = s1 / count;
    } else {
      s0 = s1 = __longlong_as_double(0x7ff8000000000000LL);
    }
    dist += log_weight * s0 + mag_weight * s1;
    if (threadIdx.x == 0) {
      double* o = terms + ((size_t)row * sc.n + scale) * 2;
      o[0] = s0;
      o[1] = s1;
    }
  }
  if (threadIdx.x == 0 && distance) distance[row] = dist;
}

// sgn with sgn(0) = 0; NaN stays NaN
__device__ __forceinline__ double sp_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d); }

// Gradient of distance[row] with respect to est[row], one (row, scale) tile per workgroup.
// ws[row][tile][SPAN] fp32: the tile's frames overlap-added in ascending frame order at span
// position i = sample f0 * HOP - W / 2 + i of the padded row; the gather kernel joins the tiles.
// Per batch: the forward's transforms and magnitudes (sp_batch_transform / sp_magnitudes /
// sp_project: E and R are the forward's bits), the per-pair g in fp64 rounded once, G-bar
// through the bands in ascending m, Y[k] = G-bar X / |X| (halved off bins 0 and N) packed back to
// a length-N spectrum, the same Stockham passes on its conjugate (the inverse by sign), window,
// and overlap-add. Nothing but the span leaves LDS; a tile past the row's frames stores nothing.
template <int W>
__global__ __launch_bounds__(SP_THREADS) void spectral_grad_tile_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, int ref_rows, long long samples,
    const long long* __restrict__ lengths, const float2* __restrict__ tw_g,
    const float* __restrict__ win_g, int n_mels, const int* __restrict__ bands,
    const float* __restrict__ bw, double eps, double pw, double log_weight, double mag_weight,
    const double* __restrict__ grad_distance, float* __restrict__ ws) {
  constexpr int N = W / 2, NB = N + 1, HOP = W / 4;
  constexpr int G = SP_POINTS / W, F = SP_BATCHES * G, SLOTS = 2 * G;
  constexpr int SPAN = W + (F - 1) * HOP;
  // magnitudes of both signals, then the G frames' g, share the idle transform buffer
  static_assert(SLOTS * NB + G * NB <= 2 * SP_POINTS, "magnitudes and g fit the idle buffer");
  static_assert(G * N * 4 % SP_THREADS == 0 && G * N <= SP_POINTS, "inverse transforms fit");
  __shared__ float2 tw[W];                // exp(-2 pi i k / W)
  __shared__ __attribute__((aligned(8))) float span[2][SPAN];
  __shared__ float2 buf[2][SP_POINTS];
  __shared__ float acc[SPAN];             // the tile's overlap-added gradient
  __shared__ int mlo[NB], mhi[NB];        // first and last mel band that holds a bin
  __shared__ float fpow[SP_WAVES > G ? SP_WAVES : G];  // sum |X|^2 of a frame (or of a wave's part)
  __shared__ int nref;
  __shared__ unsigned short rlist[SP_REFINE_CAP];  // the batch's isolated ill-conditioned bins
  constexpr int P = SP_THREADS / G;         // threads per frame of the power sums

  const int tid = threadIdx.x;
  const int row = blockIdx.y, rrow = row % ref_rows;
  const int tile = blockIdx.x, tiles = gridDim.x;
  const long long n = sp_row_length(lengths, rrow, samples);
  const long long frames = n > N ? 1 + n / HOP : 0;  // n <= W / 2: the gather kernel writes NaN
  const long long f0 = (long long)tile * F;
  const int valid = (int)(frames - f0 < 0 ? 0 : (frames - f0 > F ? F : frames - f0));
  if (valid == 0) return;  // uniform over the workgroup; the gather kernel reads no such tile

  for (int k = tid; k < W; k += SP_THREADS) tw[k] = tw_g[k];
  for (int i = tid; i < SPAN; i += SP_THREADS) acc[i] = 0.0f;
  for (int k = tid; k < NB; k += SP_THREADS) {
    mlo[k] = 0x7fffffff;
    mhi[k] = -1;
  }
  sp_stage_spans<SPAN>(est + (size_t)row * samples, ref + (size_t)rrow * samples, f0 * HOP - N, n,
                       &span[0][0], tid);
  __syncthreads();
  // integer min / max: the result does not depend on the order of arrival
  for (int m = tid; m < n_mels; m += SP_THREADS) {
    int st = bands[m], ln = bands[n_mels + m];
    st = st < 0 ? 0 : (st > NB ? NB : st);
    ln = ln > NB - st ? NB - st : ln;
    for (int j = 0; j < ln; ++j) {
      atomicMin(&mlo[st + j], m);
      atomicMax(&mhi[st + j], m);
    }
  }  // visible after the barriers of the first batch's transforms

  const int n_items = n_mels > 0 ? n_mels : NB;
  const double upstream = grad_distance[row];
  const double count = (double)frames * (double)n_items;
  const double ln10 = 2.302585092994045684;
  for (int fb = 0; fb < SP_BATCHES; ++fb) {
    const int gv = valid - fb * G < G ? valid - fb * G : G;  // frames of this batch that count
    if (gv <= 0) break;                                      // uniform

    const int cur = sp_batch_transform<W>(&span[0][0], fb, tw, win_g, buf, tid);
    float* __restrict__ mags = reinterpret_cast<float*>(buf[cur ^ 1]);
    float* __restrict__ gb = mags + SLOTS * NB;  // g[frame][element]
    sp_magnitudes<N, SLOTS>(buf[cur], tw, mags, tid);
    __syncthreads();

    {  // sum |X|^2 of each estimate frame: P threads per frame, bins l, l + P, ..., then a tree
      const int g = tid / P, l = tid % P;
      float sq = 0.0f;
      for (int k = l; k < NB; k += P) {
        const float m = mags[(2 * g) * NB + k];
        sq = fmaf(m, m, sq);
      }
#pragma unroll
      for (int m = (P < 64 ? P : 64) / 2; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);
      if (P <= 64 ? l == 0 : (tid & 63) == 0) fpow[P <= 64 ? g : tid >> 6] = sq;
      if (tid == 0) nref = 0;
    }
    // g of every (frame, element) pair, formed in fp64 and rounded once
    for (int item = tid; item < gv * n_items; item += SP_THREADS) {
      const int g = item / n_items, m = item - g * n_items;
      float E, R;
      sp_project<NB>(mags, g, m, n_mels, bands, bw, E, R);
      const double dE = (double)E, dR = (double)R;
      const double cE = dE < eps ? eps : dE, cR = dR < eps ? eps : dR;  // keeps NaN
      const double dl = pw * log10(cE) - pw * log10(cR);
      // the clamp passes the gradient where E >= eps (NaN passes too)
      const double gl = dE < eps ? 0.0 : log_weight * pw / (ln10 * dE) * sp_sign(dl);
      gb[item] = (float)(upstream * ((gl + mag_weight * sp_sign(dE - dR)) / count));
    }
    __syncthreads();

    // Y[k] of the estimate's frames into the reference's slots (their Z is spent): bins 0 and N
    // are real and share point 0, the others are halved (each bin counts once)
    auto gbar_of = [&](int g, int k) {
      if (n_mels <= 0) return gb[g * n_items + k];
      float gbar = 0.0f;
      for (int m = mlo[k]; m <= mhi[k]; ++m) {  // ascending bands
        int st = bands[m], ln = bands[n_mels + m];
        const int off = bands[2 * n_mels + m];
        st = st < 0 ? 0 : (st > NB ? NB : st);
        ln = ln > NB - st ? NB - st : ln;
        const int j = k - st;
        if (j >= 0 && j < ln) gbar = fmaf(bw[off + j], gb[g * n_items + m], gbar);
      }
      return gbar;
    };
    auto store_y = [&](int g, int k, float dx, float dy) {
      float* __restrict__ y = reinterpret_cast<float*>(buf[cur] + (2 * g + 1) * N);
      if (k == 0) {
        y[0] = dx;
      } else if (k == N) {
        y[1] = dx;
      } else {
        y[2 * k] = 0.5f * dx;
        y[2 * k + 1] = 0.5f * dy;
      }
    };
    for (int i = tid; i < gv * NB; i += SP_THREADS) {
      const int g = i / NB, k = i - g * NB;
      const float gbar = gbar_of(g, k);
      const float2 x2 = sp_unpack_bin<N>(buf[cur] + (2 * g) * N, k, tw);
      const float mag = mags[(2 * g) * NB + k];
      float2 d = make_float2(0.0f, 0.0f);
      if (mag != 0.0f) d = make_float2(gbar * ((0.5f * x2.x) / mag), gbar * ((0.5f * x2.y) / mag));
      store_y(g, k, d.x, d.y);
      // a bin under 2^-6 of the frame's rms magnitude: the transform's error, an ulp of the rms,
      // is 2^-18 of it and more, and 1 / |X| carries that into the gradient. Counted, and the
      // first SP_REFINE_CAP listed: a batch with more of them is left as fp32 gives it (below).
      // Once the count has passed the cap it only has to stay there, so later finds skip the
      // atomic; whether the count passes the cap does not depend on the order of arrival.
      float power = fpow[P <= 64 ? g : g * (P / 64)];
      for (int w = 1; w < P / 64; ++w) power += fpow[g * (P / 64) + w];
      if (mag * mag < power * (1.0f / (4096.0f * NB)) &&
          *const_cast<volatile int*>(&nref) <= SP_REFINE_CAP) {
        const int pos = atomicAdd(&nref, 1);
        if (pos < SP_REFINE_CAP) rlist[pos] = (unsigned short)i;
      }
    }
    __syncthreads();

    // Isolated ill-conditioned bins again, from the staged samples in fp64: X[k] = sum_t x[t]
    // hann[t] exp(-2 pi i k t / W). One wave per listed bin: lane l adds terms l, l + 64, ... with
    // twiddle and window advanced by a fixed rotation (sincospi once for the start and once for the
    // step, at most W / 64 = 32 steps), then the wave tree. That X / |X| replaces the fp32 one,
    // and for the linear bins its |X| the 1 / E of g (the sign and clamp decisions stay the
    // forward's). At most SP_REFINE_CAP bins, four at a time: the cost is bounded whatever the
    // signal. A batch that lists more (a steep spectrum: most bins lie under the threshold) keeps
    // the fp32 values for all of them, as the torch composition does. The order of the list plays
    // no part: every item is computed alone, the same way in any wave, and stored to its own place.
    const int nr = nref;
    if (nr <= SP_REFINE_CAP) {  // uniform
      const int lane = tid & 63;
      for (int r = tid >> 6; r < nr; r += SP_WAVES) {
        const int i = rlist[r], g = i / NB, k = i - g * NB;
        const float* __restrict__ x = &span[0][(fb * G + g) * HOP];
        double re = 0.0, im = 0.0;
        if (lane < W) {
          double sn, cs, dsn, dcs, wsn, wcs, dwsn, dwcs;
          sincospi(2.0 * ((k * lane) & (W - 1)) / W, &sn, &cs);
          sincospi(2.0 * ((k * 64) & (W - 1)) / W, &dsn, &dcs);
          sincospi(2.0 * lane / W, &wsn, &wcs);
          sincospi(2.0 * (64 & (W - 1)) / W, &dwsn, &dwcs);
          for (int t = lane; t < W; t += 64) {
            const double y = (double)x[t] * (0.5 - 0.5 * wcs);
            re = fma(y, cs, re);
            im = fma(-y, sn, im);
            const double c1 = cs * dcs - sn * dsn, w1 = wcs * dwcs - wsn * dwsn;
            sn = sn * dcs + cs * dsn;
            cs = c1;
            wsn = wsn * dwcs + wcs * dwsn;
            wcs = w1;
          }
        }
        const double xr = sp_wave_tree(re), xi = sp_wave_tree(im);
        if (lane == 0) {
          const double m = sqrt(xr * xr + xi * xi);
          double gf;
          if (n_mels > 0) {
            gf = (double)gbar_of(g, k);
          } else {
            const double dE = (double)mags[(2 * g) * NB + k], dR = (double)mags[(2 * g + 1) * NB + k];
            const double cE = dE < eps ? eps : dE, cR = dR < eps ? eps : dR;
            const double dl = pw * log10(cE) - pw * log10(cR);
            const double gl = dE < eps ? 0.0 : log_weight * pw / (ln10 * m) * sp_sign(dl);
            gf = upstream * ((gl + mag_weight * sp_sign(dE - dR)) / count);
          }
          if (m > 0.0) store_y(g, k, (float)(gf * (xr / m)), (float)(gf * (xi / m)));
        }
      }
    }
    __syncthreads();

    // Frames g >= gv of the batch are packed and transformed too; their Y slots still hold the
    // reference's Z, so anything, Inf and NaN included, may come out of them. Nothing reads it:
    // the overlap-add below takes frames g < gv only.
    // pack to the length-N spectrum whose inverse is (g[2c], g[2c+1]) and store its conjugate:
    // Z'[k] = (Y[k] + conj Y[N-k]) + i conj(w_k) (Y[k] - conj Y[N-k])
    for (int i = tid; i < G * N; i += SP_THREADS) {
      const int g = i / N, k = i - g * N;
      const float2* __restrict__ y = buf[cur] + (2 * g + 1) * N;
      float2 yk = y[k], yc = y[(N - k) & (N - 1)];
      if (k == 0) {
        yc = make_float2(yk.y, 0.0f);
        yk.y = 0.0f;
      }
      yc.y = -yc.y;
      float2 wc = tw[k];
      wc.y = -wc.y;
      const float2 a = cadd(yk, yc), b = cmul_i(cmul(csub(yk, yc), wc));
      buf[cur ^ 1][i] = make_float2(a.x + b.x, -(a.y + b.y));
    }
    __syncthreads();
    const int res = sp_passes<N, G, N>(buf, tw, tid, cur ^ 1);

    // window and overlap-add: one thread per sample of the batch's span, frames ascending
    const float* __restrict__ fv = reinterpret_cast<const float*>(buf[res]);
    const int lb = W + (gv - 1) * HOP;
    for (int i = tid; i < lb; i += SP_THREADS) {
      const int g_lo = i >= W ? (i - W) / HOP + 1 : 0;
      const int g_hi = i / HOP < gv - 1 ? i / HOP : gv - 1;
      float a = acc[fb * G * HOP + i];
      for (int g = g_lo; g <= g_hi; ++g) {
        const int s = i - g * HOP;
        const float v = fv[g * W + s];
        a = fmaf(win_g[s], (s & 1) ? -v : v, a);  // odd samples: the conjugate's sign
      }
      acc[fb * G * HOP + i] = a;
    }
    __syncthreads();  // the next batch overwrites both buffers
  }

  float* __restrict__ out = ws + ((size_t)row * tiles + tile) * SPAN;
  for (int i = tid; i < SPAN; i += SP_THREADS) out[i] = acc[i];
}

struct SpGradScales {
  int n;
  int window[SP_MAX_SCALES];
  int tiles[SP_MAX_SCALES];
  long long ws_off[SP_MAX_SCALES];  // in floats
};

// One thread per sample: per scale the (at most two) tiles that hold padded position p, tile t
// before t + 1, for p = i, then the left fold p = -i, then the right fold p = 2 (n - 1) - i; the
// scales added in their order. 0 past the row's length; NaN for a row no longer than some W / 2.
__global__ __launch_bounds__(SP_THREADS) void spectral_grad_gather_kernel(
    const float* __restrict__ ws, SpGradScales sc, int ref_rows, long long samples,
    const long long* __restrict__ lengths, float* __restrict__ grad) {
  const int row = blockIdx.y;
  const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= samples) return;
  const long long n = sp_row_length(lengths, row % ref_rows, samples);
  float total = 0.0f;
  bool nan = false;
  for (int scale = 0; scale < sc.n; ++scale) {
    const int W = sc.window[scale], N = W / 2, HOP = W / 4;
    const int F = VRVQ_SPECTRAL_TILE_FRAMES(W), TS = F * HOP, SPAN = W + (F - 1) * HOP;
    if (n <= N) {
      nan = true;
      continue;
    }
    if (i >= n) continue;
    const long long vt = (1 + n / HOP + F - 1) / F;  // tiles with frames: the others stored nothing
    const float* __restrict__ base = ws + sc.ws_off[scale] + (size_t)row * sc.tiles[scale] * SPAN;
    auto at = [&](long long p) {
      const long long u = p + N, t = u / TS;
      const int o = (int)(u - t * TS);
      float r = 0.0f;
      if (t >= 1 && o + TS < SPAN && t - 1 < vt) r = base[(size_t)(t - 1) * SPAN + o + TS];
      if (t < vt) r += base[(size_t)t * SPAN + o];
      return r;
    };
    float v = at(i);
    if (i >= 1 && i <= N) v += at(-i);
    if (i <= n - 2 && i >= n - 1 - N) v += at(2 * (n - 1) - i);
    total += v;
  }
  grad[(size_t)row * samples + i] = nan ? __int_as_float(0x7fc00000) : total;
}

bool window_ok(int w) { return w >= 32 && w <= 2048 && (w & (w - 1)) == 0; }

long long tiles_of(long long samples, int w) {
  const long long frames = 1 + samples / (w / 4), f = VRVQ_SPECTRAL_TILE_FRAMES(w);
  return (frames + f - 1) / f;
}

// Shape checks shared by the two entry points; fills sc and the workspace size.
int plan(int rows, long long samples, int n_scales, const int* windows, const int* n_mels,
         SpScales* sc, long long* doubles) {
  VRVQ_CHECK_ARG(rows > 0 && rows <= 65535 && samples > 0 && samples <= SP_MAX_SAMPLES);
  VRVQ_CHECK_ARG(windows && n_scales > 0 && n_scales <= SP_MAX_SCALES);
  long long off = 0;
  sc->n = n_scales;
  for (int s = 0; s < n_scales; ++s) {
    const int w = windows[s];
    VRVQ_CHECK_ARG(window_ok(w));
    const int nm = n_mels ? n_mels[s] : 0;
    VRVQ_CHECK_ARG(nm >= 0 && nm <= w / 2 + 1);
    sc->window[s] = w;
    sc->n_items[s] = nm > 0 ? nm : w / 2 + 1;
    sc->tiles[s] = (int)tiles_of(samples, w);
    sc->ws_off[s] = off;
    off += (long long)rows * sc->tiles[s] * 2;
  }
  *doubles = off;
  return VRVQ_OK;
}

template <int W>
void launch_tile(dim3 grid, hipStream_t st, const float* est, const float* ref, int ref_rows,
                 long long samples, const long long* lengths, const float* table, int n_mels,
                 const int* bands, const float* bw, double eps, double pw, double* ws) {
  hipLaunchKernelGGL(spectral_tile_kernel<W>, grid, dim3(SP_THREADS), 0, st, est, ref, ref_rows,
                     samples, lengths, reinterpret_cast<const float2*>(table), table + 2 * W,
                     n_mels, bands, bw, eps, pw, ws);
}

// plan() with the gradient's workspace: per scale [rows][tiles][SPAN] floats.
int grad_plan(int rows, long long samples, int n_scales, const int* windows, const int* n_mels,
              SpGradScales* gs, long long* floats) {
  SpScales sc;
  long long doubles = 0;
  const int rc = plan(rows, samples, n_scales, windows, n_mels, &sc, &doubles);
  if (rc) return rc;
  long long off = 0;
  gs->n = n_scales;
  for (int s = 0; s < n_scales; ++s) {
    const int w = sc.window[s];
    const long long span = w + (VRVQ_SPECTRAL_TILE_FRAMES(w) - 1) * (w / 4);
    gs->window[s] = w;
    gs->tiles[s] = sc.tiles[s];
    gs->ws_off[s] = off;
    off += (long long)rows * sc.tiles[s] * span;
  }
  *floats = off;
  return VRVQ_OK;
}

template <int W>
void launch_grad_tile(dim3 grid, hipStream_t st, const float* est, const float* ref, int ref_rows,
                      long long samples, const long long* lengths, const float* table, int n_mels,
                      const int* bands, const float* bw, double eps, double pw, double lw,
                      double mw, const double* grad_distance, float* ws) {
  hipLaunchKernelGGL(spectral_grad_tile_kernel<W>, grid, dim3(SP_THREADS), 0, st, est, ref,
                     ref_rows, samples, lengths, reinterpret_cast<const float2*>(table),
                     table + 2 * W, n_mels, bands, bw, eps, pw, lw, mw, grad_distance, ws);
}

}  // namespace

extern "C" int vrvq_spectral_distance_grad_workspace(int rows, long long samples, int n_scales,
                                                     const int* windows, long long* bytes) {
  VRVQ_CHECK_ARG(bytes);
  SpGradScales gs;
  long long floats = 0;
  const int rc = grad_plan(rows, samples, n_scales, windows, nullptr, &gs, &floats);
  if (rc) return rc;
  *bytes = (floats * (long long)sizeof(float) + 7) / 8 * 8;
  return VRVQ_OK;
}

extern "C" int vrvq_spectral_distance_grad(
    const float* est, const float* ref, int rows, int ref_rows, long long samples,
    const long long* lengths, int n_scales, const int* windows, const int* n_mels,
    const float* const* tables, const int* const* bands, const float* const* band_weights,
    double clamp_eps, double pow, double log_weight, double mag_weight,
    const double* grad_distance, float* grad_est, void* workspace, long long workspace_bytes,
    vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(est && ref && grad_distance && grad_est && workspace && windows && n_mels &&
                 tables);
  VRVQ_CHECK_ARG(ref_rows > 0 && rows % ref_rows == 0 && clamp_eps > 0.0);
  SpGradScales gs;
  long long floats = 0;
  int rc = grad_plan(rows, samples, n_scales, windows, n_mels, &gs, &floats);
  if (rc) return rc;
  for (int s = 0; s < n_scales; ++s) {
    VRVQ_CHECK_ARG(tables[s] && (reinterpret_cast<uintptr_t>(tables[s]) & 7) == 0);
    if (n_mels[s] > 0)
      VRVQ_CHECK_ARG(bands && band_weights && bands[s] && band_weights[s]);
    if (!lengths) VRVQ_CHECK_ARG(samples > windows[s] / 2);
  }
  VRVQ_CHECK_ARG(workspace_bytes >= floats * (long long)sizeof(float));
  VRVQ_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  for (int s = 0; s < n_scales; ++s) {
    const dim3 grid((unsigned)gs.tiles[s], (unsigned)rows);
    const int nm = n_mels[s];
    const int* bd = nm > 0 ? bands[s] : nullptr;
    const float* bw = nm > 0 ? band_weights[s] : nullptr;
    float* w = ws + gs.ws_off[s];
#define SP_CASE(WW)                                                                            \
  case WW:                                                                                     \
    launch_grad_tile<WW>(grid, st, est, ref, ref_rows, samples, lengths, tables[s], nm, bd,    \
                         bw, clamp_eps, pow, log_weight, mag_weight, grad_distance, w);        \
    break;
    switch (windows[s]) {
      SP_CASE(32)
      SP_CASE(64)
      SP_CASE(128)
      SP_CASE(256)
      SP_CASE(512)
      SP_CASE(1024)
      SP_CASE(2048)
      default:
        return VRVQ_ERR_ARG;
    }
#undef SP_CASE
    rc = vrvq_launch_status();
    if (rc) return rc;
  }
  const long long blocks = (samples + SP_THREADS - 1) / SP_THREADS;
  hipLaunchKernelGGL(spectral_grad_gather_kernel, dim3((unsigned)blocks, (unsigned)rows),
                     dim3(SP_THREADS), 0, st, ws, gs, ref_rows, samples, lengths, grad_est);
  return vrvq_launch_status();
}

extern "C" int vrvq_spectral_distance_workspace(int rows, long long samples, int n_scales,
                                                const int* windows, long long* bytes) {
  VRVQ_CHECK_ARG(bytes);
  SpScales sc;
  long long doubles = 0;
  const int rc = plan(rows, samples, n_scales, windows, nullptr, &sc, &doubles);
  if (rc) return rc;
  *bytes = doubles * (long long)sizeof(double);
  return VRVQ_OK;
}

extern "C" int vrvq_spectral_distance(const float* est, const float* ref, int rows, int ref_rows,
                                      long long samples, const long long* lengths, int n_scales,
                                      const int* windows, const int* n_mels,
                                      const float* const* tables, const int* const* bands,
                                      const float* const* band_weights, double clamp_eps,
                                      double pow, double log_weight, double mag_weight,
                                      double* terms, double* distance, void* workspace,
                                      long long workspace_bytes, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(est && ref && terms && workspace && windows && n_mels && tables);
  VRVQ_CHECK_ARG(ref_rows > 0 && rows % ref_rows == 0 && clamp_eps > 0.0);
  SpScales sc;
  long long doubles = 0;
  int rc = plan(rows, samples, n_scales, windows, n_mels, &sc, &doubles);
  if (rc) return rc;
  for (int s = 0; s < n_scales; ++s) {
    VRVQ_CHECK_ARG(tables[s] && (reinterpret_cast<uintptr_t>(tables[s]) & 7) == 0);
    if (n_mels[s] > 0)
      VRVQ_CHECK_ARG(bands && band_weights && bands[s] && band_weights[s]);
    // without lengths every row has `samples` samples: too short for this window
    if (!lengths) VRVQ_CHECK_ARG(samples > windows[s] / 2);
  }
  VRVQ_CHECK_ARG(workspace_bytes >= doubles * (long long)sizeof(double));
  VRVQ_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  double* ws = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  for (int s = 0; s < n_scales; ++s) {
    const dim3 grid((unsigned)sc.tiles[s], (unsigned)rows);
    const int nm = n_mels[s];
    const int* bd = nm > 0 ? bands[s] : nullptr;
    const float* bw = nm > 0 ? band_weights[s] : nullptr;
    double* w = ws + sc.ws_off[s];
#define SP_CASE(WW)                                                                            \
  case WW:                                                                                     \
    launch_tile<WW>(grid, st, est, ref, ref_rows, samples, lengths, tables[s], nm, bd, bw,     \
                    clamp_eps, pow, w);                                                        \
    break;
    switch (windows[s]) {
      SP_CASE(32)
      SP_CASE(64)
      SP_CASE(128)
      SP_CASE(256)
      SP_CASE(512)
      SP_CASE(1024)
      SP_CASE(2048)
      default:
        return VRVQ_ERR_ARG;
    }
#undef SP_CASE
    rc = vrvq_launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(spectral_finish_kernel, dim3((unsigned)rows), dim3(64), 0, st, ws, sc,
                     ref_rows, samples, lengths, log_weight, mag_weight, terms, distance);
  return vrvq_launch_status();
}
