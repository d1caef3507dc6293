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
#include "common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_POINTS = 2048;  // complex points of a batch: G frames x 2 signals x W / 2
constexpr int SP_BATCHES = 4;    // batches per tile
constexpr int SP_MAX_SCALES = 16;
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
  {
    // sample f0 * HOP - W / 2 + i of both rows, reflected at 0 and at n without repeating the
    // edge; positions past the row's last frame are clamped (their frames are not counted)
    const float* __restrict__ e = est + (size_t)row * samples;
    const float* __restrict__ r = ref + (size_t)rrow * samples;
    const long long base = f0 * HOP - N;
    for (int i = tid; i < SPAN; i += SP_THREADS) {
      long long idx = base + i;
      if (idx < 0) idx = -idx;
      if (idx >= n) idx = 2 * (n - 1) - idx;
      idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
      span[0][i] = e[idx];
      span[1][i] = r[idx];
    }
  }
  __syncthreads();

  const int n_items = n_mels > 0 ? n_mels : NB;
  double acc_log = 0.0, acc_mag = 0.0;
  for (int fb = 0; fb < SP_BATCHES; ++fb) {
    const int gv = valid - fb * G < G ? valid - fb * G : G;  // frames of this batch that count
    if (gv <= 0) break;                                      // uniform

    // first pass (n = N, s = 1): windowed (even, odd) sample pairs straight from the span
#pragma unroll
    for (int i = 0; i < SLOTS * Q / SP_THREADS; ++i) {
      const int b = tid + i * SP_THREADS, slot = b / Q, t = b % Q;
      const float* __restrict__ x = &span[slot & 1][(fb * G + (slot >> 1)) * HOP];
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
    int cur = 0;
    int nn = N / 4, s = 4, ls = 2;
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

    // unpack the real transform's bins 0..N from Z = buf[cur] and take magnitudes:
    // 2 X[k] = (Z[k] + conj Z[N-k]) - i w_k (Z[k] - conj Z[N-k]), w_k = exp(-2 pi i k / W)
    float* __restrict__ mags = reinterpret_cast<float*>(buf[cur ^ 1]);
    {
      const float2* __restrict__ zb = buf[cur];
      for (int i = tid; i < SLOTS * NB; i += SP_THREADS) {
        const int slot = i / NB, k = i % NB;
        const float2 zk = zb[slot * N + (k & (N - 1))];
        float2 zc = zb[slot * N + ((N - k) & (N - 1))];
        zc.y = -zc.y;
        const float2 a = cadd(zk, zc), wb = cmul(csub(zk, zc), tw[k]);
        const float xr = a.x + wb.y, xi = a.y - wb.x;
        mags[i] = 0.5f * sqrtf(fmaf(xr, xr, xi * xi));
      }
    }
    __syncthreads();

    // projection and the two differences; item = frame * n_items + element
    for (int item = tid; item < gv * n_items; item += SP_THREADS) {
      const int g = item / n_items, m = item - g * n_items;
      const float* __restrict__ me = mags + (2 * g) * NB;
      const float* __restrict__ mr = me + NB;
      float E, R;
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

}  // namespace

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
