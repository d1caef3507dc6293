// Snake-fused 1-D convolution and polyphase transposed convolution for gfx950.
//
// Implicit GEMM:  Y[M x N] = W[M x K] * Xs[K x N]
//   M = output channels (or phase-channels for the transposed conv), N = output time,
//   K = Cin * taps, Xs = im2col(snake(x)) never materialised: each workgroup stages a
//   [CK channels x (BN*stride + halo)] window of snake(x) in LDS once per K-chunk and the
//   B-operand of every tap is read from that window at offset (j*stride + tap*dil).
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fmaf chain, 64 cyc/SIMD issue).
//   A (32x2):  lane l holds W[m = l&31][k = l>>5]
//   B (2x32):  lane l holds Xs[k = l>>5][n = l&31]
//   D (32x32): lane l, reg r holds Y[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31]
// So each store instruction writes 32 consecutive time steps (128 B) per row.
//
// Reference semantics: models/layers.py:17-41 (WNConv1d, WNConvTranspose1d, snake),
// :52-110 (ResidualUnit skip, EncoderBlock, DecoderBlock), models/dac_vrvq.py:19-80,
// models/importance_subnet.py:38-45.
#include "common.h"
#include "conv_core.h"
#include "conv_x3.h"
#include <atomic>

namespace {

using namespace vrvq_conv;

template <int BM, int BN, int WM, int NW, int KS, bool X3, bool PH = false,
          bool PAIR = x3_pair<KS, BM, BN>(), bool SPLIT = false>
__global__ __launch_bounds__(64 * NW)
__attribute__((amdgpu_waves_per_eu(X3 && x3_stages<BM, BN>() == 1 ? 2 : 1)))
void conv_mfma_kernel(ConvArgs a) {
  using TC = TileCfg<BM, BN, WM, NW>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int bid = blockIdx.x;
  int ks = 0;  // split-K part (SPLIT: the a.ks_split K parts of a tile are adjacent workgroups)
  if (SPLIT) {
    ks = bid % a.ks_split;
    bid /= a.ks_split;
  }
  // M tile fastest (an M-tile-slowest order, all CUs on one weight tile for L2 reuse, measured
  // no faster in r02: the weight tiles are not what limits)
  const int mt = bid % a.n_mt;
  bid /= a.n_mt;
  const int nt = bid % a.n_nt;
  const int b = bid / a.n_nt;
  const int m0 = mt * BM;
  const int n0 = nt * BN;
  f32x16 acc[TC::RM][TC::RN];
#pragma unroll
  for (int i = 0; i < TC::RM; ++i)
#pragma unroll
    for (int j = 0; j < TC::RN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  // The 64 x 256 pair k7 tile prefetches the next chunk's x window into registers during the
  // MFMAs (conv_x3.h XPF; profiles/r06x_xpf_layers.txt: 1-3.5 % per layer).
  constexpr bool XPF = X3 && KS == 7 && PAIR && !SPLIT;
  // single-buffered operand reads (conv_x3.h) on the k1 and 128-wide 2-tap tiles: 2-6 % per
  // k1 layer, +1.7 % end to end with the ResidualUnit rule (profiles/r04q_sb_ab.txt)
#ifdef VRVQ_X3_SB_ALL  // A/B build
  constexpr bool SB = true;
#else
  // (XPF: the x prefetch registers take the place of the second operand set)
  constexpr bool SB = KS == 1 || (KS == 2 && BN == 128) || XPF;
#endif
  if constexpr (X3) {
    if constexpr (SPLIT) {
      // split-K: this part's chunks, the raw sums to ks_part in fragment order (the tile's
      // 64 NW threads x RM RN 16 floats, lane-contiguous: 256-B stores), no epilogue here
      constexpr int CK = X3Cfg<KS, PAIR>::CK;
      const int nch = (a.cin + CK - 1) / CK, per = (nch + a.ks_split - 1) / a.ks_split;
      if (ks * per < nch)  // (an empty part would store zero sums; splitk_parts makes none)
        conv_mainloop_x3<BM, BN, WM, NW, KS, PH, PAIR, SB>(a, smem, acc, b, m0, n0, ks * per,
                                                            min(nch, (ks + 1) * per));
      constexpr int NR = TC::RM * TC::RN * 16;
      const size_t tile = ((size_t)b * a.n_nt + nt) * a.n_mt + mt;
      const size_t ntile = (size_t)gridDim.x / a.ks_split;
      float* dst = a.ks_part + ((size_t)ks * ntile + tile) * (size_t)NR * 64 * NW +
                   (threadIdx.x >> 6) * NR * 64 + (threadIdx.x & 63);
#pragma unroll
      for (int i = 0; i < TC::RM; ++i)
#pragma unroll
        for (int j = 0; j < TC::RN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((i * TC::RN + j) * 16 + r) * 64] = acc[i][j][r];
      return;
    }
    conv_mainloop_x3<BM, BN, WM, NW, KS, PH, PAIR, SB, XPF>(a, smem, acc, b, m0, n0);
  } else {
    conv_mainloop<BM, BN, WM, NW, KS>(a, smem, acc, b, m0, n0);
  }
  conv_epilogue<BM, BN, WM, NW>(a, smem, acc, b, m0, n0);
}

// Split-K epilogue: one workgroup per tile (the block order of conv_mfma_kernel without its K
// parts) adds the a.ks_split partial accumulators in part order -- a fixed order that depends on
// the layer only, not on the batch -- and runs the tile's epilogue (bias, residual, activation,
// next Snake) exactly as the unsplit kernel does.
template <int BM, int BN, int WM, int NW>
__global__ __launch_bounds__(64 * NW) void conv_splitk_epilogue_kernel(ConvArgs a) {
  using TC = TileCfg<BM, BN, WM, NW>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int bid = blockIdx.x;
  const int mt = bid % a.n_mt;
  bid /= a.n_mt;
  const int nt = bid % a.n_nt;
  const int b = bid / a.n_nt;
  constexpr int NR = TC::RM * TC::RN * 16;
  const size_t tile = blockIdx.x;  // ((b n_nt + nt) n_mt + mt): the split kernel's order
  const size_t pstride = (size_t)gridDim.x * NR * 64 * NW;
  const float* src = a.ks_part + tile * (size_t)NR * 64 * NW + (threadIdx.x >> 6) * NR * 64 +
                     (threadIdx.x & 63);
  f32x16 acc[TC::RM][TC::RN];
#pragma unroll
  for (int i = 0; i < TC::RM; ++i)
#pragma unroll
    for (int j = 0; j < TC::RN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = src[((i * TC::RN + j) * 16 + r) * 64];
  for (int s = 1; s < a.ks_split; ++s)
#pragma unroll
    for (int i = 0; i < TC::RM; ++i)
#pragma unroll
      for (int j = 0; j < TC::RN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc[i][j][r] = acc[i][j][r] + src[s * pstride + ((i * TC::RN + j) * 16 + r) * 64];
  conv_epilogue<BM, BN, WM, NW>(a, smem, acc, b, mt * BM, nt * BN);
}

// Small-Cout conv (Cout <= 8, stride 1): the decoder's 96->1 k7 + Tanh output layer and the
// importance subnet's 32->8 / 8->1 k3 tail. An MFMA tile would be >= 75 % padding and the layer
// is HBM-bound on reading x, so: one thread per output sample, snake(x) rows of SC channels
// staged in LDS per step (window 256 + (k-1)*dil), every output channel accumulated in VGPRs.
constexpr int SMALL_BT = 256;
constexpr int SMALL_SC = 16;
constexpr int SMALL_COUT = 8;
constexpr int SMALL_WMAX = 2048;  // cin * k * cout weights staged in LDS

template <int COUT>
__global__ __launch_bounds__(256) void conv_small_cout_kernel(ConvArgs a, int ks) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* w_s = sm;                      // [cin][k][COUT]
  float* xs = sm + SMALL_WMAX;          // [SMALL_SC][XW]
  const int XW = SMALL_BT + (ks - 1) * a.dil;
  const int n_t = (a.ng + SMALL_BT - 1) / SMALL_BT;
  const int b = blockIdx.x / n_t;
  const int t0 = (blockIdx.x - b * n_t) * SMALL_BT;
  const int tid = threadIdx.x;
  const float* xb = a.x + (size_t)b * a.cin * a.tin;
  for (int e = tid; e < a.cin * ks * COUT; e += 256) {
    const int c = e % COUT, rk = e / COUT;
    w_s[e] = a.w[(size_t)rk * a.m_pad + c];
  }
  float acc[COUT];
#pragma unroll
  for (int c = 0; c < COUT; ++c) acc[c] = 0.0f;

  // staged positions: the window of this block's output positions only (short rows: T = 87)
  const int pmax = min(XW, a.ng - t0 + (ks - 1) * a.dil);
  for (int ci0 = 0; ci0 < a.cin; ci0 += SMALL_SC) {
    const int nc = min(SMALL_SC, a.cin - ci0);
    const int total = nc * pmax;
    // eight loads in flight per thread from clamped addresses, then the zeroing / Snake / LDS
    // stores (a load under the range branch made every iteration wait for its own load)
    for (int e0 = tid; e0 < total; e0 += 8 * 256) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = min(e0 + u * 256, total - 1);
        const int cl = e / pmax, p = e - cl * pmax;
        const int tc = min(max(t0 - a.pad + p, 0), a.tin - 1);
        v[u] = xb[(size_t)(ci0 + cl) * a.tin + tc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * 256;
        if (e < total) {
          const int cl = e / pmax, p = e - cl * pmax;
          const int ci = ci0 + cl;
          const int t = t0 - a.pad + p;
          float x = 0.0f;
          if (t >= 0 && t < a.tin) {
            x = v[u];
            if (a.alpha) x = snake_act(x, a.alpha[ci], a.inv_alpha[ci]);
          }
          xs[cl * XW + p] = x;
        }
      }
    }
    __syncthreads();
    for (int cl = 0; cl < nc; ++cl) {
      const float* wr = w_s + (size_t)(ci0 + cl) * ks * COUT;
      const float* xr = xs + cl * XW + tid;
      for (int k = 0; k < ks; ++k) {
        const float xv = xr[k * a.dil];
#pragma unroll
        for (int c = 0; c < COUT; ++c) acc[c] = fmaf(wr[k * COUT + c], xv, acc[c]);
      }
    }
    __syncthreads();
  }
  const int t = t0 + tid;
  if (t < a.ng) {
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
      if (c < a.M) {
        float v = acc[c];
        if (a.bias) v = v + a.bias[c];
        const size_t o = ((size_t)b * a.cout + c) * a.ylen + t;
        if (a.res) v = a.res[o] + v;
        v = apply_epi(v, a.epi);
        if (a.y) a.y[o] = v;
        if (a.ys) a.ys[o] = snake_act(v, a.alpha_o[c], a.inv_alpha_o[c]);
      }
    }
  }
}

// Cout = 1 as a stream (the decoder's 96->1 k7 + Tanh, HBM-bound on reading x): no LDS, no
// barriers; each thread owns 4 consecutive outputs and per input channel reads the 12-sample
// window t0-4 .. t0+7 as three 16-B loads (covers pad <= 4 and k-1-pad <= 4 at dilation 1),
// channels unrolled by 8 so their loads are in flight together (measured at B = 32, 96 -> 1 k7:
// 364 us for the LDS-staged kernel, 277 us at 8 outputs x 4 channels per thread, 235 us at
// 4 x 8, 163 us (3.4 TB/s) with the window / Snake branches hoisted out of the channel loop). Accumulation order per output:
// channel, then tap -- conv_small_cout_kernel's fmaf chain, so the two agree bit for bit.
constexpr int C1_T = 4;
constexpr int C1_W = 12;  // window samples per channel
template <int KS, int PAD, bool SNK>
__global__ __launch_bounds__(256) void conv_cout1_stream_kernel(ConvArgs a) {
  static_assert(PAD <= 4 && 4 - PAD + KS - 1 + C1_T - 1 < C1_W, "window t0-4 .. t0+7");
  constexpr int SH = 4 - PAD;  // window index of tap 0 for output t0
  const int n_t = (a.ng + 256 * C1_T - 1) / (256 * C1_T);
  const int b = blockIdx.x / n_t;
  const int t0 = ((blockIdx.x - b * n_t) * 256 + (int)threadIdx.x) * C1_T;
  if (t0 >= a.ng) return;  // no barrier in this kernel
  const float* xb = a.x + (size_t)b * a.cin * a.tin;
  const bool interior = t0 - 4 >= 0 && t0 - 4 + C1_W <= a.tin;
  float acc[C1_T];
#pragma unroll
  for (int u = 0; u < C1_T; ++u) acc[u] = 0.0f;
  // the window path and the Snake flag are decided once, outside the channel loop: a branch
  // per channel would drain each channel's loads before the next are issued
  auto run = [&](auto interior_c, auto snake_c) {
    constexpr bool INTERIOR = decltype(interior_c)::value, SNAKE = decltype(snake_c)::value;
    auto load_win = [&](int c, float (&xv)[C1_W]) {
      const float* xr = xb + (size_t)c * a.tin + t0 - 4;
      if constexpr (INTERIOR) {
#pragma unroll
        for (int q = 0; q < C1_W / 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(xr + 4 * q);
          xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < C1_W; ++j) {
          const int t = t0 - 4 + j;
          const float v = xb[(size_t)c * a.tin + min(max(t, 0), a.tin - 1)];
          xv[j] = __uint_as_float(__float_as_uint(v) & (0u - (unsigned)(t >= 0 && t < a.tin)));
        }
      }
    };
    auto accum = [&](int c, float (&xv)[C1_W]) {
      if constexpr (SNAKE) snake_n1<C1_W>(xv, a.alpha[c], a.inv_alpha[c]);  // snake(0) = 0
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const float wv = a.w[(size_t)(c * KS + k) * a.m_pad];
#pragma unroll
        for (int u = 0; u < C1_T; ++u) acc[u] = fmaf(wv, xv[SH + k + u], acc[u]);
      }
    };
    constexpr int CU = 8;
    int c = 0;
    for (; c + CU <= a.cin; c += CU) {
      float xv[CU][C1_W];
#pragma unroll
      for (int i = 0; i < CU; ++i) load_win(c + i, xv[i]);
#pragma unroll
      for (int i = 0; i < CU; ++i) accum(c + i, xv[i]);
    }
    for (; c < a.cin; ++c) {
      float xv[C1_W];
      load_win(c, xv);
      accum(c, xv);
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  if (interior) {
    run(T_{}, std::integral_constant<bool, SNK>{});
  } else {
    run(F_{}, std::integral_constant<bool, SNK>{});
  }
#pragma unroll
  for (int u = 0; u < C1_T; ++u) {
    const int t = t0 + u;
    if (t < a.ng) {
      float v = acc[u];
      if (a.bias) v = v + a.bias[0];
      const size_t o = (size_t)b * a.ylen + t;
      if (a.res) v = a.res[o] + v;
      v = apply_epi(v, a.epi);
      if (a.y) a.y[o] = v;
      if (a.ys) a.ys[o] = snake_act(v, a.alpha_o[0], a.inv_alpha_o[0]);
    }
  }
}

// Cin = 1 conv (the encoder's 1 -> 64 k7 input conv, models/dac_vrvq.py:27): no MFMA tile
// (K = 7), HBM-bound on writing y and snake(y) (2 x 64 x 4 B per sample). Thread = 4
// consecutive output samples x CI1_CG channels; its 4 + KS - 1 input samples once, per channel
// the k-ordered fmaf chain from 0, then conv_epilogue's expressions (bias, residual, act, the
// next layer's Snake) and one 16-B store per output row: a wave writes 1 KB runs per channel.
constexpr int CI1_T = 4;
constexpr int CI1_CG = 16;
template <int KS>
__global__ __launch_bounds__(256) void conv_cin1_stream_kernel(ConvArgs a) {
  const int n_t = (a.ng + 256 * CI1_T - 1) / (256 * CI1_T);
  const int n_cg = a.M / CI1_CG;
  int blk = blockIdx.x;
  const int cg = blk % n_cg;
  blk /= n_cg;
  const int tt = blk % n_t, b = blk / n_t;
  const int t0 = (tt * 256 + (int)threadIdx.x) * CI1_T;
  if (t0 >= a.ng) return;  // no barrier in this kernel
  const float* xb = a.x + (size_t)b * a.tin;
  constexpr int W = CI1_T + KS - 1;
  float xv[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {  // clamped address, zeroed outside [0, tin) (zero padding)
    const int t = t0 - a.pad + j;
    const float v = xb[min(max(t, 0), a.tin - 1)];
    xv[j] = __uint_as_float(__float_as_uint(v) & (0u - (unsigned)(t >= 0 && t < a.tin)));
  }
  const bool full = t0 + CI1_T <= a.ng;
#pragma unroll 4
  for (int c = 0; c < CI1_CG; ++c) {
    const int co = cg * CI1_CG + c;
    float v[CI1_T];
#pragma unroll
    for (int u = 0; u < CI1_T; ++u) v[u] = 0.0f;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const float wv = a.w[(size_t)k * a.m_pad + co];
#pragma unroll
      for (int u = 0; u < CI1_T; ++u) v[u] = fmaf(wv, xv[k + u], v[u]);
    }
    const float bb = a.bias ? a.bias[co] : 0.0f;
    const size_t o = ((size_t)b * a.cout + co) * a.ylen + t0;
#pragma unroll
    for (int u = 0; u < CI1_T; ++u) v[u] = v[u] + bb;
    if (a.res) {
#pragma unroll
      for (int u = 0; u < CI1_T; ++u)
        if (full || t0 + u < a.ng) v[u] = a.res[o + u] + v[u];
    }
#pragma unroll
    for (int u = 0; u < CI1_T; ++u) v[u] = apply_epi(v[u], a.epi);
    if (a.y) {
      if (full) *reinterpret_cast<float4*>(a.y + o) = make_float4(v[0], v[1], v[2], v[3]);
      else
        for (int u = 0; u < CI1_T; ++u)
          if (t0 + u < a.ng) a.y[o + u] = v[u];
    }
    if (a.ys) {
      snake_n1<CI1_T>(v, a.alpha_o[co], a.inv_alpha_o[co]);
      if (full) *reinterpret_cast<float4*>(a.ys + o) = make_float4(v[0], v[1], v[2], v[3]);
      else
        for (int u = 0; u < CI1_T; ++u)
          if (t0 + u < a.ng) a.ys[o + u] = v[u];
    }
  }
}

// What runs for a conv shape. The functions below decide it and launch it in one pass; called
// with a ConvPlan* they stop once the plan is known, before hipFuncSetAttribute and the launch
// (vrvq_conv_plan: the same code and the same status, no device touched).
enum ConvPath { PATH_MFMA = 0, PATH_SMALL_COUT = 1, PATH_CIN1 = 2 };
struct ConvPlan {
  int path;        // ConvPath
  int BM, BN, WM;  // MFMA tile and its wave rows (0 off the MFMA tiles)
  int KS;          // the GEMM's taps (2: the phase-split view, the polyphase ConvTranspose)
  int x3;          // 0 fp32-input loop | 1 x3 on plain K chunks | 2 x3 on pair chunks
  int S;           // split-K parts (0: unsplit)
};

// Tile and path of the last MFMA conv launch (vrvq_conv_last_launch, a host-side debug query:
// the tests assert the path they claim to pin). One word, so concurrent callers never read a
// torn record: BM (9 bits) | BN << 9 (9) | KS << 18 (5) | x3 << 23 (2) | S << 25 (7).
std::atomic<unsigned> g_last_launch{0};

void note_launch(const ConvPlan& p) {
  g_last_launch.store((unsigned)p.BM | (unsigned)p.BN << 9 | (unsigned)p.KS << 18 |
                      (unsigned)p.x3 << 23 | (unsigned)(p.S & 127) << 25,
                      std::memory_order_relaxed);
}

// The exit of every MFMA decision: a plan-only call (plan != null, its launches were dry) hands
// the plan back, a launch records it.
int finish(int rc, const ConvPlan& p, ConvPlan* plan) {
  if (rc == 0) {
    if (plan) *plan = p;
    else note_launch(p);
  }
  return rc;
}

// One conv kernel: its dynamic-LDS limit raised where it needs more than 64 KiB, then the
// launch. dry (a plan-only call): neither.
int launch_kernel(void (*kernel)(ConvArgs), long long nblk, int threads, size_t lds,
                  hipStream_t st, const ConvArgs& a, bool dry) {
  if (dry) return 0;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  ConvArgs arg = a;
  void* params[] = {&arg};
  hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3((unsigned)nblk),
                                 dim3(threads), params, lds, st);
  return e != hipSuccess ? (int)e : vrvq_launch_status();
}

int launch_small(const ConvArgs& a, int batch, int ks, hipStream_t st, ConvPlan* plan) {
  const ConvPlan p{PATH_SMALL_COUT, 0, 0, 0, ks, 0, 0};
  if (a.M == 1 && a.cout == 1 && a.stride == 1 && a.dil == 1 && a.tin % 4 == 0 &&
      ((ks == 7 && a.pad == 3) || (ks == 3 && a.pad == 1))) {
    const long long nblk = (long long)batch * ((a.ng + 256 * C1_T - 1) / (256 * C1_T));
    if (nblk <= 0 || nblk > 0x7fffffffLL) return VRVQ_ERR_ARG;
    if (plan) *plan = p;
    // the consumer-side Snake variant is its own kernel: its registers do not set the plain
    // variant's occupancy
    void (*kernel)(ConvArgs) =
        ks == 7 ? (a.alpha ? conv_cout1_stream_kernel<7, 3, true> : conv_cout1_stream_kernel<7, 3, false>)
                : (a.alpha ? conv_cout1_stream_kernel<3, 1, true> : conv_cout1_stream_kernel<3, 1, false>);
    return launch_kernel(kernel, nblk, 256, 0, st, a, plan != nullptr);
  }
  if (a.cin * ks * (a.M == 1 ? 1 : SMALL_COUT) > SMALL_WMAX) return VRVQ_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(SMALL_WMAX + SMALL_SC * (SMALL_BT + (ks - 1) * a.dil)) * sizeof(float);
  if (lds > 64 * 1024) return VRVQ_ERR_UNSUPPORTED;
  const long long nblk = (long long)batch * ((a.ng + SMALL_BT - 1) / SMALL_BT);
  if (nblk <= 0 || nblk > 0x7fffffffLL) return VRVQ_ERR_ARG;
  if (plan) {
    *plan = p;
    return 0;
  }
  if (a.M == 1)
    hipLaunchKernelGGL(conv_small_cout_kernel<1>, dim3((unsigned)nblk), dim3(256), lds, st, a, ks);
  else
    hipLaunchKernelGGL(conv_small_cout_kernel<SMALL_COUT>, dim3((unsigned)nblk), dim3(256), lds, st, a, ks);
  return vrvq_launch_status();
}

// The x3 launch of a tile (PAIR: its K-chunk form); VRVQ_ERR_UNSUPPORTED when its LDS does not
// fit (the caller then takes the fp32-input loop).
template <int BM, int BN, int WM, int NW, int KS, bool PAIR, bool SPLIT = false>
int launch_x3(const ConvArgs& a, int XW, size_t epi, long long nblk, hipStream_t st, bool dry) {
  // the pair tiles' Snake table only when the staging applies a Snake (the producer-side
  // snake(x) inputs of the k7 layers need none: 3-6 KB of LDS back)
  size_t lx = x3_lds_bytes<KS, BM, BN, PAIR>(XW, a.alpha ? (a.psh ? a.cin >> a.psh : a.cin) : 0);
  if (lx < epi) lx = epi;
  if (lx > 160 * 1024) return VRVQ_ERR_UNSUPPORTED;
  // A strided conv through the phase-split view: dispatch_tiles gives it a 2-tap pair tile (32-
  // or 128-wide, on plain chunks where the view's Cin is no multiple of 32) or the split-K tile,
  // which takes nothing else among the 2-tap GEMMs.
  constexpr bool PH_TILE = KS == 2 && (x3_pair<KS, BM, BN>() || SPLIT);
  if constexpr (PH_TILE) {
    if (a.psh)
      return launch_kernel(conv_mfma_kernel<BM, BN, WM, NW, KS, true, true, PAIR, SPLIT>, nblk,
                           64 * NW, lx, st, a, dry);
  }
  if constexpr (SPLIT && KS == 2) {
    return VRVQ_ERR_ARG;  // (splitk_parts: the only 2-tap GEMM that splits is the view's)
  } else {
    if (a.psh) return VRVQ_ERR_ARG;
    return launch_kernel(conv_mfma_kernel<BM, BN, WM, NW, KS, true, false, PAIR, SPLIT>, nblk,
                         64 * NW, lx, st, a, dry);
  }
}

template <int BM, int BN, int WM, int NW, int KS>
int launch_cfg(const ConvArgs& a0, int batch, hipStream_t st, ConvPlan* plan) {
  ConvArgs a = a0;
  a.n_mt = (a.M + BM - 1) / BM;
  a.n_nt = (a.ng + BN - 1) / BN;
  if (a.m_pad < a.n_mt * BM) return VRVQ_ERR_ARG;
  // transposed conv: a tile must hold whole output channels (rows co*up .. co*up + up-1), the
  // epilogue maps rows back with co0 = m0 / up
  if (a.up > 0 && BM % a.up != 0) return VRVQ_ERR_UNSUPPORTED;
  constexpr int CK = ChunkCfg<KS, BM, BN>::CK;
  const int XW = (BN - 1) * a.stride + (KS - 1) * a.dil + 1;
  const int XP = a.ssh ? (XW + a.stride - 1) >> a.ssh : XW;
  const int XWP = a.ssh ? ((XP << a.ssh) + 3) & ~3 : (XW + 3) & ~3;
  size_t epi = (size_t)BM * EpiCfg<BM, BN, NW / WM>::BNP * sizeof(float);
  if (a.pj_part) {  // RVQ in_proj epilogue: one latent split per tile, its z planes in LDS
    if (BM != 128) return VRVQ_ERR_UNSUPPORTED;
    if (epi < (size_t)PJE_LDS) epi = PJE_LDS;
  }
  const long long nblk = (long long)a.n_mt * a.n_nt * batch;
  if (nblk <= 0 || nblk > 0x7fffffffLL) return VRVQ_ERR_ARG;
  ConvPlan p{PATH_MFMA, BM, BN, WM, KS, 0, 0};
  const bool dry = plan != nullptr;
  // bf16x3 split path (conv_x3.h): stride-1 windows, a pre-split weight, the stage in LDS
  if constexpr (NW == 4 && BM <= 192 && (KS == 1 || KS == 2 || KS == 3 || KS == 7)) {
    constexpr int XW_MAX = (BN - 1) + (KS - 1) * (KS == 7 ? 9 : 1) + 1;
    if (a.w3 != nullptr && a.stride == 1 && a.ssh == 0 && XW <= XW_MAX) {
      // pair tiles (conv_x3.h) need whole K-chunks: other Cin run the tile on plain chunks
      int rc;
      if (x3_pair<KS, BM, BN>() && a.cin % X3Cfg<KS, true>::CK == 0) {
        p.x3 = 2;
        rc = launch_x3<BM, BN, WM, NW, KS, x3_pair<KS, BM, BN>()>(a, XW, epi, nblk, st, dry);
      } else {
        p.x3 = 1;
        rc = launch_x3<BM, BN, WM, NW, KS, false>(a, XW, epi, nblk, st, dry);
      }
      if (rc != VRVQ_ERR_UNSUPPORTED) return finish(rc, p, plan);
      p.x3 = 0;  // the stage does not fit in LDS: the fp32-input loop
    }
  }
  if (a.psh) return VRVQ_ERR_UNSUPPORTED;  // the phase-split view exists on the x3 loop only
  if (XW > 64 * WinCfg<KS, BN>::PER_ROW) return VRVQ_ERR_UNSUPPORTED;  // window > staged lanes
  size_t lds = 2 * (size_t)(CK * KS * BM + CK * XWP) * sizeof(float);
  if (lds < epi) lds = epi;  // epilogue tile
  if (lds > 160 * 1024) return VRVQ_ERR_UNSUPPORTED;
  return finish(launch_kernel(conv_mfma_kernel<BM, BN, WM, NW, KS, false>, nblk, 64 * NW, lds, st,
                              a, dry), p, plan);
}

// Split-K for the deep-K, narrow-N layers at T <= 96 (the encoder's 512 -> 1024 s8 conv, the
// importance subnet's k3 convs, the decoder's 1024 -> 1536 k7 at T = 87): their 32-wide tiles
// re-streamed every M tile's whole weight block per 32 columns (50 MB of planes x 87 column
// tiles for the s8 conv), and one 96-wide tile per clip gives too few workgroups to hide a
// 128-chunk serial K loop. Here: 128 x 96 tiles (one per clip: the weight block read once per
// clip) with the channel chunks cut into SPLITK_PARTS parts of at least SPLITK_MIN_CHUNKS
// chunks -- a function of the layer only, so a clip's sums do not change with the batch. Per
// layer at B = 32 (profiles/r06ks_splitk_sweep.txt, S = none / 2 / 3 / 4 / 6 / 8): 512 -> 1024 s8
// 645 / 441 / 469 / 445 / 462 / 455 us, 1024 -> 1024 k3 182 / 140 / 169 / 143 / 155 / 159,
// 1024 -> 512 k3 124 / 95 / 91 / 79 / 94 / 85, 512 -> 128 k3 48 -> 38 (S <= 4: 32 chunks),
// 1024 -> 1536 k7 518 / 525 / 530 / 467 / 496 / 479: S = 4 is within 1 % of the best everywhere.
constexpr int SPLITK_PARTS = 4;
constexpr int SPLITK_MIN_CHUNKS = 8;

// K parts of a layer (0: none). ks = the GEMM's taps (2 for the phase-split view), cin = the
// GEMM's channels (the view's for a strided conv). The same for vrvq_conv1d_proj (the encoder's
// last conv, whose shape the ImportanceSubnet's first conv shares): its projection epilogue then
// runs in the split-K epilogue launch, on the same z bits as the plain conv's.
int splitk_parts(int M, int cin, int ng, int ks, bool psh, bool up, bool x3) {
  if (!x3 || up || ng > 96 || M % 128 != 0) return 0;
  if (!(ks == 3 || ks == 7 || (ks == 2 && psh))) return 0;
  const int ck = ks == 2 ? X3Cfg<2, true>::CK : ks == 3 ? X3Cfg<3>::CK : X3Cfg<7>::CK;
  if (ks == 2 && cin % ck != 0) return 0;
  const int nch = (cin + ck - 1) / ck;
  const int S = nch / SPLITK_MIN_CHUNKS < SPLITK_PARTS ? nch / SPLITK_MIN_CHUNKS : SPLITK_PARTS;
  return S >= 2 ? S : 0;
}

size_t splitk_bytes(int S, int M, int ng, int batch) {
  return S ? (size_t)S * batch * (M / 128) * ((ng + 95) / 96) * 128 * 96 * sizeof(float) : 0;
}

template <int KS>
int launch_splitk(const ConvArgs& a0, int batch, int S, hipStream_t st, ConvPlan* plan) {
  if constexpr (KS == 2 || KS == 3 || KS == 7) {
    ConvArgs a = a0;
    a.ks_split = S;
    a.n_mt = a.M / 128;
    a.n_nt = (a.ng + 95) / 96;
    if (a.m_pad < a.n_mt * 128) return VRVQ_ERR_ARG;
    const int XW = 95 + (KS - 1) * a.dil + 1;
    constexpr int XW_MAX = 95 + (KS - 1) * (KS == 7 ? 9 : 1) + 1;
    if (XW > XW_MAX) return VRVQ_ERR_UNSUPPORTED;
    size_t epi = (size_t)128 * EpiCfg<128, 96, 1>::BNP * sizeof(float);
    if (a.pj_part && epi < (size_t)PJE_LDS) epi = PJE_LDS;
    const long long tiles = (long long)a.n_mt * a.n_nt * batch;
    if (tiles * S > 0x7fffffffLL) return VRVQ_ERR_ARG;
    const ConvPlan p{PATH_MFMA, 128, 96, 4, KS, KS == 2 ? 2 : 1, S};
    const bool dry = plan != nullptr;
    int rc = launch_x3<128, 96, 4, 4, KS, KS == 2, true>(a, XW, epi, tiles * S, st, dry);
    if (rc == 0)
      rc = launch_kernel(conv_splitk_epilogue_kernel<128, 96, 4, 4>, tiles, 256, epi, st, a, dry);
    return finish(rc, p, plan);
  } else {
    (void)a0; (void)batch; (void)S; (void)st; (void)plan;
    return VRVQ_ERR_UNSUPPORTED;
  }
}

// ---- Tile choice (DESIGN.md "Conv tiles" has the same rules as a table) ----
// (a) Column width BN of the tile for ng GEMM columns.
//
// T <= 96 layers: one 96-wide tile per clip when that gives at least this many workgroups (1.5
// per CU), else three 32-wide tiles: each N tile re-streams its M tile's whole weight block, so
// the narrow tiles triple the weight traffic, but with fewer 96-wide ones the CUs run short of
// workgroups to hide each one's serial K loop (profiles/r02zl_x3_sq_counters.txt; the k3 / k7
// layers 96-wide at B = 32 no faster, profiles/r05zf_t87_tiles_ab.txt).
constexpr long long BN96_MIN_WORKGROUPS = 384;

template <int KS>
int tile_width(const ConvArgs& a, int batch) {
  const bool x3_2tap = KS == 2 && a.w3 != nullptr;
  if (a.ng <= 32) return 32;
  if (a.ng <= 96) {
    // 2-tap x3 GEMMs: the 32-wide tile pairs its K octets (conv_x3.h x3_pair) and the 96-wide
    // one does not, so a clip's sums would change order with the batch. Their width is fixed
    // per layer type instead (batch-invariant outputs, tests/test_gpu_parity.py
    // test_batch_invariance_*): the polyphase ConvTranspose 96-wide, the others (the phase-split
    // strided convs: 96-wide 691 -> 629 us for 512 -> 1024 s8, bench within the spread,
    // profiles/r05zf_t87_tiles_ab.txt) 32-wide.
    if (x3_2tap) return a.up > 0 ? 96 : 32;
    return (long long)((a.M + 127) / 128) * batch >= BN96_MIN_WORKGROUPS ? 96 : 32;
  }
  // Longer rows: 128-wide, or 64-wide below T = 4096 where that pads markedly fewer columns.
  // Not for k = 16 (the stride-8 encoder convs on the fp32-input loop): the 8 MB weight block
  // does not fit in L2, so the 128-wide tile's halved weight re-streaming beats its padding
  // (1490 -> 1323 us at T = 696, profiles/r02u_conv_ab.txt). Nor for the x3 strided convs and
  // ConvTransposes, whose 128-wide tile runs 32-channel pair chunks: 256 -> 512 s8 at T = 696
  // 940 -> 878 us, ConvT 768 -> 384 s8 1388 -> 1296 us (profiles/r04ze_ph128_ab.txt).
  auto waste = [&](int bn) { return ((a.ng + bn - 1) / bn) * bn - a.ng; };
  if (a.ng < 4096 && KS != 16 && waste(64) * 10 < waste(128) * 7 &&
      !(x3_2tap && (a.psh > 0 || a.up > 0)))
    return 64;
  return 128;
}

// x3 k7 layers from this many columns (M a multiple of 64 and >= 128, Cin a multiple of 16) run
// 64 x 256 tiles on 16-channel "pair" K-chunks (conv_x3.h: no zero octet, 168 MFMAs per wave
// between barriers). 384 x 384 k7 at T = 5568, B = 32: 2027 -> 755-796 us, 256 x 256: 934 ->
// 781-785 us; 768 x 768 / 512 x 512 k7 at T = 696: 1125 -> 962 / 514 -> 407 us despite 72 of
// every 768 columns padded (profiles/r03_x3_pair_ab.txt).
constexpr int K7_PAIR_MIN_COLUMNS = 640;

// A BM-row tile, 64 columns wide where tile_width chose that, else 128.
template <int BM, int WM, int KS>
int launch_bn(int bn, const ConvArgs& a, int batch, hipStream_t st, ConvPlan* plan) {
  if constexpr (KS != 16) {  // (tile_width: k = 16 never runs 64-wide)
    if (bn == 64) return launch_cfg<BM, 64, WM, 4, KS>(a, batch, st, plan);
  }
  return launch_cfg<BM, 128, WM, 4, KS>(a, batch, st, plan);
}

// (b) Row tile BM from the GEMM rows M; the first rule that applies.
template <int KS>
int dispatch_tiles(const ConvArgs& a, int batch, hipStream_t st, ConvPlan* plan) {
  if (a.ks_part != nullptr) {
    const int S = splitk_parts(a.M, a.cin, a.ng, KS, a.psh > 0, a.up > 0, a.w3 != nullptr);
    if (S > 0) {
      const int rc = launch_splitk<KS>(a, batch, S, st, plan);
      if (rc != VRVQ_ERR_UNSUPPORTED) return rc;
    }
  }
  const int bn = tile_width<KS>(a, batch);
  const bool x3 = a.w3 != nullptr;
  if constexpr (KS == 2) {
    // Polyphase ConvTranspose1d with a stride that does not divide 128 (3, 6): 192-row tiles,
    // which hold whole output channels, 64-wide up to T = 96 (other strides, 5, 7, ..., are
    // rejected by launch_cfg).
    if (a.up > 0 && 128 % a.up != 0) return launch_bn<192, 2, KS>(bn <= 96 ? 64 : bn, a, batch, st, plan);
  }
  if (a.M <= 32) return launch_cfg<32, 128, 1, 4, KS>(a, batch, st, plan);
  if constexpr (KS == 7) {
    if (x3 && a.M >= 128 && a.M % 64 == 0 && a.cin % 16 == 0 && a.ng >= K7_PAIR_MIN_COLUMNS)
      return launch_cfg<64, 256, 1, 4, KS>(a, batch, st, plan);
  }
  // T <= 96: 128 rows at the width chosen above
  if (bn == 32) return launch_cfg<128, 32, 4, 4, KS>(a, batch, st, plan);
  if (bn == 96) return launch_cfg<128, 96, 4, 4, KS>(a, batch, st, plan);
  if (a.M <= 64) return launch_bn<64, 2, KS>(bn, a, batch, st, plan);
  // 96- and 192-row tiles: no padded rows for the C = 96 / 192 decoder blocks
  if (a.M <= 96) return launch_cfg<96, 128, 1, 4, KS>(a, batch, st, plan);
  if constexpr (KS == 7) {
    // 768 x 768 k7 at T = 696: 2150 -> 1795 us with 192-row x 64-col tiles (K chunk 4 channels),
    // 427 -> 434 audio-sec/s end to end (profiles/r01j_conv_k7_ab.txt)
    if (a.M % 192 == 0 && bn == 64) return launch_cfg<192, 64, 2, 4, KS>(a, batch, st, plan);
  }
  if constexpr (KS == 2) {
    // Polyphase ConvTranspose1d, M = Cout * stride phase rows. fp32-input loop, M a multiple of
    // 192: 192-row tiles (ConvT 768 -> 384 s8 2443 -> 2345 us, 384 -> 192 s4 2887 -> 2660 us,
    // profiles/r01k_convt_ab.txt); with the x3 weights the 128-row tiles, two workgroups per CU,
    // are faster (638 -> 649 audio-sec/s at B = 32, profiles/r02zh_tile_ab.txt) ...
    if (a.up > 0 && !x3 && a.M % 192 == 0) return launch_bn<192, 2, KS>(bn, a, batch, st, plan);
    // ... except M a multiple of 96 and not of 128 (192 -> 96 s2: M = 192): 96-row tiles on the
    // pair chunks, two workgroups per CU, instead of the two-stage 192 x 128 tile (981-988 vs
    // 942-954 us, profiles/r06t_convt_layers.txt)
    if (a.up > 0 && x3 && a.M % 96 == 0 && a.M % 128 != 0)
      return launch_cfg<96, 128, 1, 4, KS>(a, batch, st, plan);
  }
  if constexpr (KS >= 3) {
    if (a.M % 128 != 0 && a.M % 192 == 0) return launch_cfg<192, 128, 2, 4, KS>(a, batch, st, plan);
  }
  if constexpr (KS == 1) {
    // k = 1 GEMMs with M a multiple of 192 (the 384 / 768-channel ResidualUnit k1 + skip): 192-row
    // tiles read each x column block 2x / 4x instead of 3x / 6x. x3: 192 x 64 single-buffered
    // tiles (154 VGPRs, three workgroups per CU), 384 x 384 at T = 5568 602 -> 541 us, 768 x 768
    // at T = 696 253 -> 249 (profiles/r04x_k1_192_ab.txt). fp32-input loop (M also a multiple of
    // 128): 768 x 768 k1 + skip at T = 696 485 -> 386 us, 384: 930 -> 922; 256-row tiles for
    // 512 / 768 were slower, 248 / 473 us (profiles/r01j_conv_k1_ab.txt).
    if (x3 && a.M % 192 == 0) return launch_cfg<192, 64, 2, 4, KS>(a, batch, st, plan);
    if (!x3 && a.M % 192 == 0 && a.M % 128 == 0) return launch_bn<192, 2, KS>(bn, a, batch, st, plan);
  }
  return launch_bn<128, 2, KS>(bn, a, batch, st, plan);
}

int dispatch_ks(int ks, const ConvArgs& a, int batch, hipStream_t st, ConvPlan* plan) {
  switch (ks) {
    case 1: return dispatch_tiles<1>(a, batch, st, plan);
    case 2: return dispatch_tiles<2>(a, batch, st, plan);
    case 3: return dispatch_tiles<3>(a, batch, st, plan);
    case 4: return dispatch_tiles<4>(a, batch, st, plan);
    case 7: return dispatch_tiles<7>(a, batch, st, plan);
    case 8: return dispatch_tiles<8>(a, batch, st, plan);
    case 16: return dispatch_tiles<16>(a, batch, st, plan);
    default: return VRVQ_ERR_UNSUPPORTED;
  }
}

__global__ void pack_conv1d_kernel(const float* __restrict__ w, int cout, int cin, int k,
                                   int cout_pad, float* __restrict__ wp) {
  const size_t total = (size_t)cin * k * cout_pad;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % cout_pad);
    const size_t rk = i / cout_pad;
    const int kk = (int)(rk % k);
    const int ci = (int)(rk / k);
    wp[i] = co < cout ? w[((size_t)co * cin + ci) * k + kk] : 0.0f;
  }
}

// Polyphase layout: wp[ci][tap][co*s + r]; tap 1 <-> x[m] (kernel index r),
// tap 0 <-> x[m-1] (kernel index r + s).
__global__ void pack_convt1d_kernel(const float* __restrict__ w, int cin, int cout, int s,
                                    int cout_pad, float* __restrict__ wp) {
  const size_t total = (size_t)cin * 2 * cout_pad;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int mm = (int)(i % cout_pad);
    const size_t rk = i / cout_pad;
    const int tap = (int)(rk % 2);
    const int ci = (int)(rk / 2);
    float v = 0.0f;
    if (mm < cout * s) {
      const int co = mm / s, r = mm - co * s;
      const int kk = tap == 1 ? r : r + s;
      v = w[((size_t)ci * cout + co) * (2 * s) + kk];
    }
    wp[i] = v;
  }
}

// Pre-split weight for the x3 mainloop (conv_x3.h): from the fp32 packed layout
// wp[ci][tap][m_pad] (WNConv1d; the polyphase ConvTranspose1d layout is the same with 2 taps)
// to w3[chunk][plane][octet][m_pad][8] bf16, octet o = tap * CK/8 + channel octet (zero for
// the padding octet and channels >= cin).
template <int KS>
__global__ void pack_x3_kernel(const float* __restrict__ wp, int cin, int m_pad,
                               u32x4* __restrict__ w3, size_t total) {
  using XC = X3Cfg<KS>;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i % m_pad);
    size_t r = i / m_pad;
    const int o = (int)(r % XC::NO2);
    r /= XC::NO2;
    const int plane = (int)(r % 3);
    const int chunk = (int)(r / 3);
    const int tap = o / XC::NC8, c8 = o - tap * XC::NC8;
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ci = chunk * XC::CK + c8 * 8 + u;
      v[u] = (o < XC::NO && ci < cin) ? wp[((size_t)ci * KS + tap) * m_pad + m] : 0.0f;
    }
    unsigned h[4], mm[4], l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) split3x2(v[2 * u], v[2 * u + 1], h[u], mm[u], l[u]);
    w3[i] = plane == 0 ? u32x4{h[0], h[1], h[2], h[3]}
          : plane == 1 ? u32x4{mm[0], mm[1], mm[2], mm[3]} : u32x4{l[0], l[1], l[2], l[3]};
  }
}

static long long x3_size_u16(int cin, int k, int m_pad) {
  auto sz = [&](int ck, int no2) {
    return (long long)((cin + ck - 1) / ck) * 3 * no2 * m_pad * 8;
  };
  switch (k) {
    case 1: return sz(X3Cfg<1>::CK, X3Cfg<1>::NO2);
    case 2: return sz(X3Cfg<2>::CK, X3Cfg<2>::NO2);
    case 3: return sz(X3Cfg<3>::CK, X3Cfg<3>::NO2);
    case 7: return sz(X3Cfg<7>::CK, X3Cfg<7>::NO2);
    default: return -1;
  }
}

}  // namespace

extern "C" int vrvq_x3_weight_size(int cin, int k, int cout_pad, long long* n_u16) {
  VRVQ_CHECK_ARG(n_u16 && cin > 0 && cout_pad > 0);
  const long long n = x3_size_u16(cin, k, cout_pad);
  if (n < 0) return VRVQ_ERR_UNSUPPORTED;
  *n_u16 = n;
  return 0;
}

extern "C" int vrvq_pack_x3_weight(const float* w_packed, int cin, int k, int cout_pad,
                                   uint16_t* w_x3, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(w_packed && w_x3 && cin > 0 && cout_pad > 0);
  const long long n = x3_size_u16(cin, k, cout_pad);
  if (n < 0) return VRVQ_ERR_UNSUPPORTED;
  const size_t total = (size_t)n / 8;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  u32x4* out = reinterpret_cast<u32x4*>(w_x3);
  hipStream_t st = as_stream(stream);
  switch (k) {
    case 1: hipLaunchKernelGGL(pack_x3_kernel<1>, dim3(grid), dim3(256), 0, st, w_packed, cin, cout_pad, out, total); break;
    case 2: hipLaunchKernelGGL(pack_x3_kernel<2>, dim3(grid), dim3(256), 0, st, w_packed, cin, cout_pad, out, total); break;
    case 3: hipLaunchKernelGGL(pack_x3_kernel<3>, dim3(grid), dim3(256), 0, st, w_packed, cin, cout_pad, out, total); break;
    default: hipLaunchKernelGGL(pack_x3_kernel<7>, dim3(grid), dim3(256), 0, st, w_packed, cin, cout_pad, out, total); break;
  }
  return vrvq_launch_status();
}

extern "C" int vrvq_conv1d(const float* x, int batch, int cin, int tin, const float* alpha,
                           const float* inv_alpha, const float* w_packed,
                           const uint16_t* w_x3, int cout,
                           int cout_pad, int k, int stride, int pad, int dil, const float* bias,
                           const float* residual, int epilogue, float* y, int tout,
                           const float* alpha_out, const float* inv_alpha_out, float* y_snake,
                           vrvq_stream_t stream) {
  return vrvq_conv1d_ws(x, batch, cin, tin, alpha, inv_alpha, w_packed, w_x3, cout, cout_pad, k,
                        stride, pad, dil, bias, residual, epilogue, y, tout, alpha_out,
                        inv_alpha_out, y_snake, nullptr, 0, stream);
}

extern "C" int vrvq_conv1d_workspace(int batch, int cin, int tin, int cout, int k, int stride,
                                     int pad, int dil, int x3, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && batch > 0 && cin > 0 && tin > 0 && cout > 0 && k > 0 && stride > 0 &&
                 dil > 0 && pad >= 0);
  const long long tout = ((long long)tin + 2LL * pad - (long long)dil * (k - 1) - 1) / stride + 1;
  VRVQ_CHECK_ARG(tout > 0);
  int S = 0;
  if (stride > 1) {  // the phase-split view (vrvq_conv1d: k = 2 stride, power-of-two stride)
    if (x3 && k == 2 * stride && (stride & (stride - 1)) == 0 && pad < stride)
      S = splitk_parts(cout, cin * stride, (int)tout, 2, true, false, true);
  } else {
    S = splitk_parts(cout, cin, (int)tout, k, false, false, x3 != 0);
  }
  *bytes = (long long)splitk_bytes(S, cout, (int)tout, batch);
  return 0;
}

extern "C" int vrvq_conv_last_launch(int out[5]) {
  VRVQ_CHECK_ARG(out);
  const unsigned v = g_last_launch.load(std::memory_order_relaxed);
  out[0] = (int)(v & 511);
  out[1] = (int)(v >> 9 & 511);
  out[2] = (int)(v >> 18 & 31);
  out[3] = (int)(v >> 23 & 3);
  out[4] = (int)(v >> 25 & 127);
  return 0;
}

namespace {

// The three conv entry points below their pointer checks, shared with vrvq_conv_plan (which
// passes plan and, for the buffers a decision asks about, any non-null address).

bool conv1d_geometry_ok(int batch, int cin, int tin, int cout, int cout_pad, int k, int stride,
                        int pad, int dil, int tout) {
  return batch > 0 && cin > 0 && tin > 0 && cout > 0 && k > 0 && stride > 0 && dil > 0 &&
         pad >= 0 && tout > 0 && cout_pad >= cout && cout_pad % 128 == 0 &&
         tout == ((long long)tin + 2LL * pad - (long long)dil * (k - 1) - 1) / stride + 1;
}

// a: the pointers of the call (w3, pj_part set where given). proj: vrvq_conv1d_proj, the MFMA
// tiles only (their epilogue owns the projection).
int run_conv1d(ConvArgs a, int batch, int cin, int tin, int cout, int cout_pad, int k, int stride,
               int pad, int dil, int tout, int epilogue, void* workspace, long long ws_bytes,
               hipStream_t st, ConvPlan* plan) {
  const bool proj = a.pj_part != nullptr;
  a.cin = cin; a.tin = tin; a.M = cout; a.m_pad = cout_pad; a.cout = cout;
  a.stride = stride; a.pad = pad; a.dil = dil; a.ng = tout; a.up = 0; a.up_pad = 0;
  a.ssh = 0;
  if (stride > 1 && (stride & (stride - 1)) == 0)
    while ((1 << a.ssh) < stride) ++a.ssh;
  a.ylen = tout; a.epi = epilogue;
  if (a.w3 != nullptr && !x3_offsets_fit(tin, cout_pad)) return VRVQ_ERR_UNSUPPORTED;
  if (workspace != nullptr) {
    long long need = 0;
    const int rc = vrvq_conv1d_workspace(batch, cin, tin, cout, k, stride, pad, dil,
                                         a.w3 != nullptr, &need);
    if (rc) return rc;
    VRVQ_CHECK_ARG(ws_bytes >= need);
    if (need > 0) a.ks_part = static_cast<float*>(workspace);
  }
  if (a.w3 != nullptr && stride > 1) {
    // strided conv on the x3 loop: a stride-1 k = 2 conv over the phase-split view of x
    // (conv_core.h ConvArgs::psh); w_x3 holds the planes of W'[co][c*s + r][j] = W[co][c][j*s + r]
    if (k != 2 * stride || a.ssh == 0 || pad >= stride) return VRVQ_ERR_UNSUPPORTED;
    a.psh = a.ssh; a.ppad = pad; a.pcin = cin; a.ptin = tin;
    a.cin = cin * stride; a.tin = tout + 1;
    a.stride = 1; a.pad = 0; a.dil = 1; a.ssh = 0;
    return dispatch_ks(2, a, batch, st, plan);
  }
  if (!proj && cout <= SMALL_COUT && stride == 1 &&
      cin * k * (cout == 1 ? 1 : SMALL_COUT) <= SMALL_WMAX)
    return launch_small(a, batch, k, st, plan);
  if (!proj && cin == 1 && k == 7 && stride == 1 && dil == 1 && !a.alpha && cout % CI1_CG == 0 &&
      tout % 4 == 0) {
    const long long nblk =
        (long long)batch * ((tout + 256 * CI1_T - 1) / (256 * CI1_T)) * (cout / CI1_CG);
    if (nblk <= 0 || nblk > 0x7fffffffLL) return VRVQ_ERR_ARG;
    if (plan) *plan = ConvPlan{PATH_CIN1, 0, 0, 0, k, 0, 0};
    return launch_kernel(conv_cin1_stream_kernel<7>, nblk, 256, 0, st, a, plan != nullptr);
  }
  return dispatch_ks(k, a, batch, st, plan);
}

int run_conv_transpose1d(ConvArgs a, int batch, int cin, int tin, int cout, int cout_pad,
                         int stride, int pad, hipStream_t st, ConvPlan* plan) {
  VRVQ_CHECK_ARG(batch > 0 && cin > 0 && tin > 0 && cout > 0 && stride > 0);
  // pad 0 = the padding=False windows of the chunked codec (models/dac_base.py:72-82)
  VRVQ_CHECK_ARG(pad >= 0 && pad < stride);
  VRVQ_CHECK_ARG(cout_pad >= cout * stride && cout_pad % 64 == 0);
  if (a.w3 != nullptr && !x3_offsets_fit(tin, cout_pad)) return VRVQ_ERR_UNSUPPORTED;
  a.cin = cin; a.tin = tin; a.M = cout * stride; a.m_pad = cout_pad; a.cout = cout;
  a.stride = 1; a.pad = 1; a.dil = 1; a.ng = tin + 1; a.up = stride; a.up_pad = pad;
  a.ylen = (tin - 1) * stride - 2 * pad + 2 * stride;
  a.epi = VRVQ_EPI_NONE;
  return dispatch_ks(2, a, batch, st, plan);
}

}  // namespace

extern "C" int vrvq_conv1d_ws(const float* x, int batch, int cin, int tin, const float* alpha,
                              const float* inv_alpha, const float* w_packed,
                              const uint16_t* w_x3, int cout, int cout_pad, int k, int stride,
                              int pad, int dil, const float* bias, const float* residual,
                              int epilogue, float* y, int tout, const float* alpha_out,
                              const float* inv_alpha_out, float* y_snake, void* workspace,
                              long long ws_bytes, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(x && w_packed && (y || y_snake));
  VRVQ_CHECK_ARG(y_snake == nullptr || (alpha_out && inv_alpha_out));
  VRVQ_CHECK_ARG(conv1d_geometry_ok(batch, cin, tin, cout, cout_pad, k, stride, pad, dil, tout));
  VRVQ_CHECK_ARG(alpha == nullptr || inv_alpha != nullptr);
  VRVQ_CHECK_ARG(epilogue >= 0 && epilogue <= 2);
  ConvArgs a{};
  a.x = x; a.alpha = alpha; a.inv_alpha = inv_alpha; a.w = w_packed;
  a.bias = bias; a.res = residual; a.y = y;
  a.alpha_o = alpha_out; a.inv_alpha_o = inv_alpha_out; a.ys = y_snake;
  a.w3 = reinterpret_cast<const unsigned*>(w_x3);
  return run_conv1d(a, batch, cin, tin, cout, cout_pad, k, stride, pad, dil, tout, epilogue,
                    workspace, ws_bytes, as_stream(stream), nullptr);
}

extern "C" int vrvq_conv1d_proj(const float* x, int batch, int cin, int tin, const float* alpha,
                                const float* inv_alpha, const float* w_packed,
                                const uint16_t* w_x3, int cout, int cout_pad, int k, int pad,
                                int dil, const float* bias, float* y, int tout,
                                const uint16_t* w3in, int nq, float* part, void* workspace,
                                long long ws_bytes, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(x && w_packed && w3in && part);
  VRVQ_CHECK_ARG(batch > 0 && cin > 0 && tin > 0 && cout > 0 && k > 0 && dil > 0 && pad >= 0 &&
                 tout > 0 && nq > 0);
  VRVQ_CHECK_ARG(cout_pad >= cout && cout_pad % 128 == 0);
  VRVQ_CHECK_ARG(alpha == nullptr || inv_alpha != nullptr);
  VRVQ_CHECK_ARG(((uintptr_t)part & 15) == 0 && ((uintptr_t)w3in & 15) == 0);
  if (cout != 1024 || nq > 32) return VRVQ_ERR_UNSUPPORTED;  // the latent (RD) / CH_NQMAX
  VRVQ_CHECK_ARG(conv1d_geometry_ok(batch, cin, tin, cout, cout_pad, k, 1, pad, dil, tout));
  VRVQ_CHECK_ARG((long long)batch * tout * nq * 8 * 8 < 0x7fffffffLL);
  ConvArgs a{};
  a.x = x; a.alpha = alpha; a.inv_alpha = inv_alpha; a.w = w_packed; a.bias = bias; a.y = y;
  a.w3 = reinterpret_cast<const unsigned*>(w_x3);
  a.pj_w3 = reinterpret_cast<const unsigned*>(w3in);
  a.pj_part = part;
  a.pj_nq = nq;
  a.pj_nf = batch * tout;
  // split-K as vrvq_conv1d_ws (same shape, same parts)
  return run_conv1d(a, batch, cin, tin, cout, cout_pad, k, 1, pad, dil, tout, VRVQ_EPI_NONE,
                    workspace, ws_bytes, as_stream(stream), nullptr);
}

extern "C" int vrvq_conv_transpose1d(const float* x, int batch, int cin, int tin,
                                     const float* alpha, const float* inv_alpha,
                                     const float* w_packed, int cout, int cout_pad, int stride,
                                     const float* bias, float* y, const float* alpha_out,
                                     const float* inv_alpha_out, float* y_snake,
                                     vrvq_stream_t stream) {
  // math.ceil(stride / 2), models/layers.py:102
  return vrvq_conv_transpose1d_pad(x, batch, cin, tin, alpha, inv_alpha, w_packed, nullptr,
                                   cout, cout_pad, stride, (stride + 1) / 2, bias, y, alpha_out,
                                   inv_alpha_out, y_snake, stream);
}

extern "C" int vrvq_conv_transpose1d_pad(const float* x, int batch, int cin, int tin,
                                         const float* alpha, const float* inv_alpha,
                                         const float* w_packed, const uint16_t* w_x3,
                                         int cout, int cout_pad,
                                         int stride, int pad, const float* bias, float* y,
                                         const float* alpha_out, const float* inv_alpha_out,
                                         float* y_snake, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(x && w_packed && (y || y_snake));
  VRVQ_CHECK_ARG(y_snake == nullptr || (alpha_out && inv_alpha_out));
  VRVQ_CHECK_ARG(alpha == nullptr || inv_alpha != nullptr);
  ConvArgs a{};
  a.x = x; a.alpha = alpha; a.inv_alpha = inv_alpha; a.w = w_packed; a.bias = bias;
  a.res = nullptr; a.y = y;
  a.alpha_o = alpha_out; a.inv_alpha_o = inv_alpha_out; a.ys = y_snake;
  a.w3 = reinterpret_cast<const unsigned*>(w_x3);
  return run_conv_transpose1d(a, batch, cin, tin, cout, cout_pad, stride, pad, as_stream(stream),
                              nullptr);
}

extern "C" int vrvq_conv_plan(int kind, int batch, int cin, int tin, int cout, int k, int stride,
                              int pad, int dil, int has_x3, int has_workspace, int out[7]) {
  VRVQ_CHECK_ARG(out && kind >= VRVQ_PLAN_CONV && kind <= VRVQ_PLAN_CONV_TRANSPOSE);
  static float present[4];  // stands for every buffer a decision asks about; never dereferenced
  ConvArgs a{};
  a.w3 = has_x3 ? reinterpret_cast<const unsigned*>(present) : nullptr;
  void* ws = has_workspace ? present : nullptr;
  ConvPlan p{};
  int rc;
  if (kind == VRVQ_PLAN_CONV_TRANSPOSE) {
    VRVQ_CHECK_ARG(stride > 0 && k == 2 * stride && dil == 1);
    // the packers' padding (vrvq_pack_convt1d_weight callers: whole 128- or 192-row tiles)
    const long long rows = (long long)cout * stride, rt = 128 % stride == 0 ? 128 : 192;
    VRVQ_CHECK_ARG(cout > 0 && rows < 0x7fffff00LL);
    rc = run_conv_transpose1d(a, batch, cin, tin, cout, (int)((rows + rt - 1) / rt * rt), stride,
                              pad, nullptr, &p);
  } else {
    VRVQ_CHECK_ARG(cout > 0 && cout < 0x7fffff00 && k > 0 && stride > 0 && dil > 0 && tin > 0 &&
                   pad >= 0);
    const long long tout = ((long long)tin + 2LL * pad - (long long)dil * (k - 1) - 1) / stride + 1;
    const int cout_pad = (cout + 127) / 128 * 128;
    VRVQ_CHECK_ARG(tout > 0 && tout <= 0x7fffffffLL);
    VRVQ_CHECK_ARG(conv1d_geometry_ok(batch, cin, tin, cout, cout_pad, k, stride, pad, dil,
                                      (int)tout));
    if (kind == VRVQ_PLAN_PROJ) {
      VRVQ_CHECK_ARG(stride == 1);
      if (cout != 1024) return VRVQ_ERR_UNSUPPORTED;
      a.pj_part = present;
    }
    rc = run_conv1d(a, batch, cin, tin, cout, cout_pad, k, stride, pad, dil, (int)tout,
                    VRVQ_EPI_NONE, ws, 0x7fffffffffffffffLL, nullptr, &p);
  }
  if (rc) return rc;
  const int v[7] = {p.BM, p.BN, p.KS, p.x3, p.S, p.path, p.WM};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return 0;
}

extern "C" int vrvq_pack_conv1d_weight(const float* w, int cout, int cin, int k, int cout_pad,
                                       float* w_packed, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(w && w_packed && cout > 0 && cin > 0 && k > 0 && cout_pad >= cout);
  const size_t total = (size_t)cin * k * cout_pad;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(pack_conv1d_kernel, dim3(grid), dim3(256), 0, as_stream(stream), w, cout,
                     cin, k, cout_pad, w_packed);
  return vrvq_launch_status();
}

extern "C" int vrvq_pack_convt1d_weight(const float* w, int cin, int cout, int stride,
                                        int cout_pad, float* w_packed, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(w && w_packed && cout > 0 && cin > 0 && stride > 0 && cout_pad >= cout * stride);
  const size_t total = (size_t)cin * 2 * cout_pad;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(pack_convt1d_kernel, dim3(grid), dim3(256), 0, as_stream(stream), w, cin,
                     cout, stride, cout_pad, w_packed);
  return vrvq_launch_status();
}
