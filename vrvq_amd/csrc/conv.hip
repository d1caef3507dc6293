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
//
// This file: the entry points and their argument checks, the kernels off the MFMA tiles, the
// weight packers. Which kernel a shape runs is decided in conv_plan.h; the MFMA kernels
// (conv_kernels.h) are compiled in conv_k*.hip, each behind a launch table (conv_tables.h).
#include "common.h"
#include "conv_tables.h"
#include "conv_x3.h"
#include <atomic>

namespace {

using namespace vrvq_conv;

// Small-Cout conv (Cout <= 8, stride 1): the decoder's 96->1 k7 + Tanh output layer and the
// importance subnet's 32->8 / 8->1 k3 tail. An MFMA tile would be >= 75 % padding and the layer
// is HBM-bound on reading x, so: one thread per output sample, snake(x) rows of SC channels
// staged in LDS per step (window 256 + (k-1)*dil), every output channel accumulated in VGPRs.
// (The SMALL_*, C1_* and CI1_* constants of the three kernels here: conv_geom.h, where the
// planner reads them too.)
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

// Tile and path of the last MFMA conv launch (vrvq_conv_last_launch, a host-side debug query:
// the tests assert the path they claim to pin). One word, so concurrent callers never read a
// torn record: BM (9 bits) | BN << 9 (9) | KS << 18 (5) | x3 << 23 (2) | S << 25 (7).
std::atomic<unsigned> g_last_launch{0};

void note_launch(const ConvPlan& p) {
  g_last_launch.store((unsigned)p.BM | (unsigned)p.BN << 9 | (unsigned)p.KS << 18 |
                      (unsigned)p.x3 << 23 | (unsigned)(p.S & 127) << 25,
                      std::memory_order_relaxed);
}

// The translation unit that holds an MFMA plan's kernel (conv_k*.hip; null: no such taps).
const ConvTable* table_of(const ConvPlan& p) {
  switch (p.KS) {
    case 1: return p.x3 ? &conv_k1_x3 : &conv_k1;
    case 2: return p.view ? &conv_k2_view : p.x3 ? &conv_k2_x3 : &conv_k2;
    case 3: return p.x3 ? &conv_k3_x3 : &conv_k3;
    case 4: return &conv_k4;
    case 7: return p.x3 ? &conv_k7_x3 : &conv_k7;
    case 8: return &conv_k8;
    case 16: return &conv_k16;
    default: return nullptr;
  }
}

// Whether the plan's kernel exists (host only: vrvq_conv_plan answers it without a device).
bool plan_has_kernel(const ConvPlan& p) {
  if (p.path != PATH_MFMA) return true;  // the off-tile kernels below
  const ConvTable* t = table_of(p);
  return t != nullptr && t->has(p);
}

// Launch a plan. a: the call's pointers and the GEMM's geometry.
int launch_conv(const ConvPlan& p, ConvArgs a, hipStream_t st) {
  if (p.path == PATH_CIN1) return launch_kernel(conv_cin1_stream_kernel<7>, p.grid, 256, 0, st, a);
  if (p.path == PATH_SMALL_COUT) {
    if (p.cout1_stream) {
      // the consumer-side Snake variant is its own kernel: its registers do not set the plain
      // variant's occupancy
      void (*kernel)(ConvArgs) =
          p.KS == 7 ? (a.alpha ? conv_cout1_stream_kernel<7, 3, true> : conv_cout1_stream_kernel<7, 3, false>)
                    : (a.alpha ? conv_cout1_stream_kernel<3, 1, true> : conv_cout1_stream_kernel<3, 1, false>);
      return launch_kernel(kernel, p.grid, 256, 0, st, a);
    }
    if (a.M == 1)
      hipLaunchKernelGGL(conv_small_cout_kernel<1>, dim3((unsigned)p.grid), dim3(256), p.lds, st, a, p.KS);
    else
      hipLaunchKernelGGL(conv_small_cout_kernel<SMALL_COUT>, dim3((unsigned)p.grid), dim3(256), p.lds, st, a, p.KS);
    return vrvq_launch_status();
  }
  const ConvTable* t = table_of(p);
  if (t == nullptr) return VRVQ_ERR_UNSUPPORTED;
  a.n_mt = (a.M + p.BM - 1) / p.BM;
  a.n_nt = (a.ng + p.BN - 1) / p.BN;
  a.ks_split = p.S;
  const int rc = t->launch(p, a, st);
  if (rc == 0) note_launch(p);
  return rc;
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

// The three conv entry points below their pointer checks: the call's ConvShape (what the
// planner, vrvq_conv_plan and vrvq_conv1d_workspace see of it), then plan and launch.

bool conv1d_geometry_ok(int batch, int cin, int tin, int cout, int cout_pad, int k, int stride,
                        int pad, int dil, int tout) {
  return batch > 0 && cin > 0 && tin > 0 && cout > 0 && k > 0 && stride > 0 && dil > 0 &&
         pad >= 0 && tout > 0 && cout_pad >= cout && cout_pad % 128 == 0 &&
         tout == ((long long)tin + 2LL * pad - (long long)dil * (k - 1) - 1) / stride + 1;
}

ConvShape conv1d_shape(int batch, int cin, int tin, int cout, int cout_pad, int k, int stride,
                       int pad, int dil, int tout, bool x3, bool snake, bool proj, bool ws) {
  ConvShape s{};
  s.k = k; s.M = cout; s.cin = cin; s.tin = tin; s.ng = tout;
  s.stride = stride; s.pad = pad; s.dil = dil; s.up = 0; s.m_pad = cout_pad; s.batch = batch;
  s.x3 = x3; s.snake = snake; s.proj = proj; s.workspace = ws;
  return s;
}

// The polyphase GEMM of a transposed conv: 2 taps, M = Cout * stride phase rows, Tin + 1 columns.
ConvShape convt_shape(int batch, int cin, int tin, int cout, int cout_pad, int stride, bool x3,
                      bool snake) {
  ConvShape s{};
  s.k = 2; s.M = cout * stride; s.cin = cin; s.tin = tin; s.ng = tin + 1;
  s.stride = 1; s.pad = 1; s.dil = 1; s.up = stride; s.m_pad = cout_pad; s.batch = batch;
  s.x3 = x3; s.snake = snake;
  return s;
}

bool convt_geometry_ok(int batch, int cin, int tin, int cout, int cout_pad, int stride, int pad) {
  // pad 0 = the padding=False windows of the chunked codec (models/dac_base.py:72-82)
  return batch > 0 && cin > 0 && tin > 0 && cout > 0 && stride > 0 && pad >= 0 && pad < stride &&
         cout_pad >= cout * stride && cout_pad % 64 == 0;
}

// a: the pointers of the call (w3, pj_part set where given); s: conv1d_shape of the call.
int run_conv1d(ConvArgs a, const ConvShape& s, int epilogue, void* workspace, long long ws_bytes,
               hipStream_t st) {
  ConvPlan p;
  const int rc = plan_conv1d(s, &p);
  if (rc) return rc;
  if (p.S > 0) {
    VRVQ_CHECK_ARG(ws_bytes >= splitk_bytes(p.S, s.M, s.ng, s.batch));
    a.ks_part = static_cast<float*>(workspace);
  }
  a.cin = s.cin; a.tin = s.tin; a.M = s.M; a.m_pad = s.m_pad; a.cout = s.M;
  a.stride = s.stride; a.pad = s.pad; a.dil = s.dil; a.ng = s.ng; a.up = 0; a.up_pad = 0;
  a.ssh = 0;
  if (s.stride > 1 && (s.stride & (s.stride - 1)) == 0)
    while ((1 << a.ssh) < s.stride) ++a.ssh;
  a.ylen = s.ng; a.epi = epilogue;
  if (p.view) {
    // strided conv on the x3 loop: a stride-1 k = 2 conv over the phase-split view of x
    // (conv_core.h ConvArgs::psh); w_x3 holds the planes of W'[co][c*s + r][j] = W[co][c][j*s + r]
    a.psh = a.ssh; a.ppad = s.pad; a.pcin = s.cin; a.ptin = s.tin;
    a.cin = s.cin * s.stride; a.tin = s.ng + 1;
    a.stride = 1; a.pad = 0; a.dil = 1; a.ssh = 0;
  }
  return launch_conv(p, a, st);
}

}  // namespace

extern "C" int vrvq_conv1d_workspace(int batch, int cin, int tin, int cout, int k, int stride,
                                     int pad, int dil, int x3, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && batch > 0 && cin > 0 && tin > 0 && cout > 0 && cout < 0x7fffff00 &&
                 k > 0 && stride > 0 && dil > 0 && pad >= 0);
  const long long tout = ((long long)tin + 2LL * pad - (long long)dil * (k - 1) - 1) / stride + 1;
  VRVQ_CHECK_ARG(tout > 0 && tout <= 0x7fffffffLL);
  // the plan of the call with a workspace (the packers' row padding, no consumer-side Snake: its
  // table can only take a split away); a shape with no plan needs none
  ConvPlan p;
  const ConvShape s = conv1d_shape(batch, cin, tin, cout, (cout + 127) / 128 * 128, k, stride, pad,
                                   dil, (int)tout, x3 != 0, false, false, true);
  *bytes = plan_conv1d(s, &p) == 0 ? splitk_bytes(p.S, cout, (int)tout, batch) : 0;
  return 0;
}

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
  const ConvShape s = conv1d_shape(batch, cin, tin, cout, cout_pad, k, stride, pad, dil, tout,
                                   w_x3 != nullptr, alpha != nullptr, false, workspace != nullptr);
  return run_conv1d(a, s, epilogue, workspace, ws_bytes, as_stream(stream));
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
  const ConvShape s = conv1d_shape(batch, cin, tin, cout, cout_pad, k, 1, pad, dil, tout,
                                   w_x3 != nullptr, alpha != nullptr, true, workspace != nullptr);
  return run_conv1d(a, s, VRVQ_EPI_NONE, workspace, ws_bytes, as_stream(stream));
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
  VRVQ_CHECK_ARG(convt_geometry_ok(batch, cin, tin, cout, cout_pad, stride, pad));
  const ConvShape s = convt_shape(batch, cin, tin, cout, cout_pad, stride, w_x3 != nullptr,
                                  alpha != nullptr);
  ConvPlan p;
  const int rc = plan_conv_transpose1d(s, &p);
  if (rc) return rc;
  ConvArgs a{};
  a.x = x; a.alpha = alpha; a.inv_alpha = inv_alpha; a.w = w_packed; a.bias = bias;
  a.res = nullptr; a.y = y;
  a.alpha_o = alpha_out; a.inv_alpha_o = inv_alpha_out; a.ys = y_snake;
  a.w3 = reinterpret_cast<const unsigned*>(w_x3);
  a.cin = cin; a.tin = tin; a.M = s.M; a.m_pad = cout_pad; a.cout = cout;
  a.stride = 1; a.pad = 1; a.dil = 1; a.ng = s.ng; a.up = stride; a.up_pad = pad;
  a.ylen = (tin - 1) * stride - 2 * pad + 2 * stride;
  a.epi = VRVQ_EPI_NONE;
  return launch_conv(p, a, as_stream(stream));
}

extern "C" int vrvq_conv_plan(int kind, int batch, int cin, int tin, int cout, int k, int stride,
                              int pad, int dil, int has_x3, int has_workspace, int out[7]) {
  VRVQ_CHECK_ARG(out && kind >= VRVQ_PLAN_CONV && kind <= VRVQ_PLAN_CONV_TRANSPOSE);
  ConvPlan p;
  int rc;
  if (kind == VRVQ_PLAN_CONV_TRANSPOSE) {
    VRVQ_CHECK_ARG(stride > 0 && k == 2 * stride && dil == 1);
    // the packers' padding (vrvq_pack_convt1d_weight callers: whole 128- or 192-row tiles)
    const long long rows = (long long)cout * stride, rt = 128 % stride == 0 ? 128 : 192;
    VRVQ_CHECK_ARG(cout > 0 && rows < 0x7fffff00LL);
    const int cout_pad = (int)((rows + rt - 1) / rt * rt);
    VRVQ_CHECK_ARG(convt_geometry_ok(batch, cin, tin, cout, cout_pad, stride, pad));
    rc = plan_conv_transpose1d(
        convt_shape(batch, cin, tin, cout, cout_pad, stride, has_x3 != 0, false), &p);
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
    }
    rc = plan_conv1d(conv1d_shape(batch, cin, tin, cout, cout_pad, k, stride, pad, dil, (int)tout,
                                  has_x3 != 0, false, kind == VRVQ_PLAN_PROJ, has_workspace != 0),
                     &p);
  }
  if (rc) return rc;
  if (!plan_has_kernel(p)) return VRVQ_ERR_UNSUPPORTED;  // a plan the tables of conv_k*.hip lack
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
