// The MFMA conv kernels, for the per-tap translation units conv_k*.hip to instantiate: each names
// its kernels once, as entries of a launch table (conv_tables.h). See conv.hip for the GEMM
// mapping and the MFMA operand layouts.
#pragma once
#include "conv_tables.h"
#include "conv_x3.h"

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

// A table entry from the kernel's own template arguments (conv_mfma_kernel's list): the key the
// planner's plan has to carry to mean this kernel, and the kernel.
template <int BM, int BN, int WM, int NW, int KS, bool X3, bool PH = false,
          bool PAIR = x3_pair<KS, BM, BN>(), bool SPLIT = false>
ConvKernel conv_kernel() {
  void (*epilogue)(ConvArgs) = nullptr;
  if constexpr (SPLIT) epilogue = conv_splitk_epilogue_kernel<BM, BN, WM, NW>;
  return {plan_key(BM, BN, WM, KS, X3 ? (PAIR ? 2 : 1) : 0, PH, SPLIT), 64 * NW,
          conv_mfma_kernel<BM, BN, WM, NW, KS, X3, PH, PAIR, SPLIT>, epilogue};
}

}  // namespace
