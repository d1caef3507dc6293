// Which kernel a forward conv runs: the decision as ordinary host code. A ConvShape says what the
// decision depends on, plan_conv1d / plan_conv_transpose1d turn it into a ConvPlan (or a status),
// and the plan is all a launch needs beside the pointers: the entry points of conv.hip launch it
// through the tables of conv_k*.hip, vrvq_conv_plan hands it back without touching a device, and
// vrvq_conv1d_workspace reads its S. No HIP include and no device code: this header compiles with
// the host C++ compiler alone. DESIGN.md "Conv tiles" has the same rules as a table.
#pragma once
#include "conv_geom.h"
#include "vrvq.h"

namespace vrvq_conv {

// A conv as a call states it (plan_conv1d) or as the GEMM sees it (plan_mfma: M = GEMM rows,
// ng = GEMM columns; under the phase-split view of a strided conv cin / tin are the view's and
// stride / pad / dil are 1 / 0 / 1).
struct ConvShape {
  int k;                 // taps
  int M;                 // Cout; Cout * up phase rows for the transposed conv
  int cin, tin;
  int ng;                // output columns: Tout; Tin + 1 for the transposed conv
  int stride, pad, dil;
  int up;                // transposed conv: its stride (0: a conv)
  int m_pad;             // rows of the packed weight
  int batch;
  bool x3;               // bf16 weight planes given (conv_x3.h)
  bool snake;            // consumer-side Snake given (alpha)
  bool proj;             // RVQ in_proj epilogue (vrvq_conv1d_proj)
  bool workspace;        // split-K workspace given
};

enum ConvPath { PATH_MFMA = 0, PATH_SMALL_COUT = 1, PATH_CIN1 = 2 };

struct ConvPlan {
  int path;              // ConvPath
  int BM, BN, WM;        // MFMA tile and its wave rows (0 off the MFMA tiles)
  int KS;                // the GEMM's taps (2: the phase-split view, the polyphase ConvTranspose)
  int x3;                // 0 fp32-input loop | 1 x3 on plain K chunks | 2 x3 on pair chunks
  int S;                 // split-K parts (0: unsplit)
  bool view;             // the GEMM runs over the phase-split view of a strided conv
  bool cout1_stream;     // PATH_SMALL_COUT: conv_cout1_stream_kernel, not conv_small_cout_kernel
  int lds;               // dynamic LDS bytes of the launch
  int lds_epi;           // ... of the split-K epilogue launch (S > 0)
  int grid;              // workgroups (S > 0: tiles * S, the epilogue launch runs grid / S)
  bool split() const { return S > 0; }
};

// What selects a conv_mfma_kernel instantiation. conv_kernels.h derives a table entry's key from
// the kernel's own template arguments, the launch looks the plan's key up.
constexpr unsigned plan_key(int bm, int bn, int wm, int ks, int x3, bool view, bool split) {
  return (unsigned)bm | (unsigned)bn << 9 | (unsigned)ks << 18 | (unsigned)x3 << 23 |
         (unsigned)wm << 25 | (unsigned)view << 28 | (unsigned)split << 29;
}
inline unsigned plan_key(const ConvPlan& p) {
  return plan_key(p.BM, p.BN, p.WM, p.KS, p.x3, p.view, p.split());
}

constexpr int CONV_LDS_MAX = 160 * 1024;
constexpr long long CONV_GRID_MAX = 0x7fffffffLL;

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

// K parts of a GEMM (0: none); g.cin = the GEMM's channels (the view's for a strided conv). The
// same for vrvq_conv1d_proj (the encoder's last conv, whose shape the ImportanceSubnet's first
// conv shares): its projection epilogue then runs in the split-K epilogue launch, on the same z
// bits as the plain conv's.
inline int splitk_parts(const ConvShape& g, bool view) {
  if (!g.x3 || g.up > 0 || g.ng > 96 || g.M % 128 != 0) return 0;
  if (!(g.k == 3 || g.k == 7 || (g.k == 2 && view))) return 0;
  const int ck = x3_ck(g.k, g.k == 2);  // (the only 2-tap GEMM that splits is the view's: pair chunks)
  if (g.k == 2 && g.cin % ck != 0) return 0;
  const int nch = (g.cin + ck - 1) / ck;
  const int S = nch / SPLITK_MIN_CHUNKS < SPLITK_PARTS ? nch / SPLITK_MIN_CHUNKS : SPLITK_PARTS;
  return S >= 2 ? S : 0;
}

// Workspace bytes of a plan: S partial accumulators per 128 x 96 tile.
inline long long splitk_bytes(int S, int M, int ng, int batch) {
  return S ? (long long)S * batch * (M / 128) * ((ng + 95) / 96) * 128 * 96 * 4 : 0;
}

// ---- Tile choice ----
// (a) Column width BN of the tile for ng GEMM columns.
//
// T <= 96 layers: one 96-wide tile per clip when that gives at least this many workgroups (1.5
// per CU), else three 32-wide tiles: each N tile re-streams its M tile's whole weight block, so
// the narrow tiles triple the weight traffic, but with fewer 96-wide ones the CUs run short of
// workgroups to hide each one's serial K loop (profiles/r02zl_x3_sq_counters.txt; the k3 / k7
// layers 96-wide at B = 32 no faster, profiles/r05zf_t87_tiles_ab.txt).
constexpr long long BN96_MIN_WORKGROUPS = 384;

inline int tile_width(const ConvShape& g, bool view) {
  const bool x3_2tap = g.k == 2 && g.x3;
  if (g.ng <= 32) return 32;
  if (g.ng <= 96) {
    // 2-tap x3 GEMMs: the 32-wide tile pairs its K octets (conv_geom.h x3_pair) and the 96-wide
    // one does not, so a clip's sums would change order with the batch. Their width is fixed
    // per layer type instead (batch-invariant outputs, tests/test_gpu_parity.py
    // test_batch_invariance_*): the polyphase ConvTranspose 96-wide, the others (the phase-split
    // strided convs: 96-wide 691 -> 629 us for 512 -> 1024 s8, bench within the spread,
    // profiles/r05zf_t87_tiles_ab.txt) 32-wide.
    if (x3_2tap) return g.up > 0 ? 96 : 32;
    return (long long)((g.M + 127) / 128) * g.batch >= BN96_MIN_WORKGROUPS ? 96 : 32;
  }
  // Longer rows: 128-wide, or 64-wide below T = 4096 where that pads markedly fewer columns.
  // Not for k = 16 (the stride-8 encoder convs on the fp32-input loop): the 8 MB weight block
  // does not fit in L2, so the 128-wide tile's halved weight re-streaming beats its padding
  // (1490 -> 1323 us at T = 696, profiles/r02u_conv_ab.txt). Nor for the x3 strided convs and
  // ConvTransposes, whose 128-wide tile runs 32-channel pair chunks: 256 -> 512 s8 at T = 696
  // 940 -> 878 us, ConvT 768 -> 384 s8 1388 -> 1296 us (profiles/r04ze_ph128_ab.txt).
  auto waste = [&](int bn) { return ((g.ng + bn - 1) / bn) * bn - g.ng; };
  if (g.ng < 4096 && g.k != 16 && waste(64) * 10 < waste(128) * 7 &&
      !(x3_2tap && (view || g.up > 0)))
    return 64;
  return 128;
}

// x3 k7 layers from this many columns (M a multiple of 64 and >= 128, Cin a multiple of 16) run
// 64 x 256 tiles on 16-channel "pair" K-chunks (conv_x3.h: no zero octet, 168 MFMAs per wave
// between barriers). 384 x 384 k7 at T = 5568, B = 32: 2027 -> 755-796 us, 256 x 256: 934 ->
// 781-785 us; 768 x 768 / 512 x 512 k7 at T = 696: 1125 -> 962 / 514 -> 407 us despite 72 of
// every 768 columns padded (profiles/r03_x3_pair_ab.txt).
constexpr int K7_PAIR_MIN_COLUMNS = 640;

struct ConvTile {
  int BM, BN, WM;
};

// (b) Row tile BM from the GEMM rows M; the first rule that applies.
inline ConvTile choose_tile(const ConvShape& g, bool view) {
  const int ks = g.k, M = g.M, bn = tile_width(g, view);
  const bool x3 = g.x3;
  // a BM-row tile, 64 columns wide where tile_width chose that (k = 16 never does), else 128
  auto wide = [&](int bm, int wm, int w) { return ConvTile{bm, w == 64 && ks != 16 ? 64 : 128, wm}; };
  // Polyphase ConvTranspose1d with a stride that does not divide 128 (3, 6): 192-row tiles,
  // which hold whole output channels, 64-wide up to T = 96 (other strides, 5, 7, ..., are
  // rejected by plan_mfma).
  if (ks == 2 && g.up > 0 && 128 % g.up != 0) return wide(192, 2, bn <= 96 ? 64 : bn);
  if (M <= 32) return {32, 128, 1};
  if (ks == 7 && x3 && M >= 128 && M % 64 == 0 && g.cin % 16 == 0 && g.ng >= K7_PAIR_MIN_COLUMNS)
    return {64, 256, 1};
  // T <= 96: 128 rows at the width chosen above
  if (bn == 32) return {128, 32, 4};
  if (bn == 96) return {128, 96, 4};
  if (M <= 64) return wide(64, 2, bn);
  // 96- and 192-row tiles: no padded rows for the C = 96 / 192 decoder blocks
  if (M <= 96) return {96, 128, 1};
  // 768 x 768 k7 at T = 696: 2150 -> 1795 us with 192-row x 64-col tiles (K chunk 4 channels),
  // 427 -> 434 audio-sec/s end to end (profiles/r01j_conv_k7_ab.txt)
  if (ks == 7 && M % 192 == 0 && bn == 64) return {192, 64, 2};
  if (ks == 2) {
    // Polyphase ConvTranspose1d, M = Cout * stride phase rows. fp32-input loop, M a multiple of
    // 192: 192-row tiles (ConvT 768 -> 384 s8 2443 -> 2345 us, 384 -> 192 s4 2887 -> 2660 us,
    // profiles/r01k_convt_ab.txt); with the x3 weights the 128-row tiles, two workgroups per CU,
    // are faster (638 -> 649 audio-sec/s at B = 32, profiles/r02zh_tile_ab.txt) ...
    if (g.up > 0 && !x3 && M % 192 == 0) return wide(192, 2, bn);
    // ... except M a multiple of 96 and not of 128 (192 -> 96 s2: M = 192): 96-row tiles on the
    // pair chunks, two workgroups per CU, instead of the two-stage 192 x 128 tile (981-988 vs
    // 942-954 us, profiles/r06t_convt_layers.txt)
    if (g.up > 0 && x3 && M % 96 == 0 && M % 128 != 0) return {96, 128, 1};
  }
  if (ks >= 3 && M % 128 != 0 && M % 192 == 0) return {192, 128, 2};
  if (ks == 1) {
    // k = 1 GEMMs with M a multiple of 192 (the 384 / 768-channel ResidualUnit k1 + skip): 192-row
    // tiles read each x column block 2x / 4x instead of 3x / 6x. x3: 192 x 64 single-buffered
    // tiles (154 VGPRs, three workgroups per CU), 384 x 384 at T = 5568 602 -> 541 us, 768 x 768
    // at T = 696 253 -> 249 (profiles/r04x_k1_192_ab.txt). fp32-input loop (M also a multiple of
    // 128): 768 x 768 k1 + skip at T = 696 485 -> 386 us, 384: 930 -> 922; 256-row tiles for
    // 512 / 768 were slower, 248 / 473 us (profiles/r01j_conv_k1_ab.txt).
    if (x3 && M % 192 == 0) return {192, 64, 2};
    if (!x3 && M % 192 == 0 && M % 128 == 0) return wide(192, 2, bn);
  }
  return wide(128, 2, bn);
}

// The MFMA tiles of a GEMM g (view: over the phase-split view). snake_cin: the channels of the
// consumer-side Snake (the call's Cin; 0 without one), whose table the pair tiles keep in LDS.
inline int plan_mfma(const ConvShape& g, bool view, int snake_cin, ConvPlan* out) {
  const int ks = g.k;
  if (!(ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 7 || ks == 8 || ks == 16))
    return VRVQ_ERR_UNSUPPORTED;
  ConvPlan p{};
  p.path = PATH_MFMA;
  p.KS = ks;
  p.view = view;
  auto max2 = [](long long a, long long b) { return a > b ? a : b; };

  if (g.workspace) {
    const int S = splitk_parts(g, view);
    if (S > 0) {
      const int xw = 95 + (ks - 1) * g.dil + 1;
      const long long tiles = (long long)(g.M / 128) * ((g.ng + 95) / 96) * g.batch;
      if (g.m_pad < g.M) return VRVQ_ERR_ARG;
      if (xw <= x3_xw_max(ks, 96)) {  // (else, or where the stage does not fit: the tiles below)
        if (tiles * S > CONV_GRID_MAX) return VRVQ_ERR_ARG;
        const long long epi = max2(128LL * epi_bnp(128, 96) * 4, g.proj ? PJE_LDS : 0);
        // the pair tiles' Snake table only when the staging applies a Snake (the producer-side
        // snake(x) inputs of the k7 layers need none: 3-6 KB of LDS back)
        const long long lx = max2(x3_lds_bytes(ks, 128, 96, ks == 2, xw, snake_cin), epi);
        if (lx <= CONV_LDS_MAX) {
          p.BM = 128, p.BN = 96, p.WM = 4;
          p.x3 = ks == 2 ? 2 : 1;
          p.S = S;
          p.lds = (int)lx, p.lds_epi = (int)epi, p.grid = (int)(tiles * S);
          *out = p;
          return 0;
        }
      }
    }
  }

  const ConvTile t = choose_tile(g, view);
  p.BM = t.BM, p.BN = t.BN, p.WM = t.WM;
  const int n_mt = (g.M + t.BM - 1) / t.BM, n_nt = (g.ng + t.BN - 1) / t.BN;
  if (g.m_pad < n_mt * t.BM) return VRVQ_ERR_ARG;
  // transposed conv: a tile must hold whole output channels (rows co*up .. co*up + up-1), the
  // epilogue maps rows back with co0 = m0 / up
  if (g.up > 0 && t.BM % g.up != 0) return VRVQ_ERR_UNSUPPORTED;
  const int xw = (t.BN - 1) * g.stride + (ks - 1) * g.dil + 1;
  long long epi = (long long)t.BM * epi_bnp(t.BM, t.BN) * 4;
  if (g.proj) {  // RVQ in_proj epilogue: one latent split per tile, its z planes in LDS
    if (t.BM != 128) return VRVQ_ERR_UNSUPPORTED;
    epi = max2(epi, PJE_LDS);
  }
  const long long nblk = (long long)n_mt * n_nt * g.batch;
  if (nblk <= 0 || nblk > CONV_GRID_MAX) return VRVQ_ERR_ARG;
  p.grid = (int)nblk;

  // bf16x3 split path (conv_x3.h): stride-1 windows, a pre-split weight, the stage in LDS
  if ((ks == 1 || ks == 2 || ks == 3 || ks == 7) && g.x3 && g.stride == 1 &&
      xw <= x3_xw_max(ks, t.BN)) {
    // pair tiles (conv_x3.h) need whole K-chunks: other Cin run the tile on plain chunks
    const bool pair = x3_pair(ks, t.BM, t.BN) && g.cin % x3_ck(ks, true) == 0;
    const long long lx = max2(x3_lds_bytes(ks, t.BM, t.BN, pair, xw, snake_cin), epi);
    if (lx <= CONV_LDS_MAX) {
      p.x3 = pair ? 2 : 1;
      p.lds = (int)lx;
      *out = p;
      return 0;
    }
    // the stage does not fit in LDS: the fp32-input loop
  }
  if (view) return VRVQ_ERR_UNSUPPORTED;  // the phase-split view exists on the x3 loop only
  if (xw > 64 * win_per_row(ks, t.BN)) return VRVQ_ERR_UNSUPPORTED;  // window > staged lanes
  // a power-of-two stride stages its window split by phase, each phase padded on its own
  const bool phases = g.stride > 1 && (g.stride & (g.stride - 1)) == 0;
  const int xp = (xw + g.stride - 1) / g.stride;
  const int xwp = ((phases ? xp * g.stride : xw) + 3) & ~3;
  const long long lds = max2(conv_lds_bytes(ks, t.BM, t.BN, xwp), epi);
  if (lds > CONV_LDS_MAX) return VRVQ_ERR_UNSUPPORTED;
  p.lds = (int)lds;
  *out = p;
  return 0;
}

// Small-Cout conv (Cout <= 8, stride 1): conv_cout1_stream_kernel for the Cout = 1 k7 / k3
// layers whose 12-sample window it covers, else conv_small_cout_kernel.
inline int plan_small(const ConvShape& s, ConvPlan* out) {
  ConvPlan p{};
  p.path = PATH_SMALL_COUT;
  p.KS = s.k;
  long long nblk;
  if (s.M == 1 && s.dil == 1 && s.tin % 4 == 0 &&
      ((s.k == 7 && s.pad == 3) || (s.k == 3 && s.pad == 1))) {
    p.cout1_stream = true;
    nblk = (long long)s.batch * ((s.ng + 256 * C1_T - 1) / (256 * C1_T));
  } else {
    const long long lds = (long long)(SMALL_WMAX + SMALL_SC * (SMALL_BT + (s.k - 1) * s.dil)) * 4;
    if (lds > 64 * 1024) return VRVQ_ERR_UNSUPPORTED;
    p.lds = (int)lds;
    nblk = (long long)s.batch * ((s.ng + SMALL_BT - 1) / SMALL_BT);
  }
  if (nblk <= 0 || nblk > CONV_GRID_MAX) return VRVQ_ERR_ARG;
  p.grid = (int)nblk;
  *out = p;
  return 0;
}

// vrvq_conv1d / _ws / _proj. s: the call's shape (M = Cout, ng = Tout).
inline int plan_conv1d(const ConvShape& s, ConvPlan* out) {
  if (s.x3 && !x3_offsets_fit(s.tin, s.m_pad)) return VRVQ_ERR_UNSUPPORTED;
  const int snake_cin = s.snake ? s.cin : 0;
  if (s.x3 && s.stride > 1) {
    // strided conv on the x3 loop: a stride-1 k = 2 conv over the phase-split view of x
    // (conv_core.h ConvArgs::psh), k = 2 stride with a power-of-two stride
    if (s.k != 2 * s.stride || (s.stride & (s.stride - 1)) != 0 || s.pad >= s.stride)
      return VRVQ_ERR_UNSUPPORTED;
    ConvShape g = s;
    g.k = 2;
    g.cin = s.cin * s.stride, g.tin = s.ng + 1;
    g.stride = 1, g.pad = 0, g.dil = 1;
    return plan_mfma(g, true, snake_cin, out);
  }
  // the MFMA tiles' epilogue owns the projection: vrvq_conv1d_proj runs nothing else
  if (!s.proj && s.M <= SMALL_COUT && s.stride == 1 &&
      s.cin * s.k * (s.M == 1 ? 1 : SMALL_COUT) <= SMALL_WMAX)
    return plan_small(s, out);
  if (!s.proj && s.cin == 1 && s.k == 7 && s.stride == 1 && s.dil == 1 && !s.snake &&
      s.M % CI1_CG == 0 && s.ng % 4 == 0) {
    const long long nblk =
        (long long)s.batch * ((s.ng + 256 * CI1_T - 1) / (256 * CI1_T)) * (s.M / CI1_CG);
    if (nblk <= 0 || nblk > CONV_GRID_MAX) return VRVQ_ERR_ARG;
    ConvPlan p{};
    p.path = PATH_CIN1;
    p.KS = s.k;
    p.grid = (int)nblk;
    *out = p;
    return 0;
  }
  return plan_mfma(s, false, snake_cin, out);
}

// vrvq_conv_transpose1d / _pad. s: the polyphase GEMM (k = 2, M = Cout * up, ng = Tin + 1,
// stride / pad / dil = 1 / 1 / 1).
inline int plan_conv_transpose1d(const ConvShape& s, ConvPlan* out) {
  if (s.x3 && !x3_offsets_fit(s.tin, s.m_pad)) return VRVQ_ERR_UNSUPPORTED;
  return plan_mfma(s, false, s.snake ? s.cin : 0, out);
}

}  // namespace vrvq_conv
