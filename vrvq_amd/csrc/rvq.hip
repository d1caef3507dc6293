// Residual vector quantisation on gfx950: projection GEMM -> 8-dim chain -> HBM expansion.
//
// VBRResidualVectorQuantize.forward (models/quantize.py:328-443) runs, per frame and stage i
// (VectorQuantize.forward / decode_latents, :42-103):
//   z_e(i) = W_in(i) r_i + b_in(i),     r_i = z - sum_{j<i} z_q_j,   z_q_j = W_out(j) zst_j + b_out(j)
//   idx    = argmin_n (sum e^2 - 2 e.cbn_n) + sum cbn_n^2,  e = z_e / max(|z_e|, 1e-12)
//   zst_i  = z_e + (cb[idx] - z_e)                               (straight-through value)
// By linearity z_e(i) = ((P_i + b_in(i)) - Qb_i) - sum_{j<i} M_ij zst_j with P_i = W_in(i) z,
// M_ij = W_in(i) W_out(j) (8x8) and Qb_i = W_in(i) sum_{j<i} b_out(j): the sequential part
// lives in the 8-dim latent space and the 1024-dim work becomes two embarrassingly parallel
// streams. The quantizer is ONE launch from the in_proj partials (rvq_pt_kernel: chain parts +
// expansion workgroups that write z_q_is / z_q under the chain). The eval encode gets the
// partials from the encoder's last conv, which computes them in its epilogue (conv.hip
// vrvq_conv1d_proj); on channel-major z (vrvq_rvq_encode) rvq_project3_kernel writes the same
// partials first. rvq_pt_kernel's chain parts run the body of the three-launch form, which stays
// as the reference path:
//
//   rvq_project3_kernel  P partials over 8 channel splits (one workgroup per clip x 96-frame
//                        tile x split, the z slab staged once in LDS; split-bf16 MFMA).
//   rvq_chain_kernel     the chain: <= 16 frames per workgroup, 8 waves; wave w scans its
//                        N/8 codes for all frames at once on the matrix cores (16-code x
//                        16-frame MFMA tiles), then 8 (frame, k) lane groups finish the stage
//                        (cross-wave argmin, raw codeword, loss, projected residual, next z_e)
//                        — two barriers per stage, no global stores until the end.
//   rvq_expand_kernel    z_q_is[b,i,:,:] = W_out(i) zst_i + b_out(i) and the masked sum z_q on
//                        the matrix cores (32-channel x 32-frame tiles): the HBM write stream,
//                        with no LDS and a few VALU per element.
//
// The distance is the reference's fp32 expression (dot in k order, fma(d, -2, e2) + c2, lowest
// index on ties); the projection on the split-bf16 matrix cores (x3) is fp32-accurate but not
// the reference's summation order, so the codes match every golden fixture BY TEST (full
// batches included), not by construction: a near-tie could differ.
//
// The host side reads no environment variable. The launch geometry of both entry points (frames
// per chain part, parts, expansion windows, LDS, clips per launch, workspace) is one RvqPlan
// (rvq_plan), shared by the launcher, vrvq_rvq_workspace_part, vrvq_rvq_fused_clips and the
// host-only query vrvq_rvq_plan; the kernels of a codebook size come from one table (rvq_kernels).
#include <hip/hip_ext.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "lanes.h"

#ifdef VRVQ_STAMPS
// rvq_pt_kernel, diagnostic build: thread 0 of every workgroup records
// s_memrealtime (100 MHz, one clock for the whole chip) at its phase boundaries into
// stamps[blockIdx][64] (tools/rvq_fused_stamps.py).
#define FSTAMP(buf, slot)                                                                    \
  do {                                                                                     \
    if ((buf) && threadIdx.x == 0)                                                         \
      (buf)[(size_t)blockIdx.x * 64 + (slot)] = __builtin_amdgcn_s_memrealtime();          \
  } while (0)
// ... by thread t of the workgroup (the pt expansion's loader wave)
#define FSTAMPT(buf, slot, t)                                                                \
  do {                                                                                     \
    if ((buf) && threadIdx.x == (t))                                                       \
      (buf)[(size_t)blockIdx.x * 64 + (slot)] = __builtin_amdgcn_s_memrealtime();          \
  } while (0)
#else
#define FSTAMP(buf, slot) do {} while (0)
#define FSTAMPT(buf, slot, t) do {} while (0)
#endif

namespace {

constexpr int RD = 1024;        // latent channels
constexpr int RCD = 8;          // codebook_dim
constexpr int PJ_SPLIT = 8;     // channel splits of the projection GEMM
constexpr int PJ_CPS = RD / PJ_SPLIT;
constexpr int CH_NT = 512;      // chain threads (8 waves)
constexpr int CH_NW = CH_NT / 64;
constexpr int CH_FMAX = 16;     // frames per chain workgroup
constexpr int CH_NQMAX = 32;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;
constexpr int CPOL_SC1 = 16;    // buffer load / store aux: sc1 (L1 bypass, write-through)
constexpr int RSRC_FLAGS = 0x00020000;  // raw buffer descriptor word 3 (gfx950)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ------------------------------------------------------------------------------------------
// Prep (once per weight version, like the weight-norm fold):
//   mcol[j][i][k][m] = sum_c W_in(i)[k][c] W_out(j)[c][m] for i > j (else 0)   (this kernel)
//   qb[i][k]         = sum_c W_in(i)[k][c] (sum_{j<i} b_out(j)[c])   (cross_prep_qb_kernel)
// one fmaf chain over c in order per output. Acc = float is the inference path's; Acc = double
// (vrvq_rvq_cross_prep_precise, the training step) rounds each entry once: the entries are
// cancelling 1024-term dots, and the fp32 chain's 1e-6 of |M| is 4 - 10 x fp32's own error in
// the quantizer's weight gradients (DESIGN, "What the quantizer's training backward ...").
__device__ __forceinline__ float cp_fma(float a, float b, float acc) { return fmaf(a, b, acc); }
__device__ __forceinline__ double cp_fma(double a, double b, double acc) { return fma(a, b, acc); }

template <typename Acc>
__global__ void cross_prep_kernel(const float* __restrict__ w_in_t,  // [nq][D][8]
                                  const float* __restrict__ w_out,   // [nq][D][8]
                                  const float* __restrict__ b_out,   // [nq][D]
                                  int nq, float* __restrict__ mcol, float* __restrict__ qb) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nm = nq * nq * 64;
  if (e < nm) {
    const int m = e & 7, k = (e >> 3) & 7, ij = e >> 6;
    const int i = ij % nq, j = ij / nq;
    Acc acc = 0;
    if (i > j) {
      const float* wi = w_in_t + (size_t)i * RD * RCD + k;
      const float* wo = w_out + (size_t)j * RD * RCD + m;
      for (int c = 0; c < RD; ++c) acc = cp_fma((Acc)wi[c * RCD], (Acc)wo[c * RCD], acc);
    }
    mcol[e] = (float)acc;
  }
}

// qb with the bias prefix sums shared: workgroup = stage i; thread c forms
// bs[c] = sum_{j<i} b_out(j)[c] (left to right) into LDS, then 8 lanes run the k-th fmaf chain
// over c in order -- the values of the earlier one-thread-per-output form, which re-summed the
// biases for every channel in each of its nq * 8 threads (O(nq^2 D) serial work: ~1 ms per
// weight version at nq = 28, i.e. every training step).
template <typename Acc>
__global__ __launch_bounds__(RD) void cross_prep_qb_kernel(const float* __restrict__ w_in_t,
                                                           const float* __restrict__ b_out,
                                                           float* __restrict__ qb) {
  __shared__ Acc bs_s[RD];
  const int i = blockIdx.x, c = threadIdx.x;
  Acc bs = 0;
  for (int j = 0; j < i; ++j) bs = bs + b_out[(size_t)j * RD + c];
  bs_s[c] = bs;
  __syncthreads();
  if (c < RCD) {
    const float* wi = w_in_t + (size_t)i * RD * RCD + c;
    Acc acc = 0;
    for (int cc = 0; cc < RD; ++cc) acc = cp_fma((Acc)wi[cc * RCD], bs_s[cc], acc);
    qb[i * RCD + c] = (float)acc;
  }
}

// ------------------------------------------------------------------------------------------
// Prep: the normalised codebooks in the chain's MFMA A-fragment order, so that every lane loads
// its stage operands as contiguous float4:
//   cbf[i][w][l][t][kh] = cbn[i][w*N/8 + 16 t + (l & 15)][4 kh + (l >> 4)]
// (wave w of the chain owns codes [w N/8, (w+1) N/8) as N/128 tiles of 16 codes).
__global__ void rvq_frag_kernel(const float* __restrict__ cbn, int nq, int N,
                                float* __restrict__ cbf) {
  const size_t total = (size_t)nq * N * RCD;
  const int NT = N / 128;
  for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total;
       o += (size_t)gridDim.x * blockDim.x) {
    const int kh = (int)(o % 2);
    size_t r = o / 2;
    const int t = (int)(r % NT);
    r /= NT;
    const int l = (int)(r % 64);
    r /= 64;
    const int w = (int)(r % CH_NW);
    const int i = (int)(r / CH_NW);
    const int code = w * (N / CH_NW) + 16 * t + (l & 15);
    cbf[o] = cbn[((size_t)i * N + code) * RCD + 4 * kh + (l >> 4)];
  }
}

// ------------------------------------------------------------------------------------------
// Projection: part[s][n][r] = sum_{c in split s} W_in_t[r/8][c][r%8] z[b][c][t], n = b*T + t,
// r < R = nq*8. One workgroup of 8 waves per (clip, frame tile of <= 96, channel split): it reads
// its z slab [128 ch][<= 96 t] from HBM once and keeps it in LDS for every 16-row tile of the
// stage rows; the w_in_t operands go straight to registers. 256 workgroups at configs[1]
// (32 clips x 8 splits): one per CU, no second round.
constexpr int PJ_NT = 512;
constexpr int PJ_TC = 96;                       // frames per tile (6 MFMA column tiles)

// One (clip b, frame tile tc, channel split s) projection unit on the bf16 matrix cores: both
// operands split exactly into three bf16 terms and the six products of conv_x3.h (dropped terms
// <= 2^-23 |ab|: fp32 accuracy) on v_mfma_f32_16x16x32_bf16 -- 2.7x the fp32 MFMA rate for the
// GEMM that bounds the projection (64 rows x 128 channels x 96 frames per unit). The z slab goes to LDS transposed, as three
// bf16 planes [plane][frame][channel] (rows of 128 channels + 8 pad: conflict-free 16-B B
// reads); the W_in rows (8 channels per lane, L2) are split in registers.
constexpr int PJ3_LDB = 136;                     // bf16 per frame row (272 B)
constexpr int PJ3_PLANE = PJ_TC * PJ3_LDB * 2;  // bytes per plane
constexpr int PJ3_LDS = 3 * PJ3_PLANE;           // 78,336 B

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// v = h + m + l exactly (RNE at each step), two values per call (conv_x3.h split3x2)
__device__ __forceinline__ void rvq_split3x2(float v0, float v1, unsigned& h, unsigned& m,
                                             unsigned& l) {
  const f32x2 v = {v0, v1};
  const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 hf = {__uint_as_float(hu << 16), __uint_as_float(hu & 0xffff0000u)};
  const f32x2 r = v - hf;
  const unsigned mu = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
  const f32x2 mf = {__uint_as_float(mu << 16), __uint_as_float(mu & 0xffff0000u)};
  const f32x2 s = r - mf;
  h = hu;
  m = mu;
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(s, bf16x2));
}

__device__ __forceinline__ f32x4 mfma16_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__global__ __launch_bounds__(PJ_NT) void rvq_project3_kernel(const float* __restrict__ z, int T,
                                                              int nq, int n_tc,
                                                              const float* __restrict__ w_in_t,
                                                              float* __restrict__ part, int NF) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tc = blockIdx.x % n_tc, b = blockIdx.x / n_tc, s = blockIdx.y;
  constexpr int NIT = (PJ_CPS / 8) * PJ_TC / PJ_NT;  // (octet, frame) items per thread: 3
  constexpr int NKS = PJ_CPS / 32;                      // K steps of 32 channels
  const int R = nq * RCD;
  const int t0 = tc * PJ_TC;
  const int ntl = min(PJ_TC, T - t0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_rt = (R + 15) / 16;
  const int lr = lane & 15, kg = lane >> 4;
  // A operands of a work item (16-row tile rt): row r = 16 rt + lr, channels 32 ks + 8 kg .. +7
  // of the split (w_in_t[stage][c][k]); rows >= R zeroed
  auto load_w = [&](int rt, float (&w)[NKS][8]) {
    const int r = rt * 16 + lr;
    const unsigned rm = 0u - (unsigned)(r < R);
    const float* wp = w_in_t + ((size_t)min(r >> 3, nq - 1) * RD + s * PJ_CPS + 8 * kg) * RCD + (r & 7);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        w[ks][u] = __uint_as_float(__float_as_uint(wp[(size_t)(32 * ks + u) * RCD]) & rm);
  };
  float w[NKS][8];
  // the first item's weights (L2) first: their latency runs under the z slab's
  load_w(min(wave, 2 * n_rt - 1) >> 1, w);
  const float* zb = z + ((size_t)b * RD + s * PJ_CPS) * T + t0;
  {  // the slab: every load in flight, then split and stored transposed
    float zv[NIT][8];
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int e = tid + PJ_NT * q;
      const int o = e / PJ_TC, t = e - o * PJ_TC;
#pragma unroll
      for (int u = 0; u < 8; ++u) zv[q][u] = zb[(size_t)(8 * o + u) * T + min(t, ntl - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int e = tid + PJ_NT * q;
      const int o = e / PJ_TC, t = e - o * PJ_TC;
      const unsigned m = 0u - (unsigned)(t < ntl);
      unsigned h[4], mm[4], l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        rvq_split3x2(__uint_as_float(__float_as_uint(zv[q][2 * u]) & m),
                     __uint_as_float(__float_as_uint(zv[q][2 * u + 1]) & m), h[u], mm[u], l[u]);
      char* d = lds + t * (PJ3_LDB * 2) + o * 16;
      *reinterpret_cast<u32x4*>(d) = u32x4{h[0], h[1], h[2], h[3]};
      *reinterpret_cast<u32x4*>(d + PJ3_PLANE) = u32x4{mm[0], mm[1], mm[2], mm[3]};
      *reinterpret_cast<u32x4*>(d + 2 * PJ3_PLANE) = u32x4{l[0], l[1], l[2], l[3]};
    }
  }
  // a use of the weights here keeps their loads ahead of the slab's (else they are sunk below
  // the barrier and waited for one K step at a time)
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" ::"v"(w[ks][u]));
  __syncthreads();
  // work items (16-row tile rt, half hf = frame tiles 3 hf .. 3 hf + 2) over the 8 waves
  for (int item = wave; item < 2 * n_rt; item += PJ_NT / 64) {
    const int rt = item >> 1, hf = item & 1;
    if (item != wave) load_w(rt, w);
    f32x4 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      unsigned h[4], mm[4], l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) rvq_split3x2(w[ks][2 * u], w[ks][2 * u + 1], h[u], mm[u], l[u]);
      const u32x4 ah = {h[0], h[1], h[2], h[3]}, am = {mm[0], mm[1], mm[2], mm[3]},
                  al = {l[0], l[1], l[2], l[3]};
      // the three column tiles' products interleaved (three independent accumulators: the
      // matrix core is not left waiting on a dependent MFMA); per tile the order stays
      // m m, h l, l h, h m, m h, h h
      u32x4 bh[3], bm[3], bl[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const char* bp = lds + ((3 * hf + j) * 16 + lr) * (PJ3_LDB * 2) + (32 * ks + 8 * kg) * 2;
        bh[j] = *reinterpret_cast<const u32x4*>(bp);
        bm[j] = *reinterpret_cast<const u32x4*>(bp + PJ3_PLANE);
        bl[j] = *reinterpret_cast<const u32x4*>(bp + 2 * PJ3_PLANE);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(am, bm[j], acc[j]);  // m m
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(ah, bl[j], acc[j]);  // h l
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(al, bh[j], acc[j]);  // l h
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(ah, bm[j], acc[j]);  // h m
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(am, bh[j], acc[j]);  // m h
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = mfma16_bf16(ah, bh[j], acc[j]);  // h h
      __builtin_amdgcn_sched_barrier(0);  // one K step's operands live at a time
    }
    // D layout: lane l, reg q -> row 4 (l >> 4) + q of the tile, frame l & 15
    const int rr = rt * 16 + 4 * kg;  // rows rr..rr+3 all valid iff rr < R (R = 8 nq)
    if (rr < R) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int t = (3 * hf + j) * 16 + lr;
        if (t < ntl) {
          const size_t n = (size_t)b * T + t0 + t;
          *reinterpret_cast<float4*>(part + ((size_t)s * NF + n) * R + rr) =
              make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The chain. Workgroup = frames [n0, n0 + nf) of the flattened (b, t) axis, nf <= 16; 8 waves.
//
// Stage i, S1 (all waves):
//   - deferred U updates: pu[f][ip] -= M_{ip,i-1} zst_{i-1} for ip > i (spread over all threads,
//     issued after the candidate-row gather so they run under its L2 latency; ip = i was done on
//     the critical path in S2 of stage i-1);
//   - distance scan on the matrix cores: wave w owns codes [w N/8, (w+1) N/8) as 16-code tiles;
//     D[code][frame] = cbn . e by two v_mfma_f32_16x16x4_f32 per tile (k = 0..3, then 4..7 on
//     the same accumulator: the k-ordered fma chain of the reference's dot, bitwise), then per
//     lane dist = fma(D, -2, e2) + c2 over its 32 (code, frame) entries in code order, and a
//     lexicographic (dist, code) min across the 4 lanes of each frame -> per-wave candidate;
//   - per wave and frame, the candidate's raw codebook row (gathered from L2 into LDS);
//   - prefetches of stage i+1 (cbn fragments -> registers; c2 slice and M_{.,i+1} ->
//     registers, stored to LDS at the start of stage i+1).
// S2 (lanes (f, k), f < nf, tid = 8 f + k): cross-wave argmin (wave order = code order, lowest
// code on ties), the winner's raw codeword, loss, zst, the next stage's pu[f][i+1] and z_e.
// One workgroup per CU: F = ceil(B*T / 256) frames each (<= 16).
// Two barriers per stage; outputs stay in LDS until the epilogue.
struct ChainArgs {
  const float* part;   // [8][NFS][nq*8]
  int B, T, nq, F, NF;
  int NFS;             // split stride of part in frames (the three-launch path: NF;
                       // rvq_pt_kernel: the frames of the whole call)
  const float* b_in;   // [nq][8]
  const float* qb;     // [nq][8]
  const float* mcol;   // [nq][nq][8][8]
  const float* cb;     // [nq][N][8]
  const float* cbf;    // [nq][8][64][N/128][2] normalised codebook, fragment order
  const float* c2;     // [nq][N]
  const float* imp;    // [B][T] or null
  float level;
  int64_t* codes;      // [B][nq][T]
  float* latents;      // [B][nq*8][T]
  float* loss_pf;      // [B][nq][T]
  float* zst;          // [B][nq][T][8]
  float* mask;         // [B][nq][T] or null
  unsigned long long* stamps;  // diagnostic build only (-DVRVQ_STAMPS): [grid][nq + 1][2][8]
};

#ifdef VRVQ_STAMPS
// In-kernel s_memtime stamps (diagnostic build): lanes 0 of waves 0 and 7 record 8 points per
// stage into a buffer nothing else reads.
#define CSTAMP(stage, step)                                                                  \
  do {                                                                                     \
    if (a.stamps && (tid == 0 || tid == 448)) {                                            \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();                          \
      a.stamps[(((size_t)blockIdx.x * (a.nq + 1) + (stage)) * 2 + (tid ? 1 : 0)) * 8 +      \
               (step)] = t_;                                                               \
    }                                                                                      \
  } while (0)
#else
#define CSTAMP(stage, step) do {} while (0)
#endif

// LDS carve (floats), shared by the launcher's size computation.
struct ChainLds {
  int e, e2, cd, ci, cr, pu, lat, zs, code, loss, c2, m, total;
  __host__ __device__ ChainLds(int nq, int F, int N) {
    auto al = [](int x) { return (x + 3) & ~3; };
    int o = 0;
    e = o; o += al(CH_FMAX * RCD);
    e2 = o; o += al(CH_FMAX);
    cd = o; o += al(CH_FMAX * CH_NW);
    ci = o; o += al(CH_FMAX * CH_NW);
    cr = o; o += al(CH_FMAX * CH_NW * RCD);
    pu = o; o += al(F * nq * RCD);
    lat = o; o += al(F * nq * RCD);
    zs = o; o += al(F * nq * RCD);
    code = o; o += al(F * nq);
    loss = o; o += al(F * nq);
    c2 = o; o += al(2 * N);
    m = o; o += al(3 * nq * 64);
    total = o;
  }
};

// ------------------------------------------------------------------------------------------
// The in-launch hand-off of rvq_pt_kernel (chain parts -> expansion workgroups): tagged 8-B
// granules {value, tag}, each written whole by ONE sc1 store and read with 16-B sc1 loads (two
// granules); the reader checks the tag of every granule it uses and re-reads until it matches,
// so the data is its own flag -- no drain, no flag word (cdna_hip_programming.md Guideline 16,
// R2; MI355X_MICROARCH.md: granules are observed untorn, also as 16-B sc1 halves). Stage i's zst
// carries tag 64 epoch + i + 1; epochs grow per call, so an older call's granules never match
// (under stream capture the granule area is zeroed by a memset node and the call uses epoch 1).
// The sync block holds only the error word of the bounded waits.
constexpr unsigned SPIN_MAX = 1u << 19;  // bounded spins (~0.5 s); on the bound: *err = code

// A bounded wait that ran out (a hang averted: it cannot happen with the whole grid resident)
// records its code in the stream's sync block (vrvq_rvq_sync_error) and in the process's
// host-mapped error word (system scope: the host reads it without synchronising, and the next
// vrvq_rvq_encode* call / torch op raises on it: vrvq_rvq_pending_error). The only wait is the
// expansion's for a stage (code 2; code 1 was the retired r04 kernel's wait for its partials);
// the workgroup then writes NaN z_q / z_q_is instead of publishing garbage as valid data.
__device__ __forceinline__ void report_timeout(unsigned* err, unsigned* err_host, unsigned code) {
  __hip_atomic_store((gu32*)err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (err_host)
    __hip_atomic_store((gu32*)err_host, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct ChainHandoff {              // rvq_pt_kernel's chain parts only
  unsigned epoch;
  unsigned long long* zsh;         // this part's stage-0 block of tagged zst granules
  int zsh_stage;                   // granules per stage
  unsigned long long* stamps;      // diagnostic build only
  int dbg;                         // diagnostic build only: FusedArgs::dbg
};

// A chain part gets pu = (P + b_in) - Qb of its frames from the 8 split partials (plain loads
// after the kernel that wrote them: rvq_project3_kernel or the encoder's last conv,
// vrvq_conv1d_proj). FUSED: a chain part of rvq_pt_kernel, which publishes every stage's zst to
// the expansion workgroups of its launch; else rvq_chain_kernel, whose outputs leave at the end.
template <int NM, bool FUSED>
__device__ __forceinline__ void chain_body(const ChainArgs& a, float* sm, int n0, int nf,
                                           const ChainHandoff& hx) {
  constexpr int N = 256 * NM;
  constexpr int NPW = N / CH_NW;   // codes per wave
  constexpr int NT = NPW / 16;     // 16-code MFMA tiles per wave
  const int nq = a.nq, F = a.F;
  const ChainLds L(nq, F, N);
  float* e_s = sm + L.e;
  float* e2_s = sm + L.e2;
  float* cd_s = sm + L.cd;
  int* ci_s = reinterpret_cast<int*>(sm + L.ci);
  float* cr_s = sm + L.cr;      // [16][8 waves][8]: raw codebook row of each wave's candidate
  float* pu_s = sm + L.pu;      // [F][nq][8]: ((P + b_in) - Qb) - U
  float* lat_s = sm + L.lat;    // [F][nq][8]: z_e (output)
  float* zs_s = sm + L.zs;      // [F][nq][8]: zst (output, and the U updates' input)
  int* code_s = reinterpret_cast<int*>(sm + L.code);
  float* loss_s = sm + L.loss;
  float* c2_s = sm + L.c2;      // [2][N]
  float* m_s = sm + L.m;        // [3][nq][8][8]: M_{.,j} for j = i-1, i, i+1 (mod 3)

  const int R = nq * RCD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rf = tid >> 3, rk = tid & 7;  // S2 roles: (frame, k)
  const bool role = rf < nf;
  const int fl = lane & 15, lg = lane >> 4;  // MFMA roles: frame column, k / row group
  const int cw = wave * NPW;
  CSTAMP(nq, 0);

  // stage 0's operands first: they do not depend on the partials
  for (int e = tid; e < CH_FMAX * RCD; e += CH_NT) e_s[e] = 0.0f;
  for (int e = tid; e < CH_FMAX; e += CH_NT) e2_s[e] = 0.0f;
  float av[NT][2];  // cbn fragments of the current stage: code cw + 16 t + fl, k = 4 kh + lg
  auto load_a = [&](int i, float (&dst)[NT][2]) {  // NT / 2 contiguous float4 per lane
    const float* src = a.cbf + (((size_t)i * CH_NW + wave) * 64 + lane) * (2 * NT);
#pragma unroll
    for (int q = 0; q < NT / 2; ++q) {
      const float4 v = ld4(src + 4 * q);
      dst[2 * q][0] = v.x; dst[2 * q][1] = v.y; dst[2 * q + 1][0] = v.z; dst[2 * q + 1][1] = v.w;
    }
  };
  load_a(0, av);
  for (int e = tid; e < N; e += CH_NT) c2_s[e] = a.c2[e];
  if (nq > 1)
    for (int e = tid; e < R * RCD / 4; e += CH_NT)
      reinterpret_cast<float4*>(m_s)[e] = ld4(a.mcol + (size_t)e * 4);
  // ---- prologue: pu = (P + b_in) - Qb (partials summed in split order); stage 0 operands.
  // no wait is left in a chain part, so nothing sets this: it stays only so that rvq_pt_kernel
  // compiles to the code it had with the r04 kernel beside it (its poison arm below is dead)
  __shared__ int dead_s;
  if (tid == 0) dead_s = 0;
  // Two (frame, row) items per thread per pass with all 16 partial loads in flight.
  for (int e0 = tid; e0 < nf * R; e0 += 2 * CH_NT) {
    float v[2][PJ_SPLIT];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = e0 + h * CH_NT;
      const size_t base = (size_t)n0 * R + (e < nf * R ? e : 0);
#pragma unroll
      for (int sp = 0; sp < PJ_SPLIT; ++sp) v[h][sp] = a.part[(size_t)sp * a.NFS * R + base];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = e0 + h * CH_NT;
      if (e < nf * R) {
        const int r = e % R;
        float pv = v[h][0];
#pragma unroll
        for (int sp = 1; sp < PJ_SPLIT; ++sp) pv = pv + v[h][sp];
        pu_s[e] = (pv + a.b_in[r]) - a.qb[r];
      }
    }
  }
  __syncthreads();
  float ze = 0.0f;  // S2 lanes: z_e of (rf, rk) at the current stage
  auto set_e = [&](float zv) {  // F.normalize (eps 1e-12) of the 8-lane group's z_e
    ze = zv;
    const float n2 = vrvq::sum8(ze * ze, lane);
    const float e = ze / fmaxf(sqrtf(n2), 1e-12f);
    const float e2 = vrvq::sum8(e * e, lane);
    if (role) {
      e_s[rf * RCD + rk] = e;
      if (rk == 0) e2_s[rf] = e2;
    }
  };
  set_e(role ? pu_s[(rf * nq) * RCD + rk] : 0.0f);
  __syncthreads();
  CSTAMP(nq, 1);
  if constexpr (FUSED) FSTAMP(hx.stamps, 3);

  // next stage's c2 slice / M column: loaded during a stage, stored to LDS at the start of the
  // next (no wait on a load issued in the same stage)
  constexpr int C2W = (NPW + 63) / 64;
  float c2n[C2W];
  float4 mn = make_float4(0.f, 0.f, 0.f, 0.f);
  // fused: waves 0-1 = frames 0..15 x k publish the part's 16-frame block of a stage as tagged
  // 8-B granules {zst, 64 epoch + i + 1} (one sc1 store each: the data is its own flag, no
  // drain, no flag word), k = 2 s + h at slot 4 h + s of the frame (a consumer lane's four k
  // values are 32 contiguous bytes); frames >= nf store 0 with the tag
  auto publish = [&](int st, float v) {
    if (wave < 2) {
      const unsigned long long g =
          ((unsigned long long)(hx.epoch * 64u + (unsigned)st + 1u) << 32) | __float_as_uint(v);
      __hip_atomic_store((gu64*)(hx.zsh + (size_t)st * hx.zsh_stage +
                                 (rf * 8 + (rk & 1) * 4 + (rk >> 1))),
                         g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  for (int i = 0; i < nq; ++i) {
    const bool more = i + 1 < nq;
    // ---- S1 ----
    CSTAMP(i, 0);
    if (i > 0) {
      // stage i operands prefetched during stage i-1: M_{.,i} (read by other waves after
      // barrier 1) and this wave's c2 slice (read by this wave only)
#pragma unroll
      for (int q = 0; q < C2W; ++q)
        if (lane + 64 * q < NPW) c2_s[(i & 1) * N + cw + lane + 64 * q] = c2n[q];
      if (i + 1 < nq && tid * 4 < R * RCD)
        reinterpret_cast<float4*>(m_s + (i % 3) * R * RCD)[tid] = mn;
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the c2 slice is in LDS for the scan
    }
    // deferred U updates from stage i-1 for targets ip > i (needed from S2 of this stage on):
    // run after the scan has issued its candidate-row gather, under that L2 latency
    auto deferred_updates = [&]() {
      if (i == 0) return;
      const int nip = nq - 1 - i;
      const float* mj = m_s + ((i - 1) % 3) * R * RCD;
      for (int e = tid; e < nf * nip * RCD; e += CH_NT) {
        const int k = e & 7, q = e >> 3;
        const int f = q / nip, ip = i + 1 + (q - f * nip);
        const float* zr = zs_s + (f * nq + (i - 1)) * RCD;
        const float* mr = mj + (ip * RCD + k) * RCD;
        float* pp = pu_s + (f * nq + ip) * RCD + k;
        *pp = *pp - dot8(ld4(mr), ld4(mr + 4), ld4(zr), ld4(zr + 4));
      }
    };
    CSTAMP(i, 1);
    float an[NT][2];
    CSTAMP(i, 2);
    {
      // distance scan: 16 frames x NT 16-code tiles, K = 8 as two k-quads. All MFMAs first
      // (NT independent accumulators), c2 read before them; then 4 independent argmin chains
      // (one per accumulator row r: codes cw + 16 t + 4 lg + r in increasing t) merged
      // lexicographically (dist, code) -- the same result as one chain in code order.
      const float b0 = e_s[fl * RCD + lg], b1 = e_s[fl * RCD + 4 + lg];
      const float e2 = e2_s[fl];
      const float* c2c = c2_s + (i & 1) * N + cw + 4 * lg;
      float4 cc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) cc[t] = ld4(c2c + t * 16);
      f32x4 d[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][0], b0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      float bst[4];
      int bix[4];  // 16 t of the best entry (a constant per entry: no per-entry index add)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bst[r] = INFINITY;
        bix[r] = 0;
      }
      const f32x2 m2 = {-2.0f, -2.0f}, e22 = {e2, e2};
      auto amin_tile = [&](int t) {
        // (sum e^2 - 2 e.c) + sum c^2 with the first step as fma(d, -2, e2): 2d is exact,
        // so this is the reference's rounding (models/quantize.py:96-100); two entries per
        // packed fma / add (v_pk_fma_f32, v_pk_add_f32: the same per-element roundings)
        const f32x2 d01 = {d[t][0], d[t][1]}, d23 = {d[t][2], d[t][3]};
        const f32x2 c01 = {cc[t].x, cc[t].y}, c23 = {cc[t].z, cc[t].w};
        const f32x2 s01 = __builtin_elementwise_fma(d01, m2, e22) + c01;
        const f32x2 s23 = __builtin_elementwise_fma(d23, m2, e22) + c23;
        const float dist[4] = {s01.x, s01.y, s23.x, s23.y};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool take = dist[r] < bst[r];  // increasing code index: strict < keeps the first
          bst[r] = take ? dist[r] : bst[r];
          bix[r] = take ? t * 16 : bix[r];
        }
      };
      // the second k-quad of tile t, then the argmin of tile t - 1 (whose MFMAs are done): the
      // compare / select VALU of one tile issues while the matrix core runs the next tile
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][1], b1, d[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (t > 0) amin_tile(t - 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      amin_tile(NT - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) bix[r] += cw + 4 * lg + r;
      vrvq::amin(bst[0], bix[0], bst[1], bix[1]);
      vrvq::amin(bst[2], bix[2], bst[3], bix[3]);
      vrvq::amin(bst[0], bix[0], bst[2], bix[2]);
      float best = bst[0];
      int bidx = bix[0];
      vrvq::amin(best, bidx, vrvq::xchg<16>(best, lane), vrvq::xchg<16>(bidx, lane));
      vrvq::amin(best, bidx, vrvq::xchg<32>(best, lane), vrvq::xchg<32>(bidx, lane));
      // the candidate's raw codebook row (L2 gather, models/quantize.py:101-103): only the
      // wave's own candidates, so no per-stage staging of the whole raw codebook (measured: an
      // LDS copy of the stage's codebook, prefetched a stage ahead, is slower -- the gather's
      // latency hides behind the other wave of the SIMD). Issued before the next stage's
      // prefetch, so the wait for it does not cover the prefetch.
      const float* row = a.cb + ((size_t)i * N + (lane < nf ? bidx : 0)) * RCD;
      const float4 r0 = ld4(row), r1 = ld4(row + 4);
      __builtin_amdgcn_sched_barrier(0);  // keep the gather ahead of the prefetch (vmcnt order)
      {  // stage i+1 operands (cbn fragments, c2 slice, M column). Unconditional loads from
         // clamped addresses (the last stage re-reads its own): a branch around them makes the
         // waitcnt pass assume none are outstanding at the join, so the candidate-row wait
         // below would drain the whole prefetch.
        const int in = more ? i + 1 : i;
#ifdef VRVQ_STAMPS
        if (FUSED && (hx.dbg & 2)) {  // timing experiment: no per-stage codebook stream
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            an[t][0] = av[t][0];
            an[t][1] = av[t][1];
          }
        } else
#endif
        load_a(in, an);
#pragma unroll
        for (int q = 0; q < C2W; ++q)
          c2n[q] = a.c2[(size_t)in * N + cw + min(lane + 64 * q, NPW - 1)];
        // M_{.,i+1}: needed from stage i+1 on (stored only when i + 2 < nq)
        mn = ld4(a.mcol + (size_t)min(i + 1, nq - 1) * R * RCD + min(tid * 4, R * RCD - 4));
      }
      deferred_updates();
      if (lane < nf) {
        cd_s[lane * CH_NW + wave] = best;
        ci_s[lane * CH_NW + wave] = bidx;
        float* crw = cr_s + (lane * CH_NW + wave) * RCD;
        *reinterpret_cast<float4*>(crw) = r0;
        *reinterpret_cast<float4*>(crw + 4) = r1;
      }
    }
    CSTAMP(i, 3);
    __syncthreads();  // ------------------------------- candidates, stage i+1's c2 / M ready
    CSTAMP(i, 4);
    // ---- S2 (role lanes) ----
    int bi = 0;
    float zq = 0.0f;
    if (role) {
      const float4 d0 = ld4(cd_s + rf * CH_NW), d1 = ld4(cd_s + rf * CH_NW + 4);
      const int4 i0 = *reinterpret_cast<const int4*>(ci_s + rf * CH_NW);
      const int4 i1 = *reinterpret_cast<const int4*>(ci_s + rf * CH_NW + 4);
      const float dv[CH_NW] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
      const int iv[CH_NW] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
      float bd = dv[0];
      bi = iv[0];
      int bw = 0;
#pragma unroll
      for (int w = 1; w < CH_NW; ++w) {  // wave order = code order: strict < keeps the lowest
        const bool take = dv[w] < bd;
        bd = take ? dv[w] : bd;
        bi = take ? iv[w] : bi;
        bw = take ? w : bw;
      }
      bi = (bi >= 0 && bi < N) ? bi : 0;
      zq = cr_s[(rf * CH_NW + bw) * RCD + rk];  // raw codebook row of the winner
    }
    const float zsv = ze + (zq - ze);  // z_e + (z_q - z_e).detach(), models/quantize.py:73-75
    if constexpr (FUSED) publish(i, zsv);
    const float diff = ze - zq;
    const float l2 = vrvq::sum8(diff * diff, lane);
    if (role) {
      lat_s[(rf * nq + i) * RCD + rk] = ze;
      zs_s[(rf * nq + i) * RCD + rk] = zsv;
      if (rk == 0) {
        code_s[rf * nq + i] = bi;
        loss_s[rf * nq + i] = l2 / 8.0f;  // mse over codebook_dim, models/quantize.py:69-71
      }
    }
    CSTAMP(i, 5);
    if (more) {
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this group's zst row is in LDS
      float zn = 0.0f;
      if (role) {
        const float* zr = zs_s + (rf * nq + i) * RCD;
        const float* mr = m_s + (i % 3) * R * RCD + ((i + 1) * RCD + rk) * RCD;
        float* pp = pu_s + (rf * nq + i + 1) * RCD + rk;
        zn = *pp - dot8(ld4(mr), ld4(mr + 4), ld4(zr), ld4(zr + 4));
        *pp = zn;
      }
      set_e(zn);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        av[t][0] = an[t][0];
        av[t][1] = an[t][1];
      }
    }
    CSTAMP(i, 6);
    __syncthreads();  // ------------------------------------------------- next stage's e
    CSTAMP(i, 7);
    if constexpr (FUSED) FSTAMP(hx.stamps, 4 + i);
  }
  CSTAMP(nq, 2);

  // ---- epilogue: outputs of every stage (LDS -> HBM); poisoned after a timed-out wait
  const bool dead = FUSED && dead_s != 0;
  for (int e = tid; e < nf * nq * RCD; e += CH_NT) {
    // zst [b][i][t][k] and latents [b][i*8+k][t]
    const int k = e & 7, fi = e >> 3;
    const int i = fi / nf, f = fi - i * nf;
    const int n = n0 + f, b = n / a.T, t = n - b * a.T;
    if (a.zst) a.zst[(((size_t)b * nq + i) * a.T + t) * RCD + k] = zs_s[(f * nq + i) * RCD + k];
    a.latents[(((size_t)b * nq + i) * RCD + k) * a.T + t] =
        dead ? __builtin_nanf("") : lat_s[(f * nq + i) * RCD + k];
  }
  for (int e = tid; e < nf * nq; e += CH_NT) {
    const int i = e / nf, f = e - i * nf;
    const int n = n0 + f, b = n / a.T, t = n - b * a.T;
    const size_t o = ((size_t)b * nq + i) * a.T + t;
    a.codes[o] = dead ? (int64_t)-1 : (int64_t)code_s[f * nq + i];
    a.loss_pf[o] = loss_s[f * nq + i];
    if (a.mask) {
      const float s = a.imp ? (a.imp[n] * a.level) * (float)nq : INFINITY;
      a.mask[o] = (s - (float)i >= 0.0f) ? 1.0f : 0.0f;  // models/utils.py:55-61
    }
  }
  CSTAMP(nq, 3);
  if constexpr (FUSED) FSTAMP(hx.stamps, 36);
}

template <int NM>
__global__ __launch_bounds__(CH_NT) void rvq_chain_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int n0 = blockIdx.x * a.F;
  chain_body<NM, false>(a, sm, n0, min(a.F, a.NF - n0), ChainHandoff{});
}

// ------------------------------------------------------------------------------------------
// Expansion on the matrix cores: z_q_is[b,i,c,t] = (W_out(i)[c,:] . zst[b,i,t,:]) + b_out(i)[c]
// and z_q[b,c,t] = sum_i mask[b,i,t] * z_q_is[b,i,c,t] (stage order, from 0: the masked_sum
// kernel's expression bit for bit). One wave = one (clip, 32-channel, 32-frame) tile over all
// stages; per stage four v_mfma_f32_32x32x2_f32 (K = 8: the out_proj weights x zst, the
// k-ordered fma chain from 0) and the bias as one VALU add -- dot8(W, zst) + bias with the
// reference's roundings (r05: the bias was a 9th k of a fifth MFMA, the same value up to the
// sign of an exact zero). The accumulator layout puts 32 consecutive frames of one channel row
// in each half-wave, so every store instruction writes two 128-B row runs.
struct ExpandArgs {
  const float* zst;    // [B][nq][T][8]
  int B, D, T, nq;
  const float* w_out;  // [nq][D][8]
  const float* b_out;  // [nq][D]
  const float* imp;    // [B][T] or null
  float level;
  const float* mask_in;  // [B][nq][T] or null: explicit mask values (training), replaces imp
  float* z_q_is;       // [B][nq][D][T] or null
  float* z_q;          // [B][D][T]
  float* mask;         // [B][nq][T] or null
  int n_ct, n_tt;      // 32-channel tiles, 32-frame tiles
};

__global__ __launch_bounds__(256) void rvq_expand_kernel(ExpandArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // workgroup = 4 consecutive channel tiles of one (clip, frame tile)
  int bid = blockIdx.x;
  const int ctg = bid % ((a.n_ct + 3) / 4);
  bid /= (a.n_ct + 3) / 4;
  const int tt = bid % a.n_tt;
  const int b = bid / a.n_tt;
  const int ct = ctg * 4 + wave;
  if (ct >= a.n_ct) return;  // no barrier in this kernel
  const int c0 = ct * 32, t0 = tt * 32;
  const int col = lane & 31, h = lane >> 5;
  const int t = t0 + col;
  const bool tv = t < a.T;
  const int tc = tv ? t : a.T - 1;
  const int cr = min(c0 + col, a.D - 1);  // A-operand row of this lane (clamped: D % 32 tail)
  const float s = (a.imp && tv) ? (a.imp[(size_t)b * a.T + t] * a.level) * (float)a.nq : INFINITY;
  const float* zp = a.zst + ((size_t)b * a.nq * a.T + tc) * RCD;
  const size_t zstride = (size_t)a.T * RCD;
  const float* wp = a.w_out + (size_t)cr * RCD;
  const size_t wstride = (size_t)a.D * RCD;
  f32x16 zq;
#pragma unroll
  for (int r = 0; r < 16; ++r) zq[r] = 0.0f;
  // operands of stage i, software-pipelined one stage ahead (the wait for them never covers
  // the previous stage's stores: vmcnt counts stores too)
  // b_out of the accumulator rows c0 + 4 h + (r & 3) + 8 (r >> 2) (clamped at a D % 32 tail:
  // those rows are not stored; D >= 4), loaded for the current stage ahead of the next stage's
  // prefetch
  float4 w0 = ld4(wp), w1 = ld4(wp + 4), z0 = ld4(zp), z1 = ld4(zp + 4);
  for (int i = 0; i < a.nq; ++i) {
    const float4 cw0 = w0, cw1 = w1, cz0 = z0, cz1 = z1;
    float cb[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = ld4(a.b_out + (size_t)i * a.D + min(c0 + 4 * h + 8 * q, a.D - 4));
      cb[4 * q] = v.x; cb[4 * q + 1] = v.y; cb[4 * q + 2] = v.z; cb[4 * q + 3] = v.w;
    }
    if (i + 1 < a.nq) {
      w0 = ld4(wp + (i + 1) * wstride);
      w1 = ld4(wp + (i + 1) * wstride + 4);
      z0 = ld4(zp + (i + 1) * zstride);
      z1 = ld4(zp + (i + 1) * zstride + 4);
    }
    // lane (col, h) supplies k = 2 s + h of step s
    const float wa[4] = {h ? cw0.y : cw0.x, h ? cw0.w : cw0.z, h ? cw1.y : cw1.x, h ? cw1.w : cw1.z};
    const float zb[4] = {h ? cz0.y : cz0.x, h ? cz0.w : cz0.z, h ? cz1.y : cz1.x, h ? cz1.w : cz1.z};
    f32x16 q;
#pragma unroll
    for (int r = 0; r < 16; ++r) q[r] = 0.0f;
#pragma unroll
    for (int st = 0; st < 4; ++st) q = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[st], zb[st], q, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) q[r] = q[r] + cb[r];
    const float m = a.mask_in ? (tv ? a.mask_in[((size_t)b * a.nq + i) * a.T + t] : 0.0f)
                              : ((s - (float)i >= 0.0f) ? 1.0f : 0.0f);  // models/utils.py:45-61
    if (a.mask && ct == 0 && h == 0 && tv) a.mask[((size_t)b * a.nq + i) * a.T + t] = m;
    if (a.z_q_is && tv) {
      float* dst = a.z_q_is + (((size_t)b * a.nq + i) * a.D + c0 + 4 * h) * a.T + t;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2);
        if (c0 + 4 * h + row < a.D) dst[(size_t)row * a.T] = q[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) zq[r] = zq[r] + q[r] * m;
  }
  if (tv) {
    float* dst = a.z_q + ((size_t)b * a.D + c0 + 4 * h) * a.T + t;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);
      if (c0 + 4 * h + row < a.D) dst[(size_t)row * a.T] = zq[r];
    }
  }
}

// ------------------------------------------------------------------------------------------
// The fused RVQ launch (rvq_pt_kernel, below): one kernel instead of chain -> expansion, every
// workgroup of the grid resident at once (clips per launch from the occupancy query).
// Workgroups [0, B P) are chain parts (clip b, frames [p F, p F + F), F <= 16); the workgroups
// after them are the expansion: (clip b, frame window fb, 128-channel block cb) over all stages,
// each stage once the chain parts of its frames have published it, so the z_q_is write stream
// runs under the chain instead of after it. Same expressions as the three launches
// (tests/test_gpu_parity.py).
constexpr int FU_ROWS = 16;         // frames per part block of the stage hand-off rows (F <= 16)
constexpr int FU_CB = 128;          // channels per expansion workgroup
constexpr int SYNC_ERR = 2048;      // the error word (2: an expansion's wait for a stage ran out)
constexpr int SYNC_WORDS = 2052;    // used words (x 4 = 8208 B, a multiple of 16)

struct FusedArgs {
  ChainArgs c;                      // part, B, T, nq, F, NF; outputs
  const float* w_out;               // [nq][D][8]
  const float* b_out;               // [nq][D]
  float* z_q_is;                    // [B][nq][D][T] or null
  float* z_q;                       // [B][D][T]
  unsigned long long* zsh;          // [B][nq][P][FU_ROWS][8] tagged zst granules
  int zsh_bytes;
  int P;                            // chain parts per clip
  int n_fb;                         // expansion frame blocks per clip
  unsigned* sync;
  unsigned* err_host;               // host-mapped error word (report_timeout) or null
  unsigned spin_max;
  unsigned stall;                   // test knob: chain part 0's start delayed by stall x s_sleep(127)
  unsigned epoch;
  unsigned long long* stamps;       // diagnostic build only
  int dbg;                          // diagnostic build only: bit 0 = expansion skips its MFMAs,
                                    // bit 1 = chain parts skip the next stage's codebook
                                    // fragment loads (outputs wrong; timing only)
};

// 4 x 4 transpose inside each lane quad: lane 4 g + k, register 4 qd + u holds E(u, k) on
// entry and E(k, u) on exit (E(row, column) of the quad's 4 x 4 block). Two butterfly steps,
// each swapping one index bit of the register with the same bit of the lane.
__device__ __forceinline__ void quad_transpose(f32x16& q, int lane) {
  const bool o1 = lane & 1, o2 = lane & 2;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {  // register pairs (0, 1), (2, 3): lanes k ^ 1
      const int r0 = 4 * qd + 2 * p, r1 = r0 + 1;
      const float snd = o1 ? q[r0] : q[r1];
      const float got = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(snd), 0xB1, 0xF, 0xF, false));
      if (o1) q[r0] = got; else q[r1] = got;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {  // register pairs (0, 2), (1, 3): lanes k ^ 2
      const int r0 = 4 * qd + p, r1 = r0 + 2;
      const float snd = o2 ? q[r0] : q[r1];
      const float got = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(snd), 0x4E, 0xF, 0xF, false));
      if (o2) q[r0] = got; else q[r1] = got;
    }
  }
}

// First frame of the 32-frame tile that nominally starts at tb: a clip's last, partial tile is
// moved back to end at the clip's last frame (it overlaps the tile before it: those frames are
// computed and written twice, with identical values), so every quad of four frames is whole from
// T = 32 on.
__device__ __forceinline__ int tile_first_frame(int tb, int T) {
  return (tb + 32 > T && T >= 32) ? T - 32 : tb;
}

// The number of active stages (mask = i < n) of the output frames t0 .. t0 + 3 of clip b, one
// per byte (frames past the clip re-read its last one: loaded, never stored).
__device__ __forceinline__ unsigned active_stages4(const ChainArgs& c, int b, int t0) {
  float sv[4];  // the loads first: one memory latency
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = min(max(t0 + u, 0), c.T - 1);
    sv[u] = c.imp ? (c.imp[(size_t)b * c.T + t] * c.level) * (float)c.nq : INFINITY;
  }
  unsigned w = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    // mask[b,i,t] = (s - i >= 0) with s = (imp * level) * nq (models/utils.py:45-61). The
    // fp32 difference rounds monotonically and 0 is exact, so that is s >= i: the first
    // floor(s) + 1 stages (none for NaN or s < 0, all nq for s >= nq - 1 or CBR's inf)
    const int n = sv[u] >= 0.0f ? (int)floorf(fminf(sv[u], (float)(c.nq - 1))) + 1 : 0;
    w |= (unsigned)n << (8 * u);
  }
  return w;
}

// Four consecutive frames t .. t + 3 of one channel row: one 16-B store (rows of T floats are
// dword-aligned); elementwise only where a clip is shorter than a frame tile (T < 32)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store_quad(float* row, int t, int T, float v0, float v1, float v2,
                                           float v3) {
  if (t + 4 <= T) {
    *reinterpret_cast<f4u*>(row + t) = f4u{v0, v1, v2, v3};
  } else if (t < T) {
    row[t] = v0;
    if (t + 1 < T) row[t + 1] = v1;
    if (t + 2 < T) row[t + 2] = v2;
  }
}

__device__ __forceinline__ ChainHandoff fused_handoff(const FusedArgs& f, int b, int p) {
  ChainHandoff hx;
  hx.epoch = f.epoch;
  hx.zsh = f.zsh + (size_t)(b * f.c.nq * f.P + p) * FU_ROWS * RCD;
  hx.zsh_stage = f.P * FU_ROWS * RCD;
  hx.stamps = f.stamps;
  hx.dbg = f.dbg;
  return hx;
}

// W_in planes of vrvq_conv1d_proj's projection epilogue (conv_core.h proj_epilogue): 16-row
// tiles of the R = 8 nq stage rows
__host__ __device__ inline int pj_nrt(int nq) { return (nq * RCD + 15) / 16; }

// ------------------------------------------------------------------------------------------
// rvq_pt_kernel: the quantizer from the projection partials part[8][B T][8 nq] that an earlier
// kernel wrote: the encoder's last conv in its epilogue (vrvq_conv1d_proj) or
// rvq_project3_kernel, the same values bit for bit. Neither z nor W_in is read here.
//   Workgroups [0, B P): chain parts (clip b, frames [p F, p F + F), F <= 16): the 8 partials
// of their frames (plain loads: the writer's kernel boundary orders them) summed in split order
// -- the three-launch chain's expression, so every output equals the three-launch path's bit
// for bit -- then the chain, publishing every stage's zst as tagged granules.
//   Workgroups after: expansion (clip b, 96-frame window fb, 128-channel block cb), 8 waves,
// z_q_is and the masked z_q of the window's 4 x 3 (32-channel, 32-frame) tiles: per stage and
// tile four v_mfma_f32_32x32x2_f32, D[channel][frame] = sum_k W_out[channel][k] zst[frame][k]
// (rvq_expand_kernel's k-ordered products). D leaves the MFMA with one frame per lane and four
// consecutive channels per register quad; a 4 x 4 transpose inside each lane quad (two DPP
// quad_perm exchanges) turns that into four consecutive FRAMES of one channel per register
// quad, so z_q_is / z_q leave as 16-B stores that cover 8 whole 128-B row segments per wave
// instruction (4-B stores needed 4x the instructions; 16-B stores straight from the frame-major
// D orientation touched 32 rows per instruction and ran slower still:
// profiles/r05i_stamps.log). Bias and mask are then per register (the three-launch kernel's
// expressions, per element). What bounds a stage is the z_q_is write stream (11.4 MB per stage
// at B = 32); the same store pattern alone writes at 4-5.7 TB/s (tools/micro/expand_writes.hip),
// next to the chain ~2.7.
//   One channel tile ct = w & 3 per wave (waves w and w + 4 share a SIMD: 3 tiles per SIMD):
// waves 0-2 frame tiles {0, 2}, wave 3 {0, 1}, waves 4-6 {1}, wave 7 {2}. Wave 7 is also the
// LOADER: per stage it polls the window's zst granules (6 x 16 B per lane, tag-checked, bounded)
// into one half of a double-buffered LDS slab while every wave runs the previous stage out of
// the other half; one barrier per stage (on the bound the outputs are NaN). It issues the poll
// BEFORE its own tile's stores and checks the tags after them: vmcnt retires in order, so the
// check waits for the poll only, not for the stores. r05's expansion polled from every wave,
// and where a look came too early its second look waited behind the wave's whole stage of stores
// (a ~1 us bubble per stage while the chain was ahead).
constexpr int PT_FB = 96;                         // frames per expansion window (3 tiles)
constexpr int PT_LOADER = 7;                       // the loader wave
constexpr int PT_SLAB = PT_FB * RCD;               // floats per slab half
constexpr int PT_SL = PT_FB * 4 / 64;              // 16-B granule pairs per loader lane (6)
constexpr int PT_NI = 2;                           // tiles per wave, at most
// floats: the z_q accumulators, CH_NT unused floats after the slab halves (nothing reads them;
// they stay because the LDS bytes decide how many clips are resident)
constexpr int PT_ZQ = 2 * PT_SLAB + CH_NT;
constexpr int PT_NTILE = 12;                       // tiles of a window (4 x 3)
constexpr int PT_EX_FLOATS = PT_ZQ + PT_NTILE * 16 * 64;  // slab halves, gap, accumulators

struct PtOps {
  float wa[4];    // W_out[c0 + col][k], k = h, 2 + h, 4 + h, 6 + h (the MFMA steps' A values)
  float bb[4];    // b_out of the lane's four output channels (one per register quad)
};

// first accumulator slot of wave w (its tiles' slots are consecutive; 12 in all)
__device__ __forceinline__ int pt_slot0(int w) { return w < 4 ? 2 * w : 4 + w; }
// frame tile of slot j of wave w (-1: none)
__device__ __forceinline__ int pt_tile(int w, int j) {
  if (w < 3) return j == 0 ? 0 : 2;
  if (w == 3) return j;
  if (w < PT_LOADER) return j == 0 ? 1 : -1;
  return j == 0 ? 2 : -1;
}

__device__ __forceinline__ void pt_expand_body(const FusedArgs& f, int e, float* sm) {
  const int nq = f.c.nq, T = f.c.T, F = f.c.F;
  constexpr int NCB = RD / FU_CB;
  const int cb = e % NCB;
  const int fb = (e / NCB) % f.n_fb;
  const int b = e / (NCB * f.n_fb);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave == PT_LOADER;
  const int col = lane & 31, h = lane >> 5;
  const int nfr = min(PT_FB, T - fb * PT_FB);       // frames of this window (>= 1)
  const int n_ft = (nfr + 31) / 32;
  // the slab window: PT_FB frames from wlo (the last window ends at the clip's last frame, so it
  // holds the moved-back last tile). Partial last tiles instead (no frame written twice; 9 of
  // every 96 frames' z_q_is rows are at T = 87) measured slower: 41.75 vs 39.2-40.6 us per
  // launch, each stage's stores 0.3-0.8 us longer (profiles/r06f_stamps.log)
  const int wlo = T >= PT_FB ? min(fb * PT_FB, T - PT_FB) : 0;
  const __amdgpu_buffer_rsrc_t zr =
      __builtin_amdgcn_make_buffer_rsrc(f.zsh, (short)0, f.zsh_bytes, RSRC_FLAGS);
  const int zstage = f.P * FU_ROWS * RCD * 8;  // bytes per stage
  const unsigned base = f.epoch * 64u;
  __shared__ int xdead_s;  // the loader's wait ran out (then no wait any more; outputs NaN)
  if (tid == 0) xdead_s = 0;

  // ---- loader: lane item q = lane + 64 u -> frame wlo + (q >> 2), slots 2 (q & 3) + {0, 1}
  // (frames past the clip re-read its last one: loaded, never used)
  auto soff = [&](int u) {
    const int q = lane + 64 * u;
    const int t = min(wlo + (q >> 2), T - 1);
    const int p = t / F, fr = t - p * F;
    return ((((b * nq) * f.P + p) * FU_ROWS + fr) * RCD + 2 * (q & 3)) * 8;
  };
  // ---- compute state: the wave's channel tile and its frame tiles (wave-uniform activity)
  const int c0 = cb * FU_CB + (wave & 3) * 32;
  const int crow = c0 + col;                  // A-operand row (W_out) of this lane
  const int chk = c0 + 4 * h + (lane & 3);    // after the transpose: channels chk + 8 qd
  const size_t wstride = (size_t)RD * RCD;
  int tbs[PT_NI];  // the tiles' first frames (wave-uniform)
  unsigned nact[PT_NI];
  bool act[PT_NI];
#pragma unroll
  for (int j = 0; j < PT_NI; ++j) {
    const int ft = pt_tile(wave, j);
    act[j] = ft >= 0 && ft < n_ft;
    const int tb = tile_first_frame(fb * PT_FB + max(ft, 0) * 32, T);
    tbs[j] = __builtin_amdgcn_readfirstlane(tb);
    nact[j] = active_stages4(f.c, b, tb + 4 * (col >> 2));
  }
  // the lane's B-operand frame (col) as a slab row, and the first of its four output frames
  auto trow = [&](int j) { return min(max(tbs[j] - wlo + col, 0), PT_FB - 1); };
  auto tq = [&](int j) { return tbs[j] + 4 * (col >> 2); };
  auto load_ops = [&](int i, PtOps& o) {
    const float* wp = f.w_out + (size_t)i * wstride + (size_t)crow * RCD + h;
#pragma unroll
    for (int s = 0; s < 4; ++s) o.wa[s] = wp[2 * s];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) o.bb[qd] = f.b_out[(size_t)i * RD + chk + 8 * qd];
  };
  // the masked z_q accumulators live in LDS ([slot][quad][lane] float4: conflict-free 16-B
  // accesses; in registers they spilled at the 128-VGPR budget with three tiles per wave, and a
  // spill reload would wait behind the stage's stores)
  float4* zacc = reinterpret_cast<float4*>(sm + PT_ZQ) + pt_slot0(wave) * (4 * 64) + lane;
#pragma unroll
  for (int j = 0; j < PT_NI; ++j)
    if (pt_tile(wave, j) >= 0)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) zacc[(j * 4 + qd) * 64] = make_float4(0.f, 0.f, 0.f, 0.f);
  PtOps cur;
  load_ops(0, cur);
  __syncthreads();  // xdead_s initialised
  bool dead = false;
  u32x4 g[PT_SL];
  // iteration i: the loader fills slab half (i & 1) with stage i while every wave runs stage
  // i - 1 from the other half
  for (int i = 0; i <= nq; ++i) {
    const bool poll = loader && i < nq && !dead;
    const unsigned tag = base + (unsigned)i + 1u;
    if (poll)  // issued ahead of this wave's stores below
#pragma unroll
      for (int u = 0; u < PT_SL; ++u)
        g[u] = __builtin_amdgcn_raw_buffer_load_b128(zr, soff(u) + i * zstage, 0, CPOL_SC1);
    if (i > 0) {
      const int si = i - 1;  // the stage computed now
      FSTAMP(f.stamps, 1 + si);
      // the next stage's operands ahead of this stage's stores (vmcnt retires in order)
      PtOps nxt;
      load_ops(min(si + 1, nq - 1), nxt);
      const float* slab = sm + (si & 1) * PT_SLAB;
#pragma unroll
      for (int j = 0; j < PT_NI; ++j) {
        if (!act[j]) continue;
        const float4 zb = *reinterpret_cast<const float4*>(slab + trow(j) * RCD + 4 * h);
        f32x16 q;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = 0.0f;
        q = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.wa[0], zb.x, q, 0, 0, 0);
        q = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.wa[1], zb.y, q, 0, 0, 0);
        q = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.wa[2], zb.z, q, 0, 0, 0);
        q = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.wa[3], zb.w, q, 0, 0, 0);
        quad_transpose(q, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = q[r] + cur.bb[r >> 2];
        if (dead)  // wave-uniform (a timed-out wait): poisoned outputs
#pragma unroll
          for (int r = 0; r < 16; ++r) q[r] = __builtin_nanf("");
        if (f.z_q_is) {
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            float* row = f.z_q_is + (((size_t)b * nq + si) * RD + chk + 8 * qd) * T;
            store_quad(row, tq(j), T, q[4 * qd], q[4 * qd + 1], q[4 * qd + 2], q[4 * qd + 3]);
          }
        }
        float m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned n = (nact[j] >> (8 * u)) & 0xffu;
          m[u] = (unsigned)si < n ? 1.0f : 0.0f;  // models/utils.py:45-61
        }
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          float4 a = zacc[(j * 4 + qd) * 64];
          a.x = a.x + q[4 * qd] * m[0];
          a.y = a.y + q[4 * qd + 1] * m[1];
          a.z = a.z + q[4 * qd + 2] * m[2];
          a.w = a.w + q[4 * qd + 3] * m[3];
          zacc[(j * 4 + qd) * 64] = a;
        }
        __builtin_amdgcn_sched_barrier(0);  // one tile's 16 values live at a time
      }
      if (si < 8) FSTAMP(f.stamps, 48 + si);  // the stage's stores issued (thread 0)
      cur = nxt;
    }
    if (poll) {
      // two looks in flight: while one look's loads are checked the next one is already on its
      // way, so a stage that lands just after a look is seen half a round trip later instead of
      // a whole one (each sc1 look crosses to the chain part's XCD: ~1-2 us)
      u32x4 h[PT_SL];
      auto look_ok = [&](const u32x4 (&v)[PT_SL]) {
        bool ok = true;
#pragma unroll
        for (int u = 0; u < PT_SL; ++u) ok = ok && v[u][1] == tag && v[u][3] == tag;
        return __builtin_amdgcn_ballot_w64(!ok) == 0;
      };
      bool in_h = false;
      for (unsigned it = 0;; ++it) {
#pragma unroll
        for (int u = 0; u < PT_SL; ++u)
          h[u] = __builtin_amdgcn_raw_buffer_load_b128(zr, soff(u) + i * zstage, 0, CPOL_SC1);
        if (look_ok(g)) break;
        if (it >= f.spin_max) {
          if (lane == 0) {
            report_timeout(f.sync + SYNC_ERR, f.err_host, 2u);
            xdead_s = 1;
          }
          dead = true;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
#pragma unroll
        for (int u = 0; u < PT_SL; ++u)
          g[u] = __builtin_amdgcn_raw_buffer_load_b128(zr, soff(u) + i * zstage, 0, CPOL_SC1);
        if (look_ok(h)) {
          in_h = true;
          break;
        }
      }
      if (in_h)
#pragma unroll
        for (int u = 0; u < PT_SL; ++u) g[u] = h[u];
      if (i < 8) FSTAMPT(f.stamps, 56 + i, 64 * PT_LOADER);  // the stage's rows seen
      float* slab = sm + (i & 1) * PT_SLAB;
#pragma unroll
      for (int u = 0; u < PT_SL; ++u) {
        const int q = lane + 64 * u;
        *reinterpret_cast<float2*>(slab + (q >> 2) * RCD + 2 * (q & 3)) =
            make_float2(__uint_as_float(g[u][0]), __uint_as_float(g[u][2]));
      }
    }
    __syncthreads();  // slab half (i & 1) holds stage i; half ((i - 1) & 1) is free
    dead = xdead_s != 0;
  }
  FSTAMP(f.stamps, 40);
#pragma unroll
  for (int j = 0; j < PT_NI; ++j) {
    if (!act[j]) continue;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      float* row = f.z_q + ((size_t)b * RD + chk + 8 * qd) * T;
      const float d = dead ? __builtin_nanf("") : 0.0f;
      const float4 a = zacc[(j * 4 + qd) * 64];
      store_quad(row, tq(j), T, a.x + d, a.y + d, a.z + d, a.w + d);
    }
  }
}

template <int NM>
__global__ __launch_bounds__(CH_NT, 4) void rvq_pt_kernel(FusedArgs f) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int B = f.c.B, T = f.c.T, F = f.c.F;
  const int blk = blockIdx.x;
  FSTAMP(f.stamps, 0);
  if (blk >= B * f.P) {
    pt_expand_body(f, blk - B * f.P, sm);
    FSTAMP(f.stamps, 41);
    return;
  }
  const int b = blk / f.P, p = blk - b * f.P;
  const int t0 = p * F, nf = min(F, T - t0);
  if (f.stall && blk == 0)  // test knob (vrvq_rvq_debug_stall): a late producer
    for (unsigned k = 0; k < f.stall; ++k) __builtin_amdgcn_s_sleep(127);
  chain_body<NM, true>(f.c, sm, b * T + t0, nf, fused_handoff(f, b, p));
}

// ------------------------------------------------------------------------------------------
// Host side. The codebook size (NM = ncode / 256) is a template parameter of the two kernels
// that scan a codebook and of nothing on the host: one table, indexed by the size
// (rvq_shape_ok: 256, 512, 768 or 1024 codes).
struct RvqKernels {
  void (*chain)(ChainArgs);
  void (*pt)(FusedArgs);
};

const RvqKernels& rvq_kernels(int ncode) {
  static const RvqKernels table[4] = {{rvq_chain_kernel<1>, rvq_pt_kernel<1>},
                                      {rvq_chain_kernel<2>, rvq_pt_kernel<2>},
                                      {rvq_chain_kernel<3>, rvq_pt_kernel<3>},
                                      {rvq_chain_kernel<4>, rvq_pt_kernel<4>}};
  return table[ncode / 256 - 1];
}

int launch_project(const float* z, int batch, int frames, int nq, const float* w_in_t,
                   float* part, hipStream_t st) {
  const long long nf = (long long)batch * frames;
  VRVQ_CHECK_ARG(nf * nq * RCD * PJ_SPLIT < 0x7fffffffLL);
  const int n_tc = (frames + PJ_TC - 1) / PJ_TC;
  VRVQ_CHECK_ARG((long long)batch * n_tc < 0x7fffffffLL);
  hipError_t e = hipFuncSetAttribute((const void*)rvq_project3_kernel,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, PJ3_LDS);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rvq_project3_kernel, dim3((unsigned)(batch * n_tc), PJ_SPLIT), dim3(PJ_NT),
                     PJ3_LDS, st, z, frames, nq, n_tc, w_in_t, part, (int)nf);
  return vrvq_launch_status();
}

unsigned long long* g_stamps = nullptr;   // diagnostic build: vrvq_debug_set_stamps
unsigned long long* g_fstamps = nullptr;  // diagnostic build: vrvq_debug_set_fused_stamps
int g_fdbg = 0;                           // diagnostic build: vrvq_debug_set_fused_flags

int launch_chain(const ChainArgs& a0, int ncode, hipStream_t st) {
  ChainArgs a = a0;
  a.stamps = g_stamps;
  // frames per workgroup: one workgroup per CU (<= 256 in one round) with as few frames each
  // as that allows, at most 16 (one MFMA column tile). The stage time is latency-bound and
  // nearly independent of F (measured: F = 6 at two workgroups per CU was no faster).
  const long long nf = (long long)a.B * a.T;
  long long F = (nf + 255) / 256;
  F = F < 1 ? 1 : (F > CH_FMAX ? CH_FMAX : F);
  a.F = (int)F;
  a.NF = (int)nf;
  a.NFS = a.NFS ? a.NFS : (int)nf;
  const long long nblk = (nf + F - 1) / F;
  VRVQ_CHECK_ARG(nblk < 0x7fffffffLL);
  const size_t lds = (size_t)ChainLds(a.nq, a.F, ncode).total * sizeof(float);
  if (lds > 160 * 1024) return VRVQ_ERR_UNSUPPORTED;
  const auto kern = rvq_kernels(ncode).chain;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kern,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(CH_NT), lds, st, a);
  return vrvq_launch_status();
}

// a: every field but the tile counts
int launch_expand(ExpandArgs a, hipStream_t st) {
  a.n_ct = (a.D + 31) / 32;
  a.n_tt = (a.T + 31) / 32;
  const long long nblk = (long long)a.B * a.n_tt * ((a.n_ct + 3) / 4);
  VRVQ_CHECK_ARG(nblk < 0x7fffffffLL);
  hipLaunchKernelGGL(rvq_expand_kernel, dim3((unsigned)nblk), dim3(256), 0, st, a);
  return vrvq_launch_status();
}

bool rvq_shape_ok(int dim, int cdim, int nq, int ncode) {
  return dim == RD && cdim == RCD && nq <= CH_NQMAX && ncode > 0 && ncode % 256 == 0 &&
         ncode <= 1024;
}

// bytes of the projection partials [8][nf][nq 8] (a multiple of 256)
size_t part_bytes(long long nf, int nq) { return (size_t)PJ_SPLIT * nf * nq * RCD * sizeof(float); }

// ---- fused path, host side -----------------------------------------------------------------
// 1: chain and expansion as two launches everywhere (vrvq_rvq_path(1), the A/B and the tests'
// reference); 2: rvq_pt_kernel where the plan allows (default).
int g_rvq_path = 2;

// Process-wide state of the fused launches' in-launch hand-offs:
//  * epochs: ONE counter for every call of the process (every stream and device), so tags are
//    unique across streams -- granules a call on another stream left can never match. At
//    EPOCH_RESET the counter restarts at 2 and every library-owned granule area is cleared (on
//    its own stream, ordered after the calls that used it) before a tag can repeat.
//  * granule areas: eager calls hand off through a library-owned area per (device, stream)
//    (hipMalloc, zeroed at allocation, grown on demand), never shared with the caller or the
//    caching allocator: every tag word in it was written by this library (an older epoch). A
//    caller workspace whose previous contents happened to hold 64 * epoch in a tag slot (small
//    integer data does) could otherwise pass a check before the real granule lands.
//  * under stream capture there is no allocation: the call uses the caller's workspace,
//    (sync block, then granules) zeroed by captured memset nodes, and epoch 1 (eager epochs
//    start at 2).
//  * the error word: a per-stream device word (vrvq_rvq_sync_error, synchronising) and one
//    host-mapped word of the process (vrvq_rvq_pending_error, no synchronisation; the torch
//    ops raise on it at their next call).
struct StreamState {
  unsigned* sync = nullptr;  // SYNC_WORDS device words
  void* area = nullptr;      // granules of eager calls
  size_t area_bytes = 0;
};
std::mutex g_fu_mu;
std::map<std::pair<int, hipStream_t>, StreamState> g_fu;
unsigned g_epoch = 1;                 // last epoch handed out (guarded by g_fu_mu)
unsigned* g_err_host = nullptr;       // host-mapped error word
unsigned* g_err_host_dev = nullptr;   // its device address
unsigned g_spin_max = SPIN_MAX;       // vrvq_rvq_debug (timeout test)
int g_pt_cap_limit = 0x7fffffff;      // vrvq_rvq_debug_capacity (fallback test)
unsigned g_stall = 0;
constexpr unsigned EPOCH_RESET = 1u << 24;  // 64 epoch + stage stays below 2^32

struct FusedLaunch {
  unsigned* sync = nullptr;
  unsigned epoch = 0;
  char* area = nullptr;  // granule area of this launch (zeroed by memset nodes under capture)
};

// Sync block, epoch and granule area for one fused launch of `bytes` granules on st; false:
// the fused launch cannot run (an allocation failed, or a captured call's workspace is too small).
constexpr size_t FU_SYNC_BYTES = (SYNC_WORDS * sizeof(unsigned) + 255) & ~size_t(255);
bool fused_prepare(hipStream_t st, size_t bytes, void* caller_ws, size_t caller_bytes,
                   FusedLaunch* L) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
  const bool capturing = cs != hipStreamCaptureStatusNone;
  std::lock_guard<std::mutex> guard(g_fu_mu);
  if (!g_err_host && !capturing) {
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
      g_err_host = static_cast<unsigned*>(h);
      __atomic_store_n(g_err_host, 0u, __ATOMIC_RELAXED);
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) g_err_host_dev = static_cast<unsigned*>(d);
    }
  }
  const size_t sync_bytes = SYNC_WORDS * sizeof(unsigned);
  if (capturing) {
    // no allocation inside a capture (and the capture stream is usually new to us): the sync
    // block and the granule area both come from the caller's workspace, zeroed by memset nodes
    // (the workspace functions count FU_SYNC_BYTES in)
    if (!caller_ws || caller_bytes < bytes + FU_SYNC_BYTES) return false;
    if (hipMemsetAsync(caller_ws, 0, bytes + FU_SYNC_BYTES, st) != hipSuccess) return false;
    L->sync = static_cast<unsigned*>(caller_ws);
    L->area = static_cast<char*>(caller_ws) + FU_SYNC_BYTES;
    L->epoch = 1;
    return true;
  }
  StreamState& ss = g_fu[{device, st}];
  if (!ss.sync) {
    if (hipMalloc(&ss.sync, sync_bytes) != hipSuccess) {
      ss.sync = nullptr;
      return false;
    }
    if (hipMemsetAsync(ss.sync, 0, sync_bytes, st) != hipSuccess) return false;
  }
  {
    if (ss.area_bytes < bytes) {
      if (ss.area) {
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        (void)hipFree(ss.area);
        ss.area = nullptr;
        ss.area_bytes = 0;
      }
      const size_t want = bytes + bytes / 4;
      if (hipMalloc(&ss.area, want) != hipSuccess) {
        ss.area = nullptr;
        return false;
      }
      if (hipMemsetAsync(ss.area, 0, want, st) != hipSuccess) return false;
      ss.area_bytes = want;
    }
    if (++g_epoch >= EPOCH_RESET) {
      g_epoch = 2;
      for (auto& kv : g_fu)
        if (kv.second.area) (void)hipMemsetAsync(kv.second.area, 0, kv.second.area_bytes, kv.first.second);
    }
    L->area = static_cast<char*>(ss.area);
    L->epoch = g_epoch;
  }
  L->sync = ss.sync;
  return true;
}

// Workgroups of `kern` the current device holds resident at once. A fused launch takes no more
// clips than fit in them, so that no waiting workgroup can hold the slot of one it waits for
// (occupancy query with the launch's dynamic LDS, after the attribute that allows it; cached per
// device, kernel and LDS size). 0: the query failed.
int resident_workgroups(const void* kern, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, size_t>, int> cache;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return 0;
  std::lock_guard<std::mutex> guard(mu);
  const auto key = std::make_tuple(device, kern, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int cus = 0, per = 0;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, CH_NT, lds) != hipSuccess)
    cus = per = 0;
  return cache[key] = cus * per;
}

// Launch timing (vrvq_rvq_timing): while on, every fused launch carries a (start, stop) pair of
// HIP events in its own dispatch packet (hipExtLaunchKernelGGL), so the elapsed time is the
// kernel's own duration on its stream (what rocprofv3 reports for it), with no marker packets
// of their own around it. vrvq_rvq_timing_read averages the recorded pairs.
struct LaunchTimer {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> pool;  // 2 per recorded launch
  size_t used = 0;
  bool next(hipEvent_t* start, hipEvent_t* stop) {
    std::lock_guard<std::mutex> guard(mu);
    if (!on) return false;
    while (pool.size() < used + 2) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return false;
      pool.push_back(e);
    }
    *start = pool[used];
    *stop = pool[used + 1];
    used += 2;
    return true;
  }
};
LaunchTimer g_timer;

template <typename K>
int launch_timed(K kern, unsigned grid, size_t lds, hipStream_t st, const FusedArgs& f) {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (g_timer.next(&ev0, &ev1))
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(CH_NT), lds, st, ev0, ev1, 0, f);
  else
    hipLaunchKernelGGL(kern, dim3(grid), dim3(CH_NT), lds, st, f);
  return vrvq_launch_status();
}

// The per-call arguments of launch_pt (whole batch); the weight tables travel in a FusedArgs the
// entry point fills once (rvq_weights).
struct RvqCall {
  int batch, frames, nq, ncode;
  const float* part;  // [8][B T][nq 8]
  const float* imp;   // or null
  int64_t* codes;
  float* latents;
  float* loss_pf;
  float* z_q_is;      // or null
  float* z_q;
  float* mask;        // or null
  void* ws;
  size_t ws_bytes;
  hipStream_t st;
};

// Chunk of clips [b0, b0 + bc) of a fused launch: the outputs and inputs offset to it.
void fused_chunk_args(FusedArgs& f, const RvqCall& a, int b0, int bc, int F) {
  const size_t T = (size_t)a.frames, DT = RD * T, nq = (size_t)a.nq;
  ChainArgs& c = f.c;
  c.B = bc;
  c.T = a.frames;
  c.nq = a.nq;
  c.F = F;
  c.NF = bc * a.frames;
  c.imp = a.imp ? a.imp + b0 * T : nullptr;
  c.codes = a.codes + b0 * nq * T;
  c.latents = a.latents + b0 * nq * RCD * T;
  c.loss_pf = a.loss_pf + b0 * nq * T;
  c.zst = nullptr;
  c.mask = a.mask ? a.mask + b0 * nq * T : nullptr;
  c.stamps = nullptr;
  f.z_q_is = a.z_q_is ? a.z_q_is + b0 * nq * DT : nullptr;
  f.z_q = a.z_q + b0 * DT;
  f.err_host = g_err_host_dev;
  f.spin_max = g_spin_max;
  f.stall = g_stall;
  f.stamps = g_fstamps;
  f.dbg = g_fdbg;
}

size_t zsh_bytes(int bc, int nq, int P) { return (size_t)bc * nq * P * FU_ROWS * RCD * 8; }
size_t pt_zst_bytes(int batch, int frames, int nq) { return (size_t)batch * nq * frames * RCD * 4; }

// The launch plan of the quantizer from partials (vrvq_rvq_encode_part, and vrvq_rvq_encode after
// its projection): everything the launcher, the workspace size (vrvq_rvq_workspace_part) and the
// queries (vrvq_rvq_fused_clips, vrvq_rvq_plan) need to agree on, worked out here and nowhere else.
enum { PLAN_PT = VRVQ_RVQ_PLAN_PT, PLAN_CHAIN_EXPAND = VRVQ_RVQ_PLAN_CHAIN_EXPAND };
struct RvqPlan {
  int kind = PLAN_CHAIN_EXPAND;  // rvq_pt_kernel per group of resident clips | chain, then expand
  int F = 0, P = 0, n_fb = 0;    // frames per chain part; parts and 96-frame windows per clip
  int wpc = 0;                   // workgroups per clip: P parts + 8 channel blocks x n_fb windows
  int lds = 0;                   // dynamic LDS bytes of rvq_pt_kernel
  int resident = 0;              // workgroups the device holds at once (0: not asked)
  int clips = 0;                 // clips per launch (0: chain + expand)
  int launches = 2;
  long long ws_bytes = 0;        // the larger of the captured launch's granules + sync block and
                                 // the two launches' zst rows
};

constexpr int RESIDENT_QUERY = 0;   // rvq_plan's `resident`: ask the device (the only HIP calls)
constexpr int RESIDENT_UNUSED = -1;  // ... geometry and workspace only (no device touched)

RvqPlan rvq_plan(int batch, int frames, int nq, int ncode, int resident) {
  RvqPlan p;
  p.ws_bytes = (long long)pt_zst_bytes(batch, frames, nq);
  // 16 frames per chain part: fewer, longer chain parts measured fastest at T = 87 (in-step
  // 43.1-43.5 us vs 44.2 at F = 11, 44.4-44.8 at 12; profiles/r06g_ab.txt); fewer only where
  // the chain's LDS would not fit twice per CU (beside an expansion workgroup: slab halves and
  // z_q accumulators)
  auto lds_of = [&](int F) {
    return (size_t)max(ChainLds(nq, F, ncode).total, PT_EX_FLOATS) * sizeof(float);
  };
  p.F = min(FU_ROWS, frames);
  while (p.F >= 1 && lds_of(p.F) > 80 * 1024) --p.F;
  if (p.F < 1) return p;
  p.P = (frames + p.F - 1) / p.F;
  p.n_fb = (frames + PT_FB - 1) / PT_FB;
  p.wpc = p.P + (RD / FU_CB) * p.n_fb;
  p.lds = (int)lds_of(p.F);
  p.ws_bytes = std::max(p.ws_bytes, (long long)(zsh_bytes(batch, nq, p.P) + FU_SYNC_BYTES));
  // the two process-wide test hooks: vrvq_rvq_path(1) and vrvq_rvq_debug_capacity
  if (resident == RESIDENT_UNUSED || g_rvq_path == 1) return p;
  p.resident = resident != RESIDENT_QUERY
                   ? resident
                   : resident_workgroups((const void*)rvq_kernels(ncode).pt, (size_t)p.lds);
  // a launch's granule area is addressed with 32-bit byte offsets (never the binding limit at a
  // supported shape: one clip's granules are nq P KiB)
  const long long fit = std::max(1LL, 0x7fffffffLL / (long long)zsh_bytes(1, nq, p.P));
  p.clips = (int)std::min<long long>(min(min(p.resident / p.wpc, g_pt_cap_limit), batch), fit);
  if (p.clips < 1) return p;
  p.kind = PLAN_PT;
  p.launches = (int)(((long long)batch + p.clips - 1) / p.clips);
  return p;
}

// The weight tables of a call, as launch_pt takes them (the per-launch fields are filled there).
FusedArgs rvq_weights(const float* b_in, const float* cb, const float* cbf, const float* c2,
                      const float* w_out, const float* b_out, const float* mcol, const float* qb,
                      float level) {
  FusedArgs f{};
  ChainArgs& c = f.c;
  c.b_in = b_in; c.qb = qb; c.mcol = mcol; c.cb = cb; c.cbf = cbf; c.c2 = c2;
  c.level = level;
  f.w_out = w_out;
  f.b_out = b_out;
  return f;
}

// The quantizer from the partials as planned: rvq_pt_kernel per group of resident clips,
// or -- a clip longer than the resident grid, or vrvq_rvq_path(1) -- the chain and the expansion
// as two stream-ordered launches over the same partials (zst through the workspace). Both give
// the same outputs bit for bit.
int launch_pt(const FusedArgs& f0, const RvqCall& a) {
  const RvqPlan p = rvq_plan(a.batch, a.frames, a.nq, a.ncode, RESIDENT_QUERY);
  if (p.kind == PLAN_CHAIN_EXPAND) {
    if (a.ws_bytes < pt_zst_bytes(a.batch, a.frames, a.nq)) return VRVQ_ERR_ARG;
    float* zst = static_cast<float*>(a.ws);
    ChainArgs c = f0.c;
    c.part = a.part; c.B = a.batch; c.T = a.frames; c.nq = a.nq; c.NFS = 0;
    c.imp = a.imp; c.codes = a.codes; c.latents = a.latents; c.loss_pf = a.loss_pf; c.zst = zst;
    c.mask = a.mask;
    const int rc = launch_chain(c, a.ncode, a.st);
    if (rc) return rc;
    return launch_expand(ExpandArgs{zst, a.batch, RD, a.frames, a.nq, f0.w_out, f0.b_out, a.imp,
                                    f0.c.level, nullptr, a.z_q_is, a.z_q, nullptr},
                         a.st);
  }
  const size_t need = zsh_bytes(p.clips, a.nq, p.P);
  for (int b0 = 0; b0 < a.batch; b0 += p.clips) {
    const int bc = min(p.clips, a.batch - b0);
    FusedArgs f = f0;
    FusedLaunch L;
    if (!fused_prepare(a.st, need, a.ws, a.ws_bytes, &L)) return VRVQ_ERR_UNSUPPORTED;
    fused_chunk_args(f, a, b0, bc, p.F);
    f.c.part = a.part + (size_t)b0 * a.frames * a.nq * RCD;  // the chunk's frames within a split
    f.c.NFS = a.batch * a.frames;                            // split stride: the call's frames
    f.sync = L.sync;
    f.epoch = L.epoch;
    f.zsh = reinterpret_cast<unsigned long long*>(L.area);
    f.zsh_bytes = (int)zsh_bytes(bc, a.nq, p.P);
    f.P = p.P;
    f.n_fb = p.n_fb;
    const int rc =
        launch_timed(rvq_kernels(a.ncode).pt, (unsigned)(bc * p.wpc), (size_t)p.lds, a.st, f);
    if (rc) return rc;
  }
  return 0;
}

// W_in planes of the conv projection epilogue in the 16x16x32 A-fragment order: w3in[ks][plane][rt][lane] =
// 8 bf16 of row r = 16 rt + (lane & 15), channels 32 ks + 8 (lane >> 4) .. +7 (zero rows >= R).
__global__ void rvq_pack_w_in_kernel(const float* __restrict__ w_in_t, int nq, u32x4* __restrict__ w3) {
  const int n_rt = pj_nrt(nq), R = nq * RCD;
  const int total = 32 * 3 * n_rt * 64;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gridDim.x * blockDim.x) {
    const int lane = o & 63;
    int q = o >> 6;
    const int rt = q % n_rt;
    q /= n_rt;
    const int plane = q % 3, ks = q / 3;
    const int r = rt * 16 + (lane & 15), c0 = 32 * ks + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v[u] = r < R ? w_in_t[((size_t)(r >> 3) * RD + c0 + u) * RCD + (r & 7)] : 0.0f;
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) rvq_split3x2(v[2 * u], v[2 * u + 1], h[u], m[u], l[u]);
    w3[o] = plane == 0 ? u32x4{h[0], h[1], h[2], h[3]}
          : plane == 1 ? u32x4{m[0], m[1], m[2], m[3]} : u32x4{l[0], l[1], l[2], l[3]};
  }
}

}  // namespace

#ifdef VRVQ_STAMPS
// Diagnostic build only (not in include/vrvq.h): the chain kernel's stamp buffer.
extern "C" int vrvq_debug_set_stamps(unsigned long long* buf) {
  g_stamps = buf;
  return 0;
}
extern "C" int vrvq_debug_set_fused_stamps(unsigned long long* buf) {
  g_fstamps = buf;
  return 0;
}
// bit 0: the expansion workgroups skip their MFMAs (timing experiment; outputs wrong)
extern "C" int vrvq_debug_set_fused_flags(int flags) {
  g_fdbg = flags;
  return 0;
}
#endif

template <typename Acc>
static int cross_prep(const float* w_in_t, const float* w_out, const float* b_out, int nq, int dim,
                      int cdim, float* mcol, float* qb, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(w_in_t && w_out && b_out && mcol && qb && nq > 0);
  if (dim != RD || cdim != RCD) return VRVQ_ERR_UNSUPPORTED;
  // mcol: one thread per (j, i, k, m) chain; qb: one workgroup per stage (cross_prep_qb_kernel)
  const int total = nq * nq * 64;
  hipLaunchKernelGGL(cross_prep_kernel<Acc>, dim3((total + 255) / 256), dim3(256), 0,
                     as_stream(stream), w_in_t, w_out, b_out, nq, mcol, qb);
  hipLaunchKernelGGL(cross_prep_qb_kernel<Acc>, dim3(nq), dim3(RD), 0, as_stream(stream), w_in_t,
                     b_out, qb);
  return vrvq_launch_status();
}

extern "C" int vrvq_rvq_cross_prep(const float* w_in_t, const float* w_out, const float* b_out,
                                   int nq, int dim, int cdim, float* mcol, float* qb,
                                   vrvq_stream_t stream) {
  return cross_prep<float>(w_in_t, w_out, b_out, nq, dim, cdim, mcol, qb, stream);
}

extern "C" int vrvq_rvq_cross_prep_precise(const float* w_in_t, const float* w_out,
                                           const float* b_out, int nq, int dim, int cdim,
                                           float* mcol, float* qb, vrvq_stream_t stream) {
  return cross_prep<double>(w_in_t, w_out, b_out, nq, dim, cdim, mcol, qb, stream);
}

extern "C" int vrvq_rvq_frag(const float* cbn, int nq, int ncode, int cdim, float* cbf,
                             vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(cbn && cbf && nq > 0);
  if (!rvq_shape_ok(RD, cdim, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  const size_t total = (size_t)nq * ncode * RCD;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(rvq_frag_kernel, dim3(grid), dim3(256), 0, as_stream(stream), cbn, nq,
                     ncode, cbf);
  return vrvq_launch_status();
}

extern "C" int vrvq_rvq_project(const float* z, int batch, int dim, int frames, int nq, int cdim,
                                const float* w_in_t, float* part, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(z && w_in_t && part && batch > 0 && frames > 0 && nq > 0);
  if (dim != RD || cdim != RCD) return VRVQ_ERR_UNSUPPORTED;
  return launch_project(z, batch, frames, nq, w_in_t, part, as_stream(stream));
}

extern "C" int vrvq_rvq_chain(const float* part, int batch, int frames, int nq, int ncode,
                              int cdim, const float* b_in, const float* qb, const float* mcol,
                              const float* cb, const float* cbf, const float* c2,
                              const float* imp, float level, int64_t* codes, float* latents,
                              float* loss_pf, float* zst, float* mask, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(part && b_in && qb && mcol && cb && cbf && c2 && codes && latents && loss_pf &&
                 zst);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && nq > 0);
  if (!rvq_shape_ok(RD, cdim, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  ChainArgs a{};
  a.part = part; a.B = batch; a.T = frames; a.nq = nq;
  a.b_in = b_in; a.qb = qb; a.mcol = mcol; a.cb = cb; a.cbf = cbf; a.c2 = c2;
  a.imp = imp; a.level = level;
  a.codes = codes; a.latents = latents; a.loss_pf = loss_pf; a.zst = zst; a.mask = mask;
  return launch_chain(a, ncode, as_stream(stream));
}

extern "C" int vrvq_rvq_expand(const float* zst, int batch, int dim, int frames, int nq, int cdim,
                               const float* w_out, const float* b_out, const float* imp,
                               float level, float* z_q_is, float* z_q, float* mask,
                               vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(zst && w_out && b_out && z_q);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && nq > 0 && dim >= 4);
  if (cdim != RCD) return VRVQ_ERR_UNSUPPORTED;
  return launch_expand(ExpandArgs{zst, batch, dim, frames, nq, w_out, b_out, imp, level, nullptr,
                                  z_q_is, z_q, mask},
                       as_stream(stream));
}

extern "C" int vrvq_rvq_expand_masked(const float* zst, int batch, int dim, int frames, int nq,
                                      int cdim, const float* w_out, const float* b_out,
                                      const float* mask, float* z_q_is, float* z_q,
                                      vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(zst && w_out && b_out && mask && z_q);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && nq > 0 && dim >= 4);
  if (cdim != RCD) return VRVQ_ERR_UNSUPPORTED;
  return launch_expand(ExpandArgs{zst, batch, dim, frames, nq, w_out, b_out, nullptr, 1.0f, mask,
                                  z_q_is, z_q, nullptr},
                       as_stream(stream));
}

extern "C" int vrvq_rvq_workspace(int batch, int frames, int nq, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && batch > 0 && frames > 0 && nq > 0);
  // An upper bound kept for the ABI (callers sized buffers with it): twice the partials, the
  // larger of the zst rows and 8 KiB per clip and stage, and the sync block -- what the retired
  // r04 launch took. vrvq_rvq_encode needs the partials once plus launch_pt's workspace
  // (part_bytes + rvq_plan().ws_bytes, checked there), which is smaller at every shape: per clip
  // and stage 256 T + max(32 T, 1024 ceil(T / F)) bytes with F >= min(T, 13).
  const long long bnq = (long long)batch * nq;
  *bytes = 2 * (long long)part_bytes((long long)batch * frames, nq) +
           bnq * std::max(32LL * frames, 8192LL) + (long long)FU_SYNC_BYTES;
  return 0;
}

extern "C" int vrvq_rvq_path(int path) {
  const int prev = g_rvq_path;
  if (path == 1 || path == 2) g_rvq_path = path;
  else if (path != 0) return VRVQ_ERR_ARG;
  return prev;
}

extern "C" int vrvq_rvq_timing(int on) {
  std::lock_guard<std::mutex> guard(g_timer.mu);
  const int prev = g_timer.on ? 1 : 0;
  g_timer.on = on != 0;
  return prev;
}

extern "C" int vrvq_rvq_timing_read(float* mean_ms, int* count) {
  VRVQ_CHECK_ARG(mean_ms && count);
  std::lock_guard<std::mutex> guard(g_timer.mu);
  *mean_ms = 0.0f;
  *count = 0;
  double sum = 0.0;
  for (size_t k = 0; k + 1 < g_timer.used; k += 2) {
    hipError_t e = hipEventSynchronize(g_timer.pool[k + 1]);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_timer.pool[k], g_timer.pool[k + 1]);
    if (e != hipSuccess) return (int)e;
    sum += ms;
    ++*count;
  }
  if (*count) *mean_ms = (float)(sum / *count);
  g_timer.used = 0;
  return 0;
}

extern "C" int vrvq_rvq_sync_error(vrvq_stream_t stream, int* code) {
  VRVQ_CHECK_ARG(code);
  *code = 0;
  hipStream_t st = as_stream(stream);
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return VRVQ_ERR_ARG;
  unsigned* dev = nullptr;
  {
    std::lock_guard<std::mutex> guard(g_fu_mu);
    auto it = g_fu.find({device, st});
    if (it == g_fu.end() || !it->second.sync) return 0;
    dev = it->second.sync;
  }
  unsigned v = 0;
  hipError_t e = hipMemcpyAsync(&v, dev + SYNC_ERR, sizeof(v), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && v) e = hipMemsetAsync(dev + SYNC_ERR, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  *code = (int)v;
  if (v && g_err_host) __atomic_store_n(g_err_host, 0u, __ATOMIC_RELAXED);  // reported here
  return 0;
}

extern "C" int vrvq_rvq_pending_error(int* code) {
  VRVQ_CHECK_ARG(code);
  *code = 0;
  std::lock_guard<std::mutex> guard(g_fu_mu);
  if (g_err_host) *code = (int)__atomic_exchange_n(g_err_host, 0u, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int vrvq_rvq_debug(unsigned spin_max, unsigned stall) {
  std::lock_guard<std::mutex> guard(g_fu_mu);
  g_spin_max = spin_max ? spin_max : SPIN_MAX;
  g_stall = stall;
  return 0;
}

extern "C" int vrvq_rvq_encode(const float* z, int batch, int dim, int frames, int nq, int ncode,
                               int cdim, const float* w_in_t, const float* b_in, const float* cb,
                               const float* cbf, const float* c2, const float* w_out,
                               const float* b_out, const float* mcol, const float* qb,
                               const float* imp, float level, int64_t* codes, float* latents,
                               float* loss_pf, float* z_q_is, float* z_q, float* mask,
                               void* workspace, long long workspace_bytes,
                               vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(z && w_in_t && b_in && cb && cbf && c2 && w_out && b_out && mcol && qb &&
                 codes && latents && loss_pf && z_q && workspace);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && nq > 0);
  if (!rvq_shape_ok(dim, cdim, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  VRVQ_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  VRVQ_CHECK_ARG((long long)batch * frames * nq * RCD * PJ_SPLIT < 0x7fffffffLL);
  // the partials, then launch_pt's workspace (vrvq_rvq_workspace() covers both at every shape)
  const size_t part_b = part_bytes((long long)batch * frames, nq);
  const long long pt_b = rvq_plan(batch, frames, nq, ncode, RESIDENT_UNUSED).ws_bytes;
  VRVQ_CHECK_ARG(workspace_bytes >= (long long)part_b + pt_b);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  const int rc = launch_project(z, batch, frames, nq, w_in_t, part, st);
  if (rc) return rc;
  return launch_pt(rvq_weights(b_in, cb, cbf, c2, w_out, b_out, mcol, qb, level),
                   RvqCall{batch, frames, nq, ncode, part, imp, codes, latents, loss_pf, z_q_is,
                           z_q, mask, static_cast<char*>(workspace) + part_b,
                           (size_t)workspace_bytes - part_b, st});
}

extern "C" int vrvq_rvq_w_in_planes_size(int nq, int dim, int cdim, long long* n_u16) {
  VRVQ_CHECK_ARG(n_u16 && nq > 0);
  if (dim != RD || cdim != RCD || nq > CH_NQMAX) return VRVQ_ERR_UNSUPPORTED;
  *n_u16 = 32LL * 3 * pj_nrt(nq) * 64 * 8;
  return 0;
}

extern "C" int vrvq_rvq_pack_w_in(const float* w_in_t, int nq, int dim, int cdim, uint16_t* w3in,
                                  vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(w_in_t && w3in && nq > 0);
  if (dim != RD || cdim != RCD || nq > CH_NQMAX) return VRVQ_ERR_UNSUPPORTED;
  const int total = 32 * 3 * pj_nrt(nq) * 64;
  hipLaunchKernelGGL(rvq_pack_w_in_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     as_stream(stream), w_in_t, nq, reinterpret_cast<u32x4*>(w3in));
  return vrvq_launch_status();
}

extern "C" int vrvq_rvq_plan(int batch, int frames, int nq, int ncode, int resident,
                             long long out[10]) {
  VRVQ_CHECK_ARG(out && batch > 0 && frames > 0 && nq > 0 && ncode > 0 && resident >= 0);
  if (!rvq_shape_ok(RD, RCD, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  const RvqPlan p = rvq_plan(batch, frames, nq, ncode, resident);
  const long long v[10] = {p.kind, p.F, p.P, p.n_fb, p.wpc, p.lds, p.resident, p.clips,
                           p.launches, p.ws_bytes};
  std::copy(v, v + 10, out);
  return 0;
}

extern "C" int vrvq_rvq_workspace_part(int batch, int frames, int nq, int ncode, long long* bytes) {
  VRVQ_CHECK_ARG(bytes && batch > 0 && frames > 0 && nq > 0 && ncode > 0);
  if (!rvq_shape_ok(RD, RCD, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  *bytes = rvq_plan(batch, frames, nq, ncode, RESIDENT_UNUSED).ws_bytes;
  return 0;
}

extern "C" int vrvq_rvq_encode_part(const float* part, int batch, int dim, int frames, int nq,
                                    int ncode, int cdim, const float* b_in, const float* cb,
                                    const float* cbf, const float* c2, const float* w_out,
                                    const float* b_out, const float* mcol, const float* qb,
                                    const float* imp, float level, int64_t* codes,
                                    float* latents, float* loss_pf, float* z_q_is, float* z_q,
                                    float* mask, void* workspace, long long workspace_bytes,
                                    vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(part && b_in && cb && cbf && c2 && w_out && b_out && mcol && qb && codes &&
                 latents && loss_pf && z_q && workspace);
  VRVQ_CHECK_ARG(batch > 0 && frames > 0 && nq > 0);
  VRVQ_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)part & 15) == 0);
  if (!rvq_shape_ok(dim, cdim, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  VRVQ_CHECK_ARG((long long)batch * frames * nq * RCD * PJ_SPLIT < 0x7fffffffLL);
  VRVQ_CHECK_ARG(workspace_bytes >= rvq_plan(batch, frames, nq, ncode, RESIDENT_UNUSED).ws_bytes);
  return launch_pt(rvq_weights(b_in, cb, cbf, c2, w_out, b_out, mcol, qb, level),
                   RvqCall{batch, frames, nq, ncode, part, imp, codes, latents, loss_pf, z_q_is,
                           z_q, mask, workspace, (size_t)workspace_bytes, as_stream(stream)});
}

extern "C" int vrvq_rvq_fused_clips(int frames, int nq, int ncode, int* clips) {
  VRVQ_CHECK_ARG(clips && frames > 0 && nq > 0);
  *clips = 0;
  if (!rvq_shape_ok(RD, RCD, nq, ncode)) return VRVQ_ERR_UNSUPPORTED;
  // what a call of any batch size could hold: no batch to cap it
  *clips = rvq_plan(0x7fffffff, frames, nq, ncode, RESIDENT_QUERY).clips;
  return 0;
}

extern "C" int vrvq_rvq_debug_capacity(int clips) {
  const int prev = g_pt_cap_limit;
  g_pt_cap_limit = clips >= 0 ? clips : 0x7fffffff;
  return prev;
}
