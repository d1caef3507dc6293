// Micro-benchmark behind DESIGN.md "BSS SDR": the two forms of the correlation launch of
// vrvq_amd/csrc/sdr.hip on the same data and grid, one 256-thread workgroup per 2048-sample chunk,
// 512 lag sums b[l] = sum_i t[i] p[i + l] per chunk, fp64, timed with HIP events:
//   vector   the per-lane-lag FMA loop the library runs (8 lags per lane, a register window)
//   mfma     the (sample, lag) plane tiled into C_q[m][j] = sum_k t[16k+m] p[16k+16q+j], q < 33,
//            each a v_mfma_f64_16x16x4_f64 product, the diagonals j - m read out through LDS
//   mfma, main loop only   the same without the read-out (the accumulators are folded into one
//            number per lane so that nothing is dropped): a lower bound for any MFMA form
// and the largest difference between the two forms' lag sums. Build: hipcc -O3 -ffp-contract=off
// --offload-arch=gfx950 sdr_corr_forms.hip -o sdr_corr_forms
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

constexpr int CHUNK = 2048, FMAX = 512, THREADS = 256, PLOG = CHUNK + FMAX;
constexpr int PPHYS = PLOG / 8 * 9;
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void load_chunk(const float* t, const float* p, double* tl, double* pl,
                                           bool padded) {
  for (int i = threadIdx.x; i < CHUNK; i += THREADS) tl[i] = (double)t[i];
  for (int i = threadIdx.x; i < PLOG; i += THREADS) pl[padded ? i + (i >> 3) : i] = (double)p[i];
  __syncthreads();
}

__global__ __launch_bounds__(THREADS) void corr_vector(const float* t, const float* p, double* out) {
  __shared__ __attribute__((aligned(16))) double tl[CHUNK];
  __shared__ __attribute__((aligned(16))) double pl[PPHYS];
  const size_t base = (size_t)blockIdx.x * CHUNK;
  load_chunk(t + base, p + base, tl, pl, true);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double tot[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) tot[j] = 0.0;
  for (int seg = 0; seg < 4; ++seg) {
    const int ib = wave * 512 + seg * 128;
    const double* __restrict__ pb = pl + (ib + 8 * lane) + (ib >> 3) + lane;
    const double* __restrict__ tb = tl + ib;
    double acc[8], w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) w[j] = pb[j];
    for (int blk = 0; blk < 16; ++blk) {
      const double* __restrict__ pq = pb + blk * 9;
      const double* __restrict__ tq = tb + blk * 8;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        w[(s + 7) & 7] = pq[(s + 7) + ((s + 7) >> 3)];
        const double tv = tq[s];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fma(tv, w[(s + j) & 7], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tot[j] += acc[j];
  }
  __syncthreads();
  double* wsum = pl;
#pragma unroll
  for (int j = 0; j < 8; ++j) wsum[wave * FMAX + 8 * lane + j] = tot[j];
  __syncthreads();
  for (int l = tid; l < FMAX; l += THREADS)
    out[(size_t)blockIdx.x * FMAX + l] =
        ((wsum[l] + wsum[FMAX + l]) + wsum[2 * FMAX + l]) + wsum[3 * FMAX + l];
}

// READ_OUT false: out gets one number per thread (the sum of its accumulators)
template <bool READ_OUT>
__global__ __launch_bounds__(THREADS) void corr_mfma(const float* t, const float* p, double* out) {
  __shared__ __attribute__((aligned(16))) double tl[CHUNK];
  __shared__ __attribute__((aligned(16))) double pl[PLOG];
  const size_t base = (size_t)blockIdx.x * CHUNK;
  load_chunk(t + base, p + base, tl, pl, false);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  f64x4 acc[33];
#pragma unroll
  for (int q = 0; q < 33; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int g = wave * 8; g < wave * 8 + 8; ++g) {  // 64 samples: A[m][k] = t[64 g + 16 k + m]
    const double a = tl[64 * g + lane];
    const double* __restrict__ pg = pl + 64 * g + lane;  // B_q[k][j] = p[64 g + 16 k + 16 q + j]
#pragma unroll
    for (int q = 0; q < 33; ++q)
      acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pg[16 * q], acc[q], 0, 0, 0);
  }
  if (!READ_OUT) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 33; ++q) s += (acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3]);
    out[(size_t)blockIdx.x * FMAX + tid] = s;
    return;
  }
  // read-out: C_q[m][j] (lane: j = lane & 15, m = (lane >> 4) + 4 reg) goes to the wave's
  // scratch by diagonal, sc[(j - m + 15) * 16 + m]; lane x adds half of diagonal x >> 1, the two
  // halves meet, and lag 16 q + (j - m) of the wave's sums takes it
  __syncthreads();
  double* wl = tl + wave * FMAX;          // the wave's 512 lag sums
  double* sc = pl + wave * 512;           // 31 diagonals x 16 slots
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    wl[lane + 64 * i] = 0.0;
    sc[lane + 64 * i] = 0.0;
  }
  __syncthreads();
  const int j = lane & 15, diag = lane >> 1, half = lane & 1;
#pragma unroll
  for (int q = 0; q < 33; ++q) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = (lane >> 4) + 4 * reg;
      sc[(j - m + 15) * 16 + m] = acc[q][reg];
    }
    __syncthreads();
    double s = 0.0;
    if (diag < 31) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s += sc[diag * 16 + 8 * half + e];
    }
    s += __shfl_xor(s, 1, 64);
    const int lag = 16 * q + diag - 15;
    if (half == 0 && diag < 31 && lag >= 0 && lag < FMAX) wl[lag] += s;
    __syncthreads();
  }
  for (int l = tid; l < FMAX; l += THREADS)
    out[(size_t)blockIdx.x * FMAX + l] =
        ((tl[l] + tl[FMAX + l]) + tl[2 * FMAX + l]) + tl[3 * FMAX + l];
}

#define CHECK(x)                                                          \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                      \
      return 1;                                                           \
    }                                                                     \
  } while (0)

template <typename K>
int time_ms(K kernel, const float* t, const float* p, double* out, int chunks, float* ms) {
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  for (int i = 0; i < 5; ++i) hipLaunchKernelGGL(kernel, dim3(chunks), dim3(THREADS), 0, 0, t, p, out);
  CHECK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 7; ++rep) {
    CHECK(hipEventRecord(a, 0));
    for (int i = 0; i < 20; ++i)
      hipLaunchKernelGGL(kernel, dim3(chunks), dim3(THREADS), 0, 0, t, p, out);
    CHECK(hipEventRecord(b, 0));
    CHECK(hipEventSynchronize(b));
    float e;
    CHECK(hipEventElapsedTime(&e, a, b));
    best = e / 20 < best ? e / 20 : best;
  }
  *ms = best;
  return 0;
}

int main() {
  const int chunks = 13 * 216;  // 13 rows of 441,000 samples
  const size_t n = (size_t)chunks * CHUNK + FMAX;
  std::vector<float> ht(n), hp(n);
  unsigned s = 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    ht[i] = ((s >> 8) * (1.0f / 16777216.0f) - 0.5f);
    s = s * 1664525u + 1013904223u;
    hp[i] = 0.7f * ht[i] + 0.1f * ((s >> 8) * (1.0f / 16777216.0f) - 0.5f);
  }
  float *t, *p;
  double *ov, *om;
  const size_t outn = (size_t)chunks * FMAX;
  CHECK(hipMalloc(&t, n * sizeof(float)));
  CHECK(hipMalloc(&p, n * sizeof(float)));
  CHECK(hipMalloc(&ov, outn * sizeof(double)));
  CHECK(hipMalloc(&om, outn * sizeof(double)));
  CHECK(hipMemcpy(t, ht.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(p, hp.data(), n * sizeof(float), hipMemcpyHostToDevice));
  float v_ms, m_ms, l_ms;
  if (time_ms(corr_mfma<false>, t, p, om, chunks, &l_ms)) return 1;
  if (time_ms(corr_vector, t, p, ov, chunks, &v_ms)) return 1;
  if (time_ms(corr_mfma<true>, t, p, om, chunks, &m_ms)) return 1;
  std::vector<double> hv(outn), hm(outn);
  CHECK(hipMemcpy(hv.data(), ov, outn * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hm.data(), om, outn * sizeof(double), hipMemcpyDeviceToHost));
  double diff = 0.0, big = 0.0;
  for (size_t i = 0; i < outn; ++i) {
    diff = fmax(diff, fabs(hv[i] - hm[i]));
    big = fmax(big, fabs(hv[i]));
  }
  const double gflop = 2.0 * chunks * (double)CHUNK * FMAX * 1e-9;
  printf("{\"chunks\": %d, \"vector_ms\": %.5f, \"vector_tflops\": %.2f, \"mfma_ms\": %.5f, "
         "\"mfma_main_loop_only_ms\": %.5f, \"max_abs_diff\": %.3e, \"max_abs_lag_sum\": %.3e}\n",
         chunks, v_ms, gflop / v_ms, m_ms, l_ms, diff, big);
  return 0;
}
