// "VRVQ bitstream 1": the bit-granular VBR stream (include/vrvq.h "Bitstream").
// A stream is little-endian uint32 words; a field of width n at bit p puts bit j of its value at
// stream bit p + j (bit q = bit q & 31 of word q >> 5). Row r = plane A (T counts of cb bits,
// zero-padded to a word) then plane B (the kept codes, frame-major, stage-minor, w bits each,
// zero-padded to a word). Plane A sits at known positions, so an exclusive scan of it places
// every code: both directions run on a grid of (chunk of BS_CHUNK frames, row).
//
// Launch structure (pack; unpack mirrors it with plane A read from the stream):
//   count   grid rows * chunks   one frame per lane: count (prefix check), code range, chunk total
//   rowscan grid rows            scan of the row's chunk totals -> chunk_off, row_codes, row_words
//   offsets grid 1               exclusive scan of row_words -> row_off (the clip scan of pack.hip)
//   write   grid rows * chunks   both planes; fields are OR-ed into a zeroed LDS window and the
//                                window's words stored coalesced. A chunk's plane-A span is whole
//                                words (BS_CHUNK * cb is a multiple of 32); of its plane-B span
//                                only the first and last word can be shared with a neighbour, and
//                                those two are OR-ed into the (zeroed) stream with an integer
//                                atomic, whose result does not depend on order.
// Position arithmetic is 64-bit wherever it is in bits or in words of the whole stream.
#include "common.h"

namespace {

constexpr int BS_NT = 256;                              // threads = frames of a chunk
constexpr int BS_CHUNK = VRVQ_BITSTREAM_CHUNK_FRAMES;   // one frame per thread
constexpr int BS_WIN = 2048;                            // LDS window of plane B, words (8 KiB)
static_assert(BS_CHUNK == BS_NT, "one frame per thread");
static_assert((BS_CHUNK % 32) == 0, "a chunk's plane-A span must be whole words");

typedef unsigned int u32;
typedef unsigned long long u64;

// Exclusive scan of one int per thread over the workgroup: wave64 shuffles, then the four wave
// totals through LDS. s_w: 4 ints. Returns the exclusive prefix; *total = the block's sum.
__device__ __forceinline__ int bs_block_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();                 // s_w may still be read from an earlier call
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < BS_NT / 64; ++k) {
    const int s = s_w[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

__device__ __forceinline__ long long bs_block_scan64(long long v, long long* s_w,
                                                     long long* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < BS_NT / 64; ++k) {
    const long long s = s_w[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

__device__ __forceinline__ long long words_of(long long bits) { return (bits + 31) >> 5; }

// ------------------------------------------------------------------------------ pack: plan
// mask == nullptr: every stage kept (the fixed-count stream, cb = 0).
__global__ __launch_bounds__(BS_NT) void bs_count_kernel(const int64_t* __restrict__ codes,
                                                         const float* __restrict__ mask, int nq,
                                                         int T, int nchunk, int ncode,
                                                         int* __restrict__ counts,
                                                         int* __restrict__ chunk_total,
                                                         int* __restrict__ err) {
  __shared__ int s_w[BS_NT / 64];
  const long long r = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const int t = chunk * BS_CHUNK + threadIdx.x;
  int c = 0;
  if (t < T) {
    bool seen_zero = false, bad_prefix = false, bad_code = false;
    for (int i = 0; i < nq; ++i) {
      const size_t ci = ((size_t)r * nq + i) * T + t;
      const bool on = mask ? mask[ci] != 0.0f : true;
      if (on) {
        if (seen_zero) bad_prefix = true;
        const long long v = codes[ci];
        if (v < 0 || v >= ncode) bad_code = true;
        ++c;
      } else {
        seen_zero = true;
      }
    }
    if (bad_prefix) atomicMax(err, 1);          // not prefix-shaped
    else if (bad_code) atomicMax(err, 2);       // a kept code outside [0, ncode)
    counts[(size_t)r * T + t] = c;
  }
  int tot;
  bs_block_scan(c, s_w, &tot);
  if (threadIdx.x == 0) chunk_total[(size_t)r * nchunk + chunk] = tot;
}

// One workgroup per row: exclusive scan of the row's chunk totals (tiles of BS_NT with a carry).
// row_off_hdr == nullptr (pack): row_words[r] is written. Otherwise (unpack) the computed word
// count is compared with the header's (row_off_hdr[r + 1] - row_off_hdr[r]) and a difference
// flags the row (err 4).
__global__ __launch_bounds__(BS_NT) void bs_rowscan_kernel(const int* __restrict__ chunk_total,
                                                           int nchunk, int T, int cb, int w,
                                                           long long* __restrict__ chunk_off,
                                                           long long* __restrict__ row_codes,
                                                           long long* __restrict__ row_words,
                                                           const long long* __restrict__ row_off_hdr,
                                                           int* __restrict__ row_err,
                                                           int* __restrict__ err) {
  __shared__ long long s_w[BS_NT / 64];
  const size_t r = blockIdx.x;
  long long carry = 0;
  for (int c0 = 0; c0 < nchunk; c0 += BS_NT) {
    const int c = c0 + threadIdx.x;
    const long long v = c < nchunk ? chunk_total[r * nchunk + c] : 0;
    long long tot;
    const long long ex = bs_block_scan64(v, s_w, &tot);
    if (c < nchunk) chunk_off[r * nchunk + c] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    const long long words = words_of((long long)T * cb) + words_of(carry * w);
    if (row_codes) row_codes[r] = carry;
    if (row_off_hdr) {
      if (words != row_off_hdr[r + 1] - row_off_hdr[r]) {
        atomicOr(&row_err[r], 4);
        atomicMax(err, 4);
      }
    } else {
      row_words[r] = words;
    }
  }
}

// Exclusive scan over rows (one workgroup, tiles of BS_NT with a running carry).
__global__ __launch_bounds__(BS_NT) void bs_offsets_kernel(const long long* __restrict__ row_words,
                                                           int R, long long* __restrict__ row_off) {
  __shared__ long long s_w[BS_NT / 64];
  long long carry = 0;
  for (int r0 = 0; r0 < R; r0 += BS_NT) {
    const int r = r0 + threadIdx.x;
    const long long v = r < R ? row_words[r] : 0;
    long long tot;
    const long long ex = bs_block_scan64(v, s_w, &tot);
    if (r < R) row_off[r] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) row_off[R] = carry;
}

// ------------------------------------------------------------------------------ pack: write
__global__ __launch_bounds__(BS_NT) void bs_write_kernel(const int64_t* __restrict__ codes,
                                                         const int* __restrict__ counts,
                                                         const long long* __restrict__ chunk_off,
                                                         const long long* __restrict__ row_off,
                                                         int nq, int T, int nchunk, int cb, int w,
                                                         u32* __restrict__ words,
                                                         long long total_words) {
  __shared__ int s_w[BS_NT / 64];
  __shared__ u32 s_bits[BS_WIN];
  const long long r = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const int tid = threadIdx.x;
  const int t = chunk * BS_CHUNK + tid;
  const int c = t < T ? counts[(size_t)r * T + t] : 0;
  const long long row_base = row_off[r];
  const long long row_len = row_off[r + 1] - row_base;
  const long long a_words = words_of((long long)T * cb);

  // plane A: BS_CHUNK * cb bits = 8 cb whole words of this chunk alone
  if (cb > 0) {
    const int nw = BS_CHUNK * cb / 32;                      // <= 64
    if (tid < nw) s_bits[tid] = 0;
    __syncthreads();
    if (t < T) {
      const int p = tid * cb;
      atomicOr(&s_bits[p >> 5], (u32)c << (p & 31));
      if ((p & 31) + cb > 32) atomicOr(&s_bits[(p >> 5) + 1], (u32)c >> (32 - (p & 31)));
    }
    __syncthreads();
    const long long g = (long long)chunk * nw + tid;        // word of plane A
    if (tid < nw && g < a_words && g < row_len && row_base + g < total_words)
      words[row_base + g] = s_bits[tid];
  }

  // plane B
  int tot;
  const int ex = bs_block_scan(c, s_w, &tot);
  if (tot == 0) return;                                     // uniform over the workgroup
  const long long base = chunk_off[(size_t)r * nchunk + chunk];
  const long long b_words = row_len - a_words;
  const long long span_lo = base * w, span_hi = (base + tot) * w;      // bits of plane B
  const long long fw = span_lo >> 5, lw = (span_hi - 1) >> 5;          // first / last word
  const long long p0 = span_lo + (long long)ex * w;                    // this frame's first bit
  u32* out = words + row_base + a_words;
  const u32 field = (1u << w) - 1u;                                    // w <= 16
  for (long long win = fw; win <= lw; win += BS_WIN) {
    const long long wb = win << 5, we = (win + BS_WIN) << 5;           // window, in bits
    const int n = (int)((lw - win + 1) < BS_WIN ? (lw - win + 1) : BS_WIN);
    __syncthreads();                                                   // earlier window stored
    for (int j = tid; j < n; j += BS_NT) s_bits[j] = 0;
    __syncthreads();
    // stages of this frame whose field meets [wb, we)
    const int i_lo = p0 >= wb ? 0 : (int)((wb - p0) / w);
    const int i_hi = p0 >= we ? 0 : (int)(((we - p0 + w - 1) / w) < c ? ((we - p0 + w - 1) / w) : c);
    for (int i = i_lo; i < i_hi; ++i) {
      const u32 v = (u32)codes[((size_t)r * nq + i) * T + t] & field;
      const long long p = p0 + (long long)i * w;
      const long long j = (p >> 5) - win;
      const int sh = (int)(p & 31);
      if (j >= 0 && j < n) atomicOr(&s_bits[j], v << sh);
      if (sh + w > 32 && j + 1 >= 0 && j + 1 < n) atomicOr(&s_bits[j + 1], v >> (32 - sh));
    }
    __syncthreads();
    for (int j = tid; j < n; j += BS_NT) {
      const long long g = win + j;
      if (g >= b_words || row_base + a_words + g >= total_words) continue;   // never out of the row
      const u32 v = s_bits[j];
      if (g == fw || g == lw) {
        if (v) atomicOr(&out[g], v);       // may be shared with the neighbouring chunk
      } else {
        out[g] = v;                        // this chunk's alone
      }
    }
  }
}

// ------------------------------------------------------------------------------ unpack: plan
// Plane A -> counts and chunk totals. Bounds come from the header's row_words (row_off is its
// scan, made on the host): a field outside the row, or a count above nq, flags the row and counts as 0.
__global__ __launch_bounds__(BS_NT) void bs_read_counts_kernel(const u32* __restrict__ words,
                                                               long long total_words,
                                                               const long long* __restrict__ row_off,
                                                               int nq, int T, int nchunk, int cb,
                                                               int* __restrict__ counts,
                                                               int* __restrict__ chunk_total,
                                                               int* __restrict__ row_err,
                                                               int* __restrict__ err) {
  __shared__ int s_w[BS_NT / 64];
  const long long r = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const int t = chunk * BS_CHUNK + threadIdx.x;
  int c = 0;
  if (t < T) {
    if (cb == 0) {
      c = nq;
    } else {
      const long long row_base = row_off[r];
      const long long row_len = row_off[r + 1] - row_base;
      const long long p = (long long)t * cb;
      const long long j = p >> 5;
      const int sh = (int)(p & 31);
      const bool two = sh + cb > 32;
      const long long last = j + (two ? 1 : 0);
      if (row_base < 0 || last >= row_len || row_base + last >= total_words) {
        atomicOr(&row_err[r], 4);
        atomicMax(err, 4);
      } else {
        u32 v = words[row_base + j] >> sh;
        if (two) v |= words[row_base + j + 1] << (32 - sh);
        c = (int)(v & ((1u << cb) - 1u));
        if (c > nq) {
          atomicOr(&row_err[r], 3);
          atomicMax(err, 3);
          c = 0;
        }
      }
    }
    counts[(size_t)r * T + t] = c;
  }
  int tot;
  bs_block_scan(c, s_w, &tot);
  if (threadIdx.x == 0) chunk_total[(size_t)r * nchunk + chunk] = tot;
}

// ------------------------------------------------------------------------------ unpack: read
__global__ __launch_bounds__(BS_NT) void bs_read_kernel(const u32* __restrict__ words,
                                                        long long total_words,
                                                        const int* __restrict__ counts,
                                                        const long long* __restrict__ chunk_off,
                                                        const long long* __restrict__ row_off,
                                                        const int* __restrict__ row_err, int nq,
                                                        int T, int nchunk, int cb, int w, int ncode,
                                                        int64_t* __restrict__ codes,
                                                        float* __restrict__ mask,
                                                        int* __restrict__ err) {
  __shared__ int s_w[BS_NT / 64];
  const long long r = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const int t = chunk * BS_CHUNK + threadIdx.x;
  const bool row_ok = row_err[r] == 0;                      // uniform over the workgroup
  const int c = (t < T && row_ok) ? counts[(size_t)r * T + t] : 0;
  int tot;
  const int ex = bs_block_scan(c, s_w, &tot);
  if (t >= T) return;
  const long long row_base = row_off[r];
  const long long row_len = row_off[r + 1] - row_base;
  const long long a_words = words_of((long long)T * cb);
  const long long b_words = row_len - a_words;
  const long long base = chunk_off[(size_t)r * nchunk + chunk];
  const long long p0 = (base + ex) * w;
  const u32* in = words + row_base + a_words;
  const u32 field = (1u << w) - 1u;                          // w <= 16
  bool bad = false;
  for (int i = 0; i < nq; ++i) {
    const size_t ci = ((size_t)r * nq + i) * T + t;
    long long v = 0;
    bool on = i < c;
    if (on) {
      const long long p = p0 + (long long)i * w;
      const long long j = p >> 5;
      const int sh = (int)(p & 31);
      const bool two = sh + w > 32;
      const long long last = j + (two ? 1 : 0);
      if (row_base < 0 || last >= b_words || row_base + a_words + last >= total_words) {
        on = false;                                         // never outside the row's words
        bad = true;
      } else {
        u32 x = in[j] >> sh;
        if (two) x |= in[j + 1] << (32 - sh);
        x &= field;
        if ((long long)x >= ncode) atomicMax(err, 2);
        v = x;
      }
    }
    codes[ci] = v;
    if (mask) mask[ci] = on ? 1.0f : 0.0f;
  }
  if (bad) atomicMax(err, 4);
}

int code_bits_of(int ncode) {
  int w = 1;
  while ((1 << w) < ncode) ++w;
  return w;
}

int count_bits_of(int nq) {
  int b = 0;
  while (nq >> b) ++b;
  return b;
}

bool shape_ok(int rows, int nq, int frames, int ncode) {
  if (rows <= 0 || nq <= 0 || nq > 255 || frames <= 0 || frames > (1 << 24)) return false;
  if (ncode < 2 || ncode > 65536) return false;
  const long long nchunk = (frames + BS_CHUNK - 1) / BS_CHUNK;
  return (long long)rows * nchunk <= 0x7fffffffLL;
}

}  // namespace

extern "C" int vrvq_bitstream_chunk_frames(void) { return BS_CHUNK; }

extern "C" int vrvq_bitpack_plan(const int64_t* codes, const float* mask, int rows, int nq,
                                 int frames, int ncode, int* counts, int* chunk_total,
                                 long long* chunk_off, long long* row_codes, long long* row_words,
                                 long long* row_off, int* err, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(codes && counts && chunk_total && chunk_off && row_codes && row_words &&
                 row_off && err);
  VRVQ_CHECK_ARG(shape_ok(rows, nq, frames, ncode));
  hipStream_t st = as_stream(stream);
  const int nchunk = (frames + BS_CHUNK - 1) / BS_CHUNK;
  const int cb = mask ? count_bits_of(nq) : 0, w = code_bits_of(ncode);
  hipLaunchKernelGGL(bs_count_kernel, dim3(rows * nchunk), dim3(BS_NT), 0, st, codes, mask, nq,
                     frames, nchunk, ncode, counts, chunk_total, err);
  hipLaunchKernelGGL(bs_rowscan_kernel, dim3(rows), dim3(BS_NT), 0, st, chunk_total, nchunk,
                     frames, cb, w, chunk_off, row_codes, row_words,
                     (const long long*)nullptr, (int*)nullptr, err);
  hipLaunchKernelGGL(bs_offsets_kernel, dim3(1), dim3(BS_NT), 0, st, row_words, rows, row_off);
  return vrvq_launch_status();
}

extern "C" int vrvq_bitpack_write(const int64_t* codes, const int* counts,
                                  const long long* chunk_off, const long long* row_off, int rows,
                                  int nq, int frames, int ncode, int count_bits, uint32_t* words,
                                  long long total_words, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(codes && counts && chunk_off && row_off && total_words >= 0);
  VRVQ_CHECK_ARG(shape_ok(rows, nq, frames, ncode));
  VRVQ_CHECK_ARG(count_bits == 0 || count_bits == count_bits_of(nq));
  if (total_words == 0) return 0;
  VRVQ_CHECK_ARG(words);
  hipStream_t st = as_stream(stream);
  const int nchunk = (frames + BS_CHUNK - 1) / BS_CHUNK;
  if (hipMemsetAsync(words, 0, (size_t)total_words * 4, st) != hipSuccess)
    return vrvq_launch_status();
  hipLaunchKernelGGL(bs_write_kernel, dim3(rows * nchunk), dim3(BS_NT), 0, st, codes, counts,
                     chunk_off, row_off, nq, frames, nchunk, count_bits, code_bits_of(ncode),
                     words, total_words);
  return vrvq_launch_status();
}

extern "C" int vrvq_bitunpack_plan(const uint32_t* words, long long total_words,
                                   const long long* row_off, int rows, int nq, int frames,
                                   int ncode, int count_bits, int* counts, int* chunk_total,
                                   long long* chunk_off, int* row_err, int* err,
                                   vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(row_off && counts && chunk_total && chunk_off && row_err && err);
  VRVQ_CHECK_ARG(total_words >= 0 && (words || total_words == 0));
  VRVQ_CHECK_ARG(shape_ok(rows, nq, frames, ncode));
  VRVQ_CHECK_ARG(count_bits == 0 || count_bits == count_bits_of(nq));
  hipStream_t st = as_stream(stream);
  const int nchunk = (frames + BS_CHUNK - 1) / BS_CHUNK;
  hipLaunchKernelGGL(bs_read_counts_kernel, dim3(rows * nchunk), dim3(BS_NT), 0, st, words,
                     total_words, row_off, nq, frames, nchunk, count_bits, counts, chunk_total,
                     row_err, err);
  hipLaunchKernelGGL(bs_rowscan_kernel, dim3(rows), dim3(BS_NT), 0, st, chunk_total, nchunk,
                     frames, count_bits, code_bits_of(ncode), chunk_off, (long long*)nullptr,
                     (long long*)nullptr, row_off, row_err, err);
  return vrvq_launch_status();
}

extern "C" int vrvq_bitunpack_read(const uint32_t* words, long long total_words,
                                   const int* counts, const long long* chunk_off,
                                   const long long* row_off, const int* row_err, int rows, int nq,
                                   int frames, int ncode, int count_bits, int64_t* codes,
                                   float* mask, int* err, vrvq_stream_t stream) {
  VRVQ_CHECK_ARG(counts && chunk_off && row_off && row_err && codes && err);
  VRVQ_CHECK_ARG(total_words >= 0 && (words || total_words == 0));
  VRVQ_CHECK_ARG(shape_ok(rows, nq, frames, ncode));
  VRVQ_CHECK_ARG(count_bits == 0 || count_bits == count_bits_of(nq));
  const int nchunk = (frames + BS_CHUNK - 1) / BS_CHUNK;
  hipLaunchKernelGGL(bs_read_kernel, dim3(rows * nchunk), dim3(BS_NT), 0, as_stream(stream), words,
                     total_words, counts, chunk_off, row_off, row_err, nq, frames, nchunk,
                     count_bits, code_bits_of(ncode), ncode, codes, mask, err);
  return vrvq_launch_status();
}
