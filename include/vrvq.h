/*
 * vrvq.h — C-ABI of the MI355X (gfx950) VRVQ hot path: encode -> residual VQ -> decode.
 *
 * The reference (lixinghe1999/VRVQ) has no FFI layer: its operator surface is the Python
 * module API of models/layers.py, models/quantize.py, models/utils.py and
 * models/dac_vrvq.py. Every entry point below replaces one reference operator (cited
 * file:line) and is bound from Python by ctypes in vrvq_amd/_lib.py (INTEGRATION.md shows
 * the binding a maintainer would add on the reference side).
 *
 * Conventions
 *   - All tensors are contiguous, row-major, in device (HBM) memory; fp32 unless noted.
 *   - The caller owns every buffer (inputs, outputs, workspaces); nothing is allocated here.
 *   - Every call is asynchronous on `stream` (a hipStream_t; NULL = legacy default stream)
 *     and graph-capturable (no allocation, no host sync inside).
 *   - Return value: 0 on success, otherwise a vrvq_status_t (argument errors, detected
 *     on the host before any launch) or the hipError_t of the failed launch.
 *     vrvq_status_string() turns either into text.
 */
#ifndef VRVQ_H_
#define VRVQ_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vrvq_stream_t; /* hipStream_t */

enum vrvq_status_t {
  VRVQ_OK = 0,
  VRVQ_ERR_ARG = 10001,      /* null pointer / non-positive size / unsupported shape */
  VRVQ_ERR_UNSUPPORTED = 10002 /* shape outside the instantiated kernel set */
};

/* Conv epilogue selector (vrvq_conv1d.epilogue). */
enum vrvq_epilogue_t { VRVQ_EPI_NONE = 0, VRVQ_EPI_TANH = 1, VRVQ_EPI_SIGMOID = 2 };

const char* vrvq_status_string(int status);
/* Library version (major*10000 + minor*100 + patch). */
int vrvq_version(void);

/* ---------------------------------------------------------------------------------------
 * Weight preparation (once per load_state_dict; the reference recomputes weight norm on
 * every forward via the torch.nn.utils.weight_norm pre-hook).
 * ------------------------------------------------------------------------------------- */

/* w[r, :] = v[r, :] * (g[r] / ||v[r, :]||_2), r < rows, row length = cols.
 * Replaces torch.nn.utils.weight_norm(dim=0) as used by WNConv1d / WNConvTranspose1d
 * (models/layers.py:17-22). For Conv1d rows = Cout, cols = Cin*k; for ConvTranspose1d
 * rows = Cin, cols = Cout*k (weight-norm dim 0 is in_channels there). */
int vrvq_weight_norm(const float* g, const float* v, int rows, int cols, float* w,
                     vrvq_stream_t stream);

/* inv[c] = 1 / (alpha[c] + 1e-9f). Snake's reciprocal, models/layers.py:30. */
int vrvq_snake_inv_alpha(const float* alpha, int channels, float* inv, vrvq_stream_t stream);

/* y[b,c,t] = snake_c(x[b,c,t]) = x + inv_alpha[c] * sin(alpha[c] * x)^2 (Snake1d forward,
 * models/layers.py:26-32; the same per-element expression the conv kernels apply while
 * staging). The training step's weight gradients take snake(x) from here once instead of
 * re-evaluating it in every (row tile, chunk) that stages x. y may not alias x. */
int vrvq_snake(const float* x, int batch, int channels, int frames, const float* alpha,
               const float* inv_alpha, float* y, vrvq_stream_t stream);

/* Phase-split view y[b][c*stride + r][m] = snake_c(x[b][c][m*stride + r - pad]) (alpha NULL: no
 * Snake; 0 outside [0, frames)), m < out_frames, stride a power of two. Turns a stride-s
 * product over k = 2s taps (j = q s + r) into a stride-1 2-tap one: the training step's weight
 * gradients of the strided WNConv1d (models/layers.py:79-85) and WNConvTranspose1d
 * (:97-103) run on the x3 kernel over it. y may not alias x. */
int vrvq_phase_split(const float* x, int batch, int channels, int frames, int stride, int pad,
                     int out_frames, const float* alpha, const float* inv_alpha, float* y,
                     vrvq_stream_t stream);

/* Codebook normalisation for VectorQuantize.decode_latents (models/quantize.py:92-99):
 * cbn[n,:] = cb[n,:] / max(||cb[n,:]||, 1e-12); c2[n] = sum_k cbn[n,k]^2.
 * cb is [rows][dim] (rows = nq * codebook_size for a stacked RVQ). */
int vrvq_codebook_prep(const float* cb, int rows, int dim, float* cbn, float* c2,
                       vrvq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Snake-fused 1-D convolution (implicit GEMM on v_mfma_f32_32x32x2_f32).
 *
 *   y[b,co,t] = epi( residual[b,co,t] + (bias[co] + sum_{ci,k} W[co,ci,k] *
 *                    snake_ci(x[b,ci, t*stride - pad + k*dil])) )
 *   snake_c(v) = v + inv_alpha[c] * sin(alpha[c]*v)^2     (skipped when alpha == NULL)
 *
 * Replaces Snake1d -> WNConv1d (models/layers.py:26-41, 17-18) and the ResidualUnit skip
 * (models/layers.py:63-68), EncoderBlock / Encoder / Decoder convs
 * (models/layers.py:71-89, models/dac_vrvq.py:19-80), the ImportanceSubnet convs + Sigmoid
 * (models/importance_subnet.py:38-45) and the decoder Tanh (models/dac_vrvq.py:74).
 *
 * w_packed: [Cin][k][cout_pad] (cout_pad >= Cout, multiple of 128, zero padded) as produced
 * by vrvq_pack_conv1d_weight. residual (nullable) has the output's shape.
 * tout must equal floor((tin + 2*pad - dil*(k-1) - 1)/stride) + 1.
 *
 * Producer-side Snake: when y_snake != NULL the epilogue also writes
 *   y_snake[b,co,t] = snake_co(y[b,co,t]) with alpha_out / inv_alpha_out ([Cout]),
 * i.e. the Snake1d that the NEXT layer applies to this output (models/layers.py:52-110: every
 * consumer of a conv output starts with a Snake). The consumer then runs with alpha == NULL,
 * so the activation is evaluated once per element instead of once per consumer tile. y may be
 * NULL when only the activated tensor is needed (it must not be NULL otherwise).
 *
 * Alignment: x, residual, y and y_snake must be 16-byte aligned (where a row length is a
 * multiple of 4 the kernels move rows as 16-byte vectors and assume it); the same holds for
 * vrvq_conv1d_ws, vrvq_conv1d_proj, vrvq_conv_transpose1d* and vrvq_residual_unit (x, x_snk, y,
 * y_snake). The entry points do not check it.
 * ------------------------------------------------------------------------------------- */
int vrvq_conv1d(const float* x, int batch, int cin, int tin, const float* alpha,
                const float* inv_alpha, const float* w_packed, const uint16_t* w_x3, int cout,
                int cout_pad, int k,
                int stride, int pad, int dil, const float* bias, const float* residual,
                int epilogue, float* y, int tout, const float* alpha_out,
                const float* inv_alpha_out, float* y_snake, vrvq_stream_t stream);

/* vrvq_conv1d with a caller-owned workspace (device memory, >= the bytes vrvq_conv1d_workspace
 * gives for the same shape, or NULL): the deep-K layers at tout <= 96 on the x3 path (the
 * EncoderBlock's 512 -> 1024 stride-8 conv, the ImportanceSubnet's k3 convs, the decoder's
 * first k7; models/dac_vrvq.py:32-35, 62-63, models/importance_subnet.py:38-45) then split
 * their K loop into parts whose partial sums the workspace holds, added in part order by the
 * epilogue launch. The part count depends on the layer's shape only (a clip's output does not
 * change with the batch); the sums differ from vrvq_conv1d's (unsplit) by fp32 rounding.
 * vrvq_conv1d_workspace: *bytes = 0 where no split applies (x3 = w_x3 != NULL). */
int vrvq_conv1d_workspace(int batch, int cin, int tin, int cout, int k, int stride, int pad,
                          int dil, int x3, long long* bytes);
int vrvq_conv1d_ws(const float* x, int batch, int cin, int tin, const float* alpha,
                   const float* inv_alpha, const float* w_packed, const uint16_t* w_x3, int cout,
                   int cout_pad, int k, int stride, int pad, int dil, const float* bias,
                   const float* residual, int epilogue, float* y, int tout,
                   const float* alpha_out, const float* inv_alpha_out, float* y_snake,
                   void* workspace, long long ws_bytes, vrvq_stream_t stream);

/* fp32 convolution on the bf16 matrix cores (the "x3" path, vrvq_amd/csrc/conv_x3.h): with
 * w_x3 = vrvq_pack_x3_weight(w_packed) (null: the fp32-input MFMA path) the stride-1 convs
 * (k in {1, 2, 3, 7}; also the ConvTranspose1d and the ResidualUnit's k7) split both operands
 * exactly into three bf16 terms and accumulate the six products >= 2^-16 of each fp32
 * product in fp32 — fp32 accuracy at 2.7x the MFMA ceiling. A strided conv (k = 2 stride,
 * stride a power of two: the EncoderBlock downsamplers, models/layers.py:83-88) given w_x3 runs
 * as a stride-1 2-tap conv over the phase-split view xv[c*s + r][m] = x[c][m*s + r - pad]:
 * w_x3 then holds vrvq_pack_x3_weight(cin * stride, k = 2) of the packed phase-split weight
 * W'[co][c*s + r][j] = W[co][c][j*s + r] (other strided shapes: VRVQ_ERR_UNSUPPORTED).
 * vrvq_x3_weight_size gives the buffer length in uint16 elements. */
int vrvq_x3_weight_size(int cin, int k, int cout_pad, long long* n_u16);
int vrvq_pack_x3_weight(const float* w_packed, int cin, int k, int cout_pad, uint16_t* w_x3,
                        vrvq_stream_t stream);

/* The encoder's last conv (Snake1d -> WNConv1d k3, models/dac_vrvq.py:33-34; stride 1, no
 * residual / epilogue, cout == 1024) with the in_proj of every RVQ stage in its epilogue
 * (models/quantize.py:65, VectorQuantize.in_proj applied to z for all stages at once, without
 * bias): part[s][b*tout + t][r] = sum_{c in 128 s .. 128 s + 127} W_in[r][c] z[b][c][t] for the
 * 8 channel splits s and r < 8 nq -- vrvq_rvq_project's partials bit for bit (its x3 variant),
 * computed from the conv's accumulators, so the quantizer never reads z back (vrvq_rvq_encode_part
 * takes part). w3in = vrvq_rvq_pack_w_in(w_in_t). y (nullable) also receives z [B][1024][tout]
 * as vrvq_conv1d writes it. part: [8][B*tout][8 nq] fp32, 16-byte aligned. workspace /
 * ws_bytes: as vrvq_conv1d_ws (vrvq_conv1d_workspace of the same shape; with it the conv splits
 * its K loop exactly as vrvq_conv1d_ws does, so z is the same bits either way). */
int vrvq_conv1d_proj(const float* x, int batch, int cin, int tin, const float* alpha,
                     const float* inv_alpha, const float* w_packed, const uint16_t* w_x3, int cout,
                     int cout_pad, int k, int pad, int dil, const float* bias, float* y, int tout,
                     const uint16_t* w3in, int nq, float* part, void* workspace,
                     long long ws_bytes, vrvq_stream_t stream);

/* Debug query (host only, no launch): tile and path of the last conv launch on the MFMA tiles
 * (vrvq_conv1d / _ws / _proj, vrvq_conv_transpose1d*), process-wide: out = {BM, BN, KS (the
 * GEMM's taps: 2 for the phase-split view), x3 (0: fp32-input loop, 1: x3 on plain K chunks,
 * 2: x3 on pair chunks), S (split-K parts, 0: unsplit)}; all 0 before the first such launch.
 * The tests use it to assert the tile they claim to pin. */
int vrvq_conv_last_launch(int out[5]);

/* Debug query (host only, touches no device; library version 104): what a conv call of this
 * shape would launch, decided by the code that launches it, and the status that call would
 * return (VRVQ_ERR_UNSUPPORTED etc.; out is then left alone). kind: vrvq_conv1d / _ws,
 * vrvq_conv1d_proj (stride 1), vrvq_conv_transpose1d_pad (k = 2 stride, dil 1); cout_pad is
 * taken as the packers give it (cout rounded up to 128; the ConvTranspose's cout * stride rows
 * to 128, or to 192 where the stride does not divide 128), has_x3 = w_x3 != NULL,
 * has_workspace = a workspace of vrvq_conv1d_workspace bytes, alpha = NULL.
 * out = the five vrvq_conv_last_launch fields, then path (0: an MFMA tile; 1: the small-Cout
 * kernels, 2: the Cin = 1 stream kernel, which leave the tile fields 0 and make no
 * vrvq_conv_last_launch record) and WM (wave rows of the tile). */
enum vrvq_plan_kind_t { VRVQ_PLAN_CONV = 0, VRVQ_PLAN_PROJ = 1, VRVQ_PLAN_CONV_TRANSPOSE = 2 };
int vrvq_conv_plan(int kind, int batch, int cin, int tin, int cout, int k, int stride, int pad,
                   int dil, int has_x3, int has_workspace, int out[7]);

/* Pack a folded Conv1d weight w[Cout][Cin][k] into [Cin][k][cout_pad]. */
int vrvq_pack_conv1d_weight(const float* w, int cout, int cin, int k, int cout_pad,
                            float* w_packed, vrvq_stream_t stream);

/* Fused ResidualUnit (models/layers.py:52-68), stride 1, k = 7 then k = 1, C channels:
 *   y = x + b1 + W1 * snake2(b7 + W7 *_dil x_snk),   x_snk = snake1(x) (given)
 * with y and / or y_snake = snake_out(y) written (as vrvq_conv1d's out_snake). The
 * intermediate snake2(...) stays in LDS. Same expressions as vrvq_conv1d(k7, out_snake =
 * snake2, no raw) followed by vrvq_conv1d(k1, residual = x) — bit-identical where both use the
 * same k7 tile height (C <= 192), else the same sums in another fp32 order. Packed by
 * vrvq_pack_conv1d_weight (same cout_pad). Supported: C in {64, 96, 128, 192, 256}, dil <= 9;
 * other C return VRVQ_ERR_UNSUPPORTED (callers use the two-launch form). w7_x3 / w1_x3
 * (nullable, vrvq_pack_x3_weight of w7_packed / w1_packed): the x3 path for the k7 GEMM and,
 * where the split hs planes fit in LDS (C = 64 / 96 / 192), the k1 GEMM. */
int vrvq_residual_unit(const float* x, const float* x_snk, int batch, int channels, int frames,
                       int dil, const float* w7_packed, const uint16_t* w7_x3,
                       const uint16_t* w1_x3, const float* b7,
                       const float* alpha2,
                       const float* inv_alpha2, const float* w1_packed, const float* b1,
                       int cout_pad, float* y, const float* alpha_out,
                       const float* inv_alpha_out, float* y_snake, vrvq_stream_t stream);

/* Snake-fused ConvTranspose1d, kernel = 2*stride, padding = stride/2 (even stride), i.e.
 * the DecoderBlock upsampler (models/layers.py:92-103): y has length tin*stride.
 * Computed as a polyphase 2-tap conv with cout*stride phase-channels:
 *   y[b,co,m*s+r-p] = bias[co] + sum_ci W[ci,co,r]*xs[ci,m] + W[ci,co,r+s]*xs[ci,m-1].
 * w_packed from vrvq_pack_convt1d_weight ([Cin][2][cout_pad]: cout*stride padded to a
 * multiple of 128, or of 192 for strides that do not divide 128). Strides 5, 7, ... return
 * VRVQ_ERR_UNSUPPORTED (a tile must hold whole output channels).
 * alpha_out / inv_alpha_out / y_snake: producer-side Snake as in vrvq_conv1d. */
int vrvq_conv_transpose1d(const float* x, int batch, int cin, int tin, const float* alpha,
                          const float* inv_alpha, const float* w_packed, int cout,
                          int cout_pad, int stride, const float* bias, float* y,
                          const float* alpha_out, const float* inv_alpha_out, float* y_snake,
                          vrvq_stream_t stream);

/* vrvq_conv_transpose1d with an explicit padding 0 <= pad < stride: y has length
 * (tin - 1)*stride - 2*pad + 2*stride. pad = 0 is the padding=False window of the chunked
 * codec (CodecMixin.padding setter, models/dac_base.py:68-84: every conv's padding -> 0). */
int vrvq_conv_transpose1d_pad(const float* x, int batch, int cin, int tin, const float* alpha,
                              const float* inv_alpha, const float* w_packed,
                              const uint16_t* w_x3, int cout,
                              int cout_pad, int stride, int pad, const float* bias, float* y,
                              const float* alpha_out, const float* inv_alpha_out,
                              float* y_snake, vrvq_stream_t stream);

/* Pack a folded ConvTranspose1d weight w[Cin][Cout][2*stride] into the polyphase layout. */
int vrvq_pack_convt1d_weight(const float* w, int cin, int cout, int stride, int cout_pad,
                             float* w_packed, vrvq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Residual vector quantisation (VBRResidualVectorQuantize.forward, models/quantize.py:328-443;
 * per stage VectorQuantize.forward/decode_latents, models/quantize.py:42-103). Per frame (b,t)
 * and stage i:
 *   z_e   = W_in[i] r + b_in[i]                    (in_proj, WN k=1 conv D->d)
 *   e     = z_e / max(||z_e||, 1e-12)
 *   idx   = argmin_n ( (sum e^2 - 2 e.cbn[i,n]) + c2[i,n] ), lowest n on ties
 *   zq    = cb[i, idx]                             (raw codebook row)
 *   loss  = mean_k (z_e - zq)^2                    (commitment == codebook loss in forward)
 *   zst   = z_e + (zq - z_e)                       (straight-through value)
 *   r    -= W_out[i] zst + b_out[i]                (out_proj, WN k=1 conv d->D)
 * By linearity of in_proj / out_proj,
 *   z_e(i) = ((P_i + b_in[i]) - Qb_i) - sum_{j<i} M_ij zst_j,
 *   P_i = W_in[i] z,  M_ij = W_in[i] W_out[j] (8x8),  Qb_i = W_in[i] sum_{j<i} b_out[j],
 * so the sequential chain runs in the 8-dim latent space (vrvq_rvq_chain) between two
 * parallel 1024-dim passes: the projection of z for every stage (vrvq_rvq_project) and the
 * expansion of z_q_is / z_q with the reference's out_proj expression (vrvq_rvq_expand).
 *
 *   z       [B][D][T]         encoder output
 *   w_in_t  [nq][D][d]        folded in_proj weight, transposed (d fastest)
 *   b_in    [nq][d]
 *   cb      [nq][N][d]        raw codebooks; c2 [nq][N] squared norms of the normalised rows
 *   cbf     [nq][8][64][N/128][2]  normalised codebooks in the chain's MFMA fragment order
 *                             (vrvq_rvq_frag of vrvq_codebook_prep's cbn)
 *   w_out   [nq][D][d]        folded out_proj weight; b_out [nq][D]
 *   imp     [B][T] importance map, or NULL (CBR: mask = 1, models/quantize.py:397-400)
 *   level   s[b,t] = (imp[b,t] * level) * nq, mask[b,i,t] = (s - i >= 0)   (models/quantize.py:389,
 *           models/utils.py:45-61)
 * outputs:
 *   codes   [B][nq][T] int64  (torch argmax indices)
 *   latents [B][nq*d][T]      concatenated z_e
 *   loss_pf [B][nq][T]        per-frame loss
 *   z_q_is  [B][nq][D][T]     per-stage out_proj values (or NULL: not materialised)
 *   z_q     [B][D][T]         sum_i mask[b,i,t] * z_q_is[b,i,:,t], stage order
 *   mask    [B][nq][T]        (or NULL)
 * Supported: D == 1024 (latent_dim of every shipped config), d == 8, nq <= 32,
 * N % 256 == 0 and N <= 1024.
 * ------------------------------------------------------------------------------------- */

/* Once per weight version: mcol [nq][nq][d][d] with mcol[j][i] = M_ij for i > j (else 0) and
 * qb [nq][d]. */
int vrvq_rvq_cross_prep(const float* w_in_t, const float* w_out, const float* b_out, int nq,
                        int dim, int cdim, float* mcol, float* qb, vrvq_stream_t stream);
/* The same with every entry accumulated in fp64 and rounded once (the training step: the fp32
 * chain's 1e-6 of |M| dominates the error of the quantizer's gradients). */
int vrvq_rvq_cross_prep_precise(const float* w_in_t, const float* w_out, const float* b_out, int nq,
                                int dim, int cdim, float* mcol, float* qb, vrvq_stream_t stream);

/* Once per weight version: cbf[i][w][l][t][h] = cbn[i][w*N/8 + 16t + (l&15)][4h + (l>>4)]. */
int vrvq_rvq_frag(const float* cbn, int nq, int ncode, int cdim, float* cbf,
                  vrvq_stream_t stream);

/* The library reads no environment variable. The projection of vrvq_rvq_project /
 * vrvq_rvq_encode is one kernel: one workgroup per clip x channel split on the bf16 matrix cores
 * with both operands split exactly into three bf16 terms (six products, fp32 accuracy). */

/* Bytes of a workspace that is enough for vrvq_rvq_encode at this shape: an upper bound kept for
 * the ABI (since version 107 the call needs less: the projection partials, 256 batch frames nq
 * bytes, followed by vrvq_rvq_workspace_part's bytes, and it accepts any workspace that holds
 * those). */
int vrvq_rvq_workspace(int batch, int frames, int nq, long long* bytes);

/* RVQ launch structure (process-wide): 2 = the fused launch (default): the quantizer runs from
 * the projection partials as rvq_pt_kernel per group of resident clips, in vrvq_rvq_encode_part
 * and, after its projection launch, in vrvq_rvq_encode. 1 = never fused: chain and expansion as
 * two launches (vrvq_rvq_encode: project -> chain -> expand): the A/B and the tests' reference.
 * Both structures give the same outputs bit for bit. path 0 queries. Returns the previous path
 * (1 or 2), or VRVQ_ERR_ARG. */
int vrvq_rvq_path(int path);

/* The fused launch's in-kernel waits are bounded. A wait that runs out (a hang averted: it
 * cannot happen with the whole grid resident) records a code in the stream's sync block and in
 * a host-mapped word of the process, and the workgroup POISONS its outputs (z_q / z_q_is NaN)
 * instead of passing garbage off as results. The code is 2: an expansion workgroup's wait for a
 * stage of the chain (1 was a wait of the kernel retired in version 107; nothing reports it).
 * vrvq_rvq_sync_error: *code = the stream's word or 0, and clears it; synchronises the stream.
 * vrvq_rvq_pending_error: *code = the process word or 0 (a timeout of any launch that has
 * completed by now), and clears it; no synchronisation -- the torch ops call it at entry and
 * raise RuntimeError on a nonzero code.
 * vrvq_rvq_debug: test hook -- every later fused launch bounds its waits at spin_max polls
 * (0: the default ~0.5 s) and delays the first chain part by stall x s_sleep(127). */
int vrvq_rvq_sync_error(vrvq_stream_t stream, int* code);
int vrvq_rvq_pending_error(int* code);
int vrvq_rvq_debug(unsigned spin_max, unsigned stall);

/* Kernel timing of the fused launch (bench.py's roofline): while on (process-wide), every
 * rvq_pt_kernel launch (of vrvq_rvq_encode_part and vrvq_rvq_encode; not the projection, chain
 * or expansion launches) carries a pair of HIP events in its own dispatch
 * (hipExtLaunchKernelGGL), i.e. the kernel's duration on its stream. Returns the previous
 * setting. vrvq_rvq_timing_read waits for the recorded launches and returns the mean duration
 * (ms) and their count, then forgets them. */
int vrvq_rvq_timing(int on);
int vrvq_rvq_timing_read(float* mean_ms, int* count);

/* W_in planes of vrvq_conv1d_proj's projection epilogue (once per weight version,
 * vrvq_rvq_w_in_planes_size uint16 elements): the three bf16 terms of W_in in the
 * v_mfma_f32_16x16x32_bf16 A-fragment order. */
int vrvq_rvq_w_in_planes_size(int nq, int dim, int cdim, long long* n_u16);
int vrvq_rvq_pack_w_in(const float* w_in_t, int nq, int dim, int cdim, uint16_t* w3in,
                       vrvq_stream_t stream);

/* The whole quantizer from the projection partials of vrvq_conv1d_proj (the eval encode's path):
 * ONE launch per group of resident clips (rvq_pt_kernel): chain parts (<= 16 frames of a clip)
 * sum their frames' 8 partials in split order, run the 8-dim chain and publish every stage's zst
 * rows as tagged granules; expansion workgroups (clip, 96 frames, 128 channels; one loader wave
 * polls the stage rows into LDS while seven waves write the previous stage) write z_q_is / z_q
 * under the chain. Outputs, layouts and expressions as vrvq_rvq_encode, and equal to its three
 * launches bit for bit. When a clip does not fit the resident grid (very long clips; see
 * vrvq_rvq_fused_clips) or vrvq_rvq_path(1) is set, the chain and the expansion run as two
 * stream-ordered launches over the same partials (zst rows through the workspace), with the same
 * outputs. workspace: >= vrvq_rvq_workspace_part bytes, 16-byte aligned (eager fused calls hand
 * off through the library's granule area; under stream capture the granules and the sync block
 * live in the workspace, zeroed by captured memsets). Replaces models/quantize.py:353-365,
 * 389-421 like vrvq_rvq_encode. */
int vrvq_rvq_workspace_part(int batch, int frames, int nq, int ncode, long long* bytes);
int vrvq_rvq_encode_part(const float* part, int batch, int dim, int frames, int nq, int ncode,
                         int cdim, const float* b_in, const float* cb, const float* cbf,
                         const float* c2, const float* w_out, const float* b_out,
                         const float* mcol, const float* qb, const float* imp, float level,
                         int64_t* codes, float* latents, float* loss_pf, float* z_q_is,
                         float* z_q, float* mask, void* workspace, long long workspace_bytes,
                         vrvq_stream_t stream);
/* Clips one rvq_pt_kernel launch holds resident (0: vrvq_rvq_encode_part takes its two-launch
 * form). vrvq_rvq_debug_capacity: test hook capping that number (0 forces the two launches, a
 * negative value removes the cap); returns the previous cap. */
int vrvq_rvq_fused_clips(int frames, int nq, int ncode, int* clips);
int vrvq_rvq_debug_capacity(int clips);

/* Debug query (library version 105): the launch plan of a vrvq_rvq_encode_part call of this
 * shape (and of vrvq_rvq_encode after its projection launch), filled by the function its launcher, vrvq_rvq_workspace_part and vrvq_rvq_fused_clips
 * use. resident = workgroups of rvq_pt_kernel the device holds at once; given (> 0), the query
 * is host-only and touches no device; 0 asks the current device (its occupancy query).
 * out = {kind, F (frames per chain part, <= 16), P (parts per clip), n_fb (96-frame expansion
 * windows per clip), workgroups per clip (P + 8 n_fb), dynamic LDS bytes, resident, clips per
 * launch (0: chain + expand), launches, workspace bytes (= vrvq_rvq_workspace_part)}. The two
 * process-wide test hooks, vrvq_rvq_path(1) and vrvq_rvq_debug_capacity, show in kind, clips
 * and launches. Status as vrvq_rvq_workspace_part. */
enum vrvq_rvq_plan_kind_t { VRVQ_RVQ_PLAN_PT = 0, VRVQ_RVQ_PLAN_CHAIN_EXPAND = 1 };
int vrvq_rvq_plan(int batch, int frames, int nq, int ncode, int resident, long long out[10]);

/* The whole quantizer, the replacement of VBRResidualVectorQuantize.forward's quantizer loop,
 * importance mask and masked sum (models/quantize.py:353-365, 389-421) and of
 * ResidualVectorQuantize.forward in eval (:136-214), on channel-major z: the projection launch
 * (step 1 below) writes the partials into the workspace, then the quantizer runs from them
 * exactly as vrvq_rvq_encode_part does, at any number of frames (rvq_pt_kernel per group of
 * resident clips; chain -> expand, steps 2 and 3, under vrvq_rvq_path(1) or for a clip longer
 * than the resident grid). The fused launch hands data between its workgroups as tagged 8-byte
 * granules (the tag carries a per-call epoch from ONE process-wide counter, so nothing needs
 * clearing between eager calls on any stream): eager calls use a library-owned granule area
 * per (device, stream), allocated with the stream's sync block on first use (hipMalloc, outside
 * any stream capture); under stream capture the granules live in the workspace, and memsets of
 * them and of the sync block are captured in front of each launch (every replay uses epoch 1).
 * workspace: vrvq_rvq_workspace() bytes are always enough (see there), 16-byte aligned,
 * caller-owned, no initialisation needed. */
int vrvq_rvq_encode(const float* z, int batch, int dim, int frames, int nq, int ncode, int cdim,
                    const float* w_in_t, const float* b_in, const float* cb, const float* cbf,
                    const float* c2, const float* w_out, const float* b_out, const float* mcol,
                    const float* qb, const float* imp, float level, int64_t* codes,
                    float* latents, float* loss_pf, float* z_q_is, float* z_q, float* mask,
                    void* workspace, long long workspace_bytes, vrvq_stream_t stream);

/* Step 1: P partial sums over 8 channel splits: part [8][B*T][nq*d], part[s][b*T+t][i*d+k] =
 * sum_{c in split s} W_in[i][k][c] z[b][c][t] (in_proj without bias, all stages at once). */
int vrvq_rvq_project(const float* z, int batch, int dim, int frames, int nq, int cdim,
                     const float* w_in_t, float* part, vrvq_stream_t stream);

/* Step 2: the 8-dim chain over all nq stages (P = sum of the 8 partials in split order).
 * Outputs codes, latents (= z_e), loss_pf, zst [B][nq][T][d] (straight-through rows, the input
 * of step 3) and mask (or NULL). */
int vrvq_rvq_chain(const float* part, int batch, int frames, int nq, int ncode, int cdim,
                   const float* b_in, const float* qb, const float* mcol, const float* cb,
                   const float* cbf, const float* c2, const float* imp, float level,
                   int64_t* codes, float* latents, float* loss_pf, float* zst, float* mask,
                   vrvq_stream_t stream);

/* Step 3: HBM-streaming expansion + importance gating.
 *   z_q_is[b,i,:,t] = W_out[i] zst[b,i,t] + b_out[i]          (models/quantize.py:77)
 *   z_q[b,:,t]      = sum_i mask[b,i,t] * z_q_is[b,i,:,t]     (models/quantize.py:420-421)
 * imp == NULL: mask = 1 (CBR, and from_codes). z_q_is may be NULL (not materialised); mask, if
 * not NULL, receives the mask. Also the second half of from_codes (models/quantize.py:217-249)
 * after vrvq_rvq_gather. */
int vrvq_rvq_expand(const float* zst, int batch, int dim, int frames, int nq, int cdim,
                    const float* w_out, const float* b_out, const float* imp, float level,
                    float* z_q_is, float* z_q, float* mask, vrvq_stream_t stream);

/* Codes -> latents gather (decode_code of every stage, models/quantize.py:81-85, as used by
 * ResidualVectorQuantize.from_codes, :217-249):
 *   z_p[b, i*d + k, t] = cb[i][codes[b,i,t]][k]   (raw codebook rows, [B][nq*d][T]) or NULL
 *   zst[b][i][t][k]    = the same rows, the input layout of vrvq_rvq_expand, or NULL
 * A code outside [0, ncode) sets *err = 1 (err may be NULL) and reads row 0: the caller raises
 * IndexError as F.embedding does. */
int vrvq_rvq_gather(const int64_t* codes, int batch, int nq, int frames, const float* cb,
                    int ncode, int cdim, float* zst, float* z_p, int* err, vrvq_stream_t stream);

/* Masked loss reduction (models/quantize.py:422-423): out[0] = (loss_pf*mask).sum(1).mean().
 * One workgroup, fixed order (deterministic). */
int vrvq_masked_loss(const float* loss_pf, const float* mask, int batch, int nq, int frames,
                     float* out, vrvq_stream_t stream);

/* generate_mask_hard (models/utils.py:55-61): mask[b,n,t] = (s[b,t] - n >= 0). s is [B][T]. */
int vrvq_mask_hard(const float* s, int batch, int frames, int nq, float* mask,
                   vrvq_stream_t stream);

/* Scaled importance map: s[b,t] = (imp[b,t] * a) * c (two separate fp32 roundings, matching
 * `imp_map * level * n_codebooks` at models/quantize.py:389 with a=level, c=nq, and
 * `imp_map * (level*n_q)` at scripts/inference.py:96-97 with a=level*n_q, c=1). */
int vrvq_scale_imp(const float* imp, int n, float a, float c, float* s, vrvq_stream_t stream);

/* Masked sum over codebooks (scripts/inference.py:99-100):
 * z_q[b,:,t] = sum_i mask[b,i,t] * z_q_is[b,i,:,t]. */
int vrvq_masked_sum(const float* z_q_is, const float* mask, int batch, int nq, int dim,
                    int frames, float* z_q, vrvq_stream_t stream);

/* cal_bpf_from_mask (models/utils.py:64-73): out[0] = sum(mask*bits[n]) / (B*T). */
int vrvq_bpf(const float* mask, const float* bits, int batch, int nq, int frames, float* out,
             vrvq_stream_t stream);

/* Rate control from the importance map alone (codes, latents and z_q_is do not depend on the
 * level). The frame count is the RVQ kernels' own expression, two fp32 roundings:
 *   s = fl(fl(imp * level) * (float)nq)
 *   n(imp, level) = s >= 0 ? (int)floorf(fminf(s, nq - 1)) + 1 : 0        (NaN gives 0)
 * and a frame costs cum[n] bits, cum the prefix sum of bits[nq] (int32, device). All totals are
 * int64, so they do not depend on the reduction order. 0 < nq <= 32.
 *   vrvq_rate_curve      total_bits[b][l] = sum_t cum[n(imp[b][t], levels[l])] for imp [B][T] and
 *                        levels [L] (device), one launch, no mask materialised
 *   vrvq_rate_solve      per group g of rows group_off[g] .. group_off[g+1] (int32, device, G + 1
 *                        entries; G = B rows of one is per-clip control, G = 1 over all rows one
 *                        level for a file): the largest fp32 level in [level_lo, level_hi] whose
 *                        total is <= budget[g] (int64, device), by bisection on the bit patterns
 *                        of the positive floats (<= 31 halvings, exact). 0 < level_lo <=
 *                        level_hi, both finite. Exact for imp >= 0 (the count is then monotone in
 *                        the level); other inputs end too, with an unspecified level.
 *                        status[g]: 0 solved; 1 infeasible (level_lo already exceeds the budget:
 *                        level_out = level_lo, total_out its total); 2 saturated (level_hi fits,
 *                        level_out = level_hi; also an empty group, total 0); -1 the group's range
 *                        is not 0 <= group_off[g] <= group_off[g+1] <= B (nothing is read,
 *                        level_out = level_lo, total_out = 0). total_out[g] is the total at
 *                        level_out[g]. One 256-thread workgroup per group; a group of up to 4096
 *                        elements is held in registers, a larger one is re-read per iteration.
 *   vrvq_scale_imp_rows  out[b][t] = imp[b][t] * levels[b] (one rounding). The RVQ entry points
 *                        given this map and level = 1.0f (an exact product) compute the
 *                        expression above for each row's own level, bit for bit.
 *
 * Capped rate control (library version 111): a cap on the rate of every packet next to the
 * group's budget. A packet is a run of P = packet_frames consecutive frames of one row; a row has
 * NP = ceil(T / P) packets, packet p covers frames [p P, min((p + 1) P, T)) (the last may be
 * short, P >= T is one packet per row). bits_bp(l) is the int64 total of packet (b, p) at level l.
 *   vrvq_rate_solve_capped  bits, group_off, budget, level_lo, level_hi as for vrvq_rate_solve;
 *                        packet_budget [NP] (int64, device): the bits packet p of any row may take.
 *                        cap[b][p] = the largest fp32 level in [level_lo, level_hi] with
 *                        bits_bp(cap) <= packet_budget[p], what vrvq_rate_solve gives for that
 *                        packet alone (level_lo if even level_lo exceeds it: the packet is
 *                        infeasible; level_hi if level_hi fits). lambda[g] = the largest fp32
 *                        level in [level_lo, level_hi] with
 *                        sum over (b, p) in g of bits_bp(min(lambda, cap[b][p])) <= budget[g]: the
 *                        sum does not decrease with lambda for imp >= 0, so the same bisection is
 *                        exact (<= 31 passes, bounded by the interval and not by the data).
 *                        level_out[g] = lambda[g], total_out[g] the sum at it, status[g] as for
 *                        vrvq_rate_solve (1: over budget with every packet at level_lo; 2: level_hi
 *                        fits, the caps included). packet_level [B][NP] = min(lambda[g], cap),
 *                        packet_total [B][NP] (int64) the packet's bits at it, packet_status
 *                        [B][NP]: 0 the packet runs at its group's level, 1 infeasible (it runs at
 *                        level_lo and exceeds packet_budget[p]), 2 limited by its cap (cap <
 *                        lambda). A row of no valid group keeps packet_level = cap, the total at
 *                        it and packet_status 1 or 2. Groups should not share rows (the shared
 *                        rows' packet outputs are those of one of the groups). Two launches, no
 *                        host sync, no atomics: one wave per packet for the caps (a packet of up to
 *                        256 frames in registers, a longer one re-read per pass), then one
 *                        256-thread workgroup per group (up to 4096 elements and their caps in
 *                        registers, a larger group re-read per pass) and one wave per packet of
 *                        the group for the packet outputs.
 *   vrvq_scale_imp_packets  out[b][t] = imp[b][t] * packet_level[b][t / P] (one rounding): with
 *                        level = 1.0f the RVQ entry points run every packet at its own level. */
int vrvq_rate_curve(const float* imp, int batch, int frames, int nq, const int* bits,
                    const float* levels, int n_levels, long long* total_bits,
                    vrvq_stream_t stream);
int vrvq_rate_solve(const float* imp, int batch, int frames, int nq, const int* bits,
                    const int* group_off, int n_groups, const long long* budget, float level_lo,
                    float level_hi, float* level_out, long long* total_out, int* status,
                    vrvq_stream_t stream);
int vrvq_scale_imp_rows(const float* imp, int batch, int frames, const float* levels, float* out,
                        vrvq_stream_t stream);
int vrvq_rate_solve_capped(const float* imp, int batch, int frames, int nq, const int* bits,
                           const int* group_off, int n_groups, const long long* budget,
                           const long long* packet_budget, int packet_frames, float level_lo,
                           float level_hi, float* level_out, long long* total_out, int* status,
                           float* packet_level, long long* packet_total, int* packet_status,
                           vrvq_stream_t stream);
int vrvq_scale_imp_packets(const float* imp, int batch, int frames, const float* packet_level,
                           int packet_frames, float* out, vrvq_stream_t stream);

/* Distortion metrics (models/utils.py:91-129 cal_metrics: torchmetrics' SI-SDR / SI-SNR / SNR
 * formulas for fp32 input, and the L1 distance), per row and without a host sync.
 *
 * est [rows][samples] and ref [ref_rows][samples], rows % ref_rows == 0: row r is compared with
 * reference row r % ref_rows, the level-major (L * B, T) layout of a level sweep. lengths
 * [ref_rows] (int64, device) or NULL: only the first n = clamp(lengths[r % ref_rows], 0, samples)
 * samples of a row count (NULL: n = samples); nothing at or past n is read.
 *
 * With p = est, t = ref, every product, difference and sum formed in fp64:
 *   moments[r][8] = { sum p, sum t, sum p t, sum p^2, sum t^2, sum |p - t|, sum (p - t)^2, n }
 *   eps = 2^-23 (float32 eps)
 *   si(pt, pp, tt): alpha = (pt + eps) / (tt + eps), S = alpha^2 tt,
 *                   N = max(S - 2 alpha pt + pp, 0), 10 log10((S + eps) / (N + eps))
 *   metrics[r][0] si_sdr = si(sum p t, sum p^2, sum t^2)                      (zero_mean = False)
 *   metrics[r][1] si_snr = si of the centred moments sum p t - sum p sum t / n,
 *                          max(sum p^2 - (sum p)^2 / n, 0), max(sum t^2 - (sum t)^2 / n, 0)
 *   metrics[r][2] snr    = 10 log10((sum t^2 + eps) / (sum (p - t)^2 + eps))
 *   metrics[r][3] l1     = sum |p - t| / n
 * n = 0 gives l1 = NaN and 0 dB for the other three; NaN in the data gives NaN out.
 *
 * Two launches: workgroups of a fixed VRVQ_METRICS_CHUNK samples (it does not depend on the
 * shape, the batch or the device) store seven partial sums each to workspace[row][chunk][7];
 * one wave per row adds them and evaluates the formulas. No atomics, a fixed summation order
 * per sample index that also does not depend on the rows' addresses: a row's result is the same
 * bits alone or in any batch. No sequential fp64 summation chain exceeds 4096 terms (64 per
 * thread, trees over lanes, 4 waves, <= 4096 chunks per lane), which bounds samples at
 * 2^32 (64 * 4096 chunks); rows <= 65535. Outside those: VRVQ_ERR_ARG.
 *   vrvq_signal_metrics_workspace  *bytes = rows * ceil(samples / VRVQ_METRICS_CHUNK) * 7 * 8
 *   vrvq_signal_metrics            metrics [rows][4] fp64; moments [rows][8] fp64 or NULL;
 *                                  workspace 8-byte aligned, workspace_bytes at least the above */
#define VRVQ_METRICS_CHUNK 16384
int vrvq_signal_metrics_workspace(int rows, long long samples, long long* bytes);
int vrvq_signal_metrics(const float* est, const float* ref, int rows, int ref_rows,
                        long long samples, const long long* lengths, double* metrics,
                        double* moments, void* workspace, long long workspace_bytes,
                        vrvq_stream_t stream);

/* BSS SDR (library version 112; models/utils.py:91-143 cal_metrics' "SDR",
 * torchmetrics.functional.signal_distortion_ratio without use_cg_iter), per row and without a
 * host sync: the estimate is projected onto the span of the filter_length delayed copies of the
 * reference, and the ratio is the energy inside that span over the energy outside it.
 *
 * est [rows][samples], ref [ref_rows][samples], rows % ref_rows == 0, lengths [ref_rows] (int64,
 * device) or NULL: rows pair up and lengths count as in vrvq_signal_metrics. For one row, p = est
 * and t = ref over its first n samples, F = filter_length, everything in fp64:
 *   zero_mean != 0: p and t each lose their own mean over the n samples;
 *   t <- t / max(|t|_2, 1e-6), p <- p / max(|p|_2, 1e-6);
 *   r[l] = sum_{i=0}^{n-1-l} t[i] t[i+l], b[l] = sum_{i=0}^{n-1-l} t[i] p[i+l], l < F (a lag
 *   l >= n is an empty sum, 0: what torchmetrics' FFT of length 2^ceil(log2(2n-1)) gives
 *   whenever that length is at least F);
 *   load_diag not NaN: r[0] += load_diag;
 *   R s = b with R[i][j] = r[|i-j|]; coh = b . s; out[row] = 10 log10(coh / (1 - coh)).
 * n = 0, sum t^2 = 0 or sum p^2 = 0 gives NaN; a NaN in a row's data gives NaN in that row (in
 * a reference's data: in the rows of that reference) and in no other. R is solved by
 * Levinson-Durbin, F - 1 steps whatever the data; if a step's prediction error is not positive
 * and finite (a singular R), the rows of that reference are NaN. coh >= 1 gives what IEEE
 * arithmetic gives (+inf or NaN): no clamp.
 *
 * Three launches on `stream`, four with zero_mean (the means first); no atomics, graph-capturable.
 * Workgroups of a fixed VRVQ_SDR_CHUNK samples store the chunk's F partial sums of b and its
 * sums of p^2 and t p to the workspace; r and sum t^2 are formed once per reference row, not once per
 * estimate. One workgroup per row adds the chunks in a fixed order and divides by the clamped
 * norms. One wave per (reference row, four estimates) runs the recursion; the estimates of a wave
 * share its prediction polynomial and each keeps its own solution. A row's bits do not depend on
 * the other rows, on how many estimates share its reference, or on the row's address.
 * VRVQ_ERR_ARG before any launch: null pointers, rows outside [1, 65535], ref_rows <= 0 or
 * rows % ref_rows != 0, samples outside [1, 2^32], filter_length outside [1, 512], a workspace
 * too small or not 8-byte aligned.
 *   vrvq_bss_sdr_workspace  *bytes = 8 * (rows + ref_rows) * (1 + ceil(samples / VRVQ_SDR_CHUNK)
 *                           * (filter_length + 2) + filter_length)
 *   vrvq_bss_sdr            out [rows] fp64; load_diag NaN for none */
#define VRVQ_SDR_CHUNK 2048
int vrvq_bss_sdr_workspace(int rows, int ref_rows, long long samples, int filter_length,
                           long long* bytes);
int vrvq_bss_sdr(const float* est, const float* ref, int rows, int ref_rows, long long samples,
                 const long long* lengths, int filter_length, int zero_mean, double load_diag,
                 double* out, void* workspace, long long workspace_bytes, vrvq_stream_t stream);

/* Spectral distance (models/loss.py:168-401 MultiScaleSTFTLoss / MelSpectrogramLoss, levels=None),
 * per row and per scale and without a host sync; no spectrogram reaches memory.
 *
 * est [rows][samples], ref [ref_rows][samples], rows % ref_rows == 0, lengths [ref_rows] (int64,
 * device) or NULL: rows pair up and lengths count as in vrvq_signal_metrics; a row of length n is
 * measured as if both signals ended after n samples. For one row (e against r, n samples) and one
 * scale s with window W = windows[s] (a power of two in [32, 2048]) and n_mels[s]:
 *   hop = W / 4, frames = 1 + n / hop; frame j holds samples j hop - W/2 .. j hop + W/2 - 1,
 *   indices outside [0, n) reflected without repeating the edge (-i -> i, n-1+i -> n-1-i):
 *   torch.stft(center=True, pad_mode="reflect"), which needs n > W / 2;
 *   window: periodic Hann 0.5 - 0.5 cos(2 pi k / W), no normalisation; magnitudes |rfft| of
 *   bins 0 .. W/2 in fp32;
 *   n_mels[s] > 0: E[m] = sum_j weights[off[m] + j] * |X[start[m] + j]|, j < len[m], in ascending
 *   j (fp32 fma chain), the banded form of a mel filter bank whose rows are contiguous runs;
 *   n_mels[s] == 0: the W/2 + 1 linear bins;
 *   terms[row][s][0] = mean |pow log10(max(E, clamp_eps)) - pow log10(max(R, clamp_eps))|
 *   terms[row][s][1] = mean |E - R|
 * both in fp64 over all (element, frame) pairs of the row. A row with n <= W / 2 gets NaN in both
 * terms of that scale; NaN in a row's data gives NaN in that row.
 *   distance[row] = sum_s (log_weight terms[row][s][0] + mag_weight terms[row][s][1]), the
 * scales added in their order in fp64 (NaN if any scale is); distance may be NULL.
 *
 * Caller-owned device tables, per scale:
 *   tables[s]        3 W floats, 8-byte aligned: exp(-2 pi i k / W) as (re, im) pairs, k < W, then
 *                    the W window values; built in fp64 and rounded once to fp32
 *   bands[s]         3 n_mels int32: start[m], len[m], off[m] (start[m] + len[m] <= W/2 + 1, off[m]
 *                    the band's first entry of band_weights[s]); unused for n_mels[s] == 0
 *   band_weights[s]  the bands' fp32 weights, packed
 * windows, n_mels, tables, bands, band_weights are host arrays of n_scales (<= 16) entries.
 *
 * n_scales + 1 launches on `stream`, no atomics. A workgroup owns a tile of
 * VRVQ_SPECTRAL_TILE_FRAMES(W) consecutive frames of one (row, scale) and stores two partial sums
 * to workspace; one wave per (row, scale) adds the tiles in a fixed order. The order in which an
 * element is added is a function of (scale, frame, element) alone: a row's bits do not depend on
 * the other rows, on their number, or on the row's address.
 * VRVQ_ERR_ARG before any launch: null pointers, a window that is no power of two in [32, 2048],
 * n_mels[s] < 0 or > W/2 + 1, n_scales outside [1, 16], rows outside [1, 65535], ref_rows <= 0 or
 * rows % ref_rows != 0, samples outside [1, 2^32], samples <= max(W) / 2 without lengths,
 * clamp_eps <= 0, a workspace too small or not 8-byte aligned.
 *   vrvq_spectral_distance_workspace  *bytes = 16 * rows * sum_s ceil((1 + samples / hop_s) /
 *                                     VRVQ_SPECTRAL_TILE_FRAMES(W_s))
 *   vrvq_spectral_distance            terms [rows][n_scales][2] fp64, distance [rows] fp64 or NULL */
#define VRVQ_SPECTRAL_TILE_SAMPLES 8192
#define VRVQ_SPECTRAL_TILE_FRAMES(window) (VRVQ_SPECTRAL_TILE_SAMPLES / (window))
int vrvq_spectral_distance_workspace(int rows, long long samples, int n_scales, const int* windows,
                                     long long* bytes);
int vrvq_spectral_distance(const float* est, const float* ref, int rows, int ref_rows,
                           long long samples, const long long* lengths, int n_scales,
                           const int* windows, const int* n_mels, const float* const* tables,
                           const int* const* bands, const float* const* band_weights,
                           double clamp_eps, double pow, double log_weight, double mag_weight,
                           double* terms, double* distance, void* workspace,
                           long long workspace_bytes, vrvq_stream_t stream);

/* Gradient of the spectral distance (library version 109): grad_est [rows][samples] fp32 =
 * grad_distance[row] * d distance[row] / d est[row], grad_distance [rows] fp64 on the device; the
 * reference gets no gradient. Arguments, tables and argument rules are vrvq_spectral_distance's.
 * With the definitions above, for one row and one scale, N = elements * frames:
 *   g[m,j] = (log_weight pow / (ln 10 E) sgn(pow log10 max(E, eps) - pow log10 max(R, eps)) [E >= eps]
 *             + mag_weight sgn(E - R)) / N, sgn(0) = 0, formed in fp64 with grad_distance[row]
 *   and rounded once (the clamp passes the gradient where E >= eps, as torch.clamp's backward);
 *   to the bins G[k] = sum_m weights[m,k] g[m,j] in ascending m (fp32 fma chain; G[k] = g[k,j]
 *   for n_mels == 0); through the magnitude G[k] X[k] / |X[k]|, 0 where |X[k]| = 0; through the
 *   adjoint of the one-sided real transform (bins 0 .. W/2 each once), times the window;
 *   overlap-add of the frames at hop W/4; the adjoint of the reflection (what landed at padded
 *   position -i is added to sample i, at n-1+i to n-1-i); the scales added in their order.
 * E, R and X are recomputed by the forward's own code (its bits); nothing of the forward is saved.
 * A bin whose fp32 magnitude is under 2^-6 of its frame's rms magnitude is ill-conditioned (an
 * ulp of the rms is 2^-18 of it or more, and X / |X| and 1 / E carry that on). How many bins
 * that is depends on the spectrum's flatness: a handful per tile for a flat spectrum, most bins
 * for a steep one. Where a batch of frames (2048 / W of them) has at most 32 such bins, each X[k]
 * is summed again from the samples in fp64 (one wave per bin, window and twiddle in fp64, a fixed
 * tree) and that X / |X|, and for n_mels == 0 that |X| in 1 / E, are used; the sign and clamp
 * decisions stay those of the fp32 E and R. A batch with more keeps the fp32 values for all of
 * them, so the pass costs at most 32 bins (eight rounds of the workgroup's four waves) per batch.
 * est == ref bitwise and an all-zero est give exactly 0; samples past a row's length get 0; a row
 * with n <= W/2 at some scale gets NaN in all `samples` entries; NaN in a row's data gives NaN at
 * the samples of the frames that hold it and leaves every other row untouched.
 *
 * n_scales + 1 launches on `stream`, no float atomics. A workgroup owns the forward's tile of
 * VRVQ_SPECTRAL_TILE_FRAMES(W) frames, overlap-adds them in ascending frame order (fp32 fma chain
 * from 0) into its span of SPAN(W) = W + (frames per tile - 1) W/4 samples and stores the span to
 * workspace; adjacent spans overlap by 3 W/4 samples. The last launch computes each sample as:
 * per scale, tile t's entry then tile t+1's for the sample itself, then the same for the left
 * fold, then for the right fold; then the scales in their order, all fp32 adds in that order.
 * The order is a function of (scale, frame, sample) alone: a row's bits do not depend on the other
 * rows, on their number, on the row's address or on whether lengths or `samples` gave its length.
 * VRVQ_ERR_ARG as for vrvq_spectral_distance, and for a null grad_distance or grad_est.
 *   vrvq_spectral_distance_grad_workspace  *bytes = 4 * rows * sum_s tiles_s * SPAN(W_s) rounded
 *                                          up to 8, tiles_s as in the forward's formula */
int vrvq_spectral_distance_grad_workspace(int rows, long long samples, int n_scales,
                                          const int* windows, long long* bytes);
int vrvq_spectral_distance_grad(const float* est, const float* ref, int rows, int ref_rows,
                                long long samples, const long long* lengths, int n_scales,
                                const int* windows, const int* n_mels, const float* const* tables,
                                const int* const* bands, const float* const* band_weights,
                                double clamp_eps, double pow, double log_weight, double mag_weight,
                                const double* grad_distance, float* grad_est, void* workspace,
                                long long workspace_bytes, vrvq_stream_t stream);

/* Sample-rate conversion (library version 106): julius.resample_frac as
 * audiotools.AudioSignal.resample calls it (zeros = 24, rolloff = 0.945), which the reference runs
 * in scripts/inference.py:187, models/dac_base.py:182 / :296 and models/discriminator.py:87. A
 * polyphase windowed-sinc FIR; neither julius nor audiotools is available to the project, so the
 * definition below is the specification (parity with julius itself unpinned).
 *
 * With g = gcd(old_sr, new_sr): old = old_sr / g, new = new_sr / g, sr = min(old, new) * rolloff,
 * W = ceil(zeros * old / sr), K = 2 W + old. For phase i < new and tap j < K, in fp64:
 *   u      = (-i / new + (j - W) / old) * sr,  t = clamp(u, -zeros, +zeros) * pi
 *   k_i[j] = sinc(t) * cos(t / zeros / 2)^2    (sinc(0) = 1),   k_i /= sum_j k_i[j]
 *   y[f new + i] = sum_j k_i[j] * x[clamp(f old + j - W, 0, L - 1)]       (replicate padding)
 * Output length: floor(new L / old) by default, in 64-bit integers (julius rounds it through a
 * float32 tensor; this does not), anything in [1, ceil(new L / old)] on request.
 * Taps with |u| >= zeros carry the window's cos(pi / 2)^2, below 1e-30 of the centre tap: they are
 * dropped. The table is [new][ntaps] fp32 (built in fp64, rounded once) with ntaps the largest
 * number of kept taps of a phase (at most floor(2 zeros old / sr) + 1), and first[new]: row i
 * holds taps j = first[i] .. first[i] + ntaps - 1, zero where dropped; first is non-decreasing and
 * first[i] + ntaps <= K.
 * Supported: old, new <= 1024 after reduction, 0 < zeros <= 1024, 0 < rolloff <= 1, L <= 2^40.
 * Anything else: VRVQ_ERR_ARG, and vrvq_resample_error() names the reason (the reduced ratio).
 *
 *   vrvq_resample_plan   host only, touches no device. out = {old, new, W, K, ntaps, default
 *                        output length of `length` samples, largest output length, new * ntaps
 *                        (floats of the tap table; first has `new` entries)}. length >= 0.
 *   vrvq_resample_taps   host only: fills HOST buffers taps [new][ntaps] (taps_len floats, at least
 *                        new * ntaps) and first [new] (first_len ints, at least new).
 *   vrvq_resample        y [rows][out_length] from x [rows][length], device memory. old, new, W,
 *                        ntaps as the plan gives them, taps / first the table on the device. One
 *                        workgroup owns VRVQ_RESAMPLE_TILE consecutive outputs of one row, stages
 *                        the input window they read in LDS (the clamp applied there) and every lane
 *                        accumulates its outputs as an fp32 fma chain over the row's ntaps taps in
 *                        ascending j. No atomics, no host sync; a row's bits do not depend on the
 *                        other rows or their number. rows <= 65535.
 *   vrvq_resample_adjoint  the transpose: dx [rows][length] from dy [rows][out_length], gather
 *                        form: dx[m] = sum over the outputs whose window covers m of k_i[j] dy[n],
 *                        frames then phases ascending; a second one-workgroup-per-row launch adds
 *                        the gradient of the replicated edges to dx[0] and dx[length - 1]. No
 *                        atomics. */
#define VRVQ_RESAMPLE_TILE 512
int vrvq_resample_plan(int old_sr, int new_sr, int zeros, double rolloff, long long length,
                       long long out[8]);
int vrvq_resample_taps(int old_sr, int new_sr, int zeros, double rolloff, float* taps,
                       long long taps_len, int* first, long long first_len);
const char* vrvq_resample_error(void);
int vrvq_resample(const float* x, int rows, long long length, int old_rate, int new_rate, int width,
                  int ntaps, const float* taps, const int* first, float* y, long long out_length,
                  vrvq_stream_t stream);
int vrvq_resample_adjoint(const float* dy, int rows, long long out_length, int old_rate,
                          int new_rate, int width, int ntaps, const float* taps, const int* first,
                          float* dx, long long length, vrvq_stream_t stream);

/* Integrated loudness (library version 108): ITU-R BS.1770-4 as audiotools' AudioSignal.loudness /
 * Meter.integrated_loudness computes it (models/dac_base.py:183 / :186 / :295 measure and
 * normalize with it, conf/vrvq/vrvq_a2_lufs.yml VolumeNorm applies it to every batch), in the
 * arithmetic of vrvq_amd.codec.loudness.
 *
 * x [items][channels][length] fp32 -> one fp64 LUFS per item, floored at -70. With sr = sample_rate:
 *   K-weighting   two RBJ biquads in cascade, coefficients in fp64: high shelf +4 dB at 1500 Hz,
 *                 Q = 1 / sqrt 2, then high pass at 38 Hz, Q = 0.5, each run in fp64 in the
 *                 transposed direct form II (y = b0 x + s0; s0 = b1 x - a1 y + s1; s1 = b2 x - a2 y).
 *   blocks        win = int(0.4 sr) samples every step = int(0.4 sr * 0.25); block j of a channel is
 *                 the mean of y^2 over [j step, j step + win); blocks = (eff - win) / step + 1.
 *   short input   length / sr < 0.5: eff = length + int((0.5 - length / sr) * sr), the samples past
 *                 `length` read as zeros (the filter runs on through them); otherwise eff = length.
 *   gating        l_j = -0.691 + 10 log10(sum_c G_c z_cj), G = 1, 1, 1, 1.41, 1.41; absolute gate
 *                 l_j > -70; relative gate 10 LU under the loudness of the absolute-gated channel
 *                 means; the result is the loudness of the means over the blocks past both gates,
 *                 -70 where no block passes or the value is below -70.
 * The recurrence is exact, not windowed: every lane owns VRVQ_LOUDNESS_CHUNK consecutive samples of
 * one (item, channel) row. Pass 1 runs the cascade over each chunk from zero state and stores the
 * four final state values; a carry launch (one wave per row, fixed order) turns them into each
 * chunk's entry state with the chunk transition s' = M1 s, t' = M2 t + K s (the 4 x 4 power of the
 * zero-input cascade, built on the host in long double and rounded once); pass 2 reruns every
 * chunk from its entry state and adds y^2 in fp64 into partial sums cut at the chunk edges and at
 * the block edges; a finish launch (one workgroup per item) adds them into blocks and evaluates the
 * gates. The filtered signal is never stored. No atomics, no host sync; every sum has a fixed
 * order that depends on (sample_rate, channels, length) alone, so an item's bits do not depend on
 * the other items or their number.
 * Supported: sample_rate >= 10 (step >= 1), 1 <= channels <= 5, 1 <= length <= 2^40,
 * items * channels <= 65535. Anything else: VRVQ_ERR_ARG, and vrvq_loudness_error() names it.
 *
 *   vrvq_loudness_plan   host only, touches no device. out[VRVQ_LOUDNESS_PLAN_LEN] doubles (the
 *                        integers exactly): {eff, win, step, blocks, chunk, chunks per row,
 *                        workspace bytes per item, partial sums per row,
 *                        shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2 (a0 = 1),
 *                        M1[2][2], M2[2][2], K[2][2] row-major}.
 *   vrvq_loudness        out_lufs [items] fp64 from x, both in device memory. workspace: items times
 *                        the plan's bytes, 8-byte aligned, device memory; its contents on entry do
 *                        not matter. */
#define VRVQ_LOUDNESS_CHUNK 256
#define VRVQ_LOUDNESS_PLAN_LEN 30
int vrvq_loudness_plan(int sample_rate, int channels, long long length, double* out);
const char* vrvq_loudness_error(void);
int vrvq_loudness(const float* x, int items, int channels, long long length, int sample_rate,
                  void* workspace, double* out_lufs, vrvq_stream_t stream);

/* Variable-length code packing from importance masks (the reference's
 * DACFile, models/dac_base.py:19-58, stores the full uint16 code matrix). Packed stream is
 * clip-major, frame-major, stage-minor uint16: packed[clip_off[b] + frame_off[b,t] + i] =
 * codes[b,i,t] for i < counts[b,t]; clip_off has B+1 entries (clip_off[B] = total codes).
 *   vrvq_pack_counts     mask [B][nq][T] -> counts [B*T] (int32), clip_total [B], clip_off [B+1];
 *                        *err = 1 if a mask column is not prefix-shaped (nq <= 255)
 *   vrvq_pack_codes      codes [B][nq][T] int64 -> packed (clip_off[B] uint16); *err = 2 on a
 *                        code outside [0, ncode)
 *   vrvq_unpack_offsets  counts -> clip_total, clip_off (same scan as packing)
 *   vrvq_unpack_codes    packed -> codes [B][nq][T] int64 (0 where masked) and mask or NULL */
int vrvq_pack_counts(const float* mask, int batch, int nq, int frames, int* counts,
                     long long* clip_total, long long* clip_off, int* err, vrvq_stream_t stream);
int vrvq_pack_codes(const int64_t* codes, const int* counts, const long long* clip_off, int batch,
                    int nq, int frames, int ncode, uint16_t* packed, int* err,
                    vrvq_stream_t stream);
int vrvq_unpack_offsets(const int* counts, int batch, int frames, long long* clip_total,
                        long long* clip_off, vrvq_stream_t stream);
int vrvq_unpack_codes(const uint16_t* packed, const int* counts, const long long* clip_off,
                      int batch, int nq, int frames, int64_t* codes, float* mask,
                      vrvq_stream_t stream);

/* Bitstream ("VRVQ bitstream 1"): the bit-granular, parallel-decodable form of the stream above.
 * A stream is an array of little-endian uint32 words; a field of width n at bit position p puts
 * bit j of its value at stream bit p + j, and stream bit q is bit q & 31 of word q >> 5 (a field
 * may straddle two words). Fields: a code takes w = max(1, ceil(log2(ncode))) bits (ncode in
 * [2, 65536]), a count cb = ceil(log2(nq + 1)) bits; count_bits = 0 is the fixed-count stream
 * (every frame keeps all nq stages, mask = NULL, no plane A). Row r (a clip) is two planes:
 *   A  frames count fields c_t = sum_i mask[r][i][t], t ascending, zero-padded to a whole word
 *   B  for t ascending, i < c_t: codes[r][i][t]; the field of (t, i) starts at bit
 *      w * (sum_{t' < t} c_t' + i) of the plane; zero-padded to a whole word
 * so row_words[r] = ceil(frames * cb / 32) + ceil(w * sum_t c_t / 32); rows are concatenated,
 * row_off[r] = sum_{r' < r} row_words[r'] (rows + 1 entries). A row's words do not depend on the
 * other rows. Both directions run on a grid of (chunk of VRVQ_BITSTREAM_CHUNK_FRAMES frames, row);
 * chunk_total / chunk_off hold rows * ceil(frames / VRVQ_BITSTREAM_CHUNK_FRAMES) entries (codes
 * of a chunk; codes of the row before the chunk). *err must be zero on entry and receives the
 * largest code raised. Limits: nq <= 255, frames <= 2^24, rows * chunks < 2^31.
 *   vrvq_bitpack_plan    codes, mask -> counts [rows*frames], chunk_total, chunk_off, row_codes
 *                        [rows] (sum_t c_t), row_words [rows], row_off [rows + 1]; *err = 1: a
 *                        mask column is not prefix-shaped; 2: a kept code outside [0, ncode)
 *   vrvq_bitpack_write   zeroes words[0 .. total_words) and writes both planes of every row
 *                        (total_words = row_off[rows], read by the caller); the words are a pure
 *                        function of codes and mask
 *   vrvq_bitunpack_plan  reads plane A within the header's row_words (row_off [rows + 1] = their
 *                        exclusive scan, made by the caller from the header: a corrupt row
 *                        cannot move the others; row_off[rows] <= total_words) -> counts,
 *                        chunk_total, chunk_off, row_err [rows] (zero on entry, like *err);
 *                        *err = 3: a count above nq; 4: a row whose counts give another word
 *                        count than row_off[r + 1] - row_off[r], or leave the row
 *   vrvq_bitunpack_read  -> codes [rows][nq][frames] int64 (0 where masked) and mask (or NULL);
 *                        *err = 2: a decoded value >= ncode. A row flagged by the plan decodes
 *                        to zeros; no word outside [0, total_words) or the row is ever read. */
#define VRVQ_BITSTREAM_CHUNK_FRAMES 256
int vrvq_bitstream_chunk_frames(void);
int vrvq_bitpack_plan(const int64_t* codes, const float* mask, int rows, int nq, int frames,
                      int ncode, int* counts, int* chunk_total, long long* chunk_off,
                      long long* row_codes, long long* row_words, long long* row_off, int* err,
                      vrvq_stream_t stream);
int vrvq_bitpack_write(const int64_t* codes, const int* counts, const long long* chunk_off,
                       const long long* row_off, int rows, int nq, int frames, int ncode,
                       int count_bits, uint32_t* words, long long total_words,
                       vrvq_stream_t stream);
int vrvq_bitunpack_plan(const uint32_t* words, long long total_words, const long long* row_off,
                        int rows, int nq, int frames, int ncode, int count_bits, int* counts,
                        int* chunk_total, long long* chunk_off, int* row_err, int* err,
                        vrvq_stream_t stream);
int vrvq_bitunpack_read(const uint32_t* words, long long total_words, const int* counts,
                        const long long* chunk_off, const long long* row_off, const int* row_err,
                        int rows, int nq, int frames, int ncode, int count_bits, int64_t* codes,
                        float* mask, int* err, vrvq_stream_t stream);

/* ResidualVectorQuantize.from_latents (models/quantize.py:251-285): per stage i < nq the
 * nearest normalised codeword of the stage's own latent latents[b][8i..8i+8][t] (decode_latents,
 * :87-103; the distance expression of vrvq_rvq_chain) -> codes [B][nq][T] int64. latents has
 * nlat >= 8 nq channels; cbn [nq][ncode][8] / c2 [nq][ncode] from vrvq_codebook_prep. The
 * z_p rows and z_q follow with vrvq_rvq_gather + vrvq_rvq_expand. */
int vrvq_rvq_nearest(const float* latents, int batch, int nlat, int frames, int nq,
                     const float* cbn, const float* c2, int ncode, int cdim, int64_t* codes,
                     vrvq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training step (scripts/train.py:262-330): the backward operators of
 * the generator, used by the torch.autograd.Functions in vrvq_amd/train.py. Every reduction
 * runs in a fixed order (bitwise reproducible run to run).
 * ------------------------------------------------------------------------------------- */

/* Split-K plan for vrvq_conv1d_wgrad: *n_split partial sums and the workspace they need. */
int vrvq_wgrad_plan(int batch, int m, int ta, int c, int k, int* n_split,
                    long long* workspace_bytes);

/* Weight gradient of a (Snake-fused) convolution as a split-K MFMA GEMM:
 *   out[m][c][k] = sum_b sum_{t < ta} As[b][m][t] * Xs[b][c][t*stride - pad + k*dil]
 * As = snake(a) if alpha_a, Xs = snake(x) if alpha (x = 0 outside [0, tx)).
 *   WNConv1d (models/layers.py:17-18):      a = dY [B][Cout][Tout], x = layer input -> dW[Cout][Cin][k]
 *   WNConvTranspose1d (models/layers.py:21-22): a = layer input (snake on a), x = dY
 *                                           -> dW[Cin][Cout][k]
 * The autograd conv weight backward of the reference (torch.nn.grad.conv1d_weight). */
int vrvq_conv1d_wgrad(const float* a, int batch, int m, int ta, const float* alpha_a,
                      const float* inv_alpha_a, const float* x, int c, int tx, const float* alpha,
                      const float* inv_alpha, int k, int stride, int pad, int dil, int n_split,
                      float* workspace, long long workspace_bytes, float* out,
                      vrvq_stream_t stream);

/* Snake1d backward (models/layers.py:26-32): dx = g (1 + inv sin(2 a x) a) (dx may be NULL),
 * dalpha[c] = sum_{b,t} g (-inv^2 sin^2(a x) + inv sin(2 a x) x) (dalpha may be NULL). */
int vrvq_snake_backward_workspace(int batch, int channels, int frames, long long* bytes);
int vrvq_snake_backward(const float* x, const float* alpha, const float* inv_alpha,
                        const float* grad, int batch, int channels, int frames, float* dx,
                        float* dalpha, float* workspace, long long workspace_bytes,
                        vrvq_stream_t stream);

/* Conv bias gradient: db[c] = sum_{b,t} grad[b][c][t] (per-(clip, chunk) partials in the
 * workspace, summed in a fixed order). */
int vrvq_bias_grad_workspace(int batch, int channels, int frames, long long* bytes);
int vrvq_bias_grad(const float* grad, int batch, int channels, int frames, float* db,
                   float* workspace, long long workspace_bytes, vrvq_stream_t stream);

/* Tanh (models/dac_vrvq.py:74) / Sigmoid (models/importance_subnet.py:44) backward from the
 * saved output y: out = g (1 - y^2) | g y (1 - y). */
int vrvq_act_backward(const float* y, const float* grad, long long n, int epilogue, float* out,
                      vrvq_stream_t stream);

/* weight_norm backward (models/layers.py:17-22): per row, n = ||v||,
 * dg = (dw . v) / n, dv = (g / n) (dw - v (dw . v) / n^2). */
int vrvq_weight_norm_backward(const float* g, const float* v, const float* dw, int rows,
                              int cols, float* dg, float* dv, vrvq_stream_t stream);

/* Adjoint packing for the input gradient of a stride-1 Conv1d: w [cout][cin][k] ->
 * the vrvq_conv1d packed layout of W'[ci][co][k] = w[co][ci][k-1-k'] ([cout][k][cin_pad]). */
int vrvq_pack_conv1d_flip(const float* w, int cout, int cin, int k, int cin_pad,
                          float* w_packed, vrvq_stream_t stream);

/* Training-mode importance mask (models/quantize.py:377-414, models/utils.py:11-61): rows
 * b < n_imps: generate_mask_ste((imp * levels[b]) * nq, alpha) (value smooth + (hard - smooth)),
 * or, with levels == NULL, generate_mask_ste(imp, alpha) of an already scaled map;
 * the next n_drop rows n_imps + j: generate_mask_hard(dropout[j]) (the first n_drop draws, as
 * models/quantize.py:412-413 assigns dropout[:n_dropout]); the rest 1. imp [B][T], levels [B],
 * dropout [B] int64 (may be NULL when n_drop = 0), mask [B][nq][T]. */
int vrvq_mask_ste(const float* imp, const float* levels, const int64_t* dropout, int batch,
                  int frames, int nq, float alpha, int n_imps, int n_drop, float* mask,
                  vrvq_stream_t stream);
/* Its backward: dimp[b][t] = (sum_i dmask[b][i][t] logcosh'(x - i)) * nq * levels[b] for
 * b < n_imps (without the * nq * levels[b] when levels == NULL), 0 for the overwritten rows. */
int vrvq_mask_ste_backward(const float* imp, const float* levels, const float* dmask, int batch,
                           int frames, int nq, float alpha, int n_imps, float* dimp,
                           vrvq_stream_t stream);

/* vrvq_rvq_expand with explicit mask values [B][nq][T] (the training mask) instead of imp. */
int vrvq_rvq_expand_masked(const float* zst, int batch, int dim, int frames, int nq, int cdim,
                           const float* w_out, const float* b_out, const float* mask,
                           float* z_q_is, float* z_q, vrvq_stream_t stream);

/* Backward of the training-mode quantizer (models/quantize.py:42-79, 328-443): from
 * dz_q [B][D][T] and the device scalars g_commit / g_codebook (dL/d commitment_loss,
 * dL/d codebook_loss) and the forward state (z, zst [B][nq][T][d], latents [B][nq*d][T], codes,
 * mask values [B][nq][T]) computes dz [B][D][T], dmask [B][nq][T], dw_in [nq][d][D]
 * (the folded in_proj weight layout), db_in [nq][d], dw_out [nq][D][d], db_out [nq][D] and
 * dcb [nq][N][d]. D = 1024, d = 8, nq <= 32. The math (rvq_train.hip header) stays in the
 * 8-dim latent space: reverse chain with M_ji = W_in(j) W_out(i) (mcol of
 * vrvq_rvq_cross_prep), three split-K GEMMs and 8x8 fix-ups for the weight gradients. */
int vrvq_rvq_backward_workspace(int batch, int frames, int nq, long long* bytes);
int vrvq_rvq_backward(const float* dz_q, const float* g_commit, const float* g_codebook,
                      const float* z, const float* zst, const float* latents,
                      const int64_t* codes, const float* mask, int batch, int dim, int frames,
                      int nq, int ncode, int cdim, const float* w_in_t, const float* w_out,
                      const float* b_out, const float* mcol, const float* cb, float* dz,
                      float* dmask, float* dw_in, float* db_in, float* dw_out, float* db_out,
                      float* dcb, void* workspace, long long workspace_bytes,
                      vrvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VRVQ_H_ */
