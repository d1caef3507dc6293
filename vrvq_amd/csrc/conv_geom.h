// Geometry of the conv tiles as plain constexpr functions of int arguments: one formula per
// quantity, read at compile time by the kernels (through the template structs of conv_core.h /
// conv_x3.h, which wrap them) and at run time by the planner (conv_plan.h). No HIP include and no
// device code: this header also compiles with the host C++ compiler alone.
#pragma once

namespace vrvq_conv {

// ---- fp32-input loop (conv_core.h conv_mainloop) ----
// Input channels per K-chunk: CK*KS ~ 32..64 rows of W per stage (half for 192-row tiles,
// so two double-buffered stages still fit twice per CU).
// The strided encoder convs (KS = 2 s in {4, 8, 16}) take half of that: with their wide
// input windows a full chunk needs ~99 KB for the two stages, one workgroup per CU, and
// their short K then leaves every prologue / epilogue exposed (measured at B = 32:
// 64->128 s2 877 -> 680 us, 128->256 s4 1279 -> 1072, 512->1024 s8 at BN 32 888 -> 696;
// but 256->512 s8 at BN 128 1319 -> 1606, so k16 keeps 4 channels on 128-wide tiles).
constexpr int chunk_ck(int ks, int bm, int bn) {
  const int ck0 = ks == 1 ? 32 : ks <= 3 ? 16 : ks == 4 ? 8 : ks == 7 ? 8
                  : ks == 8 ? 4 : bn > 32 ? 4 : 2;
  return (bm > 128 && ck0 >= 8) ? ck0 / 2 : ck0;
}

// Largest input window a thread stages per K-chunk: stride <= KS/2 for the strided (k = 2s)
// encoder convs, dilation <= 9 for the k = 7 residual-unit convs.
constexpr int win_smax(int ks) { return (ks == 4 || ks == 8 || ks == 16) ? ks / 2 : 1; }
constexpr int win_dmax(int ks) { return ks == 7 ? 9 : 1; }
constexpr int win_xw_max(int ks, int bn) {
  return (bn - 1) * win_smax(ks) + (ks - 1) * win_dmax(ks) + 1;
}
constexpr int win_per_row(int ks, int bn) { return (win_xw_max(ks, bn) + 63) / 64; }

// LDS bytes of the loop's two stages [W chunk | x window of xwp floats per channel].
constexpr long long conv_lds_bytes(int ks, int bm, int bn, int xwp) {
  const long long ck = chunk_ck(ks, bm, bn);
  return 2 * (ck * ks * bm + ck * xwp) * 4;
}

// ---- epilogue (conv_core.h conv_epilogue) ----
// Column passes: the accumulator tile goes through LDS in BM x (BN / EPASS) pieces of at most
// 64 KiB, EPASS dividing the wave-column count.
constexpr int epi_passes(int bm, int bn) {
  const int need = (bm * bn * 4 + 65535) / 65536;
  return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
}
constexpr int epi_bnp(int bm, int bn) { return bn / epi_passes(bm, bn); }

// in_proj epilogue (conv_core.h proj_epilogue): z crosses LDS as three planes
// [plane][frame][channel] (rows of 128 + 8 channels: conflict-free 16-B B reads), 32 frames
// per pass.
constexpr int PJE_LDB = 136;                      // bf16 per frame row
constexpr int PJE_FR = 32;                        // frames per pass
constexpr int PJE_PLANE = PJE_FR * PJE_LDB * 2;   // bytes per plane (8,704)
constexpr int PJE_LDS = 3 * PJE_PLANE;            // 26,112 B

// ---- x3 loop (conv_x3.h conv_mainloop_x3) ----
// LDS stages of the x3 K loop. 1 (default): one stage, refilled between two barriers after
// the chunk's MFMAs; half the LDS and no prefetch registers let two workgroups share a CU,
// and each one's MFMAs cover the other's loads, barriers and epilogue. 2: double-buffered
// with the next chunk prefetched into registers during the MFMAs, one workgroup per CU for
// the larger tiles.
// Tiles up to 128 x 128 take 1 (two workgroups per CU), the 192-row x 128 tiles 2 (their
// registers allow one wave per SIMD, so the prefetch has to hide the loads).
constexpr int x3_stages(int bm, int bn) { return bm * bn <= 128 * 128 ? 1 : 2; }

// 64 x 256 k7 tiles ("pair" chunks): a K-chunk of 16 channels, two channel octets per tap, so
// the 7 taps fill 14 octet slots = 7 MFMA steps with no zero octet (an 8-channel k7 chunk pads
// its 7 octets to 8: 1/8 of its MFMAs multiply zero weights), 168 MFMAs per wave between two
// barriers instead of 96. The weight planes stay in the 8-channel packing (two packed chunks
// per K-chunk, pad octets skipped while staging): 43 KB W + <= 30 KB x per stage, two
// workgroups per CU.
// A pair tile needs Cin to be a multiple of the K-chunk (conv_plan.h plan_mfma runs the tile on
// plain chunks otherwise). The k1 + skip GEMMs on the same construction (128 x 64 tiles, two
// 32-channel packed chunks per K-chunk) measured slower: profiles/r03_x3_pair_ab.txt.
// The same pairing for the 2-tap GEMMs (the strided encoder convs through the phase-split view
// and the polyphase ConvTranspose): 32-channel K-chunks of 8 octets = 4 MFMA steps (the
// 16-channel chunk has 2), on the 128- and 32-wide tiles up to 128 rows (one LDS stage, two
// workgroups per CU). Measured per layer at B = 32 (profiles/r04d_layer_table.txt vs
// r03f_layer_table.txt): 128 x 128 tiles 5-13 % faster (64->128 s2, 128->256 s4, ConvT 384->192
// s4), 128 x 32 10 % (512->1024 s8 at T = 87); 128 x 64 and 128 x 96 4-14 % slower (the doubled
// weight stage costs the 128 x 64 tile its third workgroup per CU): those keep 16-channel chunks.
constexpr bool x3_pair(int ks, int bm, int bn) {
  return (ks == 7 && bm == 64 && bn == 256) || (ks == 2 && bm <= 128 && (bn == 128 || bn == 32));
}

// K-chunk of the x3 loop. pair = false: also the HBM packing of the weight planes
// (vrvq_pack_x3_weight).
constexpr int x3_ck(int ks, bool pair) {  // channels per K-chunk
  return (pair ? 2 : 1) * (ks == 1 ? 32 : ks <= 3 ? 16 : 8);
}
constexpr int x3_nc8(int ks, bool pair) { return x3_ck(ks, pair) / 8; }            // channel octets per tap
constexpr int x3_no(int ks, bool pair) { return ks * x3_nc8(ks, pair); }           // octets per chunk
constexpr int x3_no2(int ks, bool pair) { return (x3_no(ks, pair) + 1) & ~1; }     // padded to MFMA steps
constexpr int x3_nstep(int ks, bool pair) { return x3_no2(ks, pair) / 2; }

// Largest window of the x3 loop (stride 1; dilation <= 9 for k = 7).
constexpr int x3_xw_max(int ks, int bn) { return (bn - 1) + (ks - 1) * (ks == 7 ? 9 : 1) + 1; }
constexpr int x3_xwp(int xw) { return (xw + 3) & ~3; }

// LDS bytes of the W planes of one pipeline stage.
constexpr int x3_stage_w_bytes(int ks, int bm, bool pair) {
  return pair ? 2 * 3 * x3_no(ks, false) * bm * 16 : 3 * x3_no2(ks, false) * bm * 16;
}

// LDS bytes the x3 mainloop needs for a window of xw positions; snake_cin: the channels of the
// Snake table a pair tile keeps in LDS (0: the staging applies no Snake).
constexpr long long x3_lds_bytes(int ks, int bm, int bn, bool pair, int xw, int snake_cin) {
  const long long xb = 3LL * x3_nc8(ks, pair) * x3_xwp(xw) * 16;
  const long long snake = pair ? 2LL * snake_cin * 4 : 0;
  return x3_stages(bm, bn) * (x3_stage_w_bytes(ks, bm, pair) + xb) + snake;
}

// The K loop's 32-bit byte offsets hold: at most 32 rows of x (one K-chunk's channels) and one
// chunk's weight planes (at most 2 * 3 * 8 octet slots of m_pad rows, 16 bytes per row). The
// entry points refuse anything longer (VRVQ_ERR_UNSUPPORTED).
constexpr bool x3_offsets_fit(long long tin, long long m_pad) {
  return 32 * tin * 4 <= 0x7fffffffLL && 49 * m_pad * 16 <= 0x7fffffffLL;
}

// ---- kernels off the MFMA tiles (conv.hip) ----
constexpr int SMALL_BT = 256;     // conv_small_cout_kernel: outputs per workgroup
constexpr int SMALL_SC = 16;      // ... channels staged per step
constexpr int SMALL_COUT = 8;
constexpr int SMALL_WMAX = 2048;  // cin * k * cout weights staged in LDS
constexpr int C1_T = 4;           // conv_cout1_stream_kernel: outputs per thread
constexpr int C1_W = 12;          // ... window samples per channel
constexpr int CI1_T = 4;          // conv_cin1_stream_kernel: outputs per thread
constexpr int CI1_CG = 16;        // ... channels per thread

}  // namespace vrvq_conv
