// The 2-tap GEMMs on the x3 loop: stride-1 k = 2 convs and the polyphase ConvTranspose.
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // pair tiles (conv_geom.h x3_pair), on pair chunks
    conv_kernel<32, 128, 1, 4, 2, true, false, true>(),
    conv_kernel<128, 32, 4, 4, 2, true, false, true>(),
    conv_kernel<64, 128, 2, 4, 2, true, false, true>(),
    conv_kernel<96, 128, 1, 4, 2, true, false, true>(),
    conv_kernel<128, 128, 2, 4, 2, true, false, true>(),
    // ... on plain chunks (Cin no multiple of 32)
    conv_kernel<32, 128, 1, 4, 2, true, false, false>(),
    conv_kernel<128, 32, 4, 4, 2, true, false, false>(),
    conv_kernel<64, 128, 2, 4, 2, true, false, false>(),
    conv_kernel<96, 128, 1, 4, 2, true, false, false>(),
    conv_kernel<128, 128, 2, 4, 2, true, false, false>(),
    // the other tiles: plain chunks
    conv_kernel<128, 96, 4, 4, 2, true>(),
    conv_kernel<64, 64, 2, 4, 2, true>(),
    conv_kernel<128, 64, 2, 4, 2, true>(),
    conv_kernel<192, 64, 2, 4, 2, true>(),
    conv_kernel<192, 128, 2, 4, 2, true>(),
};

}  // namespace

bool conv_k2_x3_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k2_x3_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
