// The k = 1 GEMMs on the x3 loop.
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // plain chunks (M a multiple of 192 runs 192 x 64: no x3 192 x 128 tile)
    conv_kernel<32, 128, 1, 4, 1, true>(),
    conv_kernel<128, 32, 4, 4, 1, true>(),
    conv_kernel<128, 96, 4, 4, 1, true>(),
    conv_kernel<64, 64, 2, 4, 1, true>(),
    conv_kernel<64, 128, 2, 4, 1, true>(),
    conv_kernel<96, 128, 1, 4, 1, true>(),
    conv_kernel<128, 64, 2, 4, 1, true>(),
    conv_kernel<128, 128, 2, 4, 1, true>(),
    conv_kernel<192, 64, 2, 4, 1, true>(),
};

}  // namespace

bool conv_k1_x3_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k1_x3_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
