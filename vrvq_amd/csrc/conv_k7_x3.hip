// The k = 7 convs on the x3 loop.
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // plain chunks
    conv_kernel<32, 128, 1, 4, 7, true>(),
    conv_kernel<128, 32, 4, 4, 7, true>(),
    conv_kernel<128, 96, 4, 4, 7, true>(),
    conv_kernel<64, 64, 2, 4, 7, true>(),
    conv_kernel<64, 128, 2, 4, 7, true>(),
    conv_kernel<96, 128, 1, 4, 7, true>(),
    conv_kernel<128, 64, 2, 4, 7, true>(),
    conv_kernel<128, 128, 2, 4, 7, true>(),
    conv_kernel<192, 64, 2, 4, 7, true>(),
    conv_kernel<192, 128, 2, 4, 7, true>(),
    // 64 x 256 on pair chunks (choose_tile takes it for Cin a multiple of 16 only: no plain-chunk form)
    conv_kernel<64, 256, 1, 4, 7, true, false, true>(),
    // split-K (conv_plan.h splitk_parts)
    conv_kernel<128, 96, 4, 4, 7, true, false, false, true>(),
};

}  // namespace

bool conv_k7_x3_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k7_x3_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
