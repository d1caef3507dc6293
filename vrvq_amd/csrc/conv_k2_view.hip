// The strided k = 2 stride convs on the x3 loop: 2-tap GEMMs over the phase-split view (PH).
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // pair tiles on pair chunks
    conv_kernel<32, 128, 1, 4, 2, true, true, true>(),
    conv_kernel<128, 32, 4, 4, 2, true, true, true>(),
    conv_kernel<64, 128, 2, 4, 2, true, true, true>(),
    conv_kernel<96, 128, 1, 4, 2, true, true, true>(),
    conv_kernel<128, 128, 2, 4, 2, true, true, true>(),
    // ... on plain chunks (Cin * stride no multiple of 32)
    conv_kernel<32, 128, 1, 4, 2, true, true, false>(),
    conv_kernel<128, 32, 4, 4, 2, true, true, false>(),
    conv_kernel<64, 128, 2, 4, 2, true, true, false>(),
    conv_kernel<96, 128, 1, 4, 2, true, true, false>(),
    conv_kernel<128, 128, 2, 4, 2, true, true, false>(),
    // split-K (conv_plan.h splitk_parts)
    conv_kernel<128, 96, 4, 4, 2, true, true, true, true>(),
};

}  // namespace

bool conv_k2_view_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k2_view_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
