// k = 8: the stride-4 encoder conv and stride-1 convs of eight taps, fp32-input loop only.
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // fp32-input loop
    conv_kernel<32, 128, 1, 4, 8, false>(),
    conv_kernel<128, 32, 4, 4, 8, false>(),
    conv_kernel<128, 96, 4, 4, 8, false>(),
    conv_kernel<64, 64, 2, 4, 8, false>(),
    conv_kernel<64, 128, 2, 4, 8, false>(),
    conv_kernel<96, 128, 1, 4, 8, false>(),
    conv_kernel<128, 64, 2, 4, 8, false>(),
    conv_kernel<128, 128, 2, 4, 8, false>(),
    conv_kernel<192, 128, 2, 4, 8, false>(),
};

}  // namespace

bool conv_k8_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k8_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
