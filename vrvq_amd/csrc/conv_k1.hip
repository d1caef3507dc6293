// The k = 1 GEMMs (the ResidualUnit k1 + skip convs, the ImportanceSubnet heads) on the fp32-input loop.
#include "conv_kernels.h"

namespace vrvq_conv {
namespace {

// <BM, BN, WM, NW, KS, X3[, PH, PAIR, SPLIT]>: conv_mfma_kernel's arguments
const ConvKernel kTable[] = {
    // fp32-input loop
    conv_kernel<32, 128, 1, 4, 1, false>(),
    conv_kernel<128, 32, 4, 4, 1, false>(),
    conv_kernel<128, 96, 4, 4, 1, false>(),
    conv_kernel<64, 64, 2, 4, 1, false>(),
    conv_kernel<64, 128, 2, 4, 1, false>(),
    conv_kernel<96, 128, 1, 4, 1, false>(),
    conv_kernel<128, 64, 2, 4, 1, false>(),
    conv_kernel<128, 128, 2, 4, 1, false>(),
    conv_kernel<192, 64, 2, 4, 1, false>(),
    conv_kernel<192, 128, 2, 4, 1, false>(),
};

}  // namespace

bool conv_k1_has(const ConvPlan& p) { return find_kernel(kTable, p) != nullptr; }

int conv_k1_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  return launch_plan(kTable, p, a, st);
}

}  // namespace vrvq_conv
