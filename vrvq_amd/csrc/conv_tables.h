// The launch side of a ConvPlan (conv_plan.h): the conv_mfma_kernel instantiations live in the
// per-tap translation units conv_k*.hip, each behind a table of the kernels it holds. A table
// entry is made from the kernel's own template arguments (conv_kernels.h conv_kernel<>), which
// yield both its key and its pointer, so a key cannot name another kernel.
#pragma once
#include "conv_core.h"
#include "conv_plan.h"

namespace vrvq_conv {

struct ConvKernel {
  unsigned key;                // plan_key of the template arguments
  int threads;
  void (*main)(ConvArgs);
  void (*epilogue)(ConvArgs);  // the split-K epilogue launch (null: unsplit)
};

// One conv kernel: its dynamic-LDS limit raised where it needs more than 64 KiB, then the launch.
inline int launch_kernel(void (*kernel)(ConvArgs), int nblk, int threads, int lds, hipStream_t st,
                         const ConvArgs& a) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  ConvArgs arg = a;
  void* params[] = {&arg};
  hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3((unsigned)nblk),
                                 dim3(threads), params, (size_t)lds, st);
  return e != hipSuccess ? (int)e : vrvq_launch_status();
}

template <int N>
const ConvKernel* find_kernel(const ConvKernel (&table)[N], const ConvPlan& p) {
  const unsigned key = plan_key(p);
  for (const ConvKernel& k : table)
    if (k.key == key) return &k;
  return nullptr;
}

// The plan's kernel (a.n_mt / n_nt / ks_split set from the plan by the caller), for a split-K
// plan followed by its epilogue launch; VRVQ_ERR_UNSUPPORTED where the table has none.
template <int N>
int launch_plan(const ConvKernel (&table)[N], const ConvPlan& p, const ConvArgs& a,
                hipStream_t st) {
  const ConvKernel* k = find_kernel(table, p);
  if (k == nullptr) return VRVQ_ERR_UNSUPPORTED;
  int rc = launch_kernel(k->main, p.grid, k->threads, p.lds, st, a);
  if (rc == 0 && k->epilogue != nullptr)
    rc = launch_kernel(k->epilogue, p.grid / p.S, k->threads, p.lds_epi, st, a);
  return rc;
}

// What each conv_k*.hip exports: whether its table holds the plan's kernel (host only), and the
// launch.
struct ConvTable {
  bool (*has)(const ConvPlan&);
  int (*launch)(const ConvPlan&, const ConvArgs&, hipStream_t);
};
#define VRVQ_CONV_TABLE(name)                                         \
  bool name##_has(const ConvPlan&);                                   \
  int name##_launch(const ConvPlan&, const ConvArgs&, hipStream_t);   \
  constexpr ConvTable name{name##_has, name##_launch}
VRVQ_CONV_TABLE(conv_k1);
VRVQ_CONV_TABLE(conv_k1_x3);
VRVQ_CONV_TABLE(conv_k2);
VRVQ_CONV_TABLE(conv_k2_x3);
VRVQ_CONV_TABLE(conv_k2_view);
VRVQ_CONV_TABLE(conv_k3);
VRVQ_CONV_TABLE(conv_k3_x3);
VRVQ_CONV_TABLE(conv_k4);
VRVQ_CONV_TABLE(conv_k7);
VRVQ_CONV_TABLE(conv_k7_x3);
VRVQ_CONV_TABLE(conv_k8);
VRVQ_CONV_TABLE(conv_k16);
#undef VRVQ_CONV_TABLE

}  // namespace vrvq_conv
