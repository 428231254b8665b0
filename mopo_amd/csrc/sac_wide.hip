// The wide forms of the SAC step's forward row-block kernels (sac_rows.h: critic inputs obs_dim + act_dim in
// [32, 39], layer 1 as WIDE_KS 4-deep k-steps), launched by sac.hip for handles with obs_dim + act_dim >= 32.
// B1 (dh1_block) is the narrow kernels' own: only the forward blocks' layer 1 depends on the input width.
#define MOPO_GEMM_KERNELS 0   // the helpers of gemm_group.h only
#define MOPO_SAC_NARROW_KERNELS 0   // sac_rows.h's non-template narrow kernels are sac.hip's
#include "sac_rows.h"

namespace mopo {

template <bool HEAD>
static __global__ __launch_bounds__(256, 2) void sac_fwd_wide_kernel(const FwdArgsR a) {
  __shared__ __attribute__((aligned(16))) FwdLds L;
  fwd_block<HEAD, 0, WIDE_KS>(a, blockIdx.x, blockIdx.y, blockIdx.z, L);
}

static __global__ __launch_bounds__(256, 2) void sac_f2b1_wide_kernel(const FwdArgsR f, const Dh1Args b) {
  __shared__ __attribute__((aligned(16))) F2B1Lds S;
  if (blockIdx.z < 4)
    fwd_block<true, 1, WIDE_KS>(f, blockIdx.x, blockIdx.y, blockIdx.z, S.f);
  else
    dh1_block<1>(b, blockIdx.x, blockIdx.y, blockIdx.z - 4, S.b);
}

static __global__ __launch_bounds__(256, 2) void sac_f12b1_wide_kernel(const FwdArgsR f1, const FwdArgsR f2,
                                                                       const Dh1Args b) {
  __shared__ __attribute__((aligned(16))) F2B1Lds S;
  if (blockIdx.z < 4)
    fwd_block<false, 2, WIDE_KS>(f1, blockIdx.x, blockIdx.y, blockIdx.z, S.f);
  else if (blockIdx.z < 8)
    fwd_block<true, 2, WIDE_KS>(f2, blockIdx.x, blockIdx.y, blockIdx.z - 4, S.f);
  else
    dh1_block<2>(b, blockIdx.x, blockIdx.y, blockIdx.z - 8, S.b);
}

void sac_launch_fwd_wide(bool head, const FwdArgsR& f, hipStream_t s) {
  const dim3 grid(f.ncq, f.nrb, 4);
  if (head) hipLaunchKernelGGL(sac_fwd_wide_kernel<true>, grid, dim3(256), 0, s, f);
  else hipLaunchKernelGGL(sac_fwd_wide_kernel<false>, grid, dim3(256), 0, s, f);
}

void sac_launch_f2b1_wide(const FwdArgsR& f2, const Dh1Args& b, hipStream_t s) {
  hipLaunchKernelGGL(sac_f2b1_wide_kernel, dim3(f2.ncq, f2.nrb, 8), dim3(256), 0, s, f2, b);
}

void sac_launch_f12b1_wide(const FwdArgsR& f1, const FwdArgsR& f2, const Dh1Args& b, hipStream_t s) {
  hipLaunchKernelGGL(sac_f12b1_wide_kernel, dim3(f1.ncq, f1.nrb, 12), dim3(256), 0, s, f1, f2, b);
}

}  // namespace mopo
