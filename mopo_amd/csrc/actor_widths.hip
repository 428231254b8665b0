// The rollout actor at the kernel widths 64, 96, ..., 224 (actor.h actor_kernel_hidden: every policy width up
// to 256 is zero-embedded into the next multiple of 32 by pack_actor).  The kernels are actor_kernels.h's
// templates; they are instantiated here, in a translation unit of their own, so that the two product kernels
// of actor.hip (widths 32 and 256) keep the register allocation they were tuned and measured with.
// f16x3 runs actor_f16_kernel at these widths whether or not another launch runs beside it (the ring form
// actor_f16q_kernel is the 256-wide product kernel's only).
#include "actor_kernels.h"

namespace mopo {

template <int NB>
static int launch_actor_nb(const ActorArgs& a, hipStream_t s) {
  dim3 grid(ceil_div((int)a.B, 16 * ACT_WAVES)), block(64 * ACT_WAVES);
  if (a.dtype == DT_BF16X6) hipLaunchKernelGGL(actor_x6_kernel<NB>, grid, block, 0, s, a);
  else if (a.dtype == DT_F16X3) hipLaunchKernelGGL(actor_f16_kernel<NB>, grid, block, 0, s, a);
  else if (a.dtype != DT_FP32) return fail("actor: dtype must be 0 (fp32), 3 (bf16x6) or 4 (f16x3)");
  else if (a.O > 16) hipLaunchKernelGGL((actor_kernel<2, NB>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((actor_kernel<1, NB>), grid, block, 0, s, a);
  MOPO_HIP(hipGetLastError());
  return 0;
}

// called by launch_actor (actor.hip) behind its argument checks
int launch_actor_widths(const ActorArgs& a, hipStream_t s) {
  switch (actor_kernel_hidden(a.Hp) / 32) {
    case 2: return launch_actor_nb<4>(a, s);
    case 3: return launch_actor_nb<6>(a, s);
    case 4: return launch_actor_nb<8>(a, s);
    case 5: return launch_actor_nb<10>(a, s);
    case 6: return launch_actor_nb<12>(a, s);
    case 7: return launch_actor_nb<14>(a, s);
  }
  return fail("actor: unsupported hidden size (up to 256)");
}

}  // namespace mopo
