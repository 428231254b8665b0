// The 16-bit forms (bf16x6, f16x3) of the ensemble forward at 8 and 16 hidden blocks (bnn_widths.hip has the
// fp32 ones and the reason for the separate translation units): the ring kernel of bnn_kernels.h at NB2 = 8
// and 16, whole even block counts, so no half-depth last k-group and no packed remainder.
//
// bf16x6 at 16 blocks is the one shape with knobs of its own (BNN_RING_PF_X6_16, BNN_RING_MINB_X6_16): its
// registers are capped for 2 workgroups per CU, not 3 -- at 3 it spilled at every prefetch depth.
#include "bnn_kernels.h"

namespace mopo {

template <int NB2, int NBO, int KG0B = 1>
static int launch_widths16_t(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (!ring_shape<NB2>(h)) return fail("bnn: 16-bit hidden block count does not match its handle");
  if (h->dtype == DT_F16X3) return launch_ring<NB2, NBO, 2, BNN_RING_DEPTH_F16, KG0B>(h, mode, a, s);
  if (h->dtype == DT_BF16X6) return launch_ring_x6<NB2, NBO, KG0B>(h, mode, a, s);
  return fail(kWidths16Msg);
}

int launch_bnn_fwd_widths16(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  const BnnDev& d = h->dev;
  if (bnn_wide(d.IN, d.D)) {   // 2 input k-groups of 32, 4 head blocks; 16 blocks have no wide 16-bit form
    if (d.NB2 == 8) return launch_widths16_t<8, 4, 2>(h, mode, a, s);
    return fail(kWidths16Msg);
  }
  if (d.NBO == 3) {
    if (d.NB2 == 8) return launch_widths16_t<8, 3>(h, mode, a, s);
    if (d.NB2 == 16) return launch_widths16_t<16, 3>(h, mode, a, s);
  } else if (d.NBO == 2) {
    if (d.NB2 == 8) return launch_widths16_t<8, 2>(h, mode, a, s);
    if (d.NB2 == 16) return launch_widths16_t<16, 2>(h, mode, a, s);
  }
  return fail("bnn 16-bit: unsupported hidden/output size");
}

}  // namespace mopo
