// The ensemble forward at 8 and 16 hidden blocks of 16 (H = 128 and 256, and every narrower logical width
// that mopo_bnn_create rounds up to them: internal.h bnn_form_blocks), exact-f32 MFMA form.
//
// The kernels are bnn_kernels.h's templates; they are instantiated here, in a translation unit of their own,
// so that the kernels of bnn.hip keep the register allocation they were tuned and measured with.  The 16-bit
// forms of the same widths are in bnn_widths16.hip.
#include "bnn_kernels.h"

namespace mopo {

// one row block per wave at both widths: 16 blocks hold 64 accumulator + 64 input registers per row block
template <int KG0, int NBO>
static int launch_widths_h(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  switch (h->dev.NBH) {
    case 8: return launch_fwd_t<KG0, 8, NBO, 1>(h, mode, a, s);
    case 16: return launch_fwd_t<KG0, 16, NBO, 1>(h, mode, a, s);
  }
  return fail("bnn: launch_bnn_fwd_widths runs 8 or 16 hidden blocks");
}

int launch_bnn_fwd_widths(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (h->dtype != DT_FP32) return launch_bnn_fwd_widths16(h, mode, a, s);
  const BnnDev& d = h->dev;
  if (d.KG0 == 4 && d.NBO == 4) return launch_widths_h<4, 4>(h, mode, a, s);   // wide models: one padded form
  if (d.KG0 == 2 && d.NBO == 3) return launch_widths_h<2, 3>(h, mode, a, s);   // 17 + 6
  if (d.KG0 == 2 && d.NBO == 2) return launch_widths_h<2, 2>(h, mode, a, s);
  if (d.KG0 == 1 && d.NBO == 2) return launch_widths_h<1, 2>(h, mode, a, s);   // 11 + 3
  return fail("bnn: unsupported input / output dims at hidden widths 65..128 and 209..256");
}

}  // namespace mopo
