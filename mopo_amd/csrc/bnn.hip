// Ensemble forward dispatch: which kernel of bnn_kernels.h runs a handle's shape and dtype.  This unit owns the
// forms of 2, 4, 13 and 25 / 26 hidden blocks (H <= 64, 193..208, 385..416) and instantiates their kernels;
// 8 and 16 blocks go to bnn_widths.hip / bnn_widths16.hip.  The C ABI is in bnn_api.hip; the weight-pack kernels
// (bnn_pack.h) are compiled in this unit, the one that gives them the code they always had.
#include "bnn_kernels.h"
#include "bnn_pack.h"

#include <string>

namespace mopo {

template <int KG0, int NBO>
static int launch_fwd_h(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  switch (h->dev.NBH) {
    case 2: return launch_fwd_t<KG0, 2, NBO, 2>(h, mode, a, s);
    case 4: return launch_fwd_t<KG0, 4, NBO, 2>(h, mode, a, s);
    case 13:  // H = 200 with 17 + 6 inputs (every halfcheetah / walker2d config): skip the padding k-steps
      if constexpr (KG0 <= 2)   // the wide form (KG0 = 4) has the whole-k-group variant only
        if (KG0 == 2 && NBO == 3 && tail_steps(h->dev.IN) <= 2 && tail_steps(h->HD) <= 2)
          return launch_fwd_t<KG0, 13, NBO, BNN_R13, 2, 2>(h, mode, a, s);
      return launch_fwd_t<KG0, 13, NBO, BNN_R13>(h, mode, a, s);
    case 25:
      if constexpr (KG0 <= 2)
        if (KG0 == 2 && NBO == 3 && tail_steps(h->dev.IN) <= 2) return launch_fwd_t<KG0, 25, NBO, 1, 2, 4>(h, mode, a, s);
      return launch_fwd_t<KG0, 25, NBO, 1>(h, mode, a, s);
  }
  return fail("bnn: unsupported hidden size (supported: 32, 64, 200, 400; got H=" +
              std::to_string(h->H) + ")");
}

// split kernels (P > 1): one slice per k-group holding all P weight parts (every slice then feeds
// P (P + 1) / 2 MFMAs per block, so the copy of the next slice hides behind uniform work) is BNN_SPLIT_PS = 0;
// the tuned form stages one part per slice, BNN_SPLIT_WAVES waves per workgroup sharing the LDS
template <int NB2, int NBO, int P>
static int launch_bf16_p(const Bnn* h, int mode, FwdArgs a, hipStream_t s) {
  if constexpr (P == 1 && BNN_BF16_RING && NB2 <= 16)
    if (ring_shape<NB2>(h)) return launch_ring<NB2, NBO, 1, BNN_RING_DEPTH_BF16>(h, mode, a, s);
  if constexpr (P == 3 && BNN_BF16X6_RING && NB2 <= 16)
    if (ring_shape<NB2>(h)) return launch_ring_x6<NB2, NBO>(h, mode, a, s);
  // bnn_fwd_bf16_kernel reads the unpacked [kg][p][nb] layout only
  if (kpack_shape(h)) return fail("bnn bf16x6: a packed-remainder shape (H = 197..200) runs on the ring kernel only");
  constexpr int WV = P == 1 ? FWD_WAVES : BNN_SPLIT_WAVES;
  constexpr int PS = P == 1 ? 1 : (BNN_SPLIT_PS == 0 ? P : BNN_SPLIT_PS);
  a.ntiles = (int)ceil_div((int)a.B, 16);
  if (a.ntiles == 0) return 0;
  dim3 grid(ceil_div(a.ntiles, WV) * h->E), block(64 * WV);   // = 8 groups (E / 8) when the XCDs own members
  a.xcd_members = (BNN_BF16_XCDMEM && h->E % (8 * BNN_BF16_XCDMEM) == 0) ? BNN_BF16_XCDMEM : 0;
  // NBU, the hidden blocks in use: an odd block count leaves the last block of NB2 all padding, and it is skipped
  auto launch = [&](auto nbu) {
    with_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((bnn_fwd_bf16_kernel<NB2, NBO, decltype(m)::value, WV, P, PS, decltype(nbu)::value>), grid, block,
                         0, s, h->dev, a);
    });
  };
  const bool odd = h->dev.NBH == NB2 - 1;
  if constexpr (NB2 == 14) {   // H = 193..208 (13 blocks) only: the whole-block form is not built (it spilled 8-12 B)
    if (!odd) return fail("bnn bf16: unsupported hidden size (H in (192, 224] runs at H <= 208 only)");
    launch(std::integral_constant<int, NB2 - 1>{});
  } else if constexpr (NB2 <= 16) {   // 2 and 4 blocks: H <= 64, either parity
    if (odd) launch(std::integral_constant<int, NB2 - 1>{});
    else launch(std::integral_constant<int, NB2>{});
  } else {   // H = 385..416 runs all 26 blocks: the skipping variant takes 256 VGPRs there and spills
    launch(std::integral_constant<int, NB2>{});
  }
  MOPO_HIP(hipGetLastError());
  return 0;
}

template <int NB2, int NBO>
static int launch_f16s(const Bnn* h, int mode, FwdArgs a, hipStream_t s) {
  constexpr int WV = BNN_SPLIT_WAVES, PS = BNN_SPLIT_PS == 0 ? 2 : BNN_SPLIT_PS;
  a.ntiles = (int)ceil_div((int)a.B, 16);
  if (a.ntiles == 0) return 0;
  // H <= 256 runs the ring kernel: every supported hidden size there has a ring shape
  if constexpr (BNN_F16_RING && NB2 <= 16) {
    if (ring_shape<NB2>(h)) return launch_ring<NB2, NBO, 2, BNN_RING_DEPTH_F16>(h, mode, a, s);
    return fail("bnn f16x3: unsupported hidden size");
  }
#if BNN_F16_XCD
  dim3 grid(8 * ceil_div(ceil_div(a.ntiles, WV), 8) * h->E), block(64 * WV);
#else
  dim3 grid(ceil_div(a.ntiles, WV) * h->E), block(64 * WV);
#endif
  // NBU, the hidden blocks in use: bnn_fwd_f16s_kernel skips the padding block of an odd count at H <= 256 only
  auto launch_s = [&](auto nbu) {
    with_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((bnn_fwd_f16s_kernel<NB2, NBO, decltype(m)::value, WV, PS, decltype(nbu)::value>), grid, block, 0,
                         s, h->dev, a);
    });
  };
  const bool odd = h->dev.NBH == NB2 - 1;
  if constexpr (NB2 > 16) {
    // H = 385..400 (25 blocks): the column-half kernel, two workgroups per CU.  H = 401..416 (26 whole blocks), and
    // BNN_F16_HALF = 0 builds: bnn_fwd_f16s_kernel over all 26 -- the register allocation it gets with 25 of 26
    // (VGPR + AGPR split) measured 17 % slower
    if (BNN_F16_HALF && odd) {
      if constexpr (BNN_F16_HALF) {
        a.xcd_members = (BNN_F16H_XCDMEM && h->E % 8 == 0) ? 1 : 0;
        if (a.xcd_members) grid = dim3(8 * ceil_div(a.ntiles, WV) * (h->E / 8));   // (XCD, member, row group)
        with_mode(mode, [&](auto m) {
          hipLaunchKernelGGL((bnn_fwd_f16h_kernel<NB2, NBO, decltype(m)::value, WV, NB2 - 1>), grid, block, 0, s, h->dev, a);
        });
      }
    } else {
      launch_s(std::integral_constant<int, NB2>{});
    }
  } else {
    // H <= 256 off the ring: run by BNN_F16_RING = 0 A/B builds only.  The default build returns above but still
    // compiles these instantiations, as it always has (the library's kernel set is kept as it is)
    if (odd) launch_s(std::integral_constant<int, NB2 - 1>{});
    else launch_s(std::integral_constant<int, NB2>{});
  }
  MOPO_HIP(hipGetLastError());
  return 0;
}

template <int NB2, int NBO>
static int launch_bf16_t(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (h->dtype == DT_F16X3) return launch_f16s<NB2, NBO>(h, mode, a, s);
  switch (bf16_parts(h->dtype)) {
    case 2: return launch_bf16_p<NB2, NBO, 2>(h, mode, a, s);
    case 3:
      // bf16x6 at H > 256: its 39-slice layer loop does not unroll (the part index goes dynamic: 432 B of
      // scratch per lane, a ~70x cliff) -- f16x3 is the f32-accurate 16-bit mode there
      if constexpr (NB2 > 16) return fail("bnn bf16x6: hidden sizes <= 256 only (use f16x3 or fp32 at H = 400)");
      else return launch_bf16_p<NB2, NBO, 3>(h, mode, a, s);
  }
  return launch_bf16_p<NB2, NBO, 1>(h, mode, a, s);
}

// wide models (bnn_wide: 2 input k-groups of 32, 4 head blocks) on the ring kernel: bf16x6 and f16x3 at H = 32, 64, 200
template <int NB2>
static int launch_wide16(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (!ring_shape<NB2>(h)) return fail(kWide16Msg);
  if (h->dtype == DT_F16X3) return launch_ring<NB2, 4, 2, BNN_RING_DEPTH_F16, 2>(h, mode, a, s);
  if (h->dtype == DT_BF16X6) return launch_ring_x6<NB2, 4, 2>(h, mode, a, s);
  return fail(kWide16Msg);
}

static int launch_bf16(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (bnn_wide(h->dev.IN, h->dev.D)) {
    switch (h->dev.NB2) {
      case 2: return launch_wide16<2>(h, mode, a, s);
      case 4: return launch_wide16<4>(h, mode, a, s);
      case 14: return launch_wide16<14>(h, mode, a, s);
    }
    return fail(kWide16Msg);
  }
  if (h->dev.NBO == 3) {
    switch (h->dev.NB2) {
      case 2: return launch_bf16_t<2, 3>(h, mode, a, s);
      case 4: return launch_bf16_t<4, 3>(h, mode, a, s);
      case 14: return launch_bf16_t<14, 3>(h, mode, a, s);
      case 26: return launch_bf16_t<26, 3>(h, mode, a, s);
    }
  } else if (h->dev.NBO == 2) {
    switch (h->dev.NB2) {
      case 4: return launch_bf16_t<4, 2>(h, mode, a, s);
      case 14: return launch_bf16_t<14, 2>(h, mode, a, s);
    }
  }
  return fail("bnn bf16: unsupported hidden/output size");
}

int launch_bnn_fwd(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s) {
  if (!h->has_params) return fail("bnn: parameters not set (mopo_bnn_set_params)");
  if (h->dev.NBH == 8 || h->dev.NBH == 16) return launch_bnn_fwd_widths(h, mode, a, s);
  if (h->dtype != 0) return launch_bf16(h, mode, a, s);
  // wide models: one form per hidden width, 4 input k-groups and 4 head blocks (unused ones are zero padding)
  if (h->dev.KG0 == 4 && h->dev.NBO == 4) return launch_fwd_h<4, 4>(h, mode, a, s);
  if (h->dev.KG0 != 1 && h->dev.KG0 != 2) return fail("bnn: obs_dim + act_dim must be <= 64");
  const bool k1 = h->dev.KG0 == 1;  // hopper: 11 + 3 inputs
  switch (h->dev.NBO) {
    case 3: return k1 ? launch_fwd_h<1, 3>(h, mode, a, s) : launch_fwd_h<2, 3>(h, mode, a, s);
    case 2: return k1 ? launch_fwd_h<1, 2>(h, mode, a, s) : launch_fwd_h<2, 2>(h, mode, a, s);
  }
  return fail("bnn: unsupported output dim");
}

}  // namespace mopo
