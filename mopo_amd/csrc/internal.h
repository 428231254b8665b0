// Internal declarations shared by the libmopo_hip translation units.
#pragma once
#include "common.h"
#include "../../include/mopo_hip.h"

namespace mopo {

constexpr int MAX_IN_KG = 4;  // layer-0 input features <= 64
// A "wide" ensemble has more than 32 inputs or more than 3 head blocks (D = obs_dim + 1 > 24), e.g. ant's
// 27 + 8.  Every wide shape runs ONE padded form per hidden width: KG0 = 4 input k-groups of 16 (two of 32
// in the 16-bit kernels) and NBO = 4 head blocks; unused slots are zero weights (slot_feat / head_col: -1).
__host__ __device__ constexpr bool bnn_wide(int IN, int D) { return IN > 32 || D > 24; }

// Device view of a packed ensemble.  Weight matrices are stored "fragment-major": for
// layer input K (KG = ceil(K/16) k-groups) and output N (NB = ceil(N/16) blocks), member e,
// fragment (kg, nb) is 64 lanes x 4 floats contiguous (1 KiB):
//   frag[((e*KG + kg)*NB + nb)*256 + lane*4 + t] = W[e][kg*16 + 4*(lane>>4) + t][nb*16 + (lane&15)]
// i.e. exactly the per-lane A operand of 4 consecutive v_mfma_f32_16x16x4_f32 steps.
struct BnnDev {
  int E, O, A, IN, H, D;
  int KG0, NBH, NBO;  // layer-0 k-groups, hidden blocks (= hidden k-groups), head blocks
  const float* w0;    // [E][KG0][NBH] frags
  const float* wh;    // [3][E][NBH][NBH] frags
  const float* whd;   // [E][NBH][NBO] frags (head: n < D mean, D <= n < 2D log-var)
  const float* b0;    // [E][NBH*16]
  const float* bh;    // [3][E][NBH*16]
  const float* bhd;   // [E][NBO*16]
  const float* mu;    // [IN]
  const float* sigma; // [IN]
  const float* maxlv; // [D]
  const float* minlv; // [D]
  int BS;             // per-member bias stride (floats): even(NBH) * 16
  // bf16 fragments (dtype 1..3): 1 KiB = 64 lanes x 8 bf16 per (32-deep k-group, 16-wide block),
  // addressed in float units like the f32 fragments; hidden width padded to NB2 = even(NBH)
  int NB2;
  const float* w0b;   // [E][KG0B][P][NB2], KG0B = (KG0 + 1) / 2 input k-groups of 32 (1; wide models 2)
  const float* whb;   // [3][E][NB2/2][P][NB2]  (bnn_kpack: [3][E][(NB2/2 - 1) P + 1][NB2], the last the packed remainder)
  const float* whdb;  // [E][NB2/2][P][NBO]       (bnn_kpack: [E][(NB2/2 - 1) P + 1][NBO])
  const float* wscale;  // f16x3: [5][E] inverse power-of-two weight scales (layer 0, hidden 1..3, head)
};

enum { DT_FP32 = 0, DT_BF16 = 1, DT_BF16X3 = 2, DT_BF16X6 = 3, DT_F16X3 = 4 };
// 16-bit parts per operand of a dtype (1 bf16, 2 bf16x3, 3 bf16x6, 2 f16x3; mlp_tile.h split_*)
__host__ __device__ constexpr int bf16_parts(int dtype) { return dtype < 1 ? 1 : (dtype == DT_F16X3 ? 2 : dtype); }

// k-steps a consumer must run in the last 16-deep k-group of a width-F input (4: no skip; mlp_tile.h slot_feat)
__host__ __device__ constexpr int tail_steps(int F) { return (F & 15) == 0 ? 4 : ((F & 15) + 3) >> 2; }

// Packed remainder k-group (mlp_tile.h kpack_slot): bf16x6 at H = 197..200, where the last 32-deep k-group of a
// hidden-width input holds 2 real values per lane.  The packer (mopo_bnn_set_params) and every launch
// decide from this one predicate; whb / whdb then hold (KG - 1) P + 1 slices per member instead of KG P.
__host__ __device__ constexpr bool bnn_kpack(int dtype, int NB2, int NBH, int H) {
  return dtype == DT_BF16X6 && NB2 == 14 && NBH == 13 && tail_steps(H) == 2;
}

// ---- hidden-width forms --------------------------------------------------------------------------------------
// The forward kernels exist for a few hidden-block counts ("forms"): 2, 4, 8, 13, 16 and 25 blocks of 16.  A
// logical hidden width H with no form of its own runs on the smallest form that holds it: the packer
// (mopo_bnn_set_params) lays the H real units into the form's slots (slot_feat) and fills the rest with zero
// weights and biases, and swish(0) = 0, so the padded units contribute exact zeros.  Every API keeps H.
// Returns the form's block count for (H, dtype, wide), or -1 where no kernel runs it.  The forms of 8 and 16
// blocks are bnn_widths.hip's; block counts that ran before they existed keep the kernel they had.
inline int bnn_form_blocks(int hidden, int dtype, bool wide) {
  if (hidden < 1) return -1;
  const int nb = (hidden + 15) / 16;
  const bool split = dtype == 3 /* bf16x6 */ || dtype == 4 /* f16x3 */;
  if (!wide && dtype != 0) {
    // odd counts the non-ring 16-bit kernels take as they are (their NBU = NB2 - 1 forms), and 26 whole blocks
    if (dtype != 4 && (nb == 1 || nb == 3)) return nb;
    if (dtype != 3 && nb == 26) return nb;
    if (!split) return (nb == 2 || nb == 4 || nb == 13 || nb == 25) ? nb : -1;   // bf16, bf16x3: no new forms
  }
  if (wide && dtype != 0 && !split) return -1;
  const int forms[6] = {2, 4, 8, 13, 16, 25};
  // 16-bit limits: bf16x6 has no form above 16 blocks, a wide model none above 13
  const int top = dtype == 0 ? 25 : (wide ? 13 : (dtype == 3 ? 16 : 25));
  for (int f : forms)
    if (f >= nb && f <= top) return (f == 25 && nb < 25) ? -1 : f;   // H = 257..384: refused, not run at 400's cost
  return -1;
}
// The width the device form runs for a logical width: H itself where H lies in the last block of a form that
// takes partial blocks (every width that ran before the 8- and 16-block forms existed), otherwise the form's
// smallest own width (whole blocks for the forms of 8 and 16).  Monotone in H, >= H, -1 where refused.
inline int bnn_device_hidden(int hidden, int dtype, bool wide) {
  const int f = bnn_form_blocks(hidden, dtype, wide);
  if (f < 0) return -1;
  const int lo = (f == 8 || f == 16) ? 16 * f : 16 * (f - 1) + 1;
  return hidden > lo ? hidden : lo;
}

static const char* const kWide16Msg =
    "bnn: a wide model (obs_dim + act_dim > 32 or obs_dim > 23) runs in fp32 at every hidden size up to 256 and at "
    "385..400, and in bf16x6 / f16x3 at every hidden size up to 208; bf16, bf16x3 and "
    "other hidden sizes are not supported there";
static const char* const kWidths16Msg =
    "bnn: hidden sizes 65..128 and 209..256 run in fp32, bf16x6 and f16x3 (a wide model -- obs_dim + act_dim > 32 or "
    "obs_dim > 23 -- in fp32, and up to 128 in bf16x6 / f16x3); bf16 and bf16x3 are not supported there";

// ---- which forward form runs a shape ---------------------------------------------------------------------------
// The head kernels that exist for a narrow shape (at most 32 inputs, obs_dim <= 23), per dtype class and hidden
// form: fp32 has head-block counts NBO = 2 and 3 at every form; the 16-bit kernels 2 and 3 at 4, 8, 13 and 16
// hidden blocks (NB2 = 4, 8, 14, 16) and 3 alone at 1..2 and 25..26 (NB2 = 2, 26).  No form has a 1-block head.
// This is the table launch_bnn_fwd's arms (bnn.hip, bnn_widths.hip, bnn_widths16.hip) spell out as template
// arguments; a handle whose NBO came from bnn_forward_form always finds its arm.
inline bool bnn_head_kernel(int dtype, int nb2, int nbo) {
  if (nbo == 3) return true;
  if (nbo != 2) return false;
  return dtype == 0 || (nb2 != 2 && nb2 != 26);
}

// The form of a handle: layer-0 k-groups, hidden blocks, head blocks, wide (bnn_wide), device hidden width.
struct BnnForm {
  int KG0, NBH, NBO, wide, HD;
};

// THE statement of which forward kernel runs (obs_dim, act_dim, hidden, dtype): fills *f and returns nullptr, or
// returns the limit the shape breaks (no kernel runs it).  mopo_bnn_create builds its handle from this answer and
// the export mopo_bnn_forward_form gives it to callers; the launch dispatch only reads the handle.
// The head takes the smallest block count >= ceil(2 D / 16) that the (dtype, hidden form) has a kernel for:
// head_col leaves the slots beyond 2 D empty, the packers turn them into zero weights, and the head epilogue
// works from D alone, so the spare blocks compute and store nothing.
inline const char* bnn_forward_form(int obs_dim, int act_dim, int hidden, int dtype, BnnForm* f) {
  if (obs_dim < 1 || act_dim < 1) return "bad obs/act dims (both must be >= 1)";
  if (dtype < 0 || dtype > 4) return "dtype must be 0 (fp32), 1 (bf16), 2 (bf16x3), 3 (bf16x6) or 4 (f16x3)";
  const int IN = obs_dim + act_dim, D = obs_dim + 1;
  if (IN > 16 * MAX_IN_KG || D > 32) return "obs_dim + act_dim must be <= 64 and obs_dim <= 31";
  const bool wide = bnn_wide(IN, D);
  const bool split = dtype == DT_BF16X6 || dtype == DT_F16X3;
  const int nb = (hidden + 15) / 16, nb2 = (nb + 1) / 2 * 2;
  // every width up to 208 has a wide 16-bit ring form
  if (wide && dtype != DT_FP32 && !(split && nb <= 13))
    return kWide16Msg;
  // the 16-bit kernels' NB2 = 14 shape is H = 200's 13 blocks: bf16x6 / f16x3 run 209..224 on 16 blocks
  if ((dtype == DT_BF16 || dtype == DT_BF16X3) && nb2 == 14 && nb != 13)
    return "bf16 and bf16x3 do not support hidden sizes 209..224 (use fp32, bf16x6 or f16x3)";
  if (dtype == DT_BF16X6 && nb2 > 16)   // launch_bf16_t: no bf16x6 kernel above H = 256
    return "bf16x6 supports hidden sizes <= 256 (use f16x3 or fp32)";
  const int form = bnn_form_blocks(hidden, dtype, wide);
  if (form < 0) {
    if (dtype == DT_BF16 || dtype == DT_BF16X3)
      return "bf16 and bf16x3 run hidden sizes up to 64, 193..208 and 385..416 only (fp32, bf16x6 and f16x3 run "
             "every hidden size up to 256)";
    return "no kernel for this hidden size (every hidden size up to 256 runs in fp32, bf16x6 and f16x3, 385..400 in "
           "fp32 and f16x3; a wide model's bf16x6 / f16x3 stop at 208)";
  }
  BnnForm r;
  r.wide = wide ? 1 : 0;
  r.KG0 = wide ? MAX_IN_KG : (IN + 15) / 16;
  r.NBH = form;
  r.HD = bnn_device_hidden(hidden, dtype, wide);
  r.NBO = wide ? 4 : (2 * D + 15) / 16;
  if (!wide) {
    const int fb2 = (form + 1) / 2 * 2;
    while (r.NBO < 3 && !bnn_head_kernel(dtype, fb2, r.NBO)) ++r.NBO;
  }
  if (f) *f = r;
  return nullptr;
}

struct Bnn {
  int E, O, A, H, smv, dtype;
  int HD = 0;  // bnn_device_hidden(H): the width the tail-skipping and packed-remainder choices are made from
  bool has_params = false;
  float* buf = nullptr;      // one device allocation for all packed params
  uint16_t* bbuf = nullptr;  // bf16 packed weights
  int64_t buf_bytes = 0, bbuf_bytes = 0;  // sizes of buf / bbuf (mopo_bnn_packed_copy)
  BnnDev dev{};
  // mopo_fakeenv_step, penalty kinds >= 2: the [pen_rows] ready penalties of penalty.hip, grown on demand
  float* pen_buf = nullptr;
  int64_t pen_rows = 0;
};

// Input view: features [0, O) from xa (row stride sa), [O, IN) from xb (row stride sb).
struct FwdIn {
  const void* xa; int xa_f64; int64_t sa;
  const void* xb; int xb_f64; int64_t sb;
};

enum { FWD_PREDICT = 0, FWD_ROLLOUT = 1 };
constexpr int XS_STRIDE = 32;  // floats per pre-scaled input row (FwdArgs::xs): 2 k-groups of slots
// wide models (more than 32 inputs or more than 3 head blocks: BnnDev::KG0 = 4): 4 k-groups of slots
constexpr int XS_STRIDE_WIDE = 64;
__host__ __device__ constexpr int xs_stride(int kg0) { return kg0 > 2 ? XS_STRIDE_WIDE : XS_STRIDE; }

struct FwdArgs {
  FwdIn in;
  int64_t B;              // launch rows (grid sized for this)
  const int* d_count;     // optional device row count (<= B)
  // optional pre-scaled input rows [B][32] f32 in slot_feat order (written once per row by the
  // rollout's actor; wide models: [B][64], written by rollout_xs_wide_kernel): replaces the per-member
  // f64 obs / act loads and scaler transform
  const float* xs;
  int ntiles;             // tiles per member in the grid
  int xcd_members;        // H = 400 f16x3 kernel: 1 = every XCD owns E / 8 members (set by launch_f16s)
  // predict outputs
  float* mean;            // [E][B][D]
  float* var;
  // rollout outputs
  uint32_t* pen_bits;     // [B] max_e ||std_e|| (as ordered uint bits)
  const int32_t* sel;     // [B] selected member per row
  float* mean_sel;        // [B][D]
  float* std_sel;         // [B][D]
  // rollout, optional: every member's mean / std (mean-distance penalty and deterministic mode,
  // fake_env.py:84-86, 98-108): [E][all_stride][D], row r of this launch at all_stride rows apart
  float* mean_all;
  float* std_all;
  int64_t all_stride;
};

int launch_bnn_fwd(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s);
// the forms of 8 and 16 hidden blocks (bnn_widths.hip: fp32; bnn_widths16.hip: bf16x6, f16x3)
int launch_bnn_fwd_widths(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s);
int launch_bnn_fwd_widths16(const Bnn* h, int mode, const FwdArgs& a, hipStream_t s);
// W[E][K][N] (TF layout) -> fragment-major (see BnnDev) on stream s
// perm_k: the K side is an input width in slot_feat order (mlp_tile.h)
// perm_n: the N side likewise (1), or the fused head's head_col order (2)
int pack_frags(const float* src, float* dst, int E, int K, int N, int KG, int NB, hipStream_t s, int perm_k = 0,
               int perm_n = 0);
// the other packers of mopo_bnn_set_params (bnn_pack.h): hidden biases [E][N] -> slot order [E][NP] times mul;
// 16-bit fragments of P parts per k-group of 32 (scale: f16x3's per-member 2^k, else the bf16 split; mstride:
// fragments per member in dst); the packed remainder k-group KG - 1 of a bf16x6 input (bnn_kpack)
int pack_bias(const float* src, float* dst, int E, int N, int NP, float mul, hipStream_t s);
int pack_frags16(const float* src, short* dst, int E, int K, int N, int KG, int NB, int perm_n, int P,
                 const float* scale, int64_t mstride, hipStream_t s);
int pack_frags_kpack(const float* src, short* dst, int E, int K, int N, int KG, int NB, int perm_n, int64_t mstride,
                     hipStream_t s);

// termination kinds (mopo/static)
// nobs: next_obs[d] for d < O -- an array or any accessor callable with d
template <class F>
__device__ __forceinline__ bool term_fn_at(int kind, const F& nobs, int O) {
  if (kind == MOPO_TERM_WALKER2D) {  // walker2d.py:10-16
    double hh = nobs(0), an = nobs(1);
    bool not_done = (hh > 0.8) && (hh < 2.0) && (an > -1.0) && (an < 1.0);
    return !not_done;
  }
  if (kind == MOPO_TERM_HOPPER) {  // hopper.py:10-17 (np.abs(bool) == bool)
    bool fin = true, small = true;
    for (int d = 0; d < O; ++d) {
      double v = nobs(d);
      fin = fin && isfinite(v);
      if (d >= 1) small = small && (v < 100.0);
    }
    double hh = nobs(0), an = nobs(1);
    bool not_done = fin && small && (hh > 0.7) && (fabs(an) < 0.2);
    return !not_done;
  }
  if (kind == MOPO_TERM_ANT) {  // ant.py:9-15, antangle.py:9-15
    bool fin = true;
    for (int d = 0; d < O; ++d) fin = fin && isfinite(nobs(d));
    double x = nobs(0);
    bool not_done = fin && (x >= 0.2) && (x <= 1.0);
    return !not_done;
  }
  if (kind == MOPO_TERM_HUMANOID) {  // humanoid.py:10-11 (NaN compares false: not done)
    double z = nobs(0);
    return (z < 1.0) || (z > 2.0);
  }
  return false;  // halfcheetah.py:9-10 and the other never-done domains
}

__device__ __forceinline__ bool term_fn(int kind, const double* nobs, int O) {
  return term_fn_at(kind, [&](int d) { return nobs[d]; }, O);
}

}  // namespace mopo
