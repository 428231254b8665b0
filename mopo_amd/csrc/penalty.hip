// Model-disagreement reward penalties beyond the reference's two (fake_env.py:98-110): the largest pairwise
// member discrepancy (MOReL's halt criterion) and the standard deviation of the ensemble taken as a mixture
// (aleatoric plus epistemic).  No reference counterpart; definitions in DESIGN section 2.
//
// One kernel between the ensemble forward and the FakeEnv post step.  It reads every member's head mean
// BEFORE the residual add (the residual is common to the members and cancels in every difference) and, for
// the mixture, every member's std or variance, and stores the penalty's f32 bits where the post kernels
// read a ready penalty (Rollout::pen; fakeenv.hip's scratch).
#include "penalty.h"
#include "rollout.h"

namespace mopo {

const char* const kPenaltyKindMsg =
    ": unknown penalty kind (0 mean_distance, 1 max_aleatoric, 2 max_pairwise, 3 ensemble_std)";

int check_halt(int halt, float halt_threshold, float halt_reward, const char* who) {
  const std::string w(who);
  MOPO_REQUIRE(halt == 0 || halt == 1, w + ": halt must be 0 (off) or 1 (on)");
  if (!halt) return 0;
  MOPO_REQUIRE(std::isfinite(halt_reward), w + ": halt_reward must be finite when halt = 1");
  MOPO_REQUIRE(!std::isnan(halt_threshold), w + ": halt_threshold must not be NaN when halt = 1");
  return 0;
}

// PEN_RPB rows per block, one 32-lane group per row and one lane per output dim d < D = O + 1, as
// rollout_post_kernel lays rows out: every load of a member's D values is contiguous across the row's lanes.
// Each lane keeps running scalars only (no per-thread arrays indexed by the runtime E or D: they would live
// in scratch); a member's values are re-read from the L1/L2-resident inputs where a pair needs them again.
// Per-row sums over d run a fixed __shfl_xor tree inside the 32-lane group, sums over members run in member
// order: the same bits whatever the launch shape, the split of the batch or the compaction.
constexpr int PEN_RPB = 8;
__global__ __launch_bounds__(256) void ensemble_penalty_kernel(const PenaltyArgs a) {
  const int tid = threadIdx.x, sub = tid & 31, rl = tid >> 5;
  const int64_t count = a.d_count ? (int64_t)*a.d_count : a.B;
  if ((int64_t)blockIdx.x * PEN_RPB >= count) return;   // whole block past the live rows
  const int64_t row = (int64_t)blockIdx.x * PEN_RPB + rl;
  const int E = a.E, D = a.O + 1;
  const bool live = row < count && row < a.B;
  const bool on = live && sub < D;
  const int64_t at = (on ? row : 0) * D + (on ? sub : 0);   // this lane's element of member 0
  const int64_t es = a.stride * D;                          // elements between two members
  float u;
  if (a.kind == MOPO_PENALTY_MAX_PAIRWISE) {
    // max_{i<j} sqrt(sum_{d=1..O} (mu_i[d] - mu_j[d])^2): observation outputs only
    const bool obs = on && sub >= 1;
    float best = 0.f;
    for (int i = 0; i + 1 < E; ++i) {
      const float mi = obs ? a.mean[at + i * es] : 0.f;
      for (int j = i + 1; j < E; ++j) {
        const float df = obs ? mi - a.mean[at + j * es] : 0.f;
        float q = df * df;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) q += __shfl_xor(q, o);   // the row's 32-lane group
        best = fmaxf(best, q);
      }
    }
    u = sqrtf(best);   // sqrt is monotone and correctly rounded: the max of the roots
  } else {
    // sqrt(sum_{d=0..O} (1/E) sum_e [sigma_e[d]^2 + (mu_e[d] - mubar[d])^2]): the mixture's total std in
    // the centred form (the uncentred one cancels catastrophically in f32)
    float sum = 0.f;
    if (on)
      for (int e = 0; e < E; ++e) sum += a.mean[at + e * es];
    const float avg = sum / (float)E;
    float acc = 0.f;
    if (on)
      for (int e = 0; e < E; ++e) {
        const float sp = a.spread[at + e * es];
        const float df = a.mean[at + e * es] - avg;
        acc += (a.spread_is_var ? sp : sp * sp) + df * df;
      }
    float q = acc / (float)E;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    u = sqrtf(q);
  }
  if (live && sub == 0) a.pen[row] = __float_as_uint(u);
}

int launch_ensemble_penalty(const PenaltyArgs& a, hipStream_t s) {
  MOPO_REQUIRE(a.kind == MOPO_PENALTY_MAX_PAIRWISE || a.kind == MOPO_PENALTY_ENSEMBLE_STD,
               "ensemble penalty: the kernel computes max_pairwise (2) and ensemble_std (3)");
  MOPO_REQUIRE(a.O + 1 <= 32 && a.E >= 1, "ensemble penalty: obs_dim must be < 32");
  MOPO_REQUIRE(a.mean && a.pen && (a.kind == MOPO_PENALTY_MAX_PAIRWISE || a.spread),
               "ensemble penalty: NULL argument");
  if (a.B <= 0) return 0;
  hipLaunchKernelGGL(ensemble_penalty_kernel, dim3((unsigned)((a.B + PEN_RPB - 1) / PEN_RPB)), dim3(256), 0, s, a);
  MOPO_HIP(hipGetLastError());
  return 0;
}

}  // namespace mopo

extern "C" int mopo_penalty_from_predictions(int kind, const float* d_mean, const float* d_var, int E, int obs_dim,
                                             int64_t B, float* d_penalty, void* stream) {
  using namespace mopo;
  MOPO_REQUIRE(kind == MOPO_PENALTY_MAX_PAIRWISE || kind == MOPO_PENALTY_ENSEMBLE_STD,
               std::string("mopo_penalty_from_predictions: max_pairwise (2) or ensemble_std (3) only") +
                   (kind >= 0 && kind < MOPO_PENALTY_KINDS ? "" : kPenaltyKindMsg));
  MOPO_REQUIRE(E >= 1 && obs_dim >= 1 && obs_dim + 1 <= 32 && B >= 0,
               "mopo_penalty_from_predictions: E >= 1, 1 <= obs_dim <= 31 and B >= 0 required");
  if (B == 0) return 0;
  MOPO_REQUIRE(d_mean && d_var && d_penalty, "mopo_penalty_from_predictions: NULL argument");
  PenaltyArgs pa{};
  pa.mean = d_mean; pa.spread = d_var; pa.stride = B; pa.spread_is_var = 1;
  pa.E = E; pa.O = obs_dim; pa.B = B; pa.kind = kind; pa.pen = reinterpret_cast<uint32_t*>(d_penalty);
  return launch_ensemble_penalty(pa, (hipStream_t)stream);
}

namespace mopo {

int rollout_penalty_alloc(Rollout* h) {
  const size_t bytes = (size_t)h->bnn->E * h->Bmax * (h->bnn->O + 1) * sizeof(float);
  if (!h->mean_all) MOPO_HIP(hipMalloc(&h->mean_all, bytes));
  if (!h->std_all) MOPO_HIP(hipMalloc(&h->std_all, bytes));
  return 0;
}

int rollout_penalty(Rollout* h, int kind, int64_t off, int64_t n, const int* cnt, hipStream_t s) {
  const int D = h->bnn->O + 1;
  PenaltyArgs pa{};
  pa.mean = h->mean_all + off * D; pa.spread = h->std_all + off * D; pa.stride = h->Bmax; pa.spread_is_var = 0;
  pa.E = h->bnn->E; pa.O = h->bnn->O; pa.B = n; pa.d_count = cnt; pa.kind = kind; pa.pen = h->pen + off;
  return launch_ensemble_penalty(pa, s);
}

}  // namespace mopo
