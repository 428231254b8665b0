// The penalty u(s, a) over a dataset: mopo_rollout_penalty_profile, the distribution a halt threshold is
// calibrated on (MOReL's threshold on the data's own disagreement).  No reference counterpart.
//
// Per chunk of the handle's max_batch rows, on one stream with no host synchronisation:
//   profile_gather          the ensemble's scaled input rows xs straight from the pool's f32 observations /
//                           actions (slot_feat order, 32 or 64 slots per row), u <- 0
//   bnn_fwd ROLLOUT         the ensemble, as in the training rollout (no member is selected); its max-aleatoric
//                           norm lands in u's own bits (kind 1)
//   ensemble_penalty        kinds 2 and 3 (penalty.hip), from every member's mean / std
//   profile_mean_distance   kind 0, from every member's mean and the row's obs (penalty.h: the post step's order)
// No policy runs, nothing is drawn or sampled, the pool is only read.
#include "mlp_tile.h"
#include "penalty.h"
#include "rollout.h"

namespace mopo {

// One thread per quad of slots, QPR = stride / 4 threads per row: xs[row][slot] = (concat(obs, act)[k] - mu[k]) /
// sigma[k], k = slot_feat(slot, O + A), as actor_finish / rollout_xs_wide_kernel compute it from the f64 state of a
// rollout whose rows start at these f32 values.  The row's quad 0 also zeroes its u (the ensemble's atomicMax).
__global__ __launch_bounds__(256) void profile_gather_kernel(const float* __restrict__ obs,
                                                             const float* __restrict__ act, int O, int A,
                                                             const float* __restrict__ mu,
                                                             const float* __restrict__ sigma, int64_t n, int stride,
                                                             float* __restrict__ xs, uint32_t* __restrict__ u) {
  const int qpr = stride >> 2;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t row = i / qpr;
  if (row >= n) return;
  const int q = (int)(i - row * qpr);
  f32x4 v;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = slot_feat(4 * q + t, O + A);
    float x = 0.f;
    if (k >= 0) {
      const float raw = k < O ? obs[row * O + k] : act[row * A + (k - O)];
      x = (raw - mu[k]) / sigma[k];
    }
    v[t] = x;
  }
  *reinterpret_cast<f32x4*>(xs + row * stride + 4 * q) = v;
  if (q == 0) u[row] = 0u;
}

// Kind 0 for PROF_RPB rows per block, one 32-lane group per row and one lane per output dim, as
// rollout_post_kernel lays rows out; member_mean is post_group_step's: the f32 residual add of the row's obs.
constexpr int PROF_RPB = 8;
__global__ __launch_bounds__(256) void profile_mean_distance_kernel(const float* __restrict__ mean_all,
                                                                    int64_t all_stride, int E, int O,
                                                                    const float* __restrict__ obs, int64_t n,
                                                                    float* __restrict__ u) {
  const int tid = threadIdx.x, sub = tid & 31, rl = tid >> 5;
  const int64_t row = (int64_t)blockIdx.x * PROF_RPB + rl;
  const int D = O + 1;
  const bool on = row < n && sub < D;
  const double ob = on && sub >= 1 ? (double)obs[row * O + sub - 1] : 0.0;
  auto member_mean = [&](int e) {
    const float m = mean_all[((int64_t)e * all_stride + row) * D + sub];
    return sub >= 1 ? (float)((double)m + ob) : m;
  };
  const float pen = mean_distance_penalty(member_mean, E, on && sub >= 1);
  if (row < n && sub == 0) u[row] = pen;
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_rollout_penalty_profile(mopo_rollout_t hh, const mopo_pool_desc* pool, int64_t n_rows, int kind,
                                            float* d_u, void* stream) {
  Rollout* h = reinterpret_cast<Rollout*>(hh);
  MOPO_REQUIRE(h && pool, "mopo_rollout_penalty_profile: NULL argument");
  MOPO_REQUIRE(kind >= 0 && kind < MOPO_PENALTY_KINDS, std::string("mopo_rollout_penalty_profile") + kPenaltyKindMsg);
  MOPO_REQUIRE(n_rows >= 0, "mopo_rollout_penalty_profile: n_rows must be >= 0");
  if (n_rows == 0) return 0;
  MOPO_REQUIRE(pool->d_obs && pool->d_act, "mopo_rollout_penalty_profile: NULL pool field (observations, actions)");
  MOPO_REQUIRE(d_u, "mopo_rollout_penalty_profile: NULL d_u");
  MOPO_REQUIRE(n_rows <= pool->max_size, "mopo_rollout_penalty_profile: n_rows exceeds the pool's max_size");
  hipStream_t s = (hipStream_t)stream;
  Bnn* bnn = h->bnn;
  const int O = bnn->O, A = bnn->A, D = O + 1;
  const int stride = xs_stride(bnn->dev.KG0);
  const bool need_mean = kind != MOPO_PENALTY_MAX_ALEATORIC, need_std = kind >= MOPO_PENALTY_MAX_PAIRWISE;
  if (need_std) {
    if (rollout_penalty_alloc(h)) return -1;
  } else if (need_mean && !h->mean_all) {
    MOPO_HIP(hipMalloc(&h->mean_all, (size_t)bnn->E * h->Bmax * D * sizeof(float)));
  }
  h->next_step = 0;   // the handle's step buffers are reused: a staged step range must not continue across this
  for (int64_t j0 = 0; j0 < n_rows; j0 += h->Bmax) {
    const int64_t n = std::min<int64_t>(h->Bmax, n_rows - j0);
    const float* obs = pool->d_obs + j0 * O;
    const float* act = pool->d_act + j0 * A;
    uint32_t* ubits = reinterpret_cast<uint32_t*>(d_u + j0);
    const int64_t quads = n * (stride >> 2);
    hipLaunchKernelGGL(profile_gather_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, obs, act, O, A,
                       bnn->dev.mu, bnn->dev.sigma, n, stride, h->xs, ubits);
    MOPO_HIP(hipGetLastError());
    FwdArgs f{};
    f.in = FwdIn{obs, 0, O, act, 0, A};
    f.B = n; f.xs = h->xs;
    f.pen_bits = ubits; f.sel = nullptr; f.mean_sel = h->mean_sel; f.std_sel = h->std_sel;
    f.mean_all = need_mean ? h->mean_all : nullptr;
    f.std_all = need_std ? h->std_all : nullptr;
    f.all_stride = h->Bmax;
    if (launch_bnn_fwd(bnn, FWD_ROLLOUT, f, s)) return -1;
    if (need_std) {
      PenaltyArgs pa{};
      pa.mean = h->mean_all; pa.spread = h->std_all; pa.stride = h->Bmax; pa.spread_is_var = 0;
      pa.E = bnn->E; pa.O = O; pa.B = n; pa.kind = kind; pa.pen = ubits;
      if (launch_ensemble_penalty(pa, s)) return -1;
    } else if (need_mean) {
      hipLaunchKernelGGL(profile_mean_distance_kernel, dim3(ceil_div((int)n, PROF_RPB)), dim3(256), 0, s,
                         h->mean_all, h->Bmax, bnn->E, O, obs, n, d_u + j0);
      MOPO_HIP(hipGetLastError());
    }
  }
  return 0;
}
