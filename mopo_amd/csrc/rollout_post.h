// The device FakeEnv step (fake_env.py:66-115), stated once for the training rollout (rollout.hip), the policy
// evaluation (rollout_eval.hip) and the open-loop validation (rollout_val.hip): the observation noise, the
// 32-lane-group step (f32 residual add, mean-distance penalty, deterministic mean or f64 sample, the row's LDS
// slice), the row's verdict (termination, penalty, penalized reward) and the kept-rows count of a block.  Each
// kernel keeps its own epilogue: pool half-rows, episode accumulators, error tables.
#pragma once
#include "penalty.h"
#include "rollout.h"

namespace mopo {

constexpr int POST_RPB = 8;   // rows per block of the group kernels; PB % POST_RPB == 0: they share one chunk

// The standard normal of output dim `sub` of a row: injected, or (perf mode of fake_env.py:72) Philox block
// sub / 4 of the row's RNG_OBS_NOISE stream, Box-Muller pair (sub % 4) / 2 -- the numbers a per-row order gives.
__device__ __forceinline__ double post_obs_noise(const PostArgs& a, int64_t row, int D, int sub) {
  if (a.eps) return a.eps[row * D + sub];
  const int64_t u = a.uid[row];
  u32x4 c{(uint32_t)u, (uint32_t)((uint64_t)u >> 32) ^ ((uint32_t)(sub >> 2) << 20), a.step, RNG_OBS_NOISE};
  u32x4 r = philox(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  float z0, z1;
  if (sub & 2) box_muller(r.z, r.w, z0, z1);
  else box_muller(r.x, r.y, z0, z1);
  return (double)((sub & 1) ? z1 : z0);
}

// The sampled value of (row, sub) in f64 (fake_env.py:72): m, the selected member's mean after the f32 residual
// add (:66), plus the noise times the member's std.
__device__ __forceinline__ double post_sample(const PostArgs& a, int64_t row, int D, int sub, float m) {
  const double e = post_obs_noise(a, row, D, sub);
  return (double)m + e * (double)a.std_sel[row * D + sub];
}

// One row's step by its 32-lane group, one lane per output dim sub < D = O + 1 (`on`: a live row's lane below
// D): every load of the row's D values is contiguous across its lanes.  Returns the lane's sample s, also stored
// into the row's LDS slice, and the row's mean-distance penalty in pen_d (pen_dist only).  The caller's
// __syncthreads() comes next.
__device__ __forceinline__ double post_group_step(const PostArgs& a, int64_t row, int sub, bool on, double* lds_row,
                                                  float& pen_d) {
  const int O = a.O, D = O + 1;
  double s = 0.0;
  // member e's mean of this lane's dim after the residual add, in f32 as the reference's in-place
  // ensemble_model_means[:, :, 1:] += obs (fake_env.py:66)
  const double ob = on && sub >= 1 ? a.obs[row * O + sub - 1] : 0.0;
  auto member_mean = [&](int e) {
    const float m = a.mean_all[((int64_t)e * a.all_stride + row) * D + sub];
    return sub >= 1 ? (float)((double)m + ob) : m;
  };
  // max_e || mean_e - mean_e' mean_e' || over the obs dims (fake_env.py:98-108; penalty.h)
  pen_d = a.pen_dist ? mean_distance_penalty(member_mean, a.E, on && sub >= 1) : 0.f;
  if (on && a.det) {  // samples = mean over ALL members of the means (fake_env.py:69-70, 84-86)
    float acc = 0.f;
    for (int e = 0; e < a.E; ++e) acc += member_mean(e);
    s = (double)(acc / (float)a.E);
    lds_row[sub] = s;
  } else if (on) {
    float m = a.mean_sel[row * D + sub];
    if (sub >= 1) m = (float)((double)m + ob);                      // fake_env.py:66
    s = post_sample(a, row, D, sub, m);
    lds_row[sub] = s;
  }
  return s;
}

// What lane 0 of a live row concludes from the row's LDS slice (after the barrier) and its own s = samples[:, 0]
struct PostVerdict {
  bool term;    // fake_env.py:91, or halted
  bool rule;    // fake_env.py:91 alone: the termination rule's verdict
  bool halted;  // hard truncation: !(pen <= halt_threshold)
  float pen;    // the penalty of the selected kind
  double pr;    // rewards = samples[:, :1] - coeff * penalty (fake_env.py:115); a halted row's: halt_reward
};
// The row's verdict from the rule's (`rule`), its penalty and its sampled reward s: THE statement of the
// penalized reward and of hard truncation (mopo_hip.h "Hard truncation") for the fused loops
__device__ __forceinline__ PostVerdict post_conclude(const PostArgs& a, bool rule, float pen, double s) {
  PostVerdict v;
  v.rule = rule;
  v.pen = pen;
  v.halted = a.halt && !(pen <= a.halt_threshold);               // u > threshold, or u is NaN
  v.term = rule || v.halted;
  v.pr = v.halted ? (double)a.halt_reward : (a.coeff != 0.f ? s - (double)a.coeff * (double)pen : s);
  return v;
}
__device__ __forceinline__ PostVerdict post_verdict(const PostArgs& a, int64_t row, const double* lds_row, double s,
                                                    float pen_d) {
  return post_conclude(a, term_fn(a.term_kind, lds_row + 1, a.O), a.pen_dist ? pen_d : __uint_as_float(a.pen[row]),
                       s);
}
// a row's entry of a block's `kept` array: bit 0 the row goes on, bit 1 it was halted (0: not a live row)
__device__ __forceinline__ int post_kept_word(const PostVerdict& v) { return (v.term ? 0 : 1) | (v.halted ? 2 : 0); }

// The kept rows of a block of ROWS rows from r0 on (PB % ROWS == 0), counted into the block's PB-row chunk of
// blockcnt (with compaction; zeroed before the launch), and its halted rows into *halted_cnt: at most one atomic
// each per block.  Either pointer may be NULL.
template <int ROWS>
__device__ __forceinline__ void post_count_kept(const int* kept, int* blockcnt, unsigned long long* halted_cnt,
                                                int64_t r0) {
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0, hl = 0;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) { t += kept[i] & 1; hl += kept[i] >> 1; }
    if (blockcnt && t) atomicAdd(blockcnt + r0 / PB, t);
    if (halted_cnt && hl) atomicAdd(halted_cnt, (unsigned long long)hl);
  }
}

}  // namespace mopo
