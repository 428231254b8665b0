// The model-disagreement reward penalties beyond the reference's two (penalty.hip): one kernel between the
// ensemble forward and the FakeEnv post step, launched by the fused rollout, the model-based evaluation, the
// open-loop validation (every member's head mean / std, FwdArgs::mean_all / std_all) and by
// mopo_fakeenv_step (the predict layout, mean / var).
#pragma once
#include "common.h"

namespace mopo {

struct PenaltyArgs {
  const float* mean;      // [E][stride][D] member head means BEFORE the residual add
  const float* spread;    // [E][stride][D] member stds, or variances when spread_is_var (unused by max_pairwise)
  int64_t stride;         // rows between two members
  int spread_is_var;
  int E, O;
  int64_t B;              // launch rows (the grid is sized for this)
  const int* d_count;     // optional device live-row count (<= B), as the post kernels read *cnt
  int kind;               // MOPO_PENALTY_MAX_PAIRWISE or MOPO_PENALTY_ENSEMBLE_STD
  uint32_t* pen;          // [B] the penalty's f32 bits (>= 0)
};

int launch_ensemble_penalty(const PenaltyArgs& a, hipStream_t s);

// the refusal every entry point that reads a penalty kind gives for a value outside [0, MOPO_PENALTY_KINDS)
extern const char* const kPenaltyKindMsg;

// The hard-truncation fields (mopo_hip.h "Hard truncation") of an entry point `who` that reads them -- every one
// but the validation: halt 0 or 1 and, with halt = 1, a finite halt_reward and a halt_threshold that is not NaN.
int check_halt(int halt, float halt_threshold, float halt_reward, const char* who);

// The mean-distance penalty (kind 0) of one row by its 32-lane group, lane sub < D = O + 1 (`obs`: a live row's
// lane of an observation output, sub >= 1): max_e || mean_e - mean over members || over the obs dims
// (fake_env.py:98-108) in f32, member_mean(e) the lane's mean of member e after the residual add.  Sums over
// members in member order, over dims by a fixed __shfl_xor tree: the same bits wherever it is called from (the
// post step of the fused loops, rollout_post.h; the dataset pass, penalty_profile.hip).
template <class F>
__device__ __forceinline__ float mean_distance_penalty(const F& member_mean, int E, bool obs) {
  float sum = 0.f;
  if (obs)
    for (int e = 0; e < E; ++e) sum += member_mean(e);
  const float avg = sum / (float)E;                             // np.mean(axis=0), f32
  float pen = 0.f;
  for (int e = 0; e < E; ++e) {
    const float dd = obs ? member_mean(e) - avg : 0.f;
    float q = dd * dd;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) q += __shfl_xor(q, o);     // the row's 32-lane group
    pen = fmaxf(pen, sqrtf(q));
  }
  return pen;
}

}  // namespace mopo
