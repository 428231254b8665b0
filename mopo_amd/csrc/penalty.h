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

}  // namespace mopo
