// The rollout handle and the pieces of rollout.hip that rollout_eval.hip (model-based policy evaluation) and
// rollout_val.hip (open-loop validation on dataset trajectories) launch as they are: the start-state gather,
// the wide models' scaled input rows and the compaction.
#pragma once
#include "actor.h"

#include <utility>
#include <vector>

namespace mopo {

struct Rollout {
  // optional live kernel timing: hipEvents recorded around every launch, per kernel class
  bool profile = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev;
  std::vector<hipEvent_t> pool_ev;
  size_t ev_used = 0;
  Bnn* bnn = nullptr;
  int64_t Bmax = 0;
  int Hmax = 0;
  void* mem = nullptr;
  double* obs[2];
  int64_t* uid[2];
  float* act;
  float* wpk = nullptr;  // policy weights, fragment-major (pack_actor), repacked every run
  int wpk_hp = 0, wpk_f16 = 0;
  uint32_t* pen;
  int32_t* sel;
  float* xs;        // [B][32] the ensemble's scaled input rows (written by the actor); wide models [B][64]
  float* mean_sel;
  float* std_sel;
  float* mean_all = nullptr;  // [E][Bmax][D], allocated on first use (mean-distance penalty / deterministic)
  uint8_t* keep;
  int* blockcnt;
  int* cnt;  // [0] live rows this step, [1] survivors, [2 + k] rows of part k (split rollout)
  static constexpr int MAXSPLIT = 4;
  hipStream_t sp[MAXSPLIT] = {};        // streams of parts 1.. of the split rollout (run_impl)
  hipEvent_t ev_fork[MAXSPLIT] = {}, ev_join[MAXSPLIT] = {};
  // horizon state carried between step-range calls (mopo_rollout_run_staged_steps)
  int oc = 0, uc = 0, next_step = 0;
  // policy evaluation (rollout_eval.hip), allocated on first use: per-episode accumulators of Bmax
  // episodes, the zero policy noise [Bmax][A] of the deterministic policy, the statistics
  void* eval_mem = nullptr;
  double* ev_ret; double* ev_pen_ret; double* ev_pen_sum;
  int32_t* ev_len; uint8_t* ev_term; float* ev_eps0; double* ev_stats;
  // open-loop validation (rollout_val.hip), allocated on first use: the segments' start rows [Bmax] (as
  // drawn, and clamped into the pool for the start gather), and the [K][B] tables / statistics a caller
  // left NULL (val_tab, grown to the largest K * B asked for)
  void* val_mem = nullptr;
  int64_t* val_start; int64_t* val_gidx;
  void* val_tab = nullptr;
  size_t val_tab_bytes = 0;
  // every member's std beside mean_all, same size, allocated on first use (penalty kinds >= 2, penalty.hip)
  float* std_all = nullptr;
};

// Penalty kinds >= 2 (penalty.hip): allocates mean_all / std_all on first use.  Then, per step, the caller
// sets FwdArgs::mean_all / std_all, launches the ensemble, rollout_penalty on the same stream (rows at element
// offset `off` of the handle's buffers, live count *cnt) and the post kernel with pen_dist = 0.
int rollout_penalty_alloc(Rollout* h);
int rollout_penalty(Rollout* h, int kind, int64_t off, int64_t n, const int* cnt, hipStream_t s);

constexpr int PB = 256;  // rows per block in post / compact

struct PostArgs {
  int O;
  const int* cnt;
  const double* obs;        // current obs f64 [B][O]
  const int64_t* uid;
  const float* mean_sel;    // [B][D]
  const float* std_sel;
  const uint32_t* pen;
  const double* eps;        // injected [B][D] or NULL
  uint64_t seed; uint32_t step;
  float coeff;
  int term_kind;
  double* obs_next;         // [B][O]
  uint8_t* keep;
  int* blockcnt;
  mopo_pool_desc pool;
  int64_t stage_base;       // >= 0: staged layout
  int64_t pool_off;         // pool layout: rows go to (state[0] + pool_off + row) % max_size
  // every member's mean [E][all_stride][D] (the ensemble's mean_all), for the mean-distance penalty
  // (pen_dist, fake_env.py:98-108) and deterministic steps (det, fake_env.py:69-70, 84-86)
  const float* mean_all;
  int E;
  int64_t all_stride;
  int pen_dist, det;
};

// defined in rollout.hip
constexpr int START_ROWS = 64, START_TPB = 256;
__global__ void rollout_start_kernel(const float* env_obs, int64_t env_size, const int64_t* idx_in, int O, int64_t B,
                                     uint64_t seed, uint32_t step, int64_t uid_offset, double* obs, int64_t* uid,
                                     int* cnt, int nsplit, int64_t bpart);
__global__ void rollout_xs_wide_kernel(const double* __restrict__ obs, const float* __restrict__ act, int O, int A,
                                       const float* __restrict__ mu, const float* __restrict__ sigma, int64_t B,
                                       const int* __restrict__ d_count, float* __restrict__ xs);
__global__ void rollout_compact_kernel(int O, const int* blockcnt, const uint8_t* keepf, const int* cnt,
                                       const double* obs_src, double* obs_dst, const int64_t* uid_src,
                                       int64_t* uid_dst, int* survivors);
// defined in rollout_eval.hip
__global__ void rollout_eval_advance_kernel(int* cnt, int64_t* steps, int i);

}  // namespace mopo
