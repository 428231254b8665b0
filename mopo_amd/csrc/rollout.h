// The rollout handle and what the three device loops over the model share on the host: the training rollout
// (rollout.hip), the model-based policy evaluation (rollout_eval.hip) and the open-loop validation on dataset
// trajectories (rollout_val.hip).  One statement of a step's setup (argument checks, FakeEnv modes, the actor
// pack, the ensemble's and the post kernel's arguments, the wide-input / compaction launches, the live-count
// read-back), defined in rollout.hip; the device side of the step itself is rollout_post.h.
#pragma once
#include "actor.h"

#include <utility>
#include <vector>

namespace mopo {

struct Rollout {
  // optional live kernel timing: hipEvents recorded around every launch, per kernel class
  bool profile = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev;
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
  int32_t* ev_len; uint8_t* ev_term; float* ev_eps0; double* ev_stats; uint8_t* ev_halt;
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
  // hard truncation (mopo_hip.h "Hard truncation"): halt 1 -> a row with !(penalty <= halt_threshold) is terminal
  // with the reward halt_reward; halted_cnt: this step's count of such rows (one atomic per block), or NULL
  int halt;
  float halt_threshold, halt_reward;
  unsigned long long* halted_cnt;
};

// FakeEnv's modes for one call: deterministic steps, the mean-distance penalty (computed by the post kernel),
// a penalty kind >= 2 (penalty.hip, 0: none), and whether any of them needs every member's mean per row
struct StepModes {
  bool det, pen_dist;
  int pen_kind;
  bool need_all;
};

// The checks every entry point `who` makes on its arguments: B, term_kind, the penalty kind, the elites (an
// entry point that runs no policy needs none for deterministic steps) and, with a policy, actor_dtype.
int rollout_check_args(const Rollout* h, const mopo_rollout_args* a, const char* who, bool policy);
// The modes of `a` (always_pen: the penalty is computed whatever the coefficient, as it is with a->halt = 1);
// allocates mean_all / std_all on first use.
int rollout_modes(Rollout* h, const mopo_rollout_args* a, bool always_pen, StepModes* m);
// The start states (rollout_start_kernel): a's B rows gathered from env_obs rows idx (NULL: drawn over
// [0, env_size)) into obs[0], their ids into uid[0], the live counts of the nsplit parts of bpart rows.
int rollout_start(Rollout* h, const mopo_rollout_args* a, const float* env_obs, int64_t env_size, const int64_t* idx,
                  int nsplit, int64_t bpart, hipStream_t s);
// (Re)allocates the handle's fragment-major policy weights for a's width and dtype and packs them on s.
int rollout_pack_actor(Rollout* h, const mopo_rollout_args* a, hipStream_t s);
// Horizon step i for rows [off, off + n) of a's batch, live count *cnt, reading obs[oc] / uid[uc]: the fields
// of the actor's, the ensemble's and the post kernel's arguments that the loops share (no pool, one stream).
ActorArgs rollout_actor_args(const Rollout* h, const mopo_rollout_args* a, const StepModes& m, int i, int oc, int uc,
                             int64_t off, int64_t n, int* cnt);
FwdArgs rollout_fwd_args(const Rollout* h, const StepModes& m, int oc, int64_t off, int64_t n, int* cnt, float* xs);
PostArgs rollout_post_args(const Rollout* h, const mopo_rollout_args* a, const StepModes& m, int i, int oc, int uc,
                           int64_t off, int* cnt, bool compact);
// A wide model's scaled input rows (rollout_xs_wide_kernel) behind whatever wrote act.
int rollout_xs_wide(const Rollout* h, int oc, int64_t off, int64_t n, const int* cnt, float* xs, hipStream_t s);
// Compaction of B launch rows: the chunk counts zeroed before the post kernel, and behind it
// rollout_compact_kernel from obs[oc ^ 1] / uid[uc] into obs[oc] / uid[uc ^ 1], survivors to cnt[1].
int rollout_zero_chunks(Rollout* h, int64_t B, hipStream_t s);
int rollout_compact(Rollout* h, int64_t B, int oc, int uc, hipStream_t s);
// MOPO_EVAL_POLL=<steps between two read-backs of the live count> (0: never read it back); default 32.
// Read at every call (tests compare settings in one process); the results do not depend on it.
int rollout_poll_steps();
// Reads the live count back (synchronises s); *none: no row is alive, the remaining steps would all return on
// the zero count.
int rollout_none_alive(Rollout* h, hipStream_t s, bool* none);

// Carves one allocation into n arrays of sz[i] bytes at 256-byte-aligned offsets off[i] (an array with
// given[i] set takes no room); returns the allocation's size.
inline size_t carve(const size_t* sz, int n, size_t* off, void* const* given = nullptr) {
  size_t tot = 0;
  for (int i = 0; i < n; ++i) {
    off[i] = tot;
    if (!given || !given[i]) tot += (sz[i] + 255) & ~(size_t)255;
  }
  return tot;
}

// defined in rollout_eval.hip
__global__ void rollout_eval_advance_kernel(int* cnt, int64_t* steps, int i);

}  // namespace mopo
