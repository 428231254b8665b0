// Model-based policy evaluation: B episodes of up to T steps of the policy inside the learned model
// (RLAlgorithm._evaluation_paths / _evaluate_rollouts, rl_algorithm.py:258-304, with FakeEnv.step as the
// environment), on the device.
//
// Per step, on one stream:
//   actor_kernel             the policy (rollout.hip's launch; no pool: it writes act, the member pick, xs)
//   bnn_fwd ROLLOUT          the ensemble, as in the training rollout
//   rollout_eval_post        FakeEnv's sample / penalty / termination (rollout_post.h); instead of a pool
//                            row it adds the step's rewards to the row's episode (uid - uid_offset)
//   rollout_compact          obs = next_obs[~term] (skipped for the never-done domains)
//   rollout_eval_advance     live count <- survivors, steps[i] (with compaction only)
// then rollout_eval_stats reduces the per-episode sums to evaluate_rollouts' statistics.
#include "penalty.h"
#include "rollout_post.h"

namespace mopo {

struct EvalPostArgs {
  PostArgs p;               // pool / stage_base / pool_off unused
  int64_t uid_offset;
  double* ret;              // [B] += samples[:, 0]
  double* pen_ret;          // [B] += the penalized reward (fake_env.py:115)
  double* pen_sum;          // [B] += the penalty
  int32_t* len;             // [B] += 1
  uint8_t* terminated;      // [B] = 1 on termination by the rule
  uint8_t* halted;          // [B] = 1 on a halt
};

__global__ void rollout_eval_init_kernel(int64_t B, double* ret, double* pen_ret, double* pen_sum, int32_t* len,
                                         uint8_t* terminated, uint8_t* halted) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= B) return;
  ret[i] = 0.0; pen_ret[i] = 0.0; pen_sum[i] = 0.0; len[i] = 0; terminated[i] = 0; halted[i] = 0;
}

// One FakeEnv step (rollout_post.h) for POST_RPB rows per block, a 32-lane group per row.  Its own part: a live
// row is the only row of its episode, so the episode's accumulators take plain read-modify-writes.
__global__ __launch_bounds__(256) void rollout_eval_post_kernel(const EvalPostArgs ea) {
  const PostArgs& a = ea.p;
  __shared__ double srow[POST_RPB][33];
  __shared__ int kept[POST_RPB];
  const int tid = threadIdx.x, sub = tid & 31, rl = tid >> 5;
  const int64_t row = (int64_t)blockIdx.x * POST_RPB + rl;
  const int O = a.O, D = O + 1;
  const int64_t count = *a.cnt;
  const bool live = row < count;
  const bool on = live && sub < D;
  float pen_d;
  const double s = post_group_step(a, row, sub, on, srow[rl], pen_d);
  __syncthreads();
  if (on && sub >= 1) a.obs_next[row * O + sub - 1] = s;           // next_obs = samples[:, 1:] (:90)
  if (sub == 0) {
    int keep = 0;
    if (live) {
      const PostVerdict v = post_verdict(a, row, srow[rl], s, pen_d);
      const int64_t ep = a.uid[row] - ea.uid_offset;               // in [0, B): the start kernel's ids
      ea.ret[ep] += s;                                             // unpenalized_rewards (fake_env.py:89, 127)
      ea.pen_ret[ep] += v.pr;
      ea.pen_sum[ep] += (double)v.pen;
      ea.len[ep] += 1;
      if (v.rule) ea.terminated[ep] = 1;
      if (v.halted) ea.halted[ep] = 1;
      keep = post_kept_word(v);
      if (a.keep) a.keep[row] = keep & 1;
    }
    kept[rl] = keep;
  }
  if (a.blockcnt) post_count_kept<POST_RPB>(kept, a.blockcnt, nullptr, (int64_t)blockIdx.x * POST_RPB);
}

__global__ void rollout_eval_advance_kernel(int* cnt, int64_t* steps, int i) {
  if (steps) steps[i] = cnt[0];
  cnt[0] = cnt[1];
}

// never-done domains: every step kept all cnt[0] rows
__global__ void rollout_eval_steps_kernel(const int* cnt, int64_t* steps, int T) {
  for (int i = threadIdx.x; i < T; i += blockDim.x) steps[i] = cnt[0];
}

// evaluate_rollouts' statistics (rl_algorithm.py:281-304) by one workgroup: thread t folds episodes t,
// t + 256, ... in that order, then a fixed binary tree over the 256 partials -- the same bits every run.
// The standard deviations take a second pass around the mean (np.std: population).
constexpr int ST = 256;
enum { SQ_RET = 0, SQ_LEN, SQ_PRET, SQ_PEN, SQ_TERM, SQ_HALT, SQ_RMIN, SQ_LMIN, SQ_RMAX, SQ_LMAX, SQ_N };
__global__ __launch_bounds__(ST) void rollout_eval_stats_kernel(const double* ret, const double* pen_ret,
                                                                const double* pen_sum, const int32_t* len,
                                                                const uint8_t* terminated, const uint8_t* halted,
                                                                int64_t B, double* stats) {
  __shared__ double red[SQ_N][ST];
  const int tid = threadIdx.x;
  auto tree = [&](int nq) {   // quantities [0, SQ_RMIN) sum, [SQ_RMIN, SQ_RMAX) min, the rest max
    __syncthreads();
    for (int st = ST / 2; st > 0; st >>= 1) {
      if (tid < st)
        for (int q = 0; q < nq; ++q) {
          const double x = red[q][tid], y = red[q][tid + st];
          red[q][tid] = q < SQ_RMIN ? x + y : (q < SQ_RMAX ? fmin(x, y) : fmax(x, y));
        }
      __syncthreads();
    }
  };
  double v[SQ_N];
  for (int q = 0; q < SQ_N; ++q) v[q] = q < SQ_RMIN ? 0.0 : (q < SQ_RMAX ? INFINITY : -INFINITY);
  for (int64_t i = tid; i < B; i += ST) {
    const double r = ret[i], l = (double)len[i];
    v[SQ_RET] += r; v[SQ_LEN] += l; v[SQ_PRET] += pen_ret[i]; v[SQ_PEN] += pen_sum[i];
    v[SQ_TERM] += (double)terminated[i]; v[SQ_HALT] += (double)halted[i];
    v[SQ_RMIN] = fmin(v[SQ_RMIN], r); v[SQ_LMIN] = fmin(v[SQ_LMIN], l);
    v[SQ_RMAX] = fmax(v[SQ_RMAX], r); v[SQ_LMAX] = fmax(v[SQ_LMAX], l);
  }
  for (int q = 0; q < SQ_N; ++q) red[q][tid] = v[q];
  tree(SQ_N);
  const double n = (double)B;
  const double rmean = red[SQ_RET][0] / n, lsum = red[SQ_LEN][0], lmean = lsum / n;
  if (tid == 0) {
    stats[0] = rmean; stats[1] = red[SQ_RMIN][0]; stats[2] = red[SQ_RMAX][0];
    stats[4] = lmean; stats[5] = red[SQ_LMIN][0]; stats[6] = red[SQ_LMAX][0];
    stats[8] = red[SQ_PRET][0] / n;
    stats[9] = red[SQ_PEN][0] / lsum;
    stats[10] = red[SQ_TERM][0] / n;
    stats[11] = n;
    stats[12] = red[SQ_HALT][0] / n;
    stats[13] = stats[14] = stats[15] = 0.0;
  }
  __syncthreads();   // red is read above by every thread before the second pass overwrites it
  double dr = 0.0, dl = 0.0;
  for (int64_t i = tid; i < B; i += ST) {
    const double a = ret[i] - rmean, b = (double)len[i] - lmean;
    dr += a * a; dl += b * b;
  }
  red[0][tid] = dr; red[1][tid] = dl;
  tree(2);
  if (tid == 0) {
    stats[3] = sqrt(red[0][0] / n);
    stats[7] = sqrt(red[1][0] / n);
  }
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_rollout_evaluate(mopo_rollout_t hh, const mopo_rollout_args* a, const mopo_eval_args* e,
                                     void* stream) {
  Rollout* h = reinterpret_cast<Rollout*>(hh);
  MOPO_REQUIRE(h && a && e, "mopo_rollout_evaluate: NULL argument");
  if (rollout_check_args(h, a, "mopo_rollout_evaluate", true) ||
      check_halt(a->halt, a->halt_threshold, a->halt_reward, "mopo_rollout_evaluate"))
    return -1;
  MOPO_REQUIRE(a->horizon >= 1 && a->horizon <= 4095,
               "mopo_rollout_evaluate: the episode length T must be in [1, 4095] (the Philox step key is "
               "epoch * 4096 + 1 + step)");
  MOPO_REQUIRE(!(e->policy_deterministic && a->rollout_random),
               "mopo_rollout_evaluate: policy_deterministic with rollout_random (uniform actions have no mean)");
  MOPO_REQUIRE(a->d_env_obs && a->env_size > 0, "mopo_rollout_evaluate: empty env pool");
  MOPO_REQUIRE(a->d_pi_params, "mopo_rollout_evaluate: NULL policy params");
  MOPO_REQUIRE(!a->rollout_random || a->d_act_uniform || !a->d_eps_act,
               "mopo_rollout_evaluate: parity mode with rollout_random needs the injected uniforms (d_act_uniform)");
  if (a->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Bnn* bnn = h->bnn;
  const int A = bnn->A, T = a->horizon;
  const int64_t B = a->B;
  const bool compact = a->term_kind != MOPO_TERM_HALFCHEETAH || a->halt == 1;   // a halt ends episodes anywhere

  if (!h->eval_mem) {
    const size_t n = (size_t)h->Bmax;
    size_t sz[] = {n * 8, n * 8, n * 8, n * 4, n, n * A * 4, 16 * 8, n};
    size_t off[8];
    MOPO_HIP(hipMalloc(&h->eval_mem, carve(sz, 8, off)));
    char* m = (char*)h->eval_mem;
    h->ev_ret = (double*)(m + off[0]); h->ev_pen_ret = (double*)(m + off[1]); h->ev_pen_sum = (double*)(m + off[2]);
    h->ev_len = (int32_t*)(m + off[3]); h->ev_term = (uint8_t*)(m + off[4]); h->ev_eps0 = (float*)(m + off[5]);
    h->ev_stats = (double*)(m + off[6]); h->ev_halt = (uint8_t*)(m + off[7]);
  }
  double* ret = e->d_return ? e->d_return : h->ev_ret;
  double* pen_ret = e->d_pen_return ? e->d_pen_return : h->ev_pen_ret;
  double* pen_sum = e->d_pen_sum ? e->d_pen_sum : h->ev_pen_sum;
  int32_t* len = e->d_length ? e->d_length : h->ev_len;
  uint8_t* terminated = e->d_terminated ? e->d_terminated : h->ev_term;
  uint8_t* halted = e->d_halted ? e->d_halted : h->ev_halt;
  double* stats = e->d_stats ? e->d_stats : h->ev_stats;

  StepModes m;
  if (rollout_modes(h, a, false, &m)) return -1;

  h->next_step = 0;   // a staged step range must not continue across an evaluation
  hipLaunchKernelGGL(rollout_eval_init_kernel, dim3(ceil_div((int)B, 256)), dim3(256), 0, s, B, ret, pen_ret,
                     pen_sum, len, terminated, halted);
  MOPO_HIP(hipGetLastError());
  if (a->d_steps) MOPO_HIP(hipMemsetAsync(a->d_steps, 0, (size_t)T * sizeof(int64_t), s));
  // the deterministic policy: pi = mu + std * 0 through the sampled path, actor_finish untouched
  if (e->policy_deterministic) MOPO_HIP(hipMemsetAsync(h->ev_eps0, 0, (size_t)B * A * sizeof(float), s));
  if (rollout_start(h, a, a->d_env_obs, a->env_size, a->d_start_idx, 1, B, s)) return -1;
  if (rollout_pack_actor(h, a, s)) return -1;

  const bool wide = bnn->dev.KG0 > 2;   // internal.h bnn_wide: 64-slot xs rows, written behind the actor
  int oc = 0, uc = 0;
  const int poll = rollout_poll_steps();
  for (int i = 0; i < T; ++i) {
    ActorArgs aa = rollout_actor_args(h, a, m, i, oc, uc, 0, B, h->cnt);
    if (e->policy_deterministic) aa.eps = h->ev_eps0;
    if (launch_actor(aa, s)) return -1;
    if (wide && rollout_xs_wide(h, oc, 0, B, h->cnt, h->xs, s)) return -1;

    const FwdArgs f = rollout_fwd_args(h, m, oc, 0, B, h->cnt, h->xs);
    if (launch_bnn_fwd(bnn, FWD_ROLLOUT, f, s)) return -1;
    if (m.pen_kind && rollout_penalty(h, m.pen_kind, 0, B, h->cnt, s)) return -1;

    EvalPostArgs ea{};
    ea.p = rollout_post_args(h, a, m, i, oc, uc, 0, h->cnt, compact);
    ea.uid_offset = a->uid_offset;
    ea.ret = ret; ea.pen_ret = pen_ret; ea.pen_sum = pen_sum; ea.len = len; ea.terminated = terminated;
    ea.halted = halted; ea.p.halted_cnt = nullptr;   // per episode here, not per step
    if (compact && rollout_zero_chunks(h, B, s)) return -1;
    hipLaunchKernelGGL(rollout_eval_post_kernel, dim3(ceil_div((int)B, POST_RPB)), dim3(256), 0, s, ea);
    MOPO_HIP(hipGetLastError());
    if (compact) {
      if (rollout_compact(h, B, oc, uc, s)) return -1;
      hipLaunchKernelGGL(rollout_eval_advance_kernel, dim3(1), dim3(1), 0, s, h->cnt, a->d_steps, i);
      uc ^= 1;
    } else {
      oc ^= 1;
    }
    MOPO_HIP(hipGetLastError());
    // once no episode is alive the remaining steps would all return on the zero count: skip them
    if (compact && poll > 0 && (i + 1) % poll == 0 && i + 1 < T) {
      bool none;
      if (rollout_none_alive(h, s, &none)) return -1;
      if (none) break;
    }
  }
  if (!compact && a->d_steps)   // the live count never changed
    hipLaunchKernelGGL(rollout_eval_steps_kernel, dim3(1), dim3(256), 0, s, h->cnt, a->d_steps, T);
  hipLaunchKernelGGL(rollout_eval_stats_kernel, dim3(1), dim3(ST), 0, s, ret, pen_ret, pen_sum, len, terminated, halted,
                     B, stats);
  MOPO_HIP(hipGetLastError());
  return 0;
}
