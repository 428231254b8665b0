// Model-based policy evaluation: B episodes of up to T steps of the policy inside the learned model
// (RLAlgorithm._evaluation_paths / _evaluate_rollouts, rl_algorithm.py:258-304, with FakeEnv.step as the
// environment), on the device.
//
// Per step, on one stream:
//   actor_kernel             the policy (rollout.hip's launch; no pool: it writes act, the member pick, xs)
//   bnn_fwd ROLLOUT          the ensemble, as in the training rollout
//   rollout_eval_post        FakeEnv's sample / penalty / termination of rollout_post_kernel; instead of a pool
//                            row it adds the step's rewards to the row's episode (uid - uid_offset)
//   rollout_compact          obs = next_obs[~term] (skipped for the never-done domains)
//   rollout_eval_advance     live count <- survivors, steps[i] (with compaction only)
// then rollout_eval_stats reduces the per-episode sums to evaluate_rollouts' statistics.
#include "penalty.h"
#include "rollout.h"

#include <cstdlib>

namespace mopo {

struct EvalPostArgs {
  PostArgs p;               // pool / stage_base / pool_off unused
  int64_t uid_offset;
  double* ret;              // [B] += samples[:, 0]
  double* pen_ret;          // [B] += the penalized reward (fake_env.py:115)
  double* pen_sum;          // [B] += the penalty
  int32_t* len;             // [B] += 1
  uint8_t* terminated;      // [B] = 1 on termination
};

__global__ void rollout_eval_init_kernel(int64_t B, double* ret, double* pen_ret, double* pen_sum, int32_t* len,
                                         uint8_t* terminated) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= B) return;
  ret[i] = 0.0; pen_ret[i] = 0.0; pen_sum[i] = 0.0; len[i] = 0; terminated[i] = 0;
}

// One FakeEnv step (fake_env.py:66-115) for EVAL_RPB rows per block, a 32-lane group per row and a lane per
// output dim, as rollout_post_kernel computes it (same f32 residual add, f64 sample, Philox counters, both
// penalty kinds, deterministic mean over all members).  A live row is the only row of its episode, so the
// episode's accumulators take plain read-modify-writes.
constexpr int EVAL_RPB = 8;   // PB % EVAL_RPB == 0: a block's rows share one compaction chunk
__global__ __launch_bounds__(256) void rollout_eval_post_kernel(const EvalPostArgs ea) {
  const PostArgs& a = ea.p;
  __shared__ double srow[EVAL_RPB][33];
  __shared__ int kept[EVAL_RPB];
  const int tid = threadIdx.x, sub = tid & 31, rl = tid >> 5;
  const int64_t row = (int64_t)blockIdx.x * EVAL_RPB + rl;
  const int O = a.O, D = O + 1;
  const int64_t count = *a.cnt;
  const bool live = row < count;
  const bool on = live && sub < D;
  double s = 0.0;
  // member e's mean of this lane's dim after the residual add, in f32 (fake_env.py:66)
  const double ob = on && sub >= 1 ? a.obs[row * O + sub - 1] : 0.0;
  auto member_mean = [&](int e) {
    const float m = a.mean_all[((int64_t)e * a.all_stride + row) * D + sub];
    return sub >= 1 ? (float)((double)m + ob) : m;
  };
  float pen_d = 0.f;
  if (a.pen_dist) {  // max_e || mean_e - mean_e' mean_e' || over the obs dims (fake_env.py:98-108)
    float sum = 0.f;
    if (on && sub >= 1)
      for (int e = 0; e < a.E; ++e) sum += member_mean(e);
    const float avg = sum / (float)a.E;
    for (int e = 0; e < a.E; ++e) {
      const float dd = on && sub >= 1 ? member_mean(e) - avg : 0.f;
      float q = dd * dd;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) q += __shfl_xor(q, o);       // the row's 32-lane group
      pen_d = fmaxf(pen_d, sqrtf(q));
    }
  }
  if (on && a.det) {  // samples = mean over ALL members of the means (fake_env.py:69-70, 84-86)
    float acc = 0.f;
    for (int e = 0; e < a.E; ++e) acc += member_mean(e);
    s = (double)(acc / (float)a.E);
    srow[rl][sub] = s;
  } else if (on) {
    float m = a.mean_sel[row * D + sub];
    if (sub >= 1) m = (float)((double)m + ob);                      // fake_env.py:66
    double e;
    if (a.eps) {
      e = a.eps[row * D + sub];
    } else {  // Philox normal `sub` of the row's stream (perf mode of fake_env.py:72)
      const int64_t u = a.uid[row];
      u32x4 c{(uint32_t)u, (uint32_t)((uint64_t)u >> 32) ^ ((uint32_t)(sub >> 2) << 20), a.step, RNG_OBS_NOISE};
      u32x4 r = philox(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      float z0, z1;
      if (sub & 2) box_muller(r.z, r.w, z0, z1);
      else box_muller(r.x, r.y, z0, z1);
      e = (double)((sub & 1) ? z1 : z0);
    }
    s = (double)m + e * (double)a.std_sel[row * D + sub];          // fake_env.py:72
    srow[rl][sub] = s;
  }
  __syncthreads();
  if (on && sub >= 1) a.obs_next[row * O + sub - 1] = s;           // next_obs = samples[:, 1:] (:90)
  if (sub == 0) {
    bool keep = false;
    if (live) {
      const bool term = term_fn(a.term_kind, &srow[rl][1], O);     // fake_env.py:91
      const float pen = a.pen_dist ? pen_d : __uint_as_float(a.pen[row]);
      const double pr = a.coeff != 0.f ? s - (double)a.coeff * (double)pen : s;   // fake_env.py:115
      const int64_t ep = a.uid[row] - ea.uid_offset;               // in [0, B): the start kernel's ids
      ea.ret[ep] += s;                                             // unpenalized_rewards (fake_env.py:89, 127)
      ea.pen_ret[ep] += pr;
      ea.pen_sum[ep] += (double)pen;
      ea.len[ep] += 1;
      if (term) ea.terminated[ep] = 1;
      keep = !term;
      if (a.keep) a.keep[row] = keep ? 1 : 0;
    }
    kept[rl] = keep ? 1 : 0;
  }
  if (a.blockcnt) {
    __syncthreads();
    if (tid == 0) {
      int t = 0;
#pragma unroll
      for (int i = 0; i < EVAL_RPB; ++i) t += kept[i];
      if (t) atomicAdd(a.blockcnt + (int64_t)blockIdx.x * EVAL_RPB / PB, t);
    }
  }
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
enum { SQ_RET = 0, SQ_LEN, SQ_PRET, SQ_PEN, SQ_TERM, SQ_RMIN, SQ_LMIN, SQ_RMAX, SQ_LMAX, SQ_N };
__global__ __launch_bounds__(ST) void rollout_eval_stats_kernel(const double* ret, const double* pen_ret,
                                                                const double* pen_sum, const int32_t* len,
                                                                const uint8_t* terminated, int64_t B,
                                                                double* stats) {
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
    v[SQ_TERM] += (double)terminated[i];
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
    stats[12] = stats[13] = stats[14] = stats[15] = 0.0;
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

// MOPO_EVAL_POLL=<steps between two read-backs of the live count> (0: never read it back); default 32.
// Read at every call (tests compare settings in one process); the results do not depend on it.
static int eval_poll() {
  const char* e = std::getenv("MOPO_EVAL_POLL");
  const int n = e ? std::atoi(e) : 32;
  return n < 0 ? 0 : n;
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_rollout_evaluate(mopo_rollout_t hh, const mopo_rollout_args* a, const mopo_eval_args* e,
                                     void* stream) {
  Rollout* h = reinterpret_cast<Rollout*>(hh);
  MOPO_REQUIRE(h && a && e, "mopo_rollout_evaluate: NULL argument");
  MOPO_REQUIRE(a->B >= 0 && a->B <= h->Bmax, "mopo_rollout_evaluate: B exceeds the handle's max_batch");
  MOPO_REQUIRE(a->horizon >= 1 && a->horizon <= 4095,
               "mopo_rollout_evaluate: the episode length T must be in [1, 4095] (the Philox step key is "
               "epoch * 4096 + 1 + step)");
  MOPO_REQUIRE(a->term_kind >= 0 && a->term_kind < MOPO_TERM_KINDS, "mopo_rollout_evaluate: unknown term_kind");
  MOPO_REQUIRE(a->penalty_learned_var >= 0 && a->penalty_learned_var < MOPO_PENALTY_KINDS,
               std::string("mopo_rollout_evaluate") + kPenaltyKindMsg);
  MOPO_REQUIRE(!(e->policy_deterministic && a->rollout_random),
               "mopo_rollout_evaluate: policy_deterministic with rollout_random (uniform actions have no mean)");
  MOPO_REQUIRE(a->d_env_obs && a->env_size > 0, "mopo_rollout_evaluate: empty env pool");
  MOPO_REQUIRE(a->d_pi_params, "mopo_rollout_evaluate: NULL policy params");
  MOPO_REQUIRE(a->d_model_inds || (a->d_elites && a->n_elites > 0), "mopo_rollout_evaluate: elites required");
  MOPO_REQUIRE(!a->rollout_random || a->d_act_uniform || !a->d_eps_act,
               "mopo_rollout_evaluate: parity mode with rollout_random needs the injected uniforms (d_act_uniform)");
  MOPO_REQUIRE(a->actor_dtype == DT_FP32 || a->actor_dtype == DT_F16X3 || a->actor_dtype == DT_BF16X6,
               "mopo_rollout_evaluate: actor_dtype must be 0 (fp32), 3 (bf16x6) or 4 (f16x3)");
  if (a->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Bnn* bnn = h->bnn;
  const int O = bnn->O, A = bnn->A, D = O + 1, T = a->horizon;
  const int64_t B = a->B;
  const int nblk = ceil_div((int)B, PB);
  const uint32_t step0 = a->epoch * 4096u;
  const bool compact = a->term_kind != MOPO_TERM_HALFCHEETAH;

  if (!h->eval_mem) {
    const size_t n = (size_t)h->Bmax;
    size_t sz[] = {n * 8, n * 8, n * 8, n * 4, n, n * A * 4, 16 * 8};
    size_t off[7], tot = 0;
    for (int i = 0; i < 7; ++i) { off[i] = tot; tot += (sz[i] + 255) & ~(size_t)255; }
    MOPO_HIP(hipMalloc(&h->eval_mem, tot));
    char* m = (char*)h->eval_mem;
    h->ev_ret = (double*)(m + off[0]); h->ev_pen_ret = (double*)(m + off[1]); h->ev_pen_sum = (double*)(m + off[2]);
    h->ev_len = (int32_t*)(m + off[3]); h->ev_term = (uint8_t*)(m + off[4]); h->ev_eps0 = (float*)(m + off[5]);
    h->ev_stats = (double*)(m + off[6]);
  }
  double* ret = e->d_return ? e->d_return : h->ev_ret;
  double* pen_ret = e->d_pen_return ? e->d_pen_return : h->ev_pen_ret;
  double* pen_sum = e->d_pen_sum ? e->d_pen_sum : h->ev_pen_sum;
  int32_t* len = e->d_length ? e->d_length : h->ev_len;
  uint8_t* terminated = e->d_terminated ? e->d_terminated : h->ev_term;
  double* stats = e->d_stats ? e->d_stats : h->ev_stats;

  const int f16 = a->actor_dtype == DT_F16X3 ? 1 : (a->actor_dtype == DT_BF16X6 ? 2 : 0);   // pack_actor's split
  if (!h->wpk || h->wpk_hp != a->pi_hidden || h->wpk_f16 != f16) {
    if (h->wpk) (void)hipFree(h->wpk);
    h->wpk = nullptr;
    MOPO_HIP(hipMalloc(&h->wpk, actor_packed_floats(O, a->pi_hidden, f16) * sizeof(float)));
    h->wpk_hp = a->pi_hidden;
    h->wpk_f16 = f16;
  }
  const bool det = a->deterministic != 0;
  const bool pen_dist = a->penalty_learned_var == 0 && a->penalty_coeff != 0.f;
  // kinds >= 2 (penalty.hip): every member's mean and std, reduced by one kernel behind the ensemble
  const int pen_kind = a->penalty_learned_var >= MOPO_PENALTY_MAX_PAIRWISE && a->penalty_coeff != 0.f
                           ? a->penalty_learned_var : 0;
  const bool need_all = det || pen_dist || pen_kind;
  if (need_all && !h->mean_all)
    MOPO_HIP(hipMalloc(&h->mean_all, (size_t)bnn->E * h->Bmax * D * sizeof(float)));
  if (pen_kind && rollout_penalty_alloc(h)) return -1;

  h->next_step = 0;   // a staged step range must not continue across an evaluation
  hipLaunchKernelGGL(rollout_eval_init_kernel, dim3(ceil_div((int)B, 256)), dim3(256), 0, s, B, ret, pen_ret,
                     pen_sum, len, terminated);
  MOPO_HIP(hipGetLastError());
  if (a->d_steps) MOPO_HIP(hipMemsetAsync(a->d_steps, 0, (size_t)T * sizeof(int64_t), s));
  // the deterministic policy: pi = mu + std * 0 through the sampled path, actor_finish untouched
  if (e->policy_deterministic) MOPO_HIP(hipMemsetAsync(h->ev_eps0, 0, (size_t)B * A * sizeof(float), s));
  hipLaunchKernelGGL(rollout_start_kernel, dim3((unsigned)((B + START_ROWS - 1) / START_ROWS)), dim3(START_TPB), 0, s,
                     a->d_env_obs, a->env_size, a->d_start_idx, O, B, a->seed, step0, a->uid_offset, h->obs[0],
                     h->uid[0], h->cnt, 1, B);
  MOPO_HIP(hipGetLastError());
  if (pack_actor(a->d_pi_params, O, A, a->pi_hidden, h->wpk, s, f16)) return -1;

  const bool wide = bnn->dev.KG0 > 2;   // internal.h bnn_wide: 64-slot xs rows, written behind the actor
  int oc = 0, uc = 0;
  const int poll = eval_poll();
  for (int i = 0; i < T; ++i) {
    const uint32_t st = step0 + 1 + i;
    ActorArgs aa{};
    aa.P = a->d_pi_params; aa.Wpk = h->wpk; aa.O = O; aa.A = A; aa.Hp = a->pi_hidden;
    aa.obs = h->obs[oc]; aa.obs_f64 = 1; aa.B = B; aa.d_count = h->cnt;
    aa.eps = e->policy_deterministic ? h->ev_eps0 : (a->d_eps_act ? a->d_eps_act + (int64_t)i * B * A : nullptr);
    aa.seed = a->seed; aa.step = st; aa.d_uid = h->uid[uc];
    aa.act = h->act;
    aa.stage_base = -1;   // no pool (pool_act NULL): the obs / act half-row is not written anywhere
    aa.pen_zero = h->pen;
    aa.sel_out = det ? nullptr : h->sel;
    aa.sel_in = a->d_model_inds ? a->d_model_inds + (int64_t)i * B : nullptr;
    aa.rand_act = a->rollout_random;
    aa.dtype = a->actor_dtype;
    aa.alone = 1;
    aa.act_uni = a->d_act_uniform ? a->d_act_uniform + (int64_t)i * B * A : nullptr;
    aa.elites = a->d_elites; aa.n_elites = a->n_elites;
    aa.xs = wide ? nullptr : h->xs; aa.xs_mu = bnn->dev.mu; aa.xs_sigma = bnn->dev.sigma; aa.xs_in = bnn->dev.IN;
    if (launch_actor(aa, s)) return -1;
    if (wide) {
      hipLaunchKernelGGL(rollout_xs_wide_kernel, dim3(ceil_div((int)B, 16)), dim3(256), 0, s, h->obs[oc], h->act, O, A,
                         bnn->dev.mu, bnn->dev.sigma, B, h->cnt, h->xs);
      MOPO_HIP(hipGetLastError());
    }

    FwdArgs f{};
    f.in = FwdIn{h->obs[oc], 1, O, h->act, 0, A};
    f.B = B; f.d_count = h->cnt; f.xs = h->xs;
    f.pen_bits = h->pen; f.sel = det ? nullptr : h->sel; f.mean_sel = h->mean_sel; f.std_sel = h->std_sel;
    f.mean_all = need_all ? h->mean_all : nullptr;
    f.std_all = pen_kind ? h->std_all : nullptr;
    f.all_stride = h->Bmax;
    if (launch_bnn_fwd(bnn, FWD_ROLLOUT, f, s)) return -1;
    if (pen_kind && rollout_penalty(h, pen_kind, 0, B, h->cnt, s)) return -1;

    EvalPostArgs ea{};
    PostArgs& pa = ea.p;
    pa.O = O; pa.cnt = h->cnt; pa.obs = h->obs[oc]; pa.uid = h->uid[uc];
    pa.mean_sel = h->mean_sel; pa.std_sel = h->std_sel; pa.pen = h->pen;
    pa.eps = a->d_eps_obs ? a->d_eps_obs + (int64_t)i * B * D : nullptr;
    pa.seed = a->seed; pa.step = st; pa.coeff = a->penalty_coeff; pa.term_kind = a->term_kind;
    pa.obs_next = h->obs[oc ^ 1]; pa.keep = compact ? h->keep : nullptr;
    pa.blockcnt = compact ? h->blockcnt : nullptr;
    pa.stage_base = -1;
    pa.mean_all = f.mean_all; pa.E = bnn->E; pa.all_stride = h->Bmax; pa.pen_dist = pen_dist; pa.det = det;
    ea.uid_offset = a->uid_offset;
    ea.ret = ret; ea.pen_ret = pen_ret; ea.pen_sum = pen_sum; ea.len = len; ea.terminated = terminated;
    if (compact) MOPO_HIP(hipMemsetAsync(h->blockcnt, 0, (size_t)nblk * sizeof(int), s));
    hipLaunchKernelGGL(rollout_eval_post_kernel, dim3(ceil_div((int)B, EVAL_RPB)), dim3(256), 0, s, ea);
    MOPO_HIP(hipGetLastError());
    if (compact) {
      hipLaunchKernelGGL(rollout_compact_kernel, dim3(nblk), dim3(PB), 0, s, O, h->blockcnt, h->keep, h->cnt,
                         h->obs[oc ^ 1], h->obs[oc], h->uid[uc], h->uid[uc ^ 1], h->cnt + 1);
      hipLaunchKernelGGL(rollout_eval_advance_kernel, dim3(1), dim3(1), 0, s, h->cnt, a->d_steps, i);
      uc ^= 1;
    } else {
      oc ^= 1;
    }
    MOPO_HIP(hipGetLastError());
    // once no episode is alive the remaining steps would all return on the zero count: skip them
    if (compact && poll > 0 && (i + 1) % poll == 0 && i + 1 < T) {
      int live = 0;
      MOPO_HIP(hipMemcpyAsync(&live, h->cnt, sizeof(int), hipMemcpyDeviceToHost, s));
      MOPO_HIP(hipStreamSynchronize(s));
      if (live == 0) break;
    }
  }
  if (!compact && a->d_steps)   // the live count never changed
    hipLaunchKernelGGL(rollout_eval_steps_kernel, dim3(1), dim3(256), 0, s, h->cnt, a->d_steps, T);
  hipLaunchKernelGGL(rollout_eval_stats_kernel, dim3(1), dim3(ST), 0, s, ret, pen_ret, pen_sum, len, terminated, B,
                     stats);
  MOPO_HIP(hipGetLastError());
  return 0;
}
