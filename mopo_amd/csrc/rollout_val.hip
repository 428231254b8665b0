// Open-loop model validation: B segments of up to K steps of the DATASET's actions replayed through the
// learned model from dataset start states, the model fed its own predictions, every step compared with
// what the dataset says happened next -- on the device.  The companion of rollout_eval.hip: that one asks
// how good the policy is if the model is right, this one how right the model is and whether the penalty
// knows.  No reference counterpart (the reference validates by the one-step holdout loss, bnn.py:392-503).
//
// Per step k, on one stream:
//   rollout_val_gather       act = actions[start + k] of the row's segment, the member pick, pen = 0
//   (rollout_xs_wide         wide models only: the scaled input rows; narrow models hand the ensemble the
//                            raw f64 obs / f32 act view, FwdArgs::xs = NULL)
//   bnn_fwd ROLLOUT          the ensemble, as in the training rollout
//   rollout_val_post         FakeEnv's sample / penalty / termination (rollout_post.h), then the errors
//                            against pool row start + k and the continuation test on the DATA (terminal flag,
//                            end of pool, obs[j + 1] == next_obs[j] bit for bit)
//   rollout_compact          obs = next_obs[continues]
//   rollout_eval_advance     live count <- survivors
// then rollout_val_stats reduces the [K][B] tables to the per-step and pooled statistics.
#include "penalty.h"
#include "rollout_post.h"

namespace mopo {

struct ValTabs {
  double* err; double* err_obs; double* err_rew;   // [K][B]
  float* pen;
  uint8_t* term_pred; uint8_t* term_data;
  int32_t* len; uint8_t* end;                      // [B]
};

// the pool's valid row count, read on the device
__device__ __forceinline__ int64_t val_pool_size(const mopo_pool_desc& p) {
  const int64_t n = p.d_state[1];
  return n < 0 ? 0 : (n > p.max_size ? p.max_size : n);
}

// NaN / 0xFF / zero fills, and the segments' start rows: injected, or rollout_start_kernel's Philox draw over
// [0, size).  gidx is the row the start gather may read: the start row itself, or row 0 where it lies
// outside the pool (such a segment ends before its first step).
__global__ void rollout_val_init_kernel(int64_t B, int K, ValTabs t, mopo_pool_desc pool, const int64_t* idx_in,
                                        uint64_t seed, uint32_t step, int64_t uid_offset, int64_t* start,
                                        int64_t* gidx, int64_t* start_out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < (int64_t)K * B) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    t.err[i] = nan; t.err_obs[i] = nan; t.err_rew[i] = nan;
    t.pen[i] = __uint_as_float(0x7fc00000u);
    t.term_pred[i] = 0xFF; t.term_data[i] = 0xFF;
  }
  if (i < B) {
    const int64_t size = val_pool_size(pool);
    const int64_t u = uid_offset + i;
    int64_t src;
    if (idx_in) {
      src = idx_in[i];
    } else {
      u32x4 c{(uint32_t)u, (uint32_t)((uint64_t)u >> 32), step, RNG_START};
      u32x4 r = philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      src = (int64_t)(((uint64_t)r.x * (uint64_t)size) >> 32);
    }
    const bool inside = src >= 0 && src < size;
    start[i] = inside ? src : -1;
    gidx[i] = inside ? src : 0;
    if (start_out) start_out[i] = start[i];
    t.len[i] = 0;
    t.end[i] = inside ? 0 : 3;
  }
}

struct ValGatherArgs {
  const int* cnt;
  const int64_t* uid;
  int64_t uid_offset;
  const int64_t* start;
  int k, A;
  mopo_pool_desc pool;
  float* act;               // [B][A]
  uint32_t* pen_zero;
  int32_t* sel_out;         // NULL: deterministic
  const int32_t* sel_in;    // this step's [B] injected members, or NULL
  const int32_t* elites; int n_elites;
  uint64_t seed; uint32_t step;
};

// eight lanes per live row copy the dataset's action; lane 0 also makes the member pick exactly as the
// rollout's actor does (actor_finish: injected, or Philox RNG_MODEL over the elites) and zeroes the penalty
__global__ __launch_bounds__(256) void rollout_val_gather_kernel(const ValGatherArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t row = i >> 3;
  const int l = (int)(i & 7);
  if (row >= (int64_t)*a.cnt) return;
  const int64_t uid = a.uid[row];
  const int64_t st = a.start[uid - a.uid_offset];
  const int64_t j = st + a.k;
  const bool inside = st >= 0 && j < val_pool_size(a.pool);
  for (int c = l; c < a.A; c += 8) a.act[row * a.A + c] = inside ? a.pool.d_act[j * a.A + c] : 0.f;
  if (l == 0) {
    a.pen_zero[row] = 0u;
    if (a.sel_out) {
      int32_t sel;
      if (a.sel_in) {
        sel = a.sel_in[row];
      } else {  // perf mode of np.random.choice(elites, B) (bnn.py:343)
        u32x4 c{(uint32_t)uid, (uint32_t)((uint64_t)uid >> 32), a.step, RNG_MODEL};
        u32x4 r = philox(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        sel = a.elites[(int)(((uint64_t)r.x * (uint64_t)a.n_elites) >> 32)];
      }
      a.sel_out[row] = sel;
    }
  }
}

struct ValPostArgs {
  PostArgs p;               // pool: the validated pool (read only); stage_base / pool_off / coeff unused
  int64_t uid_offset, B;
  const int64_t* start;
  int k, K;
  ValTabs t;
};

// One FakeEnv step (rollout_post.h) for POST_RPB rows per block, a 32-lane group per row.  Its own part,
// against pool row j = start + k: the errors in f64, the termination rule's verdict beside the data's flag, and
// whether the segment goes on.  A live row is the only row of its segment, so the segment's outputs take plain
// stores.
__global__ __launch_bounds__(256) void rollout_val_post_kernel(const ValPostArgs va) {
  const PostArgs& a = va.p;
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

  // the dataset's row j: what really happened after (obs[j], actions[j])
  const int64_t size = val_pool_size(a.pool);
  const int64_t seg = live ? a.uid[row] - va.uid_offset : 0;       // in [0, B): the start kernel's ids
  const int64_t st = live ? va.start[seg] : -1;
  const int64_t j = st + va.k;
  const bool inside = live && st >= 0 && j < size;                 // false only for a start row outside the pool
  const bool more = inside && j + 1 < size;
  double q = 0.0;
  int differs = 0;
  if (inside && on && sub >= 1) {
    const float nx = a.pool.d_next_obs[j * O + sub - 1];
    const double d = s - (double)nx;
    q = d * d;
    if (more) differs = __float_as_uint(a.pool.d_obs[(j + 1) * O + sub - 1]) != __float_as_uint(nx);
  }
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) {                              // the row's 32-lane group, a fixed order
    q += __shfl_xor(q, o);
    differs |= __shfl_xor(differs, o);
  }
  if (sub == 0) {
    bool keep = false;
    if (inside) {
      const PostVerdict v = post_verdict(a, row, srow[rl], s, pen_d);   // its penalized reward is not used
      const double er = s - (double)a.pool.d_rew[j];               // unpenalized reward (fake_env.py:89)
      const uint8_t td = a.pool.d_term[j] ? 1 : 0;
      const int64_t at = (int64_t)va.k * va.B + seg;
      va.t.err[at] = sqrt(q + er * er);
      va.t.err_obs[at] = sqrt(q);
      va.t.err_rew[at] = er;
      va.t.pen[at] = v.pen;
      va.t.term_pred[at] = v.term ? 1 : 0;
      va.t.term_data[at] = td;
      va.t.len[seg] = va.k + 1;
      int end = 0;
      if (va.k + 1 < va.K) {
        if (td) end = 1;
        else if (!more) end = 3;
        else if (differs) end = 2;
        else keep = true;
      }
      if (!keep) va.t.end[seg] = (uint8_t)end;
    }
    if (live) a.keep[row] = keep ? 1 : 0;
    kept[rl] = keep ? 1 : 0;
  }
  post_count_kept<POST_RPB>(kept, a.blockcnt, nullptr, (int64_t)blockIdx.x * POST_RPB);
}

// The statistics, one 256-thread workgroup per row of the table (rollout_eval_stats_kernel's scheme): row
// k < K over the segments alive at step k, thread t folding segments t, t + 256, ...; row K over every live
// (step, segment) pair in step-major order, thread t folding pairs t, t + 256, ...; then a fixed binary
// tree over the 256 partials, and a second pass around the means for the deviations -- the same bits every
// run.  e* is err for the penalty kinds that are norms over all D outputs (max_aleatoric, ensemble_std),
// err_obs for the kinds over the obs dims (mean_distance, max_pairwise): pen_dist = "over the obs dims".
constexpr int VST = 256;
enum { VQ_N = 0, VQ_ERR, VQ_EOBS, VQ_EREW, VQ_PEN, VQ_COVER, VQ_MIS, VQ_MAX, VQ_COUNT };
__global__ __launch_bounds__(VST) void rollout_val_stats_kernel(ValTabs t, int64_t B, int K, int pen_dist,
                                                                double* stats, int64_t* steps) {
  __shared__ double red[VQ_COUNT][VST];
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  auto tree = [&](int nq) {   // quantities [0, VQ_MAX) sum, VQ_MAX max
    __syncthreads();
    for (int st = VST / 2; st > 0; st >>= 1) {
      if (tid < st)
        for (int q = 0; q < nq; ++q) {
          const double x = red[q][tid], y = red[q][tid + st];
          red[q][tid] = q < VQ_MAX ? x + y : fmax(x, y);
        }
      __syncthreads();
    }
  };
  // this row's items: [i0, i1) of the flattened [K][B] tables; item i is live when its step < its length
  const int64_t i0 = k < K ? (int64_t)k * B : 0, i1 = k < K ? i0 + B : (int64_t)K * B;
  auto alive = [&](int64_t i) { return (int)(i / B) < t.len[i % B]; };
  const double* es = pen_dist ? t.err_obs : t.err;
  double v[VQ_COUNT];
  for (int q = 0; q < VQ_COUNT; ++q) v[q] = q < VQ_MAX ? 0.0 : -INFINITY;
  for (int64_t i = i0 + tid; i < i1; i += VST) {
    if (!alive(i)) continue;
    const double e = t.err[i], u = (double)t.pen[i];
    v[VQ_N] += 1.0; v[VQ_ERR] += e; v[VQ_EOBS] += t.err_obs[i]; v[VQ_EREW] += fabs(t.err_rew[i]);
    v[VQ_PEN] += u;
    v[VQ_COVER] += u >= es[i] ? 1.0 : 0.0;
    v[VQ_MIS] += t.term_pred[i] != t.term_data[i] ? 1.0 : 0.0;
    v[VQ_MAX] = fmax(v[VQ_MAX], e);
  }
  for (int q = 0; q < VQ_COUNT; ++q) red[q][tid] = v[q];
  tree(VQ_COUNT);
  const double n = red[VQ_N][0];
  double* out = stats + (int64_t)k * 16;
  if (n == 0.0) {             // uniform: no segment alive
    if (tid < 16) out[tid] = 0.0;
    if (tid == 0 && steps && k < K) steps[k] = 0;
    return;
  }
  const double emean = red[VQ_ERR][0] / n, umean = red[VQ_PEN][0] / n;
  const double smean = (pen_dist ? red[VQ_EOBS][0] : red[VQ_ERR][0]) / n;
  if (tid == 0) {
    out[0] = n; out[1] = emean; out[3] = red[VQ_MAX][0];
    out[4] = red[VQ_EOBS][0] / n; out[5] = red[VQ_EREW][0] / n; out[6] = umean;
    out[9] = red[VQ_COVER][0] / n; out[10] = red[VQ_MIS][0] / n;
    out[11] = out[12] = out[13] = out[14] = out[15] = 0.0;
    if (steps && k < K) steps[k] = (int64_t)n;
  }
  __syncthreads();   // red is read above by every thread before the second pass overwrites it
  double de = 0.0, du = 0.0, ds = 0.0, dus = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += VST) {
    if (!alive(i)) continue;
    const double a = t.err[i] - emean, b = (double)t.pen[i] - umean, c = es[i] - smean;
    de += a * a; du += b * b; ds += c * c; dus += b * c;
  }
  red[0][tid] = de; red[1][tid] = du; red[2][tid] = ds; red[3][tid] = dus;
  tree(4);
  if (tid == 0) {
    out[2] = sqrt(red[0][0] / n);
    out[7] = sqrt(red[1][0] / n);
    const double vu = red[1][0], vs = red[2][0];
    out[8] = (n < 2.0 || vu == 0.0 || vs == 0.0) ? 0.0 : red[3][0] / sqrt(vu * vs);
  }
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_rollout_validate(mopo_rollout_t hh, const mopo_rollout_args* a, const mopo_pool_desc* pool,
                                     const mopo_val_args* v, void* stream) {
  Rollout* h = reinterpret_cast<Rollout*>(hh);
  MOPO_REQUIRE(h && a && pool && v, "mopo_rollout_validate: NULL argument");
  if (rollout_check_args(h, a, "mopo_rollout_validate", false)) return -1;
  MOPO_REQUIRE(a->horizon >= 1 && a->horizon <= 4095,
               "mopo_rollout_validate: the segment length K must be in [1, 4095] (the Philox step key is "
               "epoch * 4096 + 1 + step)");
  MOPO_REQUIRE(pool->d_obs && pool->d_act && pool->d_rew && pool->d_term && pool->d_next_obs && pool->d_state &&
                   pool->max_size >= 1,
               "mopo_rollout_validate: NULL pool field");
  if (a->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Bnn* bnn = h->bnn;
  const int A = bnn->A, K = a->horizon;
  const int64_t B = a->B;
  const uint32_t step0 = a->epoch * 4096u;

  if (!h->val_mem) {
    const size_t sz[] = {(size_t)h->Bmax * 8, (size_t)h->Bmax * 8};
    size_t off[2];
    MOPO_HIP(hipMalloc(&h->val_mem, carve(sz, 2, off)));
    h->val_start = (int64_t*)h->val_mem;
    h->val_gidx = (int64_t*)((char*)h->val_mem + off[1]);
  }
  // the tables the caller did not ask for live in the handle (the statistics are reduced from them)
  const size_t kb = (size_t)K * B;
  void* const given[] = {v->d_err, v->d_err_obs, v->d_err_rew, v->d_pen, v->d_term_pred, v->d_term_data,
                         v->d_length, v->d_end, v->d_stats};
  const size_t sz[] = {kb * 8, kb * 8, kb * 8, kb * 4, kb, kb, (size_t)B * 4, (size_t)B, (size_t)(K + 1) * 16 * 8};
  size_t off[9];
  const size_t tot = carve(sz, 9, off, given);
  if (tot > h->val_tab_bytes) {
    if (h->val_tab) (void)hipFree(h->val_tab);
    h->val_tab = nullptr;
    h->val_tab_bytes = 0;
    MOPO_HIP(hipMalloc(&h->val_tab, tot));
    h->val_tab_bytes = tot;
  }
  void* p[9];
  for (int i = 0; i < 9; ++i) p[i] = given[i] ? given[i] : (void*)((char*)h->val_tab + off[i]);
  ValTabs t{(double*)p[0], (double*)p[1], (double*)p[2], (float*)p[3], (uint8_t*)p[4], (uint8_t*)p[5],
            (int32_t*)p[6], (uint8_t*)p[7]};
  double* stats = (double*)p[8];

  StepModes m;
  if (rollout_modes(h, a, true, &m)) return -1;   // the penalty is always computed
  // the error the penalty is compared with: err_obs for the kinds over the observation outputs (0 and 2)
  const bool over_obs = m.pen_dist || m.pen_kind == MOPO_PENALTY_MAX_PAIRWISE;

  h->next_step = 0;   // a staged step range must not continue across a validation
  hipLaunchKernelGGL(rollout_val_init_kernel, dim3((unsigned)((kb + 255) / 256)), dim3(256), 0, s, B, K, t, *pool,
                     a->d_start_idx, a->seed, step0, a->uid_offset, h->val_start, h->val_gidx, v->d_start);
  MOPO_HIP(hipGetLastError());
  // the start states obs[r_b] in f64, the row ids and the live count, from the rows the init kernel chose
  if (rollout_start(h, a, pool->d_obs, pool->max_size, h->val_gidx, 1, B, s)) return -1;

  const bool wide = bnn->dev.KG0 > 2;   // internal.h bnn_wide: 64-slot xs rows
  int uc = 0;
  const int oc = 0;                     // every step compacts obs[1] back into obs[0]
  const int poll = rollout_poll_steps();
  for (int i = 0; i < K; ++i) {
    ValGatherArgs ga{};
    ga.cnt = h->cnt; ga.uid = h->uid[uc]; ga.uid_offset = a->uid_offset; ga.start = h->val_start;
    ga.k = i; ga.A = A; ga.pool = *pool; ga.act = h->act; ga.pen_zero = h->pen;
    ga.sel_out = m.det ? nullptr : h->sel;
    ga.sel_in = a->d_model_inds ? a->d_model_inds + (int64_t)i * B : nullptr;
    ga.elites = a->d_elites; ga.n_elites = a->n_elites; ga.seed = a->seed; ga.step = step0 + 1 + i;
    hipLaunchKernelGGL(rollout_val_gather_kernel, dim3((unsigned)((B * 8 + 255) / 256)), dim3(256), 0, s, ga);
    MOPO_HIP(hipGetLastError());
    if (wide && rollout_xs_wide(h, oc, 0, B, h->cnt, h->xs, s)) return -1;

    const FwdArgs f = rollout_fwd_args(h, m, oc, 0, B, h->cnt, wide ? h->xs : nullptr);
    if (launch_bnn_fwd(bnn, FWD_ROLLOUT, f, s)) return -1;
    if (m.pen_kind && rollout_penalty(h, m.pen_kind, 0, B, h->cnt, s)) return -1;

    ValPostArgs va{};
    va.p = rollout_post_args(h, a, m, i, oc, uc, 0, h->cnt, true);
    va.p.pool = *pool;
    va.p.halt = 0; va.p.halted_cnt = nullptr;   // a segment ends where the data does: the halt fields are ignored
    va.uid_offset = a->uid_offset; va.B = B; va.start = h->val_start; va.k = i; va.K = K; va.t = t;
    if (rollout_zero_chunks(h, B, s)) return -1;
    hipLaunchKernelGGL(rollout_val_post_kernel, dim3(ceil_div((int)B, POST_RPB)), dim3(256), 0, s, va);
    MOPO_HIP(hipGetLastError());
    if (rollout_compact(h, B, oc, uc, s)) return -1;
    hipLaunchKernelGGL(rollout_eval_advance_kernel, dim3(1), dim3(1), 0, s, h->cnt, (int64_t*)nullptr, i);
    uc ^= 1;
    MOPO_HIP(hipGetLastError());
    // once no segment is alive the remaining steps would all return on the zero count: skip them
    if (poll > 0 && (i + 1) % poll == 0 && i + 1 < K) {
      bool none;
      if (rollout_none_alive(h, s, &none)) return -1;
      if (none) break;
    }
  }
  hipLaunchKernelGGL(rollout_val_stats_kernel, dim3(K + 1), dim3(VST), 0, s, t, B, K, over_obs ? 1 : 0, stats,
                     v->d_steps);
  MOPO_HIP(hipGetLastError());
  return 0;
}
