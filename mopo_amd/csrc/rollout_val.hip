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
//   rollout_val_post         FakeEnv's sample / penalty / termination of rollout_post_kernel, then the errors
//                            against pool row start + k and the continuation test on the DATA (terminal flag,
//                            end of pool, obs[j + 1] == next_obs[j] bit for bit)
//   rollout_compact          obs = next_obs[continues]
//   rollout_eval_advance     live count <- survivors
// then rollout_val_stats reduces the [K][B] tables to the per-step and pooled statistics.
#include "penalty.h"
#include "rollout.h"

#include <cstdlib>

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

// One FakeEnv step for VAL_RPB rows per block in rollout_eval_post_kernel's form (a 32-lane group per row,
// a lane per output dim; same f32 residual add, f64 sample, Philox counters, both penalty kinds,
// deterministic mean over all members), then against pool row j = start + k: the errors in f64, the
// termination rule's verdict beside the data's flag, and whether the segment goes on.  A live row is the only
// row of its segment, so the segment's outputs take plain stores.
constexpr int VAL_RPB = 8;   // PB % VAL_RPB == 0: a block's rows share one compaction chunk
__global__ __launch_bounds__(256) void rollout_val_post_kernel(const ValPostArgs va) {
  const PostArgs& a = va.p;
  __shared__ double srow[VAL_RPB][33];
  __shared__ int kept[VAL_RPB];
  const int tid = threadIdx.x, sub = tid & 31, rl = tid >> 5;
  const int64_t row = (int64_t)blockIdx.x * VAL_RPB + rl;
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
      const bool term = term_fn(a.term_kind, &srow[rl][1], O);     // fake_env.py:91
      const float pen = a.pen_dist ? pen_d : __uint_as_float(a.pen[row]);
      const double er = s - (double)a.pool.d_rew[j];               // unpenalized reward (fake_env.py:89)
      const uint8_t td = a.pool.d_term[j] ? 1 : 0;
      const int64_t at = (int64_t)va.k * va.B + seg;
      va.t.err[at] = sqrt(q + er * er);
      va.t.err_obs[at] = sqrt(q);
      va.t.err_rew[at] = er;
      va.t.pen[at] = pen;
      va.t.term_pred[at] = term ? 1 : 0;
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
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int i = 0; i < VAL_RPB; ++i) t += kept[i];
    if (t) atomicAdd(a.blockcnt + (int64_t)blockIdx.x * VAL_RPB / PB, t);
  }
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

// MOPO_EVAL_POLL, as the evaluation reads it: steps between two read-backs of the live count (0: never)
static int val_poll() {
  const char* e = std::getenv("MOPO_EVAL_POLL");
  const int n = e ? std::atoi(e) : 32;
  return n < 0 ? 0 : n;
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_rollout_validate(mopo_rollout_t hh, const mopo_rollout_args* a, const mopo_pool_desc* pool,
                                     const mopo_val_args* v, void* stream) {
  Rollout* h = reinterpret_cast<Rollout*>(hh);
  MOPO_REQUIRE(h && a && pool && v, "mopo_rollout_validate: NULL argument");
  MOPO_REQUIRE(a->B >= 0 && a->B <= h->Bmax, "mopo_rollout_validate: B exceeds the handle's max_batch");
  MOPO_REQUIRE(a->horizon >= 1 && a->horizon <= 4095,
               "mopo_rollout_validate: the segment length K must be in [1, 4095] (the Philox step key is "
               "epoch * 4096 + 1 + step)");
  MOPO_REQUIRE(a->term_kind >= 0 && a->term_kind < MOPO_TERM_KINDS, "mopo_rollout_validate: unknown term_kind");
  MOPO_REQUIRE(a->penalty_learned_var >= 0 && a->penalty_learned_var < MOPO_PENALTY_KINDS,
               std::string("mopo_rollout_validate") + kPenaltyKindMsg);
  MOPO_REQUIRE(a->deterministic || a->d_model_inds || (a->d_elites && a->n_elites > 0),
               "mopo_rollout_validate: elites required");
  MOPO_REQUIRE(pool->d_obs && pool->d_act && pool->d_rew && pool->d_term && pool->d_next_obs && pool->d_state &&
                   pool->max_size >= 1,
               "mopo_rollout_validate: NULL pool field");
  if (a->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Bnn* bnn = h->bnn;
  const int O = bnn->O, A = bnn->A, D = O + 1, K = a->horizon;
  const int64_t B = a->B;
  const int nblk = ceil_div((int)B, PB);
  const uint32_t step0 = a->epoch * 4096u;

  if (!h->val_mem) {
    const size_t n = ((size_t)h->Bmax * 8 + 255) & ~(size_t)255;
    MOPO_HIP(hipMalloc(&h->val_mem, 2 * n));
    h->val_start = (int64_t*)h->val_mem;
    h->val_gidx = (int64_t*)((char*)h->val_mem + n);
  }
  // the tables the caller did not ask for live in the handle (the statistics are reduced from them)
  const size_t kb = (size_t)K * B;
  void* const given[] = {v->d_err, v->d_err_obs, v->d_err_rew, v->d_pen, v->d_term_pred, v->d_term_data,
                         v->d_length, v->d_end, v->d_stats};
  const size_t sz[] = {kb * 8, kb * 8, kb * 8, kb * 4, kb, kb, (size_t)B * 4, (size_t)B, (size_t)(K + 1) * 16 * 8};
  size_t off[9], tot = 0;
  for (int i = 0; i < 9; ++i) {
    off[i] = tot;
    if (!given[i]) tot += (sz[i] + 255) & ~(size_t)255;
  }
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

  const bool det = a->deterministic != 0;
  const bool pen_dist = a->penalty_learned_var == 0;   // the penalty is always computed
  // kinds >= 2 (penalty.hip): every member's mean and std, reduced by one kernel behind the ensemble
  const int pen_kind = a->penalty_learned_var >= MOPO_PENALTY_MAX_PAIRWISE ? a->penalty_learned_var : 0;
  // the error the penalty is compared with: err_obs for the kinds over the observation outputs (0 and 2)
  const bool over_obs = pen_dist || pen_kind == MOPO_PENALTY_MAX_PAIRWISE;
  const bool need_all = det || pen_dist || pen_kind;
  if (need_all && !h->mean_all)
    MOPO_HIP(hipMalloc(&h->mean_all, (size_t)bnn->E * h->Bmax * D * sizeof(float)));
  if (pen_kind && rollout_penalty_alloc(h)) return -1;

  h->next_step = 0;   // a staged step range must not continue across a validation
  hipLaunchKernelGGL(rollout_val_init_kernel, dim3((unsigned)((kb + 255) / 256)), dim3(256), 0, s, B, K, t, *pool,
                     a->d_start_idx, a->seed, step0, a->uid_offset, h->val_start, h->val_gidx, v->d_start);
  MOPO_HIP(hipGetLastError());
  // the start states obs[r_b] in f64, the row ids and the live count, from the rows the init kernel chose
  hipLaunchKernelGGL(rollout_start_kernel, dim3((unsigned)((B + START_ROWS - 1) / START_ROWS)), dim3(START_TPB), 0, s,
                     pool->d_obs, pool->max_size, h->val_gidx, O, B, a->seed, step0, a->uid_offset, h->obs[0],
                     h->uid[0], h->cnt, 1, B);
  MOPO_HIP(hipGetLastError());

  const bool wide = bnn->dev.KG0 > 2;   // internal.h bnn_wide: 64-slot xs rows
  int uc = 0;
  const int oc = 0;                     // every step compacts obs[1] back into obs[0]
  const int poll = val_poll();
  for (int i = 0; i < K; ++i) {
    const uint32_t st = step0 + 1 + i;
    ValGatherArgs ga{};
    ga.cnt = h->cnt; ga.uid = h->uid[uc]; ga.uid_offset = a->uid_offset; ga.start = h->val_start;
    ga.k = i; ga.A = A; ga.pool = *pool; ga.act = h->act; ga.pen_zero = h->pen;
    ga.sel_out = det ? nullptr : h->sel;
    ga.sel_in = a->d_model_inds ? a->d_model_inds + (int64_t)i * B : nullptr;
    ga.elites = a->d_elites; ga.n_elites = a->n_elites; ga.seed = a->seed; ga.step = st;
    hipLaunchKernelGGL(rollout_val_gather_kernel, dim3((unsigned)((B * 8 + 255) / 256)), dim3(256), 0, s, ga);
    MOPO_HIP(hipGetLastError());
    if (wide) {
      hipLaunchKernelGGL(rollout_xs_wide_kernel, dim3(ceil_div((int)B, 16)), dim3(256), 0, s, h->obs[oc], h->act, O, A,
                         bnn->dev.mu, bnn->dev.sigma, B, h->cnt, h->xs);
      MOPO_HIP(hipGetLastError());
    }

    FwdArgs f{};
    f.in = FwdIn{h->obs[oc], 1, O, h->act, 0, A};
    f.B = B; f.d_count = h->cnt; f.xs = wide ? h->xs : nullptr;
    f.pen_bits = h->pen; f.sel = det ? nullptr : h->sel; f.mean_sel = h->mean_sel; f.std_sel = h->std_sel;
    f.mean_all = need_all ? h->mean_all : nullptr;
    f.std_all = pen_kind ? h->std_all : nullptr;
    f.all_stride = h->Bmax;
    if (launch_bnn_fwd(bnn, FWD_ROLLOUT, f, s)) return -1;
    if (pen_kind && rollout_penalty(h, pen_kind, 0, B, h->cnt, s)) return -1;

    ValPostArgs va{};
    PostArgs& pa = va.p;
    pa.O = O; pa.cnt = h->cnt; pa.obs = h->obs[oc]; pa.uid = h->uid[uc];
    pa.mean_sel = h->mean_sel; pa.std_sel = h->std_sel; pa.pen = h->pen;
    pa.eps = a->d_eps_obs ? a->d_eps_obs + (int64_t)i * B * D : nullptr;
    pa.seed = a->seed; pa.step = st; pa.term_kind = a->term_kind;
    pa.obs_next = h->obs[oc ^ 1]; pa.keep = h->keep; pa.blockcnt = h->blockcnt;
    pa.pool = *pool; pa.stage_base = -1;
    pa.mean_all = f.mean_all; pa.E = bnn->E; pa.all_stride = h->Bmax; pa.pen_dist = pen_dist; pa.det = det;
    va.uid_offset = a->uid_offset; va.B = B; va.start = h->val_start; va.k = i; va.K = K; va.t = t;
    MOPO_HIP(hipMemsetAsync(h->blockcnt, 0, (size_t)nblk * sizeof(int), s));
    hipLaunchKernelGGL(rollout_val_post_kernel, dim3(ceil_div((int)B, VAL_RPB)), dim3(256), 0, s, va);
    MOPO_HIP(hipGetLastError());
    hipLaunchKernelGGL(rollout_compact_kernel, dim3(nblk), dim3(PB), 0, s, O, h->blockcnt, h->keep, h->cnt,
                       h->obs[oc ^ 1], h->obs[oc], h->uid[uc], h->uid[uc ^ 1], h->cnt + 1);
    hipLaunchKernelGGL(rollout_eval_advance_kernel, dim3(1), dim3(1), 0, s, h->cnt, (int64_t*)nullptr, i);
    uc ^= 1;
    MOPO_HIP(hipGetLastError());
    // once no segment is alive the remaining steps would all return on the zero count: skip them
    if (poll > 0 && (i + 1) % poll == 0 && i + 1 < K) {
      int live = 0;
      MOPO_HIP(hipMemcpyAsync(&live, h->cnt, sizeof(int), hipMemcpyDeviceToHost, s));
      MOPO_HIP(hipStreamSynchronize(s));
      if (live == 0) break;
    }
  }
  hipLaunchKernelGGL(rollout_val_stats_kernel, dim3(K + 1), dim3(VST), 0, s, t, B, K, over_obs ? 1 : 0, stats,
                     v->d_steps);
  MOPO_HIP(hipGetLastError());
  return 0;
}
