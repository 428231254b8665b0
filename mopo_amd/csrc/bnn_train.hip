// Probabilistic-ensemble training step (BNN.train) on CDNA4.
//
// Replaces the TF training graph of BNN.finalize (mopo/models/bnn.py:226-249: Gaussian NLL of
// _compile_losses :677-701 + weight decay fc.py:156-157 + 0.01 (sum maxlv - sum minlv), one
// tf.train.AdamOptimizer(1e-3) over all optvars, constructor.py:41) and the per-minibatch
// session.run of BNN.train (bnn.py:425-432); _compile_losses(inc_var_loss=False) for the holdout
// losses (bnn.py:463-475, 486-493); shuffle_rows (:385-387); _save_state / _set_state (:264-285).
// The loop control (holdout split, bootstrap indices, early stopping, elites) stays on the host
// (mopo_amd/bnn.py), drawing from numpy's global stream in the reference's order.
//
// One minibatch step = 2 launches (step_rows): train_rows_kernel (train_rows.h), the row blocks (gather +
// scaler, 4 swish layers + heads, output gradient, loss partials, then the activation-gradient chain with the
// pre-activations held in LDS), and the weight-gradient launch (train_wgrad.h), one block of which runs the
// batch-level tail (max/min log-var gradients and their Adam) beside the weight-gradient tiles, which apply
// weight decay and the TF1 Adam in their epilogue (parameters ping-pong between two buffers).  The 12-launch
// form (gather, 5 forward GEMM launches, loss kernel, 5 backward GEMM launches: step_impl, gemm_group.h)
// serves every shape train_row_form does not admit, MOPO_TRAIN_ROWS=0, and the holdout evaluation's forward.
// Full-batch steps are captured into hipGraphs (8 / 2 / 1+copy-back steps); the epoch's partial last batch
// runs eagerly.  The parameter layout (training master copy, f32) is train_rows.h's TrainLayout.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "train_wgrad.h"

namespace mopo {

namespace {

constexpr int NHID = TR_NHID;
const float WDECAY[NHID + 1] = {0.000025f, 0.00005f, 0.000075f, 0.000075f, 0.0001f};  // constructor.py:30-36

struct Train {
  TrainLayout L{};
  int maxM = 0, max_batch = 0, max_eval = 0;
  float lr = 1e-3f;
  void* mem = nullptr;
  float *Pb[2] = {nullptr, nullptr}, *G = nullptr, *M = nullptr, *V = nullptr, *S = nullptr;  // S: snapshots
  float* beta_pow = nullptr;   // [3]: beta1^t, beta2^t, this step's lr_t
  int* bstep = nullptr;        // minibatch index within the epoch (device)
  unsigned* ticket = nullptr;
  float* part = nullptr;       // loss-kernel block partials
  float* lpart = nullptr;      // row-block path: per (member, row block) loss partials (train_rows.h)
  float* logs = nullptr;       // [4]: last train loss (data term), ...
  float *mu = nullptr, *sigma = nullptr;
  float *X = nullptr, *T = nullptr, *Z[NHID] = {}, *Hh[NHID] = {}, *OUT = nullptr, *dOUT = nullptr, *dZ[NHID] = {};
  float *X2 = nullptr, *T2 = nullptr;   // the staged gather's second row buffers (odd steps of a graph)
  std::vector<int> snap;       // members with a snapshot
  int32_t* wlist = nullptr;    // weight-gradient tiles per XCD (train_wgrad2_kernel): [8][wl_per_x], counts [8]
  int32_t* wcnt = nullptr;
  int wl_per_x = 0;
  // graphs (full-batch steps), keyed by the epoch's data pointers
  hipStream_t gs = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  hipEvent_t ev_order = nullptr, ev_applied = nullptr;   // shuffle: order ready / order consumed
  hipGraphExec_t gexec[3] = {nullptr, nullptr, nullptr};
  hipGraph_t graph[3] = {nullptr, nullptr, nullptr};
  const void* gkey[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t gkey_n = -1; int gkey_b = -1;
  // shuffle workspace
  void* sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
  double* sort_keys = nullptr; int32_t* sort_vals_in = nullptr; int32_t* sort_vals = nullptr;
  int64_t sort_cap = 0;
};

constexpr int LOSS_TPB = 256;

// ---- minibatch gather: X[e][r] = scaler(inputs[row]), T[e][r] = targets[row] ----------------
// row = rows[e * stride + base + r] with base = (*bstep) * batch (training) or 0 (evaluation);
// rows == NULL: row = r for every member.
__global__ void train_gather_kernel(const float* __restrict__ inputs, const float* __restrict__ targets,
                                    const int32_t* __restrict__ rows, int64_t stride, const int* __restrict__ bstep,
                                    int batch, int M, int E, int IN, int D, const float* __restrict__ mu,
                                    const float* __restrict__ sigma, float* __restrict__ X, float* __restrict__ T) {
  const int W = IN + D;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)E * M * W) return;
  const int c = i % W;
  const int64_t er = i / W;
  const int r = er % M, e = er / M;
  const int64_t base = bstep ? (int64_t)(*bstep) * batch : 0;
  const int64_t row = rows ? rows[e * stride + base + r] : r;
  if (c < IN) X[er * IN + c] = (inputs[row * IN + c] - mu[c]) / sigma[c];   // utils.py:96
  else T[er * D + (c - IN)] = targets[row * D + (c - IN)];
}

// ---- training loss gradient (bnn.py:241-249, 677-701): block = (dim d, 256 (member, row) pairs)
// mean = OUT[..., d], raw log-var = OUT[..., D + d]; the gradient itself is train_rows.h's nll_grad.
// The last block to finish reduces the per-dim partials (in block order), adds the 0.01 terms,
// applies Adam to max/min log-var, fixes this step's lr_t and advances beta powers and bstep.
struct LossArgs {
  int E, M, D;
  const float* OUT; const float* T; float* dOUT;
  float* part; unsigned* ticket; float* logs; float* beta_pow; int* bstep; float lr;
  int64_t off_mx, off_mn;
  float* G;                          // gradient buffer (max/min log-var slots written here)
  AdamCtx ad;
};

__global__ __launch_bounds__(LOSS_TPB) void train_loss_kernel(const LossArgs a) {
  __shared__ float sh[64];
  __shared__ int last;
  const int D = a.D, n = a.E * a.M;
  const int per_d = ceil_div(n, LOSS_TPB);
  const int d = blockIdx.x / per_d, chunk = blockIdx.x % per_d;
  const int i = chunk * LOSS_TPB + threadIdx.x;  // (member, row) pair
  const float mx = a.ad.Pc[a.off_mx + d], mn = a.ad.Pc[a.off_mn + d];
  NllGrad g{};   // pairs past the batch: zeros
  if (i < n) {
    const float* o = a.OUT + (int64_t)i * 2 * D;
    const float mean = o[d], raw = o[D + d], y = a.T[(int64_t)i * D + d];
    const float s = 1.f / ((float)a.M * (float)D);
    g = nll_grad<false>(mean, raw, y, mx, mn, s);
    float* go = a.dOUT + (int64_t)i * 2 * D;
    go[d] = g.g_mean;
    go[D + d] = g.g_lv;
  }
  float v[3] = {g.c_mx, g.c_mn, g.c_loss};
  {  // block sums (butterfly per wave, waves in order)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[w * 3 + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
      float t[3] = {0.f, 0.f, 0.f};
      for (int q = 0; q < LOSS_TPB / 64; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] += sh[q * 3 + k];
      float* pp = a.part + 4 * (int64_t)blockIdx.x;
      pp[0] = t[0]; pp[1] = t[1]; pp[2] = t[2];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const unsigned tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = (tk == gridDim.x - 1);
      if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
  }
  __syncthreads();
  if (!last) return;
  // this step's TF1 Adam step size from the pre-update beta powers (every thread reads them
  // before thread 0 advances them below)
  const float b1p = a.beta_pow[0], b2p = a.beta_pow[1];
  const float lr_t = a.lr * sqrtf(1.f - b2p) / (1.f - b1p);
  __syncthreads();
  if ((int)threadIdx.x < D) {
    const int dd = threadIdx.x;
    float gmx = 0.f, gmn = 0.f, loss = 0.f;
    for (int c = 0; c < per_d; ++c) {
      const float* pp = a.part + 4 * (int64_t)(dd * per_d + c);
      gmx += pp[0]; gmn += pp[1]; loss += pp[2];
    }
    gmx += 0.01f;                                                   // 0.01 * sum(max_logvar)
    gmn -= 0.01f;                                                   // -0.01 * sum(min_logvar)
    a.G[a.off_mx + dd] = gmx;
    a.G[a.off_mn + dd] = gmn;
    adam_apply(a.ad, a.off_mx + dd, gmx, adam_load(a.ad, a.off_mx + dd), lr_t);
    adam_apply(a.ad, a.off_mn + dd, gmn, adam_load(a.ad, a.off_mn + dd), lr_t);
    sh[dd] = loss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float loss = 0.f;
    for (int dd = 0; dd < D; ++dd) loss += sh[dd];
    a.logs[0] = loss;                                               // data term of the train loss
    a.beta_pow[2] = lr_t;
    a.beta_pow[0] = b1p * 0.9f;
    a.beta_pow[1] = b2p * 0.999f;
    if (a.bstep) *a.bstep += 1;
    *a.ticket = 0u;
  }
}

// ---- mse loss per member (inc_var_loss=False): mean over rows and dims of (mean - y)^2 --------
constexpr int MSE_TPB = 1024;
__global__ __launch_bounds__(MSE_TPB) void train_mse_kernel(const float* __restrict__ OUT, const float* __restrict__ T,
                                                            int M, int D, float* __restrict__ losses) {
  __shared__ float sh[MSE_TPB / 64];
  const int e = blockIdx.x;
  float acc = 0.f;
  for (int i = threadIdx.x; i < M * D; i += blockDim.x) {
    const int r = i / D, d = i % D;
    const float err = OUT[((int64_t)e * M + r) * 2 * D + d] - T[((int64_t)e * M + r) * D + d];
    acc += err * err;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < MSE_TPB / 64; ++w) t += sh[w];
    losses[e] = t / ((float)M * (float)D);
  }
}

// ---- scaler fit (utils.py:69-86): mean / std over rows, f64 accumulation, std < 1e-12 -> 1 ----
__global__ __launch_bounds__(256) void scaler_fit_kernel(const float* __restrict__ x, int64_t n, int IN,
                                                         float* __restrict__ mu, float* __restrict__ sigma) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) s += x[r * IN + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  const double mean = (sh[0] + sh[1] + sh[2] + sh[3]) / (double)n;
  __syncthreads();
  double q = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const double dv = x[r * IN + c] - mean;
    q += dv * dv;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sd = sqrt((sh[0] + sh[1] + sh[2] + sh[3]) / (double)n);
    mu[c] = (float)mean;
    sigma[c] = sd < 1e-12 ? 1.f : (float)sd;
  }
}

// ---- format_samples_for_training (constructor.py:46-57) over pool rows ---------------------
__global__ void format_kernel(const mopo_pool_desc p, int O, int A, const int64_t* __restrict__ rows, int64_t n,
                              float* __restrict__ inputs, float* __restrict__ targets) {
  const int IN = O + A, D = O + 1, W = IN + D;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * W) return;
  const int64_t r = i / W;
  const int c = i % W;
  const int64_t src = rows ? rows[r] : r;
  if (c < O) inputs[r * IN + c] = p.d_obs[src * O + c];
  else if (c < IN) inputs[r * IN + c] = p.d_act[src * A + (c - O)];
  else if (c == IN) targets[r * D] = p.d_rew[src];
  else targets[r * D + (c - IN)] = p.d_next_obs[src * O + (c - IN - 1)] - p.d_obs[src * O + (c - IN - 1)];
}

// ---- per-member variable copy (snapshots): dir 0: P -> S, 1: S -> P --------------------------
constexpr int MAX_MEMBERS_SET = 64;
struct MemberSpan { int64_t off[2 * (NHID + 1)]; int64_t len[2 * (NHID + 1)]; };

// a set of members in one launch (blockIdx.z = position in the set)
struct MemberSet { int n; int e[MAX_MEMBERS_SET]; };

__global__ void members_copy_kernel(float* __restrict__ P, float* __restrict__ S, const MemberSpan sp,
                                    const MemberSet ms, int dir) {
  const int k = blockIdx.y, e = ms.e[blockIdx.z];
  const int64_t len = sp.len[k], off = sp.off[k] + (int64_t)e * len;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    if (dir == 0) S[off + i] = P[off + i];
    else P[off + i] = S[off + i];
  }
}

MemberSpan member_span(const TrainLayout& L) {
  MemberSpan s{};
  for (int l = 0; l <= NHID; ++l) {
    s.off[2 * l] = L.W[l]; s.len[2 * l] = (int64_t)L.K(l) * L.N(l);
    s.off[2 * l + 1] = L.b[l]; s.len[2 * l + 1] = L.N(l);
  }
  return s;
}

// ---- shuffle_rows: idx[e] <- idx[e][order[e]] ---------------------------------------------
__global__ void apply_order_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ src, int64_t n,
                                   int E, int32_t* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * E) return;
  const int64_t e = i / n;
  dst[i] = src[e * n + order[i]];
}

// sort key of member e's k-th uniform: (e << 53) | u * 2^53.  numpy's random_sample is k / 2^53 with
// an integer k < 2^53 (two MT19937 draws, 27 + 26 bits), so the integer is exact and orders as the
// double does; value = the position within the member row.
__global__ void sort_keys_kernel(const double* __restrict__ u, int64_t n, int E, uint64_t* __restrict__ keys,
                                 int32_t* __restrict__ vals) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * E) return;
  const uint64_t e = (uint64_t)(i / n);
  keys[i] = (e << 53) | (uint64_t)(u[i] * 9007199254740992.0);
  vals[i] = (int32_t)(i % n);
}

// ---------------------------------------------------------------------------------------------
int launch_gather(Train* h, const float* in, const float* tg, const int32_t* rows, int64_t stride, bool use_bstep,
                  int batch, int M, hipStream_t s) {
  const TrainLayout& L = h->L;
  const int64_t tot = (int64_t)L.E * M * (L.IN + L.D);
  hipLaunchKernelGGL(train_gather_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, in, tg, rows, stride,
                     use_bstep ? h->bstep : nullptr, batch, M, L.E, L.IN, L.D, h->mu, h->sigma, h->X, h->T);
  MOPO_HIP(hipGetLastError());
  return 0;
}

// forward of the 4 swish layers + heads on X (M rows per member) with parameters P
int forward(Train* h, const float* P, int M, hipStream_t s, int tile = 0) {
  const TrainLayout& L = h->L;
  const int E = L.E;
  for (int l = 0; l <= NHID; ++l) {
    const int K = L.K(l), N = L.N(l);
    const float* A = l == 0 ? h->X : h->Hh[l - 1];
    std::vector<GemmProb> g;
    for (int e = 0; e < E; ++e) {
      auto p = mk(M, N, K, A + (int64_t)e * M * K, K, 0, P + L.W[l] + (int64_t)e * K * N, N, 0,
                  (l == NHID ? h->OUT : h->Hh[l]) + (int64_t)e * M * N, N);
      p.bias = P + L.b[l] + (int64_t)e * N;
      if (l < NHID) { p.act = ACT_SWISH; p.Z = h->Z[l] + (int64_t)e * M * N; }
      g.push_back(p);
    }
    if (launch_group(g, s, nullptr, nullptr, nullptr, tile)) return -1;
  }
  return 0;
}

// the holdout evaluation's GEMM tiles (MOPO_EVAL_TILE, default 32: ~1000 rows per member)
int eval_tile() {
  static const int v = [] {
    const char* e = std::getenv("MOPO_EVAL_TILE");
    return e ? std::atoi(e) : 32;
  }();
  return v;
}

// the TF1 Adam of one step: reads P = Pb[par], writes Pb[1 - par]; no target copy, no gradient norm
AdamCtx adam_ctx(const Train* h, int par) {
  AdamCtx ad{};
  ad.G = h->G; ad.Pc = h->Pb[par]; ad.Pn = h->Pb[1 - par]; ad.M = h->M; ad.V = h->V; ad.T = nullptr;
  ad.lr_t = h->beta_pow + 2; ad.tau = 0.f; ad.total = h->L.total; ad.n_pi = 0; ad.n_q = 0; ad.norm_part = nullptr;
  return ad;
}

// one minibatch Adam step on the gathered X/T (M rows per member): P = Pb[par] -> Pb[1 - par]
int step_impl(Train* h, int par, int M, bool use_bstep, hipStream_t s) {
  const TrainLayout& L = h->L;
  const int E = L.E, D = L.D;
  const float* P = h->Pb[par];
  if (forward(h, P, M, s)) return -1;
  const AdamCtx ad = adam_ctx(h, par);
  {
    LossArgs a{};
    a.E = E; a.M = M; a.D = D; a.OUT = h->OUT; a.T = h->T; a.dOUT = h->dOUT; a.part = h->part; a.ticket = h->ticket;
    a.logs = h->logs; a.beta_pow = h->beta_pow; a.bstep = use_bstep ? h->bstep : nullptr; a.lr = h->lr;
    a.off_mx = L.mx; a.off_mn = L.mn; a.G = h->G; a.ad = ad;
    const int blocks = D * ceil_div(E * M, LOSS_TPB);
    hipLaunchKernelGGL(train_loss_kernel, dim3(blocks), dim3(LOSS_TPB), 0, s, a);
    MOPO_HIP(hipGetLastError());
  }
  // backward: launch l (l = NHID .. 0) forms dW_l (+ decay, Adam) and, for l >= 1, dZ_{l-1}
  for (int l = NHID; l >= 0; --l) {
    const int K = L.K(l), N = L.N(l);                         // layer l: [K -> N]
    const float* dY = l == NHID ? h->dOUT : h->dZ[l];        // gradient at layer l's output (pre-activation)
    const float* Xin = l == 0 ? h->X : h->Hh[l - 1];
    std::vector<GemmProb> g;
    for (int e = 0; e < E; ++e) {
      const float* dYe = dY + (int64_t)e * M * N;
      // dW_l = X_in^T dY  (+ db = colsum dY), fused decay + Adam
      auto w = mk(K, N, M, Xin + (int64_t)e * M * K, K, 1, dYe, N, 0, h->G + L.W[l] + (int64_t)e * K * N, N);
      w.colsum = h->G + L.b[l] + (int64_t)e * N;
      w.adam = 1;
      w.wd = WDECAY[l];
      g.push_back(w);
      if (l >= 1) {  // dZ_{l-1} = (dY W_l^T) * swish'(Z_{l-1})
        auto dz = mk(M, K, N, dYe, N, 0, P + L.W[l] + (int64_t)e * K * N, N, 1, h->dZ[l - 1] + (int64_t)e * M * K, K);
        dz.mask = h->Z[l - 1] + (int64_t)e * M * K; dz.ldm = K; dz.mask_kind = MASK_DSWISH;
        g.push_back(dz);
      }
    }
    // two problems per member: more than 8 members do not fit one group (gemm_group.h MAXP).  The problems are
    // independent (Adam reads Pb[par] and writes the other buffer), so they may go in several launches.
    for (size_t i = 0; i < g.size(); i += MAXP) {
      const std::vector<GemmProb> part(g.begin() + i, g.begin() + std::min(i + (size_t)MAXP, g.size()));
      if (launch_group(part, s, &ad, nullptr)) return -1;
    }
  }
  return 0;
}

// The dispatch rule's one home (pure, host only): does a step of these dimensions run the row kernels, and as
// which train_rows_kernel<G0, GH, GD>?  use_rows and mopo_bnn_train_step_form both ask here.  The forms are
// train_rows.h's MOPO_TRAIN_ROW_FORMS (the D4RL widths: inputs 14 / 23, hidden 32 / 200 / 256, 2D 24 / 36; ant-sized
// rows; H = 113..128); H and 2D multiples of 4 (b128 weight rows).  MOPO_TRAIN_ROWS=0 selects step_impl instead.
bool train_row_form(int IN, int H, int D, int* blocks3) {
  static const int env = [] {
    const char* e = std::getenv("MOPO_TRAIN_ROWS");
    return e ? std::atoi(e) : 1;
  }();
  const int g0 = ceil_div(IN, 16), gh = ceil_div(H, 16), gd = ceil_div(2 * D, 16);
#define MOPO_TRF(G0, GH, GD) || (g0 == G0 && gh == GH && gd == GD)
  const bool inst = false MOPO_TRAIN_ROW_FORMS(MOPO_TRF);
#undef MOPO_TRF
  if (!(env != 0 && inst && H % 4 == 0 && D % 2 == 0)) return false;
  if (blocks3) { blocks3[0] = g0; blocks3[1] = gh; blocks3[2] = gd; }
  return true;
}

bool use_rows(const Train* h) { return train_row_form(h->L.IN, h->L.H, h->L.D, nullptr); }

// MOPO_TRAIN_WG2 (default 1): the persistent XCD-local weight-gradient launch; 0: train_wgrad_kernel
int train_wg2() {
  static const int v = [] {
    const char* e = std::getenv("MOPO_TRAIN_WG2");
    return e ? std::atoi(e) : 1;
  }();
  return v;
}

// the weight-gradient tiles per XCD (train_wgrad.h make_wlist), on the device
int build_wlist(Train* h) {
  int per = 0;
  const std::vector<int32_t> host = make_wlist(h->L, &per);
  if (hipMalloc(&h->wlist, host.size() * 4) != hipSuccess) return fail("bnn train: out of device memory (tile list)");
  h->wcnt = h->wlist + (size_t)8 * per;
  h->wl_per_x = per;
  MOPO_HIP(hipMemcpy(h->wlist, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// threads per tile workgroup (MOPO_TRAIN_WG2_NT: 512, two per CU; or 1024, one per CU) and tile
// workgroups per XCD (MOPO_TRAIN_WG2_NWX; default: the CUs' resident workgroups)
int train_wg2_nt() {
  static const int v = [] {
    const char* e = std::getenv("MOPO_TRAIN_WG2_NT");
    const int n = e ? std::atoi(e) : 512;
    return n == 1024 ? 1024 : n == 256 ? 256 : 512;
  }();
  return v;
}
int train_wg2_nwx() {
  static const int v = [] {
    const char* e = std::getenv("MOPO_TRAIN_WG2_NWX");
    // the resident workgroups: three 512-thread ones per CU (TRAIN_WG2_KC), one 1024-thread one
    return e ? std::max(1, std::atoi(e)) : (train_wg2_nt() == 1024 ? 32 : train_wg2_nt() == 256 ? 192 : 96);
  }();
  return v;
}

// MOPO_TRAIN_STAGE (default 1): graph-captured full minibatches read rows the previous step gathered
// (train_rows.h TrainRows::staged); needs 16 (IN + D) <= 1024 (two items per row-block thread)
bool train_stage(const Train* h) {
  static const int v = [] {
    const char* e = std::getenv("MOPO_TRAIN_STAGE");
    return e ? std::atoi(e) : 1;
  }();
  return v != 0 && 16 * (h->L.IN + h->L.D) <= 2 * TR_WAVES * 64;
}

// the batch-level tail of a row-path step (train_wgrad.h train_loss_tail) over its nrb row blocks' partials
TrainTail tail_args(Train* h, int par, bool use_bstep, int nrb) {
  TrainTail t{};
  t.E = h->L.E; t.nrb = nrb; t.D = h->L.D; t.lpart = h->lpart; t.mx = h->L.mx; t.mn = h->L.mn;
  t.logs = h->logs; t.beta_pow = h->beta_pow; t.bstep_inc = use_bstep ? h->bstep : nullptr; t.lr = h->lr; t.G = h->G;
  t.ad = adam_ctx(h, par);
  return t;
}

// The same step as two launches: train_rows_kernel (train_rows.h), then every weight gradient (+ decay, Adam)
// and the batch-level tail (train_wgrad.h).  The row blocks gather for themselves (in / tg / idx).
int step_rows(Train* h, int par, const float* in, const float* tg, const int32_t* idx, int64_t stride, bool use_bstep,
              int batch, int M, hipStream_t s, bool staged = false) {
  const TrainLayout& L = h->L;
  const int E = L.E;
  const AdamCtx ad = adam_ctx(h, par);
  TrainRows a{};
  a.E = E; a.M = M; a.IN = L.IN; a.H = L.H; a.D = L.D; a.nrb = ceil_div(M, 16);
  a.inputs = in; a.targets = tg; a.rows = idx; a.stride = stride; a.bstep = use_bstep ? h->bstep : nullptr;
  a.batch = batch; a.mu = h->mu; a.sigma = h->sigma; a.P = h->Pb[par];
  for (int l = 0; l <= NHID; ++l) { a.W[l] = L.W[l]; a.b[l] = L.b[l]; }
  a.mx = L.mx; a.mn = L.mn;
  a.X = h->X; a.T = h->T; a.OUT = h->OUT; a.dOUT = h->dOUT;
  if (staged) {   // step parity par reads X / T[par], gathers the next step into the other pair
    a.staged = 1;
    a.X = par ? h->X2 : h->X; a.T = par ? h->T2 : h->T;
    a.Xn = par ? h->X : h->X2; a.Tn = par ? h->T : h->T2;
  }
  for (int l = 0; l < NHID; ++l) { a.Hh[l] = h->Hh[l]; a.dZ[l] = h->dZ[l]; }
  a.lpart = h->lpart; a.beta_pow = h->beta_pow; a.lr = h->lr;
  const int grid = 8 * a.nrb * ceil_div(E, 8);   // train_rows.h tr_block: a member's row blocks on one XCD
  const int g0 = ceil_div(L.IN, 16), gh = ceil_div(L.H, 16), gd = ceil_div(2 * L.D, 16);
#define MOPO_TRF(G0, GH, GD)                                                                         \
  if (g0 == G0 && gh == GH && gd == GD) {                                                            \
    hipLaunchKernelGGL((train_rows_kernel<G0, GH, GD>), dim3(grid), dim3(TR_WAVES * 64), 0, s, a);   \
    MOPO_HIP(hipGetLastError());                                                                     \
  } else
  MOPO_TRAIN_ROW_FORMS(MOPO_TRF)
  return fail("bnn train: no row-block instantiation for these widths (use_rows)");
#undef MOPO_TRF
  // on this path h->G holds only the max/min log-var gradients (the loss tail); the W/b gradients stay in
  // the tile workgroups' registers and go straight into Adam, never through G (ad.G is then only the base
  // the Adam state offsets are taken against)
  if (train_wg2()) {
    TrainWg2 g{};
    g.M = M;
    g.nwx = train_wg2_nwx();
    g.per_x = h->wl_per_x;
    g.list = h->wlist;
    g.cnt = h->wcnt;
    for (int l = 0; l <= NHID; ++l) {
      g.K[l] = L.K(l);
      g.N[l] = L.N(l);
      g.A[l] = l == 0 ? a.X : h->Hh[l - 1];   // a.X: the staged pair
      g.B[l] = l == NHID ? h->dOUT : h->dZ[l];
      g.W[l] = L.W[l];
      g.b[l] = L.b[l];
      g.wd[l] = WDECAY[l];
    }
    g.ad = ad;
    g.t = tail_args(h, par, use_bstep, a.nrb);
    if (train_wg2_nt() == 1024) hipLaunchKernelGGL(train_wgrad2_kernel<1024>, dim3(8 * g.nwx + 1), dim3(1024), 0, s, g);
    else if (train_wg2_nt() == 256) hipLaunchKernelGGL(train_wgrad2_kernel<256>, dim3(8 * g.nwx + 1), dim3(256), 0, s, g);
    else hipLaunchKernelGGL(train_wgrad2_kernel<512>, dim3(8 * g.nwx + 1), dim3(512), 0, s, g);
    MOPO_HIP(hipGetLastError());
    return 0;
  }
  TrainWgrad g{};
  g.n = NHID + 1;
  g.ad = ad;
  int tot = 0;
  for (int l = NHID, i = 0; l >= 0; --l, ++i) {   // dW_l = X_in^T dY (+ db = colsum dY), decay + Adam; batch = member
    const int K = L.K(l), N = L.N(l);
    const float* dY = l == NHID ? h->dOUT : h->dZ[l];
    const float* Xin = l == 0 ? a.X : h->Hh[l - 1];   // a.X: the staged pair
    GemmProb w = mk(K, N, M, Xin, K, 1, dY, N, 0, h->G + L.W[l], N);
    w.colsum = h->G + L.b[l];
    w.adam = 1;
    w.wd = WDECAY[l];
    w.nb = E;
    g.p[i] = w;
    g.prefix[i] = tot;
    tot += E * ceil_div(K, 32) * ceil_div(N, 32);
  }
  g.prefix[g.n] = tot;
  g.t = tail_args(h, par, use_bstep, a.nrb);
  hipLaunchKernelGGL(train_wgrad_kernel, dim3(tot + 1), dim3(256), 0, s, g);
  MOPO_HIP(hipGetLastError());
  return 0;
}

int copy_back(Train* h, hipStream_t s) {
  MOPO_HIP(hipMemcpyAsync(h->Pb[0], h->Pb[1], h->L.total * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

void drop_graphs(Train* h) {
  for (int i = 0; i < 3; ++i) {
    if (h->gexec[i]) (void)hipGraphExecDestroy(h->gexec[i]);
    if (h->graph[i]) (void)hipGraphDestroy(h->graph[i]);
    h->gexec[i] = nullptr;
    h->graph[i] = nullptr;
  }
}

constexpr int TRAIN_GRAPH_STEPS = 8;

int capture(Train* h, int which, const float* in, const float* tg, const int32_t* idx, int64_t n_idx, int batch) {
  hipStream_t gs = h->gs;
  MOPO_HIP(hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal));
  const int steps = which == 0 ? TRAIN_GRAPH_STEPS : which == 1 ? 2 : 1;
  int rc = 0;
  for (int i = 0; i < steps && !rc; ++i) {
    if (use_rows(h)) {
      rc = step_rows(h, i & 1, in, tg, idx, n_idx, true, batch, batch, gs, train_stage(h));
    } else {
      rc = launch_gather(h, in, tg, idx, n_idx, true, batch, batch, gs);
      if (!rc) rc = step_impl(h, i & 1, batch, true, gs);
    }
  }
  if (!rc && which == 2) rc = copy_back(h, gs);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(gs, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return -1; }
  if (e != hipSuccess) return fail(std::string("bnn train: capture failed: ") + hipGetErrorString(e));
  h->graph[which] = g;
  MOPO_HIP(hipGraphInstantiate(&h->gexec[which], g, nullptr, nullptr, 0));
  return 0;
}

}  // namespace
}  // namespace mopo

using namespace mopo;

extern "C" int mopo_bnn_train_create(mopo_bnn_train_t* out, int E, int obs_dim, int act_dim, int hidden,
                                     int max_batch, int max_eval, float lr) {
  MOPO_REQUIRE(out, "mopo_bnn_train_create: out is NULL");
  MOPO_REQUIRE(E >= 1 && E <= 16, "mopo_bnn_train_create: num_networks must be in [1, 16]");
  MOPO_REQUIRE(obs_dim >= 1 && act_dim >= 1 && hidden >= 1, "mopo_bnn_train_create: bad dims");
  MOPO_REQUIRE(obs_dim + 1 <= 64, "mopo_bnn_train_create: obs_dim + 1 must be <= 64");
  MOPO_REQUIRE(max_batch >= 1 && max_eval >= 0, "mopo_bnn_train_create: bad batch sizes");
  Train* h = new Train();
  h->L = make_layout(E, obs_dim + act_dim, hidden, obs_dim + 1);
  h->lr = lr;
  h->max_batch = max_batch; h->max_eval = max_eval;
  h->maxM = std::max(max_batch, max_eval);
  const TrainLayout& L = h->L;
  const int64_t tot = (L.total + 3) / 4 * 4, mM = h->maxM;
  const int loss_blocks = L.D * ceil_div(E * h->maxM, LOSS_TPB);
  std::vector<std::pair<void**, size_t>> reg;
  auto f = [&](float** p, int64_t cnt) { reg.push_back({(void**)p, (size_t)cnt * 4}); };
  f(&h->Pb[0], tot); f(&h->Pb[1], tot); f(&h->G, tot); f(&h->M, tot); f(&h->V, tot); f(&h->S, tot);
  f(&h->beta_pow, 3); f(&h->part, 4 * (int64_t)loss_blocks);
  f(&h->lpart, 4 * (int64_t)E * ceil_div(max_batch, 16) * L.D); f(&h->logs, 4); f(&h->mu, L.IN); f(&h->sigma, L.IN);
  reg.push_back({(void**)&h->bstep, 4});
  reg.push_back({(void**)&h->ticket, 4});
  f(&h->X, E * mM * L.IN); f(&h->T, E * mM * L.D); f(&h->X2, E * max_batch * L.IN); f(&h->T2, E * max_batch * L.D); f(&h->OUT, E * mM * 2 * L.D); f(&h->dOUT, E * mM * 2 * L.D);
  for (int l = 0; l < NHID; ++l) { f(&h->Z[l], E * mM * L.H); f(&h->Hh[l], E * mM * L.H); f(&h->dZ[l], E * mM * L.H); }
  size_t bytes = 0;
  for (auto& r : reg) bytes += (r.second + 255) & ~(size_t)255;
  if (hipMalloc(&h->mem, bytes) != hipSuccess) { delete h; return fail("mopo_bnn_train_create: out of device memory"); }
  if (hipMemset(h->mem, 0, bytes) != hipSuccess) { (void)hipFree(h->mem); delete h; return fail("memset failed"); }
  char* m = (char*)h->mem;
  for (auto& r : reg) { *r.first = m; m += (r.second + 255) & ~(size_t)255; }
  const float bp[3] = {0.9f, 0.999f, 0.f};
  MOPO_HIP(hipMemcpy(h->beta_pow, bp, sizeof(bp), hipMemcpyHostToDevice));
  if (build_wlist(h)) { (void)hipFree(h->mem); delete h; return -1; }
  std::vector<float> one(L.IN, 1.f);
  MOPO_HIP(hipMemcpy(h->sigma, one.data(), L.IN * 4, hipMemcpyHostToDevice));
  *out = reinterpret_cast<mopo_bnn_train_t>(h);
  return 0;
}

// host only (no device call): the weight-gradient launch's per-XCD tile lists, for tests and tools
extern "C" int mopo_bnn_train_tile_lists(int E, int obs_dim, int act_dim, int hidden, int32_t* out, int64_t cap) {
  MOPO_REQUIRE(E >= 1 && E <= 16 && obs_dim >= 1 && act_dim >= 1 && hidden >= 1 && obs_dim + 1 <= 64,
               "mopo_bnn_train_tile_lists: bad dims");
  // a packed tile id holds the tile row and column in 5 bits each (make_wlist): K, N <= 32 tiles of 32
  MOPO_REQUIRE(ceil_div(obs_dim + act_dim, TW2_T) <= 32 && ceil_div(hidden, TW2_T) <= 32 &&
               ceil_div(2 * (obs_dim + 1), TW2_T) <= 32,
               "mopo_bnn_train_tile_lists: hidden and obs_dim + act_dim must be <= 1024 (5-bit tile ids)");
  int per = 0;
  const std::vector<int32_t> host = make_wlist(make_layout(E, obs_dim + act_dim, hidden, obs_dim + 1), &per);
  if (out) {
    MOPO_REQUIRE(cap >= (int64_t)host.size(), "mopo_bnn_train_tile_lists: output too small (8 per + 8 ints)");
    std::copy(host.begin(), host.end(), out);
  }
  return per;
}

// host only (no device call): which path a trainer of these dimensions steps on in this process
extern "C" int mopo_bnn_train_step_form(int obs_dim, int act_dim, int hidden, int* blocks3) {
  if (obs_dim < 1 || act_dim < 1 || hidden < 1) return 0;
  return train_row_form(obs_dim + act_dim, hidden, obs_dim + 1, blocks3) ? 1 : 0;
}

// Diagnostic builds only (MOPO_TRAIN_STAMPS=1; otherwise -1): the rows launch's per-workgroup phase stamps
// of the last step ([block][8]: 0 start, 1 gathered, 2 layer 0, 3 forward, 4 loss, 5 / 6 / 7 backward), 100 MHz clock
extern "C" int mopo_bnn_train_debug_stamps(uint64_t* h_out, int64_t n) {
#if MOPO_TRAIN_STAMPS
  MOPO_REQUIRE(h_out && n >= 0 && n <= 2048 * 8, "mopo_bnn_train_debug_stamps: bad output");
  MOPO_HIP(hipDeviceSynchronize());
  MOPO_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_train_stamps), n * 8));
  return 0;
#else
  (void)h_out; (void)n;
  return fail("mopo_bnn_train_debug_stamps: library built without MOPO_TRAIN_STAMPS");
#endif
}

extern "C" int mopo_bnn_train_destroy(mopo_bnn_train_t hh) {
  Train* h = reinterpret_cast<Train*>(hh);
  if (!h) return 0;
  drop_graphs(h);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  if (h->ev_out) (void)hipEventDestroy(h->ev_out);
  if (h->ev_order) (void)hipEventDestroy(h->ev_order);
  if (h->ev_applied) (void)hipEventDestroy(h->ev_applied);
  if (h->gs) (void)hipStreamDestroy(h->gs);
  if (h->sort_keys) (void)hipFree(h->sort_keys);  // one allocation (keys | values | offsets | temp)
  if (h->wlist) (void)hipFree(h->wlist);
  if (h->mem) (void)hipFree(h->mem);
  delete h;
  return 0;
}

// .mat order (smv, 16 arrays): mu, sigma, (W, b) x 5 mean layers, (Wv, bv), maxlv, minlv
extern "C" int mopo_bnn_train_set_params(mopo_bnn_train_t hh, const float* const* a) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && a, "mopo_bnn_train_set_params: NULL argument");
  const TrainLayout& L = h->L;
  const int E = L.E, H = L.H, D = L.D;
  std::vector<float> P(L.total);
  for (int l = 0; l < NHID; ++l) {
    std::memcpy(P.data() + L.W[l], a[2 + 2 * l], (size_t)E * L.K(l) * H * 4);
    std::memcpy(P.data() + L.b[l], a[3 + 2 * l], (size_t)E * H * 4);
  }
  for (int e = 0; e < E; ++e) {
    for (int k = 0; k < H; ++k)
      for (int j = 0; j < D; ++j) {
        P[L.W[NHID] + ((int64_t)e * H + k) * 2 * D + j] = a[10][((int64_t)e * H + k) * D + j];
        P[L.W[NHID] + ((int64_t)e * H + k) * 2 * D + D + j] = a[12][((int64_t)e * H + k) * D + j];
      }
    for (int j = 0; j < D; ++j) {
      P[L.b[NHID] + (int64_t)e * 2 * D + j] = a[11][e * D + j];
      P[L.b[NHID] + (int64_t)e * 2 * D + D + j] = a[13][e * D + j];
    }
  }
  std::memcpy(P.data() + L.mx, a[14], D * 4);
  std::memcpy(P.data() + L.mn, a[15], D * 4);
  MOPO_HIP(hipMemcpy(h->Pb[0], P.data(), L.total * 4, hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(h->Pb[1], P.data(), L.total * 4, hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(h->mu, a[0], L.IN * 4, hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(h->sigma, a[1], L.IN * 4, hipMemcpyHostToDevice));
  // a fresh optimizer (the reference initialises the Adam slots with the graph, bnn.py:252)
  MOPO_HIP(hipMemset(h->M, 0, L.total * 4));
  MOPO_HIP(hipMemset(h->V, 0, L.total * 4));
  const float bp[3] = {0.9f, 0.999f, 0.f};
  MOPO_HIP(hipMemcpy(h->beta_pow, bp, sizeof(bp), hipMemcpyHostToDevice));
  h->snap.clear();
  return 0;
}

extern "C" int mopo_bnn_train_get_params(mopo_bnn_train_t hh, float* const* a) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && a, "mopo_bnn_train_get_params: NULL argument");
  const TrainLayout& L = h->L;
  const int E = L.E, H = L.H, D = L.D;
  MOPO_HIP(hipDeviceSynchronize());
  std::vector<float> P(L.total);
  MOPO_HIP(hipMemcpy(P.data(), h->Pb[0], L.total * 4, hipMemcpyDeviceToHost));
  MOPO_HIP(hipMemcpy(a[0], h->mu, L.IN * 4, hipMemcpyDeviceToHost));
  MOPO_HIP(hipMemcpy(a[1], h->sigma, L.IN * 4, hipMemcpyDeviceToHost));
  for (int l = 0; l < NHID; ++l) {
    std::memcpy(a[2 + 2 * l], P.data() + L.W[l], (size_t)E * L.K(l) * H * 4);
    std::memcpy(a[3 + 2 * l], P.data() + L.b[l], (size_t)E * H * 4);
  }
  for (int e = 0; e < E; ++e) {
    for (int k = 0; k < H; ++k)
      for (int j = 0; j < D; ++j) {
        a[10][((int64_t)e * H + k) * D + j] = P[L.W[NHID] + ((int64_t)e * H + k) * 2 * D + j];
        a[12][((int64_t)e * H + k) * D + j] = P[L.W[NHID] + ((int64_t)e * H + k) * 2 * D + D + j];
      }
    for (int j = 0; j < D; ++j) {
      a[11][e * D + j] = P[L.b[NHID] + (int64_t)e * 2 * D + j];
      a[13][e * D + j] = P[L.b[NHID] + (int64_t)e * 2 * D + D + j];
    }
  }
  std::memcpy(a[14], P.data() + L.mx, D * 4);
  std::memcpy(a[15], P.data() + L.mn, D * 4);
  return 0;
}

extern "C" int mopo_bnn_format_samples(const mopo_pool_desc* pool, int O, int A, const int64_t* d_rows, int64_t n,
                                       float* d_inputs, float* d_targets, void* stream) {
  MOPO_REQUIRE(pool && d_inputs && d_targets, "mopo_bnn_format_samples: NULL argument");
  MOPO_REQUIRE(n >= 0, "mopo_bnn_format_samples: n < 0");
  if (n == 0) return 0;
  const int64_t tot = n * (2 * O + A + 1);
  hipLaunchKernelGGL(format_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *pool, O, A,
                     d_rows, n, d_inputs, d_targets);
  MOPO_HIP(hipGetLastError());
  return 0;
}

extern "C" int mopo_bnn_train_fit_scaler(mopo_bnn_train_t hh, const float* d_inputs, int64_t n, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && d_inputs && n > 0, "mopo_bnn_train_fit_scaler: bad argument");
  hipLaunchKernelGGL(scaler_fit_kernel, dim3(h->L.IN), dim3(256), 0, (hipStream_t)stream, d_inputs, n, h->L.IN, h->mu,
                     h->sigma);
  MOPO_HIP(hipGetLastError());
  return 0;
}

extern "C" int mopo_bnn_train_epoch(mopo_bnn_train_t hh, const float* d_in, const float* d_tg, const int32_t* d_idxs,
                                    int64_t n_idx, int batch, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && d_in && d_tg && d_idxs, "mopo_bnn_train_epoch: NULL argument");
  MOPO_REQUIRE(batch >= 1 && batch <= h->max_batch, "mopo_bnn_train_epoch: batch exceeds max_batch");
  MOPO_REQUIRE(n_idx >= 1, "mopo_bnn_train_epoch: empty index set");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = (n_idx + batch - 1) / batch;
  const int last = (int)(n_idx - (nb - 1) * batch);
  const int64_t nfull = last == batch ? nb : nb - 1;
  if (!h->gs) {
    MOPO_HIP(hipStreamCreateWithFlags(&h->gs, hipStreamNonBlocking));
    MOPO_HIP(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    MOPO_HIP(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
  }
  hipStream_t gs = h->gs;
  MOPO_HIP(hipEventRecord(h->ev_in, s));
  MOPO_HIP(hipStreamWaitEvent(gs, h->ev_in, 0));
  MOPO_HIP(hipMemsetAsync(h->bstep, 0, 4, gs));
  if (nfull > 0) {
    if (!h->gexec[0] || h->gkey[0] != d_in || h->gkey[1] != d_tg || h->gkey[2] != d_idxs || h->gkey_n != n_idx ||
        h->gkey_b != batch) {
      drop_graphs(h);
      if (capture(h, 0, d_in, d_tg, d_idxs, n_idx, batch) || capture(h, 1, d_in, d_tg, d_idxs, n_idx, batch) ||
          capture(h, 2, d_in, d_tg, d_idxs, n_idx, batch))
        return -1;
      h->gkey[0] = d_in; h->gkey[1] = d_tg; h->gkey[2] = d_idxs; h->gkey_n = n_idx; h->gkey_b = batch;
    }
    // staged steps: the epoch's first minibatch is gathered here, every later one by the step before it
    if (use_rows(h) && train_stage(h) && launch_gather(h, d_in, d_tg, d_idxs, n_idx, true, batch, batch, gs))
      return -1;
    int64_t i = 0;
    for (; i + TRAIN_GRAPH_STEPS <= nfull; i += TRAIN_GRAPH_STEPS) MOPO_HIP(hipGraphLaunch(h->gexec[0], gs));
    for (; i + 2 <= nfull; i += 2) MOPO_HIP(hipGraphLaunch(h->gexec[1], gs));
    if (i < nfull) MOPO_HIP(hipGraphLaunch(h->gexec[2], gs));
  }
  if (nfull < nb) {  // the epoch's partial last minibatch (bnn.py:426: idxs[:, b*bs:(b+1)*bs])
    if (use_rows(h)) {
      if (step_rows(h, 0, d_in, d_tg, d_idxs, n_idx, true, batch, last, gs) || copy_back(h, gs)) return -1;
    } else if (launch_gather(h, d_in, d_tg, d_idxs, n_idx, true, batch, last, gs) || step_impl(h, 0, last, true, gs) ||
               copy_back(h, gs)) {
      return -1;
    }
  }
  MOPO_HIP(hipEventRecord(h->ev_out, gs));
  MOPO_HIP(hipStreamWaitEvent(s, h->ev_out, 0));
  return 0;
}

extern "C" int mopo_bnn_train_eval_mse(mopo_bnn_train_t hh, const float* d_in, const float* d_tg, const int32_t* d_rows,
                                       int n, float* d_losses, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && d_in && d_tg && d_losses, "mopo_bnn_train_eval_mse: NULL argument");
  MOPO_REQUIRE(n >= 1 && n <= h->maxM, "mopo_bnn_train_eval_mse: n must be in [1, max(max_batch, max_eval)]");
  hipStream_t s = (hipStream_t)stream;
  if (launch_gather(h, d_in, d_tg, d_rows, n, false, 0, n, s) ||
      forward(h, h->Pb[0], n, s, n >= 32 ? eval_tile() : 0))
    return -1;
  hipLaunchKernelGGL(train_mse_kernel, dim3(h->L.E), dim3(MSE_TPB), 0, s, h->OUT, h->T, n, h->L.D, d_losses);
  MOPO_HIP(hipGetLastError());
  return 0;
}

extern "C" int mopo_bnn_train_shuffle(mopo_bnn_train_t hh, int32_t* d_idxs, const double* d_keys, int64_t n,
                                      void* stream) {
  return mopo_bnn_train_shuffle_async(hh, d_idxs, d_keys, n, stream, stream);
}

extern "C" int mopo_bnn_train_shuffle_async(mopo_bnn_train_t hh, int32_t* d_idxs, const double* d_keys, int64_t n,
                                            void* order_stream, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && d_idxs && d_keys && n >= 1, "mopo_bnn_train_shuffle: bad argument");
  MOPO_REQUIRE(n * h->L.E < (1ll << 31), "mopo_bnn_train_shuffle: index set too large");
  hipStream_t s = (hipStream_t)stream, os = (hipStream_t)order_stream;
  const int E = h->L.E;
  const int64_t tot = n * E;
  int seg_bits = 0;
  while ((1 << seg_bits) < E) ++seg_bits;
  const int end_bit = 53 + seg_bits;
  if (!h->ev_order) {
    MOPO_HIP(hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming));
    MOPO_HIP(hipEventCreateWithFlags(&h->ev_applied, hipEventDisableTiming));
  }
  if (h->sort_cap < tot) {
    MOPO_HIP(hipStreamSynchronize(s));           // the buffers below may still be read by an earlier apply
    if (h->sort_keys) (void)hipFree(h->sort_keys);
    h->sort_tmp = nullptr; h->sort_keys = nullptr;
    size_t tb = 0;
    MOPO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                (const int32_t*)nullptr, (int32_t*)nullptr, (int)tot, 0, end_bit, os));
    // one allocation: keys in | keys out | values in | values out | temp storage
    const size_t kb = (size_t)tot * 8, vb = (size_t)tot * 4;
    char* m = nullptr;
    MOPO_HIP(hipMalloc((void**)&m, 2 * kb + 2 * vb + tb + 1024));
    h->sort_keys = (double*)m;
    h->sort_vals_in = (int32_t*)(m + 2 * kb);
    h->sort_vals = (int32_t*)(m + 2 * kb + vb);
    h->sort_tmp = (void*)(((uintptr_t)(m + 2 * kb + 2 * vb) + 255) & ~(uintptr_t)255);
    h->sort_tmp_bytes = tb;
    h->sort_cap = tot;
  } else if (os != s) {
    // the order is computed on the caller's order stream, which can run beside the epoch's steps; it
    // must not overwrite the order buffers before the previous shuffle's apply has read them
    MOPO_HIP(hipStreamWaitEvent(os, h->ev_applied, 0));
  }
  uint64_t* kin = reinterpret_cast<uint64_t*>(h->sort_keys);
  uint64_t* kout = kin + h->sort_cap;
  hipLaunchKernelGGL(sort_keys_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, os, d_keys, n, E, kin,
                     h->sort_vals_in);
  MOPO_HIP(hipGetLastError());
  size_t tb = h->sort_tmp_bytes;
  // one radix sort of (member, 53-bit integer of the uniform) == np.argsort within each member row
  MOPO_HIP(hipcub::DeviceRadixSort::SortPairs(h->sort_tmp, tb, kin, kout, h->sort_vals_in, h->sort_vals, (int)tot, 0,
                                              end_bit, os));
  if (os != s) {
    MOPO_HIP(hipEventRecord(h->ev_order, os));
    MOPO_HIP(hipStreamWaitEvent(s, h->ev_order, 0));
  }
  int32_t* tmp_idx = h->sort_vals_in;  // reuse: copy of the current indices
  MOPO_HIP(hipMemcpyAsync(tmp_idx, d_idxs, tot * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(apply_order_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, h->sort_vals, tmp_idx,
                     n, E, d_idxs);
  MOPO_HIP(hipGetLastError());
  MOPO_HIP(hipEventRecord(h->ev_applied, s));
  return 0;
}

static int copy_members(Train* h, const std::vector<int>& members, int dir, hipStream_t s) {
  for (size_t i0 = 0; i0 < members.size(); i0 += MAX_MEMBERS_SET) {
    MemberSet ms{};
    ms.n = (int)std::min(members.size() - i0, (size_t)MAX_MEMBERS_SET);
    for (int i = 0; i < ms.n; ++i) ms.e[i] = members[i0 + i];
    hipLaunchKernelGGL(members_copy_kernel, dim3(64, 2 * (NHID + 1), ms.n), dim3(256), 0, s, h->Pb[0], h->S,
                       member_span(h->L), ms, dir);
    MOPO_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int mopo_bnn_train_snapshot(mopo_bnn_train_t hh, int member, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && member >= 0 && member < h->L.E, "mopo_bnn_train_snapshot: bad member");
  if (copy_members(h, {member}, 0, (hipStream_t)stream)) return -1;
  if (std::find(h->snap.begin(), h->snap.end(), member) == h->snap.end()) h->snap.push_back(member);
  return 0;
}

extern "C" int mopo_bnn_train_snapshot_members(mopo_bnn_train_t hh, const int* h_members, int n, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && (h_members || n == 0) && n >= 0, "mopo_bnn_train_snapshot_members: bad argument");
  std::vector<int> ms;
  for (int i = 0; i < n; ++i) {
    const int e = h_members[i];
    MOPO_REQUIRE(e >= 0 && e < h->L.E, "mopo_bnn_train_snapshot_members: bad member");
    if (std::find(ms.begin(), ms.end(), e) == ms.end()) ms.push_back(e);
  }
  if (ms.empty()) return 0;
  if (copy_members(h, ms, 0, (hipStream_t)stream)) return -1;
  for (int e : ms)
    if (std::find(h->snap.begin(), h->snap.end(), e) == h->snap.end()) h->snap.push_back(e);
  return 0;
}

extern "C" int mopo_bnn_train_restore(mopo_bnn_train_t hh, void* stream) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h, "mopo_bnn_train_restore: NULL handle");
  if (!h->snap.empty() && copy_members(h, h->snap, 1, (hipStream_t)stream)) return -1;
  h->snap.clear();
  return 0;
}

extern "C" int mopo_bnn_train_logs(mopo_bnn_train_t hh, float* h_logs, int n) {
  Train* h = reinterpret_cast<Train*>(hh);
  MOPO_REQUIRE(h && h_logs && n >= 1 && n <= 4, "mopo_bnn_train_logs: bad argument");
  MOPO_HIP(hipDeviceSynchronize());
  MOPO_HIP(hipMemcpy(h_logs, h->logs, n * 4, hipMemcpyDeviceToHost));
  return 0;
}
