// Row-block kernel of the ensemble training step (bnn_train.hip): the row-local half of a minibatch step
// in one launch.
//
//   train_rows_kernel<G0, GH, GD>, one workgroup per (member, 16 rows): the minibatch gather (bootstrap
//     rows, scaler: utils.py:96), the four swish layers and the fused mean / log-var head of the member
//     for its 16 rows (fc.py:84-106; activations H stored for the weight gradients, pre-activations Z kept
//     in LDS), the output gradient of the Gaussian NLL through the soft log-var bounds (bnn.py:241-249,
//     669-701), the block's partial sums of the max/min log-var gradients and of the loss, and the
//     activation-gradient chain dZ_{l-1} = (dY_l W_l^T) * swish'(Z_{l-1}), l = 4 .. 1
//   the weight-gradient launch (train_wgrad.h) follows: every X_in^T dY (+ bias column sums, weight decay,
//     TF1 Adam in the epilogue), and one block that reduces the partials and applies the batch-level updates
//
// Every row-local quantity stays in its workgroup: the layer's 16 x K input sits in LDS, each of the 8
// waves contracts 2 output tiles of 16 columns over the whole K on v_mfma_f32_16x16x4_f32
// (exact f32 products, f32 accumulation), its weight columns streamed from L2 straight into MFMA B
// registers two k-groups ahead (b64 / b128 loads), and the layer's output goes back to LDS for the next layer.
// A member's row blocks share one XCD (tr_block), so its weights are fetched into one L2.
// Requires H, IN <= 256, 2D <= 256, H and 2D multiples of 4 (bnn_train.hip train_row_form).
#pragma once
#include <type_traits>

#include "gemm_group.h"

namespace mopo {

constexpr int TR_NHID = 4;
#ifndef TR_LD_CFG
#define TR_LD_CFG 260
#endif
constexpr int TR_LD = TR_LD_CFG;   // LDS row stride (floats) of a 16-row activation block: K <= 256 (+4: b128 reads conflict-free)

// Every train_rows_kernel<G0, GH, GD> the library holds: 16-wide k-groups of the inputs, the hidden width and
// the 2D head columns.  train_row_form admits exactly these and step_rows dispatches over them (bnn_train.hip).
#define MOPO_TRAIN_ROW_FORMS(X)                                                                  \
  X(2, 13, 3) X(1, 13, 2) X(1, 2, 2) X(2, 2, 3) X(2, 16, 3) X(1, 16, 2)                         \
  X(3, 13, 4) X(3, 4, 4) /* ant-sized rows: 27 + 8 inputs, 56 head columns */                    \
  X(2, 8, 3) X(1, 8, 2)  /* H = 113..128 */

// Training master copy of the parameters (f32): per member, the reference's optvars with the two smv heads
// concatenated column-wise so one GEMM serves both:
//   W0 [E][IN][H] b0 [E][H]  W1..W3 [E][H][H] b1..b3 [E][H]  Whd [E][H][2D] bhd [E][2D]
//   maxlv [D] minlv [D]        (Whd[e][k][n]: n < D mean head, n >= D log-var head)
struct TrainLayout {
  int E, IN, H, D;
  int64_t W[TR_NHID + 1], b[TR_NHID + 1];  // offsets (layer TR_NHID = concatenated heads)
  int64_t mx, mn, total;
  int K(int l) const { return l == 0 ? IN : H; }             // layer l: [K -> N]
  int N(int l) const { return l == TR_NHID ? 2 * D : H; }
};

static inline TrainLayout make_layout(int E, int IN, int H, int D) {
  TrainLayout L{};
  L.E = E; L.IN = IN; L.H = H; L.D = D;
  int64_t c = 0;
  for (int l = 0; l <= TR_NHID; ++l) {
    L.W[l] = c; c += (int64_t)E * L.K(l) * L.N(l);
    L.b[l] = c; c += (int64_t)E * L.N(l);
  }
  L.mx = c; c += D;
  L.mn = c; c += D;
  L.total = c;
  return L;
}

struct TrainRows {
  int E, M, IN, H, D, nrb;
  // gather: row = rows[e * stride + (*bstep) * batch + r] (rows == NULL: r)
  const float* inputs; const float* targets; const int32_t* rows; int64_t stride; const int* bstep; int batch;
  const float* mu; const float* sigma;
  const float* P;                    // this step's parameters (TrainLayout)
  int64_t W[TR_NHID + 1], b[TR_NHID + 1], mx, mn;
  float* X; float* T; float* Hh[TR_NHID]; float* OUT; float* dOUT; float* dZ[TR_NHID];
  // staged (graph-captured full minibatches): this step's rows are already gathered in X / T (by the
  // previous step, or the epoch's first gather), and the block gathers the NEXT step's rows into Xn / Tn,
  // its loads issued at the start and stored at the end (the gather's dependent chain off the step's path)
  int staged; float* Xn; float* Tn;
  float* lpart;                      // [E][nrb][D][4]: d loss / d maxlv, d loss / d minlv, loss (per row block)
  float* beta_pow; float lr;         // block 0 writes this step's lr_t = beta_pow[2] for the weight-gradient launch
};

static __device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t d, int idx) {   // idx < 0: zeros
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d, idx * 4, 0, 0));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// W, K, N, ldw are wave-uniform but computed from a runtime layer index: forced into SGPRs here, since a
// buffer descriptor the compiler believes divergent is wrapped in a readfirstlane waterfall loop around
// every load (measured: the step's forward kernel 2x slower)
static __device__ __forceinline__ const float* uniform_ptr(const float* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const float*)(((uint64_t)hi << 32) | lo);
}

// Workgroups of TR_WAVES waves: wave w owns column block cb = w % 4 (64 columns) and TW = 16 / TR_WAVES
// of its 4 tiles (two waves per SIMD at 8: one wave's memory waits overlap the other's MFMAs; 16: one
// tile per wave, four waves per SIMD -- measured 10.07k -> 8.5k grad-steps/s, same-box A/B).
#ifndef TR_WAVES_CFG
#define TR_WAVES_CFG 8
#endif
constexpr int TR_WAVES = TR_WAVES_CFG, TR_TW = 16 / TR_WAVES;

// The row-block GEMM (rows_gemm_pre): acc[q] = A[16 x K] x B over the whole K for tiles q < TW of the wave.
// Tile q's column li is column c + q, c = 64 cb + 4 li + TW (w / 4), so a lane's B values of one k are one
// b64 / b128 load (KT = false) and its outputs of one row one b64 / b128 store.  A in LDS (row stride TR_LD,
// zero past K up to the next multiple of 16); B(k, c) = W[k * ldw + c] (KT = false) or W[c * ldw + k]
// (KT = true), zero outside k < K, c < N (N and, for KT, K multiples of 4).  Lane (li, lk) contracts
// k = 16 grp + 4 lk + u (one ds_read_b128 of A per k-group).  G = ceil(K / 16) at compile time: straight-line
// code with the loads TR_PF k-groups ahead (a runtime k-group loop made the compiler wait for all but 2 of
// the prefetched loads at its header).  The layer's first TR_PF k-groups of B are loaded ahead (rows_pre),
// across the previous layer's epilogue and barrier: the weights do not depend on the activations, so a
// layer does not start on an exposed L2 round trip.
#ifndef TR_PF_CFG
#define TR_PF_CFG 2
#endif
// k-groups of B loaded ahead of their MFMAs (4 / 7: 11.52k -> 11.41k / 11.10k grad-steps/s, same-box A/B)
constexpr int TR_PF = TR_PF_CFG;
#ifndef TR_PF_B_CFG
#define TR_PF_B_CFG TR_PF_CFG   // the rows kernel's backward (transposed weight reads)
#endif
constexpr int TR_PF_B = TR_PF_B_CFG, TR_PFM = TR_PF > TR_PF_B ? TR_PF : TR_PF_B;
struct RowsW {
  __amdgpu_buffer_rsrc_t d;
  int K, N, ldw;
};
template <bool KT>
static __device__ __forceinline__ RowsW rows_w(const float* Wv, int Kv, int Nv, int ldwv) {
  const float* W = uniform_ptr(Wv);
  RowsW r;
  r.K = __builtin_amdgcn_readfirstlane(Kv);
  r.N = __builtin_amdgcn_readfirstlane(Nv);
  r.ldw = __builtin_amdgcn_readfirstlane(ldwv);
  r.d = rsrc(W, KT ? (int64_t)(r.N - 1) * r.ldw + r.K : (int64_t)(r.K - 1) * r.ldw + r.N);
  return r;
}
template <bool KT, int TW>
static __device__ __forceinline__ void rows_ld(const RowsW& W, int grp, int c, int lane, float (&bv)[4][TW]) {
  const int lk = lane >> 4, N = W.N, ldw = W.ldw;
#if defined(TR_KNOB_NOB)   // timing-only builds: no weight loads
  for (int u = 0; u < 4; ++u)
    for (int q = 0; q < TW; ++q) bv[u][q] = 0.001f * (16 * grp + 4 * lk + u + q);
  return;
#endif
  // plain offsets, no per-load bounds arithmetic (per-load masks measured slower): rows past the operand
  // (k >= K, or c >= N for KT) fall past the buffer descriptor's range and read 0; the columns c >= N of a
  // row read the next row's (finite) values, which only reach output columns the epilogue zeroes / never
  // stores, or meet the zero padding of A
  if constexpr (KT) {
#pragma unroll
    for (int q = 0; q < TW; ++q) {
      const f32x4 v = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.d, ((c + q) * ldw + 4 * lk) * 4 + 64 * grp, 0, 0));
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[u][q] = v[u];
    }
  } else {
    // a lane whose columns are all past N (the padding of the last column block) reads nothing: its base
    // offset is pushed past the range (no L2 traffic for the 56 padding columns of a 200-wide layer)
    const int vb = c < N ? (4 * lk * ldw + c) * 4 : (1 << 30);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int off = vb + (16 * grp + u) * ldw * 4;
      if constexpr (TW == 4) {
        const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.d, off, 0, 0));
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[u][q] = v[q];
      } else if constexpr (TW == 2) {
        const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(W.d, off, 0, 0));
        bv[u][0] = v[0];
        bv[u][1] = v[1];
      } else {
        bv[u][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(W.d, off, 0, 0));
      }
    }
  }
}
template <bool KT, int G, int TW>
static __device__ __forceinline__ void rows_pre(const RowsW& W, int c, int lane, float (&pre)[TR_PFM][4][TW]) {
  constexpr int PF = KT ? TR_PF_B : TR_PF;
  if (__builtin_amdgcn_readfirstlane(c - 4 * (lane & 15)) >= W.N) return;   // no columns for this wave (wave-uniform)
#pragma unroll
  for (int grp = 0; grp < PF && grp < G; ++grp) rows_ld<KT, TW>(W, grp, c, lane, pre[grp]);
}
template <bool KT, int G, int TW>
static __device__ __forceinline__ void rows_gemm_pre(const float* As, const RowsW& W, int c, int lane,
                                                     const float (&pre)[TR_PFM][4][TW], f32x4 (&acc)[TW]) {
  constexpr int PF = KT ? TR_PF_B : TR_PF;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = 0; q < TW; ++q) acc[q] = zero4();
  if (__builtin_amdgcn_readfirstlane(c - 4 * li) >= W.N) return;
  float bq[G + PF][4][TW];
#pragma unroll
  for (int grp = 0; grp < PF && grp < G; ++grp)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < TW; ++q) bq[grp][u][q] = pre[grp][u][q];
#pragma unroll
  for (int grp = 0; grp < G; ++grp) {
    if (grp + PF < G) rows_ld<KT, TW>(W, grp + PF, c, lane, bq[grp + PF]);
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 a4 = ld4(As + li * TR_LD + 16 * grp + 4 * lk);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < TW; ++q) {
#if defined(TR_KNOB_NOMFMA)   // timing-only builds: no MFMAs
        acc[q][u] = fmaf(a4[u], bq[grp][u][q], acc[q][u]);
#else
        acc[q] = mfma4(a4[u], bq[grp][u][q], acc[q]);
#endif
      }
  }
}

// a lane's TW consecutive floats at p (16-B / 8-B aligned)
template <int TW>
static __device__ __forceinline__ void st_tw(float* p, const float (&v)[TW]) {
  if constexpr (TW == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else if constexpr (TW == 2) *reinterpret_cast<f32x2*>(p) = f32x2{v[0], v[1]};
  else *p = v[0];
}
template <int TW>
static __device__ __forceinline__ void ld_tw(const float* p, float (&v)[TW]) {
  if constexpr (TW == 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
  } else if constexpr (TW == 1) {
    v[0] = *p;
  } else {
    const f32x2 x = *reinterpret_cast<const f32x2*>(p);
    v[0] = x[0]; v[1] = x[1];
  }
}

// Workgroup b -> (member, row block): workgroups are dealt round-robin over the 8 XCDs (b mod 8), so
// member e's row blocks all get b = e mod 8 (+ 8 per later row block): each member's weights are read
// into ONE XCD's L2 (grid 8 nrb ceil(E / 8); ids past E exit).
static __device__ __forceinline__ bool tr_block(int b, int nrb, int E, int& e, int& rb) {
  const int j = b >> 3;
  e = (b & 7) + 8 * (j / nrb);
  rb = j % nrb;
  return e < E;
}

// ---- output gradient of the Gaussian NLL through the soft log-var bounds, per (row, dim) -----------------
// lv1 = mx - softplus(mx - raw), lv = mn + softplus(lv1 - mn) (bnn.py:669-670); s = 1 / (M D):
// d/dmean = 2 (mean - y) e^-lv s, d/dlv = (1 - (mean - y)^2 e^-lv) s (bnn.py:241-249, 677-701); softplus' =
// sigmoid.  c_mx / c_mn / c_loss: this element's terms of d loss / d maxlv, d loss / d minlv and the loss.
struct NllGrad { float g_mean, g_lv, c_mx, c_mn, c_loss; };
static __device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
// ROUND_Q: err^2 e^-lv is rounded on its own before it is subtracted from 1 (train_rows_kernel) or fused into that
// subtraction (train_loss_kernel).  The two have always differed in this one rounding; each keeps its own, stated
// here so that neither depends on what the compiler would pick.  Where lv is added the product is fused in both.
template <bool ROUND_Q>
static __device__ __forceinline__ NllGrad nll_grad(float mean, float raw, float y, float mx, float mn, float s) {
  const float lv1 = mx - softplusf(mx - raw);
  const float lv = mn + softplusf(lv1 - mn);
  const float inv = expf(-lv);
  const float err = mean - y;
  float dlv;
  if constexpr (ROUND_Q) {
#pragma clang fp contract(off)
    dlv = (1.f - err * err * inv) * s;
  } else {
    dlv = fmaf(-(err * err), inv, 1.f) * s;
  }
  const float sb = sigm(lv1 - mn), sa = sigm(mx - raw);
  const float dlv1 = dlv * sb;
  NllGrad g;
  g.g_mean = 2.f * err * inv * s;
  g.g_lv = dlv1 * sa;
  g.c_mn = dlv * (1.f - sb);
  g.c_mx = dlv1 * (1.f - sa);
  g.c_loss = fmaf(err * err, inv, lv) * s;
  return g;
}

// ---- forward + backward rows in one launch ----------------------------------------------------------
// The forward, the output gradient and the activation-gradient chain in the same workgroup: the
// pre-activations Z stay in LDS (zb, 66 KB; no HBM round trip), the heads' output gradient goes straight into
// the backward's input buffer, and the batch-level tail runs in the weight-gradient launch (train_wgrad.h
// train_loss_tail), which only needs this step's lr_t -- block 0 writes it here (the tail advances the beta
// powers after every reader of them in this step).  The next layer's first weight k-groups are issued before
// this layer's epilogue (rows_pre).
#ifndef MOPO_TRAIN_STAMPS
#define MOPO_TRAIN_STAMPS 0   // diagnostic builds: per-workgroup phase stamps of train_rows_kernel
#endif
#if MOPO_TRAIN_STAMPS
__device__ uint64_t g_train_stamps[2048 * 8];
#endif
// stamp i of this workgroup (wave 0; its lanes all store the same value); v: a value instead of the clock
static __device__ __forceinline__ void tstamp(int i, int64_t v = -1) {
#if MOPO_TRAIN_STAMPS
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0 && blockIdx.x < 2048)
    __hip_atomic_store(&g_train_stamps[blockIdx.x * 8 + i], v < 0 ? __builtin_amdgcn_s_memrealtime() : (uint64_t)v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  (void)i; (void)v;
#endif
}
constexpr int TR_LDS_FLOATS = (2 + TR_NHID) * 16 * TR_LD + 3 * 64 * 17;
template <int G0, int GH, int GD>
static __device__ __forceinline__ void train_rows_body(const TrainRows& a, float* lds, int e, int rb) {
  float (*buf)[16 * TR_LD] = reinterpret_cast<float (*)[16 * TR_LD]>(lds);
  float (*zb)[16 * TR_LD] = reinterpret_cast<float (*)[16 * TR_LD]>(lds + 2 * 16 * TR_LD);
  float (*red)[64][17] = reinterpret_cast<float (*)[64][17]>(lds + (2 + TR_NHID) * 16 * TR_LD);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15;
  const int M = a.M, IN = a.IN, H = a.H, D = a.D, i0 = rb * 16;
  const int c0 = 64 * (w & 3) + 4 * li + TR_TW * (w >> 2);   // this lane's first column
  auto wfwd = [&](int l) {
    const int K = l == 0 ? IN : H, N = l == TR_NHID ? 2 * D : H;
    return rows_w<false>(a.P + a.W[l] + (int64_t)e * K * N, K, N, N);
  };
  auto wbwd = [&](int l) {   // layer l: [H -> Nl], read transposed
    const int Nl = l == TR_NHID ? 2 * D : H;
    return rows_w<true>(a.P + a.W[l] + (int64_t)e * H * Nl, Nl, H, Nl);
  };
  float pre[TR_PFM][4][TR_TW];
  rows_pre<false, G0, TR_TW>(wfwd(0), c0, lane, pre);   // in flight during the gather
  // the next step's rows (staged): two items per thread at most (host: 16 (IN + D) <= 2 TR_WAVES 64)
  constexpr int NPF = 2;
  float pf_v[NPF];
  int pf_src[NPF];
  const bool staged = a.staged;
  if (staged) {   // the indices now; the rows they name after layer 0; the stores at the end
    const int W = IN + D;
    const int64_t nb = (int64_t)(*a.bstep + 1) * a.batch;
    const auto drows = rsrc(reinterpret_cast<const float*>(a.rows), (int64_t)a.E * a.stride);
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int i = tid + q * TR_WAVES * 64, row = i0 + (i / W);
      // past the index array: row 0 (the last full step prefetches for a minibatch that does not come)
      // rows past the member's batch (batch % 16 != 0) are neither loaded nor stored
      pf_src[q] = i < 16 * W && row < M ? __builtin_bit_cast(int, __builtin_amdgcn_raw_buffer_load_b32(
                                              drows, (int)((e * a.stride + nb + row) * 4), 0, 0)) : 0;
    }
  }
  auto prefetch_rows = [&]() {
    if (!staged) return;
    const int W = IN + D;
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int i = tid + q * TR_WAVES * 64, c = i % W;
      const int64_t src = pf_src[q];
      pf_v[q] = i >= 16 * W || i0 + i / W >= M ? 0.f : c < IN ? (a.inputs[src * IN + c] - a.mu[c]) / a.sigma[c]   // utils.py:96
                                           : a.targets[src * D + (c - IN)];
    }
  };
  {  // gather: X rows (scaled) into buf[0] (and HBM, for dW_0), targets into HBM; staged: this step's rows from X
    const int W = IN + D, KP = ((IN + 15) >> 4) << 4;
    const int64_t base = a.bstep ? (int64_t)(*a.bstep) * a.batch : 0;
    for (int i = tid; i < 16 * KP; i += TR_WAVES * 64) buf[0][(i / KP) * TR_LD + i % KP] = 0.f;
    lds_barrier();
    if (staged) {
      for (int i = tid; i < 16 * IN; i += TR_WAVES * 64) {
        const int r = i / IN, c = i % IN;
        if (i0 + r < M) buf[0][r * TR_LD + c] = a.X[((int64_t)e * M + i0 + r) * IN + c];   // padding rows stay 0
      }
    } else
    for (int i = tid; i < 16 * W; i += TR_WAVES * 64) {
      const int r = i / W, c = i % W, row = i0 + r;
      if (row >= M) continue;
      const int64_t src = a.rows ? a.rows[e * a.stride + base + row] : row;
      const int64_t er = (int64_t)e * M + row;
      if (c < IN) {
        const float x = (a.inputs[src * IN + c] - a.mu[c]) / a.sigma[c];   // utils.py:96
        a.X[er * IN + c] = x;
        buf[0][r * TR_LD + c] = x;
      } else {
        a.T[er * D + (c - IN)] = a.targets[src * D + (c - IN)];
      }
    }
    lds_barrier();
  }
  const int lk = lane >> 4;
  auto fwd = [&](auto gtag, int l) {
    constexpr int G = decltype(gtag)::value;
    const int N = l == TR_NHID ? 2 * D : H;
    float bias[TR_TW] = {};
    if (c0 < N) ld_tw<TR_TW>(a.P + a.b[l] + (int64_t)e * N + c0, bias);
    f32x4 acc[TR_TW];
    rows_gemm_pre<false, G, TR_TW>(buf[l & 1], wfwd(l), c0, lane, pre, acc);
    if (l < TR_NHID) rows_pre<false, GH, TR_TW>(wfwd(l + 1), c0, lane, pre);
    else rows_pre<true, GD, TR_TW>(wbwd(TR_NHID), c0, lane, pre);   // the backward's first layer
    float* out = buf[(l + 1) & 1];
    if (__builtin_amdgcn_readfirstlane(c0 - 4 * li) < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lk + i, row = i0 + r;
        const bool ok = row < M && c0 < N;
        float v[TR_TW];
#pragma unroll
        for (int q = 0; q < TR_TW; ++q) v[q] = acc[q][i] + bias[q];
        if (l < TR_NHID) {
          st_tw<TR_TW>(zb[l] + r * TR_LD + c0, v);             // pre-activation, for swish' below
#pragma unroll
          for (int q = 0; q < TR_TW; ++q) v[q] = swish_fast(v[q]);
          if (ok) st_tw<TR_TW>(a.Hh[l] + ((int64_t)e * M + row) * H + c0, v);
        } else if (ok) {
          st_tw<TR_TW>(a.OUT + ((int64_t)e * M + row) * 2 * D + c0, v);
        }
        if (!ok)
#pragma unroll
          for (int q = 0; q < TR_TW; ++q) v[q] = 0.f;
        st_tw<TR_TW>(out + r * TR_LD + c0, v);
      }
    }
    lds_barrier();
  };
  tstamp(1);
  fwd(std::integral_constant<int, G0>{}, 0);
  prefetch_rows();
  tstamp(2);
  for (int l = 1; l <= TR_NHID; ++l) fwd(std::integral_constant<int, GH>{}, l);
  tstamp(3);
  // ---- output gradient (nll_grad) and the block's partial sums; dY of the heads also into buf[0] (the
  //      backward's input; zero-padded to a multiple of 16 columns)
  const float* o = buf[(TR_NHID + 1) & 1];
  float* dy = buf[TR_NHID & 1];
  const int N2 = 2 * D, NP = ((N2 + 15) >> 4) << 4;
  const float s = 1.f / ((float)M * (float)D);
  for (int i = tid; i < 16 * D; i += TR_WAVES * 64) {
    const int r = i / D, d = i % D, row = i0 + r;
    NllGrad g{};   // rows past the batch: zeros
    if (row < M) {
      const int64_t er = (int64_t)e * M + row;
      const float mx = a.P[a.mx + d], mn = a.P[a.mn + d];
      const float mean = o[r * TR_LD + d], raw = o[r * TR_LD + D + d], y = a.T[er * D + d];
      g = nll_grad<true>(mean, raw, y, mx, mn, s);
      a.dOUT[er * 2 * D + d] = g.g_mean;
      a.dOUT[er * 2 * D + D + d] = g.g_lv;
    }
    dy[r * TR_LD + d] = g.g_mean;
    dy[r * TR_LD + D + d] = g.g_lv;
    red[0][d][r] = g.c_mx;
    red[1][d][r] = g.c_mn;
    red[2][d][r] = g.c_loss;
  }
  for (int i = tid; i < 16 * (NP - N2); i += TR_WAVES * 64) dy[(i / (NP - N2)) * TR_LD + N2 + i % (NP - N2)] = 0.f;
  lds_barrier();
  if (tid < D) {                                          // rows in order (deterministic)
    float t3[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      for (int r = 0; r < 16; ++r) t3[k] += red[k][tid][r];
    float* pp = a.lpart + (((int64_t)e * a.nrb + rb) * D + tid) * 4;
    pp[0] = t3[0]; pp[1] = t3[1]; pp[2] = t3[2];
  }
  tstamp(4);
  // ---- the activation-gradient chain dZ_{l-1} = (dY_l W_l^T) * swish'(Z_{l-1}), swish'(Z) from LDS; dY of
  //      layer l sits in buf[(TR_NHID - l) & 1] (dy = buf[TR_NHID & 1] = buf[0] for 4 hidden layers)
  static_assert((TR_NHID & 1) == 0, "the backward's first input buffer is buf[0]");
  auto bwd = [&](auto gtag, int l) {
    constexpr int G = decltype(gtag)::value;
    const int Kl = H;                                    // layer l has Kl inputs: dZ_{l-1} is 16 x Kl
    float zm[4][TR_TW];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int q = 0; q < TR_TW; ++q) zm[i][q] = 0.f;
      if (c0 < Kl) ld_tw<TR_TW>(zb[l - 1] + (4 * lk + i) * TR_LD + c0, zm[i]);
    }
    f32x4 acc[TR_TW];
    rows_gemm_pre<true, G, TR_TW>(buf[(TR_NHID - l) & 1], wbwd(l), c0, lane, pre, acc);
    if (l > 1) rows_pre<true, GH, TR_TW>(wbwd(l - 1), c0, lane, pre);
    float* out = buf[(TR_NHID - l + 1) & 1];
    if (__builtin_amdgcn_readfirstlane(c0 - 4 * li) < Kl) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lk + i, row = i0 + r;
        const bool ok = row < M && c0 < Kl;
        float v[TR_TW];
#pragma unroll
        for (int q = 0; q < TR_TW; ++q) v[q] = ok ? acc[q][i] * dswish_fast(zm[i][q]) : 0.f;
        if (ok) st_tw<TR_TW>(a.dZ[l - 1] + ((int64_t)e * M + row) * H + c0, v);
        st_tw<TR_TW>(out + r * TR_LD + c0, v);
      }
    }
    lds_barrier();
  };
  bwd(std::integral_constant<int, GD>{}, TR_NHID);
  tstamp(5);
  for (int l = TR_NHID - 1; l >= 1; --l) {
    bwd(std::integral_constant<int, GH>{}, l);
    if (l == 2) tstamp(6);
  }
  tstamp(7);
  if (staged) {   // the next step's rows, loaded at the start
    const int W = IN + D;
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int i = tid + q * TR_WAVES * 64, r = i / W, c = i % W;
      const int64_t er = (int64_t)e * M + i0 + r;
      if (i < 16 * W && i0 + r < M) {   // never into the next member's rows (or past the last member's)
        if (c < IN) a.Xn[er * IN + c] = pf_v[q];
        else a.Tn[er * D + (c - IN)] = pf_v[q];
      }
    }
  }
}

template <int G0, int GH, int GD>
static __global__ __launch_bounds__(TR_WAVES * 64, 1) void train_rows_kernel(const TrainRows a) {
  __shared__ __attribute__((aligned(16))) float lds[TR_LDS_FLOATS];
  int e, rb;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float b1p = a.beta_pow[0], b2p = a.beta_pow[1];
    a.beta_pow[2] = a.lr * sqrtf(1.f - b2p) / (1.f - b1p);          // this step's TF1 Adam step size
  }
  if (!tr_block(blockIdx.x, a.nrb, a.E, e, rb)) return;
  tstamp(0);
  train_rows_body<G0, GH, GD>(a, lds, e, rb);
}

}  // namespace mopo
