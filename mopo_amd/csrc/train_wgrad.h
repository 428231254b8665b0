// The weight-gradient launch of the ensemble training step's row path (bnn_train.hip step_rows), which follows
// train_rows_kernel (train_rows.h): every weight gradient dW_l = X_in^T dY (+ db = colsum dY) of every member,
// with weight decay and the TF1 Adam in the tiles' epilogue, and one block that runs the batch-level tail
// (train_loss_tail).  Two forms: train_wgrad2_kernel, persistent and XCD-local (the default), and
// train_wgrad_kernel, one 32 x 32 tile of gemm_group.h per workgroup (MOPO_TRAIN_WG2=0).
#pragma once
#include <algorithm>
#include <vector>

#include "train_rows.h"

namespace mopo {

// the batch-level tail's inputs (train_loss_tail)
struct TrainTail {
  int E, nrb, D;
  const float* lpart;
  int64_t mx, mn;
  float* logs; float* beta_pow; int* bstep_inc; float lr; float* G; AdamCtx ad;
};

// ---- batch-level tail: the (member, row block) partial sums of train_rows_kernel in a fixed order, then the
// batch-level updates as in train_loss_kernel (the 0.01 (sum maxlv - sum minlv) terms, their Adam, the TF1
// beta powers, the minibatch counter)
constexpr int TR_TAIL_CH = 8;     // chunks per output column, at most
constexpr int TR_TAIL_SH = 512;   // floats of sh the tail may use (3 per (chunk, column))
static __device__ __forceinline__ void train_loss_tail(const TrainTail& a, float* sh) {
  const int D = a.D, n = a.E * a.nrb;
  const float b1p = a.beta_pow[0], b2p = a.beta_pow[1];  // every thread reads them before thread 0 advances them
  const float lr_t = a.lr * sqrtf(1.f - b2p) / (1.f - b1p);
  __syncthreads();
  // the E nrb partials of each d in TR_TAIL_CH interleaved chunks (thread (j, d): partials j, j + CH, ...
  // in order, 8 independent loads in flight), then the chunk sums in chunk order: deterministic, and one
  // memory latency instead of E nrb dependent ones (a serial loop made the tail ~30 us)
  const int CH = max(1, min(TR_TAIL_CH, min(TR_TAIL_SH / (3 * D), (int)blockDim.x / D)));
  const int t = threadIdx.x;
  if (t < CH * D) {
    const int dd = t % D, j = t / D;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 8
    for (int c = j; c < n; c += CH) {
      const float* pp = a.lpart + ((int64_t)c * D + dd) * 4;
      s0 += pp[0]; s1 += pp[1]; s2 += pp[2];
    }
    sh[(j * D + dd) * 3 + 0] = s0; sh[(j * D + dd) * 3 + 1] = s1; sh[(j * D + dd) * 3 + 2] = s2;
  }
  __syncthreads();
  float loss = 0.f;
  if (t < D) {
    const int dd = t;
    float gmx = 0.f, gmn = 0.f;
    for (int j = 0; j < CH; ++j) {
      gmx += sh[(j * D + dd) * 3 + 0]; gmn += sh[(j * D + dd) * 3 + 1]; loss += sh[(j * D + dd) * 3 + 2];
    }
    gmx += 0.01f;                                                   // 0.01 * sum(max_logvar)
    gmn -= 0.01f;                                                   // -0.01 * sum(min_logvar)
    a.G[a.mx + dd] = gmx;
    a.G[a.mn + dd] = gmn;
    adam_apply(a.ad, a.mx + dd, gmx, adam_load(a.ad, a.mx + dd), lr_t);
    adam_apply(a.ad, a.mn + dd, gmn, adam_load(a.ad, a.mn + dd), lr_t);
  }
  __syncthreads();                                                  // every chunk sum is read
  if (t < D) sh[t] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float loss = 0.f;
    for (int dd = 0; dd < D; ++dd) loss += sh[dd];
    a.logs[0] = loss;                                               // data term of the train loss
    a.beta_pow[2] = lr_t;
    a.beta_pow[0] = b1p * 0.9f;
    a.beta_pow[1] = b2p * 0.999f;
    if (a.bstep_inc) *a.bstep_inc += 1;
  }
}

constexpr int TRAIN_WG_P = TR_NHID + 1;   // weight-gradient problems of a step (one per layer)
// the tile-per-workgroup form: block 0 the tail, then the problems' 32x32 tiles (gemm32_body)
struct TrainWgrad {
  int n;
  int prefix[TRAIN_WG_P + 1];
  AdamCtx ad;
  GemmProb p[TRAIN_WG_P];
  TrainTail t;
};
static __global__ __launch_bounds__(256, 2) void train_wgrad_kernel(const TrainWgrad g) {
  if (blockIdx.x == 0) {   // dispatched first: its serial chain runs beside the tiles
    __shared__ float sh[TR_TAIL_SH];   // small enough to keep 4 workgroups of the tiles per CU
    train_loss_tail(g.t, sh);
    return;
  }
  gemm32_body(g, (int)blockIdx.x - 1);
}

// ---- the weight-gradient launch, persistent XCD-local form -------------------------------------------
// Every weight gradient dW_l = X_in^T dY (+ db = colsum dY, decay, TF1 Adam) of every member as 32 x 32
// output tiles over the minibatch rows k < M (sac_wgrad.h's tile: 1024 threads, wave w the 16 x 16 quadrant
// w & 3 over the K quarter w >> 2, K in chunks of 256 staged [row][k]).  The tiles are dealt to XCDs on the
// host (make_wlist): member e's tiles go to XCD e mod 8 -- the XCD whose CUs ran its row blocks
// (train_rows.h tr_block), so its X_in / dY panels, parameters and Adam slots are that L2's -- up to an even
// share, the overflow to the least-loaded XCDs.  Each XCD's workgroups walk its list (workgroup j: entries
// j, j + nwx, ...) and load the next tile's panels and Adam inputs into registers while the current tile's
// MFMAs and epilogue run, so a workgroup has two tiles in flight instead of one memory latency per tile.
// The last block runs the batch-level tail (train_loss_tail).
#ifndef TRAIN_WG2_KC
// K rows staged per chunk (LDS: 2 x 32 x (KC + 4) floats per workgroup).  128 (33 KB, 76 VGPRs) lets three
// 512-thread workgroups share a CU instead of two at 256 (66.5 KB, 95 VGPRs): same box, 13.61-13.69k vs
// 13.41-13.45k grad-steps/s (profiles/r05_train_ab_wg2_chunk.txt; four per CU at a 64-VGPR cap spill: 13.4k)
#define TRAIN_WG2_KC 128
#endif
// LDS panels [row][k] of the weight-gradient tiles: k XOR-swizzled by row group ((row >> 2) & 7, in units of
// 4 floats: a b128 read of 4 consecutive k stays contiguous) at a 140-float row stride, so the transposing
// b32 stores (8 rows x 8 k per 32-lane group) hit 32 distinct banks instead of 8 and the b128 MFMA reads
// conflict less (modelled with MI355X_MICROARCH's LDS lane groups: 128 + 320 vs 512 + 256 LDS cycles per chunk)
constexpr int TW2_T = 32, TW2_KC = TRAIN_WG2_KC, TW2_KP = TW2_KC + 12;
static __device__ __forceinline__ int tw2_at(int row, int k) { return row * TW2_KP + (k ^ (((row >> 2) & 7) << 2)); }
struct TrainWg2 {
  int M;                               // minibatch rows per member (the contraction length)
  int nwx, per_x;                      // tile workgroups per XCD; list stride per XCD
  const int32_t* list;                 // [8][per_x]: l | e << 3 | tm << 7 | tn << 12
  const int32_t* cnt;                  // [8] entries per XCD
  const float* A[TR_NHID + 1];         // X_in of layer l, member 0 ([E][M][K_l])
  const float* B[TR_NHID + 1];         // dY of layer l, member 0 ([E][M][N_l])
  int K[TR_NHID + 1], N[TR_NHID + 1];
  int64_t W[TR_NHID + 1], b[TR_NHID + 1];
  float wd[TR_NHID + 1];
  AdamCtx ad;
  TrainTail t;
};

struct Wg2Tile {
  const float* A; const float* B;
  int K, N, i0, j0;
  int64_t w0, b0;                      // parameter index of W(0, 0) / b(0) of the tile's member and layer
  float wd;
  bool cs;                             // tile-row 0: also the bias column sums
  int e, l;                            // member, layer
};

static __device__ __forceinline__ Wg2Tile wg2_tile(const TrainWg2& g, int v) {
  Wg2Tile t;
  const int l = v & 7, e = (v >> 3) & 15, tm = (v >> 7) & 31, tn = (v >> 12) & 31;
  t.K = g.K[l]; t.N = g.N[l];
  t.A = g.A[l] + (int64_t)e * g.M * t.K;
  t.B = g.B[l] + (int64_t)e * g.M * t.N;
  t.i0 = TW2_T * tm; t.j0 = TW2_T * tn;
  t.w0 = g.W[l] + (int64_t)e * t.K * t.N;
  t.b0 = g.b[l] + (int64_t)e * t.N;
  t.wd = g.wd[l];
  t.cs = tm == 0;
  t.e = e; t.l = l;
  return t;
}

// Workgroups of NT threads (512 or 1024): wave w owns quadrant w & 3 of the tile over the K part w >> 2 of
// KW = 256 / (NT / 256) rows.  Thread t stages elements (row 4 (t % 8) + u, k (t / 8) + NT / 8 q), u < 4,
// q < NQ: one b128 load per (operand, q) where the operand's row length is a multiple of 4 floats (b32
// loads otherwise -- the 14 / 23-wide inputs of layer 0).  k >= M read 0 (buffer range); rows past the
// operand's width read the next minibatch row's values, which only reach outputs that are not stored.
template <int NT>
struct Wg2 {
  static constexpr int NQ = TW2_T * TW2_KC / (4 * NT);   // b128 loads per operand and chunk
  static constexpr int NKQ = NT / 256, KW = TW2_KC / NKQ;
  static constexpr int NE = TW2_T * TW2_T / NT;          // output elements per thread
  static constexpr int CT = NT / TW2_T, CK = TW2_KC / CT; // colsum: threads per column, k per thread
};

template <int NT>
static __device__ __forceinline__ void wg2_issue(const Wg2Tile& t, int M, int kc, int tid, f32x4 (&va)[Wg2<NT>::NQ],
                                                 f32x4 (&vb)[Wg2<NT>::NQ]) {
  const auto dA = rsrc(t.A, (int64_t)M * t.K), dB = rsrc(t.B, (int64_t)M * t.N);
  const int r0 = 4 * (tid & 7), k0 = kc + (tid >> 3);
  const bool a4 = (t.K & 3) == 0, b4 = (t.N & 3) == 0;   // wave-uniform
#pragma unroll
  for (int q = 0; q < Wg2<NT>::NQ; ++q) {
    const int k = k0 + (NT / 8) * q;
    const int ia = k * t.K + t.i0 + r0, ib = k * t.N + t.j0 + r0;
    if (a4) va[q] = bload4(dA, ia);
    else va[q] = f32x4{bload(dA, ia), bload(dA, ia + 1), bload(dA, ia + 2), bload(dA, ia + 3)};
    if (b4) vb[q] = bload4(dB, ib);
    else vb[q] = f32x4{bload(dB, ib), bload(dB, ib + 1), bload(dB, ib + 2), bload(dB, ib + 3)};
  }
}

template <int NT>
static __device__ __forceinline__ void wg2_adam_in(const AdamCtx& ad, const Wg2Tile& t, int tid,
                                                   AdamIn (&a)[Wg2<NT>::NE], AdamIn& c) {
#pragma unroll
  for (int h = 0; h < Wg2<NT>::NE; ++h) {
    const int e = tid + NT * h;
    const int gi = min(t.i0 + (e >> 5), t.K - 1), gj = min(t.j0 + (e & 31), t.N - 1);
    const int64_t ix = t.w0 + (int64_t)gi * t.N + gj;
    a[h] = AdamIn{ad.Pc[ix], ad.M[ix], ad.V[ix], 0.f};   // no target copy in training (ad.T == NULL)
  }
  c = AdamIn{0.f, 0.f, 0.f, 0.f};
  if (t.cs && tid % Wg2<NT>::CT == 0) {
    const int64_t ix = t.b0 + min(t.j0 + tid / Wg2<NT>::CT, t.N - 1);
    c = AdamIn{ad.Pc[ix], ad.M[ix], ad.V[ix], 0.f};
  }
}

template <int NT>
// 512 threads: registers capped for 6 waves per SIMD, i.e. three workgroups per CU (the swizzled indexing
// otherwise takes 82 VGPRs: two)
static __global__ __launch_bounds__(NT, NT == 512 ? 6 : NT / 128) void train_wgrad2_kernel(const TrainWg2 g) {
  using C = Wg2<NT>;
  __shared__ __attribute__((aligned(16))) float As[TW2_T * TW2_KP];   // [i][k]; later the K-part partials
  __shared__ __attribute__((aligned(16))) float Bs[TW2_T * TW2_KP];   // [j][k]
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (blockIdx.x == gridDim.x - 1) {   // the batch-level tail
    train_loss_tail(g.t, As);
    return;
  }
  const int x = blockIdx.x & 7, j = blockIdx.x >> 3;   // workgroups are dealt round-robin over the XCDs
  const int cnt = g.cnt[x];
  if (j >= cnt) return;
  const int32_t* lst = g.list + (int64_t)x * g.per_x;
  const int M = g.M;
  const AdamCtx& ad = g.ad;
  const float lr_t = *ad.lr_t;
  const int qd = w & 3, qi = qd >> 1, qj = qd & 1, kq = w >> 2, li = lane & 15, lk = lane >> 4;
  int i = j;
  Wg2Tile cur = wg2_tile(g, __builtin_amdgcn_readfirstlane(lst[i]));
  f32x4 va[C::NQ], vb[C::NQ];
  wg2_issue<NT>(cur, M, 0, tid, va, vb);
  AdamIn a_in[C::NE], c_in;
  wg2_adam_in<NT>(ad, cur, tid, a_in, c_in);
  while (true) {
    const int inx = i + g.nwx;
    const bool has_nx = inx < cnt;
    const Wg2Tile nx = wg2_tile(g, has_nx ? __builtin_amdgcn_readfirstlane(lst[inx]) : 0);
    AdamIn a_nx[C::NE], c_nx{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < C::NE; ++h) a_nx[h] = AdamIn{0.f, 0.f, 0.f, 0.f};
    f32x4 acc0 = zero4(), acc1 = zero4();
    float cs = 0.f;
    for (int kc = 0; kc < M; kc += TW2_KC) {
      // re-derive the thread index here: otherwise the per-thread LDS / buffer offsets are hoisted out of
      // the loops and held in registers across them
      int tt = tid;
      asm volatile("" : "+v"(tt));
      {
        const int r0 = 4 * (tt & 7), k0 = tt >> 3;
#pragma unroll
        for (int q = 0; q < C::NQ; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            As[tw2_at(r0 + u, k0 + (NT / 8) * q)] = va[q][u];
            Bs[tw2_at(r0 + u, k0 + (NT / 8) * q)] = vb[q][u];
          }
      }
      lds_barrier();
      // the next chunk, or the next tile's first chunk and Adam inputs, in flight during this one
      if (kc + TW2_KC < M) {
        wg2_issue<NT>(cur, M, kc + TW2_KC, tt, va, vb);
      } else if (has_nx) {
        wg2_issue<NT>(nx, M, 0, tt, va, vb);
        wg2_adam_in<NT>(ad, nx, tt, a_nx, c_nx);
      }
#pragma unroll
      for (int s = 0; s < C::KW / 16; ++s) {         // k = KW kq + (KW / 4) lk + 4 s + u
        const int k = C::KW * kq + (C::KW / 4) * lk + 4 * s;
        const f32x4 a4 = ld4(As + tw2_at(16 * qi + li, k)), b4 = ld4(Bs + tw2_at(16 * qj + li, k));
        acc0 = mfma4(a4[0], b4[0], acc0);
        acc1 = mfma4(a4[1], b4[1], acc1);
        acc0 = mfma4(a4[2], b4[2], acc0);
        acc1 = mfma4(a4[3], b4[3], acc1);
      }
      if (cur.cs) {                                  // column tid / CT, k = CK (tid % CT) .. + CK - 1
        const int crow = tid / C::CT, ck0 = C::CK * (tid % C::CT);
#pragma unroll
        for (int v = 0; v < C::CK; v += 4) {
          const f32x4 x0 = ld4(Bs + tw2_at(crow, ck0 + v));
          cs += (x0[0] + x0[1]) + (x0[2] + x0[3]);
        }
      }
      lds_barrier();
    }
    // ---- K parts through LDS (As reused), then decay + Adam per element
    float* part = As;
#pragma unroll
    for (int r = 0; r < 4; ++r) part[kq * 1024 + (16 * qi + 4 * lk + r) * 32 + 16 * qj + li] = acc0[r] + acc1[r];
    if (cur.cs) {
#pragma unroll
      for (int off = C::CT / 2; off > 0; off >>= 1) cs += __shfl_xor(cs, off);
    }
    lds_barrier();
#pragma unroll
    for (int h = 0; h < C::NE; ++h) {
      const int e = tid + NT * h;
      float v = part[e];
#pragma unroll
      for (int q = 1; q < C::NKQ; ++q) v += part[1024 * q + e];
      const int gi = cur.i0 + (e >> 5), gj = cur.j0 + (e & 31);
      if (gi < cur.K && gj < cur.N)
        adam_apply(ad, cur.w0 + (int64_t)gi * cur.N + gj, v + cur.wd * a_in[h].p, a_in[h], lr_t);   // fc.py:156-157
    }
    {
      const int cj = cur.j0 + tid / C::CT;
      if (cur.cs && tid % C::CT == 0 && cj < cur.N) adam_apply(ad, cur.b0 + cj, cs, c_in, lr_t);
    }
    if (!has_nx) break;
    lds_barrier();                                   // the partials are read before the next panels land
    i = inx;
    cur = nx;
    for (int h = 0; h < C::NE; ++h) a_in[h] = a_nx[h];
    c_in = c_nx;
  }
}

// tiles of member e to XCD e mod 8 up to ceil(total / 8) per XCD, the rest to the least-loaded XCDs; within
// an XCD in (member, layer TR_NHID .. 0, tile row, tile column) order, so a round's workgroups share panels
// host image: [8][per] tile lists (-1 padded) then the 8 counts; *per = the list stride
static inline std::vector<int32_t> make_wlist(const TrainLayout& L, int* per_out) {
  const int E = L.E;
  std::vector<std::vector<int32_t>> xl(8);
  std::vector<int32_t> over;
  int total = 0;
  for (int l = 0; l <= TR_NHID; ++l) total += E * ceil_div(L.K(l), TW2_T) * ceil_div(L.N(l), TW2_T);
  const int target = ceil_div(total, 8);
  for (int e = 0; e < E; ++e) {
    auto& home = xl[e % 8];
    for (int l = TR_NHID; l >= 0; --l) {
      for (int tm = 0; tm < ceil_div(L.K(l), TW2_T); ++tm)
        for (int tn = 0; tn < ceil_div(L.N(l), TW2_T); ++tn) {
          const int32_t v = l | (e << 3) | (tm << 7) | (tn << 12);
          if ((int)home.size() < target) home.push_back(v);
          else over.push_back(v);
        }
    }
  }
  for (int32_t v : over) {
    int best = 0;
    for (int x = 1; x < 8; ++x)
      if (xl[x].size() < xl[best].size()) best = x;
    xl[best].push_back(v);
  }
  int per = 1;
  for (auto& v : xl) per = std::max(per, (int)v.size());
  std::vector<int32_t> host((size_t)8 * per + 8, -1);
  for (int x = 0; x < 8; ++x) {
    std::copy(xl[x].begin(), xl[x].end(), host.begin() + (size_t)x * per);
    host[(size_t)8 * per + x] = (int32_t)xl[x].size();
  }
  *per_out = per;
  return host;
}

}  // namespace mopo
