// The ensemble's weight-pack kernels and their launchers (declared in internal.h, called by mopo_bnn_set_params in
// bnn_api.hip).  Included by bnn.hip alone: hipcc's module-wide passes give these kernels code that depends on the
// other device functions of their unit, and in the unit of the forward kernels they compile to the code they
// always had (scripts/kernel_code_identity.sh; a unit of their own changed three instructions in four of them).
#pragma once
#include "mlp_tile.h"

#include <algorithm>

namespace mopo {

// ---------------------------------------------------------------------------------------
// weight packing:  src W[E][K][N] (TF layout, x @ W)  ->  fragment-major (see internal.h);
// perm_k / perm_n: that side is a hidden/input width laid out by slot_feat (mlp_tile.h)
__global__ void pack_frags_kernel(const float* __restrict__ src, float* __restrict__ dst, int E, int K,
                                  int N, int KG, int NB, int perm_k, int perm_n) {
  int64_t total = (int64_t)E * KG * NB * 256;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int t = i & 3, lane = (i >> 2) & 63;
    int64_t f = i >> 8;
    int nb = f % NB;
    int kg = (f / NB) % KG;
    int e = f / ((int64_t)NB * KG);
    int k = kg * 16 + 4 * (lane >> 4) + t, n = nb * 16 + (lane & 15);
    if (perm_k) k = slot_feat(k, K);
    if (perm_n == 1) n = slot_feat(n, N);
    else if (perm_n == 2) n = head_col(n, N / 2);  // fused [mean | log-var] head, N = 2D
    dst[i] = (k >= 0 && n >= 0 && k < K && n < N) ? src[((int64_t)e * K + k) * N + n] : 0.f;
  }
}

// bf16 fragments for v_mfma_f32_16x16x32_bf16 (k-group of 32, permuted k order: mlp_tile.h):
// frag (kg, nb), lane l (n = l&15, g = l>>4), element j = W[e][32 kg + bf16_kperm(g, j)][16 nb + n]
// P > 1: fragment (kg, p, nb) holds part p of the split (split_bf16), laid out [e][kg][p][nb].
// mstride: fragments per member in dst (KG P NB; more when the packed remainder follows, pack_frags_kpack_kernel)
template <int P>
__global__ void pack_frags_bf16_kernel(const float* __restrict__ src, short* __restrict__ dst, int E, int K, int N,
                                       int KG, int NB, int perm_k, int perm_n, int64_t mstride) {
  int64_t total = (int64_t)E * KG * P * NB * 512;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int j = i & 7, lane = (i >> 3) & 63;
    int64_t f = i >> 9;
    int nb = f % NB;
    int p = (f / NB) % P;
    int kg = (f / ((int64_t)NB * P)) % KG;
    int e = f / ((int64_t)NB * P * KG);
    int k = kg * 32 + bf16_kperm(lane >> 4, j), n = nb * 16 + (lane & 15);
    if (perm_k) k = slot_feat(k, K);
    if (perm_n == 1) n = slot_feat(n, N);
    else if (perm_n == 2) n = head_col(n, N / 2);
    short parts[P];
    split_bf16<P>((k >= 0 && n >= 0 && k < K && n < N) ? src[((int64_t)e * K + k) * N + n] : 0.f, parts);
    short v = parts[0];
#pragma unroll
    for (int q = 1; q < P; ++q)
      if (q == p) v = parts[q];
    dst[(e * mstride + (int64_t)(kg * P + p) * NB + nb) * 512 + (i & 511)] = v;
  }
}

// The packed remainder k-group (mlp_tile.h kpack_slot) of a K-wide input whose last 32-deep k-group KG - 1 holds 2
// real values per lane: one fragment per output block behind member e's (KG - 1) 3 NB full-depth fragments.
// Element j of lane (g, n) = weight part kpack_slot(j).wp of W[e][slot_feat(32 (KG - 1) + 4 g + kpack_slot(j).k)][n].
__global__ void pack_frags_kpack_kernel(const float* __restrict__ src, short* __restrict__ dst, int E, int K, int N,
                                        int KG, int NB, int perm_n, int64_t mstride) {
  int64_t total = (int64_t)E * NB * 512;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int j = i & 7, lane = (i >> 3) & 63;
    int64_t f = i >> 9;
    int nb = f % NB;
    int e = f / NB;
    const KPackSlot sl = kpack_slot(j);
    int k = slot_feat((KG - 1) * 32 + bf16_kperm(lane >> 4, sl.k), K), n = nb * 16 + (lane & 15);
    if (perm_n == 1) n = slot_feat(n, N);
    else if (perm_n == 2) n = head_col(n, N / 2);
    short parts[3];
    split_bf16<3>((k >= 0 && n >= 0 && k < K && n < N) ? src[((int64_t)e * K + k) * N + n] : 0.f, parts);
    short v = parts[0];
#pragma unroll
    for (int q = 1; q < 3; ++q)
      if (q == sl.wp) v = parts[q];
    dst[(e * mstride + (int64_t)(KG - 1) * 3 * NB + nb) * 512 + (i & 511)] = v;
  }
}

// f16x3 fragments: the bf16 fragment layout with P = 2 fp16 parts of W * 2^k_e (split_f16_scaled);
// scale[e] = 2^k_e puts member e's max |W| of this layer in [2^14, 2^15)
__global__ void pack_frags_f16s_kernel(const float* __restrict__ src, short* __restrict__ dst, int E, int K, int N,
                                       int KG, int NB, int perm_k, int perm_n, const float* __restrict__ scale) {
  constexpr int P = 2;
  int64_t total = (int64_t)E * KG * P * NB * 512;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int j = i & 7, lane = (i >> 3) & 63;
    int64_t f = i >> 9;
    int nb = f % NB;
    int p = (f / NB) % P;
    int kg = (f / ((int64_t)NB * P)) % KG;
    int e = f / ((int64_t)NB * P * KG);
    int k = kg * 32 + bf16_kperm(lane >> 4, j), n = nb * 16 + (lane & 15);
    if (perm_k) k = slot_feat(k, K);
    if (perm_n == 1) n = slot_feat(n, N);
    else if (perm_n == 2) n = head_col(n, N / 2);
    const F16Parts q = split_f16_scaled((k >= 0 && n >= 0 && k < K && n < N) ? src[((int64_t)e * K + k) * N + n] : 0.f,
                                        scale[e]);
    dst[i] = p == 0 ? q.hi : q.lo;
  }
}

// hidden biases in slot order (slot_feat)
// mul: the 16-bit kernels keep their hidden biases pre-multiplied by -log2(e) (see bnn_fwd_f16s_kernel)
__global__ void pack_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int E, int N,
                                 int NP, float mul) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * NP) return;
  int e = i / NP, n = slot_feat(i % NP, N);
  dst[i] = n >= 0 ? src[e * N + n] * mul : 0.f;
}

// ---------------------------------------------------------------------------------------
// launchers: grid-stride kernels over `tot` elements, at most 4096 blocks of 256
static inline dim3 pack_grid(int64_t tot) { return dim3((int)std::min<int64_t>((tot + 255) / 256, 4096)); }

int pack_frags(const float* src, float* dst, int E, int K, int N, int KG, int NB, hipStream_t s, int perm_k,
               int perm_n) {
  hipLaunchKernelGGL(pack_frags_kernel, pack_grid((int64_t)E * KG * NB * 256), dim3(256), 0, s, src, dst, E, K, N, KG, NB,
                     perm_k, perm_n);
  MOPO_HIP(hipGetLastError());
  return 0;
}

int pack_bias(const float* src, float* dst, int E, int N, int NP, float mul, hipStream_t s) {
  hipLaunchKernelGGL(pack_bias_kernel, dim3(ceil_div(E * NP, 256)), dim3(256), 0, s, src, dst, E, N, NP, mul);
  MOPO_HIP(hipGetLastError());
  return 0;
}

int pack_frags16(const float* src, short* dst, int E, int K, int N, int KG, int NB, int perm_n, int P,
                 const float* scale, int64_t mstride, hipStream_t s) {
  const dim3 grid = pack_grid((int64_t)E * KG * P * NB * 512), block(256);
  if (scale) hipLaunchKernelGGL(pack_frags_f16s_kernel, grid, block, 0, s, src, dst, E, K, N, KG, NB, 1, perm_n, scale);
  else if (P == 3) hipLaunchKernelGGL(pack_frags_bf16_kernel<3>, grid, block, 0, s, src, dst, E, K, N, KG, NB, 1, perm_n, mstride);
  else if (P == 2) hipLaunchKernelGGL(pack_frags_bf16_kernel<2>, grid, block, 0, s, src, dst, E, K, N, KG, NB, 1, perm_n, mstride);
  else hipLaunchKernelGGL(pack_frags_bf16_kernel<1>, grid, block, 0, s, src, dst, E, K, N, KG, NB, 1, perm_n, mstride);
  MOPO_HIP(hipGetLastError());
  return 0;
}

int pack_frags_kpack(const float* src, short* dst, int E, int K, int N, int KG, int NB, int perm_n, int64_t mstride,
                     hipStream_t s) {
  hipLaunchKernelGGL(pack_frags_kpack_kernel, pack_grid((int64_t)E * NB * 512), dim3(256), 0, s, src, dst, E, K, N, KG, NB,
                     perm_n, mstride);
  MOPO_HIP(hipGetLastError());
  return 0;
}

}  // namespace mopo
