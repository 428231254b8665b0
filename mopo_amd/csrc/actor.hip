// Squashed-Gaussian policy forward (rollout actions): the weight packers, the launch of the two product widths
// (32 and 256; the kernels are actor_kernels.h's, the other widths run in actor_widths.hip) and the C entry
// points.  The policy changes every SAC step, so its weights are repacked into fragment-major order once per
// rollout (pack_actor, ~0.3 MB) from the SAC parameter buffer.
#include "actor_kernels.h"

namespace mopo {

// packed layout: W1 frags | W2 frags | head frags | b1 [NB*16] | b2 [NB*16] | [bmu | bls] [16]
// (biases zero-padded to whole 16-blocks so the kernel stages them into LDS with global_load_lds)
// f16 (f16x3): W1 [1][2][NB] | W2 [NB/2][2][NB] | head [NB/2][2][1] fragments of 64 lanes x 8 fp16
// (256 floats each, the ensemble's bf16 fragment layout with its k permutation), then the same biases,
// then 3 inverse weight scales (+5 spare floats) and actor_wmax_kernel's WMAX_BLOCKS x 3 partial max-|W|
constexpr int WMAX_BLOCKS = 64;   // actor_wmax_kernel's grid (<= 64: one wave reduces the partials)

// split: 0 f32 fragments, 1 f16x3 (2 scaled fp16 parts), 2 bf16x6 (the exact 3-part bf16 split, no scales):
// W1 [1][3][NB] | W2 [NB/2][3][NB] | head [NB/2][3][1] fragments, then the biases
__host__ __device__ int64_t actor_packed_floats(int O, int Hp, int split) {
  const int KG0 = (O + 15) / 16, NB = actor_kernel_hidden(Hp) / 16;
  if (split == 2) return (int64_t)(3 * NB + 3 * (NB / 2) * NB + 3 * (NB / 2)) * 256 + 2LL * NB * 16 + 16;
  if (split) return (int64_t)(2 * NB + NB * NB + NB) * 256 + 2LL * NB * 16 + 16 + 8 + 3 * WMAX_BLOCKS;
  return (int64_t)KG0 * NB * 256 + (int64_t)NB * NB * 256 + (int64_t)NB * 256 + 2LL * NB * 16 + 16;
}

// max |W| of the three weight matrices (W1, W2, [Wmu | Wls]): block b's maxima -> wpart[3 b + q] (plain
// stores: no zeroing launch before it, no atomics; pack_actor_f16_kernel reduces the WMAX_BLOCKS partials)
__global__ __launch_bounds__(256) void actor_wmax_kernel(const float* __restrict__ P, int O, int A, int Hp,
                                                         float* __restrict__ wpart) {
  __shared__ float sm[4][3];
  const float* W1 = P;
  const float* W2 = W1 + O * Hp + Hp;
  const float* Wm = W2 + Hp * Hp + Hp;
  const float* Wl = Wm + Hp * A + A;
  const int64_t n1 = (int64_t)O * Hp, n2 = (int64_t)Hp * Hp, nh = 2LL * Hp * A;
  float m[3] = {0.f, 0.f, 0.f};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n1 + n2 + nh; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n1) m[0] = fmaxf(m[0], fabsf(W1[i]));
    else if (i < n1 + n2) m[1] = fmaxf(m[1], fabsf(W2[i - n1]));
    else {
      const int64_t j = i - n1 - n2;
      m[2] = fmaxf(m[2], fabsf(j < (int64_t)Hp * A ? Wm[j] : Wl[j - (int64_t)Hp * A]));
    }
  }
  for (int q = 0; q < 3; ++q) {
    float v = m[q];
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3)
    wpart[3 * blockIdx.x + threadIdx.x] =
        fmaxf(fmaxf(sm[0][threadIdx.x], sm[1][threadIdx.x]), fmaxf(sm[2][threadIdx.x], sm[3][threadIdx.x]));
}

// f16x3 packing: fp16 parts of W * 2^k (k per matrix from wmax: max |W| 2^k in [2^14, 2^15)), the
// biases as in the f32 packing, and the 3 inverse scales
__global__ void pack_actor_f16_kernel(const float* __restrict__ P, int O, int A, int Hp, float* __restrict__ dst,
                                      const float* __restrict__ wpart) {
  const int NB = actor_kernel_hidden(Hp) / 16, KG = NB / 2;
  const float* W1 = P;
  const float* W2 = W1 + O * Hp + Hp;
  const float* Wm = W2 + Hp * Hp + Hp;
  const float* Wl = Wm + Hp * A + A;
  __shared__ float smax[3];
  if (threadIdx.x < 64) {   // the max over actor_wmax_kernel's per-block partials (exact in any order)
    float v[3];
    for (int q = 0; q < 3; ++q) v[q] = threadIdx.x < WMAX_BLOCKS ? wpart[3 * threadIdx.x + q] : 0.f;
    for (int q = 0; q < 3; ++q)
      for (int o = 32; o >= 1; o >>= 1) v[q] = fmaxf(v[q], __shfl_xor(v[q], o));
    if (threadIdx.x == 0)
      for (int q = 0; q < 3; ++q) smax[q] = v[q];
  }
  __syncthreads();
  float sc[3], inv[3];
  for (int q = 0; q < 3; ++q) row_scale(smax[q], sc[q], inv[q]);
  const int64_t f1 = 2LL * NB, f2 = (int64_t)KG * 2 * NB, fh = (int64_t)KG * 2;
  const int64_t nfrag = (f1 + f2 + fh) * 512;  // fp16 elements
  short* d16 = reinterpret_cast<short*>(dst);
  float* tail = dst + (f1 + f2 + fh) * 256;
  const int64_t total = nfrag + 2LL * NB * 16 + 16 + 3;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nfrag) {
      const int j = i & 7, lane = (int)((i >> 3) & 63), g = lane >> 4, r = lane & 15;
      int64_t f = i >> 9;
      int which, nbs;
      if (f < f1) { which = 0; nbs = NB; }
      else if (f < f1 + f2) { which = 1; f -= f1; nbs = NB; }
      else { which = 2; f -= f1 + f2; nbs = 1; }
      const int nb = (int)(f % nbs), p = (int)((f / nbs) % 2), kg = (int)(f / (2 * nbs));
      int k = kg * 32 + bf16_kperm(g, j);
      const int n = nb * 16 + r;
      float v = 0.f;
      if (which == 0) {
        k = slot_feat(k, O);
        if (k >= 0 && n < Hp) v = W1[k * Hp + n];
      } else if (which == 1) {
        if (k < Hp && n < Hp) v = W2[k * Hp + n];
      } else if (k < Hp) {
        v = r < A ? Wm[k * A + r] : (r < 2 * A ? Wl[k * A + (r - A)] : 0.f);
      }
      const F16Parts q = split_f16_scaled(v, sc[which]);
      d16[i] = p == 0 ? q.hi : q.lo;
    } else {
      const int j = (int)(i - nfrag);  // b1 | b2 | [bmu | bls] | inverse scales
      float v;
      if (j < NB * 16) v = j < Hp ? W1[O * Hp + j] : 0.f;
      else if (j < 2 * NB * 16) v = j - NB * 16 < Hp ? W2[Hp * Hp + j - NB * 16] : 0.f;
      else if (j < 2 * NB * 16 + 16) {
        const int q = j - 2 * NB * 16;
        v = q < A ? Wm[Hp * A + q] : (q < 2 * A ? Wl[Hp * A + q - A] : 0.f);
      } else {
        v = inv[j - 2 * NB * 16 - 16];
      }
      tail[j] = v;
    }
  }
}

// bf16x6 packing: part p of the exact split (split_bf16<3>) of each weight in the bf16 fragment layout
// (k permutation of the ensemble's), [kg][p][nb] per matrix; the biases as in the f32 packing
__global__ void pack_actor_x6_kernel(const float* __restrict__ P, int O, int A, int Hp, float* __restrict__ dst) {
  constexpr int NP = 3;
  const int NB = actor_kernel_hidden(Hp) / 16, KG = NB / 2;
  const float* W1 = P;
  const float* W2 = W1 + O * Hp + Hp;
  const float* Wm = W2 + Hp * Hp + Hp;
  const float* Wl = Wm + Hp * A + A;
  const int64_t f1 = (int64_t)NP * NB, f2 = (int64_t)KG * NP * NB, fh = (int64_t)KG * NP;
  const int64_t nfrag = (f1 + f2 + fh) * 512;  // bf16 elements
  short* d16 = reinterpret_cast<short*>(dst);
  float* tail = dst + (f1 + f2 + fh) * 256;
  const int64_t total = nfrag + 2LL * NB * 16 + 16;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nfrag) {
      const int j = i & 7, lane = (int)((i >> 3) & 63), g = lane >> 4, r = lane & 15;
      int64_t f = i >> 9;
      int which, nbs;
      if (f < f1) { which = 0; nbs = NB; }
      else if (f < f1 + f2) { which = 1; f -= f1; nbs = NB; }
      else { which = 2; f -= f1 + f2; nbs = 1; }
      const int nb = (int)(f % nbs), p = (int)((f / nbs) % NP), kg = (int)(f / (NP * nbs));
      int k = kg * 32 + bf16_kperm(g, j);
      const int n = nb * 16 + r;
      float v = 0.f;
      if (which == 0) {
        k = slot_feat(k, O);
        if (k >= 0 && n < Hp) v = W1[k * Hp + n];
      } else if (which == 1) {
        if (k < Hp && n < Hp) v = W2[k * Hp + n];
      } else if (k < Hp) {
        v = r < A ? Wm[k * A + r] : (r < 2 * A ? Wl[k * A + (r - A)] : 0.f);
      }
      short parts[NP];
      split_bf16<NP>(v, parts);
      d16[i] = p == 0 ? parts[0] : (p == 1 ? parts[1] : parts[2]);
    } else {
      const int j = (int)(i - nfrag);  // b1 | b2 | [bmu | bls]
      float v;
      if (j < NB * 16) v = j < Hp ? W1[O * Hp + j] : 0.f;
      else if (j < 2 * NB * 16) v = j - NB * 16 < Hp ? W2[Hp * Hp + j - NB * 16] : 0.f;
      else {
        const int q = j - 2 * NB * 16;
        v = q < A ? Wm[Hp * A + q] : (q < 2 * A ? Wl[Hp * A + q - A] : 0.f);
      }
      tail[j] = v;
    }
  }
}

// One launch packs the whole policy (it is repacked at every rollout, after the SAC updates):
// W1 (observation side in slot_feat order), W2, the combined head (n < A -> Wmu[:, n],
// A <= n < 2A -> Wls[:, n - A]) fragment-major (mlp_tile.h), then the zero-padded biases.
__global__ void pack_actor_kernel(const float* __restrict__ P, int O, int A, int Hp, float* __restrict__ dst) {
  const int KG0 = ceil_div(O, 16), NB = actor_kernel_hidden(Hp) / 16;
  const float* W1 = P;
  const float* W2 = W1 + O * Hp + Hp;
  const float* Wm = W2 + Hp * Hp + Hp;
  const float* Wl = Wm + Hp * A + A;
  const int64_t n1 = (int64_t)KG0 * NB * 256, n2 = (int64_t)NB * NB * 256, nh = (int64_t)NB * 256;
  const int64_t total = actor_packed_floats(O, Hp);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = i & 3, lane = (i >> 2) & 63, g = lane >> 4, r = lane & 15;
    float v = 0.f;
    if (i < n1 + n2) {  // trunk layers: fragment f = kg * NB + nb
      const bool l1 = i < n1;
      const int64_t f = (l1 ? i : i - n1) >> 8;
      const int kg = (int)(f / NB), nb = (int)(f % NB);
      int k = kg * 16 + 4 * g + t;
      const int n = nb * 16 + r;
      if (l1) {
        k = slot_feat(k, O);
        if (k >= 0 && n < Hp) v = W1[k * Hp + n];
      } else if (k < Hp && n < Hp) {
        v = W2[k * Hp + n];
      }
    } else if (i < n1 + n2 + nh) {
      const int kg = (int)((i - n1 - n2) >> 8);
      const int k = kg * 16 + 4 * g + t;
      if (k < Hp) v = r < A ? Wm[k * A + r] : (r < 2 * A ? Wl[k * A + (r - A)] : 0.f);
    } else {
      const int j = (int)(i - n1 - n2 - nh);  // b1 | b2 | [bmu | bls]
      if (j < NB * 16) v = j < Hp ? W1[O * Hp + j] : 0.f;
      else if (j < 2 * NB * 16) v = j - NB * 16 < Hp ? W2[Hp * Hp + j - NB * 16] : 0.f;
      else {
        const int q = j - 2 * NB * 16;
        v = q < A ? Wm[Hp * A + q] : (q < 2 * A ? Wl[Hp * A + q - A] : 0.f);
      }
    }
    dst[i] = v;
  }
}

int pack_actor(const float* P, int O, int A, int Hp, float* dst, hipStream_t s, int split) {
  MOPO_REQUIRE(Hp >= 1 && Hp <= 256, "actor: hidden width must be in [1, 256]");
  if (split == 2) {
    MOPO_REQUIRE(O <= 32 && 2 * A <= 16, "actor bf16x6: obs_dim <= 32, act_dim <= 8");
    const int64_t tot = actor_packed_floats(O, Hp, 2) * 2;   // upper bound on the elements the kernel walks
    hipLaunchKernelGGL(pack_actor_x6_kernel, dim3((int)std::min<int64_t>((tot + 255) / 256, 1024)), dim3(256), 0, s,
                       P, O, A, Hp, dst);
    MOPO_HIP(hipGetLastError());
    return 0;
  }
  const int f16 = split;
  if (f16) {
    MOPO_REQUIRE(O <= 32 && 2 * A <= 16, "actor f16x3: obs_dim <= 32, act_dim <= 8");
    const int NB = actor_kernel_hidden(Hp) / 16;
    float* wpart = dst + (2LL * NB + NB * NB + NB) * 256 + 2LL * NB * 16 + 16 + 8;
    hipLaunchKernelGGL(actor_wmax_kernel, dim3(WMAX_BLOCKS), dim3(256), 0, s, P, O, A, Hp, wpart);
    MOPO_HIP(hipGetLastError());
    const int64_t tot = (2LL * NB + NB * NB + NB) * 512 + 2LL * NB * 16 + 16 + 3;
    hipLaunchKernelGGL(pack_actor_f16_kernel, dim3((int)std::min<int64_t>((tot + 255) / 256, 1024)), dim3(256), 0, s,
                       P, O, A, Hp, dst, (const float*)wpart);
    MOPO_HIP(hipGetLastError());
    return 0;
  }
  const int64_t tot = actor_packed_floats(O, Hp);
  hipLaunchKernelGGL(pack_actor_kernel, dim3((int)std::min<int64_t>((tot + 255) / 256, 1024)), dim3(256), 0, s, P, O,
                     A, Hp, dst);
  MOPO_HIP(hipGetLastError());
  return 0;
}

int launch_actor(const ActorArgs& a, hipStream_t s) {
  if (a.B == 0) return 0;
  MOPO_REQUIRE(!a.xs || (a.xs_mu && a.xs_sigma && a.xs_in == a.O + a.A && a.xs_in <= XS_STRIDE),
               "actor: scaled-input rows need the scaler and obs_dim + act_dim <= 32");
  MOPO_REQUIRE(a.A >= 1 && 2 * a.A <= 16, "actor: act_dim must be in [1, 8]");
  MOPO_REQUIRE(a.O >= 1 && a.O <= 32, "actor: obs_dim must be in [1, 32]");
  MOPO_REQUIRE(a.Wpk, "actor: packed weights required");
  MOPO_REQUIRE(a.Hp >= 1 && a.Hp <= 256, "actor: hidden width must be in [1, 256]");
  // every width but the two product ones (32, 256: the kernels below) runs in actor_widths.hip
  if (actor_kernel_hidden(a.Hp) != 256 && actor_kernel_hidden(a.Hp) != 32) return launch_actor_widths(a, s);
  const int Hk = actor_kernel_hidden(a.Hp);
  dim3 grid(ceil_div((int)a.B, 16 * ACT_WAVES)), block(64 * ACT_WAVES);
  if (a.dtype == DT_BF16X6) {
    if (Hk == 256) hipLaunchKernelGGL(actor_x6_kernel<16>, grid, block, 0, s, a);
    else if (Hk == 32) hipLaunchKernelGGL(actor_x6_kernel<2>, grid, block, 0, s, a);
    else return fail("actor bf16x6: unsupported hidden size (256 or 32)");
    MOPO_HIP(hipGetLastError());
    return 0;
  }
  if (a.dtype == DT_F16X3) {
#if ACT_F16_RING
    if (a.alone && Hk == 256) hipLaunchKernelGGL(actor_f16q_kernel<16>, grid, block, 0, s, a);
    else
#endif
    if (Hk == 256) hipLaunchKernelGGL(actor_f16_kernel<16>, grid, block, 0, s, a);
    else if (Hk == 32) hipLaunchKernelGGL(actor_f16_kernel<2>, grid, block, 0, s, a);
    else return fail("actor f16x3: unsupported hidden size (256 or 32)");
    MOPO_HIP(hipGetLastError());
    return 0;
  }
  const int KG0 = ceil_div(a.O, 16);
  if (Hk == 256 && KG0 == 2 && tail_steps(a.O) == 1)  // halfcheetah / walker2d: 17 = 16 + 1
    hipLaunchKernelGGL((actor_kernel<2, 16, 1>), grid, block, 0, s, a);
  else if (Hk == 256 && KG0 == 2)
    hipLaunchKernelGGL((actor_kernel<2, 16>), grid, block, 0, s, a);
  else if (Hk == 256 && KG0 == 1)
    hipLaunchKernelGGL((actor_kernel<1, 16>), grid, block, 0, s, a);
  else if (Hk == 32 && KG0 == 2)
    hipLaunchKernelGGL((actor_kernel<2, 2>), grid, block, 0, s, a);
  else if (Hk == 32 && KG0 == 1)
    hipLaunchKernelGGL((actor_kernel<1, 2>), grid, block, 0, s, a);
  else
    return fail("actor: unsupported hidden size (256 or 32)");
  MOPO_HIP(hipGetLastError());
  return 0;
}

}  // namespace mopo

using namespace mopo;

extern "C" int mopo_actor_device_hidden(int hidden, int dtype) {
  if (hidden < 1 || hidden > 256 || !(dtype == DT_FP32 || dtype == DT_F16X3 || dtype == DT_BF16X6)) return -1;
  return actor_kernel_hidden(hidden);
}

extern "C" int64_t mopo_sac_param_count(int O, int A, int H) {
  int64_t pi = (int64_t)O * H + H + (int64_t)H * H + H + 2 * ((int64_t)H * A + A);
  int64_t q = (int64_t)(O + A) * H + H + (int64_t)H * H + H + H + 1;
  return pi + 2 * q;
}

extern "C" int mopo_actor_forward_dtype(const float* P, int O, int A, int H, const void* obs, int obs_f64, int64_t B,
                                        const float* eps, uint64_t seed, uint32_t step, float* act, float* mu,
                                        int dtype, void* stream) {
  MOPO_REQUIRE(P && obs, "mopo_actor_forward: NULL pointer");
  MOPO_REQUIRE(dtype == DT_FP32 || dtype == DT_F16X3 || dtype == DT_BF16X6,
               "mopo_actor_forward: dtype must be 0 (fp32), 3 (bf16x6) or 4 (f16x3)");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int split = dtype == DT_F16X3 ? 1 : (dtype == DT_BF16X6 ? 2 : 0);
  float* wpk = nullptr;
  MOPO_HIP(hipMallocAsync((void**)&wpk, actor_packed_floats(O, H, split) * sizeof(float), s));
  int rc = pack_actor(P, O, A, H, wpk, s, split);
  if (rc == 0) {
    ActorArgs a{};
    a.P = P; a.Wpk = wpk; a.O = O; a.A = A; a.Hp = H; a.dtype = dtype;
    a.obs = obs; a.obs_f64 = obs_f64; a.B = B;
    a.eps = eps; a.seed = seed; a.step = step;
    a.act = act; a.mu = mu;
    a.stage_base = -1;
    rc = launch_actor(a, s);
  }
  (void)hipFreeAsync(wpk, s);
  return rc;
}

extern "C" int mopo_actor_forward(const float* P, int O, int A, int H, const void* obs, int obs_f64, int64_t B,
                                  const float* eps, uint64_t seed, uint32_t step, float* act, float* mu,
                                  void* stream) {
  return mopo_actor_forward_dtype(P, O, A, H, obs, obs_f64, B, eps, seed, step, act, mu, DT_FP32, stream);
}
