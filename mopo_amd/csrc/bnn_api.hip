// The ensemble's C ABI: create / destroy, set_params (lays out and packs every dtype's fragments on the device
// through the launchers of bnn_pack.h), predict and the packed-parameter copies.  The forward kernels are
// bnn_kernels.h's, dispatched by launch_bnn_fwd (bnn.hip); no kernel is compiled in this unit.
#include "mlp_tile.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace mopo;

// ---------------------------------------------------------------------------------------- C ABI
extern "C" int mopo_bnn_create(mopo_bnn_t* out, int E, int obs_dim, int act_dim, int hidden, int smv,
                               int dtype) {
  MOPO_REQUIRE(out != nullptr, "mopo_bnn_create: out is NULL");
  MOPO_REQUIRE(E >= 1 && E <= 256, "mopo_bnn_create: num_networks must be in [1, 256]");
  // the form that runs this shape (internal.h bnn_forward_form, the one statement of it): input k-groups, the
  // hidden form -- its own where the width has one, else the smallest that holds it -- and the head blocks; the
  // packers fill the form's spare units and head slots with zeros.  A shape no kernel runs is refused here.
  BnnForm f;
  if (const char* why = bnn_forward_form(obs_dim, act_dim, hidden, dtype, &f)) {
    return fail(std::string("mopo_bnn_create: ") + why + " (got obs_dim " + std::to_string(obs_dim) + ", act_dim " +
                std::to_string(act_dim) + ", hidden " + std::to_string(hidden) + ", dtype " + std::to_string(dtype) +
                ")");
  }
  auto h = std::make_unique<Bnn>();   // released to the caller only once every check has passed
  h->E = E; h->O = obs_dim; h->A = act_dim; h->H = hidden; h->smv = smv; h->dtype = dtype;
  BnnDev& d = h->dev;
  d.E = E; d.O = obs_dim; d.A = act_dim; d.IN = obs_dim + act_dim; d.H = hidden; d.D = obs_dim + 1;
  d.KG0 = f.KG0;
  d.NBH = f.NBH;
  d.NBO = f.NBO;
  h->HD = f.HD;
  d.NB2 = (d.NBH + 1) / 2 * 2;
  d.BS = d.NB2 * 16;
  *out = reinterpret_cast<mopo_bnn_t>(h.release());
  return 0;
}

extern "C" int mopo_bnn_forward_form(int obs_dim, int act_dim, int hidden, int dtype, int* blocks4) {
  BnnForm f;
  if (bnn_forward_form(obs_dim, act_dim, hidden, dtype, &f)) return 0;
  if (blocks4) { blocks4[0] = f.KG0; blocks4[1] = f.NBH; blocks4[2] = f.NBO; blocks4[3] = f.wide; }
  return 1;
}

extern "C" int mopo_bnn_device_hidden(int hidden, int dtype, int wide) {
  if (dtype < 0 || dtype > 4) return -1;
  return bnn_device_hidden(hidden, dtype, wide != 0);
}

extern "C" int mopo_bnn_destroy(mopo_bnn_t hh) {
  Bnn* h = reinterpret_cast<Bnn*>(hh);
  if (!h) return 0;
  if (h->buf) (void)hipFree(h->buf);
  if (h->bbuf) (void)hipFree(h->bbuf);
  if (h->pen_buf) (void)hipFree(h->pen_buf);
  delete h;
  return 0;
}

extern "C" int mopo_bnn_set_params(mopo_bnn_t hh, const float* const* arrs, int n) {
  Bnn* h = reinterpret_cast<Bnn*>(hh);
  MOPO_REQUIRE(h != nullptr, "mopo_bnn_set_params: NULL handle");
  MOPO_REQUIRE(n == (h->smv ? 16 : 14), "mopo_bnn_set_params: expected 16 (smv) or 14 arrays (.mat keys)");
  BnnDev& d = h->dev;
  const int E = h->E, IN = d.IN, H = h->H, D = d.D;
  const int KG0 = d.KG0, NBH = d.NBH, NBO = d.NBO;
  const int64_t hp = d.BS;  // bias stride (covers the bf16 path's even block count)
  // sizes (floats) of the packed regions
  const int64_t s_w0 = (int64_t)E * KG0 * NBH * 256, s_wh = 3LL * E * NBH * NBH * 256,
                s_whd = (int64_t)E * NBH * NBO * 256, s_b0 = E * hp, s_bh = 3 * E * hp,
                s_bhd = (int64_t)E * 3 * NBO * 16;
  const int64_t s_ws = (5LL * E + 63) / 64 * 64;  // f16x3 inverse weight scales [5][E]
  const int64_t total = s_w0 + s_wh + s_whd + s_b0 + s_bh + s_bhd + 2 * 64 + 2 * 64 + s_ws;
  if (!h->buf) MOPO_HIP(hipMalloc(&h->buf, total * sizeof(float)));
  h->buf_bytes = total * (int64_t)sizeof(float);
  float* base = h->buf;
  float* w0 = base; float* wh = w0 + s_w0; float* whd = wh + s_wh;
  float* b0 = whd + s_whd; float* bh = b0 + s_b0; float* bhd = bh + s_bh;
  float* mu = bhd + s_bhd; float* sg = mu + 64; float* mx = sg + 64; float* mn = mx + 64;
  float* wsc = mn + 64;

  // stage raw arrays on the device, then pack there (same code path as on-device repacking)
  const int n_layers = 5;
  std::vector<const float*> W(n_layers), Bv(n_layers);
  for (int i = 0; i < n_layers; ++i) { W[i] = arrs[2 + 2 * i]; Bv[i] = arrs[3 + 2 * i]; }
  // combined head raw [E][H][2D] : mean columns then log-var columns
  std::vector<float> head((size_t)E * H * 2 * D), headb((size_t)E * 2 * D);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < H; ++k)
      for (int j = 0; j < 2 * D; ++j) {
        float v;
        if (h->smv) v = j < D ? W[4][((size_t)e * H + k) * D + j] : arrs[12][((size_t)e * H + k) * D + (j - D)];
        else v = W[4][((size_t)e * H + k) * 2 * D + j];
        head[((size_t)e * H + k) * 2 * D + j] = v;
      }
  for (int e = 0; e < E; ++e)
    for (int j = 0; j < 2 * D; ++j)
      headb[(size_t)e * 2 * D + j] = h->smv ? (j < D ? Bv[4][e * D + j] : arrs[13][e * D + (j - D)])
                                            : Bv[4][e * 2 * D + j];
  const float* maxlv = arrs[h->smv ? 14 : 12];
  const float* minlv = arrs[h->smv ? 15 : 13];

  size_t stage_n = std::max((size_t)E * H * H, head.size());
  stage_n = std::max(stage_n, (size_t)E * IN * H);
  float* stage = nullptr;
  MOPO_HIP(hipMalloc(&stage, stage_n * sizeof(float)));
  struct DevFree {  // frees the staging buffers on every return path
    float*& p;
    ~DevFree() { if (p) (void)hipFree(p); }
  } stage_guard{stage};
  auto pack = [&](const float* src, size_t nsrc, float* dst, int K, int N, int KG, int NB, int perm_n) -> int {
    MOPO_HIP(hipMemcpy(stage, src, nsrc * sizeof(float), hipMemcpyHostToDevice));
    if (pack_frags(stage, dst, E, K, N, KG, NB, 0, 1, perm_n)) return -1;
    MOPO_HIP(hipDeviceSynchronize());
    return 0;
  };
  auto packb = [&](const float* src, float* dst, int N, int NP) -> int {
    MOPO_HIP(hipMemcpy(stage, src, (size_t)E * N * sizeof(float), hipMemcpyHostToDevice));
    const float mul = h->dtype != DT_FP32 ? -1.4426950408889634f : 1.f;  // 16-bit kernels: log2 domain
    if (pack_bias(stage, dst, E, N, NP, mul, 0)) return -1;
    MOPO_HIP(hipDeviceSynchronize());
    return 0;
  };
  int rc = pack(W[0], (size_t)E * IN * H, w0, IN, H, KG0, NBH, 1);  // each step runs only if all before succeeded
  if (rc == 0) rc = packb(Bv[0], b0, H, (int)hp);
  for (int l = 0; l < 3 && rc == 0; ++l) {
    rc = pack(W[1 + l], (size_t)E * H * H, wh + (int64_t)l * E * NBH * NBH * 256, H, H, NBH, NBH, 1);
    if (rc == 0) rc = packb(Bv[1 + l], bh + l * E * hp, H, (int)hp);
  }
  if (rc == 0) rc = pack(head.data(), head.size(), whd, H, 2 * D, NBH, NBO, 2);  // head outputs: head_col slots
  if (rc) return rc;
  {  // head aux [E][bias | max_logvar | min_logvar], NBO*16 each, in head_col slot order
    std::vector<float> aux((size_t)s_bhd, 0.f);
    for (int e = 0; e < E; ++e) {
      float* x = aux.data() + (size_t)e * 3 * NBO * 16;
      for (int sl = 0; sl < NBO * 16; ++sl) {
        const int c = head_col(sl, D);
        if (c < 0) continue;
        x[sl] = headb[(size_t)e * 2 * D + c];
        if (c >= D) {
          x[NBO * 16 + sl] = arrs[h->smv ? 14 : 12][c - D];
          x[2 * NBO * 16 + sl] = arrs[h->smv ? 15 : 13][c - D];
        }
      }
    }
    MOPO_HIP(hipMemcpy(bhd, aux.data(), aux.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (h->dtype != 0 && rc == 0) {
    // bf16 fragments: [E][KG0B][P][NB2] | [3][E][KG][P][NB2] | [E][KG][P][NBO], 256 floats (= 512 bf16) each;
    // KG0B = the input's 32-deep k-groups: 1, wide models (KG0 = 4) 2
    const int NB2 = d.NB2, KG = NB2 / 2, P = bf16_parts(h->dtype), KG0B = (KG0 + 1) / 2;
    // bnn_kpack: the hidden-width inputs' last k-group is ONE packed slice behind the KG - 1 full ones' P
    const bool kpack = bnn_kpack(h->dtype, NB2, NBH, h->HD);
    const int64_t SLM = kpack ? (KG - 1) * P + 1 : KG * P;   // slices per member of a hidden-width input
    const int64_t f0 = (int64_t)E * KG0B * P * NB2, fh = 3LL * E * SLM * NB2, fd = (int64_t)E * SLM * NBO;
    if (!h->bbuf) MOPO_HIP(hipMalloc(&h->bbuf, (f0 + fh + fd) * 256 * sizeof(float)));
    h->bbuf_bytes = (f0 + fh + fd) * 256 * (int64_t)sizeof(float);
    float* b0f = reinterpret_cast<float*>(h->bbuf);
    float* bhf = b0f + f0 * 256;
    float* bdf = bhf + fh * 256;
    // f16x3: per layer and member, 2^k with max |W| 2^k in [2^14, 2^15) (mlp_tile.h split_f16_scaled)
    std::vector<float> scale_h(5 * E), inv_h(5 * E, 1.f);
    float* scale_d = nullptr;
    DevFree scale_guard{scale_d};
    if (h->dtype == DT_F16X3) MOPO_HIP(hipMalloc(&scale_d, E * sizeof(float)));
    auto member_scales = [&](const float* src, int K, int N, int layer) {
      for (int e = 0; e < E; ++e) {
        float m = 0.f;
        for (int64_t i = 0; i < (int64_t)K * N; ++i) m = std::max(m, std::fabs(src[(int64_t)e * K * N + i]));
        int ex = 0;
        if (m > 0.f && std::isfinite(m)) std::frexp(m, &ex);  // m in [2^(ex-1), 2^ex)
        const int k = m > 0.f && std::isfinite(m) ? 15 - ex : 0;
        scale_h[layer * E + e] = std::ldexp(1.f, k);
        inv_h[layer * E + e] = std::ldexp(1.f, -k);
      }
    };
    int layer_idx = 0;
    // KGb: the input's 32-deep k-groups; pk: its last one goes out packed (pack_frags_kpack_kernel)
    auto packh = [&](const float* src, size_t nsrc, float* dst, int K, int N, int KGb, int NB, int perm_n,
                     bool pk = false) -> int {
      MOPO_HIP(hipMemcpy(stage, src, nsrc * sizeof(float), hipMemcpyHostToDevice));
      const int64_t mstride = (pk ? SLM : (int64_t)KGb * P) * NB;   // fragments per member
      if (pk) {
        if (pack_frags_kpack(stage, (short*)dst, E, K, N, KGb, NB, perm_n, mstride, 0)) return -1;
        --KGb;   // the full-depth k-groups
      }
      if (h->dtype == DT_F16X3) {
        member_scales(src, K, N, layer_idx);
        MOPO_HIP(hipMemcpy(scale_d, scale_h.data() + layer_idx * E, E * sizeof(float), hipMemcpyHostToDevice));
      }
      if (pack_frags16(stage, (short*)dst, E, K, N, KGb, NB, perm_n, P, h->dtype == DT_F16X3 ? scale_d : nullptr, mstride, 0))
        return -1;
      MOPO_HIP(hipDeviceSynchronize());
      ++layer_idx;
      return 0;
    };
    if (rc == 0) rc = packh(W[0], (size_t)E * IN * H, b0f, IN, H, KG0B, NB2, 1);
    for (int l = 0; l < 3 && rc == 0; ++l)
      rc = packh(W[1 + l], (size_t)E * H * H, bhf + (int64_t)l * E * SLM * NB2 * 256, H, H, KG, NB2, 1, kpack);
    if (rc == 0) rc = packh(head.data(), head.size(), bdf, H, 2 * D, KG, NBO, 2, kpack);
    if (rc == 0 && h->dtype == DT_F16X3)
      rc = hipMemcpy(wsc, inv_h.data(), 5 * E * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0
                                                                                                 : fail("bnn: scale copy");
    d.w0b = b0f; d.whb = bhf; d.whdb = bdf; d.wscale = wsc;
  }
  if (rc) return -1;
  MOPO_HIP(hipMemcpy(mu, arrs[0], IN * sizeof(float), hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(sg, arrs[1], IN * sizeof(float), hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(mx, maxlv, D * sizeof(float), hipMemcpyHostToDevice));
  MOPO_HIP(hipMemcpy(mn, minlv, D * sizeof(float), hipMemcpyHostToDevice));
  d.w0 = w0; d.wh = wh; d.whd = whd; d.b0 = b0; d.bh = bh; d.bhd = bhd;
  d.mu = mu; d.sigma = sg; d.maxlv = mx; d.minlv = mn;
  h->has_params = true;
  return 0;
}

extern "C" int mopo_bnn_predict(mopo_bnn_t hh, const void* x, int x_f64, int64_t B, float* mean,
                                float* var, void* stream) {
  Bnn* h = reinterpret_cast<Bnn*>(hh);
  MOPO_REQUIRE(h != nullptr, "mopo_bnn_predict: NULL handle");
  MOPO_REQUIRE(B >= 0 && B < (1LL << 31) / 32, "mopo_bnn_predict: batch too large");
  if (B == 0) return 0;
  MOPO_REQUIRE(x && mean && var, "mopo_bnn_predict: NULL pointer");
  FwdArgs a{};
  const int IN = h->dev.IN;
  const size_t es = x_f64 ? 8 : 4;
  a.in = FwdIn{x, x_f64, IN, (const char*)x + es * h->O, x_f64, IN};
  a.B = B;
  a.mean = mean;
  a.var = var;
  return launch_bnn_fwd(h, FWD_PREDICT, a, (hipStream_t)stream);
}

extern "C" int64_t mopo_bnn_packed_bytes(mopo_bnn_t hh) {
  const Bnn* h = reinterpret_cast<const Bnn*>(hh);
  if (!h || !h->has_params) return -1;
  return h->buf_bytes + h->bbuf_bytes;
}

extern "C" int mopo_bnn_packed_copy(mopo_bnn_t hh, int to_handle, void* d_buf, int64_t nbytes, void* stream) {
  Bnn* h = reinterpret_cast<Bnn*>(hh);
  MOPO_REQUIRE(h != nullptr, "mopo_bnn_packed_copy: NULL handle");
  MOPO_REQUIRE(h->has_params, "mopo_bnn_packed_copy: parameters not set (the packed layout comes from set_params)");
  MOPO_REQUIRE(d_buf != nullptr && nbytes == h->buf_bytes + h->bbuf_bytes,
               "mopo_bnn_packed_copy: buffer must hold exactly mopo_bnn_packed_bytes() bytes");
  hipStream_t s = (hipStream_t)stream;
  char* b = static_cast<char*>(d_buf);
  if (to_handle) {
    MOPO_HIP(hipMemcpyAsync(h->buf, b, h->buf_bytes, hipMemcpyDeviceToDevice, s));
    if (h->bbuf_bytes) MOPO_HIP(hipMemcpyAsync(h->bbuf, b + h->buf_bytes, h->bbuf_bytes, hipMemcpyDeviceToDevice, s));
  } else {
    MOPO_HIP(hipMemcpyAsync(b, h->buf, h->buf_bytes, hipMemcpyDeviceToDevice, s));
    if (h->bbuf_bytes) MOPO_HIP(hipMemcpyAsync(b + h->buf_bytes, h->bbuf, h->bbuf_bytes, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}
