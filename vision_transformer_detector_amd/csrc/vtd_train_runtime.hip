// Host runtime of the training chains of libvtd.so: vtd_head_backward and
// vtd_encoder_block_backward, each a training forward that keeps what its backward needs and
// then the backward, as one sequence of launches on the caller's stream over a caller
// workspace.  A chain is argument checks, a plan (workspace offsets and the split counts they
// were sized for), a Chain context (vtd_launch.h) and a short sequence of named stages.
#include <algorithm>
#include <cmath>

#include "vtd_launch.h"

namespace vtd {

// ------------------------------------------------------------------ chain context
int Chain::conv_t(const float* src, int K, int N, int Kp, int Np) const {
  return transpose_op_launch(src, K, N, wt, Kp, Np, op, st);
}
int Chain::conv_kn(const float* src, int K, int N, int Kp, int Np) const {
  VTD_HIP(hipMemsetAsync(wkn, 0, (size_t)Kp * m.kk(Np) * 2, st));
  return m.x3 ? split_bf16x3_launch(src, K, N, N, wkn, 3 * Np, 1, st)
              : act_forward_launch(src, K, N, N, VTD_ACT_NONE, wkn, Np, VTD_BF16, st);
}
int Chain::pad_bias(const float* b, int N, int Np) const {
  VTD_HIP(hipMemsetAsync(bias, 0, (size_t)Np * 4, st));
  VTD_HIP(hipMemcpyAsync(bias, b, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  return VTD_OK;
}
int Chain::gemm(int M, int N, int K, const void* A, int lda, const void* Bt, int ks,
                const vtd_epilogue& e, double flops) const {
  return ks > 1 ? gemm_splitk_launch(M, N, K, A, lda, Bt, K, op, &e, part, ks, st, flops)
                : gemm_launch(M, N, K, A, lda, Bt, K, op, &e, st, flops);
}
int Chain::wgrad(int M, int K, int N, const void* X, int ldx, const void* G, int ldg, float* dW,
                 int ldw, float* db, int ms) const {
  return gemm_wgrad_launch(M, K, N, X, ldx, G, ldg, op, dW, ldw, db, part, part_bytes, ms, st);
}

// ------------------------------------------------------------------ dense stages
int Chain::dense_forward(const DenseDims& L, const float* W, const float* b, const void* a_in,
                         int ks, float* z, int act, void* a_out, const DropKey* dk) const {
  if (int rc = conv_t(W, L.kv, L.uv, L.k, L.up)) return rc;
  if (int rc = pad_bias(b, L.uv, L.up)) return rc;
  vtd_epilogue e{};
  e.bias = bias; e.act = VTD_ACT_NONE;
  e.out = z; e.ldo = L.up; e.out_dtype = VTD_F32;
  if (int rc = gemm(L.M, L.up, m.kk(L.k), a_in, m.ka(L.k), wt, ks, e, 2.0 * L.M * L.kv * L.uv))
    return rc;
  if (!a_out) return VTD_OK;
  return act_forward_launch(z, L.M, L.uv, L.up, act, a_out, m.ka(L.up), op, st, dk);
}
int Chain::dense_backward(const DenseDims& L, const float* W, const void* a_in, const float* z,
                          const float* gin, int ldgin, int act, const DropKey* dk, void* gz,
                          float* dW, float* db, int ms, int ks, float* din, int nout) const {
  if (int rc = act_grad_launch(z, L.up, gin, ldgin, L.M, L.uv, act, gz, m.ka(L.up), op, st, dk))
    return rc;
  if (int rc = wgrad(L.M, L.kv, L.uv, a_in, m.ka(L.k), gz, m.ka(L.up), dW, L.uv, db, ms)) return rc;
  if (int rc = conv_kn(W, L.kv, L.uv, L.k, L.up)) return rc;
  vtd_epilogue e{};
  e.act = VTD_ACT_NONE;
  e.out = din; e.ldo = nout; e.out_dtype = VTD_F32;
  return gemm(L.M, nout, m.kk(L.up), gz, m.ka(L.up), wkn, ks, e, 2.0 * L.M * L.kv * L.uv);
}

namespace {

float* f32(char* ws, size_t off) { return reinterpret_cast<float*>(ws + off); }

// ------------------------------------------------------------------ head chain
// Workspace of vtd_head_backward.  wt / wkn / bias / part: the Chain's buffers, each sized for
// its largest use.
struct HeadPlan {
  size_t a_enc, u, z[VTD_MAX_HEAD], a[VTD_MAX_HEAD], logits, gf, gz, da[2], dt, wt, wkn, bias,
      part, part_bytes, total;
  int fwd_ks[VTD_MAX_HEAD];       // split-K of the forward GEMM of head layer j
  int bwd_ks[VTD_MAX_HEAD + 1];   // of the input-gradient GEMM of layer j (n_head: the final one)
  int wg_ms[VTD_MAX_HEAD + 2];    // msplit of the weight gradient: j, n_head = final, n_head + 1 = dense
};
HeadPlan head_plan(const vtd_dims& d, const Mode& m) {
  HeadPlan p{};
  Arena ar;
  const size_t R = (size_t)d.rows, HR = (size_t)d.head_rows, eop = m.eop;
  const int nh = d.n_head, op = m.op;
  size_t wmax = (size_t)64 * d.d_p, umax = std::max(d.tokens_p, 64), part = 0;
  p.a_enc = ar.take(R * d.d_p * eop);
  p.u = ar.take(HR * d.tokens_p * eop);
  for (int j = 0, k = d.tokens_p, kv = d.tokens; j < nh; k = d.head_units_p[j], kv = d.head_units[j], ++j) {
    const int up = d.head_units_p[j];
    p.z[j] = ar.take(HR * up * 4);
    p.a[j] = ar.take(HR * up * eop);
    wmax = std::max(wmax, (size_t)up * k);
    umax = std::max<size_t>(umax, up);
    p.fwd_ks[j] = gemm_splitk_choice((int)HR, up, m.kk(k), op);
    p.bwd_ks[j] = gemm_splitk_choice((int)HR, k, m.kk(up), op);
    p.wg_ms[j] = gemm_wgrad_choice((int)HR, kv, d.head_units[j], op);
    part = std::max(part, (size_t)p.fwd_ks[j] * HR * up * 4);
    part = std::max(part, (size_t)p.bwd_ks[j] * HR * k * 4);
    if (p.wg_ms[j] > 1) part = std::max(part, (size_t)p.wg_ms[j] * (kv + 1) * d.head_units[j] * 4);
  }
  const int kl = nh ? d.head_units_p[nh - 1] : d.tokens_p, klv = nh ? d.head_units[nh - 1] : d.tokens;
  wmax = std::max(wmax, (size_t)64 * kl);
  p.bwd_ks[nh] = gemm_splitk_choice((int)HR, kl, m.kk(64), op);
  p.wg_ms[nh] = gemm_wgrad_choice((int)HR, klv, 6, op);
  p.wg_ms[nh + 1] = gemm_wgrad_choice((int)R, d.d, VTD_MAX_DETECT, op);
  part = std::max(part, (size_t)p.bwd_ks[nh] * HR * kl * 4);
  if (p.wg_ms[nh] > 1) part = std::max(part, (size_t)p.wg_ms[nh] * (klv + 1) * 6 * 4);
  if (p.wg_ms[nh + 1] > 1)
    part = std::max(part, (size_t)p.wg_ms[nh + 1] * (d.d + 1) * VTD_MAX_DETECT * 4);
  p.logits = ar.take(HR * 6 * 4);
  p.gf = ar.take(HR * 64 * eop);
  p.gz = ar.take(HR * umax * eop);
  p.da[0] = ar.take(HR * umax * 4);
  p.da[1] = ar.take(HR * umax * 4);
  p.dt = ar.take(R * 64 * eop);
  p.wt = ar.take(wmax * (m.x3 ? 6 : 2));
  p.wkn = ar.take(wmax * (m.x3 ? 6 : 2));
  p.bias = ar.take(umax * 4);
  p.part_bytes = part;
  p.part = ar.take(part);
  p.total = ar.off;
  return p;
}
int head_mode(const vtd_config* cfg, vtd_dims* d, const char* what) {
  if (int rc = derive(cfg, d)) return rc;
  if (cfg->dtype != VTD_BF16X3 && cfg->dtype != VTD_BF16)
    return fail(VTD_ERR_UNSUPPORTED, std::string(what) + ": cfg->dtype must be VTD_BF16X3 or "
                                     "VTD_BF16 (VTD_F32 and VTD_FP8 have no backward)");
  VTD_CHECK_ARG(d->rows < (int64_t)1 << 31, std::string(what) + ": batch*tokens too large");
  return VTD_OK;
}

// One vtd_head_backward call: the head from `encoded` (vtd.py:454-493) with z and the
// activations kept, then its backward in reverse.  Dropout site j follows head layer j's
// activation, over the unpadded [B 17][units_j] plane; the backward regenerates the masks.
struct HeadChain : Chain {
  vtd_dims d;
  HeadPlan P;
  const vtd_head_params* w;
  const vtd_head_grads* g;
  int batch, act, R, HR, nh;
  DropKey dk[VTD_MAX_HEAD];
  bool drop_on;
  void *a_enc, *u;
  float *logits, *da[2];
  int cur;                 // da[cur] = d loss / d (the activation feeding the layer above)

  // head layer j (j = n_head: the final layer): its input, and as a Dense layer
  const void* ain(int j) const { return j ? ws + P.a[j - 1] : u; }
  int kp(int j) const { return j ? d.head_units_p[j - 1] : d.tokens_p; }
  int kv(int j) const { return j ? d.head_units[j - 1] : d.tokens; }
  DenseDims dims(int j) const { return {HR, kp(j), kv(j), d.head_units_p[j], d.head_units[j]}; }
  const DropKey* drop(int j) const { return drop_on ? &dk[j] : nullptr; }

  int dense17(const float* encoded) {    // Dense(17) + Reshape((17, -1)) as the scatter epilogue
    const int D = d.d, Dp = d.d_p;
    if (int rc = act_forward_launch(encoded, R, D, D, VTD_ACT_NONE, a_enc, m.ka(Dp), op, st))
      return rc;
    if (int rc = conv_t(w->w_det, D, VTD_MAX_DETECT, Dp, 64)) return rc;
    if (int rc = pad_bias(w->b_det, VTD_MAX_DETECT, 64)) return rc;
    VTD_HIP(hipMemsetAsync(u, 0, (size_t)HR * d.tokens_p * m.eop, st));
    vtd_epilogue e{};
    e.bias = bias; e.act = VTD_ACT_NONE;
    e.out = u; e.ldo = m.ka(d.tokens_p); e.out_dtype = op;
    e.scatter_tokens = d.tokens;
    return gemm(R, VTD_MAX_DETECT, m.kk(Dp), a_enc, m.ka(Dp), wt, 1, e,
                2.0 * R * D * VTD_MAX_DETECT);
  }
  int layers() {                         // vtd.py:468-486
    for (int j = 0; j < nh; ++j)
      if (int rc = dense_forward(dims(j), w->w_head[j], w->b_head[j], ain(j), P.fwd_ks[j],
                                 f32(ws, P.z[j]), act, ws + P.a[j], drop(j)))
        return rc;
    return VTD_OK;
  }
  int final_layer() {                    // MLP_Head_no_Sigmoid
    const int k = kp(nh);
    if (int rc = conv_t(w->w_final, kv(nh), 6, k, 64)) return rc;
    if (int rc = pad_bias(w->b_final, 6, 64)) return rc;
    vtd_epilogue e{};
    e.bias = bias; e.act = VTD_ACT_NONE;
    e.out = logits; e.ldo = 6; e.out_dtype = VTD_F32;
    return gemm(HR, 6, m.kk(k), ain(nh), m.ka(k), wt, 1, e, 2.0 * HR * kv(nh) * 6);
  }
  int final_backward(const float* dlogits) {
    const int k = kp(nh);
    void* gf = ws + P.gf;
    if (int rc = act_forward_launch(dlogits, HR, 6, 6, VTD_ACT_NONE, gf, m.ka(64), op, st))
      return rc;
    if (int rc = wgrad(HR, kv(nh), 6, ain(nh), m.ka(k), gf, m.ka(64), g->w_final, 6, g->b_final,
                       P.wg_ms[nh]))
      return rc;
    if (int rc = conv_kn(w->w_final, kv(nh), 6, k, 64)) return rc;
    cur = 0;
    vtd_epilogue e{};
    e.act = VTD_ACT_NONE;
    e.out = da[cur]; e.ldo = k; e.out_dtype = VTD_F32;
    return gemm(HR, k, m.kk(64), gf, m.ka(64), wkn, P.bwd_ks[nh], e, 2.0 * HR * kv(nh) * 6);
  }
  int layers_backward() {
    for (int j = nh - 1; j >= 0; --j, cur ^= 1)
      if (int rc = dense_backward(dims(j), w->w_head[j], ain(j), f32(ws, P.z[j]), da[cur],
                                  d.head_units_p[j], act, drop(j), ws + P.gz, g->w_head[j],
                                  g->b_head[j], P.wg_ms[j], P.bwd_ks[j], da[cur ^ 1], kp(j)))
        return rc;
    return VTD_OK;
  }
  int dense17_backward() {     // da[cur] = dU [B 17][Tp]: back through the Reshape, then Dense(17)
    const int D = d.d, Dp = d.d_p;
    void* dt = ws + P.dt;
    if (int rc = head_unscatter_launch(da[cur], batch, d.tokens, d.tokens_p, dt, m.ka(64), op, st))
      return rc;
    if (int rc = wgrad(R, D, VTD_MAX_DETECT, a_enc, m.ka(Dp), dt, m.ka(64), g->w_det,
                       VTD_MAX_DETECT, g->b_det, P.wg_ms[nh + 1]))
      return rc;
    if (!g->d_encoded) return VTD_OK;
    if (int rc = conv_kn(w->w_det, D, VTD_MAX_DETECT, Dp, 64)) return rc;
    vtd_epilogue e{};
    e.act = VTD_ACT_NONE;
    e.out = g->d_encoded; e.ldo = D; e.out_dtype = VTD_F32;
    return gemm(R, D, m.kk(64), dt, m.ka(64), wkn, 1, e, 2.0 * R * D * VTD_MAX_DETECT);
  }
};

int head_backward(const vtd_config* cfg, const vtd_head_params* w, const float* encoded,
                  const float* dlogits, float* logits_out, const vtd_head_grads* g, void* ws_,
                  size_t ws_bytes, void* stream, const vtd_block_dropout* drop = nullptr) {
  HeadChain h{};
  if (int rc = head_mode(cfg, &h.d, "head_backward")) return rc;
  const int nh = h.nh = h.d.n_head;
  if (drop) {
    VTD_CHECK_ARG((uint64_t)drop->site_base + nh <= 0xffffffffull,
                  "head_backward_dropout: site_base + n_head overflows 32 bits");
    for (int j = 0; j < nh; ++j) {
      const vtd_dropout dj{drop->seed, drop->step, drop->site_base + (uint32_t)j, drop->rate};
      if (int rc = drop_prepare("head_backward_dropout", &dj, &h.dk[j], &h.drop_on)) return rc;
    }
  }
  VTD_CHECK_ARG(w && encoded && ws_ && (dlogits ? g != nullptr : logits_out != nullptr),
                "head_backward: null pointer");
  VTD_CHECK_ARG(w->w_det && w->b_det && w->w_final && w->b_final,
                "head_backward: null weight pointer");
  for (int j = 0; j < nh; ++j)
    VTD_CHECK_ARG(w->w_head[j] && w->b_head[j], "head_backward: null weight pointer");
  if (dlogits) {
    VTD_CHECK_ARG(g->w_det && g->b_det && g->w_final && g->b_final,
                  "head_backward: null gradient pointer");
    for (int j = 0; j < nh; ++j)
      VTD_CHECK_ARG(g->w_head[j] && g->b_head[j], "head_backward: null gradient pointer");
  }
  const Mode m = mode_of(cfg->dtype);
  const HeadPlan& P = h.P = head_plan(h.d, m);
  if (ws_bytes < P.total)
    return fail(VTD_ERR_WORKSPACE, "head_backward: workspace too small (need " +
                                       std::to_string(P.total) + " bytes)");
  char* ws = static_cast<char*>(ws_);
  static_cast<Chain&>(h) = Chain{static_cast<hipStream_t>(stream), ws, m, m.op, f32(ws, P.part),
                                 P.part_bytes, f32(ws, P.bias), ws + P.wt, ws + P.wkn};
  h.w = w; h.g = g; h.batch = cfg->batch; h.R = (int)h.d.rows; h.HR = (int)h.d.head_rows;
  h.act = cfg->use_mish ? VTD_ACT_MISH : VTD_ACT_GELU_TANH;
  h.a_enc = ws + P.a_enc; h.u = ws + P.u;
  h.logits = logits_out ? logits_out : f32(ws, P.logits);
  h.da[0] = f32(ws, P.da[0]); h.da[1] = f32(ws, P.da[1]);
  int rc;
  if ((rc = h.dense17(encoded)) || (rc = h.layers()) || (rc = h.final_layer())) return rc;
  if (!dlogits) return VTD_OK;         // the training forward alone (logits_out)
  if ((rc = h.final_backward(dlogits)) || (rc = h.layers_backward())) return rc;
  return h.dense17_backward();
}

// ------------------------------------------------------------------ encoder block chain
struct BlockShape {
  int64_t rows;
  int B, T, D, Dp, H, kd, dkp, inner, inner_p, qkv_p, q;
  int u[VTD_MAX_MLP], up[VTD_MAX_MLP];
};
int block_shape(const vtd_block_dims* c, BlockShape* s, const char* what) {
  const std::string w(what);
  VTD_CHECK_ARG(c, w + ": null dims");
  VTD_CHECK_ARG(c->batch > 0 && c->tokens > 0 && c->d > 0 && c->num_heads > 0 && c->key_dim > 0 &&
                    c->mlp_quantities > 0,
                w + ": batch, tokens, d, num_heads, key_dim, mlp_quantities must be > 0");
  VTD_CHECK_ARG(c->mlp_quantities <= VTD_MAX_MLP, w + ": mlp_quantities too large");
  VTD_CHECK_ARG(c->key_dim <= 128, w + ": key_dim > 128 not supported");
  if (c->dtype != VTD_BF16X3 && c->dtype != VTD_BF16)
    return fail(VTD_ERR_UNSUPPORTED, w + ": dims->dtype must be VTD_BF16X3 or VTD_BF16 (VTD_F32 "
                                         "and VTD_FP8 have no backward)");
  s->rows = (int64_t)c->batch * c->tokens;
  VTD_CHECK_ARG(s->rows < (int64_t)1 << 31, w + ": batch*tokens too large");
  s->B = c->batch; s->T = c->tokens; s->D = c->d; s->H = c->num_heads; s->kd = c->key_dim;
  s->q = c->mlp_quantities;
  VTD_CHECK_ARG(c->d < (1 << 24) && (int64_t)c->num_heads * 128 * 3 < (1 << 24),
                w + ": d or num_heads too large");
  s->Dp = (int)round_up(s->D, VTD_KALIGN);
  s->dkp = key_dim_pad(s->H, s->kd);
  VTD_CHECK_ARG(s->dkp <= 128, w + ": key_dim padding exceeds 128");
  s->inner = s->H * s->kd;
  s->inner_p = s->H * s->dkp;
  s->qkv_p = (int)round_up(3 * s->inner_p, VTD_KALIGN);
  for (int j = 0; j < VTD_MAX_MLP; ++j) s->u[j] = s->up[j] = 0;
  for (int j = 0; j < s->q; ++j) {
    const int64_t u = mlp_width(s->D, s->q, j);
    VTD_CHECK_ARG(u < (1 << 24), w + ": MLP width overflow");
    s->u[j] = (int)u;
    s->up[j] = (int)round_up(u, VTD_KALIGN);
  }
  return VTD_OK;
}
// Workspace of vtd_encoder_block_backward.  wt / wkn / bias / part: the Chain's buffers, each
// sized for its largest use; ln / att: the LayerNorm and attention backward workspaces.
struct BlockPlan {
  size_t stat1, h1, wt, bias, qkv, attn, lse, x1, stat2, h2, z[VTD_MAX_MLP], a[VTD_MAX_MLP], gz,
      da[2], wkn, dx1, gop, dO, dqkv, dwqkv, dbqkv, dwo, ln, ln_bytes, att, att_bytes, part,
      part_bytes, total;
  int f_qkv, f_out, f_mlp[VTD_MAX_MLP];      // split-K of the forward GEMMs
  int b_mlp[VTD_MAX_MLP], b_out, b_qkv;      // of the input-gradient GEMMs
  int wg_mlp[VTD_MAX_MLP], wg_out, wg_qkv;   // msplit of the weight gradients
};
int block_plan(const BlockShape& s, const Mode& m, int dtype, BlockPlan* out) {
  BlockPlan p{};
  Arena ar;
  const size_t R = (size_t)s.rows, eop = m.eop, es = m.es;
  const int op = m.op, M = (int)s.rows;
  size_t part = 0;
  // split-K needs N % 4 == 0 (its reduce pass reads 16-B vectors).  The count falls back to 1
  // once the rows fill the chip, so the partials are reserved by a bound that only grows with
  // the rows and the workspace stays monotonic in the batch: gemm_splitk_choice gives at most
  // K / 64 / 8 splits, and only below 192 tiles of 256 x 256 with splits x tiles < 448.
  auto ks_of = [&](int N, int K) {
    if (N % 4 != 0) return 1;
    const int ks = gemm_splitk_choice(M, N, K, op);
    const size_t smax = (size_t)(K / 64 / 8);
    if (N > 64 && smax >= 2)
      part = std::max(part, std::min(smax * R * N * 4, (size_t)448 * 256 * 256 * 4));
    if (ks > 1) part = std::max(part, (size_t)ks * R * N * 4);
    return ks;
  };
  auto ms_of = [&](int K, int N) {
    const int ms = gemm_wgrad_choice(M, K, N, op);
    if (ms > 1) part = std::max(part, (size_t)ms * (K + 1) * N * 4);
    return ms;
  };
  size_t wmax = std::max((size_t)s.qkv_p * s.Dp, (size_t)s.Dp * s.inner_p);
  size_t umax = std::max(s.Dp, s.qkv_p);
  for (int j = 0, k = s.Dp; j < s.q; k = s.up[j], ++j) {
    wmax = std::max(wmax, (size_t)s.up[j] * k);
    umax = std::max<size_t>(umax, s.up[j]);
  }
  p.stat1 = ar.take(R * 8);
  p.h1 = ar.take(R * s.Dp * eop);
  p.wt = ar.take(wmax * (m.x3 ? 6 : 2));
  p.bias = ar.take(umax * 4);
  p.qkv = ar.take(R * s.qkv_p * es);
  p.attn = ar.take(R * s.inner_p * eop);
  p.lse = ar.take((size_t)s.B * s.H * s.T * 4);
  p.x1 = ar.take(R * s.D * 4);
  p.stat2 = ar.take(R * 8);
  p.h2 = ar.take(R * s.Dp * eop);
  p.f_qkv = ks_of(s.qkv_p, m.kk(s.Dp));
  p.f_out = ks_of(s.D, m.kk(s.inner_p));
  for (int j = 0, k = s.Dp, kv = s.D; j < s.q; k = s.up[j], kv = s.u[j], ++j) {
    p.z[j] = ar.take(R * s.up[j] * 4);
    p.a[j] = ar.take(j + 1 < s.q ? R * s.up[j] * eop : 0);
    p.f_mlp[j] = ks_of(s.up[j], m.kk(k));
    p.b_mlp[j] = ks_of(j ? k : s.D, m.kk(s.up[j]));
    p.wg_mlp[j] = ms_of(kv, s.u[j]);
  }
  p.b_out = ks_of(s.inner_p, m.kk(s.Dp));
  p.b_qkv = ks_of(s.D, m.kk(s.qkv_p));
  p.wg_out = ms_of(s.inner_p, s.D);
  p.wg_qkv = ms_of(s.D, s.qkv_p);
  p.gz = ar.take(R * umax * eop);
  p.da[0] = ar.take(R * umax * 4);
  p.da[1] = ar.take(R * umax * 4);
  p.wkn = ar.take(wmax * (m.x3 ? 6 : 2));
  p.dx1 = ar.take(R * s.D * 4);
  p.gop = ar.take(R * s.Dp * eop);
  p.dO = ar.take(R * s.inner_p * es);
  p.dqkv = ar.take(R * s.qkv_p * eop);
  p.dwqkv = ar.take((size_t)s.D * s.qkv_p * 4);
  p.dbqkv = ar.take((size_t)s.qkv_p * 4);
  p.dwo = ar.take((size_t)s.inner_p * s.D * 4);
  if (int rc = layernorm_backward_workspace_bytes(s.rows, s.D, &p.ln_bytes)) return rc;
  p.ln = ar.take(p.ln_bytes);
  if (int rc = attention_backward_workspace_bytes(s.B, s.T, s.H, s.dkp, dtype, &p.att_bytes))
    return rc;
  p.att = ar.take(p.att_bytes);
  p.part_bytes = part;
  p.part = ar.take(part);
  p.total = ar.off;
  *out = p;
  return VTD_OK;
}

// One vtd_encoder_block_backward call: one encoder block (vtd.py:350-412) with every
// pre-activation kept, then its backward.  Dropout sites: site_base the attention
// probabilities, site_base + 1 + j MLP layer j; the backward regenerates the forward's masks
// from the same (seed, step, site).
struct BlockChain : Chain {
  BlockShape s;
  BlockPlan P;
  const vtd_block_params* w;
  const vtd_block_grads* g;
  const float *x, *dy;
  int dtype, act, R;
  int adt;                 // what the attention kernels read (qkv, dO): bf16, or f32 in VTD_BF16X3
  float scale;
  DropKey dk_att, dk_mlp[VTD_MAX_MLP];
  bool drop_on;
  float *stat1, *stat2, *x1, *lse, *dx1, *da[2];
  void *h1, *h2, *qkv, *attn, *dqkv;
  const float* gin;        // d loss / d (what feeds the stage above), ldgin wide; da[cur] is free
  int ldgin, cur;
  // the fused, per-head padded query/key/value matrix [Dp][qkv_p], its bias, and
  // attention_output [inner_p][Dp] (BlockGather, vtd_launch.h)
  BlockGather gq, gqb, go;

  // MLP layer j: its input, as a Dense layer, its pre-activation; dropout site (-1: attention)
  const void* ain(int j) const { return j ? ws + P.a[j - 1] : h2; }
  DenseDims dims(int j) const {
    return {R, j ? s.up[j - 1] : s.Dp, j ? s.u[j - 1] : s.D, s.up[j], s.u[j]};
  }
  float* z(int j) const { return f32(ws, P.z[j]); }
  const DropKey* drop(int j) const { return drop_on ? (j < 0 ? &dk_att : &dk_mlp[j]) : nullptr; }

  int layernorm(const float* in, const float* gamma, const float* beta, float* stat, void* h) {
    if (int rc = ln_stats_launch(in, VTD_F32, R, s.D, s.D, 1e-3f, stat, st)) return rc;
    return layernorm_launch(in, VTD_F32, R, s.D, s.D, gamma, beta, 1e-3f, h, m.ka(s.Dp), op, st);
  }
  int qkv_proj() {                       // query / key / value, one fused GEMM
    if (int rc = block_gather_launch(gq, wt, nullptr, op, st)) return rc;
    if (int rc = block_gather_bias_launch(gqb, bias, st)) return rc;
    vtd_epilogue e{};
    e.bias = bias; e.act = VTD_ACT_NONE;
    e.out = qkv; e.ldo = s.qkv_p; e.out_dtype = adt;
    return gemm(R, s.qkv_p, m.kk(s.Dp), h1, m.ka(s.Dp), wt, P.f_qkv, e,
                2.0 * R * s.D * 3.0 * s.inner);
  }
  int attention() {
    return attention_train_launch(qkv, s.B, s.T, s.H, s.dkp, s.qkv_p, scale, attn, m.ka(s.inner_p),
                                  lse, dtype, st, drop(-1));
  }
  int out_proj() {                       // x1 = x + O Wo + bo
    if (int rc = block_gather_launch(go, wt, nullptr, op, st)) return rc;
    vtd_epilogue e{};
    e.bias = w->bo; e.act = VTD_ACT_NONE;
    e.resid = x; e.ldr = s.D;
    e.out = x1; e.ldo = s.D; e.out_dtype = VTD_F32;
    return gemm(R, s.D, m.kk(s.inner_p), attn, m.ka(s.inner_p), wt, P.f_out, e,
                2.0 * R * s.inner * s.D);
  }
  int mlp() {                            // the last layer's activation is resid_act's
    for (int j = 0; j < s.q; ++j)
      if (int rc = dense_forward(dims(j), w->w_mlp[j], w->b_mlp[j], ain(j), P.f_mlp[j], z(j), act,
                                 j + 1 < s.q ? ws + P.a[j] : nullptr, drop(j)))
        return rc;
    return VTD_OK;
  }
  int resid_act(float* y) {
    return block_resid_act_launch(x1, s.D, z(s.q - 1), s.up[s.q - 1], R, s.D, act, y, s.D, st,
                                  drop(s.q - 1));
  }
  // 1. the MLP.  The block's own width leaves unpadded: LayerNorm reads it
  int mlp_backward() {
    gin = dy; ldgin = s.D; cur = 0;
    for (int j = s.q - 1; j >= 0; --j, cur ^= 1) {
      const int nout = j ? s.up[j - 1] : s.D;
      if (int rc = dense_backward(dims(j), w->w_mlp[j], ain(j), z(j), gin, ldgin, act, drop(j),
                                  ws + P.gz, g->w_mlp[j], g->b_mlp[j], P.wg_mlp[j], P.b_mlp[j],
                                  da[cur], nout))
        return rc;
      gin = da[cur]; ldgin = nout;
    }
    return VTD_OK;
  }
  // 2. LayerNorm 2; the residual's gradient dy joins as `add`
  int ln2_backward() {
    return layernorm_backward_launch(x1, s.D, stat2, w->ln2_gamma, gin, s.D, dy, s.D, R, s.D, dx1,
                                     s.D, g->ln2_gamma, g->ln2_beta, ws + P.ln, P.ln_bytes, st);
  }
  // 3. attention_output
  int out_proj_backward() {
    void* gop = ws + P.gop;
    float* dwo = f32(ws, P.dwo);
    if (int rc = act_forward_launch(dx1, R, s.D, s.D, VTD_ACT_NONE, gop, m.ka(s.Dp), op, st))
      return rc;
    if (int rc = wgrad(R, s.inner_p, s.D, attn, m.ka(s.inner_p), gop, m.ka(s.Dp), dwo, s.D, g->bo,
                       P.wg_out))
      return rc;
    float* const dst[1] = {g->wo};
    if (int rc = block_ungather_launch(go, dst, nullptr, dwo, s.D, nullptr, st)) return rc;
    if (int rc = block_gather_launch(go, nullptr, wkn, op, st)) return rc;
    vtd_epilogue e{};                    // the pad rows of wkn are zero: so are dO's pad columns
    e.act = VTD_ACT_NONE;
    e.out = ws + P.dO; e.ldo = s.inner_p; e.out_dtype = adt;
    return gemm(R, s.inner_p, m.kk(s.Dp), gop, m.ka(s.Dp), wkn, P.b_out, e,
                2.0 * R * s.inner * s.D);
  }
  // 4. the attention core
  int attention_backward() {
    return attention_backward_launch(qkv, attn, ws + P.dO, lse, s.B, s.T, s.H, s.dkp, s.qkv_p,
                                     m.ka(s.inner_p), s.inner_p, scale, dqkv, m.ka(s.qkv_p), dtype,
                                     ws + P.att, P.att_bytes, st, drop(-1));
  }
  // 5. query / key / value
  int qkv_backward() {
    float *dwqkv = f32(ws, P.dwqkv), *dbqkv = f32(ws, P.dbqkv);
    if (int rc = wgrad(R, s.D, s.qkv_p, h1, m.ka(s.Dp), dqkv, m.ka(s.qkv_p), dwqkv, s.qkv_p, dbqkv,
                       P.wg_qkv))
      return rc;
    float* const dst[3] = {g->wq, g->wk, g->wv};
    float* const dstb[3] = {g->bq, g->bk, g->bv};
    if (int rc = block_ungather_launch(gq, dst, dstb, dwqkv, s.qkv_p, dbqkv, st)) return rc;
    if (int rc = block_gather_launch(gq, nullptr, wkn, op, st)) return rc;
    vtd_epilogue e{};
    e.act = VTD_ACT_NONE;
    e.out = da[cur]; e.ldo = s.D; e.out_dtype = VTD_F32;
    return gemm(R, s.D, m.kk(s.qkv_p), dqkv, m.ka(s.qkv_p), wkn, P.b_qkv, e,
                2.0 * R * s.D * 3.0 * s.inner);
  }
  // 6. LayerNorm 1; dx1 joins along the residual.  Without a dx output the row pass still runs
  // for dgamma / dbeta and writes in place over dx1
  int ln1_backward() {
    return layernorm_backward_launch(x, s.D, stat1, w->ln1_gamma, da[cur], s.D, dx1, s.D, R, s.D,
                                     g->dx ? g->dx : dx1, s.D, g->ln1_gamma, g->ln1_beta,
                                     ws + P.ln, P.ln_bytes, st);
  }
};

int encoder_block_backward(const vtd_block_dims* c, const vtd_block_params* w, const float* x,
                           const float* dy, float* y, const vtd_block_grads* g, void* ws_,
                           size_t ws_bytes, void* stream,
                           const vtd_block_dropout* drop = nullptr) {
  BlockChain b{};
  BlockShape& s = b.s;
  if (int rc = block_shape(c, &s, "encoder_block_backward")) return rc;
  if (drop) {
    VTD_CHECK_ARG((uint64_t)drop->site_base + s.q <= 0xffffffffull,
                  "encoder_block_backward_dropout: site_base + mlp_quantities overflows 32 bits");
    for (int j = -1; j < s.q; ++j) {
      const vtd_dropout d{drop->seed, drop->step, drop->site_base + (uint32_t)(1 + j), drop->rate};
      if (int rc = drop_prepare("encoder_block_backward_dropout", &d,
                                j < 0 ? &b.dk_att : &b.dk_mlp[j], &b.drop_on))
        return rc;
    }
  }
  VTD_CHECK_ARG(w && x && ws_ && (dy ? g != nullptr : y != nullptr),
                "encoder_block_backward: null pointer");
  VTD_CHECK_ARG(w->ln1_gamma && w->ln1_beta && w->wq && w->bq && w->wk && w->bk && w->wv && w->bv &&
                    w->wo && w->bo && w->ln2_gamma && w->ln2_beta,
                "encoder_block_backward: null weight pointer");
  for (int j = 0; j < s.q; ++j)
    VTD_CHECK_ARG(w->w_mlp[j] && w->b_mlp[j], "encoder_block_backward: null weight pointer");
  if (dy) {
    VTD_CHECK_ARG(g->ln1_gamma && g->ln1_beta && g->wq && g->bq && g->wk && g->bk && g->wv &&
                      g->bv && g->wo && g->bo && g->ln2_gamma && g->ln2_beta,
                  "encoder_block_backward: null gradient pointer");
    for (int j = 0; j < s.q; ++j)
      VTD_CHECK_ARG(g->w_mlp[j] && g->b_mlp[j], "encoder_block_backward: null gradient pointer");
  }
  const Mode m = mode_of(c->dtype);
  BlockPlan& P = b.P;
  if (int rc = block_plan(s, m, c->dtype, &P)) return rc;
  if (ws_bytes < P.total)
    return fail(VTD_ERR_WORKSPACE, "encoder_block_backward: workspace too small (need " +
                                       std::to_string(P.total) + " bytes)");
  char* ws = static_cast<char*>(ws_);
  static_cast<Chain&>(b) = Chain{static_cast<hipStream_t>(stream), ws, m, m.op, f32(ws, P.part),
                                 P.part_bytes, f32(ws, P.bias), ws + P.wt, ws + P.wkn};
  b.w = w; b.g = g; b.x = x; b.dy = dy; b.dtype = c->dtype; b.R = (int)s.rows;
  b.act = c->use_mish ? VTD_ACT_MISH : VTD_ACT_GELU_TANH;
  b.adt = m.x3 ? VTD_F32 : VTD_BF16;
  b.scale = 1.0f / std::sqrt((float)s.kd);
  b.stat1 = f32(ws, P.stat1); b.stat2 = f32(ws, P.stat2); b.x1 = f32(ws, P.x1);
  b.lse = f32(ws, P.lse); b.dx1 = f32(ws, P.dx1);
  b.da[0] = f32(ws, P.da[0]); b.da[1] = f32(ws, P.da[1]);
  b.h1 = ws + P.h1; b.h2 = ws + P.h2; b.qkv = ws + P.qkv; b.attn = ws + P.attn;
  b.dqkv = ws + P.dqkv;
  const int D = s.D, Dp = s.Dp;
  b.gq = BlockGather{{w->wq, w->wk, w->wv}, 3, D, s.inner, D, Dp, s.kd, s.dkp, s.inner_p, Dp,
                     s.qkv_p};
  b.gqb = BlockGather{{w->bq, w->bk, w->bv}, 3, 1, s.inner, 1, 1, s.kd, s.dkp, s.inner_p, 1,
                      s.qkv_p};
  b.go = BlockGather{{w->wo, nullptr, nullptr}, 1, s.inner, D, s.kd, s.dkp, D, Dp, Dp, s.inner_p,
                     Dp};
  int rc;
  if ((rc = b.layernorm(x, w->ln1_gamma, w->ln1_beta, b.stat1, b.h1)) || (rc = b.qkv_proj()) ||
      (rc = b.attention()) || (rc = b.out_proj()) ||
      (rc = b.layernorm(b.x1, w->ln2_gamma, w->ln2_beta, b.stat2, b.h2)) || (rc = b.mlp()) ||
      (y && (rc = b.resid_act(y))))
    return rc;
  if (!dy) return VTD_OK;              // the training forward alone (y_dev)
  if ((rc = b.mlp_backward()) || (rc = b.ln2_backward()) || (rc = b.out_proj_backward()) ||
      (rc = b.attention_backward()) || (rc = b.qkv_backward()))
    return rc;
  return b.ln1_backward();
}

}  // namespace

}  // namespace vtd

using namespace vtd;

extern "C" {

int vtd_head_backward_workspace_bytes(const vtd_config* cfg, size_t* bytes) {
  VTD_CHECK_ARG(bytes, "null bytes pointer");
  vtd_dims d;
  if (int rc = head_mode(cfg, &d, "head_backward_workspace_bytes")) return rc;
  *bytes = head_plan(d, mode_of(cfg->dtype)).total;
  return VTD_OK;
}

int vtd_head_backward(const vtd_config* cfg, const vtd_head_params* w, const float* encoded_dev,
                      const float* dlogits_dev, float* logits_dev, const vtd_head_grads* g,
                      void* ws, size_t ws_bytes, void* stream) {
  return head_backward(cfg, w, encoded_dev, dlogits_dev, logits_dev, g, ws, ws_bytes, stream);
}

int vtd_head_backward_dropout(const vtd_config* cfg, const vtd_head_params* w,
                              const float* encoded_dev, const float* dlogits_dev,
                              float* logits_dev, const vtd_head_grads* g, void* ws,
                              size_t ws_bytes, void* stream, const vtd_block_dropout* drop) {
  VTD_CHECK_ARG(drop, "head_backward_dropout: null dropout description");
  return head_backward(cfg, w, encoded_dev, dlogits_dev, logits_dev, g, ws, ws_bytes, stream,
                       drop);
}

int vtd_encoder_block_backward_workspace_bytes(const vtd_block_dims* dims, size_t* bytes) {
  VTD_CHECK_ARG(bytes, "null bytes pointer");
  BlockShape s;
  if (int rc = block_shape(dims, &s, "encoder_block_backward_workspace_bytes")) return rc;
  BlockPlan P;
  if (int rc = block_plan(s, mode_of(dims->dtype), dims->dtype, &P)) return rc;
  *bytes = P.total;
  return VTD_OK;
}

int vtd_encoder_block_backward(const vtd_block_dims* dims, const vtd_block_params* params,
                               const float* x_dev, const float* dy_dev, float* y_dev,
                               const vtd_block_grads* grads, void* ws, size_t ws_bytes,
                               void* stream) {
  return encoder_block_backward(dims, params, x_dev, dy_dev, y_dev, grads, ws, ws_bytes, stream);
}

int vtd_encoder_block_backward_dropout(const vtd_block_dims* dims, const vtd_block_params* params,
                                       const float* x_dev, const float* dy_dev, float* y_dev,
                                       const vtd_block_grads* grads, void* ws, size_t ws_bytes,
                                       void* stream, const vtd_block_dropout* drop) {
  VTD_CHECK_ARG(drop, "encoder_block_backward_dropout: null dropout description");
  return encoder_block_backward(dims, params, x_dev, dy_dev, y_dev, grads, ws, ws_bytes, stream,
                                drop);
}

}  // extern "C"
