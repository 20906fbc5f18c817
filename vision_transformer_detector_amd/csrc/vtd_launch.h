// The host launchers that one .hip file defines and another calls, declared once: every
// file that defines or calls one includes this header, so a definition is checked against
// its declaration.  Default arguments live here only.
#pragma once

#include "vtd_common.h"
#include "vtd_philox.h"

namespace vtd {

// ----------------------------------------------------------------- vtd_runtime.hip
// What a vtd_config.dtype means for the buffers and GEMMs of the forward and the training chains.
struct Mode {
  // activation / non-MX matrix dtype (VTD_FP8 keeps everything else in bf16; the split-bf16
  // mode VTD_BF16X3 keeps its activations -- query/key/value, attention -- in f32)
  int act;
  // GEMM operand dtype.  VTD_BF16X3: every GEMM runs on split-bf16 operands (bf16 kernels over
  // K' = 3 K_p, A rows stored [hi | lo], 2 K_p wide), which the producers write directly
  int op;
  // dtype of the residual stream x: bf16 in the bf16 / fp8 modes (the stream the GEMM
  // epilogues add into and the LayerNorms read), f32 in the f32 mode.  VTD_RESID_F32=1
  // keeps an f32 stream in the bf16 modes (A/B diagnostic; costs ~7 % at C2).
  int resid;
  // bytes per element of an activation (es) and per logical element of a GEMM A operand --
  // patches, LayerNorm out, MLP / head activations (eop; VTD_BF16X3: the pieces [hi | lo])
  size_t es, eop;
  bool fp8, x3;
  // stored width of a K-wide logical A row, and the GEMM's K (the weights' row width) for it
  int ka(int k) const { return x3 ? 2 * k : k; }
  int kk(int k) const { return x3 ? 3 * k : k; }
};
Mode mode_of(int dtype);
int derive(const vtd_config* c, vtd_dims* d);      // vtd_derive_dims
// encoder_key_dim as the attention kernels take it: 32 / 64 / 128, doubled where heads x that is
// no multiple of VTD_KALIGN (a result above 128 has no kernel: the callers reject it)
inline int key_dim_pad(int heads, int key_dim) {
  const int dkp = key_dim <= 32 ? 32 : (key_dim <= 64 ? 64 : 128);
  return (heads * dkp) % VTD_KALIGN ? 2 * dkp : dkp;
}
// units of encoder MLP layer j of q, vtd.py:385-386 (the callers bound it below 2^24)
inline int64_t mlp_width(int d, int q, int j) { return (int64_t)d << (q - 1 - j); }
// workspace offsets: buffers in take() order, each 256-B aligned; `off` ends as the total
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  }
};

// ----------------------------------------------------------------- vtd_train_runtime.hip
// One Dense layer of a training chain: M rows, kv inputs (stored k wide), uv units (stored up)
struct DenseDims {
  int M, k, kv, up, uv;
};
// The training twin of the forward's Part: what the launches of one training chain
// (vtd_head_backward, vtd_encoder_block_backward, vtd_stem_backward) share.  One stream, so the
// order of the launches is the order of use: the converted weights (wt: W^T for a forward GEMM,
// wkn: the Keras [K][N] form for an input-gradient GEMM), the padded bias and the split-K /
// msplit partials (`part`) are one buffer each, reused launch after launch.
struct Chain {
  hipStream_t st;
  char* ws;                  // workspace base
  Mode m;
  int op;                    // m.op
  float* part;
  size_t part_bytes;
  float* bias;
  void *wt, *wkn;
  // Keras kernel [K][N] -> wt = W^T [Np][kk(Kp)] in the operand dtype, pad rows and columns zero
  int conv_t(const float* src, int K, int N, int Kp, int Np) const;
  // Keras kernel [K][N] -> wkn = [Kp][kk(Np)] in the operand dtype (Bt of dA = dZ W^T): the rows
  // as stored, pad rows and columns zero
  int conv_kn(const float* src, int K, int N, int Kp, int Np) const;
  int pad_bias(const float* b, int N, int Np) const;      // -> bias fp32 [Np], the pad zero
  // C = A Bt^T over K (ldb = K); ks > 1: split-K through `part`
  int gemm(int M, int N, int K, const void* A, int lda, const void* Bt, int ks,
           const vtd_epilogue& e, double flops) const;
  // dW [K][ldw] = X^T G, db = column sums of G; ms > 1: msplit partial planes in `part`
  int wgrad(int M, int K, int N, const void* X, int ldx, const void* G, int ldg, float* dW,
            int ldw, float* db, int ms) const;
  // z fp32 [M][up] = a_in W + b, the pre-activation kept; then a_out = drop(act(z)) in the
  // operand dtype (dk null: no dropout; a_out null: the stack applies no activation here)
  int dense_forward(const DenseDims& L, const float* W, const float* b, const void* a_in, int ks,
                    float* z, int act, void* a_out, const DropKey* dk) const;
  // gz = gin * d drop(act(z)) / dz in the operand dtype; dW = a_in^T gz, db; din fp32 [M][nout] =
  // gz W^T (nout: the columns written and the leading dimension, kv <= nout <= k)
  int dense_backward(const DenseDims& L, const float* W, const void* a_in, const float* z,
                     const float* gin, int ldgin, int act, const DropKey* dk, void* gz, float* dW,
                     float* db, int ms, int ks, float* din, int nout) const;
};

// ----------------------------------------------------------------- vtd_gemm.hip
int gemm_launch(int M, int N, int K, const void* A, int lda, const void* Bt, int ldb,
                int dtype, const vtd_epilogue* epi, hipStream_t stream, double flops);
bool gemm_emits_stats(int M, int N, int dtype, const vtd_epilogue* e);
int gemm_splitk_choice(int M, int N, int K, int dtype, int target = 0);
int gemm_splitk_launch(int M, int N, int K, const void* A, int lda, const void* Bt, int ldb,
                       int dtype, const vtd_epilogue* epi, float* part, int ksplit,
                       hipStream_t stream, double flops);
bool gemm_mx8_emits_fp8(int M, int N, const vtd_epilogue* e);
int gemm_mx8_launch(int M, int N, int K, const uint8_t* A, int lda, const uint8_t* sA,
                    int64_t sa_rows, const uint8_t* Bt, int ldb, const uint8_t* sB,
                    int64_t sb_rows, const vtd_epilogue* epi, hipStream_t stream,
                    double flops);
#if VTD_DIAG
// vtd_gemm_w4.hip (diagnostic build only)
bool gemm_w4_launch(int M, int N, int K, const bf16_t* A, int lda, const bf16_t* Bt, int ldb,
                    const vtd_epilogue* epi, int ngw, hipStream_t stream);
void gemm_mx8_x4_launch(int M, int N, int K, const uint8_t* A, int lda, const uint8_t* sA,
                        int64_t sa_rows, const uint8_t* Bt, int ldb, const uint8_t* sB,
                        int64_t sb_rows, const vtd_epilogue* epi, int ngw, hipStream_t stream);
#endif

// ----------------------------------------------------------------- vtd_gemm_wgrad.hip
int gemm_wgrad_choice(int M, int K, int N, int dtype);
int gemm_wgrad_launch(int M, int K, int N, const void* X, int ldx, const void* G, int ldg,
                      int dtype, float* dW, int ldw, float* db, float* part, size_t part_bytes,
                      int msplit, hipStream_t stream);

// ----------------------------------------------------------------- vtd_attention.hip
int attention_launch(const void* qkv, int B, int N, int heads, int dkp, int ldqkv,
                     float scale, void* out, int ldo, int dtype, hipStream_t stream,
                     double flops, int parts = 1);
int attention_mx8_launch(const void* qkv, int B, int N, int heads, int dkp, int ldqkv,
                         float scale, uint8_t* q, int ldq, uint8_t* s, int64_t s_rows,
                         hipStream_t stream, double flops);
// dk: dropout on the attention probabilities (the DROP instantiations; dk from drop_prepare)
int attention_train_launch(const void* qkv, int B, int N, int heads, int dkp, int ldqkv,
                           float scale, void* out, int ldo, float* lse, int dtype,
                           hipStream_t stream, const DropKey* dk = nullptr);

// ----------------------------------------------------------------- vtd_attention_bwd.hip
int attention_backward_workspace_bytes(int B, int N, int heads, int dkp, int dtype,
                                       size_t* bytes);
int attention_backward_launch(const void* qkv, const void* o, const void* dO, const float* lse,
                              int B, int N, int heads, int dkp, int ldqkv, int ldo, int lddo,
                              float scale, void* dqkv, int lddqkv, int dtype, void* ws,
                              size_t ws_bytes, hipStream_t stream, const DropKey* dk = nullptr);

// ----------------------------------------------------------------- vtd_elementwise.hip
// checks a vtd_dropout (non-null, rate in [0, 1)) and derives what the kernels take; *on = rate > 0
int drop_prepare(const char* what, const vtd_dropout* d, DropKey* key, bool* on);
int layernorm_launch(const void* x, int x_dtype, int64_t rows, int D, int ldx, const float* g,
                     const float* b, float eps, void* y, int ldy, int dtype, hipStream_t st);
int layernorm_mx8_launch(const void* x, int x_dtype, int64_t rows, int D, int ldx,
                         const float* g, const float* b, float eps, uint8_t* q, int ldq, int Kq,
                         uint8_t* s, int64_t s_rows, hipStream_t st);
int ln_stats_launch(const void* x, int x_dtype, int64_t rows, int D, int ldx, float eps,
                    float* stat, hipStream_t st);
int ln_stats_finalize_launch(const float* part, int64_t rows, int slots, int D, float eps,
                             float* stat, hipStream_t st);
int patches_launch(const float* img, int B, int H, int W, int C, int p, void* out, int ldo,
                   int dtype, hipStream_t st);
int split_bf16x3_launch(const float* x, int64_t rows, int K, int ldx, void* y, int ldy, int role,
                        hipStream_t st);
int unpad_f32_launch(const void* x, int x_dtype, int64_t rows, int D, int ldx, float* y,
                     hipStream_t st);
int transpose_op_launch(const float* src, int K, int N, void* dst, int Kp, int Np, int dtype,
                        hipStream_t st);
// dk (both): y = drop(act(z)) and its gradient, the DROP instantiations
int act_forward_launch(const float* z, int64_t rows, int N, int ldz, int act, void* y, int ldy,
                       int dtype, hipStream_t st, const DropKey* dk = nullptr);
int act_grad_launch(const float* z, int ldz, const float* ga, int ldga, int64_t rows, int N,
                    int act, void* y, int ldy, int dtype, hipStream_t st,
                    const DropKey* dk = nullptr);
int head_unscatter_launch(const float* dU, int B, int T, int ldu, void* y, int ldy, int dtype,
                          hipStream_t st);

// ----------------------------------------------------------------- vtd_layernorm_bwd.hip
int layernorm_backward_workspace_bytes(int64_t rows, int D, size_t* bytes);
int layernorm_backward_launch(const float* x, int ldx, const float* stat, const float* gamma,
                              const float* dy, int lddy, const float* add, int ldadd,
                              int64_t rows, int D, float* dx, int lddx, float* dgamma,
                              float* dbeta, void* ws, size_t ws_bytes, hipStream_t st);

// ----------------------------------------------------------------- vtd_block_bwd.hip
// A padded matrix Wp [Kp][Np] made of up to three Keras tensors src[part] [K][N] side by side
// along n (part width part_np), with group padding on either axis: source row (k / kgp) kg +
// k % kgp for k % kgp < kg, source column likewise from n % part_np with ng / ngp; every other
// element is zero.  query/key/value: K = kg = d, kgp = Kp = d_p, N = heads key_dim, ng =
// key_dim, ngp = dkp, part_np = inner_p, 3 parts; attention_output: K = heads key_dim, kg =
// key_dim, kgp = dkp, N = ng = d, ngp = part_np = Np = d_p, 1 part.
struct BlockGather {
  const float* src[3];
  int nparts, K, N, kg, kgp, ng, ngp, part_np, Kp, Np;
};
// Wp in the operand dtype (bf16, or the split B operand [hi | hi | lo], the conversions of
// split_bf16x3 role 1): dst_t = Wp^T [Np][kk(Kp)] (a forward GEMM's Bt), dst_kn = Wp
// [Kp][kk(Np)] (an input-gradient GEMM's Bt); either may be null.  Every pad is written as zero.
int block_gather_launch(const BlockGather& g, void* dst_t, void* dst_kn, int dtype,
                        hipStream_t st);
// the biases (K = kg = kgp = 1) -> the padded fp32 vector [Np]
int block_gather_bias_launch(const BlockGather& g, float* dst, hipStream_t st);
// the inverse on fp32 gradients: W [Kp][ldw] (and b [Np], nullable) -> dst[part] [K][N]
// (dstb[part] [N]); g.src is not read
int block_ungather_launch(const BlockGather& g, float* const* dst, float* const* dstb,
                          const float* W, int ldw, const float* b, hipStream_t st);
// y = x1 + act(z), fp32 [rows][D]; dk: y = x1 + drop(act(z))
int block_resid_act_launch(const float* x1, int ldx, const float* z, int ldz, int64_t rows, int D,
                           int act, float* y, int ldy, hipStream_t st, const DropKey* dk = nullptr);

// ----------------------------------------------------------------- vtd_mx8.hip
int quantize_mx8_launch(const void* x, int x_dtype, int64_t rows, int K, int ldx, int Kq,
                        uint8_t* q, int ldq, uint8_t* s, int64_t s_rows, hipStream_t st);

}  // namespace vtd
