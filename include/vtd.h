/*
 * vtd.h — C-ABI of libvtd.so, the MI355X (gfx950) forward path of the Vision
 * Transformer detector of westlake-moonlight/vision_transformer_detector.
 *
 * The reference has no FFI: its forward is a Keras graph whose arithmetic runs in
 * TensorFlow 2.9.1's own kernels.  Each entry point below replaces one layer class
 * of that graph (cited as vtd.py:N = /root/reference/vision_transformer_detector.py);
 * `vtd_forward` replaces the whole `model(images, training=False)` call.
 *
 * Conventions
 *  - Every pointer argument named *_dev is DEVICE memory owned by the caller.  The
 *    library never allocates or frees memory inside a compute call and keeps no
 *    pointer after it returns.  `stream` is a hipStream_t (NULL = default stream).
 *  - Calls are asynchronous on `stream`, perform no host synchronisation and no
 *    allocation, and are therefore HIP-graph capturable.
 *  - Return value: VTD_OK (0) or a negative vtd_status; `vtd_last_error()` returns a
 *    thread-local message for the last failure on the calling thread.
 *  - "Padded" widths: every activation/weight row is padded with zeros to a multiple
 *    of VTD_KALIGN elements (see vtd_dims); pad columns are guaranteed zero on output.
 */
#ifndef VTD_H_
#define VTD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTD_ABI_VERSION 17
#define VTD_KALIGN 64          /* K / row padding granule, elements              */
#define VTD_MAX_MLP 16         /* max encoder_mlp_quantities                     */
#define VTD_MAX_HEAD 64        /* max mlp_head layers * repeats                   */
#define VTD_MAX_DETECT 17      /* Constants.MAX_DETECT_OBJECTS_QUANTITY vtd.py:28 */

typedef enum vtd_status {
  VTD_OK = 0,
  VTD_ERR_INVALID_ARG = -1,    /* bad shape / null pointer / unsupported combo  */
  VTD_ERR_UNSUPPORTED = -2,    /* dtype or size not supported by this build     */
  VTD_ERR_HIP = -3,            /* a HIP runtime call failed (message has code)  */
  VTD_ERR_WORKSPACE = -4       /* workspace too small                           */
} vtd_status;

typedef enum vtd_dtype {       /* compute (GEMM operand) dtype                   */
  VTD_F32 = 0,                 /* parity mode: f32 operands, f32 MFMA            */
  VTD_BF16 = 1,                /* throughput mode: bf16 operands, f32 accumulate */
  VTD_FP8 = 2,                 /* forward mode only (vtd_config.dtype): encoder  */
                               /* Dense layers in MX-fp8 (vtd_gemm_mx8), the rest */
                               /* as VTD_BF16                                     */
  VTD_BF16X3 = 3               /* split-bf16 parity mode: every Dense layer as    */
                               /* three bf16 MFMA products with f32 accumulation, */
                               /* the rest fp32 (see "Split-bf16 operands")       */
} vtd_dtype;

/* Split-bf16 operands (VTD_BF16X3).  An f32 value v is held as hi = bf16(v) (round to
 * nearest even) and lo = bf16(v - hi): hi + lo carries 16 significand bits, and
 * hi_a hi_b + lo_a hi_b + hi_a lo_b leaves out only lo_a lo_b (<= 2^-18 |a b|).  A K-wide
 * f32 row is stored as a bf16 row of P-wide pieces (P >= K, P % 64 == 0 for a GEMM, the
 * columns [K, P) of every piece zero):
 *   A operand (activations, role 0):  [ hi | lo ]        (row stride >= 2 P)
 *   B operand (weights W^T, role 1):  [ hi | hi | lo ]   (row stride >= 3 P)
 * and vtd_gemm with dtype VTD_BF16X3, K = 3 P, reads each A row as [hi | lo | hi] (its K loop
 * returns to A's column 0 after 2 P) against the B row: one bf16 GEMM whose fp32
 * accumulators sum the three products.  Producers write the A form directly:
 * vtd_epilogue.out_dtype = VTD_BF16X3, vtd_layernorm / vtd_extract_patches / vtd_attention
 * with dtype = VTD_BF16X3 (ldo / ldy = 2 P); vtd_split_bf16x3 converts any f32 matrix. */

typedef enum vtd_act {         /* activation fused in a GEMM epilogue            */
  VTD_ACT_NONE = 0,
  VTD_ACT_GELU_TANH = 1,       /* tfa.layers.GELU() approximate=True vtd.py:402 */
  VTD_ACT_MISH = 2             /* MishActivation vtd.py:119-129                  */
} vtd_act;

/* create_vision_transformer_detector(...) kwargs, vtd.py:498-506.  dropout,
 * max_weight and clip_weight only act on training (Keras Dropout / MHA dropout are the
 * identity at inference; constraints apply after optimizer steps): no fields here. */
typedef struct vtd_config {
  int batch;
  int image_h, image_w, channels;     /* input_shape                              */
  int patch_size;
  int embedding_dim;
  int num_heads;                      /* encoder_num_heads                        */
  int key_dim;                        /* encoder_key_dim                          */
  int mlp_quantities;                 /* encoder_mlp_quantities                   */
  int repeat_times;                   /* encoder_repeat_times                     */
  int head_last_units;                /* mlp_head_last_units                      */
  int head_layers;                    /* mlp_head_dense_layers_quantity           */
  int head_repeats;                   /* mlp_head_dense_mish_block_repeats        */
  int use_mish;                       /* 1 = Mish, 0 = GELU(tanh)                 */
  int dtype;                          /* vtd_dtype                                */
} vtd_config;

/* Derived sizes (elements).  Fill with vtd_derive_dims. */
typedef struct vtd_dims {
  int grid_h, grid_w;                 /* ceil(H/p), ceil(W/p)  (SAME padding)     */
  int tokens;                         /* N = grid_h*grid_w                        */
  int pad_top, pad_left;              /* SAME pad_before                          */
  int patch_dim, patch_dim_p;         /* P = p*p*C and padded                     */
  int d, d_p;                         /* embedding_dim and padded                 */
  int key_dim_p;                      /* per-head padded key dim (32/64/128)      */
  int inner_p;                        /* num_heads * key_dim_p                    */
  int qkv_p;                          /* padded 3*inner_p                         */
  int mlp_units[VTD_MAX_MLP];         /* encoder MLP widths                       */
  int mlp_units_p[VTD_MAX_MLP];
  int n_head;                         /* head Dense layers (excl. dense & final)  */
  int head_units[VTD_MAX_HEAD];
  int head_units_p[VTD_MAX_HEAD];
  int tokens_p;                       /* head input width (Reshape) padded        */
  int64_t rows;                       /* batch * tokens                           */
  int64_t head_rows;                  /* batch * 17                               */
} vtd_dims;

/* Device pointers of one encoder block, packed by vtd_pack_dense / vtd_pack_vector.
 * Matrices: dtype = cfg.dtype, layout W^T [N_p][K_p] (row = output unit).
 * Vectors: fp32, padded with zeros.
 * VTD_FP8: w_qkv / w_out / w_mlp are MX-fp8 e4m3 [N_p][K8] (K8 = K_p rounded up to 128,
 * vtd_quantize_mx8 of the packed fp32 matrix) and s_* their scales [K8/128][N_p][4];
 * the s_* fields are ignored in the other modes.
 * LayerNorm fold (VTD_BF16 only): when ln1_colsum is non-NULL, w_qkv / b_qkv hold
 * vtd_fold_layernorm's W * diag(ln1_gamma) and b + W ln1_beta, ln1_colsum its column
 * sums, and the forward applies LayerNorm 1 in the query/key/value GEMM's epilogue
 * (vtd_epilogue.lnstat) instead of a LayerNorm pass; ln2_colsum likewise for LayerNorm 2
 * and w_mlp[0] / b_mlp[0].  NULL: the LayerNorm kernels run (ln*_gamma / beta used). */
typedef struct vtd_layer_weights {
  const float* ln1_gamma; const float* ln1_beta;        /* [d_p]                  */
  const void* w_qkv; const float* b_qkv;                /* [qkv_p][d_p], [qkv_p]  */
  const void* w_out; const float* b_out;                /* [d_p][inner_p], [d_p]  */
  const float* ln2_gamma; const float* ln2_beta;        /* [d_p]                  */
  const void* w_mlp[VTD_MAX_MLP]; const float* b_mlp[VTD_MAX_MLP];
  const uint8_t* s_qkv; const uint8_t* s_out;          /* VTD_FP8 block scales   */
  const uint8_t* s_mlp[VTD_MAX_MLP];
  const float* ln1_colsum; const float* ln2_colsum;     /* LN fold, or NULL        */
} vtd_layer_weights;

typedef struct vtd_weights {
  const void* w_patch; const float* b_patch;            /* [d_p][patch_dim_p]     */
  const float* pos_embedding;                           /* [tokens] fp32          */
  const vtd_layer_weights* layers;                      /* HOST array [repeat_times] */
  const void* w_det; const float* b_det;                /* Dense(17): [64][d_p]   */
  const void* w_head[VTD_MAX_HEAD]; const float* b_head[VTD_MAX_HEAD];
  const void* w_final; const float* b_final;            /* Dense(6): [64][136_p]  */
} vtd_weights;

/* ---------------------------------------------------------------- library ------ */
int vtd_abi_version(void);
const char* vtd_last_error(void);

/* Shapes of the graph built by create_vision_transformer_detector (vtd.py:498-583). */
int vtd_derive_dims(const vtd_config* cfg, vtd_dims* out);

/* Bytes of scratch `vtd_forward` needs for this config (256-B aligned buffers). */
int vtd_workspace_bytes(const vtd_config* cfg, size_t* bytes);

/* ---------------------------------------------------------------- weights ------ */
/* Pack a Keras Dense/EinsumDense kernel (fp32, row-major [K][N], device) into the
 * transposed, zero-padded compute layout dst[n_row_offset + n'][k'] (dtype), where
 * k' = (k / k_group) * k_group_p + k % k_group   (per-head K padding, attention_output)
 * n' = (n / n_group) * n_group_p + n % n_group   (per-head N padding, query/key/value).
 * Pass k_group = k_group_p = K (resp. N) for no grouping.  dst must be pre-zeroed. */
int vtd_pack_dense(const float* src_dev, int K, int N, int k_group, int k_group_p,
                   int n_group, int n_group_p, void* dst_dev, int ld_dst,
                   int n_row_offset, int dtype, void* stream);
/* Same re-indexing for a bias / LN vector (fp32 -> fp32). */
int vtd_pack_vector(const float* src_dev, int N, int n_group, int n_group_p,
                    float* dst_dev, int offset, void* stream);

/* f32 x [rows][ldx] (first K columns) -> split-bf16 y [rows][ldy], P >= K wide pieces
 * (columns [K, P) of each piece written as zero): role 0 the A operand [hi | lo], P = ldy / 2
 * (ldy % 2 == 0); role 1 the B operand [hi | hi | lo], P = ldy / 3 (ldy % 3 == 0). */
int vtd_split_bf16x3(const float* x_dev, int64_t rows, int K, int ldx, void* y_dev, int ldy,
                     int role, void* stream);

/* ---------------------------------------------------------------- per-op ------- */
/* ExtractImagePatches (vtd.py:177-206) + Reshape flatten_patches (vtd.py:279-280):
 * images NHWC fp32 [B][H][W][C] -> patches [B*N][ld_out] (dtype), SAME zero pad,
 * (kh, kw, c) order; columns [P, ld_out) written as zero.  dtype VTD_BF16X3: the split-bf16
 * A operand, two ld_out / 2 wide pieces (ld_out % 16 == 0). */
int vtd_extract_patches(const float* images_dev, int B, int H, int W, int C, int p,
                        void* out_dev, int ld_out, int dtype, void* stream);

/* Dense + activation (vtd.py:297, 389-403, 454, 472-483, 489):
 * C[m][n] = act(sum_k A[m][k] * Bt[n][k] + bias[n] + rowadd[m % rowadd_period]
 *               (rowadd only for n < rowadd_ncols)) + resid[m][n]
 * for m < M, n < N.  A, Bt in `dtype`; K % VTD_KALIGN == 0; lda, ldb % 8 == 0.
 * dtype VTD_BF16X3: bf16 operands, A the split-bf16 A operand [hi | lo] (lda >= 2 K / 3), Bt
 * the B operand [hi | hi | lo] (ldb >= K; its two hi pieces must be equal, as
 * vtd_split_bf16x3 role 1 writes them: a kernel may read either), K = 3 P with P % 64 == 0
 * (see "Split-bf16 operands").
 * out: fp32 (out_dtype 0), bf16 (1) or split-bf16 (VTD_BF16X3: the next GEMM's A operand
 * [hi | lo], two ldo / 2 wide pieces, ldo % 2 == 0, ldo / 2 >= N; bf16 / split-bf16
 * operands only); out2 (nullable) a second bf16 copy.
 * scatter_tokens > 0 selects the head Reshape epilogue (vtd.py:461-463): element
 * (m = b*T + t, n < 17) is stored at out[(b*17 + f / T) * ldo + f % T], f = t*17 + n.
 * Pad rule: no value outside the M x K / N x K operand elements (and the epilogue vectors'
 * M, N or period entries) reaches an output, and nothing but the M x N output elements (of
 * every piece) is written -- pad columns up to the leading dimensions and neighbouring memory
 * keep their bytes (tests/test_gpu_gemm_designed.py runs every kernel inside guard bands). */
typedef struct vtd_epilogue {
  const float* bias;            /* [N] or NULL                                    */
  const float* rowadd;          /* position embedding per row, or NULL            */
  int rowadd_period, rowadd_ncols;
  int act;                      /* vtd_act                                         */
  const void* resid; int ldr;   /* residual in out_dtype (may alias out), or NULL  */
  void* out; int ldo; int out_dtype;
  void* out2; int ldo2;         /* optional bf16 copy                              */
  int scatter_tokens;
  /* LayerNorm folded into the GEMM (A = the raw rows x, Bt = W * diag(gamma) as stored,
   * bias = b + W beta): lnstat[2m], lnstat[2m+1] = mean, rstd of row m
   * (vtd_layernorm_stats) and colsum[n] = sum_k Bt[n][k]; the accumulator becomes
   * (acc - mean * colsum[n]) * rstd before bias / act.  Both NULL: no fold. */
  const float* lnstat; const float* colsum;
  /* Partial LayerNorm statistics of the output (the fold path's producer side): for row m
   * and 64-column block b, statout[2 (b stat_ld + m)] = mean and [.. + 1] = sum of squared
   * deviations from that mean, of the block's 64 stored bf16 values (centred partials:
   * exact whatever |mean| / std).  Slot-major: one plane of stat_ld >= M rows per block.
   * Only on full 256 x 256 tiles of the bf16 fast epilogues -- dtype VTD_BF16, M % 256 ==
   * N % 256 == 0 and at least 64 tiles (else vtd_gemm returns VTD_ERR_UNSUPPORTED); NULL: none. */
  float* statout; int stat_ld;
  /* out_dtype VTD_FP8 (vtd_gemm_mx8 only, every tile full: M % 256 == N % 256 == 0): the
   * output is written as the next GEMM's MX-fp8 A operand, byte for byte what
   * vtd_quantize_mx8 makes of the bf16-rounded output: e4m3 out[m * ldo + n] and
   * scale_out[n/128][scale_rows][4]. */
  uint8_t* scale_out; int64_t scale_rows;
  /* transform_predictions (vtd.py:586-647) fused into the final Dense(6) (SURVEY §8b
   * vtd_head_decode): with N == 6, an fp32 output and no scatter, detections[m * 6 + n] =
   * sigmoid(C[m][n]), clipped to [0, 1] for n >= 2, times (1, 79, 608, 608, 608, 608) --
   * what vtd_decode computes from the stored logits, bit for bit.  NULL: none. */
  float* detections;
} vtd_epilogue;
int vtd_gemm(int M, int N, int K, const void* A_dev, int lda, const void* Bt_dev,
             int ldb, int dtype, const vtd_epilogue* epi, void* stream);
/* Split-K form of vtd_gemm (dtype VTD_BF16 or VTD_BF16X3; what vtd_forward runs for the
 * detection head's few-tile, long-K Dense layers, vtd.py:468-486): `ksplit` K ranges of
 * K / 64 / ksplit
 * K-steps each write fp32 partial sums into part_dev ([ksplit][M][N] floats,
 * part_bytes >= ksplit * M * N * 4), then one pass sums them in split order and applies
 * the epilogue (the LayerNorm fold included; no partial statistics).  K % 64 == 0, N % 4 == 0,
 * 2 <= ksplit <= K / 64 with every split non-empty.  vtd_gemm_splitk_choice returns the
 * split count vtd_forward uses for (M, N, K, dtype) (1 = no split). */
int vtd_gemm_splitk(int M, int N, int K, const void* A_dev, int lda, const void* Bt_dev,
                    int ldb, int dtype, const vtd_epilogue* epi, float* part_dev,
                    size_t part_bytes, int ksplit, void* stream);
int vtd_gemm_splitk_choice(int M, int N, int K, int dtype);

/* MX-fp8 operands (OCP MX: e4m3 elements, one E8M0 scale byte e = 2^(e-127) per 32
 * consecutive K elements).  vtd_quantize_mx8: x [rows][ldx] (x_dtype F32 or BF16), first
 * K columns -> q [rows][ldq] e4m3 bytes with Kq columns (Kq % 128 == 0, columns [K, Kq)
 * zero) and scales s[Kq/128][s_rows][4] (s_rows >= rows; the 4 scales of one 128-wide
 * K-step of a row are one dword).  Block scale: the least 2^E with amax <= 448 * 2^E,
 * E in [-126, 126]; elements round to nearest even (oracle/mx8.py restates both).
 * vtd_gemm_mx8: as vtd_gemm (same epilogue) with A [M][lda], Bt [N][ldb] in that format,
 * K % 128 == 0, lda/ldb % 16 == 0, sa_rows >= M, sb_rows >= N, both % 4 == 0;
 * D = sum_k dec(A) dec(Bt) accumulated in fp32 by v_mfma_scale_f32_16x16x128_f8f6f4. */
int vtd_quantize_mx8(const void* x_dev, int x_dtype, int64_t rows, int K, int ldx, int Kq,
                     uint8_t* q_dev, int ldq, uint8_t* s_dev, int64_t s_rows, void* stream);
/* vtd_layernorm with the output quantized as vtd_quantize_mx8 does the bf16-rounded
 * LayerNorm output (Kq % 128 == 0 >= D columns, ldq % 16 == 0): LN + quantize in one pass. */
int vtd_layernorm_mx8(const void* x_dev, int x_dtype, int64_t rows, int D, int ldx,
                      const float* gamma_dev, const float* beta_dev, float eps, uint8_t* q_dev,
                      int ldq, int Kq, uint8_t* s_dev, int64_t s_rows, void* stream);
int vtd_gemm_mx8(int M, int N, int K, const uint8_t* A_dev, int lda, const uint8_t* sA_dev,
                 int64_t sa_rows, const uint8_t* Bt_dev, int ldb, const uint8_t* sB_dev,
                 int64_t sb_rows, const vtd_epilogue* epi, void* stream);

/* keras LayerNormalization(axis=-1, epsilon) (vtd.py:353-357, 375-379):
 * x (x_dtype: fp32, or the bf16 residual stream) [rows][ldx] -> y (dtype) [rows][ldy];
 * fp32 statistics over the first D columns; columns [D, ldy) of y written as zero.
 * dtype VTD_BF16X3: y is the split-bf16 A operand, two ldy / 2 wide pieces. */
int vtd_layernorm(const void* x_dev, int x_dtype, int64_t rows, int D, int ldx,
                  const float* gamma_dev, const float* beta_dev, float eps,
                  void* y_dev, int ldy, int dtype, void* stream);

/* Row statistics of keras LayerNormalization (the same two-pass fp32 mean / biased
 * variance as vtd_layernorm): stat[2r] = mean, stat[2r+1] = 1 / sqrt(var + eps) of the
 * first D columns of row r of x (x_dtype F32 or BF16). */
int vtd_layernorm_stats(const void* x_dev, int x_dtype, int64_t rows, int D, int ldx,
                        float eps, float* stat_dev, void* stream);

/* (mean, rstd) per row from the centred partials a producer GEMM wrote
 * (vtd_epilogue.statout with stat_ld == rows: `slots` planes of `rows` (mean, M2) pairs,
 * D == 64 * slots): Chan's merge of the block (mean, M2) pairs in fp32, no one-pass
 * sum(x^2) - mean^2 cancellation. */
int vtd_layernorm_stats_finalize(const float* partial_dev, int64_t rows, int slots, int D,
                                 float eps, float* stat_dev, void* stream);

/* Folds LayerNorm(gamma, beta) into the Dense layer that consumes it: w32 fp32 packed
 * W^T [N][ldw] (first K columns used) -> w_out (dtype) [N][ldo] = W^T[n][k] * gamma[k]
 * (columns [K, ldo) zero), bias_out[n] = bias_in[n] + sum_k W^T[n][k] beta[k] and
 * colsum[n] = sum_k w_out[n][k] (of the stored, rounded values); fp64 sums.
 * LN(x) W + b == (x W' - mean * colsum) * rstd + bias_out, exactly in real arithmetic. */
int vtd_fold_layernorm(const float* w32_dev, int N, int K, int ldw, const float* gamma_dev,
                       const float* beta_dev, const float* bias_in_dev, void* w_out_dev,
                       int ldo, int dtype, float* bias_out_dev, float* colsum_dev,
                       void* stream);

/* keras MultiHeadAttention core (vtd.py:364-369): per batch b, head h,
 * O = softmax(scale * Q K^T) V with Q, K, V read from qkv [B*N][ldqkv] at column
 * offsets h*dkp, inner + h*dkp, 2*inner + h*dkp (inner = heads*dkp); O written to
 * out [B*N][ldo] at column h*dkp.  dkp in {32, 64, 128}; scale = 1/sqrt(key_dim).
 * dtype VTD_BF16X3 (the split-bf16 parity mode): qkv is fp32, every product runs as three
 * bf16 MFMA products (hi.hi + lo.hi + hi.lo, fp32 softmax statistics), and out is the
 * split-bf16 A operand of the attention-output Dense, [hi | lo] in two ldo / 2 wide pieces
 * (ldo % 2 == 0, ldo / 2 >= heads*dkp; columns [heads*dkp, ldo / 2) not written).
 * scale must be positive and finite (else VTD_ERR_INVALID_ARG).  Any finite inputs whose
 * scaled scores scale * log2(e) * q.k (every partial sum over d) are finite in fp32 give a
 * finite result within the mode's tolerance (2e-5 of max(1, max |O|) for VTD_F32 /
 * VTD_BF16X3, 2e-2 for VTD_BF16), whatever the size or sign of the scores: no kernel's
 * running max costs a row more than fp32 rounding of its scores
 * (tests/test_gpu_attention_patterns.py).
 * Size: rows are indexed with 64-bit products, so qkv and out may extend past 2^32 bytes
 * (tests/test_gpu_big_operands.py).  One IMAGE is addressed through 32-bit offsets by the
 * buffer-addressed bf16 kernels: the persistent kernel is chosen only while N * ldqkv * 2 and
 * N * ldo * 2 are below 2^31 bytes (the streaming kernels run otherwise), and the long-sequence
 * kernel of VTD_KNOB_ATTN_VARIANT 6 returns VTD_ERR_INVALID_ARG before any launch for such an
 * image (tests/test_big_operands_host.py). */
int vtd_attention(const void* qkv_dev, int B, int N, int heads, int dkp, int ldqkv,
                  float scale, void* out_dev, int ldo, int dtype, void* stream);

/* vtd_attention (bf16 operands) with the output written as the MX-fp8 A operand of the
 * attention-output Dense (VTD_FP8 mode): q_dev [B*N][ldq] e4m3 bytes, s_dev
 * [heads*dkp/128][s_rows][4] E8M0 scales (the vtd_quantize_mx8 layout); byte-identical to
 * vtd_attention (bf16 out) followed by vtd_quantize_mx8. heads*dkp % 128 == 0, ldq % 16 == 0,
 * s_rows >= B*N. */
int vtd_attention_mx8(const void* qkv_dev, int B, int N, int heads, int dkp, int ldqkv,
                      float scale, uint8_t* q_dev, int ldq, uint8_t* s_dev, int64_t s_rows,
                      void* stream);

/* transform_predictions (vtd.py:586-647): logits fp32 [n][6] -> detections fp32
 * [sigmoid, sigmoid*79, clip(sigmoid)*608 x4]. */
int vtd_decode(const float* logits_dev, int64_t n, float* dets_dev, void* stream);

/* transform_predictions + the detection test of MeanAveragePrecision.update_state
 * (vtd.py:1359-1384), per slot: dets as vtd_decode; category = round-half-even of the
 * decoded class (tf.round); class confidence = (0.5 - |cls - category|) / 0.5;
 * valid = objectness > obj_threshold && confidence > cls_threshold
 * (Constants.OBJECTNESS_THRESHOLD / CLASSIFICATION_CONFIDENCE_THRESHOLD = 0.5).
 * category_dev (int32) and valid_dev (uint8) may be NULL. */
int vtd_decode_detections(const float* logits_dev, int64_t n, float* dets_dev,
                          int32_t* category_dev, uint8_t* valid_dev, float obj_threshold,
                          float cls_threshold, void* stream);

/* ---------------------------------------------------------------- input ------- */
/* _get_image_tensor_coco after decode (vision_transformer_utilities.py:418-449):
 * tf.image.resize_with_pad(image, target_h, target_w) (bilinear, half-pixel centers, no
 * antialias; TF 2.9 float32 geometry: ratio = max(w/tw, h/th), resized = floor(side/ratio),
 * pad_before = floor((target - side/ratio)/2)) -> clip [0, 255] -> /127.5 -> -1.
 * pixels_dev: B decoded uint8 HWC (C = 3) images, image b at byte offset offsets_dev[b];
 * sizes_dev: int32 [B][2] = (height, width). out_dev: fp32 NHWC [B][target_h][target_w][3]
 * in [-1, 1] (pad = -1), i.e. the `images` argument of vtd_forward. Images whose resized
 * side would be 0 (TF raises for them) must be rejected by the caller: the kernel writes
 * the pad value for them. Replaces the tf.image / tf.clip_by_value / arithmetic ops at
 * vision_transformer_utilities.py:438-447. */
int vtd_resize_with_pad(const uint8_t* pixels_dev, const int64_t* offsets_dev,
                        const int32_t* sizes_dev, int B, int target_h, int target_w,
                        float* out_dev, void* stream);

/* JPEG decode on the device, tf.image.decode_image(file, channels=3)
 * (vision_transformer_utilities.py:431) for baseline / extended sequential and progressive
 * Huffman JPEG: 8-bit, 1, 3 or 4 (CMYK / YCCK) components, 4:4:4 / 4:2:2 / 4:2:0, restart
 * intervals.  libjpeg-turbo's decode path (what TF uses): ISLOW IDCT, fancy upsampling,
 * YCbCr -> RGB; gray -> RGB replicated; CMYK (YCCK -> CMYK as jdcolor.c) -> RGB as TF's
 * jpeg_mem.cc (Adobe marker: R = K C / 255, else (255 - K)(255 - C) / 255).  The colour space
 * of a 3-component file is libjpeg's choice (jdapimin.c default_decompress_parms), in this
 * order: a JFIF APP0 marker means YCbCr; otherwise an Adobe APP14 marker decides (transform 0:
 * RGB, else YCbCr); otherwise the component ids do ('R' 'G' 'B': RGB, all others YCbCr).  Both
 * markers count only before the first scan.  Other JPEGs
 * (arithmetic-coded, lossless, 12-bit, 4:4:0, ...) return VTD_ERR_UNSUPPORTED with the reason.
 * vtd_jpeg_info: header only (host).  The images are HOST buffers; their marker segments are
 * parsed on the host, the entropy-coded data + derived tables copied to the workspace on
 * `stream` (through a pinned staging buffer the library reuses), image i written as RGB
 * uint8 HWC at out_dev + out_offsets[i] (host array). */
int vtd_jpeg_info(const uint8_t* jpeg, size_t len, int* h, int* w, int* comps);
int vtd_jpeg_workspace_bytes(const uint8_t* const* jpegs, const size_t* lens, int n,
                             int32_t* dims /* nullable: 2n ints, (h, w) per image */,
                             size_t* bytes);
int vtd_jpeg_decode(const uint8_t* const* jpegs, const size_t* lens, int n, uint8_t* out_dev,
                    const int64_t* out_offsets, void* workspace_dev, size_t workspace_bytes,
                    void* stream);

/* PNG decode, tf.image.decode_image(file, channels=3) for PNG (vision_transformer_utilities.py
 * :431) as TF's libpng path does it: every colour type and bit depth (1-16), Adam7
 * interlacing; palette -> RGB, gray -> RGB, alpha / tRNS dropped, 16-bit -> high byte.  The
 * chunk walk (critical-chunk CRCs checked) and the zlib inflate run on the host over a few
 * threads; a row filter byte above 4 is an error (libpng's "bad adaptive filter value"); the
 * filtered scanlines are copied to the workspace on `stream` (pinned staging the library
 * reuses) and un-filtered + converted on the device (rows of up to 16 KiB of filtered bytes
 * through LDS, wider ones in place in the workspace: no width limit beyond w * h <= 2^28),
 * image i written as RGB uint8 HWC at out_dev + out_offsets[i].  Same calling convention as
 * the JPEG entry points; vtd_png_info's comps = samples per pixel of the file (1-4).
 * vtd_png_inflate: the host half alone for one file (chunk walk, inflate, filter-byte check)
 * into a caller HOST buffer; *need = the filtered scanline bytes of all passes (out == NULL:
 * only *need). */
int vtd_png_info(const uint8_t* png, size_t len, int* h, int* w, int* comps);
int vtd_png_workspace_bytes(const uint8_t* const* pngs, const size_t* lens, int n,
                            int32_t* dims, size_t* bytes);
int vtd_png_decode(const uint8_t* const* pngs, const size_t* lens, int n, uint8_t* out_dev,
                   const int64_t* out_offsets, void* workspace_dev, size_t workspace_bytes,
                   void* stream);
int vtd_png_inflate(const uint8_t* png, size_t len, uint8_t* out, size_t out_bytes, size_t* need);

/* BMP decode, tf.image.decode_image(file, channels=3) for BMP as TF 2.x's DecodeImageV2 does it
 * (decode_image_op.cc): the file's channels = bits-per-pixel / 8 in {1, 3, 4}, rows bottom-up
 * (top-down for a negative height) padded to 4 bytes; 24-bit BGR -> RGB, 32-bit BGRA -> RGB
 * (alpha dropped), 8-bit -> the stored byte replicated (TF applies no palette).  Other bit
 * depths and any compression but BI_RGB / BI_BITFIELDS (RLE, BI_JPEG, BI_PNG: bytes TF would
 * misread as pixels) return VTD_ERR_UNSUPPORTED.  Same
 * calling convention as the PNG / JPEG entry points; comps = 3. */
int vtd_bmp_info(const uint8_t* bmp, size_t len, int* h, int* w, int* comps);
int vtd_bmp_workspace_bytes(const uint8_t* const* bmps, const size_t* lens, int n,
                            int32_t* dims, size_t* bytes);
int vtd_bmp_decode(const uint8_t* const* bmps, const size_t* lens, int n, uint8_t* out_dev,
                   const int64_t* out_offsets, void* workspace_dev, size_t workspace_bytes,
                   void* stream);

/* ---------------------------------------------------------------- forward ------ */
/* model(images, training=False) (vtd.py:579-581, ipynb:836):
 * images NHWC fp32 [B][H][W][C] in [-1, 1] -> logits fp32 [B][17][6] (pre-sigmoid),
 * and, if dets_dev != NULL, transform_predictions(logits) fp32 [B][17][6]. */
int vtd_forward(const vtd_config* cfg, const vtd_weights* w, const float* images_dev,
                float* logits_dev, float* dets_dev, void* workspace_dev,
                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- metric ------- */
/* iou_calculator (vtd.py:761-875), elementwise over n box pairs.  Each box is the last
 * 4 floats (x, y, height, width) of a row of `stride` floats (stride 4: bare boxes;
 * stride 6: detection rows).  iou_dev: n floats.  Intersections follow the reference's
 * strict-inequality overlap test; IoU = inter / (union + 1e-8). */
int vtd_iou(const float* label_bbox_dev, const float* pred_bbox_dev, int64_t n, int stride,
            float* iou_dev, void* stream);

/* MeanAveragePrecision (vtd.py:1268-2060).  The state is the reference's three
 * Variables, caller-allocated in device memory:
 *   latest_positive_bboxes    float [VTD_MAP_CLASSES][VTD_MAP_LATEST][VTD_MAP_PER_IMAGE][2]
 *   labels_quantity_per_image float [VTD_MAP_CLASSES][VTD_MAP_LATEST]
 *   showed_up_classes         uint8 [VTD_MAP_CLASSES]
 * vtd_map_update = update_state(y_true, y_pred, use_transform_predictions=False)
 * (vtd.py:1310-1862): y_true / y_pred fp32 [batch][boxes][6] rows (objectness, class,
 * x, y, height, width); labels mark empty rows with class -8; y_pred is DECODED (run
 * vtd_decode first for raw logits).  One launch per batch, stream-ordered.
 * vtd_map_result = result() (vtd.py:1865-2049): out_dev fp32 [11] = the AP at IoU
 * thresholds linspace(0.5, 0.95, 10), then the mAP (their mean). */
#define VTD_MAP_CLASSES 80        /* Constants.CLASSES vtd.py:20 */
#define VTD_MAP_LATEST 3          /* Constants.LATEST_RELATED_IMAGES vtd.py:32 */
#define VTD_MAP_PER_IMAGE 14      /* Constants.BBOXES_PER_IMAGE vtd.py:37 */
#define VTD_MAP_MAX_BOXES 64      /* boxes per image accepted by vtd_map_update */
int vtd_map_reset(float* latest_positive_bboxes, float* labels_quantity_per_image,
                  uint8_t* showed_up_classes, void* stream);
int vtd_map_update(float* latest_positive_bboxes, float* labels_quantity_per_image,
                   uint8_t* showed_up_classes, const float* y_true_dev,
                   const float* y_pred_dev, int batch, int boxes, void* stream);
int vtd_map_result(const float* latest_positive_bboxes, const float* labels_quantity_per_image,
                   const uint8_t* showed_up_classes, float* out_dev, void* stream);

/* ---------------------------------------------------------------- loss --------- */
/* (ABI 17) The reference's validation loss: the forward values here, the gradients w.r.t.
 * the prediction below (vtd_loss_grad, vtd_ciou_grad, vtd_decode_grad).
 * ciou_calculator with diagonal_calculator (vtd.py:878-1015), elementwise over n box pairs,
 * same argument conventions as vtd_iou (the last 4 of `stride` floats are (x, y, height,
 * width)).  float32 in the reference's operation order:
 *   iou     = vtd_iou's value
 *   r_diou  = (rho / (c + 1e-8))^2, rho the centre distance, c the diagonal of the enclosing
 *             box (max - min of the four edges per axis: what the reference's sort yields)
 *   v       = (atan(w_l / (h_l + 1e-8)) - atan(w_p / (h_p + 1e-8)))^2 * 4 / pi2, pi2 the
 *             float32 square of float32(pi) (tf.square(np.pi), vtd.py:992)
 *   alpha   = v / ((1 - iou) + v + 1e-8)
 *   out_dev[i] = 1 - iou + r_diou + alpha v, or iou - r_diou when get_diou != 0. */
int vtd_ciou(const float* label_bbox_dev, const float* pred_bbox_dev, int64_t n, int stride,
             int get_diou, float* out_dev, void* stream);
/* diagonal_calculator (vtd.py:878-943) alone: out_dev[i] = c above. */
int vtd_diagonal(const float* label_bbox_dev, const float* pred_bbox_dev, int64_t n, int stride,
                 float* out_dev, void* stream);

/* my_custom_loss (vtd.py:1122-1265) of one batch.  y_true_dev / y_pred_dev: fp32
 * [B][boxes][6] rows (objectness, class, x, y, height, width), any boxes >= 1; labels mark
 * empty rows [0, -8, -8, -8, -8, -8].
 *   from_logits = 1: y_pred holds the model's raw logits, decoded inline by vtd_decode's own
 *     device function (bit-identical to vtd_decode followed by from_logits = 0);
 *   from_logits = 0: y_pred is decoded already (use_transform_predictions=False).
 * objectness_mean: over all B * boxes slots, the Keras 2.9 binary cross-entropy
 *   -(y log(p_c + 1e-7) + (1 - y) log(1 - p_c + 1e-7)), p_c = clip(p, 1e-7, 1 - 1e-7), times
 *   (1 - p_t)^2 with p_t = y p + (1 - y)(1 - p) of the unclipped p when focal_binary_loss
 *   (BinaryFocalCrossentropy, gamma 2, no class balancing, no label smoothing).
 * A slot is positive when isclose(y_true[..., 0], 1) (rtol 1e-5, atol 1e-8).  Over the
 * positive slots: classification_mean of (coefficient |class error|)^exponent (x * x when
 * exponent == 2) and ciou_mean of vtd_ciou's loss; both 0 when the batch has no positive
 * slot.  Only positive slots reach a division or an atan, every slot's clipped objectness
 * a log: the -8 padding meets none of them.
 *   total = objectness_mean + classification_mean * weight_classification
 *           + ciou_mean * weight_ciou
 * out_dev: fp32 [5] = total, objectness_mean, classification_mean, ciou_mean,
 * positive_count.  running_dev (nullable): double [2], the kernel adds total * B and B to it
 * -- the Keras loss metric's batch-size weighted mean is running[0] / running[1].
 * Per-slot values are float32 in the reference's operation order; the sums run in fp64 in
 * a fixed order inside one workgroup (no float atomics, no grid-size dependence): the same
 * inputs give the same bits on every run.  One launch, stream-ordered, no host
 * synchronisation.  B == 0 writes zeros to out_dev and leaves running_dev alone.
 * VTD_ERR_INVALID_ARG, before any device call: a NULL p / out_dev / (B > 0) input pointer,
 * B < 0, boxes <= 0, a non-finite or negative coefficient. */
typedef struct vtd_loss_params {
  int focal_binary_loss;        /* 1: BinaryFocalCrossentropy, 0: BinaryCrossentropy  */
  float coefficient;            /* classification loss (coefficient * error)^exponent  */
  float exponent;
  float weight_classification;
  float weight_ciou;
  int from_logits;              /* 1: y_pred are logits (use_transform_predictions)   */
} vtd_loss_params;
int vtd_loss(const float* y_true_dev, const float* y_pred_dev, int B, int boxes,
             const vtd_loss_params* p, float* out_dev, double* running_dev, void* stream);

/* Gradients of the loss (additions to ABI 17; nothing above changes).  Analytic float32
 * derivatives of the graph the reference builds, w.r.t. the prediction; labels are
 * constants.  The derivatives, DESIGN.md "Loss gradients":
 *   objectness: d/dp of the cross-entropy on p_c = clip(p, 1e-7, 1 - 1e-7) -- the clip passes
 *     gradient on its closed interval, 0 outside -- and of the focal factor (1 - p_t)^2
 *     through the unclipped p; times 1 / (B * boxes);
 *   class, positive slots only: exponent coefficient (coefficient |d|)^(exponent - 1) sign(d),
 *     sign(0) = 0; times weight_classification / positives;
 *   CIoU, positive slots only: through iou, r_diou, v and alpha (no stop_gradient); the
 *     reference's edge sorts route gradient to whichever edge lands at a position (ties as a
 *     stable sort); the intersection only under the intersect condition; times weight_ciou /
 *     positives;
 *   from_logits = 1: times scale_f s (1 - s) of the decode, s vtd_decode's own sigmoid;
 *     from_logits = 0: the gradient is w.r.t. the decoded prediction.
 * Two deliberate deviations from autodiff of the reference: r_diou is differentiated as
 * (dx^2 + dy^2) / (c + 1e-8)^2 (the same value; the reference's sqrt gives 0/0 at coincident
 * centres, this form 0 in x and y), and at a kink (tied edges, zero class error, boxes that
 * just touch) one of the one-sided derivatives is returned.  Every result is finite for
 * finite inputs with positive box sizes, and bit-identical from run to run.
 *
 * vtd_loss_grad: vtd_loss's out_dev[5], bit for bit, and grad_dev fp32 [B][boxes][6] =
 * d total / d y_pred in ONE launch (one workgroup: vtd_loss's loop also writes each slot's
 * unscaled derivatives, the positive count goes through LDS, then every thread rescales the
 * slots it wrote itself; one writer per element, no atomics).  upstream_dev (nullable): one device float that multiplies the gradient, so a
 * chained backward needs no host read.  Non-positive slots get exactly 0 in channels 1..5.
 * Arguments as vtd_loss, plus: exponent must be finite and >= 1 (below 1 the class
 * derivative is unbounded at a zero class error).  B == 0 zeroes out_dev and launches
 * nothing else. */
int vtd_loss_grad(const float* y_true_dev, const float* y_pred_dev, int B, int boxes,
                  const vtd_loss_params* p, const float* upstream_dev, float* out_dev,
                  float* grad_dev, void* stream);
/* d vtd_ciou / d pred_bbox (the CIoU loss, or the DIoU with get_diou), elementwise:
 * grad_dev fp32 [n][stride], the leading stride - 4 channels 0, the last four times
 * upstream_dev[i] (fp32 [n], nullable = 1).  Arguments as vtd_ciou; n == 0 is a no-op. */
int vtd_ciou_grad(const float* label_bbox_dev, const float* pred_bbox_dev, int64_t n,
                  int stride, int get_diou, const float* upstream_dev, float* grad_dev,
                  void* stream);
/* d vtd_decode: grad_dev[i] = upstream_dev[i] * scale_f s (1 - s), fp32 [n][6] each (the
 * [0, 1] clip never closes on a sigmoid).  n == 0 is a no-op. */
int vtd_decode_grad(const float* logits_dev, const float* upstream_dev, int64_t n,
                    float* grad_dev, void* stream);

/* ---------------------------------------------------------------- head backward - */
/* Backward through the detection head (additions to ABI 17; nothing above changes): the
 * weight and input gradients of mlp_head (vtd.py:417-495) given d loss / d logits
 * (vtd_loss_grad), DESIGN.md "Head backward".  dtype below is VTD_BF16 or VTD_BF16X3; any
 * other value returns VTD_ERR_UNSUPPORTED.
 *
 * vtd_gemm_wgrad: the weight gradient of a Dense layer, contracting over the ROW index of
 * both operands:
 *   dW[k][n] = sum_m X[m][k] * G[m][n]   (k < K, n < N; fp32, row-major [K][ldw]: the Keras
 *              kernel layout),  db[n] = sum_m G[m][n]  (db_dev nullable).
 * X, G in `dtype`, exactly as the forward's producers and vtd_act_grad store them:
 *   VTD_BF16: bf16 rows, ldx >= K, ldg >= N, both % 8 == 0;
 *   VTD_BF16X3: the split-bf16 A operand [hi | lo] with piece width ld / 2 (>= K resp. N),
 *     ld % 16 == 0; dW = Xhi^T Ghi + Xlo^T Ghi + Xhi^T Glo, db from hi + lo.
 * X_dev and G_dev 16-byte aligned; fp32 accumulation.  M is arbitrary: rows beyond M
 * contribute zero (nothing is read past row M - 1).  Padding rule: K and N are the logical
 * sizes; the kernel writes rows [0, K) of dW in full -- columns [N, ldw) of each as zero -- and
 * nothing else.  A caller that wants a padded dW passes the padded K: the pad columns [K_real,
 * K) of X are zero in every operand this library produces, so those rows come out zero.
 * The grid is output tiles x `msplit` ranges of M (of ceil(M / 32) / msplit 32-row steps each):
 * msplit == 1 writes dW directly; msplit > 1 writes fp32 partials to part_dev
 * (part_bytes >= msplit * (K + 1) * N * 4; row K of each partial is its db) and one pass sums
 * them in range order.  1 <= msplit <= min(ceil(M / 32), 256).  No atomics: the same inputs
 * give the same bits on every run (the bits may differ between msplit values, as the order of
 * the fp32 sum does).  vtd_gemm_wgrad_choice: the msplit vtd_head_backward uses.
 * VTD_ERR_INVALID_ARG before any device call: a null X / G / dW (or part_dev with msplit > 1),
 * non-positive sizes, the ld / alignment rules above, ldw < N, msplit out of range, part_bytes
 * too small. */
int vtd_gemm_wgrad(int M, int K, int N, const void* X_dev, int ldx, const void* G_dev, int ldg,
                   int dtype, float* dW_dev, int ldw, float* db_dev, float* part_dev,
                   size_t part_bytes, int msplit, void* stream);
int vtd_gemm_wgrad_choice(int M, int K, int N, int dtype);

/* a = act(z): z fp32 [rows][ldz] (first N columns) -> a_dev in `dtype` form [rows][lda]: bf16
 * (lda >= N, lda % 8 == 0) or split-bf16 [hi | lo] (piece width lda / 2 >= N, lda % 16 == 0),
 * 16-byte aligned; the columns [N, piece width) written as zero.  The activation is the GEMM
 * epilogue's own device function (bit-identical); VTD_ACT_NONE converts only (for
 * VTD_BF16X3 what vtd_split_bf16x3 role 0 writes).  The training forward of the head runs its
 * Dense layers with VTD_ACT_NONE into fp32 z, keeps z, and applies this. */
int vtd_act_forward(const float* z_dev, int64_t rows, int N, int ldz, int act, void* a_dev,
                    int lda, int dtype, void* stream);
/* gz = ga * act'(z): z [rows][ldz], ga [rows][ldga] fp32 -> gz_dev in `dtype` form as above --
 * the A operand of the input-gradient GEMM and the G operand of vtd_gemm_wgrad.  The
 * derivatives use the forward's exp2 / rcp formulation (GELU-tanh through s = 1 / (1 + 2^(x (c0
 * + c1 x^2))), Mish through n = e (e + 2)); finite for every finite z, exactly 1 for Mish
 * where the forward returns x (z > 20); within 1e-5 of the fp64 derivative. */
int vtd_act_grad(const float* z_dev, int ldz, const float* ga_dev, int ldga, int64_t rows, int N,
                 int act, void* gz_dev, int ldgz, int dtype, void* stream);
/* Inverse of the Reshape scatter epilogue (vtd_epilogue.scatter_tokens, vtd.py:461-463):
 * dU fp32 [B * 17][ldu] (ldu >= T) -> dT [B * T][ldt] in `dtype` form (piece width >= 17):
 * element (b T + t, n < 17) = dU[b * 17 + f / T][f % T], f = t * 17 + n; the columns from 17
 * to the piece width zero. */
int vtd_head_unscatter(const float* dU_dev, int B, int T, int ldu, void* dT_dev, int ldt,
                       int dtype, void* stream);

/* Stages 0 .. L of vtd_forward (patches, projection, the encoder layers: the same parts, streams
 * and workspace, vtd_workspace_bytes) and then, instead of the head, the residual stream after
 * the last layer -- Keras layer `encoded_images` -- as fp32 [B * N][d], unpadded.  (VTD_BF16 /
 * VTD_FP8: the stream is held in bf16; these are its values.) */
int vtd_forward_encoded(const vtd_config* cfg, const vtd_weights* w, const float* images_dev,
                        float* encoded_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream);

/* The head's weights, fp32 device arrays in the Keras layout, unpadded: kernels [K][N]
 * row-major, biases [N].  w_det / b_det: `dense` [d][17]; w_head[j] / b_head[j], j <
 * vtd_dims.n_head: `dense_{j+1}` [tokens or head_units[j-1]][head_units[j]]; w_final / b_final:
 * `MLP_Head_no_Sigmoid` [head_units[n_head-1]][6].  vtd_head_grads: outputs of the same shapes,
 * and d_encoded fp32 [B * N][d] = d loss / d encoded_images (nullable: not computed). */
typedef struct vtd_head_params {
  const float* w_det; const float* b_det;
  const float* w_head[VTD_MAX_HEAD]; const float* b_head[VTD_MAX_HEAD];
  const float* w_final; const float* b_final;
} vtd_head_params;
typedef struct vtd_head_grads {
  float* w_det; float* b_det;
  float* w_head[VTD_MAX_HEAD]; float* b_head[VTD_MAX_HEAD];
  float* w_final; float* b_final;
  float* d_encoded;
} vtd_head_grads;
/* One call: the training forward of the head from encoded_dev (fp32 [B * N][d], as
 * vtd_forward_encoded writes it) keeping every pre-activation z and activation, then the
 * backward from dlogits_dev (fp32 [B][17][6]) into *g.  logits_dev (nullable): the training
 * forward's logits.  dlogits_dev NULL (logits_dev then required, g ignored): the training
 * forward alone, for the logits the loss gradient is taken at.  Weights change every step, so the call converts what it needs into the
 * workspace itself (W^T for the forward GEMMs, the [K][N] form for the input-gradient GEMMs).
 * cfg->dtype VTD_BF16X3 or VTD_BF16 (else VTD_ERR_UNSUPPORTED); every Dense product runs in
 * that mode's operands with fp32 accumulation.  Asynchronous on `stream` (one part, no side
 * streams), no allocation, no host synchronisation, bit-identical from run to run.
 * ws_bytes >= vtd_head_backward_workspace_bytes (else VTD_ERR_WORKSPACE). */
int vtd_head_backward_workspace_bytes(const vtd_config* cfg, size_t* bytes);
int vtd_head_backward(const vtd_config* cfg, const vtd_head_params* w, const float* encoded_dev,
                      const float* dlogits_dev, float* logits_dev, const vtd_head_grads* g,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- attention backward (VTD_BF16 / VTD_BF16X3; any other dtype VTD_ERR_UNSUPPORTED)
 * vtd_attention_train: vtd_attention that also writes lse_dev, fp32 [B][heads][N]:
 * lse[b][h][i] = ln sum_j exp(scale q_i.k_j), natural units, finite whenever the scores are.
 * It runs the streaming kernels of vtd_attention (VTD_BF16X3 at the default; VTD_BF16 as
 * under VTD_KNOB_ATTN_VARIANT 2) with the LSE store compiled in: out_dev has the same bits. */
int vtd_attention_train(const void* qkv_dev, int B, int N, int heads, int dkp, int ldqkv,
                        float scale, void* out_dev, int ldo, float* lse_dev, int dtype,
                        void* stream);
/* dqkv = d loss / d qkv of the attention core from do_dev = d loss / d O.
 *   qkv_dev  as the forward read it: bf16 (VTD_BF16) or fp32 (VTD_BF16X3), [B*N][ldqkv];
 *   o_dev    as the forward wrote it: bf16 [B*N][ldo], or the split [hi | lo] operand (piece
 *            width ldo / 2);
 *   do_dev   bf16 (VTD_BF16) or fp32 (VTD_BF16X3) [B*N][lddo], head h at column h*dkp.  The
 *            pad columns [key_dim, dkp) of a head are READ: the caller keeps them zero (they
 *            are after the attention-output input-gradient GEMM, whose packed w_out has zero
 *            rows there), as the pad columns of qkv are everywhere in this library;
 *   lse_dev  from vtd_attention_train on the same qkv and scale.
 * dqkv_dev has qkv's column layout and is written in `dtype` form exactly as vtd_act_grad
 * writes gz: bf16 rows (lddqkv % 8 == 0), or split [hi | lo] with piece width lddqkv / 2
 * (lddqkv % 16 == 0), 16-byte aligned -- directly the A operand of the qkv input-gradient GEMM
 * and the G operand of vtd_gemm_wgrad.  For rows < B*N the columns [0, 3 heads dkp) of each
 * piece are written in full (pad columns of a head come out zero); nothing else is written.
 * P = exp(scale q.k - lse) is recomputed, never stored as N x N:
 *   delta_i = sum_d dO_id O_id, dP = dO V^T, dS = P o (dP - delta) scale,
 *   dV = P^T dO, dK = dS^T Q, dQ = dS K,
 * each product one bf16 MFMA product (VTD_BF16) or the three hi.hi + lo.hi + hi.lo
 * (VTD_BF16X3; P and dS split as the forward splits P), fp32 accumulation and statistics.
 * No atomics and no workgroup waiting on another: dK, dV come from a key-stationary pass, dQ
 * from a second, query-stationary pass; bit-identical from run to run.  VTD_BF16X3 divides the
 * recomputed P by its own row sums (one more sweep of the keys), so the rounding of lse, one
 * fp32 number per row, does not reach the gradients.  Nothing is read past row B*N - 1.  Within 2e-4 (VTD_BF16X3) / 5e-2 (VTD_BF16) of max |gradient| per tensor
 * against fp64 (tests/test_gpu_attention_backward.py).
 * ld rules: ldqkv, lddo multiples of 8 (>= 3 heads dkp, >= heads dkp); ldo as vtd_attention
 * writes it; every base 16-byte aligned; scale positive and finite; else VTD_ERR_INVALID_ARG,
 * before any device call.  ws_bytes >= vtd_attention_backward_workspace_bytes (delta, and in
 * VTD_BF16X3 the reciprocal row sums: fp32 [B][heads][N] each), else VTD_ERR_WORKSPACE.  Asynchronous on `stream`, no allocation, no host
 * synchronisation. */
int vtd_attention_backward_workspace_bytes(int B, int N, int heads, int dkp, int dtype,
                                           size_t* bytes);
int vtd_attention_backward(const void* qkv_dev, const void* o_dev, const void* do_dev,
                           const float* lse_dev, int B, int N, int heads, int dkp, int ldqkv,
                           int ldo, int lddo, float scale, void* dqkv_dev, int lddqkv, int dtype,
                           void* ws_dev, size_t ws_bytes, void* stream);

/* ---- dropout (an addition to ABI 17; DESIGN.md "Dropout")
 * Keras Dropout semantics: a kept value is multiplied by inv_keep, a dropped one is +0.  The
 * mask is generated inside the kernels by Philox4x32-10 and never stored; a mask bit is a pure
 * function of (seed, step, site, logical index) -- (row, column) of the unpadded [rows][N]
 * activation at an elementwise site, (image, head, query, key) at an attention site -- and of
 * nothing else (no leading dimension, padding, batch size, kernel variant or backward pass).
 * rate is realised as thr / 65536, thr = round(rate * 65536) <= 65535; inv_keep is the fp32
 * rounding of 1 / (1 - thr / 65536), exactly 2 at rate 0.5.  TensorFlow's random stream is not
 * reproduced: the distribution is the reference's, the bits are this library's.
 * Every entry below returns VTD_ERR_INVALID_ARG before any device call for a NULL vtd_dropout
 * or a rate outside [0, 1) (NaN included); rate == 0 takes the existing entry's path (the same
 * launches, the same bits). */
typedef struct vtd_dropout { uint64_t seed, step; uint32_t site; float rate; } vtd_dropout;
/* the mask as bytes (1 = kept), through the kernels' own device function: out [rows][ldo]
 * (columns < N written) and out [B][heads][N][N] */
int vtd_dropout_mask(const vtd_dropout* drop, int64_t rows, int N, uint8_t* out_dev, int ldo,
                     void* stream);
int vtd_dropout_mask_attention(const vtd_dropout* drop, int B, int heads, int N, uint8_t* out_dev,
                               void* stream);
/* y = drop(x), fp32 [rows][ldx] -> fp32 [rows][ldy], columns < N: y = fp32(x * inv_keep) or +0.
 * The layer's gradient is the same call on the incoming gradient. */
int vtd_dropout_apply(const vtd_dropout* drop, const float* x_dev, int ldx, int64_t rows, int N,
                      float* y_dev, int ldy, void* stream);
/* vtd_act_forward / vtd_act_grad with the mask of (row, column): a = drop(act(z)) and
 * gz = act'(z) * (m * inv_keep * ga): one fp32 multiply by inv_keep before the single rounding
 * into the stored form; pad columns zero as before. */
int vtd_act_forward_dropout(const float* z_dev, int64_t rows, int N, int ldz, int act, void* a_dev,
                            int lda, int dtype, void* stream, const vtd_dropout* drop);
int vtd_act_grad_dropout(const float* z_dev, int ldz, const float* ga_dev, int ldga, int64_t rows,
                         int N, int act, void* gz_dev, int ldgz, int dtype, void* stream,
                         const vtd_dropout* drop);
/* vtd_attention_train / vtd_attention_backward with dropout on the attention probabilities
 * (the MultiHeadAttention `dropout`): O = ((P o M) inv_keep) V.  The softmax statistics, the
 * normalisation and lse_dev are those of the undropped softmax (lse_dev has vtd_attention_train's
 * bits); only the operand of the P V product is masked.  Backward, from the dropped O:
 *   delta_i = sum_d dO_id O_id (unchanged: sum_j P_ij dP_ij = dO_i . O_i still holds),
 *   dP = M inv_keep (dO V^T), dS = P (dP - delta) scale with the unmasked P,
 *   dV = (P o M inv_keep)^T dO, dK, dQ from dS as before.
 * The same (seed, step, site) as the forward regenerates its mask; nothing N x N is stored and
 * the workspace is vtd_attention_backward_workspace_bytes.  Bit-identical from run to run. */
int vtd_attention_train_dropout(const void* qkv_dev, int B, int N, int heads, int dkp, int ldqkv,
                                float scale, void* out_dev, int ldo, float* lse_dev, int dtype,
                                void* stream, const vtd_dropout* drop);
int vtd_attention_backward_dropout(const void* qkv_dev, const void* o_dev, const void* do_dev,
                                   const float* lse_dev, int B, int N, int heads, int dkp,
                                   int ldqkv, int ldo, int lddo, float scale, void* dqkv_dev,
                                   int lddqkv, int dtype, void* ws_dev, size_t ws_bytes,
                                   void* stream, const vtd_dropout* drop);
/* ---- LayerNorm backward (an addition to ABI 17; DESIGN.md "Encoder block backward")
 * The gradients of keras LayerNormalization(axis=-1) given d loss / d y, all fp32 (in training
 * the residual stream and its gradient are fp32 in every operand mode, so there is no dtype):
 *   xhat = (x - mean) rstd, gy = dy gamma,
 *   dx = rstd ((gy - mean_D(gy)) - xhat mean_D(gy xhat)) [+ add],
 *   dgamma = sum_rows dy xhat, dbeta = sum_rows dy.
 * x_dev [rows][ldx]: the forward's input rows; stat_dev: (mean, rstd) per row as
 * vtd_layernorm_stats writes them, 8-byte aligned; gamma_dev [D]; dy_dev [rows][lddy];
 * add_dev [rows][ldadd] (nullable): the gradient that reaches the same tensor along the
 * residual connection, added to dx in the same pass; dx_dev [rows][lddx] may be the very buffer
 * add_dev is (same base, same leading dimension) and overlaps no other argument.  dgamma_dev,
 * dbeta_dev [D]: both or neither; without them no workspace is needed (ws_dev may be NULL).
 * Nothing is read in rows >= `rows` or columns >= D; exactly the rows x D elements of dx and
 * the D elements of dgamma and of dbeta are written, so pad columns up to lddx keep their
 * bytes.  Every operation rounds once in fp32 (no FMA contraction); the row means are summed
 * per lane in column order and across the wave as the forward's statistics are.
 * dgamma / dbeta use no atomics and no workgroup waits on another: the rows are cut into
 * vtd_layernorm_backward_workspace_bytes / (8 D) contiguous ranges -- a function of `rows`
 * alone, never of the device -- each range's sums are written as one fp32 [2][D] plane of the
 * workspace and a second kernel adds the planes in range order: the same inputs give the same
 * bits on every run.  Rows with 16-byte aligned x / gamma / dy / add / dx, D % 4 == 0, D <= 4096
 * and leading dimensions that are multiples of 4 take the vector kernels; anything else a
 * generic path with the same summation order for dgamma / dbeta.
 * VTD_ERR_INVALID_ARG before any device call: a null x / stat / gamma / dy / dx (or workspace
 * when dgamma is given), a non-positive size, a leading dimension below D, dgamma without
 * dbeta or the reverse, stat not 8-byte, another pointer not 4-byte or the workspace not
 * 16-byte aligned.  ws_bytes below vtd_layernorm_backward_workspace_bytes (with dgamma given):
 * VTD_ERR_WORKSPACE.  Asynchronous on `stream`, no allocation, no host synchronisation. */
int vtd_layernorm_backward_workspace_bytes(int64_t rows, int D, size_t* bytes);
int vtd_layernorm_backward(const float* x_dev, int ldx, const float* stat_dev,
                           const float* gamma_dev, const float* dy_dev, int lddy,
                           const float* add_dev, int ldadd, int64_t rows, int D, float* dx_dev,
                           int lddx, float* dgamma_dev, float* dbeta_dev, void* ws_dev,
                           size_t ws_bytes, void* stream);

/* ---- encoder block backward (additions to ABI 17; DESIGN.md "Encoder block backward")
 * One encoder block of the reference with dropout=None (vtd.py:350-412):
 *   x1 = x + MultiHeadAttention(LN1(x)),  y = x1 + MLP(LN2(x1)),
 * LayerNormalization epsilon 1e-3, attention scale 1 / sqrt(key_dim), the MLP of
 * mlp_quantities Dense + activation layers of widths d 2^(q-1) ... d.  dtype VTD_BF16X3 or
 * VTD_BF16 (any other value: VTD_ERR_UNSUPPORTED): every Dense product and the attention core
 * run in that mode's operands; the residual stream x, x1, y and its gradient are fp32 in both.
 *
 * vtd_block_params: the block's weights, const fp32 device arrays in the Keras layout, unpadded:
 * ln1 / ln2 gamma, beta [d]; wq, wk, wv [d][num_heads][key_dim], bq, bk, bv [num_heads][key_dim];
 * wo [num_heads][key_dim][d], bo [d]; w_mlp[j] [K_j][N_j] (K_0 = d, K_j = N_{j-1}), b_mlp[j]
 * [N_j].  vtd_block_grads: outputs of the same shapes, and dx fp32 [rows][d] = d loss / d x
 * (nullable: not written). */
typedef struct vtd_block_dims {   /* one encoder block, vtd.py:350-412 */
  int batch, tokens;              /* rows = batch * tokens */
  int d, num_heads, key_dim;
  int mlp_quantities;             /* widths d * 2^(q-1) ... d, as the reference */
  int use_mish;                   /* 1 Mish, 0 tanh-GELU */
  int dtype;                      /* VTD_BF16X3 | VTD_BF16 */
} vtd_block_dims;
typedef struct vtd_block_params {
  const float* ln1_gamma; const float* ln1_beta;
  const float* wq; const float* bq; const float* wk; const float* bk;
  const float* wv; const float* bv; const float* wo; const float* bo;
  const float* ln2_gamma; const float* ln2_beta;
  const float* w_mlp[VTD_MAX_MLP]; const float* b_mlp[VTD_MAX_MLP];
} vtd_block_params;
typedef struct vtd_block_grads {
  float* ln1_gamma; float* ln1_beta;
  float* wq; float* bq; float* wk; float* bk;
  float* wv; float* bv; float* wo; float* bo;
  float* ln2_gamma; float* ln2_beta;
  float* w_mlp[VTD_MAX_MLP]; float* b_mlp[VTD_MAX_MLP];
  float* dx;
} vtd_block_grads;
/* One call: the training forward of the block from x_dev (fp32 [rows][d], unpadded) keeping
 * every pre-activation in the workspace (the LayerNorm statistics, LN outputs in operand form,
 * qkv, the attention output and its lse, x1, every MLP z_j and activation), then the backward
 * from dy_dev (fp32 [rows][d] = d loss / d y) into *grads, in the order MLP (vtd_act_grad,
 * vtd_gemm_wgrad, input-gradient vtd_gemm), LayerNorm 2 with the residual gradient as `add`,
 * attention-output Dense, vtd_attention_backward, query/key/value Dense, LayerNorm 1 with the
 * residual gradient.  y_dev (nullable): the block's output, fp32 [rows][d].  dy_dev NULL (y_dev
 * then required, grads ignored): the training forward alone; the same launches, so y has the
 * same bits either way.  Weights change every step, so the call converts what it needs into the
 * workspace itself: the three query/key/value kernels are gathered into both operand forms of
 * the fused, per-head padded matrix, wo likewise, and the fused gradients are un-gathered into
 * the Keras-shaped outputs.  Asynchronous on `stream` (one stream), no allocation, no host
 * synchronisation, no atomics, bit-identical from run to run.
 * VTD_ERR_INVALID_ARG before any device call: a null dims / params / x / workspace / weight
 * pointer (with dy_dev: grads and any gradient pointer but dx; without: y_dev), non-positive
 * sizes, mlp_quantities > VTD_MAX_MLP, key_dim > 128, an MLP width of 2^24 or more,
 * batch * tokens >= 2^31; VTD_ERR_UNSUPPORTED: a dtype other than the two;
 * ws_bytes < vtd_encoder_block_backward_workspace_bytes: VTD_ERR_WORKSPACE. */
int vtd_encoder_block_backward_workspace_bytes(const vtd_block_dims* dims, size_t* bytes);
int vtd_encoder_block_backward(const vtd_block_dims* dims, const vtd_block_params* params,
                               const float* x_dev, const float* dy_dev, float* y_dev,
                               const vtd_block_grads* grads, void* ws, size_t ws_bytes,
                               void* stream);

/* vtd_encoder_block_backward with the reference's `dropout` in the block
 * (vtd.py:359-369, 404-405): site_base is the attention probabilities' site, site_base + 1 + j
 * the Dropout after MLP layer j's activation -- the last layer's too, before the residual add
 * (y = x1 + drop(act(z_last))).  The backward's recomputed training forward regenerates the
 * forward's masks from the same (seed, step, site_base).  Same workspace
 * (vtd_encoder_block_backward_workspace_bytes), same checks; in addition VTD_ERR_INVALID_ARG
 * before any device call for a NULL drop, a rate outside [0, 1) or site_base + mlp_quantities
 * beyond 32 bits.  rate == 0: vtd_encoder_block_backward's launches and bits.  Blocks chained in
 * one model take distinct site_base values, i * (1 + mlp_quantities) for block i. */
typedef struct vtd_block_dropout { uint64_t seed, step; uint32_t site_base; float rate; } vtd_block_dropout;
int vtd_encoder_block_backward_dropout(const vtd_block_dims* dims, const vtd_block_params* params,
                                       const float* x_dev, const float* dy_dev, float* y_dev,
                                       const vtd_block_grads* grads, void* ws, size_t ws_bytes,
                                       void* stream, const vtd_block_dropout* drop);

/* vtd_head_backward with the reference's Dropout after every head Dense + activation
 * (mlp_head, vtd.py:468-486): drop->site_base + j is the site of head layer j, 0 <= j < n_head
 * (vtd_dims.n_head, repeats included).  None follows Dense(17) or MLP_Head_no_Sigmoid.  The site
 * is an elementwise one over the unpadded [batch * 17][head_units[j]] activation, row b * 17 + r:
 * vtd_dropout_mask(rows = batch * 17, N = head_units[j]); head_units_p and leading dimensions
 * never enter.  The forward-only call (dlogits_dev NULL) and the forward + backward call
 * regenerate the same masks from the same (seed, step, site_base).  Same workspace
 * (vtd_head_backward_workspace_bytes), same checks; in addition VTD_ERR_INVALID_ARG before any
 * device call for a NULL drop, a rate outside [0, 1) (NaN included) or site_base + n_head beyond
 * 32 bits.  rate == 0: vtd_head_backward's launches and bits.  In one model the head's site_base
 * is repeat_times * (1 + mlp_quantities), after the blocks' sites. */
int vtd_head_backward_dropout(const vtd_config* cfg, const vtd_head_params* w,
                              const float* encoded_dev, const float* dlogits_dev,
                              float* logits_dev, const vtd_head_grads* g, void* ws,
                              size_t ws_bytes, void* stream, const vtd_block_dropout* drop);

/* ---- patch embedding backward (additions to ABI 17; DESIGN.md "Whole-model gradients")
 * The stem of the reference (transformer_preprocessor, vtd.py:271-307):
 *   x0[b N + n][j] = sum_k patches[b N + n][k] W[k][j] + bias[j] + pos[n],
 * patches by tf.image.extract_patches (SAME zero pad, (kh, kw, c) order), the position
 * embedding Keras's (tokens, 1), broadcast over d.  tokens = ceil(H / patch) ceil(W / patch) and
 * patch_dim = patch^2 C are derived inside.  dtype VTD_BF16X3 or VTD_BF16 (any other value:
 * VTD_ERR_UNSUPPORTED): the operands of the two products; x0 and every gradient are fp32.
 * vtd_stem_params: const fp32 device arrays in the Keras layout, unpadded: pos [tokens], w
 * [patch_dim][d], b [d].  vtd_stem_grads: outputs of the same shapes. */
typedef struct vtd_stem_dims {
  int batch, H, W, C;             /* images fp32 [batch][H][W][C] */
  int patch, d;
  int dtype;                      /* VTD_BF16X3 | VTD_BF16 */
} vtd_stem_dims;
typedef struct vtd_stem_params { const float* pos; const float* w; const float* b; } vtd_stem_params;
typedef struct vtd_stem_grads { float* pos; float* w; float* b; } vtd_stem_grads;
/* Forward only (dx0_dev NULL; x0_dev required, grads ignored): vtd_extract_patches into the
 * workspace in the mode's operand form, the kernel converted to W^T there (weights change every
 * step), one vtd_gemm with the bias and the rowadd epilogue into x0_dev, fp32 [batch tokens][d],
 * unpadded.  Backward (dx0_dev fp32 [batch tokens][d] = d loss / d x0): the patches again; when
 * x0_dev is given also the rest of the forward, the same launches, so x0 has the same bits
 * either way; then one pass over dx0 that writes its rows in operand form (exactly what
 * vtd_act_forward(VTD_ACT_NONE) writes) and their sums, vtd_gemm_wgrad for grads->w and
 * grads->b, and grads->pos[n] = the row sums added over the batch in order.  Asynchronous on
 * `stream` (one stream), no allocation, no host synchronisation, no atomics, bit-identical from
 * run to run; exactly the elements of the outputs are written.
 * VTD_ERR_INVALID_ARG before any device call: a null dims / params / images / workspace / weight
 * pointer (with dx0_dev: grads and any gradient pointer; without: x0_dev), non-positive sizes,
 * batch * tokens >= 2^31, d or patch_dim of 2^24 or more, a workspace, x0, params->w or
 * params->b not 16-byte aligned or any other array not 4-byte aligned; VTD_ERR_UNSUPPORTED: a
 * dtype other than the two; ws_bytes < vtd_stem_backward_workspace_bytes: VTD_ERR_WORKSPACE. */
int vtd_stem_backward_workspace_bytes(const vtd_stem_dims* dims, size_t* bytes);
int vtd_stem_backward(const vtd_stem_dims* dims, const vtd_stem_params* params,
                      const float* images_dev, const float* dx0_dev, float* x0_dev,
                      const vtd_stem_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* The image gradient (an addition to ABI 17; DESIGN.md "Image gradient"): dimages_dev fp32
 * [batch][H][W][C] = d loss / d images from dx0_dev fp32 [batch tokens][d] = d loss / d x0 and
 * w_dev, the linear_projection kernel in the Keras layout [patch_dim][d].  dims as above; the
 * images themselves are not read (the stem is linear in them).  Launches: the pass over dx0 of
 * vtd_stem_backward (its rows in operand form; the row sums go to scratch), the kernel converted
 * to the mode's B operand as stored ([patch_dim_p][d_p], what vtd_head_backward makes for its
 * input gradients), one vtd_gemm dP = dx0 W^T into fp32 [batch tokens][patch_dim_p] in the
 * workspace, and one kernel that applies the adjoint of tf.image.extract_patches(SAME):
 *   dimages[b][y][x][c] = dP[b tokens + py gw + px][(ky patch + kx) C + c],
 *   py = (y + pad_top) / patch, ky = (y + pad_top) % patch, likewise in x, pad_before =
 *   floor(pad / 2) as vtd_extract_patches pads.
 * Every image element has one source and is written once; the gradient that falls on the zero
 * pad is dropped.  Asynchronous on `stream` (one stream), no allocation, no host
 * synchronisation, no atomics, bit-identical from run to run; exactly the elements of
 * dimages_dev are written.  vtd_stem_backward and this entry share nothing: each has its own
 * workspace size, and neither changes the other's outputs.
 * VTD_ERR_INVALID_ARG before any device call: a null dims / w / dx0 / dimages / workspace
 * pointer, non-positive sizes, batch * tokens >= 2^31, d or patch_dim of 2^24 or more, a
 * workspace or w_dev not 16-byte aligned, dx0_dev or dimages_dev not 4-byte aligned;
 * VTD_ERR_UNSUPPORTED: a dtype other than the two; ws_bytes <
 * vtd_stem_image_grad_workspace_bytes (a multiple of 256, monotone in batch): VTD_ERR_WORKSPACE. */
int vtd_stem_image_grad_workspace_bytes(const vtd_stem_dims* dims, size_t* bytes);
int vtd_stem_image_grad(const vtd_stem_dims* dims, const float* w_dev, const float* dx0_dev,
                        float* dimages_dev, void* ws, size_t ws_bytes, void* stream);

/* ---- optimizer step: keras.optimizers.Adam + the ClipWeight constraint + the operand re-pack,
 * ONE kernel over a table of tensors.  The table entry is vtd_train_tensor (below);
 * vtd_adam_tensor is the ungrouped, always-constrained, dense-rule form of vtd_train_tensor:
 *   k_group = K, k_group_p = K_p, n_group = n_group_p = N, row_offset = 0, constrain = 1,
 *   rule = VTD_TRAIN_RULE_DENSE, packed_dtype = packed ? VTD_TRAIN_PACK_MODE : VTD_TRAIN_PACK_NONE
 * and the vtd_adam_* entries are adapters that convert their table and run the vtd_train_* code:
 * the same checks, plan layout, kernel and bits.
 * One tensor: w, m, v (updated in place) and g (read only), fp32 device arrays in the Keras
 * layout with 16-B aligned bases.  VTD_ADAM_MATRIX: a kernel [K][N] row-major; `packed`
 * (nullable: update the master only) is the forward's operand W^T [N_p][ld] of it -- VTD_BF16:
 * bf16 rows, K_p = ld; VTD_BF16X3: the split-bf16 B operand [hi | hi | lo] with piece width
 * K_p = ld / 3 -- 16-B aligned, K_p >= K, K_p % 8 == 0.  VTD_ADAM_VECTOR: a bias [N] (K and ld
 * unused); `packed` (nullable) is the fp32 padded vector vtd_pack_vector writes, 4-B aligned. */
enum { VTD_ADAM_MATRIX = 0, VTD_ADAM_VECTOR = 1 };
typedef struct vtd_adam_tensor {
  float* w; float* m; float* v; const float* g;
  void* packed;
  int kind, K, N, ld;
} vtd_adam_tensor;
/* The full table entry: what expresses every operand Model._pack builds with vtd_pack_dense /
 * vtd_pack_vector, a per-tensor destination format, constraint flag and update rule.
 *   VTD_ADAM_MATRIX [K][N]: element (k, n) goes to packed row
 *     row_offset + (n / n_group) * n_group_p + n % n_group, packed column
 *     k' = (k / k_group) * k_group_p + k % k_group (vtd_pack_dense's map; K % k_group == 0,
 *     N % n_group == 0; k_group = K, n_group = N: no grouping).  The piece width K_p of a packed
 *     row is ld (VTD_TRAIN_PACK_F32; VTD_TRAIN_PACK_MODE in VTD_BF16) or ld / 3
 *     (VTD_TRAIN_PACK_MODE in VTD_BF16X3, rows [hi | hi | lo]); K_p % 8 == 0, K_p >= the last
 *     real k' + 1, a 16-B aligned base.
 *   VTD_ADAM_VECTOR [N]: element n goes to fp32 element row_offset + (n / n_group) * n_group_p
 *     + n % n_group of `packed` (vtd_pack_vector's map; any non-NONE packed_dtype means fp32).
 *   packed_dtype: VTD_TRAIN_PACK_NONE (packed must be null), VTD_TRAIN_PACK_MODE (the plan's
 *     dtype: bf16 or split-bf16) or VTD_TRAIN_PACK_F32 (fp32 [N_p][K_p], the staging form
 *     vtd_fold_layernorm reads).
 *   constrain: 0 exempts the tensor from ClipWeight whatever the step asks for (the reference
 *     leaves the position embedding unconstrained).
 *   rule: VTD_TRAIN_RULE_DENSE is TF's ApplyAdam functor order (at the step entries below);
 *     VTD_TRAIN_RULE_SPARSE is the order of Keras's sparse Adam path, which an Embedding's
 *     gradient takes (every index once: a dense update):
 *       m = m * beta1 + g * (1 - beta1);   v = v * beta2 + (g * g) * (1 - beta2)
 *       w = w - (alpha * m) / (sqrt(v) + epsilon)            same alpha, g clipped first
 * Padding rule: for every real n the step writes the whole piece(s) [0, K_p) of its packed row,
 * zeros at every k' that is no image of a real k (ungrouped: zeros in [K, K_p)); packed rows that
 * are no image of a real n (the pad rows inside a group, rows >= N, the rows of other tensors
 * sharing the buffer), vector elements that are no image of an n < N and everything outside the
 * buffers stay untouched. */
enum { VTD_TRAIN_PACK_NONE = 0, VTD_TRAIN_PACK_MODE = 1, VTD_TRAIN_PACK_F32 = 2 };
enum { VTD_TRAIN_RULE_DENSE = 0, VTD_TRAIN_RULE_SPARSE = 1 };
typedef struct vtd_train_tensor {
  float* w; float* m; float* v; const float* g;
  void* packed;
  int kind, K, N, ld;
  int k_group, k_group_p, n_group, n_group_p, row_offset;
  int packed_dtype, constrain, rule;
} vtd_train_tensor;
/* The plan: the table in its device form plus a tile -> tensor map, built and uploaded ONCE
 * per optimizer state into caller-owned device memory (plan_dev, 16-B aligned, plan_bytes >=
 * what the plan_bytes entry returns; *tiles is the grid the step launches).  `tensors` is a host
 * array.  The plan_upload entry copies on `stream` and waits for the copy (the only
 * synchronising entry of the three).  `dtype`: the packed operands' mode.
 * VTD_ERR_INVALID_ARG before any device call: null pointers (the table, w / m / v / g, the
 * outputs, plan_dev), non-positive sizes, misaligned bases, a bad kind / packed_dtype / rule,
 * packed_dtype NONE with a destination or a destination without one, VTD_TRAIN_PACK_MODE (any
 * vtd_adam_tensor destination) with a dtype other than VTD_BF16 / VTD_BF16X3, non-positive
 * groups, k_group_p < k_group, n_group_p < n_group, K % k_group != 0, N % n_group != 0, a negative
 * row_offset, ld % 3 != 0 in VTD_BF16X3, ld too small (K_p < the last real k' + 1; ungrouped:
 * K_p < K), K_p % 8 != 0; plan_bytes too small. */
int vtd_train_plan_bytes(const vtd_train_tensor* tensors, int n_tensors, int dtype, size_t* bytes,
                         int* tiles);
int vtd_train_plan_upload(const vtd_train_tensor* tensors, int n_tensors, int dtype,
                          void* plan_dev, size_t plan_bytes, void* stream);
int vtd_adam_plan_bytes(const vtd_adam_tensor* tensors, int n_tensors, int dtype, size_t* bytes,
                        int* tiles);
int vtd_adam_plan_upload(const vtd_adam_tensor* tensors, int n_tensors, int dtype,
                         void* plan_dev, size_t plan_bytes, void* stream);
/* Step t (1, 2, ...) of every tensor of the plan in ONE launch, per element in fp32 and in this
 * order (VTD_TRAIN_RULE_DENSE; every operation rounded once, no FMA contraction):
 *   g  = clipvalue > 0 ? clip(g, -clipvalue, +clipvalue) : g        (a NaN passes through)
 *   m += (g - m) * (1 - beta1);   v += (g * g - v) * (1 - beta2)
 *   w -= (m * alpha) / (sqrt(v) + epsilon)
 *   w  = constrain ? clip(isnan(w) ? 1.0 : w, -max_weight, +max_weight) : w     (ClipWeight;
 *        `constrain` and the tensor's own flag)
 * alpha = learning_rate sqrt(1 - beta2^t) / (1 - beta1^t) is formed on the host in double (from
 * the fp32 betas) and rounded to fp32 once; 1 - beta in fp32.  The packed destinations receive
 * the new w through the conversions of vtd_pack_dense / vtd_split_bf16x3 (role 1): the same
 * bytes as those calls on the updated master.  n_tensors and tiles: as given to / returned by
 * the plan entries.  Asynchronous on `stream`; no copy, no allocation, no host synchronisation;
 * every element owned by one thread, no atomics, bit-identical from run to run.
 * VTD_ERR_INVALID_ARG before any device call: a null plan, non-positive n_tensors / tiles,
 * t < 1, constrain with max_weight <= 0. */
int vtd_train_step(const void* plan_dev, int n_tensors, int tiles, int64_t t,
                   double learning_rate, float beta1, float beta2, float epsilon, float clipvalue,
                   int constrain, float max_weight, void* stream);
int vtd_adam_step(const void* plan_dev, int n_tensors, int tiles, int64_t t,
                  double learning_rate, float beta1, float beta2, float epsilon, float clipvalue,
                  int constrain, float max_weight, void* stream);

/* The LayerNorm fold of several layers in ONE launch: job j is vtd_fold_layernorm(w32, N, K,
 * ldw, gamma, beta, bias_in, w_out, ldo, dtype, bias_out, colsum) with the same per-row
 * arithmetic, so the same bits.  vtd_fold_plan_upload checks the host table and copies it to
 * plan_dev (caller-owned, 16-B aligned, plan_bytes >= n_jobs * sizeof(vtd_fold_job)), waits for
 * the copy and returns the largest N in *max_rows; vtd_fold_layernorm_batch launches
 * (max_rows / 4 rounded up) x n_jobs workgroups on `stream` with no copy, allocation or host
 * synchronisation.  VTD_ERR_INVALID_ARG before any device call: null pointers (bias_in may be
 * null), non-positive sizes, ldw < K, ldo < K, a dtype other than VTD_F32 / VTD_BF16, a
 * misaligned or too small plan. */
typedef struct vtd_fold_job {
  const float* w32; const float* gamma; const float* beta; const float* bias_in;
  void* w_out; float* bias_out; float* colsum;
  int N, K, ldw, ldo;
} vtd_fold_job;
int vtd_fold_plan_upload(const vtd_fold_job* jobs, int n_jobs, int dtype, void* plan_dev,
                         size_t plan_bytes, int* max_rows, void* stream);
int vtd_fold_layernorm_batch(const void* plan_dev, int n_jobs, int max_rows, int dtype,
                             void* stream);

/* Numerical health (csrc/vtd_health.hip; DESIGN.md "Numerical health"): one record per tensor of
 * a table of fp32 device tensors, in ONE pass over their elements -- what the reference's
 * check_inf_nan / check_weights / CheckModelWeight (vtd.py:46-116, 731-758, 650-687) ask of a
 * tensor, plus the sum of squares a gradient norm needs.
 *
 * A record (vtd_tensor_stat, 48 B) of a tensor x of n elements:
 *   n                       the element count, as given
 *   nan, pos_inf, neg_inf   how many elements are NaN / +inf / -inf
 *   max, min                over the elements that are not NaN, infinities included, by
 *                           comparison (x > max, x < min; never fmax / fmin); with no such element
 *                           max = -inf and min = +inf.  +0 and -0 compare equal: the sign of a
 *                           zero result is unspecified.  Subnormals are kept, not flushed.
 *   sumsq                   the sum of (double)x * (double)x over the FINITE elements: each value
 *                           converted to fp64 before the multiply, so every square is exact and
 *                           fused or unfused multiply-add give the same bits; every partial sum
 *                           is fp64.  All terms are >= 0 and exact, so whatever the order the
 *                           result is within n * 2^-53 relative of the exact sum.
 * out: NULL, or n floats that receive out[i] = x[i] != x[i] ? replace_nan : x[i] in the same pass
 * (every non-NaN element, infinities included, keeps its bits); out may alias x.  With out NULL
 * nothing but the records and the workspace is written.
 *
 * Structure: no atomics, the same bits on every run.  A workgroup (256 threads) takes one chunk
 * of VTD_STATS_CHUNK elements of one tensor, counted from that tensor's element 0, through the
 * plan's chunk -> (tensor, chunk index) map; each thread sums its elements in index order, the
 * workgroup reduces in a fixed tree and writes one 32-B partial record to `workspace`; a second
 * kernel on the same stream folds each tensor's partials -- lane l of one wave takes chunks l,
 * l + 64, ... in that order, then the same fixed tree -- into stats_dev[t].  Chunking restarts per
 * tensor, so a tensor's record depends on its elements, n and the alignment of its bases (which
 * picks the vector width: 16-B loads when x, out and 4 n are multiples of 16, else 8 B likewise,
 * else 4 B) and not on what else is in the table or where it sits.
 *
 * vtd_stats_plan_bytes: the bytes of the device plan, the bytes of the workspace (32 per chunk)
 * and the chunk count, sum over the tensors of ceil(n / VTD_STATS_CHUNK).  vtd_stats_plan_upload
 * builds the plan and copies it to plan_dev (caller-owned, 16-B aligned) on `stream`, waiting for
 * the copy -- the only synchronising entry.  vtd_tensor_stats: two launches on `stream`, no copy,
 * no allocation, no host synchronisation; stats_dev: n_tensors records in device memory.
 * VTD_ERR_INVALID_ARG before any device call: a null table or null outputs, n_tensors <= 0, a
 * null x, n <= 0, x or out not 4-B aligned, more chunks than an int holds; plan_bytes too small, a
 * null or not 16-B aligned plan_dev; chunks <= 0, a null or not 8-B aligned workspace / stats_dev,
 * workspace_bytes too small. */
#define VTD_STATS_CHUNK 16384
typedef struct vtd_stats_tensor {
  const float* x;
  float* out;                /* NULL, or n floats; may alias x */
  int64_t n;
} vtd_stats_tensor;
typedef struct vtd_tensor_stat {
  float max, min;
  int64_t n, nan, pos_inf, neg_inf;
  double sumsq;
} vtd_tensor_stat;
int vtd_stats_plan_bytes(const vtd_stats_tensor* tensors, int n_tensors, size_t* plan_bytes,
                         size_t* workspace_bytes, int* chunks);
int vtd_stats_plan_upload(const vtd_stats_tensor* tensors, int n_tensors, void* plan_dev,
                          size_t plan_bytes, void* stream);
int vtd_tensor_stats(const void* plan_dev, int n_tensors, int chunks, void* workspace,
                     size_t workspace_bytes, vtd_tensor_stat* stats_dev, float replace_nan,
                     void* stream);

/* Optional per-kernel timing of vtd_forward (hipEvents on `stream`, recorded around
 * every launch while enabled).  vtd_profile_read returns per-class totals in ms
 * summed over the forwards since the last reset; classes: 0 gemm, 1 attention,
 * 2 layernorm, 3 patches, 4 other. Also returns per-class launch counts and FLOPs. */
#define VTD_PROF_CLASSES 5
int vtd_profile_enable(int enable);
int vtd_profile_reset(void);
int vtd_profile_read(double* ms, int64_t* launches, double* flops, int n_classes);

/* Run-time switches (kernel-variant A/B knobs).  Each is read ONCE per process from its
 * environment variable at the first use of any knob; vtd_set_knob overrides one for the
 * rest of the process (returns the previous value) so tests compare variants in one
 * process.  -1 = unset: the library's default.
 *   VTD_KNOB_ATTN_VARIANT (VTD_ATTN_VARIANT): bf16 attention kernel, 4 = persistent short-
 *     sequence kernel where it applies (default), 2 = streaming, 3 = streaming 8-wave,
 *     1 = the register-staged first kernel.
 *   VTD_KNOB_ATTN_GRID (VTD_ATTN_GRID): persistent attention workgroups (default: CUs).
 *   VTD_KNOB_GEMM_NGW (VTD_GEMM_NGW): GEMM tile-order group width (0 = row-major).
 *   VTD_KNOB_SPLITK (VTD_SPLITK): 0 disables split-K (the head's and, at small batches, the
 *     encoder's), a value >= 64 sets the head's workgroup target per launch (default 256);
 *     both change the workspace size.
 *   VTD_KNOB_JPEG_CHUNK_BITS (VTD_JPEG_CHUNK_BITS): Huffman chunk length of vtd_jpeg_decode.
 *   VTD_KNOB_SKINNY (VTD_SKINNY): 0 keeps the head's narrow bf16 layers (N <= 320) on the
 *     128 x 128 kernel instead of the skinny one; a value >= 64 sets the N threshold (such
 *     layers are then not split-K).
 *   VTD_KNOB_F32_PP2 (VTD_F32_PP2): 0 keeps large fp32-mode GEMMs on the 128 x 128 kernel
 *     instead of the 256-tile f32 one.
 *   VTD_KNOB_STAGGER (VTD_STAGGER): the two-stream split's second micro-batch starts k stages
 *     (patch embedding, encoder layers) behind the first (default: 1 for parts of at most 32
 *     row tiles of 256 -- C2 at B = 64 -- else 0, in phase).
 *   VTD_KNOB_GEMM_TR (VTD_GEMM_TR): 256-tile bf16 GEMM accumulator layout, 1 = transposed
 *     (register-direct epilogue) for every layer, 0 = for none (default: activation layers).
 *   VTD_KNOB_FIN_WGS (VTD_FIN_WGS): LayerNorm-statistics finalize as n grid-stride
 *     workgroups of 1024 threads (default: one 256-thread workgroup per 256 rows).
 *   VTD_KNOB_GEMM_TPW (VTD_GEMM_TPW): consecutive 256 x 256 output tiles per bf16 GEMM
 *     workgroup (default 1); with more, the next tile's first K-stage loads during the
 *     current tile's epilogue. */
enum {
  VTD_KNOB_ATTN_VARIANT = 0,
  VTD_KNOB_ATTN_GRID = 1,
  VTD_KNOB_GEMM_NGW = 2,
  VTD_KNOB_SPLITK = 3,
  VTD_KNOB_JPEG_CHUNK_BITS = 4,
  VTD_KNOB_SKINNY = 5,
  VTD_KNOB_F32_PP2 = 6,
  VTD_KNOB_STAGGER = 7,
  VTD_KNOB_GEMM_TR = 8,
  VTD_KNOB_FIN_WGS = 9,
  VTD_KNOB_GEMM_TPW = 10,
  VTD_KNOB_COUNT = 11
};
int vtd_set_knob(int knob, int value);
int vtd_get_knob(int knob);

#ifdef __cplusplus
}
#endif
#endif /* VTD_H_ */
