/* dgq_hip.h — C ABI of libdgq_hip.so: the MI355X (gfx950) kernels behind DGQ's quantized-UNet path.
 *
 * The reference (ugonfor/DGQ) has NO FFI: its per-layer operator boundary is the Python method
 * QuantLayer.forward (quant/quant_layer.py:626-661) and the attention-side quantizer calls in
 * Attention.Attention_forward (diffusers_rewrite/sd.py:151-207).  Each entry point below names the
 * reference code it replaces.  Conventions:
 *   - plain C types only: raw DEVICE pointers, ints, floats and a hipStream_t passed as void*;
 *   - the caller owns every buffer; the library never allocates, frees or keeps device pointers;
 *   - every launch is asynchronous on `stream`; no host synchronisation, safe under hipGraph capture;
 *   - return 0 on success, a negative DGQ_E* otherwise (message via dgq_last_error()); no exceptions,
 *     no abort().
 * dtype codes for floating tensors: 0 = f32, 1 = f16, 2 = bf16.
 */
#ifndef DGQ_HIP_H
#define DGQ_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGQ_OK 0
#define DGQ_EINVAL (-1)   /* bad shape / alignment / argument */
#define DGQ_EUNSUPPORTED (-2)
#define DGQ_ELAUNCH (-3)  /* HIP reported a launch error */

#define DGQ_F32 0
#define DGQ_F16 1
#define DGQ_BF16 2

#define DGQ_KCHUNK 32     /* K granularity of one MFMA_I32_32x32x32_I8 slice = DGQ group padding */
#define DGQ_KTILE 128     /* Kp (padded, permuted K) must be a multiple of this */

/* ABI revision, major·100 + minor.  A host binding must refuse a library whose revision differs from the header it was written
 * against (dgq_amd/_lib.py does): the argument structs are passed by pointer and have grown between revisions.
 *   100  rounds 1-4
 *   110  round 5: dgq_gemm_extra_t += wfrag, act; dgq_quant_act_args_t += ups; W4 per-K clear marks (cflush == 2) at least every
 *        2176 codes (the kernels read float(T) off a biased int32 total: |T| < 2^22), plan.seg_limit
 *   120  round 6: dgq_attention_sync_timeouts; the attention workspace's δ area is 512 bytes; dgq_gemm_act_t += kpat, B, H, W, kh, kw,
 *        stride, pad; dgq_gemm_conv_act_fuses
 *   121  round 6: dgq_cfg_ddim_step takes the tensors' dtype (void pointers + `dtype`); dgq_attention_workspace_bytes grew by one fp32
 *        part area (key-split launches on 16-bit tensors)
 *   122  round 6: dgq_gemm_extra_t += y2, ldy2; dgq_conv2d_f32w takes y2 / ldy2 / gn_partial
 *   123  dgq_conv2d_wq (the weight-only state from the packed W4 / W8 codes); later, without a new revision because no existing
 *        entry or struct changed (a binding written against 123 keeps working): the real-time per-row activation quantiser tables,
 *        dgq_act_row_params / dgq_act_row_params_batch with their dgq_act_rowparams_out_t; the real-time block mode,
 *        dgq_quant_act_block / dgq_dequant_act_block / dgq_gemm_blockq with dgq_act_block_out_t and dgq_gemm_block_t; dgq_conv2d_wq_mfma16 (the weight-only
 *        state on the 16-bit matrix cores); dgq_attention_mfma16 (un-quantised attention of the 16-bit states on the same cores);
 *        dgq_attention_mfma16_f32 (the same for fp32 tensors, every operand a two-term bf16 split); the real-time MXFP6 mode,
 *        dgq_quant_act_mx6 / dgq_dequant_act_mx6 / dgq_pack_w_mx6 / dgq_gemm_mx6 with dgq_act_mx6_out_t and dgq_gemm_mx6_t;
 *        dgq_conv2d_wq_mfma16_fused with its dgq_wq16_fuse_t — norms, SiLU, GEGLU and the residual folded into the weight-only
 *        matrix-core layer — and dgq_layernorm_row_stats */
#define DGQ_ABI_VERSION 123
int dgq_version(void);
const char* dgq_last_error(void);

/* ---- weights (load time) -------------------------------------------------------------------------
 * dgq_quantize_weight: integer codes of wqtizer(self.w) — UniformAffineQuantizer.forward
 * (quant_layer.py:295-299: clamp(rne(w/δ)+z, 0, 2^b−1)) or, when alpha != NULL, AdaRoundQuantizer hard
 * mode (adaptive_rounding.py:51,58-70: clamp(floor(w/δ)+(α≥0)+z, 0, 2^b−1)).  The reference recomputes
 * these on EVERY forward (quant_layer.py:642-643); here they are computed once.
 * w [N][K] f32, delta/zp [N] f32, alpha [N][K] f32 or NULL, codes [N][K] u8. */
int dgq_quantize_weight(const float* w, const float* delta, const float* zp, const float* alpha,
                        int N, int K, int bits, uint8_t* codes, void* stream);

/* dgq_pack_w4: codes u8 [N][K] (values 0..15) -> packed [N][Kp/2] bytes.  kperm [Kp] gives for each
 * packed position the source k (or -1 = zero padding); NULL = identity (Kp == K).  Layout per 8
 * consecutive kp: one 32-bit word, byte j holds kp+j in its low nibble and kp+4+j in its high nibble,
 * so that (word & 0x0F0F0F0F) and ((word >> 4) & 0x0F0F0F0F) are 4 consecutive int8 each.
 * layout 2 (dgq_gemm_extra_t.wfrag): fragment-major for V_MFMA_I32_32X32X32_I8 B operands — N padded to 32-column tiles (zero
 * rows), [ceil(N/32)][Kp/64] blocks of 1 KiB; in block (j, p) lane l = (k half h << 5) | (n & 31) owns the 16 bytes at l·16: the two
 * words of K half h of chunk 2p, then those of chunk 2p + 1, column n = 32j + (l & 31).  `packed` holds ceil(N/32)·32·Kp/2 bytes.
 * layout 0: rows as described.  layout 1 (what dgq_gemm_wxa8 and dgq_linear_smallm_batch read): in rows n with (n & 16) != 0 the two
 * 8-byte halves of every 16 packed bytes (= one 32-wide chunk) are exchanged — the GEMM stages 16-byte pieces into LDS by
 * DMA and a lane reads the 8 bytes of its K half; with the exchange the 32 lanes of a read cover all 64 LDS banks. */
int dgq_pack_w4(const uint8_t* codes, int N, int K, const int32_t* kperm, int Kp, int layout, uint8_t* packed, void* stream);
/* exact inverse (test hook for the "bit-exact int4 unpack" requirement): out [N][Kp] u8 */
int dgq_unpack_w4(const uint8_t* packed, int N, int Kp, int layout, uint8_t* out, void* stream);
/* W8: out[n][kp] = (int8)(codes[n][kperm[kp]] - 128), 0 for padding */
int dgq_pack_w8(const uint8_t* codes, int N, int K, const int32_t* kperm, int Kp, int8_t* packed, void* stream);

/* ---- activations: quantise-on-load pre-pass ------------------------------------------------------
 * Replaces `x = self.aqtizer(x)` (quant_layer.py:640-641 -> :295-299) and, for grouped convs, the
 * F.unfold that precedes it (quant_layer.py:630-638): writes int8 codes s = q − offset of the (implicit)
 * unfolded operand, row-major [M][Kp], in the permuted/padded K order of the packed weight, plus one
 * float per row.
 *
 * x is a channels-last tensor [B][H][W][C] (a Linear input [B,T,K] is B=B·T... H=W=1, C=K); geometry
 * (kh,kw,stride,pad) as the conv; M = B·Ho·Wo.  Source of packed position kp:
 *   ksrc == NULL : natural order kp = tap·C + c   (tap = dh·kw + dw)
 *   ksrc != NULL : ksrc[kp] = (dh << 24) | (dw << 16) | c, or -1 for padding (zero code); koff (optional, NULL = derive
 *                  from ksrc) = the same table resolved for this geometry, (dh·W + dw)·ldc + c or -1, read by rows whose
 *                  taps all lie inside the image (no bounds checks); klds (optional) = (dh·kw + dw)·C + c or -1: the
 *                  index into the [tap][C] strip a wave stages in LDS (kh·kw > 1 and kh·kw·C·4 <= 64 KB).
 * Quantiser parameters:
 *   per_m == 0 : cdelta/czp [Kp/32] — one (δ,z) per 32-wide chunk (DGQ groups are chunk aligned);
 *                rowsum[m] = Σ_kp δ(kp)·s[m,kp]
 *   per_m == 1 : mdelta/mzp [L] indexed by (m % L) (L=1: scalar quantiser);
 *                rowsum[m] = Σ_kp s[m,kp]  (exact integer in f32)
 * bits: activation bits b; code offset = 2^(b-1) (s = q − 2^(b−1) is a centred int8).  Out-of-image taps read 0.0 and are
 * quantised like any value (F.unfold pads before the quantizer).
 * pre_scale/pre_shift [B][C] (or NULL): the element is first mapped to x·scale + shift (a GroupNorm folded into
 * the load, see dgq_groupnorm_scale_shift); pre_act == 1 then applies SiLU (resnet norm→SiLU→conv, and SiLU(temb) →
 * time_emb_proj); pre_act == 2 reads rows of 2C elements and forms x[c]·gelu(x[C+c]) (GEGLU in front of ff.net.2,
 * sd.py:210-236); out-of-image taps stay 0.
 * ln_gamma/ln_beta [C] (or NULL) + ln_eps: nn.LayerNorm over the C elements of each row folded into the load
 * (norm1/2/3 of BasicTransformerBlock in front of to_q/to_k/to_v/ff.net.0.proj, sd.py:245-268): the wave that
 * quantises a row computes its mean / biased variance and maps x to (x − μ)·rstd·γ + β.  1x1 only, no other prologue.
 * ksplits >= 1 splits every row's K range over that many waves (low-M layers); rowsum then has
 * dgq_quant_act_parts(Kp, ksplits) x M entries ([part][m]) which dgq_gemm_wxa8 adds in a fixed order. */
int dgq_quant_act(const void* x, int x_dtype, int B, int H, int W, int C,
                  int kh, int kw, int stride, int pad,
                  const int32_t* ksrc, const int32_t* koff, const int32_t* klds, int Kp,
                  int per_m, const float* delta, const float* zp, int L,
                  int bits, int8_t* codes, float* rowsum, int ksplits,
                  const float* pre_scale, const float* pre_shift, int pre_act,
                  const float* ln_gamma, const float* ln_beta, float ln_eps, void* stream);
int dgq_quant_act_parts(int Kp, int ksplits);
/* The same with the arguments in a struct, for 1..8 problems in ONE launch (dgq_quant_act_batch): the q / k / v
 * projections of an attention quantise one input with three tables, the to_k / to_v of every cross-attention quantise
 * the one text context.  All problems of a batch must have the same row count M, dtype, scale mode (per_m) and kernel
 * variant (dgq_quant_act_variant: 0 LDS-staged, 1 table gather, 2 natural order, 3 / 4 LDS scatter, 5 block-staged conv) —
 * DGQ_EINVAL otherwise. */
typedef struct dgq_quant_act_args {
    const void* x; int x_dtype; int B, H, W, C, kh, kw, stride, pad;
    const int32_t* ksrc; const int32_t* koff; const int32_t* klds;
    const int32_t* kdst;      /* optional [kh·kw·C]: packed position kp of element (tap, c) — the inverse of ksrc; enables the
                                 coalesced-read / LDS-scatter path for per-K conv layers (ksplits must be 1) */
    int Kp;
    int per_m; const float* delta; const float* zp; int L; int bits;
    int8_t* codes; float* rowsum; int ksplits;
    const float* pre_scale; const float* pre_shift; int pre_act;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    const int32_t* kpat;      /* optional [Kp] (convolutions): (dh·PW + dw)·C + c of packed position kp inside the input patch of
                                 a tile, PW from dgq_quant_act_conv_tile; -1 = padding.  Natural order (ksrc == NULL) too.
                                 Enables the block-staged conv path (variant 5): a workgroup stages the input patch of a tile
                                 of output positions once in LDS with the GroupNorm / SiLU prologue applied once per element
                                 (the per-row paths apply it once per tap), then gathers every row's codes from it. */
    int ups;                  /* 0, or 1: x holds (H/2) x (W/2) pixels per image and input pixel (hi, wi) reads (hi/2, wi/2) — the
                                 F.interpolate(x, scale_factor=2, mode="nearest") in front of Upsample2D's conv (diffusers_rewrite/sd.py
                                 Upsample2D.forward) folded into the load.  H, W are the UPSAMPLED dims; convolutions on the scatter /
                                 block-staged paths only (dgq_quant_act_variant 3 / 4 / 5, asked with ups set), DGQ_EINVAL otherwise. */
} dgq_quant_act_args_t;
int dgq_quant_act_batch(int n, const dgq_quant_act_args_t* args, void* stream);
int dgq_quant_act_variant(const dgq_quant_act_args_t* args);
/* tile id (1: 4x8, 2: 4x4, 3: 2x4 output positions; 0: the patch does not fit, no block-staged path) and patch width PW
 * = (TW − 1)·stride + kw of the block-staged conv path for a geometry: what the caller needs to build `kpat` */
int dgq_quant_act_conv_tile(int C, int kh, int kw, int stride, int Kp, int* patch_w);

/* ---- activations: real-time per-row quantiser tables (a mode of this library; the reference has no such layer quantiser) ----------
 * One (δ, z) per row the activation quantiser sees, from Scaler.MINMAX applied to that row at run time: lo = min(row min, 0),
 * hi = max(row max, 0), δ = fp32((double(hi) − double(lo)) / (2^bits − 1)), fp32(1e-8) when smaller, z = rne(fp32(−lo) / δ) (IEEE
 * division) — bit for bit.  The row of a Linear layer is a row of its [M][C] input; the row of a convolution is one output
 * position's row of the unfolded operand (C·kh·kw values, zeros outside the image — MINMAX includes 0 anyway).  Both AFTER the
 * folded prologue, evaluated by the device functions of dgq_quant_act, so that the quantiser sees the same x′.
 * `in` describes the input exactly as for dgq_quant_act: x, x_dtype, B, H, W, C, kh, kw, stride, pad, bits, pre_scale / pre_shift /
 * pre_act, ln_gamma / ln_beta / ln_eps, ups are read (x 16-byte aligned, C % 4 == 0); its tables, Kp and outputs are ignored.
 * delta_out / zp_out [M]: what the per-M routes take as mdelta / mzp with L = M (dgq_quant_act, dgq_gemm_wxa8 with or without
 * quantise-on-load).
 * fold_T > 0 (Linear inputs, fold_T | M): rows with equal r % fold_T share one pair — delta_out / zp_out [fold_T], the (1, T, 1) layout
 * of the attention-side quantisers (dgq_attn_fq_t mode 1, dgq_fakequant_rows mode 1).
 * ws: caller-owned scratch of 2 floats per input pixel (B·H·W, a quarter with ups), 8-byte aligned — needed by convolutions (anything
 * but 1x1 / stride 1 / pad 0) and by fold_T > 0; one launch otherwise, two with it.  No allocation, no synchronisation, no atomics:
 * capture-safe.  The batch form takes 1..4 problems of one dtype that are all of the two-launch kind or all of the one-launch kind
 * (the q / k / v outputs of an attention, any row counts) and shares the launches. */
typedef struct dgq_act_rowparams_out {
    int fold_T; float* ws; size_t ws_floats; float* delta; float* zp;
} dgq_act_rowparams_out_t;
int dgq_act_row_params(const dgq_quant_act_args_t* in, int fold_T, float* ws, size_t ws_floats, float* delta_out, float* zp_out, void* stream);
int dgq_act_row_params_batch(int n, const dgq_quant_act_args_t* in, const dgq_act_rowparams_out_t* out, void* stream);

/* ---- activations: real-time quantiser per row and 32-channel block (a mode of this library) -----------------------------------------
 * One (δ, z) per input row AND block of DGQ_KCHUNK = 32 consecutive channels, from Scaler.MINMAX applied to the block at run time
 * (the arithmetic of dgq_act_row_params on the block's extrema, bit for bit; an all-zero block gives δ = fp32(1e-8), z = 0).  In the
 * natural (tap, c) K order a 32-chunk of a convolution's unfolded row is 32 channels of one input pixel, so the INPUT is quantised,
 * once per row / pixel, and dgq_gemm_blockq gathers the taps: `in` is read as by dgq_act_row_params (x, x_dtype, B, H, W, C, bits,
 * the folded prologue, ups; C % 32 == 0, x 16-byte aligned) but kh, kw, stride, pad only tell a Linear input (1x1: GEGLU /
 * LayerNorm prologues allowed) from a convolution's.  rows = B·H·W input pixels (a quarter with ups: the source pixels).  ONE launch:
 *   codes [rows][C] int8, 16-byte aligned: centred codes s = q − 2^(bits−1) in natural channel order;
 *   table [rows][ldt] pairs of floats {δ, β = δ·(2^(bits−1) − z)}, ldt >= C/32; entries C/32 .. ldt − 1 are written {0, 0} (the chunks
 *         of a Linear layer's K padding: pass ldt = Kp/32);
 *   rho   [rows]: Σ_c δ_c·rs_c, rs_c = Σ_{k∈c} s, one fp32 addition per block in ascending block order (deterministic).
 * dgq_dequant_act_block: y [rows][C] (y_dtype) = δ·(q − z) from such codes and table — the quantizer's stand-alone fake-quant form. */
typedef struct dgq_act_block_out {
    int8_t* codes; float* table; int ldt; float* rho;
} dgq_act_block_out_t;
int dgq_quant_act_block(const dgq_quant_act_args_t* in, const dgq_act_block_out_t* out, void* stream);
int dgq_dequant_act_block(const int8_t* codes, const float* table, int ldt, int64_t rows, int C, void* y, int y_dtype, void* stream);

/* GroupNorm of a channels-last tensor x [B][HW][C] as per-(b,c) scale/shift (biased variance, eps as F.group_norm):
 * GN(x) = x·scale + shift.  Replaces norm1/norm2 of QuantResnetBlock2D.forward (quant_block.py:98-119) together with
 * the SiLU that follows, which dgq_quant_act applies while loading.  partial_ws: B·G·slices·3 floats;
 * slices > 1: a second small kernel merges the slices in slice order. */
int dgq_groupnorm_scale_shift(const void* x, int x_dtype, int B, int HW, int C, int G, float eps,
                              const float* gamma, const float* beta, float* scale, float* shift,
                              float* partial_ws, int slices, void* stream);
/* The same scale / shift from the partial statistics a producing dgq_gemm_wxa8 left behind (dgq_gemm_extra_t.gn_partial):
 * partial [B·HW/16][C][2] = (mean, Σ(x − mean)²) per 16-row block and channel; HW % 16 == 0.  One small launch, no pass
 * over the tensor; the blocks and channels of a (batch, group) are merged in a fixed order (Chan), biased variance.
 * partial2 / C2 (optional, NULL / 0): a second source whose channels FOLLOW the first's — the statistics of
 * torch.cat([a, b], dim=1) from those of a and b (the skip concatenations in front of the up blocks' norm1). */
int dgq_groupnorm_from_partials(const float* partial, int C1, const float* partial2, int C2, int B, int HW, int G, float eps,
                                const float* gamma, const float* beta, float* scale, float* shift, void* stream);

/* ---- elementwise glue of a denoise step as single launches ------------------------------------------------------------------
 * Timesteps.forward (diffusers_rewrite/sd.py:19-39: flip_sin_to_cos, no frequency shift): out [rows][dim] =
 * cat(cos(t·f), sin(t·f)), f_j = exp(−ln(10000)·j / (dim/2)).  t: rows values of int64 (t_is_float = 0) or fp32 (1), element
 * stride t_stride (0 = the one timestep expanded over the batch, sd.py:550).  Same operation order as the torch chain. */
int dgq_timestep_embedding(const void* t, int t_is_float, int64_t t_stride, int rows, int dim, void* out, int out_dtype, void* stream);
/* Classifier-free guidance + DDIM update (eta = 0) of the pipeline loop (pipeline_stable_diffusion.py:1037-1044,
 * schedulers/scheduling_ddim.py step): eps = e_u + guidance·(e_c − e_u) (eps_cond == NULL: eps = e_u),
 * out = s3·((sample − s1·eps)·inv_s2) + s4·eps with s1 = sqrt(1−a_t), inv_s2 = 1/sqrt(a_t), s3 = sqrt(a_prev), s4 = sqrt(1−a_prev); the four
 * tensors of one dtype (DGQ_F32 / F16 / BF16: a 16-bit chain rounds after every statement, as the eager one does),
 * n elements per tensor = whole [C][HW] images; sample / out contiguous [n/(C·HW)][C][HW]; the eps halves in the same layout
 * (eps_channels_last = 0) or as [.][HW][C] (1: the UNet's channels-last output); evaluated in the order of the eager torch chain. */
int dgq_cfg_ddim_step(const void* eps_uncond, const void* eps_cond, const void* sample, void* out, int dtype, int64_t n, int C, int HW,
                      int eps_channels_last, float guidance, float s1, float inv_s2, float s3, float s4, void* stream);

/* ---- weight-only state (use_wq without use_aq: quant_layer.py:642-659 with unquantised activations) -----------------
 * y[m][n] = Σ_k x_unfolded[m][k]·w[n][k] + bias[n] in exact fp32 (V_MFMA_F32_32X32X2_F32), the im2col of a convolution folded
 * into the operand load: x channels-last [B][H][W][C] (x_dtype), w [N][kh·kw·C] fp32 = the dequantised weight δw·(qw − zw) with
 * K in (tap, c) order, y [B·Ho·Wo][ldy] (y_dtype).  A Linear layer is B = rows, H = W = kh = kw = stride = 1, pad = 0.
 * Optional prologue as in dgq_quant_act: pre_scale / pre_shift [B][C] (a GroupNorm folded into the load: x·scale + shift) and
 * pre_act = 1 (SiLU) — conv_out(SiLU(conv_norm_out(x))) of the UNets in one launch.
 * Replaces F.linear / F.conv2d on the dequantised (or, for the FP conv_in / conv_out, the original) weight. 
 * y2 (or NULL), ldy2: a second copy of the output rows, as dgq_gemm_extra_t.y2; gn_partial (or NULL; M % 16 == 0, N > 8): the
 * output's GroupNorm partials [M/16][N][2], as dgq_gemm_extra_t.gn_partial. */
int dgq_conv2d_f32w(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad,
                    const float* w, const float* bias, int N, void* y, int y_dtype, int ldy,
                    const float* pre_scale, const float* pre_shift, int pre_act, void* y2, int ldy2, float* gn_partial, void* stream);

/* dgq_conv2d_wq: the same layer computed from the packed weight, bit for bit what dgq_conv2d_f32w returns on the dequantised weight
 * (N > 8).  w_packed is the natural-order image of PackedWeight.natural(): K in (tap, c) order padded to Kp (a multiple of
 * DGQ_KTILE, >= kh·kw·C); w_bits 4 = dgq_pack_w4 layout 1, 8 = dgq_pack_w8 (int8 code − 128).  Every element is dequantised once,
 * as it is staged, to ŵ = delta[n]·((float)q − zp[n]); bias [N] or NULL.  upsample = 1: x holds (H/2) x (W/2) pixels per image and
 * input pixel (hi, wi) reads (hi/2, wi/2) (F.interpolate(scale_factor=2, mode="nearest") folded into the load; H, W even);
 * geglu_rows = 1: packed row 2i is stored to column i and row 2i + 1 to column i + N/2 (QuantLayer.geglu_rows back in the
 * reference's column order).  y [B·Ho·Wo][ldy] (y_dtype). */
int dgq_conv2d_wq(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                  const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias, int N,
                  int geglu_rows, void* y, int y_dtype, int ldy, void* stream);

/* dgq_conv2d_wq_mfma16: the same layer, arguments and refusals on the 16-bit matrix cores — NOT bit-identical to dgq_conv2d_wq:
 *   y[m,n] = round_to_y( bias[n] + delta[n]·Σ_k x̃[m,k]·(q[n,k] − zp[n]) ),  k in (tap, c) order, fp32 accumulation, one K loop per
 * workgroup (no K split, no atomics: the order of summation is fixed by the shape).  q − zp[n] is converted once, as it is staged, to
 * the operand type: bf16 for bf16 and fp32 x, f16 for f16 x.  The caller guarantees that it is an integer of magnitude <= 15 (W4) /
 * 255 (W8) — exact in both types (PackedWeight.mfma16_eligible); another value is rounded to the operand type.  bf16 / f16 x: x̃ = x,
 * the products are exact in fp32.  fp32 x: x̃ = hi + lo with hi = bf16_rn(x), lo = bf16_rn(x − hi), |x − x̃| <= 2^-16·|x|; two MFMAs
 * per K step into one accumulator, first lo, then hi. */
int dgq_conv2d_wq_mfma16(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                         const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias, int N,
                         int geglu_rows, void* y, int y_dtype, int ldy, void* stream);

/* dgq_conv2d_wq_mfma16_fused: dgq_conv2d_wq_mfma16 with the layer's element-wise neighbours folded into its load and its epilogue
 * (csrc/gemm_wonly16.hip).  Every pointer of `f` may be NULL; with f NULL or every field empty the call IS dgq_conv2d_wq_mfma16 (the
 * same kernel, the same bits).
 *   x′[m,k] = act(norm(x[m,k])) in fp32, in the order and rounding of the quantisers' folded prologue; 0 exactly for a tap outside the
 *             image and for k >= K (padding comes after the norm and the activation);
 *     norm: pre_scale / pre_shift [B][C] fp32 (GroupNorm folded: x·scale[b][c] + shift[b][c], b the image of the row's pixel, the
 *           tables of dgq_groupnorm_scale_shift; allowed beside upsample),
 *        or ln_stats [M][2] fp32 (mean, rstd) of dgq_layernorm_row_stats with ln_gamma / ln_beta [C] fp32 (LayerNorm folded:
 *           (x − mean)·rstd·γ[c] + β[c]; kh = kw = 1, stride 1, no padding), or none;   pre_act: 0 none, 1 SiLU;
 *   x̃ = x′ rounded once to the operand type (bf16 / f16 x) or its two-term bf16 split (fp32 x);  acc = Σ_k x̃·(q − zp), the same K loop;
 *   t = delta[n]·acc + bias[n] [+ bias_rows[b(m)][n]];   y = round_to_y(t [+ residual[m][n]])  — all in fp32, ONE rounding;
 *   geglu_out = 1 (needs geglu_rows, an even N, no residual): y[m][i] = round_to_y(t[m][2i]·gelu(t[m][2i + 1])), y is [M][ldy >= N/2].
 * residual [M][ldr >= N] and bias_rows [B][N] hold y's dtype and are in the OUTPUT's column order: with geglu_rows = 1 packed row n reads
 * them at the column it stands for (n/2, or n/2 + N/2 for odd n) — under geglu_out too, where bias_rows [B][N] holds the value columns
 * first and the gate columns second.  The prologue's tables must be 16-byte aligned.  Refused: GroupNorm
 * and LayerNorm fields both set, a LayerNorm on a k x k window, ln_stats without gamma and beta, geglu_out with a residual, ldr < N. */
typedef struct {
    const float* pre_scale; const float* pre_shift;
    const float* ln_stats; const float* ln_gamma; const float* ln_beta;
    int pre_act;
    const void* residual; int ldr;
    const void* bias_rows;
    int geglu_out;
} dgq_wq16_fuse_t;
int dgq_conv2d_wq_mfma16_fused(const void* x, int x_dtype, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int upsample,
                               const uint8_t* w_packed, int w_bits, int Kp, const float* delta, const float* zp, const float* bias, int N,
                               int geglu_rows, void* y, int y_dtype, int ldy, const dgq_wq16_fuse_t* f, void* stream);

/* dgq_layernorm_row_stats: out[r] = (mean, rstd = 1/sqrt(var + eps)) of row r of x [rows][C] (biased variance, as nn.LayerNorm): one wave
 * per row, the row read once, mean first, then Σ(x − mean)²; the sums and the final division, square root and reciprocal are carried in
 * fp64 and rounded to fp32 once, so both values are the float64 statistics to within 2^-24 relative (the quantisers' folded LayerNorm
 * evaluates the same two passes in fp32: its statistics agree to a few 2^-24, not bit for bit).  C % 4 == 0 and C <= 2048, x 16-byte
 * aligned; anything else is refused. */
int dgq_layernorm_row_stats(const void* x, int x_dtype, int rows, int C, float eps, float* out, void* stream);

/* ---- the hot kernel: W4A8 / W8A8 MFMA GEMM with fused dequantisation ------------------------------
 * Replaces F.linear / `w.view(N,-1) @ unfolded` / F.conv2d on fake-quantised operands
 * (quant_layer.py:652-659, :562).  Integer identity, s = qx − offset, zw' = zw − woff:
 *   per_m == 0: y[m,n] = alpha[n]·( Σ_chunks cdelta[c]·Σ_{k∈c} s[m,k]·qw'[n,k]  −  zw[n]·rowsum[m] ) + gamma[n]
 *   per_m == 1: y[m,n] = alpha[n]·mdelta[m%L]·( Σ_k s·qw' − zw[n]·rowsum[m] + (offset − mzp[m%L])·vn[n] ) + gamma[n]
 * codes [M][Kp] int8; wpacked: w_bits==4 -> [N][Kp/2] (dgq_pack_w4), w_bits==8 -> [N][Kp] int8;
 * alpha = δw, zw = zero point in the stored code domain (zw − 8·0 for W4: unsigned nibbles; zw − 128 for W8);
 * gamma = bias (+ alpha·U for per_m==0, U[n] = Σ_k δx_k(offset − zx_k)(qw'[n,k] − zw[n]), precomputed per slot);
 * vn[n] = Σ_k qw'[n,k] − K·zw[n].  y [M][ldy] of y_dtype.  cdelta / cflush have Kp/32 entries (one per 32-wide chunk).
 * Every chunk of a DGQ group carries the group's δ in cdelta; the kernel sums by parts, Σ_c (cdelta[c] − cdelta[c+1])·T_c
 * with T_c the running int32 total after chunk c, so a group boundary is wherever cdelta changes.  cflush[c] == 2 on the
 * LAST chunk of a K tile (c % 4 == 3) asks for the running totals to be cleared behind that tile (the coefficient in front
 * of the clear is then the full cdelta): the caller places such marks so that float(T) is exact — W8: |T| <= 2^24 (converted);
 * W4: |T| < 2^22, REQUIRED: the W4 per-K kernels keep T biased by bits(1.5·2^23) and read the float off the bits
 * (dgq_amd/plan.py:seg_limit: every 2176 codes for W4A8, 1024 for W8A8); marks on other chunks are ignored,
 * other values (0 inside a group, 1 at a group end) are informative. */
/* Optional epilogue extras (host struct, passed by pointer; NULL = none), applied in this order to the fp32 result:
 *   fq_mode != 0 : the attention-side quantizer of the projection output, aqtizer_{q,k,v} (sd.py:174-182,199):
 *                  y = δ·(clamp(rne(y/δ)+z, 0, fq_qmax) − z) with (δ,z) = table[0] (mode 1), table[(m % fq_T) − fq_skip]
 *                  (mode 2, per token; tokens < fq_skip bypass: start_peak) or table[n % fq_D] (mode 3, per head-dim);
 *   residual     : y += residual[(m / res_div)·ldr + n]  (x + attn(x), x + ff(x), shortcut + conv2(...) of the Quant
 *                  blocks, quant_block.py:98-119,165-186; res_div = Ho·Wo broadcasts one row per image: conv1(...) +
 *                  time_emb_proj(...)[:, :, None, None]) — dtype res_dtype (DGQ_F32/F16/BF16; ldr in elements), may alias
 *                  nothing written by this call; res_div >= 1;
 *   geglu != 0   : FeedForward's GEGLU (diffusers_rewrite/sd.py:210-222) for a ff.net.0 whose weight rows were
 *                  interleaved at pack time (row 2i = value column i, row 2i+1 = gate column i; alpha / zw / gamma / vn
 *                  likewise): y has N/2 columns, y[m, i] = h[m, 2i]·gelu(h[m, 2i+1]) (erf form).  No other extra, no K
 *                  split, N % 4 == 0;
 *   gn_partial   : (or NULL) [M/16][N][2] floats: per 16-row block and column the mean and the sum of squared deviations of
 *                  the values this call stores (after residual; as rounded to y_dtype) — GroupNorm statistics of the output
 *                  for dgq_groupnorm_from_partials, instead of a pass over the tensor.  M % 16 == 0, N % 4 == 0, 16-byte
 *                  aligned.  Written by the GEMM's own epilogue, or — a K-split launch — by its combine kernel
 *                  (dgq_gemm_plan_splits tells which the shape gets; only the GEGLU epilogue forces an unsplit launch). */
/* Implicit im2col A operand (dgq_gemm_extra_t.conv): a convolution whose activation quantizer is ONE (δ, z) pair — the
 * reference's native path F.conv2d(aqtizer(x), ŵ), quant_layer.py:659 — quantises every input pixel once:
 *   codes_in [B·H·W][ldc] int8 = dgq_quant_act of the NHWC input as a 1x1 layer in natural order (ldc = its Kp >= C),
 *   pixsum   [pixsum_parts][B·H·W] = that call's rowsum (Σ_c s of a pixel, in the K-split parts the pass wrote).
 * dgq_gemm_wxa8 then takes the rows of the unfolded operand straight from codes_in: K order kp = tap·C + c (the natural
 * conv order of dgq_pack_w4's kperm == NULL image of the [N][kh][kw][C] weight), row m = (b·Ho + ho)·Wo + wo, tap (dh, dw)
 * reads pixel (ho·stride − pad + dh, wo·stride − pad + dw); a tap outside the image reads `fill` (16 bytes of the code of
 * the value 0.0, i.e. z − offset: the native F.conv2d of quant_layer.py:659 pads with 0.0 BEHIND the quantizer, which is the code
 * z — the caller offers this operand only while 0 <= z <= 2^b − 1 — followed by 16 zero bytes for the K padding).
 * `codes` / `rowsum` of the call: codes is ignored (pass codes_in), rowsum [M] is an OUTPUT scratch the call fills first
 * (Σ over the taps of pixsum, C·zero_code for a tap outside).  per_m == 1 with L == 1, C % 16 == 0, w_bits == 4. */
typedef struct dgq_gemm_conv {
    const int8_t* codes_in;
    const float* pixsum;
    const int8_t* fill;
    int B, H, W, C, ldc, kh, kw, stride, pad, Ho, Wo;
    float zero_code;
    int pixsum_parts;
} dgq_gemm_conv_t;

/* Quantise-on-load INSIDE the GEMM (dgq_gemm_extra_t.act; Linear / 1x1 layers): instead of reading the int8 codes a dgq_quant_act
 * launch wrote, the short-K kernel quantises the rows of its own workgroup tile straight from the floating-point input into its LDS
 * operand panel — `x = self.aqtizer(x)` (quant_layer.py:640-641) and F.linear (:659) in ONE launch, no code matrix in HBM.  Same
 * quantiser arithmetic as dgq_quant_act (exact-division codes, the same folded prologues); `codes` / `rowsum` of the call are
 * ignored (pass any non-NULL pointers).  The library takes it only where dgq_gemm_act_fuses() says so; otherwise DGQ_EINVAL.
 *   x [M][ldx] of x_dtype (the layer's input rows; K = C source channels, ldx >= K, 16-byte aligned rows);
 *   per_m == 0: kdst [K] = packed position kp of source channel c (the inverse of dgq_quant_act's ksrc), czp [Kp/32] the chunks'
 *               zero points (the scales are the call's cdelta); per_m == 1: natural order, tables mdelta / mzp / L of the call;
 *   bits: activation bits; pre_scale / pre_shift [M / rows_per_image][K] (or NULL) + pre_act (0 / 1 = SiLU): a GroupNorm folded
 *   into the load as in dgq_quant_act; ln_gamma / ln_beta [K] (or NULL) + ln_eps: a LayerNorm over each row folded into the load. */
typedef struct dgq_gemm_act {
    const void* x; int x_dtype; int ldx; int K;
    const int32_t* kdst; const float* czp; int bits;
    const float* pre_scale; const float* pre_shift; int rows_per_image; int pre_act;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    /* round 6 (revision 120): a k x k convolution in this form (csrc/gemm_convq.hip) — kh > 1: x is the NHWC input [B][H][W][ldx] of K = C
     * channels, the call's M = B·Ho·Wo and Kp covers C·kh·kw; kpat [Kp] = for every packed position the index (dh·PW + dw)·C + c into a
     * workgroup's staged (4 + kh − 1) x PW x C input patch, PW = 8 + kw − 1, −1 for padding (ops.ActBinding.kpat_for); per_m == 0: czp as
     * above (kdst unused); pre_scale / pre_shift per image ([B][C]); no LayerNorm.  Zero-initialised (kh == 0): a Linear / 1x1 layer. */
    const int32_t* kpat; int B, H, W, kh, kw, stride, pad;
} dgq_gemm_act_t;

typedef struct dgq_gemm_extra {
    const void* residual;
    int ldr;
    int res_div;
    int res_dtype;
    int fq_mode;
    const float* fq_delta;
    const float* fq_zp;
    int fq_T, fq_D, fq_skip;
    float fq_qmax;
    int geglu;
    float* gn_partial;
    const dgq_gemm_conv_t* conv;     /* (or NULL) implicit im2col A operand, see dgq_gemm_conv_t */
    const float* flush_coef;         /* (or NULL; per_m == 0) [Kp/32 + Kp/128] floats, 16-byte aligned: the summation-by-parts
                                      * coefficients of an unsplit launch, coef_c = cdelta[c] − cdelta[c+1] (the last chunk, and a
                                      * K tile's last chunk under a clear mark cflush == 2: cdelta[c]), then one clear flag per K
                                      * tile.  Derived from cdelta / cflush (the library forms the same table itself when this
                                      * is NULL); given here, the 256-row kernel reads it with scalar loads. */
    const void* wfrag;               /* (or NULL; w_bits == 4) the SAME weights as `wpacked` in dgq_pack_w4 layout 2 (fragment-major,
                                      * [ceil(N/32)·32][Kp/2] bytes, 16-byte aligned): lets the library take its short-K kernel
                                      * (gemm_panel.hip: the activations' whole K slice in LDS, weights streamed straight into MFMA
                                      * B fragments) for the launches it is faster on; results are those of the other kernels. */
    const dgq_gemm_act_t* act;       /* (or NULL) quantise-on-load inside the GEMM, see dgq_gemm_act_t; needs wfrag */
    void* y2;                        /* (or NULL) a SECOND copy of the output rows, y_dtype, row pitch ldy2 >= N elements: the layer's output
                                      * stored as well into its slot of a channel-concatenation buffer (the skip connections of the
                                      * up path, diffusers_rewrite/sd.py:558-613: torch.cat([h, skip], 1) of channels-last tensors is
                                      * [M][C1 + C2] rows) — with `y` / ldy pointing into such a buffer for the other half, no
                                      * concatenation launch is needed.  Not with the GEGLU epilogue. */
    int ldy2;
} dgq_gemm_extra_t;

int dgq_gemm_wxa8(const int8_t* codes, const float* rowsum, int rowsum_parts, int M, int Kp,
                  const void* wpacked, int w_bits, int N,
                  int per_m, const float* cdelta, const uint8_t* cflush,
                  const float* mdelta, const float* mzp, int L, float offset,
                  const float* alpha, const float* zw, const float* gamma, const float* vn,
                  void* y, int y_dtype, int ldy, void* workspace, size_t workspace_bytes,
                  const dgq_gemm_extra_t* extra, void* stream);
/* 1 where dgq_gemm_wxa8 / _batch accept dgq_gemm_extra_t.act for a layer of this shape (n_problems of one launch, all alike): the
 * whole padded K must fit the short-K kernel's LDS panel and the launch must be one it would give that kernel anyway. */
int dgq_gemm_act_fuses(int M, int N, int K, int Kp, int w_bits, int per_m, int n_problems, int x_dtype, int y_dtype);
/* ... and whether a dgq_gemm_wxa8 call with extra.act describing a kh x kw convolution (act.kh > 1) is accepted: 3x3, stride 1, pad 1,
 * W4, N = 160 or 320, H % 4 == 0, W % 8 == 0, the 6 x 10 x C fp32 input patch + a 10-tile operand slab within the LDS (C <= 340). */
int dgq_gemm_conv_act_fuses(int B, int H, int W, int C, int kh, int kw, int stride, int pad, int N, int Kp, int w_bits, int per_m,
                            int x_dtype, int y_dtype);
/* The same with the arguments in a struct, for 1..8 problems in ONE launch (dgq_gemm_wxa8_batch): problems that share
 * weight bits, scale mode (per_m) and output dtype, e.g. the q / k / v projections of one attention or the to_k / to_v of
 * every cross-attention (same text context).  The launch plan (tile shape) of problem 0 serves all; no K split. */
typedef struct dgq_gemm_args {
    const int8_t* codes; const float* rowsum; int rowsum_parts; int M, Kp;
    const void* wpacked; int w_bits; int N;
    int per_m; const float* cdelta; const uint8_t* cflush; const float* mdelta; const float* mzp; int L; float offset;
    const float* alpha; const float* zw; const float* gamma; const float* vn;
    void* y; int y_dtype; int ldy;
    const dgq_gemm_extra_t* extra;
} dgq_gemm_args_t;
int dgq_gemm_wxa8_batch(int n, const dgq_gemm_args_t* args, void* stream);

/* dgq_gemm_blockq: the layer under the real-time block quantiser (dgq_quant_act_block), one launch, no K split, nothing exchanged
 * between workgroups.  With s the centred codes, qw' / zw the stored weight codes and their zero point, P[m,n,c] = Σ_{k∈c} s·qw' (a
 * FRESH int32 accumulator per 32-chunk c: no running total, no clear marks), Vc[n,c] = Σ_{k∈c} (qw' − zw):
 *   y[m,n] = gamma[n] + alpha[n]·( Σ_c ( δ[m,c]·float(P[m,n,c]) + β[m,c]·Vc[n,c] ) − zw[n]·R[m] ),   R[m] = Σ_c δ[m,c]·rs[m,c]
 * (chunks in ascending order, per chunk first the δ·P term, then the β·Vc term, one fp32 fma each).  Row m = (b·Ho + ho)·Wo + wo, chunk
 * c = tap·(C/32) + cb reads the 32 code bytes and the table entry cb of input pixel (ho·stride − pad + dh, wo·stride − pad + dw)
 * (>> 1 with ups); a tap outside the image contributes exactly 0 (δ = β = 0), and R[m] adds the in-image taps' rho in tap order.  A Linear
 * layer is B = rows, H = W = kh = kw = stride = 1, pad = 0.
 * Of `g` are read: codes / rowsum (= the quantiser's codes and rho, rowsum_parts 1), M = B·Ho·Wo, Kp (>= kh·kw·C, a multiple of
 * DGQ_KTILE), wpacked + w_bits (the natural-order image: dgq_pack_w4 layout 1 / dgq_pack_w8 with kperm == NULL), N, alpha, zw, gamma
 * (= bias), y, y_dtype, ldy and extra (residual / res_div, fq_*, geglu, gn_partial, y2 / ldy2 as for dgq_gemm_wxa8; conv and act must be
 * NULL, flush_coef and wfrag are ignored); the scale-mode fields are ignored.  vc [N][Kp/32] fp32 (integer-valued, 0 on padding chunks). */
typedef struct dgq_gemm_block {
    const float* table; int ldt;      /* dgq_act_block_out_t.table / ldt */
    const float* vc;
    int B, H, W, C, kh, kw, stride, pad, ups;
} dgq_gemm_block_t;
int dgq_gemm_blockq(const dgq_gemm_args_t* g, const dgq_gemm_block_t* blk, void* stream);

/* ---- real-time MXFP6 activations on the block-scaled matrix cores (W4A6; a mode of this library) -------------------------------------
 * Every block of DGQ_KCHUNK = 32 consecutive channels of every input row gets ONE power-of-two scale 2^E and 32 FP6 E2M3 codes (sign, 2
 * exponent bits of bias 1, 3 mantissa bits: magnitudes 0 .. 0.875 and 1 .. 1.875 in steps of 0.125, 2 .. 3.75 of 0.25, 4 .. 7.5 of 0.5).
 * With amax = max |x′| of the block: E = floor(log2 amax) − 2 (the exponent field of amax; the OCP MX rule with E2M3's emax = 2), clamped
 * to [−127, 127], E = −127 for amax = 0; code = x′·2^−E rounded to nearest, ties to even, onto the grid, saturating at ±7.5 (a zero
 * magnitude is stored +0); x̂ = code·2^E.  The statement is dgq_amd/quant/quant_layer.py mx6_block.
 * dgq_quant_act_mx6: `in` is read exactly as by dgq_quant_act_block (x, x_dtype, B, H, W, C, the folded prologue, ups; C % 32 == 0, x
 * 16-byte aligned; kh, kw tell a Linear input from a convolution's; bits is only range-checked).  ONE launch, no atomics, capture-safe:
 *   codes [rows][C/32][24 bytes], 16-byte aligned: element j of a block at bits 6j .. 6j + 5 of its 192-bit little-endian string — the
 *         FP6 operand image of V_MFMA_SCALE_F32_32X32X64_F8F6F4;
 *   scale [rows][lds] E8M0 bytes E + 127, lds >= C/32; entries C/32 .. lds − 1 are written 127.
 * dgq_dequant_act_mx6: y [rows][C] (y_dtype) = x̂ from such codes and scales — the quantizer's stand-alone fake-quant form.
 * dgq_pack_w_mx6: the weight image of dgq_gemm_mx6 from the integer codes [N][C·taps] (reference order k = c·taps + tap) and the zero
 * points zw [N] (integers; |q − z| <= 15 — the caller's check): packed [N][Kp/32][24 bytes] = the E2M3 codes of (q − z)/2, each a grid
 * value, K in the natural order kp = tap·C + c, the K padding up to Kp (a multiple of DGQ_KTILE) as code 0.
 * dgq_gemm_mx6: y[m,n] = gamma[n] + alpha[n]·Σ_c 2^(E[m,c]+1)·Σ_{k∈c} a[m,k]·w6[n,k], every K step one block-scaled MFMA (activations
 * the A operand under their own scale bytes, weights the B operand under the constant byte 128), ONE fp32 accumulator over the whole K,
 * no K split, nothing exchanged between workgroups.  Rows, chunks, taps, ups and the Linear case as for dgq_gemm_blockq (a tap outside
 * the image contributes exactly 0).  Of `g` are read: codes (= the quantiser's codes), M, Kp, wpacked (dgq_pack_w_mx6), N, alpha (= δw),
 * gamma (= bias), y, y_dtype, ldy and extra (as for dgq_gemm_blockq; conv and act must be NULL); everything else is ignored. */
typedef struct dgq_act_mx6_out {
    uint8_t* codes; uint8_t* scale; int lds;
} dgq_act_mx6_out_t;
int dgq_quant_act_mx6(const dgq_quant_act_args_t* in, const dgq_act_mx6_out_t* out, void* stream);
int dgq_dequant_act_mx6(const uint8_t* codes, const uint8_t* scale, int lds, int64_t rows, int C, void* y, int y_dtype, void* stream);
int dgq_pack_w_mx6(const uint8_t* codes, const float* zw, int N, int C, int taps, int Kp, uint8_t* packed, void* stream);
typedef struct dgq_gemm_mx6 {
    const uint8_t* scale; int lds;    /* dgq_act_mx6_out_t.scale / lds */
    int B, H, W, C, kh, kw, stride, pad, ups;
} dgq_gemm_mx6_t;
int dgq_gemm_mx6(const dgq_gemm_args_t* g, const dgq_gemm_mx6_t* mx, void* stream);
/* Small tile grids are split along K (deterministic: fp32 partial slabs [S][M][N] in the caller's `workspace`,
 * summed in a fixed order by a second kernel). dgq_gemm_workspace_bytes returns what the preferred split of a
 * shape needs; with workspace == NULL (or too small) fewer / no splits are used — results do not depend on it
 * beyond fp32 summation order. */
size_t dgq_gemm_workspace_bytes(int M, int N, int Kp);
int dgq_gemm_plan_splits(int M, int N, int Kp, int w_bits, int per_m, size_t workspace_bytes);

/* ---- attention-side quantizers --------------------------------------------------------------------
 * dgq_fakequant_rows: aqtizer_q/k/v (sd.py:174-182,199 -> quant_layer.py:295-299) applied on the
 * projection output viewed as [rows][C] (row = b·T + t, col = h·D + d): y = δ·(clamp(rne(x/δ)+z,0,2^b−1) − z).
 *   mode 0: scalar (delta[0]);  mode 1: per token, index (row % T) − skip;  mode 2: per head-dim, index col % D.
 * Tokens t < skip are copied unquantised (start_peak bypass of token 0, sd.py:176-180). In-place allowed. */
int dgq_fakequant_rows(const void* x, void* y, int dtype, int rows, int C, int T, int D,
                       int mode, const float* delta, const float* zp, int skip, int bits, void* stream);

/* dgq_max_f32: out[0] = max over p[rows][S] excluding columns < skip_cols (real-time δ = x.max(),
 * quant_layer_text.py:96-97). `out` must be pre-set to 0 by the caller; probabilities are >= 0. */
int dgq_max_f32(const float* p, int64_t rows, int S, int skip_cols, float* out, void* stream);
/* dgq_logquant_f32: T2ILogQuantizer.forward (quant_layer_text.py:101-105) on softmax probabilities,
 * y = δ·2^(−clamp(rne(−log2(p/δ)),0,2^b−1)), δ read from device memory; columns < skip_cols are copied
 * (start_peak, sd.py:191-195). In-place allowed. */
int dgq_logquant_f32(const float* p, float* y, int64_t rows, int S, int skip_cols, const float* delta,
                     int bits, void* stream);

/* dgq_attention_f32: the attention core of Attention.Attention_forward (sd.py:183-201) without materialising the
 * probabilities:  o = aqtizer_w(softmax((q·kᵀ)·scale)) · v, all fp32 (exact fp32 MFMA).
 * q [B][T][H·D], k/v [B][S][H·D], o [B][T][H·D] (the projection layout: no head transposes).
 * mode 0: no quantiser; 1: T2ILogQuantizer real-time (δ = max probability over the whole [B,H,T,S≥skip] tensor,
 *         quant_layer_text.py:96-105, found by a first statistics pass); 2: T2ILogQuantizer with δ = delta_in[0];
 *         3: UniformAffineQuantizer always_zero with δ = delta_in[0] (quant_block.py:145-156).
 * skip = 1 bypasses key column 0 (start_peak, sd.py:191-195).  workspace: caller-owned, 256-byte aligned,
 * >= dgq_attention_workspace_bytes(...) (δ scalar, per-row softmax statistics, bf16 split planes of K and V).
 * head_dim D ∈ {8,16,40,64,80,160}.  Quantised modes run on the bf16 MFMA with exact three-way bf16 operand splits
 * (fp32-equivalent accuracy); mode 0 on the exact fp32 MFMA.  The quantised modes keep their running maxima over the
 * unscaled scores and need a finite scale > 0 (DGQ_EINVAL before any launch otherwise); mode 0 takes any finite scale.
 * fq (optional, NULL = none): the aqtizer_q / aqtizer_k / aqtizer_v fake-quantizers (sd.py:165-181) applied to the
 * operands as they are loaded, fq[0..2] = q, k, v, each addressed exactly like dgq_fakequant_rows (mode 0 scalar,
 * 1 per token with entry t − skip, 2 per head-dim element; mode < 0 = none for that operand; tokens < skip pass
 * through).  Only where dgq_attention_fuses_fakequant(D, mode) returns 1; DGQ_EUNSUPPORTED otherwise. */
typedef struct dgq_attn_fq {
    int mode;                  /* -1 none, 0 scalar, 1 per token, 2 per head-dim element */
    int skip;                  /* leading tokens left unquantised (start_peak key 0) */
    int bits;
    const float* delta;        /* device */
    const float* zero_point;   /* device */
} dgq_attn_fq_t;
int dgq_attention_f32(const float* q, const float* k, const float* v, float* o, int B, int H, int T, int S, int D,
                      float scale, int mode, int skip, const float* delta_in, int bits, const dgq_attn_fq_t* fq,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same for q/k/v/o of dtype DGQ_F32 / DGQ_F16 / DGQ_BF16 (the reference's --fp16 mode, quant_model.py:183-201):
 * the arithmetic is unchanged (operands widened to fp32 and split exactly, fp32 accumulation), only the loads and the
 * final store follow the tensors' dtype.  Half types are served where dgq_attention_fuses_fakequant(D, mode) is 1. */
int dgq_attention(const void* q, const void* k, const void* v, void* o, int dtype, int B, int H, int T, int S, int D,
                  float scale, int mode, int skip, const float* delta_in, int bits, const dgq_attn_fq_t* fq,
                  void* workspace, size_t workspace_bytes, void* stream);
int dgq_attention_fuses_fakequant(int D, int mode);
size_t dgq_attention_workspace_bytes(int B, int H, int T, int S, int D);
/* Calls whose key range is at most 8 tiles (S <= 256: every cross-attention over the text tokens, the 16x16 / 8x8 self-attentions)
 * run statistics, the real-time δ maximum and P·V in ONE launch (csrc/attn_one.hip; results equal to the three-launch form bit for
 * bit).  Under mode 1 the workgroups of that launch exchange their maxima through the workspace and wait for each other with a
 * bounded poll; the form is taken only for grids that are resident as a whole.  dgq_attention_sync_timeouts: how many workgroups ever
 * gave up that poll in this process (device counter, read with a synchronous copy; 0 unless a grid was not resident — then the
 * affected call's output is invalid); < 0 on a runtime error.  DGQ_ATTN_ONE=0 in the environment keeps every call on three launches. */
int dgq_attention_sync_timeouts(void);

/* dgq_attention_mfma16: o = softmax((q·kᵀ)·scale)·v with NO quantiser (mode 0 of dgq_attention) on fp16 / bf16 tensors, on the bf16 / f16
 * matrix cores, in ONE launch with no workspace (csrc/attn_mfma16.hip).  Layout of dgq_attention: q [B][T][H·D], k / v [B][S][H·D],
 * o [B][T][H·D], all of `dtype` and 16-byte aligned.  Per (batch, head, query): s_j = fp32(Σ_d q_d·k_{j,d})·scale (the 16-bit products are
 * exact in fp32, fp32 accumulation); online softmax over key tiles in fp32 (running maximum m, p_j = exp(s_j − m), l and the
 * accumulator rescaled when m moves); p_j is rounded to `dtype` (nearest even) for the P·V product only — l sums the unrounded p_j;
 * o = round_dtype(acc / l).  Per element |o − o64| <= (2u + 2E + 2^-16)·Σ_j p_j|v_j| + u·|o64|, u = 2^-9 (bf16) / 2^-11 (f16),
 * E = max_j D·2^-24·scale·Σ_d |q_d·k_{j,d}|.  dtype DGQ_F16 or DGQ_BF16; DGQ_F32 returns DGQ_EUNSUPPORTED (the fp32
 * state keeps dgq_attention's exact kernel).  D ∈ {8,16,40,64,80,160} (zero padded to the MFMA depth inside the kernel), any
 * B, H, T, S >= 1 with B·H <= 65535.  Launches on `stream`, allocates nothing, does not synchronise. */
int dgq_attention_mfma16(const void* q, const void* k, const void* v, void* o, int dtype, int B, int H, int T, int S, int D,
                         float scale, void* stream);

/* dgq_attention_mfma16_f32: the same attention on fp32 tensors, still on the bf16 matrix cores, in ONE launch with no workspace
 * (csrc/attn_mfma16.hip, the same kernel body).  Every fp32 operand enters as its two-term bf16 split hi = bf16_rn(x), lo = bf16_rn(x − hi):
 * s_j = scale·fp32(Σ_d q_lo·k_hi + q_hi·k_lo + q_hi·k_hi), online softmax in fp32 as above (l sums the unrounded p_j),
 * acc += p_lo·v_hi + p_hi·v_lo + p_hi·v_hi, o = acc / l with an IEEE division; the lo·lo terms are dropped.  Per element
 * |o − o64| <= (2E + 2^-15)·Σ_j p_j|v_j| + 2^-24·|o64|, E = (3·2^-18 + 3·D·2^-24)·|scale|·max_j Σ_d |q_d·k_{j,d}|.
 * Layout, head dims, geometry limits and alignment of dgq_attention_mfma16; fp32 tensors keep dgq_attention (mode 0, the exact fp32
 * MFMA) unless a caller asks for this entry.  Launches on `stream`, allocates nothing, does not synchronise. */
int dgq_attention_mfma16_f32(const float* q, const float* k, const float* v, float* o, int B, int H, int T, int S, int D, float scale,
                             void* stream);

/* ---- batched small-M Linear ------------------------------------------------------------------------
 * dgq_linear_smallm_batch: y_l = W_l·aqtizer_l(act(x)) + b_l for up to 24 quantized Linear layers that share one input
 * x [M][K] of M <= 16 rows — the time_emb_proj(SiLU(temb)) projections of every resnet block of a forward
 * (quant_block.py:98-119), which do not depend on the latents — in ONE launch: quantise-on-load (scalar activation
 * quantizer of each layer, SiLU prologue when pre_act == 1) + integer dot products + the per_m epilogue of dgq_gemm_wxa8
 * (same arithmetic, term for term).  Weights in the natural K order (dgq_pack_w4 layout 1 / dgq_pack_w8 with kperm == NULL... Kp
 * padded to DGQ_KTILE); K <= 2048.  probs: host array, copied into the kernel arguments. */
typedef struct dgq_smallm_problem {
    const void* wpacked;
    const float* alpha;
    const float* zw;
    const float* gamma;
    const float* vn;
    const float* mdelta;
    const float* mzp;
    void* y;
    int ldy, N, Kp, w_bits, a_bits;
} dgq_smallm_problem_t;
int dgq_linear_smallm_batch(const void* x, int x_dtype, int M, int K, int64_t ldx, int pre_act, int n_problems,
                            const dgq_smallm_problem_t* probs, int y_dtype, void* stream);

/* ---- calibration producer --------------------------------------------------------
 * dgq_minmax_rows_cols: the statistics UniformAffineQuantizer.record_min_max_ema collects for DGQ's grouping
 * (quant/quant_layer.py:301-313): for x viewed as [rows][C] (row stride ldx elements, any fp dtype) the row-wise
 * (rowmin/rowmax [rows]) and column-wise (colmin/colmax [C]) minima / maxima, fp32.  Either pair may be NULL.
 * partial_ws: 2·slices·C floats of caller-owned scratch for the column pass (slices = row slices reduced in parallel). */
int dgq_minmax_rows_cols(const void* x, int dtype, int rows, int C, int64_t ldx,
                         float* rowmin, float* rowmax, float* colmin, float* colmax,
                         float* partial_ws, int slices, void* stream);

/* ---- weight PTQ: AdaRound soft quantiser + rounding regulariser -------------------------
 * The elementwise device ops of the reconstruction loop (reference: quant/adaptive_rounding.py:39-70 with soft_tgt,
 * quant/reconstruction_util.py:68-70), forward and backward; w, alpha, out, gout, galpha are [N][K] fp32 (K = the
 * flattened C·kh·kw), delta / zp [N] per output channel.
 *   soft_fwd : out = δ·(clamp(floor(w/δ) + h(α) + z, 0, 2^bits − 1) − z),  h(α) = clamp(sigmoid(α)·1.2 − 0.1, 0, 1)
 *   soft_bwd : galpha = gout · ∂out/∂α  (the clamps pass the gradient on their closed intervals, as torch.clamp)
 *   reg_fwd  : partial[blk] = Σ_blk (1 − |2h(α) − 1|^b); blk < dgq_adaround_reg_blocks(numel); the caller adds them up
 *   reg_bwd  : galpha = g[0] · ∂/∂α Σ (1 − |2h(α) − 1|^b); g is a 1-element device tensor (no host sync) */
int dgq_adaround_soft_fwd(const float* w, const float* delta, const float* zp, const float* alpha, int N, int K, int bits,
                          float* out, void* stream);
int dgq_adaround_soft_bwd(const float* gout, const float* w, const float* delta, const float* zp, const float* alpha, int N,
                          int K, int bits, float* galpha, void* stream);
int dgq_adaround_reg_blocks(int64_t numel);
int dgq_adaround_reg_fwd(const float* alpha, int64_t numel, float b, float* partial, void* stream);
int dgq_adaround_reg_bwd(const float* alpha, int64_t numel, float b, const float* g, float* galpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif
