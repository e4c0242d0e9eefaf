/*
 * nsg.h -- C ABI of libnsg.so: hand-written gfx950 (MI355X / CDNA4) kernels for the VQ-VAE
 * training hot path of dendisuhubdy/neural_sound_generation.
 *
 * The reference has no native code on this path: it reaches its arithmetic through PyTorch ATen
 * operators.  Each entry point below therefore replaces one ATen call site of the reference
 * (file:line given per function, relative to the reference repository root).  The reference-side
 * binding a maintainer would add (ctypes, from src/models.py / src/vector_quantization.py) is
 * shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (including
 *     workspaces); the library allocates nothing, frees nothing, keeps no pointer after return;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only ENQUEUE work,
 *     they never synchronise;
 *   - return value: 0 = OK, <0 = invalid argument / unsupported shape (NSG_E_*), >0 = hipError_t;
 *     a message for the calling thread's last failure is available from nsg_last_error_string();
 *   - activations are fp32 NHWC ("channels last"): a tensor the reference holds as (B,C,H,W) is
 *     stored here as [B][H][W][C].  For C == 1 (the mel input and the reconstruction) the two
 *     layouts coincide.  Convolution weights are passed in the reference's own layouts
 *     (Conv2d: [C_out][C_in][kH][kW], ConvTranspose2d: [C_in][C_out][kH][kW]) and re-packed on the
 *     device by nsg_pack_conv_weights();
 *   - element counts of any single tensor must stay below 2^31.
 */
#ifndef NSG_H_
#define NSG_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define NSG_API __attribute__((visibility("default")))
#else
#define NSG_API
#endif

#define NSG_VERSION 104 /* bumped HERE on ANY change of an existing entry point's signature; _lib.py binds from this header and refuses a library of another version */

enum {
    NSG_OK = 0,
    NSG_E_INVALID = -1,     /* null pointer / non-positive size / misaligned pointer */
    NSG_E_UNSUPPORTED = -2, /* shape outside what the kernels implement (see each function) */
    NSG_E_WORKSPACE = -3    /* workspace too small */
};

/* storage type of activations / packed weights: fp32 is the parity mode, bf16 (fp32 accumulate,
 * fp32 BatchNorm statistics, fp32 VQ) the throughput mode */
enum { NSG_F32 = 0, NSG_BF16 = 1 };

/* flags shared by the convolution entry points */
enum {
    NSG_RELU_IN = 1,   /* apply max(0,.) to the (gathered) input operand while loading it          */
    NSG_TANH_OUT = 2,  /* apply tanh to the result (forward only)                                   */
    NSG_RELU_IN2 = 4,  /* wgrad only: apply max(0,.) to the output-side operand (see nsg_conv_wgrad) */
    NSG_OUT_F32 = 8,   /* forward only: write y as fp32 even when the layer's dtype is bf16          */
    NSG_RELU_OUT = 16  /* forward only: apply max(0,.) to the result (the consumer's leading ReLU)   */
};

/* Geometry of one convolution layer.  transposed = 0: nn.Conv2d(C_in, C_out, k, stride, pad);
 * transposed = 1: nn.ConvTranspose2d(C_in, C_out, k, stride, pad).  (IH,IW) is the layer's input
 * extent, (OH,OW) its output extent; both are given so the library never has to guess.
 * Supported: Conv2d with any k <= 7 (rectangular: see k_w), stride in {1,2}; ConvTranspose2d with k=4, stride=2, pad=1
 * (the VQ-VAE's transposed geometry: src/models.py:179,182) and, fp32 only, ConvTranspose2d with stride=1, square k <= 7,
 * 0 <= pad < k, OH = IH + k - 1 - 2 pad (the VAE decoder's: src/models.py:85,88), C_in and C_out multiples of 4, C_out > 1:
 * its forward is the data gradient of Conv2d(C_out, C_in, k, 1, pad) over the same weight tensor and runs on that kernel.
 * C_in and C_out must be multiples of 4 or equal to 1. */
typedef struct nsg_conv_desc {
    int32_t B, IH, IW, C_in;
    int32_t OH, OW, C_out;
    int32_t k, stride, pad;
    int32_t transposed;
    int32_t dtype; /* NSG_F32 / NSG_BF16: storage type of the multi-channel activations and of the packed
                      weights.  Single-channel tensors (C == 1: the mel image, the reconstruction and their
                      gradients), biases, weight gradients and the reference-layout weights are always fp32.
                      bf16 needs channel counts that are multiples of 8. */
    int32_t k_w;   /* 0: square kernel (k x k, pad on both dimensions).  > 0: rectangular Conv2d (stride 1,
                      C_in > 1): k x k_w taps, padding (pad, pad_w), reference weight layout (C_out, C_in, k, k_w).
                      A stride-1 output may also be CROPPED at the bottom / right: OH / OW smaller than the full
                      extent (the pad-then-crop of the prior's masked stacks, src/models.py:268-273). */
    int32_t pad_w; /* column padding when k_w > 0 */
} nsg_conv_desc;

NSG_API int nsg_version(void);
NSG_API const char *nsg_last_error_string(void);

/* ---------------------------------------------------------------------------------------------
 * Vector quantiser                                        src/vector_quantization.py
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace nsg_vq_forward needs for N rows and K codes. */
NSG_API size_t nsg_vq_workspace_bytes(int64_t N, int32_t D, int32_t K);

/* Fused nearest-code search.  Replaces VectorQuantization.forward (vector_quantization.py:6-23:
 * torch.sum(x**2), torch.sum(e**2), torch.addmm(..., alpha=-2, beta=1), torch.min(dim=1)) and the
 * gather of VectorQuantizationStraightThrough.forward (:40-42, torch.index_select), without ever
 * materialising the (N,K) distance matrix.
 *   x [N][D] fp32 rows, e [K][D] fp32 codebook, idx_out [N] int64 (first minimal index on ties,
 *   bit-exact with the reference's CPU result -- see DESIGN.md "bit-exact argmin"),
 *   codes_out [N][D] = e[idx] or NULL, dmin_out [N] fp32 minimal distance or NULL.
 * Supported: 1 <= D <= 256, K >= 1. */
NSG_API int nsg_vq_forward(const float *x, const float *e, int64_t N, int32_t D, int32_t K, int64_t *idx_out,
                           float *codes_out, float *dmin_out, void *workspace, size_t workspace_bytes, void *stream);

/* The same search for the bf16 compute mode: the contraction runs on the bf16 matrix pipe with both fp32 operands
 * split into bf16 hi + lo parts (3 MFMAs per 16 channels, fp32 accumulate): distances carry a relative error of
 * ~2^-16, so on near-ties the chosen code may differ from the reference's (NOT the bit-exact search; the fp32
 * parity mode uses nsg_vq_forward).  D % 8 == 0, D <= 256.  Workspace: nsg_vq_bf16x3_workspace_bytes.
 * idx_out is the FIRST minimum of the COMPUTED distances: codes whose computed distances are equal -- exact duplicates of a
 * code row always are -- resolve to the lowest index; dmin_out (or NULL) is that computed distance.
 * codes_bf16_out (or NULL): the chosen code rows as bf16 [N][D], with max(0, .) applied when bf16_relu != 0 -- the
 * decoder's input after its leading ReLU (models.py:176) in the bf16 mode, written here instead of by a separate
 * conversion pass over an fp32 copy (codes_out may then be NULL: nsg_vq_losses_indexed reads the codebook itself). */
NSG_API size_t nsg_vq_bf16x3_workspace_bytes(int64_t N, int32_t D, int32_t K);
NSG_API int nsg_vq_forward_bf16x3(const float *x, const float *e, int64_t N, int32_t D, int32_t K, int64_t *idx_out,
                                  float *codes_out, float *dmin_out, void *codes_bf16_out, int32_t bf16_relu, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* The same with a per-clip conditioning row folded into the bf16 code write (BASELINE configs[2], the speaker-conditioned
 * decoder; an extension: the reference loads the speaker id and ignores it, src/train.py:114): row n belongs to clip
 * n / rows_per_clip and codes_bf16_out[n] = [relu]( e[idx[n]] + clip_rows[clip] ), clip_rows fp32 [clips][D].  idx_out,
 * codes_out and dmin_out are unaffected.  clip_rows == NULL is nsg_vq_forward_bf16x3. */
NSG_API int nsg_vq_forward_bf16x3_cond(const float *x, const float *e, int64_t N, int32_t D, int32_t K, int64_t *idx_out,
                                       float *codes_out, float *dmin_out, void *codes_bf16_out, int32_t bf16_relu,
                                       const float *clip_rows, int64_t rows_per_clip, void *workspace, size_t workspace_bytes,
                                       void *stream);

/* Rows given as their SOURCES instead of as fp32 values (the *_bnres entry points below): the encoder's last ResBlock ends in
 * BatchNorm + skip connection (src/models.py:154-158), so every element of its output z_e is
 *     z[n][c] = ((h[n][c] - mean[c]) * (invstd[c] * gamma[c]) + beta[c]) + r[n][c]
 * with h (the BatchNorm's input) and r (the block's ReLU'd input) bf16 [N][D] and the four vectors fp32 [D].  The three
 * consumers of z_e in the bf16 training step -- the search, the loss / encoder gradient and the per-code sums -- form this
 * expression while they load their rows, exactly as nsg_bn_apply(h, ..., residual = r) spells it for an fp32 output (same order
 * of operations, no contraction), so each returns bit for bit what its fp32-row form returns on nsg_bn_apply's result: the
 * fp32 copy of z_e (a pass that reads 2 x N*D*2 bytes and writes N*D*4, then read three times) is never made. */

/* nsg_vq_forward_bf16x3_cond on such rows (no dmin_out: the distances' |x|^2 pass would need the rows).  h, r 16-byte aligned. */
NSG_API int nsg_vq_forward_bf16x3_bnres(const void *h, const void *r, const float *mean, const float *invstd, const float *gamma,
                                        const float *beta, const float *e, int64_t N, int32_t D, int32_t K, int64_t *idx_out,
                                        float *codes_out, void *codes_bf16_out, int32_t bf16_relu, const float *clip_rows,
                                        int64_t rows_per_clip, void *workspace, size_t workspace_bytes, void *stream);

/* out[r] = torch.sum(v[r]**2) with ATen's CPU summation order (vector_quantization.py:12-13). */
NSG_API int nsg_rowsumsq(const float *v, int64_t rows, int32_t D, float *out, void *stream);

/* Bytes of workspace for nsg_index_add_rows. */
NSG_API size_t nsg_index_add_workspace_bytes(int64_t N, int32_t D, int32_t K);

/* out[k][:] = sum over rows i with idx[i] == k of g[i][:]  (out fully overwritten).
 * Replaces grad_codebook.index_add_(0, indices, grad_output) (vector_quantization.py:60-61) and the
 * autograd of torch.index_select(self.embedding.weight, 0, indices) (src/models.py:137-138); also
 * yields the per-code sums of the EMA codebook extension.  Deterministic (fixed summation order).
 * counts_out [K] fp32 (rows per code) or NULL.
 * Out-of-range indices, in ALL index-add forms (this one, _bf16x2, _sorted, _sorted_bnres): a row whose index lies outside
 * [0, K) contributes nothing to the sums and nothing to the counts.  The index is compared as the 64-bit value it is (2^32 + 3
 * is out of range, not code 3); no address is ever formed from such an index.  A batch with no index in range gives zeros. */
NSG_API int nsg_index_add_rows(const int64_t *idx, const float *g, int64_t N, int32_t D, int32_t K, float *out,
                               float *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* The same for the bf16 compute mode: the one-hot reduction runs on the bf16 matrix pipe with g split into bf16
 * hi + lo parts (relative error of a sum ~2^-17; deterministic).  Falls back to nsg_index_add_rows's kernel when
 * D is not a multiple of 8 or D <= 32.  Same workspace. */
NSG_API int nsg_index_add_rows_bf16x2(const int64_t *idx, const float *g, int64_t N, int32_t D, int32_t K, float *out,
                                      float *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* The same sums as a sorted segment sum: a stable counting sort of the row INDICES by code, then every code's rows added in
 * row order (fp32, bitwise reproducible).  Moves N*D*4 bytes instead of doing 2*N*K*D flops: the form for large codebooks
 * (K = 8192) and the default of the training step.  Rows whose index lies outside [0, K) contribute nothing (see above).
 * Shapes: D in {4, 8, 16, 32, 64, 128, 256} (D / 4 a power of two up to 64) or D a multiple of 256; K <= 8192; N < 2^31.
 * Every other width (D = 260, say) is refused with NSG_E_UNSUPPORTED; ops.index_add_sorted_supported states the same rule. */
NSG_API size_t nsg_index_add_sorted_workspace_bytes(int64_t N, int32_t D, int32_t K);
NSG_API int nsg_index_add_rows_sorted(const int64_t *idx, const float *g, int64_t N, int32_t D, int32_t K, float *out,
                                      float *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* The same on rows given as their sources (see nsg_vq_forward_bf16x3_bnres): every lane adds the values the fp32 rows would
 * hold, in the same order.  D a power of two, 4 <= D <= 256.  Same workspace. */
NSG_API int nsg_index_add_rows_sorted_bnres(const int64_t *idx, const void *h, const void *r, const float *mean, const float *invstd,
                                            const float *gamma, const float *beta, int64_t N, int32_t D, int32_t K, float *out,
                                            float *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* out[i][:] = e[idx[i]][:] for i < N.  Replaces torch.index_select(codebook, 0, indices)
 * (vector_quantization.py:40-41, src/models.py:137) and self.codebook.embedding(latents)
 * (src/models.py:194).  Indices outside [0,K) are clamped. */
NSG_API int nsg_gather_rows(const float *e, const int64_t *idx, int64_t N, int32_t D, int32_t K, float *out,
                            void *stream);

/* Codebook gradient of loss_vq = mse(codebook[idx], sg(z_e)) (src/train.py:131 through index_select, src/models.py:137)
 * from per-code statistics instead of an (N, D) gradient tensor: with n[k] rows assigned to code k and s[k] = their sum
 * (nsg_index_add_rows over z_e with counts),  out[k][:] = scale * (n[k] * e[k][:] - s[k][:]),  scale = 2 / (N*D). */
NSG_API int nsg_codebook_grad_from_sums(const float *e, const float *n, const float *s, int32_t K, int32_t D, float scale,
                                        float *out, void *stream);

/* EMA codebook update (extension, not in the reference; VQ-VAE paper appendix A.1):
 *   ema_n = decay*ema_n + (1-decay)*n;  ema_s = decay*ema_s + (1-decay)*s;
 *   e[k] = ema_s[k] / ((ema_n[k]+eps) / (sum(ema_n) + K*eps) * sum(ema_n)).
 * n [K], s [K][D] are the (all-reduced) batch statistics from nsg_index_add_rows.
 * scratch: one device float (holds sum(ema_n) between the two kernels). */
NSG_API int nsg_vq_ema_update(float *e, float *ema_n, float *ema_s, const float *n, const float *s, int32_t K,
                              int32_t D, float decay, float eps, float *scratch, void *stream);

/* Codebook usage statistics and dead-code revival (extension, not in the reference: its plain nearest-neighbour codebook at the
 * U(-1/K, 1/K) initialisation keeps a handful of live codes).  Integer atomics only: every result is independent of arrival order.
 *
 * nsg_code_usage: batch_counts[k] (int32 [K], overwritten) = number of rows with idx == k, rows whose index lies outside [0, K)
 * ignored (as nsg_index_add_rows_sorted ignores them); window[k] (int32 [K]) += batch_counts[k]; stats (two doubles):
 *   stats[0] = the batch's perplexity exp(-sum_k p_k ln p_k), p_k = batch_counts[k] / sum(batch_counts), accumulated in fp64 in a
 *              fixed order (0 when no index lies in range);   stats[1] = the number of codes with batch_counts > 0.
 * 1 <= N < 2^31, K >= 1 (K <= 8192: per-block LDS bins, one global atomic per block and non-zero bin; larger K: global atomics).
 * No workspace: batch_counts is cleared by an asynchronous memset on the stream. */
NSG_API int nsg_code_usage(const int64_t *idx, int64_t N, int32_t K, int32_t *batch_counts, int32_t *window, double *stats, void *stream);

/* Re-seed the dead codes from rows of the current encoder output z [N][D] (fp32 rows, or their sources: the _bnres form, see
 * nsg_vq_forward_bf16x3_bnres; each row is formed exactly as nsg_bn_apply(..., residual = r) forms it for an fp32 output).
 *   - code k is DEAD when window[k] < min_count, or when revive_all != 0;  j(k) = the number of dead codes with an index below k;
 *   - slot[k] (int32 [K], out) = j(k) for a dead code, -1 for a live one;
 *   - a dead code takes codebook[k][:] = z[(base_row + j(k) * stride) mod N][:], a bit-for-bit copy (64-bit index arithmetic);
 *     where given (pairs, each nullable): adam_m[k][:] = adam_v[k][:] = 0 (the optimiser's moments of that row, [K][D]);
 *     ema_count[k] = 1 and ema_sum[k][:] = the same row (the EMA codebook's statistics);
 *   - live rows of every array are not written at all;   afterwards window is all zero;
 *   - stats (two int64): stats[0] = the number of revived codes, stats[1] += it (a running total the caller zeroes once).
 * The rows chosen for different dead codes are pairwise distinct while stride is coprime to N (the caller's duty) and there are
 * at most N dead codes; beyond that rows repeat.
 * NSG_E_INVALID: a null required pointer, N < 1 or >= 2^31, K < 1, stride < 1 or >= 2^31, base_row outside [0, N), half a pair;
 * NSG_E_UNSUPPORTED: D % 4 != 0 (the _bnres form: D not a power of two in 8 ... 256), tensors not 16-byte aligned. */
NSG_API int nsg_vq_revive(const float *z, int64_t N, int32_t D, float *codebook, int32_t K, int32_t *window, int32_t min_count,
                          int64_t base_row, int64_t stride, float *adam_m, float *adam_v, float *ema_count, float *ema_sum,
                          int32_t *slot, int64_t *stats, int32_t revive_all, void *stream);
NSG_API int nsg_vq_revive_bnres(const void *h, const void *r, const float *mean, const float *invstd, const float *gamma,
                                const float *beta, int64_t N, int32_t D, float *codebook, int32_t K, int32_t *window,
                                int32_t min_count, int64_t base_row, int64_t stride, float *adam_m, float *adam_v, float *ema_count,
                                float *ema_sum, int32_t *slot, int64_t *stats, int32_t revive_all, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Convolutions                                            src/models.py:150,153,165,168,179,182
 * ------------------------------------------------------------------------------------------- */

/* ELEMENTS (of d->dtype) to allocate for each packed weight image (forward image, dgrad image).
 * (The two single-channel layers keep one of their images as fp32 [C][16] for the stencil kernels whatever
 * d->dtype is; bf16 layers whose channel counts the patch-staged kernel takes -- a multiple of 128 on one side and of
 * 64 on the other -- carry a second, fragment-ordered copy behind the plain [tap][n][c] image, which the bf16 conv
 * forward / data gradient reads: the count accounts for both.  Packed images are only ever produced by
 * nsg_pack_conv_weights(_batch) into buffers of exactly this size.) */
NSG_API size_t nsg_packed_weight_floats(const nsg_conv_desc *d);

/* Re-pack reference-layout weights into the two [tap][n][c] images the GEMM kernels stream:
 * w_fwd for nsg_conv_forward, w_dgrad for nsg_conv_dgrad (either may be NULL to skip it). */
NSG_API int nsg_pack_conv_weights(const nsg_conv_desc *d, const float *w, void *w_fwd, void *w_dgrad, void *stream);

/* The same for n layers in ONE kernel launch (a training step re-packs every layer after the optimiser
 * step): descs[n], w[n], w_fwd[n], w_dgrad[n] are host arrays; NULL image pointers are skipped. */
NSG_API int nsg_pack_conv_weights_batch(int32_t n, const nsg_conv_desc *descs, const float *const *w,
                                        void *const *w_fwd, void *const *w_dgrad, void *stream);

/* Workspace bytes for forward/dgrad (C == 1 layers stage im2col/col2im images) and wgrad (split-K slabs). */
NSG_API size_t nsg_conv_workspace_bytes(const nsg_conv_desc *d);

/* y = conv(x) + bias.  Replaces F.conv2d / F.conv_transpose2d as called by nn.Conv2d /
 * nn.ConvTranspose2d.forward at src/models.py:150,153,165,168,179,182.
 * flags: NSG_RELU_IN (the preceding nn.ReLU fused into the load), NSG_TANH_OUT (models.py:183).
 * CONTRACT for w_fwd here and w_dgrad in nsg_conv_dgrad*: the pointer is an image written by nsg_pack_conv_weights(_batch) for
 * the SAME descriptor into a buffer of nsg_packed_weight_floats(d) elements.  For the bf16 shapes the patch-staged kernel takes
 * that count is TWICE taps * C_out * C_in: the kernel reads the fragment-ordered copy that the packer put behind the plain image
 * and cannot tell a shorter caller-made buffer from a packed one (it would read past it).  tests/test_abi.py pins the sizes. */
NSG_API int nsg_conv_forward(const nsg_conv_desc *d, const void *x, const void *w_fwd, const float *bias, void *y,
                             int32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* nsg_conv_forward plus the training-mode BatchNorm statistics of its output y in the same pass:
 * nn.Conv2d / nn.ConvTranspose2d followed by nn.BatchNorm2d (src/models.py:165-166, 150-151,
 * 153-154, 179-180).  The conv epilogue reduces each 128-row output tile to (count, mean, M2) while
 * the tile is still in LDS; the tiles are merged exactly as nsg_bn_stats merges its slabs.
 * mean/invstd/running_* as in nsg_bn_stats.  NSG_TANH_OUT is not allowed here.
 * CONTRACT: nsg_conv_workspace_bytes(d) holds the statistics records of whichever kernel runs the layer (one per 128-row tile, or
 * one per workgroup of the patch-staged bf16 kernel: up to 512, whatever the image's shape); a smaller workspace is refused with
 * NSG_E_WORKSPACE BEFORE anything is launched. */
NSG_API int nsg_conv_forward_bnstats(const nsg_conv_desc *d, const void *x, const void *w_fwd, const float *bias,
                                     void *y, int32_t flags, float eps, float momentum, float *mean, float *invstd,
                                     float *running_mean, float *running_var, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* dx = d loss / d x given dy (autograd of the calls above).  flags: none. */
NSG_API int nsg_conv_dgrad(const nsg_conv_desc *d, const void *dy, const void *w_dgrad, void *dx, int32_t flags,
                           void *workspace, size_t workspace_bytes, void *stream);

/* The same with the rest of a ResBlock's input gradient folded into the kernel's store:
 *   dx = (conv_dgrad(dy) + add) * (relu_x > 0)
 * add (or NULL): the gradient arriving over the skip connection; relu_x (or NULL): the ReLU'd tensor the
 * convolution read (src/models.py:149,158: x is overwritten by relu(x), so mask = relu_x > 0).  Both are laid
 * out like dx.  Replaces nsg_conv_dgrad + nsg_relu_backward_add (one write and one read of dx less). */
NSG_API int nsg_conv_dgrad_relu_add(const nsg_conv_desc *d, const void *dy, const void *w_dgrad, const void *add,
                                    const void *relu_x, void *dx, int32_t flags, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* dw (reference weight layout, fully overwritten) and dbias (or NULL) given x and dy.
 * flags: NSG_RELU_IN treats x as max(0,x) (the fused preceding ReLU).  Deterministic. */
NSG_API int nsg_conv_wgrad(const nsg_conv_desc *d, const void *x, const void *dy, float *dw, float *dbias,
                           int32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d over [M][C] (M = B*H*W)                     src/models.py:151,154,166,180
 * ------------------------------------------------------------------------------------------- */

NSG_API size_t nsg_bn_workspace_bytes(int64_t M, int32_t C);

/* Training-mode statistics: mean[C], invstd[C] = 1/sqrt(biased var + eps); if running_mean/var are
 * non-NULL they are updated with `momentum` (running_var takes the unbiased variance), as
 * F.batch_norm(training=True) does. */
NSG_API int nsg_bn_stats(const void *x, int64_t M, int32_t C, int32_t dtype, float eps, float momentum, float *mean,
                         float *invstd, float *running_mean, float *running_var, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Eval mode: mean = running_mean, invstd = 1/sqrt(running_var + eps). */
NSG_API int nsg_bn_eval_stats(const float *running_mean, const float *running_var, int32_t C, float eps, float *mean,
                              float *invstd, void *stream);

/* (BatchNorm entry points: x / residual / y_relu / dy / dx hold elements of `dtype` (NSG_F32 or NSG_BF16,
 * void* below; nsg_bn_apply may write y in a different y_dtype); statistics, per-channel parameters and all
 * arithmetic are fp32.  bf16 needs C % 8 == 0.) */
/* y = (x-mean)*invstd*gamma + beta; relu & 1: y = max(0,y); residual != NULL: y += residual
 * (relu_residual != 0: y += max(0,residual) -- the ResBlock's in-place-ReLU'd skip, models.py:149,158);
 * relu & 2: y = max(0,y) once more at the very end -- the NEXT ResBlock's leading in-place ReLU
 * (models.py:149) applied where the tensor is produced instead of where it is consumed. */
NSG_API int nsg_bn_apply(const void *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                         const void *residual, void *y, int64_t M, int32_t C, int32_t relu, int32_t relu_residual,
                         int32_t dtype, int32_t y_dtype, void *stream);

/* Backward of the call above with respect to x, gamma, beta.  When the forward used relu & 1, the ReLU mask
 * comes from ONE of: relu_beta = the forward's beta [C] (the mask (x-mean)*(invstd*gamma)+beta > 0 is then
 * re-derived from x with the forward's own arithmetic and y_relu is not read -- one tensor less of traffic),
 * or y_relu = the forward OUTPUT (its sign is the mask).  Both NULL: no ReLU.  dgamma/dbeta [C] overwritten.
 * dx_colsum [C] or NULL: column sums of dx, i.e. the bias gradient of the convolution that feeds
 * this BatchNorm (autograd of nn.Conv2d's bias at src/models.py:150,153,165,179), produced by the
 * kernel that writes dx instead of a second pass over it. */
NSG_API int nsg_bn_backward(const void *x, const void *y_relu, const void *dy, const float *mean,
                            const float *invstd, const float *gamma, const float *relu_beta, void *dx, float *dgamma,
                            float *dbeta, float *dx_colsum, int64_t M, int32_t C, int32_t dtype, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The single-channel input layer with its BatchNorm, as one operator     src/models.py:165-167
 *   encoder.0 Conv2d(1, C, 4, 2, 1) -> encoder.1 BatchNorm2d(C) -> encoder.2 ReLU(True)
 * The convolution's output is 2C times larger than the image it comes from and costs 16 multiply-adds
 * per element, so it is never stored: the statistics pass, the apply pass and both backward passes
 * recompute it from the image (one tensor write forward, two tensor reads backward, against three
 * writes and eight reads of nsg_conv_forward + nsg_bn_stats + nsg_bn_apply + nsg_bn_backward +
 * nsg_conv_wgrad, whose results these reproduce: same value for h bit for bit, same expressions).
 *   img [B][H][W] fp32 (H, W even); w the parameter's own layout (C,1,4,4) = [C][16] fp32; bias [C] or NULL;
 *   y / dy [B][H/2][W/2][C] of y_dtype / dy_dtype (NSG_F32 or NSG_BF16); C % 4 == 0, C <= 1024.
 * ------------------------------------------------------------------------------------------- */
NSG_API size_t nsg_c1conv_bn_workspace_bytes(int32_t C);
/* training != 0: mean / invstd [C] are OUTPUTS (batch statistics of the conv output; running_mean / running_var
 * updated with `momentum` when not NULL, unbiased variance as nn.BatchNorm2d); training == 0: they are INPUTS
 * (nsg_bn_eval_stats) and the workspace is not used.  y = max(0, (h - mean) * (invstd * gamma) + beta). */
NSG_API int nsg_c1conv_bn_relu_forward(const float *img, const float *w, const float *bias, const float *gamma, const float *beta,
                                       float *mean, float *invstd, float *running_mean, float *running_var, float eps,
                                       float momentum, int32_t training, void *y, int32_t y_dtype, int32_t B, int32_t H,
                                       int32_t W, int32_t C, void *workspace, size_t workspace_bytes, double *moments,
                                       void *stream);
/* Gradients of the layer's parameters from dy = dL/dy (the image is data: no input gradient):
 * dw [C][16], dbias [C] or NULL, dgamma [C], dbeta [C], all overwritten; mean / invstd as the forward left them.
 * moments (both calls; NULL allowed): NSG_C1_MOMENTS doubles = the image's tap moments S[t] = sum_p x[p][t] and
 * P[t][u] = sum_p x[p][t] x[p][u] over the 16 patch values of every output pixel (stored for values shifted by a constant,
 * the last entry: conditioning).  The bf16 layer takes its batch statistics
 * and its weight gradient from them (one pass over dy instead of two).  The bf16 training forward (y_dtype NSG_BF16,
 * C = 32, 64, 96, 128 or 256: the widths of that path) writes them when the pointer is not NULL; the bf16 backward at those
 * widths reads them when given and recomputes them from the image otherwise.  Every other form takes neither from them: the
 * forward leaves the buffer as it was, the backward ignores it. */
NSG_API int nsg_c1conv_bn_relu_backward(const float *img, const float *w, const float *bias, const float *gamma,
                                        const float *beta, const float *mean, const float *invstd, const void *dy,
                                        int32_t dy_dtype, float *dw, float *dbias, float *dgamma, float *dbeta, int32_t B,
                                        int32_t H, int32_t W, int32_t C, void *workspace, size_t workspace_bytes,
                                        const double *moments, void *stream);
#define NSG_C1_MOMENTS 273

/* ---------------------------------------------------------------------------------------------
 * The single-channel OUTPUT layer with the BatchNorm in front of it, as one operator     src/models.py:180-183
 *   decoder.4 BatchNorm2d(C) -> decoder.5 ReLU(True) -> decoder.6 ConvTranspose2d(C, 1, 4, 2, 1) [-> decoder.7 Tanh]
 * u [B][H][W][C] is the BatchNorm INPUT (the transposed conv in front wrote it; its batch statistics come from
 * nsg_bn_stats).  Neither the activated tensor a = relu(bn(u)) nor the data gradient of the transposed conv is ever
 * stored: the forward applies BatchNorm + ReLU on the operand's way into the MFMA, the backward rebuilds the
 * data gradient from the gradient image (16 taps per element, on the matrix cores) inside the BatchNorm-backward
 * passes and the weight gradient from a rebuilt on the spot -- 4 tensor reads + 1 write against 8 reads + 3 writes
 * of nsg_bn_apply + nsg_conv_forward + nsg_conv_wgrad + nsg_conv_dgrad + nsg_bn_backward.
 * Available for bf16 tensors with C = 32, 64, 96, 128, 256 (nsg_bn_relu_c1convt_supported); other shapes use the
 * separate operators.  w: the parameter's own layout (C,1,4,4) = [C][16] fp32; y / dy: [B][2H][2W] fp32.
 * ------------------------------------------------------------------------------------------- */
NSG_API int32_t nsg_bn_relu_c1convt_supported(int32_t dtype, int32_t C);
NSG_API size_t nsg_bn_relu_c1convt_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
/* y = [tanh](bias + convT(relu((u - mean) * invstd * gamma + beta)));  flags: 0 or NSG_TANH_OUT */
NSG_API int nsg_bn_relu_c1convt_forward(const void *u, int32_t dtype, const float *mean, const float *invstd, const float *gamma,
                                        const float *beta, const float *w, const float *bias, float *y, int32_t flags, int32_t B,
                                        int32_t H, int32_t W, int32_t C, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the Tanh, plus the reconstruction loss of src/train.py:118-129 taken in the pass that writes the image:
 * target [B][2H][T] fp32 with T >= 2W (x_tilde is zero-padded on the right to the target's width, as the reference pads it on the
 * host); loss_out[0] = mean((pad(x_tilde) - target)^2); dpre [B][2H][2W] = grad_scale * 2 / (B 2H T) * (x_tilde - target) *
 * (1 - x_tilde^2) = the gradient w.r.t. the Tanh's INPUT (what nsg_bn_relu_c1convt_backward takes as dy); y = x_tilde is stored
 * only when not NULL; dbias [1] or NULL = sum of dpre, the transposed conv's bias gradient (pass dbias = NULL to the backward
 * then).  Replaces nsg_bn_relu_c1convt_forward + nsg_mse_padded + nsg_tanh_backward in a training step. */
NSG_API int nsg_bn_relu_c1convt_forward_mse(const void *u, int32_t dtype, const float *mean, const float *invstd, const float *gamma,
                                            const float *beta, const float *w, const float *bias, float *y, const float *target,
                                            int32_t T, float grad_scale, float *loss_out, float *dpre, float *dbias, int32_t B,
                                            int32_t H, int32_t W, int32_t C, void *workspace, size_t workspace_bytes, void *stream);
/* dy: gradient w.r.t. the transposed conv's output (BEFORE the tanh: nsg_tanh_backward).  Outputs: du (dtype, the
 * gradient w.r.t. u), du_colsum [C] or NULL (column sums of du = the bias gradient of the conv that wrote u, as
 * nsg_bn_backward's dx_colsum), dw [C][16], dbias [1] or NULL, dgamma [C], dbeta [C], all overwritten. */
NSG_API int nsg_bn_relu_c1convt_backward(const void *u, int32_t dtype, const float *mean, const float *invstd, const float *gamma,
                                         const float *beta, const float *w, const float *dy, void *du, float *du_colsum, float *dw,
                                         float *dbias, float *dgamma, float *dbeta, int32_t B, int32_t H, int32_t W, int32_t C,
                                         void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The ResBlock's 1x1 convolution with the BatchNorm work around it folded in     src/models.py:151-155
 *   ... BatchNorm2d(dim) -> ReLU(True) -> Conv2d(dim, dim, 1) -> BatchNorm2d(dim)
 * A 1x1 conv over NHWC rows is a flat GEMM [M][C] x [C][C]: a stream kernel.  These entry points apply the
 * BatchNorm arithmetic of the neighbouring layers on the operand's way from the global-load registers into LDS,
 * so the activated tensor relu(bn(x)) is never stored and the second BatchNorm's input gradient is produced and
 * consumed in one pass.  bf16 tensors, C = 32, 64, 128, 256 (nsg_bn_relu_conv1x1_supported); w: (C, C, 1, 1) fp32.
 * ------------------------------------------------------------------------------------------- */
NSG_API int32_t nsg_bn_relu_conv1x1_supported(int32_t dtype, int32_t C);
NSG_API size_t nsg_bn_relu_conv1x1_workspace_bytes(int64_t M, int32_t C);
/* y = relu((x - mean) * invstd * gamma + beta) * w^T + bias          (replaces nsg_bn_apply + nsg_conv_forward) */
NSG_API int nsg_bn_relu_conv1x1_forward(const void *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                                        const float *w, const float *bias, void *y, int64_t M, int32_t C, int32_t dtype,
                                        void *workspace, size_t workspace_bytes, void *stream);
/* The same, plus the batch statistics of y taken from the store phase (what nsg_bn_stats(y) computes, for the BatchNorm
 * that follows): mean_y / invstd_y [C] out, running statistics updated with `momentum` when not NULL. */
NSG_API int nsg_bn_relu_conv1x1_forward_bnstats(const void *x, const float *mean, const float *invstd, const float *gamma,
                                                const float *beta, const float *w, const float *bias, void *y, float eps,
                                                float momentum, float *mean_y, float *invstd_y, float *running_mean_y,
                                                float *running_var_y, int64_t M, int32_t C, int32_t dtype, void *workspace,
                                                size_t workspace_bytes, void *stream);
/* dw[o][i] = sum_m dy[m][o] * relu(bn(x))[m][i]                        (nsg_conv_wgrad with the activation rebuilt from x) */
NSG_API int nsg_bn_relu_conv1x1_wgrad(const void *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                                      const void *dy, float *dw, int64_t M, int32_t C, int32_t dtype, void *workspace,
                                      size_t workspace_bytes, void *stream);
/* The apply half of nsg_bn_backward (no ReLU; dgamma / dbeta from nsg_bn_backward_sums) fused with the data gradient of
 * the 1x1 conv in FRONT of that BatchNorm:  dh = bn-backward(dy) at input h (stored: the weight gradient needs it),
 * dx = dh * w, dh_colsum [C] or NULL = column sums of dh (the conv's bias gradient).
 * prev_x != NULL: the conv's input was relu(bn_prev(prev_x)); the sums of THAT BatchNorm's backward over (prev_x, dx) --
 * what nsg_bn_backward_sums(prev_x, dx, ..., relu_beta = prev_beta) computes -- are formed while dx is written:
 * prev_dgamma / prev_dbeta [C] out (then nsg_bn_backward_apply finishes that BatchNorm without a reduction pass). */
NSG_API int nsg_bn_backward_conv1x1_dgrad(const void *h, const void *dy, const float *mean, const float *invstd, const float *gamma,
                                          const float *dgamma, const float *dbeta, const float *w, void *dh, void *dx,
                                          float *dh_colsum, const void *prev_x, const float *prev_mean, const float *prev_invstd,
                                          const float *prev_gamma, const float *prev_beta, float *prev_dgamma, float *prev_dbeta,
                                          int64_t M, int32_t C, int32_t dtype, void *workspace, size_t workspace_bytes, void *stream);
/* nsg_bn_backward_conv1x1_dgrad + nsg_bn_relu_conv1x1_wgrad in ONE pass over the tensors (bf16, C = 128; the BatchNorm in front is
 * required): dx, dh_colsum (or NULL), prev_dgamma / prev_dbeta as above, and dw[o][i] = sum_m dh[m][o] * relu(bn_prev(prev_x))[m][i]
 * (the autograd of src/models.py:153 for the conv weight).  dh is never stored.  4 tensor passes instead of 7. */
NSG_API int32_t nsg_bn_backward_conv1x1_dgrad_wgrad_supported(int32_t dtype, int32_t C);
NSG_API size_t nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes(int64_t M, int32_t C);
NSG_API int nsg_bn_backward_conv1x1_dgrad_wgrad(const void *h, const void *dy, const float *mean, const float *invstd, const float *gamma,
                                                const float *dgamma, const float *dbeta, const float *w, void *dx, float *dw,
                                                float *dh_colsum, const void *prev_x, const float *prev_mean, const float *prev_invstd,
                                                const float *prev_gamma, const float *prev_beta, float *prev_dgamma, float *prev_dbeta,
                                                int64_t M, int32_t C, int32_t dtype, void *workspace, size_t workspace_bytes,
                                                void *stream);
/* The apply half of nsg_bn_backward alone: dgamma / dbeta are inputs. */
NSG_API int nsg_bn_backward_apply(const void *x, const void *y_relu, const void *dy, const float *mean, const float *invstd,
                                  const float *gamma, const float *relu_beta, const float *dgamma, const float *dbeta, void *dx,
                                  float *dx_colsum, int64_t M, int32_t C, int32_t dtype, void *workspace, size_t workspace_bytes,
                                  void *stream);
/* The reduction half of nsg_bn_backward alone (same arguments, same values): dgamma, dbeta. */
NSG_API int nsg_bn_backward_sums(const void *x, const void *y_relu, const void *dy, const float *mean, const float *invstd,
                                 const float *gamma, const float *relu_beta, float *dgamma, float *dbeta, int64_t M, int32_t C,
                                 int32_t dtype, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Element-wise, losses, optimiser                         src/train.py:118-136
 * ------------------------------------------------------------------------------------------- */

/* dx = (a + b) * (x > 0)   (b may be NULL): gradient through the ResBlock's leading in-place ReLU.
 * All four tensors hold elements of `dtype`. */
NSG_API int nsg_relu_backward_add(const void *a, const void *b, const void *x, void *dx, int64_t n, int32_t dtype,
                                  void *stream);

/* dst = src (relu != 0: max(0, src)) with a change of storage type (fp32 <-> bf16, round to nearest even). */
NSG_API int nsg_convert(const void *src, int32_t src_dtype, void *dst, int32_t dst_dtype, int64_t n, int32_t relu,
                        void *stream);

/* dx = g * (1 - y*y): backward of nn.Tanh (models.py:183) from its output y. */
NSG_API int nsg_tanh_backward(const float *g, const float *y, float *dx, int64_t n, void *stream);

/* *counters[i] += 1 for i < n: the `num_batches_tracked += 1` of every nn.BatchNorm2d a training-mode forward passes
 * (src/models.py:151,154,166,180) as one launch per 32 counters.  `counters` is a HOST array of device pointers. */
NSG_API int nsg_increment_counters(int64_t *const *counters, int32_t n, void *stream);

/* y = a + b (b may be NULL -> copy). */
NSG_API int nsg_add(const float *a, const float *b, float *y, int64_t n, void *stream);

/* Speaker-conditioned decoder (extension; BASELINE configs[2]; not in the reference, whose VQVAE
 * ignores the speaker id g, src/train.py:114):  y[b][r][:] = x[b][r][:] + rows[b][:] for the
 * rows_per_clip pixels r of clip b, and its gradient w.r.t. rows: out[b][:] = sum_r x[b][r][:]. */
NSG_API int nsg_add_per_clip(const float *x, const float *rows, void *y, int32_t B, int64_t rows_per_clip, int32_t C,
                             int32_t y_dtype, void *stream);
NSG_API size_t nsg_clip_colsum_workspace_bytes(int32_t B, int32_t C);
NSG_API int nsg_clip_colsum(const void *x, int32_t dtype, int32_t B, int64_t rows_per_clip, int32_t C, float *out,
                            void *workspace, size_t workspace_bytes, void *stream);

NSG_API size_t nsg_reduce_workspace_bytes(int64_t n);

/* loss_out[0] = mean over rows*wc elements of (pad(a) - c)^2 where a is [rows][wa], c is [rows][wc],
 * wa <= wc and a is zero-padded on the right to wc: the reference's zero-pad + F.mse_loss
 * (src/train.py:118-129).  da (or NULL) receives grad_scale * 2/(rows*wc) * (a - c[:, :wa]). */
NSG_API int nsg_mse_padded(const float *a, const float *c, int64_t rows, int32_t wa, int32_t wc, float grad_scale,
                           float *loss_out, float *da, void *workspace, size_t workspace_bytes, void *stream);

/* loss_out[0] = mean((q - z)^2) over n elements (train.py:131,133: both terms have this value);
 * dz (or NULL) = dz_scale * 2/n * (z - q) (+ dz_add if non-NULL: the straight-through gradient),
 * dq (or NULL) = dq_scale * 2/n * (q - z).  z, q, dq are fp32 (the quantiser works in fp32 in both
 * modes); dz and dz_add hold elements of grad_dtype (the encoder-side activation gradient). */
NSG_API int nsg_vq_losses(const float *z, const float *q, int64_t n, float dz_scale, float dq_scale,
                          const void *dz_add, float *loss_out, void *dz, float *dq, int32_t grad_dtype,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The same loss and encoder-side gradient with q given by (codebook [K][D], idx [N]): q[r] = codebook[idx[r]] is read from
 * the cache-resident codebook instead of a materialised tensor (D % 8 == 0).  The codebook-side gradient of the loss is
 * 2/n * (n_k e_k - sum of the rows assigned to k): nsg_index_add_rows over z with counts (train.py:131). */
NSG_API int nsg_vq_losses_indexed(const float *z, const float *codebook, const int64_t *idx, int64_t N, int32_t D, int32_t K,
                                  float dz_scale, const void *dz_add, float *loss_out, void *dz, int32_t grad_dtype,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The same when dz is the incoming gradient of a BatchNorm whose input is bn_x [N][D] of grad_dtype (the encoder's last
 * ResBlock ends in one, src/models.py:154): that BatchNorm's backward sums over the dz values as stored -- bn_dbeta[d] = sum_n
 * dz[n][d], bn_dgamma[d] = sum_n dz[n][d] * (bn_x[n][d] - bn_mean[d]) * bn_invstd[d], what nsg_bn_backward_sums(bn_x, dz)
 * returns, bit for bit when grad_dtype is NSG_BF16 (the same slabs, the same order) -- are formed while dz is written, instead of
 * a pass that reads dz and bn_x back.  D: a multiple of 8 up to 2048 (nsg_vq_losses_indexed_bn_supported); dz must not be NULL. */
NSG_API int32_t nsg_vq_losses_indexed_bn_supported(int32_t D);
NSG_API size_t nsg_vq_losses_indexed_bn_workspace_bytes(int64_t N, int32_t D);
NSG_API int nsg_vq_losses_indexed_bn(const float *z, const float *codebook, const int64_t *idx, int64_t N, int32_t D, int32_t K,
                                     float dz_scale, const void *dz_add, float *loss_out, void *dz, int32_t grad_dtype,
                                     const void *bn_x, const float *bn_mean, const float *bn_invstd, float *bn_dgamma,
                                     float *bn_dbeta, void *workspace, size_t workspace_bytes, void *stream);
/* nsg_vq_losses_indexed_bn with z given as its sources (see nsg_vq_forward_bf16x3_bnres): z IS the output of that BatchNorm plus
 * the skip connection, so bn_x = h (read once for both uses), bn_mean = mean, bn_invstd = invstd.  bf16 gradients (dz, dz_add);
 * D a multiple of 8 up to 1024; workspace nsg_vq_losses_indexed_bn_workspace_bytes. */
NSG_API int nsg_vq_losses_indexed_bnres(const void *h, const void *r, const float *mean, const float *invstd, const float *gamma,
                                        const float *beta, const float *codebook, const int64_t *idx, int64_t N, int32_t D, int32_t K,
                                        float dz_scale, const void *dz_add, float *loss_out, void *dz, float *bn_dgamma,
                                        float *bn_dbeta, void *workspace, size_t workspace_bytes, void *stream);

/* torch.optim.Adam step (src/main.py:124 defaults, no weight decay, no amsgrad) over one flat
 * fp32 buffer.  g is multiplied by grad_scale first (1/world_size after a sum all-reduce).
 * step is the 1-based step count. */
NSG_API int nsg_adam_step(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2,
                          float eps, int32_t step, float grad_scale, void *stream);

/* sumsq[0] = sum of g[i]^2 over n floats, accumulated in DOUBLE ((double)g * (double)g is exact) and left on the device.
 * The partition of elements to threads and blocks depends only on n and on whether g is 16-byte aligned, and every combine
 * is in a fixed order: two calls on the same input give the same bits.  n == 0 writes 0.  workspace:
 * nsg_grad_sumsq_workspace_bytes(n) bytes; sumsq and workspace 8-byte aligned. */
NSG_API size_t nsg_grad_sumsq_workspace_bytes(int64_t n);
NSG_API int nsg_grad_sumsq(const float *g, int64_t n, double *sumsq, void *workspace, size_t workspace_bytes, void *stream);

/* nsg_adam_step extended; each extension has a neutral value, and with all of them neutral (seg_end = seg_wd = sumsq =
 * shadow = NULL, n_seg = 0, max_norm <= 0, skip_nonfinite = 0) p, m and v come out as nsg_adam_step's, bit for bit.
 *   - clipping (sumsq = the device double nsg_grad_sumsq wrote, max_norm > 0):  norm = grad_scale * sqrt(sumsq[0]) formed in
 *     double and rounded to fp32 once, coef = min(1, max_norm / (norm + 1e-6)) as torch.nn.utils.clip_grad_norm_; the gradient
 *     used is (g * grad_scale) * coef, held as the exact double product where coef < 1 (g c - m and (g c)^2 (1 - beta2) round
 *     once each; coef == 1 leaves nsg_adam_step's bits).  Every thread forms coef from the same double the same way;
 *   - skip_nonfinite != 0: when that fp32 norm is not finite, p, m, v and shadow are not written at all;
 *   - decoupled weight decay (torch.optim.AdamW): seg_end [n_seg] int64 ascending element offsets and seg_wd [n_seg] floats, in
 *     device memory: element e belongs to the first segment s with seg_end[s] > e (none: no decay) and p <- p - p * (lr * wd_s)
 *     before the Adam update.  Segments end on multiples of 4 elements (a 16-byte group takes its first element's segment);
 *   - weight EMA (shadow [n], one_minus_decay = float(1 - decay)): shadow <- shadow - one_minus_decay * (shadow - p_new),
 *     three fp32 roundings; one_minus_decay == 1 copies p_new;
 *   - stats (or NULL; 16 bytes, 4-byte aligned): float norm (-1 without sumsq), float coef, int32 finite, int32 running count
 *     of skipped steps (+= 1 when this call skipped; the caller zeroes it once).  One thread writes it with ordinary stores.
 * NSG_E_INVALID: a null p / g / m / v, n < 0, step < 1, half a segment table or n_seg not matching it, max_norm > 0 or the
 * guard without sumsq, a NaN max_norm, |one_minus_decay| > 1 (or NaN), a shadow overlapping p, a misaligned sumsq / stats. */
NSG_API int nsg_adamw_step(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps,
                           int32_t step, float grad_scale, const int64_t *seg_end, const float *seg_wd, int32_t n_seg,
                           const double *sumsq, float max_norm, int32_t skip_nonfinite, float *shadow, float one_minus_decay,
                           void *stats, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian latent of the continuous VAE                   src/models.py:77,103-112
 *   encoder.9 Conv2d -> encoder.10 BatchNorm2d(2Z) -> chunk(2, dim=1) -> KL to N(0, I) -> mu + exp(.5 logvar) * eps
 * Rows are the NHWC pixels of the encoder output, 2Z channels per row: [0, Z) is mu, [Z, 2Z) is logvar.  h [M][2Z] is the
 * BatchNorm's INPUT; its output y = (h - mean) * (invstd * gamma) + beta (nsg_bn_apply's arithmetic) is formed on load by
 * both kernels and never stored.  mean / invstd: nsg_conv_forward_bnstats (training) or nsg_bn_eval_stats (eval).
 * The kernels hold no random-number generator: eps [M][Z] is an argument.  fp32; no clamping: non-finite values propagate.
 * NSG_E_INVALID: a null required pointer, M < 1, tensors not 16-byte aligned; NSG_E_UNSUPPORTED: Z < 4, Z % 4 != 0, Z > 512,
 * M * 2Z >= 2^31; NSG_E_WORKSPACE: fewer than nsg_vae_latent_workspace_bytes(M, Z) bytes.  Every sum is in a fixed order.
 * ------------------------------------------------------------------------------------------- */
NSG_API size_t nsg_vae_latent_workspace_bytes(int64_t M, int32_t Z);
/* sigma = expf(0.5 lv);  z [M][Z] = mu + sigma * eps;  kl_out[0] = (1 / M) * sum over rows and channels of
 * 0.5 * (mu^2 + sigma^2 - 1 - lv): kl_divergence(Normal(mu, sigma), Normal(0, 1)).sum(1).mean() of models.py:108-110. */
NSG_API int nsg_vae_latent_forward(const float *h, const float *mean, const float *invstd, const float *gamma, const float *beta,
                                   const float *eps, float *z, float *kl_out, int64_t M, int32_t Z, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* dy [M][2Z] = the gradient w.r.t. the BatchNorm's OUTPUT, given dz [M][Z] = dL/dz and the KL term's weight
 * s = kl_scale * (kl_grad ? kl_grad[0] : 1) / M (kl_grad: one device float, the gradient arriving at kl_out, or NULL):
 *   dy_mu = dz + s * mu,   dy_lv = 0.5 * dz * sigma * eps + 0.5 * s * (sigma^2 - 1);
 * and that BatchNorm's backward sums over the dy values as stored, dbeta[c] = sum_m dy[m][c], dgamma[c] = sum_m dy[m][c] *
 * (h[m][c] - mean[c]) * invstd[c] ([2Z] each, overwritten): what nsg_bn_backward_sums(h, NULL, dy, ...) returns, bit for bit
 * (the same slabs, the same order), so nsg_bn_backward_apply(h, NULL, dy, ..., dgamma, dbeta, dh, ...) finishes dh. */
NSG_API int nsg_vae_latent_backward(const float *h, const float *mean, const float *invstd, const float *gamma, const float *beta,
                                    const float *eps, const float *dz, float kl_scale, const float *kl_grad, float *dy,
                                    float *dgamma, float *dbeta, int64_t M, int32_t Z, void *workspace, size_t workspace_bytes,
                                    void *stream);

/* ---------------------------------------------------------------------------------------------
 * Self-checks used by the tests
 * ------------------------------------------------------------------------------------------- */

/* out[i*K+k] = x[i]·e[k] evaluated (mode 0) as a sequential fmaf chain on the vector ALU and
 * (mode 1) on v_mfma_f32_32x32x2_f32 in the order nsg_vq_forward uses; the two must agree bit for
 * bit for the argmin to be exact.  N, K multiples of 32, D <= 256. */
NSG_API int nsg_debug_dot(const float *x, const float *e, int32_t N, int32_t D, int32_t K, int32_t mode, float *out,
                          void *stream);

/* nsg_vq_forward with the contraction on the vector ALU (an explicit fmaf chain per (row, code)) instead of the matrix
 * cores: same arguments, same results bit for bit -- the cross-check that the MFMA form keeps the reference's
 * summation order (src/vector_quantization.py:12-19).  Slow; tests only. */
NSG_API int nsg_debug_vq_forward_valu(const float *x, const float *e, int64_t N, int32_t D, int32_t K, int64_t *idx_out,
                                      float *codes_out, float *dmin_out, void *workspace, size_t workspace_bytes,
                                      void *stream);

/* ---------------------------------------------------------------------------------------------
 * Latent prior (GatedPixelCNN over the code-index grid)              src/models.py:219-341
 * Its convolutions are nsg_conv_* calls (rectangular masked kernels embedded in square ones);
 * these are the element-wise pieces.  fp32, rows [M][channels].
 * ------------------------------------------------------------------------------------------- */

/* GatedActivation with the class-conditional add folded in (models.py:219-226,268,274):
 *   y[m][c] = tanh(x[m][c] + cond[b][c]) * sigmoid(x[m][C+c] + cond[b][C+c]),  b = m / rows_per_clip.
 * x [M][2C], cond [B][2C] or NULL, y [M][C].  C % 4 == 0. */
NSG_API int nsg_gated_activation_forward(const float *x, const float *cond, float *y, int64_t M, int32_t C,
                                         int64_t rows_per_clip, void *stream);
/* dx [M][2C] given dy [M][C] (the gradient w.r.t. cond is the per-clip column sum of dx: nsg_clip_colsum). */
NSG_API int nsg_gated_activation_backward(const float *x, const float *cond, const float *dy, float *dx, int64_t M,
                                          int32_t C, int64_t rows_per_clip, void *stream);

/* F.cross_entropy(logits, target) with mean reduction on rows [M][K] (target int64 [M]):
 * loss_out[0] = mean_m( logsumexp(logits[m]) - logits[m][target[m]] ); dlogits (or NULL) = grad_scale * d loss / d logits. */
NSG_API size_t nsg_cross_entropy_workspace_bytes(int64_t M);
NSG_API int nsg_cross_entropy(const float *logits, const int64_t *target, int64_t M, int32_t K, float grad_scale,
                              float *loss_out, float *dlogits, void *workspace, size_t workspace_bytes, void *stream);

/* The training step's forms of the gate (prior_train.py).
 *
 * Gate of a sum: y = gate((a + b) + cond) for two summands a, b [M][2C], the fp32 additions in exactly that order, so that y
 * equals nsg_add(a, b) followed by nsg_gated_activation_forward bit for bit while the [M][2C] sum is never stored.  The
 * backward writes the one dx [M][2C] that both summands share (d/da = d/db = d/d(a + b)), equal bit for bit to
 * nsg_gated_activation_backward on the materialised sum.
 *
 * Column sums: with dcond != NULL the backward also writes dcond [B][2C], B = M / rows_per_clip: dcond[b][c] = sum over the
 * rows of clip b of dx[m][c], the gradient of cond (what nsg_clip_colsum(dx) returns, up to the rounding of another summation
 * order), formed while dx is written.  Deterministic: every thread sums its rows in double in a fixed order, the threads of a
 * block and then the blocks of a clip are added in a fixed order, no atomics.  M must be a whole number of clips, C <= 1024;
 * the workspace (nsg_gated_colsum_workspace_bytes, 16-byte aligned) is needed only with dcond.  cond may be NULL with dcond set
 * (rows_per_clip still says where the clips end).  nsg_gated_activation_backward_colsum is the plain gate's backward with the
 * column sums (dcond required); nsg_gated_activation_backward stays as it is.
 * All pointers 16-byte aligned, C % 4 == 0. */
NSG_API int nsg_gated_activation_sum_forward(const float *a, const float *b, const float *cond, float *y, int64_t M,
                                             int32_t C, int64_t rows_per_clip, void *stream);
NSG_API size_t nsg_gated_colsum_workspace_bytes(int64_t M, int32_t C, int64_t rows_per_clip);
NSG_API int nsg_gated_activation_sum_backward(const float *a, const float *b, const float *cond, const float *dy, float *dx,
                                              float *dcond, int64_t M, int32_t C, int64_t rows_per_clip, void *workspace,
                                              size_t workspace_bytes, void *stream);
NSG_API int nsg_gated_activation_backward_colsum(const float *x, const float *cond, const float *dy, float *dx, float *dcond,
                                                 int64_t M, int32_t C, int64_t rows_per_clip, void *workspace,
                                                 size_t workspace_bytes, void *stream);

/* nsg_cross_entropy over the valid rows only, with per-clip sums: rows [M][K], M = B * rows_per_clip, row m belongs to clip
 * m / rows_per_clip.  A row whose target is NEGATIVE is ignored (the padded positions of a zero-padded batch).  A target >= K
 * violates the precondition; such a row is treated as ignored too, never read out of range.  With row_loss[m] the loss of a
 * valid row (the formula of nsg_cross_entropy) and n_valid the number of valid rows, counted on the device:
 *   loss_out[0]   = (sum of row_loss over the valid rows) / n_valid;
 *   dlogits       = (softmax - onehot) * grad_scale / n_valid on valid rows, exact zeros on ignored rows   (or NULL);
 *   clip_nll[b]   = sum of row_loss over the valid rows of clip b, fp32                                    (or NULL);
 *   clip_count[b] = number of valid rows of clip b, int64                                                  (or NULL).
 * n_valid == 0 gives loss 0 and an all-zero gradient.  (F.cross_entropy with ignore_index returns NaN there; a training loop
 * has to survive a batch whose clips are all too short, so this does not.)  Nothing synchronises with the host.
 * Deterministic, fixed-order reductions; clip_nll[b] is formed from clip b's own rows only, so it does not depend on the other
 * clips of the batch.  With nothing ignored, loss_out and dlogits equal nsg_cross_entropy's bit for bit (the same row kernel,
 * the same summation order, the same 1 / M).  The workspace must be 16-byte aligned. */
NSG_API size_t nsg_cross_entropy_masked_workspace_bytes(int64_t M, int64_t rows_per_clip);
NSG_API int nsg_cross_entropy_masked(const float *logits, const int64_t *target, int64_t M, int32_t K, int64_t rows_per_clip,
                                     float grad_scale, float *loss_out, float *dlogits, float *clip_nll, int64_t *clip_count,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* Incremental sampling (GatedPixelCNN.sample in prior.py): the per-row column walk.  For row `row` and each clip b it walks
 * j = 0 .. W-1 and, per layer l, forms
 *     out = gate((vh[l][b][j] + horiz_l(columns j-3 .. j-1 of e for l = 0, columns j-1 and j of h_l otherwise)) + cond[l][b]),
 *     h_{l+1} = resid_l(out) (+ h_l for l >= 1),
 * then the head  logits = W2 relu(W0 h_L + b0) + b2,  then the code of (b, row, j):
 *   - teacher-forced (x_in != NULL, u == NULL): x_in[b][row][j];
 *   - sampling (u != NULL, x_in == NULL): the inverse CDF of softmax(logits) against u[b][row][j] in [0, 1):
 *     p_k = exp(l_k - max l) in fp32, S = sum_k p_k; the first k with p_k > 0 whose inclusive prefix sum exceeds u * S, or,
 *     if rounding leaves none, the last k with p_k > 0.  A code with p_k == 0 is never returned.  (The prefix sums and S
 *     come from one fixed-order scan: contiguous chunks of ceil(K / 64) codes, chunk totals scanned in chunk order, each
 *     chunk's prefix sums continuing from the scan of the chunks before it.)
 * The code goes to codes[b][row][j] (if codes != NULL) and embedding[code] to e_row + b * e_clip_stride + j * dim.
 * logits (optional) [B][H][W][K] receives the row's logits.
 * Inputs of the row, produced beforehand by the row pass on the conv kernels: vh [L][B][W][2 dim] = v2h_l(h_vert_l) of the
 * row (bias included), cond [L][B][2 dim] = the class-embedding rows.  emb [K][dim] is the code embedding.
 * w: the packed weight blob, fp32, nsg_prior_walk_weight_floats(dim, n_layers, input_dim) floats, Kp = input_dim rounded up
 * to a multiple of 4, every matrix transposed to [k][n] (input-major):
 *   layer 0:      horiz [3 dim][2 dim] (taps 0, 1, 2 of horiz_stack: row t * dim + c_in), horiz bias [2 dim],
 *                 resid [dim][dim], resid bias [dim];
 *   layer l >= 1: horiz [2 dim][2 dim] (taps 0, 1), horiz bias [2 dim], resid [dim][dim], resid bias [dim];
 *   head:         W0 [dim][512], b0 [512], W2 [512][Kp] (columns >= input_dim zero), b2 [Kp].
 * Envelope: dim % 16 == 0, dim <= 128, n_layers >= 1, input_dim <= 1024 (and the LDS of a 4-clip slice within 160 KiB);
 * outside it the size query returns 0 and the walk NSG_E_UNSUPPORTED.  One workgroup per 4 clips; no workgroup waits on
 * another; deterministic, and a clip's arithmetic does not depend on the other clips of the batch. */
NSG_API size_t nsg_prior_walk_weight_floats(int32_t dim, int32_t n_layers, int32_t input_dim);
NSG_API int nsg_prior_walk(const float *w, const float *emb, const float *cond, const float *vh, const float *u, const int64_t *x_in,
                           int64_t *codes, float *e_row, int64_t e_clip_stride, float *logits, int32_t B, int32_t H, int32_t W,
                           int32_t dim, int32_t n_layers, int32_t input_dim, int32_t row, void *stream);

/* The same walk with a controlled pick: temperature, top-k and top-p truncation, and kept (primed) codes.  u and codes are
 * required; x_in and keep ([B][H][W], one byte per position) are given together or both NULL.  The rule, for one position
 * with fp32 logits l_k (k < K), mx = max l, temperature T > 0, top_k >= 0 (0 = off) and 0 < top_p <= 1 (1 = off):
 *   1. p_k = expf((l_k - mx) * inv_t) with inv_t = 1.0f / T computed once in fp32 by the launcher (T == 1: the product is
 *      exact and p_k has nsg_prior_walk's bits).  The live codes are those with p_k > 0.
 *   2. top-k, if 1 <= top_k < the number of live codes: t = the top_k-th largest LOGIT of the live codes, counted with
 *      multiplicity, and A = {k live : l_k >= t} (codes tied at t are all kept); otherwise A = the live codes.
 *   3. top-p, if top_p < 1: S_A = sum_{k in A} p_k; v = the largest value among {p_k : k in A} with
 *      sum_{k in A, p_k >= v} p_k >= top_p * S_A; N = {k in A : p_k >= v} -- the smallest set of most probable codes that
 *      reaches the mass, ties kept (if rounding left no such v, N = A).  With top_p == 1 the step is skipped, N = A.
 *   4. the pick is nsg_prior_walk's over N in index order: the first k in N whose inclusive prefix sum over N exceeds
 *      u * S_N, or else the last k in N.  A code outside N is never returned.
 *   5. where keep[b][row][j] != 0 the code is x_in[b][row][j] (clamped to [0, input_dim)) and u is not consulted.
 * Every sum is in a fixed order that depends only on K (the scan of step 4 is nsg_prior_walk's; the masses of step 3 add each
 * chunk of ceil(K / 64) codes in index order, then the 64 chunk totals in a fixed tree).  With T == 1, top_k == 0, top_p == 1
 * and nothing kept the codes are nsg_prior_walk's, bit for bit.  Kept codes are not conditioned on by the positions before
 * them in raster order: each sampled code is drawn from the conditional given everything BEFORE it, kept or sampled.
 * Same envelope, alignment and extent checks as nsg_prior_walk; NSG_E_INVALID for a temperature that is not finite and > 0
 * (or whose fp32 reciprocal is not finite), top_k < 0, or top_p outside (0, 1]. */
NSG_API int nsg_prior_walk_ctl(const float *w, const float *emb, const float *cond, const float *vh, const float *u,
                               const int64_t *x_in, const uint8_t *keep, int64_t *codes, float *e_row, int64_t e_clip_stride,
                               float *logits, int32_t B, int32_t H, int32_t W, int32_t dim, int32_t n_layers, int32_t input_dim,
                               int32_t row, float temperature, int32_t top_k, float top_p, void *stream);

/* The controlled walk under classifier-free guidance.  B is the number of clips and is even: clips 2p and 2p + 1 are pair p,
 * the conditional branch (its cond and vh rows come from the real label) and the unconditional branch (from the null label).
 * u, x_in, keep and codes are indexed by pair, [B / 2][H][W]; cond, vh and e_row stay per clip (the next row pass needs both
 * branches' embeddings); logits (optional) stays [B][H][W][K] and receives each branch's RAW logits, before they are combined.
 * Per position, with the head's fp32 logits l_c (clip 2p) and l_u (clip 2p + 1) and guidance g:
 *     l_k = l_c,k + g * (l_c,k - l_u,k)        three separately rounded fp32 operations: subtract, multiply, add (never fused),
 * then steps 1-5 of nsg_prior_walk_ctl's rule run on l.  The chosen code goes to codes[p][row][j], and its embedding to the
 * e_row of BOTH clips of the pair: the branches walk the same codes.  With g == 0, or where l_c == l_u, l is l_c and the pair's
 * codes are those nsg_prior_walk_ctl gives clip 2p under the same u, bit for bit.
 * One workgroup per 4 clips = 2 pairs (a trailing one serves one pair); a pair never straddles workgroups.  The partition of
 * the work and every summation order are nsg_prior_walk's: a pair's arithmetic does not depend on the other pairs of the batch,
 * and each branch's logits are those the teacher-forced walk computes for that clip on the chosen codes.
 * Same envelope, alignment and extent checks as nsg_prior_walk_ctl and the same refusals; in addition NSG_E_INVALID for an odd
 * B and for a guidance that is not finite, < 0 or > 1024.  (The cap keeps l finite: |l| <= 1025 |l_c| + 1024 |l_u|, below FLT_MAX
 * for every pair of logits under FLT_MAX / 2049 ~ 1.6e35 in magnitude, which any head with finite weights of ordinary size
 * produces.) */
NSG_API int nsg_prior_walk_cfg(const float *w, const float *emb, const float *cond, const float *vh, const float *u,
                               const int64_t *x_in, const uint8_t *keep, int64_t *codes, float *e_row, int64_t e_clip_stride,
                               float *logits, int32_t B, int32_t H, int32_t W, int32_t dim, int32_t n_layers, int32_t input_dim,
                               int32_t row, float temperature, int32_t top_k, float top_p, float guidance, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mel -> waveform inversion (the epoch loop's audio export)   src/main.py:164-197, src/audio_tacotron.py:99-116,142-153
 * librosa's stft / istft / filters.mel and scipy's lfilter restated; fp32; frame-major spectrograms [B][T][F], F = n_fft/2+1.
 * ------------------------------------------------------------------------------------------- */

/* S[b][t][f] = max(1e-10, sum_m inv_basis[f][m] * 10^((clip(mel[b][m][t],0,max_abs)*(-min_db)/max_abs + min_db + ref_db)/20))^power
 * (audio_tacotron.py:242-248 _denormalize, :223 _db_to_amp, :202-206 _mel_to_linear, :115 S ** power).  mel [B][n_mels][T]. */
NSG_API int nsg_audio_mel_to_linear(const float *mel, const float *inv_basis, float *S, int32_t B, int32_t n_mels, int32_t T,
                                    int32_t F, float min_level_db, float ref_level_db, float max_abs_value, float power,
                                    void *stream);

/* Griffin-Lim (audio_tacotron.py:142-153): y [B][hop*(T-1)] from magnitudes S [B][T][F]; u [B][T][F] are the uniform
 * [0,1) numbers behind the random initial phases exp(2 pi i u).  n_fft in {512, 1024, 2048}, hop divides n_fft, T >= 2 and
 * hop*(T-1) >= 2: every such grid is reflect-padded as np.pad(mode="reflect") does, however short it is against n_fft/2. */
NSG_API size_t nsg_audio_griffin_lim_workspace_bytes(int32_t B, int32_t T, int32_t n_fft);
NSG_API int nsg_audio_griffin_lim(const float *S, const float *u, float *y, int32_t B, int32_t T, int32_t n_fft, int32_t hop,
                                  int32_t iters, void *workspace, size_t workspace_bytes, void *stream);

/* Griffin-Lim with momentum ("fast Griffin-Lim", Perraudin, Balazs, Sondergaard 2013; librosa.griffinlim's default since 0.7), an
 * extension: the reference iterates without it.  Layouts, envelope and refusals are nsg_audio_griffin_lim's.  With X_0 = 0 and
 * y_0 = istft(S exp(2 pi i u)), for i = 1 .. iters:
 *     X_i = stft(y_{i-1})
 *     t_i = X_i + momentum (X_i - X_{i-1})            per component, fp32
 *     y_i = istft(S t_i / |t_i|)                      t_i = 0: phase 0, i.e. (S, 0), as np.angle(0) = 0
 * and y = y_iters (librosa's angles = rebuilt - momentum / (1 + momentum) tprev up to a positive factor; t_1 = (1 + momentum) X_1
 * has the phase of X_1).  c [B][T][F] complex (interleaved re, im), caller-owned, is the state X_{i-1}: its content on entry is
 * never read (the first iteration uses X_0 = 0 without loading it, so it may hold NaN); with iters >= 1 it holds X_iters on
 * return, with iters == 0 it is not written.  Each (frame, bin) of c is read and rewritten by the one thread that owns it.
 * momentum == 0: c may be NULL and is not touched, and y is nsg_audio_griffin_lim's bit for bit (the same kernels).
 * workspace: nsg_audio_griffin_lim_workspace_bytes(B, T, n_fft) bytes, the same two sections (the extra spectrum is the argument c).
 * NSG_E_INVALID, before any launch: as nsg_audio_griffin_lim, momentum outside [0, 1] or NaN, c NULL with momentum > 0. */
NSG_API int nsg_audio_griffin_lim_fast(const float *S, const float *u, float *y, float *c, int32_t B, int32_t T, int32_t n_fft,
                                       int32_t hop, int32_t iters, float momentum, void *workspace, size_t workspace_bytes,
                                       void *stream);

/* Initial phases for Griffin-Lim by single-pass spectrogram inversion (SPSI; Beauregard, Harish, Wyse 2015), an extension: the
 * reference starts from random phases.  A spectral peak at the fractional bin j + p advances its phase by hop (j + p) / n_fft
 * turns a frame, and the bins of its main lobe are locked to it.  This is this project's own definition, with no parity claim.
 *   S [B][T][F] fp32 magnitudes, frame-major, F = n_fft/2 + 1  ->  angles [B][T][F] fp32, in turns in [0, 1): what
 *   nsg_audio_griffin_lim / _fast take as u.
 * All phase arithmetic is fp64, in turns, reduced mod 1 after every frame (radians accumulated in fp32 over ~900 frames lose the
 * phase); frac(x) = x - floor(x).  Per clip the state is phi[F], the centre phase last assigned to each bin, zero before frame 0.
 * With r = hop / n_fft (a power of two, so every product by it is exact), for t = 0 .. T-1 and m = S[b][t]:
 *   peaks     bin j in 1 .. F-2 is a peak iff m[j] > m[j-1] && m[j] > m[j+1], strict, on the fp32 values: a plateau is not a
 *             peak, a NaN is never one.
 *   offset    for a peak, with a, b, c = m[j-1], m[j], m[j+1] widened to fp64:  p = 0.5 * (a - c) / ((a - 2*b) + c), in that
 *             order; the denominator is strictly negative and |p| < 0.5.
 *   phase     val_j = phi[j] + (j + p) * r.
 *   regions   between consecutive peaks j < j' the boundary v is the FIRST index of the minimum of m[j .. j']; bins <= v belong to
 *             j, the rest to j'; bins below the first peak belong to it, bins above the last to the last.
 *   update    every bin k owned by j gets phi[k] = frac(val_j) (identity phase locking);
 *             a frame with no peak: phi[k] = frac(phi[k] + k * r) for every k.
 *   output    angles[b][t][k] = (float) frac(phi[k] + 0.5 * k); a result that rounds to 1.0f is written as 0.0f.  (0.5 k is the
 *             (-1)^k of a centred symmetric window's transform: adjacent main-lobe bins alternate in sign.)
 * Every operation is a correctly rounded IEEE operation or an exact product by a power of two, so angles is a function of S
 * alone, bit for bit: two calls agree, and a clip's angles do not depend on B or on its row.  The contract covers finite
 * magnitudes; non-finite ones give unspecified angles (and touch no memory outside the arguments).
 * Envelope: nsg_audio_griffin_lim's, except that T >= 1 (a single frame is legal, and hop * (T - 1) has no lower bound): n_fft in
 * {512, 1024, 2048}, hop divides n_fft, B * T < 2^31.  angles must not overlap the workspace.
 * workspace: nsg_audio_griffin_lim_workspace_bytes(B, T, n_fft) bytes (no query of its own); it holds, per (frame, bin), the fp64
 * advance and the uint16 owner: 10 F bytes a frame of that workspace's 16 F - 8.  A first launch, parallel over the B T frames, writes them; a second,
 * one workgroup per clip, walks the frames.  No atomics.
 * NSG_E_INVALID, before any launch: a null S / angles, B < 1, T < 1, hop < 1;  NSG_E_UNSUPPORTED: another n_fft, a hop that does not
 * divide it, too many frames or samples;  NSG_E_WORKSPACE: a null workspace or fewer bytes than the query's. */
NSG_API int nsg_audio_spsi_phases(const float *S, float *angles, int32_t B, int32_t T, int32_t n_fft, int32_t hop, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* The sums behind the spectral convergence || |stft(y)| - S || / || S || of waveforms y [B][hop*(T-1)] against magnitudes S [B][T][F],
 * on Griffin-Lim's grid and reflect map (n_fft, hop, T as nsg_audio_griffin_lim takes them; a grid shorter than n_fft/2 is legal).
 * With X = stft(y[b]) in fp32 and |X| = sqrtf(re^2 + im^2) as the phase kernels form it:
 *     frame_sums[b][t] = { sum_f (double)(fl32(|X[t][f]| - S[t][f]))^2,  sum_f (double)S[t][f]^2 }       [B][T][2] fp64, may be NULL
 *     clip_sums[b]     = the same pair summed over t                                                        [B][2] fp64
 * Both sums are fp64 in one fixed order (csrc/nsg_reduce.h): over the bins of a frame, thread k of 256 adds the bins k, k + 256, ...
 * to 0.0 in that order and the 256 thread sums are closed by the butterfly block sum (nsg_block_sum_butterfly); over the frames of a
 * clip, thread k adds the frames k, k + 256, ... to 0.0 in that order, closed the same way.  Two launches give the same bits, and a
 * clip's sums do not depend on B or on its row.  The spectrum is never stored and there is no workspace.  With frame_sums NULL the
 * same adds run in one workgroup per clip, frame after frame: the same bits, without the parallelism over the frames.
 * NSG_E_INVALID: a null y / S / clip_sums, B < 1, T < 2, hop < 1;  NSG_E_UNSUPPORTED: as nsg_audio_griffin_lim. */
NSG_API int nsg_audio_spectral_convergence(const float *y, const float *S, double *frame_sums, double *clip_sums, int32_t B,
                                           int32_t T, int32_t n_fft, int32_t hop, void *stream);

/* X [B][1 + L/hop][F] complex (interleaved re, im) = librosa.stft(y[b], n_fft, hop): centred, reflect-padded, periodic Hann.
 * n_fft in {512, 1024, 2048}, L > n_fft/2 (as librosa requires), any hop > 0, B * (1 + L/hop) < 2^31. */
NSG_API int nsg_audio_stft(const float *y, float *X, int32_t B, int32_t L, int32_t n_fft, int32_t hop, void *stream);

/* y[n] = x[n] + k * y[n-1] per clip (scipy.signal.lfilter([1], [1, -k], x); audio_tacotron.py:28-31), out of place,
 * |k| < 1.  Chunked with a discarded warm-up of ceil(log 1e-9 / log |k|) samples: chunks are independent to below fp32 rounding. */
NSG_API int nsg_audio_inv_preemphasis(const float *x, float *y, int32_t B, int32_t L, float k, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Waveform -> mel (the front end)   src/audio_tacotron.py:23-26,70-78,154-158,196-200,221-234 with hparams_tacotron.py
 * (use_lws=False, preemphasize, signal_normalization, allow_clipping_in_normalization, symmetric_mels=False).
 * ------------------------------------------------------------------------------------------- */

/* p[n] = x[n] - k * x[n-1], p[0] = x[0] per clip (scipy.signal.lfilter([1, -k], [1], x)); x, p [B][L], out of place. */
NSG_API int nsg_audio_preemphasis(const float *x, float *y, int32_t B, int32_t L, float k, void *stream);

/* One pass from samples to the normalised mel spectrogram, per clip b of len_b = lengths[b] samples (lengths NULL: all L):
 *     p[n]   = x[n] - k x[n-1],  p[0] = x[0]
 *     X[t]   = rfft(hann_periodic * reflect_pad(p[0:len_b], n_fft/2)[t hop : t hop + n_fft])          (librosa.stft)
 *     m[j,t] = sum_f basis[j][f] |X[t][f]|                                  over f in [bands[j][0], bands[j][1]] only
 *     S      = 20 log10(max(10^(min_level_db/20), m)) - ref_level_db
 *     out    = clip(max_abs (S - min_level_db) / (-min_level_db), 0, max_abs)
 * for t < T_b = 1 + len_b / hop; frames T_b <= t < T = 1 + L / hop are written as zeros.  A clip's result does not depend on
 * B, L or its position in the batch (bit for bit).  The spectrum never leaves the workgroup: only n_mels floats per frame
 * are stored.  wav [B][L] zero-padded; basis [n_mels][F] dense, F = n_fft/2 + 1, device; bands [n_mels][2] HOST memory: the
 * first and last bin of each row's non-zero run (first > last: an empty row, which yields the floor), read and checked
 * before the launch.  out [B][n_mels][T] (frame_major 0) or [B][T][n_mels] (frame_major 1).
 * n_fft in {512, 1024, 2048}, hop > 0, n_mels <= 128, L > n_fft/2, B * T < 2^31.
 * PRECONDITION the entry point cannot check (lengths is device memory): n_fft/2 < lengths[b] <= L for every b; the caller
 * checks it on the host copy it built lengths from.  (The kernel clamps lengths[b] into [1, L], so no read leaves wav.) */
NSG_API int nsg_audio_melspectrogram(const float *wav, const int32_t *lengths, const float *basis, const int32_t *bands,
                                     float *out, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t n_mels,
                                     float preemphasis, float min_level_db, float ref_level_db, float max_abs_value,
                                     int32_t frame_major, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Before the front end: resampling and silence trimming   src/audio_tacotron.py:12-13 (librosa.core.load(path, sr=...)),
 * src/cmu_arctic.py:72 (librosa.effects.trim(wav, top_db=20)).  parity unpinned: librosa and resampy are absent.
 * ------------------------------------------------------------------------------------------- */

/* Band-limited resampling by the rational factor up / down = P / Q (in lowest terms), per clip b of len_b = lengths[b]
 * samples (lengths NULL: all L_in):
 *     y[m] = sum_n x[n] * s h(s (m Q - n P) / P),   s = min(1, P / Q),  x zero outside [0, len_b)
 *     h(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta)  for |u| < Z, else 0;  sinc(v) = sin(pi v) / (pi v)
 * a Kaiser-windowed sinc with Z zero crossings a side, evaluated per polyphase phase phi = (m Q) mod P exactly -- no
 * interpolation in a filter table.  The caller supplies the coefficients, W = half_width = ceil(Z / s), 2 W taps a phase:
 *     c[phi][j] = s h(s (phi / P + W - 1 - j))   multiplies   x[floor(m Q / P) - W + 1 + j],   j = 0 .. 2 W - 1
 * stored tap-major with the phases in the order consecutive outputs meet them:  table[j][k] = c[(k Q) mod P][j], k = m mod P,
 * [2 W][P] floats on the device (consecutive lanes read consecutive floats).  An output is one fp32 fmaf chain over j
 * increasing, from 0: a clip's samples depend on its own samples and length alone, never on B, L_in, its row or the tiling
 * (bit for bit).  wav [B][L_in] zero-padded; out [B][L_out], L_out = ceil(L_in P / Q); clip b has ceil(len_b P / Q) samples
 * (its last one included: librosa would zero-pad it when floor != ceil), the rest of its row is written as zeros.
 * Index arithmetic in 64 bits.  NSG_E_INVALID: a null pointer, a non-positive size, up / down not in lowest terms;
 * NSG_E_UNSUPPORTED: P * 2 W > 2^20 floats, L_out >= 2^31, B * ceil(L_out / 256) >= 2^31, or a tile's input span
 * (255 Q / P + 2 W + 1 floats) above 64 KiB of LDS.  lengths[b] is clamped into [0, L_in], so no read leaves wav. */
NSG_API int nsg_audio_resample(const float *wav, const int32_t *lengths, const float *table, float *out, int32_t B, int32_t L_in,
                               int32_t up, int32_t down, int32_t half_width, void *stream);

/* librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) restated, per clip b of len_b = lengths[b] samples
 * (lengths NULL: all L):
 *     p      = reflect_pad(y[0:len_b], frame_length / 2),   T_b = 1 + len_b / hop
 *     mse[t] = mean(p[t hop : t hop + frame_length]^2),   ref = max_t mse[t]
 *     frame t is non-silent iff 10 log10(max(1e-10, mse[t])) - 10 log10(max(1e-10, ref)) > -top_db
 *     bounds[b] = (first hop, min(len_b, (last + 1) hop)) over the non-silent frames, (0, 0) if there is none
 * A frame's energy is summed in a fixed order of its own samples (64 strided partial sums, then a fixed butterfly); the
 * per-clip maximum and the first / last search are exact, so a clip's bounds do not depend on the batch.  wav [B][L]
 * zero-padded; bounds [B][2] int32; workspace: nsg_audio_trim_workspace_bytes(B, L, hop) bytes (the frame energies).
 * NSG_E_INVALID: a null pointer, a non-positive size, top_db not > 0; NSG_E_UNSUPPORTED: frame_length odd or outside
 * [2, 8192], L <= frame_length / 2, too many frames.  PRECONDITION the entry point cannot check (lengths is device memory):
 * frame_length / 2 < lengths[b] <= L; the caller checks it on its host copy (the kernels clamp into [1, L]). */
NSG_API size_t nsg_audio_trim_workspace_bytes(int32_t B, int32_t L, int32_t hop);
NSG_API int nsg_audio_trim_bounds(const float *wav, const int32_t *lengths, int32_t *bounds, int32_t B, int32_t L,
                                  int32_t frame_length, int32_t hop, float top_db, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* ---------------------------------------------------------------------------------------------
 * The loader's batch from a corpus resident in device memory   src/dataloader.py:324-434 (collate_fn, the mel case): crop,
 * zero-pad to the batch's longest item, transpose to mel-major -- one launch, no host work per batch.
 * ------------------------------------------------------------------------------------------- */

/* corpus [corpus_frames][n_mels] fp32, frame-major: the clips' (frames, n_mels) arrays as they are on disk, concatenated.
 * plan [B][3] int64, device: per item (clip, start, count) -- start = its first corpus frame, count = frames to copy; clip is
 * not read here (the loader gathers speaker ids with it).  out [B][n_mels][T] fp32, the memory of the model's (B, 1, n_mels, T):
 *     out[b][m][t] = corpus[start_b + t][m]   for t < count_b,        +0.0f   for count_b <= t < T
 * A copy, bit for bit; every element of out is written exactly once (out need not be initialised).  One workgroup per tile of
 * 32 frames of one item; B is not bound by a grid dimension; every element offset is 64-bit (corpus and out may pass 2^31
 * elements).  16-byte accesses are used only where they are aligned (loads: n_mels % 4 == 0 and corpus 16-byte aligned;
 * stores: T % 4 == 0 and out 16-byte aligned); any n_mels, T and alignment of 4 is served.
 * NSG_E_INVALID: a null pointer, B < 1, T < 1, n_mels outside [1, 128], corpus_frames < 0.
 * PRECONDITION the entry point cannot check (plan is device memory): 0 <= count_b <= T, start_b >= 0 and
 * start_b + count_b <= corpus_frames for every b; the caller checks it on the host copy it built the plan from.  (The kernel
 * clamps count_b into [0, T] and reads a frame outside [0, corpus_frames) as zero, so no access leaves either buffer.) */
NSG_API int nsg_collate_mels(const float *corpus, int64_t corpus_frames, int32_t n_mels, const int64_t *plan, int32_t B, int32_t T,
                             float *out, void *stream);

/* The same batch's waveform (collate_fn's audio: x[s hop : (s + count) hop], zero-padded to the batch's longest) from the clips'
 * samples kept beside the mels.  corpus [corpus_samples] fp32: the clips' on-disk audio arrays concatenated in the mel corpus'
 * clip order; every clip has frames * hop samples, so the clip whose mels start at corpus frame f starts at sample f * hop and
 * corpus_samples = corpus_frames * hop.  plan [B][3] int64, DEVICE memory: nsg_collate_mels' own rows (clip, start, count) in
 * FRAMES, clip not read.  out [B][T * hop] fp32, the memory of the loader's x (B, 1, T hop) and y (B, T hop, 1):
 *     out[b][i] = corpus[start_b * hop + i]   for i < count_b * hop,        +0.0f   for count_b * hop <= i < T * hop
 * A copy, bit for bit; every element of out is written exactly once (out need not be initialised).  One launch, no workspace,
 * no LDS; a lane has four independent accesses in flight; neither B nor a row's length is bound by a grid dimension; every
 * corpus and out offset is 64-bit (both may pass 2^31 elements).  16-byte accesses are used only where every such access is
 * aligned (loads: hop % 4 == 0 and corpus 16-byte aligned; stores: (T * hop) % 4 == 0 and out 16-byte aligned); any hop >= 1, any
 * T and any alignment of 4 is served.
 * NSG_E_INVALID: a null pointer, B < 1, T < 1, hop < 1, corpus_samples < 0, T * hop not below 2^31, a pointer not aligned to its
 * element (4 bytes; plan 8).
 * PRECONDITION the entry point cannot check (plan is device memory): nsg_collate_mels', with corpus_frames = corpus_samples / hop;
 * the caller checks its host copy.  (The kernel clamps count_b into [0, T] and reads a sample outside [0, corpus_samples) as
 * +0.0, so whatever the plan holds no access leaves either buffer.) */
NSG_API int nsg_collate_audio(const float *corpus, int64_t corpus_samples, int32_t hop, const int64_t *plan, int32_t B, int32_t T,
                              float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Judging a converted utterance: mel cepstra and dynamic time warping (extension; the reference has no objective figure
 * for the speaker-conditioned decoder).  evaluate.test_conversion reports the mel-cepstral distortion of parallel pairs.
 * ------------------------------------------------------------------------------------------- */

/* mel [B][n_mels][T] fp32, mel-major (the model's (B, 1, n_mels, T); what nsg_audio_melspectrogram writes with frame_major 0)
 * -> c [B][T][K] fp32, frame-major:
 *     c[b][t][k] = sum_j mel[b][j][t] * table[k][j]        for t < frames[b]   (frames NULL: every t < T)
 * one fp32 chain per output: the accumulator starts at +0.0 and takes j = 0, 1, ... in order, each product rounded to fp32 and
 * each sum rounded to fp32, never contracted.  Frames t >= frames[b] are written as +0.0 and their mels are not read.
 * table [K][n_mels] fp32 is the caller's (audio.cepstra_table: rows 1 .. K of the orthonormal DCT-II, scaled to the natural-log
 * amplitude).  Every element of c is written exactly once.  One workgroup per 64 frames of one clip: the loads run along t.
 * NSG_E_INVALID: a null mel / table / c, B < 1, T < 1, B * ceil(T / 64) >= 2^31;  NSG_E_UNSUPPORTED: K outside [1, 64], n_mels outside
 * [1, 128].  frames[b] is device memory: the kernel clamps it into [0, T]. */
NSG_API int nsg_mel_cepstra(const float *mel, const int32_t *frames, const float *table, float *c, int32_t B, int32_t n_mels,
                            int32_t T, int32_t K, void *stream);

/* Batched dynamic time warping of feature sequences under the Euclidean frame distance.
 *   a [B][Ta][K], b [B][Tb][K] fp32; len_a, len_b [B] int32: pair p compares a[p][0 : len_a[p]] with b[p][0 : len_b[p]];
 *   d(i, j) = sqrtf( sum_k (a[i][k] - b[j][k])^2 ): the accumulator starts at +0.0, k ascending; the subtraction, the product and
 *             the sum are each rounded to fp32 and never contracted; the square root is correctly rounded;
 *   D(0, 0) = d(0, 0),  D(i, j) = fl( min(D(i-1, j-1), D(i-1, j), D(i, j-1)) + d(i, j) ), predecessors outside the grid absent;
 *             among equal predecessors the first of (i-1, j-1), (i-1, j), (i, j-1) is taken;
 *   n(0, 0) = 1,  n(i, j) = n(the predecessor taken) + 1: the length of the path, carried along with D;
 *   cost[p] = D(len_a - 1, len_b - 1),  steps[p] = n(len_a - 1, len_b - 1)      (cost [B] fp32, steps [B] int32);
 *   path (or NULL) [B][Ta + Tb - 1][2] int32: the cells (i, j) of the path from (0, 0) to the end cell, steps[p] of them; rows
 *             past that are not written.
 * Elements of a and b past a pair's lengths are never read.  One wave per pair: lane l owns NSG_DTW_BLOCK_COLS / 64 adjacent
 * columns of b and walks the rows of a one row behind lane l - 1; a sequence b longer than NSG_DTW_BLOCK_COLS runs as
 * successive blocks of that many columns, a block's last column handed to the next in LDS.  Without path nothing of size
 * Ta x Tb is stored; with it the workspace holds the predecessor taken at each cell, which the same launch walks back.
 * NSG_E_INVALID: a null required pointer, B < 1;  NSG_E_UNSUPPORTED: K outside [1, 64], Ta or Tb outside [1, NSG_DTW_MAX_FRAMES];
 * NSG_E_WORKSPACE: path given with less than nsg_dtw_workspace_bytes(B, Ta, Tb, 1) bytes (path == NULL needs none).
 * PRECONDITION the entry point cannot check (the lengths are device memory): 1 <= len_a[p] <= Ta, 1 <= len_b[p] <= Tb; the
 * caller checks it on the host copy it built them from.  (The kernel clamps them into that range, so no access leaves a buffer.) */
#define NSG_DTW_MAX_FRAMES 2048
#define NSG_DTW_BLOCK_COLS 256
NSG_API size_t nsg_dtw_workspace_bytes(int32_t B, int32_t Ta, int32_t Tb, int32_t want_path);
NSG_API int nsg_dtw(const float *a, const float *b, const int32_t *len_a, const int32_t *len_b, float *cost, int32_t *steps,
                    int32_t *path, int32_t B, int32_t Ta, int32_t Tb, int32_t K, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ---------------------------------------------------------------------------------------------
 * Judging a converted utterance by its pitch: F0 tracking (YIN, de Cheveigne & Kawahara 2002) and F0 statistics along a
 * warping path (extension; the reference has no pitch code).  parity unpinned: the contract is the one stated here, restated in
 * fp32 and fp64 by tests/helpers/f0_ref.py.  evaluate.test_conversion_f0 reports F0 error, voicing error and log-F0 correlation.
 * ------------------------------------------------------------------------------------------- */

/* Per clip b of len_b = lengths[b] samples (lengths NULL: all L), x = wav[b] read as zero outside [0, len_b) (samples past
 * len_b are never read), W = frame_length, and frame t < T_b = 1 + len_b / hop of T = 1 + L / hop (the front end's frame count;
 * frame t is centred on sample t hop, as mel frame t is):
 *     s0      = t hop - W / 2
 *     d(tau)  = sum_{j=0}^{W-1} (x[s0 + j] - x[s0 + j + tau])^2                          tau = 1 .. tau_max
 *     c(tau)  = sum_{k=1}^{tau} d(k)
 *     d'(tau) = d(tau) * tau / c(tau)  if c(tau) > 0,  else 1                            (cumulative-mean-normalised difference)
 *     tau*    = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then advanced while tau + 1 <= tau_max and
 *               d'(tau + 1) < d'(tau)
 *     voiced:     a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1);  if tau* - 1 >= 1, tau* + 1 <= tau_max, a >= b, c >= b and
 *                 a - 2b + c > 0:  delta = 0.5 (a - c) / (a - 2b + c)  (so |delta| <= 0.5),  else delta = 0
 *                 f0[b][t] = sample_rate / (tau* + delta),   ap[b][t] = d'(tau*)
 *     no such tau:  f0[b][t] = +0.0 (unvoiced),   ap[b][t] = min over tau in [tau_min, tau_max] of d'(tau)
 *     t >= T_b:     f0[b][t] = +0.0,  ap[b][t] = 1.0
 * The direct sum of squared differences, never an autocorrelation or FFT identity: at a period d is a sum of tiny squares with
 * nothing to cancel, which is what makes fp32 enough.  Everything is fp32; each subtraction, product, sum and quotient is rounded
 * to fp32 and never contracted, in this order (the one place it is stated):
 *     d(tau):   one chain per lag: the accumulator starts at +0.0 and takes fl(fl(x[s0+j] - x[s0+j+tau])^2) for j = 0, 1, ... in order;
 *     c(tau):   the lags in groups of NSG_F0_LAG_GROUP = 8 (1 .. 8, 9 .. 16, ...), tau in group g = (tau - 1) / 8 with first lag
 *               g0 = 8 g + 1:  p(tau) = the chain d(g0) + d(g0 + 1) + ... + d(tau) in that order;  G(g) = the chain from +0.0 over
 *               the totals p(8 g' + 8) of the groups g' = 0 .. g - 1 in order;  c(tau) = fl(G(g) + p(tau));
 *     d'(tau):  fl(fl(d(tau) * (float)tau) / c(tau)), the division correctly rounded;
 *     delta:    fl(fl(0.5 * fl(a - c)) / fl(fl(a - fl(2 b)) + c));   f0 = fl(sample_rate / fl((float)tau* + delta)).
 * A frame's result is a function of its own samples only: bit for bit independent of B, L, the clip's row and any tiling.
 * wav [B][L]; f0, ap [B][T] fp32, every element written exactly once; no workspace.  Lanes own runs of adjacent lags over a
 * frame's span of samples staged once in LDS (csrc/f0.hip).
 * NSG_E_INVALID: a null wav / f0 / ap, a non-positive B, L, frame_length, hop, tau_min or tau_max, threshold not in (0, 1],
 * sample_rate not > 0;  NSG_E_UNSUPPORTED: frame_length odd or outside [64, 2048], tau_min > tau_max, tau_max > 1024,
 * B * T >= 2^31.  lengths[b] is device memory: the kernel clamps it into [0, L], so no read leaves wav; the caller checks it on the
 * host copy it built lengths from. */
#define NSG_F0_LAG_GROUP 8
NSG_API int nsg_audio_f0(const float *wav, const int32_t *lengths, float *f0, float *ap, int32_t B, int32_t L, int32_t frame_length,
                         int32_t hop, int32_t tau_min, int32_t tau_max, float threshold, float sample_rate, void *stream);

/* F0 statistics along warping paths.  f0_a [B][Ta], f0_b [B][Tb] fp32 (a value that is not > 0 means unvoiced); path
 * [B][Ta + Tb - 1][2] int32 and steps [B] int32 in nsg_dtw's layout; stats [B][10] fp64, over the first steps[p] cells (i, j) of
 * pair p, with x = log2((double)f0_a[p][i]), y = log2((double)f0_b[p][j]) on the cells both clips voice:
 *     { steps, n_vv, n_a_only, n_b_only, sum x, sum y, sum x^2, sum y^2, sum x y, sum (x - y)^2 }
 * (n_vv: both voiced; n_a_only / n_b_only: one voiced).  The counts are exact integers held in doubles.  One wave per pair:
 * lane l adds the cells l, l + 64, ... to 0.0 in that order, then an xor-butterfly (offsets 32 .. 1) adds the lanes, so a pair's
 * result does not depend on the batch.  steps[p] is clamped into [0, Ta + Tb - 1] and each cell into the grid, so no access
 * leaves a buffer; path rows past steps[p] are not read.
 * NSG_E_INVALID: a null pointer, B < 1, Ta < 1, Tb < 1;  NSG_E_UNSUPPORTED: Ta + Tb - 1 >= 2^30. */
NSG_API int nsg_f0_path_stats(const float *f0_a, const float *f0_b, const int32_t *path, const int32_t *steps, double *stats,
                              int32_t B, int32_t Ta, int32_t Tb, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A path finder over per-frame F0 candidates (Boersma 1993; RAPT): instead of deciding each frame on its own, keep the local
 * minima of d' and let a dynamic programme choose one per frame, or "unvoiced" (extension; parity unpinned: the contract is
 * the one stated here, restated in fp32 and fp64 by tests/helpers/f0_track_ref.py).  audio.f0_track runs the two in turn.
 * ------------------------------------------------------------------------------------------- */

/* The candidates of every frame.  wav, lengths, the frames, the zero padding, d(tau), c(tau) and d'(tau) are nsg_audio_f0's, in
 * its fp32 order (csrc/f0.hip: the two kernels share that half as code).  Per frame t < T_b a lag tau in
 * [max(tau_min, 2), tau_max] is a candidate iff
 *     d'(tau) < d'(tau - 1)    (the left neighbour is used also where it lies below tau_min),
 *     tau = tau_max  or  d'(tau) <= d'(tau + 1)    (the first lag of a plateau),    and    d'(tau) < 1.
 * Of a frame's candidates the NSG_F0_MAX_CANDIDATES = 8 with the smallest pairs (d'(tau), tau) in lexicographic order are kept
 * (exactly, whatever order the machine meets them in) and stored by ASCENDING LAG: slot 0 is the highest frequency.  Each is
 * refined by nsg_audio_f0's parabola, under its conditions (tau - 1 >= 1, tau + 1 <= tau_max, a >= b, c >= b, a - 2b + c > 0) and
 * in its fp32 order:
 *     cand_f0 = fl(sample_rate / fl((float)tau + delta)),   cand_ap = d'(tau),   cand_logf = (float)log2((double)cand_f0)
 * (the fp64 logarithm rounded once to fp32, as nsg_f0_path_stats takes logarithms).
 * cand_f0, cand_ap, cand_logf [B][T][8] fp32, count [B][T] int32 (the candidates kept, 0 .. 8); every element is written exactly
 * once: slots past count hold +0.0, 1.0 and +0.0, frames t >= T_b have count 0.  No workspace.  A frame's result is a function
 * of its own samples only.
 * NSG_E_INVALID / NSG_E_UNSUPPORTED: as nsg_audio_f0 (there is no threshold), a null output among them. */
#define NSG_F0_MAX_CANDIDATES 8
NSG_API int nsg_audio_f0_candidates(const float *wav, const int32_t *lengths, float *cand_f0, float *cand_ap, float *cand_logf,
                                    int32_t *count, int32_t B, int32_t L, int32_t frame_length, int32_t hop, int32_t tau_min,
                                    int32_t tau_max, float sample_rate, void *stream);

/* A min-sum path over candidate tensors; nothing here knows of audio.  cand_logf, cand_ap, cand_f0 [B][T][8] fp32, count [B][T]
 * int32 (each value clamped into [0, 8]; slots past it are never read), frames [B] int32 device memory (NULL: T; clamped into
 * [0, T]): clip b has T_b = frames[b] frames.  The states of frame t are 0 (unvoiced) and k = 1 .. count[t] (slot k - 1).  All
 * arithmetic is fp32, each operation rounded and never contracted, with logf_k, ap_k of frame t and logf'_j of frame t - 1:
 *     local(t, 0) = unvoiced_cost
 *     local(t, k) = fl(ap_k + fl(octave_cost * fl(logf_top - logf_k)))
 *     trans(j, k) = +0.0                                      j = k = 0
 *                 = vuv_cost                                  exactly one of j, k is 0
 *                 = fl(jump_cost * |fl(logf_k - logf'_j)|)    both voiced
 *     D(0, k)     = local(0, k)
 *     D(t, k)     = fl(local(t, k) + min_j fl(D(t - 1, j) + trans(j, k)))       (the sum with trans = +0.0 is formed too)
 * The minimum is taken over j = 0, 1, ..., count[t - 1] ascending with a strict <: ties go to the smallest j, which is the
 * back-pointer.  The end state is the smallest k that minimises D(T_b - 1, k) (strict <, k ascending); the back-pointers give the
 * path.  state [B][T] int32: the path, -1 for t >= T_b.  cost [B] fp32: D(T_b - 1, end state), +0.0 when T_b = 0.
 * f0, ap [B][T] fp32: the chosen candidate's cand_f0 and cand_ap; on an unvoiced frame +0.0 and the least cand_ap of the frame's
 * candidates (slot 0 first, then each later slot that is < the least so far), 1.0 when it has none; (+0.0, 1.0) for t >= T_b,
 * nsg_audio_f0's convention.  Every element is written exactly once.  A clip's result does not depend on B or on its row.
 * One wave per clip: lanes 0 .. 8 own the states and read frame t - 1's D and logf out of one another's registers; the
 * candidate rows are staged into LDS 64 frames at a time; a lane packs its back-pointers 4 bits a frame, a 32-bit word per 8
 * frames, into LDS when T <= NSG_F0_VITERBI_LDS_FRAMES = 2048 and into the workspace beyond (csrc/f0_track.hip).
 * nsg_f0_viterbi_workspace_bytes(B, T): 0 for T <= 2048 (workspace may then be NULL).
 * NSG_E_INVALID: a null pointer other than frames (and workspace where none is needed), B < 1, T < 1, a cost that is negative or
 * not finite, logf_top not finite;  NSG_E_UNSUPPORTED: B * T >= 2^31;  NSG_E_WORKSPACE: fewer than
 * nsg_f0_viterbi_workspace_bytes(B, T) bytes. */
#define NSG_F0_VITERBI_LDS_FRAMES 2048
NSG_API size_t nsg_f0_viterbi_workspace_bytes(int32_t B, int32_t T);
NSG_API int nsg_f0_viterbi(const float *cand_logf, const float *cand_ap, const float *cand_f0, const int32_t *count,
                           const int32_t *frames, int32_t *state, float *cost, float *f0, float *ap, int32_t B, int32_t T,
                           float logf_top, float octave_cost, float jump_cost, float vuv_cost, float unvoiced_cost,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Augmenting a recording: tempo change without pitch change (waveform-similarity overlap-add, Verhelst & Roelands 1993), and
 * gain plus noise at a level relative to the clip's RMS   src/util.py:106-134 (augment_audio_with_sox: `sox tempo ... gain ...`),
 * src/util.py:164-196 (NoiseInjection).  parity unpinned: sox is absent; the contract is the one stated here, restated in fp32 and
 * fp64 by tests/helpers/tempo_ref.py.  audio.tempo, audio.pitch_shift (tempo, then nsg_audio_resample), audio.mix_noise.
 * ------------------------------------------------------------------------------------------- */

/* S = segment length, O = overlap, W = search width, in samples; Ho = S - O, the output hop.  Per clip b: len = lengths[b]
 * (lengths NULL: L), f = factor[b] (fp64; above 1 is faster), out_len = out_lengths[b], x = wav[b] read as zero outside [0, len)
 * (samples past len are never read), M = ceil(out_len / Ho) segments:
 *     q_0 = 0;   for m = 1 .. M - 1, in order:
 *     n_m      = (int64) floor((double)(m Ho) * f)                      one fp64 product of an exact integer and f
 *     d_m(dl)  = sum_{j=0}^{O-1} (x[q_{m-1} + Ho + j] - x[n_m + dl + j])^2      dl = 0 .. W - 1
 *     q_m      = n_m + dl*,   dl* the SMALLEST dl that minimises d_m
 * d_m is fp32: one chain per dl, the accumulator starts at +0.0 and takes fl(fl(a - c)^2) for j = 0, 1, ... in order; the
 * subtraction, the product and the sum are each rounded and never contracted (nsg_audio_f0's rule).  Output sample k < out_len,
 * with m = k / Ho and j = k mod Ho:
 *     m >= 1 and j < O:   a = x[q_{m-1} + Ho + j],  b = x[q_m + j],  w = fl((float)j / (float)O):   out = fl(a + fl(w * fl(b - a)))
 *     otherwise:          out = x[q_m + j]
 * and +0.0 for out_len <= k < L_out.  (The cross-fade is written a + w (b - a): where the two segments agree the output is that
 * value exactly, so f = 1 returns the input bit for bit -- dl = 0 gives d = +0.0, the first minimum -- and a signal with an
 * integer period P <= W and small integer samples comes out as its own periodic continuation wherever every sample read lies
 * inside the clip.)  positions (or NULL) [B][M_max] int32, M_max = ceil(L_out / Ho):  positions[b][m] = q_m for m < M, -1 beyond.
 * A clip's output is a function of its own samples, length and factor: bit for bit independent of B, L, L_out, its row and any
 * tiling.  wav [B][L] fp32; out [B][L_out] fp32, every element written exactly once.
 * lengths, factor [B] fp64 and out_lengths [B] int32 are DEVICE memory.  PRECONDITION the entry point cannot check: factor finite
 * and in [0.25, 4], 0 <= lengths[b] <= L, out_lengths[b] = floor((double)lengths[b] / factor[b]) <= L_out (under it every
 * n_m < len); the caller checks it on the host copy it uploads.  The kernels clamp lengths into [0, L], out_lengths into
 * [0, L_out] and take an n_m that is not in [0, len) as len (every sample read there is zero), so no access leaves a buffer.
 * Two launches: a chain over the segments, one workgroup per clip -- tail and candidate window in LDS, lanes own runs of adjacent
 * dl over a sliding register window, the minimum as an integer minimum of bits(d) << 32 | dl; the ranges of the next step are
 * loaded while this one is searched -- and a sample-parallel pass that forms out from the positions (csrc/tsm.hip).  Without
 * positions the q_m are kept in the workspace: nsg_audio_tempo_workspace_bytes(B, L_out, S, O) bytes ([B][M_max] int32); with
 * positions no workspace is needed (it may be NULL).
 * NSG_E_INVALID: a null wav / factor / out_lengths / out, B < 1, L < 1, L_out < 1;  NSG_E_UNSUPPORTED: O outside [1, 2048], S outside
 * [2 O, 8192], W outside [1, 2048], B * L_out >= 2^31, L + S + W >= 2^31;  NSG_E_WORKSPACE: positions NULL and fewer workspace
 * bytes than the query states. */
NSG_API size_t nsg_audio_tempo_workspace_bytes(int32_t B, int32_t L_out, int32_t S, int32_t O);
NSG_API int nsg_audio_tempo(const float *wav, const int32_t *lengths, const double *factor, const int32_t *out_lengths, float *out,
                            int32_t *positions, int32_t B, int32_t L, int32_t L_out, int32_t S, int32_t O, int32_t W, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Gain, and one noise recording added at a level relative to each clip's RMS (util.py:193-195 with sox's `gain` in front;
 * data_energy / noise_energy there is sqrt(E_x / E_n): the two lengths cancel).  Per clip b of len = lengths[b] samples (lengths
 * NULL: L), with v_i = noise[(offset[b] + i) mod Ln] -- one recording, read cyclically:
 *     E_x = sum_{i < len} (double)x_i^2,   E_n = sum_{i < len} (double)v_i^2
 *     s   = (float)((double)level[b] * sqrt(E_x / E_n))    in fp64, rounded once;  s = +0.0 where E_n = 0 or len = 0
 *     out_i = fl(fl(gain[b] * x_i) + fl(s * v_i))   for i < len,   +0.0 for len <= i < L        (never contracted)
 * The two sums are fp64 in this fixed order (csrc/nsg_reduce.h): the clip in partials of NSG_MIX_PARTIAL = 4096 samples; in
 * partial p thread t of 256 adds the squares of samples 4096 p + t + 256 k, k = 0 .. 15, to 0.0 in that order, and the 256 thread
 * sums are closed by the four-then-walk block sum (nsg_block_sum_four_walk); the partials are closed by the one-wave closer
 * (nsg_wave_close_sum: lane l adds partials l, l + 64, ..., then lane 0 adds the 64 lane sums in lane order).  So a clip's result
 * does not depend on B or on its row.  wav, out [B][L] fp32 (out may not alias wav); noise [Ln] fp32; gain, level [B] fp32 and
 * offset [B] int32 in [0, Ln) are device memory (offset is clamped into that range, lengths into [0, L]); energy (or NULL)
 * [B][2] fp64 receives (E_x, E_n).  Every element of out is written exactly once.  workspace:
 * nsg_audio_mix_noise_workspace_bytes(B, L) bytes (the partials and s).
 * NSG_E_INVALID: a null pointer other than lengths and energy, B < 1, L < 1, Ln < 1;  NSG_E_UNSUPPORTED: B * ceil(L / 1024) >= 2^31;
 * NSG_E_WORKSPACE: fewer bytes than the query states. */
#define NSG_MIX_PARTIAL 4096
NSG_API size_t nsg_audio_mix_noise_workspace_bytes(int32_t B, int32_t L);
NSG_API int nsg_audio_mix_noise(const float *wav, const int32_t *lengths, const float *noise, const float *gain, const float *level,
                                const int32_t *offset, float *out, double *energy, int32_t B, int32_t L, int32_t Ln, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Judging a reconstructed waveform against the recording: short-time objective intelligibility, STOI (Taal, Hendriks, Heusdens,
 * Jensen 2011) and extended STOI (Jensen, Taal 2016).  An extension: the reference has no figure in the waveform domain.  parity
 * unpinned: pystoi is absent; the definition is this project's own, written from the two papers and stated here in full,
 * restated in fp64 by tests/helpers/stoi_ref.py.  audio.stoi_envelopes, audio.stoi (csrc/stoi.hip).
 * ------------------------------------------------------------------------------------------- */

/* Everything is at 10 000 Hz (the caller resamples).  x [B][L] fp32 is the clean batch, y [B][L] the processed one, aligned sample
 * for sample; clip b has len = lengths[b] samples of its row (lengths NULL: L; int32 DEVICE memory).
 *   window     w[n] = 0.5 - 0.5 cos(2 pi (n + 1) / 257), n = 0 .. 255 (MATLAB's hanning(256)), evaluated in fp64.
 *   candidates frame t = 0 .. T_b - 1, T_b = (len - 256) / 128 + 1, is samples 128 t .. 128 t + 255 of x, with the energy
 *                  energy[b][t] = sum_n ((double)w[n] * (double)x[128 t + n])^2                          [B][Tmax] fp64
 *              products, squares and sum in fp64 in one fixed order: with n = 4 l + i, lane l of 64 adds its squares i = 0 .. 3 to
 *              0.0 in that order, and the 64 lane sums are closed by xor-butterflies over the offsets 32, 16, .., 1
 *              (csrc/nsg_reduce.h: nsg_wave_sum_butterfly).  Tmax = (L - 256) / 128 + 1; energy[b][t] = 0.0 for t >= T_b.
 *   selection  frame t is kept iff energy[b][t] > 1e-4 * max_t energy[b][t]: a strict comparison in fp64 against the exact maximum
 *              (the 40 dB range); an all-zero clip keeps nothing.  The decision comes from x alone.  src[b][k] = the k-th kept
 *              frame, ascending, for k < C = kept[b], and -1 for C <= k < Tmax.                          [B][Tmax], [B] int32
 *   compaction xs[128 k + n] += w[n] x[128 src[k] + n], k < C, n < 256, and ys the same with the same src: a sample of xs is the
 *              sum of at most two windowed source samples.  It is formed where it is used and never stored.
 *   spectrum   frame m = 0 .. C - 1 is w[n] xs[128 m + n], n < 256, in fp32 with the window rounded to fp32:
 *                  fl(w[n] * fl(fl(w[n'] x[128 src[m'] + n']) + fl(w[n''] x[128 src[m''] + n''])))   the two (m', n'), m' < m'', with
 *              128 m' + n' = 128 m + n, or the one product when there is one; zero-padded to 512; X = its 512-point DFT; |X[f]|^2 on
 *              f = 0 .. 256.  x's and y's frame are the real and the imaginary part of one complex radix-2 FFT in fp32, split by
 *              Hermitian symmetry.
 *   bands      j = 0 .. 14: the bins [band_lo[j], band_hi[j]).  audio.stoi_bands() builds the third-octave table: with f[i] = i
 *              10000 / 512, band_lo[j] = argmin_i |f[i] - 150 * 2^((2 j - 1) / 6)|, band_hi[j] = argmin_i |f[i] - 150 * 2^((2 j + 1) / 6)|
 *              (band 0 is bins 7 .. 8; band 14 ends below bin 257).
 *                  env[0][b][m][j] = sqrtf(sum_{f in band j} |X[m][f]|^2),  env[1][b][m][j] the same for y   [2][B][Tmax][15] fp32
 *              the sum in fp32 added to 0.f in index order; rows m >= C are written as zeros.
 * A clip's five outputs depend on its own samples and length alone: bit for bit independent of B, L and its row.  Every element of
 * energy, src, kept and env is written exactly once.  No workspace, no atomics, three launches: energies (one wave per frame),
 * selection (one workgroup per clip: exact maximum, keep mask, exclusive block scan), envelopes (one workgroup per (clip, m) on a
 * grid of B * Tmax; those with m >= C write their zeros and leave).  band_lo, band_hi [15] int32 are HOST memory, read and checked
 * before the first launch.
 * NSG_E_INVALID: a null pointer other than lengths, B < 1, bands that are not 15 ascending non-empty runs inside 0 .. 256
 * (0 <= lo_0, lo_j < hi_j, hi_j <= lo_{j+1}, hi_14 <= 257);  NSG_E_UNSUPPORTED: L < 256, B * Tmax >= 2^31.
 * A lengths[b] below 256 or above L cannot be refused on the host: such a clip has T_b = 0, kept[b] = 0 and a NaN figure. */
NSG_API int nsg_audio_stoi_envelopes(const float *x, const float *y, const int32_t *lengths, const int32_t *band_lo,
                                     const int32_t *band_hi, double *energy, int32_t *src, int32_t *kept, float *env, int32_t B,
                                     int32_t L, void *stream);

/* The figure from the envelopes: env [2][B][Tmax][15] fp32 and kept [B] int32 as nsg_audio_stoi_envelopes writes them (kept is
 * clamped to Tmax) -> d [B] fp64.  All arithmetic is fp64 on the widened envelopes; eps = 2^-52.  With C = kept[b], a segment is the
 * 30 frames m - 29 .. m for m = 29 .. C - 1; x_j, y_j are the 30-vectors of band j of env[0], env[1]; every sum below runs over its
 * index ascending from 0.0.
 *   extended = 0, STOI:   alpha = sqrt(sum x_j^2 / (sum y_j^2 + eps));   y'_j = min(alpha y_j, (1 + 10^(15/20)) x_j) element-wise;
 *       d[m][j] = sum (x_j - mean x_j)(y'_j - mean y'_j) / (sqrt(sum (x_j - mean x_j)^2) * sqrt(sum (y'_j - mean y'_j)^2) + eps)
 *       with mean v = (sum v) / 30;  d[b] = the mean of d[m][j] over all 15 (C - 29) pairs.
 *   extended = 1, ESTOI:  on the 15 x 30 segment matrices of X and of Y separately, subtract each row's mean and multiply each row by
 *       1 / (its norm + eps); then subtract each column's mean (over the 15 bands) and divide each column by (its norm + eps);
 *       d[m] = (1 / 30) sum_n sum_j X~[j][n] Y~[j][n];  d[b] = the mean of d[m] over the C - 29 segments.
 * The per-item figures are added in one fixed order (csrc/nsg_reduce.h): thread k of 256 adds its items k, k + 256, ... to 0.0 in
 * that order (item i of STOI is the segment ending at 29 + i / 15, band i mod 15; item i of ESTOI the segment ending at 29 + i), the
 * 256 thread sums are closed by the butterfly block sum (nsg_block_sum_butterfly), and the total is divided by the item count.  Two
 * calls give the same bits, and a clip's figure does not depend on B or on its row.  d[b] = NaN where kept[b] < 30.  One
 * workgroup per clip, one launch, no workspace.
 * NSG_E_INVALID: a null pointer, B < 1, Tmax < 1, extended not 0 or 1;  NSG_E_UNSUPPORTED: B * Tmax >= 2^31. */
NSG_API int nsg_audio_stoi_score(const float *env, const int32_t *kept, double *d, int32_t B, int32_t Tmax, int32_t extended,
                                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * F0-conditioned decoder (extension, beside the speaker-conditioned one; not in the reference): the decoder input also gets one
 * row of an F0 table per latent COLUMN, chosen by the quantised log-F0 of the four mel frames the column covers, so the codes
 * need not carry pitch.  parity unpinned: the definitions are this project's own, stated here in full and restated in numpy by
 * tests/helpers/f0_cond_ref.py.  models.VQVAE(n_f0_bins=), train.FusedTrainStep, audio.f0_bins (csrc/f0_cond.hip).
 * None of the four entry points takes a workspace; every launcher checks all of its arguments before it launches anything.
 * ------------------------------------------------------------------------------------------- */

/* The decoder input in one pass, for the latent grid [B][H][W] of C channels:
 *     y[b][h][w][:] = act( (src(b,h,w)[:] + clip_rows[b][:]) + table[bins[b][w]][:] ),     row = (b H + h) W + w
 *   src       idx == NULL: x is the fp32 rows themselves, src = x[row][:]  ([B H W][C]);
 *             idx != NULL: x is a [K][C] fp32 table and src = x[idx[row]][:], idx [B H W] int64 -- a gather (the bf16 training
 *             step never materialises an fp32 z_q);
 *   clip_rows [B][C] fp32 or NULL (then src + table[..]: one add);  table [n_rows][C] fp32;  bins [B][W] int64;
 *   act       identity (relu == 0) or max(., 0);  y [B H W][C] of y_dtype, fp32 or bf16 (round to nearest even).
 * The two adds are fp32 additions in exactly the order written.  A bins value outside [0, n_rows) and an idx value outside [0, K)
 * are CLAMPED into range (compared as the 64-bit values they are), so caller-made bins can never read outside the tables; the
 * Python layers check their ranges on the host where they are given on the module paths.
 * NSG_E_INVALID (message names the entry point): a null x, table, bins or y;  B, H, W, C, n_rows (K with idx) not positive;  an
 * unknown y_dtype;  C not a multiple of 4 (fp32 y) or 8 (bf16 y);  x, clip_rows, table or y not 16-byte aligned, idx or bins not
 * 8-byte aligned;  B H W C, n_rows C or K C not below 2^31. */
NSG_API int nsg_add_cond(const float *x, const int64_t *idx, const float *clip_rows, const float *table, const int64_t *bins, void *y,
                         int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, int32_t n_rows, int32_t relu, int32_t y_dtype,
                         void *stream);

/* The first stage of that add's gradients: out[b][w][:] = sum over h of x[b][h][w][:], x [B][H][W][C] fp32 or bf16, out [B][W][C]
 * fp32.  One thread owns a (b, w, 16-byte channel vector) triple and adds its H values to 0.f in ascending h in fp32: the result
 * is fixed by construction and the same on every call.  The table's gradient is then nsg_index_add_rows* over bins, the clip
 * rows' gradient nsg_clip_colsum of out with rows_per_clip = W.
 * NSG_E_INVALID: a null pointer;  B, H, W or C not positive;  an unknown dtype;  C not a multiple of 4 (fp32) or 8 (bf16);  x or
 * out not 16-byte aligned;  B H W C not below 2^31. */
NSG_API int nsg_column_sum(const void *x, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, float *out, void *stream);

/* An F0 track at the mel frame rate -> one bin per latent column.  f0 [B][T] fp32 Hz, +0.0 on unvoiced frames (as nsg_audio_f0 and
 * nsg_f0_viterbi write it);  frames [B] int32 DEVICE memory or NULL (then T; clamped into [0, T]);  affine [B][3] fp32 rows of
 * (mu_src, ratio, mu_tgt) or NULL;  bins [B][W] int64;  logf [B][W] fp32 or NULL.
 * Latent column w covers frames 4w .. 4w + 3 (the encoder's two stride-2 stages).  Over those of them that are < frames[b] and
 * voiced (f0 > 0), in frame order:  n = their number,  l = (sum of fl32(log2((double)f0)) added to 0.f in fp32) / (float)n.
 *     l' = mu_tgt + (l - mu_src) * ratio      (fp32: the difference, the product, then the sum; l' = l without affine)
 *     u  = ((l' - lo) * (float)n_bins) / span (fp32: the difference, the product, then the quotient), with the launch constants
 *          lo = fl32(log2((double)fmin)), span = fl32(log2((double)fmax)) - lo (an fp32 difference)
 *     the column is voiced iff n >= 2:  bin = 1 + min(max(floor(u), 0), n_bins - 1), logf = l';  otherwise bin = 0, logf = +0.0.
 * (A column needs two voiced frames: a lone voiced frame beside three unvoiced ones is a tracker's onset or octave slip more often
 * than a pitch.)  Every element of bins (and logf) is written; a clip's row depends on its own track and length alone.
 * NSG_E_INVALID: a null f0 or bins;  B, T or W not positive;  T < 4 W;  n_bins < 1;  not 0 < fmin < fmax < inf, or a range whose
 * fp32 span is not positive;  a pointer not aligned to its element (4 bytes; bins 8);  B T not below 2^31. */
NSG_API int nsg_f0_bins(const float *f0, const int32_t *frames, const float *affine, int64_t *bins, float *logf, int32_t B, int32_t T,
                        int32_t W, int32_t n_bins, float fmin, float fmax, void *stream);

/* The same bins for a batch cropped out of a RESIDENT F0 track by nsg_collate_mels' plan -- the rows are never materialised and
 * nothing is tracked per batch (data.ResidentMelCorpus.track_f0 tracks every clip once; F0 frame t is mel frame t).
 * f0_corpus [corpus_frames] fp32 Hz, +0.0 where unvoiced: the clips' tracks concatenated exactly as the mel corpus' frames are;
 * plan [B][3] int64, DEVICE memory: nsg_collate_mels' rows (clip, start, count), clip not read;  affine [B][3] fp32 or NULL, as in
 * nsg_f0_bins;  bins [B][W] int64;  logf [B][W] fp32 or NULL;  f0_out [B][T] fp32 or NULL.
 * With  f_b[t] = f0_corpus[start_b + t]  for t < count_b,   +0.0f  for count_b <= t < T,  the outputs are exactly
 *     nsg_f0_bins(f_b, frames = count_b, affine, ...)   -- bins and logf bit for bit (one column rule serves both kernels) --
 *     f0_out[b][t] = f_b[t].
 * Reads and clamps follow nsg_collate_mels: count_b is clamped into [0, T] and a frame outside [0, corpus_frames) reads as +0.0,
 * so whatever the plan holds no access leaves a buffer.  Every element of bins (and of logf and f0_out where given) is written
 * exactly once; every corpus offset is 64-bit.  One thread per latent column (per four frames of T where f0_out is given), four
 * scalar loads each (start_b + 4w has no alignment); one launch, no workspace.
 * NSG_E_INVALID: a null f0_corpus, plan or bins;  B, T or W not positive;  T < 4 W;  n_bins < 1;  not 0 < fmin < fmax < inf, or a
 * range whose fp32 span is not positive;  corpus_frames < 0;  a pointer not aligned to its element (4 bytes; plan and bins 8);
 * B T not below 2^31.
 * PRECONDITION the entry point cannot check (plan is device memory): nsg_collate_mels'; the caller checks its host copy. */
NSG_API int nsg_collate_f0_bins(const float *f0_corpus, int64_t corpus_frames, const int64_t *plan, const float *affine,
                                int64_t *bins, float *logf, float *f0_out, int32_t B, int32_t T, int32_t W, int32_t n_bins,
                                float fmin, float fmax, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Pitch change that keeps the spectral envelope and the duration: time-domain pitch-synchronous overlap-add, TD-PSOLA (Moulines &
 * Charpentier 1990), driven by an F0 track (extension; not in the reference).  parity unpinned: the definition is this project's
 * own, stated here in full and restated in fp32 and fp64 by tests/helpers/psola_ref.py.  audio.pitch_marks,
 * audio.pitch_shift_psola, audio.perturb_pitch (csrc/psola.hip).  Neither entry point takes a workspace: every intermediate is
 * an output of the caller's; both check all of their arguments before they launch anything.
 * ------------------------------------------------------------------------------------------- */

/* What the two entry points share.  wav [B][L] fp32; clip b has len = lengths[b] samples (lengths int32 DEVICE memory, clamped
 * into [0, L]; NULL: L).  f0_in [B][T] fp32 Hz under nsg_audio_f0's conventions: frame t sits at sample t hop, and a value that
 * is not > 0 (+0.0, a negative number, NaN) means unvoiced.  Sample n belongs to frame  t(n) = min(T - 1, (n + hop / 2) / hop)
 * (integer divisions).  With the launch constants P_min <= P_max, P_u and alpha = alpha_num / alpha_den:
 *     clamp(p)  = P_min where not p >= P_min, P_max where p > P_max, else p
 *     P(n)      = clamp((int) floor((double)sample_rate / (double)f0_in[b][t(n)] + 0.5))   on a voiced frame (the clamp is applied
 *                 to the fp64 value before the conversion, so +inf, 1e30 and 1e-30 Hz give P_min, P_min and P_max)
 *               = clamp(P_u)                                                               on an unvoiced one
 *     G         = P_min - (alpha_num P_min) / alpha_den       the least distance of two marks (P - (alpha_num P) / alpha_den does
 *                                                             not fall as P grows)
 *     K_max     = ceil(L / G)                                 marks a clip can have:  m_k >= k G  and  m_k <= len - 1
 *     H_max     = P_max + (alpha_num P_max) / alpha_den       the greatest distance of two marks
 *     G_s       = max(1, (int) floor((double)G / 4.0 + 0.5))  the least distance of two synthesis marks
 *     J_max     = ceil(L / G_s)                               synthesis marks a clip can have
 * The maximum of x over a range [lo, hi] is the sample with the greatest KEY, an integer comparison with nothing left to a
 * float's corner cases:  key(i) = o(bits(x[i])) << 32 | (0xffffffff - (i - lo)),  o(u) = u ^ 0x80000000 for u < 2^31 (a cleared sign)
 * and ~u otherwise -- the order of the reals on numbers (-0.0 below +0.0), NaNs at the two ends -- so among equal samples the
 * SMALLEST index wins.
 * Shared refusals, before any launch, the message starting with the entry point's name.  NSG_E_INVALID: a null pointer other than
 * lengths;  B, L, T or hop < 1;  sample_rate not finite or not > 0;  P_u < 1;  alpha_num < 0 or alpha_den < 1;  K_max (J_max) below
 * the figure above.  NSG_E_UNSUPPORTED: hop outside [16, 2^20];  P_min < 2, P_min > P_max or P_max > 1024 (nsg_audio_f0's longest
 * lag);  2 alpha_num > alpha_den or alpha_den > 2^20;  B * L, B * K_max or B * J_max >= 2^31, or L > 2^31 - 2^21. */

/* Analysis marks: one per pitch period on voiced stretches, on the waveform's local maxima; every clamp(P_u) samples on unvoiced
 * ones.  Per clip, in order:
 *     len = 0:   no mark.
 *     m_0        = the maximum of x over [0, min(P(0), len) - 1]
 *     from m_k on a voiced frame t(m_k), with P = P(m_k) and d = (alpha_num P) / alpha_den:
 *                  lo = m_k + P - d,  hi = min(m_k + P + d, len - 1);   lo > len - 1: the chain ends;
 *                  m_{k+1} = the maximum of x over [lo, hi]
 *     from m_k on an unvoiced frame:   m_{k+1} = m_k + clamp(P_u);   m_{k+1} > len - 1: the chain ends.
 * No float arithmetic enters a mark beyond P(n).  marks [B][K_max] int32: marks[b][k] = m_k for k < n_marks[b], -1 beyond;
 * n_marks [B] int32.  Every element of both is written exactly once; a clip's marks depend on its own samples, length and track
 * alone: bit for bit independent of B, L, K_max and its row.  One launch, one wave per clip: the clip's neighbourhood (two halves
 * of 4096 samples) and its frames' periods live in LDS, the search is a wave maximum of the keys with lane l owning the samples
 * lo + l, lo + l + 64, ..., and the next half is loaded from global memory while the current range is searched (csrc/psola.hip). */
NSG_API int nsg_audio_pitch_marks(const float *wav, const int32_t *lengths, const float *f0_in, int32_t *marks, int32_t *n_marks,
                                  int32_t B, int32_t L, int32_t T, int32_t hop, float sample_rate, int32_t P_u, int32_t P_min,
                                  int32_t P_max, int32_t alpha_num, int32_t alpha_den, int32_t K_max, void *stream);

/* Synthesis marks and the overlap-add, from the marks above (marks, n_marks: nsg_audio_pitch_marks' outputs for the same wav,
 * lengths, f0_in and constants; K = n_marks[b] clamped into [0, K_max], every mark clamped into [0, len - 1]).  f0_out [B][T] fp32:
 * the track the output is to have.  Per clip:
 *     D_a   = m_{a+1} - m_a for a < K - 1,   D_{K-1} = m_{K-1} - m_{K-2},   D_0 = clamp(P_u) when K = 1      (the LOCAL spacing)
 *     s_0 = m_0,  a(0) = 0;   K = 0: no synthesis mark
 *     r_j   = (double)f0_out[t(s_j)] / (double)f0_in[t(s_j)] when both are > 0, taken into [0.25, 4] (below: 0.25, above: 4, NaN: 1);
 *             otherwise 1
 *     s_{j+1} = s_j + max(1, (int) floor((double)D_{a(j)} / r_j + 0.5));    s_{j+1} > m_{K-1}: the chain ends
 *     a(j+1)  = the a >= a(j) that minimises |m_a - s_{j+1}|, the smaller a on a tie  (the time map is the identity: duration is kept)
 * syn [B][J_max] int32 = s_j, map [B][J_max] int32 = a(j), both -1 for j >= n_syn[b];  n_syn [B] int32.
 * Grain j is x around m_a, a = a(j), under an asymmetric window of left half-length  hl = m_a - m_{a-1}  (0 for a = 0) and right
 * half-length  hr = m_{a+1} - m_a  (0 for a = K - 1): at output sample n, with dist = n - s_j,
 *     dist = 0:            w = 1
 *     -hl < dist < 0:      u = fl((float)(-dist) / (float)hl)
 *     0 < dist < hr:       u = fl((float)dist / (float)hr)         (elsewhere the grain does not reach n)
 *     w = fl(1 - fl(fl(u u) * fl(3 - fl(2 u))))                    (w(u) + w(1 - u) = 1, as for a Hann window; no cosine)
 * and over the grains that reach n, j ascending, both sums fp32 from +0.0, every operation rounded and never contracted:
 *     num = sum fl(w_j * x[m_{a(j)} + dist]),   den = sum w_j
 *     out[n] = fl(num / den)  where den >= 2^-NSG_PSOLA_MIN_WEIGHT_LOG2 = 2^-10,   x[n] elsewhere (so before s_0 and after the last s_j)
 * for n < len, and +0.0 for len <= n < L.  (m_{a-1} < m_a + dist < m_{a+1}: a grain never reads outside the clip.)  With
 * f0_out = f0_in, or with no voiced frame, s = m and a(j) = j: the output is x exactly outside [m_0, m_{K-1}] and at the marks, and
 * x to within the roundings of w, num, den and the quotient between them.  out [B][L] fp32 may not alias wav; every element of
 * syn, map, n_syn and out is written exactly once; a clip's results are bit for bit independent of B, L, K_max, J_max, its row and
 * any tiling.  Two launches: the chain over j, one thread per clip; then a thread per output sample, which finds the first grain
 * that can reach it by a binary search in s (s_j > n - H_max) and walks on while s_j < n + H_max.
 * With marks and counts that are not nsg_audio_pitch_marks' own, the clamps above keep every access inside its buffer and two more
 * rules apply, neither of which binds otherwise:  the chain over j also ends once it holds J_max synthesis marks (n_syn <= J_max);
 * and a grain reaches only |dist| < H_max, so a half-length above H_max (marks further apart than any the analysis makes) is cut
 * there, its window still taken over the full half-length.
 * Refusals: the shared ones, for marks, n_marks, f0_out, syn, map, n_syn and out too. */
#define NSG_PSOLA_MIN_WEIGHT_LOG2 10
NSG_API int nsg_audio_psola(const float *wav, const int32_t *lengths, const float *f0_in, const float *f0_out, const int32_t *marks,
                            const int32_t *n_marks, int32_t *syn, int32_t *map, int32_t *n_syn, float *out, int32_t B, int32_t L,
                            int32_t T, int32_t hop, float sample_rate, int32_t P_u, int32_t P_min, int32_t P_max, int32_t alpha_num,
                            int32_t alpha_den, int32_t K_max, int32_t J_max, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSG_H_ */
