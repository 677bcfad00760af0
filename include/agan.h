/*
 * agan.h -- C ABI of libagan_hip.so, the MI355X (gfx950) kernels under the AttnGAN training hot path.
 *
 * The reference (ku222/Attention-GAN) is pure Python on PyTorch and has no FFI of its own
 * (SURVEY.md §8b); its boundary is the Python module surface (networks/, losses/, utilities/layers.py,
 * trainers/trainer.py).  This header is the layer directly underneath that surface: each entry point
 * names the reference call site whose ATen ops it replaces.  The Python host code in
 * attention-gan_amd/ binds these with ctypes from torch.autograd.Function.forward/backward
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned, contiguous, 16-byte-aligned storage
 *     (NCHW fp32 unless stated); the library never allocates, frees, synchronises or keeps state;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*), so it is graph-capturable;
 *   - return value 0 = ok, negative AGAN_E* otherwise; agan_last_error() gives the message (thread-local);
 *   - "ws" is scratch the caller provides; the *_ws_bytes() function of an op says how much it needs.
 */
#ifndef AGAN_H_
#define AGAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGAN_VERSION 101 /* 0.1.1 */
/* 101 (round 4): agan_words_loss_fwd / agan_sent_loss_fwd carry `labels` after class_ids (added in place during round 3 without a
 * version change: a caller built against the 100 header must be rebuilt -- bind by version, backend/lib.py asserts it);
 * agan_allreduce_bucket_dt + agan_exchange_* (16-bit wire format of the gradient exchange); amax slots of agan_conv_wgrad are
 * needed whenever agan_conv_wgrad_effective_prec says AGAN_PREC_F16X3, which includes AGAN_PREC_BF16X6 callers. */
/* Added within 101 without changing any existing argument list or enum value (a binding written against the earlier 101 header keeps
 * working unchanged): the general 2-D conv (agan_conv2d_*), AGAN_PACK_DGRAD_3x3S2, AGAN_ACT_RELU and the pools / bilinear resize of the
 * Inception-v3 image-encoder trunk (agan_maxpool3s2_*, agan_avgpool3s1_*, agan_global_avgpool_*, agan_resize_bilinear_*, agan_relu_bwd);
 * the embedding gather and the LSTM recurrence of the caption encoder (agan_embedding_*, agan_lstm_*); the train-mode BatchNorm of the
 * trunk on channel slices (agan_bn_relu_slice_fwd, agan_bn_slice_bwd); the trainable general 2-D conv behind Layers.conv
 * (agan_conv2d_train_*: forward, data gradient and weight gradient of any small geometry); the batch preparation from device-resident
 * uint8 shards (agan_image_prep); the two halves of a Lloyd iteration behind the pseudo-caption clustering (agan_kmeans_*); the
 * reductions of a generator's evaluation (agan_moments_*, agan_retrieval_rank; agan_knn_radius, agan_manifold_scan and
 * agan_poly_kernel_sum for precision / recall, density / coverage and the kernel distance; agan_inception_score for the Inception
 * Score's per-split reduction over classifier logits); the sentence-conditioned BatchNorm of the generator's up blocks (agan_cbn_*); the
 * pixel-to-pixel attention of the generator's self-attention block and its gate (agan_self_attn_*, agan_scaled_residual_*); the dynamic
 * memory of the generator's refinement stages (agan_mem_write_*, agan_mem_read_*), for which agan_act_fwd / agan_act_bwd also take
 * AGAN_ACT_RELU; the channel-wise word attention of those stages (agan_chan_attn_*); the word-level
 * discriminator's word-region correlation score (agan_word_corr_*); the spectral normalisation of a discriminator's weights
 * (agan_spectral_*). */

enum {
    AGAN_OK = 0,
    AGAN_EINVAL = -1,    /* bad argument / unsupported shape */
    AGAN_EWORKSPACE = -2,/* workspace too small */
    AGAN_ELAUNCH = -3    /* HIP launch failure */
};

/* arithmetic mode of the MFMA contractions (fp32 storage everywhere, fp32 accumulate always) */
enum {
    AGAN_PREC_F32 = 0,    /* v_mfma_f32_32x32x2_f32: exact fp32 products                                              */
    AGAN_PREC_BF16 = 1,   /* operands rounded to bf16, v_mfma_f32_32x32x16_bf16 (BASELINE configs[1])                 */
    AGAN_PREC_BF16X3 = 2, /* bf16 hi/lo split (16 mantissa bits), 3 MFMAs per product                                 */
    AGAN_PREC_F16 = 3,    /* operands rounded to fp16, v_mfma_f32_32x32x16_f16 (BASELINE configs[4])                  */
    AGAN_PREC_BF16X6 = 4, /* bf16 hi/mid/lo split (24 mantissa bits), 6 MFMAs per product: fp32-grade products at 2.67x
                             the fp32-MFMA rate                                                                       */
    AGAN_PREC_F16X3 = 5   /* fp16 hi/lo split (22 mantissa bits), 3 MFMAs per product, operands scaled by powers of two into
                             fp16's range: fp32-grade products at 5.3x the fp32-MFMA rate.  The gathered operand's scale comes
                             from an amax slot (see agan_absmax below), the weights are packed times 2^11                   */
};
/* A 16-bit mode holds where the patch-resident kernels (csrc/conv_patch.hip) take the geometry: 3x3 / 2x2-per-class stride-1 and 4x4
 * stride-2 geometries with more than 4 input and output channels and images of at least 4x4; any other call (linear layers, the RGB
 * heads) runs in AGAN_PREC_F32 whatever mode is asked for.  Which kernel then runs the call is the conv routing's choice (see "Conv
 * routing" below).  agan_conv_effective_prec says which mode a geometry gets -- pack the weights for THAT precision (declared below,
 * after agan_conv_geom). */

/* Storage type of an ACTIVATION tensor in HBM (round 3).  fp32 is the reference's layout and the default everywhere.  The
 * one-plane 16-bit modes can also keep activations in their operand type -- AGAN_DT_BF16 with AGAN_PREC_BF16, AGAN_DT_F16 with
 * AGAN_PREC_F16 -- through the `*_dt` entry points below: conv outputs, BatchNorm inputs/outputs and their gradients are then
 * rounded ONCE to 16 bits when they are stored, the gathers load 16-bit values without converting, and half the bytes move.
 * BatchNorm statistics, softmax, losses, weight gradients, master weights and the optimiser stay fp32/fp64 in every mode. */
enum { AGAN_DT_F32 = 0, AGAN_DT_BF16 = 1, AGAN_DT_F16 = 2 };

int agan_version(void);
const char* agan_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Gather-convolution geometry.  One descriptor covers every convolution on the path:
 *
 *   out[b, n, y'*OS+py, x'*OS+px] = sum_{c<Cin, r<R, s<S}
 *         in[b, c, y'*SY + r*DY + OY[py], x'*SY + s*DY + OY[px]] * wk[py*OS+px][(c*R + r)*S + s][n]
 *
 * (taps outside [0,IH)x[0,IW) read zero).  OS = 1 is an ordinary strided conv; OS = 2 splits the output
 * into its 4 parity classes, each with its own RxS taps -- which is how a stride-2 transposed conv and a
 * conv over a nearest-x2-upsampled input are expressed WITHOUT zero-insertion / without materialising the
 * upsampled tensor (K3 in SURVEY.md §2.1 never exists in HBM, and costs 4/9 of the 3x3 MACs).
 *
 * wk is the packed weight  [OS*OS][K = Cin*R*S][Nld],  Nld = agan_round_up(Cout, 32), zero padded,
 * produced from the reference's OIHW parameter by agan_pack_weight().
 * ---------------------------------------------------------------------------------------------- */
typedef struct agan_conv_geom {
    int32_t B;
    int32_t Cin, IH, IW;   /* gathered tensor  [B, Cin, IH, IW]  */
    int32_t Cout, OH, OW;  /* produced tensor  [B, Cout, OH, OW] */
    int32_t R, S;          /* taps per class                      */
    int32_t OS;            /* 1 or 2                              */
    int32_t SY, DY;        /* input step per output-lattice step / per tap (same in y and x) */
    int32_t OY[2];         /* input offset for output parity 0 / 1 */
} agan_conv_geom;

/* how agan_pack_weight lays an OIHW tensor out for a given use */
enum {
    AGAN_PACK_FWD = 0,       /* conv KHxKW any stride (layers.py:50-53,122):  wk[(ci,r,s)][co] = w[co][ci][r][s]            */
    AGAN_PACK_DGRAD_S1 = 1,  /* dgrad of a stride-1 'same' conv: wk[(co,r,s)][ci] = w[co][ci][KH-1-r][KW-1-s]              */
    AGAN_PACK_DGRAD_4x4S2 = 2,/* dgrad of conv4x4 s2 p1 as 4 parity classes of 2x2 taps                                     */
    AGAN_PACK_UP_FWD = 3,    /* Upsample(x2 nearest)+conv3x3 (layers.py:64-65) folded into 4 parity classes of 2x2 taps    */
    AGAN_PACK_UP_DGRAD = 4,  /* its dgrad folded into one 4x4 stride-2 conv over dY                                         */
    AGAN_PACK_DGRAD_3x3S2 = 5/* dgrad of conv3x3 s2 p0 (agan_conv2d_dgrad) as 4 parity classes of 2x2 taps, zero-weight padded
                                (class 0: taps {2,0}, class 1: taps {1,-}); fp32 layout only                              */
};

/* Packed size in BYTES for a precision mode: AGAN_PREC_F32 -> fp32 [cls][K][Nld];  the 16-bit modes -> [cls][k-step][plane][Nld][16]
 * (k-step = 16 channels of one tap, ordered chunk of 32 channels > input phase > tap > half; planes = 1 / 2 / 3 for
 * BF16, F16 / BF16X3 / BF16X6): the 32 x 16 operand block of a wave is 1 KB contiguous.  0 = combination not supported. */
size_t agan_packed_weight_bytes(int mode, int cout, int cin, int kh, int kw, int prec);
/* w: OIHW [cout][cin][kh][kw] -> wk (see modes).  Replaces nothing in the reference: layout prep for the kernels below. */
int agan_pack_weight(const float* w, void* wk, int mode, int cout, int cin, int kh, int kw, int prec, void* stream);
/* Many packs in one launch (all jobs of one call share `prec`, i.e. one layout family): what a module re-packs after an optimiser step.  `jobs` is a DEVICE array; job i owns
 * workgroups [first_block, first_block + agan_pack_job_blocks(...)), first_block ascending from 0; total_blocks = their sum.
 * Same layouts as agan_pack_weight, including zeroed padding columns. */
typedef struct agan_pack_job {
    const float* w;
    void* wk;
    int32_t mode, cout, cin, kh, kw, first_block;
} agan_pack_job;
int agan_pack_job_blocks(int mode, int cout, int cin, int kh, int kw);
int agan_pack_job_blocks_prec(int mode, int cout, int cin, int kh, int kw, int prec);   /* ... for a 16-bit layout (prec != AGAN_PREC_F32) */
int agan_pack_weights(const agan_pack_job* jobs, int njobs, int total_blocks, int prec, void* stream);

/* conv forward / dgrad: replaces F.conv2d fwd+dgrad under Layers.conv3x3 / conv4x4 s2 / Upsample+conv3x3 /
 * nn.Linear (1x1 on a 1x1 image) -- utilities/layers.py:50-53,64-65,122,139-150; generator_submodules.py:36,152;
 * discriminators.py:15.   bias may be NULL.  act: AGAN_ACT_NONE, or AGAN_ACT_LRELU to apply the LeakyReLU(0.2) that follows a
 * conv without BatchNorm (layers.py:139-141, first stage of encode_image_by_16times) in the epilogue (fp32 MFMA path only). */
/* Reduction-index table of a geometry (one int32 pair per k = (ci,r,s), padded): build it once per geometry with
 * agan_conv_ktable() into agan_conv_ktable_elems() int32s and pass it to every conv call of that geometry.  It lets the
 * kernels fetch the im2col offsets with scalar loads instead of decoding k with integer divisions. */
size_t agan_conv_ktable_elems(const agan_conv_geom* g);
int agan_conv_ktable(const agan_conv_geom* g, int32_t* table, void* stream);

/* Conv routing.  One function per direction in csrc/conv.hip picks the kernel of a call (route_gather / route_wgrad): the first rule
 * below that takes it.  Every query of this section reads that choice, and the conv entry points run it.
 *   forward / data gradient:
 *     1. one-plane modes (AGAN_PREC_BF16 / F16): the row-block gather (csrc/conv_p16.hip), fp32 or the mode's 16-bit storage on either side;
 *     2. the other 16-bit-mode calls: the patch-resident gather (csrc/conv_patch.hip), fp32 storage;
 *     3. AGAN_PREC_F32 conv3x3 stride 1, conv4x4 stride 2 and its data gradient on enough pixels, fp32 storage, no bias / activation /
 *        mask: Winograd (csrc/conv_wino.hip);
 *     4. <= 4 output channels: the vector-ALU kernels (csrc/conv_small.hip), fp32 output, fp32 or 16-bit input (linear layers: fp32);
 *     5. the k-table MFMA kernel (csrc/conv.hip): fp32 input, fp32 or 16-bit output.
 *   weight gradient (g = the FORWARD geometry):
 *     1. AGAN_PREC_F32 conv3x3 stride 1 on enough pixels, fp32 storage: Winograd;
 *     2. the row-resident kernel (csrc/conv_wgrows.hip) where it takes the geometry, in any mode; fp32 or the one-plane mode's 16-bit storage;
 *     3. the other 16-bit-mode calls: the patch-resident weight gradient, fp32 or the one-plane mode's 16-bit storage;
 *     4. AGAN_PREC_F32 with <= 4 output channels: the vector-ALU kernel, fp32 or 16-bit x, fp32 dy;
 *     5. the k-table MFMA kernel: fp32 storage.
 * agan_conv_gather_dt_supported / agan_conv_wgrad_dt_supported say whether a rule takes the storage types asked for.
 * agan_conv_gather_ws_bytes / agan_conv_wgrad_ws_bytes return the largest workspace among the kernels this geometry can be routed to
 * over every argument the query does not name: gather -- the storage pairs, with and without an epilogue; weight gradient -- every mode,
 * the pack mode the geometry implies (AGAN_PACK_UP_FWD for OS = 2) and the storage pairs. */
int agan_conv_effective_prec(const agan_conv_geom* g, int prec);
/* ... and the one its weight gradient gets (agan_conv_wgrad demotes by itself; a caller needs this to know whether the
 * AGAN_PREC_F16X3 scales are wanted).  g = the FORWARD geometry, pack_mode = AGAN_PACK_FWD or AGAN_PACK_UP_FWD. */
int agan_conv_wgrad_effective_prec(const agan_conv_geom* g, int pack_mode, int prec);
/* Fraction of the direct contraction's multiply-adds that the kernel chosen for this call really issues (measurement aid: bench.py's
 * executed_tflops).  1.0 except where AGAN_PREC_F32 takes a Winograd kernel (csrc/conv_wino.hip): 16/36 for conv3x3 stride 1 (forward,
 * data gradient, weight gradient), 36/64 for the conv4x4 stride-2 forward, 9/16 for its class-wise data gradient.  wgrad != 0: g is the
 * FORWARD geometry of a weight gradient; plain_epilogue = 0: the call carries a bias / activation / mask (the Winograd gathers have none). */
double agan_conv_executed_fraction(const agan_conv_geom* g, int prec, int wgrad, int plain_epilogue);
size_t agan_conv_gather_ws_bytes(const agan_conv_geom* g, int prec);
/* lrelu_mask (optional, data-gradient launches): a tensor of the OUTPUT's shape; out is multiplied by LeakyReLU'(mask) = 1 where
 * mask > 0, else 0.2 -- the backward of the LeakyReLU that produced this conv's forward input (the mask is that input), folded
 * into the epilogue so that the activation's backward needs no pass of its own. */
int agan_conv_gather(const float* in, const void* wk, const float* bias, float* out, const agan_conv_geom* g,
                     const int32_t* ktable, int prec, int act, const float* lrelu_mask, void* ws, size_t ws_bytes, void* stream,
                     const float* in_amax /* AGAN_PREC_F16X3: amax slot of `in`; NULL otherwise */,
                     float* out_amax /* optional: amax slot that receives max|out| (16-bit MFMA paths) */);

/* The same call with typed activation storage: `in` has in_dtype, `out` and `lrelu_mask` have out_dtype (AGAN_DT_*).  16-bit
 * tensors go with the one-plane mode of the same type (AGAN_PREC_BF16 / AGAN_PREC_F16) on the row-block gather, or with the fp32
 * kernels (rules 4 and 5 of the conv routing): agan_conv_gather_dt_supported says so (1 / 0) -- a caller converts around an
 * unsupported layer.
 * With both dtypes AGAN_DT_F32 this IS agan_conv_gather (workspace: agan_conv_gather_ws_bytes in every case). */
int agan_conv_gather_dt_supported(const agan_conv_geom* g, int prec, int in_dtype, int out_dtype);
int agan_conv_gather_dt(const void* in, const void* wk, const float* bias, void* out, const agan_conv_geom* g,
                        const int32_t* ktable, int prec, int act, const void* lrelu_mask, void* ws, size_t ws_bytes, void* stream,
                        const float* in_amax, float* out_amax, int in_dtype, int out_dtype);

/* amax slots (AGAN_PREC_F16X3).  The fp16 split mode scales each gathered operand by the power of two that lands its largest
 * magnitude in (2^12, 2^13]; the kernels derive that scale themselves from an AMAX SLOT: AGAN_AMAX_SLOT floats of device memory,
 * ZEROED by the caller, into which the kernel that PRODUCES a tensor folds max|value| (the `*_amax` arguments of the BatchNorm
 * and conv entry points: no extra pass over the tensor), or which agan_absmax fills for a tensor that has no such producer.
 * Everything stays on the device and on the stream: no host sync, HIP-graph capturable. */
#define AGAN_AMAX_SLOT 256    /* 8 running maxima, each on its own 128-byte line */
int agan_absmax(const float* x, size_t n, float* amax_slot, void* stream);

/* conv weight gradient: x is the forward input, dy the gradient of the forward output, g the FORWARD geometry.
 * Produces dw in OIHW [cout][cin][kh][kw] (pack mode AGAN_PACK_FWD or AGAN_PACK_UP_FWD says how g was built).
 * Replaces the wgrad half of conv2d backward at the same call sites. */
size_t agan_conv_wgrad_ws_bytes(const agan_conv_geom* g);
/* accumulate != 0: dw += gradient (a parameter used twice in one backward, e.g. D on the real and the fake batch). */
/* x_amax / dy_amax: the amax slots of x and dy, REQUIRED whenever agan_conv_wgrad_effective_prec(g, pack_mode, prec) returns
 * AGAN_PREC_F16X3 -- that is prec == AGAN_PREC_F16X3 and also prec == AGAN_PREC_BF16X6, whose weight gradients run as two-plane
 * fp16 splits on the row-resident kernel (csrc/conv_wgrows.hip); NULL in every other mode. */
int agan_conv_wgrad(const float* x, const float* dy, float* dw, const agan_conv_geom* g, const int32_t* ktable, int pack_mode,
                    int kh, int kw, int prec, int accumulate, void* ws, size_t ws_bytes, void* stream,
                    const float* x_amax, const float* dy_amax);

/* the same with typed activation storage (x: x_dtype, dy: dy_dtype; dw stays fp32): 16-bit tensors where
 * agan_conv_wgrad_dt_supported says 1 -- the row-resident and patch weight gradients in the one-plane mode of the same type, and a
 * 16-bit x into the <= 4-output-channel fp32 kernel (rules 2-4 of the conv routing) */
int agan_conv_wgrad_dt_supported(const agan_conv_geom* g, int pack_mode, int prec, int x_dtype, int dy_dtype);
int agan_conv_wgrad_dt(const void* x, const void* dy, float* dw, const agan_conv_geom* g, const int32_t* ktable, int pack_mode,
                       int kh, int kw, int prec, int accumulate, void* ws, size_t ws_bytes, void* stream,
                       const float* x_amax, const float* dy_amax, int x_dtype, int dy_dtype);

/* dbias[n] = sum_{b,y,x} dy[b,n,y,x]  (bias of nn.Linear / outlogits conv: generator_submodules.py:152, discriminators.py:15) */
int agan_bias_grad(const float* dy, float* dbias, int B, int C, int HW, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm + activation (utilities/layers.py:66-67,123-124,143-144,164-174; generator_submodules.py:38)
 * ---------------------------------------------------------------------------------------------- */
enum { AGAN_ACT_NONE = 0, AGAN_ACT_GLU = 1, AGAN_ACT_LRELU = 2, AGAN_ACT_TANH = 3, AGAN_ACT_SIGMOID = 4, AGAN_ACT_RELU = 5 };

/* batch statistics over (B, HW) per channel: mean[C], invstd[C] = 1/sqrt(biased var + eps).  If running_mean is
 * non-NULL also does running = (1-momentum)*running + momentum*stat (unbiased var) and ++*num_batches_tracked. */
size_t agan_bn_stats_ws_bytes(int B, int C, int HW);
int agan_bn_stats(const float* x, int B, int C, int HW, float eps, float* mean, float* invstd,
                  float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                  void* ws, size_t ws_bytes, void* stream);
/* y = act(gamma*(x-mean)*invstd+beta) [+ residual].  GLU halves the channels (out has C/2).  residual may be NULL. */
int agan_bn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    const float* residual, float* out, int B, int C, int HW, int act, void* stream, float* out_amax);
/* Training-mode forward in one call: batch statistics (written to mean/invstd for the backward, folded into the running
 * statistics) + normalise + activation.  Tensors with B*HW <= 8192 per channel run as ONE launch (a workgroup per channel
 * keeps the channel in registers between the two phases); larger ones as agan_bn_stats + agan_bn_act_fwd.
 * groups: the batch axis is `groups` consecutive sub-batches of B/groups samples, each normalised with ITS OWN statistics
 * (mean / invstd are [groups][C]); the running statistics receive one update per group, in batch order.  That is what
 * `groups` separate forward passes through the layer do -- the discriminator's [real; fake] pass (disc_loss.py:55-61) uses 2.
 * Workspace sizes are per group: call the *_ws_bytes functions with B/groups. */
size_t agan_bn_train_fwd_ws_bytes(int B, int C, int HW);
int agan_bn_train_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* out, float* mean,
                      float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, int HW,
                      float eps, float momentum, int act, int groups, void* ws, size_t ws_bytes, void* stream, float* out_amax);
/* backward: dx[B,C,HW], dgamma[C], dbeta[C] from dout (C/2 channels under GLU); gamma/beta gradients are summed over the groups. */
size_t agan_bn_act_bwd_ws_bytes(int B, int C, int HW);
int agan_bn_act_bwd(const float* x, const float* dout, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int act, int accumulate,
                    int groups, void* ws, size_t ws_bytes, void* stream, float* dx_amax);
/* The same three calls with typed activation storage (AGAN_DT_*): x and dx have x_dtype; out, dout and the residual have
 * out_dtype.  Combinations: (F32, F32) = the calls above; (BF16, BF16), (F16, F16); (F32, BF16), (F32, F16) for a layer whose conv
 * ran on an fp32-storage kernel.  Statistics, gamma / beta and their gradients stay fp32 (sums in fp64).  [B, C] inputs
 * (BatchNorm1d) are fp32 only. */
int agan_bn_stats_dt(const void* x, int B, int C, int HW, float eps, float* mean, float* invstd, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, float momentum, void* ws, size_t ws_bytes, void* stream,
                     int x_dtype);
int agan_bn_act_fwd_dt(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                       const void* residual, void* out, int B, int C, int HW, int act, void* stream, float* out_amax, int x_dtype,
                       int out_dtype);
int agan_bn_train_fwd_dt(const void* x, const float* gamma, const float* beta, const void* residual, void* out, float* mean,
                         float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, int HW,
                         float eps, float momentum, int act, int groups, void* ws, size_t ws_bytes, void* stream, float* out_amax,
                         int x_dtype, int out_dtype);
int agan_bn_act_bwd_dt(const void* x, const void* dout, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, void* dx, float* dgamma, float* dbeta, int B, int C, int HW, int act, int accumulate,
                       int groups, void* ws, size_t ws_bytes, void* stream, float* dx_amax, int x_dtype, int out_dtype);
/* plain activations without BN (first D conv + LeakyReLU layers.py:139-140; tanh generator_submodules.py:137; ReLU of the dynamic
 * memory's keys and values): act AGAN_ACT_LRELU, AGAN_ACT_TANH, AGAN_ACT_SIGMOID or AGAN_ACT_RELU (no gradient at exactly 0) */
int agan_act_fwd(const float* x, float* out, size_t n, int act, void* stream);
int agan_act_bwd(const float* out, const float* dout, float* dx, size_t n, int act, void* stream);
/* standalone GLU over channel halves of [B,C,HW] (utilities/layers.py:13-26; the CA-net's "relu", generator_submodules.py:153) */
int agan_glu_fwd(const float* x, float* out, int B, int C, int HW, void* stream);
int agan_glu_bwd(const float* x, const float* dout, float* dx, int B, int C, int HW, void* stream);
/* Launch log of the calling thread's last agan_bn_* / agan_act_* / agan_glu_* call (tests): one code per kernel launch, in launch
 * order, code = kind*100000 + act*10000 + x_dtype*1000 + out_dtype*100 + width.  kind: 1 statistics partial sums, 2 statistics
 * final, 3 statistics of [B, C] rows, 4 forward apply, 5 one-launch small forward, 6 one-launch small backward, 7 backward partial
 * sums, 8 backward final, 9 backward apply, 10 / 11 bare activation forward / backward, 12 / 13 GLU forward / backward.  width: the
 * values per thread and loop step of the sweeping kernels (1, 4, 8), the values per thread of the small kernels (2, 8, 32), else 1
 * (4 for the bare activations).  For the statistics kernels out_dtype repeats x_dtype.  Copies up to `capacity` codes into
 * codes[] and returns how many launches the call made. */
int agan_bn_last_launch(int* codes, int capacity);

/* ------------------------------------------------------------------------------------------------
 * Sentence-conditioned BatchNorm + activation (csrc/cond_bn.hip; backend/functional.py: cond_bn_act; utilities/layers.py:
 * HipCondBatchNorm2d).  Train-mode BatchNorm over (B, HW) per channel as above, with the affine terms per (sample, channel):
 *     xhat[b,c,p] = (x[b,c,p] - mean[c]) * invstd[c]
 *     g[b,c] = gamma[c] + delta[b, c]      t[b,c] = beta[c] + delta[b, C + c]      (delta [B, 2C] fp32, row-major)
 *     z = g * xhat + t        out = z (AGAN_ACT_NONE)  or  z[:, :C/2] * sigmoid(z[:, C/2:]) (AGAN_ACT_GLU, C even)
 * fp32 storage only; any other activation is AGAN_EINVAL.
 *   agan_cbn_train_fwd: the statistics are agan_bn_train_fwd's -- mean, invstd, the running statistics and num_batches_tracked
 *     come out bit for bit as that call writes them for the same x -- followed by ONE apply pass.  With delta = 0 that pass does
 *     the arithmetic of agan_bn_act_fwd.
 *   agan_cbn_act_fwd: the apply pass alone, mean / invstd from the caller (eval mode: the running statistics).
 *   agan_cbn_act_bwd: with dz the gradient at z, S[b,c] = sum_p dz, Q[b,c] = sum_p dz * xhat and n = B * HW,
 *       ddelta[b, c] = Q[b,c]    ddelta[b, C + c] = S[b,c]    dgamma[c] = sum_b Q[b,c]    dbeta[c] = sum_b S[b,c]
 *       c0[c] = sum_b g[b,c] S[b,c] / n    c1[c] = sum_b g[b,c] Q[b,c] / n    dx = invstd[c] * (g[b,c] * dz - c0[c] - xhat * c1[c])
 *     in three passes: the sums per plane (b, c) -- one wave per plane where HW <= 1024, else one workgroup per chunk of a plane --
 *     then one wave per channel adds chunks and samples in index order (ddelta is overwritten; dgamma / dbeta are overwritten, or
 *     added to where `accumulate`), then dx.  Every sum is fp64 in a fixed order, no atomics: two runs give the same bits.
 * Null pointers (out_amax / dx_amax, the running statistics and num_batches_tracked may be NULL), an activation other than NONE /
 * GLU, odd C under GLU, B, C or HW < 1 or B * HW >= 2^31 are AGAN_EINVAL, a workspace below *_ws_bytes AGAN_EWORKSPACE, before any
 * launch (the size queries answer 0 for a dimension < 1).
 *   agan_cbn_last_launch: launch log of the calling thread's last agan_cbn_* call (tests), as agan_bn_last_launch: code =
 *     kind*100000 + act*10000 + width.  kind: 1 statistics of [B, C] rows, 2 one-launch statistics (B * HW <= 8192; width = values
 *     per thread 2, 8, 32), 3 two-pass statistics, 4 forward apply, 5 backward sums by waves, 6 backward sums by workgroups,
 *     7 backward final, 8 backward apply.  width: values per thread and loop step (4 where HW is a multiple of 4, else 1; 1 for
 *     the final).  A statistics entry stands for that path's launches and carries act 0.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_cbn_train_fwd_ws_bytes(int B, int C, int HW);
int agan_cbn_train_fwd(const float* x, const float* gamma, const float* beta, const float* delta, float* out, float* mean,
                       float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, int HW,
                       float eps, float momentum, int act, void* ws, size_t ws_bytes, void* stream, float* out_amax);
int agan_cbn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* delta, float* out, int B, int C, int HW, int act, void* stream, float* out_amax);
size_t agan_cbn_act_bwd_ws_bytes(int B, int C, int HW);
int agan_cbn_act_bwd(const float* x, const float* dout, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, const float* delta, float* dx, float* ddelta, float* dgamma, float* dbeta, int B, int C,
                     int HW, int act, int accumulate, void* ws, size_t ws_bytes, void* stream, float* dx_amax);
int agan_cbn_last_launch(int* codes, int capacity);

/* ------------------------------------------------------------------------------------------------
 * Word-context attention: AttentionModule.forward, networks/attention.py:25-79
 *   proj[b,c,t] = sum_e w[c,e] words[b,e,t]                      (:50-52, conv1x1)
 *   attn[b,t,p] = softmax_t( scale * sum_c images[b,c,p] proj[b,c,t], mask[b,t]==0 -> -inf )   (:59-68)
 *   ctx[b,c,p]  = sum_t proj[b,c,t] attn[b,t,p]                 (:73)
 * T <= 64.  mask is the reference's int64 [B,T].
 * ---------------------------------------------------------------------------------------------- */
int agan_attn_fwd(const float* images, const float* words, const float* w, const int64_t* mask, float scale,
                  float* proj, float* ctx, float* attn, int B, int C, int E, int T, int HW, void* stream);
/* dctx / dattn may be NULL (treated as zero).  Outputs dimages[B,C,HW], dwords[B,E,T], dw[C,E].  No atomics: the projected-word
 * gradient is reduced through per-workgroup slabs in `ws`, so the result is bit-reproducible. */
size_t agan_attn_bwd_ws_bytes(int B, int C, int T, int HW);
int agan_attn_bwd(const float* images, const float* words, const float* w, const float* proj, const float* attn,
                  const float* dctx, const float* dattn, float scale, float* dimages, float* dwords, float* dw,
                  int B, int C, int E, int T, int HW, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* the same two calls with typed activation storage: `images`, `ctx`, `dctx` and `dimages` have `dtype` (AGAN_DT_*); the attention
 * map, the projection and all arithmetic stay fp32 */
int agan_attn_fwd_dt(const void* images, const float* words, const float* w, const int64_t* mask, float scale, float* proj,
                     void* ctx, float* attn, int B, int C, int E, int T, int HW, void* stream, int dtype);
int agan_attn_bwd_dt(const void* images, const float* words, const float* w, const float* proj, const float* attn,
                     const void* dctx, const float* dattn, float scale, void* dimages, float* dwords, float* dw, int B, int C,
                     int E, int T, int HW, int accumulate, void* ws, size_t ws_bytes, void* stream, int dtype);

/* ------------------------------------------------------------------------------------------------
 * DAMSM losses: WordsLoss.get_loss (losses/words_loss.py:29-102, which loops func_attention
 * networks/attention.py:82-120 over captions) and SentenceLoss.get_loss (losses/sentence_loss.py:12-50).
 *   feat [B,D,S] image regions, wemb [B,D,T] words, lens[B] int64, class_ids[B] int64 or NULL.
 * Outputs: loss[1]; sim[B*B] (gamma3-scaled, masked similarity matrix: [image][caption]); attn maps
 * [B(caption)][T][S] of each caption against ITS OWN image (what the reference returns in att_maps).
 * fwd also leaves everything the backward needs in `save` (agan_words_loss_save_elems floats).
 * Rows w >= lens[i] of caption i's attention maps are NOT written (every kernel form leaves them as the
 * caller allocated them; backend/functional.py passes a zero-filled buffer).  dwemb[i][:][w >= lens[i]] is
 * written as 0.
 * Shapes: B in [1,128], D and S in [1,320], T (L) in [1,32]; every entry point, forward and backward,
 * answers AGAN_EINVAL outside them before touching the device (the two size queries answer 0; the
 * save_elems one also sets agan_last_error).  sent loss: B in [1,128], D >= 1;
 * its `save` is dS [B*B], dots [B*B] (<cnn_j, rnn_i> at [j][i]), norms [2B] (|cnn_j|, then |rnn_i|).
 * ---------------------------------------------------------------------------------------------- */
/* standalone func_attention forward (attention.py:82-120): query [B,D,L], context [B,D,S] -> wctx [B,D,L], attn [B,L,S] */
int agan_func_attention_fwd(const float* query, const float* context, float gamma1, float scale, float* wctx, float* attn,
                            int B, int D, int L, int S, void* stream);
/* its backward (plain autograd in the reference): dwctx [B,D,L] / dattn [B,L,S] are the upstream gradients (either may be NULL);
 * writes dquery [B,D,L] and dcontext [B,D,S].  Recomputes the forward of each batch element; no atomics. */
int agan_func_attention_bwd(const float* query, const float* context, const float* dwctx, const float* dattn, float gamma1,
                            float scale, float* dquery, float* dcontext, int B, int D, int L, int S, void* stream);
size_t agan_words_loss_save_elems(int B, int D, int T, int S);
/* labels [B] int64: the CE targets of words_loss.py:98-99 / sentence_loss.py:46-47 (NULL = arange(B), what train.py:104 builds;
 * a label outside [0,B) makes the loss NaN).  class_ids [B] int64 or NULL: same-class pairs masked to -inf. */
int agan_words_loss_fwd(const float* feat, const float* wemb, const int64_t* lens, const int64_t* class_ids, const int64_t* labels,
                        float gamma1, float gamma2, float gamma3, float lambda, float* loss, float* sim, float* attn_maps,
                        float* save, int B, int D, int T, int S, void* stream);
/* backward: dfeat / dwemb are overwritten.  No atomics (bit-reproducible): each (image, caption) pair writes its contribution to a
 * slab in `ws` (agan_words_loss_bwd_ws_bytes: B*B*D*(S+T) floats) and a second pass adds the B slabs of each row in index order. */
size_t agan_words_loss_bwd_ws_bytes(int B, int D, int T, int S);
int agan_words_loss_bwd(const float* feat, const float* wemb, const int64_t* lens, const float* save, const float* dloss,
                        float gamma1, float gamma2, float gamma3, float lambda, float* dfeat, float* dwemb,
                        int B, int D, int T, int S, void* ws, size_t ws_bytes, void* stream);
int agan_sent_loss_fwd(const float* cnn_code, const float* rnn_code, const int64_t* class_ids, const int64_t* labels, float gamma3, float lambda,
                       float eps, float* loss, float* save /* 2*B*B + 2*B floats */, int B, int D, void* stream);
int agan_sent_loss_bwd(const float* cnn_code, const float* rnn_code, const float* save, const float* dloss, float gamma3,
                       float lambda, float eps, float* dcnn, float* drnn, int B, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small fused heads: GAN / KL losses and the CA-net reparametrisation
 *   disc: -mean(log(pr+1e-8)+log(1-pf+1e-8))  losses/disc_loss.py:55-61   (pr = D(x), pf = D(G(z)): probabilities)
 *   gen : -mean(log(pf+1e-8))                 losses/gen_loss.py:45-46
 *   kl  : -0.5*mean(1+lv-mu^2-exp(lv))        losses/KL_loss.py:5-9
 *   reparam: c = eps*exp(0.5*lv)+mu           networks/generator_submodules.py:161-165
 * Each loss kernel also writes d(loss)/d(input) (pointers may be NULL).
 * ---------------------------------------------------------------------------------------------- */
int agan_disc_loss(const float* p_real, const float* p_fake, float* loss, float* dp_real, float* dp_fake, int B, void* stream);
int agan_gen_loss(const float* p_fake, float* loss, float* dp_fake, int B, void* stream);
int agan_kl_loss(const float* mu, const float* logvar, float* loss, float* dmu, float* dlogvar, int n, void* stream);
int agan_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* c, int n, void* stream);
int agan_reparam_bwd(const float* logvar, const float* eps, const float* dc, float* dmu, float* dlogvar, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The text-conditional discriminator head (csrc/cond_join.hip, csrc/heads.hip; backend/functional.py: cond_join, cond_disc_loss;
 * networks/discriminators.py: COND_DNET).  AttnGAN's jointConv is conv3x3 over cat(h, rep(s)) on the 4x4 code; the sentence channels
 * are constant over the map, so
 *     conv3x3(cat(h, rep(s)), W)[n, c, i, j] = conv3x3(h, W[:, :8df])[n, c, i, j] + sum_{t valid at (i, j)} P[n, c, t]
 *     P[n, c, t] = sum_e s[n, e] * W[c, 8df + e, t]
 * with t = 3 (di + 1) + (dj + 1) the tap that reads input (i + di, j + dj), valid iff 0 <= i + di < 4 and 0 <= j + dj < 4.
 * Write S(p)[c, i, j] = sum_{t valid at (i, j)} p[c, t].
 *   agan_cond_join_fwd: yi [k * B, C, 4, 4] is the image term, k consecutive groups of B rows, row n carrying caption n mod B;
 *     p [B, C, 9]; y [(k + wrong) * B, C, 4, 4].  Rows n < k * B: y[n] = yi[n] + S(p[n mod B]), the taps added in ascending t starting
 *     from yi.  With `wrong`, rows k * B + b (b < B): y = yi[b] + S(p[(b + 1) mod B]) -- the FIRST group's images with the next
 *     sample's caption, cyclically.
 *   agan_cond_join_bwd: dyi[n] = dy[n], plus dy[k * B + n] when `wrong` and n < B.  dp[b, c, t] = the sum over the rows that used
 *     caption b -- row b of group 0, then of group 1, ..., then wrong row (b - 1 + B) mod B -- and inside each row over the positions
 *     (i, j) where t is valid, in ascending (i, j): one running sum per tap.  Either output may be NULL (both: nothing is launched).
 * One lane owns one (row, channel); no atomics, one summation order: two runs give the same bits.  Null pointers, B < 1, k < 1,
 * C < 1, (k + 1) * B * C > 2^30, `wrong` with B < 2 and yi / y / dy / dyi off a 16-byte boundary are AGAN_EINVAL before any launch.
 *   agan_cond_disc_loss: pu [2B] = the unconditional scores of [real; fake], pc [3B] = the conditional scores of [real; fake; wrong]:
 *     loss = (m(-log(pu_r+1e-8)) + m(-log(pc_r+1e-8))) / 2 + (m(-log(1-pu_f+1e-8)) + m(-log(1-pc_f+1e-8)) + m(-log(1-pc_w+1e-8))) / 3
 *     with m the mean over B: AttnGAN's weights on the non-saturating terms above.  ONE launch writes the loss and both gradients
 *     (dpu [2B], dpc [3B]; either may be NULL).
 * ---------------------------------------------------------------------------------------------- */
int agan_cond_join_fwd(const float* yi, const float* p, float* y, int B, int k, int C, int wrong, void* stream);
int agan_cond_join_bwd(const float* dy, float* dyi, float* dp, int B, int k, int C, int wrong, void* stream);
int agan_cond_disc_loss(const float* pu, const float* pc, float* loss, float* dpu, float* dpc, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused Adam over one flat parameter buffer (torch.optim.Adam as configured at train.py:78-80:
 * no weight decay, no amsgrad).  grad_scale multiplies the gradient first (1/world_size after a sum all-reduce).
 * step_state: 16 bytes of device memory owned by the optimiser ([0] = int32 step count, advanced by the call; [2],[3] = the
 * bias-correction coefficients it derives) -- device-resident so that a captured HIP graph advances the step on every replay. */
int agan_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, int32_t* step_state, double lr,
                   double beta1, double beta2, double eps, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hook (bench.py `roofline`): agan_timer_arm(start, stop) makes the NEXT agan_conv_gather / agan_conv_wgrad call on
 * this thread record the two HIP events on its launch stream immediately around its main MFMA (or small-N) kernel -- not
 * around the slab-sum / unpack passes a split launch appends.  One-shot; events come from agan_timer_create.
 * ---------------------------------------------------------------------------------------------- */
int agan_timer_create(void** event);
int agan_timer_destroy(void* event);
int agan_timer_arm(void* start, void* stop);
int agan_timer_elapsed_ms(void* start, void* stop, float* ms);
/* The kernel the most recent TIMED call on this thread ran as its main kernel: the demangled symbol exactly as `rocprofv3
 * --kernel-trace --stats` names it (e.g. "void (anonymous namespace)::conv_gather_f32_kernel<128, 128, 2, 2, 0>(float const*, ...)"),
 * copied into name[capacity]; empty if nothing has been timed.  bench.py keys `roofline_by_kernel` with it. */
int agan_timer_last_kernel(char* name, size_t capacity);
/* The split factor of that kernel's launch: its plan's K split (gathers) or pixel split (weight gradients), i.e. how many partial
 * sums per output the pass after it adds up; 1 for an unsplit launch; 0 if nothing has been timed. */
int agan_timer_last_split(void);

static inline int agan_round_up(int v, int m) { return (v + m - 1) / m * m; }

/* ------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange over RCCL (new component: the reference is single-GPU).
 * One communicator per process (one process per GPU).  Rank 0 makes the id and hands its AGAN_COMM_ID_BYTES bytes to every rank out
 * of band (the Python host uses torch.distributed's store); agan_comm_init is collective over all ranks and binds the calling
 * thread's current device.  agan_allreduce_bucket sums `n` floats in place across the ranks on `stream` (reduce-scatter + all-gather
 * when n divides evenly, else one all-reduce call); the 1/world scale is applied by agan_adam_step's grad_scale.
 * RCCL is bound at run time: without a loadable librccl these calls return AGAN_EINVAL and nothing else is affected.
 * ---------------------------------------------------------------------------------------------- */
#define AGAN_COMM_ID_BYTES 128
int agan_comm_unique_id(void* id);
int agan_comm_init(void** comm, int rank, int world, const void* id);
int agan_comm_destroy(void* comm);
int agan_allreduce_bucket(void* comm, float* buf, size_t n, void* stream);
/* The same exchange with a WIRE dtype (SURVEY.md section 8b's `agan_allreduce_bucket(buf, n, dtype, comm, stream)`):
 * AGAN_DT_F32 = the call above; AGAN_DT_BF16 = the bucket travels as bf16 and is ACCUMULATED IN FP32 on arrival:
 * round (agan_exchange_pack_bf16) -> all-to-all of the `world` pieces (grouped send/recv) -> rank-ordered fp32 sum of the pieces a
 * rank owns, rounded once (agan_exchange_sum_bf16) -> all-gather of the sums -> widen (agan_exchange_unpack_bf16):
 *     buf = fp32(bf16(sum_r fp32(bf16(buf_r)))), identical on every rank, half the bytes of the fp32 exchange on every link.
 * n must be a multiple of 4; `scratch` = agan_allreduce_scratch_bytes(n, world, dtype) bytes of device memory (0 for AGAN_DT_F32). */
size_t agan_allreduce_scratch_bytes(size_t n, int world, int wire_dtype);
int agan_allreduce_bucket_dt(void* comm, float* buf, size_t n, int wire_dtype, void* scratch, size_t scratch_bytes, void* stream);
/* The three element-wise passes of the 16-bit wire format on their own (a host that moves the bytes itself -- torch.distributed's
 * all_to_all_single / all_gather_into_tensor in dataparallel.all_reduce_bf16_ -- uses them around its collectives).  16 bytes per
 * lane, HBM-bound.  agan_exchange_wire_elems(n, world) = elements of the wire image: `world` equal pieces, each a multiple of 8
 * elements (piece r = elements [r*per, (r+1)*per) of the zero-padded bucket).  n and per are multiples of 4. */
size_t agan_exchange_wire_elems(size_t n, int world);
int agan_exchange_pack_bf16(const float* g, void* wire, size_t n, size_t n_wire, void* stream);
int agan_exchange_sum_bf16(const void* pieces /* [world][per] bf16, piece r from rank r */, int world, size_t per,
                           void* sum /* [per] bf16 */, void* stream);
int agan_exchange_unpack_bf16(const void* wire, float* g, size_t n, void* stream);
/* the reduce-scatter / all-gather chunk of a bucket of n floats over `world` ranks (rank r owns elements [r*chunk, (r+1)*chunk));
 * 0 = the bucket does not split into 16-byte aligned equal chunks and goes out as one library all-reduce.  Pure host arithmetic. */
size_t agan_allreduce_chunk_elems(size_t n, int world);

/* ------------------------------------------------------------------------------------------------
 * General 2-D convolution (the frozen Inception-v3 image-encoder trunk, reference networks/cnn_encoder.py:65-101): per-axis taps,
 * stride and padding, channel-slice addressing on both sides.  fp32 products and storage in every precision mode
 * (agan_conv2d_effective_prec says AGAN_PREC_F32); runs on the k-table MFMA gather (csrc/conv.hip, conv routing rule 5).
 *
 *   y[b, out_c0 + n, oy, ox] = act(bias[n] + sum_{c<Cin, r<KH, s<KW} x[b, in_c0 + c, oy*SH + r - PH, ox*SW + s - PW] * w[n][c][r][s])
 *
 * x is [B, in_ctot, IH, IW], y is [B, out_ctot, OH, OW] (a branch of a block writes its channel range of the block output).
 * SH, SW in {1, 2}; KH*KW <= 25; 0 <= P < K per axis; OH, OW as F.conv2d computes them.  The data gradient
 *   dx[b, in_c0 + c, ...] (+)= ReLU'(relu_mask) * conv_transpose(dy[b, out_c0 + n, ...])
 * exists for stride 1 (the gather over flipped weights with padding K-1-P) and for 3x3 stride 2 unpadded (4 parity classes of 2x2
 * taps); any other stride-2 data gradient is AGAN_EINVAL.  dgrad = 0 / 1 below selects the direction.
 *   - weights: pack the OIHW weight with agan_pack_weight(mode = agan_conv2d_pack_mode(d, dgrad), prec = AGAN_PREC_F32);
 *   - k-table: agan_conv2d_ktable into agan_conv2d_ktable_elems int32s, once per descriptor and direction;
 *   - act: AGAN_ACT_NONE or AGAN_ACT_RELU (after the bias); bias may be NULL;
 *   - relu_mask (optional, data gradient): a tensor laid out like dx (the forward input, same slice); dx is zeroed where mask <= 0;
 *   - accumulate != 0: dx += gradient (a tensor several branches read: the first writes, the others add, in launch order).
 * ---------------------------------------------------------------------------------------------- */
typedef struct agan_conv2d_desc {
    int32_t B;
    int32_t Cin, IH, IW;          /* forward input  (the channels this conv reads)  */
    int32_t Cout, OH, OW;         /* forward output (the channels this conv writes) */
    int32_t KH, KW, SH, SW, PH, PW;
    int32_t in_c0, in_ctot;       /* x holds in_ctot channels; this conv reads [in_c0, in_c0 + Cin)   */
    int32_t out_c0, out_ctot;     /* y holds out_ctot channels; this conv writes [out_c0, out_c0 + Cout) */
} agan_conv2d_desc;
int agan_conv2d_pack_mode(const agan_conv2d_desc* d, int dgrad);        /* AGAN_PACK_*, or AGAN_EINVAL if no route takes it */
int agan_conv2d_effective_prec(const agan_conv2d_desc* d, int prec);
size_t agan_conv2d_ws_bytes(const agan_conv2d_desc* d, int dgrad);
size_t agan_conv2d_ktable_elems(const agan_conv2d_desc* d, int dgrad);
int agan_conv2d_ktable(const agan_conv2d_desc* d, int dgrad, int32_t* table, void* stream);
int agan_conv2d_fwd(const float* x, const void* wk, const float* bias, float* y, const agan_conv2d_desc* d, const int32_t* ktable, int act,
                    void* ws, size_t ws_bytes, void* stream);
int agan_conv2d_dgrad(const float* dy, const void* wk, float* dx, const agan_conv2d_desc* d, const int32_t* ktable, const float* relu_mask,
                      int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Trainable general 2-D convolution (csrc/conv_any.hip): what `Layers.conv(in_channels, out_channels, in_hw, out_hw)` can return and
 * the tuned kinds above do not take.  Same descriptor and formula as agan_conv2d_fwd (no activation), with all three directions:
 *
 *   y [b, out_c0 + n, oy, ox]   = bias[n] + sum_{c, r, s} x[b, in_c0 + c, oy*SH + r - PH, ox*SW + s - PW] * w[n][c][r][s]
 *   dx[b, in_c0 + c, iy, ix]  (+)= sum over the (n, r, s, oy, ox) whose window position (oy*SH + r - PH, ox*SW + s - PW) is (iy, ix)
 *   dw[n][c][r][s]            (+)= sum_{b, oy, ox} dy[b, out_c0 + n, oy, ox] * x[b, in_c0 + c, oy*SH + r - PH, ox*SW + s - PW]
 *
 * Domain, per axis independently: K in 1..5 (KH*KW <= 25), S in 1..3, P in 0..3 -- P >= K included: an output pixel whose window
 * lies wholly in the padding is the bias (or zero); OH, OW as F.conv2d computes them; channel slices on both sides as above; every
 * tensor below 2^30 elements.  Anything else is AGAN_EINVAL with a message and no launch (agan_conv2d_train_supported: 1 / 0).
 * The existing agan_conv2d_* entry points answer exactly as before.
 *   - fp32 operands and v_mfma_f32_32x32x2_f32 products in EVERY precision mode; no atomics; every split sum is added in index
 *     order, so two runs give the same bits;
 *   - w is the plain OIHW fp32 weight (the call transposes it into its workspace); dw is OIHW fp32; bias may be NULL;
 *   - direction 0 / 1 / 2 = forward / data gradient / weight gradient selects the workspace size; the workspace is 16-byte aligned;
 *   - data gradient: dx pixels no window reaches (a residue class without a tap when K < S, trailing rows / columns when
 *     (I + 2P - K) % S != 0) are written as zero; with accumulate != 0 every pixel gets dx += gradient (those: + 0);
 *   - weight gradient: the range B*OH*OW is cut into agan_conv2d_train_slabs(d) slabs whose partial results go to the workspace and
 *     are added in slab order; accumulate != 0: dw += gradient.  The bias gradient is agan_bias_grad.
 * ---------------------------------------------------------------------------------------------- */
int agan_conv2d_train_supported(const agan_conv2d_desc* d);
int agan_conv2d_train_slabs(const agan_conv2d_desc* d);                 /* slabs of the weight gradient, or AGAN_EINVAL */
size_t agan_conv2d_train_ws_bytes(const agan_conv2d_desc* d, int direction);   /* 0 for a descriptor outside the domain */
int agan_conv2d_train_fwd(const float* x, const float* w, const float* bias, float* y, const agan_conv2d_desc* d, void* ws, size_t ws_bytes,
                          void* stream);
int agan_conv2d_train_dgrad(const float* dy, const float* w, float* dx, const agan_conv2d_desc* d, int accumulate, void* ws, size_t ws_bytes,
                            void* stream);
int agan_conv2d_train_wgrad(const float* x, const float* dy, float* dw, const agan_conv2d_desc* d, int accumulate, void* ws, size_t ws_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pools and resize of the trunk (csrc/pool_resize.hip), NCHW fp32.  Every backward is a gather: each input pixel sums, in a fixed
 * order, the outputs that read it -- no atomics.  relu_mask (optional) is laid out like dx: dx is zeroed where mask <= 0 (the
 * derivative of the ReLU that produced the pool's input); accumulate != 0: dx += gradient.
 *   agan_maxpool3s2_*: 3x3 window, stride 2, no padding, OH = (H-3)/2+1.  Tie-break as torch's: the first maximum in row-major
 *     window order wins, a NaN wins over every number (a later NaN over an earlier one).  The forward writes the window-local argmax
 *     (0..8) as one byte per output pixel ([B, C, OH, OW]) and y into channels [out_c0, out_c0 + C) of a [B, out_ctot, OH, OW] tensor;
 *     the backward reads dy from that slice.
 *   agan_avgpool3s1_*: 3x3 window, stride 1, padding 1, always divided by 9 (count_include_pad).
 *   agan_global_avgpool_*: mean over H*W per (b, c): y [B, C].
 *   agan_resize_bilinear_*: align_corners=False: src = (dst + 0.5) * in / out - 0.5 clamped at 0, upper neighbour clamped to in-1.
 *   agan_relu_bwd: dx (+)= dy * (y > 0) over n elements.
 * ---------------------------------------------------------------------------------------------- */
int agan_maxpool3s2_fwd(const float* x, float* y, uint8_t* argmax, int B, int C, int H, int W, int out_c0, int out_ctot, void* stream);
int agan_maxpool3s2_bwd(const float* dy, const uint8_t* argmax, const float* relu_mask, float* dx, int B, int C, int H, int W, int out_c0,
                        int out_ctot, int accumulate, void* stream);
int agan_avgpool3s1_fwd(const float* x, float* y, int B, int C, int H, int W, void* stream);
int agan_avgpool3s1_bwd(const float* dy, const float* relu_mask, float* dx, int B, int C, int H, int W, int accumulate, void* stream);
int agan_global_avgpool_fwd(const float* x, float* y, int B, int C, int HW, void* stream);
int agan_global_avgpool_bwd(const float* dy, const float* relu_mask, float* dx, int B, int C, int HW, int accumulate, void* stream);
int agan_resize_bilinear_fwd(const float* x, float* y, int B, int C, int IH, int IW, int OH, int OW, void* stream);
int agan_resize_bilinear_bwd(const float* dy, float* dx, int B, int C, int IH, int IW, int OH, int OW, void* stream);
int agan_relu_bwd(const float* y, const float* dy, float* dx, size_t n, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm of the trunk (csrc/bn_slice.hip; CNNEncoder(backend="hip", hip_train=True)): the BatchNorm + ReLU of one conv
 * whose output feeds a channel slice of a block output.  fp32, per-channel sums in fp64 in a fixed order, no atomics.
 *   agan_bn_relu_slice_fwd: x is the contiguous raw conv output [B, C, HW].  Batch mean and biased variance per channel ->
 *     mean[C], invstd[C] = 1/sqrt(var + eps) (for the backward); if running_mean / running_var are non-NULL (together) they are
 *     updated as torch does (running = (1-momentum)*running + momentum*stat, unbiased variance n/(n-1)), and
 *     ++*num_batches_tracked if that is non-NULL.  Writes relu(gamma*(x-mean)*invstd + beta) into channels [out_c0, out_c0 + C) of
 *     a [B, out_ctot, HW] tensor.  B*HW <= 8192 is one launch (no workspace); larger ones agan_bn_stats + an apply pass.
 *   agan_bn_slice_bwd: the batch-statistics data gradient dx = gamma*invstd*(dy - mean(dy) - xhat*mean(dy*xhat)), xhat =
 *     (x-mean)*invstd, with dy read from channels [dout_c0, dout_c0 + C) of a [B, dout_ctot, HW] tensor and dx [B, C, HW]
 *     contiguous.  No activation (the caller masks dy) and no gamma / beta gradients.
 * Both return AGAN_EINVAL before any device work for a missing pointer, B, C or HW < 1, a negative c0 or c0 + C > ctot.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_bn_relu_slice_fwd_ws_bytes(int B, int C, int HW);
int agan_bn_relu_slice_fwd(const float* x, const float* gamma, const float* beta, float* out, int out_c0, int out_ctot, float* mean,
                           float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, int HW,
                           float eps, float momentum, void* ws, size_t ws_bytes, void* stream);
size_t agan_bn_slice_bwd_ws_bytes(int B, int C, int HW);
int agan_bn_slice_bwd(const float* x, const float* dout, int dout_c0, int dout_ctot, const float* mean, const float* invstd,
                      const float* gamma, float* dx, int B, int C, int HW, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Caption encoder (csrc/lstm.hip; networks/rnn_encoder.py, backend="hip"), fp32 in every precision mode.
 *   agan_embedding_fwd: y[b, t, :] = table[ids[b * ids_ld + t], :] for t < T (ids_ld >= T: the caption tensor may be wider than the
 *     longest length).  An id outside [0, V) gives a row of zeros: the table is never read out of bounds.
 *   agan_embedding_bwd: dense dtable [V, E]: each row sums dy over the (b, t) holding its id in ascending b * T + t, rows no position
 *     holds are written 0.  No atomics.
 *   agan_lstm_fwd: one layer, D = 1 or 2 directions (index 1 = reverse), per-direction hidden size H a multiple of 16 in 16..128,
 *     gate order i, f, g, o and torch's nn.LSTM equations from h = c = 0.  xg_d [B, T, 4H] is x W_ih_d^T + b_ih_d (the caller's input
 *     projection), whh_d [4H, H], bhh_d [4H], lens [B] int32 on the device (clamped to 0..T).  Row b runs t = 0 .. len-1 (forward) or
 *     len-1 .. 0 (reverse).  out [B, T, D*H] (direction d in columns d*H ..), 0 at t >= len; hN [B, D*H]: each direction's last h.
 *     gates [D, B, T, 4H] (post-activation) and cells [D, B, T, H] are what agan_lstm_bwd needs: both null when no backward follows.
 *   agan_lstm_bwd: backward through time.  dout [B, T, D*H] and dhN [B, D*H] may be null (zero gradient).  Writes dg_d [B, T, 4H], the
 *     gradient of the gate pre-activations (that of xg_d, and the per-(b, t) terms of b_hh), 0 at t >= len.
 *   agan_lstm_wgrad: dwhh [D, 4H, H] = sum over b, t of dg_d[b, t]^T h_prev, dbhh [D, 4H] = sum of dg_d, in ascending b then t; h_prev
 *     is out at t-1 (forward) / t+1 (reverse), 0 outside the sequence.
 * Every entry returns AGAN_EINVAL with a message for B < 1, T < 1, D outside {1, 2}, an unsupported H or a missing pointer.  One
 * workgroup owns 4 batch rows of one direction for the whole sequence: no inter-workgroup barrier, no atomics, run-to-run identical.
 * ---------------------------------------------------------------------------------------------- */
int agan_embedding_fwd(const int64_t* ids, int ids_ld, const float* table, float* y, int B, int T, int V, int E, void* stream);
int agan_embedding_bwd(const int64_t* ids, int ids_ld, const float* dy, float* dtable, int B, int T, int V, int E, void* stream);
int agan_lstm_fwd(const float* xg0, const float* xg1, const float* whh0, const float* whh1, const float* bhh0, const float* bhh1,
                  const int32_t* lens, float* out, float* hN, float* gates, float* cells, int B, int T, int H, int D, void* stream);
int agan_lstm_bwd(const float* dout, const float* dhN, const float* whh0, const float* whh1, const float* gates, const float* cells,
                  const int32_t* lens, float* dg0, float* dg1, int B, int T, int H, int D, void* stream);
int agan_lstm_wgrad(const float* dg0, const float* dg1, const float* out, float* dwhh, float* dbhh, int B, int T, int H, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batch preparation from device-resident uint8 shards (csrc/batch_prep.hip; data/batches.py: DeviceShardBatches).  A shard's uint8
 * images stay in device memory; ONE launch gathers a batch's rows, mirrors the samples that ask for it and writes the fp32 images in
 * [-1, 1] at up to three resolutions.  `planes` is a HOST array of n_planes (1..3) entries, read before the call returns; rows
 * [B] int32 and flip [B] uint8 are device arrays (rows NULL = 0..B-1, flip NULL = no mirror); every dst is [B, C, H, W] fp32.
 *   Direct plane (src != NULL; plane 0 always is): src is [n_src, C, H, W] uint8 and
 *     dst[b, c, y, x] = (float(src[rows[b], c, y, x']) - 127.5f) / 127.5f,  x' = W-1-x where flip[b], else x
 *     -- bit-identical to the reference's scale_255_to_1 (one IEEE division per pixel, no reciprocal multiply).
 *   Derived plane (src == NULL, plane 1 or 2): resampled from plane 0, whose size must be exactly 2x or 4x this plane's on both axes,
 *     with the antialiased bilinear (triangle) filter of torch.nn.functional.interpolate(mode="bilinear", antialias=True,
 *     align_corners=False): per axis, output o takes taps 2o-1 .. 2o+2 with weights [1 3 3 1] / 8 (factor 2) or 4o-2 .. 4o+5 with
 *     weights [1 3 5 7 7 5 3 1] / 32 (factor 4); taps outside the image are dropped and the rest renormalised by their sum (torch's
 *     float64 CPU result agrees with these weights to 1e-12: tests/test_host_device_batches.py).  The weighted byte sum is an exact
 *     integer num over an integer den, and the output is the single division (2 num - 255 den) / (255 den), every term below 2^24:
 *     the correctly rounded fp32 of the exact value.  The mirror is applied to the source (by the filter's symmetry, the same as
 *     mirroring the result).  Plane 0 may be at most 3072 (factor 4) / 6144 (factor 2) pixels wide for a derived plane.
 *   A rows[b] outside [0, n_src) writes zeros for sample b in every plane and reads nothing (the rule of agan_embedding_fwd).
 * One launch for all planes, no allocation, no synchronisation, no atomics: graph-capturable and run-to-run identical.  AGAN_EINVAL
 * before any launch for n_planes outside 1..3, a plane 0 without src, a derived plane that is not plane 0 / 2 or / 4, a non-positive B,
 * C, H, W or n_src, a missing dst, or a plane of 2^31 elements or more.
 * ---------------------------------------------------------------------------------------------- */
typedef struct agan_image_plane { const uint8_t* src; float* dst; int32_t H, W; } agan_image_plane;
int agan_image_prep(const agan_image_plane* planes /* host array */, int n_planes /* 1..3 */,
                    const int32_t* rows /* device [B], NULL = 0..B-1 */, const uint8_t* flip /* device [B], NULL = none */,
                    int B, int C, int n_src, void* stream);

/* ------------------------------------------------------------------------------------------------
 * k-means for the pseudo-captions (csrc/kmeans.hip; data/captions.py: kmeans, HierarchicalClusterer -- the reference clusters image
 * embeddings with scikit-learn's KMeans, data/bedrooms.py:279-289).  One Lloyd iteration is agan_kmeans_assign + agan_kmeans_update on
 * x [N, D] fp32 row-major and centroids [K, D] fp32.  Domain: N >= 1, 1 <= D <= 4096, 1 <= K <= 4096, N * D < 2^31; tails in N, D and K
 * are handled inside the kernels (a D tail reads as zeros).  Anything else, or a missing pointer, is AGAN_EINVAL with a message before any
 * launch (the *_ws_bytes queries then return 0); a workspace that is too small is AGAN_EWORKSPACE.
 *   agan_kmeans_assign: labels[i] = argmin_c (|c|^2 - 2 x_i.c), the LOWEST c on a tie; dist[i] = max(0, |x_i|^2 + that score).  The
 *     contraction runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, AGAN_PREC_F32's meaning; there is no 16-bit mode) and the running
 *     (min, argmin) stays in registers across the centroid chunks: no N x K matrix exists in memory.  labels is read before it is
 *     written: *n_changed = the number of rows whose new label differs from the value that was there (any value on a first call).
 *     *inertia = the sum of dist in fp64.  Whatever x and the centroids hold (NaN included), every label written lies in [0, K).
 *   agan_kmeans_update: counts[c] = rows with label c; centroids[c] = fp32(fp64 sum of those rows / counts[c]); a cluster without rows
 *     keeps the centroid passed in, bit for bit.  A label outside [0, K) contributes to nothing and is never used as an index.  The rows
 *     are ordered by a stable counting sort on the labels and summed, per cluster, in ascending row order in pieces of 512 rows whose
 *     partial sums are added in piece order: no N x K one-hot matrix.
 * No float atomics anywhere (integer LDS atomics only for the histogram, whose result does not depend on their order); every sum has one
 * fixed order: two runs on the same inputs give the same bits.  Only enqueues on `stream`: no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_kmeans_assign_ws_bytes(int N, int D, int K);
int agan_kmeans_assign(const float* x /* [N, D] */, const float* centroids /* [K, D] */, int32_t* labels /* [N] in: previous, out: new */,
                       float* dist /* [N] */, int32_t* n_changed /* [1] */, double* inertia /* [1] */, int N, int D, int K, void* ws,
                       size_t ws_bytes, void* stream);
size_t agan_kmeans_update_ws_bytes(int N, int D, int K);
int agan_kmeans_update(const float* x /* [N, D] */, const int32_t* labels /* [N] */, float* centroids /* [K, D] in: previous, out: new */,
                       int32_t* counts /* [K] */, int N, int D, int K, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation of a generator (csrc/eval.hip; evaluation.py: FeatureMoments, r_precision, Evaluator).
 *
 * Streaming raw moments of feature rows x [n, D] fp32 row-major, in fp64:
 *   agan_moments_update: sum[j] += sum_k x[k][j]; gram[i][j] += sum_k x[k][i] x[k][j] for j >= i.  The state is the UPPER triangle of
 *     gram [D, D] row-major, diagonal included; what lies below it is unspecified (never read back by agan_moments_finish).  A fresh
 *     state is all zeros; the caller keeps the row count.  fp32 -> fp64 is exact and so is a product of two fp32 values in fp64: only
 *     the additions round.  The contraction runs on v_mfma_f64_16x16x4_f64; each element is owned by one workgroup whose accumulator
 *     starts from gram and walks the rows in ascending order; sum is added in pieces of 512 rows, the pieces in order.
 *   agan_moments_finish: mean = sum / count; cov = (gram - count mean mean^T) / (count - 1), written as a full matrix that is symmetric
 *     bit for bit; count == 1 gives cov = 0.
 *   Domain: n >= 1, 1 <= D <= 4096, n * D < 2^31, 1 <= count < 2^53; tails in n and D are handled inside the kernels.
 *
 * agan_retrieval_rank: s[i][j] = q_i . b_c / max(|q_i| |b_c|, 1e-8) with c = cand[i][j] (the cosine of losses/sentence_loss.py without
 *   gamma3), over GATHERED rows of the bank: no N x M matrix.  rank[i] = #{ j >= 1 : s[i][j] >= s[i][0] } -- column 0 is the match and a
 *   tie counts against it.  scores may be NULL.  Domain: N, M >= 1, 1 <= D <= 4096, 1 <= R <= 1024.  A candidate outside [0, M) cannot
 *   be seen by the host without a synchronisation, so it is checked on the device before it is used as an address: the call still
 *   returns AGAN_OK, rank[i] of every query that holds one is -1 and that candidate's score is NaN; backend/functional.py turns a
 *   negative rank into ValueError.
 *
 * Anything outside the domains, or a missing pointer, is AGAN_EINVAL with a message before any launch (agan_moments_update_ws_bytes then
 * returns 0); a workspace that is too small is AGAN_EWORKSPACE.  No float atomics; every sum has one fixed order: two runs on the same
 * inputs give the same bits.  Only enqueues on `stream`: no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_moments_update_ws_bytes(int n, int D);
int agan_moments_update(const float* x /* [n, D] */, int n, int D, double* sum /* [D] in/out */, double* gram /* [D, D] in/out */,
                        void* ws, size_t ws_bytes, void* stream);
int agan_moments_finish(const double* sum /* [D] */, const double* gram /* [D, D] */, long long count, int D, double* mean /* [D] */,
                        double* cov /* [D, D] */, void* stream);
int agan_retrieval_rank(const float* query /* [N, D] */, const float* bank /* [M, D] */, const int32_t* cand /* [N, R] */, int N, int M,
                        int D, int R, float* scores /* [N, R] or NULL */, int32_t* rank /* [N] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable augmentation of discriminator inputs (csrc/diffaug.hip; augment.py: diffaug_reference; backend/functional.py: diffaug).
 * DiffAugment (Zhao et al. 2020): the same family of random colour, translation and cutout transforms on real and fake images on every
 * pass through a discriminator, differentiated in the generator update.  THIS text defines the transform.
 *
 * x is [N, C, H, W] fp32, 1 <= C <= 4; u is [N, 8] fp32 uniforms in [0, 1), slot 7 reserved; policy is a mask of AGAN_DIFFAUG_*.  int()
 * truncates.  Per sample n, with u0..u6 = u[n][0..6], in this order (a policy bit that is off skips its stage):
 *   COLOR        b = u0 - 0.5, s = 2 u1, c = u2 + 0.5.   v = x + b;  m = mean of v over the C channels of the pixel;  w = s (v - m) + m;
 *                M = mean of w over C, H, W of the sample;  z = c (w - M) + M.  Saturation keeps a pixel's channel mean, so
 *                M = mean(x) + b: one reduction over the input.
 *   TRANSLATION  Sy = int(0.125 H + 0.5), ty = min(int(u3 * (2 Sy + 1)), 2 Sy) - Sy with the product formed in fp32; Sx, tx likewise from
 *                W and u4.  out[y][x] = z[y - ty][x - tx], and 0 where that lies outside the image.
 *   CUTOUT       ch = int(0.5 H + 0.5), oy = min(int(u5 * (H + 1 - ch % 2)), H - ch % 2) (fp32 product); cw, ox likewise from W and u6.
 *                Rows oy - ch/2 <= y < oy - ch/2 + ch (integer ch/2) and the matching columns, clipped to the image, become 0 in the
 *                translated image.
 * The map is linear in x for fixed u; agan_diffaug_bwd is its transpose: g[y][x] = dy[y + ty][x + tx] where that position lies inside
 * the image and is not cut, else 0;  dw = c g + (1 - c) mean_CHW(g);  dx = s dw + (1 - s) mean_C(dw).
 *
 * agan_diffaug_fwd takes its N = n0 + n1 samples from TWO sources -- samples 0..n0-1 from x0, n0..N-1 from x1 (x1 NULL: n1 = 0) -- and
 * writes ONE [N, C, H, W] tensor y: the [real; fake] batch a discriminator reads is produced by the augmentation itself, no
 * concatenation pass.  y must not overlap a source; dx must not overlap dy.
 * Each call is a sum launch (per-sample sums in fp64: workgroup partials go to the workspace and are added in workgroup order; skipped
 * without COLOR, when the forward is a pure masked gather that moves bits unchanged) and an apply launch.  The kernels compute
 * w = fma(s, v, (1 - s) m) and z = fma(c, w, (1 - c) M) (and the transposes alike), so s = 1 and c = 1 are exact identities.  Stores are
 * 16 bytes per lane where W % 4 == 0 and the bases are 16-byte aligned.  No atomics, no allocation, no synchronisation: run-to-run
 * identical and graph-capturable; the workspace's contents on entry do not matter.
 * AGAN_EINVAL with a message before any launch for C outside 1..4, a non-positive size, a missing pointer, a policy outside 0..7 or
 * N * C * H * W >= 2^31 (agan_diffaug_ws_bytes then returns 0); AGAN_EWORKSPACE for a workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
#define AGAN_DIFFAUG_COLOR 1
#define AGAN_DIFFAUG_TRANSLATION 2
#define AGAN_DIFFAUG_CUTOUT 4
size_t agan_diffaug_ws_bytes(int N, int C, int H, int W);
int agan_diffaug_fwd(const float* x0 /* [n0, C, H, W] */, const float* x1 /* [n1, C, H, W] or NULL */, int n0, int n1,
                     const float* u /* [n0 + n1, 8] */, int policy, float* y /* [n0 + n1, C, H, W] */, int C, int H, int W, void* ws,
                     size_t ws_bytes, void* stream);
int agan_diffaug_bwd(const float* dy /* [N, C, H, W] */, const float* u /* [N, 8] */, int policy, float* dx /* [N, C, H, W] */, int N, int C,
                     int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same transform with every stage applied PER SAMPLE with probability p (adaptive discriminator augmentation, Karras et al. 2020;
 * augment.py: diffaug_reference(..., q, p); backend/functional.py: diffaug(..., q, p)).  THIS text defines the gates.
 *
 * q is [N, 4] fp32 uniforms in [0, 1), slot 3 reserved; p points to ONE fp32 in DEVICE memory, read by the kernels when they run (so a
 * captured HIP graph follows a p that other kernels change between replays).  For sample n, stage k (0 = COLOR, 1 = TRANSLATION,
 * 2 = CUTOUT) runs iff its policy bit is set AND q[n][k] < *p, an fp32 compare: q == p is off, *p = NaN gates everything off, *p >= 1
 * gates nothing off.  A stage that is gated off is skipped for that sample exactly as if its policy bit were off for that sample
 * alone: with all three off the sample's bits move unchanged (-0.0 and NaN payloads included); the colour stage is skipped, not run
 * with b = 0, s = c = 1.  agan_diffaug_gated_bwd is the transpose under the same gates.
 * Everything else is as for the ungated entries: the two sources of the forward, the workspace (agan_diffaug_ws_bytes), the 16-byte
 * and the one-pixel access paths, no atomics, no allocation, no synchronisation, graph-capturable.  The workspace's contents on entry
 * do not matter: the partial sums of a sample whose colour gate is off are neither written nor read, and its sum workgroups return
 * before they load anything.  With *p >= 1 the results are the ungated entries' bytes.
 * AGAN_EINVAL before any launch for a null q or p and for everything the ungated entries refuse; AGAN_EWORKSPACE likewise.
 * ---------------------------------------------------------------------------------------------- */
int agan_diffaug_gated_fwd(const float* x0 /* [n0, C, H, W] */, const float* x1 /* [n1, C, H, W] or NULL */, int n0, int n1,
                           const float* u /* [n0 + n1, 8] */, const float* q /* [n0 + n1, 4] */, const float* p /* DEVICE, one fp32 */,
                           int policy, float* y /* [n0 + n1, C, H, W] */, int C, int H, int W, void* ws, size_t ws_bytes, void* stream);
int agan_diffaug_gated_bwd(const float* dy /* [N, C, H, W] */, const float* u /* [N, 8] */, const float* q /* [N, 4] */,
                           const float* p /* DEVICE, one fp32 */, int policy, float* dx /* [N, C, H, W] */, int N, int C, int H, int W,
                           void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The controller of that probability (csrc/ada.hip; augment.py: AdaController, ada_reference; backend/functional.py: ada_observe_,
 * ada_update_).  p follows the overfitting signal r_t = E[sign(D(real) - threshold)]: up while r_t is above a target, down while below.
 *
 * state: 64 bytes of device memory owned by the caller, as int32 words:
 *   [0] signed sum accumulated in the current window      [1] number of scores accumulated in the window
 *   [2] update calls in the window                        [3] adjustments made so far
 *   [4] p as fp32 bits                                    [5] the last r_t as fp32 bits
 *   [6..7] reserved                                       [8 + 2 i], [9 + 2 i] observation slot of discriminator i, i < 4
 * Word 4 IS the p the gated augmentation entries read: hand them state + 4.
 *
 * agan_ada_observe: one workgroup.  WRITES (does not accumulate) slot[0] = #(score > threshold) - #(score < threshold), slot[1] = n.  A NaN
 * counts in n and in neither tally.  Integer arithmetic only: the result does not depend on the order of the reduction.  Every
 * discriminator observes into its own slot, on its own stream; no two streams write one word.
 * agan_ada_update: a one-thread kernel.  It adds every slot i < nslots with slot[1] > 0 into words 0 / 1 and zeroes those slots, then
 * increments word 2.  When word 2 reaches `interval` it clears words 0..2 and, if the window's count is positive, forms in double
 *     r = sum / count;    p = min(max(p + sgn(r - target) * count * rate, 0), p_max),   sgn(0) = 0
 * stores (float)p and (float)r and increments word 3; a window with count == 0 leaves p, r_t and word 3 alone.  No host scalar other
 * than the configuration enters, so a captured HIP graph keeps adapting on replay.
 * Both kernels use plain vector loads and stores and no atomics: run-to-run identical.
 * AGAN_EINVAL before any launch: observe for a null pointer, n < 1 or a NaN threshold; update for a null state, nslots outside 1..4,
 * interval < 1, rate < 0 (or NaN), p_max outside (0, 1] or a NaN target.
 * ---------------------------------------------------------------------------------------------- */
#define AGAN_ADA_STATE_WORDS 16
#define AGAN_ADA_P_WORD 4
#define AGAN_ADA_SLOT_WORD 8
int agan_ada_observe(const float* score /* [n] */, int n, float threshold, int32_t* slot /* 2 words */, void* stream);
int agan_ada_update(int32_t* state /* 16 words */, int nslots, int interval, double target, double rate, double p_max, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometric augmentation of discriminator inputs (csrc/geoaug.hip; augment.py: geometry_matrices_reference, affine_warp_reference,
 * geoaug_reference; backend/functional.py: geometry_matrices, affine_warp): the geometric stages of adaptive discriminator
 * augmentation (Karras et al. 2020) as ONE bilinear affine warp per tensor.  THIS text defines the warp and the matrices.
 *
 * Warp.  x is [N, C, H, W] fp32, 1 <= C <= 4, finite; M is [N, 6] fp32 = (a, b, tx, c, d, ty) per sample, an OUTPUT -> SOURCE map about
 * the image centre cx = (W - 1) / 2, cy = (H - 1) / 2.  For output pixel (oy, ox), every operation in fp32 and rounded on its own:
 *     sx = (a (ox - cx) + b (oy - cy)) + (tx W + cx)        sy = (c (ox - cx) + d (oy - cy)) + (ty H + cy)
 *     x0 = floor(sx), fx = sx - x0;  y0, fy likewise
 *     y[oy][ox] = sum over the taps (y0 + j, x0 + i), j outer and i inner, of  x[tap] * (wy_j * wx_i),   (w_0, w_1) = (1 - f, f)
 * A tap outside the image contributes zero (zero fill, like the translation stage of agan_diffaug_*; no reflection).  The map is
 * linear in x; agan_affine_warp_bwd is its exact transpose and no gradient goes to M.
 * agan_affine_warp_fwd takes its N = n0 + n1 samples from two sources and writes one tensor, as agan_diffaug_fwd does (x1 NULL:
 * n1 = 0); y must not overlap a source.  A thread owns 4 adjacent output pixels in all channels and stores 16 bytes per lane and
 * channel where W % 4 == 0 and y is 16-byte aligned, else one pixel; the taps are dword loads.  It works for ANY finite matrix.
 * agan_affine_warp_bwd is a gather over dy: a thread owns one input pixel, walks the integer bounding box of the outputs that can
 * reach it -- half-extents |inv00| + |inv01| and |inv10| + |inv11| of the inverse linear part, padded by one on every side, each
 * clamped at 32 -- recomputes every candidate's source position with the forward's own arithmetic and adds dy * weight for the tap
 * that lands on its pixel, in row-major candidate order.  It is SPECIFIED for linear parts that shrink no axis below 1/16 (beyond
 * that the clamp drops contributions; a singular matrix gives meaningless numbers, never a fault); dx must not overlap dy.
 * No atomics, no workspace, one fixed summation order: run-to-run identical, graph-capturable; the outputs' contents on entry do
 * not matter.
 *
 * Matrices.  g is [n, 16] fp32 uniforms in [0, 1): slots 0..4 stage values, slots 8..12 stage gates, the rest reserved; geometry is a
 * mask of AGAN_GEOAUG_* (stage order = bit order).  The linear part is the product, LEFT TO RIGHT, of the applied stages' own
 * output -> source maps, 2 x 2 products in fp32:
 *   XFLIP   diag(-1, 1) iff g0 >= 0.5, else nothing
 *   ROT90   k = min(int(4 g1), 3); [[c, -s], [s, c]] with (c, s) from the table (1, 0), (0, 1), (-1, 0), (0, -1) -- no trig
 *   SCALE   s I, s = exp2(0.7 g2 - 0.35)
 *   ROTATE  [[cos t, -sin t], [sin t, cos t]], t = (2 g3 - 1) pi
 *   ANISO   diag(r, 1 / r), r = exp2(0.7 g4 - 0.35)
 * and tx = ty = 0.  With p NULL every stage whose bit is set applies.  With p -- ONE fp32 in DEVICE memory, read when the kernel runs,
 * word AGAN_ADA_P_WORD of the controller's state -- stage k applies iff its bit is set and g[8 + k] < *p (fp32 compare; a NaN p passes
 * nothing).  A stage that does not apply is skipped, not multiplied in: a sample with no stage gets exactly (1, 0, 0, 0, 1, 0), and
 * XFLIP / ROT90 alone give entries exactly in {0, +-1} -- the warp is then the flip / quarter turn of the pixels, bit for bit, on
 * square images.  The bounded uniform log-scales (same standard deviation as the paper's log-normal 0.2) bound the backward's box:
 * at most 7 candidates per axis.  One thread per sample, one launch.
 * AGAN_EINVAL with a message before any launch: a null pointer (p may be NULL), n < 1, geometry outside 0..31; for the warps C outside
 * 1..4, a non-positive size, H or W above 2^24, N * C * H * W >= 2^31.
 * ---------------------------------------------------------------------------------------------- */
#define AGAN_GEOAUG_XFLIP 1
#define AGAN_GEOAUG_ROT90 2
#define AGAN_GEOAUG_SCALE 4
#define AGAN_GEOAUG_ROTATE 8
#define AGAN_GEOAUG_ANISO 16
#define AGAN_GEOAUG_ALL 31
#define AGAN_GEOAUG_UNIFORMS 16
int agan_geoaug_matrix(const float* g /* [n, 16] */, const float* p /* DEVICE, one fp32, or NULL */, int geometry, float* M /* [n, 6] */,
                       int n, void* stream);
int agan_affine_warp_fwd(const float* x0 /* [n0, C, H, W] */, const float* x1 /* [n1, C, H, W] or NULL */, int n0, int n1,
                         const float* M /* [n0 + n1, 6] */, float* y /* [n0 + n1, C, H, W] */, int C, int H, int W, void* stream);
int agan_affine_warp_bwd(const float* dy /* [N, C, H, W] */, const float* M /* [N, 6] */, float* dx /* [N, C, H, W] */, int N, int C, int H,
                         int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exponential moving average of a module's weights (csrc/ema.hip; optim.py: FlatEMA; backend/functional.py: ema_update_, ema_reference).
 * One call updates every segment of a DEVICE-resident table:  dst[i] = fma(omb, src[i] - dst[i], dst[i])  in fp32, src only read.
 * Segment i owns workgroups [first_block, next segment's first_block); the last one runs to total_blocks.  A segment moves 16 bytes per
 * lane where BOTH its pointers are 16-byte aligned (plus a dword tail of n % 4 elements) and one dword per lane otherwise; no float outside
 * [dst, dst + n) is read or written.  src and dst of a segment must not overlap; destinations of different segments must not overlap.
 *
 * agan_ema_plan works on a HOST copy of the table: it checks every segment (both pointers set and 4-byte aligned, n >= 1), fills
 * first_block and returns the launch's total_blocks (> 0), or AGAN_EINVAL with a message.  The caller copies the planned table to the device.
 *
 * state: 16 bytes of device memory owned by the caller ([0] = int32 count of updates so far, advanced by the call; [2] = the fp32 factor
 * the call derives).  A one-thread kernel in front of the update reads t = state[0], forms in double
 *     beta_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay
 * and stores omb = (float)(1 - beta_t): a young average follows the weights closely (beta_0 = 0.1) and settles at `decay`.  No other
 * host-side scalar enters the launch, so a captured HIP graph keeps counting on replay.  Plain loads and stores, no atomics:
 * run-to-run identical.  AGAN_EINVAL before any launch for a null pointer, nseg < 1, total_blocks < nseg or decay outside (0, 1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct agan_ema_seg {
    const float* src;
    float* dst;
    int64_t n;
    int32_t first_block, reserved;
} agan_ema_seg;
int agan_ema_plan(agan_ema_seg* segs /* HOST, nseg entries */, int nseg);
int agan_ema_update(const agan_ema_seg* table /* DEVICE */, int nseg, int total_blocks, int32_t* state, double decay, int warmup, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reductions over the pairwise geometry of two feature sets (csrc/manifold.hip; evaluation.py: manifold_metrics -- improved precision
 * and recall, Kynkaanniemi et al. 2019, density and coverage, Naeem et al. 2020 -- and kernel_distance -- KID, Binkowski et al. 2018).
 * Rows are fp32, row-major, D wide.  One contraction skeleton on v_mfma_f32_32x32x2_f32 (exact fp32 products; there is no 16-bit mode)
 * carries all three: a workgroup owns 128 query rows and walks the reference rows in chunks of 128, the scores stay in the accumulator
 * registers and each entry's reduction is the epilogue: no n x m matrix exists in memory.  Where the blocks of query rows alone would
 * not fill the chip the references are split into ranges of whole chunks over a second grid dimension (a function of the shape alone);
 * the workgroups' partial results go through the workspace and a small pass merges them by the same rules.
 *   d2(q, r) = max(0, |q|^2 + |r|^2 - 2 q.r), in fp32: the squared norms from a pass of their own, the dot product from the MFMA chain,
 *   then one addition and one fused multiply-add.  The raw-norm form cancels when the rows share a large common offset: callers
 *   translate both sets first (evaluation.manifold_metrics does).
 *   agan_knn_radius: rad2[i] = the k-th smallest d2(x_i, x_j) over j != i.  The row itself is left out BY INDEX, so a duplicate row at
 *     distance 0 counts as a neighbour (the published "(k + 1)-th smallest including self").  Every lane keeps the 8 smallest values of
 *     its rows in registers; the partial lists of a row are merged as multisets, so the result does not depend on the tiling.
 *     Domain: 1 <= k <= 8, n >= k + 1, 1 <= D <= 4096, n * D < 2^31.
 *   agan_manifold_scan: count[i] = #{ j : d2(q_i, ref_j) <= rad2[j] }; near_d2[i] = min_j d2(q_i, ref_j) and near_idx[i] the LOWEST j
 *     that attains it.  rad2 may be NULL: then nothing is counted and count is written as 0.  Domain: m, n >= 1, 1 <= D <= 4096,
 *     m * D < 2^31, n * D < 2^31.
 *   agan_poly_kernel_sum: *out = sum_ij ((x_i . y_j) / D + 1)^3, without the terms i == j when exclude_diagonal is set (the caller then
 *     passes y == x; n != m is refused).  The dot product is the fp32 MFMA's and is converted to fp64 after it; quotient, sum, cube and
 *     every addition are fp64.  Each workgroup leaves one fp64 partial in the workspace and a one-workgroup pass adds them in a fixed
 *     order.  Domain: n, m >= 1, 1 <= D <= 4096, n * D < 2^31, m * D < 2^31.
 * Tails in rows and D are handled inside the kernels (a D tail reads as zeros).  No address depends on feature data: non-finite
 * features may give meaningless numbers, never a fault.  Anything outside the domains, or a missing pointer, is AGAN_EINVAL with a
 * message before any launch (the *_ws_bytes queries then return 0); a workspace that is too small is AGAN_EWORKSPACE.  No atomics; every
 * sum has one fixed order: two runs on the same inputs give the same bits.  Only enqueues on `stream`: no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_knn_radius_ws_bytes(int n, int D, int k);
int agan_knn_radius(const float* x /* [n, D] */, int n, int D, int k, float* rad2 /* [n] */, void* ws, size_t ws_bytes, void* stream);
size_t agan_manifold_scan_ws_bytes(int m, int n, int D);
int agan_manifold_scan(const float* q /* [m, D] */, const float* ref /* [n, D] */, const float* rad2 /* [n] or NULL */, int m, int n, int D,
                       int32_t* count /* [m] */, float* near_d2 /* [m] */, int32_t* near_idx /* [m] */, void* ws, size_t ws_bytes,
                       void* stream);
size_t agan_poly_kernel_sum_ws_bytes(int n, int m, int D);
int agan_poly_kernel_sum(const float* x /* [n, D] */, const float* y /* [m, D] */, int n, int m, int D, int exclude_diagonal,
                         double* out /* [1] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Inception Score's reduction over classifier logits (csrc/iscore.hip; evaluation.py: inception_score -- Salimans et al. 2016).
 * logits [N, C] are fp32, row-major.  Split s of `splits` covers rows [s N / splits, (s + 1) N / splits) (integer division: the
 * contiguous chunks of the published protocol), n_s of them.  In fp64 throughout (fp32 -> fp64 on load is exact; every exp, log,
 * product and addition after it is fp64):
 *   m_k = max_y l[k][y];  lse_k = m_k + log sum_y exp(l[k][y] - m_k);  logp = l[k][y] - lse_k;  p = exp(logp)
 *   Hc_s = -(1 / n_s) sum_k sum_y p logp            (a term with p == 0 counts as 0; logp is never log(p))
 *   q_s[y] = (1 / n_s) sum_k p[k][y];  Hm_s = -sum_y q log q            (a term with q == 0 counts as 0)
 *   IS_s = exp(Hm_s - Hc_s) = exp(mean_k KL(p(.|x_k) || q_s))
 *   scores[s] = { IS_s, Hm_s (label entropy: diversity), Hc_s (conditional entropy: sharpness) }.
 * The logits are read twice and nothing of size N x C is stored: a row pass (one wave per row, the row in registers) leaves lse_k and
 * sum_y p logp per row in the workspace; a column pass recomputes p and leaves one fp64 partial of q per (split, piece of 64 rows
 * counted from the split's first row, class); a pass per class adds the pieces in order and a one-workgroup pass per split adds the
 * class terms and the row terms through a fixed tree.  No atomics; every sum has one fixed order that does not depend on the launch
 * geometry: two runs give the same bits, a split's numbers depend on its own rows only, and the same rows passed alone with
 * splits = 1 give the same bits.  A class whose logit is -inf contributes 0.  A row that holds +inf or a NaN, or nothing but -inf,
 * makes the three numbers of its own split NaN and leaves every other split alone; no address depends on the data.
 * Domain: N >= 1, 1 <= C <= 4096, N * C < 2^31, 1 <= splits <= min(N, 1024) (no split is empty).  Anything else, or a missing
 * pointer, is AGAN_EINVAL with a message before any launch (agan_inception_score_ws_bytes then returns 0); a workspace that is too
 * small is AGAN_EWORKSPACE.  Only enqueues on `stream`: no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_inception_score_ws_bytes(int N, int C, int splits);
int agan_inception_score(const float* logits /* [N, C] */, int N, int C, int splits, double* scores /* [splits, 3] */,
                         void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Self-attention over the positions of a feature map (csrc/self_attn.hip; utilities/layers.py: SelfAttention2d).  fp32.
 * Per sample b, with N query positions and M key positions:
 *     s[n, m] = scale * sum_d q[b, d, n] * k[b, d, m]                 q [B, Dk, N]   k [B, Dk, M]
 *     p[n, :] = softmax_m s[n, :]        lse[b, n] = log sum_m exp s[n, m]          lse [B, N] contiguous
 *     o[b, e, n] = sum_m v[b, e, m] * p[n, m]                          v [B, Dv, M]   o [B, Dv, N]
 * and for the backward, with do the gradient at o:
 *     delta[n] = sum_e do[e, n] o[e, n]     dp[n, m] = sum_e do[e, n] v[e, m]     ds[n, m] = p[n, m] (dp[n, m] - delta[n])
 *     dq[d, n] = scale sum_m ds[n, m] k[d, m]     dk[d, m] = scale sum_n ds[n, m] q[d, n]     dv[e, m] = sum_n p[n, m] do[e, n]
 * Every operand but lse carries its own batch stride in ELEMENTS (*_bs); inside a sample its channel rows are contiguous with row
 * stride N (q, o, do, dq) or M (k, v, dk, dv).  q, k and v may therefore be channel ranges of one [B, 2 Dk + Dv, N] tensor, and dq,
 * dk, dv channel ranges of one gradient tensor of that shape.
 * Nothing of size N x M is written to memory: the forward runs an online softmax (scores beyond +-88 do not overflow) and writes o
 * and lse once; the backward recomputes p from lse in two kernels -- one whose workgroups each own a block of keys and sweep the
 * queries (dk, dv), one whose workgroups each own a block of queries and sweep the keys (dq) -- after a small pass for delta (the
 * workspace holds it).  Every output element is written once by one workgroup in a fixed order: no atomics, no hand-off between
 * workgroups, two runs give the same bits.  A key past M contributes exactly 0.
 * Domain: B, N, M >= 1, 1 <= Dk <= 64, 1 <= Dv <= 128, B * N * max(Dk, Dv) and B * M * max(Dk, Dv) below 2^31, every batch stride at
 * least rows x row length, a finite scale.  Anything else, or a null pointer, is AGAN_EINVAL with the entry's name in
 * agan_last_error(); a workspace below agan_self_attn_bwd_ws_bytes is AGAN_EWORKSPACE; both before any HIP call (the size query
 * answers 0 for a refused shape).  Only enqueues on `stream`: no allocation, no synchronisation.
 *   agan_self_attn_last_launch: launch log of the calling thread's last agan_self_attn_* / agan_scaled_residual_* call (tests), as
 *     agan_cbn_last_launch: code = kind*100000 + block*100 + dk_tiles*10 + dv_tiles.  kind: 1 forward, 2 delta pass, 3 backward dk / dv,
 *     4 backward dq, 5 gate forward, 6 gate backward, 7 gate backward final.  block = positions a workgroup owns (32, 64 or 128: the
 *     largest whose LDS fits and that gives 256 workgroups, else 32); dk_tiles / dv_tiles = 32-row accumulator tiles along Dk (1, 2)
 *     and Dv (1, 2, 4) of the kernel form, 0 where the kernel has none.
 *
 * The block's gate: out = x + g[0] * y over n elements, g read on the device (two roundings, as the torch statement).
 *   agan_scaled_residual_bwd: dy = g[0] * dout; dg[0] = (accumulate ? dg[0] : 0) + sum dout * y, fp64 products summed per workgroup
 *     and then over the workgroups, both in one fixed order.  The gradient at x is dout itself.
 * n < 1 or a null pointer is AGAN_EINVAL, a short workspace AGAN_EWORKSPACE (agan_scaled_residual_bwd_ws_bytes(0) is 0).
 * ---------------------------------------------------------------------------------------------- */
int agan_self_attn_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int M, int Dk, int Dv,
                       long long q_bs, long long k_bs, long long v_bs, long long o_bs, float scale, void* stream);
size_t agan_self_attn_bwd_ws_bytes(int B, int N, int M, int Dk, int Dv);
int agan_self_attn_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dout, float* dq,
                       float* dk, float* dv, int B, int N, int M, int Dk, int Dv, long long q_bs, long long k_bs, long long v_bs,
                       long long o_bs, long long do_bs, long long dq_bs, long long dk_bs, long long dv_bs, float scale, void* ws,
                       size_t ws_bytes, void* stream);
int agan_self_attn_last_launch(int* codes, int capacity);
int agan_scaled_residual_fwd(const float* x, const float* y, const float* g, float* out, size_t n, void* stream);
size_t agan_scaled_residual_bwd_ws_bytes(size_t n);
int agan_scaled_residual_bwd(const float* dout, const float* y, const float* g, float* dy, float* dg, size_t n, int accumulate, void* ws,
                             size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Dynamic memory of a refinement stage (csrc/memory.hip; networks/memory.py: DynamicMemory; DM-GAN, Zhu et al., CVPR 2019).  fp32.
 * Write, per sample b and word t, with U [B, T, Md + 1] the word projection and Q [B, Md + 1] the projection of the mean image feature:
 *     g = sigmoid(U[b, t, Md] + Q[b, Md])          m[b, t, d] = relu(U[b, t, d]) g + relu(Q[b, d]) (1 - g)        m [B, T, Md]
 *   agan_mem_write_bwd: dm -> dU, dQ (ReLU passes no gradient at exactly 0); dQ sums over the words in word order inside one
 *     workgroup per sample.  One launch per direction.
 * Read and respond, per pixel p of h [B, C, HW], with kv [B, T, 2C] (k = kv[:, :, :C], v = kv[:, :, C:]), mask int64 [B, T]
 * (0 = ignore the word), rw [2C] and rb [1]:
 *     s[t] = sum_c k[b, t, c] h[b, c, p], -inf where mask[b, t] == 0      attn[b, t, p] = softmax_t s      o[c] = sum_t v[b, t, c] attn[b, t, p]
 *     z = sum_c (rw[c] h[b, c, p] + rw[C + c] o[c]) + rb[0]      g_r = sigmoid(z)      r[c] = h[b, c, p] (1 - g_r) + g_r o[c]
 *     x[b, c, p] = x[b, C + c, p] = r[c]                              x [B, 2C, HW]   attn [B, T, HW]
 *   One pass: h is read once, both halves of x and attn are written once.  A sample whose words are all masked gives NaN.
 *   agan_mem_read_bwd: from dx [B, 2C, HW] (dr = dx[:, :C] + dx[:, C:]) and the optional dattn [B, T, HW] (NULL = zero) to dh [B, C, HW],
 *     dkv [B, T, 2C], drw [2C] and drb [1].  Nothing but attn is kept from the forward: o and g_r are recomputed.  `mask` is not read (a
 *     masked word has attn = 0 and takes no gradient).  accumulate_rw / accumulate_rb != 0: the sums are ADDED to drw / drb (the
 *     parameter is used again in one backward; agan_attn_bwd's convention).  Every sum over pixels and samples goes through one partial
 *     slab per workgroup of 256 pixels in `ws` and an ordered reduce: no float atomics, two runs give the same bits.
 * Domain: B, T, Md, C, HW >= 1, T <= 64, C <= 64, B <= 65535, B * T * (Md + 1), B * 2C * HW and B * T * HW below 2^31.  Anything else, or
 * a null pointer (dattn excepted), is AGAN_EINVAL with the entry's name in agan_last_error() before any HIP call
 * (agan_mem_read_bwd_ws_bytes then answers 0); a workspace below agan_mem_read_bwd_ws_bytes is AGAN_EWORKSPACE.  Only enqueues on
 * `stream`: no allocation, no synchronisation; graph-capturable.
 * ---------------------------------------------------------------------------------------------- */
int agan_mem_write_fwd(const float* U, const float* Q, float* m, int B, int T, int Md, void* stream);
int agan_mem_write_bwd(const float* U, const float* Q, const float* dm, float* dU, float* dQ, int B, int T, int Md, void* stream);
int agan_mem_read_fwd(const float* h, const float* kv, const int64_t* mask, const float* rw, const float* rb, float* x, float* attn,
                      int B, int C, int T, int HW, void* stream);
size_t agan_mem_read_bwd_ws_bytes(int B, int C, int T, int HW);
int agan_mem_read_bwd(const float* h, const float* kv, const int64_t* mask, const float* rw, const float* rb, const float* attn,
                      const float* dx, const float* dattn, float* dh, float* dkv, float* drw, float* drb, int B, int C, int T, int HW,
                      int accumulate_rw, int accumulate_rb, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Channel-wise word attention of a refinement stage (csrc/chan_attn.hip; networks/attention.py: ChannelAttention; ControlGAN, Li et
 * al., NeurIPS 2019).  fp32.  Every CHANNEL of h [B, C, HW] attends over the words, seen through wt [B, T, HW] (the perception layer's
 * output, one HW-long row per word), with mask int64 [B, T] (0 = ignore the word) and p a pixel:
 *     m[b, c, t] = scale * sum_p h[b, c, p] wt[b, t, p], -inf for a masked word      alpha[b, c, :] = softmax_t m[b, c, :]
 *     f[b, c, p] = sum_t alpha[b, c, t] wt[b, t, p]                                  alpha [B, C, T]   f [B, C, HW]
 *   Three launches: the scores on the fp32 matrix cores, one partial [C, T] slab per workgroup of 256 pixels in `ws`; the ordered sum
 *   of the slabs with the softmax; the read, one pixel per lane.  A sample whose words are all masked gives NaN.
 *   agan_chan_attn_bwd: from df [B, C, HW] and the optional dalpha_out [B, C, T] (NULL = zero; the gradient at the returned alpha) to
 *     dalpha[b, c, t] = sum_p df[b, c, p] wt[b, t, p] (+ dalpha_out)        dm = alpha * (dalpha - sum_t alpha dalpha)
 *     dh[b, c, p] = scale * sum_t dm[b, c, t] wt[b, t, p]                   dwt[b, t, p] = sum_c (alpha[b, c, t] df[b, c, p] + scale dm[b, c, t] h[b, c, p])
 *   Three launches of the same forms.  One of dh and dwt may be NULL: that gradient is then neither computed nor stored.  `mask` is
 *   not read (a masked word has alpha = 0 and takes no gradient).  No float atomics: two runs give the same bits.
 * Domain: B, C, T, HW >= 1, C <= 64, T <= 64, B <= 65535, B * C * HW and B * T * HW below 2^31.  Anything else, or a null pointer
 * (dalpha_out and one of dh / dwt excepted), is AGAN_EINVAL with the entry's name in agan_last_error() before any HIP call (the
 * workspace queries then answer 0); a workspace below agan_chan_attn_{fwd,bwd}_ws_bytes is AGAN_EWORKSPACE.  Only enqueues on
 * `stream`: no allocation, no synchronisation; graph-capturable.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_chan_attn_fwd_ws_bytes(int B, int C, int T, int HW);
int agan_chan_attn_fwd(const float* h, const float* wt, const int64_t* mask, float scale, float* alpha, float* f, int B, int C, int T,
                       int HW, void* ws, size_t ws_bytes, void* stream);
size_t agan_chan_attn_bwd_ws_bytes(int B, int C, int T, int HW);
int agan_chan_attn_bwd(const float* h, const float* wt, const float* alpha, const float* df, const float* dalpha_out, float scale,
                       float* dh, float* dwt, int B, int C, int T, int HW, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Word-level discriminator score (csrc/word_corr.hip; networks/discriminators.py: WordLevelDisc; ControlGAN, Li et al., NeurIPS
 * 2019, section 3.2).  fp32.
 *   regions [B, D, S]: the image regions after the perception layer.  words [B, D, T].  lens [B] int64 on the device.
 *   shift, an integer in [0, B); gamma1, gamma2, eps.
 * Image b is paired with caption c = (b + shift) mod B: shift = 0 gives the matching pairs, shift = 1 the cyclic mismatched pairs
 * that ConditionalDiscLoss already uses.  With L = min(lens[c], T), w_l = words[c, :, l] for l < L and n_s = regions[b, :, s]:
 *     m[l, s]     = <w_l, n_s>
 *     sbar[l, s]  = softmax over l of m[., s]                  (over the L words)
 *     alpha[l, s] = softmax over s of gamma1 * sbar[l, .]      (over the S regions)
 *     ctx_l       = sum_s alpha[l, s] n_s
 *     r_l         = <ctx_l, w_l> / max(|ctx_l| |w_l|, eps)     (WordsLoss.cosine_similarity's clamp)
 *     g_l         = softmax over l of <mean_k w_k, w_l>        (word-level self-attention, mean over the L words)
 *     p_b         = sum_l g_l * sigmoid(gamma2 * r_l)
 * m, sbar, alpha and ctx are func_attention as above, without its 1 / sqrt(D).  One departure from the paper and its released code,
 * where the self-attention weight multiplies ctx_l BEFORE the cosine: the cosine is scale-invariant, so there the weight cancels;
 * here it weights word l's term of the pooled score.  p_b lies in (0, 1) because the weights sum to 1.
 *   Outputs: p [B]; r [B, T] and g [B, T], written as 0 for l >= L.  words[c, :, l >= L] is never read.  lens[c] <= 0 gives p_b = 0.
 *   agan_word_corr_fwd also leaves the per-word statistics the backward needs in `save` (agan_word_corr_save_elems floats).
 *   agan_word_corr_bwd: dregions [B, D, S] from dp [B] only.  The words are constants (the text encoder is frozen in the GAN step, and
 *   g depends on nothing else).  It recomputes m, alpha and ctx from `regions`; every image is in exactly one pair, so dregions[b] has
 *   one owner: no atomics, no workspace (agan_word_corr_bwd_ws_bytes answers 0; `ws` may be NULL), the same bits every run.
 * One launch per direction, one workgroup per pair, every contraction on the fp32 matrix cores; `lens` is read on the device: no
 * host synchronisation, no allocation, graph-capturable.
 * Domain (the DAMSM entries'): B in [1, 128], D and S in [1, 320], T in [1, 32], shift in [0, B).  Outside it, or with a null pointer,
 * every entry answers AGAN_EINVAL before touching the device; the size queries answer 0 and set agan_last_error().
 * ---------------------------------------------------------------------------------------------- */
size_t agan_word_corr_save_elems(int B, int D, int T, int S);
int agan_word_corr_fwd(const float* regions, const float* words, const int64_t* lens, int shift, float gamma1, float gamma2, float eps,
                       float* p, float* r, float* g, float* save, int B, int D, int T, int S, void* stream);
size_t agan_word_corr_bwd_ws_bytes(int B, int D, int T, int S);
int agan_word_corr_bwd(const float* regions, const float* words, const int64_t* lens, int shift, const float* save, const float* dp,
                       float gamma1, float gamma2, float eps, float* dregions, int B, int D, int T, int S, void* ws, size_t ws_bytes,
                       void* stream);

/* ----------------------------------------------------------------------------------------------
 * Spectral normalisation of a weight (csrc/spectral.hip; utilities/layers.py: HipConv2d / HipLinear(spectral=True); Miyato et al.,
 * ICLR 2018).  fp32 in every precision mode.
 * W is a weight seen as a matrix [Cout, K], K = Cin * kh * kw, row-major as the parameter lies.  W may consist of TWO COLUMN SEGMENTS
 * [Cout, K0 | K1] held in two separate contiguous tensors (w0 [Cout, K0], w1 [Cout, K1]: the conditional head's joint conv); K1 = 0
 * is the ordinary case, and w1 / wsn1 / dwsn1 / dw1 are then not read.  The state is u [Cout] and v [K], both unit vectors.
 * eps = 1e-12.
 *   agan_spectral_fwd with iterate = 1 (a training-mode forward) computes, exactly like torch.nn.utils.spectral_norm with one power
 *   iteration:
 *       v  = W^T u / max(|W^T u|, eps)
 *       t  = W v
 *       u' = t / max(|t|, eps)
 *       sigma = <u', W v>            (= |t|)
 *       W_sn  = W / sigma
 *   and writes u' to u_out, v to v_out (they may be u and v themselves: the state stored back), sigma to sigma[0] and W_sn to
 *   wsn0 (and wsn1).  `v` is not read.
 *   With iterate = 0 (an eval-mode forward) u and v are left alone, sigma = <u, W v>; u_out and v_out are not written (may be NULL).
 *   agan_spectral_bwd treats u and v as constants, as torch does.  From dW_sn, the W_sn, sigma and the (u', v) of ITS forward (u, v with
 *   iterate = 0):
 *       c  = <dW_sn, W_sn>           (over the whole matrix, both segments)
 *       dW = (dW_sn - c * u' v^T) / sigma
 *   dW is written into dw0 (dw1), or added to it where accumulate0 (accumulate1) is non-zero: the accumulate-flag convention of
 *   agan_attn_bwd, one flag per segment because the two are separate parameters.
 *   W = 0 gives 0 / 0 as it does in torch: outside the domain.
 * Forms: at most 8192 weights run one workgroup and one launch per direction, without a workspace; above that the forward is four
 * launches (three with iterate = 0) and the backward two, every sum over rows or columns through per-workgroup partials in `ws` and
 * a fixed-order final sum.  No float atomics: two runs give the same bits.  agan_spectral_last_launch fills codes[0..3] with the form
 * of the calling thread's last forward (1 small, 2 big), its slabs and column chunks, and the form of its last backward; returns 4.
 * Domain: Cout >= 1, K0 >= 1, K1 >= 0, Cout * (K0 + K1) < 2^31, iterate 0 or 1.  Anything else, or a null pointer, is AGAN_EINVAL with
 * the entry's name in agan_last_error() before any HIP call (the workspace queries then answer 0); a workspace below
 * agan_spectral_{fwd,bwd}_ws_bytes is AGAN_EWORKSPACE.  Only enqueues on `stream`: no allocation, no host read; graph-capturable.
 * ---------------------------------------------------------------------------------------------- */
size_t agan_spectral_fwd_ws_bytes(int cout, int k0, int k1);
int agan_spectral_fwd(const float* w0, const float* w1, const float* u, const float* v, float* u_out, float* v_out, float* sigma,
                      float* wsn0, float* wsn1, int cout, int k0, int k1, int iterate, void* ws, size_t ws_bytes, void* stream);
size_t agan_spectral_bwd_ws_bytes(int cout, int k0, int k1);
int agan_spectral_bwd(const float* dwsn0, const float* dwsn1, const float* wsn0, const float* wsn1, const float* u, const float* v,
                      const float* sigma, float* dw0, float* dw1, int cout, int k0, int k1, int accumulate0, int accumulate1, void* ws,
                      size_t ws_bytes, void* stream);
int agan_spectral_last_launch(int* codes, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* AGAN_H_ */
