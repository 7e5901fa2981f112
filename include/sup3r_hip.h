/* sup3r_hip.h — C-ABI of libsup3r_hip.so, the MI355X (gfx950) compute core
 * for NREL/sup3r's Sup3rGan hot path.
 *
 * The reference has NO native/FFI seam: its hot path is a Python loop over
 * keras layer objects inside TensorFlow.  This header defines the boundary a
 * sup3r maintainer binds with ctypes.  Each entry point names
 * the reference interface it replaces (paths relative to the sup3r repo).
 *
 * Conventions
 *  - plain C: opaque handles, raw device/host pointers, sizes; no torch types.
 *  - every call returns 0 on success or a negative S3_E* code; the message is
 *    retrievable with s3_last_error().  No exceptions cross the ABI.
 *  - tensors are channels-last fp32, always described 5-D (N, s1, s2, t, C);
 *    4-D (spatial) nets use t = 1.  Device pointers are caller-owned unless
 *    stated otherwise; all work is enqueued on the context's HIP stream.
 *  - a context is used by one host thread at a time (one process per GPU).
 */
#ifndef SUP3R_HIP_H
#define SUP3R_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3_OK 0
#define S3_EINVAL (-1)   /* bad argument / unsupported op description */
#define S3_EHIP (-2)     /* HIP runtime error */
#define S3_ENOMEM (-3)
#define S3_ERCCL (-4)
#define S3_ESTATE (-5)   /* call sequence error (e.g. backward w/o forward) */
#define S3_ETIMEOUT (-6) /* s3_comm_wait: the device work (collectives) did not finish in time */

/* op kinds of the fused plan (sup3r_amd/spec.py lowers the reference's
 * hidden_layers JSON — sup3r/configs/<family>/<model>.json — to these) */
enum {
  S3_OP_CONV = 1,     /* [virtual pad] + conv + bias + act + residual + d2s  */
  S3_OP_REPEAT_T = 2, /* SpatioTemporalExpansion temporal nearest            */
  S3_OP_D2S = 3,      /* depth_to_space (DCR) on (s1, s2)                    */
  S3_OP_ACT = 4,
  S3_OP_ADD = 5,      /* SkipConnection end / Sup3rAdder                     */
  S3_OP_CONCAT = 6,   /* Sup3rConcat                                         */
  S3_OP_DENSE = 7,
  S3_OP_PAD = 8,      /* FlexiblePadding not consumed by a conv              */
  S3_OP_CROP = 9,
  S3_OP_VIEW = 10,    /* Flatten / depth_to_time reshape (alias, no copy)    */
  S3_OP_ROLL_T = 11,  /* tf.roll along t (depth_to_time t_roll)              */
  S3_OP_DILATE = 12   /* zero insertion by stride[] (strided ConvNDTranspose) */
};
enum { S3_ACT_NONE = 0, S3_ACT_RELU = 1, S3_ACT_LEAKY = 2 };
enum { S3_PAD_ZERO = 0, S3_PAD_REFLECT = 1 };
/* arithmetic mode of the MFMA convolution kernels */
enum {
  S3_PREC_F32 = 0,   /* v_mfma_f32_16x16x4_f32: exact fp32 (parity mode)     */
  S3_PREC_BF16 = 1,  /* v_mfma_f32_16x16x32_bf16, fp32 accumulate            */
  S3_PREC_BF16X3 = 2 /* 3-term bf16 split (hi*hi + hi*lo + lo*hi), ~fp32     */
};
enum { S3_LOSS_MAE = 0, S3_LOSS_MSE = 1, S3_LOSS_EXP = 2 };
enum { S3_BUF_W = 0, S3_BUF_G = 1, S3_BUF_M = 2, S3_BUF_V = 3 };

typedef struct s3_ctx s3_ctx;
typedef struct s3_params s3_params;
typedef struct s3_plan s3_plan;

typedef struct {
  int64_t dims[5]; /* N, s1, s2, t, C */
} s3_tensor_desc;

typedef struct {
  int32_t kind;
  int32_t in0, in1, res, out; /* tensor ids, -1 = none                      */
  int32_t w, b;               /* parameter ids, -1 = none                   */
  int32_t k[3], stride[3], lo[3], hi[3]; /* conv / pad / crop geometry      */
  int32_t pad_mode;
  int32_t act;
  float alpha;
  int32_t d2s; /* depth-to-space block fused at the conv store (1 = none)  */
  int32_t rep; /* REPEAT_T factor / ROLL_T shift                           */
  int32_t bcast_c; /* ADD: in1 has one channel, broadcast over C           */
  int32_t reserved[4];
} s3_op_desc;

/* ---- context ----------------------------------------------------------
 * replaces: tf.device(default_device) placement in
 * sup3r/models/abstract.py:41-42,1230 and base.py:104-106.
 * stream: the hipStream_t all work is enqueued on — one the caller already
 * owns (e.g. torch.cuda.current_stream().cuda_stream; NULL is the device's
 * default stream).  create_stream != 0 ignores `stream` and creates a private
 * non-blocking stream instead. */
int s3_ctx_create(int device_id, void* stream, int create_stream, s3_ctx** out);
void s3_ctx_destroy(s3_ctx* ctx);
const char* s3_last_error(const s3_ctx* ctx);
int s3_ctx_sync(s3_ctx* ctx);
void* s3_ctx_stream(s3_ctx* ctx);
/* launch counters of run-time kernel choices the plan cannot report up front
 * (tests assert the path they mean to exercise was taken); -1 for an unknown
 * counter */
enum { S3_STAT_PERSIST_DGRAD = 0, /* trunk data gradients on the persistent kernel */
       S3_STAT_GCONV_SPLITK = 1,  /* gather-MFMA launches with a split contraction  */
       S3_STAT_BUCKET_ELEMS = 2,  /* gradient elements all-reduced bucket by bucket  */
       S3_STAT_DGRAD_C2_SLIDE = 3, /* first-layer data gradients on the sliding kernel */
       S3_STAT_BUCKETS = 4,       /* bucket collectives issued under backward passes */
       S3_STAT_ALLREDUCES = 5,    /* whole-buffer / scalar all-reduces issued        */
       /* support passes of the training step (kernels_reduce / _pointwise / _fold.hip), one per kernel launched */
       S3_STAT_BIAS_STAGE1 = 6,     /* bias gradient: one channel per lane (bias_grad_stage1)   */
       S3_STAT_BIAS_STAGE1_V4 = 7,  /* bias gradient: four channels per lane (bias_grad_stage1_v4) */
       S3_STAT_BIAS_COLS = 8,       /* bias gradient: > 256 channels, one serial walk per channel */
       S3_STAT_BIAS_COLS_SPLIT = 9, /* bias gradient: > 256 channels, rows split over blockIdx.y */
       S3_STAT_BIAS_PARTIAL = 10,   /* stage 2 over riding channel sums, launched at once       */
       S3_STAT_BIAS_PARTIAL_RIDE = 11, /* ... deferred, run inside a weight-gradient reduction  */
       S3_STAT_BIAS_PARTIAL_FLUSH = 12, /* ... deferred, launched on its own when nothing took it */
       S3_STAT_EPI_GENERIC = 13,    /* mask pass: one element per lane (conv_epilogue_bwd_kernel) */
       S3_STAT_EPI_C4 = 14,         /* mask pass: four channels per lane, no store permutation  */
       S3_STAT_EPI_D2S4 = 15,       /* mask pass: four channels per lane, depth-to-space walk   */
       S3_STAT_EPI_C4_BSUM = 16,    /* ... of EPI_C4, those with riding channel sums            */
       S3_STAT_EPI_D2S4_BSUM = 17,  /* ... of EPI_D2S4, those with riding channel sums          */
       S3_STAT_FOLD_GATHER = 18,    /* adjoint of a gather op, one element per lane             */
       S3_STAT_FOLD_PAD4 = 19,      /* fold of an fp32 frame, four channels per lane            */
       S3_STAT_FOLD_PAD4_FR16 = 20, /* fold of a bf16 frame, four channels per lane             */
       S3_STAT_FOLD16X8 = 21,       /* fold of a bf16 frame, eight channels per lane            */
       S3_STAT_FOLD_PLAIN = 22,     /* frame folds (the three above) with no mask               */
       S3_STAT_FOLD_MASKED = 23,    /* ... with the producer's activation adjoint fused         */
       S3_STAT_FOLD_ADD = 24,       /* ... added to an earlier gradient contribution            */
       S3_STAT_AXPY = 25,           /* skip accumulation, one element per lane                  */
       S3_STAT_AXPY4 = 26,          /* skip accumulation, four elements per lane                */
       S3_STAT_PERSIST_SKIPPRE = 27, /* trunk convs whose skip rows load under the last taps   */
       /* in-family variants of the discriminator's conv kernels that s3_plan_op_info does not tell apart */
       S3_STAT_HALO_S2_K64 = 28,    /* stride-2 LDS-halo forwards on the 64-channel split kernel */
       S3_STAT_FEWCH_HALO = 29,     /* few-channel forwards on the LDS-halo kernel (not the gather walk) */
       S3_STAT_FEWCH_HALO_SIGNS = 30, /* ... of those, the ones that wrote activation sign bytes   */
       S3_STAT_DGRAD_S2_O16 = 31,   /* stride-2 data gradients that stored dx as bf16 only        */
       S3_STAT_DGRAD_S2_MB = 32,    /* ... of those, the ones that masked from sign bytes         */
       /* variants of the hi-res tail conv: s3_plan_op_info reports tail_mfma / tail for all of them */
       S3_STAT_TAIL_TILE = 33,      /* forward: conv_tail_mfma_kernel<false> (4 x 8 x 64 tiles)   */
       S3_STAT_TAIL_BAND = 34,      /* forward: conv_tail_mfma_kernel<true> (banded rows, C_out 2) */
       S3_STAT_TAIL_SLIDE = 35,     /* forward: conv_tail_slide_kernel (16 x 64 column along s0)  */
       S3_STAT_TAIL_SWEEP = 36,     /* forward: conv_tail_sweep_kernel (plane sweep)              */
       S3_STAT_TAIL_X3 = 37,        /* forward: conv_tail_x3_kernel (split bf16)                  */
       S3_STAT_WGRAD_TAIL_TILE = 38,      /* weight gradient: conv_wgrad_tail_kernel<false> (fp32 cells) */
       S3_STAT_WGRAD_TAIL_TILE_IN16 = 39, /* weight gradient: conv_wgrad_tail_kernel<true> (bf16 cells)  */
       S3_STAT_WGRAD_TAIL_SWEEP = 40,     /* weight gradient: conv_wgrad_tail_sweep_kernel               */
       S3_STAT_COUNT = 41 };
int64_t s3_ctx_stat(const s3_ctx* ctx, int which);

/* ---- parameter store ---------------------------------------------------
 * replaces: phygnn.CustomNetwork.weights (list of tf.Variable: kernel, bias
 * per layer in layer order — sup3r/models/abstract.py:312-319,
 * base.py:226-235,388-392), the gradient list of tape.gradient
 * (abstract.py:1237) and the keras Adam slot variables
 * (abstract.py:566-587).  One store per network; four flat fp32 device
 * buffers (weights, grads, Adam m, Adam v) so that the optimizer step and the
 * gradient all-reduce are ONE launch / ONE collective.
 * Kernels are stored in canonical [taps..., C_in, C_out] layout (== keras
 * Conv layout; Conv2DTranspose is flipped/transposed by the host shim). */
int s3_params_create(s3_ctx* ctx, int n, const int64_t* sizes, s3_params** out);
void s3_params_destroy(s3_params* p);
int64_t s3_params_total(const s3_params* p);
int s3_params_set(s3_params* p, int which, int idx, const float* host);
int s3_params_get(s3_params* p, int which, int idx, float* host);
void* s3_params_dptr(s3_params* p, int which, int idx);
int s3_params_zero_grad(s3_params* p);
/* counter that changes whenever the weights change (set, Adam step,
 * broadcast): lets a caller reuse a forward result — Sup3rGan._train_batch
 * runs D(hi_res_true) in the generator step and again, with the SAME
 * discriminator weights, in the discriminator step (base.py:1001-1025) */
uint64_t s3_params_version(const s3_params* p);
/* mean(|x|) of one Adam slot / weight tensor (history columns
 * OptmGen/Adam/m/..., abstract.py:582-586) */
int s3_params_mean_abs(s3_params* p, int which, int idx, float* host_out);

/* keras-2.15 Adam.update_step on the whole store (abstract.py:899,912):
 * alpha = lr*sqrt(1-b2^t)/(1-b1^t); m += (g-m)(1-b1); v += (g*g-v)(1-b2);
 * w -= m*alpha/(sqrt(v)+eps).  t is the 1-based step count. */
int s3_adam_step(s3_params* p, float lr, float beta1, float beta2, float eps,
                 int64_t t);
/* The other keras optimizers ``init_optimizer`` may be handed by name
 * (abstract.py:321-350, models/utilities.py:150-158), keras-2.15
 * ``update_step`` each, one fused pass over the store (slots: BUF_M / BUF_V).
 * hp[] (doubles, cast like keras casts its Python scalars: 1 - beta in double,
 * then fp32): Adam {lr, beta_1, beta_2, epsilon}; SGD {lr, momentum, nesterov};
 * RMSprop {lr, rho, momentum, epsilon} (centered=False); Adagrad {lr,
 * epsilon, initial_accumulator_value}; Adamax {lr, beta_1, beta_2, epsilon};
 * AdamW {lr, beta_1, beta_2, epsilon, weight_decay}. */
typedef enum {
  S3_OPT_ADAM = 0, S3_OPT_SGD = 1, S3_OPT_RMSPROP = 2, S3_OPT_ADAGRAD = 3,
  S3_OPT_ADAMAX = 4, S3_OPT_ADAMW = 5
} s3_optimizer_kind;
int s3_optimizer_step(s3_params* p, int kind, const double* hp, int n_hp,
                      int64_t t);
/* The same step in two halves, for a captured graph (below): `stage` writes
 * the scalars of step t (alpha(t) of Adam, ...) to the device with a 1-thread
 * launch and is called OUTSIDE the graph before every replay; `step_staged`
 * is the update launch, reading them from there — identical every step, so it
 * can be recorded.  (Adagrad's step 1 fills the accumulator: run it with
 * s3_optimizer_step.)  `touch` tells the host side that the weights changed
 * behind its back (after a replay): packed filter images are stale. */
int s3_optimizer_stage(s3_params* p, int kind, const double* hp, int n_hp,
                       int64_t t);
int s3_optimizer_step_staged(s3_params* p, int kind);
int s3_params_touch(s3_params* p);

/* ---- captured steps ----------------------------------------------------------
 * A launch-bound training step — the reference's own CPU-runnable case
 * (tests/training/test_train_gan.py:45-114, batch 15 of 5 x 5 -> 10 x 10) is
 * ~650 launches of a few microseconds — recorded once as a hipGraph and
 * replayed with ONE launch per Sup3rGan._train_batch (base.py:944-1031).
 * Between begin and end every launch of the context is recorded instead of
 * executed.  The caller guarantees what a replay needs: every buffer the step
 * touches stays alive and in place (inputs are copied INTO the recorded input
 * buffers), no host read-back / collective / plan creation inside, the
 * optimizer steps staged.  A call that cannot be recorded fails capture_end
 * (S3_EHIP); s3_capture_abort drops a capture after an error. */
typedef struct s3_graph s3_graph;
int s3_capture_begin(s3_ctx* ctx);
int s3_capture_end(s3_ctx* ctx, s3_graph** out);
int s3_capture_abort(s3_ctx* ctx);
int s3_graph_launch(s3_graph* g);
int64_t s3_graph_nodes(const s3_graph* g);
void s3_graph_destroy(s3_graph* g);

/* ---- options ---------------------------------------------------------------
 * Kernel-selection switches (the A/B comparisons of the parity tests, the
 * profiling ablations) are options of a context and of the plans created from
 * it, not process environment: `NO_PERSIST`, `NO_WGRAD_BF16`, `MFMA_TILE`,
 * `HALO32_MIN_TILES`, ... (s3_option_name_at enumerates them; DESIGN.md §5.4
 * says what each one does).  An option is unset (the default behaviour) or
 * carries an int32.  s3_ctx_create reads the variables SUP3R_AMD_<NAME> ONCE
 * as the initial defaults of that context; nothing reads the environment
 * afterwards.  A plan snapshots the context's options when it is created,
 * overridden by the `options` of s3_plan_create_opt; the snapshot governs
 * that plan's forward / backward launches. */
#define S3_OPTION_UNSET INT32_MIN
typedef struct {
  int32_t n;                  /* number of (name, value) pairs */
  const char* const* names;   /* "NO_PERSIST" (or "SUP3R_AMD_NO_PERSIST") */
  const int32_t* values;      /* S3_OPTION_UNSET removes the option */
} s3_plan_options;
int s3_ctx_set_option(s3_ctx* ctx, const char* name, int32_t value);
/* returns 1 if the option is set (value written), 0 if unset, < 0 unknown */
int s3_ctx_get_option(const s3_ctx* ctx, const char* name, int32_t* value);
/* option names, index 0 .. until NULL */
const char* s3_option_name_at(int index);

/* ---- plan (shape-specialised executor) ---------------------------------
 * replaces: the eager/graph layer loops AbstractSingleModel._tf_generate
 * (abstract.py:1131-1173) and Sup3rGan._tf_discriminate (base.py:283-313).
 * inputs[]: tensor ids fed by the caller at forward time (low_res first, then
 * hi-res exo tensors in Sup3rConcat/Sup3rAdder layer order).
 * training != 0 keeps every activation for s3_plan_backward. */
int s3_plan_create(s3_ctx* ctx, s3_params* params, const s3_tensor_desc* tensors,
                   int n_tensors, const s3_op_desc* ops, int n_ops,
                   const int32_t* inputs, int n_inputs, int32_t output,
                   int precision, int training, s3_plan** out);
/* the same with per-plan options on top of the context's (NULL = none) */
int s3_plan_create_opt(s3_ctx* ctx, s3_params* params, const s3_tensor_desc* tensors,
                       int n_tensors, const s3_op_desc* ops, int n_ops,
                       const int32_t* inputs, int n_inputs, int32_t output,
                       int precision, int training, const s3_plan_options* options,
                       s3_plan** out);
void s3_plan_destroy(s3_plan* plan);
/* inputs: device pointers (fp32, NDHWC) in the order given at creation;
 * output: device pointer receiving the result, or NULL to leave it in the
 * plan's own buffer (s3_plan_tensor). */
int s3_plan_forward(s3_plan* plan, const void* const* inputs, void* output);
/* The chunk executor's forward (ForwardPass._run_generator + the hr_crop_slice
 * of forward_pass.py:384-425 + un_norm_output, abstract.py:243-275) in one
 * pass: the plan's LAST convolution computes only the window [lo, lo + n) of
 * its output positions per axis (the chunk without its halo), applies
 * y * scale[c] + shift[c] (affine_dev: device pointer to scale[n_c] then
 * shift[n_c], two roundings like numpy; NULL = none) and writes the dense
 * (N, n0, n1, n2, C) window to `output`.  No full-size model output exists and
 * the halo positions of the last conv are never computed.  Supported
 * (s3_plan_supports_window == 1) for inference plans whose last op is the
 * bf16-input MFMA tail conv; S3_EINVAL otherwise — the caller then runs
 * s3_plan_forward + s3_chunk_epilogue. */
int s3_plan_supports_window(const s3_plan* plan);
int s3_plan_forward_window(s3_plan* plan, const void* const* inputs, void* output,
                           const int64_t* lo3, const int64_t* n3,
                           const float* affine_dev, int n_c);
/* reverse-mode pass of the last forward (tf.GradientTape().gradient,
 * abstract.py:1230-1237).  d_output: dL/d(output); d_input: nullable, receives
 * dL/d(inputs[0]).  accumulate_wgrad != 0 adds into the grad buffer (the
 * discriminator sees true and generated batches).  need_wgrad == 0 skips
 * weight gradients (generator step: only dgrad flows through the disc). */
int s3_plan_backward(s3_plan* plan, const void* d_output, void* d_input,
                     int need_wgrad, int accumulate_wgrad);
void* s3_plan_tensor(s3_plan* plan, int32_t tensor_id);
int64_t s3_plan_workspace_bytes(const s3_plan* plan);
/* per-op kernel timing with HIP events on the ctx stream (bench.py roofline
 * object).  After s3_plan_profile_begin(plan, max_forwards) every
 * s3_plan_forward records one event between consecutive ops (up to
 * max_forwards forwards); s3_plan_profile_end synchronises, writes the MEAN
 * duration in ms of each op over the recorded forwards into ms_per_op[0..cap)
 * and returns the number of forwards averaged (or a negative error). */
int s3_plan_profile_begin(s3_plan* plan, int max_forwards);
int s3_plan_profile_end(s3_plan* plan, float* ms_per_op, int cap);
/* 0: op i is not on MFMA; 1: MFMA halo-tile kernel (one tile per workgroup);
 * 2: its persistent variant (all-bf16 64 -> 64 trunk convs, >= 1 tile per CU) */
int s3_plan_op_is_mfma(const s3_plan* plan, int op_index);
/* introspection of the kernel selection (what SUP3R_AMD_TRACE prints), used by
 * the parity tests to assert which kernels a configuration runs on and to
 * build the bf16-emulating oracle (which convs round their operands / store
 * bf16).  Fills out[0..min(cap, S3_OPINFO_COUNT)) and returns S3_OPINFO_COUNT.
 * No reference counterpart: keras picks its conv algorithm inside TF. */
enum {
  S3_OPINFO_KIND = 0,          /* S3_OP_*                                      */
  S3_OPINFO_FWD = 1,           /* S3_FWD_* (convs)                             */
  S3_OPINFO_IN16 = 2,          /* input / output / residual stored as bf16     */
  S3_OPINFO_OUT16 = 3,
  S3_OPINFO_RES16 = 4,
  S3_OPINFO_FWD_BF16_OPS = 5,  /* forward kernel rounds x and w to bf16        */
  S3_OPINFO_WGRAD = 6,         /* S3_WGRAD_* (training plans)                  */
  S3_OPINFO_DGRAD = 7,         /* S3_DGRAD_*                                   */
  S3_OPINFO_MASK_FUSED_FROM = 8, /* op whose activation adjoint this conv's
                                  dgrad store applies, or -1                  */
  S3_OPINFO_IN_REP = 9,        /* conv reads its input through a fused temporal
                                  repeat of this factor; a repeat op / a concat op
                                  (Sup3rConcat): 1 = absorbed by its consumer
                                  conv (no launch)                              */
  S3_OPINFO_RES_REP = 10,      /* ... and its residual operand                  */
  S3_OPINFO_DGRAD_FRAME16 = 11, /* the padded-frame data gradient is stored as
                                  bf16 between the conv kernel and its fold    */
  S3_OPINFO_FEWPOS_MFMA = 12,  /* the few-positions launches of this conv are the
                                  one-launch fp32-MFMA kernels (forward, data
                                  gradient from the untransposed filter, weight
                                  + bias gradient)                              */
  S3_OPINFO_COUNT = 13
};
enum {
  S3_FWD_DIRECT = 0, S3_FWD_MFMA_TILE = 1, S3_FWD_MFMA_PERSIST = 2, S3_FWD_GCONV = 3,
  S3_FWD_GCONV_FEWCH = 4, S3_FWD_HALO32 = 5, S3_FWD_FEWPOS = 6, S3_FWD_TAIL_MFMA = 7,
  S3_FWD_SMALL = 8,
  S3_FWD_FUSED2D = 9, /* the whole op list in one launch (small 2-D stacks) */
  S3_FWD_HALO_S2 = 10, /* C_in = 32 stride-2 valid conv on an LDS halo         */
  S3_FWD_MFMA_GEN = 11, /* halo-tile MFMA over logical axes: 2-D nets, few time steps,
                           any C_in <= 256 / C_out (kernels_conv_mfma_gen.hip)     */
  S3_FWD_CONV2D_WS = 12, /* weights-stationary persistent Conv2D, all-bf16 64 -> 64 k
                           trunks of the 2-D generators (kernels_conv2d_ws.hip)    */
  S3_FWD_CONV2D_HEAD = 13 /* the few-feature head conv of those generators: C_in 1 / 2
                           -> 64, fp32 field in, bf16 cells out, filter in registers */
};
enum {
  S3_WGRAD_DIRECT = 0, S3_WGRAD_F32_TRUNK = 1, S3_WGRAD_BF16_TRUNK = 2, S3_WGRAD_F32_GEN = 3,
  S3_WGRAD_BF16_GEN = 4, S3_WGRAD_BF16_2D = 5, S3_WGRAD_C2 = 6, S3_WGRAD_TAIL = 7,
  S3_WGRAD_FEWPOS = 8
};
enum {
  S3_DGRAD_DIRECT = 0, S3_DGRAD_MFMA_FRAME = 1, S3_DGRAD_MFMA_VALID = 2,
  S3_DGRAD_MFMA_CHUNKED = 3, S3_DGRAD_FEWCH_FRAME = 4, S3_DGRAD_S2 = 5, S3_DGRAD_C2 = 6,
  S3_DGRAD_GCONV = 7, S3_DGRAD_FEWPOS = 8
};
int s3_plan_op_info(const s3_plan* plan, int op_index, int32_t* out, int cap);
/* 0 = fp32, 1 = bf16 storage of a plan tensor (bf16 plans keep the trunk in bf16) */
int s3_plan_tensor_dtype(const s3_plan* plan, int32_t tensor_id);
/* raw bytes of a plan tensor (in its storage dtype) to host memory after a
 * stream sync; returns the byte count or a negative error.  Training plans
 * keep every activation: the tests read the LeakyReLU masks the device used. */
int64_t s3_plan_tensor_read(s3_plan* plan, int32_t tensor_id, void* host, size_t cap_bytes);

/* ---- losses ------------------------------------------------------------
 * content loss: keras MeanAbsoluteError / MeanSquaredError as used by
 * Sup3rGan.calc_loss_gen_content (base.py:478-503): mean over the first
 * c_used channels of a (c_a channels, generated) vs b (c_b channels, truth
 * incl. trailing exo channels).  loss_out: device float (accumulated with
 * weight); d_a (nullable): d(weight*loss)/da written (accumulate != 0: added). */
int s3_loss_content(s3_ctx* ctx, int kind, const float* a, int c_a,
                    const float* b, int c_b, int c_used, int64_t n_pos,
                    float weight, float* loss_out, float* d_a, int accumulate);
/* masked variant used by Sup3rCondMom.calc_loss_cond_mom
 * (sup3r/models/conditional.py:221-241): loss(a * mask, b * mask). */
int s3_loss_content_masked(s3_ctx* ctx, int kind, const float* a, int c_a,
                           const float* b, int c_b, const float* mask, int c_m,
                           int c_used, int64_t n_pos, float weight,
                           float* loss_out, float* d_a, int accumulate);
/* relativistic BCE of Sup3rGan.calc_loss_disc (base.py:505-549).
 * loss_out: device float; d_true / d_gen nullable (n floats each), scaled by
 * `scale` (weight_gen_advers for the adversarial term). */
int s3_loss_rel_bce(s3_ctx* ctx, const float* disc_true, const float* disc_gen,
                    int n, float scale, float* loss_out, float* d_true,
                    float* d_gen);

/* ---- structured content losses -----------------------------
 * sup3r/utilities/loss_metrics.py: every loss there is M(F(gen), F(true)) with
 * M = MeanAbsoluteError / MeanSquaredError (s3_loss_content) and F a feature
 * map.  s3_lossmap_fwd writes F(x) for x = (n, s1, s2, t, c) fp32 (t = 1 for
 * 4-D), first c_used channels; s3_lossmap_bwd ADDS F'(x)^T g_out into
 * d_x[..., :c_used].  Shapes of F(x):
 *   S3_LMAP_DERIV_S  (n, s1, s2, t, c_used)   d/ds1 + d/ds2, np.gradient scheme
 *                                             (SpatialDerivativeLoss :228-260)
 *   S3_LMAP_DERIV_T  (n, s1, s2, t, c_used)   d/dt (TemporalDerivativeLoss :263-294)
 *   S3_LMAP_MATERIAL (n, s1, s2, t, c_used/2) du/dt + u du/ds1 + v du/ds2 of each
 *                                             (u, v) pair (MaterialDerivativeLoss :150-225)
 *   S3_LMAP_MEAN_S   (n, t, c_used)           mean over (s1, s2) (CoarseMseLoss :297-322)
 *   S3_LMAP_EXT_S    2 x (n, t, c_used)       [min | max] over (s1, s2) (:325-357)
 *   S3_LMAP_EXT_T    2 x (n, s1, s2, c_used)  [min | max] over t (:360-392)
 *   S3_LMAP_COARSEN  backward only (forward = s3_coarsen): p0 = s_enhance, p1 =
 *                    t_enhance, p2 = S3_TC_AVERAGE | S3_TC_SUBSAMPLE; g_out has
 *                    c channels (LowResLoss :488-638)
 * work: spatial reductions n * 64 * t * c_used floats; extremes adjoint
 * additionally 2 * (size of one extremum) in front.  fx (bwd, extremes only) =
 * the forward map of the same x.  Ties share the gradient equally, as
 * tf.reduce_min / reduce_max do. */
enum { S3_LMAP_DERIV_S = 0, S3_LMAP_DERIV_T = 1, S3_LMAP_MATERIAL = 2, S3_LMAP_MEAN_S = 3,
       S3_LMAP_EXT_S = 4, S3_LMAP_EXT_T = 5, S3_LMAP_COARSEN = 6 };
int s3_lossmap_fwd(s3_ctx* ctx, int kind, const float* x, int n, int s1, int s2,
                   int t, int c, int c_used, int p0, int p1, int p2, float* out,
                   float* work);
int s3_lossmap_bwd(s3_ctx* ctx, int kind, const float* x, const float* fx,
                   const float* g_out, int n, int s1, int s2, int t, int c,
                   int c_used, int p0, int p1, int p2, float* d_x, float* work);
/* MmdLoss (loss_metrics.py:62-147): gaussian-kernel maximum mean discrepancy
 * over all pairs of the n observations at every one of the n_pos positions;
 * a, b = (n, n_pos, c_*).  loss_out = unweighted value; d_a (nullable) +=
 * weight * d loss / d a. */
int s3_loss_mmd(s3_ctx* ctx, const float* a, int c_a, const float* b, int c_b, int n,
                int64_t n_pos, int c_used, float sigma, float weight, float* loss_out,
                float* d_a);

/* SlicedWassersteinLoss (loss_metrics.py:724-789): n_proj (<= 4096) random unit
 * directions over the n_pos positions, the n * c_used (observation, feature)
 * columns of a, b = (n, n_pos, c_*) projected, each column's projections
 * sorted, mean squared difference of the sorted values.  The directions are a
 * counter-based draw from `seed` (Philox4x32-10 + Box-Muller), regenerated in
 * the backward pass instead of stored; the reference draws new directions per
 * call (tf.random.normal, :777), the caller does the same by passing a new
 * seed.  loss_out = unweighted value; d_a (nullable) += weight * d loss / d a.
 * s3_sw_directions writes the raw (un-normalised) direction matrix
 * [n_proj][n_pos] of a seed — how the parity tests feed the oracle. */
int s3_loss_sliced_wasserstein(s3_ctx* ctx, const float* a, int c_a, const float* b, int c_b,
                               int n, int64_t n_pos, int c_used, int n_proj, uint64_t seed,
                               float weight, float* loss_out, float* d_a);
int s3_sw_directions(s3_ctx* ctx, uint64_t seed, int n_proj, int64_t n_pos, float* out);

/* Time windows of a (outer = n * s1 * s2, t, c) field, as SolarCC.calc_loss
 * slices the hi-res tensors (sup3r/models/solar_cc.py:155-232).
 * s3_time_window: adjoint == 0 copies full[:, t0:t0+len, :] into the contiguous
 * `window`; adjoint != 0 adds scale * window back into that slice of `full`.
 * s3_time_mean: adjoint == 0 writes mean[o][c] = tf.reduce_mean(full[:, t0:t0+len,
 * :], axis=time); adjoint != 0 adds (scale / len) * mean[o][c] to every step of
 * the slice. */
int s3_time_window(s3_ctx* ctx, float* full, int64_t outer, int t, int c, int t0, int len,
                   float* window, int adjoint, float scale);
int s3_time_mean(s3_ctx* ctx, float* full, int64_t outer, int t, int c, int t0, int len,
                 float* mean, int adjoint, float scale);

/* SpatialFftLoss / SpatiotemporalFftLoss (loss_metrics.py:395-485): separable
 * direct DFT, one call per axis over a contiguous (outer, L, inner) view,
 * unnormalised; sign < 0 = forward (tf.signal.fft2d / fft3d), > 0 = adjoint;
 * in_im may be NULL (real input).  A workgroup keeps 32 columns and the
 * twiddles in LDS (264 L bytes): S3_EINVAL for an axis longer than the
 * device's LDS per workgroup / 264 (620 at the MI355X's 160 KiB).
 * s3_specmap: backward == 0 writes out0 = log(1 + w |X|) with w = k1^2 k2^2
 * (kt^2 if mode3d) over (n, s1, s2, t, c);
 * backward != 0 writes (out0, out1) = g_y * w / (1 + w |X|) * X / |X|. */
int s3_dft_axis(s3_ctx* ctx, const float* in_re, const float* in_im, float* out_re,
                float* out_im, int64_t outer, int L, int64_t inner, int sign);
int s3_specmap(s3_ctx* ctx, int backward, const float* re, const float* im,
               const float* g_y, int n, int s1, int s2, int t, int c, int mode3d,
               float* out0, float* out1);

/* ---- small tensor utilities on the ctx stream --------------------------
 * channel slice/concat used by _combine_loss_input / get_hr_exo_input
 * (abstract.py:415-459) and per-feature affine of norm_input /
 * un_norm_output (abstract.py:197-275). */
int s3_copy_channels(s3_ctx* ctx, const float* src, int c_src, int c0_src,
                     float* dst, int c_dst, int c0_dst, int nc, int64_t n_pos,
                     int accumulate);
int s3_affine_channels(s3_ctx* ctx, const float* src, float* dst, int c,
                       int64_t n_pos, const float* scale_host,
                       const float* shift_host);
int s3_fill(s3_ctx* ctx, float* dst, int64_t n, float value);
/* device -> device copy of a (d0, d1, row_elems) fp32 block between two
 * strided layouts (strides in elements; rows are contiguous): the lo-res chunk
 * window `data[lr_pad_slice]` (strategy.py:474-518) cut out of the resident
 * domain, and the halo crop `hi_res[0][hr_crop_slices]` of the generated chunk
 * (forward_pass.py:272). */
int s3_copy_block(s3_ctx* ctx, const float* src, float* dst, int64_t d0, int64_t d1,
                  int64_t row_elems, int64_t src_stride0, int64_t src_stride1,
                  int64_t dst_stride0, int64_t dst_stride1);
/* device half of ForwardPass._output_check (sup3r/pipeline/forward_pass.py:
 * 384-425: NaNs or a constant output channel mean the chunk failed): for x =
 * (n_chunks, pos_per_chunk, c) writes partial[n_chunks][64][c][3] = (min, max,
 * NaN count) per slab of positions; the caller folds the 64 slabs. */
int s3_chunk_stats(s3_ctx* ctx, const float* x, int n_chunks,
                   int64_t pos_per_chunk, int c, float* partial);
/* everything between the generator's last layer and the delivery of a batch of
 * chunks in one pass: un-normalisation (x * scale + shift per channel, the two
 * roundings of un_norm_output, sup3r/models/abstract.py:240-275; NULL scale /
 * shift: none), the halo crop hi_res[0][hr_crop_slices]
 * (sup3r/pipeline/forward_pass.py:272) and the statistics of _output_check
 * (:384-425; partial as s3_chunk_stats).  y = (n_chunks, dims[0..2], c) fp32,
 * yc = (n_chunks, crop_n[0..2], c).  c must divide 1024 and rows must be
 * 16-byte aligned ((crop_lo[2] c), (crop_n[2] c), (dims[2] c) multiples of 4):
 * S3_EINVAL otherwise, and the caller runs s3_affine_channels / s3_copy_block /
 * s3_chunk_stats instead (bit-identical results). */
int s3_chunk_epilogue(s3_ctx* ctx, const float* y, int n_chunks, const int64_t* dims,
                      const int64_t* crop_lo, const int64_t* crop_n, int c,
                      const float* scale_host, const float* shift_host, float* yc,
                      float* partial);
/* the way INTO a 2-D (spatial) model (ForwardPass._reshape_data_chunk,
 * sup3r/pipeline/forward_pass.py:274-337: np.transpose(data_chunk, (2, 0, 1,
 * 3))) fused with Sup3rGan.norm_input (sup3r/models/abstract.py:197-238): x =
 * (n_chunks, hwt[0], hwt[1], hwt[2], c) fp32 raw chunks, out = (n_chunks *
 * hwt[2], hwt[0], hwt[1], c) = (x - mean) / std per channel with numpy's
 * arithmetic — fp32 when the statistics are fp32 arrays (stats_fp32 = 1), fp64
 * rounded to fp32 otherwise; NULL mean / std: transpose only. */
int s3_chunk_time_first(s3_ctx* ctx, const float* x, int n_chunks, const int64_t* hwt, int c,
                        const double* mean_host, const double* std_host, int stats_fp32,
                        float* out);
/* a time-invariant exo field laid over a chunk's time steps on the device:
 * dst[o][a][r][b] = src[o][a][b] for r < reps (outer x a x b floats in, outer x
 * a x reps x b out).  ForwardPass.pad_source_data (sup3r/pipeline/
 * forward_pass.py:160-186) repeats 3-D exo fields along time on the host
 * (np.repeat) before every chunk; here the chunk carries a zero-stride view and
 * the executor uploads the field once. */
int s3_broadcast_axis(s3_ctx* ctx, const float* src, int64_t outer, int64_t a, int64_t b, int64_t reps,
                      float* dst);
/* between two steps of a MultiStepGan chain (MultiStepGan.generate,
 * sup3r/models/multi_step.py:233-259) on the device, position by position: y =
 * (n_pos, c_src) the NORMALISED output of step i's generator; x = (n_pos, c_sel
 * + n_exo) the normalised input of step i + 1: channel k < c_sel = norm(
 * un_norm(y[map[k]])) — un_norm_output of step i (y * scale[c] + shift[c] per
 * SOURCE channel, abstract.py:240-275), _match_model_input's selection
 * (multi_step.py:148-194), norm_input of step i + 1 ((v - mean[k]) / std[k] per
 * DESTINATION channel, abstract.py:197-238); channel c_sel + j = norm(exo[j]),
 * exo = (n_pos, n_exo) the raw 'input' exo fields _combine_fwp_input appends
 * (interface.py:259-356).  numpy's fp32 arithmetic (one rounding per
 * operation).  NULL scale / shift: no un-normalisation; NULL mean / std: none. */
int s3_step_handover(s3_ctx* ctx, const float* y, int64_t n_pos, int c_src, const int* map_host,
                     int c_sel, const float* scale_host, const float* shift_host, const float* exo,
                     int n_exo, const float* mean_host, const float* std_host, float* x);
/* the hand-over with TWO sources: the join of SolarMultiStepGan's spatial
 * branches (sup3r/models/multi_step.py:785-806).  ya = (t, h, w, ca) and yb =
 * (t, h, w, cb) are the NORMALISED, time-first outputs of the two branches'
 * last 2-D generators; x = (1, h, w, t, na + nb) is the normalised input of the
 * temporal chain: x[0,i,j,s,k] = norm(unnorm_a(ya[s,i,j,map_a[k]])) for k < na,
 * norm(unnorm_b(yb[s,i,j,map_b[k - na]])) for the rest — unnorm = v *
 * scale[src channel] + shift[src channel] (two fp32 roundings), norm = (v -
 * mean[k]) / std[k] per destination channel, as in s3_step_handover; NULL
 * scale / shift of a source: no un-normalisation of it; NULL mean / std: no
 * normalisation.  Every bit pattern takes the same arithmetic.  Maps and
 * statistics travel in the kernel arguments (no upload, no synchronisation);
 * 64-bit offsets; any t, h, w >= 1.  S3_EINVAL unless ca, cb, na + nb <= 16
 * and na + nb >= 1 (na or nb may be 0: that source is not read). */
int s3_branch_join(s3_ctx* ctx, const float* ya, int ca, const int* map_a_host, int na,
                   const float* scale_a_host, const float* shift_a_host,
                   const float* yb, int cb, const int* map_b_host, int nb,
                   const float* scale_b_host, const float* shift_b_host,
                   int64_t t, int64_t h, int64_t w,
                   const float* mean_host, const float* std_host, float* x);
/* SolarMultiStepGan.temporal_pad (multi_step.py:824-852) fused with
 * un_norm_output: y = (outer, t, c) -> out = (outer, t + 2 pad, c), out[o, i, q]
 * = unnorm(y[o, r(i - pad), q]) with r numpy's mode='reflect' for ANY pad
 * width: p = 2 (t - 1), m = ((j mod p) + p) mod p, r(j) = m if m < t else p - m;
 * r = 0 for t = 1.  c <= 16; NULL scale / shift: a pure pad; pad = 0: the
 * un-normalisation alone. */
int s3_time_pad_reflect(s3_ctx* ctx, const float* y, int64_t outer, int64_t t, int c,
                        int64_t pad, const float* scale_host, const float* shift_host,
                        float* out);
/* the same hand-over for a 2-D (spatial) model, whose batch axis is the chunk's
 * time axis (ForwardPass._reshape_data_chunk, sup3r/pipeline/forward_pass.py:
 * 274-337: np.transpose(data_chunk, (2, 0, 1, 3)) in, np.transpose(hi_res, (1,
 * 2, 0, 3)) out, then hi_res[0][hr_crop_slices], :272): y = (n_chunks * thw[0],
 * thw[1], thw[2], c) fp32 as generated, yc = (n_chunks, crop_n[0..2], c) in the
 * chunk's (s1, s2, t) order, crop_lo / crop_n over (s1, s2, t); un-normalised
 * with the two roundings of un_norm_output (sup3r/models/abstract.py:240-275;
 * NULL scale / shift: none).  s3_chunk_stats on yc completes _output_check. */
int s3_chunk_time_last(s3_ctx* ctx, const float* y, int n_chunks, const int64_t* thw,
                       const int64_t* crop_lo, const int64_t* crop_n, int c,
                       const float* scale_host, const float* shift_host, float* yc);
/* placement of a cropped hi-res chunk straight into the caller's host array
 * (the `out[hr_slice] = chunk` of the forward pass, sup3r/pipeline/
 * forward_pass.py:582-673 + the writers' window placement): one pitched
 * device -> host DMA of a contiguous (d0, d1, row_elems) device block into the
 * window dst_host[i * dst_stride0 + j * dst_stride1 + 0..row_elems) (strides
 * in elements).  The host array must be registered once (s3_host_register)
 * for the copy to be asynchronous; `stream` = a hipStream_t or NULL for the
 * context stream. */
int s3_host_register(s3_ctx* ctx, void* ptr, size_t bytes);
int s3_host_unregister(s3_ctx* ctx, void* ptr);
int s3_d2h_window(s3_ctx* ctx, const float* src, float* dst_host, int64_t d0,
                  int64_t d1, int64_t row_elems, int64_t dst_stride0,
                  int64_t dst_stride1, void* stream);
/* the delivery of a batch of cropped hi-res chunks to the host (the
 * `.numpy()` at the end of generate, sup3r/models/abstract.py:1100, as the
 * chunk executor of sup3r/pipeline/forward_pass.py:451-500 needs it: under the
 * NEXT batch's forward): a contiguous device buffer -> pinned (mapped) host
 * memory by a kernel of `blocks` workgroups (<= 0: 16) on `stream` (NULL: the
 * context stream) that writes through PCIe directly — throttled on purpose so
 * that it shares the chip with the compute stream instead of occupying every
 * wave slot like the runtime's full-grid blit copy.  16-byte aligned pointers,
 * bytes % 16 == 0. */
int s3_d2h_stream(s3_ctx* ctx, const void* src, void* dst_host, size_t bytes,
                  void* stream, int blocks);
/* delivery buffers of the chunk executor (what the reference's workers return
 * through the process pool, sup3r/pipeline/forward_pass.py:526-580): pinned,
 * device-mapped host memory.  noncoherent != 0: coarse-grained (the GPU may
 * cache its writes in L2 until the kernel ends; the host must only read after
 * the stream / event that follows the copy has completed — which is how the
 * executor uses it).  s3_d2h_async: plain hipMemcpyAsync(DeviceToHost). */
int s3_host_alloc(s3_ctx* ctx, size_t bytes, int noncoherent, void** out);
int s3_host_free(s3_ctx* ctx, void* ptr);
int s3_d2h_async(s3_ctx* ctx, const void* src, void* dst_host, size_t bytes,
                 void* stream);
/* the same delivery on an SDMA engine (ROCr hsa_amd_memory_async_copy): the
 * shader-side copies above stall the chip's other memory traffic while PCIe
 * drains them, the DMA engines do not.  Ordering is the caller's: call _begin
 * only after the work that produced `src` has COMPLETED (host-synchronised
 * event), read `dst_host` (an s3_host_alloc buffer) only after s3_dma_wait
 * returned S3_OK.  *ticket identifies the copy; s3_dma_wait consumes it
 * (timeout_ms <= 0: no deadline). */
int s3_dma_d2h_begin(s3_ctx* ctx, const void* src, void* dst_host, size_t bytes,
                     uint64_t* ticket);
int s3_dma_wait(s3_ctx* ctx, uint64_t ticket, int timeout_ms);

/* ---- batch transform on the device ----------------------
 * replaces the host numpy of SingleBatchQueue.transform
 * (sup3r/preprocessing/batch_queues/base.py:32-87):
 *   s3_coarsen         = spatial_coarsening (sup3r/utilities/utilities.py:
 *                        406-523, s x s block mean) fused with
 *                        temporal_coarsening (:345-403; t_method one of
 *                        S3_TC_*; t_enhance <= 1 = spatial only).  hr is
 *                        (n, s1, s2, t, c) fp32 (4-D batches: t = 1), lr is
 *                        (n, s1/s, s2/s, t/t_enhance, c).
 *   s3_gaussian_smooth = smooth_data (batch_queues/utilities.py:57-103):
 *                        scipy gaussian_filter(mode='nearest') over the two
 *                        spatial axes of every (obs, t, feature) slice of
 *                        channels whose bit is set in channel_mask; weights =
 *                        the 2*radius+1 normalised taps (host), tmp = scratch
 *                        of the size of x. */
#define S3_TC_SUBSAMPLE 0
#define S3_TC_AVERAGE 1
#define S3_TC_TOTAL 2
#define S3_TC_MAX 3
#define S3_TC_MIN 4
int s3_coarsen(s3_ctx* ctx, const float* hr, int n, int s1, int s2, int t, int c,
               int s_enhance, int t_enhance, int t_method, float* lr);
int s3_gaussian_smooth(s3_ctx* ctx, const float* x, int n, int s1, int s2, int t,
                       int c, const float* weights_host, int radius,
                       unsigned channel_mask, float* tmp, float* y);

/* ---- conditional-moment training targets on the device ---------------------
 * replaces the host numpy / scipy of ConditionalBatchQueue.post_proc
 * (sup3r/preprocessing/batch_queues/conditional.py:151-166): make_output of
 * QueueMom1SF / Mom2 / Mom2Sep / Mom2SF / Mom2SepSF (:178-288) and make_mask
 * (:79-127) in one streaming pass over the hi-res batch.
 *   hr   (n, s1, s2, t, c_hr) fp32 (4-D batches: t = 1)
 *   lr   (n, s1/s_enhance, s2/s_enhance, t/t_enhance, c_lr); read only with
 *        S3_CM_SUBFILTER.  lr_channel_host[c] (host, c_hr entries) = the lr
 *        channel of hr channel c (enhanced_lr[..., hr_features_ind])
 *   mom1 (n, s1, s2, t, c_m), c_m <= c_hr: the first-moment model's output;
 *        read only with S3_CM_MOM1.  For c >= c_m the first moment IS
 *        hr[..., c] (_combine_loss_input, abstract.py:438-459: the truth's
 *        exogenous channels stand in; the joined tensor is never written)
 *   out[e] = v, with v = hr[e]; v -= e^ (S3_CM_SUBFILTER); v -= m (S3_CM_MOM1);
 *        v *= v (S3_CM_SQUARE) — in this order, one fp32 rounding each.
 *        e^ = lr cell (i / s, j / s, k / t_enhance)
 *        (spatial_simple_enhancing / temporal_simple_enhancing mode
 *        'constant', batch_queues/utilities.py:12-54, :106-173: zoom(order=0)
 *        is a repeat); with S3_CM_LINEAR and t_enhance > 1 in time
 *        lo + (hi - lo) * frac, i0 = min(k / t_enhance, t / t_enhance - 2),
 *        frac = (k - i0 t_enhance) / t_enhance (interp1d(fill_value=
 *        'extrapolate') over the landmarks 0, t_enhance, 2 t_enhance, ...).
 *        t_enhance <= 1 ignores S3_CM_LINEAR, as the reference does.
 *   mask[e] = 1 for s_pad <= i < s1 - s_pad, s_pad <= j < s2 - s_pad,
 *        t_lo <= k < t_hi (every channel), else 0.
 *   out == NULL or mask == NULL: that tensor is not written (not both).
 * S3_EINVAL: extents that the enhancement factors do not divide, c_m > c_hr,
 * a channel-map entry outside [0, c_lr), S3_CM_LINEAR with t_enhance > 1 and
 * fewer than two low-res time steps (scipy returns NaN there), c_hr > 32,
 * 2^31 or more elements. */
#define S3_CM_SUBFILTER 1u
#define S3_CM_LINEAR 2u
#define S3_CM_MOM1 4u
#define S3_CM_SQUARE 8u
int s3_condmom_target(s3_ctx* ctx, const float* hr, const float* lr, const float* mom1,
                      int n, int s1, int s2, int t, int c_hr, int c_lr, int c_m,
                      const int* lr_channel_host, int s_enhance, int t_enhance,
                      unsigned flags, int s_pad, int t_lo, int t_hi, float* out,
                      float* mask);

/* ---- training samples out of a resident data cube ---------------------------
 * replaces the host slicing of Sampler.__next__ (sup3r/preprocessing/samplers/
 * base.py:228-262: _fast_batch's one box of batch_size * t steps reshaped,
 * _slow_batch's batch_size boxes stacked) and the upload of the batch:
 *   data (S1, S2, T, C) fp32, the container layout, resident on the device;
 *        offsets into it are 64-bit (a year of a 100 x 100 domain with 10
 *        features is 3.5 GB)
 *   origins_host[n][3]  host: i0, j0, k0 of every sample's box (s1, s2, t)
 *   channel_host[c_out] host: the cube channel of every channel kept
 *   out[m, i, j, k, q] = data[i0[m] + i, j0[m] + j, k0[m] + k, channel[q]],
 *        (n, s1, s2, t, c_out); a copy: every bit pattern arrives as it is.
 * Origins and channel map travel in the kernel arguments, S3_SAMPLE_MAX_ORIGINS
 * samples per launch (a larger n is split here); nothing is copied to the
 * device and nothing synchronises: the launches are asynchronous on the
 * context's stream.
 * S3_EINVAL, before anything is launched: a box that leaves the cube, a
 * channel outside [0, C), extents or n below 1, c_out above
 * S3_SAMPLE_MAX_CHANNELS, 2^31 or more elements of out. */
#define S3_SAMPLE_MAX_ORIGINS 64
#define S3_SAMPLE_MAX_CHANNELS 32
int s3_sample_gather(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T, int C,
                     const int* origins_host, int n, int s1, int s2, int t,
                     const int* channel_host, int c_out, float* out);

/* ---- DualSamplerCC: daylight window and nearest-neighbour fill ---------------
 * replaces what DualSamplerCC.__next__ (sup3r/preprocessing/samplers/cc.py:
 * 185-203) does to a batch on the host after cutting it: nsrdb_reduce_daily_data
 * (samplers/utilities.py:258-297) and nn_fill_array (sup3r/utilities/
 * utilities.py:55-75, scipy.ndimage.distance_transform_edt with indices).
 *
 * status: S3_CC_STATUS_WORDS 32-bit words on the device, read by nobody on the
 * host unless asked for:
 *   [S3_CC_NIGHT_MASK] bit k: the channel is NaN somewhere at hour k of the
 *                      24-hour windows;
 *   [S3_CC_START_RAW]  first hour kept as the reference computes it: the first
 *                      daylight hour - ceil((t - daylight hours) / 2);
 *   [S3_CC_START]      the hour the gather started at;
 *   [S3_CC_FILLED]     NaNs s3_nn_fill found in its channel (every one of them
 *                      is filled unless the channel holds nothing else).
 *
 * s3_cc_night_mask: zeroes the status words (asynchronously), then ORs the
 * mask of the n 24-hour windows data[i0 + i, j0 + j, k0 .. k0 + 24, channel]
 * (i < s1, j < s2; origins as for s3_sample_gather) into the first.
 *
 * s3_cc_window_gather: s3_sample_gather, but the origins are those of the
 * 24-hour windows and
 *   out[m, i, j, k, q] = data[i0[m] + i, j0[m] + j, k0[m] + start + k, channel[q]]
 * for t < 24 hours, start computed on the device from status[S3_CC_NIGHT_MASK]
 * and recorded.  Two deviations from the reference: start is clamped into
 * [0, 24 - t] (the reference's slice(start, start + t) of 24 steps comes out
 * short or empty when start is negative or past 24 - t), and 24 hours of night
 * give the centred window start = (24 - t) / 2 (the reference warns and
 * returns all 24 hours).
 *
 * s3_nn_fill: in place, on channel `channel` of the contiguous fp32 block x
 * (n, s1, s2, t, C): every element whose bits are a NaN receives the bits of
 * the non-NaN element of that channel that minimises (dn^2 + di^2 + dj^2 +
 * dk^2, column-major index m + n (i + s1 (j + s2 k))) — the element scipy
 * picks, ties included.  Nothing else is written: other channels (their NaNs
 * too), -0.0, infinities and denormals keep their bits; a channel without NaN
 * or with nothing but NaN is left as it is (the kernels behind the first see
 * the count on the device and return).  work: 8 bytes per element of the
 * channel (n * s1 * s2 * t), 8-byte aligned; count: one status word, zeroed
 * here.  S3_EINVAL: an extent above S3_NN_FILL_MAX_AXIS (lines are staged in
 * LDS whole; squared distances stay far below 2^32), 2^31 or more elements of
 * the channel.
 *
 * All three are asynchronous on the context's stream; nothing is uploaded. */
#define S3_CC_STATUS_WORDS 4
#define S3_CC_NIGHT_MASK 0
#define S3_CC_START_RAW 1
#define S3_CC_START 2
#define S3_CC_FILLED 3
#define S3_NN_FILL_MAX_AXIS 2048
int s3_cc_night_mask(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T, int C,
                     const int* origins_host, int n, int s1, int s2, int channel, int* status);
int s3_cc_window_gather(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T, int C,
                        const int* origins_host, int n, int s1, int s2, int t,
                        const int* channel_host, int c_out, int* status, float* out);
int s3_nn_fill(s3_ctx* ctx, float* x, int n, int s1, int s2, int t, int C, int channel,
               void* work, int* count);

/* ---- per-feature statistics and normalisation of a resident cube -----------
 * replaces the host pass of StatsCollection (sup3r/preprocessing/collections/
 * stats.py:51-74: .mean(skipna=True) / .std(skipna=True) of every feature over
 * all of space and time) and of Sup3rX.normalize (accessor.py:356-361) over a
 * channels-last fp32 cube x (n_pos, c), c <= S3_STATS_MAX_CHANNELS, any c in
 * that range, 4-byte aligned (16-byte loads run between a head and a tail of up
 * to 3 floats); element offsets are 64-bit.
 *
 * s3_channel_moments: out[c][3] (DEVICE, fp64) = the number of non-NaN values
 * of the channel, their mean, and the sum of their squared deviations from it
 * (std = sqrt(out[2] / out[0]), ddof 0), from ONE read of the cube: shifted
 * sums in fp64, folded in a fixed order without atomics — two calls on the same
 * cube give the same bits.  +-inf counts as a value: the mean is +-inf (NaN for
 * both signs) and the third word NaN, as numpy's.  A channel without a value:
 * (0, 0, 0).  Uses the context's scratch block for the workgroups' partials.
 *
 * s3_normalize_channels: x[p][q] = (x[p][q] - mean_host[q]) / std_host[q] in
 * place for every q with flag_host[q] != 0, as a correctly rounded fp32
 * subtraction followed by a correctly rounded fp32 division — bit for bit
 * numpy's float32 (x - m) / s, which neither a multiply by a reciprocal nor
 * s3_affine_channels gives.  Unflagged channels keep every bit; NaN stays NaN.
 * The three host arrays (c entries each) travel in the kernel arguments.
 *
 * Both are asynchronous on the context's stream.  S3_EINVAL: c outside 1 ..
 * S3_STATS_MAX_CHANNELS, n_pos < 1, a misaligned pointer. */
#define S3_STATS_MAX_CHANNELS 64
int s3_channel_moments(s3_ctx* ctx, const float* x, int64_t n_pos, int c, double* out);
int s3_normalize_channels(s3_ctx* ctx, float* x, int64_t n_pos, int c, const float* mean_host,
                          const float* std_host, const unsigned char* flag_host);

/* ---- bias correction of forward-pass chunks on the device ------------------
 * replaces the host numpy / rex of ForwardPassStrategy.prep_chunk_data
 * (sup3r/pipeline/strategy.py:502-517 -> bias_correct_features ->
 * sup3r/bias/bias_transforms.py) for a batch of equal-shaped chunks that are
 * ALREADY reflect-padded (forward_pass.py:66-72,122-186):
 *   x, out  (n, s1, s2, t, c) fp32; out may be x.  n <= S3_BC_MAX_CHUNKS,
 *           c <= S3_BC_MAX_CHANNELS.
 *   channels_host[c]  one descriptor per channel (host); kind S3_BC_NONE
 *           passes the channel through.  Table pointers are DEVICE pointers:
 *           domain tables (S1, S2, n_t[, n_q]) resident for the whole low-res
 *           domain; with S3_BC_PER_CHUNK per-chunk tables (n, s1, s2, n_t[,
 *           n_q]) padded like the chunks themselves (smoothed factors,
 *           bias_transforms.py:334-341,465-472); with S3_BC_GLOBAL one row
 *           for every pixel (global_linear_bc, :224-248).
 *   geom_host[n][6]   per chunk: o1, o2 = origin of the chunk's in-domain
 *           window in the domain tables; lo1, lo2 = reflect padding in front
 *           of it; e1, e2 = its un-padded extents.  Pixel (i, j) of the padded
 *           chunk reads table row (o1 + reflect(i - lo1, e1), o2 + reflect(j -
 *           lo2, e2)), reflect = the index map of np.pad(mode='reflect'): the
 *           reference corrects the window and pads the result, which is the
 *           same values.
 *   month, window     device int32 (n, t): per time step of the padded chunk
 *           the month (0 .. 11; S3_BC_MONTH) / the QDM time window
 *           (argmin |doy - time_window_center|, bias_transforms.py:788-791),
 *           mirrored along time by the host.  NULL if no channel needs it.
 *   weights           device fp64 (n, n_t): S3_BC_WEIGHTS, the share of each
 *           month in the chunk's time index; scalar = sum_m w_m table[i, j, m]
 *           (accumulated in fp64, rounded once) stands for the mean over the
 *           gathered months of temporal_avg=True (:442-448).
 * S3_BC_LINEAR: out = x * scalar + adder, multiply and add rounded separately
 *   (numpy's float32 arithmetic); S3_BC_SCALAR_RANGE / S3_BC_ADDER_RANGE clamp
 *   the factors with np.minimum(f, hi) then np.maximum(f, lo) (:474-480).
 * S3_BC_QDM (empirical distribution, linear sampling): with the rows oh, mh,
 *   mf (n_q quantile values each) at (i, j, window) and levels q_k = k / (n_q
 *   - 1): q = interp(x, mf, q_k), x_oh = interp(q, q_k, oh), x_mh = interp(q,
 *   q_k, mh), interp = numpy.interp (clamped at both ends; on repeated knots
 *   the segment is the last j with xp[j] <= x).  S3_BC_RELATIVE: x_mh = 0 ->
 *   denom_zero (S3_BC_DENOM_ZERO), x_mh = max(x_mh, denom_min)
 *   (S3_BC_DENOM_MIN), delta = x / x_mh, out = x_oh * delta; otherwise delta =
 *   x - x_mh, out = x_oh + delta; S3_BC_DELTA_RANGE clamps delta (Cannon et
 *   al. 2015, eqs. 3-6).  S3_BC_NO_TREND uses mh in place of mf.
 *   S3_BC_PRESRAT (without S3_BC_NO_TREND): out = out < tau[i, j] ? 0 : out *
 *   kfac[i, j, window] (:1115-1120).
 * S3_BC_OUT_RANGE: np.maximum(out, out_lo) then np.minimum(out, out_hi), last
 *   (:483-485, :813-815).
 * mean_host / std_host (c doubles each, or NULL): the result is written
 *   normalised, (out - mean) / std, with the arithmetic of
 *   s3_chunk_time_first (fp32 when stats_fp32, fp64 rounded once otherwise),
 *   every channel, corrected or not.
 * nonfinite: device int32[c], ADDED to: the number of corrected values per
 *   channel that are not finite (:816, NaN or inf) — with S3_BC_PRESRAT that
 *   are NaN (:1128 tests isnan only); the RuntimeError of :816-823,
 *   :1128-1135 is the caller's.
 * S3_EINVAL: more chunks / channels than the limits, a window that leaves the
 * padded chunk or the domain tables, a channel without the tables or index
 * arrays its kind and flags need. */
#define S3_BC_MAX_CHANNELS 16
#define S3_BC_MAX_CHUNKS 32
#define S3_BC_NONE 0
#define S3_BC_LINEAR 1
#define S3_BC_QDM 2
#define S3_BC_MONTH 1u
#define S3_BC_WEIGHTS 2u
#define S3_BC_SCALAR_RANGE 4u
#define S3_BC_ADDER_RANGE 8u
#define S3_BC_OUT_RANGE 16u
#define S3_BC_PER_CHUNK 32u
#define S3_BC_RELATIVE 64u
#define S3_BC_NO_TREND 128u
#define S3_BC_DENOM_ZERO 256u
#define S3_BC_DENOM_MIN 512u
#define S3_BC_DELTA_RANGE 1024u
#define S3_BC_PRESRAT 2048u
#define S3_BC_GLOBAL 4096u
typedef struct s3_bias_channel {
  int32_t kind;              /* S3_BC_NONE / LINEAR / QDM */
  uint32_t flags;
  int32_t n_t;               /* last table axis: 1 or 12 months / QDM windows */
  int32_t n_q;               /* quantiles per QDM row */
  const float* scalar;       /* LINEAR (.., n_t) */
  const float* adder;
  const float* oh;           /* QDM (.., n_t, n_q): base_{base_dset}_params */
  const float* mh;           /*     bias_{feature}_params */
  const float* mf;           /*     bias_fut_{feature}_params */
  const float* tau;          /* PRESRAT (..): {feature}_tau_fut */
  const float* kfac;         /*     (.., n_t): {feature}_k_factor */
  float scalar_lo, scalar_hi, adder_lo, adder_hi, out_lo, out_hi;
  float delta_lo, delta_hi, denom_min, denom_zero;
} s3_bias_channel;
int s3_bias_correct(s3_ctx* ctx, const float* x, int n, int s1, int s2, int t, int c,
                    const s3_bias_channel* channels_host, int S1, int S2,
                    const int32_t* geom_host, const int32_t* month, const int32_t* window,
                    const double* weights, const double* mean_host, const double* std_host,
                    int stats_fp32, float* out, int32_t* nonfinite);

/* ---- computing bias-correction factors on the device -----------------------
 * the per-pixel work of sup3r/bias/bias_calc.py (LinearCorrection and its
 * monthly / scalar kin), qdm.py (QuantileDeltaMappingCorrection) and presrat.py:
 * the tables that the correction above applies.  Every series is fp32 (P, T),
 * pixel-major (P = the low-res grid, flattened).  Sums are fp64 and rounded to
 * fp32 once; each output value comes from one thread or from one workgroup's
 * fixed reduction tree; no float atomics.  Index lists come twice: a host copy
 * that is range-checked here before anything is launched, and the device copy
 * that the kernel reads.  All six are asynchronous on the context's stream.
 *
 * s3_bc_base_series: base (T, n_sites) -> out[p, day_offset + d], d < n_days:
 *   per step the mean over the pixel's sites (CSR site_ptr (P + 1) / site_idx;
 *   S3_BCC_NANSKIP: np.nanmean, a step whose sites are all NaN is NaN;
 *   otherwise a plain mean), then the reduction over the day's steps (CSR
 *   day_ptr (n_days + 1) / step_idx, any order of steps).  The reductions skip
 *   NaN steps like pandas' groupby: avg / max / min of a day without a valid
 *   step are NaN, its sum is 0; S3_BCC_NONE wants one step per output step.
 *   S3_BCC_CS_RATIO (avg only): daily sum of base over daily sum of cs_ghi,
 *   0 / 1 where the latter is 0 (base.py:745-749).  S3_BCC_ROUND: np.around(.,
 *   decimals) in fp32, round-half-even at the scaled value.  A pixel without
 *   sites gets NaN.  D_total is the row length of out: one launch per base
 *   file writes its days at day_offset.
 * s3_bc_moments: per (pixel, group) count / np.nanmean / np.nanstd (mean,
 *   then the mean of the squared deviations, ddof = 0) of the steps with
 *   group[t] == g; group[t] = -1 belongs to none; NT <= S3_BCC_MAX_GROUPS.  A
 *   group without a non-NaN member gives count 0 and NaN.  Outputs (P, NT).
 * s3_bc_window_quantiles: per (pixel, window) the members (CSR win_ptr (W + 1)
 *   / member, indices into the series) are sorted in LDS on an integer key in
 *   float order (-0 < +0, NaN last) and out (P, W, Q) receives np.quantile at
 *   np.linspace(0, 1, Q): order statistics interpolated linearly in fp64 at
 *   (n - 1) q.  q = 0 and q = 1 are the minimum and maximum exactly; Q = 1
 *   gives the minimum.  A window that is empty or holds a NaN gives a NaN row.
 * s3_bc_match_zero_rate (base.py:557-599): in place on bias (P, T): the
 *   pixel's sorted series, np.interp of the share of exact zeros of its base
 *   row (P, D) into np.linspace(0, 1, T) in fp64 (written to min_value (P),
 *   optional), and everything below that set to 0.  nonfinite: one int32 the
 *   number of non-finite bias values is added to; such a pixel is left as it
 *   is (the reference's sorted() on NaN is undefined).
 * s3_bc_presrat (presrat.py:96-360), per pixel and in the reference's order:
 *   the QDM-corrected future series (corrected (P, Tf), written always: step t
 *   is mapped with the rows of window last_window[t], the last window that
 *   holds it, and stays NaN for -1; the mapping is that of s3_bias_correct
 *   with delta_denom_min = zero_rate_threshold when relative, on the tables
 *   (P, W, Q) given); zero_rate (P) = the share of finite base values <=
 *   threshold (compared in fp32, as numpy does); tau = the order statistic
 *   min(round(rate Tb), Tb - 1) of the bias series, round half to even on the
 *   fp64 product; z_fg = #(fut < tau) / Tf; tau_fut (P) = the order statistic
 *   round(z_fg Tf) of the corrected series, NaN sorted last; k_factor (P, W)
 *   from the four plain (not NaN-skipping) window means floored at the
 *   threshold, in fp64.  tau and z_fg (P) are optional outputs.  The window
 *   lists come as three pointers each: base, bias, future.  status
 *   (S3_BCC_PR_STATUS_WORDS int32, zeroed here): non-finite bias values,
 *   non-finite future values, pixels whose round(z_fg Tf) = Tf (the
 *   reference's IndexError; their tau_fut is NaN).  Q >= 2.
 * s3_bc_skill (SkillAssessment._run_skill_eval, bias_calc.py:431-481), one
 *   workgroup per pixel over base (P, D) and bias (P, T), D, T <=
 *   S3_BCC_MAX_SORT.  stats (P, 2, S3_BCC_SK_STATS), series 0 = base, 1 =
 *   bias: np.nanmean and np.nanstd (two passes in fp64); scipy's biased skew
 *   m3 / m2^1.5 and Fisher kurtosis m4 / m2^2 - 3 over all n values in fp64
 *   about the fp64 mean (a NaN in the series gives NaN, and so does m2 <=
 *   (eps32 mean)^2: scipy's test for a constant float32 series); zero_rate =
 *   #(x == 0) / n, NaNs counted in n; np.percentile at S3_BCC_SK_PERCENTILES
 *   = 7 points (1, 5, 25, 50, 75, 95, 99) from the sorted keys, interpolated as
 *   s3_bc_window_quantiles does at (n - 1) p / 100, NaN where the series holds
 *   one; and in both rows S3_BCC_SK_BIAS = mean(bias) - mean(base), taken
 *   between the fp64 means and rounded once (the reference subtracts its two
 *   float32 means).  status (P, S3_BCC_SK_STATUS_WORDS): NaN and non-finite counts of
 *   base, then of bias.  ks (P, S3_BCC_SK_KS_WORDS): the two-sample
 *   Kolmogorov-Smirnov counts, exact: with c1(x) = #(base <= x), c2(x) =
 *   #(bias <= x) over all data points x (scipy's searchsorted(side='right')),
 *   (c1, c2) where c1 T - c2 D is largest, then (c1, c2) where it is smallest
 *   (the smallest c1 among ties; (0, 0) stands for "never below 0").  demean
 *   != 0: the values compared are x - m32 in fp32, m32 the series' own mean as
 *   stored in stats; values that the rounding merges tie, and so do -0 and
 *   +0.  All four words are S3_BCC_SK_NO_KS where either series holds a NaN
 *   or, with demean, a non-finite value (inf - inf).  sorted_base: (P, D)
 *   uint32 workspace; the base row's sorted keys rest there while the bias
 *   row is sorted in LDS (two rows at the limit do not fit together).
 *
 * S3_EINVAL, before anything is launched: a sorted segment longer than
 * S3_BCC_MAX_SORT (its keys fill 128 KiB of the CU's 160 KiB of LDS), a site,
 * step, member or group index out of range, lists that do not ascend, days
 * that leave out, Q < 1, NT outside 1 .. 12, 2^31 or more elements. */
#define S3_BCC_MAX_SORT 32768
#define S3_BCC_MAX_GROUPS 12
#define S3_BCC_AVG 0
#define S3_BCC_MAX 1
#define S3_BCC_MIN 2
#define S3_BCC_SUM 3
#define S3_BCC_NONE 4
#define S3_BCC_NANSKIP 1u
#define S3_BCC_CS_RATIO 2u
#define S3_BCC_ROUND 4u
#define S3_BCC_PR_STATUS_WORDS 3
#define S3_BCC_PR_BIAS_NONFINITE 0
#define S3_BCC_PR_FUT_NONFINITE 1
#define S3_BCC_PR_INDEX 2
#define S3_BCC_SK_PERCENTILES 7
#define S3_BCC_SK_STATS 13
#define S3_BCC_SK_MEAN 0
#define S3_BCC_SK_STD 1
#define S3_BCC_SK_SKEW 2
#define S3_BCC_SK_KURTOSIS 3
#define S3_BCC_SK_ZERO_RATE 4
#define S3_BCC_SK_PCT0 5
#define S3_BCC_SK_BIAS 12
#define S3_BCC_SK_KS_WORDS 4
#define S3_BCC_SK_STATUS_WORDS 4
#define S3_BCC_SK_NO_KS (-1)
int s3_bc_base_series(s3_ctx* ctx, const float* base, const float* cs_ghi, int64_t T, int64_t n_sites,
                      int P, const int32_t* site_ptr_host, const int32_t* site_idx_host,
                      const int32_t* site_ptr, const int32_t* site_idx, int n_days,
                      const int32_t* day_ptr_host, const int32_t* step_idx_host,
                      const int32_t* day_ptr, const int32_t* step_idx, int reduction, uint32_t flags,
                      int decimals, int64_t D_total, int64_t day_offset, float* out);
int s3_bc_moments(s3_ctx* ctx, const float* series, int P, int64_t T, const int32_t* group_host,
                  const int32_t* group, int NT, int32_t* count, float* mean, float* sd);
int s3_bc_window_quantiles(s3_ctx* ctx, const float* series, int P, int64_t T, int W,
                           const int32_t* win_ptr_host, const int32_t* member_host,
                           const int32_t* win_ptr, const int32_t* member, int Q, float* out);
int s3_bc_match_zero_rate(s3_ctx* ctx, const float* base, int64_t D, float* bias, int P, int64_t T,
                          double* min_value, int32_t* nonfinite);
int s3_bc_presrat(s3_ctx* ctx, const float* base, int64_t D, const float* bias, int64_t Tb,
                  const float* fut, int64_t Tf, int P, int W, int Q, const float* base_params,
                  const float* bias_params, const float* fut_params, int relative,
                  double zero_rate_threshold, const int32_t* last_window_host,
                  const int32_t* last_window, const int32_t* const* win_ptr_host,
                  const int32_t* const* member_host, const int32_t* const* win_ptr,
                  const int32_t* const* member, float* corrected, float* zero_rate, float* tau,
                  float* z_fg, float* tau_fut, float* k_factor, int32_t* status);
int s3_bc_skill(s3_ctx* ctx, const float* base, int64_t D, const float* bias, int64_t T, int P,
                int demean, uint32_t* sorted_base, float* stats, int32_t* ks, int32_t* status);

/* ---- deriving input features on the device --------------------------------
 * replaces the dask passes of sup3r/preprocessing/derivers (base.py,
 * methods.py, utilities.py) and Interpolator.interp_to_level
 * (sup3r/utilities/interpolation.py:13-173).  Features are PLANAR here: one
 * fp32 tensor (s1 s2, t) per feature, a multi-level variable (s1 s2, t, L),
 * levels innermost.  Element offsets are 64-bit.  Host tables (`_host`) are
 * copied into the kernel arguments: no upload, no synchronisation in a call.
 *
 * s3_level_interp: a column is one (pixel, step), n_col = s1 s2 t of them.  Its
 *   levels are the l_ml entries of the multi-level arrays followed by n_sl
 *   single-level planes.  Level values of the first l_ml: S3_LI_LEV_COLUMN —
 *   lev_ml (n_col, l_ml) minus, when topo is given, topo[column / t]
 *   (topo_per_step = 0, topo (s1 s2)) or topo[column] (topo_per_step = 1), one
 *   fp32 subtraction; S3_LI_LEV_VECTOR — lev_vec_host (l_ml) for every column.
 *   Those of the planes: sl_level_host (n_sl).  var_ml_host: n_var device
 *   pointers (n_col, l_ml); var_sl_host: n_var n_sl device pointers (n_col),
 *   variable-major; out_host: n_var n_out device pointers (n_col),
 *   variable-major.  Per (column, target) the two levels are chosen once, for
 *   all variables, by the rule of get_level_masks (interpolation.py:17-70) on
 *   d_i = |lev_i - target| over the levels that are not NaN, ties to the lowest
 *   index: i1 = argmin d over lev < target, without one argmin d over all; i2 =
 *   argmin d over lev >= target, without one argmin d over all but i1; an
 *   empty set gives index 0.  S3_LI_LINEAR (_lin_interp :73-92): alpha = |lev2
 *   - lev1| < 1e-3 ? 0 : (target - lev1) / (lev2 - lev1), out = var1 (1 - alpha)
 *   + var2 alpha, every operation rounded to fp32 on its own (numpy's result,
 *   bit for bit).  S3_LI_LOG: _log_interp (:95-112) in its order, fp32, logf.
 *   One launch writes the n_var n_out planes; every input element is read once
 *   (64 columns = one contiguous run, loaded 16 bytes per lane into LDS).
 *   S3_EINVAL, before anything is launched: l_ml + n_sl outside 1 ..
 *   S3_LI_MAX_LEVELS, n_sl > S3_LI_MAX_SINGLE, n_var outside 1 ..
 *   S3_LI_MAX_VARS, n_out outside 1 .. S3_LI_MAX_TARGETS, a missing pointer.
 * s3_derive_pointwise: out0 (, out1) (n_pix, t) from in0 (, in1), S3_DP_*:
 *   UV_FROM_WSWD  transform_rotate_wind (derivers/utilities.py:146-201): in =
 *                 windspeed, direction in degrees; out = u, v; cos_theta /
 *                 sin_theta (n_pix) are the grid angle's tables
 *   WSWD_FROM_UV  invert_uv (:204-258): in = u, v; out = speed, direction
 *   SURFACE_RH    methods.py:63-72: in = d2m, temperature_2m
 *   RATIO_MASKED  in0 / in1, NaN where step_flag[step] != 0 (methods.py:94-102)
 *   CLOUD_MASK    in0 < in1 as 0 / 1, NaN where flagged (:152-160)
 *   RATIO_CLIP01  max(min(in0 / in1, 1), 0), NaN kept (:128-130)
 *   ADD           in0 + in1
 *   SCALE         in0 p0
 *   OFFSET        in0 + p0
 *   BCAST_PIXEL   in0 (n_pix) along time
 *   BCAST_TIME    in0 (t) along the pixels
 *   All but the first three are single fp32 operations (numpy's bits).
 * s3_time_flags: flags (t) int32, zeroed here, then OR-ed: S3_TF_LE — any x[p,
 *   step, ch] <= threshold; S3_TF_NAN — any NaN; x is (n_pix, t, c).
 * s3_stack_features: out (n_pix, t, c)[p, j, ch] = planes_host[ch][p, (j -
 *   roll) mod t] (xr.Dataset.roll), c <= S3_STACK_MAX_PLANES.
 * s3_level_stats: what Interpolator._check_lev_array (interpolation.py:
 *   176-237) reports, of lev_ml (n_col, l_ml) minus topo as in
 *   s3_level_interp: stats (S3_LS_WORDS uint64 on the device, zeroed here) =
 *   the number of NaN levels, of columns without a NaN whose minimum is
 *   above lo_target, of such columns whose maximum is below hi_target, of
 *   all-NaN columns, and the extrema over the non-NaN values of the first
 *   and of the last level as order keys: S3_LS_*_MAX holds key(max),
 *   S3_LS_*_MIN holds 0xFFFFFFFF - key(min), key(v) = the float's bits with
 *   the sign bit set for v >= 0 and all bits inverted for v < 0; a word left
 *   at 0 means that every value of that level is NaN. */
#define S3_LI_MAX_LEVELS 64
#define S3_LI_MAX_SINGLE 8
#define S3_LI_MAX_VARS 8
#define S3_LI_MAX_TARGETS 16
#define S3_LI_LINEAR 0
#define S3_LI_LOG 1
#define S3_LI_LEV_COLUMN 0
#define S3_LI_LEV_VECTOR 1
#define S3_DP_UV_FROM_WSWD 0
#define S3_DP_WSWD_FROM_UV 1
#define S3_DP_SURFACE_RH 2
#define S3_DP_RATIO_MASKED 3
#define S3_DP_CLOUD_MASK 4
#define S3_DP_RATIO_CLIP01 5
#define S3_DP_ADD 6
#define S3_DP_SCALE 7
#define S3_DP_OFFSET 8
#define S3_DP_BCAST_PIXEL 9
#define S3_DP_BCAST_TIME 10
#define S3_TF_LE 0
#define S3_TF_NAN 1
#define S3_STACK_MAX_PLANES 32
#define S3_LS_WORDS 8
#define S3_LS_NAN 0
#define S3_LS_BAD_MIN 1
#define S3_LS_BAD_MAX 2
#define S3_LS_ALL_NAN 3
#define S3_LS_FIRST_MAX 4
#define S3_LS_FIRST_MIN 5
#define S3_LS_LAST_MAX 6
#define S3_LS_LAST_MIN 7
int s3_level_interp(s3_ctx* ctx, int64_t n_col, int64_t t, int l_ml, int n_sl, int lev_source,
                    const float* lev_ml, const float* lev_vec_host, const float* topo, int topo_per_step,
                    const float* sl_level_host, int n_var, const float* const* var_ml_host,
                    const float* const* var_sl_host, int n_out, const float* target_host, int method,
                    float* const* out_host);
int s3_derive_pointwise(s3_ctx* ctx, int op, int64_t n_pix, int64_t t, const float* in0, const float* in1,
                        const float* cos_theta, const float* sin_theta, const int32_t* step_flag, float p0,
                        float* out0, float* out1);
int s3_time_flags(s3_ctx* ctx, int mode, const float* x, int64_t n_pix, int64_t t, int c, float threshold,
                  int32_t* flags);
int s3_stack_features(s3_ctx* ctx, const float* const* planes_host, int c, int64_t n_pix, int64_t t,
                      int64_t roll, float* out);
int s3_level_stats(s3_ctx* ctx, const float* lev_ml, int64_t n_col, int64_t t, int l_ml, const float* topo,
                   int topo_per_step, float lo_target, float hi_target, uint64_t* stats);

/* ---- rasterising exogenous fields on the device ------------------------------
 * replaces the host scipy / pandas of BaseExoRasterizer (sup3r/preprocessing/
 * rasterizers/exo.py:294-458): KDTree(hr_lat_lon).query(source_lat_lon,
 * distance_upper_bound=r) and the group mean per target of _get_data_2d /
 * _get_data_3d.
 *
 * s3_exo_nearest: for each of n_src source points src (n_src, 2) fp32 (lat,
 * lon) the nearest of the n_tgt target points tgt (n_tgt, 2) fp32 (any
 * layout: the grid may be curvilinear) in the plain Euclidean distance of
 * the two coordinates, in degrees, as the reference's tree measures it (no
 * longitude wrap).  Arithmetic: the inputs widened to float64, d2 = dlat *
 * dlat + dlon * dlon (two roundings of the products, one of the sum, nothing
 * contracted); a target counts only if d2 < r * r, strictly; among equal d2
 * the smallest target id wins (the tree's own choice on an exact tie follows
 * its traversal: the one documented deviation).  nn[i] = the target id, n_tgt
 * for a miss; dist (may be NULL) [i] = sqrt(d2) as float64, +inf for a miss.
 * A NaN coordinate never matches: such a source is a miss, such a target is
 * nobody's neighbour.
 *   The search structure is built by the call, on the device, in work: the
 * targets' bounding box (integer-atomic extrema of order keys), a uniform
 * cell grid over it with cell side r (1 + 2^-16) — or larger: the side grows
 * until there are at most min(2 n_tgt + 1024, 2^30) cells; the result does
 * not depend on it —, an integer-atomic count per cell, a scan, a scatter of (lat, lon, id)
 * into cell order.  A source examines the 3 x 3 cells around its own (a
 * source outside the box: around the border cell it clamps to).
 *
 * s3_exo_group_mean: out[m, col_host[k]] = float32(float64(S) / n * scale)
 * for every target m < n_tgt and k < t_used, where S is the sum and n the
 * number of the values val[i, k] (val (n_src, t_used) fp32) that are no NaN
 * and have nn[i] == m (an nn[i] outside [0, n_tgt) is a miss); NaN bits where
 * n == 0.  out is (n_tgt, t_out) fp32; columns col_host does not name are not
 * written.  nan_count: one 64-bit device word, zeroed here: the number of NaN
 * cells written.
 *   S is accumulated in fixed point with integer atomics only, so the bits do
 * not depend on the order of arrival: a pre-pass takes E = floor(log2(max
 * |val|)) over the finite values of the call; every value is rounded to a
 * multiple of 2^(E - 61) (a 63-bit integer, exact for every value whose last
 * mantissa bit is worth that or more: |val| >= 2^(E - 38)), its low 32 bits
 * and the rest go to two 64-bit limbs per (target, column), which hold 2^31
 * such terms without a carry between them; lanes of a wave that follow one
 * another with the same target are summed before the atomic.  The sum of the
 * limbs is rounded once to float64.  Error of the mean against the exact one,
 * before the two roundings above: at most q = 2^(E - 62) <= 2^-62 max |val|.
 * Infinite values are not supported (they saturate; nothing faults).
 *   work holds S3_EXO_MAX_SLAB columns of limbs and counts at most; more
 * columns are processed in slabs.
 *
 * Both are asynchronous on the context's stream and upload nothing.  work is
 * at least what the *_work_bytes query returns, 8-byte aligned.  S3_EINVAL,
 * before anything is launched: n_src or n_tgt below 1 or 2^31 and above, r
 * that is not finite or not above 0, a missing pointer, work_bytes below the
 * query's figure, t_used or t_out below 1, t_used above t_out, a col_host
 * entry outside [0, t_out). */
#define S3_EXO_MAX_SLAB 32
int64_t s3_exo_nearest_work_bytes(int64_t n_tgt);
int s3_exo_nearest(s3_ctx* ctx, const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, double r,
                   void* work, int64_t work_bytes, int32_t* nn, double* dist);
int64_t s3_exo_group_mean_work_bytes(int64_t n_tgt, int64_t t_used);
int s3_exo_group_mean(s3_ctx* ctx, const int32_t* nn, const float* val, int64_t n_src, int64_t n_tgt,
                      int64_t t_used, int64_t t_out, const int32_t* col_host, double scale, void* work,
                      int64_t work_bytes, float* out, uint64_t* nan_count);

/* ---- non-neural downscalers on the device ------------
 * replaces the host scipy / Pillow of the reference's LinearInterp and
 * SurfaceSpatialMetModel (sup3r/models/linear.py, sup3r/models/surface.py):
 *   s3_st_interp         = st_interp (sup3r/models/utilities.py:161-212) of
 *                          every (obs, feature) field of LinearInterp.generate
 *                          (linear.py:124-171): x (n, s1, s2, t, c) -> y (n,
 *                          s1 s, s2 s, t t_enhance, c), trilinear with linear
 *                          extrapolation.  axes = device table: int32 source
 *                          index i0 of every output index of the three axes
 *                          (s1 s, s2 s, t t_enhance in that order), then their
 *                          fp32 fractions (host float64).  Axes of length 1
 *                          are refused, as the reference asserts.
 *   s3_resize2d          = PIL.Image.resize in mode 'F' of every (n, :, :, c)
 *                          plane (downscale_arr, surface.py:286-318, without
 *                          the bias fix): x (n, h, w, c) -> y (n, h s, w s, c),
 *                          c <= 32.  tab_h / tab_w = device coefficient tables
 *                          of the two axes (int32 lo[O], int32 cnt[O], fp32
 *                          w[O][k]: Pillow's precompute_coeffs, host float64);
 *                          lo_h_host / cnt_h_host = the host copy of the h
 *                          axis' lo / cnt (tile geometry); planes = scratch of
 *                          (3 c + 1) n h w floats.
 *   s3_surface_downscale = SurfaceSpatialMetModel.generate (surface.py:
 *                          578-713) on the whole batch: channel kinds
 *                          S3_SURF_*, pair_host[i] = the temperature channel
 *                          of humidity channel i (_get_temp_rh_ind, :212-248),
 *                          consts_host = {temp_lapse, w_delta_temp,
 *                          w_delta_topo, pres_div, pres_exp}, fix_bias
 *                          (fix_downscaled_bias, :250-284: hr -= R(C(hr) -
 *                          lr)), noise_host[c] = stdev of the uniform [0,
 *                          stdev) noise added to channel c (0: none; null: no
 *                          noise; Philox4x32-10 keyed by seed, counter (pixel,
 *                          channel, call)).  topo_lr (h, w) and topo_hr (h s,
 *                          w s) device fp32; g_hr = scratch of h s w s floats
 *                          (needed with pressure channels).  The high-res
 *                          field is written once (three launches with the bias
 *                          fix).  min_pres_host (optional): receives the
 *                          minimum of the final pressure channels before the
 *                          noise (+inf without any); the call then waits for
 *                          the stream. */
#define S3_SURF_OTHER 0
#define S3_SURF_TEMP 1
#define S3_SURF_PRES 2
#define S3_SURF_RH 3
int s3_st_interp(s3_ctx* ctx, const float* x, int n, int s1, int s2, int t, int c,
                 int s_enhance, int t_enhance, const void* axes, float* y);
int s3_resize2d(s3_ctx* ctx, const float* x, int n, int h, int w, int c, int s_enhance,
                const void* tab_h, const void* tab_w, const int* lo_h_host,
                const int* cnt_h_host, int k, float* planes, float* y);
int s3_surface_downscale(s3_ctx* ctx, const float* x, int n, int h, int w, int c,
                         int s_enhance, const void* tab_h, const void* tab_w,
                         const int* lo_h_host, const int* cnt_h_host, int k,
                         const int* kinds_host, const int* pair_host,
                         const float* consts_host, int fix_bias,
                         const float* noise_host, uint64_t seed, uint32_t call,
                         const float* topo_lr, const float* topo_hr, float* planes,
                         float* g_hr, float* y, float* min_pres_host);

/* ---- output epilogue on the device ----------------------
 * replaces the host numpy of OutputHandler._transform_output
 * (sup3r/writers/base.py:304-345) on a hi-res chunk (s1*s2, t, c) fp32:
 *   s3_invert_uv     = invert_uv_single_pair (writers/base.py:283-302) /
 *                      invert_uv (preprocessing/derivers/utilities.py:204-258):
 *                      rotate (u, v) by the grid angle theta(s1, s2) — its
 *                      cos / sin are device tables of s1*s2 floats — and
 *                      overwrite channel u_idx with the windspeed and v_idx
 *                      with the direction in degrees [0, 360).
 *   s3_clip_channels = enforce_limits(nn_fill=False) (sup3r/utilities/
 *                      utilities.py:155-220): per-channel clipping to
 *                      [min, max] (host arrays; +-inf = no limit). */
int s3_invert_uv(s3_ctx* ctx, float* data, int64_t n_sp, int64_t t, int c,
                 int u_idx, int v_idx, const float* cos_theta,
                 const float* sin_theta);
int s3_clip_channels(s3_ctx* ctx, float* data, int c, int64_t n_pos,
                     const float* min_host, const float* max_host);
/*   s3_range_mask / s3_fill_indexed = enforce_limits(nn_fill=True) (same lines)
 *                      + nn_fill_array (utilities.py:55-75): channel ch of the
 *                      (n_pos, c) chunk — mask[p] = 1 where the value is
 *                      outside [lo, hi] or NaN (the reference writes NaN there);
 *                      then data[p, ch] = data[src[p], ch] on the masked
 *                      positions.  src is the flattened index map of
 *                      scipy.ndimage.distance_transform_edt(mask,
 *                      return_indices=True) — the reference's own call, made by
 *                      the host on the boolean mask only; the field stays on
 *                      the device. */
int s3_range_mask(s3_ctx* ctx, const float* data, int c, int ch, int64_t n_pos,
                  float lo, float hi, unsigned char* mask);
int s3_fill_indexed(s3_ctx* ctx, float* data, int c, int ch, int64_t n_pos,
                    const unsigned char* mask, const int* src);

/* ---- QA of a forward pass on the device --------------------
 * replaces the host numpy of Sup3rQa.run (sup3r/qa/qa.py:467-514) and of the
 * distributions and spectra of sup3r/qa/utilities.py.
 *
 * s3_qa_recoarsen: the high-resolution field re-coarsened onto the source grid
 *   (get_dset_out -> spatial_coarsening(obs_axis=False) -> temporal_coarsening,
 *   qa.py:296-374), the error against the source and its summary, one read of
 *   the field.  hr is S3_QA_CUBE (H1, H2, HT, C) with channel_host[f] the
 *   channel of feature f, or S3_QA_TIME_FIRST (HT, H1, H2) (C = F = 1,
 *   channel_host unused).  method_host[f] is S3_TC_*.  true_host / syn_host /
 *   err_host are host arrays of F device pointers to planar (S1, S2, T) fp32
 *   fields (S = H / s_enhance, T = HT / t_enhance): syn = the re-coarsened
 *   field, err = syn - true.  Any of the three arrays, or an entry of syn_host /
 *   err_host, may be NULL; err and the summary need true.
 *   Arithmetic, separately rounded fp32 in this order (tests/qa_ref.py): per
 *   step the s row sums over j, their sum over i, a true division by
 *   float(s^2); then over the t_enhance steps: SUBSAMPLE step 0, TOTAL a sum
 *   with NaN as +0, AVERAGE that sum / float(t_enhance), MAX / MIN hand NaN on.
 *   summary (device, F x S3_QA_SUMMARY_WORDS doubles, or NULL): over the finite
 *   errors of feature f the count, sum e, sum |e|, sum e^2 and max |e|, the
 *   sums in fp64 folded in a fixed order (no float atomics: two runs give equal
 *   bits).  Offsets are 64-bit.
 *   S3_EINVAL, before anything is launched: s_enhance not dividing H1 or H2,
 *   t_enhance not dividing HT, an unknown method or layout, F outside 1 ..
 *   S3_QA_MAX_FEATURES, a channel outside the cube, t_enhance * C above 4096
 *   (cube), s_enhance above 64 or a t_enhance whose tile exceeds a workgroup's
 *   LDS (time-first).
 *
 * The distributions (direct_dist, gradient_dist, time_derivative_dist,
 * utilities.py:170-342) never store the transformed value d: element e of it is
 *   diff == 0:  x = v[e];  has_period: x = (x + period) % period
 *   diff != 0:  x = v[src + delta] - v[src], src = (e / inner_out) inner_in +
 *               e % inner_out (np.diff(axis=1): inner_out = (s2 - 1) t,
 *               inner_in = s2 t, delta = t; v[..., k:] - v[..., :-k]: t - k, t,
 *               k);  has_period: x = (x + half_period) % period - half_period
 *   d = x / scale
 * in numpy's float32 operations (`%` with the divisor's sign).  n = the number
 * of values of d, at most 2^31 - 1 (S3_EINVAL above).
 * s3_qa_select: the order statistics rank0 <= rank1 (0-based) of |d| by a radix
 *   select over its bit patterns, four passes of 8 bits, per-workgroup
 *   histograms in LDS, integer atomics; out (device, 4 words) = bits of the two
 *   values, the NaN count (NaN sorts last, as in numpy), 0.
 * s3_qa_hist: over the kept values (|d| < diff_max, or all that are not NaN
 *   with S3_QA_HIST_KEEP_ALL) S3_QA_HIST_STATS writes stats (device, 5
 *   doubles) = count, sum d^2 (fp64, fixed order), min, max, NaN count (the
 *   NaN count is always written); S3_QA_HIST_COUNTS writes counts[n_bins]
 *   (uint32, zeroed here) = np.histogram's over uniform bins: values outside
 *   [first_edge, last_edge] dropped, the scaled index ((d - first_edge) / denom)
 *   * n_bins in fp32, or from the division on in fp64 if `wide` (numpy's
 *   arithmetic when `range` is given), then the decrement / increment against
 *   edges (device, n_bins + 1 floats, numpy's), the last edge inclusive.
 *   n_bins <= S3_QA_MAX_BINS.
 * s3_qa_power_sum: out[l] (device, L doubles) = sum over (o, i) of re^2 + im^2
 *   of an (outer, L, inner) view, of both fields if re1 / im1 are given; fp64,
 *   fixed order.  By Parseval the mean over one axis of |fftn|^2 is this sum
 *   over the 1-D transform along the other axis (s3_dft_axis). */
#define S3_QA_CUBE 0
#define S3_QA_TIME_FIRST 1
#define S3_QA_MAX_FEATURES 16
#define S3_QA_SUMMARY_WORDS 5
#define S3_QA_MAX_BINS 4096
#define S3_QA_HIST_STATS 1
#define S3_QA_HIST_COUNTS 2
#define S3_QA_HIST_KEEP_ALL 4
int s3_qa_recoarsen(s3_ctx* ctx, const float* hr, int layout, int64_t H1, int64_t H2, int64_t HT, int C,
                    const int* channel_host, const int* method_host, int F, int s_enhance, int t_enhance,
                    const float* const* true_host, float* const* syn_host, float* const* err_host,
                    double* summary);
int s3_qa_select(s3_ctx* ctx, const float* v, int diff, int64_t n, int64_t inner_out, int64_t inner_in,
                 int64_t delta, int has_period, float period, float half_period, float scale,
                 int64_t rank0, int64_t rank1, uint32_t* out);
int s3_qa_hist(s3_ctx* ctx, const float* v, int diff, int64_t n, int64_t inner_out, int64_t inner_in,
               int64_t delta, int has_period, float period, float half_period, float scale, int flags,
               float diff_max, float first_edge, float last_edge, double denom, int wide, int n_bins,
               const float* edges, uint32_t* counts, double* stats);
int s3_qa_power_sum(s3_ctx* ctx, const float* re0, const float* im0, const float* re1, const float* im1,
                    int64_t outer, int L, int64_t inner, double* out);

/* ---- the data handlers on the device -----------------------
 * replaces the xarray / numpy of Rasterizer.rasterize_data,
 * DailyDataHandler._deriver_hook and DataHandlerNCforCC.get_clearsky_ghi /
 * scale_clearsky_ghi (sup3r/preprocessing/rasterizers/base.py, extended.py,
 * data_handlers/base.py, nc_cc.py).  All four are asynchronous on the
 * context's stream, use 64-bit element offsets and no float atomics.
 *
 * s3_raster_gather: n_planes <= S3_STACK_MAX_PLANES planes per launch, src_host
 *   / out_host host arrays of device pointers; out is (n_i, n_j, n_k [, n_lev])
 *   fp32, t-contiguous; every bit pattern is copied as it is.
 *   S3_RG_GRID     src (src_s1, src_s2, src_t [, n_lev]):
 *                  out[i, j, k, l] = src[r0 + i, c0 + j, t0 + k step, l]
 *                  (a 2-D plane: src_t = n_k = 1, t0 = 0)
 *   S3_RG_FLAT     src (src_t, src_s2 sites), site (device, n_i n_j int32):
 *                  out[i, j, k] = src[t0 + k step, site[i n_j + j]]
 *                  (src_s1 = n_lev = 1)
 *   S3_RG_FLAT_1D  src (src_s2 sites): out[i, j] = src[site[i n_j + j]]
 *                  (n_k = 1)
 *   A cell whose site lies outside [0, src_s2) gets zero bits.  S3_EINVAL,
 *   before anything is launched: a window or a step outside the source.
 * s3_daily_reduce: sources (n_pix, n_days w), outputs (n_pix, n_days); output o
 *   is op out_op_host[o] of the non-NaN values of each window of source
 *   out_src_host[o].  Sums are fp64 in step order, rounded to fp32 once;
 *   S3_DAILY_MEAN divides in fp64 by the count (0 / 0 = NaN), then rounds;
 *   MAX / MIN are the element itself (NaN for a window of NaNs); SUM of such a
 *   window is 0; S3_DAILY_RATIO is the fp32 quotient of the fp32-rounded sums
 *   of the sources out_src_host[o] and out_src2_host[o].  A source is read once
 *   per launch.  n_src <= S3_DAILY_MAX_SRC, n_out <= S3_DAILY_MAX_OUT, w < 8192.
 * s3_site_day_mean: src (t_src, n_sites), idx (device, n_pix x k int32),
 *   day_map (device, d_out int32): out[p, d] = NaN where day_map[d] < 0 or the
 *   day lies behind the source's last whole day; else the mean over the m
 *   steps t_lo + day_map[d] m + s of (the mean over the k sites, NaN skipped),
 *   NaN skipped; fp64 throughout, one rounding.
 * s3_scale_to_time_max: scale[p] = nanmax_t a[p, :] / nanmax_t b[p, :] (one
 *   fp32 division), then b[p, :] *= scale[p] in place; a is only read. */
#define S3_RG_GRID 0
#define S3_RG_FLAT 1
#define S3_RG_FLAT_1D 2
#define S3_DAILY_MAX_SRC 8
#define S3_DAILY_MAX_OUT 16
#define S3_DAILY_MEAN 0
#define S3_DAILY_MAX 1
#define S3_DAILY_MIN 2
#define S3_DAILY_SUM 3
#define S3_DAILY_RATIO 4
int s3_raster_gather(s3_ctx* ctx, int layout, int n_planes, const float* const* src_host,
                     float* const* out_host, int64_t n_i, int64_t n_j, int64_t n_k, int64_t n_lev,
                     int64_t src_s1, int64_t src_s2, int64_t src_t, int64_t r0, int64_t c0, int64_t t0,
                     int64_t step, const int32_t* site);
int s3_daily_reduce(s3_ctx* ctx, int n_src, const float* const* src_host, int64_t n_pix, int64_t n_days,
                    int w, int n_out, const int* out_src_host, const int* out_src2_host,
                    const int* out_op_host, float* const* out_host);
int s3_site_day_mean(s3_ctx* ctx, const float* src, int64_t t_src, int64_t n_sites, const int32_t* idx,
                     int64_t n_pix, int k, int64_t t_lo, int m, const int32_t* day_map, int64_t d_out,
                     float* out);
int s3_scale_to_time_max(s3_ctx* ctx, const float* a, float* b, int64_t n_pix, int64_t t, float* scale);

/* ---- regridding the low-res member of a dual pair -----------
 * replaces rex's Regridder as DualRasterizer.update_lr_data calls it
 * (sup3r/preprocessing/rasterizers/dual.py:187-222): a BallTree over the
 * source points in the haversine metric, queried with k = 4, inverse-distance
 * weights, a weighted sum of whole time rows; and the NaN count of
 * check_regridded_lr_data (:224-249), from the same pass.  The arithmetic is
 * restated in tests/regrid_ref.py and is UNVERIFIED against rex, which was
 * not at hand.
 *
 * s3_regrid_knn: for each of the n_tgt points tgt (n_tgt, 2) fp32 (lat, lon,
 * degrees) the k sources (1 <= k <= S3_REGRID_MAX_K) of src (n_src, 2) fp32
 * with the smallest haversine distance — the exact k nearest, no
 * approximation.  Arithmetic: the inputs widened to float64 and multiplied by
 * pi / 180 (numpy's deg2rad), h = sin^2((lat_t - lat_s) / 2) + cos(lat_t)
 * cos(lat_s) sin^2((lon_t - lon_s) / 2) (scikit-learn's order, h capped at
 * 1), d = 2 asin(sqrt(h)), nothing contracted.  Candidates are ordered by
 * (d, source id): the smallest id wins an exact tie (the tree's own choice
 * follows its traversal: the one documented deviation, as s3_exo_nearest).
 * idx_out (n_tgt, k) int32, ascending in that order; dist_out (n_tgt, k)
 * float64 radians, may be NULL; w_out (n_tgt, k) fp32: d32 = float32(d),
 * floored at 1e-12f, w = 1 / d32, w / (w_0 + w_1 + ... left to right), every
 * operation a correctly rounded fp32 one.
 *   The search structure is built by the call, on the device, in work: the
 * boxes of sources and targets (integer-atomic extrema of order keys; the
 * host reads these 64 bytes back and lays out the grid, so the call waits for
 * the stream once), a cell grid over the sources' box with about two sources
 * per cell, an integer-atomic count per cell, a scan, a scatter of (lat, lon,
 * cos(lat), id) into cell order.  A target searches square rings of cells
 * around its own (the border cell it clamps to when it lies outside the box:
 * such a target is legal and extrapolates from its nearest sources) until its
 * k-th distance is below min(dlat to the edges of the rectangle searched,
 * asin(cos(lat_t) sin(dlon to its edges))), less a margin of 2^-20 of the
 * bound and 1e-12.  The grid has a single longitude cell (latitude bands,
 * the dlat bound alone) when the longitudes of sources and targets together
 * span more than 180 degrees or any |lat| exceeds 85 degrees; every candidate
 * of a cell is measured with the full haversine, so the date line and the
 * poles are no special case.  The result does not depend on the grid.
 *
 * s3_regrid_apply: out[v][j, t] = float32(sum_k float64(w[j, k]) *
 * float64(src[v][idx[j, k], t])) for t < T_out <= T_src (the reference's crop
 * lr[..., :T_required], fused), v < n_var; src planes (n_src, T_src), out
 * planes (n_tgt, T_out), src_planes_host / out_planes_host host arrays of
 * n_var device pointers (more than 8 variables are split into launches
 * here).  Every product is exact in fp64; the sum starts from the first
 * product, runs in rank order k = 0, 1, .. and is rounded to fp32 once, so
 * the bits depend on nothing else (np.einsum over float32 accumulates in
 * float32: a documented deviation).  NaN propagates.  nan_count (device,
 * n_var int64, zeroed here) receives the number of NaN elements written per
 * variable, one integer atomic per workgroup.  Indices are the library's own:
 * one outside [0, n_src) is not checked on the device.
 *
 * Both use 64-bit element offsets and no float atomics, run on the context's
 * stream and upload nothing; s3_regrid_apply is asynchronous.  S3_EINVAL,
 * before anything is launched: n_src or n_tgt outside 1 .. 2^31 - 1, k
 * outside 1 .. S3_REGRID_MAX_K, n_src < k, a missing or misaligned pointer,
 * work_bytes below s3_regrid_knn_work_bytes(n_src) (work 8-byte aligned),
 * n_var < 1, T_out < 1 or T_out > T_src.  A coordinate that is not finite is
 * S3_EINVAL too, found by the box pass: nothing else has been launched and no
 * output has been written by then. */
#define S3_REGRID_MAX_K 8
int64_t s3_regrid_knn_work_bytes(int64_t n_src);
int s3_regrid_knn(s3_ctx* ctx, const float* src_lat_lon, int64_t n_src, const float* tgt_lat_lon, int64_t n_tgt,
                  int k, void* work, int64_t work_bytes, int32_t* idx_out, double* dist_out, float* w_out);
int s3_regrid_apply(s3_ctx* ctx, int n_var, const float* const* src_planes_host, float* const* out_planes_host,
                    int64_t n_src, int64_t n_tgt, int64_t T_src, int64_t T_out, int k, const int32_t* idx,
                    const float* w, int64_t* nan_count);

/* ---- data-parallel gradient sync (RCCL over xGMI) -----------------------
 * replaces: the host-side python sum of per-GPU gradient lists,
 * AbstractSingleModel._sum_parallel_grad (abstract.py:785-805): elementwise
 * SUM over ranks of the flat gradient buffer, one ncclAllReduce. */
int s3_comm_unique_id(void* out128); /* rank 0; 128 bytes                  */
int s3_comm_init(s3_ctx* ctx, int rank, int nranks, const void* unique_id128);
int s3_params_allreduce_grads(s3_params* p);
int s3_allreduce_sum(s3_ctx* ctx, float* buf, int64_t n);
/* the communicator as RCCL reports it (ncclCommCount / ncclCommUserRank; 1 / 0
 * without one): what a multi-GPU bench line prints so that the first run on
 * real xGMI verifies itself. */
int s3_comm_info(s3_ctx* ctx, int* n_ranks, int* rank);
/* Overlap with the backward pass: arm the store BEFORE the s3_plan_backward
 * call that finalises its gradients (need_wgrad; the last one when several
 * accumulate).  That call then hands the finished tail of the gradient buffer
 * to RCCL bucket by bucket (>= bucket_bytes each; 0: one bucket) on a second
 * stream behind an event, so the xGMI traffic runs under the remaining
 * gradient kernels; the following s3_params_allreduce_grads only joins the two
 * streams.  Every rank arms the same store with the same bucket size.
 * The backward pass CONSUMES the arming (also when it fails), bucket_bytes < 0
 * disarms, and a context without a communicator is never armed: no later
 * backward pass on the store can issue a collective the other ranks do not.
 * A parameter layout whose offsets do not grow with the op order gets one
 * reduction after the last op instead of buckets. */
int s3_params_arm_allreduce(s3_params* p, int64_t bucket_bytes);
/* replicas must start from identical weights (the reference's towers read ONE
 * set of tf.Variables, abstract.py:827-841): ncclBroadcast of a store buffer
 * (S3_BUF_*) / any fp32 buffer from rank `root` */
int s3_params_broadcast(s3_params* p, int which, int root);
int s3_broadcast(s3_ctx* ctx, float* buf, int64_t n, int root);
void s3_comm_destroy(s3_ctx* ctx);
/* Watchdog of the collectives: bounded host wait for everything enqueued on
 * the context's streams so far (the data-parallel step reads its loss scalars
 * back once per batch, abstract.py:843-914 — this is that wait, with a
 * deadline).  While waiting it polls ncclCommGetAsyncError.  On a timeout or
 * an asynchronous RCCL error the communicator is aborted (ncclCommAbort: a
 * rank stuck in a collective whose peer died never returns otherwise), the
 * context falls back to single-rank state and S3_ETIMEOUT / S3_ERCCL comes
 * back with s3_last_error naming what was pending.  timeout_ms < 0: no
 * deadline (plain s3_ctx_sync + the error poll). */
int s3_comm_wait(s3_ctx* ctx, int64_t timeout_ms);

/* library / build information */
const char* s3_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SUP3R_HIP_H */
