// The backward pass of a plan: the op list in reverse, each conv on the weight
// and data gradient kernels chosen for it (plan.cpp), with the hand-over of
// finished gradients between neighbours (BwdState) and the bucketed all-reduce
// of the parameter gradients under it.
#include <algorithm>
#include <cassert>
#include <cstdio>

#include "plan_internal.h"

// ------------------------------------------------------------------ backward
// does the pass need dL/d(tensor id)?  (an input's only when the caller asked for it)
static bool wants_grad(const s3_plan* pl, int id) {
  const int r = root_of(pl, id);
  return !pl->t[r].is_input || r == pl->bw.dx_root;
}

// conv `prod` is processed right after conv `cons` in the reverse walk
// (nothing but views in between): a bf16-ONLY dPre handed from one to the
// other, with its channel sums in pl->bsum, cannot be clobbered on the way
static bool back_to_back(const s3_plan* pl, int prod, int cons) {
  if (prod < 0 || prod >= cons) return false;
  for (int k = prod + 1; k < cons; ++k)
    if (pl->ops[k].d.kind != S3_OP_VIEW) return false;
  return true;
}

// may a kernel leave the gradient of tensor root r in pl->dpre16 (as the bf16
// copy, or as the only copy)?  The ONE test in front of every launch that
// stores there and of every BwdState::claim_dpre16: the buffer exists, no
// other tensor's pending gradient is in it, and it is large enough.
// plan_dpre16 sizes it by the outputs of the convs with OpRec::use16 (and
// the inputs of the stride-2 data gradients that store bf16 only), so a plan
// may well hold a tensor that does not fit: a copy written without the size
// test ran past the end of the buffer (sup3rcc/gen_solar_1x_8x_1f at 8 or 16
// samples of (54, 54, 3): non-finite gradients, then a memory access fault).
static bool dpre16_free_for(const s3_plan* pl, int r) {
  return pl->dpre16 && pl->bw.dpre16_for < 0 && pl->dpre16_bytes >= (size_t)pl->t[r].numel * 2;
}
// Two callers used to rely on the plan's sizing instead of testing the size: the
// tensor is the output of a conv with use16, which plan_dpre16 counted.
static bool dpre16_free_for_out_of(const s3_plan* pl, const OpRec& o) {
  const int r = root_of(pl, o.d.out);
  assert(!o.use16 || !pl->dpre16 || pl->dpre16_bytes >= (size_t)pl->t[r].numel * 2);
  return o.use16 && dpre16_free_for(pl, r);
}

// deliver a gradient contribution `src` (numel floats) to tensor `id`.
// The first contribution that lives in another finished buffer (the gradient
// of a consumer's output: skip adds, residuals, views) is not copied: the
// tensor's gradient aliases it (state 2) until a second contribution arrives,
// which then lands as one add / in-place accumulate instead of copy + axpy.
static int grad_deliver(s3_plan* pl, int id, const float* src) {
  const int r = root_of(pl, id);
  TensorRec& t = pl->t[r];
  s3_ctx* ctx = pl->ctx;
  BwdState& bw = pl->bw;
  if (!bw.gwritten[r]) {
    if (src == t.gptr) bw.gwritten[r] = 1;
    else bw.alias(r, src);
    return S3_OK;
  }
  if (bw.dpre16_for == r && src != t.gptr) {
    // the tensor changes: its bf16 copy is stale (a bf16-only tensor has no fp32 to add to)
    if (bw.dpre16_only) S3_FAIL(ctx, S3_ESTATE, "backward: second contribution to a bf16-only gradient");
    bw.release_dpre16();
  }
  if (bw.gwritten[r] == 2) {
    bw.drop_bsum(r);   // the tensor changes: its channel sums are stale
    const float* first = bw.take_alias(r);
    if (src == t.gptr) return launch_axpy(ctx, first, t.gptr, t.numel);
    return launch_add(ctx, first, src, t.gptr, t.numel, 1, 0);
  }
  if (src == t.gptr) return S3_OK;  // accumulated in place by the producer
  bw.drop_bsum(r);
  return launch_axpy(ctx, src, t.gptr, t.numel);
}

// destination a backward kernel should write dL/d(tensor id) into
static float* grad_dest(s3_plan* pl, int id) {
  const int r = root_of(pl, id);
  return pl->bw.gwritten[r] == 1 ? pl->gtmp : pl->t[r].gptr;
}

// the finished gradient of tensor root r
static const float* grad_of(s3_plan* pl, int r) {
  return pl->bw.gwritten[r] == 2 ? pl->bw.gsrc[r] : pl->t[r].gptr;
}

// Option WGRAD_SIDE_STREAM.  A launch-bound backward pass is a chain of
// dependent launches (>= 4.6 us each on this part); the weight gradient of a
// conv is not on that chain — nothing in the pass reads it — so it can go to a
// side stream that forks off the compute stream where its operands are final
// and joins before s3_plan_backward returns (inside a stream capture: a
// parallel branch of the graph).  Measured on C1 (48 forks per mini-batch):
// 2.37 -> 2.90 ms eager, 2.38 -> 2.89 ms as a recorded graph — a cross-stream
// dependency costs more than the 6 us kernel it takes off the chain — so it is
// off unless asked for (profiles/r04/README.md).
static int wg_fork(s3_ctx* ctx, hipStream_t* side) {
  if (!ctx->wg_stream) {
    S3_HIP(ctx, hipStreamCreateWithFlags(&ctx->wg_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) S3_HIP(ctx, hipEventCreateWithFlags(&ctx->wg_ev[k], hipEventDisableTiming));
  }
  S3_HIP(ctx, hipEventRecord(ctx->wg_ev[0], ctx->stream));
  S3_HIP(ctx, hipStreamWaitEvent(ctx->wg_stream, ctx->wg_ev[0], 0));
  ctx->wg_forked = true;
  *side = ctx->wg_stream;
  return S3_OK;
}
static int wg_join(s3_ctx* ctx) {
  if (!ctx->wg_forked) return S3_OK;
  ctx->wg_forked = false;
  S3_HIP(ctx, hipEventRecord(ctx->wg_ev[1], ctx->wg_stream));
  S3_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->wg_ev[1], 0));
  return S3_OK;
}

// what the gradient kernels of a conv read as dPre = dL/d(pre-activation)
struct DPre {
  const float* f32 = nullptr;     // nullptr: not written (every reader takes bf16); holds nothing when only16
  const void* bf16 = nullptr;     // nullptr: no bf16 copy
  bool only16 = false;            // bf16 is the ONLY copy (left by the consumer's fold / stride-2 data gradient)
  bool mask_sums = false;         // pl->bsum2 holds its channel sums
  const float* mask_y = nullptr;  // one-launch fewpos kernels: f32 is dy, the activation's adjoint is
  float slope = 0.f;              // applied as they read it (from y, like the mask pass)
};

// Does this conv's weight gradient kernel read dPre as bf16?  One fact per
// Wgrad value, asked at three places that do NOT want the same answer:
//
//   wgrad       GUARD                       SKIP                DISPATCH
//   BF16_TRUNK  use16                       in16 && Cout%4==0   in16 && Cout%4==0
//   BF16_2D     use16 && in16 && s0==1      never               in16 && s0==1 && Cout%4==0
//               && Cout%4==0                                    && Cin%8==0
//   C2          yes                         never               never
//   the rest    never                       never               never
//
// (in16 = the conv's input tensor is bf16.)  GUARD: a bf16-ONLY dPre arrived
// from the consumer; the conv cannot run without this.  SKIP: the mask pass
// may leave the fp32 dPre unwritten.  DISPATCH: a bf16 copy exists NEXT TO
// the fp32 one; which to hand to the kernel (a bf16-only dPre is handed over
// whatever this says: GUARD has passed).
enum class Dy16 { GUARD, SKIP, DISPATCH };
static bool wgrad_takes_bf16(const OpRec& o, Dy16 at) {
  const ConvGeom& g = o.cg;
  const bool in16_c4 = o.io.in_bf16 && (g.Cout & 3) == 0;
  switch (o.wgrad) {
    case Wgrad::BF16_TRUNK: return at == Dy16::GUARD ? o.use16 : in16_c4;
    case Wgrad::BF16_2D:
      if (at == Dy16::SKIP || !in16_c4 || g.s[0] != 1) return false;
      return at == Dy16::GUARD ? o.use16 : (g.Cin & 7) == 0;
    case Wgrad::C2: return at == Dy16::GUARD;
    default: return false;
  }
}

// 64 -> C_out > 64: the slices of the chunked data gradient read the bf16
// copy of dPre when they run on the persistent kernel (given there is one)
static bool chunked_dgrad_persist16(const s3_ctx* ctx, const OpRec& o) {
  const int nk = (o.cg.Cout + 63) / 64;
  return o.use16 && conv_mfma_persist_dgrad_supported(ctx, conv_dgrad_chunk_geom(o.cg, 0)) &&
         conv_mfma_persist_dgrad_geom_ok(conv_dgrad_chunk_geom(o.cg, nk - 1));
}

// the reflect / zero frame of `lo` cells around a conv's input, as the pad op
// whose adjoint folds the data gradient over the frame back onto x's grid
static GatherGeom frame_fold_geom(const ConvGeom& g, const int lo[3]) {
  GatherGeom fg;
  fg.kind = S3_OP_PAD; fg.N = g.N;
  for (int q = 0; q < 3; ++q) { fg.Di[q] = g.D[q]; fg.Do[q] = g.D[q] + 2 * lo[q]; fg.lo[q] = lo[q]; }
  fg.Ci = g.Cin; fg.Co = g.Cin; fg.pad_mode = g.pad_mode;
  fg.rep = 1; fg.d2s = 1; fg.c_off = 0;
  return fg;
}

// The fold's output is (so far) the whole gradient of tensor rin, whose
// producer is a conv without activation that stages bf16: may the fold leave
// it a bf16 copy?  (grad_deliver drops the copy if a second contribution
// arrives; dpre16_free_for holds the size test and why it is there)
static bool fold_side16_ok(const s3_plan* pl, const OpRec& o, int rin) {
  if (o.in_prod < 0 || s3_opt_has(S3O_NO_FOLD16) || !dpre16_free_for(pl, rin)) return false;
  const OpRec& po = pl->ops[o.in_prod];
  return po.use16 && po.cg.act == S3_ACT_NONE && po.cg.d2s <= 1 && (po.cg.Cout & 3) == 0;
}

// the adjoint of a gather op, or the fold of an fp32 frame, with nothing fused
static int fold_plain(s3_ctx* ctx, const GatherGeom& g, const float* dout, float* din) {
  FoldJob job;
  job.frame = dout; job.din = din;
  return launch_fold(ctx, g, job);
}

// Backward of conv i in stages — dPre, bias + weight gradient, data gradient
// (+ the fold of its frame) — that hand each other `dp` and nothing else;
// what outlives the conv is in pl->bw.
struct ConvBwd {
  s3_plan* const pl;
  const int i;
  OpRec& o;
  const s3_op_desc& d;
  const ConvGeom& g;
  s3_ctx* const ctx;
  BwdState& bw;
  const uint64_t version;   // of the weights
  const bool x3;
  const int ro, rin;        // tensor roots of the output / the input
  const bool want_dx;
  DPre dp;
  // The one-launch fewpos kernels: when the weight AND the data gradient are
  // these, both go out as ONE launch, at the data gradient's place
  ConvGeom fp_gd;           // geometry of that data gradient (a reflect conv: over the padded frame)
  bool fp_both = false;

  ConvBwd(s3_plan* pl_, int i_)
      : pl(pl_), i(i_), o(pl_->ops[i_]), d(o.d), g(o.cg), ctx(pl_->ctx), bw(pl_->bw), version(pl_->params->version),
        x3(pl_->precision == S3_PREC_BF16X3), ro(root_of(pl_, d.out)), rin(root_of(pl_, d.in0)),
        want_dx(wants_grad(pl_, d.in0)) {}

  // dy = the finished gradient of the conv's output
  int run(const float* dy) {
    int rc = S3_OK;
    if (d.res >= 0 && wants_grad(pl, d.res)) rc = grad_deliver(pl, d.res, dy);
    if (!rc) rc = dpre(dy);
    if (rc) return rc;
    fp_gd = g.pad_mode == S3_PAD_REFLECT ? conv_fewpos_frame_geom(g) : g;
    fp_both = bw.need_wgrad && dp.f32 != nullptr && o.wgrad == Wgrad::FEWPOS_MFMA && o.dgrad == Dgrad::FEWPOS_MFMA &&
              want_dx && !s3_opt_has(S3O_WGRAD_SIDE_STREAM) && !s3_opt_has(S3O_NO_FEWPOS_BWD_FUSE) &&
              conv_fewpos_bwd_mfma_ok(ctx, g, fp_gd);
    if (bw.need_wgrad && !fp_both) rc = wgrad();
    if (rc || !want_dx) return rc;
    float* dst = grad_dest(pl, d.in0);
    rc = dgrad(dst);
    if (rc) return rc;
    return grad_deliver(pl, d.in0, dst);
  }

  int dpre(const float* dy) {
    dp.f32 = dy;
    switch (bw.take_dpre16(ro)) {
      case BwdState::ONLY:
        // written as bf16 ONLY by the consumer (fold_frame, dgrad_s2): the fp32
        // buffer behind dy holds nothing — every reader below takes the bf16
        // one (the consumer made sure they all can)
        dp.only16 = true;
        dp.bf16 = pl->dpre16;
        if (!wgrad_takes_bf16(o, Dy16::GUARD) || (o.wgrad == Wgrad::C2 && !dgrad_is_c2(o.dgrad) && want_dx) || d.res >= 0)
          S3_FAIL(ctx, S3_ESTATE, "backward: bf16-only dPre reached a conv that needs fp32");
        break;
      case BwdState::COPY:
        // fp32 tensor + bf16 copy (fold + earlier contribution of a skip tensor):
        // dPre = dy for a conv without activation
        if (o.use16 && g.act == S3_ACT_NONE && g.d2s <= 1 && dy == pl->t[ro].gptr) dp.bf16 = pl->dpre16;
        break;
      case BwdState::NONE: break;
    }
    // (both readers of dPre must be the one-launch kernels: the data gradient
    // of a fewpos conv may still run on another family)
    if (o.fam == Fam::FEWPOS_MFMA && (o.dgrad == Dgrad::FEWPOS_MFMA || !want_dx) &&
        g.d2s <= 1 && !o.io.out_bf16 && pl->t[ro].dtype == 0 &&
        (g.act == S3_ACT_LEAKY || g.act == S3_ACT_RELU) && !bw.premasked[ro] && !dp.only16 &&
        !s3_opt_has(S3O_NO_MASK_FUSE)) {
      dp.mask_y = (const float*)tptr(pl, d.out);
      dp.slope = g.act == S3_ACT_LEAKY ? g.alpha : 0.f;
    }
    if ((g.act != S3_ACT_NONE || g.d2s > 1) && !bw.premasked[ro] && !dp.mask_y) return mask_pass(dy);
    return S3_OK;
  }

  // the activation / depth-to-space adjoint as a pass of its own: dy -> dPre
  int mask_pass(const float* dy) {
    const int need_wgrad = bw.need_wgrad;
    // (never over a pending bf16-only dPre of another tensor)
    void* side = (dpre16_free_for_out_of(pl, o) && conv_epilogue_bwd_d16_ok(g) && (g.d2s <= 1 || o.io.out_bf16))
                     ? pl->dpre16 : nullptr;
    // the bias gradient = channel sums of dpre: they ride along this pass
    dp.mask_sums = need_wgrad && d.b >= 0 && pl->bsum2 && conv_epilogue_bwd_bsum_ok(g) &&
                   (g.d2s <= 1 || (side && o.io.out_bf16)) && !s3_opt_has(S3O_NO_BIAS_FUSE);
    // Every reader of this dPre takes the bf16 copy — transpose-read /
    // wave-specialised weight gradient, MFMA data gradient over the frame
    // (chunked: on the persistent kernel), bias gradient from the channel
    // sums riding along: the fp32 dPre (151 MB per trunk conv at C2 batch 8)
    // is not written.
    const int64_t n_el = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout;
    const bool dg16 = (o.dgrad == Dgrad::MFMA_FRAME || o.dgrad == Dgrad::MFMA_VALID || o.dgrad == Dgrad::GEN) && o.use16;
    const bool dgc16 = dgrad_is_chunked(o.dgrad) && side && (g.Cout & 7) == 0 && chunked_dgrad_persist16(ctx, o);
    const bool skip32 = side && pl->precision == S3_PREC_BF16 &&
                        (g.d2s <= 1 ? ((n_el & 3) == 0 && (g.act == S3_ACT_LEAKY || g.act == S3_ACT_RELU))
                                    : o.io.out_bf16) &&
                        (!need_wgrad || (wgrad_takes_bf16(o, Dy16::SKIP) && (d.b < 0 || dp.mask_sums))) &&
                        (!want_dx || dg16 || dgc16) && !s3_opt_has(S3O_NO_DPRE16_ONLY_MASK);
    float* out32 = skip32 ? nullptr : pl->dpre;
    dp.f32 = out32;
    dp.bf16 = side;
    return launch_conv_epilogue_bwd(ctx, g, tptr(pl, d.out), dy, out32, o.io.out_bf16, side,
                                    dp.mask_sums ? pl->bsum2 : nullptr);
  }

  int bias() {
    float* db = gparam(pl, d.b);
    // (its launch rides along the reduction of a bf16-family weight gradient)
    const bool ride = o.wgrad == Wgrad::BF16_2D || o.wgrad == Wgrad::BF16_GEN || o.wgrad == Wgrad::BF16_TRUNK;
    if (dp.mask_sums)
      return launch_bias_grad_from_partial(ctx, pl->bsum2, conv_epilogue_bwd_blocks(ctx, g, true), g.Cout, db,
                                           bw.accumulate_wgrad, ride);
    if (bw.bsum_for == ro && dp.f32 == pl->t[ro].gptr && bw.gwritten[ro] == 1)
      return launch_bias_grad_from_partial(ctx, pl->bsum, bw.bsum_nblk, g.Cout, db, bw.accumulate_wgrad, ride);
    if (dp.only16) S3_FAIL(ctx, S3_ESTATE, "backward: bf16-only dPre without its channel sums");
    return launch_bias_grad(ctx, dp.f32, (int64_t)g.N * g.O[0] * g.O[1] * g.O[2], g.Cout, db, bw.accumulate_wgrad);
  }

  // few positions: the one-launch weight gradient leaves the bias gradient too
  int wgrad_fewpos() {
    const s3_params* P = pl->params;
    // beside the data-gradient chain when dPre is a tensor's own gradient
    // buffer (final by now; the shared scratch buffers are rewritten by
    // the ops that follow) and no collective reads G under this pass
    const bool side = dp.f32 != pl->dpre && dp.f32 != pl->gtmp && dp.f32 != pl->dxp && !ctx->comm &&
                      !(P->armed || P->reduced) && s3_opt_has(S3O_WGRAD_SIDE_STREAM);
    hipStream_t main_stream = ctx->stream, ws = nullptr;
    if (side) {
      int rc = wg_fork(ctx, &ws);
      if (rc) return rc;
      ctx->stream = ws;
    }
    int rc = launch_conv_fewpos_wgrad_mfma(ctx, g, tptr(pl, d.in0), dp.f32, gparam(pl, d.w), gparam(pl, d.b),
                                           bw.accumulate_wgrad, dp.mask_y, dp.slope);
    ctx->stream = main_stream;
    return rc;
  }

  int wgrad() {
    if (dp.f32 != nullptr && o.wgrad == Wgrad::FEWPOS_MFMA) return wgrad_fewpos();
    int rc = d.b >= 0 ? bias() : S3_OK;
    if (!rc) rc = wgrad_kernel();
    if (!rc) rc = s3_flush_pending_bias(ctx);     // (nothing took the bias gradient's launch along)
    return rc;
  }

  int wgrad_kernel() {
    const float* x = tptr(pl, d.in0);
    float* dw = gparam(pl, d.w);
    float* part = pl->wg_partial;
    const size_t part_bytes = pl->wg_partial_bytes;
    const int acc = bw.accumulate_wgrad;
    // (bf16-only dPre out of the consumer's fold, or a bf16 copy next to the fp32 one)
    const bool dy16 = dp.only16 || (dp.bf16 && wgrad_takes_bf16(o, Dy16::DISPATCH));
    const float* dy = dy16 ? (const float*)dp.bf16 : dp.f32;
    switch (o.wgrad) {
      case Wgrad::FEWPOS_MFMA: case Wgrad::FEWPOS:
        return launch_conv_fewpos_wgrad(ctx, g, x, dp.f32, dw, part, part_bytes, acc);
      case Wgrad::TAIL:
        return launch_conv_wgrad_tail(ctx, g, x, dp.f32, dw, part, part_bytes, acc, o.io.in_bf16);
      case Wgrad::C2:
        return launch_conv_wgrad_c2(ctx, g, x, dy, dw, part, part_bytes, acc, dy16 ? 1 : 0, x3);
      case Wgrad::BF16_2D:
        return launch_conv_wgrad_bf16_2d(ctx, g, x, dy, dw, part, part_bytes, acc, o.io.in_bf16, dy16 ? 1 : 0);
      case Wgrad::BF16_GEN:
        return launch_conv_wgrad_bf16_gen(ctx, g, x, dp.f32, dw, part, part_bytes, acc, o.io.in_bf16, x3);
      case Wgrad::F32_GEN:
        return launch_conv_wgrad_gen(ctx, g, x, dp.f32, dw, part, part_bytes, acc);
      case Wgrad::BF16_TRUNK:
        return launch_conv_wgrad_bf16(ctx, g, x, dy, dw, part, part_bytes, acc, o.io.in_bf16, dy16 ? 1 : 0, x3 ? 1 : 0);
      case Wgrad::F32_TRUNK:
        return launch_conv_wgrad_mfma(ctx, g, x, dp.f32, dw, part, part_bytes, acc);
      case Wgrad::DIRECT:
        return launch_conv_generic_wgrad(ctx, g, x, dp.f32, dw, part, part_bytes, acc);
    }
    return S3_OK;
  }

  // fold of the padded-frame data gradient (pl->dxp) into `out`; when this
  // conv is the only consumer of an activated conv's output the fold applies
  // that activation's adjoint (the producer then skips its mask pass)
  int fold_frame(const GatherGeom& fg, float* out, int frame16) {
    const bool own = out == pl->t[rin].gptr;   // (not the staging buffer of a later contribution)
    const bool fuse = o.mask_prod >= 0 && !bw.gwritten[rin] && gather_bwd_mask_ok(fg) && !s3_opt_has(S3O_NO_MASK_FUSE);
    // the stored tensor is (so far) the whole gradient of d.in0: its channel
    // sums = the bias gradient of the conv that produced it ride along
    // (grad_deliver drops them if the tensor changes later)
    float* bs = nullptr;
    if (bw.need_wgrad && pl->bsum && own && gather_bwd_bsum_ok(fg) && gather_bwd_bsum_blocks(ctx, fg) <= 4096 &&
        !s3_opt_has(S3O_NO_BIAS_FUSE)) {
      bs = pl->bsum;
      bw.claim_bsum(rin, gather_bwd_bsum_blocks(ctx, fg));
    }
    FoldJob job;
    job.frame = pl->dxp; job.frame16 = frame16 != 0; job.din = out;
    if (!fuse) {
      // second contribution to a skip tensor: fold + the aliased first one in
      // a single store (no staging buffer, no axpy); the tensor is finished
      const bool add = bw.gwritten[rin] == 2 && own && gather_bwd_mask_ok(fg);
      // ... or a plain fold: no channel sums
      if (!add && bs) bw.drop_bsum(rin);
      const bool whole = add || (own && !bw.gwritten[rin] && gather_bwd_mask_ok(fg) && !s3_opt_has(S3O_NO_PLAIN_FOLD16));
      void* side = (whole && fold_side16_ok(pl, o, rin)) ? pl->dpre16 : nullptr;
      job.side16 = (unsigned short*)side;
      if (add) { job.mode = FoldJob::ADD; job.aux = bw.take_alias(rin); job.bsum = bs; }
      const int rc = launch_fold(ctx, fg, job);
      if (!rc && side) bw.claim_dpre16(rin, false);
      return rc;
    }
    const OpRec& po = pl->ops[o.mask_prod];
    // The folded tensor is dPre of the producer conv and nothing else
    // (single consumer, mask applied here).  When every reader of it
    // takes bf16 — halo-tile / persistent data gradient, transpose-read
    // weight gradient, bias gradient from the channel sums riding
    // along — it is stored as bf16 ONLY: the fold writes 75 instead of
    // 151 MB and the readers stage half the bytes; they would round to
    // bf16 (the same round-to-nearest-even) anyway.
    const bool to16 = own && back_to_back(pl, o.mask_prod, i) && dpre16_free_for_out_of(pl, po) &&
                      (po.wgrad == Wgrad::BF16_TRUNK ||
                       (po.wgrad == Wgrad::BF16_2D && po.cg.s[0] == 1 && !s3_opt_has(S3O_NO_TRAIN2D_BF16))) &&
                      po.io.in_bf16 && po.d.res < 0 && (po.cg.Cout & 3) == 0 &&
                      (!bw.need_wgrad || po.d.b < 0 || bs != nullptr) && pl->precision == S3_PREC_BF16;
    job.mode = FoldJob::MASKED;
    job.aux = tptr(pl, d.in0); job.aux_bf16 = pl->t[rin].dtype != 0;
    job.slope = po.cg.act == S3_ACT_LEAKY ? po.cg.alpha : 0.f;
    job.bsum = bs;
    if (to16) { job.din = (float*)pl->dpre16; job.out_bf16 = true; }
    const int rc = launch_fold(ctx, fg, job);
    if (rc) return rc;
    bw.premasked[rin] = 1;
    if (to16) bw.claim_dpre16(rin, true);
    return S3_OK;
  }

  // 64 -> C_out > 64: 64-channel slices of dPre through the 64 -> 64 halo-tile
  // kernel, accumulated in place over the padded frame, then the fold
  int dgrad_chunked(float* dst) {
    const int nk = (g.Cout + 63) / 64;
    int rc = repack_if_stale(o.dg_version, version, [&] {
      int prc = S3_OK;
      for (int k = 0; k < nk && !prc; ++k) {
        prc = launch_conv_dgrad_chunk_pack(ctx, g, wptr(pl, d.w), o.dg_w32, k);
        if (!prc) prc = launch_conv_mfma_pack(ctx, conv_dgrad_chunk_geom(g, k), pl->precision, o.dg_w32, o.dgc_wbf[k]);
      }
      return prc;
    });
    if (rc) return rc;
    float* acc_to = o.dgrad == Dgrad::CHUNKED_VALID ? dst : pl->dxp;   // valid padding: x's own grid
    // with the bf16 copy of dPre: the slices go through the persistent
    // kernel (stacked frames, the later slices add in its store)
    const bool p16 = dp.bf16 && chunked_dgrad_persist16(ctx, o);
    for (int k = 0; k < nk; ++k) {
      const ConvGeom cgk = conv_dgrad_chunk_geom(g, k);
      if (p16)
        rc = launch_conv_mfma_persist_dgrad(ctx, cgk, (const unsigned short*)dp.bf16 + 64 * k,
                                            (const char*)o.dgc_wbf[k] + (size_t)27 * 64 * 64 * 2, acc_to, k ? 1 : 0);
      else
        rc = launch_conv_mfma_fwd(ctx, cgk, pl->precision, dp.f32 + 64 * k, o.dgc_wbf[k],
                                  nullptr, k ? acc_to : nullptr, acc_to, ConvIO());
      if (rc) return rc;
    }
    if (o.dgrad == Dgrad::CHUNKED_VALID) return S3_OK;   // (x's own grid: no fold)
    const int lo[3] = {1, 1, 1};
    return fold_frame(frame_fold_geom(g, lo), dst, 0);
  }

  // dXpad = conv_zero(dPre, flip(W)^T) over the padded frame, then the adjoint
  // of the virtual padding folds the border back (MFMA_FRAME, MFMA_VALID, GEN, FEWCH)
  int dgrad_mfma(float* dst) {
    int rc = repack_if_stale(o.dg_version, version, [&] {
      const int prc = launch_conv_dgrad_pack(ctx, g, wptr(pl, d.w), o.dg_w32);
      if (prc) return prc;
      if (o.dgrad == Dgrad::FEWCH) return launch_gconv_pack(ctx, o.dg, o.dg_w32, o.dg_wbf, 0, x3);
      if (pl->precision != S3_PREC_F32) return launch_conv_mfma_pack(ctx, o.dg, pl->precision, o.dg_w32, o.dg_wbf);
      return prc;
    });
    if (rc) return rc;
    const void* wp = pl->precision != S3_PREC_F32 ? (const void*)o.dg_wbf : (const void*)o.dg_w32;
    float* frame = o.dgrad == Dgrad::MFMA_VALID ? dst : pl->dxp;   // (a valid conv's full correlation lands on x's own grid)
    int frame16 = 0;
    if (o.dgrad == Dgrad::FEWCH)
      rc = launch_gconv_fwd(ctx, o.dg, dp.f32, o.dg_wbf, nullptr, nullptr, pl->dxp, 0, 0, x3);
    else if (o.use16 && dp.bf16 && pl->precision == S3_PREC_BF16 && conv_mfma_persist_dgrad_supported(ctx, o.dg)) {
      // the persistent trunk kernel over the stacked frames
      const size_t tile_img = (size_t)((o.dg.Cout + 63) / 64) * 27 * 64 * 64 * 2;
      frame16 = o.dgrad_frame16;
      rc = launch_conv_mfma_persist_dgrad(ctx, o.dg, dp.bf16, (const char*)o.dg_wbf + tile_img, frame, 0, frame16);
    } else {
      ConvIO dio;
      dio.in_bf16 = (o.use16 && dp.bf16) ? 1 : 0;
      // 2-D 64 -> 64 k convs: the frame form of the weights-stationary
      // kernel, bf16 dPre in, bf16 frame out (folded from bf16)
      if (dio.in_bf16 && o.dgrad == Dgrad::GEN && o.dgrad_frame16 && pl->precision == S3_PREC_BF16) {
        ConvIO wio = dio;
        wio.out_bf16 = 1;
        if (conv2d_ws_supported(o.dg, pl->precision, wio, false)) { dio = wio; frame16 = 1; }
      }
      rc = launch_conv_mfma_fwd(ctx, o.dg, pl->precision, dio.in_bf16 ? dp.bf16 : (const void*)dp.f32, wp, nullptr,
                                nullptr, frame, dio);
    }
    if (rc || o.dgrad == Dgrad::MFMA_VALID) return rc;   // (x's own grid: no fold)
    const int lo[3] = {g.k[0] == 3, g.k[1] == 3, g.k[2] == 3};   // (k = 1 axes of a 2-D conv carry no frame)
    return fold_frame(frame_fold_geom(g, lo), dst, frame16);
  }

  // stride-2 valid conv (S2, S2_X3).  Single consumer of an activated conv
  // output: its LeakyReLU / ReLU adjoint is applied in the store (the producer
  // then skips its mask pass)
  int dgrad_s2(float* dst) {
    const bool s2x3 = o.dgrad == Dgrad::S2_X3;
    int rc = repack_if_stale(o.dc2_version, version, [&] {
      return s2x3 ? launch_conv_dgrad_s2_x3_pack(ctx, g, wptr(pl, d.w), o.dc2_w)
                  : launch_conv_dgrad_s2_pack(ctx, g, wptr(pl, d.w), o.dc2_w);
    });
    if (rc) return rc;
    const bool fuse = o.mask_prod >= 0 && !bw.gwritten[rin] && !s3_opt_has(S3O_NO_MASK_FUSE) &&
                      (!s2x3 || pl->t[rin].dtype == 0);
    const OpRec& po = pl->ops[fuse ? o.mask_prod : i];
    const float slope = po.cg.act == S3_ACT_LEAKY ? po.cg.alpha : 0.f;
    // BF16: dx is dPre of the few-channel conv below (mask fused, single
    // consumer).  Its weight gradient (conv_wgrad_c2_kernel), its data
    // gradient (conv_dgrad_c2_kernel, generator step only) and its bias
    // gradient (channel sums riding along here) all take bf16: store it
    // as bf16 ONLY — 0.89 instead of 1.78 GB written here and read there,
    // and no separate bias pass over it.
    const int nblk = conv_dgrad_s2_blocks(g);
    const bool sums = bw.need_wgrad && po.d.b >= 0;
    const bool to16 = fuse && back_to_back(pl, o.mask_prod, i) && dst == pl->t[rin].gptr &&
                      pl->precision == S3_PREC_BF16 && !s2x3 && po.wgrad == Wgrad::C2 &&
                      po.cg.Cin == 2 && po.cg.Cout == 32 && po.d.res < 0 &&
                      (dgrad_is_c2(po.dgrad) || !wants_grad(pl, po.d.in0)) && conv_dgrad_s2_out16_ok(g) &&
                      dpre16_free_for(pl, rin) &&
                      (!sums || (pl->bsum && nblk <= 4096 && !s3_opt_has(S3O_NO_BIAS_FUSE))) &&
                      !s3_opt_has(S3O_NO_DPRE16);
    if (s2x3)
      rc = launch_conv_dgrad_s2_x3(ctx, g, dp.f32, o.dc2_w, dst, fuse ? (const float*)tptr(pl, d.in0) : nullptr, slope);
    else
      rc = launch_conv_dgrad_s2(ctx, g, dp.f32, o.dc2_w, to16 ? (float*)pl->dpre16 : dst,
                                fuse ? tptr(pl, d.in0) : nullptr, slope, o.io.in_bf16, to16 ? 1 : 0,
                                (to16 && sums) ? pl->bsum : nullptr,
                                (to16 && fuse && o.io.in_bf16) ? po.sign_bytes : nullptr);
    if (rc) return rc;
    if (fuse) bw.premasked[rin] = 1;
    if (to16) bw.claim_dpre16(rin, true);
    if (to16 && sums) bw.claim_bsum(rin, nblk);
    return S3_OK;
  }

  // few-channel hi-res conv on the LDS halo (C2, C2_X3)
  int dgrad_c2(float* dst) {
    const float* w = wptr(pl, d.w);
    const bool c2x3 = o.dgrad == Dgrad::C2_X3;
    int rc = repack_if_stale(o.dc2_version, version, [&] {
      return c2x3 ? launch_conv_dgrad_c2_x3_pack(ctx, g, w, o.dc2_w) : launch_conv_dgrad_c2_pack(ctx, g, w, o.dc2_w);
    });
    if (rc) return rc;
    if (c2x3) return launch_conv_dgrad_c2_x3(ctx, g, dp.f32, o.dc2_w, dst);
    return launch_conv_dgrad_c2(ctx, g, dp.only16 ? (const float*)dp.bf16 : dp.f32, o.dc2_w, dst, dp.only16 ? 1 : 0);
  }

  // gather-MFMA adjoint; a reflect frame is folded by the plain adjoint of
  // the pad (no mask fusion, no bf16 copy)
  int dgrad_gconv(float* dst) {
    int rc = repack_if_stale(o.gct_version, version, [&] { return launch_gconv_pack(ctx, g, wptr(pl, d.w), o.gc_wt, 1, x3); });
    if (rc) return rc;
    if (g.pad_mode == S3_PAD_REFLECT) {
      // dXpad over the reflect-padded frame, then fold the border back
      rc = launch_gconv_dgrad(ctx, g, dp.f32, o.gc_wt, pl->dxp, 0, 1, 0, x3);
      if (rc) return rc;
      return fold_plain(ctx, frame_fold_geom(g, g.lo), pl->dxp, dst);
    }
    const bool dy16 = o.use16 && dp.bf16 != nullptr;
    return launch_gconv_dgrad(ctx, g, dy16 ? (const float*)dp.bf16 : dp.f32, o.gc_wt, dst, 0, 0, dy16 ? 1 : 0, x3);
  }

  int dgrad_fewpos_mfma(float* dst) {
    // (reads the [tap][ci][co] filter along co: no transposed copy)
    const float* wf = wptr(pl, d.w);
    const bool reflect = g.pad_mode == S3_PAD_REFLECT;
    float* to = reflect ? pl->dxp : dst;
    int rc;
    if (fp_both)
      rc = launch_conv_fewpos_bwd_mfma(ctx, g, fp_gd, tptr(pl, d.in0), dp.f32, wf, to, gparam(pl, d.w), gparam(pl, d.b),
                                       bw.accumulate_wgrad, dp.mask_y, dp.slope);
    else
      rc = launch_conv_fewpos_mfma(ctx, fp_gd, 1, dp.f32, wf, nullptr, nullptr, to, dp.mask_y, dp.slope);
    if (rc || !reflect) return rc;
    // (with the producer's activation adjoint, or the first contribution
    // of a skip tensor, in the same store: no mask pass, no axpy)
    return fold_frame(frame_fold_geom(g, g.lo), dst, 0);
  }

  // slab kernel of the fewpos family; a reflect frame is folded by the plain
  // adjoint of the pad (no mask fusion, no bf16 copy)
  int dgrad_fewpos(float* dst) {
    int rc = repack_if_stale(o.fp_version, version, [&] { return launch_conv_fewpos_transpose(ctx, g, wptr(pl, d.w), o.fp_wt); });
    if (rc) return rc;
    if (g.pad_mode != S3_PAD_REFLECT)
      return launch_conv_fewpos_dgrad(ctx, g, dp.f32, o.fp_wt, dst, pl->fp_partial, pl->fp_partial_bytes);
    // dXpad over the padded frame (zero boundary), then fold the border back
    rc = launch_conv_fewpos_dgrad(ctx, conv_fewpos_frame_geom(g), dp.f32, o.fp_wt, pl->dxp, pl->fp_partial, pl->fp_partial_bytes);
    if (rc) return rc;
    return fold_plain(ctx, frame_fold_geom(g, g.lo), pl->dxp, dst);
  }

  int dgrad(float* dst) {
    switch (o.dgrad) {
      case Dgrad::CHUNKED_FRAME: case Dgrad::CHUNKED_VALID: return dgrad_chunked(dst);
      case Dgrad::MFMA_FRAME: case Dgrad::MFMA_VALID: case Dgrad::GEN: case Dgrad::FEWCH: return dgrad_mfma(dst);
      case Dgrad::S2: case Dgrad::S2_X3: return dgrad_s2(dst);
      case Dgrad::C2: case Dgrad::C2_X3: return dgrad_c2(dst);
      case Dgrad::GCONV: return dgrad_gconv(dst);
      case Dgrad::FEWPOS_MFMA: return dgrad_fewpos_mfma(dst);
      case Dgrad::FEWPOS: return dgrad_fewpos(dst);
      case Dgrad::DIRECT: return launch_conv_generic_dgrad(ctx, g, dp.f32, wptr(pl, d.w), dst);
    }
    return S3_OK;
  }
};

// backward of op i; dy = the finished gradient of its output
static int backward_op(s3_plan* pl, int i, const float* dy) {
  s3_ctx* ctx = pl->ctx;
  const OpRec& o = pl->ops[i];
  const s3_op_desc& d = o.d;
  const TensorRec& ot = pl->t[d.out];
  const BwdState& bw = pl->bw;
  if (d.kind == S3_OP_CONV) return ConvBwd(pl, i).run(dy);
  if (d.kind == S3_OP_ADD) {
    int rc = wants_grad(pl, d.in0) ? grad_deliver(pl, d.in0, dy) : S3_OK;
    if (!rc && !d.bcast_c && wants_grad(pl, d.in1)) rc = grad_deliver(pl, d.in1, dy);
    return rc;
  }
  const bool want_dx = wants_grad(pl, d.in0);
  float* dst = want_dx ? grad_dest(pl, d.in0) : nullptr;
  int rc = S3_OK;
  switch (d.kind) {
    case S3_OP_DENSE: {
      const TensorRec& it = pl->t[d.in0];
      const int rows = (int)(it.numel / it.dims[4]);
      const int cin = (int)it.dims[4], cout = (int)ot.dims[4];
      const float* dpre = dy;
      if (d.act != S3_ACT_NONE) {
        rc = launch_act_bwd(ctx, tptr(pl, d.out), dy, pl->dpre, ot.numel, d.act, d.alpha);
        if (rc) return rc;
        dpre = pl->dpre;
      }
      if (bw.need_wgrad && d.b >= 0) rc = launch_bias_grad(ctx, dpre, rows, cout, gparam(pl, d.b), bw.accumulate_wgrad);
      if (!rc && bw.need_wgrad)
        rc = launch_dense_wgrad(ctx, tptr(pl, d.in0), dpre, gparam(pl, d.w), rows, cin, cout, bw.accumulate_wgrad);
      if (!rc && want_dx) rc = launch_dense_dgrad(ctx, dpre, wptr(pl, d.w), dst, rows, cin, cout);
    } break;
    case S3_OP_REPEAT_T: case S3_OP_D2S: case S3_OP_PAD: case S3_OP_CROP:
    case S3_OP_ROLL_T: case S3_OP_DILATE:
      if (want_dx) rc = fold_plain(ctx, o.gg, dy, dst);
      break;
    case S3_OP_CONCAT:
      if (want_dx) {
        const TensorRec& a = pl->t[d.in0];
        rc = s3_copy_channels(ctx, dy, (int)ot.dims[4], 0, dst, (int)a.dims[4], 0, (int)a.dims[4], a.numel / a.dims[4], 0);
      }
      break;
    case S3_OP_ACT:
      if (want_dx) rc = launch_act_bwd(ctx, tptr(pl, d.out), dy, dst, ot.numel, d.act, d.alpha);
      break;
    default: return S3_OK;
  }
  if (rc || !want_dx) return rc;
  return grad_deliver(pl, d.in0, dst);
}

// The bucketed reduction hands over "everything at or above this op's lowest
// offset" as the walk passes an op: true only if the parameter offsets grow
// with the op order and no parameter is shared between ops.  Checked once per
// armed pass; a store laid out any other way gets ONE reduction of the whole
// buffer after the last op instead.
static void reduce_check_layout(s3_plan* pl) {
  s3_params* P = pl->params;
  int64_t prev_end = 0;
  for (const OpRec& o : pl->ops) {
    int64_t lo = INT64_MAX, hi = -1;
    for (int id : {o.d.w, o.d.b}) {
      if (id < 0) continue;
      lo = std::min(lo, P->p[id].offset);
      hi = std::max(hi, P->p[id].offset + P->p[id].size);
    }
    if (hi < 0) continue;
    if (lo < prev_end) { P->bucket_elems = P->total + 1; return; }
    prev_end = hi;
  }
}

// Bucketed all-reduce under an armed backward pass.  The walk has passed op
// `d`: the gradients of every parameter at or above its lowest offset are
// final in stream order, and go out once they fill a bucket.  d == nullptr:
// the walk is over, the rest goes out and the store is disarmed.
static int reduce_passed(s3_plan* pl, const s3_op_desc* d) {
  s3_params* P = pl->params;
  if (!pl->bw.need_wgrad || !P->armed || (d && d->w < 0 && d->b < 0)) return S3_OK;
  int64_t lowest = d ? P->reduce_end : 0;
  if (d && d->w >= 0) lowest = std::min(lowest, P->p[d->w].offset);
  if (d && d->b >= 0) lowest = std::min(lowest, P->p[d->b].offset);
  const int64_t n = P->reduce_end - lowest;
  if (d ? n >= P->bucket_elems : n > 0) {
    const int rc = s3_comm_reduce_range(pl->ctx, P->buf[S3_BUF_G] + lowest, n);
    if (rc) return rc;
    P->reduce_end = lowest;
    P->buckets_issued++;
  }
  if (!d) {
    // consumed: a later backward pass on this store issues no collective
    // unless it is armed again
    P->armed = false;
    P->reduced = true;
  }
  return S3_OK;
}

static int plan_backward_impl(s3_plan* pl, const void* d_output, void* d_input, int need_wgrad,
                              int accumulate_wgrad) {
  s3_ctx* ctx = pl->ctx;
  S3OptScope opt_scope(&pl->opt);
  BwdState& bw = pl->bw;
  if (!pl->training) S3_FAIL(ctx, S3_ESTATE, "backward on an inference plan");
  if (!pl->forward_done) S3_FAIL(ctx, S3_ESTATE, "backward before forward");
  // (gradients about to be rewritten: a reduction nobody joined is moot)
  if (need_wgrad) pl->params->reduced = false;
  if (need_wgrad && pl->params->armed) reduce_check_layout(pl);
  const int x_id = pl->inputs.empty() ? -1 : root_of(pl, pl->inputs[0]);
  bw.reset(pl->t.size());
  bw.need_wgrad = need_wgrad;
  bw.accumulate_wgrad = accumulate_wgrad;
  bw.dx_root = d_input ? x_id : -1;
  // the caller's buffer is read-only for the duration of the call: alias it
  bw.alias(root_of(pl, pl->output), (const float*)d_output);
  int rc = pack_stale(pl, true);
  if (rc) return rc;
  const int n_ops = (int)pl->ops.size();
  for (int i = n_ops - 1; i >= 0; --i) {
    const s3_op_desc& d = pl->ops[i].d;
    if (d.kind == S3_OP_VIEW) continue;
    const int ro = root_of(pl, d.out);
    if (!bw.gwritten[ro]) continue;  // nothing flows through this op
    rc = backward_op(pl, i, grad_of(pl, ro));
    if (rc) {
      // (which launch: a failure inside a stream capture is otherwise anonymous)
      char where[96];
      snprintf(where, sizeof(where), " [backward op %d of %d, kind %d%s]", i, n_ops, d.kind,
               ctx->capturing ? ", capturing" : "");
      ctx->err += where;
      return rc;
    }
    rc = reduce_passed(pl, &d);
    if (rc) return rc;
  }
  rc = reduce_passed(pl, nullptr);
  if (rc) return rc;
  if (d_input) {
    if (x_id < 0 || !bw.gwritten[x_id]) S3_FAIL(ctx, S3_ESTATE, "backward: no gradient reached the input");
    S3_HIP(ctx, hipMemcpyAsync(d_input, grad_of(pl, x_id), (size_t)pl->t[x_id].numel * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return S3_OK;
}

extern "C" int s3_plan_backward(s3_plan* pl, const void* d_output, void* d_input,
                                int need_wgrad, int accumulate_wgrad) {
  if (!pl || !d_output) return S3_EINVAL;
  int rc = plan_backward_impl(pl, d_output, d_input, need_wgrad, accumulate_wgrad);
  const int jrc = wg_join(pl->ctx);      // (also on a failed pass: a capture must not end forked)
  if (rc == S3_OK) rc = jrc;
  if (rc != S3_OK && pl->params && (pl->params->armed || pl->params->reduced)) {
    pl->params->reduced = false;
    // an armed store must not outlive the backward pass it was armed for: the
    // next one on this store (a validation step, a non-sharded step) would
    // enqueue collectives the other ranks never issue
    pl->params->armed = false;
    pl->params->reduce_end = 0;
    pl->params->buckets_issued = 0;
  }
  return rc;
}
