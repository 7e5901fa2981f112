// Construction of the shape-specialised plan executor of libsup3r_hip.so (host
// side, C++).  The executor replaces the eager keras
// layer loops of sup3r (abstract.py:1131-1173, base.py:283-313) and
// tf.GradientTape (abstract.py:1230-1237): a fused op list runs on one HIP
// stream out of a statically planned activation arena; the backward pass walks
// the same list in reverse.  Here the op list is validated, every conv gets its
// kernels, and the passes below fuse ops, set dtypes and allocate; the passes
// themselves run in plan_forward.cpp and plan_backward.cpp, the context and the
// parameter store live in context.cpp and params.cpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "plan_internal.h"

int plan_alloc(s3_plan* pl, void** out, size_t bytes) {
  s3_ctx* ctx = pl->ctx;
  if (bytes == 0) bytes = 16;
  S3_HIP(ctx, hipMalloc(out, bytes));
  // every plan buffer starts zeroed (hipMalloc hands back stale bytes of freed
  // buffers: padding rows / halo borders that no kernel writes must not depend
  // on what ran before).  SUP3R_AMD_POISON_ALLOC=1 fills all-ones bytes instead
  // (NaN as fp32 and as bf16): a debugging aid that makes any read of a plan
  // buffer before its first write show up in the results.
  S3_HIP(ctx, hipMemsetAsync(*out, s3_opt_has(S3O_POISON_ALLOC) ? 0xFF : 0, bytes, ctx->stream));
  pl->owned.push_back(*out);
  pl->total_bytes += bytes;
  return S3_OK;
}

// --------------------------------------------------------------------- plan
static int64_t numel5(const int64_t* d) { return d[0] * d[1] * d[2] * d[3] * d[4]; }

static void fill_conv_geom(const s3_plan* pl, const s3_op_desc& d, ConvGeom& g) {
  const TensorRec& in = pl->t[d.in0];
  const TensorRec& out = pl->t[d.out];
  g.N = (int)in.dims[0];
  for (int i = 0; i < 3; ++i) {
    g.D[i] = (int)in.dims[1 + i];
    g.k[i] = d.k[i]; g.s[i] = d.stride[i]; g.lo[i] = d.lo[i];
  }
  const int b = d.d2s < 1 ? 1 : d.d2s;
  g.O[0] = (int)out.dims[1] / b; g.O[1] = (int)out.dims[2] / b; g.O[2] = (int)out.dims[3];
  g.Cin = (int)in.dims[4];
  g.Cout = (int)out.dims[4] * b * b;
  g.pad_mode = d.pad_mode; g.act = d.act; g.alpha = d.alpha; g.d2s = b;
}

static void fill_gather_geom(const s3_plan* pl, const s3_op_desc& d, GatherGeom& g) {
  const TensorRec& in = pl->t[d.in0];
  const TensorRec& out = pl->t[d.out];
  g.kind = d.kind; g.N = (int)in.dims[0];
  for (int i = 0; i < 3; ++i) {
    g.Di[i] = (int)in.dims[1 + i]; g.Do[i] = (int)out.dims[1 + i]; g.lo[i] = d.lo[i];
  }
  g.Ci = (int)in.dims[4]; g.Co = (int)out.dims[4];
  g.pad_mode = d.pad_mode; g.rep = d.rep; g.d2s = d.d2s; g.c_off = 0;
}

extern "C" int s3_plan_create(s3_ctx* ctx, s3_params* params,
                              const s3_tensor_desc* tensors, int n_tensors,
                              const s3_op_desc* ops, int n_ops,
                              const int32_t* inputs, int n_inputs,
                              int32_t output, int precision, int training,
                              s3_plan** out) {
  return s3_plan_create_opt(ctx, params, tensors, n_tensors, ops, n_ops, inputs, n_inputs, output,
                            precision, training, nullptr, out);
}

// ---- kernel selection of one conv (before the dtypes are known)
static void select_conv(s3_ctx* ctx, OpRec& o, int precision, int training, bool plan_tiny) {
  const ConvGeom& g = o.cg;
  const s3_op_desc& d = o.d;
  bool mfma = conv_mfma_supported(g, precision);
  // Round 6: a trunk-geometry conv (64 -> 64 k, 3 x 3 x 3) over <= 1 024 positions in
  // a TRAINING plan — the lo-res stack of the reference's test shapes, BASELINE
  // configs 4 / 5: lr (N, 4, 4, 4, 2) — leaves the halo-tile family: two or four
  // of its tiles keep two or four CUs busy (17 us forward, 17 us data gradient,
  // 40 + 5 us for the weight gradient whose every workgroup holds the whole 27 x
  // 64 x 64 tile), where the one-launch fewpos kernels split the work over (tap,
  // channel block) and take ~8 us for forward and ~8 us for both gradients.
  // (Training plans only: an inference plan's kernels do not depend on the batch.)
  const int64_t P_out = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2];
  // (the 3-D trunk geometry only: the logical-axes kernel of 2-D nets / few time
  // steps keeps its layers — its tests pin the selection at such sizes)
  const bool small_trunk = training && mfma && !conv_mfma_is_gen(g, precision) && !s3_opt_has(S3O_NO_FEWPOS) &&
                           !s3_opt_has(S3O_NO_FEWPOS_TRUNK) && precision != S3_PREC_BF16X3 &&
                           P_out <= 1024 && conv_fewpos_supported(g) && conv_fewpos_mfma_ok(g);
  if (small_trunk) mfma = false;
  bool fewpos = !mfma && !s3_opt_has(S3O_NO_FEWPOS) && conv_fewpos_supported(g);
  // bf16 plans: the weight-streaming fp32 path only for really few
  // positions; mid-size layers go to the gather-MFMA kernels
  // (... unless the one-launch fp32-MFMA kernels take the layer while the
  // chip is mostly idle: no per-step filter pack, no split-K epilogue)
  // (BF16X3 plans keep their split-bf16 gather-MFMA kernels)
  // (training plans only: an inference plan's kernels must not change
  // with the batch size — chunk-by-chunk and batched runs agree bit for bit)
  const bool fp_small = training && plan_tiny && !mfma && !s3_opt_has(S3O_NO_FEWPOS) && precision != S3_PREC_BF16X3 &&
                        conv_fewpos_mfma_small_ok(ctx, g);
  if (fewpos && P_out >= 256 && conv_gconv_supported(g, precision) && conv_gconv_dgrad_supported(g, precision) &&
      conv_wgrad_gen_supported(g) && !((fp_small || small_trunk) && conv_fewpos_mfma_ok(g)))
    fewpos = false;
  // the few-channel head / tail convs and small filters on those kernels too
  if (mfma) o.fam = Fam::MFMA;
  else if (fewpos) o.fam = conv_fewpos_mfma_ok(g) ? Fam::FEWPOS_MFMA : Fam::FEWPOS;
  else if (fp_small) o.fam = Fam::FEWPOS_MFMA;
  else if (conv_gconv_supported(g, precision))
    o.fam = d.res < 0 && conv_halo32_supported(ctx, g, precision)   ? Fam::HALO32
            : d.res < 0 && conv_halo_s2_supported(ctx, g, precision) ? Fam::HALO_S2
                                                                     : Fam::GCONV;
  else if (d.res < 0 && conv_tail_x3_supported(g, precision)) o.fam = Fam::TAIL_X3;
  else o.fam = Fam::DIRECT;

  if (!training) return;
  const bool fp = o.fewpos();
  const bool fp_mfma = o.fam == Fam::FEWPOS_MFMA;
  const bool bwd = !s3_opt_has(S3O_NO_MFMA_BWD);
  if (fp) o.wgrad = fp_mfma ? Wgrad::FEWPOS_MFMA : Wgrad::FEWPOS;
  else if (!bwd) o.wgrad = Wgrad::DIRECT;
  else if (conv_wgrad_tail_supported(g, precision)) o.wgrad = Wgrad::TAIL;
  else if (conv_wgrad_c2_supported(g, precision)) o.wgrad = Wgrad::C2;
  else if (!small_trunk && conv_wgrad_mfma_supported(g))
    o.wgrad = conv_wgrad_bf16_supported(g, precision) ? Wgrad::BF16_TRUNK : Wgrad::F32_TRUNK;
  else if (conv_wgrad_bf16_gen_supported(g, precision)) o.wgrad = Wgrad::BF16_GEN;
  else if (conv_wgrad_bf16_2d_supported(g, precision)) o.wgrad = Wgrad::BF16_2D;
  else if (conv_wgrad_gen_supported(g)) o.wgrad = Wgrad::F32_GEN;
  // what is left would take the generic kernel (one thread per filter
  // element walking every position: 204 us for the 1 500 positions of
  // the C1 discriminator's first layers); with few positions the slab
  // kernel of the fewpos family does any C_in / C_out
  // (its input is fp32: the dtype pass demotes the input of every conv whose
  // weight gradient does not stage bf16)
  else if (conv_fewpos_wgrad_ok(g) && !s3_opt_has(S3O_NO_FEWPOS))
    o.wgrad = conv_fewpos_wgrad_mfma_ok(g) ? Wgrad::FEWPOS_MFMA : Wgrad::FEWPOS;
  else o.wgrad = Wgrad::DIRECT;

  const bool bf = precision == S3_PREC_BF16, x3 = precision == S3_PREC_BF16X3;
  const Dgrad dg_fp = fp ? (fp_mfma ? Dgrad::FEWPOS_MFMA : Dgrad::FEWPOS) : Dgrad::DIRECT;
  bool fewch = false;
  if ((bf || x3) && !s3_opt_has(S3O_NO_DGRAD_FEWCH) && (g.Cout == 2 || g.Cout == 4) && g.Cin % 4 == 0 &&
      g.d2s == 1 && (int64_t)g.N * g.D[0] * g.D[1] * g.D[2] >= 4096) {
    // hi-res tail conv (8 -> 2): its data gradient is a conv with 2 input
    // channels — the taps-in-K few-channel kernel over the padded frame
    fewch = true;
    for (int q = 0; q < 3; ++q)
      fewch = fewch && g.k[q] == 3 && g.s[q] == 1 && g.lo[q] == 1 && g.O[q] == g.D[q];
    fewch = fewch && conv_gconv_supported(conv_dgrad_geom(g), precision);
  }
  if (!bwd) o.dgrad = dg_fp;
  else if (!small_trunk && conv_dgrad_mfma_supported(g, precision)) o.dgrad = Dgrad::MFMA_FRAME;
  else if (fp) o.dgrad = dg_fp;
  // (BF16X3: the split-bf16 tile kernel takes the same geometry — the
  // discriminator's valid 32 -> 64 conv left the gather-MFMA adjoint,
  // 2.25 -> 0.5 ms at C2 batch 8)
  else if ((bf || (x3 && !s3_opt_has(S3O_NO_DGRAD_X3))) && conv_dgrad_mfma_valid_supported(g, precision))
    o.dgrad = Dgrad::MFMA_VALID;
  else if (fewch) o.dgrad = Dgrad::FEWCH;
  else if (conv_dgrad_chunked_supported(g, precision))
    o.dgrad = g.lo[0] == 0 ? Dgrad::CHUNKED_VALID : Dgrad::CHUNKED_FRAME;
  // (BF16X3 plans: the split-bf16 forms of the next two kernels, round 4)
  else if (conv_dgrad_c2_supported(g, precision) || conv_dgrad_c2_x3_supported(g, precision))
    o.dgrad = x3 ? Dgrad::C2_X3 : Dgrad::C2;
  else if (conv_dgrad_s2_supported(ctx, g, precision) || conv_dgrad_s2_x3_supported(ctx, g, precision))
    o.dgrad = x3 ? Dgrad::S2_X3 : Dgrad::S2;
  // what is left behind a REFLECT pad (2-D nets, few time steps, odd channel
  // counts): the padded-frame correlation on the logical-axes tile kernel
  else if (conv_dgrad_gen_supported(g, precision)) o.dgrad = Dgrad::GEN;
  else if (conv_gconv_dgrad_supported(g, precision)) o.dgrad = Dgrad::GCONV;
  else o.dgrad = Dgrad::DIRECT;
  if (dgrad_is_mfma(o.dgrad))
    o.dg = o.dgrad == Dgrad::GEN          ? conv_dgrad_gen_geom(g)
           : dgrad_is_chunked(o.dgrad)   ? conv_dgrad_chunk_geom(g, 0)
           : o.dgrad == Dgrad::MFMA_VALID ? conv_dgrad_valid_geom(g)
                                          : conv_dgrad_geom(g);
}

// the forward kernel, once the dtypes (and the fused operands) of the conv are known
static Fwd resolve_fwd(const s3_ctx* ctx, const OpRec& o, int precision) {
  const ConvIO& io = o.io;
  const bool res = o.d.res >= 0;
  const bool f32_io = !io.in_bf16 && !io.out_bf16;
  const bool gconv_io = (!io.in_bf16 || o.cg.Cin % 8 == 0) && !io.res_bf16 && (!io.out_bf16 || o.cg.Cout % 4 == 0);
  const Fwd generic = fwd_of(conv_generic_fwd_variant(o.cg, io, res));
  switch (o.fam) {
    case Fam::MFMA: return fwd_of(conv_mfma_fwd_variant(ctx, o.cg, precision, io, res));
    case Fam::HALO32: return Fwd::HALO32;
    case Fam::HALO_S2: return io.in_bf16 ? Fwd::HALO_S2 : gconv_io ? Fwd::GCONV : generic;
    case Fam::GCONV: return gconv_io ? Fwd::GCONV : generic;
    case Fam::TAIL_X3: return f32_io ? Fwd::TAIL_X3 : generic;
    case Fam::FEWPOS_MFMA: return f32_io ? Fwd::FEWPOS_MFMA : generic;
    case Fam::FEWPOS: return f32_io ? Fwd::FEWPOS : generic;
    case Fam::DIRECT: break;
  }
  return generic;
}

// the shared workspaces a conv's kernels need (sized by the plan's largest)
struct WorkspaceSizes {
  size_t dpre = 0, partial = 0, dxp = 0, fp = 0;
  size_t dpre16 = 0;   // bf16 copy of dPre (plan_dpre16)
};

static void conv_workspace(const s3_ctx* ctx, const OpRec& o, int training, WorkspaceSizes& ws) {
  const ConvGeom& g = o.cg;
  auto grow = [](size_t& m, size_t b) { m = std::max(m, b); };
  size_t frame = (size_t)g.N * g.Cin * sizeof(float);   // frame of a reflect data gradient
  for (int q = 0; q < 3; ++q) frame *= (size_t)(g.D[q] + 2 * g.lo[q]);
  if (o.fewpos()) {
    grow(ws.fp, conv_fewpos_partial_bytes(g));
    if (training && g.pad_mode == S3_PAD_REFLECT) grow(ws.dxp, frame);
  }
  grow(ws.dpre, (size_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout * sizeof(float));
  grow(ws.partial, conv_generic_wgrad_partial_bytes(g));
  if (!training) return;
  switch (o.wgrad) {
    case Wgrad::FEWPOS_MFMA: case Wgrad::FEWPOS: grow(ws.partial, conv_fewpos_wgrad_partial_bytes(g)); break;
    case Wgrad::TAIL: grow(ws.partial, conv_wgrad_tail_partial_bytes(ctx, g)); break;
    case Wgrad::C2: grow(ws.partial, conv_wgrad_c2_partial_bytes(ctx, g)); break;
    case Wgrad::BF16_TRUNK: grow(ws.partial, conv_wgrad_bf16_partial_bytes(ctx, g)); break;
    case Wgrad::F32_TRUNK: grow(ws.partial, conv_wgrad_mfma_partial_bytes(ctx, g)); break;
    case Wgrad::BF16_GEN: grow(ws.partial, conv_wgrad_bf16_gen_partial_bytes(ctx, g)); break;
    case Wgrad::BF16_2D: grow(ws.partial, conv_wgrad_bf16_2d_partial_bytes(ctx, g)); break;
    case Wgrad::F32_GEN: grow(ws.partial, conv_wgrad_gen_partial_bytes(ctx, g)); break;
    case Wgrad::DIRECT: break;
  }
  if (o.dgrad == Dgrad::GCONV && g.pad_mode == S3_PAD_REFLECT) grow(ws.dxp, frame);
  if (dgrad_is_mfma(o.dgrad))
    grow(ws.dxp, (size_t)o.dg.N * o.dg.O[0] * o.dg.O[1] * o.dg.O[2] * o.dg.Cout * sizeof(float));
}

// validation of the op list and the kernel choice of every conv (S3_EINVAL: the
// message is in ctx->err)
static int plan_select(s3_plan* pl, const s3_op_desc* ops, WorkspaceSizes& ws) {
  s3_ctx* ctx = pl->ctx;
  const int precision = pl->precision, training = pl->training;
  const int n_ops = (int)pl->ops.size(), n_tensors = (int)pl->t.size();
  const s3_params* params = pl->params;
  auto bad = [&](const char* m) { ctx->err = m; return S3_EINVAL; };
  // a launch-bound plan: no tensor has more than 4 096 positions (the C1 / toy
  // training shapes) — every step of it is a chain of ~5 us launches, and the
  // few-channel head / tail convs go to the one-launch fewpos kernels as well
  bool plan_tiny = true;
  for (int i = 0; i < n_tensors; ++i)
    if (pl->t[i].numel / std::max<int64_t>(1, pl->t[i].dims[4]) > 4096) plan_tiny = false;
  const int np = (int)params->p.size();
  for (int i = 0; i < n_ops; ++i) {
    OpRec& o = pl->ops[i];
    o.d = ops[i];
    const s3_op_desc& d = o.d;
    auto tid_ok = [&](int id, bool opt) { return (opt && id < 0) || (id >= 0 && id < n_tensors); };
    if (!tid_ok(d.in0, false) || !tid_ok(d.out, false) || !tid_ok(d.in1, true) || !tid_ok(d.res, true))
      return bad("plan: op references a bad tensor id");
    if (d.w >= np || d.b >= np) return bad("plan: op references a bad parameter id");
    switch (d.kind) {
      case S3_OP_CONV: {
        if (d.w < 0) return bad("plan: conv without weights");
        fill_conv_geom(pl, d, o.cg);
        const ConvGeom& g = o.cg;
        int64_t wsz = (int64_t)g.k[0] * g.k[1] * g.k[2] * g.Cin * g.Cout;
        if (params->p[d.w].size != wsz) return bad("plan: conv weight size mismatch");
        if (d.b >= 0 && params->p[d.b].size != g.Cout) return bad("plan: conv bias size mismatch");
        const TensorRec& ot = pl->t[d.out];
        if (ot.dims[0] != g.N || ot.dims[4] * g.d2s * g.d2s != g.Cout)
          return bad("plan: conv output shape mismatch");
        for (int q = 0; q < 3; ++q) {
          if (g.s[q] < 1 || g.k[q] < 1) return bad("plan: bad conv geometry");
          int mx = (g.O[q] - 1) * g.s[q] + g.k[q] - 1 - g.lo[q];
          if (g.pad_mode == S3_PAD_REFLECT &&
              (g.lo[q] > g.D[q] - 1 || mx > 2 * (g.D[q] - 1)))
            return bad("plan: reflect padding exceeds the tensor extent");
        }
        if (d.res >= 0 && pl->t[d.res].numel != ot.numel) return bad("plan: residual shape mismatch");
        select_conv(ctx, o, precision, training, plan_tiny);
        conv_workspace(ctx, o, training, ws);
      } break;
      case S3_OP_DENSE: {
        if (d.w < 0) return bad("plan: dense without weights");
        const TensorRec& it = pl->t[d.in0];
        const TensorRec& ot = pl->t[d.out];
        if (params->p[d.w].size != it.dims[4] * ot.dims[4]) return bad("plan: dense weight size mismatch");
        ws.dpre = std::max(ws.dpre, (size_t)ot.numel * sizeof(float));
      } break;
      case S3_OP_REPEAT_T: case S3_OP_D2S: case S3_OP_PAD: case S3_OP_CROP:
      case S3_OP_ROLL_T: case S3_OP_DILATE:
        fill_gather_geom(pl, d, o.gg);
        if (d.kind == S3_OP_DILATE)
          for (int q = 0; q < 3; ++q) o.gg.lo[q] = d.stride[q] < 1 ? 1 : d.stride[q];
        break;
      case S3_OP_CONCAT:
        if (d.in1 < 0) return bad("plan: concat without second input");
        break;
      case S3_OP_ADD:
        if (d.in1 < 0) return bad("plan: add without second input");
        break;
      case S3_OP_ACT: break;
      case S3_OP_VIEW:
        if (pl->t[d.in0].numel != pl->t[d.out].numel) return bad("plan: view changes element count");
        pl->t[d.out].alias_root = d.in0;
        break;
      default:
        return bad("plan: unknown op kind");
    }
  }
  return S3_OK;
}

// ---- inference plans: Sup3rConcat of a 64-channel tensor and ONE exogenous
// channel in front of a 3 x 3 Conv2D (sup3rcc/gen_wind_5x_1x_6f at hi-res: a
// 65-channel fp32 tensor written, read back by a two-pass fp32 conv: 28 of
// 126 ms at 96 x 750 x 750).  The conv is linear in its input channels: it
// runs as the 64 -> C_out conv over the bf16 tensor on the weights-stationary
// kernel, which adds the exogenous channel's nine taps per output from the
// fp32 field itself (ConvGeom::w_cin / exo); the concat never runs.  Checked
// again once the dtypes are known; if the kernel cannot take the conv after
// all the plan is built again without the split.
static thread_local int tl_no_ws_exo = 0;

static void plan_ws_exo(s3_plan* pl) {
  const int precision = pl->precision, training = pl->training, output = pl->output;
  const int n_ops = (int)pl->ops.size();
  if (training || precision != S3_PREC_BF16 || s3_opt_has(S3O_NO_WS_EXO) || s3_opt_has(S3O_FP32_ACT) || tl_no_ws_exo)
    return;
  for (int i = 0; i < n_ops; ++i) {
    OpRec& c = pl->ops[i];
    if (c.d.kind != S3_OP_CONCAT) continue;
    const TensorRec& xt = pl->t[c.d.in0];
    const TensorRec& et = pl->t[c.d.in1];
    if (xt.dims[4] != 64 || et.dims[4] != 1 || !pl->t[root_of(pl, c.d.in1)].is_input) continue;
    const int ct_ = root_of(pl, c.d.out);
    if (ct_ == root_of(pl, output)) continue;
    int user = -1, n_use = 0;
    for (int k = 0; k < n_ops; ++k) {
      const s3_op_desc& u = pl->ops[k].d;
      for (int id : {u.in0, u.in1, u.res})
        if (id >= 0 && root_of(pl, id) == ct_) { ++n_use; user = k; }
    }
    if (n_use != 1 || user <= i) continue;
    OpRec& v = pl->ops[user];
    if (v.d.kind != S3_OP_CONV || root_of(pl, v.d.in0) != ct_ || v.cg.Cin != 65) continue;
    ConvGeom gs = v.cg;
    gs.Cin = 64; gs.w_cin = 65;
    if (!conv2d_ws_geom_ok(gs) || conv2d_ws_tail_geom_ok(gs) || !conv_mfma_supported(gs, precision)) continue;
    v.cg = gs;
    v.d.in0 = c.d.in0;
    v.exo_src = c.d.in1;
    v.fam = Fam::MFMA;
    c.fused_away = true;
  }
}

// ---- inference plans: a skip add right behind a 2-D 64 -> 64 k conv that
// already carries a residual (the last block's sum + the big skip of
// sup3rcc/gen_*_5x_1x_* at hi-res) is absorbed into that conv's store on the
// weights-stationary kernel (ConvGeom::res2): conv.out := add.out, the add
// never runs.  Verified with the dtypes below, like the concat split.
static void plan_ws_res2(s3_plan* pl) {
  const int precision = pl->precision, training = pl->training, output = pl->output;
  const int n_ops = (int)pl->ops.size();
  if (training || precision != S3_PREC_BF16 || s3_opt_has(S3O_NO_WS_RES2) || s3_opt_has(S3O_FP32_ACT) ||
      s3_opt_has(S3O_NO_ADD16) || tl_no_ws_exo)
    return;
  for (int i = 0; i < n_ops; ++i) {
    OpRec& a = pl->ops[i];
    if (a.d.kind != S3_OP_ADD || a.d.bcast_c || a.fused_away) continue;
    for (int side = 0; side < 2; ++side) {
      const int t_conv = side ? a.d.in1 : a.d.in0, t_other = side ? a.d.in0 : a.d.in1;
      const int rt = root_of(pl, t_conv);
      if (rt == root_of(pl, output) || rt == root_of(pl, t_other)) continue;
      int prod = -1, n_use = 0;
      for (int k = 0; k < n_ops; ++k) {
        const s3_op_desc& u = pl->ops[k].d;
        if (u.kind != S3_OP_VIEW && root_of(pl, u.out) == rt) prod = k;
        for (int id : {u.in0, u.in1, u.res})
          if (id >= 0 && root_of(pl, id) == rt) ++n_use;
      }
      if (prod < 0 || prod >= i || n_use != 1) continue;
      OpRec& c = pl->ops[prod];
      if (c.d.kind != S3_OP_CONV || c.res2_src >= 0 || c.d.res < 0 || c.cg.act != S3_ACT_NONE || c.cg.d2s != 1 ||
          c.cg.w_cin || c.fam != Fam::MFMA || !conv2d_ws_geom_ok(c.cg) || conv2d_ws_tail_geom_ok(c.cg))
        continue;
      // (the other operand must exist before the conv runs)
      int prod_other = -1;
      for (int k = 0; k < n_ops; ++k)
        if (pl->ops[k].d.kind != S3_OP_VIEW && root_of(pl, pl->ops[k].d.out) == root_of(pl, t_other)) prod_other = k;
      if (prod_other >= prod) continue;
      c.res2_src = t_other;
      c.d.out = a.d.out;
      a.fused_away = true;
      break;
    }
  }
}

// ---- activation dtypes.  Inference plans in bf16 mode keep a tensor in
// bf16 when its producer can write it (MFMA conv, direct conv, index op) and
// EVERY consumer can read it (MFMA conv input / residual, index op);
// everything else — plan inputs/outputs, training plans, f32 mode — is fp32.
// Training plans (SUP3R_AMD_BF16_TRAIN_ACT=0 opts out): the same, but a saved
// activation is also read by the backward pass — a tensor stays bf16 only if
// every conv that consumes it takes its weight gradient through the
// transpose-read bf16 kernel (which stages bf16 directly); the LeakyReLU
// mask pass reads the sign of a bf16 output; gradients stay fp32.  The
// forward is then bit-identical to the bf16 inference plan of the trunk.
static void plan_dtypes(s3_plan* pl) {
  const int precision = pl->precision, training = pl->training, output = pl->output;
  const int n_tensors = (int)pl->t.size();
  const bool train16 = training && precision == S3_PREC_BF16 && !s3_opt_has(S3O_FP32_ACT) &&
                       !(s3_opt_has(S3O_BF16_TRAIN_ACT) && s3_opt_int(S3O_BF16_TRAIN_ACT, 0) == 0);
  if ((!training || train16) && precision == S3_PREC_BF16 && !s3_opt_has(S3O_FP32_ACT)) {
    std::vector<int> dt(n_tensors, 1);
    auto demote = [&](int id, bool& changed) {
      if (id < 0) return;
      int r = root_of(pl, id);
      if (dt[r]) { dt[r] = 0; changed = true; }
    };
    bool changed = true;
    {
      bool c0 = false;
      for (int id : pl->inputs) demote(id, c0);
      demote(output, c0);
      // tensors nobody produces (defensive) stay fp32
      std::vector<char> produced(n_tensors, 0);
      for (auto& o : pl->ops) produced[root_of(pl, o.d.out)] = 1;
      for (int i = 0; i < n_tensors; ++i)
        if (!produced[root_of(pl, i)]) demote(i, c0);
    }
    // outputs of the few-channel gather conv: bf16 only towards a conv INPUT
    // (the consumer rounds to bf16 when it stages anyway, so nothing changes
    // numerically); as a residual the fp32 value is kept
    std::vector<char> fewch_out(n_tensors, 0);
    for (auto& o : pl->ops)
      if (o.d.kind == S3_OP_CONV && o.gconv() && o.cg.Cin <= 4) fewch_out[root_of(pl, o.d.out)] = 1;
    while (changed) {
      changed = false;
      for (auto& o : pl->ops) {
        const s3_op_desc& d = o.d;
        if ((d.kind == S3_OP_CONCAT || d.kind == S3_OP_ADD) && o.fused_away) continue;   // (never runs: its operands go to the conv)
        switch (d.kind) {
          case S3_OP_CONV:
            if (training && d.res >= 0 && fewch_out[root_of(pl, d.res)]) demote(d.res, changed);
            if (o.fam == Fam::MFMA) {
              if (!conv_mfma_bf16_out_ok(o.cg)) demote(d.out, changed);
              if (o.cg.Cin % 8 != 0) demote(d.in0, changed);   // (logical-axes kernel: 16-B bf16 chunks)
              // (a saved bf16 input is re-read by the weight gradient: the
              // transpose-read kernels stage bf16 directly)
              // (round 5: ... and so does the 2-D weight gradient, so that the
              // 64 -> 64 layers of a 2-D training plan keep bf16 cells and run
              // forward on the weights-stationary kernel)
              if (training && o.wgrad != Wgrad::BF16_TRUNK && !(o.wgrad == Wgrad::BF16_GEN && !s3_opt_has(S3O_NO_DISC_BF16)) &&
                  !(o.wgrad == Wgrad::BF16_2D && o.cg.Cin % 8 == 0 && !s3_opt_has(S3O_NO_TRAIN2D_BF16)))
                demote(d.in0, changed);
            } else if (training) {
              // every other conv reads / writes fp32 in training plans — except
              // the hi-res tail conv, whose MFMA forward takes bf16 cells and
              // whose weight gradient (conv_wgrad_tail_kernel) stages them as is
              const bool tail16 = d.res < 0 && o.wgrad == Wgrad::TAIL && conv_tail_mfma_supported(o.cg);
              // ... and the hi-res discriminator pair: the few-channel conv
              // (C_in <= 4) may write bf16 when its consumer is a gather-MFMA
              // conv (bf16 cells in, C_in % 8 == 0) whose weight gradient is
              // the general transpose-read kernel (bf16 staging)
              // ... and so on down the stack: every gather-MFMA / LDS-halo conv with
              // C_in % 8 == 0 takes and writes bf16 cells (SUP3R_AMD_DISC_BF16=1
              // keeps it to the first pair, SUP3R_AMD_NO_DISC_BF16 turns it off)
              const bool disc16 = !s3_opt_has(S3O_NO_DISC_BF16);
              const bool deep16 = disc16 && !(s3_opt_has(S3O_DISC_BF16) && s3_opt_int(S3O_DISC_BF16, 0) == 1);
              const bool gc_in16 = disc16 && o.gconv() && (o.fam != Fam::HALO32 || deep16) && d.res < 0 && o.wgrad == Wgrad::BF16_GEN &&
                                   o.cg.Cin % 8 == 0;
              const bool gc_out16 = disc16 && o.gconv() && d.res < 0 && o.cg.Cout % 8 == 0 &&
                                    (o.cg.Cin == 2 || o.cg.Cin == 4 || (deep16 && o.cg.Cin % 8 == 0));
              if (!tail16 && !gc_in16) demote(d.in0, changed);
              demote(d.res, changed);
              if (!gc_out16) demote(d.out, changed);
            } else {
              // the direct kernels read fp32, except the small-channel tail
              // convs (MFMA C_in = 8 / sliding window) which take bf16 cells
              const bool small = d.res < 0 && !o.fewpos() &&
                                 (conv_small_supported(o.cg, 1) || conv_tail_mfma_supported(o.cg));
              if (!small) demote(d.in0, changed);
              demote(d.res, changed);
              if (small || o.fewpos()) demote(d.out, changed);
            }
            break;
          case S3_OP_REPEAT_T: case S3_OP_D2S: case S3_OP_PAD: case S3_OP_CROP:
          case S3_OP_ROLL_T: case S3_OP_DILATE:
            if (dt[root_of(pl, d.in0)] != dt[root_of(pl, d.out)]) {
              demote(d.in0, changed);
              demote(d.out, changed);
            }
            break;
          case S3_OP_VIEW:
            break;  // alias: one root, one dtype (element count is preserved)
          case S3_OP_ADD:
            // inference plans: a skip add stays in bf16 when both operands and
            // the sum are bf16 tensors (add16_kernel)
            if (training || d.bcast_c || (pl->t[d.out].numel & 7) || s3_opt_has(S3O_NO_ADD16) ||
                !(dt[root_of(pl, d.in0)] && dt[root_of(pl, d.in1)] && dt[root_of(pl, d.out)])) {
              demote(d.in0, changed); demote(d.in1, changed); demote(d.out, changed);
            }
            break;
          default:
            demote(d.in0, changed); demote(d.in1, changed);
            demote(d.res, changed); demote(d.out, changed);
            break;
        }
      }
    }
    for (int i = 0; i < n_tensors; ++i) pl->t[i].dtype = dt[root_of(pl, i)];
  }
  for (auto& o : pl->ops) {
    if (o.d.kind != S3_OP_CONV) continue;
    o.io.in_bf16 = pl->t[root_of(pl, o.d.in0)].dtype;
    o.io.out_bf16 = pl->t[root_of(pl, o.d.out)].dtype;
    o.io.res_bf16 = o.d.res >= 0 ? pl->t[root_of(pl, o.d.res)].dtype : 0;
  }
}

// (2-D convs on the weights-stationary kernel: never launched off it)
static void plan_ws_only(s3_plan* pl) {
  const int precision = pl->precision;
  for (auto& o : pl->ops)
    if (o.d.kind == S3_OP_CONV && o.fam == Fam::MFMA && conv_mfma_is_gen(o.cg, precision) && o.cg.in_rep <= 1 &&
        conv2d_ws_supported(o.cg, precision, o.io, o.d.res >= 0))
      o.cg.ws_only = 1;
}

// with the dtypes known: can the weights-stationary kernel still take every
// conv that plan_ws_exo / plan_ws_res2 split or extended?
static bool plan_ws_split_holds(const s3_plan* pl) {
  const int precision = pl->precision;
  for (auto& o : pl->ops) {
    if (o.d.kind != S3_OP_CONV || (o.exo_src < 0 && o.res2_src < 0)) continue;
    if (conv2d_ws_supported(o.cg, precision, o.io, o.d.res >= 0) &&
        (o.res2_src < 0 || pl->t[root_of(pl, o.res2_src)].dtype == 1))
      continue;
    return false;
  }
  return true;
}

// ---- activation-adjoint fusion (training): a conv whose data gradient runs
// on conv_dgrad_s2_kernel and whose input is the fp32 output of an activated
// conv with no other consumer applies that conv's mask in its own store
static void plan_mask_fusion(s3_plan* pl) {
  const int training = pl->training, output = pl->output;
  const int n_ops = (int)pl->ops.size(), n_tensors = (int)pl->t.size();
  if (!training) return;
  std::vector<int> ncons(n_tensors, 0), prod(n_tensors, -1);
  for (int i = 0; i < n_ops; ++i) {
    const s3_op_desc& d = pl->ops[i].d;
    for (int id : {d.in0, d.in1, d.res})
      if (id >= 0) ++ncons[root_of(pl, id)];
    if (d.kind != S3_OP_VIEW) prod[root_of(pl, d.out)] = i;
  }
  for (auto& o : pl->ops) {
    if (o.d.kind == S3_OP_CONV) {
      const int pr = prod[root_of(pl, o.d.in0)];
      if (pr >= 0 && pl->ops[pr].d.kind == S3_OP_CONV) o.in_prod = pr;
    }
    // (the stride-2 dgrad kernel masks from an fp32 y; the frame fold of the
    // halo-tile dgrad from fp32 or bf16)
    const bool fold = (dgrad_is_mfma(o.dgrad) && !dgrad_is_valid(o.dgrad)) ||
                      (o.dgrad == Dgrad::FEWPOS_MFMA && o.cg.pad_mode == S3_PAD_REFLECT);   // (the one-launch fewpos dgrad folds its frame too)
    if (o.d.kind != S3_OP_CONV || !(dgrad_is_s2(o.dgrad) || fold)) continue;
    const int r = root_of(pl, o.d.in0);
    const int pi = prod[r];
    if (pi < 0 || ncons[r] != 1 || r == root_of(pl, output) || pl->t[r].is_input) continue;

    if (fold && (o.cg.Cin & 3)) continue;
    const OpRec& po = pl->ops[pi];
    if (po.d.kind == S3_OP_CONV && po.cg.act != S3_ACT_NONE && po.cg.d2s == 1 && po.d.res < 0)
      o.mask_prod = pi;
  }
}

// ---- inference plans: a temporal repeat whose only consumer is a conv on
// the persistent trunk kernel is read through that kernel's halo index
// (cell t of the repeated tensor = cell t / rep of the source) instead of
// being written out and read back (at C2 batch 32 the 96 -> 288
// repeat alone is a 400 MB store + load per forward)
static void plan_repeat_fusion(s3_plan* pl) {
  s3_ctx* ctx = pl->ctx;
  const int precision = pl->precision, training = pl->training, output = pl->output;
  const int n_ops = (int)pl->ops.size();
  if (training || precision != S3_PREC_BF16 || s3_opt_has(S3O_NO_REPEAT_FUSE)) return;
  for (int i = 0; i < n_ops; ++i) {
    OpRec& r = pl->ops[i];
    if (r.d.kind != S3_OP_REPEAT_T || !conv_mfma_persist_rep_ok(r.d.rep)) continue;
    const int rt = root_of(pl, r.d.out);
    if (rt == root_of(pl, output) || pl->t[root_of(pl, r.d.in0)].dtype != pl->t[rt].dtype) continue;
    // every consumer is a plain 64 -> 64 trunk conv on the persistent kernel
    // ('same' extents, one padding for all axes, no depth-to-space store)
    // taking it as the input or as the residual — SkipConnection sources sit
    // right behind the last temporal expansion in the reference's generators
    // — and carries no other repeat factor yet
    bool ok = true;
    int n_use = 0;
    for (int k = 0; k < n_ops && ok; ++k) {
      const OpRec& c = pl->ops[k];
      const bool as_in = c.d.in0 >= 0 && root_of(pl, c.d.in0) == rt;
      const bool as_in1 = c.d.in1 >= 0 && root_of(pl, c.d.in1) == rt;
      const bool as_res = c.d.res >= 0 && root_of(pl, c.d.res) == rt;
      if (!as_in && !as_in1 && !as_res) continue;
      ++n_use;
      ok = k > i && !as_in1 && c.d.kind == S3_OP_CONV && c.fam == Fam::MFMA &&
           conv_mfma_persist_supported(ctx, c.cg, c.io, c.d.res >= 0) && c.cg.d2s == 1 && c.cg.Cout == 64 &&
           c.cg.O[2] < 32768 && c.cg.O[2] % r.d.rep == 0;
      for (int q = 0; q < 3; ++q) ok = ok && c.cg.lo[q] == c.cg.lo[0] && c.cg.O[q] == c.cg.D[q];
      const int have = c.cg.in_rep > 1 ? c.cg.in_rep : c.cg.res_rep;
      if (have > 1 && have != r.d.rep) ok = false;
    }
    if (!ok || !n_use) continue;
    for (int k = i + 1; k < n_ops; ++k) {
      OpRec& c = pl->ops[k];
      if (c.d.kind != S3_OP_CONV) continue;
      if (root_of(pl, c.d.in0) == rt) { c.cg.in_rep = r.d.rep; c.rep_src = r.d.in0; }
      if (c.d.res >= 0 && root_of(pl, c.d.res) == rt) { c.cg.res_rep = r.d.rep; c.res_src = r.d.in0; }
    }
    r.fused_away = true;
  }
}

// ---- (training) bf16 copy of dPre for the MFMA gradient kernels (they round their
// operand to bf16 anyway; a bf16 source halves the bytes they stage, and
// the persistent data gradient / the wave-specialised weight gradient take
// nothing else).  Whichever pass finishes a conv's dPre leaves it: the mask
// pass (d2s walk included), the frame folds (compile-time variants: a
// run-time side store cost them 42 us per 75 MB), the stride-2 data
// gradient.  One buffer, handed from producer to consumer (dpre16_for).
// Which convs stage it (OpRec::use16), which of them write their padded frame as
// bf16 (OpRec::dgrad_frame16), and the size of the buffer; reads mask_prod.
static void plan_dpre16(s3_plan* pl, WorkspaceSizes& ws) {
  s3_ctx* ctx = pl->ctx;
  const int precision = pl->precision, training = pl->training;
  if (!training) return;
  if (precision == S3_PREC_BF16 && !s3_opt_has(S3O_NO_DPRE16)) {
    size_t max16 = 0;
    for (auto& o : pl->ops) {
      // (no look at the allocations: a plan whose allocation fails is destroyed before anyone reads these flags)
      if (o.d.kind != S3_OP_CONV) continue;
      // (... and the gather-MFMA adjoint of the strided / valid discriminator
      // convs: a lane's 8 channels of a dPre cell are one 16-B load)
      const bool gadj = o.dgrad == Dgrad::GCONV && (o.cg.Cout & 7) == 0 && o.cg.pad_mode != S3_PAD_REFLECT &&
                        !s3_opt_has(S3O_NO_GCONV_DY16);
      if (!gadj && (!dgrad_is_mfma(o.dgrad) || o.dgrad == Dgrad::FEWCH || (o.cg.Cout & 3))) continue;
      if (o.dgrad == Dgrad::GEN && (o.cg.Cout & 7)) continue;   // (16-B bf16 chunks of a dPre cell)
      if (dgrad_is_chunked(o.dgrad) && ((o.cg.Cout & 7) || s3_opt_has(S3O_NO_CHUNKED_DY16))) continue;
      o.use16 = true;
      max16 = std::max(max16, (size_t)pl->t[root_of(pl, o.d.out)].numel * 2);
      // the reflect-padded 64 -> 64 trunk conv on the persistent kernel:
      // its padded frame is written — and folded from — as bf16
      o.dgrad_frame16 = training && (o.dgrad == Dgrad::MFMA_FRAME || o.dgrad == Dgrad::GEN) &&
                        o.dg.Cout == 64 && (o.cg.Cin & 3) == 0 && o.cg.pad_mode == S3_PAD_REFLECT &&
                        conv_mfma_persist_dgrad_supported(ctx, o.dg) && !s3_opt_has(S3O_NO_FRAME16);
      // ... and so is the frame of a 2-D 64 -> 64 k conv's data gradient on the
      // weights-stationary kernel
      if (training && o.dgrad == Dgrad::GEN && conv2d_ws_frame_geom_ok(o.dg) &&
          !s3_opt_has(S3O_NO_FRAME16) && !s3_opt_on(S3O_NO_CONV2D_WS))
        o.dgrad_frame16 = true;
    }
    // ... and for the stride-2 data gradient that stores dPre of the
    // few-channel conv below it as bf16 only (see the dgrad_s2 branch)
    for (auto& o : pl->ops)
      if (o.d.kind == S3_OP_CONV && dgrad_is_s2(o.dgrad) && o.mask_prod >= 0 && pl->ops[o.mask_prod].wgrad == Wgrad::C2 &&
          conv_dgrad_s2_out16_ok(o.cg))
        max16 = std::max(max16, (size_t)pl->t[root_of(pl, o.d.in0)].numel * 2);
    ws.dpre16 = max16;
  }
}

static int plan_arena(s3_plan* pl, size_t& max_t) {
  const int training = pl->training, output = pl->output;
  const int n_ops = (int)pl->ops.size(), n_tensors = (int)pl->t.size();
  // ---- static arena planning.  Training keeps every tensor; inference
  // reuses buffers by liveness (greedy best-fit).
  std::vector<int> last_use(n_tensors, -1);
  for (int i = 0; i < n_ops; ++i) {
    const s3_op_desc& d = pl->ops[i].d;
    int ids[8] = {d.in0, d.in1, d.res, d.out, pl->ops[i].rep_src, pl->ops[i].res_src, pl->ops[i].exo_src,
                  pl->ops[i].res2_src};
    for (int q = 0; q < 8; ++q)
      if (ids[q] >= 0) last_use[root_of(pl, ids[q])] = i;
  }
  last_use[root_of(pl, output)] = n_ops + 1;
  std::vector<size_t> bsize;
  std::vector<int> bfree_at;  // op index after which the buffer is free
  for (int i = 0; i < n_ops; ++i) {
    const s3_op_desc& d = pl->ops[i].d;
    if (d.kind == S3_OP_VIEW) continue;
    if ((d.kind == S3_OP_CONCAT || d.kind == S3_OP_ADD) && pl->ops[i].fused_away) continue;   // (never materialised / written by the conv)
    TensorRec& ot = pl->t[d.out];
    size_t need = ot.bytes();
    int pick = -1;
    // (option KEEP_ACTIVATIONS: an inference plan with a buffer per tensor, so that a
    // test can read every op's output — s3_plan_tensor_read — of the kernels and
    // fusions only inference plans select)
    if (!training && !s3_opt_has(S3O_KEEP_ACTIVATIONS)) {
      for (int b = 0; b < (int)bsize.size(); ++b)
        if (bfree_at[b] < i && bsize[b] >= need &&
            (pick < 0 || bsize[b] < bsize[pick]))
          pick = b;
    }
    if (pick < 0) { bsize.push_back(need); bfree_at.push_back(0); pick = (int)bsize.size() - 1; }
    ot.buffer = pick;
    bfree_at[pick] = last_use[d.out];
    max_t = std::max(max_t, need);
  }
  for (int i = 0; i < n_tensors; ++i) max_t = std::max(max_t, (size_t)pl->t[i].numel * sizeof(float));
  pl->buffers.resize(bsize.size());
  pl->buffer_bytes = bsize;
  for (size_t b = 0; b < bsize.size(); ++b) {
    int rc = plan_alloc(pl, (void**)&pl->buffers[b], bsize[b]);
    if (rc) return rc;
  }
  for (int i = 0; i < n_tensors; ++i)
    if (pl->t[i].buffer >= 0) pl->t[i].ptr = pl->buffers[pl->t[i].buffer];
  return S3_OK;
}

static int plan_workspace(s3_plan* pl, const WorkspaceSizes& ws, size_t max_t) {
  s3_ctx* ctx = pl->ctx;
  const int precision = pl->precision, training = pl->training;
  const int n_tensors = (int)pl->t.size();
  if (training) {
    for (int i = 0; i < n_tensors; ++i) {
      if (pl->t[i].alias_root >= 0) continue;
      int rc = plan_alloc(pl, (void**)&pl->t[i].gptr, (size_t)pl->t[i].numel * sizeof(float));
      if (rc) return rc;
    }
    int rc = plan_alloc(pl, (void**)&pl->dpre, ws.dpre);
    // (its bf16 copy, sized by plan_dpre16)
    if (!rc && ws.dpre16) rc = plan_alloc(pl, &pl->dpre16, ws.dpre16);
    pl->dpre16_bytes = ws.dpre16;
    if (!rc) rc = plan_alloc(pl, (void**)&pl->gtmp, max_t);
    if (!rc) rc = plan_alloc(pl, (void**)&pl->bsum, (size_t)4096 * 256 * sizeof(float));
    if (!rc) rc = plan_alloc(pl, (void**)&pl->bsum2, (size_t)4096 * 256 * sizeof(float));
    if (!rc && ws.partial) {
      rc = plan_alloc(pl, (void**)&pl->wg_partial, ws.partial);
      pl->wg_partial_bytes = ws.partial;
    }
    if (!rc && ws.dxp) rc = plan_alloc(pl, (void**)&pl->dxp, ws.dxp);
    for (auto& o : pl->ops) {
      if (rc || o.d.kind != S3_OP_CONV || !dgrad_is_mfma(o.dgrad)) continue;
      rc = plan_alloc(pl, (void**)&o.dg_w32, (size_t)27 * o.cg.Cin * o.cg.Cout * sizeof(float));
      if (!rc && dgrad_is_chunked(o.dgrad)) {
        for (int k = 0; !rc && k < (o.cg.Cout + 63) / 64; ++k)
          rc = plan_alloc(pl, &o.dgc_wbf[k], conv_mfma_packed_bytes(o.dg, precision));
        continue;
      }
      if (!rc && precision != S3_PREC_F32)
        rc = plan_alloc(pl, &o.dg_wbf, o.dgrad == Dgrad::FEWCH ? conv_gconv_packed_bytes(o.dg, 0, precision == S3_PREC_BF16X3)
                                                     : conv_mfma_packed_bytes(o.dg, precision));
    }
    if (rc) return rc;
  }
  if (ws.fp) {
    int rc = plan_alloc(pl, (void**)&pl->fp_partial, ws.fp);
    if (rc) return rc;
    pl->fp_partial_bytes = ws.fp;
  }
  if (training) {
    for (auto& o : pl->ops) {
      if (o.d.kind != S3_OP_CONV || !o.fewpos()) continue;
      int rc = plan_alloc(pl, (void**)&o.fp_wt, (size_t)o.cg.k[0] * o.cg.k[1] * o.cg.k[2] * o.cg.Cin * o.cg.Cout * sizeof(float));
      if (rc) return rc;
    }
  }
  // packed weights of the MFMA convs
  for (auto& o : pl->ops) {
    if (o.d.kind == S3_OP_CONV && o.fam == Fam::MFMA) {
      int rc = plan_alloc(pl, &o.packed, conv_mfma_packed_bytes(o.cg, precision));
      if (rc) return rc;
    }
  }
  for (auto& o : pl->ops) {
    if (o.d.kind != S3_OP_CONV) continue;
    if (o.gconv()) {
      int rc = plan_alloc(pl, &o.gc_w, conv_gconv_packed_bytes(o.cg, 0, precision == S3_PREC_BF16X3));
      if (rc) return rc;
    }
    if (o.fam == Fam::HALO32 || o.fam == Fam::HALO_S2) {
      int rc = plan_alloc(pl, &o.h32_w, o.fam == Fam::HALO32 ? conv_halo32_packed_bytes(o.cg) : conv_halo_s2_packed_bytes(o.cg));
      if (rc) return rc;
    }
    if (dgrad_is_s2(o.dgrad)) {
      int rc = plan_alloc(pl, &o.dc2_w, precision == S3_PREC_BF16X3 ? conv_dgrad_s2_x3_packed_bytes(o.cg)
                                                                    : conv_dgrad_s2_packed_bytes(o.cg));
      if (rc) return rc;
      // its fused activation mask as sign bytes written by the producer's
      // forward kernel (4 B instead of 64 B per position read back)
      if (o.mask_prod >= 0 && precision == S3_PREC_BF16 && !s3_opt_has(S3O_NO_SIGN_BYTES)) {
        OpRec& po = pl->ops[o.mask_prod];
        if (po.gconv() && !po.sign_bytes && conv_gconv_writes_sign_bytes(ctx, po.cg, po.io.out_bf16)) {
          const size_t npos = (size_t)po.cg.N * po.cg.O[0] * po.cg.O[1] * po.cg.O[2];
          rc = plan_alloc(pl, &po.sign_bytes, npos * 4);
          if (rc) return rc;
        }
      }
    }
    if (dgrad_is_c2(o.dgrad)) {
      int rc = plan_alloc(pl, &o.dc2_w, precision == S3_PREC_BF16X3 ? conv_dgrad_c2_x3_packed_bytes()
                                                                    : conv_dgrad_c2_packed_bytes());
      if (rc) return rc;
    }
    if (o.dgrad == Dgrad::GCONV) {
      int rc = plan_alloc(pl, &o.gc_wt, conv_gconv_packed_bytes(o.cg, 1, precision == S3_PREC_BF16X3));
      if (rc) return rc;
    }
  }
  // staging copies of the graph inputs: fixed pointers for the hipGraph replay
  if (!training) {
    for (size_t i = 0; i < pl->inputs.size(); ++i) {
      void* st = nullptr;
      int rc = plan_alloc(pl, &st, (size_t)pl->t[pl->inputs[i]].numel * sizeof(float));
      if (rc) return rc;
      pl->in_stage.push_back((float*)st);
    }
  }
  pl->bw.reset(n_tensors);
  return S3_OK;
}

static void plan_fused2d(s3_plan* pl) {
  s3_ctx* ctx = pl->ctx;
  const int precision = pl->precision, training = pl->training, output = pl->output;
  const int n_tensors = (int)pl->t.size();
  const s3_params* params = pl->params;
  // small 2-D conv stacks (the spatial generators at test / C1 sizes): one launch
  // for the whole op list, activations in LDS
  if (!training && precision == S3_PREC_BF16 && pl->inputs.size() == 1) {
    std::vector<Fused2dLayer> fl;
    bool ok = true;
    for (auto& o : pl->ops) {
      if (o.d.kind != S3_OP_CONV) { ok = false; break; }
      Fused2dLayer f;
      f.g = o.cg;
      f.in_t = root_of(pl, o.d.in0);
      f.out_t = root_of(pl, o.d.out);
      f.res_t = o.d.res >= 0 ? root_of(pl, o.d.res) : -1;
      f.w_off = params->p[o.d.w].offset;
      f.b_off = o.d.b >= 0 ? params->p[o.d.b].offset : -1;
      fl.push_back(f);
    }
    if (ok) pl->fused2d = fused2d_build(ctx, fl, n_tensors, root_of(pl, pl->inputs[0]), root_of(pl, output));
    if (s3_opt_has(S3O_TRACE))
      fprintf(stderr, "[plan] fused 2-D whole-network kernel: %s\n", pl->fused2d ? "yes" : "no");
  }
}


// one line per conv under the TRACE option, once the dtypes are known (the
// tests read the family / gradient kernels from it)
static void plan_trace(const s3_plan* pl) {
  if (!s3_opt_has(S3O_TRACE)) return;
  for (const OpRec& o : pl->ops) {
    if (o.d.kind != S3_OP_CONV) continue;
    const Wgrad w = o.wgrad;
    const Dgrad d = o.dgrad;
    fprintf(stderr, "[plan] conv %d->%d %s: mfma %d fewpos %d gconv %d halo32 %d | in16 %d out16 %d res16 %d | "
            "wgrad bf16 %d gen %d 2d %d c2 %d tail %d mfma %d | dgrad mfma %d c2 %d s2 %d gconv %d\n",
            o.cg.Cin, o.cg.Cout, pl->training ? "train" : "infer", o.fam == Fam::MFMA, o.fewpos(), o.gconv(),
            o.fam == Fam::HALO32, o.io.in_bf16, o.io.out_bf16, o.io.res_bf16, w == Wgrad::BF16_TRUNK,
            w == Wgrad::BF16_GEN, w == Wgrad::BF16_2D, w == Wgrad::C2, w == Wgrad::TAIL,
            w == Wgrad::BF16_TRUNK || w == Wgrad::F32_TRUNK, dgrad_is_mfma(d), dgrad_is_c2(d), dgrad_is_s2(d),
            d == Dgrad::GCONV);
  }
}

extern "C" int s3_plan_create_opt(s3_ctx* ctx, s3_params* params,
                                  const s3_tensor_desc* tensors, int n_tensors,
                                  const s3_op_desc* ops, int n_ops,
                                  const int32_t* inputs, int n_inputs,
                                  int32_t output, int precision, int training,
                                  const s3_plan_options* options, s3_plan** out) {
  if (!ctx || !params || !tensors || !ops || !out) return S3_EINVAL;
  if (output < 0 || output >= n_tensors) S3_FAIL(ctx, S3_EINVAL, "plan: bad output id");
  S3Options plan_opt = ctx->opt;
  if (int orc = apply_options(ctx, plan_opt, options)) return orc;
  s3_plan* pl = new s3_plan();
  pl->opt = plan_opt;
  S3OptScope opt_scope(&pl->opt);
  pl->ctx = ctx; pl->params = params; pl->precision = precision;
  pl->training = training; pl->output = output;
  pl->t.resize(n_tensors);
  for (int i = 0; i < n_tensors; ++i) {
    memcpy(pl->t[i].dims, tensors[i].dims, sizeof(int64_t) * 5);
    pl->t[i].numel = numel5(tensors[i].dims);
    if (pl->t[i].numel <= 0) { delete pl; S3_FAIL(ctx, S3_EINVAL, "plan: empty tensor"); }
  }
  for (int i = 0; i < n_inputs; ++i) {
    if (inputs[i] < 0 || inputs[i] >= n_tensors) { delete pl; S3_FAIL(ctx, S3_EINVAL, "plan: bad input id"); }
    pl->inputs.push_back(inputs[i]);
    pl->t[inputs[i]].is_input = true;
  }
  pl->ops.resize(n_ops);
  WorkspaceSizes ws;
  if (int rc = plan_select(pl, ops, ws)) { delete pl; return rc; }
  plan_ws_exo(pl);
  plan_ws_res2(pl);
  plan_dtypes(pl);
  plan_trace(pl);
  plan_ws_only(pl);
  if (!plan_ws_split_holds(pl)) {
    // (a consumer of the 64-channel tensor that needs fp32 cells, ...): build
    // the plan again with the concat as it is written
    delete pl;
    ++tl_no_ws_exo;
    const int rc = s3_plan_create_opt(ctx, params, tensors, n_tensors, ops, n_ops, inputs, n_inputs, output,
                                      precision, training, options, out);
    --tl_no_ws_exo;
    return rc;
  }

  plan_mask_fusion(pl);
  plan_dpre16(pl, ws);
  plan_repeat_fusion(pl);
  for (auto& o : pl->ops)
    if (o.d.kind == S3_OP_CONV) o.fwd = resolve_fwd(ctx, o, precision);
  size_t max_t = 0;
  int rc = plan_arena(pl, max_t);
  if (!rc) rc = plan_workspace(pl, ws, max_t);
  if (rc) { s3_plan_destroy(pl); return rc; }
  plan_fused2d(pl);
  *out = pl;
  return S3_OK;
}

void graph_drop(s3_plan* pl) {
  if (pl->graph_exec) (void)hipGraphExecDestroy(pl->graph_exec);
  if (pl->graph) (void)hipGraphDestroy(pl->graph);
  pl->graph_exec = nullptr;
  pl->graph = nullptr;
}

extern "C" void s3_plan_destroy(s3_plan* pl) {
  if (!pl) return;
  (void)hipStreamSynchronize(pl->ctx->stream);
  graph_drop(pl);
  if (pl->cap_stream) (void)hipStreamDestroy(pl->cap_stream);
  for (auto& e : pl->prof_ev) (void)hipEventDestroy(e);
  for (void* p : pl->owned) (void)hipFree(p);
  fused2d_free(pl->fused2d);
  delete pl;
}
