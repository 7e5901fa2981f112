// The forward pass of a plan: the batched filter re-pack, the dispatch of one
// op on the kernel chosen for it (plan.cpp), the optional hipGraph replay, the
// per-op profile and the windowed forward of the chunk executor.
#include <algorithm>
#include <cstdio>

#include "plan_internal.h"

// ---- batched filter re-pack.  After an optimizer step every bf16 conv of the
// plan needs its images again; instead of 1 - 3 launches of ~5 us per conv and
// direction (lazily, in front of each conv) one launch per direction walks a
// device table of jobs.  Convs outside the table (other precisions, chunked /
// few-channel data gradients, gather-MFMA convs) keep their lazy packs.
static int pack_tables_build(s3_plan* pl) {
  s3_ctx* ctx = pl->ctx;
  pl->pack_built = true;
  if (pl->precision != S3_PREC_BF16 || s3_opt_has(S3O_NO_BATCHED_PACK)) return S3_OK;
  s3_params* P = pl->params;
  float* W = P->buf[S3_BUF_W];
  std::vector<S3PackJob> fwd, bwd;
  for (int i = 0; i < (int)pl->ops.size(); ++i) {
    OpRec& o = pl->ops[i];
    if (o.d.kind != S3_OP_CONV) continue;
    const ConvGeom& g = o.cg;
    const bool k3 = g.k[0] == 3 && g.k[1] == 3 && g.k[2] == 3;
    if (o.fam == Fam::MFMA && o.packed && g.Cin == 64 && k3 && !conv_mfma_is_gen(g, pl->precision)) {
      S3PackJob j;
      j.w = W + P->p[o.d.w].offset;
      j.cout = g.Cout; j.n_ct = (g.Cout + 63) / 64; j.dgrad = 0;
      j.tile = (unsigned short*)o.packed;
      j.persist = conv_mfma_persist_geom_ok(g) ? j.tile + (size_t)j.n_ct * 27 * 64 * 64 : nullptr;
      fwd.push_back(j); pl->pack_fwd_ops.push_back(i);
      pl->pack_fwd_ct = std::max(pl->pack_fwd_ct, j.n_ct);
    }
    if (pl->training && (o.dgrad == Dgrad::MFMA_FRAME || o.dgrad == Dgrad::MFMA_VALID) && o.dg_wbf && g.Cout == 64 && k3 &&
        o.dg.Cin == 64) {
      S3PackJob j;
      j.w = W + P->p[o.d.w].offset;
      j.cout = g.Cin; j.n_ct = (g.Cin + 63) / 64; j.dgrad = 1;
      j.tile = (unsigned short*)o.dg_wbf;
      j.persist = conv_mfma_persist_dgrad_geom_ok(o.dg) ? j.tile + (size_t)j.n_ct * 27 * 64 * 64 : nullptr;
      bwd.push_back(j); pl->pack_bwd_ops.push_back(i);
      pl->pack_bwd_ct = std::max(pl->pack_bwd_ct, j.n_ct);
    }
  }
  if (fwd.size() >= 2) {
    int rc = plan_alloc(pl, (void**)&pl->pack_fwd, fwd.size() * sizeof(S3PackJob));
    if (rc) return rc;
    S3_HIP(ctx, hipMemcpyAsync(pl->pack_fwd, fwd.data(), fwd.size() * sizeof(S3PackJob), hipMemcpyHostToDevice, ctx->stream));
    S3_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the host vector goes away)
  } else {
    pl->pack_fwd_ops.clear();
  }
  if (bwd.size() >= 2) {
    int rc = plan_alloc(pl, (void**)&pl->pack_bwd, bwd.size() * sizeof(S3PackJob));
    if (rc) return rc;
    S3_HIP(ctx, hipMemcpyAsync(pl->pack_bwd, bwd.data(), bwd.size() * sizeof(S3PackJob), hipMemcpyHostToDevice, ctx->stream));
    S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    pl->pack_bwd_ops.clear();
  }
  return S3_OK;
}

// re-pack every listed conv whose images are stale (all or none: the weights
// of a net change together)
int pack_stale(s3_plan* pl, bool bwd) {
  if (!pl->pack_built) {
    int rc = pack_tables_build(pl);
    if (rc) return rc;
  }
  const std::vector<int>& ops = bwd ? pl->pack_bwd_ops : pl->pack_fwd_ops;
  if (ops.empty()) return S3_OK;
  const uint64_t ver = pl->params->version;
  bool stale = false;
  for (int i : ops) stale = stale || (bwd ? pl->ops[i].dg_version : pl->ops[i].packed_version) != ver;
  if (!stale) return S3_OK;
  int rc = launch_pack_jobs(pl->ctx, bwd ? pl->pack_bwd : pl->pack_fwd, (int)ops.size(),
                            bwd ? pl->pack_bwd_ct : pl->pack_fwd_ct);
  if (rc) return rc;
  for (int i : ops) (bwd ? pl->ops[i].dg_version : pl->ops[i].packed_version) = ver;
  return S3_OK;
}

static int run_op_forward(s3_plan* pl, OpRec& o) {
  s3_ctx* ctx = pl->ctx;
  const uint64_t version = pl->params->version;
  const s3_op_desc& d = o.d;
  const TensorRec& ot = pl->t[d.out];
  switch (d.kind) {
    case S3_OP_CONV: {
      const float* w = wptr(pl, d.w);
      const float* b = wptr(pl, d.b);
      const float* res = d.res >= 0 ? tptr(pl, o.res_src >= 0 ? o.res_src : d.res) : nullptr;
      int rc = S3_OK;
      switch (o.fwd) {
        case Fwd::HALO32:
          rc = repack_if_stale(o.h32_version, version, [&] { return launch_conv_halo32_pack(ctx, o.cg, w, o.h32_w); });
          if (rc) return rc;
          return launch_conv_halo32_fwd(ctx, o.cg, tptr(pl, d.in0), o.h32_w, b, tptr(pl, d.out), o.io.in_bf16,
                                        o.io.out_bf16);
        case Fwd::HALO_S2:
          rc = repack_if_stale(o.h32_version, version, [&] { return launch_conv_halo_s2_pack(ctx, o.cg, w, o.h32_w); });
          if (rc) return rc;
          return launch_conv_halo_s2_fwd(ctx, o.cg, tptr(pl, d.in0), o.h32_w, b, tptr(pl, d.out), o.io.out_bf16);
        case Fwd::TAIL_X3:
          return launch_conv_tail_x3(ctx, o.cg, (const float*)tptr(pl, d.in0), w, b, (float*)tptr(pl, d.out));
        case Fwd::GCONV:
          rc = repack_if_stale(o.gc_version, version, [&] {
            return launch_gconv_pack(ctx, o.cg, w, o.gc_w, 0, pl->precision == S3_PREC_BF16X3);
          });
          if (rc) return rc;
          return launch_gconv_fwd(ctx, o.cg, (const float*)tptr(pl, d.in0), o.gc_w, b, res, tptr(pl, d.out), o.io.out_bf16, o.io.in_bf16,
                                  pl->precision == S3_PREC_BF16X3, o.sign_bytes);
        case Fwd::FEWPOS_MFMA:
          return launch_conv_fewpos_mfma(ctx, o.cg, 0, tptr(pl, d.in0), w, b, res, tptr(pl, d.out));
        case Fwd::FEWPOS:
          return launch_conv_fewpos_fwd(ctx, o.cg, tptr(pl, d.in0), w, b, res, tptr(pl, d.out), pl->fp_partial, pl->fp_partial_bytes);
        default: break;
      }
      if (fwd_is_mfma(o.fwd)) {
        rc = repack_if_stale(o.packed_version, version, [&] { return launch_conv_mfma_pack(ctx, o.cg, pl->precision, w, o.packed); });
        if (rc) return rc;
        const void* wp = pl->precision != S3_PREC_F32 ? (const void*)o.packed : (const void*)w;
        if (o.exo_src >= 0 || o.res2_src >= 0) {
          ConvGeom ge = o.cg;
          if (o.exo_src >= 0) ge.exo = (const float*)tptr(pl, o.exo_src);
          if (o.res2_src >= 0) ge.res2 = tptr(pl, o.res2_src);
          return launch_conv_mfma_fwd_as(ctx, mfma_of(o.fwd), ge, pl->precision, tptr(pl, d.in0), wp, b, res,
                                         tptr(pl, d.out), o.io);
        }
        return launch_conv_mfma_fwd_as(ctx, mfma_of(o.fwd), o.cg, pl->precision,
                                       tptr(pl, o.rep_src >= 0 ? o.rep_src : d.in0), wp, b, res, tptr(pl, d.out), o.io);
      }
      if (pl->win_op >= 0 && &o == &pl->ops[pl->win_op])   // s3_plan_forward_window: checked there
        return launch_conv_tail_mfma(ctx, pl->win_geom, tptr(pl, d.in0), w, b, (float*)tptr(pl, d.out), pl->win_aff);
      return launch_conv_generic_fwd(ctx, generic_of(o.fwd), o.cg, tptr(pl, d.in0), w, b, res, tptr(pl, d.out),
                                     o.io.out_bf16, o.io.in_bf16);
    }
    case S3_OP_DENSE: {
      const TensorRec& it = pl->t[d.in0];
      int rows = (int)(it.numel / it.dims[4]);
      return launch_dense_fwd(ctx, tptr(pl, d.in0), wptr(pl, d.w), wptr(pl, d.b), tptr(pl, d.out), rows, (int)it.dims[4],
                              (int)ot.dims[4], d.act, d.alpha);
    }
    case S3_OP_REPEAT_T: case S3_OP_D2S: case S3_OP_PAD: case S3_OP_CROP:
    case S3_OP_ROLL_T: case S3_OP_DILATE:
      if (o.fused_away) return S3_OK;        // read through its consumer's halo index
      return launch_gather(ctx, o.gg, tptr(pl, d.in0), tptr(pl, d.out), tdtype(pl, d.out) ? 2 : 4);
    case S3_OP_CONCAT: {
      if (o.fused_away) return S3_OK;   // its consumer conv reads both operands (OpRec::exo_src)
      // two channel-range copies: x -> out[..., :Cx], exo -> out[..., Cx:]
      const TensorRec& a = pl->t[d.in0];
      const TensorRec& b = pl->t[d.in1];
      int64_t npos = ot.numel / ot.dims[4];
      int rc = s3_copy_channels(ctx, tptr(pl, d.in0), (int)a.dims[4], 0, tptr(pl, d.out), (int)ot.dims[4], 0, (int)a.dims[4], npos, 0);
      if (rc) return rc;
      return s3_copy_channels(ctx, tptr(pl, d.in1), (int)b.dims[4], 0, tptr(pl, d.out), (int)ot.dims[4], (int)a.dims[4], (int)b.dims[4], npos, 0);
    }
    case S3_OP_ADD:
      if (o.fused_away) return S3_OK;   // absorbed by the conv in front of it (OpRec::res2_src)
      if (ot.dtype) return launch_add16(ctx, tptr(pl, d.in0), tptr(pl, d.in1), tptr(pl, d.out), ot.numel);
      return launch_add(ctx, tptr(pl, d.in0), tptr(pl, d.in1), tptr(pl, d.out), ot.numel, (int)ot.dims[4], d.bcast_c);
    case S3_OP_ACT:
      return launch_act(ctx, tptr(pl, d.in0), tptr(pl, d.out), ot.numel, d.act, d.alpha);
    case S3_OP_VIEW:
      return S3_OK;
  }
  S3_FAIL(ctx, S3_EINVAL, "forward: unknown op");
}

static int bind_inputs(s3_plan* pl, const void* const* inputs) {
  for (size_t i = 0; i < pl->inputs.size(); ++i) {
    if (!inputs || !inputs[i]) S3_FAIL(pl->ctx, S3_EINVAL, "forward: null input pointer");
    pl->t[pl->inputs[i]].ptr = (float*)inputs[i];
  }
  return S3_OK;
}

// the op list of one forward on ctx->stream (with optional per-op events)
static int forward_ops(s3_plan* pl, hipEvent_t* ev) {
  s3_ctx* ctx = pl->ctx;
  const int n_ops = (int)pl->ops.size();
  {
    int prc = pack_stale(pl, false);
    if (prc) return prc;
  }
  if (ev) S3_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  for (int i = 0; i < n_ops; ++i) {
    int rc = run_op_forward(pl, pl->ops[i]);
    if (rc) {
      // (which launch: a failure inside a stream capture is otherwise anonymous)
      char where[96];
      snprintf(where, sizeof(where), " [forward op %d of %d, kind %d%s]", i, n_ops, pl->ops[i].d.kind,
               ctx->capturing ? ", capturing" : "");
      ctx->err += where;
      return rc;
    }
    if (ev) S3_HIP(ctx, hipEventRecord(ev[i + 1], ctx->stream));
  }
  return S3_OK;
}

// Optional (SUP3R_AMD_GRAPH=1): replay the forward as ONE hipGraph.  The first forwards run eagerly
// (they set kernel attributes, pack filters and size the scratch); the next
// one is captured on a private stream — the context stream may be the legacy
// null stream, which cannot capture — and replayed from then on.
static bool graph_wanted(const s3_plan* pl) {
  if (pl->training || pl->graph_off || pl->in_stage.empty()) return false;
  // opt-in: measured on MI355X / ROCm 7.2 the replay is bit-identical but not
  // faster (C1: 0.524 ms eager vs 0.535 ms replayed — the 36 dependent
  // micro-kernels cost ~14 us each on the GPU side either way)
  return s3_opt_on(S3O_GRAPH);
}

static int forward_graph(s3_plan* pl) {
  s3_ctx* ctx = pl->ctx;
  const uint64_t ver = pl->params->version;
  if (pl->graph_exec && pl->graph_version != ver) {
    graph_drop(pl);               // weights changed: repack eagerly, re-capture
    pl->eager_forwards = 0;
  }
  if (!pl->graph_exec) {
    if (pl->eager_forwards < 1) {
      pl->eager_forwards++;
      return forward_ops(pl, nullptr);
    }
    if (!pl->cap_stream &&
        hipStreamCreateWithFlags(&pl->cap_stream, hipStreamNonBlocking) != hipSuccess) {
      pl->graph_off = true;
      return forward_ops(pl, nullptr);
    }
    // everything queued so far must be visible to the replay
    S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hipStream_t user = ctx->stream;
    ctx->stream = pl->cap_stream;
    hipError_t e = hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal);
    int rc = S3_OK;
    if (e == hipSuccess) {
      rc = forward_ops(pl, nullptr);
      e = hipStreamEndCapture(pl->cap_stream, &pl->graph);
    }
    ctx->stream = user;
    if (e == hipSuccess && rc == S3_OK)
      e = hipGraphInstantiate(&pl->graph_exec, pl->graph, nullptr, nullptr, 0);
    if (s3_opt_has(S3O_TRACE))
      fprintf(stderr, "[graph] capture of %d ops: %s\n", (int)pl->ops.size(),
              (e == hipSuccess && rc == S3_OK) ? "ok" : hipGetErrorString(e));
    if (e != hipSuccess || rc != S3_OK) {
      (void)hipGetLastError();
      graph_drop(pl);
      pl->graph_off = true;       // this plan stays on the eager path
      return forward_ops(pl, nullptr);
    }
    pl->graph_version = ver;
  }
  S3_HIP(ctx, hipGraphLaunch(pl->graph_exec, ctx->stream));
  return S3_OK;
}

extern "C" int s3_plan_forward(s3_plan* pl, const void* const* inputs, void* output) {
  if (!pl) return S3_EINVAL;
  s3_ctx* ctx = pl->ctx;
  S3OptScope opt_scope(&pl->opt);
  const int n_ops = (int)pl->ops.size();
  hipEvent_t* ev = nullptr;
  if (pl->prof_cap > 0 && pl->prof_n < pl->prof_cap)
    ev = pl->prof_ev.data() + (size_t)pl->prof_n * (n_ops + 1);
  int rc;
  if (!ev && pl->fused2d && !s3_opt_has(S3O_NO_FUSED2D)) {
    rc = bind_inputs(pl, inputs);
    if (rc) return rc;
    float* dst = output ? (float*)output : tptr(pl, pl->output);
    rc = fused2d_run(ctx, pl->fused2d, pl->params->buf[S3_BUF_W], pl->params->version,
                     (const float*)inputs[0], dst);
    if (rc) {
      ctx->err += ctx->capturing ? " [fused2d forward, capturing]" : " [fused2d forward]";
      return rc;
    }
    pl->forward_done = true;
    return S3_OK;
  }
  if (!ev && graph_wanted(pl)) {
    for (size_t i = 0; i < pl->inputs.size(); ++i) {
      if (!inputs || !inputs[i]) S3_FAIL(ctx, S3_EINVAL, "forward: null input pointer");
      S3_HIP(ctx, hipMemcpyAsync(pl->in_stage[i], inputs[i],
                                 (size_t)pl->t[pl->inputs[i]].numel * sizeof(float),
                                 hipMemcpyDeviceToDevice, ctx->stream));
      pl->t[pl->inputs[i]].ptr = pl->in_stage[i];
    }
    rc = forward_graph(pl);
  } else {
    rc = bind_inputs(pl, inputs);
    if (rc) return rc;
    // Inference plans write the caller's buffer directly: the output tensor is
    // the last thing written and nothing of the plan reads it afterwards, so
    // the device-to-device copy below (472 MB per C2 forward of 32 chunks,
    // 966 MB per C3 batch of 16: ~1 % of the step) is not needed.  Training
    // plans keep their own copy (the backward pass reads it).
    // (the output may be a view — a reshape — of the tensor the last op writes)
    TensorRec& ot = pl->t[root_of(pl, pl->output)];
    const bool direct = output && !pl->training && ot.buffer >= 0 && ot.dtype == 0 && !ot.is_input &&
                        ot.numel == pl->t[pl->output].numel && !s3_opt_has(S3O_NO_DIRECT_OUTPUT);
    if (pl->win_op >= 0 && !direct) S3_FAIL(ctx, S3_ESTATE, "forward_window: the output cannot be written in place");
    if (direct) ot.ptr = (float*)output;
    rc = forward_ops(pl, ev);
    if (direct) {
      ot.ptr = (float*)pl->buffers[ot.buffer];
      if (rc) return rc;
      if (ev) pl->prof_n++;
      pl->forward_done = true;
      return S3_OK;
    }
  }
  if (rc) return rc;
  if (ev) pl->prof_n++;
  if (output) {
    S3_HIP(ctx, hipMemcpyAsync(output, tptr(pl, pl->output),
                               (size_t)pl->t[pl->output].numel * sizeof(float),
                               hipMemcpyDeviceToDevice, ctx->stream));
  }
  pl->forward_done = true;
  return S3_OK;
}

static void prof_free(s3_plan* pl) {
  for (auto& e : pl->prof_ev) (void)hipEventDestroy(e);
  pl->prof_ev.clear();
  pl->prof_cap = 0;
  pl->prof_n = 0;
}

extern "C" int s3_plan_profile_begin(s3_plan* pl, int max_forwards) {
  if (!pl || max_forwards < 1) return S3_EINVAL;
  s3_ctx* ctx = pl->ctx;
  prof_free(pl);
  const size_t n = (size_t)max_forwards * (pl->ops.size() + 1);
  pl->prof_ev.resize(n);
  for (auto& e : pl->prof_ev) S3_HIP(ctx, hipEventCreate(&e));
  pl->prof_cap = max_forwards;
  return S3_OK;
}

extern "C" int s3_plan_profile_end(s3_plan* pl, float* ms_per_op, int cap) {
  if (!pl || !ms_per_op) return S3_EINVAL;
  s3_ctx* ctx = pl->ctx;
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n_ops = (int)pl->ops.size();
  const int nf = pl->prof_n;
  for (int i = 0; i < n_ops && i < cap; ++i) {
    double acc = 0.0;
    for (int f = 0; f < nf; ++f) {
      hipEvent_t* ev = pl->prof_ev.data() + (size_t)f * (n_ops + 1);
      float ms = 0.f;
      S3_HIP(ctx, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      acc += ms;
    }
    ms_per_op[i] = nf ? (float)(acc / nf) : 0.f;
  }
  prof_free(pl);
  return nf;
}

// ---- windowed forward: the C3 executor's halo crop + un-normalisation inside
// the tail conv.  The last conv of the plan computes only the window
// [lo, lo + n) of its output positions — the chunk without its halo — applies
// y * scale + shift and writes the (N, n0, n1, n2, C) result densely into the
// caller's buffer: no full-size model output, no epilogue pass over it, and the
// tail conv skips the halo positions (24 % of them at 110 x 110 x 624 ->
// 100 x 100 x 576).  Only for plans whose last op is the bf16-input MFMA tail.
static int window_op(const s3_plan* pl) {
  if (pl->training || pl->ops.empty()) return -1;
  if (pl->fused2d && !s3_opt_has(S3O_NO_FUSED2D)) return -1;
  if (s3_opt_on(S3O_GRAPH) || s3_opt_has(S3O_NO_DIRECT_OUTPUT) || s3_opt_has(S3O_NO_TAIL_WINDOW)) return -1;
  int i = (int)pl->ops.size() - 1;
  while (i >= 0 && pl->ops[i].d.kind == S3_OP_VIEW) --i;
  if (i < 0) return -1;
  const OpRec& o = pl->ops[i];
  if (o.d.kind != S3_OP_CONV || o.d.res >= 0 || o.cg.d2s != 1 || !o.io.in_bf16 || o.io.out_bf16) return -1;
  if (o.fwd != Fwd::TAIL_MFMA) return -1;
  const int ro = root_of(pl, o.d.out);
  if (ro != root_of(pl, pl->output)) return -1;
  const TensorRec& ot = pl->t[ro];
  if (ot.buffer < 0 || ot.dtype != 0 || ot.is_input || ot.numel != pl->t[pl->output].numel) return -1;
  // nobody else writes or reads the output tensor
  for (int k = 0; k < (int)pl->ops.size(); ++k) {
    if (k == i) continue;
    const s3_op_desc& d = pl->ops[k].d;
    if (d.kind == S3_OP_VIEW) continue;
    for (int id : {d.in0, d.in1, d.res, d.out})
      if (id >= 0 && root_of(pl, id) == ro) return -1;
  }
  return i;
}

extern "C" int s3_plan_supports_window(const s3_plan* pl) {
  if (!pl) return 0;
  S3OptScope opt_scope(&pl->opt);
  return window_op(pl) >= 0 ? 1 : 0;
}

extern "C" int s3_plan_forward_window(s3_plan* pl, const void* const* inputs, void* output, const int64_t* lo3,
                                      const int64_t* n3, const float* affine_dev, int n_c) {
  if (!pl || !output || !lo3 || !n3) return S3_EINVAL;
  s3_ctx* ctx = pl->ctx;
  int wi;
  {
    S3OptScope opt_scope(&pl->opt);
    wi = window_op(pl);
  }
  if (wi < 0) S3_FAIL(ctx, S3_EINVAL, "forward_window: the plan's last op is not the MFMA tail conv of an inference plan");
  const OpRec& o = pl->ops[wi];
  if (affine_dev && n_c != o.cg.Cout) S3_FAIL(ctx, S3_EINVAL, "forward_window: affine channel count");
  ConvGeom g = o.cg;
  for (int d = 0; d < 3; ++d) {
    if (lo3[d] < 0 || n3[d] < 1 || lo3[d] + n3[d] > o.cg.O[d]) S3_FAIL(ctx, S3_EINVAL, "forward_window: window outside the output");
    g.O[d] = (int)n3[d];
    g.lo[d] = o.cg.lo[d] - (int)lo3[d] * o.cg.s[d];
  }
  pl->win_op = wi;
  pl->win_geom = g;
  pl->win_aff = affine_dev;
  const int rc = s3_plan_forward(pl, inputs, output);
  pl->win_op = -1;
  pl->win_aff = nullptr;
  return rc;
}
