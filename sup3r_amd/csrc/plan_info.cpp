// Read-only queries on a plan: its tensors, its size and what was selected for
// each op, in the public S3_FWD_* / S3_WGRAD_* / S3_DGRAD_* values.
#include "plan_internal.h"

extern "C" void* s3_plan_tensor(s3_plan* pl, int32_t id) {
  if (!pl || id < 0 || id >= (int)pl->t.size()) return nullptr;
  return pl->t[root_of(pl, id)].ptr;
}

extern "C" int64_t s3_plan_workspace_bytes(const s3_plan* pl) {
  return pl ? (int64_t)pl->total_bytes : 0;
}

extern "C" int s3_plan_op_is_mfma(const s3_plan* pl, int i) {
  if (!pl || i < 0 || i >= (int)pl->ops.size()) return 0;
  S3OptScope opt_scope(&pl->opt);
  const auto& o = pl->ops[i];
  if (o.d.kind != S3_OP_CONV || !fwd_is_mfma(o.fwd)) return 0;
  return o.fwd == Fwd::MFMA_PERSIST || o.fwd == Fwd::MFMA_PERSIST2 ? 2 : 1;
}

extern "C" int s3_plan_tensor_dtype(const s3_plan* pl, int32_t id) {
  if (!pl || id < 0 || id >= (int)pl->t.size()) return S3_EINVAL;
  int r = id;
  while (pl->t[r].alias_root >= 0) r = pl->t[r].alias_root;
  // the whole-network kernel keeps every intermediate tensor in LDS as bf16
  if (pl->fused2d && !s3_opt_has(S3O_NO_FUSED2D)) {
    int out_r = pl->output;
    while (pl->t[out_r].alias_root >= 0) out_r = pl->t[out_r].alias_root;
    return (pl->t[r].is_input || r == out_r) ? 0 : 1;
  }
  return pl->t[r].dtype;
}

extern "C" int64_t s3_plan_tensor_read(s3_plan* pl, int32_t id, void* host, size_t cap) {
  if (!pl || !host || id < 0 || id >= (int)pl->t.size()) return S3_EINVAL;
  s3_ctx* ctx = pl->ctx;
  const TensorRec& t = pl->t[root_of(pl, id)];
  if (!t.ptr) S3_FAIL(ctx, S3_ESTATE, "tensor_read: tensor has no buffer yet");
  const size_t bytes = (size_t)pl->t[id].numel * (t.dtype ? 2 : 4);
  if (bytes > cap) S3_FAIL(ctx, S3_EINVAL, "tensor_read: host buffer too small");
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  S3_HIP(ctx, hipMemcpy(host, t.ptr, bytes, hipMemcpyDeviceToHost));
  return (int64_t)bytes;
}

// the public S3_FWD_* / S3_WGRAD_* / S3_DGRAD_* value of a stored choice
static int fwd_public(const OpRec& o) {
  switch (o.fwd) {
    case Fwd::MFMA_TILE: return S3_FWD_MFMA_TILE;
    case Fwd::MFMA_PERSIST: case Fwd::MFMA_PERSIST2: return S3_FWD_MFMA_PERSIST;
    case Fwd::MFMA_GEN: return S3_FWD_MFMA_GEN;
    case Fwd::CONV2D_WS: case Fwd::CONV2D_WS_X3: case Fwd::CONV2D_OUT: return S3_FWD_CONV2D_WS;
    case Fwd::CONV2D_HEAD: return S3_FWD_CONV2D_HEAD;
    case Fwd::FEWPOS_MFMA: case Fwd::FEWPOS: return S3_FWD_FEWPOS;
    case Fwd::GCONV: return o.cg.Cin <= 4 ? S3_FWD_GCONV_FEWCH : S3_FWD_GCONV;
    case Fwd::HALO32: return S3_FWD_HALO32;
    case Fwd::HALO_S2: return S3_FWD_HALO_S2;
    case Fwd::TAIL_X3: case Fwd::TAIL_MFMA: return S3_FWD_TAIL_MFMA;
    case Fwd::SMALL: return S3_FWD_SMALL;
    case Fwd::DIRECT: case Fwd::NONE: break;
  }
  return S3_FWD_DIRECT;
}

static int wgrad_public(Wgrad w) {
  switch (w) {
    case Wgrad::FEWPOS_MFMA: case Wgrad::FEWPOS: return S3_WGRAD_FEWPOS;
    case Wgrad::TAIL: return S3_WGRAD_TAIL;
    case Wgrad::C2: return S3_WGRAD_C2;
    case Wgrad::BF16_TRUNK: return S3_WGRAD_BF16_TRUNK;
    case Wgrad::F32_TRUNK: return S3_WGRAD_F32_TRUNK;
    case Wgrad::BF16_GEN: return S3_WGRAD_BF16_GEN;
    case Wgrad::BF16_2D: return S3_WGRAD_BF16_2D;
    case Wgrad::F32_GEN: return S3_WGRAD_F32_GEN;
    case Wgrad::DIRECT: break;
  }
  return S3_WGRAD_DIRECT;
}

static int dgrad_public(Dgrad d) {
  switch (d) {
    case Dgrad::MFMA_FRAME: case Dgrad::GEN: return S3_DGRAD_MFMA_FRAME;
    case Dgrad::MFMA_VALID: return S3_DGRAD_MFMA_VALID;
    case Dgrad::FEWCH: return S3_DGRAD_FEWCH_FRAME;
    case Dgrad::CHUNKED_FRAME: case Dgrad::CHUNKED_VALID: return S3_DGRAD_MFMA_CHUNKED;
    case Dgrad::C2: case Dgrad::C2_X3: return S3_DGRAD_C2;
    case Dgrad::S2: case Dgrad::S2_X3: return S3_DGRAD_S2;
    case Dgrad::GCONV: return S3_DGRAD_GCONV;
    case Dgrad::FEWPOS_MFMA: case Dgrad::FEWPOS: return S3_DGRAD_FEWPOS;
    case Dgrad::DIRECT: break;
  }
  return S3_DGRAD_DIRECT;
}

extern "C" int s3_plan_op_info(const s3_plan* pl, int i, int32_t* out, int cap) {
  if (!pl || !out || i < 0 || i >= (int)pl->ops.size()) return S3_EINVAL;
  S3OptScope opt_scope(&pl->opt);   // the launch-time kernel switches are the PLAN's options
  const OpRec& o = pl->ops[i];
  int32_t v[S3_OPINFO_COUNT] = {0};
  v[S3_OPINFO_KIND] = o.d.kind;
  if (o.d.kind == S3_OP_CONV) {
    int fwd = fwd_public(o);
    const bool fused = pl->fused2d && !pl->training && !s3_opt_has(S3O_NO_FUSED2D);
    if (fused) fwd = S3_FWD_FUSED2D;
    v[S3_OPINFO_FWD] = fwd;
    v[S3_OPINFO_IN16] = o.io.in_bf16; v[S3_OPINFO_OUT16] = o.io.out_bf16; v[S3_OPINFO_RES16] = o.io.res_bf16;
    v[S3_OPINFO_IN_REP] = o.cg.in_rep;
    v[S3_OPINFO_RES_REP] = o.cg.res_rep;
    // operands rounded to bf16 by the forward kernel
    v[S3_OPINFO_FWD_BF16_OPS] = (pl->precision == S3_PREC_BF16 &&
                                 (fwd == S3_FWD_FUSED2D || fwd == S3_FWD_MFMA_TILE || fwd == S3_FWD_MFMA_GEN || fwd == S3_FWD_CONV2D_WS || fwd == S3_FWD_CONV2D_HEAD || fwd == S3_FWD_MFMA_PERSIST || fwd == S3_FWD_HALO32 || fwd == S3_FWD_HALO_S2 ||
                                  fwd == S3_FWD_GCONV || fwd == S3_FWD_GCONV_FEWCH || fwd == S3_FWD_TAIL_MFMA)) ? 1 : 0;
    v[S3_OPINFO_FEWPOS_MFMA] = (o.fam == Fam::FEWPOS_MFMA || o.wgrad == Wgrad::FEWPOS_MFMA) ? 1 : 0;
    if (pl->training) {
      v[S3_OPINFO_WGRAD] = wgrad_public(o.wgrad);
      v[S3_OPINFO_DGRAD] = dgrad_public(o.dgrad);
      v[S3_OPINFO_DGRAD_FRAME16] = o.dgrad_frame16 ? 1 : 0;
      v[S3_OPINFO_MASK_FUSED_FROM] = o.mask_prod;
    }
  }
  if (o.d.kind == S3_OP_REPEAT_T || o.d.kind == S3_OP_CONCAT || o.d.kind == S3_OP_ADD)
    v[S3_OPINFO_IN_REP] = o.fused_away ? 1 : 0;
  for (int q = 0; q < cap && q < S3_OPINFO_COUNT; ++q) out[q] = v[q];
  return S3_OPINFO_COUNT;
}
