// What the host files of the plan executor share (context.cpp, params.cpp,
// plan.cpp, plan_forward.cpp, plan_info.cpp, plan_backward.cpp, comm.cpp): the
// parameter store, the records of a plan and the accessors the per-op code
// calls.  Every type here is defined here only; what one file uses stays in
// that file.  Nothing in it is exported (tests/test_abi.py).
#pragma once
#include "common.h"

struct Param {
  int64_t offset, size;
};

struct s3_params {
  s3_ctx* ctx = nullptr;
  std::vector<Param> p;
  int64_t total = 0;
  float* buf[4] = {nullptr, nullptr, nullptr, nullptr};  // W, G, M, V
  uint64_t version = 1;  // bumped whenever W changes (re-pack trigger)
  // bucketed gradient all-reduce under the backward pass (s3_params_arm_allreduce):
  // [0, reduce_end) of the gradient buffer is not yet handed to RCCL
  bool armed = false;     // the next backward pass that writes G reduces it as it goes
  bool reduced = false;   // ... and has done so: s3_params_allreduce_grads only joins
  int64_t reduce_end = 0, bucket_elems = 0;
  int buckets_issued = 0;
  float* hyper_dev = nullptr;   // the optimizer step's scalars, staged (s3_optimizer_stage)
};

struct TensorRec {
  int64_t dims[5];
  int64_t numel = 0;
  int buffer = -1;      // arena buffer id (-1: external input)
  int alias_root = -1;  // tensor id this one aliases (VIEW)
  float* ptr = nullptr;
  float* gptr = nullptr;  // gradient buffer (training plans)
  bool is_input = false;
  int dtype = 0;        // 0 = fp32, 1 = bf16 (inference plans, bf16 mode)
  size_t bytes() const { return (size_t)numel * (dtype ? 2 : 4); }
};

// ---- the kernels of a conv, chosen once per plan.  select_conv picks the
// forward family and both gradient kernels before the dtypes are known, with
// one precedence for each; resolve_fwd makes the forward concrete once they
// are.  Every later pass, the dispatch and the reports read these choices.
enum class Fam : uint8_t {
  DIRECT,         // the direct kernels (conv_generic_fwd_variant)
  MFMA,           // halo-tile / persistent / logical-axes / weights-stationary (conv_mfma_fwd_variant)
  FEWPOS_MFMA,    // few positions: the one-launch fp32-MFMA kernels
  FEWPOS,         // few positions: the weight-streaming slab kernels
  GCONV,          // general gather-MFMA conv (strided / valid-padded, C_in % 32 == 0 or C_in <= 4)
  HALO32,         // C_in = 32 stride-1 conv: LDS-halo forward (else as GCONV)
  HALO_S2,        // C_in = 32 stride-2 valid conv: LDS-halo forward, bf16 cells in (else as GCONV)
  TAIL_X3,        // BF16X3 plans: banded split-bf16 MFMA tail (8 -> 2, fp32 in / out)
};
enum class Fwd : uint8_t {
  NONE,
  // the MFMA family, in MfmaFwd order
  MFMA_TILE, MFMA_PERSIST, MFMA_PERSIST2, MFMA_GEN, CONV2D_WS, CONV2D_WS_X3, CONV2D_OUT, CONV2D_HEAD,
  FEWPOS_MFMA, FEWPOS, GCONV, HALO32, HALO_S2, TAIL_X3,
  // the direct family, in GenericFwd order
  TAIL_MFMA, SMALL, DIRECT,
};
static inline Fwd fwd_of(MfmaFwd v) { return (Fwd)((int)Fwd::MFMA_TILE + (int)v); }
static inline Fwd fwd_of(GenericFwd v) { return (Fwd)((int)Fwd::TAIL_MFMA + (int)v); }
static inline bool fwd_is_mfma(Fwd f) { return f >= Fwd::MFMA_TILE && f <= Fwd::CONV2D_HEAD; }
static inline bool fwd_is_generic(Fwd f) { return f >= Fwd::TAIL_MFMA; }
static inline MfmaFwd mfma_of(Fwd f) { return (MfmaFwd)((int)f - (int)Fwd::MFMA_TILE); }
static inline GenericFwd generic_of(Fwd f) { return (GenericFwd)((int)f - (int)Fwd::TAIL_MFMA); }
enum class Wgrad : uint8_t {
  DIRECT,
  FEWPOS_MFMA,    // one-launch fp32-MFMA kernel (fewpos convs, and the rest with few positions)
  FEWPOS,         // slab kernel of the fewpos family
  TAIL, C2,       // few-channel hi-res convs
  BF16_TRUNK, F32_TRUNK,   // 64 -> C_out 'same' 3 x 3 x 3: transpose-read bf16 / fp32 MFMA
  BF16_GEN, BF16_2D, F32_GEN,
};
enum class Dgrad : uint8_t {
  DIRECT,
  MFMA_FRAME,     // conv over the padded frame on the MFMA tile kernels, then the fold
  MFMA_VALID,     // ... of a valid-padded conv: straight onto x's grid
  GEN,            // ... on the logical-axes kernel (2-D nets, few time steps)
  FEWCH,          // C_out <= 4 'same' conv: few-channel gather conv over the frame
  CHUNKED_FRAME, CHUNKED_VALID,   // 64 -> C_out > 64: 64-channel slices of dPre
  C2, C2_X3,      // few-channel hi-res conv: LDS halo (BF16 / BF16X3)
  S2, S2_X3,      // stride-2 valid conv, C_out = 32: residue classes on an LDS halo
  GCONV,          // gather-MFMA adjoint
  FEWPOS_MFMA, FEWPOS,
};
static inline bool dgrad_is_mfma(Dgrad d) { return d >= Dgrad::MFMA_FRAME && d <= Dgrad::CHUNKED_VALID; }
static inline bool dgrad_is_valid(Dgrad d) { return d == Dgrad::MFMA_VALID || d == Dgrad::CHUNKED_VALID; }
static inline bool dgrad_is_chunked(Dgrad d) { return d == Dgrad::CHUNKED_FRAME || d == Dgrad::CHUNKED_VALID; }
static inline bool dgrad_is_c2(Dgrad d) { return d == Dgrad::C2 || d == Dgrad::C2_X3; }
static inline bool dgrad_is_s2(Dgrad d) { return d == Dgrad::S2 || d == Dgrad::S2_X3; }

struct OpRec {
  s3_op_desc d;
  ConvGeom cg;
  GatherGeom gg;
  Fam fam = Fam::DIRECT;
  Fwd fwd = Fwd::NONE;
  Wgrad wgrad = Wgrad::DIRECT;  // (training plans)
  Dgrad dgrad = Dgrad::DIRECT;
  ConvIO io;
  void* packed = nullptr;
  uint64_t packed_version = 0;
  bool dgrad_frame16 = false;  // the persistent kernel writes the padded frame as bf16
  bool use16 = false;          // data gradient stages the bf16 copy of dPre its mask pass leaves behind
  int mask_prod = -1;          // producer conv of in0 whose activation adjoint is fused into this conv's dgrad store / fold
  int in_prod = -1;            // producer conv of in0 (any number of consumers), -1: not a conv
  void* dgc_wbf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  void* h32_w = nullptr;
  uint64_t h32_version = 0;
  void* dc2_w = nullptr;
  int64_t dc2_version = -1;
  ConvGeom dg;                 // geometry of the dgrad-as-conv launch
  int rep_src = -1;            // conv: tensor read through a fused temporal repeat (cg.in_rep)
  int res_src = -1;            // ... and the residual (cg.res_rep)
  int exo_src = -1;            // conv behind a fused-away Sup3rConcat: the exogenous field (cg.w_cin)
  int res2_src = -1;           // conv that absorbed the skip add behind it: the add's other operand (cg.res2)
  void* sign_bytes = nullptr;  // training: activation sign bytes next to the output (conv_dgrad_s2's mask)
  bool fused_away = false;     // repeat op absorbed by its consumer conv: no launch
  float* dg_w32 = nullptr;     // flipped / transposed fp32 filter
  void* dg_wbf = nullptr;      // its bf16 slabs (bf16 mode)
  uint64_t dg_version = 0;
  void* gc_w = nullptr;        // gather-MFMA conv: bf16 [tap][co][ci]
  void* gc_wt = nullptr;       // bf16 [tap][ci][co] (data gradient)
  uint64_t gc_version = 0, gct_version = 0;
  float* fp_wt = nullptr;      // fewpos: [tap][co][ci] transposed filter (dgrad)
  uint64_t fp_version = 0;
  bool fewpos() const { return fam == Fam::FEWPOS_MFMA || fam == Fam::FEWPOS; }
  bool gconv() const { return fam == Fam::GCONV || fam == Fam::HALO32 || fam == Fam::HALO_S2; }
};

// State of one backward pass: where each tensor's gradient is, and which
// tensor the plan's two hand-over buffers (s3_plan::dpre16, s3_plan::bsum)
// currently belong to.  Every change of it goes through a member below.
struct BwdState {
  std::vector<char> gwritten;          // per tensor root: 0 none, 1 in gptr, 2 = one contribution, aliased (gsrc)
  std::vector<const float*> gsrc;      // the aliased first contribution (a finished gradient buffer)
  std::vector<char> premasked;         // tensor gradient already carries its producer's activation adjoint
  int dpre16_for = -1;        // tensor root whose finished gradient = dPre of its producer is in dpre16, -1: none
  bool dpre16_only = false;   // ... and ONLY there (bf16-only fold); false: the fp32 tensor is valid too
  int bsum_for = -1, bsum_nblk = 0;    // tensor root whose channel sums are in bsum (-1: none), slabs
  // the arguments of the pass
  int need_wgrad = 0, accumulate_wgrad = 0;
  int dx_root = -1;           // input tensor whose gradient the caller asked for, -1: none

  void reset(size_t n_tensors) {
    gwritten.assign(n_tensors, 0);
    gsrc.assign(n_tensors, nullptr);
    premasked.assign(n_tensors, 0);
    release_dpre16();
    drop_bsum(bsum_for);
  }
  // a first contribution that lives in another finished buffer is not copied
  void alias(int r, const float* src) { gsrc[r] = src; gwritten[r] = 2; }
  // ... until a second one arrives: whoever adds the two writes gptr
  const float* take_alias(int r) {
    const float* first = gsrc[r];
    gsrc[r] = nullptr;
    gwritten[r] = 1;
    return first;
  }
  // (callers decide with dpre16_free_for() BEFORE the launch that writes it)
  void claim_dpre16(int r, bool only) { dpre16_for = r; dpre16_only = only; }
  void release_dpre16() { dpre16_for = -1; }
  // the conv that produced r picks up what its consumer left in dpre16
  enum Held { NONE, COPY, ONLY };
  Held take_dpre16(int r) {
    if (dpre16_for != r || (dpre16_only && !premasked[r])) return NONE;
    release_dpre16();
    return dpre16_only ? ONLY : COPY;
  }
  void claim_bsum(int r, int nblk) { bsum_for = r; bsum_nblk = nblk; }
  void drop_bsum(int r) { if (bsum_for == r) bsum_for = -1; }
};

struct s3_plan {
  s3_ctx* ctx = nullptr;
  S3Options opt;              // snapshot of the options this plan was created with
  s3_params* params = nullptr;
  std::vector<TensorRec> t;
  std::vector<OpRec> ops;
  std::vector<int32_t> inputs;
  int32_t output = -1;
  int precision = S3_PREC_F32;
  int training = 0;
  // s3_plan_forward_window: op index whose conv runs over win_geom (-1: none) + its affine
  int win_op = -1;
  ConvGeom win_geom;
  const float* win_aff = nullptr;
  std::vector<float*> buffers;
  std::vector<size_t> buffer_bytes;
  std::vector<void*> owned;  // every hipMalloc of this plan
  float* dpre = nullptr;      // conv/dense epilogue-adjoint workspace
  void* dpre16 = nullptr;     // its bf16 copy (mask pass of a conv with use16)
  size_t dpre16_bytes = 0;
  float* gtmp = nullptr;      // gradient staging when a tensor has >1 consumer
  float* wg_partial = nullptr;
  size_t wg_partial_bytes = 0;
  float* dxp = nullptr;       // padded-frame data gradient of the MFMA dgrad
  float* fp_partial = nullptr;   // per-tap partials of the few-positions path
  size_t fp_partial_bytes = 0;
  size_t total_bytes = 0;
  bool forward_done = false;
  std::vector<hipEvent_t> prof_ev;  // prof_cap * (n_ops + 1)
  int prof_cap = 0, prof_n = 0;
  float* bsum = nullptr;               // channel sums left by a frame fold (bias gradient of the producer)
  float* bsum2 = nullptr;              // channel sums left by a conv's own mask pass (consumed at once)
  BwdState bw;                         // what one backward pass knows about the tensors' gradients
  // hipGraph replay of the forward op list (inference plans): inputs are
  // copied into plan-owned staging buffers so every pointer inside the
  // captured graph is fixed; re-captured when the weights change
  std::vector<float*> in_stage;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  hipStream_t cap_stream = nullptr;
  uint64_t graph_version = 0;
  int eager_forwards = 0;
  bool graph_off = false;
  Fused2dPlan* fused2d = nullptr;   // whole-network kernel (small 2-D inference plans)
  // batched filter re-pack (bf16 plans): job tables on the device, built once
  S3PackJob* pack_fwd = nullptr;
  S3PackJob* pack_bwd = nullptr;
  std::vector<int> pack_fwd_ops, pack_bwd_ops;
  int pack_fwd_ct = 1, pack_bwd_ct = 1;
  bool pack_built = false;
};

// ---- the functions that cross files
int apply_options(s3_ctx* ctx, S3Options& o, const s3_plan_options* opt);   // context.cpp
int plan_alloc(s3_plan* pl, void** out, size_t bytes);                      // plan.cpp
void graph_drop(s3_plan* pl);                                               // plan.cpp
int pack_stale(s3_plan* pl, bool bwd);                                      // plan_forward.cpp

// ---- accessors of the per-op code (inline: a step is a chain of ~5 us launches)

static inline int root_of(const s3_plan* pl, int t) {
  while (pl->t[t].alias_root >= 0) t = pl->t[t].alias_root;
  return t;
}

static inline float* tptr(s3_plan* pl, int id) { return pl->t[root_of(pl, id)].ptr; }
static inline int tdtype(s3_plan* pl, int id) { return pl->t[root_of(pl, id)].dtype; }
static inline float* gptr(s3_plan* pl, int id) { return pl->t[root_of(pl, id)].gptr; }
// parameter `id` in the weight / the gradient buffer of the store (nullptr: the op has none)
static inline float* wptr(const s3_plan* pl, int id) {
  return id < 0 ? nullptr : pl->params->buf[S3_BUF_W] + pl->params->p[id].offset;
}
static inline float* gparam(const s3_plan* pl, int id) {
  return id < 0 ? nullptr : pl->params->buf[S3_BUF_G] + pl->params->p[id].offset;
}
// a filter image packed from the weights as of version `have`: packed again
// when the store has moved on (the version is set only once the launch is out)
template <class V, class Launch>
static inline int repack_if_stale(V& have, uint64_t want, Launch&& launch) {
  if (have == (V)want) return S3_OK;
  const int rc = launch();
  if (rc == S3_OK) have = (V)want;
  return rc;
}
