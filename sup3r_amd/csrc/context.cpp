// The option table, the context (stream, device limits, counters, last error)
// and the whole-step stream capture of libsup3r_hip.so.
#include <cstdlib>
#include <cstring>

#include "plan_internal.h"

// ------------------------------------------------------------------ options
thread_local const S3Options* s3_active_options = nullptr;

static const char* const kOptionNames[S3O_COUNT] = {
#define X(n) #n,
    S3_OPTION_LIST(X)
#undef X
};

const char* s3_option_name(int id) { return (id >= 0 && id < S3O_COUNT) ? kOptionNames[id] : nullptr; }

int s3_option_id(const char* name) {
  if (!name) return -1;
  if (!strncmp(name, "SUP3R_AMD_", 10)) name += 10;
  for (int i = 0; i < S3O_COUNT; ++i)
    if (!strcmp(name, kOptionNames[i])) return i;
  return -1;
}

// initial defaults of a context: the SUP3R_AMD_<NAME> variables as they are
// when the context is created (never read again afterwards)
static void options_from_env(S3Options& o) {
  for (int i = 0; i < S3O_COUNT; ++i) {
    const std::string var = std::string("SUP3R_AMD_") + kOptionNames[i];
    const char* v = getenv(var.c_str());
    if (v) { o.has[i] = true; o.v[i] = (int32_t)atoll(v); }
  }
}

int apply_options(s3_ctx* ctx, S3Options& o, const s3_plan_options* opt) {
  if (!opt) return S3_OK;
  for (int i = 0; i < opt->n; ++i) {
    const int id = s3_option_id(opt->names ? opt->names[i] : nullptr);
    if (id < 0) S3_FAIL(ctx, S3_EINVAL, std::string("unknown option \"") + (opt->names && opt->names[i] ? opt->names[i] : "(null)") + "\"");
    if (opt->values[i] == S3_OPTION_UNSET) { o.has[id] = false; o.v[id] = 0; }
    else { o.has[id] = true; o.v[id] = opt->values[i]; }
  }
  return S3_OK;
}

extern "C" int s3_ctx_set_option(s3_ctx* ctx, const char* name, int32_t value) {
  if (!ctx) return S3_EINVAL;
  const char* names[1] = {name};
  const int32_t values[1] = {value};
  s3_plan_options o = {1, names, values};
  return apply_options(ctx, ctx->opt, &o);
}

extern "C" int s3_ctx_get_option(const s3_ctx* ctx, const char* name, int32_t* value) {
  if (!ctx) return S3_EINVAL;
  const int id = s3_option_id(name);
  if (id < 0) return S3_EINVAL;
  if (value) *value = ctx->opt.v[id];
  return ctx->opt.has[id] ? 1 : 0;
}

extern "C" const char* s3_option_name_at(int index) { return s3_option_name(index); }

// ------------------------------------------------------------------ context
extern "C" int s3_ctx_create(int device_id, void* stream, int create_stream,
                             s3_ctx** out) {
  if (!out) return S3_EINVAL;
  s3_ctx* ctx = new s3_ctx();
  ctx->device = device_id;
  options_from_env(ctx->opt);
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) {
    // keep the object so the caller can read the message
    ctx->err = std::string("hipSetDevice: ") + hipGetErrorString(e);
    *out = ctx;
    return S3_EHIP;
  }
  if (!create_stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      ctx->err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
      *out = ctx;
      return S3_EHIP;
    }
    ctx->own_stream = true;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
    ctx->num_cu = prop.multiProcessorCount;
    ctx->lds_max = prop.sharedMemPerBlock;
    // The library is compiled for gfx950 only and its persistent kernels are sized
    // for that part's 160 KB of LDS per workgroup (up to 163,072 B): say so here,
    // once, instead of failing at some kernel's first launch on anything else.
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      ctx->err = std::string("sup3r_amd is built for gfx950 (MI355X) only; device ") + std::to_string(device_id) +
                 " is " + prop.gcnArchName;
      *out = ctx;
      return S3_ESTATE;
    }
  }
  *out = ctx;
  return S3_OK;
}

extern "C" void s3_ctx_destroy(s3_ctx* ctx) {
  if (!ctx) return;
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  for (void* p : ctx->retired) (void)hipFree(p);   // scratch blocks outgrown while a graph held them
  ctx->retired.clear();
  if (ctx->capturing) (void)s3_capture_abort(ctx);
  if (ctx->cap_stream) (void)hipStreamDestroy(ctx->cap_stream);
  if (ctx->wg_stream) (void)hipStreamDestroy(ctx->wg_stream);
  for (int k = 0; k < 2; ++k)
    if (ctx->wg_ev[k]) (void)hipEventDestroy(ctx->wg_ev[k]);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" int64_t s3_ctx_stat(const s3_ctx* ctx, int which) {
  if (!ctx || which < 0 || which >= S3_STAT_COUNT) return -1;
  return ctx->stat[which];
}

extern "C" const char* s3_last_error(const s3_ctx* ctx) {
  return ctx ? ctx->err.c_str() : "null context";
}

extern "C" int s3_ctx_sync(s3_ctx* ctx) {
  if (!ctx) return S3_EINVAL;
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return S3_OK;
}

extern "C" void* s3_ctx_stream(s3_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" const char* s3_version(void) { return "sup3r_hip 0.1 (gfx950)"; }

// ------------------------------------------------------------ stream capture
// A launch-bound step (the C1 training step is ~650 launches of a few
// microseconds each) recorded once and replayed as ONE hipGraphLaunch.  Between
// begin and end every launch of this context goes to a non-blocking side
// stream that records instead of executing; what is recorded must be the same
// every step: static pointers (the caller keeps every buffer of the step
// alive), no host read-back, no collective, step-dependent scalars staged
// (s3_optimizer_stage).  A call that cannot be captured fails the capture; the
// caller then runs eagerly.
struct s3_graph {
  s3_ctx* ctx = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  size_t n_nodes = 0;
};

extern "C" int s3_capture_begin(s3_ctx* ctx) {
  if (!ctx) return S3_EINVAL;
  if (ctx->capturing) S3_FAIL(ctx, S3_EINVAL, "capture_begin: already capturing");
  if (ctx->comm) S3_FAIL(ctx, S3_EINVAL, "capture_begin: not with a communicator (collectives are not captured)");
  if (!ctx->cap_stream) S3_HIP(ctx, hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking));
  // what was enqueued so far runs before anything the capture stream does later
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  hipError_t be = hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeRelaxed);
  if (be != hipSuccess) {
    // a capture stream left in a broken state by an earlier, failed recording
    // must not poison every later one: drop it and try once on a fresh stream
    (void)hipGetLastError();
    (void)hipStreamDestroy(ctx->cap_stream);
    ctx->cap_stream = nullptr;
    S3_HIP(ctx, hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking));
    S3_HIP(ctx, hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeRelaxed));
  }
  ctx->saved_stream = ctx->stream;
  ctx->stream = ctx->cap_stream;
  ctx->capturing = true;
  return S3_OK;
}

static int capture_stop(s3_ctx* ctx, hipGraph_t* g) {
  hipError_t e = hipStreamEndCapture(ctx->cap_stream, g);
  ctx->stream = ctx->saved_stream;
  ctx->capturing = false;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
    // (the next recording starts on a fresh stream)
    if (ctx->cap_stream) { (void)hipStreamDestroy(ctx->cap_stream); ctx->cap_stream = nullptr; }
    (void)hipGetLastError();
    return S3_EHIP;
  }
  return S3_OK;
}

extern "C" int s3_capture_abort(s3_ctx* ctx) {
  if (!ctx) return S3_EINVAL;
  if (!ctx->capturing) return S3_OK;
  hipGraph_t g = nullptr;
  const std::string keep = ctx->err;
  (void)capture_stop(ctx, &g);
  if (g) (void)hipGraphDestroy(g);
  ctx->err = keep;
  return S3_OK;
}

extern "C" int s3_capture_end(s3_ctx* ctx, s3_graph** out) {
  if (!ctx || !out) return S3_EINVAL;
  if (!ctx->capturing) S3_FAIL(ctx, S3_EINVAL, "capture_end: not capturing");
  hipGraph_t g = nullptr;
  int rc = capture_stop(ctx, &g);
  if (rc) return rc;
  if (!g) S3_FAIL(ctx, S3_EHIP, "capture_end: empty graph");
  s3_graph* G = new s3_graph();
  G->ctx = ctx;
  G->graph = g;
  hipError_t e = hipGraphInstantiate(&G->exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g);
    delete G;
    ctx->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
    return S3_EHIP;
  }
  (void)hipGraphGetNodes(g, nullptr, &G->n_nodes);
  ctx->graphs_made = true;
  *out = G;
  return S3_OK;
}

extern "C" int s3_graph_launch(s3_graph* g) {
  if (!g || !g->exec) return S3_EINVAL;
  s3_ctx* ctx = g->ctx;
  if (ctx->capturing) S3_FAIL(ctx, S3_EINVAL, "graph_launch: inside a capture");
  S3_HIP(ctx, hipGraphLaunch(g->exec, ctx->stream));
  return S3_OK;
}

extern "C" int64_t s3_graph_nodes(const s3_graph* g) { return g ? (int64_t)g->n_nodes : -1; }

extern "C" void s3_graph_destroy(s3_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
}
