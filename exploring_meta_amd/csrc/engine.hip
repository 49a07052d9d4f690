// Engine: orchestrates one whole meta-batch (all tasks, all inner steps, query pass, second-order adjoint recursion) as
// a fixed sequence of batched-over-tasks kernel launches on the caller's stream, and exports the C ABI (include/mi_maml.h).
//
// Algorithm (per task t, identical to the reference's clone -> fast_adapt -> eval_loss.backward()):
//   theta_0 = theta;  for k < K:  g_k = grad L_support(theta_k);  theta_{k+1} = theta_k - alpha g_k      (l2l MAML.adapt)
//   lam = grad L_query(theta_K);   second order:  for k = K-1..0:  lam <- lam - alpha * H_support(theta_k) lam
//   meta_grad = sum_t lam_t.        H v is a forward-over-reverse tangent sweep over the SAVED step-k activations.
#include <array>
#include <string>
#include <vector>
#include <cstdio>
#include <cmath>
#include <cstring>
#include "mi_common.h"
#include "kernels.h"
#include "../../include/mi_maml.h"

#define EPI_NONE 0
#define EPI_STATS 1
#define EPI_TSTATS 2
#define EPI_BRED 3

static thread_local std::string g_err;

struct Layer {
  int ci, co, h, w, ho, wo, stride, pool, hp, wp;
  size_t off_gamma, off_beta, off_w, off_b;
};

typedef std::array<unsigned long long, 38> GraphKey;   // graph_key(): what a captured fused call depends on
struct mi_engine {
  mi_model_desc d;
  int device;
  std::vector<Layer> L;
  int head_c, head_hw, feat;
  size_t off_wl, off_bl, P;
  size_t PS;  // per-task stride of parameter-shaped buffers (P padded so every task's vectors stay 16-B aligned)
  int32_t* perm_dev;
  bool fuse1 = false;   // block 1 runs through the conv-recompute kernels of block1.hip
  bool gram1 = true;    // ... with the statistics of repeated passes from the input Gram matrix (gram.hip) and the BN-backward
                        // reductions from zhat stored at the pooling argmax, instead of further conv-recompute passes
  // ... and a Gram matrix of the QUERY images too (the query pass's statistics as quadratic forms, its weight gradient as sparse part +
  // assembly, instead of the two conv-recompute kernels): its fp64 launch runs on the side stream beside the inner loop, or once on the
  // caller's stream without one (profiles/r6/ab_gram_query.txt)
  bool gramq = true;
  // Weight gradients of blocks >= 2 run on a side stream: they depend only on dz_l and the block input, nothing downstream of
  // them until the parameter update, and they are matrix-bound while the BatchNorm kernels of the next block are HBM-bound.
  bool overlap = true;
  // BatchNorm statistic / reduction partials are folded by the last workgroup of the producing kernel (finalize.h) instead of a
  // bn_finalize launch; counters: one zero-initialised arrival counter per task, owned by the engine.
  bool fuse_fin = true;
  // block 1's BatchNorm-backward sums (dgamma, dbeta and their tangents) ride in the epilogue of block 2's dgrad instead of a
  // streaming pooled_reduce pass over p, zhat, dp (needs the fused block 1 with stored zhat and a stride-1 hidden block 2)
  bool fuse_b1red = true;
  // the tail of every pass of mi_meta_batch_maml as ONE launch (gram.hip, advance_kernel): weight-gradient partial folds, block 1's
  // Gram-matrix assembly, the fast-weight / adjoint update and the next pass's Gram statistics -- instead of 3 reduce_partials +
  // gram_wgrad + axpy + gram_stats launches and a memset per pass.  Same arithmetic in the same order: bit-identical results.
  bool fuse_tail = true;
  // the last ConvBlock's BatchNorm + pooling, the head, its backward and that block's BatchNorm-backward sums as ONE launch, four workgroups per
  // task (tail.hip), instead of four launches per pass (MI_FUSE_LAST=0 / mi_engine_set_fused_last_block(e, 0): the separate launches)
  bool fuse_last = !(getenv("MI_FUSE_LAST") && atoi(getenv("MI_FUSE_LAST")) == 0);
  unsigned long long* tail_stamps = nullptr;   // debug (mi_debug_tail_stamps)
  unsigned zoff[10] = {}, zlen[10] = {};   // conv-bias segments and the padding P..PS of a parameter-shaped vector (never written by a kernel)
  int nzero = 0;
  unsigned* counters = nullptr;
  static constexpr int kMaxCounterTasks = 65536;
  struct SideCtx { hipStream_t side = nullptr; hipEvent_t fork = nullptr, join = nullptr; } sc[1];
  std::string err;
  // Graph replay (mi_engine_set_graph): the launch sequence of mi_meta_batch_maml / _anil is a pure function of its arguments, so a
  // call whose arguments (every pointer, size and scalar) equal an earlier call's is replayed as one hipGraphLaunch -- what the
  // launch-bound few-image configurations need (cfg1: 75 launches in 0.6 ms).  First sight of a signature runs eagerly (kernel
  // attributes, lazily created streams), the second is captured, later ones replay.
  bool graph_on = false;
  struct GraphEntry { GraphKey key; hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; int seen = 0; };
  std::vector<GraphEntry> graphs;
  // BatchNorm batch statistics of every forward pass (mi_engine_set_bn_export): what torch.nn.BatchNorm2d's running_mean / running_var
  // update consumes.  Layout [pass][T][2][sum of channels over the blocks]: batch mean, biased batch variance.
  float* bn_export = nullptr;
  size_t bn_export_floats = 0;
  int export_pass = 0;
  // debug trace (mi_debug_set_trace): per-step theta_k / g_k / lam fed to the k-th Hessian-vector product / H lam, reference order
  float* trace = nullptr;
  size_t trace_floats = 0;
  // optional per-launch HIP-event profiling (bench.py's roofline leg): kind = op*8 + layer
  int prof_on = 0, prof_filter = -1;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<int> ev_kind;
  size_t ev_used = 0;
};

enum ProfOp { OP_CONV_FWD = 0, OP_BN_FINALIZE, OP_BN_FWD, OP_HEAD, OP_BN_BWD_REDUCE, OP_BN_BWD_APPLY, OP_WGRAD, OP_WGRAD_REDUCE,
              OP_DGRAD, OP_TAN_CONV, OP_BN_TAN_FWD, OP_HEAD_TAN, OP_BN_TAN_BWD_REDUCE, OP_BN_TAN_BWD_APPLY, OP_TAN_WGRAD,
              OP_TAN_DGRAD, OP_MISC, OP_GRAM, OP_GRAM_STATS, OP_METRIC_HEAD, OP_RIDGE_HEAD, OP_PROTO_INIT, OP_LOGREG_HEAD, OP_COUNT };
static const char* kOpNames[OP_COUNT] = {"conv_fwd_stats", "bn_finalize", "bn_relu_pool_fwd", "head_fwd_bwd", "bn_bwd_reduce",
                                         "bn_bwd_apply", "wgrad", "wgrad_reduce", "dgrad", "tangent_conv_fwd", "bn_tangent_fwd",
                                         "head_tangent", "bn_tangent_bwd_reduce", "bn_tangent_bwd_apply", "tangent_wgrad",
                                         "tangent_dgrad", "misc", "input_gram", "gram_stats", "metric_head", "ridge_head", "proto_init", "logreg_head"};

static bool prof_begin(mi_engine* e, hipStream_t st, int kind) {
  if (!e || !e->prof_on || (e->prof_filter >= 0 && e->prof_filter != kind)) return false;
  if (e->ev_used == e->ev0.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return false;
    e->ev0.push_back(a); e->ev1.push_back(b); e->ev_kind.push_back(0);
  }
  e->ev_kind[e->ev_used] = kind;
  (void)hipEventRecord(e->ev0[e->ev_used], st);
  return true;
}
static void prof_end(mi_engine* e, hipStream_t st, bool active) {
  if (!active) return;
  (void)hipEventRecord(e->ev1[e->ev_used], st);
  e->ev_used++;
}

static int fail(mi_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  g_err = msg;
  return code;
}
#define LAUNCH(e, st, op, layer, call)                                                             \
  do {                                                                                             \
    const bool _pa = prof_begin(e, st, (op) * 8 + (layer));                                        \
    hipError_t _s = (call);                                                                        \
    prof_end(e, st, _pa);                                                                          \
    if (_s != hipSuccess)                                                                          \
      return fail(e, MI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s) + " @" + std::to_string(__LINE__)); \
  } while (0)
#define HIPCHK(e, call)                                                                            \
  do {                                                                                             \
    hipError_t _s = (call);                                                                        \
    if (_s != hipSuccess)                                                                          \
      return fail(e, MI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s) + " @" + std::to_string(__LINE__)); \
  } while (0)

// The head's gradient launch keeps a whole task's dlogits in LDS (head.hip): sizes that do not fit are an argument error, reported before the launch.
static int head_lds_check(mi_engine* e, const char* who, int n, int ways, int tangent) {
  if (head_lds_fits(n, ways, tangent)) return MI_OK;
  return fail(e, MI_ERR_ARG, std::string(who) + ": the classifier head's " + (tangent ? "tangent" : "gradient") + " launch with n = " + std::to_string(n) +
                                 " rows per task and ways = " + std::to_string(ways) + " needs " + std::to_string(head_grads_lds_bytes(n, ways, tangent)) +
                                 " bytes of LDS, the device has " + std::to_string(head_lds_limit_bytes()) + " (n * ways <= " + (tangent ? "19712" : "39424") + ")");
}
// The metric head keeps a task's class vectors and its dz table in LDS (metric_head.hip): the same rule.
static int metric_lds_check(mi_engine* e, const char* who, int ns, int nq, int feat, int ways) {
  if (metric_head_fits(ns, nq, feat, ways)) return MI_OK;
  return fail(e, MI_ERR_ARG, std::string(who) + ": the metric head with ns = " + std::to_string(ns) + ", nq = " + std::to_string(nq) + ", feat = " +
                                 std::to_string(feat) + " and ways = " + std::to_string(ways) + " needs ns, nq, feat >= 1, ways in 1..64 and " +
                                 std::to_string(metric_head_lds_bytes(ns, nq, feat, ways)) + " bytes of LDS, the device has " +
                                 std::to_string(head_lds_limit_bytes()));
}
// The ridge head keeps a task's Gram system, its factor and the dual coefficients in LDS in fp64 (ridge_head.hip): the same rule, feat capped.
static int ridge_lds_check(mi_engine* e, const char* who, int ns, int nq, int feat, int ways) {
  if (ridge_head_fits(ns, nq, feat, ways)) return MI_OK;
  return fail(e, MI_ERR_ARG, std::string(who) + ": the ridge head with ns = " + std::to_string(ns) + ", nq = " + std::to_string(nq) + ", feat = " +
                                 std::to_string(feat) + " and ways = " + std::to_string(ways) + " needs ns, nq >= 1, feat in 1.." +
                                 std::to_string(MI_RIDGE_MAX_FEAT) + ", ways in 1..64 and " +
                                 std::to_string(ns >= 1 && nq >= 1 && ways >= 1 ? ridge_head_lds_bytes(ns, nq, ways) : 0) +
                                 " bytes of LDS, the device has " + std::to_string(head_lds_limit_bytes()));
}
// The logistic-regression head keeps G, K, the dual coefficients and its solver's tables in LDS in fp64 (logreg_head.hip): the same rule.
static int logreg_lds_check(mi_engine* e, const char* who, int ns, int nq, int feat, int ways) {
  if (logreg_head_fits(ns, nq, feat, ways)) return MI_OK;
  return fail(e, MI_ERR_ARG, std::string(who) + ": the logistic-regression head with ns = " + std::to_string(ns) + ", nq = " + std::to_string(nq) +
                                 ", feat = " + std::to_string(feat) + " and ways = " + std::to_string(ways) + " needs ns, nq >= 1, feat in 1.." +
                                 std::to_string(MI_RIDGE_MAX_FEAT) + ", ways in 1..64 and " +
                                 std::to_string(ns >= 1 && nq >= 1 && ways >= 1 ? logreg_head_lds_bytes(ns, nq, ways) : 0) +
                                 " bytes of LDS, the device has " + std::to_string(head_lds_limit_bytes()));
}
static int ridge_hyper_check(mi_engine* e, const char* who, float lam, float alpha) {
  if (!(lam > 0.f) || !std::isfinite(lam)) return fail(e, MI_ERR_ARG, std::string(who) + ": lam must be positive and finite, got " + std::to_string(lam));
  if (!(alpha > 0.f) || !std::isfinite(alpha))
    return fail(e, MI_ERR_ARG, std::string(who) + ": alpha must be positive and finite, got " + std::to_string(alpha));
  return MI_OK;
}
// The Proto-MAML initialisation keeps nothing task-sized on chip: its domain is the stated one (proto_init.hip).
static int proto_init_size_fail(mi_engine* e, const char* who, int tasks, int ns, int feat, int ways) {
  return fail(e, MI_ERR_ARG, std::string(who) + ": the prototype initialisation with tasks = " + std::to_string(tasks) + ", ns = " + std::to_string(ns) +
                                 ", feat = " + std::to_string(feat) + " and ways = " + std::to_string(ways) + " needs tasks, ns >= 1, feat in 1.." +
                                 std::to_string(MI_RIDGE_MAX_FEAT) + " and ways in 1..64");
}
static int metric_hyper_check(mi_engine* e, const char* who, int metric, float scale) {
  if (metric != MI_METRIC_PROTO && metric != MI_METRIC_COSINE)
    return fail(e, MI_ERR_ARG, std::string(who) + ": unknown metric " + std::to_string(metric) + " (MI_METRIC_PROTO = 0, MI_METRIC_COSINE = 1)");
  if (!(scale > 0.f)) return fail(e, MI_ERR_ARG, std::string(who) + ": scale must be positive, got " + std::to_string(scale));
  return MI_OK;
}
// What the closed-form heads' argument structs (A: MetricArgs, RidgeArgs, LogregArgs) share, from pointers and sizes; each caller adds its head's own fields.
template <class A>
static A closed_form_args(const float* fs, const float* fq, const int32_t* ys, const int32_t* yq, int ns, int nq, int feat, int ways,
                          float* loss, float* acc, float* logits, float* dfs, float* dfq) {
  A a{};
  a.fs = fs; a.fq = fq; a.ys = ys; a.yq = yq; a.ns = ns; a.nq = nq; a.feat = feat; a.ways = ways;
  a.loss = loss; a.acc = acc; a.logits = logits; a.dfs = dfs; a.dfq = dfq;
  return a;
}
// the closed-form head's LDS check (head: CF_METRIC, CF_RIDGE or CF_LOGREG; the ridge and metric callers' bool is the first two): the kernel
// entries and check_call end in it
enum { CF_METRIC = 0, CF_RIDGE = 1, CF_LOGREG = 2 };
static int closed_form_lds_check(mi_engine* e, const char* who, int head, int ns, int nq, int feat, int ways) {
  return head == CF_LOGREG ? logreg_lds_check(e, who, ns, nq, feat, ways)
         : head == CF_RIDGE ? ridge_lds_check(e, who, ns, nq, feat, ways) : metric_lds_check(e, who, ns, nq, feat, ways);
}
// What the closed-form heads' kernel entries refuse, in their order: null pointers, tasks, the head's own hyper-parameters (`hyper` returns
// its check's code), alignment, LDS.
template <class A, class Hyper>
static int closed_form_entry_check(const char* who, int head, const A& a, int tasks, Hyper hyper) {
  if (!a.fs || !a.fq || !a.ys || !a.yq || !a.loss || !a.acc) return fail(nullptr, MI_ERR_ARG, std::string(who) + ": null pointer argument");
  if (tasks < 1) return fail(nullptr, MI_ERR_ARG, std::string(who) + ": tasks must be >= 1, got " + std::to_string(tasks));
  if (const int hrc = hyper()) return hrc;
  if (((reinterpret_cast<uintptr_t>(a.fs) | reinterpret_cast<uintptr_t>(a.fq) | reinterpret_cast<uintptr_t>(a.dfs) | reinterpret_cast<uintptr_t>(a.dfq)) & 15) != 0)
    return fail(nullptr, MI_ERR_ARG, std::string(who) + ": fs, fq, dfs and dfq must be 16-byte aligned");
  return closed_form_lds_check(nullptr, who, head, a.ns, a.nq, a.feat, a.ways);
}
#define HEAD_LDS(e, who, n, ways, tangent)                                         \
  do {                                                                             \
    const int _hrc = head_lds_check(e, who, n, ways, tangent);                     \
    if (_hrc) return _hrc;                                                         \
  } while (0)

static FinArgs fin_of(const mi_engine* e, int T, double inv_m, int mode, float* o0, size_t s0, float* o1, size_t s1) {
  const bool on = e->fuse_fin && e->counters && T <= mi_engine::kMaxCounterTasks;
  return FinArgs{on ? e->counters : nullptr, o0, o1, s0, s1, inv_m, mode};
}

static ConvGeom geom(const Layer& l, int n) { return ConvGeom{n, l.h, l.w, l.ho, l.wo, l.ci, l.co, l.stride}; }
static ConvGeom geom_dgrad(const Layer& l, int n) {  // op input = dz (ho,wo,co), op output = dx (h,w,ci)
  return ConvGeom{n, l.ho, l.wo, l.h, l.w, l.co, l.ci, l.stride};
}

// The dgrad of block l (l >= 1) produces the cotangent of block l-1's pooled output.  If block l-1 left zhat at the argmax next to
// p (fused block 1: zhm; hidden blocks: zhl), its BatchNorm-backward sums are an epilogue of that dgrad (EPI_BRED) -- available
// for the geometry conv3x3_s1 covers: stride-1 hidden -> hidden conv of 32 or 64 channels.
static bool dgrad_carries_reduce(const mi_engine* e, int l) {
  if (!e->fuse_b1red || l < 1 || l >= (int)e->L.size()) return false;
  const Layer& L = e->L[l];
  return L.stride == 1 && L.ci == L.co && L.co == e->L[l - 1].co && L.h == L.ho && L.w == L.wo && (L.ci == 32 || L.ci == 64);
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" const char* mi_version(void) { return "mi_maml 0.1 (gfx950)"; }
extern "C" const char* mi_last_error(const mi_engine* e) { return e ? e->err.c_str() : g_err.c_str(); }

extern "C" int mi_engine_create(const mi_model_desc* d, int device, mi_engine** out) {
  if (!d || !out) return fail(nullptr, MI_ERR_ARG, "null argument");
  if (d->n_layers < 1 || d->n_layers > 8) return fail(nullptr, MI_ERR_ARG, "n_layers must be 1..8");
  if (d->hidden != 32 && d->hidden != 64) return fail(nullptr, MI_ERR_ARG, "hidden must be 32 or 64");
  if (d->in_channels != 1 && d->in_channels != 3 && d->in_channels != 32 && d->in_channels != 64)
    return fail(nullptr, MI_ERR_ARG, "in_channels must be 1, 3, 32 or 64");
  if (d->ways < 1 || d->ways > 64) return fail(nullptr, MI_ERR_ARG, "ways must be 1..64");
  mi_engine* e = new mi_engine();
  e->d = *d;
  e->device = device;
  e->perm_dev = nullptr;
  int ci = d->in_channels, h = d->in_h, w = d->in_w;
  size_t off = 0;
  std::vector<int32_t> perm;
  for (int i = 0; i < d->n_layers; ++i) {
    Layer l;
    l.ci = ci; l.co = d->hidden; l.h = h; l.w = w;
    l.stride = d->max_pool ? 1 : 2;
    l.pool = d->max_pool ? 1 : 0;
    l.ho = (h + 2 - 3) / l.stride + 1;
    l.wo = (w + 2 - 3) / l.stride + 1;
    l.hp = l.pool ? l.ho / 2 : l.ho;
    l.wp = l.pool ? l.wo / 2 : l.wo;
    if (l.hp < 1 || l.wp < 1) { delete e; return fail(nullptr, MI_ERR_ARG, "input too small for this many blocks"); }
    l.off_gamma = off; off += l.co;
    l.off_beta = off; off += l.co;
    l.off_w = off; off += (size_t)9 * l.ci * l.co;
    l.off_b = off; off += l.co;
    for (size_t k = perm.size(); k < l.off_w; ++k) perm.push_back((int32_t)k);
    for (int tap = 0; tap < 9; ++tap)
      for (int c1 = 0; c1 < l.ci; ++c1)
        for (int c2 = 0; c2 < l.co; ++c2) perm.push_back((int32_t)(l.off_w + ((size_t)c2 * l.ci + c1) * 9 + tap));
    for (size_t k = perm.size(); k < off; ++k) perm.push_back((int32_t)k);
    e->L.push_back(l);
    ci = l.co; h = l.hp; w = l.wp;
  }
  e->fuse1 = block1_supported(e->L[0].ci, e->L[0].stride, e->L[0].pool, e->L[0].ho, e->L[0].wo, e->L[0].co);
  e->head_c = ci;
  e->head_hw = h * w;
  e->feat = d->head_mean_pool ? ci : ci * h * w;
  e->off_wl = off; off += (size_t)d->ways * e->feat;
  e->off_bl = off; off += d->ways;
  e->P = off;
  e->PS = align_up(off, 64);
  for (const Layer& l : e->L) { e->zoff[e->nzero] = (unsigned)l.off_b; e->zlen[e->nzero] = (unsigned)l.co; e->nzero++; }
  if (e->PS > e->P) { e->zoff[e->nzero] = (unsigned)e->P; e->zlen[e->nzero] = (unsigned)(e->PS - e->P); e->nzero++; }
  for (int wy = 0; wy < d->ways; ++wy)
    for (int i = 0; i < e->feat; ++i) {
      size_t ref;
      if (d->head_mean_pool) ref = (size_t)wy * e->feat + i;
      else { const int s = i / e->head_c, c = i % e->head_c; ref = (size_t)wy * e->feat + (size_t)c * e->head_hw + s; }
      perm.push_back((int32_t)(e->off_wl + ref));
    }
  for (size_t k = perm.size(); k < off; ++k) perm.push_back((int32_t)k);
  // the caller's current device is left as it was (torch tracks it on its own)
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) { delete e; return fail(nullptr, MI_ERR_HIP, "hipSetDevice failed"); }
  const bool ok = hipMalloc(&e->perm_dev, perm.size() * sizeof(int32_t)) == hipSuccess &&
                  hipMemcpy(e->perm_dev, perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc(&e->counters, mi_engine::kMaxCounterTasks * sizeof(unsigned)) == hipSuccess &&
                  hipMemset(e->counters, 0, mi_engine::kMaxCounterTasks * sizeof(unsigned)) == hipSuccess;
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
  if (!ok) {
    if (e->perm_dev) (void)hipFree(e->perm_dev);
    if (e->counters) (void)hipFree(e->counters);
    delete e;
    return fail(nullptr, MI_ERR_HIP, "allocating the parameter permutation table / arrival counters failed");
  }
  *out = e;
  return MI_OK;
}

extern "C" void mi_engine_destroy(mi_engine* e) {
  if (!e) return;
  if (e->perm_dev) (void)hipFree(e->perm_dev);
  if (e->counters) (void)hipFree(e->counters);
  for (auto& g : e->graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  for (auto& c : e->sc) {
    if (c.fork) (void)hipEventDestroy(c.fork);
    if (c.join) (void)hipEventDestroy(c.join);
  }
  for (auto ev : e->ev0) (void)hipEventDestroy(ev);
  for (auto ev : e->ev1) (void)hipEventDestroy(ev);
  delete e;
}

// Ablation / test switch: run block 1 through the generic conv + BN kernels (z stored) instead of the conv-recompute kernels.
extern "C" int mi_engine_set_fused_block1(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->fuse1 = on && block1_supported(e->L[0].ci, e->L[0].stride, e->L[0].pool, e->L[0].ho, e->L[0].wo, e->L[0].co);
  e->gram1 = on != 2;      // 2 = fused kernels, statistics by conv-recompute passes (no Gram matrix)
  e->gramq = on != 3;      // 3 = the Gram matrix for the support passes only (the query pass by conv-recompute kernels: rounds 2 - 5)
  return MI_OK;
}

// Ablation / test switch: 1 (default) = BatchNorm partials folded by the last workgroup of the producing kernel, 0 = separate
// bn_finalize launches.  Results are bit-identical either way (same fold order).
extern "C" int mi_engine_set_fused_finalize(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->fuse_fin = on != 0;
  return MI_OK;
}
// Ablation / test switch: 1 (default) = block 1's BatchNorm-backward sums computed in the epilogue of block 2's dgrad kernel,
// 0 = by a separate streaming pass (pooled_reduce).  Same fp64 sums in a different order: results agree to fp32 rounding.
extern "C" int mi_engine_set_fused_block1_reduce(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->fuse_b1red = on != 0;
  return MI_OK;
}

// 1 = replay repeated identical calls of mi_meta_batch_maml / mi_meta_batch_anil as a captured hipGraph (default 0).  Identical
// means identical ARGUMENTS: the caller must pass the same device buffers (parameters, data, outputs, workspace) again; results
// are those of the eager call (same kernels, same order).  Profiling and the debug trace switch replay off for their calls.
extern "C" int mi_engine_set_graph(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->graph_on = on != 0;
  return MI_OK;
}

// Ablation / test switch: 1 (default) = one "advance" launch ends every pass of mi_meta_batch_maml (weight-gradient folds, block 1's
// Gram assembly, the update, the next pass's Gram statistics); 0 = the separate launches.  Bit-identical results.
extern "C" int mi_engine_set_fused_tail(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->fuse_tail = on != 0;
  return MI_OK;
}

// Ablation / test switch: 1 (default) = the last block's BatchNorm + pooling, the head, its backward and that block's BatchNorm-backward sums (or
// their tangents) in one launch, four workgroups per task (tail.hip); 0 = the four separate launches per pass.  Same arithmetic in the same
// order: p, logits, loss, accuracy, the head's gradients and df are bit-identical; the BatchNorm-backward sums are the same fp64 terms folded
// in a different (fixed) order.
extern "C" int mi_engine_set_fused_last_block(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->fuse_last = on != 0;
  return MI_OK;
}

// 0 = every kernel on the caller's stream; 1 (default) = weight gradients of blocks >= 2 on an engine-owned side stream,
// forked after dz_l is written and joined before the call returns control of the gradients to the caller's stream.  One fork per hidden
// block: one per pass, with the weight gradients held back until block 2's dz exists, was measured slower (profiles/r5/overlap_fork_ab.txt).
extern "C" int mi_engine_set_overlap(mi_engine* e, int on) {
  if (!e) return MI_ERR_ARG;
  e->overlap = on != 0;
  return MI_OK;
}

// Engine-owned streams: one pool per device for the life of the process, shared by every engine on it (an engine is driven by
// one host thread and fork / join order every use; creating a stream is slow on this stack while engines are created freely).
static hipStream_t pool_stream(const mi_engine* e, int which) {
  static hipStream_t g_pool[64][1] = {};
  const int d = (e->device >= 0 && e->device < 64) ? e->device : 0;
  if (!g_pool[d][which]) {          // created on the ENGINE's device, whatever device is current in the calling thread
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != e->device) (void)hipSetDevice(e->device);
    if (hipStreamCreateWithFlags(&g_pool[d][which], hipStreamNonBlocking) != hipSuccess) g_pool[d][which] = nullptr;
    if (prev >= 0 && prev != e->device) (void)hipSetDevice(prev);
  }
  return g_pool[d][which];
}
// (hipEventReleaseToDevice instead of the default system-scope release was measured in round 5: no difference -- the ~7 us the caller's stream
// idles behind an event record are the marker packet itself, not its cache write-back; profiles/r5/overlap_fork_ab.txt)
static bool make_event(hipEvent_t* ev) { return *ev || hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess; }

// fork = the side stream waits for everything issued on `st` so far; join = `st` waits for everything issued on the side stream
static hipStream_t side_fork(mi_engine* e, hipStream_t st, int half) {
  if (!e->overlap) return st;
  mi_engine::SideCtx& c = e->sc[half];
  if (!c.side) {
    c.side = pool_stream(e, 0);
    if (!c.side || !make_event(&c.fork) || !make_event(&c.join)) { e->overlap = false; return st; }
  }
  // (stream memory operations instead of the event -- hipStreamWriteValue32 on the caller's stream, hipStreamWaitValue32 on the side stream --
  // were tried in round 5 as a cheaper fork: they fail on this stack with "invalid argument")
  if (hipEventRecord(c.fork, st) != hipSuccess || hipStreamWaitEvent(c.side, c.fork, 0) != hipSuccess) return st;
  return c.side;
}
static int side_join(mi_engine* e, hipStream_t st, int half, bool used) {
  if (!used) return MI_OK;
  mi_engine::SideCtx& c = e->sc[half];
  if (hipEventRecord(c.join, c.side) != hipSuccess || hipStreamWaitEvent(st, c.join, 0) != hipSuccess)
    return fail(e, MI_ERR_HIP, "side-stream join failed");
  return MI_OK;
}

// Debug/test aid: while set, every second-order mi_meta_batch_maml call with with_grad != 0 also writes, per task and in the
// reference's parameter order, theta_k (k = 0..K), g_k = grad L_support(theta_k), the vector lam_{k+1} fed to the k-th
// Hessian-vector product and H_support(theta_k) lam_{k+1} into `buf`:  [K+1][T][P] | [K][T][P] | [K][T][P] | [K][T][P] floats.
// While set, every forward pass of mi_meta_batch_maml (support steps 0..K-1, then the query pass) / mi_meta_batch_anil (the one trunk
// pass) also writes the BatchNorm batch statistics of every block: buf [passes][tasks][2][C_total] floats (C_total = sum of the blocks'
// filters, block-major): [0] = batch mean, [1] = biased batch variance (1/rstd^2 - eps).  The reference's BatchNorm2d layers update
// their running_mean / running_var buffers from exactly these on every learner(x) (torch momentum 0.1, unbiased variance; learn2learn's
// clone shares the buffers with the base model), and utils/experiment.py:85-90 saves them: the host side folds them into the
// model's buffers in the reference's call order (core_functions/vision_models.py::fold_running_stats).
extern "C" int mi_engine_set_bn_export(mi_engine* e, float* buf, size_t floats) {
  if (!e) return MI_ERR_ARG;
  e->bn_export = buf;
  e->bn_export_floats = buf ? floats : 0;
  return MI_OK;
}

extern "C" int mi_debug_set_trace(mi_engine* e, float* buf, size_t floats) {
  if (!e) return MI_ERR_ARG;
  e->trace = buf;
  e->trace_floats = buf ? floats : 0;
  return MI_OK;
}

int mi_internal_fail(int code, const char* msg) { return fail(nullptr, code, msg); }

extern "C" int mi_param_count(const mi_engine* e, size_t* n) {
  if (!e || !n) return MI_ERR_ARG;
  *n = e->P;
  return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
struct Bump {
  char* base;
  size_t off;
  template <class T> T* take(size_t count) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

struct ActSet {
  float *z[8], *p[8], *dz[8], *dp[8], *mu[8], *rstd[8];
  float* zhl[8];  // blocks >= 2 whose BatchNorm-backward sums ride in the next block's dgrad epilogue: zhat at the argmax of every
                  // pooled output (same shape as p[l]), else nullptr
  float* zhm;     // fused block 1 with backward: zhat at every pooling window's argmax (same shape as p[0]), else nullptr
  uint8_t* arg0;  // ... and the argmax position itself (4 = did not pass the ReLU)
  float *f, *df, *prob, *dl;
};
struct TanSet {
  float *zd[8], *pd[8], *m1[8], *m2[8];
  float* zhdl[8]; // tangent of ActSet::zhl
  float* zhdm;    // fused block 1: tangent of zhat at the argmax
  float* rdz[8];   // R{dz} per block (kept per block: the side-stream weight gradient of block l reads it while block l-1 is written)
  float *dpd[2], *fd, *rdf;
};
struct Plan {
  float *theta, *g, *lam, *hv;
  float* lam2;          // fused tail: the adjoint recursion ping-pongs between lam and lam2 (the advance launch must not update in place)
  // per-parameter step sizes (mi_meta_batch_maml_lr), else nullptr: the step sizes in engine layout [lr_steps][PS]; second order: the
  // direction lr_k * lam_{k+1} of the Hessian-vector passes [T][PS], twice (ping-pong, like lam / lam2), and the products g_k * lam_{k+1}
  // [K][T][PS] the step-size gradient sums
  float *lrv = nullptr, *dir = nullptr, *dir2 = nullptr, *prod = nullptr;
  float* ofs = nullptr; // per-step parameter offsets (mi_meta_batch_maml_offsets) in engine layout [K][PS], else nullptr
  float* qg = nullptr;  // multi-step loss (mi_meta_batch_maml_steps) with a gradient: the query gradients q_1..q_K [K][T][PS], else nullptr
  float *xs, *xq;
  int32_t *ys, *yq;
  std::vector<ActSet> sup;
  ActSet qry;
  TanSet tan;
  double* bnpart;
  float* wgpart;
  float* wgpart_side;   // partials of the weight gradients that run on the side stream
  float* wgpart_l[8];   // fused tail: one partial buffer per block (the folds wait for the pass's advance launch)
  double *gram_part, *gram_s;   // input Gram matrix of the support images (block 1 statistics), or nullptr
  double *gram_q, *gram_part_q;   // ... of the query images (mi_engine::gramq), or nullptr
  int half = 0;                 // stream context (engine SideCtx) this plan's side work uses
  float *tmp_loss, *tmp_acc;
  float* hscr;   // head scratch: R{dl} [T][n][ways], row loss [T][n], row hit [T][n]
  float* tail_wpart = nullptr; double* tail_bpart = nullptr; float* tail_scr = nullptr;   // one-launch tail (tail.hip): row-group partials
  // fp16 operand form (bf16_split.h): largest-magnitude cells [slot][T], one slot per tensor a convolution reads, handed out in launch
  // order (cell_bind: the tensor's producer is about to run; cell_of: a consumer asks) and zeroed once per call (plan_begin)
  unsigned* cells;
  int cell_cap, cell_used = 0, cell_T = 0;
  bool f16 = false;
  std::vector<std::pair<const void*, unsigned*>> cellmap;
  size_t bytes;
};

static void plan_actset(const mi_engine* e, Bump& b, ActSet& A, int T, int n, bool with_bwd) {
  const int nl = (int)e->L.size();
  A.zhm = nullptr;
  A.arg0 = nullptr;
  for (int l = 0; l < 8; ++l) A.zhl[l] = nullptr;
  for (int l = 0; l < nl; ++l) {
    const Layer& L = e->L[l];
    const size_t zs = (size_t)T * n * L.ho * L.wo * L.co, ps = (size_t)T * n * L.hp * L.wp * L.co;
    const bool fused = (l == 0 && e->fuse1);   // conv output / its gradient are recomputed, never stored
    A.z[l] = fused ? nullptr : b.take<float>(zs);
    A.p[l] = b.take<float>(ps);
    A.dz[l] = (with_bwd && !fused) ? b.take<float>(zs) : nullptr;
    A.dp[l] = with_bwd ? b.take<float>(ps) : nullptr;
    if (fused && with_bwd && e->gram1) { A.zhm = b.take<float>(ps); A.arg0 = b.take<uint8_t>(ps); }
    A.zhl[l] = (!fused && with_bwd && l >= 1 && L.pool && dgrad_carries_reduce(e, l + 1)) ? b.take<float>(ps) : nullptr;
    A.mu[l] = b.take<float>((size_t)T * L.co);
    A.rstd[l] = b.take<float>((size_t)T * L.co);
  }
  if (e->d.head_mean_pool) {
    A.f = b.take<float>((size_t)T * n * e->feat);
    A.df = with_bwd ? b.take<float>((size_t)T * n * e->feat) : nullptr;
  } else {
    A.f = A.p[nl - 1];
    A.df = A.dp[nl - 1];
  }
  A.prob = b.take<float>((size_t)T * n * e->d.ways);
  A.dl = b.take<float>((size_t)T * n * e->d.ways);
}

// Everything that decides WHICH kernels a fused call launches besides the engine's own switches: the operand form of the hidden
// convolutions, its bisecting mask, the kernel of that form (16x16x32 / 32x32x16), block 1's operand form and its sparse weight gradient's.  Part of the hipGraph cache
// key: a graph captured under one selection must not be replayed under another.
static unsigned long long kernel_selection_key() {
  unsigned mask = 0;
  const unsigned form = (unsigned)mi_conv_get_split_bf16(&mask);
  return (unsigned long long)form + 4ull * (unsigned)conv_b16() + 16ull * (unsigned)block1_split_form() + 64ull * (unsigned)sparse_wgrad_split_form() + 128ull * (unsigned long long)mask;
}

// The sizes a plan depends on: T tasks, ns support / nq query images each, K inner steps; second_order: the K support passes are kept and
// a tangent set is planned; lr_steps > 0: the step-size-vector call's buffers (want_lr_grad: its products too).  Every size query and the call
// it sizes build their shape with the same helper below, so the two cannot disagree.
// steps (mi_meta_batch_maml_steps): 0 = not that call, 1 = its query passes at every theta_j, forward only, 2 = with their gradients.
// ofs (mi_meta_batch_maml_offsets): the K rows of per-step offsets in engine layout, behind everything else.
struct PlanShape { int T, ns, nq, K, second_order, lr_steps, want_lr_grad, steps; int ofs = 0; };
static PlanShape maml_shape(int tasks, int ways, int shots, int K, int second_order, int lr_steps, int want_lr_grad, int steps = 0) {
  return PlanShape{tasks, ways * shots, ways * shots, K, second_order, lr_steps, want_lr_grad, steps};
}
static PlanShape forward_shape(int tasks, int n) { return PlanShape{tasks, n, n, 0, 0, 0, 0, 0}; }   // plain forward, learner forward / backward
static PlanShape hvp_shape(int tasks, int n) { return PlanShape{tasks, n, n, 1, 1, 0, 0, 0}; }       // mi_learner_hvp: one kept pass + tangent set

// What both plans (the fused MAML call's and ANIL's) end with, for passes over n images of each of T tasks: the BatchNorm and weight-gradient
// partials (per_block: one more weight-gradient buffer per block, for the fused tail), block 1's input Gram matrices over ng images (gram:
// the plan's own rule for when they pay; gram_q: the query set's too) and the fp16 cells (pl.cell_cap of them).  The plans differ in those
// conditions and in where the cells lie: behind the Gram buffers and whatever `between` takes (the MAML call's tangent set, which is sized
// with the largest pooled activation, handed to it), or in front of them (cells_first: ANIL).
template <class Between>
static void plan_partials(const mi_engine* e, Bump& b, Plan& pl, int T, int n, bool per_block, bool gram, int ng, bool gram_q, bool cells_first,
                          Between between) {
  const int nl = (int)e->L.size();
  size_t bnp = 0, wgp = 0, pmax = 0;
  for (int l = 0; l < nl; ++l) {
    const Layer& L = e->L[l];
    const ConvGeom gg = geom(L, n);
    int blk = conv_max_blocks_per_task(gg);
    const int bb = bn_blocks_per_task(n, L.ho, L.wo, L.co, L.pool, 1);
    if (bb > blk) blk = bb;
    const size_t need = (size_t)T * blk * 2 * L.co;
    if (need > bnp) bnp = need;
    size_t w = wgrad_partial_floats(gg, T);
    if (l == 0 && e->fuse1) {
      int bpt = block1_blocks_per_task(n, L.ho, L.wo, L.co, T);
      const int sb = sparse_wgrad_blocks_per_task(n, L.ho, L.wo, L.co, T);
      if (sb > bpt) bpt = sb;
      w = (size_t)T * bpt * 9 * L.ci * L.co;
    }
    if (w > wgp) wgp = w;
    const size_t ps = (size_t)T * n * L.hp * L.wp * L.co;
    if (ps > pmax) pmax = ps;
  }
  pl.bnpart = b.take<double>(bnp);
  pl.wgpart = b.take<float>(wgp);
  pl.wgpart_side = b.take<float>(wgp);
  for (int l = 0; l < 8; ++l) pl.wgpart_l[l] = nullptr;
  for (int l = 0; per_block && l < nl; ++l) {
    if (l == 0 && e->fuse1) { pl.wgpart_l[0] = pl.wgpart; continue; }     // block 1's sparse partials: consumed inside the same advance launch
    pl.wgpart_l[l] = b.take<float>(wgrad_partial_floats(geom(e->L[l], n), T));
  }
  // (reserved only while the fp16 operand form is selected -- 4 KB per tensor and task, ~20 MB at cfg2; the workspace size is recomputed by
  // every call with the form then in force, so a caller that switches forms is asked for the larger workspace by the size check)
  auto cells = [&] {
    pl.cells = conv_operand_form() == 2 ? b.take<unsigned>((size_t)pl.cell_cap * T * MI_CELL_WORDS) : nullptr;
    pl.cell_T = T;
  };
  if (cells_first) cells();
  pl.gram_part = pl.gram_s = pl.gram_q = pl.gram_part_q = nullptr;
  if (gram && e->fuse1 && e->gram1 && gram_supported(e->L[0].w, e->L[0].ci)) {
    pl.gram_part = b.take<double>(gram_partial_doubles(T, ng, e->L[0].h, e->L[0].ci));
    pl.gram_s = b.take<double>(gram_doubles(T, e->L[0].ci));
    if (gram_q) {
      pl.gram_q = b.take<double>(gram_doubles(T, e->L[0].ci));
      pl.gram_part_q = b.take<double>(gram_partial_doubles(T, ng, e->L[0].h, e->L[0].ci));
    }
  }
  if (!cells_first) { between(pmax); cells(); }
}

static void make_plan(const mi_engine* e, void* ws, const PlanShape& s, Plan& pl) {
  const int T = s.T, ns = s.ns, nq = s.nq, K = s.K, second_order = s.second_order;
  Bump b{reinterpret_cast<char*>(ws), 0};
  const int nl = (int)e->L.size();
  const size_t TP = (size_t)T * e->PS;
  pl.theta = b.take<float>(TP * (K + 1));
  pl.g = b.take<float>(TP * (K > 0 ? K : 1));
  pl.lam = b.take<float>(TP);
  pl.hv = b.take<float>(TP);
  pl.lam2 = (second_order && K > 0) ? b.take<float>(TP) : nullptr;
  const size_t img = (size_t)e->d.in_h * e->d.in_w * e->d.in_channels;
  pl.xs = b.take<float>((size_t)T * ns * img);
  pl.xq = b.take<float>((size_t)T * nq * img);
  pl.ys = b.take<int32_t>((size_t)T * ns);
  pl.yq = b.take<int32_t>((size_t)T * nq);
  pl.tmp_loss = b.take<float>(T);
  pl.tmp_acc = b.take<float>(T);
  const int nmax = ns > nq ? ns : nq;      // (partial buffers and scratch are sized for the larger of support / query passes)
  pl.hscr = b.take<float>((size_t)T * nmax * (e->d.ways + 2));
  pl.tail_wpart = b.take<float>(tail_wpart_floats(T, e->feat, e->d.ways));
  pl.tail_bpart = b.take<double>(tail_bpart_doubles(T, e->L.back().co));
  pl.tail_scr = b.take<float>(tail_scr_floats(T, nmax, e->d.ways));
  const int nsets = (second_order && K > 0) ? K : 1;
  pl.sup.resize(nsets);
  for (int k = 0; k < nsets; ++k) plan_actset(e, b, pl.sup[k], T, ns, true);
  plan_actset(e, b, pl.qry, T, nq, true);
  pl.cell_cap = 8 + (K + 1) * 2 * nl + K * 4 * nl + 4 * nl;      // p and dz per block and pass, pd and R{dz} per Hessian-vector pass, spare
  if (s.steps) pl.cell_cap += K * 2 * nl;                        // ... and of the K further query passes
  const bool swept_twice = K >= 2 || (K >= 1 && second_order);   // the support set is swept at least twice: its Gram matrix pays
  plan_partials(e, b, pl, T, nmax, true, swept_twice, ns, e->gramq && nq == ns, false, [&](size_t pmax) {
    if (!(second_order && K > 0)) return;
    TanSet& X = pl.tan;
    for (int l = 0; l < nl; ++l) {
      const Layer& L = e->L[l];
      X.zd[l] = (l == 0 && e->fuse1) ? nullptr : b.take<float>((size_t)T * ns * L.ho * L.wo * L.co);
      X.pd[l] = b.take<float>((size_t)T * ns * L.hp * L.wp * L.co);
      if (l == 0) X.zhdm = e->fuse1 ? b.take<float>((size_t)T * ns * L.hp * L.wp * L.co) : nullptr;
      X.zhdl[l] = (!(l == 0 && e->fuse1) && l >= 1 && L.pool && dgrad_carries_reduce(e, l + 1)) ? b.take<float>((size_t)T * ns * L.hp * L.wp * L.co) : nullptr;
      X.m1[l] = b.take<float>((size_t)T * L.co);
      X.m2[l] = b.take<float>((size_t)T * L.co);
    }
    for (int l = 0; l < nl; ++l) {
      const Layer& L = e->L[l];
      X.rdz[l] = (l == 0 && e->fuse1) ? nullptr : b.take<float>((size_t)T * ns * L.ho * L.wo * L.co);
    }
    X.dpd[0] = b.take<float>(pmax);
    X.dpd[1] = b.take<float>(pmax);
    if (e->d.head_mean_pool) {
      X.fd = b.take<float>((size_t)T * ns * e->feat);
      X.rdf = b.take<float>((size_t)T * ns * e->feat);
    } else {
      X.fd = nullptr;
      X.rdf = nullptr;
    }
  });
  if (s.lr_steps > 0) {      // (behind everything else: the scalar call's layout is the prefix)
    pl.lrv = b.take<float>((size_t)s.lr_steps * e->PS);
    if (second_order && K > 0) {
      pl.dir = b.take<float>(TP);
      pl.dir2 = b.take<float>(TP);
      if (s.want_lr_grad) pl.prod = b.take<float>(TP * K);
    } else if (s.steps == 2 && s.want_lr_grad) {      // first order with the multi-step loss: lam_{k+1} differs from step to step
      pl.prod = b.take<float>(TP * K);
    }
  }
  if (s.steps == 2) pl.qg = b.take<float>(TP * K);
  if (s.ofs) pl.ofs = b.take<float>((size_t)K * e->PS);
  pl.bytes = align_up(b.off, 256);
}

// The plan of shape s laid into the caller's workspace, or the error that names the size it needs.
static int plan_in(mi_engine* e, void* workspace, size_t workspace_bytes, const PlanShape& s, Plan& pl) {
  make_plan(e, workspace, s, pl);
  if (pl.bytes > workspace_bytes)
    return fail(e, MI_ERR_WORKSPACE, "workspace too small: need " + std::to_string(pl.bytes) + " bytes");
  return MI_OK;
}

static int plan_bytes(const mi_engine* e, const PlanShape& s, size_t* bytes) {      // ... and that size alone (the mi_*_workspace_bytes queries)
  Plan pl;
  make_plan(e, nullptr, s, pl);
  *bytes = pl.bytes;
  return MI_OK;
}

// ---- fp16 operand form: the largest-magnitude cell of every tensor a convolution reads
static int plan_begin(mi_engine* e, hipStream_t st, Plan& pl) {
  pl.f16 = conv_operand_form() == 2;
  pl.cell_used = 0;
  pl.cellmap.clear();
  if (pl.f16) HIPCHK(e, hipMemsetAsync(pl.cells, 0, (size_t)pl.cell_cap * pl.cell_T * MI_CELL_WORDS * sizeof(unsigned), st));
  return MI_OK;
}
// the producer of `tensor` is about to be launched: a fresh cell for it to fold max |tensor| into (nullptr: no fp16 form, or no slot
// left -- its consumers then ask launch_amax, or fail there)
static unsigned* cell_bind(mi_engine* e, Plan& pl, const void* tensor) {
  static const bool no_hooks = getenv("MI_F16_NO_PRODUCER_AMAX") && atoi(getenv("MI_F16_NO_PRODUCER_AMAX")) != 0;   // debug: every cell from launch_amax
  if (!pl.f16 || !tensor) return nullptr;
  for (auto it = pl.cellmap.begin(); it != pl.cellmap.end(); ++it)
    if (it->first == tensor) { pl.cellmap.erase(it); break; }      // the tensor is being rewritten: its old cell is stale
  if (no_hooks || pl.cell_used >= pl.cell_cap) return nullptr;
  unsigned* c = pl.cells + (size_t)(pl.cell_used++) * pl.cell_T * MI_CELL_WORDS;
  pl.cellmap.emplace_back(tensor, c);
  return c;
}
// a convolution is about to read `tensor` ([T][per_task] floats): its cell -- from its producer, else a reduction launch here
static int cell_of(mi_engine* e, hipStream_t st, Plan& pl, const float* tensor, size_t per_task, int T, const unsigned** out) {
  *out = nullptr;
  if (!pl.f16 || !tensor) return MI_OK;
  for (const auto& kv : pl.cellmap)
    if (kv.first == tensor) { *out = kv.second; return MI_OK; }
  if (pl.cell_used >= pl.cell_cap) return fail(e, MI_ERR_WORKSPACE, "fp16 operand form: no largest-magnitude cell left for this call");
  unsigned* c = pl.cells + (size_t)(pl.cell_used++) * pl.cell_T * MI_CELL_WORDS;
  pl.cellmap.emplace_back(tensor, c);
  LAUNCH(e, st, OP_MISC, 5, launch_amax(st, tensor, per_task, T, c));
  *out = c;
  return MI_OK;
}

// Debug/test aid: byte offsets inside the workspace of a mi_meta_batch_maml call with these sizes.
// out = {theta, g, xs, sup[0].p[0], sup[0].dp[0], sup[0].mu[0], sup[0].rstd[0], sup[0].p[1], qry.p[0], total bytes}
extern "C" int mi_debug_plan_offsets(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order,
                                     size_t* out) {
  if (!e || !out) return MI_ERR_ARG;
  Plan pl;
  char* base = reinterpret_cast<char*>(4096);
  make_plan(e, base, maml_shape(tasks, ways, shots, adapt_steps, second_order, 0, 0), pl);
  auto off = [&](const void* p) { return (size_t)(reinterpret_cast<const char*>(p) - base); };
  out[0] = off(pl.theta); out[1] = off(pl.g); out[2] = off(pl.xs); out[3] = off(pl.sup[0].p[0]); out[4] = off(pl.sup[0].dp[0]);
  out[5] = off(pl.sup[0].mu[0]); out[6] = off(pl.sup[0].rstd[0]); out[7] = off(pl.sup[0].p[1]); out[8] = off(pl.qry.p[0]);
  out[9] = pl.bytes;
  return MI_OK;
}

// The step-size-vector call takes one row of step sizes for every inner step, or one per inner step (without inner steps: one row).
static bool lr_steps_ok(int lr_steps, int adapt_steps) { return lr_steps == 1 || (adapt_steps > 0 && lr_steps == adapt_steps); }

extern "C" int mi_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order,
                                  size_t* bytes) {
  if (!e || !bytes || tasks < 1 || ways < 1 || shots < 1 || adapt_steps < 0) return MI_ERR_ARG;
  return plan_bytes(e, maml_shape(tasks, ways, shots, adapt_steps, second_order, 0, 0), bytes);
}

extern "C" int mi_workspace_bytes_lr(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order, int lr_steps,
                                     int want_lr_grad, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || ways < 1 || shots < 1 || adapt_steps < 0) return MI_ERR_ARG;
  if (!lr_steps_ok(lr_steps, adapt_steps)) return MI_ERR_ARG;
  return plan_bytes(e, maml_shape(tasks, ways, shots, adapt_steps, second_order, lr_steps, want_lr_grad), bytes);
}

// mi_meta_batch_maml_steps: lr_steps = 0 for the scalar step, else as mi_workspace_bytes_lr; grad_tasks as the call's (0: no query gradients kept).
static PlanShape steps_shape(int tasks, int grad_tasks, int ways, int shots, int K, int second_order, int lr_steps, int want_lr_grad) {
  return maml_shape(tasks, ways, shots, K, (second_order && grad_tasks > 0) ? 1 : 0, lr_steps, want_lr_grad, grad_tasks > 0 ? 2 : 1);
}
extern "C" int mi_workspace_bytes_steps(const mi_engine* e, int tasks, int grad_tasks, int ways, int shots, int adapt_steps, int second_order,
                                        int lr_steps, int want_lr_grad, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || grad_tasks < 0 || grad_tasks > tasks || ways < 1 || shots < 1 || adapt_steps < 1) return MI_ERR_ARG;
  if (lr_steps != 0 && !lr_steps_ok(lr_steps, adapt_steps)) return MI_ERR_ARG;
  return plan_bytes(e, steps_shape(tasks, grad_tasks, ways, shots, adapt_steps, second_order, lr_steps, want_lr_grad), bytes);
}

// mi_meta_batch_maml_offsets: the plain plan (with_steps = 0: step_w NULL) or the steps call's, lr_steps = 0 for the scalar step, plus the
// offsets in engine layout.
static PlanShape offsets_shape(int tasks, int grad_tasks, int ways, int shots, int K, int second_order, int lr_steps, int want_lr_grad, int with_steps) {
  PlanShape s = with_steps ? steps_shape(tasks, grad_tasks, ways, shots, K, second_order, lr_steps, want_lr_grad)
                           : maml_shape(tasks, ways, shots, K, (second_order && grad_tasks > 0) ? 1 : 0, lr_steps, want_lr_grad);
  s.ofs = 1;
  return s;
}
extern "C" int mi_workspace_bytes_offsets(const mi_engine* e, int tasks, int grad_tasks, int ways, int shots, int adapt_steps, int second_order,
                                          int lr_steps, int want_lr_grad, int with_steps, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || grad_tasks < 0 || grad_tasks > tasks || ways < 1 || shots < 1 || adapt_steps < 1) return MI_ERR_ARG;
  if (lr_steps != 0 && !lr_steps_ok(lr_steps, adapt_steps)) return MI_ERR_ARG;
  return plan_bytes(e, offsets_shape(tasks, grad_tasks, ways, shots, adapt_steps, second_order, lr_steps, want_lr_grad, with_steps), bytes);
}

// ---------------------------------------------------------------------------------------------------------------------
// "This sweep is the tangent one": trunk_forward / trunk_backward given a Tangent walk the blocks exactly as the primal sweep does, over the
// SAVED primal pass A, and produce its directional derivative along v -- forward tangents into X, R{gradient} into hv (forward-over-reverse).
struct Tangent {
  const float* v;    // direction [T][PS]
  const float* g;    // gradient of the saved primal pass (its BatchNorm-backward sums)
  float* hv;         // R{g} = H v
  TanSet& X;
  int cur = 0;       // X.dpd[cur]: tangent of the cotangent of the block the backward sweep is at (ping-pong, flipped by every dgrad)
};

// (fp16 operand form) the largest-magnitude cell of a tensor a convolution is about to read, on the caller's stream `st`
#define CELL(ptr, per_task, out)                                                   \
  do {                                                                             \
    const int _crc = cell_of(e, st, pl, ptr, per_task, T, &(out));                 \
    if (_crc) return _crc;                                                         \
  } while (0)

// ---- argument builders: what every launch of a block / the head has in common; the launch sites add what they write.  Tangent fields are
// filled in the tangent sweep only.
static B1Args b1_args(const mi_engine* e, Plan& pl, const ActSet& A, const Tangent* tan, const float* x0, int n, const float* theta) {
  const Layer& L = e->L[0];
  const size_t P = e->PS;
  B1Args a{};
  a.x = x0;
  a.w = theta + L.off_w; a.wstride = P;
  a.mu = A.mu[0]; a.rstd = A.rstd[0];
  a.gamma = theta + L.off_gamma; a.beta = theta + L.off_beta; a.pstride = P;
  a.partial = pl.bnpart; a.wpartial = pl.wgpart;
  a.n = n; a.hh = L.ho; a.ww = L.wo; a.co = L.co;
  a.inv_m = 1.f / (float)(n * L.ho * L.wo);
  if (tan) {
    a.wd = tan->v + L.off_w; a.vstride = P;
    a.m1 = tan->X.m1[0]; a.m2 = tan->X.m2[0];
    a.gammad = tan->v + L.off_gamma; a.betad = tan->v + L.off_beta;
    a.dgamma = tan->g + L.off_gamma; a.dbeta = tan->g + L.off_beta; a.gstride = P;
  }
  return a;
}

// BatchNorm of generic block l over the saved pass A: inputs only (out, zh_out, amax_out, partial, fin and the sums a backward sweep has
// just formed belong to the launch site)
static BnArgs bn_args(const mi_engine* e, const ActSet& A, const Tangent* tan, int l, int n, const float* theta) {
  const Layer& L = e->L[l];
  const size_t P = e->PS;
  BnArgs ba{};
  ba.z = A.z[l]; ba.mu = A.mu[l]; ba.rstd = A.rstd[l];
  ba.gamma = theta + L.off_gamma; ba.beta = theta + L.off_beta; ba.pstride = P;
  ba.dp = A.dp[l];
  ba.n = n; ba.ho = L.ho; ba.wo = L.wo; ba.c = L.co;
  ba.inv_m = 1.f / (float)(n * L.ho * L.wo);
  if (tan) {
    ba.zd = tan->X.zd[l]; ba.m1 = tan->X.m1[l]; ba.m2 = tan->X.m2[l];
    ba.gammad = tan->v + L.off_gamma; ba.betad = tan->v + L.off_beta; ba.vstride = P;
    ba.dgamma = tan->g + L.off_gamma; ba.dbeta = tan->g + L.off_beta; ba.gstride = P;
    ba.dpd = tan->X.dpd[tan->cur];
  }
  return ba;
}

// The head on features f with weights theta (tangent: direction v): gradients (or their tangents) into g -- nullptr: none -- and df.
// hscr: head scratch R{dl} [T][n][ways], row loss [T][n], row hit [T][n] (nullptr: a launch that needs none).
static HeadArgs head_args(const mi_engine* e, float* hscr, const float* f, const float* theta, const float* v, float* g, float* df, int n, int T) {
  HeadArgs ha{};
  ha.f = f;
  ha.wl = theta + e->off_wl; ha.bl = theta + e->off_bl; ha.pstride = e->PS;
  if (v) { ha.wld = v + e->off_wl; ha.bld = v + e->off_bl; ha.vstride = e->PS; }
  ha.dwl = g ? g + e->off_wl : nullptr; ha.dbl = g ? g + e->off_bl : nullptr; ha.gstride = e->PS;
  ha.df = df;
  ha.n = n; ha.feat = e->feat; ha.ways = e->d.ways;
  if (hscr) {
    ha.rdl = hscr;
    ha.rowloss = hscr + (size_t)T * n * e->d.ways;
    ha.rowhit = ha.rowloss + (size_t)T * n;
  }
  return ha;
}
// ... of a primal pass: labels in, loss / accuracy / logits out, prob & dl saved for the tangent pass
static HeadArgs head_args_primal(const mi_engine* e, float* hscr, const float* f, const int32_t* y, int n, int T, const float* theta, float* g,
                                 float* loss, float* acc, float* logits, float* prob, float* dl, float* df, bool with_grad) {
  HeadArgs ha = head_args(e, hscr, f, theta, nullptr, with_grad ? g : nullptr, with_grad ? df : nullptr, n, T);
  ha.y = y; ha.loss = loss; ha.acc = acc; ha.logits = logits; ha.prob = prob; ha.dl = dl;
  return ha;
}

// The one-launch tail (tail.hip) serves a generic last block (not the conv-recompute block 1) feeding a flattened head, outside the fp16
// operand form (its producers would have to fold largest-magnitude cells).
static bool fused_last_ok(const mi_engine* e, const Plan& pl, int n, int T) {
  const int nl = (int)e->L.size();
  if (!e->fuse_last || e->d.head_mean_pool || pl.f16 || (nl == 1 && e->fuse1) || !e->counters || T > mi_engine::kMaxCounterTasks || T > 65535 ||
      !pl.tail_wpart)
    return false;
  const Layer& L = e->L[nl - 1];
  return tail_supported(n, L.ho, L.wo, L.co, L.pool, e->feat, e->d.ways);
}
// The last block's BatchNorm + pooling, the head `ha`, its backward and that block's BatchNorm-backward sums into g (tangent sweep: the
// tangents of all of these) as one launch.  Tb: tasks that take the backward half.
static TailArgs tail_args(const mi_engine* e, const Plan& pl, const ActSet& A, const Tangent* tan, const HeadArgs& ha, int n, const float* theta,
                          float* g, bool with_grad, int Tb) {
  const int l = (int)e->L.size() - 1;
  const Layer& L = e->L[l];
  TailArgs ta{};
  ta.bn = bn_args(e, A, tan, l, n, theta);
  ta.bn.out = tan ? tan->X.rdz[l] : A.dz[l];
  ta.hd = ha;
  ta.pooled = tan ? tan->X.pd[l] : A.p[l];
  ta.sum0 = with_grad ? g + L.off_gamma : nullptr; ta.sum1 = with_grad ? g + L.off_beta : nullptr; ta.sum_stride = e->PS;
  ta.with_grad = with_grad ? 1 : 0; ta.bwd_tasks = Tb;
  ta.wpart = pl.tail_wpart; ta.bpart = pl.tail_bpart; ta.scr = pl.tail_scr; ta.counter = e->counters; ta.stamps = e->tail_stamps;
  return ta;
}
// Debug aid: while set, every launch of the one-launch tail (tail.hip) writes the 100 MHz wall clock at its stage boundaries, thread 0 of each of
// its workgroups: buf [tasks][4][16] 64-bit words (device memory; the LAST tail launch of a call is what remains).  NULL switches it off.
extern "C" int mi_debug_tail_stamps(mi_engine* e, unsigned long long* buf) {
  if (!e) return MI_ERR_ARG;
  e->tail_stamps = buf;
  return MI_OK;
}

// Block 1's backward reads the argmax its forward stored (sparse weight gradient on the matrix pipe, dense parts from the Gram matrix)
// instead of recomputing conv1 and re-deriving the pooling / ReLU decisions.
static bool block1_reads_stored_argmax(const mi_engine* e, const ActSet& A, const double* gram) {
  const Layer& L = e->L[0];
  return gram && A.arg0 && sparse_wgrad_supported(L.wo, L.ci, L.co);
}

// Trunk forward: ConvBlocks on n images per task (conv + BN-stat epilogue, finalize, BN+ReLU+pool).
// skip_last_bn: the last block's BatchNorm + pooling belongs to the caller's tail launch.
// tan: the tangent of that sweep over the saved pass A (two-term convs with the tangent statistics m1 / m2 in the epilogue, tangent BN).
static int trunk_forward(mi_engine* e, hipStream_t st, Plan& pl, ActSet& A, const float* x0, int n, int T, const float* theta,
                         const double* gram = nullptr, bool stats_ready = false, bool skip_last_bn = false, const Tangent* tan = nullptr) {
  const int nl = (int)e->L.size();
  const size_t P = e->PS;  // task stride
  const int fin_mode = tan ? FIN_TSTATS : FIN_STATS, op_conv = tan ? OP_TAN_CONV : OP_CONV_FWD, op_bn = tan ? OP_BN_TAN_FWD : OP_BN_FWD;
  for (int l = 0; l < nl; ++l) {
    const Layer& L = e->L[l];
    const int mpix = n * L.ho * L.wo;
    const double inv_m = 1.0 / ((double)n * L.ho * L.wo);
    float* s0 = tan ? tan->X.m1[l] : A.mu[l];      // this sweep's statistics: mean / rstd of z, or mean(zd) / mean(zhat zd)
    float* s1 = tan ? tan->X.m2[l] : A.rstd[l];
    if (l == 0 && e->fuse1) {
      B1Args ba = b1_args(e, pl, A, tan, x0, n, theta);
      int blk = 0;
      if (gram && stats_ready) {   // ... already formed by the advance launch that ended the previous pass
      } else if (gram) {   // mean / variance of conv1's output as quadratic forms of this step's weights (gram.hip)
        LAUNCH(e, st, OP_GRAM_STATS, 0, launch_gram_stats(st, gram, T, L.ci, L.co, theta + L.off_w, P, ba.wd, ba.vstride, inv_m, tan ? 1 : 0, s0, s1,
                                                          tan ? A.mu[0] : nullptr, tan ? A.rstd[0] : nullptr));
      } else {
        ba.fin = fin_of(e, T, inv_m, fin_mode, s0, L.co, s1, L.co);
        LAUNCH(e, st, op_conv, 0, launch_block1(st, ba, T, L.ci, tan ? B1_TSTATS : B1_STATS, &blk));
        if (!ba.fin.counter)
          LAUNCH(e, st, OP_BN_FINALIZE, 0, launch_bn_finalize(st, pl.bnpart, blk, T, L.co, inv_m, fin_mode, s0, L.co, s1, L.co));
        ba.fin = FinArgs{};
      }
      int mode = B1_FWD;
      if (tan) {
        ba.out = tan->X.pd[0];
        ba.zh_out = A.zhm ? tan->X.zhdm : nullptr;
        mode = B1_TFWD;
        if (A.zhm && A.arg0) {   // the forward pass kept zhat and the argmax: one conv with the direction's weights suffices
          ba.arg_in = A.arg0; ba.zh_in = A.zhm;
          mode = B1_TFWD_ARG;
        }
      } else {
        ba.out = A.p[0];
        ba.zh_out = A.zhm;
        ba.arg_out = A.arg0;
        // Without the Gram path this pass's backward (or tangent) kernels recompute conv1 on the fp32 pipe and re-derive the pooling / ReLU decisions
        // from it: the forward must then round the same way.  With it every later kernel reads the decisions this launch stores.
        // (This is NOT block1_reads_stored_argmax: the two differ where the sparse weight gradient does not take the geometry -- ADVICE.md's
        // medium finding.  Making them agree changes results there and is left to its own change.)
        ba.fwd_fp32 = (gram && A.arg0) ? 0 : 1;
      }
      ba.amax_out = cell_bind(e, pl, ba.out);
      LAUNCH(e, st, op_bn, 0, launch_block1(st, ba, T, L.ci, mode, nullptr));
      continue;
    }
    ConvArgs ca{};
    int nterms = 1;
    ca.in[0] = l == 0 ? x0 : A.p[l - 1];
    ca.wt[0] = (tan ? tan->v : theta) + L.off_w;
    if (tan) {
      if (l > 0) { ca.in[1] = tan->X.pd[l - 1]; ca.wt[1] = theta + L.off_w; nterms = 2; }
      ca.z = A.z[l]; ca.mu = A.mu[l]; ca.rstd = A.rstd[l];
    }
    ca.wstride = P;
    ca.out = tan ? tan->X.zd[l] : A.z[l];
    ca.partial = pl.bnpart;
    ca.g = geom(L, n);
    ca.mpix = mpix;
    int blk = 0;
    ca.fin = fin_of(e, T, 1.0 / (double)mpix, fin_mode, s0, L.co, s1, L.co);
    if (l >= 1) {
      CELL(ca.in[0], (size_t)n * L.h * L.w * L.ci, ca.amax[0]);
      if (tan) CELL(ca.in[1], (size_t)n * L.h * L.w * L.ci, ca.amax[1]);
    }
    LAUNCH(e, st, op_conv, l, launch_conv3x3(st, ca, T, nterms, tan ? EPI_TSTATS : EPI_STATS, 0, &blk));
    if (!ca.fin.counter)
      LAUNCH(e, st, OP_BN_FINALIZE, l, launch_bn_finalize(st, pl.bnpart, blk, T, L.co, 1.0 / (double)mpix, fin_mode, s0, L.co, s1, L.co));
    if (skip_last_bn && l == nl - 1) break;
    BnArgs ba = bn_args(e, A, tan, l, n, theta);
    ba.out = tan ? tan->X.pd[l] : A.p[l];
    ba.zh_out = tan ? (A.zhl[l] ? tan->X.zhdl[l] : nullptr) : A.zhl[l];
    ba.amax_out = cell_bind(e, pl, ba.out);
    LAUNCH(e, st, op_bn, l, tan ? launch_bn_tan_fwd(st, ba, T, L.pool) : launch_bn_fwd(st, ba, T, L.pool));
  }
  return MI_OK;
}

// zhat at the argmax of block `lower`'s pooled outputs, if the forward pass kept it (fused block 1: zhm; hidden blocks: zhl)
static const float* zh_at_argmax(const mi_engine* e, const ActSet& A, int lower) {
  return (lower == 0 && e->fuse1) ? A.zhm : A.zhl[lower];
}

static void adv_add_seg(AdvanceArgs* adv, size_t off, int nelem, const float* partial, int nchunks) {
  AdvanceSeg& sg = adv->seg[adv->nseg++];
  sg.off = (unsigned)off; sg.nelem = (unsigned)nelem; sg.partial = partial; sg.nchunks = nchunks;
}
// Trunk backward from A.dp[last] (gradient w.r.t. the last block's output): writes gamma/beta/conv-weight gradients into g.
// adv != nullptr (fused tail): weight-gradient folds and block 1's Gram assembly are recorded in *adv for the caller's advance launch
// instead of being launched here; every block then writes its own partial buffer (pl.wgpart_l).
// last_bn_done: the caller's tail launch already formed the last block's dgamma / dbeta (the apply is launched here).
// tan: the tangent of that sweep, from tan->X.dpd[tan->cur]: g is then tan->hv, and every launch has the primal term and its tangent.
static int trunk_backward(mi_engine* e, hipStream_t st, Plan& pl, ActSet& A, const float* x0, int n, int T, const float* theta,
                          float* g, const double* gram = nullptr, AdvanceArgs* adv = nullptr, bool last_bn_done = false, Tangent* tan = nullptr) {
  const int nl = (int)e->L.size();
  const size_t P = e->PS;
  const int op_red = tan ? OP_BN_TAN_BWD_REDUCE : OP_BN_BWD_REDUCE, op_apply = tan ? OP_BN_TAN_BWD_APPLY : OP_BN_BWD_APPLY,
            op_wgrad = tan ? OP_TAN_WGRAD : OP_WGRAD, op_dgrad = tan ? OP_TAN_DGRAD : OP_DGRAD;
  bool forked = false, red_done[9] = {false, false, false, false, false, false, false, false, false};   // [l]: block l's sums rode in block l+1's dgrad
  auto issue_wgrad = [&](hipStream_t ws, WgradArgs& w, int wl) -> int {
    const Layer& Lw = e->L[wl];
    w.partial = adv ? pl.wgpart_l[wl] : (ws != st ? pl.wgpart_side : pl.wgpart);
    int nch = 0;
    LAUNCH(e, ws, op_wgrad, wl, launch_wgrad3x3(ws, w, T, (tan && wl > 0) ? 2 : 1, &nch));
    if (adv) adv_add_seg(adv, Lw.off_w, 9 * Lw.ci * Lw.co, w.partial, nch);
    else LAUNCH(e, ws, OP_WGRAD_REDUCE, wl, launch_wgrad_reduce(ws, w.partial, nch, 9 * Lw.ci * Lw.co, T, g + Lw.off_w, P));
    return MI_OK;
  };
  for (int l = nl - 1; l >= 0; --l) {
    const Layer& L = e->L[l];
    const int mpix = n * L.ho * L.wo;
    const float* dpd = tan ? tan->X.dpd[tan->cur] : nullptr;
    if (l == 0 && e->fuse1) {
      B1Args b1 = b1_args(e, pl, A, tan, x0, n, theta);
      b1.dp = A.dp[0]; b1.dpd = dpd;
      int blk = 0;
      const FinArgs fin = fin_of(e, T, 1.0, FIN_SUMS, g + L.off_gamma, P, g + L.off_beta, P);
      if (red_done[0]) {   // already summed in the epilogue of block 2's dgrad
      } else if (A.zhm) {   // dgamma / dbeta from pooled-resolution tensors (no conv recompute)
        PoolRedArgs pr{A.p[0], A.zhm, tan ? tan->X.zhdm : nullptr, A.dp[0], dpd, pl.bnpart, n * L.hp * L.wp, L.co, fin};
        LAUNCH(e, st, op_red, 0, launch_pooled_reduce(st, pr, T, tan ? 1 : 0, &blk));
      } else {
        b1.fin = fin;
        LAUNCH(e, st, op_red, 0, launch_block1(st, b1, T, L.ci, tan ? B1_TBWD_REDUCE : B1_BWD_REDUCE, &blk));
        b1.fin = FinArgs{};
      }
      if (!fin.counter && !red_done[0])
        LAUNCH(e, st, OP_BN_FINALIZE, 0, launch_bn_finalize(st, pl.bnpart, blk, T, L.co, 1.0, FIN_SUMS, g + L.off_gamma, P, g + L.off_beta, P));
      if (tan) { b1.rdgamma = g + L.off_gamma; b1.rdbeta = g + L.off_beta; b1.hstride = P; }
      else { b1.dgamma = g + L.off_gamma; b1.dbeta = g + L.off_beta; b1.gstride = P; }
      if (block1_reads_stored_argmax(e, A, gram)) {
        SparseWgArgs sw{};
        sw.x = x0; sw.arg = A.arg0; sw.dp = A.dp[0]; sw.wpartial = pl.wgpart; sw.n = n; sw.hh = L.ho; sw.ww = L.wo; sw.co = L.co;
        if (tan) {
          sw.dpd = dpd; sw.rstd = A.rstd[0]; sw.m2 = b1.m2;
          sw.gamma = b1.gamma; sw.pstride = P; sw.gammad = b1.gammad; sw.vstride = P;
        }
        LAUNCH(e, st, op_wgrad, 0, launch_sparse_wgrad(st, sw, T, L.ci, tan ? 1 : 0, &blk));
        GramWgArgs gw{};   // (b1's tangent fields are null / 0 in the primal sweep)
        gw.g = gram; gw.spartial = pl.wgpart; gw.nblk = blk; gw.w = b1.w; gw.wstride = P; gw.wd = b1.wd; gw.vstride = b1.vstride;
        gw.mu = A.mu[0]; gw.rstd = A.rstd[0]; gw.m1 = b1.m1; gw.m2 = b1.m2;
        gw.gamma = b1.gamma; gw.pstride = P; gw.gammad = b1.gammad;
        gw.dgamma = b1.dgamma; gw.dbeta = b1.dbeta; gw.gstride = P;
        gw.rdgamma = b1.rdgamma; gw.rdbeta = b1.rdbeta; gw.hstride = b1.hstride;
        gw.out = g + L.off_w; gw.ostride = P; gw.ci = L.ci; gw.co = L.co; gw.inv_m = 1.0 / (double)mpix;
        if (adv) { adv->b1_wgrad = 1; adv->gw_tangent = tan ? 1 : 0; adv->gw = gw; }
        else LAUNCH(e, st, OP_WGRAD_REDUCE, 0, launch_gram_wgrad(st, gw, T, tan ? 1 : 0));
        continue;
      }
      LAUNCH(e, st, op_wgrad, 0, launch_block1(st, b1, T, L.ci, tan ? B1_TBWD_WGRAD : B1_BWD_WGRAD, &blk));
      if (adv) adv_add_seg(adv, L.off_w, 9 * L.ci * L.co, pl.wgpart, blk);
      else LAUNCH(e, st, OP_WGRAD_REDUCE, 0, launch_wgrad_reduce(st, pl.wgpart, blk, 9 * L.ci * L.co, T, g + L.off_w, P));
      continue;
    }
    BnArgs ba = bn_args(e, A, tan, l, n, theta);
    ba.partial = pl.bnpart;
    int blk = 0;
    const bool bn_done = last_bn_done && l == nl - 1;
    if (!red_done[l] && !bn_done) {
      ba.fin = fin_of(e, T, 1.0, FIN_SUMS, g + L.off_gamma, P, g + L.off_beta, P);
      LAUNCH(e, st, op_red, l, tan ? launch_bn_tan_bwd_reduce(st, ba, T, L.pool, &blk) : launch_bn_bwd_reduce(st, ba, T, L.pool, &blk));
      if (!ba.fin.counter)
        LAUNCH(e, st, OP_BN_FINALIZE, l, launch_bn_finalize(st, pl.bnpart, blk, T, L.co, 1.0, FIN_SUMS, g + L.off_gamma, P, g + L.off_beta, P));
    }
    if (tan) { ba.rdgamma = g + L.off_gamma; ba.rdbeta = g + L.off_beta; ba.hstride = P; }
    else { ba.dgamma = g + L.off_gamma; ba.dbeta = g + L.off_beta; ba.gstride = P; }
    float* dz = tan ? tan->X.rdz[l] : A.dz[l];      // dz, or R{dz}
    ba.out = dz;
    ba.amax_out = cell_bind(e, pl, ba.out);
    LAUNCH(e, st, op_apply, l, tan ? launch_bn_tan_bwd_apply(st, ba, T, L.pool) : launch_bn_bwd_apply(st, ba, T, L.pool));
    WgradArgs wa{};
    wa.x[0] = l == 0 ? x0 : A.p[l - 1];
    wa.dz[0] = dz;
    if (tan && l > 0) { wa.x[1] = tan->X.pd[l - 1]; wa.dz[1] = A.dz[l]; }
    if (l >= 1) {
      CELL(wa.x[0], (size_t)n * L.h * L.w * L.ci, wa.amax_x[0]);
      CELL(wa.dz[0], (size_t)n * L.ho * L.wo * L.co, wa.amax_dz[0]);
      if (tan) {
        CELL(wa.x[1], (size_t)n * L.h * L.w * L.ci, wa.amax_x[1]);
        CELL(wa.dz[1], (size_t)n * L.ho * L.wo * L.co, wa.amax_dz[1]);
      }
    }
    wa.g = geom(L, n);
    wa.mpix = mpix;
    // The weight gradients of the hidden blocks run on the side stream beside the dgrad chain, one fork per block.  Every fork is an event
    // record on the caller's stream, which idles it for ~7 us (tools/launch_floor.py: 25 such gaps per meta-iteration, at every task
    // count; profiles/r5/launch_floor_cfg2_T*.txt).
    hipStream_t ws = l > 0 ? side_fork(e, st, pl.half) : st;
    if (ws != st) forked = true;
    const int rc = issue_wgrad(ws, wa, l);
    if (rc) return rc;
    if (l > 0) {
      ConvArgs ca{};
      ca.in[0] = dz; ca.wt[0] = theta + L.off_w; ca.amax[0] = wa.amax_dz[0];
      if (tan) { ca.in[1] = A.dz[l]; ca.wt[1] = tan->v + L.off_w; ca.amax[1] = wa.amax_dz[1]; }
      ca.wstride = P;
      ca.out = tan ? tan->X.dpd[tan->cur ^ 1] : A.dp[l - 1];
      ca.g = geom_dgrad(L, n);
      ca.mpix = n * L.h * L.w;
      const int nterms = tan ? 2 : 1;
      const float* zh_lo = dgrad_carries_reduce(e, l) ? zh_at_argmax(e, A, l - 1) : nullptr;
      const float* zhd_lo = !tan ? nullptr : (l - 1 == 0 && e->fuse1) ? tan->X.zhdm : tan->X.zhdl[l - 1];
      if (zh_lo && (!tan || zhd_lo)) {   // dgamma / dbeta (or their tangents) of the block below in this kernel's epilogue
        const Layer& L0 = e->L[l - 1];
        ca.bp = A.p[l - 1]; ca.bzh = zh_lo; ca.partial = pl.bnpart;
        if (tan) { ca.bzhd = zhd_lo; ca.bdp = A.dp[l - 1]; }
        ca.barg = (l - 1 == 0 && e->fuse1) ? A.arg0 : nullptr;   // block 1's argmax byte replaces the read of p
        ca.fin = fin_of(e, T, 1.0, FIN_SUMS, g + L0.off_gamma, P, g + L0.off_beta, P);
        int blk0 = 0;
        LAUNCH(e, st, op_dgrad, l, launch_conv3x3(st, ca, T, nterms, EPI_BRED, 1, &blk0));
        if (!ca.fin.counter)
          LAUNCH(e, st, OP_BN_FINALIZE, l - 1, launch_bn_finalize(st, pl.bnpart, blk0, T, L0.co, 1.0, FIN_SUMS, g + L0.off_gamma, P, g + L0.off_beta, P));
        red_done[l - 1] = true;
      } else {
        LAUNCH(e, st, op_dgrad, l, launch_conv3x3(st, ca, T, nterms, EPI_NONE, 1, nullptr));
      }
      if (tan) tan->cur ^= 1;
    }
  }
  return side_join(e, st, pl.half, forked);
}

// Linear + CE on features f [T][n][feat]: loss/acc/logits, prob & dl saved, and (with_grad) dwl/dbl into g, df.
static int head_pass(mi_engine* e, hipStream_t st, float* hscr, const float* f, const int32_t* y, int n, int T, const float* theta,
                     float* g, float* loss, float* acc, float* logits, float* prob, float* dl, float* df, bool with_grad) {
  const HeadArgs ha = head_args_primal(e, hscr, f, y, n, T, theta, g, loss, acc, logits, prob, dl, df, with_grad);
  if (with_grad) HEAD_LDS(e, "head", n, ha.ways, 0);
  LAUNCH(e, st, OP_HEAD, 0, launch_head_fwd_bwd(st, ha, T, with_grad ? 1 : 0));
  return MI_OK;
}

// mi_engine_set_bn_export: batch mean / biased variance of every block of the pass just run, into slot e->export_pass
static int export_bn_stats(mi_engine* e, hipStream_t st, const ActSet& A, int T) {
  if (!e->bn_export) return MI_OK;
  const int nl = (int)e->L.size();
  int ctot = 0;
  for (const Layer& L : e->L) ctot += L.co;
  const size_t need = (size_t)(e->export_pass + 1) * T * 2 * ctot;
  if (need > e->bn_export_floats) return fail(e, MI_ERR_WORKSPACE, "BatchNorm export buffer too small: need " + std::to_string(need) + " floats");
  BnExportArgs ea{};
  ea.nl = nl; ea.ctot = ctot;
  int off = 0;
  for (int l = 0; l < nl; ++l) { ea.mu[l] = A.mu[l]; ea.rstd[l] = A.rstd[l]; ea.c[l] = e->L[l].co; ea.off[l] = off; off += e->L[l].co; }
  ea.out = e->bn_export + (size_t)e->export_pass * T * 2 * ctot;
  HIPCHK(e, launch_bn_export(st, ea, T));
  e->export_pass += 1;
  return MI_OK;
}

// The BatchNorm export covers the fused calls only (mi_meta_batch_maml / mi_meta_batch_anil number their passes from 0): the
// step-wise entry points run with the export paused, so a learner(x) inside an export window neither writes a stale slot nor
// fails on the buffer size.
struct ExportPause {
  mi_engine* e; float* buf;
  explicit ExportPause(mi_engine* e_) : e(e_), buf(e_ ? e_->bn_export : nullptr) { if (e) e->bn_export = nullptr; }
  ~ExportPause() { if (e) e->bn_export = buf; }
};

// One forward (+ backward) pass of the whole net on n images per task.
// Tb: tasks that take the backward half (the first Tb of the T; -1 = all): the validation tasks of a fused train + validation call
// run the forward half only.  adv: fused tail (trunk_backward); the caller's advance launch then also zeroes what no kernel writes.
static int pass_fwd_bwd(mi_engine* e, hipStream_t st, Plan& pl, ActSet& A, const float* x0, const int32_t* y, int n, int T,
                        const float* theta, float* g, float* loss, float* acc, float* logits, bool with_grad,
                        const double* gram = nullptr, AdvanceArgs* adv = nullptr, bool stats_ready = false, int Tb = -1) {
  const int nl = (int)e->L.size();
  if (Tb < 0) Tb = T;
  const bool fused_last = fused_last_ok(e, pl, n, T);
  int rc = trunk_forward(e, st, pl, A, x0, n, T, theta, gram, stats_ready, fused_last);
  if (rc) return rc;
  rc = export_bn_stats(e, st, A, T);
  if (rc) return rc;
  if (e->d.head_mean_pool) HIPCHK(e, launch_spatial_mean(st, A.p[nl - 1], A.f, T * n, e->head_hw, e->head_c));
  if (with_grad && !adv) HIPCHK(e, hipMemsetAsync(g, 0, (size_t)T * e->PS * sizeof(float), st));
  if (fused_last) {   // the last block's BatchNorm + pooling, the head, its backward and that block's BatchNorm backward: one launch (tail.hip)
    const HeadArgs ha = head_args_primal(e, pl.hscr, A.f, y, n, T, theta, g, loss, acc, logits, A.prob, A.dl, A.df, with_grad);
    const TailArgs ta = tail_args(e, pl, A, nullptr, ha, n, theta, g, with_grad, Tb);
    LAUNCH(e, st, OP_HEAD, 0, launch_tail(st, ta, T, e->L[nl - 1].pool, 0));
    if (!with_grad || Tb == 0) return MI_OK;
    return trunk_backward(e, st, pl, A, x0, n, Tb, theta, g, gram, adv, true);
  }
  rc = head_pass(e, st, pl.hscr, A.f, y, n, T, theta, g, loss, acc, logits, A.prob, A.dl, A.df, with_grad);
  if (rc || !with_grad || Tb == 0) return rc;
  if (e->d.head_mean_pool) HIPCHK(e, launch_spatial_mean_bwd(st, A.df, A.dp[nl - 1], Tb * n, e->head_hw, e->head_c));
  return trunk_backward(e, st, pl, A, x0, n, Tb, theta, g, gram, adv);
}

// hv = H(theta) v for the saved support pass A (activations) / g (its gradient): forward-over-reverse.
// dl_fixed != nullptr: the loss is sum(logits * dl_fixed) with a GIVEN cotangent (the step-wise learner's double backward): no
// cross-entropy curvature at the head, and the logit tangents J v go to ld_out.
static int pass_hvp(mi_engine* e, hipStream_t st, Plan& pl, ActSet& A, const float* x0, int n, int T, const float* theta,
                    const float* g, const float* v, float* hv, const double* gram = nullptr, const float* dl_fixed = nullptr,
                    float* ld_out = nullptr, AdvanceArgs* adv = nullptr, bool stats_ready = false) {
  const int nl = (int)e->L.size();
  TanSet& X = pl.tan;
  Tangent tan{v, g, hv, X};
  const bool fused_last = !dl_fixed && !ld_out && fused_last_ok(e, pl, n, T);   // tangent tail in one launch (tail.hip)
  if (!adv) HIPCHK(e, hipMemsetAsync(hv, 0, (size_t)T * e->PS * sizeof(float), st));
  const int rc = trunk_forward(e, st, pl, A, x0, n, T, theta, gram, stats_ready, fused_last, &tan);
  if (rc) return rc;
  const float* fd = X.pd[nl - 1];
  if (e->d.head_mean_pool) {
    HIPCHK(e, launch_spatial_mean(st, X.pd[nl - 1], X.fd, T * n, e->head_hw, e->head_c));
    fd = X.fd;
  }
  HeadArgs ha = head_args(e, pl.hscr, A.f, theta, v, hv, e->d.head_mean_pool ? X.rdf : X.dpd[tan.cur], n, T);
  ha.fd = fd;
  ha.prob = A.prob; ha.dl = A.dl;
  if (dl_fixed) { ha.dl = const_cast<float*>(dl_fixed); ha.fixed_dl = 1; ha.ld_out = ld_out; }
  if (fused_last) {   // tangent of the last block's BatchNorm + pooling, the head's tangent and the tangent of that block's BatchNorm backward
    const TailArgs ta = tail_args(e, pl, A, &tan, ha, n, theta, hv, true, T);
    LAUNCH(e, st, OP_HEAD_TAN, 0, launch_tail(st, ta, T, e->L[nl - 1].pool, 1));
  } else {
    HEAD_LDS(e, "head tangent", n, ha.ways, 1);
    LAUNCH(e, st, OP_HEAD_TAN, 0, launch_head_tangent(st, ha, T));
  }
  if (e->d.head_mean_pool) HIPCHK(e, launch_spatial_mean_bwd(st, X.rdf, X.dpd[tan.cur], T * n, e->head_hw, e->head_c));
  return trunk_backward(e, st, pl, A, x0, n, T, theta, hv, gram, adv, fused_last, &tan);
}

// The part of an advance launch that does not depend on the pass: sizes, strides, the never-written elements, block 1's geometry.
static AdvanceArgs advance_base(const mi_engine* e, float* g) {
  AdvanceArgs a{};
  a.g = g; a.gstride = e->PS; a.ostride = e->PS; a.n = (unsigned)e->PS;
  a.nzero = e->nzero;
  for (int z = 0; z < e->nzero; ++z) { a.zoff[z] = e->zoff[z]; a.zlen[z] = e->zlen[z]; }
  a.off_w1 = (unsigned)e->L[0].off_w;
  a.ci = (e->L[0].ci == 1 || e->L[0].ci == 3) ? e->L[0].ci : 0;
  a.co = e->L[0].co;
  a.counter = e->counters;
  return a;
}

// One fused call as the entry points receive it: what mi_meta_batch_maml / _tv / _lr / _anil fill from their arguments and hand through the
// graph cache (meta_batch_entry) to the implementation.  grad_tasks = 0: evaluation only (the with_grad flag of mi_meta_batch_maml and
// mi_meta_batch_anil is grad_tasks = tasks or 0).  lr_vec == nullptr: the scalar step inner_lr; else the step sizes on the device.
// ALGO_MAML_STEPS (mi_meta_batch_maml_steps): step_w = the K weights of the multi-step loss on the device, and loss_out / acc_out / logits_out
// are the per-step outputs, row j of K + 1 holding what the plain call writes for theta_j.  lr_vec may be null (scalar step) or not.
// ALGO_ANIL_LR / ALGO_ANIL_STEPS (mi_meta_batch_anil_lr / _steps): the same fields read by meta_batch_anil_impl; lr_vec and lr_grad_out are
// [lr_steps][Ph] (the head's entries only), grad_tasks is tasks or 0.
// ALGO_MAML_OFFSETS (mi_meta_batch_maml_offsets): offsets = the [adapt_steps][P] per-step parameter offsets on the device, offsets_grad_out
// their gradient or null; step_w null: the plain call's outputs and objective, else the steps call's; lr_vec null or not as in the steps call.
// ALGO_METRIC (mi_meta_batch_metric): the ANIL call's trunk pass with a closed-form head (metric, scale) and no inner loop; adapt_steps = 0,
// grad_tasks is tasks or 0.
enum MetaAlgo { ALGO_MAML = 0, ALGO_ANIL = 1, ALGO_MAML_LR = 2, ALGO_MAML_STEPS = 3, ALGO_ANIL_LR = 4, ALGO_ANIL_STEPS = 5, ALGO_MAML_OFFSETS = 6,
                ALGO_METRIC = 7, ALGO_RIDGE = 8, ALGO_ANIL_PROTO = 9, ALGO_LOGREG = 10 };
// ALGO_RIDGE (mi_meta_batch_ridge): ALGO_METRIC's launches with the ridge-regression head (lam, alpha) in the metric head's place;
// dhyper_out [tasks][2] or null.  ALGO_LOGREG (mi_meta_batch_logreg): the same with the logistic-regression head's launch.
// ALGO_ANIL_PROTO (mi_meta_batch_anil_proto): ALGO_ANIL_LR / _STEPS' fields read by meta_batch_anil_impl, theta_0's head derived per task from
// the support prototypes with `scale` (proto_init.hip); lr_vec and step_w each null or not, dhyper_out [tasks] (d objective_t / d scale) or null.
static bool is_anil(MetaAlgo a) { return a == ALGO_ANIL || a == ALGO_ANIL_LR || a == ALGO_ANIL_STEPS || a == ALGO_ANIL_PROTO; }
static bool is_closed_form(MetaAlgo a) { return a == ALGO_METRIC || a == ALGO_RIDGE || a == ALGO_LOGREG; }
struct MetaCall {
  MetaAlgo algo;
  const float* theta; const float* data; const int64_t* labels;
  int tasks, grad_tasks, ways, shots, adapt_steps, second_order;
  float inner_lr;
  const float* lr_vec; int lr_steps; float* lr_grad_out;
  float *loss_out, *acc_out, *meta_grad_out, *logits_out;
  void* workspace; size_t workspace_bytes;
  const float* step_w = nullptr;
  const float* offsets = nullptr; float* offsets_grad_out = nullptr;
  int metric = 0; float scale = 0.f;
  float lam = 0.f, alpha = 0.f; float* dhyper_out = nullptr;
};

// Every check of a fused call that needs no plan: before the graph cache and before any HIP call.
static int check_call(mi_engine* e, const MetaCall& c) {
  if (!e) return fail(nullptr, MI_ERR_ARG, "null engine");
  if (c.grad_tasks < 0 || c.grad_tasks > c.tasks) return fail(e, MI_ERR_ARG, "grad_tasks must be in 0..tasks");
  if (c.algo == ALGO_MAML_STEPS) {
    if (c.adapt_steps < 1) return fail(e, MI_ERR_ARG, "mi_meta_batch_maml_steps needs adapt_steps >= 1: its weights are those of theta_1 .. theta_K");
    if (!c.step_w) return fail(e, MI_ERR_ARG, "step_w is NULL: mi_meta_batch_maml_steps takes adapt_steps weights on the device");
    if (e->trace) return fail(e, MI_ERR_ARG, "the debug trace does not cover mi_meta_batch_maml_steps");
    if (!c.lr_vec && c.lr_grad_out) return fail(e, MI_ERR_ARG, "lr_grad_out given without lr_vec");
  }
  if (c.algo == ALGO_MAML_OFFSETS) {
    if (c.adapt_steps < 1) return fail(e, MI_ERR_ARG, "mi_meta_batch_maml_offsets needs adapt_steps >= 1: row k of the offsets is added to theta_{k+1}");
    if (!c.offsets) return fail(e, MI_ERR_ARG, "offsets is NULL: mi_meta_batch_maml_offsets takes adapt_steps * P offsets on the device");
    if (c.offsets_grad_out && c.grad_tasks == 0)
      return fail(e, MI_ERR_ARG, "offsets_grad_out given but grad_tasks = 0: the offset gradient is summed over the train tasks");
    if (e->trace) return fail(e, MI_ERR_ARG, "the debug trace does not cover mi_meta_batch_maml_offsets");
    if (!c.lr_vec && c.lr_grad_out) return fail(e, MI_ERR_ARG, "lr_grad_out given without lr_vec");
  } else if (c.offsets || c.offsets_grad_out) {
    return fail(e, MI_ERR_ARG, "per-step offsets are taken by mi_meta_batch_maml_offsets only");
  }
  if (c.algo == ALGO_MAML_LR || ((c.algo == ALGO_MAML_STEPS || c.algo == ALGO_MAML_OFFSETS) && c.lr_vec)) {
    if (!lr_steps_ok(c.lr_steps, c.adapt_steps))
      return fail(e, MI_ERR_ARG, "lr_steps = " + std::to_string(c.lr_steps) + " must be 1 or adapt_steps = " + std::to_string(c.adapt_steps) +
                                     (c.adapt_steps == 0 ? " (without inner steps: 1)" : ""));
    if (!c.lr_vec) return fail(e, MI_ERR_ARG, "lr_vec is NULL: mi_meta_batch_maml_lr takes lr_steps * P step sizes on the device");
    if (c.lr_grad_out && c.grad_tasks == 0)
      return fail(e, MI_ERR_ARG, "lr_grad_out given but grad_tasks = 0: the step-size gradient is summed over the train tasks");
  }
  if (c.algo == ALGO_ANIL_STEPS) {
    if (c.adapt_steps < 1)
      return fail(e, MI_ERR_ARG, "mi_meta_batch_anil_steps needs adapt_steps >= 1, got " + std::to_string(c.adapt_steps) + ": its weights are those of theta_1 .. theta_K");
    if (!c.step_w) return fail(e, MI_ERR_ARG, "step_w is NULL: mi_meta_batch_anil_steps takes adapt_steps weights on the device");
    if (!c.lr_vec && c.lr_grad_out) return fail(e, MI_ERR_ARG, "mi_meta_batch_anil_steps: lr_grad_out given without lr_vec");
  }
  if (c.algo == ALGO_ANIL_PROTO) {
    const char* who = "mi_meta_batch_anil_proto";
    if (!(c.scale > 0.f) || !std::isfinite(c.scale))
      return fail(e, MI_ERR_ARG, std::string(who) + ": scale must be positive and finite, got " + std::to_string(c.scale));
    if (c.dhyper_out && c.grad_tasks == 0)
      return fail(e, MI_ERR_ARG, std::string(who) + ": dscale_out given but with_grad = 0: the scale's gradient comes with the meta-gradient");
    if (c.step_w && c.adapt_steps < 1)
      return fail(e, MI_ERR_ARG, std::string(who) + ": step_w needs adapt_steps >= 1, got " + std::to_string(c.adapt_steps) + ": its weights are those of theta_1 .. theta_K");
    if (!c.lr_vec && c.lr_grad_out) return fail(e, MI_ERR_ARG, std::string(who) + ": lr_grad_out given without lr_vec");
  }
  if (c.algo == ALGO_ANIL_LR || c.algo == ALGO_ANIL_STEPS || c.algo == ALGO_ANIL_PROTO) {
    const char* who = c.algo == ALGO_ANIL_LR ? "mi_meta_batch_anil_lr" : c.algo == ALGO_ANIL_STEPS ? "mi_meta_batch_anil_steps" : "mi_meta_batch_anil_proto";
    if (e->trace) return fail(e, MI_ERR_ARG, std::string("the debug trace does not cover ") + who);
    if (c.algo == ALGO_ANIL_LR && !c.lr_vec)
      return fail(e, MI_ERR_ARG, "lr_vec is NULL: mi_meta_batch_anil_lr takes lr_steps * (ways * fc + ways) step sizes on the device");
    if (c.lr_vec) {
      if (!lr_steps_ok(c.lr_steps, c.adapt_steps))
        return fail(e, MI_ERR_ARG, std::string(who) + ": lr_steps = " + std::to_string(c.lr_steps) + " must be 1 or adapt_steps = " +
                                       std::to_string(c.adapt_steps) + (c.adapt_steps == 0 ? " (without inner steps: 1)" : ""));
      if (c.lr_grad_out && c.grad_tasks == 0)
        return fail(e, MI_ERR_ARG, std::string(who) + ": lr_grad_out given but with_grad = 0: the step-size gradient comes with the meta-gradient");
    }
    if (c.ways == e->d.ways && c.shots >= 1) {      // (the plain call meets these limits at the launch; here they come first)
      const int n = c.ways * c.shots;
      if (c.adapt_steps > 0 || c.grad_tasks > 0) HEAD_LDS(e, who, n, c.ways, 0);
      if (c.adapt_steps > 0 && c.grad_tasks > 0 && c.second_order) HEAD_LDS(e, who, n, c.ways, 1);
      if (c.algo == ALGO_ANIL_PROTO && c.tasks >= 1 && !proto_init_fits(c.tasks, n, e->feat, c.ways)) return proto_init_size_fail(e, who, c.tasks, n, e->feat, c.ways);
    }
  }
  const int cf_head = c.algo == ALGO_LOGREG ? CF_LOGREG : c.algo == ALGO_RIDGE ? CF_RIDGE : CF_METRIC;
  const char* cf_who = cf_head == CF_LOGREG ? "mi_meta_batch_logreg" : cf_head == CF_RIDGE ? "mi_meta_batch_ridge" : "mi_meta_batch_metric";
  if (is_closed_form(c.algo)) {
    const int hrc = cf_head != CF_METRIC ? ridge_hyper_check(e, cf_who, c.lam, c.alpha) : metric_hyper_check(e, cf_who, c.metric, c.scale);
    if (hrc) return hrc;
    if (e->trace) return fail(e, MI_ERR_ARG, std::string("the debug trace does not cover ") + cf_who);
  }
  if (!c.theta || !c.data || !c.labels || !c.loss_out || !c.acc_out || !c.workspace) return fail(e, MI_ERR_ARG, "null pointer argument");
  if (c.grad_tasks > 0 && !c.meta_grad_out) return fail(e, MI_ERR_ARG, "meta_grad_out is NULL but a gradient was asked for");
  if ((is_anil(c.algo) || is_closed_form(c.algo)) && e->d.head_mean_pool)
    return fail(e, MI_ERR_ARG, "ANIL features are flattened (view(-1, fc_neurons)), not mean-pooled");
  if (c.tasks < 1 || c.shots < 1 || c.adapt_steps < 0) return fail(e, MI_ERR_ARG, "tasks/shots must be >= 1, adapt_steps >= 0");
  if (c.ways != e->d.ways) return fail(e, MI_ERR_ARG, "ways differs from the engine's classifier width");
  if (is_closed_form(c.algo)) return closed_form_lds_check(e, cf_who, cf_head, c.ways * c.shots, c.ways * c.shots, e->feat, c.ways);   // (after ways and shots)
  return MI_OK;
}

// grad_tasks: the first grad_tasks of the `tasks` tasks are TRAIN tasks (query backward, second-order adjoint recursion, summed into
// meta_grad_out); the rest are VALIDATION tasks of the same meta-iteration (reference maml_vision.py:117-124: the same clone +
// fast_adapt without backward), whose K support steps and query forward run in the SAME launches as the train tasks'.
// c.lr_vec != nullptr (mi_meta_batch_maml_lr): one step size per parameter, D_k = diag(lr_k), lr_k = row (lr_steps == 1 ? 0 : k) of lr_vec:
//   theta_{k+1} = theta_k - D_k g_k;   lam_k = lam_{k+1} - H_k (D_k lam_{k+1});   lr_grad_k = -sum_t g_k * lam_{k+1}
// The Hessian-vector pass over support step k is driven with dir = D_k lam_{k+1} (block 1's tangent statistics included) and the update is
// lam_k = lam_{k+1} - 1 * H dir.  c.lr_vec == nullptr: the scalar call, the same launches and arithmetic as before.
static int meta_batch_maml_impl(mi_engine* e, void* stream, const MetaCall& c) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int T = c.tasks, Tg = c.grad_tasks, K = c.adapt_steps, with_grad = Tg > 0, so = (c.second_order && with_grad) ? 1 : 0;
  const float inner_lr = c.inner_lr;
  e->export_pass = 0;
  Plan pl;
  const bool msl = c.algo == ALGO_MAML_STEPS || (c.algo == ALGO_MAML_OFFSETS && c.step_w);      // query passes at every theta_j, the multi-step loss's terms in the adjoint recursion
  const int prc = plan_in(e, c.workspace, c.workspace_bytes,
                          c.offsets ? offsets_shape(T, Tg, c.ways, c.shots, K, so, c.lr_vec ? c.lr_steps : 0, c.lr_grad_out != nullptr, msl) :
                          msl ? steps_shape(T, Tg, c.ways, c.shots, K, so, c.lr_vec ? c.lr_steps : 0, c.lr_grad_out != nullptr)
                              : maml_shape(T, c.ways, c.shots, K, so, c.lr_vec ? c.lr_steps : 0, c.lr_grad_out != nullptr), pl);
  if (prc) return prc;
  const int ns = c.ways * c.shots, nq = ns;
  const size_t TP = (size_t)T * e->PS;
  const Layer& L0 = e->L[0];
  const bool tail = e->fuse_tail && e->counters && T <= 65535 /* launch_advance puts the tasks on grid.y */ && T <= mi_engine::kMaxCounterTasks && 1024 % L0.co == 0;
  const double inv_m0 = 1.0 / ((double)ns * L0.ho * L0.wo);
  { const int brc = plan_begin(e, st, pl); if (brc) return brc; }
  LAUNCH(e, st, OP_MISC, 0, launch_prepare_batch(st, c.data, c.labels, T, 2 * ns, e->d.in_channels, e->d.in_h, e->d.in_w, pl.xs, pl.xq, pl.ys, pl.yq));
  LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, c.theta, 0, e->perm_dev, (int)e->P, (int)e->PS, T, pl.theta));
  // the step sizes in engine layout, once per call (padding entries zero): row k of lr_of is D_k
  if (c.lr_vec) LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, c.lr_vec, e->P, e->perm_dev, (int)e->P, (int)e->PS, c.lr_steps, pl.lrv));
  auto lr_of = [&](int k) { return pl.lrv + (c.lr_steps == 1 ? 0 : (size_t)k * e->PS); };
  // the per-step offsets in engine layout, once per call (padding entries zero): row k is s_{k+1}, added to theta_{k+1}
  if (c.offsets) LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, c.offsets, e->P, e->perm_dev, (int)e->P, (int)e->PS, K, pl.ofs));
  if (pl.gram_s)
    LAUNCH(e, st, OP_GRAM, 0, launch_input_gram(st, pl.xs, T, ns, e->L[0].h, e->L[0].w, e->L[0].ci, pl.gram_part, pl.gram_s));
  const double* gq = pl.gram_q;          // (also for forward-only calls and tasks: the same query forward whether or not a backward half follows)
  bool gq_side = false, gq_launched = false;
  if (gq && msl) {          // needed at once: theta_0 is scored before the first support pass
    LAUNCH(e, st, OP_GRAM, 0, launch_input_gram(st, pl.xq, T, nq, e->L[0].h, e->L[0].w, e->L[0].ci, pl.gram_part_q, pl.gram_q));
    gq_launched = true;
  } else if (gq && e->overlap) {   // the query images' Gram matrix beside the inner loop (on `st` if the side stream cannot be had)
    hipStream_t ws = side_fork(e, st, pl.half);
    gq_side = ws != st;
    LAUNCH(e, ws, OP_GRAM, 0, launch_input_gram(ws, pl.xq, T, nq, e->L[0].h, e->L[0].w, e->L[0].ci, pl.gram_part_q, pl.gram_q));
    gq_launched = true;
  }
  const bool stats0 = tail && pl.gram_s && K > 0;
  if (stats0) {   // block 1's statistics of the first support pass, from theta_0 (nothing folded, nothing written)
    AdvanceArgs a0 = advance_base(e, pl.theta);
    a0.nzero = 0;
    a0.stats = 1; a0.gram = pl.gram_s; a0.out0 = pl.sup[0].mu[0]; a0.out1 = pl.sup[0].rstd[0]; a0.inv_m = inv_m0;
    LAUNCH(e, st, OP_MISC, 2, launch_advance(st, a0, T));
  }
  // The steps call: the query set at theta_j, j < K, with the launches of the final query pass below and the same activation set; train tasks
  // take the backward half for j >= 1 and leave q_j finished in pl.qg[j - 1].  No BatchNorm export: the call exports the passes the plain call does.
  const size_t TL = (size_t)T * nq * c.ways;
  auto query_at = [&](int j) -> int {
    const bool bwd = with_grad && j >= 1;
    float* qj = bwd ? pl.qg + (size_t)(j - 1) * TP : pl.lam;
    AdvanceArgs aq = advance_base(e, qj);
    ExportPause pause(e);
    const int qrc = pass_fwd_bwd(e, st, pl, pl.qry, pl.xq, pl.yq, nq, T, pl.theta + (size_t)j * TP, qj, c.loss_out + (size_t)j * T, c.acc_out + (size_t)j * T,
                                 c.logits_out ? c.logits_out + (size_t)j * TL : nullptr, bwd, gq, (tail && bwd) ? &aq : nullptr, false, Tg);
    if (qrc) return qrc;
    if (tail && bwd) LAUNCH(e, st, OP_MISC, 2, launch_advance(st, aq, Tg));
    return MI_OK;
  };
  for (int k = 0; k < K; ++k) {
    if (msl) { const int qrc = query_at(k); if (qrc) return qrc; }
    ActSet& A = so ? pl.sup[k] : pl.sup[0];
    float* th = pl.theta + (size_t)k * TP;
    float* gk = pl.g + (size_t)k * TP;
    AdvanceArgs adv = advance_base(e, gk);
    int rc = pass_fwd_bwd(e, st, pl, A, pl.xs, pl.ys, ns, T, th, gk, pl.tmp_loss, pl.tmp_acc, nullptr, true, pl.gram_s, tail ? &adv : nullptr,
                          tail && pl.gram_s);
    if (rc) return rc;
    if (tail) {   // g_k finished, theta_{k+1} = theta_k - lr g_k, and block 1's statistics of the next support pass
      adv.a = th; adv.out = th + TP; adv.alpha = inner_lr;
      if (c.lr_vec) adv.lr = lr_of(k);
      if (c.offsets) adv.ofs = pl.ofs + (size_t)k * e->PS;      // theta_{k+1} = (theta_k - D_k g_k) + s_{k+1}, the statistics from the shifted weights
      if (pl.gram_s && k + 1 < K) {
        ActSet& An = so ? pl.sup[k + 1] : pl.sup[0];
        adv.stats = 1; adv.gram = pl.gram_s; adv.out0 = An.mu[0]; adv.out1 = An.rstd[0]; adv.inv_m = inv_m0;
      }
      LAUNCH(e, st, OP_MISC, 2, launch_advance(st, adv, T));
    } else if (c.lr_vec) {
      LAUNCH(e, st, OP_MISC, 2, launch_axpy_vec(st, th, gk, lr_of(k), (int)e->PS, T, th + TP));
    } else {
      LAUNCH(e, st, OP_MISC, 2, launch_axpy(st, th, gk, inner_lr, TP, th + TP));
    }
    if (c.offsets && !tail) LAUNCH(e, st, OP_MISC, 2, launch_add_offsets(st, th + TP, pl.ofs + (size_t)k * e->PS, (int)e->PS, T));
  }
  float* thK = pl.theta + (size_t)K * TP;
  // the steps call with the fused tail: q_K is finished in pl.qg[K - 1] and lam_K = w_K q_K goes to pl.lam (AdvanceArgs::inj_w); without it the
  // pass writes pl.lam and one elementwise launch scales it
  const bool msl_adv = msl && tail && with_grad;
  float* gK = msl_adv ? pl.qg + (size_t)(K - 1) * TP : pl.lam;
  AdvanceArgs advq = advance_base(e, gK);
  if (msl_adv) { advq.out = pl.lam; advq.inj_w = c.step_w + (K - 1); }
  float *loss_K = c.loss_out, *acc_K = c.acc_out, *logits_K = c.logits_out;
  if (msl) { loss_K += (size_t)K * T; acc_K += (size_t)K * T; if (logits_K) logits_K += (size_t)K * TL; }
  if (gq_side) { const int jrc = side_join(e, st, pl.half, true); if (jrc) return jrc; }
  else if (gq && !gq_launched) LAUNCH(e, st, OP_GRAM, 0, launch_input_gram(st, pl.xq, T, nq, e->L[0].h, e->L[0].w, e->L[0].ci, pl.gram_part_q, pl.gram_q));
  int rc = pass_fwd_bwd(e, st, pl, pl.qry, pl.xq, pl.yq, nq, T, thK, gK, loss_K, acc_K, logits_K, with_grad != 0, gq,
                        (tail && with_grad) ? &advq : nullptr, false, Tg);
  if (rc) return rc;
  if (!with_grad) return MI_OK;
  if (msl && !tail) LAUNCH(e, st, OP_MISC, 2, launch_scale_dev(st, pl.lam, c.step_w + (K - 1), (size_t)Tg * e->PS));
  // debug trace layout (floats): theta [K+1][T][P] | g [K][T][P] | lam_in [K][T][P] | hv [K][T][P], reference parameter order
  const size_t TPr = (size_t)T * e->P;
  const bool tr = e->trace && e->trace_floats >= (size_t)(4 * K + 1) * TPr;
  if (e->trace && !tr) return fail(e, MI_ERR_WORKSPACE, "debug trace buffer too small: need " + std::to_string((size_t)(4 * K + 1) * TPr) + " floats");
  if (tr && Tg != T) return fail(e, MI_ERR_ARG, "the debug trace covers calls whose tasks all take the backward half");
  // tangent statistics of block 1 for the Hessian-vector pass over support pass k (weights theta_k), direction = the finished vector
  auto tangent_stats = [&](AdvanceArgs& a, int k) {
    a.stats = 2; a.gram = pl.gram_s; a.sw = pl.theta + (size_t)k * TP + L0.off_w; a.swstride = e->PS;
    a.mu_in = pl.sup[k].mu[0]; a.rstd_in = pl.sup[k].rstd[0]; a.out0 = pl.tan.m1[0]; a.out1 = pl.tan.m2[0]; a.inv_m = inv_m0;
  };
  // vector form: the launch that finishes lam_{k+1} also leaves dir = D_k lam_{k+1} (the direction of the Hessian-vector pass over support
  // step k, into the buffer the pass that has just run was NOT driven with) and the products g_k * lam_{k+1}
  float *dir_cur = pl.dir, *dir_nxt = pl.dir2;
  auto vector_extras = [&](AdvanceArgs& a, int k) {
    a.dlr = lr_of(k); a.dir = dir_nxt;
    if (pl.prod) { a.dg = pl.g + (size_t)k * TP; a.prod = pl.prod + (size_t)k * TP; }
    float* t = dir_cur; dir_cur = dir_nxt; dir_nxt = t;
  };
  if (tail) {   // lam = grad L_query(theta_K) finished (folds only)
    if (so && K > 0 && pl.gram_s) tangent_stats(advq, K - 1);
    if (c.lr_vec && so && K > 0) vector_extras(advq, K - 1);
    LAUNCH(e, st, OP_MISC, 2, launch_advance(st, advq, Tg));
  }
  float *lam_cur = pl.lam, *lam_nxt = pl.lam2;
  // offsets_grad[k] = sum_t lam_{k+1}: the offset is additive, so the recursion is unchanged and each complete lam_{k+1} (its w_{k+1} q_{k+1}
  // in) is folded where it stands, before the pass that consumes it
  auto ofs_fold = [&](const float* lam, int k) -> hipError_t {
    return launch_offsets_grad_fold(st, lam, 0, e->perm_dev, (int)e->P, (int)e->PS, Tg, 1, c.offsets_grad_out + (size_t)k * e->P);
  };
  if (so) {
    for (int k = K - 1; k >= 0; --k) {
      if (c.offsets_grad_out) LAUNCH(e, st, OP_MISC, 3, ofs_fold(lam_cur, k));
      if (tr) HIPCHK(e, launch_scatter_tasks(st, lam_cur, e->perm_dev, (int)e->P, (int)e->PS, T, e->trace + (size_t)(2 * K + 1 + k) * TPr));
      if (c.lr_vec && !tail) {   // the separate launches of the vector form: dir = D_k lam, the products; below lam -= 1 * H dir
        LAUNCH(e, st, OP_MISC, 2, launch_scale_vec(st, lam_cur, lr_of(k), (int)e->PS, Tg, dir_cur));
        if (pl.prod) LAUNCH(e, st, OP_MISC, 2, launch_product(st, pl.g + (size_t)k * TP, lam_cur, (int)e->PS, Tg, pl.prod + (size_t)k * TP));
      }
      const float* v = c.lr_vec ? dir_cur : lam_cur;
      AdvanceArgs adv = advance_base(e, pl.hv);
      rc = pass_hvp(e, st, pl, pl.sup[k], pl.xs, ns, Tg, pl.theta + (size_t)k * TP, pl.g + (size_t)k * TP, v, pl.hv, pl.gram_s, nullptr, nullptr,
                    tail ? &adv : nullptr, tail);
      if (rc) return rc;
      if (tail) {   // H lam finished, lam' = lam - lr H lam (into the other buffer: the row workgroups of the advance launch read lam's
                    // block-1 entries while others write lam'), and the tangent statistics of the next Hessian-vector pass
        adv.a = lam_cur; adv.out = lam_nxt; adv.alpha = c.lr_vec ? 1.f : inner_lr;
        if (msl && k > 0) { adv.inj_w = c.step_w + (k - 1); adv.inj = pl.qg + (size_t)(k - 1) * TP; }      // lam_k takes w_k q_k
        if (k > 0 && pl.gram_s) tangent_stats(adv, k - 1);
        if (c.lr_vec && k > 0) vector_extras(adv, k - 1);
        LAUNCH(e, st, OP_MISC, 2, launch_advance(st, adv, Tg));
        float* t = lam_cur; lam_cur = lam_nxt; lam_nxt = t;
        if (tr) HIPCHK(e, launch_scatter_tasks(st, pl.hv, e->perm_dev, (int)e->P, (int)e->PS, T, e->trace + (size_t)(3 * K + 1 + k) * TPr));
      } else {
        if (tr) HIPCHK(e, launch_scatter_tasks(st, pl.hv, e->perm_dev, (int)e->P, (int)e->PS, T, e->trace + (size_t)(3 * K + 1 + k) * TPr));
        LAUNCH(e, st, OP_MISC, 2, launch_axpy(st, lam_cur, pl.hv, c.lr_vec ? 1.f : inner_lr, (size_t)Tg * e->PS, lam_cur));
        if (msl && k > 0) LAUNCH(e, st, OP_MISC, 2, launch_fma_dev(st, lam_cur, pl.qg + (size_t)(k - 1) * TP, c.step_w + (k - 1), (size_t)Tg * e->PS));
      }
    }
  } else if (msl) {   // first order: lam_k = sum_{j >= max(k, 1)} w_j q_j, the products g_k * lam_{k+1} of the step-size gradient on the way down
    for (int k = K - 1; k >= 0; --k) {
      if (c.offsets_grad_out) LAUNCH(e, st, OP_MISC, 3, ofs_fold(pl.lam, k));
      if (pl.prod) LAUNCH(e, st, OP_MISC, 2, launch_product(st, pl.g + (size_t)k * TP, pl.lam, (int)e->PS, Tg, pl.prod + (size_t)k * TP));
      if (k > 0) LAUNCH(e, st, OP_MISC, 2, launch_fma_dev(st, pl.lam, pl.qg + (size_t)(k - 1) * TP, c.step_w + (k - 1), (size_t)Tg * e->PS));
    }
  } else if (c.offsets_grad_out) {   // first order, plain objective: every lam_{k+1} is the constant lam_K, the K rows in one launch
    LAUNCH(e, st, OP_MISC, 3, launch_offsets_grad_fold(st, pl.lam, 0, e->perm_dev, (int)e->P, (int)e->PS, Tg, K, c.offsets_grad_out));
  }
  if (tr) {
    for (int k = 0; k <= K; ++k)
      HIPCHK(e, launch_scatter_tasks(st, pl.theta + (size_t)k * TP, e->perm_dev, (int)e->P, (int)e->PS, T, e->trace + (size_t)k * TPr));
    for (int k = 0; k < K; ++k)
      HIPCHK(e, launch_scatter_tasks(st, pl.g + (size_t)k * TP, e->perm_dev, (int)e->P, (int)e->PS, T, e->trace + (size_t)(K + 1 + k) * TPr));
  }
  LAUNCH(e, st, OP_MISC, 3, launch_scatter_sum(st, lam_cur, e->perm_dev, (int)e->P, (int)e->PS, Tg, c.meta_grad_out));
  // lr_grad = -sum_t g_k * lam_{k+1} in the reference's order (second order: the stored products; first order: lam is the constant pl.lam)
  if (c.lr_vec && c.lr_grad_out)
    LAUNCH(e, st, OP_MISC, 3, launch_lr_grad_fold(st, (so || msl) ? pl.prod : nullptr, pl.g, pl.lam, e->perm_dev, (int)e->P, (int)e->PS, T, Tg, K,
                                                  c.lr_steps, c.lr_grad_out));
  return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// ANIL (reference vision/anil_vision.py:86-99,116-122 + utils/data_pre.py:118-119): the conv trunk runs ONCE per task on all
// 2*shots*ways images (BatchNorm statistics over support and query together), the inner loop adapts only the Linear head,
// the outer gradient reaches the trunk through the query features (directly) and through the support features (second-
// order path:  d L_q / d f_s = -lr * sum_k  R_{lam_{k+1}}{ dL_s/df_s }(w_k), the head tangent kernel's R{df} output).
struct AnilPlan {
  float *theta, *g, *lam, *hv;
  float* x;                 // [T][2n][H][W][C] NHWC
  int32_t *ys, *yq;
  ActSet act;               // trunk activations over 2n images
  float *fs, *fq, *dfs, *dfq, *rdf;   // [T][n][feat]
  float *prob, *dl;         // [K+1][T][n][ways]  (support steps 0..K-1, query at K)
  float *tmp_loss, *tmp_acc;
  float* hscr;
  Plan scratch;             // bnpart / wgpart live here
  size_t bytes;
};

static void make_anil_plan(const mi_engine* e, void* ws, int T, int n, int K, AnilPlan& ap) {
  Bump b{reinterpret_cast<char*>(ws), 0};
  const size_t TP = (size_t)T * e->PS;
  ap.theta = b.take<float>(TP * (K + 1));
  ap.g = b.take<float>(TP * (K > 0 ? K : 1));
  ap.lam = b.take<float>(TP);
  ap.hv = b.take<float>(TP);
  const size_t img = (size_t)e->d.in_h * e->d.in_w * e->d.in_channels;
  ap.x = b.take<float>((size_t)T * 2 * n * img);
  ap.ys = b.take<int32_t>((size_t)T * n);
  ap.yq = b.take<int32_t>((size_t)T * n);
  plan_actset(e, b, ap.act, T, 2 * n, true);
  const size_t fsz = (size_t)T * n * e->feat;
  ap.fs = b.take<float>(fsz); ap.fq = b.take<float>(fsz); ap.dfs = b.take<float>(fsz); ap.dfq = b.take<float>(fsz);
  ap.rdf = b.take<float>(fsz);
  ap.prob = b.take<float>((size_t)(K + 1) * T * n * e->d.ways);
  ap.dl = b.take<float>((size_t)(K + 1) * T * n * e->d.ways);
  ap.tmp_loss = b.take<float>(T);
  ap.tmp_acc = b.take<float>(T);
  ap.hscr = b.take<float>((size_t)T * n * (e->d.ways + 2));
  ap.scratch.cell_cap = 8 + 4 * (int)e->L.size();
  // (block 1's statistics and weight gradient come from the Gram matrix of all 2n images whenever the engine can form it)
  plan_partials(e, b, ap.scratch, T, 2 * n, false, true, 2 * n, false, true, [](size_t) {});
  ap.bytes = align_up(b.off, 256);
}

extern "C" int mi_anil_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || ways < 1 || shots < 1 || adapt_steps < 0) return MI_ERR_ARG;
  AnilPlan ap;
  make_anil_plan(e, nullptr, tasks, ways * shots, adapt_steps, ap);
  *bytes = ap.bytes;
  return MI_OK;
}

// What mi_meta_batch_anil_lr / _steps keep BEHIND the plain plan (whose offsets do not move).  Head-shaped vectors are compact:
// [ways * feat weights | ways biases] at a per-task stride of hs = Ph rounded up to 64 floats, the alignment the head has inside theta.
struct AnilExt {
  float* lrh;    // [lr_steps][hs]   step sizes in engine layout                              (vector step)
  float* dir;    // [T][hs]          D_k lam_{k+1}, the direction of the next head tangent    (vector step, second order)
  float* qg;     // [K][T][hs]       q_j = grad_theta L_q(theta_j) in slot j - 1, j < K        (steps call with a gradient)
  float* dqt;    // [T][n][feat]     dL_q/df_q of the query pass that has just run             (steps call with a gradient)
  float* prod;   // [K][T][hs]       g_k * lam_{k+1}                                           (lr_grad_out, unless lam is one constant)
  size_t hs, bytes;
};
static size_t anil_head_stride(const mi_engine* e) { return align_up(e->P - e->off_wl, 64); }
static void make_anil_ext(const mi_engine* e, void* ws, size_t plain_bytes, int T, int n, int K, bool with_grad, bool so, int lr_steps,
                          bool want_lr_grad, bool steps, AnilExt& ax) {
  Bump b{reinterpret_cast<char*>(ws), plain_bytes};
  ax = AnilExt{};
  ax.hs = anil_head_stride(e);
  const size_t th = (size_t)T * ax.hs;
  if (lr_steps > 0) ax.lrh = b.take<float>((size_t)lr_steps * ax.hs);
  if (lr_steps > 0 && with_grad && so && K > 0) ax.dir = b.take<float>(th);
  if (steps && with_grad) {
    if (K > 1) ax.qg = b.take<float>(th * (K - 1));
    ax.dqt = b.take<float>((size_t)T * n * e->feat);
  }
  if (lr_steps > 0 && with_grad && want_lr_grad && K > 0 && (so || steps)) ax.prod = b.take<float>(th * K);
  ax.bytes = align_up(b.off, 256);
}

// One workspace query for the three entries.  lr_steps = 0: the scalar step; step_outputs: 0 = the plain call's outputs, 1 = the per-step ones.
// mi_meta_batch_anil_proto takes every combination; mi_meta_batch_anil_lr is (lr_steps > 0, 0), mi_meta_batch_anil_steps (any, 1).
extern "C" int mi_anil_proto_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int with_grad, int second_order,
                                             int lr_steps, int want_lr_grad, int step_outputs, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || ways < 1 || shots < 1 || adapt_steps < 0 || lr_steps < 0) return MI_ERR_ARG;
  if (lr_steps != 0 && !lr_steps_ok(lr_steps, adapt_steps)) return MI_ERR_ARG;
  AnilPlan ap;
  make_anil_plan(e, nullptr, tasks, ways * shots, adapt_steps, ap);
  AnilExt ax;
  make_anil_ext(e, nullptr, ap.bytes, tasks, ways * shots, adapt_steps, with_grad != 0, with_grad && second_order, lr_steps, want_lr_grad != 0,
                step_outputs != 0, ax);
  *bytes = ax.bytes;
  return MI_OK;
}
extern "C" int mi_anil_workspace_bytes_steps(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int with_grad, int second_order,
                                             int lr_steps, int want_lr_grad, int step_outputs, size_t* bytes) {
  if (lr_steps == 0 && !step_outputs) return MI_ERR_ARG;
  return mi_anil_proto_workspace_bytes(e, tasks, ways, shots, adapt_steps, with_grad, second_order, lr_steps, want_lr_grad, step_outputs, bytes);
}

// c.lr_vec / c.step_w (mi_meta_batch_anil_lr / _steps; `ext` below), per task with D_k = diag(lr_k) or inner_lr * I:
//   theta_{k+1} = theta_k - D_k g_k;   q_j = grad_theta L_q(theta_j), dq_j = dL_q(theta_j)/df_q;   df_q = sum_j w_j dq_j
//   second order:  lam_K = w_K q_K;  lam_k = lam_{k+1} - H_k (D_k lam_{k+1}) + w_k q_k;  df_s = -sum_k R_{D_k lam_{k+1}}{dL_s/df_s}(theta_k)
//   first order:   lam_k = sum_{j >= max(k, 1)} w_j q_j;  df_s = 0
//   lr_grad_k = -sum_t g_k * lam_{k+1}
// (without step_w: w = (0, .., 0, 1) and only theta_K is scored).  The head launches are the plain call's; the elementwise work between
// them runs on the head slice only (anil_steps.hip).  With neither, `ext` is false and the launches are exactly the plain call's.
static int meta_batch_anil_impl(mi_engine* e, void* stream, const MetaCall& c) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int T = c.tasks, K = c.adapt_steps, n = c.ways * c.shots, nl = (int)e->L.size(), with_grad = c.grad_tasks > 0;
  const float inner_lr = c.inner_lr;
  const bool proto = c.algo == ALGO_ANIL_PROTO;      // (always `ext`: the head-slice launches, whatever the step and the objective)
  const bool ext = c.lr_vec || c.step_w || proto, msl = c.step_w != nullptr, so = c.second_order && with_grad;
  AnilPlan ap;
  make_anil_plan(e, c.workspace, T, n, K, ap);
  AnilExt ax{};
  if (ext) make_anil_ext(e, c.workspace, ap.bytes, T, n, K, with_grad != 0, so, c.lr_vec ? c.lr_steps : 0, c.lr_grad_out != nullptr, msl, ax);
  if ((ext ? ax.bytes : ap.bytes) > c.workspace_bytes)
    return fail(e, MI_ERR_WORKSPACE, "workspace too small: need " + std::to_string(ext ? ax.bytes : ap.bytes) + " bytes");
  const size_t TP = (size_t)T * e->PS, fsz = (size_t)T * n * e->feat, pw = (size_t)T * n * e->d.ways;
  const int Ph = (int)(e->P - e->off_wl), hbase = (int)e->off_wl;      // the head's entries of a parameter-shaped vector: [hbase, hbase + Ph)
  const size_t hb = (size_t)e->d.ways * e->feat;                       // the bias inside a compact head-shaped vector
  const int32_t* hperm = e->perm_dev + e->off_wl;
  auto lr_of = [&](int k) { return ax.lrh + (c.lr_steps == 1 ? 0 : (size_t)k * ax.hs); };
  LAUNCH(e, st, OP_MISC, 0, launch_nchw_to_nhwc(st, c.data, (size_t)T * 2 * n, e->d.in_channels, e->d.in_h, e->d.in_w, ap.x));
  LAUNCH(e, st, OP_MISC, 0, launch_split_labels(st, c.labels, T, 2 * n, ap.ys, ap.yq));
  LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, c.theta, 0, e->perm_dev, (int)e->P, (int)e->PS, T, ap.theta));
  const double* gram = with_grad ? ap.scratch.gram_s : nullptr;       // pays off only with a backward pass
  if (gram)
    LAUNCH(e, st, OP_GRAM, 0, launch_input_gram(st, ap.x, T, 2 * n, e->L[0].h, e->L[0].w, e->L[0].ci, ap.scratch.gram_part, ap.scratch.gram_s));
  int rc = plan_begin(e, st, ap.scratch);
  if (rc) return rc;
  rc = trunk_forward(e, st, ap.scratch, ap.act, ap.x, 2 * n, T, ap.theta, gram);     // features(data) on all rows
  if (rc) return rc;
  e->export_pass = 0;
  rc = export_bn_stats(e, st, ap.act, T);
  if (rc) return rc;
  LAUNCH(e, st, OP_MISC, 4, launch_split_rows(st, ap.act.p[nl - 1], T, 2 * n, e->feat, ap.fs, ap.fq));
  // Proto-MAML: theta_0's head entries of every task from its support prototypes, over what the gather put there
  ProtoInitArgs pa{};
  pa.fs = ap.fs; pa.ys = ap.ys; pa.ns = n; pa.feat = e->feat; pa.ways = c.ways; pa.scale = c.scale; pa.stride = e->PS;
  if (proto) {
    pa.head = ap.theta + hbase;
    LAUNCH(e, st, OP_PROTO_INIT, 0, launch_proto_init(st, pa, T));
  }
  if (c.lr_vec) LAUNCH(e, st, OP_MISC, 1, launch_anil_gather_lr(st, c.lr_vec, hperm, hbase, Ph, (int)ax.hs, c.lr_steps, ax.lrh));
  if (msl && with_grad) HIPCHK(e, hipMemsetAsync(ap.dfq, 0, fsz * sizeof(float), st));
  // The steps call: the query set at theta_j with the launch of the final query pass (row j of the outputs; prob / dl in the final pass's
  // slot, which no tangent pass reads).  With a gradient and j >= 1: q_j into its slot (j = K: lam's head entries), dq_j into ax.dqt, and
  // df_q += w_j dq_j with the weight read on the device.
  auto query_at = [&](int j) -> int {
    const bool bwd = with_grad && j >= 1;
    HeadArgs ha = head_args_primal(e, ap.hscr, ap.fq, ap.yq, n, T, ap.theta + (size_t)j * TP, ap.lam, c.loss_out + (size_t)j * T,
                                   c.acc_out + (size_t)j * T, c.logits_out ? c.logits_out + (size_t)j * pw : nullptr, ap.prob + K * pw,
                                   ap.dl + K * pw, ax.dqt, bwd);
    if (bwd && j < K) { ha.dwl = ax.qg + (size_t)(j - 1) * T * ax.hs; ha.dbl = ha.dwl + hb; ha.gstride = ax.hs; }
    if (bwd) HEAD_LDS(e, "head", n, ha.ways, 0);
    LAUNCH(e, st, OP_HEAD, 0, launch_head_fwd_bwd(st, ha, T, bwd ? 1 : 0));
    if (bwd) LAUNCH(e, st, OP_MISC, 2, launch_fma_dev(st, ap.dfq, ax.dqt, c.step_w + (j - 1), fsz));
    return MI_OK;
  };
  for (int k = 0; k < K; ++k) {                                                    // head-only inner loop
    if (msl) { rc = query_at(k); if (rc) return rc; }
    float* th = ap.theta + (size_t)k * TP;
    float* gk = ap.g + (size_t)k * TP;
    if (!ext) HIPCHK(e, hipMemsetAsync(gk, 0, TP * sizeof(float), st));             // (ext: only the head's entries are read, and the head writes them all)
    rc = head_pass(e, st, ap.hscr, ap.fs, ap.ys, n, T, th, gk, ap.tmp_loss, ap.tmp_acc, nullptr, ap.prob + k * pw, ap.dl + k * pw,
                   nullptr, true);
    if (rc) return rc;
    if (ext)   // theta_{k+1}'s head entries: the trunk runs on theta_0 alone
      LAUNCH(e, st, OP_MISC, 2, launch_anil_advance(st, th + hbase, gk + hbase, e->PS, c.lr_vec ? lr_of(k) : nullptr, inner_lr, Ph, T, th + TP + hbase));
    else
      LAUNCH(e, st, OP_MISC, 2, launch_axpy(st, th, gk, inner_lr, TP, th + TP));
  }
  float* thK = ap.theta + (size_t)K * TP;
  if (with_grad) HIPCHK(e, hipMemsetAsync(ap.lam, 0, TP * sizeof(float), st));
  if (msl) rc = query_at(K);
  else rc = head_pass(e, st, ap.hscr, ap.fq, ap.yq, n, T, thK, ap.lam, c.loss_out, c.acc_out, c.logits_out, ap.prob + K * pw, ap.dl + K * pw, ap.dfq,
                      with_grad != 0);
  if (rc || !with_grad) return rc;
  HIPCHK(e, hipMemsetAsync(ap.dfs, 0, fsz * sizeof(float), st));
  if (ext) {
    // every launch below finishes lam_k on the head slice and leaves what step k - 1 needs: dir = D_{k-1} lam_k, prod_{k-1} = g_{k-1} * lam_k
    auto adjoint = [&](int k, bool hessian) -> int {
      AnilAdjArgs a{};
      a.lam = ap.lam + hbase; a.lstride = e->PS; a.cstride = ax.hs; a.ph = Ph; a.tasks = T;
      a.alpha = c.lr_vec ? 1.f : inner_lr;
      if (hessian) { a.hv = ap.hv + hbase; a.dfs = ap.dfs; a.rdf = ap.rdf; a.fcount = fsz; }
      if (msl && k == K) a.w = c.step_w + (K - 1);                                                       // lam_K = w_K q_K
      else if (msl && k >= 1) { a.w = c.step_w + (k - 1); a.inj = ax.qg + (size_t)(k - 1) * T * ax.hs; }   // lam_k takes w_k q_k
      if (k >= 1 && ax.dir) { a.lr = lr_of(k - 1); a.dir = ax.dir; }
      if (k >= 1 && ax.prod) { a.g = ap.g + (size_t)(k - 1) * TP + hbase; a.prod = ax.prod + (size_t)(k - 1) * T * ax.hs; }
      if (!a.hv && !a.w && !a.lr && !a.prod) return MI_OK;            // nothing to do (the vector call's lam_K without a successor)
      LAUNCH(e, st, OP_MISC, 2, launch_anil_adjoint(st, a));
      return MI_OK;
    };
    rc = adjoint(K, false);
    if (rc) return rc;
    for (int k = K - 1; k >= 0; --k) {
      if (so) {
        HeadArgs ha = head_args(e, ap.hscr, ap.fs, ap.theta + (size_t)k * TP, c.lr_vec ? nullptr : ap.lam, ap.hv, ap.rdf, n, T);
        if (c.lr_vec) { ha.wld = ax.dir; ha.bld = ax.dir + hb; ha.vstride = ax.hs; }
        ha.prob = ap.prob + k * pw; ha.dl = ap.dl + k * pw;
        HEAD_LDS(e, "head tangent", n, ha.ways, 1);
        LAUNCH(e, st, OP_HEAD_TAN, 0, launch_head_tangent(st, ha, T));
        rc = adjoint(k, true);
      } else if (msl && k >= 1) {
        rc = adjoint(k, false);       // first order: lam_k = lam_{k+1} + w_k q_k
      }
      if (rc) return rc;
    }
  } else if (c.second_order) {
    for (int k = K - 1; k >= 0; --k) {
      HIPCHK(e, hipMemsetAsync(ap.hv, 0, TP * sizeof(float), st));
      HeadArgs ha = head_args(e, ap.hscr, ap.fs, ap.theta + (size_t)k * TP, ap.lam, ap.hv, ap.rdf, n, T);   // (the features are fixed: no fd)
      ha.prob = ap.prob + k * pw; ha.dl = ap.dl + k * pw;
      HEAD_LDS(e, "head tangent", n, ha.ways, 1);
      LAUNCH(e, st, OP_HEAD_TAN, 0, launch_head_tangent(st, ha, T));
      LAUNCH(e, st, OP_MISC, 2, launch_axpy(st, ap.dfs, ap.rdf, inner_lr, fsz, ap.dfs));   // dfs -= lr * R{df}
      LAUNCH(e, st, OP_MISC, 2, launch_axpy(st, ap.lam, ap.hv, inner_lr, TP, ap.lam));     // lam -= lr * H lam
    }
  }
  // Proto-MAML: lam's head entries are lam_0 = d objective / d theta_0's head; through the initialisation they reach the support features
  // (on top of the loop's own df_s) and the scale
  if (proto) {
    pa.lam = ap.lam + hbase; pa.dfs = ap.dfs; pa.dscale = c.dhyper_out;
    LAUNCH(e, st, OP_PROTO_INIT, 1, launch_proto_init_bwd(st, pa, T));
  }
  LAUNCH(e, st, OP_MISC, 4, launch_interleave_rows(st, ap.dfs, ap.dfq, T, n, e->feat, ap.act.dp[nl - 1]));
  rc = trunk_backward(e, st, ap.scratch, ap.act, ap.x, 2 * n, T, ap.theta, ap.lam, gram);  // trunk grads join the head part in lam
  if (rc) return rc;
  LAUNCH(e, st, OP_MISC, 3, launch_scatter_sum(st, ap.lam, e->perm_dev, (int)e->P, (int)e->PS, T, c.meta_grad_out));
  // Proto-MAML: the learner's head enters no result.  Its entries of the gradient (the last Ph in reference order) are exact zeros; lam
  // itself keeps lam_0, which the first-order fold below still reads
  if (proto) HIPCHK(e, hipMemsetAsync(c.meta_grad_out + (e->P - Ph), 0, (size_t)Ph * sizeof(float), st));
  // lr_grad in head.parameters() order: the stored products, or (first order, final loss only) g_k times the one constant lam, whose head
  // entries the trunk backward has left as they were
  if (c.lr_vec && c.lr_grad_out)
    LAUNCH(e, st, OP_MISC, 3, launch_anil_lr_fold(st, ax.prod, ax.hs, ap.g + hbase, ap.lam + hbase, e->PS, hperm, hbase, Ph, T, K, c.lr_steps,
                                                  c.lr_grad_out));
  return MI_OK;
}

// mi_meta_batch_metric / mi_meta_batch_ridge / mi_meta_batch_logreg, the closed-form call: the launches of meta_batch_anil_impl up to the split of the features, ONE
// head launch chosen by `algo` (no head parameters, no inner loop, no tangent pass), then -- with a gradient -- the interleave, the trunk backward and the sum over tasks (without one the call ends
// at the head).  lam's head entries stay
// the zeros of the memset, so meta_grad_out's head entries are exact zeros.  The plan is the ANIL call's with K = 0.
extern "C" int mi_metric_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes) {
  (void)with_grad;                       // (one plan for both: the evaluation call leaves the backward's arrays unused)
  return mi_anil_workspace_bytes(e, tasks, ways, shots, 0, bytes);
}
static int meta_batch_closed_form_impl(mi_engine* e, void* stream, const MetaCall& c) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int T = c.tasks, n = c.ways * c.shots, nl = (int)e->L.size(), with_grad = c.grad_tasks > 0;
  AnilPlan ap;
  make_anil_plan(e, c.workspace, T, n, 0, ap);
  if (ap.bytes > c.workspace_bytes) return fail(e, MI_ERR_WORKSPACE, "workspace too small: need " + std::to_string(ap.bytes) + " bytes");
  const size_t TP = (size_t)T * e->PS;
  LAUNCH(e, st, OP_MISC, 0, launch_nchw_to_nhwc(st, c.data, (size_t)T * 2 * n, e->d.in_channels, e->d.in_h, e->d.in_w, ap.x));
  LAUNCH(e, st, OP_MISC, 0, launch_split_labels(st, c.labels, T, 2 * n, ap.ys, ap.yq));
  LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, c.theta, 0, e->perm_dev, (int)e->P, (int)e->PS, T, ap.theta));
  // Block 1's statistics through the Gram matrix with or without a backward half (the ANIL call drops it from its evaluation call, whose
  // forward then rounds differently): the evaluation call here is the training call's forward bit for bit, for one more launch
  const double* gram = ap.scratch.gram_s;
  if (gram)
    LAUNCH(e, st, OP_GRAM, 0, launch_input_gram(st, ap.x, T, 2 * n, e->L[0].h, e->L[0].w, e->L[0].ci, ap.scratch.gram_part, ap.scratch.gram_s));
  int rc = plan_begin(e, st, ap.scratch);
  if (rc) return rc;
  rc = trunk_forward(e, st, ap.scratch, ap.act, ap.x, 2 * n, T, ap.theta, gram);     // features(data) on all rows
  if (rc) return rc;
  e->export_pass = 0;
  rc = export_bn_stats(e, st, ap.act, T);
  if (rc) return rc;
  LAUNCH(e, st, OP_MISC, 4, launch_split_rows(st, ap.act.p[nl - 1], T, 2 * n, e->feat, ap.fs, ap.fq));
  float *dfs = with_grad ? ap.dfs : nullptr, *dfq = with_grad ? ap.dfq : nullptr;
  if (c.algo == ALGO_RIDGE) {              // the head launch is all that `algo` chooses
    RidgeArgs ra = closed_form_args<RidgeArgs>(ap.fs, ap.fq, ap.ys, ap.yq, n, n, e->feat, c.ways, c.loss_out, c.acc_out, c.logits_out, dfs, dfq);
    ra.h = {c.lam, c.alpha};
    ra.dhyper = with_grad ? c.dhyper_out : nullptr;
    LAUNCH(e, st, OP_RIDGE_HEAD, 0, launch_ridge_head(st, ra, T));
  } else if (c.algo == ALGO_LOGREG) {
    LogregArgs la = closed_form_args<LogregArgs>(ap.fs, ap.fq, ap.ys, ap.yq, n, n, e->feat, c.ways, c.loss_out, c.acc_out, c.logits_out, dfs, dfq);
    la.h = {c.lam, c.alpha};
    la.dhyper = with_grad ? c.dhyper_out : nullptr;
    LAUNCH(e, st, OP_LOGREG_HEAD, 0, launch_logreg_head(st, la, T));
  } else {
    MetricArgs ma = closed_form_args<MetricArgs>(ap.fs, ap.fq, ap.ys, ap.yq, n, n, e->feat, c.ways, c.loss_out, c.acc_out, c.logits_out, dfs, dfq);
    ma.h = {c.metric, c.scale};
    LAUNCH(e, st, OP_METRIC_HEAD, 0, launch_metric_head(st, ma, T));
  }
  if (!with_grad) return MI_OK;
  HIPCHK(e, hipMemsetAsync(ap.lam, 0, TP * sizeof(float), st));
  LAUNCH(e, st, OP_MISC, 4, launch_interleave_rows(st, ap.dfs, ap.dfq, T, n, e->feat, ap.act.dp[nl - 1]));
  rc = trunk_backward(e, st, ap.scratch, ap.act, ap.x, 2 * n, T, ap.theta, ap.lam, gram);
  if (rc) return rc;
  LAUNCH(e, st, OP_MISC, 3, launch_scatter_sum(st, ap.lam, e->perm_dev, (int)e->P, (int)e->PS, T, c.meta_grad_out));
  return MI_OK;
}

// ---- graph replay of the fused calls
// What a captured graph depends on, field by field (never the struct's bytes: its padding is indeterminate): two calls whose keys are equal
// make the same launches with the same arguments.  Every engine switch and the kernel selection in an element of its own: nothing packed,
// nothing that can alias.  The step sizes' VALUES are read on the device at every replay, like theta's.
static GraphKey graph_key(const mi_engine* e, void* stream, const MetaCall& c) {
  typedef unsigned long long u;
  unsigned lr_bits, scale_bits, lam_bits, alpha_bits;
  memcpy(&lr_bits, &c.inner_lr, sizeof lr_bits);
  memcpy(&lam_bits, &c.lam, sizeof lam_bits);
  memcpy(&alpha_bits, &c.alpha, sizeof alpha_bits);
  memcpy(&scale_bits, &c.scale, sizeof scale_bits);
  return GraphKey{(u)c.algo, (u)(uintptr_t)stream, (u)(uintptr_t)c.theta, (u)(uintptr_t)c.data, (u)(uintptr_t)c.labels, (u)c.tasks,
                  (u)c.grad_tasks, (u)c.ways, (u)c.shots, (u)c.adapt_steps, (u)c.second_order, (u)lr_bits, (u)(uintptr_t)c.lr_vec,
                  (u)c.lr_steps, (u)(uintptr_t)c.lr_grad_out, (u)(uintptr_t)c.loss_out, (u)(uintptr_t)c.acc_out,
                  (u)(uintptr_t)c.meta_grad_out, (u)(uintptr_t)c.logits_out, (u)(uintptr_t)c.workspace, (u)c.workspace_bytes,
                  (u)e->fuse1, (u)e->gram1, (u)e->gramq, (u)e->overlap, (u)e->fuse_fin, (u)e->fuse_b1red, (u)e->fuse_tail, (u)e->fuse_last,
                  kernel_selection_key(), (u)(uintptr_t)c.step_w, (u)(uintptr_t)c.offsets, (u)(uintptr_t)c.offsets_grad_out,
                  (u)c.metric, (u)scale_bits, (u)lam_bits, (u)alpha_bits, (u)(uintptr_t)c.dhyper_out};
}

static int meta_batch_entry(mi_engine* e, void* stream, const MetaCall& c) {
  const int crc = check_call(e, c);
  if (crc) return crc;
  const auto fn = is_closed_form(c.algo) ? meta_batch_closed_form_impl : is_anil(c.algo) ? meta_batch_anil_impl : meta_batch_maml_impl;
  if (!e->graph_on || e->prof_on || e->trace || e->bn_export || !stream)     // (capture is not permitted on the legacy default stream)
    return fn(e, stream, c);
  const GraphKey key = graph_key(e, stream, c);
  mi_engine::GraphEntry* ent = nullptr;
  for (auto& g : e->graphs)
    if (g.key == key) { ent = &g; break; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (ent && ent->exec) {
    HIPCHK(e, hipGraphLaunch(ent->exec, st));
    return MI_OK;
  }
  if (!ent) {                                   // first sight: run eagerly (kernel attributes, lazily created streams and events)
    if (e->graphs.size() >= 8) {                // small cache: drop the oldest
      if (e->graphs.front().exec) (void)hipGraphExecDestroy(e->graphs.front().exec);
      if (e->graphs.front().graph) (void)hipGraphDestroy(e->graphs.front().graph);
      e->graphs.erase(e->graphs.begin());
    }
    e->graphs.push_back(mi_engine::GraphEntry{});
    e->graphs.back().key = key;
    e->graphs.back().seen = 1;
    return fn(e, stream, c);
  }
  // second sight: capture the launch sequence (nothing executes), instantiate, launch
  HIPCHK(e, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = fn(e, stream, c);
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(st, &graph);
  if (rc != MI_OK || ce != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    e->graph_on = false;                         // do not try again; the caller gets the error of this call
    return rc != MI_OK ? rc : fail(e, MI_ERR_HIP, std::string("graph capture failed: ") + hipGetErrorString(ce));
  }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGraphDestroy(graph);
    e->graph_on = false;
    return fail(e, MI_ERR_HIP, "hipGraphInstantiate failed");
  }
  ent->graph = graph;
  ent->exec = exec;
  HIPCHK(e, hipGraphLaunch(exec, st));
  return MI_OK;
}

extern "C" int mi_meta_batch_maml(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                  int tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order,
                                  int with_grad, float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                                  void* workspace, size_t workspace_bytes) {
  return meta_batch_entry(e, stream, MetaCall{ALGO_MAML, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, adapt_steps,
                                              second_order, inner_lr, nullptr, 0, nullptr, loss_out, acc_out, meta_grad_out, logits_out,
                                              workspace, workspace_bytes});
}
// Train and validation halves of one meta-iteration in the same launches (reference maml_vision.py:102-124): the first grad_tasks
// tasks are the train tasks (their summed meta-gradient goes to meta_grad_out), the rest are adapted and scored only.
extern "C" int mi_meta_batch_maml_tv(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                     int tasks, int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order,
                                     float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                                     void* workspace, size_t workspace_bytes) {
  return meta_batch_entry(e, stream, MetaCall{ALGO_MAML, theta, data, labels, tasks, grad_tasks, ways, shots, adapt_steps, second_order,
                                              inner_lr, nullptr, 0, nullptr, loss_out, acc_out, meta_grad_out, logits_out, workspace,
                                              workspace_bytes});
}
// mi_meta_batch_maml_tv with one step size per parameter (and per inner step when lr_steps == adapt_steps), read from device memory, and
// the gradient of the summed query loss with respect to them (include/mi_maml.h).
extern "C" int mi_meta_batch_maml_lr(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                     int grad_tasks, int ways, int shots, int adapt_steps, const float* lr_vec, int lr_steps,
                                     int second_order, float* loss_out, float* acc_out, float* meta_grad_out, float* lr_grad_out,
                                     float* logits_out, void* workspace, size_t workspace_bytes) {
  return meta_batch_entry(e, stream, MetaCall{ALGO_MAML_LR, theta, data, labels, tasks, grad_tasks, ways, shots, adapt_steps, second_order,
                                              0.f, lr_vec, lr_steps, lr_grad_out, loss_out, acc_out, meta_grad_out, logits_out, workspace,
                                              workspace_bytes});
}
// mi_meta_batch_maml_tv / _lr with the query set scored at every theta_j and the multi-step loss sum_j step_w[j - 1] L_query(theta_j) as the
// outer objective (include/mi_maml.h).
extern "C" int mi_meta_batch_maml_steps(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                        int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps,
                                        const float* step_w, int second_order, float* loss_steps_out, float* acc_steps_out, float* meta_grad_out,
                                        float* lr_grad_out, float* logits_steps_out, void* workspace, size_t workspace_bytes) {
  MetaCall c{ALGO_MAML_STEPS, theta, data, labels, tasks, grad_tasks, ways, shots, adapt_steps, second_order, lr_vec ? 0.f : inner_lr, lr_vec,
             lr_vec ? lr_steps : 0, lr_grad_out, loss_steps_out, acc_steps_out, meta_grad_out, logits_steps_out, workspace, workspace_bytes};
  c.step_w = step_w;
  return meta_batch_entry(e, stream, c);
}
// mi_meta_batch_maml_tv / _lr / _steps with per-step parameter offsets theta_{k+1} = (theta_k - D_k g_k) + offsets[k] and their gradient
// (include/mi_maml.h).  step_w NULL: the plain call's outputs and objective.
extern "C" int mi_meta_batch_maml_offsets(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                          int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps,
                                          const float* step_w, const float* offsets, int second_order, float* loss_out, float* acc_out,
                                          float* meta_grad_out, float* lr_grad_out, float* offsets_grad_out, float* logits_out, void* workspace,
                                          size_t workspace_bytes) {
  MetaCall c{ALGO_MAML_OFFSETS, theta, data, labels, tasks, grad_tasks, ways, shots, adapt_steps, second_order, lr_vec ? 0.f : inner_lr, lr_vec,
             lr_vec ? lr_steps : 0, lr_grad_out, loss_out, acc_out, meta_grad_out, logits_out, workspace, workspace_bytes};
  c.step_w = step_w;
  c.offsets = offsets;
  c.offsets_grad_out = offsets_grad_out;
  return meta_batch_entry(e, stream, c);
}
extern "C" int mi_meta_batch_anil(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                  int tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order,
                                  int with_grad, float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                                  void* workspace, size_t workspace_bytes) {
  return meta_batch_entry(e, stream, MetaCall{ALGO_ANIL, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, adapt_steps,
                                              second_order, inner_lr, nullptr, 0, nullptr, loss_out, acc_out, meta_grad_out, logits_out,
                                              workspace, workspace_bytes});
}

// mi_meta_batch_anil with one step size per head parameter (and per inner step when lr_steps == adapt_steps), read from device memory, and
// the gradient of the summed query loss with respect to them (include/mi_maml.h).
extern "C" int mi_meta_batch_anil_lr(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                     int ways, int shots, int adapt_steps, const float* lr_vec, int lr_steps, int second_order, int with_grad,
                                     float* loss_out, float* acc_out, float* meta_grad_out, float* lr_grad_out, float* logits_out,
                                     void* workspace, size_t workspace_bytes) {
  return meta_batch_entry(e, stream, MetaCall{ALGO_ANIL_LR, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, adapt_steps,
                                              second_order, 0.f, lr_vec, lr_steps, lr_grad_out, loss_out, acc_out, meta_grad_out, logits_out,
                                              workspace, workspace_bytes});
}
// mi_meta_batch_anil / _anil_lr with the query set scored at every theta_j and the multi-step loss sum_j step_w[j - 1] L_query(theta_j) as
// the outer objective (include/mi_maml.h).
extern "C" int mi_meta_batch_anil_steps(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                        int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps,
                                        const float* step_w, int second_order, int with_grad, float* loss_steps_out, float* acc_steps_out,
                                        float* meta_grad_out, float* lr_grad_out, float* logits_steps_out, void* workspace,
                                        size_t workspace_bytes) {
  MetaCall c{ALGO_ANIL_STEPS, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, adapt_steps, second_order, lr_vec ? 0.f : inner_lr,
             lr_vec, lr_vec ? lr_steps : 0, lr_grad_out, loss_steps_out, acc_steps_out, meta_grad_out, logits_steps_out, workspace,
             workspace_bytes};
  c.step_w = step_w;
  return meta_batch_entry(e, stream, c);
}

// mi_meta_batch_anil_lr / _steps with theta_0's head derived per task from the support prototypes (Proto-MAML; include/mi_maml.h).
extern "C" int mi_meta_batch_anil_proto(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                                        int ways, int shots, int adapt_steps, int second_order, float inner_lr, const float* lr_vec, int lr_steps,
                                        const float* step_w, float scale, int with_grad, float* loss_out, float* acc_out, float* meta_grad_out,
                                        float* lr_grad_out, float* dscale_out, float* logits_out, void* workspace, size_t workspace_bytes) {
  MetaCall c{ALGO_ANIL_PROTO, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, adapt_steps, second_order, lr_vec ? 0.f : inner_lr,
             lr_vec, lr_vec ? lr_steps : 0, lr_grad_out, loss_out, acc_out, meta_grad_out, logits_out, workspace, workspace_bytes};
  c.step_w = step_w;
  c.scale = scale;
  c.dhyper_out = dscale_out;
  return meta_batch_entry(e, stream, c);
}

// A closed-form head (MI_METRIC_PROTO / MI_METRIC_COSINE) on the ANIL engine's trunk, no inner loop (include/mi_maml.h).
extern "C" int mi_meta_batch_metric(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                    int tasks, int ways, int shots, int metric, float scale, int with_grad,
                                    float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                                    void* workspace, size_t workspace_bytes) {
  MetaCall c{ALGO_METRIC, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, 0, 0, 0.f, nullptr, 0, nullptr, loss_out, acc_out,
             meta_grad_out, logits_out, workspace, workspace_bytes};
  c.metric = metric;
  c.scale = scale;
  return meta_batch_entry(e, stream, c);
}

// The ridge-regression head (R2-D2) on the ANIL engine's trunk: mi_meta_batch_metric's launches around launch_ridge_head (include/mi_maml.h).
extern "C" int mi_ridge_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes) {
  return mi_metric_workspace_bytes(e, tasks, ways, shots, with_grad, bytes);
}
extern "C" int mi_meta_batch_ridge(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                   int tasks, int ways, int shots, float lam, float alpha, int with_grad,
                                   float* loss_out, float* acc_out, float* meta_grad_out, float* dhyper_out, float* logits_out,
                                   void* workspace, size_t workspace_bytes) {
  MetaCall c{ALGO_RIDGE, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, 0, 0, 0.f, nullptr, 0, nullptr, loss_out, acc_out,
             meta_grad_out, logits_out, workspace, workspace_bytes};
  c.lam = lam;
  c.alpha = alpha;
  c.dhyper_out = dhyper_out;
  return meta_batch_entry(e, stream, c);
}

// The logistic-regression head on the ANIL engine's trunk: mi_meta_batch_ridge's call around launch_logreg_head (include/mi_maml.h).
extern "C" int mi_logreg_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes) {
  return mi_metric_workspace_bytes(e, tasks, ways, shots, with_grad, bytes);
}
extern "C" int mi_meta_batch_logreg(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                                    int tasks, int ways, int shots, float lam, float alpha, int with_grad,
                                    float* loss_out, float* acc_out, float* meta_grad_out, float* dhyper_out, float* logits_out,
                                    void* workspace, size_t workspace_bytes) {
  MetaCall c{ALGO_LOGREG, theta, data, labels, tasks, with_grad ? tasks : 0, ways, shots, 0, 0, 0.f, nullptr, 0, nullptr, loss_out, acc_out,
             meta_grad_out, logits_out, workspace, workspace_bytes};
  c.lam = lam;
  c.alpha = alpha;
  c.dhyper_out = dhyper_out;
  return meta_batch_entry(e, stream, c);
}

// Plain forward of the classifier (BatchNorm in train mode, i.e. statistics of the n images of each task batch), no
// adaptation: `learner(x)` / `model(x)` of the reference (vision_models.py:51-55,107-110).
extern "C" int mi_forward_logits(mi_engine* e, void* stream, const float* theta, const float* x, int tasks, int n,
                                 float* logits_out, void* workspace, size_t workspace_bytes) {
  return mi_learner_forward(e, stream, theta, 1, x, tasks, n, logits_out, 0, nullptr, workspace, workspace_bytes);   // its shared-theta case
}

extern "C" int mi_forward_workspace_bytes(const mi_engine* e, int tasks, int n, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || n < 1) return MI_ERR_ARG;
  return plan_bytes(e, forward_shape(tasks, n), bytes);
}

// ---------------------------------------------------------------------------------------------------------------------
// Step-wise learner (reference: `learner(x)`, `learner.adapt(loss)`, `get_rep`, `get_rep_i` on a learn2learn clone --
// misc_scripts/cl_vision.py:56-66, misc_scripts/rc_vision.py:66-86, core_functions/maml.py:15-19).  The fast weights live
// with the caller (theta [theta_tasks][P], reference order); forward and backward are two stateless calls, the backward
// re-runs the forward into the workspace instead of keeping activations alive between calls.
// What the three learner calls open with: the checks, the plan of shape s in the workspace, plan_begin, x as NHWC in the plan's image
// buffer `ximg` (pl.xq, or pl.xs for the kept pass of mi_learner_hvp) and the weights gathered into pl.theta.  `bad`: what is wrong with the
// call's own arguments, or nullptr.
static int learner_begin(mi_engine* e, hipStream_t st, const float* theta, int theta_tasks, const float* x, int tasks, int n, const char* bad,
                         void* workspace, size_t workspace_bytes, const PlanShape& s, Plan& pl, float* Plan::*ximg) {
  if (!e) return fail(nullptr, MI_ERR_ARG, "null engine");
  if (!theta || !x || !workspace || tasks < 1 || n < 1) return fail(e, MI_ERR_ARG, "bad learner arguments");
  if (theta_tasks != 1 && theta_tasks != tasks) return fail(e, MI_ERR_ARG, "theta_tasks must be 1 (shared) or == tasks");
  if (bad) return fail(e, MI_ERR_ARG, bad);
  int rc = plan_in(e, workspace, workspace_bytes, s, pl);
  if (rc) return rc;
  rc = plan_begin(e, st, pl);
  if (rc) return rc;
  LAUNCH(e, st, OP_MISC, 0, launch_nchw_to_nhwc(st, x, (size_t)tasks * n, e->d.in_channels, e->d.in_h, e->d.in_w, pl.*ximg));
  LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, theta, theta_tasks == 1 ? 0 : e->P, e->perm_dev, (int)e->P, (int)e->PS, tasks, pl.theta));
  return MI_OK;
}
// ... and what the two that return gradients end with: g (engine layout, per task) to the caller's [theta_tasks][P], summed over the tasks
// when they share one theta.
static int learner_scatter(mi_engine* e, hipStream_t st, const float* g, int theta_tasks, int tasks, float* out) {
  if (theta_tasks == 1) {
    LAUNCH(e, st, OP_MISC, 3, launch_scatter_sum(st, g, e->perm_dev, (int)e->P, (int)e->PS, tasks, out));
  } else {
    LAUNCH(e, st, OP_MISC, 3, launch_scatter_tasks(st, g, e->perm_dev, (int)e->P, (int)e->PS, tasks, out));
  }
  return MI_OK;
}

// Forward over x with the gathered weights pl.theta, then the backward of s = sum(logits * dlogits) with the caller's cotangent: ds/dtheta
// into g (engine layout, per task), the layer cotangents into A.
static int learner_fwd_bwd(mi_engine* e, hipStream_t st, Plan& pl, ActSet& A, const float* x, const float* dlogits, int n, int tasks, float* g) {
  const int nl = (int)e->L.size();
  int rc = trunk_forward(e, st, pl, A, x, n, tasks, pl.theta);
  if (rc) return rc;
  if (e->d.head_mean_pool) HIPCHK(e, launch_spatial_mean(st, A.p[nl - 1], A.f, tasks * n, e->head_hw, e->head_c));
  HIPCHK(e, hipMemsetAsync(g, 0, (size_t)tasks * e->PS * sizeof(float), st));
  HeadArgs ha = head_args(e, nullptr, A.f, pl.theta, nullptr, g, A.df, n, tasks);
  ha.dl = const_cast<float*>(dlogits);
  HEAD_LDS(e, "head backward", n, ha.ways, 0);
  LAUNCH(e, st, OP_HEAD, 0, launch_head_grads(st, ha, tasks));
  if (e->d.head_mean_pool) HIPCHK(e, launch_spatial_mean_bwd(st, A.df, A.dp[nl - 1], tasks * n, e->head_hw, e->head_c));
  return trunk_backward(e, st, pl, A, x, n, tasks, pl.theta, g);
}

extern "C" int mi_learner_forward(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x, int tasks,
                                  int n, float* logits_out, int rep_layer, float* rep_out, void* workspace,
                                  size_t workspace_bytes) {
  Plan pl;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const char* bad = (e && rep_out && (rep_layer < 1 || rep_layer > (int)e->L.size())) ? "rep_layer must be in 1..layers"
                    : (!logits_out && !rep_out) ? "nothing to compute: logits_out and rep_out are both NULL" : nullptr;
  ExportPause no_export(e);
  int rc = learner_begin(e, st, theta, theta_tasks, x, tasks, n, bad, workspace, workspace_bytes, forward_shape(tasks, n), pl, &Plan::xq);
  if (rc) return rc;
  HIPCHK(e, hipMemsetAsync(pl.yq, 0, (size_t)tasks * n * sizeof(int32_t), st));
  rc = pass_fwd_bwd(e, st, pl, pl.qry, pl.xq, pl.yq, n, tasks, pl.theta, pl.lam, pl.tmp_loss, pl.tmp_acc, logits_out, false);
  if (rc) return rc;
  if (rep_out) {
    const Layer& L = e->L[rep_layer - 1];
    LAUNCH(e, st, OP_MISC, 0, launch_nhwc_to_nchw(st, pl.qry.p[rep_layer - 1], (size_t)tasks * n, L.co, L.hp, L.wp, rep_out));
  }
  return MI_OK;
}

extern "C" int mi_learner_backward(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x,
                                   const float* dlogits, int tasks, int n, float* grad_out, void* workspace,
                                   size_t workspace_bytes) {
  Plan pl;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ExportPause no_export(e);
  int rc = learner_begin(e, st, theta, theta_tasks, x, tasks, n, (!dlogits || !grad_out) ? "null dlogits / grad_out" : nullptr, workspace,
                         workspace_bytes, forward_shape(tasks, n), pl, &Plan::xq);
  if (rc) return rc;
  rc = learner_fwd_bwd(e, st, pl, pl.qry, pl.xq, dlogits, n, tasks, pl.lam);
  if (rc) return rc;
  return learner_scatter(e, st, pl.lam, theta_tasks, tasks, grad_out);
}

// Double backward of the step-wise learner: with s(theta) = sum(logits(theta) * dlogits) and g = ds/dtheta (mi_learner_backward),
// autograd asks for the vector-Jacobian products of (theta, dlogits) -> g with a cotangent v on g:
//   grad_theta_out = (d^2 s / dtheta^2) v   (forward-over-reverse, dlogits held fixed),   logits_dot_out = J(theta) v.
// This is what makes `learner.adapt(loss)` of a second-order learner differentiable (learn2learn MAML.adapt with create_graph,
// driven step-wise at misc_scripts/rc_vision.py:67-70); the cross-entropy's own curvature reaches theta through logits_dot_out
// and an ordinary mi_learner_backward, by the chain rule autograd already applies.
extern "C" int mi_learner_hvp_workspace_bytes(const mi_engine* e, int tasks, int n, size_t* bytes) {
  if (!e || !bytes || tasks < 1 || n < 1) return MI_ERR_ARG;
  return plan_bytes(e, hvp_shape(tasks, n), bytes);
}

extern "C" int mi_learner_hvp(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x, const float* dlogits,
                              const float* v, int tasks, int n, float* grad_theta_out, float* logits_dot_out, void* workspace,
                              size_t workspace_bytes) {
  Plan pl;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ExportPause no_export(e);
  int rc = learner_begin(e, st, theta, theta_tasks, x, tasks, n,
                         (!dlogits || !v || !grad_theta_out || !logits_dot_out) ? "bad mi_learner_hvp arguments" : nullptr, workspace,
                         workspace_bytes, hvp_shape(tasks, n), pl, &Plan::xs);
  if (rc) return rc;
  ActSet& A = pl.sup[0];
  LAUNCH(e, st, OP_MISC, 1, launch_gather_params(st, v, theta_tasks == 1 ? 0 : e->P, e->perm_dev, (int)e->P, (int)e->PS, tasks, pl.lam));
  // primal backward with the given cotangent: the tangent sweep needs its BatchNorm sums (g) and layer cotangents (A.dp)
  rc = learner_fwd_bwd(e, st, pl, A, pl.xs, dlogits, n, tasks, pl.g);
  if (rc) return rc;
  rc = pass_hvp(e, st, pl, A, pl.xs, n, tasks, pl.theta, pl.g, pl.lam, pl.hv, nullptr, dlogits, logits_dot_out);
  if (rc) return rc;
  return learner_scatter(e, st, pl.hv, theta_tasks, tasks, grad_theta_out);
}

extern "C" int mi_adam_step(void* stream, float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                            int step, float lr, float beta1, float beta2, float eps, float grad_scale) {
  if (!theta || !grad || !exp_avg || !exp_avg_sq || step < 1) return fail(nullptr, MI_ERR_ARG, "bad adam arguments");
  hipError_t s = launch_adam(reinterpret_cast<hipStream_t>(stream), theta, grad, exp_avg, exp_avg_sq, n, step, lr, beta1,
                             beta2, eps, grad_scale);
  return s == hipSuccess ? MI_OK : fail(nullptr, MI_ERR_HIP, hipGetErrorString(s));
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-kernel entry points (unit parity tests).
#define HIPCHK0(call)                                                                     \
  do {                                                                                    \
    hipError_t _s = (call);                                                               \
    if (_s != hipSuccess) return fail(nullptr, MI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s)); \
  } while (0)

extern "C" size_t mi_kernel_scratch_bytes(int tasks, int n, int h, int w, int c) {
  // generous: covers bn partials and wgrad partials for one layer with <= 64 input channels
  ConvGeom g{n, h, w, h, w, 64, c, 1};
  ConvGeom g2{n, h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 64, c, 2};      // the stride-2 (Omniglot) weight gradient splits finer
  size_t bn = (size_t)tasks * (size_t)conv_max_blocks_per_task(g) * 2 * c * sizeof(double);
  size_t wg = wgrad_partial_floats(g, tasks) * sizeof(float);
  const size_t wg2 = wgrad_partial_floats(g2, tasks) * sizeof(float);
  if (wg2 > wg) wg = wg2;
  return align_up(bn, 256) + align_up(wg, 256) + 4096;
}

extern "C" int mi_prepare_batch(void* stream, const float* data, const int64_t* labels, int tasks, int n2, int c, int h, int w,
                                float* xs, float* xq, int32_t* ys, int32_t* yq) {
  if (n2 % 2) return fail(nullptr, MI_ERR_ARG, "task batch must hold 2*shots*ways rows");
  HIPCHK0(launch_prepare_batch(reinterpret_cast<hipStream_t>(stream), data, labels, tasks, n2, c, h, w, xs, xq, ys, yq));
  return MI_OK;
}

// Input Gram matrix of block 1 and BatchNorm statistics of conv1 from it (gram.hip); unit-test entry points.
extern "C" size_t mi_input_gram_scratch_bytes(int tasks, int n, int h, int ci) {
  return gram_partial_doubles(tasks, n, h, ci) * sizeof(double);
}
extern "C" int mi_input_gram(void* stream, const float* x, int tasks, int n, int h, int w, int ci, void* scratch,
                             size_t scratch_bytes, double* g_out) {
  if (!x || !scratch || !g_out || (ci != 1 && ci != 3)) return fail(nullptr, MI_ERR_ARG, "mi_input_gram: bad arguments (ci must be 1 or 3)");
  if (scratch_bytes < mi_input_gram_scratch_bytes(tasks, n, h, ci)) return fail(nullptr, MI_ERR_WORKSPACE, "mi_input_gram: scratch too small");
  HIPCHK0(launch_input_gram(reinterpret_cast<hipStream_t>(stream), x, tasks, n, h, w, ci, static_cast<double*>(scratch), g_out));
  return MI_OK;
}
extern "C" int mi_gram_bn_stats(void* stream, const double* g, int tasks, int ci, int co, const float* w9, size_t pstride,
                                const float* w9d, size_t vstride, int pixels, float* out0, float* out1, const float* mu,
                                const float* rstd) {
  if (!g || !w9 || !out0 || !out1 || (w9d && (!mu || !rstd))) return fail(nullptr, MI_ERR_ARG, "mi_gram_bn_stats: bad arguments");
  HIPCHK0(launch_gram_stats(reinterpret_cast<hipStream_t>(stream), g, tasks, ci, co, w9, pstride, w9d, vstride, 1.0 / (double)pixels,
                            w9d ? 1 : 0, out0, out1, mu, rstd));
  return MI_OK;
}

static bool cka_shape_ok(int pairs, int n, int p) { return pairs >= 1 && n >= 2 && n <= (1 << 18) && p >= 1 && p <= 128; }
extern "C" size_t mi_cka_scratch_bytes(int pairs, int n, int p) {
  return cka_shape_ok(pairs, n, p) ? cka_scratch_bytes(pairs, n, p) : 0;
}
extern "C" int mi_cka(void* stream, const float* x, const float* y, int pairs, int n, int p, double sigma, void* scratch,
                      size_t scratch_bytes, double* out) {
  if (!x || !y || !scratch || !out || !cka_shape_ok(pairs, n, p))
    return fail(nullptr, MI_ERR_ARG, "mi_cka: bad arguments (1 <= p <= 128, 2 <= n <= 2^18, pairs >= 1, non-null pointers)");
  if (scratch_bytes < cka_scratch_bytes(pairs, n, p)) return fail(nullptr, MI_ERR_WORKSPACE, "mi_cka: scratch too small");
  HIPCHK0(launch_cka(reinterpret_cast<hipStream_t>(stream), x, y, pairs, n, p, sigma, scratch, out));
  return MI_OK;
}

static bool cca_shape_ok(int pairs, int n, int p) { return pairs >= 1 && pairs <= (1 << 20) && n >= 2 && n <= (1 << 18) && p >= 1 && p <= 64; }
extern "C" size_t mi_cca_scratch_bytes(int pairs, int n, int p) {
  return cca_shape_ok(pairs, n, p) ? cca_scratch_bytes(pairs, n, p) : 0;
}
extern "C" int mi_cca(void* stream, const float* x, const float* y, int pairs, int n, int p, double epsilon, double threshold,
                      void* scratch, size_t scratch_bytes, double* coefs, double* stats) {
  if (!x || !y || !scratch || !coefs || !stats || !cca_shape_ok(pairs, n, p))
    return fail(nullptr, MI_ERR_ARG, "mi_cca: bad arguments (1 <= p <= 64, 2 <= n <= 2^18, 1 <= pairs <= 2^20, non-null pointers)");
  if (!(epsilon >= 0.0) || !(threshold >= 0.0 && threshold <= 1.0))
    return fail(nullptr, MI_ERR_ARG, "mi_cca: epsilon must be >= 0 and threshold in [0, 1]");
  if (scratch_bytes < cca_scratch_bytes(pairs, n, p)) return fail(nullptr, MI_ERR_WORKSPACE, "mi_cca: scratch too small");
  HIPCHK0(launch_cca(reinterpret_cast<hipStream_t>(stream), x, y, pairs, n, p, epsilon, threshold, scratch, coefs, stats));
  return MI_OK;
}

extern "C" int mi_stream_copy(void* stream, const void* src, void* dst, size_t bytes) {
  if (!src || !dst || bytes % 16) return fail(nullptr, MI_ERR_ARG, "mi_stream_copy: null pointer or size not a multiple of 16");
  HIPCHK0(launch_stream_copy(reinterpret_cast<hipStream_t>(stream), src, dst, bytes));
  return MI_OK;
}

extern "C" int mi_sample_tasks(void* stream, const void* dataset, int dataset_is_u8, size_t num_images, int c, int h, int w,
                               const int64_t* index, const uint8_t* rot, int tasks, int n2, float* data_out) {
  if (!dataset || !index || !data_out || tasks < 1 || n2 < 1 || num_images < 1) return fail(nullptr, MI_ERR_ARG, "bad sampler arguments");
  if (((size_t)c * h * w) % 4 != 0) return fail(nullptr, MI_ERR_ARG, "C*H*W must be a multiple of 4");
  if (rot && h != w) return fail(nullptr, MI_ERR_ARG, "quarter-turn rotations need square images");
  HIPCHK0(launch_sample_tasks(reinterpret_cast<hipStream_t>(stream), dataset, dataset_is_u8, index, rot, (size_t)tasks * n2, c, h, w, data_out));
  return MI_OK;
}

extern "C" int mi_draw_tasks(void* stream, const int32_t* class_offsets, const int32_t* class_index, int n_classes, int ways, int k,
                             const uint8_t* rot_table, int n_rot, int remap_shuffle, uint64_t seed, uint64_t first_slot,
                             uint64_t num_tasks, int tasks, int64_t* index_out, int64_t* labels_out, uint8_t* rot_out,
                             uint64_t* task_id_out) {
  if (!class_offsets || !class_index || !index_out || !labels_out || tasks < 1)
    return fail(nullptr, MI_ERR_ARG, "mi_draw_tasks: null pointer or tasks < 1");
  if (ways < 1 || ways > kDrawMaxWays || ways > n_classes)
    return fail(nullptr, MI_ERR_ARG, "mi_draw_tasks: ways must be 1.." + std::to_string(kDrawMaxWays) + " and at most n_classes");
  if (k < 1 || k > kDrawMaxK) return fail(nullptr, MI_ERR_ARG, "mi_draw_tasks: k must be 1.." + std::to_string(kDrawMaxK));
  if (n_rot < 0 || n_rot > 256 || (n_rot > 0) != (rot_table != nullptr) || (n_rot > 0) != (rot_out != nullptr))
    return fail(nullptr, MI_ERR_ARG, "mi_draw_tasks: rot_table and rot_out go with 1 <= n_rot <= 256, NULL with n_rot == 0");
  if (num_tasks >> 32) return fail(nullptr, MI_ERR_ARG, "mi_draw_tasks: num_tasks must be below 2^32");
  HIPCHK0(launch_draw_tasks(reinterpret_cast<hipStream_t>(stream), class_offsets, class_index, n_classes, ways, k, rot_table, n_rot,
                            remap_shuffle, seed, first_slot, num_tasks, tasks, index_out, labels_out, rot_out, task_id_out));
  return MI_OK;
}

extern "C" int mi_conv3x3_bn_stats(void* stream, const float* x, const float* w9, size_t pstride, int tasks, int n, int h,
                                   int wd, int ci, int co, int stride, float* z, float* mu, float* rstd, void* scratch,
                                   size_t scratch_bytes) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ConvArgs ca{};
  ca.in[0] = x; ca.wt[0] = w9; ca.wstride = pstride; ca.out = z;
  ca.partial = reinterpret_cast<double*>(scratch);
  ca.g = ConvGeom{n, h, wd, (h - 1) / stride + 1, (wd - 1) / stride + 1, ci, co, stride};
  ca.mpix = n * ca.g.ho * ca.g.wo;
  if ((size_t)tasks * conv_max_blocks_per_task(ca.g) * 2 * co * sizeof(double) > scratch_bytes)
    return fail(nullptr, MI_ERR_WORKSPACE, "scratch too small");
  hipError_t aerr = hipSuccess;      // (fp16 operand form: the input's largest magnitude per task, a reduction launch of its own here)
  ca.amax[0] = standalone_amax(st, 0, x, (size_t)n * h * wd * ci, tasks, &aerr);
  HIPCHK0(aerr);
  int blk = 0;
  HIPCHK0(launch_conv3x3(st, ca, tasks, 1, EPI_STATS, 0, &blk));
  HIPCHK0(launch_bn_finalize(st, ca.partial, blk, tasks, co, 1.0 / (double)ca.mpix, FIN_STATS, mu, co, rstd, co));
  return MI_OK;
}

extern "C" int mi_bn_relu_pool(void* stream, const float* z, const float* mu, const float* rstd, const float* gamma,
                               const float* beta, size_t pstride, int tasks, int n, int ho, int wo, int c, int pool, float* p) {
  BnArgs ba{};
  ba.z = z; ba.mu = mu; ba.rstd = rstd; ba.gamma = gamma; ba.beta = beta; ba.pstride = pstride; ba.out = p;
  ba.n = n; ba.ho = ho; ba.wo = wo; ba.c = c;
  HIPCHK0(launch_bn_fwd(reinterpret_cast<hipStream_t>(stream), ba, tasks, pool));
  return MI_OK;
}

extern "C" int mi_bn_relu_pool_bwd(void* stream, const float* z, const float* mu, const float* rstd, const float* gamma,
                                   const float* beta, size_t pstride, const float* dp, int tasks, int n, int ho, int wo, int c,
                                   int pool, float* dgamma, float* dbeta, size_t gstride, float* dz, void* scratch,
                                   size_t scratch_bytes) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BnArgs ba{};
  ba.z = z; ba.mu = mu; ba.rstd = rstd; ba.gamma = gamma; ba.beta = beta; ba.pstride = pstride; ba.dp = dp;
  ba.partial = reinterpret_cast<double*>(scratch);
  ba.n = n; ba.ho = ho; ba.wo = wo; ba.c = c;
  ba.inv_m = 1.f / (float)(n * ho * wo);
  if ((size_t)tasks * bn_blocks_per_task(n, ho, wo, c, pool, tasks) * 2 * c * sizeof(double) > scratch_bytes)
    return fail(nullptr, MI_ERR_WORKSPACE, "scratch too small");
  int blk = 0;
  HIPCHK0(launch_bn_bwd_reduce(st, ba, tasks, pool, &blk));
  HIPCHK0(launch_bn_finalize(st, ba.partial, blk, tasks, c, 1.0, FIN_SUMS, dgamma, gstride, dbeta, gstride));
  ba.dgamma = dgamma; ba.dbeta = dbeta; ba.gstride = gstride; ba.out = dz;
  HIPCHK0(launch_bn_bwd_apply(st, ba, tasks, pool));
  return MI_OK;
}

extern "C" int mi_conv3x3_bwd(void* stream, const float* x, const float* dz, const float* w9, size_t pstride, int tasks, int n,
                              int h, int wd, int ci, int co, int stride, float* dx, float* dw9, size_t gstride, void* scratch,
                              size_t scratch_bytes) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int ho = (h - 1) / stride + 1, wo = (wd - 1) / stride + 1;
  WgradArgs wa{};
  wa.x[0] = x; wa.dz[0] = dz; wa.partial = reinterpret_cast<float*>(scratch);
  wa.g = ConvGeom{n, h, wd, ho, wo, ci, co, stride};
  wa.mpix = n * ho * wo;
  if (wgrad_partial_floats(wa.g, tasks) * sizeof(float) > scratch_bytes) return fail(nullptr, MI_ERR_WORKSPACE, "scratch too small");
  hipError_t aerr = hipSuccess;
  wa.amax_x[0] = standalone_amax(st, 0, x, (size_t)n * h * wd * ci, tasks, &aerr);
  HIPCHK0(aerr);
  wa.amax_dz[0] = standalone_amax(st, 1, dz, (size_t)n * ho * wo * co, tasks, &aerr);
  HIPCHK0(aerr);
  int nch = 0;
  HIPCHK0(launch_wgrad3x3(st, wa, tasks, 1, &nch));
  HIPCHK0(launch_wgrad_reduce(st, wa.partial, nch, 9 * ci * co, tasks, dw9, gstride));
  if (dx) {
    ConvArgs ca{};
    ca.in[0] = dz; ca.wt[0] = w9; ca.wstride = pstride; ca.out = dx;
    ca.amax[0] = wa.amax_dz[0];
    ca.g = ConvGeom{n, ho, wo, h, wd, co, ci, stride};
    ca.mpix = n * h * wd;
    HIPCHK0(launch_conv3x3(st, ca, tasks, 1, EPI_NONE, 1, nullptr));
  }
  return MI_OK;
}

extern "C" int mi_head_fwd_bwd(void* stream, const float* f, const float* wl, const float* bl, size_t pstride, const int32_t* y,
                               int tasks, int n, int feat, int ways, float* loss, float* acc, float* logits, float* prob,
                               float* dl, float* dwl, float* dbl, size_t gstride, float* df) {
  HeadArgs ha{};
  ha.f = f; ha.wl = wl; ha.bl = bl; ha.pstride = pstride; ha.y = y; ha.loss = loss; ha.acc = acc; ha.logits = logits;
  ha.prob = prob; ha.dl = dl; ha.dwl = dwl; ha.dbl = dbl; ha.gstride = gstride; ha.df = df;
  ha.n = n; ha.feat = feat; ha.ways = ways;
  if (!df || (size_t)feat < 2) return fail(nullptr, MI_ERR_ARG, "mi_head_fwd_bwd needs df (its first 2*tasks*n floats double as row scratch)");
  if (tasks < 1 || n < 1 || ways < 1 || ways > 64) return fail(nullptr, MI_ERR_ARG, "mi_head_fwd_bwd: tasks, n >= 1 and ways in 1..64");
  if (dwl) HEAD_LDS(nullptr, "mi_head_fwd_bwd", n, ways, 0);      // (before the rows launch: a refused call launches nothing)
  ha.rowloss = df; ha.rowhit = df + (size_t)tasks * n;   // consumed by the reduce launch before the gradient launch overwrites df
  // (the engine's own passes give the rows kernel separate scratch and let the gradient launch fold loss / acc; here the row
  // scratch aliases df, so the three launches stay separate)
  HIPCHK0(launch_head_fwd_bwd(reinterpret_cast<hipStream_t>(stream), ha, tasks, 0));
  if (dwl) {
    ha.loss = nullptr; ha.acc = nullptr;
    HIPCHK0(launch_head_grads(reinterpret_cast<hipStream_t>(stream), ha, tasks));
  }
  return MI_OK;
}

// launch_metric_head: the metric heads' kernel entry (include/mi_maml.h).  Everything is folded inside the one launch: no scratch.
extern "C" size_t mi_metric_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways) {
  (void)tasks; (void)ns; (void)nq; (void)feat; (void)ways;
  return 0;
}
extern "C" int mi_metric_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq, int tasks, int ns, int nq,
                              int feat, int ways, int metric, float scale, float* loss, float* acc, float* logits, float* dfs, float* dfq,
                              void* scratch, size_t scratch_bytes) {
  (void)scratch; (void)scratch_bytes;
  MetricArgs ma = closed_form_args<MetricArgs>(fs, fq, ys, yq, ns, nq, feat, ways, loss, acc, logits, dfs, dfq);
  ma.h = {metric, scale};
  if (const int rc = closed_form_entry_check("mi_metric_head", false, ma, tasks, [&] { return metric_hyper_check(nullptr, "mi_metric_head", metric, scale); }))
    return rc;
  HIPCHK0(launch_metric_head(reinterpret_cast<hipStream_t>(stream), ma, tasks));
  return MI_OK;
}

// launch_ridge_head: the ridge head's kernel entry (include/mi_maml.h), likewise.
extern "C" size_t mi_ridge_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways) {
  return mi_metric_head_scratch_bytes(tasks, ns, nq, feat, ways);
}
extern "C" int mi_ridge_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq, int tasks, int ns, int nq,
                             int feat, int ways, float lam, float alpha, float* loss, float* acc, float* logits, float* dfs, float* dfq,
                             float* dhyper, void* scratch, size_t scratch_bytes) {
  (void)scratch; (void)scratch_bytes;
  RidgeArgs ra = closed_form_args<RidgeArgs>(fs, fq, ys, yq, ns, nq, feat, ways, loss, acc, logits, dfs, dfq);
  ra.h = {lam, alpha};
  ra.dhyper = dhyper;
  if (const int rc = closed_form_entry_check("mi_ridge_head", true, ra, tasks, [&] { return ridge_hyper_check(nullptr, "mi_ridge_head", lam, alpha); }))
    return rc;
  HIPCHK0(launch_ridge_head(reinterpret_cast<hipStream_t>(stream), ra, tasks));
  return MI_OK;
}

// launch_logreg_head: the logistic-regression head's kernel entry (include/mi_maml.h), likewise.
extern "C" size_t mi_logreg_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways) {
  return mi_metric_head_scratch_bytes(tasks, ns, nq, feat, ways);
}
extern "C" int mi_logreg_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq, int tasks, int ns, int nq,
                              int feat, int ways, float lam, float alpha, float* loss, float* acc, float* logits, float* dfs, float* dfq,
                              float* dhyper, void* scratch, size_t scratch_bytes) {
  (void)scratch; (void)scratch_bytes;
  LogregArgs la = closed_form_args<LogregArgs>(fs, fq, ys, yq, ns, nq, feat, ways, loss, acc, logits, dfs, dfq);
  la.h = {lam, alpha};
  la.dhyper = dhyper;
  if (const int rc = closed_form_entry_check("mi_logreg_head", CF_LOGREG, la, tasks, [&] { return ridge_hyper_check(nullptr, "mi_logreg_head", lam, alpha); }))
    return rc;
  HIPCHK0(launch_logreg_head(reinterpret_cast<hipStream_t>(stream), la, tasks));
  return MI_OK;
}

// launch_proto_init / launch_proto_init_bwd: the Proto-MAML initialisation's kernel entries (include/mi_maml.h).
static int proto_init_entry_check(const char* who, const ProtoInitArgs& a, int tasks) {
  if (!proto_init_fits(tasks, a.ns, a.feat, a.ways)) return proto_init_size_fail(nullptr, who, tasks, a.ns, a.feat, a.ways);
  if (!(a.scale > 0.f) || !std::isfinite(a.scale))
    return fail(nullptr, MI_ERR_ARG, std::string(who) + ": scale must be positive and finite, got " + std::to_string(a.scale));
  if (a.stride < (size_t)a.ways * a.feat + a.ways)
    return fail(nullptr, MI_ERR_ARG, std::string(who) + ": the stride between the tasks' heads, " + std::to_string(a.stride) + ", is below ways * feat + ways = " +
                                         std::to_string((size_t)a.ways * a.feat + a.ways));
  return MI_OK;
}
extern "C" int mi_proto_init(void* stream, const float* fs, const int32_t* ys, int tasks, int ns, int feat, int ways, float scale,
                             float* head_out, size_t head_stride) {
  if (!fs || !ys || !head_out) return fail(nullptr, MI_ERR_ARG, "mi_proto_init: null pointer argument");
  ProtoInitArgs a{};
  a.fs = fs; a.ys = ys; a.ns = ns; a.feat = feat; a.ways = ways; a.scale = scale; a.stride = head_stride; a.head = head_out;
  if (const int rc = proto_init_entry_check("mi_proto_init", a, tasks)) return rc;
  HIPCHK0(launch_proto_init(reinterpret_cast<hipStream_t>(stream), a, tasks));
  return MI_OK;
}
extern "C" int mi_proto_init_bwd(void* stream, const float* fs, const int32_t* ys, const float* lam_head, size_t lam_stride, int tasks, int ns,
                                 int feat, int ways, float scale, float* dfs, float* dscale) {
  if (!fs || !ys || !lam_head || !dfs) return fail(nullptr, MI_ERR_ARG, "mi_proto_init_bwd: null pointer argument");
  ProtoInitArgs a{};
  a.fs = fs; a.ys = ys; a.ns = ns; a.feat = feat; a.ways = ways; a.scale = scale; a.stride = lam_stride; a.lam = lam_head; a.dfs = dfs;
  a.dscale = dscale;
  if (const int rc = proto_init_entry_check("mi_proto_init_bwd", a, tasks)) return rc;
  HIPCHK0(launch_proto_init_bwd(reinterpret_cast<hipStream_t>(stream), a, tasks));
  return MI_OK;
}

// launch_head_grads alone: dWl, dbl, df (may be NULL) from given dlogits
extern "C" int mi_head_grads(void* stream, const float* f, const float* wl, size_t pstride, const float* dl, int tasks, int n, int feat,
                             int ways, float* dwl, float* dbl, size_t gstride, float* df) {
  if (!f || !wl || !dl || !dwl || !dbl || tasks < 1 || n < 1 || feat < 1 || ways < 1 || ways > 64)
    return fail(nullptr, MI_ERR_ARG, "mi_head_grads: null pointer, or tasks / n / feat < 1, or ways outside 1..64");
  HEAD_LDS(nullptr, "mi_head_grads", n, ways, 0);
  HeadArgs ha{};
  ha.f = f; ha.wl = wl; ha.pstride = pstride; ha.dl = const_cast<float*>(dl);
  ha.dwl = dwl; ha.dbl = dbl; ha.gstride = gstride; ha.df = df;
  ha.n = n; ha.feat = feat; ha.ways = ways;
  HIPCHK0(launch_head_grads(reinterpret_cast<hipStream_t>(stream), ha, tasks));
  return MI_OK;
}

// launch_head_tangent: the rows launch (logit tangents, R{dlogits}) and the gradient launch (R{dWl}, R{dbl}, R{df})
extern "C" int mi_head_tangent(void* stream, const float* f, const float* fd, const float* wl, const float* bl, size_t pstride,
                               const float* wld, const float* bld, size_t vstride, const float* prob, const float* dl, float* rdl,
                               float* ld_out, int fixed_dl, int tasks, int n, int feat, int ways, float* dwl, float* dbl,
                               size_t gstride, float* df) {
  if (!f || !wl || !bl || !wld || !bld || !dl || !rdl || !dwl || !dbl || (!fixed_dl && !prob) || tasks < 1 || n < 1 || feat < 1 || ways < 1 || ways > 64)
    return fail(nullptr, MI_ERR_ARG, "mi_head_tangent: null pointer, or tasks / n / feat < 1, or ways outside 1..64");
  HEAD_LDS(nullptr, "mi_head_tangent", n, ways, 1);
  HeadArgs ha{};
  ha.f = f; ha.fd = fd; ha.wl = wl; ha.bl = bl; ha.pstride = pstride; ha.wld = wld; ha.bld = bld; ha.vstride = vstride;
  ha.prob = const_cast<float*>(prob); ha.dl = const_cast<float*>(dl); ha.rdl = rdl; ha.ld_out = ld_out; ha.fixed_dl = fixed_dl ? 1 : 0;
  ha.dwl = dwl; ha.dbl = dbl; ha.gstride = gstride; ha.df = df;
  ha.n = n; ha.feat = feat; ha.ways = ways;
  HIPCHK0(launch_head_tangent(reinterpret_cast<hipStream_t>(stream), ha, tasks));
  return MI_OK;
}

extern "C" int mi_spatial_mean(void* stream, const float* p, float* f, int rows, int hw, int c) {
  if (!p || !f || rows < 1 || hw < 1 || c < 1) return fail(nullptr, MI_ERR_ARG, "mi_spatial_mean: null pointer or empty shape");
  HIPCHK0(launch_spatial_mean(reinterpret_cast<hipStream_t>(stream), p, f, rows, hw, c));
  return MI_OK;
}
extern "C" int mi_spatial_mean_bwd(void* stream, const float* df, float* dp, int rows, int hw, int c) {
  if (!df || !dp || rows < 1 || hw < 1 || c < 1) return fail(nullptr, MI_ERR_ARG, "mi_spatial_mean_bwd: null pointer or empty shape");
  HIPCHK0(launch_spatial_mean_bwd(reinterpret_cast<hipStream_t>(stream), df, dp, rows, hw, c));
  return MI_OK;
}

// The one-launch tail (tail.hip) on flat pointers.  Scratch layout: [arrival counters: tasks x u32 | BatchNorm partials (fp64) | dWl partials |
// per-row scalars | R{dlogits} | row loss | row hit], every part on a 256-byte boundary.  The counters come first and are the CALLER's to zero
// once (the kernels leave them at zero).
namespace {
struct TailCarve { size_t counter, bpart, wpart, scr, rdl, rowloss, rowhit, bytes; };
TailCarve tail_carve_host(int tasks, int n, int c, int feat, int ways) {
  TailCarve k{};
  size_t off = 0;
  auto take = [&](size_t bytes) { off = align_up(off, 256); const size_t at = off; off += bytes; return at; };
  k.counter = take((size_t)tasks * sizeof(unsigned));
  k.bpart = take(tail_bpart_doubles(tasks, c) * sizeof(double));
  k.wpart = take(tail_wpart_floats(tasks, feat, ways) * sizeof(float));
  k.scr = take(tail_scr_floats(tasks, n, ways) * sizeof(float));
  k.rdl = take((size_t)tasks * n * ways * sizeof(float));
  k.rowloss = take((size_t)tasks * n * sizeof(float));
  k.rowhit = take((size_t)tasks * n * sizeof(float));
  k.bytes = align_up(off, 256);
  return k;
}
int tail_feat(int ho, int wo, int c, int pool) { return (pool ? (ho / 2) * (wo / 2) : ho * wo) * c; }
}  // namespace

extern "C" int mi_tail_supported(int n, int ho, int wo, int c, int pool, int feat, int ways) {
  return tail_supported(n, ho, wo, c, pool, feat, ways) ? 1 : 0;
}
extern "C" size_t mi_tail_lds_bytes(int n, int feat, int ways, int tangent) {
  return (n < 1 || feat < 1 || ways < 1) ? 0 : tail_lds_bytes_host(n, feat, ways, tangent ? 1 : 0);
}
extern "C" size_t mi_tail_scratch_bytes(int tasks, int n, int ho, int wo, int c, int pool, int ways) {
  if (tasks < 1 || n < 1 || ho < 1 || wo < 1 || c < 1 || ways < 1) return 0;
  return tail_carve_host(tasks, n, c, tail_feat(ho, wo, c, pool), ways).bytes;
}
extern "C" int mi_tail_run(void* stream, const mi_tail_args* a, int tangent, void* scratch, size_t scratch_bytes) {
  if (!a || !scratch) return fail(nullptr, MI_ERR_ARG, "mi_tail_run: null argument");
  const int T = a->tasks, n = a->n, c = a->c, ways = a->ways;
  if (T < 1 || T > 65535 || n < 1 || a->ho < 1 || a->wo < 1 || c < 1 || ways < 1) return fail(nullptr, MI_ERR_ARG, "mi_tail_run: empty shape, or more than 65535 tasks");
  const int feat = tail_feat(a->ho, a->wo, c, a->pool);
  if (!tail_supported(n, a->ho, a->wo, c, a->pool, feat, ways))
    return fail(nullptr, MI_ERR_ARG, "mi_tail_run: the one-launch tail does not take n = " + std::to_string(n) + ", map " + std::to_string(a->ho) + " x " +
                                         std::to_string(a->wo) + " x " + std::to_string(c) + (a->pool ? " (pooled)" : "") + ", ways = " + std::to_string(ways) +
                                         " (tail_supported, csrc/tail.hip)");
  if (a->pstride % 4 || a->vstride % 4 || a->gstride % 4)
    return fail(nullptr, MI_ERR_ARG, "mi_tail_run: the per-task strides must be multiples of 4 floats (16-byte loads of the BatchNorm vectors, 16-byte stores of dWl)");
  const bool primal = !tangent;
  if (!a->z || !a->mu || !a->rstd || !a->gamma || !a->beta || !a->wl || !a->bl || !a->pooled || !a->prob || !a->dl ||
      (primal && (!a->y || !a->loss || !a->acc)) ||
      ((tangent || a->with_grad) && (!a->dwl || !a->dbl || !a->df || !a->sum0 || !a->sum1)) ||
      (tangent && (!a->zd || !a->m1 || !a->m2 || !a->gammad || !a->betad || !a->wld || !a->bld || !a->f || !a->dp)))
    return fail(nullptr, MI_ERR_ARG, "mi_tail_run: null pointer argument");
  const TailCarve k = tail_carve_host(T, n, c, feat, ways);
  if (scratch_bytes < k.bytes) return fail(nullptr, MI_ERR_WORKSPACE, "mi_tail_run: scratch too small: need " + std::to_string(k.bytes) + " bytes");
  char* sb = reinterpret_cast<char*>(scratch);
  TailArgs ta{};
  BnArgs& ba = ta.bn;
  ba.z = a->z; ba.zd = a->zd; ba.mu = a->mu; ba.rstd = a->rstd; ba.m1 = a->m1; ba.m2 = a->m2;
  ba.gamma = a->gamma; ba.beta = a->beta; ba.pstride = a->pstride;
  ba.gammad = a->gammad; ba.betad = a->betad; ba.vstride = a->vstride;
  ba.dp = a->dp;
  ba.n = n; ba.ho = a->ho; ba.wo = a->wo; ba.c = c;
  ba.inv_m = 1.f / (float)(n * a->ho * a->wo);
  HeadArgs& ha = ta.hd;
  ha.f = a->f;
  ha.wl = a->wl; ha.bl = a->bl; ha.pstride = a->pstride;
  ha.wld = a->wld; ha.bld = a->bld; ha.vstride = a->vstride;
  ha.y = a->y; ha.loss = a->loss; ha.acc = a->acc; ha.logits = a->logits; ha.prob = a->prob; ha.dl = a->dl;
  ha.dwl = a->dwl; ha.dbl = a->dbl; ha.gstride = a->gstride; ha.df = a->df;
  ha.rdl = reinterpret_cast<float*>(sb + k.rdl);
  ha.rowloss = reinterpret_cast<float*>(sb + k.rowloss);
  ha.rowhit = reinterpret_cast<float*>(sb + k.rowhit);
  ha.n = n; ha.feat = feat; ha.ways = ways;
  ta.pooled = a->pooled;
  ta.sum0 = a->sum0; ta.sum1 = a->sum1; ta.sum_stride = a->gstride;
  ta.with_grad = tangent ? 1 : (a->with_grad ? 1 : 0);
  ta.bwd_tasks = tangent ? T : a->bwd_tasks;
  ta.counter = reinterpret_cast<unsigned*>(sb + k.counter);
  ta.bpart = reinterpret_cast<double*>(sb + k.bpart);
  ta.wpart = reinterpret_cast<float*>(sb + k.wpart);
  ta.scr = reinterpret_cast<float*>(sb + k.scr);
  HIPCHK0(launch_tail(reinterpret_cast<hipStream_t>(stream), ta, T, a->pool ? 1 : 0, tangent ? 1 : 0));
  return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-launch profiling with HIP events on the caller's stream (used by bench.py for the roofline figures).
extern "C" int mi_profile_enable(mi_engine* e, int on, int kind_filter) {
  if (!e) return MI_ERR_ARG;
  e->prof_on = on;
  e->prof_filter = kind_filter;
  e->ev_used = 0;
  return MI_OK;
}
extern "C" int mi_profile_kinds(void) { return OP_COUNT * 8; }
extern "C" const char* mi_profile_op_name(int op) { return (op >= 0 && op < OP_COUNT) ? kOpNames[op] : "?"; }
// Sums elapsed ms / launch counts per kind (= op*8 + layer) since the last collect; blocks until the events completed.
extern "C" int mi_profile_collect(mi_engine* e, double* total_ms, int64_t* count, int n_kinds) {
  if (!e || !total_ms || !count || n_kinds < OP_COUNT * 8) return MI_ERR_ARG;
  for (int i = 0; i < n_kinds; ++i) { total_ms[i] = 0.0; count[i] = 0; }
  for (size_t i = 0; i < e->ev_used; ++i) {
    if (hipEventSynchronize(e->ev1[i]) != hipSuccess) return fail(e, MI_ERR_HIP, "hipEventSynchronize failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->ev0[i], e->ev1[i]) != hipSuccess) return fail(e, MI_ERR_HIP, "hipEventElapsedTime failed");
    total_ms[e->ev_kind[i]] += ms;
    count[e->ev_kind[i]] += 1;
  }
  e->ev_used = 0;
  return MI_OK;
}
