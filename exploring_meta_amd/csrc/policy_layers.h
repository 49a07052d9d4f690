// The per-layer passes of the policy MLP (policy.hip), shared with the files that compose them (policy_learner.hip): one dense
// launch per layer for all tasks.  theta / v with a per-task stride in floats (0 = shared); every array [T][B][.].
#pragma once
#include "mi_common.h"
#include "policy_handle.h"

struct Acts { float *h1, *h2, *mu; };        // post-activation hidden layers (phi' is formed from them) and the mean
struct PBump {
  char* base; size_t off;
  float* f(size_t n) { off = align_up(off, 256); float* r = base ? reinterpret_cast<float*>(base + off) : nullptr; off += n * 4; return r; }
};

hipError_t dense_fwd(hipStream_t st, int T, int B, int I, int O, const float* x0, const float* w0, size_t ws0, const float* x1,
                     const float* w1, size_t ws1, const float* bias, size_t bs, const float* mask, int act, float* y);
int mlp_forward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, Acts& a);
int mlp_backward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, const Acts& a,
                 const float* dmu, float* d2, float* d1, float* g, float* pre2, float* pre1, bool head_only);
int mlp_tangent_forward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, const Acts& a,
                        const float* v, Acts& ad);
int mlp_tangent_backward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, const Acts& a,
                         const Acts& ad, const float* v, const float* dmu, const float* d2, const float* d1, const float* pre2,
                         const float* pre1, const float* rdmu, float* r2, float* r1, float* hv);
