// Step-wise policy learner: the mean of the DiagNormalPolicy, loc = MLP(theta; states), as a twice-differentiable unit
// (the policy-side mirror of mi_learner_backward / mi_learner_hvp).  With cotangents dloc [T][B][A] and
//   s_t(theta_t) = sum_{row < count[t]} sum_a loc * dloc
//   mi_policy_vjp : grad[t] = d s_t / d theta_t                            (sigma slots exact zeros)
//   mi_policy_hvp : hv[t]   = (d^2 s_t / d theta^2) v_t, dloc held fixed;  loc_dot[t] = J_t v_t  (zero on rows past count[t])
// sigma -> scale, the Normal and every loss on top stay torch ops.  Two paths:
//   per-layer : mlp_forward / mlp_backward / mlp_tangent_forward / mlp_tangent_backward of policy.hip on masked copies of the
//               states and cotangents, ~10 launches per VJP and ~20 per HVP, every shape mi_policy_create accepts;
//   fused     : one sweep + one fold.  A workgroup owns slabs w, w + nwg, ... of ONE task and takes each slab of R rows through
//               the whole chain -- forward, backward, the weight-gradient products and, for the HVP, tangent forward and tangent
//               backward -- with W2 (and the direction's V2) resident in LDS for its lifetime (2 x 64 KiB at H = 128), the slab's
//               activations in LDS and every weight-gradient accumulator in registers across its slabs.  Only loc_dot rows and
//               one partial per (workgroup, task) are written; the fold sums a task's partials in workgroup order.  nwg depends
//               on the batch length alone, so a task's bits do not depend on how many tasks share the call.
// Exact fp32 (fmaf chains on the vector unit: the chain is latency / launch bound at these widths, not FLOP bound).
#include <string>
#include "mi_common.h"
#include "../../include/mi_maml.h"
#include "policy_layers.h"

#define PL_MAX_H 128
#define PL_MAX_S 16
#define PL_MAX_A 6
#define PL_DL 8              // row pitch of the cotangent slab in LDS
#define PL_WG_PER_TASK 64    // workgroups (= partials) per task at most
#define PL_R_VJP 16          // rows per slab
#define PL_R_HVP 8

struct PLArgs {
  const float* theta; size_t tstride;
  const float* v;            // [T][P] direction (HVP)
  const float* x;            // [T][B][S]
  const float* dloc;         // [T][B][A]
  const int32_t* count;      // [T] or null
  float* partial;            // [T][nwg][P]
  float* loc_dot;            // [T][B][A] (HVP)
  int T, B, S, A, H1, H2, act, head_only, nwg;
  int o_w1, o_b1, o_w2, o_b2, o_w3, o_b3, P;
};

__device__ __forceinline__ float pl_act(float z, int act) { return act == ACT_TANH ? tanhf(z) : fmaxf(z, 0.f); }
// phi'(z) from h = phi(z)
__device__ __forceinline__ float pl_gate(float h, int act) { return act == ACT_TANH ? 1.f - h * h : (h > 0.f ? 1.f : 0.f); }
// W2[o][i] in LDS: rows of 128 floats, the 16-byte chunk index XORed with the row: lanes that own consecutive rows read the same
// reduction chunk from different banks (forward), lanes that own consecutive columns read one row's chunks as a permutation (backward)
__device__ __forceinline__ int pl_swz(int o, int i) { return o * PL_MAX_H + ((((i >> 2) ^ (o & 31)) << 2) | (i & 3)); }
__device__ __forceinline__ float pl_dot4(float4 a, float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

template <bool HVP, int R>
__global__ __launch_bounds__(256) void policy_learner_sweep_kernel(PLArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HS = PL_MAX_H, RT = R / 2;
  static_assert(R * PL_MAX_S <= 256 && R * PL_DL <= 256 && R * PL_MAX_A <= 256, "slab loads are one element per thread");
  float* cur = lds;
  float* w2s = cur; cur += HS * HS;
  float* v2s = cur; if (HVP) cur += HS * HS;
  float* h1s = cur; cur += R * HS;
  float* h1d = cur; if (HVP) cur += R * HS;
  float* h2s = cur; cur += R * HS;          // h2, later the cotangent of layer 1 (d1 / R{d1}) for the W1 product
  float* h2d = cur; if (HVP) cur += R * HS;
  float* d2s = cur; cur += R * HS;
  float* r2s = cur; if (HVP) cur += R * HS;
  float* xs = cur; cur += R * PL_MAX_S;
  float* dls = cur;

  const int tid = threadIdx.x, t = blockIdx.y, wg = blockIdx.x;
  const int c = tid & 127, rg = tid >> 7;   // column owner of the layer stages, its half of the slab's rows
  const int S = a.S, A = a.A, H1 = a.H1, H2 = a.H2, B = a.B, act = a.act;
  const bool body = !a.head_only;
  const float* th = a.theta + (size_t)t * a.tstride;
  const float* vv = HVP ? a.v + (size_t)t * a.P : nullptr;
  int n = a.count ? a.count[t] : B;
  n = n < 0 ? 0 : (n > B ? B : n);

  for (int e = tid; e < HS * HS; e += 256) {
    const int o = e >> 7, i = e & 127;
    const bool ok = o < H2 && i < H1;
    w2s[pl_swz(o, i)] = ok ? th[a.o_w2 + o * H1 + i] : 0.f;
    if (HVP) v2s[pl_swz(o, i)] = (ok && body) ? vv[a.o_w2 + o * H1 + i] : 0.f;
  }

  float acc2[8][8];                          // W2 block: rows 8 (tid >> 4) .., columns 8 (tid & 15) ..
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int w = 0; w < 8; ++w) acc2[u][w] = 0.f;
  float acc1[8], acc3[3], accb1 = 0.f, accb2 = 0.f, accb3 = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) acc1[u] = 0.f;
#pragma unroll
  for (int u = 0; u < 3; ++u) acc3[u] = 0.f;
  const int to = (tid >> 4) * 8, ti = (tid & 15) * 8;
  __syncthreads();

  for (int slab = wg; slab * R < B; slab += a.nwg) {
    const int row0 = slab * R;
    if (row0 >= n) {                         // nothing valid (uniform over the workgroup): loc_dot rows are zero
      if (HVP && tid < R * A) {
        const int b = tid / A, row = row0 + b;
        if (row < B) a.loc_dot[((size_t)t * B + row) * A + (tid - b * A)] = 0.f;
      }
      continue;
    }
    // ---- the slab: states and cotangents, rows past count as zeros (they then contribute exact zeros everywhere)
    if (tid < R * PL_MAX_S) {
      const int b = tid / PL_MAX_S, s = tid % PL_MAX_S, row = row0 + b;
      xs[tid] = (row < n && s < S) ? a.x[((size_t)t * B + row) * S + s] : 0.f;
    }
    if (tid < R * PL_DL) {
      const int b = tid / PL_DL, d = tid % PL_DL, row = row0 + b;
      dls[tid] = (row < n && d < A) ? a.dloc[((size_t)t * B + row) * A + d] : 0.f;
    }
    __syncthreads();
    // ---- layer 1 (and its tangent): K = S
    {
      float z[RT], zd[RT];
      const bool ok = c < H1;
      const float b1 = ok ? th[a.o_b1 + c] : 0.f, vb1 = (HVP && ok && body) ? vv[a.o_b1 + c] : 0.f;
#pragma unroll
      for (int q = 0; q < RT; ++q) { z[q] = b1; zd[q] = vb1; }
      if (ok)
        for (int s = 0; s < S; ++s) {
          const float w = th[a.o_w1 + c * S + s], vw = (HVP && body) ? vv[a.o_w1 + c * S + s] : 0.f;
#pragma unroll
          for (int q = 0; q < RT; ++q) {
            const float xv = xs[(rg * RT + q) * PL_MAX_S + s];
            z[q] = fmaf(w, xv, z[q]);
            if (HVP) zd[q] = fmaf(vw, xv, zd[q]);
          }
        }
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        const float h = ok ? pl_act(z[q], act) : 0.f;
        h1s[(rg * RT + q) * HS + c] = h;
        if (HVP) h1d[(rg * RT + q) * HS + c] = ok ? pl_gate(h, act) * zd[q] : 0.f;
      }
    }
    __syncthreads();
    // ---- layer 2 (and its tangent): K = H1, W2 / V2 rows from LDS in 16-byte chunks
    {
      float z[RT], zd[RT];
      const bool ok = c < H2;
      const float b2 = ok ? th[a.o_b2 + c] : 0.f, vb2 = (HVP && ok && body) ? vv[a.o_b2 + c] : 0.f;
#pragma unroll
      for (int q = 0; q < RT; ++q) { z[q] = b2; zd[q] = vb2; }
      const int nk4 = (H1 + 3) >> 2;
      for (int k4 = 0; k4 < nk4; ++k4) {
        const int wo = c * HS + ((k4 ^ (c & 31)) << 2);
        const float4 w = *reinterpret_cast<const float4*>(w2s + wo);
        float4 vw = make_float4(0.f, 0.f, 0.f, 0.f);
        if (HVP) vw = *reinterpret_cast<const float4*>(v2s + wo);
#pragma unroll
        for (int q = 0; q < RT; ++q) {
          const float4 hv = *reinterpret_cast<const float4*>(h1s + (rg * RT + q) * HS + 4 * k4);
          z[q] = pl_dot4(w, hv, z[q]);
          if (HVP) {
            const float4 hd = *reinterpret_cast<const float4*>(h1d + (rg * RT + q) * HS + 4 * k4);
            zd[q] = pl_dot4(w, hd, pl_dot4(vw, hv, zd[q]));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        const float h = ok ? pl_act(z[q], act) : 0.f;
        h2s[(rg * RT + q) * HS + c] = h;
        if (HVP) h2d[(rg * RT + q) * HS + c] = ok ? pl_gate(h, act) * zd[q] : 0.f;
      }
    }
    __syncthreads();
    // ---- head: loc_dot rows, the W3 / b3 products, and the cotangents of layer 2
    if (HVP && tid < R * A) {
      const int b = tid / A, d = tid - b * A, row = row0 + b;
      if (row < B) {
        float s = 0.f;
        if (row < n) {
          s = vv[a.o_b3 + d];
          for (int j = 0; j < H2; ++j) {
            s = fmaf(vv[a.o_w3 + d * H2 + j], h2s[b * HS + j], s);
            if (body) s = fmaf(th[a.o_w3 + d * H2 + j], h2d[b * HS + j], s);
          }
        }
        a.loc_dot[((size_t)t * B + row) * A + d] = s;
      }
    }
    if (!HVP || body) {
      const float* hsrc = HVP ? h2d : h2s;    // d W3 = dloc (x) h2;  R{d W3} = dloc (x) R{h2}  (R{dloc} = 0)
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int d = rg * 3 + u;
        if (d < A)
          for (int b = 0; b < R; ++b) acc3[u] = fmaf(dls[b * PL_DL + d], hsrc[b * HS + c], acc3[u]);
      }
      if (!HVP && tid < A)
        for (int b = 0; b < R; ++b) accb3 += dls[b * PL_DL + tid];
    }
    if (body) {
      float w3[PL_MAX_A], v3[PL_MAX_A];
      const bool ok = c < H2;
#pragma unroll
      for (int d = 0; d < PL_MAX_A; ++d) {
        w3[d] = (ok && d < A) ? th[a.o_w3 + d * H2 + c] : 0.f;
        v3[d] = (HVP && ok && d < A) ? vv[a.o_w3 + d * H2 + c] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        const int b = rg * RT + q;
        float pre = 0.f, vpre = 0.f;
#pragma unroll
        for (int d = 0; d < PL_MAX_A; ++d) {
          pre = fmaf(w3[d], dls[b * PL_DL + d], pre);
          if (HVP) vpre = fmaf(v3[d], dls[b * PL_DL + d], vpre);
        }
        const float h = h2s[b * HS + c], g = pl_gate(h, act);
        d2s[b * HS + c] = g * pre;
        if (HVP) {
          float r = g * vpre;                                    // R{dz2} = phi' R{dh2} + phi'' zdot dh2
          if (act == ACT_TANH) r = fmaf(-2.f * h * h2d[b * HS + c], pre, r);
          r2s[b * HS + c] = r;
        }
      }
    }
    __syncthreads();
    if (body) {
      // ---- b2, the W2 product (8 x 8 block per thread, both operands 16-byte LDS reads), and the cotangents of layer 1
      if (tid < HS) {
        const float* src = HVP ? r2s : d2s;
        for (int b = 0; b < R; ++b) accb2 += src[b * HS + tid];
      }
      for (int b = 0; b < R; ++b) {
        float dv[8], hv[8], rv[8], hd[8];
        *reinterpret_cast<float4*>(dv) = *reinterpret_cast<const float4*>(d2s + b * HS + to);
        *reinterpret_cast<float4*>(dv + 4) = *reinterpret_cast<const float4*>(d2s + b * HS + to + 4);
        *reinterpret_cast<float4*>(hv) = *reinterpret_cast<const float4*>(h1s + b * HS + ti);
        *reinterpret_cast<float4*>(hv + 4) = *reinterpret_cast<const float4*>(h1s + b * HS + ti + 4);
        if (HVP) {
          *reinterpret_cast<float4*>(rv) = *reinterpret_cast<const float4*>(r2s + b * HS + to);
          *reinterpret_cast<float4*>(rv + 4) = *reinterpret_cast<const float4*>(r2s + b * HS + to + 4);
          *reinterpret_cast<float4*>(hd) = *reinterpret_cast<const float4*>(h1d + b * HS + ti);
          *reinterpret_cast<float4*>(hd + 4) = *reinterpret_cast<const float4*>(h1d + b * HS + ti + 4);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int w = 0; w < 8; ++w) {
            if (HVP) acc2[u][w] = fmaf(dv[u], hd[w], fmaf(rv[u], hv[w], acc2[u][w]));
            else acc2[u][w] = fmaf(dv[u], hv[w], acc2[u][w]);
          }
      }
      float pre[RT], rr[RT];
#pragma unroll
      for (int q = 0; q < RT; ++q) { pre[q] = 0.f; rr[q] = 0.f; }
      const int no4 = (H2 + 3) >> 2;
      for (int o4 = 0; o4 < no4; ++o4) {
        float w[4], vw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          w[u] = w2s[pl_swz(4 * o4 + u, c)];
          vw[u] = HVP ? v2s[pl_swz(4 * o4 + u, c)] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < RT; ++q) {
          const float4 dv = *reinterpret_cast<const float4*>(d2s + (rg * RT + q) * HS + 4 * o4);
          pre[q] = pl_dot4(make_float4(w[0], w[1], w[2], w[3]), dv, pre[q]);
          if (HVP) {
            const float4 rv = *reinterpret_cast<const float4*>(r2s + (rg * RT + q) * HS + 4 * o4);
            rr[q] = pl_dot4(make_float4(vw[0], vw[1], vw[2], vw[3]), dv, pl_dot4(make_float4(w[0], w[1], w[2], w[3]), rv, rr[q]));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        const int b = rg * RT + q;
        const float h = h1s[b * HS + c], g = pl_gate(h, act);
        float o = g * (HVP ? rr[q] : pre[q]);
        if (HVP && act == ACT_TANH) o = fmaf(-2.f * h * h1d[b * HS + c], pre[q], o);
        h2s[b * HS + c] = o;                  // (h2 has no reader left in this slab)
      }
      __syncthreads();
      // ---- W1 / b1 products: thread = (row of W1, half of the state columns)
      for (int b = 0; b < R; ++b) {
        const float dv = h2s[b * HS + c];
        accb1 += dv;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc1[u] = fmaf(dv, xs[b * PL_MAX_S + rg * 8 + u], acc1[u]);
      }
    }
    __syncthreads();
  }

  // ---- this workgroup's partial: every one of the P slots is written exactly once
  float* out = a.partial + ((size_t)t * a.nwg + wg) * a.P;
  const int o_sigma = a.o_w1 - A;
  if (tid < A) { out[o_sigma + tid] = 0.f; out[a.o_b3 + tid] = accb3; }
  if (c < H1) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (rg * 8 + u < S) out[a.o_w1 + c * S + rg * 8 + u] = acc1[u];
    if (rg == 0) out[a.o_b1 + c] = accb1;
  }
  if (tid < H2) out[a.o_b2 + tid] = accb2;
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int w = 0; w < 8; ++w)
      if (to + u < H2 && ti + w < H1) out[a.o_w2 + (to + u) * H1 + ti + w] = acc2[u][w];
  if (c < H2) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (rg * 3 + u < A) out[a.o_w3 + (rg * 3 + u) * H2 + c] = acc3[u];
  }
}

// out[t][p] = sum of the task's partials in workgroup order
__global__ __launch_bounds__(256) void policy_learner_fold_kernel(const float* __restrict__ partial, int nwg, int P, float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const size_t t = blockIdx.y;
  const float* src = partial + t * nwg * (size_t)P + p;
  float s = 0.f;
  for (int w = 0; w < nwg; ++w) s += src[(size_t)w * P];
  out[t * P + p] = s;
}

// dst[t][b][:] = b < count[t] ? src[t][b][:] : 0   (src may be dst)
__global__ __launch_bounds__(256) void policy_learner_mask_kernel(const float* src, float* dst, const int32_t* __restrict__ count, int B,
                                                                  int W, size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t r = e / W;
  const int t = (int)(r / B), b = (int)(r - (size_t)t * B);
  dst[e] = b < count[t] ? src[e] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
static int g_policy_fused_learner = 1;
extern "C" int mi_policy_set_fused_learner(int on) { g_policy_fused_learner = on ? 1 : 0; return MI_OK; }

bool policy_learner_fused_supported(int act, int h1, int h2, int s, int a) {
  return (act == ACT_RELU || act == ACT_TANH) && h1 >= 1 && h1 <= PL_MAX_H && h2 >= 1 && h2 <= PL_MAX_H && s >= 1 && s <= PL_MAX_S &&
         a >= 1 && a <= PL_MAX_A;
}
extern "C" int mi_policy_learner_fused_supported(const mi_policy* p) {
  return p && policy_learner_fused_supported(p->act, p->H1, p->H2, p->S, p->A) ? 1 : 0;
}

template <bool HVP, int R>
static constexpr size_t pl_lds_bytes() {
  return ((size_t)(HVP ? 2 : 1) * PL_MAX_H * PL_MAX_H + (size_t)(HVP ? 6 : 3) * R * PL_MAX_H + R * PL_MAX_S + R * PL_DL) * sizeof(float);
}
static_assert(pl_lds_bytes<true, PL_R_HVP>() <= 160 * 1024 && pl_lds_bytes<false, PL_R_VJP>() <= 160 * 1024, "a CU has 160 KiB of LDS");

struct PLPlan {
  Acts a, ad;                               // primal and tangent activations (the tangent mean is loc_dot_out)
  float *d2, *d1, *pre2, *pre1, *r2, *r1;
  float *xm, *dm, *zero, *g;                // masked states / cotangents, R{dloc} = 0, the primal gradient of the HVP's backward
  float* partial;                           // fused: [T][PL_WG_PER_TASK][P]
  size_t bytes;
};
static void pl_plan(const mi_policy* p, void* ws, int T, int B, PLPlan& pl) {
  PBump b{reinterpret_cast<char*>(ws), 0};
  const size_t TB = (size_t)T * B;
  pl.a.h1 = b.f(TB * p->H1); pl.a.h2 = b.f(TB * p->H2); pl.a.mu = b.f(TB * p->A);
  pl.ad.h1 = b.f(TB * p->H1); pl.ad.h2 = b.f(TB * p->H2); pl.ad.mu = nullptr;
  pl.d2 = b.f(TB * p->H2); pl.d1 = b.f(TB * p->H1); pl.pre2 = b.f(TB * p->H2); pl.pre1 = b.f(TB * p->H1);
  pl.r2 = b.f(TB * p->H2); pl.r1 = b.f(TB * p->H1);
  pl.xm = b.f(TB * p->S); pl.dm = b.f(TB * p->A); pl.zero = b.f(TB * p->A); pl.g = b.f((size_t)T * p->P);
  pl.partial = policy_learner_fused_supported(p->act, p->H1, p->H2, p->S, p->A) ? b.f((size_t)T * PL_WG_PER_TASK * p->P) : nullptr;
  pl.bytes = align_up(b.off, 256);
}
extern "C" int mi_policy_learner_workspace_bytes(const mi_policy* p, int tasks, int batch, size_t* bytes) {
  if (!p || !bytes) return mi_policy_fail(const_cast<mi_policy*>(p), MI_ERR_ARG, "mi_policy_learner_workspace_bytes: null argument");
  if (tasks < 1 || batch < 1)
    return mi_policy_fail(const_cast<mi_policy*>(p), MI_ERR_ARG,
                          "mi_policy_learner_workspace_bytes: tasks = " + std::to_string(tasks) + ", batch = " + std::to_string(batch) + " (both >= 1)");
  PLPlan pl;
  pl_plan(p, nullptr, tasks, batch, pl);
  *bytes = pl.bytes;
  return MI_OK;
}

#define PLCHK(p, call)                                                                                          \
  do {                                                                                                          \
    hipError_t _s = (call);                                                                                     \
    if (_s != hipSuccess) return mi_policy_fail(p, MI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s)); \
  } while (0)

template <bool HVP, int R>
static int pl_launch_fused(mi_policy* p, hipStream_t st, const PLPlan& pl, const float* theta, size_t tstride, const float* states,
                           const float* dloc, const float* v, const int32_t* count, int T, int B, int head_only, float* grad_out,
                           float* loc_dot) {
  static bool attr_set = false;
  constexpr size_t lds = pl_lds_bytes<HVP, R>();
  if (!attr_set) {
    PLCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&policy_learner_sweep_kernel<HVP, R>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  PLArgs a{};
  a.theta = theta; a.tstride = tstride; a.v = v; a.x = states; a.dloc = dloc; a.count = count; a.partial = pl.partial; a.loc_dot = loc_dot;
  a.T = T; a.B = B; a.S = p->S; a.A = p->A; a.H1 = p->H1; a.H2 = p->H2; a.act = p->act; a.head_only = head_only ? 1 : 0;
  a.nwg = ceil_div(B, R) < PL_WG_PER_TASK ? ceil_div(B, R) : PL_WG_PER_TASK;
  a.o_w1 = (int)p->o_w1; a.o_b1 = (int)p->o_b1; a.o_w2 = (int)p->o_w2; a.o_b2 = (int)p->o_b2; a.o_w3 = (int)p->o_w3; a.o_b3 = (int)p->o_b3;
  a.P = (int)p->P;
  hipLaunchKernelGGL((policy_learner_sweep_kernel<HVP, R>), dim3(a.nwg, T), dim3(256), lds, st, a);
  PLCHK(p, hipGetLastError());
  hipLaunchKernelGGL(policy_learner_fold_kernel, dim3(ceil_div(a.P, 256), T), dim3(256), 0, st, pl.partial, a.nwg, a.P, grad_out);
  PLCHK(p, hipGetLastError());
  return MI_OK;
}

static int pl_mask(mi_policy* p, hipStream_t st, const float* src, float* dst, const int32_t* count, int T, int B, int W) {
  const size_t total = (size_t)T * B * W;
  hipLaunchKernelGGL(policy_learner_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, dst, count, B, W, total);
  PLCHK(p, hipGetLastError());
  return MI_OK;
}

static int pl_check(mi_policy* p, const char* who, const void* theta, size_t tstride, const void* states, const void* dloc, int tasks,
                    int batch, const void* out, const void* ws, size_t ws_bytes, PLPlan& pl) {
  if (!p) return mi_policy_fail(nullptr, MI_ERR_ARG, std::string(who) + ": null policy");
  if (!theta || !states || !dloc || !out || !ws) return mi_policy_fail(p, MI_ERR_ARG, std::string(who) + ": null argument");
  if (tasks < 1 || batch < 1)
    return mi_policy_fail(p, MI_ERR_ARG, std::string(who) + ": tasks = " + std::to_string(tasks) + ", batch = " + std::to_string(batch) + " (both >= 1)");
  if (tstride != 0 && tstride != p->P)
    return mi_policy_fail(p, MI_ERR_ARG, std::string(who) + ": tstride = " + std::to_string(tstride) + " (0 or P = " + std::to_string(p->P) + ")");
  pl_plan(p, const_cast<void*>(ws), tasks, batch, pl);
  if (pl.bytes > ws_bytes) return mi_policy_fail(p, MI_ERR_WORKSPACE, std::string(who) + ": workspace too small: need " + std::to_string(pl.bytes));
  return MI_OK;
}

extern "C" int mi_policy_vjp(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* dloc,
                             const int32_t* count, int tasks, int batch, int head_only, float* grad_out, void* workspace,
                             size_t workspace_bytes) {
  PLPlan pl;
  int rc = pl_check(p, "mi_policy_vjp", theta, tstride, states, dloc, tasks, batch, grad_out, workspace, workspace_bytes, pl);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int T = tasks, B = batch;
  if (g_policy_fused_learner && pl.partial)
    return pl_launch_fused<false, PL_R_VJP>(p, st, pl, theta, tstride, states, dloc, nullptr, count, T, B, head_only, grad_out, nullptr);
  const float *x = states, *dl = dloc;
  if (count) {
    if ((rc = pl_mask(p, st, states, pl.xm, count, T, B, p->S))) return rc;
    if ((rc = pl_mask(p, st, dloc, pl.dm, count, T, B, p->A))) return rc;
    x = pl.xm; dl = pl.dm;
  }
  if ((rc = mlp_forward(p, st, T, B, x, theta, tstride, pl.a))) return rc;
  PLCHK(p, hipMemsetAsync(grad_out, 0, (size_t)T * p->P * sizeof(float), st));
  return mlp_backward(p, st, T, B, x, theta, tstride, pl.a, dl, pl.d2, pl.d1, grad_out, nullptr, nullptr, head_only != 0);
}

extern "C" int mi_policy_hvp(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* dloc,
                             const float* v, const int32_t* count, int tasks, int batch, int head_only, float* grad_theta_out,
                             float* loc_dot_out, void* workspace, size_t workspace_bytes) {
  PLPlan pl;
  int rc = pl_check(p, "mi_policy_hvp", theta, tstride, states, dloc, tasks, batch, grad_theta_out, workspace, workspace_bytes, pl);
  if (rc) return rc;
  if (!v || !loc_dot_out) return mi_policy_fail(p, MI_ERR_ARG, "mi_policy_hvp: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int T = tasks, B = batch;
  const size_t P = p->P;
  if (g_policy_fused_learner && pl.partial)
    return pl_launch_fused<true, PL_R_HVP>(p, st, pl, theta, tstride, states, dloc, v, count, T, B, head_only, grad_theta_out, loc_dot_out);
  const float *x = states, *dl = dloc;
  if (count) {
    if ((rc = pl_mask(p, st, states, pl.xm, count, T, B, p->S))) return rc;
    if ((rc = pl_mask(p, st, dloc, pl.dm, count, T, B, p->A))) return rc;
    x = pl.xm; dl = pl.dm;
  }
  if ((rc = mlp_forward(p, st, T, B, x, theta, tstride, pl.a))) return rc;
  PLCHK(p, hipMemsetAsync(grad_theta_out, 0, (size_t)T * P * sizeof(float), st));
  if (head_only) {            // loc_dot = V3 h2 + vb3; the body is constant, so s is linear in theta: no curvature
    PLCHK(p, dense_fwd(st, T, B, p->H2, p->A, pl.a.h2, v + p->o_w3, P, nullptr, nullptr, 0, v + p->o_b3, P, nullptr, ACT_NONE, loc_dot_out));
  } else {
    if ((rc = mlp_backward(p, st, T, B, x, theta, tstride, pl.a, dl, pl.d2, pl.d1, pl.g, pl.pre2, pl.pre1, false))) return rc;
    Acts ad = pl.ad;
    ad.mu = loc_dot_out;
    if ((rc = mlp_tangent_forward(p, st, T, B, x, theta, tstride, pl.a, v, ad))) return rc;
    PLCHK(p, hipMemsetAsync(pl.zero, 0, (size_t)T * B * p->A * sizeof(float), st));
    if ((rc = mlp_tangent_backward(p, st, T, B, x, theta, tstride, pl.a, ad, v, dl, pl.d2, pl.d1, pl.pre2, pl.pre1, pl.zero, pl.r2, pl.r1,
                                   grad_theta_out)))
      return rc;
  }
  if (count) return pl_mask(p, st, loc_dot_out, loc_dot_out, count, T, B, p->A);
  return MI_OK;
}
