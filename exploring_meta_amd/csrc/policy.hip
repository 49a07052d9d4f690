// MAML-TRPO policy path (BASELINE config 5) for a whole meta-batch of tasks: DiagNormalPolicy MLP (reference
// core_functions/policies.py:30-67, ReLU default) log-prob / gradient / Hessian-vector products, the inner `trpo_update`
// (core_functions/rl.py:361-374), the meta surrogate loss + KL (rl.py:441-473), its gradient and the Fisher-vector product
// used by conjugate gradient (rl.py:413-418) -- replacing per-task PyTorch autograd graphs (create_graph=True) with
// batched-over-tasks kernels and forward-over-reverse tangents.  The dense products (41.6 MFLOP per 2000-row batch forward,
// SURVEY.md a13) run on the fp32 matrix pipe, one launch per layer for all tasks, deterministic reductions.
//
// Parameter vector (reference named_parameters() order): sigma[A], W1[H1][S], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A].
//
// Mathematics (K = 1 inner step, the reference default): theta'_t = theta - lr g_t(theta), g_t = grad of -mean(logp A) on the
// support replay.  surrogate S_t(theta') = -mean(exp(logp_new - logp_old) A), KL_t(theta') = mean KL(new || old) on the query
// replay.   grad_theta mean_t S_t = mean_t (I - lr H_t) grad S_t(theta'_t)          (H_t v: tangent sweep over the support pass)
// At theta_old the adapted policy equals the stored old policy, KL's gradient is exactly zero, so
//   Fvp(v) = mean_t (I - lr H_t) F_t (I - lr H_t) v + damping v,   F_t = J^T diag(1/(B D sigma^2), 2/D) J  (Gaussian Fisher).
// One set of entry points for any number K of inner updates (K = 1 of a supported ReLU policy takes the fused sweeps):
//   MAML-TRPO (new == old, Fisher form exact)          mi_trpo_surrogate_steps / mi_trpo_fvp_steps
//   ANIL-TRPO (new != old, exact Hessian of mean KL)   ... then mi_trpo_kl_prepare_steps / mi_trpo_fvp_general_steps
// Each of them also takes a FIXED step-size table in place of the number lr (mi_policy_adapt_lr, mi_trpo_*_steps_lr: the same
// implementation: its PolicyStep holds the table; the launches differ in step_advance and AdjointWalk only).  lr_vec [rows][P] in the order
// above, shared by all tasks; update k reads row step_lr_row[k] = d_k (mi_policy_adapt_lr's head_only: times the head mask):
//   theta_{k+1} = theta_k - d_k (.) g_k                       J_k = I - D_k H_k
//   tangent  (J_k u):      u_{k+1} = u_k - d_k (.) (H_k u_k)
//   adjoint  (J_k^T lam):  lam_k   = lam_{k+1} - H_k (d_k (.) lam_{k+1})
//   surrogate gradient = mean_t lam_0, lam_K = grad S_t(theta_K);    Fisher form (new == old) = mean_t J^T F_t J v + damping v
//   exact KL Hessian:  rho_K = Hess KL_t(theta_K) u_K,
//                      rho_k = rho_{k+1} - H_k (d_k (.) rho_{k+1}) - T_k[u_k, d_k (.) lam_{k+1}],    product = mean_t rho_0 + damping v
// With one number the tangent and the adjoint recursion are the same operation (jac_apply's order flag); with a vector they are not:
// D H on the adjoint side is wrong.  The adjoint side drives its tangent pass with d (.) x and subtracts what comes back.
#include <string>
#include <vector>
#include <cmath>
#include <climits>
#include "mi_common.h"
#include "../../include/mi_maml.h"

#define HALF_LOG_2PI 0.9189385332046727f

#include "policy_sweep.h"

#define MI_DENSE_TERMS 4   // products summed into one output (2 for first tangents, up to 4 for second tangents)
struct DenseArgs {
  const float* x[MI_DENSE_TERMS];     // [T][B][I]
  const float* w[MI_DENSE_TERMS];     // [O][I] per task (stride wstride[k] floats, 0 = shared)
  size_t wstride[MI_DENSE_TERMS];
  const float* bias;     // [O] (term 0 only), may be null
  size_t bstride;
  const float* mask;     // optional [T][B][O]: stored activations h; output multiplied by phi'(z) written in terms of h
  const float* hd;       // tanh tangent-backward only: tangent activations  [T][B][.]
  const float* dpre;     // tanh tangent-backward only: primal cotangent w.r.t. h (before the phi' factor)
  float* y;              // [T][B][O]
  float* ypre;           // optional: the value before the phi' factor (primal backward of a tanh layer keeps it for the HVP)
  int B, I, O, nterms;
  int act;               // forward: activation applied to the output (ACT_*); mask users: which phi' to form from h
};
#include "policy_handle.h"   // ACT_*, struct mi_policy
#include "policy_layers.h"   // Acts, PBump and the per-layer passes other files compose
// phi'(z) from the stored activation h = phi(z): ReLU -> [h > 0], tanh -> 1 - h^2
__device__ __forceinline__ float act_gate(float s, float h, int act) {
  return act == ACT_TANH ? s * (1.f - h * h) : (h > 0.f ? s : 0.f);
}

// The three dense products of the MLP for ALL tasks in one launch each, on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32 is
// bitwise an fmaf chain, so the parity budget of the fp32 path is untouched).  One wave owns a 32 x 32 output tile; lane half
// h = lane >> 5 takes the upper / lower half of the reduction index, so a lane's A (and, for the forward product, B) operands of
// consecutive MFMAs are consecutive floats of one row.  Rows / columns / reduction indices past the end read zeros.
//   forward   y[b][o]  = sum_k x_k[b][:] . w_k[o][:]          M = B, N = O, K = I     (TRANS_W: B operand = w[n][k])
//   backward  dx[b][i] = sum_k dy_k[b][:] . w_k[:][i]         M = B, N = I, K = O     (B operand = w[k][n])
// followed by the same elementwise epilogues as before (bias / activation / phi' gate / tanh curvature term).
template <bool TRANS_W>
__global__ __launch_bounds__(256) void dense_mfma_kernel(DenseArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int t = blockIdx.y;
  const int N = TRANS_W ? a.O : a.I, Kd = TRANS_W ? a.I : a.O;
  const int nt = (N + 31) >> 5, mt = (a.B + 31) >> 5;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= mt * nt) return;
  const int m0 = (tile / nt) * 32, n0 = (tile % nt) * 32;
  const int Kh = (Kd + 1) >> 1, kbase = h * Kh;
  const int row = m0 + j, col = n0 + j;
  const bool rok = row < a.B, cok = col < N;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int term = 0; term < a.nterms; ++term) {
    const float* xr = a.x[term] + ((size_t)t * a.B + (rok ? row : 0)) * Kd;
    const float* wt = a.w[term] + (size_t)t * a.wstride[term];
    if (Kd % 4 == 0 && Kd >= 16) {
      // 16-byte operand loads: the reduction index is dealt to the two lane halves in groups of four (half h takes k = 8c + 4h .. + 3),
      // so a lane's four consecutive MFMAs read four consecutive floats of its row.  An operand load touches 32 different rows
      // (64 cache lines) whatever its width: the address unit, not the matrix pipe, bounds these products, and twice the width is
      // half the loads.  (Rows are multiples of 16 bytes; weights inside the parameter vector are only 8-byte aligned: dword-aligned
      // vector type.)
      typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
      const int nch = (Kd + 7) >> 3;
#ifndef MI_DENSE_CU
#define MI_DENSE_CU 2
#endif
      constexpr int CU = MI_DENSE_CU;                         // chunks (of 4 MFMAs) in flight
      for (int c0 = 0; c0 < nch; c0 += CU) {
        f4u av[CU], bv[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int k = 8 * (c0 + u) + 4 * h;
          const bool kok = (c0 + u < nch) && (k < Kd);
          av[u] = (f4u){0.f, 0.f, 0.f, 0.f}; bv[u] = (f4u){0.f, 0.f, 0.f, 0.f};
          if (kok && rok) av[u] = *reinterpret_cast<const f4u*>(xr + k);
          if (TRANS_W) {
            if (kok && cok) bv[u] = *reinterpret_cast<const f4u*>(wt + (size_t)col * Kd + k);
          } else if (kok && cok) {
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[u][q] = wt[(size_t)(k + q) * N + col];
          }
        }
#pragma unroll
        for (int u = 0; u < CU; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][q], bv[u][q], acc, 0, 0, 0);
      }
      continue;
    }
    constexpr int CH = 10;
    // a lane's consecutive reduction indices are consecutive floats of its row: 8-byte loads where the half-row split keeps them
    // 8-byte aligned (the 100-wide hidden layers: rows of 400 B, halves of 200 B)
    const bool vec2 = (Kd % 2 == 0) && (Kh % 2 == 0) &&
                      ((reinterpret_cast<uintptr_t>(xr + kbase) | (TRANS_W ? reinterpret_cast<uintptr_t>(wt + (size_t)(cok ? col : 0) * Kd + kbase) : 0)) & 7) == 0;
    for (int s0 = 0; s0 < Kh; s0 += CH) {
      float av[CH], bv[CH];
      if (vec2) {
#pragma unroll
        for (int c = 0; c < CH; c += 2) {
          const int k = kbase + s0 + c;
          const bool kok = (s0 + c < Kh) && (k < Kd);               // pairs never straddle Kh or Kd (both even)
          float2 a2 = make_float2(0.f, 0.f), b2 = make_float2(0.f, 0.f);
          if (kok && rok) a2 = *reinterpret_cast<const float2*>(xr + k);
          if (TRANS_W) {
            if (kok && cok) b2 = *reinterpret_cast<const float2*>(wt + (size_t)col * Kd + k);
          } else if (kok && cok) {
            b2.x = wt[(size_t)k * N + col];
            b2.y = wt[(size_t)(k + 1) * N + col];
          }
          av[c] = a2.x; av[c + 1] = a2.y; bv[c] = b2.x; bv[c + 1] = b2.y;
        }
      } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int k = kbase + s0 + c;
          const bool kok = (s0 + c < Kh) && (k < Kd);
          av[c] = (kok && rok) ? xr[k] : 0.f;
          if (TRANS_W) bv[c] = (kok && cok) ? wt[(size_t)col * Kd + k] : 0.f;
          else bv[c] = (kok && cok) ? wt[(size_t)k * N + col] : 0.f;
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bv[c], acc, 0, 0, 0);
    }
  }
  if (!cok) return;
  const float bias = (TRANS_W && a.bias) ? a.bias[(size_t)t * a.bstride + col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (m >= a.B) continue;
    const size_t oi = ((size_t)t * a.B + m) * N + col;
    float s = acc[r] + bias;
    if (TRANS_W) {
      if (a.mask) s = act_gate(s, a.mask[oi], a.act);        // tangent forward: hdot = phi'(z) zdot
      else if (a.act == ACT_RELU) s = fmaxf(s, 0.f);
      else if (a.act == ACT_TANH) s = tanhf(s);
    } else {
      if (a.ypre) a.ypre[oi] = s;
      if (a.mask) {
        const float hh = a.mask[oi];
        s = act_gate(s, hh, a.act);
        // R{dz} = phi' R{dh} + phi'' zdot dh, and for tanh phi'' zdot = -2 h hdot
        if (a.hd) s = fmaf(-2.f * hh * a.hd[oi], a.dpre[oi], s);
      }
    }
    a.y[oi] = s;
  }
}

template <bool TRANS_W>
static void launch_dense(hipStream_t st, int T, const DenseArgs& a) {
  // (an LDS-tiled variant -- 128 rows x all columns per workgroup, 32-wide reduction chunks staged with coalesced loads -- was built
  // and measured: 1.09 ms per Fisher-vector product against 1.01 ms for this kernel with 8-byte operand loads; two barriers per
  // chunk and the staging cost outweigh the better coalescing on these 100-wide layers.  A second variant -- every wave copies its
  // own contiguous 32-row operand blocks into a private LDS slice with 16-byte loads, no barriers, 2 waves per workgroup -- ran the
  // 100x100 forward product in 116 us against 87 us: 25.6 KB of LDS per wave leaves 6 waves per CU and the copy's latency is no
  // longer hidden.  The product is address-unit bound (32 rows per operand load) but short of a kernel that keeps the whole 2x100
  // MLP of a row tile on chip, occupancy is worth more than coalescing here.)
  const int N = TRANS_W ? a.O : a.I;
  hipLaunchKernelGGL(dense_mfma_kernel<TRANS_W>, dim3(ceil_div(ceil_div(a.B, 32) * ceil_div(N, 32), 4), T), dim3(256), 0, st, a);
}

struct DenseWArgs {
  const float* dy[MI_DENSE_TERMS];    // [T][B][O]
  const float* x[MI_DENSE_TERMS];     // [T][B][I]
  float* dw;             // [T][gstride] at offset: [O][I]
  float* db;             // [T][gstride] at offset: [O]  (from dy[0])
  size_t gstride;
  int B, I, O, nterms;
};
// dW[o][i] = sum_k sum_b dy_k[b][o] x_k[b][i] ; db[o] = sum_b dy_0[b][o]:  M = O, N = I + 1 (column I = the bias: a column of
// ones next to x_0), K = B.  One 8-wave workgroup per 32 x 32 tile; wave w takes the row pairs w, w + 8, ... of the batch (both
// operands are coalesced 128-B rows), the 8 partial tiles are folded through LDS in wave order => deterministic.
__global__ __launch_bounds__(512) void dense_wgrad_mfma_kernel(DenseWArgs a) {
  __shared__ float red[8 * 1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int t = blockIdx.y;
  const int N = a.I + 1, nt = (N + 31) >> 5;
  const int m0 = (blockIdx.x / nt) * 32, n0 = (blockIdx.x % nt) * 32;
  const int orow = m0 + j, col = n0 + j;
  const bool ook = orow < a.O, xok = col < a.I, one = col == a.I;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int term = 0; term < a.nterms; ++term) {
    const float* dy = a.dy[term] + (size_t)t * a.B * a.O + (ook ? orow : 0);
    const float* x = a.x[term] + (size_t)t * a.B * a.I + (xok ? col : 0);
    const float onev = (one && term == 0) ? 1.f : 0.f;
    constexpr int CH = 8;
    // (prefetching the next chunk into a second register set was measured: no gain, 1.05 vs 1.01 ms per Fisher-vector product)
    for (int p0 = wave * 2 * CH; p0 < a.B; p0 += 8 * 2 * CH) {      // this wave's chunk of CH row pairs
      float av[CH], bv[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int b = p0 + 2 * c + h;
        const bool bok = b < a.B;
        av[c] = (bok && ook) ? dy[(size_t)b * a.O] : 0.f;
        bv[c] = bok ? (xok ? x[(size_t)b * a.I] : onev) : 0.f;
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bv[c], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[r];
  __syncthreads();
  for (int e = threadIdx.x; e < 1024; e += 512) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) v += red[w * 1024 + e];
    const int r = e >> 6, l = e & 63;
    const int o = m0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), c = n0 + (l & 31);
    if (o >= a.O) continue;
    if (c < a.I) a.dw[(size_t)t * a.gstride + (size_t)o * a.I + c] = v;
    else if (c == a.I) a.db[(size_t)t * a.gstride + o] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct GaussArgs {
  const float* mu;        // [T][B][A]
  const float* mud;       // tangent of mu (tangent / fisher modes)
  const float* rho;       // sigma parameter, per task stride rstride (0 = shared)
  const float* rhod;      // tangent of rho (stride vstride)
  size_t rstride, vstride;
  const float* act;       // [T][B][A]
  const float* adv;       // [T][B]
  const float* old_loc;   // [T][B][A]
  const float* old_scale; // [T][A]
  const int32_t* count;   // [T] valid samples (rows >= count are padding)
  float* coef;            // [T][B]: dL/dlogp per sample (written in modes 0/1, read in mode 2)
  float* dmu;             // [T][B][A]
  float* drho;            // [T][gstride] at offset: [A]
  size_t gstride;
  float* loss;            // [T]
  float* kl;              // [T]
  int B, A, mode;
};
enum { G_A2C = 0, G_SURROGATE = 1, G_TANGENT = 2, G_FISHER = 3 };

// One workgroup per task.
//  G_A2C       L = -mean(logp*adv)                 (rl.py:358)  -> coef, dmu, drho, loss
//  G_SURROGATE L = -mean(exp(logp-logp_old)*adv)   (rl.py:469)  -> coef, dmu, drho, loss ; kl = mean KL(new||old) (rl.py:459-461)
//  G_TANGENT   R{dmu}, R{drho} of the coef-weighted log-prob gradient for tangents (mud, rhod)
//  G_FISHER    cotangent of the KL Hessian at new == old: dmu = mud/(B D sigma^2), drho = 2 rhod / D
__global__ __launch_bounds__(256) void gauss_kernel(GaussArgs a) {
  __shared__ float red[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int B = a.B, A = a.A, cnt = a.count ? a.count[t] : B;
  const float invB = 1.f / (float)cnt, invD = 1.f / (float)A;
  float acc[8];   // loss, kl, drho[0..5]  (A <= 6)
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (int b = tid; b < B; b += 256) {
    const bool valid = b < cnt;
    const size_t ob = (size_t)t * B + b;
    float lp = 0.f, lpo = 0.f, klb = 0.f;
    if (a.mode == G_A2C || a.mode == G_SURROGATE) {
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r);
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        lp += -(df * df) / (2.f * sg * sg) - r - HALF_LOG_2PI;
        if (a.mode == G_SURROGATE) {
          const float so = a.old_scale[(size_t)t * A + d], lo = a.old_loc[ob * A + d];
          const float dfo = a.act[ob * A + d] - lo;
          lpo += -(dfo * dfo) / (2.f * so * so) - logf(so) - HALF_LOG_2PI;
          const float vr = (sg / so) * (sg / so), t1 = (a.mu[ob * A + d] - lo) / so;
          klb += 0.5f * (vr + t1 * t1 - 1.f - logf(vr));
        }
      }
      lp *= invD;
      lpo *= invD;
      float c = 0.f;
      if (valid) {
        const float ad = a.adv[ob];
        if (a.mode == G_A2C) { c = -ad * invB; acc[0] += c * lp; }
        else { const float ratio = expf(lp - lpo); c = -ratio * ad * invB; acc[0] += -ratio * ad * invB; acc[1] += klb * invB * invD; }
      }
      if (a.coef) a.coef[ob] = c;
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        if (a.dmu) a.dmu[ob * A + d] = c * invD * df * iv;
        if (rp > LOG_EPS) acc[2 + d] += c * invD * (df * df * iv - 1.f);
      }
    } else if (a.mode == G_TANGENT) {
      const float c = valid ? a.coef[ob] : 0.f;
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const bool live = rp > LOG_EPS;
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
        const float rd = live ? a.rhod[(size_t)t * a.vstride + d] : 0.f;
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        const float md = a.mud[ob * A + d];
        a.dmu[ob * A + d] = c * invD * (-md * iv - 2.f * df * rd * iv);
        if (live) acc[2 + d] += c * invD * (-2.f * df * md * iv - 2.f * df * df * rd * iv);
      }
    } else {  // G_FISHER
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r);
        a.dmu[ob * A + d] = valid ? a.mud[ob * A + d] * invB * invD / (sg * sg) : 0.f;
      }
    }
  }
  // deterministic block reductions
  for (int k = 0; k < 2 + A; ++k) {
    red[tid] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      if (k == 0 && a.loss) a.loss[t] = red[0];
      if (k == 1 && a.kl) a.kl[t] = red[0];
      if (k >= 2 && a.drho) {
        float v = red[0];
        if (a.mode == G_FISHER) {
          const float rp = a.rho[(size_t)t * a.rstride + (k - 2)];
          v = rp > LOG_EPS ? 2.f * a.rhod[(size_t)t * a.vstride + (k - 2)] * invD : 0.f;
        }
        a.drho[(size_t)t * a.gstride + (k - 2)] = v;
      }
    }
    __syncthreads();
  }
}

__global__ void axpy_bcast_kernel(const float* __restrict__ a, size_t astride, const float* __restrict__ b, float alpha, int p,
                                  float* __restrict__ out) {   // out[t][i] = a[t*astride + i] - alpha b[t][i]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const size_t t = blockIdx.y;
  out[t * p + i] = alpha == 0.f ? a[t * astride + i] : a[t * astride + i] - alpha * b[t * p + i];   // alpha 0: pure broadcast
}
__global__ void mean_tasks_kernel(const float* __restrict__ x, int tasks, int p, float scale, const float* __restrict__ add,
                                  float add_scale, float* __restrict__ out) {   // out[i] = scale*sum_t x[t][i] + add_scale*add[i]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float s = 0.f;
  for (int t = 0; t < tasks; ++t) s += x[(size_t)t * p + i];
  out[i] = s * scale + (add ? add_scale * add[i] : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------
static thread_local std::string g_perr;
int mi_policy_fail(mi_policy* p, int code, const std::string& m) {
  if (p) p->err = m;
  g_perr = m;
  return code;
}
static int pfail(mi_policy* p, int code, const std::string& m) { return mi_policy_fail(p, code, m); }
#define PCHK(p, call)                                                                                 \
  do {                                                                                                \
    hipError_t _s = (call);                                                                           \
    if (_s != hipSuccess) return pfail(p, MI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s)); \
  } while (0)

extern "C" const char* mi_policy_last_error(const mi_policy* p) { return p ? p->err.c_str() : g_perr.c_str(); }

extern "C" int mi_policy_create(const mi_policy_desc* d, int device, mi_policy** out) {
  if (!d || !out) return pfail(nullptr, MI_ERR_ARG, "null argument");
  if (d->state_size < 1 || d->action_size < 1 || d->action_size > 6 || d->hidden1 < 1 || d->hidden2 < 1)
    return pfail(nullptr, MI_ERR_ARG, "unsupported policy sizes (action_size must be 1..6)");
  if (d->activation != 0 && d->activation != 1) return pfail(nullptr, MI_ERR_ARG, "activation must be 0 (ReLU) or 1 (tanh)");
  mi_policy* p = new mi_policy();
  p->d = *d; p->device = device;
  p->act = d->activation == 1 ? ACT_TANH : ACT_RELU;
  p->S = d->state_size; p->A = d->action_size; p->H1 = d->hidden1; p->H2 = d->hidden2;
  size_t o = 0;
  p->o_sigma = o; o += p->A;
  p->o_w1 = o; o += (size_t)p->H1 * p->S;
  p->o_b1 = o; o += p->H1;
  p->o_w2 = o; o += (size_t)p->H2 * p->H1;
  p->o_b2 = o; o += p->H2;
  p->o_w3 = o; o += (size_t)p->A * p->H2;
  p->o_b3 = o; o += p->A;
  p->P = o;
  *out = p;
  return MI_OK;
}
extern "C" void mi_policy_destroy(mi_policy* p) {
  if (p && p->fold_counters) (void)hipFree(p->fold_counters);
  delete p;
}
extern "C" int mi_policy_param_count(const mi_policy* p, size_t* n) {
  if (!p || !n) return MI_ERR_ARG;
  *n = p->P;
  return MI_OK;
}

hipError_t dense_fwd(hipStream_t st, int T, int B, int I, int O, const float* x0, const float* w0, size_t ws0,
                     const float* x1, const float* w1, size_t ws1, const float* bias, size_t bs, const float* mask,
                     int act, float* y) {
  DenseArgs a{};
  a.x[0] = x0; a.w[0] = w0; a.wstride[0] = ws0; a.x[1] = x1; a.w[1] = w1; a.wstride[1] = ws1;
  a.bias = bias; a.bstride = bs; a.mask = mask; a.y = y; a.B = B; a.I = I; a.O = O; a.nterms = x1 ? 2 : 1; a.act = act;
  launch_dense<true>(st, T, a);
  return hipGetLastError();
}
static hipError_t dense_bwd_x(hipStream_t st, int T, int B, int I, int O, const float* dy0, const float* w0, size_t ws0,
                              const float* dy1, const float* w1, size_t ws1, const float* mask, int act, float* dx,
                              float* dx_pre = nullptr, const float* hd = nullptr, const float* dpre = nullptr) {
  DenseArgs a{};
  a.x[0] = dy0; a.w[0] = w0; a.wstride[0] = ws0; a.x[1] = dy1; a.w[1] = w1; a.wstride[1] = ws1;
  a.mask = mask; a.act = act; a.y = dx; a.ypre = dx_pre; a.hd = hd; a.dpre = dpre;
  a.B = B; a.I = I; a.O = O; a.nterms = dy1 ? 2 : 1;
  launch_dense<false>(st, T, a);
  return hipGetLastError();
}
static hipError_t dense_bwd_w(hipStream_t st, int T, int B, int I, int O, const float* dy0, const float* x0, const float* dy1,
                              const float* x1, float* dw, float* db, size_t gs) {
  DenseWArgs a{};
  a.dy[0] = dy0; a.x[0] = x0; a.dy[1] = dy1; a.x[1] = x1; a.dw = dw; a.db = db; a.gstride = gs;
  a.B = B; a.I = I; a.O = O; a.nterms = dy1 ? 2 : 1;
  hipLaunchKernelGGL(dense_wgrad_mfma_kernel, dim3(ceil_div(O, 32) * ceil_div(I + 1, 32), T), dim3(512), 0, st, a);
  return hipGetLastError();
}

// MLP forward on [T][B][S]; theta with per-task stride ts (0 = shared)
int mlp_forward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, Acts& a) {
  PCHK(p, dense_fwd(st, T, B, p->S, p->H1, x, th + p->o_w1, ts, nullptr, nullptr, 0, th + p->o_b1, ts, nullptr, p->act, a.h1));
  PCHK(p, dense_fwd(st, T, B, p->H1, p->H2, a.h1, th + p->o_w2, ts, nullptr, nullptr, 0, th + p->o_b2, ts, nullptr, p->act, a.h2));
  PCHK(p, dense_fwd(st, T, B, p->H2, p->A, a.h2, th + p->o_w3, ts, nullptr, nullptr, 0, th + p->o_b3, ts, nullptr, ACT_NONE, a.mu));
  return MI_OK;
}
// MLP backward from dmu: grads into g [T][P] (sigma slot untouched); scratch d2 [T][B][H2], d1 [T][B][H1] keep dz2 / dz1;
// pre2 / pre1 (optional) keep the cotangents w.r.t. h2 / h1 before the phi' factor (a tanh HVP needs them).
// head_only: only W3 / b3 get gradients (ANIL inner loop with the body under no_grad, rl.py:381-382, policies.py:100-106).
int mlp_backward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts, const Acts& a,
                 const float* dmu, float* d2, float* d1, float* g, float* pre2 = nullptr, float* pre1 = nullptr,
                 bool head_only = false) {
  const size_t P = p->P;
  PCHK(p, dense_bwd_w(st, T, B, p->H2, p->A, dmu, a.h2, nullptr, nullptr, g + p->o_w3, g + p->o_b3, P));
  if (head_only) return MI_OK;
  PCHK(p, dense_bwd_x(st, T, B, p->H2, p->A, dmu, th + p->o_w3, ts, nullptr, nullptr, 0, a.h2, p->act, d2, pre2));
  PCHK(p, dense_bwd_w(st, T, B, p->H1, p->H2, d2, a.h1, nullptr, nullptr, g + p->o_w2, g + p->o_b2, P));
  PCHK(p, dense_bwd_x(st, T, B, p->H1, p->H2, d2, th + p->o_w2, ts, nullptr, nullptr, 0, a.h1, p->act, d1, pre1));
  PCHK(p, dense_bwd_w(st, T, B, p->S, p->H1, d1, x, nullptr, nullptr, g + p->o_w1, g + p->o_b1, P));
  return MI_OK;
}
// tangent forward: direction v [T][P] (per task), primal acts a -> tangent acts ad (h1d, h2d, mud)
int mlp_tangent_forward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts,
                        const Acts& a, const float* v, Acts& ad) {
  const size_t P = p->P;
  PCHK(p, dense_fwd(st, T, B, p->S, p->H1, x, v + p->o_w1, P, nullptr, nullptr, 0, v + p->o_b1, P, a.h1, p->act, ad.h1));
  PCHK(p, dense_fwd(st, T, B, p->H1, p->H2, a.h1, v + p->o_w2, P, ad.h1, th + p->o_w2, ts, v + p->o_b2, P, a.h2, p->act, ad.h2));
  PCHK(p, dense_fwd(st, T, B, p->H2, p->A, a.h2, v + p->o_w3, P, ad.h2, th + p->o_w3, ts, v + p->o_b3, P, nullptr, ACT_NONE, ad.mu));
  return MI_OK;
}
// tangent backward: R{grads} into hv [T][P]; needs primal cotangents dmu, da2 (d2), da1 (d1), tangent acts ad, R{dmu} = rdmu.
int mlp_tangent_backward(mi_policy* p, hipStream_t st, int T, int B, const float* x, const float* th, size_t ts,
                         const Acts& a, const Acts& ad, const float* v, const float* dmu, const float* d2,
                         const float* d1, const float* pre2, const float* pre1, const float* rdmu, float* r2, float* r1,
                         float* hv) {
  const size_t P = p->P;
  const bool th2 = p->act == ACT_TANH;      // the curvature of tanh adds  -2 h hdot dh  to R{dz}
  PCHK(p, dense_bwd_w(st, T, B, p->H2, p->A, rdmu, a.h2, dmu, ad.h2, hv + p->o_w3, hv + p->o_b3, P));
  PCHK(p, dense_bwd_x(st, T, B, p->H2, p->A, rdmu, th + p->o_w3, ts, dmu, v + p->o_w3, P, a.h2, p->act, r2, nullptr,
                      th2 ? ad.h2 : nullptr, th2 ? pre2 : nullptr));
  PCHK(p, dense_bwd_w(st, T, B, p->H1, p->H2, r2, a.h1, d2, ad.h1, hv + p->o_w2, hv + p->o_b2, P));
  PCHK(p, dense_bwd_x(st, T, B, p->H1, p->H2, r2, th + p->o_w2, ts, d2, v + p->o_w2, P, a.h1, p->act, r1, nullptr,
                      th2 ? ad.h1 : nullptr, th2 ? pre1 : nullptr));
  PCHK(p, dense_bwd_w(st, T, B, p->S, p->H1, r1, x, nullptr, nullptr, hv + p->o_w1, hv + p->o_b1, P));
  return MI_OK;
}

static hipError_t gauss(hipStream_t st, int T, GaussArgs& a) {
  hipLaunchKernelGGL(gauss_kernel, dim3(T), dim3(256), 0, st, a);
  return hipGetLastError();
}

// loc = MLP(state) for acting / densities (policies.py:49-52); theta [P] shared (tstride 0) or per task (tstride = P).
extern "C" int mi_policy_forward(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, int tasks,
                                 int batch, float* loc_out, void* workspace, size_t workspace_bytes) {
  if (!p || !theta || !states || !loc_out || !workspace) return pfail(p, MI_ERR_ARG, "null argument");
  PBump b{reinterpret_cast<char*>(workspace), 0};
  Acts a;
  a.h1 = b.f((size_t)tasks * batch * p->H1); a.h2 = b.f((size_t)tasks * batch * p->H2); a.mu = loc_out;
  if (b.off > workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, "workspace too small");
  return mlp_forward(p, reinterpret_cast<hipStream_t>(stream), tasks, batch, states, theta, tstride, a);
}

static int g_policy_fused_fvp = 1;
static unsigned long long* g_sweep_stamps = nullptr;
extern "C" int mi_debug_policy_sweep_stamps(void* buf) { g_sweep_stamps = reinterpret_cast<unsigned long long*>(buf); return MI_OK; }
// 1 (default): the Fisher-vector product of a supported policy runs as three fused sweeps + three folds (policy_sweep.h);
// 0: the per-layer path (ablation / tests).
extern "C" int mi_policy_set_fused_fvp(int on) { g_policy_fused_fvp = on ? 1 : 0; return MI_OK; }

// One recurrence of cherry.algorithms.trpo.conjugate_gradient (reference rl.py:418) on device vectors, in fp64, as ONE launch:
//   alpha = rr_old / (p . Ap + eps);  x += alpha p;  r -= alpha Ap;  rr_new = r . r;  p = r + (rr_new / rr_old) p
// (a dozen ATen launches and two rocBLAS dots per iteration otherwise: ~0.1 ms of each ~1 ms iteration).  One workgroup: the vectors
// hold the policy's ~10^4 parameters; both dot products are block reductions in a fixed order.
__global__ __launch_bounds__(1024) void cg_update_kernel(double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                         const float* __restrict__ ap, double* __restrict__ rr, float* __restrict__ p32,
                                                         size_t n, double eps, double tol) {
  // tol >= 0: the reference's `if r_dot_new < tol: break` is taken ON THE DEVICE -- rr[2] latches "converged" and every later
  // recurrence of this solve is a no-op, so the host loop needs no synchronisation per iteration (x is exactly the x of the break)
  if (tol >= 0.0 && rr[2] != 0.0) return;
  __shared__ double red[16];
  __shared__ double bcast;
  const int tid = threadIdx.x;
  auto block_sum = [&](double v) -> double {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += red[k];
      bcast = s;
    }
    __syncthreads();
    return bcast;
  };
  const double rr_old = rr[0];
  double s = 0.0;
  for (size_t i = tid; i < n; i += 1024) s += p[i] * (double)ap[i];
  const double alpha = rr_old / (block_sum(s) + eps);
  double q = 0.0;
  for (size_t i = tid; i < n; i += 1024) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * (double)ap[i];
    r[i] = ri;
    q += ri * ri;
  }
  const double rr_new = block_sum(q);
  const double beta = rr_new / rr_old;
  for (size_t i = tid; i < n; i += 1024) {
    const double pi = r[i] + beta * p[i];
    p[i] = pi;
    p32[i] = (float)pi;
  }
  if (tid == 0) { rr[0] = rr_new; rr[1] = alpha; if (tol >= 0.0 && rr_new < tol) rr[2] = 1.0; }
}

// The start of a solve as one launch: r = p = b (fp64), x = 0, p32 = b, rr = (b . b, 0, 0) -- seven tensor-library launches otherwise.
__global__ __launch_bounds__(1024) void cg_init_kernel(const float* __restrict__ b, double* __restrict__ x, double* __restrict__ r,
                                                       double* __restrict__ p, float* __restrict__ p32, double* __restrict__ rr, size_t n) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  double q = 0.0;
  for (size_t i = tid; i < n; i += 1024) {
    const float bf = b[i];
    const double bi = (double)bf;
    x[i] = 0.0; r[i] = bi; p[i] = bi; p32[i] = bf;
    q += bi * bi;
  }
  q = wave_sum(q);
  if ((tid & 63) == 0) red[tid >> 6] = q;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += red[k];
    rr[0] = s; rr[1] = 0.0; rr[2] = 0.0;
  }
}
extern "C" int mi_cg_init(void* stream, const float* b, double* x, double* r, double* p, float* p32, double* rr, size_t n) {
  if (!b || !x || !r || !p || !p32 || !rr || n == 0) return MI_ERR_ARG;
  hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), b, x, r, p, p32, rr, n);
  return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

// The step of a trust-region update from the solve's direction s and F s (reference rl.py:419-421): shs = 0.5 s . F s (summed in fp64),
// lagrange = sqrt(shs / max_kl), out = s / lagrange -- five tensor-library launches otherwise.  A negative shs gives NaN, as there.
__global__ __launch_bounds__(1024) void trpo_scale_step_kernel(const float* __restrict__ s, const float* __restrict__ fs, size_t n, float max_kl,
                                                               float* __restrict__ out, float* __restrict__ lagrange) {
  __shared__ double red[16];
  __shared__ float lm_s;
  const int tid = threadIdx.x;
  double q = 0.0;
  for (size_t i = tid; i < n; i += 1024) q += (double)s[i] * (double)fs[i];
  q = wave_sum(q);
  if ((tid & 63) == 0) red[tid >> 6] = q;
  __syncthreads();
  if (tid == 0) {
    double d = 0.0;
    for (int k = 0; k < 16; ++k) d += red[k];
    const float shs = 0.5f * (float)d;
    lm_s = sqrtf(shs / max_kl);
    if (lagrange) *lagrange = lm_s;
  }
  __syncthreads();
  const float lm = lm_s;
  for (size_t i = tid; i < n; i += 1024) out[i] = s[i] / lm;
}
extern "C" int mi_trpo_scale_step(void* stream, const float* step, const float* fstep, size_t n, float max_kl, float* out, float* lagrange_out) {
  if (!step || !fstep || !out || n == 0 || !(max_kl > 0.f)) return MI_ERR_ARG;
  hipLaunchKernelGGL(trpo_scale_step_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), step, fstep, n, max_kl, out, lagrange_out);
  return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

extern "C" int mi_cg_update(void* stream, double* x, double* r, double* p, const float* ap, double* rr, float* p32, size_t n, double eps) {
  if (!x || !r || !p || !ap || !rr || !p32 || n == 0) return MI_ERR_ARG;
  hipLaunchKernelGGL(cg_update_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), x, r, p, ap, rr, p32, n, eps, -1.0);
  return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}
extern "C" int mi_cg_update_checked(void* stream, double* x, double* r, double* p, const float* ap, double* rr, float* p32, size_t n, double eps,
                                    double tol) {
  if (!x || !r || !p || !ap || !rr || !p32 || n == 0 || tol < 0.0) return MI_ERR_ARG;
  hipLaunchKernelGGL(cg_update_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), x, r, p, ap, rr, p32, n, eps, tol);
  return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

// =====================================================================================================================
// MAML inner loop of the policy with a general number of updates and the VPG / PPO losses (reference core_functions/rl.py:
// vpg_a2c_loss :209-228 (dice=False), fast_adapt_vpg :231-255, fast_adapt_ppo :267-318, single_ppo_update :321-337; drivers
// rl/maml_ppo.py, rl/anil_ppo.py): per task  theta_{k+1} = theta_k - lr * [head mask] grad L_k(theta_k)  for k < K on replayed
// support batches, a query loss at theta_K, and -- what `av_loss.backward()` computes through learn2learn's second-order
// `learner.adapt` -- its gradient w.r.t. theta via the adjoint recursion  lam_k = lam_{k+1} - lr H_k [mask] lam_{k+1},
// every H_k v as a forward-over-reverse sweep over the saved step-k pass (as in engine.hip for the classifier).
//
// Losses as functions of the per-sample mean log-prob lp_i:   A2C  f_i = -A_i lp_i / B                    (a2c.policy_loss)
//   PPO  f_i = -min(r_i A_i, clamp(r_i, 1-c, 1+c) A_i) / B,  r_i = exp(lp_i - lp_old_i)                    (ppo.policy_loss)
// f' feeds the backward pass, f'' (0 for A2C, = f' for an active PPO sample) the Hessian-vector product:
//   R{dL/dx} = f'' (dlp/dtheta . v) dlp/dx + f' R{dlp/dx}.   torch.min splits the gradient of ties evenly between its arguments;
// inside the clip range both arguments ARE r A, so the sum is again r A -- active = inside the range, or outside with r A the
// smaller argument.
struct Gauss2Args {
  const float* mu; const float* mud;
  const float* rho; const float* rhod; size_t rstride, vstride;
  const float* act; const float* adv; const int32_t* count;
  const float* oldlp;     // [T][B] PPO: log-prob under the parameters the epoch group started from
  float* lp_out;          // [T][B] (P_LOGP)
  float* coef;            // [T][B] f'  (written by P_PRIMAL, read by P_TANGENT)
  float* coef2;           // [T][B] f''
  float* dmu; float* drho; size_t gstride;
  float* loss;            // [T]
  float clip;
  int B, A, kind, mode, value_ratio_one;
  const float* done;      // [T][B] DiCE: 1 at the last step of every episode (cherry `dones`)
  float* scratch;         // [T][B] DiCE tangent: per-sample scratch
};
enum { P_PRIMAL = 0, P_TANGENT = 1, P_LOGP = 2 };

// DiCE objective (reference core_functions/rl.py:219-226, vpg_a2c_loss(dice=True)):
//   weights_i = (1 - done_{i-1}) / E  (weights_0 = 1 / E,  E = number of episodes = sum of dones)
//   c = weighted_cumsum(log_probs, weights):  c_i = lp_i + weights_i c_{i-1},  with the reference's Python wrap-around at i = 0
//       (values[-1] is the LAST element, still unmodified): c_0 = lp_0 + weights_0 lp_{N-1}
//   loss = a2c.policy_loss(magic_box(c), A) = -mean(exp(c - stop_gradient(c)) A):  value -mean(A), d loss / d c_i = a_i = -A_i / N,
//   d^2 loss / d c_i^2 = a_i as well.  c = M lp with M fixed by the episode boundaries, so
//       d loss / d lp = M^T a,        R{d loss / d lp} = M^T (a . (M lp_dot)).
// Episodes are independent segments of the recurrence (weights_i = 0 at an episode start): whichever thread meets a segment's
// first (last) sample runs the forward (adjoint) recurrence along it; the wrap term is a one-element fix-up.
__device__ __forceinline__ bool dice_start(const float* dn, int i) { return i == 0 || dn[i - 1] != 0.f; }
// out = M x (forward) for one task; x, out: [cnt] (may not alias)
__device__ void dice_forward(const float* dn, int cnt, float invE, const float* x, float* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    if (!dice_start(dn, i)) continue;
    float c = x[i] + (i == 0 ? invE * x[cnt - 1] : 0.f);
    out[i] = c;
    for (int k = i + 1; k < cnt && !dice_start(dn, k); ++k) { c = x[k] + invE * c; out[k] = c; }
  }
  __syncthreads();
}
// out = M^T x (adjoint) for one task
__device__ void dice_adjoint(const float* dn, int cnt, float invE, const float* x, float* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    if (!(i == cnt - 1 || dn[i] != 0.f)) continue;           // last sample of a segment
    float g = x[i];
    out[i] = g;
    for (int k = i; k > 0 && !dice_start(dn, k); --k) { g = x[k - 1] + invE * g; out[k - 1] = g; }
  }
  __syncthreads();
  if (threadIdx.x == 0 && cnt > 0) out[cnt - 1] += invE * out[0];          // c_0 also reads lp_{N-1}
  __syncthreads();
}

__global__ __launch_bounds__(256) void gauss2_kernel(Gauss2Args a) {
  __shared__ float red[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int B = a.B, A = a.A, cnt = a.count ? a.count[t] : B;
  const float invB = 1.f / (float)cnt, invD = 1.f / (float)A;
  float acc[7];   // loss, drho[0..5]
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] = 0.f;
  const bool dice = a.kind == MI_PLOSS_DICE && a.mode != P_LOGP;
  float invE = 0.f;
  if (dice) {
    // per-sample coefficients through the episode recurrences BEFORE the per-sample loop below (which then reads coef / scratch)
    const float* dn = a.done + (size_t)t * B;
    float e = 0.f;
    for (int b = tid; b < cnt; b += 256) e += dn[b] != 0.f ? 1.f : 0.f;
    red[tid] = e;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
      if (tid < s2) red[tid] += red[tid + s2];
      __syncthreads();
    }
    invE = 1.f / red[0];
    __syncthreads();
    float* cf = a.coef + (size_t)t * B;
    float* c2 = a.coef2 + (size_t)t * B;
    if (a.mode == P_PRIMAL) {
      for (int b = tid; b < B; b += 256) { c2[b] = b < cnt ? -a.adv[(size_t)t * B + b] * invB : 0.f; cf[b] = 0.f; }
      __syncthreads();
      dice_adjoint(dn, cnt, invE, c2, cf);                    // coef = M^T a
    } else {
      float* sc = a.scratch + (size_t)t * B;                  // sc <- lp_dot per sample
      for (int b = tid; b < B; b += 256) {
        const size_t ob = (size_t)t * B + b;
        float lpd = 0.f;
        for (int d = 0; d < A; ++d) {
          const float rp = a.rho[(size_t)t * a.rstride + d];
          const bool live = rp > LOG_EPS;
          const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
          const float rd = live ? a.rhod[(size_t)t * a.vstride + d] : 0.f;
          const float df = a.act[ob * A + d] - a.mu[ob * A + d];
          lpd += invD * (df * iv * a.mud[ob * A + d] + (df * df * iv - 1.f) * rd);
        }
        sc[b] = b < cnt ? lpd : 0.f;
      }
      __syncthreads();
      float* tmp = a.dmu + (size_t)t * B * A;                 // [B*A] >= [B]: free until the per-sample loop writes it
      dice_forward(dn, cnt, invE, sc, tmp);                   // tmp = M lp_dot
      for (int b = tid; b < cnt; b += 256) tmp[b] *= c2[b];   // a . (M lp_dot)
      __syncthreads();
      dice_adjoint(dn, cnt, invE, tmp, sc);                   // sc = R{coef}
    }
  }
  for (int b = tid; b < B; b += 256) {
    const bool valid = b < cnt;
    const size_t ob = (size_t)t * B + b;
    float lp = 0.f;
    for (int d = 0; d < A; ++d) {
      const float r = fmaxf(a.rho[(size_t)t * a.rstride + d], LOG_EPS), sg = expf(r);
      const float df = a.act[ob * A + d] - a.mu[ob * A + d];
      lp += -(df * df) / (2.f * sg * sg) - r - HALF_LOG_2PI;
    }
    lp *= invD;
    if (a.mode == P_LOGP) { a.lp_out[ob] = lp; continue; }
    if (a.mode == P_PRIMAL) {
      float c = 0.f, c2 = 0.f;
      if (valid) {
        const float ad = a.adv[ob];
        if (a.kind == MI_PLOSS_A2C) {
          c = -ad * invB;
          acc[0] += a.value_ratio_one ? c : c * lp;          // PPO's validation loss: ratio == 1 exactly, value -mean(A)
        } else if (a.kind == MI_PLOSS_DICE) {
          c = a.coef[ob];                                     // (M^T a)_b, computed above
          c2 = a.coef2[ob];
          acc[0] += -ad * invB;                               // magic_box == 1: value -mean(A)
        } else {
          const float ratio = expf(lp - a.oldlp[ob]);
          const float o1 = ratio * ad, o2 = fminf(fmaxf(ratio, 1.f - a.clip), 1.f + a.clip) * ad;
          acc[0] += -fminf(o1, o2) * invB;
          const bool inside = ratio >= 1.f - a.clip && ratio <= 1.f + a.clip;
          const bool active = inside || o1 < o2;
          c = active ? -o1 * invB : 0.f;
          c2 = c;
        }
      }
      a.coef[ob] = c;
      a.coef2[ob] = c2;
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        a.dmu[ob * A + d] = c * invD * df * iv;
        if (rp > LOG_EPS) acc[1 + d] += c * invD * (df * df * iv - 1.f);
      }
    } else {   // P_TANGENT
      const float c = valid ? a.coef[ob] : 0.f, c2 = valid ? a.coef2[ob] : 0.f;
      float lpd = 0.f;                                       // tangent of lp along (mud, rhod)
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const bool live = rp > LOG_EPS;
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
        const float rd = live ? a.rhod[(size_t)t * a.vstride + d] : 0.f;
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        lpd += invD * (df * iv * a.mud[ob * A + d] + (df * df * iv - 1.f) * rd);
      }
      const float cd = dice ? (valid ? a.scratch[ob] : 0.f) : c2 * lpd;   // R{f'} (DiCE: through the episode recurrences, above)
      for (int d = 0; d < A; ++d) {
        const float rp = a.rho[(size_t)t * a.rstride + d];
        const bool live = rp > LOG_EPS;
        const float r = fmaxf(rp, LOG_EPS), sg = expf(r), iv = 1.f / (sg * sg);
        const float rd = live ? a.rhod[(size_t)t * a.vstride + d] : 0.f;
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        const float md = a.mud[ob * A + d];
        a.dmu[ob * A + d] = cd * invD * df * iv + c * invD * (-md * iv - 2.f * df * rd * iv);
        if (live) acc[1 + d] += cd * invD * (df * df * iv - 1.f) + c * invD * (-2.f * df * md * iv - 2.f * df * df * rd * iv);
      }
    }
  }
  if (a.mode == P_LOGP) return;
  for (int k = 0; k < 1 + A; ++k) {
    red[tid] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      if (k == 0) { if (a.loss && a.mode == P_PRIMAL) a.loss[t] = red[0]; }
      else if (a.drho) a.drho[(size_t)t * a.gstride + (k - 1)] = red[0];
    }
    __syncthreads();
  }
}

// keep only sigma and the last Linear of a [T][P] vector (ANIL: body under no_grad)
__global__ void head_mask_kernel(float* __restrict__ v, int p, int body_lo, int body_hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= body_lo && i < body_hi) v[(size_t)blockIdx.y * p + i] = 0.f;
}

// ---- per-parameter step sizes (mi_policy_meta_batch_lr / mi_policy_update_lr): per-element kernels over [T][P], one thread per entry,
// grid (ceil(P / 256), T).  lr is ONE row [P] of the step-size table; [body_lo, body_hi) is the head mask of head_only (the entries whose
// step is 0 whatever lr holds; body_lo = body_hi without head_only).
// out[t][i] = a[t*astride + i] - lr[i] * g[t][i], a separate multiply and subtract like axpy_bcast_kernel's; an entry whose step is exactly 0
// (or masked) passes through bitwise.  a may be out (in place: mi_policy_update_lr), so neither is __restrict__.
__global__ void lr_advance_kernel(const float* a, size_t astride, const float* __restrict__ g, const float* __restrict__ lr, int p, int body_lo,
                                  int body_hi, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const size_t t = blockIdx.y;
  const float d = (i >= body_lo && i < body_hi) ? 0.f : lr[i];
  const float av = a[t * astride + i];
  out[t * p + i] = d == 0.f ? av : av - d * g[t * p + i];
}
// One adjoint advance: lam_k = lam_{k+1} - mask_m(hv) in place (hv NULL: lam is lam_K as the query pass left it), and for the update
// below it (lr NULL: there is none) dir = d_{k-1} (.) lam_k, the direction of its tangent pass, and prod = m (.) g_{k-1} (.) lam_k, its
// term of lr_grad (prod NULL: not wanted).  Masked and zero-step entries of dir, masked entries of prod, are exact zeros.
// The TRPO recursions (mi_trpo_*_steps_lr) use the same launch: lam_k may go to a buffer of its own (out != lam: every entry is
// written), and the general product's rho_k = rho_{k+1} - (hv + s3) subtracts the third-derivative term with it (s3 NULL: none).
__global__ void lr_adjoint_kernel(const float* lam, const float* __restrict__ hv, const float* __restrict__ s3, const float* __restrict__ lr,
                                  const float* __restrict__ g, int p, int body_lo, int body_hi, float* out, float* __restrict__ dir,
                                  float* __restrict__ prod) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const size_t o = (size_t)blockIdx.y * p + i;
  const bool masked = i >= body_lo && i < body_hi;
  float l = lam[o];
  if (hv && !masked) {
    l = s3 ? l - (hv[o] + s3[o]) : l - hv[o];
    out[o] = l;
  } else if (out != lam) {
    out[o] = l;
  }
  if (!lr) return;
  const float d = masked ? 0.f : lr[i];
  dir[o] = d == 0.f ? 0.f : d * l;
  if (prod) prod[o] = masked ? 0.f : g[o] * l;
}
// lr_grad[r][i] = -(sum over the updates k of row r, ascending, and within an update over the tasks, ascending, of m g_k lam_{k+1}): ONE
// fp64 chain per entry in that fixed order, rounded once -- bitwise reproducible, no atomics.  prod [K][T][P] holds the fp32 products of a
// second-order call (lr_adjoint_kernel); a first-order call has lam_{k+1} = lam_K for every k and passes prod NULL: the same fp32 product
// g[k][t][i] * lam[t][i] is formed here.  Grid (ceil(P / 256), lr_rows).  The rows travel as a kernel argument (no copy, no host sync).
#define MI_POLICY_LR_MAX_STEPS 256
#define MI_POLICY_LR_MAX_ROWS 65535   // the fold's gridDim.y
struct LrRows { int32_t row[MI_POLICY_LR_MAX_STEPS]; };
__global__ void lr_fold_kernel(const float* __restrict__ prod, const float* __restrict__ g, const float* __restrict__ lam, LrRows rows, int K,
                               int T, int p, int body_lo, int body_hi, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const int r = blockIdx.y;
  double acc = 0.0;
  if (!(i >= body_lo && i < body_hi)) {
    for (int k = 0; k < K; ++k) {
      if (rows.row[k] != r) continue;
      for (int t = 0; t < T; ++t) {
        const size_t o = ((size_t)k * T + t) * p + i;
        const float v = prod ? prod[o] : g[o] * lam[(size_t)t * p + i];
        acc += (double)v;
      }
    }
  }
  out[(size_t)r * p + i] = (float)(0.0 - acc);
}

// out = a - alpha (h + s3): one step of the general product's rho recursion in one launch (out may be a)
__global__ void step_back_kernel(const float* a, const float* __restrict__ h, const float* __restrict__ s3, float alpha, size_t n, float* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] - alpha * (h[i] + s3[i]);
}
// ---- THE description of a call's inner-loop step, from the extern "C" entry to the launches: the number lr, or the step-size table
// (vec != NULL; update k reads row step_row[k] = d_k).  The two forms launch different kernels in step_advance and AdjointWalk only.
struct PolicyStep {
  float lr = 0.f;                   // the number
  const float* vec = nullptr; int rows = 0;       // device [rows][P], the table; NULL: the number
  const int32_t* step_row = nullptr;      // host [steps], or NULL = all 0
  float* lr_grad_out = nullptr;     // device [rows][P], or NULL (mi_policy_meta_batch_lr)
  size_t P = 0;                     // (check_table fills it in)
  const char* fn = nullptr;         // the entry's name in the error texts; NULL: the scalar entries whose texts carry none
  bool table() const { return vec != nullptr; }
  const float* row(int k) const { return vec ? vec + (size_t)(step_row ? step_row[k] : 0) * P : nullptr; }
  std::string prefix() const { return fn ? std::string(fn) + ": " : std::string(); }
};
struct StepsRule { int lo, hi; bool first; };      // an entry's range of `steps` (INT_MAX: unbounded); first: checked ahead of tasks / batch
static const StepsRule META_STEPS{0, MI_POLICY_LR_MAX_STEPS, false}, TRPO_STEPS{1, INT_MAX, true}, ONE_STEP{1, 1, true};
// The checks a step-size-table entry makes of the table it put into `s`, before any HIP call: the texts and the order they always had
static int check_table(mi_policy* p, PolicyStep& s, int steps, const StepsRule& r, int tasks, int batch) {
  const std::string fn = s.prefix();
  if (!p) return pfail(nullptr, MI_ERR_ARG, fn + "null policy handle");
  if (!s.vec) return pfail(p, MI_ERR_ARG, fn + "lr_vec is NULL");
  if (s.rows < 1 || s.rows > MI_POLICY_LR_MAX_ROWS)
    return pfail(p, MI_ERR_ARG, fn + "lr_rows " + std::to_string(s.rows) + " (must be 1.." + std::to_string(MI_POLICY_LR_MAX_ROWS) + ")");
  const std::string range = r.hi == INT_MAX ? ">= " + std::to_string(r.lo) : std::to_string(r.lo) + ".." + std::to_string(r.hi);
  const bool steps_bad = steps < r.lo || steps > r.hi;
  if (r.first && steps_bad) return pfail(p, MI_ERR_ARG, fn + "steps " + std::to_string(steps) + " (must be " + range + ")");
  if (tasks < 1) return pfail(p, MI_ERR_ARG, fn + "tasks " + std::to_string(tasks) + " (must be >= 1)");
  if (batch < 1) return pfail(p, MI_ERR_ARG, fn + "batch " + std::to_string(batch) + " (must be >= 1)");
  if (steps_bad) return pfail(p, MI_ERR_ARG, fn + "steps " + std::to_string(steps) + " (must be " + range + ")");
  for (int k = 0; s.step_row && k < steps; ++k)
    if (s.step_row[k] < 0 || s.step_row[k] >= s.rows)
      return pfail(p, MI_ERR_ARG, fn + "step_lr_row[" + std::to_string(k) + "] " + std::to_string(s.step_row[k]) + " (must be 0.." +
                                      std::to_string(s.rows - 1) + ")");
  s.P = p->P;
  return MI_OK;
}
// Advance of update k for all tasks: out[t] = a[t] - d_k (.) g[t]  (a: stride astride floats per task, 0 = shared; out may be a).  Table:
// lr_advance_kernel, head mask folded in.  Number: head_mask_kernel on g (not if `g_masked`: mlp_backward(head_only) left the zeros), axpy_bcast_kernel.
static int step_advance(mi_policy* p, hipStream_t st, int T, const PolicyStep& s, int k, bool head_only, bool g_masked, const float* a,
                        size_t astride, float* g, float* out) {
  const int P = (int)p->P, lo = (int)p->o_w1, hi = (int)p->o_w3;          // the body: W1, b1, W2, b2
  const dim3 grid(ceil_div(P, 256), T);
  if (s.table()) {
    hipLaunchKernelGGL(lr_advance_kernel, grid, dim3(256), 0, st, a, astride, (const float*)g, s.row(k), P, head_only ? lo : 0,
                       head_only ? hi : 0, out);
  } else {
    if (head_only && !g_masked) hipLaunchKernelGGL(head_mask_kernel, grid, dim3(256), 0, st, g, P, lo, hi);
    hipLaunchKernelGGL(axpy_bcast_kernel, grid, dim3(256), 0, st, a, astride, (const float*)g, s.lr, P, out);
  }
  PCHK(p, hipGetLastError());
  return MI_OK;
}
// One adjoint recursion through the updates K-1 .. 0 on [T][P] vectors:  x_k = x_{k+1} - H_k (d_k (.) x_{k+1}) [- s3].  The walk that owns it
// computes hv = H_k (.) itself (gauss2 tangent pass, hvp_step, sweep_hvp, mixed_sweep); this owns what differs between the forms:
//   table   seed() writes dir = d_{K-1} (.) x_K, the HVP of update k is driven with dir, back() finishes x_k and writes the dir (and the
//           lr_grad product g_{k-1} (.) x_k) of update k - 1 in the same launch (lr_adjoint_kernel)
//   number  the HVP is driven with x itself (meta-batch, `copy_dir`: with a head-masked copy of it in dir); back() is [head mask on hv +]
//           axpy_bcast_kernel, or step_back_kernel where a third-derivative term s3 comes with hv
struct AdjointWalk {
  mi_policy* p; hipStream_t st; int T; const PolicyStep& step;
  bool head_only, copy_dir;
  dim3 grid() const { return dim3(ceil_div((int)p->P, 256), T); }
  int seed(int K, float* x, const float* g, float* dir, float* prod) const {
    if (!step.table() || K < 1) return MI_OK;
    hipLaunchKernelGGL(lr_adjoint_kernel, grid(), dim3(256), 0, st, (const float*)x, (const float*)nullptr, (const float*)nullptr,
                       step.row(K - 1), g, (int)p->P, head_only ? (int)p->o_w1 : 0, head_only ? (int)p->o_w3 : 0, x, dir, prod);
    PCHK(p, hipGetLastError());
    return MI_OK;
  }
  // *with: the buffer the HVP of the next update down is driven with
  int drive(const float* x, float* dir, const float** with) const {
    *with = step.table() || copy_dir ? dir : x;
    if (step.table() || !copy_dir) return MI_OK;
    PCHK(p, hipMemcpyAsync(dir, x, (size_t)T * p->P * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (head_only) hipLaunchKernelGGL(head_mask_kernel, grid(), dim3(256), 0, st, dir, (int)p->P, (int)p->o_w1, (int)p->o_w3);
    return MI_OK;
  }
  // x_k -> out (may be x) from x = x_{k+1} and hv (+ s3); g, dir, prod: of update k - 1 (table form; k == 0 has none below it)
  int back(int k, const float* x, float* hv, const float* s3, const float* g, float* out, float* dir, float* prod) const {
    const size_t TP = (size_t)T * p->P;
    if (step.table()) {
      hipLaunchKernelGGL(lr_adjoint_kernel, grid(), dim3(256), 0, st, x, (const float*)hv, s3, k > 0 ? step.row(k - 1) : (const float*)nullptr,
                         g, (int)p->P, head_only ? (int)p->o_w1 : 0, head_only ? (int)p->o_w3 : 0, out, dir, prod);
    } else if (s3) {
      hipLaunchKernelGGL(step_back_kernel, dim3((unsigned)((TP + 255) / 256)), dim3(256), 0, st, x, (const float*)hv, s3, step.lr, TP, out);
    } else {
      if (head_only) hipLaunchKernelGGL(head_mask_kernel, grid(), dim3(256), 0, st, hv, (int)p->P, (int)p->o_w1, (int)p->o_w3);
      hipLaunchKernelGGL(axpy_bcast_kernel, grid(), dim3(256), 0, st, x, p->P, (const float*)hv, step.lr, (int)p->P, out);
    }
    PCHK(p, hipGetLastError());
    return MI_OK;
  }
};

struct StepSet { Acts a; float *dmu, *d2, *d1, *pre2, *pre1, *coef, *coef2; };
struct MetaPlan {
  std::vector<StepSet> st;          // per inner update (second order) or one shared set
  StepSet q;                        // query pass
  Acts ta;                          // tangent activations (scratch)
  float *rdmu, *r2, *r1;            // tangent cotangent scratch
  float *theta, *g, *lam, *hv, *vmask;      // [K+1][T][P], [T][P] ...
  float* oldlp;                     // [n_batches][T][B]
  size_t bytes;
};
static void step_set_plan(const mi_policy* p, PBump& b, size_t TB, StepSet& s) {      // (also the one set of mi_policy_update's plan)
  s.a.h1 = b.f(TB * p->H1); s.a.h2 = b.f(TB * p->H2); s.a.mu = b.f(TB * p->A);
  s.dmu = b.f(TB * p->A); s.d2 = b.f(TB * p->H2); s.d1 = b.f(TB * p->H1); s.pre2 = b.f(TB * p->H2); s.pre1 = b.f(TB * p->H1);
  s.coef = b.f(TB); s.coef2 = b.f(TB);
}
static void meta_plan(const mi_policy* p, void* ws, int T, int B, int K, int nb, bool keep_all, MetaPlan& pl) {
  PBump b{reinterpret_cast<char*>(ws), 0};
  const size_t TB = (size_t)T * B, TP = (size_t)T * p->P;
  auto set = [&](StepSet& s) { step_set_plan(p, b, TB, s); };
  pl.st.resize(keep_all ? (K > 0 ? K : 1) : 1);
  for (auto& s : pl.st) set(s);
  set(pl.q);
  pl.ta.h1 = b.f(TB * p->H1); pl.ta.h2 = b.f(TB * p->H2); pl.ta.mu = b.f(TB * p->A);
  pl.rdmu = b.f(TB * p->A); pl.r2 = b.f(TB * p->H2); pl.r1 = b.f(TB * p->H1);
  pl.theta = b.f(TP * (K + 1)); pl.g = b.f(TP); pl.lam = b.f(TP); pl.hv = b.f(TP); pl.vmask = b.f(TP);
  pl.oldlp = b.f(TB * (nb > 0 ? nb : 1));
  pl.bytes = align_up(b.off, 256);
}

extern "C" int mi_policy_meta_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int n_batches, int second_order,
                                              size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1 || steps < 0 || n_batches < 0) return MI_ERR_ARG;
  MetaPlan pl;
  meta_plan(p, nullptr, tasks, batch, steps, n_batches, second_order != 0, pl);
  *bytes = pl.bytes;
  return MI_OK;
}

// The step-size-vector form of the call (mi_policy_meta_batch_lr).  Its plan lies BEHIND the scalar plan, whose offsets do not move: the
// gradient of every update g [K][T][P] (the scalar call keeps one) and, second order, the products prod [K][T][P] -- both only when lr_grad
// is wanted.  The tangent direction dir lies in the scalar plan's vmask slot.
struct LrPlan { float *g, *prod; size_t bytes; };
static void lr_plan(const mi_policy* p, void* ws, size_t scalar_bytes, int T, int K, bool so, bool want_lr_grad, LrPlan& lp) {
  PBump b{reinterpret_cast<char*>(ws), scalar_bytes};
  const size_t TP = (size_t)T * p->P;
  lp.g = want_lr_grad ? b.f(TP * (K > 0 ? K : 1)) : nullptr;
  lp.prod = want_lr_grad && so ? b.f(TP * (K > 0 ? K : 1)) : nullptr;
  lp.bytes = align_up(b.off, 256);
}
extern "C" int mi_policy_meta_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int n_batches, int second_order,
                                                 int lr_rows, int want_lr_grad, size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1 || steps < 0 || steps > MI_POLICY_LR_MAX_STEPS || n_batches < 0 || lr_rows < 1 ||
      lr_rows > MI_POLICY_LR_MAX_ROWS)
    return MI_ERR_ARG;
  MetaPlan pl;
  meta_plan(p, nullptr, tasks, batch, steps, n_batches, second_order != 0, pl);
  LrPlan lp;
  lr_plan(p, nullptr, pl.bytes, tasks, steps, second_order != 0, want_lr_grad != 0, lp);
  *bytes = lp.bytes;
  return MI_OK;
}

// ---- What an extern "C" entry hands its implementation: named fields, filled one by one, in place of 20-30 positional arguments.
// the support replays: [K][T][B][.] stacks (adapt / update, and the query: the one replay), and replay k of them
struct SupStack { const float *states, *actions, *adv; const int32_t* count; const float* done; };
struct SupRef { const float *xs, *as, *adv; const int32_t* cn; };
static SupRef sup_at(const mi_policy* p, const SupStack& s, int T, int B, int k) {
  const size_t TB = (size_t)T * B;
  return {s.states + k * TB * p->S, s.actions + k * TB * p->A, s.adv ? s.adv + k * TB : nullptr,
          s.count ? s.count + (size_t)k * T : nullptr};
}
// Every entry of this file that takes a step fills the fields it has: update's epochs are `steps`; grad_out is also kl_prepare's
// kl_grad_out, `out` a curvature product.
struct PolicyCall {
  void* stream; const float* theta; size_t tstride;
  int steps; const int32_t *step_batch, *step_new_old; int n_batches;
  SupStack sup, qry; const float *old_loc, *old_scale;
  int tasks, batch, loss_kind; float clip;
  PolicyStep step;
  int head_only, second_order, with_grad;
  float damping; const float* v;
  float *loss_out, *kl_out, *theta_out, *grad_out, *out;
  void* workspace; size_t workspace_bytes;
};

// trpo_update (rl.py:361-374) for a meta-batch: theta_out[t] = theta[t] - lr * grad_t(-mean(logp * adv)).  loss_out [T].
// Workspace: the plan of one kept update (mi_policy_meta_workspace_bytes(steps = 1, n_batches = 1, second_order = 1); the TRPO
// workspaces start with it).
// mi_policy_adapt_lr: ONE row [P] of the step-size table in place of the number lr; the head mask of head_only is folded into
// the advance (lr_advance_kernel), and an entry whose step is exactly 0 leaves with the bits of theta.
static int policy_adapt_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  const int T = c.tasks, B = c.batch;
  if (!p || !c.theta || !c.sup.states || !c.sup.actions || !c.sup.adv || !c.theta_out || !c.workspace) return pfail(p, MI_ERR_ARG, fn + "null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  MetaPlan pl;
  meta_plan(p, c.workspace, T, B, 1, 1, true, pl);
  if (pl.bytes > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(pl.bytes));
  StepSet& s = pl.st[0];
  int rc = mlp_forward(p, st, T, B, c.sup.states, c.theta, c.tstride, s.a);
  if (rc) return rc;
  PCHK(p, hipMemsetAsync(pl.g, 0, (size_t)T * p->P * sizeof(float), st));
  GaussArgs ga{};
  ga.mu = s.a.mu; ga.rho = c.theta + p->o_sigma; ga.rstride = c.tstride; ga.act = c.sup.actions; ga.adv = c.sup.adv; ga.count = c.sup.count;
  ga.coef = s.coef; ga.dmu = s.dmu; ga.drho = pl.g + p->o_sigma; ga.gstride = p->P; ga.loss = c.loss_out ? c.loss_out : pl.hv;
  ga.B = B; ga.A = p->A; ga.mode = G_A2C;
  PCHK(p, gauss(st, T, ga));
  rc = mlp_backward(p, st, T, B, c.sup.states, c.theta, c.tstride, s.a, s.dmu, s.d2, s.d1, pl.g, nullptr, nullptr, c.head_only != 0);
  if (rc) return rc;
  return step_advance(p, st, T, c.step, 0, c.head_only != 0, true, c.theta, c.tstride, pl.g, c.theta_out);
}
extern "C" int mi_policy_adapt(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states,
                               const float* actions, const float* adv, const int32_t* count, int tasks, int batch, float lr,
                               int head_only, float* theta_out, float* loss_out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.tstride = tstride; c.sup = {states, actions, adv, count, nullptr}; c.tasks = tasks; c.batch = batch;
  c.step.lr = lr; c.head_only = head_only; c.theta_out = theta_out; c.loss_out = loss_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  return policy_adapt_impl(p, c);
}

// One primal pass of the VPG / PPO / DiCE losses for all tasks at parameters th (stride ts floats per task: P, or 0 = shared): forward, loss + cotangents
// (gauss2_kernel), backward into g [T][P].  Shared by mi_policy_meta_batch and mi_policy_update: same launches, same order.
static int meta_primal(mi_policy* p, hipStream_t st, int T, int B, float clip, StepSet& s, const float* th, size_t ts, const float* states,
                       const float* actions, const float* adv, const int32_t* count, int kind, const float* oldlp, int value_ratio_one,
                       float* g, float* loss, const float* done) {
  const size_t P = p->P, TP = (size_t)T * P;
  int rc = mlp_forward(p, st, T, B, states, th, ts, s.a);
  if (rc) return rc;
  PCHK(p, hipMemsetAsync(g, 0, TP * sizeof(float), st));
  Gauss2Args ga{};
  ga.mu = s.a.mu; ga.rho = th + p->o_sigma; ga.rstride = ts; ga.act = actions; ga.adv = adv; ga.count = count; ga.oldlp = oldlp;
  ga.coef = s.coef; ga.coef2 = s.coef2; ga.dmu = s.dmu; ga.drho = g + p->o_sigma; ga.gstride = P; ga.loss = loss; ga.clip = clip;
  ga.B = B; ga.A = p->A; ga.kind = kind; ga.mode = P_PRIMAL; ga.value_ratio_one = value_ratio_one; ga.done = done;
  hipLaunchKernelGGL(gauss2_kernel, dim3(T), dim3(256), 0, st, ga);
  PCHK(p, hipGetLastError());
  return mlp_backward(p, st, T, B, states, th, ts, s.a, s.dmu, s.d2, s.d1, g, s.pre2, s.pre1, false);
}
// old_log_probs = learner.log_prob(...) under no_grad (rl.py:282-283) at th [T][P] -> olp [T][B]
static int meta_old_logp(mi_policy* p, hipStream_t st, int T, int B, StepSet& s, const float* th, const float* states,
                         const float* actions, const int32_t* count, float* olp) {
  int rc = mlp_forward(p, st, T, B, states, th, p->P, s.a);
  if (rc) return rc;
  Gauss2Args gl{};
  gl.mu = s.a.mu; gl.rho = th + p->o_sigma; gl.rstride = p->P; gl.act = actions; gl.count = count; gl.lp_out = olp; gl.B = B; gl.A = p->A; gl.mode = P_LOGP;
  hipLaunchKernelGGL(gauss2_kernel, dim3(T), dim3(256), 0, st, gl);
  PCHK(p, hipGetLastError());
  return MI_OK;
}

static int policy_meta_batch_impl(mi_policy* p, const PolicyCall& c) {
  const PolicyStep& step = c.step;
  const std::string fn = step.prefix();
  const bool head_only = c.head_only != 0;
  if (!p || !c.theta || !c.qry.states || !c.qry.actions || !c.qry.adv || !c.loss_out || !c.workspace) return pfail(p, MI_ERR_ARG, fn + "null argument");
  if (c.steps > 0 && (!c.step_batch || !c.sup.states || !c.sup.actions || !c.sup.adv || c.n_batches < 1)) return pfail(p, MI_ERR_ARG, fn + "support batches missing");
  if (c.loss_kind != MI_PLOSS_A2C && c.loss_kind != MI_PLOSS_PPO && c.loss_kind != MI_PLOSS_DICE)
    return pfail(p, MI_ERR_ARG, fn + "loss_kind must be MI_PLOSS_A2C, MI_PLOSS_PPO or MI_PLOSS_DICE");
  if (c.loss_kind == MI_PLOSS_DICE && (!c.qry.done || (c.steps > 0 && !c.sup.done)))
    return pfail(p, MI_ERR_ARG, fn + "the DiCE objective needs the episode-end flags of every replay (s_done / q_done)");
  if (c.loss_kind == MI_PLOSS_PPO && c.steps > 0 && !c.step_new_old) return pfail(p, MI_ERR_ARG, fn + "PPO needs step_new_old");
  if (c.with_grad && !c.grad_out) return pfail(p, MI_ERR_ARG, fn + "grad_out is NULL but with_grad != 0");
  for (int k = 0; k < c.steps; ++k)
    if (c.step_batch[k] < 0 || c.step_batch[k] >= c.n_batches) return pfail(p, MI_ERR_ARG, fn + "step_batch entry out of range");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int T = c.tasks, B = c.batch, K = c.steps;
  const size_t P = p->P, TB = (size_t)T * B, TP = (size_t)T * P;
  const bool so = c.second_order && c.with_grad;
  MetaPlan pl;
  meta_plan(p, c.workspace, T, B, K, c.n_batches, so, pl);
  LrPlan lp{nullptr, nullptr, pl.bytes};
  if (step.table()) lr_plan(p, c.workspace, pl.bytes, T, K, so, step.lr_grad_out != nullptr, lp);
  if (lp.bytes > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(lp.bytes));
  auto g_of = [&](int k) { return lp.g ? lp.g + (size_t)k * TP : pl.g; };         // kept per update when lr_grad is wanted
  hipLaunchKernelGGL(axpy_bcast_kernel, dim3(ceil_div((int)P, 256), T), dim3(256), 0, st, c.theta, (size_t)0, pl.g, 0.f, (int)P, pl.theta);
  PCHK(p, hipGetLastError());
  // ---- inner updates
  for (int k = 0; k < K; ++k) {
    StepSet& s = so ? pl.st[k] : pl.st[0];
    float* th = pl.theta + (size_t)k * TP;
    const int bi = c.step_batch[k];
    const float* xs = c.sup.states + (size_t)bi * TB * p->S;
    const float* as = c.sup.actions + (size_t)bi * TB * p->A;
    const float* ad = c.sup.adv + (size_t)bi * TB;
    const int32_t* cn = c.sup.count ? c.sup.count + (size_t)bi * T : nullptr;
    float* olp = pl.oldlp + (size_t)bi * TB;
    if (c.loss_kind == MI_PLOSS_PPO && c.step_new_old[k]) {       // old_log_probs = learner.log_prob(...) under no_grad (rl.py:282-283)
      int rc = meta_old_logp(p, st, T, B, s, th, xs, as, cn, olp);
      if (rc) return rc;
    }
    int rc = meta_primal(p, st, T, B, c.clip, s, th, P, xs, as, ad, cn, c.loss_kind, olp, 0, g_of(k), pl.hv /* scratch: the step loss */,
                    c.sup.done ? c.sup.done + (size_t)bi * TB : nullptr);
    if (rc) return rc;
    rc = step_advance(p, st, T, step, k, head_only, false, th, P, g_of(k), th + TP);
    if (rc) return rc;
  }
  float* thK = pl.theta + (size_t)K * TP;
  if (c.theta_out) PCHK(p, hipMemcpyAsync(c.theta_out, thK, TP * sizeof(float), hipMemcpyDeviceToDevice, st));
  // ---- query loss: VPG = a2c loss; PPO = ppo loss against the adapted policy itself (ratio == 1: value -mean(A), gradient of A2C form)
  int rc = meta_primal(p, st, T, B, c.clip, pl.q, thK, P, c.qry.states, c.qry.actions, c.qry.adv, c.qry.count, c.loss_kind == MI_PLOSS_DICE ? MI_PLOSS_DICE : MI_PLOSS_A2C, nullptr,
                  c.loss_kind == MI_PLOSS_PPO ? 1 : 0, pl.lam, c.loss_out, c.qry.done);
  if (rc) return rc;
  if (!c.with_grad) return MI_OK;
  // ---- adjoint recursion through the updates: the tangent pass of update k is driven with v = d_k (.) lam_{k+1} (table) or the masked
  // lam_{k+1} (number), in vmask; the table form also keeps the lr_grad products of every update
  if (so) {
    const AdjointWalk adj{p, st, T, step, head_only, true};
    auto g_or_none = [&](int k) { return k >= 0 ? (const float*)g_of(k) : (const float*)nullptr; };
    auto prod_of = [&](int k) { return k >= 0 && lp.prod ? lp.prod + (size_t)k * TP : (float*)nullptr; };
    rc = adj.seed(K, pl.lam, g_or_none(K - 1), pl.vmask, prod_of(K - 1));
    if (rc) return rc;
    for (int k = K - 1; k >= 0; --k) {
      StepSet& s = pl.st[k];
      const float* th = pl.theta + (size_t)k * TP;
      const int bi = c.step_batch[k];
      const float* xs = c.sup.states + (size_t)bi * TB * p->S;
      const float* as = c.sup.actions + (size_t)bi * TB * p->A;
      const int32_t* cn = c.sup.count ? c.sup.count + (size_t)bi * T : nullptr;
      const float* v;                                        // hv = H_k v
      rc = adj.drive(pl.lam, pl.vmask, &v);
      if (rc) return rc;
      PCHK(p, hipMemsetAsync(pl.hv, 0, TP * sizeof(float), st));
      rc = mlp_tangent_forward(p, st, T, B, xs, th, P, s.a, v, pl.ta);
      if (rc) return rc;
      Gauss2Args gt{};
      gt.mu = s.a.mu; gt.mud = pl.ta.mu; gt.rho = th + p->o_sigma; gt.rstride = P; gt.rhod = v + p->o_sigma; gt.vstride = P;
      gt.act = as; gt.count = cn; gt.coef = s.coef; gt.coef2 = s.coef2; gt.dmu = pl.rdmu; gt.drho = pl.hv + p->o_sigma; gt.gstride = P;
      gt.B = B; gt.A = p->A; gt.mode = P_TANGENT;
      if (c.loss_kind == MI_PLOSS_DICE) {                      // the episode recurrences couple the samples of a replay
        gt.kind = MI_PLOSS_DICE; gt.done = c.sup.done + (size_t)bi * TB; gt.adv = c.sup.adv + (size_t)bi * TB;
        gt.scratch = pl.oldlp + (size_t)bi * TB;             // free: old log-probs exist only for PPO
      }
      hipLaunchKernelGGL(gauss2_kernel, dim3(T), dim3(256), 0, st, gt);
      PCHK(p, hipGetLastError());
      rc = mlp_tangent_backward(p, st, T, B, xs, th, P, s.a, pl.ta, v, s.dmu, s.d2, s.d1, s.pre2, s.pre1, pl.rdmu, pl.r2, pl.r1, pl.hv);
      if (rc) return rc;
      // (head_only: the body sat under no_grad during the update, no path from theta_{k+1} back into it)
      rc = adj.back(k, pl.lam, pl.hv, nullptr, g_or_none(k - 1), pl.lam, pl.vmask, prod_of(k - 1));
      if (rc) return rc;
    }
  }
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, pl.lam, T, (int)P, 1.f, (const float*)nullptr, 0.f, c.grad_out);
  PCHK(p, hipGetLastError());
  if (step.lr_grad_out) {           // first order: lam_{k+1} = lam_K for every k, still in pl.lam; the fold forms the products itself
    LrRows rows;
    for (int k = 0; k < MI_POLICY_LR_MAX_STEPS; ++k) rows.row[k] = k < K && step.step_row ? step.step_row[k] : 0;
    hipLaunchKernelGGL(lr_fold_kernel, dim3(ceil_div((int)P, 256), step.rows), dim3(256), 0, st, (const float*)lp.prod, (const float*)lp.g,
                       (const float*)pl.lam, rows, K, T, (int)P, head_only ? (int)p->o_w1 : 0, head_only ? (int)p->o_w3 : 0, step.lr_grad_out);
    PCHK(p, hipGetLastError());
  }
  return MI_OK;
}

extern "C" int mi_policy_meta_batch(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                                    const int32_t* step_new_old, int n_batches, const float* s_states, const float* s_actions,
                                    const float* s_adv, const int32_t* s_count, const float* q_states, const float* q_actions,
                                    const float* q_adv, const int32_t* q_count, int tasks, int batch, int loss_kind, float clip,
                                    float inner_lr, int head_only, int second_order, int with_grad, float* loss_out,
                                    float* theta_out, float* grad_out, void* workspace, size_t workspace_bytes) {
  if (loss_kind == MI_PLOSS_DICE) return pfail(p, MI_ERR_ARG, "MI_PLOSS_DICE needs the episode-end flags: call mi_policy_meta_batch_dones");
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.steps = steps; c.step_batch = step_batch; c.step_new_old = step_new_old; c.n_batches = n_batches;
  c.sup = {s_states, s_actions, s_adv, s_count, nullptr}; c.qry = {q_states, q_actions, q_adv, q_count, nullptr}; c.tasks = tasks; c.batch = batch;
  c.loss_kind = loss_kind; c.clip = clip; c.head_only = head_only; c.second_order = second_order; c.with_grad = with_grad;
  c.loss_out = loss_out; c.theta_out = theta_out; c.grad_out = grad_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.step.lr = inner_lr;
  return policy_meta_batch_impl(p, c);
}
// The same with the replays' episode-end flags (cherry `dones`: s_done [n_batches, tasks, batch], q_done [tasks, batch]; 1 at
// the last step of every episode): required by MI_PLOSS_DICE, ignored by the other losses.
extern "C" int mi_policy_meta_batch_dones(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                                          const int32_t* step_new_old, int n_batches, const float* s_states, const float* s_actions,
                                          const float* s_adv, const int32_t* s_count, const float* s_done, const float* q_states,
                                          const float* q_actions, const float* q_adv, const int32_t* q_count, const float* q_done,
                                          int tasks, int batch, int loss_kind, float clip, float inner_lr, int head_only,
                                          int second_order, int with_grad, float* loss_out, float* theta_out, float* grad_out,
                                          void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.steps = steps; c.step_batch = step_batch; c.step_new_old = step_new_old; c.n_batches = n_batches;
  c.sup = {s_states, s_actions, s_adv, s_count, s_done}; c.qry = {q_states, q_actions, q_adv, q_count, q_done}; c.tasks = tasks; c.batch = batch;
  c.loss_kind = loss_kind; c.clip = clip; c.head_only = head_only; c.second_order = second_order; c.with_grad = with_grad;
  c.loss_out = loss_out; c.theta_out = theta_out; c.grad_out = grad_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.step.lr = inner_lr;
  return policy_meta_batch_impl(p, c);
}
// The step-size-vector form (include/mi_maml.h): the same implementation with lr_vec; every check of its own comes before any HIP call.
extern "C" int mi_policy_meta_batch_lr(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                                       const int32_t* step_new_old, const int32_t* step_lr_row, int n_batches, const float* s_states,
                                       const float* s_actions, const float* s_adv, const int32_t* s_count, const float* s_done,
                                       const float* q_states, const float* q_actions, const float* q_adv, const int32_t* q_count,
                                       const float* q_done, int tasks, int batch, int loss_kind, float clip, const float* lr_vec, int lr_rows,
                                       int head_only, int second_order, int with_grad, float* loss_out, float* theta_out, float* grad_out,
                                       float* lr_grad_out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.steps = steps; c.step_batch = step_batch; c.step_new_old = step_new_old; c.n_batches = n_batches;
  c.sup = {s_states, s_actions, s_adv, s_count, s_done}; c.qry = {q_states, q_actions, q_adv, q_count, q_done}; c.tasks = tasks; c.batch = batch;
  c.loss_kind = loss_kind; c.clip = clip; c.head_only = head_only; c.second_order = second_order; c.with_grad = with_grad;
  c.loss_out = loss_out; c.theta_out = theta_out; c.grad_out = grad_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.step.vec = lr_vec; c.step.rows = lr_rows; c.step.step_row = step_lr_row; c.step.lr_grad_out = lr_grad_out; c.step.fn = "mi_policy_meta_batch_lr";
  int rc = check_table(p, c.step, steps, META_STEPS, tasks, batch);
  if (rc) return rc;
  if (lr_grad_out && !with_grad) return pfail(p, MI_ERR_ARG, c.step.prefix() + "lr_grad_out given but with_grad == 0");
  return policy_meta_batch_impl(p, c);
}

// =====================================================================================================================
// mi_policy_update: `epochs` plain (first-order) updates of per-task parameters on ONE replay per task -- the inner update of
// fast_adapt_vpg / fast_adapt_ppo (rl.py:231-255,267-318) and single_ppo_update (rl.py:319-336) without the replay of the
// earlier adapt steps mi_policy_meta_batch starts with.  Runs the passes of a first-order mi_policy_meta_batch step in the
// same order (meta_old_logp, meta_primal, head mask, axpy), so from shared parameters theta_out is bit-identical to
// mi_policy_meta_batch(steps = epochs, with_grad = 0).  theta_out itself is the working copy: u_e is updated in place.
struct UpdatePlan { StepSet s; float *g, *loss_e, *oldlp; size_t bytes; };
static void update_plan(const mi_policy* p, void* ws, int T, int B, int E, UpdatePlan& pl) {
  PBump b{reinterpret_cast<char*>(ws), 0};
  const size_t TB = (size_t)T * B, TP = (size_t)T * p->P;
  step_set_plan(p, b, TB, pl.s);
  pl.g = b.f(TP); pl.loss_e = b.f((size_t)E * T); pl.oldlp = b.f(TB);
  pl.bytes = align_up(b.off, 256);
}
// loss_e [E][T] (one row per gauss2 launch) -> loss_out [T][E]
__global__ void update_loss_transpose_kernel(const float* __restrict__ in, int E, int T, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * T) return;
  const int e = i / T, t = i % T;
  out[(size_t)t * E + e] = in[i];
}
#define MI_UPDATE_MAX_EPOCHS 64
static int update_args(mi_policy* p, const std::string& fn, int tasks, int batch, int epochs) {
  if (!p) return pfail(nullptr, MI_ERR_ARG, fn + "null policy handle");
  if (tasks < 1) return pfail(p, MI_ERR_ARG, fn + "tasks " + std::to_string(tasks) + " (must be >= 1)");
  if (batch < 1) return pfail(p, MI_ERR_ARG, fn + "batch " + std::to_string(batch) + " (must be >= 1)");
  if (epochs < 1 || epochs > MI_UPDATE_MAX_EPOCHS)
    return pfail(p, MI_ERR_ARG, fn + "epochs " + std::to_string(epochs) + " (must be 1.." + std::to_string(MI_UPDATE_MAX_EPOCHS) + ")");
  return MI_OK;
}
extern "C" int mi_policy_update_workspace_bytes(const mi_policy* p, int tasks, int batch, size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1) return MI_ERR_ARG;
  UpdatePlan pl;
  update_plan(p, nullptr, tasks, batch, MI_UPDATE_MAX_EPOCHS, pl);
  *bytes = pl.bytes;
  return MI_OK;
}
// c.sup: the one replay; c.steps: the epochs; the step of every epoch is the number, or (mi_policy_update_lr) row 0 of a one-row table
static int policy_update_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  const int T = c.tasks, B = c.batch;
  int rc = MI_OK;
  if (!c.theta || !c.sup.states || !c.sup.actions || !c.sup.adv || !c.theta_out || !c.workspace) return pfail(p, MI_ERR_ARG, fn + "null argument");
  if (c.loss_kind != MI_PLOSS_A2C && c.loss_kind != MI_PLOSS_PPO && c.loss_kind != MI_PLOSS_DICE)
    return pfail(p, MI_ERR_ARG, fn + "loss_kind " + std::to_string(c.loss_kind) + " (must be MI_PLOSS_A2C, MI_PLOSS_PPO or MI_PLOSS_DICE)");
  if (c.loss_kind == MI_PLOSS_DICE && !c.sup.done)
    return pfail(p, MI_ERR_ARG, fn + "loss_kind MI_PLOSS_DICE needs the episode-end flags (done is NULL)");
  if (c.tstride != 0 && c.tstride != p->P)
    return pfail(p, MI_ERR_ARG, fn + "tstride " + std::to_string(c.tstride) + " (must be 0 or P = " + std::to_string(p->P) + ")");
  if (c.tstride == 0 && T > 1 && c.theta == c.theta_out)
    return pfail(p, MI_ERR_ARG, fn + "theta_out may alias theta only with tstride = P");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const size_t P = p->P;
  UpdatePlan pl;
  update_plan(p, c.workspace, T, B, c.steps, pl);
  if (pl.bytes > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(pl.bytes));
  const dim3 pgrid(ceil_div((int)P, 256), T);
  hipLaunchKernelGGL(axpy_bcast_kernel, pgrid, dim3(256), 0, st, c.theta, c.tstride, pl.g, 0.f, (int)P, c.theta_out);      // u_0
  PCHK(p, hipGetLastError());
  if (c.loss_kind == MI_PLOSS_PPO) {                            // old log-probs once, at u_0 (rl.py:280-290)
    rc = meta_old_logp(p, st, T, B, pl.s, c.theta_out, c.sup.states, c.sup.actions, c.sup.count, pl.oldlp);
    if (rc) return rc;
  }
  for (int e = 0; e < c.steps; ++e) {
    rc = meta_primal(p, st, T, B, c.clip, pl.s, c.theta_out, P, c.sup.states, c.sup.actions, c.sup.adv, c.sup.count, c.loss_kind, pl.oldlp, 0, pl.g,
                     pl.loss_e + (size_t)e * T, c.sup.done);
    if (rc) return rc;
    rc = step_advance(p, st, T, c.step, 0, c.head_only != 0, false, c.theta_out, P, pl.g, c.theta_out);      // in place, elementwise
    if (rc) return rc;
  }
  if (c.loss_out) {
    hipLaunchKernelGGL(update_loss_transpose_kernel, dim3(ceil_div(c.steps * T, 256)), dim3(256), 0, st, pl.loss_e, c.steps, T, c.loss_out);
    PCHK(p, hipGetLastError());
  }
  return MI_OK;
}
extern "C" int mi_policy_update(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states,
                                const float* actions, const float* adv, const int32_t* count, const float* done, int tasks,
                                int batch, int loss_kind, int epochs, float clip, float lr, int head_only, float* theta_out,
                                float* loss_out, void* workspace, size_t workspace_bytes) {
  int rc = update_args(p, "mi_policy_update: ", tasks, batch, epochs);
  if (rc) return rc;
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.tstride = tstride; c.sup = {states, actions, adv, count, done}; c.tasks = tasks; c.batch = batch;
  c.loss_kind = loss_kind; c.steps = epochs; c.clip = clip; c.head_only = head_only; c.theta_out = theta_out; c.loss_out = loss_out;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.step.lr = lr; c.step.fn = "mi_policy_update";
  return policy_update_impl(p, c);
}
extern "C" int mi_policy_update_lr(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states,
                                   const float* actions, const float* adv, const int32_t* count, const float* done, int tasks,
                                   int batch, int loss_kind, int epochs, float clip, const float* lr_vec, int head_only,
                                   float* theta_out, float* loss_out, void* workspace, size_t workspace_bytes) {
  int rc = update_args(p, "mi_policy_update_lr: ", tasks, batch, epochs);
  if (rc) return rc;
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.tstride = tstride; c.sup = {states, actions, adv, count, done}; c.tasks = tasks; c.batch = batch;
  c.loss_kind = loss_kind; c.steps = epochs; c.clip = clip; c.head_only = head_only; c.theta_out = theta_out; c.loss_out = loss_out;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.step.vec = lr_vec; c.step.rows = 1; c.step.fn = "mi_policy_update_lr";
  rc = check_table(p, c.step, 1, ONE_STEP, tasks, batch);
  return rc ? rc : policy_update_impl(p, c);
}

// =====================================================================================================================
// MAML-TRPO with any number K of inner updates (params['adapt_steps']): meta_surrogate_loss replays `steps` second-order
// trpo_update calls, one per support replay (rl.py:447-453), before the surrogate / KL on the query replay.  With
// J = d theta_K / d theta = prod_k (I - lr H_k(theta_k)):
//   grad mean_t S_t = mean_t J_t^T grad S_t(theta_K)                 (adjoint recursion, as in mi_policy_meta_batch)
//   Fvp(v)          = mean_t J_t^T F_t J_t v + damping v              (tangent recursion forward, Fisher at the query, adjoint back;
//                                                                     exact where the adapted policy equals the stored old one)
// K = 1 of a policy the fused sweeps support (policy_sweep.h) runs the same passes as sweeps + folds: a fast path that leaves
// everything in the slots of the per-layer loop (StepSet 0, the query set, theta_0 and theta_1), not a second algorithm.
struct StepsPlan : MetaPlan {
  float *loss_t, *kl_t;                 // [T] per-task surrogate loss and KL
  float* partial;                       // fused sweeps: [T][slots][P + 2] per-workgroup gradient partials (K = 1, supported policy)
  int spt, spw, slots, sweep_grid;
};
// geometry of the fused sweeps: slabs of 32 rows, a contiguous run of slabs per workgroup, one round of workgroups on 256 CUs
static void sweep_geometry(int T, int B, int& spt, int& spw, int& slots, int& grid) {
  spt = ceil_div(B, 32);
  const int total = T * (spt + 1);      // virtual slabs: a marker in front of every task's slabs (policy_sweep.hip: what entering a task costs)
  spw = ceil_div(total, 256);
  grid = ceil_div(total, spw);
  slots = ceil_div(spt + 1, spw) + 1;
}
static bool sweep_supported(const mi_policy* p) {
  return policy_sweep_supported(p->act == ACT_RELU, p->H1, p->H2, p->S, p->A);
}
static bool fused_steps(const mi_policy* p, int K) { return K == 1 && g_policy_fused_fvp && sweep_supported(p); }
static void steps_plan(const mi_policy* p, void* ws, int T, int B, int K, StepsPlan& pl) {
  meta_plan(p, ws, T, B, K, 1, true, pl);
  PBump b{reinterpret_cast<char*>(ws), pl.bytes};
  pl.loss_t = b.f((size_t)2 * T); pl.kl_t = ws ? pl.loss_t + T : nullptr;
  sweep_geometry(T, B, pl.spt, pl.spw, pl.slots, pl.sweep_grid);
  pl.partial = (K == 1 && sweep_supported(p)) ? b.f((size_t)T * pl.slots * (p->P + 2)) : nullptr;
  pl.bytes = align_up(b.off, 256);
}
extern "C" int mi_trpo_steps_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1 || steps < 1) return MI_ERR_ARG;
  StepsPlan pl;
  steps_plan(p, nullptr, tasks, batch, steps, pl);
  *bytes = pl.bytes;
  return MI_OK;
}

// theta_k sits at pl.theta + k T P.  theta_0 is shared by all tasks: one row, read with stride 0 (per-task rows of the same values
// would cost the dense kernels their shared weight reads); from k = 1 on every task has its own row.
static size_t theta_stride(const mi_policy* p, int k) { return k == 0 ? 0 : p->P; }

// inner-loss HVP on the cached pass of one update: hv = H_k v for every task (v, hv: [T][P]).  TRPO's inner loss is always A2C,
// whose f'' is identically zero: the tangent of its cotangents is gauss_kernel's G_TANGENT, which reads no StepSet::coef2 (the
// fused primal sweep does not write one; gauss2_kernel's P_TANGENT with coef2 == 0 gives the same numbers from three loops per row).
static int hvp_step(mi_policy* p, hipStream_t st, MetaPlan& pl, StepSet& s, int T, int B, const float* th, size_t ts, const SupRef& r,
                    const float* v, float* hv) {
  const size_t P = p->P;
  PCHK(p, hipMemsetAsync(hv, 0, (size_t)T * P * sizeof(float), st));
  int rc = mlp_tangent_forward(p, st, T, B, r.xs, th, ts, s.a, v, pl.ta);
  if (rc) return rc;
  GaussArgs gt{};
  gt.mu = s.a.mu; gt.mud = pl.ta.mu; gt.rho = th + p->o_sigma; gt.rstride = ts; gt.rhod = v + p->o_sigma; gt.vstride = P;
  gt.act = r.as; gt.count = r.cn; gt.coef = s.coef; gt.dmu = pl.rdmu; gt.drho = hv + p->o_sigma; gt.gstride = P;
  gt.B = B; gt.A = p->A; gt.mode = G_TANGENT;
  PCHK(p, gauss(st, T, gt));
  return mlp_tangent_backward(p, st, T, B, r.xs, th, ts, s.a, pl.ta, v, s.dmu, s.d2, s.d1, s.pre2, s.pre1, pl.rdmu, pl.r2, pl.r1, hv);
}
// x_t <- (I - lr H_k) x_t through the updates, in place on x [T][P] (pl.hv is scratch): k = 0 .. K-1 is J_t x, the tangent
// recursion; transpose walks k = K-1 .. 0 and is J_t^T x, the adjoint recursion (every H_k is symmetric: only the order differs).
// With a step-size table (d_k = the row of update k) the two are different operations:
//   tangent    x <- x - d_k (.) (H_k x)                          (step_advance in place)
//   adjoint    x <- x - H_k (d_k (.) x)                          (AdjointWalk; dir = d_k (.) x in pl.g, idle once the inner updates are done)
static int jac_apply(mi_policy* p, hipStream_t st, StepsPlan& pl, const SupStack& sup, int T, int B, int K, bool transpose,
                     const PolicyStep& step, float* x) {
  const size_t P = p->P, TP = (size_t)T * P;
  const AdjointWalk adj{p, st, T, step, false, false};
  int rc = transpose ? adj.seed(K, x, nullptr, pl.g, nullptr) : MI_OK;
  if (rc) return rc;
  for (int i = 0; i < K; ++i) {
    const int k = transpose ? K - 1 - i : i;
    const float* v = x;
    if (transpose && (rc = adj.drive(x, pl.g, &v))) return rc;
    rc = hvp_step(p, st, pl, pl.st[k], T, B, pl.theta + (size_t)k * TP, theta_stride(p, k), sup_at(p, sup, T, B, k), v, pl.hv);
    if (rc) return rc;
    rc = transpose ? adj.back(k, x, pl.hv, nullptr, nullptr, x, pl.g, nullptr) : step_advance(p, st, T, step, k, false, false, x, P, pl.hv, x);
    if (rc) return rc;
  }
  return MI_OK;
}

// ---- the fused sweeps of K = 1 (policy_sweep.h)
static SweepArgs sweep_base(const mi_policy* p, const StepsPlan& pl, int T, int B) {
  SweepArgs a{};
  a.T = T; a.B = B; a.S = p->S; a.A = p->A; a.spt = pl.spt; a.spw = pl.spw; a.slots = pl.slots; a.partial = pl.partial;
  a.pitch = (int)p->P + 2;
  a.o_sigma = (int)p->o_sigma; a.o_w1 = (int)p->o_w1; a.o_b1 = (int)p->o_b1; a.o_w2 = (int)p->o_w2; a.o_b2 = (int)p->o_b2;
  a.o_w3 = (int)p->o_w3; a.o_b3 = (int)p->o_b3; a.P = (int)p->P;
  a.stamps = g_sweep_stamps;
  return a;
}
// H_0 over the cached support pass at theta; the caller sets the direction
static SweepArgs sweep_hvp_args(const mi_policy* p, const StepsPlan& pl, int T, int B, const SupRef& r) {
  const StepSet& s = pl.st[0];
  SweepArgs hs = sweep_base(p, pl, T, B);
  hs.x = r.xs; hs.act = r.as; hs.h1 = s.a.h1; hs.h2 = s.a.h2; hs.mu = s.a.mu; hs.coef = s.coef; hs.dmu = s.dmu;
  hs.d2 = s.d2; hs.count = r.cn; hs.theta = pl.theta; hs.tstride = 0;
  return hs;
}
// the fold takes the number, or (lrv) the row [P] of the step-size table the one update reads
static FoldArgs fold_base(const mi_policy* p, const StepsPlan& pl, int T, const PolicyStep& step) {
  FoldArgs f{};
  f.partial = pl.partial; f.slots = pl.slots; f.spt = pl.spt; f.spw = pl.spw; f.T = T; f.P = (int)p->P; f.pitch = (int)p->P + 2; f.lr = step.lr;
  f.lrv = step.row(0);
  f.o_sigma = (int)p->o_sigma; f.A = p->A;
  return f;
}

// Inner update and query pass as two PRIMAL sweeps (forward + loss + backward of a pass in one launch) instead of ~22 per-layer
// launches: theta_1, loss_t / kl_t and, with want_grad, lam = grad S_t(theta_1).
static int fused_surrogate(mi_policy* p, hipStream_t st, StepsPlan& pl, const SupRef& r, const PolicyCall& c, bool want_grad) {
  const int T = c.tasks, B = c.batch;
  const size_t P = p->P;
  float* th1 = pl.theta + (size_t)T * P;
  // The pass lands where the per-layer loop keeps it (activations, dmu, d2, coef of StepSet 0), so a per-layer product or the
  // general (ANIL) product finds it.  pre2 / pre1 are not written: only a tanh policy reads them (for ReLU they meet phi'' == 0),
  // and the sweeps run ReLU policies only.
  StepSet& s = pl.st[0];
  SweepArgs sp = sweep_base(p, pl, T, B);
  sp.x = r.xs; sp.act = r.as; sp.adv = r.adv; sp.count = r.cn; sp.theta = pl.theta; sp.tstride = 0; sp.surrogate = 0;
  sp.h1_out = s.a.h1; sp.h2_out = s.a.h2; sp.mu_out = s.a.mu; sp.dmu_out = s.dmu; sp.d2_out = s.d2; sp.coef_out = s.coef;
  PCHK(p, launch_policy_sweep(st, sp, pl.sweep_grid, SW_PRIMAL));
  FoldArgs f = fold_base(p, pl, T, c.step);
  f.mode = 0; f.v = pl.theta; f.out = th1;                        // theta_1 = theta - lr g_t   (vector: - d (.) g_t)
  PCHK(p, launch_policy_sweep_fold(st, f, T));
  SweepArgs sq = sweep_base(p, pl, T, B);
  sq.x = c.qry.states; sq.act = c.qry.actions; sq.adv = c.qry.adv; sq.count = c.qry.count; sq.theta = th1; sq.tstride = P; sq.surrogate = 1;
  sq.old_loc = c.old_loc; sq.old_scale = c.old_scale; sq.fwd_only = want_grad ? 0 : 1;
  sq.h1_out = pl.q.a.h1; sq.h2_out = pl.q.a.h2; sq.mu_out = pl.q.a.mu;
  PCHK(p, launch_policy_sweep(st, sq, pl.sweep_grid, SW_PRIMAL));
  f.mode = 3; f.out = want_grad ? pl.lam : nullptr; f.loss_t = pl.loss_t; f.kl_t = pl.kl_t;      // per-task loss / KL
  f.dout = want_grad && c.step.table() ? pl.g : nullptr;          // d (.) lam: the direction of the gradient's HVP sweep
  PCHK(p, launch_policy_sweep_fold(st, f, T));
  return MI_OK;
}

// Fvp(v) as three sweeps + three folds:  A: u_t = v - lr H_t v,  B: w_t = F_t u_t,  C: out = mean_t (w_t - lr H_t w_t) + damping v
// With a step row d:  A: u_t = v - d (.) H_t v,  B: w_t = F_t u_t and d (.) w_t (same fold, into pl.g),  C: sweep along d (.) w_t,
// out = mean_t (w_t - H_t (d (.) w_t)) + damping v -- the same six launches.
static int fused_fvp(mi_policy* p, hipStream_t st, StepsPlan& pl, const SupRef& r, const PolicyCall& c) {
  const int T = c.tasks, B = c.batch, P = (int)p->P;
  float *th1 = pl.theta + (size_t)T * P, *u = pl.vmask, *w = pl.lam, *tmp = pl.hv;
  SweepArgs hs = sweep_hvp_args(p, pl, T, B, r);
  FoldArgs f = fold_base(p, pl, T, c.step);
  f.v = c.v; f.damping = c.damping;
  hs.dir = c.v; hs.dstride = 0;
  PCHK(p, launch_policy_sweep(st, hs, pl.sweep_grid, SW_HVP));
  f.mode = 0; f.out = u;
  PCHK(p, launch_policy_sweep_fold(st, f, T));
  SweepArgs fs = sweep_base(p, pl, T, B);              // over the query pass at theta_1
  fs.x = c.qry.states; fs.h1 = pl.q.a.h1; fs.h2 = pl.q.a.h2; fs.count = c.qry.count; fs.theta = th1; fs.tstride = P; fs.dir = u; fs.dstride = P;
  PCHK(p, launch_policy_sweep(st, fs, pl.sweep_grid, SW_FISHER));
  f.mode = 1; f.out = w; f.thetap = th1; f.u = u; f.dout = c.step.table() ? pl.g : nullptr;
  PCHK(p, launch_policy_sweep_fold(st, f, T));
  hs.dir = c.step.table() ? pl.g : w; hs.dstride = P;
  PCHK(p, launch_policy_sweep(st, hs, pl.sweep_grid, SW_HVP));
  f.mode = 2; f.out = tmp; f.w = w;
  if (!p->fold_counters) {               // (once per policy object: the fold leaves the counters zero again)
    const size_t nb = (size_t)ceil_div(P, 256) * sizeof(unsigned);
    if (hipMalloc(reinterpret_cast<void**>(&p->fold_counters), nb) != hipSuccess) { p->fold_counters = nullptr; (void)hipGetLastError(); }
    else PCHK(p, hipMemsetAsync(p->fold_counters, 0, nb, st));
  }
  if (p->fold_counters) {                // the mean over tasks + damping v by the last workgroup of every parameter block: no launch of its own
    // The protocol needs the counters at zero when the fold starts; its last workgroup leaves them at zero.  A fold whose launch was
    // refused leaves the flag set, and the next product re-zeroes (stream-ordered, 4 * ceil(P / 256) bytes) instead of waiting for a
    // "last" workgroup that can no longer exist.  One stream per mi_policy at a time (include/mi_maml.h).
    if (p->fold_dirty) PCHK(p, hipMemsetAsync(p->fold_counters, 0, (size_t)ceil_div(P, 256) * sizeof(unsigned), st));
    p->fold_dirty = true;
    f.counter = p->fold_counters; f.mean_out = c.out; f.inv_T = 1.f / (float)T;
    PCHK(p, launch_policy_sweep_fold(st, f, T));
    p->fold_dirty = false;
    return MI_OK;
  }
  PCHK(p, launch_policy_sweep_fold(st, f, T));
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, tmp, T, P, 1.f / (float)T, c.v, c.damping, c.out);
  PCHK(p, hipGetLastError());
  return MI_OK;
}

// meta_surrogate_loss (rl.py:441-473) at theta for `tasks` tasks with `steps` second-order inner updates on the support replays
// ([steps][tasks][batch][.]), and optionally its gradient (rl.py:413-416).  Leaves everything the products need in `workspace`.
static int trpo_surrogate_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  if (!p || !c.theta || !c.sup.states || !c.sup.actions || !c.sup.adv || !c.qry.states || !c.qry.actions || !c.qry.adv || !c.old_loc || !c.old_scale || !c.loss_out ||
      !c.kl_out || !c.workspace || c.steps < 1)
    return pfail(p, MI_ERR_ARG, fn + "null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int T = c.tasks, B = c.batch, K = c.steps;
  const size_t P = p->P, TP = (size_t)T * P;
  StepsPlan pl;
  steps_plan(p, c.workspace, T, B, K, pl);
  if (pl.bytes > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(pl.bytes));
  const bool fused = fused_steps(p, K);
  float* thK = pl.theta + (size_t)K * TP;
  int rc = MI_OK;
  // theta_0 (one row).  The products take no theta: they read this copy.
  hipLaunchKernelGGL(axpy_bcast_kernel, dim3(ceil_div((int)P, 256), 1), dim3(256), 0, st, c.theta, (size_t)0, pl.g, 0.f, (int)P, pl.theta);
  PCHK(p, hipGetLastError());
  if (fused) {
    rc = fused_surrogate(p, st, pl, sup_at(p, c.sup, T, B, 0), c, c.grad_out != nullptr);
    if (rc) return rc;
  } else {
    for (int k = 0; k < K; ++k) {                                 // trpo_update on support replay k (a2c loss, normalised advantages)
      const SupRef r = sup_at(p, c.sup, T, B, k);
      float* th = pl.theta + (size_t)k * TP;
      const size_t ts = theta_stride(p, k);
      rc = meta_primal(p, st, T, B, 0.f, pl.st[k], th, ts, r.xs, r.as, r.adv, r.cn, MI_PLOSS_A2C, nullptr, 0, pl.g,
                       pl.hv /* step loss: unused */, nullptr);
      if (rc) return rc;
      rc = step_advance(p, st, T, c.step, k, false, false, th, ts, pl.g, th + TP);
      if (rc) return rc;
    }
    rc = mlp_forward(p, st, T, B, c.qry.states, thK, P, pl.q.a);
    if (rc) return rc;
    PCHK(p, hipMemsetAsync(pl.lam, 0, TP * sizeof(float), st));
    GaussArgs gq{};
    gq.mu = pl.q.a.mu; gq.rho = thK + p->o_sigma; gq.rstride = P; gq.act = c.qry.actions; gq.adv = c.qry.adv; gq.count = c.qry.count;
    gq.old_loc = c.old_loc; gq.old_scale = c.old_scale; gq.coef = pl.q.coef; gq.dmu = pl.q.dmu; gq.drho = pl.lam + p->o_sigma;
    gq.gstride = P; gq.loss = pl.loss_t; gq.kl = pl.kl_t; gq.B = B; gq.A = p->A; gq.mode = G_SURROGATE;
    PCHK(p, gauss(st, T, gq));
  }
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(1), dim3(64), 0, st, pl.loss_t, T, 1, 1.f / (float)T, (const float*)nullptr, 0.f, c.loss_out);
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(1), dim3(64), 0, st, pl.kl_t, T, 1, 1.f / (float)T, (const float*)nullptr, 0.f, c.kl_out);
  PCHK(p, hipGetLastError());
  if (!c.grad_out) return MI_OK;
  const float* gt = pl.lam;                                       // J_t^T grad S_t(theta_K)
  if (fused) {                                                    // one HVP sweep along lam_t + fold, instead of ~10 per-layer launches
    SweepArgs hs = sweep_hvp_args(p, pl, T, B, sup_at(p, c.sup, T, B, 0));
    hs.dir = c.step.table() ? pl.g : pl.lam; hs.dstride = P;      // (vector: d (.) lam, written by the fold that finished lam)
    PCHK(p, launch_policy_sweep(st, hs, pl.sweep_grid, SW_HVP));
    FoldArgs f = fold_base(p, pl, T, c.step);
    f.mode = 2; f.out = pl.hv; f.w = pl.lam;
    PCHK(p, launch_policy_sweep_fold(st, f, T));
    gt = pl.hv;
  } else {
    rc = mlp_backward(p, st, T, B, c.qry.states, thK, P, pl.q.a, pl.q.dmu, pl.q.d2, pl.q.d1, pl.lam);
    if (rc) return rc;
    rc = jac_apply(p, st, pl, c.sup, T, B, K, true, c.step, pl.lam);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, gt, T, (int)P, 1.f / (float)T,
                     (const float*)nullptr, 0.f, c.grad_out);
  PCHK(p, hipGetLastError());
  return MI_OK;
}
extern "C" int mi_trpo_surrogate_steps(mi_policy* p, void* stream, const float* theta, int steps, const float* s_states,
                                       const float* s_actions, const float* s_adv, const int32_t* s_count, const float* q_states,
                                       const float* q_actions, const float* q_adv, const int32_t* q_count, const float* old_loc,
                                       const float* old_scale, int tasks, int batch, float inner_lr, float* loss_out,
                                       float* kl_out, float* grad_out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, s_adv, s_count, nullptr}; c.qry = {q_states, q_actions, q_adv, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.theta = theta; c.old_loc = old_loc; c.old_scale = old_scale; c.loss_out = loss_out; c.kl_out = kl_out; c.grad_out = grad_out; c.step.lr = inner_lr;
  return trpo_surrogate_impl(p, c);
}
extern "C" int mi_policy_adapt_lr(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states,
                                  const float* actions, const float* adv, const int32_t* count, int tasks, int batch, const float* lr_vec,
                                  int head_only, float* theta_out, float* loss_out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.theta = theta; c.tstride = tstride; c.sup = {states, actions, adv, count, nullptr}; c.tasks = tasks; c.batch = batch;
  c.head_only = head_only; c.theta_out = theta_out; c.loss_out = loss_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.step.vec = lr_vec; c.step.rows = 1; c.step.fn = "mi_policy_adapt_lr";
  const int rc = check_table(p, c.step, 1, ONE_STEP, tasks, batch);
  return rc ? rc : policy_adapt_impl(p, c);
}
// The fused sweeps and the per-layer recursions take their extra direction d (.) x in the plan's g slot, idle once the inner updates are
// done: the MAML-TRPO plan does not grow.
extern "C" int mi_trpo_steps_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int lr_rows, size_t* bytes) {
  if (lr_rows < 1 || lr_rows > MI_POLICY_LR_MAX_ROWS) return MI_ERR_ARG;
  return mi_trpo_steps_workspace_bytes(p, tasks, batch, steps, bytes);
}
extern "C" int mi_trpo_surrogate_steps_lr(mi_policy* p, void* stream, const float* theta, int steps, const float* s_states,
                                          const float* s_actions, const float* s_adv, const int32_t* s_count, const float* q_states,
                                          const float* q_actions, const float* q_adv, const int32_t* q_count, const float* old_loc,
                                          const float* old_scale, int tasks, int batch, const float* lr_vec, int lr_rows,
                                          const int32_t* step_lr_row, float* loss_out, float* kl_out, float* grad_out, void* workspace,
                                          size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, s_adv, s_count, nullptr}; c.qry = {q_states, q_actions, q_adv, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.theta = theta; c.old_loc = old_loc; c.old_scale = old_scale; c.loss_out = loss_out; c.kl_out = kl_out; c.grad_out = grad_out;
  c.step.vec = lr_vec; c.step.rows = lr_rows; c.step.step_row = step_lr_row; c.step.fn = "mi_trpo_surrogate_steps_lr";
  const int rc = check_table(p, c.step, steps, TRPO_STEPS, tasks, batch);
  return rc ? rc : trpo_surrogate_impl(p, c);
}

// Fvp(v) = mean_t J_t^T F_t J_t v + damping v (cherry trpo.hessian_vector_product of the mean KL at the point where the adapted
// policy equals the old policy, rl.py:417), at the theta of the preceding mi_trpo_surrogate_steps on this workspace and replays.
static int trpo_fvp_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  if (!p || !c.sup.states || !c.sup.actions || !c.qry.states || !c.v || !c.out || !c.workspace || c.steps < 1) return pfail(p, MI_ERR_ARG, fn + "null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int T = c.tasks, B = c.batch, K = c.steps;
  const size_t P = p->P, TP = (size_t)T * P;
  StepsPlan pl;
  steps_plan(p, c.workspace, T, B, K, pl);
  if (pl.bytes > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small");
  if (fused_steps(p, K)) return fused_fvp(p, st, pl, sup_at(p, c.sup, T, B, 0), c);
  // u = J v   (pl.vmask holds u)
  hipLaunchKernelGGL(axpy_bcast_kernel, dim3(ceil_div((int)P, 256), T), dim3(256), 0, st, c.v, (size_t)0, pl.g, 0.f, (int)P, pl.vmask);
  PCHK(p, hipGetLastError());
  int rc = jac_apply(p, st, pl, c.sup, T, B, K, false, c.step, pl.vmask);
  if (rc) return rc;
  // w = F u at the query (Gaussian Fisher at new == old)
  float* thK = pl.theta + (size_t)K * TP;
  rc = mlp_tangent_forward(p, st, T, B, c.qry.states, thK, P, pl.q.a, pl.vmask, pl.ta);
  if (rc) return rc;
  PCHK(p, hipMemsetAsync(pl.lam, 0, TP * sizeof(float), st));
  GaussArgs gf{};
  gf.mu = pl.q.a.mu; gf.mud = pl.ta.mu; gf.rho = thK + p->o_sigma; gf.rstride = P; gf.rhod = pl.vmask + p->o_sigma; gf.vstride = P;
  gf.count = c.qry.count; gf.dmu = pl.rdmu; gf.drho = pl.lam + p->o_sigma; gf.gstride = P; gf.B = B; gf.A = p->A; gf.mode = G_FISHER;
  PCHK(p, gauss(st, T, gf));
  rc = mlp_backward(p, st, T, B, c.qry.states, thK, P, pl.q.a, pl.rdmu, pl.r2, pl.r1, pl.lam);
  if (rc) return rc;
  // out = mean_t J^T w + damping v
  rc = jac_apply(p, st, pl, c.sup, T, B, K, true, c.step, pl.lam);
  if (rc) return rc;
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, pl.lam, T, (int)P, 1.f / (float)T, c.v, c.damping, c.out);
  PCHK(p, hipGetLastError());
  return MI_OK;
}
extern "C" int mi_trpo_fvp_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                 const int32_t* s_count, const float* q_states, const int32_t* q_count, int tasks, int batch,
                                 float inner_lr, float damping, const float* v, float* out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.damping = damping; c.v = v; c.out = out;
  c.step.lr = inner_lr;
  return trpo_fvp_impl(p, c);
}
extern "C" int mi_trpo_fvp_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                    const int32_t* s_count, const float* q_states, const int32_t* q_count, int tasks, int batch,
                                    const float* lr_vec, int lr_rows, const int32_t* step_lr_row, float damping, const float* v, float* out,
                                    void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.damping = damping; c.v = v; c.out = out;
  c.step.vec = lr_vec; c.step.rows = lr_rows; c.step.step_row = step_lr_row; c.step.fn = "mi_trpo_fvp_steps_lr";
  const int rc = check_table(p, c.step, steps, TRPO_STEPS, tasks, batch);
  return rc ? rc : trpo_fvp_impl(p, c);
}

// =====================================================================================================================
// Exact Hessian-vector product of the mean KL where the re-adapted policy differs from the stored old one: ANIL-TRPO.
// The reference's anil_trpo.py adapts the stored old policies with the body under no_grad (core_functions/rl.py:381-382), but
// meta_surrogate_loss replays the inner step on clone_module(policy) with every parameter (rl.py:447-453): at the current
// parameters new != old, the KL gradient c_t = grad KL_t(theta'_t) is not zero, and
//   Hess_theta KL_t(theta'_t(theta)) v = J_t^T [Hess KL_t(theta'_t)] J_t v  -  lr * T_t[v, c_t],      J_t = I - lr H_t(theta),
// T_t[v, c] = d/d eps ( H_t(theta + eps v) c ): the third derivative of the inner loss contracted with v and c.  Hess KL u is a
// forward-over-reverse sweep over the query pass with the EXACT output Hessian of KL(new || old) (diag: 1/sigma_old^2 on the
// mean, 2 (sigma/sigma_old)^2 on log sigma) and a non-zero primal cotangent; T_t[v, c] = R_v{R_c{grad L_t}} is a SECOND-order
// tangent sweep over the support pass: every quantity carries a c-tangent, a v-tangent and a mixed (cv) tangent,
//   z_cv = W_c h_v + W_v h_c + W h_cv,     h_cv = phi' z_cv + phi'' z_c z_v,
//   dz_cv = phi' dh_cv + phi'' (z_v dh_c + z_c dh_v) + (phi''' z_c z_v + phi'' z_cv) dh,
//   dW_cv = dz_cv^T h + dz_c^T h_v + dz_v^T h_c + dz^T h_cv,     dh_in_cv = dz_cv W + dz_c W_v + dz_v W_c
// (tanh: phi' = 1 - h^2 =: p, phi'' = -2 h p, phi''' = p (6 h^2 - 2); ReLU: phi'' = phi''' = 0).  The c-tangent sweep depends on
// the context only and is computed once (mi_trpo_kl_prepare_steps); v-tangent and mixed sweeps run per product.  All dense products
// go through the same fp32 matrix-pipe kernels as above with up to four summed terms.
struct EwArgs {
  const float* h;                         // stored activation of the layer
  const float *a0, *a1, *a2, *a3, *a4, *a5, *a6;
  float* out;
  size_t n;
  int act, mode;
};
enum { EW_ACT_T = 0, EW_ACT_CV = 1, EW_GATE_T = 2, EW_GATE_CV = 3 };
//  EW_ACT_T   out = p a0                                                      h_t from z_t = a0
//  EW_ACT_CV  out = p a0 + phi'' a1 a2                                        h_cv from z_cv = a0 (null: 0), z_c = a1, z_v = a2
//  EW_GATE_T  out = p a0 + phi'' a1 a2                                        dz_t from dh_t = a0, z_t = a1, dh = a2
//  EW_GATE_CV out = p a0 + phi'' (a1 a2 + a3 a4) + (phi''' a3 a1 + phi'' a5) a6
//             dz_cv from dh_cv = a0, z_v = a1, dh_c = a2, z_c = a3, dh_v = a4, z_cv = a5 (null: 0), dh = a6
__global__ __launch_bounds__(256) void ew_kernel(EwArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const float h = a.h[i];
  float p, p2, p3;
  if (a.act == ACT_TANH) { p = 1.f - h * h; p2 = -2.f * h * p; p3 = p * (6.f * h * h - 2.f); }
  else { p = h > 0.f ? 1.f : 0.f; p2 = 0.f; p3 = 0.f; }
  float o;
  if (a.mode == EW_ACT_T) o = p * a.a0[i];
  else if (a.mode == EW_ACT_CV || a.mode == EW_GATE_T) o = (a.a0 ? p * a.a0[i] : 0.f) + p2 * a.a1[i] * a.a2[i];
  else {
    const float zv = a.a1[i], zc = a.a3[i];
    o = p * a.a0[i] + p2 * (zv * a.a2[i] + zc * a.a4[i]) + (p3 * zc * zv + (a.a5 ? p2 * a.a5[i] : 0.f)) * a.a6[i];
  }
  a.out[i] = o;
}
static hipError_t ew(hipStream_t st, int act, int mode, size_t n, const float* h, float* out, const float* a0, const float* a1 = nullptr,
                     const float* a2 = nullptr, const float* a3 = nullptr, const float* a4 = nullptr, const float* a5 = nullptr,
                     const float* a6 = nullptr) {
  EwArgs a{h, a0, a1, a2, a3, a4, a5, a6, out, n, act, mode};
  hipLaunchKernelGGL(ew_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

struct FTerm { const float* x; const float* w; size_t ws; };
// y = sum_k x_k w_k^T (+ bias): raw pre-activation, no gate
static hipError_t dense_fwd_n(hipStream_t st, int T, int B, int I, int O, const FTerm* tm, int n, const float* bias, size_t bs, float* y) {
  DenseArgs a{};
  for (int k = 0; k < n; ++k) { a.x[k] = tm[k].x; a.w[k] = tm[k].w; a.wstride[k] = tm[k].ws; }
  a.bias = bias; a.bstride = bs; a.y = y; a.B = B; a.I = I; a.O = O; a.nterms = n; a.act = ACT_NONE;
  launch_dense<true>(st, T, a);
  return hipGetLastError();
}
// dx = sum_k dy_k w_k: raw cotangent w.r.t. the layer input (before any phi' factor)
static hipError_t dense_bwd_x_n(hipStream_t st, int T, int B, int I, int O, const FTerm* tm, int n, float* dx) {
  DenseArgs a{};
  for (int k = 0; k < n; ++k) { a.x[k] = tm[k].x; a.w[k] = tm[k].w; a.wstride[k] = tm[k].ws; }
  a.y = dx; a.B = B; a.I = I; a.O = O; a.nterms = n; a.act = ACT_NONE;
  launch_dense<false>(st, T, a);
  return hipGetLastError();
}
struct WTerm { const float* dy; const float* x; };
static hipError_t dense_bwd_w_n(hipStream_t st, int T, int B, int I, int O, const WTerm* tm, int n, float* dw, float* db, size_t gs) {
  DenseWArgs a{};
  for (int k = 0; k < n; ++k) { a.dy[k] = tm[k].dy; a.x[k] = tm[k].x; }
  a.dw = dw; a.db = db; a.gstride = gs; a.B = B; a.I = I; a.O = O; a.nterms = n;
  hipLaunchKernelGGL(dense_wgrad_mfma_kernel, dim3(ceil_div(O, 32) * ceil_div(I + 1, 32), T), dim3(512), 0, st, a);
  return hipGetLastError();
}

struct GaussKlArgs {
  const float* mu;        // [T][B][A] policy mean on this pass
  const float* rho; size_t rstride;        // log-sigma parameter
  const float* old_loc; const float* old_scale;      // KL modes
  const float* mud;       // KL_HESS: tangent of mu;  TAN2: mixed tangent mu_cv
  const float* rhod; size_t vstride;                 // KL_HESS: tangent of rho
  const float *muc, *muv;                            // TAN2: first tangents of mu
  const float* rhoc; size_t cstride;                 // TAN2: c-direction of rho
  const float* rhov; size_t vvstride;                // TAN2: v-direction of rho
  const float* act; const float* coef;               // TAN2: actions, dL/dlogp per sample
  const int32_t* count;
  float* dmu; float* drho; size_t gstride;
  int B, A, mode;
};
enum { KL_GRAD = 0, KL_HESS = 1, G_TAN2 = 2 };
// One workgroup per task.
//  KL_GRAD  cotangent of mean KL(new || old):       dmu = (mu - mu_old) / (B D s_old^2),   drho = (vr - 1) / D,  vr = (s / s_old)^2
//  KL_HESS  its exact output Hessian times (mud, rhod):  dmu = mud / (B D s_old^2),        drho = 2 vr rhod / D
//  G_TAN2   second tangent of the A2C log-prob cotangents (kappa = coef / D, d = a - mu, iv = exp(-2 rho)):
//           R_cv{g_mu}  = kappa [ -mu_cv iv + 2 iv (mu_c rho_v + mu_v rho_c) + 4 d iv rho_c rho_v ]
//           R_cv{g_rho} = kappa [ 2 mu_c mu_v iv - 2 d mu_cv iv + 4 d iv (mu_c rho_v + mu_v rho_c) + 4 d^2 iv rho_c rho_v ]
__global__ __launch_bounds__(256) void gauss_kl_kernel(GaussKlArgs a) {
  __shared__ float red[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int B = a.B, A = a.A, cnt = a.count ? a.count[t] : B;
  const float invB = 1.f / (float)cnt, invD = 1.f / (float)A;
  float acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = 0.f;
  for (int b = tid; b < B; b += 256) {
    const bool valid = b < cnt;
    const size_t ob = (size_t)t * B + b;
    for (int d = 0; d < A; ++d) {
      const float rp = a.rho[(size_t)t * a.rstride + d];
      const bool live = rp > LOG_EPS;
      const float r = fmaxf(rp, LOG_EPS);
      if (a.mode == G_TAN2) {
        const float iv = expf(-2.f * r);
        const float kap = valid ? a.coef[ob] * invD : 0.f;
        const float df = a.act[ob * A + d] - a.mu[ob * A + d];
        const float mc = a.muc[ob * A + d], mv = a.muv[ob * A + d], mcv = a.mud[ob * A + d];
        const float rc = live ? a.rhoc[(size_t)t * a.cstride + d] : 0.f, rv = live ? a.rhov[(size_t)t * a.vvstride + d] : 0.f;
        a.dmu[ob * A + d] = kap * (-mcv * iv + 2.f * iv * (mc * rv + mv * rc) + 4.f * df * iv * rc * rv);
        if (live) acc[d] += kap * (2.f * mc * mv * iv - 2.f * df * mcv * iv + 4.f * df * iv * (mc * rv + mv * rc) + 4.f * df * df * iv * rc * rv);
      } else {
        const float so = a.old_scale[(size_t)t * A + d];
        const float w = valid ? invB * invD / (so * so) : 0.f;
        a.dmu[ob * A + d] = a.mode == KL_GRAD ? w * (a.mu[ob * A + d] - a.old_loc[ob * A + d]) : w * a.mud[ob * A + d];
      }
    }
  }
  for (int k = 0; k < A; ++k) {
    float v;
    if (a.mode == G_TAN2) {
      red[tid] = acc[k];
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      v = red[0];
      __syncthreads();
    } else {
      const float rp = a.rho[(size_t)t * a.rstride + k];
      const float sg = expf(fmaxf(rp, LOG_EPS)), so = a.old_scale[(size_t)t * A + k], vr = (sg / so) * (sg / so);
      v = rp > LOG_EPS ? (a.mode == KL_GRAD ? (vr - 1.f) * invD : 2.f * vr * a.rhod[(size_t)t * a.vstride + k] * invD) : 0.f;
    }
    if (tid == 0 && a.drho) a.drho[(size_t)t * a.gstride + k] = v;
  }
}

struct TanSweep { float *z1, *h1, *z2, *h2, *mu, *rdmu, *dh2, *dz2, *dh1, *dz1; };
struct MixSweep { float *hcv1, *zcv2, *hcv2, *mucv, *rdmu_cv, *dh2cv, *dz2cv, *dh1cv, *dz1cv; };      // scratch of the mixed sweep
static void tan_plan(const mi_policy* p, PBump& b, size_t TB, TanSweep& s) {
  s.z1 = b.f(TB * p->H1); s.h1 = b.f(TB * p->H1); s.z2 = b.f(TB * p->H2); s.h2 = b.f(TB * p->H2); s.mu = b.f(TB * p->A);
  s.rdmu = b.f(TB * p->A); s.dh2 = b.f(TB * p->H2); s.dz2 = b.f(TB * p->H2); s.dh1 = b.f(TB * p->H1); s.dz1 = b.f(TB * p->H1);
}
static void mix_plan(const mi_policy* p, PBump& b, size_t TB, MixSweep& m) {
  m.hcv1 = b.f(TB * p->H1); m.zcv2 = b.f(TB * p->H2); m.hcv2 = b.f(TB * p->H2); m.mucv = b.f(TB * p->A); m.rdmu_cv = b.f(TB * p->A);
  m.dh2cv = b.f(TB * p->H2); m.dz2cv = b.f(TB * p->H2); m.dh1cv = b.f(TB * p->H1); m.dz1cv = b.f(TB * p->H1);
}
// The cached primal pass a tangent sweep runs over: activations, cotangents (dmu, dz2; pre2 / pre1 before the phi' factor) and
// dL/dlogp per sample -- the StepSet of inner update k.
struct PassRef { const float *h1, *h2, *mu, *dmu, *d2, *pre2, *pre1, *coef; };
static PassRef pass_of(const StepSet& s) { return {s.a.h1, s.a.h2, s.a.mu, s.dmu, s.d2, s.pre2, s.pre1, s.coef}; }

// First-order tangent sweep over a cached support pass at theta (stride ts floats per task, 0 = shared) along direction d (stride
// ds, 0 = one direction for all tasks), keeping the pre-activation tangents the mixed sweep needs.  R{d L / d sigma} lands in
// drho_out + o_sigma (rows of P floats).
static int tan_sweep(mi_policy* p, hipStream_t st, const PassRef& ps, int T, int B, const float* theta, size_t ts, const float* xs,
                     const float* as, const int32_t* cn, const float* d, size_t ds, TanSweep& s, float* drho_out) {
  const size_t TB = (size_t)T * B;
  { FTerm tm[1] = {{xs, d + p->o_w1, ds}};
    PCHK(p, dense_fwd_n(st, T, B, p->S, p->H1, tm, 1, d + p->o_b1, ds, s.z1)); }
  PCHK(p, ew(st, p->act, EW_ACT_T, TB * p->H1, ps.h1, s.h1, s.z1));
  { FTerm tm[2] = {{ps.h1, d + p->o_w2, ds}, {s.h1, theta + p->o_w2, ts}};
    PCHK(p, dense_fwd_n(st, T, B, p->H1, p->H2, tm, 2, d + p->o_b2, ds, s.z2)); }
  PCHK(p, ew(st, p->act, EW_ACT_T, TB * p->H2, ps.h2, s.h2, s.z2));
  { FTerm tm[2] = {{ps.h2, d + p->o_w3, ds}, {s.h2, theta + p->o_w3, ts}};
    PCHK(p, dense_fwd_n(st, T, B, p->H2, p->A, tm, 2, d + p->o_b3, ds, s.mu)); }
  GaussArgs ga{};
  ga.mu = ps.mu; ga.mud = s.mu; ga.rho = theta + p->o_sigma; ga.rstride = ts; ga.rhod = d + p->o_sigma; ga.vstride = ds;
  ga.act = as; ga.count = cn; ga.coef = const_cast<float*>(ps.coef); ga.dmu = s.rdmu; ga.drho = drho_out + p->o_sigma; ga.gstride = p->P;
  ga.B = B; ga.A = p->A; ga.mode = G_TANGENT;
  PCHK(p, gauss(st, T, ga));
  { FTerm tm[2] = {{s.rdmu, theta + p->o_w3, ts}, {ps.dmu, d + p->o_w3, ds}};
    PCHK(p, dense_bwd_x_n(st, T, B, p->H2, p->A, tm, 2, s.dh2)); }
  PCHK(p, ew(st, p->act, EW_GATE_T, TB * p->H2, ps.h2, s.dz2, s.dh2, s.z2, ps.pre2));
  { FTerm tm[2] = {{s.dz2, theta + p->o_w2, ts}, {ps.d2, d + p->o_w2, ds}};
    PCHK(p, dense_bwd_x_n(st, T, B, p->H1, p->H2, tm, 2, s.dh1)); }
  PCHK(p, ew(st, p->act, EW_GATE_T, TB * p->H1, ps.h1, s.dz1, s.dh1, s.z1, ps.pre1));
  return MI_OK;
}

// s3_t = T_t[v, c] = R_v{R_c{grad L_t}} over a cached support pass at theta (stride ts): the mixed (cv) second-order tangent sweep
// from the first-order sweeps C (along c, stride cs) and V (along v, stride vs).  s3 [T][P] must be zero on entry.
static int mixed_sweep(mi_policy* p, hipStream_t st, const PassRef& ps, int T, int B, const float* theta, size_t ts, const float* xs,
                       const float* as, const int32_t* cn, const float* c, size_t cs, const float* v, size_t vs, const TanSweep& C,
                       const TanSweep& V, const MixSweep& m, float* s3) {
  const size_t P = p->P, TB = (size_t)T * B;
  PCHK(p, ew(st, p->act, EW_ACT_CV, TB * p->H1, ps.h1, m.hcv1, nullptr, C.z1, V.z1));
  { FTerm tm[3] = {{V.h1, c + p->o_w2, cs}, {C.h1, v + p->o_w2, vs}, {m.hcv1, theta + p->o_w2, ts}};
    PCHK(p, dense_fwd_n(st, T, B, p->H1, p->H2, tm, 3, nullptr, 0, m.zcv2)); }
  PCHK(p, ew(st, p->act, EW_ACT_CV, TB * p->H2, ps.h2, m.hcv2, m.zcv2, C.z2, V.z2));
  { FTerm tm[3] = {{V.h2, c + p->o_w3, cs}, {C.h2, v + p->o_w3, vs}, {m.hcv2, theta + p->o_w3, ts}};
    PCHK(p, dense_fwd_n(st, T, B, p->H2, p->A, tm, 3, nullptr, 0, m.mucv)); }
  GaussKlArgs g2{};
  g2.mu = ps.mu; g2.rho = theta + p->o_sigma; g2.rstride = ts; g2.mud = m.mucv; g2.muc = C.mu; g2.muv = V.mu;
  g2.rhoc = c + p->o_sigma; g2.cstride = cs; g2.rhov = v + p->o_sigma; g2.vvstride = vs; g2.act = as; g2.coef = ps.coef;
  g2.count = cn; g2.dmu = m.rdmu_cv; g2.drho = s3 + p->o_sigma; g2.gstride = P; g2.B = B; g2.A = p->A; g2.mode = G_TAN2;
  hipLaunchKernelGGL(gauss_kl_kernel, dim3(T), dim3(256), 0, st, g2);
  PCHK(p, hipGetLastError());
  { WTerm tm[4] = {{m.rdmu_cv, ps.h2}, {C.rdmu, V.h2}, {V.rdmu, C.h2}, {ps.dmu, m.hcv2}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->H2, p->A, tm, 4, s3 + p->o_w3, s3 + p->o_b3, P)); }
  { FTerm tm[3] = {{m.rdmu_cv, theta + p->o_w3, ts}, {C.rdmu, v + p->o_w3, vs}, {V.rdmu, c + p->o_w3, cs}};
    PCHK(p, dense_bwd_x_n(st, T, B, p->H2, p->A, tm, 3, m.dh2cv)); }
  PCHK(p, ew(st, p->act, EW_GATE_CV, TB * p->H2, ps.h2, m.dz2cv, m.dh2cv, V.z2, C.dh2, C.z2, V.dh2, m.zcv2, ps.pre2));
  { WTerm tm[4] = {{m.dz2cv, ps.h1}, {C.dz2, V.h1}, {V.dz2, C.h1}, {ps.d2, m.hcv1}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->H1, p->H2, tm, 4, s3 + p->o_w2, s3 + p->o_b2, P)); }
  { FTerm tm[3] = {{m.dz2cv, theta + p->o_w2, ts}, {C.dz2, v + p->o_w2, vs}, {V.dz2, c + p->o_w2, cs}};
    PCHK(p, dense_bwd_x_n(st, T, B, p->H1, p->H2, tm, 3, m.dh1cv)); }
  PCHK(p, ew(st, p->act, EW_GATE_CV, TB * p->H1, ps.h1, m.dz1cv, m.dh1cv, V.z1, C.dh1, C.z1, V.dh1, nullptr, ps.pre1));
  { WTerm tm[1] = {{m.dz1cv, xs}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->S, p->H1, tm, 1, s3 + p->o_w1, s3 + p->o_b1, P)); }
  return MI_OK;
}

// =====================================================================================================================
// That product for any number K of inner updates (rl/anil_trpo.py --adapt_steps K).
// theta_0 = theta, theta_{k+1} = theta_k - lr grad L_k(theta_k), H_k = Hess L_k(theta_k), T_k[a, b] = d/d eps H_k(theta_k + eps a) b,
// c = grad KL_t(theta_K) on the query replay.  Differentiating the adjoint recursion of the KL gradient once more along v:
//   context (mi_trpo_kl_prepare_steps):  lam_K = c,   lam_k = lam_{k+1} - lr H_k lam_{k+1},      grad mean KL = mean_t lam_0
//   product (mi_trpo_fvp_general_steps): u_0 = v,     u_{k+1} = u_k - lr H_k u_k,
//                                        rho_K = Hess KL_t(theta_K) u_K,
//                                        rho_k = rho_{k+1} - lr H_k rho_{k+1} - lr T_k[u_k, lam_{k+1}],    out = mean_t rho_0 + damping v
// which at K = 1 is the formula above.  A first-order tangent sweep over the cached pass of update k along a direction d leaves
// every tangent the mixed sweep reads AND, through three weight-gradient products, H_k d itself: the context keeps one sweep per
// update along lam_{k+1} (it yields lam_k on the way), a product keeps one per update along u_k (it yields u_{k+1}), and only
// H_k rho_{k+1} needs a sweep of its own.  u_k and lam_{k+1} are per task (stride P), and so is theta_k for k >= 1 (theta_stride).
// Workspace: the StepsPlan of mi_trpo_surrogate_steps as a prefix (theta_k, the StepSet of every update, the query pass, the
// per-task loss / KL and the fused sweeps' partials), so the surrogate's passes are found where it left them; then the KL cotangents of the query pass, lam [K+1][T][P], u [K+1][T][P], 2 K tangent sweeps and the mixed-sweep scratch.
struct GenStepsPlan {
  float *k_dmu, *k_d2, *k_d1, *k_pre2, *k_pre1;      // KL primal cotangents on the query pass at theta_K
  float *lam, *u;                                     // [K+1][T][P]
  float *rho, *s3;                                    // [T][P]
  std::vector<TanSweep> sc, sv;                       // per update: sweeps along lam_{k+1} (context) and u_k (per product)
  MixSweep mx;
  size_t bytes;
};
static void gen_steps_plan(const mi_policy* p, void* ws, int T, int B, int K, StepsPlan& pl, GenStepsPlan& gp) {
  steps_plan(p, ws, T, B, K, pl);
  PBump b{reinterpret_cast<char*>(ws), pl.bytes};
  const size_t TB = (size_t)T * B, TP = (size_t)T * p->P;
  gp.k_dmu = b.f(TB * p->A); gp.k_d2 = b.f(TB * p->H2); gp.k_d1 = b.f(TB * p->H1); gp.k_pre2 = b.f(TB * p->H2); gp.k_pre1 = b.f(TB * p->H1);
  gp.lam = b.f(TP * (K + 1)); gp.u = b.f(TP * (K + 1)); gp.rho = b.f(TP); gp.s3 = b.f(TP);
  gp.sc.resize(K); gp.sv.resize(K);
  for (auto& s : gp.sc) tan_plan(p, b, TB, s);
  for (auto& s : gp.sv) tan_plan(p, b, TB, s);
  mix_plan(p, b, TB, gp.mx);
  gp.bytes = align_up(b.off, 256);
}
extern "C" int mi_trpo_general_steps_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1 || steps < 1) return MI_ERR_ARG;
  StepsPlan pl; GenStepsPlan gp;
  gen_steps_plan(p, nullptr, tasks, batch, steps, pl, gp);
  *bytes = gp.bytes;
  return MI_OK;
}

// tangent sweep along d kept in s, and hv = H d from it: R{d L / d sigma} by the sweep, the weights by three products
static int sweep_hvp(mi_policy* p, hipStream_t st, const PassRef& ps, int T, int B, const float* theta, size_t ts, const float* xs,
                     const float* as, const int32_t* cn, const float* d, size_t ds, TanSweep& s, float* hv) {
  const size_t P = p->P;
  PCHK(p, hipMemsetAsync(hv, 0, (size_t)T * P * sizeof(float), st));
  int rc = tan_sweep(p, st, ps, T, B, theta, ts, xs, as, cn, d, ds, s, hv);
  if (rc) return rc;
  { WTerm tm[2] = {{s.rdmu, ps.h2}, {ps.dmu, s.h2}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->H2, p->A, tm, 2, hv + p->o_w3, hv + p->o_b3, P)); }
  { WTerm tm[2] = {{s.dz2, ps.h1}, {ps.d2, s.h1}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->H1, p->H2, tm, 2, hv + p->o_w2, hv + p->o_b2, P)); }
  { WTerm tm[1] = {{s.dz1, xs}};
    PCHK(p, dense_bwd_w_n(st, T, B, p->S, p->H1, tm, 1, hv + p->o_w1, hv + p->o_b1, P)); }
  return MI_OK;
}

// The step-size-vector form keeps ONE more array behind the scalar plan, whose offsets do not move: dlam [K][T][P], row k = d_k (.) lam_{k+1},
// the direction of the context's sweep of update k and the second argument of T_k in every product.
static float* gen_lr_plan(const mi_policy* p, void* ws, const GenStepsPlan& gp, int T, int K, size_t& bytes) {
  PBump b{reinterpret_cast<char*>(ws), gp.bytes};
  float* dlam = b.f((size_t)T * p->P * K);
  bytes = align_up(b.off, 256);
  return dlam;
}
extern "C" int mi_trpo_general_steps_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int lr_rows, size_t* bytes) {
  if (!p || !bytes || tasks < 1 || batch < 1 || steps < 1 || lr_rows < 1 || lr_rows > MI_POLICY_LR_MAX_ROWS) return MI_ERR_ARG;
  StepsPlan pl; GenStepsPlan gp;
  gen_steps_plan(p, nullptr, tasks, batch, steps, pl, gp);
  (void)gen_lr_plan(p, nullptr, gp, tasks, steps, *bytes);
  return MI_OK;
}

static int steps_args(mi_policy* p, const char* fn, int steps, int tasks, int batch) {
  if (steps < 1 || tasks < 1 || batch < 1)
    return pfail(p, MI_ERR_ARG, std::string(fn) + ": steps, tasks and batch must be >= 1");
  return MI_OK;
}

// After mi_trpo_surrogate_steps(theta, steps, ...) on the same workspace and replays: the KL cotangent pass on the query replay at
// theta_K (into buffers of its own: the surrogate's query cotangents stay), lam_k for every k, and the tangent sweep of every
// update along lam_{k+1}.  kl_grad_out (optional, [P]) = d mean_t KL_t / d theta = mean_t lam_0; without it lam_0 is not formed
// (the products read lam_{k+1} only): update 0 gets its tangent sweep and no weight-gradient products.
// Table form:  lam_k = lam_{k+1} - H_k (d_k (.) lam_{k+1}).  The sweep of update k runs along dlam_k = d_k (.) lam_{k+1}, which the launch
// that finished lam_{k+1} wrote (AdjointWalk), and stays for the products like the scalar one.
static int trpo_kl_prepare_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  if (!p || !c.sup.states || !c.sup.actions || !c.qry.states || !c.old_loc || !c.old_scale || !c.workspace) return pfail(p, MI_ERR_ARG, fn + "null argument");
  int rc = steps_args(p, c.step.fn ? c.step.fn : "mi_trpo_kl_prepare_steps", c.steps, c.tasks, c.batch);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int T = c.tasks, B = c.batch, K = c.steps;
  const size_t P = p->P, TP = (size_t)T * P;
  StepsPlan pl; GenStepsPlan gp;
  gen_steps_plan(p, c.workspace, T, B, K, pl, gp);
  size_t need = gp.bytes;
  float* dlam = c.step.table() ? gen_lr_plan(p, c.workspace, gp, T, K, need) : nullptr;
  if (need > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(need));
  const float* thK = pl.theta + (size_t)K * TP;
  float* lamK = gp.lam + (size_t)K * TP;
  PCHK(p, hipMemsetAsync(lamK, 0, TP * sizeof(float), st));
  GaussKlArgs gk{};
  gk.mu = pl.q.a.mu; gk.rho = thK + p->o_sigma; gk.rstride = P; gk.old_loc = c.old_loc; gk.old_scale = c.old_scale; gk.count = c.qry.count;
  gk.dmu = gp.k_dmu; gk.drho = lamK + p->o_sigma; gk.gstride = P; gk.B = B; gk.A = p->A; gk.mode = KL_GRAD;
  hipLaunchKernelGGL(gauss_kl_kernel, dim3(T), dim3(256), 0, st, gk);
  PCHK(p, hipGetLastError());
  rc = mlp_backward(p, st, T, B, c.qry.states, thK, P, pl.q.a, gp.k_dmu, gp.k_d2, gp.k_d1, lamK, gp.k_pre2, gp.k_pre1);
  if (rc) return rc;
  const AdjointWalk adj{p, st, T, c.step, false, false};
  auto dlam_of = [&](int k) { return dlam && k >= 0 ? dlam + (size_t)k * TP : (float*)nullptr; };
  rc = adj.seed(K, lamK, nullptr, dlam_of(K - 1), nullptr);
  if (rc) return rc;
  for (int k = K - 1; k >= 0; --k) {
    const float *lam1 = gp.lam + (size_t)(k + 1) * TP, *dir;
    rc = adj.drive(lam1, dlam_of(k), &dir);
    if (rc) return rc;
    const SupRef r = sup_at(p, c.sup, T, B, k);
    if (k == 0 && !c.grad_out)      // (pl.hv takes the sweep's R{d L / d sigma}: scratch)
      return tan_sweep(p, st, pass_of(pl.st[0]), T, B, pl.theta, theta_stride(p, 0), r.xs, r.as, r.cn, dir, P, gp.sc[0], pl.hv);
    rc = sweep_hvp(p, st, pass_of(pl.st[k]), T, B, pl.theta + (size_t)k * TP, theta_stride(p, k), r.xs, r.as, r.cn, dir, P, gp.sc[k], pl.hv);
    if (rc) return rc;
    rc = adj.back(k, lam1, pl.hv, nullptr, nullptr, gp.lam + (size_t)k * TP, dlam_of(k - 1), nullptr);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, gp.lam, T, (int)P, 1.f / (float)T,
                     (const float*)nullptr, 0.f, c.grad_out);
  PCHK(p, hipGetLastError());
  return MI_OK;
}
extern "C" int mi_trpo_kl_prepare_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                        const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_loc,
                                        const float* old_scale, int tasks, int batch, float inner_lr, float* kl_grad_out,
                                        void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.old_loc = old_loc; c.old_scale = old_scale; c.grad_out = kl_grad_out;
  c.step.lr = inner_lr;
  return trpo_kl_prepare_impl(p, c);
}
extern "C" int mi_trpo_kl_prepare_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                           const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_loc,
                                           const float* old_scale, int tasks, int batch, const float* lr_vec, int lr_rows,
                                           const int32_t* step_lr_row, float* kl_grad_out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.old_loc = old_loc; c.old_scale = old_scale; c.grad_out = kl_grad_out;
  c.step.vec = lr_vec; c.step.rows = lr_rows; c.step.step_row = step_lr_row; c.step.fn = "mi_trpo_kl_prepare_steps_lr";
  const int rc = check_table(p, c.step, steps, TRPO_STEPS, tasks, batch);
  return rc ? rc : trpo_kl_prepare_impl(p, c);
}

// trpo.hessian_vector_product(mean KL, params, damping)(v) (rl.py:417) at the parameters of the preceding
// mi_trpo_surrogate_steps + mi_trpo_kl_prepare_steps on this workspace; any number of calls.  11 + 36 K kernels and 1 + 3 K
// memsets, whatever the number of tasks.
// Table form:  u_{k+1} = u_k - d_k (.) (H_k u_k);   rho_k = rho_{k+1} - (H_k (d_k (.) rho_{k+1}) + T_k[u_k, d_k (.) lam_{k+1}]):  the stored
// sweeps run along u_k and along dlam_k, the sweep of its own along d_k (.) rho_{k+1} (in pl.g, written by the launch that finished rho_{k+1}).
static int trpo_fvp_general_impl(mi_policy* p, const PolicyCall& c) {
  const std::string fn = c.step.prefix();
  if (!p || !c.sup.states || !c.sup.actions || !c.qry.states || !c.old_scale || !c.v || !c.out || !c.workspace) return pfail(p, MI_ERR_ARG, fn + "null argument");
  int rc = steps_args(p, c.step.fn ? c.step.fn : "mi_trpo_fvp_general_steps", c.steps, c.tasks, c.batch);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int T = c.tasks, B = c.batch, K = c.steps;
  const size_t P = p->P, TP = (size_t)T * P;
  StepsPlan pl; GenStepsPlan gp;
  gen_steps_plan(p, c.workspace, T, B, K, pl, gp);
  size_t need = gp.bytes;
  const float* dlam = c.step.table() ? gen_lr_plan(p, c.workspace, gp, T, K, need) : nullptr;
  if (need > c.workspace_bytes) return pfail(p, MI_ERR_WORKSPACE, fn + "workspace too small: need " + std::to_string(need));
  // ---- u_0 = v for every task, u_{k+1} = u_k - lr H_k u_k; the sweep along u_k stays for the way back
  hipLaunchKernelGGL(axpy_bcast_kernel, dim3(ceil_div((int)P, 256), T), dim3(256), 0, st, c.v, (size_t)0, pl.g, 0.f, (int)P, gp.u);
  PCHK(p, hipGetLastError());
  for (int k = 0; k < K; ++k) {
    const SupRef r = sup_at(p, c.sup, T, B, k);
    const float* uk = gp.u + (size_t)k * TP;
    rc = sweep_hvp(p, st, pass_of(pl.st[k]), T, B, pl.theta + (size_t)k * TP, theta_stride(p, k), r.xs, r.as, r.cn, uk, P, gp.sv[k], pl.hv);
    if (rc) return rc;
    rc = step_advance(p, st, T, c.step, k, false, false, uk, P, pl.hv, gp.u + (size_t)(k + 1) * TP);
    if (rc) return rc;
  }
  // ---- rho_K = Hess KL_t(theta_K) u_K: tangent forward on the query pass, exact output Hessian, tangent backward
  const float* thK = pl.theta + (size_t)K * TP;
  const float* uK = gp.u + (size_t)K * TP;
  rc = mlp_tangent_forward(p, st, T, B, c.qry.states, thK, P, pl.q.a, uK, pl.ta);
  if (rc) return rc;
  PCHK(p, hipMemsetAsync(gp.rho, 0, TP * sizeof(float), st));
  GaussKlArgs gh{};
  gh.mu = pl.q.a.mu; gh.rho = thK + p->o_sigma; gh.rstride = P; gh.old_scale = c.old_scale; gh.mud = pl.ta.mu;
  gh.rhod = uK + p->o_sigma; gh.vstride = P; gh.count = c.qry.count; gh.dmu = pl.rdmu; gh.drho = gp.rho + p->o_sigma; gh.gstride = P;
  gh.B = B; gh.A = p->A; gh.mode = KL_HESS;
  hipLaunchKernelGGL(gauss_kl_kernel, dim3(T), dim3(256), 0, st, gh);
  PCHK(p, hipGetLastError());
  rc = mlp_tangent_backward(p, st, T, B, c.qry.states, thK, P, pl.q.a, pl.ta, uK, gp.k_dmu, gp.k_d2, gp.k_d1, gp.k_pre2, gp.k_pre1, pl.rdmu,
                            pl.r2, pl.r1, gp.rho);
  if (rc) return rc;
  // ---- rho_k = rho_{k+1} - lr (H_k rho_{k+1} + T_k[u_k, lam_{k+1}])
  const AdjointWalk adj{p, st, T, c.step, false, false};
  rc = adj.seed(K, gp.rho, nullptr, pl.g, nullptr);
  if (rc) return rc;
  for (int k = K - 1; k >= 0; --k) {
    const SupRef r = sup_at(p, c.sup, T, B, k);
    const float *th = pl.theta + (size_t)k * TP, *dir;
    const size_t ts = theta_stride(p, k);
    rc = adj.drive(gp.rho, pl.g, &dir);
    if (rc) return rc;
    rc = hvp_step(p, st, pl, pl.st[k], T, B, th, ts, r, dir, pl.hv);
    if (rc) return rc;
    PCHK(p, hipMemsetAsync(gp.s3, 0, TP * sizeof(float), st));
    rc = mixed_sweep(p, st, pass_of(pl.st[k]), T, B, th, ts, r.xs, r.as, r.cn, dlam ? dlam + (size_t)k * TP : gp.lam + (size_t)(k + 1) * TP, P,
                     gp.u + (size_t)k * TP, P, gp.sc[k], gp.sv[k], gp.mx, gp.s3);
    if (rc) return rc;
    rc = adj.back(k, gp.rho, pl.hv, gp.s3, nullptr, gp.rho, pl.g, nullptr);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mean_tasks_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, gp.rho, T, (int)P, 1.f / (float)T, c.v, c.damping, c.out);
  PCHK(p, hipGetLastError());
  return MI_OK;
}
extern "C" int mi_trpo_fvp_general_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                         const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_scale,
                                         int tasks, int batch, float inner_lr, float damping, const float* v, float* out,
                                         void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.old_scale = old_scale; c.damping = damping; c.v = v; c.out = out;
  c.step.lr = inner_lr;
  return trpo_fvp_general_impl(p, c);
}
extern "C" int mi_trpo_fvp_general_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                            const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_scale,
                                            int tasks, int batch, const float* lr_vec, int lr_rows, const int32_t* step_lr_row, float damping,
                                            const float* v, float* out, void* workspace, size_t workspace_bytes) {
  PolicyCall c{};
  c.stream = stream; c.steps = steps; c.sup = {s_states, s_actions, nullptr, s_count, nullptr}; c.qry = {q_states, nullptr, nullptr, q_count, nullptr};
  c.tasks = tasks; c.batch = batch; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.old_scale = old_scale; c.damping = damping; c.v = v; c.out = out;
  c.step.vec = lr_vec; c.step.rows = lr_rows; c.step.step_row = step_lr_row; c.step.fn = "mi_trpo_fvp_general_steps_lr";
  const int rc = check_table(p, c.step, steps, TRPO_STEPS, tasks, batch);
  return rc ? rc : trpo_fvp_general_impl(p, c);
}
