// Ridge-regression head (R2-D2: Bertinetto et al., "Meta-learning with differentiable closed-form solvers") for a whole meta-batch: the head's
// own inner problem solved to optimality on the support features, in the dual (Woodbury) form -- ns << feat everywhere here -- with
// CrossEntropyLoss(reduction='mean'), accuracy, the backward to the features and to the two hyper-parameters.  Per task,
// Y = onehot(ys) [ns, ways], lam > 0, alpha > 0:
//   G = Fs Fs^T + lam I   A = G^-1 Y   K = Fq Fs^T   P = K A   z = alpha P   loss = mean_q CE(z_q, yq_q)   dz = (softmax(z) - onehot(yq)) / nq
//   dalpha = sum(dz .* P)   dP = alpha dz   dA = K^T dP   B = G^-1 dA   dlam = -sum(B .* A)   S = -(B A^T + A B^T)   dK = dP A^T
//   dFq = dK Fs   dFs = dK^T Fq + S Fs
// (R2-D2's additive logit bias is left out: every row of dz sums to 0, so its gradient is identically 0.)  acc is the first-maximum argmax
// of the fp32 logits the call returns (head_bodies.h's rule on the values the caller sees).
// One workgroup of 512 threads per task, ONE launch for the whole meta-batch (forward, or forward + backward).  The features are fp32; every
// sum is accumulated in fp64 (products of two fp32 values are exact in fp64) and everything ns-sized lives in LDS in fp64, so the conditioning
// of G stays out of the error budget; only dP is kept in fp32.  Every sum runs in an order fixed by the task's own sizes, no float atomics,
// plain vector stores: a task's bits depend neither on `tasks` nor on the workgroup that ran it, and the forward-only launch gives the bits
// of the forward half.
//   sweep 1  G (lower triangle, packed) and K together: a wave per 4 x 4 tile of entries, lanes over (4 adjacent) feature column(s), 16 fp64
//            partial sums per lane, folded by a transposing butterfly (17 exchanges instead of 96)
//   factor   G = L D L^T in place (the square-root-free Cholesky), right-looking, ONE barrier per column: step j reads column j and the
//            pivot, writes columns > j.  A pivot that is not > 0 cannot happen for a sane lam; if it does, every output of THAT TASK is NaN
//            (a flag, no data-dependent loop or address anywhere)
//   solve    A = G^-1 Y in place: forward, diagonal, backward substitution, one barrier per column
//   head     a wave per query row: P_q = K_q A (lane = class), softmax and CE in fp64, dP -> LDS, the row's loss / hit / <dz, P>
//   (backward)  dA = K^T dP -> B, the same solve, dlam; S over G, dK over K
//   sweep 2  dFq and dFs together: a thread per (8 rows, 4 adjacent columns) block, coefficients broadcast from LDS, rows ascending
// fs and fq are read about ns/4 times in sweep 1 and (ns + 2 nq)/8 times in sweep 2; a task's features are at most 1.3 MB: L2 after the first.
// LDS (bytes): 8 * (ns (ns + 1) / 2 [G, S] + nq ns [K, dK] + ns ways [A] + ns ways [dA, B] + ns [1 / D] + 3 nq [row tables]) + 4 * nq ways [dP]
#include <cmath>
#include "mi_common.h"
#include "kernels.h"
#include "../../include/mi_maml.h"

namespace {
constexpr int kThreads = 512, kWaves = kThreads / 64, kRows = 8;

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i

struct Lds {
  double *g, *k, *a, *b, *invd, *rl, *rh, *ra;
  float* dp;
};
__device__ __forceinline__ Lds carve(double* sm, int ns, int nq, int ways) {
  Lds l;
  l.g = sm;
  l.k = l.g + (size_t)ns * (ns + 1) / 2;
  l.a = l.k + (size_t)nq * ns;
  l.b = l.a + (size_t)ns * ways;
  l.invd = l.b + (size_t)ns * ways;
  l.rl = l.invd + ns;
  l.rh = l.rl + nq;
  l.ra = l.rh + nq;
  l.dp = reinterpret_cast<float*>(l.ra + nq);
  return l;
}

// X [ns][ways] <- G^-1 X with G = L D L^T as the factor loop left it: g holds D on the diagonal and L D below it, invd = 1 / D.  The caller
// has synchronised after writing X; returns synchronised.  A step reads row k of X and writes other rows only: one barrier per step.
__device__ __forceinline__ void solve(const Lds& l, double* x, int NS, int WY, int tid) {
  const int w = tid % WY, r0 = tid / WY, rstep = kThreads / WY;
  const bool on = r0 < rstep;
  for (int k = 0; k + 1 < NS; ++k) {                    // L z = y
    const double inv = l.invd[k];
    if (on) {
      const double xk = x[k * WY + w];
      for (int i = k + 1 + r0; i < NS; i += rstep) x[i * WY + w] = fma(-(l.g[tri(i, k)] * inv), xk, x[i * WY + w]);
    }
    __syncthreads();
  }
  if (on)
    for (int i = r0; i < NS; i += rstep) x[i * WY + w] *= l.invd[i];       // D^-1
  __syncthreads();
  for (int k = NS - 1; k >= 1; --k) {                   // L^T x = .
    if (on) {
      const double xk = x[k * WY + w];
      for (int i = r0; i < k; i += rstep) x[i * WY + w] = fma(-(l.g[tri(k, i)] * l.invd[i]), xk, x[i * WY + w]);
    }
    __syncthreads();
  }
}

template <bool BWD, int VW>
__device__ __forceinline__ void ridge_task(const RidgeArgs& a, double* sm) {
  const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NS = a.ns, NQ = a.nq, F = a.feat, WY = a.ways;
  const double lam = (double)a.h.lam, alpha = (double)a.h.alpha;
  const float* fs = a.fs + (size_t)task * NS * F;
  const float* fq = a.fq + (size_t)task * NQ * F;
  const int32_t* ys = a.ys + (size_t)task * NS;
  const int32_t* yq = a.yq + (size_t)task * NQ;
  const Lds l = carve(sm, NS, NQ, WY);
  const int tx = tid & 31, ty = tid >> 5;               // the 32 x 16 thread grid of the triangular loops

  // ---- sweep 1: G + lam I (packed lower triangle) and K, a wave per 4 x 4 tile
  {
    const int nbs = (NS + 3) / 4, nbq = (NQ + 3) / 4;
    const int tg = nbs * (nbs + 1) / 2, total = tg + nbq * nbs;
    for (int t = wave; t < total; t += kWaves) {
      const bool isg = t < tg;
      int bi = 0, bj;
      if (isg) {
        int r = t;
        while (r >= bi + 1) { r -= bi + 1; ++bi; }
        bj = r;
      } else {
        bi = (t - tg) / nbs;
        bj = (t - tg) % nbs;
      }
      const float* xb = isg ? fs : fq;
      const int nx = isg ? NS : NQ;
      const float *xr[4], *yr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {                     // (rows past the end: the last row again, results dropped)
        xr[r] = xb + (size_t)min(4 * bi + r, nx - 1) * F;
        yr[r] = fs + (size_t)min(4 * bj + r, NS - 1) * F;
      }
      double acc[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0;
#pragma unroll 4                                        // (the loads of four steps in flight: the loop is bound by L2 latency, not by the FMAs)
      for (int i = lane * VW; i < F; i += 64 * VW) {
        float x[4][VW], y[4][VW];
#pragma unroll
        for (int r = 0; r < 4; ++r) { row_ld<VW>(xr[r] + i, x[r]); row_ld<VW>(yr[r] + i, y[r]); }
#pragma unroll
        for (int u = 0; u < VW; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r * 4 + c] = fma((double)x[r][u], (double)y[c][u], acc[r * 4 + c]);
      }
      // the 16 sums over the 64 lanes: every exchange halves the entries a lane still carries; entry e ends up in lanes 4 e .. 4 e + 3
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int h = 8 >> s, off = 32 >> s;
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (e < h) {
            const double keep = up ? acc[e + h] : acc[e];
            const double send = up ? acc[e] : acc[e + h];
            acc[e] = keep + __shfl_xor(send, off, 64);
          }
        }
      }
      double v = acc[0];
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 1, 64);
      if ((lane & 3) == 0) {
        const int e = (lane >> 2) & 15, i = 4 * bi + (e >> 2), j = 4 * bj + (e & 3);
        if (isg) {
          if (i < NS && j <= i) l.g[tri(i, j)] = i == j ? v + lam : v;
        } else if (i < NQ && j < NS) {
          l.k[i * NS + j] = v;
        }
      }
    }
  }
  for (int e = tid; e < NS * WY; e += kThreads) l.a[e] = ys[e / WY] == e % WY ? 1.0 : 0.0;      // Y
  __syncthreads();

  // ---- factor: G = L D L^T in place, right-looking; after step j column j holds L D and is final
  bool bad = false;
  for (int j = 0; j < NS; ++j) {
    const double d = l.g[tri(j, j)];
    bad |= !(d > 0.0);
    const double inv = 1.0 / d;
    if (tid == 0) l.invd[j] = inv;
    for (int i = j + 1 + ty; i < NS; i += 16) {
      const double lij = l.g[tri(i, j)] * inv;
      for (int k = j + 1 + tx; k <= i; k += 32) l.g[tri(i, k)] = fma(-lij, l.g[tri(k, j)], l.g[tri(i, k)]);
    }
    __syncthreads();
  }
  const float nanf_ = __builtin_nanf("");

  // ---- A = G^-1 Y
  solve(l, l.a, NS, WY, tid);

  // ---- head: a wave per query row, lane w holds P_qw
  const double invn = 1.0 / (double)NQ;
  for (int q = wave; q < NQ; q += kWaves) {
    const bool act = lane < WY;
    double p = 0.0;
    if (act)
      for (int j = 0; j < NS; ++j) p = fma(l.k[q * NS + j], l.a[j * WY + lane], p);
    const double z = alpha * p;
    const float zf = (float)z;
    const int y = yq[q];
    float mxf = act ? zf : -INFINITY;
    double mx = act ? z : -(double)INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mxf = fmaxf(mxf, __shfl_xor(mxf, off, 64));
      mx = fmax(mx, __shfl_xor(mx, off, 64));
    }
    const unsigned long long eq = __ballot(act && zf == mxf);
    const int am = __ffsll((long long)eq) - 1;          // the first maximum of the returned logits
    const double ex = act ? exp(z - mx) : 0.0;
    const double se = wave_sum(ex);
    const double ly = __shfl(z, y & 63, 64);
    const double dl = act ? (ex / se - (lane == y ? 1.0 : 0.0)) * invn : 0.0;
    const double da = wave_sum(dl * p);
    if (act) {
      l.dp[q * WY + lane] = (float)(alpha * dl);
      if (a.logits) a.logits[((size_t)task * NQ + q) * WY + lane] = bad ? nanf_ : zf;
    }
    if (lane == 0) {
      l.rl[q] = (mx + log(se)) - ly;
      l.rh[q] = am == y ? 1.0 : 0.0;
      l.ra[q] = da;
    }
  }
  __syncthreads();
  double dalpha = 0.0;                                   // (wave 0's lanes carry it to the dhyper store)
  if (wave == 0) {
    double ls = 0.0, cs = 0.0;
    for (int q = lane; q < NQ; q += 64) { ls += l.rl[q]; cs += l.rh[q]; dalpha += l.ra[q]; }
    ls = wave_sum(ls); cs = wave_sum(cs); dalpha = wave_sum(dalpha);
    if (lane == 0) {
      a.loss[task] = bad ? nanf_ : (float)(ls / (double)NQ);
      a.acc[task] = bad ? nanf_ : (float)(cs / (double)NQ);
    }
  }
  if (!BWD) return;

  // ---- dA = K^T dP into B, B = G^-1 dA, dlam
  for (int e = tid; e < NS * WY; e += kThreads) {
    const int j = e / WY, w = e % WY;
    double s = 0.0;
    for (int q = 0; q < NQ; ++q) s = fma(l.k[q * NS + j], (double)l.dp[q * WY + w], s);
    l.b[e] = s;
  }
  __syncthreads();
  solve(l, l.b, NS, WY, tid);
  if (wave == 0 && a.dhyper) {
    double s = 0.0;
    for (int e = lane; e < NS * WY; e += 64) s = fma(l.b[e], l.a[e], s);
    s = wave_sum(s);
    if (lane == 0) {
      a.dhyper[2 * (size_t)task] = bad ? nanf_ : (float)(-s);
      a.dhyper[2 * (size_t)task + 1] = bad ? nanf_ : (float)dalpha;
    }
  }
  if (!a.dfs && !a.dfq) return;

  // ---- S over G (the factor is dead), dK over K (dA is done)
  if (a.dfs) {
    for (int i = ty; i < NS; i += 16)
      for (int j = tx; j <= i; j += 32) {
        double s = 0.0;
        for (int w = 0; w < WY; ++w) {
          s = fma(l.b[i * WY + w], l.a[j * WY + w], s);
          s = fma(l.a[i * WY + w], l.b[j * WY + w], s);
        }
        l.g[tri(i, j)] = -s;
      }
  }
  for (int e = tid; e < NQ * NS; e += kThreads) {
    const int q = e / NS, j = e % NS;
    double s = 0.0;
    for (int w = 0; w < WY; ++w) s = fma((double)l.dp[q * WY + w], l.a[j * WY + w], s);
    l.k[e] = s;
  }
  __syncthreads();

  // ---- sweep 2: dFq = dK Fs and dFs = dK^T Fq + S Fs, a thread per (8 rows, VW columns) block
  const int ncg = (F + VW - 1) / VW;
  const int items_q = a.dfq ? ((NQ + kRows - 1) / kRows) * ncg : 0;
  const int items_s = a.dfs ? ((NS + kRows - 1) / kRows) * ncg : 0;
  float* dfq = a.dfq ? a.dfq + (size_t)task * NQ * F : nullptr;
  float* dfs = a.dfs ? a.dfs + (size_t)task * NS * F : nullptr;
  for (int item = tid; item < items_q + items_s; item += kThreads) {
    const bool isq = item < items_q;
    const int u0 = isq ? item : item - items_q;
    const int r0 = (u0 / ncg) * kRows, col = (u0 % ncg) * VW;
    double acc[kRows][VW];
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
      for (int u = 0; u < VW; ++u) acc[r][u] = 0.0;
    if (isq) {
#pragma unroll 4
      for (int j = 0; j < NS; ++j) {
        float x[VW];
        row_ld<VW>(fs + (size_t)j * F + col, x);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const double c = l.k[min(r0 + r, NQ - 1) * NS + j];
#pragma unroll
          for (int u = 0; u < VW; ++u) acc[r][u] = fma(c, (double)x[u], acc[r][u]);
        }
      }
    } else {
#pragma unroll 4
      for (int q = 0; q < NQ; ++q) {
        float x[VW];
        row_ld<VW>(fq + (size_t)q * F + col, x);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const double c = l.k[q * NS + min(r0 + r, NS - 1)];
#pragma unroll
          for (int u = 0; u < VW; ++u) acc[r][u] = fma(c, (double)x[u], acc[r][u]);
        }
      }
#pragma unroll 4
      for (int j = 0; j < NS; ++j) {
        float x[VW];
        row_ld<VW>(fs + (size_t)j * F + col, x);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const int i = min(r0 + r, NS - 1);
          const double c = l.g[i >= j ? tri(i, j) : tri(j, i)];
#pragma unroll
          for (int u = 0; u < VW; ++u) acc[r][u] = fma(c, (double)x[u], acc[r][u]);
        }
      }
    }
    float* out = isq ? dfq : dfs;
    const int nr = isq ? NQ : NS;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      if (r0 + r < nr) {
        float o[VW];
#pragma unroll
        for (int u = 0; u < VW; ++u) o[u] = bad ? nanf_ : (float)acc[r][u];
        row_st<VW>(out + (size_t)(r0 + r) * F + col, o);
      }
    }
  }
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void ridge_head_kernel(RidgeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ridge_sm[];
  // 16-byte global accesses when every row starts on a 16-byte boundary (the entry points require 16-byte aligned bases)
  const bool vec = a.feat % 4 == 0;
  if (vec) ridge_task<BWD, 4>(a, ridge_sm);
  else ridge_task<BWD, 1>(a, ridge_sm);
}
}  // namespace

// Dynamic LDS of one task (the kernel has no static LDS, so a request may take all of a CU's 160 KiB); feat does not enter:
//   8 * (ns (ns + 1) / 2 + nq * ns + 2 * ns * ways + ns + 3 * nq) + 4 * nq * ways <= 163840, ways <= 64, feat <= MI_RIDGE_MAX_FEAT.
// ns = nq = 100, ways = 20 (Omniglot 20-way 5-shot): 163600.
size_t ridge_head_lds_bytes(int ns, int nq, int ways) {
  const size_t s = (size_t)ns, q = (size_t)nq, w = (size_t)ways;
  return 8 * (s * (s + 1) / 2 + q * s + 2 * s * w + s + 3 * q) + 4 * q * w;
}
bool ridge_head_fits(int ns, int nq, int feat, int ways) {
  return ns >= 1 && nq >= 1 && feat >= 1 && feat <= MI_RIDGE_MAX_FEAT && ways >= 1 && ways <= 64 &&
         ridge_head_lds_bytes(ns, nq, ways) <= head_lds_limit_bytes();
}

// A request above 64 KiB needs allow_dynamic_lds (mi_common.h), raised to the device's whole LDS: head_grads_launch's rule.
template <bool BWD>
static hipError_t ridge_launch(hipStream_t st, const RidgeArgs& a, int tasks) {
  const size_t sm = ridge_head_lds_bytes(a.ns, a.nq, a.ways);
  if (sm > 64 * 1024) {
    static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(ridge_head_kernel<BWD>), head_lds_limit_bytes(), &attr_done); e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(ridge_head_kernel<BWD>, dim3(tasks), dim3(kThreads), sm, st, a);
  return hipGetLastError();
}

// Forward (a.dfs == a.dfq == a.dhyper == NULL) or forward + backward, one launch either way.  Outside the domain: hipErrorInvalidValue,
// nothing launched (callers check ridge_head_fits first and report MI_ERR_ARG).
hipError_t launch_ridge_head(hipStream_t st, const RidgeArgs& a, int tasks) {
  if (tasks < 1 || !ridge_head_fits(a.ns, a.nq, a.feat, a.ways) || !(a.h.lam > 0.f) || !(a.h.alpha > 0.f) || !std::isfinite(a.h.lam) || !std::isfinite(a.h.alpha))
    return hipErrorInvalidValue;
  return (a.dfs || a.dfq || a.dhyper) ? ridge_launch<true>(st, a, tasks) : ridge_launch<false>(st, a, tasks);
}
