// Logistic-regression head for a whole meta-batch: the head's inner problem under the loss ANIL's inner loop runs -- L2-regularised multinomial
// logistic regression (softmax cross-entropy, no bias) on the support features -- solved to optimality in the dual form and differentiated
// through the optimum by the implicit function theorem (LR-D2 of the R2-D2 paper for any number of classes; MetaOptNet's convex head; the
// test-time classifier of "Rethinking Few-Shot Image Classification").  DESIGN.md section 31.  Per task, Y = onehot(ys) [ns, ways], lam > 0, alpha > 0:
//   W* = argmin_W sum_i CE(W fs_i, ys_i) + (lam / 2) |W|^2,  W = A^T Fs:   G = Fs Fs^T   S = G A   P = softmax_rows(S)   R(A) = lam A + P - Y = 0
//   K = Fq Fs^T   Pq = K A   z = alpha Pq   loss = mean_q CE(z_q, yq_q)   dz = (softmax(z) - onehot(yq)) / nq   dalpha = sum(dz .* Pq)
//   dP = alpha dz   dK = dP A^T   dA = K^T dP   X = (lam I + D G)^-1 (D dA)   B = (dA - G X) / lam   dlam = -sum(B .* A)
//   St = -(X A^T + A X^T)   dFq = dK Fs   dFs = dK^T Fq + St Fs           (D acts row-wise: D_i = diag(p_i) - p_i p_i^T)
// acc is the first-maximum argmax of the fp32 logits the call returns.  One workgroup of 512 threads per task, ONE launch for the whole
// meta-batch (forward, or forward + backward).  The features are fp32; every sum is accumulated in fp64, everything ns-sized lives in LDS in
// fp64, and no intermediate is kept in fp32.  Every sum runs in an order fixed by the task's own sizes, no float atomics, plain vector stores:
// a task's bits depend neither on `tasks` nor on the workgroup that ran it, and the forward-only launch gives the bits of the forward half.
//   sweep 1  G and K together, the ridge head's tile scheme (a wave per 4 x 4 tile, 16 fp64 partial sums per lane, a transposing butterfly);
//            G is kept square
//   solve    Newton from A = 0 on R.  The operator lam I + D G is not symmetric; with D_i = C_i C_i^T, C_i = diag(u_i) (I - u_i u_i^T), u = sqrt(p),
//              (lam I + D G)^-1 V = (V - C (lam I + C^T G C)^-1 C^T G V) / lam
//            and lam I + C^T G C is symmetric positive definite with every eigenvalue >= lam: plain conjugate gradients from 0, stopped at
//            |r|^2 <= 1e-26 |b|^2.  A step is accepted if it lowers |R|_inf, or (while |R|_inf > 1e-10) if it meets Armijo's condition on the
//            inner objective; otherwise it is halved.  The iteration stops at |R|_inf <= 1e-13, or when |R|_inf <= 1e-10 and the step does not
//            lower it.  Every rule compares quantities that are unchanged when the features are doubled and lam quadrupled (R, the relative
//            CG residual, the objective), so that pair of calls gives the same bits up to the exact powers of two.
//   head     a wave per query row: Pq = K_q A (lane = class), softmax and CE in fp64, dP -> LDS (fp64), the row's loss / hit / <dz, Pq>
//   (backward)  dA = K^T dP, V = D dA, the same conjugate-gradient routine -> X, B, dlam; St over G, dK over K
//   sweep 2  dFq and dFs together, the ridge head's: a thread per (8 rows, 4 adjacent columns) block, coefficients broadcast from LDS
// Bounded work: no loop bound and no address depends on data; the Newton, CG and halving loops stop at MI_LOGREG_NEWTON_CAP, MI_LOGREG_CG_CAP
// and MI_LOGREG_HALVE_CAP (include/mi_maml.h) and leave at once on a residual that is not finite.  A task that has not reached
// |R|_inf <= 1e-10, whose residual is not finite, or whose backward solve has not met its tolerance at the cap, gets NaN in every output
// (a flag every thread sees); other tasks are untouched.
// LDS (bytes): 8 * (ns ns [G, St] + nq ns [K, dK] + 10 ns ways [A, trial A, P, U, R, and the CG's x, r, d, q, G-product] + nq ways [dP] +
//              2 ns + 3 nq [row tables] + 32 [reduction slots])
#include <cmath>
#include "mi_common.h"
#include "kernels.h"
#include "../../include/mi_maml.h"

namespace {
constexpr int kThreads = 512, kWaves = kThreads / 64, kRows = 8;
constexpr double kStop = 1e-13, kAccept = 1e-10, kCgTol2 = 1e-26, kArmijo = 1e-4;

struct Lds {
  double *g, *k, *a, *at, *p, *u, *r, *x, *cr, *cd, *w, *t, *dp, *sf, *sm, *rl, *rh, *ra, *red;
};
__device__ __forceinline__ Lds carve(double* sm, int ns, int nq, int ways) {
  const size_t tab = (size_t)ns * ways;
  Lds l;
  l.g = sm;
  l.k = l.g + (size_t)ns * ns;
  l.a = l.k + (size_t)nq * ns;
  l.at = l.a + tab;
  l.p = l.at + tab;
  l.u = l.p + tab;
  l.r = l.u + tab;
  l.x = l.r + tab;
  l.cr = l.x + tab;
  l.cd = l.cr + tab;
  l.w = l.cd + tab;
  l.t = l.w + tab;
  l.dp = l.t + tab;
  l.sf = l.dp + (size_t)nq * ways;
  l.sm = l.sf + ns;
  l.rl = l.sm + ns;
  l.rh = l.rl + nq;
  l.ra = l.rh + nq;
  l.red = l.ra + nq;
  return l;
}

// the maximum that keeps a NaN once it has seen one
__device__ __forceinline__ double nanmax(double m, double x) { return (x > m || x != x) ? x : m; }

struct Task {
  Lds l;
  int NS, WY, N, tid, lane, wave, flip;
  double lam;

  // (a, b) <- their sums over the workgroup, the same bits in every thread: lanes, then the eight waves in order.  Two slot sets in turn: a
  // thread still reading one set is at most one barrier behind the threads that write the other.
  __device__ __forceinline__ void block_sum2(double& a, double& b) {
    double* s = l.red + 16 * flip;
    flip ^= 1;
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) { s[wave] = a; s[kWaves + wave] = b; }
    __syncthreads();
    a = 0.0; b = 0.0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) { a += s[v]; b += s[kWaves + v]; }
  }
  // out <- G v (tables [ns][ways]); the caller has synchronised after writing v; returns synchronised
  __device__ __forceinline__ void gemv(const double* v, double* out) {
    for (int e = tid; e < N; e += kThreads) {
      const int i = e / WY, c = e - i * WY;
      double s = 0.0;
      for (int j = 0; j < NS; ++j) s = fma(l.g[i * NS + j], v[j * WY + c], s);
      out[e] = s;
    }
    __syncthreads();
  }
  // sum_c x_ic y_ic of the row of element e
  __device__ __forceinline__ double rowdot(const double* x, const double* y, int i) {
    double s = 0.0;
    for (int c = 0; c < WY; ++c) s = fma(x[i * WY + c], y[i * WY + c], s);
    return s;
  }
  // P, U, R, the row maxima of |R| and the rows of the inner objective at the table `a` whose G-product is in l.t; then (|R|_inf, objective) in
  // every thread.  A wave per support row, lane = class.  The caller has synchronised; returns synchronised.
  __device__ __forceinline__ void evaluate(const double* a, const int32_t* ys, double& rn, double& f) {
    for (int i = wave; i < NS; i += kWaves) {
      const bool act = lane < WY;
      const double s = act ? l.t[i * WY + lane] : -(double)INFINITY, av = act ? a[i * WY + lane] : 0.0;
      double mx = s;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = nanmax(mx, __shfl_xor(mx, off, 64));
      const double ex = act ? exp(s - mx) : 0.0;
      const double se = wave_sum(ex);
      const double p = ex / se;
      const int y = ys[i];
      const double r = act ? fma(lam, av, p - (lane == y ? 1.0 : 0.0)) : 0.0;
      double rm = fabs(r);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) rm = nanmax(rm, __shfl_xor(rm, off, 64));
      const double as = wave_sum(act ? av * s : 0.0);
      const double sy = __shfl(s, y & 63, 64);
      if (act) {
        l.p[i * WY + lane] = p;
        l.u[i * WY + lane] = sqrt(p);
        l.r[i * WY + lane] = r;
      }
      if (lane == 0) {
        l.sm[i] = rm;
        l.sf[i] = ((mx + log(se)) - sy) + 0.5 * lam * as;
      }
    }
    __syncthreads();
    rn = 0.0; f = 0.0;
    for (int i = 0; i < NS; ++i) { rn = nanmax(rn, l.sm[i]); f += l.sf[i]; }
    __syncthreads();                                     // (the row tables are free for the next evaluation)
  }
  // l.w <- sign * (lam I + D G)^-1 V at the P, U in LDS, V a table that is left as it was; returns whether the conjugate gradients met their
  // tolerance (the same in every thread).  The caller has synchronised after writing V; returns synchronised.
  __device__ __forceinline__ bool apply_inverse(const double* v, double sign, int& steps_out) {
    gemv(v, l.t);
    double bb = 0.0, zero = 0.0;
    for (int e = tid; e < N; e += kThreads) {             // b = C^T G V; x = 0, r = d = b
      const int i = e / WY;
      const double b = l.u[e] * (l.t[e] - rowdot(l.p, l.t, i));
      l.x[e] = 0.0; l.cr[e] = b; l.cd[e] = b;
      bb = fma(b, b, bb);
    }
    block_sum2(bb, zero);
    double rr = bb;
    int steps = 0;
    __syncthreads();
    while (steps < MI_LOGREG_CG_CAP && rr > kCgTol2 * bb) {        // (a NaN compares false: out at once)
      for (int e = tid; e < N; e += kThreads) {           // w = C d
        const int i = e / WY;
        l.w[e] = fma(l.u[e], l.cd[e], -(l.p[e] * rowdot(l.u, l.cd, i)));
      }
      __syncthreads();
      gemv(l.w, l.t);
      double dq = 0.0;
      for (int e = tid; e < N; e += kThreads) {           // q = lam d + C^T t, over w
        const int i = e / WY;
        const double q = fma(lam, l.cd[e], l.u[e] * (l.t[e] - rowdot(l.p, l.t, i)));
        l.w[e] = q;
        dq = fma(l.cd[e], q, dq);
      }
      block_sum2(dq, zero);
      const double al = rr / dq;
      double rn = 0.0;
      for (int e = tid; e < N; e += kThreads) {
        l.x[e] = fma(al, l.cd[e], l.x[e]);
        const double r = fma(-al, l.w[e], l.cr[e]);
        l.cr[e] = r;
        rn = fma(r, r, rn);
      }
      block_sum2(rn, zero);
      const double beta = rn / rr;
      for (int e = tid; e < N; e += kThreads) l.cd[e] = fma(beta, l.cd[e], l.cr[e]);
      rr = rn;
      ++steps;
      __syncthreads();
    }
    steps_out = steps;
    const double inv = sign / lam;
    for (int e = tid; e < N; e += kThreads) {             // (V - C x) / lam
      const int i = e / WY;
      l.w[e] = (v[e] - fma(l.u[e], l.x[e], -(l.p[e] * rowdot(l.u, l.x, i)))) * inv;
    }
    __syncthreads();
    return rr <= kCgTol2 * bb;
  }
};

template <bool BWD, int VW>
__device__ __forceinline__ void logreg_task(const LogregArgs& a, double* sm) {
  const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NS = a.ns, NQ = a.nq, F = a.feat, WY = a.ways;
  const double lam = (double)a.h.lam, alpha = (double)a.h.alpha;
  const float* fs = a.fs + (size_t)task * NS * F;
  const float* fq = a.fq + (size_t)task * NQ * F;
  const int32_t* ys = a.ys + (size_t)task * NS;
  const int32_t* yq = a.yq + (size_t)task * NQ;
  Task k{carve(sm, NS, NQ, WY), NS, WY, NS * WY, tid, lane, wave, 0, lam};
  const Lds& l = k.l;
  const int N = NS * WY;

  // ---- sweep 1: G (square) and K, a wave per 4 x 4 tile (G: the tiles of the lower triangle, mirrored at the store)
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
#pragma unroll 4
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
          if (i < NS && j <= i) { l.g[i * NS + j] = v; l.g[j * NS + i] = v; }
        } else if (i < NQ && j < NS) {
          l.k[i * NS + j] = v;
        }
      }
    }
  }
  for (int e = tid; e < N; e += kThreads) { l.a[e] = 0.0; l.t[e] = 0.0; }
  __syncthreads();

  // ---- the inner problem: Newton from A = 0 (whose G-product is 0)
  double rn, f;
  double *cur = l.a, *alt = l.at;
  k.evaluate(cur, ys, rn, f);
  for (int it = 0; it < MI_LOGREG_NEWTON_CAP && rn > kStop; ++it) {           // (a NaN compares false)
    int cg_steps;
    k.apply_inverse(l.r, -1.0, cg_steps);                // the step, in l.w
    k.gemv(l.w, l.t);
    double slope = 0.0, zero = 0.0;
    for (int e = tid; e < N; e += kThreads) slope = fma(l.r[e], l.t[e], slope);
    k.block_sum2(slope, zero);
    double step = 1.0;
    bool moved = false;
    for (int h = 0; h <= MI_LOGREG_HALVE_CAP; ++h) {
      for (int e = tid; e < N; e += kThreads) alt[e] = fma(step, l.w[e], cur[e]);
      __syncthreads();
      k.gemv(alt, l.t);
      double rnt, ft;
      k.evaluate(alt, ys, rnt, ft);
      if (!(isfinite(rnt) && isfinite(ft))) { rn = rnt + ft; break; }         // not finite: NaN, out of both loops
      if (rnt < rn || (rn > kAccept && ft <= f + kArmijo * step * slope)) {
        double* s = cur; cur = alt; alt = s;
        rn = rnt; f = ft; moved = true;
        break;
      }
      if (rn <= kAccept) break;
      step *= 0.5;
    }
    if (!moved) {
      if (isfinite(rn)) {                                // P, U, R of the point kept, not of the trial
        k.gemv(cur, l.t);
        double rn2, f2;
        k.evaluate(cur, ys, rn2, f2);
      }
      break;
    }
  }
  bool bad = !(rn <= kAccept);
  const double* A = cur;
  const float nanf_ = __builtin_nanf("");

  // ---- head: a wave per query row, lane w holds Pq_qw
  const double invn = 1.0 / (double)NQ;
  for (int q = wave; q < NQ; q += kWaves) {
    const bool act = lane < WY;
    double p = 0.0;
    if (act)
      for (int j = 0; j < NS; ++j) p = fma(l.k[q * NS + j], A[j * WY + lane], p);
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
      l.dp[q * WY + lane] = alpha * dl;
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

  // ---- dA = K^T dP (over the trial table), V = D dA (over R), X = (lam I + D G)^-1 V (into W), B = (dA - G X) / lam (over dA), dlam
  double* dA = alt;
  for (int e = tid; e < N; e += kThreads) {
    const int j = e / WY, w = e % WY;
    double s = 0.0;
    for (int q = 0; q < NQ; ++q) s = fma(l.k[q * NS + j], l.dp[q * WY + w], s);
    dA[e] = s;
  }
  __syncthreads();
  for (int e = tid; e < N; e += kThreads) {
    const int i = e / WY;
    l.r[e] = l.p[e] * (dA[e] - k.rowdot(l.p, dA, i));
  }
  __syncthreads();
  int cg_steps;
  bad |= !k.apply_inverse(l.r, 1.0, cg_steps);
  k.gemv(l.w, l.t);
  {
    const double inv = 1.0 / lam;
    double s = 0.0, zero = 0.0;
    for (int e = tid; e < N; e += kThreads) {
      const double b = (dA[e] - l.t[e]) * inv;
      dA[e] = b;
      s = fma(b, A[e], s);
    }
    k.block_sum2(s, zero);
    if (tid == 0 && a.dhyper) {
      a.dhyper[2 * (size_t)task] = bad ? nanf_ : (float)(-s);
      a.dhyper[2 * (size_t)task + 1] = bad ? nanf_ : (float)dalpha;
    }
  }
  if (!a.dfs && !a.dfq) return;

  // ---- St over G (the solver is done), dK over K (dA is done)
  __syncthreads();
  if (a.dfs) {
    for (int e = tid; e < NS * NS; e += kThreads) {
      const int i = e / NS, j = e % NS;
      double s = 0.0;
      for (int w = 0; w < WY; ++w) {
        s = fma(l.w[i * WY + w], A[j * WY + w], s);
        s = fma(A[i * WY + w], l.w[j * WY + w], s);
      }
      l.g[e] = -s;
    }
  }
  for (int e = tid; e < NQ * NS; e += kThreads) {
    const int q = e / NS, j = e % NS;
    double s = 0.0;
    for (int w = 0; w < WY; ++w) s = fma(l.dp[q * WY + w], A[j * WY + w], s);
    l.k[e] = s;
  }
  __syncthreads();

  // ---- sweep 2: dFq = dK Fs and dFs = dK^T Fq + St Fs, a thread per (8 rows, VW columns) block
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
          const double c = l.g[min(r0 + r, NS - 1) * NS + j];
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
__global__ __launch_bounds__(kThreads) void logreg_head_kernel(LogregArgs a) {
  extern __shared__ __attribute__((aligned(16))) double logreg_sm[];
  // 16-byte global accesses when every row starts on a 16-byte boundary (the entry points require 16-byte aligned bases)
  const bool vec = a.feat % 4 == 0;
  if (vec) logreg_task<BWD, 4>(a, logreg_sm);
  else logreg_task<BWD, 1>(a, logreg_sm);
}
}  // namespace

// Dynamic LDS of one task (the kernel has no static LDS, so a request may take all of a CU's 160 KiB); feat does not enter:
//   8 * (ns ns + nq ns + 10 ns ways + nq ways + 2 ns + 3 nq + 32) <= 163840, ways <= 64, feat <= MI_RIDGE_MAX_FEAT.
// ns = nq = 25, ways = 5: 22256; ns = nq = 20, ways = 20: 42656.
size_t logreg_head_lds_bytes(int ns, int nq, int ways) {
  const size_t s = (size_t)ns, q = (size_t)nq, w = (size_t)ways;
  return 8 * (s * s + q * s + 10 * s * w + q * w + 2 * s + 3 * q + 32);
}
bool logreg_head_fits(int ns, int nq, int feat, int ways) {
  return ns >= 1 && nq >= 1 && feat >= 1 && feat <= MI_RIDGE_MAX_FEAT && ways >= 1 && ways <= 64 &&
         logreg_head_lds_bytes(ns, nq, ways) <= head_lds_limit_bytes();
}

// A request above 64 KiB needs allow_dynamic_lds (mi_common.h), raised to the device's whole LDS: the ridge head's rule.
template <bool BWD>
static hipError_t logreg_launch(hipStream_t st, const LogregArgs& a, int tasks) {
  const size_t sm = logreg_head_lds_bytes(a.ns, a.nq, a.ways);
  if (sm > 64 * 1024) {
    static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(logreg_head_kernel<BWD>), head_lds_limit_bytes(), &attr_done); e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(logreg_head_kernel<BWD>, dim3(tasks), dim3(kThreads), sm, st, a);
  return hipGetLastError();
}

// Forward (a.dfs == a.dfq == a.dhyper == NULL) or forward + backward, one launch either way.  Outside the domain: hipErrorInvalidValue,
// nothing launched (callers check logreg_head_fits first and report MI_ERR_ARG).
hipError_t launch_logreg_head(hipStream_t st, const LogregArgs& a, int tasks) {
  if (tasks < 1 || !logreg_head_fits(a.ns, a.nq, a.feat, a.ways) || !(a.h.lam > 0.f) || !(a.h.alpha > 0.f) || !std::isfinite(a.h.lam) || !std::isfinite(a.h.alpha))
    return hipErrorInvalidValue;
  return (a.dfs || a.dfq || a.dhyper) ? logreg_launch<true>(st, a, tasks) : logreg_launch<false>(st, a, tasks);
}
