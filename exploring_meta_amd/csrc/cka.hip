// Centred kernel alignment of layer representations (reference utils/cka.py:9-60) without any n x n matrix.
//
// Input: `pairs` independent pairs (X_k, Y_k) of fp32 row-major [n, p] matrices (rows = points, p <= 128 features).
// Output per pair: {linear_cka, kernel_cka, sigma_x, sigma_y} in fp64.
//
//   Linear CKA: HSIC_lin(X, Y) = ||Xc^T Yc||_F^2 with Xc = X - column means: p x p cross products in fp64 (O(n p^2)).
//   Kernel CKA: D_ij = sum_k (x_ik - x_jk)^2 in fp32 (exactly 0 iff the rows are equal, never negative), K = exp(-D / (2 sigma^2)),
//     C = K - r_i/n - r_j/n + s/n^2 (r = row sums, s = their sum), HSIC = sum_ij Cx_ij Cy_ij in fp64.  The n^2 entries are
//     recomputed tile by tile from the [n, p] inputs in every pass; the median bandwidth (sigma^2 = median of the nonzero D_ij, i < j)
//     is an exact radix selection on the IEEE bits of D over three histogram rounds (11 + 11 + 10 bits) that follows both middle
//     ranks.  Every pass computes D through the one function tile_dist, so a round sees the same bits as the one before it.
//
// Passes per call: column sums -> cross products -> linear finish | histogram round + select (x3, or the given sigma) ->
// row sums -> centring vector -> centred products -> kernel finish.  Work on the kernel side is dominated by the distances
// (2 p vector instructions per entry); the symmetric passes (histograms, centred products) visit the tiles with j >= i only.
// Determinism: every fp64 sum has a fixed order (per-block partials in scratch, fixed-order final folds); the only atomics are
// integer adds to histogram bins.  Nothing depends on `pairs` except the grid's last dimension.
#include <math.h>
#include "mi_common.h"
#include "kernels.h"

namespace {

constexpr int TR = 64;             // rows (and columns) of a distance tile
constexpr int NT = 256;            // threads of the tile kernels: 16 x 16, 4 x 4 entries each
constexpr int BINS = 2048;         // histogram bins per round (11 bits; the last round uses 1024)
constexpr int STATE = 8;           // per matrix: M, rank[2], prefix[2]
constexpr int XROWS = 16;          // rows staged per step of the cross-product kernel
constexpr int XPER = 8;            // cross-product entries per thread
constexpr int MAX_PAIRS = 8192;    // pairs per launch sequence (grid dimension limit); larger calls are split

struct Geo {
  int n, p, T, S, C, E;
};

Geo geo(int n, int p) {
  Geo g;
  g.n = n;
  g.p = p;
  g.T = (n + TR - 1) / TR;
  g.S = g.T / 8 < 1 ? 1 : (g.T / 8 > 16 ? 16 : g.T / 8);      // column splits of the symmetric passes (a function of n only)
  const int c = (n + 2047) / 2048;
  g.C = c > 16 ? 16 : c;                                       // row chunks of the linear pass
  g.E = (3 * p * p + NT * XPER - 1) / (NT * XPER);             // entry groups of the cross products
  return g;
}

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t colpart, cross, hist, state, sig2, cvec, hpart, total;
};

Layout layout(int pairs, const Geo& g) {
  const size_t mats = 2 * (size_t)pairs;
  Layout L;
  size_t o = 0;
  L.colpart = o; o += al(mats * g.C * g.p * sizeof(double));
  L.cross = o;   o += al((size_t)pairs * g.C * 3 * g.p * g.p * sizeof(double));
  L.hist = o;    o += al(mats * 2 * BINS * sizeof(unsigned long long));
  L.state = o;   o += al(mats * STATE * sizeof(unsigned long long));
  L.sig2 = o;    o += al(mats * sizeof(double));
  L.cvec = o;    o += al(mats * g.n * sizeof(double));
  L.hpart = o;   o += al((size_t)pairs * g.T * g.S * 3 * sizeof(double));
  L.total = o;
  return L;
}

// fixed-order tree sum of v over the workgroup (blockDim.x a power of two, red >= blockDim.x doubles); result in red[0]
__device__ __forceinline__ void block_tree(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Linear CKA

// grid (C, mats): column sums of rows [c n / C, (c+1) n / C) -> colpart[mat][c][p]
__global__ __launch_bounds__(NT) void cka_colsum_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int C,
                                                        double* __restrict__ colpart) {
  __shared__ double red[NT];
  const int t = threadIdx.x, c = blockIdx.x, m = blockIdx.y;
  const float* src = ((m & 1) ? y : x) + (size_t)(m >> 1) * n * p;
  const int G = NT / p, g = t / p, k = t - g * p;
  const int r0 = (int)((long)c * n / C), r1 = (int)((long)(c + 1) * n / C);
  double s = 0.0;
  if (g < G)
    for (int r = r0 + g; r < r1; r += G) s += (double)src[(size_t)r * p + k];
  red[t] = s;
  __syncthreads();
  if (t < p) {
    double v = 0.0;
    for (int gg = 0; gg < G; ++gg) v += red[gg * p + t];
    colpart[((size_t)m * C + c) * p + t] = v;
  }
}

// grid (C, E, pairs): entries e = (q, k, l) of the three p x p cross products Xc^T Yc, Xc^T Xc, Yc^T Yc over one row chunk.
// Every workgroup folds the column means itself (C x p values, fixed order).
__global__ __launch_bounds__(NT) void cka_cross_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int C,
                                                       const double* __restrict__ colpart, double* __restrict__ cross) {
  extern __shared__ double xs[];          // [2][p] means, then [XROWS][2p] centred rows
  double* mean = xs;
  double* rows = xs + 2 * p;
  const int t = threadIdx.x, c = blockIdx.x, pair = blockIdx.z;
  const int pp = p * p, ne = 3 * pp;
  const float* xp = x + (size_t)pair * n * p;
  const float* yp = y + (size_t)pair * n * p;
  for (int e = t; e < 2 * p; e += NT) {
    const int w = e / p, k = e - w * p;
    const double* cp = colpart + ((size_t)(2 * pair + w) * C) * p + k;
    double s = 0.0;
    for (int cc = 0; cc < C; ++cc) s += cp[(size_t)cc * p];
    mean[e] = s / (double)n;
  }
  int aoff[XPER], boff[XPER];
  bool valid[XPER];
#pragma unroll
  for (int u = 0; u < XPER; ++u) {
    const int e = blockIdx.y * NT * XPER + t + NT * u;
    valid[u] = e < ne;
    const int q = valid[u] ? e / pp : 0, kl = valid[u] ? e - q * pp : 0;
    const int k = kl / p, l = kl - (kl / p) * p;
    aoff[u] = (q == 2 ? p : 0) + k;     // q 0: (X, Y), 1: (X, X), 2: (Y, Y)
    boff[u] = (q == 1 ? 0 : p) + l;
  }
  double acc[XPER];
#pragma unroll
  for (int u = 0; u < XPER; ++u) acc[u] = 0.0;
  const int r0 = (int)((long)c * n / C), r1 = (int)((long)(c + 1) * n / C);
  for (int rb = r0; rb < r1; rb += XROWS) {
    __syncthreads();
    for (int e = t; e < XROWS * 2 * p; e += NT) {
      const int rr = e / (2 * p), w2 = e - rr * 2 * p, w = w2 >= p, k = w2 - w * p;
      const int r = rb + rr;
      double v = 0.0;
      if (r < r1) v = (double)(w ? yp : xp)[(size_t)r * p + k] - mean[w * p + k];
      rows[e] = v;
    }
    __syncthreads();
    const int nr = r1 - rb < XROWS ? r1 - rb : XROWS;
    for (int rr = 0; rr < nr; ++rr) {
      const double* row = rows + rr * 2 * p;
#pragma unroll
      for (int u = 0; u < XPER; ++u) acc[u] = fma(row[aoff[u]], row[boff[u]], acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < XPER; ++u)
    if (valid[u]) cross[((size_t)pair * C + c) * ne + blockIdx.y * NT * XPER + t + NT * u] = acc[u];
}

// grid pairs: HSIC_lin of the three products (chunks folded in order, squared, summed in a fixed tree) -> out[pair][0]
__global__ __launch_bounds__(NT) void cka_linear_finish_kernel(const double* __restrict__ cross, int p, int C, double* __restrict__ out) {
  __shared__ double red[NT];
  __shared__ double h[3];
  const int t = threadIdx.x, pair = blockIdx.x, pp = p * p;
  const double* cp = cross + (size_t)pair * C * 3 * pp;
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int e = t; e < pp; e += NT) {
      double v = 0.0;
      for (int cc = 0; cc < C; ++cc) v += cp[(size_t)cc * 3 * pp + q * pp + e];
      s = fma(v, v, s);
    }
    block_tree(red, s);
    if (t == 0) h[q] = red[0];
    __syncthreads();
  }
  if (t == 0) out[(size_t)pair * 4 + 0] = h[0] / sqrt(h[1] * h[2]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Kernel CKA: the distance tiles

// rows [r0, r0 + TR) of an [n, p] matrix -> LDS [p][TR] (rows past n are zeros)
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int r0, int n, int p, float* __restrict__ lds) {
  const int lim = (n - r0 < TR ? n - r0 : TR) * p;
  const float* s = src + (size_t)r0 * p;
  for (int e = threadIdx.x; e < TR * p; e += NT) {
    const int r = e / p, k = e - r * p;
    lds[k * TR + r] = e < lim ? s[e] : 0.f;
  }
}

// D[a][b] = sum_k (A[k][4 ty + a] - B[k][4 tx + b])^2, k in order: the ONE definition of a distance every pass uses
__device__ __forceinline__ void tile_dist(const float* __restrict__ A, const float* __restrict__ B, int p, int ty, int tx, float d[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) d[a][b] = 0.f;
#pragma unroll 4
  for (int k = 0; k < p; ++k) {
    const floatx4 av = *reinterpret_cast<const floatx4*>(A + k * TR + 4 * ty);
    const floatx4 bv = *reinterpret_cast<const floatx4*>(B + k * TR + 4 * tx);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float df = av[a] - bv[b];
        d[a][b] = fmaf(df, df, d[a][b]);
      }
  }
}

// K = exp(-D / (2 sigma^2)) = exp2(D * kc), kc = -log2(e) / (2 sigma^2)
__device__ __forceinline__ float kernel_scale(double sig2) { return (float)(-1.4426950408889634 * 0.5 / sig2); }
__device__ __forceinline__ float kval(float d, float kc) { return __builtin_amdgcn_exp2f(d * kc); }

// column tiles [j0, j1) of a workgroup of a symmetric pass: split s of S, restricted to j >= ti
__device__ __forceinline__ void sym_range(int T, int S, int s, int ti, int& j0, int& j1) {
  j0 = (int)((long)s * T / S);
  j1 = (int)((long)(s + 1) * T / S);
  if (j0 < ti) j0 = ti;
}

// Histogram round R (1, 2, 3) over the nonzero D_ij, i < j.  grid (T, S, mats).
//   R = 1: bin = bits >> 21 (one table);  R = 2: table t counts bins (bits >> 10) & 2047 of the entries whose bits >> 21 equal
//   prefix[t];  R = 3: table t counts bits & 1023 of the entries whose bits >> 10 equal prefix[t].
template <int R>
__global__ __launch_bounds__(NT) void cka_hist_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int S,
                                                      const unsigned long long* __restrict__ state, unsigned long long* __restrict__ ghist) {
  extern __shared__ float lds[];
  float* A = lds;
  float* B = lds + TR * p;
  unsigned* h = reinterpret_cast<unsigned*>(lds + 2 * TR * p);     // [2][BINS]
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int ti = blockIdx.x, m = blockIdx.z, T = gridDim.x;
  const unsigned long long* st = state + (size_t)m * STATE;
  if (R > 1 && st[0] == 0) return;                                   // no nonzero distance: sigma is NaN
  unsigned pf0 = 0, pf1 = 0;
  if (R > 1) { pf0 = (unsigned)st[3]; pf1 = (unsigned)st[4]; }
  for (int e = t; e < 2 * BINS; e += NT) h[e] = 0u;
  const float* src = ((m & 1) ? y : x) + (size_t)(m >> 1) * n * p;
  int j0, j1;
  sym_range(T, S, blockIdx.y, ti, j0, j1);
  load_tile(src, ti * TR, n, p, A);
  for (int tj = j0; tj < j1; ++tj) {
    __syncthreads();
    load_tile(src, tj * TR, n, p, B);
    __syncthreads();
    float d[4][4];
    tile_dist(A, B, p, ty, tx, d);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = ti * TR + 4 * ty + a, j = tj * TR + 4 * tx + b;
        const unsigned u = __float_as_uint(d[a][b]);
        if (j >= n || j <= i || u == 0u) continue;
        if (R == 1) {
          atomicAdd(&h[u >> 21], 1u);
        } else if (R == 2) {
          if ((u >> 21) == pf0) atomicAdd(&h[(u >> 10) & 2047u], 1u);
          if ((u >> 21) == pf1) atomicAdd(&h[BINS + ((u >> 10) & 2047u)], 1u);
        } else {
          if ((u >> 10) == pf0) atomicAdd(&h[u & 1023u], 1u);
          if ((u >> 10) == pf1) atomicAdd(&h[BINS + (u & 1023u)], 1u);
        }
      }
  }
  __syncthreads();
  unsigned long long* gh = ghist + (size_t)m * 2 * BINS;
  for (int e = t; e < (R == 1 ? BINS : 2 * BINS); e += NT)
    if (h[e]) atomicAdd(&gh[e], (unsigned long long)h[e]);
}

// grid mats: after round R, find the bins of the two middle ranks and clear the histogram for the next round.  After round 3 the
// selected values are D bit patterns: sigma^2 = their mean (numpy's median of an even count), sigma -> out[pair][2 + (mat & 1)].
__global__ __launch_bounds__(NT) void cka_select_kernel(int R, unsigned long long* __restrict__ ghist, unsigned long long* __restrict__ state,
                                                        double* __restrict__ sig2, double* __restrict__ out) {
  __shared__ unsigned long long h[2 * BINS];
  __shared__ unsigned long long part[NT];
  const int t = threadIdx.x, m = blockIdx.x;
  unsigned long long* st = state + (size_t)m * STATE;
  unsigned long long* gh = ghist + (size_t)m * 2 * BINS;
  if (R > 1 && st[0] == 0) return;
  for (int e = t; e < 2 * BINS; e += NT) {
    h[e] = gh[e];
    gh[e] = 0ull;
  }
  __syncthreads();
  if (R == 1) {
    unsigned long long s = 0;
    for (int b = 0; b < BINS / NT; ++b) s += h[t * (BINS / NT) + b];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
      unsigned long long M = 0;
      for (int q = 0; q < NT; ++q) M += part[q];
      st[0] = M;
      st[1] = M ? (M - 1) / 2 : 0;
      st[2] = M / 2;
      st[3] = st[4] = 0;
      if (M == 0) {
        sig2[m] = __builtin_nan("");
        out[(size_t)(m >> 1) * 4 + 2 + (m & 1)] = __builtin_nan("");
      }
    }
    __syncthreads();
  }
  for (int tt = 0; tt < 2; ++tt) {
    const unsigned long long* ht = h + (R == 1 ? 0 : tt * BINS);
    unsigned long long s = 0;
    for (int b = 0; b < BINS / NT; ++b) s += ht[t * (BINS / NT) + b];
    part[t] = s;
    __syncthreads();
    if (t == 0 && st[0] != 0) {
      unsigned long long k = st[1 + tt], cum = 0;
      int q = 0;
      while (q < NT - 1 && cum + part[q] <= k) cum += part[q++];
      int b = q * (BINS / NT);
      while (b < BINS - 1 && cum + ht[b] <= k) cum += ht[b++];
      st[1 + tt] = k - cum;
      const unsigned pf = (unsigned)st[3 + tt];
      st[3 + tt] = R == 1 ? (unsigned)b : (R == 2 ? (pf << 11) | (unsigned)b : (pf << 10) | (unsigned)b);
    }
    __syncthreads();
  }
  if (R == 3 && t == 0) {
    const double v = 0.5 * ((double)__uint_as_float((unsigned)st[3]) + (double)__uint_as_float((unsigned)st[4]));
    sig2[m] = v;
    out[(size_t)(m >> 1) * 4 + 2 + (m & 1)] = sqrt(v);
  }
}

// a given bandwidth for every matrix (the reference passes one sigma to both rbf calls)
__global__ void cka_fixed_sigma_kernel(int mats, double sigma, double* __restrict__ sig2, double* __restrict__ out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= mats) return;
  sig2[m] = sigma * sigma;
  out[(size_t)(m >> 1) * 4 + 2 + (m & 1)] = sigma;
}

// grid (T, 1, mats): r_i = sum_j K_ij over the full row (fp64, j in order per thread, the 16 column threads folded in order)
__global__ __launch_bounds__(NT) void cka_rowsum_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p,
                                                        const double* __restrict__ sig2, double* __restrict__ rvec) {
  extern __shared__ float lds[];
  float* A = lds;
  float* B = lds + TR * p;
  double* red = reinterpret_cast<double*>(lds + 2 * TR * p);        // [TR][16]
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int ti = blockIdx.x, m = blockIdx.z, T = gridDim.x;
  const float* src = ((m & 1) ? y : x) + (size_t)(m >> 1) * n * p;
  const float kc = kernel_scale(sig2[m]);
  double rs[4] = {0.0, 0.0, 0.0, 0.0};
  load_tile(src, ti * TR, n, p, A);
  for (int tj = 0; tj < T; ++tj) {
    __syncthreads();
    load_tile(src, tj * TR, n, p, B);
    __syncthreads();
    float d[4][4];
    tile_dist(A, B, p, ty, tx, d);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (tj * TR + 4 * tx + b >= n) continue;
#pragma unroll
      for (int a = 0; a < 4; ++a) rs[a] += (double)kval(d[a][b], kc);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) red[(4 * ty + a) * 16 + tx] = rs[a];
  __syncthreads();
  if (t < TR && ti * TR + t < n) {
    double s = 0.0;
    for (int q = 0; q < 16; ++q) s += red[t * 16 + q];
    rvec[(size_t)m * n + ti * TR + t] = s;
  }
}

// grid mats: s = sum_i r_i (fixed tree), then c_i = r_i / n - s / (2 n^2) in place, so that C_ij = K_ij - c_i - c_j
__global__ __launch_bounds__(NT) void cka_center_kernel(int n, double* __restrict__ rvec) {
  __shared__ double red[NT];
  const int t = threadIdx.x;
  double* r = rvec + (size_t)blockIdx.x * n;
  double s = 0.0;
  for (int i = t; i < n; i += NT) s += r[i];
  block_tree(red, s);
  const double half = red[0] / (2.0 * (double)n * (double)n), inv_n = 1.0 / (double)n;
  for (int i = t; i < n; i += NT) r[i] = r[i] * inv_n - half;
}

// grid (T, S, pairs): sum over the tiles j >= i of w Cx Cy, w Cx^2, w Cy^2 (w = 1 on diagonal tiles, whose both halves are visited,
// 2 elsewhere) -> hpart[pair][ti S + s][3]
__global__ __launch_bounds__(NT) void cka_hsic_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int S,
                                                      const double* __restrict__ sig2, const double* __restrict__ cvec,
                                                      double* __restrict__ hpart) {
  extern __shared__ float lds[];
  float* Ax = lds;
  float* Ay = lds + TR * p;
  float* B = lds + 2 * TR * p;
  double* red = reinterpret_cast<double*>(lds + 3 * TR * p);         // [NT]
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int ti = blockIdx.x, pair = blockIdx.z, T = gridDim.x;
  const float* xp = x + (size_t)pair * n * p;
  const float* yp = y + (size_t)pair * n * p;
  const float kx = kernel_scale(sig2[2 * pair]), ky = kernel_scale(sig2[2 * pair + 1]);
  const double* cx = cvec + (size_t)(2 * pair) * n;
  const double* cy = cvec + (size_t)(2 * pair + 1) * n;
  double cxi[4], cyi[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti * TR + 4 * ty + a;
    cxi[a] = i < n ? cx[i] : 0.0;
    cyi[a] = i < n ? cy[i] : 0.0;
  }
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  int j0, j1;
  sym_range(T, S, blockIdx.y, ti, j0, j1);
  load_tile(xp, ti * TR, n, p, Ax);
  load_tile(yp, ti * TR, n, p, Ay);
  for (int tj = j0; tj < j1; ++tj) {
    float dx[4][4], dy[4][4];
    __syncthreads();
    load_tile(xp, tj * TR, n, p, B);
    __syncthreads();
    tile_dist(Ax, B, p, ty, tx, dx);
    __syncthreads();
    load_tile(yp, tj * TR, n, p, B);
    __syncthreads();
    tile_dist(Ay, B, p, ty, tx, dy);
    double txy = 0.0, txx = 0.0, tyy = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tj * TR + 4 * tx + b;
      if (j >= n) continue;
      const double cxj = cx[j], cyj = cy[j];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (ti * TR + 4 * ty + a >= n) continue;
        const double vx = ((double)kval(dx[a][b], kx) - cxi[a]) - cxj;
        const double vy = ((double)kval(dy[a][b], ky) - cyi[a]) - cyj;
        txy = fma(vx, vy, txy);
        txx = fma(vx, vx, txx);
        tyy = fma(vy, vy, tyy);
      }
    }
    const double w = tj == ti ? 1.0 : 2.0;
    sxy = fma(w, txy, sxy);
    sxx = fma(w, txx, sxx);
    syy = fma(w, tyy, syy);
  }
  double* hp = hpart + ((size_t)pair * T * S + (size_t)ti * S + blockIdx.y) * 3;
  __syncthreads();
  block_tree(red, sxy);
  if (t == 0) hp[0] = red[0];
  __syncthreads();
  block_tree(red, sxx);
  if (t == 0) hp[1] = red[0];
  __syncthreads();
  block_tree(red, syy);
  if (t == 0) hp[2] = red[0];
}

// grid pairs: fold the T S partials of each sum (fixed tree) -> out[pair][1] = HSIC(X, Y) / sqrt(HSIC(X, X) HSIC(Y, Y))
__global__ __launch_bounds__(NT) void cka_kernel_finish_kernel(const double* __restrict__ hpart, int nb, double* __restrict__ out) {
  __shared__ double red[NT];
  __shared__ double h[3];
  const int t = threadIdx.x, pair = blockIdx.x;
  const double* hp = hpart + (size_t)pair * nb * 3;
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int b = t; b < nb; b += NT) s += hp[(size_t)b * 3 + q];
    block_tree(red, s);
    if (t == 0) h[q] = red[0];
    __syncthreads();
  }
  if (t == 0) out[(size_t)pair * 4 + 1] = h[0] / sqrt(h[1] * h[2]);
}

template <typename K>
hipError_t allow_lds(K* k, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

#define CKA_LAUNCH(...)                                   \
  do {                                                    \
    hipLaunchKernelGGL(__VA_ARGS__);                      \
    if (hipError_t _e = hipGetLastError(); _e != hipSuccess) return _e; \
  } while (0)

hipError_t cka_chunk(hipStream_t st, const float* x, const float* y, int pairs, int n, int p, double sigma, char* ws, double* out) {
  const Geo g = geo(n, p);
  const Layout L = layout(pairs, g);
  const int mats = 2 * pairs;
  double* colpart = reinterpret_cast<double*>(ws + L.colpart);
  double* cross = reinterpret_cast<double*>(ws + L.cross);
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(ws + L.hist);
  unsigned long long* state = reinterpret_cast<unsigned long long*>(ws + L.state);
  double* sig2 = reinterpret_cast<double*>(ws + L.sig2);
  double* cvec = reinterpret_cast<double*>(ws + L.cvec);
  double* hpart = reinterpret_cast<double*>(ws + L.hpart);

  // linear CKA
  CKA_LAUNCH(cka_colsum_kernel, dim3(g.C, mats), dim3(NT), 0, st, x, y, n, p, g.C, colpart);
  CKA_LAUNCH(cka_cross_kernel, dim3(g.C, g.E, pairs), dim3(NT), (size_t)(2 * p + XROWS * 2 * p) * sizeof(double), st, x, y, n, p, g.C,
             colpart, cross);
  CKA_LAUNCH(cka_linear_finish_kernel, dim3(pairs), dim3(NT), 0, st, cross, p, g.C, out);

  // bandwidths
  const size_t tile_bytes = (size_t)TR * p * sizeof(float);
  if (sigma > 0.0) {
    CKA_LAUNCH(cka_fixed_sigma_kernel, dim3((mats + 255) / 256), dim3(256), 0, st, mats, sigma, sig2, out);
  } else {
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)mats * 2 * BINS * sizeof(unsigned long long), st); e != hipSuccess) return e;
    const size_t lds = 2 * tile_bytes + 2 * BINS * sizeof(unsigned);
    const dim3 grid(g.T, g.S, mats);
    if (hipError_t e = allow_lds(cka_hist_kernel<1>, lds); e != hipSuccess) return e;
    if (hipError_t e = allow_lds(cka_hist_kernel<2>, lds); e != hipSuccess) return e;
    if (hipError_t e = allow_lds(cka_hist_kernel<3>, lds); e != hipSuccess) return e;
    CKA_LAUNCH(cka_hist_kernel<1>, grid, dim3(NT), lds, st, x, y, n, p, g.S, state, hist);
    CKA_LAUNCH(cka_select_kernel, dim3(mats), dim3(NT), 0, st, 1, hist, state, sig2, out);
    CKA_LAUNCH(cka_hist_kernel<2>, grid, dim3(NT), lds, st, x, y, n, p, g.S, state, hist);
    CKA_LAUNCH(cka_select_kernel, dim3(mats), dim3(NT), 0, st, 2, hist, state, sig2, out);
    CKA_LAUNCH(cka_hist_kernel<3>, grid, dim3(NT), lds, st, x, y, n, p, g.S, state, hist);
    CKA_LAUNCH(cka_select_kernel, dim3(mats), dim3(NT), 0, st, 3, hist, state, sig2, out);
  }

  // centring and the centred products
  const size_t lds_r = 2 * tile_bytes + TR * 16 * sizeof(double);
  if (hipError_t e = allow_lds(cka_rowsum_kernel, lds_r); e != hipSuccess) return e;
  CKA_LAUNCH(cka_rowsum_kernel, dim3(g.T, 1, mats), dim3(NT), lds_r, st, x, y, n, p, sig2, cvec);
  CKA_LAUNCH(cka_center_kernel, dim3(mats), dim3(NT), 0, st, n, cvec);
  const size_t lds_h = 3 * tile_bytes + NT * sizeof(double);
  if (hipError_t e = allow_lds(cka_hsic_kernel, lds_h); e != hipSuccess) return e;
  CKA_LAUNCH(cka_hsic_kernel, dim3(g.T, g.S, pairs), dim3(NT), lds_h, st, x, y, n, p, g.S, sig2, cvec, hpart);
  CKA_LAUNCH(cka_kernel_finish_kernel, dim3(pairs), dim3(NT), 0, st, hpart, g.T * g.S, out);
  return hipSuccess;
}

}  // namespace

size_t cka_scratch_bytes(int pairs, int n, int p) {
  return layout(pairs < MAX_PAIRS ? pairs : MAX_PAIRS, geo(n, p)).total;
}

hipError_t launch_cka(hipStream_t st, const float* x, const float* y, int pairs, int n, int p, double sigma, void* scratch, double* out) {
  for (int k0 = 0; k0 < pairs; k0 += MAX_PAIRS) {
    const int k = pairs - k0 < MAX_PAIRS ? pairs - k0 : MAX_PAIRS;
    const size_t off = (size_t)k0 * n * p;
    if (hipError_t e = cka_chunk(st, x + off, y + off, k, n, p, sigma, static_cast<char*>(scratch), out + (size_t)k0 * 4); e != hipSuccess)
      return e;
  }
  return hipSuccess;
}
