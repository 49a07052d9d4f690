// Canonical correlation analysis of layer representations: the SVCCA measure the reference's representation-change study runs
// (reference utils/cca.py:226-362 with compute_ccas :104-174, remove_small :69-101, sum_threshold :177-195).
//
// Input: `pairs` independent pairs (X_k, Y_k) of fp32 row-major [n, p] matrices (rows = datapoints, p <= 64 neurons).
// Output per pair: the canonical correlations (descending, NaN after `count`) and
// {mean, thresholded_mean, sum, count, kept_x, kept_y, cond_x, cond_y}, all fp64.
//
// Passes per call (three launches, whatever `pairs` is):
//   cca_colsum_kernel  column sums per row chunk                                            (X, Y read once)
//   cca_cross_kernel   the centred cross products Xc^T Xc, Xc^T Yc, Yc^T Yc per row chunk   (X, Y read once more)
//   cca_solve_kernel   one workgroup per pair, everything else, matrices resident in LDS:
//     fold the chunk partials in chunk order; Sxx / max|Sxx|, Syy / max|Syy|, Sxy / sqrt(max|Sxx| max|Syy|) (the 1/(n-1) of the
//     covariance cancels here); keep neuron i iff |Sxx_ii| >= epsilon (kept neurons are compacted, which equals cropping); add
//     epsilon to the diagonals; eigen-decompose both blocks by parallel cyclic Jacobi; inverse square roots by the PSEUDO-INVERSE
//     RULE: an eigenvalue with |w_i| <= 1e-15 max|w| contributes 0, every other one |w_i|^(-1/2); M = Sxx^(-1/2) Sxy Syy^(-1/2);
//     singular values of M by one-sided (Hestenes) Jacobi on its columns; rank sort; statistics.
//
// LDS of the solver: four [p][LD] fp64 buffers, LD = p | 1 (odd, so that a column walk of 8-byte words touches every bank pair
// once): A (Sxx, later T = Sxx^(-1/2) Sxy), V (eigenvectors), R (fold target, then the inverse square root), S (Sxy, later Syy,
// later M), and about 10 KB of vectors: 4 p LD 8 + 10.3 KB, 140 KB at p = 64, 30 KB at p = 25.
//
// Ordering of both Jacobi loops: round-robin (circle method) over m = p rounded up to even players, m - 1 steps per sweep, the m / 2
// disjoint pairs of a step rotated concurrently; a pair with the padding player of an odd p is idle.
// Determinism: every sum has a fixed order, there are no atomics, and a pair's result depends on nothing but its own data.
#include <math.h>
#include "mi_common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;            // threads of every kernel here
constexpr int XROWS = 16;          // rows staged per step of the cross-product kernel
constexpr int XPER = 8;            // cross-product entries per thread
constexpr int MAXP = 64;
constexpr int HALF = MAXP / 2;     // concurrent rotations of a step
constexpr int LANES = NT / HALF;   // threads that share the dot products of one column pair
constexpr int SYM_CAP = 40;        // sweep caps (seen: DESIGN.md section 12)
constexpr int SVD_CAP = 60;
constexpr int MASK_WORDS = 2;      // per pair: kept masks of X and Y (bit i = neuron i), 64-bit words
constexpr int INFO_INTS = 4;       // per pair: sweeps of the X and Y eigen-problems and of the SVD, 1 if a cap was hit

struct Geo {
  int C, E;
};

Geo geo(int n, int p) {
  Geo g;
  const int c = (n + 1023) / 1024;
  g.C = c > 64 ? 64 : c;                                         // row chunks (a function of n only)
  g.E = (3 * p * p + NT * XPER - 1) / (NT * XPER);               // entry groups of the cross products
  return g;
}

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t mask, info, colpart, cross, total;
};

Layout layout(int pairs, int p, const Geo& g) {
  Layout L;
  size_t o = 0;
  L.mask = o;    o += al((size_t)pairs * MASK_WORDS * sizeof(unsigned long long));
  L.info = o;    o += al((size_t)pairs * INFO_INTS * sizeof(int));
  L.colpart = o; o += al((size_t)pairs * 2 * g.C * p * sizeof(double));
  L.cross = o;   o += al((size_t)pairs * g.C * 3 * p * p * sizeof(double));
  L.total = o;
  return L;
}

// grid (mats * C): column sums of rows [c n / C, (c+1) n / C) -> colpart[mat][c][p]
__global__ __launch_bounds__(NT) void cca_colsum_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int C,
                                                        double* __restrict__ colpart) {
  __shared__ double red[NT];
  const int t = threadIdx.x, c = blockIdx.x % C;
  const size_t m = blockIdx.x / C;
  const float* src = ((m & 1) ? y : x) + (m >> 1) * (size_t)n * p;
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
    colpart[(m * C + c) * p + t] = v;
  }
}

// grid (pairs * C, E): entries e = (q, k, l) of Xc^T Xc (q 0), Xc^T Yc (1), Yc^T Yc (2) over one row chunk -> cross[pair][c][3 p p].
// Every workgroup folds the column means itself (C x p values, chunk order).
__global__ __launch_bounds__(NT) void cca_cross_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int p, int C,
                                                       const double* __restrict__ colpart, double* __restrict__ cross) {
  extern __shared__ double xs[];          // [2][p] means, then [XROWS][2p] centred rows
  double* mean = xs;
  double* rows = xs + 2 * p;
  const int t = threadIdx.x, c = blockIdx.x % C;
  const size_t pair = blockIdx.x / C;
  const int pp = p * p, ne = 3 * pp;
  const float* xp = x + pair * (size_t)n * p;
  const float* yp = y + pair * (size_t)n * p;
  for (int e = t; e < 2 * p; e += NT) {
    const int w = e / p, k = e - w * p;
    const double* cp = colpart + ((2 * pair + w) * C) * p + k;
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
    const int k = kl / p, l = kl - k * p;
    aoff[u] = (q == 2 ? p : 0) + k;
    boff[u] = (q == 0 ? 0 : p) + l;
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
    if (valid[u]) cross[(pair * C + c) * ne + blockIdx.y * NT * XPER + t + NT * u] = acc[u];
}

// ---------------------------------------------------------------------------------------------------------------------
// The solver's pieces.  Every function is called by the whole workgroup; values that steer a loop come out of LDS after a
// barrier, so every thread sees the same one.

struct Sm {
  double *A, *V, *R, *S;                 // [p][LD]
  double *red;                           // [NT]
  double *cs, *sn;                       // [HALF] rotation of each pair of the step
  double *w, *f;                         // [MAXP] eigenvalues / singular values, their inverse square roots / the sorted values
  double *part;                          // [HALF][LANES][3] partial dot products
  double *misc;                          // [8]
  int *ix, *iy;                          // [MAXP] kept neurons
  int *cnt;                              // [4] kept_x, kept_y
};

__device__ __forceinline__ double block_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = NT >> 1; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double block_max(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = NT >> 1; s > 0; s >>= 1) {
    if (t < s) red[t] = fmax(red[t], red[t + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// pair q of step s of the round-robin over m (even) players; i < j
__device__ __forceinline__ void rr_pair(int m, int s, int q, int& i, int& j) {
  int a, b;
  if (q == 0) {
    a = m - 1;
    b = s;
  } else {
    a = (s + q) % (m - 1);
    b = (s - q + (m - 1)) % (m - 1);
  }
  i = a < b ? a : b;
  j = a < b ? b : a;
}

// t = tan of the rotation angle from z = cot of twice the angle (the smaller root, stable for every z), then c, s
__device__ __forceinline__ void rotation(double z, double& c, double& s) {
  const double t = (z < 0.0 ? -1.0 : 1.0) / (fabs(z) + sqrt(1.0 + z * z));
  c = 1.0 / sqrt(1.0 + t * t);
  s = t * c;
}

// dst[p][LD] = the p x p block q of the cross products, chunk partials folded in chunk order
__device__ void fold_block(const double* __restrict__ cp, int q, int p, int C, int LD, double* dst) {
  const int pp = p * p;
  for (int e = threadIdx.x; e < pp; e += NT) {
    double v = 0.0;
    for (int cc = 0; cc < C; ++cc) v += cp[(size_t)cc * 3 * pp + q * pp + e];
    dst[(e / p) * LD + (e % p)] = v;
  }
  __syncthreads();
}

__device__ double block_absmax(const double* M, int p, int LD, double* red) {
  double v = 0.0;
  for (int e = threadIdx.x; e < p * p; e += NT) v = fmax(v, fabs(M[(e / p) * LD + (e % p)]));
  return block_max(red, v);
}

// kept[] = neurons with |M_ii / mx| >= eps in index order (a NaN ratio keeps nothing); returns how many, the same in every thread
__device__ int keep_neurons(const double* M, int p, int LD, double mx, double eps, int* kept, int* cnt, unsigned long long* mask) {
  if (threadIdx.x == 0) {
    int k = 0;
    unsigned long long bits = 0ull;
    for (int i = 0; i < p; ++i)
      if (fabs(M[i * LD + i] / mx) >= eps) {
        kept[k++] = i;
        bits |= 1ull << i;
      }
    *cnt = k;
    *mask = bits;
  }
  __syncthreads();
  return *cnt;
}

// Symmetric eigen-decomposition of A[k][k] by parallel cyclic Jacobi: A -> diagonal (eigenvalues), V -> eigenvectors (columns).
// Stops when the off-diagonal norm is at most 1e-16 of the Frobenius norm, or at the sweep cap.  Returns the sweeps made.
__device__ int jacobi_sym(double* A, double* V, int k, int LD, const Sm& sm) {
  const int t = threadIdx.x, m = (k + 1) & ~1, half = m >> 1;
  for (int e = t; e < k * k; e += NT) V[(e / k) * LD + (e % k)] = (e / k == e % k) ? 1.0 : 0.0;
  __syncthreads();
  int sweeps = 0;
  for (;;) {
    double off = 0.0, fro = 0.0;
    for (int e = t; e < k * k; e += NT) {
      const int a = e / k, b = e - a * k;
      const double v = A[a * LD + b];
      fro = fma(v, v, fro);
      if (a != b) off = fma(v, v, off);
    }
    off = block_sum(sm.red, off);
    fro = block_sum(sm.red, fro);
    if (!(off > 1e-32 * fro) || sweeps >= SYM_CAP) break;
    for (int s = 0; s < m - 1; ++s) {
      if (t < half) {
        int i, j;
        rr_pair(m, s, t, i, j);
        double c = 1.0, sn = 0.0;
        if (j < k) {
          const double aij = A[i * LD + j];
          if (aij != 0.0) rotation((A[j * LD + j] - A[i * LD + i]) / (2.0 * aij), c, sn);
        }
        sm.cs[t] = c;
        sm.sn[t] = sn;
      }
      __syncthreads();
      for (int e = t; e < half * k; e += NT) {           // rows i, j of J^T A
        const int q = e / k, col = e - q * k;
        const double c = sm.cs[q], sn = sm.sn[q];
        if (sn == 0.0) continue;
        int i, j;
        rr_pair(m, s, q, i, j);
        const double u = A[i * LD + col], v = A[j * LD + col];
        A[i * LD + col] = c * u - sn * v;
        A[j * LD + col] = sn * u + c * v;
      }
      __syncthreads();
      for (int e = t; e < half * k; e += NT) {           // columns i, j of (J^T A) J and of V J
        const int q = e / k, row = e - q * k;
        const double c = sm.cs[q], sn = sm.sn[q];
        if (sn == 0.0) continue;
        int i, j;
        rr_pair(m, s, q, i, j);
        double u = A[row * LD + i], v = A[row * LD + j];
        A[row * LD + i] = c * u - sn * v;
        A[row * LD + j] = sn * u + c * v;
        u = V[row * LD + i];
        v = V[row * LD + j];
        V[row * LD + i] = c * u - sn * v;
        V[row * LD + j] = sn * u + c * v;
      }
      __syncthreads();
      if (t < half && sm.sn[t] != 0.0) {                 // the entry the rotation annihilates
        int i, j;
        rr_pair(m, s, t, i, j);
        A[i * LD + j] = 0.0;
        A[j * LD + i] = 0.0;
      }
      __syncthreads();
    }
    ++sweeps;
  }
  return sweeps;
}

// R = V diag(f) V^T with f from the eigenvalues on A's diagonal by the pseudo-inverse rule; returns cond = max|w| / min|w|
// (inf if the smallest eigenvalue is cut).
__device__ double inv_sqrt(const double* A, const double* V, double* R, int k, int LD, const Sm& sm) {
  const int t = threadIdx.x;
  if (t == 0) {
    double wmax = 0.0, wmin = INFINITY;
    for (int i = 0; i < k; ++i) {
      const double a = fabs(A[i * LD + i]);
      sm.w[i] = a;
      wmax = fmax(wmax, a);
      wmin = fmin(wmin, a);
    }
    const double cut = 1e-15 * wmax;
    for (int i = 0; i < k; ++i) sm.f[i] = sm.w[i] <= cut ? 0.0 : 1.0 / sqrt(sm.w[i]);
    sm.misc[0] = wmin <= cut ? INFINITY : wmax / wmin;
  }
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {
    const int a = e / k, b = e - a * k;
    double s = 0.0;
    for (int i = 0; i < k; ++i) s = fma(V[a * LD + i] * sm.f[i], V[b * LD + i], s);
    R[a * LD + b] = s;
  }
  __syncthreads();
  return sm.misc[0];
}

// D[r][c] = L[r][:] . Rt[:][c]  (r x inner x c), all [.][LD]
__device__ void matmul(const double* L, const double* Rt, double* D, int r, int inner, int c, int LD) {
  for (int e = threadIdx.x; e < r * c; e += NT) {
    const int a = e / c, b = e - a * c;
    double s = 0.0;
    for (int i = 0; i < inner; ++i) s = fma(L[a * LD + i], Rt[i * LD + b], s);
    D[a * LD + b] = s;
  }
  __syncthreads();
}

// One-sided (Hestenes) Jacobi on the columns of M[rows][cols]: columns are rotated in pairs until every pair is orthogonal to
// |m_i . m_j| <= tol |m_i| |m_j| with tol = sqrt(rows) 2^-53 (a sweep that rotates nothing ends the loop).  The singular values are
// the column norms, left in sm.w[0 .. cols).  Returns the sweeps made, the last, idle one included.
__device__ int jacobi_svd(double* M, int rows, int cols, int LD, const Sm& sm) {
  const int t = threadIdx.x, m = (cols + 1) & ~1, half = m >> 1;
  const double tol = sqrt((double)rows) * 1.1102230246251565e-16;
  const int q = t / LANES, g = t - q * LANES;
  int sweeps = 0;
  for (;;) {
    double worst = 0.0;
    for (int s = 0; s < m - 1; ++s) {
      if (q < half) {
        int i, j;
        rr_pair(m, s, q, i, j);
        double aa = 0.0, bb = 0.0, ab = 0.0;
        if (j < cols)
          for (int r = g; r < rows; r += LANES) {
            const double u = M[r * LD + i], v = M[r * LD + j];
            aa = fma(u, u, aa);
            bb = fma(v, v, bb);
            ab = fma(u, v, ab);
          }
        double* pt = sm.part + (q * LANES + g) * 3;
        pt[0] = aa;
        pt[1] = bb;
        pt[2] = ab;
      }
      __syncthreads();
      if (t < half) {
        double aa = 0.0, bb = 0.0, ab = 0.0;
        for (int l = 0; l < LANES; ++l) {
          const double* pt = sm.part + (t * LANES + l) * 3;
          aa += pt[0];
          bb += pt[1];
          ab += pt[2];
        }
        double c = 1.0, sn = 0.0;
        const double scale = sqrt(aa) * sqrt(bb);
        if (scale > 0.0 && fabs(ab) > tol * scale) {
          worst = fmax(worst, fabs(ab) / scale);
          rotation((bb - aa) / (2.0 * ab), c, sn);
        }
        sm.cs[t] = c;
        sm.sn[t] = sn;
      }
      __syncthreads();
      for (int e = t; e < half * rows; e += NT) {
        const int qq = e / rows, r = e - qq * rows;
        const double c = sm.cs[qq], sn = sm.sn[qq];
        if (sn == 0.0) continue;
        int i, j;
        rr_pair(m, s, qq, i, j);
        const double u = M[r * LD + i], v = M[r * LD + j];
        M[r * LD + i] = c * u - sn * v;
        M[r * LD + j] = sn * u + c * v;
      }
      __syncthreads();
    }
    ++sweeps;
    worst = block_max(sm.red, worst);
    if (!(worst > 0.0) || sweeps >= SVD_CAP) break;
  }
  if (t < cols) {
    double aa = 0.0;
    for (int r = 0; r < rows; ++r) aa = fma(M[r * LD + t], M[r * LD + t], aa);
    sm.w[t] = sqrt(aa);
  }
  __syncthreads();
  return sweeps;
}

// grid pairs: steps 2-6 of the reference for one pair
__global__ __launch_bounds__(NT) void cca_solve_kernel(const double* __restrict__ cross, int p, int C, double eps, double threshold,
                                                       unsigned long long* __restrict__ masks, int* __restrict__ info,
                                                       double* __restrict__ coefs, double* __restrict__ stats) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, LD = p | 1, B = p * LD;
  const size_t pair = blockIdx.x;
  Sm sm;
  sm.A = lds;
  sm.V = sm.A + B;
  sm.R = sm.V + B;
  sm.S = sm.R + B;
  sm.red = sm.S + B;
  sm.cs = sm.red + NT;
  sm.sn = sm.cs + HALF;
  sm.w = sm.sn + HALF;
  sm.f = sm.w + MAXP;
  sm.part = sm.f + MAXP;
  sm.misc = sm.part + HALF * LANES * 3;
  sm.ix = reinterpret_cast<int*>(sm.misc + 8);
  sm.iy = sm.ix + MAXP;
  sm.cnt = sm.iy + MAXP;
  const double* cp = cross + pair * (size_t)C * 3 * p * p;
  double* co = coefs + pair * p;
  double* so = stats + pair * 8;
  const double nan = __builtin_nan("");

  // block maxima and the kept neurons of both sides (Syy is folded again when its turn comes: R is needed in between)
  fold_block(cp, 2, p, C, LD, sm.R);
  const double ymax = block_absmax(sm.R, p, LD, sm.red);
  const int ky = keep_neurons(sm.R, p, LD, ymax, eps, sm.iy, sm.cnt + 1, masks + pair * MASK_WORDS + 1);
  fold_block(cp, 0, p, C, LD, sm.R);
  const double xmax = block_absmax(sm.R, p, LD, sm.red);
  const int kx = keep_neurons(sm.R, p, LD, xmax, eps, sm.ix, sm.cnt, masks + pair * MASK_WORDS);
  const int count = kx < ky ? kx : ky;
  if (count == 0) {
    for (int e = t; e < p; e += NT) co[e] = nan;
    if (t == 0) {
      so[0] = so[1] = so[2] = so[3] = 0.0;
      so[4] = (double)kx;
      so[5] = (double)ky;
      so[6] = so[7] = nan;
      int* io = info + pair * INFO_INTS;
      io[0] = io[1] = io[2] = io[3] = 0;
    }
    return;
  }

  // A = Sxx / xmax cropped, + eps on the diagonal;  S = Sxy / sqrt(xmax ymax) cropped
  for (int e = t; e < kx * kx; e += NT) {
    const int a = e / kx, b = e - a * kx;
    sm.A[a * LD + b] = sm.R[sm.ix[a] * LD + sm.ix[b]] / xmax + (a == b ? eps : 0.0);
  }
  __syncthreads();
  fold_block(cp, 1, p, C, LD, sm.R);
  const double xymax = sqrt(xmax * ymax);
  for (int e = t; e < kx * ky; e += NT) {
    const int a = e / ky, b = e - a * ky;
    sm.S[a * LD + b] = sm.R[sm.ix[a] * LD + sm.iy[b]] / xymax;
  }
  __syncthreads();

  const int sweeps_x = jacobi_sym(sm.A, sm.V, kx, LD, sm);
  const double cond_x = inv_sqrt(sm.A, sm.V, sm.R, kx, LD, sm);
  matmul(sm.R, sm.S, sm.A, kx, kx, ky, LD);                        // A = T = Sxx^(-1/2) Sxy

  fold_block(cp, 2, p, C, LD, sm.R);
  for (int e = t; e < ky * ky; e += NT) {
    const int a = e / ky, b = e - a * ky;
    sm.S[a * LD + b] = sm.R[sm.iy[a] * LD + sm.iy[b]] / ymax + (a == b ? eps : 0.0);
  }
  __syncthreads();
  const int sweeps_y = jacobi_sym(sm.S, sm.V, ky, LD, sm);
  const double cond_y = inv_sqrt(sm.S, sm.V, sm.R, ky, LD, sm);
  matmul(sm.A, sm.R, sm.S, kx, ky, ky, LD);                        // S = M = T Syy^(-1/2)

  const int sweeps_s = jacobi_svd(sm.S, kx, ky, LD, sm);

  // descending rank sort of the ky column norms (ties by index); the first `count` are the canonical correlations
  if (t < ky) {
    const double v = sm.w[t];
    int rank = 0;
    for (int j = 0; j < ky; ++j) {
      const double u = sm.w[j];
      rank += (u > v) || (u == v && j < t) || (u != u && v == v) || (u != u && v != v && j < t);
    }
    sm.f[rank] = v;
  }
  __syncthreads();
  for (int e = t; e < p; e += NT) co[e] = e < count ? sm.f[e] : nan;
  if (t == 0) {
    double sum = 0.0;
    for (int i = 0; i < count; ++i) sum += sm.f[i];
    // first i in [0, count) with sum(s[:i]) / sum(s) >= threshold; all of s if there is none
    int idx = count;
    double head = 0.0;
    for (int i = 0; i < count; ++i) {
      if (head / sum >= threshold) {
        idx = i;
        break;
      }
      head += sm.f[i];
    }
    double hs = 0.0;
    for (int i = 0; i < idx; ++i) hs += sm.f[i];
    so[0] = sum / (double)count;
    so[1] = idx > 0 ? hs / (double)idx : nan;                     // numpy's mean of an empty slice
    so[2] = sum;
    so[3] = (double)count;
    so[4] = (double)kx;
    so[5] = (double)ky;
    so[6] = cond_x;
    so[7] = cond_y;
    int* io = info + pair * INFO_INTS;
    io[0] = sweeps_x;
    io[1] = sweeps_y;
    io[2] = sweeps_s;
    io[3] = (sweeps_x >= SYM_CAP) || (sweeps_y >= SYM_CAP) || (sweeps_s >= SVD_CAP);
  }
}

size_t solve_lds_bytes(int p) {
  const size_t doubles = 4 * (size_t)p * (p | 1) + NT + 2 * HALF + 2 * MAXP + HALF * LANES * 3 + 8;
  return doubles * sizeof(double) + (2 * MAXP + 4) * sizeof(int);
}

#define CCA_LAUNCH(...)                                   \
  do {                                                    \
    hipLaunchKernelGGL(__VA_ARGS__);                      \
    if (hipError_t _e = hipGetLastError(); _e != hipSuccess) return _e; \
  } while (0)

}  // namespace

size_t cca_scratch_bytes(int pairs, int n, int p) { return layout(pairs, p, geo(n, p)).total; }

hipError_t launch_cca(hipStream_t st, const float* x, const float* y, int pairs, int n, int p, double epsilon, double threshold,
                      void* scratch, double* coefs, double* stats) {
  const Geo g = geo(n, p);
  const Layout L = layout(pairs, p, g);
  char* ws = static_cast<char*>(scratch);
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(ws + L.mask);
  int* info = reinterpret_cast<int*>(ws + L.info);
  double* colpart = reinterpret_cast<double*>(ws + L.colpart);
  double* cross = reinterpret_cast<double*>(ws + L.cross);
  CCA_LAUNCH(cca_colsum_kernel, dim3(2 * pairs * g.C), dim3(NT), 0, st, x, y, n, p, g.C, colpart);
  CCA_LAUNCH(cca_cross_kernel, dim3(pairs * g.C, g.E), dim3(NT), (size_t)(2 * p + XROWS * 2 * p) * sizeof(double), st, x, y, n, p, g.C,
             colpart, cross);
  const size_t lds = solve_lds_bytes(p);
  if (lds > 64 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cca_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        e != hipSuccess)
      return e;
  CCA_LAUNCH(cca_solve_kernel, dim3(pairs), dim3(NT), lds, st, cross, p, g.C, epsilon, threshold, masks, info, coefs, stats);
  return hipSuccess;
}
