// Elementwise kernels of the vector-step / multi-step-loss ANIL calls (mi_meta_batch_anil_lr, mi_meta_batch_anil_steps; engine.hip,
// meta_batch_anil_impl).  ANIL adapts the Linear head only, so every kernel here walks the head slice [T][Ph] (Ph = ways * feat + ways) of
// its vectors at their own per-task strides, never the whole parameter vector: the plain call's axpy moves the trunk's entries K times
// for nothing.  Flat one-dimensional grids (element = global thread index): the launch count and the grid shape limits do not depend on
// the number of tasks.  Contraction is off in this build (-ffp-contract=off): `a - b * c` is a multiply and a subtract, the expression of
// misc.hip's axpy_kernel, which is what makes the new calls reproduce the plain call's bits.
#include "mi_common.h"
#include "kernels.h"

// lr_eng[r][e] = lr_ref[r][ref(e)]: the step sizes from head.parameters() order (weight in the reference's view(-1, fc) column order, then
// bias) into the engine's head layout, with the permutation the engine applies to theta's head weight.  perm points at the head's entries
// of the parameter permutation table, base is the head's offset in the parameter vector.
__global__ void anil_gather_lr_kernel(const float* __restrict__ lr_ref, const int32_t* __restrict__ perm, int base, int ph, int ostride,
                                      int rows, float* __restrict__ lr_eng) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * ph) return;
  const size_t r = i / ph, e = i - r * ph;
  lr_eng[r * ostride + e] = lr_ref[r * ph + (perm[e] - base)];
}

// theta_{k+1} = theta_k - lr * g on the head slice (lr == nullptr: the scalar alpha).  An entry whose step is exactly 0 is copied bit for
// bit, whatever its gradient holds.
__global__ void anil_advance_kernel(const float* __restrict__ th, const float* __restrict__ g, size_t pstride, const float* __restrict__ lr,
                                    float alpha, int ph, int tasks, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)tasks * ph) return;
  const size_t t = i / ph, e = i - t * ph, o = t * pstride + e;
  const float a = th[o];
  if (lr) {
    const float l = lr[e];
    out[o] = l == 0.f ? a : a - l * g[o];
  } else {
    out[o] = a - alpha * g[o];
  }
}

// One launch per adjoint step: finishes lam_k on the head slice, leaves what the NEXT Hessian-vector pass and the step-size gradient need,
// and applies the support-feature cotangent of the pass that has just run.  The update expression comes first and unchanged, the weighted
// term behind it as a fused multiply-add: a zero weight leaves the bits of the plain recursion.
__global__ void anil_adjoint_kernel(AnilAdjArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)a.tasks * a.ph) {
    const size_t t = i / a.ph, e = i - t * a.ph;
    float l = a.lam[t * a.lstride + e];
    if (a.hv) l = l - a.alpha * a.hv[t * a.lstride + e];
    if (a.inj) l = fmaf(*a.w, a.inj[t * a.cstride + e], l);
    else if (a.w) l = *a.w * l;
    a.lam[t * a.lstride + e] = l;
    if (a.lr) a.dir[t * a.cstride + e] = a.lr[e] * l;
    if (a.prod) a.prod[t * a.cstride + e] = a.g[t * a.lstride + e] * l;
  }
  if (a.rdf && i < a.fcount) a.dfs[i] = a.dfs[i] - a.alpha * a.rdf[i];
}

// lr_grad[r][ref(e)] = -sum_k sum_t prod[k][t][e] (or g_k[t][e] * lam[t][e]: a first-order call with one constant lam), k over the
// updates of row r ascending, t ascending: ONE fp64 chain in that fixed order, rounded once, no atomics.  grid (ceil(ph / 256), lr_steps).
__global__ void anil_lr_fold_kernel(const float* __restrict__ prod, size_t cstride, const float* __restrict__ g, const float* __restrict__ lam,
                                    size_t pstride, const int32_t* __restrict__ perm, int base, int ph, int tasks, int steps, int lr_steps,
                                    float* __restrict__ out_ref) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ph) return;
  const int r = blockIdx.y;
  const int k0 = lr_steps == 1 ? 0 : r, k1 = lr_steps == 1 ? steps : r + 1;
  double acc = 0.0;
  for (int k = k0; k < k1; ++k)
    for (int t = 0; t < tasks; ++t) {
      const size_t kt = (size_t)k * tasks + t;
      const float pr = prod ? prod[kt * cstride + e] : g[kt * pstride + e] * lam[(size_t)t * pstride + e];
      acc += (double)pr;
    }
  out_ref[(size_t)r * ph + (perm[e] - base)] = (float)(0.0 - acc);
}

static unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_anil_gather_lr(hipStream_t st, const float* lr_ref, const int32_t* perm, int base, int ph, int ostride, int rows,
                                 float* lr_eng) {
  hipLaunchKernelGGL(anil_gather_lr_kernel, dim3(blocks_of((size_t)rows * ph)), dim3(256), 0, st, lr_ref, perm, base, ph, ostride, rows, lr_eng);
  return hipGetLastError();
}
hipError_t launch_anil_advance(hipStream_t st, const float* th, const float* g, size_t pstride, const float* lr, float alpha, int ph,
                               int tasks, float* out) {
  hipLaunchKernelGGL(anil_advance_kernel, dim3(blocks_of((size_t)tasks * ph)), dim3(256), 0, st, th, g, pstride, lr, alpha, ph, tasks, out);
  return hipGetLastError();
}
hipError_t launch_anil_adjoint(hipStream_t st, const AnilAdjArgs& a) {
  const size_t head = (size_t)a.tasks * a.ph, n = a.rdf && a.fcount > head ? a.fcount : head;
  hipLaunchKernelGGL(anil_adjoint_kernel, dim3(blocks_of(n)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_anil_lr_fold(hipStream_t st, const float* prod, size_t cstride, const float* g, const float* lam, size_t pstride,
                               const int32_t* perm, int base, int ph, int tasks, int steps, int lr_steps, float* out_ref) {
  hipLaunchKernelGGL(anil_lr_fold_kernel, dim3(ceil_div(ph, 256), lr_steps), dim3(256), 0, st, prod, cstride, g, lam, pstride, perm, base, ph,
                     tasks, steps, lr_steps, out_ref);
  return hipGetLastError();
}
