// Proto-MAML head initialisation for a whole meta-batch (Triantafillou et al., "Meta-Dataset", eq. 8): the linear head
// that reproduces the Prototypical-Networks logits up to a per-row constant, derived per task from the support features, and its backward.
// Per task, N_w = #{i : ys_i = w} >= 1 for every class (the caller's contract, as for metric_head.hip), s = scale:
//   c_w = (1/N_w) sum_{i in w} fs_i          W_0[w] = 2 s c_w          b_0[w] = -s |c_w|^2
//   dc_w = 2 s (lamW[w] - lamb[w] c_w)       dfs_i += dc_{ys_i} / N_{ys_i}       dscale = sum_w (2 <lamW[w], c_w> - lamb[w] |c_w|^2)
// where (lamW, lamb) = d objective / d (W_0, b_0).  Two kernels, ONE launch each for the whole meta-batch; fp32 VALU arithmetic on the
// elements, the two reductions over feat (|c_w|^2, dscale) in fp64; every sum in a fixed order that depends on the task's own sizes only, no
// float atomics, plain vector stores: a task's bits do not depend on `tasks` or on where it ran.  No loop bound depends on data; the labels
// select which support rows a class reads (a branch, uniform over the workgroup in the forward kernel).
//   forward   a workgroup of 256 threads per (class, task): a thread per 4 adjacent feature columns forms c_w over the support rows in
//             ascending order, stores W_0 and keeps c^2 in an fp64 partial; lanes, then waves, are folded in ascending order for b_0.
//   backward  a workgroup of 512 threads per task, a thread per (class, 4 adjacent columns) item, items ascending: c_w AGAIN by the forward
//             kernel's code (class_mean: the same bits, nothing kept between the launches), dc, then one read-modify-write of dfs per
//             support row of the class -- each element by the one thread that owns its (class, column) item -- and the item's fp64 term of
//             dscale; lanes, then waves, folded in ascending order.
// fs is read once by either kernel (a row belongs to one class); the labels are re-read per item from L1/L2 (ns words).
#include "mi_common.h"
#include "kernels.h"
#include "../../include/mi_maml.h"

namespace {
constexpr int kFwdThreads = 256, kBwdThreads = 512;

// Up to four adjacent floats of a row from column i: one 16-byte access (VEC: every row starts on a 16-byte boundary and feat % 4 == 0), or
// nv <= 4 words.  Either way a thread owns the same columns, so a result's bits do not depend on the alignment of the caller's pointers.
template <bool VEC>
__device__ __forceinline__ void ld4(const float* p, int nv, float (&x)[4]) {
  if constexpr (VEC) {
    row_ld<4>(p, x);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = u < nv ? p[u] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void st4(float* p, int nv, const float (&x)[4]) {
  if constexpr (VEC) {
    row_st<4>(p, x);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < nv) p[u] = x[u];
  }
}

// c_w on the (up to) four columns from column i, and N_w: support rows ascending, one rounding per addition, one division at the end.  The
// ONE definition both kernels use, so that the backward's c_w is the forward's bit for bit.  Columns past feat hold zeros.
template <bool VEC>
__device__ __forceinline__ float class_mean(const float* fs, const int32_t* ys, int NS, int F, int w, int i, int nv, float (&c)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) c[u] = 0.f;
  int n = 0;
  for (int s = 0; s < NS; ++s) {
    if (ys[s] != w) continue;
    float x[4];
    ld4<VEC>(fs + (size_t)s * F + i, nv, x);
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] += x[u];
    ++n;
  }
  const float nw = (float)(n > 0 ? n : 1);
#pragma unroll
  for (int u = 0; u < 4; ++u) c[u] = c[u] / nw;
  return nw;
}

// Sum of one fp64 value per thread: lanes by wave_sum, waves ascending by thread 0 (which alone holds the result).
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double tot = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) tot += red[k];
  }
  return tot;
}

template <bool VEC>
__global__ __launch_bounds__(kFwdThreads) void proto_init_kernel(ProtoInitArgs a) {
  __shared__ double red[kFwdThreads / 64];
  const int task = blockIdx.x / a.ways, w = blockIdx.x - task * a.ways, F = a.feat;
  const float* fs = a.fs + (size_t)task * a.ns * F;
  const int32_t* ys = a.ys + (size_t)task * a.ns;
  float* out = a.head + (size_t)task * a.stride;
  const float two_s = 2.f * a.scale;
  double sq = 0.0;
  for (int i = threadIdx.x * 4; i < F; i += kFwdThreads * 4) {
    const int nv = F - i < 4 ? F - i : 4;
    float c[4], o[4];
    class_mean<VEC>(fs, ys, a.ns, F, w, i, nv, c);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      o[u] = two_s * c[u];
      sq += (double)c[u] * (double)c[u];
    }
    st4<VEC>(out + (size_t)w * F + i, nv, o);
  }
  const double tot = block_sum<kFwdThreads>(sq, red);
  if (threadIdx.x == 0) out[(size_t)a.ways * F + w] = (float)(-(double)a.scale * tot);
}

template <bool VEC>
__global__ __launch_bounds__(kBwdThreads) void proto_init_bwd_kernel(ProtoInitArgs a) {
  __shared__ double red[kBwdThreads / 64];
  const int task = blockIdx.x, F = a.feat, NS = a.ns;
  const float* fs = a.fs + (size_t)task * NS * F;
  const int32_t* ys = a.ys + (size_t)task * NS;
  const float* lam = a.lam + (size_t)task * a.stride;
  const float* lamb = lam + (size_t)a.ways * F;
  float* dfs = a.dfs + (size_t)task * NS * F;
  const float two_s = 2.f * a.scale;
  const int chunks = (F + 3) / 4, items = a.ways * chunks;
  double ds = 0.0;
  for (int it = threadIdx.x; it < items; it += kBwdThreads) {
    const int w = it / chunks, i = (it - w * chunks) * 4, nv = F - i < 4 ? F - i : 4;
    float c[4], lw[4], dc[4];
    const float nw = class_mean<VEC>(fs, ys, NS, F, w, i, nv, c);
    ld4<VEC>(lam + (size_t)w * F + i, nv, lw);
    const float lb = lamb[w];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dc[u] = (two_s * (lw[u] - lb * c[u])) / nw;
      ds += (double)c[u] * (2.0 * (double)lw[u] - (double)lb * (double)c[u]);
    }
    for (int s = 0; s < NS; ++s) {
      if (ys[s] != w) continue;
      float d[4];
      ld4<VEC>(dfs + (size_t)s * F + i, nv, d);
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] += dc[u];
      st4<VEC>(dfs + (size_t)s * F + i, nv, d);
    }
  }
  if (!a.dscale) return;
  const double tot = block_sum<kBwdThreads>(ds, red);
  if (threadIdx.x == 0) a.dscale[task] = (float)tot;
}
}  // namespace

// The kernels keep nothing task-sized on chip, so the domain is the stated one: sizes >= 1, ways <= 64 (the head kernels' lane per class), feat <= MI_RIDGE_MAX_FEAT (a stated cap, as for the ridge head), scale > 0 and finite.
bool proto_init_fits(int tasks, int ns, int feat, int ways) {
  return tasks >= 1 && ns >= 1 && feat >= 1 && feat <= MI_RIDGE_MAX_FEAT && ways >= 1 && ways <= 64;
}
static bool proto_init_ok(const ProtoInitArgs& a, int tasks) {
  return proto_init_fits(tasks, a.ns, a.feat, a.ways) && a.scale > 0.f && a.scale <= 3.402823466e38f && a.fs && a.ys;
}

// 16-byte accesses when every row starts on a 16-byte boundary: feat % 4 == 0, 16-byte aligned bases and a stride that is a multiple of 4
// floats; words otherwise, with the same bits.  Outside the domain: hipErrorInvalidValue, nothing launched (callers check proto_init_fits first).
static bool rows_aligned(const ProtoInitArgs& a, const void* p, const void* q) {
  return a.feat % 4 == 0 && a.stride % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.fs) | reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}
hipError_t launch_proto_init(hipStream_t st, const ProtoInitArgs& a, int tasks) {
  if (!proto_init_ok(a, tasks) || !a.head) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tasks * a.ways);
  if (rows_aligned(a, a.head, nullptr)) hipLaunchKernelGGL(proto_init_kernel<true>, grid, dim3(kFwdThreads), 0, st, a);
  else hipLaunchKernelGGL(proto_init_kernel<false>, grid, dim3(kFwdThreads), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_proto_init_bwd(hipStream_t st, const ProtoInitArgs& a, int tasks) {
  if (!proto_init_ok(a, tasks) || !a.lam || !a.dfs) return hipErrorInvalidValue;
  if (rows_aligned(a, a.lam, a.dfs)) hipLaunchKernelGGL(proto_init_bwd_kernel<true>, dim3(tasks), dim3(kBwdThreads), 0, st, a);
  else hipLaunchKernelGGL(proto_init_bwd_kernel<false>, dim3(tasks), dim3(kBwdThreads), 0, st, a);
  return hipGetLastError();
}
