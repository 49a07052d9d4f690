// Classifier head for a whole meta-batch: Linear(F, ways) + CrossEntropyLoss(reduction='mean') forward, backward and
// tangent (per-task fast weights).
// Replaces (reference): MiniImagenetCNN.forward's `self.linear(x.view(-1, 25*hidden))` (core_functions/vision_models.py:109),
// OmniglotCNN.forward's mean+linear (:53-54), `loss(learner(adapt_data), adapt_labels)` (core_functions/vision.py:11,16),
// `accuracy` (vision.py:21-23) and the autograd backward / double-backward of addmm + log_softmax + nll_loss.
// Features arrive in NHWC flatten order; the engine permutes linear.weight's columns once at the boundary so the result
// equals the reference's NCHW `view`.
#include "mi_common.h"
#include "kernels.h"
#include "head_bodies.h"

template <bool TANGENT>
__global__ __launch_bounds__(256) void head_rows_kernel(HeadArgs a) {
  const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y * 4 + wave;
  if (n >= a.n) return;
  head_row<TANGENT>(a, task, n, lane);
}

template <bool TANGENT>
__global__ __launch_bounds__(256) void head_grads_kernel(HeadArgs a) {
  extern __shared__ float sm[];
  const int task = blockIdx.x, tid = threadIdx.x;
  const int N = a.n, WY = a.ways;
  float* s_a = sm;               // [N][WY]: dl (primal) or R{dl} (tangent)
  float* s_b = sm + N * WY;      // [N][WY]: dl (tangent only)
  head_stage_dl<TANGENT>(a, task, tid, 256, s_a, s_b);
  __syncthreads();
  float* s_red = sm + (TANGENT ? 2 : 1) * N * WY;   // [3][8][64] partial sums of groups 1..3
  head_grads_chunk<TANGENT>(a, task, blockIdx.y, tid, s_a, s_b, s_red);
  if (blockIdx.y == 0) head_task_sums<TANGENT>(a, task, tid, 256, s_a);
}

// loss[t] = mean_n rowloss, acc[t] = mean_n rowhit (fixed order)
__global__ void head_reduce_kernel(const float* __restrict__ rowloss, const float* __restrict__ rowhit, int tasks, int n,
                                   float* __restrict__ loss, float* __restrict__ acc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tasks) return;
  // (the row losses in fp64: a sequential fp32 sum of n terms is off by ~sqrt(n) ulp of the SUM -- 2.8e-6 of the mean at n = 2464; the hits are
  // small integers, exact in fp32)
  double ls = 0.0;
  float cs = 0.f;
  for (int k = 0; k < n; ++k) { ls += (double)rowloss[(size_t)t * n + k]; cs += rowhit[(size_t)t * n + k]; }
  loss[t] = (float)(ls / (double)n);
  acc[t] = cs / (float)n;
}

// OmniglotCNN: x.mean(dim=[2,3]) (vision_models.py:53).  rows = T*N, p [rows][hw][c] -> f [rows][c]; linear, so the
// tangent uses the same kernel and the backward is a broadcast / hw.
__global__ void spatial_mean_kernel(const float* __restrict__ p, float* __restrict__ f, int rows, int hw, int c) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)rows * c) return;
  const size_t row = e / c, ch = e - row * c;
  float s = 0.f;
  for (int k = 0; k < hw; ++k) s += p[(row * hw + k) * c + ch];
  f[e] = s / (float)hw;
}
__global__ void spatial_mean_bwd_kernel(const float* __restrict__ df, float* __restrict__ dp, int rows, int hw, int c) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)rows * hw * c) return;
  const size_t ch = e % c, row = e / ((size_t)hw * c);
  dp[e] = df[row * c + ch] / (float)hw;
}

// Dynamic LDS of head_grads_kernel: a whole task's dl [n][ways] (tangent: R{dl} and dl) and the [3][8][64] fold buffer of the row groups.
// The kernel has no static LDS, so a request may take all of a CU's 160 KiB (gfx950; one workgroup may hold the whole of it):
//   primal  n * ways <= 39424,   tangent  n * ways <= 19712.
size_t head_grads_lds_bytes(int n, int ways, int tangent) { return ((size_t)(tangent ? 2 : 1) * (size_t)n * (size_t)ways + 3 * 8 * 64) * sizeof(float); }
size_t head_lds_limit_bytes() { return (size_t)160 * 1024; }
bool head_lds_fits(int n, int ways, int tangent) { return n >= 1 && ways >= 1 && head_grads_lds_bytes(n, ways, tangent) <= head_lds_limit_bytes(); }

// A request above 64 KiB needs allow_dynamic_lds (mi_common.h): raised to the device's whole LDS, so that a later, larger request of the same
// process is covered too.  A request above the device's LDS is refused before anything is launched.
template <bool TANGENT>
static hipError_t head_grads_launch(hipStream_t st, const HeadArgs& a, int tasks) {
  const size_t sm = head_grads_lds_bytes(a.n, a.ways, TANGENT ? 1 : 0);
  if (sm > head_lds_limit_bytes()) return hipErrorInvalidValue;
  if (sm > 64 * 1024) {
    static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(head_grads_kernel<TANGENT>), head_lds_limit_bytes(), &attr_done); e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(head_grads_kernel<TANGENT>, dim3(tasks, ceil_div(a.feat, 64)), dim3(256), sm, st, a);
  return hipGetLastError();
}

hipError_t launch_head_fwd_bwd(hipStream_t st, const HeadArgs& a, int tasks, int with_grad) {
  if (a.ways > 64) return hipErrorInvalidValue;
  if (with_grad && !head_lds_fits(a.n, a.ways, 0)) return hipErrorInvalidValue;      // (before the rows launch: nothing runs)
  hipLaunchKernelGGL(head_rows_kernel<false>, dim3(tasks, ceil_div(a.n, 4)), dim3(256), 0, st, a);
  if (with_grad) return head_grads_launch<false>(st, a, tasks);     // the gradient launch also folds the row losses / hits into loss[t], acc[t]
  hipLaunchKernelGGL(head_reduce_kernel, dim3(ceil_div(tasks, 64)), dim3(64), 0, st, a.rowloss, a.rowhit, tasks, a.n, a.loss, a.acc);
  return hipGetLastError();
}
hipError_t launch_head_tangent(hipStream_t st, const HeadArgs& a, int tasks) {
  if (a.ways > 64 || !head_lds_fits(a.n, a.ways, 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_rows_kernel<true>, dim3(tasks, ceil_div(a.n, 4)), dim3(256), 0, st, a);
  return head_grads_launch<true>(st, a, tasks);
}
// Backward of the linear head from caller-supplied dlogits (a.dl): dWl, dbl, df.  Used by the step-wise learner whose loss
// is computed outside the engine (rc_vision.py:68-70 scales it, cl_vision.py:58-59 does not).
hipError_t launch_head_grads(hipStream_t st, const HeadArgs& a, int tasks) {
  if (a.ways > 64 || !head_lds_fits(a.n, a.ways, 0)) return hipErrorInvalidValue;
  return head_grads_launch<false>(st, a, tasks);
}
hipError_t launch_spatial_mean(hipStream_t st, const float* p, float* f, int rows, int hw, int c) {
  const size_t n = (size_t)rows * c;
  hipLaunchKernelGGL(spatial_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, f, rows, hw, c);
  return hipGetLastError();
}
hipError_t launch_spatial_mean_bwd(hipStream_t st, const float* df, float* dp, int rows, int hw, int c) {
  const size_t n = (size_t)rows * hw * c;
  hipLaunchKernelGGL(spatial_mean_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, df, dp, rows, hw, c);
  return hipGetLastError();
}
