// Metric heads for a whole meta-batch: the closed-form classifiers of Prototypical Networks and of NIL ("No Inner Loop", the ANIL paper's
// test-time head) on the trunk's flattened features, with CrossEntropyLoss(reduction='mean'), accuracy and the backward to the features.
// No head parameters, no inner loop.  Per task, N_w = #{i : ys_i = w} >= 1 for every class (the caller's contract):
//   MI_METRIC_PROTO   c_w = (1/N_w) sum_{i in w} fs_i              z_qw = -scale * sum_k (fq_qk - c_wk)^2   (the difference form, never expanded)
//   MI_METRIC_COSINE  xh = x / max(|x|, 1e-8),  c_w = sum_{i in w} sh_i   z_qw = scale * <qh_q, c_w>
//   loss = mean_q CE(z_q, yq_q), acc = mean_q [argmax_w z_q == yq_q] (first maximum, as head_bodies.h), dz = (softmax(z) - onehot) / nq
//   proto   dfq_q = -2 scale sum_w dz_qw (fq_q - c_w),  dc_w = 2 scale sum_q dz_qw (fq_q - c_w),  dfs_i = dc_{ys_i} / N_{ys_i}
//   cosine  dqh_q = scale sum_w dz_qw c_w,  dc_w = scale sum_q dz_qw qh_q,  dsh_i = dc_{ys_i};  through the normalisation
//           dx = (dxh - <dxh, xh> xh) / |x| for |x| >= 1e-8, dx = dxh / 1e-8 below it.
// One workgroup of 512 threads per task, ONE launch for the whole meta-batch (forward, or forward + backward); fp32 VALU arithmetic, every sum
// in a fixed order that depends on the task's own sizes only, no float atomics: a task's bits do not depend on `tasks` or on where it ran.
//   phase 0  class counts; cosine: the support rows' norms (a wave per row)
//   phase 1  class vectors into LDS, a thread per (4 adjacent) feature column(s), support rows in ascending order
//   phase 2  a wave per query row: `ways` distances / inner products against the LDS block (8 classes per sweep of the row), softmax, dz -> LDS;
//            cosine backward: one more sweep of the row for <dqh_q, qh_q>
//   phase 3  a thread per (4) feature column(s): one sweep over the query rows gives dfq[:, i] and dc[:, i]; dc replaces c in LDS
//   phase 4  a wave per support row: dfs from the dc block
// fq is read twice (phases 2 and 3; cosine backward: a third time in phase 2; once more per further 8 classes), fs twice (proto: 1, 4) or
// three times (cosine: 0, 1, 4); a task's
// features are at most 160 KB, so every read after the first comes from L2.
// LDS (floats): c [ways * feat, rounded up to 4] | dz [nq * ways] | counts [ways] | support norms [ns] | query norms, <dz, z>, row loss, row hit [4 * nq]
#include "mi_common.h"
#include "kernels.h"
#include "../../include/mi_maml.h"

namespace {
constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr float kEps = 1e-8f;

// max(|x|, 1e-8) of a row, NEGATED when the clamp is active (the backward then has no projection term).  Rows are DIVIDED by it, as the
// definition says: a one-feature row is then exactly +-1 and its gradient exactly 0.
__device__ __forceinline__ float signed_norm(float ss) {
  const float nrm = sqrtf(ss);
  return nrm >= kEps ? nrm : -kEps;
}

struct Lds {
  float *c, *dz, *cnt, *rns, *rnq, *pq, *rl, *rh;
};
__device__ __forceinline__ Lds carve(float* sm, int ns, int nq, int feat, int ways) {
  Lds l;
  l.c = sm;
  l.dz = sm + (((size_t)ways * feat + 3) & ~(size_t)3);
  l.cnt = l.dz + (size_t)nq * ways;
  l.rns = l.cnt + ways;
  l.rnq = l.rns + ns;
  l.pq = l.rnq + nq;
  l.rl = l.pq + nq;
  l.rh = l.rl + nq;
  return l;
}

template <bool BWD, int VW>
__device__ __forceinline__ void metric_task(const MetricArgs& a, float* sm) {
  const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NS = a.ns, NQ = a.nq, F = a.feat, WY = a.ways;
  const bool cosine = a.h.metric == MI_METRIC_COSINE;
  const float scale = a.h.scale;
  const float* fs = a.fs + (size_t)task * NS * F;
  const float* fq = a.fq + (size_t)task * NQ * F;
  const int32_t* ys = a.ys + (size_t)task * NS;
  const int32_t* yq = a.yq + (size_t)task * NQ;
  const Lds l = carve(sm, NS, NQ, F, WY);

  // ---- phase 0: N_w; cosine: 1 / max(|fs_i|, 1e-8)
  for (int w = tid; w < WY; w += kThreads) {
    int n = 0;
    for (int s = 0; s < NS; ++s) n += ys[s] == w ? 1 : 0;
    l.cnt[w] = (float)(n > 0 ? n : 1);
  }
  if (cosine) {
    for (int s = wave; s < NS; s += kWaves) {
      float ss = 0.f;
      for (int i = lane * VW; i < F; i += 64 * VW) {
        float x[VW];
        row_ld<VW>(fs + (size_t)s * F + i, x);
#pragma unroll
        for (int u = 0; u < VW; ++u) ss = fmaf(x[u], x[u], ss);
      }
      ss = wave_sum(ss);
      if (lane == 0) l.rns[s] = signed_norm(ss);
    }
  }
  __syncthreads();

  // ---- phase 1: class vectors, each thread on columns of its own (support rows ascending: a fixed order)
  for (int i = tid * VW; i < F; i += kThreads * VW) {
    float z[VW];
#pragma unroll
    for (int u = 0; u < VW; ++u) z[u] = 0.f;
    for (int w = 0; w < WY; ++w) row_st<VW>(l.c + (size_t)w * F + i, z);
    for (int s = 0; s < NS; ++s) {
      const int w = ys[s];
      if ((unsigned)w >= (unsigned)WY) continue;
      float x[VW], cur[VW];
      row_ld<VW>(fs + (size_t)s * F + i, x);
      row_ld<VW>(l.c + (size_t)w * F + i, cur);
      const float r = cosine ? fabsf(l.rns[s]) : 1.f;
#pragma unroll
      for (int u = 0; u < VW; ++u) cur[u] += cosine ? x[u] / r : x[u];
      row_st<VW>(l.c + (size_t)w * F + i, cur);
    }
    if (!cosine) {
      for (int w = 0; w < WY; ++w) {
        float cur[VW];
        row_ld<VW>(l.c + (size_t)w * F + i, cur);
        const float nw = l.cnt[w];
#pragma unroll
        for (int u = 0; u < VW; ++u) cur[u] = cur[u] / nw;
        row_st<VW>(l.c + (size_t)w * F + i, cur);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the [nq][ways] table, a wave per query row; lane w ends up with z_qw
  const float invn = 1.f / (float)NQ;
  for (int q = wave; q < NQ; q += kWaves) {
    const float* xq = fq + (size_t)q * F;
    float mine = 0.f, ss = 0.f;
    for (int c0 = 0; c0 < WY; c0 += 8) {
      float part[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) part[w] = 0.f;
      float ssp = 0.f;
      for (int i = lane * VW; i < F; i += 64 * VW) {
        float x[VW];
        row_ld<VW>(xq + i, x);
        if (cosine && c0 == 0) {
#pragma unroll
          for (int u = 0; u < VW; ++u) ssp = fmaf(x[u], x[u], ssp);
        }
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          if (c0 + w < WY) {
            float cv[VW];
            row_ld<VW>(l.c + (size_t)(c0 + w) * F + i, cv);
#pragma unroll
            for (int u = 0; u < VW; ++u) {
              if (cosine) {
                part[w] = fmaf(x[u], cv[u], part[w]);
              } else {
                const float d = x[u] - cv[u];
                part[w] = fmaf(d, d, part[w]);
              }
            }
          }
        }
      }
      if (cosine && c0 == 0) ss = wave_sum(ssp);
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        if (c0 + w < WY) {
          const float d = wave_sum(part[w]);
          if (lane == c0 + w) mine = d;
        }
      }
    }
    const float rq = cosine ? signed_norm(ss) : 1.f;
    const float zq = cosine ? scale * (mine / fabsf(rq)) : -scale * mine;
    // softmax over lanes 0..WY-1, first maximal index (head_bodies.h)
    const bool act = lane < WY;
    const int y = yq[q];
    float mx = act ? zq : -INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const unsigned long long eq = __ballot(act && zq == mx);
    const int am = __ffsll((long long)eq) - 1;
    const float ex = act ? expf(zq - mx) : 0.f;
    const float se = wave_sum(ex);
    const float ly = __shfl(zq, y & 63, 64);
    const float dl = act ? (ex / se - (lane == y ? 1.f : 0.f)) * invn : 0.f;
    // cosine backward: <dqh_q, qh_q> with dqh_q = scale sum_w dz_qw c_w, formed per feature exactly as phase 3 forms it (8 classes per sweep,
    // classes ascending), so that what phase 3 subtracts is the projection of the very vector it holds
    float proj = 0.f;
    if (BWD && cosine && rq > 0.f) {
      for (int c0 = 0; c0 < WY; c0 += 8) {
        float g[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) g[w] = __shfl(dl, (c0 + w) & 63, 64);
        for (int i = lane * VW; i < F; i += 64 * VW) {
          float x[VW], av[VW];
          row_ld<VW>(xq + i, x);
#pragma unroll
          for (int u = 0; u < VW; ++u) av[u] = 0.f;
#pragma unroll
          for (int w = 0; w < 8; ++w) {
            if (c0 + w < WY) {
              float cv[VW];
              row_ld<VW>(l.c + (size_t)(c0 + w) * F + i, cv);
#pragma unroll
              for (int u = 0; u < VW; ++u) av[u] = fmaf(g[w], cv[u], av[u]);
            }
          }
#pragma unroll
          for (int u = 0; u < VW; ++u) proj = fmaf(scale * av[u], x[u] / rq, proj);
        }
      }
      proj = wave_sum(proj);
    }
    if (act) {
      l.dz[(size_t)q * WY + lane] = dl;
      if (a.logits) a.logits[((size_t)task * NQ + q) * WY + lane] = zq;
    }
    if (lane == 0) {
      l.rnq[q] = rq;
      l.pq[q] = proj;
      l.rl[q] = (mx + logf(se)) - ly;
      l.rh[q] = am == y ? 1.f : 0.f;
    }
  }
  __syncthreads();
  if (tid == 0) {                       // (the row losses in fp64, as head_reduce_kernel)
    double ls = 0.0;
    float cs = 0.f;
    for (int q = 0; q < NQ; ++q) { ls += (double)l.rl[q]; cs += l.rh[q]; }
    a.loss[task] = (float)(ls / (double)NQ);
    a.acc[task] = cs / (float)NQ;
  }
  if (!BWD) return;

  // ---- phase 3: dfq[:, i] and dc[:, i] from one sweep over the query rows per 8 classes; dc[w][i] then replaces c[w][i] (this thread's own column)
  const float two_s = 2.f * scale;
  float* dfq = a.dfq ? a.dfq + (size_t)task * NQ * F : nullptr;
  for (int i = tid * VW; i < F; i += kThreads * VW) {
    for (int c0 = 0; c0 < WY; c0 += 8) {
      float cv[8][VW], dc[8][VW];
#pragma unroll
      for (int w = 0; w < 8; ++w) {
#pragma unroll
        for (int u = 0; u < VW; ++u) { cv[w][u] = 0.f; dc[w][u] = 0.f; }
        if (c0 + w < WY) row_ld<VW>(l.c + (size_t)(c0 + w) * F + i, cv[w]);
      }
      for (int q = 0; q < NQ; ++q) {
        float x[VW], av[VW];
        row_ld<VW>(fq + (size_t)q * F + i, x);
        const float rq = l.rnq[q], ra = fabsf(rq);
        if (cosine) {
#pragma unroll
          for (int u = 0; u < VW; ++u) x[u] = x[u] / ra;        // qh
        }
#pragma unroll
        for (int u = 0; u < VW; ++u) av[u] = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          if (c0 + w < WY) {
            const float g = l.dz[(size_t)q * WY + c0 + w];
#pragma unroll
            for (int u = 0; u < VW; ++u) {
              if (cosine) {
                av[u] = fmaf(g, cv[w][u], av[u]);
                dc[w][u] = fmaf(g, x[u], dc[w][u]);
              } else {
                const float d = x[u] - cv[w][u];
                av[u] = fmaf(g, d, av[u]);
                dc[w][u] = fmaf(g, d, dc[w][u]);
              }
            }
          }
        }
        if (dfq) {
          float o[VW];
          const float proj = (c0 == 0 && rq > 0.f) ? l.pq[q] : 0.f;
#pragma unroll
          for (int u = 0; u < VW; ++u) o[u] = cosine ? (scale * av[u] - proj * x[u]) / ra : -two_s * av[u];
          if (c0 > 0) {                  // more than 8 classes: this thread's own element again, chunks ascending
            float prev[VW];
            row_ld<VW>(dfq + (size_t)q * F + i, prev);
#pragma unroll
            for (int u = 0; u < VW; ++u) o[u] = prev[u] + o[u];
          }
          row_st<VW>(dfq + (size_t)q * F + i, o);
        }
      }
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        if (c0 + w < WY) {
#pragma unroll
          for (int u = 0; u < VW; ++u) dc[w][u] = (cosine ? scale : two_s) * dc[w][u];
          row_st<VW>(l.c + (size_t)(c0 + w) * F + i, dc[w]);
        }
      }
    }
  }
  if (!a.dfs) return;
  __syncthreads();

  // ---- phase 4: dfs, a wave per support row
  float* dfs = a.dfs + (size_t)task * NS * F;
  for (int s = wave; s < NS; s += kWaves) {
    const int w = ys[s];
    const bool ok = (unsigned)w < (unsigned)WY;
    const float* dcw = l.c + (size_t)(ok ? w : 0) * F;
    const float* xs = fs + (size_t)s * F;
    const float rs = cosine ? l.rns[s] : 1.f, ra = fabsf(rs);
    float dot = 0.f;
    if (cosine && rs > 0.f) {
      for (int i = lane * VW; i < F; i += 64 * VW) {
        float x[VW], d[VW];
        row_ld<VW>(xs + i, x);
        row_ld<VW>(dcw + i, d);
#pragma unroll
        for (int u = 0; u < VW; ++u) dot = fmaf(d[u], x[u] / ra, dot);
      }
      dot = wave_sum(dot);
    }
    const float nw = ok ? l.cnt[w] : 1.f;
    for (int i = lane * VW; i < F; i += 64 * VW) {
      float d[VW], o[VW];
      row_ld<VW>(dcw + i, d);
      if (cosine) {
        float x[VW];
        row_ld<VW>(xs + i, x);
#pragma unroll
        for (int u = 0; u < VW; ++u) o[u] = (d[u] - dot * (x[u] / ra)) / ra;
      } else {
#pragma unroll
        for (int u = 0; u < VW; ++u) o[u] = d[u] / nw;
      }
      if (!ok) {
#pragma unroll
        for (int u = 0; u < VW; ++u) o[u] = 0.f;
      }
      row_st<VW>(dfs + (size_t)s * F + i, o);
    }
  }
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void metric_head_kernel(MetricArgs a) {
  extern __shared__ __attribute__((aligned(16))) float metric_sm[];
  // 16-byte global and LDS accesses when every row starts on a 16-byte boundary (the entry points require 16-byte aligned bases)
  const bool vec = a.feat % 4 == 0;
  if (vec) metric_task<BWD, 4>(a, metric_sm);
  else metric_task<BWD, 1>(a, metric_sm);
}
}  // namespace

// Dynamic LDS of one task (the kernel has no static LDS, so a request may take all of a CU's 160 KiB):
//   4 * (roundup4(ways * feat) + nq * ways + ways + ns + 4 * nq) <= 163840, ways <= 64.
// 5-way: feat <= 8180 at ns = nq = 5, 8140 at ns = nq = 25;  20-way 1600 features (128 KB): nq <= 357 at ns = nq.
size_t metric_head_lds_bytes(int ns, int nq, int feat, int ways) {
  return ((((size_t)ways * feat + 3) & ~(size_t)3) + (size_t)nq * ways + ways + ns + 4 * (size_t)nq) * sizeof(float);
}
bool metric_head_fits(int ns, int nq, int feat, int ways) {
  return ns >= 1 && nq >= 1 && feat >= 1 && ways >= 1 && ways <= 64 && metric_head_lds_bytes(ns, nq, feat, ways) <= head_lds_limit_bytes();
}

// A request above 64 KiB needs allow_dynamic_lds (mi_common.h): raised to the device's whole LDS (not to this launch's size), so that a later,
// larger request of the same process is covered too.
template <bool BWD>
static hipError_t metric_launch(hipStream_t st, const MetricArgs& a, int tasks) {
  const size_t sm = metric_head_lds_bytes(a.ns, a.nq, a.feat, a.ways);
  if (sm > 64 * 1024) {
    static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(metric_head_kernel<BWD>), head_lds_limit_bytes(), &attr_done); e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(metric_head_kernel<BWD>, dim3(tasks), dim3(kThreads), sm, st, a);
  return hipGetLastError();
}

// Forward (a.dfs == a.dfq == NULL) or forward + backward, one launch either way.  Outside the domain: hipErrorInvalidValue, nothing launched
// (callers check metric_head_fits first and report MI_ERR_ARG).
hipError_t launch_metric_head(hipStream_t st, const MetricArgs& a, int tasks) {
  if (tasks < 1 || !metric_head_fits(a.ns, a.nq, a.feat, a.ways) || (a.h.metric != MI_METRIC_PROTO && a.h.metric != MI_METRIC_COSINE) || !(a.h.scale > 0.f))
    return hipErrorInvalidValue;
  return (a.dfs || a.dfq) ? metric_launch<true>(st, a, tasks) : metric_launch<false>(st, a, tasks);
}
