// Counter-based task draw: the image indices, task labels and class rotations of a meta-batch, drawn on the
// device so that the sampler of utils/data_pre.py:16-112 (NWays / KShots / RemapLabels / ConsecutiveLabels / RandomClassRotation)
// needs no host arrays and no copies.  A task is a pure function of (seed, task id): Philox4x32-10 with key = seed and counter =
// (id_lo, id_hi, stream, block), integer arithmetic only -- exploring_meta_amd/utils/task_sampler.py restates it in numpy and the
// two agree bit for bit.
//
// One wave per task.  Phase 1: lane 0 picks the classes (stream 1), lane 1 the label permutation (stream 2) -- the same selection
// routine on different arguments, so the two run together -- then lane 2 the rotations (stream 3) while lane 0 sorts the classes.
// Phase 2: lane j draws the k samples of the j-th class on stream 16 + j.  Phase 3: all lanes write the rows.  The result depends
// on none of this: every stream is consumed strictly in order by exactly one lane.
#include "mi_common.h"
#include "kernels.h"
#include "philox.h"

namespace {

constexpr int kMaxWays = kDrawMaxWays, kMaxK = kDrawMaxK;
constexpr int kSel = kMaxK > kMaxWays ? kMaxK : kMaxWays;   // most entries one selection writes

// Ordered selection of k out of m without replacement, a Fisher-Yates shuffle of the identity that never materialises it:
// out[i] = a[j], a[j] = a[i] with j = i + bounded(m - i); the entries of `a` that differ from the identity are the list
// (opos, oval)[e * kMaxWays], at most k long, searched linearly (a[i] is looked up too: an earlier step may have landed on i).
__device__ void select_ordered(Philox& g, int k, uint32_t m, int* opos, int* oval, int* out) {
  int n = 0;
  for (int i = 0; i < k; ++i) {
    const int j = i + (int)g.bounded(m - (uint32_t)i);
    int aj = j, ai = i, ej = -1;
    for (int e = 0; e < n; ++e) {
      const int p = opos[e * kMaxWays];
      if (p == j) { aj = oval[e * kMaxWays]; ej = e; }
      if (p == i) ai = oval[e * kMaxWays];
    }
    out[i] = aj;
    if (ej < 0) { ej = n++; opos[ej * kMaxWays] = j; }
    oval[ej * kMaxWays] = ai;
  }
}

__global__ __launch_bounds__(64) void draw_tasks_kernel(const int32_t* __restrict__ class_offsets, const int32_t* __restrict__ class_index,
                                                        int n_classes, int ways, int k, const uint8_t* __restrict__ rot_table, int n_rot,
                                                        int remap_shuffle, uint64_t seed, uint64_t first_slot, uint64_t num_tasks,
                                                        int64_t* __restrict__ index_out, int64_t* __restrict__ labels_out,
                                                        uint8_t* __restrict__ rot_out, uint64_t* __restrict__ task_id_out) {
  __shared__ int opos[kSel * kMaxWays], oval[kSel * kMaxWays];   // override lists, entry-major: the lanes of a step touch consecutive words
  __shared__ int pick[2 * kMaxWays];                 // [0..ways): chosen classes, [kMaxWays..): their task labels
  __shared__ int turns[kMaxWays];
  __shared__ int spos[kMaxWays * kMaxK];             // sample positions, row-major [ways][k]
  const int lane = threadIdx.x;
  const uint64_t slot = first_slot + blockIdx.x;
  uint64_t tid = slot;
  if (num_tasks) tid = Philox(seed, slot, 0).bounded((uint32_t)num_tasks);
  if (lane == 0 && task_id_out) task_id_out[blockIdx.x] = tid;

  if (lane < 2) {
    Philox g(seed, tid, 1 + lane);
    const int kk = lane == 0 ? ways : (remap_shuffle ? ways : 0);
    select_ordered(g, kk, lane == 0 ? (uint32_t)n_classes : (uint32_t)ways, opos + lane, oval + lane, pick + lane * kMaxWays);
    if (lane == 1 && !remap_shuffle)
      for (int j = 0; j < ways; ++j) pick[kMaxWays + j] = j;
  }
  if (lane == 0) {                                   // ConsecutiveLabels: ascending original label = ascending class number
    for (int i = 1; i < ways; ++i) {
      const int v = pick[i];
      int p = i;
      for (; p > 0 && pick[p - 1] > v; --p) pick[p] = pick[p - 1];
      pick[p] = v;
    }
  } else if (lane == 2 && n_rot) {
    Philox g(seed, tid, 3);
    for (int j = 0; j < ways; ++j) turns[j] = rot_table[g.bounded((uint32_t)n_rot)];
  }
  __syncthreads();

  if (lane < ways) {
    const int c = pick[lane];
    Philox g(seed, tid, 16 + lane);
    select_ordered(g, k, (uint32_t)(class_offsets[c + 1] - class_offsets[c]), opos + lane, oval + lane, spos + lane * k);
  }
  __syncthreads();

  const int n2 = ways * k;
  const size_t row0 = (size_t)blockIdx.x * n2;
  for (int e = lane; e < n2; e += 64) {
    const int j = e / k;
    index_out[row0 + e] = class_index[class_offsets[pick[j]] + spos[e]];
    labels_out[row0 + e] = pick[kMaxWays + j];
    if (n_rot) rot_out[row0 + e] = (uint8_t)turns[j];
  }
}

}  // namespace

hipError_t launch_draw_tasks(hipStream_t st, const int32_t* class_offsets, const int32_t* class_index, int n_classes, int ways, int k,
                             const uint8_t* rot_table, int n_rot, int remap_shuffle, uint64_t seed, uint64_t first_slot,
                             uint64_t num_tasks, int tasks, int64_t* index_out, int64_t* labels_out, uint8_t* rot_out,
                             uint64_t* task_id_out) {
  hipLaunchKernelGGL(draw_tasks_kernel, dim3((unsigned)tasks), dim3(64), 0, st, class_offsets, class_index, n_classes, ways, k, rot_table,
                     n_rot, remap_shuffle, seed, first_slot, num_tasks, index_out, labels_out, rot_out, task_id_out);
  return hipGetLastError();
}
