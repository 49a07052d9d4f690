// The policy handle of the C ABI (mi_policy_create), shared by the files that implement entry points on it (policy.hip, rollout.hip).
#pragma once
#include "../../include/mi_maml.h"
#include <string>

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

struct mi_policy {
  mi_policy_desc d;
  int device;
  int S, A, H1, H2;
  int act;   // ACT_RELU / ACT_TANH between the dense layers (policies.py:32-37,76)
  size_t o_sigma, o_w1, o_b1, o_w2, o_b2, o_w3, o_b3, P;
  std::string err;
  unsigned* fold_counters = nullptr;   // device, one per 256-parameter block: arrival counters of the fold that also takes the mean over tasks
  bool fold_dirty = false;             // a counted fold was issued and not seen to launch cleanly: re-zero the counters before the next one
                                       // (policy_sweep.h FoldArgs::counter; zero between launches).  Allocated at the first fused product.
};

int mi_policy_fail(mi_policy* p, int code, const std::string& m);   // policy.hip: records the message on the handle and for the thread
