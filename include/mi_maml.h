/* mi_maml.h -- C ABI of the MI355X-native MAML/ANIL inner/outer-loop engine (libmi_maml.so).
 *
 * Drop-in boundary for the reference's hot path (Kostis-S-Z/exploring_meta).  The reference is pure Python with no FFI of
 * its own; each entry point below names the reference interface it replaces (file:line under /root/reference).  A
 * maintainer binds these with ctypes; exploring_meta_amd/_lib.py is that binding.
 *
 * Conventions: extern "C", plain pointers and sizes, no torch types.  Every function returns 0 on success and a negative
 * code on error; mi_last_error() returns a message for the last failing call on that engine (or the global message when
 * engine is NULL).  All tensor pointers are caller-owned DEVICE memory (fp32 unless noted), the engine keeps nothing
 * across calls except its model description; work is enqueued on `stream` (a hipStream_t passed as void*), stream
 * ordered, with no internal synchronisation.  One engine per device; a handle is not re-entrant.
 *
 * Parameter vectors ("theta", gradients) are FLAT fp32 vectors in the reference's `module.parameters()` order and
 * layouts: per ConvBlock  normalize.weight[C], normalize.bias[C], conv.weight[Co,Ci,3,3], conv.bias[Co]
 * (vision_models.py:168-186), then linear.weight[ways,F], linear.bias[ways] (vision_models.py:47,103).
 */
#ifndef MI_MAML_H
#define MI_MAML_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_ERR_ARG (-1)      /* invalid argument / unsupported shape */
#define MI_ERR_HIP (-2)      /* HIP runtime error */
#define MI_ERR_WORKSPACE (-3) /* workspace too small */

typedef struct mi_engine mi_engine;

/* Model family of core_functions/vision_models.py: ConvBase (:121-146) + optional classifier head.
 *   MiniImagenetCNN(ways)   (:66-118): {4, 3,84,84, 32, max_pool=1, ways, head_mean_pool=0}
 *   OmniglotCNN(ways)       (:10-63) : {4, 1,28,28, 64, max_pool=0, ways, head_mean_pool=1}
 *   ANIL trunk ConvBase(...)(anil_vision.py:86-91): ways=0 is not a classifier; see mi_anil_* below. */
typedef struct {
  int32_t n_layers;       /* ConvBlocks */
  int32_t in_channels, in_h, in_w;
  int32_t hidden;         /* filters per block (32 or 64) */
  int32_t max_pool;       /* 1: stride-1 conv + MaxPool2d(2,2,floor); 0: stride-2 conv, no pooling (vision_models.py:157-165) */
  int32_t ways;           /* classifier outputs, 1..64.  The head's gradient launch keeps a task's dlogits [n, ways] in LDS (n = rows per task,
                           * ways * shots in the meta-batch calls): first-order passes take n * ways <= 39424 (160 KiB of LDS: 5 ways n <= 7884,
                           * 8 ways 4928, 20 ways 1971, 64 ways 616), Hessian-vector (tangent) passes n * ways <= 19712 (5 ways n <= 3942, 8 ways
                           * 2464, 20 ways 985, 64 ways 308); a call beyond that returns MI_ERR_ARG naming n, ways and the bytes, and launches
                           * no head kernel */
  int32_t head_mean_pool; /* 1: x.mean(dim=[2,3]) then Linear(hidden,ways) (:53-54); 0: view(-1, hw*hidden) then Linear (:109) */
} mi_model_desc;

int mi_engine_create(const mi_model_desc* desc, int device, mi_engine** out);
void mi_engine_destroy(mi_engine* e);
const char* mi_last_error(const mi_engine* e);
const char* mi_version(void);

/* Ablation/test switch: 0 = block 1 through the generic (z-storing) kernels, 1 = fused conv-recompute kernels (default when
 * the geometry allows: Ci in {1,3}, stride-1 conv + pooling, even H/W) with the BatchNorm statistics of repeated support
 * passes taken from the input Gram matrix (mi_input_gram) and the BatchNorm-backward reductions from zhat kept at the pooling
 * argmax, 2 = fused kernels only: every statistic / reduction by a conv-recompute pass.  Since round 6 mode 1 also takes the QUERY pass of a
 * call with a backward half through a Gram matrix of the query images (formed on the engine's side stream beside the inner loop); 3 = as 1 with
 * the Gram matrix for the support passes only (the behaviour of rounds 2 - 5: the query pass by conv-recompute kernels). */
int mi_engine_set_fused_block1(mi_engine* e, int on);

/* 1 (default): the weight gradients of blocks >= 2 run on an engine-owned side stream, forked from the caller's stream once
 * dz of the block is written and joined before the pass's gradients are used (they are matrix-bound, the BatchNorm kernels
 * that follow on the main stream are HBM-bound).  0: every kernel on the caller's stream.  Any other value (default 1): one fork of the
 * side stream per hidden block.  (ONE fork per backward pass, the weight gradients issued together once the last hidden block's dz exists,
 * saved two event records per pass -- each idles the caller's stream for ~7 us -- but lost more overlap than that: +2.9 % on cfg2; removed.)
 * Results are identical in both modes (per-launch times from mi_profile_* are only additive with 0). */
int mi_engine_set_overlap(mi_engine* e, int on);

/* 1: a call of mi_meta_batch_maml / mi_meta_batch_anil whose arguments (every pointer, size and scalar, the stream included) equal
 * those of an earlier call on this engine is replayed as ONE hipGraphLaunch of the captured launch sequence (first sight of a
 * signature runs eagerly, the second is captured and instantiated; a small cache holds up to 8 signatures).  For callers that keep
 * their parameter / data / output / workspace buffers in place between meta-iterations (bench.py, the drivers): it removes the host
 * launch cost of the ~75-280 kernel launches of a call, which dominates the few-image configurations.  Default 0.  Results are
 * those of the eager call.  mi_profile_enable and mi_debug_set_trace suspend it for their calls. */
int mi_engine_set_graph(mi_engine* e, int on);

/* While buf != NULL every forward pass of mi_meta_batch_maml (inner steps 0..K-1, then the query pass) and the trunk pass of
 * mi_meta_batch_anil also writes the BatchNorm batch statistics of every block: buf [passes][tasks][2][C_total] floats (C_total = sum
 * of the blocks' filters, block-major; [0] batch mean, [1] biased batch variance).  torch.nn.BatchNorm2d updates running_mean /
 * running_var from these on every learner(x) of the reference (vision_models.py:168-174; the buffers are shared by learn2learn's clones
 * and saved by utils/experiment.py:85-90); core_functions/vision_models.py (running_stats_contribution / apply_running_stats) folds them in the reference's call order. */
/* Only the fused calls export (their passes are numbered from 0 per call); mi_forward_logits / mi_learner_* run with the export paused. */
int mi_engine_set_bn_export(mi_engine* e, float* buf, size_t floats);

/* 1 (default): the per-workgroup fp64 partials of every BatchNorm statistic / reduction are folded, in a fixed order, by the
 * last workgroup of the producing kernel (arrival counter per task); 0: by separate bn_finalize launches.  Bit-identical
 * results either way; the switch exists for ablation and tests. */
int mi_engine_set_fused_finalize(mi_engine* e, int on);

/* 1 (default): the BatchNorm-backward sums of a fused block 1 (dgamma, dbeta and, in the Hessian-vector product, their tangents) are
 * formed in the epilogue of block 2's dgrad kernel, whose output tile IS the cotangent of block 1's pooled output; 0: by a
 * separate streaming pass over the pooled-resolution tensors.  Same fp64 sums in another order (results agree to fp32 rounding). */
int mi_engine_set_fused_block1_reduce(mi_engine* e, int on);

/* Debug/test aid: byte offsets of {theta, g, xs, sup[0].p[0], sup[0].dp[0], sup[0].mu[0], sup[0].rstd[0], sup[0].p[1],
 * qry.p[0], total} inside the workspace of a mi_meta_batch_maml call with these sizes (out: 10 entries). */
int mi_debug_plan_offsets(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order, size_t* out);

/* Number of fp32 parameters (= sum(p.numel() for p in model.parameters())). */
int mi_param_count(const mi_engine* e, size_t* n);

/* Bytes of caller-provided scratch for one mi_meta_batch_* call with these sizes. */
int mi_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order, size_t* bytes);

/* One meta-batch of MAML tasks: replaces, for `tasks` tasks at once, the body of the reference's per-task loop
 *   learner = maml.clone(); fast_adapt(batch, learner, loss, adapt_steps, shots, ways, device); eval_loss.backward()
 * (vision/maml_vision.py:102-114; core_functions/vision.py:6-18; utils/data_pre.py:115-129; learn2learn MAML.clone/adapt)
 * with loss = CrossEntropyLoss(reduction='mean') (maml_vision.py:86).
 *   theta       [P]                      meta-parameters (read only)
 *   data        [tasks, 2*shots*ways, C, H, W]  NCHW fp32, exactly the reference's task batches stacked
 *   labels      [tasks, 2*shots*ways]    int64, as sampled by the reference (sorted by class)
 *   inner_lr    MAML(model, lr=...)      (maml_vision.py:84)
 *   second_order 1 = create_graph inner updates (the reference's hard-coded first_order=False), 0 = first-order MAML
 *   with_grad   0 = evaluation only (core_functions/vision.py:26-42 evaluate, and the validation half :117-124)
 * Outputs:
 *   loss_out    [tasks]  query loss per task          (valid_loss, vision.py:16)
 *   acc_out     [tasks]  query accuracy per task      (valid_accuracy, vision.py:17,21-23)
 *   meta_grad_out [P]    SUM over tasks of d valid_loss / d theta  (what .backward() accumulates, maml_vision.py:112);
 *                        the caller applies 1/meta_batch_size (:139-140).  May be NULL when with_grad == 0.
 *   logits_out  [tasks, shots*ways, ways] query predictions, or NULL. */
int mi_meta_batch_maml(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                       int tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order, int with_grad,
                       float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                       void* workspace, size_t workspace_bytes);

/* The train AND the validation half of one meta-iteration in the same launches.  The reference runs, per train task, a second
 *   learner = maml.clone(); fast_adapt(valid_batch, ...)        without backward
 * (vision/maml_vision.py:117-124): the K support steps and the query forward of those validation tasks are the same kernels as the
 * train tasks'.  `tasks` task batches are stacked as for mi_meta_batch_maml; the FIRST grad_tasks of them are train tasks -- query
 * backward, second-order adjoint recursion, summed into meta_grad_out -- the remaining tasks - grad_tasks are adapted and scored only.
 * loss_out / acc_out [tasks] cover both halves.  grad_tasks == tasks is mi_meta_batch_maml(with_grad = 1), grad_tasks == 0 is
 * with_grad = 0; the workspace is mi_workspace_bytes(tasks, ..., second_order). */
int mi_meta_batch_maml_tv(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                          int tasks, int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order,
                          float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                          void* workspace, size_t workspace_bytes);

/* mi_meta_batch_maml_tv with one inner-loop step size PER PARAMETER, optionally per inner step, and the gradient of the summed query
 * loss with respect to those step sizes (layer freezing = step 0, per-tensor steps, learn2learn MetaSGD's learnable steps).  With
 * D_k = diag(lr_k), lr_k = row (lr_steps == 1 ? 0 : k) of lr_vec:
 *   theta_{k+1} = theta_k - D_k g_k,                      g_k = grad L_support(theta_k)
 *   lam_K       = grad L_query(theta_K)
 *   second order:  lam_k = lam_{k+1} - H_k (D_k lam_{k+1})          first order:  lam_k = lam_K
 *   meta_grad   = sum_t lam_0           lr_grad_k = -sum_t g_k * lam_{k+1}   (lr_steps == 1: summed over k as well)
 *   lr_vec      [lr_steps, P]  device memory, the reference's parameter order; any finite value is a legal step (negative ones occur with
 *                              learnable steps).  The VALUES are read on the device by every call -- also by a graph replay: a caller may
 *                              update the buffer in place between calls.
 *   lr_steps    1 (one vector for every step) or adapt_steps (one per step; with adapt_steps == 0 only 1)
 *   lr_grad_out [lr_steps, P]  SUM over the grad_tasks train tasks, like meta_grad_out, or NULL.  fp32 products, summed over steps and
 *                              tasks in one fixed-order fp64 chain rounded once: bitwise reproducible from call to call.  Entries of a
 *                              step size that is 0 are in general NOT 0; conv-bias entries are exact zeros (g is).
 * Everything else as mi_meta_batch_maml_tv.  MI_ERR_ARG before any launch: lr_steps not 1 / adapt_steps, lr_vec NULL, lr_grad_out given
 * with grad_tasks == 0.  A uniform vector computes theta_k, the loss, accuracy and logits of the scalar call bit for bit, and its
 * first-order meta-gradient; the second-order recursion drives the Hessian-vector pass with D_k lam instead of scaling its result, which
 * is the same number only up to rounding unless the step is a power of two.  Launches: those of the scalar call + 1 (the step sizes into
 * engine layout) + 1 with lr_grad_out (fold and scatter); without the one-launch advance, second order, per inner step + 1 (the direction)
 * + 1 with lr_grad_out (the products).  Workspace: mi_workspace_bytes_lr. */
int mi_workspace_bytes_lr(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int second_order, int lr_steps,
                          int want_lr_grad, size_t* bytes);
int mi_meta_batch_maml_lr(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                          int tasks, int grad_tasks, int ways, int shots, int adapt_steps, const float* lr_vec, int lr_steps,
                          int second_order, float* loss_out, float* acc_out, float* meta_grad_out, float* lr_grad_out,
                          float* logits_out, void* workspace, size_t workspace_bytes);

/* mi_meta_batch_maml_tv (lr_vec NULL: the scalar step inner_lr) or mi_meta_batch_maml_lr (lr_vec, lr_steps as there) with the query set
 * scored at EVERY theta_j, j = 0..adapt_steps, inside the one call, and the multi-step loss of MAML++ (Antoniou et al., 2019) as the outer
 * objective:  J = sum_{t < grad_tasks} sum_{j = 1..K} step_w[j - 1] L_query,t(theta_j).  With q_j = grad L_query(theta_j):
 *   second order:  lam_K = w_K q_K,   lam_k = lam_{k+1} - H_k (D_k lam_{k+1}) + w_k q_k  (k = K-1..1),   lam_0 = lam_1 - H_0 (D_0 lam_1)
 *   first order:   lam_k = sum_{j >= max(k, 1)} w_j q_j
 *   meta_grad = sum_t lam_0,   lr_grad_k = -sum_t g_k * lam_{k+1}
 *   step_w           [adapt_steps]  device memory, fp32; theta_0 is scored but carries no weight.  Like lr_vec the VALUES are read on the
 *                                   device by every call, graph replays included: annealing the weights in place never recaptures.
 *   loss_steps_out   [adapt_steps + 1, tasks]   mean query loss at theta_j; acc_steps_out likewise
 *   logits_steps_out [adapt_steps + 1, tasks, ways * shots, ways] or NULL
 * The query passes at theta_j, j < K, make the launches of the final query pass with the same activation set and the same query Gram
 * matrix; train tasks take their backward half for j >= 1, validation tasks and j = 0 the forward half only, and with grad_tasks == 0 no
 * backward half runs.  They never write the BatchNorm export: mi_engine_set_bn_export sees the adapt_steps + 1 passes of the plain call.
 * The weighted terms are added as fmaf(w, q, x) behind the unchanged update expression: step_w = (0, .., 0, 1) returns the plain call's
 * last-step loss, accuracy, logits, meta_grad and lr_grad bit for bit.  MI_ERR_ARG before any launch: adapt_steps < 1, step_w NULL,
 * lr_grad_out without lr_vec, a debug trace being set, and what the plain calls refuse.  Workspace: mi_workspace_bytes_steps (lr_steps = 0
 * for the scalar step): the plain call's plan plus, with grad_tasks > 0, adapt_steps * tasks gradient-shaped vectors (the q_j). */
int mi_workspace_bytes_steps(const mi_engine* e, int tasks, int grad_tasks, int ways, int shots, int adapt_steps, int second_order,
                             int lr_steps, int want_lr_grad, size_t* bytes);
int mi_meta_batch_maml_steps(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                             int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps,
                             const float* step_w, int second_order, float* loss_steps_out, float* acc_steps_out, float* meta_grad_out,
                             float* lr_grad_out, float* logits_steps_out, void* workspace, size_t workspace_bytes);

/* The calls above with PER-STEP PARAMETER OFFSETS, shared by all tasks and meta-learned with the model: inner step k ends in
 *   theta_{k+1} = (theta_k - D_k g_k) + offsets[k]            k = 0..K-1   (D_k: the scalar step inner_lr, or row k of lr_vec)
 * MAML++'s per-step BatchNorm weights and biases (Antoniou et al., 2019) are the preset whose offsets are non-zero on the BatchNorm
 * tensors only, with those tensors' inner step sizes 0: theta_j then carries gamma + offsets[0] + .. + offsets[j-1].  The reference has
 * no counterpart.  The objective is the steps call's J = sum_{t < grad_tasks} sum_j step_w[j - 1] L_query,t(theta_j), or with step_w NULL
 * the plain L_query(theta_K).  The offset is additive, so d theta_{k+1} / d theta_k and with it the adjoint recursion are unchanged
 * (evaluated on the shifted trajectory), and lam_{k+1} is the total derivative of J with respect to theta_{k+1}:
 *   offsets_grad[k] = sum_{t < grad_tasks} lam_{k+1,t}         meta_grad and lr_grad keep their formulas
 *   offsets          [adapt_steps, P]  device memory, fp32, the reference's parameter order and layout; required.  Like lr_vec the VALUES
 *                                      are read on the device by every call, graph replays included: update the buffer in place.
 *   offsets_grad_out [adapt_steps, P]  or NULL; needs grad_tasks > 0.  Each row is one fixed-order fp64 chain over the train tasks, rounded
 *                                      once: bitwise reproducible.
 *   step_w           NULL: loss_out / acc_out [tasks], logits_out [tasks, ..] and the launches of mi_meta_batch_maml_tv / _lr;
 *                    else [adapt_steps] and the [adapt_steps + 1, tasks, ..] outputs of mi_meta_batch_maml_steps.
 *   lr_vec           NULL (the scalar inner_lr) or as in mi_meta_batch_maml_steps.
 * The finished element is u = a - step * g first, then (s == 0) ? u : u + s: with all offsets zero every output has the bits of the same
 * call without offsets, signed zeros included.  MI_ERR_ARG before any launch: adapt_steps < 1, offsets NULL, offsets_grad_out with
 * grad_tasks == 0, lr_grad_out without lr_vec, a debug trace being set, and what the calls above refuse.  Launches beyond the same call
 * without offsets: + 1 (the offsets into engine layout); with offsets_grad_out + adapt_steps (one fold per complete lam_{k+1}; a
 * first-order call without step_w: + 1, its lam is one constant); without the one-launch advance + adapt_steps more (the additions).
 * Workspace: mi_workspace_bytes_offsets (with_steps = step_w != NULL; lr_steps = 0 for the scalar step): the plan of the same call without
 * offsets plus adapt_steps parameter-shaped rows. */
int mi_workspace_bytes_offsets(const mi_engine* e, int tasks, int grad_tasks, int ways, int shots, int adapt_steps, int second_order,
                               int lr_steps, int want_lr_grad, int with_steps, size_t* bytes);
int mi_meta_batch_maml_offsets(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                               int grad_tasks, int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps,
                               const float* step_w, const float* offsets, int second_order, float* loss_out, float* acc_out,
                               float* meta_grad_out, float* lr_grad_out, float* offsets_grad_out, float* logits_out, void* workspace,
                               size_t workspace_bytes);

/* Ablation / test switch: 1 (default) = every pass of mi_meta_batch_maml ends in ONE "advance" launch (weight-gradient partial folds,
 * block 1's Gram-matrix assembly, p <- p - lr g of learn2learn's maml_update / the adjoint recursion, the next pass's Gram statistics);
 * 0 = the separate launches (reduce_partials x3, gram_wgrad, axpy, gram_stats, a memset).  Bit-identical results. */
int mi_engine_set_fused_tail(mi_engine* e, int on);

/* Ablation / test switch: 1 (default) = the LAST ConvBlock's BatchNorm + ReLU + MaxPool (core_functions/vision_models.py:188-193), the linear
 * head with its cross-entropy and accuracy (vision_models.py:109, core_functions/vision.py:11,16-18,21-23), the head's backward and that block's
 * BatchNorm-backward sums -- in the Hessian-vector passes their tangents -- run as ONE launch per pass, four workgroups (row groups) per task whose
 * sums meet in the last-arriving workgroup (csrc/tail.hip); 0 = the four separate launches per pass (bn_fwd, head rows, head grads,
 * bn_bwd_reduce).  Same arithmetic in the same order: the pooled output, logits, loss, accuracy, head gradients and feature cotangents are
 * bit-identical; the BatchNorm-backward sums are the same fp64 terms folded in a fixed order that no longer depends on the tasks per call.  Applies to nets whose last block is a generic (hidden -> hidden) block
 * feeding a flattened head (MiniImagenetCNN; not the mean-pooled OmniglotCNN head) outside the opt-in fp16 operand form. */
int mi_engine_set_fused_last_block(mi_engine* e, int on);
/* Debug aid (tools/tail_stamps.py): the 100 MHz wall clock at the stage boundaries of the one-launch tail, thread 0 of each of its four workgroups
 * per task: buf [tasks][4][16] 64-bit words of device memory, overwritten by every tail launch; NULL = off (the default). */
int mi_debug_tail_stamps(mi_engine* e, unsigned long long* buf);

/* One meta-batch of ANIL tasks (vision/anil_vision.py:116-122 with features = Sequential(ConvBase, view(-1, fc_neurons)),
 * head = MAML(Linear(fc_neurons, ways)), :86-94): the trunk runs once per task on all 2*shots*ways images (BatchNorm over
 * support and query together, utils/data_pre.py:118-119), only the head is adapted, and the outer gradient reaches both.
 * The engine is created with the trunk's ConvBase geometry and `ways`; theta / meta_grad_out are
 * [features.parameters() ..., head.weight[ways, fc_neurons], head.bias[ways]] -- the order of the reference's optimizer list
 * (anil_vision.py:97).  Other arguments as mi_meta_batch_maml. */
int mi_anil_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, size_t* bytes);
int mi_meta_batch_anil(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                       int tasks, int ways, int shots, int adapt_steps, float inner_lr, int second_order, int with_grad,
                       float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                       void* workspace, size_t workspace_bytes);

/* mi_meta_batch_anil with one inner-loop step size per HEAD parameter, optionally per inner step, and the gradient of the summed query
 * loss with respect to them (freezing the head's weight or bias = step 0, per-tensor steps, learnable steps); and the same call, scalar
 * or vector step, with the query set scored at EVERY theta_j and the multi-step loss as the outer objective.  Per task, phi = trunk,
 * theta = head (W, b), Ph = ways * fc_neurons + ways, D_k = diag(lr_k) with lr_k = row (lr_steps == 1 ? 0 : k) of lr_vec (scalar step:
 * D_k = inner_lr * I); the trunk runs once on all 2n images and is split into f_s, f_q as in mi_meta_batch_anil:
 *   theta_{k+1} = theta_k - D_k g_k,                      g_k = grad_theta L_s(theta_k; f_s)
 *   q_j = grad_theta L_q(theta_j; f_q),  dq_j = dL_q(theta_j)/df_q,     J = sum_t sum_{j = 1..K} w_j L_q,t(theta_j)
 *   second order:  lam_K = w_K q_K,   lam_k = lam_{k+1} - H_k (D_k lam_{k+1}) + w_k q_k  (k = K-1..1),   lam_0 = lam_1 - H_0 (D_0 lam_1)
 *                  df_s  = -sum_k R_{D_k lam_{k+1}}{ dL_s/df_s }(theta_k)
 *   first order:   lam_k = sum_{j >= max(k, 1)} w_j q_j,   df_s = 0
 *   df_q = sum_j w_j dq_j;   head part of meta_grad = sum_t lam_0;   trunk part = ONE trunk backward from the interleaved [df_s, df_q]
 *   lr_grad_k [Ph] = -sum_t g_k * lam_{k+1}          (lr_steps == 1: summed over k as well)
 * mi_meta_batch_anil_lr is the case w = (0, .., 0, 1) with the plain call's outputs.  The head tangent pass is driven with D_k lam and the
 * update is lam - 1 * (H dir), as in mi_meta_batch_maml_lr.
 *   lr_vec      [lr_steps, Ph]  device memory, the order of head.parameters(): weight [ways, fc_neurons] in the reference's
 *                               view(-1, fc_neurons) column order, then bias; the engine applies the column permutation it applies to
 *                               theta's head weight.  The VALUES are read on the device by every call, graph replays included.  An entry
 *                               whose step is exactly 0 keeps its parameter bit for bit.
 *   lr_steps    1 or adapt_steps (with adapt_steps == 0 only 1); 0 with lr_vec == NULL in the steps call (the scalar step inner_lr)
 *   step_w      [adapt_steps]   device memory, fp32, read on the device like lr_vec; theta_0 is scored but carries no weight
 *   lr_grad_out [lr_steps, Ph]  sum over the tasks, in lr_vec's order, or NULL.  fp32 products, one fixed-order fp64 chain over the
 *                               updates of a row ascending and the tasks ascending, rounded once: bitwise reproducible.
 *   loss_steps_out / acc_steps_out [adapt_steps + 1, tasks], logits_steps_out [adapt_steps + 1, tasks, ways * shots, ways] or NULL:
 *                               row j is what mi_meta_batch_anil writes with adapt_steps = j.
 * The head forward / backward / tangent launches are those of mi_meta_batch_anil; the elementwise work between them touches the head's
 * Ph entries per task, not the whole parameter vector.  A uniform lr_vec gives the plain call's loss, accuracy, logits and first-order
 * meta-gradient bit for bit, and its second-order one when the step is a power of two; step_w = (0, .., 0, 1) with the scalar step gives
 * the plain call in row adapt_steps and in meta_grad_out.  The BatchNorm export sees the one trunk pass.  MI_ERR_ARG before any HIP call:
 * lr_vec NULL in _lr, lr_steps not 1 / adapt_steps, lr_grad_out with with_grad == 0 or without lr_vec, step_w NULL or adapt_steps < 1 in
 * _steps, a debug trace being set, and what mi_meta_batch_anil refuses (a mean-pooled head; ways * shots beyond the head's LDS limits).
 * Launches on top of mi_meta_batch_anil's (K = adapt_steps), never a function of tasks: see DESIGN.md section 23.
 * Workspace: mi_anil_workspace_bytes_steps, one query for both entries (lr_steps = 0: scalar step; step_outputs 0: _lr, 1: _steps): the
 * plain plan at unchanged offsets, and behind it the step sizes in engine layout, the direction, the q_j, one dq and the products. */
int mi_anil_workspace_bytes_steps(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int with_grad, int second_order,
                                  int lr_steps, int want_lr_grad, int step_outputs, size_t* bytes);
int mi_meta_batch_anil_lr(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                          int ways, int shots, int adapt_steps, const float* lr_vec, int lr_steps, int second_order, int with_grad,
                          float* loss_out, float* acc_out, float* meta_grad_out, float* lr_grad_out, float* logits_out,
                          void* workspace, size_t workspace_bytes);
int mi_meta_batch_anil_steps(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels, int tasks,
                             int ways, int shots, int adapt_steps, float inner_lr, const float* lr_vec, int lr_steps, const float* step_w,
                             int second_order, int with_grad, float* loss_steps_out, float* acc_steps_out, float* meta_grad_out,
                             float* lr_grad_out, float* logits_steps_out, void* workspace, size_t workspace_bytes);

/* Metric heads: no inner loop at all.  The class vectors come from the support features in closed form (csrc/metric_head.hip, DESIGN.md
 * section 27), per task with N_w = #{i : ys_i = w}; THE CONTRACT IS N_w >= 1 FOR EVERY CLASS and labels in [0, ways):
 *   MI_METRIC_PROTO   (Prototypical Networks)  c_w = (1/N_w) sum_{i in w} fs_i,   z_qw = -scale * |fq_q - c_w|^2  (summed squared differences)
 *   MI_METRIC_COSINE  (NIL, the ANIL paper)    xh = x / max(|x|_2, 1e-8),  c_w = sum_{i in w} sh_i,   z_qw = scale * <qh_q, c_w>
 *   loss_t = mean_q CE(z_q, yq_q);  acc_t = mean_q [argmax_w z_q == yq_q] (first maximum);  dfs, dfq = d(sum_t loss_t)/d(fs, fq).
 * mi_metric_head is the kernel entry: fs [tasks, ns, feat], fq [tasks, nq, feat] fp32 (16-byte aligned, like dfs / dfq), ys [tasks, ns],
 * yq [tasks, nq] int32; ns != nq and unbalanced classes are fine.  loss, acc [tasks]; logits [tasks, nq, ways], dfs, dfq may be NULL (dfs and
 * dfq both NULL: the forward-only launch, whose loss, acc and logits are the bits of the forward + backward launch).  ONE launch whatever
 * `tasks`; a task's results do not depend on the other tasks of the call.  The domain (MI_ERR_ARG before any launch otherwise): tasks, ns,
 * nq, feat >= 1, 1 <= ways <= 64, metric one of MI_METRIC_*, scale > 0, and one task's class vectors and tables inside the 160 KiB of LDS:
 *   4 * (roundup4(ways * feat) + nq * ways + ways + ns + 4 * nq) <= 163840 bytes
 * -- ways * feat <= 40960 - (nq * ways + ways + ns + 4 * nq) rounded down to 4: 5 ways at ns = nq = 5: feat <= 8180 (at ns = nq = 25:
 * 8140); 20 ways x 1600 features (128 KB): nq * ways + ... leaves nq = ns <= 357; feat = 128, 5 ways: nq = ns <= 4031.
 * mi_metric_head_scratch_bytes: the kernel folds everything inside its launch and needs no scratch today: 0, and scratch may be NULL. */
#define MI_METRIC_PROTO 0
#define MI_METRIC_COSINE 1
size_t mi_metric_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways);
int mi_metric_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq,
                   int tasks, int ns, int nq, int feat, int ways, int metric, float scale,
                   float* loss, float* acc, float* logits /*nullable*/, float* dfs /*nullable*/, float* dfq /*nullable*/,
                   void* scratch, size_t scratch_bytes);
/* One meta-batch scored (and differentiated) by a metric head on the ANIL trunk: the engine is one made for mi_meta_batch_anil, theta and
 * meta_grad_out keep its layout [features.parameters() ..., head.weight, head.bias]; the head's entries of theta do not enter any result
 * and the head's entries of meta_grad_out are written as exact zeros.  data / labels as mi_meta_batch_anil (the even split of
 * utils/data_pre.py:118-119: ns = nq = ways * shots), logits_out [tasks, ways * shots, ways] or NULL.  The launches are mi_meta_batch_anil's
 * up to the split of the features, then ONE metric-head launch, then (with_grad) the interleave, the trunk backward and the sum over
 * tasks; without a gradient the call ends at the head, and its loss, acc and logits are the bits of the call with one (it keeps the
 * input Gram matrix that mi_meta_batch_anil drops from its evaluation call, whose block-1 statistics then round differently).  Graph replay and the BatchNorm export (one pass) as for
 * mi_meta_batch_anil; metric and scale are part of the graph's signature.  MI_ERR_ARG before any launch: a mean-pooled head, an unknown
 * metric, scale not > 0, sizes outside mi_metric_head's domain, and what mi_meta_batch_anil refuses. */
int mi_metric_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes);
int mi_meta_batch_metric(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                         int tasks, int ways, int shots, int metric, float scale, int with_grad,
                         float* loss_out, float* acc_out, float* meta_grad_out, float* logits_out,
                         void* workspace, size_t workspace_bytes);

/* Ridge-regression head (R2-D2, "Meta-learning with differentiable closed-form solvers"): the head's inner problem under a squared loss,
 * solved to optimality on the support features in the dual form and differentiated through the solve (csrc/ridge_head.hip, DESIGN.md
 * section 28).  Per task, Y = onehot(ys) [ns, ways], labels in [0, ways):
 *   G = fs fs^T + lam I,  A = G^-1 Y,  z = alpha * (fq fs^T) A;  loss_t = mean_q CE(z_q, yq_q);  acc_t = mean_q [argmax_w z_q == yq_q]
 *   (first maximum of the fp32 logits returned);  dfs, dfq = d(sum_t loss_t)/d(fs, fq);  dhyper[t] = (dloss_t/dlam, dloss_t/dalpha).
 * No additive logit bias: under softmax cross-entropy its gradient is identically zero.  A class without a support row is legal here (its
 * column of A is zero).  mi_ridge_head is the kernel entry: fs [tasks, ns, feat], fq [tasks, nq, feat] fp32 (16-byte aligned, like dfs /
 * dfq), ys [tasks, ns], yq [tasks, nq] int32; ns != nq and unbalanced classes are fine.  loss, acc [tasks]; logits [tasks, nq, ways], dfs,
 * dfq [as fs, fq] and dhyper [tasks, 2] may each be NULL, in any combination (dfs, dfq and dhyper all NULL: the forward-only launch, whose
 * loss, acc and logits are the bits of the forward + backward launch).  dhyper is per task, so that the sum over tasks is the caller's and
 * stays deterministic.  ONE launch whatever `tasks`; a task's results do not depend on the other tasks of the call.  The Gram system is
 * accumulated, factorised (G = L D L^T) and solved in fp64 in LDS.  A pivot that is not > 0 cannot occur for a sane lam (G is positive
 * definite); should it occur, every output of that task is NaN -- never a fault, never an endless loop.  The domain (MI_ERR_ARG naming
 * the sizes before any launch otherwise): tasks, ns, nq >= 1, 1 <= feat <= MI_RIDGE_MAX_FEAT (a stated cap: feat does not enter the LDS
 * request), 1 <= ways <= 64, lam and alpha > 0 and finite, and one task's tables inside the 160 KiB of LDS:
 *   8 * (ns (ns + 1) / 2 + nq * ns + 2 * ns * ways + ns + 3 * nq) + 4 * nq * ways <= 163840 bytes
 * -- ns = nq = 100 with 20 ways (Omniglot 20-way 5-shot) takes 163600; ns = nq = 25, 5 ways: 10900; ns = nq = 5, 5 ways: 980.
 * mi_ridge_head_scratch_bytes: the kernel folds everything inside its launch and needs no scratch today: 0, and scratch may be NULL. */
#define MI_RIDGE_MAX_FEAT 65536
size_t mi_ridge_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways);
int mi_ridge_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq,
                  int tasks, int ns, int nq, int feat, int ways, float lam, float alpha,
                  float* loss, float* acc, float* logits /*nullable*/, float* dfs /*nullable*/, float* dfq /*nullable*/,
                  float* dhyper /*nullable*/, void* scratch, size_t scratch_bytes);
/* One meta-batch scored (and differentiated) by the ridge head on the ANIL trunk: mi_meta_batch_metric's call with mi_ridge_head's launch
 * in the metric head's place -- the same engine, theta / meta_grad_out layout (the head's entries of theta are unused, those of
 * meta_grad_out exact zeros), data / labels, workspace plan, launches, graph replay and BatchNorm export; the evaluation call keeps the
 * input Gram matrix, so its loss, acc and logits are the bits of the call with a gradient.  dhyper_out [tasks, 2] or NULL: (dlam, dalpha)
 * per task, written only with a gradient.  The bits of lam and alpha are part of the graph's signature.  MI_ERR_ARG before any launch:
 * lam or alpha not > 0 or not finite, sizes outside mi_ridge_head's domain, and what mi_meta_batch_metric refuses. */
int mi_ridge_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes);
int mi_meta_batch_ridge(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                        int tasks, int ways, int shots, float lam, float alpha, int with_grad,
                        float* loss_out, float* acc_out, float* meta_grad_out, float* dhyper_out /*nullable*/, float* logits_out /*nullable*/,
                        void* workspace, size_t workspace_bytes);

/* Logistic-regression head: the head's inner problem under the loss ANIL's inner loop runs -- L2-regularised multinomial logistic regression
 * (softmax cross-entropy, no bias) on the support features -- solved to optimality and differentiated through the optimum by the implicit
 * function theorem (csrc/logreg_head.hip; LR-D2 of the R2-D2 paper for any number of classes, MetaOptNet's convex head).
 * Per task, Y = onehot(ys) [ns, ways], labels in [0, ways), in the dual form W = A^T fs:
 *   G = fs fs^T,  R(A) = lam A + softmax_rows(G A) - Y = 0  (one solution for lam > 0, also when G is singular),  z = alpha * (fq fs^T) A;
 *   loss_t = mean_q CE(z_q, yq_q);  acc_t = mean_q [argmax_w z_q == yq_q] (first maximum of the fp32 logits returned);
 *   dfs, dfq = d(sum_t loss_t)/d(fs, fq);  dhyper[t] = (dloss_t/dlam, dloss_t/dalpha).
 * A class without a support row is legal.  mi_logreg_head is the kernel entry, with mi_ridge_head's arguments and rules: fs [tasks, ns, feat],
 * fq [tasks, nq, feat] fp32 (16-byte aligned, like dfs / dfq), ys, yq int32; logits, dfs, dfq and dhyper [tasks, 2] may each be NULL, in any
 * combination (dfs, dfq and dhyper all NULL: the forward-only launch, whose loss, acc and logits are the bits of the forward + backward
 * launch).  ONE launch whatever `tasks`; a task's results do not depend on the other tasks of the call.  G, K, the solver and the backward
 * are fp64 in LDS; no intermediate is kept in fp32.
 * The solver: Newton from A = 0; each step solves (lam I + D G) dA = -R (D_i = diag(p_i) - p_i p_i^T, row-wise) through the symmetric
 * positive definite system lam I + C^T G C (D = C C^T) by conjugate gradients to |r| <= 1e-13 |b|; a step is accepted if it lowers |R|_inf, or,
 * while |R|_inf > 1e-10, if it meets Armijo's condition (1e-4) on the inner objective, else halved; the iteration stops at |R|_inf <= 1e-13, or
 * at |R|_inf <= 1e-10 when the step no longer lowers it.  Every rule is scale-free: features times 2 with lam times 4 gives loss, acc, logits
 * and dalpha bit for bit, dfs and dfq exactly halved, dlam exactly quartered.  The loops are bounded by the caps below (at least twice the
 * largest count over the tests' cases: 10 Newton steps, 52 CG steps, 1 halving) and leave at once on a residual that is not finite.  A task
 * that has not reached |R|_inf <= 1e-10 at the caps, whose residual is not finite, or whose backward solve has not met its tolerance gets NaN
 * in every output -- never a fault, never an endless loop; other tasks are untouched.  The domain (MI_ERR_ARG naming the sizes and the bytes
 * before any launch otherwise, the outputs untouched): tasks, ns, nq >= 1, 1 <= feat <= MI_RIDGE_MAX_FEAT, 1 <= ways <= 64, lam and alpha > 0
 * and finite, and one task's tables inside the 160 KiB of LDS:
 *   8 * (ns * ns + nq * ns + 10 * ns * ways + nq * ways + 2 * ns + 3 * nq + 32) <= 163840 bytes
 * -- ns = nq = 25, 5 ways: 22256; ns = nq = 20, 20 ways: 42656; ns = nq = 5, 5 ways: 3056.  (The ridge head's 100 x 100 x 20 is outside.)
 * mi_logreg_head_scratch_bytes: no scratch today: 0, and scratch may be NULL. */
#define MI_LOGREG_NEWTON_CAP 32
#define MI_LOGREG_CG_CAP 256
#define MI_LOGREG_HALVE_CAP 8
size_t mi_logreg_head_scratch_bytes(int tasks, int ns, int nq, int feat, int ways);
int mi_logreg_head(void* stream, const float* fs, const float* fq, const int32_t* ys, const int32_t* yq,
                   int tasks, int ns, int nq, int feat, int ways, float lam, float alpha,
                   float* loss, float* acc, float* logits /*nullable*/, float* dfs /*nullable*/, float* dfq /*nullable*/,
                   float* dhyper /*nullable*/, void* scratch, size_t scratch_bytes);
/* One meta-batch scored (and differentiated) by the logistic-regression head on the ANIL trunk: mi_meta_batch_ridge's call with
 * mi_logreg_head's launch in the ridge head's place (`logreg_head/0` in the profile) -- the same theta / meta_grad_out layout (the head's
 * entries of theta are unused, those of meta_grad_out exact zeros), workspace plan, launches, graph replay (the bits of lam and alpha are
 * part of the graph's signature) and dhyper_out [tasks, 2] or NULL, written only with a gradient.  MI_ERR_ARG before any launch: lam or
 * alpha not > 0 or not finite, sizes outside mi_logreg_head's domain, and what mi_meta_batch_metric refuses. */
int mi_logreg_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int with_grad, size_t* bytes);
int mi_meta_batch_logreg(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                         int tasks, int ways, int shots, float lam, float alpha, int with_grad,
                         float* loss_out, float* acc_out, float* meta_grad_out, float* dhyper_out /*nullable*/, float* logits_out /*nullable*/,
                         void* workspace, size_t workspace_bytes);

/* Proto-MAML head initialisation (Triantafillou et al., "Meta-Dataset", eq. 8; csrc/proto_init.hip): the linear head
 * whose logits are the Prototypical-Networks logits up to a per-row constant, derived per task from the support features, and its
 * backward.  Per task, N_w = #{i : ys_i = w}; THE CONTRACT IS N_w >= 1 FOR EVERY CLASS and labels in [0, ways), as for mi_metric_head (a
 * class without a support row gets W_0 = 0, b_0 = 0 and no gradient: never a fault, but not the definition):
 *   c_w = (1/N_w) sum_{i in w} fs_i,   W_0[w] = 2 scale c_w,   b_0[w] = -scale |c_w|^2
 *   2 scale <q, c_w> - scale |c_w|^2 = -scale |q - c_w|^2 + scale |q|^2
 * mi_proto_init: fs [tasks, ns, feat] fp32, ys [tasks, ns] int32; writes [W_0 (ways x feat, row w = class w) | b_0 (ways)] of task t at
 * head_out + t * head_stride (floats; head_stride >= ways * feat + ways).
 * mi_proto_init_bwd: lam_head, laid out like head_out at lam_stride, holds d objective / d (W_0, b_0) = (lamW, lamb);
 *   dc_w = 2 scale (lamW[w] - lamb[w] c_w),   dfs_i += dc_{ys_i} / N_{ys_i},   dscale[t] = sum_w (2 <lamW[w], c_w> - lamb[w] |c_w|^2)
 * dfs [tasks, ns, feat] is ACCUMULATED INTO (every element read, modified and written by the one thread that owns it); dscale [tasks] may be
 * NULL, which changes no other output.  It is per task, so that the sum over tasks is the caller's and stays deterministic.  c_w is
 * recomputed by the forward's code in the forward's order (nothing is kept between the two launches).
 * ONE launch each whatever `tasks`; a task's bits do not depend on `tasks`, on the workgroup that ran it, or on the alignment of the
 * pointers (16-byte accesses when feat % 4 == 0, the strides are multiples of 4 and the bases 16-byte aligned; words otherwise, same bits).
 * fp32 arithmetic on the elements; |c_w|^2 and dscale, the two sums over feat, are accumulated in fp64 in a fixed order and rounded once.
 * No float atomics.  The domain (MI_ERR_ARG naming the sizes before any launch otherwise, the outputs untouched): tasks, ns, feat >= 1,
 * feat <= MI_RIDGE_MAX_FEAT, 1 <= ways <= 64, scale > 0 and finite. */
int mi_proto_init(void* stream, const float* fs, const int32_t* ys, int tasks, int ns, int feat, int ways, float scale,
                  float* head_out, size_t head_stride);
int mi_proto_init_bwd(void* stream, const float* fs, const int32_t* ys, const float* lam_head, size_t lam_stride,
                      int tasks, int ns, int feat, int ways, float scale, float* dfs /*accumulated into*/, float* dscale /*[tasks], nullable*/);
/* Proto-MAML on the ANIL trunk: mi_meta_batch_anil_lr / _steps with theta_0's head of every task derived from its support prototypes by
 * mi_proto_init's kernel, and differentiated through -- the inner loop, the adjoint recursion, the step sizes and the multi-step loss are
 * those calls', with two launches added: the initialisation after the split of the features, and (with_grad) its backward between the
 * adjoint recursion and the interleave, which adds dfs through theta_0 on top of the loop's own and writes dscale_out.
 *   theta_0^head = (2 s c, -s |c|^2);  theta_{k+1} = theta_k - D_k g_k;  objective = L_q(theta_K), or sum_j step_w[j-1] L_q(theta_j)
 *   lam_0 = d objective / d theta_0^head (what the adjoint recursion leaves);  first order keeps theta_0's dependence on fs: lam_0 = sum_j
 *   w_j q_j, only the g_k are constants.
 * Every combination is one entry: lr_vec NULL = the scalar step inner_lr, else [lr_steps, Ph] as in mi_meta_batch_anil_lr (lr_grad_out
 * likewise); step_w NULL = the plain outputs loss_out / acc_out [tasks], logits_out [tasks, ways * shots, ways]; step_w [adapt_steps] = the
 * per-step outputs [adapt_steps + 1, tasks(, ..)] of mi_meta_batch_anil_steps, row 0 being the Prototypical-Networks score of the query
 * set.  adapt_steps = 0 without step_w is Prototypical Networks (loss, accuracy and trunk gradient of mi_meta_batch_metric(MI_METRIC_PROTO,
 * scale) up to rounding; the logits differ by scale |q|^2 per row).  The head's entries of theta enter no result; the head's entries of
 * meta_grad_out are written as exact zeros.  dscale_out [tasks] or NULL: d objective_t / d scale, written only with a gradient.  The bits
 * of scale are part of the graph's signature.  The profile shows the launches as proto_init/0 and proto_init/1.  MI_ERR_ARG before any
 * launch: scale not > 0 or not finite, dscale_out with with_grad == 0, step_w with adapt_steps < 1, a debug trace being set, sizes outside
 * mi_proto_init's domain, and what mi_meta_batch_anil_steps refuses.  Workspace: mi_anil_proto_workspace_bytes, the arguments of
 * mi_anil_workspace_bytes_steps (lr_steps = 0 with step_outputs = 0 is legal here). */
int mi_anil_proto_workspace_bytes(const mi_engine* e, int tasks, int ways, int shots, int adapt_steps, int with_grad, int second_order,
                                  int lr_steps, int want_lr_grad, int step_outputs, size_t* bytes);
int mi_meta_batch_anil_proto(mi_engine* e, void* stream, const float* theta, const float* data, const int64_t* labels,
                             int tasks, int ways, int shots, int adapt_steps, int second_order,
                             float inner_lr, const float* lr_vec /*nullable*/, int lr_steps, const float* step_w /*nullable*/,
                             float scale, int with_grad,
                             float* loss_out, float* acc_out, float* meta_grad_out, float* lr_grad_out /*nullable*/,
                             float* dscale_out /*[tasks], nullable*/, float* logits_out /*nullable*/, void* workspace, size_t workspace_bytes);

/* Plain classifier forward, no adaptation: `learner(x)` / `model(x)` (vision_models.py:51-55,107-110), BatchNorm in train
 * mode over the n images of each of the `tasks` batches.  x [tasks, n, C, H, W] NCHW; logits_out [tasks, n, ways]. */
int mi_forward_workspace_bytes(const mi_engine* e, int tasks, int n, size_t* bytes);
int mi_forward_logits(mi_engine* e, void* stream, const float* theta, const float* x, int tasks, int n, float* logits_out,
                      void* workspace, size_t workspace_bytes);

/* Step-wise learner: the reference's `learner = maml.clone(); learner(x); learner.adapt(loss); learner.get_rep_i(x, i)`
 * (misc_scripts/cl_vision.py:56-66, misc_scripts/rc_vision.py:66-86, core_functions/maml.py:15-19,
 * core_functions/vision_models.py:57-63,112-118) with the fast weights held by the caller.
 *   theta [theta_tasks, P]  reference parameter order; theta_tasks = 1 (all task batches share theta) or = tasks
 *   x     [tasks, n, C, H, W] NCHW; BatchNorm in train mode over the n images of each task batch
 * mi_learner_forward:  logits_out [tasks, n, ways] (or NULL); rep_out (or NULL) = output of the first `rep_layer` ConvBlocks,
 *   rep_layer in 1..layers, NCHW [tasks, n, hidden, h', w'] (`Sequential(*base.children()[:layer])(x)`; layers = base(x)).
 * mi_learner_backward: grad_out [theta_tasks, P] = d sum(logits * dlogits) / d theta (summed over task batches when theta
 *   is shared): the vector-Jacobian product autograd asks of `learner(x)`; conv biases get exact zeros (batch-stat BN).
 *   Its own derivative is mi_learner_hvp; the fused second-order path is mi_meta_batch_maml.
 * Workspace: mi_forward_workspace_bytes(e, tasks, n). */
int mi_learner_forward(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x, int tasks, int n,
                       float* logits_out, int rep_layer, float* rep_out, void* workspace, size_t workspace_bytes);
int mi_learner_backward(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x, const float* dlogits,
                        int tasks, int n, float* grad_out, void* workspace, size_t workspace_bytes);

/* Double backward of the step-wise learner (learn2learn `MAML.adapt` of a second-order learner differentiates through
 * `grad(loss, params, create_graph=True)`, learn2learn maml.py adapt / maml_update; driven step-wise at misc_scripts/rc_vision.py:67-70).
 * With s(theta) = sum(logits(theta) * dlogits) and g = ds/dtheta (mi_learner_backward), for a cotangent v [theta_tasks, P] on g:
 *   grad_theta_out [theta_tasks, P] = (d^2 s / dtheta^2) v with dlogits held fixed (forward-over-reverse sweep),
 *   logits_dot_out [tasks, n, ways] = J(theta) v  -- the vector-Jacobian product with respect to dlogits.
 * Workspace: mi_learner_hvp_workspace_bytes(e, tasks, n). */
int mi_learner_hvp_workspace_bytes(const mi_engine* e, int tasks, int n, size_t* bytes);
int mi_learner_hvp(mi_engine* e, void* stream, const float* theta, int theta_tasks, const float* x, const float* dlogits,
                   const float* v, int tasks, int n, float* grad_theta_out, float* logits_dot_out, void* workspace,
                   size_t workspace_bytes);

/* One recurrence of cherry.algorithms.trpo.conjugate_gradient (reference rl.py:418, the loop body) on device vectors, fp64, one launch:
 *   alpha = rr[0] / (p . ap + eps);  x += alpha p;  r -= alpha ap;  rr_new = r . r;  p = r + (rr_new / rr[0]) p;  rr[0] = rr_new, rr[1] = alpha.
 * x, r, p: fp64 [n];  ap: fp32 [n] (the Fisher-vector product of p32);  p32: fp32 [n], the new p for the next product. */
int mi_cg_update(void* stream, double* x, double* r, double* p, const float* ap, double* rr, float* p32, size_t n, double eps);
/* The same with the reference's convergence test `if r_dot_new < tol: break` (cherry conjugate_gradient, rl.py:418) taken on the device:
 * rr is [3] (rr[2] = 0 on entry of a solve); once rr_new < tol, rr[2] latches to 1 and every later call of the solve leaves x, r, p, p32
 * untouched -- the host loop runs its fixed number of iterations without synchronising, x is exactly the x at the break. */
int mi_cg_update_checked(void* stream, double* x, double* r, double* p, const float* ap, double* rr, float* p32, size_t n, double eps,
                         double tol);

/* The start of that solve as one launch: r = p = b (fp64), x = 0, p32 = b, rr = (b . b, 0, 0)  (rl.py:418; cherry's conjugate_gradient
 * begins with x = 0, r = p = b). */
int mi_cg_init(void* stream, const float* b, double* x, double* r, double* p, float* p32, double* rr, size_t n);

/* The trust-region step from the solve's direction and its Fisher-vector product (reference rl.py:419-421), one launch:
 *   shs = 0.5 step . fstep (summed in fp64);  lagrange = sqrt(shs / max_kl);  out = step / lagrange;  *lagrange_out = lagrange (or NULL).
 * A negative shs yields NaN, as in the reference. */
int mi_trpo_scale_step(void* stream, const float* step, const float* fstep, size_t n, float max_kl, float* out, float* lagrange_out);

/* Generalised advantage estimation with cherry's LinearValue baseline for a list of replays, one launch (reference
 * core_functions/rl.py:95-110 compute_advantages: ch.td.discount, LinearValue.fit / __call__ (features [s, s^2, t, t^2, t^3, 1],
 * t = row/100, ridge normal equations with `reg`; rl/maml_trpo.py:85 passes env.action_size as reg), bootstraps,
 * cherry.pg.generalized_advantage; normalize != 0 applies ch.normalize (rl.py:355) -- (adv - mean) / (unbiased std + 1e-8)).
 *   states, next_states [replays, rows, state_dim]; rewards, dones [replays, rows]; count [replays] rows in use (NULL = rows);
 *   adv_out [replays, rows] (0 past a replay's count); weight_out [replays, 2*state_dim+4] fitted baseline weights (fp64) or NULL;
 *   weight_in [replays, 2*state_dim+4] != NULL: use these baseline weights instead of fitting (compute_advantages' update_vf=False,
 *   rl.py:401 -- the query replay's loss is computed with the baseline fitted to the last support replay).
 * fp64 arithmetic throughout; state_dim <= 8 and rows <= mi_gae_max_rows(state_dim) (the replay is staged in LDS). */
int mi_gae_max_rows(int state_dim);
int mi_gae_advantages(void* stream, const float* states, const float* next_states, const float* rewards, const float* dones,
                      const int32_t* count, const double* weight_in, int replays, int rows, int state_dim, double gamma, double tau,
                      double reg, int normalize, float* adv_out, double* weight_out);

/* Assembly of a padded device batch from a list of contiguous fp32 device arrays -- the fields of the replays a meta-iteration collected
 * (reference core_functions/rl.py:444-465 walks them task by task, replay by replay) and the parameters of the stored adapted policies
 * (rl.py:447-449): segment k copies nfloat[k] floats from src[k] to dst[k] and writes zeros up to npad[k] (>= nfloat[k]) floats.
 * src, dst, nfloat, npad are HOST arrays of nseg entries holding DEVICE pointers; the pointers travel in kernel arguments, one launch per
 * 128 segments. */
int mi_copy_segments(void* stream, const void* const* src, void* const* dst, const uint32_t* nfloat, const uint32_t* npad, int nseg);
/* n int32 values from HOST memory to the device array dst, carried in kernel arguments (512 per launch): the per-replay row counts of
 * the batch above without a staging copy. */
int mi_upload_i32(void* stream, int32_t* dst, const int32_t* host_values, int n);

/* Adam step on the flat meta-parameters with torch.optim.Adam defaults (maml_vision.py:85,139-141):
 * grad is first scaled by grad_scale (= 1/meta_batch_size). step is the 1-based step count after increment. */
int mi_adam_step(void* stream, float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, int step,
                 float lr, float beta1, float beta2, float eps, float grad_scale);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-kernel entry points (unit parity tests against oracle/kernels_ref.py).  Engine-internal layouts:
 * activations NHWC [tasks, N, H, W, C]; conv weights tap-major [9, Ci, Co]; all per-task parameter pointers advance by
 * `pstride` floats per task. */

/* utils/data_pre.py:115-129 prepare_batch: even rows -> support, odd rows -> query, NCHW -> NHWC, labels -> int32. */
int mi_prepare_batch(void* stream, const float* data, const int64_t* labels, int tasks, int n2, int c, int h, int w,
                     float* xs, float* xq, int32_t* ys, int32_t* yq);

/* Block-1 statistics without running conv1 (gram.hip): conv1's output is linear in its weights, so BatchNorm's per-channel
 * sums are quadratic forms of G = P^T P, P = the zero-padded 3x3xCi patches of the images (+ a constant-one column).
 *   mi_input_gram: x [tasks,n,H,W,ci] NHWC (ci = 1 or 3) -> g_out [tasks, NG, NG] fp64, NG = 32 (ci=3) / 16 (ci=1);
 *     entry (a, b) for a,b < 9ci = sum over pixels of patch_a * patch_b (a = tap*ci + c), row/column 9ci = the patch sums.
 *   mi_gram_bn_stats: w9d == NULL -> out0 = mean, out1 = 1/sqrt(biased var + eps) of conv3x3(x, w9) over `pixels` = n*H*W
 *     positions (what mi_conv3x3_bn_stats finalises); w9d != NULL -> out0 = mean(zd), out1 = mean(zhat * zd) for the tangent
 *     zd = conv3x3(x, w9d), zhat = (z - mu) * rstd (the statistics of the tangent BatchNorm). */
size_t mi_input_gram_scratch_bytes(int tasks, int n, int h, int ci);
int mi_input_gram(void* stream, const float* x, int tasks, int n, int h, int w, int ci, void* scratch, size_t scratch_bytes,
                  double* g_out);
int mi_gram_bn_stats(void* stream, const double* g, int tasks, int ci, int co, const float* w9, size_t pstride, const float* w9d,
                     size_t vstride, int pixels, float* out0, float* out1, const float* mu, const float* rstd);

/* Centred kernel alignment of layer representations (reference utils/cka.py:9-60; the CKA calls the reference leaves commented
 * out in misc_scripts/rc_vision.py:89-91, on the [c*h*w, b] reshape of rc_vision.py:150-165), computed without any n x n matrix
 * (cka.hip).  x, y: fp32 [pairs][n][p] row-major, rows = points; 1 <= p <= 128, 2 <= n <= 2^18, pairs >= 1 (MI_ERR_ARG otherwise,
 * before any HIP call; the scratch size is 0 then).  sigma > 0: fixed bandwidth for every matrix; sigma <= 0: the median heuristic
 * per matrix (sigma^2 = median of the nonzero squared distances, numpy's rule).  out: fp64 [pairs][4] = {linear_cka, kernel_cka,
 * sigma_x, sigma_y}, device memory; degenerate inputs give NaN as numpy does.  Scratch is O(pairs (n + p^2)); results are
 * bitwise reproducible and do not depend on how many pairs share the call. */
size_t mi_cka_scratch_bytes(int pairs, int n, int p);
int mi_cka(void* stream, const float* x, const float* y, int pairs, int n, int p, double sigma,
           void* scratch, size_t scratch_bytes, double* out);

/* Canonical correlation analysis of layer representations: the SVCCA measure the reference's representation-change study runs and
 * writes to cca_results.json (reference utils/cca.py:226-362, compute_ccas :104-174, remove_small :69-101, sum_threshold :177-195;
 * called as get_cca_similarity(adapted_rep.T, init_rep.T, epsilon=1e-10)[1] in misc_scripts/rc_vision.py:84-88 and rc_rl.py:276).
 * x, y: fp32 [pairs][n][p] row-major, rows = datapoints, columns = neurons, the same p on both sides; 1 <= p <= 64,
 * 2 <= n <= 2^18, 1 <= pairs <= 2^20, epsilon >= 0, 0 <= threshold <= 1 (MI_ERR_ARG otherwise, before any HIP call; the scratch
 * size is 0 for an unsupported shape).  Per pair, in fp64 (cca.hip): covariance blocks, each scaled by its largest magnitude;
 * neuron i of a side is kept iff its scaled variance is >= epsilon; epsilon is added to both diagonals; inverse square roots by
 * Jacobi eigen-decomposition with the pseudo-inverse rule (|w_i| <= 1e-15 max|w| contributes 0, every other eigenvalue
 * |w_i|^(-1/2)); the singular values of Sxx^(-1/2) Sxy Syy^(-1/2) by one-sided Jacobi.
 * coefs: fp64 [pairs][p], the canonical correlations in descending order in the first `count` slots, NaN after them.
 * stats: fp64 [pairs][8] = {mean, thresholded_mean, sum, count, kept_x, kept_y, cond_x, cond_y}: count = min(kept_x, kept_y);
 * thresholded_mean = mean of the first idx coefficients, idx the first i in [0, count) with sum(s[:i]) / sum(s) >= threshold (all
 * of them if there is none); cond_* = max|w| / min|w| of the block as it enters the inverse, inf if the smallest eigenvalue is cut.
 * Either side keeps no neuron (a constant matrix, for every epsilon): mean = thresholded_mean = sum = count = 0, every
 * coefficient NaN, cond_* NaN.  A singular block with epsilon = 0 gives the finite value of the pseudo-inverse rule (the reference
 * does not return there).  On return the scratch begins with the kept masks, uint64 [pairs][2] (X, Y; bit i = neuron i kept),
 * followed at the next multiple of 256 bytes by int32 [pairs][4] = {sweeps of the X and the Y eigen-problem, sweeps of the
 * singular-value iteration, 1 if a sweep cap was reached}.  Results are bitwise reproducible and do not depend on how many pairs
 * share the call; the number of launches does not depend on pairs either. */
size_t mi_cca_scratch_bytes(int pairs, int n, int p);
int mi_cca(void* stream, const float* x, const float* y, int pairs, int n, int p, double epsilon, double threshold,
           void* scratch, size_t scratch_bytes, double* coefs, double* stats);

/* Device-to-device streaming copy (bytes % 16 == 0): the kernel bench.py uses to measure the achievable HBM bandwidth in the
 * same run as the engine kernels ("measured HBM roofline"). */
int mi_stream_copy(void* stream, const void* src, void* dst, size_t bytes);

/* Task sampling from a dataset resident in HBM: `tasks.sample()` of learn2learn's TaskDataset with LoadData
 * (utils/data_pre.py:16-112; call sites vision/maml_vision.py:103,116) for a whole meta-batch, no host pixel traffic.
 *   dataset [num_images, C, H, W]  fp32, or uint8 when dataset_is_u8 (raw 0..255 pixels, converted exactly)
 *   index   [tasks, n2] int64      image ids drawn on the host (NWays / KShots(2*shots) / ConsecutiveLabels order), each in
 *                                  [0, num_images) -- the caller guarantees the range, the kernel does not check it
 *   rot     [tasks, n2] uint8      quarter turns counter-clockwise per row (RandomClassRotation, data_pre.py:34), or NULL
 *   data_out [tasks, n2, C, H, W]  exactly the stacked task batches mi_meta_batch_maml / _anil take */
int mi_sample_tasks(void* stream, const void* dataset, int dataset_is_u8, size_t num_images, int c, int h, int w,
                    const int64_t* index, const uint8_t* rot, int tasks, int n2, float* data_out);

/* The draw that precedes mi_sample_tasks, on the device: the task transforms of utils/data_pre.py:16-112 (FilterLabels, NWays,
 * KShots(2*shots), RemapLabels, ConsecutiveLabels, RandomClassRotation, num_tasks) for `tasks` tasks in one launch, with no host
 * arrays, copies or synchronisation.  A task is a pure function of (seed, task id): Philox4x32-10, key = seed, counter =
 * (id_lo, id_hi, stream, block), Lemire's bounded integers and an ordered Fisher-Yates selection, all in integer arithmetic
 * (exploring_meta_amd.utils.task_sampler.TaskSampler.describe_task is the numpy restatement, equal bit for
 * bit).  Slot first_slot + t becomes task id bounded(num_tasks) on stream 0 of the slot, or the slot itself when num_tasks == 0;
 * the result does not depend on `tasks` or on which other slots share the launch.
 *   class_offsets [n_classes + 1] int32   the eligible classes in ascending original label: class c owns
 *   class_index   [class_offsets[n_classes]] int32   class_index[class_offsets[c] .. class_offsets[c + 1]), ascending image ids
 *   rot_table     [n_rot] uint8           quarter turns to choose from per class and task; n_rot == 0: no rotations
 *   index_out, labels_out [tasks, ways * k] int64, rot_out [tasks, ways * k] uint8 (NULL iff n_rot == 0): the layout
 *                                         mi_sample_tasks and the engine take;  task_id_out [tasks] uint64 or NULL
 * 1 <= ways <= min(32, n_classes), 1 <= k <= 64, 0 <= n_rot <= 256, num_tasks < 2^32, tasks >= 1 (MI_ERR_ARG otherwise, before any
 * HIP call).  The tables are trusted: every class must hold at least k images (the caller checks, the kernel does not). */
int mi_draw_tasks(void* stream, const int32_t* class_offsets, const int32_t* class_index, int n_classes, int ways, int k,
                  const uint8_t* rot_table, int n_rot, int remap_shuffle, uint64_t seed, uint64_t first_slot, uint64_t num_tasks,
                  int tasks, int64_t* index_out, int64_t* labels_out, uint8_t* rot_out, uint64_t* task_id_out);

/* conv3x3 pad 1 (ConvBlock.conv, vision_models.py:177-185, bias dropped: batch-stat BN cancels it) + per-channel
 * sum / sum-of-squares partials; then finalize -> mu, rstd (BatchNorm2d train mode, eps 1e-5, biased variance). */
int mi_conv3x3_bn_stats(void* stream, const float* x, const float* w9, size_t pstride, int tasks, int n, int h, int wd,
                        int ci, int co, int stride, float* z, float* mu, float* rstd, void* scratch, size_t scratch_bytes);
/* BN-apply + ReLU + MaxPool2d(2,2) (or identity). */
int mi_bn_relu_pool(void* stream, const float* z, const float* mu, const float* rstd, const float* gamma, const float* beta,
                    size_t pstride, int tasks, int n, int ho, int wo, int c, int pool, float* p);
/* backward of BN+ReLU+pool: dgamma, dbeta, dz. */
int mi_bn_relu_pool_bwd(void* stream, const float* z, const float* mu, const float* rstd, const float* gamma, const float* beta,
                        size_t pstride, const float* dp, int tasks, int n, int ho, int wo, int c, int pool,
                        float* dgamma, float* dbeta, size_t gstride, float* dz, void* scratch, size_t scratch_bytes);
/* conv backward: dx = dgrad(dz, w9) (may be NULL), dw9 = wgrad(x, dz). */
int mi_conv3x3_bwd(void* stream, const float* x, const float* dz, const float* w9, size_t pstride, int tasks, int n, int h,
                   int wd, int ci, int co, int stride, float* dx, float* dw9, size_t gstride, void* scratch, size_t scratch_bytes);
/* Linear + CrossEntropy(mean) forward/backward on features f [tasks, n, F]. */
int mi_head_fwd_bwd(void* stream, const float* f, const float* wl, const float* bl, size_t pstride, const int32_t* y,
                    int tasks, int n, int feat, int ways, float* loss, float* acc, float* logits, float* prob, float* dl,
                    float* dwl, float* dbl, size_t gstride, float* df);
size_t mi_kernel_scratch_bytes(int tasks, int n, int h, int w, int c);
/* The head's backward alone, from given dlogits dl [tasks, n, ways]: dwl, dbl, df (may be NULL). */
int mi_head_grads(void* stream, const float* f, const float* wl, size_t pstride, const float* dl, int tasks, int n, int feat,
                  int ways, float* dwl, float* dbl, size_t gstride, float* df);
/* Tangent (R-operator) of the head along the direction (wld, bld) [+ the feature tangent fd, may be NULL]:
 *   ld = fd wl^T + f wld^T + bld (-> ld_out, may be NULL);  R{dl} = prob * (ld - sum(prob * ld)) / n  (-> rdl; fixed_dl != 0: dl is a given
 *   cotangent, R{dl} = 0 and prob is not read);  dwl = R{dl}^T f + dl^T fd,  dbl = sum_n R{dl},  df (may be NULL) = R{dl} wl + dl wld. */
int mi_head_tangent(void* stream, const float* f, const float* fd, const float* wl, const float* bl, size_t pstride,
                    const float* wld, const float* bld, size_t vstride, const float* prob, const float* dl, float* rdl,
                    float* ld_out, int fixed_dl, int tasks, int n, int feat, int ways, float* dwl, float* dbl, size_t gstride,
                    float* df);
/* OmniglotCNN's x.mean(dim=[2,3]): p [rows, hw, c] -> f [rows, c], and its backward df -> dp = df / hw at every position. */
int mi_spatial_mean(void* stream, const float* p, float* f, int rows, int hw, int c);
int mi_spatial_mean_bwd(void* stream, const float* df, float* dp, int rows, int hw, int c);

/* The one-launch tail of a pass (csrc/tail.hip): the last block's BatchNorm + ReLU + MaxPool, the head with loss and accuracy, the head's
 * backward and that block's BatchNorm-backward sums -- tangent != 0: their tangents.  mi_tail_supported: the shapes the kernel takes
 * (feat = hp * wp * c); mi_tail_lds_bytes: the dynamic LDS of a launch (the tangent kernel's is held to 150 KiB).
 * All per-task vectors of theta / the direction / the gradients advance by pstride / vstride / gstride floats, multiples of 4.
 * Scratch (mi_tail_scratch_bytes) starts with `tasks` 32-bit arrival counters that the CALLER zeroes once; every launch leaves them at zero. */
typedef struct {
  const float *z, *zd;                  /* conv output [tasks, n, ho, wo, c] and (tangent) its tangent */
  const float *mu, *rstd, *m1, *m2;     /* [tasks, c]; m1, m2 tangent only */
  const float *gamma, *beta, *wl, *bl; size_t pstride;          /* BatchNorm and head parameters */
  const float *gammad, *betad, *wld, *bld; size_t vstride;      /* the direction's (tangent) */
  const int32_t* y;                     /* [tasks, n] labels (primal) */
  const float *f, *dp;                  /* tangent: the primal pass's pooled output and its cotangent (= the primal df) */
  float *prob, *dl;                     /* [tasks, n, ways]: written by the primal pass, read by the tangent pass */
  float *pooled;                        /* [tasks, n, hp, wp, c]: p (tangent: its tangent) */
  float *loss, *acc, *logits;           /* primal: [tasks], [tasks], [tasks, n, ways] (logits may be NULL) */
  float *dwl, *dbl, *sum0, *sum1; size_t gstride;               /* head gradients, dgamma, dbeta (tangent: their tangents) */
  float *df;                            /* [tasks, n, feat] */
  int32_t tasks, n, ho, wo, c, pool, ways;
  int32_t with_grad, bwd_tasks;         /* primal: 0 = loss and accuracy only; tasks >= bwd_tasks stop after the loss */
} mi_tail_args;
int mi_tail_supported(int n, int ho, int wo, int c, int pool, int feat, int ways);
size_t mi_tail_lds_bytes(int n, int feat, int ways, int tangent);
size_t mi_tail_scratch_bytes(int tasks, int n, int ho, int wo, int c, int pool, int ways);
int mi_tail_run(void* stream, const mi_tail_args* a, int tangent, void* scratch, size_t scratch_bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Tangent (R-operator) and fused block-1 kernels: unit-test entry points (tests/test_gpu_tangent_kernels.py).  They are the
 * kernels behind the second-order path -- the double-backward of ConvBlock.forward (vision_models.py:188-193) that the
 * reference gets from autograd with create_graph=True (learn2learn MAML.adapt, call site core_functions/vision.py:13). */

/* zd = conv3x3(x0, w0) [+ conv3x3(x1, w1) when x1 != NULL]  with the tangent-BatchNorm statistics
 *   m1 = mean(zd), m2 = mean(zhat * zd), zhat = (z - mu) * rstd          (all [tasks, co]). */
int mi_conv3x3_tangent(void* stream, const float* x0, const float* w0, const float* x1, const float* w1, size_t pstride,
                       const float* z, const float* mu, const float* rstd, int tasks, int n, int h, int wd, int ci, int co,
                       int stride, float* zd, float* m1, float* m2, void* scratch, size_t scratch_bytes);
/* Two-term conv backward of the tangent pass:  dw9 = wgrad(x0, dz0) + wgrad(x1, dz1);  dx (may be NULL) = dgrad(dz0, w0) +
 * dgrad(dz1, w1). */
int mi_conv3x3_bwd2(void* stream, const float* x0, const float* dz0, const float* x1, const float* dz1, const float* w0,
                    const float* w1, size_t pstride, int tasks, int n, int h, int wd, int ci, int co, int stride, float* dx,
                    float* dw9, size_t gstride, void* scratch, size_t scratch_bytes);

/* Tangent of BN + ReLU + MaxPool (formulas: oracle/kernels_ref.py header).  Per-task vectors advance by their stride. */
typedef struct {
  const float *z, *zd;                  /* conv output and its tangent [tasks, n, ho, wo, c] */
  const float *mu, *rstd, *m1, *m2;     /* [tasks, c] */
  const float *gamma, *beta; size_t pstride;      /* parameters */
  const float *gammad, *betad; size_t vstride;    /* tangent direction */
  const float *dgamma, *dbeta; size_t gstride;    /* primal BatchNorm gradients (backward only) */
  const float *dp, *dpd;                /* cotangent of the block output and its tangent [tasks, n, hp, wp, c] (backward only) */
  int32_t tasks, n, ho, wo, c, pool;
} mi_bn_tangent_args;
int mi_bn_tangent_fwd(void* stream, const mi_bn_tangent_args* a, float* pd);
int mi_bn_tangent_bwd(void* stream, const mi_bn_tangent_args* a, float* rdgamma, float* rdbeta, size_t hstride, float* rdz,
                      void* scratch, size_t scratch_bytes);

/* Fused first ConvBlock (conv recomputed inside every kernel; Ci in {1,3}, stride 1, pooling, even H/W >= 16). */
#define MI_B1_STATS 0        /* -> out0 = mean, out1 = rstd of conv1's output */
#define MI_B1_FWD 1          /* -> p_out (+ zh_out = zhat at each window's argmax, arg_out = argmax position, 4 = ReLU off) */
#define MI_B1_BWD_REDUCE 2   /* -> out0 = dgamma, out1 = dbeta */
#define MI_B1_BWD_WGRAD 3    /* -> out0 = dW [tasks][ostride] */
#define MI_B1_TSTATS 4       /* -> out0 = m1, out1 = m2 */
#define MI_B1_TFWD 5         /* -> p_out = tangent of the block output (+ zh_out = tangent of zhat at the argmax) */
#define MI_B1_TBWD_REDUCE 6  /* -> out0 = R{dgamma}, out1 = R{dbeta} */
#define MI_B1_TBWD_WGRAD 7   /* -> out0 = R{dW} */
#define MI_B1_TFWD_ARG 8     /* as TFWD, from the stored argmax / zhat (arg_in, zh_in) with one conv instead of two */
typedef struct {
  const float* x;                       /* [tasks, n, h, w, ci] NHWC */
  const float *w, *wd;                  /* conv weights [9*ci, co] of theta / of the tangent direction */
  const float *gamma, *beta; size_t pstride;      /* stride of w / gamma / beta */
  const float *gammad, *betad; size_t vstride;    /* stride of wd / gammad / betad */
  const float *mu, *rstd, *m1, *m2;     /* [tasks, co] */
  const float *dgamma, *dbeta; size_t gstride;
  const float *rdgamma, *rdbeta; size_t hstride;
  const float *dp, *dpd;                /* [tasks, n, h/2, w/2, co] */
  const uint8_t* arg_in; const float* zh_in;      /* outputs of MI_B1_FWD (TFWD_ARG, mi_block1_wgrad_gram) */
  int32_t tasks, n, h, w_, ci, co;
} mi_block1_args;
size_t mi_block1_scratch_bytes(int tasks, int n, int h, int w, int ci, int co);
/* mode | 0x100 (forward modes MI_B1_FWD / MI_B1_TFWD_ARG): run the general block1_kernel instead of the lean block1_fwd_kernel the
 * engine uses for tasks of fewer than ~198 84x84x3 images (tests keep the fallback honest). */
int mi_block1_run(void* stream, int mode, const mi_block1_args* a, float* p_out, float* zh_out, uint8_t* arg_out, float* out0,
                  float* out1, size_t ostride, void* scratch, size_t scratch_bytes);
/* dgamma / dbeta of a fused block 1 (zhd, dpd != NULL: their tangents) from pooled-resolution tensors [tasks, rows, c]. */
int mi_pooled_reduce(void* stream, const float* p, const float* zh, const float* zhd, const float* dp, const float* dpd,
                     int tasks, int rows, int c, float* out0, float* out1, size_t ostride, void* scratch, size_t scratch_bytes);
/* Block-1 weight gradient (tangent != 0: its tangent) without conv1: sparse MFMA pass over the pooling argmax + dense parts
 * from the input Gram matrix g of mi_input_gram. */
int mi_block1_wgrad_gram(void* stream, const mi_block1_args* a, const double* g, int tangent, float* dw, size_t ostride,
                         void* scratch, size_t scratch_bytes);

/* Debug/test aids.  mi_debug_conv_tiles_per_wave: the tiles-per-wave split the conv kernels use for this problem (lets a test
 * assert it exercises the multi-tile loop).  mi_debug_set_trace: while buf != NULL every mi_meta_batch_maml call with
 * with_grad != 0 also writes, per task and in the reference's parameter order,
 *   theta_k [K+1][tasks][P] | g_k = grad L_support(theta_k) [K][tasks][P] | lam_{k+1} (the vector fed to the k-th
 *   Hessian-vector product) [K][tasks][P] | H_support(theta_k) lam_{k+1} [K][tasks][P]
 * (the last two only for second-order calls): the per-step state the teacher-forced parity tests check against the oracle. */
int mi_debug_conv_tiles_per_wave(int tasks, int n, int ho, int wo, int co);
/* Launch plans (test aids; host arithmetic only, no HIP call: they answer without a GPU).  The problem is given as the kernel entry points
 * take it (forward geometry n, h, w, ci, co, stride); the answer is what the launchers themselves launch from, under the operand form in
 * force (mi_conv_set_split_bf16, mi_conv_set_b16), with the fp16 form's scales taken as present.  out receives 8 ints.
 * mi_debug_wgrad_plan (launch_wgrad3x3; nterms 1 or 2):
 *   out[0] kernel family: 0 first layer (wgrad3x3_first_mfma_kernel), 1 generic chunked (wgrad3x3_mfma_kernel), 2 fp32 rows
 *          (wgrad3x3_rows_mfma_kernel), 3 split-bf16 rows (wgrad3x3_rows_bf16_kernel), 4 split-bf16 strips (wgrad3x3_strip_bf16_kernel)
 *   out[1] fp32 rows: RH (columns per segment: 7, 8, 5 or 4); bf16 rows: 8; strips: rows per piece; families 0 / 1: pixels per chunk
 *   out[2] fp32 rows: 1 = the EXACT instance
 *   out[3] rows / strips: units / items of the [term][unit] stream per workgroup; families 0 / 1: chunks per workgroup
 *   out[4] workgroups per task     out[5] rows / strips: units / items per term; families 0 / 1: output pixels per task
 *   out[6] operand form of the launch (0 fp32, 1 split bf16, 2 fp16 planes)     out[7] partials per task
 * mi_debug_conv_plan (launch_conv3x3; mode 0 forward, 1 dgrad; epi 0 none, 1 BatchNorm statistics, 2 tangent statistics):
 *   out[0] kernel: 0 first layer, 1 generic (conv3x3_mfma_kernel), 2 stride-1 fp32 (conv3x3_s1_mfma_kernel), 3 split bf16 on 32x32x16
 *          MFMAs, 4 split bf16 on 16x16x32 MFMAs (conv3x3_s1_b16_kernel), 5 fp16 planes
 *   out[1] tiles per wave   out[2] tiles per task   out[3] workgroups per task and filter tile   out[4] pixels per tile (32 / 30)
 *   out[5] waves per workgroup   out[6] operand form of the launch
 *   out[7] 1 = the 16x16x32 kernel's instance that adds every value to the BatchNorm statistics in fp64 (a task of one tile)
 * Both return MI_ERR_ARG (out still filled) where no kernel takes the geometry. */
int mi_debug_wgrad_plan(int tasks, int n, int h, int w, int ci, int co, int stride, int nterms, int* out);
int mi_debug_conv_plan(int tasks, int n, int h, int w, int ci, int co, int stride, int nterms, int epi, int mode, int* out);
int mi_debug_set_trace(mi_engine* e, float* buf, size_t floats);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-launch profiling with HIP events on the caller's stream (the reference has no profiler hooks, SURVEY.md section 5;
 * bench.py uses this for its roofline figures).  kind = op * 8 + layer; kind_filter < 0 profiles every launch. */
int mi_profile_enable(mi_engine* e, int on, int kind_filter);
int mi_profile_kinds(void);
const char* mi_profile_op_name(int op);
int mi_profile_collect(mi_engine* e, double* total_ms, int64_t* count, int n_kinds);

/* ------------------------------------------------------------------------------------------------------------------
 * MAML-TRPO policy path (BASELINE config 5; core_functions/policies.py:30-67, core_functions/rl.py:346-473).
 * Policy parameters are a flat fp32 vector in DiagNormalPolicy's named_parameters() order:
 *   sigma[A], mean.0.weight[H1,S], mean.0.bias[H1], mean.2.weight[H2,H1], mean.2.bias[H2], mean.4.weight[A,H2], mean.4.bias[A].
 * Replays are padded to `batch` rows per task: states [tasks,batch,S], actions [tasks,batch,A], advantages [tasks,batch]
 * (already normalised, rl.py:354-355), count[tasks] = valid rows.  The baseline fit / GAE (rl.py:95-110) stay on the host. */
typedef struct mi_policy mi_policy;
typedef struct {
  int32_t state_size, action_size, hidden1, hidden2;
  int32_t activation; /* 0 = ReLU (DiagNormalPolicy default), 1 = tanh (activation='tanh', policies.py:32-37; the
                         DiagNormalPolicyANIL body, policies.py:76) */
} mi_policy_desc;

/* Accepted domain: state_size >= 1, hidden1 >= 1, hidden2 >= 1 (the two widths need not be equal), action_size 1 .. 6, activation 0 or 1;
 * anything else is MI_ERR_ARG with a text in mi_policy_last_error(NULL), and *out is left alone.  Every mi_policy_* / mi_trpo_* entry
 * below takes every policy of this domain (mi_particles_rollout alone is narrower: see there).
 * Which kernels run: a policy with hidden1 == hidden2 == 100, ReLU, state_size <= 4 (any action_size) takes the fused sweeps of
 * csrc/policy_sweep.h in mi_trpo_surrogate_steps and mi_trpo_fvp_steps at steps == 1 (mi_policy_set_fused_fvp(0) switches them off).  Every other shape, and every
 * other entry point at any shape, runs the per-layer kernels of csrc/policy.hip: one dense product per layer and pass for all tasks
 * (operand loads of 16 bytes where the reduction width is a multiple of 4 and at least 16, of 8 bytes where it and its half are even and
 * the operands 8-byte aligned, scalar otherwise) and one weight-gradient launch per layer with the bias as column I of an (I + 1)-wide
 * tile grid.  tests/test_gpu_policy_shapes.py holds the per-layer path to fp64 autograd at widths from 1 to 160. */
int mi_policy_create(const mi_policy_desc* desc, int device, mi_policy** out);
void mi_policy_destroy(mi_policy* p);
const char* mi_policy_last_error(const mi_policy* p);
int mi_policy_param_count(const mi_policy* p, size_t* n);

/* density(state).loc (policies.py:49-52) for acting; theta shared (tstride 0) or one vector per task (tstride = P).  A workspace that
 * serves mi_policy_adapt (below) serves this call. */
int mi_policy_forward(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, int tasks, int batch,
                      float* loc_out, void* workspace, size_t workspace_bytes);

/* Particles2D episodes on the device (rollout.hip): what Particles2DRunner.run does with a host loop of
 * max_path_length steps (reference core_functions/runner.py + learn2learn's Particles2D), for `episodes` episodes of each of `tasks`
 * tasks in two launches -- whatever `tasks` is -- and with no host synchronisation.  Per episode, in fp32: s_0 = 0,
 * scale = exp(max(sigma, log 1e-6)); for t = 0 .. L-1: loc = MLP(s_t), a = loc + scale * eps_t (stored UNclipped),
 * s_{t+1} = s_t + clamp(a, -0.1, 0.1), reward = -|s_{t+1} - goal|_2, done = both |s_{t+1} - goal| < 0.01, stored dones = done or
 * t == L-1; the episode's rows are steps 0 .. t_done.  The noise is a pure function of (seed, rollout id, episode, step):
 * Philox4x32-10, key = seed, counter = (id_lo, id_hi, episode, step); u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24,
 * r = sqrt(-2 log u1), eps = (r cos 2 pi u2, r sin 2 pi u2) (exploring_meta_amd.utils.rollout_ref restates it in numpy).  A task's
 * result depends on its own theta, goal and id alone: not on `tasks`, on the other tasks of the call, or on tstride.
 *   theta        shared (tstride 0) or one vector per task (tstride = P), the parameter order above
 *   goals        [tasks, 2];  rollout_ids [tasks] uint64, DEVICE memory
 *   states, actions, next_states [tasks, B, 2], rewards, dones [tasks, B], B = episodes * max_path_length (8-byte aligned): the
 *                episodes of a task concatenated in episode order, every row past count[t] zero in all fields -- the padded batch
 *                mi_gae_advantages and mi_policy_adapt take
 *   count [tasks] rows in use;  ep_len [tasks, episodes] or NULL;  noise_out [tasks, B, 2] or NULL: eps of each packed row
 * state_size == action_size == 2, 1 <= hidden1, hidden2 <= 128, ReLU or tanh, tasks >= 1 (tasks * episodes < 2^31),
 * 1 <= episodes <= 256, 1 <= max_path_length <= 1000 (MI_ERR_ARG naming the value otherwise, before any HIP call; the scratch size
 * is 0 then).  Results are bitwise reproducible. */
size_t mi_particles_rollout_scratch_bytes(const mi_policy* p, int tasks, int episodes, int max_path_length);
int mi_particles_rollout(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* goals,
                         const uint64_t* rollout_ids, uint64_t seed, int tasks, int episodes, int max_path_length,
                         float* states, float* actions, float* next_states, float* rewards, float* dones,
                         int32_t* count, int32_t* ep_len, float* noise_out, void* scratch, size_t scratch_bytes);
/* trpo_update (rl.py:361-374): theta_out[t] = theta[t] - lr * grad_t( a2c.policy_loss = -mean(log_prob * advantages) ).
 * head_only != 0: the hidden layers run under no_grad (DiagNormalPolicyANIL.turn_off_body_grads, policies.py:100-106,
 * rl.py:381-382), so only sigma and the last Linear are updated (learn2learn maml_update skips None gradients).
 * Workspace: mi_policy_meta_workspace_bytes(steps = 1, n_batches = 1, second_order = 1) bytes; every mi_trpo_*_workspace_bytes is
 * at least that. */
int mi_policy_adapt(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* actions,
                    const float* adv, const int32_t* count, int tasks, int batch, float lr, int head_only, float* theta_out,
                    float* loss_out, void* workspace, size_t workspace_bytes);
/* 1 (default): mi_trpo_surrogate_steps / mi_trpo_fvp_steps with steps == 1 of a supported policy (ReLU, 100-wide hidden layers: the
 * reference's DiagNormalPolicy defaults, policies.py:30-37) run as fused sweeps over the stored passes + folds (csrc/policy_sweep.h:
 * a product is three of each instead of ~34 per-layer launches); 0: the per-layer path.  Process-wide ablation / test switch; results
 * agree to fp32 rounding. */
int mi_policy_set_fused_fvp(int on);
/* Step-wise policy learner (csrc/policy_learner.hip): the mean loc = MLP(theta; states) as a twice-differentiable unit, the policy-side
 * mirror of mi_learner_backward / mi_learner_hvp (learn2learn `learner.adapt(loss)` on a policy: reference misc_scripts/cl_rl.py:71-75).
 * sigma -> scale, the Normal and the loss stay with the caller.  With cotangents dloc [tasks, batch, A] and
 *   s_t(theta_t) = sum_{row < count[t]} sum_a loc * dloc          (count NULL: every row)
 *   mi_policy_vjp: grad_out [tasks, P] = d s_t / d theta_t in the parameter order above; the sigma slots are exact zeros; rows past
 *     count[t] contribute nothing, whatever they hold.
 *   mi_policy_hvp: for a direction v [tasks, P] (its sigma entries are ignored), grad_theta_out [tasks, P] = (d^2 s_t / d theta^2) v_t
 *     with dloc held fixed, and loc_dot_out [tasks, batch, A] = J_t v_t, zero on rows past count[t]: the double backward of the VJP.
 *   head_only != 0 (DiagNormalPolicyANIL.turn_off_body_grads(): the hidden layers are constants): only W3 / b3 receive a gradient,
 *     loc_dot = V3 h2 + vb3 and grad_theta_out is exactly zero.
 * theta shared (tstride 0) or one vector per task (tstride = P).  Results are bitwise reproducible, and a task's outputs do not depend
 * on the other tasks of the call.  tasks, batch >= 1, tstride 0 or P, non-null arrays: MI_ERR_ARG naming the entry and the value
 * otherwise, before any HIP call.
 * Which kernels run: 1 <= hidden1, hidden2 <= 128, state_size <= 16 (any action_size, ReLU or tanh) takes one fused sweep + one fold
 * per call (W2 and the direction's V2 resident in LDS); every other shape, and every shape after mi_policy_set_fused_learner(0) (a
 * process-wide ablation / test switch, default 1), composes the per-layer kernels of csrc/policy.hip.  The two agree to fp32 rounding.
 * Measured at 2-100-100-2, 2000 rows per task: the fused sweep is faster for one task (what the Python learner
 * calls), the per-layer path for 20 tasks per call; the path is never chosen from the task count (a task's bits would depend on it). */
int mi_policy_learner_workspace_bytes(const mi_policy* p, int tasks, int batch, size_t* bytes);
int mi_policy_vjp(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* dloc,
                  const int32_t* count, int tasks, int batch, int head_only, float* grad_out, void* workspace, size_t workspace_bytes);
int mi_policy_hvp(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* dloc, const float* v,
                  const int32_t* count, int tasks, int batch, int head_only, float* grad_theta_out, float* loc_dot_out, void* workspace,
                  size_t workspace_bytes);
int mi_policy_set_fused_learner(int on);
int mi_policy_learner_fused_supported(const mi_policy* p);   /* 1: the shape takes the fused sweep while the switch is on */
/* Debug aid: shader-clock stamps (stage id << 56 | s_memtime) of workgroup 0 of every fused sweep into buf (>= 256 u64; the three sweeps of a
 * product overwrite each other: read after the call, last sweep wins); NULL switches it off. */
int mi_debug_policy_sweep_stamps(void* buf);
/* Debug aid: s_memtime stamps {start, weights staged, first tile done, tiles done, epilogue done} of workgroup (0,0,0) of every stride-1
 * conv launch (csrc/conv_mfma.hip) into buf (>= 8 u64, the last launch wins); NULL switches it off. */
int mi_debug_conv_stamps(void* buf);
/* Operand form of the stride-1 hidden -> hidden 3x3 convolutions with 32 filters (forward, dgrad, their two-term tangent forms and the
 * weight gradient on maps at least 16 wide) and with 64 filters (one-term forward and dgrad, weight gradient on maps at least 16 wide) --
 * the implicit ATen conv2d launches behind
 * ConvBlock.conv, reference core_functions/vision_models.py:177-185,189.  1: split-bf16 -- every fp32 operand as the
 * exact sum of three bf16 pieces, six v_mfma_f32_32x32x16_bf16 products per K = 16 accumulated in fp32 (the three dropped cross terms
 * are <= 2^-24 of a product: one fp32 rounding).  2: two scaled fp16 planes -- x s = h + l with s a power of two chosen per task and
 * tensor from the tensor's largest magnitude (the producing kernels record it; standalone operator entries run a reduction launch),
 * three v_mfma_f32_32x32x16_f16 products per K = 16, the scales multiplied out of the fp32 sums exactly: 22 bits of every operand, an
 * absolute floor 2^-39 below the tensor's maximum, per-kernel errors against fp64 at or below those of the fp32 pipe; a launch whose
 * operands come without a recorded magnitude takes form 1.  Form 2 is an OPT-IN: its operands are narrower than the reference's fp32
 * (22 bits), so benchmark lines that use it say so and it is never the default.  0: the fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
 * Default 1 (environment variable MI_CONV_BF16X3=0 / 2 starts with another); returns the previous setting.  All three forms meet the
 * same fp32 parity bars (tests run all three).  Values above 0xff (0x100 * variant mask + form) select single kernel variants for bisecting
 * (tools/wgrad_probe.py, csrc/conv_mfma.hip) and are not part of the interface. */
int mi_conv_set_split_bf16(int on);
/* The operand form in force (2 scaled fp16 planes, 1 split-bf16, 0 fp32 matrix pipe) read without side effects; mask_out (may be NULL)
 * receives the variant mask a bisecting run set through MI_CONV_BF16X3_MASK / mi_conv_set_split_bf16(0x100 * mask + form). */
int mi_conv_get_split_bf16(unsigned* mask_out);
/* Which kernel runs the split-bf16 form (form 1) of the stride-1 hidden convolutions (forward, dgrad and their two-term tangent forms;
 * ConvBlock.conv of blocks >= 2, reference core_functions/vision_models.py:177-185,189): 16x16x32 MFMAs with one accumulator per horizontal
 * tap (csrc/conv_b16.h) or the 32x32x16 kernel with lane-shifted operands of rounds 3-4.  0 = always the latter, 2 = always the former,
 * 1 (default; MI_CONV_B16 starts with another) = the former for launches of at least 6 tiles per wave, rounded up (MI_CONV_B16_MIN_TPW), where its
 * longer pipeline fill is amortised.  Same operands, products and tiles; the two kernels differ in summation order only and meet the same
 * parity bars (the kernel tests run both on every case).  on < 0 only reads.  Returns the previous setting. */
int mi_conv_set_b16(int on);
/* Operand form of conv1 inside the two lean block-1 forward kernels (ConvBlock 1 of a three-channel net: conv + BatchNorm + ReLU + pool
 * with the conv output never stored, and its tangent from the stored argmax; reference core_functions/vision_models.py:188-193).
 * 0: the fp32 matrix pipe, bit-identical to the general block-1 kernel.  1: split bf16 with all
 * eight products down to 2^-24 (raw-pixel inputs: the six-product form of the hidden blocks is measurably noisier here) and the
 * BatchNorm normalisation folded into the product.  2: the split form in the tangent-forward kernel only -- it takes no pooling / ReLU
 * decisions (the argmax is the forward pass's stored one), so its rounding cannot re-route anything; the forward kernel stays on the fp32 pipe.
 * Default (on < 0, or never set; MI_B1_BF16X3 in the environment sets it): 1 since round 6, in every pass whose later kernels read the pooling /
 * ReLU decisions the forward stored (the Gram-matrix path of block 1: support passes and, since round 6, the query pass); passes whose backward
 * recomputes conv1 on the fp32 pipe and re-derives the decisions keep the forward on the fp32 pipe, so the two always agree.  (Rounds 4 - 5: 2.
 * Post-adaptation accuracy over 1024 tasks cannot tell forms 1 and 2 from fp64 or from each other,
 * profiles/r6/accuracy_parity_cfg2_1024tasks_b1forms.md; form 1 failed decision-level bars only while the query pass's backward re-derived its
 * decisions: csrc/block1.hip.)  With the hidden blocks on the fp32 pipe (mi_conv_set_split_bf16(0)) the default is 2.
 * Returns the form in force before the call. */
int mi_block1_set_split_bf16(int on);
/* Operand form of the sparse part of block 1's weight gradient on 84-wide three-channel inputs (dW1 = sum over pooling windows of the input
 * patch at the window's argmax times the cotangent: what autograd's conv2d backward computes for ConvBlock 1, reference
 * core_functions/vision_models.py:188-193, after max-pool and ReLU have zeroed three of every four positions).  1: split-bf16 operands on
 * the 16-bit matrix pipe with the six partial products of an fp32 product laid out along K (csrc/gram.hip) -- fp32-equivalent, same parity
 * bars; 0: fp32-input MFMAs.  on < 0 (default; MI_SPARSE_WGRAD_BF16 in the environment sets it): follow mi_conv_set_split_bf16 (fp32 pipe
 * there -> fp32 here).  Returns the form in force before the call. */
int mi_sparse_wgrad_set_split_bf16(int on);

/* ANIL-TRPO (rl/anil_trpo.py:104-129, core_functions/rl.py:409-473 with anil=True): the stored old policies were adapted with
 * the body under no_grad (rl.py:381-382) while meta_surrogate_loss re-adapts clone_module(policy) with every parameter
 * (rl.py:447-453), so at the current parameters new != old and trpo.hessian_vector_product(kl) (rl.py:417) is the EXACT Hessian
 * of the mean KL:  mean_t [ J_t^T Hess KL_t(theta'_t) J_t v - lr T_t[v, grad KL_t(theta'_t)] ] + damping v,  T_t = the third
 * derivative of the inner loss (second-order tangent sweep, policy.hip): mi_trpo_kl_prepare_steps / mi_trpo_fvp_general_steps
 * below, for any number of inner updates. */

/* MAML inner loop of the policy with K updates and the VPG / PPO losses, all tasks per call (core_functions/rl.py:
 * fast_adapt_vpg :231-255 with vpg_a2c_loss :209-228 (dice=False), fast_adapt_ppo :267-318; drivers rl/maml_ppo.py, anil_ppo.py).
 *   theta_{k+1} = theta_k - inner_lr * grad L_k(theta_k), k < steps; update k replays support batch step_batch[k] (host array):
 *     VPG: one batch per adapt step; PPO: ppo_epochs consecutive updates share a batch, step_new_old[k] = 1 on the first of them
 *     (old_log_probs are taken at theta_k under no_grad, rl.py:282-283).
 *   support batches [n_batches, tasks, batch, ...] padded like the TRPO replays; count [n_batches, tasks] (NULL = all valid).
 *   loss_out[t] = the validation loss of task t at theta_steps: VPG a2c.policy_loss, PPO ppo.policy_loss against the adapted
 *     policy itself (ratio 1).  theta_out [tasks, P] (or NULL) = adapted parameters.
 *   with_grad: grad_out [P] = SUM over tasks of d loss_out[t] / d theta -- what `av_loss.backward()` leaves in .grad after the
 *     caller's 1/meta_batch_size; second_order = learn2learn's default adapt (0: first-order MAML).
 *   head_only: updates touch only sigma and the last Linear (ANIL, body under no_grad). */
#define MI_PLOSS_A2C 0
#define MI_PLOSS_PPO 1
#define MI_PLOSS_DICE 2   /* vpg_a2c_loss(dice=True), rl.py:219-226: needs mi_policy_meta_batch_dones */
int mi_policy_meta_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int n_batches, int second_order,
                                   size_t* bytes);
int mi_policy_meta_batch(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                         const int32_t* step_new_old, int n_batches, const float* s_states, const float* s_actions,
                         const float* s_adv, const int32_t* s_count, const float* q_states, const float* q_actions,
                         const float* q_adv, const int32_t* q_count, int tasks, int batch, int loss_kind, float clip,
                         float inner_lr, int head_only, int second_order, int with_grad, float* loss_out, float* theta_out,
                         float* grad_out, void* workspace, size_t workspace_bytes);
/* The same with the replays' episode-end flags (cherry `dones`; s_done [n_batches, tasks, batch], q_done [tasks, batch], 1.0 at
 * the last step of every episode).  Required by loss_kind MI_PLOSS_DICE -- vpg_a2c_loss(dice=True), rl.py:219-226: the adapt
 * losses AND the validation loss use  a2c.policy_loss(magic_box(weighted_cumsum(log_probs, weights)), advantages)  with
 * weights = (1 - dones shifted by one) / dones.sum(), including the reference's wrap-around at the first sample. */
int mi_policy_meta_batch_dones(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                               const int32_t* step_new_old, int n_batches, const float* s_states, const float* s_actions,
                               const float* s_adv, const int32_t* s_count, const float* s_done, const float* q_states,
                               const float* q_actions, const float* q_adv, const int32_t* q_count, const float* q_done, int tasks,
                               int batch, int loss_kind, float clip, float inner_lr, int head_only, int second_order,
                               int with_grad, float* loss_out, float* theta_out, float* grad_out, void* workspace,
                               size_t workspace_bytes);

/* The inner update of fast_adapt_vpg / fast_adapt_ppo (rl.py:231-255,267-318) and single_ppo_update (rl.py:319-336) on its own,
 * for all tasks per call and from PER-TASK parameters: per task u_0 = theta[t] (tstride 0: shared, P: one row per task),
 *   u_{e+1} = u_e - lr * grad L(u_e), e < epochs;   theta_out[t] = u_epochs;   loss_out[t][e] = L(u_e)   (loss_out may be NULL)
 * with L the loss mi_policy_meta_batch uses for loss_kind on the task's replay (states [tasks,batch,S], actions [tasks,batch,A],
 * adv [tasks,batch], count [tasks] or NULL, padded like the TRPO replays).  MI_PLOSS_PPO takes the old log-probabilities once, at
 * u_0 (rl.py:280-290); MI_PLOSS_DICE needs done [tasks,batch] (NULL otherwise).  head_only as in mi_policy_adapt.  The updates are
 * plain (nothing is kept for a meta-gradient): the passes of a first-order mi_policy_meta_batch step in the same order, so from
 * shared parameters theta_out is bit-identical to mi_policy_meta_batch(steps = epochs, with_grad = 0) on the same replay.  The number
 * of launches does not depend on `tasks`.  theta_out may be theta itself when tstride = P.
 * tasks, batch >= 1, 1 <= epochs <= 64, tstride 0 or P, loss_kind one of MI_PLOSS_*: MI_ERR_ARG with a text naming mi_policy_update
 * and the value otherwise, before any HIP call.  The workspace size covers every epochs in range. */
int mi_policy_update_workspace_bytes(const mi_policy* p, int tasks, int batch, size_t* bytes);
int mi_policy_update(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* actions,
                     const float* adv, const int32_t* count, const float* done, int tasks, int batch, int loss_kind, int epochs,
                     float clip, float lr, int head_only, float* theta_out, float* loss_out, void* workspace, size_t workspace_bytes);

/* The two calls above with per-parameter inner-loop step sizes (learn2learn MetaSGD beside MAML; core_functions/inner_lr.py): lr_vec
 * [lr_rows][P] on the device, in the engine's parameter order (sigma, W1, b1, W2, b2, W3, b3), shared by all tasks; update k reads row
 * step_lr_row[k] (host array; NULL = every update reads row 0).  With m the head mask of head_only (1 on sigma, W3, b3, else 0; all ones
 * without head_only) and d_k = lr_vec[row(k)] (.) m:
 *   theta_{k+1} = theta_k - d_k (.) g_k,   g_k = grad L_k(theta_k)       (an entry whose step is exactly 0 passes through bitwise)
 *   lam_K = grad L_query(theta_K);   second order: lam_k = lam_{k+1} - mask_m(H_k (d_k (.) lam_{k+1}));   first order: lam_k = lam_K
 *   grad_out = SUM_t lam_0;   lr_grad_out[r] = - SUM_{k: row(k) = r} SUM_t m (.) g_k (.) lam_{k+1}      (NULL: not computed)
 * -- d loss / d lr_vec, the MetaSGD gradient: at a frozen (zero-step) entry it is in general not 0; under head_only the body entries are
 * exact zeros.  lr_grad_out is one fp64 chain per entry over the updates of its row, ascending, and within an update over the tasks,
 * ascending, rounded once: bitwise reproducible.  steps == 0: exact zeros.  A uniform lr_vec is the scalar call up to rounding, bit for bit
 * in loss_out, theta_out and the first-order grad_out, and in the second-order grad_out when the step is a power of two (the tangent pass
 * is driven with d (.) lam where the scalar call scales H lam afterwards).  The same implementation as the scalar calls: their launches with
 * the vector advance in place of the scalar one (head mask folded in), one launch per update of the adjoint recursion in place of copy +
 * mask + mask + advance, one more at its start, and one for lr_grad_out; the count does not depend on `tasks`.  A task's theta_out /
 * loss_out do not depend on the other tasks.  mi_policy_update_lr takes ONE row lr_vec [P] for every epoch of the call; from shared
 * parameters its theta_out is bit-identical to mi_policy_meta_batch_lr(steps = epochs, with_grad = 0) on the same replay and row; its
 * workspace is mi_policy_update_workspace_bytes.  s_done / q_done as in mi_policy_meta_batch_dones (NULL unless MI_PLOSS_DICE).
 * Workspace: mi_policy_meta_lr_workspace_bytes -- the scalar plan, then g per update and (second order) the products, both only when
 * want_lr_grad.  MI_ERR_ARG with a text naming the entry and the value, before any HIP call: lr_vec NULL, lr_rows outside 1..65535, steps outside
 * 0..256, a step_lr_row entry outside 0..lr_rows-1, lr_grad_out with with_grad == 0, and every check of the scalar entries. */
int mi_policy_meta_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int n_batches, int second_order, int lr_rows,
                                      int want_lr_grad, size_t* bytes);
int mi_policy_meta_batch_lr(mi_policy* p, void* stream, const float* theta, int steps, const int32_t* step_batch,
                            const int32_t* step_new_old, const int32_t* step_lr_row, int n_batches, const float* s_states,
                            const float* s_actions, const float* s_adv, const int32_t* s_count, const float* s_done,
                            const float* q_states, const float* q_actions, const float* q_adv, const int32_t* q_count,
                            const float* q_done, int tasks, int batch, int loss_kind, float clip, const float* lr_vec, int lr_rows,
                            int head_only, int second_order, int with_grad, float* loss_out, float* theta_out, float* grad_out,
                            float* lr_grad_out, void* workspace, size_t workspace_bytes);
int mi_policy_update_lr(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* actions,
                        const float* adv, const int32_t* count, const float* done, int tasks, int batch, int loss_kind, int epochs,
                        float clip, const float* lr_vec, int head_only, float* theta_out, float* loss_out, void* workspace,
                        size_t workspace_bytes);

/* MAML-TRPO with `steps` >= 1 inner updates (params['adapt_steps'], one support replay per update, rl.py:447-453).
 * mi_trpo_surrogate_steps: meta_surrogate_loss (rl.py:441-473) with `steps` second-order inner updates per task: mean surrogate loss,
 * mean KL(new||old), and (grad_out != NULL) the gradient w.r.t. theta (rl.py:413-416).  old_loc [tasks,batch,A], old_scale [tasks,A]
 * are the stored adapted policies' densities on the query states.  Support arrays carry a leading [steps] axis (also at steps == 1):
 * s_states [steps,tasks,batch,S], s_actions [steps,tasks,batch,A], s_adv [steps,tasks,batch], s_count [steps,tasks].
 * mi_trpo_fvp_steps: trpo.hessian_vector_product(old_kl, params, damping)(v) (rl.py:417) where the adapted policies equal the stored
 * old ones.  It takes no theta: it must follow mi_trpo_surrogate_steps on the same workspace and replays, and works at the theta of
 * that call (the surrogate keeps a copy next to the saved passes).
 * Calls on ONE mi_policy are ordered by the caller (one stream at a time): the fused product keeps a few arrival counters in device
 * memory owned by the policy object (its last fold also takes the mean over tasks; they are zero between launches). */
int mi_trpo_steps_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, size_t* bytes);
int mi_trpo_surrogate_steps(mi_policy* p, void* stream, const float* theta, int steps, const float* s_states,
                            const float* s_actions, const float* s_adv, const int32_t* s_count, const float* q_states,
                            const float* q_actions, const float* q_adv, const int32_t* q_count, const float* old_loc,
                            const float* old_scale, int tasks, int batch, float inner_lr, float* loss_out, float* kl_out,
                            float* grad_out, void* workspace, size_t workspace_bytes);
int mi_trpo_fvp_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions, const int32_t* s_count,
                      const float* q_states, const int32_t* q_count, int tasks, int batch, float inner_lr, float damping,
                      const float* v, float* out, void* workspace, size_t workspace_bytes);

/* ANIL-TRPO with `steps` >= 1 inner updates (rl/anil_trpo.py --adapt_steps K): the exact Hessian of the mean KL for new != old
 * (see above).  With theta_{k+1} = theta_k - lr grad L_k(theta_k),
 * H_k = Hess L_k(theta_k), T_k the third derivative of L_k at theta_k and c = grad KL_t(theta_K):
 *   lam_K = c, lam_k = lam_{k+1} - lr H_k lam_{k+1};   u_0 = v, u_{k+1} = u_k - lr H_k u_k;   rho_K = Hess KL_t(theta_K) u_K,
 *   rho_k = rho_{k+1} - lr H_k rho_{k+1} - lr T_k[u_k, lam_{k+1}];   product = mean_t rho_0 + damping v.
 * Support arrays carry the leading [steps] axis of mi_trpo_surrogate_steps.
 *   mi_trpo_general_steps_workspace_bytes: workspace for the two calls below AND for mi_trpo_surrogate_steps / mi_trpo_fvp_steps
 *     (it starts with the plan mi_trpo_steps_workspace_bytes reports); it keeps two tangent sweeps per inner update.
 *   mi_trpo_kl_prepare_steps: after mi_trpo_surrogate_steps(theta, steps, ...) on the same workspace and replays; the surrogate's
 *     own query cotangents are left alone.  kl_grad_out (or NULL: lam_0 is then not formed) [P] = d mean KL / d theta = mean_t lam_0.
 *   mi_trpo_fvp_general_steps: the product, any number of times after the two calls above.
 * steps, tasks, batch >= 1 (MI_ERR_ARG otherwise, before any HIP call).  The number of launches depends on `steps` only. */
int mi_trpo_general_steps_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, size_t* bytes);
int mi_trpo_kl_prepare_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                             const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_loc,
                             const float* old_scale, int tasks, int batch, float inner_lr, float* kl_grad_out, void* workspace,
                             size_t workspace_bytes);
int mi_trpo_fvp_general_steps(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                              const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_scale,
                              int tasks, int batch, float inner_lr, float damping, const float* v, float* out, void* workspace,
                              size_t workspace_bytes);

/* The TRPO calls with per-parameter inner-loop step sizes (fixed: TRPO's outer step is a trust region over theta alone, the steps get
 * no gradient).  Each entry is its scalar namesake with `const float* lr_vec, int lr_rows, const int32_t* step_lr_row` where that takes
 * `float inner_lr`: lr_vec [lr_rows][P] on the device in the parameter order (sigma, W1, b1, W2, b2, W3, b3), shared by all tasks;
 * update k reads row step_lr_row[k] (host array [steps]; NULL: row 0 for every update).  With d_k that row,
 *   theta_{k+1} = theta_k - d_k (.) g_k                     J_k = I - D_k H_k
 *   tangent  (J_k u):      u_{k+1} = u_k - d_k (.) (H_k u_k)
 *   adjoint  (J_k^T lam):  lam_k   = lam_{k+1} - H_k (d_k (.) lam_{k+1})            (NOT lam - d (.) (H lam): D H is not symmetric)
 *   surrogate gradient = mean_t lam_0 with lam_K = grad S_t(theta_K);   Fisher form (new == old) = mean_t J^T F_t J v + damping v
 *   exact KL Hessian:  rho_K = Hess KL_t(theta_K) u_K,
 *                      rho_k = rho_{k+1} - H_k (d_k (.) rho_{k+1}) - T_k[u_k, d_k (.) lam_{k+1}],   product = mean_t rho_0 + damping v
 * An entry whose step is exactly 0 (a frozen tensor) leaves theta_K with the bits of theta, yet still receives the cross-Hessian terms.
 * The same implementation as the scalar entries (which are its lr_vec == NULL case and launch what they launched before): the fused
 * sweeps at steps == 1 of a supported policy -- the fold that finishes w = F u (or lam) also writes d (.) w for the next sweep, no launch
 * is added -- the per-layer path otherwise; the number of launches depends on `steps` only.
 *   mi_policy_adapt_lr: mi_policy_adapt with ONE row lr_vec [P]; head_only multiplies it by the head mask.
 *   mi_trpo_steps_lr_workspace_bytes: equals mi_trpo_steps_workspace_bytes (the extra direction lives in a slot of that plan that is
 *     idle once the inner updates are done).  mi_trpo_general_steps_lr_workspace_bytes: the scalar plan, offsets unmoved, then
 *     [steps][tasks][P] floats (d_k (.) lam_{k+1}); it serves every *_lr call and every scalar call.
 * Argument errors are MI_ERR_ARG before any HIP call, outputs untouched, with a text naming the entry and the value: lr_vec NULL,
 * lr_rows < 1, a step_lr_row entry outside 0..lr_rows-1, steps / tasks / batch < 1, and the scalar entries' own checks. */
int mi_policy_adapt_lr(mi_policy* p, void* stream, const float* theta, size_t tstride, const float* states, const float* actions,
                       const float* adv, const int32_t* count, int tasks, int batch, const float* lr_vec, int head_only,
                       float* theta_out, float* loss_out, void* workspace, size_t workspace_bytes);
int mi_trpo_steps_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int lr_rows, size_t* bytes);
int mi_trpo_surrogate_steps_lr(mi_policy* p, void* stream, const float* theta, int steps, const float* s_states,
                               const float* s_actions, const float* s_adv, const int32_t* s_count, const float* q_states,
                               const float* q_actions, const float* q_adv, const int32_t* q_count, const float* old_loc,
                               const float* old_scale, int tasks, int batch, const float* lr_vec, int lr_rows,
                               const int32_t* step_lr_row, float* loss_out, float* kl_out, float* grad_out, void* workspace,
                               size_t workspace_bytes);
int mi_trpo_fvp_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions, const int32_t* s_count,
                         const float* q_states, const int32_t* q_count, int tasks, int batch, const float* lr_vec, int lr_rows,
                         const int32_t* step_lr_row, float damping, const float* v, float* out, void* workspace, size_t workspace_bytes);
int mi_trpo_general_steps_lr_workspace_bytes(const mi_policy* p, int tasks, int batch, int steps, int lr_rows, size_t* bytes);
int mi_trpo_kl_prepare_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_loc,
                                const float* old_scale, int tasks, int batch, const float* lr_vec, int lr_rows,
                                const int32_t* step_lr_row, float* kl_grad_out, void* workspace, size_t workspace_bytes);
int mi_trpo_fvp_general_steps_lr(mi_policy* p, void* stream, int steps, const float* s_states, const float* s_actions,
                                 const int32_t* s_count, const float* q_states, const int32_t* q_count, const float* old_scale,
                                 int tasks, int batch, const float* lr_vec, int lr_rows, const int32_t* step_lr_row, float damping,
                                 const float* v, float* out, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MI_MAML_H */
