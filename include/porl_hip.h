/*
 * porl_hip.h — C ABI of libporl_hip.so: the MI355X (gfx950) engine for porl's batched offline-RL
 * update step.  Plain pointers and sizes only; no torch types.  All device pointers are fp32 unless
 * noted; every call enqueues on `stream` (a hipStream_t passed as void*) and returns without
 * synchronising.  Return value: 0 on success, a negative PORL_ERR_* or a positive hipError_t.
 *
 * The reference (/root/reference, Python) has no FFI layer; each entry point below names the
 * reference Python interface it replaces, and INTEGRATION.md shows the ctypes stub a maintainer
 * would add on the reference side.
 */
#ifndef PORL_HIP_H
#define PORL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PORL_ABI_VERSION 12
#define PORL_MAX_HIDDEN 8

#define PORL_OK 0
#define PORL_ERR_INVALID (-1)      /* bad argument / shape */
#define PORL_ERR_UNSUPPORTED (-2)  /* configuration not implemented on device yet */
#define PORL_ERR_UNBOUND (-3)      /* engine used before porl_iql_bind() */

int porl_abi_version(void);
/* Human-readable text for the last failing call on this thread. */
const char* porl_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * IQL-family engine: POR (agent/por.py:20-112) and SORL (agent/sorl.py:20-152) share one value
 * step (twin-V expectile regression against an EMA target) and an advantage-weighted Gaussian
 * regression step; they differ in the regression target, the mean's output activation and the
 * weight formula.
 * --------------------------------------------------------------------------------------------- */
typedef struct porl_iql_cfg {
  int32_t obs_dim;      /* S: input width of vf / policy (args.state_size or args.feature_dim)       */
  int32_t pol_out_dim;  /* POR: S (goal policy predicts s', por.py:36-39); SORL: args.action_size     */
  int32_t hidden_dim;   /* args.hidden_dim                                                            */
  int32_t n_hidden;     /* args.n_hidden (>= 1)                                                       */
  int32_t layer_norm;   /* args.layer_norm: LayerNorm in TwinV only (value_functions.py:35-36)        */
  int32_t pol_tanh;     /* 1 = BoundedGaussianPolicy (policy.py:35-59), 0 = GaussianPolicy (:12-33)   */
  int32_t weight_mode;  /* 0 = exp(adv/alpha) (por.py:100), 1 = exp(alpha*adv) (sorl.py:104)          */
  int32_t max_batch;    /* workspace is sized for this many rows per call                             */
} porl_iql_cfg;

typedef struct porl_iql porl_iql;   /* opaque host-side handle; owns no device memory */

int porl_iql_create(const porl_iql_cfg* cfg, porl_iql** out);
void porl_iql_destroy(porl_iql* h);

/* Parameter groups.  Each group is ONE flat fp32 range so Adam/EMA/all-reduce are single sweeps;
 * tensors start on 16-byte boundaries, padding floats stay zero.
 *   group 0 "vf"     : TwinV  v1 then v2; per net, per Linear: weight (out,in), bias (out)
 *                       [, LayerNorm weight, bias after each hidden Linear when layer_norm]
 *   group 1 "policy" : log_std (pol_out_dim) first, then net Linear weights/biases
 * The EMA target network uses the layout of group 0.  Tensor order inside a group equals
 * nn.Module.named_parameters() order of the reference modules. */
int64_t porl_iql_group_floats(const porl_iql* h, int group);
int32_t porl_iql_group_tensors(const porl_iql* h, int group);
/* rows == 0 marks a 1-D tensor of `cols` elements. */
int porl_iql_tensor_info(const porl_iql* h, int group, int index, int64_t* offset, int32_t* rows,
                         int32_t* cols);

int64_t porl_iql_workspace_floats(const porl_iql* h);

typedef struct porl_iql_buffers {
  float* params_vf;   /* group 0 floats */
  float* params_tgt;  /* group 0 floats (v_target / v_tgt) */
  float* params_pol;  /* group 1 floats */
  float* grads_vf;
  float* grads_pol;
  float* adam_m_vf;   /* exp_avg    */
  float* adam_v_vf;   /* exp_avg_sq */
  float* adam_m_pol;
  float* adam_v_pol;
  float* workspace;   /* porl_iql_workspace_floats() floats, 16-byte aligned */
  float* stats;       /* >= 8 floats: [0] v_loss, [1] g_loss, [2] min NLL of the batch (por.py:104) */
} porl_iql_buffers;

int porl_iql_bind(porl_iql* h, const porl_iql_buffers* bufs);

/* Minibatch hand-over (replaces the tensor arguments of POR.por_residual_update, por.py:73, and
 * SORL.update, sorl.py:78).  Inputs may be strided column slices of one packed (B,row) tensor
 * (por_train.py:74-78): *_rs are row strides in floats, matrices have unit column stride, vectors
 * have element stride *_rs.  `pol_target` is s' for POR and the action matrix for SORL; it may be NULL
 * when only the value step is run.  Caller keeps ownership; inputs are not modified. */
int porl_iql_load_batch(porl_iql* h, int32_t batch,
                        const float* obs, int64_t obs_rs,
                        const float* next_obs, int64_t next_rs,
                        const float* rew, int64_t rew_rs,
                        const float* term, int64_t term_rs,
                        const float* pol_target, int64_t pt_rs,
                        void* stream);

/* Same hand-over, but the minibatch is DRAWN on the device from a resident packed-row replay store
 * (rows of [s(S) | r | s'(S) | d | a(A)], the wire format of por_train.py:74-78): row i of the batch is
 * store row perm_{seed,step}(i) for a keyed bijection perm of [0, n_rows) — `batch` distinct rows, i.e.
 * np.random.choice(size, B, replace=False) semantics (buffer/replay_buffer.py:64) without the O(N)
 * host permutation or any host->device copy.  One kernel does draw + gather + split.  The policy target
 * is s' (target_is_action = 0, POR) or the action columns (1, SORL).  idx_out (batch int64) may be NULL. */
int porl_iql_load_batch_sampled(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride,
                                int64_t n_rows, int32_t act_dim, int32_t target_is_action,
                                uint64_t seed, uint64_t step, int64_t* idx_out, void* stream);

/* porl_iql_load_batch for rows idx[0..batch) of a packed store [s(state_dim) | r | s'(state_dim) | d | a(act_dim)]:
 * r, d and the policy target (s' if !target_is_action, else the action columns) come from the rows; observations
 * and next observations come from obs_feat / next_feat (batch, cfg.obs_dim) when given (encoder features), or from
 * the rows themselves when both are NULL (then state_dim must equal cfg.obs_dim).  clamp_target_gt8: stage target
 * values > 8 as 0 (POR with a backbone regresses the next state as the encoder's clamp leaves it, por.py:75-79).
 * Honours PORL_IQL_MODE_TWO_SLOTS and resets the same per-batch flags as porl_iql_load_batch_sampled.  The store is
 * only read.  Contract for idx as porl_gather_rows: 0 <= idx[b] < n_rows is the caller's; duplicates are allowed. */
int porl_iql_load_batch_indexed(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                                const int64_t* idx, int32_t state_dim, int32_t act_dim, int32_t target_is_action,
                                int32_t clamp_target_gt8, const float* obs_feat, int64_t obs_rs,
                                const float* next_feat, int64_t next_rs, void* stream);

/* Execution mode of the phase calls (default 0).
 *   PORL_IQL_MODE_TWO_SLOTS   : the minibatch staging buffers the policy phase reads (s, policy target, TD target)
 *       exist PORL_IQL_SLOTS times and every porl_iql_load_batch* call moves to the next copy.  The policy phase of
 *       update t may then run on a second stream while updates t+1 .. t+PORL_IQL_SLOTS-1 are loaded and their value
 *       phases run (a load must only wait for the policy phase PORL_IQL_SLOTS updates back): the caller orders
 *       value_apply(t) -> policy_backward(t) and policy_apply(t) -> value_apply(t+1) with events (the policy phase
 *       reads the value parameters of update t; everything else it touches is private to it).  The reference runs
 *       the two phases back to back (agent/por.py:81-110); results are identical, only completion order differs.
 *   PORL_IQL_MODE_FOLD_COMBINE: *_backward leaves its split-K slabs / per-block partial sums uncombined and
 *       *_apply combines them inside the Adam launch (one launch less per phase).  grads_* are complete only after
 *       *_apply; a data-parallel caller that all-reduces grads_* between the two calls must not set it. */
#define PORL_IQL_SLOTS 3           /* copies of the staging buffers in PORL_IQL_MODE_TWO_SLOTS (name kept from ABI 3 drafts) */
#define PORL_IQL_MODE_TWO_SLOTS 1
#define PORL_IQL_MODE_FOLD_COMBINE 2
/*   PORL_IQL_MODE_SHORT_BLOCKS : the big products use 64x64 tiles (3 short blocks per CU) instead of 64x128 / 128x128.
 *       Alone on the chip they are ~10 % slower, but kernels of a second stream are only placed when blocks retire, so
 *       this is what lets the policy phase of a pipelined caller actually run beside the value phase. */
#define PORL_IQL_MODE_SHORT_BLOCKS 4
int porl_iql_set_mode(porl_iql* h, int32_t mode);

/* Redirect where the next updates write their 3 loss statistics (>= 8 floats, 16-byte aligned): lets a
 * training loop keep a device-side loss history without copies or host syncs. */
int porl_iql_set_stats(porl_iql* h, float* stats);

/* How the last Adam launch of `group` (0 = value, 1 = policy) dealt with the combine jobs handed to it (read-only; all
 * zero before the group's first launch, and for a launch without pending jobs):
 *   out[0] jobs summed inside the float4 sweep (regions),  out[1] / out[2] jobs folded as reduce+Adam blocks at width
 *   32 / width 4,  out[3] jobs outside the gradient buffer (loss statistics: plain reduce blocks),  out[4] ranges the
 *   sweep skips,  out[5] reduce blocks in front of the sweep blocks. */
int porl_iql_adam_plan(const porl_iql* h, int group, int32_t out[6]);

typedef struct porl_iql_hyper {
  float tau;         /* expectile                                   */
  float discount;    /* gamma                                       */
  float alpha;       /* advantage temperature                       */
  float inv_batch;   /* 1/B_global: a data-parallel shard passes 1/(world*B_local) */
  int32_t value_step;   /* Adam step counter t >= 1 of the value optimizer for this update  */
  int32_t policy_step;  /* ditto for the policy optimizer                                   */
  int32_t reserved;
  /* torch keeps these as Python doubles and rounds derived quantities (1-beta, lr/bias_correction) to
   * fp32 once; they are doubles here so that the same roundings happen */
  double ema_beta;   /* Polyak coefficient (por.py:31, beta=0.005)  */
  double value_lr;   /* constant (no schedule on the value optimizer) */
  double policy_lr;  /* CosineAnnealingLR value for THIS update (host-computed, Appendix A.3) */
  double adam_beta1, adam_beta2, adam_eps;   /* torch defaults 0.9, 0.999, 1e-8 */
} porl_iql_hyper;

/* por.py:81-89 — target-V forward, TD target, twin forward, expectile loss, backward.
 * Leaves dL/dtheta in grads_vf and stats[0] = this rank's share of v_loss.  (A data-parallel
 * caller all-reduces grads_vf and stats[0] here.) */
int porl_iql_value_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream);
/* por.py:90-93 — Adam on vf, then v_target <- (1-beta) v_target + beta vf, one fused sweep. */
int porl_iql_value_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream);
/* por.py:97-108 — second twin forward with the updated vf, advantage weights, policy forward,
 * weighted NLL, backward.  Leaves grads_pol, stats[1] = g_loss share, stats[2] = min NLL. */
/* optional, before porl_iql_policy_backward on the same batch: the policy MLP's forward (independent of the value
 * networks), e.g. while the value-gradient all-reduce is in flight; policy_backward then skips it */
int porl_iql_policy_prefetch(porl_iql* h, void* stream);
/* optional: the forward half of porl_iql_policy_backward on its own — second twin forward, policy forward, weights,
 * NLL and dL/dmean, i.e. every read of the VALUE parameters the policy phase makes.  A pipelined caller records its
 * "value parameters may change again" event right after it; porl_iql_policy_backward then only runs the rest. */
int porl_iql_policy_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream);
int porl_iql_policy_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream);
/* por.py:109 — Adam on the policy (lr = hp->policy_lr). */
int porl_iql_policy_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream);
/* The four phases back to back (single-GPU update; batch must have been loaded). */
int porl_iql_step(porl_iql* h, const porl_iql_hyper* hp, void* stream);
/* Policy-only step: the policy phase of two-phase SORL training with FROZEN value nets — reference agent/sorl.py:154-176
 * (SORL.policy_update) with the TD target of sorl.py:85-89, which that method uses without assigning it.  For the loaded
 * batch: the target twin on s' and the online twin on s run forward-only beside the policy MLP (five nets per layer in
 * one launch, no V-net activation kept), one head kernel turns their scalar outputs into
 *     target_v = r + (1 - d) * discount * min(target),  adv = target_v - min(online),
 *     weight   = min(exp(alpha * adv), 100)   (cfg.weight_mode 1)   or   min(exp(adv / alpha), 100)   (weight_mode 0),
 * then the weighted NLL, its backward and Adam on the policy as in the joint update (hp->policy_lr, hp->policy_step).
 * Writes grads_pol, params_pol, adam_*_pol, stats[1] = g_loss share, stats[2] = min NLL; params_vf, params_tgt,
 * grads_vf, adam_*_vf and stats[0] are not written.  Errors as porl_iql_step (unbound engine, no batch loaded, no
 * policy target in the batch: an error code, nothing launched).
 *   porl_iql_policy_only_step    : the whole step in one call, combines folded into the Adam launch.
 *   porl_iql_policy_only_forward : its forward half; porl_iql_policy_backward and porl_iql_policy_apply on the same
 *       batch complete it (a data-parallel caller all-reduces grads_pol between those two). */
int porl_iql_policy_only_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream);
int porl_iql_policy_only_step(porl_iql* h, const porl_iql_hyper* hp, void* stream);

/* Goal-conditioned behaviour cloning — the action policy pi(a | s, g) of POR and RvS, reference agent/por.py:178-183:
 *     policy(concat([obs, goal], dim=1)),  mean(-log_prob(actions)),  Adam.
 * The engine is created with cfg.obs_dim = S + G and cfg.pol_out_dim = A; its value nets are not used.
 *
 * The two loaders stage, in ONE launch (one wave per batch row), straight into the engine's staging buffers
 *     input  row i = [ obs (S) | goal (G) | 0 padding ],   target row i = [ action (A) | 0 padding ],   weight i = 1.0f
 * so there is no concatenated tensor and no staging copy, and the NLL kernel runs unchanged on unit weights.
 *   porl_iql_load_batch_cat   : dense or strided tensors obs (batch, S = cfg.obs_dim - goal_dim), goals (batch, goal_dim),
 *       actions (batch, cfg.pol_out_dim); *_rs are row strides in floats, columns have unit stride.
 *   porl_iql_load_batch_pairs : rows of a packed store [s(state_dim) | r | s' | d | a(act_dim)].  Row `start` gives s and a,
 *       row `goal` gives columns [goal_col, goal_col + goal_dim), which must lie in the state part of a row
 *       (goal_col + goal_dim <= 2*state_dim + 2).  Which rows:
 *         start and goal given (int64, batch each)  : those pairs; duplicates and goal == start are allowed;
 *         start given, goal NULL                     : the goal row is the start row (goal_col = state_dim + 1: POR's [s | s']);
 *         start NULL, ep_starts / ep_lengths given   : hindsight pairs drawn in the kernel with porl_hindsight_pairs' counter
 *                                                      stream — the same (seed, step) gives its pairs, index for index;
 *         start NULL, no table                       : `batch` distinct rows by the keyed permutation of
 *                                                      porl_iql_load_batch_sampled (seed, step); goal row = start row.
 *       start_out / goal_out (batch int64, optional) receive the rows used.  A row number outside [0, n_rows) is not
 *       read: that batch row is staged as NaN (porl_gather_pairs' rule) and the loss comes out NaN.
 * Both honour PORL_IQL_MODE_TWO_SLOTS.  Every argument is judged before the first device call.
 *
 *   porl_iql_bc_step    : por.py:178-183 on the staged batch — the policy net's hidden layers (one net per launch), mean,
 *       NLL with the unit weights, the policy phase's gradient half, Adam with the combine folded in (2 L + 4 launches at
 *       n_hidden = L).  Reads hp->policy_lr, policy_step, inv_batch and the Adam constants; writes params_pol, grads_pol,
 *       adam_*_pol, stats[1] = the loss, stats[2] = min NLL; nothing of group 0, of the target net, or stats[0].
 *   porl_iql_bc_forward : its forward half (up to NLL, dL/dmean and the loss partials); porl_iql_policy_backward on the
 *       same batch completes it without an apply (grads_pol, stats[1], stats[2]) and porl_iql_policy_apply applies it.
 * A goal-conditioned batch carries no next observations, rewards or flags: every other phase call on it returns
 * PORL_ERR_INVALID and launches nothing, and so do the bc calls on a batch staged by any other loader. */
int porl_iql_load_batch_cat(porl_iql* h, int32_t batch, const float* obs, int64_t obs_rs, const float* goals,
                            int64_t goals_rs, int32_t goal_dim, const float* actions, int64_t act_rs, void* stream);
int porl_iql_load_batch_pairs(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                              int32_t state_dim, int32_t act_dim, int32_t goal_col, int32_t goal_dim,
                              const int64_t* start, const int64_t* goal, const int64_t* ep_starts,
                              const int64_t* ep_lengths, int64_t n_episodes, uint64_t seed, uint64_t step,
                              int64_t* start_out, int64_t* goal_out, void* stream);
int porl_iql_bc_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream);
int porl_iql_bc_step(porl_iql* h, const porl_iql_hyper* hp, void* stream);

/* Forward-only paths: TwinV.both (value_functions.py:38-39) on vf (which=0) or the target (which=1),
 * and the policy mean (policy.py:19 / sorl.py:71-76).  x is (batch, obs_dim) with row stride x_rs. */
int porl_iql_forward_value(porl_iql* h, int which, const float* x, int64_t x_rs, int32_t batch,
                           float* v1_out, float* v2_out, void* stream);
int porl_iql_forward_policy(porl_iql* h, const float* x, int64_t x_rs, int32_t batch, float* mean_out,
                            int64_t mean_rs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Discrete-action Q-network engine: CQL(H) on a plain-DQN TD target
 * (CQLTrainer.learn / compute_cql_penalty, src/porl/train/cql_trainer.py:60-124; QNetwork,
 * src/porl/net/q_network.py:8-30; hard target sync, src/porl/train/dqn_trainer.py:195-196).
 * --------------------------------------------------------------------------------------------- */
typedef struct porl_qnet_cfg {
  int32_t state_dim;
  int32_t n_actions;                 /* outputs, <= 4096.  Up to 128 outputs (and every other width <= 128, <= 5 Linear
                                      * layers, the LDS plan fits: porl_qnet_one_launch) the learn step runs on the
                                      * one-launch kernels; wider output layers take the multi-launch path.  Both are
                                      * tested per row against an fp64 step up to 128 outputs, the multi-launch path at
                                      * 129 as well (tests/test_qstep_gpu.py). */
  int32_t n_hidden;                  /* QNetwork default: 3 */
  int32_t hidden[PORL_MAX_HIDDEN];   /* QNetwork default: 64, 128, 64 */
  int32_t max_batch;
} porl_qnet_cfg;

typedef struct porl_qnet porl_qnet;

typedef struct porl_qnet_buffers {
  float* params;      /* online net, porl_qnet_param_floats() floats: per Linear weight (out,in), bias (out) */
  float* params_tgt;  /* target net, same layout */
  float* grads;
  float* adam_m;
  float* adam_v;
  float* workspace;   /* porl_qnet_workspace_floats() floats */
  float* stats;       /* >= 8 floats: [0] loss, [1] td loss, [2] cql penalty */
} porl_qnet_buffers;

typedef struct porl_qnet_hyper {
  float gamma;        /* discount */
  float alpha;        /* penalty weight (cql_trainer.py:42, default 1) */
  float inv_batch;    /* 1/B_global */
  int32_t step;       /* Adam step counter t >= 1 */
  double lr;          /* dqn_trainer.py:71: 5e-4 */
  double adam_beta1, adam_beta2, adam_eps;
} porl_qnet_hyper;

int porl_qnet_create(const porl_qnet_cfg* cfg, porl_qnet** out);
void porl_qnet_destroy(porl_qnet* h);
/* Flat parameter group = per Linear layer an IMAGE of round32(out) rows x (round16(in) + 4) floats with the (out, in)
 * weight matrix in its top-left corner and zeros elsewhere, followed by round32(out) bias floats (zero padded): the
 * step kernel stages a layer into LDS with one linear copy.  tensor_info gives, for tensor `index` (weights and
 * biases alternate), its float offset, shape (rows == 0: a vector of `cols`) and the row stride of a weight matrix. */
int64_t porl_qnet_param_floats(const porl_qnet* h);
int32_t porl_qnet_tensors(const porl_qnet* h);
int porl_qnet_tensor_info(const porl_qnet* h, int index, int64_t* offset, int32_t* rows, int32_t* cols,
                          int32_t* row_stride);
int64_t porl_qnet_workspace_floats(const porl_qnet* h);
int porl_qnet_bind(porl_qnet* h, const porl_qnet_buffers* bufs);
/* The five tensors ReplayBuffer.sample returns (buffer/replay_buffer.py:53-75); *_rs = row / element
 * strides; actions are int64.  Any of actions / rewards / next_states / dones may be NULL for
 * forward-only use. */
int porl_qnet_load_batch(porl_qnet* h, int32_t batch, const float* states, int64_t s_rs,
                         const int64_t* actions, int64_t a_rs, const float* rewards, int64_t r_rs,
                         const float* next_states, int64_t n_rs, const float* dones, int64_t d_rs,
                         void* stream);
/* cql_trainer.py:94-111: both forwards, TD + penalty, backward -> grads, stats[0..2]. */
int porl_qnet_cql_backward(porl_qnet* h, const porl_qnet_hyper* hp, void* stream);
/* cql_trainer.py:112-113: Adam step. */
/* Building blocks for losses computed outside the engine (QR-DQN, C51 — porl_qr_loss / porl_c51_loss below): forward of
 * the online (which_params 0) / target (1) network on the loaded batch's states (which_input 0) / next states (1) into
 * out (batch, n_actions) [here n_actions = all outputs, e.g. actions x quantiles]; keep != 0 retains the activations
 * for porl_qnet_backward, which back-propagates a caller-supplied dL/d(output) and leaves the complete gradient in
 * `grads` (porl_qnet_apply then runs Adam). */
int porl_qnet_forward_loaded(porl_qnet* h, int which_params, int which_input, int keep, float* out, int64_t out_rs,
                             void* stream);
int porl_qnet_backward(porl_qnet* h, const float* dout, int64_t dout_rs, void* stream);

/* QR-DQN quantile-Huber loss (src/porl/train/qr_dqn_trainer.py:97-205): rows of (n_actions, n_quantiles) quantile values
 * with row stride ld; dz_out = dL/d(z_cur) for loss = mean_b row_loss[b] (1/batch already applied), row_loss (batch,). */
int porl_qr_loss(const float* z_cur, const float* z_next_online, const float* z_next_target, int64_t ld,
                 const int64_t* actions, const float* rewards, const float* dones, int32_t batch, int32_t n_actions,
                 int32_t n_quantiles, float gamma, float kappa, float* dz_out, float* row_loss, void* stream);
/* IQN quantile-Huber loss head only (src/porl/train/iqn_trainer.py:136-149): current (batch, n_current) quantile values
 * of the taken actions at fractions taus (batch, n_current), target (batch, n_target) Bellman targets; dcurrent_out =
 * dL/dcurrent for loss = mean_b row_loss[b].  (Upstream's IQNTrainer / IQNNetwork pair cannot run as shipped:
 * porl_amd/train/iqn_trainer.py states how learn() is read.) */
int porl_iqn_quantile_huber(const float* current, const float* target, const float* taus, int32_t batch, int32_t n_current,
                            int32_t n_target, float kappa, float* dcurrent_out, float* row_loss, void* stream);
/* The parts of an Implicit Quantile Network step that are not Linear layers (src/porl/net/iqn_network.py:35-91,
 * src/porl/train/iqn_trainer.py:92-134; csrc/iqn.hpp).  Row-major fp32, `n_tau` quantile fractions per sample.
 *   cos_embed        out (n, E): cos(pi * i * taus[r]), i = 1..E                                   iqn_network.py:74-91
 *   hadamard         out (batch*n_tau, H) = feat[b, :] (row stride ldf) * emb (batch*n_tau, H)     iqn_network.py:58-62
 *   hadamard_backward  dfeat (batch, H) = sum_n dout * emb, demb = dout * feat; either may be null
 *   select / scatter   out (batch, n_tau) = z[b, n, actions[b]] and its adjoint dz (batch, n_tau, A) iqn_trainer.py:101-103
 *   target           a* = argmax_a mean_n z_online_next[b, n, a]; td (batch, n_tau) = r + gamma * z_target_next[b, n, a*] *
 *                    (1 - done); next_actions (batch,) optional                                     iqn_trainer.py:108-121 */
int porl_iqn_cos_embed(const float* taus, int64_t n, int32_t embedding_dim, float* out, void* stream);
int porl_iqn_hadamard(const float* feat, int64_t ldf, const float* emb, int32_t batch, int32_t n_tau, int32_t width,
                      float* out, void* stream);
int porl_iqn_hadamard_backward(const float* dout, const float* feat, int64_t ldf, const float* emb, int32_t batch,
                               int32_t n_tau, int32_t width, float* dfeat, float* demb, void* stream);
int porl_iqn_select(const float* z, const int64_t* actions, int32_t batch, int32_t n_tau, int32_t n_actions, float* out,
                    void* stream);
int porl_iqn_scatter(const float* dsel, const int64_t* actions, int32_t batch, int32_t n_tau, int32_t n_actions, float* dz,
                     void* stream);
int porl_iqn_target(const float* z_online_next, const float* z_target_next, const float* rewards, const float* dones,
                    float gamma, int32_t batch, int32_t n_tau, int32_t n_actions, float* td, int64_t* next_actions,
                    void* stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) on one flat gradient buffer (iqn_trainer.py:131): norm_coef[0] = the
 * total 2-norm, norm_coef[1] = min(1, max_norm / (norm + 1e-6)), grads scaled in place.  workspace: >= 256 doubles. */
int porl_grad_clip(float* grads, int64_t n, float max_norm, float* norm_coef, double* workspace, void* stream);
/* C51 projection + cross-entropy (src/porl/train/c51_trainer.py:52-174) on PRE-softmax outputs (the log_softmax of
 * categorical_q_network.py:76-78 is applied inside, to both networks' rows). */
int porl_c51_loss(const float* logits_cur, const float* logits_next_target, int64_t ld, const int64_t* actions,
                  const float* rewards, const float* dones, const float* support, int32_t batch, int32_t n_actions,
                  int32_t n_atoms, float gamma, float v_min, float v_max, float* dlogits_out, float* row_loss, void* stream);
/* out[0] = mean(x[0..n)) with a fixed summation order (loss reporting). */
int porl_reduce_mean(const float* x, int32_t n, float* out, void* stream);

int porl_qnet_apply(porl_qnet* h, const porl_qnet_hyper* hp, void* stream);
int porl_qnet_learn(porl_qnet* h, const porl_qnet_hyper* hp, void* stream);   /* the two above */
/* target_network.load_state_dict(q_network.state_dict()) */
/* 1 when the network fits the one-launch step kernel (porl_qnet_learn_indexed and the fast path of
 * porl_qnet_cql_backward), else 0 */
int32_t porl_qnet_one_launch(const porl_qnet* h);
/* learn() on the minibatch { row idx[b] (or b when idx is NULL) of the given replay arrays : b < batch } without
 * materialising it: the gather of ReplayBuffer.sample (buffer/replay_buffer.py:64-73) happens inside the step
 * kernel.  Only for networks the one-launch kernel covers (every layer <= 128 wide, <= 5 Linear layers);
 * PORL_ERR_UNSUPPORTED otherwise.  actions int64, dones fp32 (1.0 = terminal). */
int porl_qnet_learn_indexed(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions,
                            const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                            const int64_t* idx, int32_t batch, const porl_qnet_hyper* hp, void* stream);
/* porl_qnet_learn_indexed with the loss of src/porl/train/dqn_per_trainer.py:75-123: Double-DQN target
 * (argmax by the online net, value by the target net), importance-sampling weights, |TD error| per sample for the
 * priority write-back.  Use hp->alpha = 0 for plain (un-regularised) DQN.  The reference multiplies a (B,1) weight
 * tensor with a (B,) error tensor, i.e. its loss is mean(w) * mean(td^2): pass that mean as `uniform_weight`
 * (device scalar) to reproduce it, or `is_weights` (B,) for per-sample weighting; either may be NULL. */
typedef struct porl_qnet_variant {
  int32_t double_dqn;
  const float* is_weights;
  const float* uniform_weight;
  float* td_abs;
  /* BCQ (src/porl/policy/bcq.py:59-74): (batch, n_actions) fp32 0/1 mask of the actions the behaviour policy allows in
   * s', row b for minibatch position b; the bootstrap action is argmax_a [Q_target(s',a) + (mask - 1) * 1e10] and is
   * valued by Q_target.  NULL = off. */
  const float* next_mask;
  /* 1: drop the TD term; with hyper.alpha = 1 the loss is the cross-entropy of softmax(Q(s)) against the taken
   * action minus ln(n_actions) — the behaviour-policy pre-training step of bcq.py:23-47 on a "Q" network that holds
   * the behaviour policy's logits. */
  int32_t td_off;
} porl_qnet_variant;
/* learn() on B distinct rows drawn INSIDE the step kernel: batch row b is row perm_{seed,draw}(b) of the n_rows-row replay
 * arrays, the keyed permutation of porl_sample_indices (same indices, no sampler launch, no index buffer).  Replaces
 * ReplayBuffer.sample + learn (buffer/replay_buffer.py:64, cql_trainer.py:88-124) for device-resident buffers.
 * porl_qnet_can_sample: 1 when the engine's network runs on the two-group one-launch kernel. */
int32_t porl_qnet_can_sample(const porl_qnet* h);
int porl_qnet_learn_sampled(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                            const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, uint64_t seed,
                            uint64_t draw, int32_t batch, const porl_qnet_hyper* hp, void* stream);
int porl_qnet_learn_variant(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions,
                            const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                            const int64_t* idx, int32_t batch, const porl_qnet_hyper* hp,
                            const porl_qnet_variant* variant, void* stream);
/* porl_qnet_learn_sampled with a porl_qnet_variant (non-NULL): the rows are drawn inside the step kernel and the variant's
 * loss is applied to them — td_off for the behaviour-policy pre-training of bcq.py:23-47, next_mask / is_weights /
 * td_abs indexed by minibatch position as in porl_qnet_learn_variant. */
int porl_qnet_learn_sampled_variant(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions,
                                    const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                                    int64_t n_rows, uint64_t seed, uint64_t draw, int32_t batch, const porl_qnet_hyper* hp,
                                    const porl_qnet_variant* variant, void* stream);
/* Discrete BCQ (src/porl/policy/bcq.py:50-86) from one call.  `beh` is a second engine that holds the behaviour policy
 * (src/porl/net/behavior_policy.py) as its online parameters; it must agree with `h` on state_dim and n_actions.
 *   porl_qnet_bcq_mask: mask_out[b, j] = softmax(beh(next_states[idx[b]]))[j] > threshold ? 1 : 0, (batch, n_actions)
 *     fp32 by minibatch position — one launch (csrc/bcq_mask.hpp) when porl_qnet_one_launch(beh), else gather, one launch
 *     per layer and porl_softmax_mask's kernel.  Nothing past batch * n_actions floats is written.
 *   porl_qnet_bcq_learn: that mask into h's workspace, then porl_qnet_learn_variant on rows idx with next_mask set
 *     (one-launch step kernel + reduction/Adam, or the multi-launch path for wide Q networks).  A row whose mask is all
 *     zero bootstraps from action 0, as torch.argmax does on the tie.
 *   porl_qnet_bcq_learn_sampled: the same with batch row b = row perm_{seed,draw}(b) of [0, n_rows) drawn inside both
 *     kernels (porl_sample_indices' permutation); needs porl_qnet_can_sample(h), else PORL_ERR_UNSUPPORTED.
 * Null pointers, batch outside [1, max_batch] of either engine, engines that disagree on state_dim / n_actions, row
 * strides below state_dim and a non-finite threshold are PORL_ERR_INVALID, checked before anything is launched. */
int porl_qnet_bcq_mask(porl_qnet* beh, const float* next_states, int64_t n_rs, const int64_t* idx, int32_t batch,
                       float threshold, float* mask_out, void* stream);
int porl_qnet_bcq_learn(porl_qnet* h, porl_qnet* beh, const float* states, int64_t s_rs, const int64_t* actions,
                        const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                        const int64_t* idx, int32_t batch, const porl_qnet_hyper* hp, float threshold, void* stream);
int porl_qnet_bcq_learn_sampled(porl_qnet* h, porl_qnet* beh, const float* states, int64_t s_rs, const int64_t* actions,
                                const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                                int64_t n_rows, uint64_t seed, uint64_t draw, int32_t batch, const porl_qnet_hyper* hp,
                                float threshold, void* stream);
/* One learn step of a distributional trainer (src/porl/train/qr_dqn_trainer.py:97-222, c51_trainer.py:52-174) on the
 * minibatch { row idx[b] (or b when idx is NULL) of the given replay arrays : b < batch } from one call: gather into the
 * staging buffers, the forwards as one grouped launch per layer (online net on s with its activations kept, target net
 * on s', for QR-DQN also the online net on s'), the loss head on the workspace's padded output rows writing
 * dL/d(output) where the backward chain reads it, stats[0] = batch mean of the row losses (porl_reduce_mean's order),
 * backward, Adam.  Parameters, Adam moments, row losses and the mean are bit-equal to porl_qnet_load_batch +
 * porl_qnet_forward_loaded + porl_qr_loss / porl_c51_loss + porl_qnet_backward + porl_qnet_apply + porl_reduce_mean on
 * the same rows.  hp->gamma, inv_batch (unused: 1/batch is applied), step, lr, adam_*: as porl_qnet_apply.
 * head: kind PORL_DIST_QR (n_sub quantiles per action, kappa) or PORL_DIST_C51 (n_sub >= 2 atoms, v_min < v_max,
 * support = n_sub device floats); n_actions * n_sub must equal the engine's outputs, n_sub <= 256.  Every argument is
 * checked before the first launch. */
#define PORL_DIST_QR 0
#define PORL_DIST_C51 1
typedef struct porl_dist_head {
  int32_t kind;
  int32_t n_actions;
  int32_t n_sub;
  float kappa;
  float v_min, v_max;
  const float* support;
} porl_dist_head;
int porl_qnet_dist_learn(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                         const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                         const porl_qnet_hyper* hp, const porl_dist_head* head, void* stream);
/* porl_qnet_dist_learn on `batch` distinct rows of the first n_rows rows of the replay arrays: row b is position b of the
 * keyed permutation (seed, draw) of [0, n_rows), the rows porl_sample_indices(n_rows, batch, seed, draw) writes, drawn
 * inside the gather launch — no index array and no extra launch; bit-equal to porl_sample_indices followed by
 * porl_qnet_dist_learn.  batch <= n_rows <= 2^40.  Every argument is checked before the first launch. */
int porl_qnet_dist_learn_sampled(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                                 const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, uint64_t seed,
                                 uint64_t draw, int32_t batch, const porl_qnet_hyper* hp, const porl_dist_head* head,
                                 void* stream);
int porl_qnet_sync_target(porl_qnet* h, void* stream);
/* q_network(states) (which=0) or target_network(states) (which=1) -> (batch, n_actions) */
int porl_qnet_forward(porl_qnet* h, int which, const float* states, int64_t s_rs, int32_t batch,
                      float* q_out, int64_t q_rs, void* stream);
/* compute_cql_penalty(states, actions) -> out[0] (device float) */
int porl_qnet_penalty(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions,
                      int64_t a_rs, int32_t batch, float* out, void* stream);

/* Online loop (src/porl/train/dqn_trainer.py:119-180): one launch per recorded transition, one per greedy action.
 *
 * porl_qnet_record: replay_buffer.push(state, action, reward, next_state, done) into slot `slot` of a device replay
 * mirror (the five arrays of buffer/replay_buffer.py; states rows of state_dim floats, actions int64).  The transition
 * is copied into the kernel's arguments at launch, so `state` / `next_state` (host, state_dim floats each) may be
 * reused as soon as the call returns.  state_dim <= PORL_RECORD_MAX_STATE, else PORL_ERR_UNSUPPORTED. */
#define PORL_RECORD_MAX_STATE 480
typedef struct porl_qnet_mirror {
  float* states;
  float* next_states;
  int64_t* actions;
  float* rewards;
  float* dones;
  int64_t capacity;                  /* rows of each array */
} porl_qnet_mirror;
int porl_qnet_record(porl_qnet* h, int64_t slot, const float* state, const float* next_state, int64_t action,
                     float reward, float done, const porl_qnet_mirror* mirror, void* stream);

/* porl_qnet_act: argmax_a Q(s_b, a) for batch (1..8) states with the online (which 0) or target (1) parameters, in
 * one workgroup.  States: rows [row, row + batch) of a device array of n_rows rows (row stride s_rs), or, when
 * `states` is NULL, batch x state_dim floats of host memory `inline_states` (<= 256 floats) copied into the kernel's
 * arguments.  Epilogue: kind 0 argmax over the n_actions outputs; 1 C51, outputs (n_act, n_sub) logits, argmax of
 * sum_i softmax(logits)_i support[i]; 2 QR, outputs (n_act, n_sub) quantiles, argmax of their mean.  Ties go to the
 * lowest index (torch.argmax).  `out` = a 16-word record in device or pinned host memory: int32 actions at [0, batch),
 * at [8, 8 + n_stats) fp32 copies of stats[0, n_stats) (NULL stats: the engine's own loss statistics, n_stats <= 3)
 * taken in stream order, i.e. after the step launched before.
 * porl_qnet_act_ok: 1 when the network suits one workgroup (every layer <= 1024 wide and <= 2^19 padded parameter
 * floats, i.e. <= 2 MiB streamed by one CU), else 0 and porl_qnet_act returns PORL_ERR_INVALID. */
typedef struct porl_qnet_act_src {
  int32_t batch;
  const float* states;
  int64_t s_rs;
  int64_t row;
  int64_t n_rows;
  const float* inline_states;
} porl_qnet_act_src;
typedef struct porl_qnet_act_epilogue {
  int32_t kind;
  int32_t n_act;
  int32_t n_sub;
  const float* support;
  const float* stats;
  int32_t n_stats;
} porl_qnet_act_epilogue;
int32_t porl_qnet_act_ok(const porl_qnet* h);
int porl_qnet_act(porl_qnet* h, int which, const porl_qnet_act_src* src, const porl_qnet_act_epilogue* epi,
                  int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * IQN engine: IQNTrainer.learn (src/porl/train/iqn_trainer.py:92-134) and its greedy action (:82-91) on
 * IQNNetwork(state, actions, embedding_dim, hidden) (src/porl/net/iqn_network.py:10-62) from one call each.
 * The engine owns no parameters: it binds to flat buffers that hold the network's ten tensors in
 * parameters() order — feature_net.0 w/b, feature_net.2 w/b, quantile_embedding w/b, value_net.0 w/b,
 * value_net.2 w/b — each dense row-major (out, in) at cfg.offset[i] floats (a multiple of 4; gaps are
 * never written), n_params floats per buffer.  Limits: embedding_dim <= 128, n_actions <= 64, max_tau
 * (fractions per state) <= 256, else PORL_ERR_UNSUPPORTED.
 * porl_iqn_learn: rows idx[b] (NULL: rows 0..batch-1) of the replay arrays; taus_prime (batch, n_cur) and
 *   taus_dprime (batch, n_tgt) dense on the device.  Gather, the three forwards grouped per layer, loss head, mean loss
 *   -> stats[0], backward into `grads` (every tensor stored whole), clip_grad_norm_(max_norm) with the total norm ->
 *   stats[1] and the coefficient -> stats[2], Adam.  No host synchronisation.  A row whose action is outside
 *   0..n_actions-1 contributes no gradient and makes stats[0] NaN.
 * porl_iqn_act: greedy action of ONE state (src->batch == 1; a row of a device array or inline, <= 256 floats) under
 *   n_tau fractions `taus` (device): argmax_a mean_n Z(s, tau_n)[a], first maximum.  `record` as porl_qnet_act's:
 *   int32 action at word 0, fp32 stats[0, n_stats) at words 8.., device or pinned host memory.  which: 0 online, 1 target.
 * porl_iqn_mix / porl_iqn_head: the two fused kernels of the step on their own (tests).  mix: out[(b, n), :] =
 *   feat[b, :] * (cos(pi i tau[b, n])_{i=1..E} . weight^T + bias) for 1..3 problems in one launch, emb (optional) = the
 *   factor in brackets.  head: Double-DQN choice on the tau''-mean of z_online_next, Bellman targets from z_target_next,
 *   quantile-Huber loss of the taken action's quantiles of z_cur against them; z rows (batch * n, ld); dz (batch * n_cur,
 *   ld) = dL/dz_cur for the batch-mean loss, row_loss (batch), next_actions (batch, optional).
 * The entry points of the vectorised loop (N robots per step, nothing read back; csrc/iqn_vector.hpp) follow
 *   porl_iqn_head below, each with its own comment.
 * --------------------------------------------------------------------------------------------- */
#define PORL_IQN_TENSORS 10
typedef struct porl_iqn porl_iqn;
typedef struct porl_iqn_cfg {
  int32_t state_dim, n_actions, embedding_dim, hidden;
  int32_t max_batch, max_tau;
  int64_t offset[PORL_IQN_TENSORS];
  int64_t n_params;
} porl_iqn_cfg;
typedef struct porl_iqn_buffers {
  float* params;
  float* params_tgt;
  float* grads;
  float* adam_m;
  float* adam_v;
  float* workspace;
  float* stats;               /* >= 8 floats */
} porl_iqn_buffers;
typedef struct porl_iqn_hyper {
  float gamma, kappa, max_norm;
  int32_t step;               /* Adam step count of this update, >= 1 */
  double lr, adam_beta1, adam_beta2, adam_eps;
} porl_iqn_hyper;
typedef struct porl_iqn_mix_prob {
  const float* feat;          /* (batch, hidden), row stride ldf */
  int64_t ldf;
  const float* taus;          /* (batch * n_tau) */
  const float* weight;        /* (hidden, embedding_dim), row stride ldw */
  int64_t ldw;
  const float* bias;          /* (hidden) */
  float* out;                 /* (batch * n_tau, hidden), row stride ldo */
  int64_t ldo;
  float* emb;                 /* like out, or NULL */
  int32_t batch, n_tau;
} porl_iqn_mix_prob;
int porl_iqn_create(const porl_iqn_cfg* cfg, porl_iqn** out);
void porl_iqn_destroy(porl_iqn* h);
int64_t porl_iqn_workspace_floats(const porl_iqn* h);
int porl_iqn_bind(porl_iqn* h, const porl_iqn_buffers* buffers);
int porl_iqn_learn(porl_iqn* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                   const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                   const float* taus_prime, int32_t n_cur, const float* taus_dprime, int32_t n_tgt,
                   const porl_iqn_hyper* hp, void* stream);
int porl_iqn_act(porl_iqn* h, int which, const porl_qnet_act_src* src, const float* taus, int32_t n_tau,
                 int32_t n_stats, int32_t* record, void* stream);
int porl_iqn_mix(int32_t nprob, const porl_iqn_mix_prob* probs, int32_t embedding_dim, int32_t hidden, void* stream);
int porl_iqn_head(const float* z_cur, const float* z_online_next, const float* z_target_next, int64_t ld,
                  const int64_t* actions, const float* rewards, const float* dones, const float* taus_prime,
                  int32_t batch, int32_t n_cur, int32_t n_tgt, int32_t n_actions, float gamma, float kappa, float* dz,
                  float* row_loss, int64_t* next_actions, void* stream);
/* The keyed fraction stream: out[k] = tau(seed, use, draw, first + k) for k < count, where
 *   tau(seed, use, draw, e) = (float)(sm64(key ^ sm64((draw << 32) | e)) >> 40) * 2^-24,  key = sm64(seed ^ TAG ^ use),
 * sm64 the mixer of porl_per_sample_keyed's stream and TAG = 0x30C9E7BC03E23535 (csrc/iqn_vector.hpp).  use: 0 acting, 1 tau',
 * 2 tau''.  Every value is a multiple of 2^-24 in [0, 1).  draw <= 2^32 - 1, 0 <= first, first + count <= 2^32.
 * Stand-alone: no engine; one launch. */
int porl_iqn_draw_taus(uint64_t seed, int32_t use, uint64_t draw, int64_t first, int64_t count, float* out, void* stream);
/* Epsilon-greedy over the quantile values of n robots: z (n * n_tau, ld) fp32, robot i's n_tau rows one after the other,
 * n_actions values per row (n_actions <= ld <= 128).  q[i, a] = (sum over the rows, ascending, of z[., a]) / n_tau — the
 * order in which porl_iqn_learn ranks the next state's actions — goes to q (n, n_actions) with row stride q_rs and the
 * action to out (n) int64, both always, also when the robot explores; the action is porl_qnet_select's rule on those
 * values, with the same key and draws (seed, env_offset + i, act-step t).  n_tau <= 256, n_actions <= 64, t <= 2^32 - 1.
 * Stand-alone; one launch, one wave per robot. */
int porl_iqn_select_rows(const float* z, int64_t ld, int64_t n, int32_t n_tau, int32_t n_actions, double epsilon, uint64_t seed,
                         uint64_t t, int64_t env_offset, float* q, int64_t q_rs, int64_t* out, void* stream);
/* Acting for n robots: rows of states (n, row stride s_rs) in chunks of cfg.max_batch — per chunk one staging launch
 * (states and fractions), the feature layers, the mix, the value layers and porl_iqn_select_rows' kernel on the output rows
 * where the forward left them: 7 launches.  Robot i's n_tau fractions are taus[i, :] of the caller's dense (n, n_tau)
 * array, or with taus NULL elements (env_offset + i) * n_tau + j of the acting stream (use 0) at draw t, whatever the
 * chunking; then (env_offset + n) * n_tau <= 2^32.  n_tau <= cfg.max_tau.  which: 0 online, 1 target.  q, out as
 * porl_iqn_select_rows'.  Borrows the workspace rows of the learn step's second forward. */
int porl_iqn_act_rows(porl_iqn* h, int which, const float* states, int64_t s_rs, int64_t n, const float* taus, int32_t n_tau,
                      double epsilon, uint64_t seed, uint64_t t, int64_t env_offset, float* q, int64_t q_rs, int64_t* out,
                      void* stream);
/* porl_iqn_learn on `batch` distinct rows of the first n_rows rows of the replay arrays — the rows
 * porl_sample_indices(n_rows, batch, seed, draw) writes, drawn inside the gather launch — with tau' (batch, n_cur) and
 * tau'' (batch, n_tgt) the elements b * n + j of uses 1 and 2 of the fraction stream at draw `draw`, written into the
 * workspace by one extra launch: bit-equal to porl_sample_indices, two porl_iqn_draw_taus and porl_iqn_learn.
 * batch <= n_rows <= 2^40, draw <= 2^32 - 1. */
int porl_iqn_learn_sampled(porl_iqn* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                           const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, int32_t batch,
                           uint64_t seed, uint64_t draw, int32_t n_cur, int32_t n_tgt, const porl_iqn_hyper* hp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Building blocks, exported for tests, the replay buffer and other trainers
 * --------------------------------------------------------------------------------------------- */
/* C = epilogue(op(A) * op(B)); mode 0 "NT": A (M,K), B (N,K); 1 "NN": A (M,K), B (K,N);
 * 2 "TN": A (K,M), B (K,N).  act: 0 none, 1 relu, 2 tanh.  bias (N) / mask (M,N; ld=ldmask) may be
 * NULL.  tile: 0 128x128, 1 128x64, 2 64x128, 3 64x64, -1 auto.  splitk > 1 needs `slab`
 * (splitk*M*ldc floats) and is combined in fixed order. */
int porl_gemm_f32(int mode, int tile, int32_t M, int32_t N, int32_t K,
                  const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc,
                  const float* bias, int act, const float* mask, int32_t ldmask,
                  int splitk, float* slab, void* stream);

/* One launch of 1..8 independent products on the same kernel, each with the full prologue / epilogue set the engines
 * use (csrc/gemm_f32.hpp, GemmProb).  A descriptor-level test surface: what a descriptor asks for is what one block
 * grid computes, nothing is combined afterwards.  Per problem, in this order:
 *   a(m,k)  = A, or max(A*a_colscale[k] + a_colshift[k], 0) when both are set (NT only, tiles 1, 3, 4, K % 32 == 0),
 *             or for a_grp > 0 (NT only) the gathered-patch operand: row m starts at m*lda + (m / a_grp)*a_grp_jump
 *             floats and columns from a_seg_tiles*32 on lie a_seg_jump floats further;
 *   v       = act(a.b + bias), then v = mask > 0 ? v : 0, then v = resid + rscale[(m + rs_row0) / rs_rows] * v
 *             (rscale NULL = 1; resid has C's leading dimension and may be C); v is the STORED C (store_c = 0: C is
 *             not written, the other outputs are);
 *   cstat   ((M+31)/32, 2, N): per 32-row block the column sums [rb][0][n] and sums of squares [rb][1][n] of the stored C;
 *   headout (ceil(N/32), M): headout[p][m] = sum of C(m,n)*headw[n] over the 32 columns of part p, from the stored C;
 *   colsum  (M,): TN only, sum_k A(k,m).
 * The kernel applies mask / resid after it has taken cstat / the head on some tiles, so a descriptor with (mask or
 * resid) and (cstat or headw) is refused (PORL_ERR_UNSUPPORTED) rather than computed two ways.
 * splitk > 1: C and colsum are RAW slab bases (slab s at C + s*M*ldc and colsum + s*M, s < splitk; a slab whose K
 * range is empty is written with zeros); bias, act, mask, head, resid and cstat are refused with it.
 * Leading dimensions below the contiguous extent (ldc < N, ldmask < N, lda / ldb below K, M or N by layout), negative
 * jumps of a gathered A, jumps that are no multiple of 4 floats under a 16-byte-readable A, jumps set for a dense A and
 * a non-zero `reserved` are refused as well (PORL_ERR_INVALID).
 * tile as for porl_gemm_f32 (-1 = automatic, 0..4).  single_buffer != 0 asks for the single-LDS-buffer schedule, which exists
 * on tile 3 with 16-byte-readable operands (elsewhere the usual schedule runs).  Every refusal happens on the host,
 * before anything is launched. */
typedef struct porl_gemm_desc {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* mask;
  const float* headw;
  float* headout;
  float* colsum;
  const float* a_colscale;
  const float* a_colshift;
  const float* resid;
  const float* rscale;
  float* cstat;
  int32_t mode;        /* 0 NT, 1 NN, 2 TN */
  int32_t M, N, K;
  int32_t lda, ldb, ldc, ldmask;
  int32_t act;
  int32_t rs_rows, rs_row0;
  int32_t a_grp, a_grp_jump, a_seg_tiles, a_seg_jump;
  int32_t splitk;      /* <= 1: one pass over K */
  int32_t store_c;
  int32_t reserved;    /* 0 */
} porl_gemm_desc;
int porl_gemm_f32_group(const porl_gemm_desc* probs, int32_t nprob, int tile, int single_buffer, void* stream);

/* torch.optim.Adam single-tensor arithmetic over a flat range (n multiple of 4, 16-byte aligned),
 * optionally fused with target <- (1-ema_beta) target + ema_beta p (target may be NULL). */
int porl_adam_ema(float* p, const float* g, float* m, float* v, float* target, int64_t n,
                  double lr, int32_t step, double beta1, double beta2, double eps, double ema_beta,
                  void* stream);
/* F.softmax(logits, -1) > threshold as a 0/1 fp32 mask (src/porl/net/behavior_policy.py:41-55), or the probabilities
 * themselves when write_probs == 1 (:30-39), or log_softmax when write_probs == 2: logits (batch, ld) rows, n_actions
 * columns used; mask_out
 * (batch, n_actions) dense. */
int porl_softmax_mask(const float* logits, int64_t ld, int32_t batch, int32_t n_actions, float threshold,
                      int32_t write_probs, float* mask_out, void* stream);

/* util/util.py:54-56 on its own: target <- (1 - ema_beta) * target + ema_beta * source over n floats (n % 4 == 0).
 * Same rounding as the sweep fused into porl_adam_ema. */
int porl_ema(float* target, const float* source, int64_t n, double ema_beta, void* stream);

/* out[i,:] = rows[idx[i],:] — minibatch gather from a device-resident packed-row replay store
 * (replaces the numpy fancy-index + H2D copies of ReplayBuffer.sample, buffer/replay_buffer.py:64-73). */
int porl_gather_rows(const float* rows, int64_t row_stride, const int64_t* idx, int32_t n,
                     int32_t width, float* out, int64_t out_stride, void* stream);

/* `batch` distinct indices base + perm_{seed,step}(i), i < batch, perm a keyed bijection of [0, n_rows):
 * uniform sampling WITHOUT replacement on the device (semantics of np.random.choice(size, B,
 * replace=False), buffer/replay_buffer.py:64; the stream differs from numpy's). */
int porl_sample_indices(int64_t n_rows, int32_t batch, uint64_t seed, uint64_t step, int64_t base,
                        int64_t* out, void* stream);
/* Positions first .. first+count-1 of the keyed permutation (seed, epoch) of [0, n_rows): consecutive calls walk
 * one shuffled epoch — DataLoader(shuffle=True, drop_last=False) of por_train.py:61-63 without host work; the
 * last call of an epoch simply asks for fewer rows.  out[i] = base + perm(first + i), int64. */
int porl_epoch_indices(int64_t n_rows, int64_t first, int32_t count, uint64_t seed, uint64_t epoch, int64_t base,
                       int64_t* out, void* stream);

/* state2costmap (util/costmap.py:7-64; called by FasterNet.forward_cls, agent/fasternet.py:431):
 * (batch, n_ang + 2) lidar ranges + relative goal (x, y), row stride state_rs -> out (batch, 3, n_ang, n_dist)
 * contiguous.  The reference uses n_ang = 360, n_dist = 256.  Like the reference, entries > 8 of `state` are
 * zeroed in place. */
int porl_state2costmap(float* state, int64_t state_rs, int32_t batch, int32_t n_ang, int32_t n_dist,
                       float* out, void* stream);

/* The labelling pass between the CSV shards and the value dataset (preprocess.py:11-68 `preprocessing`, planner
 * dataloader/a_star.py:8-221; CustomDataset.__init__ runs the same pass, dataloader/dataloader.py:18-30), one
 * workgroup per row with the occupancy grid and the distance field in LDS (csrc/astar.hpp).  Per row: the n_beams
 * ranges become obstacle points (beams with range_lo < d < range_hi, at beam_dirs[i] * d), the points block every
 * cell whose centre (ix * resolution + min_x, iy * resolution + min_y) lies within robot_radius, and the row is
 * labelled with the number of nodes on a cheapest 8-connected path from the cell of (0, 0) to the goal's cell,
 * goal = R(heading) (row[goal_off .. +1] - row[pose_off .. +1]).  All geometry is fp64 on the fp32 row's values.
 * The grid is round((max - min) / resolution) cells per axis; it is rejected (PORL_ERR_INVALID, before any launch)
 * when its distance field does not fit in one workgroup's LDS or a path could overflow the packed (a, b) pair. */
typedef struct porl_astar_params {
  double resolution, robot_radius;            /* reference: 0.1, 0.13 (also the row filter's threshold) */
  double min_x, max_x, min_y, max_y;          /* reference: -10, 10, -5, 5 */
  double range_lo, range_hi;                  /* reference: 0.15, 3.5 (both exclusive) */
  int32_t n_beams;                            /* reference: 360, at row[0 .. n_beams) */
  int32_t pose_off, heading_off, goal_off;    /* reference: 360 (x, y), 362, 363 (x, y) */
} porl_astar_params;

enum {
  PORL_ASTAR_LABELLED = 0,       /* value = value_table[path_len] */
  PORL_ASTAR_TOO_CLOSE = 1,      /* min(scan) < robot_radius (numpy's min: false when a beam is NaN) */
  PORL_ASTAR_GOAL_IS_START = 2,
  PORL_ASTAR_GOAL_OFF_GRID = 3,
  PORL_ASTAR_GOAL_BLOCKED = 4,
  PORL_ASTAR_UNREACHABLE = 5,
  PORL_ASTAR_NON_FINITE = 6,     /* the goal cell is not a finite number (the reference raises from round()) */
  PORL_ASTAR_NOT_CONVERGED = 7   /* the sweep bound was reached: never expected, reported instead of spinning */
};

/* rows (n_rows, >= highest offset read) fp32 with `row_stride` floats between rows; beam_dirs (n_beams, 2) fp64
 * (cos, sin) of each beam, built on the host; value_table[n] fp32 = the label of an n-node path, n_values >= cells + 2.
 * Outputs, one per row: value (0 unless labelled), path_len (a + b + 1, or 0), status (above); `sweeps` (relaxation
 * sweeps the row took) may be null.  The reference drops every row whose status is not 0. */
int porl_astar_label(const float* rows, int64_t row_stride, int64_t n_rows, const porl_astar_params* params,
                     const double* beam_dirs, const float* value_table, int32_t n_values, float* value,
                     int32_t* path_len, int32_t* status, int32_t* sweeps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory-level dataset passes (util/util.py:67-138; kernels in csrc/episodes.hpp).  A done flag is SET iff
 * d != 0.0f (NaN set, -0.0 clear: np.where(dones) / `if d`).  Flag and reward vectors are read in place through
 * (base, stride in floats, n_rows): a dense vector or one column of a packed row store.
 * --------------------------------------------------------------------------------------------- */

/* int64 words of workspace porl_episode_count / _fill need for n_rows rows (-1 when n_rows is outside [1, 2^40]);
 * also reports the scan's tile constants: rows per block and partials per sweep of the partial scan (either pointer
 * may be null). */
int64_t porl_episode_workspace(int64_t n_rows, int32_t* rows_per_block, int32_t* partials_per_sweep);

/* The episode table, first call (extract_done_makers, util/util.py:83-87; with cap > 0 the walk of return_range,
 * :67-80, where an episode also closes when ep_len == cap): counts the rows that close an episode.  On return (in stream
 * order) workspace[0] = K, the number of closed episodes, and workspace[1] = the rows after the last of them (the
 * trailing run the reference drops, :77-78).  The rest of the workspace carries the block offsets to porl_episode_fill.
 * cap 0 = none.  Separate launches (block partials, a scan of the partials, the pass proper): no block waits on
 * another.  The caller reads K back — the one synchronisation per dataset. */
int porl_episode_count(const float* flags, int64_t stride, int64_t n_rows, int64_t cap, int64_t* workspace, void* stream);

/* Second call, same flags / stride / n_rows / cap and the workspace the count left: starts[k], ends[k] (int64, k <
 * n_episodes = K) of every closed episode, ascending; starts[0] = 0, starts[k] = ends[k-1] + 1.  No store goes past
 * n_episodes entries. */
int porl_episode_fill(const float* flags, int64_t stride, int64_t n_rows, int64_t cap, const int64_t* workspace,
                      int64_t n_episodes, int64_t* starts, int64_t* ends, void* stream);

/* return_range (util/util.py:67-80): returns[k] = the fp64 sum of the fp32 rewards of rows starts[k] .. ends[k] added in
 * row order from 0.0 — bit for bit the reference's Python float.  With range_out (3 doubles) also min(returns),
 * max(returns) over the returns that are not NaN and range_out[2] = 1.0 if any return is NaN, else 0.0; range_ws is
 * then 4 * 256 int64 words of scratch. */
int porl_episode_returns(const float* rewards, int64_t stride, int64_t n_rows, const int64_t* starts, const int64_t* ends,
                         int64_t n_episodes, double* returns, int64_t* range_ws, double* range_out, void* stream);

/* _sample_indces (util/util.py:90-116): per sample i < batch a trajectory `traj` in [0, n_episodes) and u1, u2 in [0, 1);
 * t1 = floor(u1 * (lengths[traj] - 1)), t2 = floor(u2 * lengths[traj]) in fp64; start[i] = starts[traj] + min(t1, t2),
 * goal[i] = starts[traj] + max(t1, t2).  The draws are the caller's (traj, u1, u2 all non-null) or a counter-based
 * stream keyed by (seed, step, i, stream 0|1|2): x = sm64(sm64(seed ^ sm64(step)) ^ sm64(3 i + stream)) with splitmix64's
 * output function sm64, traj = mulhi64(x0, n_episodes), u = (x >> 11) * 2^-53.  traj_out / u1_out / u2_out (optional)
 * receive the draws used.  A given traj outside the table yields start = goal = -1. */
int porl_hindsight_pairs(const int64_t* starts, const int64_t* lengths, int64_t n_episodes, int32_t batch, uint64_t seed,
                         uint64_t step, const int64_t* traj, const double* u1, const double* u2, int64_t* start, int64_t* goal,
                         int64_t* traj_out, double* u1_out, double* u2_out, void* stream);

/* rvs_sample_batch (util/util.py:129-138) in the packed wire format [s | r | s' | d | a]:
 * out[i] = [ rows[start[i]][:obs_dim] | 0 | rows[goal[i]][:obs_dim] | 0 | rows[start[i]][2*obs_dim + 2 ..] ].
 * One wave per batch row; a start or goal outside [0, n_rows) makes the output row NaN instead of a stray read. */
int porl_gather_pairs(const float* rows, int64_t row_stride, int64_t n_rows, const int64_t* start, const int64_t* goal,
                      int32_t batch, int32_t obs_dim, int32_t act_dim, float* out, int64_t out_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stable two-way partition of the rows of a resident store (generate_test_generlaization_data, util/util.py:219-238;
 * kernels in csrc/partition.hpp).  Rows are read in place through (rows, stride_bytes, n_rows) — a dense store, a
 * row-strided view or a column block of a wider one — and copied as raw 32-bit words (16-byte lanes when both buffers,
 * the stride and row_bytes allow), so NaN payloads and -0.0 survive.  The input is never written.  A row is HELD iff
 * held[i] != 0 (form a) or iff both fp32 words box->cx, box->cy of it lie in the box, bounds inclusive, compared in
 * fp32 (form b; a NaN coordinate is not held — numpy's comparisons in the reference).
 * --------------------------------------------------------------------------------------------- */
typedef struct porl_partition_box {
  int32_t cx, cy;             /* the two fp32 words of a row that are tested */
  float x_lo, x_hi, y_lo, y_hi;
} porl_partition_box;

/* int64 words of workspace porl_partition_rows needs for n_rows rows (-1 when n_rows is outside [1, 2^36]); also
 * reports the tile constants: rows per block and partials per sweep of the one-wave scan (either pointer may be null). */
int64_t porl_partition_workspace(int64_t n_rows, int32_t* rows_per_block, int32_t* partials_per_sweep);

/* mask[i] = 1 if row i is held by `box`, else 0 (uint8, n_rows entries): form (b) made storable, for callers that
 * compact several arrays by one predicate.  One launch. */
int porl_partition_mask(const void* rows, int64_t stride_bytes, int64_t n_rows, int64_t row_bytes,
                        const porl_partition_box* box, uint8_t* mask, void* stream);

/* out (n_rows dense rows of row_bytes) = every row that is not held, in input order, then every held row, in input
 * order: row i goes to rank_kept(i), or to K + (i - rank_kept(i)) when held.  Exactly one of `held` (uint8, n_rows) and
 * `box` is non-null; with `box` both passes recompute the predicate from the rows and no mask is stored.  `index`
 * (optional, int64 n_rows) receives the original row numbers in the same arrangement.  On return (in stream order)
 * workspace[0] = K, the number of kept rows, and workspace[1] = n_rows - K.  Three launches (tile counts, a one-wave scan
 * of them, recompute-and-scatter): no block waits on another; every store is bounded by n_rows.  row_bytes and
 * stride_bytes are multiples of 4, row_bytes <= stride_bytes <= 2^22.  The caller reads K back once, to cut the two
 * views — the only synchronisation. */
int porl_partition_rows(const void* rows, int64_t stride_bytes, int64_t n_rows, int64_t row_bytes, const uint8_t* held,
                        const porl_partition_box* box, void* out, int64_t* index, int64_t* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Column statistics and the affine column pass of a resident store (kernels in csrc/colstats.hpp): what the reference's
 * `--normalize` (por_train.py:141) takes from a dataset — mean / std of the observation columns, obs = (obs - mean) / std
 * (util/util.py:146,160,177) — and the reward rescaling r /= (max_ret - min_ret); r *= max_episode_steps that return_range
 * (util/util.py:67-80) exists for.  Rows are fp32 and read in place through (rows, stride_floats, n_rows): a dense store,
 * a row-strided view or a column block of a wider one.  The statistics never write their input; they accumulate in fp64
 * and combine partial results only by the pairwise update d = mean_b - mean_a, mean = mean_a + d n_b / n,
 * M2 = M2_a + M2_b + d^2 n_a n_b / n (with the rounding residual of every partial mean carried along), in an order that follows from n_rows, n_cols and the two tile constants alone: no
 * floating-point atomics, no block waits on another, two calls on equal values (dense or strided) return equal bits, a
 * constant column has M2 == 0.0 exactly, a column holding a NaN has NaN in all four results.
 * --------------------------------------------------------------------------------------------- */
/* doubles of workspace for n_rows x n_cols; -1 when out of range.  Also reports the tile constants
 * (rows per block, partials per sweep); either pointer may be null. */
int64_t porl_colstats_workspace(int64_t n_rows, int32_t n_cols, int32_t* rows_per_block, int32_t* partials_per_sweep);

/* out = [mean(C) | M2(C) | min(C) | max(C)], fp64, C = n_cols.  Columns [col0, col0 + n_cols) of an fp32 row view are read
 * in place through (rows, stride_floats, n_rows).  M2 = sum (x - mean)^2.  The input is never written.  n_rows in
 * [1, 2^36], n_cols in [1, 4096], col0 + n_cols <= stride_floats <= 2^20.  One launch over the rows (16-byte lanes when
 * rows + col0, stride_floats and n_cols allow, else 4-byte lanes; same result either way), then one launch per merge
 * level.  The caller reads `out` back — the only synchronisation. */
int porl_col_stats(const float* rows, int64_t stride_floats, int64_t n_rows, int32_t col0, int32_t n_cols,
                   double* workspace, double* out, void* stream);

typedef struct porl_col_span { int32_t col0, n_cols, param0, flags; } porl_col_span;   /* flags bit 0: multiply */

/* for every span and j < n_cols:
 *   out[i, col0+j] = fl( fl(rows[i, col0+j] - shift[param0+j]) / div[param0+j] )
 * then, if flags&1, fl( . * mul[param0+j] ): three IEEE round-to-nearest fp32 operations, never fused, the quotient
 * never a multiplication by a reciprocal.  Columns outside the spans are not touched (neither loaded nor stored).
 * `spans` is a HOST array, 1..8 entries, validated before any device call: every span inside `width` and inside
 * n_params, no two overlapping; mul may be null only if no span has bit 0 set.  shift / div / mul are device vectors
 * of n_params floats.  out may be rows itself (in place, then with the same stride: every element is read and written
 * once, by the same lane) or another buffer of at least `width` columns that does not otherwise overlap rows.
 * width <= stride_floats, out_stride_floats <= 2^20.  One launch. */
int porl_affine_cols(const float* rows, int64_t stride_floats, int64_t n_rows, int32_t width,
                     const porl_col_span* spans, int32_t n_spans, const float* shift, const float* div,
                     const float* mul, int32_t n_params, float* out, int64_t out_stride_floats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Costmap encoder engine: FasterNet.forward_cls (agent/fasternet.py:428-438) as built by
 * sorl_train.py:29 `FasterNet(3, args.feature_dim)` — state2costmap, PatchEmbed 4x4s4 + BN (:234-246),
 * depth0 MLPBlocks (:141-194, Partial_conv3 :110-138), PatchMerging 2x2s2 + BN (:249-261), depth1
 * MLPBlocks, AdaptiveAvgPool2d(1) + 1x1 conv + ReLU (:367-371), Linear head (:372).  Forward only: the
 * reference keeps the backbone out of every optimizer (agent/sorl.py:58-64), so its backward never
 * changes a result.  BatchNorm follows nn.BatchNorm2d: batch statistics + running-stat update when
 * `training`, running statistics otherwise.
 * --------------------------------------------------------------------------------------------- */
#define PORL_ENC_MAX_BLOCKS 8
typedef struct porl_enc porl_enc;
typedef struct porl_enc_cfg {
  int32_t n_ang, n_dist;      /* costmap image height x width (reference: 360 x 256) */
  int32_t embed_dim;          /* 96 */
  int32_t depth0, depth1;     /* MLPBlocks per stage (reference depths=(1,2)) */
  int32_t n_div;              /* PConv acts on embed_dim/n_div channels (4) */
  int32_t feature_dim;        /* width of the pre-head 1x1 conv (1280) */
  int32_t num_classes;        /* output features per sample (sorl_train.py:29 -> 256) */
  int32_t max_batch;
  float mlp_ratio;            /* 2.0 */
  float bn_eps, bn_momentum;  /* nn.BatchNorm2d defaults 1e-5, 0.1 */
  /* 0 (default, the parity path): fp32 operands on the fp32-input MFMA.  1: the 1x1 / merge convolutions round their
   * operands to bf16 on the way into LDS and multiply on the bf16 matrix pipe, fp32 accumulate; activations, BatchNorm
   * statistics, the partial 3x3 conv, the patch embedding and the two head products stay fp32.  The reference has no
   * bf16 path (fp32 everywhere): results then differ from it by bf16 rounding (tests state the tolerance).
   * 2: bf16 ACTIVATIONS in HBM behind the patch embedding; partial 3x3 conv, MLP blocks (fused: one kernel per pass over
   * x) and the 2x2s2 merge on the bf16 matrix pipe, fp32 accumulate, fp32 BatchNorm statistics and head
   * (csrc/encoder_bf16.hpp).  Instantiated for the reference architecture (embed 96, mlp_ratio 2, n_div 4); other shapes
   * run mode 1. */
  int32_t bf16_operands;
} porl_enc_cfg;

int porl_enc_create(const porl_enc_cfg* cfg, porl_enc** out);
void porl_enc_destroy(porl_enc* h);
int64_t porl_enc_param_floats(const porl_enc* h);      /* flat parameter buffer, state_dict order + layouts */
int64_t porl_enc_stat_floats(const porl_enc* h);       /* BatchNorm running_mean / running_var buffer */
int64_t porl_enc_workspace_floats(const porl_enc* h);
int32_t porl_enc_tensors(const porl_enc* h);
int32_t porl_enc_norms(const porl_enc* h);
int32_t porl_enc_blocks(const porl_enc* h);            /* MLPBlocks = rows of drop_scale */
/* name = the reference's state_dict key ("stages.0.blocks.0.mlp.0.weight", ...) */
int porl_enc_tensor_info(const porl_enc* h, int32_t index, int64_t* offset, int64_t* numel, char* name,
                         int32_t name_len);
/* name = module prefix ("patch_embed.norm"); offsets into the stat buffer */
int porl_enc_norm_info(const porl_enc* h, int32_t index, int64_t* mean_offset, int64_t* var_offset,
                       int32_t* channels, char* name, int32_t name_len);
int porl_enc_bind(porl_enc* h, float* params, float* bn_stats, float* workspace);
/* Where the last porl_enc_forward left its intermediate results in the workspace (a pure host query; the contents are
 * valid until the next forward).  Tap `which` of a batch of b samples is a dense row-major (b * rows_per_sample, cols)
 * matrix, NHWC position rows, starting offset_floats FLOATS into the workspace whatever its element type.  elem_bytes is
 * 2 (bf16) for the two stage outputs exactly when the forward runs the bf16-activation branch (bf16_operands == 2 on
 * the architecture it is instantiated for), 4 (fp32) otherwise.  All four output pointers are required. */
#define PORL_ENC_TAP_STAGE1 0   /* output of the last stage-1 MLPBlock, rows_per_sample = (n_ang/4) * (n_dist/4), cols = E */
#define PORL_ENC_TAP_STAGE2 1   /* output of the last stage-2 MLPBlock, (n_ang/8) * (n_dist/8) rows of 2E */
#define PORL_ENC_TAP_POOLED 2   /* global average pool, one row of 2E per sample, fp32 */
#define PORL_ENC_TAP_PREHEAD 3  /* relu(1x1 conv) before the Linear head, one row of feature_dim per sample, fp32 */
#define PORL_ENC_TAPS 4
int porl_enc_tap_info(const porl_enc* h, int32_t which, int64_t* offset_floats, int64_t* rows_per_sample,
                      int32_t* cols, int32_t* elem_bytes);
/* The encoder keeps permuted copies of its convolution weights in the workspace and refreshes them on the first
 * forward after porl_enc_bind.  Call this after writing new values into `params` (load_state_dict, an optimizer step on
 * the backbone) so the next forward refreshes them again. */
int porl_enc_weights_changed(porl_enc* h);
/* state (batch, n_ang + 2) row stride state_rs, entries > 8 zeroed in place like the reference
 * (util/costmap.py:17); drop_scale (blocks, batch) = DropPath keep mask / keep_prob per MLPBlock and
 * sample (fasternet.py:76-93) or NULL for none; features (batch, num_classes), row stride feat_rs. */
int porl_enc_forward(porl_enc* h, float* state, int64_t state_rs, int32_t batch, int32_t training,
                     const float* drop_scale, float* features, int64_t feat_rs, void* stream);
/* porl_enc_forward on rows of a resident packed store, read in place: sample b is the n_ang + 2 floats at
 * rows + idx[b] * row_stride + col_offset.  The store is NOT modified: values > 8 are read as 0 (what the
 * reference's in-place clamp, util/costmap.py:17, would leave), nothing is written back.  Everything after the
 * patch embedding is porl_enc_forward's code.  Contract for idx as porl_gather_rows: 0 <= idx[b] < n_rows is the
 * caller's. */
int porl_enc_forward_rows(porl_enc* h, const float* rows, int64_t row_stride, int64_t n_rows, const int64_t* idx,
                          int32_t col_offset, int32_t batch, int32_t training, const float* drop_scale,
                          float* features, int64_t feat_rs, void* stream);

/* Prioritized replay on the device (src/porl/buffer/sum_tree.py:4-77, prioritized_replay_buffer.py:36-108).
 * `tree`: 2*capacity-1 doubles in the reference's heap layout (leaf of data slot d at d + capacity - 1).
 * porl_per_update: SumTree.update for a batch (add() and update_priorities()): leaf <- (|td_error| + eps)^alpha,
 *   a leaf named twice keeps the last value, ancestors are recomputed from their children.  `stamp`: capacity
 *   zero-initialised int32 of scratch that the call leaves zeroed.
 * porl_per_sample: PrioritizedReplayBuffer.sample: segment i of the total priority, s = a + (b-a)*u[i] with the
 *   caller's uniforms u (random.random() of the reference's generator), tree walk -> out_idx (tree indices);
 *   out_prio needs 2*batch doubles (priorities, then scratch); out_w = (n_entries * p/total)^-beta / max. */
int porl_per_update(double* tree, int64_t capacity, const int64_t* tree_idx, const double* td_error, int32_t n,
                    double eps, double alpha, int32_t* stamp, void* stream);
int porl_per_sample(const double* tree, int64_t capacity, const double* u, int32_t batch, int64_t n_entries,
                    double beta, int64_t* out_idx, double* out_prio, float* out_w, void* stream);

/* The same three operations shaped for the online loop (dqn_per_trainer.py:127-175), one launch each; every tree value,
 * tree index and weight is bit-equal to what the two calls above give for the same inputs.
 * porl_per_record: memory.add of one transition into data slot `slot`: the row (host floats, state_dim <=
 *   PORL_RECORD_MAX_STATE each, else PORL_ERR_UNSUPPORTED) is copied into the kernel's arguments at launch and written
 *   to the five arrays of `store` (store->capacity == capacity), the slot's leaf becomes (|td_error| + eps)^alpha and
 *   its ancestors are recomputed, leaf to root.
 * porl_per_sample_slots: porl_per_sample without the priorities; also out_slots = out_idx - (capacity - 1) (the rows
 *   porl_qnet_learn_variant gathers) and out_wmean[0] = fp32 of (fp64 sum of the raw weights, i = 0..batch-1) / max /
 *   batch — the uniform_weight of the reference's (B,1)x(B,) loss.  `scratch`: batch doubles.
 * porl_per_update_f32: porl_per_update in one launch on fp32 |TD errors| (widened to fp64 as they are read), e.g.
 *   the td_abs of porl_qnet_variant; tree indices outside the leaves are ignored; `stamp` as above. */
int porl_per_record(double* tree, int64_t capacity, int64_t slot, double td_error, double eps, double alpha,
                    const float* state, const float* next_state, int32_t state_dim, int64_t action, float reward,
                    float done, const porl_qnet_mirror* store, void* stream);
int porl_per_sample_slots(const double* tree, int64_t capacity, const double* u, int32_t batch, int64_t n_entries,
                          double beta, int64_t* out_idx, int64_t* out_slots, float* out_w, float* out_wmean,
                          double* scratch, void* stream);
int porl_per_update_f32(double* tree, int64_t capacity, const int64_t* tree_idx, const float* td_abs, int32_t n,
                        double eps, double alpha, int32_t* stamp, void* stream);

/* The two operations a loop needs that writes N rows per launch and never returns to the host (csrc/per_vector.hpp), one
 * launch each, one block, no scratch; both bit-equal to the calls above for the same inputs.
 * porl_per_fill_range: memory.add(td_error, ...) for the n data slots (first_slot + i) % capacity, i < n — the tree only,
 *   the rows are the caller's: each leaf becomes (|td_error| + eps)^alpha and every ancestor of one of them is recomputed
 *   as left + right, what porl_per_update leaves for those n tree indices with a constant td_error.  The leaves are one run
 *   of tree indices (two when the ring wraps) and the parents of a run [a, b] are the run [(a-1)/2, (b-1)/2], so the call
 *   writes about 2n + 4*levels nodes, not n*levels; no other node is written.  0 <= n <= capacity <= 2^40 (n == 0: PORL_OK,
 *   no launch), 0 <= first_slot < capacity, td_error / eps / alpha finite; anything else is PORL_ERR_INVALID before a launch.
 * porl_per_sample_keyed: porl_per_sample_slots whose uniforms are drawn in the kernel: sample i of draw `draw` uses
 *   u_i = (double)(sm64(key ^ sm64((draw << 32) | i)) >> 11) * 2^-53,  key = sm64(seed ^ TAG),
 *   TAG = 0xF08CDF1E9B01AC12 = sm64(0x5045524B45594544) ("PERKEYED"), sm64 as for porl_hindsight_pairs.  The tag keeps the
 *   stream apart from what else the same seed keys: porl_qnet_select and the simulator key robot e by sm64(seed ^ sm64(e))
 *   with e <= 2^40 + 2^24, and sm64 is a bijection; porl_sample_indices derives 32-bit Feistel round keys by another mixer.
 *   Everything after u_i is porl_per_sample_slots' arithmetic (one shared device function).  Rejections as
 *   porl_per_sample_slots, and 0 <= draw < 2^32 (batch is an int32 and fits its half of the counter). */
int porl_per_fill_range(double* tree, int64_t capacity, int64_t first_slot, int64_t n, double td_error, double eps,
                        double alpha, void* stream);
int porl_per_sample_keyed(const double* tree, int64_t capacity, uint64_t seed, int64_t draw, int32_t batch,
                          int64_t n_entries, double beta, int64_t* out_idx, int64_t* out_slots, float* out_w,
                          float* out_wmean, double* scratch, void* stream);

/* The lidar navigation task on the device (env/gazebo.py without ROS and Gazebo; csrc/navsim.hpp): a unicycle step and
 * a 2-D ray cast against a world of wall segments and pillars replace the physics and the laser.  One workgroup per
 * robot, one launch per call for any n, no host synchronisation.
 *
 * World: segments (M, 4) fp32 x1 y1 x2 y2 and circles (C, 3) fp32 cx cy r, dense, on the device, shared by all robots;
 * M + C <= PORL_NAV_MAX_PRIMS.  Coordinates are widened to fp64 exactly; all geometry is fp64 and a range is rounded once
 * to fp32.  A circle is solid and seen from outside (near root only).  beam_dirs (n_beams, 2) fp64: cos, sin of beam i's
 * angle in the robot frame, built by the caller (i * pi / 180 for 360 beams) and rotated by sincos(yaw) in the kernel.
 * A beam's range is the smallest t with 0 < t < range_max over segments (den != 0, 0 <= s <= 1) and circles (disc >= 0,
 * t = b - sqrt(disc)), else no_return.
 *
 * Per robot: state (n, 8) fp64 x y yaw goal_x goal_y prev_goal_distance prev_goal_angle 0; counters (n, 4) int64 n_step
 * episode status draws_used.  Status: PORL_NAV_RUNNING / HIT / GOAL / TIMELIMITED, and bit PORL_NAV_DRAW_CAP when a reset
 * stopped at PORL_NAV_MAX_DRAWS draws.  Observation rows (S wide): layout PORL_NAV_LAYOUT_GOAL [scan | goal in the robot
 * frame], S = n_beams + 2 (getState, env/gazebo.py:135-147); PORL_NAV_LAYOUT_POSE [scan | x y | yaw | goal_x goal_y],
 * S = n_beams + 5 (the rows preprocess.py:23-36 reads). */
#define PORL_NAV_MAX_PRIMS 2048
#define PORL_NAV_MAX_BEAMS 1024
#define PORL_NAV_MAX_DRAWS 256
#define PORL_NAV_RUNNING 0
#define PORL_NAV_HIT 1
#define PORL_NAV_GOAL 2
#define PORL_NAV_TIMELIMITED 3   /* truncated without termination */
#define PORL_NAV_DRAW_CAP 256    /* status bit 8 */
#define PORL_NAV_LAYOUT_GOAL 0
#define PORL_NAV_LAYOUT_POSE 1
#define PORL_NAV_TERMINATED 1    /* flags bit 0 */
#define PORL_NAV_TRUNCATED 2     /* flags bit 1 */
typedef struct porl_nav_params {
  double dt;            /* 0.2   seconds per step (the scan period env.step waits for) */
  double max_lin_vel;   /* 0.15  v = clamp(a0, 0, max_lin_vel) */
  double max_ang_vel;   /* 1.5   w = clamp(a1, -max_ang_vel, max_ang_vel) */
  double min_range;     /* 0.13  0 < min(scan) < min_range: hit; max_lin_vel * dt < min_range is required */
  double range_max;     /* 3.5 */
  double no_return;     /* 10.0  what lidarPreprocess makes of inf */
  double goal_radius;   /* 0.2 */
  double hit_reward;    /* -500 */
  double goal_reward;   /* +500 */
  double origin_x;      /* random_pts_map: map_x + (rank % 4) * 5 */
  double origin_y;      /*                 map_y + (3 - rank / 4) * 5 */
  double spawn_lo;      /* 0.16  a coordinate is floor(cells * u) + spawn_lo + spawn_span * u' */
  double spawn_span;    /* 0.68 */
  double min_gap_sq;    /* 0.01  redraw while (x1 - x2)^2 < min_gap_sq, the same on y */
  double goal_dist_lo;  /* 0.3   redraw the goal while dist < goal_dist_lo or dist > goal_dist_hi */
  double goal_dist_hi;  /* 3.5 */
  int32_t n_beams;      /* 360   1 .. PORL_NAV_MAX_BEAMS */
  int32_t episode_step; /* 500   truncated = n_step >= episode_step */
  int32_t cells;        /* 5     randint(cells) */
  int32_t layout;       /* PORL_NAV_LAYOUT_* */
  int32_t auto_reset;   /* != 0: a robot that finishes in porl_nav_step is reset in the same launch */
  int32_t reserved;     /* 0 */
} porl_nav_params;
/* The ray cast alone: out[i * out_stride + b] = range of beam b from poses[i] = (x, y, yaw), fp64 (n, 3). */
int porl_nav_scan(const float* segments, int32_t M, const float* circles, int32_t C, const double* poses,
                  const double* beam_dirs, const porl_nav_params* params, float* out, int64_t out_stride, int64_t n,
                  void* stream);
/* random_pts_map (env/gazebo.py:280-318) statement for statement on a counter stream: key = sm64(seed ^ sm64(env_offset +
 * i)), draw j of episode e is u = (sm64(key ^ sm64(256 e + j)) >> 11) * 2^-53 (sm64 = the splitmix64 finaliser of
 * porl_hindsight_pairs); each coordinate takes an integer draw, then a uniform draw.  Robot i with mask == NULL or
 * mask[i] != 0: episode += 1, new start and goal, yaw = 0, n_step = 0, prev_* from the new pose, status running,
 * obs[i] = the observation from there.  Other robots are not touched.  A spawn is NOT tested against the world. */
int porl_nav_reset(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                   const porl_nav_params* params, uint64_t seed, int64_t env_offset, const uint8_t* mask, double* state,
                   int64_t* counters, float* obs, int64_t obs_stride, int64_t n, void* stream);
/* One step of every running robot (env.step, env/gazebo.py:149-181, getSarsa :91-133): clip the command actions[i] =
 * (v, w) (a non-finite component counts as 0), exact arc over dt, scan at the new pose, relative goal, shaped reward,
 * hit (reward hit_reward) then goal (goal_reward, wins), n_step += 1, truncated = n_step >= episode_step.
 * obs (n, S) in/out: the observation each robot acted on; on return the one to act on next (next_obs, or with auto_reset
 * the observation after the reset).  next_obs, reward (n), flags (n) int32, status (n) int32 are required.  rows is
 * optional: robot i's transition [s | r | s' | terminated | v w] (2S + 4 floats, the clipped command) at rows + i *
 * row_stride.  A robot whose status is not running is left as it is: reward 0, flags 0, its row all NaN. */
int porl_nav_step(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                  const porl_nav_params* params, uint64_t seed, int64_t env_offset, const float* actions,
                  int64_t act_stride, double* state, int64_t* counters, float* obs, int64_t obs_stride, float* next_obs,
                  int64_t next_stride, float* reward, int32_t* flags, int32_t* status, float* rows, int64_t row_stride,
                  int64_t n, void* stream);

/* The discrete lidar navigation task (env/env.py, the 5-action task runner.py hands to DQN_CQL; csrc/navsim_discrete.hpp)
 * on the same world, ray cast, reset draw and counter stream as above.  The robot drives at lin_vel; action a of
 * n_actions picks w = ((n_actions - 1) / 2 - a) * ang_step (an index outside [0, n_actions) is clamped into range).
 * Observation rows [scan | heading | distance], S = n_beams + 2 (params->layout must be PORL_NAV_LAYOUT_GOAL), heading =
 * round2(wrap(atan2(gy - y, gx - x) - yaw)), distance = round2(|goal - position|), round2(x) = rint(100 x) / 100 in fp64.
 * Hit: 0 < min(scan) < min_range; goal: distance < goal_radius, and the goal wins.  Reward: round2(5 tr) * 2^(distance /
 * goal_distance), tr = 1 - 4 |0.5 - frac(0.25 + ((0.5 angle) mod 2 pi) / pi)|, angle = -pi/4 + heading + pi/8 a + pi/2
 * (mod non-negative), or goal_reward / hit_reward of this struct (params' two are not read).  truncated = n_step >=
 * episode_step; the status is PORL_NAV_TIMELIMITED then, also on a step that terminated (flags keep both bits), and the
 * reward is not altered.  state (n, 8) fp64: x y yaw goal_x goal_y 0 0 goal_distance (the rounded distance at reset);
 * counters as above.  Geometry, limits and reset constants travel in porl_nav_params (the reference's reset uses
 * goal_dist_lo = 0.25 and maps a beam without return to no_return = 3.5). */
typedef struct porl_nav_discrete {
  int32_t n_actions;    /* 5     1 .. 5: the reference's yaw table has five entries */
  double lin_vel;       /* 0.15  lin_vel * dt < min_range is required */
  double ang_step;      /* 0.75  max_ang_vel * 0.5 */
  double goal_reward;   /* +200 */
  double hit_reward;    /* -200 */
} porl_nav_discrete;
/* porl_nav_reset for the discrete task; returns (n) fp64, optional: the running episode return, zeroed for a robot that
 * is reset. */
int porl_nav_dreset(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                    const porl_nav_params* params, const porl_nav_discrete* task, uint64_t seed, int64_t env_offset,
                    const uint8_t* mask, double* state, int64_t* counters, float* obs, int64_t obs_stride, double* returns,
                    int64_t n, void* stream);
/* One step of every running robot with actions (n) int64.  obs, next_obs, reward, flags, status as porl_nav_step; a robot
 * whose status is not running is left as it is (reward 0, flags 0) and writes to neither optional output:
 *   replay (NULL: none): robot i's transition goes into slot (replay_base + i) % capacity of the five arrays — states the
 *     observation acted on, next_states the one reached, actions the clamped index, rewards, dones = terminated |
 *     truncated as 1.0 / 0.0 (what dqn_trainer.py:119-180 pushes).  Rows are S floats, dense.  n <= capacity and
 *     0 <= replay_base < capacity are required: no two robots share a slot.
 *   tallies (n, 4) fp64 with returns (n) fp64 (both or neither): returns[i] += reward; at an episode's end tallies[i] +=
 *     (1, returns[i], goal, hit) and returns[i] = 0.
 * No atomics, no communication between blocks.  Every argument is checked before the launch (PORL_ERR_INVALID). */
int porl_nav_dstep(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                   const porl_nav_params* params, const porl_nav_discrete* task, uint64_t seed, int64_t env_offset,
                   const int64_t* actions, double* state, int64_t* counters, float* obs, int64_t obs_stride, float* next_obs,
                   int64_t next_stride, float* reward, int32_t* flags, int32_t* status, const porl_qnet_mirror* replay,
                   int64_t replay_base, double* tallies, double* returns, int64_t n, void* stream);
/* Epsilon-greedy over a table q (n, n_actions) fp32 with row stride q_rs, n_actions <= 64, into out (n) int64 on the
 * device; nothing is read back.  Robot i at act-step t draws u1, u2 = draws 0, 1 of "episode" t of the stream keyed
 * sm64(seed ^ sm64(env_offset + i)) (porl_nav_reset's construction); u1 < epsilon: floor(n_actions * u2); otherwise the
 * arg-max, ties to the lowest index, a NaN counting as the maximum (torch.argmax). */
int porl_qnet_select(const float* q, int64_t q_rs, int32_t n_actions, int64_t n, double epsilon, uint64_t seed,
                     int64_t env_offset, uint64_t t, int64_t* out, void* stream);
/* porl_qnet_forward on n rows of states, walked in chunks of the engine's max_batch, into the caller's scratch q (n,
 * n_actions), then porl_qnet_select on it: acting for n robots from one call.  Plain-Q networks only (DQN, Double DQN,
 * Dueling through the composed output layer, CQL); C51 and QR-DQN have porl_qnet_act_rows_dist, IQN porl_iqn_act_rows. */
int porl_qnet_act_rows(porl_qnet* h, int which, const float* states, int64_t s_rs, int64_t n, float* q, int64_t q_rs,
                       double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, int64_t* out, void* stream);
/* Epsilon-greedy over the outputs of a distributional network: z (n, n_actions * n_sub) fp32 with row stride z_rs, action
 * a in columns [a * n_sub, (a + 1) * n_sub).  One value per action — PORL_DIST_QR: the mean of the n_sub quantiles;
 * PORL_DIST_C51: sum_n softmax(z[a, :])_n support[n] — summed in the order the loss heads rank the next state's actions
 * by (lane-strided partials of a 64-lane wave, then the xor butterfly), so acting and bootstrapping agree.  The n_actions
 * values go to q (n, n_actions) with row stride q_rs and the action to out (n) int64, both always, also when the robot
 * explores; the action is porl_qnet_select's rule on those values, with the same key and draws.  Of head only kind,
 * n_actions (<= 64), n_sub (<= 256; C51: >= 2) and support (C51: n_sub device floats) are read.  Stateless; one launch;
 * every argument is checked before it. */
int porl_dist_select(const float* z, int64_t z_rs, const porl_dist_head* head, int64_t n, float* q, int64_t q_rs,
                     double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, int64_t* out, void* stream);
/* porl_qnet_act_rows for a C51 / QR-DQN network: n rows of states in chunks of the engine's max_batch, each chunk staged,
 * forwarded, and handed to porl_dist_select's kernel where the forward left its output rows in the workspace — the
 * n x n_actions * n_sub outputs are never copied out.  head->n_actions * head->n_sub must equal the engine's outputs. */
int porl_qnet_act_rows_dist(porl_qnet* h, int which, const float* states, int64_t s_rs, int64_t n, const porl_dist_head* head,
                            float* q, int64_t q_rs, double epsilon, uint64_t seed, int64_t env_offset, uint64_t t,
                            int64_t* out, void* stream);
/* Epsilon-greedy under discrete BCQ's constraint (bcq.py:59-72), for n robots in one launch: q (n, n_actions) fp32 action
 * values with row stride q_rs, logits (n, n_actions) fp32 outputs of the behaviour network with row stride z_rs,
 * n_actions <= 64.  Per robot: p = softmax(logits) in porl_softmax_mask's order and expressions (the same bits);
 * allowed_j = p_j > threshold (absolute, finite and in [0, 1]); mask (NULL: none), dense (n, n_actions) fp32, receives the
 * 0 / 1 row, also when the robot explores.  Exploration is porl_qnet_select's — the same key and draws, u1 < epsilon:
 * floor(n_actions * u2) over ALL actions, as the reference explores.  Otherwise the arg-max of v_j = q_j + (mask_j - 1) *
 * 1e10f in fp32 — the expression porl_qnet_bcq_learn's step kernel ranks the next state's actions by — first maximum, a
 * NaN in v counting as the maximum.  A row with every action masked is ranked by the same v_j (action 0 when every
 * |q_j| < 512).  With threshold 0 and finite logits in [-20, 20] every action is allowed and the result is
 * porl_qnet_select's.  Stateless; nothing is read back; every argument is checked before the launch. */
int porl_bcq_select(const float* q, int64_t q_rs, const float* logits, int64_t z_rs, int32_t n_actions, int64_t n,
                    float threshold, double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, float* mask, int64_t* out,
                    void* stream);
/* porl_qnet_act_rows under the constraint: n rows of states walked in chunks of the smaller max_batch of the two engines,
 * porl_qnet_forward of h (parameters `which`) into the caller's q (n, n_actions) and of beh (its online parameters) into
 * the caller's logits (n, n_actions), then ONE launch of porl_bcq_select's kernel for all n.  As porl_qnet_forward
 * writes them, a row of q and of logits is written over its whole stride (zeros behind the n_actions values): n * q_rs
 * and n * z_rs floats must be writable.  The two engines must be bound, distinct, on one device and agree in state_dim
 * and n_actions. */
int porl_qnet_act_rows_bcq(porl_qnet* h, porl_qnet* beh, int which, const float* states, int64_t s_rs, int64_t n, float* q,
                           int64_t q_rs, float* logits, int64_t z_rs, float threshold, double epsilon, uint64_t seed,
                           int64_t env_offset, uint64_t t, float* mask, int64_t* out, void* stream);

/* ---- An A* expert for the navigation task, planned on the device (csrc/expert.hpp) ------------------------------------
 * The device form of the reference's dataloader/a_star.py AStarPlanner.planning for n robots per call, with no read-back.
 * Grid: w x h cells, the centre of cell (ix, iy) at ix * resolution + min_x, iy * resolution + min_y (a product, then a
 * sum); the cell of a position is rint((x - min_x) / resolution), half to even.  A cell is blocked iff its centre lies
 * within `inflate` of a primitive of the world (segments (M, 4), circles (C, 3) fp32 as porl_nav_scan reads them, widened
 * to fp64; a segment of length 0 is a point).  Limits: (w + 2)(h + 2) <= 65536 padded cells, the padded field and the
 * bitmap within one workgroup's LDS (porl_astar_label's limit), w + h <= 65534. */
typedef struct porl_nav_grid {
  double resolution;    /* > 0 */
  double inflate;       /* >= 0: the clearance kept from every primitive */
  double min_x, min_y;  /* centre of cell (0, 0) */
  int32_t w, h;
} porl_nav_grid;
#define PORL_EXPERT_OK 0             /* a waypoint was found */
#define PORL_EXPERT_NO_FIELD 1       /* the robot's cell is off the grid, or it and its eight neighbours are unreached */
#define PORL_EXPERT_GOAL_OFF_GRID 2
#define PORL_EXPERT_GOAL_BLOCKED 3
#define PORL_EXPERT_NON_FINITE 4     /* pose or goal */
#define PORL_EXPERT_NOT_CONVERGED 5  /* the field kernel reached its sweep bound of w * h */
typedef struct porl_nav_expert_params {
  double dt;            /* porl_nav_params.dt */
  double max_lin_vel;   /* porl_nav_params.max_lin_vel: v = max_lin_vel * max(0, cos e) */
  double max_ang_vel;   /* porl_nav_params.max_ang_vel: w = clip(e / dt, +-max_ang_vel) */
  double ang_step;      /* porl_nav_discrete.ang_step (scores only) */
  int32_t n_actions;    /* porl_nav_discrete.n_actions, 1 .. 64 (scores only) */
  int32_t lookahead;    /* >= 1: the waypoint is the centre of the cell this many steps down the path */
  int32_t max_path;     /* >= 0: cells written per robot when path is given */
  int32_t reserved;     /* 0 */
} porl_nav_expert_params;
/* The occupancy bitmap of a world: bit (iy + 1) * (w + 2) + ix + 1 of n_words >= ceil((w + 2)(h + 2) / 32) uint32 words on
 * the device (porl_astar_label's padded layout; halo bits read 0).  One launch. */
int porl_nav_rasterize(const float* segments, int32_t M, const float* circles, int32_t C, const porl_nav_grid* grid,
                       uint32_t* bitmap, int64_t n_words, void* stream);
/* Plan and steer n robots from state (n, 8) fp64 `x y yaw goal_x goal_y ...` (porl_nav_step's), two launches on `stream`.
 * (1) Robot i whose goal cell is on the grid and free and differs from the one tag[i] names gets its exact 8-connected
 * distance field from the goal cell — pairs a << 16 | b, 0xFFFFFFFF unreached, (w + 2)(h + 2) uint32 in row i of `field` —
 * and tag[i] = iy * w + ix + 1 of the goal cell (tag (n) int64, 0 = no field; start from zeros); every other robot's row
 * and tag stay as they are.  (2) Every robot: status (above); for PORL_EXPERT_OK the path is the descent of the field
 * from the robot's cell in the reference's motion order — the first neighbour n with field[n] + move == field[c] as
 * integers; from an unreached cell the first step goes to its reached neighbour of least cost — path_len the node count
 * from the robot's cell to the goal's, both included, and the waypoint the centre of the cell `lookahead` steps down, or
 * the goal position itself once the descent reaches the goal cell.  For every other status the waypoint is the goal
 * position and path_len 0.  With e the heading error to the waypoint wrapped into [-pi, pi]: commands (n, 2) fp32 with row
 * stride cmd_stride `v = max_lin_vel * max(0, cos e), w = clip(e / dt, +-max_ang_vel)`; scores (n, n_actions) fp32 with row
 * stride score_stride `-|e - w_a dt|`, w_a = ((n_actions - 1) / 2 - a) * ang_step, porl_nav_dstep's command table, so
 * porl_qnet_select on them picks the nearest turn.  PORL_EXPERT_NON_FINITE: zero command, zero scores.  path (n, max_path,
 * 2) int32 receives the cells (ix, iy) from the robot's to the goal's, truncated at max_path, the rest -1.  commands,
 * scores, waypoint (n, 2) fp64, path_len (n), status (n) and path are each optional (NULL).  Robots that are not running
 * are planned from the state they hold.  Nothing is read back; every argument is checked before the first launch. */
int porl_nav_expert(const porl_nav_grid* grid, const uint32_t* bitmap, const porl_nav_expert_params* params,
                    const double* state, uint32_t* field, int64_t* tag, float* commands, int64_t cmd_stride, float* scores,
                    int64_t score_stride, double* waypoint, int32_t* path_len, int32_t* status, int32_t* path, int64_t n,
                    void* stream);

/* Experiment knobs (scheduling only, never the mathematics).  "gemm_lds_pad": extra dynamic LDS bytes per GEMM block,
 * limiting how many blocks share a CU.  "qnet_fused": 0 forces the multi-launch CQL path.  porl_tune_set sets the process
 * defaults, copied by porl_iql / qnet / enc handles when created; porl_iql_tune_set sets one live IQL engine's copy. */
int porl_tune_set(const char* key, int value);
int porl_iql_tune_set(porl_iql* h, const char* key, int value);
/* Diagnostics taking a device pointer.  "qnet_stamps": >= 32 uint64 receiving block 0's shader-clock stamps at
 * the phase boundaries of the one-launch CQL kernel (NULL switches it off). */
int porl_tune_set_ptr(const char* key, void* ptr);

/* Stream signals (no reference counterpart; used by the pipelined update of porl_amd/agent/_iql.py): a 64-bit counter
 * in device signal memory.  porl_signal_write enqueues "counter = value" on `stream` (after everything enqueued before
 * it), porl_signal_wait_ge holds `stream` until counter >= value.  Values must only grow. */
int porl_signal_create(void** out);
int porl_signal_destroy(void* sig);
int porl_signal_write(void* sig, uint64_t value, void* stream);
int porl_signal_wait_ge(void* sig, uint64_t value, void* stream);
/* One pipelined update (sampled minibatch) from one call: value phase on main_stream, policy phase on side_stream,
 * ordered by the three counters (value Adam done / policy forward half done / policy phase done) exactly as
 * porl_amd/agent/_iql.py issues the phase calls — reference agent/por.py:73-112 (one update), por_train.py:71-82 (the
 * loop that calls it).  seq = update number (>= 1, growing); wait_policy_seq / wait_fwd_seq = counter values the main
 * stream waits for before loading the batch / before the value Adam (0 = no wait); write_policy != 0 publishes seq on
 * sig_policy at the end.  The engine must be in PORL_IQL_MODE_TWO_SLOTS | PORL_IQL_MODE_FOLD_COMBINE mode. */
int porl_iql_update_pipelined(porl_iql* h, const porl_iql_hyper* hp, int32_t batch, const float* rows, int64_t row_stride,
                              int64_t n_rows, int32_t act_dim, int32_t target_is_action, uint64_t seed, uint64_t step,
                              void* sig_value, void* sig_fwd, void* sig_policy, uint64_t seq, uint64_t wait_policy_seq,
                              uint64_t wait_fwd_seq, int32_t write_policy, void* main_stream, void* side_stream);

/* Per-launch timing with HIP events on the launch stream (off by default; adds two event records per
 * kernel).  porl_prof_read synchronises the device and returns the number of entries filled. */
typedef struct porl_prof_entry {
  char name[96];
  int64_t launches;
  double total_ms;
  double flops;   /* algorithmic, summed over launches (GEMMs: 2*M*N*K per problem) */
  double bytes;   /* algorithmic operand + result bytes, summed over launches */
} porl_prof_entry;
int porl_prof_enable(int on);
int porl_prof_read(porl_prof_entry* out, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* PORL_HIP_H */
