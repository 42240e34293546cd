// The discrete lidar navigation task and acting for N robots without a read-back (porl_nav_dreset, porl_nav_dstep,
// porl_qnet_select, porl_qnet_act_rows, porl_dist_select, porl_qnet_act_rows_dist): the host side of
// csrc/navsim_discrete.hpp and csrc/dist_act.hpp.  Included by porl_api.hip behind navsim_api.inc and qnet_api.inc, whose
// checks it shares.  Every argument is judged before the first device call; no allocation and no synchronisation.
//
// porl_qnet_act_rows covers the plain-Q epilogue — DQN, Double DQN, Dueling (through the composed output layer) and CQL;
// porl_qnet_act_rows_dist the distributional heads on the same engine (C51, QR-DQN), whose n x A*NS outputs stay in the
// workspace.  IQN has its own engine: porl_iqn_act_rows (csrc/iqn_api.inc).  porl_bcq_select and porl_qnet_act_rows_bcq are
// discrete BCQ's constrained rule on two engines (csrc/bcq_act.hpp).

namespace {

int navd_check_task(const porl_nav_params* p, const porl_nav_discrete* d) {
  if (!d) PORL_FAIL(PORL_ERR_INVALID, "null task");
  if (d->n_actions < 1 || d->n_actions > NAVD_MAX_ACTIONS)
    PORL_FAIL(PORL_ERR_INVALID, "n_actions %d outside [1, %d]", d->n_actions, NAVD_MAX_ACTIONS);
  if (p->layout != PORL_NAV_LAYOUT_GOAL) PORL_FAIL(PORL_ERR_INVALID, "layout must be PORL_NAV_LAYOUT_GOAL: the observation is [scan | heading | distance]");
  if (!(d->lin_vel >= 0.0) || !std::isfinite(d->lin_vel)) PORL_FAIL(PORL_ERR_INVALID, "lin_vel must be finite and not negative");
  if (!(d->ang_step >= 0.0) || !std::isfinite(d->ang_step)) PORL_FAIL(PORL_ERR_INVALID, "ang_step must be finite and not negative");
  if (!(d->lin_vel * p->dt < p->min_range))
    PORL_FAIL(PORL_ERR_INVALID, "lin_vel * dt must stay below min_range: a robot could pass a wall between two scans");
  if (!((double)(d->n_actions - 1) / 2.0 * d->ang_step * p->dt < 3.141592653589793))
    PORL_FAIL(PORL_ERR_INVALID, "(n_actions - 1) / 2 * ang_step * dt must stay below pi");
  if (!std::isfinite(d->goal_reward)) PORL_FAIL(PORL_ERR_INVALID, "task goal_reward must be finite");
  if (!std::isfinite(d->hit_reward)) PORL_FAIL(PORL_ERR_INVALID, "task hit_reward must be finite");
  return PORL_OK;
}

int navd_check_offset(int64_t env_offset) {
  if (env_offset < 0 || env_offset > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "env_offset %lld outside [0, 2^40]", (long long)env_offset);
  return PORL_OK;
}

size_t navd_lds_bytes(int32_t M, int32_t C, const porl_nav_params* p) {
  return (size_t)(M + C) * 16 + sizeof(NavdShared) + (size_t)p->n_beams * 4;
}

int select_check(const float* q, int64_t q_rs, int32_t n_actions, int64_t n, double epsilon, int64_t env_offset, uint64_t t,
                 const int64_t* out) {
  if (!q) PORL_FAIL(PORL_ERR_INVALID, "null action values");
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (n < 1 || n > NAV_MAX_ROBOTS) PORL_FAIL(PORL_ERR_INVALID, "n %lld outside [1, 2^24]", (long long)n);
  if (n_actions < 1 || n_actions > SELECT_MAX_ACTIONS)
    PORL_FAIL(PORL_ERR_INVALID, "n_actions %d outside [1, %d]", n_actions, SELECT_MAX_ACTIONS);
  if (q_rs < n_actions || q_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "q_rs %lld: a row of action values is %d floats", (long long)q_rs, n_actions);
  if (!std::isfinite(epsilon) || epsilon < 0.0 || epsilon > 1.0) PORL_FAIL(PORL_ERR_INVALID, "epsilon must lie in [0, 1]");
  PORL_TRY(navd_check_offset(env_offset));
  if (t > (uint64_t(1) << 54)) PORL_FAIL(PORL_ERR_INVALID, "act-step t outside [0, 2^54]");
  return PORL_OK;
}

int select_launch(const float* q, int64_t q_rs, int32_t n_actions, int64_t n, double epsilon, uint64_t seed, int64_t env_offset,
                  uint64_t t, int64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(qnet_select_kernel, dim3((unsigned)((n + SELECT_THREADS - 1) / SELECT_THREADS)), dim3(SELECT_THREADS), 0, s, q,
                     (long long)q_rs, (int)n_actions, (long long)n, epsilon, seed, (long long)env_offset, (long long)t,
                     reinterpret_cast<long long*>(out));
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// the head rules of porl_qnet_dist_learn (n_out: the network's outputs, < 0: no network), then select_check's
int dist_select_check(const porl_dist_head* head, int64_t n_out, int64_t n, const float* q, int64_t q_rs, double epsilon,
                      int64_t env_offset, uint64_t t, const int64_t* out) {
  if (!head) PORL_FAIL(PORL_ERR_INVALID, "null head");
  PORL_TRY(dist_head_ok(head, n_out));
  return select_check(q, q_rs, head->n_actions, n, epsilon, env_offset, t, out);
}

int dist_select_launch(const float* z, int64_t z_rs, const porl_dist_head* head, int64_t n, float* q, int64_t q_rs,
                       double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, int64_t* out, hipStream_t s) {
  DistSelectArgs a{};
  a.z = z; a.z_rs = (long long)z_rs; a.support = head->support;
  a.q = q; a.q_rs = (long long)q_rs; a.out = reinterpret_cast<long long*>(out);
  a.n = (long long)n; a.env_offset = (long long)env_offset; a.t = (long long)t;
  a.epsilon = epsilon; a.seed = seed;
  a.kind = head->kind == PORL_DIST_QR ? 0 : 1; a.A = head->n_actions; a.NS = head->n_sub;
  hipLaunchKernelGGL(dist_select_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// select_check's rules, then the behaviour logits, the threshold and the optional mask of the BCQ-constrained rule
int bcq_select_check(const float* q, int64_t q_rs, const float* logits, int64_t z_rs, int32_t n_actions, int64_t n,
                     float threshold, double epsilon, int64_t env_offset, uint64_t t, const float* mask, const int64_t* out) {
  PORL_TRY(select_check(q, q_rs, n_actions, n, epsilon, env_offset, t, out));
  if (!logits) PORL_FAIL(PORL_ERR_INVALID, "null behaviour logits");
  if (z_rs < n_actions || z_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "z_rs %lld: a row of behaviour logits is %d floats", (long long)z_rs, n_actions);
  if (!std::isfinite(threshold) || threshold < 0.f || threshold > 1.f) PORL_FAIL(PORL_ERR_INVALID, "threshold must lie in [0, 1]");
  if (mask && (mask == q || mask == logits)) PORL_FAIL(PORL_ERR_INVALID, "mask must not be q or logits");
  return PORL_OK;
}

int bcq_select_launch(const float* q, int64_t q_rs, const float* logits, int64_t z_rs, int32_t n_actions, int64_t n,
                      float threshold, double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, float* mask, int64_t* out,
                      hipStream_t s) {
  hipLaunchKernelGGL(bcq_select_kernel, dim3((unsigned)((n + SELECT_THREADS - 1) / SELECT_THREADS)), dim3(SELECT_THREADS), 0, s, q,
                     (long long)q_rs, logits, (long long)z_rs, (int)n_actions, (long long)n, threshold, epsilon, seed,
                     (long long)env_offset, (long long)t, mask, reinterpret_cast<long long*>(out));
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // namespace

extern "C" {

int porl_nav_dreset(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                    const porl_nav_params* params, const porl_nav_discrete* task, uint64_t seed, int64_t env_offset,
                    const uint8_t* mask, double* state, int64_t* counters, float* obs, int64_t obs_stride, double* returns,
                    int64_t n, void* stream) {
  PORL_TRY(nav_check_world(segments, M, circles, C, beam_dirs, params, n));
  PORL_TRY(nav_check_task(params, state, counters, obs, obs_stride));
  PORL_TRY(navd_check_task(params, task));
  PORL_TRY(navd_check_offset(env_offset));
  DevGuard _dg(device_of(state));
  const NavWorldArgs w{segments, M, circles, C, beam_dirs};
  hipLaunchKernelGGL(navd_reset_kernel, dim3((unsigned)n), dim3(NAV_THREADS), navd_lds_bytes(M, C, params), (hipStream_t)stream,
                     w, *params, seed, (long long)env_offset, mask, state, reinterpret_cast<long long*>(counters), obs,
                     (long long)obs_stride, returns);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_nav_dstep(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                   const porl_nav_params* params, const porl_nav_discrete* task, uint64_t seed, int64_t env_offset,
                   const int64_t* actions, double* state, int64_t* counters, float* obs, int64_t obs_stride, float* next_obs,
                   int64_t next_stride, float* reward, int32_t* flags, int32_t* status, const porl_qnet_mirror* replay,
                   int64_t replay_base, double* tallies, double* returns, int64_t n, void* stream) {
  PORL_TRY(nav_check_world(segments, M, circles, C, beam_dirs, params, n));
  PORL_TRY(nav_check_task(params, state, counters, obs, obs_stride));
  PORL_TRY(navd_check_task(params, task));
  PORL_TRY(navd_check_offset(env_offset));
  const int S = params->n_beams + 2;
  if (!actions) PORL_FAIL(PORL_ERR_INVALID, "null actions");
  if (!next_obs) PORL_FAIL(PORL_ERR_INVALID, "null next_obs");
  if (next_obs == obs) PORL_FAIL(PORL_ERR_INVALID, "next_obs must not be obs (obs is read as s and rewritten)");
  if (next_stride < S || next_stride > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "next_stride %lld: an observation is %d floats", (long long)next_stride, S);
  if (!reward) PORL_FAIL(PORL_ERR_INVALID, "null reward");
  if (!flags) PORL_FAIL(PORL_ERR_INVALID, "null flags");
  if (!status) PORL_FAIL(PORL_ERR_INVALID, "null status");
  if (replay) {
    if (!replay->states || !replay->next_states || !replay->actions || !replay->rewards || !replay->dones)
      PORL_FAIL(PORL_ERR_INVALID, "null replay array");
    if (replay->capacity < 1 || replay->capacity > (int64_t(1) << 40))
      PORL_FAIL(PORL_ERR_INVALID, "replay capacity %lld outside [1, 2^40]", (long long)replay->capacity);
    if (n > replay->capacity)
      PORL_FAIL(PORL_ERR_INVALID, "n %lld robots > replay capacity %lld: two robots would share a slot", (long long)n,
                (long long)replay->capacity);
    if (replay_base < 0 || replay_base >= replay->capacity)
      PORL_FAIL(PORL_ERR_INVALID, "replay_base %lld outside [0, %lld)", (long long)replay_base, (long long)replay->capacity);
    if (replay->states == obs || replay->next_states == obs || replay->states == next_obs || replay->next_states == next_obs)
      PORL_FAIL(PORL_ERR_INVALID, "the replay arrays must not be obs or next_obs");
  } else if (replay_base != 0) {
    PORL_FAIL(PORL_ERR_INVALID, "replay_base %lld without a replay target (pass 0)", (long long)replay_base);
  }
  if ((tallies == nullptr) != (returns == nullptr)) PORL_FAIL(PORL_ERR_INVALID, "tallies and returns go together: both or neither");
  DevGuard _dg(device_of(state));
  const NavWorldArgs w{segments, M, circles, C, beam_dirs};
  NavdStepArgs a{};
  a.seed = seed; a.env_offset = (long long)env_offset;
  a.actions = reinterpret_cast<const long long*>(actions);
  a.state = state; a.counters = reinterpret_cast<long long*>(counters);
  a.obs = obs; a.obs_stride = (long long)obs_stride; a.next_obs = next_obs; a.next_stride = (long long)next_stride;
  a.reward = reward; a.flags = flags; a.status = status;
  if (replay) {
    a.r_states = replay->states; a.r_next = replay->next_states; a.r_actions = reinterpret_cast<long long*>(replay->actions);
    a.r_rewards = replay->rewards; a.r_dones = replay->dones;
    a.r_capacity = (long long)replay->capacity; a.r_base = (long long)replay_base;
  }
  a.tallies = tallies; a.returns = returns;
  hipLaunchKernelGGL(navd_step_kernel, dim3((unsigned)n), dim3(NAV_THREADS), navd_lds_bytes(M, C, params), (hipStream_t)stream,
                     w, *params, *task, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_qnet_select(const float* q, int64_t q_rs, int32_t n_actions, int64_t n, double epsilon, uint64_t seed,
                     int64_t env_offset, uint64_t t, int64_t* out, void* stream) {
  PORL_TRY(select_check(q, q_rs, n_actions, n, epsilon, env_offset, t, out));
  DevGuard _dg(device_of(out));
  return select_launch(q, q_rs, n_actions, n, epsilon, seed, env_offset, t, out, (hipStream_t)stream);
}

int porl_qnet_act_rows(porl_qnet* h, int which, const float* states, int64_t s_rs, int64_t n, float* q, int64_t q_rs,
                       double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, int64_t* out, void* stream) {
  PORL_TRY(qnet_ready(h, false));
  if (which != 0 && which != 1) PORL_FAIL(PORL_ERR_INVALID, "which %d: 0 online, 1 target", which);
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  if (s_rs < h->cfg.state_dim || s_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "s_rs %lld: a state is %d floats", (long long)s_rs, h->cfg.state_dim);
  PORL_TRY(select_check(q, q_rs, h->cfg.n_actions, n, epsilon, env_offset, t, out));
  DevGuard _dg(h->device);
  const int64_t mb = h->cfg.max_batch;
  for (int64_t r = 0; r < n; r += mb) {
    const int32_t nb = (int32_t)std::min(mb, n - r);
    PORL_TRY(porl_qnet_forward(h, which, states + r * s_rs, s_rs, nb, q + r * q_rs, q_rs, stream));
  }
  return select_launch(q, q_rs, h->cfg.n_actions, n, epsilon, seed, env_offset, t, out, (hipStream_t)stream);
}

int porl_dist_select(const float* z, int64_t z_rs, const porl_dist_head* head, int64_t n, float* q, int64_t q_rs,
                     double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, int64_t* out, void* stream) {
  if (!z) PORL_FAIL(PORL_ERR_INVALID, "null outputs z");
  PORL_TRY(dist_select_check(head, -1, n, q, q_rs, epsilon, env_offset, t, out));
  if (z_rs < (int64_t)head->n_actions * head->n_sub || z_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "z_rs %lld: a row of outputs is %d x %d floats", (long long)z_rs, head->n_actions, head->n_sub);
  DevGuard _dg(device_of(out));
  return dist_select_launch(z, z_rs, head, n, q, q_rs, epsilon, seed, env_offset, t, out, (hipStream_t)stream);
}

// chunks of max_batch: stage the states, forward, and the select kernel on the output rows where the forward left them
int porl_qnet_act_rows_dist(porl_qnet* h, int which, const float* states, int64_t s_rs, int64_t n, const porl_dist_head* head,
                            float* q, int64_t q_rs, double epsilon, uint64_t seed, int64_t env_offset, uint64_t t,
                            int64_t* out, void* stream) {
  PORL_TRY(qnet_ready(h, false));
  if (which != 0 && which != 1) PORL_FAIL(PORL_ERR_INVALID, "which %d: 0 online, 1 target", which);
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  if (s_rs < h->cfg.state_dim || s_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "s_rs %lld: a state is %d floats", (long long)s_rs, h->cfg.state_dim);
  const int L = h->cfg.n_hidden;
  PORL_TRY(dist_select_check(head, h->cfg.n_actions, n, q, q_rs, epsilon, env_offset, t, out));
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t mb = h->cfg.max_batch;
  for (int64_t r = 0; r < n; r += mb) {
    const int32_t nb = (int32_t)std::min(mb, n - r);
    PORL_TRY(porl_qnet_load_batch(h, nb, states + r * s_rs, s_rs, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, stream));
    h->batch = 0;
    float* z = nullptr;
    PORL_TRY(qnet_forward_one(h, which ? h->buf.params_tgt : h->buf.params, h->buf.workspace + h->ws.xs, false, nb, s, &z));
    PORL_TRY(dist_select_launch(z, h->ld[L], head, nb, q + r * q_rs, q_rs, epsilon, seed, env_offset + r, t, out + r, s));
  }
  return PORL_OK;
}

int porl_bcq_select(const float* q, int64_t q_rs, const float* logits, int64_t z_rs, int32_t n_actions, int64_t n,
                    float threshold, double epsilon, uint64_t seed, int64_t env_offset, uint64_t t, float* mask, int64_t* out,
                    void* stream) {
  PORL_TRY(bcq_select_check(q, q_rs, logits, z_rs, n_actions, n, threshold, epsilon, env_offset, t, mask, out));
  DevGuard _dg(device_of(out));
  return bcq_select_launch(q, q_rs, logits, z_rs, n_actions, n, threshold, epsilon, seed, env_offset, t, mask, out,
                           (hipStream_t)stream);
}

// chunks of the smaller max_batch: the Q engine's forward into q, the behaviour engine's into logits; one select launch
int porl_qnet_act_rows_bcq(porl_qnet* h, porl_qnet* beh, int which, const float* states, int64_t s_rs, int64_t n, float* q,
                           int64_t q_rs, float* logits, int64_t z_rs, float threshold, double epsilon, uint64_t seed,
                           int64_t env_offset, uint64_t t, float* mask, int64_t* out, void* stream) {
  PORL_TRY(qnet_ready(h, false));
  PORL_TRY(qnet_ready(beh, false));
  if (which != 0 && which != 1) PORL_FAIL(PORL_ERR_INVALID, "which %d: 0 online, 1 target", which);
  if (beh == h) PORL_FAIL(PORL_ERR_INVALID, "the behaviour engine must not be the Q engine");
  if (beh->device != h->device) PORL_FAIL(PORL_ERR_INVALID, "the two engines live on different devices");
  if (beh->cfg.state_dim != h->cfg.state_dim || beh->cfg.n_actions != h->cfg.n_actions)
    PORL_FAIL(PORL_ERR_INVALID, "behaviour network (%d -> %d) does not match the Q network (%d -> %d)", beh->cfg.state_dim,
              beh->cfg.n_actions, h->cfg.state_dim, h->cfg.n_actions);
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  if (s_rs < h->cfg.state_dim || s_rs > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "s_rs %lld: a state is %d floats", (long long)s_rs, h->cfg.state_dim);
  PORL_TRY(bcq_select_check(q, q_rs, logits, z_rs, h->cfg.n_actions, n, threshold, epsilon, env_offset, t, mask, out));
  if (q == logits) PORL_FAIL(PORL_ERR_INVALID, "q and logits must be two tables");
  DevGuard _dg(h->device);
  const int64_t mb = std::min(h->cfg.max_batch, beh->cfg.max_batch);
  for (int64_t r = 0; r < n; r += mb) {
    const int32_t nb = (int32_t)std::min(mb, n - r);
    PORL_TRY(porl_qnet_forward(h, which, states + r * s_rs, s_rs, nb, q + r * q_rs, q_rs, stream));
    PORL_TRY(porl_qnet_forward(beh, 0, states + r * s_rs, s_rs, nb, logits + r * z_rs, z_rs, stream));
  }
  return bcq_select_launch(q, q_rs, logits, z_rs, h->cfg.n_actions, n, threshold, epsilon, seed, env_offset, t, mask, out,
                           (hipStream_t)stream);
}

}  // extern "C"
