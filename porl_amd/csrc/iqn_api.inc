// IQN engine (porl_iqn_*): one learn step of IQNTrainer (reference src/porl/train/iqn_trainer.py:92-134) and its greedy
// action (:82-91) from one native call each, on the trainer's own flat parameter / gradient / Adam buffers.  Included by
// porl_api.hip.
//
// Network (src/porl/net/iqn_network.py:10-62), tensors in parameters() order:
//   0/1 feature_net.0 (H, S) + bias   2/3 feature_net.2 (H, H) + bias   4/5 quantile_embedding (H, E) + bias
//   6/7 value_net.0 (H, H) + bias     8/9 value_net.2 (A, H) + bias
// Launches of porl_iqn_learn (B rows, N' / N'' fractions):
//   gather | feature layer 0, 1 (three forwards grouped) | mix | value layer 0, 1 (grouped) | head | mean loss |
//   value.2 wgrad + dgrad | value.0 wgrad + dgrad | Hadamard backward | embedding wgrad | feature.2 wgrad + dgrad |
//   feature.0 wgrad | clip (3) | Adam                                                                         = 18
// porl_iqn_learn_sampled is the same body: its gather launch draws the rows (QnetGatherArgs' samp_* fields) and one launch
// in front of it writes tau' and tau'' from the keyed stream (csrc/iqn_vector.hpp) into the workspace                  = 19
// Launches of porl_iqn_act_rows, per chunk of max_batch robots (m robots, K fractions each):
//   staging (states + fractions) | feature layer 0, 1 (M = m) | mix (m * K rows) | value layer 0, 1 | rows head       = 7

namespace {

enum { IQN_F0W = 0, IQN_F0B, IQN_F1W, IQN_F1B, IQN_QEW, IQN_QEB, IQN_V0W, IQN_V0B, IQN_V1W, IQN_V1B };

}  // namespace

struct porl_iqn {
  porl_iqn_cfg cfg;
  porl_iqn_buffers buf{};
  bool bound = false;
  int device = -1;
  int Sp = 0, Hp = 0, Ap = 0;                    // padded leading dimensions of the workspace rows
  struct {
    int64_t xs, xn, rew, done, actions;          // actions: int64 stored in 2 floats each
    int64_t f0[3], feat[3], emb0, mix[3], hv[3], z[3];
    int64_t dz, row_loss, dhv, dmix, demb, dfeat, df0, clip;
    int64_t taup, taupp;                         // fractions drawn on the device: tau' | tau'' and the act path's
    int64_t total;
  } ws;
  Tune tune = g_tune;
  const void* act_out_host = nullptr;            // porl_iqn_act: last record pointer seen and its device address
  int32_t* act_out_dev = nullptr;
};

namespace {

int iqn_ready(const porl_iqn* h) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_iqn_bind() has not been called");
  return 0;
}

// one Linear layer of up to three forwards as one grouped launch; the tile is the one problem 0 would get alone
int iqn_fwd_layer(porl_iqn* h, int nprob, const float* const* in, int ldin, const int* M, const float* const* par,
                  int wi, float* const* out, int ldo, int Nn, int K, int act, hipStream_t s) {
  GemmGroup g{};
  g.nprob = nprob;
  for (int k = 0; k < nprob; ++k) {
    GemmProb p = make_prob(GEMM_NT, in[k], ldin, par[k] + h->cfg.offset[wi], K, out[k], ldo, M[k], Nn, K);
    p.bias = par[k] + h->cfg.offset[wi + 1];
    p.act = act;
    g.p[k] = p;
  }
  GemmGroup one{};
  one.nprob = 1; one.p[0] = g.p[0];
  return launch_group(g, pick_tile(one, h->tune), h->tune, s);
}

// dW = dZ^T In (+ bias gradient as column sums) into the flat gradient buffer and, when dprev is given, dIn = dZ W
// (masked by 1[mask > 0] when mask is given) — one launch
int iqn_bwd_layer(porl_iqn* h, const float* dz, int lddz, const float* in, int ldin, int wi, int out_d, int in_d, int rows,
                  float* dprev, int ldprev, const float* mask, int ldmask, hipStream_t s) {
  float* G = h->buf.grads;
  GemmGroup g{};
  g.p[0] = make_prob(GEMM_TN, dz, lddz, in, ldin, G + h->cfg.offset[wi], in_d, out_d, in_d, rows);
  g.p[0].colsum = G + h->cfg.offset[wi + 1];
  g.nprob = 1;
  if (dprev) {
    GemmProb q = make_prob(GEMM_NN, dz, lddz, h->buf.params + h->cfg.offset[wi], in_d, dprev, ldprev, rows, in_d, out_d);
    q.mask = mask; q.ldmask = ldmask;
    g.p[g.nprob++] = q;
  }
  return launch_group(g, TILE_64x64, h->tune, s);
}

int iqn_launch_mix(const IqnMixArgs& a, hipStream_t s) {
  int rows = 0;
  for (int k = 0; k < a.nprob; ++k) rows = std::max(rows, a.p[k].rows);
  ProfScope ps("iqn_mix_kernel", s, 0.0, 0.0);
  hipLaunchKernelGGL(iqn_mix_kernel, dim3(cdiv(a.H, IQN_MIX_COLS), cdiv(rows, IQN_MIX_ROWS), a.nprob), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// draw and element range of the fraction stream: the counter packs (draw, e) as (draw << 32) | e
int iqn_tau_range_ok(uint64_t draw, int64_t first, int64_t count) {
  if (draw > (uint64_t)IQN_TAU_MAX_DRAW) PORL_FAIL(PORL_ERR_INVALID, "draw %llu above 2^32 - 1", (unsigned long long)draw);
  if (first < 0 || first >= IQN_TAU_MAX_ELEMS) PORL_FAIL(PORL_ERR_INVALID, "first %lld outside [0, 2^32)", (long long)first);
  if (count < 1 || count > IQN_TAU_MAX_ELEMS - first)
    PORL_FAIL(PORL_ERR_INVALID, "count %lld: elements [%lld, %lld) must be non-empty and end at 2^32", (long long)count, (long long)first, (long long)(first + count));
  return PORL_OK;
}

int iqn_launch_taus(const IqnTauArgs& a, int njobs, hipStream_t s) {
  int64_t most = 0;
  for (int k = 0; k < njobs; ++k) most = std::max(most, a.job[k].count);
  hipLaunchKernelGGL(iqn_taus_kernel, dim3((unsigned)((most + 255) / 256), njobs), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// the checks porl_iqn_select_rows and porl_iqn_act_rows share (select_check's rules, in this file's words)
int iqn_rows_check(int64_t n, int32_t n_tau, int32_t max_tau, int32_t n_actions, double epsilon, uint64_t t, int64_t env_offset,
                   const float* q, int64_t q_rs, const int64_t* out) {
  if (!q) PORL_FAIL(PORL_ERR_INVALID, "null q");
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (n < 1 || n > (int64_t(1) << 24)) PORL_FAIL(PORL_ERR_INVALID, "n %lld outside [1, 2^24]", (long long)n);
  if (n_tau < 1 || n_tau > max_tau) PORL_FAIL(PORL_ERR_INVALID, "n_tau %d outside [1,%d]", n_tau, max_tau);
  if (n_actions < 1 || n_actions > IQN_MAX_A) PORL_FAIL(PORL_ERR_INVALID, "n_actions %d outside [1,%d]", n_actions, IQN_MAX_A);
  if (q_rs < n_actions || q_rs > (int64_t(1) << 24)) PORL_FAIL(PORL_ERR_INVALID, "q_rs %lld: a row of action values is %d floats", (long long)q_rs, n_actions);
  if (!(epsilon >= 0.0 && epsilon <= 1.0)) PORL_FAIL(PORL_ERR_INVALID, "epsilon %g outside [0, 1]", epsilon);
  if (env_offset < 0 || env_offset > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "env_offset %lld outside [0, 2^40]", (long long)env_offset);
  if (t > (uint64_t)IQN_TAU_MAX_DRAW) PORL_FAIL(PORL_ERR_INVALID, "act-step t %llu above 2^32 - 1", (unsigned long long)t);
  return PORL_OK;
}

int iqn_launch_rows_head(const float* z, int64_t ld, int64_t n, int32_t n_tau, int32_t n_actions, double epsilon, uint64_t seed,
                         uint64_t t, int64_t env_offset, float* q, int64_t q_rs, int64_t* out, hipStream_t s) {
  IqnRowsHeadArgs a{};
  a.z = z; a.ld = (long long)ld; a.q = q; a.q_rs = (long long)q_rs; a.out = reinterpret_cast<long long*>(out);
  a.n = (long long)n; a.env_offset = (long long)env_offset; a.t = (long long)t;
  a.epsilon = epsilon; a.seed = seed; a.K = n_tau; a.A = n_actions;
  a.vec = aligned16(z) && ld % 4 == 0;
  ProfScope ps("iqn_rows_head_kernel", s, 0.0, 0.0);
  hipLaunchKernelGGL(iqn_rows_head_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // namespace

extern "C" {

int porl_iqn_create(const porl_iqn_cfg* c, porl_iqn** out) {
  if (!c || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (c->state_dim < 1 || c->n_actions < 1 || c->embedding_dim < 1 || c->hidden < 1 || c->max_batch < 1 || c->max_tau < 1)
    PORL_FAIL(PORL_ERR_INVALID, "dimensions must be positive");
  if (c->embedding_dim > IQN_MAX_E) PORL_FAIL(PORL_ERR_UNSUPPORTED, "embedding_dim %d > %d", c->embedding_dim, IQN_MAX_E);
  if (c->max_tau > IQN_MAX_TAU) PORL_FAIL(PORL_ERR_UNSUPPORTED, "max_tau %d > %d", c->max_tau, IQN_MAX_TAU);
  if (c->n_actions > IQN_MAX_A) PORL_FAIL(PORL_ERR_UNSUPPORTED, "n_actions %d > %d", c->n_actions, IQN_MAX_A);
  if ((int64_t)c->max_batch * c->max_tau > (1 << 20) || c->hidden > (1 << 14) || c->state_dim > (1 << 14))
    PORL_FAIL(PORL_ERR_UNSUPPORTED, "max_batch x max_tau > 2^20 rows, or a layer wider than 2^14");
  const int64_t S = c->state_dim, H = c->hidden, E = c->embedding_dim, A = c->n_actions;
  const int64_t numel[PORL_IQN_TENSORS] = {H * S, H, H * H, H, H * E, H, H * H, H, A * H, A};
  int64_t end = 0;
  for (int i = 0; i < PORL_IQN_TENSORS; ++i) {
    if (c->offset[i] < end || c->offset[i] % 4) PORL_FAIL(PORL_ERR_INVALID, "tensor %d: offset %lld overlaps its predecessor or is not a multiple of 4", i, (long long)c->offset[i]);
    end = c->offset[i] + numel[i];
  }
  if (c->n_params < end || c->n_params % 4) PORL_FAIL(PORL_ERR_INVALID, "n_params %lld: below the last tensor's end %lld or not a multiple of 4", (long long)c->n_params, (long long)end);
  porl_iqn* h = new porl_iqn();
  h->cfg = *c;
  h->Sp = (int)ru4(S); h->Hp = (int)ru4(H); h->Ap = (int)ru4(A);
  const int64_t B = c->max_batch, R = B * c->max_tau;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += ru4(n); return r; };
  h->ws.xs = take(B * h->Sp); h->ws.xn = take(B * h->Sp);
  h->ws.rew = take(B); h->ws.done = take(B); h->ws.actions = take(2 * B);
  for (int k = 0; k < 3; ++k) { h->ws.f0[k] = take(B * h->Hp); h->ws.feat[k] = take(B * h->Hp); }
  h->ws.emb0 = take(R * h->Hp);
  for (int k = 0; k < 3; ++k) { h->ws.mix[k] = take(R * h->Hp); h->ws.hv[k] = take(R * h->Hp); h->ws.z[k] = take(R * h->Ap); }
  h->ws.dz = take(R * h->Ap); h->ws.row_loss = take(B);
  h->ws.dhv = take(R * h->Hp); h->ws.dmix = take(R * h->Hp); h->ws.demb = take(R * h->Hp);
  h->ws.dfeat = take(B * h->Hp); h->ws.df0 = take(B * h->Hp);
  h->ws.clip = take(2 * CLIP_BLOCKS);                       // CLIP_BLOCKS doubles
  h->ws.taup = take(R); h->ws.taupp = take(R);
  h->ws.total = o;
  *out = h;
  return PORL_OK;
}

void porl_iqn_destroy(porl_iqn* h) { delete h; }
int64_t porl_iqn_workspace_floats(const porl_iqn* h) { return h ? h->ws.total : 0; }

int porl_iqn_bind(porl_iqn* h, const porl_iqn_buffers* b) {
  if (!h || !b) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  const void* ptrs[] = {b->params, b->params_tgt, b->grads, b->adam_m, b->adam_v, b->workspace, b->stats};
  for (const void* p : ptrs) {
    if (!p) PORL_FAIL(PORL_ERR_INVALID, "null buffer");
    if (!aligned16(p)) PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  }
  h->buf = *b;
  h->bound = true;
  h->device = device_of(b->workspace);
  return PORL_OK;
}

int porl_iqn_mix(int32_t nprob, const porl_iqn_mix_prob* probs, int32_t embedding_dim, int32_t hidden, void* stream) {
  if (!probs || nprob < 1 || nprob > 3) PORL_FAIL(PORL_ERR_INVALID, "need 1..3 problems");
  if (embedding_dim < 1 || embedding_dim > IQN_MAX_E) PORL_FAIL(PORL_ERR_INVALID, "embedding_dim %d outside [1,%d]", embedding_dim, IQN_MAX_E);
  if (hidden < 1) PORL_FAIL(PORL_ERR_INVALID, "hidden %d must be >= 1", hidden);
  IqnMixArgs a{};
  a.nprob = nprob; a.E = embedding_dim; a.H = hidden;
  for (int k = 0; k < nprob; ++k) {
    const porl_iqn_mix_prob& q = probs[k];
    if (!q.feat || !q.taus || !q.weight || !q.bias || !q.out) PORL_FAIL(PORL_ERR_INVALID, "problem %d: null argument", k);
    if (q.batch < 1 || q.n_tau < 1 || (int64_t)q.batch * q.n_tau > (1 << 24)) PORL_FAIL(PORL_ERR_INVALID, "problem %d: batch %d, n_tau %d", k, q.batch, q.n_tau);
    if (q.ldf < hidden || q.ldo < hidden || q.ldw < embedding_dim) PORL_FAIL(PORL_ERR_INVALID, "problem %d: a row stride is below its row's width", k);
    a.p[k] = IqnMixProb{q.feat, (long)q.ldf, q.taus, q.weight, (long)q.ldw, q.bias, q.out, (long)q.ldo, q.emb, q.batch * q.n_tau, q.n_tau};
  }
  DevGuard _dg(device_of(probs[0].out));
  return iqn_launch_mix(a, (hipStream_t)stream);
}

int porl_iqn_head(const float* z_cur, const float* z_online_next, const float* z_target_next, int64_t ld, const int64_t* actions,
                  const float* rewards, const float* dones, const float* taus_prime, int32_t batch, int32_t n_cur, int32_t n_tgt,
                  int32_t n_actions, float gamma, float kappa, float* dz, float* row_loss, int64_t* next_actions, void* stream) {
  if (!z_cur || !z_online_next || !z_target_next || !actions || !rewards || !dones || !taus_prime || !dz || !row_loss)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (batch < 1 || n_cur < 1 || n_tgt < 1 || n_actions < 1) PORL_FAIL(PORL_ERR_INVALID, "batch %d, n_cur %d, n_tgt %d, n_actions %d must be >= 1", batch, n_cur, n_tgt, n_actions);
  if (n_cur > IQN_MAX_TAU || n_tgt > IQN_MAX_TAU) PORL_FAIL(PORL_ERR_INVALID, "n_cur %d / n_tgt %d above %d", n_cur, n_tgt, IQN_MAX_TAU);
  if (n_actions > IQN_MAX_A) PORL_FAIL(PORL_ERR_INVALID, "n_actions %d above %d", n_actions, IQN_MAX_A);
  if (ld < n_actions) PORL_FAIL(PORL_ERR_INVALID, "row stride %lld < n_actions %d", (long long)ld, n_actions);
  DevGuard _dg(device_of(dz));
  IqnHeadArgs a{z_cur, z_online_next, z_target_next, (long)ld, actions, rewards, dones, taus_prime, dz, row_loss, next_actions,
                batch, n_cur, n_tgt, n_actions, gamma, kappa, 1.0f / batch};
  hipLaunchKernelGGL(iqn_head_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// The learn step on `rows`: idx and the caller's fractions, or — sampled — the keyed draw of rows.samp_n rows inside the
// gather launch and tau' / tau'' from the fraction stream (uses 1 and 2, draw rows.samp_step) in the workspace.
static int iqn_learn_rows(porl_iqn* h, const QnetRows& rows, bool sampled, int32_t batch, const float* taus_prime, int32_t n_cur,
                          const float* taus_dprime, int32_t n_tgt, const porl_iqn_hyper* hp, void* stream) {
  PORL_TRY(iqn_ready(h));
  const float* states = rows.states; const float* next_states = rows.next_states;
  const int64_t s_rs = rows.s_rs, n_rs = rows.n_rs;
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hp");
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  if (!rows.actions) PORL_FAIL(PORL_ERR_INVALID, "null actions");
  if (!rows.rewards) PORL_FAIL(PORL_ERR_INVALID, "null rewards");
  if (!next_states) PORL_FAIL(PORL_ERR_INVALID, "null next_states");
  if (!rows.dones) PORL_FAIL(PORL_ERR_INVALID, "null dones");
  if (!sampled && !taus_prime) PORL_FAIL(PORL_ERR_INVALID, "null taus_prime");
  if (!sampled && !taus_dprime) PORL_FAIL(PORL_ERR_INVALID, "null taus_dprime");
  const porl_iqn_cfg& c = h->cfg;
  if (batch < 1 || batch > c.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, c.max_batch);
  if (sampled && (rows.samp_n < batch || rows.samp_n > (int64_t(1) << 40)))
    PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld: need batch %d <= n_rows <= 2^40", (long long)rows.samp_n, batch);
  if (s_rs < c.state_dim) PORL_FAIL(PORL_ERR_INVALID, "s_rs %lld below state_dim %d", (long long)s_rs, c.state_dim);
  if (n_rs < c.state_dim) PORL_FAIL(PORL_ERR_INVALID, "n_rs %lld below state_dim %d", (long long)n_rs, c.state_dim);
  if (n_cur < 1 || n_cur > c.max_tau) PORL_FAIL(PORL_ERR_INVALID, "n_cur %d outside [1,%d]", n_cur, c.max_tau);
  if (n_tgt < 1 || n_tgt > c.max_tau) PORL_FAIL(PORL_ERR_INVALID, "n_tgt %d outside [1,%d]", n_tgt, c.max_tau);
  if (sampled) PORL_TRY(iqn_tau_range_ok(rows.samp_step, 0, (int64_t)batch * std::max(n_cur, n_tgt)));
  if (hp->step < 1) PORL_FAIL(PORL_ERR_INVALID, "step %d: adam step must be >= 1", hp->step);
  if (!(hp->max_norm > 0.f)) PORL_FAIL(PORL_ERR_INVALID, "max_norm must be positive");
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  float* W = h->buf.workspace;
  const int B = batch, S = c.state_dim, H = c.hidden, E = c.embedding_dim, A = c.n_actions;
  const int Sp = h->Sp, Hp = h->Hp, Ap = h->Ap;
  if (sampled) {
    IqnTauArgs a{};
    a.job[0] = IqnTauJob{W + h->ws.taup, iqn_tau_key(rows.samp_seed, 1), rows.samp_step, 0, (int64_t)B * n_cur};
    a.job[1] = IqnTauJob{W + h->ws.taupp, iqn_tau_key(rows.samp_seed, 2), rows.samp_step, 0, (int64_t)B * n_tgt};
    PORL_TRY(iqn_launch_taus(a, 2, s));
    taus_prime = W + h->ws.taup; taus_dprime = W + h->ws.taupp;
  }
  {
    QnetGatherArgs a{};
    a.states = states; a.next_states = next_states; a.s_rs = (long)s_rs; a.n_rs = (long)n_rs;
    a.actions = rows.actions; a.rew = rows.rewards; a.done = rows.dones; a.idx = rows.idx;
    a.xs = W + h->ws.xs; a.xn = W + h->ws.xn; a.act_out = reinterpret_cast<int64_t*>(W + h->ws.actions);
    a.rew_out = W + h->ws.rew; a.done_out = W + h->ws.done;
    a.B = B; a.S = S; a.ld = Sp;
    if (sampled) {
      a.samp_n = rows.samp_n; a.samp_seed = rows.samp_seed; a.samp_step = rows.samp_step; a.samp_hb = feistel_half_bits(rows.samp_n);
      a.idx = nullptr;
    }
    hipLaunchKernelGGL(qnet_gather_kernel, dim3((unsigned)(((long)B * Sp + 255) / 256)), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  // forward 0: online net, tau' on s (activations kept); 1: online net, tau'' on s'; 2: target net, tau'' on s'
  const float* par[3] = {h->buf.params, h->buf.params, h->buf.params_tgt};
  const float* x[3] = {W + h->ws.xs, W + h->ws.xn, W + h->ws.xn};
  const int nt[3] = {n_cur, n_tgt, n_tgt};
  const int Mb[3] = {B, B, B}, Mr[3] = {B * n_cur, B * n_tgt, B * n_tgt};
  float *f0[3], *feat[3], *mix[3], *hv[3], *z[3];
  for (int k = 0; k < 3; ++k) {
    f0[k] = W + h->ws.f0[k]; feat[k] = W + h->ws.feat[k]; mix[k] = W + h->ws.mix[k]; hv[k] = W + h->ws.hv[k]; z[k] = W + h->ws.z[k];
  }
  PORL_TRY(iqn_fwd_layer(h, 3, x, Sp, Mb, par, IQN_F0W, f0, Hp, H, S, ACT_RELU, s));
  PORL_TRY(iqn_fwd_layer(h, 3, f0, Hp, Mb, par, IQN_F1W, feat, Hp, H, H, ACT_RELU, s));
  {
    IqnMixArgs a{};
    a.nprob = 3; a.E = E; a.H = H;
    for (int k = 0; k < 3; ++k)
      a.p[k] = IqnMixProb{feat[k], (long)Hp, k == 0 ? taus_prime : taus_dprime, par[k] + c.offset[IQN_QEW], (long)E,
                          par[k] + c.offset[IQN_QEB], mix[k], (long)Hp, k == 0 ? W + h->ws.emb0 : nullptr, Mr[k], nt[k]};
    PORL_TRY(iqn_launch_mix(a, s));
  }
  PORL_TRY(iqn_fwd_layer(h, 3, mix, Hp, Mr, par, IQN_V0W, hv, Hp, H, H, ACT_RELU, s));
  PORL_TRY(iqn_fwd_layer(h, 3, hv, Hp, Mr, par, IQN_V1W, z, Ap, A, H, ACT_NONE, s));
  float* dz = W + h->ws.dz;
  float* row_loss = W + h->ws.row_loss;
  {
    IqnHeadArgs a{z[0], z[1], z[2], (long)Ap, reinterpret_cast<const int64_t*>(W + h->ws.actions), W + h->ws.rew, W + h->ws.done,
                  taus_prime, dz, row_loss, nullptr, B, n_cur, n_tgt, A, hp->gamma, hp->kappa, 1.0f / B};
    ProfScope ps("iqn_head_kernel", s, 0.0, 0.0);
    hipLaunchKernelGGL(iqn_head_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  {
    ReduceArgs r{};
    add_reduce(r, h->buf.stats, row_loss, 1, 1, B, 0, 1.0f / B);       // porl_reduce_mean's job
    PORL_TRY(launch_reduce(r, s));
  }
  // backward of forward 0, top down; every gradient tensor is stored whole (the padding between tensors is never written)
  const int R0 = Mr[0];
  float* dhv = W + h->ws.dhv; float* dmix = W + h->ws.dmix; float* demb = W + h->ws.demb;
  float* dfeat = W + h->ws.dfeat; float* df0 = W + h->ws.df0;
  PORL_TRY(iqn_bwd_layer(h, dz, Ap, hv[0], Hp, IQN_V1W, A, H, R0, dhv, Hp, hv[0], Hp, s));
  PORL_TRY(iqn_bwd_layer(h, dhv, Hp, mix[0], Hp, IQN_V0W, H, H, R0, dmix, Hp, nullptr, 0, s));
  hipLaunchKernelGGL(iqn_hadamard_bwd_relu_kernel, dim3(iqn_blocks((long)B * H)), dim3(256), 0, s, dmix, feat[0], W + h->ws.emb0, B,
                     n_cur, H, (long)Hp, dfeat, demb);
  PORL_HIP(hipGetLastError());
  hipLaunchKernelGGL(iqn_embed_wgrad_kernel, dim3(cdiv(H, IQN_WG_T), cdiv(E, IQN_WG_T)), dim3(256), 0, s, demb, (long)Hp, taus_prime, R0, H,
                     E, h->buf.grads + c.offset[IQN_QEW], (long)E, h->buf.grads + c.offset[IQN_QEB]);
  PORL_HIP(hipGetLastError());
  PORL_TRY(iqn_bwd_layer(h, dfeat, Hp, f0[0], Hp, IQN_F1W, H, H, B, df0, Hp, f0[0], Hp, s));
  PORL_TRY(iqn_bwd_layer(h, df0, Hp, x[0], Sp, IQN_F0W, H, S, B, nullptr, 0, nullptr, 0, s));
  // clip_grad_norm_ (porl_grad_clip's launches): total norm -> stats[1], coefficient -> stats[2]
  {
    const int64_t n = c.n_params;
    double* part = reinterpret_cast<double*>(W + h->ws.clip);
    const int nb = (int)std::min<long>(CLIP_BLOCKS, std::max<long>(1, (n + 4095) / 4096));
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, h->buf.grads, (long)n, part);
    PORL_HIP(hipGetLastError());
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, s, part, nb, hp->max_norm, h->buf.stats + 1);
    PORL_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_by_kernel, dim3(iqn_blocks(n)), dim3(256), 0, s, h->buf.grads, (long)n, h->buf.stats + 1);
    PORL_HIP(hipGetLastError());
  }
  return adam_launch(h->buf.params, h->buf.grads, h->buf.adam_m, h->buf.adam_v, nullptr, c.n_params, hp->lr, hp->step,
                     hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0, s);
}

int porl_iqn_learn(porl_iqn* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                   const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                   const float* taus_prime, int32_t n_cur, const float* taus_dprime, int32_t n_tgt, const porl_iqn_hyper* hp,
                   void* stream) {
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, idx};
  return iqn_learn_rows(h, rows, false, batch, taus_prime, n_cur, taus_dprime, n_tgt, hp, stream);
}

int porl_iqn_learn_sampled(porl_iqn* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                           const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, int32_t batch,
                           uint64_t seed, uint64_t draw, int32_t n_cur, int32_t n_tgt, const porl_iqn_hyper* hp, void* stream) {
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, nullptr, n_rows, seed, draw};
  return iqn_learn_rows(h, rows, true, batch, nullptr, n_cur, nullptr, n_tgt, hp, stream);
}

int porl_iqn_draw_taus(uint64_t seed, int32_t use, uint64_t draw, int64_t first, int64_t count, float* out, void* stream) {
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (use < 0 || use > 2) PORL_FAIL(PORL_ERR_INVALID, "use %d: 0 acting, 1 tau', 2 tau''", use);
  PORL_TRY(iqn_tau_range_ok(draw, first, count));
  DevGuard _dg(device_of(out));
  IqnTauArgs a{};
  a.job[0] = IqnTauJob{out, iqn_tau_key(seed, use), draw, first, count};
  return iqn_launch_taus(a, 1, (hipStream_t)stream);
}

int porl_iqn_select_rows(const float* z, int64_t ld, int64_t n, int32_t n_tau, int32_t n_actions, double epsilon, uint64_t seed,
                         uint64_t t, int64_t env_offset, float* q, int64_t q_rs, int64_t* out, void* stream) {
  if (!z) PORL_FAIL(PORL_ERR_INVALID, "null z");
  PORL_TRY(iqn_rows_check(n, n_tau, IQN_MAX_TAU, n_actions, epsilon, t, env_offset, q, q_rs, out));
  if (ld < n_actions || ld > IQN_ROWS_MAX_LD) PORL_FAIL(PORL_ERR_INVALID, "ld %lld outside [n_actions %d, %d]", (long long)ld, n_actions, IQN_ROWS_MAX_LD);
  DevGuard _dg(device_of(out));
  return iqn_launch_rows_head(z, ld, n, n_tau, n_actions, epsilon, seed, t, env_offset, q, q_rs, out, (hipStream_t)stream);
}

// chunks of max_batch robots, each through the rows of forward 1 (a learn step on the same stream has finished with them)
int porl_iqn_act_rows(porl_iqn* h, int which, const float* states, int64_t s_rs, int64_t n, const float* taus, int32_t n_tau,
                      double epsilon, uint64_t seed, uint64_t t, int64_t env_offset, float* q, int64_t q_rs, int64_t* out,
                      void* stream) {
  PORL_TRY(iqn_ready(h));
  if (which != 0 && which != 1) PORL_FAIL(PORL_ERR_INVALID, "which %d: 0 online, 1 target", which);
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  const porl_iqn_cfg& c = h->cfg;
  PORL_TRY(iqn_rows_check(n, n_tau, c.max_tau, c.n_actions, epsilon, t, env_offset, q, q_rs, out));
  if (s_rs < c.state_dim || s_rs > (int64_t(1) << 24)) PORL_FAIL(PORL_ERR_INVALID, "s_rs %lld below state_dim %d or above 2^24", (long long)s_rs, c.state_dim);
  if (!taus && (env_offset + n) * n_tau > IQN_TAU_MAX_ELEMS)
    PORL_FAIL(PORL_ERR_INVALID, "(env_offset %lld + n %lld) x n_tau %d: the fraction stream numbers elements below 2^32", (long long)env_offset, (long long)n, n_tau);
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  float* W = h->buf.workspace;
  const float* P = which ? h->buf.params_tgt : h->buf.params;
  const int S = c.state_dim, H = c.hidden, E = c.embedding_dim, A = c.n_actions, K = n_tau;
  const int Sp = h->Sp, Hp = h->Hp, Ap = h->Ap;
  float* x = W + h->ws.xn; float* tau = W + h->ws.taupp;
  float* f0 = W + h->ws.f0[1]; float* feat = W + h->ws.feat[1]; float* mix = W + h->ws.mix[1]; float* hv = W + h->ws.hv[1];
  float* z = W + h->ws.z[1];
  const float* par[1] = {P};
  const uint64_t key = iqn_tau_key(seed, 0);
  for (int64_t r = 0; r < n; r += c.max_batch) {
    const int m = (int)std::min<int64_t>(c.max_batch, n - r);
    {
      IqnStageArgs a{};
      a.states = states + r * s_rs; a.s_rs = (long long)s_rs; a.xs = x;
      a.taus = taus ? taus + r * K : nullptr; a.taus_out = tau;
      a.key = key; a.t = t; a.first_e = (long long)((env_offset + r) * K);
      a.m = m; a.S = S; a.Sp = Sp; a.K = K;
      const long groups = std::max((long)m * (Sp / 4), ((long)m * K + 3) / 4);
      hipLaunchKernelGGL(iqn_act_stage_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, a);
      PORL_HIP(hipGetLastError());
    }
    const int Mb[1] = {m}, Mr[1] = {m * K};
    { const float* in[1] = {x}; float* o[1] = {f0}; PORL_TRY(iqn_fwd_layer(h, 1, in, Sp, Mb, par, IQN_F0W, o, Hp, H, S, ACT_RELU, s)); }
    { const float* in[1] = {f0}; float* o[1] = {feat}; PORL_TRY(iqn_fwd_layer(h, 1, in, Hp, Mb, par, IQN_F1W, o, Hp, H, H, ACT_RELU, s)); }
    {
      IqnMixArgs a{};
      a.nprob = 1; a.E = E; a.H = H;
      a.p[0] = IqnMixProb{feat, (long)Hp, tau, P + c.offset[IQN_QEW], (long)E, P + c.offset[IQN_QEB], mix, (long)Hp, nullptr, m * K, K};
      PORL_TRY(iqn_launch_mix(a, s));
    }
    { const float* in[1] = {mix}; float* o[1] = {hv}; PORL_TRY(iqn_fwd_layer(h, 1, in, Hp, Mr, par, IQN_V0W, o, Hp, H, H, ACT_RELU, s)); }
    { const float* in[1] = {hv}; float* o[1] = {z}; PORL_TRY(iqn_fwd_layer(h, 1, in, Hp, Mr, par, IQN_V1W, o, Ap, A, H, ACT_NONE, s)); }
    PORL_TRY(iqn_launch_rows_head(z, Ap, m, K, A, epsilon, seed, t, env_offset + r, q + r * q_rs, q_rs, out + r, s));
  }
  return PORL_OK;
}

int porl_iqn_act(porl_iqn* h, int which, const porl_qnet_act_src* src, const float* taus, int32_t n_tau, int32_t n_stats,
                 int32_t* record, void* stream) {
  PORL_TRY(iqn_ready(h));
  if (!src) PORL_FAIL(PORL_ERR_INVALID, "null src");
  if (!taus) PORL_FAIL(PORL_ERR_INVALID, "null taus");
  if (!record) PORL_FAIL(PORL_ERR_INVALID, "null record");
  const porl_iqn_cfg& c = h->cfg;
  if (n_tau < 1 || n_tau > c.max_tau) PORL_FAIL(PORL_ERR_INVALID, "n_tau %d outside [1,%d]", n_tau, c.max_tau);
  if (n_stats < 0 || n_stats > 3) PORL_FAIL(PORL_ERR_INVALID, "n_stats %d outside [0,3]", n_stats);
  if (src->batch != 1) PORL_FAIL(PORL_ERR_INVALID, "batch %d: one state per call", src->batch);
  const int S = c.state_dim, H = c.hidden, E = c.embedding_dim, A = c.n_actions, Hp = h->Hp;
  DevGuard _dg(h->device);
  IqnActL0Args l0;
  if (src->states) {
    if (src->row < 0 || src->row >= src->n_rows) PORL_FAIL(PORL_ERR_INVALID, "row %lld outside the %lld-row array", (long long)src->row, (long long)src->n_rows);
    if (src->s_rs < S) PORL_FAIL(PORL_ERR_INVALID, "row stride %lld < state_dim %d", (long long)src->s_rs, S);
    l0.state = src->states + src->row * src->s_rs;
  } else {
    if (!src->inline_states) PORL_FAIL(PORL_ERR_INVALID, "no state source");
    if (S > IQN_ACT_MAX_INLINE) PORL_FAIL(PORL_ERR_INVALID, "inline state: %d floats > %d", S, IQN_ACT_MAX_INLINE);
    l0.state = nullptr;
    memcpy(l0.x_inline, src->inline_states, sizeof(float) * S);
  }
  if (record != h->act_out_host) {               // the record may be pinned host memory: the kernel stores through its device address
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, record) != hipSuccess) {
      (void)hipGetLastError();
      PORL_FAIL(PORL_ERR_INVALID, "act record is neither device memory nor pinned host memory");
    }
    int32_t* dev = nullptr;
    if (pa.type == hipMemoryTypeDevice) dev = record;
    else if (pa.type == hipMemoryTypeHost && pa.devicePointer) dev = static_cast<int32_t*>(pa.devicePointer);
    if (!dev) PORL_FAIL(PORL_ERR_INVALID, "act record is neither device memory nor pinned host memory");
    h->act_out_host = record;
    h->act_out_dev = dev;
  }
  hipStream_t s = (hipStream_t)stream;
  float* W = h->buf.workspace;
  const float* P = which ? h->buf.params_tgt : h->buf.params;
  // the act path borrows the rows of forward 1 (a learn step on the same stream has finished with them)
  float* f0 = W + h->ws.f0[1]; float* feat = W + h->ws.feat[1]; float* mix = W + h->ws.mix[1]; float* hv = W + h->ws.hv[1];
  l0.W = P + c.offset[IQN_F0W]; l0.ldw = S; l0.bias = P + c.offset[IQN_F0B]; l0.out = f0; l0.S = S; l0.H = H;
  hipLaunchKernelGGL(iqn_act_l0_kernel, dim3(cdiv(H, 4)), dim3(256), 0, s, l0);
  PORL_HIP(hipGetLastError());
  const float* par[1] = {P};
  {
    const float* in[1] = {f0}; float* out[1] = {feat}; const int M[1] = {1};
    PORL_TRY(iqn_fwd_layer(h, 1, in, Hp, M, par, IQN_F1W, out, Hp, H, H, ACT_RELU, s));
  }
  {
    IqnMixArgs a{};
    a.nprob = 1; a.E = E; a.H = H;
    a.p[0] = IqnMixProb{feat, (long)Hp, taus, P + c.offset[IQN_QEW], (long)E, P + c.offset[IQN_QEB], mix, (long)Hp, nullptr, n_tau, n_tau};
    PORL_TRY(iqn_launch_mix(a, s));
  }
  {
    const float* in[1] = {mix}; float* out[1] = {hv}; const int M[1] = {n_tau};
    PORL_TRY(iqn_fwd_layer(h, 1, in, Hp, M, par, IQN_V0W, out, Hp, H, H, ACT_RELU, s));
  }
  const int vec = H % 4 == 0 && aligned16(P + c.offset[IQN_V1W]) && aligned16(hv);        // (Hp == H then: both row strides are multiples of 4)
  IqnActHeadArgs a{hv, (long)Hp, P + c.offset[IQN_V1W], (long)H, P + c.offset[IQN_V1B], h->buf.stats, n_stats, h->act_out_dev, n_tau, H, A, vec};
  // up to 256 x 64 floats of dynamic LDS beside the kernel's static 256 bytes
  PORL_TRY(dyn_lds_once<&iqn_act_head_kernel>((int)sizeof(float) * IQN_MAX_TAU * IQN_MAX_A));
  hipLaunchKernelGGL(iqn_act_head_kernel, dim3(1), dim3(n_tau >= 16 ? 1024 : 256), sizeof(float) * n_tau * A, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
