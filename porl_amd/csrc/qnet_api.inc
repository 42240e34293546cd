// Q-network engine (porl_qnet_*): the discrete-action MLP S -> hidden... -> A of the Q-learning trainers (CQL, DQN,
// Double / dueling DQN, PER, BCQ, QR-DQN, C51; reference src/porl/net/q_network.py:8-30) and the stateless loss heads of
// the distributional trainers (porl_qr_loss, porl_c51_loss, porl_iqn_*).  Included by porl_api.hip.
//
// Two ways through one learn step:
//   one-launch path (qnet_fused.hpp): every width <= 128, at most QF_MAX_LIN Linear layers, the LDS plan fits —
//     step kernel (32 or 16 rows per block) + block-order reduction with Adam: qnet_fused_backward
//   multi-launch path (any widths): gather, forwards through the grouped GEMM, loss head, backward chain, Adam:
//     qnet_general_learn
// Every row-sourced entry point names where its minibatch comes from (QnetRows) and which loss variant it runs, and
// goes through qnet_learn_rows, the one place that chooses between the two.

// =====================================================================================================
// Discrete-action CQL engine (QNetwork S -> hidden... -> A; src/porl/net/q_network.py:8-30)
// =====================================================================================================
struct porl_qnet {
  porl_qnet_cfg cfg;
  MlpLayout net;
  int64_t n_params = 0;
  std::vector<TensorInfo> tensors;
  porl_qnet_buffers buf{};
  bool bound = false;
  int device = -1;
  int batch = 0;
  int Sp = 0, Ap = 0, ld[PORL_MAX_HIDDEN + 2] = {0};     // padded leading dims per layer output
  int wld[PORL_MAX_HIDDEN + 1] = {0};                    // row stride of layer l's weight image (floats)
  struct {
    int64_t xs, xn, rew, done, actions;                  // actions: int64 stored in 2 floats each
    int64_t act[PORL_MAX_HIDDEN + 1], tmp[2], dz[2], slab, part_td, part_pen, fslab, total;
    int64_t tmp2[2], row_loss;                           // porl_qnet_dist_learn: third forward's ping-pong, per-row losses
    int64_t mask;                                        // porl_qnet_bcq_learn*: (max_batch, n_actions) behaviour mask
  } ws;
  // one-launch path (qnet_fused.hpp): every width <= 128, at most QF_MAX_LIN Linear layers, LDS plan fits
  bool fused_ok = false;
  QnetFusedArgs fargs{};
  int fused_lds_bytes = 0;
  int fused2_lds_w2 = 0, fused2_lds_bytes = 0;       // two-group kernel: offset of the second weight image; 0 = does not fit
  QnetFusedArgs fargs16{};                           // the same plan for 16 rows per block (qnet_fused2_kernel<16>)
  int fused16_lds_w2 = 0, fused16_lds_bytes = 0;
  int64_t fslab_stride = 0;
  bool fslab_clean = false;          // alignment gaps of the flat layout are never written: zeroed once
  bool slab_clean = false;           // same for the split-K slabs of the multi-launch path
  Tune tune = g_tune;                // kernel selection: the process defaults at creation
  const void* act_out_host = nullptr;  // porl_qnet_act: last record pointer seen and its device address
  int32_t* act_out_dev = nullptr;
};

// ---- LDS plans (in floats) -----------------------------------------------------------------------------------------------
// What the step kernels (qnet_fused.hpp) and the mask kernel (bcq_mask.hpp) size their shared buffers by:
// maxw = the widest activation row among dims[first..n_lin], rounded up to 32; wmax = the largest layer as it is parked
// in LDS, round32(out) rows of the weight image plus one bias float per row.
struct QnetLdsWidths { int maxw = 0, wmax = 0; };
static QnetLdsWidths qnet_lds_widths(const int* dims, int n_lin, int first) {
  QnetLdsWidths w;
  for (int l = first; l <= n_lin; ++l) w.maxw = std::max(w.maxw, (dims[l] + 31) & ~31);
  for (int l = 0; l < n_lin; ++l) w.wmax = std::max(w.wmax, ((dims[l + 1] + 31) & ~31) * (((dims[l] + 15) & ~15) + 4 + 1));
  return w;
}

// Plan of a step kernel with `rows` minibatch rows per block, from fa.dims and fa.n_lin: every layer's activation rows,
// the target network's two ping-pong buffers, one weight image.  Returns the float count, which is also the offset of
// the two-group kernel's second image.
static int qnet_lds_plan(QnetFusedArgs& fa, int rows) {
  const QnetLdsWidths w = qnet_lds_widths(fa.dims, fa.n_lin, 0);
  int off = 0;
  for (int l = 0; l <= fa.n_lin; ++l) { fa.lds_act[l] = off; off += rows * (((fa.dims[l] + 31) & ~31) + 4); }
  fa.lds_tmp[0] = off; off += rows * (w.maxw + 4);
  fa.lds_tmp[1] = off; off += rows * (w.maxw + 4);
  fa.lds_w = off;
  return off + w.wmax;
}

static bool qnet_is_fused(const porl_qnet* h) { return h->fused_ok && h->tune.qnet_fused; }

extern "C" {

int porl_qnet_create(const porl_qnet_cfg* c, porl_qnet** out) {
  if (!c || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (c->state_dim < 1 || c->n_actions < 1 || c->max_batch < 1) PORL_FAIL(PORL_ERR_INVALID, "dimensions must be positive");
  if (c->n_hidden < 1 || c->n_hidden > PORL_MAX_HIDDEN) PORL_FAIL(PORL_ERR_INVALID, "n_hidden must be in [1,%d]", PORL_MAX_HIDDEN);
  if (c->n_actions > 4096) PORL_FAIL(PORL_ERR_UNSUPPORTED, "more than 4096 outputs");   // (A x N outputs of the distributional nets)
  porl_qnet* h = new porl_qnet();
  h->cfg = *c;
  const int L = c->n_hidden, B = c->max_batch;
  MlpLayout& m = h->net;
  m.n_lin = L + 1;
  m.dims[0] = c->state_dim;
  for (int l = 0; l < L; ++l) {
    if (c->hidden[l] < 1) { delete h; PORL_FAIL(PORL_ERR_INVALID, "hidden size must be positive"); }
    m.dims[l + 1] = c->hidden[l];
  }
  m.dims[L + 1] = c->n_actions;
  // Parameter layout = the image the one-launch step kernel parks in LDS (csrc/qnet_fused.hpp): layer l is
  // round32(out) rows of (round16(in) + 4) floats — the (out, in) weights in the top-left corner, zeros elsewhere —
  // directly followed by round32(out) bias floats.  A block stages a layer with one linear, fully coalesced copy:
  // no per-element address arithmetic, no bounds selects.  Zeros stay zeros under Adam (their gradient is always 0).
  int64_t cur = 0;
  for (int l = 0; l <= L; ++l) {
    const int rows = (m.dims[l + 1] + 31) & ~31;
    h->wld[l] = ((m.dims[l] + 15) & ~15) + 4;
    m.w[l] = cur;
    h->tensors.push_back({cur, m.dims[l + 1], m.dims[l]});
    cur += (int64_t)rows * h->wld[l];
    m.b[l] = cur;
    h->tensors.push_back({cur, 0, m.dims[l + 1]});
    cur += rows;
  }
  h->n_params = cur;
  h->Sp = (int)ru4(c->state_dim);
  h->Ap = (int)ru4(c->n_actions);
  int maxld = h->Ap;
  for (int l = 0; l <= L; ++l) { h->ld[l] = (int)ru4(m.dims[l + 1]); maxld = std::max(maxld, h->ld[l]); }
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += ru4(n); return r; };
  h->ws.xs = take((int64_t)B * h->Sp); h->ws.xn = take((int64_t)B * h->Sp);
  h->ws.rew = take(B); h->ws.done = take(B); h->ws.actions = take(2 * (int64_t)B);
  for (int l = 0; l <= L; ++l) h->ws.act[l] = take((int64_t)B * h->ld[l]);
  h->ws.tmp[0] = take((int64_t)B * maxld); h->ws.tmp[1] = take((int64_t)B * maxld);
  h->ws.dz[0] = take((int64_t)B * maxld); h->ws.dz[1] = take((int64_t)B * maxld);
  h->ws.slab = take((int64_t)SK_MAX * (cur + 64));
  const int nblk = cdiv(B, 16);                          // (16-row blocks: the finest partition any step kernel uses)
  h->ws.part_td = take(nblk); h->ws.part_pen = take(nblk);
  {
    // LDS plans of the step kernels: one weight image (qnet_fused_kernel), two (qnet_fused2_kernel<32>), and two at
    // half the rows (qnet_fused2_kernel<16>: same buffers)
    bool ok = (L + 1 <= QF_MAX_LIN);
    for (int l = 0; l <= L + 1 && ok; ++l) ok = m.dims[l] <= QF_MAX_W;
    QnetFusedArgs& fa = h->fargs;
    int off = 0;
    if (ok) {
      fa.n_lin = L + 1;
      for (int l = 0; l <= L + 1; ++l) fa.dims[l] = m.dims[l];
      for (int l = 0; l <= L; ++l) { fa.w_off[l] = m.w[l]; fa.b_off[l] = m.b[l]; }
      const int wmax = qnet_lds_widths(m.dims, L + 1, 0).wmax;
      off = qnet_lds_plan(fa, QF_ROWS);
      ok = off * (int)sizeof(float) <= QF_MAX_LDS_BYTES;
      if (ok && (off + wmax) * (int)sizeof(float) <= QF_MAX_LDS_BYTES) {
        h->fused2_lds_w2 = off;
        h->fused2_lds_bytes = (off + wmax) * (int)sizeof(float);
        h->fargs16 = fa;
        h->fused16_lds_w2 = qnet_lds_plan(h->fargs16, 16);
        h->fused16_lds_bytes = (h->fused16_lds_w2 + wmax) * (int)sizeof(float);
      }
    }
    h->fused_ok = ok;
    h->fused_lds_bytes = off * (int)sizeof(float);
    h->fslab_stride = ru4(cur);
    h->ws.fslab = ok ? take((int64_t)nblk * h->fslab_stride) : 0;
  }
  // appended behind everything older, so every earlier offset keeps its meaning
  h->ws.tmp2[0] = take((int64_t)B * maxld); h->ws.tmp2[1] = take((int64_t)B * maxld);
  h->ws.row_loss = take(B);
  h->ws.mask = take((int64_t)B * c->n_actions);
  h->ws.total = o;
  *out = h;
  return PORL_OK;
}

void porl_qnet_destroy(porl_qnet* h) { delete h; }
int64_t porl_qnet_param_floats(const porl_qnet* h) { return h ? h->n_params : 0; }
int32_t porl_qnet_tensors(const porl_qnet* h) { return h ? (int32_t)h->tensors.size() : 0; }
int porl_qnet_tensor_info(const porl_qnet* h, int index, int64_t* offset, int32_t* rows, int32_t* cols, int32_t* row_stride) {
  if (!h || index < 0 || index >= (int)h->tensors.size()) PORL_FAIL(PORL_ERR_INVALID, "tensor index out of range");
  if (offset) *offset = h->tensors[index].off;
  if (rows) *rows = h->tensors[index].rows;
  if (cols) *cols = h->tensors[index].cols;
  if (row_stride) *row_stride = h->tensors[index].rows ? h->wld[index / 2] : 1;
  return PORL_OK;
}
int64_t porl_qnet_workspace_floats(const porl_qnet* h) { return h ? h->ws.total : 0; }
int32_t porl_qnet_one_launch(const porl_qnet* h) { return h && qnet_is_fused(h) ? 1 : 0; }
int32_t porl_qnet_can_sample(const porl_qnet* h) {
  return h && qnet_is_fused(h) && h->tune.qnet_two_groups && h->fused2_lds_w2 > 0 ? 1 : 0;
}

int porl_qnet_bind(porl_qnet* h, const porl_qnet_buffers* b) {
  if (!h || !b) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  const void* ptrs[] = {b->params, b->params_tgt, b->grads, b->adam_m, b->adam_v, b->workspace, b->stats};
  for (const void* p : ptrs) {
    if (!p) PORL_FAIL(PORL_ERR_INVALID, "null buffer");
    if (!aligned16(p)) PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  }
  h->buf = *b;
  h->bound = true;
  h->device = device_of(b->workspace);
  h->batch = 0;
  h->fslab_clean = false;
  h->slab_clean = false;
  return PORL_OK;
}

static int qnet_ready(const porl_qnet* h, bool need_batch) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_qnet_bind() has not been called");
  if (need_batch && h->batch <= 0) PORL_FAIL(PORL_ERR_INVALID, "no minibatch loaded (porl_qnet_load_batch)");
  return 0;
}

// The argument checks several entry points share.  Each entry point calls them in its own order: which check wins when
// two could fire is part of the ABI.
static int qnet_in_range(const char* what, int v, int hi) {
  if (v < 1 || v > hi) PORL_FAIL(PORL_ERR_INVALID, "%s %d outside [1,%d]", what, v, hi);
  return 0;
}
static int qnet_batch_ok(const porl_qnet* h, int batch) { return qnet_in_range("batch", batch, h->cfg.max_batch); }
static int qnet_n_rows_ok(int64_t n_rows, int batch) {
  if (n_rows < batch || n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "need batch <= n_rows <= 2^40");
  return 0;
}
static int qnet_can_sample_ok(const porl_qnet* h) {
  if (!porl_qnet_can_sample(h)) PORL_FAIL(PORL_ERR_UNSUPPORTED, "in-kernel sampling needs the two-group one-launch step kernel");
  return 0;
}
static int qnet_sampling_ok(const porl_qnet* h, int64_t n_rows, int batch) {
  PORL_TRY(qnet_n_rows_ok(n_rows, batch));
  return qnet_can_sample_ok(h);
}

// one job of pack_kernel: B rows of `cols` floats from src (row stride src_rs) to dst (row stride ld, zero-padded)
static int qnet_copy_rows(const float* src, int64_t src_rs, float* dst, int ld, int cols, int B, hipStream_t s) {
  PackArgs a{};
  a.rows = B; a.njobs = 1;
  a.job[0].src = src; a.job[0].dst = dst; a.job[0].src_row_stride = src_rs; a.job[0].src_col_stride = 1;
  a.job[0].cols = cols; a.job[0].ld = ld;
  const long n = (long)B * ld;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024), 1), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_qnet_load_batch(porl_qnet* h, int32_t batch, const float* states, int64_t s_rs, const int64_t* actions,
                         int64_t a_rs, const float* rewards, int64_t r_rs, const float* next_states, int64_t n_rs,
                         const float* dones, int64_t d_rs, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  PORL_TRY(qnet_batch_ok(h, batch));
  if (!states) PORL_FAIL(PORL_ERR_INVALID, "null states");
  float* W = h->buf.workspace;
  hipStream_t s = (hipStream_t)stream;
  PackArgs a{};
  a.rows = batch;
  auto job = [&](const float* src, int64_t rs, float* dst, int cols, int ld) {
    PackJob& j = a.job[a.njobs++];
    j.src = src; j.dst = dst; j.src_row_stride = rs; j.src_col_stride = 1; j.cols = cols; j.ld = ld;
  };
  job(states, s_rs, W + h->ws.xs, h->cfg.state_dim, h->Sp);
  if (next_states) job(next_states, n_rs, W + h->ws.xn, h->cfg.state_dim, h->Sp);
  if (rewards) job(rewards, r_rs, W + h->ws.rew, 1, 1);
  if (dones) job(dones, d_rs, W + h->ws.done, 1, 1);
  const long n = (long)batch * h->Sp;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024), a.njobs), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  if (actions) {
    hipLaunchKernelGGL(pack_i64_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, s, actions, (long)a_rs, batch,
                       reinterpret_cast<int64_t*>(W + h->ws.actions));
    PORL_HIP(hipGetLastError());
  }
  h->batch = batch;
  return PORL_OK;
}

// forward of `nnets` parameter sets; set k reads input in_k and writes hidden activations to dst_k[l]
// tile_as_alone: choose each layer's tile as a launch of one of the (equally shaped) problems alone would, so that every
// problem of the group runs the tile and K order — hence the bits — of its own single-problem launch
static int qnet_forward(porl_qnet* h, int nnets, const float* const* params, const float* const* inputs,
                        float* const (*dst)[PORL_MAX_HIDDEN + 1], int B, hipStream_t s, bool tile_as_alone = false) {
  const int L = h->cfg.n_hidden;
  for (int l = 0; l <= L; ++l) {
    GemmGroup g{};
    g.nprob = nnets;
    const int K = h->net.dims[l], Nn = h->net.dims[l + 1];
    for (int k = 0; k < nnets; ++k) {
      const float* in = l == 0 ? inputs[k] : dst[k][l - 1];
      const int ldin = l == 0 ? h->Sp : h->ld[l - 1];
      GemmProb p = make_prob(GEMM_NT, in, ldin, params[k] + h->net.w[l], h->wld[l], dst[k][l], h->ld[l], B, Nn, K);
      p.bias = params[k] + h->net.b[l];
      p.act = l < L ? ACT_RELU : ACT_NONE;
      g.p[k] = p;
    }
    int tile;
    if (tile_as_alone) {
      GemmGroup one{};
      one.nprob = 1; one.p[0] = g.p[0];
      tile = pick_tile(one, h->tune);
    } else {
      tile = pick_tile(g, h->tune);
    }
    PORL_TRY(launch_group(g, tile, h->tune, s));
  }
  return PORL_OK;
}

// one network alone on B rows of `input` (row stride Sp): hidden activations kept in ws.act[] for the backward chain
// (keep) or ping-ponged through ws.tmp[]; *out = the output rows (row stride ld[n_hidden])
static int qnet_forward_one(porl_qnet* h, const float* params, const float* input, bool keep, int B, hipStream_t s,
                            float** out) {
  const int L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  float* dst[1][PORL_MAX_HIDDEN + 1];
  for (int l = 0; l <= L; ++l) dst[0][l] = keep ? W + h->ws.act[l] : W + h->ws.tmp[l & 1];
  const float* p[1] = {params};
  const float* in[1] = {input};
  *out = dst[0][L];
  return qnet_forward(h, 1, p, in, dst, B, s);
}

// Where a minibatch comes from: rows idx[b] of the caller's arrays (idx null: rows 0..B-1), or, with samp_n > 0, the rows
// the keyed permutation of [0, samp_n) draws inside the kernel.  Members in the order the entry points take them.
struct QnetRows {
  const float* states; int64_t s_rs;
  const int64_t* actions; const float* rewards;
  const float* next_states; int64_t n_rs;
  const float* dones;
  const int64_t* idx;
  int64_t samp_n; uint64_t samp_seed, samp_step;
};

// the minibatch porl_qnet_load_batch staged in the workspace
static QnetRows qnet_staged_rows(const porl_qnet* h) {
  float* W = h->buf.workspace;
  QnetRows r{};
  r.states = W + h->ws.xs; r.s_rs = h->Sp; r.next_states = W + h->ws.xn; r.n_rs = h->Sp;
  r.actions = reinterpret_cast<const int64_t*>(W + h->ws.actions); r.rewards = W + h->ws.rew; r.dones = W + h->ws.done;
  return r;
}

// rows idx[b] of the caller's arrays — or, with samp_n > 0, the rows the keyed permutation draws — into the staging
// buffers: one launch
static int qnet_gather(porl_qnet* h, const QnetRows& r, int B, hipStream_t s) {
  float* W = h->buf.workspace;
  QnetGatherArgs a{};
  a.states = r.states; a.next_states = r.next_states; a.s_rs = (long)r.s_rs; a.n_rs = (long)r.n_rs;
  a.actions = r.actions; a.rew = r.rewards; a.done = r.dones; a.idx = r.idx;
  a.xs = W + h->ws.xs; a.xn = W + h->ws.xn; a.act_out = reinterpret_cast<int64_t*>(W + h->ws.actions);
  a.rew_out = W + h->ws.rew; a.done_out = W + h->ws.done;
  a.B = B; a.S = h->cfg.state_dim; a.ld = h->Sp;
  if (r.samp_n > 0) {
    a.samp_n = r.samp_n; a.samp_seed = r.samp_seed; a.samp_step = r.samp_step; a.samp_hb = feistel_half_bits(r.samp_n);
    a.idx = nullptr;
  }
  hipLaunchKernelGGL(qnet_gather_kernel, dim3((unsigned)(((long)B * h->Sp + 255) / 256)), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  h->batch = B;
  return PORL_OK;
}

// Adam over the flat parameter group
static int qnet_adam(porl_qnet* h, const porl_qnet_hyper* hp, hipStream_t s) {
  return adam_launch(h->buf.params, h->buf.grads, h->buf.adam_m, h->buf.adam_v, nullptr, h->n_params, hp->lr, hp->step,
                     hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0, s);
}

// gradient of one minibatch in two launches: the fused step kernel (32 or 16 rows per block), then the block-order
// sum of the partial gradients (+ loss statistics, + Adam with with_adam).  `var` may be null (plain CQL / DQN).
static int qnet_fused_backward(porl_qnet* h, const porl_qnet_hyper* hp, int B, const QnetRows& rows,
                               const porl_qnet_variant* var, bool with_adam, hipStream_t s) {
  float* W = h->buf.workspace;
  // 16 rows per block while 32-row blocks would leave CUs idle (config 3 at B = 4096: 128 blocks on 256 CUs)
  const bool two = h->tune.qnet_two_groups && h->fused2_lds_w2 > 0;
  const bool rows16 = two && h->tune.qnet_rows16 && h->fused16_lds_w2 > 0 && cdiv(B, QF_ROWS) < NUM_CU;
  const int nblk = cdiv(B, rows16 ? 16 : QF_ROWS);
  QnetFusedArgs a = rows16 ? h->fargs16 : h->fargs;      // (the same arguments but for the LDS offsets)
  a.params = h->buf.params; a.params_tgt = h->buf.params_tgt;
  a.states = rows.states; a.s_rs = rows.s_rs; a.next_states = rows.next_states; a.n_rs = rows.n_rs;
  a.actions = rows.actions; a.rew = rows.rewards; a.done = rows.dones; a.idx = rows.idx;
  a.slab = W + h->ws.fslab; a.slab_stride = h->fslab_stride;
  a.part_td = W + h->ws.part_td; a.part_pen = W + h->ws.part_pen;
  a.B = B;
  a.gamma = hp->gamma; a.alpha = hp->alpha; a.inv_batch = hp->inv_batch;
  a.log_A = (float)std::log((double)h->cfg.n_actions);
  a.stamps = g_qnet_stamps;
  if (var) {
    a.double_dqn = var->double_dqn; a.is_w = var->is_weights; a.w_uniform = var->uniform_weight; a.td_abs = var->td_abs;
    a.next_mask = var->next_mask; a.td_off = var->td_off;
  }
  a.wgrad_share = h->tune.qnet_wgrad_share;
  // all three step kernels on the first step, whichever runs (dyn_lds_once: hipFuncSetAttribute, once per process)
  PORL_TRY(dyn_lds_once<&qnet_fused_kernel>(QF_MAX_LDS_BYTES));
  PORL_TRY(dyn_lds_once<&qnet_fused2_kernel<32>>(QF_MAX_LDS_BYTES));
  PORL_TRY(dyn_lds_once<&qnet_fused2_kernel<16>>(QF_MAX_LDS_BYTES));
  if (rows.samp_n > 0) {
    if (!two) PORL_FAIL(PORL_ERR_UNSUPPORTED, "in-kernel sampling needs the two-group step kernel");
    a.samp_n = rows.samp_n; a.samp_seed = rows.samp_seed; a.samp_step = rows.samp_step; a.samp_hb = feistel_half_bits(rows.samp_n);
    a.idx = nullptr;
  }
  if (!h->fslab_clean) {
    PORL_HIP(hipMemsetAsync(W + h->ws.fslab, 0, sizeof(float) * cdiv(h->cfg.max_batch, 16) * h->fslab_stride, s));
    h->fslab_clean = true;
  }
  {
    double macs = 0;
    for (int l = 0; l < a.n_lin; ++l) macs += (double)a.dims[l] * a.dims[l + 1];
    ProfScope ps("qnet_fused_kernel", s, 2.0 * B * macs * 4.0, 8.0 * B * a.dims[0]);
    if (rows16)
      hipLaunchKernelGGL(qnet_fused2_kernel<16>, dim3(nblk), dim3(512), (size_t)h->fused16_lds_bytes, s, a, h->fused16_lds_w2);
    else if (two)
      hipLaunchKernelGGL(qnet_fused2_kernel<32>, dim3(nblk), dim3(512), (size_t)h->fused2_lds_bytes, s, a, h->fused2_lds_w2);
    else
      hipLaunchKernelGGL(qnet_fused_kernel, dim3(nblk), dim3(256), (size_t)h->fused_lds_bytes, s, a);
    PORL_HIP(hipGetLastError());
  }
  QnetAdam ad{};
  if (with_adam) {
    if (hp->step < 1) PORL_FAIL(PORL_ERR_INVALID, "adam step must be >= 1");
    // the scalars of adam_launch: python doubles, rounded to fp32 where they meet tensors
    ad.p = h->buf.params; ad.m = h->buf.adam_m; ad.v = h->buf.adam_v;
    ad.omb1 = (float)(1.0 - hp->adam_beta1); ad.beta2 = (float)hp->adam_beta2; ad.omb2 = (float)(1.0 - hp->adam_beta2);
    ad.eps = (float)hp->adam_eps;
    ad.step_size = (float)(hp->lr / (1.0 - std::pow(hp->adam_beta1, (double)hp->step)));
    ad.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(hp->adam_beta2, (double)hp->step));
  }
  ProfScope ps(with_adam ? "qnet_reduce_kernel+adam" : "qnet_reduce_kernel", s, 0.0, 4.0 * nblk * h->n_params);
  hipLaunchKernelGGL(qnet_reduce_kernel, dim3(cdiv((int)h->n_params, 32)), dim3(256), 0, s, W + h->ws.fslab, (long)h->fslab_stride,
                     nblk, (long)h->n_params, h->buf.grads, W + h->ws.part_td, W + h->ws.part_pen, hp->inv_batch, hp->alpha,
                     h->buf.stats, ad);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// backward of the multi-launch path from dL/d(output) `dz` (B, ld[L]): dW_l = dZ_l^T In_l (split over the batch),
// dZ_{l-1} = (dZ_l W_l) . 1[In_l > 0], top down; needs the online forward's activations in ws.act[] and the batch in ws.xs
static int qnet_backward_chain(porl_qnet* h, float* dz, int B, hipStream_t s) {
  const int L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  float* G = h->buf.grads;
  ReduceArgs red{};
  float* slab = W + h->ws.slab;
  for (int l = L; l >= 0; --l) {
    const int out_d = h->net.dims[l + 1], in_d = h->net.dims[l];
    const float* in = l == 0 ? W + h->ws.xs : W + h->ws.act[l - 1];
    const int ldin = l == 0 ? h->Sp : h->ld[l - 1];
    GemmGroup g{};
    g.p[g.nprob] = make_prob(GEMM_TN, dz, h->ld[l], in, ldin, G + h->net.w[l], h->wld[l], out_d, in_d, B);
    g.p[g.nprob].colsum = G + h->net.b[l];
    GemmProb& wg = g.p[g.nprob++];
    float* dz_next = nullptr;
    if (l > 0) {
      dz_next = W + h->ws.dz[(l - 1) & 1];
      GemmProb q = make_prob(GEMM_NN, dz, h->ld[l], h->buf.params + h->net.w[l], h->wld[l], dz_next, h->ld[l - 1], B, in_d, out_d);
      q.mask = in; q.ldmask = ldin;
      g.p[g.nprob++] = q;
    }
    const int tile = TILE_64x64;
    const int sk = pick_splitk(out_d, in_d, B, 1, 64, 64);
    if (sk > 1) {
      const int64_t per = (int64_t)out_d * h->wld[l];          // slabs have the padded row stride of the gradient image
      if (!h->slab_clean) {                                    // their padding columns are never written: zero them once
        PORL_HIP(hipMemsetAsync(W + h->ws.slab, 0, sizeof(float) * (size_t)SK_MAX * (h->n_params + 64), s));
        h->slab_clean = true;
      }
      if (red.njobs + 2 > 8) { PORL_TRY(launch_reduce(red, s)); red = ReduceArgs{}; }
      float* slabW = slab; slab += (int64_t)sk * per;
      float* slabC = slab; slab += (int64_t)sk * out_d;
      wg.splitk = sk; wg.C = slabW; wg.colsum = slabC;
      add_reduce(red, G + h->net.w[l], slabW, per, per, sk);
      add_reduce(red, G + h->net.b[l], slabC, out_d, out_d, sk);
    }
    PORL_TRY(launch_group(g, tile, h->tune, s));
    if (red.njobs == 8 || l == 0) { PORL_TRY(launch_reduce(red, s)); red = ReduceArgs{}; }
    dz = dz_next;
  }
  return PORL_OK;
}

// Multi-launch gradient of the loaded minibatch (any layer widths): forwards through the grouped GEMM, loss head with
// the optional DQN variants, backward chain.  `var` may be null (plain CQL / DQN).
static int qnet_general_backward(porl_qnet* h, const porl_qnet_hyper* hp, const porl_qnet_variant* var, hipStream_t s) {
  const int B = h->batch, L = h->cfg.n_hidden, A = h->cfg.n_actions;
  float* W = h->buf.workspace;
  // forward: target net on s' (activations ping-pong in tmp), online net on s (activations kept)
  float* dst[2][PORL_MAX_HIDDEN + 1];
  for (int l = 0; l <= L; ++l) { dst[0][l] = W + h->ws.tmp[l & 1]; dst[1][l] = W + h->ws.act[l]; }
  const float* params[2] = {h->buf.params_tgt, h->buf.params};
  const float* inputs[2] = {W + h->ws.xn, W + h->ws.xs};
  PORL_TRY(qnet_forward(h, 2, params, inputs, dst, B, s));
  float* Qn = dst[0][L];
  float* Q = dst[1][L];
  float* dz = W + h->ws.dz[L & 1];
  const float* Qon = nullptr;
  if (var && var->double_dqn) {
    // Double DQN: the online network on s' as well; its activations ping-pong through the two dZ buffers (free until the
    // loss head writes dL/dQ), so Q_online(s') ends in the buffer dL/dQ goes to — a row is read before it is written
    float* dst2[1][PORL_MAX_HIDDEN + 1];
    for (int l = 0; l <= L; ++l) dst2[0][l] = W + h->ws.dz[l & 1];
    const float* p2[1] = {h->buf.params};
    const float* in2[1] = {W + h->ws.xn};
    PORL_TRY(qnet_forward(h, 1, p2, in2, dst2, B, s));
    Qon = dst2[0][L];
  }
  const int nblk = cdiv(B, 256);
  {
    CqlLossArgs a{};
    a.Qon = Qon;
    if (var) { a.is_w = var->is_weights; a.w_uniform = var->uniform_weight; a.td_abs = var->td_abs; a.next_mask = var->next_mask; a.td_off = var->td_off; }
    a.Q = Q; a.Qn = Qn; a.ldq = h->ld[L];
    a.actions = reinterpret_cast<const int64_t*>(W + h->ws.actions); a.rew = W + h->ws.rew; a.done = W + h->ws.done;
    a.dQ = dz; a.part_td = W + h->ws.part_td; a.part_pen = W + h->ws.part_pen;
    a.B = B; a.A = A; a.gamma = hp->gamma; a.alpha = hp->alpha; a.inv_batch = hp->inv_batch;
    a.log_A = (float)std::log((double)A);
    hipLaunchKernelGGL(cql_loss_kernel, dim3(nblk), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
    hipLaunchKernelGGL(cql_finalize_kernel, dim3(1), dim3(64), 0, s, W + h->ws.part_td, W + h->ws.part_pen, nblk,
                       hp->inv_batch, hp->alpha, h->buf.stats);
    PORL_HIP(hipGetLastError());
  }
  return qnet_backward_chain(h, dz, B, s);
}

int porl_qnet_cql_backward(porl_qnet* h, const porl_qnet_hyper* hp, void* stream) {
  PORL_TRY(qnet_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  hipStream_t s = (hipStream_t)stream;
  if (qnet_is_fused(h)) return qnet_fused_backward(h, hp, h->batch, qnet_staged_rows(h), nullptr, false, s);
  return qnet_general_backward(h, hp, nullptr, s);      // (the batch is staged already: no gather)
}

// ---- general forward / backward pieces for losses computed outside the engine (QR-DQN, C51: dist_losses.hpp) ----------
// Forward of the online (which_params = 0) or target (1) network on the LOADED batch's states (which_input = 0) or
// next states (1); out (batch, n_outputs) with row stride out_rs.  keep != 0 stores the hidden activations for
// porl_qnet_backward (online network on the states only).
int porl_qnet_forward_loaded(porl_qnet* h, int which_params, int which_input, int keep, float* out, int64_t out_rs,
                             void* stream) {
  PORL_TRY(qnet_ready(h, true)); DevGuard _dg(h->device);
  if (!out || out_rs < h->cfg.n_actions) PORL_FAIL(PORL_ERR_INVALID, "bad output");
  if (keep && (which_params != 0 || which_input != 0)) PORL_FAIL(PORL_ERR_INVALID, "keep: online network on the states only");
  hipStream_t s = (hipStream_t)stream;
  float* W = h->buf.workspace;
  float* q = nullptr;
  PORL_TRY(qnet_forward_one(h, which_params ? h->buf.params_tgt : h->buf.params, W + (which_input ? h->ws.xn : h->ws.xs),
                            keep != 0, h->batch, s, &q));
  return qnet_copy_rows(q, h->ld[h->cfg.n_hidden], out, (int)out_rs, h->cfg.n_actions, h->batch, s);
}

// Backward from dL/d(output) `dout` (batch, n_outputs; row stride dout_rs) through the online network whose forward was
// kept by porl_qnet_forward_loaded: leaves the gradient in grads (complete: slabs combined); porl_qnet_apply follows.
int porl_qnet_backward(porl_qnet* h, const float* dout, int64_t dout_rs, void* stream) {
  PORL_TRY(qnet_ready(h, true)); DevGuard _dg(h->device);
  if (!dout || dout_rs < h->cfg.n_actions) PORL_FAIL(PORL_ERR_INVALID, "bad gradient input");
  hipStream_t s = (hipStream_t)stream;
  const int L = h->cfg.n_hidden, B = h->batch;
  float* W = h->buf.workspace;
  float* dz = W + h->ws.dz[L & 1];
  PORL_TRY(qnet_copy_rows(dout, dout_rs, dz, h->ld[L], h->cfg.n_actions, B, s));
  return qnet_backward_chain(h, dz, B, s);
}

static int dist_args_ok(int B, int A, int N, int64_t ld) {
  if (B < 1 || A < 1 || N < 1 || N > DIST_MAX_N || ld < (int64_t)A * N) PORL_FAIL(PORL_ERR_INVALID, "bad distributional-loss shapes (N <= %d)", DIST_MAX_N);
  return 0;
}

int porl_qr_loss(const float* z_cur, const float* z_next_online, const float* z_next_target, int64_t ld, const int64_t* actions,
                 const float* rewards, const float* dones, int32_t batch, int32_t n_actions, int32_t n_quantiles, float gamma,
                 float kappa, float* dz_out, float* row_loss, void* stream) {
  if (!z_cur || !z_next_online || !z_next_target || !actions || !rewards || !dones || !dz_out || !row_loss)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(dist_args_ok(batch, n_actions, n_quantiles, ld));
  DevGuard _dg(device_of(dz_out));
  QrLossArgs a{z_cur, z_next_online, z_next_target, (long)ld, actions, rewards, dones, dz_out, row_loss, batch, n_actions,
               n_quantiles, gamma, kappa, 1.0f / batch};
  hipLaunchKernelGGL(qr_loss_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_quantile_huber(const float* current, const float* target, const float* taus, int32_t batch, int32_t n_current,
                            int32_t n_target, float kappa, float* dcurrent_out, float* row_loss, void* stream) {
  if (!current || !target || !taus || !dcurrent_out || !row_loss || batch < 1 || n_current < 1 || n_target < 1)
    PORL_FAIL(PORL_ERR_INVALID, "bad arguments");
  DevGuard _dg(device_of(dcurrent_out));
  IqnLossArgs a{current, target, taus, dcurrent_out, row_loss, batch, n_current, n_target, kappa, 1.0f / batch};
  hipLaunchKernelGGL(iqn_loss_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

namespace {
inline unsigned iqn_blocks(long items) { return (unsigned)std::min<long>(std::max<long>((items + 255) / 256, 1), 256L * 16); }
inline int iqn_dims_ok(int32_t batch, int32_t n_tau, int32_t third) {
  if (batch < 1 || n_tau < 1 || third < 1) PORL_FAIL(PORL_ERR_INVALID, "batch %d, n_tau %d, width/actions %d must be >= 1", batch, n_tau, third);
  if ((int64_t)batch * n_tau * third > (int64_t)1 << 40) PORL_FAIL(PORL_ERR_INVALID, "tensor too large");
  return PORL_OK;
}
}  // namespace

int porl_iqn_cos_embed(const float* taus, int64_t n, int32_t embedding_dim, float* out, void* stream) {
  if (!taus || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (n < 1 || embedding_dim < 1 || n > ((int64_t)1 << 40) / embedding_dim) PORL_FAIL(PORL_ERR_INVALID, "n %lld, embedding_dim %d", (long long)n, embedding_dim);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(iqn_cos_embed_kernel, dim3(iqn_blocks(n * embedding_dim)), dim3(256), 0, (hipStream_t)stream, taus, (long)n,
                     embedding_dim, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_hadamard(const float* feat, int64_t ldf, const float* emb, int32_t batch, int32_t n_tau, int32_t width,
                      float* out, void* stream) {
  if (!feat || !emb || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(iqn_dims_ok(batch, n_tau, width));
  if (ldf < width) PORL_FAIL(PORL_ERR_INVALID, "feature row stride %lld < width %d", (long long)ldf, width);
  const bool al = !((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(out)) & 15u);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(iqn_hadamard_kernel, dim3(iqn_blocks((long)batch * n_tau * width / 4)), dim3(256), 0, (hipStream_t)stream,
                     feat, (long)ldf, emb, batch, n_tau, width, out, al ? 1 : 0);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_hadamard_backward(const float* dout, const float* feat, int64_t ldf, const float* emb, int32_t batch,
                               int32_t n_tau, int32_t width, float* dfeat, float* demb, void* stream) {
  if (!dout || !feat || !emb || (!dfeat && !demb)) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(iqn_dims_ok(batch, n_tau, width));
  if (ldf < width) PORL_FAIL(PORL_ERR_INVALID, "feature row stride %lld < width %d", (long long)ldf, width);
  DevGuard _dg(device_of(dout));
  hipLaunchKernelGGL(iqn_hadamard_bwd_kernel, dim3(iqn_blocks((long)batch * width)), dim3(256), 0, (hipStream_t)stream, dout,
                     feat, (long)ldf, emb, batch, n_tau, width, dfeat, demb);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_select(const float* z, const int64_t* actions, int32_t batch, int32_t n_tau, int32_t n_actions, float* out,
                    void* stream) {
  if (!z || !actions || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(iqn_dims_ok(batch, n_tau, n_actions));
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(iqn_select_kernel, dim3(iqn_blocks((long)batch * n_tau)), dim3(256), 0, (hipStream_t)stream, z, actions,
                     batch, n_tau, n_actions, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_scatter(const float* dsel, const int64_t* actions, int32_t batch, int32_t n_tau, int32_t n_actions, float* dz,
                     void* stream) {
  if (!dsel || !actions || !dz) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(iqn_dims_ok(batch, n_tau, n_actions));
  DevGuard _dg(device_of(dz));
  hipLaunchKernelGGL(iqn_scatter_kernel, dim3(iqn_blocks((long)batch * n_tau * n_actions)), dim3(256), 0, (hipStream_t)stream,
                     dsel, actions, batch, n_tau, n_actions, dz);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iqn_target(const float* z_online_next, const float* z_target_next, const float* rewards, const float* dones,
                    float gamma, int32_t batch, int32_t n_tau, int32_t n_actions, float* td, int64_t* next_actions,
                    void* stream) {
  if (!z_online_next || !z_target_next || !rewards || !dones || !td) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(iqn_dims_ok(batch, n_tau, n_actions));
  DevGuard _dg(device_of(td));
  hipLaunchKernelGGL(iqn_target_kernel, dim3(iqn_blocks(batch)), dim3(256), 0, (hipStream_t)stream, z_online_next,
                     z_target_next, rewards, dones, gamma, batch, n_tau, n_actions, td, next_actions);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_grad_clip(float* grads, int64_t n, float max_norm, float* norm_coef, double* workspace, void* stream) {
  if (!grads || !norm_coef || !workspace) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (n < 0 || n > (int64_t)1 << 40) PORL_FAIL(PORL_ERR_INVALID, "n = %lld", (long long)n);
  if (!(max_norm > 0.f)) PORL_FAIL(PORL_ERR_INVALID, "max_norm must be positive");
  DevGuard _dg(device_of(grads));
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)std::min<long>(CLIP_BLOCKS, std::max<long>(1, (n + 4095) / 4096));
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, grads, (long)n, workspace);
  PORL_HIP(hipGetLastError());
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, s, workspace, nb, max_norm, norm_coef);
  PORL_HIP(hipGetLastError());
  if (n > 0) {
    hipLaunchKernelGGL(scale_by_kernel, dim3(iqn_blocks(n)), dim3(256), 0, s, grads, (long)n, norm_coef);
    PORL_HIP(hipGetLastError());
  }
  return PORL_OK;
}

int porl_c51_loss(const float* logits_cur, const float* logits_next_target, int64_t ld, const int64_t* actions,
                  const float* rewards, const float* dones, const float* support, int32_t batch, int32_t n_actions,
                  int32_t n_atoms, float gamma, float v_min, float v_max, float* dlogits_out, float* row_loss, void* stream) {
  if (!logits_cur || !logits_next_target || !actions || !rewards || !dones || !support || !dlogits_out || !row_loss)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(dist_args_ok(batch, n_actions, n_atoms, ld));
  if (n_atoms < 2 || !(v_max > v_min)) PORL_FAIL(PORL_ERR_INVALID, "need n_atoms >= 2 and v_max > v_min");
  DevGuard _dg(device_of(dlogits_out));
  // delta_z as the reference forms it (python double (v_max - v_min) / (atom_size - 1), meeting fp32 tensors as fp32)
  const float delta = (float)(((double)v_max - (double)v_min) / (double)(n_atoms - 1));
  C51LossArgs a{logits_cur, logits_next_target, (long)ld, actions, rewards, dones, support, dlogits_out, row_loss, batch, n_actions,
                n_atoms, gamma, v_min, v_max, delta, 1.0f / batch};
  hipLaunchKernelGGL(c51_loss_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_qnet_apply(porl_qnet* h, const porl_qnet_hyper* hp, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  return qnet_adam(h, hp, (hipStream_t)stream);
}

int porl_qnet_learn(porl_qnet* h, const porl_qnet_hyper* hp, void* stream) {
  PORL_TRY(qnet_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  hipStream_t s = (hipStream_t)stream;
  if (qnet_is_fused(h)) return qnet_fused_backward(h, hp, h->batch, qnet_staged_rows(h), nullptr, true, s);
  PORL_TRY(qnet_general_backward(h, hp, nullptr, s));      // (the batch is staged already: no gather)
  return qnet_adam(h, hp, s);
}

// learn() on rows idx[b] of the replay arrays for networks the one-launch kernel does not cover: gather into the staging
// buffers (one launch), multi-launch gradient with the variant's loss head, Adam.  Same arithmetic per element as the
// one-launch kernel's loss stage; sums run in the grouped GEMM's order instead of per 32-row block.
static int qnet_general_learn(porl_qnet* h, const porl_qnet_hyper* hp, int B, const QnetRows& rows,
                              const porl_qnet_variant* var, hipStream_t s) {
  PORL_TRY(qnet_gather(h, rows, B, s));
  PORL_TRY(qnet_general_backward(h, hp, var, s));
  return qnet_adam(h, hp, s);
}

// One learn step on `rows` with the loss variant `var` (null: plain CQL / DQN): the one-launch kernel where it covers the
// network, else the multi-launch path (a layer > 128 wide, > 5 Linear layers, or switched off by porl_tune_set)
static int qnet_learn_rows(porl_qnet* h, const porl_qnet_hyper* hp, int B, const QnetRows& rows,
                           const porl_qnet_variant* var, hipStream_t s) {
  if (!qnet_is_fused(h)) return qnet_general_learn(h, hp, B, rows, var, s);
  return qnet_fused_backward(h, hp, B, rows, var, true, s);
}

int porl_qnet_learn_variant(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                            const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                            const porl_qnet_hyper* hp, const porl_qnet_variant* variant, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!hp || !states || !actions || !rewards || !next_states || !dones || !variant) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(qnet_batch_ok(h, batch));
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, idx};
  return qnet_learn_rows(h, hp, batch, rows, variant, (hipStream_t)stream);
}

int porl_qnet_learn_indexed(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                            const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                            const porl_qnet_hyper* hp, void* stream) {
  static const porl_qnet_variant plain{};      // every variant off: what both paths do without one
  return porl_qnet_learn_variant(h, states, s_rs, actions, rewards, next_states, n_rs, dones, idx, batch, hp, &plain, stream);
}

int porl_qnet_learn_sampled(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                            const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, uint64_t seed,
                            uint64_t draw, int32_t batch, const porl_qnet_hyper* hp, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!hp || !states || !actions || !rewards || !next_states || !dones) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(qnet_batch_ok(h, batch));
  PORL_TRY(qnet_sampling_ok(h, n_rows, batch));
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, nullptr, n_rows, seed, draw};
  return qnet_learn_rows(h, hp, batch, rows, nullptr, (hipStream_t)stream);
}

int porl_qnet_learn_sampled_variant(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                                    const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, uint64_t seed,
                                    uint64_t draw, int32_t batch, const porl_qnet_hyper* hp, const porl_qnet_variant* variant,
                                    void* stream) {
  // (the argument checks come before the bound check here, unlike in the entry points above)
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!hp || !states || !actions || !rewards || !next_states || !dones || !variant) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(qnet_batch_ok(h, batch));
  PORL_TRY(qnet_n_rows_ok(n_rows, batch));
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  PORL_TRY(qnet_can_sample_ok(h));
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, nullptr, n_rows, seed, draw};
  return qnet_learn_rows(h, hp, batch, rows, variant, (hipStream_t)stream);
}

// ---- discrete BCQ from one call (csrc/bcq_mask.hpp) -------------------------------------------------------------------
// mask[b, :] of the behaviour engine `beh` on `rows` (of which next_states, n_rs, idx and samp_* are read).  One launch
// when beh's network fits one block's LDS (beh->fused_ok), else [sampler,] gather, one launch per layer and
// softmax_mask_kernel — the launches of BehaviorPolicy.sample on the gathered rows, the same numbers.
static int bcq_mask_launch(porl_qnet* beh, const QnetRows& rows, int B, float threshold, float* mask_out, hipStream_t s) {
  const int L = beh->cfg.n_hidden, A = beh->cfg.n_actions, S = beh->cfg.state_dim;
  const bool sampled = rows.samp_n > 0;
  const int64_t* idx = rows.idx;
  if (qnet_is_fused(beh)) {
    BcqMaskArgs a{};
    a.params = beh->buf.params; a.next_states = rows.next_states; a.n_rs = (long)rows.n_rs; a.idx = sampled ? nullptr : idx;
    a.mask = mask_out; a.B = B; a.n_lin = L + 1; a.threshold = threshold;
    for (int l = 0; l <= L + 1; ++l) a.dims[l] = beh->net.dims[l];
    for (int l = 0; l <= L; ++l) a.w_off[l] = beh->net.w[l];
    // the step kernel's plan (qnet_lds_plan) without the per-layer activations: the row indices, the input rows, two
    // ping-pong buffers of the widest layer behind the input, one weight image
    const QnetLdsWidths w = qnet_lds_widths(a.dims, L + 1, 1);
    int off = 0;
    a.lds_rows = off; off += 2 * QF_ROWS;
    a.lds_x = off; off += QF_ROWS * (((S + 31) & ~31) + 4);
    a.lds_act[0] = off; off += QF_ROWS * (w.maxw + 4);
    a.lds_act[1] = off; off += QF_ROWS * (w.maxw + 4);
    a.lds_w = off; off += w.wmax;
    const int lds_bytes = off * (int)sizeof(float);     // below the step kernel's own plan, which fused_ok vouches for
    if (lds_bytes > QF_MAX_LDS_BYTES) PORL_FAIL(PORL_ERR_UNSUPPORTED, "behaviour network needs %d bytes of LDS", lds_bytes);
    if (sampled) { a.samp_n = rows.samp_n; a.samp_seed = rows.samp_seed; a.samp_step = rows.samp_step; a.samp_hb = feistel_half_bits(rows.samp_n); }
    PORL_TRY(dyn_lds_once<&bcq_mask_kernel>(QF_MAX_LDS_BYTES));
    double macs = 0;
    for (int l = 0; l <= L; ++l) macs += (double)a.dims[l] * a.dims[l + 1];
    ProfScope ps("bcq_mask_kernel", s, 2.0 * B * macs, 4.0 * B * (S + A));
    hipLaunchKernelGGL(bcq_mask_kernel, dim3(cdiv(B, QF_ROWS)), dim3(256), (size_t)lds_bytes, s, a);
    PORL_HIP(hipGetLastError());
    return PORL_OK;
  }
  float* W = beh->buf.workspace;
  if (sampled) {
    int64_t* drawn = reinterpret_cast<int64_t*>(W + beh->ws.actions);       // (max_batch) int64 of staging space
    hipLaunchKernelGGL(sample_indices_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, rows.samp_n, B, rows.samp_seed, rows.samp_step,
                       feistel_half_bits(rows.samp_n), (int64_t)0, (int64_t)0, drawn);
    PORL_HIP(hipGetLastError());
    idx = drawn;
  }
  hipLaunchKernelGGL(bcq_gather_kernel, dim3((unsigned)(((long)B * beh->Sp + 255) / 256)), dim3(256), 0, s, rows.next_states,
                     (long)rows.n_rs, idx, W + beh->ws.xs, B, S, beh->Sp);
  PORL_HIP(hipGetLastError());
  beh->batch = 0;
  float* logits = nullptr;
  PORL_TRY(qnet_forward_one(beh, beh->buf.params, W + beh->ws.xs, false, B, s, &logits));
  hipLaunchKernelGGL(softmax_mask_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, logits, (long)beh->ld[L], B, A, threshold, 0,
                     mask_out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_qnet_bcq_mask(porl_qnet* beh, const float* next_states, int64_t n_rs, const int64_t* idx, int32_t batch,
                       float threshold, float* mask_out, void* stream) {
  if (!beh) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!next_states || !idx || !mask_out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(qnet_batch_ok(beh, batch));
  if (n_rs < beh->cfg.state_dim) PORL_FAIL(PORL_ERR_INVALID, "row stride below state_dim %d", beh->cfg.state_dim);
  if (!std::isfinite(threshold)) PORL_FAIL(PORL_ERR_INVALID, "threshold is not finite");
  PORL_TRY(qnet_ready(beh, false)); DevGuard _dg(beh->device);
  QnetRows rows{};
  rows.next_states = next_states; rows.n_rs = n_rs; rows.idx = idx;
  return bcq_mask_launch(beh, rows, batch, threshold, mask_out, (hipStream_t)stream);
}

static int bcq_learn_check(const porl_qnet* h, const porl_qnet* beh, const void* const* ptrs, int nptrs, int32_t batch,
                           int64_t s_rs, int64_t n_rs, float threshold) {
  if (!h || !beh) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  for (int i = 0; i < nptrs; ++i)
    if (!ptrs[i]) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  const int mb = std::min(h->cfg.max_batch, beh->cfg.max_batch);
  PORL_TRY(qnet_in_range("batch", batch, mb));
  if (beh->cfg.state_dim != h->cfg.state_dim || beh->cfg.n_actions != h->cfg.n_actions)
    PORL_FAIL(PORL_ERR_INVALID, "behaviour network (%d -> %d) does not match the Q network (%d -> %d)", beh->cfg.state_dim,
              beh->cfg.n_actions, h->cfg.state_dim, h->cfg.n_actions);
  if (s_rs < h->cfg.state_dim || n_rs < h->cfg.state_dim) PORL_FAIL(PORL_ERR_INVALID, "row stride below state_dim %d", h->cfg.state_dim);
  if (!std::isfinite(threshold)) PORL_FAIL(PORL_ERR_INVALID, "threshold is not finite");
  PORL_TRY(qnet_ready(h, false));
  PORL_TRY(qnet_ready(beh, false));
  if (beh->device != h->device) PORL_FAIL(PORL_ERR_INVALID, "the two engines live on different devices");
  return PORL_OK;
}

// mask kernel into the (max_batch, A) region at the end of h's workspace, then the learn step with it as next_mask
static int bcq_learn_rows(porl_qnet* h, porl_qnet* beh, const porl_qnet_hyper* hp, int B, const QnetRows& rows,
                          float threshold, hipStream_t s) {
  float* mask = h->buf.workspace + h->ws.mask;
  PORL_TRY(bcq_mask_launch(beh, rows, B, threshold, mask, s));
  porl_qnet_variant var{};
  var.next_mask = mask;
  return qnet_learn_rows(h, hp, B, rows, &var, s);
}

int porl_qnet_bcq_learn(porl_qnet* h, porl_qnet* beh, const float* states, int64_t s_rs, const int64_t* actions,
                        const float* rewards, const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx,
                        int32_t batch, const porl_qnet_hyper* hp, float threshold, void* stream) {
  const void* ptrs[] = {states, actions, rewards, next_states, dones, idx, hp};
  PORL_TRY(bcq_learn_check(h, beh, ptrs, 7, batch, s_rs, n_rs, threshold));
  DevGuard _dg(h->device);
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, idx};
  return bcq_learn_rows(h, beh, hp, batch, rows, threshold, (hipStream_t)stream);
}

int porl_qnet_bcq_learn_sampled(porl_qnet* h, porl_qnet* beh, const float* states, int64_t s_rs, const int64_t* actions,
                                const float* rewards, const float* next_states, int64_t n_rs, const float* dones,
                                int64_t n_rows, uint64_t seed, uint64_t draw, int32_t batch, const porl_qnet_hyper* hp,
                                float threshold, void* stream) {
  const void* ptrs[] = {states, actions, rewards, next_states, dones, hp};
  PORL_TRY(bcq_learn_check(h, beh, ptrs, 6, batch, s_rs, n_rs, threshold));
  PORL_TRY(qnet_sampling_ok(h, n_rows, batch));
  DevGuard _dg(h->device);
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, nullptr, n_rows, seed, draw};
  return bcq_learn_rows(h, beh, hp, batch, rows, threshold, (hipStream_t)stream);
}

// ---- one learn step of the distributional trainers from one call (QR-DQN, C51: dist_losses.hpp) -------------------------
// The launches of porl_qnet_load_batch + porl_qnet_forward_loaded (x2 / x3) + porl_qr_loss / porl_c51_loss + porl_qnet_backward +
// porl_qnet_apply + porl_reduce_mean without the copies between them: one gather, the forwards grouped per layer, the loss
// head reading the padded output rows and writing dL/dz where the backward chain reads it (the head zero-fills columns
// A*N .. ld-1, as pack_kernel did), the mean into stats[0].  Same kernels on the same numbers: bit-equal results.
// The head rules porl_qnet_dist_learn and the acting entry points share; n_out: the network's outputs (< 0: no network)
static int dist_head_ok(const porl_dist_head* head, int64_t n_out) {
  if (head->kind != PORL_DIST_QR && head->kind != PORL_DIST_C51) PORL_FAIL(PORL_ERR_INVALID, "unknown head kind %d", head->kind);
  PORL_TRY(qnet_in_range("n_sub", head->n_sub, DIST_MAX_N));
  if (n_out >= 0 && (head->n_actions < 1 || (int64_t)head->n_actions * head->n_sub != n_out))
    PORL_FAIL(PORL_ERR_INVALID, "n_actions %d x n_sub %d != the network's %d outputs", head->n_actions, head->n_sub, (int)n_out);
  if (head->kind == PORL_DIST_C51) {
    if (head->n_sub < 2 || !(head->v_max > head->v_min)) PORL_FAIL(PORL_ERR_INVALID, "C51 needs n_sub >= 2 and v_max > v_min");
    if (!head->support) PORL_FAIL(PORL_ERR_INVALID, "C51 needs the support (null)");
  }
  return PORL_OK;
}

// the step on `rows` (idx, or with sampled the keyed draw of rows.samp_n rows inside the gather launch)
static int qnet_dist_learn_rows(porl_qnet* h, const QnetRows& rows, bool sampled, int32_t batch, const porl_qnet_hyper* hp,
                                const porl_dist_head* head, void* stream) {
  PORL_TRY(qnet_ready(h, false));
  if (!hp || !head || !rows.states || !rows.actions || !rows.rewards || !rows.next_states || !rows.dones)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  PORL_TRY(qnet_batch_ok(h, batch));
  if (sampled) PORL_TRY(qnet_n_rows_ok(rows.samp_n, batch));
  if (rows.s_rs < h->cfg.state_dim || rows.n_rs < h->cfg.state_dim) PORL_FAIL(PORL_ERR_INVALID, "row stride below state_dim %d", h->cfg.state_dim);
  PORL_TRY(dist_head_ok(head, h->cfg.n_actions));
  if (hp->step < 1) PORL_FAIL(PORL_ERR_INVALID, "adam step must be >= 1");
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  float* W = h->buf.workspace;
  const int L = h->cfg.n_hidden, B = batch, A = head->n_actions, N = head->n_sub;
  const bool qr = head->kind == PORL_DIST_QR;
  PORL_TRY(qnet_gather(h, rows, B, s));
  // online net on s (kept), target net on s', QR-DQN: online net on s' — one launch per layer
  float* dst[3][PORL_MAX_HIDDEN + 1];
  for (int l = 0; l <= L; ++l) { dst[0][l] = W + h->ws.act[l]; dst[1][l] = W + h->ws.tmp[l & 1]; dst[2][l] = W + h->ws.tmp2[l & 1]; }
  const float* params[3] = {h->buf.params, h->buf.params_tgt, h->buf.params};
  const float* inputs[3] = {W + h->ws.xs, W + h->ws.xn, W + h->ws.xn};
  PORL_TRY(qnet_forward(h, qr ? 3 : 2, params, inputs, dst, B, s, true));
  float* dz = W + h->ws.dz[L & 1];
  float* row_loss = W + h->ws.row_loss;
  const int64_t* act = reinterpret_cast<const int64_t*>(W + h->ws.actions);
  if (qr) {
    QrLossArgs a{dst[0][L], dst[2][L], dst[1][L], (long)h->ld[L], act, W + h->ws.rew, W + h->ws.done, dz, row_loss, B, A, N,
                 hp->gamma, head->kappa, 1.0f / B};
    hipLaunchKernelGGL(qr_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, a);
  } else {
    const float delta = (float)(((double)head->v_max - (double)head->v_min) / (double)(N - 1));      // as porl_c51_loss
    C51LossArgs a{dst[0][L], dst[1][L], (long)h->ld[L], act, W + h->ws.rew, W + h->ws.done, head->support, dz, row_loss, B, A, N,
                  hp->gamma, head->v_min, head->v_max, delta, 1.0f / B};
    hipLaunchKernelGGL(c51_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, a);
  }
  PORL_HIP(hipGetLastError());
  {
    ReduceArgs r{};
    add_reduce(r, h->buf.stats, row_loss, 1, 1, B, 0, 1.0f / B);       // porl_reduce_mean's job
    PORL_TRY(launch_reduce(r, s));
  }
  PORL_TRY(qnet_backward_chain(h, dz, B, s));
  return qnet_adam(h, hp, s);
}

int porl_qnet_dist_learn(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                         const float* next_states, int64_t n_rs, const float* dones, const int64_t* idx, int32_t batch,
                         const porl_qnet_hyper* hp, const porl_dist_head* head, void* stream) {
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, idx};
  return qnet_dist_learn_rows(h, rows, false, batch, hp, head, stream);
}

// porl_qnet_dist_learn on the rows feistel_index(n_rows, b, seed, draw, hb) gives — porl_sample_indices' rows — drawn inside
// the gather launch: no index tensor, no extra launch
int porl_qnet_dist_learn_sampled(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, const float* rewards,
                                 const float* next_states, int64_t n_rs, const float* dones, int64_t n_rows, uint64_t seed,
                                 uint64_t draw, int32_t batch, const porl_qnet_hyper* hp, const porl_dist_head* head,
                                 void* stream) {
  const QnetRows rows{states, s_rs, actions, rewards, next_states, n_rs, dones, nullptr, n_rows, seed, draw};
  return qnet_dist_learn_rows(h, rows, true, batch, hp, head, stream);
}

int porl_qnet_sync_target(porl_qnet* h, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  PORL_HIP(hipMemcpyAsync(h->buf.params_tgt, h->buf.params, sizeof(float) * h->n_params, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  return PORL_OK;
}

// Q(s, .) for a loaded batch of states (which = 0 online, 1 target) -> q_out (batch, n_actions), row stride q_rs
int porl_qnet_forward(porl_qnet* h, int which, const float* states, int64_t s_rs, int32_t batch, float* q_out,
                      int64_t q_rs, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!q_out) PORL_FAIL(PORL_ERR_INVALID, "null output");
  hipStream_t s = (hipStream_t)stream;
  PORL_TRY(porl_qnet_load_batch(h, batch, states, s_rs, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, stream));
  h->batch = 0;
  float* q = nullptr;
  PORL_TRY(qnet_forward_one(h, which ? h->buf.params_tgt : h->buf.params, h->buf.workspace + h->ws.xs, false, batch, s, &q));
  // (checked only here, behind the forward's launches: callers may rely on the order of these side effects)
  if (q_rs < h->cfg.n_actions) PORL_FAIL(PORL_ERR_INVALID, "q_rs smaller than n_actions");
  return qnet_copy_rows(q, h->ld[h->cfg.n_hidden], q_out, (int)q_rs, h->cfg.n_actions, batch, s);
}

// mean_b( logsumexp_a Q(s_b, a) - ln A - Q(s_b, a_b) ) -> out[0]   (compute_cql_penalty)
int porl_qnet_penalty(porl_qnet* h, const float* states, int64_t s_rs, const int64_t* actions, int64_t a_rs,
                      int32_t batch, float* out, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!out || !actions) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  hipStream_t s = (hipStream_t)stream;
  PORL_TRY(porl_qnet_load_batch(h, batch, states, s_rs, actions, a_rs, nullptr, 0, nullptr, 0, nullptr, 0, stream));
  h->batch = 0;
  float* W = h->buf.workspace;
  float* q = nullptr;
  PORL_TRY(qnet_forward_one(h, h->buf.params, W + h->ws.xs, false, batch, s, &q));
  const int nblk = cdiv(batch, 256);
  hipLaunchKernelGGL(cql_penalty_kernel, dim3(nblk), dim3(256), 0, s, q, h->ld[h->cfg.n_hidden],
                     reinterpret_cast<const int64_t*>(W + h->ws.actions), batch, h->cfg.n_actions,
                     (float)std::log((double)h->cfg.n_actions), W + h->ws.part_pen);
  PORL_HIP(hipGetLastError());
  // sum of the per-block partials, scaled by 1/B: reuse the finalize kernel (td part = 0)
  hipLaunchKernelGGL(cql_finalize_kernel, dim3(1), dim3(64), 0, s, W + h->ws.part_pen, W + h->ws.part_pen, nblk,
                     1.0f / batch, 0.0f, W + h->ws.part_td);
  PORL_HIP(hipGetLastError());
  PORL_HIP(hipMemcpyAsync(out, W + h->ws.part_td + 2, sizeof(float), hipMemcpyDeviceToDevice, s));
  return PORL_OK;
}

// ---- online loop: record / act (csrc/online.hpp) ----------------------------------------------------------------------
int porl_qnet_record(porl_qnet* h, int64_t slot, const float* state, const float* next_state, int64_t action,
                     float reward, float done, const porl_qnet_mirror* m, void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!state || !next_state || !m || !m->states || !m->next_states || !m->actions || !m->rewards || !m->dones)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  const int S = h->cfg.state_dim;
  if (S > ONL_MAX_RECORD_S) PORL_FAIL(PORL_ERR_UNSUPPORTED, "state_dim %d > %d: too wide for the kernel arguments", S, ONL_MAX_RECORD_S);
  if (slot < 0 || slot >= m->capacity) PORL_FAIL(PORL_ERR_INVALID, "slot %lld outside [0,%lld)", (long long)slot, (long long)m->capacity);
  OnlineRecordArgs a;
  a.states = m->states; a.next_states = m->next_states; a.actions = m->actions; a.rewards = m->rewards; a.dones = m->dones;
  a.slot = slot; a.action = action; a.reward = reward; a.done = done; a.S = S;
  memcpy(a.x, state, sizeof(float) * S);
  memcpy(a.x + S, next_state, sizeof(float) * S);
  hipLaunchKernelGGL(online_record_kernel, dim3(1), dim3(S > 64 ? 256 : 64), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

static bool qnet_act_fits(const porl_qnet* h) {
  for (int l = 0; l <= h->cfg.n_hidden + 1; ++l)
    if (h->net.dims[l] > ONL_MAX_W) return false;
  return h->n_params <= (int64_t(1) << 19);
}

int32_t porl_qnet_act_ok(const porl_qnet* h) { return h && qnet_act_fits(h) ? 1 : 0; }

int porl_qnet_act(porl_qnet* h, int which, const porl_qnet_act_src* src, const porl_qnet_act_epilogue* epi, int32_t* out,
                  void* stream) {
  PORL_TRY(qnet_ready(h, false)); DevGuard _dg(h->device);
  if (!src || !epi || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (!qnet_act_fits(h))
    PORL_FAIL(PORL_ERR_INVALID, "network too large for the one-workgroup act kernel (a layer > %d wide or > 2^19 parameter "
              "floats); use porl_qnet_forward", ONL_MAX_W);
  const int B = src->batch, S = h->cfg.state_dim, n_out = h->cfg.n_actions;
  if (B < 1 || B > ONL_MAX_B) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", B, ONL_MAX_B);
  OnlineActArgs a;
  if (src->states) {
    if (src->row < 0 || src->row + B > src->n_rows) PORL_FAIL(PORL_ERR_INVALID, "rows [%lld,%lld) outside the %lld-row array",
                                                                (long long)src->row, (long long)(src->row + B), (long long)src->n_rows);
    if (src->s_rs < S) PORL_FAIL(PORL_ERR_INVALID, "row stride %lld < state_dim %d", (long long)src->s_rs, S);
    a.states = src->states + src->row * src->s_rs;
    a.s_rs = src->s_rs;
  } else {
    if (!src->inline_states) PORL_FAIL(PORL_ERR_INVALID, "no state source");
    if (B * S > ONL_MAX_INLINE) PORL_FAIL(PORL_ERR_INVALID, "inline states: %d x %d floats > %d", B, S, ONL_MAX_INLINE);
    a.states = nullptr;
    a.s_rs = S;
    memcpy(a.x_inline, src->inline_states, sizeof(float) * B * S);
  }
  a.kind = epi->kind;
  if (epi->kind == 0) {
    a.n_act = n_out; a.n_sub = 1;
  } else if (epi->kind == 1 || epi->kind == 2) {
    if (epi->n_act < 1 || epi->n_sub < 1 || (int64_t)epi->n_act * epi->n_sub != n_out)
      PORL_FAIL(PORL_ERR_INVALID, "epilogue (%d actions x %d) does not match the %d outputs", epi->n_act, epi->n_sub, n_out);
    if (epi->kind == 1 && !epi->support) PORL_FAIL(PORL_ERR_INVALID, "C51 epilogue needs the support");
    a.n_act = epi->n_act; a.n_sub = epi->n_sub;
  } else {
    PORL_FAIL(PORL_ERR_INVALID, "unknown epilogue kind %d", epi->kind);
  }
  a.support = epi->support;
  if (epi->n_stats < 0 || epi->n_stats > 3) PORL_FAIL(PORL_ERR_INVALID, "n_stats %d outside [0,3]", epi->n_stats);
  a.stats = epi->stats ? epi->stats : h->buf.stats;
  a.n_stats = epi->n_stats;
  // the record may be pinned host memory: the kernel stores through its device address
  if (out != h->act_out_host) {
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, out) != hipSuccess) {
      (void)hipGetLastError();
      PORL_FAIL(PORL_ERR_INVALID, "act record is neither device memory nor pinned host memory");
    }
    int32_t* dev = nullptr;
    if (pa.type == hipMemoryTypeDevice) dev = out;
    else if (pa.type == hipMemoryTypeHost && pa.devicePointer) dev = static_cast<int32_t*>(pa.devicePointer);
    if (!dev) PORL_FAIL(PORL_ERR_INVALID, "act record is neither device memory nor pinned host memory");
    h->act_out_host = out;
    h->act_out_dev = dev;
  }
  a.out = h->act_out_dev;
  a.params = which ? h->buf.params_tgt : h->buf.params;
  const int L = h->cfg.n_hidden;
  a.n_lin = L + 1;
  int maxw = 0;
  for (int l = 0; l <= L + 1; ++l) { a.dims[l] = h->net.dims[l]; maxw = std::max(maxw, h->net.dims[l]); }
  for (int l = 0; l <= L; ++l) { a.w_off[l] = h->net.w[l]; a.b_off[l] = h->net.b[l]; a.wld[l] = h->wld[l]; }
  a.B = B;
  a.ldx = (int)ru4(maxw);
  const size_t lds = sizeof(float) * 2 * B * a.ldx;          // <= 2 x 8 x 1024 floats = 64 KiB
  hipLaunchKernelGGL(online_act_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
