// IQL-family engine (porl_iql_*): twin value nets + target twin + Gaussian policy of POR and SORL (reference
// agent/por.py, agent/sorl.py), the update bench.py measures.  Included by porl_api.hip, which keeps what the other
// engines share (launch_group, pick_tile, pick_splitk, launch_reduce, add_reduce, adam_launch, ProfScope, Tune, DevGuard,
// the signals).
//
// One update = value phase (V1 load, V2/V3 forward of 4 nets, V4 head, V5/V6 backward, V7 combine, V8 Adam + Polyak) and
// policy phase (P1/P2 forward of 2 twins + policy, P3 mean, P4 NLL, P5 output layer, P6/P7 backward, P8 combine, P9 Adam);
// the policy-only step replaces P1..P4 by O1..O5 (5 forward-only nets, policy_weight_kernel).  Each host step exists once:
//   twin_fwd_net / policy_fwd_net     one net's share of a hidden-layer forward launch (fwd_hidden_layer)
//   bwd_layer_group                   one net's share of a hidden-layer backward launch: dW (+ db), dZ of the layer below
//   slabs / slab_floats               where the partial sums of a weight gradient live; porl_iql_create sizes by the same
//   dw0_splitk / splitk_to_slabs      a product split over K writes slabs, `red` gets the jobs that combine them
//   policy_mean_nll                   mean + NLL, the end of both forward halves
//   value_adam / policy_adam          the two Adam launches
//   iql_batch_loaded                  what every loader leaves behind
//   iql_enter, check_batch, check_replay_rows, need_pol_target, need_kind     the rejections; no HIP call comes before them
// The goal-conditioned behaviour-cloning step (porl_iql_bc_*, reference agent/por.py:178-183) is the policy phase on a
// batch of its own kind: stage_pairs_kernel (pairs.hpp) stages [obs | goal], the actions and unit weights, then B1/B2 the
// policy net's hidden layers alone, B3 mean, B4 NLL, P5..P7 the ordinary gradient half, B9 Adam.
// Nothing here allocates per launch outside g_prof.on: small configurations are bound by host time.

namespace {

int64_t add_tensor(std::vector<TensorInfo>& v, int64_t& cur, int rows, int cols) {
  const int64_t off = cur;
  v.push_back({off, rows, cols});
  cur += ru4((int64_t)(rows ? rows : 1) * cols);
  return off;
}

// named_parameters() order of util.mlp: Linear(w,b) [LayerNorm(w,b)] per hidden layer, final Linear
void layout_mlp(MlpLayout& m, std::vector<TensorInfo>& v, int64_t& cur, int in, int hid, int L, int out, bool ln) {
  m.n_lin = L + 1;
  m.ln = ln;
  m.dims[0] = in;
  for (int l = 0; l < L; ++l) m.dims[l + 1] = hid;
  m.dims[L + 1] = out;
  for (int l = 0; l <= L; ++l) {
    m.w[l] = add_tensor(v, cur, m.dims[l + 1], m.dims[l]);
    m.b[l] = add_tensor(v, cur, 0, m.dims[l + 1]);
    if (ln && l < L) {
      m.lnw[l] = add_tensor(v, cur, 0, hid);
      m.lnb[l] = add_tensor(v, cur, 0, hid);
    }
  }
}

struct Workspace {
  // xs / xt / target_v exist PORL_IQL_SLOTS times ("batch slots"): with PORL_IQL_MODE_TWO_SLOTS every load moves to the
  // next slot, so the policy phase of update t (on its own stream) can still read its minibatch while updates t+1 and
  // t+2 are being loaded
  int64_t xs_slot[PORL_IQL_SLOTS], xt_slot[PORL_IQL_SLOTS], target_v_slot[PORL_IQL_SLOTS];
  int64_t xn, rew, term;
  int64_t act_v[2][PORL_MAX_HIDDEN], act_t[2][2], act_p[PORL_MAX_HIDDEN];
  int64_t dz_v[2][2], dz_p[2];
  int64_t hp_t[2], hp_v[2];
  int64_t act_q[2][2], hp_q[2];      // policy phase only: scratch of the second twin forward and its head partials
  int64_t dv[2], dmu;
  int64_t slab_mean, slab_a, slab_b, slab_pa;   // slab_pa: the policy phase's own split-K slabs for dW0
  int64_t part_loss, part_min, part_dls;
  int64_t xhat_v[2][PORL_MAX_HIDDEN], rstd_v[2][PORL_MAX_HIDDEN];   // LayerNorm only
  int64_t ln_dg[2], ln_db[2], ln_dh[2];
  int64_t head_part[2], head_loss, head_db[2];                       // relu_head_bwd partials
  int64_t pol_w;                                                     // policy-only step: per-row weights (policy_weight_kernel)
  int64_t total;
};

}  // namespace

struct porl_iql {
  porl_iql_cfg cfg;
  MlpLayout v[2], pol;
  int64_t logstd_off = 0, n_vf = 0, n_pol = 0;
  std::vector<TensorInfo> t_vf, t_pol;
  porl_iql_buffers buf{};
  bool bound = false;
  int device = -1;                  // ordinal of the device that owns the bound buffers
  int mode = 0;                     // PORL_IQL_MODE_* bits
  int slot = 0;                     // batch slot of the most recent load
  ReduceArgs fin_v{}, fin_p{};      // PORL_IQL_MODE_FOLD_COMBINE: combines left pending by *_backward for *_apply
  bool fin_v_pending = false, fin_p_pending = false;
  int32_t adam_plan[2][6] = {};     // porl_iql_adam_plan: what the last Adam launch of each group did with its jobs
  int batch = 0;
  bool have_pol_target = false;
  bool pair_batch = false;          // staged by porl_iql_load_batch_cat / _pairs: [obs | goal], actions, unit weights and nothing else
  bool pol_prefetched = false;      // porl_iql_policy_prefetch ran for the loaded batch: policy forward is done
  bool pol_fwd_done = false;        // porl_iql_policy_forward ran for the loaded batch
  int pol_nslab = 1;
  int Sp = 0, Dp = 0, Hp = 0, parts_max = 0;
  Workspace ws{};
  Tune tune = g_tune;               // kernel selection: the process defaults at creation, porl_iql_tune_set
};

namespace {

// ---- rejections: every one of them comes before the entry point's first HIP call and leaves the engine as it was --------
int check_ready(const porl_iql* h, bool need_batch) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_iql_bind() has not been called");
  if (need_batch && h->batch <= 0) PORL_FAIL(PORL_ERR_INVALID, "no minibatch loaded (porl_iql_load_batch)");
  return 0;
}
// the entry points that take hyper-parameters
int iql_enter(const porl_iql* h, bool need_batch, const porl_iql_hyper* hp) {
  PORL_TRY(check_ready(h, need_batch));
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  return 0;
}
// every per-row buffer of the workspace holds max_batch rows
int check_batch(const porl_iql* h, int batch) {
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  return 0;
}
// a packed-row store [s | r | s' | d | a] that sampled_batch_kernel draws `batch` distinct rows from
int check_replay_rows(const porl_iql* h, int batch, const float* rows, int64_t row_stride, int64_t n_rows, int act_dim,
                      int target_is_action) {
  const int S = h->cfg.obs_dim, D = h->cfg.pol_out_dim;
  if (!rows || n_rows < batch || n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "replay rows: need batch <= n_rows <= 2^40");
  if (act_dim < 0 || row_stride < 2 * (int64_t)S + 2 + act_dim) PORL_FAIL(PORL_ERR_INVALID, "replay rows: row stride shorter than 2*S+2+A");
  if (target_is_action ? D != act_dim : D != S) PORL_FAIL(PORL_ERR_INVALID, "policy target width mismatch");
  return 0;
}
int need_pol_target(const porl_iql* h) {
  if (!h->have_pol_target) PORL_FAIL(PORL_ERR_INVALID, "policy step needs pol_target in porl_iql_load_batch");
  return 0;
}
// A batch staged by porl_iql_load_batch_cat / _pairs carries no next observations, rewards or flags: only the bc calls
// run on it, and they run on nothing else.
int need_kind(const porl_iql* h, bool pairs, const char* who) {
  if (h->pair_batch == pairs) return 0;
  if (pairs)
    PORL_FAIL(PORL_ERR_INVALID, "%s: the loaded batch was not staged by porl_iql_load_batch_cat / porl_iql_load_batch_pairs "
              "(a goal-conditioned batch: [obs | goal], actions, unit weights)", who);
  PORL_FAIL(PORL_ERR_INVALID, "%s: the loaded batch is a goal-conditioned one (porl_iql_load_batch_cat / porl_iql_load_batch_pairs): "
            "it has no next observations, rewards or flags; only porl_iql_bc_step / porl_iql_bc_forward run on it", who);
}

// What a loader leaves behind once its kernel is enqueued: the batch and what is known about it.
void iql_batch_loaded(porl_iql* h, int batch, bool have_target, bool pairs = false) {
  h->batch = batch;
  h->have_pol_target = have_target;
  h->pair_batch = pairs;
  h->pol_prefetched = false;
  h->pol_fwd_done = false;
}
// the staging slot a loader writes (moves on first under PORL_IQL_MODE_TWO_SLOTS)
int next_slot(porl_iql* h) {
  if (h->mode & PORL_IQL_MODE_TWO_SLOTS) h->slot = (h->slot + 1) % PORL_IQL_SLOTS;
  return h->slot;
}

// ---- kernel selection ---------------------------------------------------------------------------------------------------
bool short_blocks(const porl_iql* h) { return (h->mode & PORL_IQL_MODE_SHORT_BLOCKS) != 0; }
int skinny_mask(const porl_iql* h) {
  const Tune& t = h->tune;
  if (!short_blocks(h)) return t.skinny;
  return t.skinny_pipelined >= 0 ? t.skinny_pipelined : h->cfg.hidden_dim <= t.skinny_pipelined_max_h ? t.skinny : 0;
}
int iql_tile(const porl_iql* h, const GemmGroup& g) { return pick_tile(g, h->tune, short_blocks(h)); }

// `policy`: a launch of the update's policy phase (outside the two phases of an update the value pad applies)
int iql_launch(const porl_iql* h, GemmGroup& g, int tile, bool policy, hipStream_t s) {
  const Tune& t = h->tune;
  return launch_group(g, tile, t, s, !short_blocks(h) ? -1 : policy ? t.iql_pad_policy : t.iql_pad_value);
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// One hidden layer of up to MAX_FWD_NETS MLPs (at most 4 of them with LayerNorm) as one grouped launch (+ one LayerNorm launch for the nets that have it).
constexpr int MAX_FWD_NETS = 5;      // the policy-only step: target twin, online twin, policy
struct FwdNet {
  const float* in; int ldin;       // (B, K)
  const float* W; const float* b;  // (H, K), (H)
  float* out;                      // (B, Hp); may be null without LayerNorm when only the head is needed
  const float* headw; float* headout;
  const float* ln_g = nullptr; const float* ln_b = nullptr;   // LayerNorm affine (null = no LayerNorm)
  float* xhat = nullptr; float* rstd = nullptr;              // kept for backward when non-null
};

int fwd_hidden_layer(porl_iql* h, const FwdNet* nets, int nnets, int B, int K, bool last, int* parts_out, bool policy,
                     hipStream_t s) {
  const int H = h->cfg.hidden_dim;
  // input layer (K = obs_dim <= 64), plain Linear + ReLU with a stored output: its own one-round kernel (l0_fwd.hpp)
  if (h->tune.l0_kernel && K <= L0_KP && nnets <= L0_MAX_NETS) {
    L0Args a{};
    a.nnets = nnets; a.B = B; a.H = H; a.K = K; a.ldw = K; a.ldo = h->Hp;
    bool plain = true;
    for (int n = 0; n < nnets; ++n) {
      plain = plain && !nets[n].ln_g && nets[n].out && !(last && nets[n].headw);
      a.net[n] = L0Net{nets[n].in, nets[n].W, nets[n].b, nets[n].out, nets[n].ldin};
    }
    if (plain && l0_fwd_supported(a)) {
      if (parts_out) *parts_out = head_parts(H, 0);
      ProfScope ps("l0_fwd_kernel", s, 2.0 * nnets * B * (double)H * K, 4.0 * nnets * ((double)B * K + (double)H * K + (double)B * H));
      PORL_HIP(launch_l0_fwd(a, s));
      return 0;
    }
  }
  GemmGroup g{};
  g.nprob = nnets;
  bool any_ln = false;
  for (int n = 0; n < nnets; ++n) {
    const bool ln = nets[n].ln_g != nullptr;
    any_ln = any_ln || ln;
    GemmProb p = make_prob(GEMM_NT, nets[n].in, nets[n].ldin, nets[n].W, K, nets[n].out, h->Hp, B, H, K);
    p.bias = nets[n].b;
    p.act = ln ? ACT_NONE : ACT_RELU;
    p.store_c = nets[n].out != nullptr;
    if (ln && !nets[n].out) PORL_FAIL(PORL_ERR_INVALID, "LayerNorm needs a pre-activation buffer");
    if (!ln && last && nets[n].headw) { p.headw = nets[n].headw; p.headout = nets[n].headout; }
    g.p[n] = p;
  }
  const int tile = (K <= 128 && h->tune.l0_tile >= 0) ? h->tune.l0_tile : iql_tile(h, g);
  if (parts_out) *parts_out = any_ln ? 1 : head_parts(H, tile);
  PORL_TRY(iql_launch(h, g, tile, policy, s));
  if (any_ln) {
    LnFwdArgs a{};
    for (int n = 0; n < nnets; ++n) {
      if (!nets[n].ln_g) continue;
      const int k = a.nnets++;
      a.Z[k] = nets[n].out; a.xhat[k] = nets[n].xhat; a.rstd[k] = nets[n].rstd;
      a.gamma[k] = nets[n].ln_g; a.beta[k] = nets[n].ln_b;
      a.headw[k] = last ? nets[n].headw : nullptr; a.headb[k] = nullptr; a.headout[k] = nets[n].headout;
    }
    a.B = B; a.H = H; a.ld = h->Hp; a.rows_per_block = LN_ROWS_PER_BLOCK;
    hipLaunchKernelGGL(ln_relu_fwd_kernel, dim3(cdiv(B, LN_ROWS_PER_BLOCK), a.nnets), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  return 0;
}

// Layer l of value twin i with parameters P (online or target arena).  Layer 0 reads the staged rows at workspace offset
// `in0`, later layers the previous activation.  `keep`: `act` holds one buffer per layer, every output is stored, and
// with LayerNorm the row statistics are kept for the backward pass; otherwise `act` is a ping-pong pair and the last
// layer's output is not stored unless LayerNorm needs it (only the head partials at `headout` are wanted).
FwdNet twin_fwd_net(const porl_iql* h, const float* P, int i, int l, int64_t in0, const int64_t* act, bool keep, int64_t headout) {
  float* W = h->buf.workspace;
  const MlpLayout& m = h->v[i];
  const int L = h->cfg.n_hidden;
  const bool LN = h->cfg.layer_norm != 0;
  FwdNet f{};
  if (l == 0) { f.in = W + in0; f.ldin = h->Sp; }
  else { f.in = W + act[keep ? l - 1 : (l - 1) & 1]; f.ldin = h->Hp; }
  f.W = P + m.w[l]; f.b = P + m.b[l];
  f.out = (!keep && l == L - 1 && !LN) ? nullptr : W + act[keep ? l : l & 1];
  f.headw = P + m.w[L]; f.headout = W + headout;
  if (LN) {
    f.ln_g = P + m.lnw[l]; f.ln_b = P + m.lnb[l];
    if (keep) { f.xhat = W + h->ws.xhat_v[i][l]; f.rstd = W + h->ws.rstd_v[i][l]; }
  }
  return f;
}

// Layer l of the policy net: every activation is kept in act_p (its backward reads them), no head.
FwdNet policy_fwd_net(const porl_iql* h, int l, int64_t in0) {
  float* W = h->buf.workspace;
  const float* Pp = h->buf.params_pol;
  FwdNet f{};
  if (l == 0) { f.in = W + in0; f.ldin = h->Sp; }
  else { f.in = W + h->ws.act_p[l - 1]; f.ldin = h->Hp; }
  f.W = Pp + h->pol.w[l]; f.b = Pp + h->pol.b[l];
  f.out = W + h->ws.act_p[l];
  return f;
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// One net's share of hidden layer l's backward launch: dW_l = dZ_l^T In with db_l as its column sums and, above layer 0
// (dz_prev non-null), dZ_{l-1} = dZ_l W_l, times 1[mask > 0] where a ReLU sits between (mask null: LayerNorm's own
// backward kernel applies it).
struct BwdNet {
  const float* dz;                    // (B, H) dZ_l
  const float* in; int ldin;          // (B, Kin) input of layer l
  float* gw; float* gb;               // gradients of W_l, b_l
  const float* W; float* dz_prev; const float* mask;
};
void bwd_layer_group(const porl_iql* h, GemmGroup& g, const BwdNet& n, int Kin) {
  const int B = h->batch, H = h->cfg.hidden_dim, Hp = h->Hp;
  GemmProb p = make_prob(GEMM_TN, n.dz, Hp, n.in, n.ldin, n.gw, Kin, H, Kin, B);
  p.colsum = n.gb;
  g.p[g.nprob++] = p;
  if (!n.dz_prev) return;
  GemmProb q = make_prob(GEMM_NN, n.dz, Hp, n.W, Kin, n.dz_prev, Hp, B, Kin, H);
  if (n.mask) { q.mask = n.mask; q.ldmask = Hp; }
  g.p[g.nprob++] = q;
}

// Partial sums of a weight gradient (rows x cols) and of its column sums: SK_MAX slabs of `per` floats at W, then SK_MAX
// slabs of `perc` floats at C.  Written by a product split over K (or by the skinny kernels, over batch chunks), combined
// by multi_reduce_kernel or inside the Adam launch.
enum SlabSet { SLAB_TWIN0 = 0, SLAB_TWIN1 = 1, SLAB_POLICY, SLAB_OUT };   // dW0 of a value twin / of the policy; the policy's output layer
struct Slabs { float* W; float* C; long per, perc; };
int64_t slab_floats(const porl_iql_cfg& c, SlabSet which) {
  const int64_t S = c.obs_dim, D = c.pol_out_dim, H = c.hidden_dim;
  return which == SLAB_OUT ? SK_MAX * (D * H + D + 8) : SK_MAX * (H * S + 2 * H + 8);
}
Slabs slabs(const porl_iql* h, SlabSet which) {
  const long rows = which == SLAB_OUT ? h->cfg.pol_out_dim : h->cfg.hidden_dim;
  const long cols = which == SLAB_OUT ? h->cfg.hidden_dim : h->cfg.obs_dim;
  const Workspace& ws = h->ws;
  float* base = h->buf.workspace + (which == SLAB_OUT ? ws.slab_b : which == SLAB_POLICY ? ws.slab_pa
                                                                     : ws.slab_a + which * slab_floats(h->cfg, which));
  return Slabs{base, base + SK_MAX * rows * cols, rows * cols, rows};
}

// Problem p (a weight gradient with column sums) is split `sk` ways over K: it writes slabs instead of the gradient, and
// `red` gets the two jobs that combine them into where p pointed.
void splitk_to_slabs(GemmProb& p, const Slabs& sl, int sk, ReduceArgs& red) {
  add_reduce(red, p.C, sl.W, sl.per, sl.per, sk);
  add_reduce(red, p.colsum, sl.C, sl.perc, sl.perc, sk);
  p.splitk = sk; p.C = sl.W; p.colsum = sl.C;
}

// The layer-0 group (problem i = dW0 of net i, nothing else) is a skinny (H x S) product: split the batch (K) dimension
// to fill the chip.
void dw0_splitk(const porl_iql* h, GemmGroup& g, int tile, int nnets, SlabSet first, ReduceArgs& red) {
  int bm, bn;
  tile_dims(tile, bm, bn);
  const int sk = pick_splitk(h->cfg.hidden_dim, h->cfg.obs_dim, h->batch, nnets, bm, bn);
  if (sk > 1)
    for (int i = 0; i < nnets; ++i) splitk_to_slabs(g.p[i], slabs(h, SlabSet(first + i)), sk, red);
}

// Input-layer weight gradients dW0 = dZ0^T X (+ db0) of up to 4 nets on wgrad_skinny_kernel (skinny.hpp): slabs over
// batch chunks in the split-K layout, combine jobs appended to `red`.  Returns false when the shapes do not qualify
// (the caller then takes the grouped-GEMM path).
struct Dw0Net { const float* dz; float* gw; float* gb; Slabs sl; };
bool dw0_skinny(const porl_iql* h, const Dw0Net* nets, int nnets, ReduceArgs& red, const char* phase, hipStream_t s, int* rc) {
  const int B = h->batch, H = h->cfg.hidden_dim, S = h->cfg.obs_dim, ldx = h->Sp, ldz = h->Hp;
  const float* X = h->buf.workspace + h->ws.xs_slot[h->slot];
  *rc = 0;
  if (!(skinny_mask(h) & 1) || S > SKN_T || nnets > SKN_MAX_NETS || H % 4 || !skn_ok4(X, ldx) || ldz % 4) return false;
  for (int i = 0; i < nnets; ++i) if (!skn_ok4(nets[i].dz, ldz)) return false;
  WgradSkinnyArgs a{};
  a.nnets = nnets; a.B = B; a.H = H; a.S = S; a.ldz = ldz; a.ldx = ldx; a.ldo = S;
  a.tiles_n = cdiv(H, SKN_T);
  skn_split(cdiv(B, SKN_T), h->tune.dw0_slabs, a.nslab, a.rtiles);
  a.slabW_stride = (long)H * S; a.slabC_stride = H;
  for (int i = 0; i < nnets; ++i) {
    a.net[i] = WgradSkinnyNet{nets[i].dz, X, nets[i].sl.W, nets[i].sl.C};
    add_reduce(red, nets[i].gw, nets[i].sl.W, (long)H * S, (long)H * S, a.nslab);
    add_reduce(red, nets[i].gb, nets[i].sl.C, H, H, a.nslab);
  }
  g_phase = phase;
  {
    ProfScope ps("wgrad_skinny_kernel", s, 2.0 * nnets * B * (double)H * S,
                 4.0 * nnets * ((double)B * H + (double)B * S + (double)a.nslab * H * (S + 1)));
    hipLaunchKernelGGL(wgrad_skinny_kernel, dim3(nnets * a.nslab * a.tiles_n), dim3(256), 0, s, a);
  }
  g_phase = "";
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_err = std::string("wgrad_skinny_kernel: ") + hipGetErrorString(e); *rc = (int)e; }
  return true;
}

// The backward pass ends with its combine: issued as a launch, or handed to the caller who folds it into the Adam launch.
int combine_or_defer(ReduceArgs& red, ReduceArgs* defer, hipStream_t s) {
  if (defer) { *defer = red; return 0; }
  return launch_reduce(red, s);
}

// ---- value phase --------------------------------------------------------------------------------------------------------
// forward: target twins on s', online twins on s — 4 nets per launch; returns the head partials per row in *parts
int value_forward(porl_iql* h, hipStream_t s, int* parts) {
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  const Workspace& ws = h->ws;
  for (int l = 0; l < L; ++l) {
    FwdNet nets[4];
    for (int i = 0; i < 2; ++i) {
      nets[i] = twin_fwd_net(h, h->buf.params_tgt, i, l, ws.xn, ws.act_t[i], false, ws.hp_t[i]);
      nets[2 + i] = twin_fwd_net(h, h->buf.params_vf, i, l, ws.xs_slot[h->slot], ws.act_v[i], true, ws.hp_v[i]);
    }
    g_phase = l == 0 ? "V2.L0fwd:" : "V3.fwd:";
    PORL_TRY(fwd_hidden_layer(h, nets, 4, h->batch, l == 0 ? S : H, l == L - 1, parts, false, s));
  }
  g_phase = "V4.head:";
  return PORL_OK;
}

// LayerNorm variant of the value backward: TD target, expectile loss and dL/dv from a kernel of their own; dZ of every
// hidden layer is materialised by the LayerNorm backward kernel (row statistics), gamma/beta/(head) gradients come from
// its per-block partial sums.  (Its launches keep the profile prefix the forward left, "V4.head:".)
int value_backward_ln(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, int parts, ReduceArgs* defer) {
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, Hp = h->Hp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  const float* Pt = h->buf.params_tgt;
  float* Gv = h->buf.grads_vf;
  {
    ValueLossArgs a{};
    for (int i = 0; i < 2; ++i) {
      a.hp_t[i] = W + ws.hp_t[i]; a.hp_v[i] = W + ws.hp_v[i];
      a.b_t[i] = Pt + h->v[i].b[L]; a.b_v[i] = Pv + h->v[i].b[L];
      a.dv[i] = W + ws.dv[i];
      a.db_out[i] = Gv + h->v[i].b[L];
    }
    a.rew = W + ws.rew; a.term = W + ws.term; a.target_v = W + ws.target_v_slot[h->slot]; a.stats = h->buf.stats;
    a.B = B; a.parts = parts; a.tau = hp->tau; a.discount = hp->discount; a.inv_batch = hp->inv_batch;
    hipLaunchKernelGGL(value_loss_kernel, dim3(1), dim3(1024), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  const int nln = cdiv(B, LN_ROWS_PER_BLOCK);
  for (int l = L - 1; l >= 0; --l) {
    const bool top = l == L - 1;
    {
      LnBwdArgs a{};
      a.nnets = 2;
      for (int i = 0; i < 2; ++i) {
        a.dH[i] = top ? nullptr : W + ws.dz_v[i][0];
        a.dv[i] = W + ws.dv[i]; a.headw[i] = Pv + h->v[i].w[L];
        a.Hact[i] = W + ws.act_v[i][l]; a.xhat[i] = W + ws.xhat_v[i][l]; a.rstd[i] = W + ws.rstd_v[i][l];
        a.gamma[i] = Pv + h->v[i].lnw[l];
        a.dZ[i] = W + ws.dz_v[i][1];
        a.part_dgamma[i] = W + ws.ln_dg[i]; a.part_dbeta[i] = W + ws.ln_db[i]; a.part_dhead[i] = W + ws.ln_dh[i];
      }
      a.B = B; a.H = H; a.ld = Hp; a.rows_per_block = LN_ROWS_PER_BLOCK;
      hipLaunchKernelGGL(ln_relu_bwd_kernel, dim3(nln, 2), dim3(256), 0, s, a);
      PORL_HIP(hipGetLastError());
      ReduceArgs r{};
      for (int i = 0; i < 2; ++i) {
        add_reduce(r, Gv + h->v[i].lnw[l], W + ws.ln_dg[i], H, H, nln);
        add_reduce(r, Gv + h->v[i].lnb[l], W + ws.ln_db[i], H, H, nln);
        if (top) add_reduce(r, Gv + h->v[i].w[L], W + ws.ln_dh[i], H, H, nln);
      }
      PORL_TRY(launch_reduce(r, s));
    }
    ReduceArgs red{};
    GemmGroup g{};
    for (int i = 0; i < 2; ++i) {
      const MlpLayout& m = h->v[i];
      BwdNet n{W + ws.dz_v[i][1], nullptr, Hp, Gv + m.w[l], Gv + m.b[l], Pv + m.w[l], nullptr, nullptr};
      if (l == 0) { n.in = W + ws.xs_slot[h->slot]; n.ldin = h->Sp; }
      else { n.in = W + ws.act_v[i][l - 1]; n.dz_prev = W + ws.dz_v[i][0]; }
      bwd_layer_group(h, g, n, l == 0 ? S : H);
    }
    const int tile = iql_tile(h, g);
    if (l == 0) dw0_splitk(h, g, tile, 2, SLAB_TWIN0, red);
    PORL_TRY(iql_launch(h, g, tile, false, s));
    // only the last combine can wait for the Adam launch: the LayerNorm partial buffers are reused layer by layer
    PORL_TRY(combine_or_defer(red, l == 0 ? defer : nullptr, s));
  }
  return PORL_OK;
}

// Plain-ReLU variant: TD target, expectile loss and dL/dv are fused into the head backward.
int value_backward_relu(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, int parts, ReduceArgs* defer) {
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, Hp = h->Hp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  const float* Pt = h->buf.params_tgt;
  float* Gv = h->buf.grads_vf;
  ReduceArgs red{};
  // -- head + last ReLU backward: dZ_{L-1} = dv w_L^T . 1[H_{L-1} > 0], dW_L = dv^T H_{L-1} (partials) -----
  {
    const int nhb = cdiv(B, HEAD_ROWS_PER_BLOCK);
    HeadBwdArgs a{};
    for (int i = 0; i < 2; ++i) {
      a.Hact[i] = W + ws.act_v[i][L - 1]; a.w[i] = Pv + h->v[i].w[L];
      a.dZ[i] = W + ws.dz_v[i][(L - 1) & 1]; a.part_dw[i] = W + ws.head_part[i];
      a.hp_t[i] = W + ws.hp_t[i]; a.hp_v[i] = W + ws.hp_v[i];
      a.b_t[i] = Pt + h->v[i].b[L]; a.b_v[i] = Pv + h->v[i].b[L];
      a.dv[i] = W + ws.dv[i]; a.part_db[i] = W + ws.head_db[i];
      add_reduce(red, Gv + h->v[i].w[L], W + ws.head_part[i], H, H, nhb);
      add_reduce(red, Gv + h->v[i].b[L], W + ws.head_db[i], 1, 1, nhb);
    }
    a.rew = W + ws.rew; a.term = W + ws.term; a.target_v = W + ws.target_v_slot[h->slot]; a.part_loss = W + ws.head_loss;
    add_reduce(red, h->buf.stats, W + ws.head_loss, 1, 1, nhb, 0, hp->inv_batch);     // stats[0] = v_loss
    a.B = B; a.H = H; a.ld = Hp; a.parts = parts;
    a.tau = hp->tau; a.discount = hp->discount; a.inv_batch = hp->inv_batch;
    ProfScope ps("relu_head_bwd_kernel", s, 0.0, 16.0 * B * H);
    hipLaunchKernelGGL(relu_head_bwd_kernel, dim3(nhb, 2), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  for (int l = L - 1; l >= 0; --l) {
    if (l == 0) {
      // skinny (H x S) weight gradient on its own kernel: one 64 x 64 tile of dZ0 per block, slabs over batch chunks
      Dw0Net dn[2];
      for (int i = 0; i < 2; ++i) dn[i] = Dw0Net{W + ws.dz_v[i][0], Gv + h->v[i].w[0], Gv + h->v[i].b[0], slabs(h, SlabSet(SLAB_TWIN0 + i))};
      int rc = 0;
      if (dw0_skinny(h, dn, 2, red, "V6.dW0:", s, &rc)) {
        if (rc) return rc;
        break;
      }
    }
    GemmGroup g{};
    for (int i = 0; i < 2; ++i) {
      const MlpLayout& m = h->v[i];
      BwdNet n{W + ws.dz_v[i][l & 1], nullptr, Hp, Gv + m.w[l], Gv + m.b[l], Pv + m.w[l], nullptr, nullptr};
      if (l == 0) { n.in = W + ws.xs_slot[h->slot]; n.ldin = h->Sp; }
      else { n.in = n.mask = W + ws.act_v[i][l - 1]; n.dz_prev = W + ws.dz_v[i][(l - 1) & 1]; }
      bwd_layer_group(h, g, n, l == 0 ? S : H);
    }
    int tile = iql_tile(h, g);
    if (l > 0 && short_blocks(h) && h->tune.vbwd_tile_short >= 0) tile = h->tune.vbwd_tile_short;
    if (l == 0) dw0_splitk(h, g, tile, 2, SLAB_TWIN0, red);
    g_phase = l == 0 ? "V6.dW0:" : "V5.bwd:";
    PORL_TRY(iql_launch(h, g, tile, false, s));
  }
  g_phase = "V7.combine:";
  PORL_TRY(combine_or_defer(red, defer, s));
  g_phase = "";
  return PORL_OK;
}

// `defer` (optional): the final combine launch is not issued; its jobs are handed to the caller, who folds them into
// the Adam launch (porl_iql_step, PORL_IQL_MODE_FOLD_COMBINE).
int value_backward_impl(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, ReduceArgs* defer) {
  int parts = 0;
  PORL_TRY(value_forward(h, s, &parts));
  return h->cfg.layer_norm ? value_backward_ln(h, hp, s, parts, defer) : value_backward_relu(h, hp, s, parts, defer);
}

int value_adam(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, const ReduceArgs* fin) {
  g_phase = "V8.";
  const int rc = adam_launch(h->buf.params_vf, h->buf.grads_vf, h->buf.adam_m_vf, h->buf.adam_v_vf, h->buf.params_tgt, h->n_vf,
                             hp->value_lr, hp->value_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, hp->ema_beta, s, fin,
                             h->adam_plan[0]);
  g_phase = "";
  return rc;
}

// ---- policy phase -------------------------------------------------------------------------------------------------------
// `phase`: "P9." in the joint update, "O9." in the policy-only step
int policy_adam(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, const ReduceArgs* fin, const char* phase) {
  g_phase = phase;
  const int rc = adam_launch(h->buf.params_pol, h->buf.grads_pol, h->buf.adam_m_pol, h->buf.adam_v_pol, nullptr, h->n_pol,
                             hp->policy_lr, hp->policy_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0, s, fin, h->adam_plan[1]);
  g_phase = "";
  return rc;
}

// policy mean (pre-bias, pre-activation) as split-K slabs: act_p[L-1] (B,H) x W_L^T (H,D)
int policy_mean_slabs(porl_iql* h, int B, int* nslab, bool policy, hipStream_t s) {
  const int H = h->cfg.hidden_dim, D = h->cfg.pol_out_dim, L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  if ((skinny_mask(h) & 2) && D <= SKN_T && H % 4 == 0 && skn_ok4(W + h->ws.act_p[L - 1], h->Hp) &&
      skn_ok4(h->buf.params_pol + h->pol.w[L], H) && h->Dp % 4 == 0) {
    MeanSkinnyArgs a{};
    a.A = W + h->ws.act_p[L - 1]; a.W = h->buf.params_pol + h->pol.w[L]; a.slab = W + h->ws.slab_mean;
    a.B = B; a.H = H; a.D = D; a.lda = h->Hp; a.ldw = H; a.ldo = h->Dp;
    a.tiles_m = cdiv(B, SKN_T);
    // few row tiles (small batches): more slabs keep the chip busy; at B >= 1024 eight 128-deep slabs halve what the
    // NLL kernel reads back
    skn_split(cdiv(H, SKN_T), a.tiles_m >= 16 ? SK_MAX / 2 : SK_MAX, a.nslab, a.ktiles);
    a.slab_stride = (long)B * h->Dp;
    *nslab = a.nslab;
    ProfScope ps("mean_skinny_kernel", s, 2.0 * B * (double)H * D, 4.0 * ((double)B * H + (double)D * H + (double)a.nslab * B * h->Dp));
    hipLaunchKernelGGL(mean_skinny_kernel, dim3(a.tiles_m * a.nslab), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
    return 0;
  }
  GemmGroup g{};
  g.nprob = 1;
  g.p[0] = make_prob(GEMM_NT, W + h->ws.act_p[L - 1], h->Hp, h->buf.params_pol + h->pol.w[L], H, W + h->ws.slab_mean,
                     h->Dp, B, D, H);
  const int tile = iql_tile(h, g);
  int bm, bn;
  tile_dims(tile, bm, bn);
  const int sk = pick_splitk(B, D, H, 1, bm, bn);
  // splitk == 1 still writes the raw product (bias and tanh are applied by the consumer)
  g.p[0].splitk = sk;
  *nslab = sk;
  if (sk == 1) { g.p[0].bias = nullptr; g.p[0].act = ACT_NONE; }
  return iql_launch(h, g, tile, policy, s);
}

// The end of both forward halves: the policy mean (unless porl_iql_policy_prefetch left it: `pre`), then advantage
// weights, NLL, dL/dmean and dL/dlog_std.  The weights come per row from `weight` (policy-only step) or are formed from
// the twins' `parts` head partials and the value phase's target_v.
int policy_mean_nll(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, bool pre, int parts, const float* weight,
                    const char* mean_phase, const char* nll_phase) {
  const int B = h->batch, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim, Dp = h->Dp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pp = h->buf.params_pol;
  int nslab = h->pol_nslab;
  g_phase = mean_phase;
  if (!pre) PORL_TRY(policy_mean_slabs(h, B, &nslab, true, s));
  g_phase = nll_phase;
  {
    PolicyNllArgs a{};
    for (int i = 0; i < 2; ++i) { a.hp_v[i] = W + ws.hp_q[i]; a.b_v[i] = h->buf.params_vf + h->v[i].b[L]; }
    a.parts = weight ? 0 : parts; a.target_v = W + ws.target_v_slot[h->slot];
    a.weight = weight;
    a.mean_slab = W + ws.slab_mean; a.nslab = nslab; a.slab_stride = (long)B * Dp;
    a.mean_bias = Pp + h->pol.b[L]; a.log_std = Pp + h->logstd_off;
    a.x = W + ws.xt_slot[h->slot]; a.ldx = Dp; a.dmean = W + ws.dmu; a.ldd = Dp;
    a.part_loss = W + ws.part_loss; a.part_min = W + ws.part_min; a.part_dls = W + ws.part_dls;
    a.B = B; a.D = D; a.ldm = Dp; a.tanh_mean = h->cfg.pol_tanh; a.weight_mode = h->cfg.weight_mode;
    a.alpha = hp->alpha; a.inv_batch = hp->inv_batch; a.rows_per_block = NLL_ROWS_PER_BLOCK;
    ProfScope ps("policy_nll_kernel", s, 0.0, 4.0 * B * (nslab + 2.0) * Dp);
    hipLaunchKernelGGL(policy_nll_kernel, dim3(cdiv(B, NLL_ROWS_PER_BLOCK)), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  g_phase = "";
  h->pol_fwd_done = true;
  return PORL_OK;
}

// Forward half of the joint update's policy phase — everything of it that reads the VALUE parameters: the updated twins
// (head only) + the policy's hidden layers, 3 nets per launch, then mean and NLL.  The policy net is left out when
// porl_iql_policy_prefetch already ran it for this batch.
int policy_forward_half(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s) {
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  const Workspace& ws = h->ws;
  const bool pre = h->pol_prefetched;
  h->pol_prefetched = false;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    FwdNet nets[3];
    for (int i = 0; i < 2; ++i) nets[i] = twin_fwd_net(h, h->buf.params_vf, i, l, ws.xs_slot[h->slot], ws.act_q[i], false, ws.hp_q[i]);
    nets[2] = policy_fwd_net(h, l, ws.xs_slot[h->slot]);
    g_phase = l == 0 ? "P1.L0fwd:" : "P2.fwd:";
    PORL_TRY(fwd_hidden_layer(h, nets, pre ? 2 : 3, h->batch, l == 0 ? S : H, l == L - 1, &parts, true, s));
  }
  return policy_mean_nll(h, hp, s, pre, parts, nullptr, "P3.mean:", "P4.");
}

// Forward half of the policy-only step (porl_iql_policy_only_*): all five nets forward-only — target twin on s', online
// twin on s, policy on s — in one grouped launch per layer, no V-net activation kept, and the per-row weights from
// policy_weight_kernel (TD target included) instead of the value phase's target_v.
int policy_only_forward_half(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s) {
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  const float* Pt = h->buf.params_tgt;
  const bool pre = h->pol_prefetched;
  h->pol_prefetched = false;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    FwdNet nets[MAX_FWD_NETS];
    for (int i = 0; i < 2; ++i) {
      nets[i] = twin_fwd_net(h, Pt, i, l, ws.xn, ws.act_t[i], false, ws.hp_t[i]);
      nets[2 + i] = twin_fwd_net(h, Pv, i, l, ws.xs_slot[h->slot], ws.act_q[i], false, ws.hp_q[i]);
    }
    nets[4] = policy_fwd_net(h, l, ws.xs_slot[h->slot]);
    g_phase = l == 0 ? "O1.L0fwd:" : "O2.fwd:";
    PORL_TRY(fwd_hidden_layer(h, nets, pre ? 4 : 5, B, l == 0 ? S : H, l == L - 1, &parts, true, s));
  }
  g_phase = "O3.head:";
  PolicyWeightArgs a{};
  for (int i = 0; i < 2; ++i) {
    a.hp_t[i] = W + ws.hp_t[i]; a.hp_v[i] = W + ws.hp_q[i];
    a.b_t[i] = Pt + h->v[i].b[L]; a.b_v[i] = Pv + h->v[i].b[L];
  }
  a.rew = W + ws.rew; a.term = W + ws.term; a.target_v = W + ws.target_v_slot[h->slot]; a.weight = W + ws.pol_w;
  a.B = B; a.parts = parts; a.weight_mode = h->cfg.weight_mode; a.discount = hp->discount; a.alpha = hp->alpha;
  {
    ProfScope ps("policy_weight_kernel", s, 0.0, 4.0 * B * (4.0 * parts + 4.0));
    hipLaunchKernelGGL(policy_weight_kernel, dim3(cdiv(B, PW_ROWS_PER_BLOCK)), dim3(256), 0, s, a);
  }
  PORL_HIP(hipGetLastError());
  return policy_mean_nll(h, hp, s, pre, parts, W + ws.pol_w, "O4.mean:", "O5.");
}

// Forward half of the behaviour-cloning step (porl_iql_bc_*, reference por.py:178-180): the policy net's hidden layers,
// one net per launch as porl_iql_policy_prefetch issues them, then mean and NLL with the unit weights the loader staged.
// No V net runs and no weight kernel: L + 2 launches.
int bc_forward_half(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s) {
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  h->pol_prefetched = false;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    const FwdNet f = policy_fwd_net(h, l, h->ws.xs_slot[h->slot]);
    g_phase = l == 0 ? "B1.L0fwd:" : "B2.fwd:";
    PORL_TRY(fwd_hidden_layer(h, &f, 1, h->batch, l == 0 ? S : H, l == L - 1, &parts, true, s));
  }
  return policy_mean_nll(h, hp, s, false, 0, h->buf.workspace + h->ws.pol_w, "B3.mean:", "B4.");
}

// Gradient half: needs a forward half of the same batch (dL/dmean, the NLL partials, act_p).  Touches policy state only.
int policy_gradient_half(porl_iql* h, hipStream_t s, ReduceArgs* defer) {
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim;
  const int Hp = h->Hp, Dp = h->Dp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pp = h->buf.params_pol;
  float* Gp = h->buf.grads_pol;
  const int nblk = cdiv(B, NLL_ROWS_PER_BLOCK);
  h->pol_fwd_done = false;

  ReduceArgs red{};
  // the NLL kernel's per-block partials are combined by the step's final reduce launch
  add_reduce(red, Gp + h->logstd_off, W + ws.part_dls, D, D, nblk);            // d/dlog_std (already clamp-masked)
  add_reduce(red, h->buf.stats + 1, W + ws.part_loss, 1, 1, nblk);            // stats[1] = g_loss
  add_reduce(red, h->buf.stats + 2, W + ws.part_min, 1, 1, nblk, /*min*/ 1);  // stats[2] = min NLL
  const Slabs out = slabs(h, SLAB_OUT);
  if ((skinny_mask(h) & 4) && D <= SKN_T && H % 4 == 0 && Dp % 4 == 0 && Hp % 4 == 0 && skn_ok4(Pp + h->pol.w[L], H)) {
    // output layer on out_bwd_kernel (skinny.hpp): one pass over the last hidden activation gives dZ_{L-1} and the
    // dW_L / db_L slabs
    OutBwdArgs a{};
    a.dmu = W + ws.dmu; a.W = Pp + h->pol.w[L]; a.A = W + ws.act_p[L - 1];
    a.dZ = W + ws.dz_p[(L - 1) & 1];
    a.slabW = out.W; a.slabC = out.C;
    a.B = B; a.H = H; a.D = D; a.lddmu = Dp; a.ldw = H; a.lda = Hp; a.lddz = Hp;
    a.tiles_n = cdiv(H, SKN_T);
    skn_split(cdiv(B, SKN_T), SK_MAX, a.nslab, a.rtiles);
    a.slabW_stride = out.per; a.slabC_stride = out.perc;
    add_reduce(red, Gp + h->pol.w[L], out.W, out.per, out.per, a.nslab);
    add_reduce(red, Gp + h->pol.b[L], out.C, out.perc, out.perc, a.nslab);
    g_phase = "P5.outbwd:";
    {
      ProfScope ps("out_bwd_kernel", s, 4.0 * B * (double)H * D, 4.0 * (2.0 * B * H + (double)B * D + (double)D * H + (double)a.nslab * D * H));
      hipLaunchKernelGGL(out_bwd_kernel, dim3(a.nslab * a.tiles_n), dim3(256), 0, s, a);
    }
    g_phase = "";
    PORL_HIP(hipGetLastError());
  } else {
    // output layer: dW_L = dmu^T H_{L-1} (D x H, skinny M), and dZ_{L-1} = (dmu W_L) . 1[H_{L-1} > 0]
    GemmGroup g{};
    g.nprob = 2;
    g.p[0] = make_prob(GEMM_TN, W + ws.dmu, Dp, W + ws.act_p[L - 1], Hp, Gp + h->pol.w[L], H, D, H, B);
    g.p[0].colsum = Gp + h->pol.b[L];
    g.p[1] = make_prob(GEMM_NN, W + ws.dmu, Dp, Pp + h->pol.w[L], H, W + ws.dz_p[(L - 1) & 1], Hp, B, H, D);
    g.p[1].mask = W + ws.act_p[L - 1]; g.p[1].ldmask = Hp;
    const int tile = D <= 64 ? TILE_64x128 : iql_tile(h, g);
    int bm, bn;
    tile_dims(tile, bm, bn);
    const int sk = pick_splitk(D, H, B, 1, bm, bn);
    if (sk > 1) splitk_to_slabs(g.p[0], out, sk, red);
    g_phase = "P5.outbwd:";
    PORL_TRY(iql_launch(h, g, tile, true, s));
  }
  for (int l = L - 1; l >= 0; --l) {
    if (l == 0) {
      const Dw0Net dn{W + ws.dz_p[0], Gp + h->pol.w[0], Gp + h->pol.b[0], slabs(h, SLAB_POLICY)};
      int rc = 0;
      if (dw0_skinny(h, &dn, 1, red, "P7.dW0:", s, &rc)) {
        if (rc) return rc;
        break;
      }
    }
    GemmGroup g{};
    BwdNet n{W + ws.dz_p[l & 1], nullptr, Hp, Gp + h->pol.w[l], Gp + h->pol.b[l], Pp + h->pol.w[l], nullptr, nullptr};
    if (l == 0) { n.in = W + ws.xs_slot[h->slot]; n.ldin = h->Sp; }
    else { n.in = n.mask = W + ws.act_p[l - 1]; n.dz_prev = W + ws.dz_p[(l - 1) & 1]; }
    bwd_layer_group(h, g, n, l == 0 ? S : H);
    const int tile = iql_tile(h, g);
    if (l == 0) dw0_splitk(h, g, tile, 1, SLAB_POLICY, red);
    g_phase = l == 0 ? "P7.dW0:" : "P6.bwd:";
    PORL_TRY(iql_launch(h, g, tile, true, s));
  }
  g_phase = "P8.combine:";
  PORL_TRY(combine_or_defer(red, defer, s));
  g_phase = "";
  return PORL_OK;
}

// The joint update's policy phase: the forward half unless porl_iql_policy_forward already ran it, then the gradient half.
int policy_backward_impl(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, ReduceArgs* defer) {
  PORL_TRY(need_pol_target(h));
  if (!h->pol_fwd_done) PORL_TRY(policy_forward_half(h, hp, s));
  return policy_gradient_half(h, s, defer);
}

// ---- forward-only entry points ------------------------------------------------------------------------------------------
int pack_x(porl_iql* h, const float* x, int64_t x_rs, int batch, int64_t dst_off, hipStream_t s) {
  if (!x) PORL_FAIL(PORL_ERR_INVALID, "null input");
  PackArgs a{};
  a.rows = batch; a.njobs = 1;
  a.job[0].src = x; a.job[0].dst = h->buf.workspace + dst_off; a.job[0].src_row_stride = x_rs;
  a.job[0].src_col_stride = 1; a.job[0].cols = h->cfg.obs_dim; a.job[0].ld = h->Sp;
  const long n = (long)batch * h->Sp;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024), 1), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// The small-batch path stages the B x K input of every layer in LDS (K = obs_dim, then hidden_dim): whether the whole
// layer chain fits is decided before its first launch, and a chain that does not takes the batched path instead.
constexpr size_t SMALL_FWD_LDS_BYTES = 64 * 1024;
bool small_fwd_fits(const porl_iql* h, int batch) {
  return batch >= 1 && batch <= SMALL_FWD_MAX_B &&
         sizeof(float) * (size_t)batch * std::max(h->cfg.obs_dim, h->cfg.hidden_dim) <= SMALL_FWD_LDS_BYTES;
}

// One Linear layer of up to 2 networks on a handful of rows (kernels.hpp: small_fwd_kernel).
int small_fwd(int nnets, const float* const* Wt, const float* const* bias, const float* const* X, const long* ldx,
              float* const* Y, const long* ldy, int N, int K, int B, int act, hipStream_t s) {
  SmallFwdArgs a{};
  for (int i = 0; i < nnets; ++i) { a.W[i] = Wt[i]; a.bias[i] = bias[i]; a.X[i] = X[i]; a.ldx[i] = ldx[i]; a.Y[i] = Y[i]; a.ldy[i] = ldy[i]; }
  a.N = N; a.K = K; a.B = B; a.act = act;
  const size_t lds = sizeof(float) * (size_t)B * K;
  if (lds > SMALL_FWD_LDS_BYTES) PORL_FAIL(PORL_ERR_UNSUPPORTED, "small-batch path: B*K too large");
  ProfScope ps("small_fwd_kernel", s, 2.0 * nnets * B * N * K, 4.0 * nnets * ((double)N * K + B * (N + K)));
  hipLaunchKernelGGL(small_fwd_kernel, dim3(std::min(cdiv(N, 4), 1024), nnets), dim3(256), lds, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// The one launch both goal-conditioned loaders end in.
int stage_pairs(porl_iql* h, PairStageArgs& a, int batch, int S, int G, int A, int64_t* start_out, int64_t* goal_out,
                void* stream) {
  DevGuard _dg(h->device);
  float* W = h->buf.workspace;
  const int slot = next_slot(h);
  a.batch = batch; a.S = S; a.G = G; a.A = A; a.Sp = h->Sp; a.Dp = h->Dp;
  a.xs = W + h->ws.xs_slot[slot]; a.xt = W + h->ws.xt_slot[slot]; a.w = W + h->ws.pol_w;
  a.start_out = reinterpret_cast<long long*>(start_out); a.goal_out = reinterpret_cast<long long*>(goal_out);
  {
    g_phase = "B0.";
    ProfScope ps("stage_pairs_kernel", (hipStream_t)stream, 0.0, 8.0 * batch * (S + G + A + 1));
    hipLaunchKernelGGL(stage_pairs_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
    g_phase = "";
  }
  PORL_HIP(hipGetLastError());
  iql_batch_loaded(h, batch, true, true);
  return PORL_OK;
}

}  // namespace

// =====================================================================================================
extern "C" {

int porl_iql_create(const porl_iql_cfg* c, porl_iql** out) {
  if (!c || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (c->obs_dim < 1 || c->pol_out_dim < 1 || c->hidden_dim < 1 || c->max_batch < 1)
    PORL_FAIL(PORL_ERR_INVALID, "dimensions must be positive");
  if (c->n_hidden < 1 || c->n_hidden > PORL_MAX_HIDDEN) PORL_FAIL(PORL_ERR_INVALID, "n_hidden must be in [1,%d]", PORL_MAX_HIDDEN);
  if (c->pol_out_dim > 64 * NLL_MAX_COLS_PER_LANE) PORL_FAIL(PORL_ERR_UNSUPPORTED, "pol_out_dim > %d", 64 * NLL_MAX_COLS_PER_LANE);
  if (c->layer_norm && c->hidden_dim > 256 * LN_MAX_COLS)
    PORL_FAIL(PORL_ERR_UNSUPPORTED, "layer_norm with hidden_dim > %d", 256 * LN_MAX_COLS);
  porl_iql* h = new porl_iql();
  h->cfg = *c;
  const int S = c->obs_dim, D = c->pol_out_dim, H = c->hidden_dim, L = c->n_hidden, B = c->max_batch;
  int64_t cur = 0;
  layout_mlp(h->v[0], h->t_vf, cur, S, H, L, 1, c->layer_norm != 0);
  layout_mlp(h->v[1], h->t_vf, cur, S, H, L, 1, c->layer_norm != 0);
  h->n_vf = cur;
  cur = 0;
  h->logstd_off = add_tensor(h->t_pol, cur, 0, D);
  layout_mlp(h->pol, h->t_pol, cur, S, H, L, D, false);
  h->n_pol = cur;

  h->Sp = (int)ru4(S); h->Dp = (int)ru4(D); h->Hp = (int)ru4(H);
  h->parts_max = 0;
  for (int tile = 0; tile < TILE_COUNT; ++tile) h->parts_max = std::max(h->parts_max, head_parts(H, tile));
  Workspace& w = h->ws;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += ru4(n); return r; };
  const int64_t BH = (int64_t)B * h->Hp;
  for (int k = 0; k < PORL_IQL_SLOTS; ++k) {
    w.xs_slot[k] = take((int64_t)B * h->Sp); w.xt_slot[k] = take((int64_t)B * h->Dp); w.target_v_slot[k] = take(B);
  }
  w.xn = take((int64_t)B * h->Sp);
  w.rew = take(B); w.term = take(B);
  for (int i = 0; i < 2; ++i) {
    for (int l = 0; l < L; ++l) w.act_v[i][l] = take(BH);
    w.act_t[i][0] = take(BH); w.act_t[i][1] = take(BH);
    w.act_q[i][0] = take(BH); w.act_q[i][1] = take(BH);
    w.hp_q[i] = take((int64_t)h->parts_max * B);
    w.dz_v[i][0] = take(BH); w.dz_v[i][1] = take(BH);
    w.hp_t[i] = take((int64_t)h->parts_max * B); w.hp_v[i] = take((int64_t)h->parts_max * B);
    w.dv[i] = take(B);
  }
  for (int l = 0; l < L; ++l) w.act_p[l] = take(BH);
  w.dz_p[0] = take(BH); w.dz_p[1] = take(BH);
  w.dmu = take((int64_t)B * h->Dp);
  w.slab_mean = take((int64_t)SK_MAX * B * h->Dp);
  w.slab_a = take(slab_floats(*c, SLAB_TWIN0) + slab_floats(*c, SLAB_TWIN1));
  w.slab_b = take(slab_floats(*c, SLAB_OUT));
  w.slab_pa = take(slab_floats(*c, SLAB_POLICY));
  const int nblk = cdiv(B, NLL_ROWS_PER_BLOCK);
  w.part_loss = take(nblk); w.part_min = take(nblk); w.part_dls = take((int64_t)nblk * D);
  for (int i = 0; i < 2; ++i) { w.head_part[i] = take((int64_t)cdiv(B, HEAD_ROWS_PER_BLOCK) * H); w.head_db[i] = take(cdiv(B, HEAD_ROWS_PER_BLOCK)); }
  w.head_loss = take(cdiv(B, HEAD_ROWS_PER_BLOCK));
  if (c->layer_norm) {
    const int nln = cdiv(B, LN_ROWS_PER_BLOCK);
    for (int i = 0; i < 2; ++i) {
      for (int l = 0; l < L; ++l) { w.xhat_v[i][l] = take(BH); w.rstd_v[i][l] = take(B); }
      w.ln_dg[i] = take((int64_t)nln * H); w.ln_db[i] = take((int64_t)nln * H); w.ln_dh[i] = take((int64_t)nln * H);
    }
  }
  w.pol_w = take(B);
  w.total = o;
  *out = h;
  return PORL_OK;
}

void porl_iql_destroy(porl_iql* h) { delete h; }

int64_t porl_iql_group_floats(const porl_iql* h, int group) { return !h ? 0 : (group == 0 ? h->n_vf : h->n_pol); }
int32_t porl_iql_group_tensors(const porl_iql* h, int group) {
  return !h ? 0 : (int32_t)(group == 0 ? h->t_vf.size() : h->t_pol.size());
}
int porl_iql_tensor_info(const porl_iql* h, int group, int index, int64_t* offset, int32_t* rows, int32_t* cols) {
  if (!h || group < 0 || group > 1) PORL_FAIL(PORL_ERR_INVALID, "bad group");
  const auto& v = group == 0 ? h->t_vf : h->t_pol;
  if (index < 0 || index >= (int)v.size()) PORL_FAIL(PORL_ERR_INVALID, "tensor index out of range");
  if (offset) *offset = v[index].off;
  if (rows) *rows = v[index].rows;
  if (cols) *cols = v[index].cols;
  return PORL_OK;
}
int64_t porl_iql_workspace_floats(const porl_iql* h) { return h ? h->ws.total : 0; }

int porl_iql_bind(porl_iql* h, const porl_iql_buffers* b) {
  if (!h || !b) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  const void* ptrs[] = {b->params_vf, b->params_tgt, b->params_pol, b->grads_vf, b->grads_pol, b->adam_m_vf,
                        b->adam_v_vf, b->adam_m_pol, b->adam_v_pol, b->workspace, b->stats};
  for (const void* p : ptrs) {
    if (!p) PORL_FAIL(PORL_ERR_INVALID, "null buffer");
    if (!aligned16(p)) PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  }
  h->buf = *b;
  h->bound = true;
  h->device = device_of(b->workspace);
  h->batch = 0;
  return PORL_OK;
}

int porl_iql_set_mode(porl_iql* h, int32_t mode) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (mode & ~(PORL_IQL_MODE_TWO_SLOTS | PORL_IQL_MODE_FOLD_COMBINE | PORL_IQL_MODE_SHORT_BLOCKS)) PORL_FAIL(PORL_ERR_INVALID, "unknown mode bits");
  if (h->fin_v_pending || h->fin_p_pending) PORL_FAIL(PORL_ERR_INVALID, "a backward pass is waiting for its apply call");
  h->mode = mode;
  return PORL_OK;
}

int porl_iql_set_stats(porl_iql* h, float* stats) {
  PORL_TRY(check_ready(h, false));
  if (!stats) PORL_FAIL(PORL_ERR_INVALID, "null stats");
  h->buf.stats = stats;
  return PORL_OK;
}

int porl_iql_adam_plan(const porl_iql* h, int group, int32_t out[6]) {
  if (!h || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (group < 0 || group > 1) PORL_FAIL(PORL_ERR_INVALID, "bad group");
  std::copy(h->adam_plan[group], h->adam_plan[group] + 6, out);
  return PORL_OK;
}

int porl_iql_tune_set(porl_iql* h, const char* key, int value) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  return tune_apply(h->tune, key, value);
}

// ---- loaders: every argument is judged before the first HIP call and before the slot moves ---------------------------
int porl_iql_load_batch(porl_iql* h, int32_t batch, const float* obs, int64_t obs_rs, const float* next_obs,
                        int64_t next_rs, const float* rew, int64_t rew_rs, const float* term, int64_t term_rs,
                        const float* pol_target, int64_t pt_rs, void* stream) {
  PORL_TRY(check_ready(h, false));
  PORL_TRY(check_batch(h, batch));
  if (!obs || !next_obs || !rew || !term) PORL_FAIL(PORL_ERR_INVALID, "null batch tensor");
  DevGuard _dg(h->device);
  float* W = h->buf.workspace;
  const int slot = next_slot(h);
  PackArgs a{};
  a.rows = batch;
  auto job = [&](const float* src, int64_t rs, float* dst, int cols, int ld) {
    PackJob& j = a.job[a.njobs++];
    j.src = src; j.dst = dst; j.src_row_stride = rs; j.src_col_stride = 1; j.cols = cols; j.ld = ld;
  };
  job(obs, obs_rs, W + h->ws.xs_slot[slot], h->cfg.obs_dim, h->Sp);
  job(next_obs, next_rs, W + h->ws.xn, h->cfg.obs_dim, h->Sp);
  job(rew, rew_rs, W + h->ws.rew, 1, 1);
  job(term, term_rs, W + h->ws.term, 1, 1);
  if (pol_target) job(pol_target, pt_rs, W + h->ws.xt_slot[slot], h->cfg.pol_out_dim, h->Dp);
  const long n = (long)batch * std::max(h->Sp, h->Dp);
  dim3 grid((unsigned)std::min<long>((n + 255) / 256, 1024), a.njobs);
  hipLaunchKernelGGL(pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  iql_batch_loaded(h, batch, pol_target != nullptr);
  return PORL_OK;
}

int porl_iql_load_batch_sampled(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                                int32_t act_dim, int32_t target_is_action, uint64_t seed, uint64_t step,
                                int64_t* idx_out, void* stream) {
  PORL_TRY(check_ready(h, false));
  PORL_TRY(check_batch(h, batch));
  PORL_TRY(check_replay_rows(h, batch, rows, row_stride, n_rows, act_dim, target_is_action));
  DevGuard _dg(h->device);
  const int S = h->cfg.obs_dim, D = h->cfg.pol_out_dim;
  float* W = h->buf.workspace;
  const int slot = next_slot(h);
  SampledBatchArgs a{};
  a.rows = rows; a.row_stride = (long)row_stride; a.n_rows = n_rows;
  a.batch = batch; a.S = S; a.A = act_dim; a.D = D; a.Sp = h->Sp; a.Dp = h->Dp;
  a.hb = feistel_half_bits(n_rows); a.target_is_action = target_is_action;
  a.seed = seed; a.step = step;
  a.xs = W + h->ws.xs_slot[slot]; a.xn = W + h->ws.xn; a.xt = W + h->ws.xt_slot[slot]; a.rew = W + h->ws.rew; a.term = W + h->ws.term;
  a.idx_out = idx_out;
  {
    g_phase = "V1.";
    ProfScope ps("sampled_batch_kernel", (hipStream_t)stream, 0.0, 8.0 * batch * (2 * S + 2 + act_dim));
    hipLaunchKernelGGL(sampled_batch_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
    g_phase = "";
  }
  PORL_HIP(hipGetLastError());
  iql_batch_loaded(h, batch, true);
  return PORL_OK;
}

int porl_iql_load_batch_indexed(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                                const int64_t* idx, int32_t state_dim, int32_t act_dim, int32_t target_is_action,
                                int32_t clamp_target_gt8, const float* obs_feat, int64_t obs_rs, const float* next_feat,
                                int64_t next_rs, void* stream) {
  PORL_TRY(check_ready(h, false));
  PORL_TRY(check_batch(h, batch));
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (!idx) PORL_FAIL(PORL_ERR_INVALID, "null idx");
  if (n_rows < 1) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld must be at least 1", (long long)n_rows);
  const int F = h->cfg.obs_dim, D = h->cfg.pol_out_dim;
  if (state_dim < 1 || act_dim < 0) PORL_FAIL(PORL_ERR_INVALID, "state_dim %d / act_dim %d out of range", state_dim, act_dim);
  if (row_stride < 2 * (int64_t)state_dim + 2 + act_dim)
    PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld shorter than 2*state_dim+2+act_dim = %lld", (long long)row_stride,
              2 * (long long)state_dim + 2 + act_dim);
  if ((obs_feat == nullptr) != (next_feat == nullptr))
    PORL_FAIL(PORL_ERR_INVALID, "obs_feat and next_feat must be given together (%s is null)", obs_feat ? "next_feat" : "obs_feat");
  if (obs_feat && obs_rs < F) PORL_FAIL(PORL_ERR_INVALID, "obs_rs %lld below obs_dim %d", (long long)obs_rs, F);
  if (next_feat && next_rs < F) PORL_FAIL(PORL_ERR_INVALID, "next_rs %lld below obs_dim %d", (long long)next_rs, F);
  if (!obs_feat && state_dim != F)
    PORL_FAIL(PORL_ERR_INVALID, "state_dim %d != obs_dim %d and no feature matrices given", state_dim, F);
  if (target_is_action ? D != act_dim : D != state_dim)
    PORL_FAIL(PORL_ERR_INVALID, "policy target width mismatch: pol_out_dim %d vs %s %d", D, target_is_action ? "act_dim" : "state_dim",
              target_is_action ? act_dim : state_dim);
  DevGuard _dg(h->device);
  float* W = h->buf.workspace;
  const int slot = next_slot(h);
  IndexedBatchArgs a{};
  a.rows = rows; a.row_stride = (long)row_stride; a.idx = idx;
  a.batch = batch; a.S = state_dim; a.F = F; a.D = D; a.Sp = h->Sp; a.Dp = h->Dp;
  a.target_is_action = target_is_action; a.clamp_target = clamp_target_gt8;
  a.obs_feat = obs_feat; a.obs_rs = (long)obs_rs; a.next_feat = next_feat; a.next_rs = (long)next_rs;
  a.xs = W + h->ws.xs_slot[slot]; a.xn = W + h->ws.xn; a.xt = W + h->ws.xt_slot[slot]; a.rew = W + h->ws.rew; a.term = W + h->ws.term;
  {
    g_phase = "V1.";
    ProfScope ps("indexed_batch_kernel", (hipStream_t)stream, 0.0, 4.0 * batch * (2.0 * h->Sp + h->Dp + 2) * 2.0);
    hipLaunchKernelGGL(indexed_batch_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
    g_phase = "";
  }
  PORL_HIP(hipGetLastError());
  iql_batch_loaded(h, batch, true);
  return PORL_OK;
}

int porl_iql_load_batch_cat(porl_iql* h, int32_t batch, const float* obs, int64_t obs_rs, const float* goals, int64_t goals_rs,
                            int32_t goal_dim, const float* actions, int64_t act_rs, void* stream) {
  PORL_TRY(check_ready(h, false));
  PORL_TRY(check_batch(h, batch));
  if (!obs) PORL_FAIL(PORL_ERR_INVALID, "null obs");
  if (!goals) PORL_FAIL(PORL_ERR_INVALID, "null goals");
  if (!actions) PORL_FAIL(PORL_ERR_INVALID, "null actions");
  if (goal_dim < 1 || goal_dim >= h->cfg.obs_dim)
    PORL_FAIL(PORL_ERR_INVALID, "goal_dim %d outside [1, obs_dim %d): the engine's input is [obs | goal]", goal_dim, h->cfg.obs_dim);
  const int S = h->cfg.obs_dim - goal_dim, A = h->cfg.pol_out_dim;
  if (batch > 1 && obs_rs < S) PORL_FAIL(PORL_ERR_INVALID, "obs_rs %lld below the %d observation columns", (long long)obs_rs, S);
  if (batch > 1 && goals_rs < goal_dim) PORL_FAIL(PORL_ERR_INVALID, "goals_rs %lld below goal_dim %d", (long long)goals_rs, goal_dim);
  if (batch > 1 && act_rs < A) PORL_FAIL(PORL_ERR_INVALID, "act_rs %lld below pol_out_dim %d", (long long)act_rs, A);
  PairStageArgs a{};
  a.mode = PAIR_DENSE; a.n_rows = batch;
  a.s = PairSrc{obs, (long long)obs_rs, 0}; a.g = PairSrc{goals, (long long)goals_rs, 0}; a.a = PairSrc{actions, (long long)act_rs, 0};
  return stage_pairs(h, a, batch, S, goal_dim, A, nullptr, nullptr, stream);
}

int porl_iql_load_batch_pairs(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                              int32_t state_dim, int32_t act_dim, int32_t goal_col, int32_t goal_dim, const int64_t* start,
                              const int64_t* goal, const int64_t* ep_starts, const int64_t* ep_lengths, int64_t n_episodes,
                              uint64_t seed, uint64_t step, int64_t* start_out, int64_t* goal_out, void* stream) {
  PORL_TRY(check_ready(h, false));
  PORL_TRY(check_batch(h, batch));
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (n_rows < 1 || n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^40]", (long long)n_rows);
  if (state_dim < 1 || act_dim < 1 || goal_dim < 1)
    PORL_FAIL(PORL_ERR_INVALID, "state_dim %d / act_dim %d / goal_dim %d must be positive", state_dim, act_dim, goal_dim);
  const int64_t S = state_dim, state_part = 2 * S + 2;
  if (row_stride < state_part + act_dim || row_stride > (int64_t(1) << 26))
    PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld: a row is 2*state_dim+2+act_dim = %lld floats", (long long)row_stride,
              (long long)(state_part + act_dim));
  if (goal_col < 0) PORL_FAIL(PORL_ERR_INVALID, "goal_col %d must not be negative", goal_col);
  if ((int64_t)goal_col + goal_dim > state_part)
    PORL_FAIL(PORL_ERR_INVALID, "goal_col %d + goal_dim %d runs past the state part of a row (2*state_dim+2 = %lld)", goal_col,
              goal_dim, (long long)state_part);
  if (S + goal_dim != h->cfg.obs_dim)
    PORL_FAIL(PORL_ERR_INVALID, "state_dim %d + goal_dim %d != obs_dim %d", state_dim, goal_dim, h->cfg.obs_dim);
  if (act_dim != h->cfg.pol_out_dim) PORL_FAIL(PORL_ERR_INVALID, "act_dim %d != pol_out_dim %d", act_dim, h->cfg.pol_out_dim);
  if (goal && !start) PORL_FAIL(PORL_ERR_INVALID, "null start (goal is given)");
  if ((ep_starts == nullptr) != (ep_lengths == nullptr))
    PORL_FAIL(PORL_ERR_INVALID, "ep_starts and ep_lengths are given together (%s is null)", ep_starts ? "ep_lengths" : "ep_starts");
  if (ep_starts && start) PORL_FAIL(PORL_ERR_INVALID, "an episode table and start are both given: the pairs are drawn or named, not both");
  if (ep_starts && (n_episodes < 1 || n_episodes > n_rows))
    PORL_FAIL(PORL_ERR_INVALID, "n_episodes %lld outside [1, n_rows]", (long long)n_episodes);
  if (!start && !ep_starts && n_rows < batch)
    PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld below batch %d: the draw takes distinct rows", (long long)n_rows, batch);
  PairStageArgs a{};
  a.n_rows = n_rows;
  a.s = PairSrc{rows, (long long)row_stride, 0};
  a.g = PairSrc{rows, (long long)row_stride, goal_col};
  a.a = PairSrc{rows, (long long)row_stride, (int)state_part};
  if (start) {
    a.mode = PAIR_GIVEN;
    a.start = reinterpret_cast<const long long*>(start); a.goal = reinterpret_cast<const long long*>(goal);
  } else if (ep_starts) {
    a.mode = PAIR_HINDSIGHT;
    a.ep_starts = reinterpret_cast<const long long*>(ep_starts); a.ep_lengths = reinterpret_cast<const long long*>(ep_lengths);
    a.E = n_episodes; a.key = ep_sm64(seed ^ ep_sm64(step));
  } else {
    a.mode = PAIR_PERMUTED;
    a.seed = seed; a.step = step; a.hb = feistel_half_bits(n_rows);
  }
  return stage_pairs(h, a, batch, state_dim, goal_dim, act_dim, start_out, goal_out, stream);
}

// ---- the four phase calls -----------------------------------------------------------------------------------------------
int porl_iql_value_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, false, "porl_iql_value_backward")); DevGuard _dg(h->device);
  const bool fold = (h->mode & PORL_IQL_MODE_FOLD_COMBINE) != 0;
  h->fin_v = ReduceArgs{};
  PORL_TRY(value_backward_impl(h, hp, (hipStream_t)stream, fold ? &h->fin_v : nullptr));
  h->fin_v_pending = fold;
  return PORL_OK;
}

int porl_iql_value_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, false, hp)); DevGuard _dg(h->device);
  const int rc = value_adam(h, hp, (hipStream_t)stream, h->fin_v_pending ? &h->fin_v : nullptr);
  h->fin_v_pending = false;
  return rc;
}

int porl_iql_policy_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, false, hp)); DevGuard _dg(h->device);
  const int rc = policy_adam(h, hp, (hipStream_t)stream, h->fin_p_pending ? &h->fin_p : nullptr, "P9.");
  h->fin_p_pending = false;
  return rc;
}

// The part of the policy step that does not depend on the value networks: the policy MLP's forward on the loaded
// observations.  In data-parallel mode it runs while the value-gradient all-reduce is on the wire.
int porl_iql_policy_prefetch(porl_iql* h, void* stream) {
  PORL_TRY(check_ready(h, true));
  PORL_TRY(need_kind(h, false, "porl_iql_policy_prefetch"));
  PORL_TRY(need_pol_target(h));
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    const FwdNet f = policy_fwd_net(h, l, h->ws.xs_slot[h->slot]);
    PORL_TRY(fwd_hidden_layer(h, &f, 1, h->batch, l == 0 ? S : H, l == L - 1, &parts, false, s));
  }
  PORL_TRY(policy_mean_slabs(h, h->batch, &h->pol_nslab, false, s));
  h->pol_prefetched = true;
  return PORL_OK;
}

// Forward half only; a second call for the same batch does nothing.
int porl_iql_policy_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, false, "porl_iql_policy_forward")); DevGuard _dg(h->device);
  PORL_TRY(need_pol_target(h));
  return h->pol_fwd_done ? PORL_OK : policy_forward_half(h, hp, (hipStream_t)stream);
}

int porl_iql_policy_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp));
  // on a goal-conditioned batch this call only completes porl_iql_bc_forward: the joint update's forward half needs V nets
  if (h->pair_batch && !h->pol_fwd_done) PORL_TRY(need_kind(h, false, "porl_iql_policy_backward without porl_iql_bc_forward"));
  DevGuard _dg(h->device);
  const bool fold = (h->mode & PORL_IQL_MODE_FOLD_COMBINE) != 0;
  h->fin_p = ReduceArgs{};
  PORL_TRY(policy_backward_impl(h, hp, (hipStream_t)stream, fold ? &h->fin_p : nullptr));
  h->fin_p_pending = fold;
  return PORL_OK;
}

// The whole update in one call.  Same arithmetic as the four phase calls; the two slab / partial-sum combines are
// folded into the Adam launches instead of running as launches of their own.
int porl_iql_step(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, false, "porl_iql_step")); DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs fin{};
  PORL_TRY(value_backward_impl(h, hp, s, h->tune.iql_fold ? &fin : nullptr));
  PORL_TRY(value_adam(h, hp, s, &fin));
  fin = ReduceArgs{};
  PORL_TRY(policy_backward_impl(h, hp, s, h->tune.iql_fold ? &fin : nullptr));
  return policy_adam(h, hp, s, &fin, "P9.");
}

// Policy-only step (SORL.policy_update, reference agent/sorl.py:154-176 + the TD target of sorl.py:85-89): the value
// nets are read, never written.  Forward half = five forward-only nets per layer in one launch, policy_weight_kernel,
// mean, NLL; then the gradient half and Adam of the ordinary policy phase.  2 L + 5 launches at n_hidden = L (9 at L = 2;
// the joint update takes 14, each plus the minibatch load).
int porl_iql_policy_only_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, false, "porl_iql_policy_only_forward")); DevGuard _dg(h->device);
  h->pol_fwd_done = false;             // a forward half of the joint update's policy phase does not stand in for this one
  PORL_TRY(need_pol_target(h));
  return policy_only_forward_half(h, hp, (hipStream_t)stream);
}

// porl_iql_policy_only_forward + porl_iql_policy_backward + porl_iql_policy_apply in one call, the combine folded into
// the Adam launch (single-GPU update; batch must have been loaded).  stats[1] = g_loss, stats[2] = min NLL; stats[0],
// grads_vf, adam_*_vf, params_vf and params_tgt are not written.
int porl_iql_policy_only_step(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, false, "porl_iql_policy_only_step")); DevGuard _dg(h->device);
  PORL_TRY(need_pol_target(h));
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs fin{};
  PORL_TRY(policy_only_forward_half(h, hp, s));
  PORL_TRY(policy_gradient_half(h, s, h->tune.iql_fold ? &fin : nullptr));
  return policy_adam(h, hp, s, &fin, "O9.");
}

// Goal-conditioned behaviour cloning (reference agent/por.py:178-183: policy(concat[obs, goal]), mean(-log_prob(actions)),
// Adam) on a batch staged by porl_iql_load_batch_cat / porl_iql_load_batch_pairs.  L + 2 forward launches (the policy net
// alone, mean, NLL with unit weights), the gradient half of the ordinary policy phase, Adam with the combine folded in:
// 2 L + 4 launches at n_hidden = L (8 at L = 2), plus the load.  Group 0, the target net and stats[0] are not touched.
int porl_iql_bc_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, true, "porl_iql_bc_forward")); DevGuard _dg(h->device);
  return bc_forward_half(h, hp, (hipStream_t)stream);
}

int porl_iql_bc_step(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(iql_enter(h, true, hp)); PORL_TRY(need_kind(h, true, "porl_iql_bc_step")); DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs fin{};
  PORL_TRY(bc_forward_half(h, hp, s));
  PORL_TRY(policy_gradient_half(h, s, h->tune.iql_fold ? &fin : nullptr));
  return policy_adam(h, hp, s, &fin, "B9.");
}

// ---- forward-only: TwinV.both, GaussianPolicy.forward / act --------------------------------------------------------------
int porl_iql_forward_value(porl_iql* h, int which, const float* x, int64_t x_rs, int32_t batch, float* v1_out,
                           float* v2_out, void* stream) {
  PORL_TRY(check_ready(h, false));
  if (!v1_out || !v2_out) PORL_FAIL(PORL_ERR_INVALID, "null output");
  PORL_TRY(check_batch(h, batch));
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* P = which ? h->buf.params_tgt : h->buf.params_vf;
  if (small_fwd_fits(h, batch) && !h->cfg.layer_norm && x) {
    // inference-sized batch: 3 GEMV launches straight from the caller's rows (no staging copy, no split-K)
    const float* in[2] = {x, x};
    long ldin[2] = {(long)x_rs, (long)x_rs};
    for (int l = 0; l <= L; ++l) {
      const float* Wt[2] = {P + h->v[0].w[l], P + h->v[1].w[l]};
      const float* bs[2] = {P + h->v[0].b[l], P + h->v[1].b[l]};
      float* out[2];
      long ldo[2];
      for (int i = 0; i < 2; ++i) {
        out[i] = l == L ? (i ? v2_out : v1_out) : W + ws.act_t[i][l & 1];
        ldo[i] = l == L ? 1 : h->Hp;
      }
      PORL_TRY(small_fwd(2, Wt, bs, in, ldin, out, ldo, l == L ? 1 : H, l == 0 ? S : H, batch, l == L ? ACT_NONE : ACT_RELU, s));
      for (int i = 0; i < 2; ++i) { in[i] = out[i]; ldin[i] = ldo[i]; }
    }
    return PORL_OK;
  }
  // uses the s' staging buffer and the target scratch activations; invalidates a loaded minibatch
  PORL_TRY(pack_x(h, x, x_rs, batch, ws.xn, s));
  h->batch = 0;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    const FwdNet nets[2] = {twin_fwd_net(h, P, 0, l, ws.xn, ws.act_t[0], false, ws.hp_t[0]),
                            twin_fwd_net(h, P, 1, l, ws.xn, ws.act_t[1], false, ws.hp_t[1])};
    PORL_TRY(fwd_hidden_layer(h, nets, 2, batch, l == 0 ? S : H, l == L - 1, &parts, false, s));
  }
  hipLaunchKernelGGL(head_finish_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, s, W + ws.hp_t[0], W + ws.hp_t[1],
                     P + h->v[0].b[L], P + h->v[1].b[L], parts, batch, v1_out, v2_out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iql_forward_policy(porl_iql* h, const float* x, int64_t x_rs, int32_t batch, float* mean_out,
                            int64_t mean_rs, void* stream) {
  PORL_TRY(check_ready(h, false));
  if (!mean_out) PORL_FAIL(PORL_ERR_INVALID, "null output");
  PORL_TRY(check_batch(h, batch));
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim;
  float* W = h->buf.workspace;
  const float* P = h->buf.params_pol;
  if (small_fwd_fits(h, batch) && x) {
    const float* in[1] = {x};
    long ldin[1] = {(long)x_rs};
    for (int l = 0; l <= L; ++l) {
      const float* Wt[1] = {P + h->pol.w[l]};
      const float* bs[1] = {P + h->pol.b[l]};
      // hidden activations go to the TARGET-net scratch: the policy-phase buffers may still be in use by a pipelined
      // update on another stream, the value-phase scratch is ordered on the caller's stream
      float* out[1] = {l == L ? mean_out : W + h->ws.act_t[0][l & 1]};
      long ldo[1] = {l == L ? (long)mean_rs : (long)h->Hp};
      const int act = l < L ? ACT_RELU : (h->cfg.pol_tanh ? ACT_TANH : ACT_NONE);
      PORL_TRY(small_fwd(1, Wt, bs, in, ldin, out, ldo, l == L ? D : H, l == 0 ? S : H, batch, act, s));
      in[0] = out[0]; ldin[0] = ldo[0];
    }
    return PORL_OK;
  }
  PORL_TRY(pack_x(h, x, x_rs, batch, h->ws.xn, s));
  h->batch = 0;
  for (int l = 0; l < L; ++l) {
    const FwdNet f = policy_fwd_net(h, l, h->ws.xn);
    PORL_TRY(fwd_hidden_layer(h, &f, 1, batch, l == 0 ? S : H, false, nullptr, false, s));
  }
  int nslab = 1;
  PORL_TRY(policy_mean_slabs(h, batch, &nslab, false, s));
  const long n = (long)batch * D;
  hipLaunchKernelGGL(mean_finish_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024)), dim3(256), 0, s,
                     W + h->ws.slab_mean, nslab, (long)batch * h->Dp, batch, D, h->Dp, P + h->pol.b[L],
                     h->cfg.pol_tanh, mean_out, (long)mean_rs);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// One pipelined update from ONE call: what porl_amd/agent/_iql.py:_full_update issues in signal mode on a single GPU —
// value phase on `main_stream`, policy phase on `side_stream`, ordered by the three counters — without a round trip
// through the caller's language per phase (the Python sequence costs ~110 us of host time per update, which is what
// bounds small configurations; this entry is ~20 launches back to back).  Same launches, same order per stream, same
// results as the phase calls.
int porl_iql_update_pipelined(porl_iql* h, const porl_iql_hyper* hp, int32_t batch, const float* rows, int64_t row_stride,
                              int64_t n_rows, int32_t act_dim, int32_t target_is_action, uint64_t seed, uint64_t step,
                              void* sig_value, void* sig_fwd, void* sig_policy, uint64_t seq, uint64_t wait_policy_seq,
                              uint64_t wait_fwd_seq, int32_t write_policy, void* main_stream, void* side_stream) {
  PORL_TRY(iql_enter(h, false, hp));
  if (!sig_value || !sig_fwd || !sig_policy || seq < 1) PORL_FAIL(PORL_ERR_INVALID, "three signal counters and seq >= 1 are required");
  if (main_stream == side_stream) PORL_FAIL(PORL_ERR_INVALID, "the two phases need two streams");
  if (!(h->mode & PORL_IQL_MODE_TWO_SLOTS) || !(h->mode & PORL_IQL_MODE_FOLD_COMBINE))
    PORL_FAIL(PORL_ERR_INVALID, "pipelined updates need PORL_IQL_MODE_TWO_SLOTS | PORL_IQL_MODE_FOLD_COMBINE");
  // reject bad minibatch arguments before anything is enqueued (porl_iql_load_batch_sampled checks them again)
  PORL_TRY(check_batch(h, batch));
  PORL_TRY(check_replay_rows(h, batch, rows, row_stride, n_rows, act_dim, target_is_action));
  DevGuard _dg(h->device);
  // the staging slot loaded next was last read by the policy phase PORL_IQL_SLOTS updates ago
  if (wait_policy_seq) PORL_TRY(porl_signal_wait_ge(sig_policy, wait_policy_seq, main_stream));
  PORL_TRY(porl_iql_load_batch_sampled(h, batch, rows, row_stride, n_rows, act_dim, target_is_action, seed, step, nullptr, main_stream));
  PORL_TRY(porl_iql_value_backward(h, hp, main_stream));
  // the previous update's policy phase has read the old value nets
  if (wait_fwd_seq) PORL_TRY(porl_signal_wait_ge(sig_fwd, wait_fwd_seq, main_stream));
  PORL_TRY(porl_iql_value_apply(h, hp, main_stream));
  PORL_TRY(porl_signal_write(sig_value, seq, main_stream));
  PORL_TRY(porl_signal_wait_ge(sig_value, seq, side_stream));
  PORL_TRY(porl_iql_policy_forward(h, hp, side_stream));
  PORL_TRY(porl_signal_write(sig_fwd, seq, side_stream));
  PORL_TRY(porl_iql_policy_backward(h, hp, side_stream));
  PORL_TRY(porl_iql_policy_apply(h, hp, side_stream));
  if (write_policy) PORL_TRY(porl_signal_write(sig_policy, seq, side_stream));
  return PORL_OK;
}

}  // extern "C"
