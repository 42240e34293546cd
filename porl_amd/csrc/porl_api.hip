// libporl_hip.so — C ABI (include/porl_hip.h) over the gfx950 kernels.  Host-side planning only:
// parameter/workspace layouts, the launch sequence of one update, and the group/tile/split-K choices
// that keep 256 CUs busy with 1024-wide MLPs.  No device allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/porl_hip.h"
#include "gemm_f32.hpp"
#include "gemm_bf16.hpp"
#include "kernels.hpp"
#include "l0_fwd.hpp"
#include "skinny.hpp"
#include "iqn.hpp"
#include "qnet_fused.hpp"
#include "per_tree.hpp"
#include "dist_losses.hpp"
#include "online.hpp"
#include "per_online.hpp"
#include "bcq_mask.hpp"
#include "astar.hpp"
#include "episodes.hpp"
#include "partition.hpp"

using namespace porl;

namespace {

thread_local std::string g_err;

#define PORL_FAIL(code, ...)                         \
  do {                                               \
    char _b[512];                                    \
    snprintf(_b, sizeof _b, __VA_ARGS__);            \
    g_err = _b;                                      \
    return (code);                                   \
  } while (0)

#define PORL_HIP(expr)                                                        \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      g_err = std::string(#expr) + ": " + hipGetErrorString(_e);              \
      return (int)_e;                                                         \
    }                                                                         \
  } while (0)

#define PORL_TRY(expr)          \
  do {                          \
    int _r = (expr);            \
    if (_r != 0) return _r;     \
  } while (0)

// Every entry point launches on the device that owns its buffers, whatever the calling thread's current device is:
// handles remember the ordinal of their workspace at bind time, stateless entry points look it up from a pointer.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(int dev) {
    if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};
int device_of(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

// Raises Kernel's dynamic-LDS limit above the 64 KiB default, once per process: on the first call, and again only if
// that call failed.  One flag per kernel, so a launch site that needs several raised lists them one after another.
template <auto Kernel>
int dyn_lds_once(int bytes) {
  static bool done = false;
  if (!done) {
    PORL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done = true;
  }
  return 0;
}

// ---- optional per-launch timing with HIP events (bench.py's roofline leg) ---------------------------
struct ProfRec { int label; hipEvent_t e0, e1; double flops, bytes; };
struct ProfState {
  bool on = false;
  std::vector<std::string> labels;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  size_t pool_used = 0;
  hipEvent_t get() {
    if (pool_used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
    return pool[pool_used++];
  }
  int label_id(const std::string& s) {
    for (size_t i = 0; i < labels.size(); ++i) if (labels[i] == s) return (int)i;
    labels.push_back(s);
    return (int)labels.size() - 1;
  }
} g_prof;

const char* g_phase = "";     // prefix of the profile labels: which launch of the update step this is (profiling only)

struct ProfScope {
  bool active; ProfRec r; hipStream_t s;
  ProfScope(const std::string& label, hipStream_t st, double flops, double bytes) : active(g_prof.on), s(st) {
    if (!active) return;
    r.label = g_prof.label_id(std::string(g_phase) + label); r.flops = flops; r.bytes = bytes;
    r.e0 = g_prof.get(); r.e1 = g_prof.get();
    (void)hipEventRecord(r.e0, s);
  }
  ~ProfScope() {
    if (!active) return;
    (void)hipEventRecord(r.e1, s);
    g_prof.recs.push_back(r);
  }
};

// porl_gemm_f32 diagnostics (scripts/bench_gemm_enc.py): the encoder's operand prologue / epilogue on a bare product
const float* g_dbg_a_scale = nullptr; const float* g_dbg_a_shift = nullptr; const float* g_dbg_resid = nullptr;
float* g_dbg_cstat = nullptr;
unsigned long long* g_qnet_stamps = nullptr;   // porl_tune_set_ptr("qnet_stamps", device buffer of >= 32 u64)

constexpr int NUM_CU = 256;
constexpr int SK_MAX = 16;
constexpr int NLL_ROWS_PER_BLOCK = 4;    // one row per wave
constexpr int LN_ROWS_PER_BLOCK = 8;
constexpr int HEAD_ROWS_PER_BLOCK = HEAD_ROWS;

// Kernel selection: every integer key of porl_tune_set, with its default.  porl_iql, porl_qnet and porl_enc copy the
// process defaults (g_tune) when they are created; the entry points without a handle (porl_gemm_f32) read g_tune.
struct Tune {
  // What pick_tile returns where its occupancy rule selects tile i ("tile_map<i>" / "tile_map_short<i>").
  // Measured on the POR step (round 2, bench.py PORL_TILE_MAP): with two co-resident 64x128 blocks per CU the
  // 4 x 1024^3 launches take 71 instead of 75 us (each block's prologue / C store under the other's MFMA loop), and the
  // 3-net forward / policy backward take 55 / 41 us on 64x64 tiles (768 / 512 blocks = exactly 3 / 2 per CU) instead of
  // 69 / 45 on 128x64 (384 blocks: 1.5 per CU).  SHORT-BLOCK mode (PORL_IQL_MODE_SHORT_BLOCKS, the pipelined update):
  // 64x64 everywhere — alone those launches are slower (77 / 84 us), but a second stream's kernels only get CUs when
  // blocks retire, and 20 us blocks retire often: 2 990 -> 3 110 updates/s.
  int tile_map[4] = {TILE_64x128, TILE_64x64, TILE_64x128, TILE_64x64};
  int tile_map_short[4] = {TILE_64x64, TILE_64x64, TILE_64x128, TILE_64x64};
  int vbwd_tile_short = -1;   // tile of the value nets' hidden-layer backward in short-block mode (A/B)
  int l0_kernel = 1;          // 0: input layers (K <= 64) through the grouped GEMM instead of l0_fwd_kernel (A/B, bit-identical)
  int l0_tile = -1;           // tile override for the K <= 128 forward layers of the IQL step (A/B)
  // Which of the <= 64-wide products of the IQL step run on skinny.hpp instead of the grouped GEMM — bit 0: input-layer
  // weight gradients dW0, bit 1: policy mean, bit 2: policy output-layer backward; 0 = round 2's path (A/B; same sums,
  // other order inside a 64-chunk), 1 is read as "all" (7)
  int skinny = 7;
  // The same mask for the PIPELINED update (PORL_IQL_MODE_SHORT_BLOCKS), "skinny_pipelined".  There the policy phase is
  // not the critical stream, and shortening its launches moved the two queues against each other — same-box A/B
  // (round 3, sustained updates/s, two runs each): mask 0: 3 306 / 3 309; 7: 3 206 / 3 204; 4:
  // 3 233 / 3 238; 6: 3 221 / 3 218 — while the one-stream update gains 10-12 us (380 -> 369 us event-timed).
  // Round 3, later: that holds for H = 1024, where the big products dominate.  At H = 256 (B = 1024) the update is a chain
  // of short launches and the skinny kernels are worth +10 % pipelined as well (8 600 -> 9 530 updates/s), at H = 512
  // +0.5 ... +5 % (6 570-6 860 -> 6 890-6 950), at H = 768 +2 % (4 490 -> 4 570), two runs each: -1 = by width — on up to
  // `skinny_pipelined_max_h`, off above.
  int skinny_pipelined = -1, skinny_pipelined_max_h = 768;
  int dw0_slabs = 16;         // slabs of the skinny dW0 kernel (<= SK_MAX; A/B: fewer slabs = fewer partial bytes, fewer blocks)
  int iql_fold = 1;           // 0: porl_iql_step keeps the slab combines as launches of their own (A/B)
  int gemm_lds_pad = 0, gemm_lds_pad_min_blocks = 0;   // extra LDS bytes per GEMM block of launches with >= min blocks
  // Short-block mode (the pipelined update), while gemm_lds_pad is 0: the pad of a GEMM launch of the value / policy phase
  // whose K is at least iql_pad_min_k, from iql_pad_min_blocks blocks on.  18 KB -> 55 KB per block -> TWO 64x64 blocks
  // per CU instead of three.  Two effects, both measured (bench.py PORL_IQL_PAD="value,policy,min_blocks",
  // PORL_GEMM_LDS_PAD; updates/s): (1) wave quantisation — the value nets' 4 x 1024^3 launches have 1 024 blocks: at three
  // per CU that is one full round of 768 and a ragged one of 256, at two per CU two full rounds (backward launch alone on
  // the chip: 84.6 -> 73.4 us; the 768-block 3-net forward gets WORSE at two per CU, 55.1 -> 59.1 us); (2) room for the
  // other stream — a third of every CU's registers and 50 KB of LDS stay free for the policy stream's small kernels
  // (with a 45 KB pad, i.e. two blocks and NO LDS left over, the update is slower than unpadded: 3 044 vs 3 106).
  // none 3 106; every GEMM launch 3 256; value phase only 3 248; policy phase only 3 065; only launches of >= 1 000 blocks
  // 3 270.  Default: the value phase's launches of at least 4 blocks per CU.
  int iql_pad_value = 18432, iql_pad_policy = 0, iql_pad_min_blocks = 4 * NUM_CU, iql_pad_min_k = 0;
  int enc_tile_n96 = 0;       // 1: 128x96 blocks for the encoder's N = 96 row product (A/B)
  int enc_gemm_sb = 1;        // 0: the encoder's 64x64 row products on the double-buffered schedule (A/B)
  int enc_patch_rows = 0;     // patch rows per block of patch_bn_kernel (0 = by grid size; A/B)
  int enc_s2d = 0;            // 1: materialise the 2x2 patches before the merge GEMM (cross-check)
  int enc_bf16_operands_only = 0;   // 1: compute_dtype="bf16" runs round 2's bf16-OPERAND mode (fp32 tensors in memory) instead of encoder_bf16.hpp (A/B)
  int enc_pconv_mfma = 0;     // 1: the fp32 partial 3x3 conv as an implicit GEMM on the matrix pipe (round 3) instead of the direct vector-ALU kernel.  Measured SLOWER (5.8 vs 3.7 ms per update at 360x256 B=512): the step moves ~2.5 GB per stage-1 call (input tile, result, the copy of the untouched channels) and is bound by that, not by the 184 GFLOP; the MFMA form parks more LDS per block (77 / 117 KB) and hides less latency.  Kept as a cross-check (tests/test_fasternet_gpu.py)
  int enc_bn_sweep = 0;       // 1: BatchNorm + ReLU of the MLP blocks as a separate sweep (cross-check)
  int enc_dense_patch = 0;    // 1: rasterise + dense patch embedding (cross-check)
  int qnet_fused = 1;         // 0 forces the multi-launch CQL path (A/B measurements)
  // 16 rows per block (v_mfma_f32_16x16x4_f32 tiles) while 32-row blocks would leave CUs idle (config 3 at B = 4096: 128 blocks
  // on 256 CUs).  No faster in round 2; with round 3's loss stage on eight lanes per row it is: 22 800 -> 25 300 updates/s,
  // step kernel 41.4 -> 34.6 us event-timed (round 3: same box, two runs each).  0 = A/B.
  int qnet_rows16 = 1;
  int qnet_wgrad_share = 11;  // sixteenths of a 32-tile layer's dW tiles the dW group keeps (16 = all: round 2's split)
  int qnet_two_groups = 1;    // 0: the one-group (256-thread) step kernel (A/B, bit-identical)
} g_tune;

// How porl_tune_set reads a value: as given, as 0 / 1, at least 0, clamped to [1, 16], or as a skinny mask (1 = all)
enum TuneClamp { TC_ANY, TC_BOOL, TC_NONNEG, TC_1_16, TC_MASK };
struct TuneKey { const char* key; int Tune::*field; TuneClamp clamp; };
#define TK(key, clamp) {#key, &Tune::key, clamp}     // the key is the field's name
const TuneKey k_tune_keys[] = {
    TK(gemm_lds_pad, TC_NONNEG), TK(gemm_lds_pad_min_blocks, TC_NONNEG), TK(iql_pad_value, TC_NONNEG), TK(iql_pad_policy, TC_NONNEG),
    TK(iql_pad_min_blocks, TC_NONNEG), TK(iql_pad_min_k, TC_NONNEG), TK(qnet_fused, TC_BOOL), TK(qnet_two_groups, TC_BOOL),
    TK(qnet_wgrad_share, TC_1_16), TK(qnet_rows16, TC_BOOL), TK(enc_dense_patch, TC_BOOL), TK(enc_s2d, TC_BOOL), TK(enc_patch_rows, TC_NONNEG),
    TK(enc_gemm_sb, TC_ANY), TK(enc_tile_n96, TC_BOOL), TK(enc_bn_sweep, TC_BOOL), TK(enc_pconv_mfma, TC_BOOL), TK(enc_bf16_operands_only, TC_BOOL),
    TK(iql_fold, TC_BOOL), TK(skinny, TC_MASK), TK(skinny_pipelined, TC_MASK), TK(skinny_pipelined_max_h, TC_ANY), TK(dw0_slabs, TC_1_16),
    TK(l0_tile, TC_ANY), TK(l0_kernel, TC_BOOL), TK(vbwd_tile_short, TC_ANY),
};

int tune_apply(Tune& t, const char* key, int value) {
  if (!key) PORL_FAIL(PORL_ERR_INVALID, "null key");
  for (const TuneKey& k : k_tune_keys) {
    if (strcmp(key, k.key)) continue;
    const TuneClamp c = k.clamp;
    t.*k.field = c == TC_BOOL ? value != 0 : c == TC_NONNEG ? std::max(0, value) : c == TC_1_16 ? std::max(1, std::min(value, 16))
               : c == TC_MASK && value == 1 ? 7 : value;
    return PORL_OK;
  }
  const bool sh = !strncmp(key, "tile_map_short", 14);
  const char* i = key + (sh ? 14 : 8);
  if (!strncmp(key, "tile_map", 8) && *i >= '0' && *i <= '3' && !i[1] && value >= 0 && value < TILE_COUNT) {
    (sh ? t.tile_map_short : t.tile_map)[*i - '0'] = value;
    return PORL_OK;
  }
  PORL_FAIL(PORL_ERR_INVALID, "unknown tuning key '%s'", key);
}

inline int64_t ru4(int64_t x) { return (x + 3) & ~int64_t(3); }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

struct TensorInfo { int64_t off; int rows, cols; };

struct MlpLayout {
  int n_lin = 0;                       // Linear layers = n_hidden + 1
  int dims[PORL_MAX_HIDDEN + 2] = {0};
  int64_t w[PORL_MAX_HIDDEN + 1] = {0}, b[PORL_MAX_HIDDEN + 1] = {0};
  int64_t lnw[PORL_MAX_HIDDEN] = {0}, lnb[PORL_MAX_HIDDEN] = {0};
  bool ln = false;
};

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
  int batch = 0;
  bool have_pol_target = false;
  bool pol_prefetched = false;      // porl_iql_policy_prefetch ran for the loaded batch: policy forward is done
  bool pol_fwd_done = false;        // porl_iql_policy_forward ran for the loaded batch
  int pol_nslab = 1;
  int Sp = 0, Dp = 0, Hp = 0, parts_max = 0;
  Workspace ws{};
  Tune tune = g_tune;               // kernel selection: the process defaults at creation, porl_iql_tune_set
};

namespace {

// ---- launch helpers -------------------------------------------------------------------------------
int pick_tile(const GemmGroup& g, const Tune& t, bool short_blocks = false) {
  int minM = 1 << 30, minN = 1 << 30, maxK = 0;
  for (int i = 0; i < g.nprob; ++i) {
    minM = std::min(minM, g.p[i].M); minN = std::min(minN, g.p[i].N); maxK = std::max(maxK, g.p[i].K);
  }
  // a short K loop cannot hide its own prologue/epilogue: many small blocks per CU overlap them instead
  if (maxK <= 128) return TILE_64x64;
  auto blocks = [&](int tile) {
    int bm, bn, n = 0;
    tile_dims(tile, bm, bn);
    for (int i = 0; i < g.nprob; ++i) n += cdiv(g.p[i].M, bm) * cdiv(g.p[i].N, bn) * std::max(1, g.p[i].splitk);
    return n;
  };
  int cand[3], nc = 0;
  if (minN <= 64 && minM <= 64) { cand[nc++] = TILE_64x64; }
  else if (minN <= 64) { cand[nc++] = TILE_128x64; cand[nc++] = TILE_64x64; }
  else if (minM <= 64) { cand[nc++] = TILE_64x128; cand[nc++] = TILE_64x64; }
  else { cand[nc++] = TILE_128x128; cand[nc++] = TILE_128x64; cand[nc++] = TILE_64x64; }
  const int* map = short_blocks ? t.tile_map_short : t.tile_map;
  for (int i = 0; i < nc; ++i)
    if (blocks(cand[i]) >= NUM_CU) return map[cand[i]];
  return map[cand[nc - 1]];
}

// split-K factor for an output too small to fill the chip on its own
int pick_splitk(int M, int N, int K, int nprob, int bm, int bn) {
  const int tiles = nprob * cdiv(M, bm) * cdiv(N, bn);
  int sk = cdiv(NUM_CU, tiles);
  sk = std::min(sk, std::max(1, K / 64));
  return std::max(1, std::min(sk, SK_MAX));
}

// iql_pad >= 0: a launch of the short-block IQL update, whose phase pads by iql_pad (Tune::iql_pad_value / _policy)
int launch_group(GemmGroup& g, int tile, const Tune& t, hipStream_t s, int iql_pad = -1) {
  const bool iql = iql_pad >= 0 && !t.gemm_lds_pad && g.nprob > 0 && g.p[0].K >= t.iql_pad_min_k;
  g.lds_pad = iql ? iql_pad : t.gemm_lds_pad;
  g.lds_pad_min_blocks = iql ? t.iql_pad_min_blocks : t.gemm_lds_pad_min_blocks;
  double flops = 0.0, bytes = 0.0;
  std::string label;
  if (g_prof.on) {
    bool vec = true, apro = false;
    for (int i = 0; i < g.nprob; ++i) {
      const GemmProb& p = g.p[i];
      flops += 2.0 * p.M * p.N * p.K;
      bytes += 4.0 * ((double)p.M * p.K + (double)p.N * p.K + (p.store_c ? (double)p.M * p.N : 0.0));
      vec = vec && p.a_vec && p.b_vec;
      apro = apro || p.apro != APRO_NONE;
    }
    int bm, bn;
    tile_dims(tile, bm, bn);
    const TileCfg tc = tile_cfg(tile);
    label = "gemm_f32_kernel<" + std::to_string(bm) + "," + std::to_string(bn) + "," + std::to_string(GEMM_BK) + "," +
            std::to_string(tc.wm) + "," + std::to_string(tc.wn) + "," + (vec ? "true" : "false") + "," +
            (apro ? "true" : "false") + (g.single_buffer && vec && tile == TILE_64x64 ? ",true>" : ">");   // ONEBUF
  }
  ProfScope ps(label, s, flops, bytes);
  hipError_t e = launch_gemm_group(tile, g, s);
  if (e != hipSuccess) {
    g_err = std::string("gemm launch: ") + hipGetErrorString(e);
    return (int)e;
  }
  return 0;
}

// bf16-operand / fp32-accumulate variant (gemm_bf16.hpp): the costmap encoder's opt-in mode
int launch_group_bf16(GemmGroup& g, int tile, hipStream_t s) {
  double flops = 0.0, bytes = 0.0;
  std::string label;
  if (g_prof.on) {
    for (int i = 0; i < g.nprob; ++i) {
      const GemmProb& p = g.p[i];
      flops += 2.0 * p.M * p.N * p.K;
      bytes += 4.0 * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * p.N * (p.resid ? 2.0 : 1.0));
    }
    int bm, bn;
    tile_dims(tile, bm, bn);
    label = "gemm_bf16_kernel<" + std::to_string(bm) + "," + std::to_string(bn) + "," +
            (g.p[0].apro != APRO_NONE ? "true" : "false") + ">";
  }
  ProfScope ps(label, s, flops, bytes);
  hipError_t e = launch_gemm_bf16_group(tile, g, s);
  if (e != hipSuccess) {
    g_err = std::string("bf16 gemm launch: ") + hipGetErrorString(e);
    return (int)e;
  }
  return 0;
}

int launch_reduce(ReduceArgs& r, hipStream_t s) {
  if (r.njobs == 0) return 0;
  long maxn = 0;
  for (int i = 0; i < r.njobs; ++i) maxn = std::max(maxn, r.job[i].n);
  dim3 grid((unsigned)std::min<long>((maxn + 31) / 32, 2048), r.njobs);
  ProfScope ps("multi_reduce_kernel", s, 0.0, 0.0);
  hipLaunchKernelGGL(multi_reduce_kernel, grid, dim3(256), 0, s, r);
  PORL_HIP(hipGetLastError());
  return 0;
}

void add_reduce(ReduceArgs& r, float* out, const float* slab, long n, long stride, int nslab, int op = 0,
                float scale = 1.f) {
  ReduceJob& j = r.job[r.njobs++];
  j.out = out; j.slab = slab; j.bias = nullptr; j.n = n; j.stride = stride; j.nslab = nslab; j.ncols = 1; j.act = 0;
  j.op = op; j.scale = scale; j.adam_off = -1;
  j.width = nslab > 64 ? 4 : 32;        // long lists of partials: 64 slab lanes per output instead of 8
}

int check_ready(const porl_iql* h, bool need_batch) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_iql_bind() has not been called");
  if (need_batch && h->batch <= 0) PORL_FAIL(PORL_ERR_INVALID, "no minibatch loaded (porl_iql_load_batch)");
  return 0;
}

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

}  // namespace

// =====================================================================================================
extern "C" {

int porl_abi_version(void) { return PORL_ABI_VERSION; }
const char* porl_last_error(void) { return g_err.c_str(); }

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
  w.slab_a = take((int64_t)SK_MAX * 2 * ((int64_t)H * S + 2 * H + 8));
  w.slab_b = take((int64_t)SK_MAX * ((int64_t)D * H + D + 8));
  w.slab_pa = take((int64_t)SK_MAX * ((int64_t)H * S + 2 * H + 8));
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

int porl_iql_load_batch(porl_iql* h, int32_t batch, const float* obs, int64_t obs_rs, const float* next_obs,
                        int64_t next_rs, const float* rew, int64_t rew_rs, const float* term, int64_t term_rs,
                        const float* pol_target, int64_t pt_rs, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  if (!obs || !next_obs || !rew || !term) PORL_FAIL(PORL_ERR_INVALID, "null batch tensor");
  float* W = h->buf.workspace;
  if (h->mode & PORL_IQL_MODE_TWO_SLOTS) h->slot = (h->slot + 1) % PORL_IQL_SLOTS;
  PackArgs a{};
  a.rows = batch;
  auto job = [&](const float* src, int64_t rs, float* dst, int cols, int ld) {
    PackJob& j = a.job[a.njobs++];
    j.src = src; j.dst = dst; j.src_row_stride = rs; j.src_col_stride = 1; j.cols = cols; j.ld = ld;
  };
  job(obs, obs_rs, W + h->ws.xs_slot[h->slot], h->cfg.obs_dim, h->Sp);
  job(next_obs, next_rs, W + h->ws.xn, h->cfg.obs_dim, h->Sp);
  job(rew, rew_rs, W + h->ws.rew, 1, 1);
  job(term, term_rs, W + h->ws.term, 1, 1);
  if (pol_target) job(pol_target, pt_rs, W + h->ws.xt_slot[h->slot], h->cfg.pol_out_dim, h->Dp);
  h->have_pol_target = pol_target != nullptr;
  h->pol_prefetched = false;
  h->pol_fwd_done = false;
  const long n = (long)batch * std::max(h->Sp, h->Dp);
  dim3 grid((unsigned)std::min<long>((n + 255) / 256, 1024), a.njobs);
  hipLaunchKernelGGL(pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  h->batch = batch;
  return PORL_OK;
}

// LayerNorm variant of the value backward: dZ of every hidden layer is materialised by the LayerNorm
// backward kernel (row statistics), gamma/beta/(head) gradients come from its per-block partial sums.
static int value_backward_ln(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, ReduceArgs* defer) {
  (void)hp;
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, Hp = h->Hp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  float* Gv = h->buf.grads_vf;
  const int nln = cdiv(B, LN_ROWS_PER_BLOCK);
  for (int l = L - 1; l >= 0; --l) {
    const bool top = l == L - 1;
    const int Kin = l == 0 ? S : H;
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
      const float* dz = W + ws.dz_v[i][1];
      const float* in = l == 0 ? W + ws.xs_slot[h->slot] : W + ws.act_v[i][l - 1];
      const int ldin = l == 0 ? h->Sp : Hp;
      GemmProb p = make_prob(GEMM_TN, dz, Hp, in, ldin, Gv + h->v[i].w[l], Kin, H, Kin, B);
      p.colsum = Gv + h->v[i].b[l];
      g.p[g.nprob++] = p;
      if (l > 0)   // unmasked: the ReLU mask of layer l-1 is applied by its own LayerNorm backward
        g.p[g.nprob++] = make_prob(GEMM_NN, dz, Hp, Pv + h->v[i].w[l], Kin, W + ws.dz_v[i][0], Hp, B, Kin, H);
    }
    const int tile = iql_tile(h, g);
    if (l == 0) {
      int bm, bn;
      tile_dims(tile, bm, bn);
      const int sk = pick_splitk(H, Kin, B, 2, bm, bn);
      if (sk > 1) {
        const int64_t per = (int64_t)H * Kin, perc = H;
        for (int i = 0; i < 2; ++i) {
          float* slabW = W + ws.slab_a + (int64_t)i * SK_MAX * (per + 2 * perc + 8);
          float* slabC = slabW + (int64_t)SK_MAX * per;
          g.p[i].splitk = sk; g.p[i].C = slabW; g.p[i].colsum = slabC;
          add_reduce(red, Gv + h->v[i].w[0], slabW, per, per, sk);
          add_reduce(red, Gv + h->v[i].b[0], slabC, perc, perc, sk);
        }
      }
    }
    PORL_TRY(iql_launch(h, g, tile, false, s));
    if (l == 0 && defer) *defer = red;       // only the last combine can wait for the Adam launch: the LayerNorm
    else PORL_TRY(launch_reduce(red, s));    // partial buffers are reused layer by layer
  }
  return PORL_OK;
}

static int feistel_half_bits(int64_t n_rows) {
  int bits = 1;
  while ((int64_t(1) << bits) < n_rows) ++bits;
  return std::max(1, (bits + 1) / 2);
}

int porl_iql_load_batch_sampled(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                                int32_t act_dim, int32_t target_is_action, uint64_t seed, uint64_t step,
                                int64_t* idx_out, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  if (!rows || n_rows < batch || n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "need batch <= n_rows");
  const int S = h->cfg.obs_dim, D = h->cfg.pol_out_dim;
  if (row_stride < 2 * (int64_t)S + 2 + act_dim) PORL_FAIL(PORL_ERR_INVALID, "row stride shorter than 2*S+2+A");
  if (target_is_action ? D != act_dim : D != S) PORL_FAIL(PORL_ERR_INVALID, "policy target width mismatch");
  float* W = h->buf.workspace;
  if (h->mode & PORL_IQL_MODE_TWO_SLOTS) h->slot = (h->slot + 1) % PORL_IQL_SLOTS;
  SampledBatchArgs a{};
  a.rows = rows; a.row_stride = (long)row_stride; a.n_rows = n_rows;
  a.batch = batch; a.S = S; a.A = act_dim; a.D = D; a.Sp = h->Sp; a.Dp = h->Dp;
  a.hb = feistel_half_bits(n_rows); a.target_is_action = target_is_action;
  a.seed = seed; a.step = step;
  a.xs = W + h->ws.xs_slot[h->slot]; a.xn = W + h->ws.xn; a.xt = W + h->ws.xt_slot[h->slot]; a.rew = W + h->ws.rew; a.term = W + h->ws.term;
  a.idx_out = idx_out;
  {
    g_phase = "V1.";
    ProfScope ps("sampled_batch_kernel", (hipStream_t)stream, 0.0, 8.0 * batch * (2 * S + 2 + act_dim));
    hipLaunchKernelGGL(sampled_batch_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
    g_phase = "";
  }
  PORL_HIP(hipGetLastError());
  h->batch = batch;
  h->have_pol_target = true;
  h->pol_prefetched = false;
  h->pol_fwd_done = false;
  return PORL_OK;
}

int porl_iql_load_batch_indexed(porl_iql* h, int32_t batch, const float* rows, int64_t row_stride, int64_t n_rows,
                                const int64_t* idx, int32_t state_dim, int32_t act_dim, int32_t target_is_action,
                                int32_t clamp_target_gt8, const float* obs_feat, int64_t obs_rs, const float* next_feat,
                                int64_t next_rs, void* stream) {
  PORL_TRY(check_ready(h, false));
  // every argument is judged before the first HIP call
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
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
  if (h->mode & PORL_IQL_MODE_TWO_SLOTS) h->slot = (h->slot + 1) % PORL_IQL_SLOTS;
  IndexedBatchArgs a{};
  a.rows = rows; a.row_stride = (long)row_stride; a.idx = idx;
  a.batch = batch; a.S = state_dim; a.F = F; a.D = D; a.Sp = h->Sp; a.Dp = h->Dp;
  a.target_is_action = target_is_action; a.clamp_target = clamp_target_gt8;
  a.obs_feat = obs_feat; a.obs_rs = (long)obs_rs; a.next_feat = next_feat; a.next_rs = (long)next_rs;
  a.xs = W + h->ws.xs_slot[h->slot]; a.xn = W + h->ws.xn; a.xt = W + h->ws.xt_slot[h->slot]; a.rew = W + h->ws.rew; a.term = W + h->ws.term;
  {
    g_phase = "V1.";
    ProfScope ps("indexed_batch_kernel", (hipStream_t)stream, 0.0, 4.0 * batch * (2.0 * h->Sp + h->Dp + 2) * 2.0);
    hipLaunchKernelGGL(indexed_batch_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a);
    g_phase = "";
  }
  PORL_HIP(hipGetLastError());
  h->batch = batch;
  h->have_pol_target = true;
  h->pol_prefetched = false;
  h->pol_fwd_done = false;
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
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!stats) PORL_FAIL(PORL_ERR_INVALID, "null stats");
  h->buf.stats = stats;
  return PORL_OK;
}


// Input-layer weight gradients dW0 = dZ0^T X (+ db0) of up to 4 nets on wgrad_skinny_kernel (skinny.hpp): slabs over
// batch chunks in the split-K layout, combine jobs appended to `red`.  Returns false when the shapes do not qualify
// (the caller then takes the grouped-GEMM path).
struct Dw0Net { const float* dz; float* gw; float* gb; float* slabW; float* slabC; };
static bool dw0_skinny(const porl_iql* h, const Dw0Net* nets, int nnets, const float* X, int ldx, int B, int H, int S, int ldz,
                       ReduceArgs& red, const char* phase, hipStream_t s, int* rc) {
  *rc = 0;
  if (!(skinny_mask(h) & 1) || S > SKN_T || nnets > SKN_MAX_NETS || H % 4 || !skn_ok4(X, ldx) || ldz % 4) return false;
  for (int i = 0; i < nnets; ++i) if (!skn_ok4(nets[i].dz, ldz)) return false;
  WgradSkinnyArgs a{};
  a.nnets = nnets; a.B = B; a.H = H; a.S = S; a.ldz = ldz; a.ldx = ldx; a.ldo = S;
  a.tiles_n = cdiv(H, SKN_T);
  skn_split(cdiv(B, SKN_T), h->tune.dw0_slabs, a.nslab, a.rtiles);
  a.slabW_stride = (long)H * S; a.slabC_stride = H;
  for (int i = 0; i < nnets; ++i) {
    a.net[i] = WgradSkinnyNet{nets[i].dz, X, nets[i].slabW, nets[i].slabC};
    add_reduce(red, nets[i].gw, nets[i].slabW, (long)H * S, (long)H * S, a.nslab);
    add_reduce(red, nets[i].gb, nets[i].slabC, H, H, a.nslab);
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

// ---------------------------------------------------------------------------------------------------
// `defer` (optional): the final combine launch is not issued; its jobs are handed to the caller, who folds them into
// the Adam launch (porl_iql_step).
static int value_backward_impl(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, ReduceArgs* defer) {
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, Hp = h->Hp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  const float* Pt = h->buf.params_tgt;
  float* Gv = h->buf.grads_vf;
  int parts = 0;
  const bool LN = h->cfg.layer_norm != 0;

  // -- forward: target twins on s', online twins on s — 4 nets per launch ---------------------------
  for (int l = 0; l < L; ++l) {
    FwdNet nets[4];
    const int K = l == 0 ? S : H;
    for (int n = 0; n < 4; ++n) {
      const bool tgt = n < 2;
      const int i = n & 1;
      const float* P = tgt ? Pt : Pv;
      FwdNet& f = nets[n];
      if (l == 0) { f.in = W + (tgt ? ws.xn : ws.xs_slot[h->slot]); f.ldin = h->Sp; }
      else { f.in = W + (tgt ? ws.act_t[i][(l - 1) & 1] : ws.act_v[i][l - 1]); f.ldin = Hp; }
      f.W = P + h->v[i].w[l]; f.b = P + h->v[i].b[l];
      const bool last = l == L - 1;
      f.out = tgt ? ((last && !LN) ? nullptr : W + ws.act_t[i][l & 1]) : W + ws.act_v[i][l];
      f.headw = P + h->v[i].w[L];
      f.headout = W + (tgt ? ws.hp_t[i] : ws.hp_v[i]);
      if (LN) {
        f.ln_g = P + h->v[i].lnw[l]; f.ln_b = P + h->v[i].lnb[l];
        if (!tgt) { f.xhat = W + ws.xhat_v[i][l]; f.rstd = W + ws.rstd_v[i][l]; }
      }
    }
    g_phase = l == 0 ? "V2.L0fwd:" : "V3.fwd:";
    PORL_TRY(fwd_hidden_layer(h, nets, 4, B, K, l == L - 1, &parts, false, s));
  }
  g_phase = "V4.head:";

  // -- TD target, expectile loss, dL/dv: with LayerNorm a kernel of its own; otherwise fused into the head
  //    backward below --------------------------------------------------------------------------------------
  if (LN) {
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

  ReduceArgs red{};
  if (LN) return value_backward_ln(h, hp, s, defer);
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
    const int Kin = l == 0 ? S : H;
    if (l == 0) {
      // skinny (H x S) weight gradient on its own kernel: one 64 x 64 tile of dZ0 per block, slabs over batch chunks
      Dw0Net dn[2];
      const int64_t per = (int64_t)H * S, perc = H;
      for (int i = 0; i < 2; ++i) {
        float* slabW = W + ws.slab_a + (int64_t)i * SK_MAX * (per + 2 * perc + 8);
        dn[i] = Dw0Net{W + ws.dz_v[i][0], Gv + h->v[i].w[0], Gv + h->v[i].b[0], slabW, slabW + (int64_t)SK_MAX * per};
      }
      int rc = 0;
      if (dw0_skinny(h, dn, 2, W + ws.xs_slot[h->slot], h->Sp, B, H, S, Hp, red, "V6.dW0:", s, &rc)) {
        if (rc) return rc;
        break;
      }
    }
    GemmGroup g{};
    for (int i = 0; i < 2; ++i) {
      const float* dz = W + ws.dz_v[i][l & 1];
      const float* in = l == 0 ? W + ws.xs_slot[h->slot] : W + ws.act_v[i][l - 1];
      const int ldin = l == 0 ? h->Sp : Hp;
      GemmProb p = make_prob(GEMM_TN, dz, Hp, in, ldin, Gv + h->v[i].w[l], Kin, H, Kin, B);
      p.colsum = Gv + h->v[i].b[l];
      g.p[g.nprob++] = p;
      if (l > 0) {
        GemmProb q = make_prob(GEMM_NN, dz, Hp, Pv + h->v[i].w[l], Kin, W + ws.dz_v[i][(l - 1) & 1], Hp, B, Kin, H);
        q.mask = W + ws.act_v[i][l - 1]; q.ldmask = Hp;
        g.p[g.nprob++] = q;
      }
    }
    int tile = iql_tile(h, g);
    if (l > 0 && short_blocks(h) && h->tune.vbwd_tile_short >= 0) tile = h->tune.vbwd_tile_short;
    if (l == 0) {
      // skinny (H x S) weight gradient: split the batch (K) dimension to fill the chip
      int bm, bn;
      tile_dims(tile, bm, bn);
      const int sk = pick_splitk(H, Kin, B, 2, bm, bn);
      if (sk > 1) {
        const int64_t per = (int64_t)H * Kin, perc = H;
        for (int i = 0; i < 2; ++i) {
          float* slabW = W + ws.slab_a + (int64_t)i * SK_MAX * (per + 2 * perc + 8);
          float* slabC = slabW + (int64_t)SK_MAX * per;
          g.p[i].splitk = sk; g.p[i].C = slabW; g.p[i].colsum = slabC;
          add_reduce(red, Gv + h->v[i].w[0], slabW, per, per, sk);
          add_reduce(red, Gv + h->v[i].b[0], slabC, perc, perc, sk);
        }
      }
    }
    g_phase = l == 0 ? "V6.dW0:" : "V5.bwd:";
    PORL_TRY(iql_launch(h, g, tile, false, s));
  }
  g_phase = "V7.combine:";
  if (defer) *defer = red;
  else PORL_TRY(launch_reduce(red, s));
  g_phase = "";
  return PORL_OK;
}

int porl_iql_value_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  const bool fold = (h->mode & PORL_IQL_MODE_FOLD_COMBINE) != 0;
  h->fin_v = ReduceArgs{};
  PORL_TRY(value_backward_impl(h, hp, (hipStream_t)stream, fold ? &h->fin_v : nullptr));
  h->fin_v_pending = fold;
  return PORL_OK;
}

// ---------------------------------------------------------------------------------------------------
// Adam(+EMA) over one flat group.  `fin` (optional): combine jobs that the backward pass left pending; those whose
// output lies inside the gradient buffer `g` are folded into this launch (short slab lists inside the float4 sweep,
// long ones as extra reduce+Adam blocks), the others (loss statistics) ride along as plain reduce blocks.
static int adam_launch(float* p, float* g, float* m, float* v, float* tgt, int64_t n, double lr, int step,
                       double b1, double b2, double eps, double ema_beta, hipStream_t s, const ReduceArgs* fin = nullptr) {
  if (n < 0 || n % 4) PORL_FAIL(PORL_ERR_INVALID, "adam range must be a non-negative multiple of 4 floats");
  if (step < 1) PORL_FAIL(PORL_ERR_INVALID, "adam step must be >= 1");
  if (n == 0 && !(fin && fin->njobs)) return PORL_OK;      // an empty range is an empty sweep (the grid maths below divide by it)
  AdamArgs a{};
  a.p = p; a.g = g; a.m = m; a.v = v; a.tgt = tgt;
  // torch._single_tensor_adam: python doubles, rounded to fp32 where they meet tensors
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  a.s.step_size = (float)(lr / bc1);
  a.s.bc2_sqrt = (float)std::sqrt(bc2);
  a.s.omb1 = (float)(1.0 - b1); a.s.beta2 = (float)b2; a.s.omb2 = (float)(1.0 - b2);
  a.s.eps = (float)eps; a.s.ema_beta = (float)ema_beta; a.s.omeb = (float)(1.0 - ema_beta);
  a.n4 = n / 4;
  // one float4 per thread and a single trip through the block's loop whenever the grid allows it: a second, nearly
  // empty trip would double every block's memory round trips (measured: 12 -> 19 us on the 80 MB value group)
  const int sweep_blocks = (int)std::min<long>((a.n4 + 255) / 256, 1 << 20);
  a.span4 = sweep_blocks ? ((a.n4 + sweep_blocks - 1) / sweep_blocks + 255) / 256 * 256 : 256;
  int reduce_blocks = 0;
  double extra_bytes = 0.0;
  if (fin) {
    for (int q = 0; q < fin->njobs; ++q) {
      ReduceJob j = fin->job[q];
      const bool inside = j.out >= g && j.out + j.n <= g + n;
      const long off = inside ? (long)(j.out - g) : -1;
      extra_bytes += 4.0 * (double)j.n * j.nslab;
      const bool plain = j.op == 0 && j.scale == 1.f && !j.bias && j.act == 0;
      if (inside && plain && j.nslab <= ADAM_SWEEP_SLABS && off % 4 == 0 && j.n % 4 == 0 && j.stride % 4 == 0 &&
          aligned16(j.slab) && a.nregions < MAX_ADAM_REGIONS) {
        AdamRegion& R = a.region[a.nregions++];
        R.lo = off; R.hi = off + j.n; R.slab = j.slab; R.stride = j.stride; R.nslab = j.nslab;
        continue;
      }
      if (inside) {
        if (off % 4) PORL_FAIL(PORL_ERR_INVALID, "gradient tensors start on 16-byte boundaries");
        j.adam_off = off;
        a.skip_lo[a.nskip] = off; a.skip_hi[a.nskip] = ru4(off + j.n); ++a.nskip;
      } else {
        j.adam_off = -1;
      }
      a.job_block0[a.r.njobs] = reduce_blocks;
      a.r.job[a.r.njobs++] = j;
      reduce_blocks += (int)((j.n + j.width - 1) / j.width);
    }
    a.job_block0[a.r.njobs] = reduce_blocks;
  }
  ProfScope ps("adam_ema_kernel", s, 0.0, (double)n * (tgt ? 36.0 : 28.0) + extra_bytes);
  a.reduce_blocks = reduce_blocks;
  hipLaunchKernelGGL(adam_ema_kernel, dim3(sweep_blocks + reduce_blocks), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iql_value_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  g_phase = "V8.";
  const int rc = adam_launch(h->buf.params_vf, h->buf.grads_vf, h->buf.adam_m_vf, h->buf.adam_v_vf, h->buf.params_tgt,
                             h->n_vf, hp->value_lr, hp->value_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps,
                             hp->ema_beta, (hipStream_t)stream, h->fin_v_pending ? &h->fin_v : nullptr);
  g_phase = "";
  h->fin_v_pending = false;
  return rc;
}

int porl_iql_policy_apply(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  g_phase = "P9.";
  const int rc = adam_launch(h->buf.params_pol, h->buf.grads_pol, h->buf.adam_m_pol, h->buf.adam_v_pol, nullptr, h->n_pol,
                             hp->policy_lr, hp->policy_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0,
                             (hipStream_t)stream, h->fin_p_pending ? &h->fin_p : nullptr);
  g_phase = "";
  h->fin_p_pending = false;
  return rc;
}

// ---------------------------------------------------------------------------------------------------
// policy mean (pre-bias, pre-activation) as split-K slabs: act_p[L-1] (B,H) x W_L^T (H,D)
static int policy_mean_slabs(porl_iql* h, int B, int* nslab, bool policy, hipStream_t s) {
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

// The part of the policy step that does not depend on the value networks: the policy MLP's forward on the loaded
// observations.  In data-parallel mode it runs while the value-gradient all-reduce is on the wire.
int porl_iql_policy_prefetch(porl_iql* h, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!h->have_pol_target) PORL_FAIL(PORL_ERR_INVALID, "policy step needs pol_target in porl_iql_load_batch");
  hipStream_t s = (hipStream_t)stream;
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pp = h->buf.params_pol;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    FwdNet f{};
    if (l == 0) { f.in = W + ws.xs_slot[h->slot]; f.ldin = h->Sp; }
    else { f.in = W + ws.act_p[l - 1]; f.ldin = h->Hp; }
    f.W = Pp + h->pol.w[l]; f.b = Pp + h->pol.b[l];
    f.out = W + ws.act_p[l]; f.headw = nullptr; f.headout = nullptr;
    PORL_TRY(fwd_hidden_layer(h, &f, 1, B, l == 0 ? S : H, l == L - 1, &parts, false, s));
  }
  PORL_TRY(policy_mean_slabs(h, B, &h->pol_nslab, false, s));
  h->pol_prefetched = true;
  return PORL_OK;
}

// part: 1 = forward half only (second twin forward, policy forward, mean, weights + NLL + dL/dmean: everything of the
// policy phase that reads the VALUE parameters), 2 = gradient half only (needs the forward half of the same batch),
// 3 = both.
// only_policy: the policy-only step (porl_iql_policy_only_*).  Its forward half runs all five nets forward-only — target
// twin on s', online twin on s, policy on s — in one grouped launch per layer, keeps no V-net activation, and takes the
// per-row weights from policy_weight_kernel (TD target included) instead of the value phase's target_v.
static int policy_backward_impl(porl_iql* h, const porl_iql_hyper* hp, hipStream_t s, ReduceArgs* defer, int part = 3,
                                bool only_policy = false) {
  if (!h->have_pol_target) PORL_FAIL(PORL_ERR_INVALID, "policy step needs pol_target in porl_iql_load_batch");
  const int B = h->batch, S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim;
  const int Hp = h->Hp, Dp = h->Dp;
  float* W = h->buf.workspace;
  const Workspace& ws = h->ws;
  const float* Pv = h->buf.params_vf;
  const float* Pp = h->buf.params_pol;
  float* Gp = h->buf.grads_pol;
  int parts = 0;
  const bool LN = h->cfg.layer_norm != 0;

  const int nblk = cdiv(B, NLL_ROWS_PER_BLOCK);
  if (part == 2 && !h->pol_fwd_done) PORL_FAIL(PORL_ERR_INVALID, "porl_iql_policy_forward has not run for this batch");
  if ((part & 1) && !h->pol_fwd_done) {
  // -- forward: updated twins (head only) + policy hidden layers, 3 nets per launch; the policy net is left out
  //    when porl_iql_policy_prefetch already ran it for this batch ---------------------------------------------
  const bool pre = h->pol_prefetched;
  const bool pre_weight = only_policy;
  h->pol_prefetched = false;
  if (only_policy) {
    const float* Pt = h->buf.params_tgt;
    for (int l = 0; l < L; ++l) {
      FwdNet nets[MAX_FWD_NETS];
      const int K = l == 0 ? S : H;
      const bool last = l == L - 1;
      for (int n = 0; n < 4; ++n) {
        const bool tgt = n < 2;
        const int i = n & 1;
        const float* P = tgt ? Pt : Pv;
        const int64_t* act = tgt ? ws.act_t[i] : ws.act_q[i];      // two ping-pong scratch buffers per net
        FwdNet& f = nets[n];
        if (l == 0) { f.in = W + (tgt ? ws.xn : ws.xs_slot[h->slot]); f.ldin = h->Sp; }
        else { f.in = W + act[(l - 1) & 1]; f.ldin = Hp; }
        f.W = P + h->v[i].w[l]; f.b = P + h->v[i].b[l];
        f.out = (last && !LN) ? nullptr : W + act[l & 1];
        f.headw = P + h->v[i].w[L]; f.headout = W + (tgt ? ws.hp_t[i] : ws.hp_q[i]);
        if (LN) { f.ln_g = P + h->v[i].lnw[l]; f.ln_b = P + h->v[i].lnb[l]; }
      }
      int first = 4;
      if (!pre) {
        FwdNet& f = nets[4];
        if (l == 0) { f.in = W + ws.xs_slot[h->slot]; f.ldin = h->Sp; }
        else { f.in = W + ws.act_p[l - 1]; f.ldin = Hp; }
        f.W = Pp + h->pol.w[l]; f.b = Pp + h->pol.b[l];
        f.out = W + ws.act_p[l]; f.headw = nullptr; f.headout = nullptr;
        first = 5;
      }
      g_phase = l == 0 ? "O1.L0fwd:" : "O2.fwd:";
      PORL_TRY(fwd_hidden_layer(h, nets, first, B, K, last, &parts, true, s));
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
  }
  for (int l = 0; l < L && !only_policy; ++l) {
    FwdNet nets[3];
    const int K = l == 0 ? S : H;
    const bool last = l == L - 1;
    for (int i = 0; i < 2; ++i) {
      FwdNet& f = nets[i];
      if (l == 0) { f.in = W + ws.xs_slot[h->slot]; f.ldin = h->Sp; }
      else { f.in = W + ws.act_q[i][(l - 1) & 1]; f.ldin = Hp; }
      f.W = Pv + h->v[i].w[l]; f.b = Pv + h->v[i].b[l];
      f.out = (last && !LN) ? nullptr : W + ws.act_q[i][l & 1];
      f.headw = Pv + h->v[i].w[L]; f.headout = W + ws.hp_q[i];
      if (LN) { f.ln_g = Pv + h->v[i].lnw[l]; f.ln_b = Pv + h->v[i].lnb[l]; }
    }
    FwdNet& f = nets[2];
    if (l == 0) { f.in = W + ws.xs_slot[h->slot]; f.ldin = h->Sp; }
    else { f.in = W + ws.act_p[l - 1]; f.ldin = Hp; }
    f.W = Pp + h->pol.w[l]; f.b = Pp + h->pol.b[l];
    f.out = W + ws.act_p[l]; f.headw = nullptr; f.headout = nullptr;
    g_phase = l == 0 ? "P1.L0fwd:" : "P2.fwd:";
    PORL_TRY(fwd_hidden_layer(h, nets, pre ? 2 : 3, B, K, last, &parts, true, s));
  }
  int nslab = h->pol_nslab;
  g_phase = only_policy ? "O4.mean:" : "P3.mean:";
  if (!pre) PORL_TRY(policy_mean_slabs(h, B, &nslab, true, s));
  g_phase = only_policy ? "O5." : "P4.";

  // -- advantage weights, NLL, dL/dmean, dL/dlog_std --------------------------------------------------
  {
    PolicyNllArgs a{};
    for (int i = 0; i < 2; ++i) { a.hp_v[i] = W + ws.hp_q[i]; a.b_v[i] = Pv + h->v[i].b[L]; }
    a.parts = pre_weight ? 0 : parts; a.target_v = W + ws.target_v_slot[h->slot];
    a.weight = pre_weight ? W + ws.pol_w : nullptr;
    a.mean_slab = W + ws.slab_mean; a.nslab = nslab; a.slab_stride = (long)B * Dp;
    a.mean_bias = Pp + h->pol.b[L]; a.log_std = Pp + h->logstd_off;
    a.x = W + ws.xt_slot[h->slot]; a.ldx = Dp; a.dmean = W + ws.dmu; a.ldd = Dp;
    a.part_loss = W + ws.part_loss; a.part_min = W + ws.part_min; a.part_dls = W + ws.part_dls;
    a.B = B; a.D = D; a.ldm = Dp; a.tanh_mean = h->cfg.pol_tanh; a.weight_mode = h->cfg.weight_mode;
    a.alpha = hp->alpha; a.inv_batch = hp->inv_batch; a.rows_per_block = NLL_ROWS_PER_BLOCK;
    ProfScope ps("policy_nll_kernel", s, 0.0, 4.0 * B * (nslab + 2.0) * Dp);
    hipLaunchKernelGGL(policy_nll_kernel, dim3(nblk), dim3(256), 0, s, a);
    PORL_HIP(hipGetLastError());
  }
  g_phase = "";
  h->pol_fwd_done = true;
  }
  if (!(part & 2)) return PORL_OK;
  h->pol_fwd_done = false;

  // -- backward ---------------------------------------------------------------------------------------
  ReduceArgs red{};
  // the NLL kernel's per-block partials are combined by the step's final reduce launch
  add_reduce(red, Gp + h->logstd_off, W + ws.part_dls, D, D, nblk);            // d/dlog_std (already clamp-masked)
  add_reduce(red, h->buf.stats + 1, W + ws.part_loss, 1, 1, nblk);            // stats[1] = g_loss
  add_reduce(red, h->buf.stats + 2, W + ws.part_min, 1, 1, nblk, /*min*/ 1);  // stats[2] = min NLL
  if ((skinny_mask(h) & 4) && D <= SKN_T && H % 4 == 0 && Dp % 4 == 0 && Hp % 4 == 0 && skn_ok4(Pp + h->pol.w[L], H)) {
    // output layer on out_bwd_kernel (skinny.hpp): one pass over the last hidden activation gives dZ_{L-1} and the
    // dW_L / db_L slabs
    OutBwdArgs a{};
    a.dmu = W + ws.dmu; a.W = Pp + h->pol.w[L]; a.A = W + ws.act_p[L - 1];
    a.dZ = W + ws.dz_p[(L - 1) & 1];
    a.slabW = W + ws.slab_b; a.slabC = a.slabW + (int64_t)SK_MAX * D * H;
    a.B = B; a.H = H; a.D = D; a.lddmu = Dp; a.ldw = H; a.lda = Hp; a.lddz = Hp;
    a.tiles_n = cdiv(H, SKN_T);
    skn_split(cdiv(B, SKN_T), SK_MAX, a.nslab, a.rtiles);
    a.slabW_stride = (long)D * H; a.slabC_stride = D;
    add_reduce(red, Gp + h->pol.w[L], a.slabW, (long)D * H, (long)D * H, a.nslab);
    add_reduce(red, Gp + h->pol.b[L], a.slabC, D, D, a.nslab);
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
    if (sk > 1) {
      float* slabW = W + ws.slab_b;
      float* slabC = slabW + (int64_t)SK_MAX * D * H;
      g.p[0].splitk = sk; g.p[0].C = slabW; g.p[0].colsum = slabC;
      add_reduce(red, Gp + h->pol.w[L], slabW, (long)D * H, (long)D * H, sk);
      add_reduce(red, Gp + h->pol.b[L], slabC, D, D, sk);
    }
    g_phase = "P5.outbwd:";
    PORL_TRY(iql_launch(h, g, tile, true, s));
  }
  for (int l = L - 1; l >= 0; --l) {
    const int Kin = l == 0 ? S : H;
    if (l == 0) {
      const int64_t per = (int64_t)H * S;
      float* slabW = W + ws.slab_pa;
      Dw0Net dn{W + ws.dz_p[0], Gp + h->pol.w[0], Gp + h->pol.b[0], slabW, slabW + (int64_t)SK_MAX * per};
      int rc = 0;
      if (dw0_skinny(h, &dn, 1, W + ws.xs_slot[h->slot], h->Sp, B, H, S, Hp, red, "P7.dW0:", s, &rc)) {
        if (rc) return rc;
        break;
      }
    }
    const float* dz = W + ws.dz_p[l & 1];
    const float* in = l == 0 ? W + ws.xs_slot[h->slot] : W + ws.act_p[l - 1];
    const int ldin = l == 0 ? h->Sp : Hp;
    GemmGroup g{};
    g.p[g.nprob] = make_prob(GEMM_TN, dz, Hp, in, ldin, Gp + h->pol.w[l], Kin, H, Kin, B);
    g.p[g.nprob++].colsum = Gp + h->pol.b[l];
    if (l > 0) {
      GemmProb q = make_prob(GEMM_NN, dz, Hp, Pp + h->pol.w[l], Kin, W + ws.dz_p[(l - 1) & 1], Hp, B, Kin, H);
      q.mask = W + ws.act_p[l - 1]; q.ldmask = Hp;
      g.p[g.nprob++] = q;
    }
    const int tile = iql_tile(h, g);
    if (l == 0) {
      int bm, bn;
      tile_dims(tile, bm, bn);
      const int sk = pick_splitk(H, Kin, B, 1, bm, bn);
      if (sk > 1) {
        const int64_t per = (int64_t)H * Kin;
        float* slabW = W + ws.slab_pa;
        float* slabC = slabW + (int64_t)SK_MAX * per;
        g.p[0].splitk = sk; g.p[0].C = slabW; g.p[0].colsum = slabC;
        add_reduce(red, Gp + h->pol.w[0], slabW, per, per, sk);
        add_reduce(red, Gp + h->pol.b[0], slabC, H, H, sk);
      }
    }
    g_phase = l == 0 ? "P7.dW0:" : "P6.bwd:";
    PORL_TRY(iql_launch(h, g, tile, true, s));
  }
  g_phase = "P8.combine:";
  if (defer) *defer = red;
  else PORL_TRY(launch_reduce(red, s));
  g_phase = "";
  return PORL_OK;
}

int porl_iql_policy_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  return policy_backward_impl(h, hp, (hipStream_t)stream, nullptr, 1);
}

int porl_iql_policy_backward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  const bool fold = (h->mode & PORL_IQL_MODE_FOLD_COMBINE) != 0;
  h->fin_p = ReduceArgs{};
  PORL_TRY(policy_backward_impl(h, hp, (hipStream_t)stream, fold ? &h->fin_p : nullptr));
  h->fin_p_pending = fold;
  return PORL_OK;
}

// The whole update in one call.  Same arithmetic as the four phase calls; the two slab / partial-sum combines are
// folded into the Adam launches instead of running as launches of their own.
int porl_iql_step(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs fin{};
  PORL_TRY(value_backward_impl(h, hp, s, h->tune.iql_fold ? &fin : nullptr));
  g_phase = "V8.";
  PORL_TRY(adam_launch(h->buf.params_vf, h->buf.grads_vf, h->buf.adam_m_vf, h->buf.adam_v_vf, h->buf.params_tgt, h->n_vf,
                       hp->value_lr, hp->value_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, hp->ema_beta, s, &fin));
  fin = ReduceArgs{};
  PORL_TRY(policy_backward_impl(h, hp, s, h->tune.iql_fold ? &fin : nullptr));
  g_phase = "P9.";
  PORL_TRY(adam_launch(h->buf.params_pol, h->buf.grads_pol, h->buf.adam_m_pol, h->buf.adam_v_pol, nullptr, h->n_pol,
                       hp->policy_lr, hp->policy_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0, s, &fin));
  g_phase = "";
  return PORL_OK;
}

// Policy-only step (SORL.policy_update, reference agent/sorl.py:154-176 + the TD target of sorl.py:85-89): the value
// nets are read, never written.  Forward half = five forward-only nets per layer in one launch, policy_weight_kernel,
// mean, NLL; then the gradient half and Adam of the ordinary policy phase.  2 L + 5 launches at n_hidden = L (9 at L = 2;
// the joint update takes 14, each plus the minibatch load).
int porl_iql_policy_only_forward(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  h->pol_fwd_done = false;             // a forward half of the joint update's policy phase does not stand in for this one
  return policy_backward_impl(h, hp, (hipStream_t)stream, nullptr, 1, true);
}

// porl_iql_policy_only_forward + porl_iql_policy_backward + porl_iql_policy_apply in one call, the combine folded into
// the Adam launch (single-GPU update; batch must have been loaded).  stats[1] = g_loss, stats[2] = min NLL; stats[0],
// grads_vf, adam_*_vf, params_vf and params_tgt are not written.
int porl_iql_policy_only_step(porl_iql* h, const porl_iql_hyper* hp, void* stream) {
  PORL_TRY(check_ready(h, true)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  if (!h->have_pol_target) PORL_FAIL(PORL_ERR_INVALID, "policy step needs pol_target in porl_iql_load_batch");
  hipStream_t s = (hipStream_t)stream;
  h->pol_fwd_done = false;
  ReduceArgs fin{};
  PORL_TRY(policy_backward_impl(h, hp, s, h->tune.iql_fold ? &fin : nullptr, 3, true));
  g_phase = "O9.";
  PORL_TRY(adam_launch(h->buf.params_pol, h->buf.grads_pol, h->buf.adam_m_pol, h->buf.adam_v_pol, nullptr, h->n_pol,
                       hp->policy_lr, hp->policy_step, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, 0.0, s, &fin));
  g_phase = "";
  return PORL_OK;
}

// ---------------------------------------------------------------------------------------------------
static int pack_x(porl_iql* h, const float* x, int64_t x_rs, int batch, int64_t dst_off, hipStream_t s) {
  if (!x) PORL_FAIL(PORL_ERR_INVALID, "null input");
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
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
static bool small_fwd_fits(const porl_iql* h, int batch) {
  return batch >= 1 && batch <= SMALL_FWD_MAX_B &&
         sizeof(float) * (size_t)batch * std::max(h->cfg.obs_dim, h->cfg.hidden_dim) <= SMALL_FWD_LDS_BYTES;
}
static int check_forward_batch(const porl_iql* h, int batch) {
  // both paths write `batch` rows of scratch sized for max_batch rows
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  return PORL_OK;
}

// One Linear layer of up to 2 networks on a handful of rows (kernels.hpp: small_fwd_kernel).
static int small_fwd(int nnets, const float* const* Wt, const float* const* bias, const float* const* X, const long* ldx,
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

int porl_iql_forward_value(porl_iql* h, int which, const float* x, int64_t x_rs, int32_t batch, float* v1_out,
                           float* v2_out, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!v1_out || !v2_out) PORL_FAIL(PORL_ERR_INVALID, "null output");
  PORL_TRY(check_forward_batch(h, batch));
  hipStream_t s = (hipStream_t)stream;
  if (small_fwd_fits(h, batch) && !h->cfg.layer_norm && x) {
    // inference-sized batch: 3 GEMV launches straight from the caller's rows (no staging copy, no split-K)
    const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
    float* W = h->buf.workspace;
    const float* P = which ? h->buf.params_tgt : h->buf.params_vf;
    const float* in[2] = {x, x};
    long ldin[2] = {(long)x_rs, (long)x_rs};
    for (int l = 0; l <= L; ++l) {
      const float* Wt[2] = {P + h->v[0].w[l], P + h->v[1].w[l]};
      const float* bs[2] = {P + h->v[0].b[l], P + h->v[1].b[l]};
      float* out[2];
      long ldo[2];
      for (int i = 0; i < 2; ++i) {
        out[i] = l == L ? (i ? v2_out : v1_out) : W + h->ws.act_t[i][l & 1];
        ldo[i] = l == L ? 1 : h->Hp;
      }
      PORL_TRY(small_fwd(2, Wt, bs, in, ldin, out, ldo, l == L ? 1 : H, l == 0 ? S : H, batch, l == L ? ACT_NONE : ACT_RELU, s));
      for (int i = 0; i < 2; ++i) { in[i] = out[i]; ldin[i] = ldo[i]; }
    }
    return PORL_OK;
  }
  // uses the s' staging buffer and the target scratch activations; invalidates a loaded minibatch
  PORL_TRY(pack_x(h, x, x_rs, batch, h->ws.xn, s));
  h->batch = 0;
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden;
  float* W = h->buf.workspace;
  const float* P = which ? h->buf.params_tgt : h->buf.params_vf;
  int parts = 0;
  for (int l = 0; l < L; ++l) {
    FwdNet nets[2];
    for (int i = 0; i < 2; ++i) {
      FwdNet& f = nets[i];
      if (l == 0) { f.in = W + h->ws.xn; f.ldin = h->Sp; }
      else { f.in = W + h->ws.act_t[i][(l - 1) & 1]; f.ldin = h->Hp; }
      f.W = P + h->v[i].w[l]; f.b = P + h->v[i].b[l];
      const bool LN = h->cfg.layer_norm != 0;
      f.out = (l == L - 1 && !LN) ? nullptr : W + h->ws.act_t[i][l & 1];
      f.headw = P + h->v[i].w[L]; f.headout = W + h->ws.hp_t[i];
      if (LN) { f.ln_g = P + h->v[i].lnw[l]; f.ln_b = P + h->v[i].lnb[l]; }
    }
    PORL_TRY(fwd_hidden_layer(h, nets, 2, batch, l == 0 ? S : H, l == L - 1, &parts, false, s));
  }
  hipLaunchKernelGGL(head_finish_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, s, W + h->ws.hp_t[0], W + h->ws.hp_t[1],
                     P + h->v[0].b[L], P + h->v[1].b[L], parts, batch, v1_out, v2_out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_iql_forward_policy(porl_iql* h, const float* x, int64_t x_rs, int32_t batch, float* mean_out,
                            int64_t mean_rs, void* stream) {
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!mean_out) PORL_FAIL(PORL_ERR_INVALID, "null output");
  PORL_TRY(check_forward_batch(h, batch));
  hipStream_t s = (hipStream_t)stream;
  if (small_fwd_fits(h, batch) && x) {
    const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim;
    float* W = h->buf.workspace;
    const float* P = h->buf.params_pol;
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
  const int S = h->cfg.obs_dim, H = h->cfg.hidden_dim, L = h->cfg.n_hidden, D = h->cfg.pol_out_dim;
  float* W = h->buf.workspace;
  const float* P = h->buf.params_pol;
  for (int l = 0; l < L; ++l) {
    FwdNet f{};
    if (l == 0) { f.in = W + h->ws.xn; f.ldin = h->Sp; }
    else { f.in = W + h->ws.act_p[l - 1]; f.ldin = h->Hp; }
    f.W = P + h->pol.w[l]; f.b = P + h->pol.b[l]; f.out = W + h->ws.act_p[l];
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

// ---------------------------------------------------------------------------------------------------
int porl_gemm_f32(int mode, int tile, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B,
                  int32_t ldb, float* C, int32_t ldc, const float* bias, int act, const float* mask, int32_t ldmask,
                  int splitk, float* slab, void* stream) {
  if (mode < 0 || mode > 2) PORL_FAIL(PORL_ERR_INVALID, "mode must be 0..2");
  if (M < 1 || N < 1 || K < 0 || !A || !B || !C) PORL_FAIL(PORL_ERR_INVALID, "bad GEMM arguments");
  if (splitk > 1 && !slab) PORL_FAIL(PORL_ERR_INVALID, "splitk > 1 needs a slab buffer");
  if (splitk > 1 && ldc != N) PORL_FAIL(PORL_ERR_INVALID, "splitk > 1 needs a dense C (ldc == N)");
  DevGuard _dg(device_of(C));
  hipStream_t s = (hipStream_t)stream;
  GemmGroup g{};
  g.nprob = 1;
  g.p[0] = make_prob(mode, A, lda, B, ldb, C, ldc, M, N, K);
  if (tile < 0) tile = pick_tile(g, g_tune);
  if (tile >= TILE_COUNT) PORL_FAIL(PORL_ERR_INVALID, "tile must be -1..%d", TILE_COUNT - 1);
  if (splitk > 1) {
    g.p[0].splitk = splitk; g.p[0].C = slab;
    PORL_TRY(launch_group(g, tile, g_tune, s));
    // rows of the slab have stride ldc; combine all M*ldc floats (padding columns carry garbage that the
    // caller's ldc padding tolerates), then apply bias/act/mask per element
    if (mask) PORL_FAIL(PORL_ERR_UNSUPPORTED, "mask with splitk");
    const long n = (long)M * ldc;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024)), dim3(256), 0, s, C, slab,
                       splitk, n, n, bias, ldc, act);
    PORL_HIP(hipGetLastError());
    return PORL_OK;
  }
  g.p[0].bias = bias; g.p[0].act = act; g.p[0].mask = mask; g.p[0].ldmask = ldmask;
  if (g_dbg_a_scale && g_dbg_a_shift && mode == GEMM_NT) {
    g.p[0].apro = APRO_AFFINE_RELU; g.p[0].a_colscale = g_dbg_a_scale; g.p[0].a_colshift = g_dbg_a_shift;
  }
  if (g_dbg_resid) g.p[0].resid = g_dbg_resid;
  if (g_dbg_cstat) g.p[0].cstat = g_dbg_cstat;
  return launch_group(g, tile, g_tune, s);
}

// Descriptor-level launch of one group (tests/test_gemm_epilogues_gpu.py): every caller-set field of GemmProb, validated
// on the host so that nothing launch_tile would refuse, and nothing the kernel would silently ignore, reaches a launch.
int porl_gemm_f32_group(const porl_gemm_desc* probs, int32_t nprob, int tile, int single_buffer, void* stream) {
  if (!probs) PORL_FAIL(PORL_ERR_INVALID, "null descriptors");
  if (nprob < 1 || nprob > MAX_GROUP) PORL_FAIL(PORL_ERR_INVALID, "nprob %d outside [1,%d]", nprob, MAX_GROUP);
  if (tile < -1 || tile >= TILE_COUNT) PORL_FAIL(PORL_ERR_INVALID, "tile must be -1..%d", TILE_COUNT - 1);
  GemmGroup g{};
  g.nprob = nprob;
  g.single_buffer = single_buffer != 0;
  int n_apro = 0;
  bool vec = true;
  for (int i = 0; i < nprob; ++i) {
    const porl_gemm_desc& d = probs[i];
    if (d.mode < 0 || d.mode > 2) PORL_FAIL(PORL_ERR_INVALID, "problem %d: mode must be 0..2", i);
    if (!d.A || !d.B || !d.C) PORL_FAIL(PORL_ERR_INVALID, "problem %d: null A, B or C", i);
    if (d.M < 1 || d.N < 1 || d.K < 0) PORL_FAIL(PORL_ERR_INVALID, "problem %d: need M >= 1, N >= 1, K >= 0", i);
    if (d.headw && !d.headout) PORL_FAIL(PORL_ERR_INVALID, "problem %d: headw without headout", i);
    if (d.colsum && d.mode != GEMM_TN) PORL_FAIL(PORL_ERR_INVALID, "problem %d: colsum needs the TN layout (A stored (K, M))", i);
    if (d.rscale && d.rs_rows < 1) PORL_FAIL(PORL_ERR_INVALID, "problem %d: rscale needs rs_rows >= 1", i);
    if (d.rscale && !d.resid) PORL_FAIL(PORL_ERR_INVALID, "problem %d: rscale without resid", i);
    const bool apro = d.a_colscale || d.a_colshift;
    if (d.splitk > 1 && (d.bias || d.act || d.mask || d.headw || d.resid || d.cstat || apro))
      PORL_FAIL(PORL_ERR_UNSUPPORTED, "problem %d: splitk > 1 writes raw slabs: no bias, act, mask, head, resid, cstat or prologue", i);
    if ((d.mask || d.resid) && (d.cstat || d.headw))
      PORL_FAIL(PORL_ERR_UNSUPPORTED, "problem %d: mask / resid together with cstat / head", i);
    if (d.a_grp < 0 || (d.a_grp > 0 && (d.mode != GEMM_NT || d.a_seg_tiles < 1)))
      PORL_FAIL(PORL_ERR_INVALID, "problem %d: a gathered A (a_grp > 0) needs the NT layout and a_seg_tiles >= 1", i);
    if (d.reserved) PORL_FAIL(PORL_ERR_INVALID, "problem %d: reserved must be 0", i);
    // extents: a leading dimension shorter than the contiguous extent aliases rows (a gathered A reads a_seg_tiles
    // K-tiles per stored row, then jumps)
    const int a_ext = d.mode == GEMM_TN ? d.M : (d.a_grp > 0 && d.a_seg_tiles * GEMM_BK < d.K ? d.a_seg_tiles * GEMM_BK : d.K);
    const int b_ext = d.mode == GEMM_NT ? d.K : d.N;
    if (d.lda < a_ext || d.ldb < b_ext || d.ldc < d.N)
      PORL_FAIL(PORL_ERR_INVALID, "problem %d: lda %d / ldb %d / ldc %d below the contiguous extents %d / %d / %d", i,
                d.lda, d.ldb, d.ldc, a_ext, b_ext, d.N);
    if (d.mask && d.ldmask < d.N) PORL_FAIL(PORL_ERR_INVALID, "problem %d: ldmask %d < N", i, d.ldmask);
    if (d.a_grp > 0 ? (d.lda < 1 || d.a_grp_jump < 0 || d.a_seg_jump < 0) : (d.a_grp_jump || d.a_seg_tiles || d.a_seg_jump))
      PORL_FAIL(PORL_ERR_INVALID, "problem %d: a_grp_jump / a_seg_jump must be >= 0, and 0 (with a_seg_tiles) for a dense A", i);
    GemmProb p = make_prob(d.mode, d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K);
    if (p.a_vec && (d.a_grp_jump % 4 || d.a_seg_jump % 4))     // the jumps move 16-byte loads
      PORL_FAIL(PORL_ERR_INVALID, "problem %d: a_grp_jump / a_seg_jump must be multiples of 4 floats with a 16-byte-readable A", i);
    p.bias = d.bias; p.act = d.act; p.mask = d.mask; p.ldmask = d.ldmask;
    p.headw = d.headw; p.headout = d.headout; p.colsum = d.colsum;
    p.resid = d.resid; p.rscale = d.rscale; p.rs_rows = d.rs_rows >= 1 ? d.rs_rows : 1; p.rs_row0 = d.rs_row0;
    p.cstat = d.cstat;
    p.a_grp = d.a_grp; p.a_grp_jump = d.a_grp_jump; p.a_seg_tiles = d.a_seg_tiles; p.a_seg_jump = d.a_seg_jump;
    p.splitk = d.splitk > 1 ? d.splitk : 1;
    p.store_c = d.store_c != 0;
    if (apro) {
      if (!d.a_colscale || !d.a_colshift) PORL_FAIL(PORL_ERR_INVALID, "problem %d: the prologue needs a_colscale and a_colshift", i);
      if (d.mode != GEMM_NT) PORL_FAIL(PORL_ERR_UNSUPPORTED, "problem %d: the operand prologue exists for the NT layout only", i);
      if (d.K % GEMM_BK) PORL_FAIL(PORL_ERR_UNSUPPORTED, "problem %d: the operand prologue needs K %% %d == 0", i, GEMM_BK);
      if (!aligned16(d.a_colscale) || !aligned16(d.a_colshift))
        PORL_FAIL(PORL_ERR_INVALID, "problem %d: a_colscale / a_colshift must be 16-byte aligned", i);
      p.apro = APRO_AFFINE_RELU; p.a_colscale = d.a_colscale; p.a_colshift = d.a_colshift;
      ++n_apro;
    }
    vec = vec && p.a_vec && p.b_vec;
    g.p[i] = p;
  }
  if (tile < 0) tile = pick_tile(g, g_tune);
  if (n_apro) {                      // what launch_tile refuses for the prologue instantiations
    if (n_apro != nprob) PORL_FAIL(PORL_ERR_UNSUPPORTED, "a group shares the operand prologue: all problems or none");
    if (tile != TILE_128x64 && tile != TILE_64x64 && tile != TILE_128x96)
      PORL_FAIL(PORL_ERR_UNSUPPORTED, "the operand prologue exists on tiles 1, 3 and 4, not %d", tile);
    if (!vec) PORL_FAIL(PORL_ERR_UNSUPPORTED, "the operand prologue needs 16-byte-readable operands");
    const int max_k = g.single_buffer && tile == TILE_64x64 ? 512 : 1024;    // the scale / shift table lives in LDS
    for (int i = 0; i < nprob; ++i)
      if (g.p[i].K > max_k) PORL_FAIL(PORL_ERR_UNSUPPORTED, "problem %d: the operand prologue holds K <= %d", i, max_k);
  }
  DevGuard _dg(device_of(probs[0].C));
  return launch_group(g, tile, g_tune, (hipStream_t)stream);
}

int porl_adam_ema(float* p, const float* g, float* m, float* v, float* target, int64_t n, double lr, int32_t step,
                  double beta1, double beta2, double eps, double ema_beta, void* stream) {
  if (!p || !g || !m || !v) PORL_FAIL(PORL_ERR_INVALID, "null buffer");
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (target && !aligned16(target)))
    PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  DevGuard _dg(device_of(p));
  return adam_launch(p, const_cast<float*>(g), m, v, target, n, lr, step, beta1, beta2, eps, ema_beta, (hipStream_t)stream);
}

int porl_ema(float* target, const float* source, int64_t n, double ema_beta, void* stream) {
  if (!target || !source || n < 0 || n % 4) PORL_FAIL(PORL_ERR_INVALID, "need buffers and a multiple of 4 floats");
  if (!aligned16(target) || !aligned16(source)) PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  if (n == 0) return PORL_OK;
  DevGuard _dg(device_of(target));
  const long n4 = n / 4;
  ProfScope ps("ema_kernel", (hipStream_t)stream, 0.0, 12.0 * n);
  hipLaunchKernelGGL(ema_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, target, source, n4,
                     (float)(1.0 - ema_beta), (float)ema_beta);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_reduce_mean(const float* x, int32_t n, float* out, void* stream) {
  if (!x || !out || n < 1) PORL_FAIL(PORL_ERR_INVALID, "bad arguments");
  DevGuard _dg(device_of(out));
  ReduceArgs r{};
  add_reduce(r, out, x, 1, 1, n, 0, 1.0f / n);          // fixed summation order (multi_reduce_kernel)
  return launch_reduce(r, (hipStream_t)stream);
}

int porl_softmax_mask(const float* logits, int64_t ld, int32_t batch, int32_t n_actions, float threshold,
                      int32_t write_probs, float* mask_out, void* stream) {
  if (!logits || !mask_out || batch < 1 || n_actions < 1 || n_actions > 4096 || ld < n_actions)
    PORL_FAIL(PORL_ERR_INVALID, "bad softmax-mask arguments");
  DevGuard _dg(device_of(mask_out));
  hipLaunchKernelGGL(softmax_mask_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, batch,
                     n_actions, threshold, write_probs, mask_out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_gather_rows(const float* rows, int64_t row_stride, const int64_t* idx, int32_t n, int32_t width, float* out,
                     int64_t out_stride, void* stream) {
  if (!rows || !idx || !out || n < 0 || width < 1) PORL_FAIL(PORL_ERR_INVALID, "bad gather arguments");
  if (n == 0) return PORL_OK;
  DevGuard _dg(device_of(out));
  const int blocks = std::min(cdiv(n, 4), 2048);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, (long)row_stride, idx, n,
                     width, out, (long)out_stride);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_sample_indices(int64_t n_rows, int32_t batch, uint64_t seed, uint64_t step, int64_t base, int64_t* out,
                        void* stream) {
  if (n_rows < 1 || batch < 1 || batch > n_rows || !out) PORL_FAIL(PORL_ERR_INVALID, "need 1 <= batch <= n_rows");
  if (n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "n_rows too large");
  const int hb = feistel_half_bits(n_rows);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(sample_indices_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, (hipStream_t)stream, n_rows, batch,
                     seed, step, hb, base, (int64_t)0, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_epoch_indices(int64_t n_rows, int64_t first, int32_t count, uint64_t seed, uint64_t epoch, int64_t base,
                       int64_t* out, void* stream) {
  if (n_rows < 1 || count < 1 || first < 0 || first + count > n_rows || !out)
    PORL_FAIL(PORL_ERR_INVALID, "need 0 <= first, 1 <= count, first + count <= n_rows");
  if (n_rows > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "n_rows too large");
  const int hb = feistel_half_bits(n_rows);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(sample_indices_kernel, dim3(cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream, n_rows, count,
                     seed, epoch, hb, base, first, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// ---- prioritized replay: sum tree in HBM (per_tree.hpp) ------------------------------------------------------
int porl_per_update(double* tree, int64_t capacity, const int64_t* tree_idx, const double* td_error, int32_t n, double eps,
                    double alpha, int32_t* stamp, void* stream) {
  if (!tree || !tree_idx || !td_error || !stamp || capacity < 1 || n < 0) PORL_FAIL(PORL_ERR_INVALID, "bad arguments");
  if (n == 0) return PORL_OK;
  DevGuard _dg(device_of(tree));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(per_stamp_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, tree_idx, n, capacity, stamp);
  hipLaunchKernelGGL(per_set_leaves_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, tree, tree_idx, td_error, n, capacity, eps,
                     alpha, stamp);
  int levels = 0;                                                        // keep in step with per_levels() below
  for (int64_t v = 2 * capacity - 1; v > 1; v >>= 1) ++levels;          // depth of the deepest leaf
  hipLaunchKernelGGL(per_propagate_kernel, dim3(1), dim3(1024), 0, s, tree, tree_idx, n, levels);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_per_sample(const double* tree, int64_t capacity, const double* u, int32_t batch, int64_t n_entries, double beta,
                    int64_t* out_idx, double* out_prio, float* out_w, void* stream) {
  if (!tree || !u || !out_idx || !out_prio || !out_w || capacity < 1 || batch < 1 || n_entries < 1)
    PORL_FAIL(PORL_ERR_INVALID, "bad arguments");
  DevGuard _dg(device_of(tree));
  PerSampleArgs a{tree, capacity, u, batch, n_entries, beta, out_idx, out_prio, out_w};
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// ---- prioritized replay inside the online loop (per_online.hpp) -----------------------------------------------------
static int per_levels(int64_t capacity) {                               // the loop of porl_per_update above: keep in step
  int levels = 0;
  for (int64_t v = 2 * capacity - 1; v > 1; v >>= 1) ++levels;          // depth of the deepest leaf
  return levels;
}

int porl_per_record(double* tree, int64_t capacity, int64_t slot, double td_error, double eps, double alpha,
                    const float* state, const float* next_state, int32_t state_dim, int64_t action, float reward,
                    float done, const porl_qnet_mirror* store, void* stream) {
  if (!tree || !state || !next_state || !store || !store->states || !store->next_states || !store->actions ||
      !store->rewards || !store->dones)
    PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (capacity < 1 || store->capacity != capacity)
    PORL_FAIL(PORL_ERR_INVALID, "capacity %lld < 1 or the store holds %lld rows", (long long)capacity, (long long)store->capacity);
  if (state_dim < 1) PORL_FAIL(PORL_ERR_INVALID, "state_dim %d < 1", state_dim);
  if (state_dim > ONL_MAX_RECORD_S)
    PORL_FAIL(PORL_ERR_UNSUPPORTED, "state_dim %d > %d: too wide for the kernel arguments", state_dim, ONL_MAX_RECORD_S);
  if (slot < 0 || slot >= capacity) PORL_FAIL(PORL_ERR_INVALID, "slot %lld outside [0,%lld)", (long long)slot, (long long)capacity);
  DevGuard _dg(device_of(tree));
  PerRecordArgs a;
  a.states = store->states; a.next_states = store->next_states; a.actions = store->actions; a.rewards = store->rewards;
  a.dones = store->dones; a.tree = tree; a.capacity = capacity; a.slot = slot; a.action = action;
  a.td_error = td_error; a.eps = eps; a.alpha = alpha; a.reward = reward; a.done = done; a.S = state_dim;
  memcpy(a.x, state, sizeof(float) * state_dim);
  memcpy(a.x + state_dim, next_state, sizeof(float) * state_dim);
  hipLaunchKernelGGL(per_record_kernel, dim3(1), dim3(state_dim > 64 ? 256 : 64), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_per_sample_slots(const double* tree, int64_t capacity, const double* u, int32_t batch, int64_t n_entries,
                          double beta, int64_t* out_idx, int64_t* out_slots, float* out_w, float* out_wmean,
                          double* scratch, void* stream) {
  if (!tree || !u || !out_idx || !out_slots || !out_w || !out_wmean || !scratch) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (capacity < 1 || batch < 1 || n_entries < 1 || n_entries > capacity)
    PORL_FAIL(PORL_ERR_INVALID, "need capacity >= 1, batch >= 1, 1 <= n_entries <= capacity");
  DevGuard _dg(device_of(tree));
  PerSampleSlotsArgs a{tree, capacity, u, batch, n_entries, beta, out_idx, out_slots, out_w, out_wmean, scratch};
  hipLaunchKernelGGL(per_sample_slots_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_per_update_f32(double* tree, int64_t capacity, const int64_t* tree_idx, const float* td_abs, int32_t n, double eps,
                        double alpha, int32_t* stamp, void* stream) {
  if (!tree || !tree_idx || !td_abs || !stamp) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (capacity < 1 || n < 1) PORL_FAIL(PORL_ERR_INVALID, "need capacity >= 1 and n >= 1");
  DevGuard _dg(device_of(tree));
  const int threads = n >= 1024 ? 1024 : (n + 63) / 64 * 64;
  hipLaunchKernelGGL(per_update_f32_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, tree, tree_idx, td_abs, n, capacity,
                     eps, alpha, stamp, per_levels(capacity));
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_tune_set(const char* key, int value) { return tune_apply(g_tune, key, value); }

int porl_iql_tune_set(porl_iql* h, const char* key, int value) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  return tune_apply(h->tune, key, value);
}

// ---- stream signals: cross-stream ordering by 64-bit counters in signal memory ----------------------------------------
// (hipStreamWriteValue64 / hipStreamWaitValue64 on memory from hipExtMallocWithFlags(hipMallocSignalMemory): the command
// processor writes / polls a value in stream order.)  The pipelined update orders its two streams three times per
// update; as event record + stream-wait-event pairs each crossing showed up as 6-12 us of idle queue in the kernel
// trace even when the event had completed long before.
int porl_signal_create(void** out) {
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  int dev = 0, can = 0;
  PORL_HIP(hipGetDevice(&dev));
  PORL_HIP(hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev));
  if (!can) PORL_FAIL(PORL_ERR_UNSUPPORTED, "stream wait-value operations are not supported on this device");
  void* p = nullptr;
  PORL_HIP(hipExtMallocWithFlags(&p, 8, hipMallocSignalMemory));
  PORL_HIP(hipMemset(p, 0, 8));
  *out = p;
  return PORL_OK;
}
int porl_signal_destroy(void* sig) {
  if (sig) PORL_HIP(hipFree(sig));
  return PORL_OK;
}
int porl_signal_write(void* sig, uint64_t value, void* stream) {
  if (!sig) PORL_FAIL(PORL_ERR_INVALID, "null signal");
  PORL_HIP(hipStreamWriteValue64((hipStream_t)stream, sig, value, 0));
  return PORL_OK;
}
int porl_signal_wait_ge(void* sig, uint64_t value, void* stream) {
  if (!sig) PORL_FAIL(PORL_ERR_INVALID, "null signal");
  PORL_HIP(hipStreamWaitValue64((hipStream_t)stream, sig, value, hipStreamWaitValueGte, 0xFFFFFFFFFFFFFFFFull));
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
  PORL_TRY(check_ready(h, false)); DevGuard _dg(h->device);
  if (!hp) PORL_FAIL(PORL_ERR_INVALID, "null hyper-parameters");
  if (!sig_value || !sig_fwd || !sig_policy || seq < 1) PORL_FAIL(PORL_ERR_INVALID, "three signal counters and seq >= 1 are required");
  if (main_stream == side_stream) PORL_FAIL(PORL_ERR_INVALID, "the two phases need two streams");
  if (!(h->mode & PORL_IQL_MODE_TWO_SLOTS) || !(h->mode & PORL_IQL_MODE_FOLD_COMBINE))
    PORL_FAIL(PORL_ERR_INVALID, "pipelined updates need PORL_IQL_MODE_TWO_SLOTS | PORL_IQL_MODE_FOLD_COMBINE");
  // reject bad minibatch arguments before anything is enqueued (porl_iql_load_batch_sampled checks them again)
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  if (!rows || n_rows < batch || n_rows > (int64_t(1) << 40) || act_dim < 0 ||
      row_stride < 2 * (int64_t)h->cfg.obs_dim + 2 + act_dim)
    PORL_FAIL(PORL_ERR_INVALID, "bad replay rows (need batch <= n_rows <= 2^40, row stride >= 2*S+2+A)");
  if (target_is_action ? h->cfg.pol_out_dim != act_dim : h->cfg.pol_out_dim != h->cfg.obs_dim)
    PORL_FAIL(PORL_ERR_INVALID, "policy target width mismatch");
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

int porl_tune_set_ptr(const char* key, void* ptr) {
  if (!key) PORL_FAIL(PORL_ERR_INVALID, "null key");
  if (!strcmp(key, "qnet_stamps")) { g_qnet_stamps = (unsigned long long*)ptr; return PORL_OK; }
  if (!strcmp(key, "gemm_a_scale")) { g_dbg_a_scale = (const float*)ptr; return PORL_OK; }
  if (!strcmp(key, "gemm_a_shift")) { g_dbg_a_shift = (const float*)ptr; return PORL_OK; }
  if (!strcmp(key, "gemm_resid")) { g_dbg_resid = (const float*)ptr; return PORL_OK; }
  if (!strcmp(key, "gemm_cstat")) { g_dbg_cstat = (float*)ptr; return PORL_OK; }
  PORL_FAIL(PORL_ERR_INVALID, "unknown tuning key '%s'", key);
}

// the rasteriser alone on any row source (reads only): porl_state2costmap, and the encoder's dense patch path on rows of a
// replay store (encoder_api.inc)
static int costmap_rasterise(const RowSrc& src, int32_t batch, int32_t n_ang, int32_t n_dist, float* out, hipStream_t s) {
  // constants exactly as util/costmap.py:19-20,34,45 forms them (python doubles rounded to fp32 at the tensor op)
  const double pi = 3.14159265358979323846;
  const float dist_inc = (float)((4.0 + 1e-4) / n_dist);
  const float ang_inc = (float)((2.0 * pi + 1e-4) / n_ang);
  const float deg_min = (float)(-pi + (2.0 * pi + 2e-4) / n_ang), deg_max = (float)(pi - (2.0 * pi + 2e-4) / n_ang);
  const float dist_max = (float)(4.0 - 4.0 / n_dist);
  hipLaunchKernelGGL(costmap_kernel, dim3(n_ang, batch), dim3(std::min(256, n_dist)), 0, s, src, n_ang, n_dist, dist_inc,
                     ang_inc, deg_min, deg_max, dist_max, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_state2costmap(float* state, int64_t state_rs, int32_t batch, int32_t n_ang, int32_t n_dist, float* out,
                        void* stream) {
  if (!state || !out || batch < 1 || n_ang < 4 || n_dist < 4) PORL_FAIL(PORL_ERR_INVALID, "bad costmap arguments");
  if (batch > 65535) PORL_FAIL(PORL_ERR_INVALID, "batch > 65535");
  DevGuard _dg(device_of(out));
  hipStream_t s = (hipStream_t)stream;
  PORL_TRY(costmap_rasterise(RowSrc{state, (long)state_rs, nullptr, 0}, batch, n_ang, n_dist, out, s));
  const long n = (long)batch * (n_ang + 2);
  hipLaunchKernelGGL(clamp_gt8_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024)), dim3(256), 0, s, state,
                     (long)state_rs, n_ang + 2, batch);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

// ---- dataset labelling (astar.hpp) ---------------------------------------------------------------------------------
namespace {
// Grid and launch constants of a parameter set; every rejection names its argument.  No HIP call.
int astar_plan(const porl_astar_params& p, int64_t row_stride, int32_t n_values, AstarGrid* out) {
  const double vals[] = {p.resolution, p.robot_radius, p.min_x, p.max_x, p.min_y, p.max_y, p.range_lo, p.range_hi};
  for (double v : vals) if (!std::isfinite(v)) PORL_FAIL(PORL_ERR_INVALID, "params: every field must be finite");
  if (!(p.resolution > 0.0)) PORL_FAIL(PORL_ERR_INVALID, "params.resolution %g must be positive", p.resolution);
  if (p.robot_radius < 0.0) PORL_FAIL(PORL_ERR_INVALID, "params.robot_radius %g must not be negative", p.robot_radius);
  if (!(p.max_x > p.min_x) || !(p.max_y > p.min_y)) PORL_FAIL(PORL_ERR_INVALID, "params: need min_x < max_x and min_y < max_y");
  if (p.n_beams < 1) PORL_FAIL(PORL_ERR_INVALID, "params.n_beams %d must be positive", p.n_beams);
  if (p.pose_off < 0 || p.heading_off < 0 || p.goal_off < 0) PORL_FAIL(PORL_ERR_INVALID, "params: negative row offset");
  const int64_t need = std::max<int64_t>(std::max<int64_t>(p.n_beams, (int64_t)p.pose_off + 2),
                                         std::max<int64_t>((int64_t)p.heading_off + 1, (int64_t)p.goal_off + 2));
  if (row_stride < need)
    PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld shorter than the highest offset read (%lld floats)", (long long)row_stride,
              (long long)need);
  // cells per axis as the reference counts them: round() of the quotient, half to even (nearbyint in the default mode)
  const double wd = std::nearbyint((p.max_x - p.min_x) / p.resolution), hd = std::nearbyint((p.max_y - p.min_y) / p.resolution);
  if (wd < 1.0 || hd < 1.0) PORL_FAIL(PORL_ERR_INVALID, "params.resolution %g leaves no cell in the window", p.resolution);
  const double pcd = (wd + 2.0) * (hd + 2.0);
  if (wd * hd > (double)AS_MAX_PAIR || pcd > (double)AS_MAX_PADDED_CELLS || astar_lds_bytes((int64_t)pcd) > (size_t)AS_MAX_LDS_BYTES)
    PORL_FAIL(PORL_ERR_INVALID, "params.resolution %g: a %.0f x %.0f grid does not fit one workgroup (%.0f bytes of LDS needed, "
              "%d available; at most %d cells)", p.resolution, wd, hd, pcd * 4.0 + pcd / 8.0, AS_MAX_LDS_BYTES, AS_MAX_PAIR);
  const double sx = std::nearbyint((0.0 - p.min_x) / p.resolution), sy = std::nearbyint((0.0 - p.min_y) / p.resolution);
  if (sx < 0.0 || sx >= wd || sy < 0.0 || sy >= hd)
    PORL_FAIL(PORL_ERR_INVALID, "params: the robot's cell (%.0f, %.0f) lies outside the %.0f x %.0f grid", sx, sy, wd, hd);
  if ((double)n_values < wd * hd + 2.0)
    PORL_FAIL(PORL_ERR_INVALID, "n_values %d: value_table must cover path lengths up to cells + 1 = %.0f", n_values, wd * hd + 1.0);
  AstarGrid g;
  g.res = p.resolution; g.rr = p.robot_radius; g.min_x = p.min_x; g.min_y = p.min_y; g.range_lo = p.range_lo; g.range_hi = p.range_hi;
  g.w = (int32_t)wd; g.h = (int32_t)hd; g.pw = g.w + 2; g.pcells = (g.w + 2) * (g.h + 2);
  g.start_ix = (int32_t)sx; g.start_iy = (int32_t)sy;
  g.n_beams = p.n_beams; g.pose_off = p.pose_off; g.heading_off = p.heading_off; g.goal_off = p.goal_off;
  g.max_sweeps = g.w * g.h;
  *out = g;
  return PORL_OK;
}
}  // namespace

int porl_astar_label(const float* rows, int64_t row_stride, int64_t n_rows, const porl_astar_params* params,
                     const double* beam_dirs, const float* value_table, int32_t n_values, float* value, int32_t* path_len,
                     int32_t* status, int32_t* sweeps, void* stream) {
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (!params) PORL_FAIL(PORL_ERR_INVALID, "null params");
  if (!beam_dirs) PORL_FAIL(PORL_ERR_INVALID, "null beam_dirs");
  if (!value_table) PORL_FAIL(PORL_ERR_INVALID, "null value_table");
  if (!value) PORL_FAIL(PORL_ERR_INVALID, "null value");
  if (!path_len) PORL_FAIL(PORL_ERR_INVALID, "null path_len");
  if (!status) PORL_FAIL(PORL_ERR_INVALID, "null status");
  if (n_rows < 1 || n_rows >= (int64_t(1) << 31)) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^31)", (long long)n_rows);
  AstarGrid g;
  PORL_TRY(astar_plan(*params, row_stride, n_values, &g));
  const size_t lds = astar_lds_bytes(g.pcells);
  DevGuard _dg(device_of(status));
  PORL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&astar_label_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL(astar_label_kernel, dim3((unsigned)n_rows), dim3(AS_THREADS), lds, (hipStream_t)stream, rows,
                     (long)row_stride, g, beam_dirs, value_table, value, path_len, status, sweeps);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_prof_enable(int on) {
  g_prof.on = on != 0;
  g_prof.recs.clear();
  g_prof.pool_used = 0;
  return PORL_OK;
}

int porl_prof_read(porl_prof_entry* out, int max_entries) {
  if (!out || max_entries < 1) PORL_FAIL(PORL_ERR_INVALID, "bad profile buffer");
  PORL_HIP(hipDeviceSynchronize());
  const int nl = std::min<int>((int)g_prof.labels.size(), max_entries);
  for (int i = 0; i < nl; ++i) {
    memset(&out[i], 0, sizeof(out[i]));
    strncpy(out[i].name, g_prof.labels[i].c_str(), sizeof(out[i].name) - 1);
  }
  for (const ProfRec& r : g_prof.recs) {
    if (r.label >= nl) continue;
    float ms = 0.f;
    PORL_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
    out[r.label].launches += 1;
    out[r.label].total_ms += ms;
    out[r.label].flops += r.flops;
    out[r.label].bytes += r.bytes;
  }
  return nl;
}

}  // extern "C"

#include "qnet_api.inc"
#include "encoder_api.inc"
#include "iqn_api.inc"
#include "episodes_api.inc"
#include "partition_api.inc"
