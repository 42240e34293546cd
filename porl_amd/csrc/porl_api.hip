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
#include "per_vector.hpp"
#include "bcq_mask.hpp"
#include "astar.hpp"
#include "episodes.hpp"
#include "pairs.hpp"
#include "partition.hpp"
#include "colstats.hpp"
#include "navsim.hpp"
#include "navsim_discrete.hpp"
#include "dist_act.hpp"
#include "iqn_vector.hpp"
#include "bcq_act.hpp"
#include "expert.hpp"

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

// Raises Kernel's dynamic-LDS limit above the 64 KiB default whenever `bytes` exceeds what this process has already set
// for it: with a constant size once, on the first call (again only if that failed); with a shape's size whenever it grows.
// One record per kernel, so a launch site that needs several raised lists them one after another.
template <auto Kernel>
int dyn_lds_once(int bytes) {
  static int set = 0;
  if (bytes > set) {
    PORL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    set = bytes;
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

// half the bits of the Feistel permutation that draws distinct rows of an n_rows store (sample_indices_kernel and kin)
int feistel_half_bits(int64_t n_rows) {
  int bits = 1;
  while ((int64_t(1) << bits) < n_rows) ++bits;
  return std::max(1, (bits + 1) / 2);
}

// Adam(+EMA) over one flat group.  `fin` (optional): combine jobs that the backward pass left pending; those whose
// output lies inside the gradient buffer `g` are folded into this launch (short slab lists inside the float4 sweep,
// long ones as extra reduce+Adam blocks), the others (loss statistics) ride along as plain reduce blocks.
int adam_launch(float* p, float* g, float* m, float* v, float* tgt, int64_t n, double lr, int step,
                       double b1, double b2, double eps, double ema_beta, hipStream_t s, const ReduceArgs* fin = nullptr,
                       int32_t* plan = nullptr) {
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
  int32_t nplan[6] = {0, 0, 0, 0, 0, 0};      // porl_iql_adam_plan: regions, folded width 32 / 4, unfolded, skips, blocks
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
        ++nplan[0];
        continue;
      }
      if (inside) {
        if (off % 4) PORL_FAIL(PORL_ERR_INVALID, "gradient tensors start on 16-byte boundaries");
        j.adam_off = off;
        a.skip_lo[a.nskip] = off; a.skip_hi[a.nskip] = ru4(off + j.n); ++a.nskip;
        ++nplan[j.width == 4 ? 2 : 1];
      } else {
        j.adam_off = -1;
        ++nplan[3];
      }
      a.job_block0[a.r.njobs] = reduce_blocks;
      a.r.job[a.r.njobs++] = j;
      reduce_blocks += (int)((j.n + j.width - 1) / j.width);
    }
    a.job_block0[a.r.njobs] = reduce_blocks;
  }
  ProfScope ps("adam_ema_kernel", s, 0.0, (double)n * (tgt ? 36.0 : 28.0) + extra_bytes);
  a.reduce_blocks = reduce_blocks;
  if (plan) {
    nplan[4] = a.nskip; nplan[5] = reduce_blocks;
    std::copy(nplan, nplan + 6, plan);
  }
  hipLaunchKernelGGL(adam_ema_kernel, dim3(sweep_blocks + reduce_blocks), dim3(256), 0, s, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // namespace

// =====================================================================================================
extern "C" {

int porl_abi_version(void) { return PORL_ABI_VERSION; }
const char* porl_last_error(void) { return g_err.c_str(); }

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
  const CostmapGeom g = costmap_geom(n_ang, n_dist);
  hipLaunchKernelGGL(costmap_kernel, dim3(n_ang, batch), dim3(std::min(256, n_dist)), 0, s, src, n_ang, n_dist, g.dist_inc,
                     g.ang_inc, g.deg_min, g.deg_max, g.dist_max, out);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}
// the reference's in-place side effect (util/costmap.py:17) on a caller's own (batch, n_ang + 2) tensor
static int clamp_state(float* state, int64_t state_rs, int32_t n_ang, int32_t batch, hipStream_t s) {
  const long n = (long)batch * (n_ang + 2);
  hipLaunchKernelGGL(clamp_gt8_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 1024)), dim3(256), 0, s, state,
                     (long)state_rs, n_ang + 2, batch);
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
  return clamp_state(state, state_rs, n_ang, batch, s);
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

#include "iql_api.inc"
#include "qnet_api.inc"
#include "encoder_api.inc"
#include "iqn_api.inc"
#include "episodes_api.inc"
#include "partition_api.inc"
#include "colstats_api.inc"
#include "navsim_api.inc"
#include "navsim_discrete_api.inc"
#include "expert_api.inc"
#include "per_vector_api.inc"
