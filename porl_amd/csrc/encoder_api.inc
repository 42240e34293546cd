// Costmap encoder engine (porl_enc_*): host planning for FasterNet.forward_cls (reference
// agent/fasternet.py:428-438) on NHWC activations.  Included by porl_api.hip.
//
// Forward of one batch (B samples, P1 = (n_ang/4)*(n_dist/4) positions at stage 1, P2 = P1/4 at stage 2):
//   costmap image -> PatchEmbed 4x4s4 + BN -> MLPBlock(E) x depth0 -> PatchMerging 2x2s2 + BN
//   -> MLPBlock(2E) x depth1 -> global average pool -> 1x1 (2E -> feature_dim) + ReLU -> Linear(+bias)
// MLPBlock: y = [PConv3x3(x[:, :C/n_div]) | x[:, C/n_div:]];  x += drop_scale * W2 relu(BN(W1 y))
// Every convolution except the 4x4 patch embedding is a grouped fp32-MFMA GEMM over position rows.
//
// enc_forward_src is that sequence, one host function per step; fp32 or bf16 activations (`fused16`) is an `if` inside a step:
//   enc_pack_weights (if stale) -> enc_patch_embed (sparse | dense) -> enc_stage (enc_block | enc_block_bf16) -> enc_merge
//   (enc_merge_bf16 | enc_merge_gather | enc_merge_s2d, + BatchNorm) -> enc_stage -> enc_pool -> enc_head
// Packed weight images are sized by the functions beside their pack kernels; LDS limits are raised by dyn_lds_once alone.

#include "encoder.hpp"
#include "encoder_bf16.hpp"

namespace {

constexpr int ENC_LDS_LIMIT = 150 * 1024;   // the most dynamic LDS an encoder kernel is launched with (160 KiB per CU)

struct EncBn {
  int C = 0;
  int64_t gamma = 0, bias = 0;    // float offsets into params
  int64_t mean = 0, var = 0;      // float offsets into bn_stats
  int64_t alpha = 0, beta = 0;    // float offsets into workspace
};
struct EncBlock {
  int dim = 0, hidden = 0, cp = 0, stage = 0;
  int64_t w1 = 0, w2 = 0, wp = 0;   // params
  int64_t wp_packed = 0, wp_direct = 0;   // workspace: (oc,ky,kx,ci) for the patch-matrix GEMM, (ky,ci,kx,oc) direct
  int64_t w1_bf16 = 0, w2_bf16 = 0, wp_bf16 = 0;   // workspace (bf16-activation mode): bf16 copies, encoder_bf16.hpp layouts
  int64_t wp_mfma = 0;                             // workspace: [pass][tap][32][cp + 4] image of pconv_f32_mfma_kernel
  EncBn bn;
};
struct EncTensor { std::string name; int64_t off; int64_t numel; };
struct EncBnInfo { std::string name; EncBn* bn; };

}  // namespace

struct porl_enc {
  porl_enc_cfg cfg{};
  int Hp = 0, Wp = 0, H2 = 0, W2 = 0, P1 = 0, P2 = 0, E = 0, E2 = 0;
  std::vector<EncTensor> tensors;
  std::vector<EncBlock> blocks;
  EncBn bn_patch, bn_merge;
  std::vector<EncBnInfo> bns;
  int64_t w_patch = 0, w_merge = 0, w_pre = 0, w_head = 0, b_head = 0;
  int64_t n_params = 0, n_stats = 0, n_ws = 0;
  // workspace offsets (floats)
  int64_t ws_img = 0, ws_x1 = 0, ws_y = 0, ws_h = 0, ws_col = 0, ws_x2 = 0, ws_pool = 0, ws_feat = 0, ws_wmerge = 0,
          ws_partial = 0, ws_cstat = 0;
  float* params = nullptr;
  float* stats = nullptr;
  float* W = nullptr;
  bool bound = false;
  bool packed_valid = false;        // the permuted copies of the conv weights in the workspace are current
  bool bf16_fused = false;          // cfg.bf16_operands == 2 and the shape is one encoder_bf16.hpp is instantiated for
  int64_t ws_wmerge_bf16 = 0;
  int device = -1;
  Tune tune = g_tune;               // kernel selection: the process defaults at creation
};

namespace {

int64_t enc_add_tensor(porl_enc* h, const std::string& name, int64_t numel) {
  const int64_t off = h->n_params;
  h->tensors.push_back({name, off, numel});
  h->n_params += ru4(numel);
  return off;
}

void enc_add_bn(porl_enc* h, EncBn* bn, const std::string& name, int C) {
  bn->C = C;
  bn->gamma = enc_add_tensor(h, name + ".weight", C);
  bn->bias = enc_add_tensor(h, name + ".bias", C);
  bn->mean = h->n_stats; h->n_stats += ru4(C);
  bn->var = h->n_stats; h->n_stats += ru4(C);
  h->bns.push_back({name, bn});
}

int64_t enc_ws(porl_enc* h, int64_t n) {
  const int64_t off = h->n_ws;
  h->n_ws += ru4(n);
  return off;
}

// The forward's two branch predicates, shared with porl_enc_tap_info so the query cannot drift from what ran.
// sparse patch embedding: straight from the lidar state (weight + one patch row of masks fit in LDS)
bool enc_sparse_patch(const porl_enc* h) {
  return h->E <= PE_MAX_E && !h->tune.enc_dense_patch && (size_t)PE_K * h->E * sizeof(float) + (size_t)h->P1 * 12 <= ENC_LDS_LIMIT;
}
// bf16-activation mode: needs the sparse patch embedding (it writes bf16 directly); otherwise the bf16-operand mode
bool enc_fused16(const porl_enc* h) { return h->bf16_fused && enc_sparse_patch(h) && !h->tune.enc_bf16_operands_only; }

inline unsigned sweep_blocks(long items) { return (unsigned)std::min<long>((items + 255) / 256, 256L * 32); }

// (rows, K) x (N, K)^T over position rows, split into problems whose operands stay below the 2 GiB reach
// of a buffer descriptor, up to MAX_GROUP problems per launch
struct EncEpi {
  const float* resid = nullptr;    // C = resid + rscale[row / rs_rows] * acc (resid may be C itself)
  const float* rscale = nullptr;
  int rs_rows = 1;
  float* cstat = nullptr;          // per-32-row column sums / sums of squares of C, (rows/32, 2, N)
  const float* a_scale = nullptr;  // A-operand prologue: a = max(A * a_scale[k] + a_shift[k], 0)  (BatchNorm + ReLU of the
  const float* a_shift = nullptr;  // producer folded into this product's operand staging; K % 32 == 0)
  bool bf16 = false;               // operands rounded to bf16, fp32 accumulate (gemm_bf16.hpp)
};

int enc_gemm_rows(const porl_enc* h, hipStream_t s, const float* A, int lda, long rows, const float* Wt, int N, int K, float* C, int ldc,
                  const float* bias, int act, const EncEpi& epi = EncEpi()) {
  const long reach = ((1L << 31) - (1L << 20)) / (4L * std::max(lda, ldc));
  const long chunk = std::max<long>(128, reach & ~127L);
  long done = 0;
  while (done < rows) {
    GemmGroup g{};
    while (done < rows && g.nprob < MAX_GROUP) {
      const long m = std::min(chunk, rows - done);
      GemmProb p = make_prob(GEMM_NT, A + done * lda, lda, Wt, K, C + done * ldc, ldc, (int)m, N, K);
      p.bias = bias; p.act = act;
      if (epi.resid) {
        p.resid = epi.resid + done * ldc; p.rscale = epi.rscale; p.rs_rows = epi.rs_rows; p.rs_row0 = (int)(done % epi.rs_rows);
        if (p.rscale) p.rscale += done / epi.rs_rows;
      }
      if (epi.cstat) p.cstat = epi.cstat + (done / 32) * 2 * N;
      if (epi.a_scale) { p.apro = APRO_AFFINE_RELU; p.a_colscale = epi.a_scale; p.a_colshift = epi.a_shift; }
      g.p[g.nprob++] = p;
      done += m;
    }
    // huge M, small K: three co-resident 64x64 blocks per CU (154 registers) hide the ~5 us of descriptor +
    // first-load latency and the C store behind each other's 1-3 us of MFMA work; the register-heavy 128x128 tile
    // (one block per CU) cannot.  Measured on these shapes: scripts/bench_gemm_enc.py, scripts/bench_stamp_enc.py.
    // (with the residual epilogue the 64x64 tile also wins at K = 384: 1 077 vs 1 211 us on 737 k x 192 x 384,
    //  scripts/bench_gemm_enc.py VARIANTS=apro+resid)
    // Tile and schedule for the row products (millions of rows, 3-12 K-tiles per block).  Measured, updates/s at 360x256
    // B = 512 (gpurun_out/r03/t96, pf2, sb): MFMA-paced double-buffered 64x64 blocks everywhere 38.5; + 128x96 blocks for
    // the N = 96 product 39.9; SINGLE-buffered 64x64 blocks (`single_buffer`: 18 KB of LDS and 44 registers, eight
    // blocks per CU instead of four) 42.1 with, 44.8 without the 128x96 exception — a block spends ~5 us fetching its
    // first operands and ~2.5 us storing C around 1.5-3 us of matrix work, and only co-resident blocks fill that.
    // porl_tune_set("enc_gemm_sb", 0) / ("enc_tile_n96", 1) bring the other forms back (A/B; results are bit-identical).
    const bool n96 = N == 96 && h->tune.enc_tile_n96;
    const int tile = (rows >= 4096 && n96 && !epi.bf16) ? TILE_128x96
                     : (rows >= 4096 || epi.a_scale || epi.bf16)
                         ? ((K >= 384 && !(epi.resid && !epi.bf16)) ? TILE_128x64 : TILE_64x64) : pick_tile(g, h->tune);
    g.single_buffer = (rows >= 4096 && tile == TILE_64x64 && h->tune.enc_gemm_sb && K <= 512) ? 1 : 0;
    if (epi.bf16) PORL_TRY(launch_group_bf16(g, tile, s));
    else PORL_TRY(launch_group(g, tile, h->tune, s));
  }
  return 0;
}

// `nblocks` partial sums (eval: none, the running statistics) -> bn's folded scale / shift.  The caller owns the ProfScope.
int enc_bn_finish(porl_enc* h, const EncBn& bn, const double* partial, int nblocks, long rows, int training, hipStream_t s) {
  hipLaunchKernelGGL(bn_finish_kernel, dim3(bn.C), dim3(64), 0, s, partial, nblocks, bn.C, rows, h->params + bn.gamma,
                     h->params + bn.bias, h->stats + bn.mean, h->stats + bn.var, training, (double)h->cfg.bn_eps,
                     (double)h->cfg.bn_momentum, h->W + bn.alpha, h->W + bn.beta);
  PORL_HIP(hipGetLastError());
  return 0;
}

// apply = false: only the statistics and the folded scale / shift (W + bn.alpha, W + bn.beta) are produced; the
// consumer applies them while it stages x (EncEpi::a_scale)
int enc_batchnorm(porl_enc* h, const EncBn& bn, float* x, long rows, int relu, int training, hipStream_t s,
                  const float* cstat = nullptr, bool apply = true, int cstat_rows = 32) {
  const int C = bn.C;
  int nblocks = 0;
  double* partial = reinterpret_cast<double*>(h->W + h->ws_partial);
  if (training && cstat) {
    const long nrb = (rows + cstat_rows - 1) / cstat_rows;      // entries of cstat: one per cstat_rows rows
    nblocks = (int)std::min<long>(1024, std::max<long>(1, nrb / 16));
    ProfScope ps("colstats_from_blocks_kernel", s, 0.0, 8.0 * nrb * C);
    hipLaunchKernelGGL(colstats_from_blocks_kernel, dim3(nblocks), dim3(256), 0, s, cstat, nrb, C, partial);
    PORL_HIP(hipGetLastError());
  } else if (training) {
    const int rows_par = 256 / (C / 4);
    nblocks = (int)std::min<long>(CS_MAX_BLOCKS, std::max<long>(1, rows / (rows_par * 8L)));
    ProfScope ps("colstats_partial_kernel", s, 0.0, 4.0 * rows * C);
    hipLaunchKernelGGL(colstats_partial_kernel, dim3(nblocks), dim3(256), (size_t)rows_par * 2 * C * sizeof(double), s, x,
                       rows, C, partial);
    PORL_HIP(hipGetLastError());
  }
  {
    ProfScope ps("bn_finish_kernel", s, 0.0, 0.0);
    PORL_TRY(enc_bn_finish(h, bn, partial, nblocks, rows, training, s));
  }
  if (!apply) return 0;
  const long n4 = rows * (C / 4);
  ProfScope ps("bn_apply_kernel", s, 0.0, 8.0 * rows * C);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(sweep_blocks(n4)), dim3(256), 0, s, x, x, n4, C / 4, h->W + bn.alpha,
                     h->W + bn.beta, relu);
  PORL_HIP(hipGetLastError());
  return 0;
}

// Partial_conv3 of one block: direct kernels for the reference's two shapes, patch matrix + GEMM otherwise
template <int CP, int OCB, int WW>
int enc_pconv_launch(const float* x, const float* w, float* y, int batch, int Hh, int C, hipStream_t s) {
  constexpr int TR = 64 / (WW / 4);
  const size_t lds = (size_t)((TR + 2) * CP * (WW + 8)) * sizeof(float);
  PORL_TRY((dyn_lds_once<&pconv3x3_kernel<CP, OCB, WW>>((int)lds)));
  ProfScope ps("pconv3x3_kernel", s, 2.0 * batch * Hh * WW * 9.0 * CP * CP, 8.0 * batch * Hh * WW * C);
  hipLaunchKernelGGL((pconv3x3_kernel<CP, OCB, WW>), dim3(cdiv(Hh, TR), batch, CP / OCB), dim3(64 * (OCB / 8)), lds, s, x,
                     w, y, Hh, C);
  PORL_HIP(hipGetLastError());
  return 0;
}

template <int CP>
int enc_pconv_mfma_launch(const float* x, const float* w, float* y, int batch, int Hh, int Ww, int C, hipStream_t s) {
  PconvMfmaArgs a{};
  a.x = x; a.y = y; a.w = w; a.C = C; a.Hh = Hh; a.Ww = Ww;
  a.tiles_per_sample = cdiv(Hh * Ww, 128);
  a.tiles_total = batch * a.tiles_per_sample;
  // one 32-channel pass: the weight stays parked, a block walks several tiles; two passes: one tile per block
  a.tiles_per_block = CP <= 32 ? std::max(1, std::min(8, a.tiles_total / (2 * NUM_CU))) : 1;
  const int lds = 4 * (pconv_mfma_pass_floats(CP) + (128 / Ww + 4) * (Ww + 2) * (CP + 4));   // weights + rows with halo
  if (lds > ENC_LDS_LIMIT) return -1;                           // caller falls back to the direct / patch-matrix kernels
  PORL_TRY(dyn_lds_once<&pconv_f32_mfma_kernel<CP>>(lds));
  const double rows = (double)batch * Hh * Ww;
  ProfScope ps("pconv_f32_mfma_kernel", s, 2.0 * rows * 9.0 * CP * CP, 8.0 * rows * C);
  hipLaunchKernelGGL(pconv_f32_mfma_kernel<CP>, dim3(cdiv(a.tiles_total, a.tiles_per_block)), dim3(256), lds, s, a);
  PORL_HIP(hipGetLastError());
  return 0;
}

int enc_pconv(porl_enc* h, const EncBlock& b, const float* x, float* y, float* col, long rows, int Hh, int Ww,
              hipStream_t s) {
  const int batch = (int)(rows / ((long)Hh * Ww));
  if (h->tune.enc_pconv_mfma && b.dim % 4 == 0 && (b.cp == 24 || b.cp == 48)) {
    const int rc = b.cp == 24 ? enc_pconv_mfma_launch<24>(x, h->W + b.wp_mfma, y, batch, Hh, Ww, b.dim, s)
                              : enc_pconv_mfma_launch<48>(x, h->W + b.wp_mfma, y, batch, Hh, Ww, b.dim, s);
    if (rc >= 0) return rc;
  }
  if (b.cp == 24 && Ww == 64) return enc_pconv_launch<24, 24, 64>(x, h->W + b.wp_direct, y, batch, Hh, b.dim, s);
  if (b.cp == 48 && Ww == 32) return enc_pconv_launch<48, 48, 32>(x, h->W + b.wp_direct, y, batch, Hh, b.dim, s);
  {
    const long items = rows * (9L * (b.cp / 4) + (b.dim - b.cp) / 4);
    ProfScope ps("im2col3x3_kernel", s, 0.0, 4.0 * rows * (9.0 * b.cp + 2.0 * b.dim));
    hipLaunchKernelGGL(im2col3x3_kernel, dim3(sweep_blocks(items)), dim3(256), 0, s, x, col, y, rows, Hh, Ww, b.dim, b.cp);
    PORL_HIP(hipGetLastError());
  }
  EncEpi ep;
  ep.bf16 = h->cfg.bf16_operands != 0;
  return enc_gemm_rows(h, s, col, 9 * b.cp, rows, h->W + b.wp_packed, b.cp, 9 * b.cp, y, b.dim, nullptr, ACT_NONE, ep);
}

// one MLPBlock on x (rows, dim) in place; H x W is the position grid of its stage
int enc_block(porl_enc* h, const EncBlock& b, float* x, long rows, int Hh, int Ww, const float* scale, int training,
              hipStream_t s) {
  float* W = h->W; float* col = W + h->ws_col; float* y = W + h->ws_y; float* hid = W + h->ws_h;
  PORL_TRY(enc_pconv(h, b, x, y, col, rows, Hh, Ww, s));
  // W1 with the BatchNorm column statistics gathered in its epilogue; W2 adds the (DropPath-scaled) product onto
  // the shortcut in its epilogue, in place: x = x + scale * (hid W2^T)   (MLPBlock.forward, fasternet.py:186-190)
  EncEpi e1, e2;
  e1.bf16 = e2.bf16 = h->cfg.bf16_operands != 0;
  if (training) e1.cstat = W + h->ws_cstat;
  PORL_TRY(enc_gemm_rows(h, s, y, b.dim, rows, h->params + b.w1, b.hidden, b.dim, hid, b.hidden, nullptr, ACT_NONE, e1));
  // BatchNorm + ReLU of the hidden activation: folded into W2's operand staging when the shape allows (the hidden
  // tensor is then read once instead of read + written + read), a separate sweep otherwise
  const bool fold = (b.hidden % GEMM_BK == 0 || e2.bf16) && b.hidden <= 1024 && !h->tune.enc_bn_sweep;
  PORL_TRY(enc_batchnorm(h, b.bn, hid, rows, 1, training, s, e1.cstat, !fold));
  if (fold) { e2.a_scale = W + b.bn.alpha; e2.a_shift = W + b.bn.beta; }
  e2.resid = x; e2.rscale = scale; e2.rs_rows = Hh * Ww;
  PORL_TRY(enc_gemm_rows(h, s, hid, b.hidden, rows, h->params + b.w2, b.dim, b.hidden, x, b.dim, nullptr, ACT_NONE, e2));
  return 0;
}

// ---- bf16-activation mode (encoder_bf16.hpp) ---------------------------------------------------------------------------
template <int CP, int CPP, int CPN, int POS>
int enc_pconv_bf16_launch(const __bf16* x, int ldx, const __bf16* w, __bf16* yc, int batch, int Hh, int Ww, hipStream_t s) {
  static_assert(CPP == pconv_bf16_cpp(CP) && CPN == pconv_bf16_cpn(CP), "the kernel's padding is the packed image's");
  PconvBf16Args a{};
  a.x = x; a.yc = yc; a.w = w; a.ldx = ldx; a.Hh = Hh; a.Ww = Ww;
  a.tiles_per_sample = cdiv(Hh * Ww, POS);
  a.nr_max = POS / Ww + 4;
  a.tiles_total = batch * a.tiles_per_sample;
  // enough tiles per block to amortise the weight's trip into LDS (23 / 83 KB), enough blocks to fill the chip twice
  a.tiles_per_block = std::max(1, std::min(8, a.tiles_total / (2 * NUM_CU)));
  const int lds = 2 * (pconv_bf16_image_elems(CP) + a.nr_max * (Ww + 2) * (CPP + 8));
  if (lds > ENC_LDS_LIMIT) PORL_FAIL(PORL_ERR_UNSUPPORTED, "partial conv tile does not fit in LDS (%d bytes)", lds);
  PORL_TRY((dyn_lds_once<&pconv_bf16_kernel<CP, CPP, CPN, POS>>(lds)));
  const double rows = (double)batch * Hh * Ww;
  ProfScope ps("pconv_bf16_kernel", s, 2.0 * rows * 9.0 * CP * CP, 2.0 * rows * 2.0 * CP);
  hipLaunchKernelGGL((pconv_bf16_kernel<CP, CPP, CPN, POS>), dim3(cdiv(a.tiles_total, a.tiles_per_block)), dim3(256), lds, s, a);
  PORL_HIP(hipGetLastError());
  return 0;
}

template <int DIM, int HID, int CP>
int enc_mlp_bf16_launch(porl_enc* h, const EncBlock& b, __bf16* x, const __bf16* yc, long rows, const float* scale, int rs_rows,
                        int training, hipStream_t s) {
  float* W = h->W;
  EncMlpArgs a{};
  a.x = x; a.yc = yc;
  a.w1 = reinterpret_cast<const __bf16*>(W + b.w1_bf16); a.w2 = reinterpret_cast<const __bf16*>(W + b.w2_bf16);
  a.alpha = W + b.bn.alpha; a.beta = W + b.bn.beta; a.rscale = scale; a.rs_rows = rs_rows;
  a.cstat = W + h->ws_cstat; a.out = x; a.rows = rows;
  const unsigned grid = (unsigned)((rows + 127) / 128);            // one 128-row tile per block (see PFA in the kernel)
  constexpr int LDS1 = enc_mlp_lds_bytes<DIM, HID, CP>(1), LDS2 = enc_mlp_lds_bytes<DIM, HID, CP>(2);
  PORL_TRY((dyn_lds_once<&enc_mlp_bf16_kernel<DIM, HID, CP, 1>>(LDS1)));
  PORL_TRY((dyn_lds_once<&enc_mlp_bf16_kernel<DIM, HID, CP, 2>>(LDS2)));
  if (training) {                                                  // the statistics pass: column sums per 128 rows
    ProfScope ps("enc_mlp_bf16_kernel<stats>", s, 2.0 * rows * DIM * HID, 2.0 * rows * DIM);
    hipLaunchKernelGGL((enc_mlp_bf16_kernel<DIM, HID, CP, 1>), dim3(grid), dim3(256), LDS1, s, a);
    PORL_HIP(hipGetLastError());
  }
  PORL_TRY(enc_batchnorm(h, b.bn, nullptr, rows, 1, training, s, training ? a.cstat : nullptr, false, 128));
  ProfScope ps("enc_mlp_bf16_kernel<apply>", s, 4.0 * rows * DIM * HID, 2.0 * rows * (2.0 * DIM + CP));
  hipLaunchKernelGGL((enc_mlp_bf16_kernel<DIM, HID, CP, 2>), dim3(grid), dim3(256), LDS2, s, a);
  PORL_HIP(hipGetLastError());
  return 0;
}

// one MLPBlock on bf16 x (rows, dim) in place
int enc_block_bf16(porl_enc* h, const EncBlock& b, __bf16* x, long rows, int Hh, int Ww, const float* scale, int training,
                   hipStream_t s) {
  float* W = h->W; __bf16* yc = reinterpret_cast<__bf16*>(W + h->ws_y);
  const __bf16* wp = reinterpret_cast<const __bf16*>(W + b.wp_bf16);
  const int batch = (int)(rows / ((long)Hh * Ww));
  if (b.cp == 24) {
    PORL_TRY((enc_pconv_bf16_launch<24, 32, 32, 128>(x, b.dim, wp, yc, batch, Hh, Ww, s)));
    return enc_mlp_bf16_launch<96, 192, 24>(h, b, x, yc, rows, scale, Hh * Ww, training, s);
  }
  PORL_TRY((enc_pconv_bf16_launch<48, 48, 64, 64>(x, b.dim, wp, yc, batch, Hh, Ww, s)));
  return enc_mlp_bf16_launch<192, 384, 48>(h, b, x, yc, rows, scale, Hh * Ww, training, s);
}
}  // namespace

extern "C" {

int porl_enc_create(const porl_enc_cfg* c, porl_enc** out) {
  if (!c || !out) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  // 4x4s4 patches need multiples of 4; the 2x2s2 merge takes floor(./2) like Conv2d(stride 2) does on an odd grid
  // (fasternet.py:253 — e.g. an 84 x 84 costmap: 21 x 21 patches -> 10 x 10 merged positions)
  if (c->n_ang < 8 || c->n_dist < 8 || c->n_ang % 4 || c->n_dist % 4)
    PORL_FAIL(PORL_ERR_INVALID, "costmap size must be a multiple of 4, >= 8, in both directions");
  if (c->embed_dim < 32 || c->embed_dim % 32) PORL_FAIL(PORL_ERR_INVALID, "embed_dim must be a multiple of 32");
  if (c->n_div < 1 || (c->embed_dim / c->n_div) % 4 || c->embed_dim % c->n_div)
    PORL_FAIL(PORL_ERR_INVALID, "embed_dim / n_div must be a multiple of 4");
  if (c->depth0 < 1 || c->depth1 < 1 || c->depth0 + c->depth1 > PORL_ENC_MAX_BLOCKS)
    PORL_FAIL(PORL_ERR_INVALID, "1 <= depth0, depth1 and depth0 + depth1 <= %d", PORL_ENC_MAX_BLOCKS);
  const int hid0 = (int)(c->embed_dim * c->mlp_ratio), hid1 = (int)(2 * c->embed_dim * c->mlp_ratio);
  if (hid0 < 4 || hid0 % 4 || hid1 % 4 || hid1 > 1024) PORL_FAIL(PORL_ERR_INVALID, "mlp hidden width must be a multiple of 4, <= 1024");
  if (c->feature_dim < 4 || c->feature_dim % 4 || c->num_classes < 1 || c->max_batch < 1)
    PORL_FAIL(PORL_ERR_INVALID, "bad head sizes or max_batch");
  if (c->max_batch > 65535) PORL_FAIL(PORL_ERR_INVALID, "max_batch > 65535");
  porl_enc* h = new porl_enc();
  h->cfg = *c;
  h->E = c->embed_dim; h->E2 = 2 * c->embed_dim;
  h->Hp = c->n_ang / 4; h->Wp = c->n_dist / 4; h->H2 = h->Hp / 2; h->W2 = h->Wp / 2;
  h->P1 = h->Hp * h->Wp; h->P2 = h->H2 * h->W2;
  const int E = h->E, E2 = h->E2;
  // parameters in the reference's state_dict order and layouts (fasternet.py:264-378)
  h->w_patch = enc_add_tensor(h, "patch_embed.proj.weight", (int64_t)E * 48);
  enc_add_bn(h, &h->bn_patch, "patch_embed.norm", E);
  h->blocks.resize(c->depth0 + c->depth1);
  for (int i = 0; i < c->depth0 + c->depth1; ++i) {
    EncBlock& b = h->blocks[i];
    b.stage = i < c->depth0 ? 0 : 1;
    b.dim = b.stage == 0 ? E : E2;
    b.hidden = (int)(b.dim * c->mlp_ratio);
    b.cp = b.dim / c->n_div;
    if (i == c->depth0) {
      h->w_merge = enc_add_tensor(h, "stages.1.reduction.weight", (int64_t)E2 * E * 4);
      enc_add_bn(h, &h->bn_merge, "stages.1.norm", E2);
    }
    const std::string pre = "stages." + std::to_string(b.stage == 0 ? 0 : 2) + ".blocks." +
                            std::to_string(b.stage == 0 ? i : i - c->depth0);
    b.w1 = enc_add_tensor(h, pre + ".mlp.0.weight", (int64_t)b.hidden * b.dim);
    enc_add_bn(h, &b.bn, pre + ".mlp.1", b.hidden);
    b.w2 = enc_add_tensor(h, pre + ".mlp.3.weight", (int64_t)b.dim * b.hidden);
    b.wp = enc_add_tensor(h, pre + ".spatial_mixing.partial_conv3.weight", (int64_t)b.cp * b.cp * 9);
  }
  h->w_pre = enc_add_tensor(h, "avgpool_pre_head.1.weight", (int64_t)c->feature_dim * E2);
  h->w_head = enc_add_tensor(h, "head.weight", (int64_t)c->num_classes * c->feature_dim);
  h->b_head = enc_add_tensor(h, "head.bias", c->num_classes);
  // bns was filled with pointers into h->blocks after the resize, so they are stable

  const int64_t Bm = c->max_batch;
  const int hidmax_rows1 = h->blocks[0].hidden;                // per stage-1 position
  const int hid2 = h->blocks[c->depth0].hidden;
  h->ws_img = enc_ws(h, Bm * 3 * c->n_ang * c->n_dist);
  h->ws_x1 = enc_ws(h, Bm * h->P1 * E);
  h->ws_y = enc_ws(h, Bm * std::max<int64_t>((int64_t)h->P1 * E, (int64_t)h->P2 * E2));
  h->ws_h = enc_ws(h, Bm * std::max<int64_t>((int64_t)h->P1 * hidmax_rows1, (int64_t)h->P2 * hid2));
  const int64_t col1 = (int64_t)h->P1 * 9 * (E / c->n_div), col2 = (int64_t)h->P2 * 9 * (E2 / c->n_div),
                s2d = (int64_t)h->P2 * 4 * E;
  h->ws_col = enc_ws(h, Bm * std::max(col1, std::max(col2, s2d)));
  h->ws_x2 = enc_ws(h, Bm * h->P2 * E2);
  h->ws_pool = enc_ws(h, Bm * E2);
  h->ws_feat = enc_ws(h, Bm * c->feature_dim);
  h->ws_wmerge = enc_ws(h, (int64_t)E2 * E * 4);
  for (EncBlock& b : h->blocks) {
    b.wp_packed = enc_ws(h, (int64_t)b.cp * b.cp * 9); b.wp_direct = enc_ws(h, (int64_t)b.cp * b.cp * 9);
    b.wp_mfma = enc_ws(h, pconv_mfma_image_floats(b.cp));
  }
  // bf16-activation mode: instantiated for the reference's architecture (embed 96, mlp_ratio 2, n_div 4); other shapes
  // asked for in that mode run the bf16-OPERAND mode (fp32 tensors in memory)
  h->bf16_fused = c->bf16_operands == 2 && E == 96 && hidmax_rows1 == 192 && hid2 == 384 && E / c->n_div == 24;
  if (h->bf16_fused) {
    for (EncBlock& b : h->blocks) {
      b.w1_bf16 = enc_ws(h, bf16_copy_floats((int64_t)b.hidden * b.dim));
      b.w2_bf16 = enc_ws(h, bf16_copy_floats((int64_t)b.hidden * b.dim));
      b.wp_bf16 = enc_ws(h, bf16_copy_floats(pconv_bf16_image_elems(b.cp)));
    }
    h->ws_wmerge_bf16 = enc_ws(h, bf16_copy_floats((int64_t)E2 * E * 4));
  }
  for (EncBnInfo& bi : h->bns) { bi.bn->alpha = enc_ws(h, bi.bn->C); bi.bn->beta = enc_ws(h, bi.bn->C); }
  int cmax = 0;
  for (EncBnInfo& bi : h->bns) cmax = std::max(cmax, bi.bn->C);
  h->ws_partial = enc_ws(h, 2L * CS_MAX_BLOCKS * 2 * cmax + 4);
  h->ws_cstat = enc_ws(h, Bm * std::max<int64_t>((int64_t)(h->P1 / 32 + 1) * 2 * hidmax_rows1, (int64_t)(h->P2 / 32 + 1) * 2 * std::max(hid2, E2)) + 2 * 1024);   // doubles, 16-byte aligned like every offset
  *out = h;
  return PORL_OK;
}

void porl_enc_destroy(porl_enc* h) { delete h; }

int64_t porl_enc_param_floats(const porl_enc* h) { return h ? h->n_params : -1; }
int64_t porl_enc_stat_floats(const porl_enc* h) { return h ? h->n_stats : -1; }
int64_t porl_enc_workspace_floats(const porl_enc* h) { return h ? h->n_ws : -1; }
int32_t porl_enc_tensors(const porl_enc* h) { return h ? (int32_t)h->tensors.size() : -1; }
int32_t porl_enc_norms(const porl_enc* h) { return h ? (int32_t)h->bns.size() : -1; }
int32_t porl_enc_blocks(const porl_enc* h) { return h ? (int32_t)h->blocks.size() : -1; }

int porl_enc_tensor_info(const porl_enc* h, int32_t index, int64_t* offset, int64_t* numel, char* name, int32_t name_len) {
  if (!h || index < 0 || index >= (int)h->tensors.size()) PORL_FAIL(PORL_ERR_INVALID, "tensor index out of range");
  const EncTensor& t = h->tensors[index];
  if (offset) *offset = t.off;
  if (numel) *numel = t.numel;
  if (name && name_len > 0) { strncpy(name, t.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
  return PORL_OK;
}

int porl_enc_norm_info(const porl_enc* h, int32_t index, int64_t* mean_offset, int64_t* var_offset, int32_t* channels,
                       char* name, int32_t name_len) {
  if (!h || index < 0 || index >= (int)h->bns.size()) PORL_FAIL(PORL_ERR_INVALID, "norm index out of range");
  const EncBnInfo& b = h->bns[index];
  if (mean_offset) *mean_offset = b.bn->mean;
  if (var_offset) *var_offset = b.bn->var;
  if (channels) *channels = b.bn->C;
  if (name && name_len > 0) { strncpy(name, b.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
  return PORL_OK;
}

int porl_enc_tap_info(const porl_enc* h, int32_t which, int64_t* offset_floats, int64_t* rows_per_sample, int32_t* cols,
                      int32_t* elem_bytes) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (which < 0 || which >= PORL_ENC_TAPS) PORL_FAIL(PORL_ERR_INVALID, "tap index out of range (0..%d)", PORL_ENC_TAPS - 1);
  if (!offset_floats || !rows_per_sample || !cols || !elem_bytes) PORL_FAIL(PORL_ERR_INVALID, "null output pointer");
  const int act_bytes = enc_fused16(h) ? 2 : 4;
  switch (which) {
    case PORL_ENC_TAP_STAGE1: *offset_floats = h->ws_x1; *rows_per_sample = h->P1; *cols = h->E; *elem_bytes = act_bytes; break;
    case PORL_ENC_TAP_STAGE2: *offset_floats = h->ws_x2; *rows_per_sample = h->P2; *cols = h->E2; *elem_bytes = act_bytes; break;
    case PORL_ENC_TAP_POOLED: *offset_floats = h->ws_pool; *rows_per_sample = 1; *cols = h->E2; *elem_bytes = 4; break;
    default: *offset_floats = h->ws_feat; *rows_per_sample = 1; *cols = h->cfg.feature_dim; *elem_bytes = 4; break;
  }
  return PORL_OK;
}

int porl_enc_bind(porl_enc* h, float* params, float* bn_stats, float* workspace) {
  if (!h || !params || !bn_stats || !workspace) PORL_FAIL(PORL_ERR_INVALID, "null buffer");
  if (!aligned16(params) || !aligned16(bn_stats) || !aligned16(workspace))
    PORL_FAIL(PORL_ERR_INVALID, "buffers must be 16-byte aligned");
  h->params = params; h->stats = bn_stats; h->W = workspace;
  h->device = device_of(workspace);
  h->bound = true;
  h->packed_valid = false;
  return PORL_OK;
}

int porl_enc_weights_changed(porl_enc* h) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  h->packed_valid = false;
  return PORL_OK;
}

}  // extern "C"

namespace {
// conv weights in the k order of the patch matrices: re-made only after the weights may have changed (bind, or
// porl_enc_weights_changed from the module's load_state_dict / .to()), not on every forward of a frozen backbone
int enc_pack_weights(porl_enc* h, hipStream_t s) {
  float* W = h->W; const float* P = h->params;
  const int nm = h->E2 * h->E * 4;
  auto pack_bf16 = [&](const float* src, int64_t dst, long n) {
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(cdiv((int)n, 256)), dim3(256), 0, s, src, reinterpret_cast<__bf16*>(W + dst), n);
  };
  for (const EncBlock& b : h->blocks) {
    const dim3 grid(cdiv(b.cp * b.cp * 9, 256));
    hipLaunchKernelGGL(permute_oihw_ohwi_kernel, grid, dim3(256), 0, s, P + b.wp, W + b.wp_packed, b.cp, b.cp, 9);
    hipLaunchKernelGGL(pack_pconv_kernel, grid, dim3(256), 0, s, P + b.wp, W + b.wp_direct, b.cp);
    hipLaunchKernelGGL(pack_pconv_mfma_kernel, dim3(cdiv(pconv_mfma_image_floats(b.cp), 256)), dim3(256), 0, s, P + b.wp,
                       W + b.wp_mfma, b.cp, pconv_mfma_passes(b.cp));
  }
  hipLaunchKernelGGL(permute_oihw_ohwi_kernel, dim3(cdiv(nm, 256)), dim3(256), 0, s, P + h->w_merge, W + h->ws_wmerge, h->E2, h->E, 4);
  PORL_HIP(hipGetLastError());
  if (h->bf16_fused) {
    for (const EncBlock& b : h->blocks) {
      pack_bf16(P + b.w1, b.w1_bf16, (long)b.hidden * b.dim);
      pack_bf16(P + b.w2, b.w2_bf16, (long)b.hidden * b.dim);
      hipLaunchKernelGGL(pack_pconv_bf16_kernel, dim3(cdiv(pconv_bf16_image_elems(b.cp), 256)), dim3(256), 0, s, P + b.wp,
                         reinterpret_cast<__bf16*>(W + b.wp_bf16), b.cp, pconv_bf16_cpn(b.cp), pconv_bf16_cpp(b.cp) + 8);
    }
    pack_bf16(W + h->ws_wmerge, h->ws_wmerge_bf16, nm);
  }
  PORL_HIP(hipGetLastError());
  h->packed_valid = true;
  return 0;
}

// PatchEmbed 4x4s4 + its BatchNorm -> x1 (bf16 when fused16, which implies the sparse branch); clamps a caller's own `state`
int enc_patch_embed(porl_enc* h, const RowSrc& src, float* state, int64_t state_rs, int32_t batch, int32_t training,
                    bool fused16, hipStream_t s) {
  const porl_enc_cfg& c = h->cfg;
  float* W = h->W; float* x1 = W + h->ws_x1; const float* w = h->params + h->w_patch;
  const int E = h->E; const long rows1 = (long)batch * h->P1;
  if (!enc_sparse_patch(h)) {
    // rasterise (+ the in-place clamp on a caller's own tensor), then the dense 4x4 convolution; store rows go through
    // the rasteriser alone, which only reads
    if (state) PORL_TRY(porl_state2costmap(state, state_rs, batch, c.n_ang, c.n_dist, W + h->ws_img, s));
    else PORL_TRY(costmap_rasterise(src, batch, c.n_ang, c.n_dist, W + h->ws_img, s));
    {
      ProfScope ps("patch_embed_kernel", s, 2.0 * rows1 * E * 48, 4.0 * (3.0 * batch * c.n_ang * c.n_dist + rows1 * E));
      const size_t lds = (size_t)(12 * c.n_dist + PE_K * E) * sizeof(float);
      hipLaunchKernelGGL(patch_embed_kernel, dim3(h->Hp, batch), dim3(256), lds, s, W + h->ws_img, w, x1, c.n_ang, c.n_dist, E);
      PORL_HIP(hipGetLastError());
    }
    return enc_batchnorm(h, h->bn_patch, x1, rows1, 0, training, s);
  }
  // straight from the lidar state: only the ~6 % non-empty patches are convolved (statistics first, then every
  // position is written once, already normalised); no costmap image at all
  const CostmapGeom gm = costmap_geom(c.n_ang, c.n_dist); const int nblk = std::min(batch, 1024);
  const EncBn& bn = h->bn_patch; double* partial = reinterpret_cast<double*>(W + h->ws_partial);
  if (training) {
    const size_t lds_stats = (size_t)PE_K * E * sizeof(float) + (size_t)h->P1 * (sizeof(unsigned long long) + sizeof(int));
    ProfScope ps("patch_stats_kernel", s, 0.0, 4.0 * batch * (c.n_ang + 2));
    PORL_TRY(dyn_lds_once<&patch_stats_kernel>((int)lds_stats));
    hipLaunchKernelGGL(patch_stats_kernel, dim3(nblk), dim3(256), lds_stats, s, src, batch, gm, w, E, partial);
    PORL_HIP(hipGetLastError());
  }
  PORL_TRY(enc_bn_finish(h, bn, partial, nblk, rows1, training, s));
  {
    ProfScope ps("patch_bn_kernel", s, 0.0, 4.0 * rows1 * E);
    // patch rows per block: as many as keep >= 4 blocks per CU in the grid, at most 16 (the weight is parked once per
    // block; measured at B = 512, bf16: 84x84 828 -> 888 updates/s, 360x256 123.1 -> 127.8, gpurun_out/r03/prow)
    int rpb = h->tune.enc_patch_rows > 0 ? h->tune.enc_patch_rows : (int)std::max<long>(1, std::min<long>(16, (long)h->Hp * batch / (4L * NUM_CU)));
    rpb = std::min(rpb, h->Hp);
    const dim3 grid(cdiv(h->Hp, rpb), batch);
    const size_t lds = (size_t)PE_K * E * sizeof(float) + (size_t)(c.n_dist / 4) * sizeof(unsigned long long);
    if (fused16)
      hipLaunchKernelGGL(patch_bn_kernel<true>, grid, dim3(256), lds, s, src, gm, w, E, W + bn.alpha, W + bn.beta, x1, rpb);
    else
      hipLaunchKernelGGL(patch_bn_kernel<false>, grid, dim3(256), lds, s, src, gm, w, E, W + bn.alpha, W + bn.beta, x1, rpb);
    PORL_HIP(hipGetLastError());
  }
  return state ? clamp_state(state, state_rs, c.n_ang, batch, s) : 0;
}

// blocks [first, first + count) in place on x (rows, dim): fp32, or bf16 activations when fused16
int enc_stage(porl_enc* h, int first, int count, float* x, long rows, int Hh, int Ww, const float* drop_scale, int32_t batch,
              int32_t training, bool fused16, hipStream_t s) {
  for (int i = first; i < first + count; ++i) {
    const float* scale = drop_scale ? drop_scale + (long)i * batch : nullptr;
    if (fused16) PORL_TRY(enc_block_bf16(h, h->blocks[i], reinterpret_cast<__bf16*>(x), rows, Hh, Ww, scale, training, s));
    else PORL_TRY(enc_block(h, h->blocks[i], x, rows, Hh, Ww, scale, training, s));
  }
  return 0;
}

// PatchMerging 2x2s2, x1 -> x2, in its three forms; `cstat` (training) receives the column statistics of x2
int enc_merge_bf16(porl_enc* h, long rows2, float* cstat, hipStream_t s) {
  float* W = h->W; EncMergeArgs a{};
  a.x1 = reinterpret_cast<const __bf16*>(W + h->ws_x1); a.w = reinterpret_cast<const __bf16*>(W + h->ws_wmerge_bf16);
  a.out = reinterpret_cast<__bf16*>(W + h->ws_x2); a.cstat = cstat;
  a.Hp = h->Hp; a.Wp = h->Wp; a.H2 = h->H2; a.W2 = h->W2; a.rows2 = rows2;
  constexpr int MLDS = 2 * (64 * (4 * 96 + 8) + 192 * (96 + 8));
  PORL_TRY(dyn_lds_once<&enc_merge_bf16_kernel<96>>(MLDS));
  ProfScope ps("enc_merge_bf16_kernel", s, 2.0 * rows2 * 4.0 * h->E * h->E2, 2.0 * rows2 * (4.0 * h->E + h->E2));
  hipLaunchKernelGGL(enc_merge_bf16_kernel<96>, dim3((unsigned)((rows2 + 63) / 64)), dim3(256), MLDS, s, a);
  PORL_HIP(hipGetLastError());
  return 0;
}

// the GEMM gathers each output position's patch itself — two runs of 2E contiguous floats, one image row apart —
// through the grouped-row addressing of GemmProb (no space_to_depth copy).  Chunked per problem like enc_gemm_rows;
// chunks start on image-row boundaries so the group arithmetic stays local.
int enc_merge_gather(porl_enc* h, long rows2, float* cstat, hipStream_t s) {
  const float* x1 = h->W + h->ws_x1; float* x2 = h->W + h->ws_x2;
  const int E = h->E, E2 = h->E2, W2 = h->W2;
  const long reach = ((1L << 31) - (1L << 22)) / (4L * 4 * E);          // rows per problem: A spans ~2x (M x 2E)
  const long chunk = std::max<long>(W2, (reach / (32L * W2)) * (32L * W2));   // multiple of 32 rows and of W2
  long done = 0;
  while (done < rows2) {
    GemmGroup g{};
    while (done < rows2 && g.nprob < MAX_GROUP) {
      const long m = std::min(chunk, rows2 - done);
      // output row r (global) = (image row pair q = r / W2, ox = r % W2): its patch starts at float (r + q * W2) * 2E
      const float* Abase = x1 + (done + (done / W2) * W2) * 2L * E;
      GemmProb p = make_prob(GEMM_NT, Abase, 2 * E, h->W + h->ws_wmerge, 4 * E, x2 + done * E2, E2, (int)m, E2, 4 * E);
      p.a_grp = W2; p.a_grp_jump = W2 * 2 * E; p.a_seg_tiles = 2 * E / GEMM_BK; p.a_seg_jump = h->Wp * E - 2 * E;
      if (cstat) p.cstat = cstat + (done / 32) * 2 * E2;
      g.p[g.nprob++] = p;
      done += m;
    }
    g.single_buffer = (h->tune.enc_gemm_sb & 2) ? 1 : 0;
    PORL_TRY(launch_group(g, (h->tune.enc_gemm_sb & 2) ? TILE_64x64 : TILE_128x64, h->tune, s));
  }
  return 0;
}

int enc_merge_s2d(porl_enc* h, long rows1, long rows2, const EncEpi& em, hipStream_t s) {
  float* W = h->W; const int E = h->E, E2 = h->E2;
  {
    ProfScope ps("space_to_depth_kernel", s, 0.0, 8.0 * rows1 * E);
    hipLaunchKernelGGL(space_to_depth_kernel, dim3(sweep_blocks(rows2 * 4 * (E / 4))), dim3(256), 0, s, W + h->ws_x1,
                       W + h->ws_col, rows2, h->Hp, h->Wp, E);
    PORL_HIP(hipGetLastError());
  }
  return enc_gemm_rows(h, s, W + h->ws_col, 4 * E, rows2, W + h->ws_wmerge, E2, 4 * E, W + h->ws_x2, E2, nullptr, ACT_NONE, em);
}

// the merge and its BatchNorm (no ReLU), applied to x2 in place
int enc_merge(porl_enc* h, long rows1, long rows2, int32_t training, bool fused16, hipStream_t s) {
  float* W = h->W; const int E = h->E, E2 = h->E2;
  EncEpi em; em.bf16 = h->cfg.bf16_operands != 0;
  if (training) em.cstat = W + h->ws_cstat;
  if (fused16) PORL_TRY(enc_merge_bf16(h, rows2, em.cstat, s));
  else if ((2 * E) % GEMM_BK == 0 && !h->tune.enc_s2d && h->Hp % 2 == 0 && h->Wp % 2 == 0 && !em.bf16)
    PORL_TRY(enc_merge_gather(h, rows2, em.cstat, s));
  else PORL_TRY(enc_merge_s2d(h, rows1, rows2, em, s));
  PORL_TRY(enc_batchnorm(h, h->bn_merge, W + h->ws_x2, rows2, 0, training, s, em.cstat, !fused16));
  if (!fused16) return 0;
  const long n8 = rows2 * (E2 / 8);
  ProfScope ps("bn_apply_bf16_kernel", s, 0.0, 4.0 * rows2 * E2);
  hipLaunchKernelGGL(bn_apply_bf16_kernel, dim3(sweep_blocks(n8)), dim3(256), 0, s, reinterpret_cast<__bf16*>(W + h->ws_x2), n8,
                     E2 / 8, W + h->bn_merge.alpha, W + h->bn_merge.beta);
  PORL_HIP(hipGetLastError());
  return 0;
}

// global average pool of x2 -> the pooled vector (fp32 in both modes)
int enc_pool(porl_enc* h, int32_t batch, bool fused16, hipStream_t s) {
  float* x2 = h->W + h->ws_x2; float* pool = h->W + h->ws_pool;
  const long rows2 = (long)batch * h->P2;
  ProfScope ps(fused16 ? "gap_bf16_kernel" : "gap_kernel", s, 0.0, (fused16 ? 2.0 : 4.0) * rows2 * h->E2);
  if (fused16)
    hipLaunchKernelGGL(gap_bf16_kernel, dim3(batch), dim3(256), 0, s, reinterpret_cast<const __bf16*>(x2), pool, h->P2, h->E2);
  else
    hipLaunchKernelGGL(gap_kernel, dim3(cdiv(h->E2, 64), batch), dim3(256), 0, s, x2, pool, h->P2, h->E2);
  PORL_HIP(hipGetLastError());
  return 0;
}

// 1x1 (2E -> feature_dim) + ReLU, then the Linear head into the caller's `features`
int enc_head(porl_enc* h, int32_t batch, float* features, int64_t feat_rs, hipStream_t s) {
  const porl_enc_cfg& c = h->cfg; float* W = h->W;
  PORL_TRY(enc_gemm_rows(h, s, W + h->ws_pool, h->E2, batch, h->params + h->w_pre, c.feature_dim, h->E2, W + h->ws_feat,
                         c.feature_dim, nullptr, ACT_RELU));
  return enc_gemm_rows(h, s, W + h->ws_feat, c.feature_dim, batch, h->params + h->w_head, c.num_classes, c.feature_dim,
                       features, (int)feat_rs, h->params + h->b_head, ACT_NONE);
}

// The forward on a row source.  `state` is the caller's own dense tensor (porl_enc_forward: entries > 8 are zeroed in it
// afterwards, the reference's side effect) or null (porl_enc_forward_rows: the source is only read).
int enc_forward_src(porl_enc* h, const RowSrc& src, float* state, int64_t state_rs, int32_t batch, int32_t training,
                    const float* drop_scale, float* features, int64_t feat_rs, void* stream) {
  DevGuard _dg(h->device);
  hipStream_t s = (hipStream_t)stream; const porl_enc_cfg& c = h->cfg;
  const long rows1 = (long)batch * h->P1, rows2 = (long)batch * h->P2;
  const bool fused16 = enc_fused16(h);
  if (!h->packed_valid) PORL_TRY(enc_pack_weights(h, s));
  PORL_TRY(enc_patch_embed(h, src, state, state_rs, batch, training, fused16, s));
  PORL_TRY(enc_stage(h, 0, c.depth0, h->W + h->ws_x1, rows1, h->Hp, h->Wp, drop_scale, batch, training, fused16, s));
  PORL_TRY(enc_merge(h, rows1, rows2, training, fused16, s));
  PORL_TRY(enc_stage(h, c.depth0, c.depth1, h->W + h->ws_x2, rows2, h->H2, h->W2, drop_scale, batch, training, fused16, s));
  PORL_TRY(enc_pool(h, batch, fused16, s));
  return enc_head(h, batch, features, feat_rs, s);
}
}  // namespace

extern "C" {

int porl_enc_forward(porl_enc* h, float* state, int64_t state_rs, int32_t batch, int32_t training, const float* drop_scale,
                     float* features, int64_t feat_rs, void* stream) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_enc_bind() has not been called");
  if (!state || !features || batch < 1 || batch > h->cfg.max_batch)
    PORL_FAIL(PORL_ERR_INVALID, "need 1 <= batch <= max_batch (%d)", h->cfg.max_batch);
  if (feat_rs < h->cfg.num_classes || feat_rs > (1 << 20)) PORL_FAIL(PORL_ERR_INVALID, "bad feature row stride");
  return enc_forward_src(h, RowSrc{state, (long)state_rs, nullptr, 0}, state, state_rs, batch, training, drop_scale, features,
                         feat_rs, stream);
}

int porl_enc_forward_rows(porl_enc* h, const float* rows, int64_t row_stride, int64_t n_rows, const int64_t* idx,
                          int32_t col_offset, int32_t batch, int32_t training, const float* drop_scale, float* features,
                          int64_t feat_rs, void* stream) {
  if (!h) PORL_FAIL(PORL_ERR_INVALID, "null engine");
  if (!h->bound) PORL_FAIL(PORL_ERR_UNBOUND, "porl_enc_bind() has not been called");
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (!idx) PORL_FAIL(PORL_ERR_INVALID, "null idx");
  if (!features) PORL_FAIL(PORL_ERR_INVALID, "null features");
  if (batch < 1 || batch > h->cfg.max_batch) PORL_FAIL(PORL_ERR_INVALID, "batch %d outside [1,%d]", batch, h->cfg.max_batch);
  if (n_rows < 1) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld must be at least 1", (long long)n_rows);
  if (col_offset < 0 || (int64_t)col_offset + h->cfg.n_ang + 2 > row_stride)
    PORL_FAIL(PORL_ERR_INVALID, "col_offset %d: a state of %d floats does not fit a row of stride %lld there", col_offset,
              h->cfg.n_ang + 2, (long long)row_stride);
  if (feat_rs < h->cfg.num_classes || feat_rs > (1 << 20))
    PORL_FAIL(PORL_ERR_INVALID, "feat_rs %lld outside [num_classes = %d, 2^20]", (long long)feat_rs, h->cfg.num_classes);
  return enc_forward_src(h, RowSrc{rows, (long)row_stride, idx, col_offset}, nullptr, 0, batch, training, drop_scale, features,
                         feat_rs, stream);
}

}  // extern "C"
