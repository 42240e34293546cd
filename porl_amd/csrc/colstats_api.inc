// Column statistics and the affine column pass of a resident store (porl_colstats_workspace, porl_col_stats,
// porl_affine_cols): the host side of csrc/colstats.hpp.  Included by porl_api.hip.  Every argument is checked before the
// first device call; nothing here allocates or synchronises — the caller reads the 4 * n_cols doubles of `out` back.

namespace {

constexpr int64_t CS_MAX_ROWS = int64_t(1) << 36;
constexpr int64_t CS_MAX_STRIDE = int64_t(1) << 20;      // floats; keeps row * stride inside an int64 at CS_MAX_ROWS
constexpr int32_t CS_MAX_COLS = 4096;

// partials of level 0 and of every further level that is stored (the last merge writes `out`)
int64_t cs_partials(int64_t n_rows) {
  int64_t cnt = (n_rows + CS_TILE - 1) / CS_TILE, total = cnt;
  while (cnt > CS_SWEEP) { cnt = (cnt + CS_SWEEP - 1) / CS_SWEEP; total += cnt; }
  return total;
}

int cs_check_view(const char* what, const void* p, const char* stride_name, int64_t stride, int64_t width, int64_t n_rows) {
  if (!p) PORL_FAIL(PORL_ERR_INVALID, "null %s", what);
  if (reinterpret_cast<uintptr_t>(p) % 4 != 0) PORL_FAIL(PORL_ERR_INVALID, "%s must be 4-byte aligned", what);
  if (n_rows < 1 || n_rows > CS_MAX_ROWS) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^36]", (long long)n_rows);
  if (stride < width || stride > CS_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "%s %lld outside [%lld columns read or written, 2^20]", stride_name, (long long)stride, (long long)width);
  return PORL_OK;
}

bool cs_vec16(const float* first, int64_t stride_floats, int32_t n_cols) {
  return reinterpret_cast<uintptr_t>(first) % 16 == 0 && stride_floats % 4 == 0 && n_cols % 4 == 0;
}

}  // namespace

extern "C" {

int64_t porl_colstats_workspace(int64_t n_rows, int32_t n_cols, int32_t* rows_per_block, int32_t* partials_per_sweep) {
  if (rows_per_block) *rows_per_block = CS_TILE;
  if (partials_per_sweep) *partials_per_sweep = CS_SWEEP;
  if (n_rows < 1 || n_rows > CS_MAX_ROWS) { g_err = "n_rows outside [1, 2^36]"; return -1; }
  if (n_cols < 1 || n_cols > CS_MAX_COLS) { g_err = "n_cols outside [1, 4096]"; return -1; }
  return CS_STATS * (int64_t)n_cols * cs_partials(n_rows);
}

int porl_col_stats(const float* rows, int64_t stride_floats, int64_t n_rows, int32_t col0, int32_t n_cols, double* workspace,
                   double* out, void* stream) {
  if (n_cols < 1 || n_cols > CS_MAX_COLS) PORL_FAIL(PORL_ERR_INVALID, "n_cols %d outside [1, 4096]", n_cols);
  if (col0 < 0 || col0 > CS_MAX_STRIDE - n_cols) PORL_FAIL(PORL_ERR_INVALID, "col0 %d outside [0, 2^20 - n_cols]", col0);
  PORL_TRY(cs_check_view("rows", rows, "stride_floats", stride_floats, (int64_t)col0 + n_cols, n_rows));
  if (!workspace) PORL_FAIL(PORL_ERR_INVALID, "null workspace");
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0 || reinterpret_cast<uintptr_t>(out) % 8 != 0)
    PORL_FAIL(PORL_ERR_INVALID, "workspace and out must be 8-byte aligned");
  const float* base = rows + col0;
  const int64_t C = n_cols;
  int64_t cnt = (n_rows + CS_TILE - 1) / CS_TILE;
  const dim3 grid((unsigned)cnt, (unsigned)((n_cols + CS_CHUNK - 1) / CS_CHUNK));
  hipStream_t s = (hipStream_t)stream;
  DevGuard _dg(device_of(out));
  if (cs_vec16(base, stride_floats, n_cols))
    hipLaunchKernelGGL(cs_tile_kernel<true>, grid, dim3(CS_THREADS), 0, s, base, (long long)stride_floats, (long long)n_rows, n_cols, workspace);
  else
    hipLaunchKernelGGL(cs_tile_kernel<false>, grid, dim3(CS_THREADS), 0, s, base, (long long)stride_floats, (long long)n_rows, n_cols, workspace);
  // level l -> level l + 1 until one partial is left; that one goes to `out`
  double* level = workspace;
  long long span = CS_TILE;
  for (;;) {
    const int64_t cnt_out = (cnt + CS_SWEEP - 1) / CS_SWEEP;
    const dim3 mgrid((unsigned)((cnt_out * C + CS_THREADS - 1) / CS_THREADS));
    if (cnt_out == 1) {
      hipLaunchKernelGGL(cs_merge_kernel<true>, mgrid, dim3(CS_THREADS), 0, s, level, out, (long long)cnt, (long long)cnt_out,
                         (long long)n_rows, span, n_cols);
      break;
    }
    double* dst = level + CS_STATS * C * cnt;
    hipLaunchKernelGGL(cs_merge_kernel<false>, mgrid, dim3(CS_THREADS), 0, s, level, dst, (long long)cnt, (long long)cnt_out,
                       (long long)n_rows, span, n_cols);
    level = dst; cnt = cnt_out; span *= CS_SWEEP;
  }
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_affine_cols(const float* rows, int64_t stride_floats, int64_t n_rows, int32_t width, const porl_col_span* spans,
                     int32_t n_spans, const float* shift, const float* div, const float* mul, int32_t n_params, float* out,
                     int64_t out_stride_floats, void* stream) {
  if (width < 1 || width > CS_MAX_STRIDE) PORL_FAIL(PORL_ERR_INVALID, "width %d outside [1, 2^20]", width);
  PORL_TRY(cs_check_view("rows", rows, "stride_floats", stride_floats, width, n_rows));
  PORL_TRY(cs_check_view("out", out, "out_stride_floats", out_stride_floats, width, n_rows));
  if (static_cast<const void*>(rows) == static_cast<const void*>(out) && stride_floats != out_stride_floats)
    PORL_FAIL(PORL_ERR_INVALID, "out_stride_floats %lld != stride_floats %lld with out == rows (in place)", (long long)out_stride_floats,
              (long long)stride_floats);
  if (!spans) PORL_FAIL(PORL_ERR_INVALID, "null spans");
  if (n_spans < 1 || n_spans > AF_MAX_SPANS) PORL_FAIL(PORL_ERR_INVALID, "n_spans %d outside [1, %d]", n_spans, AF_MAX_SPANS);
  if (!shift) PORL_FAIL(PORL_ERR_INVALID, "null shift");
  if (!div) PORL_FAIL(PORL_ERR_INVALID, "null div");
  if (n_params < 1 || n_params > CS_MAX_STRIDE) PORL_FAIL(PORL_ERR_INVALID, "n_params %d outside [1, 2^20]", n_params);
  for (int i = 0; i < n_spans; ++i) {
    const porl_col_span& p = spans[i];
    if (p.n_cols < 1 || p.col0 < 0 || p.col0 > width - p.n_cols)
      PORL_FAIL(PORL_ERR_INVALID, "spans[%d]: columns [%d, %d + %d) do not lie inside width %d", i, p.col0, p.col0, p.n_cols, width);
    if (p.param0 < 0 || p.param0 > n_params - p.n_cols)
      PORL_FAIL(PORL_ERR_INVALID, "spans[%d]: parameters [%d, %d + %d) do not lie inside n_params %d", i, p.param0, p.param0, p.n_cols,
                n_params);
    if (p.flags & ~1) PORL_FAIL(PORL_ERR_INVALID, "spans[%d]: flags %d has bits other than bit 0 (multiply)", i, p.flags);
    if ((p.flags & 1) && !mul) PORL_FAIL(PORL_ERR_INVALID, "null mul with the multiply flag of spans[%d] set", i);
    for (int j = 0; j < i; ++j)
      if (p.col0 < spans[j].col0 + spans[j].n_cols && spans[j].col0 < p.col0 + p.n_cols)
        PORL_FAIL(PORL_ERR_INVALID, "spans[%d] and spans[%d] overlap", j, i);
  }
  AfArgs a{};
  a.rows = rows; a.stride = (long long)stride_floats; a.out = out; a.out_stride = (long long)out_stride_floats;
  a.n_rows = (long long)n_rows; a.shift = shift; a.div = div; a.mul = mul; a.n_spans = n_spans;
  int64_t units = 0;
  for (int i = 0; i < n_spans; ++i) {
    const porl_col_span& p = spans[i];
    const bool vec = cs_vec16(rows + p.col0, stride_floats, p.n_cols) && cs_vec16(out + p.col0, out_stride_floats, p.n_cols);
    a.sp[i].col0 = p.col0; a.sp[i].param0 = p.param0; a.sp[i].flags = (p.flags & 1) | (vec ? 2 : 0);
    a.sp[i].units = vec ? p.n_cols / 4 : p.n_cols; a.sp[i].unit0 = (int)units;
    units += a.sp[i].units;
  }
  a.units_per_row = (int)units;                                   // <= width <= 2^20: the spans are disjoint
  a.rows_per_block = (int)std::max<int64_t>(1, AF_BLOCK_UNITS / units);
  a.n_blocks = (long long)((n_rows + a.rows_per_block - 1) / a.rows_per_block);
  const unsigned grid = (unsigned)std::min<long long>(a.n_blocks, 8192);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(af_cols_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
