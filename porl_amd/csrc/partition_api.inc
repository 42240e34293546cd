// Stable row partition of a resident store (porl_partition_*): the host side of csrc/partition.hpp.  Included by
// porl_api.hip.  Every argument is checked before the first device call; nothing here allocates or synchronises — the
// caller reads K back from the workspace once both launches of porl_partition_rows are queued.

namespace {

constexpr int64_t PT_MAX_ROWS = int64_t(1) << 36;
constexpr int64_t PT_MAX_STRIDE = int64_t(1) << 22;      // bytes; keeps row * stride inside an int64 at PT_MAX_ROWS

int64_t pt_tiles(int64_t n_rows) { return (n_rows + PT_TILE - 1) / PT_TILE; }

// the checks the mask pass and the partition share
int pt_check_rows(const void* rows, int64_t stride_bytes, int64_t n_rows, int64_t row_bytes) {
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (n_rows < 1 || n_rows > PT_MAX_ROWS) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^36]", (long long)n_rows);
  if (row_bytes < 4 || row_bytes % 4 != 0 || row_bytes > PT_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "row_bytes %lld must be a positive multiple of 4, at most 2^22", (long long)row_bytes);
  if (stride_bytes < row_bytes || stride_bytes % 4 != 0 || stride_bytes > PT_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "stride_bytes %lld must be a multiple of 4 in [row_bytes = %lld, 2^22]", (long long)stride_bytes,
              (long long)row_bytes);
  if (reinterpret_cast<uintptr_t>(rows) % 4 != 0) PORL_FAIL(PORL_ERR_INVALID, "rows must be 4-byte aligned");
  return PORL_OK;
}

int pt_check_box(const porl_partition_box* box, int64_t row_bytes) {
  if (box->cx < 0 || box->cx >= row_bytes / 4) PORL_FAIL(PORL_ERR_INVALID, "cx %d outside the row's %lld words", box->cx, (long long)(row_bytes / 4));
  if (box->cy < 0 || box->cy >= row_bytes / 4) PORL_FAIL(PORL_ERR_INVALID, "cy %d outside the row's %lld words", box->cy, (long long)(row_bytes / 4));
  return PORL_OK;
}

PtPred pt_pred(const void* rows, int64_t stride_bytes, int64_t n_rows, const uint8_t* held, const porl_partition_box* box) {
  PtPred p{};
  p.mask = held; p.base = static_cast<const char*>(rows); p.stride = (long long)stride_bytes; p.n = (long long)n_rows;
  if (box) { p.cx = box->cx; p.cy = box->cy; p.x_lo = box->x_lo; p.x_hi = box->x_hi; p.y_lo = box->y_lo; p.y_hi = box->y_hi; }
  return p;
}

}  // namespace

extern "C" {

int64_t porl_partition_workspace(int64_t n_rows, int32_t* rows_per_block, int32_t* partials_per_sweep) {
  if (rows_per_block) *rows_per_block = PT_TILE;
  if (partials_per_sweep) *partials_per_sweep = EP_SWEEP;
  if (n_rows < 1 || n_rows > PT_MAX_ROWS) { g_err = "n_rows outside [1, 2^36]"; return -1; }
  return 2 + 2 * pt_tiles(n_rows);
}

int porl_partition_mask(const void* rows, int64_t stride_bytes, int64_t n_rows, int64_t row_bytes,
                        const porl_partition_box* box, uint8_t* mask, void* stream) {
  PORL_TRY(pt_check_rows(rows, stride_bytes, n_rows, row_bytes));
  if (!box) PORL_FAIL(PORL_ERR_INVALID, "null box");
  if (!mask) PORL_FAIL(PORL_ERR_INVALID, "null mask");
  PORL_TRY(pt_check_box(box, row_bytes));
  const PtPred p = pt_pred(rows, stride_bytes, n_rows, nullptr, box);
  DevGuard _dg(device_of(mask));
  hipLaunchKernelGGL(pt_mask_kernel, dim3((unsigned)((n_rows + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0,
                     (hipStream_t)stream, p, mask);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_partition_rows(const void* rows, int64_t stride_bytes, int64_t n_rows, int64_t row_bytes, const uint8_t* held,
                        const porl_partition_box* box, void* out, int64_t* index, int64_t* workspace, void* stream) {
  PORL_TRY(pt_check_rows(rows, stride_bytes, n_rows, row_bytes));
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (!workspace) PORL_FAIL(PORL_ERR_INVALID, "null workspace");
  if (held && box) PORL_FAIL(PORL_ERR_INVALID, "held and box are both given: the predicate is one or the other");
  if (!held && !box) PORL_FAIL(PORL_ERR_INVALID, "neither held nor box is given");
  if (reinterpret_cast<uintptr_t>(out) % 4 != 0) PORL_FAIL(PORL_ERR_INVALID, "out must be 4-byte aligned");
  if (box) PORL_TRY(pt_check_box(box, row_bytes));
  const int64_t nb = pt_tiles(n_rows);
  long long* info = reinterpret_cast<long long*>(workspace);
  long long *cnt = info + 2, *off = cnt + nb;
  const PtPred p = pt_pred(rows, stride_bytes, n_rows, held, box);
  const int64_t units = pt_vec16(rows, stride_bytes, out, row_bytes) ? row_bytes / 16 : row_bytes / 4;
  int lpr = 1;
  while (lpr < 64 && lpr < units) lpr <<= 1;
  hipStream_t s = (hipStream_t)stream;
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(pt_count_kernel, dim3((unsigned)nb), dim3(PT_THREADS), 0, s, p, cnt);
  hipLaunchKernelGGL(pt_scan_kernel, dim3(1), dim3(EP_SWEEP), 0, s, cnt, off, (long long)nb, info, (long long)n_rows);
  hipLaunchKernelGGL(pt_scatter_kernel, dim3((unsigned)nb), dim3(PT_THREADS), 0, s, p, off, info, static_cast<char*>(out),
                     reinterpret_cast<long long*>(index), (long long)row_bytes, lpr);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
