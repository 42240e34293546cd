// Driver of tests/test_normalize_host.py — the rejected-argument paths of the column-statistics and affine entry points
// (porl_colstats_workspace, porl_col_stats, porl_affine_cols) on the HOST-ONLY sanitized build of csrc/porl_api.hip
// (-fsanitize=address,undefined), beside abi_reject_holdout.cpp.  Every call below must fail validation before it
// reaches a HIP call, so the program makes no launch and runs without a GPU.  Exit code 0 = every rejection was a clean
// error return with a message that names the argument and the sanitizers stayed silent (they abort the process
// otherwise).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/porl_hip.h"

static int g_checks = 0, g_bad = 0;
// a rejection must name what it refuses: `word` has to appear in the message
#define REJECT(word, expr)                                                                     \
  do {                                                                                         \
    ++g_checks;                                                                                \
    const long _r = (long)(expr);                                                              \
    const char* _m = porl_last_error();                                                        \
    if (_r != -1) { ++g_bad; std::fprintf(stderr, "returned %ld: %s\n", _r, #expr); }          \
    else if (!_m || !_m[0]) { ++g_bad; std::fprintf(stderr, "no message: %s\n", #expr); }      \
    else if (!std::strstr(_m, word)) { ++g_bad; std::fprintf(stderr, "message '%s' does not name '%s': %s\n", _m, word, #expr); } \
  } while (0)
#define EXPECT(cond)                                                                           \
  do {                                                                                         \
    ++g_checks;                                                                                \
    if (!(cond)) { ++g_bad; std::fprintf(stderr, "failed: %s\n", #cond); }                     \
  } while (0)

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  static_assert(sizeof(porl_col_span) == 16, "porl_col_span is four int32");
  const int64_t BIG = (int64_t(1) << 36) + 1;
  const int64_t WIDE = (int64_t(1) << 20) + 4;
  alignas(16) float f[256] = {0};
  alignas(16) float o[256] = {0};
  alignas(16) float prm[16] = {0};
  double w[256] = {0}, d[64] = {0};
  // ---- porl_colstats_workspace (pure host) ----------------------------------------------------------------------------
  int32_t T = 0, P = 0;
  const int64_t K = porl_colstats_workspace(1, 1, &T, &P);       // doubles per column of a stored partial
  EXPECT(K >= 4 && T >= 64 && P >= 2);
  EXPECT(porl_colstats_workspace((int64_t)T, 3, nullptr, nullptr) == 3 * K);
  EXPECT(porl_colstats_workspace((int64_t)T + 1, 3, nullptr, nullptr) == 6 * K);
  EXPECT(porl_colstats_workspace((int64_t)T * P + 1, 3, nullptr, nullptr) == 3 * K * ((int64_t)P + 3));
  EXPECT(porl_colstats_workspace(int64_t(1) << 36, 4096, nullptr, nullptr) > 0);
  REJECT("n_rows", porl_colstats_workspace(0, 3, nullptr, nullptr));
  REJECT("n_rows", porl_colstats_workspace(-3, 3, &T, &P));
  REJECT("n_rows", porl_colstats_workspace(BIG, 3, nullptr, nullptr));
  REJECT("n_cols", porl_colstats_workspace(8, 0, nullptr, nullptr));
  REJECT("n_cols", porl_colstats_workspace(8, 4097, nullptr, nullptr));
  REJECT("n_cols", porl_colstats_workspace(8, INT32_MIN, nullptr, nullptr));
  // ---- porl_col_stats: 8 rows of 12 floats, columns [0, 4) --------------------------------------------------------------
  REJECT("null rows", porl_col_stats(nullptr, 12, 8, 0, 4, w, d, nullptr));
  REJECT("null workspace", porl_col_stats(f, 12, 8, 0, 4, nullptr, d, nullptr));
  REJECT("null out", porl_col_stats(f, 12, 8, 0, 4, w, nullptr, nullptr));
  REJECT("n_rows", porl_col_stats(f, 12, 0, 0, 4, w, d, nullptr));
  REJECT("n_rows", porl_col_stats(f, 12, -1, 0, 4, w, d, nullptr));
  REJECT("n_rows", porl_col_stats(f, 12, BIG, 0, 4, w, d, nullptr));
  REJECT("n_cols", porl_col_stats(f, 12, 8, 0, 0, w, d, nullptr));
  REJECT("n_cols", porl_col_stats(f, 12, 8, 0, 4097, w, d, nullptr));
  REJECT("n_cols", porl_col_stats(f, 12, 8, 0, INT32_MIN, w, d, nullptr));
  REJECT("col0", porl_col_stats(f, 12, 8, -1, 4, w, d, nullptr));
  REJECT("col0", porl_col_stats(f, 12, 8, INT32_MAX, 4, w, d, nullptr));
  REJECT("stride_floats", porl_col_stats(f, 3, 8, 0, 4, w, d, nullptr));
  REJECT("stride_floats", porl_col_stats(f, 12, 8, 9, 4, w, d, nullptr));
  REJECT("stride_floats", porl_col_stats(f, 0, 8, 0, 4, w, d, nullptr));
  REJECT("stride_floats", porl_col_stats(f, INT64_MIN, 8, 0, 4, w, d, nullptr));
  REJECT("stride_floats", porl_col_stats(f, WIDE, 8, 0, 4, w, d, nullptr));
  REJECT("aligned", porl_col_stats(reinterpret_cast<const float*>(reinterpret_cast<const char*>(f) + 2), 12, 8, 0, 4, w, d, nullptr));
  REJECT("aligned", porl_col_stats(f, 12, 8, 0, 4, w, reinterpret_cast<double*>(reinterpret_cast<char*>(d) + 4), nullptr));
  // ---- porl_affine_cols: 8 rows of 12 floats, [s | r | s' | d | a] with S = 4 ------------------------------------------------
  const porl_col_span ok[3] = {{0, 4, 0, 0}, {5, 4, 0, 0}, {4, 1, 4, 1}};
  REJECT("null rows", porl_affine_cols(nullptr, 12, 8, 12, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("null out", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 5, nullptr, 12, nullptr));
  REJECT("null spans", porl_affine_cols(f, 12, 8, 12, nullptr, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("null shift", porl_affine_cols(f, 12, 8, 12, ok, 3, nullptr, prm, prm, 5, o, 12, nullptr));
  REJECT("null div", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, nullptr, prm, 5, o, 12, nullptr));
  REJECT("null mul", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, nullptr, 5, o, 12, nullptr));
  REJECT("n_rows", porl_affine_cols(f, 12, 0, 12, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("n_rows", porl_affine_cols(f, 12, BIG, 12, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("width", porl_affine_cols(f, 12, 8, 0, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("width", porl_affine_cols(f, 12, 8, INT32_MIN, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("width", porl_affine_cols(f, 12, 8, (int32_t)WIDE, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("stride_floats", porl_affine_cols(f, 11, 8, 12, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("stride_floats", porl_affine_cols(f, INT64_MAX, 8, 12, ok, 3, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("out_stride_floats", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 5, o, 11, nullptr));
  REJECT("out_stride_floats", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 5, o, INT64_MIN, nullptr));
  REJECT("out_stride_floats", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 5, f, 16, nullptr));
  REJECT("n_spans", porl_affine_cols(f, 12, 8, 12, ok, 0, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("n_spans", porl_affine_cols(f, 12, 8, 12, ok, 9, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("n_spans", porl_affine_cols(f, 12, 8, 12, ok, -1, prm, prm, prm, 5, o, 12, nullptr));
  REJECT("n_params", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 0, o, 12, nullptr));
  REJECT("n_params", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 4, o, 12, nullptr));
  REJECT("aligned", porl_affine_cols(f, 12, 8, 12, ok, 3, prm, prm, prm, 5, reinterpret_cast<float*>(reinterpret_cast<char*>(o) + 2), 12, nullptr));
  {
    const porl_col_span overlap[2] = {{0, 4, 0, 0}, {3, 4, 0, 0}};
    REJECT("overlap", porl_affine_cols(f, 12, 8, 12, overlap, 2, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span same[2] = {{5, 1, 0, 0}, {5, 1, 0, 0}};
    REJECT("overlap", porl_affine_cols(f, 12, 8, 12, same, 2, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span past[1] = {{9, 4, 0, 0}};
    REJECT("width", porl_affine_cols(f, 12, 8, 12, past, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span huge[1] = {{1, INT32_MAX, 0, 0}};
    REJECT("width", porl_affine_cols(f, 12, 8, 12, huge, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span neg[1] = {{INT32_MIN, 4, 0, 0}};
    REJECT("width", porl_affine_cols(f, 12, 8, 12, neg, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span empty[1] = {{0, 0, 0, 0}};
    REJECT("width", porl_affine_cols(f, 12, 8, 12, empty, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span pp[1] = {{0, 4, 2, 0}};
    REJECT("n_params", porl_affine_cols(f, 12, 8, 12, pp, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span pn[1] = {{0, 4, INT32_MIN, 0}};
    REJECT("n_params", porl_affine_cols(f, 12, 8, 12, pn, 1, prm, prm, prm, 5, o, 12, nullptr));
    const porl_col_span fl[1] = {{0, 4, 0, 6}};
    REJECT("flags", porl_affine_cols(f, 12, 8, 12, fl, 1, prm, prm, prm, 5, o, 12, nullptr));
  }
  std::printf("abi_reject_normalize: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
