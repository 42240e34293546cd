// Episode tables, episode returns and hindsight-goal batches (porl_episode_*, porl_hindsight_pairs, porl_gather_pairs):
// the host side of csrc/episodes.hpp.  Included by porl_api.hip.  Every argument is checked before the first device
// call; nothing here allocates or synchronises — the caller reads K back from the workspace between count and fill.

namespace {

constexpr int64_t EP_MAX_ROWS = int64_t(1) << 40;
constexpr int64_t EP_MAX_STRIDE = int64_t(1) << 20;      // keeps row * stride inside an int64 at EP_MAX_ROWS

int64_t ep_tiles(int64_t n_rows) { return (n_rows + EP_TILE - 1) / EP_TILE; }

// the checks count and fill share
int ep_check_flags(const float* flags, int64_t stride, int64_t n_rows, int64_t cap, const void* workspace) {
  if (!flags) PORL_FAIL(PORL_ERR_INVALID, "null flags");
  if (!workspace) PORL_FAIL(PORL_ERR_INVALID, "null workspace");
  if (n_rows < 1 || n_rows > EP_MAX_ROWS) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^40]", (long long)n_rows);
  if (stride < 1 || stride > EP_MAX_STRIDE) PORL_FAIL(PORL_ERR_INVALID, "stride %lld outside [1, 2^20]", (long long)stride);
  if (cap < 0) PORL_FAIL(PORL_ERR_INVALID, "cap %lld must not be negative (0 = no cap)", (long long)cap);
  return PORL_OK;
}

struct EpWorkspace {
  long long *info, *lastdone, *carry, *cnt, *off, *lastclose;
  EpWorkspace(const int64_t* ws, int64_t nb) {
    long long* p = reinterpret_cast<long long*>(const_cast<int64_t*>(ws));
    info = p; lastdone = p + 2; carry = lastdone + nb; cnt = carry + nb; off = cnt + nb; lastclose = off + nb;
  }
};

}  // namespace

extern "C" {

int64_t porl_episode_workspace(int64_t n_rows, int32_t* rows_per_block, int32_t* partials_per_sweep) {
  if (rows_per_block) *rows_per_block = EP_TILE;
  if (partials_per_sweep) *partials_per_sweep = EP_SWEEP;
  if (n_rows < 1 || n_rows > EP_MAX_ROWS) { g_err = "n_rows outside [1, 2^40]"; return -1; }
  return 2 + 5 * ep_tiles(n_rows);
}

int porl_episode_count(const float* flags, int64_t stride, int64_t n_rows, int64_t cap, int64_t* workspace, void* stream) {
  PORL_TRY(ep_check_flags(flags, stride, n_rows, cap, workspace));
  const int64_t nb = ep_tiles(n_rows);
  const EpWorkspace w(workspace, nb);
  const EpFlags f{flags, (long long)stride, (long long)n_rows};
  hipStream_t s = (hipStream_t)stream;
  DevGuard _dg(device_of(workspace));
  if (cap > 0) {
    hipLaunchKernelGGL(ep_lastdone_kernel, dim3((unsigned)nb), dim3(EP_THREADS), 0, s, f, w.lastdone);
    hipLaunchKernelGGL(ep_scan_partials_kernel<true>, dim3(1), dim3(EP_SWEEP), 0, s, w.lastdone, w.carry, (long long)nb,
                       (const long long*)nullptr, (long long*)nullptr, (long long)n_rows);
  }
  hipLaunchKernelGGL(ep_close_kernel<false>, dim3((unsigned)nb), dim3(EP_THREADS), 0, s, f, (long long)cap, w.carry,
                     (const long long*)nullptr, w.cnt, w.lastclose, 0ll, (long long*)nullptr, (long long*)nullptr);
  hipLaunchKernelGGL(ep_scan_partials_kernel<false>, dim3(1), dim3(EP_SWEEP), 0, s, w.cnt, w.off, (long long)nb, w.lastclose,
                     w.info, (long long)n_rows);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_episode_fill(const float* flags, int64_t stride, int64_t n_rows, int64_t cap, const int64_t* workspace,
                      int64_t n_episodes, int64_t* starts, int64_t* ends, void* stream) {
  PORL_TRY(ep_check_flags(flags, stride, n_rows, cap, workspace));
  if (!starts) PORL_FAIL(PORL_ERR_INVALID, "null starts");
  if (!ends) PORL_FAIL(PORL_ERR_INVALID, "null ends");
  if (n_episodes < 1 || n_episodes > n_rows)
    PORL_FAIL(PORL_ERR_INVALID, "n_episodes %lld outside [1, n_rows]", (long long)n_episodes);
  const int64_t nb = ep_tiles(n_rows);
  const EpWorkspace w(workspace, nb);
  const EpFlags f{flags, (long long)stride, (long long)n_rows};
  DevGuard _dg(device_of(ends));
  hipLaunchKernelGGL(ep_close_kernel<true>, dim3((unsigned)nb), dim3(EP_THREADS), 0, (hipStream_t)stream, f, (long long)cap,
                     w.carry, w.off, (long long*)nullptr, (long long*)nullptr, (long long)n_episodes,
                     reinterpret_cast<long long*>(starts), reinterpret_cast<long long*>(ends));
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_episode_returns(const float* rewards, int64_t stride, int64_t n_rows, const int64_t* starts, const int64_t* ends,
                         int64_t n_episodes, double* returns, int64_t* range_ws, double* range_out, void* stream) {
  if (!rewards) PORL_FAIL(PORL_ERR_INVALID, "null rewards");
  if (!starts) PORL_FAIL(PORL_ERR_INVALID, "null starts");
  if (!ends) PORL_FAIL(PORL_ERR_INVALID, "null ends");
  if (!returns) PORL_FAIL(PORL_ERR_INVALID, "null returns");
  if (range_out && !range_ws) PORL_FAIL(PORL_ERR_INVALID, "null range_ws (range_out is given)");
  if (n_rows < 1 || n_rows > EP_MAX_ROWS) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^40]", (long long)n_rows);
  if (stride < 1 || stride > EP_MAX_STRIDE) PORL_FAIL(PORL_ERR_INVALID, "stride %lld outside [1, 2^20]", (long long)stride);
  if (n_episodes < 1 || n_episodes > n_rows)
    PORL_FAIL(PORL_ERR_INVALID, "n_episodes %lld outside [1, n_rows]", (long long)n_episodes);
  hipStream_t s = (hipStream_t)stream;
  DevGuard _dg(device_of(returns));
  const unsigned blocks = (unsigned)std::min<int64_t>((n_episodes + 3) / 4, int64_t(1) << 16);
  hipLaunchKernelGGL(ep_returns_kernel, dim3(blocks), dim3(256), 0, s, rewards, (long long)stride, (long long)n_rows,
                     reinterpret_cast<const long long*>(starts), reinterpret_cast<const long long*>(ends), (long long)n_episodes,
                     returns);
  if (range_out) {
    const unsigned rb = (unsigned)std::min<int64_t>((n_episodes + 255) / 256, EP_RANGE_BLOCKS);
    hipLaunchKernelGGL(ep_range_kernel<false>, dim3(rb), dim3(256), 0, s, returns, (long long)n_episodes,
                       reinterpret_cast<long long*>(range_ws), (double*)nullptr);
    hipLaunchKernelGGL(ep_range_kernel<true>, dim3(1), dim3(256), 0, s, (const double*)nullptr, (long long)rb,
                       reinterpret_cast<long long*>(range_ws), range_out);
  }
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_hindsight_pairs(const int64_t* starts, const int64_t* lengths, int64_t n_episodes, int32_t batch, uint64_t seed,
                         uint64_t step, const int64_t* traj, const double* u1, const double* u2, int64_t* start, int64_t* goal,
                         int64_t* traj_out, double* u1_out, double* u2_out, void* stream) {
  if (!starts) PORL_FAIL(PORL_ERR_INVALID, "null starts");
  if (!lengths) PORL_FAIL(PORL_ERR_INVALID, "null lengths");
  if (!start) PORL_FAIL(PORL_ERR_INVALID, "null start");
  if (!goal) PORL_FAIL(PORL_ERR_INVALID, "null goal");
  if (n_episodes < 1 || n_episodes > EP_MAX_ROWS)
    PORL_FAIL(PORL_ERR_INVALID, "n_episodes %lld outside [1, 2^40]", (long long)n_episodes);
  if (batch < 1) PORL_FAIL(PORL_ERR_INVALID, "batch %d must be positive", batch);
  if (traj || u1 || u2) {                                   // given draws come as all three
    if (!traj) PORL_FAIL(PORL_ERR_INVALID, "null traj (u1 or u2 is given)");
    if (!u1) PORL_FAIL(PORL_ERR_INVALID, "null u1 (traj is given)");
    if (!u2) PORL_FAIL(PORL_ERR_INVALID, "null u2 (traj is given)");
  }
  EpPairArgs a;
  a.starts = reinterpret_cast<const long long*>(starts); a.lengths = reinterpret_cast<const long long*>(lengths);
  a.E = n_episodes; a.batch = batch; a.key = ep_sm64(seed ^ ep_sm64(step));
  a.traj_in = reinterpret_cast<const long long*>(traj); a.u1_in = u1; a.u2_in = u2;
  a.start = reinterpret_cast<long long*>(start); a.goal = reinterpret_cast<long long*>(goal);
  a.traj_out = reinterpret_cast<long long*>(traj_out); a.u1_out = u1_out; a.u2_out = u2_out;
  DevGuard _dg(device_of(start));
  hipLaunchKernelGGL(ep_pairs_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_gather_pairs(const float* rows, int64_t row_stride, int64_t n_rows, const int64_t* start, const int64_t* goal,
                      int32_t batch, int32_t obs_dim, int32_t act_dim, float* out, int64_t out_stride, void* stream) {
  if (!rows) PORL_FAIL(PORL_ERR_INVALID, "null rows");
  if (!start) PORL_FAIL(PORL_ERR_INVALID, "null start");
  if (!goal) PORL_FAIL(PORL_ERR_INVALID, "null goal");
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (n_rows < 1 || n_rows > EP_MAX_ROWS) PORL_FAIL(PORL_ERR_INVALID, "n_rows %lld outside [1, 2^40]", (long long)n_rows);
  if (batch < 1) PORL_FAIL(PORL_ERR_INVALID, "batch %d must be positive", batch);
  if (obs_dim < 1 || obs_dim > (1 << 24)) PORL_FAIL(PORL_ERR_INVALID, "obs_dim %d outside [1, 2^24]", obs_dim);
  if (act_dim < 0 || act_dim > (1 << 24)) PORL_FAIL(PORL_ERR_INVALID, "act_dim %d outside [0, 2^24]", act_dim);
  const int64_t width = 2 * (int64_t)obs_dim + 2 + act_dim;
  if (row_stride < width || row_stride > EP_MAX_STRIDE * 64)
    PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld: a row is 2*obs_dim + 2 + act_dim = %lld floats", (long long)row_stride,
              (long long)width);
  if (out_stride < width || out_stride > EP_MAX_STRIDE * 64)
    PORL_FAIL(PORL_ERR_INVALID, "out_stride %lld: a row is 2*obs_dim + 2 + act_dim = %lld floats", (long long)out_stride,
              (long long)width);
  DevGuard _dg(device_of(out));
  hipLaunchKernelGGL(ep_gather_pairs_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, rows, (long long)row_stride,
                     (long long)n_rows, reinterpret_cast<const long long*>(start), reinterpret_cast<const long long*>(goal), batch,
                     obs_dim, act_dim, out, (long long)out_stride);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
