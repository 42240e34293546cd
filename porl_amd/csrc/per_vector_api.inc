// Prioritized replay for the vectorised loop (porl_per_fill_range, porl_per_sample_keyed): the host side of
// csrc/per_vector.hpp.  Included by porl_api.hip behind per_online.hpp's entry points, whose per_levels() it shares.  Every
// argument is judged before the first device call; one launch each, no allocation and no synchronisation.

extern "C" {

int porl_per_fill_range(double* tree, int64_t capacity, int64_t first_slot, int64_t n, double td_error, double eps,
                        double alpha, void* stream) {
  if (!tree) PORL_FAIL(PORL_ERR_INVALID, "null tree");
  if (capacity < 1 || capacity > (int64_t(1) << 40))
    PORL_FAIL(PORL_ERR_INVALID, "capacity %lld outside [1, 2^40]", (long long)capacity);
  if (n < 0 || n > capacity) PORL_FAIL(PORL_ERR_INVALID, "n %lld outside [0, capacity = %lld]", (long long)n, (long long)capacity);
  if (first_slot < 0 || first_slot >= capacity)
    PORL_FAIL(PORL_ERR_INVALID, "first_slot %lld outside [0,%lld)", (long long)first_slot, (long long)capacity);
  if (!std::isfinite(td_error)) PORL_FAIL(PORL_ERR_INVALID, "td_error must be finite");
  if (!std::isfinite(eps)) PORL_FAIL(PORL_ERR_INVALID, "eps must be finite");
  if (!std::isfinite(alpha)) PORL_FAIL(PORL_ERR_INVALID, "alpha must be finite");
  if (n == 0) return PORL_OK;
  PerFillArgs a{};
  a.tree = tree; a.capacity = capacity; a.first_slot = first_slot; a.n = n;
  a.td_error = td_error; a.eps = eps; a.alpha = alpha;
  a.top = per_levels(capacity);
  per_fill_plan(&a);
  DevGuard _dg(device_of(tree));
  const int threads = n >= 1024 ? 1024 : (int)((n + 63) / 64 * 64);
  hipLaunchKernelGGL(per_fill_range_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_per_sample_keyed(const double* tree, int64_t capacity, uint64_t seed, int64_t draw, int32_t batch, int64_t n_entries,
                          double beta, int64_t* out_idx, int64_t* out_slots, float* out_w, float* out_wmean, double* scratch,
                          void* stream) {
  if (!tree || !out_idx || !out_slots || !out_w || !out_wmean || !scratch) PORL_FAIL(PORL_ERR_INVALID, "null argument");
  if (capacity < 1 || batch < 1 || n_entries < 1 || n_entries > capacity)
    PORL_FAIL(PORL_ERR_INVALID, "need capacity >= 1, batch >= 1, 1 <= n_entries <= capacity");
  // the counter is (draw << 32) | i: both halves must fit their 32 bits
  static_assert(sizeof(batch) <= 4, "sample i < batch rides in the low 32 bits of the counter");
  if (draw < 0 || draw > PER_KEYED_MAX_DRAW)
    PORL_FAIL(PORL_ERR_INVALID, "draw %lld outside [0, 2^32): it rides in the high half of the counter", (long long)draw);
  DevGuard _dg(device_of(tree));
  PerSampleSlotsArgs a{tree, capacity, nullptr, batch, n_entries, beta, out_idx, out_slots, out_w, out_wmean, scratch};
  hipLaunchKernelGGL(per_sample_keyed_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, per_keyed_key(seed), (uint64_t)draw);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
