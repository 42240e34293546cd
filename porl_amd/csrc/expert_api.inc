// The A* expert of the navigation task (porl_nav_rasterize, porl_nav_expert): the host side of csrc/expert.hpp.  Included
// by porl_api.hip behind navsim_api.inc and navsim_discrete_api.inc, whose limits it shares.  Every argument is judged
// before the first device call; no allocation and no synchronisation.

namespace {

// Grid constants of a porl_nav_grid; every rejection names its argument.  No HIP call.
int expert_plan(const porl_nav_grid* p, ExpertGrid* out) {
  if (!p) PORL_FAIL(PORL_ERR_INVALID, "null grid");
  if (!std::isfinite(p->resolution) || !(p->resolution > 0.0))
    PORL_FAIL(PORL_ERR_INVALID, "grid.resolution %g must be positive and finite", p->resolution);
  if (!std::isfinite(p->inflate) || p->inflate < 0.0)
    PORL_FAIL(PORL_ERR_INVALID, "grid.inflate %g must be finite and not negative", p->inflate);
  if (!std::isfinite(p->min_x) || !std::isfinite(p->min_y)) PORL_FAIL(PORL_ERR_INVALID, "grid.min_x / min_y must be finite");
  if (p->w < 1 || p->h < 1) PORL_FAIL(PORL_ERR_INVALID, "grid: w %d and h %d must be positive", p->w, p->h);
  const int64_t pc = ((int64_t)p->w + 2) * ((int64_t)p->h + 2);
  if (pc > AS_MAX_PADDED_CELLS || astar_lds_bytes(pc) > (size_t)AS_MAX_LDS_BYTES || (int64_t)p->w + p->h > AS_MAX_PAIR)
    PORL_FAIL(PORL_ERR_INVALID, "grid: %d x %d cells do not fit one workgroup (%lld padded cells, at most %d; %.0f bytes of "
              "LDS, %d available; w + h at most %d)", p->w, p->h, (long long)pc, AS_MAX_PADDED_CELLS,
              (double)pc * 4.0 + (double)pc / 8.0, AS_MAX_LDS_BYTES, AS_MAX_PAIR);
  ExpertGrid g;
  g.res = p->resolution; g.inflate = p->inflate; g.min_x = p->min_x; g.min_y = p->min_y;
  g.w = p->w; g.h = p->h; g.pw = p->w + 2; g.pcells = (int32_t)pc;
  g.max_sweeps = p->w * p->h;
  *out = g;
  return PORL_OK;
}

}  // namespace

extern "C" {

int porl_nav_rasterize(const float* segments, int32_t M, const float* circles, int32_t C, const porl_nav_grid* grid,
                       uint32_t* bitmap, int64_t n_words, void* stream) {
  if (M < 0) PORL_FAIL(PORL_ERR_INVALID, "M %d must not be negative", M);
  if (C < 0) PORL_FAIL(PORL_ERR_INVALID, "C %d must not be negative", C);
  if ((int64_t)M + (int64_t)C > PORL_NAV_MAX_PRIMS)
    PORL_FAIL(PORL_ERR_INVALID, "M + C = %lld primitives, at most %d", (long long)M + C, PORL_NAV_MAX_PRIMS);
  if (M > 0 && !segments) PORL_FAIL(PORL_ERR_INVALID, "null segments (M = %d)", M);
  if (C > 0 && !circles) PORL_FAIL(PORL_ERR_INVALID, "null circles (C = %d)", C);
  ExpertGrid g;
  PORL_TRY(expert_plan(grid, &g));
  if (!bitmap) PORL_FAIL(PORL_ERR_INVALID, "null bitmap");
  const int64_t need = ((int64_t)g.pcells + 31) / 32;
  if (n_words < need || n_words > (int64_t(1) << 24))
    PORL_FAIL(PORL_ERR_INVALID, "n_words %lld: the bitmap of %d padded cells is %lld words", (long long)n_words, g.pcells,
              (long long)need);
  DevGuard _dg(device_of(bitmap));
  hipLaunchKernelGGL(nav_rasterize_kernel, dim3((unsigned)((g.pcells + EX_RASTER_THREADS - 1) / EX_RASTER_THREADS)),
                     dim3(EX_RASTER_THREADS), 0, (hipStream_t)stream, segments, (int)M, circles, (int)C, g, bitmap, (int)need);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_nav_expert(const porl_nav_grid* grid, const uint32_t* bitmap, const porl_nav_expert_params* params,
                    const double* state, uint32_t* field, int64_t* tag, float* commands, int64_t cmd_stride, float* scores,
                    int64_t score_stride, double* waypoint, int32_t* path_len, int32_t* status, int32_t* path, int64_t n,
                    void* stream) {
  ExpertGrid g;
  PORL_TRY(expert_plan(grid, &g));
  if (!bitmap) PORL_FAIL(PORL_ERR_INVALID, "null bitmap");
  if (!params) PORL_FAIL(PORL_ERR_INVALID, "null params");
  if (!nav_pos(params->dt) || params->dt > 10.0) PORL_FAIL(PORL_ERR_INVALID, "dt outside (0, 10]");
  if (!(params->max_lin_vel >= 0.0) || !std::isfinite(params->max_lin_vel))
    PORL_FAIL(PORL_ERR_INVALID, "max_lin_vel must be finite and not negative");
  if (!(params->max_ang_vel >= 0.0) || !std::isfinite(params->max_ang_vel))
    PORL_FAIL(PORL_ERR_INVALID, "max_ang_vel must be finite and not negative");
  if (params->lookahead < 1) PORL_FAIL(PORL_ERR_INVALID, "lookahead %d must be at least 1", params->lookahead);
  if (params->max_path < 0) PORL_FAIL(PORL_ERR_INVALID, "max_path %d must not be negative", params->max_path);
  if (params->reserved) PORL_FAIL(PORL_ERR_INVALID, "reserved must be 0");
  if (!state) PORL_FAIL(PORL_ERR_INVALID, "null state");
  if (!field) PORL_FAIL(PORL_ERR_INVALID, "null field");
  if (!tag) PORL_FAIL(PORL_ERR_INVALID, "null tag");
  if (n < 1 || n > NAV_MAX_ROBOTS) PORL_FAIL(PORL_ERR_INVALID, "n %lld outside [1, 2^24]", (long long)n);
  if (commands) {
    if (cmd_stride < 2 || cmd_stride > NAV_MAX_STRIDE)
      PORL_FAIL(PORL_ERR_INVALID, "cmd_stride %lld: a command is 2 floats", (long long)cmd_stride);
  } else if (cmd_stride != 0) {
    PORL_FAIL(PORL_ERR_INVALID, "cmd_stride %lld without commands (pass 0)", (long long)cmd_stride);
  }
  if (scores) {
    if (params->n_actions < 1 || params->n_actions > SELECT_MAX_ACTIONS)
      PORL_FAIL(PORL_ERR_INVALID, "n_actions %d outside [1, %d]", params->n_actions, SELECT_MAX_ACTIONS);
    if (!(params->ang_step >= 0.0) || !std::isfinite(params->ang_step))
      PORL_FAIL(PORL_ERR_INVALID, "ang_step must be finite and not negative");
    if (score_stride < params->n_actions || score_stride > NAV_MAX_STRIDE)
      PORL_FAIL(PORL_ERR_INVALID, "score_stride %lld: a row of scores is %d floats", (long long)score_stride, params->n_actions);
  } else if (score_stride != 0) {
    PORL_FAIL(PORL_ERR_INVALID, "score_stride %lld without scores (pass 0)", (long long)score_stride);
  }
  if (path && (int64_t)params->max_path * n > (int64_t(1) << 40))
    PORL_FAIL(PORL_ERR_INVALID, "max_path %d x n %lld: the path output is too large", params->max_path, (long long)n);
  const size_t lds = astar_lds_bytes(g.pcells);
  DevGuard _dg(device_of(state));
  hipStream_t s = (hipStream_t)stream;
  PORL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&nav_field_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL(nav_field_kernel, dim3((unsigned)n), dim3(AS_THREADS), lds, s, g, bitmap, state, field,
                     reinterpret_cast<long long*>(tag));
  PORL_HIP(hipGetLastError());
  ExpertSteerArgs a{};
  a.state = state; a.tag = reinterpret_cast<const long long*>(tag); a.field = field; a.bitmap = bitmap;
  a.n = (long long)n;
  a.lookahead = params->lookahead; a.max_path = path ? params->max_path : 0; a.n_actions = params->n_actions;
  a.dt = params->dt; a.max_lin_vel = params->max_lin_vel; a.max_ang_vel = params->max_ang_vel; a.ang_step = params->ang_step;
  a.commands = commands; a.cmd_stride = (long long)cmd_stride;
  a.scores = scores; a.score_stride = (long long)score_stride;
  a.waypoint = waypoint; a.path_len = path_len; a.status = status; a.path = path;
  hipLaunchKernelGGL(nav_steer_kernel, dim3((unsigned)((n + EX_STEER_THREADS - 1) / EX_STEER_THREADS)), dim3(EX_STEER_THREADS),
                     0, s, g, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
