// emu_opd.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the optimistic planner's tree kernel of the product source
// (highwayenv_amd/csrc/hwy_opd.h: hwy_opd_kernel) on the CPU through hip_emu.h, with the validation (opd_validate) that
// hwy_engine.hip makes, and hwy_fork_kernel in its DEVICE form: the source indices are not validated, an index outside the source
// copies nothing -- which is what the planner's scatter relies on.  The simulation is the family's own driver's:
// tests/emu/emu_opd.py launches kernel, gather, step and scatter behind each other the way hwy_opd_plan_device enqueues them.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_opd.h"

static std::string g_error;

extern "C" {

size_t emu_opd_config_size(void) { return sizeof(hwy_config); }
size_t emu_opd_params_size(void) { return sizeof(hwy_opd_params); }
int emu_opd_max_nodes(void) { return HWY_OPD_MAX_NODES; }
const char *emu_opd_last_error(void) { return g_error.c_str(); }

// what hwy_opd_plan_device answers for three configs and the parameters before any launch
int emu_opd_validate(const hwy_config *src, const hwy_config *tree, const hwy_config *work, const hwy_opd_params *params, int has_action) {
  const char *why = "";
  const int rc = hwy::opd_validate(*src, *tree, *work, params, has_action != 0, &why);
  g_error = why;
  return rc;
}

// hwy_fork_device with source indices (tests/emu/emu_lookahead.cpp: emu_lookahead_fork is the validated host form)
int emu_opd_fork_device(const hwy_config *dst_cfg, const hwy_config *src_cfg, const hwy_state *dst, const hwy_state *src, double *dst_extra,
                        const double *src_extra, uint8_t *dst_done, uint32_t *dst_episode, const uint32_t *src_episode, int32_t branches,
                        const int32_t *src_env) {
  const char *why = "";
  if (const int rc = hwy::fork_validate(*dst_cfg, *src_cfg, dst->x == src->x, branches, src_env != nullptr, &why)) { g_error = why; return rc; }
  hwy::ForkParams p;
  memset(&p, 0, sizeof p);
  const double *sf[9] = {src->x, src->y, src->heading, src->speed, src->timer, src->target_speed, src->delta, src->impact_x, src->impact_y};
  double *df[9] = {dst->x, dst->y, dst->heading, dst->speed, dst->timer, dst->target_speed, dst->delta, dst->impact_x, dst->impact_y};
  for (int f = 0; f < 9; ++f) { p.src_f64[f] = sf[f]; p.dst_f64[f] = df[f]; }
  p.n_f64 = 9;
  const int N = dst_cfg->num_vehicles;
  if (dst_cfg->traffic_model == HWY_TRAFFIC_LINEAR)
    for (int f = 0; f < HWY_BEHAVIOR_PARAMS; ++f, ++p.n_f64) {
      p.src_f64[9 + f] = src_extra + (size_t)f * src_cfg->num_envs * N;
      p.dst_f64[9 + f] = dst_extra + (size_t)f * dst_cfg->num_envs * N;
    }
  const int32_t *si[4] = {src->lane, src->target_lane, src->speed_index, src->flags};
  int32_t *di[4] = {dst->lane, dst->target_lane, dst->speed_index, dst->flags};
  for (int f = 0; f < 4; ++f) { p.src_i32[f] = si[f]; p.dst_i32[f] = di[f]; }
  p.n_i32 = 4;
  if (dst_cfg->ego_control == HWY_EGO_DIRECT) { p.src_controls = src_extra; p.dst_controls = dst_extra; }
  p.src_time = src->time; p.dst_time = dst->time;
  p.src_episode = src_episode; p.dst_episode = dst_episode;
  p.dst_done = dst_done;
  p.src_env = src_env;
  p.pitch = N; p.A = dst_cfg->num_agents; p.branches = branches;
  p.src_envs = src_cfg->num_envs; p.dst_envs = dst_cfg->num_envs;
  emu::launch([](const hwy::ForkParams &a) { hwy::hwy_fork_kernel<HWY_FORK_THREADS>(a); }, p.dst_envs, HWY_FORK_THREADS, p);
  return HWY_OK;
}

// launch x of hwy_opd_kernel on host arrays (the layout of hwy::OpdParams)
int emu_opd_kernel(int32_t E, int32_t n, int32_t X, int32_t x, double gamma, double bound, double *ret, double *disc, double *upper0,
                   uint8_t *done, int32_t *expanded_node, const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                   int32_t *gather_src, int32_t *scatter_src, int32_t *root_src, int32_t *actions, int32_t *action, double *value,
                   double *upper, int32_t *sequence, int32_t *expanded) {
  hwy::OpdParams p;
  memset(&p, 0, sizeof p);
  p.ret = ret; p.disc = disc; p.upper0 = upper0; p.done = done; p.expanded_node = expanded_node;
  p.reward = reward; p.terminated = terminated; p.truncated = truncated;
  p.gather_src = gather_src; p.scatter_src = scatter_src; p.root_src = root_src; p.actions = actions;
  p.action = action; p.value = value; p.upper = upper; p.sequence = sequence; p.expanded = expanded;
  p.gamma = gamma; p.bound = bound;
  p.x = x; p.X = X; p.n = n; p.M = 1 + X * n; p.E = E;
  if (p.M > HWY_OPD_MAX_NODES || x < 0 || x > X) { g_error = "launch outside the kernel's capacity"; return HWY_ERR_INVALID_ARG; }
  emu::launch([](const hwy::OpdParams &a) { hwy::hwy_opd_kernel<HWY_OPD_MAX_NODES>(a); }, E, 64, p);
  return HWY_OK;
}
}
