// emu_lookahead.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the environment fork and the rollout scoring kernel of the product source
// (highwayenv_amd/csrc/hwy_lookahead.h: hwy_fork_kernel, hwy_score_kernel) on the CPU through hip_emu.h, with the validation
// (fork_validate, score_validate) that hwy_engine.hip makes.  The fork copies between the host SoA arrays of two emulated engines
// (pitch == N; the four integer planes stand where the engine has its packed words); the simulation itself is the family's own
// driver's: tests/emu/emu_lookahead.py rolls the branches out with it and hands the outputs to the scoring kernel, the way the
// engine launches the three on one stream.  The library also exports hip_emu.h's emu_set_schedule / emu_schedule_errors (defined in
// that header, once per emulator library): the scoring kernel's LDS atomics and barriers run under them.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_lookahead.h"

static std::string g_error;

static int refuse(int rc, const std::string &why) { g_error = why; return rc; }

extern "C" {

size_t emu_lookahead_config_size(void) { return sizeof(hwy_config); }
const char *emu_lookahead_last_error(void) { return g_error.c_str(); }

// `extra`: the family's extra planes in the device layout -- behaviour [HWY_BEHAVIOR_PARAMS][E][N] of a Linear engine, stored
// controls [2][E][A] of a direct-control engine, NULL otherwise.  src_env: host indices (validated like hwy_fork) or NULL.
int emu_lookahead_fork(const hwy_config *dst_cfg, const hwy_config *src_cfg, const hwy_state *dst, const hwy_state *src, double *dst_extra,
                       const double *src_extra, uint8_t *dst_done, uint32_t *dst_episode, const uint32_t *src_episode, int32_t branches,
                       const int32_t *src_env) {
  const char *why = "";
  if (const int rc = hwy::fork_validate(*dst_cfg, *src_cfg, dst->x == src->x, branches, src_env != nullptr, &why)) return refuse(rc, why);
  if (src_env)
    for (int j = 0; j < dst_cfg->num_envs; ++j)
      if (src_env[j] < 0 || src_env[j] >= src_cfg->num_envs) return refuse(HWY_ERR_INVALID_ARG, "source index outside [0, src.num_envs)");
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

// what hwy_fork_device answers for two configs before any launch
int emu_lookahead_fork_status(const hwy_config *dst_cfg, const hwy_config *src_cfg, int same_engine, int32_t branches, int has_src_env) {
  const char *why = "";
  const int rc = hwy::fork_validate(*dst_cfg, *src_cfg, same_engine != 0, branches, has_src_env != 0, &why);
  g_error = why;
  return rc;
}

// hwy_score_device on host arrays
int emu_lookahead_score(const hwy_config *cfg, int32_t k_steps, int32_t branches, double gamma, const int32_t *first_action,
                        const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *ret, double *q,
                        int32_t *best_action, int32_t *best_branch) {
  const char *why = "";
  if (const int rc = hwy::score_validate(*cfg, k_steps, branches, gamma, first_action != nullptr, reward && terminated && truncated,
                                         q != nullptr, best_action != nullptr, &why))
    return refuse(rc, why);
  hwy::ScoreParams p;
  memset(&p, 0, sizeof p);
  p.first_action = first_action; p.reward = reward; p.terminated = terminated; p.truncated = truncated;
  p.ret = ret; p.q = q; p.best_action = best_action; p.best_branch = best_branch;
  p.gamma = gamma;
  p.K = k_steps; p.branches = branches; p.A = cfg->num_agents; p.n_ids = hwy::lookahead_num_ids(*cfg);
  p.groups = cfg->num_envs / branches;
  emu::launch([](const hwy::ScoreParams &a) { hwy::hwy_score_kernel<HWY_SCORE_MAX_IDS>(a); }, p.groups, 64, p);
  return HWY_OK;
}
}
