// emu_lookahead.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the environment fork and the rollout scoring kernel of the product source
// (highwayenv_amd/csrc/hwy_lookahead.h: hwy_fork_kernel, hwy_score_kernel) on the CPU through hip_emu.h, with the product's
// validation (fork_validate, score_validate), arguments (fork_params, score_params) and launch rules (hwy_launch_units.h).  The fork
// copies between the host SoA arrays of two emulated engines (emu_fork.h); the simulation itself is the family's own driver's:
// tests/emu/emu.py rolls the branches out with it and hands the outputs to the scoring kernel, the way the engine launches the
// three on one stream.  The library also exports hip_emu.h's emu_set_schedule / emu_schedule_errors (defined in that header, once
// per emulator library): the scoring kernel's LDS atomics and barriers run under them.
#include "hip_emu.h"

#include <string>

#include "emu_fork.h"

static std::string g_error;

static int refuse(int rc, const std::string &why) { g_error = why; return rc; }

extern "C" {

size_t emu_lookahead_config_size(void) { return sizeof(hwy_config); }
const char *emu_lookahead_last_error(void) { return g_error.c_str(); }

// what hwy_fork_device answers for two configs before any launch
int emu_lookahead_fork_status(const hwy_config *dst_cfg, const hwy_config *src_cfg, int same_engine, int32_t branches, int has_src_env) {
  const char *why = "";
  return refuse(hwy::fork_validate(*dst_cfg, *src_cfg, same_engine != 0, branches, has_src_env != 0, &why), why);
}
// The launch behind a passed emu_lookahead_fork_status.  host_indices: src_env is hwy_fork's host array, validated like there;
// otherwise it stands for hwy_fork_device's device array.
int emu_lookahead_fork(const emu_engine_view *dst, const emu_engine_view *src, int32_t branches, const int32_t *src_env, int host_indices) {
  if (src_env && host_indices)
    for (int j = 0; j < dst->cfg->num_envs; ++j)
      if (src_env[j] < 0 || src_env[j] >= src->cfg->num_envs) return refuse(HWY_ERR_INVALID_ARG, "source index outside [0, src.num_envs)");
  return refuse(emu_fork::fork(*dst, *src, branches, src_env), "the launch rule refused the arguments");
}

// what hwy_score_device answers before any launch
int emu_lookahead_score_status(const hwy_config *cfg, int32_t k_steps, int32_t branches, double gamma, int has_first, int has_reward_and_flags,
                               int has_q, int has_best_action) {
  const char *why = "";
  return refuse(hwy::score_validate(*cfg, k_steps, branches, gamma, has_first != 0, has_reward_and_flags != 0, has_q != 0, has_best_action != 0,
                                    &why), why);
}
// The launch behind a passed emu_lookahead_score_status: hwy_score_device on host arrays
int emu_lookahead_score(const hwy_config *cfg, int32_t k_steps, int32_t branches, double gamma, const int32_t *first_action,
                        const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *ret, double *q,
                        int32_t *best_action, int32_t *best_branch) {
  const hwy::ScoreParams p = hwy::score_params(*cfg, k_steps, branches, gamma, first_action, reward, terminated, truncated, ret, q,
                                               best_action, best_branch);
  return refuse(emu::launch_status(hwy::select_score<emu::PlainBackend>(p, nullptr)), "the launch rule refused the arguments");
}
}
