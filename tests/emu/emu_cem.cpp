// emu_cem.cpp -- TEST INFRASTRUCTURE ONLY.  Runs a plan of the CEM planner on the CPU through hip_emu.h: the product's validation
// (cem_validate), arguments (cem_params), launch rules (hwy_launch_units.h: select_cem_sample, select_cem_refit, select_fork,
// select_score) and SEQUENCE (highwayenv_amd/csrc/hwy_cem.h: cem_iterate, the template hwy_cem_plan_device enqueues on the device),
// with the two kernels, the fork (emu_fork.h) and the fold run here, inside the one call that holds the schedule, and the work
// engine's K (act, step) pairs -- which live in other emulator libraries -- called back into tests/emu/emu_cem.py.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_cem.h"
#include "emu_fork.h"

static std::string g_error;

// a backend that launches nothing and records the grid and the block a rule asked for
struct Dry {
  template <typename K_, typename A>
  static hipError_t launch_plain(K_, int grid, int block, int, hipStream_t, const A &) { g = grid; b = block; return hipSuccess; }
  static inline int g = 0, b = 0;
};

extern "C" {

size_t emu_cem_config_size(void) { return sizeof(hwy_config); }
size_t emu_cem_continuous_size(void) { return sizeof(hwy_continuous_params); }
size_t emu_cem_params_size(void) { return sizeof(hwy_cem_params); }
size_t emu_cem_arrays_size(void) { return sizeof(hwy::CemArrays); }
int emu_cem_max_pop(void) { return HWY_CEM_MAX_POP; }
int emu_cem_max_horizon(void) { return HWY_CEM_MAX_HORIZON; }
int emu_cem_refit_lds_cap(void) { return HWY_CEM_REFIT_LDS_CAP; }
unsigned emu_cem_stream_tag(void) { return HWY_CEM_STREAM_TAG; }
const char *emu_cem_last_error(void) { return g_error.c_str(); }

// what hwy_cem_plan_device answers for two configs and the parameters before any launch
int emu_cem_validate(const hwy_config *src, const hwy_config *work, const hwy_continuous_params *cp, const hwy_cem_params *params,
                     int has_action) {
  const char *why = "";
  const int rc = hwy::cem_validate(*src, *work, cp, params, has_action != 0, &why);
  g_error = why;
  return rc;
}
// what hwy_cem_plan answers for the values of an init_mean (HWY_ERR_ACTION: one is not finite)
int emu_cem_check_finite(const double *init_mean, long long n) {
  if (hwy::cem_all_finite(init_mean, (size_t)n)) return HWY_OK;
  g_error = "init_mean must be finite";
  return HWY_ERR_ACTION;
}

// the two uniforms of the sample kernel's Philox block of (environment, branch, draw) under `seed`
void emu_cem_uniform2(uint64_t seed, uint32_t env, uint32_t branch, uint32_t draw, double *u0, double *u1) {
  hwy::cem_uniform2(seed, env, branch, draw, u0, u1);
}

// the work engine's K (act, step) pairs on a->actions, outputs to reward | terminated | truncated: 0 or a status
typedef int (*emu_cem_callback)(void);

// The launches behind a passed emu_cem_validate: hwy_cem_plan_device on the host arrays of two engines and of the planner.
int emu_cem_plan(const emu_engine_view *src, const emu_engine_view *work, const hwy_continuous_params *cp, const hwy_cem_params *params,
                 const hwy::CemArrays *a, double *ret, const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                 emu_cem_callback rollout) {
  struct Ops {
    const emu_engine_view *src, *work;
    double gamma, *ret;
    const double *reward;
    const uint8_t *terminated, *truncated;
    emu_cem_callback rollout_;
    int sample(const hwy::CemParams &p) { return emu::launch_status(hwy::select_cem_sample<emu::PlainBackend>(p, nullptr)); }
    int fork(int32_t branches) {
      const char *why = "";
      if (const int rc = hwy::fork_validate(*work->cfg, *src->cfg, false, branches, false, &why)) { g_error = why; return rc; }
      return emu_fork::fork(*work, *src, branches, nullptr);
    }
    int rollout(int32_t) { return rollout_(); }
    int score(int32_t k_steps, int32_t branches) {
      const char *why = "";
      if (const int rc = hwy::score_validate(*work->cfg, k_steps, branches, gamma, false, true, false, false, &why)) { g_error = why; return rc; }
      return emu::launch_status(hwy::select_score<emu::PlainBackend>(
          hwy::score_params(*work->cfg, k_steps, branches, gamma, nullptr, reward, terminated, truncated, ret, nullptr, nullptr, nullptr), nullptr));
    }
    int refit(const hwy::CemParams &p) { return emu::launch_status(hwy::select_cem_refit<emu::PlainBackend>(p, nullptr)); }
  };
  g_error = "a launch rule refused the arguments";
  return hwy::cem_iterate(hwy::cem_params(*params, *cp, src->cfg->num_envs, *a, ret),
                          Ops{src, work, params->gamma, ret, reward, terminated, truncated, rollout});
}

// One launch of the sample kernel alone (iteration `iter` of a search of E environments), for the statistics of its draws.
int emu_cem_sample(const hwy_continuous_params *cp, const hwy_cem_params *params, int32_t num_envs, int32_t iter, const hwy::CemArrays *a) {
  hwy::CemParams p = hwy::cem_params(*params, *cp, num_envs, *a, nullptr);
  p.iter = iter;
  g_error = "a launch rule refused the arguments";
  return emu::launch_status(hwy::select_cem_sample<emu::PlainBackend>(p, nullptr));
}

// what the two launch rules answer for a shape (0: launched nothing but would; -2: refused), without running a kernel
int emu_cem_rules(int32_t E, int32_t B, int32_t K, int32_t size, int32_t M, int32_t I, int32_t iter, int with_arrays, int *sample, int *refit) {
  static float f32[4];
  static double f64[4];
  hwy::CemParams p;
  memset(&p, 0, sizeof p);
  p.E = E; p.B = B; p.K = K; p.size = size; p.M = M; p.I = I; p.iter = iter;
  if (with_arrays) { p.actions = f32; p.mean = f64; p.stddev = f64; p.ret = f64; p.best_return = f64; p.best_sequence = f32; p.action = f32; }
  Dry::g = Dry::b = 0;
  sample[0] = emu::launch_status(hwy::select_cem_sample<Dry>(p, nullptr)); sample[1] = Dry::g; sample[2] = Dry::b;
  Dry::g = Dry::b = 0;
  refit[0] = emu::launch_status(hwy::select_cem_refit<Dry>(p, nullptr)); refit[1] = Dry::g; refit[2] = Dry::b;
  return 0;
}

// The sequence cem_iterate runs for I iterations of B branches and K steps, as text: one word per operation, in order.
int emu_cem_sequence(int32_t I, int32_t B, int32_t K, char *buf, int len) {
  struct Ops {
    std::string text;
    int sample(const hwy::CemParams &p) { text += "sample(" + std::to_string(p.iter) + ") "; return 0; }
    int fork(int32_t branches) { text += "fork(work,src," + std::to_string(branches) + ") "; return 0; }
    int rollout(int32_t k) { text += "rollout(" + std::to_string(k) + ") "; return 0; }
    int score(int32_t k, int32_t b) { text += "score(" + std::to_string(k) + "," + std::to_string(b) + ") "; return 0; }
    int refit(const hwy::CemParams &p) { text += "refit(" + std::to_string(p.iter) + ") "; return 0; }
  } ops;
  hwy::CemParams p;
  memset(&p, 0, sizeof p);
  p.I = I; p.B = B; p.K = K;
  const int rc = hwy::cem_iterate(p, ops);
  if (len > 0) { strncpy(buf, ops.text.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
  return rc;
}
}
