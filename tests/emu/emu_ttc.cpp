// emu_ttc.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the time-to-collision grid / finite-MDP planner kernel of the product source
// (highwayenv_amd/csrc/hwy_ttc.h: hwy_ttc_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a state, with the
// validation (ttc_validate) and the choice of the LDS class that hwy_engine.hip / hwy_kernels_ttc.hip make.  The simulation itself
// is the family's own driver's: tests/emu/emu_ttc.py runs it and then this, the way the engine launches the kernel on its stream.
// The library also exports hip_emu.h's emu_set_schedule / emu_schedule_errors (defined in that header, once per emulator library):
// tests/test_schedule_independence.py runs the kernel's LDS atomics, its barriers and its double-buffered value slices under them.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_ttc.h"

static std::string g_ttc_error;

static int run(const hwy_config *cfg, const hwy_state *st, const hwy_ttc_params *tp, bool plan, float *grid, int32_t *action, double *q) {
  const char *why = "";
  if (const int rc = hwy::ttc_validate(*cfg, tp, &why)) { g_ttc_error = why; return rc; }
  if (plan ? !action : !grid) { g_ttc_error = "NULL output"; return HWY_ERR_INVALID_ARG; }
  const int E = cfg->num_envs, N = cfg->num_vehicles;
  std::vector<int32_t> packed((size_t)E * N);
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = hwy::pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k], (int)(k % N));
  const hwy::TtcParams p = hwy::ttc_params(*cfg, *tp, st->x, st->heading, st->speed, packed.data(), N, grid, action, q);
  const int rows = E * cfg->num_agents;
  const bool small = hwy::ttc_cells(*cfg, *tp) <= HWY_TTC_SMALL_CELLS;
  if (plan) {
    if (small) emu::launch([](const hwy::TtcParams &a) { hwy::hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, true>(a); }, rows, 64, p);
    else emu::launch([](const hwy::TtcParams &a) { hwy::hwy_ttc_kernel<HWY_TTC_MAX_CELLS, true>(a); }, rows, 64, p);
  } else {
    if (small) emu::launch([](const hwy::TtcParams &a) { hwy::hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, false>(a); }, rows, 64, p);
    else emu::launch([](const hwy::TtcParams &a) { hwy::hwy_ttc_kernel<HWY_TTC_MAX_CELLS, false>(a); }, rows, 64, p);
  }
  return HWY_OK;
}

extern "C" {

size_t emu_ttc_config_size(void) { return sizeof(hwy_config); }
size_t emu_ttc_params_size(void) { return sizeof(hwy_ttc_params); }
const char *emu_ttc_last_error(void) { return g_ttc_error.c_str(); }

// what the entry points answer for (config, params) before any launch
int emu_ttc_validate(const hwy_config *cfg, const hwy_ttc_params *tp) {
  const char *why = "";
  const int rc = hwy::ttc_validate(*cfg, tp, &why);
  g_ttc_error = why;
  return rc;
}
// the grid of the state `st` ([E][N] planes, pitch == N) -> f32 [E][A][V][L][T]
int emu_ttc_grid(const hwy_config *cfg, const hwy_state *st, const hwy_ttc_params *tp, float *grid) {
  return run(cfg, st, tp, false, grid, nullptr, nullptr);
}
// ... and the plan on it: action int32 [E][A], q f64 [E][A][5] (may be NULL), grid (may be NULL)
int emu_mdp_plan(const hwy_config *cfg, const hwy_state *st, const hwy_ttc_params *tp, int32_t *action, double *q, float *grid) {
  return run(cfg, st, tp, true, grid, action, q);
}
}
