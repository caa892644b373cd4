// emu_continuous.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the continuous-action kernel of the product source
// (highwayenv_amd/csrc/hwy_act.h: hwy_act_continuous_kernel) on the CPU through hip_emu.h, on host arrays, with the product's
// validation (act_validate, act_all_finite) and launch rule (hwy_launch_units.h: select_act_continuous).  The step behind it is the
// direct family's own driver's (emu_control.cpp) with no action ids: tests/emu/emu_continuous.py runs this and then that, the way
// the engine enqueues the two launches on its stream.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_act.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

static std::string g_continuous_error;

extern "C" {

size_t emu_continuous_config_size(void) { return sizeof(hwy_config); }
size_t emu_continuous_params_size(void) { return sizeof(hwy_continuous_params); }
const char *emu_continuous_last_error(void) { return g_continuous_error.c_str(); }

// what the entry points answer for (config, params) before any launch
int emu_continuous_validate(const hwy_config *cfg, const hwy_continuous_params *params) {
  const char *why = "";
  const int rc = hwy::act_validate(*cfg, params, &why);
  g_continuous_error = why;
  return rc;
}
// what the host-pointer entry points answer for the values of `n` action components (HWY_ERR_ACTION: one is not finite)
int emu_continuous_check_finite(const float *actions, long long n) {
  if (hwy::act_all_finite(actions, (size_t)n)) return HWY_OK;
  g_continuous_error = "a continuous action must be finite";
  return HWY_ERR_ACTION;
}
// The launch behind a passed emu_continuous_validate: actions f32 [E][A][size] -> controls (acceleration [E][A] | steering [E][A])
int emu_continuous_act(const hwy_config *cfg, const hwy_continuous_params *params, const float *actions, double *controls) {
  const hwy::ActParams p = hwy::act_params(*cfg, *params, actions, controls);
  g_continuous_error = "the launch rule refused the arguments";
  return emu::launch_status(hwy::select_act_continuous<emu::PlainBackend>(p, nullptr));
}
}
