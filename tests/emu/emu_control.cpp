// emu_control.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the direct-ego-control kernels of the product source
// (highwayenv_amd/csrc/hwy_wave.h: hwy_step_wave_direct_kernel, hwy_rollout_wave_direct_kernel; hwy_device.h: hwy_step_direct_kernel,
// hwy_rollout_direct_kernel, hwy_reset_direct_kernel) on the CPU through hip_emu.h, on host SoA arrays plus the stored controls of
// the agents.  (emu_engine.cpp is the meta-action driver; it has no slot for them.)  The driver itself is emu_straight.h's.
#include "hip_emu.h"

#include "../../highwayenv_amd/csrc/hwy_device.h"
#include "../../highwayenv_amd/csrc/hwy_wave.h"
#include "../../highwayenv_amd/csrc/hwy_params.h"
#include "emu_straight.h"

using emu_straight::ResetArgs;
using hwy::DirectParams;
using hwy::StepParams;

namespace {
struct DirectEmu {
  using Params = DirectParams;
  static StepParams &step_params(Params &a) { return a.s; }
  static const StepParams &step_params(const Params &a) { return a.s; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy::hwy_step_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy::hwy_rollout_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy::hwy_step_direct_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy::hwy_rollout_direct_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy::hwy_reset_direct_kernel<NW>; }
};
DirectParams extra_args(const hwy_config *cfg, double *controls) {
  DirectParams dp;
  std::memset(&dp, 0, sizeof dp);
  dp.da.ctl_accel = controls;
  dp.da.ctl_steer = controls + (size_t)cfg->num_envs * cfg->num_agents;
  dp.da.n_accel = cfg->n_accel;
  dp.da.n_steer = cfg->n_steer;
  for (int k = 0; k < HWY_MAX_ACTIONS_PER_AXIS; ++k) {
    dp.da.accel_axis[k] = cfg->accel_axis[k];
    dp.da.steer_axis[k] = cfg->steer_axis[k];
  }
  return dp;
}
}  // namespace

extern "C" {

size_t emu_control_config_size(void) { return sizeof(hwy_config); }

// mode, k_steps: emu_straight::run.  controls: the stored pairs of the agents, acceleration [E][A] | steering [E][A].
int emu_control_run(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, int mode, int n_frames,
                    int k_steps, const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
                    uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
                    int initial_lane_id) {
  DirectParams a = extra_args(cfg, controls);
  return emu_straight::run<DirectEmu>(cfg, st, a, done, episode, mode, n_frames, k_steps, actions, obs, reward, term, trunc, speed, crashed,
                                  autoreset, ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id});
}

int emu_control_reset(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, const uint8_t *mask,
                      const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density, int initial_lane_id,
                      float *obs) {
  DirectParams a = extra_args(cfg, controls);
  return emu_straight::reset<DirectEmu>(cfg, st, a, done, episode, mask, seeds,
                                    ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, obs);
}
}
