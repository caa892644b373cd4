// emu_control.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the direct-ego-control kernels of the product source
// (highwayenv_amd/csrc/hwy_wave.h: hwy_step_wave_direct_kernel, hwy_rollout_wave_direct_kernel; hwy_device.h: hwy_step_direct_kernel,
// hwy_rollout_direct_kernel, hwy_reset_direct_kernel) on the CPU through hip_emu.h, on host SoA arrays plus the stored controls of
// the agents.  (emu_engine.cpp is the meta-action driver; it has no slot for them.)  The driver is emu_straight.h's, the arguments
// and the choice of a kernel the product's own (hwy_params.h: direct_args; hwy_launch_family.h: DirectFamily).
#include "hip_emu.h"

#include "../../highwayenv_amd/csrc/hwy_launch_family.h"
#include "emu_straight.h"

using emu_straight::HostImage;
using emu_straight::ResetArgs;
using hwy::DirectParams;
using hwy::StepParams;

namespace {
// controls: the stored pairs of the agents, acceleration [E][A] | steering [E][A]
auto direct_family(const hwy_config *cfg, double *controls) {
  return [=](const StepParams &p, auto &&fn) { fn(DirectParams{p, hwy::direct_args(*cfg, controls)}); };
}
}  // namespace

extern "C" {

size_t emu_control_config_size(void) { return sizeof(hwy_config); }

// mode, k_steps: emu_straight::run
int emu_control_run(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, int mode, int n_frames,
                    int k_steps, const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
                    uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
                    int initial_lane_id) {
  HostImage img(*cfg, *st);
  return emu_straight::run(cfg, st, img, emu_straight::launch_of(*cfg), direct_family(cfg, controls), done, episode, mode, n_frames, k_steps,
                           actions, obs, reward, term, trunc, speed, crashed, autoreset,
                           ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id});
}

int emu_control_reset(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, const uint8_t *mask,
                      const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density, int initial_lane_id,
                      float *obs) {
  HostImage img(*cfg, *st);
  return emu_straight::reset(cfg, st, img, emu_straight::launch_of(*cfg), direct_family(cfg, controls), done, episode, mask, seeds,
                             ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, obs);
}
}
