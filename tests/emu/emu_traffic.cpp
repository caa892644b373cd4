// emu_traffic.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the Linear traffic family's kernels of the product source
// (highwayenv_amd/csrc/hwy_wave.h: hwy_step_wave_linear_kernel, hwy_rollout_wave_linear_kernel; hwy_device.h: hwy_step_linear_kernel,
// hwy_rollout_linear_kernel, hwy_reset_linear_kernel) on the CPU through hip_emu.h, on host SoA arrays plus the per-vehicle
// parameter planes.  (emu_engine.cpp is the IDM driver; it has no slot for the planes.)  The driver is emu_straight.h's, the
// arguments and the choice of a kernel the product's own (hwy_params.h: linear_args; hwy_launch_family.h: LinearFamily).
#include "hip_emu.h"

#include "../../highwayenv_amd/csrc/hwy_launch_family.h"
#include "emu_straight.h"

using emu_straight::HostImage;
using emu_straight::ResetArgs;
using hwy::LinearParams;
using hwy::StepParams;

namespace {
// behavior: HWY_BEHAVIOR_PARAMS planes [k][E][N] (pitch == N)
auto linear_family(const hwy_config *cfg, double *behavior) {
  return [=](const StepParams &p, auto &&fn) { fn(LinearParams{p, hwy::linear_args(*cfg, behavior, cfg->num_vehicles)}); };
}
}  // namespace

extern "C" {

size_t emu_traffic_config_size(void) { return sizeof(hwy_config); }

// mode, k_steps: emu_straight::run
int emu_traffic_run(const hwy_config *cfg, hwy_state *st, double *behavior, uint8_t *done, uint32_t *episode, int mode, int n_frames,
                    int k_steps, const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
                    uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
                    int initial_lane_id) {
  HostImage img(*cfg, *st);
  return emu_straight::run(cfg, st, img, emu_straight::launch_of(*cfg), linear_family(cfg, behavior), done, episode, mode, n_frames, k_steps,
                           actions, obs, reward, term, trunc, speed, crashed, autoreset,
                           ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id});
}

int emu_traffic_reset(const hwy_config *cfg, hwy_state *st, double *behavior, uint8_t *done, uint32_t *episode, const uint8_t *mask,
                      const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density, int initial_lane_id,
                      float *obs) {
  HostImage img(*cfg, *st);
  return emu_straight::reset(cfg, st, img, emu_straight::launch_of(*cfg), linear_family(cfg, behavior), done, episode, mask, seeds,
                             ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, obs);
}

void emu_traffic_debug_math(int op, const double *in, double *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = hwy::math_probe(op, in[k]);
}

// the device rule of LinearVehicle.randomize_behavior on Philox draws 2 .. 4 (hwy_device.h: linear_behavior_draw)
void emu_traffic_behavior_draw(uint64_t seed, int vehicle, uint32_t episode, double *out) {
  hwy::linear_behavior_draw(seed, vehicle, episode, out);
}
}
