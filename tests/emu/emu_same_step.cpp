// emu_same_step.cpp -- TEST INFRASTRUCTURE ONLY.  hwy_step_same_step_device on the CPU: the product's validation and sequence
// (highwayenv_amd/csrc/hwy_same_step.h: same_step_validate, same_step_sequence), its stash kernel (hwy_final_kernel) and the
// re-spawn kernels of every family (hwy_device.h: hwy_respawn_kernel / _linear_kernel / _direct_kernel; hwy_wave.h:
// hwy_respawn_wave_kernel / _linear_kernel / _direct_kernel; hwy_wave2.h: hwy_respawn_wide_kernel; hwy_net.h:
// hwy_net_respawn_kernel) through hip_emu.h, on the host SoA arrays of an emulated engine, chosen by the product's launch rules
// (hwy_launch_family.h / hwy_launch_rules.h: select_respawn; hwy_launch_units.h: select_final, select_mask, select_lidar).  The step
// launch itself is the family's own driver's: tests/emu/emu_same_step.py hands it in as a callback, the way hwy_engine.hip's sequence
// calls its step launch first.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_launch_rules.h"
#include "../../highwayenv_amd/csrc/hwy_lidar.h"
#include "../../highwayenv_amd/csrc/hwy_mask.h"
#include "../../highwayenv_amd/csrc/hwy_same_step.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

#include "emu_straight.h"

using emu_straight::EmuBackend;
using emu_straight::HostImage;
using emu_straight::ResetArgs;
using hwy::StepParams;

static std::string g_same_step_error;

namespace {
std::vector<int32_t> packed_words(const hwy_config &c, const hwy_state &st) {
  std::vector<int32_t> packed((size_t)c.num_envs * c.num_vehicles);
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = hwy::pack_word(st.lane[k], st.target_lane[k], st.speed_index[k], st.flags[k], (int)(k % c.num_vehicles));
  return packed;
}

// the planes of one call (the arguments of hwy_step_same_step_device, on host arrays) and the engine's own arrays
struct Call {
  const hwy_config *cfg;
  hwy_state *st;
  double *extra;  // the family's extra planes in the device layout: behaviour [k][E][N] or controls 2 x [E][A]; null otherwise
  uint8_t *done;
  uint32_t *episode;
  float *obs;
  double *reward;
  uint8_t *term, *trunc;
  double *speed;
  uint8_t *crashed;
  float *final_obs;
  double *final_speed;
  uint8_t *final_crashed, *final_mask, *action_mask, *final_action_mask;
  ResetArgs ra;
  int (*step_cb)(void);

  int step() { return step_cb(); }
  int mask(bool final) {
    const std::vector<int32_t> packed = packed_words(*cfg, *st);
    const hwy::MaskParams p = hwy::mask_params(*cfg, st->x, st->y, packed.data(), cfg->num_vehicles, final ? final_action_mask : action_mask);
    return emu::launch_status(hwy::select_mask<emu::PlainBackend>(p, nullptr));
  }
  int stash() {
    const hwy::FinalParams fp = hwy::final_params(*cfg, hwy::obs_len(*cfg), done, final_mask, obs, final_obs, speed, final_speed, crashed,
                                                  final_crashed);
    return emu::launch_status(hwy::select_final<emu::PlainBackend>(fp, nullptr));
  }
  // hwy_engine.hip: launch_stage(RESPAWN) -- the family's kernel around the full step's arguments, a Lidar engine's with a null
  // observation and the trace behind it
  int respawn() {
    const bool lidar = cfg->obs_type == HWY_OBS_LIDAR;
    HostImage img(*cfg, *st);
    StepParams p;
    emu_straight::fill_step_params(cfg, img, st, done, episode, ra, p);
    p.autoreset = 1;
    p.n_frames = cfg->frames_per_step;
    p.full_step = 1;
    p.obs = lidar ? nullptr : obs;
    p.reward = reward; p.terminated = term; p.truncated = trunc; p.info_speed = speed; p.info_crashed = crashed;
    const hwy::Launch l = emu_straight::launch_of(*cfg);
    hipError_t e;
    if (cfg->scenario != HWY_SCENARIO_HIGHWAY) {
      hwy::NetParams np;
      hwy::net_params_from_config(*cfg, p, np);
      e = hwy::select_respawn<EmuBackend>(np, l);
    } else if (cfg->traffic_model == HWY_TRAFFIC_LINEAR) {
      e = hwy::select_respawn<EmuBackend>(hwy::LinearParams{p, hwy::linear_args(*cfg, extra, cfg->num_vehicles)}, l);
    } else if (cfg->ego_control == HWY_EGO_DIRECT) {
      e = hwy::select_respawn<EmuBackend>(hwy::DirectParams{p, hwy::direct_args(*cfg, extra)}, l);
    } else {
      e = hwy::select_respawn<EmuBackend>(p, l);
    }
    img.store(*st);
    if (e != hipSuccess || !lidar) return emu::launch_status(e);
    const std::vector<int32_t> packed = packed_words(*cfg, *st);
    const hwy::LidarParams lp = hwy::lidar_params(*cfg, st->x, st->y, st->heading, st->speed, packed.data(), cfg->num_vehicles, obs);
    return emu::launch_status(hwy::select_lidar<emu::PlainBackend>(lp, cfg->lidar_normalize != 0, cfg->num_envs * cfg->num_agents, nullptr));
  }
};
}  // namespace

extern "C" {

size_t emu_same_step_config_size(void) { return sizeof(hwy_config); }
const char *emu_same_step_last_error(void) { return g_same_step_error.c_str(); }

// what the entry point answers before any launch
int emu_same_step_validate(const hwy_config *cfg, int autoreset, int has_final_obs, int has_final_mask, int has_mask_pointer) {
  const char *why = "";
  int rc = hwy::same_step_validate(*cfg, autoreset != 0, has_final_obs != 0, has_final_mask != 0, &why);
  if (rc == HWY_OK && has_mask_pointer) rc = hwy::mask_validate(*cfg, &why);
  g_same_step_error = why;
  return rc;
}

// The launches behind a passed emu_same_step_validate.  `step`: the family's step launch with auto-reset on (and a Lidar engine's
// trace), which fills obs / reward / term / trunc / speed / crashed and leaves the state in `st`; 0 or a status.
int emu_same_step_run(const hwy_config *cfg, hwy_state *st, double *extra, uint8_t *done, uint32_t *episode, float *obs, double *reward,
                      uint8_t *term, uint8_t *trunc, double *speed, uint8_t *crashed, float *final_obs, double *final_speed,
                      uint8_t *final_crashed, uint8_t *final_mask, uint8_t *action_mask, uint8_t *final_action_mask, uint64_t base_seed,
                      double ego_spacing, double vehicles_density, int initial_lane_id, int (*step)(void)) {
  Call call{cfg, st, extra, done, episode, obs, reward, term, trunc, speed, crashed, final_obs, final_speed, final_crashed, final_mask,
            action_mask, final_action_mask, ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, step};
  g_same_step_error = "a launch rule refused the arguments";
  return hwy::same_step_sequence(call, final_action_mask != nullptr, action_mask != nullptr);
}
}
