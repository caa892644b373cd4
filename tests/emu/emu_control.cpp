// emu_control.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the direct-ego-control kernels of the product source
// (highwayenv_amd/csrc/hwy_wave.h: hwy_step_wave_direct_kernel, hwy_rollout_wave_direct_kernel; hwy_device.h: hwy_step_direct_kernel,
// hwy_rollout_direct_kernel, hwy_reset_direct_kernel) on the CPU through hip_emu.h, on host SoA arrays plus the stored controls of
// the agents.  (emu_engine.cpp is the meta-action driver; it has no slot for them.)
#include "hip_emu.h"

#include <cstring>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_device.h"
#include "../../highwayenv_amd/csrc/hwy_wave.h"
#include "../../highwayenv_amd/csrc/hwy_params.h"

using hwy::DirectParams;
using hwy::StepParams;

namespace {
// the device image of the state: 9 f64 planes [field][E][N] + the packed words (pitch == N)
struct Image {
  int E, N;
  std::vector<double> f64;
  std::vector<int32_t> packed;
  Image(const hwy_config &c, const hwy_state &h) : E(c.num_envs), N(c.num_vehicles) {
    const size_t plane = (size_t)E * N;
    f64.resize(plane * 9);
    packed.resize(plane);
    const double *fields[9] = {h.x, h.y, h.heading, h.speed, h.timer, h.target_speed, h.delta, h.impact_x, h.impact_y};
    for (int f = 0; f < 9; ++f) std::memcpy(&f64[f * plane], fields[f], plane * sizeof(double));
    for (size_t k = 0; k < plane; ++k) packed[k] = hwy::pack_word(h.lane[k], h.target_lane[k], h.speed_index[k], h.flags[k], (int)(k % N));
  }
  void store(hwy_state &h) const {
    const size_t plane = (size_t)E * N;
    double *fields[9] = {h.x, h.y, h.heading, h.speed, h.timer, h.target_speed, h.delta, h.impact_x, h.impact_y};
    for (int f = 0; f < 9; ++f) std::memcpy(fields[f], &f64[f * plane], plane * sizeof(double));
    for (size_t k = 0; k < plane; ++k) {
      const int32_t w = packed[k];
      h.lane[k] = hwy::word_lane(w); h.target_lane[k] = hwy::word_target(w); h.speed_index[k] = hwy::word_speed_index(w);
      h.flags[k] = hwy::word_flags(w);
      if (!(h.flags[k] & HWY_F_HAS_IMPACT)) h.impact_x[k] = h.impact_y[k] = 0.0;  // as hwy_get_state does
    }
  }
};

// controls: the stored pairs of the agents, acceleration [E][A] | steering [E][A]
void fill(const hwy_config *cfg, Image &img, hwy_state *st, uint8_t *done, uint32_t *episode, double *controls, uint64_t base_seed,
          double ego_spacing, double vehicles_density, int initial_lane_id, DirectParams &dp) {
  std::memset(&dp, 0, sizeof dp);
  StepParams &p = dp.s;
  hwy::params_from_config(*cfg, cfg->num_vehicles, p);
  hwy::bind_planes(img.f64.data(), (size_t)cfg->num_envs * cfg->num_vehicles, p.st);
  p.st.packed = img.packed.data();
  p.st.time = st->time;
  p.st.done = done;
  p.st.episode = episode;
  p.rp.ego_spacing = ego_spacing;
  p.rp.other_spacing = 1 / vehicles_density;
  p.rp.lane_factor = exp(-5.0 / 40.0 * cfg->lanes_count);
  p.rp.initial_lane_id = initial_lane_id;
  p.rp.fast = (cfg->flags & HWY_C_EGO_ONLY_COLLISIONS) ? 1 : 0;
  p.rp.base_seed = base_seed;
  dp.da.ctl_accel = controls;
  dp.da.ctl_steer = controls + (size_t)cfg->num_envs * cfg->num_agents;
  dp.da.n_accel = cfg->n_accel;
  dp.da.n_steer = cfg->n_steer;
  for (int k = 0; k < HWY_MAX_ACTIONS_PER_AXIS; ++k) {
    dp.da.accel_axis[k] = cfg->accel_axis[k];
    dp.da.steer_axis[k] = cfg->steer_axis[k];
  }
}

enum Which { STEP, ROLLOUT, RESET, OBSERVE };
// same dispatch rule as hwy_kernels_direct.hip: the one-wavefront kernel for N <= 64 unless tune_block_kernel == 1
void dispatch(Which which, const DirectParams &dp, int E, const hwy_config *cfg) {
  const int nw = (dp.s.N + 63) / 64;
  if ((which == STEP || which == ROLLOUT) && dp.s.N <= 64 && cfg->tune_block_kernel != 1) {
    const bool full = !(dp.s.flags & HWY_C_EGO_ONLY_COLLISIONS);
    if (which == ROLLOUT) {
      if (full) emu::launch([](const DirectParams &q) { hwy::hwy_rollout_wave_direct_kernel<1, true>(q); }, E, 64, dp);
      else emu::launch([](const DirectParams &q) { hwy::hwy_rollout_wave_direct_kernel<1, false>(q); }, E, 64, dp);
    } else {
      if (full) emu::launch([](const DirectParams &q) { hwy::hwy_step_wave_direct_kernel<1, true>(q); }, E, 64, dp);
      else emu::launch([](const DirectParams &q) { hwy::hwy_step_wave_direct_kernel<1, false>(q); }, E, 64, dp);
    }
    return;
  }
#define RUN(NW)                                                                                                         \
  switch (which) {                                                                                                      \
    case STEP: emu::launch([](const DirectParams &q) { hwy::hwy_step_direct_kernel<NW, 1>(q); }, E, NW * 64, dp); break;     \
    case ROLLOUT: emu::launch([](const DirectParams &q) { hwy::hwy_rollout_direct_kernel<NW, 1>(q); }, E, NW * 64, dp); break; \
    case RESET: emu::launch([](const DirectParams &q) { hwy::hwy_reset_direct_kernel<NW>(q); }, E, NW * 64, dp); break;      \
    case OBSERVE: emu::launch([](const StepParams &q) { hwy::hwy_observe_kernel<NW>(q); }, E, NW * 64, dp.s); break;        \
  }
  switch (nw) {
    case 1: RUN(1) break;
    case 2: RUN(2) break;
    case 3: RUN(3) break;
    default: RUN(4) break;
  }
#undef RUN
}
}  // namespace

extern "C" {

size_t emu_control_config_size(void) { return sizeof(hwy_config); }

// mode: 0 = frames only (hwy_step_frames), 1 = full policy step(s) (hwy_step; k_steps > 0: hwy_rollout_device), 2 = observe only.
int emu_control_run(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, int mode, int n_frames,
                    int k_steps, const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
                    uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
                    int initial_lane_id) {
  Image img(*cfg, *st);
  DirectParams dp;
  fill(cfg, img, st, done, episode, controls, base_seed, ego_spacing, vehicles_density, initial_lane_id, dp);
  StepParams &p = dp.s;
  p.autoreset = autoreset;
  p.actions = actions; p.obs = obs; p.reward = reward; p.terminated = term; p.truncated = trunc;
  p.info_speed = speed; p.info_crashed = crashed;
  if (mode == 2) {
    dispatch(OBSERVE, dp, cfg->num_envs, cfg);
  } else {
    p.n_frames = n_frames;
    p.full_step = mode == 1;
    if (mode == 0) p.autoreset = 0;
    if (mode == 1 && k_steps > 0) {
      p.k_steps = k_steps;
      p.num_envs = cfg->num_envs;
      dispatch(ROLLOUT, dp, cfg->num_envs, cfg);
    } else {
      dispatch(STEP, dp, cfg->num_envs, cfg);
    }
  }
  img.store(*st);
  return 0;
}

int emu_control_reset(const hwy_config *cfg, hwy_state *st, double *controls, uint8_t *done, uint32_t *episode, const uint8_t *mask,
                      const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density, int initial_lane_id,
                      float *obs) {
  Image img(*cfg, *st);
  DirectParams dp;
  fill(cfg, img, st, done, episode, controls, base_seed, ego_spacing, vehicles_density, initial_lane_id, dp);
  dp.s.reset_mask = mask;
  dp.s.reset_seeds = seeds;
  dp.s.obs = obs;
  dispatch(RESET, dp, cfg->num_envs, cfg);
  img.store(*st);
  return 0;
}
}
