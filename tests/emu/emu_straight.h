// emu_straight.h -- TEST INFRASTRUCTURE ONLY.  The ONE driver of the CPU emulation (emu_engine.cpp: IDM with meta-actions on every
// scenario, emu_traffic.cpp: Linear traffic, emu_control.cpp: direct ego control): the host image of the state, the binding of
// StepParams to it, and the emulation's backend of the product's launch layer.  Nothing here builds a family's arguments or picks a
// kernel: hwy_config -> arguments is highwayenv_amd/csrc/hwy_params.h, (arguments, Launch) -> (kernel, grid, block) is
// hwy_launch_family.h / hwy_launch_rules.h -- the code hwy_engine.hip and the hwy_kernels*.hip units run, here with EmuBackend.
// Include it AFTER hip_emu.h and the product headers, so that a driver's own #defines (HWY_EMU_ULP_NOISE) come before the product source.
#pragma once
#include <cstring>
#include <type_traits>
#include <vector>

namespace emu_straight {
using hwy::StepParams;

// the packed word of one vehicle <-> the fields of hwy_state (emu_engine.cpp has the intersection scenario's pair)
inline int32_t pack_hwy(const hwy_state &h, size_t k, int slot) {
  return hwy::pack_word(h.lane[k], h.target_lane[k], h.speed_index[k], h.flags[k], slot);
}
inline void unpack_hwy(int32_t w, hwy_state &h, size_t k) {
  h.lane[k] = hwy::word_lane(w); h.target_lane[k] = hwy::word_target(w); h.speed_index[k] = hwy::word_speed_index(w);
  h.flags[k] = hwy::word_flags(w);
  if (!(h.flags[k] & HWY_F_HAS_IMPACT)) h.impact_x[k] = h.impact_y[k] = 0.0;  // as hwy_get_state does
}
// the device image of the state: 9 f64 planes [field][E][N] + the packed words (pitch == N)
struct HostImage {
  int E, N;
  void (*unpack)(int32_t, hwy_state &, size_t);
  std::vector<double> f64;
  std::vector<int32_t> packed;
  HostImage(const hwy_config &c, const hwy_state &h, int32_t (*pack)(const hwy_state &, size_t, int) = pack_hwy,
            void (*unpack_)(int32_t, hwy_state &, size_t) = unpack_hwy) : E(c.num_envs), N(c.num_vehicles), unpack(unpack_) {
    const size_t plane = (size_t)E * N;
    f64.resize(plane * 9);
    packed.resize(plane);
    const double *fields[9] = {h.x, h.y, h.heading, h.speed, h.timer, h.target_speed, h.delta, h.impact_x, h.impact_y};
    for (int f = 0; f < 9; ++f) std::memcpy(&f64[f * plane], fields[f], plane * sizeof(double));
    for (size_t k = 0; k < plane; ++k) packed[k] = pack(h, k, (int)(k % N));
  }
  void store(hwy_state &h) const {
    const size_t plane = (size_t)E * N;
    double *fields[9] = {h.x, h.y, h.heading, h.speed, h.timer, h.target_speed, h.delta, h.impact_x, h.impact_y};
    for (int f = 0; f < 9; ++f) std::memcpy(fields[f], &f64[f * plane], plane * sizeof(double));
    for (size_t k = 0; k < plane; ++k) unpack(packed[k], h, k);
  }
};

// the reset parameters every driver call carries (hwy_set_autoreset / hwy_reset)
struct ResetArgs {
  uint64_t base_seed;
  double ego_spacing, vehicles_density;
  int initial_lane_id;
};
// StepParams from hwy_config, the image and the reset parameters (zeroes everything else of p)
inline void fill_step_params(const hwy_config *cfg, HostImage &img, hwy_state *st, uint8_t *done, uint32_t *episode, const ResetArgs &ra,
                             StepParams &p) {
  static std::vector<int32_t> grid_ws;  // the OccupancyGrid workspace hwy_engine.hip allocates for every family
  hwy::params_from_config(*cfg, cfg->num_vehicles, p);
  hwy::bind_planes(img.f64.data(), (size_t)cfg->num_envs * cfg->num_vehicles, p.st);
  p.st.packed = img.packed.data();
  p.st.time = st->time;
  p.st.done = done;
  p.st.episode = episode;
  p.rp = hwy::default_reset_params(*cfg);
  hwy::set_reset_args(p.rp, ra.ego_spacing, ra.vehicles_density, ra.initial_lane_id);
  p.rp.base_seed = ra.base_seed;
  grid_ws.assign(hwy::grid_ws_len(*cfg), 0);
  p.grid_ws = grid_ws.empty() ? nullptr : grid_ws.data();
}

// the emulation's backend of the launch layer (hwy_launch_family.h): workgroups run one after the other on the CPU, nothing is
// resident, and the waves-per-EU builds of a kernel are one source -- one of them is compiled
struct EmuBackend {
  template <typename K, typename... A>
  static hipError_t launch(K kernel, int grid, int block, int, const hwy::Launch &, const A &...a) {
    emu::launch(kernel, grid, block, a...);
    return hipSuccess;
  }
  template <typename K> static int resident(K, int, int) { return 0; }
  template <typename Fn> static auto pick_wpe(int, Fn &&fn) { return fn(std::integral_constant<int, 1>{}); }
};
// the Launch hwy_create would resolve from the config; force_block: emu_force_block_kernel
inline hwy::Launch launch_of(const hwy_config &c, bool force_block = false) {
  return {c.num_envs, nullptr, 1, 1, force_block || hwy::force_block_kernel(c), 0, nullptr, nullptr};
}

// The body of every driver's run entry point.  with_family(p, fn): builds the family's kernel argument around p and calls fn on it
// (hwy_engine.hip: with_family).
// mode: 0 = frames only (hwy_step_frames), 1 = full policy step(s) (hwy_step; k_steps > 0: hwy_rollout_device, the action / output
// arrays hold k_steps blocks), 2 = observe only.
template <typename WithFamily>
int run(const hwy_config *cfg, hwy_state *st, HostImage &img, const hwy::Launch &l, WithFamily &&with_family, uint8_t *done,
        uint32_t *episode, int mode, int n_frames, int k_steps, const int32_t *actions, float *obs, double *reward, uint8_t *term,
        uint8_t *trunc, double *speed, uint8_t *crashed, int autoreset, const ResetArgs &ra, const uint16_t *block_env = nullptr) {
  StepParams p;
  fill_step_params(cfg, img, st, done, episode, ra, p);
  p.autoreset = mode == 0 ? 0 : autoreset;
  p.block_env = block_env;
  p.actions = actions; p.obs = obs; p.reward = reward; p.terminated = term; p.truncated = trunc;
  p.info_speed = speed; p.info_crashed = crashed;
  const bool rollout = mode != 2 && k_steps > 0;
  if (mode != 2) {
    p.n_frames = n_frames;
    p.full_step = mode == 1;
  }
  if (rollout) {
    p.k_steps = k_steps;
    p.num_envs = cfg->num_envs;
  }
  hipError_t e = hipSuccess;
  with_family(p, [&](const auto &a) {
    e = mode == 2 ? hwy::select_observe<EmuBackend>(a, l) : hwy::select_step<EmuBackend>(a, l, rollout);
  });
  img.store(*st);
  return e == hipSuccess ? 0 : 1;
}
// the body of every driver's reset entry point
template <typename WithFamily>
int reset(const hwy_config *cfg, hwy_state *st, HostImage &img, const hwy::Launch &l, WithFamily &&with_family, uint8_t *done,
          uint32_t *episode, const uint8_t *mask, const uint64_t *seeds, const ResetArgs &ra, float *obs) {
  StepParams p;
  fill_step_params(cfg, img, st, done, episode, ra, p);
  p.reset_mask = mask;
  p.reset_seeds = seeds;
  p.obs = obs;
  hipError_t e = hipSuccess;
  with_family(p, [&](const auto &a) { e = hwy::select_reset<EmuBackend>(a, l); });
  img.store(*st);
  return e == hipSuccess ? 0 : 1;
}
}  // namespace emu_straight
