// emu_engine.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's kernel source
// (highwayenv_amd/csrc/hwy_device.h) on the CPU through hip_emu.h, on host SoA arrays.
#include "hip_emu.h"

#include <cstring>
#include <vector>

#ifdef HWY_EMU_ULP_NOISE
// Sensitivity probe: perturb every libm result by +-1 ulp (pseudo-randomly) to mimic a different
// libm (ocml vs glibc vs numpy) and see which discrete decisions of the simulation can flip.
namespace emu {
inline double noisy(double v) {
  static thread_local uint64_t s = 0x9E3779B97F4A7C15ull;
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  const unsigned r = (unsigned)(s >> 33) % 3;  // 0: keep, 1: up, 2: down
  return r == 0 ? v : nextafter(v, r == 1 ? INFINITY : -INFINITY);
}
}  // namespace emu
#define cos(x) emu::noisy(cos(x))
#define sin(x) emu::noisy(sin(x))
#define tan(x) emu::noisy(tan(x))
#define atan(x) emu::noisy(atan(x))
#define asin(x) emu::noisy(asin(x))
#define pow(x, y) emu::noisy(pow(x, y))
#endif
#include "../../highwayenv_amd/csrc/hwy_device.h"
#include "../../highwayenv_amd/csrc/hwy_wave.h"
#include "../../highwayenv_amd/csrc/hwy_wave2.h"
#include "../../highwayenv_amd/csrc/hwy_net.h"
#include "../../highwayenv_amd/csrc/hwy_ix.h"
#include "../../highwayenv_amd/csrc/hwy_params.h"

#include "emu_straight.h"

using emu_straight::fill_step_params;
using emu_straight::HostImage;
using emu_straight::ResetArgs;
using emu_straight::Which;
using emu_straight::OBSERVE; using emu_straight::RESET; using emu_straight::ROLLOUT; using emu_straight::STEP;
using hwy::StepParams;

namespace {
// the intersection scenario's packed word (hwy_ix.h)
int32_t pack_ix(const hwy_state &h, size_t k, int) { return hwy::ix_pack_word(h.lane[k], h.target_lane[k], h.speed_index[k], h.flags[k]); }
void unpack_ix(int32_t w, hwy_state &h, size_t k) {
  h.lane[k] = hwy::ix_word_lane(w); h.target_lane[k] = hwy::ix_word_target(w); h.speed_index[k] = hwy::ix_word_speed_index(w); h.flags[k] = hwy::ix_word_flags(w);
}
HostImage image_of(const hwy_config &c, const hwy_state &h) {
  return c.scenario == HWY_SCENARIO_INTERSECTION ? HostImage(c, h, pack_ix, unpack_ix) : HostImage(c, h);
}
struct IdmEmu {
  using Params = StepParams;
  static const StepParams &step_params(const Params &a) { return a; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy::hwy_step_wave_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy::hwy_rollout_wave_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy::hwy_step_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy::hwy_rollout_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy::hwy_reset_kernel<NW>; }
};

bool g_force_block = false;
int g_k_steps = 0;  // > 0: the next STEP dispatch of the one-wavefront kernel is a multi-step launch (hwy_rollout_device)
const hwy_config *g_cfg = nullptr;  // config of the call being dispatched (road-network scenarios need the lane table)
hwy_state *g_st = nullptr;          // host state of the call (intersection scenario: route / road_steps planes)
// hwy_set_block_order: environment of workgroup b in the one-wavefront step kernel (nullptr: b)
static const uint16_t *g_block_env = nullptr;
// intersection scenario, next-episode pre-warming: shadow planes owned by the Python side (emu_set_shadow)
double *g_shadow_f64 = nullptr;
int32_t *g_shadow_packed = nullptr, *g_shadow_meta = nullptr;
long long *g_shadow_route = nullptr;
void dispatch(Which which, const StepParams &p, int E) {
  const int nw = (p.N + 63) / 64;
  if (g_cfg && g_cfg->scenario == HWY_SCENARIO_INTERSECTION) {
    hwy::IxParams ip;
    hwy::ix_params_from_config(*g_cfg, p, ip);
    ip.lanes = g_cfg->gnet;
    ip.route = (long long *)g_st->route;  // pitch == N in the emulation
    ip.road_steps = g_st->road_steps;
    int grid = E;
    if (g_shadow_meta && !(g_cfg->flags & HWY_C_HOST_TRAFFIC)) {
      hwy::bind_planes(g_shadow_f64, (size_t)E * p.N, ip.shadow);
      ip.shadow.packed = g_shadow_packed;
      ip.shadow_route = g_shadow_route;
      ip.shadow_meta = g_shadow_meta;
      if (which == STEP && p.autoreset && p.full_step) grid = 2 * E;
    }
    if (which == STEP && g_k_steps > 0) {  // hwy_rollout_device: k steps in one launch, STEP blocks only (same rule as hwy_kernels.hip)
      ip.s.k_steps = g_k_steps;
      ip.s.num_envs = E;
      if (p.N <= 32 && ip.helpers) emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_rollout_kernel<1, 32, 64>(q); }, E, 64, ip);
      else if (p.N <= 32) emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_rollout_kernel<1, 32>(q); }, E, 32, ip);
      else emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_rollout_kernel<1, 64>(q); }, E, 64, ip);
      return;
    }
    if (p.N <= 32 && ip.helpers) {  // same dispatch rule as hwy_kernels.hip
      switch (which) {
        case STEP: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_step_kernel<1, 32, 64>(q); }, grid, 64, ip); break;
        case RESET: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_reset_kernel<1, 32, 64>(q); }, E, 64, ip); break;
        case OBSERVE: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_observe_kernel<1, 32>(q); }, E, 32, ip); break;
      }
    } else if (p.N <= 32) {
      switch (which) {
        case STEP: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_step_kernel<1, 32>(q); }, grid, 32, ip); break;
        case RESET: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_reset_kernel<1, 32>(q); }, E, 32, ip); break;
        case OBSERVE: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_observe_kernel<1, 32>(q); }, E, 32, ip); break;
      }
    } else {
      switch (which) {
        case STEP: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_step_kernel<1, 64>(q); }, grid, 64, ip); break;
        case RESET: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_reset_kernel<1, 64>(q); }, E, 64, ip); break;
        case OBSERVE: emu::launch([](const hwy::IxParams &q) { hwy::hwy_ix_observe_kernel<1, 64>(q); }, E, 64, ip); break;
      }
    }
    return;
  }
  if (g_cfg && g_cfg->scenario != HWY_SCENARIO_HIGHWAY) {  // same dispatch rule as hwy_engine.hip
    hwy::NetParams np;
    hwy::net_params_from_config(*g_cfg, p, np);
    const bool grid = p.obs_type != HWY_OBS_KINEMATICS;
    switch (which) {
      // same dispatch rule as hwy_kernels.hip: the OccupancyGrid observation has its own instantiation
      case STEP: if (g_k_steps > 0) {  // hwy_rollout_device: k steps in one launch
                   np.s.k_steps = g_k_steps;
                   np.s.num_envs = E;
                   if (grid) emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_rollout_kernel<1, true>(q); }, E, 64, np);
                   else emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_rollout_kernel<1>(q); }, E, 64, np);
                 }
                 else if (grid) emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_step_kernel<1, true>(q); }, E, 64, np);
                 else emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_step_kernel<1>(q); }, E, 64, np);
                 break;
      case RESET: if (grid) emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_reset_kernel<1, true>(q); }, E, 64, np);
                  else emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_reset_kernel<1>(q); }, E, 64, np);
                  break;
      case OBSERVE: if (grid) emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_observe_kernel<1, true>(q); }, E, 64, np);
                    else emu::launch([](const hwy::NetParams &q) { hwy::hwy_net_observe_kernel<1>(q); }, E, 64, np);
                    break;
    }
    return;
  }
  if (which == STEP && nw >= 2 && nw <= 4 && p.obs_type == HWY_OBS_KINEMATICS && !g_force_block &&
      (g_cfg->tune_block_kernel == 2 || (g_cfg->tune_block_kernel == 0 && nw == 2))) {
    // same dispatch rule as hwy_kernels.hip (wide_kernel_applies): one wavefront per environment, nw vehicles per thread
#define RUN_WIDE(KV)                                                                                           \
    if (g_k_steps > 0) {                                                                                       \
      StepParams pk = p;                                                                                       \
      pk.k_steps = g_k_steps;                                                                                  \
      pk.num_envs = E;                                                                                         \
      emu::launch([](const StepParams &q) { hwy::hwy_rollout_wide_kernel<KV, 1>(q); }, E, 64, pk);             \
    } else {                                                                                                   \
      emu::launch([](const StepParams &q) { hwy::hwy_step_wide_kernel<KV, 1>(q); }, E, 64, p);                 \
    }
    if (nw == 2) { RUN_WIDE(2) } else if (nw == 3) { RUN_WIDE(3) } else { RUN_WIDE(4) }
#undef RUN_WIDE
    return;
  }
  // the one-wavefront and the workgroup kernels: the straight-road family dispatch
  const bool force_block = g_force_block || g_cfg->tune_block_kernel == 1;
  if (which == STEP && g_k_steps > 0) {
    StepParams pk = p;
    pk.k_steps = g_k_steps;
    pk.num_envs = E;
    emu_straight::dispatch<IdmEmu>(ROLLOUT, pk, E, force_block);
  } else {
    emu_straight::dispatch<IdmEmu>(which, p, E, force_block);
  }
}
}  // namespace

extern "C" {

size_t emu_config_size(void) { return sizeof(hwy_config); }
// k > 0: emu_run(mode 1) on the one-wavefront kernel runs k policy steps in one launch; the action / output arrays hold k blocks
void emu_set_rollout(int k) { g_k_steps = k; }
int emu_has_rollout_kernel(const hwy_config *cfg) {
  (void)cfg;
  return 1;  // every step kernel has a multi-step form
}

// mode: 0 = frames only (hwy_step_frames), 1 = full policy step (hwy_step), 2 = observe only
static std::vector<int32_t> g_grid_ws;
static int32_t *grid_ws_for(const hwy_config *cfg) {
  if (cfg->obs_type != HWY_OBS_OCCUPANCY_GRID) return nullptr;
  g_grid_ws.assign((size_t)cfg->num_envs * cfg->num_agents * 2 * cfg->grid_shape[0] * cfg->grid_shape[1], 0);
  return g_grid_ws.data();
}

int emu_run(const hwy_config *cfg, hwy_state *st, uint8_t *done, uint32_t *episode, int mode, int n_frames,
            const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
            uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
            int initial_lane_id) {
  HostImage img = image_of(*cfg, *st);
  g_cfg = cfg;
  g_st = st;
  StepParams p;
  fill_step_params(cfg, img, st, done, episode, ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, p);
  p.autoreset = autoreset;
  p.grid_ws = grid_ws_for(cfg);
  p.block_env = g_block_env;
  p.actions = actions; p.obs = obs; p.reward = reward; p.terminated = term; p.truncated = trunc;
  p.info_speed = speed; p.info_crashed = crashed;
  if (mode == 2) {
    dispatch(OBSERVE, p, cfg->num_envs);
  } else {
    p.n_frames = n_frames;
    p.full_step = mode == 1;
    if (mode == 0) p.autoreset = 0;
    dispatch(STEP, p, cfg->num_envs);
  }
  img.store(*st);
  return 0;
}

int emu_reset(const hwy_config *cfg, hwy_state *st, uint8_t *done, uint32_t *episode, const uint8_t *mask,
              const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density,
              int initial_lane_id, float *obs) {
  HostImage img = image_of(*cfg, *st);
  g_cfg = cfg;
  g_st = st;
  StepParams p;
  fill_step_params(cfg, img, st, done, episode, ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, p);
  p.reset_mask = mask;
  p.reset_seeds = seeds;
  p.obs = obs;
  p.grid_ws = grid_ws_for(cfg);
  dispatch(RESET, p, cfg->num_envs);
  img.store(*st);
  return 0;
}

void emu_force_block_kernel(int on) { g_force_block = on != 0; }

void emu_set_block_order(const uint16_t *env_of_block) { g_block_env = env_of_block; }

void emu_set_shadow(double *f64, int32_t *packed, long long *route, int32_t *meta) {
  g_shadow_f64 = f64; g_shadow_packed = packed; g_shadow_route = route; g_shadow_meta = meta;
}

void emu_debug_math(int op, const double *in, double *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = hwy::math_probe(op, in[k]);
}

// host-side Philox, for tests of the device spawn rule
void emu_philox_uniform2(uint64_t seed, uint32_t vehicle, uint32_t episode, uint32_t draw, double *u0, double *u1) {
  hwy::philox_uniform2(seed, vehicle, episode, draw, u0, u1);
}
}
