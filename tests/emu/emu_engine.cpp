// emu_engine.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's kernel source (highwayenv_amd/csrc/hwy_device.h, hwy_wave.h,
// hwy_wave2.h, hwy_net.h, hwy_ix.h) on the CPU through hip_emu.h, on host SoA arrays: IDM with meta-actions on every scenario.  The
// driver is emu_straight.h's; the arguments and the choice of a kernel are the product's own (hwy_params.h, hwy_launch_rules.h).
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
#include "../../highwayenv_amd/csrc/hwy_launch_rules.h"

#include "emu_straight.h"

using emu_straight::HostImage;
using emu_straight::ResetArgs;
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

bool g_force_block = false;  // emu_force_block_kernel: Launch::force_block_kernel whatever the config says
int g_k_steps = 0;           // emu_set_rollout: > 0: the next full step is a multi-step launch (hwy_rollout_device)
// hwy_set_block_order: environment of workgroup b in the one-wavefront step kernel (nullptr: b)
const uint16_t *g_block_env = nullptr;
// intersection scenario, next-episode pre-warming: shadow planes owned by the Python side (emu_set_shadow)
double *g_shadow_f64 = nullptr;
int32_t *g_shadow_packed = nullptr, *g_shadow_meta = nullptr;
long long *g_shadow_route = nullptr;

// hwy_engine.hip: with_family / fill_ix on the host arrays of the call (pitch == N)
auto scenario_family(const hwy_config *cfg, hwy_state *st) {
  return [=](const StepParams &p, auto &&fn) {
    if (cfg->scenario == HWY_SCENARIO_INTERSECTION) {
      hwy::IxParams ip;
      hwy::ix_params_from_config(*cfg, p, ip);
      ip.lanes = cfg->gnet;
      ip.route = (long long *)st->route;
      ip.road_steps = st->road_steps;
      if (g_shadow_meta && !(cfg->flags & HWY_C_HOST_TRAFFIC)) {
        hwy::bind_planes(g_shadow_f64, (size_t)cfg->num_envs * p.N, ip.shadow);
        ip.shadow.packed = g_shadow_packed;
        ip.shadow_route = g_shadow_route;
        ip.shadow_meta = g_shadow_meta;
      }
      fn(ip);
    } else if (cfg->scenario != HWY_SCENARIO_HIGHWAY) {
      hwy::NetParams np;
      hwy::net_params_from_config(*cfg, p, np);
      fn(np);
    } else {
      fn(p);
    }
  };
}
}  // namespace

extern "C" {

size_t emu_config_size(void) { return sizeof(hwy_config); }
// k > 0: emu_run(mode 1) runs k policy steps in one launch; the action / output arrays hold k blocks
void emu_set_rollout(int k) { g_k_steps = k; }
int emu_has_rollout_kernel(const hwy_config *cfg) {
  (void)cfg;
  return 1;  // every step kernel has a multi-step form
}

// mode: emu_straight::run
int emu_run(const hwy_config *cfg, hwy_state *st, uint8_t *done, uint32_t *episode, int mode, int n_frames,
            const int32_t *actions, float *obs, double *reward, uint8_t *term, uint8_t *trunc, double *speed,
            uint8_t *crashed, int autoreset, uint64_t base_seed, double ego_spacing, double vehicles_density,
            int initial_lane_id) {
  HostImage img = image_of(*cfg, *st);
  return emu_straight::run(cfg, st, img, emu_straight::launch_of(*cfg, g_force_block), scenario_family(cfg, st), done, episode, mode,
                           n_frames, g_k_steps, actions, obs, reward, term, trunc, speed, crashed, autoreset,
                           ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, g_block_env);
}

int emu_reset(const hwy_config *cfg, hwy_state *st, uint8_t *done, uint32_t *episode, const uint8_t *mask,
              const uint64_t *seeds, uint64_t base_seed, double ego_spacing, double vehicles_density,
              int initial_lane_id, float *obs) {
  HostImage img = image_of(*cfg, *st);
  return emu_straight::reset(cfg, st, img, emu_straight::launch_of(*cfg, g_force_block), scenario_family(cfg, st), done, episode, mask,
                             seeds, ResetArgs{base_seed, ego_spacing, vehicles_density, initial_lane_id}, obs);
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
