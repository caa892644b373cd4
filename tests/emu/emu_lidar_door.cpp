// emu_lidar_door.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the Lidar door's kernel of the product source
// (highwayenv_amd/csrc/hwy_lidar_door.h: hwy_lidar_any_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a state, with
// the product's validation (lidar_door_validate), arguments (lidar_door_params), launch rule (hwy_launch_units.h:
// select_lidar_door) and SEQUENCE (lidar_door_rollout_sequence: the template hwy_engine.hip runs).  The step launch lives in the
// simulation's emulator libraries and is called back into tests/emu/emu_lidar_door.py, as the TimeToCollision unit calls back its step.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_lidar_door.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

static std::string g_error;

namespace {
// a backend that launches nothing and records what a rule asked for
struct Dry {
  template <typename K_, typename A>
  static hipError_t launch_plain(K_, int grid, int block, int lds, hipStream_t, const A &) { g = grid; b = block; l = lds; return hipSuccess; }
  static inline int g = 0, b = 0, l = 0;
};

int observe(const hwy_config &c, const hwy_state &st, const hwy_lidar_params &lp, float *obs) {
  const int N = c.num_vehicles;
  std::vector<int32_t> packed((size_t)c.num_envs * N);
  const bool ix = c.scenario == HWY_SCENARIO_INTERSECTION;  // the engine's own word of each family
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = ix ? hwy::ix_pack_word(st.lane[k], st.target_lane[k], st.speed_index[k], st.flags[k])
                   : hwy::pack_word(st.lane[k], st.target_lane[k], st.speed_index[k], st.flags[k], (int)(k % N));
  const hwy::LidarDoorParams p = hwy::lidar_door_params(c, lp, st.x, st.y, st.heading, st.speed, packed.data(), N, obs);
  return emu::launch_status(hwy::select_lidar_door<emu::PlainBackend>(p, lp.normalize != 0, c.num_envs * c.num_agents, nullptr));
}
}  // namespace

extern "C" {

size_t emu_lidar_door_config_size(void) { return sizeof(hwy_config); }
size_t emu_lidar_door_params_size(void) { return sizeof(hwy_lidar_params); }
int emu_lidar_door_lds_bytes(void) { return hwy::LIDAR_PLANES * 64 * (int)sizeof(double) + 64 * (int)sizeof(int32_t); }  // what the source declares
const char *emu_lidar_door_last_error(void) { return g_error.c_str(); }

// what the entry points answer for (config, params, was the engine reset, is it the K-step door) before any launch
int emu_lidar_door_validate(const hwy_config *cfg, const hwy_lidar_params *lp, int has_state, int rollout) {
  const char *why = "";
  const int rc = hwy::lidar_door_validate(*cfg, lp, has_state != 0, rollout != 0, &why);
  g_error = why;
  return rc;
}

// The launch behind a passed emu_lidar_door_validate, on the state `st` ([E][N] planes, pitch == N): obs f32 [E][A][cells][2].
int emu_lidar_door_launch(const hwy_config *cfg, const hwy_state *st, const hwy_lidar_params *lp, float *obs) {
  g_error = "the launch rule refused the arguments";
  return observe(*cfg, *st, *lp, obs);
}

// what the launch rule answers for a shape without running the kernel: out = {status (0 / -2), grid, block, dynamic LDS}
int emu_lidar_door_rules(int32_t cells, int32_t N, int32_t pitch, int32_t A, int32_t rows, int32_t scenario, int with_arrays, int *out) {
  static double f64[4];
  static int32_t i32[4];
  static float f32[4];
  hwy::LidarDoorParams p;
  memset(&p, 0, sizeof p);
  p.cells = cells; p.N = N; p.pitch = pitch; p.A = A; p.scenario = scenario; p.max_range = 60.0;
  if (with_arrays) { p.x = f64; p.y = f64; p.heading = f64; p.speed = f64; p.packed = i32; p.obs = f32; }
  Dry::g = Dry::b = Dry::l = 0;
  out[0] = emu::launch_status(hwy::select_lidar_door<Dry>(p, true, rows, nullptr));
  out[1] = Dry::g; out[2] = Dry::b; out[3] = Dry::l;
  return 0;
}

// the step launch of another emulator library: 0 or a status
typedef int (*emu_lidar_door_callback1)(int);

// hwy_rollout_lidar_device on host arrays: obs f32 [K][E][A][cells][2]; `step`(k): the step launch on block k of the other planes.
int emu_lidar_door_rollout(const hwy_config *cfg, hwy_state *st, const hwy_lidar_params *lp, int32_t k_steps, float *obs,
                           emu_lidar_door_callback1 step) {
  struct Ops {
    const hwy_config *cfg;
    hwy_state *st;
    const hwy_lidar_params *lp;
    float *obs;
    emu_lidar_door_callback1 step_;
    int step(int32_t k) { return step_(k); }
    int observe(int32_t k) {
      return ::observe(*cfg, *st, *lp, obs + (size_t)k * cfg->num_envs * cfg->num_agents * hwy::lidar_door_len(*lp));
    }
  } ops{cfg, st, lp, obs, step};
  g_error = "a launch rule refused the arguments";
  return hwy::lidar_door_rollout_sequence(ops, k_steps);
}
}
