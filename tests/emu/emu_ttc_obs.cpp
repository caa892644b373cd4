// emu_ttc_obs.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the TimeToCollision observation kernel of the product source
// (highwayenv_amd/csrc/hwy_collision_obs.h: hwy_collision_obs_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a
// state, with the product's validation (ttc_obs_validate), arguments (collision_obs_params), launch rule (hwy_launch_units.h:
// select_collision_obs) and SEQUENCES (ttc_obs_same_step_sequence, ttc_obs_rollout_sequence: the templates hwy_engine.hip runs).
// The observe launch and the stash (hwy_same_step.h: hwy_final_kernel, select_final) run here; the step launch, the re-spawn and
// the mask kernel live in other emulator libraries and are called back into tests/emu/emu_ttc_obs.py, as the OPD unit calls back
// its step.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_collision_obs.h"
#include "../../highwayenv_amd/csrc/hwy_same_step.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

static std::string g_error;

namespace {
// a backend that launches nothing and records what a rule asked for
struct Dry {
  template <typename K_, typename A>
  static hipError_t launch_plain(K_, int grid, int block, int lds, hipStream_t, const A &) { g = grid; b = block; l = lds; return hipSuccess; }
  static inline int g = 0, b = 0, l = 0;
};

std::vector<int32_t> packed_words(const hwy_config &c, const hwy_state &st) {
  std::vector<int32_t> packed((size_t)c.num_envs * c.num_vehicles);
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = hwy::pack_word(st.lane[k], st.target_lane[k], st.speed_index[k], st.flags[k], (int)(k % c.num_vehicles));
  return packed;
}

int observe(const hwy_config &c, const hwy_state &st, const hwy_ttc_params &tp, float *obs) {
  const std::vector<int32_t> packed = packed_words(c, st);
  const hwy::CollisionObsParams p = hwy::collision_obs_params(c, tp, st.x, st.heading, st.speed, packed.data(), c.num_vehicles, obs);
  return emu::launch_status(hwy::select_collision_obs<emu::PlainBackend>(p, c.num_envs * c.num_agents, nullptr));
}
}  // namespace

extern "C" {

size_t emu_ttc_obs_config_size(void) { return sizeof(hwy_config); }
size_t emu_ttc_obs_params_size(void) { return sizeof(hwy_ttc_params); }
int emu_ttc_obs_lds_bytes(void) { return HWY_COLLISION_OBS_CELLS * (int)sizeof(int32_t); }  // what the source declares
const char *emu_ttc_obs_last_error(void) { return g_error.c_str(); }

// what the entry points answer for (config, params) before any launch
int emu_ttc_obs_validate(const hwy_config *cfg, const hwy_ttc_params *tp) {
  const char *why = "";
  const int rc = hwy::ttc_obs_validate(*cfg, tp, &why);
  g_error = why;
  return rc;
}
// ... and hwy_step_same_step_ttc_device (the mask pointers' own check is the mask unit's)
int emu_ttc_obs_same_step_validate(const hwy_config *cfg, const hwy_ttc_params *tp, int autoreset, int has_final_obs, int has_final_mask) {
  const char *why = "";
  int rc = hwy::ttc_obs_validate(*cfg, tp, &why);
  if (rc == HWY_OK) rc = hwy::same_step_validate(*cfg, autoreset != 0, has_final_obs != 0, has_final_mask != 0, &why);
  g_error = why;
  return rc;
}

// The launch behind a passed emu_ttc_obs_validate, on the state `st` ([E][N] planes, pitch == N): obs f32 [E][A][3][3][T].
int emu_ttc_obs_launch(const hwy_config *cfg, const hwy_state *st, const hwy_ttc_params *tp, float *obs) {
  g_error = "the launch rule refused the arguments";
  return observe(*cfg, *st, *tp, obs);
}

// what the launch rule answers for a shape without running the kernel: out = {status (0 / -2), grid, block, dynamic LDS}
int emu_ttc_obs_rules(int32_t V, int32_t L, int32_t T, int32_t N, int32_t pitch, int32_t A, int32_t rows, int with_arrays, int *out) {
  static double f64[4];
  static int32_t i32[4];
  static float f32[4];
  hwy::CollisionObsParams p;
  memset(&p, 0, sizeof p);
  p.V = V; p.L = L; p.T = T; p.N = N; p.pitch = pitch; p.A = A;
  if (with_arrays) { p.x = f64; p.heading = f64; p.speed = f64; p.packed = i32; p.obs = f32; }
  Dry::g = Dry::b = Dry::l = 0;
  out[0] = emu::launch_status(hwy::select_collision_obs<Dry>(p, rows, nullptr));
  out[1] = Dry::g; out[2] = Dry::b; out[3] = Dry::l;
  return 0;
}

// the launches of other emulator libraries: 0 or a status
typedef int (*emu_ttc_obs_callback)(void);
typedef int (*emu_ttc_obs_callback1)(int);

// The launches behind a passed emu_ttc_obs_same_step_validate: hwy_step_same_step_ttc_device on host arrays.  `step`: the family's
// step launch with auto-reset on, which fills reward / terminated / truncated / speed / crashed and leaves the state in `st`;
// `respawn`: the family's re-spawn kernel; `mask`(final): the mask kernel into the call's mask planes.
int emu_ttc_obs_same_step(const hwy_config *cfg, hwy_state *st, const hwy_ttc_params *tp, const uint8_t *done, float *obs, float *final_obs,
                          const double *speed, double *final_speed, const uint8_t *crashed, uint8_t *final_crashed, uint8_t *final_mask,
                          int final_action_mask, int action_mask, emu_ttc_obs_callback step, emu_ttc_obs_callback1 mask,
                          emu_ttc_obs_callback respawn) {
  struct Ops {
    const hwy_config *cfg;
    hwy_state *st;
    const hwy_ttc_params *tp;
    const uint8_t *done;
    float *obs, *final_obs;
    const double *speed;
    double *final_speed;
    const uint8_t *crashed;
    uint8_t *final_crashed, *final_mask;
    emu_ttc_obs_callback step_, respawn_;
    emu_ttc_obs_callback1 mask_;
    int step() { return step_(); }
    int mask(bool final) { return mask_(final ? 1 : 0); }
    int observe() { return ::observe(*cfg, *st, *tp, obs); }
    int stash() {
      const hwy::FinalParams fp = hwy::final_params(*cfg, hwy::collision_obs_len(*tp), done, final_mask, obs, final_obs, speed, final_speed,
                                                    crashed, final_crashed);
      return emu::launch_status(hwy::select_final<emu::PlainBackend>(fp, nullptr));
    }
    int respawn() { return respawn_(); }
  } ops{cfg, st, tp, done, obs, final_obs, speed, final_speed, crashed, final_crashed, final_mask, step, respawn, mask};
  g_error = "a launch rule refused the arguments";
  return hwy::ttc_obs_same_step_sequence(ops, final_action_mask != 0, action_mask != 0);
}

// hwy_rollout_ttc_device on host arrays: obs f32 [K][E][A][3][3][T]; `step`(k): the step launch on block k of the other planes.
int emu_ttc_obs_rollout(const hwy_config *cfg, hwy_state *st, const hwy_ttc_params *tp, int32_t k_steps, float *obs, emu_ttc_obs_callback1 step) {
  struct Ops {
    const hwy_config *cfg;
    hwy_state *st;
    const hwy_ttc_params *tp;
    float *obs;
    emu_ttc_obs_callback1 step_;
    int step(int32_t k) { return step_(k); }
    int observe(int32_t k) {
      return ::observe(*cfg, *st, *tp, obs + (size_t)k * cfg->num_envs * cfg->num_agents * hwy::collision_obs_len(*tp));
    }
  } ops{cfg, st, tp, obs, step};
  g_error = "a launch rule refused the arguments";
  return hwy::ttc_obs_rollout_sequence(ops, k_steps);
}

// The two sequences as text: one word per operation, in order.
int emu_ttc_obs_sequence(int final_action_mask, int action_mask, int32_t k_steps, char *buf, int len) {
  struct Ops {
    std::string text;
    int step() { text += "step "; return 0; }
    int mask(bool final) { text += final ? "mask(final) " : "mask "; return 0; }
    int observe() { text += "observe "; return 0; }
    int stash() { text += "stash "; return 0; }
    int respawn() { text += "respawn "; return 0; }
    int step(int32_t k) { text += "step(" + std::to_string(k) + ") "; return 0; }
    int observe(int32_t k) { text += "observe(" + std::to_string(k) + ") "; return 0; }
  } ops;
  const int rc = k_steps > 0 ? hwy::ttc_obs_rollout_sequence(ops, k_steps)
                             : hwy::ttc_obs_same_step_sequence(ops, final_action_mask != 0, action_mask != 0);
  if (len > 0) { strncpy(buf, ops.text.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
  return rc;
}
}
