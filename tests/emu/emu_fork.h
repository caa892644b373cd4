// emu_fork.h -- TEST INFRASTRUCTURE ONLY.  The environment fork between the host arrays of two emulated engines, for the two emulator
// libraries that hold hwy_fork_kernel (emu_lookahead.cpp: Engine.fork_from / fork_device; emu_opd.cpp: the forks of a plan).  The
// arguments and the launch are the product's own (hwy_lookahead.h: fork_params; hwy_launch_units.h: select_fork); the four integer
// planes stand where the engine has its packed words (pitch == N).  Include it after hip_emu.h.
#pragma once
#include "../../highwayenv_amd/csrc/hwy_lookahead.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

extern "C" {
// one emulated engine's host arrays (tests/emu/emu.py: EmuEngine._view).  extra: the family's extra planes in the device layout --
// behaviour [HWY_BEHAVIOR_PARAMS][E][N] of a Linear engine, stored controls [2][E][A] of a direct-control engine, NULL otherwise
struct emu_engine_view {
  const hwy_config *cfg;
  hwy_state *st;
  double *extra;
  uint8_t *done;
  uint32_t *episode;
};
}

namespace emu_fork {
inline hwy::ForkView view(const emu_engine_view &e) {
  const hwy_state &s = *e.st;
  return {e.cfg, {s.x, s.y, s.heading, s.speed, s.timer, s.target_speed, s.delta, s.impact_x, s.impact_y}, e.extra,
          {s.lane, s.target_lane, s.speed_index, s.flags}, 4, e.extra, s.time, e.episode, e.done, e.cfg->num_vehicles};
}
// hwy_fork_device behind a passed fork_validate.  src_env: the indices or NULL; the device form does not validate them (an index
// outside the source copies nothing, which the planner's scatter relies on)
inline int fork(const emu_engine_view &dst, const emu_engine_view &src, int32_t branches, const int32_t *src_env) {
  return emu::launch_status(hwy::select_fork<emu::PlainBackend>(hwy::fork_params(view(dst), view(src), branches, src_env), nullptr));
}
}  // namespace emu_fork
