// emu_lidar.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the LidarObservation kernel of the product source
// (highwayenv_amd/csrc/hwy_lidar.h: hwy_lidar_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a state, by the
// product's own launch rule (hwy_launch_units.h: select_lidar).  The simulation itself is the family's own driver's
// (emu_engine.cpp / emu_traffic.cpp / emu_control.cpp): tests/emu/emu.py runs it and then this, the way hwy_engine.hip launches the
// lidar kernel after the step kernel.
#include "hip_emu.h"

#include <vector>

#include "../../highwayenv_amd/csrc/hwy_lidar.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

extern "C" {

size_t emu_lidar_config_size(void) { return sizeof(hwy_config); }

// LidarObservation of the state `st` ([E][N] planes, pitch == N) -> obs f32 [E][A][cells][2]
int emu_lidar_observe(const hwy_config *cfg, const hwy_state *st, float *obs) {
  const int E = cfg->num_envs, N = cfg->num_vehicles;
  std::vector<int32_t> packed((size_t)E * N);
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = hwy::pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k], (int)(k % N));
  const hwy::LidarParams lp = hwy::lidar_params(*cfg, st->x, st->y, st->heading, st->speed, packed.data(), N, obs);
  return emu::launch_status(hwy::select_lidar<emu::PlainBackend>(lp, cfg->lidar_normalize != 0, E * cfg->num_agents, nullptr));
}
}
