// emu_mask.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the action-mask kernel of the product source (highwayenv_amd/csrc/hwy_mask.h:
// hwy_mask_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a state, with the product's validation (mask_validate)
// and launch rule (hwy_launch_units.h: select_mask).  The simulation itself is the family's own driver's: tests/emu/emu.py runs it
// and then this, the way the engine launches the kernel on its stream.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_mask.h"
#include "../../highwayenv_amd/csrc/hwy_launch_units.h"

static std::string g_mask_error;

extern "C" {

size_t emu_mask_config_size(void) { return sizeof(hwy_config); }
const char *emu_mask_last_error(void) { return g_mask_error.c_str(); }
int emu_mask_num_ids(const hwy_config *cfg) { return hwy::mask_num_ids(*cfg); }

// what the entry points answer for a config before any launch
int emu_mask_validate(const hwy_config *cfg) {
  const char *why = "";
  const int rc = hwy::mask_validate(*cfg, &why);
  g_mask_error = why;
  return rc;
}
// The launch behind a passed emu_mask_validate: the mask of the state `st` ([E][N] planes read at `pitch`, the engine's N) -> u8
// [E][A][n_ids]
int emu_mask_launch(const hwy_config *cfg, const hwy_state *st, int pitch, uint8_t *mask) {
  const int E = cfg->num_envs, N = cfg->num_vehicles;
  std::vector<int32_t> packed((size_t)E * N);
  const bool ix = cfg->scenario == HWY_SCENARIO_INTERSECTION;  // the engine's own word of each family
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = ix ? hwy::ix_pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k])
                   : hwy::pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k], (int)(k % N));
  const hwy::MaskParams p = hwy::mask_params(*cfg, st->x, st->y, packed.data(), pitch, mask);
  g_mask_error = "the launch rule refused the arguments";
  return emu::launch_status(hwy::select_mask<emu::PlainBackend>(p, nullptr));
}
}
