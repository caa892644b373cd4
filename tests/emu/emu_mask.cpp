// emu_mask.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the action-mask kernel of the product source (highwayenv_amd/csrc/hwy_mask.h:
// hwy_mask_kernel) on the CPU through hip_emu.h, on the host SoA arrays of a state, with the validation (mask_validate) and the
// launch shape that hwy_engine.hip / hwy_kernels_mask.hip use.  The simulation itself is the family's own driver's:
// tests/emu/emu_mask.py runs it and then this, the way the engine launches the kernel on its stream.
#include "hip_emu.h"

#include <string>
#include <vector>

#include "../../highwayenv_amd/csrc/hwy_mask.h"

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
// the mask of the state `st` ([E][N] planes, pitch == N) -> u8 [E][A][n_ids]
int emu_action_mask(const hwy_config *cfg, const hwy_state *st, uint8_t *mask) {
  if (const int rc = emu_mask_validate(cfg)) return rc;
  if (!mask) { g_mask_error = "mask must be non-NULL"; return HWY_ERR_INVALID_ARG; }
  const int E = cfg->num_envs, N = cfg->num_vehicles;
  std::vector<int32_t> packed((size_t)E * N);
  const bool ix = cfg->scenario == HWY_SCENARIO_INTERSECTION;  // the engine's own word of each family
  for (size_t k = 0; k < packed.size(); ++k)
    packed[k] = ix ? hwy::ix_pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k])
                   : hwy::pack_word(st->lane[k], st->target_lane[k], st->speed_index[k], st->flags[k], (int)(k % N));
  const hwy::MaskParams p = hwy::mask_params(*cfg, st->x, st->y, packed.data(), N, mask);
  const int blocks = (p.rows + HWY_MASK_BLOCK - 1) / HWY_MASK_BLOCK;
  emu::launch([](const hwy::MaskParams &a) { hwy::hwy_mask_kernel<HWY_MASK_BLOCK>(a); }, blocks, HWY_MASK_BLOCK, p);
  return HWY_OK;
}
}
