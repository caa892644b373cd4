// emu_opd_mask.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the MASKED tree kernel of the optimistic planner (highwayenv_amd/csrc/hwy_opd.h:
// hwy_opd_masked_kernel, which shares opd_tree_step with hwy_opd_kernel) on the CPU through hip_emu.h, on host arrays in the layout
// of hwy::OpdParams with its two tail fields set.  The forks, the validation and the unmasked kernel are tests/emu/emu_opd.cpp's,
// the mask of a leaf tests/emu/emu_mask.cpp's; tests/emu/emu_opd_mask.py launches them behind each other the way
// hwy_opd_plan_device enqueues them.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_opd.h"

static std::string g_error;

extern "C" {

size_t emu_opd_mask_params_size(void) { return sizeof(hwy_opd_params); }
const char *emu_opd_mask_last_error(void) { return g_error.c_str(); }

// launch x of hwy_opd_masked_kernel on host arrays
int emu_opd_masked_kernel(int32_t E, int32_t n, int32_t X, int32_t x, double gamma, double bound, double *ret, double *disc, double *upper0,
                          uint8_t *done, int32_t *expanded_node, const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                          int32_t *gather_src, int32_t *scatter_src, int32_t *root_src, int32_t *actions, int32_t *action, double *value,
                          double *upper, int32_t *sequence, int32_t *expanded, const uint8_t *child_mask, uint8_t *created) {
  hwy::OpdParams p;
  memset(&p, 0, sizeof p);
  p.ret = ret; p.disc = disc; p.upper0 = upper0; p.done = done; p.expanded_node = expanded_node;
  p.reward = reward; p.terminated = terminated; p.truncated = truncated;
  p.gather_src = gather_src; p.scatter_src = scatter_src; p.root_src = root_src; p.actions = actions;
  p.action = action; p.value = value; p.upper = upper; p.sequence = sequence; p.expanded = expanded;
  p.gamma = gamma; p.bound = bound;
  p.x = x; p.X = X; p.n = n; p.M = 1 + X * n; p.E = E;
  p.child_mask = child_mask; p.created = created;
  if (p.M > HWY_OPD_MAX_NODES || x < 0 || x > X || !child_mask || !created) { g_error = "launch outside the kernel's capacity"; return HWY_ERR_INVALID_ARG; }
  emu::launch([](const hwy::OpdParams &a) { hwy::hwy_opd_masked_kernel<HWY_OPD_MAX_NODES>(a); }, E, 64, p);
  return HWY_OK;
}
}
