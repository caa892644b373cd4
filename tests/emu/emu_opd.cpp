// emu_opd.cpp -- TEST INFRASTRUCTURE ONLY.  Runs a plan of the optimistic planner on the CPU through hip_emu.h: the product's
// validation (opd_validate), arguments (opd_params), launch rule (hwy_launch_units.h: select_opd -- masked or not) and SEQUENCE
// (highwayenv_amd/csrc/hwy_opd.h: opd_expand, the template hwy_opd_plan_device enqueues on the device), with the tree kernels and the
// forks (emu_fork.h: hwy_fork_kernel in its device form) run here, inside the one call that holds the schedule, and the work engine's
// mask and step -- which live in other emulator libraries -- called back into tests/emu/emu.py.
#include "hip_emu.h"

#include <string>

#include "../../highwayenv_amd/csrc/hwy_opd.h"
#include "emu_fork.h"

static std::string g_error;

extern "C" {

size_t emu_opd_config_size(void) { return sizeof(hwy_config); }
size_t emu_opd_params_size(void) { return sizeof(hwy_opd_params); }
size_t emu_opd_tree_size(void) { return sizeof(hwy::OpdTree) + sizeof(hwy::OpdPlan); }
int emu_opd_max_nodes(void) { return HWY_OPD_MAX_NODES; }
const char *emu_opd_last_error(void) { return g_error.c_str(); }

// what hwy_opd_plan_device answers for three configs and the parameters before any launch
int emu_opd_validate(const hwy_config *src, const hwy_config *tree, const hwy_config *work, const hwy_opd_params *params, int has_action) {
  const char *why = "";
  const int rc = hwy::opd_validate(*src, *tree, *work, params, has_action != 0, &why);
  g_error = why;
  return rc;
}

// the work engine's mask into t->child_mask / its step with t->actions, outputs to reward | terminated | truncated: 0 or a status
typedef int (*emu_opd_callback)(void);

// The launches behind a passed emu_opd_validate: hwy_opd_plan_device on the host arrays of three engines and of the planner.
int emu_opd_plan(const emu_engine_view *src, const emu_engine_view *tree, const emu_engine_view *work, const hwy_opd_params *params,
                 const hwy::OpdTree *t, const double *reward, const uint8_t *terminated, const uint8_t *truncated, const hwy::OpdPlan *out,
                 emu_opd_callback mask, emu_opd_callback step) {
  struct Ops {
    const emu_engine_view *eng[3];  // by hwy::OpdEngine
    emu_opd_callback mask_, step_;
    int after(int, int) { return HWY_OK; }  // (no streams: every operation is over when it returns)
    int kernel(const hwy::OpdParams &p) { return emu::launch_status(hwy::select_opd<emu::PlainBackend>(p, nullptr)); }
    int fork(int dst, int src, int32_t branches, const int32_t *src_env) {
      const char *why = "";
      if (const int rc = hwy::fork_validate(*eng[dst]->cfg, *eng[src]->cfg, false, branches, src_env != nullptr, &why)) { g_error = why; return rc; }
      return emu_fork::fork(*eng[dst], *eng[src], branches, src_env);
    }
    int mask() { return mask_(); }
    int step(const int32_t *) { return step_(); }
  };
  g_error = "a launch rule refused the arguments";
  return hwy::opd_expand(hwy::opd_params(*params, src->cfg->num_envs, *t, reward, terminated, truncated, *out), Ops{{src, tree, work}, mask, step});
}

// The sequence opd_expand runs for n action ids, X expansions, masked or not, as text: one word per operation, in order.
int emu_opd_sequence(int32_t n, int32_t X, int masked, char *buf, int len) {
  static const char *who[3] = {"src", "tree", "work"};
  struct Ops {
    std::string text;
    hwy::OpdParams q;
    int after(int waiter, int signaler) { text += std::string("after(") + who[waiter] + "," + who[signaler] + ") "; return 0; }
    int kernel(const hwy::OpdParams &p) { text += "kernel(" + std::to_string(p.x) + ") "; return 0; }
    int fork(int dst, int src, int32_t branches, const int32_t *src_env) {
      const char *idx = !src_env ? "none" : src_env == q.root_src ? "root" : src_env == q.gather_src ? "gather" : src_env == q.scatter_src ? "scatter" : "?";
      text += std::string("fork(") + who[dst] + "," + who[src] + "," + std::to_string(branches) + "," + idx + ") ";
      return 0;
    }
    int mask() { text += "mask "; return 0; }
    int step(const int32_t *actions) { text += actions == q.actions ? "step " : "step(?) "; return 0; }
  };
  int32_t idx[4];  // (only their addresses are used)
  uint8_t bytes[2];
  const hwy_opd_params params = {X * n, n, 1 + X * n, masked ? HWY_OPD_MASKED : 0, 0.5, 2.0};
  const hwy::OpdTree t = {nullptr, nullptr, nullptr, nullptr, nullptr, &idx[0], &idx[1], &idx[2], &idx[3], &bytes[0], &bytes[1]};
  Ops ops{"", hwy::opd_params(params, 2, t, nullptr, nullptr, nullptr, hwy::OpdPlan{})};
  const int rc = hwy::opd_expand(ops.q, ops);
  if (len > 0) { strncpy(buf, ops.text.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
  return rc;
}
}
