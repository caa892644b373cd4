// hwy_kernels_direct.hip -- gfx950 translation unit of direct ego control (hwy_config.ego_control == HWY_EGO_DIRECT, the
// reference's DiscreteAction): instantiates the DirectEgo policy of the one-wavefront kernel (hwy_wave.h: hwy_step_wave_direct_kernel
// / hwy_rollout_wave_direct_kernel, N <= 64) and of the workgroup kernel (hwy_device.h: hwy_step_direct_kernel /
// hwy_rollout_direct_kernel / hwy_reset_direct_kernel) with IDM traffic; their launch functions are hwy_launch_family.h's.  Its own
// translation unit so that every kernel of hwy_kernels.hip and hwy_kernels_linear.hip keeps its code and its register allocation.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_launch_family.h"

namespace hwy {

struct DirectFamily {
  using Params = DirectParams;
  static const StepParams &step_params(const Params &a) { return a.s; }
  template <int WPE, bool FULL_SCAN> static auto step_wave() { return hwy_step_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int WPE, bool FULL_SCAN> static auto rollout_wave() { return hwy_rollout_wave_direct_kernel<WPE, FULL_SCAN>; }
  template <int NW, int WPE> static auto step_block() { return hwy_step_direct_kernel<NW, WPE>; }
  template <int NW, int WPE> static auto rollout_block() { return hwy_rollout_direct_kernel<NW, WPE>; }
  template <int NW> static auto reset_block() { return hwy_reset_direct_kernel<NW>; }
};
using Direct = FamilyLaunch<DirectFamily>;

hipError_t launch_step(const DirectParams &a, const Launch &l) { return Direct::step(a, l, false); }
hipError_t launch_rollout(const DirectParams &a, const Launch &l) { return Direct::step(a, l, true); }
hipError_t launch_reset(const DirectParams &a, const Launch &l) { return Direct::reset(a, l); }
int step_resident_blocks(const DirectParams &a, const Launch &l) { return Direct::resident_blocks(a, l); }

}  // namespace hwy
