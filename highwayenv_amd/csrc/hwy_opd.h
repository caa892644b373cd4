// hwy_opd.h -- optimistic planning of deterministic systems (OPD, Hren & Munos 2008) on the device, one tree per environment: the
// budgeted tree search that the reference's scripts/highway_planning.ipynb runs on copy.deepcopy(env) + env.step (its
// DeterministicPlannerAgent with budget = 50, gamma = 0.7), restated exactly in DESIGN.md ("OPD on the device").
//
//   hwy_opd_kernel   one launch per expansion x = 0 .. X (X = budget / n expansions of n action ids each; node 0 is the root,
//                    expansion x creates nodes 1 + x * n + a, so a child always has a higher index than its parent).  Launch x
//                      1. ingests the n children of expansion x - 1 from the work engine's reward / terminated / truncated,
//                      2. backs the tree up: the expansions in reverse order (a node is always expanded after its parent, so
//                         every expanded node is visited after the expanded nodes below it -- the same values as a walk in
//                         reverse creation order), value lower / upper of the expanded node = maximum over its children,
//                      3. x < X: selects the leaf with the largest value upper (ties: the lowest node index) and writes the
//                         index arrays of the gather tree -> work and the scatter work -> tree that hwy_fork_kernel executes
//                         around the work engine's step; a selected leaf that is done makes this expansion void (index -1
//                         everywhere: "copies nothing") -- and, since the tree no longer changes, every later one;
//                         x == X: writes the plan (first action, value, upper, greedy sequence, expansions made).
//                    One 64-wide wavefront per environment, lane == node (or child, or expansion) in passes of 64.  What persists
//                    between launches is per node its path return, discount, upper bound at creation and done mark, and per
//                    expansion the node it expanded; the values are rebuilt from them in LDS by every launch.  Maxima are taken
//                    on score_key (hwy_lookahead.h) with LDS atomic max, the index among the holders of a maximum with LDS atomic
//                    min: neither depends on the order of lanes or passes.  Barriers separate the phases, and no LDS word is
//                    read again after the barrier behind which another lane may rewrite it.  Every loop is bounded by X, n, M.
//
// A child's bounds: t = disc_p * r; lower = ret_p + t; disc = disc_p * gamma; upper = done ? lower : lower + disc * bound -- every
// product and sum a statement of its own (the rule of score_return), so the path return of a node equals what hwy_score_kernel
// computes for its action sequence, bit for bit.
//
// hwy_opd_masked_kernel (hwy_opd_params.flags & HWY_OPD_MASKED) is the same tree step with one rule added: a node's unavailable
// actions -- the action mask of its state, written by hwy_mask.h's kernel on the work engine between the gather and the step -- get
// no child.  The two kernels share the __device__ body opd_tree_step<CAP, MASKED>; see there.
//
// Like hwy_lookahead.h this header includes no HIP runtime.  The launch rule of the two kernels is hwy_launch_units.h's and the
// sequence of launches around them opd_expand's below, for the product and for the CPU emulation (tests/emu/emu_opd.cpp).
#pragma once

#include "hwy_lookahead.h"

namespace hwy {

#define HWY_OPD_MAX_NODES 1024  // nodes of one tree, root included: the capacity of the kernel's LDS staging

struct OpdParams {
  // the tree, [E][M] per node and [E][X] per expansion
  double *ret;          // path return of the node (its lower bound at creation)
  double *disc;         // gamma ** depth
  double *upper0;       // upper bound at creation
  uint8_t *done;        // terminated | truncated
  int32_t *expanded_node;  // [E][X]: the node expansion j expanded, -1 = void
  // the work engine's outputs of the step behind expansion x - 1
  const double *reward;                   // [E * n]
  const uint8_t *terminated, *truncated;  // [E * n]
  // what the forks and the step around this launch read
  int32_t *gather_src;   // [E * n]: tree environment e * M + leaf, or -1
  int32_t *scatter_src;  // [E * M]: work environment e * n + a in the n new slots, -1 elsewhere
  int32_t *root_src;     // [E * M]: e in slot e * M, -1 elsewhere (written by launch 0)
  int32_t *actions;      // [E * n]: j % n (written by launch 0)
  // the plan (launch X)
  int32_t *action;       // [E]
  double *value, *upper; // [E]            (may be null)
  int32_t *sequence;     // [E][X]         (may be null)
  int32_t *expanded;     // [E]            (may be null)
  double gamma, bound;
  int32_t x, X, n, M, E;
  // the masked search (HWY_OPD_MASKED; both null: the unmasked one)
  const uint8_t *child_mask;  // [E * n][n]: the mask kernel's output on the work engine -- row e * n holds the mask of the selected leaf
  uint8_t *created;           // [E][M]: 1 where the node was created (its action was available in its parent's state)
};

// host side: what hwy_opd_plan_device accepts (include/hwy_engine.h).  Shared by hwy_engine.hip and the CPU emulation.
inline int opd_validate(const hwy_config &src, const hwy_config &tree, const hwy_config &work, const hwy_opd_params *params, bool has_action,
                        const char **why) {
  *why = "";
  if (src.scenario != HWY_SCENARIO_HIGHWAY) {
    *why = "OPD plans on the highway scenario only (the merge and intersection scenarios are outside the hot-path scope)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (src.num_agents != 1) {
    *why = "OPD plans for a single agent (joint-action trees are outside the hot-path scope)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (!params) { *why = "params is NULL"; return HWY_ERR_INVALID_ARG; }
  if (params->flags & ~HWY_OPD_MASKED) { *why = "unknown bits in flags"; return HWY_ERR_INVALID_ARG; }
  if ((params->flags & HWY_OPD_MASKED) && src.ego_control != HWY_EGO_META) {
    *why = "the masked search needs a DiscreteMetaAction ego (a DiscreteAction ego has no get_available_actions)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (!has_action) { *why = "action must be non-NULL"; return HWY_ERR_INVALID_ARG; }
  if (!(src.flags & HWY_C_NORMALIZE_REWARD)) { *why = "OPD needs normalize_reward (its bound assumes rewards in [0, 1])"; return HWY_ERR_INVALID_ARG; }
  if (!(params->gamma > 0.0 && params->gamma < 1.0)) { *why = "gamma must be in (0, 1)"; return HWY_ERR_INVALID_ARG; }
  if (!(params->bound > 0.0 && params->bound < 1e300)) { *why = "bound must be 1 / (1 - gamma): positive and finite"; return HWY_ERR_INVALID_ARG; }
  const int n = lookahead_num_ids(src);
  if (params->n_ids != n) { *why = "n_ids is not the size of the engine's action table"; return HWY_ERR_INVALID_ARG; }
  if (params->budget < n) { *why = "budget must be at least n_ids (one expansion)"; return HWY_ERR_INVALID_ARG; }
  const int64_t nodes = 1 + (int64_t)(params->budget / n) * n;
  if (nodes > HWY_OPD_MAX_NODES) { *why = "1 + (budget / n_ids) * n_ids nodes exceed HWY_OPD_MAX_NODES"; return HWY_ERR_INVALID_ARG; }
  if (params->nodes != nodes) { *why = "nodes must be 1 + (budget / n_ids) * n_ids"; return HWY_ERR_INVALID_ARG; }
  if ((int64_t)tree.num_envs != (int64_t)src.num_envs * nodes) { *why = "tree.num_envs must be src.num_envs * nodes"; return HWY_ERR_INVALID_ARG; }
  if ((int64_t)work.num_envs != (int64_t)src.num_envs * n) { *why = "work.num_envs must be src.num_envs * n_ids"; return HWY_ERR_INVALID_ARG; }
  return HWY_OK;
}

// host side: the planner's own arrays (the layout of OpdParams' fields of the same names; created / child_mask: the masked search's)
struct OpdTree {
  double *ret, *disc, *upper0;
  uint8_t *done;
  int32_t *expanded_node, *gather_src, *scatter_src, *root_src, *actions;
  uint8_t *created, *child_mask;
};
// ... the plan's outputs (everything but action may be null)
struct OpdPlan {
  int32_t *action;
  double *value, *upper;
  int32_t *sequence, *expanded;
};
// ... and the arguments of the tree kernel over them and the work engine's step outputs (opd_validate has passed); p.x is the
// launch's own
inline OpdParams opd_params(const hwy_opd_params &params, int32_t num_envs, const OpdTree &t, const double *reward,
                            const uint8_t *terminated, const uint8_t *truncated, const OpdPlan &out) {
  OpdParams p;
  memset(&p, 0, sizeof p);
  p.ret = t.ret; p.disc = t.disc; p.upper0 = t.upper0; p.done = t.done;
  p.expanded_node = t.expanded_node;
  p.reward = reward; p.terminated = terminated; p.truncated = truncated;
  p.gather_src = t.gather_src; p.scatter_src = t.scatter_src; p.root_src = t.root_src;
  p.actions = t.actions;
  p.action = out.action; p.value = out.value; p.upper = out.upper; p.sequence = out.sequence; p.expanded = out.expanded;
  p.gamma = params.gamma; p.bound = params.bound;
  p.X = params.budget / params.n_ids; p.n = params.n_ids; p.M = params.nodes; p.E = num_envs;
  if (params.flags & HWY_OPD_MASKED) { p.created = t.created; p.child_mask = t.child_mask; }
  return p;
}

// host side: THE sequence of a plan -- per expansion x the tree kernel, the root's state into tree slot e * M and the parent's into all
// n work environments of e (x == 0) or the gather tree -> work, the mask of the selected leaf on the work engine (masked search:
// work's n copies of its state, row e * n is read, before the step moves them), one step of the work engine with the action plane
// the kernel wrote, the scatter work -> tree; and one more kernel for the plan.  Generic over what enqueues (hwy_engine.hip:
// hwy_opd_plan_device, on streams) or runs (tests/emu/emu_opd.cpp) the operations, each returning 0 or the status the plan ends with:
//   ops.after(waiter, signaler)             waiter's stream continues behind what signaler's holds so far (the emulation: nothing)
//   ops.kernel(const OpdParams &)           the tree kernel
//   ops.fork(dst, src, branches, src_env)   hwy_fork_device between two of the three engines (it orders destination behind source)
//   ops.mask()                              the action mask of the work engine into p.child_mask
//   ops.step(actions)                       one policy step of the work engine, outputs to p.reward / p.terminated / p.truncated
// Everything of the planner's own runs on work's stream.  Before a tree kernel rewrites the scatter's indices, the scatter that reads
// them on tree's stream has to be over.
enum OpdEngine { OPD_SRC, OPD_TREE, OPD_WORK };
template <typename Ops>
int opd_expand(OpdParams p, Ops &&ops) {
  for (int32_t x = 0; x <= p.X; ++x) {
    if (int rc = ops.after(OPD_WORK, OPD_TREE)) return rc;
    p.x = x;
    if (int rc = ops.kernel(p)) return rc;
    if (x == p.X) break;
    if (x == 0) {
      if (int rc = ops.after(OPD_TREE, OPD_WORK)) return rc;
      if (int rc = ops.fork(OPD_TREE, OPD_SRC, 1, p.root_src)) return rc;
      if (int rc = ops.fork(OPD_WORK, OPD_SRC, p.n, nullptr)) return rc;
    } else {
      if (int rc = ops.fork(OPD_WORK, OPD_TREE, 1, p.gather_src)) return rc;
    }
    if (p.child_mask)
      if (int rc = ops.mask()) return rc;
    if (int rc = ops.step(p.actions)) return rc;
    if (int rc = ops.fork(OPD_TREE, OPD_WORK, 1, p.scatter_src)) return rc;
  }
  return HWY_OK;
}

// The tree step shared by the two kernels below.  MASKED: a node's unavailable actions get no child -- the slot 1 + x * n + a stays
// reserved and counts as never created (sh_exp == -2): it is not ingested, and the backup, the selection and the plan run over
// created children only (IDLE always exists, so an expanded node always has a child).  The values of a never-created slot are
// +inf in LDS, so that a read which forgets the guard cannot go unnoticed.
template <int CAP, bool MASKED>
__device__ __forceinline__ void opd_tree_step(const OpdParams &p) {
  __shared__ double sh_lo[CAP], sh_up[CAP];   // value lower / upper of every node
  __shared__ int32_t sh_exp[CAP];             // the expansion that expanded the node; -1: a leaf; -2: never created
  __shared__ int32_t sh_node[CAP];            // the node expansion j expanded (-1: void)
  __shared__ uint8_t sh_done[CAP];
  __shared__ unsigned long long sh_key[2];    // keys of the maxima of the phase at hand
  __shared__ int32_t sh_arg;                  // lowest index holding the maximum
  const int lane = (int)threadIdx.x, e = (int)blockIdx.x;
  const int n = p.n, M = p.M, X = p.X, x = p.x;
  const size_t row = (size_t)e * M, xrow = (size_t)e * X;
  const int old = x > 0 ? 1 + (x - 1) * n : 0;  // nodes [0, old) were created by earlier launches
  const int prev = x > 0 ? p.expanded_node[xrow + x - 1] : -1;  // (wavefront-uniform) the leaf whose children arrive now

  // ---- 1. the tree as the earlier launches left it, and the children of expansion x - 1 ----------------------------------------------
  for (int j = lane; j < x; j += 64) sh_node[j] = p.expanded_node[xrow + j];
  for (int i = lane; i < M; i += 64) {
    bool created = i == 0 || ((i - 1) / n < x && p.expanded_node[xrow + (i - 1) / n] >= 0);
    if (MASKED && created && i > 0)  // (the children that arrive now: from the mask kernel's output; the older ones: as recorded)
      created = ((i - 1) / n == x - 1 ? p.child_mask[(size_t)e * n * n + (i - 1) % n] : p.created[row + i]) != 0;
    sh_exp[i] = created ? -1 : -2;
    if (MASKED && !created) { sh_lo[i] = __builtin_inf(); sh_up[i] = __builtin_inf(); }
    if (i < old && created && x > 0) {
      sh_lo[i] = p.ret[row + i];
      sh_up[i] = p.upper0[row + i];
      sh_done[i] = p.done[row + i];
    }
  }
  if (x == 0 && lane == 0) {  // the root
    p.ret[row] = 0.0; p.disc[row] = 1.0; p.upper0[row] = p.bound; p.done[row] = 0;
    sh_lo[0] = 0.0; sh_up[0] = p.bound; sh_done[0] = 0;
  }
  if (prev >= 0) {
    const double ret_p = p.ret[row + prev], disc_p = p.disc[row + prev];
    for (int a = lane; a < n; a += 64) {
      const int c = old + a;
      const size_t w = (size_t)e * n + a;
      if (MASKED) {
        const bool available = p.child_mask[(size_t)e * n * n + a] != 0;
        p.created[row + c] = available ? 1 : 0;
        if (!available) continue;  // no child: nothing is ingested
      }
      const double t = disc_p * p.reward[w];
      const double lower = ret_p + t;
      const double disc = disc_p * p.gamma;
      const bool done = (p.terminated[w] | p.truncated[w]) != 0;
      double upper = lower;
      if (!done) {
        const double u = disc * p.bound;
        upper = lower + u;
      }
      p.ret[row + c] = lower; p.disc[row + c] = disc; p.upper0[row + c] = upper; p.done[row + c] = done ? 1 : 0;
      sh_lo[c] = lower; sh_up[c] = upper; sh_done[c] = done ? 1 : 0;
    }
  }
  if (lane < 2) sh_key[lane] = 0ull;
  if (lane == 0) sh_arg = 0x7fffffff;
  __syncthreads();
  for (int j = lane; j < x; j += 64)
    if (sh_node[j] >= 0) sh_exp[sh_node[j]] = j;
  __syncthreads();

  // ---- 2. backup: the expansions in reverse order ------------------------------------------------------------------------------------
  for (int j = x - 1; j >= 0; --j) {
    const int node = sh_node[j];
    if (node < 0) continue;  // (uniform) a void expansion
    for (int a = lane; a < n; a += 64) {
      if (MASKED && sh_exp[1 + j * n + a] == -2) continue;  // never created
      const unsigned long long klo = score_key(sh_lo[1 + j * n + a]), kup = score_key(sh_up[1 + j * n + a]);
      __hip_atomic_fetch_max(&sh_key[0], klo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_max(&sh_key[1], kup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (lane == 0) {
      sh_lo[node] = score_unkey(sh_key[0]);
      sh_up[node] = score_unkey(sh_key[1]);
      sh_key[0] = 0ull; sh_key[1] = 0ull;
    }
    __syncthreads();
  }

  if (x < X) {
    // ---- 3a. selection: the leaf of the largest value upper, the lowest index among its holders ---------------------------------------
    for (int i = lane; i < M; i += 64)
      if (sh_exp[i] == -1) {
        const unsigned long long key = score_key(sh_up[i]);
        __hip_atomic_fetch_max(&sh_key[0], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    __syncthreads();
    const unsigned long long top = sh_key[0];
    for (int i = lane; i < M; i += 64)
      if (sh_exp[i] == -1 && score_key(sh_up[i]) == top) __hip_atomic_fetch_min(&sh_arg, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const int leaf = sh_arg;                 // (the root or a created node: there is always a leaf)
    const bool is_void = sh_done[leaf] != 0;    // the tree is solved: nothing is created any more
    if (lane == 0) p.expanded_node[xrow + x] = is_void ? -1 : leaf;
    const int first = 1 + x * n;
    for (int a = lane; a < n; a += 64) {
      p.gather_src[(size_t)e * n + a] = is_void ? -1 : (int32_t)(row + leaf);
      if (x == 0) p.actions[(size_t)e * n + a] = a;
    }
    for (int i = lane; i < M; i += 64) {
      p.scatter_src[row + i] = (!is_void && i >= first && i < first + n) ? (int32_t)((size_t)e * n + (i - first)) : -1;
      if (x == 0) p.root_src[row + i] = i == 0 ? e : -1;
    }
    return;
  }

  // ---- 3b. the plan: from the root along the children that hold their parent's value lower (the maximum), lowest id first ------------
  int node = 0, made = 0;
  for (int j = 0; j < X; ++j) made += sh_node[j] >= 0;
  for (int d = 0; d < X; ++d) {
    const int j = node >= 0 ? sh_exp[node] : -1;   // (uniform)
    int a_best = -1;
    if (j >= 0) {
      unsigned long long want = score_key(sh_lo[node]);
      if (MASKED) {  // the maximum over the created children themselves (what the backup gave the node)
        for (int a = lane; a < n; a += 64)
          if (sh_exp[1 + j * n + a] != -2) __hip_atomic_fetch_max(&sh_key[0], score_key(sh_lo[1 + j * n + a]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        want = sh_key[0];
        __syncthreads();               // everyone has read it
        if (lane == 0) sh_key[0] = 0ull;
        __syncthreads();
      }
      for (int a = lane; a < n; a += 64)
        if ((!MASKED || sh_exp[1 + j * n + a] != -2) && score_key(sh_lo[1 + j * n + a]) == want) __hip_atomic_fetch_min(&sh_arg, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __syncthreads();
      a_best = sh_arg;
      __syncthreads();                 // everyone has read it
      if (lane == 0) sh_arg = 0x7fffffff;
      __syncthreads();
    }
    if (lane == 0) {
      if (p.sequence) p.sequence[xrow + d] = a_best;
      if (d == 0) p.action[e] = a_best;
    }
    node = j >= 0 ? 1 + j * n + a_best : -1;
  }
  if (lane == 0) {
    if (p.value) p.value[e] = sh_lo[0];
    if (p.upper) p.upper[e] = sh_up[0];
    if (p.expanded) p.expanded[e] = made;
  }
}

template <int CAP>
__global__ void __launch_bounds__(64) hwy_opd_kernel(const OpdParams p) {
  opd_tree_step<CAP, false>(p);
}
// the masked search (hwy_opd_params.flags & HWY_OPD_MASKED): p.child_mask and p.created are set
template <int CAP>
__global__ void __launch_bounds__(64) hwy_opd_masked_kernel(const OpdParams p) {
  opd_tree_step<CAP, true>(p);
}

}  // namespace hwy
