"""``plan_opd`` tied to code that other tests pin, and its index arithmetic, on the CPU emulation and (marked ``gpu``) the MI355X.

* one expansion is ``plan_lookahead(1)``; ``score_sequences`` of the greedy sequence at the same gamma gives ``value`` bit for bit
  (the path return of a node IS score_return of its action sequence); value <= upper; for a tree that is not solved
  upper - value <= gamma ** depth_min * bound, depth_min the depth of its shallowest leaf.  (In exact arithmetic
  upper = max over the leaves of ret + gamma ** depth * bound <= value + gamma ** depth_min * bound.  ``lower + u`` rounds once, so
  the inequality could miss by an ulp only where the leaf that holds the value is also a shallowest leaf; with 3 and 17 expansions of
  5 actions the shallowest leaves are at depth 1 with returns <= 1 and the value, from a deeper leaf, is about 2.)
* the plan of ``env.fork(source=[2, 0])`` is rows [2, 0] of the parent's plan, an E == 1 environment gives row 0, two calls in a row
  are identical, and a plan leaves the parent's state, stored controls and next step exactly as they were."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import opd_util as ou

GAMMA, SEED = 0.7, 11
BOUND = 1.0 / (1.0 - GAMMA)
_cache = {}


def base(backend):
    """The E = 3 environment the module shares (never stepped), its plans at budgets 15 and 85 and the yardstick's trees."""
    if backend not in _cache:
        env = ou.make_env(backend, ou.fast_config(8), 3, SEED)
        plans = {b: env.plan_opd(b, GAMMA, return_details=True) for b in (15, 85)}
        trees = {b: ou.restate_opd(backend, env, b, GAMMA) for b in (15, 85)}
        _cache[backend] = (env, plans, trees)
    return _cache[backend]


@pytest.mark.parametrize("backend", ou.BACKENDS)
def test_one_expansion_is_the_depth_one_lookahead(backend):
    env, _, _ = base(backend)
    action, details = env.plan_opd(5, GAMMA, return_details=True)
    best, q = env.plan_lookahead(1, gamma=GAMMA, return_q=True)
    np.testing.assert_array_equal(action, best)
    ou.assert_bits(details["value"], q.max(axis=1), "value == the best one-step return")
    np.testing.assert_array_equal(details["sequence"][:, 0], best)


@pytest.mark.parametrize("backend", ou.BACKENDS)
@pytest.mark.parametrize("budget", [15, 85])
def test_value_is_the_scored_return_of_the_sequence_and_the_bounds_hold(backend, budget):
    env, plans, trees = base(backend)
    action, details = plans[budget]
    seq, value, upper = details["sequence"], details["value"], details["upper"]
    length = (seq >= 0).sum(axis=1)
    assert (length >= 1).all() and all((seq[e, :length[e]] >= 0).all() and (seq[e, length[e]:] == -1).all() for e in range(3))
    for L in np.unique(length):   # one call per distinct length, the sequences cut at it
        returns = env.score_sequences(np.maximum(seq[:, None, :L], 0), gamma=GAMMA)
        rows = length == L
        ou.assert_bits(returns[rows, 0], value[rows], f"score_sequences of the sequences of length {L}")
    assert (value <= upper).all()
    for e in range(3):
        if details["expanded"][e] == seq.shape[1]:   # not solved
            d = ou.depth_min(trees[budget]["trees"][e])
            print("budget", budget, "env", e, "upper - value", upper[e] - value[e], "gamma ** depth_min * bound", GAMMA ** d * BOUND, "depth_min", d)
            assert upper[e] - value[e] <= GAMMA ** d * BOUND


@pytest.mark.parametrize("backend", ou.BACKENDS)
def test_rows_of_a_fork_a_single_environment_and_a_second_call(backend):
    env, plans, _ = base(backend)
    action, details = plans[15]
    again_action, again = env.plan_opd(15, GAMMA, return_details=True)   # (budget 85 ran in between on the same tree engine)
    child = env.fork(source=[2, 0])
    sub_action, sub = child.plan_opd(15, GAMMA, return_details=True)
    one = ou.make_env(backend, ou.fast_config(8), 1, SEED)
    one_action, one_details = one.plan_opd(15, GAMMA, return_details=True)
    one.close()
    np.testing.assert_array_equal(again_action, action)
    np.testing.assert_array_equal(sub_action, action[[2, 0]])
    np.testing.assert_array_equal(one_action, action[:1])
    for k in ("value", "upper", "sequence", "expanded"):
        ou.assert_bits(again[k], details[k], f"second call: {k}")
        ou.assert_bits(sub[k], details[k][[2, 0]], f"fork(source=[2, 0]): {k}")
        ou.assert_bits(one_details[k], details[k][:1], f"E == 1: {k}")


@pytest.mark.parametrize("backend", ou.BACKENDS)
def test_a_plan_leaves_the_parent_as_it_was(backend):
    config = ou.fast_config(8, action={"type": "DiscreteAction"})
    planner, witness = (ou.make_env(backend, config, 3, 13, warm=(5,)) for _ in range(2))
    before, controls = planner.get_state(), planner._engine.get_controls()
    assert np.abs(controls[0]).max() > 0 or np.abs(controls[1]).max() > 0
    planner.plan_opd(27, GAMMA)
    after = planner.get_state()
    for k in ou.STATE_KEYS:
        ou.assert_bits(before[k], after[k], k)
    for a, b in zip(controls, planner._engine.get_controls()):
        ou.assert_bits(a, b, "stored controls")
    acts = np.array([7, 2, 4], np.int32)
    for got, want in zip(planner.step(acts)[:4], witness.step(acts)[:4]):
        ou.assert_bits(got, want, "the step after a plan")
    planner.close(), witness.close()
