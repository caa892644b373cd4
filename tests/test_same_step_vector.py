"""``HighwayVectorEnv(..., output="torch", autoreset_mode="SameStep")``: gymnasium's SameStep contract without a host round trip.

The torch SameStep env against the torch NextStep env on the same seed, with actions a function of (environment, episode, step in
the episode): the same useful steps, the terminal observation in ``infos["final_obs"]`` where NextStep returns it as ``obs``, the
first observation of the next episode as ``obs`` where NextStep returns it one call later.  The dense extras are checked key by key;
with ``action_masks=True`` the ended episode's mask and the new state's are checked against ``get_available_actions()`` of engines
that ARE in those states (the NextStep env right after its ending step; the SameStep env itself after the call)."""
import numpy as np
import pytest

from highwayenv_amd import vector

E, CALLS = 8, 20
CFG = {"duration": 3, "vehicles_density": 2.0}


def test_intersection_keeps_a_value_error():
    with pytest.raises(ValueError, match="intersection"):
        vector.HighwayVectorEnv("intersection-v0", num_envs=2, output="torch", autoreset_mode="SameStep")


def _action(e, episode, k):
    h = (e * 7919 + episode * 104729 + k * 1299709) % 11
    return 3 if h < 7 else h % 5  # mostly FASTER: episodes end by a crash as well as by the time limit


def _actions(episode, k):
    return np.array([_action(e, int(episode[e]), int(k[e])) for e in range(E)], np.int32)


def _host(x):
    return x.cpu().numpy().copy()


def _run_same_step(torch, venv, calls, seed):
    """[per call: dict of host copies], and per environment the list of its useful steps."""
    obs0, _ = venv.reset(seed=seed)
    episode, k = np.zeros(E, int), np.zeros(E, int)
    raw, steps = [], [[] for _ in range(E)]
    for _ in range(calls):
        obs, reward, term, trunc, infos = venv.step(torch.as_tensor(_actions(episode, k), device="cuda"))
        # keys, dtypes and shapes of the dense extras
        assert set(infos) == {"speed", "crashed", "action_mask", "final_obs", "_final_obs", "final_info", "_final_info"}
        assert infos["final_obs"].shape == obs.shape == (E, 5, 5) and infos["final_obs"].dtype == torch.float32 and infos["final_obs"].is_cuda
        assert infos["_final_obs"].dtype == torch.bool and infos["_final_obs"].shape == (E,)
        assert infos["_final_info"] is infos["_final_obs"] or torch.equal(infos["_final_info"], infos["_final_obs"])
        assert set(infos["final_info"]) == {"speed", "crashed", "action_mask"}
        assert infos["final_info"]["speed"].dtype == torch.float64 and infos["final_info"]["speed"].shape == (E,)
        assert infos["final_info"]["crashed"].dtype == torch.bool and infos["final_info"]["crashed"].shape == (E,)
        assert infos["final_info"]["action_mask"].dtype == torch.bool and infos["final_info"]["action_mask"].shape == (E, 5)
        assert infos["action_mask"].dtype == torch.bool and infos["action_mask"].shape == (E, 5)
        assert torch.equal(infos["_final_obs"], term | trunc)
        c = {"obs": _host(obs), "reward": _host(reward), "terminated": _host(term), "truncated": _host(trunc),
             "speed": _host(infos["speed"]), "crashed": _host(infos["crashed"]), "action_mask": _host(infos["action_mask"]),
             "final_obs": _host(infos["final_obs"]), "final_mask": _host(infos["_final_obs"]),
             "final_speed": _host(infos["final_info"]["speed"]), "final_crashed": _host(infos["final_info"]["crashed"]),
             "final_action_mask": _host(infos["final_info"]["action_mask"])}
        # the mask next to the returned observation is that of the state the engine is in now
        np.testing.assert_array_equal(c["action_mask"], venv.env.get_available_actions())
        raw.append(c)
        for e in range(E):
            end = bool(c["final_mask"][e])
            src = ("final_obs", "final_speed", "final_crashed", "final_action_mask") if end else ("obs", "speed", "crashed", "action_mask")
            steps[e].append({"episode": int(episode[e]), "k": int(k[e]), "obs": c[src[0]][e], "reward": c["reward"][e],
                             "terminated": bool(c["terminated"][e]), "truncated": bool(c["truncated"][e]), "speed": c[src[1]][e],
                             "crashed": bool(c[src[2]][e]), "mask": c[src[3]][e], "next_obs": c["obs"][e] if end else None,
                             "next_speed": c["speed"][e] if end else None, "next_mask": c["action_mask"][e] if end else None})
            episode[e], k[e] = (episode[e] + 1, 0) if end else (episode[e], k[e] + 1)
    return _host(obs0), raw, steps


def _run_next_step(torch, venv, calls, seed):
    obs0, _ = venv.reset(seed=seed)
    episode, k = np.zeros(E, int), np.zeros(E, int)
    pending = np.zeros(E, bool)
    steps = [[] for _ in range(E)]
    for _ in range(4 * calls):
        if min(len(s) for s in steps) >= calls and not pending.any():
            break
        obs, reward, term, trunc, infos = venv.step(torch.as_tensor(_actions(episode, k), device="cuda"))
        obs, reward, term, trunc = _host(obs), _host(reward), _host(term), _host(trunc)
        speed, crashed, mask = _host(infos["speed"]), _host(infos["crashed"]), _host(infos["action_mask"])
        np.testing.assert_array_equal(mask, venv.env.get_available_actions())  # (the engine IS in the state the mask is of)
        for e in range(E):
            if pending[e]:
                steps[e][-1].update(next_obs=obs[e], next_speed=speed[e], next_mask=mask[e])
                pending[e] = False
                continue
            end = bool(term[e] | trunc[e])
            steps[e].append({"episode": int(episode[e]), "k": int(k[e]), "obs": obs[e], "reward": reward[e], "terminated": bool(term[e]),
                             "truncated": bool(trunc[e]), "speed": speed[e], "crashed": bool(crashed[e]), "mask": mask[e],
                             "next_obs": None, "next_speed": None, "next_mask": None})
            pending[e] = end
            episode[e], k[e] = (episode[e] + 1, 0) if end else (episode[e], k[e] + 1)
    return _host(obs0), [s[:calls] for s in steps]


@pytest.mark.gpu
def test_torch_same_step_describes_the_episodes_of_next_step():
    import torch
    same = vector.HighwayVectorEnv("highway-fast-v0", E, config=CFG, output="torch", autoreset_mode="SameStep", action_masks=True)
    nxt = vector.HighwayVectorEnv("highway-fast-v0", E, config=CFG, output="torch", action_masks=True)
    try:
        obs_s, raw, got = _run_same_step(torch, same, CALLS, seed=11)
        obs_n, want = _run_next_step(torch, nxt, CALLS, seed=11)
        np.testing.assert_array_equal(obs_s, obs_n)
        n_term = n_trunc = 0
        for e in range(E):
            assert len(got[e]) == len(want[e]) == CALLS
            for j, (a, b) in enumerate(zip(got[e], want[e])):
                assert set(a) == set(b)
                for key in a:
                    if a[key] is None or b[key] is None:
                        assert a[key] is None and b[key] is None, f"env {e} useful step {j}: {key}"
                    else:
                        np.testing.assert_array_equal(a[key], b[key], err_msg=f"env {e} useful step {j}: {key}")
                n_term += a["terminated"]
                n_trunc += a["truncated"] and not a["terminated"]
        print(f"{n_term} episodes ended by terminated, {n_trunc} by truncated alone")
        assert n_term > 0 and n_trunc > 0, "the run must see both kinds of ending"
        # a user stream (stream=): the same calls while that stream is current
        lane = torch.cuda.Stream()
        on_lane = vector.HighwayVectorEnv("highway-fast-v0", E, config=CFG, output="torch", autoreset_mode="SameStep", action_masks=True,
                                          stream=lane)
        try:
            assert on_lane.stream is lane
            with torch.cuda.stream(lane):
                _, raw_lane, _ = _run_same_step(torch, on_lane, 8, seed=11)
            assert any(c["final_mask"].any() for c in raw_lane)
            for j, (a, b) in enumerate(zip(raw_lane, raw)):
                ended = b["final_mask"]
                for key in a:
                    rows = ended if key.startswith("final_") and key != "final_mask" else slice(None)  # (final rows: under the mask)
                    np.testing.assert_array_equal(a[key][rows], b[key][rows], err_msg=f"call {j}: {key}")
        finally:
            on_lane.close()
    finally:
        same.close()
        nxt.close()


@pytest.mark.gpu
def test_torch_same_step_on_merge_without_masks():
    import torch
    venv = vector.HighwayVectorEnv("merge-v0", 4, output="torch", autoreset_mode="SameStep")
    try:
        obs, _ = venv.reset(seed=3)
        ended = 0
        for _ in range(16):  # (the ego passes x = 370 m after twelve steps at 30 m/s)
            obs, reward, term, trunc, infos = venv.step(torch.full((4,), 1, dtype=torch.int32, device="cuda"))
            assert set(infos) == {"speed", "crashed", "final_obs", "_final_obs", "final_info", "_final_info"}
            assert set(infos["final_info"]) == {"speed", "crashed"}
            assert torch.equal(infos["_final_obs"], term | trunc)
            ended += int(infos["_final_obs"].sum())
        assert ended > 0
    finally:
        venv.close()
