"""Envs of varying human count (config.sim.human_nums), the parts that need no GPU: the group assignment of
config.make_varied_cn_configs and its agreement across shards, the observation space, the configurations that
are turned down before anything touches the GPU, and that a config without the opt-in translates as ever."""
import hashlib
import types

import numpy as np
import pytest

from crowdnav_dsrnn_amd import spaces
from crowdnav_dsrnn_amd.config import (Config, UnsupportedConfig, clone_config, make_cn_config,
                                       make_varied_cn_configs, varied_human_nums)


def _cfg(**sim):
    c = clone_config(Config())
    for k, v in sim.items():
        setattr(c.sim, k, v)
    return c


def _bytes_but(c, *skip):
    """The struct's fields as a dict without `skip` (ctypes arrays as tuples)."""
    out = {}
    for name, _ in c._fields_:
        if name not in skip:
            v = getattr(c, name)
            out[name] = tuple(v) if hasattr(v, "__len__") else v
    return out


def test_group_assignment_follows_the_global_env_index():
    c = _cfg()
    cfgs, eg = make_varied_cn_configs(c, [5, 10, 5, 1], 11, env_offset=3, nenv=19, phase="train", seed=4)
    assert [k.human_num for k in cfgs] == [5, 10, 1]            # one group per distinct count, first-seen order
    want = [[5, 10, 5, 1][(3 + r) % 4] for r in range(11)]
    assert [cfgs[g].human_num for g in eg] == want
    assert eg.dtype == np.int32 and [k.num_envs for k in cfgs] == [int((eg == g).sum()) for g in range(3)]
    # identical except the count (and the group's size); each carries the full scenario list
    plain = make_cn_config(c, num_envs=11, env_offset=3, nenv=19, phase="train", seed=4)
    for k in cfgs:
        assert _bytes_but(k, "human_num", "num_envs") == _bytes_but(plain, "human_num", "num_envs")
        assert k.num_scenarios == len(c.sim.train_val_sim) and (k.env_offset, k.nenv, k.seed) == (3, 19, 4)


def test_shards_agree_with_the_unsharded_run():
    c, nums, E = _cfg(), [3, 7, 12], 20
    whole, eg = make_varied_cn_configs(c, nums, E, nenv=E)
    counts = [whole[g].human_num for g in eg]
    got = []
    for rank in range(4):
        cfgs, egs = make_varied_cn_configs(c, nums, E // 4, env_offset=rank * (E // 4), nenv=E)
        got += [cfgs[g].human_num for g in egs]
        assert all(k.nenv == E and k.env_offset == rank * (E // 4) for k in cfgs)
    assert got == counts == [nums[g % 3] for g in range(E)]


@pytest.mark.parametrize("nums", [[], [0, 5], [5, 32], [5, -1], [2.5], "5", 5])
def test_bad_human_nums_are_unsupported(nums):
    with pytest.raises(UnsupportedConfig):
        make_varied_cn_configs(_cfg(), nums, 4)


def test_caller_config_is_left_unmodified():
    c = _cfg(human_num=6)
    before = {s: dict(vars(getattr(c, s))) for s in dir(c) if type(getattr(c, s)).__name__ == "BaseConfig"}
    make_varied_cn_configs(c, [2, 9], 8)
    after = {s: dict(vars(getattr(c, s))) for s in dir(c) if type(getattr(c, s)).__name__ == "BaseConfig"}
    assert after == before and c.sim.human_num == 6 and c.sim.human_nums is None
    assert varied_human_nums(c) is None


def test_observation_space_keys_and_shapes():
    sp = spaces.observation_space(12, detected_human_num=True).spaces
    assert list(sp) == ["robot_node", "temporal_edges", "spatial_edges", "detected_human_num"]
    assert [tuple(sp[k].shape) for k in sp] == [(1, 7), (1, 2), (12, 2), (1,)]
    assert all(sp[k].dtype == np.float32 for k in sp)
    plain = spaces.observation_space(12).spaces
    assert list(plain) == ["robot_node", "temporal_edges", "spatial_edges"]


def test_convgru_with_human_nums_is_unsupported_before_the_gpu():
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv, make_vec_envs

    c = _cfg(human_nums=[5, 10])
    c.robot.policy = "convgru"
    c.lidar.enable = True
    with pytest.raises(UnsupportedConfig, match="convgru"):
        CrowdNavVecEnv(c, 4, 0, "cpu")
    with pytest.raises(UnsupportedConfig, match="convgru"):
        make_vec_envs("CrowdSimDict-v0", 0, 4, 0.99, None, "cpu", False, config=c)
    c = _cfg(human_nums=[5, 40])
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        CrowdNavVecEnv(c, 4, 0, "cpu")


def test_scripted_robot_and_behaviour_cloning_are_unsupported_before_the_gpu():
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner.imitation import BehaviourCloning
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c = _cfg(human_nums=[5, 10])
    venv = types.SimpleNamespace(config=c, obs_mode="srnn")   # (no engine: the checks read the config alone)
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        ScriptedRobot(venv, "orca")
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        ScriptedRobot.check_rollout(venv, "social_force")
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        BehaviourCloning(c, venv, types.SimpleNamespace(srnn=True), expert="orca")
    bare = CrowdNavVecEnv.__new__(CrowdNavVecEnv)          # the env's own rollout / robot_act: same answer
    bare.config = c
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        bare.rollout("orca", 4)
    with pytest.raises(UnsupportedConfig, match="human_nums"):
        bare.robot_act("orca")
    ScriptedRobot.check(types.SimpleNamespace(config=_cfg()), "orca")   # without the opt-in: as ever


def test_config_without_human_nums_translates_as_before():
    """The default config's cn_config, byte for byte (sha256 of the struct, recorded before sim.human_nums
    existed), with the attribute at its default None and with the attribute absent altogether."""
    want = {"a": "094303c151f1acadcbe9f225689c061ebe2d6f0c30560a2e891428758f225d08",
            "b": "9d37dbc723c9d6abcd7df005e374e459b9dcc61e3b09cab56c5be53b60266b54"}
    c = _cfg()
    absent = _cfg()
    del absent.sim.human_nums
    assert not hasattr(absent.sim, "human_nums")
    for cfg in (c, absent):
        assert hashlib.sha256(bytes(make_cn_config(cfg, num_envs=12))).hexdigest() == want["a"]
        assert hashlib.sha256(bytes(make_cn_config(cfg, num_envs=7, env_offset=3, nenv=19, phase="train",
                                                   seed=11))).hexdigest() == want["b"]
    assert varied_human_nums(absent) is None


def test_edge_attention_torch_branch_masks_padded_slots(monkeypatch):
    """EdgeAttention's torch branch (sizes the kernels do not serve; here H = 96 on the CPU with the pooling
    restated in torch) with per-row counts: every row equals the plain forward over its first count slots, attn
    is 0 in the padded slots, and NaN held there reaches neither an output nor a gradient."""
    import torch

    from crowdnav_dsrnn_amd import ops
    from crowdnav_dsrnn_amd.policy.srnn_model import EdgeAttention
    from tests.helpers import attention_pool_ref

    monkeypatch.setattr(ops, "attention_pool", attention_pool_ref)
    c = _cfg()
    c.SRNN.human_human_edge_rnn_size = 96
    torch.manual_seed(2)
    att = EdgeAttention(c)
    T, B, N, Hh = 2, 3, 5, 96
    count = torch.tensor([1, 3, 5, 2, 5, 4], dtype=torch.int32)
    ht = torch.randn(T, B, Hh)
    hs = torch.randn(T, B, N, Hh)
    pad = ~(torch.arange(N)[None, :] < count[:, None]).reshape(T, B, N)
    hs_nan = hs.masked_fill(pad.unsqueeze(-1), float("nan")).requires_grad_(True)
    w, a = att(ht, hs_nan, count)
    (w.sum() + (a.reshape(T, B, N)[~pad]).sum()).backward()
    assert torch.isfinite(w).all() and torch.isfinite(a).all() and torch.isfinite(hs_nan.grad).all()
    assert (a.reshape(T, B, N)[pad] == 0).all() and (hs_nan.grad[pad] == 0).all()
    for r in range(T * B):
        t, b, n = r // B, r % B, int(count[r])
        w1, a1 = att(ht[t:t + 1, b:b + 1], hs[t:t + 1, b:b + 1, :n])
        np.testing.assert_allclose(w[t, b].detach().numpy(), w1[0, 0].detach().numpy(), atol=1e-6, rtol=1e-5)
        np.testing.assert_allclose(a[r, :n, 0].detach().numpy(), a1[0, :, 0].detach().numpy(), atol=1e-6, rtol=1e-5)
