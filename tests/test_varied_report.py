"""The per-human-count block of the evaluation report (evaluation.per_count_summary / log_per_count / _report), on
synthetic episode records: no GPU."""
import numpy as np

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config
from crowdnav_dsrnn_amd.evaluation import EpisodeRecorder, _report, evaluate, per_count_summary

S, C, TO = abi.EV_REACHGOAL, abi.EV_COLLISION, abi.EV_TIMEOUT


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


class _Envs:
    scenario_names = list(abi.SCENARIOS)

    def close(self):
        pass


def _records(events, humans):
    """Per-episode records as EpisodeRecorder.host_records returns them, with the given ends and counts."""
    n = len(events)
    rec = EpisodeRecorder(1, n, 0, 1, "cpu", 0.25, 0.99, 1.0)
    r = {k: v[:n].numpy().copy() for k, v in rec.rec.items()}
    r["event"][:] = events
    r["done"][:] = 1
    r["steps"][:] = 4
    for j, k in enumerate(("gt", "raw", "disc", "path", "chc")):   # (distinct values: the metrics' intervals exist)
        r[k][:] = 1.0 + 0.25 * (j + 1) * np.arange(n)
    r["scenario"][:] = abi.SCENARIOS.index("circle_crossing")
    if humans is None:
        del r["humans"]
    else:
        r["humans"][:] = humans
    return r


def _run_report(r):
    c = clone_config(Config())
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    log = _Log()
    _report(r, {}, c, log, len(r["event"]), 0.25, 0.99, False, None, _Envs(), verbose=False)
    return log.lines, dict(evaluate.last)


EVENTS = [S, S, C, TO, S, C, S, S, TO, S]
HUMANS = [5, 10, 5, 10, 5, 10, 7, 5, 10, 5]


def test_per_count_summary_rates():
    pc = per_count_summary(_records(EVENTS, HUMANS))
    assert list(pc) == [5, 7, 10]
    assert pc[5] == {"episodes": 5, "success_rate": 4 / 5, "collision_rate": 1 / 5, "timeout_rate": 0.0}
    assert pc[7] == {"episodes": 1, "success_rate": 1.0, "collision_rate": 0.0, "timeout_rate": 0.0}
    assert pc[10] == {"episodes": 4, "success_rate": 1 / 4, "collision_rate": 1 / 4, "timeout_rate": 2 / 4}
    for key, ev in (("success_rate", S), ("collision_rate", C), ("timeout_rate", TO)):
        assert abs(sum(v[key] * v["episodes"] for v in pc.values()) - EVENTS.count(ev)) < 1e-12


def test_per_count_summary_is_absent_for_one_count_or_no_counts():
    assert per_count_summary(_records(EVENTS, [5] * 10)) is None
    assert per_count_summary(_records(EVENTS, None)) is None
    assert per_count_summary(_records(EVENTS, [0] * 10)) is None       # a recorder that was given no counts


def test_recorder_writes_the_count_of_the_env_that_ran_the_episode():
    """3 envs of counts 5, 10, 7, episodes of one step: episode g is run by env g % 3."""
    import torch

    rec = EpisodeRecorder(3, 7, 0, 3, "cpu", 0.25, 0.99, 1.0, env_humans=[5, 10, 7])
    obs = {"robot_node": torch.zeros(3, 1, 7), "temporal_edges": torch.zeros(3, 1, 2)}
    rec.start(obs)
    while not rec.finished():
        rec.step(obs, torch.zeros(3), torch.ones(3, dtype=torch.uint8), torch.full((3,), S, dtype=torch.int8),
                 torch.zeros(3, abi.INFO_K))
    assert rec.host_records()["humans"].tolist() == [5, 10, 7, 5, 10, 7, 5]
    plain = EpisodeRecorder(3, 7, 0, 3, "cpu", 0.25, 0.99, 1.0)
    assert plain.host_records()["humans"].tolist() == [0] * 7


def test_report_gains_the_block_only_for_varied_counts():
    """Equal counts: the log is line for line the log of records without counts, and evaluate.last has no
    'per_count'. Varied counts: the same lines, then the block, one line per count in ascending order."""
    base, last0 = _run_report(_records(EVENTS, None))
    same, last1 = _run_report(_records(EVENTS, [5] * 10))
    assert same == base and "per_count" not in last0 and "per_count" not in last1
    assert not any("PER HUMAN COUNT" in ln for ln in base)
    varied, last2 = _run_report(_records(EVENTS, HUMANS))
    assert varied[:len(base)] == base
    assert varied[len(base):] == [
        "", "PER HUMAN COUNT: ",
        "5 humans: success rate: 0.800, collision rate: 0.200, timeout rate: 0.000, episodes: 5",
        "7 humans: success rate: 1.000, collision rate: 0.000, timeout rate: 0.000, episodes: 1",
        "10 humans: success rate: 0.250, collision rate: 0.250, timeout rate: 0.500, episodes: 4"]
    assert last2["per_count"] == per_count_summary(_records(EVENTS, HUMANS))
    assert last2["success_rate"] == 0.6 and np.isclose(
        sum(v["success_rate"] * v["episodes"] for v in last2["per_count"].values()) / 10, 0.6)
