"""Multi-step launches whose goal changes run on waves 2 and 3 beside the state stores (GOAL_EARLY in
cn_step_kernel's SEQ instantiations) against the same engine at set_seq_chunk(1): the single-step
kernels, which keep the goal changes in phase 5 and which the rest of the suite pins to the oracle. The nine outputs
of the last step and the whole state blob, bit for bit.

The cases are the places where the new order can go wrong: several goal items on one serving wave, a random and an
end goal change in one item, a reset beside goal items in one workgroup and step, many envs per workgroup, the other
LDS shapes (robot.visible, FOV pi), the Philox stream, one workgroup that is full or nearly empty. Every case
asserts its premise on the reference run, stepped one step at a time with the state taken out after each: an env
"changed a goal" in a step when one of its humans' goals differs from the step before and its reset_count did not
move, it "reset" when reset_count moved. The seeds were picked with oracle.cpu_ref.RefEngine on the CPU, so the
premises were known to hold before a GPU saw them. The action streams come from a CPU generator."""
import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

pytestmark = pytest.mark.gpu

OUTPUTS = ("robot_node", "temporal_edges", "spatial_edges", "reward", "done", "event", "info", "ep_return", "ep_len")
CHUNKS = (2, 8, 32)
GOAL_STEP = 19   # the random goal change falls at gtime 5.0: the 20th step of every env's first episode (index 19)


def _cfg(N=10, kin="unicycle", E=13, fov=None, robot_visible=False, seed=None, rng=None):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.robot.visible = robot_visible
    if fov is not None:
        c.robot.FOV = c.humans.FOV = fov
    return make_cn_config(c, num_envs=E, nenv=E, phase="train", seed=seed, rng=rng)


def actions_cpu(T, E, kin, seed):
    """unicycle: U[-0.1, 0.1]^2 (the C2 benchmark's); holonomic: N(0, 0.5^2)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kin == "unicycle":
        return torch.rand((T, E, 2), generator=g) * 0.2 - 0.1
    return torch.randn((T, E, 2), generator=g) * 0.5


class Trace:
    """The state after cn_reset and after every step: goals, positions, radii [T + 1, E, N], reset_count [T + 1, E]."""

    def __init__(self):
        self.gx, self.gy, self.px, self.py, self.r, self.rc = [], [], [], [], [], []

    def add(self, sv):
        for lst, f in ((self.gx, sv.h_gx), (self.gy, sv.h_gy), (self.px, sv.h_px), (self.py, sv.h_py), (self.r, sv.h_r),
                       (self.rc, sv.reset_count)):
            lst.append(np.array(f).copy())

    def done(self):
        for k in ("gx", "gy", "px", "py", "r", "rc"):
            setattr(self, k, np.stack(getattr(self, k)))
        E = self.rc.shape[1]
        for k in ("gx", "gy", "px", "py", "r"):
            setattr(self, k, getattr(self, k).reshape(self.rc.shape[0], E, -1))
        self.reset = self.rc[1:] != self.rc[:-1]                                            # [T, E]
        self.hchg = (self.gx[1:] != self.gx[:-1]) | (self.gy[1:] != self.gy[:-1])           # [T, E, N]
        self.changed = self.hchg.any(axis=2) & ~self.reset                                  # [T, E]
        # the human was within its radius of its old goal after the step's move: update_human_goal's condition
        self.reached = np.hypot(self.gx[:-1] - self.px[1:], self.gy[:-1] - self.py[1:]) < self.r[:-1]
        return self


def _reference(cfg, acts):
    """The chunk-1 engine, one step per call: outputs of the last step, state blob, and the Trace."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(cfg, "cuda:0")
    eng.set_seq_chunk(1)
    eng.reset()
    tr = Trace()
    tr.add(eng.get_state())
    for t in range(acts.shape[0]):
        eng.step_seq(acts[t:t + 1])
        tr.add(eng.get_state())
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in OUTPUTS}
    out["state"] = np.asarray(eng.get_state().blob).view(np.uint8).copy()
    eng.close()
    return out, tr.done()


def _run(cfg, acts, chunk):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(cfg, "cuda:0")
    eng.set_seq_chunk(chunk)
    eng.reset()
    eng.step_seq(acts)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in OUTPUTS}
    out["state"] = np.asarray(eng.get_state().blob).view(np.uint8).copy()
    eng.close()
    return out


def _same(got, ref, what):
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s: %s" % (what, k))


def _check(cfg, acts_cpu, premise, what, chunks=CHUNKS):
    acts = acts_cpu.to("cuda:0").contiguous()
    ref, tr = _reference(cfg, acts)
    premise(tr)
    for chunk in chunks:
        _same(_run(cfg, acts, chunk), ref, "%s, chunk %d" % (what, chunk))
    return ref


# ---- the premises (on a Trace; tools can evaluate them on the CPU oracle's trace as well) -----------------------------

def premise_many_in_block(tr, t, lo, hi, atleast):
    n = int(tr.changed[t, lo:hi].sum())
    print("step %d: %d of envs %d..%d changed a goal" % (t + 1, n, lo, hi - 1))
    assert n >= atleast, n


def premise_both_kinds(tr):
    """Some env and random-goal step with two humans' goals changing, one of which had reached its old goal (the end
    goal change) and one of which had not (the random one)."""
    hits = []
    for t in range(GOAL_STEP, tr.changed.shape[0], 20):
        for e in np.nonzero(tr.changed[t])[0]:
            ch = tr.hchg[t, e]
            if (ch & tr.reached[t, e]).any() and (ch & ~tr.reached[t, e]).any():
                hits.append((t + 1, int(e)))
    print("random and end goal change in one item: (step, env) %s" % hits)
    assert hits


def premise_reset_beside_goal(tr, epb):
    E = tr.changed.shape[1]
    wg = np.arange(E) // epb
    beside, alone = [], []
    for t in range(tr.changed.shape[0]):
        for b in np.unique(wg[tr.reset[t]]):
            (beside if tr.changed[t, wg == b].any() else alone).append((t + 1, int(b)))
    print("(step, workgroup) with a reset beside a goal change: %s; with a reset and no goal change: %s" % (beside, alone))
    assert beside and alone


# ---- the cases ---------------------------------------------------------------------------------------------------------

C1 = dict(N=10, kin="unicycle", E=13, seed=None, aseed=5)


@pytest.mark.parametrize("T", [20, 21])
def test_several_items_per_serving_wave(T):
    """C2's configuration, a partial last workgroup. The random goal change of step 20 falls in the launch's last
    (emitting) step at T = 20 and in its second-to-last at T = 21."""
    cfg = _cfg(C1["N"], C1["kin"], C1["E"], seed=C1["seed"])
    _check(cfg, actions_cpu(T, C1["E"], C1["kin"], C1["aseed"]),
           lambda tr: premise_many_in_block(tr, GOAL_STEP, 0, 6, 4), "C2, T %d" % T)


C2 = dict(E=13, T=45, seed=None, aseed=5)


def test_random_and_end_goal_change_in_one_item():
    cfg = _cfg(10, "unicycle", C2["E"], seed=C2["seed"])
    _check(cfg, actions_cpu(C2["T"], C2["E"], "unicycle", C2["aseed"]), premise_both_kinds, "both kinds")


C3 = dict(E=64, T=60, seed=None, aseed=5)


def test_reset_beside_goal_items_in_one_workgroup_step():
    cfg = _cfg(10, "unicycle", C3["E"], seed=C3["seed"])
    _check(cfg, actions_cpu(C3["T"], C3["E"], "unicycle", C3["aseed"]), lambda tr: premise_reset_beside_goal(tr, 6),
           "reset beside goal items")


# N = 2: a human changes its goal with chance 0.25, so an env does with 0.44: 10 of workgroup 0's 16 envs is the most
# the seeds 0..299 offer (five items per serving wave)
C4 = {4: dict(E=37, seed=29, aseed=5, atleast=12), 2: dict(E=16, seed=95, aseed=5, atleast=10)}


@pytest.mark.parametrize("N", [4, 2])
def test_many_envs_per_workgroup(N):
    """16 envs per workgroup: each serving wave runs half of workgroup 0's items, one after the other (six or more
    at N = 4, five at N = 2)."""
    p = C4[N]
    cfg = _cfg(N, "holonomic", p["E"], seed=p["seed"])
    _check(cfg, actions_cpu(21, p["E"], "holonomic", p["aseed"]),
           lambda tr: premise_many_in_block(tr, GOAL_STEP, 0, 16, p["atleast"]), "N %d" % N)


@pytest.mark.parametrize("shape", ["robot_visible", "fov_pi"])
def test_other_lds_shapes(shape):
    """robot.visible at N = 9 (10 agents per simulator, 9 observed slots) and FOV pi at N = 10 (the belief path)."""
    if shape == "robot_visible":
        cfg, N, E = _cfg(9, "unicycle", 13, robot_visible=True), 9, 13
    else:
        cfg, N, E = _cfg(10, "unicycle", 13, fov=1.0), 10, 13
    _check(cfg, actions_cpu(25, E, "unicycle", 5), lambda tr: premise_many_in_block(tr, GOAL_STEP, 0, E, E // 2), shape)


def test_philox_stream():
    cfg = _cfg(10, "unicycle", 13, rng="philox")
    _check(cfg, actions_cpu(21, 13, "unicycle", 5), lambda tr: premise_many_in_block(tr, GOAL_STEP, 0, 6, 4), "philox")


@pytest.mark.parametrize("E", [1, 6])
def test_one_workgroup(E):
    cfg = _cfg(10, "unicycle", E, seed={1: 1, 6: 0}[E])
    _check(cfg, actions_cpu(21, E, "unicycle", 5), lambda tr: premise_many_in_block(tr, GOAL_STEP, 0, E, min(E, 4)),
           "E %d" % E)


def test_twice_the_same():
    """Case 1 at chunk 32, twice: equal outputs and state (no dependence on which wave finishes first)."""
    cfg = _cfg(C1["N"], C1["kin"], C1["E"], seed=C1["seed"])
    acts = actions_cpu(21, C1["E"], C1["kin"], C1["aseed"]).to("cuda:0").contiguous()
    a = _run(cfg, acts, 32)
    b = _run(cfg, acts, 32)
    _same(b, a, "second run")
    ref, tr = _reference(cfg, acts)
    premise_many_in_block(tr, GOAL_STEP, 0, 6, 4)
    _same(a, ref, "first run against chunk 1")
