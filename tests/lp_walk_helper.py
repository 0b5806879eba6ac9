"""Host side of tests/test_lp_walk.py: RVO2's linearProgram2 restated in float32 with a record of what its loop did,
and the crafted simulators the test runs.

`trace()` solves agent 0 of one simulator with the float32 RVO2 stand-in of oracle/shims/rvo2.py (the ORCA lines, its
linearProgram1 and linearProgram3), but with linearProgram2 restated here so that it also returns, for the lines
the loop acted on (the lines the result violated when the loop reached them), their indices, and beside each one
the later lines its update made satisfied again or newly violated. test_lp_walk.py checks it against
oracle.cpu_ref (velocity bit for bit, and whether linearProgram2 failed) before it relies on any of that.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _shim():
    sys.path.insert(0, os.path.join(REPO, "oracle", "shims"))
    try:
        import rvo2
    finally:
        sys.path.pop(0)
    return rvo2


class Trace(object):
    """velocity (2 x float32), n lines, fail (the failing line, or n), acted (the line indices linearProgram2 ran
    linearProgram1 on, in order; the last one is `fail` when it failed), healed / hurt (later lines an update made
    satisfied again / newly violated), parallel (the failure was RVO2's parallel-line exit)."""


def _violated(rvo2, lines, result, lo):
    return {j for j in range(lo, len(lines)) if rvo2._det(lines[j][1], rvo2._sub(lines[j][0], result)) > rvo2.ZERO}


def _lp2_traced(rvo2, tr, lines, radius, optVelocity):
    """RVO2's linearProgram2 (directionOpt false), float32, recording into tr."""
    if rvo2._dot(optVelocity, optVelocity) > radius * radius:
        n = rvo2._normalize(optVelocity)
        result = (n[0] * radius, n[1] * radius)
    else:
        result = optVelocity
    tr.n, tr.acted, tr.healed, tr.hurt, tr.parallel = len(lines), [], set(), set(), False
    for i in range(len(lines)):
        point, direction = lines[i]
        if rvo2._det(direction, rvo2._sub(point, result)) > rvo2.ZERO:
            tr.acted.append(i)
            before = _violated(rvo2, lines, result, i + 1)
            temp = result
            ok, result = rvo2._lp1(lines, i, radius, optVelocity, False, result)
            if not ok:
                for j in range(i):   # the exit RVO2 took: parallel line j with a negative numerator?
                    den = rvo2._det(direction, lines[j][1])
                    num = rvo2._det(lines[j][1], rvo2._sub(point, lines[j][0]))
                    if abs(den) <= rvo2.RVO_EPSILON and num < rvo2.ZERO:
                        tr.parallel = True
                tr.fail = i
                return i, temp
            after = _violated(rvo2, lines, result, i + 1)
            tr.healed |= before - after
            tr.hurt |= after - before
    tr.fail = len(lines)
    return len(lines), result


def trace(agents, vmax, pref, dt):
    """orca.py's call sequence (neighborDist 10, timeHorizon 5, maxNeighbors A - 1) on agents [A][5] = x, y, vx, vy, r."""
    rvo2 = _shim()
    A = len(agents)
    sim = rvo2.PyRVOSimulator(dt, 10.0, max(A - 1, 1), 5.0, 5.0, 0.3, 1.0)
    for k, (x, y, vx, vy, r) in enumerate(agents):
        sim.addAgent((float(x), float(y)), 10.0, max(A - 1, 1), 5.0, 5.0, float(r), float(vmax) if k == 0 else 1.0,
                     (float(vx), float(vy)))
    sim.setAgentPrefVelocity(0, (float(pref[0]), float(pref[1])))
    tr = Trace()
    orig = rvo2._lp2

    def lp2(lines, radius, optVelocity, directionOpt, result):
        if directionOpt:
            return orig(lines, radius, optVelocity, directionOpt, result)
        return _lp2_traced(rvo2, tr, lines, radius, optVelocity)

    rvo2._lp2 = lp2
    try:
        sim.doStep()
    finally:
        rvo2._lp2 = orig
    v = sim.agents[0].velocity
    tr.velocity = np.array([v[0], v[1]], np.float32)
    return tr


def sim(agents, vmax, pref, dt=0.25):
    return (np.asarray(agents, np.float32), f32(vmax), np.asarray(pref, np.float32), dt)


def random_sim(rng, A):
    """A clustered simulator of A agents (as tests/test_orca_known_answers.py draws them), some with neighbours out
    of range (fewer lines than A - 1)."""
    spread = rng.choice([0.6, 1.5, 4.0])
    ag = np.zeros((A, 5), np.float32)
    ag[:, 0:2] = rng.uniform(-spread, spread, (A, 2))
    ag[:, 2:4] = rng.uniform(-1, 1, (A, 2))
    ag[:, 4] = rng.uniform(0.3, 0.6, A)
    if A > 2 and rng.rand() < 0.15:   # the last neighbours beyond neighborDist
        k = rng.randint(1, A)
        ag[k:, 0] = 30.0 + np.arange(A - k)
    return sim(ag, rng.uniform(0.5, 1.5), rng.uniform(-1.2, 1.2, 2))


def far_sim(A):
    """Every neighbour beyond neighborDist: no line."""
    ag = np.zeros((A, 5), np.float32)
    ag[1:, 0] = 20.0 + np.arange(A - 1)
    ag[:, 4] = 0.3
    return sim(ag, 1.0, (0.3, -0.2))


def parallel_fail_sim():
    """Agent 0 overlapped from both sides along x: lines x <= -0.2 and x >= 0.2, exactly antiparallel, so
    linearProgram1 on line 1 leaves by the parallel-line rule (|den| <= RVO_EPSILON, num < 0)."""
    return sim([(0, 0, 0, 0, 0.3), (0.5, 0, 0, 0, 0.3), (-0.5, 0, 0, 0, 0.3)], 1.0, (0.0, 0.0))


GOLDEN = os.path.join(REPO, "tests", "golden", "lp_walk_sims.npz")
MIXED_ROLES = ("none", "one", "five", "last_only", "first_only", "consecutive", "healed", "hurt", "fail_first",
               "fail_last")


def role(tr):
    """The roles (MIXED_ROLES) a traced simulator can play in the mixed batch."""
    a, n, ok = tr.acted, tr.n, tr.fail == tr.n
    r = set()
    if n >= 1 and not a: r.add("none")
    if ok and len(a) == 1: r.add("one")
    if len(a) >= 5: r.add("five")
    if ok and n >= 2 and a == [n - 1]: r.add("last_only")
    if ok and n >= 2 and a == [0]: r.add("first_only")
    if any(j == i + 1 for i, j in zip(a, a[1:])): r.add("consecutive")
    if tr.healed: r.add("healed")
    if tr.hurt: r.add("hurt")
    if not ok and a == [tr.fail] and tr.fail < n - 1: r.add("fail_first")
    if not ok and tr.fail == n - 1 and len(a) >= 2: r.add("fail_last")
    return r


def pack(sims):
    return (np.stack([s[0] for s in sims]), np.array([s[1] for s in sims], np.float32),
            np.stack([s[2] for s in sims]).astype(np.float32))


def unpack(ag, vmax, pref):
    return [sim(ag[k], vmax[k], pref[k]) for k in range(len(ag))]


def generate(path=GOLDEN, seed=7, pool=1500):
    """Draws the batches of tests/test_lp_walk.py and writes them to tests/golden/lp_walk_sims.npz
    (python tests/lp_walk_helper.py): `count<A>`, 17 simulators of A agents (the last one without a neighbour in
    range), A = 2..10, and `mixed`, 64 simulators of 10 agents whose first 16 (one wave) start with a quad that acts
    on no line, on one, and on five or more, followed by one simulator per further role of MIXED_ROLES, found in a
    pool of random ones. The test asserts every role again from its own trace of what it loaded."""
    rng = np.random.RandomState(seed)
    out = {}
    for A in range(2, 11):
        b = [random_sim(rng, A) for _ in range(16)]
        b[0][0][1:, 0:2] = rng.uniform(-1.0, 1.0, (A - 1, 2))   # every neighbour in range: A - 1 lines
        out["count%d" % A] = b + [far_sim(A)]
    found, rest = {}, []
    for _ in range(pool):
        s = random_sim(rng, 10)
        new = [r for r in MIXED_ROLES if r in role(trace(*s)) and r not in found]
        if new:
            found[new[0]] = s
        elif len(rest) < 64:
            rest.append(s)
        if len(found) == len(MIXED_ROLES) and len(rest) >= 64:
            break
    missing = [r for r in MIXED_ROLES if r not in found]
    assert not missing, missing
    out["mixed"] = ([found[r] for r in MIXED_ROLES] + rest)[:64]
    flat = {}
    for k, b in out.items():
        flat[k + "_ag"], flat[k + "_vmax"], flat[k + "_pref"] = pack(b)
    np.savez_compressed(path, **flat)
    return out


def load(path=GOLDEN):
    d = np.load(path)
    names = sorted({k.rsplit("_", 1)[0] for k in d.files})
    return {n: unpack(d[n + "_ag"], d[n + "_vmax"], d[n + "_pref"]) for n in names}


if __name__ == "__main__":
    for name, b in sorted(generate().items()):
        print(name, len(b), "simulators of", len(b[0][0]), "agents")
