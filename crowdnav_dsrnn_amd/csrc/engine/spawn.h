// spawn.h -- the pending-spawn slots, spawn_env with its rejection tests, reset_env, the goal changes (goal_pass,
// goal_changes) and the spawning waves (pend_waves). Needs plan.h, stamps.h, geometry.h and rng.h.
#pragma once

// ------------------------------------------------------------------------------------------------
// RNG work (goal changes, spawn): numpy legacy MT19937 per env, one wave per env
// ------------------------------------------------------------------------------------------------
// Pending next-episode spawns. CrowdSimDict.reset (crowd_sim_dict.py:105-203) is a pure function of the
// seed schedule (offset + case_counter + thisSeed) and the scenario, both fixed as soon as the previous
// reset has run, so the spawn of env e's NEXT episode is drawn ahead of time by spare waves of kernel A
// (off the critical path) and kernel B's auto-reset only copies it. (case_counter, reset_count) is
// the validity key: a stale entry (e.g. after cn_set_state) is never used, the reset is then drawn inline.
// Two slots per env (slot = reset_count & 1): the spawn of the env's next reset and of the one after, so
// an env that ends an episode one step after a reset (common where spawns overlap, e.g. 25 humans in
// square_crossing) finds its spawn drawn instead of drawing it inline. Arrays are [2][...].
struct PendPtrs {
    uint32_t *mt;   // [E][624] key words after the spawn draws
    int32_t *pos;   // [E] stream position
    uint32_t *ovf;  // [E] bounded-rejection overflows of the spawn
    int32_t *sc;    // [E] scenario
    int64_t *cc;    // [E] key: case_counter the spawn was drawn for
    int32_t *rc;    // [E] key: reset_count (sequential scenario mode)
    uint64_t *ok;   // [E] (reset_count key << 32) | id of the launch that completed the entry (0: parked / none);
                    // one 8-byte store, written last: consumed only by a LATER launch, and only for its own key
    int32_t *prog;  // [E] humans placed so far by a spawn parked mid-way (resumable spawns)
    double *r;      // [5][E] robot px, py, gx, gy, theta
    double *h;      // [7][E*N] human px, py, gx, gy, radius, v_pref, theta
};
__host__ __device__ inline PendPtrs pend_slot(const PendPtrs &P, int s, int64_t E, int64_t EN)
{
    PendPtrs q = P;
    q.mt += s * E * CN_MT_N; q.pos += s * E; q.ovf += s * E; q.sc += s * E; q.cc += s * E; q.rc += s * E;
    q.ok += s * E; q.prog += s * E; q.r += s * 5 * E; q.h += s * 7 * EN;
    return q;
}

// Output view of a group engine inside a mixed engine (cn_create_mixed): local env e of
// the group is row `row[e]` of the caller's (E_total, ...) buffers, whose spatial_edges have NS human
// slots (NS >= N; slots N..NS-1 are padding). row == nullptr: identity, NS == N (a plain engine).
struct OutView {
    const int32_t *row;
    int NS;
};
__device__ __forceinline__ int64_t orow(const OutView &v, int64_t e) { return v.row ? (int64_t)v.row[e] : e; }
// padding slot of a mixed engine's spatial_edges: a human that is never seen, i.e. the belief the
// reference gives an unseen human at reset (crowd_sim.py:437-455: [15, 15, 0, 0, 0.3], zero velocity, so
// it never moves), relative to the robot
#define CN_PAD_POS 15.0

// where a reset writes: state + the first observation of the new episode
struct ResetOut {
    cn_state_ptrs s;
    float *robot_node, *temporal, *spatial;
    int64_t case_size;
    OutView ov;
};

// pending-spawn modes of a step launch (PendLaunch::all): after cn_set_state every env's next spawn and the one
// after are drawn (resets of that launch draw inline); after cn_reset the reset kernel drew both (ok word
// CN_OK_RESET, never a step launch's id) and the launch draws none -- both modes ignore the spawn and resume
// lists of launches before them
#define PEND_BOTH 1
#define PEND_FRESH 2
#define CN_OK_RESET 0xffffffffu

struct RngArgs {   // cn_reset_kernel
    ResetOut o;
    PendPtrs pend;
    int E;
    int64_t counter_offset;
    int draw_next;   // also draw the spawns of every env's next two resets (then PEND_FRESH); cn_reset always sets it
};

// words one try of create_agent_attributes(scenario) consumes (crowd_sim.py:296-357)
__host__ __device__ inline int cand_words(int scenario)
{
    switch (scenario) {
    case CN_SC_CIRCLE_CROSSING: return 6;
    case CN_SC_SQUARE_CROSSING: return 12;
    case CN_SC_PARALLEL_TRAFFIC: case CN_SC_PERPENDICULAR_TRAFFIC: return 10;
    default: return 6;
    }
}

// create_agent_attributes from the words starting at q
template <typename Src>
__device__ void cand_attributes(const cn_config &c, const Src &w, int q, int scenario, double agent_vpref,
                                double agent_radius, double robot_radius, double &px, double &py, double &gx,
                                double &gy, double &heading, double &vp)
{
    double v_pref = agent_vpref == 0 ? 1.0 : agent_vpref;
    const double pxn = (w.dbl(q) - 0.5) * v_pref;
    const double pyn = (w.dbl(q + 2) - 0.5) * v_pref;
    q += 4;
    const double R = c.circle_radius;
    auto rwp = [&](int qq) { return (w.dbl(qq) - 0.5) * c.square_width / 2; };
    heading = 0;
    switch (scenario) {
    case CN_SC_CIRCLE_CROSSING:
        px = R * w.cos2pi(q) + pxn; py = R * w.sin2pi(q) + pyn;
        gx = -px; gy = -py;
        break;
    case CN_SC_SQUARE_CROSSING:
        px = rwp(q) * 0.4 + pxn;
        py = rwp(q + 2) * 0.4 + pyn;
        gx = rwp(q + 4) * 0.4 + pxn;
        gy = rwp(q + 6) * 0.4 + pyn;
        break;
    case CN_SC_PARALLEL_TRAFFIC: {
        const double sign = w.dbl(q) >= 0.5 ? 1 : -1;
        px = rwp(q + 2) * 0.4 + pxn;
        py = sign * (w.dbl(q + 4) * 3 + 1 + pyn);
        gx = px; gy = -py;
    } break;
    case CN_SC_PERPENDICULAR_TRAFFIC: {
        const double sign = w.dbl(q) >= 0.5 ? 1 : -1;
        px = sign * (w.dbl(q + 2) * 3 + 1 + pxn);
        gx = -px;
        py = rwp(q + 4) * 0.4 + pyn;
        gy = py;
    } break;
    case CN_SC_SIDE_PREF_PASSING:
    case CN_SC_SIDE_PREF_OVERTAKING: {
        const double min_x = -(robot_radius + agent_radius), max_x = -min_x;
        const double hx = (max_x - min_x) * w.dbl(q) + min_x;
        px = hx; gx = hx;
        if (scenario == CN_SC_SIDE_PREF_PASSING) { py = R; gy = -R; heading = -CN_PI / 2; }
        else { py = -R + 2; gy = R + 2; heading = CN_PI / 2; v_pref = 0.3; }
    } break;
    default: {
        const double min_x = -(R + robot_radius + agent_radius), max_x = -(R - robot_radius - agent_radius);
        const double hx = (max_x - min_x) * w.dbl(q) + min_x;
        px = hx; gx = -hx; py = 0; gy = 0;
    } break;
    }
    vp = v_pref;
}

struct Env1 {  // one env's agents in LDS (kernel B)
    double rpx, rpy, rgx, rgy, rr;
    double *hpx, *hpy, *hgx, *hgy, *hr, *hvp, *hth;  // [N]
};

// One agent test of the goal rejection loops (crowd_sim.py:744-760, 792-806): does goal candidate
// (gx, gy) of human `self` (radius r_self) come within r_self + r_agent + discomfort_dist of agent a's
// position or goal? a = 0 is the robot, a >= 1 the other humans in index order (self skipped).
__device__ __forceinline__ bool goal_hit(const cn_config &c, const Env1 &en, int self, double r_self, double gx,
                                         double gy, int a)
{
    double ax, ay, agx, agy, ar;
    if (a == 0) { ax = en.rpx; ay = en.rpy; agx = en.rgx; agy = en.rgy; ar = en.rr; }
    else {
        const int j = a - 1 < self ? a - 1 : a;
        ax = en.hpx[j]; ay = en.hpy[j]; agx = en.hgx[j]; agy = en.hgy[j]; ar = en.hr[j];
    }
    const double md = r_self + ar + c.discomfort_dist;
    return norm_lt(gx - ax, gy - ay, md) || norm_lt(gx - agx, gy - agy, md);
}

// Rejection loop of the reference (`while True: draw; if not collide: break`), speculative over the
// wave. Each try consumes W words, so try t's words start at p + W*t. The first pass spreads the tries
// AND the agent tests: lane = (try t, agent a), t = lane / NA, a = lane % NA, J = 64 / NA tries; later
// passes (crowded scenes, where early tries keep failing) put one try per lane, 64 per pass, each lane
// testing the agents in turn. `cand(q, t)` leaves try t's candidate in slot t of m.sl; `hit(t, a)` is
// one agent test (true = collision). The first try without a hit wins, as in the reference. Bounded by
// max_tries (the reference loops forever; after max_tries the last try is accepted and `ovf` counts
// it). Returns the winning slot; m.p is after its words.
template <typename FC, typename FT>
__device__ int wave_reject2(WRng &m, int W, int NA, int max_tries, uint32_t &ovf, FC cand, FT hit)
{
    const int lane = m.lane;
    const uint64_t gmask = NA >= 64 ? ~0ull : ((1ull << NA) - 1ull);
    int t0 = 0;
    {   // first pass, lane = (try, agent): the common case (an early try is accepted) in one short pass
        const int J = min(64 / NA, CN_MT_N / W);
        const int t = lane / NA, a = lane - t * NA;
        m.ensure(W * J);
        const int nt = min(J, max_tries);
        const bool valid = t < nt;
        if (valid && a == 0) cand(m.p + W * t, t);
        wsync();
        const uint64_t badm = __ballot(valid && hit(t, a));
        for (int k = 0; k < nt; ++k)
            if (((badm >> (k * NA)) & gmask) == 0) { m.p += W * (k + 1); return k; }
        if (J >= max_tries) { m.p += W * nt; ++ovf; return nt - 1; }
        m.p += W * J;
        t0 = J;
        wsync();
    }
    // crowded: lane = try (64 per pass), each lane tests the agents in turn
    const int J = min(64, CN_MT_N / W);
    for (;; t0 += J) {
        m.ensure(W * J);
        const int nt = min(J, max_tries - t0);
        const bool valid = lane < nt;
        if (valid) cand(m.p + W * lane, lane);
        wsync();
        bool bad = !valid;
        for (int a = 0; a < NA && !bad; ++a) bad = hit(lane, a);
        const uint64_t okm = __ballot(!bad);
        if (okm) {
            const int first = __ffsll((long long)okm) - 1;
            m.p += W * (first + 1);
            return first;
        }
        if (t0 + J >= max_tries) { m.p += W * nt; ++ovf; return nt - 1; }
        m.p += W * J;
        wsync();   // slots are rewritten by the next pass
    }
}

// Binned disc test for the crowded passes of the spawn's rejection loops (wave_reject_discs): a try is
// rejected iff its point lies strictly inside one of the agents' discs; the discs except agent 0's (the
// robot, often far from the crowd, tested exactly) are binned once per call into a 16 x 16 grid over their
// bounding box (4 cells per lane, float32 with a 1e-4 m margin, so the binning is conservative): a cell
// lying inside some disc rejects every try that lands in it, a try outside the box hits nothing, and
// otherwise only the agents overlapping its cell are tested exactly (norm_lt). Same result as testing
// every agent. The crowded goal rejection (goal_reject_crowded<GRID>) uses it on the kd-tree path only
// (the quad path's scenes are sparse and its code stays smaller).
struct DiscGrid {
    uint32_t *mask;   // [256] per cell: bit a = agent a's position or goal disc overlaps the cell (NA <= 32)
    uint64_t *cov;    // [4] bit = cell entirely inside some disc
    double *par;      // x0, y0, 16 / width, 16 / height
};

template <bool GOALS = true>
__device__ __forceinline__ void disc_grid_build(const DiscGrid &gr, const double *tx, const double *ty, const double *tgx,
                                                const double *tgy, const double *tmd, int NA, int lane)
{
    // bounding box of every disc (wave-uniform: each lane scans the table)
    // agent 0 (the robot, often far from the crowd) stays out of the grid: disc_grid_hit tests it exactly
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int a = 1; a < NA; ++a) {
        const double d = tmd[a] + 1e-3;
        const double ax = tx[a], ay = ty[a], bx = GOALS ? tgx[a] : ax, by = GOALS ? tgy[a] : ay;
        x0 = fmin(x0, fmin(ax, bx) - d); x1 = fmax(x1, fmax(ax, bx) + d);
        y0 = fmin(y0, fmin(ay, by) - d); y1 = fmax(y1, fmax(ay, by) + d);
    }
    const double ivx = CN_GRID / (x1 - x0), ivy = CN_GRID / (y1 - y0);
    // cells lane + 64 j (j < 4): column lane & 15, row 4 j + lane / 16; each expanded by 1e-4 m (a try is
    // binned in double precision; near a cell edge it may land in the neighbour, which the expansion covers)
    const float m = 1e-4f;
    const int ix = lane & 15;
    const float cx0 = (float)(x0 + ix / ivx) - m, cx1 = (float)(x0 + (ix + 1) / ivx) + m;
    float cy0[4], cy1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int iy = 4 * j + (lane >> 4);
        cy0[j] = (float)(y0 + iy / ivy) - m; cy1[j] = (float)(y0 + (iy + 1) / ivy) + m;
    }
    uint32_t msk[4] = {0u, 0u, 0u, 0u};
    bool covered[4] = {false, false, false, false};
    for (int a = 1; a < NA; ++a) {
        const float d = (float)tmd[a], dl = d + m, ds = d - m;
#pragma unroll
        for (int g = 0; g < (GOALS ? 2 : 1); ++g) {
            const float px = (float)(g ? tgx[a] : tx[a]), py = (float)(g ? tgy[a] : ty[a]);
            const float nx = fmaxf(0.0f, fmaxf(cx0 - px, px - cx1));
            const float fx = fmaxf(fabsf(px - cx0), fabsf(px - cx1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ny = fmaxf(0.0f, fmaxf(cy0[j] - py, py - cy1[j]));
                const float fy = fmaxf(fabsf(py - cy0[j]), fabsf(py - cy1[j]));
                if (nx * nx + ny * ny <= dl * dl) msk[j] |= 1u << a;
                if (ds > 0.0f && fx * fx + fy * fy < ds * ds) covered[j] = true;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gr.mask[lane + 64 * j] = msk[j];
        const uint64_t cv = __ballot(covered[j]);
        if (lane == 0) gr.cov[j] = cv;
    }
    if (lane == 0) { gr.par[0] = x0; gr.par[1] = y0; gr.par[2] = ivx; gr.par[3] = ivy; }
}

// does the goal (gx, gy) lie strictly inside one of the discs? Exact tests (norm_lt) of the agents
// binned in its cell, two agents (four discs) per round with their loads issued together
template <bool GOALS = true>
__device__ __forceinline__ bool disc_grid_hit(const DiscGrid &gr, const double *tx, const double *ty, const double *tgx,
                                              const double *tgy, const double *tmd, double gx, double gy)
{
    if (norm_lt(gx - tx[0], gy - ty[0], tmd[0]) || (GOALS && norm_lt(gx - tgx[0], gy - tgy[0], tmd[0]))) return true;
    const double fx = (gx - gr.par[0]) * gr.par[2], fy = (gy - gr.par[1]) * gr.par[3];
    if (!(fx >= 0.0 && fx < CN_GRID && fy >= 0.0 && fy < CN_GRID)) return false;   // outside every other disc
    const int cell = (int)fy * CN_GRID + (int)fx;
    if ((gr.cov[cell >> 6] >> (cell & 63)) & 1ull) return true;
    uint32_t msk = gr.mask[cell];
    bool hit = false;
    while (msk && !hit) {
        const int a0 = __ffs(msk) - 1;
        msk &= msk - 1;
        const int a1 = msk ? __ffs(msk) - 1 : a0;
        msk &= msk - 1;
        const double x0 = tx[a0], y0 = ty[a0], d0 = tmd[a0];
        const double x1 = tx[a1], y1 = ty[a1], d1 = tmd[a1];
        hit = norm_lt(gx - x0, gy - y0, d0) | norm_lt(gx - x1, gy - y1, d1);
        if (GOALS) {
            const double u0 = tgx[a0], v0 = tgy[a0], u1 = tgx[a1], v1 = tgy[a1];
            hit = hit | norm_lt(gx - u0, gy - v0, d0) | norm_lt(gx - u1, gy - v1, d1);
        }
    }
    return hit;
}

// Cover of a crowded rejection loop's candidate box (kd-tree path: square_crossing end goals and random goals
// on the circle in goal_reject_crowded, square_crossing spawn positions in wave_reject_discs): the box
// [-hb, hb]^2 that holds every candidate (0.4 * rand_world_pt + noise, crowd_sim.py:313-318; R cos / sin +
// noise, :736-741) in CN_GC x CN_GC
// cells. Per row of cells, `cov` has bit i set where cell i lies inside ONE of the agents' position / goal
// discs (so every try landing there is rejected); `arow` / `acol` are the agents whose discs' bounding boxes
// overlap the row / column strip, so a try in an uncovered cell tests only the agents of arow & acol
// exactly. Built per loop in one short pass (lane = row strip x half of the agents), unlike DiscGrid over the
// discs' bounding box, whose ~0.45 m cells left ~30 % of the tries to the exact test (~2 % here).
#define CN_GC 32
struct GoalCover {
    uint32_t *cov, *arow, *acol;   // [CN_GC] each
    double *par;                   // x0 (= y0), CN_GC / (2 hb)
};

// Built in float32 with a 1e-4 m margin on both the cells (expanded) and the discs (shrunk for coverage,
// grown for overlap), so no rounding of the build can mark a cell that the exact test (norm_lt, f64) would
// not reject everywhere: a try is binned in float64 (at most ~1e-14 m off its cell), float32 coordinates
// are ~1e-6 m off, and a cell can only be covered where the chord half-width w > s / 2 = 0.08 m, where
// sqrtf is well conditioned.
template <bool GOALS = true>
__device__ __forceinline__ void goal_cover_build(const GoalCover &gc, const double *tx, const double *ty,
                                                 const double *tgx, const double *tgy, const double *tmd, int NA,
                                                 double hb, int lane)
{
    const double sd = 2 * hb / CN_GC;
    const int r = lane & (CN_GC - 1), half = lane >> 5;
    const float m = 1e-4f, x0 = (float)-hb, inv = (float)(CN_GC / (2 * hb));
    const float s0 = (float)(-hb + r * sd) - m, s1 = (float)(-hb + (r + 1) * sd) + m;   // strip r, expanded
    uint32_t cov = 0u, arow = 0u, acol = 0u;
    for (int a = half; a < NA; a += 2) {
        const float d = (float)tmd[a], dl = d + m, ds = d - m;
#pragma unroll
        for (int g = 0; g < (GOALS ? 2 : 1); ++g) {
            const float cx = (float)(g ? tgx[a] : tx[a]), cy = (float)(g ? tgy[a] : ty[a]);
            if (cy + dl >= s0 && cy - dl <= s1) arow |= 1u << a;
            if (cx + dl >= s0 && cx - dl <= s1) acol |= 1u << a;
            const float dy = fmaxf(fabsf(s0 - cy), fabsf(s1 - cy));   // farthest point of the strip in y
            if (ds > dy) {
                const float w = sqrtf(ds * ds - dy * dy);
                // cells i with [x0 + i s - m, x0 + (i + 1) s + m] inside (cx - w, cx + w)
                const int lo = max((int)floorf((cx - w - x0 + m) * inv) + 1, 0);
                const int hi = min((int)floorf((cx + w - x0 - m) * inv) - 1, CN_GC - 1);
                if (lo <= hi) cov |= (hi - lo == 31 ? ~0u : ((1u << (hi - lo + 1)) - 1u)) << lo;
            }
        }
    }
    cov |= __shfl_xor(cov, 32); arow |= __shfl_xor(arow, 32); acol |= __shfl_xor(acol, 32);
    if (lane < CN_GC) { gc.cov[lane] = cov; gc.arow[lane] = arow; gc.acol[lane] = acol; }
    if (lane == 0) { gc.par[0] = -hb; gc.par[1] = CN_GC / (2 * hb); }
}

// does the goal (gx, gy) lie strictly inside one of the agents' discs? Same answer as goal_hit over every
// agent (GOALS = false: the position discs only, the spawn's placement test)
template <bool GOALS = true>
__device__ __forceinline__ bool goal_cover_hit(const GoalCover &gc, const double *tx, const double *ty,
                                               const double *tgx, const double *tgy, const double *tmd, int NA,
                                               double gx, double gy)
{
    const double fx = (gx - gc.par[0]) * gc.par[1], fy = (gy - gc.par[0]) * gc.par[1];
    uint32_t msk;
    if (fx >= 0.0 && fx < CN_GC && fy >= 0.0 && fy < CN_GC) {
        const int ix = (int)fx, iy = (int)fy;
        if ((gc.cov[iy] >> ix) & 1u) return true;
        msk = gc.arow[iy] & gc.acol[ix];
    } else msk = NA >= 32 ? ~0u : (1u << NA) - 1u;   // outside the box (not reached by its candidates)
    bool hit = false;
    while (msk && !hit) {
        const int a0 = __ffs(msk) - 1;
        msk &= msk - 1;
        const int a1 = msk ? __ffs(msk) - 1 : a0;
        msk &= msk - 1;
        const double x0 = tx[a0], y0 = ty[a0], d0 = tmd[a0];
        const double x1 = tx[a1], y1 = ty[a1], d1 = tmd[a1];
        hit = norm_lt(gx - x0, gy - y0, d0) | norm_lt(gx - x1, gy - y1, d1);
        if (GOALS) {
            const double u0 = tgx[a0], v0 = tgy[a0], u1 = tgx[a1], v1 = tgy[a1];
            hit = hit | norm_lt(gx - u0, gy - v0, d0) | norm_lt(gx - u1, gy - v1, d1);
        }
    }
    return hit;
}

// wave_reject2 for "the candidate point (m.sl[t], m.sl[64 + t]) lies strictly inside one of NA discs"
// (`disc(a, x, y, md)`: centre and radius of agent a): the spawn's human placement (crowd_sim.py:369-390).
// When the wave has grid space (m.grid) the crowded passes bin the discs once into a DiscGrid (see
// goal_reject_crowded) and test each try against its cell's agents only; same result.
template <bool GRID, typename FC, typename FD>
__device__ int wave_reject_discs(WRng &m, int W, int NA, int max_tries, uint32_t &ovf, FC cand, FD disc, double hb = 0.0)
{
    auto hit = [&](int t, int a) {
        double x, y, md;
        disc(a, x, y, md);
        return norm_lt(m.sl[t] - x, m.sl[64 + t] - y, md);
    };
    if (!GRID || !m.grid || NA < 8) return wave_reject2(m, W, NA, max_tries, ovf, cand, hit);
    const int lane = m.lane;
    const uint64_t gmask = NA >= 64 ? ~0ull : ((1ull << NA) - 1ull);
    int t0 = 0;
    {   // first pass, lane = (try, agent), as wave_reject2
        const int J = min(64 / NA, CN_MT_N / W);
        const int t = lane / NA, a = lane - t * NA;
        m.ensure(W * J);
        const int nt = min(J, max_tries);
        const bool valid = t < nt;
        if (valid && a == 0) cand(m.p + W * t, t);
        wsync();
        const uint64_t badm = __ballot(valid && hit(t, a));
        for (int k = 0; k < nt; ++k)
            if (((badm >> (k * NA)) & gmask) == 0) { m.p += W * (k + 1); return k; }
        if (J >= max_tries) { m.p += W * nt; ++ovf; return nt - 1; }
        m.p += W * J;
        t0 = J;
    }
    double *tx = (double *)m.grid, *ty = tx + 32, *tmd = tx + 64;
    DiscGrid gr;
    GoalCover gc;
    const bool cover = hb > 0.0 && NA <= 32;   // a candidate box: cover it (see GoalCover) instead of the discs' box
    gr.mask = (uint32_t *)(tx + 96); gr.cov = (uint64_t *)(tx + 96 + CN_GRID * CN_GRID / 2); gr.par = (double *)(gr.cov + 4);
    gc.cov = (uint32_t *)(tx + 96); gc.arow = gc.cov + CN_GC; gc.acol = gc.arow + CN_GC; gc.par = (double *)(gc.acol + CN_GC);
    if (lane < NA) { double x, y, md; disc(lane, x, y, md); tx[lane] = x; ty[lane] = y; tmd[lane] = md; }
    wsync();
    if (cover) goal_cover_build<false>(gc, tx, ty, tx, ty, tmd, NA, hb, lane);
    else disc_grid_build<false>(gr, tx, ty, tx, ty, tmd, NA, lane);
    const int J = min(64, CN_MT_N / W);
    for (;; t0 += J) {
        m.template ensure<true>(W * J);
        const int nt = min(J, max_tries - t0);
        const bool valid = lane < nt;
        if (valid) cand(m.p + W * lane, lane);
        wsync();
        const bool bad = !valid || (cover ? goal_cover_hit<false>(gc, tx, ty, tx, ty, tmd, NA, m.sl[lane], m.sl[64 + lane])
                                          : disc_grid_hit<false>(gr, tx, ty, tx, ty, tmd, m.sl[lane], m.sl[64 + lane]));
        const uint64_t okm = __ballot(!bad);
        if (okm) {
            const int first = __ffsll((long long)okm) - 1;
            m.p += W * (first + 1);
            return first;
        }
        if (t0 + J >= max_tries) { m.p += W * nt; ++ovf; return nt - 1; }
        m.p += W * J;
        wsync();   // slots are rewritten by the next pass
    }
}

// Crowded goal rejection (a goal pass whose first batch was all rejected; in square_crossing at N = 25
// most of these loops run to max_tries): one try per lane, 64 at a time, straight from the stream; the
// agents (robot, then the other humans in index order) sit in an LDS table with their minimum distance
// precomputed, and each lane tests them four at a time with the loads of a group issued together (the
// agent-at-a-time loop was bound by dependent LDS latency). Same result as goal_hit over the tries in
// order; returns the winning slot (m.sl[t], m.sl[64 + t]), m.p after its words.
// GRID (the kd-tree path, whose waves have DiscGrid space in m.grid): the position and goal discs of the
// agents are binned once per loop (disc_grid_build<true>) and each try tests only its cell's agents --
// at 25 humans in square_crossing most of these loops run all max_tries = 1000 tries (16 passes), so the
// one-off binning is repaid many times over; same result. With a candidate box (hb > 0: square_crossing's
// end goals) a GoalCover over the box replaces the DiscGrid.
template <bool GRID, typename FC>
__device__ int goal_reject_crowded(const cn_config &c, const Env1 &en, WRng &m, int self, double r_self, int W,
                                   int max_tries, uint32_t &ovf, FC cand, double hb = 0.0)
{
    const int lane = m.lane, NA = c.human_num;
    double *tx = m.sl + 128, *ty = tx + 32, *tgx = tx + 64, *tgy = tx + 96, *tmd = tx + 128;   // [32] each
    if (lane < NA) {
        double ar;
        if (lane == 0) { tx[0] = en.rpx; ty[0] = en.rpy; tgx[0] = en.rgx; tgy[0] = en.rgy; ar = en.rr; }
        else {
            const int j = lane - 1 < self ? lane - 1 : lane;
            tx[lane] = en.hpx[j]; ty[lane] = en.hpy[j]; tgx[lane] = en.hgx[j]; tgy[lane] = en.hgy[j]; ar = en.hr[j];
        }
        tmd[lane] = r_self + ar + c.discomfort_dist;
    }
    wsync();
    DiscGrid gr;
    GoalCover gc;
    const bool cover = GRID && m.grid && NA >= 8 && NA <= 32 && hb > 0.0;
    const bool grid = GRID && m.grid && NA >= 8 && !cover;
    if (cover) {
        gc.cov = (uint32_t *)(m.grid + 96 * 8);
        gc.arow = gc.cov + CN_GC; gc.acol = gc.arow + CN_GC;
        gc.par = (double *)(gc.acol + CN_GC);
        goal_cover_build<true>(gc, tx, ty, tgx, tgy, tmd, NA, hb, lane);
        wsync();
    }
    if (grid) {
        gr.mask = (uint32_t *)(m.grid + 96 * 8);
        gr.cov = (uint64_t *)(m.grid + 96 * 8 + CN_GRID * CN_GRID * 4);
        gr.par = (double *)(gr.cov + 4);
        disc_grid_build<true>(gr, tx, ty, tgx, tgy, tmd, NA, lane);
        wsync();
    }
    const int J = min(64, CN_MT_N / W);
#ifdef CN_STAMPS
    unsigned long long tq = clock64(), tc_e = 0, tc_c = 0, tc_t = 0, tc_n = 0;
#endif
    for (int t0 = 0;; t0 += J) {
        m.template ensure<true>(W * J);
#ifdef CN_STAMPS
        { const unsigned long long t_ = clock64(); tc_e += t_ - tq; tq = t_; ++tc_n; }
#endif
        const int nt = min(J, max_tries - t0);
        double gx = 0, gy = 0;
        if (lane < nt) {
            cand(m.p + W * lane, lane);
            gx = m.sl[lane]; gy = m.sl[64 + lane];
        }
        wsync();
#ifdef CN_STAMPS
        { const unsigned long long t_ = clock64(); tc_c += t_ - tq; tq = t_; }
#endif
        bool bad = lane >= nt;
        if (cover) bad = bad || goal_cover_hit<true>(gc, tx, ty, tgx, tgy, tmd, NA, gx, gy);
        else if (grid) bad = bad || disc_grid_hit<true>(gr, tx, ty, tgx, tgy, tmd, gx, gy);
        else
        for (int a0 = 0; a0 < NA && !bad; a0 += 4) {
            double x[4], y[4], u[4], v[4], d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int a = min(a0 + k, NA - 1);   // a repeated last agent does not change the outcome
                x[k] = tx[a]; y[k] = ty[a]; u[k] = tgx[a]; v[k] = tgy[a]; d[k] = tmd[a];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                bad = bad | norm_lt(gx - x[k], gy - y[k], d[k]) | norm_lt(gx - u[k], gy - v[k], d[k]);
        }
#ifdef CN_STAMPS
        { const uint64_t bb_ = __ballot(bad); (void)bb_; const unsigned long long t_ = clock64(); tc_t += t_ - tq; tq = t_;
          if (lane == 0 && m.edbg >= 0 && m.edbg < 8192) { cn_stamp_c[m.edbg * 4] += tc_e; cn_stamp_c[m.edbg * 4 + 1] += tc_c; cn_stamp_c[m.edbg * 4 + 2] += tc_t; cn_stamp_c[m.edbg * 4 + 3] += 1; }
          tc_e = tc_c = tc_t = 0; }
#endif
        const uint64_t okm = __ballot(!bad);
        if (okm) {
            const int first = __ffsll((long long)okm) - 1;
            m.p += W * (first + 1);
            return first;
        }
        if (t0 + nt >= max_tries) { m.p += W * nt; ++ovf; return nt - 1; }
        m.p += W * J;
        wsync();   // slots are rewritten by the next batch
    }
}

// The random part of CrowdSimDict.reset (crowd_sim_dict.py:110-156; generate_robot_humans,
// crowd_sim.py:555-663; generate_circle_crossing_human :359-393): reseed the env's stream with
// counter_offset + case_counter + thisSeed, draw the robot and then each human with rejection.
// One wave; the result is left in `en` (LDS), rth, ovf, sc and the stream `m`.
// Resumable (spare-workgroup spawns): i0 > 0 continues a spawn parked after its first i0 humans -- the
// caller restored the stream, the robot, rth, ovf, sc and those humans -- and with a `deadline` (clock64
// value, 0 = none) the spawn parks itself before a human once the deadline has passed (at least one
// human per call). Returns the number of humans placed (N = complete).
template <bool GRID>
__device__ __forceinline__ int spawn_env(const cn_config &c, int64_t gidx, int64_t case_counter, int32_t reset_count,
                          int64_t counter_offset, WRng &m, Env1 &en, double &rth, uint32_t &ovf, int &sc,
                          int i0 = 0, long long deadline = 0)
{
    const int lane = m.lane;
    const int N = c.human_num;
    const double R = c.circle_radius;
    const int W0 = i0;
    STAMP_S(gidx, 0);
    if (i0 == 0) {
    uint32_t *mtw = m.w;
    m.off = 0;   // a fresh stream: the key at the start of the ring
    if (c.scenario_mode == CN_SCMODE_SEQUENTIAL) sc = c.scenarios[reset_count % c.num_scenarios];
    else sc = c.scenarios[gidx % c.num_scenarios];
    const uint32_t seed0 = (uint32_t)(counter_offset + case_counter + (c.seed + gidx));
    if (m.phx) {
        if (lane == 0) mtw[0] = seed0;   // the key is the whole stream state (written back with the reset)
        m.key = seed0;
        m.p = 0;
    } else {
        // mt19937_seed: the sequential Knuth chain, wave-uniform so it runs on the scalar unit (s_mul_i32 /
        // s_xor / s_lshr: a few cycles per word instead of a quarter-rate v_mul_lo_u32 chain on one lane);
        // word j*64 + k is dropped into lane k of a VGPR (v_writelane) and each lane stores its word
        uint32_t seed = __builtin_amdgcn_readfirstlane(seed0);
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) {
            int mine = 0;
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                asm("v_writelane_b32 %0, %1, %2" : "+v"(mine) : "s"(seed), "n"(k));
                seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)(j * 64 + k + 1);
            }
            if (j * 64 + lane < CN_MT_N) mtw[j * 64 + lane] = (uint32_t)mine;
        }
        m.p = CN_MT_N;   // numpy: pos = 624 after seeding, the first draw runs mt19937_gen
    }
    wsync();
    STAMP_S(gidx, 1);
    m.have1 = false; m.slid = false;
    ovf = 0;
    en.rr = c.robot_radius;
    if (c.kinematics == CN_UNICYCLE) {
        const double angle = m.unif(0, CN_PI * 2);
        en.rpx = R * cos(angle); en.rpy = R * sin(angle);
        // goal: uniform in the square until >= 6 m away (crowd_sim.py:620-634)
        const int tw = wave_reject2(m, 4, 1, c.max_tries, ovf, [&](int q, int t) {
            m.sl[t] = -R + (R - -R) * m.dbl(q); m.sl[64 + t] = -R + (R - -R) * m.dbl(q + 2);
        }, [&](int t, int) { return norm_lt(en.rpx - m.sl[t], en.rpy - m.sl[64 + t], 6.0); });
        en.rgx = m.sl[tw]; en.rgy = m.sl[64 + tw];
        wsync();
        rth = m.unif(0, 2 * CN_PI);
    } else if (c.social_metrics || c.side_preference) {
        en.rpx = 0; en.rpy = -R; en.rgx = 0; en.rgy = R; rth = CN_PI / 2;
    } else {
        // holonomic robot: start and goal uniform in the square until >= 6 m apart (crowd_sim.py:652-660)
        const int tw = wave_reject2(m, 8, 1, c.max_tries, ovf, [&](int q, int t) {
            m.sl[t] = -R + (R - -R) * m.dbl(q); m.sl[64 + t] = -R + (R - -R) * m.dbl(q + 2);
            m.sl[128 + t] = -R + (R - -R) * m.dbl(q + 4); m.sl[192 + t] = -R + (R - -R) * m.dbl(q + 6);
        }, [&](int t, int) { return norm_lt(m.sl[t] - m.sl[128 + t], m.sl[64 + t] - m.sl[192 + t], 6.0); });
        en.rpx = m.sl[tw]; en.rpy = m.sl[64 + tw]; en.rgx = m.sl[128 + tw]; en.rgy = m.sl[192 + tw];
        wsync();
        rth = CN_PI / 2;
    }
    }   // i0 == 0
    STAMP_S(gidx, 2);
    const int W = cand_words(sc);
    for (int i = i0; i < N; ++i) {
        if (deadline && i > W0 && (long long)clock64() > deadline) return i;   // park (wave-uniform clock)
        double vpref = c.human_vpref, rad = c.human_radius;
        if (c.randomize_attributes) { vpref = m.unif(0.5, 1.5); rad = m.unif(0.3, 0.5); }
        // candidate vs the robot and the humans placed so far (crowd_sim.py:369-390): i + 1 agent tests
        const int tw = wave_reject_discs<GRID>(m, W, i + 1, c.max_tries, ovf, [&](int q, int t) {
            double px, py, gx, gy, hd, vp;
            cand_attributes(c, m, q, sc, vpref, rad, en.rr, px, py, gx, gy, hd, vp);
            m.sl[t] = px; m.sl[64 + t] = py; m.sl[128 + t] = gx; m.sl[192 + t] = gy; m.sl[256 + t] = hd;
            m.sl[320 + t] = vp;
        }, [&](int a, double &ax, double &ay, double &md) {
            if (a == 0) {
                ax = en.rpx; ay = en.rpy;
                md = c.kinematics == CN_UNICYCLE ? R / 2 : rad + en.rr + c.discomfort_dist;
            } else {
                ax = en.hpx[a - 1]; ay = en.hpy[a - 1];
                md = rad + en.hr[a - 1] + c.discomfort_dist;
            }
        }, sc == CN_SC_SQUARE_CROSSING ? 0.1 * c.square_width + 0.5 * fabs(vpref == 0 ? 1.0 : vpref) + 1e-3 : 0.0);
        if (lane == 0) {
            en.hpx[i] = m.sl[tw]; en.hpy[i] = m.sl[64 + tw]; en.hgx[i] = m.sl[128 + tw]; en.hgy[i] = m.sl[192 + tw];
            en.hth[i] = m.sl[256 + tw]; en.hvp[i] = m.sl[320 + tw]; en.hr[i] = rad;
        }
        wsync();
        if (i < 13) STAMP_S(gidx, 3 + i);
    }
    return N;
}

// Store a drawn spawn as env e's pending episode for the reset with key (cc, rc), slot rc & 1.
// okv: the completing launch's id, or 0 with `prog` = humans placed for a spawn parked mid-way (the
// stream at the park point, the robot and the first prog humans are stored; resumed by a later launch).
// FENCE: device-scope fences around the slot's handshake, the round-5 protocol (ok zeroed and fenced before a slot's
// new key; key, fence, ok on the reader's side, reset_env). On gfx950 each is buffer_wbl2 sc1 + buffer_inv sc1: a
// write-back AND invalidation of the XCD's whole L2, once per spawn written and per reset, so only cn_reset_kernel
// keeps them. A step launch needs none (round 6): the ok word, written last, carries the entry's key and the
// completing launch's id, which is all a reset of a later launch needs (reset_env)
template <bool FENCE>
__device__ __forceinline__ void write_pending(const PendPtrs &P2, const cn_config &c, int64_t E, int64_t e, const Env1 &en, double rth,
                              int sc, uint32_t ovf, const uint32_t *mt_src, int pos, int64_t cc, int32_t rc, int lane,
                              uint32_t okv, int prog)
{
    const int N = c.human_num;
    const PendPtrs P = pend_slot(P2, rc & 1, E, E * N);
    const int nk = c.rng_mode == CN_RNG_PHILOX ? 1 : CN_MT_N;   // key words to copy
    // Invalidate the slot before rewriting it, visible device-wide before any new payload or key store:
    // a reset of the same launch that reads the slot (reset_env: key, fence, then ok) and sees a new key
    // then sees ok == 0 (or this launch's id) and draws inline instead of reading a half-written payload.
    if (FENCE) {
        if (lane == 0) P.ok[e] = 0ull;
        __threadfence();
    }
    {
        uint32_t v[(CN_MT_N + 63) / 64];
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; v[j] = k < nk ? mt_src[k] : 0u; }
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; if (k < nk) P.mt[e * CN_MT_N + k] = v[j]; }
    }
    if (lane < prog) {
        const int64_t h = e * N + lane, EN = E * N;
        P.h[h] = en.hpx[lane]; P.h[EN + h] = en.hpy[lane]; P.h[2 * EN + h] = en.hgx[lane];
        P.h[3 * EN + h] = en.hgy[lane]; P.h[4 * EN + h] = en.hr[lane]; P.h[5 * EN + h] = en.hvp[lane];
        P.h[6 * EN + h] = en.hth[lane];
    }
    if (lane == 0) {
        P.r[e] = en.rpx; P.r[E + e] = en.rpy; P.r[2 * E + e] = en.rgx; P.r[3 * E + e] = en.rgy; P.r[4 * E + e] = rth;
        P.pos[e] = pos; P.ovf[e] = ovf; P.sc[e] = sc; P.cc[e] = cc; P.rc[e] = rc;
        P.prog[e] = okv ? 0 : prog;
    }
    if (FENCE) __threadfence();   // the whole entry before its ok word (release)
    if (lane == 0) P.ok[e] = ((uint64_t)(uint32_t)rc << 32) | okv;
}

// The deterministic rest of CrowdSimDict.reset (crowd_sim_dict.py:136-203): state of the new episode,
// case_counter advance, first observation. `mt_src` = key words after the spawn (LDS or pending buffer).
// OBS_OPT (the SEQ kernels): g.robot_node == nullptr means the first observation is not wanted (a later step of the
// same launch overwrites it)
template <bool OBS_OPT = false>
__device__ __forceinline__ void write_reset(const ResetOut &g, const cn_config &c, int64_t e, const Env1 &en, double rth, int sc,
                            uint32_t ovf, const uint32_t *mt_src, int pos, int lane)
{
    const bool obs = !OBS_OPT || g.robot_node != nullptr;
    const cn_state_ptrs &S = g.s;
    const int N = c.human_num;
    const int64_t hb = e * N;
    const double rpx = en.rpx, rpy = en.rpy;
    const int64_t orw = orow(g.ov, e);
    if (obs && lane >= N && lane < g.ov.NS) {
        g.spatial[(orw * g.ov.NS + lane) * 2] = (float)(CN_PAD_POS - rpx);
        g.spatial[(orw * g.ov.NS + lane) * 2 + 1] = (float)(CN_PAD_POS - rpy);
    }
    if (lane < N) {
        const int64_t h = hb + lane;
        const double px = en.hpx[lane], py = en.hpy[lane];
        S.h_px[h] = px; S.h_py[h] = py; S.h_gx[h] = en.hgx[lane]; S.h_gy[h] = en.hgy[lane];
        S.h_vx[h] = 0.0; S.h_vy[h] = 0.0; S.h_r[h] = en.hr[lane]; S.h_vpref[h] = en.hvp[lane];
        S.h_theta[h] = en.hth[lane];
        S.o_r[h] = 0.0f; S.o_vmax[h] = 0.0f; S.o_dmask[h] = 0u;
        // generate_ob(reset=True): robot velocity is 0 (ints) -> float64 FOV path
        const double th0 = c.kinematics == CN_HOLONOMIC ? 0.0 : rth;   // atan2(0, 0) = 0
        int v = c.robot_fov >= 2.0 * CN_PI ? vis360(isfinite(th0), rpx, rpy, px, py) : -1;
        if (v < 0) v = reset_fov_test(th0, rpx, rpy, px, py, c.robot_fov);
        double bpx, bpy, bvx, bvy, br;
        if (v) { bpx = px; bpy = py; bvx = 0; bvy = 0; br = en.hr[lane]; }
        else { bpx = 15.0; bpy = 15.0; bvx = 0.0; bvy = 0.0; br = 0.3; }
        S.b_px[h] = bpx; S.b_py[h] = bpy; S.b_vx[h] = bvx; S.b_vy[h] = bvy; S.b_r[h] = br;
        if (obs) {
            g.spatial[(orw * g.ov.NS + lane) * 2] = (float)(bpx - rpx);
            g.spatial[(orw * g.ov.NS + lane) * 2 + 1] = (float)(bpy - rpy);
        }
    }
    const int A = N + (c.robot_visible ? 1 : 0);
    if (A > 10) for (int k = lane; k < N * A; k += 64) S.o_perm[e * N * A + k] = 0;
    const int nk = c.rng_mode == CN_RNG_PHILOX ? 1 : CN_MT_N;   // key words to copy
    {   // all loads first, then all stores: mt_src may be LDS or global, so the compiler cannot pipeline
        uint32_t v[(CN_MT_N + 63) / 64];
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; v[j] = k < nk ? mt_src[k] : 0u; }
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; if (k < nk) S.mt[e * CN_MT_N + k] = v[j]; }
    }
    if (lane == 0) {
        S.scenario[e] = (int32_t)sc;
        S.gtime[e] = 0.0; S.r_dv[e] = 0.0;
        S.r_px[e] = rpx; S.r_py[e] = rpy; S.r_gx[e] = en.rgx; S.r_gy[e] = en.rgy; S.r_theta[e] = rth;
        S.r_vx[e] = 0.0; S.r_vy[e] = 0.0; S.r_radius[e] = c.robot_radius; S.r_vpref[e] = c.robot_vpref;
        S.case_counter[e] = (S.case_counter[e] + c.nenv) % g.case_size;
        S.potential[e] = -fabs(np_norm2(rpx - en.rgx, rpy - en.rgy));
        S.reset_count[e] += 1;
        S.ep_return[e] = 0.0; S.ep_len[e] = 0;
        S.flags[e] = 0; S.overflow[e] = ovf; S.mt_pos[e] = pos;
        if (obs) {
            float *rn = g.robot_node + orw * 7;
            rn[0] = (float)rpx; rn[1] = (float)rpy; rn[2] = (float)c.robot_radius;
            rn[3] = (float)en.rgx; rn[4] = (float)en.rgy; rn[5] = (float)c.robot_vpref; rn[6] = (float)rth;
            g.temporal[orw * 2] = 0.0f; g.temporal[orw * 2 + 1] = 0.0f;
        }
    }
}


// Word page of a goal pass: the doubles of the next 128 stream words (64 draws) and, where the pass
// needs angles, cos / sin of 2*pi*draw, computed by the 64 lanes at once (one draw + one f64 sincos per
// lane) so that the sequential walk over the humans only reads tables. Index k holds the draw at word
// pb + 2k. Wave-uniform reads are LDS broadcasts (v_readlane broadcasts of loop-carried values
// miscompiled in this loop nest: wrong winners and NaN goals on the GPU, tools/diag_goal.py).
struct GPage {
    double *d, *cs, *sn;   // LDS [64] each (the wave's try-slot area m.sl, unused by the goal passes)
    int pb;
    __device__ double dbl(int q) const { return d[(q - pb) >> 1]; }
    __device__ double cos2pi(int q) const { return cs[(q - pb) >> 1]; }
    __device__ double sin2pi(int q) const { return sn[(q - pb) >> 1]; }
};

// (re)build the page at the stream position m.p (all lanes)
__device__ __forceinline__ void gpage_build(WRng &m, GPage &pg, bool trig)
{
    wsync();   // earlier reads of the old page are done before it is overwritten
    m.ensure(128);
    pg.pb = m.p;
    const double d = m.dbl(m.p + 2 * m.lane);
    pg.d[m.lane] = d;
    if (trig) {
        const double a = d * CN_PI * 2;
        pg.cs[m.lane] = cos(a);
        pg.sn[m.lane] = sin(a);
    }
    wsync();
}

// One of the two goal-change loops at the end of CrowdSimDict.step:
//   KIND 0  update_human_goals_randomly (crowd_sim.py:724-766): humans with v_pref != 0 draw U; if
//           U <= goal_change_chance a new goal on the circle is rejection-sampled (angle, gx_noise, gy_noise);
//   KIND 1  update_human_goal (crowd_sim.py:769-811): humans within their radius of the goal draw U; if
//           U <= end_goal_change_chance radius / v_pref are jittered and create_agent_attributes'
//           candidate is rejection-sampled.
// Both walk the humans in index order, as the reference does, over a page of precomputed draws (GPage):
// the walk itself is wave-uniform table reads; a changing human tests J tries at once, lane = (try t,
// agent a), against the robot and the other humans (earlier humans already carry their new goals); the
// first try without a hit wins. Bounded by max_tries like every rejection loop.
template <int KIND, bool GRID>
__device__ __forceinline__ int goal_pass(const cn_config &c, Env1 &en, WRng &m, uint32_t &ovf, int sc, double *sp,
                                         int64_t edbg = -1)
{
#ifdef CN_STAMPS
    unsigned long long tq = clock64(), t_walk = 0, t_first = 0, t_rej = 0;
#define GP_LAP(acc) do { const unsigned long long t_ = clock64(); acc += t_ - tq; tq = t_; } while (0)
#else
#define GP_LAP(acc) do { } while (0)
#endif
    (void)sp;
    int dbg = 0;   // diagnostics: 1000 * batches + eligible humans + 100 * changes
    const int N = c.human_num, lane = m.lane;
    const double chance = KIND == 0 ? c.goal_change_chance : c.end_goal_change_chance;
    const int W = KIND == 0 ? 6 : cand_words(sc);
    const bool trig = KIND == 0 || sc == CN_SC_CIRCLE_CROSSING;
    bool elig_l = false;       // eligibility reads only the human's own goal / radius: fixed up front
    if (lane < N) {
        if (KIND == 0) elig_l = en.hvp[lane] != 0;
        else elig_l = norm_lt(en.hgx[lane] - en.hpx[lane], en.hgy[lane] - en.hpy[lane], en.hr[lane]);
    }
    uint64_t rem = __ballot(elig_l);
    dbg += __popcll(rem);
    if (!rem) return dbg;
    GPage pg;
    pg.d = m.sl; pg.cs = m.sl + 64; pg.sn = m.sl + 128;
    gpage_build(m, pg, trig);
    const int NA = N;              // robot + the other N-1 humans
    const int JA = 64 / NA;        // tries per batch the lanes hold
    const int JP = 128 / W;        // tries per batch a fresh page holds
    GP_LAP(t_walk);
    while (rem) {
        // The remaining eligible humans draw U at consecutive stream positions until one of them changes its
        // goal, so all of them are tested at once: lane = human index, rank = its place among them; the
        // first rank with U <= chance (within the page) changes, the draws of the ranks before it are spent.
        if (m.p + 2 > pg.pb + 128) gpage_build(m, pg, trig);
        const int avail = (pg.pb + 128 - m.p) >> 1;   // draws left in the page (>= 1)
        const bool mine = ((rem >> lane) & 1ull) != 0;
        const int rank = __popcll(rem & ((1ull << lane) - 1ull));
        bool hit = false;
        if (mine && rank < avail) hit = pg.dbl(m.p + 2 * rank) <= chance;
        const uint64_t hits = __ballot(hit);
        if (!hits) {   // none of the first min(avail, |rem|) changes: their draws are spent
            const int nr = min(avail, __popcll(rem));
            rem &= ~__ballot(mine && rank < nr);
            m.p += 2 * nr;
            continue;
        }
        const int h = __ffsll((long long)hits) - 1;
        m.p += 2 * (__popcll(rem & ((1ull << h) - 1ull)) + 1);
        rem &= ~((2ull << h) - 1ull);   // h and the humans before it are done
        dbg += 100;
        double r_self = en.hr[h], vpc = en.hvp[h];
        if (KIND == 1) {
            const int jw = 2 * ((c.random_radii ? 1 : 0) + (c.random_v_pref ? 1 : 0));
            if (jw) {
                if (m.p + jw > pg.pb + 128) gpage_build(m, pg, trig);
                if (c.random_radii) { r_self += -0.1 + (0.1 - -0.1) * pg.dbl(m.p); m.p += 2; }
                if (c.random_v_pref) { vpc += -0.1 + (0.1 - -0.1) * pg.dbl(m.p); m.p += 2; }
                if (lane == 0) { en.hr[h] = r_self; en.hvp[h] = vpc; }
            }
        }
        const double vpk = (KIND == 0 && vpc == 0) ? 1.0 : vpc;
        GP_LAP(t_walk);
        for (int t0 = 0;; ) {
            if (t0 > 0) {
                // crowded (the first batch was all rejected): the remaining tries 64 candidates at a time
                // straight from the stream (goal_reject_crowded); its try slots overwrite the page
                const int tw = goal_reject_crowded<GRID>(c, en, m, h, r_self, W, c.max_tries - t0, ovf, [&](int q, int tt) {
                    double gx, gy;
                    if (KIND == 0) {
                        gx = c.circle_radius * m.cos2pi(q) + (m.dbl(q + 2) - 0.5) * vpk;
                        gy = c.circle_radius * m.sin2pi(q) + (m.dbl(q + 4) - 0.5) * vpk;
                    } else {
                        double px, py, hd, vp;
                        cand_attributes(c, m, q, sc, vpc, r_self, en.rr, px, py, gx, gy, hd, vp);
                    }
                    m.sl[tt] = gx; m.sl[64 + tt] = gy;
                }, KIND == 0 ? c.circle_radius + 0.5 * fabs(vpk) + 1e-3
                   : sc == CN_SC_SQUARE_CROSSING ? 0.1 * c.square_width + 0.5 * fabs(vpc == 0 ? 1.0 : vpc) + 1e-3 : 0.0);
                if (lane == 0) { en.hgx[h] = m.sl[tw]; en.hgy[h] = m.sl[64 + tw]; }
                wsync();
                pg.pb = -(1 << 28);   // forces a rebuild before the next read
                GP_LAP(t_rej);
                break;
            }
            if (m.p + W * min(JA, JP) > pg.pb + 128) gpage_build(m, pg, trig);
            const int J = min(min(JA, (pg.pb + 128 - m.p) / W), c.max_tries - t0);   // >= 1
            const int t = lane / NA, a = lane - t * NA;
            const bool valid = t < J;
            double gx = 0, gy = 0;
            bool bad = true;
            if (valid) {
                const int q = m.p + W * t;
                if (KIND == 0) {
                    gx = c.circle_radius * pg.cos2pi(q) + (pg.dbl(q + 2) - 0.5) * vpk;
                    gy = c.circle_radius * pg.sin2pi(q) + (pg.dbl(q + 4) - 0.5) * vpk;
                } else {
                    double px, py, hd, vp;
                    cand_attributes(c, pg, q, sc, vpc, r_self, en.rr, px, py, gx, gy, hd, vp);
                }
                bad = goal_hit(c, en, h, r_self, gx, gy, a);
            }
            dbg += 1000;
            const uint64_t badm = __ballot(bad);
            const uint64_t gmask = NA >= 64 ? ~0ull : ((1ull << NA) - 1ull);
            int win = -1;
            for (int k = 0; k < J; ++k)
                if (((badm >> (k * NA)) & gmask) == 0) { win = k; break; }
            if (win < 0 && t0 + J >= c.max_tries) { win = J - 1; ++ovf; }
            if (win >= 0) {
                if (lane == win * NA) { en.hgx[h] = gx; en.hgy[h] = gy; }   // the winning try's a = 0 lane
                m.p += W * (win + 1);
                wsync();
                break;
            }
            m.p += W * J;
            t0 += J;
        }
        GP_LAP(t_first);
    }
#ifdef CN_STAMPS
    if (lane == 0 && edbg >= 0 && edbg < 8192) {
        cn_stamp_b[edbg * CN_NSTAMP + 8 + 3 * KIND] = t_walk;
        cn_stamp_b[edbg * CN_NSTAMP + 9 + 3 * KIND] = t_first;
        cn_stamp_b[edbg * CN_NSTAMP + 10 + 3 * KIND] = t_rej;
    }
#endif
#undef GP_LAP
    (void)edbg;
    return dbg;
}

// Goal changes at the end of CrowdSimDict.step (crowd_sim_dict.py:260-269) for one env, one wave:
// update_human_goals_randomly when `rgoal`, then update_human_goal when `egoal` (goal_pass).
// `en` holds the post-move agents (LDS); the env's MT19937 stream is loaded from / written back to
// the state; `sp` = wave LDS scratch.
template <bool GRID>
__device__ __forceinline__ void goal_changes(const cn_config &c, const cn_state_ptrs &S, int64_t e, Env1 &en, WRng &m,
                                             bool rgoal, bool egoal, double *sp)
{
    const int N = c.human_num;
    const int lane = m.lane;
    uint32_t *mtw = m.w;
    const int64_t hb = e * N;
    m.off = 0;
    if (m.phx) m.key = S.mt[e * CN_MT_N];
    else {
        uint32_t v[(CN_MT_N + 63) / 64];
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; v[j] = k < CN_MT_N ? S.mt[e * CN_MT_N + k] : 0u; }
#pragma unroll
        for (int j = 0; j < (CN_MT_N + 63) / 64; ++j) { const int k = lane + 64 * j; if (k < CN_MT_N) mtw[k] = v[j]; }
    }
    m.p = S.mt_pos[e];
    m.have1 = false; m.slid = false;
    uint32_t ovf = S.overflow[e];
    const int sc = S.scenario[e];
    wsync();
    STAMP_B(m.edbg, 1);
    int dbg0 = 0, dbg1 = 0;
    if (rgoal) dbg0 = goal_pass<0, GRID>(c, en, m, ovf, sc, sp, m.edbg);
    STAMP_B(m.edbg, 2);
    if (egoal) dbg1 = goal_pass<1, GRID>(c, en, m, ovf, sc, sp, m.edbg);
    STAMP_B(m.edbg, 3);
#ifdef CN_STAMPS
    if (lane == 0 && (unsigned long long)m.edbg < 8192) { cn_stamp_b[m.edbg * CN_NSTAMP + 6] = dbg0; cn_stamp_b[m.edbg * CN_NSTAMP + 7] = dbg1; }
#endif
    (void)dbg0; (void)dbg1;
    // numpy twists lazily: a stream that consumed exactly the 624 words is (old key, pos 624)
    const bool in1 = !m.phx && m.p > CN_MT_N;
    if (lane < N) {
        S.h_gx[hb + lane] = en.hgx[lane]; S.h_gy[hb + lane] = en.hgy[lane];
        S.h_r[hb + lane] = en.hr[lane]; S.h_vpref[hb + lane] = en.hvp[lane];
    }
    if (in1 || m.slid)
        for (int k = lane; k < CN_MT_N; k += 64) S.mt[e * CN_MT_N + k] = m.blk(in1 ? 1 : 0)[k];
    if (lane == 0) { S.mt_pos[e] = in1 ? m.p - CN_MT_N : m.p; S.overflow[e] = ovf; }
    wsync();
    STAMP_B(m.edbg, 4);
}

// Auto-reset of env e (VecEnv worker, shmem_vec_env.py:164-168 -> CrowdSimDict.reset): copy the pending
// spawn when `may_consume` and it is valid for the current key, else draw it here. One wave.
template <bool GRID, bool FENCE = GRID, bool OBS_OPT = false>
__device__ __forceinline__ void reset_env(const ResetOut &o, const PendPtrs &P2, const cn_config &c, int64_t E, int64_t e,
                          int64_t counter_offset, bool may_consume, uint32_t launch_id, WRng &m, Env1 &en,
                          uint32_t *inline_count = nullptr)
{
    const cn_state_ptrs &S = o.s;
    const int N = c.human_num;
    const int lane = m.lane;
    const int64_t cc = S.case_counter[e];
    const int32_t rc = S.reset_count[e];
    const PendPtrs P = pend_slot(P2, rc & 1, E, E * N);
    // An entry completed by THIS launch (a resumed spawn finishing beside this reset) is not consumed: its
    // stores need not be visible yet; the reset draws inline instead.
    // The ok word carries the key it completes and is read first: only an entry completed by an earlier launch
    // FOR THIS KEY is consumed, and no wave of this launch writes such a slot (a slot is rewritten for key rc + 2
    // only after this reset; a spawn of key rc that is written for the first time in this very launch shows the
    // key in its ok word only with id 0 or this launch's), so the payload read after it needs no fence.
    // Multi-step launches (an env may reset several times in one launch, at keys rc, rc + 1, rc + 2, ...): the same
    // holds. The spawn waves of launch L write, per env and slot parity, at most one item: the one entry the env's
    // workgroup kept in launch L - 1's list (cn_step_kernel, phase 5) or a spawn parked by L - 1, never both live
    // (a parked spawn of key K is dropped once reset_count > K, and an entry of its parity queued in L - 1 comes
    // from a reset at a key >= K, after which reset_count > K). An item written in L has a key K' <= rc for a
    // reset at key rc of L itself (it was queued by a reset at K' - 2 of an earlier launch, and keys only grow);
    // K' == rc shows this launch's id or 0, K' < rc another key: neither is consumed, and an entry that IS
    // consumed (key rc, completed by an earlier launch) has no writer in L, because the one item of its parity
    // alive in L would have to carry a key > rc. So no two waves of a launch write one slot, a slot consumed in L
    // is rewritten in L + 1 at the earliest, and a reset consumes only what an earlier launch completed for its key.
    const uint64_t okw = P.ok[e];
    const uint32_t ok = (uint32_t)okw;
    if (FENCE) __threadfence();
    const bool key_ok = (int32_t)(uint32_t)(okw >> 32) == rc && P.cc[e] == cc && P.rc[e] == rc;
    if (may_consume && ok && ok != launch_id && key_ok) {
        if (lane < N) {
            const int64_t h = e * N + lane, EN = E * N;
            double v[7];
#pragma unroll
            for (int f = 0; f < 7; ++f) v[f] = P.h[f * EN + h];
            asm volatile("" ::: "memory");
            en.hpx[lane] = v[0]; en.hpy[lane] = v[1]; en.hgx[lane] = v[2]; en.hgy[lane] = v[3];
            en.hr[lane] = v[4]; en.hvp[lane] = v[5]; en.hth[lane] = v[6];
        }
        en.rpx = P.r[e]; en.rpy = P.r[E + e]; en.rgx = P.r[2 * E + e]; en.rgy = P.r[3 * E + e];
        const double rth = P.r[4 * E + e];
        wsync();
        write_reset<OBS_OPT>(o, c, e, en, rth, P.sc[e], P.ovf[e], P.mt + e * CN_MT_N, P.pos[e], lane);
    } else {
        double rth;
        uint32_t ovf;
        int sc;
        if (inline_count && lane == 0) atomicAdd(inline_count, 1u);
        spawn_env<GRID>(c, c.env_offset + orow(o.ov, e), cc, rc, counter_offset, m, en, rth, ovf, sc);
        const bool in1 = !m.phx && m.p > CN_MT_N;
        write_reset<OBS_OPT>(o, c, e, en, rth, sc, ovf, m.blk(in1 ? 1 : 0), in1 ? m.p - CN_MT_N : m.p, lane);
    }
    wsync();
}

// Spawn waves of kernel A: draw the next episode of every env reset by the previous kernel A
// (or of every env after cn_reset / cn_set_state). One wave per env, independent of the other waves.
struct PendLaunch {
    PendPtrs P;
    const uint32_t *list;   // envs reset by the previous launch: {e, reset_count, case_counter lo, hi} after it
    const uint32_t *count;
    const uint32_t *rlist;  // spawns parked by the previous launch: {e | 2^31 if not started, key rc, cc lo, cc hi}
    const uint32_t *rcount;
    uint32_t *rlist_w;      // spawns this launch parks
    uint32_t *rcount_w;
    int all;                // PEND_BOTH: every env's two spawns, PEND_FRESH: none (lists ignored); 0: the lists
    int step_blocks, pend_blocks;
    int first;              // 1: workgroups [0, pend_blocks) (kd-tree path); 0: after the step workgroups
    int waves;              // spawning waves per spare workgroup (RNG regions that fit the launch's LDS)
    int stride;             // bytes per spawning wave's region (StepPlan::rng_stride)
    int64_t counter_offset;
    int64_t case_size;
    OutView ov;             // global env index = c.env_offset + orow(ov, e)
    long long budget;       // clock cycles a spawning wave works before parking (0: never parks)
    uint32_t launch_id;     // nonzero id of this launch (pending entries it completes carry it)
    uint32_t *stats;        // [4] cumulative (kd-tree path): parked unstarted, parked mid-way, resumed, completed on
                            // resume; [7] resets of the step workgroups that drew their spawn inline (every path)
};

// GRID: the spawn's crowded rejection through a DiscGrid (the kd-tree path's plans have LDS for it).
// Spawns are parked after the launch's budget and resumed later (kd-tree and quad path alike, see CN_QUAD_BUDGET).
// Items: the envs reset by the previous launch (their spawn for the reset after next), then the spawns
// the previous launch parked. With a budget, a wave parks its spawn between two humans once the budget
// is spent (stream, robot and humans so far go to the pending slot, the item to rlist_w) and parks the
// items it has not started; a later launch resumes them. The pending slot of a spawn is written only by
// the wave that owns the item, and a reset consumes an entry only if an EARLIER launch completed it.
// RESUME_FIRST (multi-step launches): the parked spawns come before the new items. A multi-step launch reads the
// entries of a whole chunk of steps, many more than there are spawning waves; with the new items first, every
// wave's first item (the one it works on whatever the budget) would be a new one, and under a small budget the
// parked spawns, which are the older ones and needed sooner, would be parked again in every launch until stale.
template <bool PHX, bool GRID, bool RESUME_FIRST = false>
__device__ __forceinline__ void pend_waves(const PendLaunch &pl, const cn_state_ptrs &S, const cn_config &c, int E, char *smem)
{
    const int nw = pl.waves, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= nw) return;
    const int N = c.human_num;
    char *base = smem + w * pl.stride;
    uint32_t *mtw = (uint32_t *)base;
    double *hb = (double *)(base + 2 * CN_MT_N * 4);
    // envs reset by the previous launch: the reset after next (the next one was drawn earlier); after
    // cn_set_state (PEND_BOTH): both the next (items [0, E)) and the one after ([E, 2E)); after cn_reset
    // (PEND_FRESH, its kernel pre-drew both): none
    const uint32_t nnew = pl.all == PEND_BOTH ? (uint32_t)(2 * E) : pl.all ? 0u : min(*pl.count, (uint32_t)E);
    // parked spawns of the previous launch
    const uint32_t nres = pl.all ? 0u : min(*pl.rcount, (uint32_t)(2 * E));
    const int pb = pl.first ? (int)blockIdx.x : (int)blockIdx.x - pl.step_blocks;
    const long long deadline = pl.budget ? (long long)clock64() + pl.budget : 0;
    bool worked = false;   // a wave always works on its first item of the launch (progress for any budget)
    for (uint32_t it0 = (uint32_t)(pb * nw + w); it0 < nnew + nres; it0 += (uint32_t)(pl.pend_blocks * nw)) {
        uint32_t it = it0;   // item: [0, nnew) the new ones, [nnew, nnew + nres) the parked ones
        if constexpr (RESUME_FIRST) {   // the same list, rotated to start at the parked spawns
            it = it0 + nnew;
            if (it >= nnew + nres) it -= nnew + nres;
            it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);   // wave-uniform: the entries stay scalar loads
        }
        int64_t e, cc;
        int32_t rc;
        bool started = false;
        if (it < nnew) {
            const bool ahead2 = pl.all != PEND_BOTH || it >= (uint32_t)E;
            // the key's counters come from a list entry, never from the state: the step workgroups of this
            // same launch reset terminal envs and rewrite reset_count / case_counter while the spawn waves run.
            // PEND_BOTH: cn_keysnap_kernel's snapshot of every env's counters, written (stream-ordered) by
            // cn_set_state / cn_reset before this launch (entry e for items e and e + E); otherwise the
            // counters the previous launch's reset wrote (round 5: read back by the resetting wave)
            const uint32_t *q = pl.list + 4 * (pl.all ? it % (uint32_t)E : it);
            e = (int64_t)q[0];
            rc = (int32_t)q[1];
            cc = (int64_t)((uint64_t)q[2] | ((uint64_t)q[3] << 32));
            if (ahead2) { cc = (cc + c.nenv) % pl.case_size; rc += 1; }   // write_reset's counter update
        } else {
            const uint32_t *q = pl.rlist + 4 * (it - nnew);
            e = (int64_t)(q[0] & 0x7fffffffu);
            started = (q[0] >> 31) == 0u;
            rc = (int32_t)q[1];
            cc = (int64_t)((uint64_t)q[2] | ((uint64_t)q[3] << 32));
            // its reset has come and gone (drawn inline). reset_count may be advanced by a reset of this same
            // launch while it is read; either value is safe: such a reset draws inline (the parked entry is not
            // complete), so the item only turns stale, and the next writer of its slot (key rc + 2, queued by
            // that reset) belongs to the next launch, stream-ordered after this item's stores.
            // (multi-step launches: several resets of the env may follow in this launch; they queue one entry per
            // slot parity, for the next launch, and reset_count only grows, so the item stays stale)
            if (rc < S.reset_count[e]) continue;
        }
        if (deadline && worked && (long long)clock64() > deadline) {   // out of budget: park the item unstarted / as is
            if (lane == 0) {
                atomicAdd(pl.stats + (started ? 1 : 0), 1u);
                const uint32_t k = atomicAdd(pl.rcount_w, 1u);
                if (k < (uint32_t)(2 * E)) {
                    uint32_t *q = pl.rlist_w + 4 * k;
                    q[0] = (uint32_t)e | (started ? 0u : 0x80000000u); q[1] = (uint32_t)rc;
                    q[2] = (uint32_t)(uint64_t)cc; q[3] = (uint32_t)((uint64_t)cc >> 32);
                }
            }
            continue;
        }
        Env1 en;
        en.hpx = hb; en.hpy = hb + 32; en.hgx = hb + 64; en.hgy = hb + 96; en.hr = hb + 128; en.hvp = hb + 160;
        en.hth = hb + 192;
        WRng m;
        m.w = mtw; m.off = 0; m.lane = lane; m.phx = PHX; m.edbg = -1;
        m.grid = pl.stride > CN_PEND_LDS ? base + CN_PEND_LDS : nullptr;
        m.sl = (double *)(base + 2 * CN_MT_N * 4 + 7 * 32 * 8);
        double rth = 0;
        uint32_t ovf = 0;
        int sc = 0, i0 = 0;
        if (started) {   // restore the parked spawn: stream at the park point, robot, the humans so far
            const PendPtrs P = pend_slot(pl.P, rc & 1, E, (int64_t)E * N);
            i0 = P.prog[e];
            const int nk = PHX ? 1 : CN_MT_N;
            for (int k = lane; k < nk; k += 64) mtw[k] = P.mt[e * CN_MT_N + k];
            if (lane < i0) {
                const int64_t h = e * N + lane, EN = (int64_t)E * N;
                en.hpx[lane] = P.h[h]; en.hpy[lane] = P.h[EN + h]; en.hgx[lane] = P.h[2 * EN + h];
                en.hgy[lane] = P.h[3 * EN + h]; en.hr[lane] = P.h[4 * EN + h]; en.hvp[lane] = P.h[5 * EN + h];
                en.hth[lane] = P.h[6 * EN + h];
            }
            en.rpx = P.r[e]; en.rpy = P.r[E + e]; en.rgx = P.r[2 * E + e]; en.rgy = P.r[3 * E + e];
            rth = P.r[4 * E + e];
            en.rr = c.robot_radius;
            ovf = P.ovf[e]; sc = P.sc[e];
            m.p = P.pos[e]; m.have1 = false; m.slid = false;
            m.key = mtw[0];
            if (lane == 0) atomicAdd(pl.stats + 2, 1u);
            wsync();
        }
#ifdef CN_STAMPS
        const unsigned long long ts0 = clock64();
#endif
        const int done = spawn_env<GRID>(c, c.env_offset + orow(pl.ov, e), cc, rc, pl.counter_offset, m, en, rth, ovf,
                                         sc, i0, deadline);
        worked = true;
        const bool in1 = !m.phx && m.p > CN_MT_N;
        write_pending<false>(pl.P, c, E, e, en, rth, sc, ovf, m.blk(in1 ? 1 : 0), in1 ? m.p - CN_MT_N : m.p, cc, rc, lane,
                             done == N ? pl.launch_id : 0u, done);
        if (started && done == N && lane == 0) atomicAdd(pl.stats + 3, 1u);
        if (done < N && lane == 0) {   // parked mid-way
            atomicAdd(pl.stats + 1, 1u);
            const uint32_t k = atomicAdd(pl.rcount_w, 1u);
            if (k < (uint32_t)(2 * E)) {
                uint32_t *q = pl.rlist_w + 4 * k;
                q[0] = (uint32_t)e; q[1] = (uint32_t)rc;
                q[2] = (uint32_t)(uint64_t)cc; q[3] = (uint32_t)((uint64_t)cc >> 32);
            }
        }
#ifdef CN_STAMPS
        if (lane == 0 && e < 8192 && done == N) { cn_stamp_p[2 * e] = ts0; cn_stamp_p[2 * e + 1] = clock64(); }
#endif
        wsync();
    }
}
