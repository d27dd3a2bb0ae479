// ctrl_feedback_lane.hip.h -- the lane loop of the angle-feedback rollout kernels and the staging of a block's policy, shared by
// ctrl_rollout_feedback.hip (the kernels with the default controller folded in), ctrl_rollout_feedback_pid.hip (their PID
// instantiations: per-env gains), ctrl_rollout_feedback_dist.hip (their disturbance instantiations: per-env plant noise) and
// ctrl_rollout_feedback_loss.hip (their loss instantiations: per-env packet erasures as well).  What the loop does is stated at
// the top of ctrl_rollout_feedback.hip.  Everything here is local to the including file (an unnamed namespace): each of the
// four compiles its own instantiations.
#pragma once
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

constexpr int S = GW_MAX_NSTATES;
constexpr int FB_LEN_MAX = 64;                               // entries of one bin's schedule (1 <= L <= 64)
constexpr int FB_BINS = GW_CTRL_FB_MAX_BINS;

struct FbRows {                                              // gw_ctrl_feedback_rows, all [steps][N]
    int32_t *device_out, *duration_out, *obs;
    float* reward;
    double* angle_deg;
    uint8_t* ended;
};

// The loop of both kernels, one lane per env.  ROWS: row k receives the action taken and what gw_ctrl_rollout would write,
// stores nothing waits for.  PID: the controller is the PID on the env's own gains, as in ctrl_rollout.hip's loop.
// (A __forceinline__ template, not a kernel: the kernels below are plain functions.)
// DIST (with PID): the plant is disturbed, as in that loop -- the env's record in registers, its count stored back once, a reset
// leaves it alone.
// LOSS (with PID and DIST): every transmission takes a draw of the env's own erasures, as in that loop -- the record in
// registers, its count and erasure counts stored back once, a reset leaves it alone.  x is the last parameter, and defaulted.
template <bool ROWS, bool PID, bool DIST, bool LOSS = false>
__device__ __forceinline__ void ctrl_feedback_lane(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w,
                                                   const int steps, const uint32_t max_steps, const double fail_deg, const uint8_t* s_trans, const double* s_ber, double* col0,
                                                   double* col1, const int64_t e, const uint8_t* s_sched, const int32_t* s_edges,
                                                   const uint32_t* s_par, const FbRows& r, double* __restrict__ tally,
                                                   const GwCtrlLoss& x = GwCtrlLoss{nullptr})
{
    static_assert(DIST || !LOSS, "the loss instantiations are disturbance instantiations");
    const GwDevConst k = *(const GW_AS_CONST GwDevConst*)c.cst;
    Lane L;
    L.now = c.now[e]; L.wake = c.wake[e]; L.u = c.u[e]; L.ang = c.ang[e]; L.ktick = c.ktick[e];
    for (int i = 0; i < 4; ++i) L.x[i] = c.x[e * 4 + i];
    Q q0, q1;
    { const uint32_t hl = c.qhl[e]; q0.head = hl & 0xffu; q0.len = hl >> 8; }
    { const uint32_t hl = c.qhl[c.N + e]; q1.head = hl & 0xffu; q1.len = hl >> 8; }
#pragma unroll
    for (int j = 0; j < CR; ++j) L.rxs[j] = c.rxs[j * c.N + e];
    L.got1 = c.got[e * 2]; L.got2 = c.got[e * 2 + 1];
    L.ntx = c.ntx[e]; L.ncmd = c.ncmd[e]; L.nsub = c.nsub[e]; L.fl = c.flags[e];
    double* ring0 = c.pay + ((size_t)e * 2 + 0) * GW_RING_PHYS;
    double* ring1 = c.pay + ((size_t)e * 2 + 1) * GW_RING_PHYS;
    Pid G;
    if (PID) pid_load(G, g, e);
    Dist W;
    if (DIST) dist_load(W, w, e);
    Loss X;
    if (LOSS) loss_load(X, x, e);
    uint32_t age = s.age[e];
    double cost = s.cost[e];
    const double deg_per_rad = 180.0 / 3.141592653589793;
    const uint32_t Ls = s_par[0];                            // from LDS, not the kernel's arguments: the step's body leaves no
    const bool abs_key = s_par[1] != 0u;                     // scalar register free, these live in vector registers

    uint32_t at_sched = age % Ls;                            // the entry the env acts on next: a running counter, no modulo per step
    uint32_t n_ended = 0u, n_failed = 0u, n_bin0 = 0u;
    double cost_ended = 0.0, airtime = 0.0, elapsed = 0.0, area = 0.0;

    for (int step = 0; step < steps; ++step) {
        const int64_t at = (int64_t)step * c.N + e;
        // what the env sees: the angle of its current state as the int32 observation, defined for every f64 (NaN -> -1e9)
        const int32_t o = (int32_t)fmin(fmax(L.x[2] * deg_per_rad, -1e9), 1e9);
        const int32_t key = abs_key ? (o < 0 ? -o : o) : o;
        uint32_t bin = 0u;
#pragma unroll
        for (int j = 0; j < FB_BINS - 1; ++j) bin += s_edges[j] <= key ? 1u : 0u;     // any edges, sorted or not, mean this count
        n_bin0 += bin == 0u ? 1u : 0u;
        const uint32_t ent = (bin * Ls + at_sched) * 2u;     // a byte outside the action space is clamped where it is read
        const int d = (int)gw_min_u32((uint32_t)s_sched[ent], 1u);
        const int du = (int)gw_min_u32((uint32_t)s_sched[ent + 1u], (uint32_t)k.max_duration - 1u);
        const double t_before = L.now;
        q_open(q0);
        q_open(q1);
        if constexpr (LOSS) {
#define GW_CTRL_PID
#define GW_CTRL_DIST
#define GW_CTRL_LOSS
#include "ctrl_step_body.h"
#undef GW_CTRL_LOSS
#undef GW_CTRL_DIST
#undef GW_CTRL_PID
        } else if constexpr (DIST) {
#define GW_CTRL_PID
#define GW_CTRL_DIST
#include "ctrl_step_body.h"
#undef GW_CTRL_DIST
#undef GW_CTRL_PID
        } else if constexpr (PID) {
#define GW_CTRL_PID
#include "ctrl_step_body.h"
#undef GW_CTRL_PID
        } else {
#include "ctrl_step_body.h"
        }
        const double deg = L.x[2] * deg_per_rad;             // InvertedPendulumInterpreter, envs/inverted_pendulum.py:27-57
        if (ROWS) {
            r.device_out[at] = d;
            r.duration_out[at] = du;
            r.obs[at] = (int32_t)deg;
            r.reward[at] = (float)fabs(180.0 - deg);
            if (r.angle_deg) r.angle_deg[at] = deg;
        }
        q_flush(q0, ring0, col0);
        q_flush(q1, ring1, col1);
        const double dt = L.now - t_before;                  // the env's clock after the step, before any reset
        airtime = airtime + (double)du;
        elapsed = elapsed + dt;
        area = area + fabs(deg) * dt;
        age++;                                               // the episode rule: the step's own outputs stand, then the env is reset
        cost = cost + fabs(deg);
        const uint32_t cause = ((max_steps > 0u && age == max_steps) ? 1u : 0u) | ((fail_deg > 0.0 && fabs(deg) > fail_deg) ? 2u : 0u);
        if (ROWS) r.ended[at] = (uint8_t)cause;
        at_sched = at_sched + 1u == Ls ? 0u : at_sched + 1u;
        if (cause) {                                         // gw_ctrl_reset for this one env, in registers; flags are sticky
            n_ended++;
            n_failed += cause >> 1;
            cost_ended = cost_ended + cost;
            L.now = 0.0; L.wake = 0.0; L.ang = 0.0; L.ktick = 0u;
            for (int i = 0; i < 4; ++i) L.x[i] = s.x_init[e * 4 + i];
            L.u = s.u_init[e];
            q0.head = q0.len = 0u; q1.head = q1.len = 0u;
#pragma unroll
            for (int j = 0; j < CR; ++j) L.rxs[j] = 0u;
            L.got1 = L.got2 = 0u;
            L.ntx = L.ncmd = L.nsub = 0u;
            age = 0u; cost = 0.0; at_sched = 0u;
            if (PID) G.last = 0.0;
        }
    }

    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));
#pragma unroll
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl;
    s.age[e] = age; s.cost[e] = cost;
    if (PID) pid_store(G, g, e);
    if (DIST) dist_store(W, w, e);
    if (LOSS) loss_store(X, x, e);
    double* t = tally + e * GW_CTRL_FB_COLS;
    t[0] = (double)n_ended; t[1] = (double)n_failed; t[2] = (double)steps; t[3] = cost_ended;
    t[4] = airtime;         t[5] = elapsed;          t[6] = area;          t[7] = (double)n_bin0;
}

// the block's policy -> LDS: B Ls schedule entries of two bytes and B - 1 edges (B and Ls are the host's, checked there; the
// bounds here keep a wrong call inside the arrays).  The edges beyond B - 1 are INT32_MAX, above every key (|key| <= 1e9): the
// lanes always count seven compares and need neither B nor a loop.
__device__ __forceinline__ void stage_policy(uint8_t* s_sched, int32_t* s_edges, uint32_t* s_par, const uint8_t* __restrict__ sched,
                                             const int32_t* __restrict__ edges, uint32_t envs_per_policy, uint32_t B, uint32_t Ls,
                                             int abs_key)
{
    if (threadIdx.x < (uint32_t)(FB_BINS - 1)) s_edges[threadIdx.x] = 0x7fffffff;
    if (threadIdx.x == 0) { s_par[0] = Ls; s_par[1] = abs_key ? 1u : 0u; }
    const uint32_t p = (uint32_t)(((int64_t)blockIdx.x * 64) / envs_per_policy);
    const uint32_t nb = 2u * B * Ls;
    for (uint32_t i = threadIdx.x; i < nb && i < (uint32_t)(FB_BINS * FB_LEN_MAX * 2); i += blockDim.x) s_sched[i] = sched[(size_t)p * nb + i];
    if (threadIdx.x + 1u < B && threadIdx.x < (uint32_t)(FB_BINS - 1)) s_edges[threadIdx.x] = edges[(size_t)p * (B - 1u) + threadIdx.x];
}

inline int launched() { return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP; }

} // namespace
