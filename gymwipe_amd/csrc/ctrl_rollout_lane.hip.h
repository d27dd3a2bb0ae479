// ctrl_rollout_lane.hip.h -- the lane loop of the fused control-loop rollout kernels, shared by ctrl_rollout.hip (the kernels
// with the default controller folded in and their PID instantiations), ctrl_rollout_dist.hip (their disturbance
// instantiations: per-env plant noise) and ctrl_rollout_loss.hip (their loss instantiations: per-env packet erasures as well).
// What fusion changes around the step is stated at the top of ctrl_rollout.hip.
// Everything here is local to the including file (an unnamed namespace): each of the three compiles its own instantiations.
#pragma once
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

constexpr int S = GW_MAX_NSTATES;
constexpr int SCHED_MAX = 64;                                // entries of a schedule (gw_ctrl_rollout_schedules: 1 <= L <= 64)

// The loop of both fused kernels, one lane per env.  SCHED: the action is entry `age % Ls` of the block's schedule in LDS
// (clamped into the action space where it is read) and nothing is stored per step; else it is row k of the caller's [K][N]
// arrays, step k + 1's loaded while step k is walked, and the step's outputs are stores nothing waits for.
// PID: the controller is the PID on the env's own gains (the step's text included under GW_CTRL_PID), its four f64 loaded from
// g and held in registers across the K steps, `last` cleared by the in-launch reset and stored back once; else g is not read.
// DIST (with PID): every plant substep ends with a draw of the env's own noise (the text under GW_CTRL_DIST as well), its record
// loaded from w and held in registers, the count of draws stored back once; the in-launch reset leaves it alone -- a reset env's
// plant goes on drawing where the old one stopped.  Else w is not read.
// LOSS (with PID and DIST): every transmission takes a draw of the env's own erasures (the text under GW_CTRL_LOSS as well), the
// record loaded from x and held in registers, the count of draws and the four erasure counts stored back once; the in-launch
// reset leaves it alone, for the disturbance's reason.  Else x is not read: it is the last parameter, and defaulted.
// (A __forceinline__ template, not a kernel: the kernels are plain functions.)
template <bool SCHED, bool PID, bool DIST, bool LOSS = false>
__device__ __forceinline__ void ctrl_rollout_lane(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w,
                                                  const int steps, const bool episodes, const uint32_t max_steps, const double fail_deg,
                                                  const uint8_t* s_trans, const double* s_ber, double* col0, double* col1, const int64_t e,
                                                  const int32_t* __restrict__ device, const int32_t* __restrict__ duration,
                                                  int32_t* __restrict__ obs, float* __restrict__ reward,
                                                  double* __restrict__ angle_deg, uint8_t* __restrict__ ended,
                                                  const uint8_t* s_sched, const uint32_t Ls, double* __restrict__ tally,
                                                  const GwCtrlLoss& x = GwCtrlLoss{nullptr})
{
    static_assert(PID || !DIST, "the disturbance instantiations are PID instantiations");
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
    uint32_t age = 0u;
    double cost = 0.0;
    if (episodes) { age = s.age[e]; cost = s.cost[e]; }
    const double deg_per_rad = 180.0 / 3.141592653589793;

    uint32_t at_sched = 0u, n_ended = 0u, n_failed = 0u;    // SCHED: the entry the env acts on next, and its tally
    double cost_ended = 0.0;
    int d_next = 0, du_next = 0;
    if (SCHED) at_sched = age % Ls;
    else if (steps > 0) { d_next = device[e]; du_next = duration[e]; }

    for (int step = 0; step < steps; ++step) {
        const int64_t at = (int64_t)step * c.N + e;
        int d_now, du_now;
        if (SCHED) {                                          // a byte outside the action space is clamped where it is read
            d_now = (int)gw_min_u32((uint32_t)s_sched[at_sched * 2u], 1u);
            du_now = (int)gw_min_u32((uint32_t)s_sched[at_sched * 2u + 1u], (uint32_t)k.max_duration - 1u);
        } else {
            d_now = d_next; du_now = du_next;
            if (step + 1 < steps) { d_next = device[at + c.N]; du_next = duration[at + c.N]; }
        }
        const int d = d_now, du = du_now;
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
        if (!SCHED) {
            obs[at] = (int32_t)deg;
            reward[at] = (float)fabs(180.0 - deg);
            if (angle_deg) angle_deg[at] = deg;
        }
        q_flush(q0, ring0, col0);
        q_flush(q1, ring1, col1);
        if (episodes) {                                       // the episode rule: the step's own outputs stand, then the env is reset
            age++;
            cost = cost + fabs(deg);
            const uint32_t cause = ((max_steps > 0u && age == max_steps) ? 1u : 0u) | ((fail_deg > 0.0 && fabs(deg) > fail_deg) ? 2u : 0u);
            if (!SCHED) ended[at] = (uint8_t)cause;
            at_sched = at_sched + 1u == Ls ? 0u : at_sched + 1u;
            if (cause) {                                      // gw_ctrl_reset for this one env, in registers; flags are sticky
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
    }

    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));
#pragma unroll
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl;
    if (episodes) { s.age[e] = age; s.cost[e] = cost; }
    if (PID) pid_store(G, g, e);
    if (DIST) dist_store(W, w, e);
    if (LOSS) loss_store(X, x, e);
    if (SCHED) {
        tally[e * 4 + 0] = (double)n_ended; tally[e * 4 + 1] = (double)n_failed;
        tally[e * 4 + 2] = (double)steps;   tally[e * 4 + 3] = cost_ended;
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP; }

} // namespace
