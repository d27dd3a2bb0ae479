// ctrl_rollout.hip -- the closed control loop beyond one step per launch: per-env initial states, gains, disturbance and loss
// records and reset (small kernels), and K steps fused into one launch, with optional episodes (gw_ctrl_rollout) or with P cyclic
// schedules read from LDS and only a per-env tally written (gw_ctrl_rollout_schedules).  BUILDER-DEFINED as the whole control
// loop is; the specification is the event-driven ControlLoopModel of the test infrastructure, a reset env being a freshly
// constructed model of its own x0 / u0.
// The step is ctrl_step_kernel's, from the same text (ctrl_step_body.h).  What fusion changes around it: the link tables go to
// LDS once per launch, the env's state stays in registers across the K steps and is loaded and stored once; a step's appends
// are still staged in the lane's LDS columns and flushed to its rings at the end of each step, and the head prefetch stays
// per step -- a lane only ever reads ring slots it wrote itself, in program order (or the zeros gw_ctrl_create left there).
// Two kernel shapes, each in the four variants of a handle (ctrl_step.hip lists them) around one lane loop.
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

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
// reset leaves it alone, for the disturbance's reason.  Else x is not read.
// (A __forceinline__ template, not a kernel: the kernels are plain functions.)
template <bool SCHED, bool PID, bool DIST, bool LOSS>
__device__ __forceinline__ void ctrl_rollout_lane(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w,
                                                  const GwCtrlLoss& x, const int steps, const bool episodes, const uint32_t max_steps,
                                                  const double fail_deg, const uint8_t* s_trans, const double* s_ber, double* col0,
                                                  double* col1, const int64_t e, const int32_t* __restrict__ device,
                                                  const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                  float* __restrict__ reward, double* __restrict__ angle_deg,
                                                  uint8_t* __restrict__ ended, const uint8_t* s_sched, const uint32_t Ls,
                                                  double* __restrict__ tally)
{
    static_assert(PID || !DIST, "the disturbance instantiations are PID instantiations");
    static_assert(DIST || !LOSS, "the loss instantiations are disturbance instantiations");
    CTRL_LANE_LOAD();
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
#include "ctrl_step_variant.h"
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
            if (cause) { CTRL_LANE_RESET(); }
        }
    }

    CTRL_LANE_STORE();
    if (episodes) { s.age[e] = age; s.cost[e] = cost; }
    if (PID) pid_store(G, g, e);
    if (DIST) dist_store(W, w, e);
    if (LOSS) loss_store(X, x, e);
    if (SCHED) {
        tally[e * 4 + 0] = (double)n_ended; tally[e * 4 + 1] = (double)n_failed;
        tally[e * 4 + 2] = (double)steps;   tally[e * 4 + 3] = cost_ended;
    }
}

// every 64-env block follows one schedule (the host refuses N / P that is no multiple of 64): its 2 Ls bytes -> s_sched in LDS.
// (Text: as a function it commuted two operands of one multiply in the four schedule kernels.)
#define STAGE_SCHEDULE()                                                                                                           \
    const uint32_t p = (uint32_t)(((int64_t)blockIdx.x * 64) / envs_per_schedule);                                                 \
    for (uint32_t i = threadIdx.x; i < 2u * Ls && i < (uint32_t)SCHED_MAX * 2u; i += blockDim.x) s_sched[i] = sched[(size_t)p * 2u * Ls + i]

// a kernel's call of its lane: the variant's flags and blocks (an empty one where the flag is false: not read) are the kernel's
// own, the rest is the shape's -- its arguments by their names, and nothing for the other shape's
#define ROWS_LANE(PID, DIST, LOSS, g, w, x)                                                                                        \
    ctrl_rollout_lane<false, PID, DIST, LOSS>(c, s, g, w, x, steps, episodes != 0, max_steps, fail_deg, s_trans, s_ber, col0, col1, e, \
                                              device, duration, obs, reward, angle_deg, ended, nullptr, 1u, nullptr)
#define SCHED_LANE(PID, DIST, LOSS, g, w, x)                                                                                       \
    ctrl_rollout_lane<true, PID, DIST, LOSS>(c, s, g, w, x, steps, true, max_steps, fail_deg, s_trans, s_ber, col0, col1, e, nullptr,  \
                                             nullptr, nullptr, nullptr, nullptr, nullptr, s_sched, Ls, tally)

// The variants' blocks are the LAST arguments, in the order g, w, x: with the gains' block in front of `steps` the schedule
// kernel came out with a 68-byte private segment that no instruction touches; behind the parents' arguments, whose offsets then
// stay what they are, it has none.
__global__ __launch_bounds__(64) void ctrl_rollout_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                          double fail_deg, const int32_t* __restrict__ device,
                                                          const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                          float* __restrict__ reward, double* __restrict__ angle_deg,
                                                          uint8_t* __restrict__ ended)
{
    CTRL_KERNEL_OPEN();
    ROWS_LANE(false, false, false, GwCtrlPid{}, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                              double fail_deg, const int32_t* __restrict__ device,
                                                              const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                              float* __restrict__ reward, double* __restrict__ angle_deg,
                                                              uint8_t* __restrict__ ended, GwCtrlPid g)
{
    CTRL_KERNEL_OPEN();
    ROWS_LANE(true, false, false, g, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_dist_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                               double fail_deg, const int32_t* __restrict__ device,
                                                               const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                               float* __restrict__ reward, double* __restrict__ angle_deg,
                                                               uint8_t* __restrict__ ended, GwCtrlPid g, GwCtrlDist w)
{
    CTRL_KERNEL_OPEN();
    ROWS_LANE(true, true, false, g, w, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                               double fail_deg, const int32_t* __restrict__ device,
                                                               const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                               float* __restrict__ reward, double* __restrict__ angle_deg,
                                                               uint8_t* __restrict__ ended, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
{
    CTRL_KERNEL_OPEN();
    ROWS_LANE(true, true, true, g, w, x);
}

__global__ __launch_bounds__(64) void ctrl_rollout_sched_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                uint32_t Ls, double* __restrict__ tally)
{
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    CTRL_KERNEL_OPEN(STAGE_SCHEDULE());
    SCHED_LANE(false, false, false, GwCtrlPid{}, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_sched_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                    const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                    uint32_t Ls, double* __restrict__ tally, GwCtrlPid g)
{
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    CTRL_KERNEL_OPEN(STAGE_SCHEDULE());
    SCHED_LANE(true, false, false, g, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_sched_dist_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                     const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                     uint32_t Ls, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w)
{
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    CTRL_KERNEL_OPEN(STAGE_SCHEDULE());
    SCHED_LANE(true, true, false, g, w, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_sched_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                     const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                     uint32_t Ls, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w,
                                                                     GwCtrlLoss x)
{
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    CTRL_KERNEL_OPEN(STAGE_SCHEDULE());
    SCHED_LANE(true, true, true, g, w, x);
}

// x_init / u_init of every env <- one state (gw_ctrl_create); the episode record starts at 0
__global__ void ctrl_fill_initial_kernel(int64_t N, GwCtrlEpi s, double x0, double x1, double x2, double x3, double u0)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    s.x_init[e * 4 + 0] = x0; s.x_init[e * 4 + 1] = x1; s.x_init[e * 4 + 2] = x2; s.x_init[e * 4 + 3] = x3;
    s.u_init[e] = u0;
    s.age[e] = 0u; s.cost[e] = 0.0;
}

__global__ void ctrl_set_initial_kernel(int64_t N, GwCtrlEpi s, const double* __restrict__ x0, const double* __restrict__ u0,
                                        const uint8_t* __restrict__ mask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    for (int i = 0; i < 4; ++i) s.x_init[e * 4 + i] = x0[e * 4 + i];
    if (u0) s.u_init[e] = u0[e];
}

// the gains of the masked envs <- gains[N][3]; last_error, the block's fourth column, is running state and is not touched
__global__ void ctrl_set_gains_kernel(int64_t N, GwCtrlPid g, const double* __restrict__ gains, const uint8_t* __restrict__ mask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    for (int i = 0; i < 3; ++i) g.pid[e * 4 + i] = gains[e * 3 + i];
}

// the record of the masked envs <- {g[e][0..3], key[e], n = 0}: the count of draws restarts with the record and with nothing else
__global__ void ctrl_set_disturbance_kernel(int64_t N, GwCtrlDist w, const double* __restrict__ g, const uint64_t* __restrict__ key,
                                            const uint8_t* __restrict__ mask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    for (int i = 0; i < 4; ++i) w.rec[e * 6 + i] = (uint64_t)__double_as_longlong(g[e * 4 + i]);
    w.rec[e * 6 + 4] = key[e];
    w.rec[e * 6 + 5] = 0ull;
}

// the record of the masked envs <- {thr[e][0..3], key[e], n = 0, lost = 0}: the count of draws and the erasure counts restart
// with the record and with nothing else
__global__ void ctrl_set_loss_kernel(int64_t N, GwCtrlLoss x, const uint32_t* __restrict__ thr, const uint64_t* __restrict__ key,
                                     const uint8_t* __restrict__ mask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    x.rec[e * 6 + 0] = (uint64_t)thr[e * 4 + 0] | ((uint64_t)thr[e * 4 + 1] << 32);
    x.rec[e * 6 + 1] = (uint64_t)thr[e * 4 + 2] | ((uint64_t)thr[e * 4 + 3] << 32);
    x.rec[e * 6 + 2] = key[e];
    x.rec[e * 6 + 3] = 0ull;
    x.rec[e * 6 + 4] = 0ull;
    x.rec[e * 6 + 5] = 0ull;
}

// the controller's part of a reset, launched behind ctrl_reset_kernel on a handle with gains set (a kernel of its own: that
// one keeps its code): the last error of the masked envs <- 0; the gains survive a reset, as x_init does
__global__ void ctrl_reset_pid_kernel(int64_t N, GwCtrlPid g, const uint8_t* __restrict__ mask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    g.pid[e * 4 + 3] = 0.0;
}

// the masked envs -> exactly what ctrl_init_kernel leaves, with the env's own initial state; flags stay (sticky)
__global__ void ctrl_reset_kernel(GwCtrlDev c, GwCtrlEpi s, const uint8_t* __restrict__ mask, int32_t* __restrict__ obs)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    double angle = c.x[e * 4 + 2];
    if (!mask || mask[e]) {
        c.now[e] = 0.0; c.wake[e] = 0.0; c.u[e] = s.u_init[e]; c.ang[e] = 0.0; c.ktick[e] = 0u;
        for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = s.x_init[e * 4 + i];
        angle = s.x_init[e * 4 + 2];
        c.qhl[e] = 0; c.qhl[c.N + e] = 0;
        for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = 0;
        c.got[e * 2] = 0u; c.got[e * 2 + 1] = 0u;
        c.ntx[e] = 0u; c.ncmd[e] = 0u; c.nsub[e] = 0u;
        s.age[e] = 0u; s.cost[e] = 0.0;
    }
    if (obs) obs[e] = (int32_t)(angle * (180.0 / 3.141592653589793));
}

inline dim3 grid256(const GwCtrlDev& c) { return dim3((unsigned)((c.N + 255) / 256)); }

} // namespace

int gw_ctrl_launch_fill_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, double u0, void* stream)
{
    hipLaunchKernelGGL(ctrl_fill_initial_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, s, x0[0], x0[1], x0[2], x0[3], u0);
    return launched();
}

int gw_ctrl_launch_set_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, const double* u0, const uint8_t* mask,
                               void* stream)
{
    hipLaunchKernelGGL(ctrl_set_initial_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, s, x0, u0, mask);
    return launched();
}

int gw_ctrl_launch_set_gains(const GwCtrlDev& c, const GwCtrlPid& g, const double* gains, const uint8_t* mask, void* stream)
{
    hipLaunchKernelGGL(ctrl_set_gains_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, g, gains, mask);
    return launched();
}

int gw_ctrl_launch_set_disturbance(const GwCtrlDev& c, const GwCtrlDist& w, const double* g, const uint64_t* key, const uint8_t* mask,
                                   void* stream)
{
    hipLaunchKernelGGL(ctrl_set_disturbance_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, w, g, key, mask);
    return launched();
}

int gw_ctrl_launch_set_loss(const GwCtrlDev& c, const GwCtrlLoss& x, const uint32_t* thr, const uint64_t* key, const uint8_t* mask,
                            void* stream)
{
    hipLaunchKernelGGL(ctrl_set_loss_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, x, thr, key, mask);
    return launched();
}

// (the disturbance's and the loss's records survive a reset: only the controller has a part in it)
int gw_ctrl_launch_reset(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, const uint8_t* mask, int32_t* obs, void* stream)
{
    hipLaunchKernelGGL(ctrl_reset_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c, s, mask, obs);
    if (v.g) hipLaunchKernelGGL(ctrl_reset_pid_kernel, grid256(c), dim3(256), 0, (hipStream_t)stream, c.N, *v.g, mask);
    return launched();
}

int gw_ctrl_launch_rollout(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps, const int32_t* device,
                           const int32_t* duration, const gw_ctrl_episodes* ep, int32_t* obs, float* reward, double* angle_deg,
                           uint8_t* ended, void* stream)
{
    return launch_variant(v, ctrl_rollout_kernel, ctrl_rollout_pid_kernel, ctrl_rollout_dist_kernel, ctrl_rollout_loss_kernel,
                          dim3((unsigned)((c.N + 63) / 64)), stream, c, s, (int)steps, ep ? 1 : 0, ep ? (uint32_t)ep->max_steps : 0u,
                          ep ? ep->fail_deg : 0.0, device, duration, obs, reward, angle_deg, ended);
}

int gw_ctrl_launch_rollout_schedules(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps, const uint8_t* sched,
                                     int32_t P, int32_t L, const gw_ctrl_episodes& ep, double* tally, void* stream)
{
    return launch_variant(v, ctrl_rollout_sched_kernel, ctrl_rollout_sched_pid_kernel, ctrl_rollout_sched_dist_kernel,
                          ctrl_rollout_sched_loss_kernel, dim3((unsigned)(c.N / 64)), stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                          ep.fail_deg, sched, (uint32_t)(c.N / P), (uint32_t)L, tally);
}
