// ctrl_rollout.hip -- the closed control loop beyond one step per launch: per-env initial states and reset (small kernels), and
// K steps fused into one launch, with optional episodes (gw_ctrl_rollout) or with P cyclic schedules read from LDS and only a
// per-env tally written (gw_ctrl_rollout_schedules).  BUILDER-DEFINED as the whole control loop is; the specification is the
// event-driven ControlLoopModel of the test infrastructure, a reset env being a freshly constructed model of its own x0 / u0.
// The step is ctrl_step_kernel's, from the same text (ctrl_step_body.h).  What fusion changes around it: the link tables go to
// LDS once per launch, the env's state stays in registers across the K steps and is loaded and stored once; a step's appends
// are still staged in the lane's LDS columns and flushed to its rings at the end of each step, and the head prefetch stays
// per step -- a lane only ever reads ring slots it wrote itself, in program order (or the zeros gw_ctrl_create left there).
// The lane loop is ctrl_rollout_lane.hip.h, shared with the disturbance instantiations of the two fused kernels in
// ctrl_rollout_dist.hip.
#include "ctrl_rollout_lane.hip.h"

namespace {

__global__ __launch_bounds__(64) void ctrl_rollout_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                          double fail_deg, const int32_t* __restrict__ device,
                                                          const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                          float* __restrict__ reward, double* __restrict__ angle_deg,
                                                          uint8_t* __restrict__ ended)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_rollout_lane<false, false, false>(c, s, GwCtrlPid{nullptr}, GwCtrlDist{nullptr}, steps, episodes != 0, max_steps, fail_deg, s_trans, s_ber,
                                    s_new0 + (threadIdx.x & 63), s_new1 + (threadIdx.x & 63), e, device, duration, obs, reward, angle_deg, ended, nullptr, 1u, nullptr);
}

// every 64-env block follows one schedule (the host refuses N / P that is no multiple of 64): its 2 Ls bytes in LDS
__global__ __launch_bounds__(64) void ctrl_rollout_sched_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                uint32_t Ls, double* __restrict__ tally)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    const uint32_t p = (uint32_t)(((int64_t)blockIdx.x * 64) / envs_per_schedule);
    for (uint32_t i = threadIdx.x; i < 2u * Ls && i < (uint32_t)SCHED_MAX * 2u; i += blockDim.x) s_sched[i] = sched[(size_t)p * 2u * Ls + i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_rollout_lane<true, false, false>(c, s, GwCtrlPid{nullptr}, GwCtrlDist{nullptr}, steps, true, max_steps, fail_deg, s_trans, s_ber,
                                   s_new0 + (threadIdx.x & 63), s_new1 + (threadIdx.x & 63), e, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s_sched, Ls, tally);
}

// The two kernels above in their PID instantiation: what a handle launches once gw_ctrl_set_gains has been called on it.  The
// gains' block is the LAST argument: in front of `steps` the schedule kernel came out with a 68-byte private segment that no
// instruction touches; behind the parents' arguments, whose offsets then stay what they are, it has none.
__global__ __launch_bounds__(64) void ctrl_rollout_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                          double fail_deg, const int32_t* __restrict__ device,
                                                          const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                          float* __restrict__ reward, double* __restrict__ angle_deg,
                                                          uint8_t* __restrict__ ended, GwCtrlPid g)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_rollout_lane<false, true, false>(c, s, g, GwCtrlDist{nullptr}, steps, episodes != 0, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                             s_new1 + (threadIdx.x & 63), e, device, duration, obs, reward, angle_deg, ended, nullptr, 1u, nullptr);
}

__global__ __launch_bounds__(64) void ctrl_rollout_sched_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                uint32_t Ls, double* __restrict__ tally, GwCtrlPid g)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    __shared__ uint8_t s_sched[SCHED_MAX * 2];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    const uint32_t p = (uint32_t)(((int64_t)blockIdx.x * 64) / envs_per_schedule);
    for (uint32_t i = threadIdx.x; i < 2u * Ls && i < (uint32_t)SCHED_MAX * 2u; i += blockDim.x) s_sched[i] = sched[(size_t)p * 2u * Ls + i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_rollout_lane<true, true, false>(c, s, g, GwCtrlDist{nullptr}, steps, true, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                            s_new1 + (threadIdx.x & 63), e, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s_sched, Ls, tally);
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

} // namespace

int gw_ctrl_launch_fill_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, double u0, void* stream)
{
    hipLaunchKernelGGL(ctrl_fill_initial_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c.N, s, x0[0],
                       x0[1], x0[2], x0[3], u0);
    return launched();
}

int gw_ctrl_launch_set_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, const double* u0, const uint8_t* mask,
                               void* stream)
{
    hipLaunchKernelGGL(ctrl_set_initial_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c.N, s, x0, u0,
                       mask);
    return launched();
}

int gw_ctrl_launch_set_gains(const GwCtrlDev& c, const GwCtrlPid& g, const double* gains, const uint8_t* mask, void* stream)
{
    hipLaunchKernelGGL(ctrl_set_gains_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c.N, g, gains, mask);
    return launched();
}

int gw_ctrl_launch_reset(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid* g, const uint8_t* mask, int32_t* obs, void* stream)
{
    const dim3 grid((unsigned)((c.N + 255) / 256)), block(256);
    hipLaunchKernelGGL(ctrl_reset_kernel, grid, block, 0, (hipStream_t)stream, c, s, mask, obs);
    if (g) hipLaunchKernelGGL(ctrl_reset_pid_kernel, grid, block, 0, (hipStream_t)stream, c.N, *g, mask);
    return launched();
}

int gw_ctrl_launch_rollout(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid* g, int32_t steps, const int32_t* device,
                           const int32_t* duration, const gw_ctrl_episodes* ep, int32_t* obs, float* reward, double* angle_deg,
                           uint8_t* ended, void* stream)
{
    const dim3 grid((unsigned)((c.N + 63) / 64)), block(64);
    const int episodes = ep ? 1 : 0;
    const uint32_t max_steps = ep ? (uint32_t)ep->max_steps : 0u;
    const double fail_deg = ep ? ep->fail_deg : 0.0;
    if (g)
        hipLaunchKernelGGL(ctrl_rollout_pid_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, episodes, max_steps, fail_deg, device,
                           duration, obs, reward, angle_deg, ended, *g);
    else
        hipLaunchKernelGGL(ctrl_rollout_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, episodes, max_steps, fail_deg, device,
                           duration, obs, reward, angle_deg, ended);
    return launched();
}

int gw_ctrl_launch_rollout_schedules(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid* g, int32_t steps, const uint8_t* sched,
                                     int32_t P, int32_t L, const gw_ctrl_episodes& ep, double* tally, void* stream)
{
    const dim3 grid((unsigned)(c.N / 64)), block(64);
    if (g)
        hipLaunchKernelGGL(ctrl_rollout_sched_pid_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, sched, (uint32_t)(c.N / P), (uint32_t)L, tally, *g);
    else
        hipLaunchKernelGGL(ctrl_rollout_sched_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, sched, (uint32_t)(c.N / P), (uint32_t)L, tally);
    return launched();
}
