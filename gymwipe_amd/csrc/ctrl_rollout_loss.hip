// ctrl_rollout_loss.hip -- the two fused kernels of ctrl_rollout.hip in their loss instantiation, and the kernel that sets an
// env's loss record: what a handle launches once gw_ctrl_set_loss has been called on it.  The controller is the PID on the env's
// own gains, every plant substep ends with one draw of the env's own noise, and every transmission takes one draw of the env's
// own erasures (ctrl_step_body.h under GW_CTRL_PID, GW_CTRL_DIST and GW_CTRL_LOSS; the rule is stated in
// include/gymwipe_amd.h).  The same lane loop (ctrl_rollout_lane.hip.h) around the same step; a file of its own, as
// ctrl_rollout_dist.hip is.  The gains', the disturbance's and the loss's blocks are the last kernel arguments, in that order.
#include "ctrl_rollout_lane.hip.h"

namespace {

__global__ __launch_bounds__(64) void ctrl_rollout_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, int episodes, uint32_t max_steps,
                                                               double fail_deg, const int32_t* __restrict__ device,
                                                               const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                               float* __restrict__ reward, double* __restrict__ angle_deg,
                                                               uint8_t* __restrict__ ended, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_rollout_lane<false, true, true, true>(c, s, g, w, steps, episodes != 0, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                         s_new1 + (threadIdx.x & 63), e, device, duration, obs, reward, angle_deg, ended, nullptr, 1u, nullptr, x);
}

// every 64-env block follows one schedule (the host refuses N / P that is no multiple of 64): its 2 Ls bytes in LDS
__global__ __launch_bounds__(64) void ctrl_rollout_sched_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                     const uint8_t* __restrict__ sched, uint32_t envs_per_schedule,
                                                                     uint32_t Ls, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
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
    ctrl_rollout_lane<true, true, true, true>(c, s, g, w, steps, true, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                        s_new1 + (threadIdx.x & 63), e, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s_sched, Ls, tally, x);
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

} // namespace

int gw_ctrl_launch_set_loss(const GwCtrlDev& c, const GwCtrlLoss& x, const uint32_t* thr, const uint64_t* key, const uint8_t* mask,
                            void* stream)
{
    hipLaunchKernelGGL(ctrl_set_loss_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c.N, x, thr, key, mask);
    return launched();
}

int gw_ctrl_launch_rollout_loss(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w, const GwCtrlLoss& x,
                                int32_t steps, const int32_t* device, const int32_t* duration, const gw_ctrl_episodes* ep, int32_t* obs,
                                float* reward, double* angle_deg, uint8_t* ended, void* stream)
{
    hipLaunchKernelGGL(ctrl_rollout_loss_kernel, dim3((unsigned)((c.N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, c, s, (int)steps,
                       ep ? 1 : 0, ep ? (uint32_t)ep->max_steps : 0u, ep ? ep->fail_deg : 0.0, device, duration, obs, reward, angle_deg,
                       ended, g, w, x);
    return launched();
}

int gw_ctrl_launch_rollout_schedules_loss(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w, const GwCtrlLoss& x,
                                          int32_t steps, const uint8_t* sched, int32_t P, int32_t L, const gw_ctrl_episodes& ep, double* tally,
                                          void* stream)
{
    hipLaunchKernelGGL(ctrl_rollout_sched_loss_kernel, dim3((unsigned)(c.N / 64)), dim3(64), 0, (hipStream_t)stream, c, s, (int)steps,
                       (uint32_t)ep.max_steps, ep.fail_deg, sched, (uint32_t)(c.N / P), (uint32_t)L, tally, g, w, x);
    return launched();
}
