// ctrl_rollout_feedback_loss.hip -- the two kernels of ctrl_rollout_feedback.hip in their loss instantiation: the PID controller
// on the env's own gains, the env's own noise at the end of every plant substep and one draw of the env's own erasures per
// transmission (ctrl_step_body.h under GW_CTRL_PID, GW_CTRL_DIST and GW_CTRL_LOSS), what a handle launches once gw_ctrl_set_loss
// has been called on it.  The same lane loop (ctrl_feedback_lane.hip.h) around the same step; a file of its own, as
// ctrl_rollout_feedback_dist.hip is.  The gains', the disturbance's and the loss's blocks are the last kernel arguments.
#include "ctrl_feedback_lane.hip.h"

namespace {

__global__ __launch_bounds__(64) void ctrl_rollout_fb_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                  const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                  uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                  double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    __shared__ uint8_t s_sched[FB_BINS * FB_LEN_MAX * 2];
    __shared__ int32_t s_edges[FB_BINS - 1];
    __shared__ uint32_t s_par[2];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    stage_policy(s_sched, s_edges, s_par, sched, edges, envs_per_policy, B, Ls, abs_key);
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    const FbRows none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ctrl_feedback_lane<false, true, true, true>(c, s, g, w, steps, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                          s_new1 + (threadIdx.x & 63), e, s_sched, s_edges, s_par, none, tally, x);
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                       const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                       uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                       FbRows rows, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    __shared__ uint8_t s_sched[FB_BINS * FB_LEN_MAX * 2];
    __shared__ int32_t s_edges[FB_BINS - 1];
    __shared__ uint32_t s_par[2];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    stage_policy(s_sched, s_edges, s_par, sched, edges, envs_per_policy, B, Ls, abs_key);
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    ctrl_feedback_lane<true, true, true, true>(c, s, g, w, steps, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                         s_new1 + (threadIdx.x & 63), e, s_sched, s_edges, s_par, rows, tally, x);
}

} // namespace

int gw_ctrl_launch_rollout_feedback_loss(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w, const GwCtrlLoss& x,
                                         int32_t steps, const gw_ctrl_feedback& fb, const gw_ctrl_episodes& ep,
                                         const gw_ctrl_feedback_rows* rows, double* tally, void* stream)
{
    const dim3 grid((unsigned)(c.N / 64)), block(64);
    const uint32_t per = (uint32_t)(c.N / fb.num_policies);
    const int abs_key = (fb.flags & GW_CTRL_FB_ABS) ? 1 : 0;
    if (rows) {
        const FbRows r = {rows->device_out_dev, rows->duration_out_dev, rows->obs_dev, rows->reward_dev, rows->angle_deg_dev, rows->ended_dev};
        hipLaunchKernelGGL(ctrl_rollout_fb_rows_loss_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, fb.sched_dev, fb.edges_dev, per, (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, r, tally, g, w, x);
    } else {
        hipLaunchKernelGGL(ctrl_rollout_fb_loss_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, fb.sched_dev, fb.edges_dev, per, (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, tally, g, w, x);
    }
    return launched();
}
