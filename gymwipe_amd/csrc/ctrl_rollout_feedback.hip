// ctrl_rollout_feedback.hip -- angle-feedback band schedulers inside the fused control-loop rollout (gw_ctrl_rollout_feedback).
// Every env looks at its own pendulum before each step: the angle of its current state, truncated to the int32 observation, is
// sorted into one of B bins by the policy's B - 1 edges, and the step's action is entry `age % L` of that bin's cyclic schedule.
// P policies run in one launch, 64 envs per block, every block under one policy (the host refuses N / P that is no multiple of
// 64); the block's policy -- 2 B L schedule bytes and B - 1 edges, at most 1 052 bytes -- is staged into LDS beside the link
// tables and the two append columns, with L and the key's flag (8 bytes more: as kernel arguments they sat in scalar registers
// across the step's body, which has none to spare, and the spill reloads cost a quarter of the step's time).  The step is ctrl_step_kernel's, from the same text (ctrl_step_body.h), and the episode
// rule and the in-launch reset are ctrl_rollout.hip's, restated so that its kernels keep their code: the lane loop
// (ctrl_feedback_lane.hip.h, shared with the PID instantiations of these two kernels in ctrl_rollout_feedback_pid.hip) is that
// file's loop with the action's source and the tally changed.  The specification is tests/ctrl_feedback_model.py.
#include "ctrl_feedback_lane.hip.h"

namespace {

__global__ __launch_bounds__(64) void ctrl_rollout_fb_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                             const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                             uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                             double* __restrict__ tally)
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
    ctrl_feedback_lane<false, false, false>(c, s, GwCtrlPid{nullptr}, GwCtrlDist{nullptr}, steps, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                     s_new1 + (threadIdx.x & 63), e, s_sched, s_edges, s_par, none, tally);
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                  const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                  uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                  FbRows rows, double* __restrict__ tally)
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
    ctrl_feedback_lane<true, false, false>(c, s, GwCtrlPid{nullptr}, GwCtrlDist{nullptr}, steps, max_steps, fail_deg, s_trans, s_ber, s_new0 + (threadIdx.x & 63),
                                    s_new1 + (threadIdx.x & 63), e, s_sched, s_edges, s_par, rows, tally);
}

} // namespace

int gw_ctrl_launch_rollout_feedback(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid* g, int32_t steps,
                                    const gw_ctrl_feedback& fb, const gw_ctrl_episodes& ep, const gw_ctrl_feedback_rows* rows,
                                    double* tally, void* stream)
{
    if (g) return gw_ctrl_launch_rollout_feedback_pid(c, s, *g, steps, fb, ep, rows, tally, stream);
    const dim3 grid((unsigned)(c.N / 64)), block(64);
    const uint32_t per = (uint32_t)(c.N / fb.num_policies);
    const int abs_key = (fb.flags & GW_CTRL_FB_ABS) ? 1 : 0;
    if (rows) {
        const FbRows r = {rows->device_out_dev, rows->duration_out_dev, rows->obs_dev, rows->reward_dev, rows->angle_deg_dev, rows->ended_dev};
        hipLaunchKernelGGL(ctrl_rollout_fb_rows_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, fb.sched_dev, fb.edges_dev, per, (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, r, tally);
    } else {
        hipLaunchKernelGGL(ctrl_rollout_fb_kernel, grid, block, 0, (hipStream_t)stream, c, s, (int)steps, (uint32_t)ep.max_steps,
                           ep.fail_deg, fb.sched_dev, fb.edges_dev, per, (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, tally);
    }
    return launched();
}
