// ctrl_rollout_feedback.hip -- angle-feedback band schedulers inside the fused control-loop rollout (gw_ctrl_rollout_feedback).
// Every env looks at its own pendulum before each step: the angle of its current state, truncated to the int32 observation, is
// sorted into one of B bins by the policy's B - 1 edges, and the step's action is entry `age % L` of that bin's cyclic schedule.
// P policies run in one launch, 64 envs per block, every block under one policy (the host refuses N / P that is no multiple of
// 64); the block's policy -- 2 B L schedule bytes and B - 1 edges, at most 1 052 bytes -- is staged into LDS beside the link
// tables and the two append columns, with L and the key's flag (8 bytes more: as kernel arguments they sat in scalar registers
// across the step's body, which has none to spare, and the spill reloads cost a quarter of the step's time).
// The step is ctrl_step_kernel's, from the same text (ctrl_step_body.h); the episode rule is ctrl_rollout.hip's, and the lane's
// load, store and in-launch reset are that file's, from the same text (ctrl_common.hip.h): the lane loop here is that file's loop
// with the action's source and the tally changed.  Two kernel shapes, without and with per-step rows, each in the four variants
// of a handle (ctrl_step.hip lists them).  The specification is tests/ctrl_feedback_model.py.
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

constexpr int FB_LEN_MAX = 64;                               // entries of one bin's schedule (1 <= L <= 64)
constexpr int FB_BINS = GW_CTRL_FB_MAX_BINS;

struct FbRows {                                              // gw_ctrl_feedback_rows, all [steps][N]
    int32_t *device_out, *duration_out, *obs;
    float* reward;
    double* angle_deg;
    uint8_t* ended;
};

// The loop of both kernels, one lane per env.  ROWS: row k receives the action taken and what gw_ctrl_rollout would write,
// stores nothing waits for.  PID, DIST, LOSS: the variant, as in ctrl_rollout.hip's loop -- the controller on the env's own
// gains; the plant disturbed, the env's record in registers and its count stored back once; every transmission under a draw of
// the env's own erasures, the record in registers, its count and erasure counts stored back once.  A reset clears the
// controller's last error and leaves the two records alone.  A block whose flag is false is not read.
// (A __forceinline__ template, not a kernel: the kernels below are plain functions.)
template <bool ROWS, bool PID, bool DIST, bool LOSS>
__device__ __forceinline__ void ctrl_feedback_lane(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlPid& g, const GwCtrlDist& w,
                                                   const GwCtrlLoss& x, const int steps, const uint32_t max_steps, const double fail_deg,
                                                   const uint8_t* s_trans, const double* s_ber, double* col0, double* col1,
                                                   const int64_t e, const uint8_t* s_sched, const int32_t* s_edges,
                                                   const uint32_t* s_par, const FbRows& r, double* __restrict__ tally)
{
    static_assert(PID || !DIST, "the disturbance instantiations are PID instantiations");
    static_assert(DIST || !LOSS, "the loss instantiations are disturbance instantiations");
    CTRL_LANE_LOAD();
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
#include "ctrl_step_variant.h"
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
        if (cause) { CTRL_LANE_RESET(); }
    }

    CTRL_LANE_STORE();
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

// A kernel's text between its braces: the policy's LDS and the kernel's opening, then its lane in the variant given -- the flags
// and blocks (an empty one where the flag is false) are the kernel's own, the rest its arguments by their names.
#define FB_KERNEL(ROWS, rows, PID, DIST, LOSS, g, w, x)                                                                            \
    __shared__ uint8_t s_sched[FB_BINS * FB_LEN_MAX * 2];                                                                          \
    __shared__ int32_t s_edges[FB_BINS - 1];                                                                                       \
    __shared__ uint32_t s_par[2];                                                                                                  \
    CTRL_KERNEL_OPEN(stage_policy(s_sched, s_edges, s_par, sched, edges, envs_per_policy, B, Ls, abs_key));                        \
    ctrl_feedback_lane<ROWS, PID, DIST, LOSS>(c, s, g, w, x, steps, max_steps, fail_deg, s_trans, s_ber, col0, col1, e, s_sched,   \
                                              s_edges, s_par, rows, tally)

// (the variants' blocks are the last arguments, in the order g, w, x: ctrl_rollout.hip says why)
__global__ __launch_bounds__(64) void ctrl_rollout_fb_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                             const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                             uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                             double* __restrict__ tally)
{
    FB_KERNEL(false, FbRows{}, false, false, false, GwCtrlPid{}, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                 const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                 uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                 double* __restrict__ tally, GwCtrlPid g)
{
    FB_KERNEL(false, FbRows{}, true, false, false, g, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_dist_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                  const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                  uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                  double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w)
{
    FB_KERNEL(false, FbRows{}, true, true, false, g, w, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                  const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                  uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                  double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w, GwCtrlLoss x)
{
    FB_KERNEL(false, FbRows{}, true, true, true, g, w, x);
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                  const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                  uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                  FbRows rows, double* __restrict__ tally)
{
    FB_KERNEL(true, rows, false, false, false, GwCtrlPid{}, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_pid_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                      const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                      uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                      FbRows rows, double* __restrict__ tally, GwCtrlPid g)
{
    FB_KERNEL(true, rows, true, false, false, g, GwCtrlDist{}, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_dist_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                       const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                       uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                       FbRows rows, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w)
{
    FB_KERNEL(true, rows, true, true, false, g, w, GwCtrlLoss{});
}

__global__ __launch_bounds__(64) void ctrl_rollout_fb_rows_loss_kernel(GwCtrlDev c, GwCtrlEpi s, int steps, uint32_t max_steps, double fail_deg,
                                                                       const uint8_t* __restrict__ sched, const int32_t* __restrict__ edges,
                                                                       uint32_t envs_per_policy, uint32_t B, uint32_t Ls, int abs_key,
                                                                       FbRows rows, double* __restrict__ tally, GwCtrlPid g, GwCtrlDist w,
                                                                       GwCtrlLoss x)
{
    FB_KERNEL(true, rows, true, true, true, g, w, x);
}

} // namespace

int gw_ctrl_launch_rollout_feedback(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps,
                                    const gw_ctrl_feedback& fb, const gw_ctrl_episodes& ep, const gw_ctrl_feedback_rows* rows,
                                    double* tally, void* stream)
{
    const dim3 grid((unsigned)(c.N / 64));
    const uint32_t per = (uint32_t)(c.N / fb.num_policies);
    const int abs_key = (fb.flags & GW_CTRL_FB_ABS) ? 1 : 0;
    if (!rows)
        return launch_variant(v, ctrl_rollout_fb_kernel, ctrl_rollout_fb_pid_kernel, ctrl_rollout_fb_dist_kernel, ctrl_rollout_fb_loss_kernel,
                              grid, stream, c, s, (int)steps, (uint32_t)ep.max_steps, ep.fail_deg, fb.sched_dev, fb.edges_dev, per,
                              (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, tally);
    const FbRows r = {rows->device_out_dev, rows->duration_out_dev, rows->obs_dev, rows->reward_dev, rows->angle_deg_dev, rows->ended_dev};
    return launch_variant(v, ctrl_rollout_fb_rows_kernel, ctrl_rollout_fb_rows_pid_kernel, ctrl_rollout_fb_rows_dist_kernel,
                          ctrl_rollout_fb_rows_loss_kernel, grid, stream, c, s, (int)steps, (uint32_t)ep.max_steps, ep.fail_deg,
                          fb.sched_dev, fb.edges_dev, per, (uint32_t)fb.num_bins, (uint32_t)fb.length, abs_key, r, tally);
}
