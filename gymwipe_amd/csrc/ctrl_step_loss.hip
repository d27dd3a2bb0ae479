// ctrl_step_loss.hip -- ctrl_step_loss_kernel (ctrl_step_dist.hip) with packets erased: the step's text under GW_CTRL_PID,
// GW_CTRL_DIST and GW_CTRL_LOSS, so that every transmission takes one draw of the env's own counter-based erasures
// (gw_ctrl_set_loss in include/gymwipe_amd.h).  The kernel a handle launches for a single step once a loss has been set on it.
// The same text around the same step, restated as that kernel restates ctrl_step_pid_kernel; what differs is X, loaded beside
// the lane's state, its count of draws and its four erasure counts stored back.  The loss block is the last kernel argument.
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

constexpr int S = GW_MAX_NSTATES;

__global__ __launch_bounds__(64) void ctrl_step_loss_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                            const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                            float* __restrict__ reward, double* __restrict__ angle_deg, GwCtrlPid g,
                                                            GwCtrlDist w, GwCtrlLoss x)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    double* col0 = s_new0 + (threadIdx.x & 63);
    double* col1 = s_new1 + (threadIdx.x & 63);
    const GwDevConst k = *(const GW_AS_CONST GwDevConst*)c.cst;
    Lane L;
    L.now = c.now[e]; L.wake = c.wake[e]; L.u = c.u[e]; L.ang = c.ang[e]; L.ktick = c.ktick[e];
    for (int i = 0; i < 4; ++i) L.x[i] = c.x[e * 4 + i];
    Q q0, q1;
    { const uint32_t hl = c.qhl[e]; q0.head = hl & 0xffu; q0.len = hl >> 8; }
    { const uint32_t hl = c.qhl[c.N + e]; q1.head = hl & 0xffu; q1.len = hl >> 8; }
    q_open(q0);
    q_open(q1);
#pragma unroll
    for (int j = 0; j < CR; ++j) L.rxs[j] = c.rxs[j * c.N + e];
    L.got1 = c.got[e * 2]; L.got2 = c.got[e * 2 + 1];
    L.ntx = c.ntx[e]; L.ncmd = c.ncmd[e]; L.nsub = c.nsub[e]; L.fl = c.flags[e];
    double* ring0 = c.pay + ((size_t)e * 2 + 0) * GW_RING_PHYS;
    double* ring1 = c.pay + ((size_t)e * 2 + 1) * GW_RING_PHYS;
    Pid G;
    pid_load(G, g, e);
    Dist W;
    dist_load(W, w, e);
    Loss X;
    loss_load(X, x, e);

    const int d = device[e], du = duration[e];
    const double deg_per_rad = 180.0 / 3.141592653589793;
#define GW_CTRL_PID
#define GW_CTRL_DIST
#define GW_CTRL_LOSS
#include "ctrl_step_body.h"
#undef GW_CTRL_LOSS
#undef GW_CTRL_DIST
#undef GW_CTRL_PID
    const double deg = L.x[2] * deg_per_rad;                                    // InvertedPendulumInterpreter, envs/inverted_pendulum.py:27-57
    obs[e] = (int32_t)deg;
    reward[e] = (float)fabs(180.0 - deg);
    if (angle_deg) angle_deg[e] = deg;

    q_flush(q0, ring0, col0);                                                   // this step's appends -> the rings
    q_flush(q1, ring1, col1);

    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));
#pragma unroll
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl;
    pid_store(G, g, e);
    dist_store(W, w, e);
    loss_store(X, x, e);
}

} // namespace

int gw_ctrl_launch_step_loss(const GwCtrlDev& c, const GwCtrlPid& g, const GwCtrlDist& w, const GwCtrlLoss& x, const int32_t* device,
                             const int32_t* duration, int32_t* obs, float* reward, double* angle_deg, void* stream)
{
    hipLaunchKernelGGL(ctrl_step_loss_kernel, dim3((unsigned)((c.N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, c, device, duration,
                       obs, reward, angle_deg, g, w, x);
    return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP;
}
