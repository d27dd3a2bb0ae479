// ctrl_step.hip -- SURVEY 8f rank 2, second half: the pendulum env's control loop CLOSED over the receive-mode MACs.
//
// BUILDER-DEFINED (the reference never runs this loop: nobody sets `receiving`, and its env cannot be constructed);
// the specification this kernel is held to, bit for bit, is the event-driven ControlLoopModel of the test
// infrastructure.  Three network devices -- sensor (0), controller (1), actuator (2, not assignable) -- and the RRM:
//   * every counter tick the sensor queues the plant's angle for the controller, then the plant advances one
//     substep x <- A x + B u (plants/sliding_pendulum.py:116-135, plants/core.py:38-49);
//   * every `period` ticks from tick `start` on the controller runs the reference's three-term PID rule
//     (control/inverted_pendulum.py:46-69; stated in include/gymwipe_amd.h at gw_ctrl_set_gains) on gains of its env's own and
//     queues the result for the actuator unless its angle is 0.  Their default, the reference's shipped kp = 1, ki = kd = 0,
//     queues -angle_deg, and ctrl_step_kernel has exactly that compiled in; ctrl_step_pid_kernel reads the gains;
//   * a data packet decoded by its destination's receive-mode MAC is handed up: the controller takes degrees(value)
//     as its angle (:39-41), the actuator takes value as the motor velocity (sliding_pendulum.py:154-155);
//   * band assignment, announcement, window loop, slot alignment, BER integration, decode: exactly the step of
//     ct_step.hip, whose helpers are shared.
// One lane per environment; both MAC queues are explicit rings of payload values (packet sizes are constant); a step's
// appends are staged in LDS and flushed once, the addressed queue's head is prefetched.
// Event order at equal times follows the insertion rule: a tick at t runs BEFORE the delivery of a transmission that ends
// at t.  The tick's event was queued one interval ago; the delivery is not the transmission's completion event itself but
// two events further on (the receiving MAC's process starts, then hands the payload up), both queued at t, behind the tick.
// So the controller answers, and the plant moves, on what they held before the packet.  A tick on the step's end belongs to
// the step.  Either tie raises GW_FLAG_TIE.
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

constexpr int S = GW_MAX_NSTATES;

__global__ __launch_bounds__(64) void ctrl_step_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                       const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                       float* __restrict__ reward, double* __restrict__ angle_deg)
{
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];
    // the noise-state transitions and the BER per (listener, talker, state): looked up for every radio at every transmission
    // (a window of the sensor's queue is dozens of them) -- from LDS, not a dependent global round trip apiece
    __shared__ uint8_t s_trans[CR * CR * S];
    __shared__ double s_ber[CR * CR * S];
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    double* col0 = s_new0 + (threadIdx.x & 63);
    double* col1 = s_new1 + (threadIdx.x & 63);
    // (the handle's constants by value through the constant address space: scalar loads the compiler may hoist and keep)
    const GwDevConst k = *(const GW_AS_CONST GwDevConst*)c.cst;
    Lane L;
    L.now = c.now[e]; L.wake = c.wake[e]; L.u = c.u[e]; L.ang = c.ang[e]; L.ktick = c.ktick[e];
    for (int i = 0; i < 4; ++i) L.x[i] = c.x[e * 4 + i];
    Q q0, q1;
    { const uint32_t hl = c.qhl[e]; q0.head = hl & 0xffu; q0.len = hl >> 8; }
    { const uint32_t hl = c.qhl[c.N + e]; q1.head = hl & 0xffu; q1.len = hl >> 8; }
    q0.app = q1.app = 0u;
    q0.head0 = q0.head; q1.head0 = q1.head;
    q0.tail0 = (q0.head + q0.len) & GW_RING_MASK; q1.tail0 = (q1.head + q1.len) & GW_RING_MASK;
#pragma unroll
    for (int j = 0; j < CR; ++j) L.rxs[j] = c.rxs[j * c.N + e];
    L.got1 = c.got[e * 2]; L.got2 = c.got[e * 2 + 1];
    L.ntx = c.ntx[e]; L.ncmd = c.ncmd[e]; L.nsub = c.nsub[e]; L.fl = c.flags[e];
    double* ring0 = c.pay + ((size_t)e * 2 + 0) * GW_RING_PHYS;
    double* ring1 = c.pay + ((size_t)e * 2 + 1) * GW_RING_PHYS;

    const int d = device[e], du = duration[e];
    const double deg_per_rad = 180.0 / 3.141592653589793;
#include "ctrl_step_body.h"
    const double deg = L.x[2] * deg_per_rad;                                    // InvertedPendulumInterpreter, envs/inverted_pendulum.py:27-57
    obs[e] = (int32_t)deg;
    reward[e] = (float)fabs(180.0 - deg);
    if (angle_deg) angle_deg[e] = deg;

    // this step's appends -> the rings: value j of queue q sits in slot (tail0 + j) & mask
    for (uint32_t j = 0; j < q0.app; ++j) ring0[(q0.tail0 + j) & GW_RING_MASK] = col0[j << 6];
    for (uint32_t j = 0; j < q1.app; ++j) ring1[(q1.tail0 + j) & GW_RING_MASK] = col1[j << 6];

    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));
#pragma unroll
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl;
}

// ctrl_step_kernel with the controller's rule switched to the PID on per-env gains (ctrl_step_body.h under GW_CTRL_PID): the
// kernel a handle launches once gw_ctrl_set_gains has been called on it.  The same text around the same step, restated and not
// shared so that ctrl_step_kernel keeps its code; what differs is G, loaded beside the lane's state and its `last` stored back.
__global__ __launch_bounds__(64) void ctrl_step_pid_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                           const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                           float* __restrict__ reward, double* __restrict__ angle_deg, GwCtrlPid g)
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
    q0.app = q1.app = 0u;
    q0.head0 = q0.head; q1.head0 = q1.head;
    q0.tail0 = (q0.head + q0.len) & GW_RING_MASK; q1.tail0 = (q1.head + q1.len) & GW_RING_MASK;
#pragma unroll
    for (int j = 0; j < CR; ++j) L.rxs[j] = c.rxs[j * c.N + e];
    L.got1 = c.got[e * 2]; L.got2 = c.got[e * 2 + 1];
    L.ntx = c.ntx[e]; L.ncmd = c.ncmd[e]; L.nsub = c.nsub[e]; L.fl = c.flags[e];
    double* ring0 = c.pay + ((size_t)e * 2 + 0) * GW_RING_PHYS;
    double* ring1 = c.pay + ((size_t)e * 2 + 1) * GW_RING_PHYS;
    Pid G;
    pid_load(G, g, e);

    const int d = device[e], du = duration[e];
    const double deg_per_rad = 180.0 / 3.141592653589793;
#define GW_CTRL_PID
#include "ctrl_step_body.h"
#undef GW_CTRL_PID
    const double deg = L.x[2] * deg_per_rad;                                    // InvertedPendulumInterpreter, envs/inverted_pendulum.py:27-57
    obs[e] = (int32_t)deg;
    reward[e] = (float)fabs(180.0 - deg);
    if (angle_deg) angle_deg[e] = deg;

    // this step's appends -> the rings: value j of queue q sits in slot (tail0 + j) & mask
    for (uint32_t j = 0; j < q0.app; ++j) ring0[(q0.tail0 + j) & GW_RING_MASK] = col0[j << 6];
    for (uint32_t j = 0; j < q1.app; ++j) ring1[(q1.tail0 + j) & GW_RING_MASK] = col1[j << 6];

    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));
#pragma unroll
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl;
    pid_store(G, g, e);
}

__global__ void ctrl_init_kernel(GwCtrlDev c, double x0, double x1, double x2, double x3, double u0)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    c.now[e] = 0.0; c.wake[e] = 0.0; c.u[e] = u0; c.ang[e] = 0.0; c.ktick[e] = 0u;
    c.x[e * 4 + 0] = x0; c.x[e * 4 + 1] = x1; c.x[e * 4 + 2] = x2; c.x[e * 4 + 3] = x3;
    c.qhl[e] = 0; c.qhl[c.N + e] = 0;
    for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = 0;
    c.got[e * 2] = 0u; c.got[e * 2 + 1] = 0u;
    c.ntx[e] = 0u; c.ncmd[e] = 0u; c.nsub[e] = 0u; c.flags[e] = 0u;
}

} // namespace

int gw_ctrl_launch_step(const GwCtrlDev& c, const GwCtrlPid* g, const int32_t* device, const int32_t* duration, int32_t* obs,
                        float* reward, double* angle_deg, void* stream)
{
    const dim3 grid((unsigned)((c.N + 63) / 64)), block(64);
    if (g) hipLaunchKernelGGL(ctrl_step_pid_kernel, grid, block, 0, (hipStream_t)stream, c, device, duration, obs, reward, angle_deg, *g);
    else hipLaunchKernelGGL(ctrl_step_kernel, grid, block, 0, (hipStream_t)stream, c, device, duration, obs, reward, angle_deg);
    return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP;
}

int gw_ctrl_launch_init(const GwCtrlDev& c, const double* x0, double u0, void* stream)
{
    hipLaunchKernelGGL(ctrl_init_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, x0[0], x0[1], x0[2],
                       x0[3], u0);
    return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP;
}
