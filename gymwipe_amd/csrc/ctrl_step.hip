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
//     queues -angle_deg, and ctrl_step_kernel has exactly that compiled in; the other three kernels read the gains;
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
// Four kernels, one per variant of a handle: the default rule; the gains of gw_ctrl_set_gains; with them the plant disturbance of
// gw_ctrl_set_disturbance; with both the packet erasures of gw_ctrl_set_loss.  Each is its argument list -- the parent's, then
// its blocks, last and in the order g, w, x (ctrl_rollout.hip says why last) -- around one text, ctrl_step_kernel_body.h.
#include "ctrl_common.hip.h"

using namespace gwk;

namespace {

__global__ __launch_bounds__(64) void ctrl_step_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                       const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                       float* __restrict__ reward, double* __restrict__ angle_deg)
{
    constexpr bool PID = false, DIST = false, LOSS = false;
    const GwCtrlPid g{nullptr};
    const GwCtrlDist w{nullptr};
    const GwCtrlLoss x{nullptr};
#include "ctrl_step_kernel_body.h"
}

__global__ __launch_bounds__(64) void ctrl_step_pid_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                           const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                           float* __restrict__ reward, double* __restrict__ angle_deg, GwCtrlPid g)
{
    constexpr bool PID = true, DIST = false, LOSS = false;
    const GwCtrlDist w{nullptr};
    const GwCtrlLoss x{nullptr};
#include "ctrl_step_kernel_body.h"
}

__global__ __launch_bounds__(64) void ctrl_step_dist_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                            const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                            float* __restrict__ reward, double* __restrict__ angle_deg, GwCtrlPid g,
                                                            GwCtrlDist w)
{
    constexpr bool PID = true, DIST = true, LOSS = false;
    const GwCtrlLoss x{nullptr};
#include "ctrl_step_kernel_body.h"
}

__global__ __launch_bounds__(64) void ctrl_step_loss_kernel(GwCtrlDev c, const int32_t* __restrict__ device,
                                                            const int32_t* __restrict__ duration, int32_t* __restrict__ obs,
                                                            float* __restrict__ reward, double* __restrict__ angle_deg, GwCtrlPid g,
                                                            GwCtrlDist w, GwCtrlLoss x)
{
    constexpr bool PID = true, DIST = true, LOSS = true;
#include "ctrl_step_kernel_body.h"
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

int gw_ctrl_launch_step(const GwCtrlDev& c, const GwCtrlBlocks& v, const int32_t* device, const int32_t* duration, int32_t* obs,
                        float* reward, double* angle_deg, void* stream)
{
    return launch_variant(v, ctrl_step_kernel, ctrl_step_pid_kernel, ctrl_step_dist_kernel, ctrl_step_loss_kernel,
                          dim3((unsigned)((c.N + 63) / 64)), stream, c, device, duration, obs, reward, angle_deg);
}

int gw_ctrl_launch_init(const GwCtrlDev& c, const double* x0, double u0, void* stream)
{
    hipLaunchKernelGGL(ctrl_init_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, x0[0], x0[1], x0[2],
                       x0[3], u0);
    return launched();
}
