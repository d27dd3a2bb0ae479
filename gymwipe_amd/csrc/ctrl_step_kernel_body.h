// ctrl_step_kernel_body.h -- what stands between the braces of the four step kernels of ctrl_step.hip: one lane per env, its
// state loaded, one step in the kernel's variant, the step's outputs and appends written, the state stored.  Text, as
// ctrl_step_body.h is and for its reason: as a __forceinline__ template called from the four kernels it moved three of them
// (profiles/ctrl_one_text/README.md).  The including kernel provides its arguments under the names of ctrl_step_kernel's, the
// variant's flags PID, DIST, LOSS and the blocks g, w, x (an empty one where its flag is false).
    CTRL_KERNEL_OPEN();
    CTRL_LANE_LOAD(q_open(q0); q_open(q1));

    const int d = device[e], du = duration[e];
    const double deg_per_rad = 180.0 / 3.141592653589793;
#include "ctrl_step_variant.h"
    const double deg = L.x[2] * deg_per_rad;                                    // InvertedPendulumInterpreter, envs/inverted_pendulum.py:27-57
    obs[e] = (int32_t)deg;
    reward[e] = (float)fabs(180.0 - deg);
    if (angle_deg) angle_deg[e] = deg;

    q_flush(q0, ring0, col0);                                                   // this step's appends -> the rings
    q_flush(q1, ring1, col1);

    CTRL_LANE_STORE();
    if (PID) pid_store(G, g, e);
    if (DIST) dist_store(W, w, e);
    if (LOSS) loss_store(X, x, e);
