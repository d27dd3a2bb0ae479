// ctrl_step_variant.h -- one step of the control loop in the including kernel's variant: ctrl_step_body.h under the symbols that
// the kernel's compile-time flags PID, DIST and LOSS stand for (each implies the ones before it).  Text included inside a
// kernel, as the body is and for its reason; the body's switches are preprocessor symbols, the kernels' are constants, and this
// is the one place that turns the second into the first.  What the body needs in scope is listed at its top; the branches not
// taken are discarded where they stand.
        if constexpr (LOSS) {
#define GW_CTRL_PID
#define GW_CTRL_DIST
#define GW_CTRL_LOSS
#include "ctrl_step_body.h"
#undef GW_CTRL_LOSS
#undef GW_CTRL_DIST
#undef GW_CTRL_PID
        } else if constexpr (DIST) {
#define GW_CTRL_PID
#define GW_CTRL_DIST
#include "ctrl_step_body.h"
#undef GW_CTRL_DIST
#undef GW_CTRL_PID
        } else if constexpr (PID) {
#define GW_CTRL_PID
#include "ctrl_step_body.h"
#undef GW_CTRL_PID
        } else {
#include "ctrl_step_body.h"
        }
