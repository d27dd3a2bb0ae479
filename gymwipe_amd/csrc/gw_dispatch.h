// gw_dispatch.h -- how the launchers (ct_step*.hip, ct_rollout_*.hip) get from a handle's run-time values to ONE kernel
// instantiation: nested around a generic lambda that names the kernel,
//     gw_with_dt<GW_DTS_LIVE>(st.D, [&](auto dt) { gw_with_flag(st.prx_env != nullptr, [&](auto per_env) {
//         hipLaunchKernelGGL((ct_step_live_kernel<decltype(dt)::value, decltype(per_env)::value>), ...); }); });
// so a family's instantiations are its sender-count list (GW_DTS_*, gw_internal.h) plus DT = 0, times its other parameters.
#pragma once
#include <type_traits>
#include "gw_internal.h"

// f(std::integral_constant<int, DT>) for the DT of the list that equals D, else for DT = 0 (any sender count); returns f's result
template <class F>
auto gw_with_dt(int, F&& f) { return f(std::integral_constant<int, 0>{}); }
template <int DT, int... REST, class F>
auto gw_with_dt(int D, F&& f)
{
    if (D == DT) return f(std::integral_constant<int, DT>{});
    return gw_with_dt<REST...>(D, f);
}
// f(std::integral_constant<int, MODE>) for MODE 0, 1 or 2 (gw_step_mode)
template <class F>
auto gw_with_mode(int mode, F&& f) { return gw_with_dt<1, 2>(mode, f); }
// f(std::bool_constant<B>) for a two-way template flag (PER_ENV_STATS, SPLIT, HALF, PER_ENV)
template <class F>
auto gw_with_flag(bool on, F&& f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

// MODE of the suffix-queue kernels (ct_step_sfx.hip): 0 = every exact fast form behind its run-time flag; 1 = FAST, all of
// them were validated for this handle at gw_create: the instantiation without their fallbacks; 2 = FAST, and the host rules
// out that any env reaches the fast forms' validity limits during this launch: no per-lane limit tests either.
// needs_idem: FAST also stands for idempotent noise states (GwDevConst::idem_states).  True for the per-step kernels (step,
// pendulum); the two rollout kernels walk the full transition table and stay FAST without it (GW_NO_IDEM:
// tests/test_kernel_variants.py).
inline int gw_step_mode(const GwDevConst& cst, bool below_limits, bool needs_idem)
{
    const bool fast = cst.fast_fmod && cst.fast_div && cst.fast_decide && cst.fast_ticks && (!needs_idem || cst.idem_states);
    return fast ? (below_limits ? 2 : 1) : 0;
}
