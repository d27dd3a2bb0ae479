// ct_rollout_policy.hip -- the closed loop that stores its rows: actions drawn from a policy table inside the launch, every
// step's action and outputs written out.  Serves gw_rollout_policy (ct_rollout_policy, gw_launch_rollout_policy_sfx),
// gw_rollout_episodes and gw_rollout_episodes_scored (ct_rollout_policy_ep / ct_rollout_policy_eps,
// gw_launch_rollout_policy_ep_sfx), and the per-step draw of every closed loop on handles without a fused kernel
// (policy_sample_kernel, gw_launch_policy_sample).  The draw, the episode's book and the launcher: ct_rollout_sync.hip.h.
#include "ct_rollout_sync.hip.h"

namespace {

// gw_rollout_policy's source: the draw, and the action taken stored with the step's outputs.
struct PolicyActions : PolicyDraw {
    int32_t center;                                      // (c.counter_bound, read at the kernel's entry as it always was: read
                                                         //  where first() runs, the kernel's argument loads change)
    int32_t* __restrict__ device_out;
    int32_t* __restrict__ duration_out;
    __device__ __forceinline__ void stepped(size_t at, int k, int K, int32_t latest)
    {
        device_out[at] = d_cur;
        duration_out[at] = du_cur;
        next(k, K, latest);
    }
};

// The closed loop in one launch: the same K steps, each env's action drawn from the table's row for the observation its own
// previous step produced (obs_prev for step 0; apart from every output -- the C-ABI's rule: the outputs are __restrict__ too,
// rollout_policy() copies a row of its own `out`).  No `_kernel` suffix: the catalogue of tests/test_kernel_variants.py is about
// the families it lists; this one's cases are tests/test_rollout_policy.py's.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_policy(GwState st, GwDevConst c, int K, GwPolicyArgs p,
                                                       int32_t* __restrict__ device_out, int32_t* __restrict__ duration_out,
                                                       int32_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done)
{
    extern __shared__ uint32_t s_policy_cdf[];
    PolicyActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.table_at(s_policy_cdf);
    src.center = c.counter_bound;
    src.device_out = device_out; src.duration_out = duration_out;
#define GW_ROLLOUT_SRC_STAGE src.stage_cdf();
#define GW_ROLLOUT_SRC_FIRST src.first(e, p.obs_prev[e], src.center);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn) GW_ROLLOUT_STORE_OUTPUTS(at, latest, r, dn) src.stepped(at, k, K, latest);
#include "ct_rollout_sync_body.h"
}

template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_policy_ep(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea,
                                                          int32_t* device_out, int32_t* duration_out, int32_t* obs, float* reward,
                                                          uint8_t* done, uint8_t* ended)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    EpisodeActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.table_at(s_policy_cdf);
    src.device_out = device_out; src.duration_out = duration_out; src.ended = ended;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage_cdf(); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    GW_ROLLOUT_STORE_OUTPUTS(at, latest, r, dn)                                                                                  \
    {                                                                                                                            \
        GW_ROLLOUT_EP_STEPPED(r, dn)                                                                                             \
        src.stepped(at, k, K, latest, cause_next);                                                                               \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// ct_rollout_policy_ep with the score where it has the reward: the reward row, the book's return -- and the packets per step.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_policy_eps(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, gw_score w,
                                                           int32_t* device_out, int32_t* duration_out, int32_t* obs, float* reward,
                                                           uint8_t* done, uint8_t* ended, int32_t* delivered)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    ScoredEpisodeActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.table_at(s_policy_cdf);
    src.sc.weights_at(s_policy_cdf + 3u * src.A, w);
    src.device_out = device_out; src.duration_out = duration_out; src.ended = ended; src.delivered_out = delivered;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage_cdf(); src.sc.stage(w, DT == 0 ? c.D : DT); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.sc.first(); src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    {                                                                                                                            \
        const uint32_t dl_next = src.sc.delivered(kt.deliv);                                                                     \
        const int32_t score_next = src.sc.of(r, src.d_cur, dl_next);                                                             \
        GW_ROLLOUT_STORE_OUTPUTS(at, latest, score_next, dn)                                                                     \
        src.delivered_out[at] = (int32_t)dl_next;                                                                                \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.stepped(at, k, K, latest, cause_next);                                                                               \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// The per-step form's draw, for handles without a fused rollout: one step's actions for every env from the observations
// p.obs_prev, env e from table e / M of p.cdf's [P][3][A] (one table: M = N).  deliv_before != nullptr (the scored calls): each
// env's delivered counter (GwState::sa, word 2 e + 1: what gw_delivered reads) into that row as well, in front of the step.
__global__ __launch_bounds__(256) void policy_sample_kernel(uint32_t N, uint32_t A, uint32_t md, int32_t center, GwPolicyArgs p,
                                                            uint32_t M, const uint32_t* __restrict__ sa,
                                                            int32_t* __restrict__ device_out, int32_t* __restrict__ duration_out,
                                                            uint32_t* __restrict__ deliv_before)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const uint32_t cls = gw_policy_cls(p.obs_prev[e], center);
    const uint32_t* row = p.cdf + ((size_t)(e / M) * 3u + cls) * A;
    const uint32_t a = gw_policy_count(row, A, gw_policy_u(p.seed, gw_policy_env_term(p.env0, e), p.step0));
    const uint32_t dv = a / md;
    device_out[e] = (int32_t)dv;
    duration_out[e] = (int32_t)(a - dv * md);
    if (deliv_before) deliv_before[e] = sa[(size_t)2 * e + 1];
}

} // namespace

// One step of the per-step forms (every queue mode), around the step's launch.  In front of it, the closed loops' draw for step
// pol.step0 from `obs_in` into row's action rows, env e from table e / M (one table: M = st.N); deliv_before: where a scored
// call's copy of the delivered counters goes, or nullptr (behind the step: gw_launch_episodes_step, ct_rollout_autoreset.hip).
int gw_launch_policy_sample(const GwState& st, const GwDevConst& cst, const GwPolicyStream& pol, int64_t M, const int32_t* obs_in,
                            const GwRows& row, uint32_t* deliv_before, void* stream)
{
    hipLaunchKernelGGL(policy_sample_kernel, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)st.N,
                       (uint32_t)st.D * (uint32_t)cst.max_duration, (uint32_t)cst.max_duration, cst.counter_bound,
                       policy_args(pol, obs_in), (uint32_t)M, (const uint32_t*)st.sa, row.device, row.duration, deliv_before);
    return gw_launch_status();
}

// The fused forms.  Each returns GW_EUNSUPPORTED where there is none (fused_unavailable): the caller draws and steps per step,
// or -- the two tallying forms -- refuses the call before its first launch.
int gw_launch_rollout_policy_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                 const int32_t* obs_prev, const GwRows& out)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POLICY, GW_FUSED_TABLE, GW_KERNEL_OF(ct_rollout_policy), policy_args(pol, obs_prev),
                        out.device, out.duration, out.obs, out.reward, out.done);
}

// gw_rollout_episodes / gw_rollout_episodes_stats: their parents' rules, with the caller's gw_episodes and obs_next passed on.
// score (here and below): nullptr, or the _scored call's weights -- the same rules with the D weights counted into the launch's
// LDS, the family with the score, and `delivered` where the call keeps the packets per step.
int gw_launch_rollout_policy_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                    const gw_episodes& ep, const gw_score* score, const int32_t* obs_prev, int32_t* obs_next,
                                    const GwRows& out, int32_t* delivered)
{
    if (fused_unavailable(st, cst, ch.K, score ? GW_FUSED_TABLE_SCORE : GW_FUSED_TABLE)) return GW_EUNSUPPORTED;
    if (score)
        return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POLICY_EPS, GW_FUSED_TABLE_SCORE, GW_KERNEL_OF(ct_rollout_policy_eps),
                            policy_args(pol, obs_prev), episode_args(ep, obs_next), *score, out.device, out.duration, out.obs, out.reward,
                            out.done, out.ended, delivered);
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POLICY_EP, GW_FUSED_TABLE, GW_KERNEL_OF(ct_rollout_policy_ep),
                        policy_args(pol, obs_prev), episode_args(ep, obs_next), out.device, out.duration, out.obs, out.reward, out.done,
                        out.ended);
}
