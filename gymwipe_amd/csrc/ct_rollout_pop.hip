// ct_rollout_pop.hip -- a population of policy tables in one launch, one per block, nothing stored per step.  Serves
// gw_rollout_population and gw_rollout_population_scored (ct_rollout_pop_ep / ct_rollout_pop_eps, gw_launch_rollout_pop_ep_sfx).
// The draw, the episode's book, the score and the launcher: ct_rollout_sync.hip.h.
#include "ct_rollout_sync.hip.h"

namespace {

// ---- a population of policies in one launch: gw_rollout_population (include/gymwipe_amd.h) ---------------------------------
// Env e runs policy e / M.  A block is one wave of 64 consecutive envs and M is a multiple of 64 (the launcher refuses any
// other), so a block has ONE policy, p = blockIdx.x * 64 / M: it stages that policy's [3][A] slice and flushes its episode
// tally into that policy's row.  ct_rollout_policy_ep's source with nothing stored per step (PopulationActions,
// ct_rollout_sync.hip.h).
// p.cdf is [P][3][A] here, pop_tally [P][GW_EP_COLS]; ea.tally the call-wide row (or nullptr), which gets every block's words too:
// at most 2 * GW_EP_COLS global adds per block.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pop_ep(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, uint32_t M,
                                                       int64_t* pop_tally)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    PopulationActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    {
        const uint32_t pol = (blockIdx.x * 64u) / M;
        src.cdf = p.cdf + (size_t)pol * 3u * src.A;
        src.row = pop_tally + (size_t)pol * GW_EP_COLS;
    }
    src.table_at(s_policy_cdf);
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage_cdf(); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        GW_ROLLOUT_EP_STEPPED(r, dn)                                                                                             \
        src.next(k, K, cause_next ? 0 : latest);                                                                                 \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(true, src.row)
}

// ct_rollout_pop_ep with the book's return the score.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pop_eps(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, gw_score w,
                                                        uint32_t M, int64_t* pop_tally)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    ScoredPopulationActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    {
        const uint32_t pol = (blockIdx.x * 64u) / M;
        src.cdf = p.cdf + (size_t)pol * 3u * src.A;
        src.row = pop_tally + (size_t)pol * GW_EP_COLS;
    }
    src.table_at(s_policy_cdf);
    src.sc.weights_at(s_policy_cdf + 3u * src.A, w);
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage_cdf(); src.sc.stage(w, DT == 0 ? c.D : DT); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.sc.first(); src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        const int32_t score_next = src.sc.of(r, src.d_cur, src.sc.delivered(kt.deliv));                                          \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.next(k, K, cause_next ? 0 : latest);                                                                                 \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(true, src.row)
}

} // namespace

// gw_rollout_population (pol.cdf: the population's tables): gw_rollout_episodes' rules, and envs_per_policy a multiple of 64, so
// that no wave spans two policies.  (The caller has checked num_policies * envs_per_policy == N: every block's policy index is
// below num_policies.)
int gw_launch_rollout_pop_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_population& pop,
                                 const GwPolicyStream& pol, const gw_episodes& ep, const gw_score* score, const int32_t* obs_prev,
                                 int32_t* obs_next)
{
    if (fused_unavailable(st, cst, ch.K, score ? GW_FUSED_TABLE_SCORE : GW_FUSED_TABLE) || pop.envs_per_policy % 64 != 0)
        return GW_EUNSUPPORTED;
    if (score)
        return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POP_EPS, GW_FUSED_TABLE_SCORE, GW_KERNEL_OF(ct_rollout_pop_eps),
                            policy_args(pol, obs_prev), episode_args(ep, obs_next), *score, (uint32_t)pop.envs_per_policy, pop.tally_dev);
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POP_EP, GW_FUSED_TABLE, GW_KERNEL_OF(ct_rollout_pop_ep), policy_args(pol, obs_prev),
                        episode_args(ep, obs_next), (uint32_t)pop.envs_per_policy, pop.tally_dev);
}
