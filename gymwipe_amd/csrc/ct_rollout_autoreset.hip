// ct_rollout_autoreset.hip -- episodes for actions the caller staged.  Serves gw_rollout_autoreset and gw_rollout_autoreset_scored
// (ct_rollout_sync_ep / ct_rollout_sync_eps, gw_launch_rollout_autoreset_sfx), and the bookkeeping step of every episodic
// call's per-step form (episodes_step_kernel, gw_launch_episodes_step).  The staged hooks, the sources (StagedEpisodes,
// ScoredStagedEpisodes), the episode's book, the score and the launcher: ct_rollout_sync.hip.h.
#include "ct_rollout_sync.hip.h"

namespace {

// gw_rollout_autoreset: ct_rollout_sync_kernel's staged source with the episode's book -- the caller chooses the actions, the
// launch ends the episodes.  Nothing of the call is baked into the launch (no step0), so it may be recorded into a hipGraph.
// A rejected action (GW_FLAG_BADACT) leaves the env alone and repeats the current values, and is still a step of the episode:
// the body's put_feedback runs the hook below for it with reward 0 and the current done, as episodes_step_kernel sees such a row.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_sync_ep(GwState st, GwDevConst c, int K, GwEpisodeArgs ea,
                                                        const int32_t* __restrict__ device, const int32_t* __restrict__ duration,
                                                        int32_t* obs, float* reward, uint8_t* done, uint8_t* ended)
{
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    StagedEpisodes src;
    src.ended = ended;
    src.latest_next = 0;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); GW_ROLLOUT_STAGED_FIRST
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_STAGED_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_STAGED_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    GW_ROLLOUT_STORE_OUTPUTS(at, latest, r, dn)                                                                                  \
    {                                                                                                                            \
        GW_ROLLOUT_EP_STEPPED(r, dn)                                                                                             \
        src.ended[at] = (uint8_t)cause_next;                                                                                     \
        src.latest_next = cause_next ? 0 : latest;                                                                               \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// gw_rollout_autoreset_scored: ct_rollout_sync_ep with the score where it has the reward, and the packets per step.  The hook
// that scores (GW_ROLLOUT_SRC_STEPPED) expands in the body's put_feedback, in front of the step loop's `d`, so the source keeps
// the step's sender itself (d_cur, as the drawn sources do).  There is no table here, so the weights' LDS copy is static: D
// words beside the body's own tables, their sum checked when the kernel is compiled.  Nothing of the call but its pointers,
// limits and weights is baked into the launch: it may be recorded into a hipGraph as its parent may.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_sync_eps(GwState st, GwDevConst c, int K, GwEpisodeArgs ea, gw_score w,
                                                         const int32_t* __restrict__ device, const int32_t* __restrict__ duration,
                                                         int32_t* obs, float* reward, uint8_t* done, uint8_t* ended, int32_t* delivered)
{
    __shared__ uint32_t s_score_w[DT == 0 ? GW_MAX_DEVICES : DT];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    ScoredStagedEpisodes src;
    src.ended = ended;
    src.latest_next = 0;
    src.sc.weights_at(s_score_w, w);
    src.delivered_out = delivered;
    src.d_cur = 0;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.sc.stage(w, DT == 0 ? c.D : DT); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.sc.first(); GW_ROLLOUT_STAGED_FIRST
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_STAGED_TAKE src.d_cur = d;
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_STAGED_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    {                                                                                                                            \
        const uint32_t dl_next = src.sc.delivered(kt.deliv);                                                                     \
        const int32_t score_next = src.sc.of_staged(r, src.d_cur, dl_next, DT == 0 ? c.D : DT);                                  \
        GW_ROLLOUT_STORE_OUTPUTS(at, latest, score_next, dn)                                                                     \
        src.delivered_out[at] = (int32_t)dl_next;                                                                                \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.ended[at] = (uint8_t)cause_next;                                                                                     \
        src.latest_next = cause_next ? 0 : latest;                                                                               \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// The per-step form's bookkeeping, for handles without the fused kernels: after a step's launch, steps 1-4 and 6 of the
// semantics for every env -- {age, ret} (EpisodeBook: the fused kernels' rule, one step of it), ended, the tally, the observation
// acted on next -- and the mask gw_reset's launch takes.
//   SCORED                   a scored call: the delivered counter (GwState::sa, word 2 e + 1) differenced against the copy the
//                            draw took (deliv_before), the step scored with the sender in `device` (clamped: a staged one may
//                            lie outside the action space, and such a step moved neither counter nor reward) -- `reward` comes
//                            in as the step's reward and goes out as its score.  Otherwise the reward is the return's term, and
//                            w, D, sa, deliv_before and `device` are not read.  A template flag (two instantiations): tested
//                            at run time, the score's loads wait behind the branch for the reward's and the kernel takes one
//                            memory round trip more (profiles/per_step_fold/README.md).  (Not a family of
//                            tests/test_kernel_variants.py's catalogue: tests/test_host_logic.py lists it as out of scope and
//                            checks that these two instantiations are the library's.)
//   delivered_out            the packets per step, or nullptr (the population's form keeps none).
//   pop_tally                gw_rollout_population's [P][GW_EP_COLS], env e's episodes into row e / M as well as into the
//                            call-wide ea.tally (either may be nullptr).  Any M: a block whose 256 envs run one policy sums in
//                            LDS and adds its words to both rows; a block that spans policies sums the call-wide words in LDS
//                            and sends each ended episode's words to its policy's row directly.  nullptr: M = N.
template <bool SCORED>
__global__ __launch_bounds__(256) void episodes_step_kernel(uint32_t N, uint32_t D, int32_t center, GwEpisodeArgs ea, gw_score w,
                                                           uint32_t M, int64_t* pop_tally, const uint32_t* sa,
                                                           const uint32_t* deliv_before, const int32_t* device, const int32_t* obs,
                                                           float* reward, const uint8_t* done, uint8_t* ended, uint8_t* mask,
                                                           int32_t* delivered_out)
{
    __shared__ unsigned long long s_ep[GW_EP_COLS];
    gw_ep_zero(s_ep);
    __syncthreads();
    const uint32_t e0 = blockIdx.x * blockDim.x, e = e0 + threadIdx.x;
    const uint32_t pol0 = e0 / M;                                               // (e0 < N: the grid is ceil(N / 256) blocks)
    const bool block_row = pop_tally && pol0 == gw_min_u32(e0 + blockDim.x - 1u, N - 1u) / M;
    if (e < N) {
        EpisodeBook ep;
        ep.load(ea, e);
        int32_t r = (int32_t)reward[e];
        if constexpr (SCORED) {
            const uint32_t dl = sa[(size_t)2 * e + 1] - deliv_before[e];
            r = w.w_reward * r + w.w_delivered[gw_min_u32((uint32_t)device[e], D - 1u)] * (int32_t)dl;
            reward[e] = (float)r;
            if (delivered_out) delivered_out[e] = (int32_t)dl;
        }
        const uint32_t cause = ep.stepped(r, done[e]);
        GwEpisodeArgs own = ea;                          // (the book adds into LDS whenever there is a tally)
        if (block_row) own.tally = pop_tally;
        ep.store(own, e, s_ep);
        if (cause && pop_tally && !block_row) {
            int64_t* row = pop_tally + (size_t)(e / M) * GW_EP_COLS;
            const unsigned long long v[GW_EP_COLS] = {ep.n, ep.n_done, (unsigned long long)ep.len_sum, (unsigned long long)ep.ret_sum,
                                                      (unsigned long long)ep.ret_sq};
#pragma unroll
            for (int j = 0; j < GW_EP_COLS; ++j)
                if (v[j]) gw_ts_add(row + j, v[j]);
        }
        ended[e] = (uint8_t)cause;
        mask[e] = (uint8_t)(cause != 0u);
        ea.obs_next[e] = cause ? center : obs[e];
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)GW_EP_COLS && s_ep[threadIdx.x]) {
        if (block_row) gw_ts_add(pop_tally + (size_t)pol0 * GW_EP_COLS + threadIdx.x, s_ep[threadIdx.x]);
        if (ea.tally) gw_ts_add(ea.tally + threadIdx.x, s_ep[threadIdx.x]);
    }
}

} // namespace

// One step of the per-step forms (every queue mode), behind the step's launch (in front of it: gw_launch_policy_sample,
// ct_rollout_policy.hip): the episodes' bookkeeping on that row (row.device: the senders the step took), with the handle's reset
// mask.  score: the weights and deliv_before's copy to score the step with, or nullptr; pop_tally: the population's rows for M
// envs each, or nullptr; delivered_out: the packets per step, or nullptr.
int gw_launch_episodes_step(const GwState& st, const GwDevConst& cst, const gw_episodes& ep, const gw_score* score, int64_t M,
                            int64_t* pop_tally, const uint32_t* deliv_before, int32_t* obs_next, const GwRows& row, uint8_t* mask,
                            int32_t* delivered_out, void* stream)
{
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)st.N,
                           (uint32_t)st.D, cst.counter_bound, episode_args(ep, obs_next), score ? *score : gw_score{}, (uint32_t)M,
                           pop_tally, (const uint32_t*)st.sa, deliv_before, (const int32_t*)row.device, (const int32_t*)row.obs,
                           row.reward, (const uint8_t*)row.done, row.ended, mask, delivered_out);
    };
    if (score) launch(episodes_step_kernel<true>); else launch(episodes_step_kernel<false>);
    return gw_launch_status();
}

// gw_rollout_autoreset: the handle's rules alone (there is no table; the weights' LDS copy is static, part of the kernel's own
// figure).
int gw_launch_rollout_autoreset_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const int32_t* device,
                                    const int32_t* duration, const gw_episodes& ep, const gw_score* score, int32_t* obs_next,
                                    const GwRows& out, int32_t* delivered)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_NO_TABLE)) return GW_EUNSUPPORTED;
    if (score)
        return launch_fused(st, cst, ch, GW_LS_ROLLOUT_SYNC_EPS, GW_FUSED_NO_TABLE, GW_KERNEL_OF(ct_rollout_sync_eps),
                            episode_args(ep, obs_next), *score, device, duration, out.obs, out.reward, out.done, out.ended, delivered);
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_SYNC_EP, GW_FUSED_NO_TABLE, GW_KERNEL_OF(ct_rollout_sync_ep), episode_args(ep, obs_next),
                        device, duration, out.obs, out.reward, out.done, out.ended);
}
