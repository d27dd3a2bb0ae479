// ct_rollout_fsc.hip -- finite-state controllers inside the launch: the scored closed loops with a small memory.  Serves
// gw_rollout_controller (ct_rollout_fsc, gw_launch_rollout_fsc_sfx) and gw_rollout_controller_population (ct_rollout_fsc_pop,
// gw_launch_rollout_fsc_pop_sfx).  There is no per-step form: a handle without these kernels is refused.
// The draw, the episode's book, the score and the launcher: ct_rollout_sync.hip.h.
#include "ct_rollout_sync.hip.h"

namespace {

// What both calls pass on besides their parents' arguments: the controller's two byte tables, each env's node, and S - 1.
// (The controller's cdf travels in GwPolicyArgs::cdf: [S][3][A], or [P][S][3][A].)
struct GwFscArgs {
    const uint8_t* next;          // [S][3][2] (the population: [P][S][3][2])
    const uint8_t* need;          // [S]       (the population: [P][S])
    uint8_t* node;                // [N], read before step 0 and written behind the last step
    uint32_t last;                // S - 1: what every node read from memory is clamped to
};

// The controller beside a PolicyDraw (the source derives from its parent's, which has one): the node in a register, the two
// byte tables behind the score's weights in the launch's dynamic LDS.  The draw reads row node * 3 + cls of the table -- to
// PolicyDraw::draw that is just another row index --, and behind every step the node moves on the class of what the env now
// sees and on whether the step delivered at least need[node] packets.  Every index is clamped where its byte is read: node to
// S - 1, the class is 0 .. 2 by construction, the bit 0 or 1 -- any content of the three arrays is memory-safe and has one
// meaning (actions.controller_step_numpy restates it).
struct ControllerNode {
    uint8_t* s_bytes;                                    // the launch's dynamic LDS, as bytes
    uint32_t next_at, need_at;                           // where [S][3][2] and [S] begin in it (next_at: a multiple of 4)
    uint32_t S3A;                                        // words of the controller's table: S * 3 * A
    uint32_t last;                                       // S - 1
    uint32_t node;
    // lds: the launch's dynamic part -- S * 3 * A words of cdf, the score's D weights, then the two byte tables
    __device__ __forceinline__ void tables_at(uint32_t* lds, uint32_t S, uint32_t A, int D)
    {
        last = S - 1u;
        S3A = S * 3u * A;
        s_bytes = reinterpret_cast<uint8_t*>(lds);
        next_at = (S3A + (uint32_t)D) * 4u;
        need_at = next_at + 6u * S;
    }
    __device__ __forceinline__ void stage(uint32_t* s_cdf, const uint32_t* cdf, const uint8_t* next, const uint8_t* need) const
    {
        const uint32_t S = last + 1u;
        for (uint32_t i = threadIdx.x; i < S3A; i += blockDim.x) s_cdf[i] = cdf[i];
        for (uint32_t i = threadIdx.x; i < 6u * S; i += blockDim.x) s_bytes[next_at + i] = next[i];
        for (uint32_t i = threadIdx.x; i < S; i += blockDim.x) s_bytes[need_at + i] = need[i];
    }
    __device__ __forceinline__ void first(uint8_t stored) { node = gw_min_u32((uint32_t)stored, last); }
    // Step k is over: it delivered dl packets, the env now sees `latest` (minus counter_bound), and `cause` says whether its
    // episode ended.  Returns the class the next draw is for.  The pair next[node][cls][0 .. 1] is one 16-bit LDS read that
    // does not wait for need[node]'s.
    __device__ __forceinline__ uint32_t move(uint32_t dl, int32_t latest, uint32_t cause)
    {
        const uint32_t cls = (uint32_t)((int)(latest > 0) - (int)(latest < 0) + 1);
        const uint32_t pair = *reinterpret_cast<const uint16_t*>(s_bytes + (next_at + node * 6u + cls * 2u));
        const uint32_t to = dl >= (uint32_t)s_bytes[need_at + node] ? pair >> 8 : pair & 0xffu;
        node = cause ? 0u : gw_min_u32(to, last);
        return cause ? 1u : cls;
    }
};

// ct_rollout_policy_eps' source with the node.  first_at / stepped_at shadow PolicyDraw's first / EpisodeActions' stepped:
// the same statements with the row index in the class's place.
struct ControllerActions : ScoredEpisodeActions {
    ControllerNode fsc;
    uint8_t* node_out;
    __device__ __forceinline__ void first_at(uint32_t e, int32_t obs_seen, int32_t center, uint8_t stored)
    {
        env_term = gw_policy_env_term(env0, e);
        latest_next = obs_seen - center;
        fsc.first(stored);
        draw(fsc.node * 3u + gw_policy_cls(obs_seen, center), step0);
    }
    __device__ __forceinline__ void stepped_at(size_t at, int k, int K, int32_t latest, uint32_t cause, uint32_t dl)
    {
        device_out[at] = d_cur;
        duration_out[at] = du_cur;
        ended[at] = (uint8_t)cause;
        node_out[at] = (uint8_t)fsc.node;
        const uint32_t cls = fsc.move(dl, latest, cause);
        latest_next = cause ? 0 : latest;
        if (k + 1 < K) draw(fsc.node * 3u + cls, step0 + (uint64_t)(k + 1));
    }
};

// gw_rollout_controller: ct_rollout_policy_eps with the controller.  Dynamic LDS: S * 3 * A words of cdf, the score's D
// weights, then next (6 S bytes) and need (S bytes).
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_fsc(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, gw_score w,
                                                    GwFscArgs fa, int32_t* device_out, int32_t* duration_out, int32_t* obs,
                                                    float* reward, uint8_t* done, uint8_t* ended, int32_t* delivered, uint8_t* node_out)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    ControllerActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.table_at(s_policy_cdf);
    src.fsc.tables_at(s_policy_cdf, fa.last + 1u, src.A, DT == 0 ? c.D : DT);
    src.sc.weights_at(s_policy_cdf + src.fsc.S3A, w);
    src.device_out = device_out; src.duration_out = duration_out; src.ended = ended; src.delivered_out = delivered;
    src.node_out = node_out;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE                                                                                                     \
    src.fsc.stage(s_policy_cdf, p.cdf, fa.next, fa.need);                                                                        \
    src.sc.stage(w, DT == 0 ? c.D : DT);                                                                                         \
    gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.sc.first(); src.first_at(e, p.obs_prev[e], c.counter_bound, fa.node[e]);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    {                                                                                                                            \
        const uint32_t dl_next = src.sc.delivered(kt.deliv);                                                                     \
        const int32_t score_next = src.sc.of(r, src.d_cur, dl_next);                                                             \
        GW_ROLLOUT_STORE_OUTPUTS(at, latest, score_next, dn)                                                                     \
        src.delivered_out[at] = (int32_t)dl_next;                                                                                \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.stepped_at(at, k, K, latest, cause_next, dl_next);                                                                   \
    }
#include "ct_rollout_sync_body.h"
    // (in front of the tail: behind its wave-ordered flush the pointer and the node stay live across the flush's loops, and the
    // records form then gets a private segment)
    fa.node[e] = (uint8_t)src.fsc.node;
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// ct_rollout_pop_eps' source with the node.
struct ControllerPopulationActions : ScoredPopulationActions {
    ControllerNode fsc;
    __device__ __forceinline__ void first_at(uint32_t e, int32_t obs_seen, int32_t center, uint8_t stored)
    {
        env_term = gw_policy_env_term(env0, e);          // the stream is the env's, whichever controller it runs
        latest_next = obs_seen - center;
        fsc.first(stored);
        draw(fsc.node * 3u + gw_policy_cls(obs_seen, center), step0);
    }
    __device__ __forceinline__ void stepped_at(int k, int K, int32_t latest, uint32_t cause, uint32_t dl)
    {
        const uint32_t cls = fsc.move(dl, latest, cause);
        latest_next = cause ? 0 : latest;
        if (k + 1 < K) draw(fsc.node * 3u + cls, step0 + (uint64_t)(k + 1));
    }
};

// gw_rollout_controller_population: env e runs controller e / M, nothing is stored per step, and the block's episodes go into
// its controller's row of pop_tally.  M is a multiple of 64 (the launcher refuses any other), so a block has ONE controller,
// blockIdx.x * 64 / M: it stages that controller's three slices.  p.cdf is [P][S][3][A], fa.next [P][S][3][2], fa.need [P][S].
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_fsc_pop(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, gw_score w,
                                                        GwFscArgs fa, uint32_t M, int64_t* pop_tally)
{
    extern __shared__ uint32_t s_policy_cdf[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    ControllerPopulationActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.table_at(s_policy_cdf);
    src.fsc.tables_at(s_policy_cdf, fa.last + 1u, src.A, DT == 0 ? c.D : DT);
    const uint32_t pol_next = (blockIdx.x * 64u) / M;
    src.cdf = p.cdf + (size_t)pol_next * src.fsc.S3A;
    src.row = pop_tally + (size_t)pol_next * GW_EP_COLS;
    src.sc.weights_at(s_policy_cdf + src.fsc.S3A, w);
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE                                                                                                     \
    src.fsc.stage(s_policy_cdf, src.cdf, fa.next + (size_t)pol_next * 6u * (fa.last + 1u), fa.need + (size_t)pol_next * (fa.last + 1u)); \
    src.sc.stage(w, DT == 0 ? c.D : DT);                                                                                         \
    gw_ep_zero(s_ep_tally);
    // (Opaque copies of the scalars every step reads, as in ct_rollout_backlog_pop: with nothing stored per step the compiler
    // otherwise reloads them from the kernel-argument segment inside the step loop.)
#define GW_FSC_POP_PIN(x) asm volatile("" : "+s"(x))
    GW_FSC_POP_PIN(K);
#define GW_ROLLOUT_SRC_FIRST                                                                                                     \
    src.ep.load(ea, e); src.sc.first(); src.first_at(e, p.obs_prev[e], c.counter_bound, fa.node[e]);                             \
    GW_FSC_POP_PIN(src.ep.max_steps); GW_FSC_POP_PIN(src.ep.on_done); GW_FSC_POP_PIN(src.sc.w_reward); GW_FSC_POP_PIN(src.fsc.last);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        const uint32_t dl_next = src.sc.delivered(kt.deliv);                                                                     \
        const int32_t score_next = src.sc.of(r, src.d_cur, dl_next);                                                             \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.stepped_at(k, K, latest, cause_next, dl_next);                                                                       \
    }
#include "ct_rollout_sync_body.h"
#undef GW_FSC_POP_PIN
    fa.node[e] = (uint8_t)src.fsc.node;
    GW_ROLLOUT_EP_TAIL(true, src.row)
}

// the launch's dynamic LDS: the controller's table, the score's weights, the two byte tables padded to a word
inline size_t fsc_lds_bytes(const GwState& st, const GwDevConst& cst, int S)
{
    const size_t A = (size_t)st.D * (size_t)cst.max_duration;
    return ((size_t)S * 3 * A + (size_t)st.D) * sizeof(uint32_t) + ((size_t)S * 7 + 3) / 4 * 4;
}

} // namespace

// gw_rollout_controller: gw_rollout_episodes_scored's rules, and the controller has to fit the block's LDS beside the kernel's
// own (launch_fused_lds asks the instantiation).  pol.cdf: the controller's [S][3][A].
int gw_launch_rollout_fsc_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_controller& ctl,
                              const GwPolicyStream& pol, const gw_episodes& ep, const gw_score& score, const int32_t* obs_prev,
                              int32_t* obs_next, const GwRows& out, int32_t* delivered, uint8_t* node_out)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_SCORE)) return GW_EUNSUPPORTED;
    const GwFscArgs fa = {ctl.next_dev, ctl.need_dev, ctl.node_dev, (uint32_t)ctl.num_states - 1u};
    return launch_fused_lds(st, cst, ch, GW_LS_ROLLOUT_FSC, true, fsc_lds_bytes(st, cst, ctl.num_states), GW_KERNEL_OF(ct_rollout_fsc),
                            policy_args(pol, obs_prev), episode_args(ep, obs_next), score, fa, out.device, out.duration, out.obs,
                            out.reward, out.done, out.ended, delivered, node_out);
}

// gw_rollout_controller_population: the same, and envs_per_policy a multiple of 64, so that no wave spans two controllers.  (The
// caller has checked num_policies * envs_per_policy == N: every block's controller index is below num_policies.)
int gw_launch_rollout_fsc_pop_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_controller_population& pop,
                                  const GwPolicyStream& pol, const gw_episodes& ep, const gw_score& score, const int32_t* obs_prev,
                                  int32_t* obs_next)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_SCORE) || pop.envs_per_policy % 64 != 0) return GW_EUNSUPPORTED;
    const GwFscArgs fa = {pop.next_dev, pop.need_dev, pop.node_dev, (uint32_t)pop.num_states - 1u};
    return launch_fused_lds(st, cst, ch, GW_LS_ROLLOUT_FSC_POP, true, fsc_lds_bytes(st, cst, pop.num_states),
                            GW_KERNEL_OF(ct_rollout_fsc_pop), policy_args(pol, obs_prev), episode_args(ep, obs_next), score, fa,
                            (uint32_t)pop.envs_per_policy, pop.tally_dev);
}
