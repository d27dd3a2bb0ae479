// ct_rollout_backlog.hip -- the queue-aware scheduler inside the launch.  Serves gw_rollout_backlog (ct_rollout_backlog,
// gw_launch_rollout_backlog_sfx; per step: backlog_select_rows, gw_launch_backlog_select) and gw_rollout_backlog_population
// (ct_rollout_backlog_pop, gw_launch_rollout_backlog_pop_sfx; per step: backlog_select_pop_rows, gw_launch_backlog_select_pop).
// Its parent's source (ScoredStagedEpisodes), the episode's book, the score and the launcher: ct_rollout_sync.hip.h.
#include "ct_rollout_sync.hip.h"

namespace {

// gw_rollout_backlog: ct_rollout_sync_eps with the action not loaded from rows but chosen at the step boundary from the body's
// own queue lengths (queues_now(), ct_rollout_sync_body.h): the lowest sender attaining the largest w_len[i] * len[i], for
// duration_of_len[its length] clamped into the action space.  The policy's 128 + 101 bytes lie in static LDS beside the score's
// weights: one LDS read per sender and one per step, all at wave-uniform or per-lane byte addresses.  DT != 0: the scan is
// unrolled over the length registers; DT == 0: it walks the lane's LDS column.  What was chosen and the length it was chosen
// for are stored with the step's outputs.  No draws and no step0: it may be recorded into a hipGraph as its parent may.
struct BacklogEpisodes : ScoredStagedEpisodes {
    const uint32_t* s_w;                                 // [D] in LDS
    const uint8_t* s_dur;                                // [GW_QUEUE_CAP + 1] in LDS
    int32_t* device_out;
    int32_t* duration_out;
    int32_t* seen_len;
    int du_cur;
    uint32_t q_cur;                                      // the chosen sender's length when it was chosen
    __device__ __forceinline__ void stage(const gw_backlog_policy& pol, int D, uint32_t* lds_w, uint8_t* lds_dur) const
    {
        for (int i = threadIdx.x; i < D; i += blockDim.x) lds_w[i] = (uint32_t)pol.w_len[i];
        for (int i = threadIdx.x; i <= GW_QUEUE_CAP; i += blockDim.x) lds_dur[i] = pol.duration_of_len[i];
    }
    // the step's action from the lengths `len` (all at the env's current time); a strict > keeps the lowest index of a tie,
    // and sender 0 where every priority is 0
    template <int DT, class ARR>
    __device__ __forceinline__ int pick(ARR& len, int D, int max_duration)
    {
        const int n = DT ? DT : D;
        uint32_t q = len[0], p = s_w[0] * q;
        int d = 0;
#pragma unroll
        for (int i = 1; i < n; ++i) {
            const uint32_t qi = len[i], pi = s_w[i] * qi;
            const bool more = pi > p;
            p = more ? pi : p; q = more ? qi : q; d = more ? i : d;
        }
        d_cur = d;
        q_cur = q;
        du_cur = (int)gw_min_u32((uint32_t)s_dur[gw_min_u32(q, (uint32_t)GW_QUEUE_CAP)], (uint32_t)max_duration - 1u);
        return d;
    }
};

template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_backlog(GwState st, GwDevConst c, int K, GwEpisodeArgs ea, gw_score w, gw_backlog_policy pol,
                                                        int32_t* device_out, int32_t* duration_out, int32_t* seen_len, int32_t* obs,
                                                        float* reward, uint8_t* done, uint8_t* ended, int32_t* delivered)
{
    __shared__ uint32_t s_score_w[DT == 0 ? GW_MAX_DEVICES : DT];
    __shared__ uint32_t s_backlog_w[DT == 0 ? GW_MAX_DEVICES : DT];
    __shared__ uint8_t s_backlog_dur[(GW_QUEUE_CAP + 1 + 3) / 4 * 4];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    BacklogEpisodes src;
    src.ended = ended;
    src.latest_next = 0;
    src.sc.weights_at(s_score_w, w);
    src.delivered_out = delivered;
    src.d_cur = 0; src.du_cur = 0; src.q_cur = 0;
    src.s_w = s_backlog_w; src.s_dur = s_backlog_dur;
    src.device_out = device_out; src.duration_out = duration_out; src.seen_len = seen_len;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_QUEUES
#define GW_ROLLOUT_SRC_STAGE                                                                                                     \
    src.sc.stage(w, DT == 0 ? c.D : DT);                                                                                         \
    src.stage(pol, DT == 0 ? c.D : DT, s_backlog_w, s_backlog_dur);                                                              \
    gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.sc.first();
#define GW_ROLLOUT_SRC_TAKE                                                                                                      \
    queues_now();                                                                                                                \
    const int d = src.pick<DT>(len, D, c.max_duration), du = src.du_cur;
#define GW_ROLLOUT_SRC_CHECKED(bad) false
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    {                                                                                                                            \
        const uint32_t dl_next = src.sc.delivered(kt.deliv);                                                                     \
        const int32_t score_next = src.sc.of(r, src.d_cur, dl_next);                                                             \
        GW_ROLLOUT_STORE_OUTPUTS(at, latest, score_next, dn)                                                                     \
        src.delivered_out[at] = (int32_t)dl_next;                                                                                \
        src.device_out[at] = src.d_cur;                                                                                          \
        src.duration_out[at] = src.du_cur;                                                                                       \
        src.seen_len[at] = (int32_t)src.q_cur;                                                                                   \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.ended[at] = (uint8_t)cause_next;                                                                                     \
        src.latest_next = cause_next ? 0 : latest;                                                                               \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
}

// gw_rollout_backlog_population: ct_rollout_backlog crossed with ct_rollout_pop_eps -- env e runs policy e / M of an array in
// DEVICE memory, nothing is stored per step, and the block's episodes go into its policy's row of pop_tally.  M is a multiple
// of 64 (the launcher refuses any other), so a block has ONE policy, p = blockIdx.x * 64 / M.  Its record is 232 bytes, 58
// dwords: lane i loads dword i -- one coalesced load per wave, through the global address space -- and the first D lanes put
// the weights, clamped into [0, GW_SCORE_W_MAX], the lanes from GW_MAX_DEVICES on the table's dwords into the static LDS
// ct_rollout_backlog keeps them in.  The array is never read on the host: after the clamp, with pick's clamped index, any
// content is memory-safe and has one meaning (actions.backlog_sample_population_numpy).  No draws, no step0 and no policy in
// the launch's arguments: a recorded launch reads whatever the array holds when it is replayed.
__device__ __forceinline__ uint32_t gw_backlog_weight(int32_t w)
{
    return (uint32_t)(w < 0 ? 0 : w > GW_SCORE_W_MAX ? GW_SCORE_W_MAX : w);
}
struct BacklogPopulationEpisodes : BacklogEpisodes {
    int64_t* row;                                        // the block's policy: [GW_EP_COLS] of the caller's [P][GW_EP_COLS]
    __device__ __forceinline__ void stage_from(const gw_backlog_policy* pol, int D, uint32_t* lds_w, uint8_t* lds_dur) const
    {
        constexpr uint32_t W = GW_MAX_DEVICES, WORDS = sizeof(gw_backlog_policy) / 4u;
        static_assert(sizeof(gw_backlog_policy) % 4u == 0 && WORDS <= 64u && offsetof(gw_backlog_policy, duration_of_len) == 4u * W,
                      "one dword of the record per lane");
        const uint32_t i = threadIdx.x;
        if (i < WORDS) {
            const uint32_t v = ld_global<uint32_t>(pol, i << 2);
            if (i < (uint32_t)D) lds_w[i] = gw_backlog_weight((int32_t)v);
            if (i >= W) reinterpret_cast<uint32_t*>(lds_dur)[i - W] = v;
        }
    }
};

template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_backlog_pop(GwState st, GwDevConst c, int K, GwEpisodeArgs ea, gw_score w,
                                                            const gw_backlog_policy* __restrict__ policies, uint32_t M, int64_t* pop_tally)
{
    __shared__ uint32_t s_score_w[DT == 0 ? GW_MAX_DEVICES : DT];
    __shared__ uint32_t s_backlog_w[DT == 0 ? GW_MAX_DEVICES : DT];
    __shared__ __attribute__((aligned(4))) uint8_t s_backlog_dur[(GW_QUEUE_CAP + 1 + 3) / 4 * 4];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    static_assert(sizeof(gw_backlog_policy) == 4u * GW_MAX_DEVICES + sizeof s_backlog_dur, "the table's dwords fill its LDS copy");
    BacklogPopulationEpisodes src;
    src.ended = nullptr;
    src.latest_next = 0;
    src.sc.weights_at(s_score_w, w);
    src.delivered_out = nullptr;
    src.d_cur = 0; src.du_cur = 0; src.q_cur = 0;
    src.s_w = s_backlog_w; src.s_dur = s_backlog_dur;
    src.device_out = nullptr; src.duration_out = nullptr; src.seen_len = nullptr;
    const uint32_t pol_next = (blockIdx.x * 64u) / M;
    src.row = pop_tally + (size_t)pol_next * GW_EP_COLS;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_QUEUES
#define GW_ROLLOUT_SRC_STAGE                                                                                                     \
    src.sc.stage(w, DT == 0 ? c.D : DT);                                                                                         \
    src.stage_from(policies + pol_next, DT == 0 ? c.D : DT, s_backlog_w, s_backlog_dur);                                         \
    gw_ep_zero(s_ep_tally);
    // (Opaque copies of the scalars every step reads.  With nothing stored per step the compiler otherwise reloads them from
    // the kernel-argument segment inside the step loop -- the step count, the episode's limits and the reward's weight, a scalar
    // load and a wait each per step -- where the rows-writing parent keeps them in registers.)
#define GW_BACKLOG_POP_PIN(x) asm volatile("" : "+s"(x))
    GW_BACKLOG_POP_PIN(K);
#define GW_ROLLOUT_SRC_FIRST                                                                                                     \
    src.ep.load(ea, e); src.sc.first();                                                                                          \
    GW_BACKLOG_POP_PIN(src.ep.max_steps); GW_BACKLOG_POP_PIN(src.ep.on_done); GW_BACKLOG_POP_PIN(src.sc.w_reward);
#define GW_ROLLOUT_SRC_TAKE                                                                                                      \
    queues_now();                                                                                                                \
    const int d = src.pick<DT>(len, D, c.max_duration), du = src.du_cur;
#define GW_ROLLOUT_SRC_CHECKED(bad) false
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        const int32_t score_next = src.sc.of(r, src.d_cur, src.sc.delivered(kt.deliv));                                          \
        GW_ROLLOUT_EP_STEPPED(score_next, dn)                                                                                    \
        src.latest_next = cause_next ? 0 : latest;                                                                               \
    }
#include "ct_rollout_sync_body.h"
#undef GW_BACKLOG_POP_PIN
    GW_ROLLOUT_EP_TAIL(true, src.row)
}

// The per-step forms' choice, for handles without the fused kernels: one step's (d, du, q_d) for an env from the queue-length
// bytes in its qb record -- where gw_get_state "qlen" reads them; every step and reset kernel leaves them at the env's current
// time -- by BacklogEpisodes::pick's rule.  CLAMP: the weights are clamped where they are read (a policy in device memory).
template <bool CLAMP>
__device__ __forceinline__ void gw_backlog_select(const uint8_t* row, uint32_t D, uint32_t md, const gw_backlog_policy& pol, uint32_t& d_out,
                                                  uint32_t& du_out, uint32_t& q_out)
{
    auto weight = [&](uint32_t i) { return CLAMP ? gw_backlog_weight(pol.w_len[i]) : (uint32_t)pol.w_len[i]; };
    uint32_t q = row[0], p = weight(0) * q, d = 0;
    for (uint32_t i = 1; i < D; ++i) {
        const uint32_t qi = row[i], pi = weight(i) * qi;
        const bool more = pi > p;
        p = more ? pi : p; q = more ? qi : q; d = more ? i : d;
    }
    d_out = d;
    du_out = gw_min_u32((uint32_t)pol.duration_of_len[gw_min_u32(q, (uint32_t)GW_QUEUE_CAP)], md - 1u);
    q_out = q;
}
__global__ __launch_bounds__(256) void backlog_select_rows(uint32_t N, uint32_t D, uint32_t RB, uint32_t md, gw_backlog_policy pol,
                                                           const uint8_t* __restrict__ qb, int32_t* __restrict__ device_out,
                                                           int32_t* __restrict__ duration_out, int32_t* __restrict__ seen_len)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    uint32_t d, du, q;
    gw_backlog_select<false>(qb + (size_t)e * RB, D, md, pol, d, du, q);
    device_out[e] = (int32_t)d;
    duration_out[e] = (int32_t)du;
    seen_len[e] = (int32_t)q;
}
// ... and the population's: env e under policy e / M of the array in device memory (gw_rollout_backlog_population keeps no
// seen_len)
__global__ __launch_bounds__(256) void backlog_select_pop_rows(uint32_t N, uint32_t D, uint32_t RB, uint32_t md, uint32_t M,
                                                               const gw_backlog_policy* __restrict__ policies,
                                                               const uint8_t* __restrict__ qb, int32_t* __restrict__ device_out,
                                                               int32_t* __restrict__ duration_out)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    uint32_t d, du, q;
    gw_backlog_select<true>(qb + (size_t)e * RB, D, md, policies[e / M], d, du, q);
    device_out[e] = (int32_t)d;
    duration_out[e] = (int32_t)du;
}

} // namespace

// gw_rollout_backlog: gw_rollout_autoreset_scored's rules (the policy's LDS copy is static too).  out.device / out.duration:
// where the chosen actions go.
int gw_launch_rollout_backlog_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_backlog_policy& pol,
                                  const gw_episodes& ep, const gw_score& score, int32_t* obs_next, const GwRows& out, int32_t* seen_len,
                                  int32_t* delivered)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_NO_TABLE)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_BACKLOG, GW_FUSED_NO_TABLE, GW_KERNEL_OF(ct_rollout_backlog), episode_args(ep, obs_next),
                        score, pol, out.device, out.duration, seen_len, out.obs, out.reward, out.done, out.ended, delivered);
}
// ... and its per-step form's choice for one step, into row.device / row.duration / seen_len (default queue mode: st.qb)
int gw_launch_backlog_select(const GwState& st, const GwDevConst& cst, const gw_backlog_policy& pol, const GwRows& row, int32_t* seen_len,
                             void* stream)
{
    hipLaunchKernelGGL(backlog_select_rows, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)st.N,
                       (uint32_t)st.D, (uint32_t)st.RB, (uint32_t)cst.max_duration, pol, (const uint8_t*)st.qb, row.device, row.duration,
                       seen_len);
    return gw_launch_status();
}

// gw_rollout_backlog_population: gw_rollout_backlog's rules, and envs_per_policy a multiple of 64, so that no wave spans two
// policies.  (The caller has checked num_policies * envs_per_policy == N: every block's policy index is below num_policies.)
int gw_launch_rollout_backlog_pop_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_backlog_population& pop,
                                      const gw_episodes& ep, const gw_score& score, int32_t* obs_next)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_NO_TABLE) || pop.envs_per_policy % 64 != 0) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_BACKLOG_POP, GW_FUSED_NO_TABLE, GW_KERNEL_OF(ct_rollout_backlog_pop),
                        episode_args(ep, obs_next), score, pop.policies_dev, (uint32_t)pop.envs_per_policy, pop.tally_dev);
}
// ... and its per-step form's choice for one step, into row.device / row.duration (default queue mode: st.qb)
int gw_launch_backlog_select_pop(const GwState& st, const GwDevConst& cst, const gw_backlog_population& pop, const GwRows& row, void* stream)
{
    hipLaunchKernelGGL(backlog_select_pop_rows, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)st.N,
                       (uint32_t)st.D, (uint32_t)st.RB, (uint32_t)cst.max_duration, (uint32_t)pop.envs_per_policy, pop.policies_dev,
                       (const uint8_t*)st.qb, row.device, row.duration);
    return gw_launch_status();
}
