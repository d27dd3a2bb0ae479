// ct_rollout_stats.hip -- the tally: closed loops that count every transition into a table over (observation class, action)
// instead of storing it.  Serves gw_rollout_policy_stats (ct_rollout_pstats, gw_launch_rollout_pstats_sfx),
// gw_rollout_episodes_stats (ct_rollout_pstats_ep, gw_launch_rollout_pstats_ep_sfx) and gw_transition_stats /
// gw_transition_stats_ep (transition_stats_rows, gw_launch_transition_stats).  The draw, the episode's book and the launcher:
// ct_rollout_sync.hip.h.  Behind them, the same three with the packets a step delivered as an eighth column -- the _delivered
// calls: ct_rollout_pstats_d, ct_rollout_pstats_epd, transition_stats_rows_d and their launchers.
#include "ct_rollout_sync.hip.h"

namespace {

// ---- the tally: gw_rollout_policy_stats and gw_transition_stats (include/gymwipe_amd.h: int64 table[3][A][GW_TS_COLS]) --------
// Everything a learner or an evaluator takes from a transition of this env is a function of (observation class, flat action):
// the kernels below count into a per-block histogram in LDS and add its non-empty bins to the caller's table once per block.
// A bin is two 64-bit words, each updated by ONE LDS atomic add per transition:
//     word 0   bits  0-12 / 13-25 / 26-38   transitions whose next observation was below / at / above counter_bound
//              bits 39-51                   transitions with done != 0                      (n = the sum of the first three)
//     word 1   bits  0-16  sum of (reward + 10)        bits 17-35  sum of reward^2
// Bit budget: between zeroing and flush a histogram takes at most TS_EVENTS transitions -- one wave of 64 envs over at most
// TS_STEPS = 64 steps in ct_rollout_pstats, a tile of TS_EVENTS rows in transition_stats_rows -- and a reward is an integer in
// [-10, 10] (ct_rollout_sync_body.h clamps it; transition_stats_rows rounds and clamps what it reads).  So a count is at most
// 4 096 < 2^13, sum(reward + 10) at most 20 * 4 096 < 2^17, sum(reward^2) at most 100 * 4 096 < 2^19: no field carries into
// its neighbour.  Integer adds commute, in LDS and in the table alike: the result does not depend on the order of arrival.
constexpr uint32_t TS_EVENTS = 64 * TS_STEPS;            // (TS_STEPS, TS_BIN_BYTES, gw_ts_add, gw_wave_lds_order: ct_rollout_sync.hip.h)
constexpr int TS_CNT_BITS = 13, TS_RS_BITS = 17, TS_RQ_BITS = 19;
constexpr int TS_RMAX = 10;
static_assert(TS_EVENTS < (1u << TS_CNT_BITS), "a count field overflows into its neighbour");
static_assert(2 * TS_RMAX * TS_EVENTS < (1u << TS_RS_BITS), "the reward-sum field overflows");
static_assert(TS_RMAX * TS_RMAX * TS_EVENTS < (1u << TS_RQ_BITS), "the reward-square-sum field overflows");
static_assert(4 * TS_CNT_BITS <= 64 && TS_RS_BITS + TS_RQ_BITS <= 64, "a bin is two 64-bit words");
static_assert(TS_BIN_BYTES == 2 * sizeof(uint64_t), "a bin is two 64-bit words");

// one transition into the LDS histogram: bin = cls * A + a, next_cls in [0, 3), r in [-TS_RMAX, TS_RMAX]
__device__ __forceinline__ void gw_ts_count(uint64_t* hist, uint32_t bin, uint32_t next_cls, int32_t r, uint32_t dn)
{
    const uint64_t w0 = (1ull << (TS_CNT_BITS * next_cls)) | ((uint64_t)(dn != 0u ? 1u : 0u) << (3 * TS_CNT_BITS));
    const uint64_t w1 = (uint64_t)(uint32_t)(r + TS_RMAX) | ((uint64_t)(uint32_t)(r * r) << TS_RS_BITS);
    __hip_atomic_fetch_add(hist + 2u * bin, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(hist + 2u * bin + 1u, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the seven columns of one (cls, a) pair into the table (a zero adds nothing and is not sent)
__device__ __forceinline__ void gw_ts_row(int64_t* row, uint64_t n0, uint64_t n1, uint64_t n2, uint64_t dn, int64_t rs, uint64_t rq)
{
    gw_ts_add(row + 0, n0 + n1 + n2);
    if (rs != 0) gw_ts_add(row + 1, (uint64_t)rs);
    if (rq != 0u) gw_ts_add(row + 2, rq);
    if (n0 != 0u) gw_ts_add(row + 3, n0);
    if (n1 != 0u) gw_ts_add(row + 4, n1);
    if (n2 != 0u) gw_ts_add(row + 5, n2);
    if (dn != 0u) gw_ts_add(row + 6, dn);
}
// The histogram's non-empty bins into the table: lane `first` of `stride` takes every stride-th bin.  The caller has ordered
// the LDS adds before this (a barrier, or a fence within the one wave that made them).
__device__ __forceinline__ void gw_ts_flush(const uint64_t* hist, uint32_t bins, uint32_t first, uint32_t stride, int64_t* table)
{
    constexpr uint64_t CM = (1ull << TS_CNT_BITS) - 1u;
    for (uint32_t b = first; b < bins; b += stride) {
        const uint64_t w0 = hist[2u * b];
        if (w0 == 0u) continue;                          // every transition sets one of the next-observation counts
        const uint64_t w1 = hist[2u * b + 1u];
        const uint64_t n0 = w0 & CM, n1 = (w0 >> TS_CNT_BITS) & CM, n2 = (w0 >> (2 * TS_CNT_BITS)) & CM;
        const int64_t rs = (int64_t)(w1 & ((1ull << TS_RS_BITS) - 1u)) - (int64_t)TS_RMAX * (int64_t)(n0 + n1 + n2);
        gw_ts_row(table + (size_t)b * GW_TS_COLS, n0, n1, n2, (w0 >> (3 * TS_CNT_BITS)) & CM, rs,
                  (w1 >> TS_RS_BITS) & ((1ull << TS_RQ_BITS) - 1u));
    }
}

// What gw_rollout_policy_stats passes on to ct_rollout_pstats.  obs_prev and obs_last may be one array (an env reads its own
// element before the step loop and writes it after).  (Not GwPolicyArgs plus three pointers: the kernel's signature is part
// of its symbol, and its argument layout of its code.)
struct GwStatsArgs {
    const uint32_t* cdf;          // [3][A]
    const int32_t* obs_prev;      // [N]
    int32_t* obs_last;            // [N]
    int32_t* ret;                 // [N] += the env's reward sum, or nullptr
    int64_t* table;               // [3][A][GW_TS_COLS]
    uint64_t seed, step0, env0;
};

// The draw of a kernel that tallies: the histogram in front of the table's copy in the launch's dynamic LDS -- [3 * A] bins of
// two words, then 3 * A words.
struct StatsDraw : PolicyDraw {
    uint64_t* s_hist;
    __device__ __forceinline__ void hist_at(uint64_t* dyn)
    {
        s_hist = dyn;
        table_at(reinterpret_cast<uint32_t*>(dyn + 6u * A));
    }
    __device__ __forceinline__ void stage() const
    {
        for (uint32_t i = threadIdx.x; i < 6u * A; i += blockDim.x) s_hist[i] = 0u;
        stage_cdf();
    }
};

// The draw without the action stores, and the step's outcome into the histogram instead of three output arrays.
struct StatsActions : StatsDraw {
    int32_t center;                                      // (as PolicyActions')
    int32_t ret, latest_last;
    // step k is over: one transition of the bin its action was drawn for; the next action from what the agent now sees.
    // (Spelled out, not through next(): with latest_next in latest_last's place and the class computed a second time all 30
    // instantiations of ct_rollout_pstats came out different.)
    __device__ __forceinline__ void stepped(int k, int K, int32_t latest, int32_t r, uint32_t dn)
    {
        const uint32_t next_cls = (uint32_t)((int)(latest > 0) - (int)(latest < 0) + 1);
        gw_ts_count(s_hist, bin_cur, next_cls, r, dn);
        ret += r;
        latest_last = latest;
        if (k + 1 < K) draw(next_cls, step0 + (uint64_t)(k + 1));
    }
};

// gw_rollout_policy_stats: ct_rollout_policy's closed loop with none of its five output streams.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pstats(GwState st, GwDevConst c, int K, GwStatsArgs p)
{
    extern __shared__ uint64_t s_stats_dyn[];
    StatsActions src;
    src.init({p.cdf, p.obs_prev, p.seed, p.step0, p.env0}, c, DT == 0 ? c.D : DT);
    src.hist_at(s_stats_dyn);
    src.center = c.counter_bound;
    src.ret = 0; src.latest_last = 0;
#define GW_ROLLOUT_SRC_STAGE src.stage();
#define GW_ROLLOUT_SRC_FIRST src.first(e, p.obs_prev[e], src.center);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn) (void)at; src.stepped(k, K, latest, r, dn);
#include "ct_rollout_sync_body.h"
    p.obs_last[e] = src.latest_last + c.counter_bound;
    if (p.ret) p.ret[e] += src.ret;
    // the wave's lanes that have an env (all 64 but in the last block) share the bins out among themselves
    gw_wave_lds_order();
    gw_ts_flush(src.s_hist, 3u * src.A, threadIdx.x, gw_min_u32(64u, N - blockIdx.x * 64u), p.table);
}

// ct_rollout_pstats' source with the episode's book.  A transition is counted under the class the env acted on (the reset's
// observation after an episode's end), with the next observation and done the step returned.
struct EpisodeStatsActions : StatsDraw {
    EpisodeBook ep;
    __device__ __forceinline__ void stepped(int k, int K, int32_t latest, int32_t r, uint32_t dn, uint32_t cause)
    {
        gw_ts_count(s_hist, bin_cur, (uint32_t)((int)(latest > 0) - (int)(latest < 0) + 1), r, dn);
        next(k, K, cause ? 0 : latest);
    }
};

template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pstats_ep(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, int64_t* table)
{
    extern __shared__ uint64_t s_stats_dyn[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    EpisodeStatsActions src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.hist_at(s_stats_dyn);
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage(); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        const uint32_t dn_step = dn;                     /* (a reset clears the body's dn) */                                    \
        GW_ROLLOUT_EP_STEPPED(r, dn_step)                                                                                        \
        src.stepped(k, K, latest, r, dn_step, cause_next);                                                                       \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
    gw_ts_flush(src.s_hist, 3u * src.A, threadIdx.x, gw_min_u32(64u, N - blockIdx.x * 64u), table);
}

// gw_transition_stats: the same table from recorded [K][N] transitions.  A block takes tiles of TS_EVENTS consecutive
// elements (the histogram's bit budget), 16 per thread, and flushes after each.  Any content is safe: a row whose action lies
// outside the action space is skipped, a reward is rounded to nearest and clamped (NaN counts as -10), done is != 0.
// LDS = false (a histogram of 3 * A bins would not fit): every row's seven columns straight into the table.
// EP (gw_transition_stats_ep): rows recorded by gw_rollout_episodes -- where ended[k - 1] != 0 step k acted on the reset's
// observation, counter_bound.
template <bool LDS, bool EP>
__global__ __launch_bounds__(256) void transition_stats_rows(uint64_t total, uint32_t N, uint32_t D, uint32_t md, int32_t center,
                                                            const int32_t* __restrict__ obs_prev, const int32_t* __restrict__ device,
                                                            const int32_t* __restrict__ duration, const int32_t* __restrict__ obs,
                                                            const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            const uint8_t* __restrict__ ended, int64_t* __restrict__ table)
{
    extern __shared__ uint64_t s_stats_dyn[];
    const uint64_t A = (uint64_t)D * md;
    const uint64_t tiles = (total + TS_EVENTS - 1u) / TS_EVENTS;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if constexpr (LDS) {
            for (uint32_t i = threadIdx.x; i < 6u * (uint32_t)A; i += blockDim.x) s_stats_dyn[i] = 0u;
            __syncthreads();
        }
#pragma unroll 4
        for (uint32_t j = 0; j < TS_EVENTS / 256u; ++j) {
            const uint64_t i = tile * TS_EVENTS + j * 256u + threadIdx.x;
            if (i >= total) break;
            const uint32_t dv = (uint32_t)device[i], du = (uint32_t)duration[i];
            if (dv >= D || du >= md) continue;                                  // a GW_FLAG_BADACT step: the env did nothing
            int32_t seen = i < N ? obs_prev[i] : obs[i - N];                    // row k - 1 of obs, same env
            if constexpr (EP) seen = (i >= N && ended[i - N] != 0) ? center : seen;
            const float x = rintf(reward[i]);
            const int32_t r = (int32_t)(x >= (float)-TS_RMAX ? (x <= (float)TS_RMAX ? x : (float)TS_RMAX) : (float)-TS_RMAX);
            const uint32_t next_cls = gw_policy_cls(obs[i], center), dn = done[i];
            const uint64_t bin = (uint64_t)gw_policy_cls(seen, center) * A + (uint64_t)dv * md + du;
            if constexpr (LDS) {
                gw_ts_count(s_stats_dyn, (uint32_t)bin, next_cls, r, dn);
            } else {
                gw_ts_row(table + bin * GW_TS_COLS, next_cls == 0u, next_cls == 1u, next_cls == 2u, dn != 0u, r, (uint64_t)(r * r));
            }
        }
        if constexpr (LDS) {
            __syncthreads();
            gw_ts_flush(s_stats_dyn, 3u * (uint32_t)A, threadIdx.x, blockDim.x, table);
            __syncthreads();
        }
    }
}

} // namespace

// The two tallying forms return GW_EUNSUPPORTED where there is no fused launch (fused_unavailable), and the call is refused
// before its first launch.
int gw_launch_rollout_pstats_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                 const int32_t* obs_prev, int32_t* obs_last, int32_t* ret, int64_t* table)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_HIST)) return GW_EUNSUPPORTED;
    const GwStatsArgs p = {pol.cdf, obs_prev, obs_last, ret, table, pol.seed, pol.step0, pol.env_id0};
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_PSTATS, GW_FUSED_TABLE_HIST, GW_KERNEL_OF(ct_rollout_pstats), p);
}

int gw_launch_transition_stats(int64_t N, int K, int D, int max_duration, int counter_bound, const int32_t* obs_prev,
                               const int32_t* device, const int32_t* duration, const int32_t* obs, const float* reward,
                               const uint8_t* done, const uint8_t* ended, int64_t* table, void* stream)
{
    const uint64_t total = (uint64_t)N * (uint64_t)K, tiles = (total + TS_EVENTS - 1u) / TS_EVENTS;
    if (total == 0u) return GW_OK;
    const uint64_t A = (uint64_t)D * (uint64_t)max_duration;
    const size_t dyn = (size_t)(3u * A) * TS_BIN_BYTES;
    const unsigned grid = (unsigned)(tiles < 4096u ? tiles : 4096u);
    const bool lds = dyn <= GW_LDS_PER_BLOCK / 2;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds ? dyn : 0, (hipStream_t)stream, total, (uint32_t)N, (uint32_t)D,
                           (uint32_t)max_duration, counter_bound, obs_prev, device, duration, obs, reward, done, ended, table);
    };
    if (ended) { if (lds) launch(transition_stats_rows<true, true>); else launch(transition_stats_rows<false, true>); }
    else       { if (lds) launch(transition_stats_rows<true, false>); else launch(transition_stats_rows<false, false>); }
    return gw_launch_status();
}

// gw_rollout_episodes_stats: its parent's rules, with the caller's gw_episodes and obs_next passed on.
int gw_launch_rollout_pstats_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                    const gw_episodes& ep, const int32_t* obs_prev, int32_t* obs_next, int64_t* table)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_HIST)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_PSTATS_EP, GW_FUSED_TABLE_HIST, GW_KERNEL_OF(ct_rollout_pstats_ep),
                        policy_args(pol, obs_prev), episode_args(ep, obs_next), table);
}

// ---- the tally with the packets a step delivered: the _delivered calls (include/gymwipe_amd.h: int64 table[3][A][GW_TSD_COLS]) ----
// A step's score is linear -- w_reward * reward + w_delivered[sender] * delivered -- and the flat action names the sender, so a
// bin's score sum under ANY gw_score is w_reward * (column 1) + w_delivered[a / max_duration] * (sum of delivered): the table
// needs one more sum per bin and no weights.  That sum rides in the bits word 1 has left:
//     word 1   bits  0-16  sum of (reward + 10)        bits 17-35  sum of reward^2        bits 36-63  sum of min(delivered, 65 535)
// 65 535 * 4 096 < 2^28, so the field cannot wrap within a histogram's TS_EVENTS transitions: the same two LDS atomics per
// transition, the same TS_BIN_BYTES, the same availability (GW_FUSED_TABLE_HIST).  The kernels below are their parents' sources
// with that field, kept apart from them so that every parent stays instruction for instruction what it was.
namespace {

constexpr int TS_DL_SHIFT = TS_RS_BITS + TS_RQ_BITS, TS_DL_BITS = 28;
constexpr uint32_t TS_DL_MAX = 65535u;
static_assert(TS_DL_SHIFT == 36 && TS_DL_SHIFT + TS_DL_BITS <= 64, "the delivered sum lies in word 1's bits 36-63");
static_assert((uint64_t)TS_DL_MAX * TS_EVENTS < (1ull << TS_DL_BITS), "the delivered-sum field overflows");

// gw_ts_count with the step's packets: dl is clamped to TS_DL_MAX here
__device__ __forceinline__ void gw_ts_count_d(uint64_t* hist, uint32_t bin, uint32_t next_cls, int32_t r, uint32_t dn, uint32_t dl)
{
    const uint64_t w0 = (1ull << (TS_CNT_BITS * next_cls)) | ((uint64_t)(dn != 0u ? 1u : 0u) << (3 * TS_CNT_BITS));
    const uint64_t w1 = (uint64_t)(uint32_t)(r + TS_RMAX) | ((uint64_t)(uint32_t)(r * r) << TS_RS_BITS) |
                        ((uint64_t)gw_min_u32(dl, TS_DL_MAX) << TS_DL_SHIFT);
    __hip_atomic_fetch_add(hist + 2u * bin, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(hist + 2u * bin + 1u, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the eight columns of one (cls, a) pair: `row` is a row of GW_TSD_COLS
__device__ __forceinline__ void gw_ts_row_d(int64_t* row, uint64_t n0, uint64_t n1, uint64_t n2, uint64_t dn, int64_t rs, uint64_t rq,
                                            uint64_t dl)
{
    gw_ts_row(row, n0, n1, n2, dn, rs, rq);
    if (dl != 0u) gw_ts_add(row + 7, dl);
}
// gw_ts_flush into a table of GW_TSD_COLS columns.  Every block of a launch flushes at about the same time and adds into the same
// rows; each starts at a bin of its own (rot, the same for all of its threads), so that the blocks do not queue up at one row
// after the other together.
__device__ __forceinline__ void gw_ts_flush_d(const uint64_t* hist, uint32_t bins, uint32_t first, uint32_t stride, int64_t* table)
{
    constexpr uint64_t CM = (1ull << TS_CNT_BITS) - 1u;
    const uint32_t rot = (blockIdx.x * 37u) % bins;
    for (uint32_t i = first; i < bins; i += stride) {
        const uint32_t b = i + rot < bins ? i + rot : i + rot - bins;
        const uint64_t w0 = hist[2u * b];
        if (w0 == 0u) continue;
        const uint64_t w1 = hist[2u * b + 1u];
        const uint64_t n0 = w0 & CM, n1 = (w0 >> TS_CNT_BITS) & CM, n2 = (w0 >> (2 * TS_CNT_BITS)) & CM;
        const int64_t rs = (int64_t)(w1 & ((1ull << TS_RS_BITS) - 1u)) - (int64_t)TS_RMAX * (int64_t)(n0 + n1 + n2);
        gw_ts_row_d(table + (size_t)b * GW_TSD_COLS, n0, n1, n2, (w0 >> (3 * TS_CNT_BITS)) & CM, rs,
                    (w1 >> TS_RS_BITS) & ((1ull << TS_RQ_BITS) - 1u), w1 >> TS_DL_SHIFT);
    }
}

// StatsActions with the body's running kt.deliv as it stood when the step being walked began.  The counter restarts at 0 in
// every launch, and the baseline with it (GW_ROLLOUT_SRC_FIRST, as StepScore::first); a reset inside the launch leaves it alone.
struct StatsActionsD : StatsDraw {
    int32_t center;
    int32_t ret, latest_last;
    uint32_t deliv_next;
    __device__ __forceinline__ void stepped(int k, int K, int32_t latest, int32_t r, uint32_t dn, uint32_t deliv_now)
    {
        const uint32_t next_cls = (uint32_t)((int)(latest > 0) - (int)(latest < 0) + 1);
        gw_ts_count_d(s_hist, bin_cur, next_cls, r, dn, deliv_now - deliv_next);
        deliv_next = deliv_now;
        ret += r;
        latest_last = latest;
        if (k + 1 < K) draw(next_cls, step0 + (uint64_t)(k + 1));
    }
};

// gw_rollout_policy_stats_delivered: ct_rollout_pstats with the packets per step in the tally
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pstats_d(GwState st, GwDevConst c, int K, GwStatsArgs p)
{
    extern __shared__ uint64_t s_stats_dyn[];
    StatsActionsD src;
    src.init({p.cdf, p.obs_prev, p.seed, p.step0, p.env0}, c, DT == 0 ? c.D : DT);
    src.hist_at(s_stats_dyn);
    src.center = c.counter_bound;
    src.ret = 0; src.latest_last = 0; src.deliv_next = 0u;
#define GW_ROLLOUT_SRC_STAGE src.stage();
#define GW_ROLLOUT_SRC_FIRST src.deliv_next = 0u; src.first(e, p.obs_prev[e], src.center);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn) (void)at; src.stepped(k, K, latest, r, dn, kt.deliv);
#include "ct_rollout_sync_body.h"
    p.obs_last[e] = src.latest_last + c.counter_bound;
    if (p.ret) p.ret[e] += src.ret;
    gw_wave_lds_order();
    gw_ts_flush_d(src.s_hist, 3u * src.A, threadIdx.x, gw_min_u32(64u, N - blockIdx.x * 64u), p.table);
}

struct EpisodeStatsActionsD : StatsDraw {
    EpisodeBook ep;
    uint32_t deliv_next;
    __device__ __forceinline__ void stepped(int k, int K, int32_t latest, int32_t r, uint32_t dn, uint32_t cause, uint32_t deliv_now)
    {
        gw_ts_count_d(s_hist, bin_cur, (uint32_t)((int)(latest > 0) - (int)(latest < 0) + 1), r, dn, deliv_now - deliv_next);
        deliv_next = deliv_now;
        next(k, K, cause ? 0 : latest);
    }
};

// gw_rollout_episodes_stats_delivered: ct_rollout_pstats_ep with the packets per step in the tally.  The book keeps the built-in
// reward, as its parent's does: the table is score-free.
template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_pstats_epd(GwState st, GwDevConst c, int K, GwPolicyArgs p, GwEpisodeArgs ea, int64_t* table)
{
    extern __shared__ uint64_t s_stats_dyn[];
    __shared__ unsigned long long s_ep_tally[GW_EP_COLS];
    EpisodeStatsActionsD src;
    src.init(p, c, DT == 0 ? c.D : DT);
    src.hist_at(s_stats_dyn);
    src.deliv_next = 0u;
#define GW_ROLLOUT_SRC_RESETS
#define GW_ROLLOUT_SRC_STAGE src.stage(); gw_ep_zero(s_ep_tally);
#define GW_ROLLOUT_SRC_FIRST src.ep.load(ea, e); src.deliv_next = 0u; src.first(e, p.obs_prev[e], c.counter_bound);
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_DRAWN_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_DRAWN_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn)                                                                                \
    (void)at;                                                                                                                    \
    {                                                                                                                            \
        const uint32_t dn_step = dn;                     /* (a reset clears the body's dn) */                                    \
        GW_ROLLOUT_EP_STEPPED(r, dn_step)                                                                                        \
        src.stepped(k, K, latest, r, dn_step, cause_next, kt.deliv);                                                             \
    }
#include "ct_rollout_sync_body.h"
    GW_ROLLOUT_EP_TAIL(false, nullptr)
    gw_ts_flush_d(src.s_hist, 3u * src.A, threadIdx.x, gw_min_u32(64u, N - blockIdx.x * 64u), table);
}

// gw_transition_stats_delivered: transition_stats_rows with a row of packets per step -- a negative count is 0, one above
// TS_DL_MAX is TS_DL_MAX.  The direct form (LDS = false) makes an eighth add where the count is not 0.
template <bool LDS, bool EP>
__global__ __launch_bounds__(256) void transition_stats_rows_d(uint64_t total, uint32_t N, uint32_t D, uint32_t md, int32_t center,
                                                              const int32_t* __restrict__ obs_prev, const int32_t* __restrict__ device,
                                                              const int32_t* __restrict__ duration, const int32_t* __restrict__ obs,
                                                              const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                              const uint8_t* __restrict__ ended, const int32_t* __restrict__ delivered,
                                                              int64_t* __restrict__ table)
{
    extern __shared__ uint64_t s_stats_dyn[];
    const uint64_t A = (uint64_t)D * md;
    const uint64_t tiles = (total + TS_EVENTS - 1u) / TS_EVENTS;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if constexpr (LDS) {
            for (uint32_t i = threadIdx.x; i < 6u * (uint32_t)A; i += blockDim.x) s_stats_dyn[i] = 0u;
            __syncthreads();
        }
#pragma unroll 4
        for (uint32_t j = 0; j < TS_EVENTS / 256u; ++j) {
            const uint64_t i = tile * TS_EVENTS + j * 256u + threadIdx.x;
            if (i >= total) break;
            const uint32_t dv = (uint32_t)device[i], du = (uint32_t)duration[i];
            if (dv >= D || du >= md) continue;                                  // a GW_FLAG_BADACT step: the env did nothing
            int32_t seen = i < N ? obs_prev[i] : obs[i - N];                    // row k - 1 of obs, same env
            if constexpr (EP) seen = (i >= N && ended[i - N] != 0) ? center : seen;
            const float x = rintf(reward[i]);
            const int32_t r = (int32_t)(x >= (float)-TS_RMAX ? (x <= (float)TS_RMAX ? x : (float)TS_RMAX) : (float)-TS_RMAX);
            const int32_t dl_in = delivered[i];
            const uint32_t dl = dl_in < 0 ? 0u : gw_min_u32((uint32_t)dl_in, TS_DL_MAX);
            const uint32_t next_cls = gw_policy_cls(obs[i], center), dn = done[i];
            const uint64_t bin = (uint64_t)gw_policy_cls(seen, center) * A + (uint64_t)dv * md + du;
            if constexpr (LDS) {
                gw_ts_count_d(s_stats_dyn, (uint32_t)bin, next_cls, r, dn, dl);
            } else {
                gw_ts_row_d(table + bin * GW_TSD_COLS, next_cls == 0u, next_cls == 1u, next_cls == 2u, dn != 0u, r, (uint64_t)(r * r), dl);
            }
        }
        if constexpr (LDS) {
            __syncthreads();
            gw_ts_flush_d(s_stats_dyn, 3u * (uint32_t)A, threadIdx.x, blockDim.x, table);
            __syncthreads();
        }
    }
}

} // namespace

int gw_launch_rollout_pstats_d_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                   const int32_t* obs_prev, int32_t* obs_last, int32_t* ret, int64_t* table)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_HIST)) return GW_EUNSUPPORTED;
    const GwStatsArgs p = {pol.cdf, obs_prev, obs_last, ret, table, pol.seed, pol.step0, pol.env_id0};
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_PSTATS_D, GW_FUSED_TABLE_HIST, GW_KERNEL_OF(ct_rollout_pstats_d), p);
}

int gw_launch_rollout_pstats_epd_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                     const gw_episodes& ep, const int32_t* obs_prev, int32_t* obs_next, int64_t* table)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_HIST)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_PSTATS_EPD, GW_FUSED_TABLE_HIST, GW_KERNEL_OF(ct_rollout_pstats_epd),
                        policy_args(pol, obs_prev), episode_args(ep, obs_next), table);
}

int gw_launch_transition_stats_d(int64_t N, int K, int D, int max_duration, int counter_bound, const int32_t* obs_prev,
                                 const int32_t* device, const int32_t* duration, const int32_t* obs, const float* reward,
                                 const uint8_t* done, const uint8_t* ended, const int32_t* delivered, int64_t* table, void* stream)
{
    const uint64_t total = (uint64_t)N * (uint64_t)K, tiles = (total + TS_EVENTS - 1u) / TS_EVENTS;
    if (total == 0u) return GW_OK;
    const uint64_t A = (uint64_t)D * (uint64_t)max_duration;
    const size_t dyn = (size_t)(3u * A) * TS_BIN_BYTES;
    const unsigned grid = (unsigned)(tiles < 4096u ? tiles : 4096u);
    const bool lds = dyn <= GW_LDS_PER_BLOCK / 2;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds ? dyn : 0, (hipStream_t)stream, total, (uint32_t)N, (uint32_t)D,
                           (uint32_t)max_duration, counter_bound, obs_prev, device, duration, obs, reward, done, ended, delivered, table);
    };
    if (ended) { if (lds) launch(transition_stats_rows_d<true, true>); else launch(transition_stats_rows_d<false, true>); }
    else       { if (lds) launch(transition_stats_rows_d<true, false>); else launch(transition_stats_rows_d<false, false>); }
    return gw_launch_status();
}
