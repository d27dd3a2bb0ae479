// ct_rollout_sync.hip.h -- what the step-synchronous rollout families share, on the device and on the host side.  Each family
// file (the catalogue below names them) includes this once; everything here has internal linkage, so every file carries its own
// copy of what it uses and the families meet nowhere but in gw_internal.h's launcher declarations.
//   device side   the per-lane arrays (RegArr ... ArrSel, the event loop's too), the policy's draw (gw_policy_*, GwPolicyArgs,
//                 PolicyDraw), the staged / drawn action hooks and GW_ROLLOUT_STORE_OUTPUTS, the episode's book and the episodic
//                 tail (GwEpisodeArgs, EpisodeBook, GW_ROLLOUT_EP_*), the step's score (StepScore), and the sources that files
//                 other than their kernel's derive from (StagedEpisodes, ScoredStagedEpisodes, ScoredEpisodeActions,
//                 ScoredPopulationActions)
//   host side     fused_unavailable, launch_fused, launch_fused_lds, GW_KERNEL_OF, policy_args, episode_args
// The loop's body itself is ct_rollout_sync_body.h.  The step semantics and reference citations are those of ct_step_sfx.hip /
// ct_common.hip.h.
#pragma once
#include "ct_common.hip.h"
#include "gw_dispatch.h"
#include "gw_queue.h"

using namespace gwk;

namespace {

// Per-lane arrays of the rollout kernel.  DT > 0: registers (every loop over senders is unrolled, indices are static);
// DT == 0 (any sender count): one LDS column per lane -- the same source lines index either.
template <int N>
struct RegArr {
    uint32_t v[N];
    __device__ __forceinline__ uint32_t& operator[](int i) { return v[i]; }
};
struct LdsArr {
    uint32_t* p;                                         // this lane's column: element i at p[i * 64]
    __device__ __forceinline__ uint32_t& operator[](int i) const { return p[i << 6]; }
};
template <int N> struct ConstRegArr {
    uint32_t v[N];
    __device__ __forceinline__ uint32_t operator[](int i) const { return v[i]; }
};
struct ConstMemArr {                                     // wave-uniform index into the handle's constants in device memory
    const void* p; int shift16;
    __device__ __forceinline__ uint32_t operator[](int i) const
    {
        return shift16 ? (uint32_t)reinterpret_cast<const uint16_t*>(p)[i] : reinterpret_cast<const uint32_t*>(p)[i];
    }
};
template <bool GEN, int N> struct ArrSel { typedef RegArr<N> rw; typedef ConstRegArr<N> ro; };
template <int N> struct ArrSel<true, N> { typedef LdsArr rw; typedef ConstMemArr ro; };

// ---- the step-synchronous form (every sender count) --------------------------------------------------------------
// The event loop (ct_rollout_sfx.hip) was built when a data packet cost as much as an announcement (one pass of a
// ~140-instruction body either way) and letting lanes run ahead of each other evened the work out.  Since the window loop
// has a straight-line form (ct_step_sfx.hip: ~45 instructions per packet, every per-packet decision settled for the step up
// front), a packet is a third of an announcement, and the lock-step of whole steps costs less than the event loop's ~60 exec-mask regions per pass: here
// every lane takes step k together -- announcement, window (straight line, general loop where that declines), feedback -- with
// the env's state in registers across all K steps, queue lengths of the senders not addressed and the ticks behind a window
// lazy exactly as there; DT == 0 = any sender count, the per-lane arrays as LDS columns.  Same results bit for bit (the tests
// run both forms against the oracle; GW_ROLLOUT_EVENT_LOOP=1 selects the event loop).
//
// Where a step's action comes from is the loop's one parameter, so that its body exists once (ct_rollout_sync_body.h).  The
// families, each with the file that holds its kernel and its launcher:
//   ct_rollout_sync_kernel  gw_rollout: the caller's pre-staged rows, step k + 1's action loaded while step k is walked
//                           (ct_rollout_sfx.hip);
//   ct_rollout_policy       gw_rollout_policy: drawn at the step boundary from a three-row table over the observation the
//                           env just produced (PolicyActions), and stored with that step's outputs (ct_rollout_policy.hip).
//   ct_rollout_pstats       gw_rollout_policy_stats: the same draw, nothing stored per step -- the transition is counted into a
//                           table over (observation class, action) instead (StatsActions; ct_rollout_stats.hip).
//   ct_rollout_policy_ep    gw_rollout_episodes: ct_rollout_policy with episodes -- an env whose step returned done, or whose
//   ct_rollout_pstats_ep    episode reached its step limit, is reset in registers at the step boundary and draws its next
//                           action from the reset's observation; gw_rollout_episodes_stats: the same with ct_rollout_pstats' tally
//                           (ct_rollout_policy.hip, ct_rollout_stats.hip).
//   ct_rollout_sync_ep      gw_rollout_autoreset: ct_rollout_sync_kernel's staged rows with the same episodes -- the caller's
//                           actions, the launch's resets (ct_rollout_autoreset.hip).
//   ct_rollout_pop_ep       gw_rollout_population: ct_rollout_policy_ep with one table per block and nothing stored per step
//                           (ct_rollout_pop.hip).
//   ct_rollout_policy_eps   gw_rollout_episodes_scored / gw_rollout_population_scored: the two before with the step's score --
//   ct_rollout_pop_eps      the reward and the packets the step delivered, weighted -- where they have the reward
//                           (ct_rollout_policy.hip, ct_rollout_pop.hip).
//   ct_rollout_sync_eps     gw_rollout_autoreset_scored: ct_rollout_sync_ep with the same score, the sender the caller's
//                           (ct_rollout_autoreset.hip).
//   ct_rollout_backlog      gw_rollout_backlog: ct_rollout_sync_eps with the action chosen at the step boundary from the queue
//                           lengths, which the body brings to the current tick there (BacklogEpisodes; ct_rollout_backlog.hip).
//   ct_rollout_backlog_pop  gw_rollout_backlog_population: ct_rollout_backlog with one policy per block, read from device memory,
//                           and nothing stored per step (as ct_rollout_pop_eps; ct_rollout_backlog.hip).
//   ct_rollout_fsc          gw_rollout_controller / gw_rollout_controller_population: ct_rollout_policy_eps / ct_rollout_pop_eps
//   ct_rollout_fsc_pop      with a finite-state controller -- the env's node picks which three rows of the table the draw reads,
//                           and moves on the new observation class and on whether the step delivered enough
//                           (ct_rollout_fsc.hip).
// A launcher stays in the file that holds every kernel it may launch.  The per-step forms' small row kernels live beside the
// family they serve: policy_sample_kernel (ct_rollout_policy.hip), episodes_step_kernel (ct_rollout_autoreset.hip),
// backlog_select_rows / backlog_select_pop_rows (ct_rollout_backlog.hip), transition_stats_rows (ct_rollout_stats.hip).
// The policy's draw (include/gymwipe_amd.h, gw_rollout_policy): the first 32 bits of the action stream's hash
// (gymwipe_amd/actions.py) against the observation class's row of the table.
__device__ __forceinline__ uint32_t gw_policy_u(uint64_t seed, uint64_t env_term, uint64_t step)
{
    uint64_t z = seed ^ env_term ^ (step * 0xD1B54A32D192ED03ull);
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return gw_min_u32((uint32_t)z, 0xfffffffeu);
}
__device__ __forceinline__ uint64_t gw_policy_env_term(uint64_t env0, uint32_t e)     // env env0 + e's term of the stream
{
    return (env0 + e) * 0x9E3779B97F4A7C15ull;
}
// #{ j in [0, A) : row[j] <= u } for a non-decreasing row: the upper bound by halving.  Every index read lies in [0, A),
// whatever the row holds.  gw_policy_count: the draw's action, that count clamped to A - 1.
template <class ROW>
__device__ __forceinline__ uint32_t gw_policy_upper(ROW row, uint32_t A, uint32_t u)
{
    uint32_t lo = 0, n = A;
    while (n != 0u) {
        const uint32_t half = n >> 1;
        const bool le = row[lo + half] <= u;
        lo = le ? lo + half + 1u : lo;
        n = le ? n - half - 1u : half;
    }
    return lo;
}
template <class ROW>
__device__ __forceinline__ uint32_t gw_policy_count(ROW row, uint32_t A, uint32_t u)
{
    return gw_min_u32(gw_policy_upper(row, A, u), A - 1u);
}
__device__ __forceinline__ uint32_t gw_policy_cls(int32_t obs, int32_t center)        // sign(obs - center) + 1
{
    return (uint32_t)((int)(obs > center) - (int)(obs < center) + 1);
}

constexpr int GW_POLICY_A_MAX = GW_MAX_DEVICES * 20;     // flat actions the fused form stages (3 rows of them in LDS)
constexpr size_t GW_LDS_PER_BLOCK = 65536;               // what one workgroup may allocate, static and dynamic together

// What gw_rollout_policy and its descendants pass on to the kernels below besides the outputs.
struct GwPolicyArgs {
    const uint32_t* cdf;          // [3][A], A = D * max_duration
    const int32_t* obs_prev;      // [N] what each env's agent saw last
    uint64_t seed, step0, env0;
};

// The closed loop's draw, once for every kernel that has it: the table's LDS copy, the env's stream, the action being taken.
// A source derives from it and adds what is its own (output pointers, the histogram, the episode's book, the population's row);
// what a kernel does not use of it (bin_cur without a histogram, latest_next without episodes) the compiler drops.
struct PolicyDraw {
    const uint32_t* __restrict__ cdf;                    // [3][A]
    uint64_t seed, step0, env0;
    uint32_t* s_cdf;                                     // the table in LDS (the launch's dynamic part: 3 * A words)
    uint32_t A, md, inv20;                               // inv20 = ceil(2^20 / md): a / md == (a * inv20) >> 20 for a < A <= 640
    uint64_t env_term;
    uint32_t bin_cur;                                    // cls * A + a of the action being taken
    int d_cur, du_cur;
    int32_t latest_next;                                 // what the env acts on next, minus counter_bound
    // The fields every kernel sets from its arguments; D: the kernel's sender count (DT, or c.D where DT == 0).  In two parts,
    // because a kernel that computes something of its own from A (where the table lies behind a histogram, which policy's
    // slice a block stages) did so between them, and with inv20's division in front of that its instructions change order.
    __device__ __forceinline__ void init(const GwPolicyArgs& p, const GwDevConst& c, int D)
    {
        cdf = p.cdf; seed = p.seed; step0 = p.step0; env0 = p.env0;
        md = (uint32_t)c.max_duration;
        A = (uint32_t)D * md;
        env_term = 0; bin_cur = 0; d_cur = 0; du_cur = 0; latest_next = 0;
    }
    __device__ __forceinline__ void table_at(uint32_t* lds_cdf)
    {
        s_cdf = lds_cdf;
        inv20 = ((1u << 20) + md - 1u) / md;
    }
    __device__ __forceinline__ void stage_cdf() const
    {
        for (uint32_t i = threadIdx.x; i < 3u * A; i += blockDim.x) s_cdf[i] = cdf[i];
    }
    __device__ __forceinline__ void draw(uint32_t cls, uint64_t step)
    {
        const uint32_t a = gw_policy_count(s_cdf + cls * A, A, gw_policy_u(seed, env_term, step));
        // exact: inv20 * md = 2^20 + r with 0 <= r < md, and a * r < 640 * 320 < 2^20 (md <= A / 2: at least two senders)
        const uint32_t dv = (a * inv20) >> 20;
        bin_cur = cls * A + a;
        d_cur = (int)dv;
        du_cur = (int)(a - dv * md);
    }
    __device__ __forceinline__ void first(uint32_t e, int32_t obs_seen, int32_t center)
    {
        env_term = gw_policy_env_term(env0, e);          // the stream is the env's, whichever policy it runs
        latest_next = obs_seen - center;
        draw(gw_policy_cls(obs_seen, center), step0);
    }
    // step k is over and the env now sees `latest` (minus counter_bound; 0 behind a reset): the next action is drawn from that
    __device__ __forceinline__ void next(int k, int K, int32_t latest)
    {
        latest_next = latest;
        if (k + 1 < K) draw((uint32_t)((int)(latest_next > 0) - (int)(latest_next < 0) + 1), step0 + (uint64_t)(k + 1));
    }
};

// The two ways a step gets its action, as the body's hooks (ct_rollout_sync_body.h).  Staged: the caller's [K][N] rows
// `device` / `duration`, step k + 1's action requested while step k is walked; such an action may lie outside the action space
// (GW_FLAG_BADACT).  Drawn: `src`, a PolicyDraw; inside the action space by construction.
#define GW_ROLLOUT_STAGED_FIRST int d_next = device[e], du_next = duration[e];
#define GW_ROLLOUT_STAGED_TAKE                                                                                                   \
    const int d = d_next, du = du_next;                                                                                          \
    if (k + 1 < K) { d_next = device[(size_t)(k + 1) * N + e]; du_next = duration[(size_t)(k + 1) * N + e]; }
#define GW_ROLLOUT_STAGED_CHECKED(bad) (bad)
#define GW_ROLLOUT_DRAWN_TAKE const int d = src.d_cur, du = src.du_cur;
#define GW_ROLLOUT_DRAWN_CHECKED(bad) false

// step k's three outputs as the C-ABI lays them out: GW_ROLLOUT_SRC_STEPPED's first part in a kernel with obs, reward and done arrays
#define GW_ROLLOUT_STORE_OUTPUTS(at, latest, r, dn)                                                                              \
    obs[at] = latest + c.counter_bound;                                                                                          \
    reward[at] = (float)r;                                                                                                       \
    done[at] = (uint8_t)dn;

// Of the tally (ct_rollout_stats.hip: the histogram's layout and bit budget) what more than one file needs: its step limit and a
// bin's size, which decide a launch's availability and dynamic LDS below, and the two primitives the episodes' tally uses too.
constexpr uint32_t TS_STEPS = GW_TS_STEPS;
constexpr uint32_t TS_BIN_BYTES = 16;
__device__ __forceinline__ void gw_ts_add(int64_t* cell, uint64_t v)      // a 64-bit global atomic add, nothing returned
{
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The block is one wave: its LDS adds and a flush's reads are operations of the same wave, kept in order by the hardware; the
// fences keep the compiler from moving them, and no block barrier is needed (or possible: lanes beyond N have left).
__device__ __forceinline__ void gw_wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- episodes inside the closed loop: gw_rollout_episodes / gw_rollout_episodes_stats (include/gymwipe_amd.h) --------------
// What both calls pass on besides their parents' arguments: the caller's gw_episodes, and where the observation each env acts
// on next goes.  obs_prev and obs_next may be one array (an env reads its element before the step loop and writes it after).
struct GwEpisodeArgs {
    int32_t max_steps, on_done;
    int32_t* state;               // [N][2] {age, ret}
    int64_t* tally;               // [GW_EP_COLS], or nullptr
    int32_t* obs_next;            // [N]
};

// One env's episode bookkeeping over a launch: {age, ret} in registers, the episodes it ended summed per lane (a launch is at
// most 64 steps, so the two counts fit 32 bits; lengths and returns are sums of int32 values).
struct EpisodeBook {
    int32_t max_steps, on_done;
    int32_t age, ret;
    uint32_t n, n_done;
    int64_t len_sum, ret_sum, ret_sq;
    __device__ __forceinline__ void load(const GwEpisodeArgs& a, uint32_t e)
    {
        max_steps = a.max_steps; on_done = a.on_done;
        const int2 s = *reinterpret_cast<const int2*>(a.state + 2 * (size_t)e);
        age = s.x; ret = s.y;
        n = 0; n_done = 0; len_sum = 0; ret_sum = 0; ret_sq = 0;
    }
    // a step returned (r, dn): 0 the episode goes on, 1 it ended by done, 2 by the step limit (done wins)
    __device__ __forceinline__ uint32_t stepped(int32_t r, uint32_t dn)
    {
        age += 1; ret += r;
        const uint32_t cause = (on_done != 0 && dn != 0u) ? 1u : ((max_steps > 0 && age >= max_steps) ? 2u : 0u);
        if (cause) {
            n += 1u; n_done += cause == 1u ? 1u : 0u;
            len_sum += age; ret_sum += ret; ret_sq += (int64_t)ret * (int64_t)ret;
            age = 0; ret = 0;
        }
        return cause;
    }
    // {age, ret} back, and the lane's episodes into the block's tally in LDS
    __device__ __forceinline__ void store(const GwEpisodeArgs& a, uint32_t e, unsigned long long* s_ep) const
    {
        *reinterpret_cast<int2*>(a.state + 2 * (size_t)e) = make_int2(age, ret);
        if (!a.tally || !n) return;
        const unsigned long long v[GW_EP_COLS] = {n, n_done, (unsigned long long)len_sum, (unsigned long long)ret_sum,
                                                  (unsigned long long)ret_sq};
#pragma unroll
        for (int j = 0; j < GW_EP_COLS; ++j)
            if (v[j]) __hip_atomic_fetch_add(s_ep + j, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
__device__ __forceinline__ void gw_ep_zero(unsigned long long* s_ep)       // the block's tally, before the block's barrier
{
    if (threadIdx.x < (uint32_t)GW_EP_COLS) s_ep[threadIdx.x] = 0ull;
}
// the block's tally into the caller's: GW_EP_COLS global adds per block at most (behind gw_wave_lds_order)
__device__ __forceinline__ void gw_ep_flush(const unsigned long long* s_ep, uint32_t first, uint32_t stride, int64_t* tally)
{
    if (!tally) return;
    for (uint32_t j = first; j < (uint32_t)GW_EP_COLS; j += stride)
        if (s_ep[j]) gw_ts_add(tally + j, s_ep[j]);
}

// What an episodic kernel does with an env behind the body, GW_ROLLOUT_EP_TAIL(own_row, row): the `ip` record of an env that may
// have been reset in the launch (the body's bpc / bpp), the observation it acts on next, its book, the block's tally.
// OWN_ROW (ct_rollout_pop_ep): the block's episodes go into `row`, which always exists, and into ea.tally as well where there
// is one.  A template flag: tested at run time, all 30 instantiations of ct_rollout_pop_ep came out different.
template <bool OWN_ROW>
__device__ __forceinline__ void gw_ep_tail(const GwEpisodeArgs& ea, const EpisodeBook& ep, int32_t obs_next, uint32_t e, uint32_t N,
                                           unsigned long long* s_ep, int64_t* row)
{
    ea.obs_next[e] = obs_next;
    GwEpisodeArgs own = ea;                              // (the book adds into LDS whenever there is a tally)
    if constexpr (OWN_ROW) own.tally = row;
    ep.store(own, e, s_ep);
    // the wave's lanes that have an env (all 64 but in the last block) share the words out among themselves
    const uint32_t lanes = gw_min_u32(64u, N - blockIdx.x * 64u);
    gw_wave_lds_order();
    if constexpr (OWN_ROW) gw_ep_flush(s_ep, threadIdx.x, lanes, row);
    gw_ep_flush(s_ep, threadIdx.x, lanes, ea.tally);
}
#define GW_ROLLOUT_EP_TAIL(own_row, row)                                                                                         \
    st_plain(st.ip, o16, make_uint4(bpc.t0, bpc.c0, bpp.t0, bpp.c0));                                                            \
    gw_ep_tail<own_row>(ea, src.ep, src.latest_next + c.counter_bound, e, N, s_ep_tally, row);
// The head of an episodic kernel's GW_ROLLOUT_SRC_STEPPED: the book takes the step, and an env whose episode ended is reset in
// registers (the body's reset_env).  Defines cause_next: 0, or why the episode ended.
#define GW_ROLLOUT_EP_STEPPED(r, dn)                                                                                             \
    const uint32_t cause_next = src.ep.stepped(r, dn);                                                                           \
    if (cause_next) reset_env();

// ct_rollout_sync_ep's source (ct_rollout_autoreset.hip): the staged hooks above with the episode's book.
struct StagedEpisodes {
    uint8_t* ended;
    int32_t latest_next;                                 // what the env acts on next, minus counter_bound
    EpisodeBook ep;
};

// ---- episodes scored by what they delivered: gw_rollout_episodes_scored / gw_rollout_population_scored ------------------------
// score_k = w_reward * reward_k + w_delivered[d_k] * delivered_k (include/gymwipe_amd.h).  delivered_k is the step's share of
// the body's running kt.deliv, which restarts at 0 in every launch -- and the baseline with it (first()).  The D weights lie
// behind the policy table's copy in the launch's dynamic LDS: one LDS read per step, indexed by the sender the step assigned.
struct StepScore {
    int32_t* s_w;                                        // [D] in LDS
    int32_t w_reward;
    uint32_t deliv_next;                                 // kt.deliv when the step that is being walked began
    __device__ __forceinline__ void weights_at(uint32_t* lds_w, const gw_score& w)
    {
        s_w = reinterpret_cast<int32_t*>(lds_w);
        w_reward = w.w_reward;
    }
    __device__ __forceinline__ void stage(const gw_score& w, int D) const
    {
        for (int i = threadIdx.x; i < D; i += blockDim.x) s_w[i] = w.w_delivered[i];
    }
    __device__ __forceinline__ void first() { deliv_next = 0u; }
    // the packets step k delivered, given the running count behind it
    __device__ __forceinline__ uint32_t delivered(uint32_t deliv_now)
    {
        const uint32_t dl = deliv_now - deliv_next;
        deliv_next = deliv_now;
        return dl;
    }
    __device__ __forceinline__ int32_t of(int32_t r, int d, uint32_t dl) const { return w_reward * r + s_w[d] * (int32_t)dl; }
    // ... for a sender the caller staged, which may lie outside [0, D): the index is clamped, and a rejected step has r == 0 and
    // dl == 0 (the env was left alone), so whichever weight is read its score is exactly 0
    __device__ __forceinline__ int32_t of_staged(int32_t r, int d, uint32_t dl, int D) const
    {
        return w_reward * r + s_w[gw_min_u32((uint32_t)d, (uint32_t)D - 1u)] * (int32_t)dl;
    }
};

// ct_rollout_sync_eps' source (ct_rollout_autoreset.hip), which ct_rollout_backlog.hip's BacklogEpisodes derives from.
struct ScoredStagedEpisodes : StagedEpisodes {
    StepScore sc;
    int32_t* delivered_out;
    int d_cur;                                           // the sender step k was staged with, inside the action space or not
};

// The sources of ct_rollout_policy.hip's and ct_rollout_pop.hip's episodic kernels, which ct_rollout_fsc.hip's derive from.
// ct_rollout_policy's source with the episode's book (obs_prev may be obs_next here): the draw after a step that ended an
// episode is for the reset's observation, counter_bound (class 1).
struct EpisodeActions : PolicyDraw {
    int32_t* device_out;
    int32_t* duration_out;
    uint8_t* ended;
    EpisodeBook ep;
    __device__ __forceinline__ void stepped(size_t at, int k, int K, int32_t latest, uint32_t cause)
    {
        device_out[at] = d_cur;
        duration_out[at] = du_cur;
        ended[at] = (uint8_t)cause;
        next(k, K, cause ? 0 : latest);
    }
};

// ct_rollout_policy_eps' source
struct ScoredEpisodeActions : EpisodeActions {
    StepScore sc;
    int32_t* delivered_out;
};

// ct_rollout_pop_ep's source (ct_rollout_pop.hip says what a block's row is)
struct PopulationActions : PolicyDraw {
    int64_t* row;                                        // the block's policy: [GW_EP_COLS] of the caller's [P][GW_EP_COLS]
    EpisodeBook ep;
};

// ct_rollout_pop_eps' source
struct ScoredPopulationActions : PopulationActions {
    StepScore sc;
};

// ---- launching the step-synchronous family (host side) -------------------------------------------------------------------------
// What a family keeps in the launch's dynamic LDS decides its availability rules beyond the handle's, and that LDS's size.
enum GwFusedLds {
    GW_FUSED_NO_TABLE,            // staged actions: nothing
    GW_FUSED_TABLE,               // the policy table's copy: 3 * A words, for A <= GW_POLICY_A_MAX
    GW_FUSED_TABLE_SCORE,         // ... and the score's D weights behind it (checked against the block's LDS as the next one is)
    GW_FUSED_TABLE_HIST           // ... behind a histogram of 3 * A bins: at most TS_STEPS steps, where both fit beside the
};                                //     kernel's own tables (decided by the handle alone, never by K)

// No fused launch of K steps on this handle: more steps than its capacity, a handle created for the event-loop form, an action
// space larger than the table's LDS copy, more steps than the histogram's bit budget.  The caller goes on step by step.
inline bool fused_unavailable(const GwState& st, const GwDevConst& cst, int K, GwFusedLds lds)
{
    if (K <= 0 || K > st.rcap || st.ract != nullptr) return true;
    if (lds != GW_FUSED_NO_TABLE && (int64_t)st.D * cst.max_duration > GW_POLICY_A_MAX) return true;
    return lds == GW_FUSED_TABLE_HIST && K > (int)TS_STEPS;
}

// One launch of kernel_of(dt, m) -- the family's instantiation for the handle's sender count and the launch's MODE -- over a
// grid of 64-lane blocks, recorded in the family's slots from slot_base on.  The kernel's arguments are st, cst, K, args...
// launch_fused_lds: with `dyn` bytes of dynamic LDS, for a family that sizes them itself (ct_rollout_fsc.hip; `fits`: refuse the
// launch, before it, where they do not fit the block's LDS beside the instantiation's own).  launch_fused, behind it: sized by
// what the family keeps there (GwFusedLds).
template <class KERNEL_OF, class... ARGS>
int launch_fused_lds(const GwState& st, const GwDevConst& cst, const GwChunk& ch, int slot_base, bool fits, size_t dyn,
                     KERNEL_OF kernel_of, const ARGS&... args)
{
    const unsigned grid = (unsigned)((st.N + 63) / 64);
    const int mode = gw_step_mode(cst, ch.below_limits, false);
    return gw_with_dt<GW_DTS_ROLLOUT_SYNC>(st.D, [&](auto dt) {          // (any other D: per-lane arrays in LDS)
        return gw_with_mode(mode, [&](auto m) {
            constexpr int DT = decltype(dt)::value, MODE = decltype(m)::value;
            const auto kernel = kernel_of(dt, m);
            if (fits) {
                // The instantiation's own LDS, asked once (the same on every device).  One static per kernel: this generic
                // lambda is instantiated per (KERNEL_OF, dt, m), and every GW_KERNEL_OF lambda is a type of its own, so
                // ct_rollout_pstats and ct_rollout_pstats_ep do not share theirs.
                static const int fixed = [&] {
                    hipFuncAttributes fa;
                    return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess ? (int)fa.sharedSizeBytes : -1;
                }();
                if (fixed < 0) return gw_launch_status(hipErrorInvalidDeviceFunction);
                if ((size_t)fixed + dyn > GW_LDS_PER_BLOCK) return (int)GW_EUNSUPPORTED;
            }
            gw_note_launch(ch.rec, slot_base + 3 * gw_ls_dt(DT) + MODE);
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), dyn, (hipStream_t)ch.stream, st, cst, ch.K, args...);
            return gw_launch_status();
        });
    });
}
template <class KERNEL_OF, class... ARGS>
int launch_fused(const GwState& st, const GwDevConst& cst, const GwChunk& ch, int slot_base, GwFusedLds lds, KERNEL_OF kernel_of,
                 const ARGS&... args)
{
    const size_t A = (size_t)st.D * (size_t)cst.max_duration;
    const size_t dyn = lds == GW_FUSED_NO_TABLE ? 0 : 3 * A * (sizeof(uint32_t) + (lds == GW_FUSED_TABLE_HIST ? TS_BIN_BYTES : 0)) +
                                                      (lds == GW_FUSED_TABLE_SCORE ? (size_t)st.D * sizeof(int32_t) : 0);
    return launch_fused_lds(st, cst, ch, slot_base, lds == GW_FUSED_TABLE_HIST || lds == GW_FUSED_TABLE_SCORE, dyn, kernel_of, args...);
}
#define GW_KERNEL_OF(family) [](auto dt, auto m) { return &family<decltype(dt)::value, decltype(m)::value>; }

inline GwPolicyArgs policy_args(const GwPolicyStream& pol, const int32_t* obs_prev)
{
    return {pol.cdf, obs_prev, pol.seed, pol.step0, pol.env_id0};
}
inline GwEpisodeArgs episode_args(const gw_episodes& ep, int32_t* obs_next)
{
    return {ep.max_steps, ep.on_done, ep.state_dev, ep.tally_dev, obs_next};
}

} // namespace
