// ct_rollout_sfx.hip -- gw_rollout(): K consecutive env.step() calls from pre-staged actions in ONE
// persistent launch, for the default (suffix) state layout.
//
// Two forms live here: the step-synchronous kernel (ct_rollout_sync_kernel: what gw_rollout launches since round 3, see its
// comment) and the event loop it replaced (ct_rollout_sfx_kernel with the packing / expanding kernels: GW_ROLLOUT_EVENT_LOOP=1,
// the A/B reference, kept under test), whose rationale follows.
// Why a second kernel: with one launch per step every wave lasts as long as its slowest env (0..9
// data transmissions per step, 1.6 on average), so ~80% of the lane-iterations of the window loop are
// idle.  Here a lane is not tied to the step boundary of its neighbours: the loop body is ONE
// TRANSMISSION (the announcement of a step or a data packet, same arithmetic), and a lane that
// finishes a step immediately starts its next one.  Over K steps the per-lane work evens out, the env
// state stays in registers, and the only per-step memory traffic is 2 bytes of action in and 1 byte of
// feedback out:
//     pack kernel    actions int32[K][N] x2  ->  u16[N][K]  (device | duration << 8)
//     rollout kernel state <-> registers once; feedback u8[N][K] = (diff+1) | (reward+10) << 2 | done << 7
//     expand kernel  u8[N][K] -> obs int32[K][N], reward f32[K][N], done u8[K][N]
// Results are bit-identical to K calls of the step kernel (tests compare both with the oracle).
// The step semantics and reference citations are those of ct_step_sfx.hip / ct_common.hip.h.
#include "ct_common.hip.h"
#include "gw_dispatch.h"
#include "gw_queue.h"

using namespace gwk;

namespace {

// (ld, st_plain, word_of: ct_common.hip.h)

// The rollout kernel wants each env's actions and feedback contiguous ([N][Kp]: one 16-byte load = 8 steps of
// actions, one dword store = 4 steps of feedback); the C-ABI takes and returns step-major arrays ([K][N]).  Both
// transposes go through an LDS tile of 64 envs x 64 steps so that every global access is a coalesced 16-byte
// (or, for `done`, 4-byte) access.  Pure streaming kernels, ~42 MB per 64 steps x 65 536 envs each.
constexpr int TP_ENVS = 64, TP_STEPS = 64;

// actions [K][N] int32 x 2  ->  [N][Kp] u16 (device | duration << 8; 0xffff = invalid or beyond K)
__global__ __launch_bounds__(256) void pack_actions_kernel(uint32_t N, int K, int Kp, const int32_t* __restrict__ device,
                                                           const int32_t* __restrict__ duration, uint16_t* __restrict__ packed)
{
    __shared__ __attribute__((aligned(16))) uint16_t tile[TP_ENVS][TP_STEPS + 2];                  // +2: rows start on different banks
    const uint32_t e0 = blockIdx.x * TP_ENVS;
    const int t = threadIdx.x;
    const bool vec_ok = (N & 3u) == 0;                                // rows of [K][N] stay 16-byte aligned
    for (int k0 = 0; k0 < Kp; k0 += TP_STEPS) {
        // load: thread -> (row r of 16, 4 consecutive envs)
        const int c4 = (t & 15) * 4, r = t >> 4;
#pragma unroll
        for (int pass = 0; pass < TP_STEPS / 16; ++pass) {
            const int kk = pass * 16 + r, k = k0 + kk;
            uint32_t v[4] = {0xffffu, 0xffffu, 0xffffu, 0xffffu};
            if (k < K) {
                int32_t dv[4], du[4];
                const uint32_t e = e0 + (uint32_t)c4;
                if (vec_ok && e + 3 < N) {
                    const int4 a = *reinterpret_cast<const int4*>(device + (size_t)k * N + e);
                    const int4 b = *reinterpret_cast<const int4*>(duration + (size_t)k * N + e);
                    dv[0] = a.x; dv[1] = a.y; dv[2] = a.z; dv[3] = a.w;
                    du[0] = b.x; du[1] = b.y; du[2] = b.z; du[3] = b.w;
                } else {
                    for (int j = 0; j < 4; ++j) {
                        const bool in = e + j < N;
                        dv[j] = in ? device[(size_t)k * N + e + j] : -1;
                        du[j] = in ? duration[(size_t)k * N + e + j] : -1;
                    }
                }
                // anything outside a byte is invalid for every configuration (D <= 32, max_duration checked by the caller)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = ((uint32_t)dv[j] > 0xfeu || (uint32_t)du[j] > 0xfeu) ? 0xffffu : ((uint32_t)dv[j] | ((uint32_t)du[j] << 8));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[c4 + j][kk] = (uint16_t)v[j];
        }
        __syncthreads();
        // store: thread -> (env row, 8 consecutive steps = 16 bytes); 8 threads cover one env's 64 steps
        const int cols = (Kp - k0) < TP_STEPS ? (Kp - k0) : TP_STEPS;   // multiple of 16
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int env = pass * 32 + (t >> 3), s0 = (t & 7) * 8;
            if (e0 + env < N && s0 < cols) {
                uint32_t w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = (uint32_t)tile[env][s0 + 2 * j] | ((uint32_t)tile[env][s0 + 2 * j + 1] << 16);
                *reinterpret_cast<uint4*>(packed + (size_t)(e0 + env) * Kp + k0 + s0) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();
    }
}

// feedback u8[N][Kp] -> obs/reward/done [K][N]
__global__ __launch_bounds__(256) void expand_feedback_kernel(uint32_t N, int K, int Kp, int center, int pv, const uint8_t* __restrict__ fb,
                                                              int32_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[TP_ENVS][TP_STEPS + 4];                   // rows 68 bytes apart: 4-byte aligned, banks spread
    const uint32_t e0 = blockIdx.x * TP_ENVS;
    const int t = threadIdx.x;
    const bool vec_ok = (N & 3u) == 0;
    for (int k0 = 0; k0 < Kp; k0 += TP_STEPS) {
        const int cols = (Kp - k0) < TP_STEPS ? (Kp - k0) : TP_STEPS;   // multiple of 16
        {   // load: thread -> (env row, 16 consecutive steps = 16 bytes); 4 threads cover one env's 64 steps
            const int env = t >> 2, s0 = (t & 3) * 16;
            if (e0 + env < N && s0 < cols) {
                const uint4 w = *reinterpret_cast<const uint4*>(fb + (size_t)(e0 + env) * Kp + k0 + s0);
                uint32_t* row = reinterpret_cast<uint32_t*>(&tile[env][s0]);
                row[0] = w.x; row[1] = w.y; row[2] = w.z; row[3] = w.w;
            }
        }
        __syncthreads();
        // store: thread -> (step row r of 16, 4 consecutive envs)
        const int c4 = (t & 15) * 4, r = t >> 4;
#pragma unroll
        for (int pass = 0; pass < TP_STEPS / 16; ++pass) {
            const int kk = pass * 16 + r, k = k0 + kk;
            const uint32_t e = e0 + (uint32_t)c4;
            if (k < K && e < N) {
                int32_t o[4]; float rw[4]; uint8_t dn[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t b = tile[c4 + j][kk];
                    o[j] = center + pv * ((int)(b & 3u) - 1);
                    rw[j] = (float)((int)((b >> 2) & 31u) - 10);
                    dn[j] = (uint8_t)(b >> 7);
                }
                if (vec_ok && e + 3 < N) {
                    *reinterpret_cast<int4*>(obs + (size_t)k * N + e) = make_int4(o[0], o[1], o[2], o[3]);
                    *reinterpret_cast<float4*>(reward + (size_t)k * N + e) = make_float4(rw[0], rw[1], rw[2], rw[3]);
                    *reinterpret_cast<uchar4*>(done + (size_t)k * N + e) = make_uchar4(dn[0], dn[1], dn[2], dn[3]);
                } else {
                    for (int j = 0; j < 4 && e + j < N; ++j) {
                        obs[(size_t)k * N + e + j] = o[j]; reward[(size_t)k * N + e + j] = rw[j]; done[(size_t)k * N + e + j] = dn[j];
                    }
                }
            }
        }
        __syncthreads();
    }
}

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

// MODE as in ct_step_sfx.hip: 0 run-time flags, 1 every fast form validated (FAST), 2 FAST and no env can reach the fast
// forms' validity limits during this launch (host-side bound on the simulated time over all K steps).
template <int DT, int MODE>
__global__ __launch_bounds__(256) void ct_rollout_sfx_kernel(GwState st, GwDevConst c, int K, int Kp,
                                                            const uint16_t* __restrict__ actions,
                                                            uint8_t* __restrict__ feedback)
{
    constexpr bool GEN = DT == 0;                        // any sender count: per-lane arrays in LDS, launched with 64 threads
    constexpr int DM = GEN ? GW_MAX_DEVICES : DT;        // capacity
    constexpr int NWC = (2 * DM + 1 + 15) / 16;
    constexpr int S = GW_MAX_NSTATES;
    const int D = GEN ? c.D : DT, R = D + 1, RRM = D;
    const uint32_t N = (uint32_t)st.N;
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;

    // ---- lookup tables -> LDS ----------------------------------------------------------------------
    constexpr int TRANS_B = ((DM + 1) * (DM + 1) * S + 15) / 16 * 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_trans[TRANS_B];
    __shared__ __attribute__((aligned(16))) double  s_ber[2 * DM * S];
    __shared__ __attribute__((aligned(16))) uint8_t s_cls[2 * DM * S];
    __shared__ uint32_t s_cols[GEN ? (3 * DM + 1) * 64 : 1];     // GEN: len[D], tb[D], sta[R] columns per lane
    __shared__ uint2 s_mi[GEN ? DM : 1];                 // GEN: {mult, ceil(65536/mult)} and terminal-state masks, indexed by
    __shared__ uint32_t s_term[GEN ? DM : 1];            //      the lane's own addressed sender
    if constexpr (GEN) {
        for (int i = threadIdx.x; i < D; i += blockDim.x) {
            s_mi[i] = make_uint2((uint32_t)st.cst->mult[i], st.cst->inv16[i]);
            s_term[i] = st.cst->term[i];
        }
    }
    {
        const int n_tr = (R * R * S + 15) >> 4, n_be = (2 * D * S * 8) >> 4, n_cl = (2 * D * S) >> 4;
        for (int i = threadIdx.x; i < n_tr; i += blockDim.x) *reinterpret_cast<uint4*>(s_trans + ((uint32_t)i << 4)) = ld<uint4>(st.trans, (uint32_t)i << 4);
        for (int i = threadIdx.x; i < n_be; i += blockDim.x) *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(s_ber) + ((uint32_t)i << 4)) = ld<uint4>(st.ber2, (uint32_t)i << 4);
        for (int i = threadIdx.x; i < n_cl; i += blockDim.x) *reinterpret_cast<uint4*>(s_cls + ((uint32_t)i << 4)) = ld<uint4>(st.cls2, (uint32_t)i << 4);
    }
    __syncthreads();
    if (e >= N) return;

    // ---- state -> registers --------------------------------------------------------------------------
    const uint32_t RB = GEN ? (uint32_t)st.RB : 16u * NWC;
    const uint32_t o16 = e << 4, oq = e * RB;
    const uint4 ip = ld<uint4>(st.ip, o16);
    const double2 tw = ld<double2>(st.tw, o16);
    const uint4 tk = ld<uint4>(st.tk, o16);
    typename ArrSel<GEN, DM>::rw len, tb;
    typename ArrSel<GEN, DM + 1>::rw sta;
    if constexpr (GEN) {
        uint32_t* col = s_cols + (threadIdx.x & 63);
        len.p = col; tb.p = col + DM * 64; sta.p = col + 2 * DM * 64;
        for (int i = 0; i < D; ++i) len[i] = st.qb[oq + (uint32_t)i];
        for (int j = 0; j < R; ++j) sta[j] = st.qb[oq + (uint32_t)(D + j)];
    } else {
        uint4 qw[NWC];
#pragma unroll
        for (int w = 0; w < NWC; ++w) qw[w] = ld<uint4>(st.qb, oq + 16u * w);
#pragma unroll
        for (int i = 0; i < DT; ++i) len[i] = (word_of(qw[i >> 4], (i >> 2) & 3) >> ((i & 3) * 8)) & 0xffu;
#pragma unroll
        for (int j = 0; j < DT + 1; ++j) sta[j] = (word_of(qw[(DT + j) >> 4], ((DT + j) >> 2) & 3) >> (((DT + j) & 3) * 8)) & 0xffu;
    }
    double now = tw.x, wake = tw.y;
    uint32_t tau = tk.x;
    const uint32_t nbp = tk.y;
    GwBp bpc, bpp;
    bpc.t0 = ip.x; bpc.c0 = ip.y;                // (record layout: ct_step_sfx.hip)
    bpp.t0 = ip.z; bpp.c0 = ip.w;
    const GwBp* hist = st.bph + ((size_t)e << 7);
    uint32_t rvm = tk.z;
    int32_t last_abs = (int32_t)(tk.w & 0x7fffffffu);
    uint32_t dn = tk.w >> 31;

    constexpr bool FAST = MODE >= 1, NOLIM = MODE == 2;
    const StepMathT<FAST, NOLIM> m(c);
    const double slot = c.slot, br = c.bit_rate, hd = c.hdr_dur, hdr_bits = c.hdr_bits, interval = c.counter_interval;
    const double inv_interval = c.inv_interval, tie_filter = c.tie_filter;
    const bool fast_ticks = FAST || c.fast_ticks != 0;
    const uint32_t bound = (uint32_t)c.counter_bound, base_bytes = (uint32_t)(c.mac_hdr + c.net_hdr);
    const int mh = c.mac_hdr, pv = c.payload_value;
    uint32_t live_mask = 0u;                             // any-D kernel: bit i = sender i is in a non-terminal noise state
    if constexpr (GEN) {
        for (int i = 0; i < D; ++i) live_mask |= ((s_term[i] >> sta[i]) & 1u) ? 0u : (1u << i);
    }
    typename ArrSel<GEN, DM>::ro mult, term, inv16;
    if constexpr (GEN) {
        mult.p = st.cst->mult; mult.shift16 = 0; term.p = st.cst->term; term.shift16 = 1; inv16.p = st.cst->inv16; inv16.shift16 = 0;
    } else {
#pragma unroll
        for (int i = 0; i < DT; ++i) { mult.v[i] = (uint32_t)c.mult[i]; term.v[i] = c.term[i]; inv16.v[i] = c.inv16[i]; }
    }

    Tally kt = {0, 0, 0, 0, 0};
    uint32_t k_bad = 0, fl = 0;

    // ---- per-step variables of the lane's current step -------------------------------------------------
    // Laziness that keeps the loop body small (all exact):
    //   * queue lengths: len[i] is valid as of tick tb[i]; a sender is brought up to date when it is
    //     addressed (and everyone once at the end): k ticks are min(len + k*mult, 100) in one go;
    //   * counter ticks between the end of a window and the end of the step are not counted at the
    //     step end but by the next step's first count (tick counting is cumulative in time).
    int k = 0;                      // step index
    bool data_mode = false;         // false: the next transmission is the announcement of step k
    bool finish = false;            // the current step is over: close it at the top of the next iteration
    int d = 0;                      // addressed sender of the current step
    uint32_t len_d = 0, mult_d = 0, inv16_d = 65536u;
#pragma unroll
    for (int i = 0; i < D; ++i) tb[i] = tau;
    uint32_t n_data = 0, s_r_run = 0;
    double cur = now, stopw = 0.0, t_end = 0.0;
    bool cls_valid = false;
    uint32_t fbw = 0;               // feedback bytes of up to 4 steps, flushed as one dword

    const uint16_t* act = actions + (size_t)e * Kp;
    uint8_t* fbp = feedback + (size_t)e * Kp;
    uint4 aw = ld<uint4>(act, 0);   // actions of steps 0..7

    auto put_feedback = [&](uint32_t byte) {
        fbw |= byte << ((k & 3) * 8);
        if ((k & 3) == 3 || k == K - 1) { st_plain(fbp, (uint32_t)(k & ~3), fbw); fbw = 0; }
        k++;
        if ((k & 7) == 0 && k < K) aw = ld<uint4>(act, (uint32_t)k * 2u);                // next 8 actions
    };

    // ---- the lane's event loop: at most ONE transmission per iteration, every block appears once ----------
    while (k < K) {
        // (1) data mode: is there a packet that still fits the window?  (simple_stack.py:397-434)
        uint32_t s = 0;
        if (data_mode && !finish) {
            bool have = true;
            if (len_d == 0) {
                if (mult_d != 0u && wake < stopw) {          // mult 0: a silent sender, nothing will ever arrive
                    cur = wake;
                    wake = wake + interval;
                    tau++;
                    len_d = gw_len_after_ticks(0u, 1u, mult_d, kt);
                } else have = false;
            }
            if (have) {
                const uint32_t age = gw_ceil_div(len_d, mult_d, inv16_d);
                s = base_bytes + gw_tick_value(tau - age, bpc, bpp, nbp, hist, bound);
                const double need = m.over_rate((double)(s * 8u));
                if (!((stopw - cur) > need)) have = false;
            }
            if (!have) finish = true;
        }

        // (2) close the step (A.5 + interpreter feedback); the other senders' queues stay lazy
        if (finish) {
            // A.5, lazily: the counter ticks between the end of the window and the end of the step are counted by the
            // next step's first count (counting is cumulative in time).  What must not be lost is the diagnostic bit
            // for a tick falling EXACTLY on t_end.  A tie needs (t_end - wake) / interval within tie_filter of an
            // integer (host-side bound on the accumulated rounding of the running sum, gw_api.cpp); only then is the
            // exact comparison made, by the plain loop.
            {
                const double dd = t_end - wake;
                if (dd >= 0.0) {
                    const double q = dd * inv_interval;
                    if (!(fabs(q - rint(q)) > tie_filter) || !(wake >= 0.0625) || !(wake < 2097152.0)) {
                        for (double w = wake; w <= t_end; w = w + interval)
                            if (w == t_end) fl |= GW_FLAG_TIE;
                    }
                }
            }
            // the listeners' noise states: nothing to look up once every one of them is terminal
            bool all_term = true;
            if constexpr (GEN) {
                // any-D kernel: which senders sit in a non-terminal noise state is kept as a bit mask per lane, so the
                // common case (everyone terminal) costs no pass over the senders
                all_term = (live_mask & ~(1u << d)) == 0u;
                len[d] = len_d; tb[d] = tau;
            } else {
#pragma unroll
                for (int i = 0; i < D; ++i) all_term = all_term && (i == d || ((term[i] >> sta[i]) & 1u));
#pragma unroll
                for (int i = 0; i < D; ++i)
                    if (i == d) { len[i] = len_d; tb[i] = tau; }
            }
            if (!all_term) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    if (i == d) continue;
                    uint32_t si = s_trans[(uint32_t)((i * R + RRM) * S) + sta[i]];      // heard the announcement
                    for (uint32_t n = 0; n < n_data; ++n) {                              // ... and d's data
                        const uint32_t s2 = s_trans[(uint32_t)((i * R + d) * S) + si];
                        if (s2 == si) break;
                        si = s2;
                    }
                    sta[i] = si;
                    if constexpr (GEN) live_mask = ((term[i] >> si) & 1u) ? (live_mask & ~(1u << i)) : (live_mask | (1u << i));
                }
            }
            sta[RRM] = s_r_run;
            const int32_t latest = pv * ((int)(rvm & 1u) - (int)((rvm >> 1) & 1u));
            const int32_t abs_d = latest < 0 ? -latest : latest;
            int32_t r = last_abs - abs_d;
            last_abs = abs_d;
            r = r > 10 ? 10 : (r < -10 ? -10 : r);
            now = t_end;
            finish = false;
            data_mode = false;
            mult_d = 0;                              // no addressed sender between steps
            put_feedback((uint32_t)((int)(rvm & 1u) - (int)((rvm >> 1) & 1u) + 1) | ((uint32_t)(r + 10) << 2) | (dn << 7));
            if (k >= K) break;
        }

        // (3) start of step k (counter_traffic.py:146-158): set up the announcement
        int pay_bytes;
        bool is_data = data_mode;
        if (!data_mode) {
            const uint32_t a = (word_of(aw, (k & 7) >> 1) >> ((k & 1) * 16)) & 0xffffu;
            d = (int)(a & 0xffu);
            const int du = (int)(a >> 8);
            if ((unsigned)d >= (unsigned)D || (unsigned)du >= (unsigned)c.max_duration) {
                fl |= GW_FLAG_BADACT;                // env untouched, feedback repeats the current values
                k_bad++;
                put_feedback((uint32_t)((int)(rvm & 1u) - (int)((rvm >> 1) & 1u) + 1) | (10u << 2) | (dn << 7));
                continue;
            }
            uint32_t l0 = 0, t0 = 0, s_d_old = 0;
            if constexpr (GEN) {
                l0 = len[d]; t0 = tb[d]; s_d_old = sta[d];
                mult_d = s_mi[d].x; inv16_d = s_mi[d].y;
            } else {
#pragma unroll
                for (int i = 0; i < D; ++i)
                    if (i == d) { l0 = len[i]; t0 = tb[i]; mult_d = mult[i]; inv16_d = inv16[i]; s_d_old = sta[i]; }
            }
            len_d = gw_len_after_ticks(l0, tau - t0, mult_d, kt);          // the addressed queue, up to date
            const int slots = du * c.duration_factor;
            pay_bytes = ndigits(slots);
            cur = now;
            cls_valid = NOLIM || now < c.cls_limit;
            const uint32_t s_d = s_trans[(uint32_t)((d * R + RRM) * S) + s_d_old];   // d after hearing the RRM
#pragma unroll
            for (int i = 0; i < (GEN ? 0 : D); ++i) if (i == d) sta[i] = s_d;
            if constexpr (GEN) {
                sta[d] = s_d;
                live_mask = ((s_term[d] >> s_d) & 1u) ? (live_mask & ~(1u << d)) : (live_mask | (1u << d));
            }
            s_r_run = sta[RRM];
            n_data = 0;
            stopw = (double)slots * slot;            // become absolute times once t_r is known
            t_end = (double)(slots + 1) * slot;
        } else {
            len_d--;                                 // simple_stack.py:425
            kt.pop++;
            pay_bytes = (int)s - mh;
        }

        // (4) the transmission: slot alignment, durations, decode at the receiver
        uint32_t cls_x;
        double ber_x;
        if (is_data) {
            s_r_run = s_trans[(uint32_t)((RRM * R + d) * S) + s_r_run];     // the RRM hears sender d (again)
            ber_x = s_ber[(uint32_t)((D + d) * S) + s_r_run];
            cls_x = s_cls[(uint32_t)((D + d) * S) + s_r_run];
        } else {
            uint32_t s_d_now = 0;
#pragma unroll
            for (int i = 0; i < (GEN ? 0 : D); ++i) if (i == d) s_d_now = sta[i];
            if constexpr (GEN) s_d_now = sta[d];
            ber_x = s_ber[(uint32_t)(d * S) + s_d_now];
            cls_x = s_cls[(uint32_t)(d * S) + s_d_now];
        }
        const TxTimes x = tx_times(m, cur, hd, m.over_rate((double)(pay_bytes * 8)));
        kt.tx++;
        const bool ok = decode(m, cls_x, cls_valid, ber_x, x, br, hdr_bits, (double)(pay_bytes * 8) * c.coded_factor, fl);

        // (5) consequences + the counter ticks up to the new current time (one instance of the counting loop)
        bool incl;
        if (is_data) {
            n_data++;
            if (ok) {                                // devices.py:163-168, counter_traffic.py:75-80
                kt.deliv++;
                rvm |= (1u << d);
                if (pv == c.counter_bound) dn = 1u;
            }
            if (!(x.t_e < t_end)) fl |= GW_FLAG_CARRY;
            cur = x.t_e;
            incl = true;                             // ticks are older events than the MAC's resume
            if (!(cur < stopw)) finish = true;       // window timeout already processed
        } else {
            const double t_r = x.t_e;
            stopw = t_r + stopw;                     // simple_stack.py:401
            t_end = t_r + t_end;                     // simple_stack.py:557-558
            cur = t_r;
            incl = false;                            // ties at the window start: the MAC runs first
            data_mode = true;
            if (!ok) finish = true;                  // announcement not decoded: no window
        }
        {
            // the first count of a step also covers the ticks since the previous window closed (up to ~21):
            // one jump (gw_fastmath.h; exact, validated at gw_create) instead of a loop every lane would wait for
            uint32_t kk = 0;
            double wj = wake;
            bool tiej = false;
            if (fast_ticks && gw_tick_jump(wake, cur, interval, inv_interval, incl, &kk, &wj, &tiej)) {
                wake = wj;
                if (tiej) fl |= GW_FLAG_TIE;
            } else {
                kk = 0;
                for (;;) {
                    const double w1 = wake + interval, w2 = w1 + interval, w3 = w2 + interval, w4 = w3 + interval;
                    const bool b0 = incl ? (wake <= cur) : (wake < cur);
                    const bool b1 = incl ? (w1 <= cur) : (w1 < cur);
                    const bool b2 = incl ? (w2 <= cur) : (w2 < cur);
                    const bool b3 = incl ? (w3 <= cur) : (w3 < cur);
                    if (incl && (wake == cur || w1 == cur || w2 == cur || w3 == cur)) fl |= GW_FLAG_TIE;
                    kk += (uint32_t)b0 + (uint32_t)b1 + (uint32_t)b2 + (uint32_t)b3;
                    wake = b3 ? w4 : (b2 ? w3 : (b1 ? w2 : (b0 ? w1 : wake)));
                    if (!b3) break;
                }
            }
            tau += kk;
            len_d = gw_len_after_ticks(len_d, kk, mult_d, kt);
        }
    }

    // ---- catch up: ticks up to the end of the last step, every queue to the final tick ----------------------
    {
        uint32_t kk = 0;
        while (wake <= now) { if (wake == now) fl |= GW_FLAG_TIE; wake = wake + interval; kk++; }
        tau += kk;
#pragma unroll
        for (int i = 0; i < D; ++i) len[i] = gw_len_after_ticks(len[i], tau - tb[i], mult[i], kt);
    }

    // ---- registers -> state --------------------------------------------------------------------------------
    if constexpr (GEN) {
        for (int i = 0; i < D; ++i) st.qb[oq + (uint32_t)i] = (uint8_t)len[i];
        for (int j = 0; j < R; ++j) st.qb[oq + (uint32_t)(D + j)] = (uint8_t)sta[j];
    } else {
        uint32_t nb[16 * NWC];
#pragma unroll
        for (int b = 0; b < 16 * NWC; ++b) nb[b] = 0u;
#pragma unroll
        for (int i = 0; i < DT; ++i) nb[i] = len[i];
#pragma unroll
        for (int j = 0; j < DT + 1; ++j) nb[DT + j] = sta[j];
#pragma unroll
        for (int w = 0; w < NWC; ++w) {
            const int b = 16 * w;
            uint4 o;
            o.x = nb[b + 0] | (nb[b + 1] << 8) | (nb[b + 2] << 16) | (nb[b + 3] << 24);
            o.y = nb[b + 4] | (nb[b + 5] << 8) | (nb[b + 6] << 16) | (nb[b + 7] << 24);
            o.z = nb[b + 8] | (nb[b + 9] << 8) | (nb[b + 10] << 16) | (nb[b + 11] << 24);
            o.w = nb[b + 12] | (nb[b + 13] << 8) | (nb[b + 14] << 16) | (nb[b + 15] << 24);
            st_plain(st.qb, oq + 16u * w, o);
        }
    }
    st_plain(st.tw, o16, make_double2(now, wake));
    st_plain(st.tk, o16, make_uint4(tau, nbp, rvm, (uint32_t)last_abs | (dn << 31)));
    publish_env_counters(st.sa, N, e, kt.pop, kt.deliv, k_bad, fl, (uint32_t)K);
}

// ---- the step-synchronous form (every sender count) --------------------------------------------------------------
// The event loop above was built when a data packet cost as much as an announcement (one pass of a ~140-instruction body
// either way) and letting lanes run ahead of each other evened the work out.  Since the window loop has a straight-line form
// (ct_step_sfx.hip: ~45 instructions per packet, every per-packet decision settled for the step up front), a packet is a third
// of an announcement, and the lock-step of whole steps costs less than the event loop's ~60 exec-mask regions per pass: here
// every lane takes step k together -- announcement, window (straight line, general loop where that declines), feedback -- with
// the env's state in registers across all K steps, queue lengths of the senders not addressed and the ticks behind a window
// lazy exactly as above; DT == 0 = any sender count, the per-lane arrays as LDS columns.  Same results bit for bit (the tests
// run both forms against the oracle; GW_ROLLOUT_EVENT_LOOP=1 selects the event loop).
//
// Where a step's action comes from is the loop's one parameter, so that its body exists once (ct_rollout_sync_body.h):
//   ct_rollout_sync_kernel  gw_rollout: the caller's pre-staged rows, step k + 1's action loaded while step k is walked;
//   ct_rollout_policy       gw_rollout_policy: drawn at the step boundary from a three-row table over the observation the
//                           env just produced (PolicyActions), and stored with that step's outputs.
//   ct_rollout_pstats       gw_rollout_policy_stats: the same draw, nothing stored per step -- the transition is counted into a
//                           table over (observation class, action) instead (StatsActions).
//   ct_rollout_policy_ep    gw_rollout_episodes: ct_rollout_policy with episodes -- an env whose step returned done, or whose
//   ct_rollout_pstats_ep    episode reached its step limit, is reset in registers at the step boundary and draws its next
//                           action from the reset's observation; gw_rollout_episodes_stats: the same with ct_rollout_pstats' tally.
//   ct_rollout_sync_ep      gw_rollout_autoreset: ct_rollout_sync_kernel's staged rows with the same episodes -- the caller's
//                           actions, the launch's resets.
//   ct_rollout_pop_ep       gw_rollout_population: ct_rollout_policy_ep with one table per block and nothing stored per step.
//   ct_rollout_policy_eps   gw_rollout_episodes_scored / gw_rollout_population_scored: the two before with the step's score --
//   ct_rollout_pop_eps      the reward and the packets the step delivered, weighted -- where they have the reward.
//   ct_rollout_sync_eps     gw_rollout_autoreset_scored: ct_rollout_sync_ep with the same score, the sender the caller's.
//   ct_rollout_backlog      gw_rollout_backlog: ct_rollout_sync_eps with the action chosen at the step boundary from the queue
//                           lengths, which the body brings to the current tick there (BacklogEpisodes).
//   ct_rollout_backlog_pop  gw_rollout_backlog_population: ct_rollout_backlog with one policy per block, read from device memory,
//                           and nothing stored per step (as ct_rollout_pop_eps).
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

template <int DT, int MODE>
__global__ __launch_bounds__(64) void ct_rollout_sync_kernel(GwState st, GwDevConst c, int K,
                                                            const int32_t* __restrict__ device, const int32_t* __restrict__ duration,
                                                            int32_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done)
{
#define GW_ROLLOUT_SRC_STAGE
#define GW_ROLLOUT_SRC_FIRST GW_ROLLOUT_STAGED_FIRST
#define GW_ROLLOUT_SRC_TAKE GW_ROLLOUT_STAGED_TAKE
#define GW_ROLLOUT_SRC_CHECKED(bad) GW_ROLLOUT_STAGED_CHECKED(bad)
#define GW_ROLLOUT_SRC_STEPPED(at, latest, r, dn) GW_ROLLOUT_STORE_OUTPUTS(at, latest, r, dn)
#include "ct_rollout_sync_body.h"
}

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
constexpr uint32_t TS_STEPS = GW_TS_STEPS, TS_EVENTS = 64 * TS_STEPS;
constexpr int TS_CNT_BITS = 13, TS_RS_BITS = 17, TS_RQ_BITS = 19;
constexpr int TS_RMAX = 10;
static_assert(TS_EVENTS < (1u << TS_CNT_BITS), "a count field overflows into its neighbour");
static_assert(2 * TS_RMAX * TS_EVENTS < (1u << TS_RS_BITS), "the reward-sum field overflows");
static_assert(TS_RMAX * TS_RMAX * TS_EVENTS < (1u << TS_RQ_BITS), "the reward-square-sum field overflows");
static_assert(4 * TS_CNT_BITS <= 64 && TS_RS_BITS + TS_RQ_BITS <= 64, "a bin is two 64-bit words");
constexpr uint32_t TS_BIN_BYTES = 16;

// one transition into the LDS histogram: bin = cls * A + a, next_cls in [0, 3), r in [-TS_RMAX, TS_RMAX]
__device__ __forceinline__ void gw_ts_count(uint64_t* hist, uint32_t bin, uint32_t next_cls, int32_t r, uint32_t dn)
{
    const uint64_t w0 = (1ull << (TS_CNT_BITS * next_cls)) | ((uint64_t)(dn != 0u ? 1u : 0u) << (3 * TS_CNT_BITS));
    const uint64_t w1 = (uint64_t)(uint32_t)(r + TS_RMAX) | ((uint64_t)(uint32_t)(r * r) << TS_RS_BITS);
    __hip_atomic_fetch_add(hist + 2u * bin, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(hist + 2u * bin + 1u, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void gw_ts_add(int64_t* cell, uint64_t v)      // a 64-bit global atomic add, nothing returned
{
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
// The block is one wave: its LDS adds and a flush's reads are operations of the same wave, kept in order by the hardware; the
// fences keep the compiler from moving them, and no block barrier is needed (or possible: lanes beyond N have left).
__device__ __forceinline__ void gw_wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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

// gw_rollout_autoreset: ct_rollout_sync_kernel's staged source with the episode's book -- the caller chooses the actions, the
// launch ends the episodes.  Nothing of the call is baked into the launch (no step0), so it may be recorded into a hipGraph.
// A rejected action (GW_FLAG_BADACT) leaves the env alone and repeats the current values, and is still a step of the episode:
// the body's put_feedback runs the hook below for it with reward 0 and the current done, as episodes_step_kernel sees such a row.
struct StagedEpisodes {
    uint8_t* ended;
    int32_t latest_next;                                 // what the env acts on next, minus counter_bound
    EpisodeBook ep;
};

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

// ---- a population of policies in one launch: gw_rollout_population (include/gymwipe_amd.h) ---------------------------------
// Env e runs policy e / M.  A block is one wave of 64 consecutive envs and M is a multiple of 64 (the launcher refuses any
// other), so a block has ONE policy, p = blockIdx.x * 64 / M: it stages that policy's [3][A] slice and flushes its episode
// tally into that policy's row.  ct_rollout_policy_ep's source with nothing stored per step.
struct PopulationActions : PolicyDraw {
    int64_t* row;                                        // the block's policy: [GW_EP_COLS] of the caller's [P][GW_EP_COLS]
    EpisodeBook ep;
};

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

struct ScoredEpisodeActions : EpisodeActions {
    StepScore sc;
    int32_t* delivered_out;
};

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

struct ScoredPopulationActions : PopulationActions {
    StepScore sc;
};

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

// gw_rollout_autoreset_scored: ct_rollout_sync_ep with the score where it has the reward, and the packets per step.  The hook
// that scores (GW_ROLLOUT_SRC_STEPPED) expands in the body's put_feedback, in front of the step loop's `d`, so the source keeps
// the step's sender itself (d_cur, as the drawn sources do).  There is no table here, so the weights' LDS copy is static: D
// words beside the body's own tables, their sum checked when the kernel is compiled.  Nothing of the call but its pointers,
// limits and weights is baked into the launch: it may be recorded into a hipGraph as its parent may.
struct ScoredStagedEpisodes : StagedEpisodes {
    StepScore sc;
    int32_t* delivered_out;
    int d_cur;                                           // the sender step k was staged with, inside the action space or not
};

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
bool fused_unavailable(const GwState& st, const GwDevConst& cst, int K, GwFusedLds lds)
{
    if (K <= 0 || K > st.rcap || st.ract != nullptr) return true;
    if (lds != GW_FUSED_NO_TABLE && (int64_t)st.D * cst.max_duration > GW_POLICY_A_MAX) return true;
    return lds == GW_FUSED_TABLE_HIST && K > (int)TS_STEPS;
}

// One launch of kernel_of(dt, m) -- the family's instantiation for the handle's sender count and the launch's MODE -- over a
// grid of 64-lane blocks, recorded in the family's slots from slot_base on.  The kernel's arguments are st, cst, K, args...
template <class KERNEL_OF, class... ARGS>
int launch_fused(const GwState& st, const GwDevConst& cst, const GwChunk& ch, int slot_base, GwFusedLds lds, KERNEL_OF kernel_of,
                 const ARGS&... args)
{
    const unsigned grid = (unsigned)((st.N + 63) / 64);
    const int mode = gw_step_mode(cst, ch.below_limits, false);
    const size_t A = (size_t)st.D * (size_t)cst.max_duration;
    const size_t dyn = lds == GW_FUSED_NO_TABLE ? 0 : 3 * A * (sizeof(uint32_t) + (lds == GW_FUSED_TABLE_HIST ? TS_BIN_BYTES : 0)) +
                                                      (lds == GW_FUSED_TABLE_SCORE ? (size_t)st.D * sizeof(int32_t) : 0);
    return gw_with_dt<GW_DTS_ROLLOUT_SYNC>(st.D, [&](auto dt) {          // (any other D: per-lane arrays in LDS)
        return gw_with_mode(mode, [&](auto m) {
            constexpr int DT = decltype(dt)::value, MODE = decltype(m)::value;
            const auto kernel = kernel_of(dt, m);
            if (lds == GW_FUSED_TABLE_HIST || lds == GW_FUSED_TABLE_SCORE) {
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
#define GW_KERNEL_OF(family) [](auto dt, auto m) { return &family<decltype(dt)::value, decltype(m)::value>; }

GwPolicyArgs policy_args(const GwPolicyStream& pol, const int32_t* obs_prev)
{
    return {pol.cdf, obs_prev, pol.seed, pol.step0, pol.env_id0};
}
GwEpisodeArgs episode_args(const gw_episodes& ep, int32_t* obs_next)
{
    return {ep.max_steps, ep.on_done, ep.state_dev, ep.tally_dev, obs_next};
}

} // namespace

// One step of the per-step forms (every queue mode), around the step's launch.  In front of it, the closed loops' draw for step
// pol.step0 from `obs_in` into row's action rows, env e from table e / M (one table: M = st.N); deliv_before: where a scored
// call's copy of the delivered counters goes, or nullptr ...
int gw_launch_policy_sample(const GwState& st, const GwDevConst& cst, const GwPolicyStream& pol, int64_t M, const int32_t* obs_in,
                            const GwRows& row, uint32_t* deliv_before, void* stream)
{
    hipLaunchKernelGGL(policy_sample_kernel, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)st.N,
                       (uint32_t)st.D * (uint32_t)cst.max_duration, (uint32_t)cst.max_duration, cst.counter_bound,
                       policy_args(pol, obs_in), (uint32_t)M, (const uint32_t*)st.sa, row.device, row.duration, deliv_before);
    return gw_launch_status();
}
// ... and behind it the episodes' bookkeeping on that row (row.device: the senders the step took), with the handle's reset
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

// The fused forms.  Each returns GW_EUNSUPPORTED where there is none (fused_unavailable): the caller draws and steps per step,
// or -- the two tallying forms -- refuses the call before its first launch.
int gw_launch_rollout_policy_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                 const int32_t* obs_prev, const GwRows& out)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_POLICY, GW_FUSED_TABLE, GW_KERNEL_OF(ct_rollout_policy), policy_args(pol, obs_prev),
                        out.device, out.duration, out.obs, out.reward, out.done);
}

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

int gw_launch_rollout_pstats_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                    const gw_episodes& ep, const int32_t* obs_prev, int32_t* obs_next, int64_t* table)
{
    if (fused_unavailable(st, cst, ch.K, GW_FUSED_TABLE_HIST)) return GW_EUNSUPPORTED;
    return launch_fused(st, cst, ch, GW_LS_ROLLOUT_PSTATS_EP, GW_FUSED_TABLE_HIST, GW_KERNEL_OF(ct_rollout_pstats_ep),
                        policy_args(pol, obs_prev), episode_args(ep, obs_next), table);
}

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

// gw_rollout's launch.  Returns GW_EUNSUPPORTED when this (D, K) has no fused kernel: the caller falls back to K step launches.
// (Its own availability rule, not fused_unavailable: a handle created for the event-loop form runs the step-synchronous one too
// when the switch is no longer set.)
int gw_launch_rollout_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const int32_t* device, const int32_t* duration,
                          const GwRows& out)
{
    const int K = ch.K, Kp = (K + 15) / 16 * 16, k_cap = st.rcap;
    uint16_t* const act_buf = st.ract;
    uint8_t* const fb_buf = st.rfb;
    int32_t* const obs = out.obs;
    float* const reward = out.reward;
    uint8_t* const done = out.done;
    if (K <= 0 || Kp > k_cap) return GW_EUNSUPPORTED;
    // A/B switch: the older form -- for handles created while the switch was set (they have its scratch records)
    const bool event_loop = getenv("GW_ROLLOUT_EVENT_LOOP") != nullptr && act_buf != nullptr && fb_buf != nullptr;
    if (!event_loop)                                      // the step-synchronous form: the caller's step-major arrays directly
        return launch_fused(st, cst, ch, GW_LS_ROLLOUT_SYNC, GW_FUSED_NO_TABLE, GW_KERNEL_OF(ct_rollout_sync_kernel), device, duration,
                            obs, reward, done);
    const unsigned grid = (unsigned)((st.N + 63) / 64);
    const int mode = gw_step_mode(cst, ch.below_limits, false);
    hipStream_t s = (hipStream_t)ch.stream;
    uint64_t* const rec = ch.rec;
    if (cst.max_duration > 0xfe) return GW_EUNSUPPORTED;  // (the event loop's packed action records hold a byte of duration)
    const uint32_t N = (uint32_t)st.N;
    const unsigned g256 = (unsigned)((st.N + TP_ENVS - 1) / TP_ENVS);      // one block per 64-env tile
    hipLaunchKernelGGL(pack_actions_kernel, dim3(g256), dim3(256), 0, s, N, K, Kp, device, duration, act_buf);
    gw_with_dt<GW_DTS_ROLLOUT_LOOP>(st.D, [&](auto dt) {                 // (any other D -- 5, 7, ...: per-lane arrays in LDS)
        gw_with_mode(mode, [&](auto m) {
            gw_note_launch(rec, GW_LS_ROLLOUT + 3 * gw_ls_dt(decltype(dt)::value) + decltype(m)::value);
            hipLaunchKernelGGL((ct_rollout_sfx_kernel<decltype(dt)::value, decltype(m)::value>), dim3(grid), dim3(64), 0, s,
                               st, cst, K, Kp, (const uint16_t*)act_buf, fb_buf);
        });
    });
    if (const int rc = gw_launch_status()) return rc;
    hipLaunchKernelGGL(expand_feedback_kernel, dim3(g256), dim3(256), 0, s, N, K, Kp, cst.counter_bound,
                       cst.payload_value, fb_buf, obs, reward, done);
    return gw_launch_status();
}
