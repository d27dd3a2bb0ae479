// gw_internal.h -- what the host side (gw_*_api.cpp, gw_tables.cpp) and every kernel file (*.hip) share: the device-side
// structs and table layouts, the launchers' prototypes, the launch record's slots.  Not part of the public C-ABI.
// (Device helpers: ct_common.hip.h; picking a kernel instantiation: gw_dispatch.h.)
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../include/gymwipe_amd.h"

#define GW_RING_PHYS      128          // physical ring slots per (env, sender); logical capacity GW_QUEUE_CAP
#define GW_RING_MASK      (GW_RING_PHYS - 1)
#ifndef GW_MAX_NSTATES
#define GW_MAX_NSTATES    16           // rx-power (noise residue) states per radio, see gw_tables.cpp
#endif

// Constants the kernels need, resident in device global memory (read through
// the scalar cache: every field is wave-uniform).
struct GwDevConst {
    int32_t D, R;                       // senders, radios (D+1)
    int32_t counter_bound, payload_value, mac_hdr, net_hdr, duration_factor, max_duration;
    int32_t mult[GW_MAX_DEVICES];
    double  slot, data_rate, bit_rate, coded_factor, max_ber, counter_interval;
    double  hdr_dur;                    // (mac_hdr*8)/data_rate
    double  hdr_bits;                   // (mac_hdr*8)*coded_factor
    // exact fast paths, each validated on the host at gw_create (gw_fastmath.h); 0 = use the plain form
    uint32_t inv16[GW_MAX_DEVICES];     // ceil(65536 / mult[i])
    uint16_t term[GW_MAX_RADIOS + 1];   // bit s of term[j]: noise state s of radio j is terminal (no talker changes it)
    double  inv_slot;                   // RN(1/slot)
    double  fmod_limit;                 // fast fmod is used for t < fmod_limit
    double  rcp_data_rate;              // RN(1/data_rate)
    double  cls_limit;                  // decode-certainty classes are valid for t < cls_limit
    int32_t fast_fmod, fast_div, fast_decide, idem_states;
    double  start_time;                 // simulated time at creation (test hook; the reference starts at 0)
    int32_t fast_ticks;                 // gw_tick_jump validated for counter_interval
    double  inv_interval;               // RN(1/counter_interval)
    double  tie_filter;                 // a tick can only fall exactly on t when (t - wake)/interval is this close to an integer
    int32_t no_traffic, peer_receive, float_duration;   // GW_CFG_NO_COUNTER_TRAFFIC / PEER_RECEIVE / FLOAT_DURATION
    int32_t dest[GW_MAX_DEVICES];
    double  ten_log_br, twenty_log_f, tx_power_dbm;   // 10*log10(bit_rate), 20*log10(frequency) (host glibc), tx power: live-PHY kernel
    uint32_t inv20[GW_MAX_DEVICES];     // ceil(2^20 / mult[i]): p / mult for p * mult < 2^20 (generic kernel's append index -> tick)
    double  inv_slot_lo, inv_interval_lo;   // one-sided reciprocals of gw_fast_fmod_lo / gw_tick_jump_lo (gw_fastmath.h)
};

struct GwBp { uint32_t t0, c0; };        // counting restarts at tick t0 with counter value c0
struct alignas(16) GwRec { uint32_t x, y, z, w; };   // a run-length queue's 16-byte record (gw_runq.h)

// Per-handle device state: sizes and device pointers (N = num_envs, D senders, R = D+1 radios), by value to the kernels that
// are not launched per step and in the header in front of the `ip` records for those that are (gw_blob_header below).  A
// pointer the handle's mode does not use is null.  Grouped by the gw_create branch that sets the fields -- but their ORDER is
// part of the kernels' code (the compiler merges the scalar loads of neighbouring fields: moving a group changes the
// instruction stream of every kernel that reads it), so the explicit-queue mode's fields and the common ones come in two
// groups each, and `block` keeps peer_rx and pe_stats apart.
struct GwState {
    // ---- every mode: sizes (gw_create, before any branch) ----
    int64_t   N;
    int32_t   D, R;     // host-side copies of the constants (launch sizing)
    int32_t   stage_chunks;  // default mode: 16-byte chunks of the state-major tables a step kernel stages in LDS (GwStripeLayout)

    // ---- explicit-queue mode (gw_create's GW_CFG_EXPLICIT_QUEUE branch), packed so that an env's scalars are three 16-byte
    //      loads and stores; MAC queues (SimpleMac._packetQueue) as run-length deques, gw_runq.h ----
    double*   xw;         // [N][2]     {now, next counter tick}
    uint32_t* xc;         // [N][4]     {counter, rvmask, last_abs | done << 31, sticky GW_FLAG_* bits}
    uint8_t*  xs;         // [N][XB]    rx-power state index per radio 0..D (stands for phy._receivedPower), padded to 16 bytes
    int32_t   XB;         //            bytes per xs record: 16 * ceil((D + 1) / 16)
    GwRec*    qrec;       // [D][N]     16-byte record: head run, tail run, bookkeeping
    uint64_t* runs;       // [N][D][GW_RING_PHYS]  the runs in between (touched only when a run is created or used up)

    // ---- default (suffix) mode (gw_create's branch without GW_CFG_EXPLICIT_QUEUE): MAC queues in the encoding of
    //      gw_queue.h, packed so that one env costs four 16-byte loads ----
    double*   tw;         // [N][2]     {now, next counter tick}
    uint32_t* tk;         // [N][4]     {tau = ticks so far, nbp = breakpoints so far, rvmask, last_abs | done << 31}: stored whole per step
    uint32_t* ip;         // [N][4]     {newest breakpoint (t0, c0), second newest breakpoint (t0, c0)}: written by reset / init only
    uint8_t*  qb;         // [N][RB]    bytes: queue length of sender 0..D-1, rx-power state of radio 0..D, pad
    GwBp*     bph;        // [N][GW_RING_PHYS]  ring of all breakpoints, entry j at [j & 127] (read only after >2 resets/100 ticks)
    int32_t   RB;         //            bytes per qb record: 16 * ceil((2*D + 1) / 16)
    uint16_t* ract;       // [N][rcap]  event-loop rollout scratch: packed actions (device | duration << 8), or nullptr
    uint8_t*  rfb;        // [N][rcap]  event-loop rollout scratch: packed feedback bytes, or nullptr
    int32_t   rcap;       //            steps per fused rollout launch (multiple of 16)
    uint32_t* sa;         // [4N + 2]   per-env event counters that cannot be derived from the state: {popped, delivered} bad
                          //            actions, sticky flags (layout: GW_SA_WORDS), bumped by no-return atomics only where
                          //            something happened; + the handle's step count.
                          //            (steps = launches - bad; transmissions = steps + popped; appended = tau * sum(mult);
                          //            dropped = appended - popped - sum(len): gw_api.cpp derives them)

    // ---- explicit-queue mode, continued: its event counters ----
    uint32_t* peer_rx;    // [D][N] or nullptr (GW_CFG_PEER_RECEIVE): packets a receive-mode MAC handed up
    int32_t   block;      //            threads per workgroup of the generic step kernel (GW_BLOCK; host only)
    uint64_t* pe_stats;   // [5][N] or nullptr (GW_CFG_PER_ENV_STATS): n_tx, n_delivered, n_appended, n_popped, n_dropped
    unsigned long long* totals;  // [n_slots][GW_T_COUNT], one 64-B slot per wave of the step launch:
                                 // steps, tx, delivered, appended, popped, dropped, flags_or, bad_actions

    // ---- every mode, continued: the link tables (gw_create, after the branches) ----
    int64_t   n_slots;           // waves a step launch can have: slots of `totals` (and of `stamps`)
    unsigned long long* stamps;  // diagnostic build only (make STAMPS=1): [n_slots][16] s_memtime stamps of the last launch
    const GwDevConst* cst;
    const uint8_t*    trans;     // [R to][R from][S]  state after hearing `from`
    const double*     ber;       // [R to][R from][S]  BER at `to` while hearing `from`, indexed by the NEW state
    const uint8_t*    cls;       // [R to][R from][S]  decode certainty at `to` hearing `from` (GW_CLS_*), by the NEW state
    // compact slices of ber/cls: [0][d][s] sender d hearing the RRM's announcement;  [1][d][s] the RRM hearing sender d
    const double*     ber2;      // [2][D][S]
    const uint8_t*    cls2;      // [2][D][S]
    const uint8_t*    blob;      // the step tables in one block: GwStripeLayout (default mode: the start of the `ip` block)
                                 // or GwBlobLayout (explicit-queue mode)

    // ---- live PHY (ct_step_dyn.hip; with either queue mode): gw_create's `dyn` branch (GW_CFG_PER_ENV_GEOMETRY, or a
    //      geometry without a finite noise-state set).  f64 received power per radio instead of the noise-state bytes.  One
    //      env's radios are CONTIGUOUS (rows of RP = gw_rp(R) doubles, 16-byte aligned): the all-pairs update of a step touches
    //      every radio of an env and one or two rows of its link matrix, so whole rows are what a lane -- or, for D >= 8, a
    //      group of D lanes -- reads ----
    double*   rxp;        // [N][RP]    phy._receivedPower, or nullptr (table PHY)
    const double* prx_tab;   // [R][R]  link power from -> to, mW (host glibc tables)
    const double* pos_tab;   // [R][2]  the handle's geometry
    const double* extra_tab; // [R][R]  custom attenuation per pair, dB
    double*   prx_env;    // [N][R][RP] per-env link powers, row = talker (GW_CFG_PER_ENV_GEOMETRY), else nullptr
    double*   pos_env;    // [N][R][2]  per-env positions
    double*   bcache;     // [N][D][2][2] {noise power, BER} last evaluated for: sender i hearing the RRM (entry 2i), the RRM
                          //            hearing sender i (entry 2i + 1: the same 32 bytes, one memory line); key NaN = empty.  BpskMcs.calculateBitErrorRate is two
                          //            log10, three pow and a sqrt in f64 (physical.py:25-58,208-212): ~350 instructions that
                          //            a step would otherwise spend twice; received powers settle on a few residue values.
    double*   rxr;        // [N]        default queue mode: a MIRROR of rxp[e][RRM], the RRM's own received power, which the walking lane
                          //            needs every step -- above 16 radios it is the only word of the rxp row's second memory line
                          //            that a step reads (the row's authoritative copy is written along with it, when it changes)
    uint64_t* talk;       // [N]        bit r: radio r has transmitted, i.e. its attenuation models exist (physical.py:500-528
                          //            creates a pair's model at first use) -- what Position.set's keep-stale rules ask
};
#if defined(__HIPCC__)
__host__ __device__
#endif
// doubles per row of rxp / prx_env (the row pitch).  Rows are read as whole 128-byte memory lines, and on this GPU the live-PHY
// step is bound by the NUMBER of lines a CU has in flight times their latency (in-kernel stamps): so a row never
// straddles a line -- up to 16 radios the pitch is the next power of two (one line holds 16 / pitch whole rows), above that a
// multiple of 16 doubles, with the D senders' entries in the first lines and the RRM's (index D, read by the walking lane only)
// behind them: at D = 16 the lane groups' row reads are ONE aligned line each (pitch 18 = 144 bytes took two or three).
constexpr int gw_rp(int R)
{
    return R <= 2 ? 2 : (R <= 4 ? 4 : (R <= 8 ? 8 : (R <= 16 ? 16 : ((R + 15) & ~15))));
}

// byte offsets inside GwState::blob (the default step kernel's tables; see ct_step_sfx.hip)
struct GwBlobLayout {
    int ber, mi, h1, r1, cls, lds_total, h2, total;
#if defined(__HIPCC__)
    __host__ __device__
#endif
    constexpr explicit GwBlobLayout(int D)
        : ber(0), mi(2 * D * GW_MAX_NSTATES * 8), h1(mi + (D * 8 + 15) / 16 * 16), r1(h1 + D * GW_MAX_NSTATES),
          cls(r1 + D * GW_MAX_NSTATES), lds_total(cls + 2 * D * GW_MAX_NSTATES), h2(lds_total),
          total(h2 + D * D * GW_MAX_NSTATES) {}
};

// The same tables for the default (suffix-queue) step kernels, STATE-MAJOR: after the multiplicity table one stripe per noise
// state s, holding everything the step looks up for that state --
//     [ mi u32[D][2] | stripe 0 | stripe 1 | ... | stripe 15 | h2 u8[S][D][D] ]
//     stripe s = { ber0 f64[D] (sender d hears the RRM), ber1 f64[D] (the RRM hears d), h1 u8[D], r1 u8[D], cls0 u8[D], cls1 u8[D] }
// -- so that a step kernel stages only the prefix that covers the states this handle's layout actually has (3 at D = 2, 4 at
// D = 4, 6 at D = 16, 8 at D = 32 with the default geometry; 16 is the limit): 352 bytes instead of 1.3 KB at D = 4, 2 KB instead
// of 5.2 KB at D = 16, through an L1 path that four waves per CU share at 64 bytes per clock.
struct GwStripeLayout {
    int mi, s0, stripe, ber0, ber1, h1, r1, cls0, cls1, h2, total;
#if defined(__HIPCC__)
    __host__ __device__
#endif
    constexpr explicit GwStripeLayout(int D)
        : mi(0), s0((8 * D + 15) / 16 * 16), stripe((20 * D + 15) / 16 * 16), ber0(0), ber1(8 * D), h1(16 * D), r1(17 * D),
          cls0(18 * D), cls1(19 * D), h2(s0 + GW_MAX_NSTATES * stripe), total(h2 + D * D * GW_MAX_NSTATES) {}
#if defined(__HIPCC__)
    __host__ __device__
#endif
    constexpr int staged_chunks(int nstates) const { return (s0 + nstates * stripe + 15) / 16; }   // 16-byte chunks to put in LDS
};

// In the default (suffix-queue) mode the step tables, the handle's GwDevConst and its GwState live in the SAME allocation as
// the `ip` records, in a header of gw_blob_header(D) bytes in front of them (gw_create uploads it; gw_set_state puts the two
// structs back after restoring the block):
//     [ tables (GwStripeLayout, gw_stripe_image) | GwDevConst at gw_hdr_cst_off | GwState at gw_hdr_st_off | pad to 256 ] [ ip records ... ]
// (sizeof both structs therefore shows in the block's size, gw_state_bytes and the snapshot layout.)
// The per-step kernels get `ip` as a preloaded leading argument and derive everything else from it.  Their argument block
// shrinks from 1.2 KB (both structs by value) to under 100 bytes: the runtime writes a launch's arguments into
// device-visible memory, and for 1.2 KB that alone took 3.6 us of the host's 5.5 us per launch (tools/launch_floor.hip).
#if defined(__HIPCC__)
#define GW_HDC __host__ __device__
#else
#define GW_HDC
#endif
GW_HDC constexpr int gw_hdr_cst_off(int D) { return (GwStripeLayout(D).total + 16 + 15) / 16 * 16; }
GW_HDC constexpr int gw_hdr_st_off(int D) { return gw_hdr_cst_off(D) + ((int)sizeof(GwDevConst) + 15) / 16 * 16; }
GW_HDC constexpr int gw_blob_header(int D) { return (gw_hdr_st_off(D) + (int)sizeof(GwState) + 255) / 256 * 256; }

// decode certainty of a link in a given noise state (host: gw_tables.cpp; valid while t < fmod_limit)
enum { GW_CLS_COMPUTE = 0, GW_CLS_OK = 1, GW_CLS_HDR_FAIL = 2, GW_CLS_PAY_FAIL = 3 };

// layout of GwState::sa (uint32 words): [0, 2N) = per env {popped, delivered} as ONE u64 (one atomic bumps both),
// [2N, 3N) bad actions, [3N, 4N) sticky flags, then two words = the handle's env.step() count as a u64 (bumped by one lane
// per launch, so that launches replayed from a hipGraph are counted too)
enum { GW_SA_WORDS = 4 };

enum { GW_T_STEPS = 0, GW_T_TX, GW_T_DELIV, GW_T_APP, GW_T_POP, GW_T_DROP, GW_T_FLAGS, GW_T_BAD, GW_T_COUNT };

// Linear plant (plant_mfma.hip, gw_plant_api.cpp)
struct GwPlantDev {
    int64_t N;
    double* x;                    // [N][4]
    double* u;                    // [N]
    double* t_last;               // [N]
    unsigned long long* nsub;     // [N] substeps applied so far
    const double* Pop;            // [KMAX/4][64]  A operand of the state MFMA, by lane
    const double* Qtab;           // [KMAX+1][4]   Q_k = sum_{j<k} A^j B, the accumulated input vector of k substeps (Q_0 = 0)
    double dt, inv_dt;
};

// PHY grid (grid_phy.hip, gw_grid_api.cpp)
#define GW_GRID_EVENTS 11
struct GwGridLane {                     // one radio of one replica
    double   ev_t[GW_GRID_EVENTS];      // pending events of this device: time (+inf = none) ...
    uint32_t ev_k[GW_GRID_EVENTS];      // ... and key = priority bit | insertion id
    double   rx_power, tx_stop, rx_stop, rxi_stop, err_sum, ber, t_seg, px, py;
    uint32_t move_k, tx_on;             // moves made so far; 1 while this device's transmission is on the air (NOTIFY..END)
    uint32_t n_sent, queued, hdr_ok, hdr_fail, pay_ok, pay_fail, flags;
    int32_t  rx_src, rxi_src;
    uint8_t  started, handler_running, transmitting, receiving, waiting_rx, rx_running, rx_phase, pad;
};
struct GwGridEnv { double now; uint32_t eid, events, n_tx, first_run; };
struct GwGridDev {
    int64_t N; int32_t n, pad;
    GwGridLane* lanes;                  // [N][n]
    GwGridEnv*  envs;                   // [N]
    const double* prx;                  // [n from][n to] received power, mW
    double slot, send_interval, bit_rate, hdr_bits, pay_bits, hdr_dur, pay_dur, ten_log_br, sqrt2pi;
    uint32_t max_events, mobile;        // bound on events per launch (a logic error must not hang the GPU)
    double   move_interval, move_span, tx_power_dbm, twenty_log_f;
    double*  txp;                       // [N][n][n] mobile: received power of transmission i stored at radio j; behind it the
                                        // stand-by state of the links (grid_phy.hip: grid_link_row, grid_link_masks)
    unsigned long long seed;
};
// Lanes per replica of grid_run_kernel<MOBILE, GW>: the power of two that holds its n radios, 64 / GW replicas per wave ...
// unless that leaves SIMDs without a wave (1 024 of them): a small batch spreads out first (4 096 replicas of 4 radios:
// groups of 16 lanes, four replicas per wave, 1 024 waves -- sixteen per wave would be 256 waves on a quarter of the chip).
// Pure: the launcher and gw_grid_selftest_width both ask here.
static inline int gw_grid_pick_width(int64_t N, int n)
{
    int gw = n <= 4 ? 4 : (n <= 8 ? 8 : (n <= 16 ? 16 : (n <= 32 ? 32 : 64)));
    while (gw < 64 && N <= (65536 - 64) / gw) gw *= 2;      // fewer than 1 024 waves: (N * gw + 63) / 64 < 1024, without the product
    return gw;
}
int gw_grid_launch_run(const GwGridDev& g, double seconds, void* stream, int* width_ran);   // width_ran: the GW it launched
int gw_grid_launch_set_position(const GwGridDev& g, int dev, const double* xs, const double* ys, void* stream);
int gw_grid_launch_init(const GwGridDev& g, const double* delays_dev, const double* pos_dev, double thermal, void* stream);

struct GwHostTables;

// Closed control loop (ctrl_step.hip, ctrl_rollout.hip, ctrl_rollout_feedback.hip, gw_ctrl_api.cpp)
struct GwCtrlDev {
    int64_t N;
    double *now, *wake, *x, *u, *ang;          // [N], [N], [N][4], [N], [N]
    uint32_t *ktick, *got, *ntx, *ncmd, *nsub, *flags;   // [N], [N][2], [N] ...
    uint16_t* qhl;                             // [2][N]  head | len << 8 of the sensor's and the controller's queue
    uint8_t*  rxs;                             // [4][N]  rx-power state per radio
    double*   pay;                             // [N][2][GW_RING_PHYS] payload values of the queued packets
    double A[16], B[4];
    uint32_t start, period;
    const GwDevConst* cst;
    const uint8_t* trans;                      // [4][4][S]
    const double*  ber;                        // [4][4][S]
};
// Per-env initial state and episode record (ctrl_rollout.hip).  A struct of its own: GwCtrlDev is ctrl_step_kernel's by-value
// argument, and a field added there would change that kernel's code.
struct GwCtrlEpi {
    double *x_init, *u_init, *cost;            // [N][4], [N], [N]
    uint32_t* age;                             // [N]
};
// Per-env controller: the PID gains and the controller's last error (the rule: include/gymwipe_amd.h, gw_ctrl_set_gains).  One
// block f64[N][4] = {kp, ki, kd, last_error}; a struct of its own for GwCtrlEpi's reason.
struct GwCtrlPid {
    double* pid;                               // [N][4]
};
// Per-env plant disturbance (the rule: include/gymwipe_amd.h, gw_ctrl_set_disturbance).  One block of 48-byte records
// {g[4] f64, key u64, n u64}, addressed as u64[N][6]; a struct of its own for GwCtrlEpi's reason.
struct GwCtrlDist {
    uint64_t* rec;                             // [N][6]
};
// Per-env packet erasures (the rule: include/gymwipe_amd.h, gw_ctrl_set_loss).  One block of 48-byte records
// {thr[4] u32, key u64, n u64, lost[4] u32}, addressed as u64[N][6]; a struct of its own for GwCtrlEpi's reason.
struct GwCtrlLoss {
    uint64_t* rec;                             // [N][6]
};
// The variant of its kernels a handle launches, named by the blocks they read.  The set pointers form a prefix: none (the
// kernels with the default rule compiled in, no block read), g (their PID instantiations), g and w (the plant disturbed at the
// end of every substep as well), all three (one erasure draw per transmission as well).  The step and rollout launchers below
// pick the kernel from it and pass the set blocks as the kernel's last arguments, in this order.
struct GwCtrlBlocks {
    const GwCtrlPid* g;
    const GwCtrlDist* w;
    const GwCtrlLoss* x;
};
int gw_ctrl_launch_init(const GwCtrlDev& c, const double* x0, double u0, void* stream);                   // ctrl_step.hip, as the next
int gw_ctrl_launch_step(const GwCtrlDev& c, const GwCtrlBlocks& v, const int32_t* device, const int32_t* duration, int32_t* obs,
                        float* reward, double* angle_deg, void* stream);
int gw_ctrl_launch_fill_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, double u0, void* stream);   // ctrl_rollout.hip
int gw_ctrl_launch_set_initial(const GwCtrlDev& c, const GwCtrlEpi& s, const double* x0, const double* u0, const uint8_t* mask,
                               void* stream);
int gw_ctrl_launch_set_gains(const GwCtrlDev& c, const GwCtrlPid& g, const double* gains, const uint8_t* mask, void* stream);
int gw_ctrl_launch_set_disturbance(const GwCtrlDev& c, const GwCtrlDist& w, const double* g, const uint64_t* key, const uint8_t* mask,
                                   void* stream);
int gw_ctrl_launch_set_loss(const GwCtrlDev& c, const GwCtrlLoss& x, const uint32_t* thr, const uint64_t* key, const uint8_t* mask,
                            void* stream);
int gw_ctrl_launch_reset(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, const uint8_t* mask, int32_t* obs, void* stream);
int gw_ctrl_launch_rollout(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps, const int32_t* device,
                           const int32_t* duration, const gw_ctrl_episodes* ep, int32_t* obs, float* reward, double* angle_deg,
                           uint8_t* ended, void* stream);
int gw_ctrl_launch_rollout_schedules(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps, const uint8_t* sched,
                                     int32_t P, int32_t L, const gw_ctrl_episodes& ep, double* tally, void* stream);
int gw_ctrl_launch_rollout_feedback(const GwCtrlDev& c, const GwCtrlEpi& s, const GwCtrlBlocks& v, int32_t steps,
                                    const gw_ctrl_feedback& fb, const gw_ctrl_episodes& ep, const gw_ctrl_feedback_rows* rows,
                                    double* tally, void* stream);                       // ctrl_rollout_feedback.hip
int gw_fill_dev_const(const gw_config& cfg, const GwHostTables& tab, GwDevConst& k);   // gw_api.cpp
int gw_validate_config(const gw_config& cfg);                                           // gw_api.cpp

// Host-side link tables (gw_tables.cpp)
struct GwHostTables {
    int D, R;
    double att[GW_MAX_RADIOS][GW_MAX_RADIOS];        // dB
    double prx[GW_MAX_RADIOS][GW_MAX_RADIOS];        // mW, [from][to]
    double thermal;                                   // mW
    double data_rate, coded_factor;
    int    overflow;                                  // some radio's state closure exceeds GW_MAX_NSTATES: live-PHY kernel
    int    nstates[GW_MAX_RADIOS];
    double state_val[GW_MAX_RADIOS][GW_MAX_NSTATES];  // mW; index 0 = thermal
    // flattened [to][from][s]
    uint8_t trans[GW_MAX_RADIOS * GW_MAX_RADIOS * GW_MAX_NSTATES];
    uint8_t cls[GW_MAX_RADIOS * GW_MAX_RADIOS * GW_MAX_NSTATES];
    double  ber[GW_MAX_RADIOS * GW_MAX_RADIOS * GW_MAX_NSTATES];
};

// returns GW_OK or an error code; msg receives a description on failure
int gw_build_tables(const gw_config& cfg, GwHostTables& out, char* msg, size_t msglen);
// What gw_create uploads of them (gw_tables.cpp).  The two links a step uses per sender, [0][d][s] sender d hearing the RRM
// and [1][d][s] the RRM hearing sender d (GwState::ber2 / cls2); and the step tables as one image: GwBlobLayout for the
// generic kernel, GwStripeLayout for the suffix mode, whose *stage_chunks is GwState::stage_chunks.
void gw_link_slices(const GwHostTables& tab, std::vector<double>& ber2, std::vector<uint8_t>& cls2);
std::vector<uint8_t> gw_blob_image(const GwHostTables& tab, const GwDevConst& k);
std::vector<uint8_t> gw_stripe_image(const GwHostTables& tab, const GwDevConst& k, int* stage_chunks);

// kernel launchers (ct_step.hip); stream is a hipStream_t
int gw_launch_init(const GwState& st, void* stream);
int gw_launch_reset(const GwState& st, const uint8_t* mask, int32_t* obs, void* stream);
int gw_launch_step(const GwState& st, const int32_t* device, const int32_t* duration,
                   int32_t* obs, float* reward, uint8_t* done, void* stream, bool no_split, uint64_t* rec);
int gw_launch_received(const GwState& st, int32_t* out, void* stream);
int gw_launch_enqueue(const GwState& st, int sender, const int32_t* payload_bytes, void* stream);
// The hipFunction_t (as void*) of a handle's per-call kernels on ITS device: ct_step_sfx_kernel<D, MODE> for MODE 0..2 and
// ct_reset_sfx_kernel.  Resolved once, at gw_create with the handle's device current (a module's functions belong to the
// device it was loaded on), so that a launch neither asks for the current device nor looks the kernel up -- nor dispatches
// on the sender count: step_slot is the launch-record slot of step[0].  A null entry sends that launch through `<<< >>>`.
struct GwSfxFns { void* step[3]; void* reset; int step_slot; };
void gw_resolve_sfx_functions(int D, GwSfxFns* out);       // ct_step_sfx.hip
int gw_launch_step_sfx(const GwState& st, const GwDevConst& cst, const int32_t* device, const int32_t* duration,
                       int32_t* obs, float* reward, uint8_t* done, uint8_t* feedback_byte, void* stream, bool below_limits,
                       uint64_t* rec, const GwSfxFns* fns);
int gw_launch_reset_sfx(const GwState& st, const uint8_t* mask, int32_t* obs, void* stream, const GwSfxFns* fns);
int gw_launch_init_sfx(const GwState& st, void* stream);
// The rollout launchers (ct_rollout_*.hip, one file per group of families: ct_rollout_sync.hip.h names each family's; the file
// behind each declaration below).  What a call passes to every one of its launches travels as three small values:
struct GwChunk {                        // one launch of a call: its steps, where it goes, what the host knows about it
    int K;
    void* stream;
    bool below_limits;                  // (gw_env_below_limits, for all K steps)
    uint64_t* rec;                      // the handle's launch record, or nullptr
};
struct GwPolicyStream {                 // the policy a closed loop draws from, and the identity of its action stream
    const uint32_t* cdf;                // [3][A] (gw_rollout_population: [P][3][A])
    uint64_t seed, step0, env_id0;      // step0: of the launch's (or the per-step draw's) first step
    GwPolicyStream at(int32_t s) const { return {cdf, seed, step0 + (uint64_t)s, env_id0}; }
};
struct GwRows {                         // a call's [K][N] outputs; a member a call does not have is nullptr
    int32_t *device, *duration;         // the actions drawn (the closed loops)
    int32_t* obs; float* reward; uint8_t* done;
    uint8_t* ended;                     // the episodic calls
    GwRows at(int64_t o) const          // the rows from element o on
    {
        return {device ? device + o : nullptr, duration ? duration + o : nullptr, obs + o, reward + o, done + o, ended ? ended + o : nullptr};
    }
};
// Each fused form returns GW_EUNSUPPORTED where the handle (or the call) has none; the per-step forms' launches follow.
int gw_launch_rollout_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const int32_t* device, const int32_t* duration,
                          const GwRows& out);                                                       // gw_rollout (ct_rollout_sfx.hip)
int gw_launch_rollout_policy_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                 const int32_t* obs_prev, const GwRows& out);                       // gw_rollout_policy (ct_rollout_policy.hip)
#define GW_TS_STEPS 64                  // steps per ct_rollout_pstats launch at most: its LDS histogram's bit budget (ct_rollout_stats.hip)
int gw_launch_rollout_pstats_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                 const int32_t* obs_prev, int32_t* obs_last, int32_t* ret, int64_t* table);   // gw_rollout_policy_stats (ct_rollout_stats.hip)
// score (the three episodic forms that take one): nullptr, or the _scored call's weights -- the family with the step's score
// where it has the reward; delivered: that call's packets per step
int gw_launch_rollout_policy_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                    const gw_episodes& ep, const gw_score* score, const int32_t* obs_prev, int32_t* obs_next,
                                    const GwRows& out, int32_t* delivered);                         // gw_rollout_episodes[_scored] (ct_rollout_policy.hip)
int gw_launch_rollout_pstats_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                    const gw_episodes& ep, const int32_t* obs_prev, int32_t* obs_next, int64_t* table);   // gw_rollout_episodes_stats (ct_rollout_stats.hip)
int gw_launch_rollout_autoreset_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const int32_t* device,
                                    const int32_t* duration, const gw_episodes& ep, const gw_score* score, int32_t* obs_next,
                                    const GwRows& out, int32_t* delivered);                         // gw_rollout_autoreset[_scored] (ct_rollout_autoreset.hip)
// gw_rollout_backlog: the scored autoreset form with the actions chosen in the launch from the queue lengths (out.device /
// out.duration / seen_len receive them) ... (these four: ct_rollout_backlog.hip)
int gw_launch_rollout_backlog_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_backlog_policy& pol,
                                  const gw_episodes& ep, const gw_score& score, int32_t* obs_next, const GwRows& out, int32_t* seen_len,
                                  int32_t* delivered);
// ... and one step's choice for its per-step form, from the queue-length bytes of the default queue mode
int gw_launch_backlog_select(const GwState& st, const GwDevConst& cst, const gw_backlog_policy& pol, const GwRows& row, int32_t* seen_len,
                             void* stream);
// gw_rollout_backlog_population: env e under scheduler policy e / envs_per_policy of pop.policies_dev, nothing stored per step ...
int gw_launch_rollout_backlog_pop_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_backlog_population& pop,
                                      const gw_episodes& ep, const gw_score& score, int32_t* obs_next);
// ... and one step's choice for its per-step form, into row.device / row.duration
int gw_launch_backlog_select_pop(const GwState& st, const GwDevConst& cst, const gw_backlog_population& pop, const GwRows& row, void* stream);
// gw_rollout_population[_scored]: env e runs policy e / envs_per_policy (pol.cdf: the population's tables), nothing stored per step
// (ct_rollout_pop.hip)
int gw_launch_rollout_pop_ep_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_population& pop,
                                 const GwPolicyStream& pol, const gw_episodes& ep, const gw_score* score, const int32_t* obs_prev,
                                 int32_t* obs_next);
// gw_rollout_controller / gw_rollout_controller_population: the scored closed loops with a finite-state controller (pol.cdf: its
// [S][3][A], or the population's [P][S][3][A]); fused or GW_EUNSUPPORTED, there is no per-step form (ct_rollout_fsc.hip)
int gw_launch_rollout_fsc_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_controller& ctl,
                              const GwPolicyStream& pol, const gw_episodes& ep, const gw_score& score, const int32_t* obs_prev,
                              int32_t* obs_next, const GwRows& out, int32_t* delivered, uint8_t* node_out);
int gw_launch_rollout_fsc_pop_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const gw_controller_population& pop,
                                  const GwPolicyStream& pol, const gw_episodes& ep, const gw_score& score, const int32_t* obs_prev,
                                  int32_t* obs_next);
// the table from recorded transitions (ended: nullptr, or gw_transition_stats_ep's rows; ct_rollout_stats.hip)
int gw_launch_transition_stats(int64_t N, int K, int D, int max_duration, int counter_bound, const int32_t* obs_prev,
                               const int32_t* device, const int32_t* duration, const int32_t* obs, const float* reward,
                               const uint8_t* done, const uint8_t* ended, int64_t* table, void* stream);
// The three tallying forms with the packets a step delivered in an eighth column (table: [3][A][GW_TSD_COLS]; delivered: the
// recorded rows' int32[K][N]; ct_rollout_stats.hip)
int gw_launch_rollout_pstats_d_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                   const int32_t* obs_prev, int32_t* obs_last, int32_t* ret, int64_t* table);   // gw_rollout_policy_stats_delivered
int gw_launch_rollout_pstats_epd_sfx(const GwState& st, const GwDevConst& cst, const GwChunk& ch, const GwPolicyStream& pol,
                                     const gw_episodes& ep, const int32_t* obs_prev, int32_t* obs_next, int64_t* table);   // gw_rollout_episodes_stats_delivered
int gw_launch_transition_stats_d(int64_t N, int K, int D, int max_duration, int counter_bound, const int32_t* obs_prev,
                                 const int32_t* device, const int32_t* duration, const int32_t* obs, const float* reward,
                                 const uint8_t* done, const uint8_t* ended, const int32_t* delivered, int64_t* table, void* stream);
// One step of the per-step forms.  The draw for step pol.step0 from `obs_in` into row.device / row.duration, env e from table
// e / M (one table: M = st.N), with a scored call's copy of the delivered counters into deliv_before (or nullptr); and, behind
// the step's launch, the episodes' bookkeeping on that row (ended, the handle's reset mask, obs_next): scored with deliv_before
// where there is a score, into row e / M of pop_tally where there is one, the packets per step into delivered_out where kept.  (The draw:
// ct_rollout_policy.hip; the bookkeeping: ct_rollout_autoreset.hip.)
int gw_launch_policy_sample(const GwState& st, const GwDevConst& cst, const GwPolicyStream& pol, int64_t M, const int32_t* obs_in,
                            const GwRows& row, uint32_t* deliv_before, void* stream);
int gw_launch_episodes_step(const GwState& st, const GwDevConst& cst, const gw_episodes& ep, const gw_score* score, int64_t M,
                            int64_t* pop_tally, const uint32_t* deliv_before, int32_t* obs_next, const GwRows& row, uint8_t* mask,
                            int32_t* delivered_out, void* stream);
int gw_launch_received_sfx(const GwState& st, int32_t* out, void* stream);
int gw_launch_delivered_sfx(const GwState& st, uint32_t* out, void* stream);
int gw_launch_clear_flags(const GwState& st, void* stream);          // ct_step_sfx.hip (both queue modes)
int gw_launch_step_dyn(const GwState& st, const GwDevConst& cst, const int32_t* device, const int32_t* duration,
                       int32_t* obs, float* reward, uint8_t* done, void* stream, uint64_t* rec);
int gw_launch_init_dyn(const GwState& st, const GwDevConst& cst, double thermal, void* stream);
int gw_launch_set_position(const GwState& st, const GwDevConst& cst, int radio, const double* xs, const double* ys,
                           const double* all_pos, const uint8_t* mask, void* stream);

int gw_launch_pack_feedback(int64_t count, int center, int pv, const int32_t* obs, const float* reward, const uint8_t* done,
                            uint8_t* packed, uint32_t* bad, void* stream);
int gw_launch_unpack_feedback(int64_t count, int center, int pv, const uint8_t* packed, int32_t* obs, float* reward, uint8_t* done,
                              void* stream);

#define GW_MAX_MULT        100         // packets per tick in the suffix encoding = the handle-wide limit (the deque's capacity: more
                                       // than 100 packets per tick only ever leaves the last 100 in the queue).  gw_ceil_div's
                                       // reciprocal is exact for len <= 100 up to multiplicity 256 (checked exhaustively by
                                       // tests/test_host_logic.py), the kernels' 24-bit multiplies far beyond.

// Sender counts with a kernel instantiation of their own (template parameter DT; every other count runs DT = 0), one list
// per kernel family.  Each family's launcher dispatches over its list (gw_dispatch.h) and nothing else restates it.
#define GW_DTS_STEP          2, 3, 4, 5, 6, 7, 8, 16, 32    // ct_step_sfx_kernel
#define GW_DTS_ROLLOUT_SYNC  2, 3, 4, 5, 6, 7, 8, 16, 32    // every includer of ct_rollout_sync_body.h, through launch_fused (ct_rollout_sync.hip.h lists the families)
#define GW_DTS_ROLLOUT_LOOP  2, 3, 4, 6, 8, 16, 32          // ct_rollout_sfx_kernel (event loop, ct_rollout_sfx.hip)
#define GW_DTS_LIVE          2, 3, 4, 6, 8, 16, 32          // ct_step_live_kernel
#define GW_DTS_GENERIC       2, 3, 4, 8, 16                 // ct_step_kernel on the table PHY
#define GW_DTS_GENERIC_LIVE  4, 16                          // ct_step_kernel on the live PHY (DYN)

// Launch record (gw_selftest_launches): one slot per instantiation of the step / rollout kernel families, counted by the
// launcher that picks the instantiation -- in the handle's own array (rec, may be null) and in the process-wide one (a relaxed
// atomic).  Slot = family base + sender-count index (gw_ls_dt) x the family's template combinations + their index; names are
// formatted only by the query (gw_api.cpp).
#define GW_LS_DTS GW_DTS_STEP, 0                            // the record's sender-count order (every family's list is a subset); 0 = any D
enum {
    GW_LS_NDT = 10,
    GW_LS_STEP_SFX = 0,                                    // ct_step_sfx_kernel<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_SYNC = GW_LS_STEP_SFX + 3 * GW_LS_NDT,   // ct_rollout_sync_kernel<DT, MODE>
    GW_LS_ROLLOUT = GW_LS_ROLLOUT_SYNC + 3 * GW_LS_NDT,    // ct_rollout_sfx_kernel<DT, MODE> (event loop)
    GW_LS_PEND = GW_LS_ROLLOUT + 3 * GW_LS_NDT,            // pend_step_kernel<MODE, HALF>: 6
    GW_LS_GENERIC = GW_LS_PEND + 6,                        // ct_step_kernel<DT, PER_ENV_STATS, DYN, SPLIT>: 8 per DT
    GW_LS_LIVE = GW_LS_GENERIC + 8 * GW_LS_NDT,            // ct_step_live_kernel<DT, PER_ENV>: 2 per DT
    GW_LS_ROLLOUT_POLICY = GW_LS_LIVE + 2 * GW_LS_NDT,     // ct_rollout_policy<DT, MODE>: 3 per DT (appended: the slots above keep
    GW_LS_ROLLOUT_PSTATS = GW_LS_ROLLOUT_POLICY + 3 * GW_LS_NDT,   // ct_rollout_pstats<DT, MODE>: 3 per DT    their numbers)
    GW_LS_ROLLOUT_POLICY_EP = GW_LS_ROLLOUT_PSTATS + 3 * GW_LS_NDT,      // ct_rollout_policy_ep<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_PSTATS_EP = GW_LS_ROLLOUT_POLICY_EP + 3 * GW_LS_NDT,   // ct_rollout_pstats_ep<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_SYNC_EP = GW_LS_ROLLOUT_PSTATS_EP + 3 * GW_LS_NDT,     // ct_rollout_sync_ep<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_POP_EP = GW_LS_ROLLOUT_SYNC_EP + 3 * GW_LS_NDT,        // ct_rollout_pop_ep<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_POLICY_EPS = GW_LS_ROLLOUT_POP_EP + 3 * GW_LS_NDT,     // ct_rollout_policy_eps<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_POP_EPS = GW_LS_ROLLOUT_POLICY_EPS + 3 * GW_LS_NDT,    // ct_rollout_pop_eps<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_SYNC_EPS = GW_LS_ROLLOUT_POP_EPS + 3 * GW_LS_NDT,      // ct_rollout_sync_eps<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_BACKLOG = GW_LS_ROLLOUT_SYNC_EPS + 3 * GW_LS_NDT,      // ct_rollout_backlog<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_BACKLOG_POP = GW_LS_ROLLOUT_BACKLOG + 3 * GW_LS_NDT,   // ct_rollout_backlog_pop<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_FSC = GW_LS_ROLLOUT_BACKLOG_POP + 3 * GW_LS_NDT,       // ct_rollout_fsc<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_FSC_POP = GW_LS_ROLLOUT_FSC + 3 * GW_LS_NDT,           // ct_rollout_fsc_pop<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_PSTATS_D = GW_LS_ROLLOUT_FSC_POP + 3 * GW_LS_NDT,      // ct_rollout_pstats_d<DT, MODE>: 3 per DT
    GW_LS_ROLLOUT_PSTATS_EPD = GW_LS_ROLLOUT_PSTATS_D + 3 * GW_LS_NDT,   // ct_rollout_pstats_epd<DT, MODE>: 3 per DT
    GW_LS_COUNT = GW_LS_ROLLOUT_PSTATS_EPD + 3 * GW_LS_NDT
};
constexpr int gw_ls_dt(int DT)                             // index of DT in GW_LS_DTS (a count without a slot of its own: DT = 0's)
{
    constexpr int dts[GW_LS_NDT] = {GW_LS_DTS};
    int i = 0;
    while (i < GW_LS_NDT - 1 && dts[i] != DT) ++i;
    return i;
}
void gw_note_launch(uint64_t* rec, int slot);              // gw_api.cpp
