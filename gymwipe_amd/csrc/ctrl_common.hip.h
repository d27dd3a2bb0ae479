// ctrl_common.hip.h -- what the control-loop kernels share: the step kernels (ctrl_step.hip: one step per launch), the fused
// kernels of ctrl_rollout.hip (K steps per launch) and the angle-feedback kernels of ctrl_rollout_feedback.hip.  A lane's state,
// its two queues during a step and the staging of a step's appends; the controller's gains, the plant's disturbance and the
// links' packet erasures where a kernel's variant reads them; and the pieces every kernel is put together from -- its opening,
// the lane's load, store and in-register reset -- each stated once, as text (below: why not as functions).  The step itself is
// text as well: ctrl_step_body.h, under the variant's symbols through ctrl_step_variant.h.
#pragma once
#include "ct_common.hip.h"

namespace gwk {

constexpr int CR = 4, CRRM = 3;                             // radios (3 network devices + RRM), index of the RRM
constexpr int S = GW_MAX_NSTATES;

struct Lane {                                               // everything indexed by a run-time device id goes through
    double now, wake, x[4], u, ang;                         // selects below: a dynamically indexed member array would
    uint32_t ktick, got1, got2, ntx, ncmd, nsub, fl;        // send the whole struct to scratch memory
    uint32_t rxs[CR];
};

// The controller of one env in the PID instantiations (ctrl_step_body.h under GW_CTRL_PID): its gains and its last error, four
// f64 in registers across all steps of a launch.  GwCtrlPid's block holds them as {kp, ki, kd, last_error}, 32 bytes per env:
// two 16-byte loads when a launch opens, one 8-byte store of `last` when it closes (nothing inside a launch changes a gain).
struct Pid {
    double kp, ki, kd, last;
};

__device__ __forceinline__ void pid_load(Pid& G, const GwCtrlPid& g, int64_t e)
{
    const double2* p = reinterpret_cast<const double2*>(g.pid + e * 4);       // hipMalloc'ed, 32-byte records: 16-byte aligned
    const double2 a = p[0], b = p[1];
    G.kp = a.x; G.ki = a.y; G.kd = b.x; G.last = b.y;
}

__device__ __forceinline__ void pid_store(const Pid& G, const GwCtrlPid& g, int64_t e)
{
    g.pid[e * 4 + 3] = G.last;
}

// The plant disturbance of one env in the disturbance instantiations (ctrl_step_body.h under GW_CTRL_DIST): its four weights,
// its key and the count of draws, in registers across all steps of a launch.  GwCtrlDist's block holds {g[4], key, n}, 48
// bytes per env: three 16-byte loads when a launch opens, one 8-byte store of n when it closes.  `nc` is n * DIST_STEP mod
// 2^64 carried as a running sum: one multiply per launch, an add per draw.
constexpr uint64_t DIST_STEP = 0xD1B54A32D192ED03ull;

struct Dist {
    double g[4];
    uint64_t key, n, nc;
};

__device__ __forceinline__ void dist_load(Dist& W, const GwCtrlDist& w, int64_t e)
{
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(w.rec + e * 6);  // hipMalloc'ed, 48-byte records: 16-byte aligned
    const ulonglong2 a = p[0], b = p[1], d = p[2];
    W.g[0] = __longlong_as_double((long long)a.x); W.g[1] = __longlong_as_double((long long)a.y);
    W.g[2] = __longlong_as_double((long long)b.x); W.g[3] = __longlong_as_double((long long)b.y);
    W.key = d.x; W.n = d.y;
    W.nc = d.y * DIST_STEP;
}

__device__ __forceinline__ void dist_store(const Dist& W, const GwCtrlDist& w, int64_t e)
{
    w.rec[e * 6 + 5] = W.n;
}

// the mixer of gw_policy_u (ct_rollout_sync.hip.h): what both kinds of draw below put their key ^ (n * STEP) through
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one draw: the mixer on key ^ (n * DIST_STEP), its top 32 bits as a signed integer times 2^-31 -- uniform on [-1, 1), a
// multiple of 2^-31, every operation exact
__device__ __forceinline__ double dist_draw(Dist& W)
{
    const uint64_t z = mix64(W.key ^ W.nc);
    W.n += 1ull;
    W.nc += DIST_STEP;
    return (double)(int32_t)(uint32_t)(z >> 32) * 0x1p-31;
}

// The packet erasures of one env in the loss instantiations (ctrl_step_body.h under GW_CTRL_LOSS): the four links' thresholds,
// the key, the count of draws and the four links' erasure counts, in registers across all steps of a launch.  GwCtrlLoss's
// block holds {thr[4] u32, key u64, n u64, lost[4] u32}, 48 bytes per env: three 16-byte loads when a launch opens, one 8-byte
// store of n and one 16-byte store of lost when it closes.  `nc` is n * LOSS_STEP mod 2^64 carried as a running sum, as
// Dist::nc is.  thr and lost are only ever indexed by constants: the step selects its two thresholds from the device once and
// adds its erasures to the right counters with selects (Lane says why).
constexpr uint64_t LOSS_STEP = 0xA0761D6478BD642Full;

struct Loss {
    uint32_t thr[4], lost[4];
    uint64_t key, n, nc;
};

__device__ __forceinline__ void loss_load(Loss& X, const GwCtrlLoss& x, int64_t e)
{
    const uint4* p = reinterpret_cast<const uint4*>(x.rec + e * 6);            // hipMalloc'ed, 48-byte records: 16-byte aligned
    const uint4 a = p[0], c = p[2];
    const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(p + 1);
    X.thr[0] = a.x; X.thr[1] = a.y; X.thr[2] = a.z; X.thr[3] = a.w;
    X.lost[0] = c.x; X.lost[1] = c.y; X.lost[2] = c.z; X.lost[3] = c.w;
    X.key = b.x; X.n = b.y;
    X.nc = b.y * LOSS_STEP;
}

__device__ __forceinline__ void loss_store(const Loss& X, const GwCtrlLoss& x, int64_t e)
{
    x.rec[e * 6 + 3] = X.n;
    *reinterpret_cast<uint4*>(x.rec + e * 6 + 4) = make_uint4(X.lost[0], X.lost[1], X.lost[2], X.lost[3]);
}

// one draw: the mixer on key ^ (n * LOSS_STEP); the transmission is erased when the top 32 bits are below `thr`
__device__ __forceinline__ bool loss_draw(Loss& X, uint32_t thr)
{
    const uint64_t z = mix64(X.key ^ X.nc);
    X.n += 1ull;
    X.nc += LOSS_STEP;
    return (uint32_t)(z >> 32) < thr;
}

__device__ __forceinline__ uint32_t pick(const uint32_t (&a)[CR], int i)
{
    return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3]));
}

// Queue handling of one step.  The values a step appends (the sensor's sample of every tick: up to 22; the controller's
// command every `period` ticks) are staged in LDS, one column per lane, and written to the rings once, at the end of the
// step; the first PRE entries at the addressed queue's head are loaded before the walk.  A pop therefore never waits for
// memory inside the window loop (round 1: one dependent 8-byte load per transmission, one scattered 8-byte store per tick).
//   queue = the last `len` values of its append stream; this step's appends are the last `app` of it:
//   the head is a value of this step iff len <= app (then it is append number app - len).
constexpr int NEW0 = 24, NEW1 = 24, PRE = 8;

struct Q {                                                 // one queue during a step (scalars only: no dynamic indexing)
    uint32_t head, len, app, head0, tail0;
};

__device__ __forceinline__ void q_push(Q& q, double* s_col, double v)      // deque(maxlen=100): drop the oldest when full
{
    if (q.len == GW_QUEUE_CAP) { q.head = (q.head + 1u) & GW_RING_MASK; q.len--; }
    s_col[q.app << 6] = v;                                 // column of this lane: element j at [j * 64]
    q.app++;
    q.len++;
}

// a step's opening: nothing appended yet, and where the queue stood
__device__ __forceinline__ void q_open(Q& q)
{
    q.app = 0u;
    q.head0 = q.head;
    q.tail0 = (q.head + q.len) & GW_RING_MASK;
}

// this step's appends -> the ring: value j of the queue sits in slot (tail0 + j) & mask
__device__ __forceinline__ void q_flush(const Q& q, double* ring, const double* col)
{
    for (uint32_t j = 0; j < q.app; ++j) ring[(q.tail0 + j) & GW_RING_MASK] = col[j << 6];
}

// ---- the text every control-loop kernel is put together from ---------------------------------------------------------------------
// Macros, not functions: the same statements behind a __forceinline__ call came out of the compiler with other register numbers
// and another prologue schedule in some kernels and not in others (profiles/ctrl_one_text/README.md has the list), and a kernel
// that moves is a kernel to measure again.  Pasted as text, every kernel is instruction for instruction what it was when each
// restated these lines.  They name the kernel's own variables, as ctrl_step_body.h does:
//   c (GwCtrlDev), s (GwCtrlEpi, the reset only), g / w / x (GwCtrlPid / GwCtrlDist / GwCtrlLoss) and the variant's three
//   compile-time flags PID, DIST, LOSS (each implies the ones before it): a block whose flag is false is never read.

// A kernel's opening.  The two append columns (NEW0 + NEW1 values per lane) and the link tables -- the noise-state transitions
// and the BER per (listener, talker, state), looked up for every radio at every transmission -- go to LDS: a window of the
// sensor's queue is dozens of lookups, not a dependent global round trip apiece.  MORE is what else the block stages before the
// barrier (a schedule, a policy; may be empty).  Leaves e, the lane's env, with the lanes beyond N gone, and its two columns.
#define CTRL_KERNEL_OPEN(MORE)                                                                                                     \
    __shared__ double s_new0[NEW0 * 64], s_new1[NEW1 * 64];                                                                        \
    __shared__ uint8_t s_trans[CR * CR * S];                                                                                       \
    __shared__ double s_ber[CR * CR * S];                                                                                          \
    for (int i = threadIdx.x; i < CR * CR * S; i += blockDim.x) { s_trans[i] = c.trans[i]; s_ber[i] = c.ber[i]; }                  \
    MORE;                                                                                                                          \
    __syncthreads();                                                                                                               \
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;                                                              \
    if (e >= c.N) return;                                                                                                          \
    double* const col0 = s_new0 + (threadIdx.x & 63);                                                                              \
    double* const col1 = s_new1 + (threadIdx.x & 63)

// The lane's state <- GwCtrlDev and the variant's blocks, once per launch: declares k (the handle's constants by value through
// the constant address space: scalar loads the compiler may hoist and keep), L, q0 / q1, ring0 / ring1 and G, W, X.  OPEN is
// what stands behind the queues' load: in a step kernel their opening (q_open), which stood there in each restated copy --
// three statements further down it renumbers ctrl_step_loss_kernel's registers; in a lane loop, which opens them at every
// step, nothing -- opened here as well, dead stores and all, every fused kernel moved.
#define CTRL_LANE_LOAD(OPEN)                                                                                                       \
    const GwDevConst k = *(const GW_AS_CONST GwDevConst*)c.cst;                                                                    \
    Lane L;                                                                                                                        \
    L.now = c.now[e]; L.wake = c.wake[e]; L.u = c.u[e]; L.ang = c.ang[e]; L.ktick = c.ktick[e];                                    \
    for (int i = 0; i < 4; ++i) L.x[i] = c.x[e * 4 + i];                                                                           \
    Q q0, q1;                                                                                                                      \
    { const uint32_t hl = c.qhl[e]; q0.head = hl & 0xffu; q0.len = hl >> 8; }                                                      \
    { const uint32_t hl = c.qhl[c.N + e]; q1.head = hl & 0xffu; q1.len = hl >> 8; }                                                \
    OPEN;                                                                                                                          \
    _Pragma("unroll") for (int j = 0; j < CR; ++j) L.rxs[j] = c.rxs[j * c.N + e];                                                  \
    L.got1 = c.got[e * 2]; L.got2 = c.got[e * 2 + 1];                                                                              \
    L.ntx = c.ntx[e]; L.ncmd = c.ncmd[e]; L.nsub = c.nsub[e]; L.fl = c.flags[e];                                                   \
    double* ring0 = c.pay + ((size_t)e * 2 + 0) * GW_RING_PHYS;                                                                    \
    double* ring1 = c.pay + ((size_t)e * 2 + 1) * GW_RING_PHYS;                                                                    \
    Pid G;                                                                                                                         \
    if (PID) pid_load(G, g, e);                                                                                                    \
    Dist W;                                                                                                                        \
    if (DIST) dist_load(W, w, e);                                                                                                  \
    Loss X;                                                                                                                        \
    if (LOSS) loss_load(X, x, e)

// ... and back, once per launch (the rings were written step by step: q_flush)
#define CTRL_LANE_STORE()                                                                                                          \
    c.now[e] = L.now; c.wake[e] = L.wake; c.u[e] = L.u; c.ang[e] = L.ang; c.ktick[e] = L.ktick;                                    \
    for (int i = 0; i < 4; ++i) c.x[e * 4 + i] = L.x[i];                                                                           \
    c.qhl[e] = (uint16_t)(q0.head | (q0.len << 8));                                                                                \
    c.qhl[c.N + e] = (uint16_t)(q1.head | (q1.len << 8));                                                                          \
    _Pragma("unroll") for (int j = 0; j < CR; ++j) c.rxs[j * c.N + e] = (uint8_t)L.rxs[j];                                         \
    c.got[e * 2] = L.got1; c.got[e * 2 + 1] = L.got2;                                                                              \
    c.ntx[e] = L.ntx; c.ncmd[e] = L.ncmd; c.nsub[e] = L.nsub; c.flags[e] = L.fl

// The end of an episode inside a launch: the tally takes it, then gw_ctrl_reset for this one env, in registers -- its own
// initial state, empty queues, a fresh controller; flags are sticky, and the disturbance's and the loss's records go on
// counting (a reset env's plant draws where the old one stopped).  On the lane loop's own n_ended, n_failed, cost_ended, age,
// cost, at_sched and the cause just computed.
#define CTRL_LANE_RESET()                                                                                                          \
    n_ended++;                                                                                                                     \
    n_failed += cause >> 1;                                                                                                        \
    cost_ended = cost_ended + cost;                                                                                                \
    L.now = 0.0; L.wake = 0.0; L.ang = 0.0; L.ktick = 0u;                                                                          \
    for (int i = 0; i < 4; ++i) L.x[i] = s.x_init[e * 4 + i];                                                                      \
    L.u = s.u_init[e];                                                                                                             \
    q0.head = q0.len = 0u; q1.head = q1.len = 0u;                                                                                  \
    _Pragma("unroll") for (int j = 0; j < CR; ++j) L.rxs[j] = 0u;                                                                  \
    L.got1 = L.got2 = 0u;                                                                                                          \
    L.ntx = L.ncmd = L.nsub = 0u;                                                                                                  \
    age = 0u; cost = 0.0; at_sched = 0u;                                                                                           \
    if (PID) G.last = 0.0

} // namespace gwk

// ---- host side: which variant a handle launches ----------------------------------------------------------------------------------
inline int launched() { return hipGetLastError() == hipSuccess ? GW_OK : GW_EHIP; }

// One launch of a kernel family's variant: k0 (the default rule compiled in), kg (+ gains), kw (+ disturbance), kx (+ loss),
// picked by the blocks v carries.  Every variant takes its parent's arguments `a` and then its blocks, last and in that order.
template <class K0, class Kg, class Kw, class Kx, class... A>
int launch_variant(const GwCtrlBlocks& v, K0 k0, Kg kg, Kw kw, Kx kx, dim3 grid, void* stream, const A&... a)
{
    const dim3 block(64);
    if (v.x) hipLaunchKernelGGL(kx, grid, block, 0, (hipStream_t)stream, a..., *v.g, *v.w, *v.x);
    else if (v.w) hipLaunchKernelGGL(kw, grid, block, 0, (hipStream_t)stream, a..., *v.g, *v.w);
    else if (v.g) hipLaunchKernelGGL(kg, grid, block, 0, (hipStream_t)stream, a..., *v.g);
    else hipLaunchKernelGGL(k0, grid, block, 0, (hipStream_t)stream, a...);
    return launched();
}
