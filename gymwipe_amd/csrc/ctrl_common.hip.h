// ctrl_common.hip.h -- what the control-loop kernels share: ctrl_step_kernel (ctrl_step.hip: one step per launch) and the fused
// kernels of ctrl_rollout.hip (K steps per launch).  A lane's state, its two queues during a step, and the staging of a step's
// appends, the controller's gains where a kernel reads them, the plant's disturbance where a kernel draws it, and the links'
// packet erasures where a kernel draws them.  The step itself is text: ctrl_step_body.h.
#pragma once
#include "ct_common.hip.h"

namespace gwk {

constexpr int CR = 4, CRRM = 3;                             // radios (3 network devices + RRM), index of the RRM

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

// one draw: the mixer of gw_policy_u (ct_rollout_sync.hip.h) on key ^ (n * DIST_STEP), its top 32 bits as a signed integer
// times 2^-31 -- uniform on [-1, 1), a multiple of 2^-31, every operation exact
__device__ __forceinline__ double dist_draw(Dist& W)
{
    uint64_t z = (W.key ^ W.nc) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
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

// one draw: dist_draw's mixer on key ^ (n * LOSS_STEP); the transmission is erased when the top 32 bits are below `thr`
__device__ __forceinline__ bool loss_draw(Loss& X, uint32_t thr)
{
    uint64_t z = (X.key ^ X.nc) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
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

} // namespace gwk
