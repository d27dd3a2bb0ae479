// gw_ctrl_api.cpp -- C-ABI of the closed control loop (include/gymwipe_amd.h, "Control loop"): host side.
#include "gw_internal.h"

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>

int gw_set_error(int code, const char* fmt, ...);      // gw_api.cpp

struct gw_ctrl {
    gw_ctrl_config cfg;
    GwHostTables tab;
    GwCtrlDev dev;
    GwCtrlEpi epi;                     // per-env initial state and episode record (not part of the step kernel's argument)
    GwCtrlPid pid;                     // per-env gains and last error: {1, 0, 0, 0} from gw_ctrl_create on
    bool pid_on;                       // gw_ctrl_set_gains has been called: the launches take the PID instantiations, for good
    GwCtrlDist dist;                   // per-env plant disturbance {g[4], key, n}: all 0 from gw_ctrl_create on
    bool dist_on;                      // gw_ctrl_set_disturbance has been called: the disturbance instantiations, for good (pid_on too)
    GwCtrlLoss loss;                   // per-env packet erasures {thr[4], key, n, lost[4]}: all 0 from gw_ctrl_create on
    bool loss_on;                      // gw_ctrl_set_loss has been called: the loss instantiations, for good (dist_on and pid_on too)
    void* blocks[32];
    int nblocks;
};

namespace {

#define CTRL_HIP(expr, cleanup)                                                                   \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            cleanup;                                                                              \
            return gw_set_error(GW_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e));          \
        }                                                                                         \
    } while (0)

template <class T>
int calloc_dev(gw_ctrl* c, T** out, size_t count)
{
    void* q = nullptr;
    if (c->nblocks >= (int)(sizeof c->blocks / sizeof c->blocks[0]) || hipMalloc(&q, count * sizeof(T)) != hipSuccess)
        return gw_set_error(GW_ENOMEM, "hipMalloc failed in gw_ctrl_create");
    c->blocks[c->nblocks++] = q;
    *out = (T*)q;
    return GW_OK;
}

// the launchers' variant argument: the blocks of the switches that have been set on the handle (each sets the ones before it)
inline GwCtrlBlocks blocks_of(const gw_ctrl* c)
{
    GwCtrlBlocks v = {nullptr, nullptr, nullptr};
    if (c->pid_on) v.g = &c->pid;
    if (c->dist_on) v.w = &c->dist;
    if (c->loss_on) v.x = &c->loss;
    return v;
}

} // namespace

extern "C" {

int gw_ctrl_config_default(gw_ctrl_config* c, int64_t num_envs)
{
    if (!c) return gw_set_error(GW_EINVAL, "cfg is NULL");
    memset(c, 0, sizeof *c);
    int rc = gw_config_default(&c->net, num_envs, 3);
    if (rc) return rc;
    // envs/inverted_pendulum.py:75-93: controller at (0, -1), RRM at (0, 1), sensor and actuator on the wagon.  The
    // actuator sits half a metre along the wagon here: two co-located radios would keep the reference's "attenuation 0".
    c->net.pos[0][0] = 0.0; c->net.pos[0][1] = 0.0;
    c->net.pos[1][0] = 0.0; c->net.pos[1][1] = -1.0;
    c->net.pos[2][0] = 0.5; c->net.pos[2][1] = 0.0;
    c->net.pos[3][0] = 0.0; c->net.pos[3][1] = 1.0;
    c->net.mult[0] = 1; c->net.mult[1] = 0; c->net.mult[2] = 0;
    c->net.dest[0] = 1; c->net.dest[1] = 2; c->net.dest[2] = 0;
    gw_plant_config pc;
    rc = gw_plant_config_default(&pc, num_envs);
    if (rc) return rc;
    memcpy(c->A, pc.A, sizeof c->A);
    for (int i = 0; i < 4; ++i) { c->B[i] = -pc.B[i]; c->x0[i] = pc.x0[i]; }   // input sign: the reference's control law (u = -angle) damps
    c->u0 = pc.u0;
    c->ctrl_start_tick = 20;
    c->ctrl_period_ticks = 10;                  // 10 ms, control/inverted_pendulum.py:69
    return GW_OK;
}

int gw_ctrl_destroy(gw_ctrl* c)
{
    if (!c) return GW_OK;
    (void)hipSetDevice(c->cfg.net.hip_device);
    for (int i = 0; i < c->nblocks; ++i) (void)hipFree(c->blocks[i]);
    delete c;
    return GW_OK;
}

int gw_ctrl_create(const gw_ctrl_config* cfg, gw_ctrl** out)
{
    if (!cfg || !out) return gw_set_error(GW_EINVAL, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->net.num_devices != 3) return gw_set_error(GW_EINVAL, "the control loop has three network devices (sensor, controller, actuator)");
    if (cfg->ctrl_period_ticks < 1 || cfg->ctrl_start_tick < 0) return gw_set_error(GW_EINVAL, "ctrl_start_tick / ctrl_period_ticks out of range");
    int rc = gw_validate_config(cfg->net);
    if (rc) return rc;
    {
        // the step kernel stages a step's queue appends in LDS, 24 per queue: a step must not contain more counter ticks
        const double step_max = ((double)(cfg->net.max_duration - 1) * cfg->net.duration_factor + 3.0) * cfg->net.slot
                                + (double)(cfg->net.mac_header_bytes + 16) * 8.0 / (cfg->net.code_rate * cfg->net.bit_rate);
        if (step_max / cfg->net.counter_interval + 2.0 > 24.0)
            return gw_set_error(GW_EUNSUPPORTED, "more than 24 counter ticks can fall into one step with this duration range / counter interval");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return gw_set_error(GW_ENODEVICE, "no HIP device available (this library has no CPU fallback)");
    if (cfg->net.hip_device < 0 || cfg->net.hip_device >= ndev) return gw_set_error(GW_EINVAL, "hip_device out of range");
    gw_ctrl* c = new (std::nothrow) gw_ctrl();
    if (!c) return gw_set_error(GW_ENOMEM, "out of host memory");
    memset(c, 0, sizeof *c);
    c->cfg = *cfg;
    char msg[256] = "";
    rc = gw_build_tables(c->cfg.net, c->tab, msg, sizeof msg);
    if (!rc && c->tab.overflow) rc = GW_EUNSUPPORTED;        // (the control-loop kernel keeps the byte noise states)
    if (rc) { delete c; return gw_set_error(rc, "%s", msg); }
    CTRL_HIP(hipSetDevice(cfg->net.hip_device), delete c);
    GwDevConst k;
    memset(&k, 0, sizeof k);
    gw_fill_dev_const(c->cfg.net, c->tab, k);
    const int64_t N = cfg->net.num_envs;
    const int R = 4;
    GwCtrlDev& d = c->dev;
    d.N = N;
    memcpy(d.A, cfg->A, sizeof d.A);
    memcpy(d.B, cfg->B, sizeof d.B);
    d.start = (uint32_t)cfg->ctrl_start_tick;
    d.period = (uint32_t)cfg->ctrl_period_ticks;
    GwDevConst* d_cst = nullptr; uint8_t* d_trans = nullptr; double* d_ber = nullptr;
    const size_t tcount = (size_t)R * R * GW_MAX_NSTATES;
#define CA(ptr, cnt) do { rc = calloc_dev(c, &(ptr), (size_t)(cnt)); if (rc) { gw_ctrl_destroy(c); return rc; } } while (0)
    CA(d.now, N); CA(d.wake, N); CA(d.x, N * 4); CA(d.u, N); CA(d.ang, N);
    CA(d.ktick, N); CA(d.got, N * 2); CA(d.ntx, N); CA(d.ncmd, N); CA(d.nsub, N); CA(d.flags, N);
    CA(d.qhl, N * 2); CA(d.rxs, N * R); CA(d.pay, N * 2 * GW_RING_PHYS);
    CA(d_cst, 1); CA(d_trans, tcount); CA(d_ber, tcount);
    CA(c->epi.x_init, N * 4); CA(c->epi.u_init, N); CA(c->epi.cost, N); CA(c->epi.age, N);
    CA(c->pid.pid, N * 4);
    CA(c->dist.rec, N * 6);
    CA(c->loss.rec, N * 6);
#undef CA
    d.cst = d_cst; d.trans = d_trans; d.ber = d_ber;
    CTRL_HIP(hipMemcpy(d_cst, &k, sizeof k, hipMemcpyHostToDevice), gw_ctrl_destroy(c));
    CTRL_HIP(hipMemcpy(d_trans, c->tab.trans, tcount, hipMemcpyHostToDevice), gw_ctrl_destroy(c));
    CTRL_HIP(hipMemcpy(d_ber, c->tab.ber, tcount * sizeof(double), hipMemcpyHostToDevice), gw_ctrl_destroy(c));
    CTRL_HIP(hipMemset(d.pay, 0, (size_t)N * 2 * GW_RING_PHYS * sizeof(double)), gw_ctrl_destroy(c));
    CTRL_HIP(hipMemset(c->dist.rec, 0, (size_t)N * 6 * sizeof(uint64_t)), gw_ctrl_destroy(c));    // g = 0, key = 0, n = 0
    CTRL_HIP(hipMemset(c->loss.rec, 0, (size_t)N * 6 * sizeof(uint64_t)), gw_ctrl_destroy(c));    // thr = 0, key = 0, n = 0, lost = 0
    {
        const double def[4] = {1.0, 0.0, 0.0, 0.0};          // the reference's shipped gains, and a fresh controller's last error
        std::vector<double> fill((size_t)N * 4);
        for (size_t i = 0; i < fill.size(); ++i) fill[i] = def[i & 3];
        CTRL_HIP(hipMemcpy(c->pid.pid, fill.data(), fill.size() * sizeof(double), hipMemcpyHostToDevice), gw_ctrl_destroy(c));
    }
    if (gw_ctrl_launch_init(d, cfg->x0, cfg->u0, nullptr) || gw_ctrl_launch_fill_initial(d, c->epi, cfg->x0, cfg->u0, nullptr)) {
        gw_ctrl_destroy(c);
        return gw_set_error(GW_EHIP, "control-loop init launch failed");
    }
    CTRL_HIP(hipDeviceSynchronize(), gw_ctrl_destroy(c));
    *out = c;
    return GW_OK;
}

int gw_ctrl_step(gw_ctrl* c, const int32_t* device_dev, const int32_t* duration_dev, int32_t* obs_dev, float* reward_dev,
                 double* angle_deg_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!device_dev || !duration_dev || !obs_dev || !reward_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_step: NULL device pointer");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_step(c->dev, blocks_of(c), device_dev, duration_dev, obs_dev, reward_dev, angle_deg_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop step launch failed");
    return GW_OK;
}

int gw_ctrl_set_initial(gw_ctrl* c, const double* x0_dev, const double* u0_dev, const uint8_t* mask_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!x0_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_initial: x0_dev is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_set_initial(c->dev, c->epi, x0_dev, u0_dev, mask_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop set_initial launch failed");
    return GW_OK;
}

int gw_ctrl_set_gains(gw_ctrl* c, const double* gains_dev, const uint8_t* mask_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!gains_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_gains: gains_dev is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_set_gains(c->dev, c->pid, gains_dev, mask_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop set_gains launch failed");
    c->pid_on = true;
    return GW_OK;
}

int gw_ctrl_set_disturbance(gw_ctrl* c, const double* g_dev, const uint64_t* key_dev, const uint8_t* mask_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!g_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_disturbance: g_dev is NULL");
    if (!key_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_disturbance: key_dev is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_set_disturbance(c->dev, c->dist, g_dev, key_dev, mask_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop set_disturbance launch failed");
    c->dist_on = true;                 // the disturbance instantiations are PID instantiations: a reset clears last_error
    c->pid_on = true;                  // from here on, as on a handle that has set gains
    return GW_OK;
}

int gw_ctrl_set_loss(gw_ctrl* c, const uint32_t* thr_dev, const uint64_t* key_dev, const uint8_t* mask_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!thr_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_loss: thr_dev is NULL");
    if (!key_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_set_loss: key_dev is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_set_loss(c->dev, c->loss, thr_dev, key_dev, mask_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop set_loss launch failed");
    c->loss_on = true;                 // the loss instantiations are disturbance and PID instantiations: the plant runs the
    c->dist_on = true;                 // disturbance rule at the g last stored (0 if never) and a reset clears last_error
    c->pid_on = true;                  // from here on
    return GW_OK;
}

int gw_ctrl_reset(gw_ctrl* c, const uint8_t* mask_dev, int32_t* obs_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_reset(c->dev, c->epi, blocks_of(c), mask_dev, obs_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop reset launch failed");
    return GW_OK;
}

int gw_ctrl_rollout(gw_ctrl* c, int32_t steps, const int32_t* device_dev, const int32_t* duration_dev, const gw_ctrl_episodes* ep,
                    int32_t* obs_dev, float* reward_dev, double* angle_deg_dev, uint8_t* ended_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!device_dev || !duration_dev || !obs_dev || !reward_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout: NULL device pointer");
    if (ep && !ended_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout: ended_dev is NULL (required with episodes)");
    if (ep && ep->max_steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout: max_steps < 0");
    if (steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout: steps < 0");
    if (steps == 0) return GW_OK;
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_rollout(c->dev, c->epi, blocks_of(c), steps, device_dev, duration_dev, ep, obs_dev, reward_dev, angle_deg_dev, ended_dev,
                               stream))
        return gw_set_error(GW_EHIP, "control-loop rollout launch failed");
    return GW_OK;
}

int gw_ctrl_rollout_schedules(gw_ctrl* c, int32_t steps, const uint8_t* sched_dev, int32_t P, int32_t L, const gw_ctrl_episodes* ep,
                              double* tally_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!sched_dev || !tally_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: NULL device pointer");
    if (!ep) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: ep is NULL (episodes are required)");
    if (ep->max_steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: max_steps < 0");
    if (steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: steps < 0");
    if (P < 1) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: P must be >= 1");
    if (L < 1 || L > 64) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_schedules: L must be in [1, 64]");
    if (steps == 0) return GW_OK;
    const int64_t N = c->dev.N;
    if (N % P != 0 || (N / P) % 64 != 0)
        return gw_set_error(GW_EUNSUPPORTED, "gw_ctrl_rollout_schedules: num_envs / P must be a whole multiple of 64 (one schedule per block)");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_rollout_schedules(c->dev, c->epi, blocks_of(c), steps, sched_dev, P, L, *ep, tally_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop schedule rollout launch failed");
    return GW_OK;
}

int gw_ctrl_rollout_feedback(gw_ctrl* c, int32_t steps, const gw_ctrl_feedback* fb, const gw_ctrl_episodes* ep,
                             const gw_ctrl_feedback_rows* rows, double* tally_dev, void* stream)
{
    if (!c) return gw_set_error(GW_EINVAL, "handle is NULL");
    if (!fb) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: fb is NULL");
    if (!ep) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: ep is NULL (episodes are required)");
    if (!tally_dev || !fb->sched_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: NULL device pointer");
    if (ep->max_steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: max_steps < 0");
    if (steps < 0) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: steps < 0");
    if (fb->num_policies < 1) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: P must be >= 1");
    if (fb->num_bins < 1 || fb->num_bins > GW_CTRL_FB_MAX_BINS)
        return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: B must be in [1, %d]", GW_CTRL_FB_MAX_BINS);
    if (fb->length < 1 || fb->length > 64) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: L must be in [1, 64]");
    if (fb->num_bins > 1 && !fb->edges_dev) return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: edges_dev is NULL with B > 1");
    if (rows && (!rows->device_out_dev || !rows->duration_out_dev || !rows->obs_dev || !rows->reward_dev || !rows->ended_dev))
        return gw_set_error(GW_EINVAL, "gw_ctrl_rollout_feedback: NULL pointer in rows (only angle_deg_dev may be NULL)");
    if (steps == 0) return GW_OK;
    const int64_t N = c->dev.N;
    const int32_t P = fb->num_policies;
    if (N % P != 0 || (N / P) % 64 != 0)
        return gw_set_error(GW_EUNSUPPORTED, "gw_ctrl_rollout_feedback: num_envs / P must be a whole multiple of 64 (one policy per block)");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    if (gw_ctrl_launch_rollout_feedback(c->dev, c->epi, blocks_of(c), steps, *fb, *ep, rows, tally_dev, stream))
        return gw_set_error(GW_EHIP, "control-loop feedback rollout launch failed");
    return GW_OK;
}

int gw_ctrl_get_state(gw_ctrl* c, const char* field, void* dst, size_t bytes)
{
    if (!c || !field || !dst) return gw_set_error(GW_EINVAL, "handle/field/dst is NULL");
    CTRL_HIP(hipSetDevice(c->cfg.net.hip_device), (void)0);
    CTRL_HIP(hipDeviceSynchronize(), (void)0);
    const GwCtrlDev& d = c->dev;
    const int64_t N = d.N;
    const void* src = nullptr; size_t need = 0;
    if (!strcmp(field, "now")) { src = d.now; need = N * sizeof(double); }
    else if (!strcmp(field, "wake")) { src = d.wake; need = N * sizeof(double); }
    else if (!strcmp(field, "x")) { src = d.x; need = N * 4 * sizeof(double); }
    else if (!strcmp(field, "u")) { src = d.u; need = N * sizeof(double); }
    else if (!strcmp(field, "angle_deg")) { src = d.ang; need = N * sizeof(double); }
    else if (!strcmp(field, "received")) { src = d.got; need = N * 2 * sizeof(uint32_t); }
    else if (!strcmp(field, "n_tx")) { src = d.ntx; need = N * sizeof(uint32_t); }
    else if (!strcmp(field, "commands")) { src = d.ncmd; need = N * sizeof(uint32_t); }
    else if (!strcmp(field, "substeps")) { src = d.nsub; need = N * sizeof(uint32_t); }
    else if (!strcmp(field, "flags")) { src = d.flags; need = N * sizeof(uint32_t); }
    else if (!strcmp(field, "age")) { src = c->epi.age; need = N * sizeof(uint32_t); }
    else if (!strcmp(field, "cost")) { src = c->epi.cost; need = N * sizeof(double); }
    else if (!strcmp(field, "x_init")) { src = c->epi.x_init; need = N * 4 * sizeof(double); }
    else if (!strcmp(field, "u_init")) { src = c->epi.u_init; need = N * sizeof(double); }
    if (src) {
        if (bytes != need) return gw_set_error(GW_EFIELD, "field %s needs %zu bytes, got %zu", field, need, bytes);
        CTRL_HIP(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost), (void)0);
        return GW_OK;
    }
    if (!strcmp(field, "qlen")) {                          // int32[N][2]: sensor, controller
        if (bytes != (size_t)N * 2 * sizeof(int32_t)) return gw_set_error(GW_EFIELD, "field qlen needs %zu bytes", (size_t)N * 2 * sizeof(int32_t));
        std::vector<uint16_t> hl((size_t)N * 2);
        CTRL_HIP(hipMemcpy(hl.data(), d.qhl, hl.size() * sizeof(uint16_t), hipMemcpyDeviceToHost), (void)0);
        for (int64_t e = 0; e < N; ++e) for (int q = 0; q < 2; ++q) ((int32_t*)dst)[e * 2 + q] = hl[(size_t)q * N + e] >> 8;
        return GW_OK;
    }
    if (!strcmp(field, "gains") || !strcmp(field, "last_error")) {     // f64[N][3] / f64[N]: columns of the {kp, ki, kd, last_error} block
        const bool gains = field[0] == 'g';
        const size_t cols = gains ? 3 : 1;
        if (bytes != (size_t)N * cols * sizeof(double)) return gw_set_error(GW_EFIELD, "field %s needs %zu bytes", field, (size_t)N * cols * sizeof(double));
        CTRL_HIP(hipMemcpy2D(dst, cols * sizeof(double), c->pid.pid + (gains ? 0 : 3), 4 * sizeof(double), cols * sizeof(double), (size_t)N,
                             hipMemcpyDeviceToHost), (void)0);
        return GW_OK;
    }
    if (!strcmp(field, "disturbance") || !strcmp(field, "noise_key") || !strcmp(field, "noise_count")) {
        // f64[N][4] / u64[N] / u64[N]: columns of the {g[4], key, n} records
        const size_t cols = field[0] == 'd' ? 4 : 1, first = field[0] == 'd' ? 0 : (field[6] == 'k' ? 4 : 5);
        if (bytes != (size_t)N * cols * 8) return gw_set_error(GW_EFIELD, "field %s needs %zu bytes", field, (size_t)N * cols * 8);
        CTRL_HIP(hipMemcpy2D(dst, cols * 8, c->dist.rec + first, 6 * 8, cols * 8, (size_t)N, hipMemcpyDeviceToHost), (void)0);
        return GW_OK;
    }
    if (!strcmp(field, "loss") || !strcmp(field, "loss_key") || !strcmp(field, "loss_count") || !strcmp(field, "lost")) {
        // u32[N][4] / u64[N] / u64[N] / u32[N][4]: columns of the {thr[4], key, n, lost[4]} records
        const bool wide = !field[4];
        const size_t width = wide ? 16 : 8, first = !strcmp(field, "loss") ? 0 : (field[3] == 't' ? 32 : (field[5] == 'k' ? 16 : 24));
        if (bytes != (size_t)N * width) return gw_set_error(GW_EFIELD, "field %s needs %zu bytes", field, (size_t)N * width);
        CTRL_HIP(hipMemcpy2D(dst, width, (const char*)c->loss.rec + first, 48, width, (size_t)N, hipMemcpyDeviceToHost), (void)0);
        return GW_OK;
    }
    if (!strcmp(field, "rx_power")) {                      // f64[N][4]
        if (bytes != (size_t)N * 4 * sizeof(double)) return gw_set_error(GW_EFIELD, "field rx_power needs %zu bytes", (size_t)N * 4 * sizeof(double));
        std::vector<uint8_t> s((size_t)N * 4);
        CTRL_HIP(hipMemcpy(s.data(), d.rxs, s.size(), hipMemcpyDeviceToHost), (void)0);
        for (int64_t e = 0; e < N; ++e) for (int r = 0; r < 4; ++r) ((double*)dst)[e * 4 + r] = c->tab.state_val[r][s[(size_t)r * N + e]];
        return GW_OK;
    }
    return gw_set_error(GW_EFIELD, "unknown control-loop field %s", field);
}

} // extern "C"
