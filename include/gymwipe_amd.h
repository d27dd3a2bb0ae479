/*
 * gymwipe_amd.h -- C-ABI of the MI355X-native vectorised Gym-WiPE env.step().
 *
 * Drop-in boundary for ONE path of the reference (Gryph66/gymwipe): the
 * discrete-event advance behind the frequency-band-assignment environment
 * `CounterTrafficEnv` (gymwipe/envs/counter_traffic.py).  N independent
 * environments live structure-of-arrays in HBM and are advanced by hand-written
 * HIP kernels for gfx950.  There is NO CPU fallback in this library: every
 * compute entry point needs a HIP device and fails loudly without one.
 *
 * Conventions
 *   - every function returns 0 on success or a negative GW_E* code;
 *     gw_last_error() returns a thread-local message for the last failure
 *   - `*_dev` pointers are DEVICE pointers owned by the caller (e.g. torch
 *     tensors), contiguous, length num_envs unless stated; `stream` is a
 *     hipStream_t passed as void* (NULL = default stream); gw_step/gw_reset are
 *     asynchronous on that stream and allocate nothing
 *   - one gw_env per GPU; a handle is not thread-safe; different handles may be
 *     driven from different host threads
 *
 * Reference interface each entry point replaces (file:line in the reference):
 *   gw_config_default  class constants: envs/core.py:25,27; counter_traffic.py:31-35,124-127;
 *                      simple_stack.py:27,57,361,364; physical.py:192-197,298; messages.py:154,180
 *   gw_create          CounterTrafficEnv.__init__            counter_traffic.py:114-133
 *   gw_reset           CounterTrafficEnv.reset               counter_traffic.py:135-144
 *   gw_step            CounterTrafficEnv.step                counter_traffic.py:146-158
 *                        -> SimpleRrmDevice.assignFrequencyBand   networking/devices.py:178-203
 *                        -> SimMan.runSimulation(eProcessed)      simtools.py:77-88
 *                        -> Interpreter.getFeedback               envs/core.py:142-153
 *   gw_set_position(s) Position.set -> PositionalAttenuationModel -> FsplAttenuation   devices/core.py:52-86, physical.py:380-386,
 *                      attenuation_models.py:28-36
 *   gw_received        CounterTrafficInterpreter.receivedValues / getInfo   counter_traffic.py:72,109-112
 *   gw_get_state       attribute reads the reference's tests perform: SimMan.now, sender.counter,
 *                      sender._mac._packetQueue, phy._receivedPower
 *   gw_delivered       what SimpleRrmDevice.onPacketReceived feeds a custom Interpreter     networking/devices.py:163-168
 *   gw_enqueue         SimpleNetworkDevice.send -> SimpleMac queue           networking/devices.py:84-86, simple_stack.py:463-471
 *   gw_rollout         a Python loop over step()
 *   gw_rollout_autoreset   that loop with the caller's reset on done or after nb_max_episode_steps (keras-rl's fit, as the
 *                      reference drives it: agents/dqn_counter_traffic.py:63-70); steps = 1 is one env.step() with autoreset
 *   gw_rollout_episodes_scored / gw_rollout_population_scored   the closed loops with a custom Interpreter's getReward in
 *                      place of the built-in one: a weighted sum of the step's reward and of the packets the RRM sniffed
 *                      (envs/core.py:59-159, networking/devices.py:163-168)
 *   gw_rollout_autoreset_scored   keras-rl's fit loop (gw_rollout_autoreset) around an env with such a custom Interpreter: the
 *                      caller's actions, the launch's resets, the score as the reward the agent remembers
 *   gw_rollout_backlog (builder-defined: the reference's RRM cannot read sender._mac._packetQueue) that loop with a genie
 *                      scheduler in the RRM's place, which assigns the band to the longest queue -- a baseline, not a reference path
 *   gw_rollout_backlog_population   (builder-defined) the search that tunes that scheduler per configuration: P of its policies
 *                      on num_envs / P envs each, ranked by their episode tallies
 *   gw_step_fb         gw_step + the step's feedback as one byte per env (the row a multi-GPU job gathers)
 *   gw_pack_feedback / gw_unpack_feedback   (multi-GPU exchange format; the reference is single-process)
 *   gw_pendulum_step   InvertedPendulumEnv.step              envs/inverted_pendulum.py:101-113
 *   gw_plant_*         OdePlant.updateState, SlidingPendulum getters / setMotorVelocity   plants/core.py:38-49,
 *                      plants/sliding_pendulum.py:57-85   (builder-defined linear plant)
 *   gw_grid_*          SimMan.runSimulation(seconds) over the benchmark fixture, Position.set
 *                      tests/test_benchmark.py:20-91, devices/core.py:77-86
 *   gw_destroy         (garbage collection)
 */
#ifndef GYMWIPE_AMD_H
#define GYMWIPE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_ABI_VERSION   1

#define GW_MAX_DEVICES   32                 /* assignable senders per env */
#define GW_MAX_RADIOS    (GW_MAX_DEVICES + 1)
#define GW_QUEUE_CAP     100                /* simple_stack.py:361 deque(maxlen=100) */

/* error codes */
#define GW_OK             0
#define GW_EINVAL        -1                 /* bad argument / config */
#define GW_ENODEVICE     -2                 /* no usable HIP device */
#define GW_EHIP          -3                 /* HIP runtime error (message has details) */
#define GW_ENOMEM        -4
#define GW_EUNSUPPORTED  -5                 /* config outside what the kernels model */
#define GW_EFIELD        -6                 /* unknown gw_get_state field / size mismatch */

/* per-env sticky flag bits (gw_get_state "flags"; OR over envs in gw_stats) */
#define GW_FLAG_CARRY    1u   /* a transmission would outlive its step: horizon not closed */
#define GW_FLAG_REFEXC   2u   /* the reference would raise here (simple_stack.py:166 KeyError) */
#define GW_FLAG_TIE      4u   /* an exact f64 time tie was resolved by the insertion-order rule */
#define GW_FLAG_BADACT   8u   /* action outside the action space: env left untouched this step */
#define GW_FLAG_INTERNAL 16u  /* a kernel self-check of an exact fast path failed (never expected; the env's state is invalid) */

typedef struct gw_config {
    int32_t abi_version;                    /* GW_ABI_VERSION */
    int32_t hip_device;                     /* device ordinal */
    int64_t num_envs;                       /* N */
    int32_t num_devices;                    /* D senders; radio index D is the RRM */
    int32_t flags;                          /* GW_CFG_* */
    double  pos[GW_MAX_RADIOS][2];          /* metres; [D] = RRM */
    int32_t mult[GW_MAX_DEVICES];           /* packets per counter tick (packetMultiplicity); 0 = a sender with nothing to send */
    int32_t dest[GW_MAX_DEVICES];           /* destination sender index */
    double  slot;                           /* TIME_SLOT_LENGTH 1e-6 s */
    double  frequency;                      /* 2.4e9 Hz */
    double  bandwidth;                      /* 22e6 Hz */
    double  temperature_c;                  /* 20.0 */
    double  bit_rate;                       /* 133.33333e3 bps */
    double  code_rate;                      /* 3/4 */
    double  max_ber;                        /* 0.25 (Varshamov-Gilbert bound for 3/4) */
    double  tx_power_dbm;                   /* 0.0 */
    double  counter_interval;               /* COUNTER_INTERVAL 1e-3 s */
    int32_t counter_bound;                  /* COUNTER_BOUND 65536 */
    int32_t payload_value;                  /* 2: value field of every data payload (swapped ctor args) */
    int32_t mac_header_bytes;               /* 13 */
    int32_t net_header_bytes;               /* 12 */
    int32_t duration_factor;                /* ASSIGNMENT_DURATION_FACTOR 1000 */
    int32_t max_duration;                   /* MAX_ASSIGN_DURATION 20 */
    /* Custom attenuation models (AttenuationModelFactory.setCustomModels + JoinedAttenuationModel, physical.py:402-457,
     * 477-498): geometry is static here, so the models a caller sets for a device pair reduce to one number, the sum of
     * their attenuations in dB, which the joined model adds to the free-space term (sum() over [FSPL, custom...]).
     * Must be symmetric; 0 = the pair keeps the plain FSPL model. */
    double  extra_att_db[GW_MAX_RADIOS][GW_MAX_RADIOS];
    /* Simulated time at creation (the reference always starts at 0: SimMan.init).  A test hook: the clock and the first
     * counter tick start here, which puts the f64 arithmetic of the step (slot remainders, tick sums, decode sums) into
     * the coarser binades a run reaches only after ~10^8 steps, and past the limits of the validated fast paths. */
    double  start_time;
} gw_config;

#define GW_CFG_PER_ENV_STATS  1             /* explicit-queue mode only: keep per-env event counters (the default
                                               mode always keeps them, as 32-bit counters that wrap) */
#define GW_CFG_EXPLICIT_QUEUE 2             /* MAC queues as deques of packet-size runs that hold ANY traffic (generic kernel,
                                               gw_runq.h); default: exact suffix encoding of counter traffic, gw_queue.h */

/* The three flags below widen the path towards the callers SURVEY 8f ranks next (receive-mode MACs and
 * traffic other than counters); they need GW_CFG_EXPLICIT_QUEUE.  Together they replay the reference's
 * test_simple_mac (tests/networking/test_stack.py:134-235). */
#define GW_CFG_NO_COUNTER_TRAFFIC 4         /* no counter processes: packets come from gw_enqueue only */
#define GW_CFG_PEER_RECEIVE   8             /* `device.receiving = True` on every sender (networking/devices.py:71-111: a
                                               RECEIVE command re-issued on completion, as test_stack.py:176-186 does by
                                               hand; SimpleMac side simple_stack.py:435-444,453-461,473-484): data packets
                                               decoded at dest[d] while it is idle are handed up and counted
                                               ("peer_received") */
#define GW_CFG_FLOAT_DURATION 16            /* the assignment duration is passed as a float (test_stack.py:197):
                                               the announcement payload is len(str(float(slots))) bytes */

#define GW_CFG_PER_ENV_GEOMETRY 32          /* positions per ENVIRONMENT (either queue mode): every env starts with cfg.pos and
                                               gw_set_position(s) moves radios between steps -- Position.set,
                                               devices/core.py:52-86; link powers per env, rebuilt on the device (ct_step_dyn.hip) */

typedef struct gw_stats {                   /* totals since gw_create, over all envs */
    uint64_t steps;                         /* env-steps executed */
    uint64_t transmissions;                 /* announcements + data packets */
    uint64_t delivered;                     /* data packets decoded by the RRM */
    uint64_t appended;                      /* queue appends  (k_app of SURVEY 8d) */
    uint64_t popped;                        /* queue pops     (k_pop) */
    uint64_t dropped;                       /* drop-oldest events */
    uint64_t flags_or;                      /* OR of all per-env flag words */
    uint64_t bad_actions;                   /* env-steps skipped for an invalid action */
} gw_stats;

typedef struct gw_env gw_env;

int         gw_abi_version(void);
const char* gw_last_error(void);
int         gw_device_count(int* count);

int gw_config_default(gw_config* cfg, int64_t num_envs, int32_t num_devices);

int gw_create(const gw_config* cfg, gw_env** out);
int gw_destroy(gw_env* env);

/* reset(): counters <- 0, interpreter <- 0, simulated time NOT rewound.
 * mask_dev: NULL = all envs, else uint8[N] (non-zero = reset).  obs_dev may be NULL. */
int gw_reset(gw_env* env, const uint8_t* mask_dev, int32_t* obs_dev, void* stream);

/* one env.step() for all N envs.  device_dev in [0,D), duration_dev in [0,max_duration). */
int gw_step(gw_env* env, const int32_t* device_dev, const int32_t* duration_dev,
            int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);

/* gw_step that ALSO writes the step's feedback in the one-byte exchange format of gw_pack_feedback (below) to
 * feedback_byte_dev[N] -- the row a multi-GPU job all-gathers at the end of the step (Interpreter.getFeedback, envs/core.py:142-153,
 * in the form the gather moves).  Fused into the step kernel in the default mode (one more byte stored per env, no extra launch);
 * the other modes run gw_step and then the packing kernel.  feedback_byte_dev == NULL: exactly gw_step. */
int gw_step_fb(gw_env* env, const int32_t* device_dev, const int32_t* duration_dev,
               int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, uint8_t* feedback_byte_dev, void* stream);

/* SimpleNetworkDevice.send(data, dest[sender]) (networking/devices.py:84-86) -> SimpleMac queue append with
 * drop-oldest (simple_stack.py:463-471), for every env with payload_bytes_dev[e] >= 0 (int32[N]: byte size of
 * the network payload; headers are added).  GW_CFG_EXPLICIT_QUEUE only. */
int gw_enqueue(gw_env* env, int32_t sender, const int32_t* payload_bytes_dev, void* stream);

/* One byte per env-step for the end-of-step observation gather of a multi-GPU job: bits 0-1 sign(obs - COUNTER_BOUND) + 1,
 * bits 2-6 reward + 10, bit 7 done -- lossless for the built-in interpreter (counter_traffic.py:85-112, envs/core.py:142-153),
 * 9x less xGMI traffic than the (int32, float32, uint8) triple.  `count` elements in any layout (e.g. [steps][N]).
 * gw_pack_feedback fails with GW_EINVAL (synchronously, it reads a flag back) if a value is not representable, i.e. the
 * buffers do not hold the built-in interpreter's feedback. */
int gw_pack_feedback(gw_env* env, int64_t count, const int32_t* obs_dev, const float* reward_dev, const uint8_t* done_dev,
                     uint8_t* packed_dev, int32_t check, void* stream);
int gw_unpack_feedback(gw_env* env, int64_t count, const uint8_t* packed_dev, int32_t* obs_dev, float* reward_dev,
                       uint8_t* done_dev, void* stream);

/* K consecutive env.step() calls from pre-staged actions, inputs/outputs laid out [K][N].  In the default
 * mode this is ONE persistent launch per 64 steps (state in registers, lanes free-running through their
 * own event sequences: ct_rollout_sfx.hip); results are identical to K gw_step calls. */
int gw_rollout(gw_env* env, int32_t steps, const int32_t* device_dev, const int32_t* duration_dev,
               int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);

/* gw_rollout with the policy inside: `steps` env.step() calls in which every env's action is drawn from the observation it
 * just got, as the reference's caller does between two steps (agents/dqn_counter_traffic.py:63-70: a policy over
 * window_length = 1 observations; :25-31 flat action -> device, duration).  The agent sees one of three values,
 * counter_bound + payload_value * {-1, 0, +1}, so any such policy is a table of three rows over the A = num_devices *
 * max_duration flat actions -- cdf_dev: uint32[3][A], row-major, non-decreasing per row (gymwipe_amd/actions.py policy_cdf).
 * Env e at step k of the call acts on obs_prev_dev[e] (int32[N]) for k = 0 and on its own observation of step k - 1 afterwards:
 *     cls = sign(obs - counter_bound) + 1
 *     h   = splitmix64(seed ^ ((env_id0 + e) * 0x9E3779B97F4A7C15) ^ ((step0 + k) * 0xD1B54A32D192ED03))     (actions.py)
 *     u   = min(h & 0xffffffff, 0xfffffffe)
 *     a   = min(A - 1, #{ j in [0, A) : cdf[cls][j] <= u });   device = a / max_duration, duration = a % max_duration
 * The five outputs are [steps][N] and none may be NULL; device_out_dev / duration_out_dev have the layout gw_rollout takes, so
 * a recorded closed loop can be replayed through it.  obs_prev_dev and cdf_dev overlap none of the outputs: to continue from
 * the last row of an earlier call's obs_dev while writing the same buffer again, copy that row first.  The table is read stream-ordered (rewrite it on the same stream between
 * calls), never validated or read back: the clamp keeps any content memory-safe, and a drawn action is always inside the
 * action space (no GW_FLAG_BADACT).  Continue a stream of draws by advancing step0 by `steps`; shard it by env_id0.
 * Default mode: ONE launch per 64 steps (ct_rollout_policy in ct_rollout_policy.hip), the draw at each step boundary inside it.
 * Every other handle (explicit queues, live PHY, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0), or any
 * handle while GW_ROLLOUT_POLICY_UNFUSED is set: a sampling launch and a step launch per step, same results;
 * GW_ROLLOUT_STRICT turns that into GW_EUNSUPPORTED.  steps == 0 is GW_OK; a NULL pointer or steps < 0 is GW_EINVAL before
 * any HIP call.  Not for hipGraph capture: step0 is baked into the recorded launch, so every replay repeats the same draws. */
int gw_rollout_policy(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0, uint64_t env_id0,
                      const int32_t* obs_prev_dev, int32_t* device_out_dev, int32_t* duration_out_dev,
                      int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);

/* The table of a closed loop: everything a learner or an evaluator takes from a transition of this env is a function of the
 * observation class the agent saw and the flat action it took. */
#define GW_TS_COLS 7
/* int64 table[3][A][GW_TS_COLS], row-major; cls = sign(obs_seen - counter_bound) + 1, a = device * max_duration + duration
 *   0 n          transitions taken from (cls, a)
 *   1 r_sum      sum of rewards (signed)          2 r_sq   sum of reward^2
 *   3,4,5 next   transitions whose resulting observation was below / at / above counter_bound (columns 3 + 4 + 5 == column 0)
 *   6 done       transitions whose step returned done != 0 */

/* gw_rollout_policy without its five [steps][N] outputs: the env trajectory, the draws and the state changes are exactly those
 * of gw_rollout_policy with the same arguments, and every transition is ADDED into table_dev (the caller zeroes it; calls
 * accumulate).  obs_last_dev[e] (int32[N]) receives the env's last observation; it may be obs_prev_dev itself (an env reads its
 * own element before it writes it), which is how a caller continues: obs in place, step0 += steps.  return_dev (int32[N], may
 * be NULL): return_dev[e] += the env's reward sum over the call.  Allocates nothing, stream-ordered, the tables never
 * validated.  Default mode only (ct_rollout_pstats in ct_rollout_stats.hip, one launch per 64 steps, the tally in LDS).  A handle
 * without that form -- explicit queues, live PHY, created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0, A > 640, a
 * histogram of 3 * A bins that does not fit LDS beside the kernel's tables (sender counts without a kernel of their own from
 * 12 up at max_duration 20), or any handle while GW_ROLLOUT_POLICY_UNFUSED is set -- gets GW_EUNSUPPORTED before anything is
 * launched: call gw_rollout_policy and gw_transition_stats instead.  steps == 0 is GW_OK; a NULL pointer other than return_dev /
 * stream, or steps < 0, is GW_EINVAL before any HIP call. */
int gw_rollout_policy_stats(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0, uint64_t env_id0,
                            const int32_t* obs_prev_dev, int32_t* obs_last_dev, int32_t* return_dev, int64_t* table_dev, void* stream);

/* The same table from recorded transitions ([steps][N] arrays as gw_rollout_policy returns them), ADDED into table_dev.  Step
 * k's observation seen is obs_prev_dev for k = 0 and row k - 1 of obs_dev afterwards.  Every handle (it reads the configuration
 * only).  Memory-safe for any content: a row whose action lies outside the action space is skipped (a GW_FLAG_BADACT step: the
 * env did nothing), a reward is rounded to nearest and clamped to [-10, 10], done counts where != 0. */
int gw_transition_stats(gw_env* env, int32_t steps, const int32_t* obs_prev_dev, const int32_t* device_dev, const int32_t* duration_dev,
                        const int32_t* obs_dev, const float* reward_dev, const uint8_t* done_dev, int64_t* table_dev, void* stream);

/* Episodes inside the closed loop.  gw_rollout_policy cannot end an episode: an env is reset only by gw_reset between calls.
 * Here each env carries two caller-owned int32 values {age, ret} -- the steps and the reward sum since its last reset -- and
 * after step k of env e has produced its (obs, reward, done), in this order:
 *   1. age += 1; ret += reward
 *   2. cause = (on_done && done) ? 1 : (max_steps > 0 && age >= max_steps) ? 2 : 0        (done wins over the step limit)
 *   3. ended[k][e] = cause
 *   4. cause != 0: {1, cause == 1, age, ret, ret * ret} is added into the episode tally
 *   5. cause != 0: the env is reset exactly as gw_reset with mask[e] != 0 would reset it between step k and step k + 1
 *      (counters to 0 from the current tick, interpreter cleared, simulated time not rewound)
 *   6. cause != 0: age = ret = 0, and at step k + 1 the env acts on the reset's observation, counter_bound (class 1)
 * Row k of obs / reward / done stays what the step returned (obs[k] is the terminal observation). */
#define GW_EP_COLS 5   /* int64 tally: episodes ended, of those by done, sum of lengths, sum of returns, sum of returns^2 */
typedef struct gw_episodes {
    int32_t  max_steps;     /* > 0: reset after the max_steps-th step since the env's last reset; 0: no time limit */
    int32_t  on_done;       /* != 0: reset after a step that returned done */
    int32_t* state_dev;     /* int32[N][2] {age, ret}, in/out, never NULL (the caller zeroes it after its own gw_reset) */
    int64_t* tally_dev;     /* int64[GW_EP_COLS], ADDED into; may be NULL */
} gw_episodes;

/* gw_rollout_policy with episodes: the same draws -- the hash of (seed, env_id0 + e, step0 + k); a reset does not shift the
 * stream -- and the same five [steps][N] outputs, plus ended_dev (uint8[steps][N]) and obs_next_dev (int32[N]): the observation
 * each env acts on next, its last one or counter_bound where it has just been reset.  Pass obs_next_dev as the next call's
 * obs_prev_dev; it may be the same array (an env reads its element before writing it), but neither overlaps the [steps][N]
 * outputs.  max_steps == 0 && on_done == 0 gives exactly gw_rollout_policy's outputs and state, ended all zero.
 * Default mode: ONE launch per 64 steps (ct_rollout_policy_ep in ct_rollout_policy.hip), the reset in registers at the step
 * boundary.  Every other handle (as for gw_rollout_policy), or any handle while GW_ROLLOUT_POLICY_UNFUSED is set: per step a
 * sampling launch, a step launch, a bookkeeping launch and gw_reset's launch with a mask the handle owns -- same results;
 * GW_ROLLOUT_STRICT turns that into GW_EUNSUPPORTED.  steps == 0 is GW_OK; a NULL pointer other than tally_dev / stream,
 * steps < 0 or max_steps < 0 is GW_EINVAL before any HIP call.  Allocates nothing, stream-ordered, the table never validated.
 * Not for hipGraph capture: step0 is baked into the recorded launch, so every replay repeats the same draws. */
int gw_rollout_episodes(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0, uint64_t env_id0,
                        const gw_episodes* ep, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                        int32_t* device_out_dev, int32_t* duration_out_dev, int32_t* obs_dev, float* reward_dev,
                        uint8_t* done_dev, uint8_t* ended_dev, void* stream);

/* gw_rollout_episodes without its [steps][N] outputs: every transition ADDED into table_dev (gw_rollout_policy_stats' table)
 * under the class of the observation the env acted on -- counter_bound after a reset, otherwise its last observation; the
 * next-observation and done columns are what the step returned.  Default mode only (ct_rollout_pstats_ep), available where
 * gw_rollout_policy_stats is; elsewhere GW_EUNSUPPORTED before anything is launched: call gw_rollout_episodes and
 * gw_transition_stats_ep instead.  Argument rules and the hipGraph caveat as above. */
int gw_rollout_episodes_stats(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0, uint64_t env_id0,
                              const gw_episodes* ep, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                              int64_t* table_dev, void* stream);

/* gw_rollout with episodes: `steps` env.step() calls from the caller's pre-staged actions (device_dev / duration_dev and the four
 * outputs are [steps][N]), with steps 1-6 of the semantics above gw_episodes applied after every step of every env -- the caller chooses the actions, the
 * call ends the episodes.  Row k of obs / reward / done is what step k returned; ended_dev[k][e] is its cause (0, 1 done,
 * 2 step limit); obs_next_dev[e] (int32[N]) receives what env e acts on next: its last observation, or counter_bound where its
 * last step ended the episode.  obs_next_dev overlaps none of the [steps][N] arrays, and the inputs none of the outputs.
 * One step with autoreset is steps = 1.
 * An action outside the action space (GW_FLAG_BADACT) leaves its env untouched as in gw_rollout -- the row repeats the current
 * obs and done with reward 0 -- and still counts as a step of the episode: age += 1, ret += 0, the cause from the repeated
 * done.  A rejected action can so end an episode by the step limit, and the env is then reset.
 * max_steps == 0 && on_done == 0 gives exactly gw_rollout's outputs and state, ended all zero; {age, ret} still advance.
 * Default mode: ONE launch per 64 steps (ct_rollout_sync_ep in ct_rollout_autoreset.hip), the reset in registers at the step
 * boundary.  Every other handle (explicit queues, live PHY, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0):
 * per step a step launch, a bookkeeping launch and gw_reset's launch with a mask the handle owns -- same results;
 * GW_ROLLOUT_STRICT turns that into GW_EUNSUPPORTED before anything is launched.  steps == 0 is GW_OK; a NULL pointer other
 * than tally_dev / stream, steps < 0 or max_steps < 0 is GW_EINVAL before any HIP call.  Allocates nothing, stream-ordered.
 * This call MAY be captured into a hipGraph: nothing of the call but its pointers and limits is baked into the recorded
 * launches (there is no step0), so a replay continues the episodes from the arrays' current contents.  As for every captured
 * launch of a handle, the recorded kernels keep the fast forms' validity-limit tests, and so does the handle from then on. */
int gw_rollout_autoreset(gw_env* env, int32_t steps, const int32_t* device_dev, const int32_t* duration_dev,
                         const gw_episodes* ep, int32_t* obs_next_dev,
                         int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, uint8_t* ended_dev, void* stream);

/* A population of policies on one handle: P tables, M envs each -- what evolution strategies, the cross-entropy method or a
 * comparison of checkpoints evaluate and rank by episode return. */
typedef struct gw_population {
    int32_t num_policies;      /* P >= 1 */
    int32_t envs_per_policy;   /* M >= 1, P * M == num_envs; env e runs policy e / M (its index in THIS handle) */
    const uint32_t* cdf_dev;   /* uint32[P][3][A], each [3][A] slice a table as gw_rollout_policy takes it */
    int64_t* tally_dev;        /* int64[P][GW_EP_COLS], ADDED into (the caller zeroes it; calls accumulate), never NULL */
} gw_population;

/* gw_rollout_episodes for P policies at once, without its [steps][N] outputs.  For every env e the draws are those of
 * gw_rollout_episodes called with cdf_dev + (e / M) * 3 * A and otherwise the same arguments -- the hash of (seed, env_id0 + e,
 * step0 + k): env_id0 shifts the stream, not the policy index -- and so are the state changes, the resets, {age, ret} and
 * obs_next_dev[e].  pop->tally_dev[p] receives the episode tally of policy p's envs; ep->tally_dev, where not NULL, that of all
 * envs: the column sums of the per-policy rows.  obs_next_dev may be obs_prev_dev.  max_steps == 0 && on_done == 0 leaves every
 * tally untouched and gives gw_rollout_policy's trajectory per policy.  Stream-ordered.  Not for hipGraph capture: step0 is
 * baked into the recorded launch.
 * Fused form -- a handle that has one for gw_rollout_episodes, M % 64 == 0 (a wave then never spans two policies; a policy may
 * span many blocks) and GW_ROLLOUT_POLICY_UNFUSED unset: ONE launch per 64 steps (ct_rollout_pop_ep in ct_rollout_pop.hip), at
 * most 2 * GW_EP_COLS global adds per block; integer adds commute, so no result depends on their order of arrival.
 * Per-step form -- any other M, explicit queues, live PHY, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0:
 * per step a sampling launch, a step launch, a bookkeeping launch and gw_reset's launch with a mask the handle owns -- same
 * results.  It steps into six N-long scratch rows that the HANDLE owns (device, duration, obs, reward, done, ended): the first
 * call that takes this form allocates them, and so synchronises the device once; gw_destroy frees them, gw_state_bytes counts
 * them from then on, a snapshot does not hold them (scratch, not state).  A handle that never takes this form holds nothing
 * more.  GW_ROLLOUT_STRICT turns the per-step form into GW_EUNSUPPORTED before anything is launched or allocated.
 * GW_EINVAL before any HIP call: env / pop / ep NULL; a NULL pointer other than ep->tally_dev / stream; steps < 0 or
 * max_steps < 0; P < 1, M < 1 or P * M != num_envs.  steps == 0 is GW_OK.  The tables are never validated or read back: the
 * draw's clamp keeps any content memory-safe. */
int gw_rollout_population(gw_env* env, int32_t steps, const gw_population* pop, uint64_t seed, uint64_t step0, uint64_t env_id0,
                          const gw_episodes* ep, const int32_t* obs_prev_dev, int32_t* obs_next_dev, void* stream);

/* Episodes scored by what they delivered.  The built-in reward is lastAbs - abs of received[0] - received[1]
 * (envs/counter_traffic.py:85-101): over an episode it telescopes to -|final difference|, so an episode's return is 0 or
 * -payload_value whatever the policy does, and the policy that assigns nothing attains the maximum.  What a band-assignment
 * scheduler exists for is delivered packets, so the two calls below score a step as
 *     score_k = w_reward * reward_k + w_delivered[d_k] * delivered_k
 * d_k: the sender the step assigned; delivered_k: the data packets of d_k that the RRM decoded in step k
 * (SimpleRrmDevice.onPacketReceived, networking/devices.py:163-168) -- the increase of gw_delivered's counter over the step; a
 * reset does not touch that counter.  All integer arithmetic; every weight lies in [-GW_SCORE_W_MAX, GW_SCORE_W_MAX] (all
 * GW_MAX_DEVICES entries of w_delivered are checked, those from num_devices on are not otherwise read), so (float)score_k is
 * exact.  w_reward = 1 with every w_delivered = 0 gives the parents' results bit for bit. */
#define GW_SCORE_W_MAX 1024
typedef struct gw_score {
    int32_t w_reward;                      /* weight of the built-in reward of the step */
    int32_t w_delivered[GW_MAX_DEVICES];   /* weight of ONE data packet of sender d decoded by the RRM in the step */
} gw_score;

/* gw_rollout_episodes with {age, ret}, the tally's return columns and reward_dev carrying the SCORE where the parent carries
 * the reward: reward_dev[k][e] = (float)score_k, ret += score_k; delivered_dev (int32[steps][N], never NULL) receives
 * delivered_k.  The draws, the episode causes, the resets, obs_next_dev, device_out_dev / duration_out_dev, obs_dev, done_dev
 * and ended_dev are exactly the parent's.  The score is read by value before the call returns.
 * Default mode: ONE launch per 64 steps (ct_rollout_policy_eps in ct_rollout_policy.hip), the weights staged beside the table.
 * Per-step form -- live PHY with default queues, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0, or any
 * handle while GW_ROLLOUT_POLICY_UNFUSED is set: per step a sampling launch that also copies each env's delivered counter
 * into a uint32[N] scratch row the HANDLE owns, a step launch, a bookkeeping launch that differences the counter and scores,
 * and gw_reset's launch -- same results.  The first call that takes this form allocates the row (and so synchronises the
 * device once); gw_destroy frees it, gw_state_bytes counts it from then on, a snapshot does not hold it.  GW_ROLLOUT_STRICT
 * turns the per-step form into GW_EUNSUPPORTED before anything is launched or allocated.  An explicit-queue handle has no
 * per-env delivered counter (gw_delivered refuses it too): GW_EUNSUPPORTED before any launch.
 * GW_EINVAL before any HIP call: score NULL (call the parent), a weight outside the bounds, delivered_dev NULL, and the
 * parent's cases.  steps == 0 is GW_OK.  Stream-ordered; not for hipGraph capture (step0 is baked into the launch). */
int gw_rollout_episodes_scored(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0, uint64_t env_id0,
                               const gw_episodes* ep, const gw_score* score, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                               int32_t* device_out_dev, int32_t* duration_out_dev, int32_t* obs_dev, float* reward_dev,
                               uint8_t* done_dev, uint8_t* ended_dev, int32_t* delivered_dev, void* stream);

/* gw_rollout_population with columns 3 and 4 of pop->tally_dev[p] and of ep->tally_dev the sums of episode SCORES and of their
 * squares ({age, ret} carries the score too); everything else is the parent's.  Fused form where the parent has one
 * (ct_rollout_pop_eps); the per-step form, its scratch (the parent's six rows and the uint32[N] row above), GW_ROLLOUT_STRICT,
 * explicit-queue handles and the argument rules as for gw_rollout_episodes_scored. */
int gw_rollout_population_scored(gw_env* env, int32_t steps, const gw_population* pop, uint64_t seed, uint64_t step0, uint64_t env_id0,
                                 const gw_episodes* ep, const gw_score* score, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                                 void* stream);

/* gw_rollout_autoreset with the SCORE where the parent carries the reward, as gw_rollout_episodes_scored relates to
 * gw_rollout_episodes: reward_dev[k][e] = (float)score_k, ret += score_k, the tally's return columns are sums of episode scores
 * and of their squares; delivered_dev (int32[steps][N], never NULL) receives delivered_k.  d_k is the sender the caller staged
 * for the step.  The episode causes, the resets, obs_dev, done_dev, ended_dev, obs_next_dev and every state change are exactly
 * the parent's; w_reward = 1 with every w_delivered = 0 gives the parent's outputs, {age, ret}, tally and state bit for bit.
 * An action outside the action space (GW_FLAG_BADACT) delivers nothing and scores exactly 0: its row repeats the current obs
 * and done, delivered 0, reward 0, and it is still a step of the episode.  No weight is read at an unchecked sender: the
 * index is clamped to [0, num_devices).
 * Default mode: ONE launch per 64 steps (ct_rollout_sync_eps in ct_rollout_autoreset.hip), the weights in LDS.  Per-step form -- live
 * PHY with default queues, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0: per step gw_delivered's launch
 * into the uint32[N] scratch row above, a step launch, the scored bookkeeping launch and gw_reset's launch -- same results.
 * The row's rules are as above: the first call that takes this form allocates it (and so synchronises the device once),
 * gw_destroy frees it, gw_state_bytes counts it from then on, a snapshot does not hold it.  GW_ROLLOUT_STRICT turns the
 * per-step form into GW_EUNSUPPORTED before anything is launched or allocated.  An explicit-queue handle, which the parent
 * accepts, has no per-env delivered counter: GW_EUNSUPPORTED before any launch.
 * GW_EINVAL before any HIP call: env / ep / score NULL, a NULL pointer other than ep->tally_dev / stream, steps < 0,
 * max_steps < 0, a weight outside the bounds (all GW_MAX_DEVICES entries, also when steps == 0).  steps == 0 with valid
 * arguments is GW_OK.  Stream-ordered.
 * This call MAY be captured into a hipGraph, as the parent may: there is no step0.  The score is read by value before the
 * call returns, so a recorded launch keeps the weights it was recorded with -- record again to change them.  Because of the
 * scratch row's allocation, a capture of the PER-STEP form needs one eager call on the handle first. */
int gw_rollout_autoreset_scored(gw_env* env, int32_t steps, const int32_t* device_dev, const int32_t* duration_dev,
                                const gw_episodes* ep, const gw_score* score, int32_t* obs_next_dev,
                                int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, uint8_t* ended_dev,
                                int32_t* delivered_dev, void* stream);

/* A queue-aware scheduler inside the rollout: assign the band to the sender with the largest weighted backlog, for as long as
 * a table says its backlog needs.  The reference's RRM cannot see sender._mac._packetQueue, so this is a builder-defined genie
 * baseline -- the yardstick for what a policy that acts on the three-valued observation leaves undelivered -- and not a
 * reference path. */
typedef struct gw_backlog_policy {
    int32_t w_len[GW_MAX_DEVICES];              /* priority of sender i = w_len[i] * qlen_i; each in [0, GW_SCORE_W_MAX] */
    uint8_t duration_of_len[GW_QUEUE_CAP + 1];  /* duration for a chosen sender whose queue holds L packets */
} gw_backlog_policy;

/* gw_rollout_autoreset_scored with the actions chosen in the call from the queue lengths.  Step k of env e:
 *   1. q_i is the length of sender i's MAC queue at the env's current time -- exactly what gw_get_state "qlen" would return
 *      had the call ended before step k: every counter tick with wake <= now has been counted, a reset at the previous step
 *      boundary is already applied (a reset leaves the queues alone);
 *   2. d is the lowest index attaining max_i w_len[i] * q_i over i in [0, num_devices) -- 0 where every priority is 0;
 *   3. du = min(duration_of_len[q_d], max_duration - 1);
 *   4. seen_len_dev[k][e] = q_d, device_out_dev[k][e] = d, duration_out_dev[k][e] = du (each int32[steps][N]);
 *   5. the step, its score, delivered_dev and steps 1-6 of the gw_episodes bookkeeping run exactly as
 *      gw_rollout_autoreset_scored runs them for the staged action (d, du).
 * So an action is always inside the action space (no GW_FLAG_BADACT), any byte in duration_of_len is valid, and replaying
 * device_out_dev / duration_out_dev through gw_rollout_autoreset_scored from the same state gives every other output,
 * {age, ret}, the tally and the state bit for bit.  score == NULL is {1, 0...}: the built-in reward.
 * Default mode: ONE launch per 64 steps (ct_rollout_backlog in ct_rollout_backlog.hip) on the handles that have
 * ct_rollout_sync_eps; the queues are brought to the current tick in registers at every step boundary, the policy lies in
 * LDS.  Per-step form -- live PHY with default queues, a handle created under GW_ROLLOUT_EVENT_LOOP, rollout capacity 0, or
 * any handle while GW_ROLLOUT_POLICY_UNFUSED is set (read per call): per step one small launch that reads each env's
 * queue-length bytes where gw_get_state "qlen" reads them and writes (d, du, q_d) into row k, then
 * gw_rollout_autoreset_scored's per-step sequence on that row -- same results.  The uint32[N] scratch row's rules are that
 * call's: allocated by the first call that takes this form, counted by gw_state_bytes from then on, freed by gw_destroy, not
 * in snapshots.  GW_ROLLOUT_STRICT turns the per-step form into GW_EUNSUPPORTED before anything is launched or allocated.
 * An explicit-queue handle has no per-env delivered counter: GW_EUNSUPPORTED before any launch.
 * GW_EINVAL before any HIP call: env / pol / ep NULL, a NULL pointer other than score / ep->tally_dev / stream, steps < 0,
 * max_steps < 0, a w_len entry outside [0, GW_SCORE_W_MAX] (all GW_MAX_DEVICES entries, also when steps == 0), a score weight
 * outside its bounds.  steps == 0 with valid arguments is GW_OK.  Stream-ordered.
 * There are no draws and no step0, so this call MAY be captured into a hipGraph under gw_rollout_autoreset_scored's rules;
 * the policy and the score are read by value before the call returns. */
int gw_rollout_backlog(gw_env* env, int32_t steps, const gw_backlog_policy* pol, const gw_episodes* ep, const gw_score* score,
                       int32_t* obs_next_dev, int32_t* device_out_dev, int32_t* duration_out_dev, int32_t* seen_len_dev,
                       int32_t* obs_dev, float* reward_dev, uint8_t* done_dev, uint8_t* ended_dev, int32_t* delivered_dev,
                       void* stream);

/* gw_rollout_backlog for P policies at once, for a caller that tunes the scheduler: what gw_rollout_population is to
 * gw_rollout_episodes.  Nothing [steps][N] is stored; each policy's episodes are tallied into its own row. */
typedef struct gw_backlog_population {
    int32_t num_policies;                     /* P >= 1 */
    int32_t envs_per_policy;                  /* M >= 1, P * M == num_envs; env e runs policy e / M */
    const gw_backlog_policy* policies_dev;    /* gw_backlog_policy[P] in DEVICE memory, stride sizeof (232), 4-byte aligned */
    int64_t* tally_dev;                       /* int64[P][GW_EP_COLS], ADDED into, never NULL */
} gw_backlog_population;

/* For every env e the choices, the steps, the scores, the resets, {age, ret}, obs_next_dev[e] and every state change are those
 * of gw_rollout_backlog called with policy e / M; pop->tally_dev[p] receives the episode tally of policy p's envs and
 * ep->tally_dev, where not NULL, the column sums of those rows.  score == NULL is the built-in reward.
 * The policies lie in device memory and are never read back, so they are not validated: each w_len[i] is clamped into
 * [0, GW_SCORE_W_MAX] where it is read, any byte of duration_of_len is valid, and every index is clamped as in
 * gw_rollout_backlog -- any content is memory-safe and has one meaning (actions.backlog_sample_population_numpy restates it).
 * Default mode, envs_per_policy a multiple of 64: ONE launch per 64 steps (ct_rollout_backlog_pop in ct_rollout_backlog.hip) on
 * the handles that have ct_rollout_backlog; a block of 64 envs stages its policy's 232 bytes into LDS with one load per wave.
 * Per-step form -- any other envs_per_policy, live PHY with default queues, a handle created under GW_ROLLOUT_EVENT_LOOP,
 * rollout capacity 0, or any handle while GW_ROLLOUT_POLICY_UNFUSED is set (read per call): per step a choice launch that
 * reads policy e / M, gw_delivered's copy, the step, the scored bookkeeping with the population's rows and gw_reset with the
 * handle's mask, in the scratch rows gw_rollout_population_scored's per-step form uses (allocated by the first call that
 * takes this form, counted by gw_state_bytes from then on, not in snapshots) -- same results, and the host's bound on the
 * clocks is left as the fused form leaves it.  GW_ROLLOUT_STRICT turns the per-step form into GW_EUNSUPPORTED before anything
 * is launched or allocated.  An explicit-queue handle has no per-env delivered counter: GW_EUNSUPPORTED before any launch.
 * GW_EINVAL before any HIP call: env / pop / ep NULL; policies_dev, pop->tally_dev, ep->state_dev or obs_next_dev NULL;
 * steps < 0; max_steps < 0; a score weight outside its bounds; policies_dev not 4-byte aligned; P < 1 or M < 1 (all of these
 * also when steps == 0); P * M != num_envs.  steps == 0 with valid arguments is GW_OK.  Stream-ordered.
 * There are no draws and no step0, so this call MAY be captured into a hipGraph under gw_rollout_autoreset_scored's rules: the
 * score is read by value before the call returns and baked into the recording, the policies are NOT -- every replay reads
 * what policies_dev holds when it runs, so a search loop is: write P policies, replay, read P rows. */
int gw_rollout_backlog_population(gw_env* env, int32_t steps, const gw_backlog_population* pop, const gw_episodes* ep,
                                  const gw_score* score, int32_t* obs_next_dev, void* stream);

/* ---- finite-state controllers inside the scored closed loop ----
 * A policy table over the observation class cannot remember what it did.  A controller has S nodes, 1 <= S <=
 * GW_FSC_MAX_STATES: the env's node and the observation class pick the row the action is drawn from, and the node then moves
 * on the new observation class and on one bit -- whether the step delivered at least the node's threshold of packets.  Both
 * are things a real RRM knows.  Three arrays in DEVICE memory, never validated and never read back on the host:
 *   cdf  uint32[S][3][A]   for each (node, class) a row as gw_rollout_policy takes it, A = num_devices * max_duration
 *   next uint8[S][3][2]    the node to move to, by (node, new class, bit)
 *   need uint8[S]          each node's delivered-packet threshold
 * and each env's node in the caller's node_dev uint8[N], read at the start of a call and written at its end as {age, ret} is
 * (the caller's array, not handle state: snapshots do not hold it).  For env e:
 *   at the start of a call   n = min(node_dev[e], S - 1), c = cls(obs_prev_dev[e])
 *   step k's action          gw_rollout_policy's draw from row cdf[n][c] with u(seed, env_id0 + e, step0 + k)
 *   the step runs            delivered_k, score_k and the episode's book exactly as in gw_rollout_episodes_scored
 *   behind EVERY step        the step ended an episode: n = 0, c = 1 (the reset's observation); otherwise c = cls(obs_k),
 *                            b = (delivered_k >= need[n]), n = min(next[n][c][b], S - 1) -- need[n] and next[n] of the node
 *                            the step was taken at
 *   at the end of a call     node_dev[e] = n, obs_next_dev[e] as in the parents
 * The clamps apply where the bytes are read, so any content is memory-safe and has one meaning
 * (actions.controller_step_numpy restates it).  A call split at any step gives the rows of one call; with S == 1 the call is
 * gw_rollout_episodes_scored bit for bit. */
#define GW_FSC_MAX_STATES 16
typedef struct gw_controller {
    int32_t num_states;                       /* S */
    const uint32_t* cdf_dev;                  /* uint32[S][3][A] */
    const uint8_t* next_dev;                  /* uint8[S][3][2] */
    const uint8_t* need_dev;                  /* uint8[S] */
    uint8_t* node_dev;                        /* uint8[N], in/out */
} gw_controller;
typedef struct gw_controller_population {
    int32_t num_policies;                     /* P >= 1 */
    int32_t envs_per_policy;                  /* M >= 1, P * M == num_envs; env e runs controller e / M */
    int32_t num_states;                       /* one S for all */
    const uint32_t* cdf_dev;                  /* uint32[P][S][3][A] */
    const uint8_t* next_dev;                  /* uint8[P][S][3][2] */
    const uint8_t* need_dev;                  /* uint8[P][S] */
    uint8_t* node_dev;                        /* uint8[N], in/out */
    int64_t* tally_dev;                       /* int64[P][GW_EP_COLS], ADDED into, never NULL */
} gw_controller_population;

/* gw_rollout_controller: gw_rollout_episodes_scored's outputs, and node_out_dev uint8[steps][N], the node each step was taken
 * at.  gw_rollout_controller_population: gw_rollout_population_scored's tallies -- env e runs controller e / M, env_id0 shifts
 * the stream and not the controller index; pop->tally_dev[p] receives the episodes of controller p's envs and ep->tally_dev,
 * where not NULL, the column sums.
 * ONE launch per 64 steps (ct_rollout_fsc / ct_rollout_fsc_pop in ct_rollout_fsc.hip); the controller's tables lie in the
 * block's LDS.  There is no per-step form.  GW_EUNSUPPORTED, before any launch and with the state and node_dev untouched: a
 * handle without a fused rollout for gw_rollout_episodes (explicit queues, live PHY, a handle created under
 * GW_ROLLOUT_EVENT_LOOP, rollout capacity 0); GW_ROLLOUT_POLICY_UNFUSED set; envs_per_policy not a multiple of 64 (the
 * population call); a controller whose (3 S A + num_devices) words and 7 S bytes do not fit the 65 536 bytes of a block's LDS
 * beside the kernel's own tables.
 * GW_EINVAL before any HIP call: env / ctl / pop / ep / score NULL; any array of the controller, node_dev and node_out_dev
 * included, any output, ep->state_dev, obs_prev_dev or obs_next_dev NULL; steps < 0; max_steps < 0; S outside
 * [1, GW_FSC_MAX_STATES]; a score weight outside its bounds; P < 1 or M < 1 (all of these also when steps == 0);
 * P * M != num_envs.  steps == 0 with valid arguments is GW_OK.  Stream-ordered.  Not for hipGraph capture: step0 would be
 * baked into the recording. */
int gw_rollout_controller(gw_env* env, int32_t steps, const gw_controller* ctl, uint64_t seed, uint64_t step0, uint64_t env_id0,
                          const gw_episodes* ep, const gw_score* score, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                          int32_t* device_out_dev, int32_t* duration_out_dev, int32_t* obs_dev, float* reward_dev,
                          uint8_t* done_dev, uint8_t* ended_dev, int32_t* delivered_dev, uint8_t* node_out_dev, void* stream);
int gw_rollout_controller_population(gw_env* env, int32_t steps, const gw_controller_population* pop, uint64_t seed, uint64_t step0,
                                     uint64_t env_id0, const gw_episodes* ep, const gw_score* score, const int32_t* obs_prev_dev,
                                     int32_t* obs_next_dev, void* stream);

/* gw_transition_stats for rows recorded by gw_rollout_episodes: step k's observation seen is counter_bound where
 * ended_dev[k - 1] != 0; row 0 uses obs_prev_dev as it is. */
int gw_transition_stats_ep(gw_env* env, int32_t steps, const int32_t* obs_prev_dev, const int32_t* device_dev,
                           const int32_t* duration_dev, const int32_t* obs_dev, const float* reward_dev, const uint8_t* done_dev,
                           const uint8_t* ended_dev, int64_t* table_dev, void* stream);

/* The tally with the packets a step delivered.  A step's score (gw_score) is linear, w_reward * reward + w_delivered[device] *
 * delivered, and the flat action names the sender (a / max_duration): a bin's score sum under ANY gw_score is
 *     w_reward * column 1 + w_delivered[a / max_duration] * column 7
 * so the table carries one more sum per bin and no weights; the caller applies whichever score afterwards. */
#define GW_TSD_COLS 8
/* int64 table[3][A][GW_TSD_COLS], row-major: columns 0-6 are GW_TS_COLS' columns,
 *   7 delivered   sum of min(delivered, 65 535) over the bin's transitions -- delivered: the data packets of the assigned sender
 *                 the RRM decoded in the step (what gw_rollout_episodes_scored records).  A step delivers at most 100 + 100 *
 *                 (counter ticks inside its window) packets -- 25 600 with one tick per duration unit and max_duration 254,
 *                 9 at the default configuration -- so the clamp binds only where a window spans more than 654 ticks.
 *
 * gw_rollout_policy_stats_delivered / gw_rollout_episodes_stats_delivered: the arguments, draws, state changes, episode
 * bookkeeping (the built-in reward's: the table is score-free), availability and refusals of gw_rollout_policy_stats /
 * gw_rollout_episodes_stats, the table one column wider (ct_rollout_pstats_d / ct_rollout_pstats_epd in ct_rollout_stats.hip: the
 * sum rides in bits the histogram's second word had left, no LDS byte and no atomic more).  GW_EUNSUPPORTED before anything is
 * launched where the parents answer it; the episodic call is then composed from gw_rollout_episodes_scored with the neutral
 * score and gw_transition_stats_delivered, the other one from nothing (gw_rollout_policy records no packets). */
int gw_rollout_policy_stats_delivered(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0,
                                      uint64_t env_id0, const int32_t* obs_prev_dev, int32_t* obs_last_dev, int32_t* return_dev,
                                      int64_t* table_dev, void* stream);
int gw_rollout_episodes_stats_delivered(gw_env* env, int32_t steps, const uint32_t* cdf_dev, uint64_t seed, uint64_t step0,
                                        uint64_t env_id0, const gw_episodes* ep, const int32_t* obs_prev_dev, int32_t* obs_next_dev,
                                        int64_t* table_dev, void* stream);
/* gw_transition_stats / gw_transition_stats_ep (ended_dev NULL / not NULL) with a row of packets per step, delivered_dev
 * int32[steps][N], into the eight-column table.  A negative count is 0, one above 65 535 is 65 535; a row whose action lies
 * outside the action space is skipped.  Every handle.  A NULL pointer other than ended_dev / stream, or steps < 0, is
 * GW_EINVAL before any HIP call; steps == 0 is GW_OK. */
int gw_transition_stats_delivered(gw_env* env, int32_t steps, const int32_t* obs_prev_dev, const int32_t* device_dev,
                                  const int32_t* duration_dev, const int32_t* obs_dev, const float* reward_dev, const uint8_t* done_dev,
                                  const uint8_t* ended_dev, const int32_t* delivered_dev, int64_t* table_dev, void* stream);

/* Cumulative number of data packets the RRM has decoded per env since gw_create: uint32[N], device pointer
 * (default mode).  A custom Interpreter (envs/core.py:59-159) differences this across a step to learn how many
 * packets of the assigned sender the RRM sniffed (networking/devices.py:163-168). */
int gw_delivered(gw_env* env, uint32_t* out_dev, void* stream);

/* Position.set(x, y) on radio `radio` (0..D-1 senders, D = the RRM) of every env with mask_dev == NULL or mask_dev[e] != 0,
 * at the envs' current time, i.e. between two env.step() calls (devices/core.py:77-86); the attenuation of every link of
 * that radio is recomputed (physical.py:380-386, attenuation_models.py:28-36) with the device libm.  x_dev / y_dev:
 * double[N] device pointers.  Needs GW_CFG_PER_ENV_GEOMETRY. */
int gw_set_position(gw_env* env, int32_t radio, const double* x_dev, const double* y_dev, const uint8_t* mask_dev, void* stream);
/* the same for every radio at once: pos_dev is double[N][R][2] (device pointer), R = num_devices + 1 */
int gw_set_positions(gw_env* env, const double* pos_dev, const uint8_t* mask_dev, void* stream);

/* receivedValues of every env: int32[N][D] (row-major), device pointer. */
int gw_received(gw_env* env, int32_t* out_dev, void* stream);

/* Synchronous state readers for tests/debugging: copies `field` of every env to HOST memory.
 *   "now" f64[N] | "wake" f64[N][D] | "counter" u32[N][D] | "qlen" i32[N][D]
 *   "queue" u32[N][D][GW_QUEUE_CAP] (logical order from the head, zero padded)
 *   "received" i32[N][D] | "latest_diff" i32[N] | "last_abs" i32[N] | "rx_power" f64[N][R]
 *   "flags" u32[N] | "n_tx","n_delivered","n_appended","n_popped","n_dropped" u64[N] (per-env event counts)
 *   GW_CFG_PER_ENV_GEOMETRY: "pos" f64[N][R][2] | "link_power" f64[N][R][R] (mW, from -> to) */
int gw_get_state(gw_env* env, const char* field, void* dst_host, size_t bytes);

/* Ranges of the event counts in the DEFAULT queue mode, where most of them are derived rather than counted (only popped,
 * delivered, bad actions and flags are bumped on the device): steps = env.step() launches - bad actions; transmissions =
 * steps + popped; appended = ticks * sum(multiplicity); dropped = appended - popped - queued.  `popped` and `delivered` of
 * one env share a 64-bit word (popped in the low half): beyond 2^32 - 1 pops per env the carry would reach `delivered`; the
 * tick counter is 32 bits (2^32 ticks = 49 days of simulated time at the reference's 1 ms interval).  Neither limit is
 * checked; a handle that may get there should use GW_CFG_EXPLICIT_QUEUE | GW_CFG_PER_ENV_STATS (64-bit counts per event). */
int gw_stats_read(gw_env* env, gw_stats* out);          /* synchronises the device */
/* the sticky per-env flag words back to zero (gw_get_state "flags", gw_stats.flags_or), so that a later check tells
 * WHEN a condition arose; counters are untouched */
int gw_clear_flags(gw_env* env, void* stream);
int gw_state_bytes(gw_env* env, uint64_t* bytes);       /* HBM held by this handle */

/* Checkpoint / restore.  The reference cannot snapshot a running simulation (SimPy generators; only the agent's weights are
 * saved, agents/dqn_counter_traffic.py:73); here an env's state is a handful of arrays in HBM.  gw_get_snapshot copies all of it
 * to host memory (gw_snapshot_bytes bytes; synchronises the device); gw_set_state restores it into a handle created with the
 * same gw_config -- the same handle later on, or a fresh one on any GPU -- after which every step continues bit for bit as the
 * snapshotted handle would have.  GW_EINVAL for a blob that is not a snapshot of this ABI / configuration. */
int gw_snapshot_bytes(gw_env* env, uint64_t* bytes);
int gw_get_snapshot(gw_env* env, void* dst_host, uint64_t bytes);
int gw_set_state(gw_env* env, const void* src_host, uint64_t bytes);

/* static link tables (host side, for tests): attenuation dB, rx power mW, thermal mW,
 * and the rx-power state machine used instead of per-env f64 noise state */
int gw_link_info(gw_env* env, int32_t from, int32_t to, double* attenuation_db, double* rx_power_mw);
int gw_noise_states(gw_env* env, int32_t radio, int32_t* count, double* values_mw /* [16] */);

/* ---------------------------------------------------------------------------------------------------
 * Linear plant (BASELINE config 4): the plant side of the pendulum env.
 *   replaces  OdePlant.updateState -- "advance the plant to the current simulated time, lazily"
 *             (gymwipe/plants/core.py:38-49) and the SlidingPendulum getters / setMotorVelocity
 *             (gymwipe/plants/sliding_pendulum.py:57-85)
 * with a fixed-dt linear model  x <- A x + B u  (4 states, 1 input), n = round((now - last)/dt) substeps
 * per call, evaluated on the f64 matrix cores (v_mfma_f64_16x16x4_f64).  BUILDER-DEFINED: the
 * reference's plant is an ODE rigid-body world (py3ode, absent) inside an env that cannot be
 * constructed (simtools.py:39-42), so there is nothing to pin parity to; the oracle is this library's
 * own scalar restatement of the same recurrence (test tree), tolerance 1e-5 relative.
 * ------------------------------------------------------------------------------------------------- */
#define GW_PLANT_DIM   4
#define GW_PLANT_KMAX  32                   /* substeps applied per matrix-core pass */

typedef struct gw_plant_config {
    int32_t abi_version;                    /* GW_ABI_VERSION */
    int32_t hip_device;
    int64_t num_envs;
    double  A[GW_PLANT_DIM * GW_PLANT_DIM]; /* row-major one-substep state matrix */
    double  B[GW_PLANT_DIM];                /* one-substep input vector */
    double  dt;                             /* substep length, s */
    double  x0[GW_PLANT_DIM];               /* initial state {wagon pos, wagon vel, angle, angle rate} */
    double  u0;                             /* initial input (motor velocity; reference: 0.1) */
} gw_plant_config;

typedef struct gw_plant gw_plant;

/* pendulum-like default: velocity-servoed wagon, small-angle pendulum, forward-Euler at dt = 1 ms */
int gw_plant_config_default(gw_plant_config* cfg, int64_t num_envs);
int gw_plant_create(const gw_plant_config* cfg, gw_plant** out);
int gw_plant_destroy(gw_plant* p);
/* advance env e to time *(double*)((char*)now_dev + e*stride_bytes); no-op where that is not later than its last update */
int gw_plant_update(gw_plant* p, const void* now_dev, int64_t stride_bytes, void* stream);
/* u[e] <- u_dev[e] where mask_dev is NULL or mask_dev[e] != 0 (setMotorVelocity; the caller updates first) */
int gw_plant_set_input(gw_plant* p, const double* u_dev, const uint8_t* mask_dev, void* stream);
/* InvertedPendulumInterpreter (envs/inverted_pendulum.py:27-57) for every plant: obs = int(degrees(angle)),
 * reward = float(abs(180 - degrees(angle))), optionally the angle in degrees ("Sensor angle").  Any pointer may be NULL. */
int gw_plant_feedback(gw_plant* p, int32_t* obs_dev, float* reward_dev, double* angle_deg_dev, void* stream);
/* gw_plant_update and gw_plant_feedback in one launch (what an env.step() of the pendulum env needs after the network step) */
int gw_plant_update_feedback(gw_plant* p, const void* now_dev, int64_t stride_bytes, int32_t* obs_dev, float* reward_dev,
                             double* angle_deg_dev, void* stream);
/* env.step() of the pendulum env (InvertedPendulumEnv.step, envs/inverted_pendulum.py:101-113) in ONE launch: gw_step of the env's
 * network (two assignable devices, default queue mode; its own CounterTraffic feedback is not produced) + gw_plant_update to the
 * env's new clock + gw_plant_feedback.  Same results as the three calls.  Any output pointer may be NULL. */
int gw_pendulum_step(gw_env* env, gw_plant* p, const int32_t* device_dev, const int32_t* duration_dev, int32_t* obs_dev,
                     float* reward_dev, double* angle_deg_dev, void* stream);
/* device pointer to the state, double[N][4] (row e = {pos, vel, angle, rate}); valid until gw_plant_destroy */
int gw_plant_state_ptr(gw_plant* p, double** x_dev);
/* host copies for tests: "x" f64[N][4] | "u" f64[N] | "t_last" f64[N] | "substeps" u64[N] */
int gw_plant_get_state(gw_plant* p, const char* field, void* dst_host, size_t bytes);

/* device pointer + stride of the per-env simulated time of a gw_env (default mode), for gw_plant_update */
int gw_now_ptr(gw_env* env, const void** now_dev, int64_t* stride_bytes);

/* ---------------------------------------------------------------------------------------------------
 * PHY grid: N independent replicas of the reference's benchmark scenario
 * (tests/test_benchmark.py:20-91) -- n uncoordinated PHY-only devices, each sending one 39-byte packet
 * every 10 ms at 40 dBm from its own phase.  The one workload of the reference with CONCURRENT
 * transmissions: every radio sums the power of all active transmissions (simple_stack.py:99-157) and
 * re-integrates its bit errors at every power change (:161-188,:214-267); a device that wants to send
 * while receiving waits for the reception to end (:199-200).
 *   replaces  SimMan.runSimulation(seconds) over SendingDevice / SimplePhy / FrequencyBand
 * One wave per replica, one lane per radio; events are popped in SimPy's (time, priority, insertion id)
 * order.  Integer outcomes are compared bit-exact with the event-driven oracle; BER uses the device
 * libm (log10/pow/sqrt), so floating-point state is compared to 1e-9 relative.
 * ------------------------------------------------------------------------------------------------- */
#define GW_GRID_MAX_DEVICES 64

typedef struct gw_grid_config {
    int32_t abi_version;                    /* GW_ABI_VERSION */
    int32_t hip_device;
    int64_t num_envs;                       /* replicas */
    int32_t num_devices;                    /* n <= GW_GRID_MAX_DEVICES */
    int32_t mobile;                         /* 1: every device also random-walks (mobile_device_grid, :73-85) */
    double  pos[GW_GRID_MAX_DEVICES][2];    /* metres (default: (i / cols, i % cols), cols = int(sqrt(n))) */
    double  slot, frequency, bandwidth, temperature_c, bit_rate, code_rate, max_ber;
    double  tx_power_dbm;                   /* 40.0   tests/test_benchmark.py:47 */
    double  send_interval;                  /* 1e-2   :17 */
    int32_t header_bytes;                   /* 13 */
    int32_t payload_bytes;                  /* 26 = len("A message to all my homies") */
    double  move_interval;                  /* 1e-3   tests/test_benchmark.py:18 */
    double  move_span;                      /* 0.2: offsets uniform(-span, span) per axis and move (:79-80) */
    uint64_t seed;                          /* the walk of replica e, device i, move k is splitmix64(seed, e, i, k) */
} gw_grid_config;

typedef struct gw_grid gw_grid;

int gw_grid_config_default(gw_grid_config* cfg, int64_t num_envs, int32_t num_devices);
/* initial_delays_host: double[N][n], the random.uniform(0, SEND_INTERVAL) of tests/test_benchmark.py:67 */
int gw_grid_create(const gw_grid_config* cfg, const double* initial_delays_host, gw_grid** out);
int gw_grid_destroy(gw_grid* g);
/* SimMan.runSimulation(seconds) for every replica */
int gw_grid_run(gw_grid* g, double seconds, void* stream);
/* Position.set(x, y) of device `device` in every replica at the replicas' current time (devices/core.py:77-86):
 * the attenuation of every link of that device changes and every radio that is hearing a transmission over
 * such a link updates its received power and re-integrates its bit errors (simple_stack.py:119-128).
 * A move that leaves two radios 3000 m or more apart puts their link in stand-by (physical.py:371-386): powers already
 * stored stay, and transmissions that start later are still received over the link's old attenuation, until a move brings
 * the two within 3000 m again.
 * x_host / y_host: double[N].  Needs cfg.mobile != 0 (per-replica geometry); set move_interval very large to
 * have scripted moves only. */
int gw_grid_set_position(gw_grid* g, int32_t device, const double* x_host, const double* y_host, void* stream);
/* host copies: "now" f64[N] | "events","n_tx","flags","on_air" u32[N] (on_air = transmissions currently active) | "n_sent","hdr_ok","hdr_fail","pay_ok","pay_fail" u32[N][n]
 *              | "rx_power" f64[N][n] | "pos" f64[N][n][2] */
int gw_grid_get_state(gw_grid* g, const char* field, void* dst_host, size_t bytes);
/* Test hook (cf. gw_selftest_launches): the lanes per replica (4, 8, 16, 32 or 64) of grid_run_kernel<mobile, width>.
 * With a handle: the width of that handle's last gw_grid_run, 0 before any run (num_envs / num_devices are ignored).
 * With g == NULL: the width the launcher would pick for (num_envs, num_devices); needs no GPU.  Negative GW_E* code for
 * num_envs <= 0 or num_devices outside [1, GW_GRID_MAX_DEVICES]. */
int32_t gw_grid_selftest_width(const gw_grid* g, int64_t num_envs, int32_t num_devices);

/* ---- Control loop (second half): the pendulum env with its loop closed -------------------------------
 * BUILDER-DEFINED: the reference intends this loop (plants/sliding_pendulum.py:116-155, control/inverted_pendulum.py:16-69,
 * envs/inverted_pendulum.py:60-113) but never runs it -- nobody sets `receiving`, and the env cannot be constructed.  Three
 * network devices (sensor 0, controller 1, actuator 2 -- not assignable) and the RRM; the sensor queues the plant angle
 * every counter tick and the plant then advances one substep x <- A x + B u; every ctrl_period_ticks from ctrl_start_tick on
 * the controller runs the reference's three-term PID rule on gains of its env's own (gw_ctrl_set_gains, below); their default,
 * the reference's shipped gains kp = 1, ki = kd = 0, queues -angle_deg unless the angle is 0; packets decoded by
 * their destination's receive-mode MAC are handed up (controller: angle := degrees(value); actuator: u := value);
 * observation and reward as InvertedPendulumInterpreter computes them.  Checked bit for bit against an event-driven
 * model of the same rules; parity with the reference is unpinned by construction. */
typedef struct gw_ctrl_config {
    gw_config net;                          /* num_devices must be 3; geometry, radio constants, counter_interval */
    double  A[16], B[4];                    /* one-substep plant matrices (row-major), substep = counter_interval */
    double  x0[4], u0;                      /* initial plant state {wagon pos, wagon vel, angle, angle rate}, initial input */
    int32_t ctrl_start_tick;                /* first control tick */
    int32_t ctrl_period_ticks;              /* control period in ticks (10 = the reference's 10 ms) */
} gw_ctrl_config;

typedef struct gw_ctrl gw_ctrl;

int gw_ctrl_config_default(gw_ctrl_config* cfg, int64_t num_envs);
int gw_ctrl_create(const gw_ctrl_config* cfg, gw_ctrl** out);
int gw_ctrl_destroy(gw_ctrl* c);
/* one env.step() of every env: device in {0 sensor, 1 controller}, duration in [0, max_duration); angle_deg_dev may be NULL */
int gw_ctrl_step(gw_ctrl* c, const int32_t* device_dev, const int32_t* duration_dev, int32_t* obs_dev, float* reward_dev,
                 double* angle_deg_dev, void* stream);
/* host copies: "now","wake","u","angle_deg" f64[N] | "x" f64[N][4] | "rx_power" f64[N][4] | "qlen" int32[N][2] |
 *              "received" u32[N][2] (controller, actuator) | "n_tx","commands","substeps","flags" u32[N] |
 *              "age" u32[N], "cost" f64[N] (the running episode's record) | "x_init" f64[N][4], "u_init" f64[N] |
 *              "gains" f64[N][3] {kp, ki, kd}, "last_error" f64[N] (the controller, gw_ctrl_set_gains) |
 *              "disturbance" f64[N][4], "noise_key" u64[N], "noise_count" u64[N] (the plant's, gw_ctrl_set_disturbance) |
 *              "loss" u32[N][4], "loss_key" u64[N], "loss_count" u64[N], "lost" u32[N][4] (the links', gw_ctrl_set_loss) */
int gw_ctrl_get_state(gw_ctrl* c, const char* field, void* dst_host, size_t bytes);

/* Per-env initial state and reset.  Every env keeps an initial state of its own (x_init, u_init; cfg.x0 / cfg.u0 at create) and
 * the record of its running episode: age (steps taken) and cost (sum of |angle in degrees| the steps reported), both 0 at create.
 * gw_ctrl_set_initial stores x0_dev f64[N][4] (and u0_dev f64[N] unless NULL) for the envs with mask_dev[e] != 0 (NULL: all);
 * it changes no env's running state.  gw_ctrl_reset puts the masked envs into exactly the state gw_ctrl_create leaves, with the
 * env's own initial state: clock, wake and tick 0, controller angle 0, both queues empty (head = len = 0), noise states 0,
 * received, n_tx, commands, substeps, age, cost and the controller's last_error 0.  flags are sticky and stay, and so do the
 * gains, the plant's disturbance record (g, key and the count n) and the links' loss record (thr, key, n and lost).  Envs
 * outside the mask are untouched, bit for bit.
 * obs_dev (NULL ok) receives (int32) degrees(x[2]) of all N envs. */
int gw_ctrl_set_initial(gw_ctrl* c, const double* x0_dev, const double* u0_dev, const uint8_t* mask_dev, void* stream);
int gw_ctrl_reset(gw_ctrl* c, const uint8_t* mask_dev, int32_t* obs_dev, void* stream);

/* The controller: control() of control/inverted_pendulum.py:46-69, on gains {kp, ki, kd} and a last_error that every env holds
 * of its own, all f64; {1, 0, 0} (the reference's shipped gains) and 0 at create.  At a control tick -- a tick at or after
 * ctrl_start_tick whose (tick - ctrl_start_tick) % ctrl_period_ticks is 0 -- with ang the controller's angle in degrees:
 *     e    = fabs(ang)                                              abs(sp - angle), sp = 0
 *     pid  = ((kp * e) + (ki * (e + last))) + (kd * (e - last))     this association, no contraction
 *     last = e                                                      also when nothing is sent
 *     if (ang != 0.0) queue (ang < 0.0 ? pid : -pid) for the actuator, commands += 1
 * ki * (e + last) is the reference's term as written, not an integral.  Before ctrl_start_tick nothing is evaluated and last
 * stays.  With (1, 0, 0) the queued value is -ang bit for bit wherever e + last is finite; a NaN ang queues -pid, a NaN.  No
 * gain is validated: any f64 has this one meaning.  A reset (gw_ctrl_reset, or the end of an episode inside a rollout) puts
 * last_error back to 0 and leaves the gains.
 * gw_ctrl_set_gains stores gains_dev f64[N][3] = {kp, ki, kd} for the envs with mask_dev[e] != 0 (NULL: all); it touches no
 * running state, last_error included, is stream-ordered and allocates nothing.  A NULL c or gains_dev: GW_EINVAL before any
 * device call.  A handle on which it has never been called launches kernels with the default gains compiled in, which read
 * no gains; its first call switches the handle, for good, to the kernels that read them.  Results do not depend on which
 * kernels run: a handle set to (1, 0, 0) computes what an unswitched one computes, and its last_error moves. */
int gw_ctrl_set_gains(gw_ctrl* c, const double* gains_dev, const uint8_t* mask_dev, void* stream);

/* Plant disturbance: seeded, counter-based noise on the plant's state, per env.  BUILDER-DEFINED, as the whole loop is.  Every
 * env holds a record of 48 bytes {g[4] f64, key u64, n u64}, all 0 at create.  On a handle on which gw_ctrl_set_disturbance has
 * been called, every counter tick runs the plant substep nx = A x + B u as before and then ends with, all integers mod 2^64:
 *     z  = key ^ (n * 0xD1B54A32D192ED03)
 *     z += 0x9E3779B97F4A7C15
 *     z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z ^= z >> 31
 *     w  = (double)(int32_t)(uint32_t)(z >> 32) * 0x1p-31          uniform on [-1, 1), a multiple of 2^-31, every operation exact
 *     x[i] = nx[i] + g[i] * w      for i = 0..3                    the product rounded, then the sum; no contraction
 *     n += 1
 * n counts the substeps since the env's record was last set, and nothing else restarts it: gw_ctrl_reset and the reset at an
 * episode's end inside a rollout leave g, key and n alone -- a reset env is a fresh env whose plant goes on drawing where the old
 * one stopped (else every episode of an env would replay one noise sequence).  n lives in the handle: two calls of K / 2 steps
 * equal one of K.  The draw depends on (key, n) alone, so two envs with equal key, g, gains, initial state and actions walk
 * bit-identical trajectories wherever they sit in the batch; giving env j of every candidate the same key compares candidates on
 * common random numbers.  With g = 0 the rule adds +-0: it may turn a -0.0 of the plant into +0.0 and changes nothing else.
 * gw_ctrl_set_disturbance stores g_dev f64[N][4] and key_dev u64[N] and sets n = 0 for the envs with mask_dev[e] != 0 (NULL:
 * all); other envs are untouched, bit for bit, and so is all other running state.  Stream-ordered; allocates nothing.  A NULL
 * c, g_dev or key_dev: GW_EINVAL before any device call.  No value is validated: any f64 has the one meaning the rule gives it.
 * A handle on which it has never been called launches exactly the kernels it launched before; its first call switches the
 * handle, for good, to the disturbance instantiations of the step, rollout, schedule and both feedback kernels, which are PID
 * instantiations as well (the gains are what gw_ctrl_set_gains last stored, {1, 0, 0} if it never did). */
int gw_ctrl_set_disturbance(gw_ctrl* c, const double* g_dev, const uint64_t* key_dev, const uint8_t* mask_dev, void* stream);

/* Packet loss: seeded, counter-based erasures per env and link.  BUILDER-DEFINED, as the whole loop is.  Every env holds a loss
 * record of 48 bytes, 16-byte aligned, all 0 at create:
 *     struct { uint32_t thr[4]; uint64_t key; uint64_t n; uint32_t lost[4]; }
 *     links: 0 RRM -> sensor (the announcement of a step with device 0)     2 sensor -> controller (data)
 *            1 RRM -> controller (the announcement, device 1)               3 controller -> actuator (data)
 * On a handle on which gw_ctrl_set_loss has been called, every transmission of a step -- the announcement first, then each data
 * packet, in the order they go on the air -- takes exactly one draw, whatever the PHY decides about the transmission; all
 * integers mod 2^64:
 *     z  = key ^ (n * 0xA0761D6478BD642F)       an odd constant of its own: the disturbance and the loss under one key do not
 *     z += 0x9E3779B97F4A7C15                   draw the same sequence; then the disturbance's mixer
 *     z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z ^= z >> 31
 *     r  = (uint32_t)(z >> 32)
 *     erased = r < thr[link]                    probability thr * 2^-32: thr = 0 never, thr = 0xFFFFFFFF all but one draw in 2^32
 *     if (erased) lost[link] += 1               wraps; counted whatever the PHY decided
 *     n += 1
 *     outcome = (what the PHY decided) && !erased
 * An erased announcement is an ungranted step: nothing is sent, the counter ticks run to the step's end and the queues keep
 * their packets.  An erased data packet has been popped and sent -- n_tx counts it and every other radio's noise state moves as
 * before -- and is not delivered: neither the controller's angle nor the plant's input, neither count of "received" moves.  The
 * flags the PHY's decision sets are set as before; a step flagged GW_FLAG_BADACT sends nothing and draws nothing.
 * n counts the transmissions since the env's record was last set, and nothing else restarts it: gw_ctrl_reset and the reset at
 * an episode's end inside a rollout leave thr, key, n and lost alone, for the disturbance's reason.  n lives in the handle: two
 * calls of K / 2 steps equal one of K.  Two envs with equal loss records, disturbance, gains, initial state and actions walk
 * bit-identical trajectories wherever they sit in the batch.
 * gw_ctrl_set_loss stores thr_dev u32[N][4] and key_dev u64[N] and sets n = 0 and lost = 0 for the envs with mask_dev[e] != 0
 * (NULL: all); other envs are untouched, bit for bit, and so is all other running state.  Stream-ordered; allocates nothing.  A
 * NULL c, thr_dev or key_dev: GW_EINVAL before any device call.  No value is validated.
 * A handle on which it has never been called launches exactly the kernels it launched before; its first call switches the
 * handle, for good, to the loss instantiations of the step, rollout, schedule and both feedback kernels, which are disturbance
 * and PID instantiations as well: gains and g stay at what was last stored ({1, 0, 0} and 0 if never).  So a handle switched by
 * gw_ctrl_set_loss alone runs the disturbance rule at g = 0, which may turn a -0.0 of the plant into +0.0 and changes nothing
 * else.  At thr = 0 a switched handle computes, bit for bit, what a handle switched by gw_ctrl_set_disturbance computes; its n
 * still counts transmissions. */
int gw_ctrl_set_loss(gw_ctrl* c, const uint32_t* thr_dev, const uint64_t* key_dev, const uint8_t* mask_dev, void* stream);

typedef struct gw_ctrl_episodes {
    int32_t max_steps;                      /* an episode ends when its age reaches this; 0: no limit */
    int32_t pad;
    double  fail_deg;                       /* ... or when |angle in degrees| exceeds this; <= 0: no limit */
} gw_ctrl_episodes;

/* K = steps calls of gw_ctrl_step in one launch: step k reads device_dev / duration_dev [k][N] and writes obs_dev, reward_dev,
 * angle_deg_dev (NULL ok) [k][N].  ep == NULL: outputs and every state field equal `steps` calls of gw_ctrl_step bit for bit
 * (an action outside the action space is flagged and skipped as there; age and cost do not move).  With ep: after each step
 * age += 1 and cost += fabs(deg) (deg: the f64 angle the step reports; one running f64 sum per env in step order); the env has
 * ended if fail_deg > 0 && fabs(deg) > fail_deg (bit 1 of ended_dev[k][e]) or max_steps > 0 && age == max_steps (bit 0); the
 * step's own outputs are written, then the env is reset inside the launch exactly as gw_ctrl_reset resets it (a flagged and
 * skipped step reports the unchanged angle and counts like any other).  age and cost
 * live in the handle: two calls of K/2 steps equal one call of K.  ended_dev is required iff ep.  steps == 0: GW_OK, no launch;
 * steps < 0, a NULL pointer, ep->max_steps < 0: GW_EINVAL before any device call. */
int gw_ctrl_rollout(gw_ctrl* c, int32_t steps, const int32_t* device_dev, const int32_t* duration_dev, const gw_ctrl_episodes* ep,
                    int32_t* obs_dev, float* reward_dev, double* angle_deg_dev, uint8_t* ended_dev, void* stream);

/* P cyclic schedules evaluated in one launch, nothing stored per step.  sched_dev: u8[P][L][2] = {device, duration}; env e follows
 * schedule e / (N / P) and acts on its entry age % L (a reset restarts the schedule).  A byte outside the action space is clamped
 * where it is read: device to {0, 1}, duration to [0, max_duration - 1].  Episodes as in gw_ctrl_rollout (ep is required).
 * tally_dev f64[N][4] is overwritten per env: {episodes ended, of those by fail_deg, steps taken, sum of the costs of the ended
 * episodes} -- per env, not per schedule: deterministic, no f64 atomics; the [P] reduction is the caller's.
 * 1 <= L <= 64, P >= 1 (else GW_EINVAL); N % P == 0 and (N / P) % 64 == 0 (else GW_EUNSUPPORTED): every 64-env block then
 * follows one schedule.  Refusals come before any launch. */
int gw_ctrl_rollout_schedules(gw_ctrl* c, int32_t steps, const uint8_t* sched_dev, int32_t P, int32_t L, const gw_ctrl_episodes* ep,
                              double* tally_dev, void* stream);

/* P angle-feedback band schedulers evaluated in one launch: before each step the env looks at its own pendulum and picks, by the
 * angle, which of B cyclic schedules it acts on.  Step k of env e, with p = e / (N / P):
 *   1. deg = x[2] * (180.0 / 3.141592653589793) of the env's CURRENT state -- the angle its last step reported, or that of its
 *      own x_init where the previous step ended an episode: the value gw_ctrl_reset reports.
 *      o = (int32_t) fmin(fmax(deg, -1e9), 1e9): the observation for every |deg| < 1e9, and defined beyond (NaN gives -1e9).
 *      key = (flags & GW_CTRL_FB_ABS) ? |o| : o.
 *   2. bin = #{ j < B - 1 : edges[p][j] <= key }.  The edges need not be sorted: any content has this one meaning.
 *   3. the action is entry age % L of sched[p][bin], age being the running episode's age in the handle; a byte outside the
 *      action space is clamped where it is read as in gw_ctrl_rollout_schedules (device to {0, 1}, duration to
 *      [0, max_duration - 1]), so no step is ever flagged GW_FLAG_BADACT.
 *   4. the step and the episode rule run exactly as gw_ctrl_rollout with ep runs them for that action (ep is required): age,
 *      cost, both ending bits, the in-launch reset to a fresh env of its own x_init / u_init.
 *   5. with rows: row k receives the action taken and what gw_ctrl_rollout would write (angle_deg_dev may be NULL).
 *   6. tally_dev f64[N][GW_CTRL_FB_COLS] is overwritten per env, one running f64 each in step order: columns 0-3 are
 *      gw_ctrl_rollout_schedules' four; 4 the sum of the durations assigned; 5 `elapsed`, the sum of dt, dt being the env's
 *      clock after the step, BEFORE any reset, minus its clock before the step; 6 area = area + fabs(deg_k) * dt with deg_k
 *      the angle the step reports; 7 the steps taken in bin 0.  A policy's time-weighted mean error is sum(col 6) / sum(col 5),
 *      its airtime per second sum(col 4) / sum(col 5); the [P] reduction is the caller's.
 * No handle state is added: two calls of K/2 leave the state, and write the rows, of one call of K.  The policies are read
 * stream-ordered from device memory when the launch runs; they are never validated and never read back.
 * GW_EINVAL: a NULL c / fb / ep / tally_dev / sched_dev, edges_dev NULL with B > 1, a NULL required pointer in rows, steps < 0,
 * max_steps < 0, P < 1, B outside [1, GW_CTRL_FB_MAX_BINS], L outside [1, 64] -- before any device call and, as in
 * gw_ctrl_rollout_schedules, before steps == 0 is looked at.  steps == 0 is then GW_OK with no launch, the handle not read and
 * the tally untouched.  GW_EUNSUPPORTED, state untouched, before any device call: N % P != 0 or (N / P) % 64 != 0 (every 64-env
 * block follows one policy). */
#define GW_CTRL_FB_MAX_BINS 8
#define GW_CTRL_FB_COLS     8
#define GW_CTRL_FB_ABS      1      /* flags: the key is |o| instead of o */
typedef struct gw_ctrl_feedback {
    int32_t num_policies;          /* P >= 1; env e follows policy e / (N / P) */
    int32_t num_bins;              /* B in [1, GW_CTRL_FB_MAX_BINS] */
    int32_t length;                /* L in [1, 64] */
    int32_t flags;                 /* GW_CTRL_FB_ABS or 0 */
    const int32_t* edges_dev;      /* int32[P][B - 1]; may be NULL iff B == 1 */
    const uint8_t* sched_dev;      /* uint8[P][B][L][2] = {device, duration} */
} gw_ctrl_feedback;
typedef struct gw_ctrl_feedback_rows {   /* all [steps][N]; angle_deg_dev may be NULL, the others not */
    int32_t *device_out_dev, *duration_out_dev, *obs_dev;
    float* reward_dev; double* angle_deg_dev; uint8_t* ended_dev;
} gw_ctrl_feedback_rows;
int gw_ctrl_rollout_feedback(gw_ctrl* c, int32_t steps, const gw_ctrl_feedback* fb, const gw_ctrl_episodes* ep,
                             const gw_ctrl_feedback_rows* rows /* NULL: nothing stored per step */,
                             double* tally_dev /* f64[N][GW_CTRL_FB_COLS], overwritten, never NULL */, void* stream);

/* Host-only self-test hook (no GPU needed): fuzzes the MAC-queue encoding the default kernel uses
 * against an explicit deque(maxlen=100).  Returns the number of mismatches (0 = identical). */
int gw_selftest_queue(uint64_t seed, int32_t operations, int32_t mult, int32_t counter_bound);

/* Host-only: the same fuzz for the run-length queues of the generic kernel (GW_CFG_EXPLICIT_QUEUE, csrc/gw_runq.h): counter ticks,
 * resets, pops and arbitrary gw_enqueue packets; mult up to GW_QUEUE_CAP.  Returns the number of mismatches. */
int gw_selftest_runq(uint64_t seed, int32_t operations, int32_t mult, int32_t counter_bound);

/* Host-only: bit mask of the exact arithmetic fast paths gw_create enables for cfg after validating
 * them (1 slot remainder, 2 division by the data rate, 4 integer decode decision, 8 idempotent
 * noise-state map, 16 counter ticks counted in one jump); negative on error.  max_noise_states may be NULL. */
int gw_selftest_fastmath(const gw_config* cfg, int32_t* max_noise_states);

/* Test hook: the step / rollout kernel instantiations launched by this handle since gw_create (env != NULL), or by the whole
 * process (env == NULL), one line each: "<kernel><template args> <count>\n", spelled as c++filt prints the kernel's symbol,
 * e.g. "ct_step_sfx_kernel<4, 2> 37".  A launch captured into a hipGraph counts once, however often it is replayed.
 * Writes at most cap bytes incl. the NUL (out may be NULL when cap is 0); returns the length needed without the NUL,
 * negative on error. */
int64_t gw_selftest_launches(gw_env* env, char* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GYMWIPE_AMD_H */
