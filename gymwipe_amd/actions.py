"""
Counter-based synthetic action streams (SURVEY.md 8d "synthetic inputs").

The env is deterministic (the reference never uses its seeded ``np_random``, envs/core.py:46-52), so
"synthetic traffic" means action streams only.  The action of env ``e`` at step ``k`` is a pure function
of ``(seed, e, k)``:

    h        = splitmix64(seed ^ (e * 0x9E3779B97F4A7C15) ^ (k * 0xD1B54A32D192ED03))
    device   = (h & 0xffffffff) % num_devices
    duration = (h >> 32)        % max_duration

so the GPU (torch int64 arithmetic, wrapping) and the CPU baseline (numpy uint64) draw IDENTICAL streams
without storing or exchanging them, and a rank generates the actions of its own shard from global env ids.
"""
import numpy as np

_M64 = (1 << 64) - 1
_G1, _G2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _i64(x):
    """Python int (mod 2^64) -> the int64 with the same bit pattern."""
    x &= _M64
    return x - (1 << 64) if x >= (1 << 63) else x


def actions_numpy(seed, env_lo, env_hi, step_lo, step_hi, num_devices, max_duration=20):
    """(device, duration) int32[steps][envs] for envs [env_lo, env_hi) and steps [step_lo, step_hi)."""
    e = np.arange(env_lo, env_hi, dtype=np.uint64)[None, :]
    k = np.arange(step_lo, step_hi, dtype=np.uint64)[:, None]
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) ^ (e * np.uint64(_G1)) ^ (k * np.uint64(_G2))
        z = z + np.uint64(_G1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
        z = z ^ (z >> np.uint64(31))
    dev = ((z & np.uint64(0xffffffff)) % np.uint64(num_devices)).astype(np.int32)
    dur = ((z >> np.uint64(32)) % np.uint64(max_duration)).astype(np.int32)
    return dev, dur


def actions_torch(seed, env_lo, env_hi, step_lo, step_hi, num_devices, max_duration=20, device="cpu"):
    """Same stream as :func:`actions_numpy`, evaluated with torch on ``device`` (int64, wrapping)."""
    import torch

    def lsr(x, s):                                    # logical shift right on int64
        return (x >> s) & ((1 << (64 - s)) - 1)

    e = torch.arange(env_lo, env_hi, dtype=torch.int64, device=device)[None, :]
    k = torch.arange(step_lo, step_hi, dtype=torch.int64, device=device)[:, None]
    z = (e * _i64(_G1)) ^ (k * _i64(_G2)) ^ _i64(seed)
    z = z + _i64(_G1)
    z = (z ^ lsr(z, 30)) * _i64(_C1)
    z = (z ^ lsr(z, 27)) * _i64(_C2)
    z = z ^ lsr(z, 31)
    dev = ((z & 0xffffffff) % num_devices).to(torch.int32)
    dur = (lsr(z, 32) % max_duration).to(torch.int32)
    return dev.contiguous(), dur.contiguous()


# ---- policies over the last observation (gw_rollout_policy, include/gymwipe_amd.h) -------------------------------------------
# The agent sees counter_bound + payload_value * {-1, 0, +1}, so a policy over the last observation is three rows of
# probabilities over the A = num_devices * max_duration flat actions (agents/dqn_counter_traffic.py:25-31).  The kernels draw
# from a table of cumulative sums in 32-bit fixed point:
#     u = min(h & 0xffffffff, 0xfffffffe)      h: the stream above, at (seed, env, step)
#     a = min(A - 1, #{ j : cdf[cls][j] <= u })
def policy_cdf(p):
    """Probabilities ``[..., A]`` (numpy array or torch tensor, on whichever device it lives) -> the table of
    :func:`policy_sample_numpy` / ``gw_rollout_policy``: ``floor(2^32 * cumsum_f64(p))`` clipped to ``2^32 - 1``, and
    ``0xffffffff`` from the last action with ``p > 0`` onwards.  An action with ``p == 0`` gets ``cdf[j] == cdf[j - 1]``
    (0 for ``j == 0``) and is never drawn; ``u <= 0xfffffffe`` never reaches past the last action with ``p > 0``.
    numpy's cumsum adds in sequence, which gives both properties by itself.  ``torch.cumsum`` on a GPU is a parallel scan:
    two neighbouring prefixes may be summed in different orders and differ by an ulp, so there the entries of ``p == 0``
    actions are taken from their predecessor and the row is made non-decreasing explicitly (a running maximum); an entry with
    ``p > 0`` may still differ by 1 from the numpy table's.
    numpy in: uint32 out.  torch in: int64 out on the same device (no host sync; ``rollout_policy`` stores it as 32-bit words)."""
    if isinstance(p, np.ndarray) or not hasattr(p, "cumsum") or not hasattr(p, "device"):
        p = np.asarray(p, dtype=np.float64)
        A = p.shape[-1]
        v = np.minimum(np.floor(np.cumsum(p, axis=-1, dtype=np.float64) * 4294967296.0), 4294967295.0)
        idx = np.arange(A)
        last = np.where(p > 0, idx, -1).max(axis=-1, keepdims=True)
        return np.where(idx >= last, 4294967295.0, v).astype(np.uint32)
    import torch
    A = p.shape[-1]
    v = torch.floor(torch.cumsum(p.to(torch.float64), dim=-1) * 4294967296.0).clamp(max=4294967295.0)
    v = torch.cummax(torch.where(p > 0, v, torch.zeros_like(v)), dim=-1).values     # p == 0: the predecessor's entry
    idx = torch.arange(A, device=p.device)
    last = torch.where(p > 0, idx, torch.full_like(idx, -1)).max(dim=-1, keepdim=True).values
    return torch.where(idx >= last, torch.full_like(v, 4294967295.0), v).to(torch.int64)


def policy_u_numpy(seed, env_lo, env_hi, step):
    """The draw's uniform 32-bit number for envs [env_lo, env_hi) at stream position ``step``."""
    e = np.arange(env_lo, env_hi, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) ^ (e * np.uint64(_G1)) ^ (np.uint64(step & _M64) * np.uint64(_G2))
        z = z + np.uint64(_G1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
        z = z ^ (z >> np.uint64(31))
    return np.minimum(z & np.uint64(0xffffffff), np.uint64(0xfffffffe)).astype(np.uint32)


def policy_count_numpy(cdf, cls, u):
    """``min(A - 1, #{ j : cdf[cls[i]][j] <= u[i] })`` for every i (rows non-decreasing)."""
    cdf = np.asarray(cdf, dtype=np.uint32)
    A = cdf.shape[-1]
    a = np.empty(len(u), np.int64)
    for c in range(cdf.shape[0]):
        sel = cls == c
        a[sel] = np.searchsorted(cdf[c], u[sel], side="right")
    return np.minimum(a, A - 1)


def policy_sample_numpy(seed, env_lo, env_hi, step, cdf, obs, counter_bound, max_duration):
    """CPU restatement of the kernels' draw: ``(device, duration)`` int32[envs] for envs [env_lo, env_hi) at stream position
    ``step`` (= step0 + k), acting on the observations ``obs`` int32[envs] with the table ``cdf`` uint32[3][A]."""
    obs = np.asarray(obs).astype(np.int64)
    cls = np.sign(obs - int(counter_bound)).astype(np.int64) + 1
    a = policy_count_numpy(cdf, cls, policy_u_numpy(seed, env_lo, env_hi, step))
    dev = a // int(max_duration)
    return dev.astype(np.int32), (a - dev * int(max_duration)).astype(np.int32)


def policy_sample_population_numpy(seed, env_lo, env_hi, step, cdfs, envs_per_policy, obs, counter_bound, max_duration):
    """CPU restatement of ``gw_rollout_population``'s draw: :func:`policy_sample_numpy` for a slice of a population -- env
    index ``i`` of the slice (0 for ``env_lo``: the env's index in its handle) draws from table ``i // envs_per_policy`` of
    ``cdfs`` uint32[P][3][A], with the hash ids of ``[env_lo, env_hi)``: ``env_lo`` shifts the stream, not the policy index."""
    cdfs = np.asarray(cdfs, dtype=np.uint32)
    obs = np.asarray(obs)
    n, M = int(env_hi) - int(env_lo), int(envs_per_policy)
    if cdfs.ndim != 3 or cdfs.shape[1] != 3 or M < 1 or n != cdfs.shape[0] * M or obs.shape != (n,):
        raise ValueError("cdfs must be [P][3][A] with P * envs_per_policy == env_hi - env_lo == len(obs)")
    dev, dur = np.empty(n, np.int32), np.empty(n, np.int32)
    for p in range(cdfs.shape[0]):
        lo, hi = p * M, (p + 1) * M
        dev[lo:hi], dur[lo:hi] = policy_sample_numpy(seed, env_lo + lo, env_lo + hi, step, cdfs[p], obs[lo:hi], counter_bound,
                                                     max_duration)
    return dev, dur


# ---- the table of a closed loop (gw_rollout_policy_stats / gw_transition_stats, include/gymwipe_amd.h) -----------------------
TS_COLS = 7                     # n, r_sum, r_sq, next below / at / above the bound, done
TSD_COLS = 8                    # ... and the sum of min(delivered, TSD_DELIVERED_MAX): the _delivered calls' table (GW_TSD_COLS)
TSD_DELIVERED_MAX = 65535


def transition_stats_numpy(obs_prev, device, duration, obs, reward, done, center, max_duration, num_devices, ended=None,
                           delivered=None):
    """CPU restatement of both entry points' table: ``int64[3][A][TS_COLS]`` over (observation class, flat action) from
    recorded transitions ``[steps][N]``.  Step k's observation seen is ``obs_prev`` for k = 0 and row k - 1 of ``obs``
    afterwards -- or, with ``ended`` (``[steps][N]``, what ``rollout_episodes`` records: gw_transition_stats_ep), ``center``
    where ``ended[k - 1] != 0``: the env was reset and acted on the reset's observation.
    ``cls = sign(obs_seen - center) + 1``, ``a = device * max_duration + duration``.  Columns: transitions,
    reward sum, reward-square sum, next observation below / at / above ``center``, ``done != 0``.  A row whose action lies
    outside the action space is skipped (the env did nothing in that step); a reward is rounded to nearest (ties to even) and
    clamped to [-10, 10], anything that is not a number counting as -10.
    ``delivered`` (``[steps][N]`` integers, what the scored calls record: gw_transition_stats_delivered): the table is
    ``int64[3][A][TSD_COLS]``, its eighth column the sum of the counts, each clamped to ``[0, TSD_DELIVERED_MAX]``."""
    md, D = int(max_duration), int(num_devices)
    A = D * md
    dev = np.asarray(device).astype(np.int64)
    dur = np.asarray(duration).astype(np.int64)
    nxt = np.asarray(obs).astype(np.int64)
    steps = dev.shape[0]
    table = np.zeros((3, A, TS_COLS if delivered is None else TSD_COLS), np.int64)
    if steps == 0:
        return table
    after = nxt[:-1] if ended is None else np.where(np.asarray(ended)[:-1] != 0, int(center), nxt[:-1])
    seen = np.concatenate([np.asarray(obs_prev).astype(np.int64).reshape(1, -1), after])
    with np.errstate(invalid="ignore"):
        x = np.rint(np.asarray(reward, dtype=np.float64))
        x = np.where(x >= -10.0, x, -10.0)               # (a NaN fails the comparison)
        r = np.where(x <= 10.0, x, 10.0).astype(np.int64)
    ok = (dev >= 0) & (dev < D) & (dur >= 0) & (dur < md)
    row = ((np.sign(seen - int(center)) + 1) * A + dev * md + dur)[ok]
    ncl = (np.sign(nxt - int(center)) + 1)[ok]
    r = r[ok]
    dn = (np.asarray(done)[ok] != 0).astype(np.int64)
    flat = table.reshape(3 * A, table.shape[-1])
    np.add.at(flat[:, 0], row, 1)
    np.add.at(flat[:, 1], row, r)
    np.add.at(flat[:, 2], row, r * r)
    np.add.at(flat, (row, 3 + ncl), 1)
    np.add.at(flat[:, 6], row, dn)
    if delivered is not None:
        np.add.at(flat[:, 7], row, np.clip(np.asarray(delivered).astype(np.int64), 0, TSD_DELIVERED_MAX)[ok])
    return table


def table_score(table, score, max_duration):
    """The score sum of every bin of an eight-column table under ``score`` (``make_score``'s image): int64 ``[3][A]``,
    ``score[0] * table[..., 1] + score[1 + a // max_duration] * table[..., 7]``.  A step's score is linear in its reward and in
    the packets it delivered, and the flat action names the sender whose weight applies, so the sums of the two are all the
    table has to carry -- whichever score is applied afterwards.  ``table``: a numpy array or a torch tensor (the result lives
    where it does)."""
    score = np.asarray(score)
    if score.shape != (1 + MAX_DEVICES,):
        raise ValueError("score must be make_score()'s int32[%d]" % (1 + MAX_DEVICES))
    if table.ndim != 3 or table.shape[0] != 3 or table.shape[2] != TSD_COLS:
        raise ValueError("table must be [3][A][%d], got %s" % (TSD_COLS, tuple(table.shape)))
    A, md = int(table.shape[1]), int(max_duration)
    if md < 1 or A % md or A // md > MAX_DEVICES:
        raise ValueError("table_score: %d actions are not num_devices x max_duration %d" % (A, md))
    w = score.astype(np.int64)
    w_sender = w[1 + np.arange(A) // md]
    if isinstance(table, np.ndarray):
        return int(w[0]) * table[..., 1].astype(np.int64) + w_sender[None, :] * table[..., 7].astype(np.int64)
    import torch
    t = table.to(torch.int64)
    return int(w[0]) * t[..., 1] + torch.from_numpy(w_sender).to(t.device)[None, :] * t[..., 7]


# ---- episodes inside a closed loop (gw_rollout_episodes, include/gymwipe_amd.h) -------------------------------------------------
EP_COLS = 5                     # episodes ended, of those by done, sum of lengths, sum of returns, sum of returns^2


def episodes_numpy(state, reward, done, max_steps, on_done):
    """The per-step bookkeeping of ``gw_rollout_episodes`` after one step of every env: ``state`` int32[N][2] ``{age, ret}``
    is updated in place (``age += 1; ret += reward``, both back to 0 where the episode ended); returns ``(ended, tally)`` --
    ``ended`` uint8[N]: 1 where the step returned ``done`` and ``on_done`` is set, else 2 where ``max_steps > 0`` and the
    episode has reached ``max_steps`` steps, else 0 (done wins over the step limit); ``tally`` int64[EP_COLS]: what the ended
    episodes add.  The caller resets the envs with ``ended != 0``; they act on the reset's observation next."""
    assert state.dtype == np.int32 and state.ndim == 2 and state.shape[1] == 2
    state[:, 0] += 1
    state[:, 1] += np.asarray(reward).astype(np.int32)
    by_done = (np.asarray(done) != 0) if on_done else np.zeros(len(state), bool)
    by_limit = (state[:, 0] >= int(max_steps)) if int(max_steps) > 0 else np.zeros(len(state), bool)
    ended = np.where(by_done, 1, np.where(by_limit, 2, 0)).astype(np.uint8)
    over = ended != 0
    age, ret = state[over, 0].astype(np.int64), state[over, 1].astype(np.int64)
    tally = np.array([over.sum(), (ended == 1).sum(), age.sum(), ret.sum(), (ret * ret).sum()], np.int64)
    state[over] = 0
    return ended, tally


# ---- episodes scored by what they delivered (gw_rollout_episodes_scored, include/gymwipe_amd.h) ---------------------------------
MAX_DEVICES = 32                # GW_MAX_DEVICES
SCORE_W_MAX = 1024              # GW_SCORE_W_MAX


def make_score(num_devices, reward=1, delivered=0):
    """The ``int32[1 + MAX_DEVICES]`` image of ``gw_score``: ``[0]`` the weight of a step's built-in reward, ``[1 + d]`` the
    weight of ONE data packet of sender ``d`` that the RRM decoded in the step (0 from ``num_devices`` on).  ``delivered``: one
    weight for every sender, or a sequence of ``num_devices``.  Every weight is an integer in ``[-SCORE_W_MAX, SCORE_W_MAX]``.
    ``make_score(D)`` is the neutral score: the scored calls then give their parents' results."""
    D = int(num_devices)
    if not 2 <= D <= MAX_DEVICES:
        raise ValueError("make_score: num_devices must be in [2, %d]" % MAX_DEVICES)
    w = np.asarray(delivered)
    if w.ndim == 0:
        w = np.full(D, w)
    if w.shape != (D,):
        raise ValueError("make_score: delivered must be a scalar or a sequence of %d weights, got shape %s" % (D, w.shape))
    vals = np.concatenate([np.asarray(reward).reshape(1), w])
    if vals.dtype.kind not in "iu" and not (np.isfinite(vals.astype(np.float64)).all() and (vals == np.rint(vals.astype(np.float64))).all()):
        raise ValueError("make_score: weights must be integers")
    vals = vals.astype(np.int64)
    if (np.abs(vals) > SCORE_W_MAX).any():
        raise ValueError("make_score: a weight lies outside [-%d, %d]" % (SCORE_W_MAX, SCORE_W_MAX))
    out = np.zeros(1 + MAX_DEVICES, np.int32)
    out[:1 + D] = vals
    return out


def score_numpy(score, reward, device, delivered):
    """CPU restatement of a step's score: ``score[0] * reward + score[1 + device] * delivered`` per env, int32 (``reward``: the
    built-in interpreter's, an integer in [-10, 10] in any dtype; ``device``: the sender each step assigned; ``delivered``: the
    data packets of that sender the RRM decoded in the step)."""
    score = np.asarray(score)
    if score.shape != (1 + MAX_DEVICES,):
        raise ValueError("score must be make_score()'s int32[%d]" % (1 + MAX_DEVICES))
    w = score.astype(np.int64)
    r = np.rint(np.asarray(reward, dtype=np.float64)).astype(np.int64)
    return (w[0] * r + w[1 + np.asarray(device).astype(np.int64)] * np.asarray(delivered).astype(np.int64)).astype(np.int32)


# ---- a queue-aware scheduler inside the rollout (gw_rollout_backlog, include/gymwipe_amd.h) --------------------------------------
QUEUE_CAP = 100                 # GW_QUEUE_CAP
BACKLOG_BYTES = 4 * MAX_DEVICES + QUEUE_CAP + 1


def make_backlog_policy(num_devices, weights=1, duration_of_len=None, max_duration=20):
    """The ``uint8[BACKLOG_BYTES]`` image of ``gw_backlog_policy``: ``MAX_DEVICES`` little-endian int32 weights -- sender i's
    priority is ``weights[i] * qlen_i``, each weight an integer in ``[0, SCORE_W_MAX]``, 0 from ``num_devices`` on -- then the
    duration for a chosen sender whose queue holds ``L`` packets, ``L`` in ``[0, QUEUE_CAP]``, one byte each (the call clamps
    it to ``max_duration - 1``).  ``weights``: one for every sender, or a sequence of ``num_devices``.  ``duration_of_len``:
    ``QUEUE_CAP + 1`` values in ``[0, 255]``; the default is ``min(max_duration - 1, 4 * L)``.  With the defaults: the band
    goes to the longest queue for as long as its backlog needs."""
    D = int(num_devices)
    if not 2 <= D <= MAX_DEVICES:
        raise ValueError("make_backlog_policy: num_devices must be in [2, %d]" % MAX_DEVICES)
    w = np.asarray(weights)
    if w.ndim == 0:
        w = np.full(D, w)
    if w.shape != (D,):
        raise ValueError("make_backlog_policy: weights must be a scalar or a sequence of %d, got shape %s" % (D, w.shape))
    if w.dtype.kind not in "iu" and not (np.isfinite(w.astype(np.float64)).all() and (w == np.rint(w.astype(np.float64))).all()):
        raise ValueError("make_backlog_policy: weights must be integers")
    w = w.astype(np.int64)
    if (w < 0).any() or (w > SCORE_W_MAX).any():
        raise ValueError("make_backlog_policy: a weight lies outside [0, %d]" % SCORE_W_MAX)
    if duration_of_len is None:
        t = np.minimum(int(max_duration) - 1, 4 * np.arange(QUEUE_CAP + 1))
    else:
        t = np.asarray(duration_of_len)
        if t.shape != (QUEUE_CAP + 1,) or t.dtype.kind not in "iu":
            raise ValueError("make_backlog_policy: duration_of_len must be %d integers" % (QUEUE_CAP + 1))
    t = t.astype(np.int64)
    if (t < 0).any() or (t > 255).any():
        raise ValueError("make_backlog_policy: a duration lies outside [0, 255]")
    wl = np.zeros(MAX_DEVICES, "<i4")
    wl[:D] = w
    return np.concatenate([wl.view(np.uint8), t.astype(np.uint8)])


def backlog_sample_numpy(policy, qlen, max_duration):
    """CPU restatement of gw_rollout_backlog's choice for one step: ``qlen`` int[N][D], each sender's queue length at the env's
    current time (``get_state("qlen")``) -> ``(device, duration, seen_len)``, int32[N] each: the lowest index attaining the
    largest ``w_len[i] * qlen[i]`` (sender 0 where every priority is 0), ``min(duration_of_len[its length], max_duration - 1)``
    and that length."""
    policy = np.asarray(policy)
    if policy.shape != (BACKLOG_BYTES,) or policy.dtype != np.uint8:
        raise ValueError("policy must be make_backlog_policy()'s uint8[%d]" % BACKLOG_BYTES)
    q = np.asarray(qlen).astype(np.int64)
    if q.ndim != 2 or not 1 <= q.shape[1] <= MAX_DEVICES or (q < 0).any() or (q > QUEUE_CAP).any():
        raise ValueError("qlen must be [N][D] with lengths in [0, %d]" % QUEUE_CAP)
    w = policy[:4 * MAX_DEVICES].view("<i4").astype(np.int64)[:q.shape[1]]
    table = policy[4 * MAX_DEVICES:].astype(np.int64)
    dev = np.argmax(w[None, :] * q, axis=1)              # (the first index of the maximum)
    seen = q[np.arange(len(q)), dev]
    dur = np.minimum(table[seen], int(max_duration) - 1)
    return dev.astype(np.int32), dur.astype(np.int32), seen.astype(np.int32)


# ---- a population of scheduler policies (gw_rollout_backlog_population) ----------------------------------------------------------
BACKLOG_STRIDE = (BACKLOG_BYTES + 3) // 4 * 4       # sizeof(gw_backlog_policy): the image padded to the int32's alignment


def make_backlog_population(policies):
    """``uint8[P][BACKLOG_STRIDE]``: the ``gw_backlog_policy[P]`` array ``env.rollout_backlog_population`` uploads, from a
    sequence of ``make_backlog_policy`` images (``uint8[BACKLOG_BYTES]`` each), every row padded with zeros to the record's
    size."""
    rows = list(policies)
    if not rows:
        raise ValueError("make_backlog_population: at least one policy")
    out = np.zeros((len(rows), BACKLOG_STRIDE), np.uint8)
    for p, image in enumerate(rows):
        image = np.asarray(image)
        if image.shape != (BACKLOG_BYTES,) or image.dtype != np.uint8:
            raise ValueError("make_backlog_population: policy %d is not make_backlog_policy()'s uint8[%d]" % (p, BACKLOG_BYTES))
        out[p, :BACKLOG_BYTES] = image
    return out


def backlog_sample_population_numpy(population, envs_per_policy, qlen, max_duration):
    """CPU restatement of gw_rollout_backlog_population's choice for one step: env ``e`` of ``qlen`` int[N][D] chooses by row
    ``e // envs_per_policy`` of ``population`` (``uint8[P][BACKLOG_STRIDE]``, ``P * envs_per_policy == N``) as
    ``backlog_sample_numpy`` would -- with each weight clamped into ``[0, SCORE_W_MAX]`` first, since the call cannot validate
    an array it never reads on the host.  Returns ``(device, duration, seen_len)``, int32[N] each."""
    pop = np.asarray(population)
    if pop.ndim != 2 or pop.shape[1] != BACKLOG_STRIDE or pop.dtype != np.uint8:
        raise ValueError("population must be make_backlog_population()'s uint8[P][%d]" % BACKLOG_STRIDE)
    q = np.asarray(qlen).astype(np.int64)
    M = int(envs_per_policy)
    if q.ndim != 2 or not 1 <= q.shape[1] <= MAX_DEVICES or (q < 0).any() or (q > QUEUE_CAP).any():
        raise ValueError("qlen must be [N][D] with lengths in [0, %d]" % QUEUE_CAP)
    if M < 1 or len(pop) * M != len(q):
        raise ValueError("%d policies x %d envs is not qlen's %d envs" % (len(pop), M, len(q)))
    pop = np.ascontiguousarray(pop)
    w = np.clip(pop[:, :4 * MAX_DEVICES].view("<i4").astype(np.int64), 0, SCORE_W_MAX)[:, :q.shape[1]]
    table = pop[:, 4 * MAX_DEVICES:BACKLOG_BYTES].astype(np.int64)
    of = np.arange(len(q)) // M
    dev = np.argmax(w[of] * q, axis=1)                   # (the first index of the maximum)
    seen = q[np.arange(len(q)), dev]
    dur = np.minimum(table[of, seen], int(max_duration) - 1)
    return dev.astype(np.int32), dur.astype(np.int32), seen.astype(np.int32)


# ---- finite-state controllers inside the scored closed loop (gw_rollout_controller, include/gymwipe_amd.h) --------------------
# A controller has S nodes.  The env's node n and the class c of the observation it acts on pick the row the action is drawn
# from, cdf[n][c]; behind the step the node moves on the class of the new observation and on one bit, whether the step
# delivered at least need[n] packets: n <- next[n][c'][b].  A step that ends an episode puts the env at node 0, class 1.
FSC_MAX_STATES = 16             # GW_FSC_MAX_STATES


def make_controller(num_devices, cdf, next, need, max_duration=20):
    """The three arrays of a ``gw_controller``, checked: ``(cdf uint32[S][3][A], next uint8[S][3][2], need uint8[S])`` with
    ``1 <= S <= FSC_MAX_STATES`` and ``A = num_devices * max_duration``.  ``cdf``: per (node, observation class) a row as
    ``policy_cdf`` makes it -- integers in ``[0, 2^32)``, non-decreasing along a row.  ``next``: the node to move to by (node,
    new observation class, delivered bit), each in ``[0, S)``.  ``need``: each node's delivered-packet threshold in
    ``[0, 255]`` (0: the bit is always set; 255: never, a step delivers fewer).  The native calls validate none of this --
    they clamp where they read (``controller_step_numpy``) -- so a controller built here means what it says."""
    D, md = int(num_devices), int(max_duration)
    if not 2 <= D <= MAX_DEVICES or md < 1:
        raise ValueError("make_controller: num_devices must be in [2, %d] and max_duration >= 1" % MAX_DEVICES)
    A = D * md
    c, nx, nd = np.asarray(cdf), np.asarray(next), np.asarray(need)
    if c.ndim != 3 or not 1 <= c.shape[0] <= FSC_MAX_STATES or c.shape[1:] != (3, A):
        raise ValueError("make_controller: cdf must be [S][3][%d] with 1 <= S <= %d, got shape %s" % (A, FSC_MAX_STATES, c.shape))
    S = c.shape[0]
    if nx.shape != (S, 3, 2) or nd.shape != (S,):
        raise ValueError("make_controller: next must be [%d][3][2] and need [%d], got shapes %s and %s" % (S, S, nx.shape, nd.shape))
    for name, a in (("cdf", c), ("next", nx), ("need", nd)):
        if a.dtype.kind not in "iu":
            raise ValueError("make_controller: %s must hold integers" % name)
    c, nx, nd = c.astype(np.int64), nx.astype(np.int64), nd.astype(np.int64)
    if (c < 0).any() or (c > 0xffffffff).any() or (np.diff(c, axis=-1) < 0).any():
        raise ValueError("make_controller: a cdf row leaves [0, 2^32) or decreases")
    if (nx < 0).any() or (nx >= S).any():
        raise ValueError("make_controller: a next entry lies outside [0, %d)" % S)
    if (nd < 0).any() or (nd > 255).any():
        raise ValueError("make_controller: a need entry lies outside [0, 255]")
    return c.astype(np.uint32), nx.astype(np.uint8), nd.astype(np.uint8)


def _controller_arrays(controller):
    cdf, nxt, need = (np.asarray(a) for a in controller)
    if cdf.ndim != 3 or cdf.shape[1] != 3 or not 1 <= cdf.shape[0] <= FSC_MAX_STATES:
        raise ValueError("controller: cdf must be uint32[S][3][A] with 1 <= S <= %d" % FSC_MAX_STATES)
    S = cdf.shape[0]
    if cdf.dtype != np.uint32 or nxt.dtype != np.uint8 or need.dtype != np.uint8 or nxt.shape != (S, 3, 2) or need.shape != (S,):
        raise ValueError("controller must be (uint32[S][3][A], uint8[S][3][2], uint8[S])")
    return cdf, nxt, need


def controller_step_numpy(seed, env_lo, env_hi, step, controller, node, obs, counter_bound, max_duration):
    """CPU restatement of the controller's draw: ``(device, duration, node_used)`` for envs [env_lo, env_hi) at stream position
    ``step``, each at ``node`` uint8[envs] and acting on ``obs`` int32[envs].  ``node_used = min(node, S - 1)`` -- the clamp
    applies where the byte is read -- and the action is ``policy_sample_numpy``'s from row ``cdf[node_used][cls(obs)]``.
    ``controller``: ``make_controller``'s arrays, or any arrays of their dtypes and shapes."""
    cdf, _, _ = _controller_arrays(controller)
    S, A = cdf.shape[0], cdf.shape[2]
    n = np.minimum(np.asarray(node).astype(np.int64), S - 1)
    cls = np.sign(np.asarray(obs).astype(np.int64) - int(counter_bound)).astype(np.int64) + 1
    a = policy_count_numpy(cdf.reshape(3 * S, A), n * 3 + cls, policy_u_numpy(seed, env_lo, env_hi, step))
    dev = a // int(max_duration)
    return dev.astype(np.int32), (a - dev * int(max_duration)).astype(np.int32), n.astype(np.uint8)


def controller_move_numpy(controller, node, obs, delivered, ended, counter_bound):
    """CPU restatement of the controller's transition behind a step taken at ``node`` (clamped as the draw clamps it): where
    ``ended != 0`` the env is at node 0; elsewhere at ``min(next[n][cls(obs)][delivered >= need[n]], S - 1)``, ``obs`` the
    observation the step returned and ``delivered`` the packets it delivered.  Returns uint8[envs]."""
    cdf, nxt, need = _controller_arrays(controller)
    S = cdf.shape[0]
    n = np.minimum(np.asarray(node).astype(np.int64), S - 1)
    cls = np.sign(np.asarray(obs).astype(np.int64) - int(counter_bound)).astype(np.int64) + 1
    b = (np.asarray(delivered).astype(np.int64) >= need.astype(np.int64)[n]).astype(np.int64)
    to = np.minimum(nxt.astype(np.int64)[n, cls, b], S - 1)
    return np.where(np.asarray(ended) != 0, 0, to).astype(np.uint8)


def _one_hot_rows(D, duration, max_duration):
    """uint32[D][3][A]: node i's three rows all draw (sender i, duration) with certainty."""
    md = int(max_duration)
    if not 0 <= int(duration) < md:
        raise ValueError("duration must be in [0, %d)" % md)
    p = np.zeros((D, 3, D * md))
    for i in range(D):
        p[i, :, i * md + int(duration)] = 1.0
    return policy_cdf(p)


def round_robin_controller(num_devices, duration, max_duration=20):
    """D nodes: node i assigns sender i for ``duration`` and moves to node i + 1 (mod D) whatever happens."""
    D = int(num_devices)
    nxt = np.empty((D, 3, 2), np.uint8)
    nxt[:] = ((np.arange(D) + 1) % D)[:, None, None]
    return make_controller(D, _one_hot_rows(D, duration, max_duration), nxt, np.full(D, 255, np.uint8), max_duration)


def stay_while_productive_controller(num_devices, duration, need, max_duration=20):
    """D nodes: node i assigns sender i for ``duration``; it stays while the step delivered at least ``need`` packets and moves
    to node i + 1 (mod D) otherwise.  ``need >= 255`` (or more than ``duration`` can carry) is ``round_robin_controller``."""
    D = int(num_devices)
    nxt = np.empty((D, 3, 2), np.uint8)
    nxt[:, :, 0] = ((np.arange(D) + 1) % D)[:, None]
    nxt[:, :, 1] = np.arange(D)[:, None]
    return make_controller(D, _one_hot_rows(D, duration, max_duration), nxt, np.full(D, int(need), np.int64), max_duration)


def make_controller_population(controllers):
    """``(cdf uint32[P][S][3][A], next uint8[P][S][3][2], need uint8[P][S])`` from a sequence of controllers of one size: what
    ``env.rollout_controller_population`` uploads."""
    rows = [_controller_arrays(c) for c in controllers]
    if not rows:
        raise ValueError("make_controller_population: at least one controller")
    if len({r[0].shape for r in rows}) != 1:
        raise ValueError("make_controller_population: every controller needs the same S and A")
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


# ---- control loop: cyclic band schedules (gw_ctrl_rollout_schedules) --------------------------------------------------------------------
CTRL_SCHEDULE_MAX = 64          # entries of one schedule
CTRL_TALLY_COLS = 4             # episodes ended, of those by fail_deg, steps taken, sum of the costs of the ended episodes


def make_ctrl_schedules(schedules, L=None):
    """``uint8[P][L][2]`` = (device, duration) from a list of lists of ``(device, duration)`` pairs: what
    ``VecControlLoopEnv.rollout_schedules`` uploads.  ``L`` defaults to the longest list; a shorter schedule is padded
    cyclically (entry j is its entry ``j % len``), which changes what it does only if ``L`` is no multiple of its length."""
    rows = [[(int(d), int(u)) for d, u in s] for s in schedules]
    if not rows or any(not r for r in rows):
        raise ValueError("make_ctrl_schedules: at least one schedule, each with at least one entry")
    L = max(len(r) for r in rows) if L is None else int(L)
    if not 1 <= L <= CTRL_SCHEDULE_MAX or any(len(r) > L for r in rows):
        raise ValueError("make_ctrl_schedules: 1 <= L <= %d, no schedule longer than L" % CTRL_SCHEDULE_MAX)
    if any(not (0 <= v <= 255) for r in rows for pair in r for v in pair):
        raise ValueError("make_ctrl_schedules: device and duration are bytes")
    return np.array([[r[j % len(r)] for j in range(L)] for r in rows], np.uint8).reshape(len(rows), L, 2)


def ctrl_schedule_numpy(schedules, age, envs_per_schedule, max_duration=20):
    """The action env e takes at episode age ``age[e]`` under ``schedules`` (uint8[P][L][2]): entry ``age % L`` of schedule
    ``e // envs_per_schedule``, clamped where it is read -- device to {0, 1}, duration to [0, max_duration - 1].  Returns
    ``(device, duration)`` as int32[N]."""
    sch = np.asarray(schedules)
    if sch.dtype != np.uint8 or sch.ndim != 3 or sch.shape[2] != 2:
        raise ValueError("ctrl_schedule_numpy: schedules is uint8[P][L][2]")
    age = np.asarray(age, np.int64)
    p = np.arange(age.shape[0]) // int(envs_per_schedule)
    row = sch[p, age % sch.shape[1]].astype(np.int32)
    return np.minimum(row[:, 0], 1).astype(np.int32), np.minimum(row[:, 1], int(max_duration) - 1).astype(np.int32)


# ---- control loop: angle-feedback band schedulers (gw_ctrl_rollout_feedback) -----------------------------------------------------------
CTRL_FB_MAX_BINS = 8            # bins of one policy
CTRL_FB_COLS = 8                # the schedule tally's four, then: durations assigned, time elapsed, sum of |angle| dt, steps in bin 0


def make_ctrl_feedback(policies, edges, L=None):
    """``(sched uint8[P][B][L][2], edges int32[P][B - 1])`` from P policies, each a list of B cyclic schedules of
    ``(device, duration)`` pairs, and their B - 1 edges each: what ``VecControlLoopEnv.rollout_feedback`` uploads.  An env whose
    key (its int32 observation, or the absolute value of it) has ``n`` edges at or below it acts on schedule ``n`` of its policy.
    ``L`` defaults to the longest schedule; shorter ones are padded cyclically as ``make_ctrl_schedules`` pads.  The edges need
    not be sorted."""
    pols = [list(p) for p in policies]
    if not pols or any(not p for p in pols):
        raise ValueError("make_ctrl_feedback: at least one policy, each with at least one bin")
    B = len(pols[0])
    if not 1 <= B <= CTRL_FB_MAX_BINS or any(len(p) != B for p in pols):
        raise ValueError("make_ctrl_feedback: every policy needs the same number of bins, 1 <= B <= %d" % CTRL_FB_MAX_BINS)
    edge_rows = [[int(v) for v in r] for r in edges]
    if len(edge_rows) != len(pols) or any(len(r) != B - 1 for r in edge_rows):
        raise ValueError("make_ctrl_feedback: B - 1 edges for each policy")
    if any(not (-2 ** 31 <= v < 2 ** 31) for r in edge_rows for v in r):
        raise ValueError("make_ctrl_feedback: an edge is an int32")
    if L is None:
        L = max((len(s) for p in pols for s in p), default=0)
    sched = np.stack([make_ctrl_schedules(p, L) for p in pols])
    return sched, np.array(edge_rows, np.int32).reshape(len(pols), B - 1)


def ctrl_feedback_numpy(sched, edges, x_angle_rad, age, envs_per_policy, abs_key, max_duration=20):
    """The action env e takes in a state whose angle is ``x_angle_rad[e]`` at episode age ``age[e]``, rules 1-3 of
    ``gw_ctrl_rollout_feedback``: ``o = int32(min(max(angle * (180 / pi), -1e9), 1e9))`` (NaN gives -1e9), the key is ``o`` or
    ``|o|``, the bin is the number of the policy's edges at or below the key, the action entry ``age % L`` of that bin's schedule
    of policy ``e // envs_per_policy``, clamped where it is read -- device to {0, 1}, duration to [0, max_duration - 1].
    Returns ``(device, duration, bin)`` as int32[N]."""
    sch, edg = np.asarray(sched), np.asarray(edges)
    if sch.dtype != np.uint8 or sch.ndim != 4 or sch.shape[3] != 2:
        raise ValueError("ctrl_feedback_numpy: sched is uint8[P][B][L][2]")
    P, B, L = sch.shape[:3]
    if edg.dtype != np.int32 or edg.shape != (P, B - 1):
        raise ValueError("ctrl_feedback_numpy: edges is int32[P][B - 1]")
    deg = np.asarray(x_angle_rad, np.float64) * (180.0 / 3.141592653589793)
    deg = np.where(np.isnan(deg), -1e9, deg)                         # fmax(NaN, -1e9) is -1e9
    o = np.minimum(np.maximum(deg, -1e9), 1e9).astype(np.int64)      # truncation toward zero, as the int32 cast
    key = np.abs(o) if abs_key else o
    age = np.asarray(age, np.int64)
    p = np.arange(age.shape[0]) // int(envs_per_policy)
    bins = (edg[p].astype(np.int64) <= key[:, None]).sum(1)
    row = sch[p, bins, age % L].astype(np.int32)
    return (np.minimum(row[:, 0], 1).astype(np.int32), np.minimum(row[:, 1], int(max_duration) - 1).astype(np.int32),
            bins.astype(np.int32))


# ---- control loop: per-env PID gains (gw_ctrl_set_gains) -----------------------------------------------------------------------------------
CTRL_DEFAULT_GAINS = (1.0, 0.0, 0.0)    # the reference's shipped gains (control/inverted_pendulum.py:48-50): what every env starts with


def make_ctrl_gains(gain_sets, num_envs, envs_per_set=None):
    """``float64[N][3]`` = {kp, ki, kd} per env from G gain sets: what ``VecControlLoopEnv.set_gains`` uploads.  Env e gets set
    ``(e // envs_per_set) % G``.  The default ``envs_per_set = N // G`` gives G contiguous groups; a smaller value repeats the
    sets, which lays all G inside each schedule's (or policy's) block of envs: with P schedules, ``envs_per_set = N // (P * G)``
    makes ``rollout_schedules`` evaluate the whole G x P grid, env e being pair ``((e // envs_per_set) % G, e // (N // P))``."""
    sets = np.asarray(gain_sets, np.float64)
    if sets.ndim != 2 or sets.shape[1] != 3 or sets.shape[0] < 1:
        raise ValueError("make_ctrl_gains: gain_sets is G x 3 = (kp, ki, kd), G >= 1")
    N, G = int(num_envs), sets.shape[0]
    if N < 1 or N % G != 0:
        raise ValueError("make_ctrl_gains: num_envs must be a whole multiple of the number of gain sets")
    per = N // G if envs_per_set is None else int(envs_per_set)
    if per < 1 or N % (per * G) != 0:
        raise ValueError("make_ctrl_gains: num_envs must be a whole multiple of envs_per_set * G")
    return np.ascontiguousarray(sets[(np.arange(N) // per) % G])


def ctrl_pid_numpy(gains, ang, last):
    """The controller's rule at a control tick (``gw_ctrl_set_gains`` in include/gymwipe_amd.h; ``control()`` of the reference's
    control/inverted_pendulum.py:46-69), vectorised: ``gains`` f64[N][3] (or one set of 3), ``ang`` the controller's angle in
    degrees, ``last`` its last error.  ``e = |ang|``, ``pid = ((kp e) + (ki (e + last))) + (kd (e - last))``; a command goes out
    iff ``ang != 0`` and its value is ``pid`` where ``ang < 0``, else ``-pid``.  Returns ``(value, send, new_last)``; ``value``
    is meaningful where ``send``."""
    g = np.asarray(gains, np.float64)
    ang, last = np.asarray(ang, np.float64), np.asarray(last, np.float64)
    if g.shape[-1] != 3:
        raise ValueError("ctrl_pid_numpy: gains is f64[N][3] or one (kp, ki, kd)")
    kp, ki, kd = g[..., 0], g[..., 1], g[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.fabs(ang)
        pid = ((kp * e) + (ki * (e + last))) + (kd * (e - last))
    return np.where(ang < 0.0, pid, -pid), ang != 0.0, e + np.zeros_like(last)


# ---- control loop: seeded plant disturbances per env (gw_ctrl_set_disturbance) ------------------------------------------------------------
_M64 = (1 << 64) - 1
_STREAM_STEP = 0x9E3779B97F4A7C15                          # key[e] = seed ^ (streams[e] * this mod 2^64)


def make_ctrl_disturbance(g, num_envs, seed=0, streams=None, envs_per_set=None):
    """``(g float64[N][4], key uint64[N])``: what ``VecControlLoopEnv.set_disturbance`` uploads.  ``g`` is one weight vector of 4
    or G of them, laid across the envs the way ``make_ctrl_gains`` lays gains (env e gets set ``(e // envs_per_set) % G``, by
    default G contiguous groups).  ``key[e] = seed ^ (streams[e] * 0x9E3779B97F4A7C15 mod 2^64)``; ``streams`` defaults to
    ``arange(N)``, every env a noise sequence of its own.  Envs with equal stream numbers face the same sequence:
    ``streams = arange(N) % envs_per_policy`` gives env j of every policy (or schedule, or gain set) the same disturbance --
    common random numbers, the only way two candidates' tallies can be compared at less than the spread between sequences."""
    sets = np.asarray(g, np.float64)
    if sets.ndim == 1:
        sets = sets[None]
    if sets.ndim != 2 or sets.shape[1] != 4 or sets.shape[0] < 1:
        raise ValueError("make_ctrl_disturbance: g is 4 weights, one per plant state, or G x 4")
    N, G = int(num_envs), sets.shape[0]
    if N < 1 or N % G != 0:
        raise ValueError("make_ctrl_disturbance: num_envs must be a whole multiple of the number of sets")
    per = N // G if envs_per_set is None else int(envs_per_set)
    if per < 1 or N % (per * G) != 0:
        raise ValueError("make_ctrl_disturbance: num_envs must be a whole multiple of envs_per_set * G")
    if streams is None:
        st = np.arange(N, dtype=np.uint64)
    else:
        st = np.asarray(streams)
        if st.shape != (N,) or st.dtype.kind not in "iu":
            raise ValueError("make_ctrl_disturbance: streams is an integer array of num_envs stream numbers")
        st = st.astype(np.uint64)                         # (a negative number means its two's complement)
    with np.errstate(over="ignore"):
        key = np.uint64(int(seed) & _M64) ^ (st * np.uint64(_STREAM_STEP))
    return np.ascontiguousarray(sets[(np.arange(N) // per) % G]), key


def ctrl_noise_numpy(key, n):
    """The disturbance's draw ``w`` for key ``key`` at count ``n`` (``gw_ctrl_set_disturbance`` in include/gymwipe_amd.h),
    vectorised on numpy uint64 (both broadcast): uniform on [-1, 1), a multiple of 2^-31.  An env whose record was set n
    substeps ago adds ``g[i] * ctrl_noise_numpy(key, n)`` to ``x[i]`` at the end of its next substep."""
    u = np.uint64
    key, n = np.asarray(key).astype(np.uint64), np.asarray(n).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = key ^ (n * u(0xD1B54A32D192ED03))
        z = z + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(32)).astype(np.uint32).view(np.int32).astype(np.float64) * 2.0 ** -31


# ---- control loop: seeded packet erasures per env and link (gw_ctrl_set_loss) --------------------------------------------------------------
CTRL_LOSS_LINKS = ("rrm->sensor", "rrm->controller", "sensor->controller", "controller->actuator")
CTRL_LOSS_DEFAULT_SEED = 0x10551055AA55AA55               # not the disturbance's 0: equal stream numbers, other keys


def ctrl_loss_threshold(p):
    """Loss probabilities -> the rule's uint32 thresholds (``gw_ctrl_set_loss`` in include/gymwipe_amd.h): ``p`` is clipped to
    [0, 1] (NaN: 0) and ``thr = min(floor(p * 2^32), 2^32 - 1)``.  A transmission is erased when its draw, uniform on the 2^32
    values of a uint32, is below ``thr``: probability ``thr * 2^-32``, so ``p = 0`` never erases and ``p = 1`` erases all but one
    draw in 2^32.  Any shape; returns uint32 of that shape."""
    q = np.nan_to_num(np.asarray(p, np.float64), nan=0.0)
    q = np.clip(q, 0.0, 1.0)
    return np.minimum(np.floor(q * 4294967296.0), 4294967295.0).astype(np.uint32)


def make_ctrl_loss(p, num_envs, seed=CTRL_LOSS_DEFAULT_SEED, streams=None, envs_per_set=None):
    """``(thr uint32[N][4], key uint64[N])``: what ``VecControlLoopEnv.set_loss`` uploads.  ``p`` is one vector of 4 loss
    probabilities, one per link of ``CTRL_LOSS_LINKS`` -- the two announcements, then the two data links -- or G of them, laid
    across the envs the way ``make_ctrl_disturbance`` lays ``g`` (env e gets set ``(e // envs_per_set) % G``) and converted by
    ``ctrl_loss_threshold``.  The keys are that helper's formula, ``seed ^ (streams[e] * 0x9E3779B97F4A7C15 mod 2^64)``, from a
    default seed of their own; ``streams = arange(N) % envs_per_policy`` makes env j of every candidate lose the same
    transmissions, counted in the order they go on the air."""
    sets = np.asarray(p, np.float64)
    if sets.ndim == 1:
        sets = sets[None]
    if sets.ndim != 2 or sets.shape[1] != 4 or sets.shape[0] < 1:
        raise ValueError("make_ctrl_loss: p is 4 loss probabilities, one per link, or G x 4")
    laid, key = make_ctrl_disturbance(sets, num_envs, seed=seed, streams=streams, envs_per_set=envs_per_set)
    return ctrl_loss_threshold(laid), key


def ctrl_loss_numpy(key, n):
    """The loss rule's draw ``r`` for key ``key`` at count ``n`` (``gw_ctrl_set_loss`` in include/gymwipe_amd.h), vectorised on
    numpy uint64 (both broadcast); returns uint32.  The env's n-th transmission since its record was set is erased on link l
    iff ``ctrl_loss_numpy(key, n) < thr[l]``."""
    u = np.uint64
    key, n = np.asarray(key).astype(np.uint64), np.asarray(n).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = key ^ (n * u(0xA0761D6478BD642F))
        z = z + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(32)).astype(np.uint32)
