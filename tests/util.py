"""Shared helpers for the parity tests."""
import re
import subprocess

import numpy as np


def action_stream(seed, steps, num_envs, num_devices, max_duration=20):
    """Seeded uniform actions: device in [0,D), duration in [0,20) -- the env itself is
    deterministic, so actions are the only random input."""
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, num_devices, size=(steps, num_envs), dtype=np.int32)
    dur = rng.integers(0, max_duration, size=(steps, num_envs), dtype=np.int32)
    return dev, dur


LOSSY_RADII = (1.0, 3.4168, 4.5, 5.5459, 2.0)            # by i % 5: delivers all, partly decoded, never granted (x 2), delivers all
LOSSY_PARTLY, LOSSY_NEVER = (1,), (2, 3)                   # the residues i % 5 of the partly decoded and the never-granted senders


def lossy_layout(num_devices):
    """The layout on which packets are lost and grants refused: the RRM at the origin, sender i at angle 2 pi i / D and radius
    LOSSY_RADII[i % 5].  Returns (positions, rrm_position) as VecCounterTrafficEnv and oracle.ct_oracle.default_config take
    them.  A sender at 3.4168 m decodes the announcement but only some of its data packets reach the RRM; one at 4.5 m or
    5.5459 m never decodes an announcement, so it is never granted the band (tests/test_rollout_lossy_cpu.py gates both)."""
    D = int(num_devices)
    pos = [(LOSSY_RADII[i % 5] * float(np.cos(2.0 * np.pi * i / D)), LOSSY_RADII[i % 5] * float(np.sin(2.0 * np.pi * i / D)))
           for i in range(D)]
    return pos, (0.0, 0.0)


STATE_FIELDS = ("now", "wake", "counter", "qlen", "queue", "received", "latest_diff",
                "last_abs", "rx_power", "flags")
STAT_FIELDS = ("n_tx", "n_delivered", "n_appended", "n_popped", "n_dropped")


def assert_state_equal(gpu_env, oracle, fields=STATE_FIELDS, where=""):
    for f in fields:
        a = gpu_env.get_state(f)
        b = oracle.get(f)
        if a.dtype.kind == "f":
            same = a.view(np.uint64) == b.view(np.uint64)      # bit-exact, not approx
        else:
            same = a == b
        if not same.all():
            bad = np.argwhere(~same)[:5]
            raise AssertionError("state field %r differs %s at %s: gpu=%r oracle=%r"
                                 % (f, where, bad.tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def kernel_instantiations(path, family):
    """Every ``<family><...>`` template instantiation in the symbol table of the library at ``path``, as c++filt spells it (no
    namespace, no parameter list).  ``family``: a kernel's name, or a regular expression for several (``r"\\w+_kernel"``)."""
    nm = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    dem = subprocess.run(["c++filt"], input=nm, capture_output=True, text=True, check=True).stdout
    names = set()
    for line in dem.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"(?:^|[\s:])(" + family + r"<[^()]*>)\(", line)
        if m:
            names.add(m.group(1))
    return names


def private_segments(tmp_path, source):
    """Cross-compile ``gymwipe_amd/csrc/<source>`` for the device alone with the product build's own flags (``make
    print-flags``: they change register allocation) and return {kernel symbol: private_segment_fixed_size}: a kernel that uses
    no scratch memory has 0.  Needs hipcc and no GPU; skips the test where there is no hipcc."""
    import os
    import shutil
    import pytest
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gymwipe_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags, flags
    out = tmp_path / (source + ".s")
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", str(out), "-x", "hip", os.path.join(csrc, source)],
                   check=True, capture_output=True, timeout=900, cwd=csrc)
    text = out.read_text()
    sizes = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M)
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert sizes and len(sizes) == len(names)
    return dict(zip(names, map(int, sizes)))


# ---- linear plant: models, the substep schedule, a long-double reference and a float64 emulation of the tabulated form ----
# Test infrastructure in numpy alone: nothing here imports the library.
PLANT_KMAX = 32                                                # GW_PLANT_KMAX: the largest tabulated substep count
PLANT_DTS = {"1e-3": 1e-3, "3e-4": 3e-4, "2^-10": 2.0 ** -10}   # 1/dt inexact for the first two, exact for the third
PLANT_ERR_FLOOR = 64 * 2.0 ** -52                              # the bound's floor (plant_error_bound)
DENSE_SEEDS = (101, 202, 303)                                  # model (b)
QRQ_SEED = 404                                                 # model (c)


def plant_default_model():
    """(a): the forward-Euler pendulum of gw_plant_config_default, by the same expressions (bit-identical, which
    tests/test_plant_models.py checks against the library)."""
    tau, g_l, damp, dt = 0.05, 9.81, 0.2, 1e-3
    Ac = [[0, 1, 0, 0], [0, -1 / tau, 0, 0], [0, 0, 0, 1], [0, 1 / tau, -g_l, -damp]]
    Bc = [0, 1 / tau, 0, -1 / tau]
    A = np.array([[(1.0 if i == j else 0.0) + dt * Ac[i][j] for j in range(4)] for i in range(4)])
    return {"A": A, "B": np.array([dt * b for b in Bc]), "x0": np.array([0.0, 0.0, 0.05, 0.0]), "u0": 0.1}


def plant_dense_model(seed):
    """(b): a Gaussian 4x4 scaled to spectral radius 0.999, B ~ N(0, 0.1), four non-zero entries in x0."""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(4, 4))
    A = G * (0.999 / np.abs(np.linalg.eigvals(G)).max())
    x0 = rng.uniform(0.05, 0.5, 4) * rng.choice([-1.0, 1.0], 4)
    return {"A": A, "B": rng.normal(0.0, 0.1, 4), "x0": x0, "u0": float(rng.normal(0.0, 0.3))}


def plant_qrq_model(seed=QRQ_SEED):
    """(c): Q R Q^T with Q random orthogonal and R two rotation blocks, one undamped and one scaled by 0.995."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
    R = np.zeros((4, 4))
    for b, (th, s) in enumerate(((0.31, 1.0), (1.17, 0.995))):
        R[2 * b:2 * b + 2, 2 * b:2 * b + 2] = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    x0 = rng.uniform(0.05, 0.5, 4) * rng.choice([-1.0, 1.0], 4)
    return {"A": Q @ R @ Q.T, "B": rng.normal(0.0, 0.1, 4), "x0": x0, "u0": float(rng.normal(0.0, 0.3))}


def plant_models():
    m = {"default": plant_default_model()}
    for i, s in enumerate(DENSE_SEEDS):
        m["dense%d" % i] = plant_dense_model(s)
    m["qrq"] = plant_qrq_model()
    return m


PLANT_MODELS = plant_models()
DENSE_MODELS = tuple(k for k in PLANT_MODELS if k != "default")


def assert_dense(A):
    A = np.asarray(A)
    assert A.shape == (4, 4) and (A != 0).all(), "a dense plant model needs all 16 entries of A non-zero"
    assert not np.allclose(A, A.T, rtol=1e-3, atol=1e-6), "a dense plant model must not be symmetric"


PLANT_SCHEDULE_UPDATES = 12
PLANT_DESIGNED_ENVS = 48                                       # the designed block: three 16-env tiles


def _draw_heavy(rng, shape):
    """n from {0..5, 31..33, 63..65, 97, random < 130}, a tenth of the envs standing still."""
    pool = np.array(list(range(6)) + [31, 32, 33, 63, 64, 65, 97, -1, -1, -1])
    n = rng.choice(pool, size=shape)
    n = np.where(n < 0, rng.integers(0, 130, size=shape), n)
    return np.where(rng.random(shape) < 0.1, 0, n).astype(np.float64)


def plant_schedule(N, seed=7):
    """The clock increments of PLANT_SCHEDULE_UPDATES updates for N envs, in units of dt and all multiples of 1/4 (so that at
    dt = 2^-10 every clock is exact and a .5 is a tie): float64[T][N]; ``now = cumsum * dt``.  The first 48 envs are designed
    (tests/test_plant_models.py asserts what they cover, on the reference's own substep counts), envs up to 2048 and the
    last 64 draw from the heavy set, the envs between them (only at a large N) take 0..5 substeps and sometimes 33."""
    T = PLANT_SCHEDULE_UPDATES
    rng = np.random.default_rng(seed)
    inc = _draw_heavy(rng, (T, N))
    if N > 2048 + 64:
        light = rng.integers(0, 6, size=(T, N)).astype(np.float64)
        light[rng.random((T, N)) < 0.02] = 33.0
        inc[:, 2048:N - 64] = light[:, 2048:N - 64]
    inc += rng.choice([-0.25, 0.0, 0.25], size=(T, N))
    D = np.zeros((T, PLANT_DESIGNED_ENVS))
    D[4:] = _draw_heavy(np.random.default_rng(seed + 1), (T - 4, PLANT_DESIGNED_ENVS))
    e = np.arange(16)
    # tile 0: every chunk value 1..32 as a one-pass count, and again as the remainder after two passes and after one
    D[0, :16], D[1, :16], D[2, :16], D[3, :16] = e + 1, e + 17, 64 + e + 1, 32 + e + 17
    D[0:4, :16] += np.array([0.0, 0.25, -0.25, 0.0])[:, None]
    # tile 1: the totals 0, 32, 33, 64, 65, 97 and more side by side with 1..4; then the special clocks
    D[0, 16:27] = [0, 32, 33, 64, 65, 97, 129, 1, 4, 2, 0.25]
    D[1, 16:27] = [97, 0, 1, 2, 3, 4, 32, 161, 33, 65, 64]
    D[2, 16:27] = [3, 130, 0, 0.25, 96, 31, 1, 0, 128, 4, 2]
    D[3, 16:27] = [64, 65, 97, 5, 0, 33, 2, 3, 1, 100, 0]
    D[0:4, 27] = [5, -2, 1, 3]                # the clock falls below t_last, stays below, then passes it
    D[0:4, 28] = [7, 0, 0, 40]                # the clock stands still
    D[0:4, 29] = [2.5, 3.5, 0.5, 1.0]         # ties: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 (t_last stays), then 1.5 -> 2
    D[0:4, 30] = [33.5, 64.5, 4.5, 97.5]      # 33.5 -> 34, 64.5 -> 64, 4.5 -> 4, 97.5 -> 98
    D[0:4, 31] = [0, 0, 0, 0]                 # nothing at all in the first four updates
    D[0:4, 32:48] = _draw_heavy(np.random.default_rng(seed + 2), (4, 16)) + 0.25
    k = min(N, PLANT_DESIGNED_ENVS)
    inc[:, :k] = D[:, :k]
    return inc


def plant_substeps(now, t_last, dt):
    """n = llrint((now - t_last) * (1.0 / dt)) in float64, ties to even, as oracle/plant_oracle.c; 0 where now <= t_last."""
    now, t_last = np.asarray(now, np.float64), np.asarray(t_last, np.float64)
    inv_dt = np.float64(1.0) / np.float64(dt)
    scaled = (now - t_last) * inv_dt
    return np.where(now > t_last, np.rint(scaled), 0.0).astype(np.int64), scaled


def plant_reference_ld(A, B, dt, x0, u, now_sequence, input_changes=None):
    """The plant's recurrence in long double: for every row of ``now_sequence`` (float64[T][N]) each env takes n applications
    of x <- A x + B u, n as plant_substeps computes it, and keeps its state and t_last where n is 0.  ``u``: float64[N], the
    inputs before the first update; ``input_changes``: {t: (u_new[N], mask[N])}, applied after update t.
    Returns {"x": longdouble[T][N][4], "n": int64[T][N], "scaled": float64[T][N], "t_last": float64[T][N],
    "substeps": uint64[T][N] (cumulative), "xmax": the largest |component| any state took on the way}."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, ("np.longdouble has a %d-bit mantissa on this platform: it is no wider than float64, so it "
                                      "cannot serve as the plant's high-precision reference" % np.finfo(ld).nmant)
    now_sequence = np.asarray(now_sequence, np.float64)
    T, N = now_sequence.shape
    Al, Bl = np.asarray(A, np.float64).reshape(4, 4).astype(ld), np.asarray(B, np.float64).reshape(4).astype(ld)
    x = np.empty((4, N), ld)
    x[:] = np.asarray(x0, np.float64).astype(ld).reshape(4, 1) if np.ndim(x0) == 1 else np.asarray(x0, np.float64).T.astype(ld)
    u = np.array(u, np.float64)
    t_last, total = np.zeros(N), np.zeros(N, np.uint64)
    out = {"x": np.empty((T, N, 4), ld), "n": np.empty((T, N), np.int64), "scaled": np.empty((T, N)),
           "t_last": np.empty((T, N)), "substeps": np.empty((T, N), np.uint64)}
    xmax = float(np.abs(x).max())
    for t in range(T):
        n, scaled = plant_substeps(now_sequence[t], t_last, dt)
        order = np.argsort(-n, kind="stable")                  # most substeps first: the envs still moving are a prefix
        ns = n[order]
        xs, bu = x[:, order], Bl[:, None] * u[order].astype(ld)[None, :]
        for s in range(int(ns[0]) if N else 0):
            m = int(np.searchsorted(-ns, -s, side="left"))     # envs with n > s
            a = xs[:, :m]
            xs[:, :m] = Al @ a + bu[:, :m]                     # (long double has no BLAS: numpy's own left-to-right loop)
            xmax = max(xmax, float(np.abs(xs[:, :m]).max()))
        x[:, order] = xs
        t_last = np.where(n > 0, now_sequence[t], t_last)
        total = total + n.astype(np.uint64)
        out["x"][t], out["n"][t], out["scaled"][t], out["t_last"][t], out["substeps"][t] = x.T, n, scaled, t_last, total
        if input_changes and t in input_changes:
            un, mask = input_changes[t]
            u = np.where(np.asarray(mask, bool), np.asarray(un, np.float64), u)
    out["xmax"] = xmax
    return out


class PlantEmulation:
    """What the kernels compute, in float64 numpy: the tables P_k = A^k and Q_k = sum_{j<k} A^j B (k = 1..32) by the recurrence
    of gw_plant_create (P_1 = A, P_{k+1} = A P_k; q_1 = B, q_{k+1} = B + A q_k, each sum left to right), applied in chunks of
    at most 32 substeps: x <- P_c x + Q_c u."""

    def __init__(self, A, B, dt, x0, u, num_envs):
        A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4)
        K = PLANT_KMAX
        self.P, self.Q = np.zeros((K + 1, 4, 4)), np.zeros((K + 1, 4))
        self.P[1], self.Q[1] = A, B
        for k in range(1, K):
            for i in range(4):
                for j in range(4):
                    s = 0.0
                    for m in range(4):
                        s += float(A[i, m]) * float(self.P[k, m, j])
                    self.P[k + 1, i, j] = s
                s = float(B[i])
                for m in range(4):
                    s += float(A[i, m]) * float(self.Q[k, m])
                self.Q[k + 1, i] = s
        self.dt = float(dt)
        self.x = np.tile(np.asarray(x0, np.float64), (num_envs, 1))
        self.u = np.array(u, np.float64)
        self.t_last = np.zeros(num_envs)
        self.substeps = np.zeros(num_envs, np.uint64)

    def update(self, now):
        n, _ = plant_substeps(now, self.t_last, self.dt)
        left = n.copy()
        while (left > 0).any():
            chunk = np.minimum(left, PLANT_KMAX)
            for c in np.unique(chunk[chunk > 0]):
                m = chunk == c
                self.x[m] = self.x[m] @ self.P[c].T + self.Q[c] * self.u[m, None]
            left -= chunk
        self.t_last = np.where(n > 0, now, self.t_last)
        self.substeps += n.astype(np.uint64)

    def set_input(self, u, mask):
        self.u = np.where(np.asarray(mask, bool), np.asarray(u, np.float64), self.u)


def plant_err(x, x_ref):
    """max over envs of |x_e - ref_e|_inf / max(1, |ref_e|_inf), ``x_ref`` the long-double state."""
    d = np.abs(np.asarray(x).astype(np.longdouble) - x_ref).max(axis=-1)
    return float((d / np.maximum(1.0, np.abs(x_ref).max(axis=-1))).max())


def plant_error_bound(err_orc, err_emu):
    """What a kernel's plant_err may reach: 16 x the larger of the float64 recurrence's and the emulation's own error against
    the long-double reference in the same run (floor 64 ulp).  The emulation models neither the MFMA's internal summation
    order nor the fused multiply-add of the Q_k u term; each changes an application by a few ulp, not by an order of
    magnitude.  16 leaves one order over the reference's own error and stays eleven orders under the smallest error a wrong
    candidate (A^(k-1) for A^k: >= 0.43; Q_(k-1) for Q_k: >= 4.8e-2) produces."""
    return 16.0 * max(err_orc, err_emu, PLANT_ERR_FLOOR)


def plant_chunks(n):
    """The chunk values (1..32) the kernels go through for a substep count n."""
    out = []
    while n > 0:
        c = min(n, PLANT_KMAX)
        out.append(c)
        n -= c
    return out
