"""
PHY grid, second checker (the first is tests/test_grid.py): the packed forms of grid_run_kernel<MOBILE, GW>, the power
regime where the BER formula decides, and Position.set() between runs.

grid_run_kernel has ten instantiations, MOBILE x GW in {4, 8, 16, 32, 64}; 64 / GW replicas share a wave.  The launcher keeps
the minimal width GW0(n) (the power of two >= n, at least 4) if N * GW0 + 63 >= 65536 and doubles it otherwise until that
holds or it reaches 64 -- so width 4 needs n <= 4 and N >= 16369, width 8 n <= 8 and N >= 8185, width 16 n <= 16 and
N >= 4093, width 32 n <= 32 and N >= 2047, and every smaller batch (all of tests/test_grid.py) runs at width 64.  The tests
here reach a width the way a user does, through N, and each asserts afterwards that the handle ran the width it meant to
(gw_grid_selftest_width).

A batch of 16 000 replicas cannot each have an oracle run of its own, so replica e takes delay row e % K of K = 7 rows: 7 is
coprime to every replicas-per-wave count (16, 8, 4, 2), so each wave mixes rows -- its groups diverge in the handler switch
-- and the row a group position sees rotates from wave to wave.  The static grid depends on the row alone: the oracle runs
once per row and all N replicas are compared.  The mobile walk depends on the replica index: every replica of four whole
waves (first, last, two by a fixed seed) is compared with an oracle run of its own, and the rest by what needs none.

At the fixture's 40 dBm the BER is ~0 without an interferer and ~0.49 with one, so ber_bpsk's constants decide nothing and
no payload ever fails.  Between -10 and 0 dBm all four outcomes occur; those cases assert on the oracle's own decision records
that they do and that no decision is within 1e-3 bit of the rounding boundary that flips it (device and host libm differ by
many orders less on a sum of a few hundred bits).
"""
import contextlib
import functools

import numpy as np
import pytest

K = 7                                                    # delay rows; replica e uses row e % K
WAVE = 64
COUNTERS = ("n_sent", "hdr_ok", "hdr_fail", "pay_ok", "pay_fail")
MOBILE_SEED = 1234                                       # the walk's seed in tests/test_grid.py
# The mobile cases' walk seed and, where it is not run_length(n), simulated seconds, by (n, N, tx power).  Picked on the CPU, by
# the event-driven model alone, for two properties of the scenario (not of the kernel):
#   1. in every compared replica the tolerance can resolve every radio's received power (assert_powers_resolvable, which the
#      suite re-checks: test_mobile_cases_compare_powers_the_tolerance_can_resolve);
#   2. in ALL N replicas the model runs through.  The reference asserts noise >= 0 and takes its log10; when two radios walk
#      within millimetres of each other the rounding residue of a 10^4 mW sum can eat the 9e-11 mW of thermal noise, and the
#      reference raises.  The kernel flags a replica with noise < 0 GW_FLAG_REFEXC and neither side means anything from
#      there on, so `flags == 0` in every replica needs a walk on which that happens nowhere.  One in a few thousand
#      four-radio replicas of 0.1 s does it, so the three largest batches run 0.04 s.  Minutes of oracle time per case:
#      `python tests/soak_grid.py walks` repeats it, the suite does not.
MOBILE_SETUP = {(4, 16389, 40.0): (212, 0.04), (3, 16369, 40.0): (19, 0.04), (8, 8185, 40.0): (20, 0.04),
                (9, 4100, 40.0): (1234, None), (17, 2050, 40.0): (1234, None),
                (4, 4, -10.0): (2, None), (9, 3, 0.0): (3, None), (9, 4100, 0.0): (10, None)}


def walk_seed(n, N, power):
    return MOBILE_SETUP[(n, N, power)][0]


def mobile_run_length(n, N, power):
    return MOBILE_SETUP[(n, N, power)][1] or run_length(n)


# (width, n, N): the last wave partial, or a group with idle lanes (n < width), or both
STATIC_CASES = [(4, 4, 16389), (4, 3, 16369), (4, 2, 16400),
                (8, 8, 8185), (8, 5, 8200), (8, 4, 8190),
                (16, 16, 4093), (16, 9, 4100), (16, 2, 4094),
                (32, 32, 2047), (32, 17, 2050), (32, 4, 2048)]
MOBILE_CASES = [(4, 4, 16389), (8, 8, 8185), (16, 9, 4100), (32, 17, 2050), (4, 3, 16369)]
# the regime where the BER decides: (n, tx power), each at width 64 and one packed case per kind
BER_POWERS = {4: -10.0, 9: 0.0}
BER_STATIC_CASES = [(64, 4, 6), (64, 9, 5), (4, 4, 16389)]
BER_MOBILE_CASES = [(64, 4, 4), (64, 9, 3), (16, 9, 4100)]
# what this file runs, for tests/test_host_logic.py: (mobile, width) of grid_run_kernel<mobile, width>
WIDTH_PAIRS = ({(False, w) for w, _, _ in STATIC_CASES + BER_STATIC_CASES}
               | {(True, w) for w, _, _ in MOBILE_CASES + BER_MOBILE_CASES})


def launcher_width(N, n):
    """The launcher's rule as the module docstring states it, in Python."""
    gw = 4
    while gw < n:
        gw *= 2
    while gw < 64 and N * gw + 63 < 65536:
        gw *= 2
    return gw


def run_length(n):
    """Simulated seconds: 0.04 .. 0.12, shorter for larger n (ten packets per radio at n <= 4, four at n = 32).  The three
    largest mobile batches run 0.04 s whatever their n, four packets per radio (MOBILE_SETUP says why)."""
    return 0.1 if n <= 4 else (0.08 if n <= 9 else (0.06 if n <= 17 else 0.04))


def delay_rows(n, seed):
    return np.random.default_rng(seed).uniform(0, 1e-2, (K, n))


def last_width(grid):
    from gymwipe_amd import _native as nat
    return nat.lib().gw_grid_selftest_width(grid._h, 0, 0)


def flip_boundary(bits):
    """The one value of err_sum at which the model's rule round(err_sum) / bits <= max_correctable_ber() changes its answer:
    m + 0.5 with m the largest integer the rule accepts (round() is monotone, so there is one such value)."""
    from oracle import des_model as dm
    ber = dm.BpskMcs().max_correctable_ber()
    m = int(np.floor(bits * ber))
    assert m / bits <= ber < (m + 1) / bits
    assert round(m + 0.5 - 1e-3) == m and round(m + 0.5 + 1e-3) == m + 1
    return m + 0.5


def assert_ber_decides(decisions, where):
    """(a) all four outcomes occur; (b) every decision is at least 1e-3 bit from the boundary that would flip it."""
    seen = {(what, ok) for what, ok, _, _ in decisions}
    assert seen == {("hdr", True), ("hdr", False), ("pay", True), ("pay", False)}, "%s: outcomes %s" % (where, sorted(seen))
    margin = min(abs(err - flip_boundary(bits)) for _, _, err, bits in decisions)
    assert margin >= 1e-3, "%s: a decision %.3g bit from its rounding boundary" % (where, margin)
    for what, ok, err, bits in decisions:
        assert ok == (err < flip_boundary(bits))


def count(decisions, what, ok):
    return sum(1 for k in decisions if k[0] == what and k[1] is ok)


# ---- the oracle, once per delay row (static) or per replica (mobile), shared by every test that needs it -------------------
@functools.lru_cache(maxsize=None)
def static_rows(n, seed, T, power):
    """K oracle runs of the static grid, split 0.4 T + 0.6 T like tests/test_grid.py: arrays indexed by row, and the rows'
    decision records."""
    from oracle import des_model as dm
    rows = delay_rows(n, seed)
    out = {f: [] for f in ("now", "n_tx", "rx_power") + COUNTERS}
    decisions = []
    for r in range(K):
        w = dm.World()
        devs = [dm.GridDevice(w, i, *dm.grid_positions(n)[i], dm.GRID_SEND_INTERVAL, float(rows[r, i]), power) for i in range(n)]
        w.sim.run(T * 0.4)
        w.sim.run(T * 0.6)
        out["now"].append(w.sim.now)
        out["n_tx"].append(len(w.band.log))
        out["rx_power"].append([d.phy.rx_power for d in devs])
        out["n_sent"].append([d.n_sent for d in devs])
        for key, what, ok in (("hdr_ok", "hdr", True), ("hdr_fail", "hdr", False), ("pay_ok", "pay", True), ("pay_fail", "pay", False)):
            out[key].append([count(d.phy.decisions, what, ok) for d in devs])
        decisions += [k for d in devs for k in d.phy.decisions]
    out = {f: np.array(v) for f, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out, tuple(decisions)


@contextlib.contextmanager
def recorded_devices():
    """The GridDevice objects the oracle's scenarios build while this is open (they return counters, not decision records)."""
    from oracle import des_model as dm
    orig, made = dm.GridDevice, []

    class Recorded(orig):
        def __init__(self, *a, **kw):
            orig.__init__(self, *a, **kw)
            self.peak = self.phy.rx_power                # the largest received power this radio ever held

            def note(_delta):
                self.peak = max(self.peak, self.phy.rx_power)
            self.phy.n_pow.subscribe_callback(note)      # after the PHY's own update (priority 1); creates no event
            made.append(self)
    dm.GridDevice = Recorded
    try:
        yield made
    finally:
        dm.GridDevice = orig


@functools.lru_cache(maxsize=None)
def mobile_replica(n, seed, T, power, walk, replica):
    """(scenario_mobile_grid's result, the decision records, each radio's peak received power) of one replica."""
    from oracle import des_model as dm
    row = delay_rows(n, seed)[replica % K]
    with recorded_devices() as devs:
        want = dm.scenario_mobile_grid(n, row.tolist(), T, seed=walk, replica=replica, runs=[T * 0.5, T * 0.5], tx_power_dbm=power)
    return want, tuple(k for d in devs for k in d.phy.decisions), tuple(d.peak for d in devs)


def mobile_atol(power):
    """The existing mobile test's atol, 1e-13 at 40 dBm; every power scales with the transmit power, so it does too."""
    from oracle import des_model as dm
    return 1e-13 * 10 ** ((power - dm.GRID_TX_POWER_DBM) / 10)


def assert_powers_resolvable(want, peaks, power, where):
    """A received power is a running sum: + p when a transmission starts, + (p' - p) when a radio moves, - p' when it ends.
    Device and host evaluate p with different libms and may disagree in its last bit, and a sum that once held P keeps
    every later value only to ulp(P) -- after the walk brought two radios within centimetres (P of 10^3 mW and more, at
    40 dBm) an idle radio's 9e-11 mW of thermal noise is known to ~1e-13, the whole tolerance.  That is a property of the
    scenario, not of the kernel, and the oracle alone shows it: the walk seeds (MOBILE_SETUP) are picked, on the CPU, so that
    in every compared replica the tolerance of every radio covers at least 4 ulp of the largest power it ever held."""
    tol = mobile_atol(power) + 1e-7 * np.abs(np.array(want["rx_power"]))
    ok = 4 * np.spacing(np.array(peaks)) <= tol
    assert ok.all(), "%s: radio %s held %s mW, its final %s mW cannot be compared to %s" % (
        where, first_bad(ok), np.array(peaks)[~ok], np.array(want["rx_power"])[~ok], tol[~ok])


def sampled_replicas(N, width):
    """Every replica of four whole waves: the first, the last (partial where N says so) and two drawn with a fixed seed;
    plus replicas 0 .. K-1, one per delay row."""
    per_wave = WAVE // width
    waves = (N + per_wave - 1) // per_wave
    pick = {0, waves - 1}
    if waves > 4:
        pick |= {1 + int(w) for w in np.random.default_rng(N).choice(waves - 2, 2, replace=False)}
    reps = {e for w in pick for e in range(w * per_wave, min(N, (w + 1) * per_wave))}
    return sorted(reps | set(range(min(K, N))))


def first_bad(same):
    return np.argwhere(~same)[:3].tolist()


# ---- packed widths, static: every replica -----------------------------------------------------------------------------------
def check_static(width, n, N, power, seed):
    import gymwipe_amd
    from oracle import des_model as dm
    T = run_length(n)
    assert launcher_width(N, n) == width
    want, decisions = static_rows(n, seed, T, power)
    row = np.arange(N) % K
    kw = {} if power == dm.GRID_TX_POWER_DBM else {"tx_power_dbm": power}
    grid = gymwipe_amd.VecPhyGrid(N, n, delay_rows(n, seed)[row], **kw)
    assert last_width(grid) == 0
    grid.runSimulation(T * 0.4)
    grid.runSimulation(T * 0.6)
    got = {f: grid.get_state(f) for f in ("now", "n_tx", "rx_power", "flags") + COUNTERS}
    assert last_width(grid) == width, "N = %d, n = %d ran grid_run_kernel<false, %d>, not <false, %d>" % (N, n, last_width(grid), width)
    grid.close()
    assert (got["flags"] == 0).all(), first_bad(got["flags"] == 0)
    for f in ("now", "n_tx") + COUNTERS:
        same = got[f] == want[f][row]
        assert same.all(), "%s differs at %s" % (f, first_bad(same))
    close = np.isclose(got["rx_power"], want["rx_power"][row], rtol=1e-9, atol=0.0)
    assert close.all(), "rx_power differs at %s" % first_bad(close)
    return decisions


@pytest.mark.gpu
@pytest.mark.parametrize("width,n,N", STATIC_CASES)
def test_packed_static_grid_matches_oracle_in_every_replica(width, n, N):
    from oracle import des_model as dm
    check_static(width, n, N, dm.GRID_TX_POWER_DBM, 700 + n)


# ---- packed widths, mobile: whole waves sampled -----------------------------------------------------------------------------
def check_mobile(width, n, N, power, seed):
    import gymwipe_amd
    from oracle import des_model as dm
    T = mobile_run_length(n, N, power)
    assert launcher_width(N, n) == width
    row = np.arange(N) % K
    kw = {} if power == dm.GRID_TX_POWER_DBM else {"tx_power_dbm": power}
    walk = walk_seed(n, N, power)
    grid = gymwipe_amd.VecPhyGrid(N, n, delay_rows(n, seed)[row], mobile=True, seed=walk, **kw)
    grid.runSimulation(T * 0.5)
    grid.runSimulation(T * 0.5)
    got = {f: grid.get_state(f) for f in ("now", "n_tx", "rx_power", "pos", "flags") + COUNTERS}
    assert last_width(grid) == width, "N = %d, n = %d ran grid_run_kernel<true, %d>, not <true, %d>" % (N, n, last_width(grid), width)
    grid.close()
    decisions = []
    for e in sampled_replicas(N, width):
        want, dec, peaks = mobile_replica(n, seed, T, power, walk, e)
        decisions += dec
        assert got["now"][e] == want["now"]
        assert np.array_equal(got["pos"][e], np.array(want["pos"])), "replica %d: the random walk itself must be bit-identical" % e
        assert int(got["n_tx"][e]) == want["n_tx"], "replica %d" % e
        for key in COUNTERS:
            assert got[key][e].tolist() == want[key], "%s replica %d: %s vs %s" % (key, e, got[key][e].tolist(), want[key])
        assert_powers_resolvable(want, peaks, power, "replica %d" % e)
        assert np.allclose(got["rx_power"][e], np.array(want["rx_power"]), rtol=1e-7, atol=mobile_atol(power)), \
            "rx_power replica %d: %s vs %s" % (e, got["rx_power"][e].tolist(), want["rx_power"])
    # every replica: no flag, the same clock, and the sender ticks of its delay row (they do not depend on the PHY)
    assert (got["flags"] == 0).all(), (
        "flags %s in replicas %s.  GW_FLAG_REFEXC (2) marks a replica in which the reference trips its own `assert noise >= 0`; "
        "MOBILE_SETUP's walk seeds are picked so that none does.  If a seed, a run length, a delay seed or the walk's hash "
        "changed, pick again: `python tests/soak_grid.py walks` says which replica the model does not run through"
        % (sorted(set(got["flags"][got["flags"] != 0].tolist())), first_bad(got["flags"] == 0)))
    now = mobile_replica(n, seed, T, power, walk, 0)[0]["now"]
    assert (got["now"] == now).all(), first_bad(got["now"] == now)
    sent = np.array([mobile_replica(n, seed, T, power, walk, r)[0]["n_sent"] for r in range(min(K, N))])
    same = got["n_sent"] == sent[row]
    assert same.all(), "n_sent differs at %s" % first_bad(same)
    return decisions


@pytest.mark.gpu
@pytest.mark.parametrize("width,n,N", MOBILE_CASES)
def test_packed_mobile_grid_matches_oracle_in_sampled_waves(width, n, N):
    from oracle import des_model as dm
    check_mobile(width, n, N, dm.GRID_TX_POWER_DBM, 800 + n)


# ---- where the BER decides --------------------------------------------------------------------------------------------------
BER_STATIC_SEED, BER_MOBILE_SEED = 900, 950


def ber_static_decisions(n):
    return static_rows(n, BER_STATIC_SEED + n, run_length(n), BER_POWERS[n])[1]


def mobile_case_replicas(width, n, N, power, seed):
    return [(e, mobile_replica(n, seed, mobile_run_length(n, N, power), power, walk_seed(n, N, power), e)) for e in sampled_replicas(N, width)]


def ber_mobile_decisions(width, n, N):
    return [k for _, rep in mobile_case_replicas(width, n, N, BER_POWERS[n], BER_MOBILE_SEED + n) for k in rep[1]]


def test_mobile_cases_compare_powers_the_tolerance_can_resolve():
    """assert_powers_resolvable for every replica the GPU cases compare, on the oracle alone."""
    from oracle import des_model as dm
    cases = [(w, n, N, dm.GRID_TX_POWER_DBM, 800 + n) for w, n, N in MOBILE_CASES]
    cases += [(w, n, N, BER_POWERS[n], BER_MOBILE_SEED + n) for w, n, N in BER_MOBILE_CASES]
    for width, n, N, power, seed in cases:
        for e, (want, _, peaks) in mobile_case_replicas(width, n, N, power, seed):
            assert_powers_resolvable(want, peaks, power, "n = %d, N = %d, replica %d" % (n, N, e))


def test_ber_regime_oracle_makes_all_four_decisions_away_from_the_boundary():
    """The conditions the GPU cases below rest on, on the oracle alone: with these seeds every case sees header and payload
    decisions of both kinds, none within 1e-3 bit of flipping.  At 40 dBm the same rows never fail a payload."""
    from oracle import des_model as dm
    for n in BER_POWERS:
        assert_ber_decides(ber_static_decisions(n), "static n = %d" % n)
        loud = static_rows(n, BER_STATIC_SEED + n, run_length(n), dm.GRID_TX_POWER_DBM)[1]
        assert count(loud, "pay", False) == 0 and count(loud, "hdr", False) > 0
    for width, n, N in BER_MOBILE_CASES:
        assert_ber_decides(ber_mobile_decisions(width, n, N), "mobile n = %d, N = %d" % (n, N))
    assert flip_boundary(130.0) == 32.5 and flip_boundary(260.0) == 65.5


@pytest.mark.gpu
@pytest.mark.parametrize("width,n,N", BER_STATIC_CASES)
def test_static_grid_where_the_ber_decides(width, n, N):
    decisions = check_static(width, n, N, BER_POWERS[n], BER_STATIC_SEED + n)
    assert_ber_decides(decisions, "static n = %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("width,n,N", BER_MOBILE_CASES)
def test_mobile_grid_where_the_ber_decides(width, n, N):
    decisions = check_mobile(width, n, N, BER_POWERS[n], BER_MOBILE_SEED + n)
    assert_ber_decides(decisions, "mobile n = %d, N = %d" % (n, N))


# ---- Position.set() between runs ---------------------------------------------------------------------------------------------
SETPOS_ENVS = 5
SETPOS_MOVE_INTERVAL = 1e12                              # a mobile handle whose walk never takes a step
FAR = 5000.0                                             # beyond STANDBY_THRESHOLD (3000 m) from every radio of the grid


class SetPositionWorld:
    """The event-driven model driven like the handle: run, position.set, run.  Mover processes exist (and wait for
    SETPOS_MOVE_INTERVAL) as in scenario_mobile_grid, so every event gets the id it has on the GPU; the move itself is a
    plain call between two runs, not a process."""

    def __init__(self, n, delays, replica, move_interval=SETPOS_MOVE_INTERVAL):
        from oracle import des_model as dm
        self.w = w = dm.World()
        pos = dm.grid_positions(n)
        self.devs = devs = [dm.GridDevice(w, i, pos[i][0], pos[i][1], dm.GRID_SEND_INTERVAL, float(delays[i])) for i in range(n)]
        sim = w.sim

        def mover(dv):
            yield sim.timeout(dm.grid_uniform(MOBILE_SEED, replica, dv.index, 0, 0) * move_interval)
            k = 0
            while True:
                xo = -.2 + (.2 - -.2) * dm.grid_uniform(MOBILE_SEED, replica, dv.index, k, 1)
                yo = -.2 + (.2 - -.2) * dm.grid_uniform(MOBILE_SEED, replica, dv.index, k, 2)
                dv.position.set(dv.position.x + xo, dv.position.y + yo)
                k += 1
                yield sim.timeout(move_interval)
        for dv in devs:
            sim.process(mover(dv))

    def run(self, seconds):
        self.w.sim.run(seconds)

    def state(self):
        devs = self.devs
        out = {"now": self.w.sim.now, "n_tx": len(self.w.band.log), "on_air": len(self.w.band.active()),
               "rx_power": [d.phy.rx_power for d in devs], "pos": [(d.position.x, d.position.y) for d in devs],
               "n_sent": [d.n_sent for d in devs]}
        for key, what, ok in (("hdr_ok", "hdr", True), ("hdr_fail", "hdr", False), ("pay_ok", "pay", True), ("pay_fail", "pay", False)):
            out[key] = [count(d.phy.decisions, what, ok) for d in devs]
        return out


def test_set_position_world_is_the_mobile_scenario():
    """With the fixture's move interval the helper above is scenario_mobile_grid: same walk, same ids, same outcome."""
    from oracle import des_model as dm
    n, T = 4, 0.05
    row = delay_rows(n, 5)[0]
    w = SetPositionWorld(n, row, 3, move_interval=dm.GRID_MOVE_INTERVAL)
    w.run(T * 0.5)
    w.run(T * 0.5)
    got, want = w.state(), dm.scenario_mobile_grid(n, row.tolist(), T, seed=MOBILE_SEED, replica=3, runs=[T * 0.5, T * 0.5])
    for key, value in want.items():
        assert got[key] == value, key


@functools.lru_cache(maxsize=None)
def setpos_plan(n, case):
    """(delays, t1, device, targets[N][2], t2) from the oracle's own log: at t1 the situation of `case` holds for certain.
      "A"       the moved radio is transmitting and others receive it;
      "B"       the moved radio is receiving while two (or more) others transmit;
      "standby" as B, but the radio goes FAR away: every stored power stays stale, and so does the attenuation of its links
                (physical.py:371-386) -- the transmissions of the second run, the moved radio's own included, are received
                with the powers of the OLD geometry."""
    from oracle import des_model as dm
    delays = delay_rows(n, 40 + n)[0]
    probe = SetPositionWorld(n, delays, 0)
    probe.run(0.06)
    log = [(t.start, t.stop, t.sender.index) for t in probe.w.band.log]
    found = None
    for i, (s, e, who) in enumerate(log):
        if s < 0.02:                                     # let every radio have transmitted once
            continue
        if case == "A":
            t1, dev, need_air = s + 0.3 * (e - s), who, 1
        else:
            over = [(max(s, s2), min(e, e2)) for s2, e2, _ in log[i + 1:] if s2 < e]
            if not over:
                continue
            t1, dev, need_air = over[0][0] + 0.4 * (over[0][1] - over[0][0]), None, 2
        w = SetPositionWorld(n, delays, 0)
        w.run(t1)
        air = w.w.band.active()
        if len(air) < need_air:
            continue
        if case == "A":
            if not w.devs[dev].phy.transmitting or not any(d.phy.receiving for d in w.devs if d is not w.devs[dev]):
                continue
        else:
            rx = [d.index for d in w.devs if d.phy.receiving and not d.phy.transmitting and all(t.sender is not d for t in air)]
            if not rx:
                continue
            dev = rx[0]
        found = (t1, dev)
        break
    assert found, "no instant for case %s in the oracle's log" % case
    t1, dev = found
    x0, y0 = dm.grid_positions(n)[dev]
    e = np.arange(SETPOS_ENVS, dtype=np.float64)
    if case == "standby":
        targets = np.stack([FAR + 100.0 * e, FAR + 0 * e], axis=1)
    else:
        targets = np.stack([x0 + 0.5 + 0.3 * e, y0 - 0.25 * e], axis=1)
    t2 = 0.03                                            # every radio transmits three more times
    targets.setflags(write=False)
    return delays, t1, dev, targets, t2


@pytest.mark.parametrize("n", [4, 9])
@pytest.mark.parametrize("case", ["A", "B", "standby"])
def test_set_position_plan_holds_on_the_oracle(n, case):
    """The situation each GPU case below is about is certain at its instant, and the move has the effect it is there for."""
    delays, t1, dev, targets, t2 = setpos_plan(n, case)
    w = SetPositionWorld(n, delays, 0)
    w.run(t1)
    air = w.w.band.active()
    before = [d.phy.rx_power for d in w.devs]
    w.devs[dev].position.set(float(targets[0, 0]), float(targets[0, 1]))
    after = [d.phy.rx_power for d in w.devs]
    if case == "A":
        assert any(t.sender is w.devs[dev] for t in air)
        assert all(a != b for i, (a, b) in enumerate(zip(after, before)) if i != dev)
    else:
        assert len(air) >= 2 and w.devs[dev].phy.receiving and all(t.sender is not w.devs[dev] for t in air)
        if case == "B":
            assert after[dev] != before[dev]
        else:
            assert after == before, "beyond the stand-by threshold nothing is re-evaluated"
            others = [d for d in w.devs if d is not w.devs[dev]]
            assert min(d.position.distance_to(w.devs[dev].position) for d in others) >= 3000.0
            # ... and the links stay as they were: what starts in the second run is received at the old geometry's power
            w.run(t2)
            late = [t for t in w.w.band.log if t.start > t1]
            assert any(t.sender is w.devs[dev] for t in late) and any(t.sender is not w.devs[dev] for t in late)
            att = [w.w.band.link(w.devs[dev], d).attenuation for d in others]
            assert max(att) < 60.0, "dB: the links still hold metres; 7 km would be 117 dB"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 9])
@pytest.mark.parametrize("case", ["A", "B", "standby"])
def test_set_position_between_runs_matches_oracle(n, case):
    from gymwipe_amd.grid import VecPhyGrid
    delays, t1, dev, targets, t2 = setpos_plan(n, case)
    N = SETPOS_ENVS
    g = VecPhyGrid(N, n, np.tile(delays, (N, 1)), mobile=True, seed=MOBILE_SEED, move_interval=SETPOS_MOVE_INTERVAL)
    worlds = [SetPositionWorld(n, delays, e) for e in range(N)]
    fields = ("now", "n_tx", "on_air", "rx_power", "pos", "flags") + COUNTERS

    def compare(stage):
        got = {f: g.get_state(f) for f in fields}
        assert (got["flags"] == 0).all()
        for e, w in enumerate(worlds):
            want = w.state()
            for f in ("now", "n_tx", "on_air"):
                assert got[f][e] == want[f], "%s: %s replica %d: %s vs %s" % (stage, f, e, got[f][e], want[f])
            assert np.array_equal(got["pos"][e], np.array(want["pos"])), "%s: pos replica %d" % (stage, e)
            for f in COUNTERS:
                assert got[f][e].tolist() == want[f], "%s: %s replica %d: %s vs %s" % (stage, f, e, got[f][e].tolist(), want[f])
            assert np.allclose(got["rx_power"][e], np.array(want["rx_power"]), rtol=1e-7, atol=1e-13), \
                "%s: rx_power replica %d: %s vs %s" % (stage, e, got["rx_power"][e], want["rx_power"])
        return got

    g.runSimulation(t1)
    for w in worlds:
        w.run(t1)
    before = compare("before the move")
    assert (before["on_air"] >= (1 if case == "A" else 2)).all()
    g.setPosition(dev, targets[:, 0], targets[:, 1])
    for e, w in enumerate(worlds):
        w.devs[dev].position.set(float(targets[e, 0]), float(targets[e, 1]))
    moved = compare("after the move")
    others = [i for i in range(n) if i != dev]
    if case == "A":
        assert (moved["rx_power"][:, others] != before["rx_power"][:, others]).all()
    elif case == "B":
        assert (moved["rx_power"][:, dev] != before["rx_power"][:, dev]).all()
    else:
        assert np.array_equal(moved["rx_power"], before["rx_power"]), "stored powers stay stale beyond 3000 m"
    g.runSimulation(t2)
    for w in worlds:
        w.run(t2)
    compare("after the second run")
    assert last_width(g) == 64
    g.close()
