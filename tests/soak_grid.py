#!/usr/bin/env python3
"""Longer PHY-grid parity runs than the pytest tier affords (the event-driven Python model is the slow side):
   python tests/soak_grid.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_grid as t
import test_grid_widths as tw

BIG = len(sys.argv) > 1 and sys.argv[1] == "big"
if len(sys.argv) > 1 and sys.argv[1] == "walks":
    # CPU only: the event-driven model runs through in EVERY replica of the mobile cases of tests/test_grid_widths.py (where
    # the reference would trip its own `assert noise >= 0`, it raises here) -- what their `flags == 0` over all N rests on
    from oracle import des_model as dm
    for (n, N, power), (walk, _) in sorted(tw.MOBILE_SETUP.items()):
        T, rows = tw.mobile_run_length(n, N, power), tw.delay_rows(n, (800 if power == 40.0 else tw.BER_MOBILE_SEED) + n)
        for e in range(N):
            dm.scenario_mobile_grid(n, rows[e % tw.K].tolist(), T, seed=walk, replica=e, runs=[T * 0.5, T * 0.5], tx_power_dbm=power)
        print("n=%d N=%d %+.0f dBm walk seed %d: the model runs through in all replicas" % (n, N, power, walk), flush=True)
    sys.exit(0)
STATIC = ((4, 8, 1.0), (9, 8, 1.0), (16, 6, 1.0), (25, 3, 0.5))
MOBILE = ((4, 4, 0.6), (9, 4, 0.5), (16, 2, 0.4))
if BIG:
    STATIC = ((2, 32, 5.0), (4, 32, 4.0), (16, 32, 3.0), (20, 16, 2.0), (32, 8, 1.0), (49, 4, 0.6), (64, 4, 0.5))
    MOBILE = ((2, 16, 3.0), (4, 16, 2.0), (16, 8, 1.5), (32, 4, 0.5), (64, 2, 0.2))
t0 = time.time()
for n, N, T in STATIC:
    t.test_grid_kernel_matches_event_driven_oracle(n, N, T)
    print("static n=%d N=%d T=%.1f ok (%.0f s)" % (n, N, T, time.time() - t0), flush=True)
for n, N, T in MOBILE:
    t.test_mobile_grid_kernel_matches_event_driven_oracle(n, N, T)
    print("mobile n=%d N=%d T=%.1f ok (%.0f s)" % (n, N, T, time.time() - t0), flush=True)
# tests/test_grid_widths.py.  The mobile cases and Position.set() exactly as the suite runs them (the walk seeds hold for their
# own run lengths only, the Position.set() instants come from the oracle's log); then the static grid, all replicas
# compared, at longer T
for width, n, N in tw.MOBILE_CASES:
    tw.check_mobile(width, n, N, 40.0, 800 + n)
    print("mobile width=%d n=%d N=%d ok (%.0f s)" % (width, n, N, time.time() - t0), flush=True)
for width, n, N in tw.BER_MOBILE_CASES:
    tw.assert_ber_decides(tw.check_mobile(width, n, N, tw.BER_POWERS[n], tw.BER_MOBILE_SEED + n), "mobile n = %d" % n)
    print("ber mobile width=%d n=%d N=%d ok (%.0f s)" % (width, n, N, time.time() - t0), flush=True)
for case in ("A", "B", "standby"):
    for n in (4, 9):
        tw.test_set_position_between_runs_matches_oracle(n, case)
        print("setPosition %s n=%d ok (%.0f s)" % (case, n, time.time() - t0), flush=True)
tw.run_length = lambda n: (0.6 if BIG else 0.3) if n <= 9 else (0.3 if BIG else 0.15)
for width, n, N in tw.STATIC_CASES:
    tw.check_static(width, n, N, 40.0, 700 + n)
    print("static width=%d n=%d N=%d ok (%.0f s)" % (width, n, N, time.time() - t0), flush=True)
for width, n, N in tw.BER_STATIC_CASES:
    tw.check_static(width, n, N, tw.BER_POWERS[n], tw.BER_STATIC_SEED + n)
    print("ber static width=%d n=%d N=%d ok (%.0f s)" % (width, n, N, time.time() - t0), flush=True)
print("grid soak ok")
