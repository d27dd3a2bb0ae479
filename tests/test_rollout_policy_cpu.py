"""
gw_rollout_policy, the part that needs no GPU: the table rules of actions.policy_cdf, the CPU restatement of the draw
(actions.policy_sample_numpy), argument validation of the entry point, and the catalogue of the fused family --
the library's ct_rollout_policy<DT, MODE> instantiations are exactly the cases tests/test_rollout_policy.py runs.
"""
import ctypes as C
import os
import sys

import numpy as np

from gymwipe_amd import actions


def _rows(A=40, seed=3):
    """Three Dirichlet(0.3) rows with a quarter of the actions at p = 0, a one-hot row, and a row whose last action has
    p = 0 (and whose first has, too)."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(A, 0.3), size=3)
    p[:, rng.permutation(A)[:A // 4]] = 0.0
    p /= p.sum(axis=1, keepdims=True)
    onehot = np.zeros(A)
    onehot[17] = 1.0
    tail0 = rng.dirichlet(np.full(A, 0.3))
    tail0[[0, A - 1]] = 0.0
    tail0 /= tail0.sum()
    return np.vstack([p, onehot, tail0])


def test_policy_cdf_rows_are_monotone_with_the_all_ones_tail():
    p = _rows()
    cdf = actions.policy_cdf(p)
    assert cdf.dtype == np.uint32 and cdf.shape == p.shape
    assert (np.diff(cdf.astype(np.int64), axis=1) >= 0).all()
    for row, c in zip(p, cdf):
        last = np.flatnonzero(row > 0)[-1]
        assert (c[last:] == 0xffffffff).all() and (c[:last] < 0xffffffff).all()
        exact = np.floor(np.cumsum(row, dtype=np.float64) * 2.0 ** 32)
        assert (c[:last] == exact[:last]).all()
        zero = np.flatnonzero(row == 0)
        prev = np.where(zero > 0, c[np.maximum(zero - 1, 0)], 0)      # cdf[-1] is 0 by convention
        assert (c[zero][zero < last] == prev[zero < last]).all()      # (behind `last` both are the all-ones tail)
    import torch
    assert (actions.policy_cdf(torch.from_numpy(p)).numpy() == cdf).all()          # the torch form, same rule


def test_draws_never_hit_a_zero_probability_action_and_match_the_probabilities():
    """2^20 draws per row from the counter-based stream (fixed seed: deterministic).  Per action the count is binomial, so
    its standard error is sqrt(n p (1 - p)); the table's own quantisation (2^-32 per entry) is far below that."""
    p = _rows()
    cdf = actions.policy_cdf(p)
    n = 1 << 20
    u = actions.policy_u_numpy(20260117, 0, n, 5)
    assert u.dtype == np.uint32 and u.max() <= 0xfffffffe
    for r in range(len(p)):
        a = actions.policy_count_numpy(cdf, np.full(n, r), u)
        counts = np.bincount(a, minlength=p.shape[1])
        assert counts[p[r] == 0].sum() == 0, r
        se = np.sqrt(n * p[r] * (1.0 - p[r]))
        assert (np.abs(counts - n * p[r]) <= 5.0 * se).all(), (r, np.abs(counts - n * p[r]).max())


def test_the_ends_of_the_draw():
    """u = 0 picks the first action with p > 0; the hash's 0xffffffff is clamped to 0xfffffffe and picks the last action with
    p > 0; a table that is not a cdf at all still yields an action inside [0, A)."""
    p = _rows()
    cdf = actions.policy_cdf(p)
    A = p.shape[1]
    for r in range(len(p)):
        nz = np.flatnonzero(p[r] > 0)
        lo = actions.policy_count_numpy(cdf, np.array([r]), np.array([0], np.uint32))[0]
        hi = actions.policy_count_numpy(cdf, np.array([r]), np.array([0xfffffffe], np.uint32))[0]
        assert lo == nz[0] and hi == nz[-1], (r, lo, hi)
    zeros = np.zeros((3, A), np.uint32)                                # every entry <= u: the count is A, clamped to A - 1
    assert actions.policy_count_numpy(zeros, np.array([1]), np.array([7], np.uint32))[0] == A - 1
    # policy_sample_numpy: class from the observation, flat action -> (device, duration)
    obs = np.array([65534, 65536, 65538, 65538], np.int32)
    dev, dur = actions.policy_sample_numpy(9, 10, 14, 3, cdf[:3], obs, 65536, 20)
    a = actions.policy_count_numpy(cdf[:3], np.array([0, 1, 2, 2]), actions.policy_u_numpy(9, 10, 14, 3))
    assert dev.dtype == np.int32 and (dev == a // 20).all() and (dur == a % 20).all()
    # the stream is the action stream's own hash (low 32 bits), so shards and steps line up with actions_numpy
    low, _ = actions.actions_numpy(9, 10, 14, 3, 4, 1 << 32, 1)
    assert (np.minimum(low[0].view(np.uint32), 0xfffffffe) == actions.policy_u_numpy(9, 10, 14, 3)).all()


def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = C.c_void_p(16)
    assert L.gw_rollout_policy(None, 4, one, 1, 0, 0, one, one, one, one, one, one, None) == nat.EINVAL
    assert b"env is NULL" in L.gw_last_error()
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    assert L.gw_rollout_policy(fake, -1, one, 1, 0, 0, one, one, one, one, one, one, None) == nat.EINVAL
    for hole in range(7):
        ptrs = [one] * 7
        ptrs[hole] = None
        rc = L.gw_rollout_policy(fake, 4, ptrs[0], 1, 0, 0, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], None)
        assert rc == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_rollout_policy(fake, 0, one, 1, 0, 0, one, one, one, one, one, one, None) == nat.OK


def test_every_policy_rollout_instantiation_has_a_gpu_case(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_policy as rp
    from util import kernel_instantiations
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_policy")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(rp.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(rp.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"
