"""
gw_rollout_autoreset, the part that needs no GPU: argument validation of the entry point, the shim's function for it, and the
catalogue of the fused family -- the library's ct_rollout_sync_ep<DT, MODE> instantiations are exactly the cases
tests/test_rollout_autoreset.py runs.
"""
import ctypes as C
import os
import sys

import pytest

from util import kernel_instantiations


def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = C.c_void_p(16)
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, 16, None)                                   # tally_dev may be NULL
    # gw_rollout_autoreset(env, steps, device, duration, ep, obs_next, obs, reward, done, ended, stream)
    def call(env, steps, ptrs, ep_ref):
        return L.gw_rollout_autoreset(env, steps, ptrs[0], ptrs[1], ep_ref, *ptrs[2:], None)
    seven = [one] * 7
    assert call(None, 4, seven, C.byref(ep)) == nat.EINVAL
    assert b"env is NULL" in L.gw_last_error()
    assert call(fake, -1, seven, C.byref(ep)) == nat.EINVAL
    assert b"steps" in L.gw_last_error()
    for hole in range(7):
        ptrs = list(seven)
        ptrs[hole] = None
        assert call(fake, 4, ptrs, C.byref(ep)) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
        assert call(fake, 0, ptrs, C.byref(ep)) == nat.EINVAL, hole     # (before steps == 0 is looked at)
    assert call(fake, 4, seven, None) == nat.EINVAL
    assert call(fake, 4, seven, C.byref(nat.Episodes(5, 1, None, 16))) == nat.EINVAL
    assert b"NULL" in L.gw_last_error()
    assert call(fake, 4, seven, C.byref(nat.Episodes(-1, 1, 16, 16))) == nat.EINVAL
    assert b"max_steps" in L.gw_last_error()
    assert call(fake, 0, seven, C.byref(ep)) == nat.OK
    assert call(fake, 0, seven, C.byref(nat.Episodes(0, 0, 16, None))) == nat.OK


def test_the_shim_builds_the_episode_record_itself(native_lib):
    """rollout_autoreset(env, steps, device, duration, max_steps, on_done, state, tally, obs_next, obs, reward, done, ended,
    stream): the same validation answers as through ctypes, so the record reached the library with its fields in place."""
    from gymwipe_amd import _native as nat
    fast = nat.fast()
    if fast is None:
        pytest.skip("the CPython shim is not built")
    L = native_lib
    args = [4096, 4, 16, 16, 5, 1, 16, 0, 16, 16, 16, 16, 16, 0]
    assert fast.rollout_autoreset(*(args[:1] + [0] + args[2:])) == nat.OK              # steps == 0
    assert fast.rollout_autoreset(*([0] + args[1:])) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert fast.rollout_autoreset(*(args[:1] + [-1] + args[2:])) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert fast.rollout_autoreset(*(args[:4] + [-1] + args[5:])) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    assert fast.rollout_autoreset(*(args[:6] + [0] + args[7:])) == nat.EINVAL and b"NULL" in L.gw_last_error()   # state_dev
    for hole in (2, 3, 8, 9, 10, 11, 12):
        a = list(args)
        a[hole] = 0
        assert fast.rollout_autoreset(*a) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    with pytest.raises(TypeError):
        fast.rollout_autoreset(*args[:-1])
    with pytest.raises(OverflowError):
        fast.rollout_autoreset(*(args[:1] + [1 << 40] + args[2:]))


def test_step_outputs_takes_an_ended_tensor_beside_its_four_addresses():
    """The native stepper reads StepOutputs._ptrs as four addresses: `ended` has a slot of its own."""
    from gymwipe_amd import StepOutputs
    assert {"ended", "_ended_ptr", "_ptrs"} <= set(StepOutputs.__slots__)


def test_every_autoreset_rollout_instantiation_has_a_gpu_case(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_autoreset as ra
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_sync_ep")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(ra.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(ra.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"
