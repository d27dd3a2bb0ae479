"""The tier record of tests/ctrl_tiers.py and the shared comparison of tests/ctrl_gpu_harness.py, CPU tier: each tier's field
tuples are pinned literally, and the comparison the three GPU files share is shown to visit every one of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_gpu_harness as h
from ctrl_tiers import DIST, LOSS, PID

BASE_STATE = ("now", "x", "u", "angle_deg", "rx_power", "qlen", "received", "n_tx", "commands", "substeps",
              "wake", "flags", "age", "cost", "x_init", "u_init")
BASE_MODEL = ("now", "x", "u", "angle_deg", "rx_power", "qlen", "received", "n_tx", "commands", "substeps")
PID_NEW = ("gains", "last_error")
DIST_NEW = ("gains", "last_error", "disturbance", "noise_key", "noise_count")
LOSS_NEW = ("gains", "last_error", "disturbance", "noise_key", "noise_count", "loss", "loss_key", "loss_count", "lost")
PINNED = {PID: (BASE_STATE + PID_NEW, BASE_MODEL + PID_NEW), DIST: (BASE_STATE + DIST_NEW, BASE_MODEL + DIST_NEW),
          LOSS: (BASE_STATE + LOSS_NEW, BASE_MODEL + LOSS_NEW)}
DTYPES = {"gains": np.float64, "last_error": np.float64, "disturbance": np.float64, "noise_key": np.uint64, "noise_count": np.uint64,
          "loss": np.uint32, "loss_key": np.uint64, "loss_count": np.uint64, "lost": np.uint32,
          "qlen": np.int32, "received": np.int32, "n_tx": np.int32, "commands": np.int32, "substeps": np.int64, "flags": np.int32,
          "age": np.int32}
N = 5


def _state(fields):
    """A state of N envs with every field of ``fields`` in a dtype of its own kind, three values per env, none of them 0."""
    rng = np.random.default_rng(3)
    out = {}
    for f in fields:
        dtype = DTYPES.get(f, np.float64)
        if dtype == np.float64:
            out[f] = rng.uniform(0.5, 1.5, (N, 3))
        else:
            out[f] = (rng.integers(1, 2 ** 20, (N, 3)) * 4).astype(dtype)        # (flags: bits 0 and 1 clear)
    return out


def _one_bit_off(state, f):
    """``state`` with the lowest bit of one element of field f flipped; every other field is the same array."""
    other = dict(state)
    a = state[f].copy()
    bits = a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
    bits[2, 1] ^= 1
    other[f] = a
    return other


def test_each_tiers_field_tuples_are_pinned_and_the_shared_comparison_visits_every_field():
    import test_ctrl_disturbance
    import test_ctrl_gains
    import test_ctrl_loss
    used = {PID: (test_ctrl_gains.PID_FIELDS, test_ctrl_gains.MODEL_FIELDS), DIST: (test_ctrl_disturbance.DIST_FIELDS, test_ctrl_disturbance.MODEL_FIELDS),
            LOSS: (test_ctrl_loss.LOSS_STATE, test_ctrl_loss.MODEL_FIELDS)}
    for tier in (PID, DIST, LOSS):
        state_fields, model_fields = PINNED[tier]
        assert used[tier] == (state_fields, model_fields), tier.name
        assert h.state_fields(tier) == state_fields and h.model_fields(tier) == model_fields, tier.name
        st = _state(state_fields)
        h.assert_states_equal(tier, st, dict(st), "equal")
        for f in state_fields:
            with pytest.raises(AssertionError):
                h.assert_states_equal(tier, st, _one_bit_off(st, f), f)
            with pytest.raises(AssertionError):
                h.assert_states_equal(tier, _one_bit_off(st, f), st, f)
        # check_final: the reference holds the same values behind an index; the model fields, age and cost are compared
        final = {f: np.stack([v, v]) for f, v in st.items()}
        h.check_final(tier, st, final, 1, "equal")
        for f in model_fields + ("age", "cost"):
            with pytest.raises(AssertionError):
                h.check_final(tier, _one_bit_off(st, f), final, 1, f)
            wrong = dict(final)
            wrong[f] = np.stack([st[f], _one_bit_off(st, f)[f]])
            with pytest.raises(AssertionError):
                h.check_final(tier, st, wrong, 1, f)
        flagged = dict(st)
        flagged["flags"] = st["flags"] | 1
        with pytest.raises(AssertionError):
            h.check_final(tier, flagged, final, 1, "flags")
