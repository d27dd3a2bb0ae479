"""Test infrastructure, not a test: the control-loop model with the plant of gw_ctrl_set_disturbance (include/gymwipe_amd.h) --
``oracle/des_model.LinearPlant`` whose substep ends with one draw of counter-based noise.  The rule, the weight sets and the seed
are stated here; tests/ctrl_tiers.py builds the references from them, and its reset hands the old plant's record to the fresh model.

``DisturbedPlant.step()`` runs the parent's substep ``nx = A x + B u`` and then, in pure Python integers and floats:

    z  = key ^ (n * 0xD1B54A32D192ED03)                       (mod 2^64)
    z += 0x9E3779B97F4A7C15
    z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z ^= z >> 31
    w  = (signed 32-bit reading of z >> 32) * 2^-31            every operation exact
    x[i] = nx[i] + g[i] * w                                    Python rounds the product, then the sum
    n += 1

``disturb(model, g, key, n)`` assigns such a plant to ``model.plant`` of a built ``PidControlLoopModel``: the sensor's process, the
actuator's delivery and the snapshot all look the attribute up when they run.  A reset env is a fresh model whose plant goes on
drawing where the old one stopped: ``g``, ``key`` and ``n`` survive, everything else is new.  ``restart_n`` (tests/ctrl_tiers.py) is
the wrong reset the CPU qualification compares against.

The weight sets tests/test_ctrl_disturbance.py runs on are defined here and qualified on the model alone in
tests/test_ctrl_disturbance_cpu.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_pid_model as pm
from oracle import des_model as dm

M64 = (1 << 64) - 1
STREAM_STEP = 0x9E3779B97F4A7C15


def noise(key, n):
    """The rule's ``w`` for one key and count, Python integers throughout."""
    z = (key ^ ((n * 0xD1B54A32D192ED03) & M64)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    top = z >> 32
    return float(top - (1 << 32) if top >= (1 << 31) else top) * 2.0 ** -31


def key_of(seed, stream):
    """``actions.make_ctrl_disturbance``'s key of one stream number, restated."""
    return (int(seed) ^ ((int(stream) * STREAM_STEP) & M64)) & M64


class DisturbedPlant(dm.LinearPlant):
    def __init__(self, A, B, x0, u0, g=(0.0, 0.0, 0.0, 0.0), key=0, n=0):
        dm.LinearPlant.__init__(self, A, B, x0, u0)
        self.g, self.key, self.n = tuple(float(v) for v in g), int(key), int(n)

    def step(self):
        dm.LinearPlant.step(self)                          # nx = A x + B u, substeps += 1
        w = noise(self.key, self.n)
        self.x = [self.x[i] + self.g[i] * w for i in range(4)]
        self.n += 1


def disturb(model, g, key, n=0):
    """Replace the plant of a built model by a disturbed one in the same state; returns the model."""
    old = model.plant
    model.plant = DisturbedPlant(old.A, old.B, old.x, old.u, g, key, n)
    model.plant.substeps = old.substeps
    return model


# ---- fixtures of tests/test_ctrl_disturbance.py ---------------------------------------------------------------------------------------------
# 8 weight sets: none first (its envs must walk the undisturbed trajectory), each plant state alone, then mixtures of both
# signs.  Set i runs under pm.GAIN_SETS[i]: the disturbance instantiations are PID instantiations, and both rules are exercised.
G_SETS = ((0.0, 0.0, 0.0, 0.0), (0.01, 0.0, 0.0, 0.0), (0.0, 0.01, 0.0, 0.0), (0.0, 0.0, 0.002, 0.0), (0.0, 0.0, 0.0, 0.01),
          (0.001, 0.002, 0.0005, 0.01), (0.0, 0.0, 0.0, 0.05), (-0.002, 0.0, 0.001, -0.02))
G = len(G_SETS)
assert G == pm.G
SEED = 0xC0FFEE0DDF00D5EED                                   # wider than 64 bits: the helper takes its low 64
SEED64 = SEED & M64
STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = pm.STEPS, pm.MAX_STEPS, pm.SHORT_MAX_STEPS, pm.FAIL_DEG
P, N_FUSED, PER_SET = pm.P, pm.N_FUSED, pm.PER_SET


def g_array():
    return np.array(G_SETS, np.float64)


def step_noise_stream(gi, s):
    """The step cases' noise stream number of (weight set, action stream): one per pair, so that 64 models stand for N envs."""
    return int(gi) * 8 + int(s)


def fused_noise_stream(p, g, b):
    """The fused cases' noise stream number of (schedule or policy, weight set, b): one per model."""
    return (p * G + g) * 2 + b
