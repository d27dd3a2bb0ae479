"""Test infrastructure, not a test: the control-loop model with the packet erasures of gw_ctrl_set_loss (include/gymwipe_amd.h)
-- tests/ctrl_dist_model.py's disturbed PID model whose band takes one counter-based draw per transmission.  The rule, the loss
sets and the seed are stated here; tests/ctrl_tiers.py builds the references from them, and its reset hands the old model's loss
record to the fresh one.

``attach(model, thr, key, n, lost)`` hooks a built model from outside, nothing in oracle/des_model.py is edited:

  * ``model.world.band.transmit`` is wrapped as an instance attribute.  Every transmission goes through it exactly once, when it
    goes on the air and before any PHY has decided about it.  The link comes from the packet's MAC header: ``src == RRM`` makes
    it link 0 (``dst`` the sensor) or 1 (the controller); otherwise it is 2 + the sender's index (sensor 2, controller 3).  In
    pure Python integers:

        z  = key ^ (n * 0xA0761D6478BD642F)                       (mod 2^64)
        z += 0x9E3779B97F4A7C15
        z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
        z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
        z ^= z >> 31
        r  = z >> 32
        erased = r < thr[link];  lost[link] += erased (mod 2^32);  n += 1

    and the packet is marked.
  * every radio's ``phy.mac_out.trigger`` is wrapped, an instance attribute as well (``Phy._receive`` looks it up when it has
    decoded a packet): an erased packet is not handed up.  The MAC of an erased announcement's addressee never opens its window;
    an erased data packet has left its queue and been on the air, and reaches nobody.

A reset env is a fresh model that goes on drawing where the old one stopped: ``thr``, ``key``, ``n`` and ``lost`` survive.
``mode`` selects one of the wrong rules the CPU qualification compares against: ``"phy_only"`` (the draw is taken only when the
addressee's PHY decoded the packet), ``"one_thr"`` (threshold 0 for all links), ``"no_pop"`` (an erased data packet goes back to
the head of its queue); ``restart_loss_n`` (tests/ctrl_tiers.py) is the wrong reset.

The loss sets tests/test_ctrl_loss.py runs on are defined here and qualified on the model alone in tests/test_ctrl_loss_cpu.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_pid_model as pm
from oracle import des_model as dm

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
LOSS_FIELDS = ("loss", "loss_key", "loss_count", "lost")


def draw(key, n):
    """The rule's ``r`` for one key and count, Python integers throughout."""
    z = (key ^ ((n * 0xA0761D6478BD642F) & M64)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


class LossRecord:
    """An env's record {thr, key, n, lost}, and what the qualification asks about it: per link the receptions the addressee's PHY
    decoded and the rule erased, and those delivered; the draws that fell on transmissions the addressee's PHY rejected."""

    def __init__(self, thr, key, n=0, lost=(0, 0, 0, 0), mode=None):
        self.thr, self.key, self.n, self.lost = [int(v) for v in thr], int(key), int(n), [int(v) for v in lost]
        self.mode = mode
        self.erased_decoded, self.delivered = [0, 0, 0, 0], [0, 0, 0, 0]
        self.sent = []                                       # every packet that took a draw

    def take(self, link):
        r = draw(self.key, self.n)
        erased = r < self.thr[0 if self.mode == "one_thr" else link]
        if erased:
            self.lost[link] = (self.lost[link] + 1) & M32
        self.n = (self.n + 1) & M64
        return erased

    @property
    def rejected_draws(self):
        return sum(1 for p in self.sent if not p.loss_decoded)

    def carry(self, old):
        """Bookkeeping across a reset: the qualification counts over all episodes of an env."""
        self.erased_decoded, self.delivered, self.sent = old.erased_decoded, old.delivered, old.sent


def attach(model, thr, key, n=0, lost=(0, 0, 0, 0), mode=None):
    """Hook the rule into a built model; returns the model.  ``model.loss`` is its LossRecord."""
    rec = model.loss = LossRecord(thr, key, n, lost, mode)
    band = model.world.band
    sensor, controller, _ = model.devs
    index_of = {d.mac_addr: i for i, d in enumerate(model.devs)}

    def link_of(packet):
        h = packet.header
        if h.src == dm.RRM_ADDR:
            return 0 if h.dst == sensor.mac_addr else 1
        return 2 + index_of[h.src]

    inner_transmit = band.transmit

    def transmit(sender, power, packet, mcs_h, mcs_p):
        packet.loss_link = link_of(packet)
        packet.loss_decoded = False
        packet.loss_erased = False
        if rec.mode != "phy_only":
            packet.loss_erased = rec.take(packet.loss_link)
            rec.sent.append(packet)
            if packet.loss_erased and rec.mode == "no_pop" and packet.loss_link >= 2:
                sender.mac.queue.appendleft(packet)
        return inner_transmit(sender, power, packet, mcs_h, mcs_p)
    band.transmit = transmit

    def hook(radio, addr):
        inner = radio.phy.mac_out.trigger

        def trigger(packet):
            if packet.header.dst == addr:                    # the addressee's PHY has decoded it
                packet.loss_decoded = True
                if rec.mode == "phy_only":
                    packet.loss_erased = rec.take(packet.loss_link)
                    rec.sent.append(packet)
                if packet.loss_erased:
                    rec.erased_decoded[packet.loss_link] += 1
                else:
                    rec.delivered[packet.loss_link] += 1
            if not packet.loss_erased:
                inner(packet)
        radio.phy.mac_out.trigger = trigger
    for d in model.devs:
        hook(d, d.mac_addr)
    hook(model.rrm, dm.RRM_ADDR)
    return model


# ---- fixtures of tests/test_ctrl_loss.py ----------------------------------------------------------------------------------------------------
# 8 loss sets as probabilities per link (announcement to the sensor, to the controller, sensor's data, controller's data): none
# first (its envs must walk the disturbance model's trajectory), the announcements only, the data links only, mixtures, and last
# both announcements at thr = 0xFFFFFFFF, where no step is ever granted.  Set i runs under cd.G_SETS[i] and pm.GAIN_SETS[i]: the
# loss instantiations are disturbance and PID instantiations, and all three rules run together.
P_SETS = ((0.0, 0.0, 0.0, 0.0), (0.3, 0.3, 0.0, 0.0), (0.0, 0.0, 0.3, 0.3), (0.25, 0.1, 0.4, 0.2), (0.1, 0.25, 0.2, 0.4),
          (0.5, 0.5, 0.5, 0.5), (0.05, 0.6, 0.7, 0.05), (1.0, 1.0, 0.5, 0.5))
G = len(P_SETS)
assert G == pm.G == cd.G
ALL_LOST = 7                                                 # the set with 0xFFFFFFFF on both announcement links
SEED = 0x5EED0F10557DA7A5EED                                 # wider than 64 bits: the helper takes its low 64
SEED64 = SEED & M64
STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = pm.STEPS, pm.MAX_STEPS, pm.SHORT_MAX_STEPS, pm.FAIL_DEG
P, N_FUSED, PER_SET = pm.P, pm.N_FUSED, pm.PER_SET
FAILING_LAYOUT = "same_distance"                             # tests/ctrl_fixtures.LAYOUTS: the commands do not decode


def threshold(p):
    """``actions.ctrl_loss_threshold`` restated for one probability in [0, 1]."""
    return min(int(p * 4294967296.0), M32)


THR_SETS = tuple(tuple(threshold(p) for p in row) for row in P_SETS)
assert THR_SETS[0] == (0, 0, 0, 0) and THR_SETS[ALL_LOST][:2] == (M32, M32)


def thr_array():
    return np.array(THR_SETS, np.uint32)
