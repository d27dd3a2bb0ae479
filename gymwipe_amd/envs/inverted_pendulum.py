"""
Host-side mirror of gymwipe/envs/inverted_pendulum.py for N environments on one MI355X.

The reference env assigns the frequency band to an angle sensor (device index 0) and a PID controller
(index 1) of a sliding pendulum and reads observation and reward straight off the plant
(``InvertedPendulumInterpreter``, envs/inverted_pendulum.py:27-57):

    observation = int(degrees(angle))        reward = float(abs(180 - degrees(angle)))       done = False

What this class keeps of it, and what it cannot:

* the gym surface (action space of two devices x 20 durations, ``observation_space = Discrete(180)``,
  ``step`` = assign, run to the end of the assignment, read the plant) and the interpreter's formulas, evaluated on
  the GPU (``gw_plant_feedback``);
* the network of the env AS SHIPPED: the sensor samples every millisecond (sliding_pendulum.py:116-135), nobody sets
  ``receiving``, so the controller's angle stays 0, its control loop never sends (control/inverted_pendulum.py:52-69)
  and the loop is open -- a sender with multiplicity 1 and a silent one (multiplicity 0) on the CounterTraffic step
  kernel, controller at (0, -1), RRM at (0, 1), sensor at the wagon's start (0, 0) (envs/inverted_pendulum.py:75-93);
* the plant is BUILDER-DEFINED: the reference integrates an ODE rigid-body world (py3ode, absent) inside an env that
  cannot even be constructed (simtools.py:39-42); here ``VecLinearPlant`` advances a linear model ``x <- A x + B u`` to the
  env clock on the f64 matrix cores.  Parity with the reference is therefore unpinned for this env; the sensor's packet
  sizes follow the counter-traffic rule (25 + counter bytes), not the reference's ``Transmittable(2, angle)``, whose
  byte size is the angle itself.
"""
import ctypes as C

from .. import _native as nat
from .. import spaces
from ..plants import VecLinearPlant
from .core import BaseEnv
from .counter_traffic import VecCounterTrafficEnv


class VecInvertedPendulumEnv(BaseEnv):
    SENSOR, CONTROLLER = 0, 1                              # deviceIndexToMacDict, envs/inverted_pendulum.py:86-89
    SAMPLE_INTERVAL = 0.001                                # :79

    _scalar_api = False

    def __init__(self, num_envs, device="cuda:0", plant=None):
        import torch
        self._torch = torch
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        BaseEnv.__init__(self, 2)                          # deviceCount=2, :70
        self.observation_space = spaces.Discrete(180)      # :73
        self.network = VecCounterTrafficEnv(self.num_envs, 2, device=self.device,
                                            positions=[(0.0, 0.0), (0.0, -1.0)], rrm_position=(0.0, 1.0),
                                            multiplicity=[1, 0], dest=[1, 0])
        self.plant = plant if plant is not None else VecLinearPlant(self.num_envs, device=self.device)
        base, stride = C.c_void_p(), C.c_int64()
        nat.check(self.network._L.gw_now_ptr(self.network._h, C.byref(base), C.byref(stride)))
        self._now = (base.value, stride.value)             # the env clock, read by the plant kernel in place
        n = self.num_envs
        self._obs = torch.empty(n, dtype=torch.int32, device=self.device)
        self._rew = torch.empty(n, dtype=torch.float32, device=self.device)
        self._angle = torch.empty(n, dtype=torch.float64, device=self.device)
        self._done = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._out_ptrs = (self._obs.data_ptr(), self._rew.data_ptr(), self._angle.data_ptr())   # fixed output buffers
        self._fb = (self._obs, self._rew, self._done, {"Sensor angle": self._angle})

    def _feedback(self):
        torch = self._torch
        with torch.cuda.device(self.device):
            nat.check(self.plant._L.gw_plant_feedback(self.plant._h, self._obs.data_ptr(), self._rew.data_ptr(),
                                                      self._angle.data_ptr(),
                                                      torch.cuda.current_stream(self.device).cuda_stream))
        return self._obs, self._rew, self._done, {"Sensor angle": self._angle}

    def reset(self):
        """envs/inverted_pendulum.py:95-99: returns an observation, resets nothing."""
        return self._feedback()[0]

    def step(self, action, fused=True):
        """:101-113 for every env: assign the band, run to the end of the assignment, read the plant -- ONE kernel launch
        (``gw_pendulum_step``: band-assignment step + plant advance on the matrix cores + interpreter feedback).
        ``fused=False`` issues the same work as two launches (``gw_step`` + ``gw_plant_update_feedback``); results are identical."""
        torch = self._torch
        net = self.network
        if not fused:
            net.step(action)
            with torch.cuda.device(self.device):           # OdePlant.updateState to the new env clock + the interpreter's
                nat.check(self.plant._L.gw_plant_update_feedback(    # reading of the plant
                    self.plant._h, self._now[0], self._now[1], self._obs.data_ptr(), self._rew.data_ptr(),
                    self._angle.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
            return self._obs, self._rew, self._done, {"Sensor angle": self._angle}
        dev = net._checked(action["device"], "device")
        dur = net._checked(action["duration"], "duration")
        idx = net._dev_index
        if torch._C._cuda_getDevice() == idx:                  # the one-process-per-GPU case: no context switch
            fast = net._fast
            if fast is not None:
                rc = fast.pendulum_step(net._h.value or 0, self.plant._h.value or 0, dev.data_ptr(), dur.data_ptr(),
                                        self._out_ptrs[0], self._out_ptrs[1], self._out_ptrs[2],
                                        torch._C._cuda_getCurrentRawStream(idx))
            else:
                rc = net._L.gw_pendulum_step(net._h, self.plant._h, dev.data_ptr(), dur.data_ptr(), self._out_ptrs[0],
                                             self._out_ptrs[1], self._out_ptrs[2], torch._C._cuda_getCurrentRawStream(idx))
        else:
            with torch.cuda.device(self.device):
                rc = net._L.gw_pendulum_step(net._h, self.plant._h, dev.data_ptr(), dur.data_ptr(), self._out_ptrs[0],
                                             self._out_ptrs[1], self._out_ptrs[2],
                                             torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            nat.check(rc)
        return self._fb

    def render(self, mode="human", close=False):           # :115-116
        pass

    def close(self):
        self.network.close()
        self.plant.close()


class InvertedPendulumEnv(VecInvertedPendulumEnv):
    """N = 1 with the reference's scalar surface: ``step({"device": int, "duration": int}) ->
    (int, float, bool, {"Sensor angle": float})``, ``AssertionError`` on an action outside the action space."""
    _scalar_api = True

    def __init__(self, device="cuda:0"):
        VecInvertedPendulumEnv.__init__(self, 1, device=device)
        self._act = self._torch.zeros((2, 1), dtype=self._torch.int32, device=self.device)

    def _scalars(self, fb):
        obs, rew, done, info = fb
        return int(obs.item()), float(rew.item()), bool(done.item()), {"Sensor angle": float(info["Sensor angle"].item())}

    def reset(self):
        return self._scalars(self._feedback())[0]

    def step(self, action):
        assert self.action_space.contains(action)          # :102
        self._act[0, 0] = int(action["device"])
        self._act[1, 0] = int(action["duration"])
        return self._scalars(VecInvertedPendulumEnv.step(self, {"device": self._act[0], "duration": self._act[1]}))


class VecControlLoopEnv(BaseEnv):
    """The pendulum env with its control loop CLOSED over receive-mode MACs: what the reference
    intends (sensor -> controller -> actuator, plants/sliding_pendulum.py:116-155, control/inverted_pendulum.py:16-69)
    but never runs.  Builder-defined where the reference leaves it open -- see ``gw_ctrl_config`` in
    include/gymwipe_amd.h for the rules -- and checked bit for bit against an event-driven model of those rules.
    Same gym surface as ``VecInvertedPendulumEnv``: ``step({"device": int32[N] in {0 sensor, 1 controller},
    "duration": int32[N]}) -> (obs, reward, done, {"Sensor angle": deg})``.
    Beyond one step per launch: ``set_initial_state`` / ``reset_envs`` (an initial state per env; a masked reset that leaves a
    fresh env), ``rollout`` (K steps in one launch, optionally with episodes that end at a time limit or a failure angle and
    reset inside the launch), ``rollout_schedules`` (P cyclic band schedules, a per-env tally, nothing stored per step) and
    ``rollout_feedback`` (P angle-feedback schedulers: the env's own angle picks which of B schedules it acts on).
    The controller is the reference's three-term PID on gains every env holds of its own: ``set_gains`` (or ``gains=`` here);
    the default, the reference's shipped (1, 0, 0), commands ``-angle``.  Gains laid across the envs of each schedule
    (``actions.make_ctrl_gains``) make the rollout calls rank controllers and schedulers together.
    The plant is exact unless ``set_disturbance`` (or ``disturbance=`` here) gives envs seeded noise on their plant's state:
    something to hold the pendulum against after the transient, keyed per env so that candidates can face the same noise.
    The radio links are the PHY's deterministic ones unless ``set_loss`` (or ``loss=`` here) gives each of the four links a loss
    probability: every transmission then takes one seeded draw and an erased packet is sent and not delivered, an erased
    announcement an ungranted step; keyed per env as the disturbance is."""
    SENSOR, CONTROLLER, ACTUATOR = 0, 1, 2

    def __init__(self, num_envs, device="cuda:0", ctrl_start_tick=None, ctrl_period_ticks=None, positions=None, x0=None,
                 A=None, B=None, u0=None, counter_interval=None, gains=None, disturbance=None, loss=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gymwipe_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self._torch = torch
        self._L = nat.lib()
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        BaseEnv.__init__(self, 2)
        self.observation_space = spaces.Discrete(180)
        cfg = nat.CtrlConfig()
        nat.check(self._L.gw_ctrl_config_default(C.byref(cfg), self.num_envs))
        cfg.net.hip_device = self.device.index or 0
        if ctrl_start_tick is not None:
            cfg.ctrl_start_tick = int(ctrl_start_tick)
        if ctrl_period_ticks is not None:
            cfg.ctrl_period_ticks = int(ctrl_period_ticks)
        if positions is not None:                          # sensor, controller, actuator, RRM
            for i, (x, y) in enumerate(positions):
                cfg.net.pos[i][0], cfg.net.pos[i][1] = float(x), float(y)
        if counter_interval is not None:                   # seconds between two counter ticks (sensor sample + plant substep)
            cfg.net.counter_interval = float(counter_interval)
        if x0 is not None:
            for i, v in enumerate(x0):
                cfg.x0[i] = float(v)
        if A is not None:                                  # the plant x <- A x + B u: 4x4 row-major, 4, and the input before
            for i, row in enumerate(A):                    # the first command arrives
                for j, v in enumerate(row):
                    cfg.A[i * 4 + j] = float(v)
        if B is not None:
            for i, v in enumerate(B):
                cfg.B[i] = float(v)
        if u0 is not None:
            cfg.u0 = float(u0)
        self.config = cfg
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_create(C.byref(cfg), C.byref(self._h)))
            n = self.num_envs
            self._obs = torch.empty(n, dtype=torch.int32, device=self.device)
            self._rew = torch.empty(n, dtype=torch.float32, device=self.device)
            self._angle = torch.empty(n, dtype=torch.float64, device=self.device)
            self._done = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._stepped = False
        if gains is not None:                              # (None: the handle never reads gains; its kernels have (1, 0, 0) folded in)
            self.set_gains(gains)
        if disturbance is not None:                        # (None: the plant is exact and the handle's kernels draw nothing)
            self.set_disturbance(disturbance)
        if loss is not None:                               # (None: no packet is erased and the handle's kernels draw nothing for it)
            self.set_loss(loss)

    def reset(self):
        """envs/inverted_pendulum.py:95-99: returns an observation, resets nothing."""
        import math
        if not self._stepped:                              # before the first step: the initial plant state
            self._obs.fill_(int(math.degrees(self.config.x0[2])))
        return self._obs

    def step(self, action):
        torch = self._torch
        self._stepped = True
        dev = action["device"].to(device=self.device, dtype=torch.int32).contiguous()
        dur = action["duration"].to(device=self.device, dtype=torch.int32).contiguous()
        assert dev.shape == (self.num_envs,) and dur.shape == (self.num_envs,)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_step(self._h, dev.data_ptr(), dur.data_ptr(), self._obs.data_ptr(), self._rew.data_ptr(),
                                           self._angle.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
        return self._obs, self._rew, self._done, {"Sensor angle": self._angle}

    # -- per-env initial states, reset, and K steps in one launch (gw_ctrl_set_initial / _reset / _rollout / _rollout_schedules) --
    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _mask(self, mask):
        """``mask`` as uint8[N] on the env's GPU (None: every env); returns the tensor, to be kept alive across the call."""
        torch = self._torch
        if mask is None:
            return None
        m = torch.as_tensor(mask).to(device=self.device)
        m = (m != 0).to(torch.uint8).contiguous()
        assert m.shape == (self.num_envs,)
        return m

    def _keys(self, key):
        """One 64-bit key per env -- numpy uint64[N], or an int64 tensor holding the bit patterns -- as a contiguous int64[N]
        tensor on the env's GPU, to be kept alive across the call."""
        import numpy as np
        torch = self._torch
        if isinstance(key, torch.Tensor):
            if key.dtype != torch.int64:
                raise ValueError("key as a tensor is int64[num_envs] holding the keys' bit patterns")
            kt = key.to(self.device)
        else:
            ka = np.asarray(key)
            if ka.dtype != np.uint64:
                raise ValueError("key is numpy uint64[num_envs] (or an int64 tensor holding the bit patterns)")
            kt = torch.from_numpy(np.ascontiguousarray(ka).view(np.int64)).to(self.device)
        if tuple(kt.shape) != (self.num_envs,):
            raise ValueError("key holds one key per env")
        return kt.contiguous()

    def set_initial_state(self, x0, u0=None, mask=None):
        """Give the masked envs (None: all) initial states of their own: ``x0`` f64[N][4] (a single state of 4 is broadcast),
        ``u0`` f64[N] or a number (None: keep).  Takes effect at the env's next reset -- ``reset_envs`` or the end of an
        episode inside ``rollout`` / ``rollout_schedules``; the running state is not touched."""
        torch = self._torch
        x = torch.as_tensor(x0, dtype=torch.float64).to(self.device)
        x = x.expand(self.num_envs, 4).contiguous() if x.dim() == 1 else x.contiguous()
        assert x.shape == (self.num_envs, 4)
        u = None
        if u0 is not None:
            u = torch.as_tensor(u0, dtype=torch.float64).to(self.device)
            u = u.expand(self.num_envs).contiguous()
        m = self._mask(mask)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_set_initial(self._h, x.data_ptr(), u.data_ptr() if u is not None else None,
                                                  m.data_ptr() if m is not None else None, self._stream()))

    def set_gains(self, gains, mask=None):
        """Give the masked envs (None: all) PID gains of their own: ``gains`` f64[N][3] = (kp, ki, kd), a tensor or an array, on
        the GPU or not (one set of 3 is broadcast; ``actions.make_ctrl_gains`` lays G sets across the envs).  At every control
        tick the controller computes ``e = |angle|``, ``pid = kp e + ki (e + last_error) + kd (e - last_error)``,
        ``last_error = e`` and, unless its angle is 0, commands ``pid`` against the angle's sign.  No running state is touched,
        ``last_error`` included; the gains survive every reset.  From the first call on the handle launches the kernels that
        read the gains; with (1, 0, 0) they compute what the default kernels compute."""
        torch = self._torch
        g = torch.as_tensor(gains, dtype=torch.float64).to(self.device)
        if tuple(g.shape) == (3,):
            g = g.expand(self.num_envs, 3)
        if tuple(g.shape) != (self.num_envs, 3):
            raise ValueError("gains must be (kp, ki, kd) or float64[num_envs][3]")
        g = g.contiguous()
        m = self._mask(mask)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_set_gains(self._h, g.data_ptr(), m.data_ptr() if m is not None else None, self._stream()))

    def set_disturbance(self, g, key=None, mask=None):
        """Disturb the plant of the masked envs (None: all): ``g`` f64[N][4], one weight per plant state (a single vector of 4
        is broadcast), and ``key``, one 64-bit noise key per env -- numpy uint64[N], or an int64 tensor holding the bit
        patterns; None: ``actions.make_ctrl_disturbance``'s default keys, a sequence of its own for every env.  From then on
        every plant substep of those envs ends with ``x[i] += g[i] * w``, ``w`` uniform on [-1, 1) and a function of the env's
        key and of the count of substeps since this call alone (``actions.ctrl_noise_numpy``): envs with equal keys face the
        same noise.  The count restarts here and nowhere else: a reset keeps g, key and count, so that every episode of an env
        meets fresh noise.  No other running state is touched.  From the first call on the handle launches the kernels that
        draw, which also read the gains; with ``g = 0`` they compute what the gains' kernels compute."""
        import numpy as np
        torch = self._torch
        gt = torch.as_tensor(g, dtype=torch.float64).to(self.device)
        if tuple(gt.shape) == (4,):
            gt = gt.expand(self.num_envs, 4)
        if tuple(gt.shape) != (self.num_envs, 4):
            raise ValueError("g must be 4 weights or float64[num_envs][4]")
        gt = gt.contiguous()
        if key is None:
            from .. import actions
            key = actions.make_ctrl_disturbance(np.zeros(4), self.num_envs)[1]
        kt = self._keys(key)
        m = self._mask(mask)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_set_disturbance(self._h, gt.data_ptr(), kt.data_ptr(), m.data_ptr() if m is not None else None,
                                                      self._stream()))

    def set_loss(self, p, key=None, mask=None):
        """Erase packets of the masked envs (None: all): ``p`` f64[N][4], one loss probability per link -- the RRM's announcement
        to the sensor, its announcement to the controller, sensor -> controller, controller -> actuator (4 values are
        broadcast) -- clipped to [0, 1] and converted by ``actions.ctrl_loss_threshold``; and ``key``, one 64-bit key per env
        as in ``set_disturbance`` (None: ``actions.make_ctrl_loss``'s default keys).  From then on every transmission of those
        envs takes one draw (``actions.ctrl_loss_numpy`` of the env's key and of the count of transmissions since this call),
        whatever the PHY decides about it.  An erased announcement is an ungranted step; an erased data packet leaves its queue,
        goes on the air and is not delivered.  ``get_state("lost")`` counts the erasures per link, ``"loss_count"`` the draws.
        The counts restart here and nowhere else: a reset keeps thresholds, key and counts.  No other running state is touched.
        From the first call on the handle launches the kernels that draw, which are the disturbance's kernels as well: with
        ``p = 0`` they compute what a handle that called ``set_disturbance`` computes (at ``g = 0`` if it never did)."""
        import numpy as np
        from .. import actions
        torch = self._torch
        pa = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        if pa.dtype.kind not in "fiu":
            raise ValueError("p holds loss probabilities (float64)")
        pa = pa.astype(np.float64)
        if pa.shape == (4,):
            pa = np.broadcast_to(pa, (self.num_envs, 4))
        if pa.shape != (self.num_envs, 4):
            raise ValueError("p must be 4 loss probabilities, one per link, or float64[num_envs][4]")
        thr = actions.ctrl_loss_threshold(pa)
        tt = torch.from_numpy(np.ascontiguousarray(thr).view(np.int32)).to(self.device).contiguous()
        if key is None:
            key = actions.make_ctrl_loss(np.zeros(4), self.num_envs)[1]
        kt = self._keys(key)
        m = self._mask(mask)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_set_loss(self._h, tt.data_ptr(), kt.data_ptr(), m.data_ptr() if m is not None else None,
                                               self._stream()))

    def reset_envs(self, mask=None):
        """Put the masked envs (None: all) back into the state a fresh env of their own initial state has -- clock, queues,
        noise states, counters, the episode record (``age``, ``cost``) and the controller's ``last_error`` 0; ``flags`` are
        sticky and stay, and so do the gains, the disturbance (weights, key and count) and the loss (thresholds, key and counts) -- and return the observations of all N envs.  (``reset()`` keeps the reference's meaning: it resets nothing.)"""
        torch = self._torch
        m = self._mask(mask)
        self._stepped = True                               # the observation buffer now holds what the GPU wrote
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_reset(self._h, m.data_ptr() if m is not None else None, self._obs.data_ptr(), self._stream()))
        return self._obs

    @staticmethod
    def _episodes(episodes):
        """``episodes``: None or the pair ``(max_steps, fail_deg)``, 0 = no limit."""
        if episodes is None:
            return None
        max_steps, fail_deg = episodes
        return nat.CtrlEpisodes(int(max_steps), 0, float(fail_deg))

    def rollout(self, device, duration, episodes=None, out=None):
        """K consecutive steps from pre-staged actions ``int32[K][N]`` in ONE launch, the env's state in registers in between.
        Without ``episodes`` the results equal K calls of ``step`` bit for bit and the third tensor is ``done`` (all False).
        With ``episodes`` (``(max_steps, fail_deg)``, 0 = no limit): after each step ``age += 1``, ``cost += |angle|``; an env
        whose age reaches ``max_steps`` (bit 0) or whose |angle| exceeds ``fail_deg`` (bit 1) has ended, the third tensor
        holds those bits, and the env is reset inside the launch as ``reset_envs`` would.  ``out``: ``(obs int32, reward
        float32, ended uint8, angle float64)``, each [K][N] on the env's GPU, written in place.
        Returns ``(obs, reward, done_or_ended, {"Sensor angle": angle})``."""
        torch = self._torch
        dev = torch.as_tensor(device).to(device=self.device, dtype=torch.int32).contiguous()
        dur = torch.as_tensor(duration).to(device=self.device, dtype=torch.int32).contiguous()
        K, n = dev.shape[0], self.num_envs
        assert dev.shape == (K, n) and dur.shape == dev.shape
        ep = self._episodes(episodes)
        if out is None:
            out = (torch.empty((K, n), dtype=torch.int32, device=self.device), torch.empty((K, n), dtype=torch.float32, device=self.device),
                   torch.zeros((K, n), dtype=torch.uint8, device=self.device), torch.empty((K, n), dtype=torch.float64, device=self.device))
        obs, rew, ended, ang = out
        for t, dt in zip(out, (torch.int32, torch.float32, torch.uint8, torch.float64)):
            assert t.shape == (K, n) and t.dtype == dt and t.is_contiguous() and t.device == dev.device
        if ep is None:
            ended.zero_()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_rollout(self._h, K, dev.data_ptr(), dur.data_ptr(), C.byref(ep) if ep is not None else None,
                                              obs.data_ptr(), rew.data_ptr(), ang.data_ptr(), ended.data_ptr(), self._stream()))
        return obs, rew, ended, {"Sensor angle": ang}

    def rollout_schedules(self, schedules, episodes, steps):
        """Evaluate P cyclic schedules (``actions.make_ctrl_schedules``: uint8[P][L][2]) for ``steps`` steps in one launch, env e
        under schedule ``e // (N / P)``, acting on entry ``age % L``; nothing is stored per step.  Returns ``(tally f64[N][4],
        sums f64[P][4])``: per env {episodes ended, of those by fail_deg, steps taken, sum of the costs of the ended
        episodes}, and their sums per schedule."""
        torch = self._torch
        sch = torch.as_tensor(schedules)
        if sch.dtype != torch.uint8 or sch.dim() != 3 or sch.shape[2] != 2:
            raise ValueError("schedules must be uint8[P][L][2] (actions.make_ctrl_schedules)")
        sch = sch.to(self.device).contiguous()
        P, L = int(sch.shape[0]), int(sch.shape[1])
        ep = self._episodes(episodes)
        tally = torch.zeros((self.num_envs, 4), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_rollout_schedules(self._h, int(steps), sch.data_ptr(), P, L,
                                                        C.byref(ep) if ep is not None else None, tally.data_ptr(), self._stream()))
        return tally, tally.view(P, self.num_envs // P, 4).sum(1)

    def rollout_feedback(self, sched, edges, episodes, steps, abs_key=True, record=False):
        """Evaluate P angle-feedback band schedulers (``actions.make_ctrl_feedback``: ``sched`` uint8[P][B][L][2], ``edges``
        int32[P][B - 1]) for ``steps`` steps in one launch, env e under policy ``e // (N / P)``.  Before each step the env's key
        is the int32 observation of its current state (``abs_key``: the absolute value of it), its bin the number of its
        policy's edges at or below the key, its action entry ``age % L`` of that bin's schedule; episodes as in ``rollout``
        (required).  Both tensors are read on the GPU when the launch runs.  Returns ``(tally f64[N][8], sums f64[P][8])``: per
        env {episodes ended, of those by fail_deg, steps taken, sum of the costs of the ended episodes, durations assigned,
        time elapsed, sum of |angle| dt, steps taken in bin 0} and their sums per policy -- a policy's time-weighted mean
        error is ``sums[p, 6] / sums[p, 5]``, its airtime per second ``sums[p, 4] / sums[p, 5]``.  ``record=True`` returns
        as a third value the dict of the six [steps][N] rows: ``device``, ``duration``, ``obs``, ``reward``, ``angle``,
        ``ended``."""
        torch = self._torch
        sch, edg = torch.as_tensor(sched), torch.as_tensor(edges)
        if sch.dtype != torch.uint8 or sch.dim() != 4 or sch.shape[3] != 2:
            raise ValueError("sched must be uint8[P][B][L][2] (actions.make_ctrl_feedback)")
        P, B, L = int(sch.shape[0]), int(sch.shape[1]), int(sch.shape[2])
        if edg.dtype != torch.int32 or tuple(edg.shape) != (P, B - 1):
            raise ValueError("edges must be int32[P][B - 1] (actions.make_ctrl_feedback)")
        sch, edg = sch.to(self.device).contiguous(), edg.to(self.device).contiguous()
        ep = self._episodes(episodes)
        K, n = int(steps), self.num_envs
        fb = nat.CtrlFeedback(P, B, L, nat.CTRL_FB_ABS if abs_key else 0, edg.data_ptr() if B > 1 else None, sch.data_ptr())
        tally = torch.zeros((n, nat.CTRL_FB_COLS), dtype=torch.float64, device=self.device)
        rows = out = None
        if record:
            dts = (("device", torch.int32), ("duration", torch.int32), ("obs", torch.int32), ("reward", torch.float32),
                   ("angle", torch.float64), ("ended", torch.uint8))
            out = {name: torch.empty((max(K, 0), n), dtype=dt, device=self.device) for name, dt in dts}
            if K > 0:                                      # (an empty tensor has no address to pass)
                rows = nat.CtrlFeedbackRows(*(out[name].data_ptr() for name, _ in dts))
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_ctrl_rollout_feedback(self._h, K, C.byref(fb), C.byref(ep) if ep is not None else None,
                                                       C.byref(rows) if rows is not None else None, tally.data_ptr(), self._stream()))
        sums = tally.view(P, n // P, nat.CTRL_FB_COLS).sum(1)
        return (tally, sums, out) if record else (tally, sums)

    _FIELDS = {"now": ((), "f8"), "wake": ((), "f8"), "u": ((), "f8"), "angle_deg": ((), "f8"), "x": ((4,), "f8"),
               "rx_power": ((4,), "f8"), "qlen": ((2,), "i4"), "received": ((2,), "u4"), "n_tx": ((), "u4"),
               "commands": ((), "u4"), "substeps": ((), "u4"), "flags": ((), "u4"),
               "age": ((), "u4"), "cost": ((), "f8"), "x_init": ((4,), "f8"), "u_init": ((), "f8"),
               "gains": ((3,), "f8"), "last_error": ((), "f8"),
               "disturbance": ((4,), "f8"), "noise_key": ((), "u8"), "noise_count": ((), "u8"),
               "loss": ((4,), "u4"), "loss_key": ((), "u8"), "loss_count": ((), "u8"), "lost": ((4,), "u4")}

    def get_state(self, field):
        import numpy as np
        shape, dt = self._FIELDS[field]
        out = np.empty((self.num_envs,) + shape, np.dtype(dt))
        nat.check(self._L.gw_ctrl_get_state(self._h, field.encode(), out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.gw_ctrl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
