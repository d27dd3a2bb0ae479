"""
Host-side mirror of gymwipe/envs/counter_traffic.py on top of the HIP C-ABI.

``VecCounterTrafficEnv``  N independent CounterTraffic environments resident in HBM on one
                          GPU, advanced together by one kernel launch per ``step``.
``CounterTrafficEnv``     the N = 1 drop-in with the reference's exact Python surface:
                          ``step({"device": int, "duration": int}) -> (int, float, bool, dict)``.

Reference behaviour kept on purpose:
  * ``reset()`` zeroes the counters and the interpreter only; simulated time, MAC queues
    and radio state persist (counter_traffic.py:135-144)
  * a fresh env starts with counters at 1, a reset env at 0 (:48 vs :140)
  * data payloads carry ``value == 2`` and ``byteSize == counter`` (swapped constructor
    arguments, :57), so observations are 65534 / 65536 / 65538 and ``done`` never fires
"""
import ctypes as C
import os
import weakref

import numpy as np

from .. import _native as nat
from .. import spaces
from .core import BaseEnv, Interpreter, VecInterpreter, VecPayload


def _torch():
    import torch
    return torch


class _DeviceInterpreter(Interpreter):
    """Facade over the interpreter state that lives on the GPU
    (CounterTrafficEnv.CounterTrafficInterpreter, counter_traffic.py:63-112)."""

    def __init__(self, env):
        self._env = env

    def reset(self):
        self._env.reset()

    def onPacketReceived(self, senderIndex, receiverIndex, payload):
        raise NotImplementedError("packets are interpreted inside the HIP step kernel")

    @property
    def receivedValues(self):
        rv = self._env.received()
        return rv[0].tolist() if self._env._scalar_api else rv

    def getObservation(self):
        return self._env._last[0]

    def getReward(self):
        return self._env._last[1]

    def getDone(self):
        return self._env._last[2]

    def getInfo(self):
        return self._env._info()


class StepOutputs:
    """Where one ``env.step(action, out=...)`` writes: ``obs`` int32[N], ``reward`` float32[N], ``done`` uint8[N] and, optionally,
    ``feedback_bytes`` uint8[N] (the step's feedback in the one-byte exchange format, ``gw_step_fb``), ``ended`` uint8[N]
    (``step_autoreset``'s cause per env: 0, 1 done, 2 step limit) and ``delivered`` int32[N] (``step_autoreset(score=)``'s
    packets per env) -- preallocated, contiguous tensors on the env's GPU.  Their device addresses are taken ONCE, here (a step is enqueued every few
    microseconds; four ``data_ptr()`` calls are 10 % of that), so the tensors must not be resized or re-pointed afterwards;
    the object keeps them alive."""
    __slots__ = ("obs", "reward", "done", "feedback_bytes", "ended", "delivered", "_ptrs", "_as_tuple", "_dev", "_ended_ptr",
                 "_delivered_ptr")

    def __init__(self, obs, reward, done, feedback_bytes=None, ended=None, delivered=None):
        torch = _torch()
        n = obs.shape[0]
        for t, dt in ((obs, torch.int32), (reward, torch.float32), (done, torch.uint8), (feedback_bytes, torch.uint8),
                      (ended, torch.uint8), (delivered, torch.int32)):
            if t is None:
                continue
            assert (type(t) is torch.Tensor and t.dtype is dt and t.dim() == 1 and t.shape[0] == n and t.is_contiguous()
                    and t.device == obs.device and t.is_cuda), "StepOutputs: contiguous 1-D tensors of one length on one GPU"
        self.obs, self.reward, self.done, self.feedback_bytes, self.ended = obs, reward, done, feedback_bytes, ended
        self._ended_ptr = ended.data_ptr() if ended is not None else 0     # (beside _ptrs: the native stepper reads four)
        self.delivered = delivered
        self._delivered_ptr = delivered.data_ptr() if delivered is not None else 0
        self._ptrs = (obs.data_ptr(), reward.data_ptr(), done.data_ptr(),
                      feedback_bytes.data_ptr() if feedback_bytes is not None else 0)
        self._as_tuple = (obs, reward, done)
        self._dev = obs.device.index or 0                 # step() refuses outputs that live on another GPU than the env


class VecCounterTrafficEnv(BaseEnv):
    """N CounterTraffic environments on one MI355X.

    Args:
        num_envs: N.
        num_devices: D assignable senders (reference: 2).  For D > 2 the senders sit on a
            circle of radius 2 m around the RRM with multiplicities 1,3,1,3,....
        device: torch device string or index ('cuda:0').
        positions / multiplicity / dest / rrm_position: optional overrides of the layout.
        per_env_stats: explicit-queue mode only -- keep per-env event counters (the default mode always
            keeps them in its 32-byte counter record).
        explicit_queue: hold the MAC queues as explicit rings of packet sizes (generic, slower)
            instead of the default exact suffix encoding of counter traffic (gw_queue.h).
        reuse_outputs: return the same output tensors every step (fast path).
        extra_attenuation: custom attenuation models per device pair (the reference's
            AttenuationModelFactory.setCustomModels / JoinedAttenuationModel, physical.py:402-498), reduced to what they
            amount to with static geometry: ``{(a, b): dB}`` added to the free-space term of the pair (radio index
            ``num_devices`` is the RRM), or a callable ``(a, b, pos_a, pos_b) -> dB`` evaluated for every pair.
        per_env_geometry: positions per ENVIRONMENT (default queue mode): every env starts with the layout above and
            ``set_position`` / ``set_positions`` move radios between steps (the reference's ``Position.set``,
            devices/core.py:52-86); link powers are then kept per env and rebuilt on the GPU.
        counter_traffic / peer_receive / float_duration (explicit_queue only): switch the
            counter processes off so that packets come from enqueue() only; keep every sender MAC in receive
            mode (get_state("peer_received") counts what it hands up); pass assignment durations as floats
            like tests/networking/test_stack.py:197 does.
    """
    COUNTER_INTERVAL = 0.001                              # counter_traffic.py:31
    COUNTER_BYTE_LENGTH = 2                               # :33
    COUNTER_BOUND = 2 ** (8 * COUNTER_BYTE_LENGTH)        # :35

    _scalar_api = False

    def __init__(self, num_envs, num_devices=2, device="cuda:0", positions=None,
                 multiplicity=None, dest=None, rrm_position=None, per_env_stats=False,
                 reuse_outputs=True, explicit_queue=False, counter_bound=None, interpreter=None,
                 counter_traffic=True, peer_receive=False, float_duration=False, extra_attenuation=None,
                 start_time=None, per_env_geometry=False, counter_interval=None, duration_factor=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("gymwipe_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self._L = nat.lib()
        self.num_envs = int(num_envs)
        self.num_devices = int(num_devices)
        self.device = torch.device(device)
        BaseEnv.__init__(self, self.num_devices)
        self.observation_space = spaces.Discrete(2 * self.COUNTER_BOUND)   # :120

        cfg = nat.default_config(self.num_envs, self.num_devices)
        cfg.hip_device = self.device.index or 0
        D = self.num_devices
        if positions is not None:
            assert len(positions) == D
            for i, (x, y) in enumerate(positions):
                cfg.pos[i][0], cfg.pos[i][1] = float(x), float(y)
        if rrm_position is not None:
            cfg.pos[D][0], cfg.pos[D][1] = float(rrm_position[0]), float(rrm_position[1])
        if multiplicity is not None:
            assert len(multiplicity) == D
            for i, m in enumerate(multiplicity):
                cfg.mult[i] = int(m)
        if dest is not None:
            assert len(dest) == D
            for i, m in enumerate(dest):
                cfg.dest[i] = int(m)
        if extra_attenuation is not None:
            if callable(extra_attenuation):
                pos = [(cfg.pos[i][0], cfg.pos[i][1]) for i in range(D + 1)]
                extra_attenuation = {(a, b): extra_attenuation(a, b, pos[a], pos[b])
                                     for a in range(D + 1) for b in range(a + 1, D + 1)}
            for (a, b), db in extra_attenuation.items():
                cfg.extra_att_db[a][b] = cfg.extra_att_db[b][a] = float(db)
        if start_time is not None:             # test hook: simulated time at creation (the reference starts at 0)
            cfg.start_time = float(start_time)
        if per_env_stats:
            cfg.flags |= nat.CFG_PER_ENV_STATS
        if explicit_queue:
            cfg.flags |= nat.CFG_EXPLICIT_QUEUE
        if not counter_traffic:
            cfg.flags |= nat.CFG_NO_COUNTER_TRAFFIC
        if peer_receive:
            cfg.flags |= nat.CFG_PEER_RECEIVE
        if float_duration:
            cfg.flags |= nat.CFG_FLOAT_DURATION
        if per_env_geometry:
            cfg.flags |= nat.CFG_PER_ENV_GEOMETRY
        if counter_interval is not None:       # COUNTER_INTERVAL (counter_traffic.py:31)
            cfg.counter_interval = float(counter_interval)
        if duration_factor is not None:        # ASSIGNMENT_DURATION_FACTOR (envs/core.py:27)
            cfg.duration_factor = int(duration_factor)
            self.ASSIGNMENT_DURATION_FACTOR = int(duration_factor)
        if counter_bound is not None:          # tests: reach counter saturation quickly
            cfg.counter_bound = int(counter_bound)
            self.COUNTER_BOUND = int(counter_bound)
            self.observation_space = spaces.Discrete(2 * self.COUNTER_BOUND)
        self.config = cfg

        self._h = C.c_void_p()
        self._hv = 0
        self._fb = None
        self._fast = nat.fast()
        self._cuda_get_device = torch._C._cuda_getDevice
        self._cuda_raw_stream = torch._C._cuda_getCurrentRawStream
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_create(C.byref(cfg), C.byref(self._h)))
            self._hv = self._h.value or 0
            n = self.num_envs
            self._obs = torch.empty(n, dtype=torch.int32, device=self.device)
            self._rew = torch.empty(n, dtype=torch.float32, device=self.device)
            self._done = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._reuse = bool(reuse_outputs)
        self._seen = {}                                   # action tensor objects already validated (step())
        self._dev_index = self.device.index or 0
        self._last = (None, None, None)
        self._scored_records = None                       # _autoreset(score=): the last gw_episodes / gw_score records passed
        self._stats_last = None                           # rollout_policy_stats: the last observations, and the fallback's
        self._stats_buf = None                            # 64-step transition buffers (both allocated on first use)
        self._ep_state = self._ep_tally = self._ep_next = None   # rollout_episodes: {age, ret}[N], the episode tally, the
        self._ep_buf = None                               # observations acted on next; the fallback's ended rows (first use)
        self._packets_buf = None                          # ... and, with packets=True, its delivered rows (first use)
        self._ctl_node = None                             # rollout_controller: each env's node (first use)
        self._custom = interpreter
        if interpreter is not None:                       # a user-supplied Interpreter replaces the fused one
            if explicit_queue:
                raise ValueError("custom interpreters need the default queue mode")
            self._dest = torch.tensor([int(cfg.dest[i]) for i in range(D)], dtype=torch.int64, device=self.device)
            self._deliv = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._deliv_prev = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self.interpreter = interpreter
        else:
            self.interpreter = _DeviceInterpreter(self)
        # env.step(action, out) as ONE native call (csrc/gw_pyfast.c: Stepper), installed over the method below as an instance
        # attribute -- where the method's flat fast path applies at all (the shim is there, the built-in interpreter) and nothing
        # overrides what it would skip (a subclass's step() or _info()).  Every other case is handed on to the method.
        self._fast_native = self._fast is not None and not os.environ.get("GW_NO_FASTSTEP")   # (reset()'s short route too)
        if (self._fast_native and interpreter is None
                and type(self).step is VecCounterTrafficEnv.step and type(self)._info is VecCounterTrafficEnv._info):
            self.step = self._fast.Stepper(self._hv, self._dev_index, self._seen, self._cuda_get_device, self._cuda_raw_stream,
                                           self, self._step_py, nat.check, StepOutputs)

    # -- helpers ------------------------------------------------------------------------------
    def _stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    def _as_i32(self, x, name):
        torch = _torch()
        if isinstance(x, torch.Tensor):
            t = x
        else:
            t = torch.as_tensor(np.asarray(x))
        if t.dim() == 0:
            t = t.reshape(1)
        if t.shape != (self.num_envs,):
            raise AssertionError("action[%r] must have shape (%d,), got %s"
                                 % (name, self.num_envs, tuple(t.shape)))
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def _outputs(self):
        if self._reuse:
            return self._obs, self._rew, self._done
        torch = _torch()
        n = self.num_envs
        return (torch.empty(n, dtype=torch.int32, device=self.device),
                torch.empty(n, dtype=torch.float32, device=self.device),
                torch.empty(n, dtype=torch.uint8, device=self.device))

    def _info(self):
        return {}

    # -- gym surface ----------------------------------------------------------------------------
    def reset(self, mask=None):
        """Mirror of CounterTrafficEnv.reset (counter_traffic.py:135-144) for every env, or for
        the envs selected by ``mask`` (bool/uint8 [N])."""
        torch = _torch()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            assert m.shape == (self.num_envs,)
        obs = self._outputs()[0]
        idx = self._dev_index
        if self._fast_native and self._cuda_get_device() == idx:   # the one-process-per-GPU case, as in step(): no context
            rc = self._fast.reset(self._hv, m.data_ptr() if m is not None else 0, obs.data_ptr(), self._cuda_raw_stream(idx))
            if rc:                                                  # manager, no Stream object, no ctypes conversion
                nat.check(rc)
        else:
            with torch.cuda.device(self.device):
                nat.check(self._L.gw_reset(self._h, m.data_ptr() if m is not None else None,
                                           obs.data_ptr(), self._stream()))
        if self._custom is not None:                      # counter_traffic.py:142-144
            self._custom.reset()
            return self._custom.getObservation()
        if self._ep_state is not None:                    # rollout_episodes' {age, ret}: a reset env starts a new episode
            if m is None:
                self._ep_state.zero_()
            else:
                self._ep_state.masked_fill_(m.bool().unsqueeze(1), 0)
        if self._ctl_node is not None:                    # rollout_controller's nodes: a reset env starts at node 0
            if m is None:
                self._ctl_node.zero_()
            else:
                self._ctl_node.masked_fill_(m.bool(), 0)
        self._last = (obs,) + tuple(self._last[1:])       # the observation the agent acts on next (rollout_policy)
        return obs

    def _ready(self, t):
        """int32, contiguous, right shape, on this env's GPU: usable in place."""
        torch = _torch()
        return (type(t) is torch.Tensor and t.dtype is torch.int32 and t.device == self.device
                and t.dim() == 1 and t.shape[0] == self.num_envs and t.is_contiguous())

    def _checked(self, t, name):
        """The action tensor, validated (int32, contiguous, right shape, on this env's GPU) or converted.  A tensor OBJECT
        that passed once is not re-validated (a caller steps with the same pre-staged tensors again and again; dtype, device
        and shape of a tensor object do not change under ordinary use): one dict probe instead of seven attribute tests."""
        hit = self._seen.get(id(t))
        if hit is not None and hit[0]() is t:
            return t
        if not self._ready(t):
            return self._as_i32(t, name)
        if len(self._seen) >= 8192:
            self._seen.clear()
        # weak: the env must not keep a caller's action buffers alive; the device address is taken once, with the validation
        self._seen[id(t)] = (weakref.ref(t), t.data_ptr())
        return t

    def _step_py(self, action, out=None):
        """One env.step() for all N envs: ``action = {"device": int32[N], "duration": int32[N]}``
        (torch tensors on the env's GPU are used in place).  Returns
        ``(obs int32[N], reward float32[N], done uint8[N], info)``; an action outside the action
        space flags its env (``check()`` raises) and leaves that env untouched.
        ``out``: a ``StepOutputs`` to write this step's outputs into (instead of the env's own buffers).

        Aliasing contract of the fast path: an action tensor OBJECT that passed validation once, and the tensors inside a
        ``StepOutputs``, are taken at their word afterwards -- their device addresses, dtype, shape and device must not be
        changed behind the env's back (``set_()``, ``resize_()``, swapping ``.data``); writing new VALUES into them is what
        they are for.  A ``StepOutputs`` on another GPU than the env is refused.

        Where the CPython shim is built, an env with the built-in interpreter carries ``step`` as an instance attribute: a
        native callable (``_gw_fast.Stepper``) that does the common case below -- cached action tensors, a ``StepOutputs``,
        the caller on this env's device -- itself and hands every other call to this method."""
        # (this method is enqueued ~200 000 times a second: the common path -- pre-staged int32 tensors on this GPU, reused
        #  output buffers, the caller on this env's device -- is written out flat, without helper calls)
        dev = action["device"]
        dur = action["duration"]
        seen = self._seen
        hit = seen.get(id(dev))
        if hit is None or hit[0]() is not dev:
            dev = self._checked(dev, "device")
            dev_ptr = dev.data_ptr()
        else:
            dev_ptr = hit[1]
        hit = seen.get(id(dur))
        if hit is None or hit[0]() is not dur:
            dur = self._checked(dur, "duration")
            dur_ptr = dur.data_ptr()
        else:
            dur_ptr = hit[1]
        idx = self._dev_index
        if out is not None and out._dev != idx:
            raise ValueError("StepOutputs on cuda:%d passed to an env on cuda:%d" % (out._dev, idx))
        if out is not None and self._cuda_get_device() == idx and self._fast is not None and self._custom is None:
            p = out._ptrs                                       # preallocated outputs, addresses taken at construction
            if p[3]:
                rc = self._fast.step_fb(self._hv, dev_ptr, dur_ptr, p[0], p[1], p[2], p[3], self._cuda_raw_stream(idx))
            else:
                rc = self._fast.step(self._hv, dev_ptr, dur_ptr, p[0], p[1], p[2], self._cuda_raw_stream(idx))
            if rc:
                nat.check(rc)
            self._last = out._as_tuple
            return out.obs, out.reward, out.done, self._info()
        if out is not None:                                     # (no shim / another device current / custom interpreter: the general path)
            obs, rew, done, fb = out.obs, out.reward, out.done, out.feedback_bytes
        else:
            fb = self._fb                                       # feedback_bytes_into(): the step's one-byte feedback row
            if self._reuse:
                obs, rew, done = self._obs, self._rew, self._done
            else:
                obs, rew, done = self._outputs()
        if self._cuda_get_device() == idx:                     # the one-process-per-GPU case: no context switch
            fast = self._fast                                   # CPython fast-call shim (csrc/gw_pyfast.c) when built
            if fb is not None:
                rc = (fast.step_fb if fast is not None else self._L.gw_step_fb)(
                    self._hv, dev_ptr, dur_ptr, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), fb.data_ptr(),
                    self._cuda_raw_stream(idx))
            elif fast is not None:
                rc = fast.step(self._hv, dev_ptr, dur_ptr, obs.data_ptr(), rew.data_ptr(),
                               done.data_ptr(), self._cuda_raw_stream(idx))
            else:
                rc = self._L.gw_step(self._h, dev_ptr, dur_ptr, obs.data_ptr(), rew.data_ptr(),
                                     done.data_ptr(), self._cuda_raw_stream(idx))
        else:
            torch = _torch()
            with torch.cuda.device(self.device):
                rc = self._L.gw_step_fb(self._h, dev_ptr, dur_ptr, obs.data_ptr(), rew.data_ptr(),
                                        done.data_ptr(), fb.data_ptr() if fb is not None else None, self._stream())
        if rc:
            nat.check(rc)
        if self._custom is not None:
            return self._feed_custom(dev, dur)
        self._last = (obs, rew, done)
        return obs, rew, done, self._info()

    step = _step_py

    def feedback_bytes_into(self, row):
        """From now on every step() also writes its feedback in the one-byte exchange format of ``pack_feedback`` into
        ``row`` (uint8[N] on this env's GPU; ``None`` switches it off) -- the row a multi-GPU job gathers
        (``sharding.ChunkedFeedbackGather``).  In the default mode the step kernel stores the byte itself: no packing launch."""
        if row is not None:
            torch = _torch()
            assert (type(row) is torch.Tensor and row.dtype is torch.uint8 and row.device == self.device and row.dim() == 1
                    and row.shape[0] == self.num_envs and row.is_contiguous()), "feedback row: contiguous uint8[N] on the env's GPU"
        self._fb = row

    def _feed_custom(self, dev, dur):
        """Drive a user-supplied VecInterpreter from what the RRM sniffed in this step."""
        torch = _torch()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_delivered(self._h, self._deliv.data_ptr(), self._stream()))
        count = self._deliv - self._deliv_prev
        self._deliv_prev.copy_(self._deliv)
        it = self._custom
        it.onFrequencyBandAssignment(dur * self.ASSIGNMENT_DURATION_FACTOR, dev)    # swapped, networking/devices.py:200
        it.onPacketReceived(dev, self._dest[dev.long()].to(torch.int32), VecPayload(self.config.payload_value, count))
        self._last = it.getFeedback()
        return self._last

    def rollout(self, device, duration, out=None):
        """K consecutive steps from pre-staged actions ``int32[K][N]``; one launch per step, no
        Python in between.  Returns ``(obs[K][N], reward[K][N], done[K][N])``."""
        torch = _torch()
        dev = torch.as_tensor(device).to(device=self.device, dtype=torch.int32).contiguous()
        dur = torch.as_tensor(duration).to(device=self.device, dtype=torch.int32).contiguous()
        K = dev.shape[0]
        assert dev.shape == (K, self.num_envs) and dur.shape == dev.shape
        if out is None:
            out = self._rows(K, (torch.int32, torch.float32, torch.uint8), None)
        obs, rew, done = out
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout(self._h, K, dev.data_ptr(), dur.data_ptr(), obs.data_ptr(),
                                         rew.data_ptr(), done.data_ptr(), self._stream()))
        if K:
            self._last = (obs[-1], rew[-1], done[-1])
        return obs, rew, done

    def _policy_table(self, cdf, population=False):
        """``cdf`` as the 32-bit words gw_rollout_policy reads: [3][A] on this env's GPU (a tensor that already is, is used in
        place, so a caller may keep rewriting it on the same stream).  ``population``: [P][3][A], any P >= 1."""
        torch = _torch()
        A = self.num_devices * int(self.config.max_duration)
        if isinstance(cdf, torch.Tensor):
            t = cdf
            if t.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)):
                t = t.to(self.device).contiguous()
            else:                                         # actions.policy_cdf's int64: keep the low 32 bits, bit for bit
                t = (t.to(self.device).to(torch.int64) & 0xffffffff)
                t = torch.where(t >= (1 << 31), t - (1 << 32), t).to(torch.int32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(cdf, dtype=np.uint32).view(np.int32)).to(self.device)
        if population:
            if t.dim() != 3 or t.shape[0] < 1 or tuple(t.shape[1:]) != (3, A):
                raise ValueError("policy tables must have shape (P, 3, %d), got %s" % (A, tuple(t.shape)))
        elif tuple(t.shape) != (3, A):
            raise ValueError("policy table must have shape (3, %d), got %s" % (A, tuple(t.shape)))
        return t

    # -- what the closed-loop calls share ------------------------------------------------------------
    def _obs_prev(self, obs_prev, who):
        """The checked ``obs_prev`` int32[N] on this env's GPU (default: what the env returned last)."""
        if obs_prev is None:
            obs_prev = self._last[0]
            if obs_prev is None:
                raise ValueError("%s: no observation yet -- reset() or step() first, or pass obs_prev" % who)
        n = self.num_envs
        prev = _torch().as_tensor(obs_prev).to(device=self.device, dtype=_torch().int32).contiguous()
        if prev.shape != (n,):
            raise ValueError("obs_prev must have shape (%d,), got %s" % (n, tuple(prev.shape)))
        return prev

    def _rows(self, K, kinds, out):
        """A call's ``[K][N]`` outputs, one per dtype of ``kinds``: the caller's ``out``, checked, or new tensors."""
        n = self.num_envs
        if out is None:
            out = tuple(_torch().empty((K, n), dtype=dt, device=self.device) for dt in kinds)
        for t, dt in zip(out, kinds):
            assert t.dtype is dt and tuple(t.shape) == (K, n) and t.is_contiguous() and t.device == self.device
        return tuple(out)

    @staticmethod
    def _apart(prev, out):
        """``prev``, or a copy of it where it lies inside one of the tensors ``out`` (the native calls want them apart)."""
        lo, hi = prev.data_ptr(), prev.data_ptr() + prev.numel() * prev.element_size()
        if any(lo < t.data_ptr() + t.numel() * t.element_size() and t.data_ptr() < hi for t in out):
            return prev.clone()
        return prev

    @staticmethod
    def _stream_id(seed, step0, env_id0):
        """The action stream's identity as the three 64-bit words of the C-ABI."""
        return int(seed) & (2 ** 64 - 1), int(step0) & (2 ** 64 - 1), int(env_id0) & (2 ** 64 - 1)

    def _compose_stats(self, K, table, seen, episodic, record, packets=False):
        """A tallying call on a handle without its fused form, composed from the two other calls in chunks of at most 64 steps
        into buffers the env keeps: ``record(s, k, out)`` runs steps ``s .. s + k`` from the observations ``seen`` into the
        rows ``out`` and returns what each env acts on next; ``transition_stats`` adds the rows into ``table``.  ``packets``
        (episodic only): ``out`` has a seventh row, the packets per step, which goes into the table's eighth column."""
        torch = _torch()
        n = self.num_envs
        if self._stats_buf is None:
            self._stats_buf = tuple(torch.empty((64, n), dtype=t, device=self.device)
                                    for t in (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8))
        bufs = self._stats_buf
        if episodic:
            if self._ep_buf is None:
                self._ep_buf = torch.empty((64, n), dtype=torch.uint8, device=self.device)
            bufs = bufs + (self._ep_buf,)
        if packets:
            if self._packets_buf is None:
                self._packets_buf = torch.empty((64, n), dtype=torch.int32, device=self.device)
            bufs = bufs + (self._packets_buf,)
        for s in range(0, K, 64):
            k = min(64, K - s)
            out = tuple(b[:k] for b in bufs)
            nxt = record(s, k, out)
            self.transition_stats(seen, *out[:5], table=table, ended=out[5] if episodic else None,
                                  delivered=out[6] if packets else None)
            seen.copy_(nxt)

    def rollout_policy(self, cdf, steps, seed, step0=0, env_id0=0, obs_prev=None, out=None):
        """``steps`` consecutive steps with the policy inside the launch (gw_rollout_policy): every env draws its action from
        row ``sign(obs - COUNTER_BOUND) + 1`` of ``cdf`` (``actions.policy_cdf``, [3][num_devices * max_duration]) for the
        observation it got last -- ``obs_prev`` int32[N] before the first step (default: what the env returned last), its own
        afterwards -- with the counter-based stream of ``actions.policy_sample_numpy`` at ``(seed, env_id0 + e, step0 + k)``.
        Returns ``(device, duration, obs, reward, done)``, each ``[steps][N]``: the transitions a replay memory wants; the two
        action arrays can be replayed through ``rollout``.  Advance ``step0`` by ``steps`` from call to call.  Not for
        hipGraph capture: ``step0`` would be baked in and every replay would repeat the same draws.
        The native call wants ``obs_prev`` apart from its outputs.  With the same ``out`` buffers call after call the default
        ``obs_prev`` is the last row of ``out``'s own ``obs``; an ``obs_prev`` inside any of ``out`` is copied first."""
        torch = _torch()
        if self._custom is not None:
            raise ValueError("rollout_policy needs the built-in interpreter: a custom interpreter's observations are not "
                             "the ones the kernel draws from")
        K = int(steps)
        prev = self._obs_prev(obs_prev, "rollout_policy")
        table = self._policy_table(cdf)
        out = self._rows(K, (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8), out)
        dev, dur, obs, rew, done = out
        if K:
            prev = self._apart(prev, out)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout_policy(self._h, K, table.data_ptr(), *self._stream_id(seed, step0, env_id0), prev.data_ptr(),
                                                *[t.data_ptr() for t in out], self._stream()))
        if K:
            self._last = (obs[-1], rew[-1], done[-1])
        return dev, dur, obs, rew, done

    def _stats_table(self, table, packets=False):
        """The ``int64[3][A][TS_COLS]`` table on this env's GPU (``packets``: ``[3][A][TSD_COLS]``): the caller's (added into) or
        a new one of zeros."""
        torch = _torch()
        from ..actions import TS_COLS, TSD_COLS
        shape = (3, self.num_devices * int(self.config.max_duration), TSD_COLS if packets else TS_COLS)
        if table is None:
            return torch.zeros(shape, dtype=torch.int64, device=self.device)
        if not (type(table) is torch.Tensor and table.dtype is torch.int64 and table.device == self.device
                and tuple(table.shape) == shape and table.is_contiguous()):
            raise ValueError("table must be a contiguous int64 tensor of shape %s on %s" % (shape, self.device))
        return table

    def transition_stats(self, obs_prev, device, duration, obs, reward, done, table=None, ended=None, delivered=None):
        """Recorded transitions ``[steps][N]`` (what ``rollout_policy`` returns; ``obs_prev`` int32[N] is what step 0 acted on)
        added into ``table`` (gw_transition_stats; ``actions.transition_stats_numpy`` restates it): ``int64[3][A][7]`` over
        (observation class, flat action).  Returns the table (a new one of zeros when none is passed).
        ``ended`` (uint8[steps][N], what ``rollout_episodes`` returns; gw_transition_stats_ep): an env whose step k - 1 ended
        an episode acted on the reset's observation at step k.
        ``delivered`` (int32[steps][N], what the scored calls return -- ``rollout_episodes(score=)``, ``rollout_autoreset(score=)``
        with its ``ended``; gw_transition_stats_delivered): the table is ``int64[3][A][8]``, its eighth column the packets
        delivered, each step's count clamped to [0, 65 535]; ``actions.table_score`` turns it into any score's sum per bin."""
        torch = _torch()
        table = self._stats_table(table, packets=delivered is not None)
        K, n = int(obs.shape[0]), self.num_envs
        args = []
        rows = [(obs_prev, torch.int32), (device, torch.int32), (duration, torch.int32), (obs, torch.int32),
                (reward, torch.float32), (done, torch.uint8)] + ([(ended, torch.uint8)] if ended is not None else [])
        if delivered is not None:
            rows.append((delivered, torch.int32))
        for t, dt in rows:
            t = torch.as_tensor(t).to(device=self.device, dtype=dt).contiguous()
            if tuple(t.shape) != ((n,) if not args else (K, n)):
                raise ValueError("transition_stats: obs_prev is [N], the other arrays [steps][N]; got %s" % (tuple(t.shape),))
            args.append(t)
        ptrs = [t.data_ptr() for t in args]
        with torch.cuda.device(self.device):
            if delivered is not None:
                if ended is None:
                    ptrs.insert(6, None)
                nat.check(self._L.gw_transition_stats_delivered(self._h, K, *ptrs, table.data_ptr(), self._stream()))
            else:
                call = self._L.gw_transition_stats if ended is None else self._L.gw_transition_stats_ep
                nat.check(call(self._h, K, *ptrs, table.data_ptr(), self._stream()))
        return table

    def rollout_policy_stats(self, cdf, steps, seed, step0=0, env_id0=0, obs_prev=None, table=None, returns=None, packets=False):
        """``rollout_policy`` for a caller that wants the tally, not the transitions (gw_rollout_policy_stats): the same
        ``steps`` steps, draws and state changes, and every transition ADDED into ``table`` -- ``int64[3][A][7]`` over
        (observation class ``sign(obs_seen - COUNTER_BOUND) + 1``, flat action ``device * max_duration + duration``) with the
        columns n, reward sum, reward-square sum, next observation below / at / above the bound, done.  Returns the table (a
        new one of zeros when none is passed).  ``returns`` (int32[N], optional) gets each env's reward sum added.  The last
        observation is kept as ``reset()`` keeps its own, so a following ``rollout_policy`` / ``rollout_policy_stats``
        continues from it; advance ``step0`` by ``steps``.  Nothing here is sized by ``steps * N``.
        A handle without the fused form (explicit queues, live PHY, ...) runs ``rollout_policy`` in chunks of at most 64 steps
        into buffers the env keeps, then ``transition_stats``: the same table.
        ``packets=True`` (gw_rollout_policy_stats_delivered): the table is ``int64[3][A][8]``, its eighth column the data
        packets of the assigned sender the RRM decoded, summed per bin (``actions.table_score`` applies a score to it).  Only
        the fused form has it: ``rollout_policy`` keeps no record of packets to compose the table from, so a handle without
        the fused form raises ``GW_EUNSUPPORTED`` (use ``rollout_episodes_stats(packets=True)``, whose fallback records them)."""
        torch = _torch()
        if self._custom is not None:
            raise ValueError("rollout_policy_stats needs the built-in interpreter")
        K, n = int(steps), self.num_envs
        prev = self._obs_prev(obs_prev, "rollout_policy_stats")
        cdf_t = self._policy_table(cdf)
        table = self._stats_table(table, packets)
        if returns is not None and not (type(returns) is torch.Tensor and returns.dtype is torch.int32 and returns.device == self.device
                                        and tuple(returns.shape) == (n,) and returns.is_contiguous()):
            raise ValueError("returns must be a contiguous int32[N] tensor on the env's GPU")
        if K == 0:
            return table
        last = self._stats_last
        if last is None:
            last = self._stats_last = torch.empty(n, dtype=torch.int32, device=self.device)
        seed, step0, env_id0 = self._stream_id(seed, step0, env_id0)
        call = self._L.gw_rollout_policy_stats_delivered if packets else self._L.gw_rollout_policy_stats
        with torch.cuda.device(self.device):
            rc = call(self._h, K, cdf_t.data_ptr(), seed, step0, env_id0, prev.data_ptr(), last.data_ptr(),
                      returns.data_ptr() if returns is not None else None, table.data_ptr(), self._stream())
        if rc == nat.EUNSUPPORTED and not packets and not os.environ.get("GW_ROLLOUT_STRICT"):
            def record(s, k, out):                         # refused before anything ran: compose it from the two other calls
                self.rollout_policy(cdf_t, k, seed, step0=step0 + s, env_id0=env_id0, obs_prev=last, out=out)
                if returns is not None:
                    returns.add_(out[3].sum(dim=0).to(torch.int32))
                return out[2][k - 1]
            last.copy_(prev)
            self._compose_stats(K, table, last, False, record)
        else:
            nat.check(rc)
        self._last = (last,) + tuple(self._last[1:])
        return table

    # -- episodes inside the closed loop (gw_rollout_episodes) -----------------------------------------
    def _episode_tensors(self):
        if self._ep_state is None:                        # (first use: an env that never runs episodes pays nothing in reset())
            torch = _torch()
            from ..actions import EP_COLS
            self._ep_state = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
            self._ep_tally = torch.zeros(EP_COLS, dtype=torch.int64, device=self.device)
            self._ep_next = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)

    @property
    def episode_state(self):
        """int32[N][2] on the GPU: each env's ``{age, ret}`` -- steps and reward sum since its last reset -- as
        ``rollout_episodes`` keeps them; ``reset()`` zeroes the envs it resets."""
        self._episode_tensors()
        return self._ep_state

    @property
    def episode_tally(self):
        """int64[5] on the GPU, added into by ``rollout_episodes`` / ``rollout_episodes_stats``: episodes ended, of those by
        done, sum of lengths, sum of returns, sum of squared returns (``episode_stats()``); the caller may zero it."""
        self._episode_tensors()
        return self._ep_tally

    def _episodes(self, max_steps, on_done, obs_prev, who, needs_obs=True):
        """What the episodic calls share: the env's own ``{age, ret}`` / tally / next-observation tensors (first use), the
        gw_episodes record and the checked ``obs_prev`` -- ``None`` for a caller that brings the actions (``needs_obs``
        false: nothing in the call reads an observation)."""
        if self._custom is not None:
            raise ValueError("%s needs the built-in interpreter" % who)
        if int(max_steps) < 0:
            raise ValueError("%s: max_steps must be >= 0" % who)
        self._episode_tensors()
        ep = nat.Episodes(int(max_steps), 1 if on_done else 0, self._ep_state.data_ptr(), self._ep_tally.data_ptr())
        return ep, (self._obs_prev(obs_prev, who) if needs_obs else None)

    def _score(self, score):
        """``actions.make_score``'s image as the gw_score record the scored calls read (by value, before they return)."""
        w = np.asarray(score)
        if w.shape != (1 + nat.MAX_DEVICES,) or w.dtype.kind not in "iu":
            raise ValueError("score must be actions.make_score()'s int32[%d]" % (1 + nat.MAX_DEVICES))
        if (np.abs(w.astype(np.int64)) > nat.SCORE_W_MAX).any():
            raise ValueError("score: a weight lies outside [-%d, %d]" % (nat.SCORE_W_MAX, nat.SCORE_W_MAX))
        return nat.Score.from_buffer_copy(np.ascontiguousarray(w, dtype=np.int32).tobytes())

    def rollout_episodes(self, cdf, steps, seed, max_steps=0, on_done=True, step0=0, env_id0=0, obs_prev=None, out=None, score=None):
        """``rollout_policy`` with episodes (gw_rollout_episodes): an env whose step returned ``done`` (``on_done``), or whose
        episode has reached ``max_steps`` steps (0: no limit), is reset inside the launch exactly as ``reset(mask)`` would reset
        it between two steps, and draws its next action from the reset's observation.  Returns ``(device, duration, obs,
        reward, done, ended)``, each ``[steps][N]``: row k is what step k returned (``obs[k]`` the terminal observation where
        ``ended[k]`` is 1 = done or 2 = step limit).  The env keeps each env's ``{age, ret}`` since its last reset, adds every
        ended episode into its tally (``episode_stats()``) and remembers the observation each env acts on next, so calls
        continue one another; advance ``step0`` by ``steps``.  The draws are ``rollout_policy``'s: resets do not shift the
        stream.  ``out``: six ``[steps][N]`` tensors to write into.  Not for hipGraph capture (``step0`` would be baked in).
        ``score`` (``actions.make_score``; gw_rollout_episodes_scored): ``reward``, each env's ``ret`` and the tally's return
        columns carry the step's score -- ``score[0] * reward + score[1 + device] * delivered`` -- and a seventh output,
        ``delivered`` int32[steps][N], the data packets of the assigned sender the RRM decoded in the step (``out``: seven
        tensors).  Everything else is as without; ``None`` is the call above, unchanged."""
        torch = _torch()
        ep, prev = self._episodes(max_steps, on_done, obs_prev, "rollout_episodes")
        K = int(steps)
        table = self._policy_table(cdf)
        kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8)
        out = self._rows(K, kinds + ((torch.int32,) if score is not None else ()), out)
        if K:
            prev = self._apart(prev, out)
        with torch.cuda.device(self.device):
            if score is not None:
                sc = self._score(score)
                nat.check(self._L.gw_rollout_episodes_scored(self._h, K, table.data_ptr(), *self._stream_id(seed, step0, env_id0),
                                                             C.byref(ep), C.byref(sc), prev.data_ptr(), self._ep_next.data_ptr(),
                                                             *[t.data_ptr() for t in out], self._stream()))
            else:
                nat.check(self._L.gw_rollout_episodes(self._h, K, table.data_ptr(), *self._stream_id(seed, step0, env_id0),
                                                      C.byref(ep), prev.data_ptr(), self._ep_next.data_ptr(),
                                                      *[t.data_ptr() for t in out], self._stream()))
        if K:
            self._last = (self._ep_next, out[3][-1], out[4][-1])
        return out

    def rollout_episodes_stats(self, cdf, steps, seed, max_steps=0, on_done=True, step0=0, env_id0=0, obs_prev=None, table=None,
                               packets=False):
        """``rollout_episodes`` for a caller that wants the tally, not the transitions (gw_rollout_episodes_stats): the same
        steps, draws, resets and episode bookkeeping, every transition ADDED into ``table`` (``rollout_policy_stats``' table)
        under the class of the observation the env acted on -- the reset's after an episode's end.  Returns the table.  A
        handle without the fused form runs ``rollout_episodes`` in chunks of at most 64 steps into buffers the env keeps, then
        ``transition_stats(..., ended=...)``: the same table.
        ``packets=True`` (gw_rollout_episodes_stats_delivered): the table is ``int64[3][A][8]``, its eighth column the data
        packets of the assigned sender the RRM decoded, summed per bin; the episodes' ``{age, ret}`` and tally keep the built-in
        reward -- the table is score-free, ``actions.table_score`` applies any score to it afterwards.  The fallback records
        with ``rollout_episodes(score=actions.make_score(D))`` -- the neutral score, under which ``reward`` is the built-in
        reward -- and ``transition_stats(..., delivered=)``: the same table; an explicit-queue handle, which keeps no delivered
        counter per env, is refused there with ``GW_EUNSUPPORTED``."""
        torch = _torch()
        ep, prev = self._episodes(max_steps, on_done, obs_prev, "rollout_episodes_stats")
        K, n = int(steps), self.num_envs
        cdf_t = self._policy_table(cdf)
        table = self._stats_table(table, packets)
        if K == 0:
            return table
        seed, step0, env_id0 = self._stream_id(seed, step0, env_id0)
        call = self._L.gw_rollout_episodes_stats_delivered if packets else self._L.gw_rollout_episodes_stats
        with torch.cuda.device(self.device):
            rc = call(self._h, K, cdf_t.data_ptr(), seed, step0, env_id0, C.byref(ep), prev.data_ptr(), self._ep_next.data_ptr(),
                      table.data_ptr(), self._stream())
        if rc == nat.EUNSUPPORTED and not os.environ.get("GW_ROLLOUT_STRICT"):
            seen = prev.clone()
            neutral = None
            if packets:
                from ..actions import make_score
                neutral = make_score(self.num_devices)

            def record(s, k, out):                         # refused before anything ran: compose it from the two other calls
                self.rollout_episodes(cdf_t, k, seed, max_steps, on_done, step0=step0 + s, env_id0=env_id0, obs_prev=seen, out=out,
                                      score=neutral)
                return self._ep_next
            self._compose_stats(K, table, seen, True, record, packets)
        else:
            nat.check(rc)
        self._last = (self._ep_next,) + tuple(self._last[1:])
        return table

    # -- a population of policies in one call (gw_rollout_population) -----------------------------------
    def rollout_population(self, cdfs, steps, seed, max_steps=0, on_done=True, step0=0, env_id0=0, obs_prev=None, tally=None,
                           score=None):
        """``rollout_episodes`` for P policies at once, for a caller that ranks them (gw_rollout_population): ``cdfs`` is
        ``[P][3][A]`` (``actions.policy_cdf`` of ``[P][3][A]`` probabilities), P divides ``num_envs``, and env ``e`` runs policy
        ``e // (num_envs // P)`` -- with the draws, state changes, resets and episode bookkeeping ``rollout_episodes`` would give
        it under that table (the stream is at ``(seed, env_id0 + e, step0 + k)``: ``env_id0`` shifts the stream, not the policy
        index).  Nothing ``[steps][N]`` is stored.  Returns the ``int64[P][5]`` tally, one ``episode_tally`` row per policy
        (``population_stats``): a new one of zeros, or the caller's ``tally``, ADDED into.  The episodes are the env's own --
        ``episode_state``, ``episode_tally`` (which gets every policy's episodes too) and the observation each env acts on next
        are shared with ``rollout_episodes``, so the calls continue one another; advance ``step0`` by ``steps``.
        One launch per 64 steps where ``num_envs // P`` is a multiple of 64 on a handle with a fused rollout; otherwise four
        small launches per step into six N-long rows the handle allocates at its first such call -- same results.  Not for
        hipGraph capture (``step0`` would be baked in).
        ``score`` (``actions.make_score``; gw_rollout_population_scored): the tally's return columns, and each env's ``ret``,
        are sums of step scores -- ``score[0] * reward + score[1 + device] * delivered`` -- so a caller can rank policies by the
        packets they delivered.  ``None`` is the call above, unchanged."""
        torch = _torch()
        from ..actions import EP_COLS
        ep, prev = self._episodes(max_steps, on_done, obs_prev, "rollout_population")
        K, n = int(steps), self.num_envs
        table = self._policy_table(cdfs, population=True)
        P = int(table.shape[0])
        if n % P:
            raise ValueError("rollout_population: %d policies do not divide %d envs" % (P, n))
        if tally is None:
            tally = torch.zeros((P, EP_COLS), dtype=torch.int64, device=self.device)
        elif not (type(tally) is torch.Tensor and tally.dtype is torch.int64 and tally.device == self.device
                  and tuple(tally.shape) == (P, EP_COLS) and tally.is_contiguous()):
            raise ValueError("tally must be a contiguous int64 tensor of shape (%d, %d) on %s" % (P, EP_COLS, self.device))
        pop = nat.Population(P, n // P, table.data_ptr(), tally.data_ptr())
        with torch.cuda.device(self.device):
            if score is not None:
                sc = self._score(score)
                nat.check(self._L.gw_rollout_population_scored(self._h, K, C.byref(pop), *self._stream_id(seed, step0, env_id0),
                                                               C.byref(ep), C.byref(sc), prev.data_ptr(), self._ep_next.data_ptr(),
                                                               self._stream()))
            else:
                nat.check(self._L.gw_rollout_population(self._h, K, C.byref(pop), *self._stream_id(seed, step0, env_id0), C.byref(ep),
                                                        prev.data_ptr(), self._ep_next.data_ptr(), self._stream()))
        if K:
            self._last = (self._ep_next,) + tuple(self._last[1:])
        return tally

    @staticmethod
    def population_stats(tally):
        """``episode_stats()`` per policy from a ``[P][5]`` tally (``rollout_population``): a dict of tensors of length P on
        the tally's device -- ``episodes`` and ``by_done`` int64, ``mean_length``, ``mean_return`` and ``return_stderr`` float64,
        ``nan`` where a policy ended no episode.  No host sync."""
        torch = _torch()
        t = torch.as_tensor(tally)
        if t.dim() != 2 or t.shape[1] != 5:
            raise ValueError("tally must have shape (P, 5), got %s" % (tuple(t.shape),))
        n, by_done = t[:, 0], t[:, 1]
        nf = n.to(torch.float64)
        nan = torch.full_like(nf, float("nan"))
        some = n > 0
        safe = torch.where(some, nf, torch.ones_like(nf))
        mean = t[:, 3].to(torch.float64) / safe
        err = ((t[:, 4].to(torch.float64) / safe - mean * mean).clamp(min=0.0) / safe).sqrt()
        return {"episodes": n, "by_done": by_done, "mean_length": torch.where(some, t[:, 2].to(torch.float64) / safe, nan),
                "mean_return": torch.where(some, mean, nan), "return_stderr": torch.where(some, err, nan)}

    # -- episodes for a caller that chooses the actions (gw_rollout_autoreset) ---------------------------
    def _autoreset(self, K, dev_ptr, dur_ptr, max_steps, on_done, ptrs, score=None):
        """gw_rollout_autoreset on the env's own episode tensors; ``ptrs``: the addresses of obs, reward, done, ended -- and, with
        a ``score`` (gw_rollout_autoreset_scored, through ctypes), of delivered."""
        idx = self._dev_index
        fast = self._fast
        if score is not None:
            # a step-by-step caller passes the same weights and limits every time: the two records are rebuilt only when the
            # score's bytes or the limits change (the episode tensors are allocated once, so their addresses hold)
            key = (score.tobytes() if type(score) is np.ndarray and score.dtype == np.int32 else None, max_steps, on_done)
            hit = self._scored_records
            if key[0] is None or hit is None or hit[0] != key:
                ep = nat.Episodes(max_steps, 1 if on_done else 0, self._ep_state.data_ptr(), self._ep_tally.data_ptr())
                hit = self._scored_records = (key, C.byref(ep), C.byref(self._score(score)), self._ep_next.data_ptr())
            if self._cuda_get_device() == idx:                        # the one-process-per-GPU case: no context manager
                rc = self._L.gw_rollout_autoreset_scored(self._h, K, dev_ptr, dur_ptr, hit[1], hit[2], hit[3], ptrs[0], ptrs[1],
                                                         ptrs[2], ptrs[3], ptrs[4], self._cuda_raw_stream(idx))
            else:
                with _torch().cuda.device(self.device):
                    rc = self._L.gw_rollout_autoreset_scored(self._h, K, dev_ptr, dur_ptr, hit[1], hit[2], hit[3], ptrs[0],
                                                             ptrs[1], ptrs[2], ptrs[3], ptrs[4], self._stream())
        elif fast is not None and self._cuda_get_device() == idx:     # the per-step route: no ctypes, no context manager
            rc = fast.rollout_autoreset(self._hv, K, dev_ptr, dur_ptr, max_steps, 1 if on_done else 0, self._ep_state.data_ptr(),
                                        self._ep_tally.data_ptr(), self._ep_next.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                        self._cuda_raw_stream(idx))
        else:
            ep = nat.Episodes(max_steps, 1 if on_done else 0, self._ep_state.data_ptr(), self._ep_tally.data_ptr())
            with _torch().cuda.device(self.device):
                rc = self._L.gw_rollout_autoreset(self._h, K, dev_ptr, dur_ptr, C.byref(ep), self._ep_next.data_ptr(), ptrs[0],
                                                  ptrs[1], ptrs[2], ptrs[3], self._stream())
        if rc:
            nat.check(rc)

    def rollout_autoreset(self, device, duration, max_steps=0, on_done=True, out=None, score=None):
        """``rollout()`` with episodes (gw_rollout_autoreset): K consecutive steps from pre-staged actions ``int32[K][N]``, in
        which an env whose step returned ``done`` (``on_done``), or whose episode has reached ``max_steps`` steps (0: no
        limit), is reset inside the launch exactly as ``reset(mask)`` would reset it between two steps.  Returns ``(obs, reward,
        done, ended)``, each ``[K][N]``: row k is what step k returned (``obs[k]`` the terminal observation where ``ended[k]``
        is 1 = done or 2 = step limit).  The episodes are the env's own -- ``episode_state``, ``episode_tally`` and the
        observation each env acts on next are shared with ``rollout_episodes``, ``step_autoreset`` and ``reset()``, so the
        calls continue one another.  An action outside the action space flags its env, leaves it untouched and still counts
        as a step of its episode.  ``out``: four ``[K][N]`` tensors to write into.  May be captured into a hipGraph.
        ``score`` (``actions.make_score``; gw_rollout_autoreset_scored): ``reward``, each env's ``ret`` and the tally's return
        columns carry the step's score -- ``score[0] * reward + score[1 + device] * delivered`` -- and a fifth output,
        ``delivered`` int32[K][N], the data packets of the staged sender the RRM decoded in the step (``out``: five tensors).
        A rejected action delivers 0 and scores 0.  Everything else is as without; ``None`` is the call above, unchanged."""
        torch = _torch()
        self._episodes(max_steps, on_done, None, "rollout_autoreset", needs_obs=False)
        dev = torch.as_tensor(device).to(device=self.device, dtype=torch.int32).contiguous()
        dur = torch.as_tensor(duration).to(device=self.device, dtype=torch.int32).contiguous()
        K, n = dev.shape[0], self.num_envs
        assert dev.shape == (K, n) and dur.shape == dev.shape
        out = self._rows(K, (torch.int32, torch.float32, torch.uint8, torch.uint8) + ((torch.int32,) if score is not None else ()), out)
        self._autoreset(K, dev.data_ptr(), dur.data_ptr(), int(max_steps), on_done, [t.data_ptr() for t in out], score)
        if K:
            self._last = (self._ep_next, out[1][-1], out[2][-1])
        return tuple(out)

    def rollout_backlog(self, steps, policy=None, max_steps=0, on_done=True, score=None, out=None):
        """``rollout_autoreset(score=)`` with a queue-aware scheduler choosing the actions inside the call (gw_rollout_backlog):
        at every step the band goes to the sender with the largest ``w_len[i] * qlen_i`` (the lowest index of a tie), for
        ``duration_of_len[its length]`` clamped to ``MAX_ASSIGN_DURATION - 1`` -- ``policy`` is ``actions.make_backlog_policy``'s
        image, ``None`` its default: the longest queue, for ``min(19, 4 * length)``.  The reference's RRM cannot see the
        senders' queues: this is a genie baseline to measure observation-bound policies against, not a reference path.
        Returns ``(obs, reward, done, ended, delivered, device, duration, seen_len)``, each ``[steps][N]``: the first five are
        ``rollout_autoreset(score=)``'s for the chosen actions (``score=None`` is ``actions.make_score(D)``: ``reward`` is the
        built-in reward), ``device`` / ``duration`` the actions chosen and ``seen_len`` the chosen sender's queue length when it
        was chosen.  Replaying ``device`` / ``duration`` through ``rollout_autoreset(score=)`` from the same state gives the
        same rows and state.  ``episode_state``, ``episode_tally`` and the observation acted on next are kept as that call
        keeps them.  ``out``: eight ``[steps][N]`` tensors to write into.  May be captured into a hipGraph."""
        torch = _torch()
        from ..actions import make_backlog_policy, BACKLOG_BYTES
        ep, _ = self._episodes(max_steps, on_done, None, "rollout_backlog", needs_obs=False)
        K = int(steps)
        if K < 0:
            raise ValueError("rollout_backlog: steps must be >= 0")
        if policy is None:
            policy = make_backlog_policy(self.num_devices, max_duration=self.MAX_ASSIGN_DURATION)
        image = np.asarray(policy)
        if image.shape != (BACKLOG_BYTES,) or image.dtype != np.uint8:
            raise ValueError("policy must be actions.make_backlog_policy()'s uint8[%d]" % BACKLOG_BYTES)
        pol = nat.BacklogPolicy.from_buffer_copy(image.tobytes() + b"\0" * (C.sizeof(nat.BacklogPolicy) - BACKLOG_BYTES))
        sc = self._score(score) if score is not None else None
        kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
        out = self._rows(K, kinds, out)
        if K == 0:
            return out
        p = [t.data_ptr() for t in out]
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout_backlog(self._h, K, C.byref(pol), C.byref(ep), C.byref(sc) if sc is not None else None,
                                                 self._ep_next.data_ptr(), p[5], p[6], p[7], p[0], p[1], p[2], p[3], p[4],
                                                 self._stream()))
        self._last = (self._ep_next, out[1][-1], out[2][-1])
        return out

    def rollout_backlog_population(self, policies, steps, max_steps=0, on_done=True, score=None, tally=None):
        """``rollout_backlog`` for P scheduler policies at once, for a caller that tunes them (gw_rollout_backlog_population):
        ``policies`` is ``actions.make_backlog_population``'s ``uint8[P][232]`` -- a tensor on the env's device, read in place,
        or the numpy image, which is uploaded -- P divides ``num_envs``, and env ``e`` runs policy ``e // (num_envs // P)``
        with the choices, steps, scores, resets and episode bookkeeping ``rollout_backlog`` would give it under that policy.
        Nothing ``[steps][N]`` is stored.  Returns the ``int64[P][5]`` tally, one ``episode_tally`` row per policy
        (``population_stats``): a new one of zeros, or the caller's ``tally``, ADDED into.  ``episode_state``,
        ``episode_tally`` (which gets every policy's episodes too) and the observation each env acts on next are kept as
        ``rollout_population(score=)`` keeps them.  The policies are not validated: a weight outside ``[0, SCORE_W_MAX]`` is
        clamped where it is read (``actions.backlog_sample_population_numpy``).  One launch per 64 steps where ``num_envs // P``
        is a multiple of 64 on a handle with a fused rollout; otherwise five small launches per step -- same results.
        May be captured into a hipGraph once ``policies`` and ``tally`` are the caller's tensors: a replay reads the policies
        the tensor holds then, so a search writes P policies, replays and reads P rows."""
        torch = _torch()
        from ..actions import EP_COLS, BACKLOG_STRIDE
        ep, _ = self._episodes(max_steps, on_done, None, "rollout_backlog_population", needs_obs=False)
        K, n = int(steps), self.num_envs
        if K < 0:
            raise ValueError("rollout_backlog_population: steps must be >= 0")
        if type(policies) is torch.Tensor:
            pols = policies
            if not (pols.dtype is torch.uint8 and pols.device == self.device and pols.dim() == 2 and pols.shape[1] == BACKLOG_STRIDE
                    and pols.is_contiguous()):
                raise ValueError("policies must be a contiguous uint8 tensor of shape (P, %d) on %s" % (BACKLOG_STRIDE, self.device))
        else:
            image = np.asarray(policies)
            if image.ndim != 2 or image.shape[1] != BACKLOG_STRIDE or image.dtype != np.uint8:
                raise ValueError("policies must be actions.make_backlog_population()'s uint8[P][%d]" % BACKLOG_STRIDE)
            pols = torch.from_numpy(np.array(image, order="C")).to(self.device)     # (a copy: the image may be read-only)
        P = int(pols.shape[0])
        if P < 1 or n % P:
            raise ValueError("rollout_backlog_population: %d policies do not divide %d envs" % (P, n))
        if tally is None:
            tally = torch.zeros((P, EP_COLS), dtype=torch.int64, device=self.device)
        elif not (type(tally) is torch.Tensor and tally.dtype is torch.int64 and tally.device == self.device
                  and tuple(tally.shape) == (P, EP_COLS) and tally.is_contiguous()):
            raise ValueError("tally must be a contiguous int64 tensor of shape (%d, %d) on %s" % (P, EP_COLS, self.device))
        sc = self._score(score) if score is not None else None
        pop = nat.BacklogPopulation(P, n // P, pols.data_ptr(), tally.data_ptr())
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout_backlog_population(self._h, K, C.byref(pop), C.byref(ep),
                                                            C.byref(sc) if sc is not None else None, self._ep_next.data_ptr(),
                                                            self._stream()))
        if K:
            self._last = (self._ep_next,) + tuple(self._last[1:])
        return tally

    # -- finite-state controllers inside the scored closed loop (gw_rollout_controller) -----------------
    @property
    def controller_node(self):
        """uint8[N] on the GPU: the node each env's controller is at, as ``rollout_controller`` /
        ``rollout_controller_population`` read it before a call and leave it after; ``reset()`` zeroes the envs it resets.
        The caller may write it."""
        if self._ctl_node is None:
            self._ctl_node = _torch().zeros(self.num_envs, dtype=_torch().uint8, device=self.device)
        return self._ctl_node

    def _controller(self, controller, population=False):
        """A controller's three arrays as tensors on this env's GPU: ``(cdf int32 words [S][3][A], next uint8[S][3][2], need
        uint8[S])``, each with a leading ``[P]`` for a population.  Shapes and dtypes are checked, contents are not (the native
        calls clamp where they read).  Tensors that already lie on the device are used in place."""
        torch = _torch()
        from ..actions import FSC_MAX_STATES
        A = self.num_devices * int(self.config.max_duration)
        if len(controller) != 3:
            raise ValueError("a controller is (cdf, next, need)")

        def put(a, np_dtype, torch_dtype):
            if isinstance(a, torch.Tensor):
                if a.dtype is not torch_dtype:
                    raise ValueError("a controller tensor must be %s, got %s" % (torch_dtype, a.dtype))
                return a.to(self.device).contiguous()
            a = np.asarray(a)
            if a.dtype != np_dtype:
                raise ValueError("a controller array must be %s, got %s" % (np.dtype(np_dtype), a.dtype))
            a = np.array(a, order="C")                    # (a copy: the array may be read-only)
            return torch.from_numpy(a.view(np.int32) if np_dtype is np.uint32 else a).to(self.device)
        cdf, nxt, need = put(controller[0], np.uint32, torch.int32), put(controller[1], np.uint8, torch.uint8), \
            put(controller[2], np.uint8, torch.uint8)
        lead = cdf.dim() - 3
        if lead != (1 if population else 0) or tuple(cdf.shape[-2:]) != (3, A) or not 1 <= cdf.shape[-3] <= FSC_MAX_STATES:
            raise ValueError("controller cdf must have shape (%sS, 3, %d) with 1 <= S <= %d, got %s"
                             % ("P, " if population else "", A, FSC_MAX_STATES, tuple(cdf.shape)))
        head = tuple(cdf.shape[:-2])
        if tuple(nxt.shape) != head + (3, 2) or tuple(need.shape) != head:
            raise ValueError("controller next / need must have shapes %s / %s, got %s / %s"
                             % (head + (3, 2), head, tuple(nxt.shape), tuple(need.shape)))
        return cdf, nxt, need

    def rollout_controller(self, controller, steps, seed, max_steps=0, on_done=True, step0=0, env_id0=0, obs_prev=None, out=None,
                           score=None):
        """``rollout_episodes(score=)`` under a finite-state controller (gw_rollout_controller): ``controller`` is
        ``actions.make_controller``'s ``(cdf, next, need)``; env ``e`` at node ``n`` draws from row ``cdf[n][cls(obs)]``, and
        behind every step moves to ``next[n][cls(new obs)][delivered >= need[n]]`` -- to node 0 where the step ended an
        episode (``actions.controller_step_numpy`` / ``controller_move_numpy`` restate both, with the clamps that make any
        content memory-safe).  The nodes live in ``controller_node`` and continue across calls, as ``episode_state`` does;
        advance ``step0`` by ``steps``.  Returns the scored ``rollout_episodes`` tuple plus ``node`` uint8[steps][N], the node
        each step was taken at (``out``: eight tensors).  ``score``: ``actions.make_score``; ``None`` is the neutral score.  With
        one node the call is ``rollout_episodes(score=)`` bit for bit.  One launch per 64 steps; a handle without the fused
        rollout, or a controller that does not fit the block's LDS, is refused (``NativeError``, ``EUNSUPPORTED``) before
        anything runs: there is no per-step form.  Not for hipGraph capture (``step0`` would be baked in)."""
        torch = _torch()
        from ..actions import make_score
        ep, prev = self._episodes(max_steps, on_done, obs_prev, "rollout_controller")
        K = int(steps)
        cdf, nxt, need = self._controller(controller)
        kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.uint8)
        out = self._rows(K, kinds, out)
        if K:
            prev = self._apart(prev, out)
        sc = self._score(score if score is not None else make_score(self.num_devices))
        ctl = nat.Controller(int(cdf.shape[0]), cdf.data_ptr(), nxt.data_ptr(), need.data_ptr(), self.controller_node.data_ptr())
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout_controller(self._h, K, C.byref(ctl), *self._stream_id(seed, step0, env_id0), C.byref(ep),
                                                    C.byref(sc), prev.data_ptr(), self._ep_next.data_ptr(),
                                                    *[t.data_ptr() for t in out], self._stream()))
        if K:
            self._last = (self._ep_next, out[3][-1], out[4][-1])
        return out

    def rollout_controller_population(self, controllers, steps, seed, max_steps=0, on_done=True, step0=0, env_id0=0, obs_prev=None,
                                      tally=None, score=None):
        """``rollout_controller`` for P controllers of one size at once, for a caller that ranks them
        (gw_rollout_controller_population): ``controllers`` is ``actions.make_controller_population``'s ``(cdf [P][S][3][A],
        next [P][S][3][2], need [P][S])`` -- tensors on the env's device are read in place -- P divides ``num_envs``, and env
        ``e`` runs controller ``e // (num_envs // P)`` (``env_id0`` shifts the stream, not the controller index).  Nothing
        ``[steps][N]`` is stored.  Returns the ``int64[P][5]`` tally as ``rollout_population(score=)`` does: a new one of
        zeros, or the caller's ``tally``, ADDED into.  ``num_envs // P`` must be a multiple of 64; there is no per-step form."""
        torch = _torch()
        from ..actions import EP_COLS, make_score
        ep, prev = self._episodes(max_steps, on_done, obs_prev, "rollout_controller_population")
        K, n = int(steps), self.num_envs
        cdf, nxt, need = self._controller(controllers, population=True)
        P = int(cdf.shape[0])
        if P < 1 or n % P:
            raise ValueError("rollout_controller_population: %d controllers do not divide %d envs" % (P, n))
        if tally is None:
            tally = torch.zeros((P, EP_COLS), dtype=torch.int64, device=self.device)
        elif not (type(tally) is torch.Tensor and tally.dtype is torch.int64 and tally.device == self.device
                  and tuple(tally.shape) == (P, EP_COLS) and tally.is_contiguous()):
            raise ValueError("tally must be a contiguous int64 tensor of shape (%d, %d) on %s" % (P, EP_COLS, self.device))
        sc = self._score(score if score is not None else make_score(self.num_devices))
        pop = nat.ControllerPopulation(P, n // P, int(cdf.shape[1]), cdf.data_ptr(), nxt.data_ptr(), need.data_ptr(),
                                       self.controller_node.data_ptr(), tally.data_ptr())
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_rollout_controller_population(self._h, K, C.byref(pop), *self._stream_id(seed, step0, env_id0),
                                                               C.byref(ep), C.byref(sc), prev.data_ptr(), self._ep_next.data_ptr(),
                                                               self._stream()))
        if K:
            self._last = (self._ep_next,) + tuple(self._last[1:])
        return tally

    def step_autoreset(self, action, max_steps=0, on_done=True, out=None, score=None):
        """One ``env.step()`` with autoreset -- ``rollout_autoreset`` of one step on 1-D tensors: the step, the episode
        bookkeeping and the reset of the envs whose episode it ended, in one launch.  Returns ``(obs, reward, done, ended,
        obs_next)``: what the step returned (``obs`` is the terminal observation where ``ended`` is not 0) and the
        observation to act on next (``COUNTER_BOUND`` for the envs just reset; the env's own tensor, rewritten by every
        episodic call).  ``out``: a ``StepOutputs`` with an ``ended`` tensor.  Action tensors go through ``step()``'s cache and
        its aliasing contract.  May be captured into a hipGraph.
        ``score`` (``actions.make_score``; gw_rollout_autoreset_scored): ``reward`` is the step's score and the return value
        gains ``delivered`` int32[N] -- ``(obs, reward, done, ended, obs_next, delivered)``; ``out`` then needs a ``delivered``
        tensor too.  A recorded graph keeps the weights it was recorded with."""
        if self._ep_state is None or self._custom is not None or max_steps < 0:
            self._episodes(max_steps, on_done, None, "step_autoreset", needs_obs=False)
        dev = action["device"]
        dur = action["duration"]
        seen = self._seen
        hit = seen.get(id(dev))
        if hit is None or hit[0]() is not dev:
            dev = self._checked(dev, "device")
            dev_ptr = dev.data_ptr()
        else:
            dev_ptr = hit[1]
        hit = seen.get(id(dur))
        if hit is None or hit[0]() is not dur:
            dur = self._checked(dur, "duration")
            dur_ptr = dur.data_ptr()
        else:
            dur_ptr = hit[1]
        if out is None:
            torch = _torch()
            obs, rew, done = self._outputs()
            ended = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
            ptrs = (obs.data_ptr(), rew.data_ptr(), done.data_ptr(), ended.data_ptr())
            if score is not None:
                delivered = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
                ptrs += (delivered.data_ptr(),)
        else:
            if out._dev != self._dev_index:
                raise ValueError("StepOutputs on cuda:%d passed to an env on cuda:%d" % (out._dev, self._dev_index))
            if not out._ended_ptr:
                raise ValueError("step_autoreset: the StepOutputs needs an `ended` tensor")
            obs, rew, done, ended = out.obs, out.reward, out.done, out.ended
            p = out._ptrs
            ptrs = (p[0], p[1], p[2], out._ended_ptr)
            if score is not None:
                if not out._delivered_ptr:
                    raise ValueError("step_autoreset(score=): the StepOutputs needs a `delivered` tensor")
                delivered = out.delivered
                ptrs += (out._delivered_ptr,)
        self._autoreset(1, dev_ptr, dur_ptr, int(max_steps), on_done, ptrs, score)
        self._last = (self._ep_next, rew, done)
        if score is not None:
            return obs, rew, done, ended, self._ep_next, delivered
        return obs, rew, done, ended, self._ep_next

    def episode_stats(self):
        """The episodes the episodic calls (``rollout_episodes``, ``rollout_episodes_stats``, ``rollout_autoreset``,
        ``step_autoreset``) have ended on this env so far, from the tally:
        ``{"episodes", "by_done", "mean_length", "mean_return", "return_stderr"}`` (the means are ``nan`` before the first
        episode ends).  Reads five numbers back: a host sync."""
        n, by_done, length, ret, sq = (int(x) for x in self._ep_tally.cpu()) if self._ep_tally is not None else (0,) * 5
        if n == 0:
            nan = float("nan")
            return {"episodes": 0, "by_done": 0, "mean_length": nan, "mean_return": nan, "return_stderr": nan}
        mean = ret / n
        return {"episodes": n, "by_done": by_done, "mean_length": length / n, "mean_return": mean,
                "return_stderr": (max(sq / n - mean * mean, 0.0) / n) ** 0.5}

    def render(self, mode='human', close=False):          # counter_traffic.py:160-162
        values = self.received()[0].tolist()
        print("Last Received: {}, difference: {:6d}".format(values, values[1] - values[0]), end='\r')

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.gw_destroy(self._h)
            self._h = C.c_void_p()
            self._hv = 0
            stepper = self.__dict__.get("step")                # the native stepper holds the handle's address too
            if stepper is not None and hasattr(stepper, "handle"):
                stepper.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state access ---------------------------------------------------------------------------
    def received(self):
        """interpreter.receivedValues of every env: int32[N][D] tensor on the GPU."""
        torch = _torch()
        out = torch.empty((self.num_envs, self.num_devices), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_received(self._h, out.data_ptr(), self._stream()))
        return out

    def pack_feedback(self, obs, reward, done, out=None, check=False):
        """(obs int32, reward float32, done uint8) tensors of any common shape -> one byte per element
        (bits 0-1 sign(obs - COUNTER_BOUND) + 1, bits 2-6 reward + 10, bit 7 done).  Lossless for the built-in
        interpreter; the unit the multi-GPU observation gather moves (sharding.ChunkedFeedbackGather)."""
        torch = _torch()
        assert obs.is_contiguous() and reward.is_contiguous() and done.is_contiguous()
        assert obs.dtype == torch.int32 and reward.dtype == torch.float32 and done.dtype == torch.uint8
        if out is None:
            out = torch.empty(obs.shape, dtype=torch.uint8, device=self.device)
        assert out.is_contiguous() and out.numel() == obs.numel() == reward.numel() == done.numel()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_pack_feedback(self._h, obs.numel(), obs.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                               out.data_ptr(), 1 if check else 0, self._stream()))
        return out

    def unpack_feedback(self, packed, obs=None, reward=None, done=None):
        torch = _torch()
        assert packed.is_contiguous() and packed.dtype == torch.uint8
        obs = torch.empty(packed.shape, dtype=torch.int32, device=self.device) if obs is None else obs
        reward = torch.empty(packed.shape, dtype=torch.float32, device=self.device) if reward is None else reward
        done = torch.empty(packed.shape, dtype=torch.uint8, device=self.device) if done is None else done
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_unpack_feedback(self._h, packed.numel(), packed.data_ptr(), obs.data_ptr(),
                                                 reward.data_ptr(), done.data_ptr(), self._stream()))
        return obs, reward, done

    def set_position(self, radio, x, y, mask=None):
        """``device.position.set(x, y)`` on radio ``radio`` (0..D-1 senders, D = the RRM) of every env (or of the envs
        selected by ``mask``), between two steps (devices/core.py:77-86): float64[N] tensors/arrays or scalars."""
        torch = _torch()
        xs = torch.as_tensor(x, dtype=torch.float64, device=self.device).expand(self.num_envs).contiguous()
        ys = torch.as_tensor(y, dtype=torch.float64, device=self.device).expand(self.num_envs).contiguous()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            assert m.shape == (self.num_envs,)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_set_position(self._h, int(radio), xs.data_ptr(), ys.data_ptr(),
                                              m.data_ptr() if m is not None else None, self._stream()))

    def set_positions(self, positions, mask=None):
        """Positions of every radio of every env at once: float64[N][D+1][2] (row D = the RRM)."""
        torch = _torch()
        pos = torch.as_tensor(positions, dtype=torch.float64, device=self.device).contiguous()
        assert pos.shape == (self.num_envs, self.num_devices + 1, 2)
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            assert m.shape == (self.num_envs,)
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_set_positions(self._h, pos.data_ptr(), m.data_ptr() if m is not None else None, self._stream()))

    def enqueue(self, device, payload_bytes):
        """SimpleNetworkDevice.send(data, dest) on sender `device` of every env (networking/devices.py:84-86):
        payload_bytes is an int or an int32[N] tensor/array; negative entries enqueue nothing."""
        torch = _torch()
        pb = torch.as_tensor(payload_bytes, dtype=torch.int32, device=self.device).expand(self.num_envs).contiguous()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_enqueue(self._h, int(device), pb.data_ptr(), self._stream()))

    _FIELDS = {
        "peer_received": (np.uint32, lambda D, R: (D,)),
        "now": (np.float64, lambda D, R: ()), "wake": (np.float64, lambda D, R: (D,)),
        "counter": (np.uint32, lambda D, R: (D,)), "qlen": (np.int32, lambda D, R: (D,)),
        "queue": (np.uint32, lambda D, R: (D, nat.QUEUE_CAP)),
        "received": (np.int32, lambda D, R: (D,)), "latest_diff": (np.int32, lambda D, R: ()),
        "last_abs": (np.int32, lambda D, R: ()), "rx_power": (np.float64, lambda D, R: (R,)),
        "pos": (np.float64, lambda D, R: (R, 2)), "link_power": (np.float64, lambda D, R: (R, R)),
        "flags": (np.uint32, lambda D, R: ()), "n_tx": (np.uint64, lambda D, R: ()),
        "n_delivered": (np.uint64, lambda D, R: ()), "n_appended": (np.uint64, lambda D, R: ()),
        "n_popped": (np.uint64, lambda D, R: ()), "n_dropped": (np.uint64, lambda D, R: ()),
    }

    def get_state(self, field):
        """Synchronous host copy of one state field (numpy), in the oracle's logical layout."""
        dtype, shp = self._FIELDS[field]
        out = np.empty((self.num_envs,) + shp(self.num_devices, self.num_devices + 1), dtype)
        nat.check(self._L.gw_get_state(self._h, field.encode(), out.ctypes.data, out.nbytes))
        return out

    def stats(self):
        s = nat.Stats()
        nat.check(self._L.gw_stats_read(self._h, C.byref(s)))
        return s.as_dict()

    def state_bytes(self):
        b = C.c_uint64()
        nat.check(self._L.gw_state_bytes(self._h, C.byref(b)))
        return int(b.value)

    def snapshot(self):
        """Checkpoint: every byte of this env's device state as one uint8 numpy array (synchronises).  ``restore()`` puts it
        back -- into this env later on, or into a fresh env created with the same arguments -- and every later step continues
        bit for bit as this one would have (gw_get_snapshot / gw_set_state)."""
        n = C.c_uint64()
        nat.check(self._L.gw_snapshot_bytes(self._h, C.byref(n)))
        out = np.empty(int(n.value), np.uint8)
        nat.check(self._L.gw_get_snapshot(self._h, out.ctypes.data, out.nbytes))
        return out

    def restore(self, snap):
        snap = np.ascontiguousarray(snap, dtype=np.uint8)
        nat.check(self._L.gw_set_state(self._h, snap.ctypes.data, snap.nbytes))
        self._seen.clear()

    def link_info(self, frm, to):
        a, p = C.c_double(), C.c_double()
        nat.check(self._L.gw_link_info(self._h, frm, to, C.byref(a), C.byref(p)))
        return a.value, p.value

    def noise_states(self, radio):
        n = C.c_int32()
        vals = (C.c_double * nat.MAX_NSTATES)()
        nat.check(self._L.gw_noise_states(self._h, radio, C.byref(n), vals))
        return [vals[i] for i in range(n.value)]

    def check(self, strict=False):
        """Raise if any env hit a condition outside the modelled horizon or got a bad action.  The returned totals carry
        ``"ties"``: whether an exact f64 time tie was resolved by the insertion-order rule (GW_FLAG_TIE) -- the kernels and
        the oracle resolve it the same way, but the reference's order there rests on SimPy's event ids; ``strict=True``
        raises on it too.  Flags are sticky: ``clear_flags()`` resets them so that a later check tells when they arose."""
        st = self.stats()
        fl = st["flags_or"]
        st["ties"] = bool(fl & nat.FLAG_TIE)
        if fl & nat.FLAG_BADACT:
            raise AssertionError("%d env-step(s) had an action outside the action space" % st["bad_actions"])
        if fl & nat.FLAG_INTERNAL:
            raise RuntimeError("a kernel self-check failed in some env (GW_FLAG_INTERNAL): state invalid, please report")
        if fl & (nat.FLAG_CARRY | nat.FLAG_REFEXC):
            raise RuntimeError("step horizon not closed in some env (flags 0x%x)" % fl)
        if strict and st["ties"]:
            raise RuntimeError("an exact time tie was resolved by the insertion-order rule in some env (GW_FLAG_TIE)")
        return st

    def clear_flags(self):
        """Zero the sticky per-env GW_FLAG_* words (event counters are untouched)."""
        torch = _torch()
        with torch.cuda.device(self.device):
            nat.check(self._L.gw_clear_flags(self._h, self._stream()))


class CounterTrafficEnv(VecCounterTrafficEnv):
    """Drop-in for gymwipe.envs.CounterTrafficEnv (2 senders + RRM, one env): Python scalars in,
    Python scalars out, ``AssertionError`` on an action outside the action space
    (counter_traffic.py:146-158)."""
    _scalar_api = True

    def __init__(self, device="cuda:0", num_devices=2, **kw):
        VecCounterTrafficEnv.__init__(self, 1, num_devices=num_devices, device=device,
                                      reuse_outputs=True, **kw)
        torch = _torch()
        self._act = torch.zeros((2, 1), dtype=torch.int32, device=self.device)

    def _info(self):
        return {"Latest received values": str(self.received()[0].tolist())}   # :109-112

    def reset(self):
        return int(VecCounterTrafficEnv.reset(self).item())

    def step(self, action):
        assert self.action_space.contains(action)                              # :147
        self._act[0, 0] = int(action["device"])
        self._act[1, 0] = int(action["duration"])
        obs, rew, done, _ = VecCounterTrafficEnv.step(self, {"device": self._act[0], "duration": self._act[1]})
        self._last = (int(obs.item()), float(rew.item()), bool(done.item()))
        return self._last + (self._info(),)
