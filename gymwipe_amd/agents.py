"""
The caller side of the hot path: what the reference's example agent
(agents/dqn_counter_traffic.py) needs between a flat-action DQN and the env, vectorised and kept on
the GPU so that ``policy -> env.step -> replay`` involves no host round trip.

``CounterTrafficProcessor``  the keras-rl ``Processor`` of the reference (:23-33): flat action ->
                             ``{"device", "duration"}``; Python ints in, ints out (same arithmetic),
                             or an int tensor in, int32 tensors out (used in place by the env).
``DqnCounterTrafficAgent``   a small torch DQN with the reference example's shape (:47-63):
                             Dense 16-16-16 with ReLU on the 1-d observation, Boltzmann policy, Adam
                             1e-3, soft target update 1e-2, sequential replay memory -- over N envs.
                             It exists to drive the env from a GPU-resident policy, not to be a
                             tuned learner (the reference's own reward shaping is "most likely far
                             away from being perfect", counter_traffic.py:86-92).
"""
from .envs.core import BaseEnv


class CounterTrafficProcessor:
    """agents/dqn_counter_traffic.py:23-33."""

    def __init__(self, max_duration=BaseEnv.MAX_ASSIGN_DURATION):
        self.max_duration = int(max_duration)

    def process_action(self, flat_action):
        assert flat_action is not None
        md = self.max_duration
        try:
            import torch
            is_tensor = isinstance(flat_action, torch.Tensor)
        except ImportError:                                   # pragma: no cover
            is_tensor = False
        if is_tensor:
            flat = flat_action.to(torch.int32)
            device = torch.div(flat, md, rounding_mode="trunc")          # int(flat_action / max_duration)
            return {"device": device, "duration": flat - device * md}
        device = int(flat_action / md)
        return {"device": device, "duration": flat_action - (device * md)}


class DqnCounterTrafficAgent:
    def __init__(self, env, hidden=16, lr=1e-3, gamma=0.99, tau=1.0, target_update=1e-2, memory_limit=50000,
                 batch_size=32, warmup_steps=1000, seed=123):
        import torch
        from torch import nn
        self.torch = torch
        self.env = env
        self.n = env.num_envs
        self.dev = env.device
        self.processor = CounterTrafficProcessor(env.MAX_ASSIGN_DURATION)
        self.nb_devices = env.action_space.spaces["device"].n
        self.nb_durations = env.action_space.spaces["duration"].n
        self.nb_actions = self.nb_devices * self.nb_durations      # agents/dqn_counter_traffic.py:41-44
        torch.manual_seed(seed)

        def net():
            return nn.Sequential(nn.Linear(1, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                                 nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, self.nb_actions)).to(self.dev)
        self.q, self.q_target = net(), net()
        self.q_target.load_state_dict(self.q.state_dict())
        self.opt = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.gamma, self.tau, self.target_update = gamma, tau, target_update
        self.batch_size, self.warmup = batch_size, warmup_steps
        # sequential memory of the last `memory_limit` transitions, on the GPU (rl.memory.SequentialMemory)
        cap = max(memory_limit, self.n)
        self.cap = cap // self.n * self.n
        self.m_obs = torch.zeros(self.cap, device=self.dev)
        self.m_next = torch.zeros(self.cap, device=self.dev)
        self.m_act = torch.zeros(self.cap, dtype=torch.int64, device=self.dev)
        self.m_rew = torch.zeros(self.cap, device=self.dev)
        self.m_done = torch.zeros(self.cap, device=self.dev)
        self.m_pos, self.m_len, self.steps = 0, 0, 0
        self.center = float(env.COUNTER_BOUND)
        self.seed, self.stream_pos = int(seed), 0             # collect(): the draws' stream and how far it has been used

    def _features(self, obs):
        return (obs.to(self.torch.float32) - self.center).unsqueeze(-1)   # the observation is centred on COUNTER_BOUND

    def act(self, obs):
        """Boltzmann policy over Q (rl.policy.BoltzmannQPolicy: exp(clip(q / tau, -500, 500)))."""
        torch = self.torch
        with torch.no_grad():
            qv = self.q(self._features(obs))
            p = torch.softmax(torch.clamp(qv / self.tau, -500.0, 500.0), dim=-1)
            return torch.multinomial(p, 1).squeeze(-1)

    def policy_cdf(self):
        """The policy of ``act()`` as the table ``env.rollout_policy`` draws from: Q at the three values an observation takes
        (COUNTER_BOUND + payload_value * {-1, 0, +1}), the same clip and softmax, ``actions.policy_cdf`` -- built on the GPU,
        no host sync."""
        from .actions import policy_cdf
        torch = self.torch
        pv = float(self.env.config.payload_value)
        with torch.no_grad():
            obs = torch.tensor([self.center - pv, self.center, self.center + pv], device=self.dev)
            qv = self.q(self._features(obs))
            return policy_cdf(torch.softmax(torch.clamp(qv / self.tau, -500.0, 500.0), dim=-1))

    def collect(self, steps, episode_steps=None, score=None):
        """``steps`` env steps of all N envs under the current policy in ONE ``env.rollout_policy`` call -- observation ->
        policy -> step inside the launch -- and their transitions into the replay memory.  Returns the rollout's
        ``(device, duration, obs, reward, done)``.
        ``episode_steps``: episodes of at most that many steps, ended by ``done`` too, through ``env.rollout_episodes`` (the
        reference's caller: keras-rl resets on done and after nb_max_episode_steps).  The memory then holds the observation
        each step acted on -- the reset's after an episode's end -- as ``m_obs`` and the terminal observation as ``m_next``;
        the return value gains ``ended``.
        ``score`` (``actions.make_score``; needs ``episode_steps``): passed on to ``rollout_episodes`` -- the memory's reward
        is the step's score, the return value gains ``delivered``."""
        torch = self.torch
        steps = int(steps)
        if score is not None and episode_steps is None:
            raise ValueError("collect(score=) needs episode_steps: only the episodic rollout has a scored form")
        if self.env._last[0] is None:
            self.env.reset()
        first = self.env._last[0].clone()
        if episode_steps is None:
            rows = self.env.rollout_policy(self.policy_cdf(), steps, self.seed, step0=self.stream_pos)
            after = rows[2][:-1]
        else:
            rows = self.env.rollout_episodes(self.policy_cdf(), steps, self.seed, max_steps=int(episode_steps), on_done=True,
                                             step0=self.stream_pos, score=score)
            after = torch.where(rows[5][:-1] != 0, torch.full_like(rows[2][:-1], int(self.center)), rows[2][:-1])
        dev, dur, obs, rew, done = rows[:5]
        self.stream_pos += steps
        self.steps += steps
        keep = min(steps, self.cap // self.n)                  # (more steps than the memory holds: the last ones)
        if keep:
            seen = torch.cat([first.unsqueeze(0), after])[steps - keep:]
            flat = (dev.to(torch.int64) * self.processor.max_duration + dur.to(torch.int64))[steps - keep:]
            at = (self.m_pos + torch.arange(keep * self.n, device=self.dev)) % self.cap
            self.m_obs[at] = seen.reshape(-1).to(torch.float32)
            self.m_next[at] = obs[steps - keep:].reshape(-1).to(torch.float32)
            self.m_act[at] = flat.reshape(-1)
            self.m_rew[at] = rew[steps - keep:].reshape(-1)
            self.m_done[at] = done[steps - keep:].reshape(-1).to(torch.float32)
            self.m_pos = (self.m_pos + keep * self.n) % self.cap
            self.m_len = min(self.m_len + keep * self.n, self.cap)
        return rows

    def remember(self, obs, act, rew, nxt, done):
        i = self.m_pos
        sl = slice(i, i + self.n)
        self.m_obs[sl] = obs.to(self.torch.float32)
        self.m_next[sl] = nxt.to(self.torch.float32)
        self.m_act[sl] = act
        self.m_rew[sl] = rew
        self.m_done[sl] = done.to(self.torch.float32)
        self.m_pos = (i + self.n) % self.cap
        self.m_len = min(self.m_len + self.n, self.cap)

    def learn(self):
        torch = self.torch
        idx = torch.randint(0, self.m_len, (self.batch_size,), device=self.dev)
        q = self.q(self._features(self.m_obs[idx])).gather(1, self.m_act[idx].unsqueeze(1)).squeeze(1)
        with torch.no_grad():
            target = self.m_rew[idx] + self.gamma * (1.0 - self.m_done[idx]) * self.q_target(self._features(self.m_next[idx])).max(dim=1).values
        loss = torch.nn.functional.mse_loss(q, target)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        with torch.no_grad():                                  # soft target update (target_model_update = 1e-2)
            for pt, p in zip(self.q_target.parameters(), self.q.parameters()):
                pt.mul_(1.0 - self.target_update).add_(p, alpha=self.target_update)
        return loss

    def fit(self, nb_steps, reset_every=64, episode_steps=None, score=None):
        """Vectorised dqn.fit(): nb_steps env.step() calls of all N envs; returns the last loss (tensor).
        ``episode_steps``: per-env episodes of at most that many steps, ended by ``done`` too, through
        ``env.step_autoreset`` (keras-rl's reset on done and nb_max_episode_steps) instead of the global reset every
        ``reset_every`` steps: the memory gets the terminal observation as ``m_next``, and the next action is for the
        observation the env acts on next -- the reset's where the step ended an episode.
        ``score`` (``actions.make_score``; needs ``episode_steps``, there is no scored plain ``step()``): the steps go through
        ``env.step_autoreset(score=)`` and the memory's reward is the step's score -- ``make_score(D, reward=0, delivered=1)``
        trains on the packets the RRM decoded -- as are the returns of ``env.episode_stats()``."""
        if score is not None and episode_steps is None:
            raise ValueError("fit(score=) needs episode_steps: only step_autoreset has a scored form")
        obs = self.env.reset().clone()
        loss = None
        if episode_steps is not None:
            for k in range(nb_steps):
                flat = self.act(obs)
                o, r, d, _, nxt = self.env.step_autoreset(self.processor.process_action(flat), max_steps=int(episode_steps),
                                                          on_done=True, score=score)[:5]
                self.remember(obs, flat, r, o, d)
                obs = nxt.clone()
                self.steps += 1
                if self.steps * self.n >= self.warmup and self.m_len >= self.batch_size:
                    loss = self.learn()
            return loss
        for k in range(nb_steps):
            if k and reset_every and k % reset_every == 0:
                obs = self.env.reset().clone()
            flat = self.act(obs)
            o, r, d, _ = self.env.step(self.processor.process_action(flat))
            self.remember(obs, flat, r, o, d)
            obs = o.clone()
            self.steps += 1
            if self.steps * self.n >= self.warmup and self.m_len >= self.batch_size:
                loss = self.learn()
        return loss


class TabularCounterTrafficAgent:
    """The agent this env admits exactly: it sees one of three observation values and picks one of A = num_devices *
    max_duration flat actions, so its Q function is a ``[3][A]`` table and everything it learns from is the table of
    ``env.rollout_policy_stats`` -- visits, reward sums, where the next observation landed, how often ``done`` fired, per
    (observation class, action).  ``collect`` is one launch per 64 steps and no per-env array; ``learn`` and ``evaluate`` are
    arithmetic on ``[3][A]`` tensors on the GPU.  Nothing here is sized by the number of envs.

    ``score`` (``actions.make_score``): the agent learns from the step's score instead of the built-in reward, whose return
    telescopes to 0 or ``-payload_value`` per episode and is highest for the policy that assigns nothing.  It then keeps the
    eight-column table (``packets=True``: the packets delivered per bin beside the reward sum) and ``learn`` uses
    ``actions.table_score / n`` in place of ``r_sum / n`` -- exact, because the score is linear and the flat action names the
    sender.  ``evaluate`` returns the mean score per step and ``None`` for the standard error: the table holds no score
    squares.  ``score=None`` is the agent above, unchanged."""

    def __init__(self, env, gamma=0.99, tau=1.0, seed=123, episode_steps=None, score=None):
        import torch
        self.torch = torch
        self.env = env
        self.episode_steps = None if episode_steps is None else int(episode_steps)   # episodes inside the launch (see _rollout)
        self.dev = env.device
        self.max_duration = int(env.config.max_duration)
        self.nb_actions = int(env.num_devices) * self.max_duration
        self.gamma, self.tau = float(gamma), float(tau)
        self.score = score
        self.q = torch.zeros((3, self.nb_actions), dtype=torch.float64, device=self.dev)
        self.table = torch.zeros((3, self.nb_actions, 7 if score is None else 8), dtype=torch.int64, device=self.dev)   # everything collected so far
        self.seed, self.stream_pos = int(seed), 0

    def policy_cdf(self):
        """Boltzmann policy over Q (``DqnCounterTrafficAgent.act``'s rule: exp(clip(q / tau, -500, 500)), normalised) as the
        table ``env.rollout_policy_stats`` draws from; built where Q lives, no host sync."""
        from .actions import policy_cdf
        torch = self.torch
        return policy_cdf(torch.softmax(torch.clamp(self.q / self.tau, -500.0, 500.0), dim=-1))

    def _rollout(self, steps, table):
        """``episode_steps`` set: ``env.rollout_episodes_stats`` -- an env is reset inside the launch on done and after that
        many steps, so no caller-side ``env.reset()`` is needed to keep the envs out of their absorbing state."""
        steps = int(steps)
        if self.env._last[0] is None:
            self.env.reset()
        kw = {} if self.score is None else {"packets": True}
        if self.episode_steps is None:
            self.env.rollout_policy_stats(self.policy_cdf(), steps, self.seed, step0=self.stream_pos, table=table, **kw)
        else:
            self.env.rollout_episodes_stats(self.policy_cdf(), steps, self.seed, max_steps=self.episode_steps, on_done=True,
                                            step0=self.stream_pos, table=table, **kw)
        self.stream_pos += steps
        return table

    def collect(self, steps):
        """``steps`` env steps of all N envs under the current policy, their transitions added into ``self.table``."""
        return self._rollout(steps, self.table)

    @staticmethod
    def q_iteration(q, table, gamma, sweeps=1, r_sum=None):
        """``sweeps`` sweeps of Q-iteration on the empirical model of the visited pairs of ``table`` (int64[3][A][7], or the
        eight-column table): ``Q[s,a] <- r_sum/n + gamma * (1 - done/n) * sum_s' next[s']/n * max_a' Q[s',a']``; unvisited
        pairs keep their value.  ``r_sum`` ([3][A], e.g. ``actions.table_score``'s): what a pair's transitions earned in all,
        in place of the table's reward sums.  Returns the new Q (float64[3][A], same device)."""
        import torch
        t = table.to(torch.float64)
        n = t[..., 0]
        visited = n > 0
        nn = torch.clamp(n, min=1.0)
        earned = t[..., 1] if r_sum is None else r_sum.to(torch.float64)
        r_mean, cont, p_next = earned / nn, 1.0 - t[..., 6] / nn, t[..., 3:6] / nn.unsqueeze(-1)
        for _ in range(int(sweeps)):
            v = q.max(dim=1).values                            # [3]: the value of each observation class
            q = torch.where(visited, r_mean + gamma * cont * (p_next * v).sum(dim=-1), q)
        return q

    def learn(self, sweeps=1):
        if self.score is None:
            self.q = self.q_iteration(self.q, self.table, self.gamma, sweeps)
        else:
            from .actions import table_score
            self.q = self.q_iteration(self.q, self.table, self.gamma, sweeps, r_sum=table_score(self.table, self.score, self.max_duration))
        return self.q

    def evaluate(self, steps):
        """Mean reward per env-step under the current policy over ``steps`` further steps of all N envs, and its standard
        error: ``(mean, stderr)`` from n, r_sum and r_sq of a table of this call's own (``self.table`` is not touched).
        With a ``score``: ``(mean score per env-step, None)`` -- the table sums scores, not their squares, so it has no
        standard error to give."""
        torch = self.torch
        if self.score is not None:
            from .actions import table_score
            t = self._rollout(steps, torch.zeros_like(self.table))
            return float(table_score(t, self.score, self.max_duration).sum().cpu()) / float(t[..., 0].sum().cpu()), None
        t = self._rollout(steps, torch.zeros_like(self.table)).to(torch.float64)
        n, r_sum, r_sq = (float(x) for x in t[..., :3].sum(dim=(0, 1)).cpu())
        mean = r_sum / n
        return mean, (max(r_sq / n - mean * mean, 0.0) / n) ** 0.5


class PopulationSearchAgent:
    """Cross-entropy search over the ``[3][A]`` logits of a tabular policy, one generation per ``env.rollout_population``
    call: P candidate tables run on ``num_envs / P`` envs each inside one launch per 64 steps and come back as a ``[P][5]``
    episode tally -- nothing is sized by ``steps * num_envs``, and the only host traffic per generation is the tables in and
    the tally out.

    Per generation: P logit tables ``mu + sigma * eps`` from a seeded ``numpy.random.Generator``; softmax in float64 numpy and
    ``actions.policy_cdf`` in numpy (the torch form of ``policy_cdf`` may differ by 1 in an entry; the numpy form is the one a
    CPU oracle can reproduce); ``evaluate(cdfs, generation)`` -> the tally; ``fitness = ret_sum / episodes`` (``-inf`` where a
    policy ended no episode); ``mu`` and ``sigma`` become the mean and standard deviation of the elites' logits, ``sigma``
    floored at ``SIGMA_MIN``.  ``history`` keeps ``{"generation", "fitness", "mean", "best"}`` per generation.

    ``evaluate`` defaults to the env: ``env.reset()``, the episode state zeroed, ``env.rollout_population(cdfs, steps, seed,
    max_steps=episode_steps, step0=generation * steps)``.  Pass a callable (and ``env=None`` with ``nb_actions``) to let
    anything else that returns a ``[P][5]`` tally stand in for the GPU.

    ``score`` (``actions.make_score``) is passed on to ``rollout_population``: the fitness is then the mean episode SCORE --
    with ``make_score(D, reward=0, delivered=1)`` the packets delivered per episode, where the built-in reward's return is 0
    or ``-payload_value`` whatever the policy does and is highest for the policy that assigns nothing.  A caller's own
    ``evaluate`` reads it from ``self.score``."""

    SIGMA_MIN = 1e-3                    # the floor of sigma: a collapsed elite set must not end the search

    def __init__(self, env, num_policies, steps, episode_steps, elite_frac=0.25, sigma0=1.0, seed=0, evaluate=None,
                 nb_actions=None, score=None):
        import numpy as np
        self.np = np
        self.env = env
        if nb_actions is None:
            if env is None:
                raise ValueError("PopulationSearchAgent: without an env, pass nb_actions")
            nb_actions = int(env.num_devices) * int(env.config.max_duration)
        if env is None and evaluate is None:
            raise ValueError("PopulationSearchAgent: without an env, pass evaluate")
        self.nb_actions = int(nb_actions)
        self.num_policies, self.steps, self.episode_steps = int(num_policies), int(steps), int(episode_steps)
        self.num_elites = max(1, int(round(float(elite_frac) * self.num_policies)))
        if self.num_policies < 1 or self.num_elites > self.num_policies:
            raise ValueError("PopulationSearchAgent: need 1 <= elites <= num_policies")
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.mu = np.zeros((3, self.nb_actions), np.float64)
        self.sigma = np.full((3, self.nb_actions), float(sigma0), np.float64)
        self.score = score
        self.evaluate = evaluate if evaluate is not None else self._evaluate_on_env
        self.generation = 0
        self.history = []

    def _evaluate_on_env(self, cdfs, generation):
        env = self.env
        env.reset()
        env.episode_state.zero_()
        kw = {} if self.score is None else {"score": self.score}
        return env.rollout_population(cdfs, self.steps, self.seed, max_steps=self.episode_steps, on_done=True,
                                      step0=generation * self.steps, **kw)

    def tables(self, logits):
        """Logits ``[..., A]`` -> the 32-bit tables the launch reads (numpy): softmax in float64, then ``policy_cdf``."""
        from .actions import policy_cdf
        np = self.np
        z = np.asarray(logits, np.float64)
        z = np.exp(z - z.max(axis=-1, keepdims=True))
        return policy_cdf(z / z.sum(axis=-1, keepdims=True))

    def policy_cdf(self):
        """The table of the current mean logits."""
        return self.tables(self.mu)

    def step(self):
        """One generation; returns its ``history`` entry."""
        np = self.np
        logits = self.mu + self.sigma * self.rng.standard_normal((self.num_policies, 3, self.nb_actions))
        tally = self.evaluate(self.tables(logits), self.generation)
        tally = np.asarray(tally.cpu() if hasattr(tally, "cpu") else tally).astype(np.int64)
        if tally.shape != (self.num_policies, 5):
            raise ValueError("evaluate must return a [%d][5] tally, got %s" % (self.num_policies, tally.shape))
        episodes = tally[:, 0]
        fitness = np.where(episodes > 0, tally[:, 3] / np.maximum(episodes, 1), -np.inf)
        elites = logits[np.argsort(-fitness, kind="stable")[:self.num_elites]]
        self.mu = elites.mean(axis=0)
        self.sigma = np.maximum(elites.std(axis=0), self.SIGMA_MIN)
        ran = fitness[episodes > 0]
        entry = {"generation": self.generation, "fitness": fitness, "mean": float(ran.mean()) if ran.size else float("-inf"),
                 "best": float(fitness.max())}
        self.history.append(entry)
        self.generation += 1
        return entry

    def fit(self, generations):
        for _ in range(int(generations)):
            self.step()
        return self.history


class BacklogSearchAgent:
    """Cross-entropy search over the queue-aware scheduler's policy (``actions.make_backlog_policy``), one generation per
    ``env.rollout_backlog_population`` call: P candidate policies run on ``num_envs / P`` envs each inside one launch per 64
    steps and come back as a ``[P][5]`` episode tally.  The default table, ``min(19, 4 * length)`` with unit weights, is a
    guess; which table delivers most depends on the load, so the baseline is tuned per configuration.

    The genome is real-valued: D weight genes, then one duration gene per knot ``L`` in ``KNOTS``.  A genome's policy: the
    weights rounded and clipped to ``[0, W_MAX]``; the knots interpolated piecewise-linearly over ``L = 0 .. QUEUE_CAP``,
    rounded and clipped to ``[0, max_duration - 1]``.  ``mu`` starts at the default policy (the knots at ``min(4 L,
    max_duration + 4)``, which interpolates and clips to exactly the default table).  Per generation: candidate 0 is ``mu``
    itself, the others ``mu + sigma * eps`` from a seeded ``numpy.random.Generator``; ``evaluate(population, generation)`` ->
    the tally (``population``: ``actions.make_backlog_population``'s image); ``fitness = ret_sum / episodes`` (``-inf`` where
    a policy ended no episode); ``mu`` and ``sigma`` become the mean and standard deviation of the elites' genomes, ``sigma``
    floored at ``SIGMA_MIN``.  ``history`` keeps ``{"generation", "fitness", "mean", "best", "of_mu"}`` per generation.

    ``evaluate`` defaults to the env: a ``snapshot()`` is taken at construction, after ``env.reset()``, and before every
    generation it is ``restore()``d and the episode state zeroed -- a reset leaves the queues alone, so without the restore a
    candidate would inherit the queues its slot's predecessor left, and generations would not be comparable.  Pass a callable
    (and ``env=None`` with ``num_devices``) to let anything else that returns a ``[P][5]`` tally stand in for the GPU.
    ``score`` (``actions.make_score``) is passed on; a caller's own ``evaluate`` reads it from ``self.score``."""

    KNOTS = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 100)
    W_MAX = 16
    SIGMA_MIN = 0.25                    # the floor of sigma: genes are rounded, a collapsed elite set must not end the search

    def __init__(self, env, num_policies, steps, episode_steps, elite_frac=0.25, sigma_weight=1.0, sigma_duration=4.0, seed=0,
                 evaluate=None, num_devices=None, max_duration=None, score=None):
        import numpy as np
        self.np = np
        self.env = env
        if env is None and (evaluate is None or num_devices is None):
            raise ValueError("BacklogSearchAgent: without an env, pass evaluate and num_devices")
        self.num_devices = int(env.num_devices if num_devices is None else num_devices)
        if max_duration is None:
            max_duration = env.MAX_ASSIGN_DURATION if env is not None else 20
        self.max_duration = int(max_duration)
        self.num_policies, self.steps, self.episode_steps = int(num_policies), int(steps), int(episode_steps)
        self.num_elites = max(1, int(round(float(elite_frac) * self.num_policies)))
        if self.num_policies < 1 or self.num_elites > self.num_policies:
            raise ValueError("BacklogSearchAgent: need 1 <= elites <= num_policies")
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        D, knots = self.num_devices, np.asarray(self.KNOTS, np.float64)
        self.mu = np.concatenate([np.ones(D), np.minimum(4.0 * knots, self.max_duration + 4.0)])
        self.sigma = np.concatenate([np.full(D, float(sigma_weight)), np.full(len(knots), float(sigma_duration))])
        self.score = score
        self.evaluate = evaluate if evaluate is not None else self._evaluate_on_env
        self._start = None
        if evaluate is None:
            env.reset()
            self._start = env.snapshot()
        self.generation = 0
        self.history = []

    def _evaluate_on_env(self, population, generation):
        env = self.env
        env.restore(self._start)
        env.episode_state.zero_()
        kw = {} if self.score is None else {"score": self.score}
        return env.rollout_backlog_population(population, self.steps, max_steps=self.episode_steps, on_done=True, **kw)

    def image(self, genome):
        """A genome -> ``make_backlog_policy``'s image."""
        from .actions import make_backlog_policy, QUEUE_CAP
        np = self.np
        g = np.asarray(genome, np.float64)
        D = self.num_devices
        w = np.clip(np.rint(g[:D]), 0, self.W_MAX).astype(np.int64)
        t = np.interp(np.arange(QUEUE_CAP + 1), self.KNOTS, g[D:])
        t = np.clip(np.rint(t), 0, self.max_duration - 1).astype(np.int64)
        return make_backlog_policy(D, w, t, self.max_duration)

    def policy(self):
        """The image of the current mean genome."""
        return self.image(self.mu)

    def step(self):
        """One generation; returns its ``history`` entry."""
        from .actions import make_backlog_population
        np = self.np
        genomes = self.mu + self.sigma * self.rng.standard_normal((self.num_policies, self.mu.size))
        genomes[0] = self.mu
        tally = self.evaluate(make_backlog_population([self.image(g) for g in genomes]), self.generation)
        tally = np.asarray(tally.cpu() if hasattr(tally, "cpu") else tally).astype(np.int64)
        if tally.shape != (self.num_policies, 5):
            raise ValueError("evaluate must return a [%d][5] tally, got %s" % (self.num_policies, tally.shape))
        episodes = tally[:, 0]
        fitness = np.where(episodes > 0, tally[:, 3] / np.maximum(episodes, 1), -np.inf)
        elites = genomes[np.argsort(-fitness, kind="stable")[:self.num_elites]]
        self.mu = elites.mean(axis=0)
        self.sigma = np.maximum(elites.std(axis=0), self.SIGMA_MIN)
        ran = fitness[episodes > 0]
        entry = {"generation": self.generation, "fitness": fitness, "mean": float(ran.mean()) if ran.size else float("-inf"),
                 "best": float(fitness.max()), "of_mu": float(fitness[0])}
        self.history.append(entry)
        self.generation += 1
        return entry

    def fit(self, generations):
        for _ in range(int(generations)):
            self.step()
        return self.history


class ControllerSearchAgent:
    """Cross-entropy search over finite-state controllers (``actions.make_controller``), one generation per
    ``env.rollout_controller_population`` call: P candidate controllers of S nodes run on ``num_envs / P`` envs each inside
    one launch per 64 steps and come back as a ``[P][5]`` episode tally.  A controller sees what an RRM sees -- the
    observation class, what it did (its node) and whether the step it granted delivered enough -- not the queues.

    The genome is real-valued, ``GENES = D + 8`` genes per node: D sender logits, a duration, ``need``, and the six ``next``
    entries (by new observation class and delivered bit).  A genome's controller: node n draws its sender from
    ``softmax(logits)`` for the duration rounded and clipped to ``[0, max_duration - 1]``, the same row for the three classes;
    ``need`` rounded and clipped to ``[0, 255]``; each ``next`` gene rounded and taken modulo S.  ``mu`` starts at
    ``actions.stay_while_productive_controller(D, max_duration - 1, need0)`` spread over S nodes (node n serves sender
    ``n % D`` with logit ``LOGIT0``).  Per generation: candidate 0 is ``mu`` itself, the others ``mu + sigma * eps`` from a
    seeded ``numpy.random.Generator``; ``evaluate(population, generation)`` -> the tally (``population``:
    ``actions.make_controller_population``'s arrays); ``fitness = ret_sum / episodes`` (``-inf`` where a controller ended no
    episode); ``mu`` and ``sigma`` become the mean and standard deviation of the elites' genomes, ``sigma`` floored at
    ``SIGMA_MIN``.  ``history`` keeps ``{"generation", "fitness", "mean", "best", "of_mu"}`` per generation.

    ``evaluate`` defaults to the env, as ``BacklogSearchAgent``'s does: a ``snapshot()`` taken at construction is restored
    before every generation, and the episode state and the nodes are zeroed.  Pass a callable (and ``env=None`` with
    ``num_devices``) to let anything else that returns a ``[P][5]`` tally stand in for the GPU.  ``score``
    (``actions.make_score``) is passed on; the default counts delivered packets."""

    LOGIT0 = 6.0
    SIGMA_MIN = 0.25

    def __init__(self, env, num_policies, steps, episode_steps, num_states=None, need0=8, elite_frac=0.25, sigma_logit=1.0,
                 sigma_duration=2.0, sigma_need=1.5, sigma_next=0.5, seed=0, evaluate=None, num_devices=None, max_duration=None,
                 score=None):
        import numpy as np
        from .actions import FSC_MAX_STATES, make_score
        self.np = np
        self.env = env
        if env is None and (evaluate is None or num_devices is None):
            raise ValueError("ControllerSearchAgent: without an env, pass evaluate and num_devices")
        self.num_devices = D = int(env.num_devices if num_devices is None else num_devices)
        if max_duration is None:
            max_duration = env.MAX_ASSIGN_DURATION if env is not None else 20
        self.max_duration = int(max_duration)
        self.num_states = S = int(D if num_states is None else num_states)
        if not 1 <= S <= FSC_MAX_STATES:
            raise ValueError("ControllerSearchAgent: num_states must be in [1, %d]" % FSC_MAX_STATES)
        self.num_policies, self.steps, self.episode_steps = int(num_policies), int(steps), int(episode_steps)
        self.num_elites = max(1, int(round(float(elite_frac) * self.num_policies)))
        if self.num_policies < 1 or self.num_elites > self.num_policies:
            raise ValueError("ControllerSearchAgent: need 1 <= elites <= num_policies")
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.GENES = D + 8
        mu = np.zeros((S, self.GENES))
        sigma = np.empty((S, self.GENES))
        for n in range(S):
            mu[n, n % D] = self.LOGIT0
            mu[n, D], mu[n, D + 1] = self.max_duration - 1, need0
            mu[n, D + 2:] = [(n + 1) % S, n] * 3                    # by class: {not enough: the next node, enough: stay}
        sigma[:, :D], sigma[:, D], sigma[:, D + 1], sigma[:, D + 2:] = sigma_logit, sigma_duration, sigma_need, sigma_next
        self.mu, self.sigma = mu.ravel(), sigma.ravel()
        self.score = score if score is not None else make_score(D, reward=0, delivered=1)
        self.evaluate = evaluate if evaluate is not None else self._evaluate_on_env
        self._start = self._obs0 = None
        if evaluate is None:
            self._obs0 = env.reset().clone()                        # what every env sees at the snapshot
            self._start = env.snapshot()
        self.generation = 0
        self.history = []

    def _evaluate_on_env(self, population, generation):
        env = self.env
        env.restore(self._start)
        env.episode_state.zero_()
        env.controller_node.zero_()
        return env.rollout_controller_population(population, self.steps, self.seed, max_steps=self.episode_steps, on_done=True,
                                                 step0=generation * self.steps, obs_prev=self._obs0, score=self.score)

    def controller(self, genome=None):
        """A genome (default: the current mean) -> ``make_controller``'s arrays."""
        from .actions import make_controller, policy_cdf
        np = self.np
        D, S, md = self.num_devices, self.num_states, self.max_duration
        g = np.asarray(self.mu if genome is None else genome, np.float64).reshape(S, self.GENES)
        z = g[:, :D] - g[:, :D].max(axis=1, keepdims=True)
        p_sender = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
        dur = np.clip(np.rint(g[:, D]), 0, md - 1).astype(np.int64)
        p = np.zeros((S, 3, D * md))
        for n in range(S):
            p[n, :, np.arange(D) * md + dur[n]] = p_sender[n][:, None]
        need = np.clip(np.rint(g[:, D + 1]), 0, 255).astype(np.int64)
        nxt = (np.rint(g[:, D + 2:]).astype(np.int64) % S).reshape(S, 3, 2)
        return make_controller(D, policy_cdf(p), nxt, need, md)

    def step(self):
        """One generation; returns its ``history`` entry."""
        from .actions import make_controller_population
        np = self.np
        genomes = self.mu + self.sigma * self.rng.standard_normal((self.num_policies, self.mu.size))
        genomes[0] = self.mu
        tally = self.evaluate(make_controller_population([self.controller(g) for g in genomes]), self.generation)
        tally = np.asarray(tally.cpu() if hasattr(tally, "cpu") else tally).astype(np.int64)
        if tally.shape != (self.num_policies, 5):
            raise ValueError("evaluate must return a [%d][5] tally, got %s" % (self.num_policies, tally.shape))
        episodes = tally[:, 0]
        fitness = np.where(episodes > 0, tally[:, 3] / np.maximum(episodes, 1), -np.inf)
        elites = genomes[np.argsort(-fitness, kind="stable")[:self.num_elites]]
        self.mu = elites.mean(axis=0)
        self.sigma = np.maximum(elites.std(axis=0), self.SIGMA_MIN)
        ran = fitness[episodes > 0]
        entry = {"generation": self.generation, "fitness": fitness, "mean": float(ran.mean()) if ran.size else float("-inf"),
                 "best": float(fitness.max()), "of_mu": float(fitness[0])}
        self.history.append(entry)
        self.generation += 1
        return entry

    def fit(self, generations):
        for _ in range(int(generations)):
            self.step()
        return self.history
