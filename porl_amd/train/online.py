"""`train_online` of the Q-learning trainers: the environment loop of src/porl/train/dqn_trainer.py:119-180
(c51_trainer.py:176-225, dqn_per_trainer.py:127-175 differ only in the action rule, the memory and the learn threshold),
statement for statement — the same env protocol (reset -> (state, info), step -> 5 values, done = done or truncated), the
same order of draws from the global numpy stream (epsilon draw, randint when exploring, np.random.choice inside the
sample), the same logger calls with the same values, per-episode epsilon decay and target sync.

Fast path (`_Fast`), taken when the network lives on a QnetEngine and the memory is the device-mirrored ReplayBuffer:
  * greedy action: porl_qnet_act — one launch on the state just recorded (a slot of the mirror's next_states) or, right
    after env.reset(), on the state carried in the kernel's arguments; the action comes back in a pinned record, read
    after one stream synchronisation;
  * push: ReplayBuffer.record — one launch writes the row into the mirror (no _sync_mirror before the next sample);
  * learn (plain / Double / dueling DQN and CQL on the one-launch step kernel): the sampled rows are gathered inside the
    step kernel (learn_indexed); the only host->device copy is the minibatch's indices.  The loss is not read back at
    once: the act record carries the statistics of the step before it, and losses of steps followed by an exploring
    step are parked in a device log, read at the next greedy action or the episode's end.  The logger calls are
    replayed then, in their original order.
  * learn (C51 / QR-DQN, whose A x N outputs the step kernel does not cover): the same index ring and deferred loss
    around DistTrainerBase._learn_rows — one native call (porl_qnet_dist_learn) that gathers the rows, runs the
    forwards as one grouped launch per layer, the loss head on the padded output rows, backward and Adam, and leaves the
    mean loss in the engine's statistics.
PER flavour (`_FastPER`, PERTrainer on the one-launch step kernel; dqn_per_trainer.py:127-175): the memory is the
device-resident PrioritizedReplayBuffer, so
  * push: PrioritizedReplayBuffer.record — one launch writes the row and the leaf (max_initial_priority) and
    recomputes the leaf's ancestors; the greedy action reads the row of the store's next_states just recorded;
  * learn: sample_slots (one copy of the batch's uniforms, drawn from Python's `random` exactly as the reference draws
    them, one launch for tree walk, weights and their mean) -> the step kernel on rows `slots` (Double-DQN, importance
    weights or their mean, |TD| out) -> update_priorities_device (one launch); losses deferred as above.
BCQ flavour (`_FastBCQ`, BCQTrainer.train_online(policy=bcq_learn)): the same ring and deferred loss around
porl_qnet_bcq_learn — the behaviour mask computed from the replay rows by one kernel, then the step kernel with the
masked bootstrap action, reduction and Adam, all from one native call.
IQN flavour (`_FastIQN`, IQNTrainer; the reference's scripts/train_iqn.py drives exactly this loop): the network is not
an MLP a QnetEngine covers, so the trainer's own IqnEngine (csrc/iqn_api.inc) stands in for it:
  * greedy action: the fractions are drawn as select_action draws them (torch.rand(1, N_policy) on the device), then
    porl_iqn_act — feature net on the one state, mix kernel, value layer, act head — writes the same pinned record;
  * push: ReplayBuffer.record, as above;
  * learn: the index ring and deferred loss around IQNTrainer._learn_rows — tau' and tau'' drawn as learn() draws them,
    then one native call (porl_iqn_learn): gather, the three forwards grouped per layer, loss head, backward into the
    flat gradient buffer, clip, Adam; mean loss, gradient norm and clip coefficient in the engine's statistics.
Everything else (user `policy` callables, subclasses that override learn / learn_on / select_action, networks too large
for one workgroup) runs the reference loop on the trainer's own select_action / push / learn.

Nothing here makes a ctypes call: the engines of porl_amd/engine.py (the one ctypes layer) do, and they check the replay
arrays (engine.replay_args).  The three `fast_*_ok` tests share `_rows_fit` (memory class, device, row width); `_Fast`
knows which engine `record` writes through and how an act record is read (`_read_action`), so the flavours only override
what differs.  Learn steps advance the Adam step number after their native call (cql_trainer._FlatAdam.hyper).
`run_offline` is train_offline of the CQL family and of IQNTrainer.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from ..buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
from ..buffer.replay_buffer import ReplayBuffer
from ..engine import IqnEngine, QnetEngine, _norm_device
from ..net.iqn_network import IQNNetwork


class _Fast:
    def __init__(self, trainer, kind=0, n_sub=1, support=None, learn_rows=None, memory=None, engine=None):
        self.t, self.eng = trainer, trainer._engine if engine is None else engine
        self.rec_eng = getattr(trainer, "_engine", None)     # the QnetEngine `record` writes through (None: the buffer's own)
        self.rb = trainer.replay_buffer if memory is None else memory
        self.kind, self.n_sub, self.support = kind, n_sub, support
        self.n_act = trainer.action_size
        self.learn_rows = learn_rows               # None: the trainer's own learn()
        self.S = int(np.prod(self.rb.state_shape))
        self.rec = torch.zeros(16, dtype=torch.int32).pin_memory()
        self.rec_f = self.rec.view(torch.float32)
        self.stream = torch.cuda.current_stream(self.eng.device)
        self.state_row = None                      # mirror row holding the current state (None: pass it inline)
        # deferred losses
        self.calls = []                            # (method, args, loss slot or None)
        self.log = None                            # device losses of learn steps followed by an exploring step
        self.parked = []                           # their loss slots, in log order
        self.in_stats = None                       # loss slot of the newest learn, its value still only in eng.stats
        self.values = []                           # loss per slot (None until read)
        self._make_ring()

    def _make_ring(self):
        trainer = self.t
        # minibatch indices: pinned staging ring; a slot is rewritten only after its copy has completed
        self.R = 32
        B = trainer.batch_size
        self.idx_host = torch.zeros(self.R, B, dtype=torch.int64).pin_memory()
        self.idx_dev = torch.zeros(self.R, B, dtype=torch.int64, device=self.eng.device)
        self.idx_ev = [None] * self.R
        self.idx_k = 0

    # -- acting / recording -------------------------------------------------------------------------------------------
    def greedy(self, state):
        eng = self.eng
        n_stats = 1 if self.in_stats is not None else 0
        kw = dict(kind=self.kind, n_act=self.n_act, n_sub=self.n_sub, support=self.support, n_stats=n_stats)
        if self.state_row is not None:
            eng.act(self.rec, states=self._next_states(), row=self.state_row, **kw)
        else:
            eng.act(self.rec, inline=np.asarray(state, dtype=np.float32).reshape(-1), **kw)
        return self._read_action(n_stats)

    def _read_action(self, n_stats):
        """Wait for the act record just launched: the action, and with it (n_stats) the newest learn step's loss."""
        self.stream.synchronize()
        if n_stats:
            self.resolve(float(self.rec_f[8]))
        return int(self.rec[0])

    def _next_states(self):
        return self.rb._mirror["next_states"]

    def explore(self):
        """An exploring step: park the newest loss (if any) before the next learn overwrites the statistics."""
        if self.in_stats is not None:
            n = len(self.parked)
            self.log[n:n + 1].copy_(self.eng.stats[:1])
            self.parked.append(self.in_stats)
            self.in_stats = None

    def push(self, state, action, reward, next_state, done):
        p = self.rb.position
        self.state_row = p if self.rb.record(state, action, reward, next_state, done, engine=self.rec_eng) else None

    # -- learning -----------------------------------------------------------------------------------------------------
    def learn(self):
        t = self.t
        if self.learn_rows is None:
            return t.learn()
        idx = np.random.choice(self.rb.size, t.batch_size, replace=False)       # ReplayBuffer.sample's draw
        self.rb._sync_mirror()
        k = self.idx_k
        self.idx_k = (k + 1) % self.R
        if self.idx_ev[k] is not None:
            self.idx_ev[k].synchronize()
        else:
            self.idx_ev[k] = torch.cuda.Event()
        self.idx_host[k].numpy()[:] = idx
        d = self.idx_dev[k]
        d.copy_(self.idx_host[k], non_blocking=True)
        self.idx_ev[k].record(self.stream)
        self.learn_rows(d)
        return self._deferred_loss()

    def _deferred_loss(self):
        """The loss of the step just launched: the device statistics (async_losses) or a slot to be filled later."""
        if self.t.async_losses:
            return self.eng.stats[:3]
        if self.log is None:
            self.log = torch.zeros(self.max_steps + 1, dtype=torch.float32, device=self.eng.device)
        self.values.append(None)
        self.in_stats = len(self.values) - 1
        return _Loss(len(self.values) - 1)

    def resolve(self, newest=None):
        """Read every outstanding loss (one readback at most) and replay the queued logger calls.  `newest`: the value
        of the newest learn step's loss, already on the host (from the act record)."""
        if newest is not None:
            self.values[self.in_stats] = newest
            self.in_stats = None
        self.explore()
        if self.parked:
            for i, v in zip(self.parked, self.log[:len(self.parked)].tolist()):
                self.values[i] = v
        for fn, args in self.calls:
            fn(*[self.values[a.i] if isinstance(a, _Loss) else a for a in args])
        self.calls, self.values, self.parked = [], [], []

    def log_call(self, fn, *args):
        if self.calls or any(isinstance(a, _Loss) for a in args):
            self.calls.append((fn, args))
        else:
            fn(*args)


class _FastPER(_Fast):
    """PERTrainer: the memory is the PrioritizedReplayBuffer; push = record, learn = sample_slots -> step kernel on the
    store's rows -> fused priority write-back (PERTrainer.learn's arithmetic, launch for launch on the step kernel)."""

    def __init__(self, trainer):
        super().__init__(trainer, memory=trainer.memory)
        self.views = None

    def _make_ring(self):
        pass                                       # no index ring: the slots are drawn on the device (sample_slots)

    def _next_states(self):
        return self.rb._store["next_states"]

    def push(self, state, action, reward, next_state, done):
        p = self.rb.data_pointer
        ok = self.rb.record(self.t.max_initial_priority, state, action, reward, next_state, done)
        self.state_row = p if ok else None

    def learn(self):
        t, mem, eng = self.t, self.rb, self.eng
        B = t.batch_size
        slots, is_w, wmean, tree_idx = mem.sample_slots(B)
        if self.views is None:
            st = mem._store
            self.views = (st["states"], st["actions"], st["rewards"].view(-1), st["next_states"], st["dones"].view(-1))
        hp = t.optimizer.hyper(t.gamma, 0.0, 1.0 / B)
        td_abs = t._td_abs[:B]
        if t.per_sample_weights:
            var = N.QnetVariant(1, is_w.data_ptr(), None, td_abs.data_ptr())
        else:
            var = N.QnetVariant(1, None, wmean.data_ptr(), td_abs.data_ptr())
        eng.learn_indexed(hp, *self.views, slots, variant=var)
        t.optimizer.step_count = hp.step
        mem.update_priorities_device(tree_idx, td_abs)
        return self._deferred_loss()


class _FastBCQ(_Fast):
    """BCQTrainer with policy=bcq_learn: act and record as _Fast; learn = numpy's draw through the index ring into
    policy.bcq.bcq_learn_rows' launch (porl_qnet_bcq_learn: behaviour mask from the rows, masked-argmax step, Adam)."""

    def __init__(self, trainer):
        from ..policy.bcq import _launch_rows
        super().__init__(trainer, learn_rows=lambda idx: _launch_rows(trainer, idx))


class _FastIQN(_Fast):
    """IQNTrainer: act and learn on the trainer's IqnEngine; ring, record and deferred losses as _Fast."""

    def __init__(self, trainer):
        super().__init__(trainer, learn_rows=trainer._learn_rows, engine=trainer._native_engine())

    def greedy(self, state):
        n_stats = 1 if self.in_stats is not None else 0
        self.t._act(self.rec, state=state if self.state_row is None else None, row=self.state_row, n_stats=n_stats,
                    array="next_states")
        return self._read_action(n_stats)

    def learn(self):
        self.eng = self.t._native_engine()         # (the same engine unless a larger one had to be made)
        return super().learn()


class _Loss:
    __slots__ = ("i",)

    def __init__(self, i):
        self.i = i


def run(trainer, env, policy, num_episodes, max_steps, threshold, memory, push, fast=None):
    """dqn_trainer.py:119-180 with `memory` / `push` / the learn threshold of the trainer at hand; `fast` replaces the
    action rule, push and learn by the one-launch forms (loop semantics unchanged)."""
    t = trainer
    if fast is not None:
        fast.max_steps = max_steps
        push = fast.push
    rewards_history = []
    for episode in range(num_episodes):
        state, _ = env.reset()
        episode_reward = 0
        if fast is not None:
            fast.state_row = None
        for step in range(max_steps):
            if fast is None:
                action = t.select_action(state)
            elif np.random.rand() < t.epsilon:
                fast.explore()
                action = np.random.randint(t.action_size)
            else:
                action = fast.greedy(state)
            next_state, reward, done, truncated, _ = env.step(action)
            done = done or truncated

            push(state, action, reward, next_state, done)
            state = next_state
            episode_reward += reward

            log = t.logger.log_step if fast is None else (lambda *a: fast.log_call(t.logger.log_step, *a))
            log(episode, step, reward, None, t.epsilon)

            if len(memory) >= threshold:
                if policy is None:
                    loss = t.learn() if fast is None else fast.learn()
                else:
                    loss = policy()
                if t.logger is not None:
                    log(episode, step, reward, loss, t.epsilon)

            if done:
                break

        if fast is not None:
            fast.resolve()
        t.epsilon = max(t.epsilon_min, t.epsilon * t.epsilon_decay)
        if episode % t.update_target_freq == 0:
            t.sync_target()

        t.logger.log_episode(episode)
        rewards_history.append(episode_reward)

        if episode % 10 == 0:
            print(f"Episode {episode}, Reward: {episode_reward:.2f}, Epsilon: {t.epsilon:.3f}")

    env.close()
    t.logger.close()
    return rewards_history


def run_offline(trainer, policy=None, num_iterations: int = 10000):
    """dqn_trainer.py:182-204: `num_iterations` learn steps (or calls of `policy`), each loss logged, the target network
    synchronised every update_target_freq steps (dqn_trainer.py:195-196)."""
    t = trainer
    losses = []
    for t.training_step in range(num_iterations):
        loss = t.learn() if policy is None else policy()
        t.logger.log_loss(t.training_step, loss)
        if t.training_step % t.update_target_freq == 0:
            t.sync_target()
        losses.append(loss)
    t.logger.close()
    return losses


def _rows_fit(memory, cls, device, S, max_inline):
    """What the fast paths ask of the memory: exactly `cls`, on the HIP device `device`, its rows the network's S floats
    and within what the record kernel and an inline act launch carry in their arguments."""
    device = _norm_device(device)
    return device.type == "cuda" and type(memory) is cls and _norm_device(memory.device) == device and \
        memory.state_shape is not None and int(np.prod(memory.state_shape)) == S and \
        S <= QnetEngine.RECORD_MAX_STATE and S <= max_inline


def fast_per_ok(trainer):
    """The one-launch PER path applies: the trainer's own learn() on the one-launch step kernel, a network the act
    kernel covers, a device PrioritizedReplayBuffer whose rows fit the record kernel, no gradient exchange."""
    eng = getattr(trainer, "_engine", None)
    if eng is None or not _rows_fit(trainer.memory, PrioritizedReplayBuffer, eng.device, eng.cfg.state_dim,
                                    eng.ACT_MAX_INLINE) or \
            trainer._exchange.active or trainer.batch_size > trainer._td_abs.numel():
        return False
    eng._ensure_bound()
    return eng.fused and eng.act_ok


def fast_ok(trainer):
    """The one-launch path applies: a QnetEngine on a HIP device behind a device-mirrored ReplayBuffer whose rows fit
    the record kernel, and a network the act kernel covers."""
    eng = getattr(trainer, "_engine", None)
    if eng is None or not _rows_fit(trainer.replay_buffer, ReplayBuffer, eng.device, eng.cfg.state_dim, eng.ACT_MAX_INLINE):
        return False
    eng._ensure_bound()
    return eng.act_ok


def fast_iqn_ok(trainer):
    """The native IQN path applies: a HIP device, the device-mirrored ReplayBuffer with rows that fit the record and
    inline limits, both networks exactly IQNNetwork on the trainer's flat buffers, learn / learn_on / select_action not
    overridden, sizes within the engine's limits."""
    from .iqn_trainer import IQNTrainer
    t = trainer
    if not _rows_fit(t.replay_buffer, ReplayBuffer, t.device, t.state_size, IqnEngine.ACT_MAX_INLINE):
        return False
    if type(t.q_network) is not IQNNetwork or type(t.target_network) is not IQNNetwork:
        return False
    cls = type(t)
    if cls.learn is not IQNTrainer.learn or cls.learn_on is not IQNTrainer.learn_on or \
            cls.select_action is not IQNTrainer.select_action:
        return False
    q = t.q_network
    if q.embedding_dim != t.embedding_dim or q.embedding_dim > IqnEngine.MAX_EMBED or t.action_size > IqnEngine.MAX_ACTIONS or \
            max(t.num_quantiles_n_policy, t.num_quantiles_n_prime_loss, t.num_quantiles_n_double_prime_loss) > IqnEngine.MAX_TAU:
        return False
    return t._views_intact()
