"""The ctypes layer over libporl_hip.so's three engines on one MI355X: IqlEngine (POR / SORL), QnetEngine (the
Q-learning trainers' MLPs) and IqnEngine.  Every native call on an engine handle is a method of its class here;
`replay_args` is the one check of device-resident replay arrays in front of the row-sourced steps.

PyTorch supplies device memory and the stream; all arithmetic of the step runs in libporl_hip.so
(porl_amd/_native.py).  Parameters, gradients and Adam moments each live in ONE flat fp32 tensor per
optimizer group so the Adam(+EMA) sweep and the data-parallel all-reduce are single operations; the
nn.Parameters of the agent modules are views into those tensors.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N


def _norm_device(device):
    """torch.device('cuda') and torch.device('cuda:0') must compare equal for the checks below."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class IqlEngine:
    GROUP_VF, GROUP_POL = 0, 1
    MODE_TWO_SLOTS, MODE_FOLD_COMBINE, MODE_SHORT_BLOCKS = 1, 2, 4     # include/porl_hip.h: PORL_IQL_MODE_*
    SLOTS = 3                                         # PORL_IQL_SLOTS: copies of the minibatch staging buffers

    def __init__(self, obs_dim, pol_out_dim, hidden_dim, n_hidden, layer_norm=False, pol_tanh=False,
                 weight_mode=0, max_batch=1024, device="cpu"):
        self.device = _norm_device(device)
        self.cfg = N.IqlCfg(int(obs_dim), int(pol_out_dim), int(hidden_dim), int(n_hidden),
                            int(bool(layer_norm)), int(bool(pol_tanh)), int(weight_mode), int(max_batch))
        self._lib = N.lib()
        h = C.c_void_p()
        N.check(self._lib.porl_iql_create(C.byref(self.cfg), C.byref(h)), "porl_iql_create")
        self._h = h
        self.n_vf = int(self._lib.porl_iql_group_floats(h, 0))
        self.n_pol = int(self._lib.porl_iql_group_floats(h, 1))
        self._bound = False
        self._mode = 0
        # pipelined updates (agent/_iql.py): the policy phase of update t runs on `side_stream` while the value phase
        # of update t+1 runs on the caller's stream; `_policy_done` is the event the side stream recorded last
        self._side = None
        self._policy_done = None
        self._values_read = None
        self._slot_users = [None] * self.SLOTS         # policy-done events of the last SLOTS pipelined updates, oldest first
        self._events = []
        self._alloc()

    # -- streams -----------------------------------------------------------------------------------
    def side_stream(self):
        if self._side is None:
            import os
            self._side = torch.cuda.Stream(device=self.device, priority=int(os.environ.get("PORL_SIDE_PRIORITY", "0")))
        return self._side

    def event(self, i):
        """Small ring of reusable events (re-recording an event does not disturb waits already enqueued on it)."""
        while len(self._events) <= i:
            self._events.append(torch.cuda.Event(enable_timing=False, blocking=False))
        return self._events[i]

    # Cross-stream ordering of the pipelined update by counters in signal memory (csrc: porl_signal_*).  Three counters:
    # 0 = value Adam done (update number), 1 = policy forward half done, 2 = policy phase done (written and waited for
    # only under PORL_PIPE_SYNC=signal; the default, signal2, relies on the in-order side stream for slot reuse).
    # PORL_PIPE_SYNC=event keeps the event record / stream-wait-event pairs (A/B).
    SIG_VALUE, SIG_FWD, SIG_POLICY = 0, 1, 2

    def signals(self):
        """The three counters, or None when the device has no stream wait-value operations (events are used then)."""
        if getattr(self, "_signals", None) is None:
            sig = []
            with torch.cuda.device(self.device):
                for _ in range(3):
                    p = C.c_void_p()
                    if self._lib.porl_signal_create(C.byref(p)) != 0:
                        sig = False
                        break
                    sig.append(p)
            self._signals = sig
            self._seq = 0
        return self._signals or None

    def signal(self, which, value, stream):
        N.check(self._lib.porl_signal_write(self.signals()[which], int(value), C.c_void_p(stream.cuda_stream)), "porl_signal_write")

    def wait_signal(self, which, value, stream):
        if value > 0:
            N.check(self._lib.porl_signal_wait_ge(self.signals()[which], int(value), C.c_void_p(stream.cuda_stream)),
                    "porl_signal_wait_ge")

    def join(self):
        """Order the current stream behind an outstanding policy phase on the side stream (no host wait)."""
        ev, self._policy_done, self._values_read = self._policy_done, None, None
        self._slot_users = [None] * self.SLOTS
        if ev is True:                                 # signal mode: no per-update event; order behind the side stream now
            ev = self.event(3 * self.SLOTS)
            ev.record(self.side_stream())
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def wait_slot_free(self):
        """The staging slots rotate: the slot the next load writes was last read by the policy phase SLOTS pipelined
        updates ago, i.e. the oldest of the SLOTS events kept here (practically always complete already)."""
        ev = self._slot_users[0]
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def wait_values_read(self):
        """Order the current stream behind the forward half of the outstanding policy phase: after it the value
        parameters may be overwritten (the rest of that phase only touches policy state and its own scratch)."""
        ev, self._values_read = self._values_read, None
        if isinstance(ev, tuple):                      # signal mode: ("sig", update number of that policy phase)
            self.wait_signal(self.SIG_FWD, ev[1], torch.cuda.current_stream(self.device))
        elif ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def set_mode(self, mode):
        if mode != self._mode:
            N.check(self._lib.porl_iql_set_mode(self._h, int(mode)), "porl_iql_set_mode")
            self._mode = mode

    def tune_set(self, key, value):
        """porl_tune_set for this engine only (it copied the process defaults when it was created)."""
        N.check(self._lib.porl_iql_tune_set(self._h, key.encode(), int(value)), "porl_iql_tune_set")

    ADAM_PLAN = ("regions", "fold32", "fold4", "unfolded", "skips", "reduce_blocks")

    def adam_plan(self, group):
        """How the last Adam launch of `group` dealt with the combine jobs handed to it (porl_iql_adam_plan): jobs summed
        inside the sweep, folded as reduce+Adam blocks at width 32 / 4, left as plain reduce blocks (loss statistics),
        ranges the sweep skips, reduce blocks.  Read-only; synchronises nothing."""
        out = (C.c_int32 * 6)()
        N.check(self._lib.porl_iql_adam_plan(self._h, int(group), C.byref(out)), "porl_iql_adam_plan")
        return dict(zip(self.ADAM_PLAN, out))

    # -- memory ------------------------------------------------------------------------------------
    # Flat groups are allocated a little longer than the C library needs (zero tail) so that they split into equal,
    # 16-byte-aligned slices for every data-parallel world size that divides 840 (1..8, 10, 12, ...): the
    # reduce-scatter / sharded Adam / all-gather exchange (agent/_iql.py) works on those slices.
    SLICE_QUANTUM = 4 * 840

    def _alloc(self):
        dev = self.device
        q = self.SLICE_QUANTUM
        z = lambda n: torch.zeros((n + q - 1) // q * q, dtype=torch.float32, device=dev)
        self.params_vf, self.params_tgt, self.params_pol = z(self.n_vf), z(self.n_vf), z(self.n_pol)
        self.grads_vf, self.grads_pol = z(self.n_vf), z(self.n_pol)
        self.adam_m_vf, self.adam_v_vf = z(self.n_vf), z(self.n_vf)
        self.adam_m_pol, self.adam_v_pol = z(self.n_pol), z(self.n_pol)
        self.stats = z(8)
        self.workspace = None
        self._bound = False

    def _ensure_bound(self):
        if self.device.type != "cuda":
            raise N.NativeError("porl_amd computes on a HIP device only (device='cuda'); there is no CPU path")
        if self._bound:
            return
        nws = int(self._lib.porl_iql_workspace_floats(self._h))
        self.workspace = torch.empty(nws, dtype=torch.float32, device=self.device)
        b = N.IqlBuffers(*[C.c_void_p(t.data_ptr()) for t in (
            self.params_vf, self.params_tgt, self.params_pol, self.grads_vf, self.grads_pol,
            self.adam_m_vf, self.adam_v_vf, self.adam_m_pol, self.adam_v_pol, self.workspace, self.stats)])
        N.check(self._lib.porl_iql_bind(self._h, C.byref(b)), "porl_iql_bind")
        self._bound = True
        self._mode = 0
        N.check(self._lib.porl_iql_set_mode(self._h, 0), "porl_iql_set_mode")

    def to(self, device):
        """Move every flat tensor; views handed out earlier must be re-created by the caller."""
        device = _norm_device(device)
        if device == self.device:
            return self
        if self.device.type == "cuda":                 # an engine still on the CPU has no streams, events or signals
            self.join()
            torch.cuda.synchronize(self.device)
            self._free_signals()
        self._side, self._events = None, []
        self._policy_done = self._values_read = None
        for name in ("params_vf", "params_tgt", "params_pol", "grads_vf", "grads_pol", "adam_m_vf",
                     "adam_v_vf", "adam_m_pol", "adam_v_pol", "stats"):
            setattr(self, name, getattr(self, name).to(device))
        self.device = device
        self.workspace = None
        self._bound = False
        return self

    def tensor_table(self, group):
        """[(offset, shape)] of a group's tensors in named_parameters() order."""
        n = int(self._lib.porl_iql_group_tensors(self._h, group))
        out = []
        off, r, c = C.c_int64(), C.c_int32(), C.c_int32()
        for i in range(n):
            N.check(self._lib.porl_iql_tensor_info(self._h, group, i, C.byref(off), C.byref(r), C.byref(c)))
            out.append((off.value, (c.value,) if r.value == 0 else (r.value, c.value)))
        return out

    @staticmethod
    def views(flat, table):
        return [flat[o:o + math.prod(shape)].view(shape) for o, shape in table]

    # -- step --------------------------------------------------------------------------------------
    @staticmethod
    def _mat(t, cols, what):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what}: expected float32, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != cols:
            raise RuntimeError(f"{what}: expected shape (B, {cols}), got {tuple(t.shape)}")
        if t.stride(1) != 1:
            t = t.contiguous()
        return t

    def _vec(self, t, B, what):
        if t.dim() != 1 or t.shape[0] != B:
            raise RuntimeError(f"{what}: expected shape ({B},), got {tuple(t.shape)}")
        return t if t.dtype == torch.float32 else t.float()

    def load_batch(self, obs, next_obs, rew, term, pol_target=None):
        self._ensure_bound()
        for t in (obs, next_obs, rew, term, pol_target):
            if t is not None and t.device != self.device:
                raise RuntimeError(f"batch tensor on {t.device}, engine on {self.device}")
        S, D = self.cfg.obs_dim, self.cfg.pol_out_dim
        obs, next_obs = self._mat(obs, S, "observations"), self._mat(next_obs, S, "next_observations")
        B = obs.shape[0]
        if next_obs.shape[0] != B:
            raise RuntimeError("observations / next_observations batch mismatch")
        if B > self.cfg.max_batch:
            raise RuntimeError(f"batch {B} exceeds engine max_batch {self.cfg.max_batch}")
        rew, term = self._vec(rew, B, "rewards"), self._vec(term, B, "terminals")
        if pol_target is not None:
            pol_target = self._mat(pol_target, D, "policy target")
        # keep references alive until the pack kernel has run (stream-ordered; torch caches the memory)
        self._held = (obs, next_obs, rew, term, pol_target)
        N.check(self._lib.porl_iql_load_batch(
            self._h, B, N.ptr(obs), obs.stride(0), N.ptr(next_obs), next_obs.stride(0),
            N.ptr(rew), rew.stride(0), N.ptr(term), term.stride(0),
            N.ptr(pol_target), 0 if pol_target is None else pol_target.stride(0),
            N.current_stream_ptr(self.device)), "porl_iql_load_batch")
        self.last_batch = B
        return B

    def load_batch_sampled(self, rows, batch, seed, step, act_dim, target_is_action, idx_out=None):
        """Draw `batch` distinct rows of a device-resident packed-row store and stage them (one kernel)."""
        self._ensure_bound()
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1:
            raise RuntimeError("replay rows must be a 2-D fp32 tensor on the engine's device")
        N.check(self._lib.porl_iql_load_batch_sampled(
            self._h, batch, N.ptr(rows), rows.stride(0), rows.shape[0], act_dim, int(target_is_action),
            seed & 0xFFFFFFFFFFFFFFFF, step, N.ptr(idx_out), N.current_stream_ptr(self.device)), "porl_iql_load_batch_sampled")
        self.last_batch = batch
        return batch

    def load_batch_indexed(self, rows, idx, state_dim, act_dim, target_is_action, obs_feat=None, next_feat=None,
                           clamp_target_gt8=False):
        """Stage rows `idx` (int64, on the device) of a packed-row store [s | r | s' | d | a] (one kernel, the store is
        only read): rewards, terminals and the policy target from the rows, observations from the rows too, or from
        the (B, obs_dim) feature matrices `obs_feat` / `next_feat` an encoder made of them.  Index range is the caller's
        contract, as for `gather_rows`."""
        self._ensure_bound()
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1:
            raise RuntimeError("replay rows must be a 2-D fp32 tensor on the engine's device")
        if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != self.device:
            raise RuntimeError(f"indices: expected a contiguous 1-D int64 tensor on {self.device}, got {idx.dtype} "
                               f"{tuple(idx.shape)} on {idx.device}")
        B = idx.numel()
        if B > self.cfg.max_batch:
            raise RuntimeError(f"batch {B} exceeds engine max_batch {self.cfg.max_batch}")
        if (obs_feat is None) != (next_feat is None):
            raise RuntimeError("obs_feat and next_feat must be given together")
        if obs_feat is not None:
            for t in (obs_feat, next_feat):
                if t.device != self.device:
                    raise RuntimeError(f"feature tensor on {t.device}, engine on {self.device}")
            obs_feat, next_feat = self._mat(obs_feat, self.cfg.obs_dim, "features"), self._mat(next_feat, self.cfg.obs_dim, "next features")
            if obs_feat.shape[0] != B or next_feat.shape[0] != B:
                raise RuntimeError(f"features: expected {B} rows, got {obs_feat.shape[0]} and {next_feat.shape[0]}")
        # keep references alive until the load kernel has run (stream-ordered; torch caches the memory)
        self._held = (idx, obs_feat, next_feat)
        N.check(self._lib.porl_iql_load_batch_indexed(
            self._h, B, N.ptr(rows), rows.stride(0), rows.shape[0], N.ptr(idx), int(state_dim), int(act_dim),
            int(bool(target_is_action)), int(bool(clamp_target_gt8)), N.ptr(obs_feat),
            0 if obs_feat is None else obs_feat.stride(0), N.ptr(next_feat), 0 if next_feat is None else next_feat.stride(0),
            N.current_stream_ptr(self.device)), "porl_iql_load_batch_indexed")
        self.last_batch = B
        return B

    # -- goal-conditioned behaviour cloning (porl_iql_load_batch_cat / _pairs, porl_iql_bc_*) -------
    def load_batch_cat(self, obs, goals, actions):
        """Stage [obs | goals] as the policy's input, `actions` as its regression target and unit weights (one kernel,
        no concatenated tensor).  obs (B, obs_dim - G), goals (B, G), actions (B, pol_out_dim): fp32 device tensors,
        strided views with unit column stride are read in place."""
        self._ensure_bound()
        for t, what in ((obs, "observations"), (goals, "goals"), (actions, "actions")):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise RuntimeError(f"{what}: expected a 2-D tensor, got {getattr(t, 'shape', type(t))}")
            if t.device != self.device:
                raise RuntimeError(f"{what} on {t.device}, engine on {self.device}")
        G = int(goals.shape[1])
        S, A = self.cfg.obs_dim - G, self.cfg.pol_out_dim
        if G < 1 or S < 1:
            raise RuntimeError(f"goals: {G} columns do not fit the engine's {self.cfg.obs_dim}-wide [obs | goal] input")
        obs, goals, actions = self._mat(obs, S, "observations"), self._mat(goals, G, "goals"), self._mat(actions, A, "actions")
        B = obs.shape[0]
        if goals.shape[0] != B or actions.shape[0] != B:
            raise RuntimeError(f"observations / goals / actions batch mismatch: {B}, {goals.shape[0]}, {actions.shape[0]}")
        if not 1 <= B <= self.cfg.max_batch:
            raise RuntimeError(f"batch {B} outside [1, {self.cfg.max_batch}] (max_batch)")
        # keep references alive until the staging kernel has run (stream-ordered; torch caches the memory)
        self._held = (obs, goals, actions)
        N.check(self._lib.porl_iql_load_batch_cat(
            self._h, B, N.ptr(obs), obs.stride(0), N.ptr(goals), goals.stride(0), G, N.ptr(actions), actions.stride(0),
            N.current_stream_ptr(self.device)), "porl_iql_load_batch_cat")
        self.last_batch = B
        return B

    def _index_vec(self, t, B, what):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.device != self.device:
            raise RuntimeError(f"{what}: expected a contiguous 1-D int64 tensor on {self.device}, got "
                               f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
        if t.numel() != B:
            raise RuntimeError(f"{what}: expected {B} entries, got {t.numel()}")
        return t

    def load_batch_pairs(self, rows, batch, state_dim, act_dim, goal_col, goal_dim, start=None, goal=None, episodes=None,
                         seed=0, step=0, start_out=None, goal_out=None):
        """Stage `batch` (state, goal, action) samples of a packed-row store [s | r | s' | d | a] (one kernel, the store is
        only read): s and a from row `start`, columns [goal_col, goal_col + goal_dim) from row `goal`.  `start` / `goal`
        (int64 device tensors) name the rows (`goal` None: the start row); without `start` the rows are drawn in the
        kernel — hindsight pairs of `episodes` (an EpisodeIndex) keyed by (seed, step) as `hindsight_indices` draws them,
        or, without a table, distinct rows as `load_batch_sampled` draws them.  `start_out` / `goal_out` receive the rows
        used.  A given row number outside the store stages NaN (the loss says so); nothing is read there."""
        self._ensure_bound()
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1:
            raise RuntimeError("replay rows must be a 2-D fp32 tensor on the engine's device")
        batch = int(batch)
        if not 1 <= batch <= self.cfg.max_batch:
            raise RuntimeError(f"batch {batch} outside [1, {self.cfg.max_batch}] (max_batch)")
        start, goal = self._index_vec(start, batch, "start"), self._index_vec(goal, batch, "goal")
        start_out, goal_out = self._index_vec(start_out, batch, "start_out"), self._index_vec(goal_out, batch, "goal_out")
        if goal is not None and start is None:
            raise RuntimeError("goal rows are given without start rows")
        ep_s = ep_l = None
        n_ep = 0
        if episodes is not None:
            if start is not None:
                raise RuntimeError("an episode table and start rows are both given: the pairs are drawn or named, not both")
            if episodes.n_episodes < 1:
                raise IndexError("load_batch_pairs: the dataset has no closed episode")
            ep_s, ep_l, n_ep = episodes.starts, episodes.lengths, episodes.n_episodes
            for t, what in ((ep_s, "episode starts"), (ep_l, "episode lengths")):
                self._index_vec(t, n_ep, what)
        n = rows.shape[0]
        stride = rows.stride(0) if n > 1 else max(rows.stride(0), rows.shape[1])
        mask = 0xFFFFFFFFFFFFFFFF
        self._held = (start, goal, ep_s, ep_l)
        N.check(self._lib.porl_iql_load_batch_pairs(
            self._h, batch, N.ptr(rows), stride, n, int(state_dim), int(act_dim), int(goal_col), int(goal_dim),
            N.ptr(start), N.ptr(goal), N.ptr(ep_s), N.ptr(ep_l), n_ep, seed & mask, step & mask, N.ptr(start_out),
            N.ptr(goal_out), N.current_stream_ptr(self.device)), "porl_iql_load_batch_pairs")
        self.last_batch = batch
        return batch

    # the behaviour-cloning step on a batch staged by the two loaders above: the whole step, or its forward half followed by
    # policy_backward (/ policy_apply)
    def bc_step(self, hp): self._phase("porl_iql_bc_step", hp)
    def bc_forward(self, hp): self._phase("porl_iql_bc_forward", hp)

    def set_stats(self, stats):
        """Point the loss statistics of the following updates at `stats` (>= 8 fp32 on the device)."""
        self._ensure_bound()
        if stats.device != self.device or stats.dtype != torch.float32 or stats.numel() < 8 or not stats.is_contiguous():
            raise RuntimeError("stats must be >= 8 contiguous fp32 on the engine's device")
        N.check(self._lib.porl_iql_set_stats(self._h, N.ptr(stats)), "porl_iql_set_stats")
        self.stats = stats

    def group(self, g):
        """(params, grads, exp_avg, exp_avg_sq, target or None) flat tensors of optimizer group g."""
        if g == self.GROUP_VF:
            return self.params_vf, self.grads_vf, self.adam_m_vf, self.adam_v_vf, self.params_tgt
        return self.params_pol, self.grads_pol, self.adam_m_pol, self.adam_v_pol, None

    def hyper(self, **kw):
        d = dict(tau=0.9, discount=0.99, alpha=10.0, ema_beta=0.005, inv_batch=1.0, value_lr=1e-4,
                 policy_lr=1e-4, value_step=1, policy_step=1, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
        d.update(kw)
        return N.IqlHyper(**d)

    def _phase(self, name, hp):
        N.check(getattr(self._lib, name)(self._h, C.byref(hp), N.current_stream_ptr(self.device)), name)

    def value_backward(self, hp): self._phase("porl_iql_value_backward", hp)
    def value_apply(self, hp): self._phase("porl_iql_value_apply", hp)
    def policy_forward(self, hp): self._phase("porl_iql_policy_forward", hp)
    def policy_backward(self, hp): self._phase("porl_iql_policy_backward", hp)
    def policy_apply(self, hp): self._phase("porl_iql_policy_apply", hp)
    def step(self, hp): self._phase("porl_iql_step", hp)
    # policy-only step (frozen value nets): the whole step, or its forward half followed by policy_backward / policy_apply
    def policy_only(self, hp): self._phase("porl_iql_policy_only_step", hp)
    def policy_only_forward(self, hp): self._phase("porl_iql_policy_only_forward", hp)

    def update_pipelined(self, hp, replay, batch, seq, wait_policy_seq, wait_fwd_seq, write_policy):
        """One pipelined update on rows drawn from `replay` (PackedReplay): value phase on the current stream, policy
        phase on the side stream, ordered by the signal counters — include/porl_hip.h:porl_iql_update_pipelined."""
        rows = replay.rows
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1:
            raise RuntimeError("replay rows must be a 2-D fp32 tensor on the engine's device")
        sig = self.signals()
        N.check(self._lib.porl_iql_update_pipelined(
            self._h, C.byref(hp), batch, N.ptr(rows), rows.stride(0), rows.shape[0], replay.act_dim,
            int(self.cfg.weight_mode == 1), replay.seed & 0xFFFFFFFFFFFFFFFF, replay.draws,
            sig[self.SIG_VALUE], sig[self.SIG_FWD], sig[self.SIG_POLICY], int(seq), int(wait_policy_seq),
            int(wait_fwd_seq), int(bool(write_policy)), N.current_stream_ptr(self.device),
            C.c_void_p(self.side_stream().cuda_stream)), "porl_iql_update_pipelined")
        self.last_batch = batch

    def policy_prefetch(self):
        N.check(self._lib.porl_iql_policy_prefetch(self._h, N.current_stream_ptr(self.device)), "porl_iql_policy_prefetch")

    # -- forward-only ------------------------------------------------------------------------------
    def forward_value(self, x, target=False):
        self._ensure_bound()
        self.join()
        x = self._mat(x, self.cfg.obs_dim, "state")
        B = x.shape[0]
        v1 = torch.empty(B, dtype=torch.float32, device=self.device)
        v2 = torch.empty_like(v1)
        N.check(self._lib.porl_iql_forward_value(self._h, int(target), N.ptr(x), x.stride(0), B, N.ptr(v1),
                                                 N.ptr(v2), N.current_stream_ptr(self.device)), "porl_iql_forward_value")
        return v1, v2

    def forward_policy(self, x):
        self._ensure_bound()
        self.join()
        x = self._mat(x, self.cfg.obs_dim, "obs")
        B, D = x.shape[0], self.cfg.pol_out_dim
        mean = torch.empty(B, D, dtype=torch.float32, device=self.device)
        N.check(self._lib.porl_iql_forward_policy(self._h, N.ptr(x), x.stride(0), B, N.ptr(mean), D,
                                                  N.current_stream_ptr(self.device)), "porl_iql_forward_policy")
        return mean

    SMALL_BATCH = 8                                       # kernels.hpp: SMALL_FWD_MAX_B

    def forward_policy_host(self, x):
        """Rollout path (reference test.py:28-30: one observation in, one action out as numpy): the three small-batch
        launches read the observation from and write the mean to PINNED HOST memory — no copy launches, no torch
        kernels, one stream synchronisation.  `x`: (B <= 8, obs_dim) float32, a device tensor, a CPU tensor or an
        ndarray.  Returns a fresh (B, D) float32 ndarray.  Rows too wide for the small-batch kernels (more than
        64 KiB for the B inputs of a layer) take the batched path, which reads and writes the same pinned buffers."""
        self._ensure_bound()
        self.join()
        B, D, S = int(x.shape[0]), self.cfg.pol_out_dim, self.cfg.obs_dim
        if B < 1 or B > self.SMALL_BATCH or tuple(x.shape) != (B, S):
            raise RuntimeError(f"obs: expected shape (1..{self.SMALL_BATCH}, {S}), got {tuple(x.shape)}")
        if getattr(self, "_pin", None) is None:
            self._pin = (torch.empty(self.SMALL_BATCH, S, dtype=torch.float32).pin_memory(),
                         torch.empty(self.SMALL_BATCH, D, dtype=torch.float32).pin_memory())
        pin_in, pin_out = self._pin
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            if x.dtype != torch.float32:
                raise RuntimeError(f"obs: expected float32, got {x.dtype}")
            src = x if x.stride(1) == 1 else x.contiguous()
            xp, xrs = N.ptr(src), src.stride(0)
        else:
            pin_in[:B].copy_(torch.as_tensor(x, dtype=torch.float32))      # host memcpy into the staging rows
            xp, xrs = N.ptr(pin_in), S
        stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.porl_iql_forward_policy(self._h, xp, xrs, B, N.ptr(pin_out), D, C.c_void_p(stream.cuda_stream)),
                "porl_iql_forward_policy")
        stream.synchronize()
        return pin_out[:B].numpy().copy()

    def _free_signals(self):
        for p in (getattr(self, "_signals", None) or []):
            self._lib.porl_signal_destroy(p)
        self._signals = None

    def __del__(self):
        try:
            self._free_signals()
            if getattr(self, "_h", None):
                self._lib.porl_iql_destroy(self._h)
                self._h = None
        except Exception:
            pass


def replay_args(states, actions, rewards, next_states, dones, state_dim, device, n_rows=None, idx=None):
    """The one check of device-resident replay arrays in front of a row-sourced native call: each array contiguous, of its
    dtype, on `device` and (with `n_rows`) at least that long, rows `state_dim` wide, `idx` (if given) contiguous int64 on
    `device`.  Raises RuntimeError naming the offending array; returns the arrays as the C ABI takes them:
    (states, s_rs, actions, rewards, next_states, n_rs, dones)."""
    short = n_rows is not None
    for name, x, dt in (("states", states, torch.float32), ("next_states", next_states, torch.float32),
                        ("actions", actions, torch.int64), ("rewards", rewards, torch.float32),
                        ("dones", dones, torch.float32)):
        if x.dtype != dt or x.device != device or not x.is_contiguous() or (short and x.shape[0] < n_rows):
            rows = "" if n_rows is None else f" of >= {n_rows} rows"
            raise RuntimeError(f"{name}: need a contiguous {dt} tensor{rows} on {device}")
    if states.shape[1:].numel() != state_dim:
        raise RuntimeError(f"states: rows of {states.shape[1:].numel()} floats, the network's state_dim is {state_dim}")
    if next_states.shape != states.shape:
        raise RuntimeError(f"next_states: shape {tuple(next_states.shape)}, states have {tuple(states.shape)}")
    if idx is not None and (idx.dtype != torch.int64 or idx.device != device or not idx.is_contiguous()):
        raise RuntimeError(f"idx: need a contiguous torch.int64 tensor on {device}")
    return N.ptr(states), state_dim, N.ptr(actions), N.ptr(rewards), N.ptr(next_states), state_dim, N.ptr(dones)


class QnetEngine:
    """The Q-network engine of the C ABI (porl_qnet_*): every ctypes call on its handle is a method here."""

    def __init__(self, state_dim, n_actions, hidden, max_batch, device):
        self.device = _norm_device(device)
        hid = (C.c_int32 * 8)(*hidden)
        self.cfg = N.QnetCfg(int(state_dim), int(n_actions), len(hidden), hid, int(max_batch))
        self._lib = N.lib()
        h = C.c_void_p()
        N.check(self._lib.porl_qnet_create(C.byref(self.cfg), C.byref(h)), "porl_qnet_create")
        self._h = h
        self.n_params = int(self._lib.porl_qnet_param_floats(h))
        z = lambda: torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.params, self.params_tgt, self.grads, self.adam_m, self.adam_v = z(), z(), z(), z(), z()
        self.stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.workspace, self._bound = None, False

    @property
    def fused(self):
        """True when the network fits the one-launch step kernel (csrc/qnet_fused.hpp)."""
        return bool(self._lib.porl_qnet_one_launch(self._h))

    def tensor_table(self):
        """[(offset, shape, row stride)] — weight matrices sit inside zero-padded images (include/porl_hip.h)."""
        out = []
        off, r, c, ld = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        for i in range(int(self._lib.porl_qnet_tensors(self._h))):
            N.check(self._lib.porl_qnet_tensor_info(self._h, i, C.byref(off), C.byref(r), C.byref(c), C.byref(ld)))
            out.append((off.value, (c.value,) if r.value == 0 else (r.value, c.value), ld.value))
        return out

    def views(self, flat):
        """Parameter-shaped views into a flat group (weights: strided (out, in) windows of their padded images)."""
        return [flat[o:o + s[0]] if len(s) == 1 else flat[o:o + s[0] * ld].view(s[0], ld)[:, :s[1]]
                for o, s, ld in self.tensor_table()]

    def adopt(self, mod, which=0, params=None):
        """Move a module onto this engine: copy its parameters (`params`: the ones the engine owns, default all) into the
        views of the online (0) / target (1) group, re-point them there, and route the module's forward to the engine."""
        with torch.no_grad():
            for p, v in zip(mod.parameters() if params is None else params,
                            self.views(self.params if which == 0 else self.params_tgt)):
                v.copy_(p)
                p.data = v
        mod._engine, mod._which = self, which

    def _ensure_bound(self):
        if self.device.type != "cuda":
            raise N.NativeError("porl_amd computes on a HIP device only (device='cuda'); there is no CPU path")
        if self._bound:
            return
        self.workspace = torch.empty(int(self._lib.porl_qnet_workspace_floats(self._h)), dtype=torch.float32,
                                     device=self.device)
        b = N.QnetBuffers(*[C.c_void_p(t.data_ptr()) for t in (self.params, self.params_tgt, self.grads,
                                                                 self.adam_m, self.adam_v, self.workspace, self.stats)])
        N.check(self._lib.porl_qnet_bind(self._h, C.byref(b)), "porl_qnet_bind")
        self._bound = True

    def _states(self, x, what="states"):
        if x.dtype != torch.float32:
            x = x.float()
        x = x.reshape(x.shape[0], -1)
        if x.shape[1] != self.cfg.state_dim:
            raise RuntimeError(f"{what}: expected (B, {self.cfg.state_dim}), got {tuple(x.shape)}")
        if x.device != self.device:
            raise RuntimeError(f"{what} on {x.device}, engine on {self.device}")
        return x if x.stride(1) == 1 else x.contiguous()

    def load_batch(self, states, actions, rewards, next_states, dones):
        self._ensure_bound()
        states, next_states = self._states(states), self._states(next_states, "next_states")
        B = states.shape[0]
        if B > self.cfg.max_batch:
            raise RuntimeError(f"batch {B} exceeds engine max_batch {self.cfg.max_batch}")
        if actions.dtype != torch.int64:
            actions = actions.long()
        rewards, dones = rewards.float(), dones.float()
        self._held = (states, actions, rewards, next_states, dones)
        N.check(self._lib.porl_qnet_load_batch(self._h, B, N.ptr(states), states.stride(0), N.ptr(actions),
                                               actions.stride(0), N.ptr(rewards), rewards.stride(0),
                                               N.ptr(next_states), next_states.stride(0), N.ptr(dones),
                                               dones.stride(0), N.current_stream_ptr(self.device)), "porl_qnet_load_batch")
        return B

    def hyper(self, gamma, alpha, inv_batch, step, lr, betas=(0.9, 0.999), eps=1e-8):
        return N.QnetHyper(gamma, alpha, inv_batch, step, lr, betas[0], betas[1], eps)

    post_step = None      # callable(hp) run after every optimizer step of this engine (dueling heads: _DuelingHeads)

    def _stepped(self, hp):
        if self.post_step is not None:
            self.post_step(hp)

    def cql_backward(self, hp): N.check(self._lib.porl_qnet_cql_backward(self._h, C.byref(hp), N.current_stream_ptr(self.device)), "porl_qnet_cql_backward")

    def apply(self, hp):
        N.check(self._lib.porl_qnet_apply(self._h, C.byref(hp), N.current_stream_ptr(self.device)), "porl_qnet_apply")
        self._stepped(hp)

    def learn(self, hp):
        N.check(self._lib.porl_qnet_learn(self._h, C.byref(hp), N.current_stream_ptr(self.device)), "porl_qnet_learn")
        self._stepped(hp)

    # -- the loaded minibatch, stage by stage (the distributional trainers' learn_on) ---------------------------------
    def forward_loaded(self, which_params, which_input, keep, out):
        """Forward of the online (0) / target (1) parameters on the loaded states (0) / next states (1) into `out`;
        `keep`: hold the activations for backward()."""
        self._ensure_bound()
        N.check(self._lib.porl_qnet_forward_loaded(self._h, which_params, which_input, int(keep), N.ptr(out), out.stride(0),
                                                   N.current_stream_ptr(self.device)), "porl_qnet_forward_loaded")
        return out

    def backward(self, dout):
        """Backward of the kept forward from dL/d(output) `dout` into the gradient group."""
        self._ensure_bound()
        N.check(self._lib.porl_qnet_backward(self._h, N.ptr(dout), dout.stride(0), N.current_stream_ptr(self.device)),
                "porl_qnet_backward")

    # -- row-sourced steps: the replay arrays stay where they are, the kernels read rows of them -----------------------
    def _replay(self, batch, states, actions, rewards, next_states, dones, n_rows=None, idx=None):
        """What every row-sourced step does first: bound engine, batch within max_batch, replay_args."""
        self._ensure_bound()
        cfg = self.cfg
        if batch > cfg.max_batch:
            raise RuntimeError(f"batch {batch} exceeds engine max_batch {cfg.max_batch}")
        return replay_args(states, actions, rewards, next_states, dones, cfg.state_dim, self.device, n_rows, idx)

    def learn_indexed(self, hp, states, actions, rewards, next_states, dones, idx, variant=None):
        """learn() on rows `idx` (int64, device) of device-resident replay arrays: gathered inside the one-launch step
        kernel, or — networks with a layer wider than 128 or more than five Linear layers — by one gather launch in
        front of the multi-launch path (same loss arithmetic, incl. the Double-DQN / importance-weight / BCQ-mask
        variants)."""
        B = idx.numel()
        args = self._replay(B, states, actions, rewards, next_states, dones, idx=idx)
        if variant is None:
            N.check(self._lib.porl_qnet_learn_indexed(self._h, *args, N.ptr(idx), B, C.byref(hp),
                                                      N.current_stream_ptr(self.device)), "porl_qnet_learn_indexed")
        else:
            N.check(self._lib.porl_qnet_learn_variant(self._h, *args, N.ptr(idx), B, C.byref(hp), C.byref(variant),
                                                      N.current_stream_ptr(self.device)), "porl_qnet_learn_variant")
        self._stepped(hp)
        return B

    def learn_sampled(self, hp, states, actions, rewards, next_states, dones, n_rows, batch, seed, draw, variant=None):
        """learn() on `batch` distinct rows of the first `n_rows` rows of device-resident replay arrays, drawn inside
        the step kernel (the indices of engine.sample_indices(n_rows, batch, seed, draw), never materialised); `variant`:
        a QnetVariant, e.g. td_off for BCQ's pre-training."""
        args = self._replay(batch, states, actions, rewards, next_states, dones, n_rows)
        draw_ = (int(n_rows), int(seed), int(draw), int(batch), C.byref(hp))
        if variant is None:
            N.check(self._lib.porl_qnet_learn_sampled(self._h, *args, *draw_, N.current_stream_ptr(self.device)),
                    "porl_qnet_learn_sampled")
        else:
            N.check(self._lib.porl_qnet_learn_sampled_variant(self._h, *args, *draw_, C.byref(variant),
                                                              N.current_stream_ptr(self.device)),
                    "porl_qnet_learn_sampled_variant")
        self._stepped(hp)
        return batch

    def dist_learn(self, hp, states, actions, rewards, next_states, dones, idx, head):
        """One C51 / QR-DQN step (N.DistHead `head`) on rows `idx` from one native call (porl_qnet_dist_learn): gather,
        the forwards grouped per layer, loss head, backward, Adam; the mean loss lands in stats[0]."""
        B = idx.numel()
        args = self._replay(B, states, actions, rewards, next_states, dones, idx=idx)
        if B < 1:
            raise RuntimeError(f"batch {B} outside [1, {self.cfg.max_batch}]")
        N.check(self._lib.porl_qnet_dist_learn(self._h, *args, N.ptr(idx), B, C.byref(hp), C.byref(head),
                                               N.current_stream_ptr(self.device)), "porl_qnet_dist_learn")
        return B

    # -- discrete BCQ (csrc/bcq_mask.hpp): `self` holds the behaviour policy in bcq_mask, the Q-networks in bcq_learn_* ----
    def bcq_mask(self, next_states, idx, threshold, out=None):
        """(B, A) fp32 0/1 mask of the actions whose behaviour probability in next_states[idx[b]] exceeds `threshold`
        (porl_qnet_bcq_mask; this engine's online parameters are the behaviour policy)."""
        self._ensure_bound()
        B, A = idx.numel(), self.cfg.n_actions
        if next_states.dtype != torch.float32 or next_states.device != self.device or not next_states.is_contiguous() or \
                next_states.shape[1:].numel() != self.cfg.state_dim:
            raise RuntimeError(f"next_states: need contiguous float32 rows of {self.cfg.state_dim} on {self.device}")
        if idx.dtype != torch.int64 or idx.device != self.device or not idx.is_contiguous():
            raise RuntimeError(f"idx: need a contiguous torch.int64 tensor on {self.device}")
        if out is None:
            out = torch.empty(B, A, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() or out.numel() < B * A:
            raise RuntimeError(f"out: need >= {B * A} contiguous float32 on {self.device}")
        N.check(self._lib.porl_qnet_bcq_mask(self._h, N.ptr(next_states), self.cfg.state_dim, N.ptr(idx), B, float(threshold),
                                             N.ptr(out), N.current_stream_ptr(self.device)), "porl_qnet_bcq_mask")
        return out

    def bcq_learn_indexed(self, beh_engine, hp, states, actions, rewards, next_states, dones, idx, threshold):
        """One BCQ step on rows `idx` of the replay arrays from one native call (porl_qnet_bcq_learn): behaviour mask of
        `beh_engine`, masked-argmax step, Adam."""
        B = idx.numel()
        args = self._replay(B, states, actions, rewards, next_states, dones, idx=idx)
        beh_engine._ensure_bound()
        N.check(self._lib.porl_qnet_bcq_learn(self._h, beh_engine._h, *args, N.ptr(idx), B, C.byref(hp), float(threshold),
                                              N.current_stream_ptr(self.device)), "porl_qnet_bcq_learn")
        self._stepped(hp)
        return B

    def bcq_learn_sampled(self, beh_engine, hp, states, actions, rewards, next_states, dones, n_rows, batch, seed, draw,
                          threshold):
        """bcq_learn_indexed on the rows engine.sample_indices(n_rows, batch, seed, draw) would give, drawn inside the
        mask kernel and the step kernel (porl_qnet_bcq_learn_sampled); needs can_sample."""
        args = self._replay(batch, states, actions, rewards, next_states, dones, n_rows)
        beh_engine._ensure_bound()
        N.check(self._lib.porl_qnet_bcq_learn_sampled(
            self._h, beh_engine._h, *args, int(n_rows), int(seed), int(draw), int(batch), C.byref(hp), float(threshold),
            N.current_stream_ptr(self.device)), "porl_qnet_bcq_learn_sampled")
        self._stepped(hp)
        return batch

    @property
    def can_sample(self):
        return bool(self._lib.porl_qnet_can_sample(self._h))

    post_sync = None      # callable() run after the target network was overwritten (dueling heads)

    def sync_target(self):
        self._ensure_bound()
        N.check(self._lib.porl_qnet_sync_target(self._h, N.current_stream_ptr(self.device)), "porl_qnet_sync_target")
        if self.post_sync is not None:
            self.post_sync()

    def forward(self, x, which=0):
        self._ensure_bound()
        x = self._states(x)
        q = torch.empty(x.shape[0], self.cfg.n_actions, dtype=torch.float32, device=self.device)
        N.check(self._lib.porl_qnet_forward(self._h, which, N.ptr(x), x.stride(0), x.shape[0], N.ptr(q),
                                            self.cfg.n_actions, N.current_stream_ptr(self.device)), "porl_qnet_forward")
        return q

    # -- online loop (csrc/online.hpp) ----------------------------------------------------------------
    RECORD_MAX_STATE = 480          # PORL_RECORD_MAX_STATE: 2 x state_dim floats ride in the record kernel's arguments
    ACT_MAX_BATCH = 8
    ACT_MAX_INLINE = 256            # floats of inline states per act launch

    def record(self, mirror, slot, state, next_state, action, reward, done):
        """Write one transition (host float32 rows `state` / `next_state`) into row `slot` of a device replay mirror
        (the dict of ReplayBuffer._mirror) with one launch; the values travel in the kernel's arguments."""
        self._ensure_bound()
        key = tuple(mirror[k].data_ptr() for k in ("states", "next_states", "actions", "rewards", "dones"))
        if getattr(self, "_mirror_key", None) != key:
            replay_args(mirror["states"], mirror["actions"], mirror["rewards"], mirror["next_states"], mirror["dones"],
                        self.cfg.state_dim, self.device)
            self._mirror_c = N.QnetMirror(*[C.c_void_p(p) for p in key], int(mirror["states"].shape[0]))
            self._mirror_key = key
        N.check(self._lib.porl_qnet_record(self._h, int(slot), state.ctypes.data, next_state.ctypes.data, int(action),
                                           float(reward), float(done), C.byref(self._mirror_c),
                                           N.current_stream_ptr(self.device)), "porl_qnet_record")

    @property
    def act_ok(self):
        """True when the network suits the one-workgroup act kernel (every layer <= 1024 wide, <= 2^19 parameter floats)."""
        return bool(self._lib.porl_qnet_act_ok(self._h))

    def act(self, out, states=None, row=0, batch=1, inline=None, which=0, kind=0, n_act=0, n_sub=1, support=None,
            stats=None, n_stats=0):
        """Greedy action(s) in one launch (porl_qnet_act) into the int32 record `out` (16 words, device or pinned host):
        out[:batch] = argmax_a Q(s_b, a) of rows [row, row + batch) of the device array `states`, or of `inline`
        (host float32, batch x state_dim); out[8:8+n_stats] (as fp32) = stats[:n_stats] (None: the engine's statistics).
        kind 0: argmax of the outputs; 1: C51 expectation over n_sub atoms with `support`; 2: QR mean of n_sub quantiles."""
        self._ensure_bound()
        if states is not None:
            if states.dtype != torch.float32 or states.device != self.device or states.stride(-1) != 1:
                raise RuntimeError(f"states: need float32 rows on {self.device}")
            src = N.QnetActSrc(int(batch), states.data_ptr(), states.stride(0), int(row), states.shape[0], None)
        else:
            inline = np.ascontiguousarray(inline, dtype=np.float32)
            src = N.QnetActSrc(int(batch), None, self.cfg.state_dim, 0, 0, inline.ctypes.data)
        epi = N.QnetActEpilogue(int(kind), int(n_act), int(n_sub), None if support is None else support.data_ptr(),
                                None if stats is None else stats.data_ptr(), int(n_stats))
        N.check(self._lib.porl_qnet_act(self._h, int(which), C.byref(src), C.byref(epi), C.c_void_p(out.data_ptr()),
                                        N.current_stream_ptr(self.device)), "porl_qnet_act")
        return out

    def act_rows(self, states, epsilon, seed, t, env_offset=0, q=None, out=None, which=0):
        """Epsilon-greedy actions (n,) int64 for n rows of states from one native call (porl_qnet_act_rows): the batched
        forward in chunks of max_batch into the scratch `q` (n, A), then qnet_select's kernel.  Plain-Q networks only."""
        self._ensure_bound()
        x = self._states(states)
        if q is None:
            q = torch.empty(x.shape[0], self.cfg.n_actions, dtype=torch.float32, device=self.device)
        if q.shape != (x.shape[0], self.cfg.n_actions) or q.device != self.device:
            raise RuntimeError(f"q: expected ({x.shape[0]}, {self.cfg.n_actions}) on {self.device}, got {tuple(q.shape)} on {q.device}")
        out, q_rs = _select_args(q, out)
        N.check(self._lib.porl_qnet_act_rows(self._h, int(which), N.ptr(x), x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1]),
                                             x.shape[0], N.ptr(q), q_rs, float(epsilon), int(seed) & (2 ** 64 - 1),
                                             int(env_offset), int(t), N.ptr(out), N.current_stream_ptr(self.device)),
                "porl_qnet_act_rows")
        return out

    def act_rows_dist(self, states, head, epsilon, seed, t, env_offset=0, q=None, out=None, which=0):
        """act_rows for a C51 / QR-DQN network (N.DistHead `head`, porl_qnet_act_rows_dist): the batched forward in chunks
        of max_batch, each chunk's output rows read in the workspace by dist_select's kernel — the (n, A * n_sub) outputs
        are never copied out.  `q` (n, A) receives the action values."""
        self._ensure_bound()
        x = self._states(states)
        q, out, q_rs = _dist_select_args(x.shape[0], head, q, out, self.device)
        N.check(self._lib.porl_qnet_act_rows_dist(self._h, int(which), N.ptr(x), x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1]),
                                                  x.shape[0], C.byref(head), N.ptr(q), q_rs, float(epsilon),
                                                  int(seed) & (2 ** 64 - 1), int(env_offset), int(t), N.ptr(out),
                                                  N.current_stream_ptr(self.device)), "porl_qnet_act_rows_dist")
        return out

    def act_rows_bcq(self, beh_engine, states, threshold, epsilon, seed, t, env_offset=0, q=None, logits=None, mask=None,
                     out=None, which=0):
        """act_rows under discrete BCQ's constraint (porl_qnet_act_rows_bcq; `self` holds the Q-networks, `beh_engine` the
        behaviour policy): both forwards in chunks of the smaller max_batch into the scratch `q` and `logits` (n, A, dense),
        then bcq_select's kernel once for all n rows.  `mask` (n, A), optional, receives the 0 / 1 rows."""
        self._ensure_bound()
        beh_engine._ensure_bound()
        x = self._states(states)
        n, A = x.shape[0], self.cfg.n_actions
        if q is None:
            q = torch.empty(n, A, dtype=torch.float32, device=self.device)
        if logits is None:
            logits = torch.empty(n, A, dtype=torch.float32, device=self.device)
        for name, tab in (("q", q), ("logits", logits)):
            # dense: porl_qnet_forward writes a row over its whole stride, zeros behind the A values
            if tab.shape != (n, A) or tab.device != self.device or tab.dtype != torch.float32 or not tab.is_contiguous():
                raise RuntimeError(f"{name}: expected a contiguous ({n}, {A}) float32 table on {self.device}, got "
                                   f"{tuple(tab.shape)} on {tab.device}")
        out, q_rs, z_rs, mask = _bcq_select_args(q, logits, mask, out)
        N.check(self._lib.porl_qnet_act_rows_bcq(self._h, beh_engine._h, int(which), N.ptr(x),
                                                 x.stride(0) if n > 1 else max(x.stride(0), x.shape[1]), n, N.ptr(q), q_rs,
                                                 N.ptr(logits), z_rs, float(threshold), float(epsilon), int(seed) & (2 ** 64 - 1),
                                                 int(env_offset), int(t), N.ptr(mask), N.ptr(out),
                                                 N.current_stream_ptr(self.device)), "porl_qnet_act_rows_bcq")
        return out

    def dist_learn_sampled(self, hp, states, actions, rewards, next_states, dones, n_rows, batch, seed, draw, head):
        """dist_learn on the rows engine.sample_indices(n_rows, batch, seed, draw) would give, drawn inside the gather
        launch (porl_qnet_dist_learn_sampled); the mean loss lands in stats[0]."""
        args = self._replay(batch, states, actions, rewards, next_states, dones, n_rows)
        N.check(self._lib.porl_qnet_dist_learn_sampled(self._h, *args, int(n_rows), int(seed), int(draw), int(batch),
                                                       C.byref(hp), C.byref(head), N.current_stream_ptr(self.device)),
                "porl_qnet_dist_learn_sampled")
        return batch

    def penalty(self, states, actions):
        self._ensure_bound()
        states = self._states(states)
        actions = actions.long()
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        N.check(self._lib.porl_qnet_penalty(self._h, N.ptr(states), states.stride(0), N.ptr(actions),
                                            actions.stride(0), states.shape[0], N.ptr(out),
                                            N.current_stream_ptr(self.device)), "porl_qnet_penalty")
        return out[0]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.porl_qnet_destroy(self._h)
                self._h = None
        except Exception:
            pass


class IqnEngine:
    """The IQN engine of the C ABI (porl_iqn_*): one learn step / one greedy action of IQNTrainer per native call, on flat
    buffers the caller owns (`bind`).  Tensors in IQNNetwork.parameters() order, each starting on a 16-byte boundary —
    the layout train.iqn_trainer._FlatAdam builds."""

    MAX_EMBED, MAX_TAU, MAX_ACTIONS, ACT_MAX_INLINE = 128, 256, 64, 256

    def __init__(self, state_dim, n_actions, embedding_dim, hidden, max_batch, max_tau, device):
        self.device = _norm_device(device)
        S, A, Ed, H = int(state_dim), int(n_actions), int(embedding_dim), int(hidden)
        numel = [H * S, H, H * H, H, H * Ed, H, H * H, H, A * H, A]
        offs, off = [], 0
        for k in numel:
            offs.append(off)
            off += (k + 3) // 4 * 4
        self.offsets, self.n_params = offs, off
        self.cfg = N.IqnCfg(S, A, Ed, H, int(max_batch), int(max_tau), (C.c_int64 * 10)(*offs), off)
        self._lib = N.lib()
        h = C.c_void_p()
        N.check(self._lib.porl_iqn_create(C.byref(self.cfg), C.byref(h)), "porl_iqn_create")
        self._h = h
        self.stats = self.workspace = None
        self._bound = False

    def bind(self, params, params_tgt, grads, adam_m, adam_v):
        if self.device.type != "cuda":
            raise N.NativeError("porl_amd computes on a HIP device only (device='cuda'); there is no CPU path")
        for name, t in (("params", params), ("params_tgt", params_tgt), ("grads", grads), ("adam_m", adam_m), ("adam_v", adam_v)):
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.numel() != self.n_params:
                raise RuntimeError(f"{name}: need {self.n_params} contiguous float32 on {self.device}")
        self.workspace = torch.empty(int(self._lib.porl_iqn_workspace_floats(self._h)), dtype=torch.float32, device=self.device)
        self.stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        self._held = (params, params_tgt, grads, adam_m, adam_v)
        b = N.QnetBuffers(*[C.c_void_p(t.data_ptr()) for t in (*self._held, self.workspace, self.stats)])
        N.check(self._lib.porl_iqn_bind(self._h, C.byref(b)), "porl_iqn_bind")
        self._bound = True
        return self

    def hyper(self, gamma, kappa, max_norm, step, lr, betas=(0.9, 0.999), eps=1e-8):
        return N.IqnHyper(gamma, kappa, max_norm, step, lr, betas[0], betas[1], eps)

    def learn(self, hp, states, actions, rewards, next_states, dones, idx, taus_prime, taus_double_prime):
        """One learn step on rows `idx` (int64, device) of the replay arrays (porl_iqn_learn); the mean loss, the total
        gradient norm and the clip coefficient land in stats[0:3]."""
        B = idx.numel()
        args = replay_args(states, actions, rewards, next_states, dones, self.cfg.state_dim, self.device, idx=idx)
        for name, x in (("taus_prime", taus_prime), ("taus_double_prime", taus_double_prime)):
            if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous():
                raise RuntimeError(f"{name}: need a contiguous {torch.float32} tensor on {self.device}")
            if x.dim() != 2 or x.shape[0] != B:
                raise RuntimeError(f"{name}: fractions come as a (batch, n) tensor, got {tuple(x.shape)} for batch {B}")
        N.check(self._lib.porl_iqn_learn(self._h, *args, N.ptr(idx), B, N.ptr(taus_prime), taus_prime.shape[1],
                                         N.ptr(taus_double_prime), taus_double_prime.shape[1], C.byref(hp),
                                         N.current_stream_ptr(self.device)), "porl_iqn_learn")
        return B

    def act(self, out, taus, states=None, row=0, inline=None, which=0, n_stats=0):
        """Greedy action of one state in the int32 record `out` (16 words, device or pinned host; porl_iqn_act):
        out[0] = argmax_a mean_n Z(s, taus[n])[a] for row `row` of the device array `states` or the host floats `inline`;
        out[8:8+n_stats] (as fp32) = the engine's statistics in stream order."""
        if taus.dtype != torch.float32 or taus.device != self.device or not taus.is_contiguous():
            raise RuntimeError(f"taus: need contiguous float32 on {self.device}")
        if states is not None:
            if states.dtype != torch.float32 or states.device != self.device or states.stride(-1) != 1:
                raise RuntimeError(f"states: need float32 rows on {self.device}")
            src = N.QnetActSrc(1, states.data_ptr(), states.stride(0), int(row), states.shape[0], None)
        else:
            inline = np.ascontiguousarray(inline, dtype=np.float32).reshape(-1)
            if inline.size != self.cfg.state_dim:
                raise RuntimeError(f"state: expected {self.cfg.state_dim} floats, got {inline.size}")
            src = N.QnetActSrc(1, None, self.cfg.state_dim, 0, 0, inline.ctypes.data)
        N.check(self._lib.porl_iqn_act(self._h, int(which), C.byref(src), N.ptr(taus), taus.numel(), int(n_stats),
                                       C.c_void_p(out.data_ptr()), N.current_stream_ptr(self.device)), "porl_iqn_act")
        return out

    def act_rows(self, states, n_tau, epsilon, seed, t, env_offset=0, taus=None, q=None, out=None, which=0):
        """Epsilon-greedy actions (n,) int64 on the device for the n rows of `states` (porl_iqn_act_rows): the forward in
        chunks of max_batch under `n_tau` fractions per robot — `taus` (n, n_tau), or with None the elements
        (env_offset + i) * n_tau + j of the acting stream at draw `t` (iqn_draw_taus, use 0) — then iqn_select_rows' kernel
        on each chunk's output rows in the workspace.  `q` (n, A) receives the action values; nothing is read back."""
        if not self._bound:
            raise N.NativeError("porl_iqn_act_rows: the engine is not bound")
        x = states
        if x.dim() != 2 or x.dtype != torch.float32 or x.device != self.device or x.shape[1] != self.cfg.state_dim or \
                (x.shape[1] > 1 and x.stride(1) != 1):
            raise RuntimeError(f"states: need (n, {self.cfg.state_dim}) float32 rows with unit column stride on {self.device}")
        n, A = x.shape[0], self.cfg.n_actions
        if taus is not None and (taus.dtype != torch.float32 or taus.device != self.device or not taus.is_contiguous() or
                                 tuple(taus.shape) != (n, int(n_tau))):
            raise RuntimeError(f"taus: need a contiguous ({n}, {int(n_tau)}) float32 tensor on {self.device}")
        if q is None:
            q = torch.empty(n, A, dtype=torch.float32, device=self.device)
        if q.dim() != 2 or q.shape != (n, A) or q.device != self.device:
            raise RuntimeError(f"q: expected ({n}, {A}) on {self.device}, got {tuple(q.shape)} on {q.device}")
        out, q_rs = _select_args(q, out)
        s_rs = x.stride(0) if n > 1 else max(x.stride(0), x.shape[1])
        N.check(self._lib.porl_iqn_act_rows(self._h, int(which), N.ptr(x), s_rs, n, N.ptr(taus), int(n_tau), float(epsilon),
                                            int(seed) & (2 ** 64 - 1), int(t), int(env_offset), N.ptr(q), q_rs, N.ptr(out),
                                            N.current_stream_ptr(self.device)), "porl_iqn_act_rows")
        return out

    def learn_sampled(self, hp, states, actions, rewards, next_states, dones, n_rows, batch, seed, draw, n_cur, n_tgt):
        """learn on the rows engine.sample_indices(n_rows, batch, seed, draw) would give, drawn inside the gather launch, with
        tau' (batch, n_cur) and tau'' (batch, n_tgt) from the fraction stream (iqn_draw_taus, uses 1 and 2, draw `draw`)
        (porl_iqn_learn_sampled); the statistics land in stats[0:3]."""
        args = replay_args(states, actions, rewards, next_states, dones, self.cfg.state_dim, self.device, n_rows=n_rows)
        N.check(self._lib.porl_iqn_learn_sampled(self._h, *args, int(n_rows), int(batch), int(seed) & (2 ** 64 - 1), int(draw),
                                                 int(n_cur), int(n_tgt), C.byref(hp), N.current_stream_ptr(self.device)),
                "porl_iqn_learn_sampled")
        return batch

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.porl_iqn_destroy(self._h)
                self._h = None
        except Exception:
            pass


# -- thin wrappers over the building blocks ---------------------------------------------------------
def gemm_f32(mode, A, B, M, N_, K, lda, ldb, C_out, ldc, bias=None, act=0, mask=None, ldmask=0, tile=-1,
             splitk=1, slab=None):
    """Test/utility entry: raw pointers of torch tensors, see include/porl_hip.h:porl_gemm_f32."""
    N.check(N.lib().porl_gemm_f32(mode, tile, M, N_, K, N.ptr(A), lda, N.ptr(B), ldb, N.ptr(C_out), ldc,
                                  N.ptr(bias), act, N.ptr(mask), ldmask, splitk, N.ptr(slab),
                                  N.current_stream_ptr(C_out)), "porl_gemm_f32")


_GEMM_DESC_TENSORS = ("A", "B", "C", "bias", "mask", "headw", "headout", "colsum", "a_colscale", "a_colshift", "resid",
                      "rscale", "cstat")


def gemm_f32_group(descs, tile=-1, single_buffer=0):
    """Test/utility entry: one launch of up to 8 products, see include/porl_hip.h:porl_gemm_f32_group.  Each descriptor
    is a dict of porl_gemm_desc fields: torch tensors (or None) for the pointers, ints for the rest; store_c defaults
    to 1, everything else to 0 / NULL."""
    arr = (N.GemmDesc * max(len(descs), 1))()
    for d, a in zip(descs, arr):
        unknown = set(d) - {n for n, _ in N.GemmDesc._fields_}
        if unknown:
            raise KeyError(f"not porl_gemm_desc fields: {sorted(unknown)}")
        a.store_c = 1
        for k, v in d.items():
            setattr(a, k, (None if v is None else v.data_ptr()) if k in _GEMM_DESC_TENSORS else int(v))
    dev = descs[0].get("C") if descs else None
    N.check(N.lib().porl_gemm_f32_group(arr, len(descs), tile, single_buffer, N.current_stream_ptr(dev)),
            "porl_gemm_f32_group")


def adam_ema(p, g, m, v, target, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, ema_beta=0.0):
    N.check(N.lib().porl_adam_ema(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(target), p.numel(), lr, step,
                                  beta1, beta2, eps, ema_beta, N.current_stream_ptr(p)), "porl_adam_ema")


def ema(target, source, ema_beta):
    N.check(N.lib().porl_ema(N.ptr(target), N.ptr(source), target.numel(), ema_beta, N.current_stream_ptr(target)), "porl_ema")


def gather_rows(rows, idx, out=None):
    """out[i] = rows[idx[i]] for a 2-D fp32 (or bit-reinterpreted) device tensor."""
    if rows.dim() != 2 or rows.stride(1) != 1:
        raise RuntimeError("rows must be 2-D with unit column stride")
    n, w = idx.numel(), rows.shape[1]
    if out is None:
        out = torch.empty(n, w, dtype=rows.dtype, device=rows.device)
    N.check(N.lib().porl_gather_rows(N.ptr(rows), rows.stride(0), N.ptr(idx), n, w, N.ptr(out), out.stride(0),
                                     N.current_stream_ptr(out)), "porl_gather_rows")
    return out


def sample_indices(n_rows, batch, seed, step, out=None, base=0, device="cuda"):
    """`batch` distinct row indices in [base, base + n_rows) drawn on the device (int64)."""
    if out is None:
        out = torch.empty(batch, dtype=torch.int64, device=device)
    N.check(N.lib().porl_sample_indices(n_rows, batch, seed, step, base, N.ptr(out), N.current_stream_ptr(out)),
            "porl_sample_indices")
    return out


def _select_args(q, out):
    if q.dim() != 2 or q.dtype != torch.float32 or q.device.type != "cuda" or (q.shape[1] > 1 and q.stride(1) != 1):
        raise RuntimeError("q: need a (n, n_actions) float32 table with unit column stride on a HIP device")
    n = q.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=q.device)
    elif out.dtype != torch.int64 or out.device != q.device or out.shape != (n,) or not out.is_contiguous():
        raise RuntimeError(f"out: need a contiguous ({n},) int64 tensor on {q.device}")
    return out, (q.stride(0) if n > 1 else max(q.stride(0), q.shape[1]))


def qnet_select(q, epsilon, seed, t, env_offset=0, out=None):
    """Epsilon-greedy actions (n,) int64 on the device from action values q (n, A <= 64) (porl_qnet_select): robot i at
    act-step `t` draws from the counter stream keyed (seed, env_offset + i, t); nothing is read back."""
    out, q_rs = _select_args(q, out)
    N.check(N.lib().porl_qnet_select(N.ptr(q), q_rs, q.shape[1], q.shape[0], float(epsilon), int(seed) & (2 ** 64 - 1),
                                     int(env_offset), int(t), N.ptr(out), N.current_stream_ptr(q)), "porl_qnet_select")
    return out


def _bcq_select_args(q, logits, mask, out):
    """_select_args for the value table, the same rules for the behaviour logits, and the optional dense (n, A) mask."""
    out, q_rs = _select_args(q, out)
    n, A = q.shape
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.device != q.device or logits.shape != (n, A) or \
            (A > 1 and logits.stride(1) != 1):
        raise RuntimeError(f"logits: need a ({n}, {A}) float32 table with unit column stride on {q.device}")
    if mask is not None and (mask.dtype != torch.float32 or mask.device != q.device or mask.shape != (n, A) or
                             not mask.is_contiguous()):
        raise RuntimeError(f"mask: need a contiguous ({n}, {A}) float32 tensor on {q.device}")
    return out, q_rs, (logits.stride(0) if n > 1 else max(logits.stride(0), A)), mask


def bcq_select(q, logits, threshold, epsilon, seed, t, env_offset=0, mask=None, out=None):
    """Epsilon-greedy actions (n,) int64 on the device under discrete BCQ's constraint (porl_bcq_select): from action values
    `q` and behaviour logits `logits`, both (n, A <= 64) — the arg-max of q over the actions whose softmax probability
    exceeds `threshold` (the learn step's expression q + (mask - 1) * 1e10), or with probability `epsilon` a uniform action
    out of all A, drawn as qnet_select draws it.  `mask` (n, A) float32, optional, receives the 0 / 1 rows — the bits of
    BehaviorPolicy.sample on the same logits.  Nothing is read back."""
    out, q_rs, z_rs, mask = _bcq_select_args(q, logits, mask, out)
    N.check(N.lib().porl_bcq_select(N.ptr(q), q_rs, N.ptr(logits), z_rs, q.shape[1], q.shape[0], float(threshold), float(epsilon),
                                    int(seed) & (2 ** 64 - 1), int(env_offset), int(t), N.ptr(mask), N.ptr(out),
                                    N.current_stream_ptr(q)), "porl_bcq_select")
    return out


def _dist_select_args(n, head, q, out, device):
    """The (n, A) value table (a scratch one when None) and the (n,) int64 actions of a distributional select."""
    A = int(head.n_actions)
    if q is None:
        q = torch.empty(n, max(A, 1), dtype=torch.float32, device=device)
    if q.dim() != 2 or q.shape != (n, A) or q.device != device:
        raise RuntimeError(f"q: expected ({n}, {A}) on {device}, got {tuple(q.shape)} on {q.device}")
    out, q_rs = _select_args(q, out)
    return q, out, q_rs


def dist_select(z, head, epsilon, seed, t, env_offset=0, q=None, out=None):
    """Epsilon-greedy actions (n,) int64 on the device from the outputs z (n, A * n_sub) of a distributional network
    (N.DistHead `head`; porl_dist_select): one value per action — the quantile mean (QR-DQN) or the expectation of the
    softmax over the atoms (C51), in the loss heads' summation order — written to `q` (n, A) when given, then qnet_select's
    rule on them with the same key and draws; nothing is read back."""
    if z.dim() != 2 or z.dtype != torch.float32 or z.device.type != "cuda" or (z.shape[1] > 1 and z.stride(1) != 1):
        raise RuntimeError("z: need a (n, n_actions * n_sub) float32 table with unit column stride on a HIP device")
    n, w = z.shape[0], int(head.n_actions) * int(head.n_sub)
    if z.shape[1] != w:
        raise RuntimeError(f"z: expected ({n}, {head.n_actions} x {head.n_sub}), got {tuple(z.shape)}")
    q, out, q_rs = _dist_select_args(n, head, q, out, z.device)
    z_rs = z.stride(0) if n > 1 else max(z.stride(0), w)
    N.check(N.lib().porl_dist_select(N.ptr(z), z_rs, C.byref(head), n, N.ptr(q), q_rs, float(epsilon), int(seed) & (2 ** 64 - 1),
                                     int(env_offset), int(t), N.ptr(out), N.current_stream_ptr(z)), "porl_dist_select")
    return out


def iqn_draw_taus(seed, use, draw, first, count, out=None, device="cuda"):
    """Elements [first, first + count) of the keyed fraction stream (float32, on the device; porl_iqn_draw_taus):
    use 0 the acting fractions, 1 tau', 2 tau''.  Every value is a multiple of 2^-24 in [0, 1)."""
    if out is None:
        out = torch.empty(max(int(count), 0), dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or out.numel() != count or not out.is_contiguous():
        raise RuntimeError(f"out: need {count} contiguous float32")
    N.check(N.lib().porl_iqn_draw_taus(int(seed) & (2 ** 64 - 1), int(use), int(draw), int(first), int(count), N.ptr(out),
                                       N.current_stream_ptr(out)), "porl_iqn_draw_taus")
    return out


def iqn_select_rows(z, n_tau, epsilon, seed, t, env_offset=0, q=None, out=None):
    """Epsilon-greedy actions (n,) int64 on the device from the quantile values z (n * n_tau, A) of n robots, robot i's
    n_tau rows one after the other (a column slice of a wider table is fine; porl_iqn_select_rows): the mean over a
    robot's rows, summed in the order the learn step ranks the next state's actions by, written to `q` (n, A) when given,
    then qnet_select's rule on it with the same key and draws; nothing is read back."""
    if z.dim() != 2 or z.dtype != torch.float32 or z.device.type != "cuda" or (z.shape[1] > 1 and z.stride(1) != 1):
        raise RuntimeError("z: need a (n * n_tau, n_actions) float32 table with unit column stride on a HIP device")
    n_tau = int(n_tau)
    if n_tau < 1 or z.shape[0] % n_tau:
        raise RuntimeError(f"z: {z.shape[0]} rows are not a multiple of n_tau {n_tau}")
    n, A = z.shape[0] // n_tau, z.shape[1]
    if q is None:
        q = torch.empty(n, max(A, 1), dtype=torch.float32, device=z.device)
    if q.dim() != 2 or q.shape != (n, A) or q.device != z.device:
        raise RuntimeError(f"q: expected ({n}, {A}) on {z.device}, got {tuple(q.shape)} on {q.device}")
    out, q_rs = _select_args(q, out)
    ld = z.stride(0) if z.shape[0] > 1 else max(z.stride(0), A)
    N.check(N.lib().porl_iqn_select_rows(N.ptr(z), ld, n, n_tau, A, float(epsilon), int(seed) & (2 ** 64 - 1), int(t),
                                         int(env_offset), N.ptr(q), q_rs, N.ptr(out), N.current_stream_ptr(z)),
            "porl_iqn_select_rows")
    return out


def epoch_indices(n_rows, first, count, seed, epoch, out=None, base=0, device="cuda"):
    """Positions first..first+count-1 of the keyed permutation (seed, epoch) of [0, n_rows) (int64, on the device)."""
    if out is None:
        out = torch.empty(count, dtype=torch.int64, device=device)
    N.check(N.lib().porl_epoch_indices(n_rows, first, count, seed, epoch, base, N.ptr(out), N.current_stream_ptr(out)),
            "porl_epoch_indices")
    return out


def prof_enable(on=True):
    N.check(N.lib().porl_prof_enable(int(on)), "porl_prof_enable")


def prof_read(max_entries=64):
    """[{name, launches, total_ms, flops, bytes}] — synchronises the device."""
    buf = (N.ProfEntry * max_entries)()
    n = N.lib().porl_prof_read(buf, max_entries)
    if n < 0:
        N.check(n, "porl_prof_read")
    return [dict(name=buf[i].name.decode(), launches=int(buf[i].launches), total_ms=float(buf[i].total_ms),
                 flops=float(buf[i].flops), bytes=float(buf[i].bytes)) for i in range(n)]


def tune_set(key, value):
    """Process defaults (porl_tune_set): engines created afterwards copy them; IqlEngine.tune_set edits a live one."""
    N.check(N.lib().porl_tune_set(key.encode(), int(value)), "porl_tune_set")
