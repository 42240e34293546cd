"""Prioritized replay with the sum tree on the device — the counterpart of
/root/reference/src/porl/buffer/prioritized_replay_buffer.py:7-108 (+ sum_tree.py:4-77) for typed transitions.

Same constructor, `add(td_error, state, action, reward, next_state, done)`, `sample(batch_size)` ->
(states, actions, rewards, next_states, dones, is_weights, idxs), `update_priorities(idxs, td_errors)`, `len()`,
beta annealing and ring semantics.  The tree is 2*capacity-1 fp64 values in HBM in the reference's heap layout, so
`idxs` are the reference's tree indices.  The host draws the stratified uniforms from Python's `random` exactly as
the reference does (`random.uniform(a, b)` = a + (b - a) * `random.random()`), the device does the tree walk, the
importance weights and the gather; results are device tensors instead of numpy arrays.

Differences: experiences are typed SoA rows (like ReplayBuffer) rather than arbitrary Python objects; ancestors are
recomputed from their children instead of accumulating rounded differences (sums agree to ~1e-16 relative, so a
sampled index can differ from the reference only when s falls within that distance of a boundary); the reference's
"resample from the full range when an empty slot is hit" branch is not needed because empty leaves carry zero
priority.  `add` queues on the host and is flushed in one batch before the next `sample`/`update_priorities`.

For the online loop (train/online.py) three one-launch forms sit beside them, bit-equal in everything they write:
`record` (= `add` + flush of that transition, the row carried in the kernel's arguments), `sample_slots` (= `sample`
without the gathers: data slots for the step kernel, weights, their mean, tree indices) and `update_priorities_device`
(= `update_priorities` on a device fp32 tensor, e.g. the step kernel's |TD errors|).

For a loop that writes N rows per launch (train/vector_online.py; csrc/per_vector.hpp) the buffer is also a WRITER in
DeviceReplay's protocol — `states`, `next_states`, `state_dim`, `mirror()`, `position`, `advance(n)` — so
`DiscreteLidarNavSim.step(actions, replay=memory)` writes the rows and `advance(n)` gives the n new leaves the priority
`priority_for_new` by one launch (`fill_range`, porl_per_fill_range: bit-equal to `add(priority_for_new, ...)` n times and
a flush).  `sample_slots_keyed(batch_size, seed, draw)` is `sample_slots` with the uniforms drawn in the kernel from the
counter stream (seed, draw, i): nothing is taken from Python's `random`, nothing is copied, nothing waits.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import torch

from .. import _native as N
from .. import engine as E


class PrioritizedReplayBuffer:
    def __init__(self, capacity, alpha=0.6, beta_start=0.4, beta_frames=100000, epsilon=1e-5, state_shape=None,
                 device="cuda"):
        self.capacity, self.alpha, self.beta_start, self.beta_frames = int(capacity), alpha, beta_start, beta_frames
        self.beta, self.epsilon, self.frame_count = beta_start, epsilon, 0
        self.device = E._norm_device(device)
        if self.device.type != "cuda":
            raise N.NativeError("PrioritizedReplayBuffer keeps its tree on a HIP device (device='cuda'); no CPU path")
        self.state_shape = None if state_shape is None else tuple(state_shape)
        self.tree = torch.zeros(2 * self.capacity - 1, dtype=torch.float64, device=self.device)
        self._stamp = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self._store = None
        self.data_pointer, self.n_entries = 0, 0
        self._pending = []                 # (slot, td_error, state, action, reward, next_state, done)
        self._store_c = None               # the store's arrays as porl_qnet_mirror (record)
        self._u = None                     # sample_slots: staging ring of the uniforms + the raw-weight scratch
        self._raw = None                   # sample_slots_keyed: the raw-weight scratch
        self.priority_for_new = 1.0        # advance(n): the td_error new rows enter with (a trainer's max_initial_priority)
        if self.state_shape is not None:
            self._alloc(None)

    # -- storage ---------------------------------------------------------------------------------------
    def _alloc(self, state):
        if self.state_shape is None:
            self.state_shape = tuple(np.shape(state))
        sdim = int(np.prod(self.state_shape)) if self.state_shape else 1
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=self.device)
        self._store = dict(states=z(self.capacity, sdim), next_states=z(self.capacity, sdim), rewards=z(self.capacity, 1),
                           dones=z(self.capacity, 1), actions=z(self.capacity, dt=torch.int64))

    def add(self, td_error, *experience):
        state, action, reward, next_state, done = experience
        if self._store is None:
            self._alloc(state)
        self._pending.append((self.data_pointer, float(td_error), np.asarray(state, dtype=np.float32).reshape(-1),
                              int(action), float(reward), np.asarray(next_state, dtype=np.float32).reshape(-1), float(done)))
        self.data_pointer += 1
        if self.data_pointer >= self.capacity:
            self.data_pointer = 0
        if self.n_entries < self.capacity:
            self.n_entries += 1

    def _flush(self):
        if not self._pending:
            return
        slots = torch.tensor([p[0] for p in self._pending], dtype=torch.int64, device=self.device)
        st = self._store
        # a slot overwritten twice within one flush keeps the later experience (index_copy_ applies in order on one stream)
        last = {}
        for i, p in enumerate(self._pending):
            last[p[0]] = i
        keep = sorted(last.values())
        ks = torch.tensor([self._pending[i][0] for i in keep], dtype=torch.int64, device=self.device)
        st["states"][ks] = torch.from_numpy(np.stack([self._pending[i][2] for i in keep])).to(self.device)
        st["next_states"][ks] = torch.from_numpy(np.stack([self._pending[i][5] for i in keep])).to(self.device)
        st["actions"][ks] = torch.tensor([self._pending[i][3] for i in keep], dtype=torch.int64, device=self.device)
        st["rewards"][ks, 0] = torch.tensor([self._pending[i][4] for i in keep], dtype=torch.float32, device=self.device)
        st["dones"][ks, 0] = torch.tensor([self._pending[i][6] for i in keep], dtype=torch.float32, device=self.device)
        td = torch.tensor([p[1] for p in self._pending], dtype=torch.float64, device=self.device)
        self._update(slots + (self.capacity - 1), td)
        self._pending = []

    def _update(self, tree_idx, td_errors):
        n = tree_idx.numel()
        N.check(N.lib().porl_per_update(N.ptr(self.tree), self.capacity, N.ptr(tree_idx), N.ptr(td_errors), n, self.epsilon,
                                        self.alpha, N.ptr(self._stamp), N.current_stream_ptr(self.device)), "porl_per_update")

    # -- reference API ---------------------------------------------------------------------------------
    def total_priority(self):
        self._flush()
        return float(self.tree[0])

    def sample(self, batch_size):
        self._flush()
        if self.n_entries < 1:
            raise ValueError("cannot sample from an empty buffer")
        self.beta = np.min([1.0, self.beta_start + self.frame_count * (1.0 - self.beta_start) / self.beta_frames])
        self.frame_count += 1
        # random.uniform(a, b) == a + (b - a) * random.random(): one draw per segment, in segment order
        u = torch.tensor([random.random() for _ in range(batch_size)], dtype=torch.float64).to(self.device)
        idxs = torch.empty(batch_size, dtype=torch.int64, device=self.device)
        prio = torch.empty(2 * batch_size, dtype=torch.float64, device=self.device)
        w = torch.empty(batch_size, dtype=torch.float32, device=self.device)
        N.check(N.lib().porl_per_sample(N.ptr(self.tree), self.capacity, N.ptr(u), batch_size, self.n_entries, float(self.beta),
                                        N.ptr(idxs), N.ptr(prio), N.ptr(w), N.current_stream_ptr(self.device)), "porl_per_sample")
        slots = idxs - (self.capacity - 1)
        st = self._store
        states = E.gather_rows(st["states"], slots).view(batch_size, *self.state_shape)
        next_states = E.gather_rows(st["next_states"], slots).view(batch_size, *self.state_shape)
        rewards = E.gather_rows(st["rewards"], slots).view(batch_size)
        dones = E.gather_rows(st["dones"], slots).view(batch_size)
        actions = st["actions"][slots]
        self.last_priorities = prio[:batch_size]
        return states, actions, rewards, next_states, dones, w, idxs

    def update_priorities(self, tree_indices, td_errors):
        self._flush()
        idx = torch.as_tensor(tree_indices, dtype=torch.int64, device=self.device).contiguous()
        td = torch.as_tensor(td_errors, device=self.device).to(torch.float64).reshape(-1).contiguous()
        if idx.numel() != td.numel():
            raise ValueError("tree_indices and td_errors differ in length")
        self._update(idx, td)

    # -- one-launch forms for the online loop (csrc/per_online.hpp) ---------------------------------------
    _RING = 8

    def record(self, td_error, *experience):
        """`add` whose transition reaches the store and the tree by one launch (porl_per_record), nothing left pending;
        earlier `add`s are flushed first.  False (and a plain `add`) when the state is too wide for the arguments."""
        state, action, reward, next_state, done = experience
        if self._store is None:
            self._alloc(state)
        st = self._store
        sdim = st["states"].shape[1]
        if sdim > E.QnetEngine.RECORD_MAX_STATE:                 # PORL_RECORD_MAX_STATE: the row rides in the kernel's arguments
            self.add(td_error, *experience)
            return False
        if self._pending:
            self._flush()
        state = np.ascontiguousarray(state, dtype=np.float32).reshape(-1)
        next_state = np.ascontiguousarray(next_state, dtype=np.float32).reshape(-1)
        if state.size != sdim or next_state.size != sdim:
            raise ValueError(f"state of {state.size} / {next_state.size} values in a buffer of {sdim}-wide rows")
        if self._store_c is None:
            self._store_c = N.QnetMirror(*[C.c_void_p(st[k].data_ptr()) for k in
                                           ("states", "next_states", "actions", "rewards", "dones")], self.capacity)
        N.check(N.lib().porl_per_record(N.ptr(self.tree), self.capacity, self.data_pointer, float(td_error), self.epsilon,
                                        self.alpha, state.ctypes.data, next_state.ctypes.data, sdim, int(action),
                                        float(reward), float(done), C.byref(self._store_c),
                                        N.current_stream_ptr(self.device)), "porl_per_record")
        self.data_pointer += 1
        if self.data_pointer >= self.capacity:
            self.data_pointer = 0
        if self.n_entries < self.capacity:
            self.n_entries += 1
        return True

    def sample_slots(self, batch_size):
        """`sample` without the gathers, one launch (porl_per_sample_slots) -> (slots, is_weights, wmean, tree_idx):
        int64 data slots (= tree_idx - (capacity - 1)) for a kernel that reads the store's rows itself, the fp32
        normalised weights, their mean as a 1-element fp32 tensor, the int64 tree indices.  Same beta / frame_count
        bookkeeping and the same batch_size draws from `random`, in the same order, as `sample`."""
        if self._pending:
            self._flush()
        if self.n_entries < 1:
            raise ValueError("cannot sample from an empty buffer")
        B = int(batch_size)
        self.beta = np.min([1.0, self.beta_start + self.frame_count * (1.0 - self.beta_start) / self.beta_frames])
        self.frame_count += 1
        if self._u is None or self._u["host"].shape[1] != B:
            self._u = dict(host=torch.zeros(self._RING, B, dtype=torch.float64).pin_memory(),
                           dev=torch.zeros(self._RING, B, dtype=torch.float64, device=self.device),
                           raw=torch.zeros(B, dtype=torch.float64, device=self.device), ev=[None] * self._RING, k=0)
        r = self._u
        k = r["k"]
        r["k"] = (k + 1) % self._RING
        # a staging slot is rewritten only after its copy has completed
        if r["ev"][k] is not None:
            r["ev"][k].synchronize()
        else:
            r["ev"][k] = torch.cuda.Event()
        # random.uniform(a, b) == a + (b - a) * random.random(): one draw per segment, in segment order
        rnd = random.random
        r["host"][k].numpy()[:] = [rnd() for _ in range(B)]
        u = r["dev"][k]
        u.copy_(r["host"][k], non_blocking=True)
        r["ev"][k].record(torch.cuda.current_stream(self.device))
        idx = torch.empty(2, B, dtype=torch.int64, device=self.device)             # tree indices | data slots
        w = torch.empty(B + 1, dtype=torch.float32, device=self.device)             # weights | their mean
        N.check(N.lib().porl_per_sample_slots(N.ptr(self.tree), self.capacity, N.ptr(u), B, self.n_entries, float(self.beta),
                                              N.ptr(idx[0]), N.ptr(idx[1]), N.ptr(w), C.c_void_p(w.data_ptr() + 4 * B),
                                              N.ptr(r["raw"]), N.current_stream_ptr(self.device)), "porl_per_sample_slots")
        return idx[1], w[:B], w[B:], idx[0]

    def update_priorities_device(self, tree_indices, td_errors):
        """`update_priorities` for device tensors as they are — int64 tree indices, fp32 TD errors — in one launch
        (porl_per_update_f32); the tree comes out bit-equal to update_priorities(tree_indices, td_errors)."""
        if self._pending:
            self._flush()
        for name, x, dt in (("tree_indices", tree_indices, torch.int64), ("td_errors", td_errors, torch.float32)):
            if x.dtype != dt or x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{name}: need a contiguous {dt} tensor on {self.device}")
        if tree_indices.numel() != td_errors.numel():
            raise ValueError("tree_indices and td_errors differ in length")
        if tree_indices.numel() == 0:
            return
        N.check(N.lib().porl_per_update_f32(N.ptr(self.tree), self.capacity, N.ptr(tree_indices), N.ptr(td_errors),
                                            tree_indices.numel(), self.epsilon, self.alpha, N.ptr(self._stamp),
                                            N.current_stream_ptr(self.device)), "porl_per_update_f32")

    # -- the writer protocol of DeviceReplay and the keyed sampler (csrc/per_vector.hpp) ---------------------
    def _need_store(self):
        if self._store is None:
            raise ValueError("the store is not allocated yet: construct the buffer with state_shape, or add a transition first")
        return self._store

    @property
    def states(self):
        return self._need_store()["states"]

    @property
    def next_states(self):
        return self._need_store()["next_states"]

    @property
    def state_dim(self):
        return self._need_store()["states"].shape[1]

    @property
    def position(self):
        return self.data_pointer

    def arrays(self):
        """(states, actions, rewards, next_states, dones) in the shapes QnetEngine's row-sourced steps take."""
        st = self._need_store()
        return st["states"], st["actions"], st["rewards"].view(-1), st["next_states"], st["dones"].view(-1)

    def mirror(self):
        """The store's arrays as a porl_qnet_mirror (N.QnetMirror); pending host `add`s are flushed first, so a kernel
        that writes through it writes after them."""
        st = self._need_store()
        if self._pending:
            self._flush()
        if self._store_c is None:
            self._store_c = N.QnetMirror(*[C.c_void_p(st[k].data_ptr()) for k in
                                           ("states", "next_states", "actions", "rewards", "dones")], self.capacity)
        return self._store_c

    def fill_range(self, first_slot, n, td_error):
        """The tree half of `add(td_error, ...)` for the n data slots (first_slot + i) % capacity in one launch
        (porl_per_fill_range): leaves (|td_error| + eps)^alpha, their ancestors recomputed.  Moves no pointer."""
        if self._pending:
            self._flush()
        N.check(N.lib().porl_per_fill_range(N.ptr(self.tree), self.capacity, int(first_slot), int(n), float(td_error),
                                            self.epsilon, self.alpha, N.current_stream_ptr(self.device)), "porl_per_fill_range")

    def advance(self, n):
        """A launch wrote n rows from `position` on (wrapping): give their leaves `priority_for_new` and move the ring."""
        n = int(n)
        if not 0 <= n <= self.capacity:
            raise ValueError(f"advance({n}): a launch writes at most capacity = {self.capacity} rows")
        self.fill_range(self.data_pointer, n, self.priority_for_new)
        self.data_pointer = (self.data_pointer + n) % self.capacity
        self.n_entries = min(self.n_entries + n, self.capacity)

    def sample_slots_keyed(self, batch_size, seed, draw):
        """`sample_slots` with the uniforms drawn in the kernel (porl_per_sample_keyed) -> (slots, is_weights, wmean,
        tree_idx).  Same beta / frame_count bookkeeping; consumes nothing from Python's `random`."""
        if self._pending:
            self._flush()
        if self.n_entries < 1:
            raise ValueError("cannot sample from an empty buffer")
        B = int(batch_size)
        self.beta = np.min([1.0, self.beta_start + self.frame_count * (1.0 - self.beta_start) / self.beta_frames])
        self.frame_count += 1
        if self._raw is None or self._raw.numel() < B:
            self._raw = torch.zeros(B, dtype=torch.float64, device=self.device)
        idx = torch.empty(2, B, dtype=torch.int64, device=self.device)             # tree indices | data slots
        w = torch.empty(B + 1, dtype=torch.float32, device=self.device)             # weights | their mean
        N.check(N.lib().porl_per_sample_keyed(N.ptr(self.tree), self.capacity, int(seed) & (2 ** 64 - 1), int(draw), B,
                                              self.n_entries, float(self.beta), N.ptr(idx[0]), N.ptr(idx[1]), N.ptr(w),
                                              C.c_void_p(w.data_ptr() + 4 * B), N.ptr(self._raw),
                                              N.current_stream_ptr(self.device)), "porl_per_sample_keyed")
        return idx[1], w[:B], w[B:], idx[0]

    def __len__(self):
        return self.n_entries
