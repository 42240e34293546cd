"""`DeviceReplay`: the five arrays of `ReplayBuffer` (buffer/replay_buffer.py) on the device only, in its dtypes and shapes
— states / next_states (capacity, state_dim) fp32, actions (capacity,) int64, rewards and dones (capacity,) fp32.  Kernels
write it (DiscreteLidarNavSim.step(actions, replay=...) puts robot i's transition into slot (position + i) % capacity) and
kernels read it (QnetEngine.learn_sampled / learn_indexed); the ring's position and size are host integers advanced by
`advance(n)` after a launch that wrote n rows.  There is no host copy."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native as N


class DeviceReplay:
    def __init__(self, capacity: int, state_dim: int, device="cuda"):
        if capacity < 1 or state_dim < 1:
            raise ValueError("capacity and state_dim must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise N.NativeError(f"DeviceReplay lives on a HIP device only (device {self.device}); no CPU path")
        self.capacity, self.state_dim = int(capacity), int(state_dim)
        self.state_shape = (self.state_dim,)
        self.position, self.size = 0, 0
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=self.device)
        self.states, self.next_states = z(capacity, state_dim), z(capacity, state_dim)
        self.actions = z(capacity, dtype=torch.int64)
        self.rewards, self.dones = z(capacity), z(capacity)
        self._mirror_c = None

    def __len__(self) -> int:
        return self.size

    def arrays(self):
        """(states, actions, rewards, next_states, dones): the order QnetEngine's row-sourced steps take them in."""
        return self.states, self.actions, self.rewards, self.next_states, self.dones

    def mirror(self):
        """The arrays as a porl_qnet_mirror (N.QnetMirror)."""
        if self._mirror_c is None:
            self._mirror_c = N.QnetMirror(*[C.c_void_p(t.data_ptr()) for t in (self.states, self.next_states, self.actions,
                                                                               self.rewards, self.dones)], self.capacity)
        return self._mirror_c

    def advance(self, n: int) -> None:
        """n rows were written from `position` on (wrapping): move the ring."""
        if not 0 <= n <= self.capacity:
            raise ValueError(f"advance({n}): a launch writes at most capacity = {self.capacity} rows")
        self.position = (self.position + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
