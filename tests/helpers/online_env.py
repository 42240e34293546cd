"""Deterministic toy environment for the train_online fixtures and tests (gymnasium protocol: reset() -> (state, info),
step(a) -> (next_state, reward, terminated, truncated, info), close()).  S = 8 float32 features, A = 4 actions; all
randomness comes from the environment's own numpy Generator, never from the global numpy stream the trainers consume.
Episodes end either by termination (first feature above a threshold) or by truncation after `max_len` steps."""
import numpy as np


class ToyEnv:
    def __init__(self, seed=0, state_size=8, action_size=4, max_len=22):
        self.rng = np.random.default_rng(seed)
        self.S, self.A, self.max_len = state_size, action_size, max_len
        self.w = (0.6 * self.rng.standard_normal((action_size, state_size))).astype(np.float32)
        self.actions, self.ends = [], []
        self.closed = False

    def reset(self, seed=None):
        self.t = 0
        self.s = self.rng.standard_normal(self.S).astype(np.float32)
        return self.s.copy(), {}

    def step(self, action):
        a = int(action)
        self.actions.append(a)
        reward = float(np.tanh(self.w[a] @ self.s))
        nxt = (0.8 * np.roll(self.s, a + 1) + 0.4 * self.rng.standard_normal(self.S)).astype(np.float32)
        self.t += 1
        terminated = bool(nxt[0] > 1.2)
        truncated = self.t >= self.max_len
        if terminated or truncated:
            self.ends.append("terminated" if terminated else "truncated")
        self.s = nxt
        return nxt.copy(), reward, terminated, truncated, {}

    def close(self):
        self.closed = True


class RecordingLogger:
    """Stands in for the trainers' logger: every call, in order."""

    def __init__(self):
        self.calls = []

    def log_hyperparameters(self, hparams):
        self.calls.append(("log_hyperparameters", dict(hparams)))

    def log_step(self, *args):
        self.calls.append(("log_step",) + tuple(args))

    def log_episode(self, *args):
        self.calls.append(("log_episode",) + tuple(args))

    def log_loss(self, *args):
        self.calls.append(("log_loss",) + tuple(args))

    def close(self):
        self.calls.append(("close",))
