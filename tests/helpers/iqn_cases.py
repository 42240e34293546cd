"""Shared inputs of the IQN online tests (tests/test_iqn_online.py on the CPU, tests/test_iqn_online_gpu.py on the device):
the greedy-action cases — seeded network, 32 states, fixed fractions — with the fp64 oracle's answer and the states whose
top-two gap is wide enough for exact action equality to mean something."""
import numpy as np
import torch

from oracle import iqn_oracle as IO

ACT_S, ACT_A, ACT_E, ACT_STATES = 11, 5, 16, 32
ACT_CASES = [(32, 1), (32, 32), (512, 1), (512, 32)]          # (hidden, N_policy)
ACT_SEED = 3
ACT_MIN_GAP = 1e-4


def act_case(H, n_policy):
    """-> (state_dict as numpy, states (32, S) float32, taus (32, n_policy) float32, oracle actions, keep mask)."""
    from porl_amd.net.iqn_network import IQNNetwork
    torch.manual_seed(ACT_SEED)
    net = IQNNetwork(ACT_S, ACT_A, ACT_E, H)                   # built on the CPU: the weights a seeded trainer gets
    P = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    P["value_net.2.bias"][:] = 0.0                             # a default-initialised head answers with its largest bias
    P["value_net.2.weight"] *= 4.0
    rng = np.random.default_rng(1000 * H + n_policy)
    states = (1.5 * rng.standard_normal((ACT_STATES, ACT_S))).astype(np.float32)
    taus = rng.random((ACT_STATES, n_policy)).astype(np.float32)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    q = IO.forward(P64, states.astype(np.float64), taus.astype(np.float64)).mean(1)      # (32, A)
    top = np.sort(q, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= ACT_MIN_GAP
    return P, states, taus, q.argmax(1), keep
