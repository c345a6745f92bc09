"""Shared by the RecurrentPPO tests.  A CPU stand-in for BatchedSalpEnv (seeded
random observations and rewards, episodes of a fixed length, the step result's
shapes and dtypes as BatchedSalpEnv.step returns them without ``out``), and
what a learner's update reads or writes as one flat {name: tensor} with its
bitwise comparison (CPU and GPU checkpoint tests)."""
import torch

from grasp_lab_salp_amd._abi import INFO, INFO_DIM
from grasp_lab_salp_amd.batched_env import StepResult


class StubSim:
    device = torch.device("cpu")

    def __init__(self, n_envs=4, obs_dim=10, ep_len=5, seed=0):
        self.n_envs, self.obs_dim, self.ep_len = n_envs, obs_dim, ep_len
        self.g = torch.Generator().manual_seed(seed)
        self.t = torch.zeros(n_envs, dtype=torch.int64)
        self.ret = torch.zeros(n_envs, dtype=torch.float64)
        self.actions = []

    def _obs(self):
        return torch.randn(self.n_envs, self.obs_dim, generator=self.g)

    def reset(self, mask=None):
        if mask is None:
            self.t.zero_()
            self.ret.zero_()
        return self._obs()

    def step(self, actions, auto_reset=False, want_terminal_obs=True, out=None):
        self.actions.append(actions.clone())
        n = self.n_envs
        rew = torch.randn(n, generator=self.g, dtype=torch.float64)
        self.t += 1
        self.ret += rew
        trunc = self.t >= self.ep_len + torch.arange(n) % 2        # odd envs run one step longer
        info = torch.zeros(n, INFO_DIM, dtype=torch.float64)
        info[:, INFO["ep_return"]] = self.ret
        info[:, INFO["ep_len"]] = self.t.double()
        self.t[trunc] = 0
        self.ret[trunc] = 0.0
        return StepResult(self._obs(), rew, torch.zeros(n, dtype=torch.bool), trunc, self._obs(), info)


class StubEnv:
    def __init__(self, **kw):
        self.sim = StubSim(**kw)


def state_of(m):
    out = {f"policy/{k}": v for k, v in m.policy.state_dict().items()}
    for i, s in m.opt.state_dict()["state"].items():
        for k, v in s.items():
            out[f"opt/{i}/{k}"] = torch.as_tensor(v)
    out["sample_gen"], out["gen"] = m.sample_gen.get_state(), m.gen.get_state()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same(sa, sb, what):
    assert sa.keys() == sb.keys(), what
    assert any(k.startswith("opt/") and k.endswith("exp_avg_sq") for k in sa), what
    for k in sa:
        x, y = sa[k], sb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), (what, k)


def fill(m, seed):
    """The same seeded contents into a learner's rollout buffer and sequence states."""
    g = torch.Generator().manual_seed(seed)
    b = m.buf
    for t in (b.obs, b.actions, b.rewards, b.values, b.log_probs, b.advantages, b.returns, m.seq_states):
        t.copy_(torch.randn(t.shape, generator=g).to(t.device))
    b.episode_starts.copy_((torch.rand(b.episode_starts.shape, generator=g) < 0.2).float().to(m.device))
