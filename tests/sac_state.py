"""What a SAC gradient step reads or writes, as one flat {name: tensor}, and its
bitwise comparison: shared by the checkpoint tests on the CPU and the GPU."""
import torch


def learner_state(m):
    out = {f"policy/{k}": v for k, v in m.policy.state_dict().items()}
    for name, opt in (("actor_opt", m.actor_opt), ("critic_opt", m.critic_opt), ("ent_coef_opt", m.ent_coef_opt)):
        for i, s in opt.state_dict()["state"].items():
            for k, v in s.items():
                out[f"{name}/{i}/{k}"] = torch.as_tensor(v)
    out["log_ent_coef"] = m.log_ent_coef.detach()
    out["_update"] = m._update
    out["sample_gen"] = m.sample_gen.get_state()
    out["counters"] = torch.tensor([m.num_timesteps, m.n_updates])
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same_state(sa, sb, what):
    """``sa``, ``sb``: learners or :func:`learner_state` snapshots."""
    sa = sa if isinstance(sa, dict) else learner_state(sa)
    sb = sb if isinstance(sb, dict) else learner_state(sb)
    assert sa.keys() == sb.keys(), what
    assert any(k.startswith("critic_opt/") and k.endswith("exp_avg_sq") for k in sa), what
    for k in sa:
        x, y = sa[k], sb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), (what, k)
