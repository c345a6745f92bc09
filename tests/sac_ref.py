"""NumPy restatements the SAC tests compare against (no torch, no library):
the replay ring of include/salp.h "SAC" env by env in plain loops, a vectorised
Philox4x32-10, the sampler's integer draw, and the closed forms of the heads
in float64."""
import numpy as np

REPLAY_STREAM = 0x52504C59          # csrc/salp_sac.hip SP_STREAM_REPLAY
OBS_ABS, REWARD_ABS = 1e3, 1e4      # ppo.DIVERGED_OBS_ABS / DIVERGED_REWARD_ABS
LOG_STD_MIN, LOG_STD_MAX, SQUASH_EPS = -20.0, 2.0, 1e-6
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [k, 4], key (k0, k1): Salmon et al.'s Philox4x32-10, [k, 4] uint64 words < 2^32."""
    c = [np.asarray(ctr, dtype=np.uint64)[:, i].copy() for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]   # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, 1)


def sample_indices(size, update, seed, batch):
    """(env, slot) of rows 0 .. batch-1 as salp_replay_sample draws them."""
    n = len(size)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = [[update & 0xFFFFFFFF, (update >> 32) & 0xFFFFFFFF, b, REPLAY_STREAM] for b in range(batch)]
    v = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    env, slot = np.zeros(batch, np.int64), np.zeros(batch, np.int64)
    for b in range(batch):
        e = (int(v[b, 0]) * n) >> 32
        while size[e] == 0:
            e = (e + 1) % n
        env[b], slot[b] = e, (int(v[b, 1]) * int(size[e])) >> 32
    return env, slot


class Ring:
    """The replay ring with per-env cursors; add() is salp_replay_add."""

    def __init__(self, capacity, n_envs, obs_dim):
        z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
        self.capacity, self.n_envs = capacity, n_envs
        self.obs, self.next_obs = z(capacity, n_envs, obs_dim), z(capacity, n_envs, obs_dim)
        self.actions, self.rewards, self.dones = z(capacity, n_envs, 3), z(capacity, n_envs), z(capacity, n_envs)
        self.pos, self.size = np.zeros(n_envs, np.int64), np.zeros(n_envs, np.int64)

    def add(self, obs, actions, obs_after, terminal_obs, reward, terminated, truncated, guard=True):
        bad = np.zeros(self.n_envs, bool)
        for e in range(self.n_envs):
            nxt = terminal_obs[e] if (terminated[e] or truncated[e]) else obs_after[e]
            with np.errstate(over="ignore"):
                rew = np.float32(reward[e])
            bad[e] = guard and not (np.isfinite(nxt).all() and np.isfinite(rew) and (np.abs(nxt) <= OBS_ABS).all()
                                    and abs(rew) <= REWARD_ABS)
            if bad[e]:
                continue
            p = self.pos[e]
            self.obs[p, e], self.next_obs[p, e], self.actions[p, e] = obs[e], nxt, actions[e]
            self.rewards[p, e], self.dones[p, e] = rew, 1.0 if terminated[e] else 0.0
            self.pos[e] = (p + 1) % self.capacity
            self.size[e] = min(self.size[e] + 1, self.capacity)
        return bad

    def rows(self, env, slot):
        return (self.obs[slot, env], self.actions[slot, env], self.next_obs[slot, env], self.rewards[slot, env],
                self.dones[slot, env])


def replay_script(n_envs, obs_dim, steps, seed=0):
    """`steps` synthetic env-steps for the replay tests: every flag
    combination, a staggered divergence pattern (env e diverges at steps where
    (t + e) % 3 == 0, by a NaN, a huge observation, an infinite or a huge
    reward in turn) and the last env diverging at every step."""
    g = np.random.default_rng(seed)
    out = []
    for t in range(steps):
        s = {"obs": g.standard_normal((n_envs, obs_dim)), "actions": g.uniform(-1, 1, (n_envs, 3)),
             "obs_after": g.standard_normal((n_envs, obs_dim)), "terminal_obs": g.standard_normal((n_envs, obs_dim))}
        s = {k: v.astype(np.float32) for k, v in s.items()}
        s["reward"] = g.standard_normal(n_envs) * 100
        s["terminated"] = np.array([(t + e) % 4 in (1, 3) for e in range(n_envs)], np.uint8)
        s["truncated"] = np.array([(t + e) % 4 in (2, 3) for e in range(n_envs)], np.uint8)
        for e in range(n_envs):
            if e == n_envs - 1 or (t + e) % 3 == 0:
                kind = (t + e) % 4
                row = s["terminal_obs"] if (s["terminated"][e] or s["truncated"][e]) else s["obs_after"]
                if kind == 0:
                    row[e, t % obs_dim] = np.nan
                elif kind == 1:
                    row[e, (t + 1) % obs_dim] = -1.5e3
                elif kind == 2:
                    s["reward"][e] = 1e300        # float32 inf
                else:
                    s["reward"][e] = -2e4
        out.append(s)
    return out


def actor_head(log_std, eps, a, da, dlogp):
    """float64 closed forms of include/salp.h's actor head at a given action a:
    (logp, dmu, dls)."""
    log_std, eps, a, da, dlogp = (np.asarray(x, np.float64) for x in (log_std, eps, a, da, dlogp))
    ls = np.clip(log_std, LOG_STD_MIN, LOG_STD_MAX)
    om = 1.0 - a * a
    logp = (-0.5 * eps * eps - ls - 0.5 * np.log(2 * np.pi)).sum(1) - np.log(om + SQUASH_EPS).sum(1)
    du = da * om + dlogp[:, None] * 2 * a * om / (om + SQUASH_EPS)
    inside = (log_std >= LOG_STD_MIN) & (log_std <= LOG_STD_MAX)
    return logp, du, np.where(inside, du * np.exp(ls) * eps - dlogp[:, None], 0.0)


def td_head(r, d, q1t, q2t, lpn, q1, q2, lp, log_alpha, gamma, target_entropy):
    """float64: (target, dq1, dq2, critic_loss, ent_coef_loss, d_log_alpha, alpha)."""
    r, d, q1t, q2t, lpn, q1, q2, lp = (np.asarray(x, np.float64) for x in (r, d, q1t, q2t, lpn, q1, q2, lp))
    alpha = np.exp(np.float64(log_alpha))
    t = r + (1 - d) * gamma * (np.minimum(q1t, q2t) - alpha * lpn)
    B = len(r)
    m = (lp + target_entropy).mean()
    return (t, (q1 - t) / B, (q2 - t) / B, 0.5 * (((q1 - t) ** 2).mean() + ((q2 - t) ** 2).mean()),
            -np.float64(log_alpha) * m, -m, alpha)


def pi_head(alpha, lp, q1, q2):
    """float64: (actor_loss, dlogp, dq1, dq2); a tie goes to q1."""
    lp, q1, q2 = (np.asarray(x, np.float64) for x in (lp, q1, q2))
    B = len(lp)
    first = q1 <= q2
    return ((alpha * lp - np.where(first, q1, q2)).mean(), np.full(B, alpha / B), np.where(first, -1.0 / B, 0.0),
            np.where(first, 0.0, -1.0 / B))
