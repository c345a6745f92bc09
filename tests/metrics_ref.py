"""Host restatements of include/salp.h "Episode metrics and evaluation" for the
tests: the episode window as one ``collections.deque(maxlen=window)`` per
column with the push rule of the header, its summary with ``math.fsum``, SB3's
``evaluate_policy`` bookkeeping as a Python loop, and the scripted steps the
CPU and GPU tests share."""
import collections
import math

import numpy as np

from grasp_lab_salp_amd._abi import INFO, INFO_DIM

COLS = 20
SUM_DIM = 84
FIRST, LAST = INFO["path_length"], INFO["avg_rewards_obstacle"]
# every mean, standard deviation and derived mean: within BOUND * max|x| (the derivation is in
# tests/test_metrics_host.py's docstring)
BOUND = 2.0 ** -38


class DequeWindow:
    def __init__(self, window):
        self.window = window
        self.cols = [collections.deque(maxlen=window) for _ in range(COLS)]
        self.count = 0

    def push(self, info, terminated, truncated, skip=None):
        fin = (terminated | truncated) != 0
        if skip is not None:
            fin &= skip == 0
        who = np.nonzero(fin)[0]                 # ascending: the order of `for idx, info in enumerate(infos)`
        # a deque(maxlen=window) keeps the last `window` appends: the earlier ones of a long push
        # are only counted (65 537 envs finishing at once would cost a million appends otherwise)
        self.count += max(len(who) - self.window, 0)
        for idx in who[-self.window:]:
            term = terminated[idx] != 0
            row = [info[idx, INFO["ep_return"]], info[idx, INFO["ep_len"]], 1.0 if term else 0.0,
                   1.0 if (truncated[idx] != 0 and not term) else 0.0, *info[idx, FIRST:LAST + 1]]
            for c, v in zip(self.cols, row):
                c.append(v)
            self.count += 1

    def episodes(self):
        """[n, COLS], oldest first."""
        return np.array([list(c) for c in self.cols], dtype=np.float64).T.reshape(-1, COLS)

    def rows(self):
        """The ring as the kernels lay it out: episode e in row e % window, NaN where nothing was written."""
        out = np.full((self.window, COLS), np.nan)
        ep = self.episodes()
        for k, e in enumerate(range(self.count - len(ep), self.count)):
            out[e % self.window] = ep[k]
        return out

    def summary(self):
        return summary(self.episodes())


def summary(ep):
    """([SUM_DIM] summary with math.fsum, [SUM_DIM] max|x| of what each entry was formed from)."""
    n = len(ep)
    out, scale = np.full(SUM_DIM, np.nan), np.zeros(SUM_DIM)
    out[0] = n
    if n == 0:
        return out, scale
    for c in range(COLS):
        x = [float(v) for v in ep[:, c]]
        mean = math.fsum(x) / n
        out[1 + 4 * c: 5 + 4 * c] = [mean, math.sqrt(math.fsum((v - mean) ** 2 for v in x) / n), min(x), max(x)]
        scale[1 + 4 * c: 5 + 4 * c] = max(abs(v) for v in x)
    per = [float(p) / float(l) for p, l in zip(ep[:, 4], ep[:, 1])]
    out[81], scale[81] = math.fsum(per) / n, max(abs(v) for v in per)
    good = [float(l) for l, s in zip(ep[:, 1], ep[:, 2]) if s == 1.0]
    if good:
        out[82], scale[82] = math.fsum(good) / len(good), max(good)
    out[83] = len(good)
    return out, scale


EXACT = [0, 83] + [1 + 4 * c + k for c in range(COLS) for k in (2, 3)]   # n, the success count, min, max


def assert_summary(got, want, scale, what=""):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (SUM_DIM,)
    if want[0] == 0:
        assert got[0] == 0 and np.isnan(got[1:]).all(), what
        return
    for k in range(SUM_DIM):
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (what, k)
        elif k in EXACT:
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert abs(got[k] - want[k]) <= BOUND * scale[k], (what, k, got[k], want[k], scale[k])


def make_step(rng, n_envs, finishers, skip=None, nan_payload=False):
    """One synthetic env-step: ``finishers`` a list of env indices."""
    info = rng.normal(size=(n_envs, INFO_DIM)) * rng.choice([1e-3, 1.0, 1e3], size=(1, INFO_DIM))
    info[:, INFO["ep_len"]] = rng.integers(1, 501, n_envs)
    info[:, INFO["path_length"]] = np.abs(info[:, INFO["path_length"]])
    terminated, truncated = np.zeros(n_envs, np.uint8), np.zeros(n_envs, np.uint8)
    finishers = np.asarray(finishers, dtype=np.int64)
    kind = rng.integers(0, 5, len(finishers))      # 0, 1: terminated; 2, 3: truncated; 4: both at once
    terminated[finishers] = np.isin(kind, (0, 1, 4))
    truncated[finishers] = np.isin(kind, (2, 3, 4)) * np.where(np.arange(len(finishers)) % 7 == 3, 255, 1)
    if nan_payload and len(finishers):
        row = info[finishers[0]].view(np.uint64)
        row[INFO["path_efficiency"]] = 0x7FF800000000BEEF    # a NaN with a payload: rows are bit copies
    return {"info": info, "terminated": terminated, "truncated": truncated, "skip": skip}


def finisher_counts(n_envs, window):
    return sorted({min(k, n_envs) for k in (0, 1, window - 1, window, window + 1, n_envs) if k >= 0})


def push_script(n_envs, window, seed, nan_payload=False, lanes=False):
    """Steps with 0, 1, window - 1, window, window + 1 and all envs finishing
    (twice over, so the ring wraps across pushes), one with a skip mask, and
    with ``lanes`` finishers in env 0 only, the last env only and every env."""
    rng = np.random.default_rng(seed)
    steps = []
    for rep in range(2):
        for k in finisher_counts(n_envs, window):
            who = sorted(rng.choice(n_envs, size=k, replace=False).tolist())
            steps.append(make_step(rng, n_envs, who, nan_payload=nan_payload and rep == 0))
    who = list(range(0, n_envs, 2)) or [0]
    skip = np.zeros(n_envs, np.uint8)
    skip[rng.choice(n_envs, size=max(n_envs // 3, 1), replace=False)] = 1
    steps.append(make_step(rng, n_envs, who, skip=skip))
    if lanes:
        for who in ([0], [n_envs - 1], list(range(n_envs))):
            steps.append(make_step(rng, n_envs, who))
            steps.append(make_step(rng, n_envs, who, skip=skip))
    # few envs and a long window: go on with every env finishing until the ring has wrapped
    have = episodes_in(steps)
    while have <= window + n_envs:
        steps.append(make_step(rng, n_envs, list(range(n_envs))))
        have += n_envs
    return steps


def episodes_in(steps):
    return sum(int((((s["terminated"] | s["truncated"]) != 0) & ((s["skip"] if s["skip"] is not None else 0) == 0)).sum())
               for s in steps)


# -------------------------------------------------------------- evaluation
EVAL_CASES = [(5, 1), (5, 5), (5, 8), (10, 3)]


def eval_script(n_eval, n_envs, seed):
    """Steps in which every env finishes now and then, long enough that each
    meets its target and most go on past it."""
    rng = np.random.default_rng(seed)
    steps = []
    for t in range(3 * (n_eval // n_envs + 2) + 2):
        who = [e for e in range(n_envs) if (t + e) % 3 == 2 or rng.random() < 0.2]
        steps.append(make_step(rng, n_envs, who))
    return steps


class EvalLoop:
    """SB3 evaluate_policy's loop: env i's first (n_eval + i) // n_envs episodes, slots in env order."""

    def __init__(self, n_eval, n_envs):
        self.target = [(n_eval + i) // n_envs for i in range(n_envs)]
        self.offset = [sum(self.target[:i]) for i in range(n_envs)]
        self.done = [0] * n_envs
        self.ep_return, self.ep_len = np.full(n_eval, np.nan), np.full(n_eval, np.nan)
        self.success = np.zeros(n_eval, np.uint8)
        self.remaining = n_eval

    def push(self, info, terminated, truncated, skip=None):
        for i in range(len(terminated)):
            if (terminated[i] or truncated[i]) and self.done[i] < self.target[i]:
                s = self.offset[i] + self.done[i]
                self.ep_return[s], self.ep_len[s] = info[i, INFO["ep_return"]], info[i, INFO["ep_len"]]
                self.success[s] = terminated[i] != 0
                self.done[i] += 1
                self.remaining -= 1
