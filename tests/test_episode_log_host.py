"""The merge of a chained collection's episode log into the episode window
(metrics.torch_episode_window_push_log, the readable restatement of
salp_episode_window_push_log) against a plain Python replay, and the learner's
episode_log surface that needs no GPU.

The replay sorts the full episode list by (step, env) and appends it to a
``deque(maxlen=W)``, counting episodes so that it knows the ring row
``(c + r) % W`` each one lands in.  The logs are synthetic: built from that
full list, so the test knows which episodes a short per-env ring dropped."""
import collections
import math
import random

import pytest
import torch

from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd.callbacks import CallbackList, DetailedMetricsCallback
from grasp_lab_salp_amd.metrics import EpisodeLog, EpisodeWindow, torch_episode_window_push_log
from grasp_lab_salp_amd.ppo import PPO, episode_log_per_env
from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO

COLS = _lib.EPWIN_COLS


def _row(t, i):
    """A row that names its episode (exact in fp64)."""
    return [float(1000 * t + i) + 0.25 * c for c in range(COLS)]


def _make_log(episodes, n, K):
    """episodes: {env: [steps, ascending]} -> (EpisodeLog on the CPU, the kept (t, i) set)."""
    log = EpisodeLog(n, K, "cpu")
    kept = set()
    for i, steps in episodes.items():
        log.count[i] = len(steps)
        for e, t in enumerate(steps):
            log.rows[i, e % K] = torch.tensor(_row(t, i), dtype=torch.float64)
            log.step[i, e % K] = t
        kept |= {(t, i) for t in steps[-K:]}
    return log, kept


def _replay(rows0, count0, episodes, W):
    """The lock-step pushes: every episode in (t, i) order into the ring."""
    rows = [list(r) for r in rows0]
    order = sorted((t, i) for i, steps in episodes.items() for t in steps)
    dq = collections.deque(maxlen=W)
    c = count0
    for t, i in order:
        rows[c % W] = _row(t, i)
        dq.append((t, i))
        c += 1
    return rows, c, order, dq


def _lost_rule(episodes, kept, K, W):
    """include/salp.h: an env that dropped episodes counts once if its oldest kept
    episode is among the last W kept keys."""
    top = set(sorted(kept)[-W:])
    return sum(1 for i, steps in episodes.items() if len(steps) > K and (steps[-K], i) in top)


def _same(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (a.isnan() & b.isnan())).all())


def _check(episodes, n, K, W, count0=0):
    log, kept = _make_log(episodes, n, K)
    win = EpisodeWindow(W, "cpu", fused=False)
    # a window that already holds count0 episodes, with rows that name them
    for e in range(max(0, count0 - W), count0):
        win.rows[e % W] = torch.tensor([-(e + 1.0)] * COLS, dtype=torch.float64)
    win.count.fill_(count0)
    rows0 = win.rows.tolist()
    win.push_log(log, n)
    D = sum(len(s) for s in episodes.values())
    want_rows, want_count, order, dq = _replay(rows0, count0, episodes, W)
    assert int(win.count) == want_count == count0 + D
    lost = int(win.lost)
    assert lost == _lost_rule(episodes, kept, K, W)
    if lost == 0:
        # the guarantee: exact whenever nothing is reported lost
        assert _same(win.rows, want_rows), (n, K, W, count0)
        # ... which holds the deque built from the full list in its newest rows
        newest = range(want_count - len(dq), want_count)
        assert [win.rows[e % W, 0].item() for e in newest] == [float(1000 * t + i) for t, i in dq]
    else:
        # what the rule promises when episodes are missing: the kept ones still land in their true rows
        # as long as nothing dropped lies above them
        dropped = set(order) - kept
        for r, (t, i) in enumerate(order):
            if r >= D - W and (t, i) in kept and not any(d > (t, i) for d in dropped):
                assert win.rows[(count0 + r) % W].tolist() == _row(t, i)
    return lost


def _random_episodes(rng, n, n_steps, p):
    return {i: sorted(t for t in range(n_steps) if rng.random() < p) for i in range(n)}


@pytest.mark.parametrize("W", [1, 7, 100])
def test_designed_cases(W):
    n, T = 13, 24
    rng = random.Random(W)
    # D = 0
    assert _check({i: [] for i in range(n)}, n, 3, W, count0=5) == 0
    # D < W, D == W, D > W with K large enough to keep everything
    full = _random_episodes(rng, n, T, 0.5)
    flat = sorted((t, i) for i, s in full.items() for t in s)
    for D in (max(W - 1, 0), W, W + 5, len(flat)):
        take = set(flat[:D])
        eps = {i: [t for t in s if (t, i) in take] for i, s in full.items()}
        for count0 in (0, W + 3, 2 * W + 1):       # a count on entry that is not a multiple of W (W > 1)
            assert _check(eps, n, T, W, count0) == 0
    # K = 1 and K = 2 with wrapped rings
    for K in (1, 2):
        _check(full, n, K, W, count0=3)
    # one env holds most of the last W
    eps = {i: [] for i in range(n)}
    eps[4] = list(range(T))
    eps[9] = [0, 5, 23]
    for K in (1, 2, 24):
        lost = _check(eps, n, K, W, count0=11)
        assert lost == 0 if K == 24 else True
    # many envs finish in the last step only
    eps = {i: [T - 1] for i in range(n)}
    eps[0] = [2, T - 1]
    for K in (1, 2):
        _check(eps, n, K, W, count0=1)


def test_generated_cases_keep_the_guarantee():
    rng = random.Random(7)
    seen = {"lost": 0, "exact_with_drops": 0}
    for case in range(150):
        n, T = rng.choice([1, 2, 5, 33, 70]), rng.choice([1, 4, 24])
        K, W = rng.choice([1, 2, 3, T]), rng.choice([1, 7, 100])
        eps = _random_episodes(rng, n, T, rng.choice([0.05, 0.3, 0.9]))
        lost = _check(eps, n, K, W, count0=rng.choice([0, 1, W, 3 * W + 2]))
        drops = any(len(s) > K for s in eps.values())
        seen["lost"] += lost > 0
        seen["exact_with_drops"] += lost == 0 and drops
    assert seen["lost"] > 0 and seen["exact_with_drops"] > 0   # both sides of the rule were exercised


def test_two_pushes_accumulate():
    W, n, T = 7, 5, 6
    rng = random.Random(1)
    win = EpisodeWindow(W, "cpu", fused=False)
    dq, c = collections.deque(maxlen=W), 0
    for _ in range(3):
        eps = _random_episodes(rng, n, T, 0.4)
        log, _ = _make_log(eps, n, T)
        win.push_log(log)
        for t, i in sorted((t, i) for i, s in eps.items() for t in s):
            dq.append((c % W, _row(t, i)))
            c += 1
    assert int(win.count) == c and int(win.lost) == 0
    for row, want in dq:
        assert win.rows[row].tolist() == want


def test_log_sizing():
    assert episode_log_per_env(64, 16, 100) == 16          # min(n_steps, W): can never lose an episode
    assert episode_log_per_env(64, 2048, 100) == 100
    assert episode_log_per_env(32768, 256, 100) == 2       # config 5: 65 536 rows, 10.9 MB with step and count
    assert episode_log_per_env(100000, 256, 100) == 2
    assert EpisodeLog(3, 2, "cpu").rows.isnan().all() and int(EpisodeLog(3, 2, "cpu").step.max()) == -1
    with pytest.raises(ValueError):
        EpisodeLog(3, 0, "cpu")


class _Sim:
    """What PPO's constructor reads of an env."""
    n_envs, obs_dim, device = 4, 10, torch.device("cpu")


class _Chained:
    """A learner as a callback sees it."""
    collect, num_timesteps, device, fused = "chained", 0, torch.device("cpu"), False

    def __init__(self, episode_log):
        self.episode_log = episode_log


def test_learner_surface_without_a_gpu():
    with pytest.raises(ValueError, match="episode_log"):
        PPO("MlpPolicy", _Sim(), n_steps=8, batch_size=8, collect="lockstep", episode_log=True)
    with pytest.raises(ValueError, match="episode_log"):
        PPO("MlpPolicy", _Sim(), n_steps=8, batch_size=8, collect="chained", episode_log=50)   # a CPU learner
    m = PPO("MlpPolicy", _Sim(), n_steps=8, batch_size=8, collect="lockstep")
    assert m.episode_log == 0 and m._episode_log is None and m.locals == {}
    with pytest.raises(ValueError, match="episode_log"):
        RecurrentPPO("MlpLstmPolicy", _Sim(), n_steps=16, batch_size=16, episode_log=True)
    # the refusal on a chained learner without a log is kept, for the callback alone and in a list
    for cb in (DetailedMetricsCallback(), CallbackList([DetailedMetricsCallback()])):
        with pytest.raises(ValueError, match='DetailedMetricsCallback.*collect="lockstep"'):
            cb.init_callback(_Chained(0))
    # with a log: accepted up to the log's window, refused beyond it
    DetailedMetricsCallback(window=100, fused=False).init_callback(_Chained(100))
    CallbackList([DetailedMetricsCallback(window=50, fused=False)]).init_callback(_Chained(100))
    with pytest.raises(ValueError, match="episode_log=200"):
        DetailedMetricsCallback(window=200, fused=False).init_callback(_Chained(100))


def test_save_load_round_trip_of_the_key(tmp_path):
    import json
    import zipfile
    m = PPO("MlpPolicy", _Sim(), n_steps=8, batch_size=8, collect="lockstep")
    path = m.save(tmp_path / "m")
    data = json.loads(zipfile.ZipFile(path).read("data.json"))
    assert data["episode_log"] == 0 and data["version"] == PPO.FORMAT_VERSION == 1
    assert PPO.load(path, env=_Sim()).episode_log == 0
    # a file that says 100 loads as 0 where the collection is lock-step (no GPU), a file without the key as 0,
    # and an explicit keyword overrides the file
    for value in (100, None):
        if value is None:
            del data["episode_log"]
        else:
            data["episode_log"] = value
        other = str(tmp_path / f"o{value}.zip")
        with zipfile.ZipFile(path) as zin, zipfile.ZipFile(other, "w") as zout:
            for name in zin.namelist():
                zout.writestr(name, json.dumps(data) if name == "data.json" else zin.read(name))
        assert PPO.load(other, env=_Sim()).episode_log == 0
        with pytest.raises(ValueError, match="episode_log"):
            PPO.load(other, env=_Sim(), episode_log=True)


def test_restatement_handles_nan_rows_bit_for_bit():
    log = EpisodeLog(2, 2, "cpu")
    log.count[:] = torch.tensor([1, 1], dtype=torch.int32)
    log.step[:, 0] = torch.tensor([3, 3], dtype=torch.int32)
    log.rows[0, 0] = 1.0
    log.rows[1, 0] = 2.0
    log.rows[1, 0, 5] = math.nan
    win = EpisodeWindow(7, "cpu", fused=False)
    rows, count, lost = torch_episode_window_push_log(win.rows, win.count, win.lost, log.rows, log.step, log.count)
    assert int(count) == 2 and int(lost) == 0
    assert rows[0].tolist() == [1.0] * COLS and rows[1, 0] == 2.0 and rows[1, 5].isnan() and rows[2].isnan().all()
