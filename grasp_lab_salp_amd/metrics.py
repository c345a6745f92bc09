"""Episode metrics and evaluation bookkeeping in device memory
(include/salp.h "Episode metrics and evaluation", csrc/salp_metrics.hip).

The reference's ``DetailedMetricsCallback`` (src/tensorboard_callback.py)
keeps a ``deque(maxlen=100)`` per metric and walks the vec-env's list of info
dicts on every env-step; SB3's ``evaluate_policy`` does the same for its
episode returns.  Here both are one kernel launch per env-step on the step's
device tensors, without a host copy:

* :class:`EpisodeWindow`: a ring of the last ``window`` finished episodes
  (20 columns each) and their summary statistics;
* :class:`EvalAccount`: the first ``target[i]`` episodes of every env into
  ``n_eval_episodes`` slots, and how many are still missing.

``fused=True`` (the default on a GPU) runs the HIP kernels; ``fused=False``
computes the same from torch ops (``torch_episode_window_push``,
``torch_episode_window_summary``, ``torch_eval_account``): the readable
restatement, and the path that runs on the CPU.  The rows and counters of the
two agree bit for bit; the summaries agree to rounding.
"""
import ctypes
import math

import torch

from . import _lib
from ._abi import INFO, INFO_DIM, INFO_KEYS

__all__ = ["EpisodeWindow", "EpisodeLog", "EvalAccount", "ROW_KEYS", "SUMMARY_STATS", "torch_episode_window_push",
           "torch_episode_window_push_log", "torch_episode_window_summary", "torch_eval_account", "eval_targets",
           "summary_dict"]

_FIRST, _LAST = INFO["path_length"], INFO["avg_rewards_obstacle"]
# column names of a window row (include/salp.h SalpEpisodeWindow)
ROW_KEYS = ("ep_return", "ep_len", "success", "truncation") + tuple(INFO_KEYS[_FIRST:_LAST + 1])
SUMMARY_STATS = ("mean", "std", "min", "max")
assert len(ROW_KEYS) == _lib.EPWIN_COLS and _lib.EPSUM_DIM == 1 + 4 * _lib.EPWIN_COLS + 3
_EP_RETURN, _EP_LEN = INFO["ep_return"], INFO["ep_len"]
_PATH, _LEN, _SUCCESS = ROW_KEYS.index("path_length"), ROW_KEYS.index("ep_len"), ROW_KEYS.index("success")


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _fused(fused, device, what):
    on = device.type == "cuda" if fused is None else bool(fused)
    if on and device.type != "cuda":
        raise ValueError(f"{what}: fused=True runs HIP kernels: it needs a ROCm GPU device")
    return on


def _check_step(what, device, n, info, terminated, truncated, skip=None):
    for name, t, shape, dt in (("info", info, (n, INFO_DIM), torch.float64), ("terminated", terminated, (n,), torch.uint8),
                               ("truncated", truncated, (n,), torch.uint8), ("skip", skip, (n,), torch.uint8)):
        if t is None and name == "skip":
            continue
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{what}: {name!r} must be a contiguous {dt} tensor of shape {shape} on {device}")


# ------------------------------------------------- plain torch restatements
def torch_episode_window_push(rows, count, info, terminated, truncated, skip=None):
    """``salp_episode_window_push`` (include/salp.h) as torch ops without a
    host sync, in place on ``rows`` [window, 20] f64 and ``count`` [1] int64."""
    window = rows.shape[0]
    term, trunc = terminated != 0, truncated != 0
    fin = term | trunc
    if skip is not None:
        fin = fin & (skip == 0)
    rank = torch.cumsum(fin.to(torch.int64), 0) - 1      # among the finishers, in env order
    total = fin.sum()
    write = fin & (rank >= total - window)                # the last `window` of them: distinct rows
    new = torch.cat([info[:, _EP_RETURN:_EP_RETURN + 1], info[:, _EP_LEN:_EP_LEN + 1],
                     term.to(rows.dtype).unsqueeze(1), (trunc & ~term).to(rows.dtype).unsqueeze(1),
                     info[:, _FIRST:_LAST + 1]], dim=1)
    # envs that do not write go to one row past the ring, which is dropped
    row = torch.where(write, (count + rank) % window, torch.full_like(rank, window))
    ring = torch.cat([rows, rows.new_zeros(1, rows.shape[1])])
    ring[row] = new
    rows.copy_(ring[:window])
    count += total
    return rows, count


def torch_episode_window_push_log(rows, count, lost, log_rows, log_step, log_count):
    """``salp_episode_window_push_log`` (include/salp.h) as torch ops without a
    host sync, in place on ``rows`` [window, 20] f64, ``count`` and ``lost``
    [1] int64.  The log: ``log_rows`` [n, K, 20] f64, ``log_step`` [n, K] and
    ``log_count`` [n] int32.  The kept episodes are sorted by (step, env) from
    the top; the g-th from the top is episode ``count + D - 1 - g``."""
    window, (n, K) = rows.shape[0], log_step.shape
    dev = rows.device
    cnt = log_count.to(torch.int64).clamp(min=0).unsqueeze(1)             # [n, 1]
    slot = torch.arange(K, device=dev).unsqueeze(0)                        # [1, K]
    kept = slot < cnt
    # a wrapped ring's slot holds the env's latest episode e with e % K == slot
    e = (cnt - 1) // K * K + slot
    e = torch.where(e > cnt - 1, e - K, e)
    oldest_of_dropper = kept & (cnt > K) & (e == cnt - K)
    env = torch.arange(n, device=dev).unsqueeze(1)
    key = torch.where(kept, log_step.to(torch.int64) * n + env, torch.full_like(e, -1)).reshape(-1)
    D, M = cnt.sum(), kept.sum()
    S = min(window, n * K)
    top = torch.argsort(key, descending=True)[:S]                          # distinct keys: the kept ones first
    g = torch.arange(S, device=dev)
    valid = g < M
    row = torch.where(valid, (count + D - 1 - g) % window, torch.full_like(g, window))
    # candidates that do not write go to one row past the ring, which is dropped
    ring = torch.cat([rows, rows.new_zeros(1, rows.shape[1])])
    ring[row] = log_rows.reshape(n * K, -1)[top]
    rows.copy_(ring[:window])
    lost += (valid & oldest_of_dropper.reshape(-1)[top]).sum()
    count += D
    return rows, count, lost


def torch_episode_window_summary(rows, count):
    """``salp_episode_window_summary`` as torch ops: [84] f64, same layout."""
    window = rows.shape[0]
    n = torch.clamp(count.reshape(()), max=window)
    valid = (torch.arange(window, device=rows.device) < n).unsqueeze(1)
    nf = n.to(rows.dtype)
    zero, nan = rows.new_zeros(()), rows.new_full((), math.nan)
    x = torch.where(valid, rows, zero)
    mean = x.sum(0) / nf
    std = torch.sqrt(torch.where(valid, (rows - mean) ** 2, zero).sum(0) / nf)
    lo = torch.where(valid, rows, rows.new_full((), math.inf)).min(0).values
    hi = torch.where(valid, rows, rows.new_full((), -math.inf)).max(0).values
    per = torch.where(valid[:, 0], rows[:, _PATH] / rows[:, _LEN], zero).sum() / nf
    ok = valid[:, 0] & (rows[:, _SUCCESS] == 1.0)
    k = ok.sum().to(rows.dtype)
    to_success = torch.where(k > 0, torch.where(ok, rows[:, _LEN], zero).sum() / k, nan)
    out = torch.cat([nf.reshape(1), torch.stack([mean, std, lo, hi], 1).reshape(-1), per.reshape(1),
                     to_success.reshape(1), k.reshape(1)])
    empty = torch.cat([torch.zeros(1, dtype=torch.bool, device=rows.device),
                       (n == 0).expand(_lib.EPSUM_DIM - 1)])
    return torch.where(empty, nan, out)


def eval_targets(n_eval_episodes, n_envs):
    """SB3 ``evaluate_policy``'s ``episode_count_targets`` and their exclusive prefix (host lists)."""
    target = [(int(n_eval_episodes) + i) // int(n_envs) for i in range(int(n_envs))]
    offset = [sum(target[:i]) for i in range(len(target))]
    return target, offset


def torch_eval_account(state, info, terminated, truncated):
    """``salp_eval_account`` as torch ops in place on ``state``, a dict of
    target, offset, done_count, ep_return, ep_len, success, remaining."""
    fin = ((terminated | truncated) != 0) & (state["done_count"] < state["target"])
    n_slots = state["ep_return"].numel()
    slot = torch.where(fin, state["offset"] + state["done_count"], torch.full_like(state["offset"], n_slots))
    for key, new in (("ep_return", info[:, _EP_RETURN]), ("ep_len", info[:, _EP_LEN]),
                     ("success", (terminated != 0).to(torch.uint8))):
        ext = torch.cat([state[key], state[key].new_zeros(1)])
        ext[slot] = new
        state[key].copy_(ext[:n_slots])
    state["done_count"] += fin.to(torch.int32)
    state["remaining"] -= fin.sum()
    return state


def summary_dict(out):
    """The [84] summary (a host sequence) keyed by name: ``n``, ``<column>/<stat>``
    for every column of :data:`ROW_KEYS` and stat of :data:`SUMMARY_STATS`,
    ``distance_per_cycle``, ``cycles_to_success``, ``n_success``."""
    out = [float(v) for v in out]
    d = {"n": int(out[0])}
    for c, key in enumerate(ROW_KEYS):
        for s, stat in enumerate(SUMMARY_STATS):
            d[f"{key}/{stat}"] = out[1 + 4 * c + s]
    d["distance_per_cycle"], d["cycles_to_success"] = out[81], out[82]
    d["n_success"] = 0 if math.isnan(out[83]) else int(out[83])
    return d


# ------------------------------------------------------------------ classes
class EpisodeWindow:
    """The last ``window`` finished episodes of a vector env, on ``device``.

    ``rows`` [window, 20] f64 (columns :data:`ROW_KEYS`; NaN until written) and
    ``count`` [1] int64 (episodes pushed since creation); episode ``e`` lives in
    row ``e % window``.  :meth:`push` is one launch and no host traffic;
    :meth:`summary` is one launch and one host copy."""

    def __init__(self, window=100, device="cuda", fused=None):
        self.window = int(window)
        if not 1 <= self.window <= _lib.EPWIN_MAX_WINDOW:
            raise ValueError(f"window must be in 1 .. {_lib.EPWIN_MAX_WINDOW}")
        self.device = _device(device)
        self.fused = _fused(fused, self.device, "EpisodeWindow")
        self.rows = torch.full((self.window, _lib.EPWIN_COLS), math.nan, dtype=torch.float64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.lost = torch.zeros(1, dtype=torch.int64, device=self.device)   # push_log: envs whose dropped episodes may be missing
        self._c = None
        if self.fused:
            self._c = _lib.SalpEpisodeWindow(self.window, 0, self.rows.data_ptr(), self.count.data_ptr())
            self._out = torch.empty(_lib.EPSUM_DIM, dtype=torch.float64, device=self.device)

    def push(self, info, terminated, truncated, skip=None):
        """One env-step of every env: ``info`` [n, INFO_DIM] f64, ``terminated``
        / ``truncated`` / ``skip`` [n] u8 as ``BatchedSalpEnv.step(out=...)``
        and ``ReplayBuffer.add`` write them.  Envs with (terminated |
        truncated) and no skip byte are appended in env order."""
        if not self.fused:
            torch_episode_window_push(self.rows, self.count, info, terminated, truncated, skip)
            return
        n = info.shape[0]
        _check_step("EpisodeWindow.push", self.device, n, info, terminated, truncated, skip)
        p = _lib.SalpEpisodePush(n, info.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                                 skip.data_ptr() if skip is not None else None)
        _lib.check(_lib.load().salp_episode_window_push(ctypes.byref(self._c), ctypes.byref(p), _stream(self.device)))

    def push_log(self, log, n_envs=None):
        """One chained collection's :class:`EpisodeLog`: the window afterwards
        is what a :meth:`push` after every env-step of the collection would
        have left, unless an env finished more episodes than the log keeps and
        one of the dropped ones might have belonged to the window; ``lost``
        [1] int64 counts those envs (0: the window is exact).  One launch, no
        host traffic."""
        n = log.n_envs if n_envs is None else int(n_envs)
        if n != log.n_envs or log.device != self.device:
            raise ValueError(f"EpisodeWindow.push_log: the log holds {log.n_envs} envs on {log.device}")
        if not self.fused:
            torch_episode_window_push_log(self.rows, self.count, self.lost, log.rows, log.step, log.count)
            return
        _lib.check(_lib.load().salp_episode_window_push_log(ctypes.byref(self._c), ctypes.byref(log.c_struct()), n,
                                                            ctypes.c_void_p(self.lost.data_ptr()),
                                                            _stream(self.device)))

    def summary_tensor(self):
        """The [84] summary on the device (include/salp.h salp_episode_window_summary)."""
        if not self.fused:
            return torch_episode_window_summary(self.rows, self.count)
        _lib.check(_lib.load().salp_episode_window_summary(ctypes.byref(self._c),
                                                           ctypes.c_void_p(self._out.data_ptr()),
                                                           _stream(self.device)))
        return self._out

    def summary(self):
        """:func:`summary_dict` of the window (synchronises: one host copy)."""
        return summary_dict(self.summary_tensor().tolist())


class EpisodeLog:
    """The caller-owned log of ``salp_collect_episodes`` (include/salp.h):
    ``rows`` [n_envs, per_env, 20] f64 (NaN until written), ``step`` [n_envs,
    per_env] int32 (-1 until written) and ``count`` [n_envs] int32.  Env ``i``'s
    ``e``-th episode of a collection is in slot ``e % per_env``;
    :meth:`BatchedSalpEnv.collect(..., episode_log=log)
    <grasp_lab_salp_amd.batched_env.BatchedSalpEnv.collect>` fills it and
    :meth:`EpisodeWindow.push_log` merges it."""

    def __init__(self, n_envs, per_env, device="cuda"):
        self.n_envs, self.per_env = int(n_envs), int(per_env)
        if self.n_envs < 1 or self.per_env < 1:
            raise ValueError("n_envs and per_env must be positive")
        self.device = _device(device)
        self.rows = torch.full((self.n_envs, self.per_env, _lib.EPWIN_COLS), math.nan, dtype=torch.float64,
                               device=self.device)
        self.step = torch.full((self.n_envs, self.per_env), -1, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)

    def c_struct(self):
        return _lib.SalpEpisodeLog(self.per_env, self.rows.data_ptr(), self.step.data_ptr(), self.count.data_ptr())


class EvalAccount:
    """SB3 ``evaluate_policy``'s bookkeeping for ``n_envs`` envs stepped in
    lock-step: env ``i`` contributes its first ``(n_eval_episodes + i) //
    n_envs`` episodes, into slots in env order.  :meth:`push` is one launch per
    env-step; ``remaining`` [1] int64 counts the episodes still missing."""

    def __init__(self, n_eval_episodes, n_envs, device="cuda", fused=None):
        self.n_eval_episodes, self.n_envs = int(n_eval_episodes), int(n_envs)
        if self.n_eval_episodes < 1 or self.n_envs < 1:
            raise ValueError("n_eval_episodes and n_envs must be positive")
        self.device = _device(device)
        self.fused = _fused(fused, self.device, "EvalAccount")
        target, offset = eval_targets(self.n_eval_episodes, self.n_envs)
        dev, N = self.device, self.n_eval_episodes
        self.target = torch.tensor(target, dtype=torch.int32, device=dev)
        self.offset = torch.tensor(offset, dtype=torch.int64, device=dev)
        self.done_count = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        self.ep_return = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
        self.ep_len = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
        self.success = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.remaining = torch.full((1,), N, dtype=torch.int64, device=dev)
        self.max_target = max(target)
        self._c = None
        if self.fused:
            self._c = _lib.SalpEvalState(self.n_envs, *(t.data_ptr() for t in (
                self.target, self.offset, self.done_count, self.ep_return, self.ep_len, self.success, self.remaining)))

    def _state(self):
        return {k: getattr(self, k) for k in ("target", "offset", "done_count", "ep_return", "ep_len", "success",
                                              "remaining")}

    def push(self, info, terminated, truncated):
        if not self.fused:
            torch_eval_account(self._state(), info, terminated, truncated)
            return
        _check_step("EvalAccount.push", self.device, self.n_envs, info, terminated, truncated)
        p = _lib.SalpEpisodePush(self.n_envs, info.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), None)
        _lib.check(_lib.load().salp_eval_account(ctypes.byref(self._c), ctypes.byref(p), _stream(self.device)))

    def left(self):
        """Episodes still missing (host int; synchronises)."""
        return int(self.remaining)
