"""Training callbacks for :class:`~grasp_lab_salp_amd.sac.SAC`,
:class:`~grasp_lab_salp_amd.ppo.PPO` and
:class:`~grasp_lab_salp_amd.recurrent_ppo.RecurrentPPO` with SB3's names
and constructor arguments, so the reference's training scripts
(src/train_robot.py:71-122, src/train_robot_recurrent_ppo.py:110-165) change
only their import lines::

    from grasp_lab_salp_amd.callbacks import (CheckpointCallback, EvalCallback, CallbackList,
                                              DetailedMetricsCallback)

Stable-Baselines3 is not installed here: its callback protocol is restated
(``init_callback``, ``on_training_start``, ``on_step``, ``on_training_end``;
``n_calls`` counts vec-env steps, ``num_timesteps`` transitions, so
``eval_freq=5000`` with 8 envs is every 40 000 transitions, as in the
reference run), and parity with it is unpinned.

What differs from SB3 is where the per-step work happens.  ``self.locals``
holds the step's *device* tensors (``obs``, ``actions``, ``rewards``,
``terminated``, ``truncated``, ``dones``, ``info`` [n_envs, INFO_DIM],
``diverged``), not a list of per-env info dicts, and they are overwritten two
steps later: a callback consumes them inside ``_on_step``.  ``_on_step`` runs
on the learner's collection stream.  ``logger.record(key, value)`` keeps the
value in ``model.callback_metrics`` and adds it to the learner's next
``history`` row; no TensorBoard event file is written.

:class:`~grasp_lab_salp_amd.ppo.PPO` with ``collect="chained"`` steps its envs
inside one kernel launch per collection: there is no env-step boundary on the
host to call ``on_step`` at.  It calls ``on_steps(n_steps)`` once per
collection instead: ``n_calls`` advances by ``n_steps``, ``locals`` is empty,
and ``_on_steps(first, last)`` receives the 1-based numbers of the calls
covered.  ``CheckpointCallback`` and ``EvalCallback`` then fire once if a
multiple of their frequency lies in ``[first, last]``, under the current
``num_timesteps``.  A callback that overrides ``_on_step`` but not
``_on_steps`` needs the per-step tensors: such a learner refuses it with
ValueError when training starts; it runs under ``collect="lockstep"``.

``DetailedMetricsCallback`` runs on a chained learner built with
``episode_log=True`` (or the largest window wanted): the collection kernels
then record every finished episode's window row into a per-env log
(``salp_collect_episodes``), ``locals`` is ``{"episode_log": log}``, and
``_on_steps`` merges the log into the callback's window on the device in the
order the per-step pushes would have used (``EpisodeWindow.push_log``).
Without the log it is refused like any per-step callback.
"""
import os

import numpy as np
import torch

from .metrics import EpisodeWindow, summary_dict

__all__ = ["BaseCallback", "CallbackList", "CheckpointCallback", "EvalCallback", "DetailedMetricsCallback",
           "evaluate_policy"]


class _Logger:
    """``record(key, value)`` into the model (``model.record``), as SB3's logger takes it."""

    def __init__(self, model):
        self._model = model

    def record(self, key, value, exclude=None):
        self._model.record(key, value)


class BaseCallback:
    """SB3 ``BaseCallback``: subclasses implement ``_on_step() -> bool`` (False stops training)."""

    def __init__(self, verbose=0):
        self.verbose = verbose
        self.model = None
        self.logger = None
        self.n_calls = 0
        self.num_timesteps = 0
        self.locals = {}
        self.globals = {}
        self.parent = None

    @property
    def training_env(self):
        return self.model.env

    def init_callback(self, model):
        self.model = model
        self.logger = _Logger(model)
        self.num_timesteps = model.num_timesteps
        if getattr(model, "collect", None) == "chained":
            per_step = self.per_step_only()
            if per_step:
                raise ValueError(f"{', '.join(per_step)}: _on_step needs every env-step's tensors, and the chained "
                                 "collection has no env-step boundary on the host (callbacks run once per "
                                 'collection, on_steps): build the learner with collect="lockstep" (or, for '
                                 "DetailedMetricsCallback, with episode_log=True)")
        self._init_callback()

    def _init_callback(self):
        pass

    def on_training_start(self, locals_, globals_):
        self.locals, self.globals = locals_, globals_
        self.num_timesteps = self.model.num_timesteps
        self._on_training_start()

    def _on_training_start(self):
        pass

    def on_step(self):
        self.n_calls += 1
        self.num_timesteps = self.model.num_timesteps
        self.locals = self.model.locals
        return bool(self._on_step())

    def _on_step(self):
        return True

    def on_steps(self, k):
        """``k`` vec-env steps at once (a learner without a per-step boundary
        on the host: PPO's chained collection)."""
        first = self.n_calls + 1
        self.n_calls += int(k)
        self.num_timesteps = self.model.num_timesteps
        self.locals = self.model.locals   # {} unless the learner logs episodes in its kernels ("episode_log")
        return bool(self._on_steps(first, self.n_calls))

    def _on_steps(self, first, last):
        """Calls ``first .. last`` (1-based, inclusive) have passed; False stops training."""
        return True

    def per_step_only(self):
        """Class names of the callbacks here that work per env-step only:
        ``_on_step`` overridden, ``_on_steps`` not."""
        cls = type(self)
        only = cls._on_step is not BaseCallback._on_step and cls._on_steps is BaseCallback._on_steps
        return [cls.__name__] if only else []

    @staticmethod
    def _due(freq, first, last):
        """Does a multiple of ``freq`` lie in ``[first, last]``?"""
        return last // freq > (first - 1) // freq

    def on_training_end(self):
        self._on_training_end()

    def _on_training_end(self):
        pass


class CallbackList(BaseCallback):
    """Several callbacks called in order; training stops when any of them returns False
    (all of them still see the step, as in SB3)."""

    def __init__(self, callbacks):
        super().__init__()
        self.callbacks = list(callbacks)
        for cb in self.callbacks:
            if not isinstance(cb, BaseCallback):
                raise TypeError("CallbackList: every member must be a BaseCallback")

    def _init_callback(self):
        for cb in self.callbacks:
            cb.init_callback(self.model)
            cb.parent = self.parent

    def _on_training_start(self):
        for cb in self.callbacks:
            cb.on_training_start(self.locals, self.globals)

    def _on_step(self):
        go_on = True
        for cb in self.callbacks:
            go_on = cb.on_step() and go_on
        return go_on

    def _on_steps(self, first, last):
        go_on = True
        for cb in self.callbacks:
            go_on = cb.on_steps(last - first + 1) and go_on
        return go_on

    def per_step_only(self):
        for cb in self.callbacks:   # asked before _init_callback: a member may need the learner to answer
            if cb.model is None:
                cb.model = self.model
        return [name for cb in self.callbacks for name in cb.per_step_only()]

    def _on_training_end(self):
        for cb in self.callbacks:
            cb.on_training_end()


class CheckpointCallback(BaseCallback):
    """Every ``save_freq`` calls: ``{save_path}/{name_prefix}_{num_timesteps}_steps.zip``
    (``model.save``) and, with ``save_replay_buffer``,
    ``{name_prefix}_replay_buffer_{num_timesteps}_steps.pt``."""

    def __init__(self, save_freq, save_path, name_prefix="rl_model", save_replay_buffer=False, verbose=0):
        super().__init__(verbose)
        self.save_freq = int(save_freq)
        if self.save_freq < 1:
            raise ValueError("save_freq must be >= 1")
        self.save_path, self.name_prefix = os.fspath(save_path), name_prefix
        self.save_replay_buffer = bool(save_replay_buffer)

    def _init_callback(self):
        os.makedirs(self.save_path, exist_ok=True)

    def _checkpoint_path(self, kind="", extension="zip"):
        return os.path.join(self.save_path, f"{self.name_prefix}_{kind}{self.num_timesteps}_steps.{extension}")

    def _on_step(self):
        if self.n_calls % self.save_freq == 0:
            self._save()
        return True

    def _on_steps(self, first, last):
        if self._due(self.save_freq, first, last):
            self._save()
        return True

    def _save(self):
        path = self._checkpoint_path()
        self.model.save(path)
        if self.verbose:
            print(f"Saving model checkpoint to {path}", flush=True)
        if self.save_replay_buffer:
            self.model.save_replay_buffer(self._checkpoint_path("replay_buffer_", "pt"))


class EvalCallback(BaseCallback):
    """Every ``eval_freq`` calls: ``model.evaluate(eval_env, n_eval_episodes,
    deterministic)`` (lock-step on the device; see ``SAC.evaluate``), recorded
    as ``eval/mean_reward``, ``eval/mean_ep_length`` and ``eval/success_rate``;
    ``timesteps``, ``results`` and ``ep_lengths`` appended to
    ``{log_path}/evaluations.npz``; ``{best_model_save_path}/best_model.zip``
    saved when the mean return beats ``best_mean_reward`` (strictly).
    ``eval_env`` is a vector env of this package of any size: the episodes are
    spread over its envs as SB3 spreads them, so ``SalpVecEnv(n_eval_episodes)``
    runs them all at once.  Rendering is not built."""

    def __init__(self, eval_env, n_eval_episodes=5, eval_freq=10000, log_path=None, best_model_save_path=None,
                 deterministic=True, render=False, verbose=1):
        super().__init__(verbose)
        if render:
            raise NotImplementedError("EvalCallback(render=True): rendering is not built")
        sim = getattr(eval_env, "sim", eval_env)
        if not all(hasattr(sim, a) for a in ("step", "reset", "n_envs", "obs_dim", "params", "device")):
            raise TypeError(f"EvalCallback: eval_env must be a SalpVecEnv or BatchedSalpEnv, not "
                            f"{type(eval_env).__name__}: evaluation steps a batch of envs on the device; build one "
                            "with SalpVecEnv(n_eval_episodes)")
        self.eval_env = eval_env
        self.n_eval_episodes, self.eval_freq = int(n_eval_episodes), int(eval_freq)
        if self.eval_freq < 1 or self.n_eval_episodes < 1:
            raise ValueError("eval_freq and n_eval_episodes must be >= 1")
        self.deterministic = bool(deterministic)
        self.best_model_save_path = None if best_model_save_path is None else os.fspath(best_model_save_path)
        self.log_path = None if log_path is None else os.path.join(os.fspath(log_path), "evaluations")
        self.best_mean_reward, self.last_mean_reward = -np.inf, -np.inf
        self.evaluations_timesteps, self.evaluations_results, self.evaluations_length = [], [], []

    def _init_callback(self):
        if self.best_model_save_path is not None:
            os.makedirs(self.best_model_save_path, exist_ok=True)
        if self.log_path is not None:
            os.makedirs(os.path.dirname(self.log_path), exist_ok=True)

    def _on_step(self):
        if self.n_calls % self.eval_freq == 0:
            self._evaluate()
        return True

    def _on_steps(self, first, last):
        if self._due(self.eval_freq, first, last):
            self._evaluate()
        return True

    def _evaluate(self):
        returns, lengths = self.model.evaluate(self.eval_env, n_eval_episodes=self.n_eval_episodes,
                                               deterministic=self.deterministic, return_episode_rewards=True)
        successes = (getattr(self.model, "last_eval", None) or {}).get("successes")
        if self.log_path is not None:
            self.evaluations_timesteps.append(self.num_timesteps)
            self.evaluations_results.append(list(returns))
            self.evaluations_length.append(list(lengths))
            np.savez(self.log_path, timesteps=self.evaluations_timesteps, results=self.evaluations_results,
                     ep_lengths=self.evaluations_length)
        mean, std = float(np.mean(returns)), float(np.std(returns))
        self.last_mean_reward = mean
        if self.verbose:
            print(f"Eval num_timesteps={self.num_timesteps}, episode_reward={mean:.2f} +/- {std:.2f}, "
                  f"episode length {np.mean(lengths):.2f}", flush=True)
        self.logger.record("eval/mean_reward", mean)
        self.logger.record("eval/mean_ep_length", float(np.mean(lengths)))
        if successes is not None:
            self.logger.record("eval/success_rate", float(np.mean(successes)))
        if mean > self.best_mean_reward:
            self.best_mean_reward = mean
            if self.best_model_save_path is not None:
                self.model.save(os.path.join(self.best_model_save_path, "best_model"))


# (recorded key, summary key) in the order of src/tensorboard_callback.py:136-205
_SUMMARY_KEYS = (
    ("custom/navigation/success_rate", "success/mean"), ("custom/navigation/truncation_rate", "truncation/mean"),
    ("custom/navigation/avg_final_distance", "final_distance/mean"), ("custom/path/path_length", "path_length/mean"),
    ("custom/path/direct_distance", "direct_distance/mean"), ("custom/path/efficiency", "path_efficiency/mean"),
    ("custom/path/target_distance", "initial_distance/mean"), ("custom/performance/avg_cycles", "ep_len/mean"),
    ("custom/performance/distance_per_cycle", "distance_per_cycle"),
    ("custom/performance/cycles_to_success", "cycles_to_success"),
    ("custom/actions/avg_compression", "avg_compression/mean"), ("custom/actions/compression_std", "avg_compression/std"),
    ("custom/actions/avg_coast_time", "avg_coast_time/mean"), ("custom/actions/avg_nozzle_angle", "avg_nozzle_angle/mean"),
    ("custom/actions/nozzle_angle_std", "avg_nozzle_angle/std"), ("custom/motion/avg_velocity", "avg_velocity/mean"),
    ("reward/stats/total_mean", "ep_return/mean"), ("reward/stats/total_std", "ep_return/std"),
    ("reward/stats/best_episode_reward", "ep_return/max"),
) + tuple((f"reward/components/{k}", f"avg_rewards_{k}/mean")
          for k in ("track", "heading", "smooth", "yaw", "time", "sideslip", "obstacle"))


class DetailedMetricsCallback(BaseCallback):
    """The reference's ``DetailedMetricsCallback`` (src/tensorboard_callback.py)
    without its per-step host work: ``_on_step`` is one
    :meth:`EpisodeWindow.push <grasp_lab_salp_amd.metrics.EpisodeWindow.push>` of
    the step's device tensors (episodes of envs whose transition the divergence
    guard dropped are not logged), and every ``log_freq`` calls, if the window
    holds an episode, one ``summary()`` (one launch, one host copy) is recorded
    under the reference's names: ``custom/navigation/*``, ``custom/path/*``,
    ``custom/performance/*`` (``cycles_to_success`` only when the window holds
    a success), ``custom/actions/*``, ``custom/motion/avg_velocity`` and
    ``reward/stats/*``.  ``window``: the reference's deque length, 100.

    One deviation: the reference reads ``avg_r_track`` and its siblings from
    the info dict, which its env never emits (it emits ``avg_rewards_*``), so
    it logs no reward component.  Here the seven ``avg_rewards_*`` columns are
    recorded as ``reward/components/<name>`` (track, heading, smooth, yaw,
    time, sideslip, obstacle)."""

    def __init__(self, log_freq=1000, verbose=0, window=100, fused=None):
        super().__init__(verbose)
        self.log_freq = int(log_freq)
        if self.log_freq < 1:
            raise ValueError("log_freq must be >= 1")
        self.window_size, self.fused = int(window), fused
        self.window = None
        self.last_summary = None

    def per_step_only(self):
        """On a chained learner the window is fed from the learner's in-kernel
        episode log; without one this callback needs every env-step."""
        return [] if getattr(self.model, "episode_log", 0) else [type(self).__name__]

    def _init_callback(self):
        w = getattr(self.model, "episode_log", 0)
        if getattr(self.model, "collect", None) == "chained" and self.window_size > w:
            raise ValueError(f"DetailedMetricsCallback(window={self.window_size}): the learner's episode log is sized "
                             f"for windows up to {w}; build it with episode_log={self.window_size}")
        if self.window is None or self.window.device != self.model.device:
            fused = getattr(self.model, "fused", None) if self.fused is None else self.fused
            self.window = EpisodeWindow(self.window_size, self.model.device, fused=fused)

    def _on_step(self):
        lo = self.locals
        self.window.push(lo["info"], lo["terminated"], lo["truncated"], skip=lo["diverged"])
        if self.n_calls % self.log_freq == 0:
            s = self.window.summary()
            if s["n"] > 0:
                self._record(s)
        return True

    def _record(self, s):
        self.last_summary = s
        for key, name in _SUMMARY_KEYS:
            if name == "cycles_to_success" and s["n_success"] == 0:
                continue
            self.logger.record(key, s[name])

    def _on_steps(self, first, last):
        self.window.push_log(self.locals["episode_log"])
        if self._due(self.log_freq, first, last):
            # one host copy for the summary and the lost counter together
            host = torch.cat([self.window.summary_tensor(), self.window.lost.to(torch.float64)]).tolist()
            s, lost = summary_dict(host[:-1]), int(host[-1])
            if s["n"] > 0:
                self._record(s)
            if lost:
                self.logger.record("custom/episodes_lost", lost)
        return True


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False):
    """SB3's ``evaluate_policy``: ``model.evaluate(env, ...)``."""
    return model.evaluate(env, n_eval_episodes=n_eval_episodes, deterministic=deterministic,
                          return_episode_rewards=return_episode_rewards)
