"""grasp_lab_salp_amd/metrics.py on the CPU (fused=False): the torch
restatements of include/salp.h "Episode metrics and evaluation" against the
deque / fsum / Python-loop restatements of tests/metrics_ref.py.

Rows and counters are compared bit for bit.  The summary's bound, 2^-38 max|x|
(metrics_ref.BOUND), for n <= 1024 = 2^10 doubles and unit roundoff 2^-53: a
sum in any order errs by at most 2^-43 n max|x|, so the mean by 2^-43 max|x|;
each deviation carries that error, the deviations' errors enter the
root-mean-square at most once and the sum of squares adds a 2^-42 relative
term, so the standard deviation errs by at most 2^-41 max|x|; 8x is left for
the divisions and the square root.  n, min, max and the success count are exact."""
import numpy as np
import pytest
import torch

import metrics_ref
from grasp_lab_salp_amd import metrics


def _t(step):
    return {k: (None if v is None else torch.from_numpy(v)) for k, v in step.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("window", [1, 3, 100])
@pytest.mark.parametrize("n_envs", [1, 3, 65])
def test_torch_window_equals_the_deques_bit_for_bit(n_envs, window):
    win = metrics.EpisodeWindow(window, device="cpu")
    assert not win.fused and np.isnan(win.rows.numpy()).all()
    ref = metrics_ref.DequeWindow(window)
    script = metrics_ref.push_script(n_envs, window, seed=n_envs * 1000 + window, nan_payload=True)
    assert any(s["skip"] is not None for s in script)
    for t, s in enumerate(script):
        win.push(**_t(s))
        ref.push(**s)
        assert int(win.count) == ref.count, t
        assert np.array_equal(_bits(win.rows.numpy()), _bits(ref.rows())), t
    assert ref.count > window          # the ring wrapped


def test_window_counts_of_the_script():
    """The script holds every count of finishers the window's edges need."""
    assert metrics_ref.finisher_counts(65, 3) == [0, 1, 2, 3, 4, 65]
    assert metrics_ref.finisher_counts(3, 100) == [0, 1, 3]
    assert metrics_ref.finisher_counts(1, 1) == [0, 1]


@pytest.mark.parametrize("window", [1, 3, 100])
@pytest.mark.parametrize("n_envs", [1, 3, 65])
def test_torch_summary_is_within_the_bound_of_fsum(n_envs, window):
    win = metrics.EpisodeWindow(window, device="cpu")
    ref = metrics_ref.DequeWindow(window)
    metrics_ref.assert_summary(win.summary_tensor().numpy(), *ref.summary(), what="empty")
    assert win.summary()["n"] == 0
    for t, s in enumerate(metrics_ref.push_script(n_envs, window, seed=7 + n_envs + window)):
        win.push(**_t(s))
        ref.push(**s)
        metrics_ref.assert_summary(win.summary_tensor().numpy(), *ref.summary(), what=t)
    d = win.summary()
    want, _ = ref.summary()
    assert d["n"] == min(ref.count, window) and d["n_success"] == int(want[83])
    assert d["ep_return/max"] == want[1 + 3] and d["path_length/min"] == want[1 + 4 * 4 + 2]
    assert set(d) == {"n", "distance_per_cycle", "cycles_to_success", "n_success"} | {
        f"{k}/{s}" for k in metrics.ROW_KEYS for s in metrics.SUMMARY_STATS}


def test_summary_without_a_success_row_has_no_cycles_to_success():
    win = metrics.EpisodeWindow(4, device="cpu")
    rng = np.random.default_rng(0)
    s = metrics_ref.make_step(rng, 3, [0, 2])
    s["terminated"][:] = 0
    s["truncated"][[0, 2]] = 1
    win.push(**_t(s))
    d = win.summary()
    assert d["n"] == 2 and d["n_success"] == 0 and np.isnan(d["cycles_to_success"])
    assert d["truncation/mean"] == 1.0 and d["success/mean"] == 0.0


def test_row_keys_are_the_headers_columns():
    assert metrics.ROW_KEYS[:4] == ("ep_return", "ep_len", "success", "truncation")
    assert metrics.ROW_KEYS[4] == "path_length" and metrics.ROW_KEYS[-1] == "avg_rewards_obstacle"
    assert len(metrics.ROW_KEYS) == metrics_ref.COLS


def test_window_argument_checks():
    for w in (0, 1025):
        with pytest.raises(ValueError):
            metrics.EpisodeWindow(w, device="cpu")
    with pytest.raises(ValueError):
        metrics.EpisodeWindow(4, device="cpu", fused=True)      # HIP kernels need a GPU: no quiet fall-back
    with pytest.raises(ValueError):
        metrics.EvalAccount(5, 2, device="cpu", fused=True)


@pytest.mark.parametrize("n_eval,n_envs", metrics_ref.EVAL_CASES)
def test_torch_eval_account_equals_the_loop(n_eval, n_envs):
    acc = metrics.EvalAccount(n_eval, n_envs, device="cpu")
    ref = metrics_ref.EvalLoop(n_eval, n_envs)
    assert acc.target.tolist() == [(n_eval + i) // n_envs for i in range(n_envs)] == ref.target
    assert acc.offset.tolist() == ref.offset and sum(ref.target) == n_eval and acc.left() == n_eval
    hit_zero = None
    for t, s in enumerate(metrics_ref.eval_script(n_eval, n_envs, seed=n_eval * 10 + n_envs)):
        s = dict(s)
        s.pop("skip")
        acc.push(**_t(s))
        ref.push(**s)
        assert acc.left() == ref.remaining and acc.done_count.tolist() == ref.done, t
        assert (acc.left() == 0) == all(d == g for d, g in zip(ref.done, ref.target)), t
        if hit_zero is None and acc.left() == 0:
            hit_zero = t
        for k in ("ep_return", "ep_len", "success"):
            assert np.array_equal(getattr(acc, k).numpy(), getattr(ref, k), equal_nan=True), (t, k)
    # every target was met before the script ended, so the later episodes were ignored
    assert hit_zero is not None and hit_zero < t and acc.left() == 0
    assert not np.isnan(acc.ep_return.numpy()).any()
