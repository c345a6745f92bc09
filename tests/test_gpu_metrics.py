"""csrc/salp_metrics.hip on the GPU against tests/metrics_ref.py: the push
kernel's rows and counter bit for bit with the deque restatement (between
canaries, twice over), the summary kernel within the bound derived in
tests/test_metrics_host.py of the fsum reference, and the evaluation
bookkeeping against SB3's loop.  The inputs are synthetic info arrays: no
simulator runs here."""
import numpy as np
import pytest
import torch

import metrics_ref
from grasp_lab_salp_amd import _lib, metrics

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, PAD = 1234.5, 0x5A5A5A5A5A5A5A5A, 64


def _dev(step):
    return {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in step.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _guarded_window(window):
    """An EpisodeWindow whose rows and counter sit between canaries."""
    win = metrics.EpisodeWindow(window, device="cuda")
    assert win.fused
    fbuf = torch.full((2 * PAD + window * _lib.EPWIN_COLS,), CANARY_F, dtype=torch.float64, device="cuda")
    ibuf = torch.full((2 * PAD + 1,), CANARY_I, dtype=torch.int64, device="cuda")
    win.rows = fbuf[PAD:PAD + window * _lib.EPWIN_COLS].view(window, _lib.EPWIN_COLS)
    win.rows.fill_(float("nan"))
    win.count = ibuf[PAD:PAD + 1]
    win.count.zero_()
    win._c = _lib.SalpEpisodeWindow(window, 0, win.rows.data_ptr(), win.count.data_ptr())

    def intact():
        f, i = fbuf.cpu().numpy(), ibuf.cpu().numpy()
        return ((f[:PAD] == CANARY_F).all() and (f[-PAD:] == CANARY_F).all() and (i[:PAD] == CANARY_I).all()
                and (i[-PAD:] == CANARY_I).all())
    return win, intact


@pytest.mark.parametrize("window", [1, 3, 100, 1024])
@pytest.mark.parametrize("n_envs", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 65537])
def test_push_kernel_equals_the_deques_bit_for_bit(n_envs, window):
    script = metrics_ref.push_script(n_envs, window, seed=n_envs * 7 + window, nan_payload=True, lanes=True)
    assert any(s["skip"] is not None for s in script) and any(s["skip"] is None for s in script)
    dev = [_dev(s) for s in script]
    win, intact = _guarded_window(window)
    ref = metrics_ref.DequeWindow(window)
    every = max(len(script) // 24, 1)        # a long script (few envs, a long window) is compared now and then
    for t, (s, d) in enumerate(zip(script, dev)):
        win.push(**d)
        ref.push(**s)
        if t % every == 0 or t == len(script) - 1:
            assert int(win.count) == ref.count, t
            assert np.array_equal(_bits(win.rows.cpu().numpy()), _bits(ref.rows())), t
    assert ref.count > window and intact()
    # the same sequence again: the same bits
    again, intact2 = _guarded_window(window)
    for d in dev:
        again.push(**d)
    assert int(again.count) == ref.count and intact2()
    assert np.array_equal(_bits(again.rows.cpu().numpy()), _bits(win.rows.cpu().numpy()))


@pytest.mark.parametrize("window", [1, 3, 100, 1024])
@pytest.mark.parametrize("n_envs", [1, 65, 1025])
def test_summary_kernel_is_within_the_bound_of_fsum(n_envs, window):
    win = metrics.EpisodeWindow(window, device="cuda")
    ref = metrics_ref.DequeWindow(window)
    metrics_ref.assert_summary(win.summary_tensor().cpu().numpy(), *ref.summary(), what="empty")
    script = metrics_ref.push_script(n_envs, window, seed=n_envs + 31 * window)
    every = max(len(script) // 12, 1)
    for t, s in enumerate(script):
        win.push(**_dev(s))
        ref.push(**s)
        if t % every == 0 or t == len(script) - 1:
            got = win.summary_tensor().cpu().numpy()
            metrics_ref.assert_summary(got, *ref.summary(), what=t)
            assert np.array_equal(_bits(win.summary_tensor().cpu().numpy()), _bits(got)), t     # the same bits again
    assert win.summary()["n"] == window


def test_summary_kernel_without_a_success_row():
    win = metrics.EpisodeWindow(8, device="cuda")
    s = metrics_ref.make_step(np.random.default_rng(1), 5, [1, 3, 4])
    s["terminated"][:] = 0
    s["truncated"][[1, 3, 4]] = 1
    win.push(**_dev(s))
    d = win.summary()
    assert d["n"] == 3 and d["n_success"] == 0 and np.isnan(d["cycles_to_success"]) and d["truncation/mean"] == 1.0


@pytest.mark.parametrize("n_eval,n_envs", metrics_ref.EVAL_CASES + [(700, 300)])
def test_eval_account_kernel_equals_the_loop(n_eval, n_envs):
    acc = metrics.EvalAccount(n_eval, n_envs, device="cuda")
    assert acc.fused
    ref = metrics_ref.EvalLoop(n_eval, n_envs)
    for t, s in enumerate(metrics_ref.eval_script(n_eval, n_envs, seed=n_eval + n_envs)):
        s = dict(s)
        s.pop("skip")
        acc.push(**_dev(s))
        ref.push(**s)
        assert acc.left() == ref.remaining and acc.done_count.tolist() == ref.done, t
        for k in ("ep_return", "ep_len", "success"):
            assert np.array_equal(getattr(acc, k).cpu().numpy(), getattr(ref, k), equal_nan=True), (t, k)
    assert acc.left() == 0 and max(ref.done) == max(ref.target)


def test_wrappers_check_their_tensors():
    win = metrics.EpisodeWindow(4, device="cuda")
    s = _dev(metrics_ref.make_step(np.random.default_rng(0), 3, [0]))
    with pytest.raises(ValueError, match="terminated"):
        win.push(s["info"], s["terminated"].bool(), s["truncated"])
    with pytest.raises(ValueError, match="info"):
        win.push(s["info"].float(), s["terminated"], s["truncated"])
    with pytest.raises(ValueError, match="skip"):
        win.push(s["info"], s["terminated"], s["truncated"], skip=s["terminated"][:2])
    assert int(win.count) == 0
