"""The learner entry points' argument checks (include/salp.h: salp_ppo_*,
salp_lstm_*, salp_gae, salp_replay_*, salp_sac_*, salp_episode_window_*,
salp_eval_account): every rejected call's return value and the full text it
leaves behind salp_last_error(NULL), and the accepted empty sizes.  Each
function is defined in the unit that owns its kernels, while the last-error
string lives in salp_kernels.hip: a row passes only if the two still meet.
Every call returns before a launch.  No GPU needed."""
import ctypes
import threading

import pytest

from grasp_lab_salp_amd import _lib

P = 4096            # a non-NULL pointer; never dereferenced, the checks come first
NAN = float("nan")
# what salp_math_selftest (salp_kernels.hip) leaves when it is called before a row
SENTINEL = "salp_math_selftest: bad argument"


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    build.build()
    return _lib.load()


def _struct(cls, **kw):
    """cls with every pointer (and pointer array element) non-NULL, then the overrides; (i, v) sets element i."""
    s = cls()
    for name, ct in cls._fields_:
        if ct is ctypes.c_void_p:
            setattr(s, name, P)
        elif issubclass(ct, ctypes.Array):
            for i in range(ct._length_):
                getattr(s, name)[i] = P
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(s, k)[v[0]] = v[1]
        else:
            setattr(s, k, v)
    return ctypes.byref(s)


def _mb(**kw):
    return _struct(_lib.SalpPpoMinibatch, **{**dict(batch=64, obs_dim=14, clip_range=0.2), **kw})


def _adam(**kw):
    return _struct(_lib.SalpPpoAdam, **{**dict(obs_dim=14), **kw})


def _rb(**kw):
    return _struct(_lib.SalpReplay, **{**dict(capacity=8, n_envs=4, obs_dim=10), **kw})


def _add(**kw):
    return _struct(_lib.SalpReplayAdd, **kw)


def _sample(**kw):
    return _struct(_lib.SalpReplaySample, **{**dict(batch=64), **kw})


def _td(**kw):
    return _struct(_lib.SalpSacTd, **{**dict(batch=64), **kw})


def _pi(**kw):
    return _struct(_lib.SalpSacPi, **{**dict(batch=64), **kw})


def _fwd(**kw):
    return _struct(_lib.SalpSacNetForward, **{**dict(batch=64, d0=10, d1=3, out_dim=1, n_nets=2), **kw})


def _bwd(**kw):
    return _struct(_lib.SalpSacNetBackward, **{**dict(batch=64, d0=10, d1=3, out_dim=1, n_nets=2), **kw})


def _bwd_nothing_asked():
    b = _lib.SalpSacNetBackward(batch=64, d0=10, d1=3, out_dim=1, n_nets=2, workspace=P)
    for name in ("params", "x0", "x1", "h1", "h2", "dout"):
        for i in range(4):
            getattr(b, name)[i] = P
    return ctypes.byref(b)


def _win(**kw):
    return _struct(_lib.SalpEpisodeWindow, **{**dict(window=100), **kw})


def _push(**kw):
    return _struct(_lib.SalpEpisodePush, **{**dict(n_envs=8), **kw})


def _eval(**kw):
    return _struct(_lib.SalpEvalState, **{**dict(n_envs=8), **kw})


def _ppo_loss(batch=64, mu=P, clip=0.2):
    return (batch, mu, P, P, P, P, P, P, clip, 0.0, 0.5, 1, P, P, P, P, None)


EPWIN = "window must be in 1 .. 1024, rows and count set"
NET_DIMS = "d0 >= 1, d1 >= 0, d0 + d1 <= 17 and out_dim in 1 .. 6"

# (function, arguments, return value, salp_last_error(NULL) afterwards); a function
# that reports by its return value alone leaves the text as it was: SENTINEL
REJECTED = [
    ("salp_ppo_loss", _ppo_loss(batch=0), -1, "salp_ppo_loss: batch must be positive"),
    ("salp_ppo_loss", _ppo_loss(batch=-5), -1, "salp_ppo_loss: batch must be positive"),
    ("salp_ppo_loss", _ppo_loss(mu=None), -1, "salp_ppo_loss: null buffer"),
    ("salp_ppo_loss", _ppo_loss(clip=-0.1), -1, "salp_ppo_loss: clip_range must be >= 0"),
    ("salp_ppo_loss", _ppo_loss(clip=NAN), -1, "salp_ppo_loss: clip_range must be >= 0"),

    ("salp_ppo_mlp_num_params", (0,), -1, SENTINEL),
    ("salp_ppo_mlp_num_params", (15,), -1, SENTINEL),
    ("salp_ppo_mlp_offset", (15, 0), -1, SENTINEL),
    ("salp_ppo_mlp_offset", (14, -1), -1, SENTINEL),
    ("salp_ppo_mlp_offset", (14, 14), -1, SENTINEL),
    ("salp_ppo_mlp_workspace_doubles", (0, 14), -1, SENTINEL),
    ("salp_ppo_mlp_workspace_doubles", (64, 15), -1, SENTINEL),
    ("salp_ppo_mlp_grads", (None, None), -1, "salp_ppo_mlp_grads: batch must be positive"),
    ("salp_ppo_mlp_grads", (_mb(batch=0), None), -1, "salp_ppo_mlp_grads: batch must be positive"),
    ("salp_ppo_mlp_grads", (_mb(obs_dim=15), None), -1, "salp_ppo_mlp_grads: obs_dim out of range"),
    ("salp_ppo_mlp_grads", (_mb(obs_dim=0), None), -1, "salp_ppo_mlp_grads: obs_dim out of range"),
    ("salp_ppo_mlp_grads", (_mb(idx=None), None), -1, "salp_ppo_mlp_grads: null buffer"),
    ("salp_ppo_mlp_grads", (_mb(workspace=None), None), -1, "salp_ppo_mlp_grads: null buffer"),
    ("salp_ppo_mlp_grads", (_mb(params=(12, None)), None), -1, "salp_ppo_mlp_grads: null parameter tensor"),
    ("salp_ppo_mlp_grads", (_mb(clip_range=-1.0), None), -1, "salp_ppo_mlp_grads: clip_range must be >= 0"),
    ("salp_ppo_mlp_adv_partials", (0, 4, P, P, P, None), -1,
     "salp_ppo_mlp_adv_partials: batch > 0 and 0 < n_minibatches <= 65535"),
    ("salp_ppo_mlp_adv_partials", (64, 0, P, P, P, None), -1,
     "salp_ppo_mlp_adv_partials: batch > 0 and 0 < n_minibatches <= 65535"),
    ("salp_ppo_mlp_adv_partials", (64, 65536, P, P, P, None), -1,
     "salp_ppo_mlp_adv_partials: batch > 0 and 0 < n_minibatches <= 65535"),
    ("salp_ppo_mlp_adv_partials", (64, 4, None, P, P, None), -1, "salp_ppo_mlp_adv_partials: null buffer"),
    ("salp_ppo_mlp_apply", (None, None), -1, "salp_ppo_mlp_apply: obs_dim out of range"),
    ("salp_ppo_mlp_apply", (_adam(obs_dim=15), None), -1, "salp_ppo_mlp_apply: obs_dim out of range"),
    ("salp_ppo_mlp_apply", (_adam(step=None), None), -1, "salp_ppo_mlp_apply: null buffer"),
    ("salp_ppo_mlp_apply", (_adam(params=(0, None)), None), -1, "salp_ppo_mlp_apply: null parameter tensor"),

    ("salp_lstm_cell_forward", (-1, 64, P, P, P, P, P, P, None), -1, "salp_lstm_cell_forward: bad size"),
    ("salp_lstm_cell_forward", (8, 0, P, P, P, P, P, P, None), -1, "salp_lstm_cell_forward: bad size"),
    ("salp_lstm_cell_forward", (8, 64, None, P, P, P, P, P, None), -1, "salp_lstm_cell_forward: null buffer"),
    ("salp_lstm_cell_forward", (0, 64, P, P, P, P, P, None, None), -1, "salp_lstm_cell_forward: null buffer"),
    ("salp_lstm_step_forward", (-1, 64, P, P, P, P, P, P, P, P, P, None), -1, "salp_lstm_step_forward: bad size"),
    ("salp_lstm_step_forward", (8, 64, P, None, P, None, None, P, P, P, None, None), -1,
     "salp_lstm_step_forward: null buffer"),
    ("salp_lstm_step_forward", (8, 64, P, P, P, P, P, P, P, P, None, None), -1,
     "salp_lstm_step_forward: keep_next and hk_next go together"),
    ("salp_lstm_step_forward", (8, 64, P, P, P, P, None, P, P, P, P, None), -1,
     "salp_lstm_step_forward: keep_next and hk_next go together"),
    ("salp_lstm_cell_backward", (8, -64, P, P, P, P, P, P, P, P, None), -1, "salp_lstm_cell_backward: bad size"),
    ("salp_lstm_cell_backward", (8, 64, P, P, P, P, None, None, P, P, None), -1,
     "salp_lstm_cell_backward: null buffer"),
    ("salp_lstm_step_backward", (-1, 64, P, P, P, P, P, P, P, P, P, P, None), -1, "salp_lstm_step_backward: bad size"),
    ("salp_lstm_step_backward", (8, 64, P, P, P, P, P, None, None, None, P, None, None), -1,
     "salp_lstm_step_backward: null buffer"),
    ("salp_lstm_step_backward", (8, 64, P, P, P, P, P, P, None, P, P, P, None), -1,
     "salp_lstm_step_backward: dhk_next and keep_next go together"),
    ("salp_lstm_step_backward", (8, 64, P, P, P, P, P, None, P, P, P, P, None), -1,
     "salp_lstm_step_backward: dhk_next and keep_next go together"),

    ("salp_gae", (-1, 8, P, P, P, P, P, 0.99, 0.95, P, P, None), -1, "salp_gae: negative size"),
    ("salp_gae", (8, -1, P, P, P, P, P, 0.99, 0.95, P, P, None), -1, "salp_gae: negative size"),
    ("salp_gae", (8, 8, P, P, P, P, None, 0.99, 0.95, P, P, None), -1, "salp_gae: null buffer"),
    ("salp_gae", (0, 8, P, P, P, P, P, 0.99, 0.95, P, None, None), -1, "salp_gae: null buffer"),

    ("salp_replay_add", (None, _add(), None), -1, "salp_replay_add: bad replay buffer"),
    ("salp_replay_add", (_rb(obs_dim=15), _add(), None), -1, "salp_replay_add: bad replay buffer"),
    ("salp_replay_add", (_rb(n_envs=1 << 31), _add(), None), -1, "salp_replay_add: bad replay buffer"),
    ("salp_replay_add", (_rb(size=None), _add(), None), -1, "salp_replay_add: bad replay buffer"),
    ("salp_replay_add", (_rb(), None, None), -1, "salp_replay_add: null buffer"),
    ("salp_replay_add", (_rb(), _add(truncated=None), None), -1, "salp_replay_add: null buffer"),
    ("salp_replay_sample", (_rb(capacity=0), _sample(), None), -1, "salp_replay_sample: bad replay buffer"),
    ("salp_replay_sample", (_rb(), None, None), -1, "salp_replay_sample: batch must be in 1 .. 2^32"),
    ("salp_replay_sample", (_rb(), _sample(batch=0), None), -1, "salp_replay_sample: batch must be in 1 .. 2^32"),
    ("salp_replay_sample", (_rb(), _sample(batch=(1 << 32) + 1), None), -1,
     "salp_replay_sample: batch must be in 1 .. 2^32"),
    ("salp_replay_sample", (_rb(), _sample(update=None), None), -1, "salp_replay_sample: null buffer"),
    ("salp_sac_actor_head_forward", (0, P, P, P, P, P, None), -1,
     "salp_sac_actor_head_forward: batch must be positive"),
    ("salp_sac_actor_head_forward", (64, P, P, None, P, P, None), -1, "salp_sac_actor_head_forward: null buffer"),
    ("salp_sac_actor_head_backward", (0, P, P, P, P, P, P, P, None), -1,
     "salp_sac_actor_head_backward: batch must be positive"),
    ("salp_sac_actor_head_backward", (64, P, P, P, None, None, P, None, None), -1,
     "salp_sac_actor_head_backward: null buffer"),
    ("salp_sac_td_head", (None, None), -1, "salp_sac_td_head: batch must be positive"),
    ("salp_sac_td_head", (_td(batch=0), None), -1, "salp_sac_td_head: batch must be positive"),
    ("salp_sac_td_head", (_td(alpha_used=None), None), -1, "salp_sac_td_head: null buffer"),
    ("salp_sac_pi_head", (None, None), -1, "salp_sac_pi_head: batch must be positive"),
    ("salp_sac_pi_head", (_pi(batch=-1), None), -1, "salp_sac_pi_head: batch must be positive"),
    ("salp_sac_pi_head", (_pi(dq2=None), None), -1, "salp_sac_pi_head: null buffer"),
    ("salp_sac_polyak", (0, P, P, 0.005, None), -1, "salp_sac_polyak: bad argument"),
    ("salp_sac_polyak", (64, P, None, 0.005, None), -1, "salp_sac_polyak: bad argument"),
    ("salp_sac_polyak", (64, P, P, 1.5, None), -1, "salp_sac_polyak: tau must be in [0, 1]"),
    ("salp_sac_polyak", (64, P, P, -0.1, None), -1, "salp_sac_polyak: tau must be in [0, 1]"),
    ("salp_sac_polyak", (64, P, P, NAN, None), -1, "salp_sac_polyak: tau must be in [0, 1]"),

    ("salp_sac_net_num_params", (18, 1), -1,
     "salp_sac_net_offset: in_dim in 1 .. 17, out_dim in 1 .. 6, tensor in 0 .. 6"),
    ("salp_sac_net_num_params", (9, 7), -1,
     "salp_sac_net_offset: in_dim in 1 .. 17, out_dim in 1 .. 6, tensor in 0 .. 6"),
    ("salp_sac_net_offset", (0, 1, 0), -1,
     "salp_sac_net_offset: in_dim in 1 .. 17, out_dim in 1 .. 6, tensor in 0 .. 6"),
    ("salp_sac_net_offset", (9, 1, 7), -1,
     "salp_sac_net_offset: in_dim in 1 .. 17, out_dim in 1 .. 6, tensor in 0 .. 6"),
    ("salp_sac_net_workspace_floats", (0, 10, 3, 1, 2), -1, "salp_sac_net_workspace_floats: bad argument"),
    ("salp_sac_net_workspace_floats", (1 << 31, 10, 3, 1, 2), -1, "salp_sac_net_workspace_floats: bad argument"),
    ("salp_sac_net_workspace_floats", (64, 15, 3, 1, 2), -1, "salp_sac_net_workspace_floats: bad argument"),
    ("salp_sac_net_workspace_floats", (64, 10, 3, 1, 5), -1, "salp_sac_net_workspace_floats: bad argument"),
    ("salp_sac_net_forward", (None, None), -1, "salp_sac_net_forward: null argument"),
    ("salp_sac_net_forward", (_fwd(batch=0), None), -1, "salp_sac_net_forward: batch must be in 1 .. 2^31 - 1"),
    ("salp_sac_net_forward", (_fwd(batch=1 << 31), None), -1,
     "salp_sac_net_forward: batch must be in 1 .. 2^31 - 1"),
    ("salp_sac_net_forward", (_fwd(d0=15), None), -1, "salp_sac_net_forward: " + NET_DIMS),
    ("salp_sac_net_forward", (_fwd(d1=-1), None), -1, "salp_sac_net_forward: " + NET_DIMS),
    ("salp_sac_net_forward", (_fwd(out_dim=7), None), -1, "salp_sac_net_forward: " + NET_DIMS),
    ("salp_sac_net_forward", (_fwd(n_nets=5), None), -1, "salp_sac_net_forward: n_nets must be in 1 .. 4"),
    ("salp_sac_net_forward", (_fwd(params=(1, None)), None), -1, "salp_sac_net_forward: null params, x0 or x1"),
    ("salp_sac_net_forward", (_fwd(x1=(0, None)), None), -1, "salp_sac_net_forward: null params, x0 or x1"),
    ("salp_sac_net_forward", (_fwd(out=(1, None)), None), -1, "salp_sac_net_forward: null out"),
    ("salp_sac_net_forward", (_fwd(h1=(0, None)), None), -1,
     "salp_sac_net_forward: h1 and h2 are both NULL or both set"),
    ("salp_sac_net_backward", (None, None), -1, "salp_sac_net_backward: null argument"),
    ("salp_sac_net_backward", (_bwd(batch=0), None), -1, "salp_sac_net_backward: batch must be in 1 .. 2^31 - 1"),
    ("salp_sac_net_backward", (_bwd(d0=0), None), -1, "salp_sac_net_backward: " + NET_DIMS),
    ("salp_sac_net_backward", (_bwd(n_nets=0), None), -1, "salp_sac_net_backward: n_nets must be in 1 .. 4"),
    ("salp_sac_net_backward", (_bwd(x0=(1, None)), None), -1, "salp_sac_net_backward: null params, x0 or x1"),
    ("salp_sac_net_backward", (_bwd(dout=(1, None)), None), -1, "salp_sac_net_backward: null h1, h2 or dout"),
    ("salp_sac_net_backward", (_bwd(dparams=(1, None)), None), -1,
     "salp_sac_net_backward: dparams are all NULL or all set"),
    ("salp_sac_net_backward", (_bwd_nothing_asked(), None), -1,
     "salp_sac_net_backward: neither dparams nor dx1 is set"),
    ("salp_sac_net_backward", (_bwd(d0=13, d1=0), None), -1, "salp_sac_net_backward: dx1 needs d1 > 0"),
    ("salp_sac_net_backward", (_bwd(workspace=None), None), -1, "salp_sac_net_backward: null workspace"),

    ("salp_episode_window_push", (None, _push(), None), -1, "salp_episode_window_push: " + EPWIN),
    ("salp_episode_window_push", (_win(window=1025), _push(), None), -1, "salp_episode_window_push: " + EPWIN),
    ("salp_episode_window_push", (_win(window=0), _push(), None), -1, "salp_episode_window_push: " + EPWIN),
    ("salp_episode_window_push", (_win(count=None), _push(), None), -1, "salp_episode_window_push: " + EPWIN),
    ("salp_episode_window_push", (_win(), None, None), -1,
     "salp_episode_window_push: n_envs >= 1 and info, terminated, truncated set"),
    ("salp_episode_window_push", (_win(), _push(n_envs=0), None), -1,
     "salp_episode_window_push: n_envs >= 1 and info, terminated, truncated set"),
    ("salp_episode_window_push", (_win(), _push(info=None), None), -1,
     "salp_episode_window_push: n_envs >= 1 and info, terminated, truncated set"),
    ("salp_episode_window_summary", (_win(window=1025), P, None), -1, "salp_episode_window_summary: " + EPWIN),
    ("salp_episode_window_summary", (_win(rows=None), P, None), -1, "salp_episode_window_summary: " + EPWIN),
    ("salp_episode_window_summary", (_win(), None, None), -1, "salp_episode_window_summary: null out"),
    ("salp_eval_account", (None, _push(), None), -1, "salp_eval_account: n_envs must be positive"),
    ("salp_eval_account", (_eval(n_envs=0), _push(n_envs=0), None), -1, "salp_eval_account: n_envs must be positive"),
    ("salp_eval_account", (_eval(n_envs=1 << 39), _push(n_envs=1 << 39), None), -1,
     "salp_eval_account: n_envs must be positive"),
    ("salp_eval_account", (_eval(remaining=None), _push(), None), -1, "salp_eval_account: null state buffer"),
    ("salp_eval_account", (_eval(), None, None), -1,
     "salp_eval_account: the step must be of the state's n_envs, buffers set"),
    ("salp_eval_account", (_eval(n_envs=8), _push(n_envs=9), None), -1,
     "salp_eval_account: the step must be of the state's n_envs, buffers set"),
    ("salp_eval_account", (_eval(), _push(truncated=None), None), -1,
     "salp_eval_account: the step must be of the state's n_envs, buffers set"),
]

# sizes at which there is nothing to do: SALP_OK before any launch, optional buffers NULL
ACCEPTED = [
    ("salp_gae", (0, 8, P, P, P, P, P, 0.99, 0.95, P, P, None)),
    ("salp_gae", (8, 0, P, P, P, P, P, 0.99, 0.95, P, P, None)),
    ("salp_lstm_cell_forward", (0, 64, P, P, P, P, P, P, None)),
    ("salp_lstm_step_forward", (0, 64, P, None, P, P, None, P, P, P, None, None)),
    ("salp_lstm_step_forward", (0, 64, P, P, P, P, P, P, P, P, P, None)),
    ("salp_lstm_cell_backward", (0, 64, P, P, P, P, P, None, P, P, None)),
    ("salp_lstm_step_backward", (0, 64, P, P, P, P, P, None, None, None, P, P, None)),
    ("salp_lstm_step_backward", (0, 64, P, P, P, P, P, P, P, P, P, P, None)),
]

MOVED = ["salp_ppo_loss", "salp_ppo_mlp_num_params", "salp_ppo_mlp_offset", "salp_ppo_mlp_workspace_doubles",
         "salp_ppo_mlp_grads", "salp_ppo_mlp_adv_partials", "salp_ppo_mlp_apply", "salp_lstm_cell_forward",
         "salp_lstm_step_forward", "salp_lstm_cell_backward", "salp_lstm_step_backward", "salp_gae",
         "salp_replay_add", "salp_replay_sample", "salp_sac_actor_head_forward", "salp_sac_actor_head_backward",
         "salp_sac_td_head", "salp_sac_pi_head", "salp_sac_polyak", "salp_sac_net_num_params", "salp_sac_net_offset",
         "salp_sac_net_tile_rows", "salp_sac_net_max_blocks", "salp_sac_net_workspace_floats", "salp_sac_net_forward",
         "salp_sac_net_backward", "salp_episode_window_push", "salp_episode_window_summary", "salp_eval_account"]


def _last(lib):
    return lib.salp_last_error(None).decode()


def _set_sentinel(lib):
    assert lib.salp_math_selftest(None, None, 0, None, None) == -1
    assert _last(lib) == SENTINEL


def test_table_covers_every_learner_entry_point():
    # the two geometry queries take no argument and cannot be refused
    assert {r[0] for r in REJECTED} == set(MOVED) - {"salp_sac_net_tile_rows", "salp_sac_net_max_blocks"}
    assert len(MOVED) == 29 and all(f in _lib.SIGNATURES for f in MOVED)


@pytest.mark.parametrize("row", range(len(REJECTED)), ids=lambda i: f"{i}-{REJECTED[i][0]}")
def test_rejected_call(lib, row):
    name, args, rc, text = REJECTED[row]
    _set_sentinel(lib)
    assert getattr(lib, name)(*args) == rc
    assert _last(lib) == text


@pytest.mark.parametrize("row", range(len(ACCEPTED)), ids=lambda i: f"{i}-{ACCEPTED[i][0]}")
def test_empty_sizes_are_accepted_without_a_launch(lib, row):
    name, args = ACCEPTED[row]
    _set_sentinel(lib)
    assert getattr(lib, name)(*args) == 0
    assert _last(lib) == SENTINEL          # success leaves the text alone


def test_geometry_queries(lib):
    tr, mb = lib.salp_sac_net_tile_rows(), lib.salp_sac_net_max_blocks()
    assert tr > 0 and 0 < mb <= 64
    assert lib.salp_sac_net_workspace_floats(tr * mb + 1, 10, 0, 1, 1) == mb * lib.salp_sac_net_num_params(10, 1)


def test_last_error_is_per_thread(lib):
    """A learner unit's failure on another thread is read there and does not change this thread's text."""
    _set_sentinel(lib)
    seen = []

    def other():
        seen.append(_last(lib))
        seen.append(lib.salp_sac_polyak(64, P, P, 1.5, None))
        seen.append(_last(lib))

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == ["", -1, "salp_sac_polyak: tau must be in [0, 1]"]
    assert _last(lib) == SENTINEL
