"""BASELINE.json config 5: PPO on 32 768 envs per GPU with the HIP GAE scan.

    python tools/bench_ppo.py [--n-envs 32768] [--n-steps 32] [--iters 2] [--trend-iters 0]
    python -m torch.distributed.run --nproc-per-node N tools/bench_ppo.py ...

Prints one JSON line: full-iteration env-steps/s (collection + GAE + update,
max time over ranks), the split (HIP events on the stream: collection, GAE and
update each where the GPU ran them), the per-iteration history (losses, mean
return of the episodes that ended, envs reset by the divergence guard), and the
GAE kernel alone against the HBM roofline (12 B read + 8 B written per (step,
env)).  --trend-iters K first runs K untimed iterations and reports their
history (a learning trend), then the timed ones.

The reference's RecurrentPPO uses n_steps 2048, batch 64 with 4 envs
(src/train_robot_recurrent_ppo.py:91-93): 128 minibatches per epoch.  At
32 768 envs the buffer of n_steps 2048 (MLP policy: obs, actions, rewards,
starts, values, log-probs, advantages, returns = 19 floats per (step, env),
5.1 GB) fits in HBM easily; batch 64 would mean 1 048 576 minibatches per
epoch, so the batch is scaled with the env count (default 32 768).

    python tools/bench_ppo.py --recurrent --reference-config [--fused-step]
    python tools/bench_ppo.py --recurrent --ab-fused-step OUT.json [--reference-config | --n-envs ...]

--reference-config: the reference script's own settings (4 envs, n_steps 2048,
batch_size 64, seq_len 16).  --fused-step: RecurrentPPO(fused_step=True), the
policy step as salp_lstm_policy_step.  --ab-fused-step: two learners of the
same settings in this one process, fused_step off and on, one warm-up
iteration each and then --iters timed iterations each in turn (off, on, off,
on, ...); env-steps/s and the collect / GAE / update seconds of every
iteration (HIP events) are printed as one JSON line and written to OUT.json.
--collect-only K: K lock-step env-steps of one collection and nothing else
(for a kernel trace: the launches per env-step are the difference of two K).

    python tools/bench_ppo.py --ab-fused-act OUT.json [--iters 2]
    python tools/bench_ppo.py --collect-only K --n-envs 4 [--fused-act]

--ab-fused-act: lock-step PPO (collect="lockstep", n_steps 64) at 4, 1 024 and
32 768 envs, two learners per size in this one process, fused_act off and on
(the policy step as torch ops / as salp_ppo_mlp_act), one warm-up iteration
each and then --iters timed iterations each in turn (off, on, off, on); the
means of the collection's seconds per iteration (HIP events) and of env-steps/s
(wall), and the wall time of evaluate(SalpVecEnv(5), 5) off and on, are printed
as one JSON line and written to OUT.json.  --collect-only without --recurrent:
one lock-step PPO collection of K env-steps (--fused-act: with the kernel).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0


def gae_roofline(T, n, reps=20):
    from grasp_lab_salp_amd.ppo import compute_gae
    g = torch.Generator(device="cuda").manual_seed(0)
    rew = torch.randn(T, n, device="cuda", generator=g)
    val = torch.randn(T, n, device="cuda", generator=g)
    st = (torch.rand(T, n, device="cuda", generator=g) < 0.02).float()
    lv, dn = torch.randn(n, device="cuda", generator=g), torch.zeros(n, device="cuda")
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    compute_gae(rew, val, st, lv, dn, advantages=adv, returns=ret)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        compute_gae(rew, val, st, lv, dn, advantages=adv, returns=ret)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    byts = T * n * 20 + n * 8
    gbs = byts / (ms / 1e3) / 1e9
    return {"n_steps": T, "n_envs": n, "ms": ms, "bytes": byts,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": gbs / HBM_PEAK_GBS}}


def recurrent_ab(a):
    """--ab-fused-step / --collect-only (see the module docstring); one GPU."""
    from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO
    from grasp_lab_salp_amd.vec_env import SalpVecEnv

    def make(fused):
        env = SalpVecEnv(a.n_envs, seed=0, infos=False)
        return RecurrentPPO("MlpLstmPolicy", env, n_steps=a.n_steps, batch_size=a.batch_size, n_epochs=a.n_epochs,
                            seed=0, seq_len=a.seq_len, policy_kwargs={"lstm_hidden_size": a.lstm_hidden},
                            fused_step=fused)
    if a.collect_only:
        a.n_steps = a.collect_only - a.collect_only % a.seq_len
        a.batch_size = a.seq_len
        m = make(a.fused_step)
        m.collect_rollouts()
        torch.cuda.synchronize()
        print(json.dumps({"collect_only_steps": a.n_steps, "n_envs": a.n_envs, "fused_step": a.fused_step}), flush=True)
        return
    per_iter = a.n_steps * a.n_envs
    models = {"off": make(False), "on": make(True)}
    rows = []
    for r in range(a.iters + 1):       # round 0: warm-up (graph capture, allocator)
        for name, m in models.items():
            before = dict(m.timing)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.learn(m.num_timesteps + per_iter)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            row = {"fused_step": name, "round": r, "warmup": r == 0, "wall_s": el, "env_steps_per_s": per_iter / el,
                   **{k: m.timing[k] - before[k] for k in m.timing}}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    res = {"metric": "RecurrentPPO iteration, fused_step off / on in turn (one process)", "n_envs": a.n_envs,
           "n_steps": a.n_steps, "batch_size": a.batch_size, "n_epochs": a.n_epochs, "seq_len": a.seq_len,
           "lstm_hidden": a.lstm_hidden, "iterations": rows}
    for name in models:
        timed = [x for x in rows if x["fused_step"] == name and not x["warmup"]]
        res[name] = {k: sum(x[k] for x in timed) / len(timed) for k in ("env_steps_per_s", "collect_s", "gae_s",
                                                                         "train_s", "wall_s")}
    with open(a.ab_fused_step, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("metric", "n_envs", "n_steps", "off", "on")}), flush=True)


def ppo_act_ab(a):
    """--ab-fused-act / --collect-only without --recurrent (see the module docstring); one GPU."""
    from grasp_lab_salp_amd.ppo import PPO
    from grasp_lab_salp_amd.vec_env import SalpVecEnv

    def make(n_envs, n_steps, fused):
        env = SalpVecEnv(n_envs, seed=0, infos=False)
        return PPO("MlpPolicy", env, n_steps=n_steps, batch_size=min(n_envs * n_steps, 32768), n_epochs=2, seed=0,
                   collect="lockstep", fused_act=fused)
    if a.collect_only:
        m = make(a.n_envs, a.collect_only, a.fused_act)
        m.collect_rollouts()
        torch.cuda.synchronize()
        print(json.dumps({"collect_only_steps": a.collect_only, "n_envs": a.n_envs, "fused_act": a.fused_act}),
              flush=True)
        return
    n_steps = 64
    res = {"metric": "lock-step PPO iteration, fused_act off / on in turn (one process)", "n_steps": n_steps,
           "n_epochs": 2, "iters": a.iters, "sizes": {}}
    for n_envs in (4, 1024, 32768):
        per_iter = n_steps * n_envs
        models = {"off": make(n_envs, n_steps, False), "on": make(n_envs, n_steps, True)}
        rows = []
        for r in range(a.iters + 1):       # round 0: warm-up (graph capture, allocator)
            for name, m in models.items():
                before = dict(m.timing)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.learn(m.num_timesteps + per_iter)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                row = {"fused_act": name, "round": r, "warmup": r == 0, "wall_s": el, "env_steps_per_s": per_iter / el,
                       **{k: m.timing[k] - before[k] for k in m.timing}}
                rows.append(row)
                print(json.dumps({"n_envs": n_envs, **row}), file=sys.stderr, flush=True)
        size = {"iterations": rows}
        for name in models:
            timed = [x for x in rows if x["fused_act"] == name and not x["warmup"]]
            size[name] = {k: sum(x[k] for x in timed) / len(timed) for k in ("env_steps_per_s", "collect_s", "gae_s",
                                                                             "train_s", "wall_s")}
        if n_envs == 4:     # evaluate(SalpVecEnv(5), 5): a warm-up run, then the timed ones in turn
            ev = {name: [] for name in models}
            for r in range(a.iters + 1):
                for name, m in models.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.evaluate(SalpVecEnv(5, seed=1), 5)
                    if r:
                        ev[name].append(time.perf_counter() - t0)
            res["evaluate_wall_s"] = {name: sum(v) / len(v) for name, v in ev.items()}
            res["evaluate_steps"] = max(models["on"].last_eval["lengths"])
        res["sizes"][str(n_envs)] = size
        del models
        torch.cuda.empty_cache()
    with open(a.ab_fused_act, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"metric": res["metric"], "evaluate_wall_s": res["evaluate_wall_s"],
                      **{n: {k: v[k] for k in ("off", "on")} for n, v in res["sizes"].items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=32768)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=32768)
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--gae-steps", type=int, default=2048)
    ap.add_argument("--trend-iters", type=int, default=0)
    ap.add_argument("--lockstep-order", type=int, default=-1, help="salp_set_lockstep_order mode")
    ap.add_argument("--collect", default="auto", choices=("auto", "lockstep", "chained"),
                    help="collection: salp_step per env-step, or salp_collect (policy inside the kernel)")
    ap.add_argument("--no-graphs", action="store_true", help="eager minibatch steps (PPO(use_graphs=False))")
    ap.add_argument("--recurrent", action="store_true",
                    help="RecurrentPPO with the MlpLstmPolicy (LSTM 256) of src/train_robot_recurrent_ppo.py")
    ap.add_argument("--lstm-hidden", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--fused-step", action="store_true", help="RecurrentPPO(fused_step=True)")
    ap.add_argument("--reference-config", action="store_true",
                    help="src/train_robot_recurrent_ppo.py:85-107: 4 envs, n_steps 2048, batch_size 64, seq_len 16")
    ap.add_argument("--ab-fused-step", metavar="OUT.json", help="fused_step off / on in turn in one process")
    ap.add_argument("--collect-only", type=int, default=0, metavar="K", help="one collection of K env-steps, no update")
    ap.add_argument("--fused-act", action="store_true", help="PPO(fused_act=True) (with --collect-only)")
    ap.add_argument("--ab-fused-act", metavar="OUT.json", help="lock-step PPO, fused_act off / on in turn in one process")
    ap.add_argument("--episode-log", action="store_true",
                    help="PPO(episode_log=True) with DetailedMetricsCallback(log_freq=n_steps): the chained collection "
                         "records its episodes in the kernel; also times the merge kernel alone")
    a = ap.parse_args()
    if a.reference_config:
        a.n_envs, a.n_steps, a.batch_size, a.seq_len, a.recurrent = 4, 2048, 64, 16, True
    if a.ab_fused_act or (a.collect_only and not a.recurrent):
        return ppo_act_ab(a)
    if a.ab_fused_step or a.collect_only:
        return recurrent_ab(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from grasp_lab_salp_amd.ppo import PPO
    from grasp_lab_salp_amd.shard import env_id_offset, reduce_run
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    env = SalpVecEnv(a.n_envs, seed=0, env_id_offset=env_id_offset(rank, a.n_envs), infos=False)
    env.sim.set_lockstep_order(a.lockstep_order)
    if a.recurrent:
        from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO
        model = RecurrentPPO("MlpLstmPolicy", env, n_steps=a.n_steps, batch_size=a.batch_size, n_epochs=a.n_epochs,
                             seed=0, seq_len=a.seq_len, policy_kwargs={"lstm_hidden_size": a.lstm_hidden},
                             fused_step=a.fused_step)
    else:
        model = PPO("MlpPolicy", env, n_steps=a.n_steps, batch_size=a.batch_size, n_epochs=a.n_epochs, seed=0,
                    collect=a.collect, use_graphs=False if a.no_graphs else None, episode_log=a.episode_log)
    callback = None
    if a.episode_log:
        from grasp_lab_salp_amd.callbacks import DetailedMetricsCallback
        callback = DetailedMetricsCallback(log_freq=a.n_steps)
    # warm-up (+ trend) iterations, one learn() call each so that a long trend
    # reports progress on stderr (a GPU job silent for minutes looks hung)
    for it in range(max(1, a.trend_iters)):
        model.learn((it + 1) * a.n_steps * a.n_envs, callback=callback)
        if rank == 0:
            print(json.dumps(model.history[-1]), file=sys.stderr, flush=True)
    trend = list(model.history)
    for k in model.timing:
        model.timing[k] = 0.0
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    model.num_timesteps = 0
    h0 = len(model.history)
    model.learn(a.iters * a.n_steps * a.n_envs, callback=callback)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    merge = None
    if a.episode_log:   # the merge kernel alone, on the last collection's log (into a scratch window)
        from grasp_lab_salp_amd.metrics import EpisodeWindow
        log, win = model._episode_log, EpisodeWindow(callback.window_size, model.device)
        win.push_log(log)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            win.push_log(log)
        e1.record()
        torch.cuda.synchronize()
        merge = {"ms": e0.elapsed_time(e1) / 20, "per_env": log.per_env, "episodes_in_log": int(log.count.sum()),
                 "window_count": int(callback.window.count), "lost": int(callback.window.lost),
                 "log_bytes": sum(t.numel() * t.element_size() for t in (log.rows, log.step, log.count))}
    el, steps, _, _ = reduce_run(el, model.num_timesteps, 0.0, 0.0, device=torch.device("cuda", local))
    if rank == 0:
        res = {"metric": "PPO env-steps/sec (collect + GAE + update), config 5", "value": steps / el,
               "unit": "env-steps/s", "n_gpus": world, "n_envs_per_gpu": a.n_envs, "n_steps": a.n_steps,
               "batch_size": a.batch_size, "n_epochs": a.n_epochs, "iters": a.iters, "collect": model.collect,
               "policy": (f"MlpLstmPolicy (LSTM {a.lstm_hidden}, seq_len {a.seq_len})" if a.recurrent
                          else "MlpPolicy 64-64 tanh"),
               "timing_s": model.timing, "episode_log": model.episode_log, "merge_kernel": merge,
               "losses": model.logger,
               "history": model.history[h0:], "trend": trend if a.trend_iters else None,
               "diverged_envs_reset": model.nonfinite_resets,
               "gae_kernel": gae_roofline(a.gae_steps, a.n_envs)}
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
