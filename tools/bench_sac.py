"""The on-device SAC learner (grasp_lab_salp_amd/sac.py), fused and plain.

    python tools/bench_sac.py [--iters 300] [--warmup 30] [--configs ref,wide] [--out FILE]
    python tools/bench_sac.py --callbacks [--iters 300] [--warmup 30] [--out FILE]

Prints one JSON line (and writes it to FILE).  Per configuration, for ``fused``
on and off and for ``fused=True, fused_mlp=True`` (the networks as HIP kernels
too, csrc/salp_sac_mlp.hip): full iteration env-steps/s (collection + sample + update, host clock around a
device synchronise) and the milliseconds per iteration of each phase (HIP
events: the collection, and the first gradient step's sample and update).

  ref   8 envs with the settings of src/train_robot.py:62-69 (buffer 100 000,
        batch 256, train_freq 1, gradient_steps 1)
  wide  4 096 envs, batch_size 4 096, gradient_steps 1

learning_starts is one env-step, so every timed iteration trains; the warm-up
iterations (untimed) fill the buffer and load the GEMMs' kernels.  The
fused / plain and fused_mlp / fused ratios are reported, not judged.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONFIGS = {"ref": dict(n_envs=8, batch_size=256, buffer_size=100000),
           "wide": dict(n_envs=4096, batch_size=4096, buffer_size=1 << 20)}


def run(name, fused, iters, warmup, fused_mlp=False, callbacks=False):
    """``callbacks``: learn with DetailedMetricsCallback(log_freq=1000), as src/train_robot.py:75 builds it."""
    from grasp_lab_salp_amd.callbacks import DetailedMetricsCallback
    from grasp_lab_salp_amd.sac import SAC
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    c = CONFIGS[name]
    n = c["n_envs"]
    env = SalpVecEnv(n, seed=0, infos=False)
    model = SAC("MlpPolicy", env, learning_rate=3e-4, buffer_size=c["buffer_size"], learning_starts=n,
                batch_size=c["batch_size"], tau=0.005, gamma=0.99, train_freq=1, gradient_steps=1, seed=0,
                fused=fused, fused_mlp=fused_mlp)
    cb = DetailedMetricsCallback(log_freq=1000) if callbacks else None
    model.learn((warmup + 1) * n, log_interval=warmup + 1, callback=cb)
    for k in model.timing:
        model.timing[k] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.learn(iters * n, log_interval=iters, callback=cb)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"fused": fused, "fused_mlp": fused_mlp, "callbacks": bool(callbacks), "env_steps_per_s": iters * n / el,
           "iteration_ms": el / iters * 1e3,
           "phase_ms": {k[:-2]: v / iters * 1e3 for k, v in model.timing.items()},
           "losses": {k: model.logger[k] for k in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")},
           "diverged_envs": model.nonfinite_resets}
    env.close()
    return out


def callbacks_cost(a):
    """The `ref` configuration with and without the metrics callback, alternating, for the library-GEMM
    and the fused_mlp learner: the iteration times and their difference (reported, not judged)."""
    res = {"metric": "SAC iteration ms with / without DetailedMetricsCallback(log_freq=1000)", "unit": "ms",
           "config": {"name": "ref", **CONFIGS["ref"]}, "iters": a.iters, "warmup": a.warmup, "learners": {}}
    for label, mlp in (("fused", False), ("fused_mlp", True)):
        rows = [run("ref", True, a.iters, a.warmup, mlp, callbacks=on) for on in (False, True, False, True)]
        off = sum(r["iteration_ms"] for r in rows[0::2]) / 2
        on = sum(r["iteration_ms"] for r in rows[1::2]) / 2
        res["learners"][label] = {"runs": rows, "iteration_ms_off": off, "iteration_ms_on": on,
                                  "callback_ms_per_iteration": on - off}
    line = json.dumps(res)
    print(line, flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "sac_callbacks_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--configs", default="ref,wide")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--callbacks", action="store_true",
                    help="instead: what DetailedMetricsCallback(log_freq=1000) costs per iteration of `ref`, "
                         "off / on / off / on in this one process (default --out profiles/sac_callbacks_bench.json)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.callbacks:
        return callbacks_cost(a)
    res = {"metric": "SAC env-steps/sec (collect + sample + update)", "unit": "env-steps/s", "iters": a.iters,
           "warmup": a.warmup, "configs": {}}
    for name in a.configs.split(","):
        rows = [run(name, fused, a.iters, a.warmup, mlp) for fused, mlp in ((True, False), (False, False), (True, True))]
        res["configs"][name] = {**CONFIGS[name], "runs": rows,
                                "fused_over_plain": rows[0]["env_steps_per_s"] / rows[1]["env_steps_per_s"],
                                "fused_mlp_over_fused": rows[2]["env_steps_per_s"] / rows[0]["env_steps_per_s"]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
