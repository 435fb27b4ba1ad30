#!/usr/bin/env python3
"""The shipped jsonfiles/agent/ddpg_layer.json sweep (49 settings, norm_type 'layer', 200-wide layers, batch 32) on
Pendulum-v0 through the on-device experiment loop (main.py --device_rollout semantics), twice over the same indices: on
the any-shape kernel (no "hip_kernel" key) and with "hip_kernel": "mfma" (the layer-norm form of the MFMA kernel).  A step
budget short enough for one sitting replaces the json's 100,000 steps.  Writes wall time and updates/s of both runs to
profiles/ddpg_layer_device_sweep.json.  A record, not a check: no ratio is asserted.

Each run is a fresh child process under its own time limit, the any-shape kernel (unchanged code) first; a run that
fails ends the job and nothing more is started on the GPU.  This process itself never opens the GPU.
    python scripts/ddpg_layer_device_sweep.py [--steps 4000] [--seeds 1]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(kernel, a):
    import main as drv
    import rlcontrol_amd.environments.environments as envs
    from rlcontrol_amd.utils.main_utils import get_sweep_parameters
    with open(os.path.join(ROOT, "jsonfiles", "environment", "Pendulum-v0.json")) as f:
        env_json = json.load(f, object_pairs_hook=OrderedDict)
    env_json["TotalMilSteps"] = a.steps / 1e6
    env_json["EvalIntervalMilSteps"] = a.eval_interval / 1e6
    env_json["EvalEpisodes"] = a.eval_episodes
    with open(os.path.join(ROOT, "jsonfiles", "agent", "ddpg_layer.json")) as f:
        agent_json = json.load(f, object_pairs_hook=OrderedDict)
    # a run never stores more than its steps: the default 1e6-transition replay would only cost device memory
    agent_json["sweeps"]["buffer_size"] = [a.steps]
    if kernel != "auto":
        agent_json["sweeps"]["hip_kernel"] = [kernel]
    env = envs.create_environment(env_json)
    env_params = {"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min, "state_max": env.state_max,
                  "action_dim": env.action_dim, "action_min": env.action_min, "action_max": env.action_max}
    n_settings = get_sweep_parameters(agent_json["sweeps"], 0)[1]
    indices = list(range(n_settings * a.seeds))
    seen = []

    def inspect(group, pop):
        seen.append((len(group), pop.kernel_in_use(), [int(pop.replay_size(i)) for i in range(len(group))],
                     bool(all(np.all(np.isfinite(pop.get_blob(i, "theta"))) for i in range(len(group)))), int(pop.B)))

    data = drv.new_data_dict(agent_json, env_json)
    t0 = time.time()
    drv.run_indices_on_device(indices, agent_json, env_json, env_params, {"write_log": False, "write_plot": False, "device": 0},
                              data, verbose=False, inspect=inspect)
    wall = time.time() - t0
    assert len(seen) == 1, seen                   # one population: every setting shares the shape
    n_agents, in_use, sizes, finite, batch = seen[0]
    # learn() runs at every step once the replay holds more than a batch (the first `batch` steps store only; a
    # transition truncated at the 200-step limit is not stored, but learn() still runs at that step)
    updates = n_agents * max(0, a.steps - batch)
    final = np.array([np.mean(r["eval_episode_rewards"][-1]) for sd in data["experiment_data"].values() for r in sd["runs"]])
    return OrderedDict(hip_kernel=kernel, kernel_in_use=in_use, agents=n_agents, steps_per_agent=a.steps, batch_size=batch,
                       wall_s=wall, updates=updates, updates_per_s=updates / wall, env_steps_per_s=n_agents * a.steps / wall,
                       replay_sizes_min_max=[min(sizes), max(sizes)], all_weights_finite=finite,
                       final_eval_return_mean=float(final.mean()), final_eval_return_best=float(final.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000, help="training steps per agent")
    ap.add_argument("--seeds", type=int, default=1, help="runs per setting (49 settings)")
    ap.add_argument("--eval-interval", type=int, default=1000)
    ap.add_argument("--eval-episodes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one run in seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_layer_device_sweep.json"))
    ap.add_argument("--kernel", default="", help="(child) auto or mfma")
    ap.add_argument("--kernel-out", default="")
    a = ap.parse_args()
    if a.kernel:
        with open(a.kernel_out, "w") as f:
            json.dump(child(a.kernel, a), f)
        return 0
    runs = OrderedDict()
    with tempfile.TemporaryDirectory() as tmp:
        for kernel in ("auto", "mfma"):
            path = os.path.join(tmp, kernel + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--kernel", kernel, "--kernel-out", path, "--steps", str(a.steps),
                   "--seeds", str(a.seeds), "--eval-interval", str(a.eval_interval), "--eval-episodes", str(a.eval_episodes)]
            try:
                rc = subprocess.run(cmd, cwd=ROOT, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("the %s run ended with status %d: nothing more is started" % (kernel, rc), flush=True)
                return rc
            with open(path) as f:
                runs[kernel] = json.load(f, object_pairs_hook=OrderedDict)
            print(kernel, json.dumps(runs[kernel]), flush=True)
    assert runs["auto"]["kernel_in_use"] == "generic" and runs["mfma"]["kernel_in_use"] == "mfma"
    out = OrderedDict(
        workload="jsonfiles/agent/ddpg_layer.json x %d seed(s) on Pendulum-v0 in the on-device loop, %d steps per agent, an "
                 "evaluation of %d episodes every %d steps; wall time covers the whole driver call (population, loop, "
                 "evaluations, logs)" % (a.seeds, a.steps, a.eval_episodes, a.eval_interval),
        any_shape_kernel=runs["auto"], mfma_kernel=runs["mfma"],
        mfma_over_any_shape_wall=runs["auto"]["wall_s"] / runs["mfma"]["wall_s"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
