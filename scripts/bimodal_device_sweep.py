#!/usr/bin/env python3
"""The reference's whole ddpg.json, reverse_kl.json and forward_kl.json sweeps x 5 seeds on Bimodal1DEnv, every run
on the device (main.py --device_rollout semantics; 750 one-step episodes per run).  Writes
profiles/bimodal_device_sweep.json with, per agent: wall time, the final mean evaluation return (the environment's
maximum is 1.5 at a = 1, the lower peak is 1.0 at a = -1) and the share of runs whose final greedy action lies
within 0.2 of each peak.  A record, not a check: no threshold is set.
    python scripts/bimodal_device_sweep.py [--seeds 5]"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import main as drv  # noqa: E402
import rlcontrol_amd.environments.environments as envs  # noqa: E402
from rlcontrol_amd.utils.main_utils import get_sweep_parameters  # noqa: E402

AGENTS = ("ddpg", "reverse_kl", "forward_kl")


def run():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--env_json", default=os.path.join(ROOT, "jsonfiles/environment/Bimodal1DEnv.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bimodal_device_sweep.json"))
    args = ap.parse_args()
    with open(args.env_json) as f:
        env_json = json.load(f, object_pairs_hook=OrderedDict)
    env = envs.create_environment(env_json)
    env_params = {"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min,
                  "state_max": env.state_max, "action_dim": env.action_dim, "action_min": env.action_min,
                  "action_max": env.action_max}
    out = OrderedDict(env=env_json, seeds=args.seeds, agents=OrderedDict())
    for tag in AGENTS:
        with open(os.path.join(ROOT, "jsonfiles", "agent", tag + ".json")) as f:
            agent_json = json.load(f, object_pairs_hook=OrderedDict)
        # a run never stores more than its steps: the default 1e6-transition replay would only cost device memory
        agent_json["sweeps"]["buffer_size"] = [int(env_json["TotalMilSteps"] * 1000000)]
        n_settings = get_sweep_parameters(agent_json["sweeps"], 0)[1]
        indices = list(range(n_settings * args.seeds))
        greedy = {}

        def inspect(group, pop):
            acts = pop.act(np.zeros((len(group), env.state_dim)))          # the greedy action at the start state
            greedy.update({i: float(a[0]) for i, a in zip(group, acts)})

        data = drv.new_data_dict(agent_json, env_json)
        t0 = time.time()
        drv.run_indices_on_device(indices, agent_json, env_json, env_params,
                                  {"write_log": False, "write_plot": False, "device": 0}, data, verbose=False,
                                  inspect=inspect)
        wall = time.time() - t0
        final = np.array([np.mean(r["eval_episode_rewards"][-1]) for sd in data["experiment_data"].values()
                          for r in sd["runs"]])
        a = np.array([greedy[i] for i in indices])
        per_setting = OrderedDict()
        for sweep, sd in data["experiment_data"].items():
            ga = np.array([greedy[i] for i in indices if i % n_settings == sweep])
            per_setting[str(sweep)] = {
                "agent_params": {k: v for k, v in sd["agent_params"].items() if k != "writer"},
                "final_eval_return_mean": float(np.mean([np.mean(r["eval_episode_rewards"][-1]) for r in sd["runs"]])),
                "final_greedy_actions": ga.tolist()}
        rec = OrderedDict(agent=agent_json["agent"], n_settings=n_settings, n_runs=len(indices), wall_s=wall,
                          final_eval_return_mean=float(final.mean()), final_eval_return_max=float(final.max()),
                          share_near_upper_peak=float(np.mean(np.abs(a - 1.0) <= 0.2)),
                          share_near_lower_peak=float(np.mean(np.abs(a + 1.0) <= 0.2)), settings=per_setting)
        out["agents"][tag] = rec
        print("%-10s %3d settings x %d seeds in %6.1f s: final eval return %.3f (best run %.3f); greedy action within 0.2 of "
              "+1: %.0f %%, of -1: %.0f %%" % (tag, n_settings, args.seeds, wall, rec["final_eval_return_mean"],
                                               rec["final_eval_return_max"], 100 * rec["share_near_upper_peak"],
                                               100 * rec["share_near_lower_peak"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    run()
