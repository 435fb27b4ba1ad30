#!/usr/bin/env python3
"""ReverseKL at action_dim 2 (the Bimodal2DEnv json shape: S=2, A=2, four 200-wide layers, batch 32, l_param 6 -> 187
sparse-grid nodes, 5984 (state, node) rows per update): throughput of the any-shape kernel and of the MFMA kernel, 256
co-resident agents on 1e6-record synthetic replays, timed as bench.py's `kl` record is (warm-up, then launches between
rlc_timer_begin / rlc_timer_end); then one whole Bimodal2DEnv device-loop run (main.py --device_rollout semantics) per
agent kind on each kernel.  A record, not a check: writes profiles/kl_action2_throughput.json.

Every GPU step runs in a fresh child process under its own time limit, one after the other; the first one that fails
ends the job (nothing more is started on the GPU).  This process itself never opens the GPU.
    python scripts/kl_action2_throughput.py [--agents 256] [--updates 8] [--steps 30] [--warmup 3]"""
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
DIMS = (2, 2, 200, 200, 200, 200)
B, L_PARAM, NODES = 32, 6, 187
PEAK_FP32_MATRIX = 157.3e12       # as bench.py: v_mfma_f32_* dense peak


def flop_per_update(B=B, K=NODES, S=DIMS[0], A=DIMS[1], L=200):
    """bench.py's _kl_flop with S + A inputs of the Q network: multiply-adds x 2 of pi, V, V' forward, Q(s,a) and
    Q(s,a_new) forward, Q at the B*K (state, node) pairs, the input and weight gradients of the three trained networks"""
    fwd = lambda rows, k_in: 2 * rows * (k_in * L + L * L + L)
    return float(fwd(B, S) * 3 + fwd(B, S + A) * 2 + fwd(B * K, S + A) + 3 * 2 * B * (L * L + L)
                 + 3 * 2 * B * (L * L + (S + A) * L + 2 * L))


def throughput(kernel, a):
    import torch
    from bench import REPLAY_N, _fill_from_host, measure, synthetic_uniform_replay
    from rlcontrol_amd.hip_kl import KLPopulation, init_params
    seeds = np.arange(a.agents, dtype=np.uint64) + 1
    pop = KLPopulation("reverse", a.agents, *DIMS, B, REPLAY_N, 0.01, 1.0, 1e-3, 1e-3, 0.1, seeds=seeds, n_param=64,
                       optim_type="intg", l_param=L_PARAM, action_max=np.ones(2))
    assert pop.n_nodes == NODES, pop.n_nodes
    pop.set_kernel(kernel)
    for i in range(a.agents):
        pop.set_params(i, init_params(*DIMS, int(seeds[i])))
    _fill_from_host(pop, synthetic_uniform_replay(REPLAY_N, DIMS[0], DIMS[1]), torch)
    dt, ev_ms = measure(pop, a.updates, a.steps, a.warmup, None, torch.cuda.synchronize)
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))
    n = a.agents * a.updates * a.steps
    flop = flop_per_update()
    rec = OrderedDict(kernel=pop.kernel_in_use(), updates_per_s=n / dt, updates_per_s_device_events=n / (ev_ms * 1e-3),
                      ms_per_launch=ev_ms / a.steps, updates_per_launch=a.agents * a.updates, launches_timed=a.steps,
                      warmup_launches=a.warmup, tflops=n / dt * flop / 1e12,
                      frac_of_fp32_matrix_peak=n / dt * flop / PEAK_FP32_MATRIX)
    pop.close()
    return rec


def device_loop(kernel, a):
    """one run (sweep index 0) of reverse_kl.json and of forward_kl.json on Bimodal2DEnv.json, on the device"""
    import main as drv
    import rlcontrol_amd.environments.environments as envs
    with open(os.path.join(ROOT, "jsonfiles", "environment", "Bimodal2DEnv.json")) as f:
        env_json = json.load(f, object_pairs_hook=OrderedDict)
    env = envs.create_environment(env_json)
    env_params = {"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min,
                  "state_max": env.state_max, "action_dim": env.action_dim, "action_min": env.action_min,
                  "action_max": env.action_max}
    out = OrderedDict()
    for tag in ("reverse_kl", "forward_kl"):
        with open(os.path.join(ROOT, "jsonfiles", "agent", tag + ".json")) as f:
            agent_json = json.load(f, object_pairs_hook=OrderedDict)
        agent_json["sweeps"]["buffer_size"] = [int(env_json["TotalMilSteps"] * 1000000)]
        agent_json["sweeps"]["hip_kernel"] = [kernel]
        used = {}

        def inspect(group, pop):
            used["kernel"] = pop.kernel_in_use()

        data = drv.new_data_dict(agent_json, env_json)
        t0 = time.time()
        drv.run_indices_on_device([0], agent_json, env_json, env_params,
                                  {"write_log": False, "write_plot": False, "device": 0}, data, verbose=False,
                                  inspect=inspect)
        wall = time.time() - t0
        run = [r for sd in data["experiment_data"].values() for r in sd["runs"]][0]
        out[agent_json["agent"]] = OrderedDict(kernel=used["kernel"], wall_s=wall, steps=int(run["total_timesteps"]),
                                               final_eval_return=float(np.mean(run["eval_episode_rewards"][-1])))
    return out


def run_steps(a, tmp):
    results = OrderedDict()
    # the any-shape kernel first (the yardstick), then the MFMA kernel, each in a fresh process
    for step, limit in (("throughput:generic", 240), ("throughput:mfma", 180), ("device_loop:generic", 240),
                        ("device_loop:mfma", 180)):
        path = os.path.join(tmp, "kl_action2_%s.json" % step.replace(":", "_"))
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--step-out", path, "--agents", str(a.agents),
               "--updates", str(a.updates), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            rc = subprocess.run(cmd, cwd=ROOT, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("%s ended with status %d: nothing more is started" % (step, rc), flush=True)
            return results, rc
        with open(path) as f:
            results[step] = json.load(f, object_pairs_hook=OrderedDict)
        print(step, json.dumps(results[step]), flush=True)
    return results, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--updates", type=int, default=8, help="updates per agent per launch")
    ap.add_argument("--steps", type=int, default=30, help="timed launches")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_action2_throughput.json"))
    ap.add_argument("--step", default="", help="(child) throughput:<kernel> or device_loop:<kernel>")
    ap.add_argument("--step-out", default="")
    a = ap.parse_args()
    if a.step:
        what, kernel = a.step.split(":")
        rec = throughput(kernel, a) if what == "throughput" else device_loop(kernel, a)
        with open(a.step_out, "w") as f:
            json.dump(rec, f)
        return 0
    with tempfile.TemporaryDirectory() as tmp:           # the children's partial records
        results, rc = run_steps(a, tmp)
    if rc != 0:
        return rc
    g, m = results["throughput:generic"], results["throughput:mfma"]
    out = OrderedDict(
        workload="ReverseKL optim_type intg, S=2 A=2, four 200-wide layers, batch 32, l_param 6 (187 nodes: 5984 Q "
                 "evaluations per update), %d agents, 1e6-record synthetic replays, device sampler" % a.agents,
        flop_per_update=flop_per_update(), fp32_matrix_peak_tflops=PEAK_FP32_MATRIX / 1e12,
        any_shape_kernel=g, mfma_kernel=m, mfma_over_any_shape=m["updates_per_s"] / g["updates_per_s"],
        bimodal2d_device_loop=OrderedDict(any_shape_kernel=results["device_loop:generic"],
                                          mfma_kernel=results["device_loop:mfma"]))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
