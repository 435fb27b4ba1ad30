#!/usr/bin/env python3
"""WireFitting on the MI355X at the shipped settings -- Pendulum (3, 1), 200-wide layers, 100 wires, batch 32: updates
per second of 256 co-resident agents (device sampler, several updates per agent per launch), and for one agent alone the
microseconds per update and per `act`.  Beside it, measured the same way in the same process: the NAF any-shape kernel at
the same widths, and the torch restatement of WireFitting (tests/torch_ref_wf.py) on one CPU thread.  Every figure is the
median of `--repeats` timed launches after `--warmup` untimed ones, timed with device events on the handle's stream
(rlc_timer_begin / rlc_timer_end) and, beside it, a host clock around a synchronisation.  A record, not a check: writes
profiles/wf_throughput.json.
    python scripts/wf_throughput.py [--agents 256] [--updates 8] [--repeats 15] [--warmup 3]"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S, A, L1, L2, N, B, CAP = 3, 1, 200, 200, 100, 32, 4096
SMIN, SMAX = [-1, -1, -8], [1, 1, 8]


def replay_data():
    rng = np.random.RandomState(0)
    th = rng.uniform(0, 2 * np.pi, CAP)
    s = np.stack([np.cos(th), np.sin(th), rng.uniform(-8, 8, CAP)], 1)
    th2 = th + rng.uniform(-0.2, 0.2, CAP)
    s2 = np.stack([np.cos(th2), np.sin(th2), rng.uniform(-8, 8, CAP)], 1)
    return (s, rng.uniform(-2, 2, (CAP, A)), rng.uniform(-16, 0, CAP), s2, np.full(CAP, 0.99))


def population(kind, agents):
    seeds = np.arange(agents, dtype=np.uint64) + 1
    if kind == "wf":
        from rlcontrol_amd.hip_wf import WFPopulation, init_params
        pop = WFPopulation(agents, S, A, L1, L2, N, B, CAP, 0.01, SMIN, SMAX, 2.0, 1e-3, seeds=seeds)
        theta = lambda seed: init_params(S, A, L1, L2, N, seed)
    else:
        from rlcontrol_amd.hip_naf import NAFPopulation, init_params
        pop = NAFPopulation(agents, S, A, L1, L2, B, CAP, 0.01, SMIN, SMAX, [2.0], 1e-3, seeds=seeds)
        pop.set_kernel("generic")
        theta = lambda seed: init_params(S, A, L1, L2, seed)
    data = replay_data()
    for i in range(agents):
        pop.set_params(i, theta(int(seeds[i])))
        pop.replay_add_batch(i, *data)
    return pop


def timed(pop, fn, repeats, warmup):
    """median device-event and host milliseconds of fn()"""
    for _ in range(warmup):
        fn()
    pop.sync()
    ev, host = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        pop.timer_begin()
        fn()
        ev.append(pop.timer_end())
        host.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ev)), float(np.median(host)), [float(v) for v in ev]


def device_record(kind, a):
    out = OrderedDict()
    pop = population(kind, a.agents)
    ev, host, all_ev = timed(pop, lambda: pop.update(a.updates), a.repeats, a.warmup)
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))
    n = a.agents * a.updates
    out["population"] = OrderedDict(agents=a.agents, updates_per_agent_per_launch=a.updates, repeats=a.repeats, warmup=a.warmup,
                                    ms_per_launch_device_events=ev, ms_per_launch_host=host,
                                    updates_per_s=n / (ev * 1e-3), updates_per_s_host=n / (host * 1e-3),
                                    ms_per_launch_all=all_ev)
    pop.close()
    pop = population(kind, 1)
    ev, host, _ = timed(pop, lambda: pop.update(a.single_updates), a.repeats, a.warmup)
    state = np.array([[0.6, 0.8, 0.5]])
    ev1, host1, _ = timed(pop, lambda: pop.update(1), a.repeats, a.warmup)
    eva, hosta, _ = timed(pop, lambda: pop.act(state), a.repeats * 4, a.warmup)
    out["one_agent"] = OrderedDict(us_per_update_in_a_launch_of_many=ev * 1e3 / a.single_updates,
                                   updates_per_launch=a.single_updates, us_per_single_update_launch_device_events=ev1 * 1e3,
                                   us_per_single_update_launch_host=host1 * 1e3,
                                   us_per_act_device_events=eva * 1e3, us_per_act_host=hosta * 1e3)
    pop.close()
    return out


def restatement_record(a):
    import torch
    import torch_ref_wf as R
    torch.set_num_threads(1)
    o = R.TorchWireFitting((S, A, L1, L2, N), R.init_params((S, A, L1, L2, N), 1), 1e-3, 0.01, SMIN, SMAX, 2.0)
    s, act, r, s2, g = replay_data()
    rng = np.random.RandomState(1)
    batches = [rng.choice(CAP, B, replace=False) for _ in range(a.warmup + a.repeats)]
    ms = []
    for k, j in enumerate(batches):
        t0 = time.perf_counter()
        o.update(s[j], act[j], s2[j], r[j], g[j])
        if k >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    state = np.array([[0.6, 0.8, 0.5]])
    acts = []
    for k in range(a.warmup + a.repeats * 4):
        t0 = time.perf_counter()
        o.act(state)
        if k >= a.warmup:
            acts.append((time.perf_counter() - t0) * 1e6)
    return OrderedDict(threads=1, us_per_update=float(np.median(ms)) * 1e3, us_per_act=float(np.median(acts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--updates", type=int, default=8)
    ap.add_argument("--single-updates", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wf_throughput.json"))
    a = ap.parse_args()
    out = OrderedDict()
    out["workload"] = ("WireFitting (%d, %d), widths %d / %d, %d wires, batch %d, %d-record synthetic replays, device sampler"
                       % (S, A, L1, L2, N, B, CAP))
    out["wirefitting"] = device_record("wf", a)
    out["naf_any_shape_kernel_same_widths"] = device_record("naf", a)
    out["torch_restatement_one_cpu_thread"] = restatement_record(a)
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
