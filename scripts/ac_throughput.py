#!/usr/bin/env python3
"""ActorCritic on the MI355X at the shipped settings -- Pendulum (3, 1), 200-wide layers, critic_update sampled,
actor_update ll, 30 samples: updates per second of 256 co-resident agents at batch 32 and at batch 100 (device sampler, the device's own
draws, several updates per agent per launch), and for one agent alone at batch 32 the microseconds per update and per
acting step (greedy and sampled).  Every figure is the median of `--repeats` timed launches after `--warmup` untimed ones,
timed with device events on the handle's stream (rlc_timer_begin / rlc_timer_end) and, beside it, a host clock around a
synchronisation.  A record, not a check: writes profiles/ac_throughput.json.
    python scripts/ac_throughput.py [--agents 256] [--updates 8] [--repeats 15] [--warmup 3]"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, A, L1, LA, LC, N, K, CAP = 3, 1, 200, 200, 200, 30, 6, 4096
SMIN, SMAX = [-1, -1, -8], [1, 1, 8]


def replay_data():
    rng = np.random.RandomState(0)
    th = rng.uniform(0, 2 * np.pi, CAP)
    s = np.stack([np.cos(th), np.sin(th), rng.uniform(-8, 8, CAP)], 1)
    th2 = th + rng.uniform(-0.2, 0.2, CAP)
    s2 = np.stack([np.cos(th2), np.sin(th2), rng.uniform(-8, 8, CAP)], 1)
    return (s, rng.uniform(-2, 2, (CAP, A)), rng.uniform(-16, 0, CAP), s2, np.full(CAP, 0.99))


def population(agents, batch):
    from rlcontrol_amd.hip_ac import ACPopulation, init_params
    seeds = np.arange(agents, dtype=np.uint64) + 1
    pop = ACPopulation(agents, S, A, L1, LA, LC, N, K, batch, CAP, 0.01, SMIN, SMAX, [2.0], 1e-3, 1e-2, seeds=seeds,
                       critic_update="sampled", actor_update="ll")
    data = replay_data()
    for i in range(agents):
        pop.set_params(i, init_params(S, A, L1, LA, LC, int(seeds[i])))
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


def population_record(a, batch):
    pop = population(a.agents, batch)
    ev, host, all_ev = timed(pop, lambda: pop.update(a.updates), a.repeats, a.warmup)
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))
    n = a.agents * a.updates
    pop.close()
    return OrderedDict(agents=a.agents, batch=batch, updates_per_agent_per_launch=a.updates, repeats=a.repeats,
                       warmup=a.warmup, ms_per_launch_device_events=ev, ms_per_launch_host=host,
                       updates_per_s=n / (ev * 1e-3), updates_per_s_host=n / (host * 1e-3), ms_per_launch_all=all_ev)


def one_agent_record(a):
    pop = population(1, 32)
    ev, _, _ = timed(pop, lambda: pop.update(a.single_updates), a.repeats, a.warmup)
    state = np.array([[0.6, 0.8, 0.5]])
    ev1, host1, _ = timed(pop, lambda: pop.update(1), a.repeats, a.warmup)
    eva, hosta, _ = timed(pop, lambda: pop.act(state), a.repeats * 4, a.warmup)
    evs, hosts, _ = timed(pop, lambda: pop.act(state, sample=True), a.repeats * 4, a.warmup)
    pop.close()
    return OrderedDict(batch=32, us_per_update_in_a_launch_of_many=ev * 1e3 / a.single_updates,
                       updates_per_launch=a.single_updates, us_per_single_update_launch_device_events=ev1 * 1e3,
                       us_per_single_update_launch_host=host1 * 1e3, us_per_greedy_act_device_events=eva * 1e3,
                       us_per_greedy_act_host=hosta * 1e3, us_per_sampled_act_device_events=evs * 1e3,
                       us_per_sampled_act_host=hosts * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--updates", type=int, default=8)
    ap.add_argument("--single-updates", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ac_throughput.json"))
    a = ap.parse_args()
    out = OrderedDict()
    out["workload"] = ("ActorCritic (%d, %d), widths %d / %d / %d, critic_update sampled, actor_update ll, %d samples, "
                       "%d-record synthetic replays, device sampler, device draws" % (S, A, L1, LA, LC, N, CAP))
    out["one_agent"] = one_agent_record(a)
    out["population_batch_32"] = population_record(a, 32)
    out["population_batch_100"] = population_record(a, 100)
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
