#!/usr/bin/env python3
"""The layer-norm form of the DDPG MFMA kernel (norm_type 'layer', the hydra network at state_dim <= 8, action_dim <= 2;
set_kernel("mfma")) against the any-shape kernel at the Pendulum shape of jsonfiles/agent/ddpg_layer.json: 256 co-resident
agents at (3, 1, 200, 200, 200) batch 32 and batch 64 and at (3, 1, 128, 128, 128) batch 100, on 1e6-record synthetic
replays, device sampler, timed as bench.py times its record (warm-up launches, then launches between rlc_timer_begin /
rlc_timer_end and a host clock around a sync).  Both kernels of a shape run in ONE process, the any-shape kernel (the
yardstick: unchanged code) first.  Then one agent alone at batch 32, and the table of what the LDS carve takes per tile
count.  A record, not a check: writes profiles/ddpg_layer_throughput.json.

Every GPU step runs in a fresh child process under its own time limit, one after the other; the first one that fails
ends the job (nothing more is started on the GPU).  This process itself never opens the GPU.
    python scripts/ddpg_layer_throughput.py [--agents 256] [--updates 16] [--steps 30] [--warmup 3]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, A = 3, 1
CASES = [(200, 32), (200, 64), (128, 100)]          # (layer width, batch)
PEAK_FP32_MATRIX = 157.3e12       # as bench.py: v_mfma_f32_* dense peak


def flop_per_update(B, L):
    """multiply-adds x 2 of one update as scripts/ddpg_wide_throughput.py counts them (the layer norms' O(B L) work is
    not counted)"""
    l1 = S * L
    actor = L * L + L * A
    critic = (L + A) * L + L
    mac = (l1 + actor + critic)
    mac += l1 + critic
    mac += critic + L * L + l1 + critic
    mac += l1 + actor
    mac += critic + L * A
    mac += L * A + L * L + l1 + actor
    return 2.0 * mac * B


def _population(L, B, agents, cap):
    from rlcontrol_amd.hip_ddpg import DDPGPopulation, init_params
    seeds = np.arange(agents, dtype=np.uint64) + 1
    pop = DDPGPopulation(agents, S, A, L, L, L, B, cap, 0.01, -np.ones(S), np.ones(S), -np.ones(A), np.ones(A), 1e-3, 1e-2,
                         seeds=seeds, norm_type="layer")
    for i in range(agents):
        pop.set_params(i, init_params(S, A, L, L, L, int(seeds[i]), "layer"))
    return pop

def _timed(pop, kernel, a, agents, updates, flop):
    import torch
    from bench import measure
    pop.set_kernel(kernel)
    assert pop.kernel_in_use() == kernel
    dt, ev_ms = measure(pop, updates, a.steps, a.warmup, None, torch.cuda.synchronize)
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))
    n = agents * updates * a.steps
    return OrderedDict(kernel=kernel, updates_per_s=n / dt, updates_per_s_device_events=n / (ev_ms * 1e-3),
                       ms_per_launch=ev_ms / a.steps, us_per_update_per_agent=ev_ms * 1e3 / (a.steps * updates),
                       updates_per_launch=agents * updates, launches_timed=a.steps, warmup_launches=a.warmup,
                       tflops=n / dt * flop / 1e12, frac_of_fp32_matrix_peak=n / dt * flop / PEAK_FP32_MATRIX)


def throughput(L, B, a, agents, updates):
    """both kernels on one population in one process: the any-shape kernel, then the same agents re-packed for MFMA"""
    import torch
    from bench import REPLAY_N, _fill_from_host, synthetic_uniform_replay
    from rlcontrol_amd._lib import RlcError
    pop = _population(L, B, agents, REPLAY_N)
    try:
        pop.set_kernel("mfma")
    except RlcError as e:                         # the LDS carve does not take the shape at this batch
        pop.close()
        return OrderedDict(width=L, batch=B, mfma_refused=str(e))
    pop.set_kernel("generic")
    _fill_from_host(pop, synthetic_uniform_replay(REPLAY_N, S, A), torch)
    flop = flop_per_update(B, L)
    g = _timed(pop, "generic", a, agents, updates, flop)
    m = _timed(pop, "mfma", a, agents, updates, flop)
    pop.close()
    return OrderedDict(state_dim=S, action_dim=A, width=L, batch=B, agents=agents, flop_per_update=flop, any_shape_kernel=g,
                       mfma_kernel=m, mfma_over_any_shape=m["updates_per_s"] / g["updates_per_s"])


def lds_table():
    """what the kernel's LDS carve takes per tile count (batch 32 / 64 / 112 / 128 = 2 / 4 / 7 / 8 tiles) at equal layer
    widths; a refusal carries the byte counts"""
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    from rlcontrol_amd._lib import RlcError
    out = OrderedDict()
    for B in (32, 64, 112, 128):
        for L in (256, 200, 136, 128, 120, 104):
            pop = DDPGPopulation(1, S, A, L, L, L, B, 128, 0.01, -np.ones(S), np.ones(S), -np.ones(A), np.ones(A), 1e-3, 1e-2,
                                 seeds=[1], norm_type="layer")
            try:
                pop.set_kernel("mfma")
                out["batch=%d width=%d" % (B, L)] = "fits"
            except RlcError as e:
                out["batch=%d width=%d" % (B, L)] = str(e)
            pop.close()
    for k, v in out.items():
        print(k, v)
    return out


def child(step, a):
    what = step.split(":")
    if what[0] == "throughput":
        return throughput(int(what[1]), int(what[2]), a, a.agents, a.updates)
    if what[0] == "single":
        return throughput(200, 32, a, 1, 200)
    return lds_table()


def run_steps(a, tmp):
    results = OrderedDict()
    steps = [("lds_table", 120)] + [("throughput:%d:%d" % c, 420) for c in CASES] + [("single", 180)]
    for step, limit in steps:
        path = os.path.join(tmp, "ddpg_layer_%s.json" % step.replace(":", "_"))
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
    ap.add_argument("--updates", type=int, default=16, help="updates per agent per launch")
    ap.add_argument("--steps", type=int, default=30, help="timed launches")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_layer_throughput.json"))
    ap.add_argument("--step", default="", help="(child) lds_table, throughput:<width>:<batch> or single")
    ap.add_argument("--step-out", default="")
    a = ap.parse_args()
    if a.step:
        with open(a.step_out, "w") as f:
            json.dump(child(a.step, a), f)
        return 0
    with tempfile.TemporaryDirectory() as tmp:           # the children's partial records
        results, rc = run_steps(a, tmp)
    if rc != 0:
        return rc
    shapes = OrderedDict()
    for step, rec in results.items():
        if step.startswith("throughput:"):
            _, L, B = step.split(":")
            shapes["(3, 1, %s, %s, %s) batch %s" % (L, L, L, B)] = rec
    out = OrderedDict(
        workload="DDPG with norm_type 'layer', hydra network, %d agents, 1e6-record synthetic replays, device sampler, %d "
                 "updates per agent per launch; the any-shape kernel is the yardstick" % (a.agents, a.updates),
        fp32_matrix_peak_tflops=PEAK_FP32_MATRIX / 1e12, throughput=shapes,
        one_agent_alone_width200_batch32=results["single"], lds_fit=results["lds_table"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
