#!/usr/bin/env python3
"""The wide form of the NAF MFMA kernel (state_dim <= 32, action_dim in {1,2,3,4,6}; set_kernel("mfma")) against the
any-shape kernel at the reference's MuJoCo shapes -- Reacher-v2 (11, 2), Hopper-v2 (11, 3), HalfCheetah-v2 (17, 6) --
with 128-wide layers and 200-wide ones (the shipped naf.json), batch 32, 64 and 100: 256 co-resident agents on 1e6-record
synthetic replays, device sampler, timed as bench.py times its record (warm-up launches, then launches between
rlc_timer_begin / rlc_timer_end and a host clock around a sync).  Both kernels of a shape run in ONE process, the
any-shape kernel (the yardstick: unchanged code) first; a shape the LDS carve refuses is recorded with the refusal.  Then
one agent alone at (17, 6) batch 32, the table of LDS bytes from the library's own refusals, and -- given the tree of the
parent commit, built -- the DDPG headline and the `naf` record of bench.py on both trees in turn.
A record, not a check: writes profiles/naf_wide_throughput.json.

Every GPU step runs in a fresh child process under its own time limit, one after the other; the first one that fails
ends the job (nothing more is started on the GPU).  This process itself never opens the GPU.
    python scripts/naf_wide_throughput.py [--agents 256] [--updates 16] [--steps 30] [--warmup 3] [--parent-tree DIR]"""
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
WIDTHS = (128, 200)
SHAPES = OrderedDict([("Reacher-v2", (11, 2)), ("Hopper-v2", (11, 3)), ("HalfCheetah-v2", (17, 6))])
PEAK_FP32_MATRIX = 157.3e12       # as bench.py: v_mfma_f32_* dense peak


def flop_per_update(S, A, B, L):
    """multiply-adds x 2 of one update, counted from the kernel's phase list (naf_mfma_kernel.h): seven [B, L] x [L, L]
    contractions (V', mu and V forward; two input-gradient and two weight-gradient ones), two first-layer passes and one
    first-layer gradient, the A(A+1)/2 L heads (forward, their term of the first-layer gradient, weight gradient), the A
    mu columns and the V column (forward, seed, weight gradient) and V'"""
    NH = A * (A + 1) // 2
    mac = 7 * L * L + 3 * S * L + 3 * NH * L + 3 * (A + 1) * L + L
    return 2.0 * mac * B


def _population(S, A, B, L, agents, cap):
    from rlcontrol_amd.hip_naf import NAFPopulation, init_params
    seeds = np.arange(agents, dtype=np.uint64) + 1
    pop = NAFPopulation(agents, S, A, L, L, B, cap, 0.01, -np.ones(S) * 10, np.ones(S) * 10, np.ones(A), 1e-3, seeds=seeds)
    for i in range(agents):
        pop.set_params(i, init_params(S, A, L, L, int(seeds[i])))
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


def throughput(S, A, B, L, a, agents, updates):
    """both kernels on one population in one process: the any-shape kernel, then the same agents re-packed for MFMA"""
    import torch
    from bench import REPLAY_N, _fill_from_host, synthetic_uniform_replay
    from rlcontrol_amd._lib import RlcError
    pop = _population(S, A, B, L, agents, REPLAY_N)
    try:
        pop.set_kernel("mfma")
    except RlcError as e:                         # the LDS carve does not take the shape at this batch
        pop.close()
        return OrderedDict(state_dim=S, action_dim=A, batch=B, widths=L, mfma_refused=str(e))
    pop.set_kernel("generic")
    _fill_from_host(pop, synthetic_uniform_replay(REPLAY_N, S, A), torch)
    flop = flop_per_update(S, A, B, L)
    g = _timed(pop, "generic", a, agents, updates, flop)
    m = _timed(pop, "mfma", a, agents, updates, flop)
    pop.close()
    return OrderedDict(state_dim=S, action_dim=A, batch=B, widths=L, agents=agents, flop_per_update=flop, any_shape_kernel=g,
                       mfma_kernel=m, mfma_over_any_shape=m["updates_per_s"] / g["updates_per_s"])


def lds_table():
    """LDS bytes of the wide carve at the MuJoCo shapes, from the library's own refusals: a population one float too wide
    to fit never exists, so each cell asks set_kernel("mfma") and records "fits" or the refusal with its byte count"""
    from rlcontrol_amd._lib import RlcError
    out = OrderedDict()
    for L in WIDTHS:
        for S, A in SHAPES.values():
            for B in (32, 64, 100, 128):
                pop = _population(S, A, B, L, 1, 128)
                key = "S=%d A=%d widths %d batch %d" % (S, A, L, B)
                try:
                    pop.set_kernel("mfma")
                    out[key] = "fits"
                except RlcError as e:
                    out[key] = str(e)
                pop.close()
    for k, v in out.items():
        print(k, v)
    return out


def child(step, a):
    what = step.split(":")
    if what[0] == "throughput":
        S, A, B, L = int(what[1]), int(what[2]), int(what[3]), int(what[4])
        return throughput(S, A, B, L, a, a.agents, a.updates)
    if what[0] == "single":
        return throughput(17, 6, 32, 128, a, 1, 200)
    return lds_table()


def headline_ab(parent, runs):
    """the DDPG headline (plain bench.py) and the `naf` record of bench.py --full (its --side-only naf form: the same
    measurement without the other side records) on the parent commit's tree and on this one, alternating"""
    cmds = OrderedDict([("", ["bench.py", "--gpus", "1"]), ("_naf", ["bench.py", "--gpus", "1", "--side-only", "naf"])])
    rec = OrderedDict(commands=[" ".join(c) for c in cmds.values()], parent=[], this=[], parent_naf=[], this_naf=[])
    for i in range(runs):
        for tag, tree in (("parent", parent), ("this", ROOT)):
            for what, cmd in cmds.items():
                try:
                    p = subprocess.run([sys.executable] + cmd, cwd=tree, timeout=240, stdout=subprocess.PIPE, text=True)
                    rc = p.returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print("%s in %s ended with status %d: nothing more is started" % (" ".join(cmd), tree, rc), flush=True)
                    return None, rc
                line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
                rec[tag + what].append(float(json.loads(line)["value"]))
                print("headline" + what, tag, i, rec[tag + what][-1], flush=True)
    for what in cmds:
        for tag in ("parent", "this"):
            v = np.array(rec[tag + what])
            rec[tag + what + "_mean"], rec[tag + what + "_spread_max_minus_min"] = float(v.mean()), float(v.max() - v.min())
        diff = rec["this" + what + "_mean"] - rec["parent" + what + "_mean"]
        rec["mean_difference_this_minus_parent" + what] = diff
        rec["inside_parent_spread" + what] = bool(abs(diff) <= rec["parent" + what + "_spread_max_minus_min"])
    return rec, 0


def run_steps(a, tmp):
    results = OrderedDict()
    steps = [("lds_table", 120)]
    for L in WIDTHS:
        for B in (32, 64, 100):
            steps += [("throughput:%d:%d:%d:%d" % (sa + (B, L)), 420) for sa in SHAPES.values()]
    steps += [("single", 180)]
    for step, limit in steps:
        path = os.path.join(tmp, "naf_wide_%s.json" % step.replace(":", "_"))
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
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: adds the headline_ab record")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "naf_wide_throughput.json"))
    ap.add_argument("--step", default="", help="(child) lds_table, throughput:<S>:<A>:<batch>:<widths> or single")
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
    names = {v: k for k, v in SHAPES.items()}
    shapes = OrderedDict()
    for step, rec in results.items():
        if step.startswith("throughput:"):
            _, S, A, B, L = step.split(":")
            shapes["%s (%s, %s) widths %s batch %s" % (names[(int(S), int(A))], S, A, L, B)] = rec
    out = OrderedDict(
        workload="NAF, %d agents, 1e6-record synthetic replays, device sampler, %d updates per "
                 "agent per launch; the any-shape kernel is the yardstick" % (a.agents, a.updates),
        fp32_matrix_peak_tflops=PEAK_FP32_MATRIX / 1e12, throughput=shapes,
        one_agent_alone_17_6_widths128_batch32=results["single"], lds_table=results["lds_table"])
    if a.parent_tree:
        ab, rc = headline_ab(os.path.abspath(a.parent_tree), a.ab_runs)
        if rc != 0:
            return rc
        out["headline_ab"] = ab
    else:
        out["headline_ab"] = "not measured"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
