#!/usr/bin/env python3
"""Generate tests/golden/optimalq_grid.json by calling the REFERENCE's own
OptimalQ_Network.compute_discretized_action_pairs (agents/network/optimal_q_network.py:163-179).

    RLCONTROL_REFERENCE=<checkout of the reference> python tests/golden/make_optimalq_golden.py

The reference's module imports TensorFlow 1.15 at its top, which is absent; the grid method uses numpy only, so the
module is imported with an empty stand-in for ``tensorflow`` in sys.modules and the method is called on an instance made
with object.__new__ that carries just the four attributes it reads (action_min, action_max, action_dim,
discretization).  Only inputs and outputs are recorded -- no reference source text:

  * four small cases with their full float64 grids [n_nodes][action_dim];
  * the shipped Pendulum grid ([-2], [2], 1e-3, action_dim 1): the node count, its first three and last three values
    and the sha256 of its float64 bytes (little-endian, C order).
"""
import hashlib
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RLCONTROL_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set RLCONTROL_REFERENCE (or pass the path) to a checkout of the reference")

sys.modules.setdefault("tensorflow", types.ModuleType("tensorflow"))
sys.path.insert(0, REF)
from agents.network.optimal_q_network import OptimalQ_Network  # noqa: E402

FULL = [([-2.0], [2.0], 0.1, 1), ([-2.0], [2.0], 0.5, 2), ([-1.0], [1.0], 1.0, 3), ([-2.0], [2.0], 8.0, 1)]
DIGEST = ([-2.0], [2.0], 1e-3, 1)


def grid(action_min, action_max, discretization, action_dim):
    net = object.__new__(OptimalQ_Network)
    net.action_min, net.action_max = np.array(action_min), np.array(action_max)
    net.action_dim, net.discretization = action_dim, discretization
    g = np.asarray(net.compute_discretized_action_pairs(), np.float64)
    return g.reshape(-1, action_dim)


def case(args):
    return OrderedDict(zip(("action_min", "action_max", "discretization", "action_dim"), args))


def main():
    out = OrderedDict()
    out["source"] = ("OptimalQ_Network.compute_discretized_action_pairs (agents/network/optimal_q_network.py:163-179) of "
                     "the reference, run by tests/golden/make_optimalq_golden.py")
    out["full"] = []
    for args in FULL:
        g = grid(*args)
        rec = case(args)
        rec["n_nodes"] = int(g.shape[0])
        rec["grid"] = g.tolist()
        out["full"].append(rec)
    g = grid(*DIGEST)
    rec = case(DIGEST)
    rec["n_nodes"] = int(g.shape[0])
    rec["first"] = g[:3, 0].tolist()
    rec["last"] = g[-3:, 0].tolist()
    rec["sha256_float64"] = hashlib.sha256(np.ascontiguousarray(g, "<f8").tobytes()).hexdigest()
    out["digest"] = rec
    path = os.path.join(HERE, "optimalq_grid.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
