#!/usr/bin/env python3
"""Generate tests/golden/bimodal_envs.json by running the REFERENCE's own toy environments
(environments/environments.py:158-912: the seven Bimodal1DEnv* classes and Bimodal2DEnvironment).

    RLCONTROL_REFERENCE=<checkout of the reference> python tests/golden/make_bimodal_golden.py

The reference's module imports gym and matplotlib at its top; neither is used by the toy environments, so the
module is imported with an empty stand-in for ``gym`` in sys.modules and matplotlib on the Agg backend.  Only
inputs and outputs are recorded -- no reference source text:

  * per environment: the attributes Experiment and main.py read, the EPISODE_STEPS_LIMIT a json with
    ``EpisodeSteps: -1`` gives, and ``reset()``;
  * 1-D family: the settings of the reference's seven jsonfiles/environment/Bimodal1DEnv*.json (the step budgets the
    shipped files are compared with) and ``(state', reward, done)`` for about 200 actions per variant.  Every action
    is a float32 value held in a float64 array (device actions are float32): a grid over [-3, 3] -- points beyond the
    [-2, 2] box included, since NAF's and SoftActorCritic's samples can leave it before clipping -- plus +-2, every
    variant's peaks and 0;
  * Bimodal2DEnv (the reference ships no json for it: it is built from this repository's own Bimodal2DEnv.json):
    scripted trajectories of float32 actions recorded step by step -- a straight run into each goal, an oblique
    run into a goal, a run into the wall where the clip is active, and one that never terminates.

A run of the reference's Experiment.run_episode_train bookkeeping is NOT recorded: experiment.py imports the
TensorFlow 1.15 agents, which are absent.  The episode rules the device loop and tests/helpers/bimodal_rollout.py
follow are taken from the text of experiment.py:102-160,196-215.
"""
import contextlib
import io
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("RLCONTROL_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set RLCONTROL_REFERENCE (or pass the path) to a checkout of the reference")

sys.modules.setdefault("gym", types.ModuleType("gym"))
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    import environments.environments as ref_envs  # noqa: E402

NAMES_1D = ["Bimodal1DEnv", "Bimodal1DEnv_uneq_var1", "Bimodal1DEnv_uneq_var2", "Bimodal1DEnv_uneq_var3",
            "Bimodal1DEnv_eq_var1", "Bimodal1DEnv_eq_var2", "Bimodal1DEnv_eq_var3"]
ATTRS = ["name", "eval_interval", "eval_episodes", "TOTAL_STEPS_LIMIT", "EPISODE_STEPS_LIMIT", "state_dim", "state_min",
         "state_max", "state_range", "state_bounded", "action_dim", "action_min", "action_max", "action_range"]


def plain(v):
    if isinstance(v, np.ndarray):
        return [plain(x) for x in v.tolist()]
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.bool_, bool)):
        return bool(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return v


def make(env_json):
    with contextlib.redirect_stdout(io.StringIO()):        # Bimodal2DEnvironment prints from its constructor
        return ref_envs.create_environment(env_json)


def describe(env_json):
    env = make(env_json)
    out = OrderedDict()
    out["env_json"] = OrderedDict(env_json)
    out["attrs"] = OrderedDict((k, plain(getattr(env, k))) for k in ATTRS)
    out["episode_steps_limit_default"] = plain(make(dict(env_json, EpisodeSteps=-1)).EPISODE_STEPS_LIMIT)
    out["reset"] = plain(env.reset())
    return env, out


def actions_1d():
    grid = np.linspace(-3.0, 3.0, 193).astype(np.float32)
    special = np.array([-2.0, 2.0, -1.0, 1.0, -0.6, 0.6, -0.8, 0.8, 0.0, -2.5, 2.5, 1e-3, -1e-3], np.float32)
    return np.unique(np.concatenate([grid, special])).astype(np.float64)


def trajectories_2d():
    f = np.float32
    rng = np.random.RandomState(20)
    return OrderedDict([
        ("into_upper_goal", np.tile(np.array([[1.0, 1.0]], f), (6, 1))),
        ("into_lower_goal", np.tile(np.array([[-1.0, -1.0]], f), (6, 1))),
        ("oblique_into_lower_goal", np.tile(np.array([[-0.7, -0.9]], f), (12, 1))),
        ("into_the_wall", np.tile(np.array([[0.9, -1.0]], f), (10, 1))),
        ("never_terminates", rng.uniform(-0.3, 0.3, (12, 2)).astype(f)),
    ])


def main():
    out = OrderedDict()
    out["source"] = "environments/environments.py:158-912 of the reference, run by tests/golden/make_bimodal_golden.py"
    out["envs"] = OrderedDict()
    for name in NAMES_1D:
        with open(os.path.join(REF, "jsonfiles", "environment", name + ".json")) as fh:
            env_json = json.load(fh, object_pairs_hook=OrderedDict)
        env, rec = describe(env_json)
        steps = []
        for a in actions_1d():
            env.reset()
            s2, r, done, _ = env.step(np.array([a]))
            steps.append([float(a), plain(s2), float(r), bool(done)])
        rec["steps"] = steps
        out["envs"][name] = rec
    with open(os.path.join(ROOT, "jsonfiles", "environment", "Bimodal2DEnv.json")) as fh:
        env_json = json.load(fh, object_pairs_hook=OrderedDict)
    env, rec = describe(env_json)
    rec["trajectories"] = OrderedDict()
    for tname, acts in trajectories_2d().items():
        env.reset()
        steps = []
        for a in acts.astype(np.float64):
            s2, r, done, _ = env.step(a)
            steps.append([plain(a), plain(s2), float(r), bool(done)])
            if done:
                break
        rec["trajectories"][tname] = steps
    out["envs"]["Bimodal2DEnv"] = rec
    path = os.path.join(HERE, "bimodal_envs.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
