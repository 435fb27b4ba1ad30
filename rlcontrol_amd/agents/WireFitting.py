"""WireFitting agent on MI355X (mirrors agents/WireFitting.py:11-83 + agents/network/wf_network.py).

``WireFitting(config)`` is built from the Config of jsonfiles/agent/wirefitting.json.  One network puts out
``app_points`` wires -- an action and a value each -- and Q(s, a) interpolates the wire values by inverse distance
(wf_network.py:106-125).  The greedy action is the action of the wire with the largest value, for training and
evaluation alike (WireFitting.py:23-64); training adds the external exploration policy (ou_noise) on the host.  The TD
target takes the target network's largest wire value (WireFitting.py:66-77).

Not carried over: write_plot's Q-function plots (WireFitting.py:42-50), predict_q_target (unused and unverified in the
reference, wf_network.py:145-151), and norm_type 'layer' / 'batch', which are refused.
"""
import numpy as np

from .base_agent import BaseAgent
from .network.base_network_manager import BaseNetwork_Manager, check_norm_type
from ..hip_wf import WFPopulation, init_params


class WireFitting_Network_Manager(BaseNetwork_Manager):
    queues_next_action = True        # update_from_replay(indices, next_state=...) queues the forward step() will fetch
    _queued_state = None

    def __init__(self, config):
        super(WireFitting_Network_Manager, self).__init__(config)
        check_norm_type(config, "WireFitting", ('none', 'input_norm'))
        # optional json key "hip_kernel": "auto" or "generic" -- both the any-shape kernel, the only one this agent has
        kernel = getattr(config, "hip_kernel", "auto")
        if kernel not in ("auto", "generic"):
            raise ValueError("hip_kernel %r: WireFitting runs on the any-shape kernel only (expected 'auto' or 'generic')" % (kernel,))
        self.app_points = int(config.app_points)
        self.population = WFPopulation(
            n_agents=1, state_dim=config.state_dim, action_dim=config.action_dim, l1_dim=config.l1_dim,
            l2_dim=config.l2_dim, app_points=self.app_points, batch_size=config.batch_size,
            buffer_size=int(config.buffer_size), tau=config.tau, state_min=config.state_min, state_max=config.state_max,
            action_max0=float(np.reshape(config.action_max, -1)[0]),      # the scalar of wf_network.py:88
            learning_rate=config.learning_rate, seeds=[np.uint64(config.random_seed)],
            clip_state=(config.norm_type != 'none'), device=int(getattr(config, "device", 0)),
            norm_type=config.norm_type)
        self.population.set_kernel(kernel)
        # sess.run(global_variables_initializer()) + init_target_network() (WireFitting.py:19-20)
        theta0 = init_params(config.state_dim, config.action_dim, config.l1_dim, config.l2_dim, self.app_points,
                             config.random_seed)
        self.population.set_params(0, theta0, init_target=True)

    def device_replay(self):
        return (self.population, 0)

    def _greedy(self, state):
        # the forward for this very state may already be queued behind the last update (update_from_replay below)
        queued, self._queued_state = self._queued_state, None
        if queued is not None and np.array_equal(queued, np.asarray(state, np.float64).reshape(-1)):
            return self.population.act_fetch(1)[0]
        return self.population.act(np.asarray(state, np.float64).reshape(1, -1))[0]

    def take_action(self, state, is_train, is_start):
        greedy_action = self._greedy(state)
        if is_train:
            if is_start:
                self.train_ep_count += 1
            self.train_global_steps += 1
            if self.use_external_exploration:
                return self.exploration_policy.generate(greedy_action, self.train_global_steps)
            return greedy_action
        if is_start:
            self.eval_ep_count += 1
        self.eval_global_steps += 1
        return greedy_action

    def update_network(self, state, action, next_state, reward, gamma):
        self._queued_state = None
        self.population.update_batch(0, state, action, next_state, reward, gamma)

    def update_from_replay(self, logical_indices, next_state=None):
        """One fused update on the device replay.  `next_state`: the observation Experiment asks an action for next
        (experiment.py:132-135): its forward is queued behind the update -- one launch sequence, one synchronisation per
        environment step; the exploration noise is still added on the host after the fetch."""
        self._queued_state = None
        self.population.update(1, host_indices=logical_indices)
        if next_state is not None:
            self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1))
            self._queued_state = np.array(next_state, np.float64).reshape(-1)


class WireFitting(BaseAgent):
    def __init__(self, config):
        network_manager = WireFitting_Network_Manager(config)
        super(WireFitting, self).__init__(config, network_manager)
