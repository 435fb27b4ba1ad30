"""OptimalQ agent on MI355X (mirrors agents/OptimalQ.py:11-94 + agents/network/optimal_q_network.py).

``OptimalQ(config)`` is built from the Config of jsonfiles/agent/optimalq.json.  A Q-learner without an actor: the
greedy action is the row of a discretised action grid with the largest online Q, for training and evaluation alike
(OptimalQ.py:26-66), and the TD target takes the maximum of the target network over the same grid (OptimalQ.py:68-89).
The grid is built here, on the host, exactly as the reference builds it (hip_optq.action_grid) and uploaded once; the
search itself runs on the device.  Training adds the external exploration policy (ou_noise) when there is one.

Differences from the reference, both deliberate: every batch size the any-shape kernels take is accepted (the reference
raises ValueError("Invalid batch_size") for anything but 32 or 1, an artefact of its precomputed tiling,
optimal_q_network.py:134-139), and norm_type 'layer' / 'batch' are refused.
"""
import numpy as np

from .base_agent import BaseAgent
from .network.base_network_manager import BaseNetwork_Manager, check_norm_type
from ..hip_optq import MAX_NODES, OptQPopulation, action_grid, init_params


class OptimalQ_Network_Manager(BaseNetwork_Manager):
    queues_next_action = True        # update_from_replay(indices, next_state=...) queues the forward step() will fetch
    _queued_state = None

    def __init__(self, config):
        super(OptimalQ_Network_Manager, self).__init__(config)
        check_norm_type(config, "OptimalQ", ('none', 'input_norm'))
        self.rng = np.random.RandomState(config.random_seed)      # OptimalQ_Network_Manager.rng (OptimalQ.py:15)
        # optional json key "hip_kernel": "auto" or "generic" -- both the any-shape kernel, the only one this agent has
        kernel = getattr(config, "hip_kernel", "auto")
        if kernel not in ("auto", "generic"):
            raise ValueError("hip_kernel %r: OptimalQ runs on the any-shape kernel only (expected 'auto' or 'generic')" % (kernel,))
        # the first dimension's bounds for every dimension (optimal_q_network.py:166-169)
        n_axis = int(np.floor((float(np.reshape(config.action_max, -1)[0]) + 1e-10 - float(np.reshape(config.action_min, -1)[0]))
                              / float(config.discretization))) + 1
        if n_axis ** int(config.action_dim) > MAX_NODES:
            raise ValueError("OptimalQ: discretization %r gives about %d^%d grid nodes, above the %d the library takes" %
                             (config.discretization, n_axis, config.action_dim, MAX_NODES))
        self.action_grid = action_grid(config.action_min, config.action_max, config.discretization, config.action_dim)
        self.population = OptQPopulation(
            n_agents=1, state_dim=config.state_dim, action_dim=config.action_dim, l1_dim=config.l1_dim,
            l2_dim=config.l2_dim, batch_size=config.batch_size, buffer_size=int(config.buffer_size), tau=config.tau,
            state_min=config.state_min, state_max=config.state_max, learning_rate=config.learning_rate,
            seeds=[np.uint64(config.random_seed)], node_actions=self.action_grid,
            clip_state=(config.norm_type != 'none'), device=int(getattr(config, "device", 0)),
            norm_type=config.norm_type)
        self.population.set_kernel(kernel)
        # sess.run(global_variables_initializer()) + init_target_network() (OptimalQ.py:22-24)
        theta0 = init_params(config.state_dim, config.action_dim, config.l1_dim, config.l2_dim, config.random_seed)
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
        (experiment.py:132-135): its greedy grid search is queued behind the update -- one launch sequence, one
        synchronisation per environment step; the exploration noise is still added on the host after the fetch."""
        self._queued_state = None
        self.population.update(1, host_indices=logical_indices)
        if next_state is not None:
            self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1))
            self._queued_state = np.array(next_state, np.float64).reshape(-1)


class OptimalQ(BaseAgent):
    def __init__(self, config):
        network_manager = OptimalQ_Network_Manager(config)
        super(OptimalQ, self).__init__(config, network_manager)
