"""ActorExpert agent on MI355X (mirrors agents/ActorExpert.py:13-192 + agents/network/ae_network.py).

``ActorExpert(config)`` is built from the Config of jsonfiles/agent/ae.json.  A hydra network: a shared first layer, a
mixture-density actor (``num_modal`` Gaussians) and an expert Q(s, a).  The expert learns by Q-learning with the mean of
the actor's largest-alpha mode as the next action; the actor is fitted to the ``int(num_samples * rho)`` best of
``num_samples`` of its own actions per state, ranked by the expert (ActorExpert.py:116-185).

Random draws come from ``numpy.random.RandomState(random_seed)`` on the host, in the order the reference's network draws
them (ae_network.py:461-496): per call, one uniform per sample and row for the mode (``RandomState.choice`` consumes
exactly these), then the standard normals of every row.  They reach the kernel as float32.

Quirks of the reference that are mirrored: ``sarsa_update`` is read and has no effect (ActorExpert.py:39-42 sets a
misspelt attribute, so the Q-learning branch always runs); the weights_regularizers never enter a loss.

Not carried over, refused by name: ``use_true_q``, ``use_better_q_gd``, ``use_uniform_sampling`` set to "True";
norm_type 'layer' / 'batch'; hip_kernel "mfma".  write_plot's plots are not drawn.
"""
import numpy as np

from .base_agent import BaseAgent
from .network.base_network_manager import BaseNetwork_Manager, check_norm_type
from ..hip_ae import AEPopulation, init_params, top_k


class ActorExpert_Network_Manager(BaseNetwork_Manager):
    queues_next_action = True        # update_from_replay(indices, next_state=...) queues the forward step() will fetch
    _queued_state = None
    _queued_sample = False

    def __init__(self, config):
        super(ActorExpert_Network_Manager, self).__init__(config)
        check_norm_type(config, "ActorExpert", ('none', 'input_norm'))
        for key in ("use_true_q", "use_better_q_gd", "use_uniform_sampling"):
            if getattr(config, key, "False") == "True":
                raise NotImplementedError("ActorExpert: %s = \"True\" is not implemented in the HIP path" % key)
        # optional json key "hip_kernel": "auto" or "generic" -- both the any-shape kernel, the only one this agent has
        kernel = getattr(config, "hip_kernel", "auto")
        if kernel not in ("auto", "generic"):
            raise ValueError("hip_kernel %r: ActorExpert runs on the any-shape kernel only (expected 'auto' or 'generic')" % (kernel,))
        getattr(config, "sarsa_update", None)        # accepted and ignored, as in the reference (see the module docstring)
        self.rng = np.random.RandomState(config.random_seed)
        self.sample_for_eval = getattr(config, "sample_for_eval", "False") == "True"
        self.num_samples, self.num_modal = int(config.num_samples), int(config.num_modal)
        self.top_k = top_k(config.num_samples, config.rho)
        self.dims = (config.state_dim, config.action_dim, config.shared_l1_dim, config.actor_l2_dim, config.expert_l2_dim,
                     self.num_modal)
        self.population = AEPopulation(
            n_agents=1, state_dim=config.state_dim, action_dim=config.action_dim, shared_l1_dim=config.shared_l1_dim,
            actor_l2_dim=config.actor_l2_dim, expert_l2_dim=config.expert_l2_dim, num_modal=self.num_modal,
            num_samples=self.num_samples, top_k=self.top_k, batch_size=config.batch_size,
            buffer_size=int(config.buffer_size), tau=config.tau, state_min=config.state_min, state_max=config.state_max,
            action_min=config.action_min, action_max=config.action_max, actor_lr=config.actor_lr,
            expert_lr=config.expert_lr, seeds=[np.uint64(config.random_seed)], clip_state=(config.norm_type != 'none'),
            device=int(getattr(config, "device", 0)), norm_type=config.norm_type)
        self.population.set_kernel(kernel)
        # sess.run(global_variables_initializer()) + init_target_network() (ActorExpert.py:31-33)
        self.population.set_params(0, init_params(*self.dims, seed=config.random_seed), init_target=True)

    def device_replay(self):
        return (self.population, 0)

    def _draws(self, rows, n):
        """the draws of sample_action for `rows` states and n samples each: every row's uniforms, then every row's
        normals (ae_network.py:485-488)"""
        u = self.rng.random_sample((rows, n)).astype(np.float32)
        eps = self.rng.standard_normal((rows, n, self.action_dim)).astype(np.float32)
        return u, eps

    # ---- the next action, queued behind the update (one synchronisation per environment step) ----
    def _drop_queued(self):
        if self._queued_state is not None:
            if self._queued_sample:
                self.rng.set_state(self._queued_rng)
            self._queued_state = None

    def _act(self, state, sample):
        """the forward for this very state may already be queued behind the last update (update_from_replay below); a
        queued sample has consumed the draws take_action would have made -- the stream is put back when it is dropped"""
        queued, self._queued_state = self._queued_state, None
        s = np.asarray(state, np.float64).reshape(-1)
        if queued is not None:
            if self._queued_sample == bool(sample) and np.array_equal(queued, s):
                return self.population.act_fetch(1)[0]
            if self._queued_sample:
                self.rng.set_state(self._queued_rng)
        if not sample:
            return self.population.act(s.reshape(1, -1))[0]
        u, eps = self._draws(1, 1)
        return self.population.act(s.reshape(1, -1), sample=True, u=u, eps=eps)[0]

    def take_action(self, state, is_train, is_start):
        if is_train:
            if is_start:
                self.train_ep_count += 1
            self.train_global_steps += 1
            if self.use_external_exploration:
                return self.exploration_policy.generate(self._act(state, False), self.train_global_steps)
            return self._act(state, True)
        if is_start:
            self.eval_ep_count += 1
        self.eval_global_steps += 1
        return self._act(state, self.sample_for_eval)

    def update_network(self, state, action, next_state, reward, gamma):
        self._drop_queued()
        u, eps = self._draws(len(np.reshape(reward, -1)), self.num_samples)
        self.population.update_batch(0, state, action, next_state, reward, gamma, u=u, eps=eps)

    def update_from_replay(self, logical_indices, next_state=None):
        """One fused update on the device replay.  `next_state`: the observation Experiment asks an action for next
        (experiment.py:132-135): its forward -- a sample, or the greedy action the host adds its noise to -- is queued
        behind the update: one launch sequence, one synchronisation per environment step."""
        self._drop_queued()
        u, eps = self._draws(len(logical_indices), self.num_samples)
        self.population.update(1, host_indices=logical_indices, u=u, eps=eps)
        if next_state is not None:
            sample = not self.use_external_exploration
            if sample:
                self._queued_rng = self.rng.get_state()
                qu, qeps = self._draws(1, 1)
                self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1), sample=True, u=qu, eps=qeps)
            else:
                self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1))
            self._queued_sample = sample
            self._queued_state = np.array(next_state, np.float64).reshape(-1)


class ActorExpert(BaseAgent):
    def __init__(self, config):
        network_manager = ActorExpert_Network_Manager(config)
        super(ActorExpert, self).__init__(config, network_manager)
