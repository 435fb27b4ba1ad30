"""ActorCritic agent on MI355X (mirrors agents/ActorCritic.py:12-270 + agents/network/ac_network.py).

``ActorCritic(config)`` is built from the Config of jsonfiles/agent/ac.json.  A hydra network: a shared first layer, a
one-mode Gaussian actor in pre-tanh space (mu linear, sigma = exp(-20 + 11 (tanh + 1)), action = tanh(raw) * action_max)
and a critic Q(s, a).  The critic learns by a TD step whose next action comes from the online actor (``critic_update``:
``mean`` the greedy action, ``sampled`` one draw, ``expected`` the target Q averaged over ``num_samples`` draws); the actor
by a likelihood-ratio or cross-entropy step on ``num_samples`` of its own raw samples per state (``actor_update``:
``ll`` sample 0 weighted by q_0 - mean q, ``ll_update_all`` every sample by q_j - mean q, ``cem`` the
``int(num_samples * rho)`` best by Q with weight 1) -- ActorCritic.py:116-263.

Random draws come from ``numpy.random.RandomState(random_seed).standard_normal`` on the host and reach the kernel as
float32, in this order: per update ``eps_next`` [batch][n_next][A] (n_next = 0, 1 or num_samples for mean, sampled,
expected; nothing is drawn for 0), then ``eps`` [batch][num_samples][A]; per sampled action one ``[1][1][A]``.

Where the reference cannot run as written, this port does the following:
 * ac.json sweeps ``num_modal: [2]`` against the network's ``assert num_modal == 1`` (ac_network.py:175): the shipped
   json here carries ``[1]``, and the agent refuses any other value;
 * ac.json lacks ``use_true_q`` and ``add_entropy``, which the constructor reads (ActorCritic.py:39-47): both are read
   with the default "False"; the shipped json appends them as single-valued keys at the end (the sweep stays at 18
   settings in the reference's index order);
 * the samples come from TF's random ops (``mvn.sample``, ac_network.py:221): here they are the host's standard normals
   above, or the device's Philox stream at the C ABI.
Parity unpinned: no reference fixture exercises this agent.

With ``exploration_policy: ou_noise`` the host's OU noise is added to the greedy action (ActorCritic.py:58-59).
``equal_modal_selection`` is read and ignored (the reference marks it "Not being used", ac_network.py:38-41).  The alpha
head is carried in the parameters and never trained (no loss reaches it).

Not carried over, refused by name: ``critic_update: random_q``; ``actor_update: reparam``; ``use_true_q`` or
``add_entropy`` set to "True"; ``num_modal`` != 1; norm_type 'layer' / 'batch'; hip_kernel "mfma".  write_plot's plots
are not drawn.
"""
import numpy as np

from .base_agent import BaseAgent
from .network.base_network_manager import BaseNetwork_Manager, check_norm_type
from ..hip_ac import ACTOR_UPDATES, CRITIC_UPDATES, ACPopulation, init_params, next_draws, top_k


class ActorCritic_Network_Manager(BaseNetwork_Manager):
    queues_next_action = True        # update_from_replay(indices, next_state=...) queues the forward step() will fetch
    _queued_state = None
    _queued_sample = False

    def __init__(self, config):
        super(ActorCritic_Network_Manager, self).__init__(config)
        check_norm_type(config, "ActorCritic", ('none', 'input_norm'))
        for key in ("use_true_q", "add_entropy"):
            if getattr(config, key, "False") == "True":
                raise NotImplementedError("ActorCritic: %s = \"True\" is not implemented in the HIP path" % key)
        if int(config.num_modal) != 1:
            raise ValueError("ActorCritic: num_modal must be 1 (got %r): the network is unimodal, the reference asserts it "
                             "(ac_network.py:175)" % (config.num_modal,))
        if config.critic_update not in CRITIC_UPDATES:
            raise NotImplementedError("ActorCritic: critic_update %r is not implemented in the HIP path (expected one of %s)"
                                      % (config.critic_update, ", ".join(sorted(CRITIC_UPDATES))))
        if config.actor_update not in ACTOR_UPDATES:
            raise NotImplementedError("ActorCritic: actor_update %r is not implemented in the HIP path (expected one of %s)"
                                      % (config.actor_update, ", ".join(sorted(ACTOR_UPDATES))))
        # optional json key "hip_kernel": "auto" or "generic" -- both the any-shape kernel, the only one this agent has
        kernel = getattr(config, "hip_kernel", "auto")
        if kernel not in ("auto", "generic"):
            raise ValueError("hip_kernel %r: ActorCritic runs on the any-shape kernel only (expected 'auto' or 'generic')" % (kernel,))
        getattr(config, "equal_modal_selection", None)     # accepted and ignored, as in the reference
        self.rng = np.random.RandomState(config.random_seed)
        self.sample_for_eval = getattr(config, "sample_for_eval", "False") == "True"
        self.num_samples = int(config.num_samples)
        self.critic_update, self.actor_update = config.critic_update, config.actor_update
        self.n_next = next_draws(self.critic_update, self.num_samples)
        self.top_k = top_k(config.num_samples, config.rho)
        self.dims = (config.state_dim, config.action_dim, config.shared_l1_dim, config.actor_l2_dim, config.critic_l2_dim)
        self.population = ACPopulation(
            n_agents=1, state_dim=config.state_dim, action_dim=config.action_dim, shared_l1_dim=config.shared_l1_dim,
            actor_l2_dim=config.actor_l2_dim, critic_l2_dim=config.critic_l2_dim, num_samples=self.num_samples,
            top_k=self.top_k, batch_size=config.batch_size, buffer_size=int(config.buffer_size), tau=config.tau,
            state_min=config.state_min, state_max=config.state_max, action_max=config.action_max,
            actor_lr=config.actor_lr, critic_lr=config.critic_lr, seeds=[np.uint64(config.random_seed)],
            critic_update=self.critic_update, actor_update=self.actor_update, clip_state=(config.norm_type != 'none'),
            device=int(getattr(config, "device", 0)), norm_type=config.norm_type)
        self.population.set_kernel(kernel)
        # sess.run(global_variables_initializer()) + init_target_network() (ActorCritic.py:31-33)
        self.population.set_params(0, init_params(*self.dims, seed=config.random_seed), init_target=True)

    def device_replay(self):
        return (self.population, 0)

    def _update_draws(self, rows):
        """the draws of one update for `rows` states: eps_next (None when critic_update is 'mean'), then eps"""
        eps_next = None
        if self.n_next:
            eps_next = self.rng.standard_normal((rows, self.n_next, self.action_dim)).astype(np.float32)
        return eps_next, self.rng.standard_normal((rows, self.num_samples, self.action_dim)).astype(np.float32)

    def _act_draw(self):
        return self.rng.standard_normal((1, 1, self.action_dim)).astype(np.float32)

    # ---- the next action, queued behind the update (one synchronisation per environment step) ----
    def _drop_queued(self):
        if self._queued_state is not None:
            if self._queued_sample:
                self.rng.set_state(self._queued_rng)
            self._queued_state = None

    def _act(self, state, sample):
        """the forward for this very state may already be queued behind the last update (update_from_replay below); a
        queued sample has consumed the draw take_action would have made -- the stream is put back when it is dropped"""
        queued, self._queued_state = self._queued_state, None
        s = np.asarray(state, np.float64).reshape(-1)
        if queued is not None:
            if self._queued_sample == bool(sample) and np.array_equal(queued, s):
                return self.population.act_fetch(1)[0]
            if self._queued_sample:
                self.rng.set_state(self._queued_rng)
        if not sample:
            return self.population.act(s.reshape(1, -1))[0]
        return self.population.act(s.reshape(1, -1), sample=True, eps=self._act_draw())[0]

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
        eps_next, eps = self._update_draws(len(np.reshape(reward, -1)))
        self.population.update_batch(0, state, action, next_state, reward, gamma, eps_next=eps_next, eps=eps)

    def update_from_replay(self, logical_indices, next_state=None):
        """One fused update on the device replay.  `next_state`: the observation Experiment asks an action for next
        (experiment.py:132-135): its forward -- a sample, or the greedy action the host adds its noise to -- is queued
        behind the update: one launch sequence, one synchronisation per environment step."""
        self._drop_queued()
        eps_next, eps = self._update_draws(len(logical_indices))
        self.population.update(1, host_indices=logical_indices, eps_next=eps_next, eps=eps)
        if next_state is not None:
            sample = not self.use_external_exploration
            if sample:
                self._queued_rng = self.rng.get_state()
                self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1), sample=True, eps=self._act_draw())
            else:
                self.population.act_queue(np.asarray(next_state, np.float64).reshape(1, -1))
            self._queued_sample = sample
            self._queued_state = np.array(next_state, np.float64).reshape(-1)


class ActorCritic(BaseAgent):
    def __init__(self, config):
        network_manager = ActorCritic_Network_Manager(config)
        super(ActorCritic, self).__init__(config, network_manager)
