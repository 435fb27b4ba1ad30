// rlc_api_kl.hip -- C ABI of the ReverseKL / ForwardKL populations (declared in include/rlcontrol_hip.h).
// The two agents share SoftActorCritic's network family (a Gaussian policy, a Q and a V network with a V target), so
// the handle reuses the device view RlcSacDev (with the Q network's action rows at the INPUT layer: RlcSacDims::qcat)
// and the blob / act / update / tap bodies of rlc_api_sac.hip; what is particular to them -- the action-integral
// update kernel, torch's Adam bookkeeping, the quadrature nodes -- lives here and in kl_generic.hip.
#include <algorithm>

#include "rlc_handle.h"

extern "C" {

int rlc_kl_create(const rlc_kl_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->actor_l1_dim >= 1 && cfg->actor_l2_dim >= 1 && cfg->critic_l1_dim >= 1 && cfg->critic_l2_dim >= 1,
                "layer widths must be >= 1");
    RLC_REQUIRE(cfg->pi_lr && cfg->qf_vf_lr && cfg->entropy_scale, "null per-agent array");
    RLC_REQUIRE(cfg->kind == RLC_KL_REVERSE || cfg->kind == RLC_KL_FORWARD, "kind must be RLC_KL_REVERSE or RLC_KL_FORWARD");
    RLC_REQUIRE(cfg->optim_type >= RLC_KL_OPTIM_INTG && cfg->optim_type <= RLC_KL_OPTIM_HARD_LL, "unknown optim_type %d",
                cfg->optim_type);
    // forwardkl_network.py:153-158: 'll' raises NotImplementedError, the other names are never matched
    RLC_REQUIRE(cfg->kind == RLC_KL_REVERSE || cfg->optim_type == RLC_KL_OPTIM_INTG,
                "ForwardKL implements optim_type 'intg' only");
    RLC_REQUIRE(cfg->q_update_type == RLC_KL_Q_NON_SAC || cfg->q_update_type == RLC_KL_Q_SAC, "unknown q_update_type %d",
                cfg->q_update_type);
    RLC_REQUIRE(cfg->action_dim >= 1 && cfg->action_dim <= 6, "action_dim %d outside [1,6]", cfg->action_dim);
    const bool integral = cfg->optim_type == RLC_KL_OPTIM_INTG || cfg->optim_type == RLC_KL_OPTIM_HARD_INTG;
    RLC_REQUIRE(!integral || (cfg->n_nodes >= 1 && cfg->node_actions && cfg->node_weights),
                "the integral updates need n_nodes >= 1 quadrature nodes and weights");
    RLC_REQUIRE(cfg->n_nodes >= 0 && cfg->n_nodes <= 4096, "n_nodes %d outside [0,4096]", cfg->n_nodes);
    RLC_REQUIRE(cfg->action_max0 > 0.0f, "action_max0 must be positive");
    for (int i = 0; i < cfg->n_agents; i++)
        RLC_REQUIRE(cfg->kind == RLC_KL_REVERSE || cfg->entropy_scale[i] > 0.0f,
                    "agent %d: ForwardKL divides Q by entropy_scale, which must be positive", i);
    if (integral)   // atanh of the normalised node must be finite (the reference cuts the end points for this reason)
        for (int k = 0; k < cfg->n_nodes * cfg->action_dim; k++)
            RLC_REQUIRE(cfg->node_actions[k] > -cfg->action_max0 && cfg->node_actions[k] < cfg->action_max0,
                        "node %d component %d (%g) is not strictly inside (-action_max, action_max)", k / cfg->action_dim,
                        k % cfg->action_dim, (double)cfg->node_actions[k]);
    RlcCreate c(RLC_ALGO_KL, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_kl_create", out);
    RlcSacDev& dv = c.h->sac;
    dv.kl_nodes = integral ? cfg->n_nodes : 0;
    dv.d = rlc_sac_make_dims(cfg->state_dim, cfg->action_dim, cfg->actor_l1_dim, cfg->actor_l2_dim, cfg->critic_l1_dim,
                             cfg->critic_l2_dim, cfg->batch_size, 0, 1);
    // the tile-blocked weight layout goes with the MFMA kernel: the default whenever it supports the shape at
    // action_dim 1; above that it is chosen by rlc_kl_set_kernel only, and a new population runs the any-shape kernel
    if (cfg->action_dim == 1 && rlc_kl_mfma_supported(dv.d, dv.kl_nodes)) dv.d = rlc_with_layout(dv.d, 1);
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = 0;   // the networks never apply the input normaliser they are handed (reversekl_network.py:43)
    dv.tau = cfg->tau;
    dv.smin0 = dv.smax0 = 0.0f;
    dv.amax0 = cfg->action_max0;
    dv.kl_kind = cfg->kind; dv.kl_optim = cfg->optim_type; dv.kl_qupdate = cfg->q_update_type;
    const size_t NA = cfg->n_agents, K = dv.kl_nodes;
    c.blobs(dv, false);                  // torch's Adam keeps the step count, not the beta powers
    c.alloc(&dv.kl_step, NA);
    c.upload(&dv.pi_lr, cfg->pi_lr, NA);
    c.upload(&dv.qv_lr, cfg->qf_vf_lr, NA);
    c.upload(&dv.alpha, cfg->entropy_scale, NA);
    c.upload(&dv.kl_node_a, cfg->node_actions, K * (size_t)cfg->action_dim);
    c.upload(&dv.kl_node_w, cfg->node_weights, K);
    c.alloc(&dv.noise_ctr, NA);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_v, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_logp, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_qpi, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_loss, NA * 4);
    c.alloc(&dv.kl_tap_iq, NA * (size_t)cfg->batch_size * K);
    size_t need = rlc_kl_scratch_floats(dv.d, dv.kl_nodes);
    if (rlc_kl_mfma_supported(dv.d, dv.kl_nodes)) need = std::max(need, rlc_kl_mfma_scratch_floats(dv.d, dv.kl_nodes));
    dv.scratch_stride = (long long)((need + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_kl_create", out);
}

int rlc_kl_set_step(rlc_handle* h, int32_t agent, int32_t step) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_KL);
    RLC_REQUIRE(step >= 0, "negative step");
    RLC_HIP(hipMemcpyAsync(h->sac.kl_step + agent, &step, sizeof(int), hipMemcpyHostToDevice, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    return 0;
}

int rlc_kl_get_step(rlc_handle* h, int32_t agent, int32_t* step) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_KL);
    RLC_REQUIRE(step, "null step");
    RLC_HIP(hipMemcpyAsync(step, h->sac.kl_step + agent, sizeof(int), hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    return 0;
}

int rlc_kl_set_kernel(rlc_handle* h, int32_t variant) {
    const char* why = h && h->algo == RLC_ALGO_KL && variant == 2 ? rlc_kl_mfma_refusal(h->sac.d, h->sac.kl_nodes) : nullptr;
    if (int rc = rlc_h_set_kernel(h, RLC_ALGO_KL, variant,
                                  why ? std::string("MFMA KL kernel does not support these dimensions: ") + why : "", false))
        return rc;
    if (rlc_h_variant(h) != 2) h->split_c = 1;        // latency mode belongs to the MFMA kernel
    return 0;
}

int rlc_kl_set_split(rlc_handle* h, int32_t n_workgroups) {
    if (int rc = rlc_h_split_check(h, RLC_ALGO_KL, n_workgroups)) return rc;
    if (n_workgroups == 1) return 0;
    RLC_REQUIRE(rlc_h_variant(h) == 2, "latency mode is a variant of the MFMA kernel (these dimensions run the any-shape one)");
    RLC_REQUIRE(h->sac.d.A == 1, "latency mode of the KL agents is built for action_dim 1 (got %d)", h->sac.d.A);
    RLC_REQUIRE(h->sac.kl_optim == RLC_KL_OPTIM_INTG || h->sac.kl_optim == RLC_KL_OPTIM_HARD_INTG,
                "latency mode splits the action integral; the 'll' updates have none");
    // the partial-integral buffer does not depend on the workgroup count: allocated with the barrier words, once
    return rlc_h_split_arm(h, n_workgroups, rlc_kl_split_grid(h->sac.n_agents, n_workgroups),
                           h->split_bar ? 0 : (size_t)h->sac.n_agents * rlc_kl_split_zbuf_floats(h->sac.d));
}

int rlc_kl_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_KL, variant_in_use); }
int rlc_kl_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_KL, out_p); }
int rlc_kl_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_KL, agent, which, src, n);
}
int rlc_kl_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_KL, agent, which, dst, n);
}
int rlc_kl_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_KL, agent); }
int rlc_kl_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* eps,
               float* out_actions) {
    return rlc_sacfam_act(RLC_ALGO_KL, h, first_agent, n, states, sample, eps, false, out_actions);
}
int rlc_kl_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* eps) {
    return rlc_sacfam_act(RLC_ALGO_KL, h, first_agent, n, states, sample, eps, true, nullptr);
}
int rlc_kl_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_actions) {
    RLC_NEED(h, RLC_ALGO_KL);
    return rlc_h_act_fetch(h, RLC_ALGO_KL, first_agent, n, (size_t)n * h->rep.A, out_actions);
}
int rlc_kl_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices, const float* eps) {
    return rlc_sacfam_update(RLC_ALGO_KL, h, n_updates, host_indices, eps);
}
int rlc_kl_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                        const double* next_states, const double* rewards, const double* gammas, const float* eps) {
    return rlc_sacfam_update_batch(RLC_ALGO_KL, h, agent, batch, states, actions, next_states, rewards, gammas, eps);
}
int rlc_kl_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_KL, on); }
int rlc_kl_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_KL, agent, which, dst, n);
}

}  // extern "C"
