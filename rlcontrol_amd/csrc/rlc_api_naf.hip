// rlc_api_naf.hip -- C ABI of the NAF population (declared in include/rlcontrol_hip.h).
#include "rlc_handle.h"

int rlc_h_naf_launch_update(rlc_handle* h, int first, int n, int n_updates, int source, const long long* idx_dev,
                            const RlcNafRollout* rollout) {
    if (rlc_h_variant(h) == 2) {
        return rlc_launch_naf_update_mfma(h->naf, first, n, n_updates, source, idx_dev, h->grad_taps, h->st, rollout);
    }
    return rlc_launch_naf_update(h->naf, first, n, n_updates, source, idx_dev, h->grad_taps, h->st, rollout);
}

// floats of one agent's acting output: mu [A], then the L columns [A(A+1)/2]
static size_t naf_lcols(const rlc_handle* h) { return (size_t)h->rep.A * (h->rep.A + 1) / 2; }

extern "C" {

int rlc_naf_create(const rlc_naf_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->l1_dim >= 1 && cfg->l2_dim >= 1, "layer widths must be >= 1");
    RLC_REQUIRE(cfg->action_dim <= RLC_NAF_MAX_A, "NAF supports action_dim <= %d (got %d)", RLC_NAF_MAX_A, cfg->action_dim);
    RLC_REQUIRE(cfg->state_min && cfg->state_max && cfg->action_max && cfg->learning_rate, "null array");
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE || cfg->norm_type == RLC_NORM_LAYER,
                "norm_type %d: 'batch' (fused batch norm with moving averages, base_network.py:57-59) is not implemented",
                cfg->norm_type);
    const int norm = cfg->norm_type == RLC_NORM_LAYER ? 1 : 0;
    RLC_REQUIRE(!norm || (cfg->l1_dim <= 1024 && cfg->l2_dim <= 1024), "layer norm: layer widths must be <= 1024");
    RlcCreate c(RLC_ALGO_NAF, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_naf_create", out);
    RlcNafDev& dv = c.h->naf;
    dv.d = rlc_naf_make_dims(cfg->state_dim, cfg->action_dim, cfg->l1_dim, cfg->l2_dim, cfg->batch_size, 0, norm);
    // the tile-blocked weight layout goes with the MFMA kernel (the default whenever it supports the shape)
    if (rlc_naf_mfma_supported(dv.d)) dv.d = rlc_with_layout(dv.d, 1);
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.tau = cfg->tau;
    const size_t NA = cfg->n_agents, S = dv.d.S, A = dv.d.A;
    c.blobs(dv);
    c.upload(&dv.lr, cfg->learning_rate, NA);
    c.upload(&dv.smin, cfg->state_min, S);
    c.upload(&dv.smax, cfg->state_max, S);
    c.upload(&dv.amax, cfg->action_max, A);
    std::vector<float> amin(A);          // default: a symmetric box
    for (size_t j = 0; j < A; j++) amin[j] = cfg->action_min ? cfg->action_min[j] : -cfg->action_max[j];
    c.upload(&dv.amin, amin.data(), A);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_y, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_V, NA * RLC_MAX_BATCH);
    dv.scratch_stride = (long long)((rlc_naf_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_naf_create", out);
}

int rlc_naf_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_NAF, out_p); }
int rlc_naf_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_NAF, agent, which, src, n);
}
int rlc_naf_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_NAF, agent, which, dst, n);
}
int rlc_naf_get_beta_powers(rlc_handle* h, int32_t agent, float* pw2) {
    return rlc_h_beta_powers(h, RLC_ALGO_NAF, agent, pw2, false);
}
int rlc_naf_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_NAF, agent); }

int rlc_naf_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, float* out_mu, float* out_lcols) {
    RLC_NEED(h, RLC_ALGO_NAF);
    const size_t mu_f = (size_t)n * h->rep.A, lc_f = n * naf_lcols(h);
    return rlc_h_act(h, RLC_ALGO_NAF, first_agent, n, states, nullptr, 0, mu_f + lc_f, false,
                     [&](const float* in, float* out) {
                         return rlc_launch_naf_act(h->naf, first_agent, n, in, out, out + mu_f, h->st);
                     },
                     out_mu, out_lcols, lc_f);
}

// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_naf_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states) {
    RLC_NEED(h, RLC_ALGO_NAF);
    const size_t mu_f = (size_t)n * h->rep.A, lc_f = n * naf_lcols(h);
    return rlc_h_act(h, RLC_ALGO_NAF, first_agent, n, states, nullptr, 0, mu_f + lc_f, true,
                     [&](const float* in, float* out) {
                         return rlc_launch_naf_act(h->naf, first_agent, n, in, out, out + mu_f, h->st, rlc_h_aq_flag(h),
                                                   h->aq_seq);
                     });
}

int rlc_naf_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_mu, float* out_lcols) {
    RLC_NEED(h, RLC_ALGO_NAF);
    const size_t lc_f = n * naf_lcols(h);
    return rlc_h_act_fetch(h, RLC_ALGO_NAF, first_agent, n, (size_t)n * h->rep.A + lc_f, out_mu, out_lcols, lc_f);
}

int rlc_naf_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices) {
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, RLC_ALGO_NAF, n_updates, host_indices, 0, false, &source, &idx);
    if (rc || n_updates == 0) return rc;
    return rlc_h_naf_launch_update(h, 0, h->naf.n_agents, n_updates, source, idx, nullptr);
}

int rlc_naf_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                         const double* next_states, const double* rewards, const double* gammas) {
    if (int rc = rlc_h_stage_batch(h, RLC_ALGO_NAF, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    return rlc_h_naf_launch_update(h, agent, 1, 1, RLC_SRC_STAGING, nullptr, nullptr);
}

int rlc_naf_set_kernel(rlc_handle* h, int32_t variant) {
    // 2 also takes the wide shapes (state_dim <= 32, action_dim in {1,2,3,4,6}), which 0 leaves on the any-shape kernel
    const char* why = h && h->algo == RLC_ALGO_NAF && variant == 2 ? rlc_naf_mfma_refusal(h->naf.d) : nullptr;
    return rlc_h_set_kernel(h, RLC_ALGO_NAF, variant,
                            why ? std::string("MFMA NAF kernel does not support these dimensions: ") + why : std::string());
}
int rlc_naf_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_NAF, variant_in_use); }
int rlc_naf_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_NAF, on); }
int rlc_naf_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_NAF, agent, which, dst, n);
}

}  // extern "C"
