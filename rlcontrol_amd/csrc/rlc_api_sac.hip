// rlc_api_sac.hip -- C ABI of the SoftActorCritic population (declared in include/rlcontrol_hip.h), and the bodies it
// shares with the ReverseKL / ForwardKL populations (rlc_api_kl.hip), which use the same device view RlcSacDev.
#include "rlc_handle.h"

namespace {

// host eps [count] -> device buffer behind the index upload area; returns device pointer (or null if eps null)
int upload_eps(rlc_handle* h, const float* eps, size_t count, const float** out_dev, size_t idx_count) {
    *out_dev = nullptr;
    if (!eps) return 0;
    // layout of idx_dev: [idx_count long long][count floats]
    const size_t need_ll = idx_count + (count * sizeof(float) + 7) / 8;
    if (rlc_h_ensure_idx(h, need_ll)) return 1;
    float* dst = (float*)(h->idx_dev + idx_count);
    RLC_HIP(hipMemcpyAsync(dst, eps, sizeof(float) * count, hipMemcpyHostToDevice, h->st));
    *out_dev = dst;
    return 0;
}

}  // namespace

int rlc_h_sac_launch_update(rlc_handle* h, int first, int n, int n_updates, int source, const long long* idx_dev,
                            const float* eps_dev, const RlcSacRollout* rollout) {
    if (h->algo == RLC_ALGO_KL) {
        if (rlc_h_variant(h) == 2 && h->split_c > 1 && !rollout) {
            if (rlc_h_split_before_launch(h)) return 1;
            if (rlc_launch_kl_update_mfma_split(h->sac, h->split_part, h->split_bar, h->split_err, h->split_c, first, n,
                                                n_updates, source, idx_dev, eps_dev, h->grad_taps, h->st))
                return 1;
            return rlc_h_split_after_launch(h);
        }
        if (rlc_h_variant(h) == 2)
            return rlc_launch_kl_update_mfma(h->sac, first, n, n_updates, source, idx_dev, eps_dev, h->grad_taps, h->st,
                                             rollout);
        return rlc_launch_kl_update(h->sac, first, n, n_updates, source, idx_dev, eps_dev, h->grad_taps, h->st, rollout);
    }
    if (rlc_h_variant(h) == 2) {
        return rlc_launch_sac_update_mfma(h->sac, first, n, n_updates, source, idx_dev, eps_dev, h->grad_taps, h->st, rollout);
    }
    return rlc_launch_sac_update(h->sac, first, n, n_updates, source, idx_dev, eps_dev, h->grad_taps, h->st, rollout);
}

// ---- bodies of the rlc_sac_* and rlc_kl_* entry points that take eps; algo = RLC_ALGO_SAC or RLC_ALGO_KL ----
int rlc_sacfam_act(int algo, rlc_handle* h, int first_agent, int n, const double* states, int sample, const float* eps,
                   bool queued, float* out_actions) {
    RLC_NEED(h, algo);
    const size_t out_f = (size_t)n * h->rep.A, eps_f = (sample && eps) ? out_f : 0;
    return rlc_h_act(h, algo, first_agent, n, states, eps, eps_f, out_f, queued,
                     [&](const float* in, float* out) {
                         return (algo == RLC_ALGO_KL ? rlc_launch_kl_act : rlc_launch_sac_act)(
                             h->sac, first_agent, n, in, eps_f ? out - eps_f : nullptr, sample ? 1 : 0, out, h->st,
                             queued ? rlc_h_aq_flag(h) : nullptr, queued ? h->aq_seq : 0);
                     },
                     out_actions);
}

int rlc_sacfam_update(int algo, rlc_handle* h, int n_updates, const int64_t* host_indices, const float* eps) {
    RLC_NEED(h, algo);
    const size_t count = (size_t)h->rep.n_agents * (n_updates > 0 ? n_updates : 0) * h->B, A = h->rep.A;
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, algo, n_updates, host_indices, eps ? (count * A * sizeof(float) + 7) / 8 : 0, false,
                                      &source, &idx);
    if (rc || n_updates == 0) return rc;
    const float* eps_dev = nullptr;
    if (upload_eps(h, eps, count * A, &eps_dev, host_indices ? count : 0)) return 1;
    return rlc_h_sac_launch_update(h, 0, h->rep.n_agents, n_updates, source, h->idx_dev, eps_dev, nullptr);
}

int rlc_sacfam_update_batch(int algo, rlc_handle* h, int agent, int batch, const double* states, const double* actions,
                            const double* next_states, const double* rewards, const double* gammas, const float* eps) {
    if (int rc = rlc_h_stage_batch(h, algo, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    const float* eps_dev = nullptr;
    if (upload_eps(h, eps, (size_t)batch * h->rep.A, &eps_dev, 0)) return 1;
    return rlc_h_sac_launch_update(h, agent, 1, 1, RLC_SRC_STAGING, nullptr, eps_dev, nullptr);
}

extern "C" {

int rlc_sac_create(const rlc_sac_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->actor_l1_dim >= 1 && cfg->actor_l2_dim >= 1 && cfg->critic_l1_dim >= 1 && cfg->critic_l2_dim >= 1,
                "layer widths must be >= 1");
    RLC_REQUIRE(cfg->pi_lr && cfg->qf_vf_lr && cfg->entropy_scale, "null per-agent array");
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE || cfg->norm_type == RLC_NORM_LAYER,
                "norm_type %d: 'batch' (fused batch norm with moving averages, base_network.py:57-59) is not implemented",
                cfg->norm_type);
    const int norm = cfg->norm_type == RLC_NORM_LAYER ? 1 : 0;
    RLC_REQUIRE(!norm || (cfg->actor_l1_dim <= 1024 && cfg->actor_l2_dim <= 1024 && cfg->critic_l1_dim <= 1024 &&
                          cfg->critic_l2_dim <= 1024), "layer norm: layer widths must be <= 1024");
    RlcCreate c(RLC_ALGO_SAC, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_sac_create", out);
    RlcSacDev& dv = c.h->sac;
    dv.d = rlc_sac_make_dims(cfg->state_dim, cfg->action_dim, cfg->actor_l1_dim, cfg->actor_l2_dim,
                             cfg->critic_l1_dim, cfg->critic_l2_dim, cfg->batch_size, 0, 0, norm);
    // the tile-blocked weight layout goes with the MFMA kernel (the default whenever it supports the shape)
    if (rlc_sac_mfma_supported(dv.d)) dv.d = rlc_with_layout(dv.d, 1);
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.tau = cfg->tau;
    dv.smin0 = cfg->state_min0; dv.smax0 = cfg->state_max0; dv.amax0 = cfg->action_max0;
    const size_t NA = cfg->n_agents;
    c.blobs(dv);
    c.upload(&dv.pi_lr, cfg->pi_lr, NA);
    c.upload(&dv.qv_lr, cfg->qf_vf_lr, NA);
    c.upload(&dv.alpha, cfg->entropy_scale, NA);
    c.alloc(&dv.noise_ctr, NA);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_v, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_logp, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_qpi, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_loss, NA * 4);
    dv.scratch_stride = (long long)((rlc_sac_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_sac_create", out);
}

int rlc_sac_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_SAC, out_p); }
int rlc_sac_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_SAC, agent, which, src, n);
}
int rlc_sac_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_SAC, agent, which, dst, n);
}
int rlc_sac_set_beta_powers(rlc_handle* h, int32_t agent, const float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_SAC, agent, const_cast<float*>(pw4), true);
}
int rlc_sac_get_beta_powers(rlc_handle* h, int32_t agent, float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_SAC, agent, pw4, false);
}
int rlc_sac_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_SAC, agent); }
int rlc_sac_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* eps,
                float* out_actions) {
    return rlc_sacfam_act(RLC_ALGO_SAC, h, first_agent, n, states, sample, eps, false, out_actions);
}
// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_sac_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* eps) {
    return rlc_sacfam_act(RLC_ALGO_SAC, h, first_agent, n, states, sample, eps, true, nullptr);
}
int rlc_sac_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_actions) {
    RLC_NEED(h, RLC_ALGO_SAC);
    return rlc_h_act_fetch(h, RLC_ALGO_SAC, first_agent, n, (size_t)n * h->rep.A, out_actions);
}
int rlc_sac_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices, const float* eps) {
    return rlc_sacfam_update(RLC_ALGO_SAC, h, n_updates, host_indices, eps);
}
int rlc_sac_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                         const double* next_states, const double* rewards, const double* gammas, const float* eps) {
    return rlc_sacfam_update_batch(RLC_ALGO_SAC, h, agent, batch, states, actions, next_states, rewards, gammas, eps);
}
int rlc_sac_set_kernel(rlc_handle* h, int32_t variant) {
    // 2 also takes the wide shapes (state_dim <= 32, action_dim in {1,2,3,4,6}), which 0 leaves on the any-shape kernel
    const char* why = h && h->algo == RLC_ALGO_SAC && variant == 2 ? rlc_sac_mfma_refusal(h->sac.d) : nullptr;
    return rlc_h_set_kernel(h, RLC_ALGO_SAC, variant,
                            why ? std::string("MFMA SAC kernel does not support these dimensions: ") + why : std::string());
}
int rlc_sac_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_SAC, variant_in_use); }
int rlc_sac_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_SAC, on); }
int rlc_sac_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_SAC, agent, which, dst, n);
}

}  // extern "C"
