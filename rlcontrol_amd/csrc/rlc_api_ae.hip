// rlc_api_ae.hip -- C ABI of the ActorExpert population (declared in include/rlcontrol_hip.h).
#include "rlc_handle.h"

namespace {

// the caller's draws u [count] and eps [count * A] -> the device buffer behind the index upload area (both null: the
// device draws); layout of idx_dev: [idx_count long long][count floats of u][count * A floats of eps]
int upload_draws(rlc_handle* h, const float* u, const float* eps, size_t count, size_t idx_count, const float** u_dev,
                 const float** eps_dev) {
    *u_dev = *eps_dev = nullptr;
    RLC_REQUIRE((u == nullptr) == (eps == nullptr), "u and eps: both null (the device's Philox stream) or neither");
    if (!u) return 0;
    const size_t A = h->rep.A, floats = count * (1 + A);
    if (rlc_h_ensure_idx(h, idx_count + (floats * sizeof(float) + 7) / 8)) return 1;
    float* dst = (float*)(h->idx_dev + idx_count);
    RLC_HIP(hipMemcpyAsync(dst, u, sizeof(float) * count, hipMemcpyHostToDevice, h->st));
    RLC_HIP(hipMemcpyAsync(dst + count, eps, sizeof(float) * count * A, hipMemcpyHostToDevice, h->st));
    *u_dev = dst;
    *eps_dev = dst + count;
    return 0;
}

int ae_act(rlc_handle* h, int first_agent, int n, const double* states, int sample, const float* u, const float* eps,
           bool queued, float* out_actions) {
    RLC_NEED(h, RLC_ALGO_AE);
    RLC_REQUIRE((u == nullptr) == (eps == nullptr), "u and eps: both null (the device's Philox stream) or neither");
    RLC_REQUIRE(n >= 1, "agent range [%d,%d) invalid", first_agent, first_agent + n);
    const size_t A = h->rep.A, out_f = (size_t)n * A, extra_f = (sample && u) ? (size_t)n * (1 + A) : 0;
    std::vector<float> extra(extra_f);
    if (extra_f) {
        memcpy(extra.data(), u, sizeof(float) * n);
        memcpy(extra.data() + n, eps, sizeof(float) * n * A);
    }
    return rlc_h_act(h, RLC_ALGO_AE, first_agent, n, states, extra.data(), extra_f, out_f, queued,
                     [&](const float* in, float* out) {
                         const float* ud = extra_f ? out - extra_f : nullptr;
                         return rlc_launch_ae_act(h->ae, first_agent, n, in, ud, ud ? ud + n : nullptr, sample ? 1 : 0, out,
                                                  h->st, queued ? rlc_h_aq_flag(h) : nullptr, queued ? h->aq_seq : 0);
                     },
                     out_actions);
}

}  // namespace

extern "C" {

int rlc_ae_create(const rlc_ae_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->shared_l1_dim >= 1 && cfg->actor_l2_dim >= 1 && cfg->expert_l2_dim >= 1, "layer widths must be >= 1");
    RLC_REQUIRE(cfg->state_dim >= 1 && cfg->action_dim >= 1 && cfg->batch_size >= 1, "state_dim/action_dim/batch_size must be >= 1");
    RLC_REQUIRE(cfg->action_dim <= RLC_AE_MAX_A, "ActorExpert supports action_dim <= %d (got %d)", RLC_AE_MAX_A,
                cfg->action_dim);
    RLC_REQUIRE(cfg->num_modal >= 1 && cfg->num_modal <= RLC_AE_MAX_M, "ActorExpert supports 1 <= num_modal <= %d (got %d)",
                RLC_AE_MAX_M, cfg->num_modal);
    RLC_REQUIRE(cfg->num_samples >= 1 && cfg->num_samples <= RLC_AE_MAX_SAMPLES,
                "ActorExpert supports 1 <= num_samples <= %d (got %d)", RLC_AE_MAX_SAMPLES, cfg->num_samples);
    RLC_REQUIRE(cfg->top_k >= 1 && cfg->top_k <= cfg->num_samples,
                "top_k = int(num_samples * rho) must be in [1, num_samples] (got %d of %d)", cfg->top_k, cfg->num_samples);
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE,
                "norm_type %d (%s): ActorExpert implements 'none' / 'input_norm' (0) only; 'layer' (layer norm) and 'batch' "
                "(batch norm, which the reference itself refuses, ae_network.py:93-94) are not implemented", cfg->norm_type,
                cfg->norm_type == RLC_NORM_LAYER ? "layer" : cfg->norm_type == 2 ? "batch" : "unknown");
    RLC_REQUIRE(cfg->state_min && cfg->state_max && cfg->action_min && cfg->action_max && cfg->actor_lr && cfg->expert_lr,
                "null array");
    const RlcAeDims dims = rlc_ae_make_dims(cfg->state_dim, cfg->action_dim, cfg->shared_l1_dim, cfg->actor_l2_dim,
                                            cfg->expert_l2_dim, cfg->num_modal, cfg->num_samples, cfg->top_k, cfg->batch_size);
    const char* why = rlc_ae_refusal(dims);
    RLC_REQUIRE(!why, "ActorExpert kernel does not support these dimensions: %s", why);
    RlcCreate c(RLC_ALGO_AE, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_ae_create", out);
    RlcAeDev& dv = c.h->ae;
    dv.d = dims;
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.tau = cfg->tau;
    for (int j = 0; j < cfg->action_dim; j++) { dv.amin[j] = cfg->action_min[j]; dv.amax[j] = cfg->action_max[j]; }
    const size_t NA = cfg->n_agents, S = dv.d.S, B = dv.d.B, ns = dv.d.n, A = dv.d.A;
    c.blobs(dv);
    c.upload(&dv.actor_lr, cfg->actor_lr, NA);           // on the handle's stream, as every upload here
    c.upload(&dv.expert_lr, cfg->expert_lr, NA);
    c.upload(&dv.smin, cfg->state_min, S);
    c.upload(&dv.smax, cfg->state_max, S);
    c.alloc(&dv.noise_ctr, NA);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_y, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_anext, NA * RLC_MAX_BATCH * A);
    c.alloc(&dv.tap_sa, NA * B * ns * A);
    c.alloc(&dv.tap_sq, NA * B * ns);
    c.alloc(&dv.tap_sel, NA * B * dv.d.k);
    c.alloc(&dv.tap_loss, NA * 4);
    dv.scratch_stride = (long long)((rlc_ae_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_ae_create", out);
}

int rlc_ae_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_AE, out_p); }
int rlc_ae_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_AE, agent, which, src, n);
}
int rlc_ae_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_AE, agent, which, dst, n);
}
int rlc_ae_set_beta_powers(rlc_handle* h, int32_t agent, const float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_AE, agent, const_cast<float*>(pw4), true);
}
int rlc_ae_get_beta_powers(rlc_handle* h, int32_t agent, float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_AE, agent, pw4, false);
}
int rlc_ae_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_AE, agent); }

int rlc_ae_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* u,
               const float* eps, float* out_actions) {
    return ae_act(h, first_agent, n, states, sample, u, eps, false, out_actions);
}
// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_ae_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* u,
                     const float* eps) {
    return ae_act(h, first_agent, n, states, sample, u, eps, true, nullptr);
}
int rlc_ae_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_actions) {
    RLC_NEED(h, RLC_ALGO_AE);
    return rlc_h_act_fetch(h, RLC_ALGO_AE, first_agent, n, (size_t)n * h->rep.A, out_actions);
}

int rlc_ae_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices, const float* u, const float* eps) {
    RLC_NEED(h, RLC_ALGO_AE);
    RLC_REQUIRE((u == nullptr) == (eps == nullptr), "u and eps: both null (the device's Philox stream) or neither");
    const size_t rows = (size_t)h->rep.n_agents * (n_updates > 0 ? n_updates : 0) * h->B, count = rows * h->ae.d.n;
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, RLC_ALGO_AE, n_updates, host_indices,
                                      u ? (count * (1 + h->rep.A) * sizeof(float) + 7) / 8 : 0, false, &source, &idx);
    if (rc || n_updates == 0) return rc;
    const float *u_dev = nullptr, *eps_dev = nullptr;
    if (upload_draws(h, u, eps, count, host_indices ? rows : 0, &u_dev, &eps_dev)) return 1;
    return rlc_launch_ae_update(h->ae, 0, h->ae.n_agents, n_updates, source, h->idx_dev, u_dev, eps_dev, h->grad_taps, h->st);
}

int rlc_ae_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                        const double* next_states, const double* rewards, const double* gammas, const float* u,
                        const float* eps) {
    if (int rc = rlc_h_stage_batch(h, RLC_ALGO_AE, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    const float *u_dev = nullptr, *eps_dev = nullptr;
    if (upload_draws(h, u, eps, (size_t)batch * h->ae.d.n, 0, &u_dev, &eps_dev)) return 1;
    return rlc_launch_ae_update(h->ae, agent, 1, 1, RLC_SRC_STAGING, nullptr, u_dev, eps_dev, h->grad_taps, h->st);
}

int rlc_ae_qval(rlc_handle* h, int32_t agent, int32_t n, const double* states, const double* actions, float* out_q) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_AE);
    RLC_REQUIRE(n >= 1 && states && actions && out_q, "bad arguments");
    const size_t S = h->rep.S, A = h->rep.A;
    const size_t in_b = sizeof(float) * n * (S + A), out_b = sizeof(float) * n;
    if (rlc_h_ensure_io(h, in_b + out_b)) return 1;
    float* hin = (float*)h->io_host;
    for (size_t i = 0; i < (size_t)n * S; i++) hin[i] = (float)states[i];
    for (size_t i = 0; i < (size_t)n * A; i++) hin[n * S + i] = (float)actions[i];
    RLC_HIP(hipMemcpyAsync(h->io_dev, hin, in_b, hipMemcpyHostToDevice, h->st));
    float* dout = h->io_dev + n * (S + A);
    if (rlc_launch_ae_qval(h->ae, agent, n, h->io_dev, h->io_dev + n * S, dout, h->st)) return 1;
    RLC_HIP(hipMemcpyAsync(hin + n * (S + A), dout, out_b, hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    memcpy(out_q, hin + n * (S + A), out_b);
    return 0;
}

int rlc_ae_set_kernel(rlc_handle* h, int32_t variant) {
    return rlc_h_set_kernel(h, RLC_ALGO_AE, variant, "ActorExpert runs on the any-shape kernel only");
}
int rlc_ae_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_AE, variant_in_use); }
int rlc_ae_set_split(rlc_handle* h, int32_t n_workgroups) {
    if (int rc = rlc_h_split_check(h, RLC_ALGO_AE, n_workgroups)) return rc;
    RLC_REQUIRE(n_workgroups == 1, "ActorExpert has no latency mode: one workgroup per agent (the any-shape kernel only)");
    return 0;
}
int rlc_ae_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_AE, on); }
int rlc_ae_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_AE, agent, which, dst, n);
}

}  // extern "C"
