// rlc_api_ac.hip -- C ABI of the ActorCritic population (declared in include/rlcontrol_hip.h).
#include "rlc_handle.h"

namespace {

// the caller's normals eps_next [rows * nd * A] and eps [rows * n * A] -> the device buffer behind the index upload area
// (both null: the device draws); layout of idx_dev: [idx_count long long][eps_next floats][eps floats]
size_t draw_floats(const rlc_handle* h, size_t rows) {
    const RlcAcDev& v = h->ac;
    return rows * ((size_t)rlc_ac_next_draws(v.critic_mode, v.d.n) + v.d.n) * v.d.A;
}

int check_draws(const rlc_handle* h, const float* eps_next, const float* eps) {
    const bool wants_next = rlc_ac_next_draws(h->ac.critic_mode, h->ac.d.n) > 0;
    RLC_REQUIRE(eps || !eps_next, "eps_next without eps: pass both, or neither (the device's Philox stream)");
    RLC_REQUIRE(!eps || (eps_next != nullptr) == wants_next,
                "eps_next must be %s for this critic_update (mean: no draw, sampled: one per row, expected: num_samples)",
                wants_next ? "given along with eps" : "NULL");
    return 0;
}

int upload_draws(rlc_handle* h, const float* eps_next, const float* eps, size_t rows, size_t idx_count,
                 const float** eps_next_dev, const float** eps_dev) {
    *eps_next_dev = *eps_dev = nullptr;
    if (!eps) return 0;
    const RlcAcDev& v = h->ac;
    const size_t n_next = rows * rlc_ac_next_draws(v.critic_mode, v.d.n) * v.d.A, n_eps = rows * v.d.n * v.d.A;
    if (rlc_h_ensure_idx(h, idx_count + ((n_next + n_eps) * sizeof(float) + 7) / 8)) return 1;
    float* dst = (float*)(h->idx_dev + idx_count);
    if (n_next) RLC_HIP(hipMemcpyAsync(dst, eps_next, sizeof(float) * n_next, hipMemcpyHostToDevice, h->st));
    RLC_HIP(hipMemcpyAsync(dst + n_next, eps, sizeof(float) * n_eps, hipMemcpyHostToDevice, h->st));
    *eps_next_dev = n_next ? dst : nullptr;
    *eps_dev = dst + n_next;
    return 0;
}

int ac_act(rlc_handle* h, int first_agent, int n, const double* states, int sample, const float* eps, bool queued,
           float* out_actions) {
    RLC_NEED(h, RLC_ALGO_AC);
    RLC_REQUIRE(n >= 1, "agent range [%d,%d) invalid", first_agent, first_agent + n);
    const size_t A = h->rep.A, out_f = (size_t)n * A, extra_f = (sample && eps) ? (size_t)n * A : 0;
    std::vector<float> extra(extra_f);
    if (extra_f) memcpy(extra.data(), eps, sizeof(float) * n * A);
    return rlc_h_act(h, RLC_ALGO_AC, first_agent, n, states, extra.data(), extra_f, out_f, queued,
                     [&](const float* in, float* out) {
                         const float* ed = extra_f ? out - extra_f : nullptr;
                         return rlc_launch_ac_act(h->ac, first_agent, n, in, ed, sample ? 1 : 0, out, h->st,
                                                  queued ? rlc_h_aq_flag(h) : nullptr, queued ? h->aq_seq : 0);
                     },
                     out_actions);
}

}  // namespace

extern "C" {

int rlc_ac_create(const rlc_ac_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->shared_l1_dim >= 1 && cfg->actor_l2_dim >= 1 && cfg->critic_l2_dim >= 1, "layer widths must be >= 1");
    RLC_REQUIRE(cfg->state_dim >= 1 && cfg->action_dim >= 1 && cfg->batch_size >= 1, "state_dim/action_dim/batch_size must be >= 1");
    RLC_REQUIRE(cfg->action_dim <= RLC_AC_MAX_A, "ActorCritic supports action_dim <= %d (got %d)", RLC_AC_MAX_A,
                cfg->action_dim);
    RLC_REQUIRE(cfg->num_samples >= 1 && cfg->num_samples <= RLC_AC_MAX_SAMPLES,
                "ActorCritic supports 1 <= num_samples <= %d (got %d)", RLC_AC_MAX_SAMPLES, cfg->num_samples);
    RLC_REQUIRE(cfg->critic_update >= RLC_AC_CRITIC_MEAN && cfg->critic_update <= RLC_AC_CRITIC_EXPECTED,
                "critic_update %d: expected 0 (mean), 1 (sampled) or 2 (expected); 'random_q' is not implemented",
                cfg->critic_update);
    RLC_REQUIRE(cfg->actor_update >= RLC_AC_ACTOR_LL && cfg->actor_update <= RLC_AC_ACTOR_CEM,
                "actor_update %d: expected 0 (ll), 1 (ll_update_all) or 2 (cem); 'reparam' is not implemented",
                cfg->actor_update);
    RLC_REQUIRE(cfg->actor_update != RLC_AC_ACTOR_CEM || (cfg->top_k >= 1 && cfg->top_k <= cfg->num_samples),
                "top_k = int(num_samples * rho) must be in [1, num_samples] for actor_update cem (got %d of %d)", cfg->top_k,
                cfg->num_samples);
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE,
                "norm_type %d (%s): ActorCritic implements 'none' / 'input_norm' (0) only; 'layer' (layer norm) and 'batch' "
                "(batch norm, which the reference itself refuses, ac_network.py:78-79) are not implemented", cfg->norm_type,
                cfg->norm_type == RLC_NORM_LAYER ? "layer" : cfg->norm_type == 2 ? "batch" : "unknown");
    RLC_REQUIRE(cfg->state_min && cfg->state_max && cfg->action_max && cfg->actor_lr && cfg->critic_lr, "null array");
    const int top_k = cfg->actor_update == RLC_AC_ACTOR_CEM ? cfg->top_k : 1;
    const RlcAcDims dims = rlc_ac_make_dims(cfg->state_dim, cfg->action_dim, cfg->shared_l1_dim, cfg->actor_l2_dim,
                                            cfg->critic_l2_dim, cfg->num_samples, top_k, cfg->batch_size);
    const char* why = rlc_ac_refusal(dims);
    RLC_REQUIRE(!why, "ActorCritic kernel does not support these dimensions: %s", why);
    RlcCreate c(RLC_ALGO_AC, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_ac_create", out);
    RlcAcDev& dv = c.h->ac;
    dv.d = dims;
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.critic_mode = cfg->critic_update;
    dv.actor_mode = cfg->actor_update;
    dv.tau = cfg->tau;
    for (int j = 0; j < cfg->action_dim; j++) dv.amax[j] = cfg->action_max[j];
    const size_t NA = cfg->n_agents, S = dv.d.S, B = dv.d.B, ns = dv.d.n, A = dv.d.A;
    const size_t nn = rlc_ac_next_actions(dv.critic_mode, dv.d.n);
    c.blobs(dv);
    c.upload(&dv.actor_lr, cfg->actor_lr, NA);           // on the handle's stream, as every upload here
    c.upload(&dv.critic_lr, cfg->critic_lr, NA);
    c.upload(&dv.smin, cfg->state_min, S);
    c.upload(&dv.smax, cfg->state_max, S);
    c.alloc(&dv.noise_ctr, NA);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_y, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_anext, NA * B * nn * A);
    c.alloc(&dv.tap_raw, NA * B * ns * A);
    c.alloc(&dv.tap_sa, NA * B * ns * A);
    c.alloc(&dv.tap_sq, NA * B * ns);
    c.alloc(&dv.tap_w, NA * B * ns);
    dv.scratch_stride = (long long)((rlc_ac_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_ac_create", out);
}

int rlc_ac_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_AC, out_p); }
int rlc_ac_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_AC, agent, which, src, n);
}
int rlc_ac_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_AC, agent, which, dst, n);
}
int rlc_ac_set_beta_powers(rlc_handle* h, int32_t agent, const float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_AC, agent, const_cast<float*>(pw4), true);
}
int rlc_ac_get_beta_powers(rlc_handle* h, int32_t agent, float* pw4) {
    return rlc_h_beta_powers(h, RLC_ALGO_AC, agent, pw4, false);
}
int rlc_ac_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_AC, agent); }

int rlc_ac_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample, const float* eps,
               float* out_actions) {
    return ac_act(h, first_agent, n, states, sample, eps, false, out_actions);
}
// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_ac_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, int32_t sample,
                     const float* eps) {
    return ac_act(h, first_agent, n, states, sample, eps, true, nullptr);
}
int rlc_ac_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_actions) {
    RLC_NEED(h, RLC_ALGO_AC);
    return rlc_h_act_fetch(h, RLC_ALGO_AC, first_agent, n, (size_t)n * h->rep.A, out_actions);
}

int rlc_ac_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices, const float* eps_next, const float* eps) {
    RLC_NEED(h, RLC_ALGO_AC);
    if (check_draws(h, eps_next, eps)) return 1;
    const size_t rows = (size_t)h->rep.n_agents * (n_updates > 0 ? n_updates : 0) * h->B;
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, RLC_ALGO_AC, n_updates, host_indices,
                                      eps ? (draw_floats(h, rows) * sizeof(float) + 7) / 8 : 0, false, &source, &idx);
    if (rc || n_updates == 0) return rc;
    const float *next_dev = nullptr, *eps_dev = nullptr;
    if (upload_draws(h, eps_next, eps, rows, host_indices ? rows : 0, &next_dev, &eps_dev)) return 1;
    return rlc_launch_ac_update(h->ac, 0, h->ac.n_agents, n_updates, source, h->idx_dev, next_dev, eps_dev, h->grad_taps,
                                h->st);
}

int rlc_ac_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                        const double* next_states, const double* rewards, const double* gammas, const float* eps_next,
                        const float* eps) {
    RLC_NEED(h, RLC_ALGO_AC);
    if (check_draws(h, eps_next, eps)) return 1;
    if (int rc = rlc_h_stage_batch(h, RLC_ALGO_AC, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    const float *next_dev = nullptr, *eps_dev = nullptr;
    if (upload_draws(h, eps_next, eps, (size_t)batch, 0, &next_dev, &eps_dev)) return 1;
    return rlc_launch_ac_update(h->ac, agent, 1, 1, RLC_SRC_STAGING, nullptr, next_dev, eps_dev, h->grad_taps, h->st);
}

int rlc_ac_qval(rlc_handle* h, int32_t agent, int32_t n, const double* states, const double* actions, float* out_q) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_AC);
    RLC_REQUIRE(n >= 1 && states && actions && out_q, "bad arguments");
    const size_t S = h->rep.S, A = h->rep.A;
    const size_t in_b = sizeof(float) * n * (S + A), out_b = sizeof(float) * n;
    if (rlc_h_ensure_io(h, in_b + out_b)) return 1;
    float* hin = (float*)h->io_host;
    for (size_t i = 0; i < (size_t)n * S; i++) hin[i] = (float)states[i];
    for (size_t i = 0; i < (size_t)n * A; i++) hin[n * S + i] = (float)actions[i];
    RLC_HIP(hipMemcpyAsync(h->io_dev, hin, in_b, hipMemcpyHostToDevice, h->st));
    float* dout = h->io_dev + n * (S + A);
    if (rlc_launch_ac_qval(h->ac, agent, n, h->io_dev, h->io_dev + n * S, dout, h->st)) return 1;
    RLC_HIP(hipMemcpyAsync(hin + n * (S + A), dout, out_b, hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    memcpy(out_q, hin + n * (S + A), out_b);
    return 0;
}

int rlc_ac_set_kernel(rlc_handle* h, int32_t variant) {
    return rlc_h_set_kernel(h, RLC_ALGO_AC, variant, "ActorCritic runs on the any-shape kernel only");
}
int rlc_ac_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_AC, variant_in_use); }
int rlc_ac_set_split(rlc_handle* h, int32_t n_workgroups) {
    if (int rc = rlc_h_split_check(h, RLC_ALGO_AC, n_workgroups)) return rc;
    RLC_REQUIRE(n_workgroups == 1, "ActorCritic has no latency mode: one workgroup per agent (the any-shape kernel only)");
    return 0;
}
int rlc_ac_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_AC, on); }
int rlc_ac_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_AC, agent, which, dst, n);
}

}  // extern "C"
