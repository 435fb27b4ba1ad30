// rlc_api_wf.hip -- C ABI of the WireFitting population (declared in include/rlcontrol_hip.h).
#include "rlc_handle.h"

// floats of one acting launch's output: the arg-max wire's action [n][A], then every wire's action [n][N][A] and
// every wire's value [n][N]
static size_t wf_wire_floats(const rlc_handle* h, int n) { return (size_t)n * h->wf.d.N * (h->rep.A + 1); }
static size_t wf_act_floats(const rlc_handle* h, int n) { return (size_t)n * h->rep.A + wf_wire_floats(h, n); }

extern "C" {

int rlc_wf_create(const rlc_wf_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->l1_dim >= 1 && cfg->l2_dim >= 1, "layer widths must be >= 1");
    RLC_REQUIRE(cfg->state_dim >= 1 && cfg->action_dim >= 1 && cfg->batch_size >= 1, "state_dim/action_dim/batch_size must be >= 1");
    RLC_REQUIRE(cfg->action_dim <= RLC_WF_MAX_A, "WireFitting supports action_dim <= %d (got %d)", RLC_WF_MAX_A,
                cfg->action_dim);
    RLC_REQUIRE(cfg->app_points >= 1, "app_points must be >= 1 (got %d)", cfg->app_points);
    RLC_REQUIRE((long long)cfg->app_points * cfg->action_dim <= RLC_WF_MAX_NA,
                "WireFitting supports app_points * action_dim <= %d (got %d * %d)", RLC_WF_MAX_NA, cfg->app_points,
                cfg->action_dim);
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE,
                "norm_type %d (%s): WireFitting implements 'none' / 'input_norm' (0) only; 'layer' (layer norm) and 'batch' "
                "(batch norm, wf_network.py:43-44,77-79) are not implemented", cfg->norm_type,
                cfg->norm_type == RLC_NORM_LAYER ? "layer" : cfg->norm_type == 2 ? "batch" : "unknown");
    RLC_REQUIRE(cfg->state_min && cfg->state_max && cfg->learning_rate, "null array");
    const RlcWfDims dims = rlc_wf_make_dims(cfg->state_dim, cfg->action_dim, cfg->l1_dim, cfg->l2_dim, cfg->app_points,
                                            cfg->batch_size);
    const char* why = rlc_wf_refusal(dims);
    RLC_REQUIRE(!why, "WireFitting kernel does not support these dimensions: %s", why);
    RlcCreate c(RLC_ALGO_WF, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_wf_create", out);
    RlcWfDev& dv = c.h->wf;
    dv.d = dims;
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.tau = cfg->tau;
    dv.amax0 = cfg->action_max0;
    const size_t NA = cfg->n_agents, S = dv.d.S;
    c.blobs(dv);
    c.upload(&dv.lr, cfg->learning_rate, NA);            // on the handle's stream, as every upload here
    c.upload(&dv.smin, cfg->state_min, S);
    c.upload(&dv.smax, cfg->state_max, S);
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_y, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_maxq, NA * RLC_MAX_BATCH);
    dv.scratch_stride = (long long)((rlc_wf_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_wf_create", out);
}

int rlc_wf_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_WF, out_p); }
int rlc_wf_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_WF, agent, which, src, n);
}
int rlc_wf_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_WF, agent, which, dst, n);
}
int rlc_wf_set_beta_powers(rlc_handle* h, int32_t agent, const float* pw2) {
    return rlc_h_beta_powers(h, RLC_ALGO_WF, agent, const_cast<float*>(pw2), true);
}
int rlc_wf_get_beta_powers(rlc_handle* h, int32_t agent, float* pw2) {
    return rlc_h_beta_powers(h, RLC_ALGO_WF, agent, pw2, false);
}
int rlc_wf_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_WF, agent); }

int rlc_wf_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, float* out_action, float* out_wires) {
    RLC_NEED(h, RLC_ALGO_WF);
    return rlc_h_act(h, RLC_ALGO_WF, first_agent, n, states, nullptr, 0, wf_act_floats(h, n), false,
                     [&](const float* in, float* out) { return rlc_launch_wf_act(h->wf, first_agent, n, in, out, h->st); },
                     out_action, out_wires, wf_wire_floats(h, n));
}

// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_wf_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states) {
    RLC_NEED(h, RLC_ALGO_WF);
    return rlc_h_act(h, RLC_ALGO_WF, first_agent, n, states, nullptr, 0, wf_act_floats(h, n), true,
                     [&](const float* in, float* out) {
                         return rlc_launch_wf_act(h->wf, first_agent, n, in, out, h->st, rlc_h_aq_flag(h), h->aq_seq);
                     });
}

int rlc_wf_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_action, float* out_wires) {
    RLC_NEED(h, RLC_ALGO_WF);
    return rlc_h_act_fetch(h, RLC_ALGO_WF, first_agent, n, wf_act_floats(h, n), out_action, out_wires, wf_wire_floats(h, n));
}

int rlc_wf_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices) {
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, RLC_ALGO_WF, n_updates, host_indices, 0, false, &source, &idx);
    if (rc || n_updates == 0) return rc;
    return rlc_launch_wf_update(h->wf, 0, h->wf.n_agents, n_updates, source, idx, h->grad_taps, h->st);
}

int rlc_wf_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                        const double* next_states, const double* rewards, const double* gammas) {
    if (int rc = rlc_h_stage_batch(h, RLC_ALGO_WF, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    return rlc_launch_wf_update(h->wf, agent, 1, 1, RLC_SRC_STAGING, nullptr, h->grad_taps, h->st);
}

int rlc_wf_qval(rlc_handle* h, int32_t agent, int32_t n, const double* states, const double* actions, float* out_q) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_WF);
    RLC_REQUIRE(n >= 1 && states && actions && out_q, "bad arguments");
    const size_t S = h->rep.S, A = h->rep.A;
    const size_t in_b = sizeof(float) * n * (S + A), out_b = sizeof(float) * n;
    if (rlc_h_ensure_io(h, in_b + out_b)) return 1;
    float* hin = (float*)h->io_host;
    for (size_t i = 0; i < (size_t)n * S; i++) hin[i] = (float)states[i];
    for (size_t i = 0; i < (size_t)n * A; i++) hin[n * S + i] = (float)actions[i];
    RLC_HIP(hipMemcpyAsync(h->io_dev, hin, in_b, hipMemcpyHostToDevice, h->st));
    float* dout = h->io_dev + n * (S + A);
    if (rlc_launch_wf_qval(h->wf, agent, n, h->io_dev, h->io_dev + n * S, dout, h->st)) return 1;
    RLC_HIP(hipMemcpyAsync(hin + n * (S + A), dout, out_b, hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    memcpy(out_q, hin + n * (S + A), out_b);
    return 0;
}

int rlc_wf_set_kernel(rlc_handle* h, int32_t variant) {
    return rlc_h_set_kernel(h, RLC_ALGO_WF, variant, "WireFitting runs on the any-shape kernel only");
}
int rlc_wf_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_WF, variant_in_use); }
int rlc_wf_set_split(rlc_handle* h, int32_t n_workgroups) {
    if (int rc = rlc_h_split_check(h, RLC_ALGO_WF, n_workgroups)) return rc;
    RLC_REQUIRE(n_workgroups == 1, "WireFitting has no latency mode: one workgroup per agent (the any-shape kernel only)");
    return 0;
}
int rlc_wf_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_WF, on); }
int rlc_wf_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_WF, agent, which, dst, n);
}

}  // extern "C"
