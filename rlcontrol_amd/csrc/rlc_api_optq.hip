// rlc_api_optq.hip -- C ABI of the OptimalQ population (declared in include/rlcontrol_hip.h).
#include "rlc_handle.h"

// floats of one acting launch's output: the grid rows [n][A], then their Q [n]
static size_t optq_act_floats(const rlc_handle* h, int n) { return (size_t)n * (h->rep.A + 1); }

extern "C" {

int rlc_optq_create(const rlc_optq_config* cfg, rlc_handle** out) {
    RLC_REQUIRE(cfg && out, "null argument");
    RLC_REQUIRE(cfg->l1_dim >= 1 && cfg->l2_dim >= 1, "layer widths must be >= 1");
    RLC_REQUIRE(cfg->action_dim <= RLC_OPTQ_MAX_A, "OptimalQ supports action_dim <= %d (got %d)", RLC_OPTQ_MAX_A,
                cfg->action_dim);
    RLC_REQUIRE(cfg->norm_type == RLC_NORM_NONE,
                "norm_type %d (%s): OptimalQ implements 'none' / 'input_norm' (0) only; 'layer' (layer norm) and 'batch' "
                "(batch norm, optimal_q_network.py:33-45) are not implemented", cfg->norm_type,
                cfg->norm_type == RLC_NORM_LAYER ? "layer" : cfg->norm_type == 2 ? "batch" : "unknown");
    RLC_REQUIRE(cfg->n_nodes >= 1 && cfg->n_nodes <= RLC_OPTQ_MAX_NODES, "n_nodes %d outside [1, %d]", cfg->n_nodes,
                RLC_OPTQ_MAX_NODES);
    RLC_REQUIRE(cfg->state_min && cfg->state_max && cfg->learning_rate && cfg->node_actions, "null array");
    RLC_REQUIRE(cfg->state_dim >= 1 && cfg->action_dim >= 1 && cfg->batch_size >= 1, "state_dim/action_dim/batch_size must be >= 1");
    const RlcOptqDims dims = rlc_optq_make_dims(cfg->state_dim, cfg->action_dim, cfg->l1_dim, cfg->l2_dim, cfg->batch_size);
    const char* why = rlc_optq_refusal(dims);
    RLC_REQUIRE(!why, "OptimalQ kernel does not support these dimensions: %s", why);
    RlcCreate c(RLC_ALGO_OPTQ, cfg->device, cfg->n_agents, cfg->state_dim, cfg->action_dim, cfg->batch_size,
                cfg->buffer_size, cfg->seed);
    if (c.rc) return c.finish("rlc_optq_create", out);
    RlcOptqDev& dv = c.h->optq;
    dv.d = dims;
    dv.rep = c.h->rep;
    dv.n_agents = cfg->n_agents;
    dv.clip_state = cfg->clip_state;
    dv.tau = cfg->tau;
    dv.n_nodes = cfg->n_nodes;
    const size_t NA = cfg->n_agents, S = dv.d.S, A = dv.d.A;
    c.blobs(dv);
    c.upload(&dv.lr, cfg->learning_rate, NA);
    c.upload(&dv.smin, cfg->state_min, S);
    c.upload(&dv.smax, cfg->state_max, S);
    c.upload(&dv.grid, cfg->node_actions, (size_t)cfg->n_nodes * A);     // on the handle's stream, as every upload here
    c.alloc(&dv.tap_q, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_y, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_maxq, NA * RLC_MAX_BATCH);
    c.alloc(&dv.tap_astar, NA * RLC_MAX_BATCH * A);
    dv.scratch_stride = (long long)((rlc_optq_scratch_floats(dv.d) + 63) & ~(size_t)63);
    c.alloc(&dv.scratch, NA * (size_t)dv.scratch_stride, false);
    return c.finish("rlc_optq_create", out);
}

int rlc_optq_param_count(const rlc_handle* h, int64_t* out_p) { return rlc_h_param_count(h, RLC_ALGO_OPTQ, out_p); }
int rlc_optq_set_blob(rlc_handle* h, int32_t agent, int32_t which, const float* src, int64_t n) {
    return rlc_h_set_blob(h, RLC_ALGO_OPTQ, agent, which, src, n);
}
int rlc_optq_get_blob(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_get_blob(h, RLC_ALGO_OPTQ, agent, which, dst, n);
}
int rlc_optq_get_beta_powers(rlc_handle* h, int32_t agent, float* pw2) {
    return rlc_h_beta_powers(h, RLC_ALGO_OPTQ, agent, pw2, false);
}
int rlc_optq_init_target(rlc_handle* h, int32_t agent) { return rlc_h_init_target(h, RLC_ALGO_OPTQ, agent); }

int rlc_optq_act(rlc_handle* h, int32_t first_agent, int32_t n, const double* states, float* out_action, float* out_q) {
    RLC_NEED(h, RLC_ALGO_OPTQ);
    const size_t a_f = (size_t)n * h->rep.A;
    return rlc_h_act(h, RLC_ALGO_OPTQ, first_agent, n, states, nullptr, 0, optq_act_floats(h, n), false,
                     [&](const float* in, float* out) {
                         return rlc_launch_optq_act(h->optq, first_agent, n, in, out, out + a_f, h->st);
                     },
                     out_action, out_q, (size_t)n);
}

// the acting forward queued behind the update that was just launched (see rlc_ddpg_act_queue, rlc_api.hip)
int rlc_optq_act_queue(rlc_handle* h, int32_t first_agent, int32_t n, const double* states) {
    RLC_NEED(h, RLC_ALGO_OPTQ);
    const size_t a_f = (size_t)n * h->rep.A;
    return rlc_h_act(h, RLC_ALGO_OPTQ, first_agent, n, states, nullptr, 0, optq_act_floats(h, n), true,
                     [&](const float* in, float* out) {
                         return rlc_launch_optq_act(h->optq, first_agent, n, in, out, out + a_f, h->st, rlc_h_aq_flag(h),
                                                    h->aq_seq);
                     });
}

int rlc_optq_act_fetch(rlc_handle* h, int32_t first_agent, int32_t n, float* out_action, float* out_q) {
    RLC_NEED(h, RLC_ALGO_OPTQ);
    return rlc_h_act_fetch(h, RLC_ALGO_OPTQ, first_agent, n, optq_act_floats(h, n), out_action, out_q, (size_t)n);
}

int rlc_optq_update(rlc_handle* h, int32_t n_updates, const int64_t* host_indices) {
    int source = 0;
    const long long* idx = nullptr;
    const int rc = rlc_h_update_begin(h, RLC_ALGO_OPTQ, n_updates, host_indices, 0, false, &source, &idx);
    if (rc || n_updates == 0) return rc;
    return rlc_launch_optq_update(h->optq, 0, h->optq.n_agents, n_updates, source, idx, h->grad_taps, h->st);
}

int rlc_optq_update_batch(rlc_handle* h, int32_t agent, int32_t batch, const double* states, const double* actions,
                          const double* next_states, const double* rewards, const double* gammas) {
    if (int rc = rlc_h_stage_batch(h, RLC_ALGO_OPTQ, agent, batch, states, actions, next_states, rewards, gammas)) return rc;
    return rlc_launch_optq_update(h->optq, agent, 1, 1, RLC_SRC_STAGING, nullptr, h->grad_taps, h->st);
}

int rlc_optq_qval(rlc_handle* h, int32_t agent, int32_t n, const double* states, const double* actions, float* out_q) {
    if (rlc_h_check_agent(h, agent) || rlc_h_use_device(h)) return 2;
    RLC_NEED(h, RLC_ALGO_OPTQ);
    RLC_REQUIRE(n >= 1 && states && actions && out_q, "bad arguments");
    const size_t S = h->rep.S, A = h->rep.A;
    const size_t in_b = sizeof(float) * n * (S + A), out_b = sizeof(float) * n;
    if (rlc_h_ensure_io(h, in_b + out_b)) return 1;
    float* hin = (float*)h->io_host;
    for (size_t i = 0; i < (size_t)n * S; i++) hin[i] = (float)states[i];
    for (size_t i = 0; i < (size_t)n * A; i++) hin[n * S + i] = (float)actions[i];
    RLC_HIP(hipMemcpyAsync(h->io_dev, hin, in_b, hipMemcpyHostToDevice, h->st));
    float* dout = h->io_dev + n * (S + A);
    if (rlc_launch_optq_qval(h->optq, agent, n, h->io_dev, h->io_dev + n * S, dout, h->st)) return 1;
    RLC_HIP(hipMemcpyAsync(hin + n * (S + A), dout, out_b, hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    memcpy(out_q, hin + n * (S + A), out_b);
    return 0;
}

int rlc_optq_set_kernel(rlc_handle* h, int32_t variant) {
    return rlc_h_set_kernel(h, RLC_ALGO_OPTQ, variant, "OptimalQ runs on the any-shape kernel only");
}
int rlc_optq_get_kernel(const rlc_handle* h, int32_t* variant_in_use) { return rlc_h_get_kernel(h, RLC_ALGO_OPTQ, variant_in_use); }
int rlc_optq_enable_grad_taps(rlc_handle* h, int32_t on) { return rlc_h_enable_grad_taps(h, RLC_ALGO_OPTQ, on); }
int rlc_optq_last_tap(rlc_handle* h, int32_t agent, int32_t which, float* dst, int64_t n) {
    return rlc_h_last_tap(h, RLC_ALGO_OPTQ, agent, which, dst, n);
}

}  // extern "C"
