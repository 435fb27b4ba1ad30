// rlc_handle.h -- the one opaque handle type behind rlc_ddpg / rlc_sac / rlc_naf (include/rlcontrol_hip.h):
// a population of independent agents of ONE algorithm on one GPU.  The replay ring, the staging buffers,
// the stream and the timer are common; the networks and optimizer state are per algorithm.
#pragma once
#include <string.h>

#include <string>

#include "rlc_common.h"
#include "sac_common.h"
#include "naf_common.h"
#include "optq_common.h"
#include "wf_common.h"
#include "ae_common.h"
#include "ac_common.h"

// KL: ReverseKL / ForwardKL, on RlcSacDev
enum RlcAlgo { RLC_ALGO_DDPG = 1, RLC_ALGO_SAC = 2, RLC_ALGO_NAF = 3, RLC_ALGO_KL = 4, RLC_ALGO_OPTQ = 5, RLC_ALGO_WF = 6,
               RLC_ALGO_AE = 7, RLC_ALGO_AC = 8 };

struct rlc_handle {
    int algo;
    int device;
    int B;                               // batch_size
    hipStream_t st;
    hipEvent_t ev0, ev1;
    RlcReplayDev rep;                    // device view of the replay (also copied into the per-algorithm views)
    std::vector<RlcRingMeta> ring;       // host mirror of the ring metadata
    std::vector<void*> allocs;           // every hipMalloc of this handle
    long long* idx_dev; size_t idx_cap;  // host-index upload buffer
    float* io_dev; size_t io_cap;        // act / qval / gather staging (device, bytes)
    void* io_host; size_t io_host_cap;   // pinned host staging (bytes)
    bool io_pending;                     // async copies out of io_host may still be in flight (the update_batch paths)
    // queued acting forward (rlc_ddpg_act_queue / rlc_ddpg_act_fetch): buffers of their own, nothing else writes them
    float* aq_dev; float* aq_host; size_t aq_cap;   // device / pinned host staging: [n][S] states then [n][A] actions
    int aq_first, aq_n;                  // agent range of the queued forward; aq_n == 0: nothing queued
    int aq_seq;                          // completion flag protocol of one-agent forwards: the kernel stores ++aq_seq
    size_t aq_out;                       // float offset of the queued forward's outputs in aq_host
    bool aq_flagged;                     // the queued forward reports through the flag word (aq_host[aq_cap / 4 - 1])
    long long* idx_pin; size_t idx_pin_cap;   // pinned, device-readable index staging for small host-index updates
    hipEvent_t idx_ev; bool idx_ev_armed;     // recorded behind the launch that reads idx_pin
    // ---- DDPG
    RlcDev dv;
    int variant;                         // requested kernel: 0 auto, 1 generic, 2 mfma
    int grad_taps;
    int split_c;                         // > 1: latency mode, one agent's minibatch over split_c workgroups (ddpg_split.hip)
    float* split_part; unsigned int* split_bar; int* split_err;
    bool split_poisoned;                 // a latency-mode update failed at a cross-workgroup barrier: refuse further ones
    bool split_fail_next;                // test hook (rlc_debug_fail_next_split): the next launch finds the error word set
    // ---- SAC
    RlcSacDev sac;
    // ---- NAF
    RlcNafDev naf;
    // ---- OptimalQ
    RlcOptqDev optq;
    // ---- WireFitting
    RlcWfDev wf;
    // ---- ActorExpert
    RlcAeDev ae;
    // ---- ActorCritic
    RlcAcDev ac;
    // ---- on-device experiment loop (rlc_api_rollout.hip)
    bool has_env;
    RlcEnvDev env;
    RlcRollout* rollout_dev;             // device copy of {dv, env}: argument block of the fused step launches
    struct RlcSacRollout* sac_rollout_dev;   // same for a SoftActorCritic population
    struct RlcNafRollout* naf_rollout_dev;   // same for a NAF population
    long long ro_total_limit, ro_eval_interval, ro_steps, ro_evals;
    int ro_pending_q8;                   // an evaluation ran after the last update: next step resets OU after acting
};

// Latency-mode launches (ddpg_split.hip / kl_mfma.hip): the error word is cleared before every launch (set instead when
// the test hook asked for a failure) and read back after it.  On failure every workgroup has left the kernel at the
// barrier that failed, before any store of the phase behind it: parameters / optimizer state are those of the last
// COMPLETED phase of the failed update.  The handle then refuses latency-mode updates until rlc_*_set_split re-arms it
// (after the caller has reloaded or accepted the state).
int rlc_h_split_before_launch(rlc_handle* h);
int rlc_h_split_after_launch(rlc_handle* h);

// ---- what differs between the algorithms on the host side is data: the tables below; the bodies are in rlc_api.hip ----
inline const char* rlc_algo_name(int algo) {
    return algo == RLC_ALGO_DDPG ? "DDPG" : algo == RLC_ALGO_SAC ? "SoftActorCritic" : algo == RLC_ALGO_NAF ? "NAF"
           : algo == RLC_ALGO_OPTQ ? "OptimalQ" : algo == RLC_ALGO_WF ? "WireFitting"
           : algo == RLC_ALGO_AE ? "ActorExpert" : algo == RLC_ALGO_AC ? "ActorCritic" : "ReverseKL / ForwardKL";
}
#define RLC_NEED(h, a) RLC_REQUIRE((h) && (h)->algo == (a), "handle is not a %s population", rlc_algo_name(a))

// f(device view of the handle's algorithm)
template <class F>
int rlc_h_with_dev(rlc_handle* h, F f) {
    return h->algo == RLC_ALGO_DDPG ? f(h->dv) : h->algo == RLC_ALGO_NAF ? f(h->naf) : h->algo == RLC_ALGO_OPTQ ? f(h->optq)
           : h->algo == RLC_ALGO_WF ? f(h->wf) : h->algo == RLC_ALGO_AE ? f(h->ae) : h->algo == RLC_ALGO_AC ? f(h->ac)
           : f(h->sac);
}

// the per-agent parameter-shaped blobs [n_agents][Ppad], in the order of the ABI's blob selector
inline std::vector<float**> rlc_blobs(RlcDev& v) { return {&v.theta, &v.theta_t, &v.m_a, &v.v_a, &v.m_c, &v.v_c}; }
inline std::vector<float**> rlc_blobs(RlcSacDev& v) { return {&v.theta, &v.theta_t, &v.m, &v.v}; }
inline std::vector<float**> rlc_blobs(RlcNafDev& v) { return {&v.theta, &v.theta_t, &v.m, &v.v}; }
inline std::vector<float**> rlc_blobs(RlcOptqDev& v) { return {&v.theta, &v.theta_t, &v.m, &v.v}; }
inline std::vector<float**> rlc_blobs(RlcWfDev& v) { return {&v.theta, &v.theta_t, &v.m, &v.v}; }
inline std::vector<float**> rlc_blobs(RlcAeDev& v) { return {&v.theta, &v.theta_t, &v.m_a, &v.v_a, &v.m_c, &v.v_c}; }
inline std::vector<float**> rlc_blobs(RlcAcDev& v) { return {&v.theta, &v.theta_t, &v.m_a, &v.v_a, &v.m_c, &v.v_c}; }
// the gradient taps, blobs that exist only after *_enable_grad_taps
inline std::vector<float**> rlc_grad_taps(RlcDev& v) { return {&v.tap_gc, &v.tap_ga}; }
inline std::vector<float**> rlc_grad_taps(RlcSacDev& v) { return {&v.tap_g}; }
inline std::vector<float**> rlc_grad_taps(RlcNafDev& v) { return {&v.tap_g}; }
inline std::vector<float**> rlc_grad_taps(RlcOptqDev& v) { return {&v.tap_g}; }
inline std::vector<float**> rlc_grad_taps(RlcWfDev& v) { return {&v.tap_g}; }
inline std::vector<float**> rlc_grad_taps(RlcAeDev& v) { return {&v.tap_ga, &v.tap_gc}; }
inline std::vector<float**> rlc_grad_taps(RlcAcDev& v) { return {&v.tap_ga, &v.tap_gc}; }
// the same dims with the other weight layout
inline RlcDims rlc_with_layout(const RlcDims& d, int blocked) {
    return rlc_make_dims(d.S, d.A, d.H1, d.HA, d.HC, d.B, blocked, d.norm, d.sep);
}
inline RlcSacDims rlc_with_layout(const RlcSacDims& d, int blocked) {
    return rlc_sac_make_dims(d.S, d.A, d.L1A, d.L2A, d.L1C, d.L2C, d.B, blocked, d.qcat, d.norm);
}
inline RlcNafDims rlc_with_layout(const RlcNafDims& d, int blocked) {
    return rlc_naf_make_dims(d.S, d.A, d.L1, d.L2, d.B, blocked, d.norm);
}
inline RlcOptqDims rlc_with_layout(const RlcOptqDims& d, int) { return d; }     // one layout: row-major
inline RlcWfDims rlc_with_layout(const RlcWfDims& d, int) { return d; }         // one layout: row-major
inline RlcAeDims rlc_with_layout(const RlcAeDims& d, int) { return d; }         // one layout: row-major
inline RlcAcDims rlc_with_layout(const RlcAcDims& d, int) { return d; }         // one layout: row-major
inline int rlc_beta_powers(const RlcDev&) { return 4; }
inline int rlc_beta_powers(const RlcSacDev&) { return 4; }
inline int rlc_beta_powers(const RlcNafDev&) { return 2; }
inline int rlc_beta_powers(const RlcOptqDev&) { return 2; }
inline int rlc_beta_powers(const RlcWfDev&) { return 2; }
inline int rlc_beta_powers(const RlcAeDev&) { return 4; }
inline int rlc_beta_powers(const RlcAcDev&) { return 4; }
// tap `which` of the last update: all agents' array (null: not available), per-agent stride, floats the caller gets,
// blob = stored in the padded device layout of a parameter blob
struct RlcTap { const float* base; size_t stride; long long len; bool blob; };
inline RlcTap rlc_tap(const RlcDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH, A = v.d.A;
    const RlcTap t[] = {{v.tap_q, MB, B, false},
                        {v.tap_y, MB, B, false},
                        {v.tap_aout, MB * A, B * (long long)A, false},
                        {v.tap_dqda, MB * A, B * (long long)A, false},
                        {v.tap_gc, (size_t)v.d.Ppad, v.d.P, true},
                        {v.tap_ga, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 6 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcSacDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH, IQ = (size_t)B * v.kl_nodes;
    const RlcTap t[] = {{v.tap_q, MB, B, false},
                        {v.tap_v, MB, B, false},
                        {v.tap_logp, MB, B, false},
                        {v.tap_qpi, MB, B, false},
                        {v.tap_loss, 4, 3, false},
                        {v.tap_g, (size_t)v.d.Ppad, v.d.P, true},
                        {v.kl_tap_iq, IQ, (long long)IQ, false}};      // Q at the quadrature nodes: KL populations only
    return which >= 0 && which < 7 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcNafDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH;
    const RlcTap t[] = {{v.tap_q, MB, B, false}, {v.tap_y, MB, B, false}, {v.tap_V, MB, B, false},
                        {v.tap_g, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 4 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcOptqDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH, A = v.d.A;
    const RlcTap t[] = {{v.tap_q, MB, B, false}, {v.tap_y, MB, B, false}, {v.tap_maxq, MB, B, false},
                        {v.tap_astar, MB * A, B * (long long)A, false}, {v.tap_g, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 5 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcWfDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH;
    const RlcTap t[] = {{v.tap_q, MB, B, false}, {v.tap_y, MB, B, false}, {v.tap_maxq, MB, B, false},
                        {v.tap_g, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 4 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcAeDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH, A = v.d.A, SN = (size_t)B * v.d.n, SK = (size_t)B * v.d.k;
    const RlcTap t[] = {{v.tap_q, MB, B, false},
                        {v.tap_y, MB, B, false},
                        {v.tap_anext, MB * A, B * (long long)A, false},
                        {v.tap_sa, SN * A, (long long)(SN * A), false},
                        {v.tap_sq, SN, (long long)SN, false},
                        {v.tap_sel, SK, (long long)SK, false},
                        {v.tap_loss, 4, 1, false},
                        {v.tap_ga, (size_t)v.d.Ppad, v.d.P, true},
                        {v.tap_gc, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 9 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
inline RlcTap rlc_tap(const RlcAcDev& v, int which, int B) {
    const size_t MB = RLC_MAX_BATCH, A = v.d.A, SN = (size_t)B * v.d.n;
    const size_t NX = (size_t)B * rlc_ac_next_actions(v.critic_mode, v.d.n) * A;
    const RlcTap t[] = {{v.tap_q, MB, B, false},
                        {v.tap_y, MB, B, false},
                        {v.tap_anext, NX, (long long)NX, false},
                        {v.tap_raw, SN * A, (long long)(SN * A), false},
                        {v.tap_sa, SN * A, (long long)(SN * A), false},
                        {v.tap_sq, SN, (long long)SN, false},
                        {v.tap_w, SN, (long long)SN, false},
                        {v.tap_ga, (size_t)v.d.Ppad, v.d.P, true},
                        {v.tap_gc, (size_t)v.d.Ppad, v.d.P, true}};
    return which >= 0 && which < 9 ? t[which] : RlcTap{nullptr, 0, 0, false};
}
// kernel variant in use (1 generic, 2 mfma): the request h->variant (0 auto) resolved against the shape support
inline int rlc_h_variant(const rlc_handle* h) {
    if (h->variant == 1 || h->variant == 2) return h->variant;
    switch (h->algo) {
        case RLC_ALGO_DDPG: return rlc_mfma_supported(h->dv.d) ? 2 : 1;
        case RLC_ALGO_SAC: return rlc_sac_mfma_supported(h->sac.d) ? 2 : 1;
        case RLC_ALGO_NAF: return rlc_naf_mfma_supported(h->naf.d) ? 2 : 1;
        case RLC_ALGO_OPTQ: return 1;     // the any-shape kernel only
        case RLC_ALGO_WF: return 1;       // the any-shape kernel only
        case RLC_ALGO_AE: return 1;       // the any-shape kernel only
        case RLC_ALGO_AC: return 1;       // the any-shape kernel only
        // above one action dimension the KL MFMA kernel is opt-in (rlc_kl_set_kernel)
        default: return (h->sac.d.A == 1 && rlc_kl_mfma_supported(h->sac.d, h->sac.kl_nodes)) ? 2 : 1;
    }
}
// fused update launch of the variant in use (rlc_api_sac.hip / rlc_api_naf.hip)
int rlc_h_sac_launch_update(rlc_handle* h, int first, int n, int n_updates, int source, const long long* idx_dev,
                            const float* eps_dev, const struct RlcSacRollout* rollout);
int rlc_h_naf_launch_update(rlc_handle* h, int first, int n, int n_updates, int source, const long long* idx_dev,
                            const struct RlcNafRollout* rollout);

// bodies of the rlc_sac_* / rlc_kl_* entry points that carry eps (rlc_api_sac.hip); algo = RLC_ALGO_SAC or RLC_ALGO_KL
int rlc_sacfam_act(int algo, rlc_handle* h, int first_agent, int n, const double* states, int sample, const float* eps,
                   bool queued, float* out_actions);
int rlc_sacfam_update(int algo, rlc_handle* h, int n_updates, const int64_t* host_indices, const float* eps);
int rlc_sacfam_update_batch(int algo, rlc_handle* h, int agent, int batch, const double* states, const double* actions,
                            const double* next_states, const double* rewards, const double* gammas, const float* eps);

// ---- one body per operation for every algorithm (rlc_api.hip); `algo` is the one the calling entry point belongs to ----
int rlc_h_check_agent(const rlc_handle* h, int agent);
int rlc_h_use_device(const rlc_handle* h);
int rlc_h_param_count(const rlc_handle* h, int algo, int64_t* out_p);
int rlc_h_set_blob(rlc_handle* h, int algo, int agent, int which, const float* src, int64_t n);
int rlc_h_get_blob(rlc_handle* h, int algo, int agent, int which, float* dst, int64_t n);
int rlc_h_init_target(rlc_handle* h, int algo, int agent);
int rlc_h_beta_powers(rlc_handle* h, int algo, int agent, float* pw, bool set);
int rlc_h_enable_grad_taps(rlc_handle* h, int algo, int on);
int rlc_h_last_tap(rlc_handle* h, int algo, int agent, int which, float* dst, int64_t n);
// re-pack every blob between the row-major and the tile-blocked layout (a kernel switch changes the weight layout)
int rlc_h_relayout(rlc_handle* h, int blocked);
// (re)write the device copy of a DDPG handle's views {dv, env}, the argument block of the fused step launches: when the
// rollout is created, and when a kernel switch has changed dv (the weight layout) with a rollout attached
int rlc_h_upload_ddpg_rollout(rlc_handle* h);
// set_kernel: argument checks (mfma_refusal: why variant 2 cannot run, empty if it can), then the re-pack
int rlc_h_set_kernel(rlc_handle* h, int algo, int variant, const std::string& mfma_refusal, bool refuse_rollout = true);
int rlc_h_get_kernel(const rlc_handle* h, int algo, int32_t* variant_in_use);
// set_split, first half: handle / range / rollout checks; n_workgroups == 1 switches latency mode off
int rlc_h_split_check(rlc_handle* h, int algo, int n_workgroups);
// set_split, second half: `grid` co-resident workgroups must fit the GPU; barrier and error words; `part_floats` > 0:
// a (new) zeroed partial-result buffer of that size; re-arm
int rlc_h_split_arm(rlc_handle* h, int n_workgroups, int grid, size_t part_floats);
// update, front half: checks, then the minibatch source and (host indices) their device-readable copy in *idx, with room
// for extra_ll more 8-byte words behind them in h->idx_dev.  pinned_small: up to 1024 indices are read by the kernel
// straight from pinned host memory (*idx == h->idx_pin; the caller then calls rlc_h_update_launched behind its launch)
int rlc_h_update_begin(rlc_handle* h, int algo, int n_updates, const int64_t* host_indices, size_t extra_ll,
                       bool pinned_small, int* source, const long long** idx);
int rlc_h_update_launched(rlc_handle* h, const long long* idx);
// update_batch, front half: checks, fp64 minibatch -> pinned staging -> the agent's gather slots
int rlc_h_stage_batch(rlc_handle* h, int algo, int agent, int batch, const double* states, const double* actions,
                      const double* next_states, const double* rewards, const double* gammas);
// queued acting forward: pinned staging + completion word
int rlc_h_aq_begin(rlc_handle* h, size_t floats, bool flagged);
int* rlc_h_aq_flag(rlc_handle* h);
int rlc_h_aq_wait(rlc_handle* h, int first_agent, int n);
int rlc_h_ensure_io(rlc_handle* h, size_t bytes);
int rlc_h_ensure_idx(rlc_handle* h, size_t count);
int rlc_h_init_common(rlc_handle* h, int algo, int device, int n_agents, int S, int A, int B, long long cap,
                      const uint64_t* seeds);
void rlc_h_destroy(rlc_handle* h);
template <typename T>
int rlc_h_malloc(rlc_handle* h, T** out, size_t count, bool zero = true) {
    void* p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    RLC_HIP(hipMalloc(&p, bytes));
    if (zero) RLC_HIP(hipMemsetAsync(p, 0, bytes, h->st));
    h->allocs.push_back(p);
    *out = (T*)p;
    return 0;
}

// Acting, both forms: agent-range check, fp64 states -> fp32 staging with `extra_f` more input floats behind them
// (SoftActorCritic's eps), launch(inputs, outputs), and for the plain form the out_f output floats copied to `out` /
// `out2` (the last out2_f of them; may be null).  queued: zero-copy through pinned memory, nothing is waited for.
template <class L>
int rlc_h_act(rlc_handle* h, int algo, int first_agent, int n, const double* states, const float* extra, size_t extra_f,
              size_t out_f, bool queued, L launch, float* out = nullptr, float* out2 = nullptr, size_t out2_f = 0) {
    RLC_NEED(h, algo);
    if (rlc_h_use_device(h)) return 1;
    RLC_REQUIRE(n >= 1 && first_agent >= 0 && first_agent + n <= h->rep.n_agents, "agent range [%d,%d) invalid",
                first_agent, first_agent + n);
    RLC_REQUIRE(states && (queued || out), "null array");
    const size_t in_f = (size_t)n * h->rep.S + extra_f;
    if (queued ? rlc_h_aq_begin(h, in_f + out_f, n == 1) : rlc_h_ensure_io(h, sizeof(float) * (in_f + out_f))) return 1;
    float* hin = queued ? h->aq_host : (float*)h->io_host;
    for (size_t i = 0; i < in_f - extra_f; i++) hin[i] = (float)states[i];
    for (size_t i = 0; i < extra_f; i++) hin[in_f - extra_f + i] = extra[i];
    if (queued) {
        if (launch(hin, hin + in_f)) return 1;
        h->aq_first = first_agent; h->aq_n = n;
        h->aq_out = in_f;
        return 0;
    }
    RLC_HIP(hipMemcpyAsync(h->io_dev, hin, sizeof(float) * in_f, hipMemcpyHostToDevice, h->st));
    if (launch(h->io_dev, h->io_dev + in_f)) return 1;
    RLC_HIP(hipMemcpyAsync(hin + in_f, h->io_dev + in_f, sizeof(float) * out_f, hipMemcpyDeviceToHost, h->st));
    RLC_HIP(hipStreamSynchronize(h->st));
    memcpy(out, hin + in_f, sizeof(float) * (out_f - out2_f));
    if (out2) memcpy(out2, hin + in_f + out_f - out2_f, sizeof(float) * out2_f);
    return 0;
}
// wait for the queued forward of agents [first_agent, first_agent + n) and copy its out_f output floats out
int rlc_h_act_fetch(rlc_handle* h, int algo, int first_agent, int n, size_t out_f, float* out, float* out2 = nullptr,
                    size_t out2_f = 0);

// The skeleton of every rlc_*_create: the handle, device allocations and host -> device uploads on the handle's stream
// (behind the zero-fill of their buffers); the first failure sticks and finish() reports it.
struct RlcCreate {
    rlc_handle* h;
    int rc;
    hipError_t e = hipSuccess;
    std::vector<float> pw;
    RlcCreate(int algo, int device, int n_agents, int S, int A, int B, long long cap, const uint64_t* seeds)
        : h(new rlc_handle()) {
        rc = rlc_h_init_common(h, algo, device, n_agents, S, A, B, cap, seeds);
    }
    template <typename T>
    void alloc(T** out, size_t count, bool zero = true) {
        if (!rc) rc = rlc_h_malloc(h, out, count, zero);
    }
    void up(void* dst, const void* src, size_t bytes) {
        if (!rc && e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->st);
    }
    // a device copy of src[count]
    template <typename T>
    void upload(const T** out, const T* src, size_t count) {
        T* p = nullptr;
        alloc(&p, count);
        up(p, src, count * sizeof(T));
        *out = p;
    }
    // parameters, target, optimizer moments; Adam's beta powers start at beta1, beta2
    template <class Dev>
    void blobs(Dev& dv, bool beta_powers = true) {
        const size_t NA = dv.n_agents, n = rlc_beta_powers(dv);
        for (float** b : rlc_blobs(dv)) alloc(b, NA * dv.d.Ppad);
        if (!beta_powers) return;
        pw.resize(NA * n);
        for (size_t i = 0; i < pw.size(); i++) pw[i] = i % 2 ? 0.999f : 0.9f;
        alloc(&dv.pw, pw.size());
        up(dv.pw, pw.data(), pw.size() * sizeof(float));
    }
    int finish(const char* who, rlc_handle** out) {
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(h->st);
        if (!rc && e != hipSuccess) {
            rlc_set_error("%s: upload failed: %s", who, hipGetErrorString(e));
            rc = 1;
        }
        if (rc) rlc_h_destroy(h);
        else *out = h;
        return rc;
    }
};
