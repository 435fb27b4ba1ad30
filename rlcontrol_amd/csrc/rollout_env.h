// rollout_env.h -- the simulated environment and the algorithm-independent half of one training step of the
// on-device experiment loop: env.step, BaseAgent.update's insert rule, the learn
// gate and the episode bookkeeping of experiment.py:113-135 / agents/base_agent.py:54-70.  Shared by the DDPG and
// SAC train steps (ddpg_rollout_device.h, sac_rollout_device.h) and by the evaluation kernels.
//
// Environments (selected by RlcEnvDev::env_id, uniform across a launch):
//   * Pendulum-v0 restated from the public gym 0.18.0 definition (third-party; see
//     rlcontrol_amd/environments/pendulum.py), simulated in float64 like gym does.  Reset draws come from a
//     Philox stream per agent, in the order a sequential run would draw them.  done == time limit (gym's TimeLimit).
//   * The reference's Bimodal toy environments (environments/environments.py:158-912; host restatement in
//     rlcontrol_amd/environments/bimodal.py), float64 in the reference's expression order, contraction off:
//     the seven one-step Bimodal1DEnv* bandits (one function, a constant table) and Bimodal2DEnv.  They report
//     `done` themselves and draw nothing at reset.  tests/golden/bimodal_envs.json pins them to the reference.
#pragma once
#include "rlc_common.h"

#ifdef __HIPCC__

#define RLC_KEY_ENV_TRAIN 0x7261696Eull
#define RLC_KEY_ENV_TEST 0x74657374ull
#define RLC_PI 3.14159265358979323846

__device__ inline double rlc_u01(unsigned int hi, unsigned int lo) {
    return (double)((((unsigned long long)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}

// ---- Pendulum-v0 -------------------------------------------------------------------------------
__device__ inline void pendulum_reset(double* sim, unsigned long long key, unsigned long long ctr) {
    const Philox4 p = philox4x32_10(key, ctr, 0);
    sim[0] = -RLC_PI + 2.0 * RLC_PI * rlc_u01(p.x, p.y);   // np_random.uniform(-[pi,1], [pi,1])
    sim[1] = -1.0 + 2.0 * rlc_u01(p.z, p.w);
}
__device__ inline void pendulum_obs(const double* sim, double* obs) {
    obs[0] = cos(sim[0]); obs[1] = sin(sim[0]); obs[2] = sim[1];
}
// returns the reward; advances sim
__device__ inline double pendulum_step(double* sim, const float* action) {
    const double th = sim[0], thdot = sim[1];
    const double u = fmin(fmax((double)action[0], -2.0), 2.0);
    double wrapped = fmod(th + RLC_PI, 2.0 * RLC_PI);
    if (wrapped < 0.0) wrapped += 2.0 * RLC_PI;          // Python's % is non-negative
    wrapped -= RLC_PI;
    const double cost = wrapped * wrapped + 0.1 * thdot * thdot + 0.001 * (u * u);
    double nthdot = thdot + (-3.0 * 10.0 / (2.0 * 1.0) * sin(th + RLC_PI) + 3.0 / (1.0 * 1.0 * 1.0) * u) * 0.05;
    const double nth = th + nthdot * 0.05;
    nthdot = fmin(fmax(nthdot, -8.0), 8.0);
    sim[0] = nth; sim[1] = nthdot;
    return -cost;
}

// ---- Bimodal1DEnv and its six variants ------------------------------------------------------------
// reward(a) = h1 exp(-0.5 ((a - m1) / s1)^2) + h2 exp(-0.5 ((a - m2) / s2)^2); rows in RLC_ENV_BIMODAL1D.. order
__device__ inline double bimodal1d_reward(int variant, double a) {
#pragma clang fp contract(off)
    //                               m1    m2   s1   s2   h1   h2
    static const double T[7][6] = {{-1.0, 1.0, 0.2, 0.2, 1.0, 1.5},      // Bimodal1DEnv
                                   {-1.0, 1.0, 0.4, 0.2, 1.0, 1.5},      // _uneq_var1
                                   {-1.0, 1.0, 0.3, 0.1, 1.0, 1.5},      // _uneq_var2
                                   {-1.0, 1.0, 0.3, 0.1, 1.0, 1.0},      // _uneq_var3
                                   {-0.6, 0.6, 0.2, 0.2, 1.0, 1.0},      // _eq_var1
                                   {-0.8, 0.8, 0.2, 0.2, 1.0, 1.0},      // _eq_var2
                                   {-1.0, 1.0, 0.2, 0.2, 1.0, 1.0}};     // _eq_var3
    const double* t = T[variant];
    const double z1 = (a - t[0]) / t[2], z2 = (a - t[1]) / t[3];
    const double modal1 = t[4] * exp(-0.5 * (z1 * z1));
    const double modal2 = t[5] * exp(-0.5 * (z2 * z2));
    return modal1 + modal2;
}
// state' = state + a (not clipped), reward of the ACTION, always done
__device__ inline double bimodal1d_step(int variant, double* sim, const float* action) {
    const double a = (double)action[0];
    sim[0] = sim[0] + a;
    return bimodal1d_reward(variant, a);
}

// ---- Bimodal2DEnv ---------------------------------------------------------------------------------
// state' = clip(state + a, -6, 6); reward = 125 mixture(state') - 2; done within sqrt(0.5) of (-4,-4) or (4,4)
__device__ inline int bimodal2d_step(double* sim, const float* action, double* reward) {
#pragma clang fp contract(off)
    const double stddev = 2.25, coeff1 = 0.5, coeff2 = 1 - coeff1;
    const double x = fmin(fmax(sim[0] + (double)action[0], -6.0), 6.0);
    const double y = fmin(fmax(sim[1] + (double)action[1], -6.0), 6.0);
    sim[0] = x; sim[1] = y;
    const double xa = (x - -4.0) / stddev, ya = (y - -4.0) / stddev, xb = (x - 4.0) / stddev, yb = (y - 4.0) / stddev;
    const double modal1 = coeff1 * 1.0 / (2 * RLC_PI * (stddev * stddev)) * exp(-0.5 * (xa * xa + ya * ya));
    const double modal2 = coeff2 * 1.0 / (2 * RLC_PI * (stddev * stddev)) * exp(-0.5 * (xb * xb + yb * yb));
    *reward = 125 * (modal1 + modal2) - 2;
    const double ax = fabs(-4.0 - x), ay = fabs(-4.0 - y), bx = fabs(4.0 - x), by = fabs(4.0 - y);
    return (ax * ax + ay * ay <= 0.5) || (bx * bx + by * by <= 0.5);
}

__device__ inline bool rlc_env_is_bimodal1d(int env_id) {
    return env_id >= RLC_ENV_BIMODAL1D && env_id <= RLC_ENV_BIMODAL1D_EQ_VAR3;
}

__device__ inline void env_reset(int env_id, double* sim, double* obs, unsigned long long key, unsigned long long ctr) {
    if (env_id == RLC_ENV_PENDULUM) {
        pendulum_reset(sim, key, ctr);
        pendulum_obs(sim, obs);
    } else if (env_id == RLC_ENV_BIMODAL2D) {
        sim[0] = 0.0; sim[1] = 0.0;
        obs[0] = 0.0; obs[1] = 0.0;
    } else {                                              // the 1-D family starts at 0
        sim[0] = 0.0;
        obs[0] = 0.0;
    }
}
// one simulator step: reward out, obs <- next observation, returns 1 when the environment reports done
__device__ inline int env_step(int env_id, double* sim, const float* action, double* obs, double* reward,
                               int ep_step, int limit) {
    if (env_id == RLC_ENV_PENDULUM) {
        *reward = pendulum_step(sim, action);
        pendulum_obs(sim, obs);
        return ep_step >= limit;                          // gym.wrappers.TimeLimit
    }
    if (env_id == RLC_ENV_BIMODAL2D) {
        const int done = bimodal2d_step(sim, action, reward);
        obs[0] = sim[0]; obs[1] = sim[1];
        return done;
    }
    *reward = bimodal1d_step(env_id - RLC_ENV_BIMODAL1D, sim, action);
    obs[0] = sim[0];
    return 1;
}

// Episode start of the training environment (run_episode_train: env.reset(), experiment.py:103-107); thread 0 only.
__device__ inline void rlc_env_begin_episode(const RlcReplayDev& rep, const RlcEnvDev& env, int agent) {
    double* sim = env.sim + (size_t)agent * RLC_ENV_STATE;
    double* obs = env.obs + (size_t)agent * rep.S;
    const unsigned long long c = env.reset_ctr[agent];
    env_reset(env.env_id, sim, obs, rep.seed[agent] ^ RLC_KEY_ENV_TRAIN, c);
    env.reset_ctr[agent] = c + 1;
    env.ep_step[agent] = 0;
    env.ep_ret[agent] = 0.0;
}

// env.step(action) -> BaseAgent.update (store unless truncated, gamma_i = 0 at terminals) -> bookkeeping; thread 0
// only.  Returns 1 when learn() would run (size > max(warmup, batch), agents/base_agent.py:65-70).
// Episode rules (experiment.py:102-135): `done` at the step limit is truncated -- not stored -- except in the
// Bimodal1DEnv family, whose single step is always stored with gamma 0 (experiment.py:122-125); `done` before the
// limit is stored with gamma 0; the limit without `done` is stored with gamma and ends the episode.  In that last
// case the reference still draws one action (agent.step) and discards it: need_reset = 2 tells the next train
// step to skip one draw of the agent's exploration stream.
__device__ inline int rlc_env_advance_store(const RlcReplayDev& rep, const RlcEnvDev& env, int agent, const float* act) {
    const int S = rep.S, A = rep.A;
    double* sim = env.sim + (size_t)agent * RLC_ENV_STATE;
    double* obs = env.obs + (size_t)agent * S;
    const int step = env.ep_step[agent] + 1;
    double s_prev[8], reward;
    for (int i = 0; i < S && i < 8; i++) s_prev[i] = obs[i];
    const int done = env_step(env.env_id, sim, act, obs, &reward, step, env.episode_limit);
    const double ret = env.ep_ret[agent] + reward;
    const int at_limit = step == env.episode_limit;
    const int truncated = done && at_limit && !rlc_env_is_bimodal1d(env.env_id);
    RlcRingMeta m = rep.ring[agent];
    if (!truncated) {
        const long long cap = rep.cap;
        long long slot = m.start + m.size;
        if (slot >= cap) slot -= cap;
        if (m.size == cap) m.start = (m.start + 1 == cap) ? 0 : m.start + 1;
        else m.size += 1;
        const size_t at = (size_t)agent * cap + slot;
        for (int i = 0; i < S; i++) {
            rep.rs[at * S + i] = (float)s_prev[i];
            rep.rs2[at * S + i] = (float)obs[i];
        }
        for (int j = 0; j < A; j++) rep.ra[at * A + j] = act[j];
        rep.rr[at] = reward;
        rep.rg[at] = done ? 0.0 : env.gamma;
        rep.ring[agent] = m;
    }
    env.total_steps[agent] += 1;
    env.ep_step[agent] = step;
    env.ep_ret[agent] = ret;
    if (done || at_limit) {
        const int e = env.n_train_ep[agent];
        if (e < env.max_episodes) {
            env.train_ret[(size_t)agent * env.max_episodes + e] = ret;
            env.train_len[(size_t)agent * env.max_episodes + e] = step;
            env.train_cum[(size_t)agent * env.max_episodes + e] = env.total_steps[agent];
        }
        env.n_train_ep[agent] = e + 1;
        env.need_reset[agent] = done ? 1 : 2;
    } else {
        env.need_reset[agent] = 0;
    }
    __threadfence();                                   // the replay slot is read back by this workgroup's gather
    return m.size > env.learn_threshold ? 1 : 0;
}

#endif  // __HIPCC__
