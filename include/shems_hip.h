/*
 * shems_hip.h -- C ABI of libshems_hip.so: the batched, MI355X-native (gfx950)
 * replacement for the hot path of the reference
 *   RL-SHEMS/RL_environments/envs/shems_LU1.jl        (LU1, the environment)
 *   RL-SHEMS/algorithms/DDPG.jl                        (DDPG.jl, act/replay/episode!)
 *   RL-SHEMS/src/memory_plotting_saving.jl             (MPS, replay buffer + normalisation)
 *
 * The reference has no FFI today: LU1 extends the Reinforce.jl generics
 * `reset!/step!/action/finished` on `Shems <: AbstractEnvironment` (LU1:62-65,169).
 * Each entry point below names the reference method it replaces; the Julia
 * `ccall` stubs a maintainer would add are in INTEGRATION.md, and the Python
 * `ctypes` mirror used by this repo's tests is the package's `_capi.py`.
 *
 * Conventions
 *   - plain C types only; every function returns SHEMS_OK (0) or a negative error
 *     code, and shems_last_error() returns a thread-local message.
 *   - "host" pointers are ordinary CPU memory; "dev" pointers are HIP device memory.
 *   - row / step indices are 1-based at this boundary, exactly as in the Julia code.
 *   - observation layout is [N][9] float32 = Julia's 9xN column-major Matrix{Float32}
 *     (state order LU1:101-111: Soc_b, Soc_ev, c_ev, d_e, g_e, p_buy, h_cos, h_sin, season).
 *   - a table is [nrow][8] float32: h_countdown, soc_ev, electkwh, PV_generation,
 *     p_buy, hour_cos, hour_sin, season  (the columns LU1:251-260 / 268-279 read).
 *   - `stream` arguments are a hipStream_t passed as void* (NULL = the legacy default stream).
 */
#ifndef SHEMS_HIP_H
#define SHEMS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHEMS_ABI_VERSION 1

enum {
    SHEMS_OK          =  0,
    SHEMS_ERR_ARG     = -1,  /* bad argument (NULL, size, range)                                   */
    SHEMS_ERR_HIP     = -2,  /* a HIP runtime call failed                                           */
    SHEMS_ERR_INDEX   = -3,  /* table access out of range: Julia BoundsError (LU1:227,239,265-279) */
    SHEMS_ERR_NOMEM   = -4,
    SHEMS_ERR_NODEVICE= -5,  /* no gfx950 device visible: the library never falls back to the CPU   */
    SHEMS_ERR_STATE   = -6   /* call order (tables/configs not set, not reset)                      */
};

enum { SHEMS_NSTATE = 9, SHEMS_NACTION = 2, SHEMS_NCOL = 8, SHEMS_NRESULT = 23 };

/* track modes of step!(env, s, a; track) (LU1:343-354, 466-484) */
enum {
    SHEMS_TRACK_OFF   = 0,   /* track == 0 : a = SoC targets in [0,1]                               */
    SHEMS_TRACK_DRL   = 1,   /* track  > 0 : same, plus the 23-column results row (LU1:476-478)     */
    SHEMS_TRACK_RULE  = -1   /* track  < 0 : a = kWh set-points (B, EV); penalty forced to 0        */
};

/* One "config" = what the reference spreads over module globals and env.path:
 * charger capacities (LU1:47-59), Battery/EV/Market constants (LU1:92-99), reward weights
 * (LU1:40-43; per-env in the discomfort-weight sweep) and the input table (env.path, LU1:176). */
typedef struct shems_config {
    float   cap_ev;          /* ev.soc_max  [kWh]   capacities[id][1]                               */
    float   soc_max;         /* b.soc_max   [kWh]   capacities[id][2] (an f32 product, e.g. 7.5f0*0.9f0) */
    double  rate_max;        /* b.rate_max  [kW]    capacities[id][3] (Float64)                     */
    double  disc_weight;     /* m.discomfort_weight_ev = Float64(DISCOMFORT_WEIGHT_EV::Float32)     */
    double  disc_pot;        /* m.disc_pot             = Float64(DISC_POT::Float32)                 */
    float   penalty_weight;  /* penalty_weight::Float32 (LU1:43)                                    */
    int32_t table_row0;      /* 0-based first row of this config's table in the uploaded row array  */
    int32_t nrow;            /* nrow(df) of that table                                              */
    int32_t reserved;
} shems_config;              /* 48 bytes */

typedef struct shems_env shems_env;      /* opaque: N parallel Shems instances on one GPU */

/* ------------------------------------------------------------------ library -- */
int         shems_abi_version(void);
const char *shems_last_error(void);
int         shems_device_count(int *out_count);

/* ------------------------------------------------- handle API (host arrays) -- */
/* Shems(maxsteps, path) x n_envs (LU1:203; called from input.jl:162-164).  Selects `device`
 * (the reference: CUDA.device!(GPU_ID), DDPG_reinforce_charger_v1.jl:12-14). */
int shems_create(int64_t n_envs, int32_t maxsteps, int device, shems_env **out);
int shems_destroy(shems_env *env);
int shems_n_envs(const shems_env *env, int64_t *out);

/* Replaces CSV.read(env.path, DataFrame) (LU1:217, 265): all tables, concatenated row-wise,
 * are uploaded once.  rows = [total_rows][8] float32 host memory. */
int shems_set_tables(shems_env *env, const float *rows, int64_t total_rows);
/* Replaces the module globals LU1:40-59, 92-99.  cfg_of_env = [n_envs] host indices into cfgs
 * (NULL: every env uses cfgs[0]). */
int shems_set_configs(shems_env *env, const shems_config *cfgs, int32_t n_cfg,
                      const uint16_t *cfg_of_env);

/* reset!(env; rng) (LU1:206-262).  rng_minus1 != 0  <=>  rng == -1: Soc_b = 0.5*(soc_min+soc_max),
 * idx = 1.  Otherwise the two MersenneTwister draws are inputs: idx0[i] in 1..(nrow-maxsteps)
 * (1-based) and soc_b0[i]; the episode-extension loop LU1:227-246 runs on the device. */
int shems_reset(shems_env *env, int rng_minus1, const int32_t *idx0, const float *soc_b0);
/* Same, with both draws taken from the library's counter-based generator (Philox4x32-10):
 * idx0 = 1 + x0 mod (nrow-maxsteps), soc_b0 = float(x1 >> 8) * 2^-24 * soc_max,
 * (x0,x1,..) = philox(key = seed, counter = (env index, episode, 0, 0)). */
int shems_reset_seeded(shems_env *env, uint64_t seed, uint32_t episode);

/* step!(env, s, a; track) (LU1:343-485).  actions = [n][2] host float32.  Outputs (each may be
 * NULL): rewards [n] Float64, obs [n][9] (= Vector{Float32}(env.state)), results [n][23] Float64
 * (column order LU1:476-478; written for every track_mode if non-NULL).
 * Returns SHEMS_ERR_INDEX (and steps no env past the table) if any env has idx+1 > nrow. */
int shems_step(shems_env *env, const float *actions, int track_mode,
               double *rewards, float *obs, double *results);

/* action(env, a::ShemsAction) (LU1:283-316): targets [n][2] -> kWh set-points [n][2] (B, EV). */
int shems_action(shems_env *env, const float *targets, float *out_b_ev);
/* action(env, track) (LU1:318-340), the rule-based controller -> [n][2] (B, EV). */
int shems_rule_action(shems_env *env, float *out_b_ev);
/* finished(env, s') (LU1:487-502): always false; done = [n] bytes. */
int shems_finished(shems_env *env, uint8_t *done);

/* inference(env; track != 0) (memory_plotting_saving.jl:62-89): the whole tracking pass -- `nsteps` hours from the envs' current
 * state (call shems_reset(env, 1, NULL, NULL) first, as episode!(...; rng_ep = -1) does) -- in ONE launch, host arrays in and out:
 * track_mode > 0: the deterministic actor (`actor` = the 129002 parameters in Flux.params order, s_min / s_max [9]); track_mode < 0:
 * the rule-based controller (actor / s_min / s_max may be NULL).  results [nsteps][23] Float64 receives the rows of env 0
 * (shems_LU1.jl:476-478), returns [n_envs] the summed rewards (DDPG.jl:223); either may be NULL.  SHEMS_ERR_INDEX if the pass
 * runs off the table (Julia: BoundsError).  The device-pointer form, with one actor per env, is shems_track_dev. */
int shems_track(shems_env *env, const float *actor, const float *s_min, const float *s_max, int track_mode, int32_t nsteps,
                double *results, double *returns);

/* env.state / env.idx / env.step accessors (LU1:169-177).  Any pointer may be NULL. */
int shems_get_state(shems_env *env, float *obs, int32_t *idx, int32_t *step);
int shems_set_state(shems_env *env, const float *obs, const int32_t *idx, const int32_t *step);

/* ----------------------------------------- device-pointer (zero-copy) API -- */
/* Device views of a handle, for chaining with the policy / DDPG kernels without host copies. */
typedef struct shems_view {
    int64_t  n_envs;
    int32_t  maxsteps;
    int32_t  n_cfg;
    float   *obs;            /* dev [n][9]                         */
    int32_t *idx;            /* dev [n]   1-based row index        */
    int32_t *step;           /* dev [n]                            */
    const uint16_t     *cfg_of_env;   /* dev [n]                   */
    const shems_config *cfgs;         /* dev [n_cfg]               */
    const float        *tables;       /* dev [total_rows][8]       */
    int64_t  total_rows;
    int32_t *err;            /* dev [1]: sticky error word (SHEMS_ERR_*) set by kernels */
} shems_view;
int shems_get_view(shems_env *env, shems_view *out);
int shems_set_stream(shems_env *env, void *stream);     /* stream used by the handle API         */
int shems_check_error(shems_env *env);                  /* syncs, reads + clears view.err          */

/* step! on device buffers.  d_actions [n][2]; optional outputs: d_rewards [n] Float64,
 * d_rewards_f32 [n] (the Float32 the replay buffer keeps, MPS:37 + gpu()), d_results [n][23],
 * d_block_reward [ceil(n/256)] per-workgroup reward sums (wavefront reduction). */
int shems_step_dev(const shems_view *v, const float *d_actions, int track_mode,
                   double *d_rewards, float *d_rewards_f32, double *d_results,
                   double *d_block_reward, void *stream);
int shems_action_dev(const shems_view *v, const float *d_targets, int rule_based,
                     float *d_out_b_ev, void *stream);
int shems_reset_dev(const shems_view *v, int rng_minus1, const int32_t *d_idx0,
                    const float *d_soc_b0, void *stream);
int shems_reset_seeded_dev(const shems_view *v, uint64_t seed, uint32_t episode, void *stream);

/* Whole-episode rollout without host round trips: `nsteps` x { a = policy; step! } in ONE launch,
 * env state held in registers.  policy = SHEMS_ROLLOUT_RULE: a = action(env, track), track < 0
 * (BASELINE config 1 at scale, MPS:62-71 + DDPG.jl:209-212); SHEMS_ROLLOUT_RANDOM: uniform random
 * actions in [-1,1] -> scale_action (populate_memory, MPS:9-29), Philox keyed by (seed, env, step).
 * d_returns [n] Float64 episode sums (DDPG.jl:223).  If ring != NULL every transition is appended
 * of the first `ring_envs` envs (0 = all) is appended to the replay ring (see shems_replay below) at
 * slot (ring_pos + env*nsteps + t) mod capacity, i.e. in the reference's episode-major push order;
 * pushes that a later push of the same launch would overwrite (order < ring_envs*nsteps - capacity)
 * are skipped, so the ring content is deterministic (= what the CircularBuffer would hold). */
enum { SHEMS_ROLLOUT_RULE = 0, SHEMS_ROLLOUT_RANDOM = 1 };
struct shems_replay;
int shems_rollout_dev(const shems_view *v, int policy, int32_t nsteps, uint64_t seed,
                      double *d_returns, const struct shems_replay *ring, int64_t ring_pos,
                      int64_t ring_envs, void *stream);

/* ------------------------------------------------------------ replay ring -- */
/* memory = CircularBuffer{Any}(MEM_SIZE) of [s, a, r, s', done] (input.jl:139-140, MPS:46-47),
 * kept in HBM as struct-of-arrays.  `a` is the UNSCALED policy output in [-1,1] (DDPG.jl:229). */
typedef struct shems_replay {
    int64_t  capacity;       /* MEM_SIZE                                   */
    float   *s;              /* dev [capacity][9]                          */
    float   *a;              /* dev [capacity][2]                          */
    float   *r;              /* dev [capacity]    Float32(reward)          */
    float   *s2;             /* dev [capacity][9]                          */
    uint8_t *done;           /* dev [capacity]                             */
} shems_replay;              /* the push position is host state and is passed by value */


/* ------------------------------------------------------- policy (actor) -- */
/* Network parameters are ONE flat float32 device array per network in Flux's own order and
 * layout (Flux.params(Chain(Dense, Dense, Dense)) = W1, b1, W2, b2, W3, b3 with each W a
 * column-major out x in Matrix, DDPG.jl:30-46):
 *   actor  (9 -> 250 -> 500 -> 2, relu, relu, tanh):  W1[9][250] b1[250] W2[250][500] b2[500] W3[500][2] b3[2]  = 129 002
 *   critic (11 -> 250 -> 500 -> 1, relu, relu, id):   W1[11][250] b1[250] W2[250][500] b2[500] W3[500][1] b3[1] = 129 001
 * ([k][n] = C order of the Julia out x in column-major matrix: the out index is contiguous). */
enum { SHEMS_L1 = 250, SHEMS_L2 = 500, SHEMS_ACTOR_PARAMS = 129002, SHEMS_CRITIC_PARAMS = 129001 };

typedef struct shems_act_params {
    const float *actor;      /* dev [129002]                                                        */
    const float *s_min;      /* dev [9]  normalize(): (s - s_min) / (s_max - s_min + 1f-8), MPS:55-57 */
    const float *s_max;      /* dev [9]                                                             */
    float    noise_mu;       /* gn = GNoise(mu, sigma_act, .) / ou = OUNoise(mu, sigma, theta, dt, X)  input.jl:190-237 */
    float    noise_sigma;
    int32_t  train;          /* act(...; train): 1 = explore (DDPG.jl:151-172)                      */
    uint32_t tick;           /* counter word of the noise stream (the reference's rng_step, DDPG.jl:197) */
    uint64_t seed;           /* Philox key                                                          */
    int32_t  noise_kind;     /* SHEMS_NOISE_*: which branch of act() (noise_type "gn" / "ou" / "en") */
    float    ou_theta;       /* OUNoise theta                                                       */
    float    ou_dt;          /* OUNoise dt (1f-2)                                                   */
    float    eps;            /* EpsNoise: current xi = max(0.5 - zeta*(episode - MEM/EP), xi_min), DDPG.jl:69-72 */
    float   *ou_state;       /* dev [n][2]: OUNoise.X per env (persistent, DDPG.jl:49-55); required for SHEMS_NOISE_OU */
    float   *noise_acc;      /* dev [n] or NULL: += act()'s second return value for this step (DDPG.jl:148-176): mean(noise) of the
                              * two action noise samples (gn, ou), mean(|act_pred - act_uni|) when an epsilon step explores, else 0 */
} shems_act_params;
/* act()'s exploration branches (DDPG.jl:148-176).  GAUSS: clamp(a + N(mu, sigma)); OU: X += theta(mu - X)dt +
 * sigma sqrt(dt) N(0,1), clamp(a + X); EPS: with probability eps a uniform action in [-1,1]^2, else the
 * unperturbed a (returned unclamped by the reference -- tanh already bounds it). */
enum { SHEMS_NOISE_GAUSS = 0, SHEMS_NOISE_OU = 1, SHEMS_NOISE_EPS = 2 };

/* Which transitions of a vector step enter the replay ring: envs i with ((i - offset) mod n) < count
 * are stored at slot (pos + ((i - offset) mod n)) mod capacity.  count = 0 stores nothing. */
typedef struct shems_ring_window {
    int64_t pos;
    int64_t count;
    int64_t offset;
} shems_ring_window;

/* act(): a = clamp(actor(normalize(s)) + noise, -1, 1) for m observations (DDPG.jl:148-176).
 * d_obs [m][9] -> d_a [m][2] (UNSCALED action in [-1, 1]).  fp32 MFMA (v_mfma_f32_32x32x2_f32). */
int shems_actor_forward_dev(const shems_act_params *p, const float *d_obs, int64_t m, float *d_a,
                            void *stream);

/* One fused vector step of episode! (DDPG.jl:195-234) for every env of the view, in ONE launch:
 *   s = env.state; a = act(normalize(s)); step!(env, s, scale_action(a)); remember(s, a, r, s', false).
 * Optional outputs: d_a [n][2] unscaled actions, d_rewards [n] f64, d_rewards_f32 [n],
 * d_block_reward [grid] per-workgroup reward sums, d_returns_acc [n] f64 += reward (reward_eps, DDPG.jl:223).  ring/window may be NULL (evaluation episodes). */
int shems_act_step_dev(const shems_view *v, const shems_act_params *p, float *d_a, double *d_rewards,
                       float *d_rewards_f32, double *d_block_reward, double *d_returns_acc,
                       const shems_replay *ring, const shems_ring_window *window, void *stream);
/* The same fused step (DDPG.jl:195-234) for the envs [env_lo, env_lo + env_count) of the view only (the other envs are not touched).  Every env
 * draws its noise from (seed, tick, ITS index in the view) and the ring window is still defined on the whole batch, so stepping a
 * batch range by range -- in any order, on any streams -- leaves the same bytes as one shems_act_step_dev over the view.  The training
 * loop's order-exact pipelined mode steps the window's envs first with it (shems_train_steps). */
int shems_act_step_range_dev(const shems_view *v, const shems_act_params *p, int64_t env_lo, int64_t env_count, float *d_rewards_f32,
                             const shems_replay *ring, const shems_ring_window *window, void *stream);
/* scale_action (DDPG.jl:178-184) on device: d_a [n][2] in [-1,1] -> d_out [n][2] SoC targets in [0,1]. */
int shems_scale_action_dev(const float *d_a, int64_t n, float *d_out, void *stream);
/* The kernel that shems_act_step_dev (grouped = 0) or else shems_act_step_group_dev dispatches for n_envs envs, by the name a
 * profiler shows (e.g. "shems::k_act2", "shems::k_actg<1, 8, 1, 3>"), NUL-terminated into out[cap]: bench.py's roofline.kernel. */
int shems_act_step_kernel(int64_t n_envs, int grouped, char *out, int32_t cap);
/* The same for a learner group of envs_per_learner households per learner (a tile never straddles two learners; tiled != 0: the group's
 * W2 is read from its tiled regions, t != NULL). */
int shems_act_step_group_kernel(int64_t n_envs, int64_t envs_per_learner, int tiled, char *out, int32_t cap);
/* Number of workgroups shems_act_step_dev launches for n envs (length of d_block_reward). */
int shems_act_step_grid(int64_t n_envs, int64_t *out_blocks);

/* inference(env; track != 0) (memory_plotting_saving.jl:62-89 -> episode!(env; train = false, track, rng_ep = -1), DDPG.jl:186-242;
 * 80 such passes per job, DDPG_reinforce_charger_v1.jl:87-105) as ONE launch: every env of the view runs `nsteps` hours from
 * its current state (reset it first: shems_reset_dev(rng_minus1 = 1)), one workgroup per env, no host round trip per hour:
 *   track_mode > 0: a = scale_action(actor(normalize(s)))   -- the deterministic actor (act(...; train = false), DDPG.jl:148-184)
 *   track_mode < 0: a = action(env, track)                  -- the rule-based controller (shems_LU1.jl:318-340)
 * then step!(env, s, a; track) (shems_LU1.jl:343-485).  Env e uses the actor / s_min / s_max at p's pointers + e * actor_stride_bytes
 * (0: one actor for every env; a learner-group slab stride: 40 seeds x {last, best} in one launch); p may be NULL for track < 0.
 * d_results: the 23-column rows of shems_LU1.jl:476-478, [n_envs][nsteps][23] Float64 (results_env = -1) or [nsteps][23] of env
 * `results_env` only, or NULL.  d_returns [n_envs]: sum of rewards (DDPG.jl:223), or NULL.  The layers are tolerance-class
 * arithmetic (as shems_act_step_dev); step! is exact. */
int shems_track_dev(const shems_view *v, const shems_act_params *p, int64_t actor_stride_bytes, int track_mode, int32_t nsteps,
                    double *d_results, int64_t results_env, double *d_returns, void *stream);


/* -------------------------------------------------------- DDPG update -- */
/* replay() (DDPG.jl:121-145).  Batch <= 128 (BATCH_SIZE = 120 in the tuned config).  All pointers are device memory;
 * `ws` is a scratch block of shems_ddpg_workspace_floats() floats (zero it once).
 *
 * Single replica: shems_ddpg_update runs the whole function in five dependent launches (csrc/shems_ddpg.hip):
 *   getData (sample WITH replacement, MPS:31-42) -> normalize -> a' = actor_target(s'), q' = critic_target([s';a']),
 *   y = r + gamma(1-done)q' -> update_model!(critic, opt_crit, loss_crit, y, s, a) -> update_model!(actor, opt_act,
 *   loss_act, s) -> soft_update!(actor_target, actor), soft_update!(critic_target, critic).
 * ADAM and the soft target update of an element are applied by the workgroup that produced its gradient.
 *
 * Data-parallel replicas exchange gradients at two points; for them the same function is split there:
 *   shems_ddpg_critic_grad : ... -> d mse(critic([s;a]), y) / d critic  into grad_critic [129001]
 *   (all-reduce grad_critic across replicas here)
 *   shems_ddpg_critic_apply: ADAM(eta_crit) on critic, then soft_update!(critic_target, critic; tau)
 *   shems_ddpg_actor_grad  : d(-mean(critic([s; actor(s)]))) / d actor  into grad_actor [129002]
 *   (all-reduce grad_actor here)
 *   shems_ddpg_actor_apply : ADAM(eta_act) on actor, then soft_update!(actor_target, actor; tau)
 * Both forms run the same gradient kernels and the same ADAM arithmetic: with grad_scale = 1 they produce the same bits.
 * ADAM is Flux 0.12.1's: m,v float32 arrays, scalars in Float64, bias-correction powers beta^t are
 * host state passed by value (bp1 = beta1^t, bp2 = beta2^t for the t-th step, t >= 1). */
typedef struct shems_ddpg {
    float *actor, *critic, *actor_t, *critic_t;     /* [129002] [129001] [129002] [129001]        */
    float *m_actor, *v_actor, *m_critic, *v_critic; /* ADAM moments                                */
    float *grad_actor, *grad_critic;                /* gradient outputs (sum over the local batch / batch) */
    const float *s_min, *s_max;                     /* [9]                                         */
    float *ws;                                      /* workspace                                   */
    float *losses;                                  /* [2] out: critic mse, actor loss (-mean q)   */
    float gamma, tau;
    int32_t batch;                                  /* BATCH_SIZE (<= 128)                         */
    int32_t flags;                                  /* SHEMS_DDPG_* bits (0 = default)             */
} shems_ddpg;

/* flags: DEFER_ACTOR_E -- split form only: shems_ddpg_critic_grad leaves the actor's two E products (independent of the critic
 * update) out of its second launch; the caller issues them with shems_ddpg_actor_prepare between shems_ddpg_critic_grad and
 * shems_ddpg_actor_grad, typically right after starting the asynchronous all-reduce of grad_critic, so that they run under it. */
enum { SHEMS_DDPG_DEFER_ACTOR_E = 1 };

int shems_ddpg_workspace_floats(int64_t *out);
/* The whole replay() for one replica.  grad_actor / grad_critic still receive the complete gradients.  excl_pos / excl_count:
 * as shems_ddpg_critic_grad_ex (0, 0 = none).  d_publish: optional second copy [129002] of the updated actor (see
 * shems_ddpg_actor_apply_pub), or NULL. */
int shems_ddpg_update(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                      int64_t excl_pos, int64_t excl_count, double eta_crit, double bp1_crit, double bp2_crit,
                      double eta_act, double bp1_act, double bp2_act, float *d_publish, void *stream);
int shems_ddpg_critic_grad(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len,
                           uint64_t seed, uint32_t tick, void *stream);
/* Pipelined variant for running replay() on a second stream WHILE the fused act/step kernel of the same vector step
 * inserts into the ring: slots [excl_pos, excl_pos + excl_count) (mod capacity) -- the window being written -- are
 * excluded from sampling, i.e. the minibatch is drawn from the buffer as it stood before this step's inserts.
 * excl_count = 0 is shems_ddpg_critic_grad. */
int shems_ddpg_critic_grad_ex(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len,
                              uint64_t seed, uint32_t tick, int64_t excl_pos, int64_t excl_count, void *stream);
int shems_ddpg_actor_prepare(const shems_ddpg *d, void *stream);   /* see SHEMS_DDPG_DEFER_ACTOR_E */
int shems_ddpg_critic_apply(const shems_ddpg *d, double eta, double bp1, double bp2, double grad_scale,
                            void *stream);
int shems_ddpg_actor_grad(const shems_ddpg *d, void *stream);
int shems_ddpg_actor_apply(const shems_ddpg *d, double eta, double bp1, double bp2, double grad_scale,
                           void *stream);
/* Same, and also writes the updated actor into d_publish [129002] (a second copy the policy kernel of the NEXT
 * vector step reads while this stream already works on the next update). */
int shems_ddpg_actor_apply_pub(const shems_ddpg *d, double eta, double bp1, double bp2, double grad_scale,
                               float *d_publish, void *stream);
/* One SUPERVISED update of the actor on demonstrations (behaviour cloning; the reference has no such step):
 *   loss = Flux.mse(actor(normalize(s)), a_demo), the mean over the 2 * batch elements,
 * on a minibatch the ordinary sampler draws from `ring` (shems_ddpg_sample_indices predicts the slots), of which only s and a are
 * read.  Three dependent launches (csrc/shems_ddpg.hip): the actor's forward pass with the gather, the actor's two E products, and
 * the actor's gradient launch with the cloning head, d3[o][m] = (a_pi - a_demo) (1 - a_pi^2) / batch; ADAM and the soft update of
 * actor_t ride in the gradient launch as in shems_ddpg_update (tau = 1 keeps actor_t equal to actor: 1 p + 0 t).  grad_actor
 * receives the complete gradient and losses[1] the loss; the critic, its target, its moments, grad_critic and losses[0] are not
 * touched.  Arguments and validation as shems_ddpg_update's for the actor. */
int shems_ddpg_clone_update(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                            double eta, double bp1, double bp2, float *d_publish, void *stream);
/* One CRITIC-ONLY update (policy evaluation): update_model!(critic, ...) and soft_update!(critic_target, critic) of DDPG.jl:131-137
 * and 143, in three launches of the update's own kernels -- the first without the actor's forward job, the second without the actor's
 * two E products, the third the critic's gradient with ADAM and the soft update inside.  actor, actor_t, m_actor, v_actor, grad_actor
 * and losses[1] are not touched.  From the same state, ring, seed and tick it leaves the bits of shems_ddpg_critic_grad followed by
 * shems_ddpg_critic_apply(grad_scale = 1) in critic, critic_t, m_critic, v_critic, grad_critic and losses[0].  Arguments and
 * validation as shems_ddpg_update's for the critic. */
int shems_ddpg_critic_update(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                             double eta, double bp1, double bp2, void *stream);
/* ------------------------------------------------------------ TD3 update -- */
/* One update of TD3 (Fujimoto, van Hoof, Meger 2018: twin critics, target-policy smoothing, delayed actor) in this library's
 * conventions: Float32 arithmetic, Flux 0.12.1 ADAM, the order of replay() (DDPG.jl:121-145), the minibatch of
 * shems_ddpg_sample_indices(seed, tick).  The reference carries the hyper-parameter (noise_trg = 0.2f0, input.jl:231) and no algorithm
 * file; the definition is this one:
 *   1. gather and normalise the minibatch as replay() does (columns m >= batch are padding and enter no sum);
 *   2. (z0, z1)[m] = Box-Muller on words x, y of the Philox4x32-10 block at counter (m, 0, tick, 0x5452474E), key seed (the act
 *      noise's transform on a stream tag of its own); eps = clamp(sigma_trg z, -clip_trg, clip_trg);
 *      a~' = clamp(actor_t(s'_n) + eps, -1, 1);
 *   3. q'_i = critic_i_t([s'_n; a~']), y = r + gamma (1 - done) min(q'_1, q'_2) -- one y for both critics;
 *   4. each critic i: gradient of Flux.mse(critic_i([s_n; a]), y), ADAM(eta_crit) with its own moments and the shared powers;
 *      losses[0] and losses2[0] receive the two mse values;
 *   5. update_policy = 1: the actor's gradient of -mean(critic_1([s_n; actor(s_n)])) through the UPDATED critic 1 (DDPG.jl:137-140),
 *      ADAM(eta_act), losses[1]; soft updates of actor_t, critic_t and critic2_t with tau.
 *      update_policy = 0: actor, actor_t, m_actor, v_actor, grad_actor and losses[1] are not touched, and both critic targets keep
 *      their values (the soft update runs with tau = 0: 1 t + 0 p).
 * The beta powers are host state as for shems_ddpg_update: the critics' advance on every update, the actor's on policy steps.
 * `d` is the learner exactly as shems_ddpg_update takes it (actor + critic 1, Flux order); the second critic has blocks of its own
 * [129001], which must not overlap critic 1's.  ws2: shems_td3_workspace_floats() floats, zeroed once; after an update it begins
 * with a~' [2][128], y [128], q'_1 [128], q'_2 [128].  Three dependent launches, five on a policy step (csrc/shems_ddpg.hip).
 * SHEMS_ERR_ARG, nothing launched: whatever shems_ddpg_update refuses; a NULL, misaligned or overlapping critic-2 buffer; sigma_trg or
 * clip_trg negative or not finite; update_policy outside {0, 1}.  SHEMS_ERR_STATE: a learner between shems_ddpg_tiled_enter and
 * shems_ddpg_tiled_leave.  With sigma_trg = 0 and critic 2 a copy of critic 1, update_policy = 1 leaves shems_ddpg_update's bits. */
typedef struct shems_td3 {
    shems_ddpg d;                                   /* actor + critic 1, as for shems_ddpg_update                     */
    float *critic2, *critic2_t;                     /* [129001] each                                                 */
    float *m_critic2, *v_critic2, *grad_critic2;    /* [129001] each                                                 */
    float *ws2;                                     /* shems_td3_workspace_floats() floats, zeroed once              */
    float *losses2;                                 /* [1] out: mse of critic 2                                      */
    float sigma_trg, clip_trg;                      /* 0.2 (input.jl:231), 0.5                                       */
} shems_td3;
int shems_td3_workspace_floats(int64_t *out);
int shems_td3_update(const shems_td3 *t, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                     double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act,
                     int update_policy, void *stream);
/* --------------------------- behaviour-regularised actor update (TD3+BC) -- */
/* One update of replay() (shems_ddpg_update) or of TD3 (shems_td3_update) with only the ACTOR's loss changed to the TD3+BC objective
 * (Fujimoto, Gu 2021): the normalised critic value plus a mean-squared pull towards the ring's stored action.  The reference has no
 * such loss; the definition is this one (csrc/shems_bc_core.h holds the scalar arithmetic).  With B = batch, the live
 * columns m < B, a_pi = actor(s_n) as K4 forms it, a = the ring's stored, unscaled action of the minibatch, and
 * q_m = critic([s_n; a_pi])_m through the critic AS UPDATED BY THIS SAME UPDATE (critic 1 for TD3):
 *   1. Qbar = (1/B) sum_{m<B} |q_m|;
 *   2. lambda = normalise ? alpha / max(Qbar, 1e-8f) : alpha -- a constant of the update: no gradient flows through it;
 *   3. loss_act = -lambda mean_m(q_m) + weight Flux.mse(a_pi, a), the mse over the 2 B elements (as shems_ddpg_clone_update has it);
 *   4. at the actor's output, for m < B: d loss / d a_pi[o][m] = lambda da[o][m] + weight (a_pi - a)[o][m] / B, where da is the sum of
 *      K4's 32 partials of d(-mean q) / d a_pi, in the order shems_ddpg_update sums them; pad columns m >= B contribute 0 to both terms
 *      and to Qbar; then through tanh, d3 = (...) (1 - a_pi^2);
 *   5. everything downstream is the actor's gradient launch as it is: every gradient block, ADAM and the soft update of actor_t in the
 *      workgroup that made the gradient, the d_publish copy.  The critic side is untouched.
 * The paper's values are alpha = 2.5, weight = 1, normalise = 1.  With normalise = 0, alpha = 1, weight = 0 the update leaves
 * shems_ddpg_update's (shems_td3_update's) bits; with alpha = 0 it is the cloning gradient on the update's minibatch.
 * The same launches as the plain entry points, the last one replaced by k_grad_bc (csrc/shems_ddpg.hip).
 * out: a 16-byte aligned device buffer of the caller's, SHEMS_BC_OUT_FLOATS = 4 + 128 floats, written by the actor's gradient launch:
 * out[0] = lambda, out[1] = Qbar, out[2] = -mean q, out[3] = mse(a_pi, a), out[4 + m] = q_m (columns >= batch are padding).  losses[1]
 * receives loss_act.  shems_td3_update_bc with update_policy = 0 checks bc and neither reads nor writes out.
 * SHEMS_ERR_ARG, nothing launched: whatever the plain entry point refuses; NULL bc or out; misaligned out; out overlapping ws, ws2,
 * losses, losses2 or a parameter, moment or gradient block; alpha or weight negative or not finite; normalise outside {0, 1};
 * reserved != 0.  SHEMS_ERR_STATE: a learner between shems_ddpg_tiled_enter and shems_ddpg_tiled_leave (the tiled layout has no
 * behaviour-regularised gradient launch). */
#define SHEMS_BC_OUT_FLOATS (4 + 128)
typedef struct shems_bc {
    float alpha, weight;         /* 2.5, 1 (the paper's)                                             */
    int32_t normalise, reserved; /* 1 = lambda = alpha / Qbar; reserved = 0                          */
    float *out;                  /* [SHEMS_BC_OUT_FLOATS] device, 16-byte aligned                    */
} shems_bc;
int shems_ddpg_update_bc(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                         int64_t excl_pos, int64_t excl_count, double eta_crit, double bp1_crit, double bp2_crit,
                         double eta_act, double bp1_act, double bp2_act, float *d_publish, const shems_bc *bc, void *stream);
int shems_td3_update_bc(const shems_td3 *t, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick,
                        double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act,
                        int update_policy, const shems_bc *bc, void *stream);
/* ------------------------------------------- prioritized replay update -- */
/* Prioritized experience replay (Schaul et al. 2016, proportional variant) for the single learner, in replay()'s conventions.  The
 * reference has no such sampler; the definition is this one (csrc/shems_per_core.h states it again with every summation order;
 * DESIGN.md 4p).  A prioritized ring is a shems_replay plus prio [capacity] (pi_j = p_j^alpha >= 0, the power applied) and pmax [1]
 * (the running maximum of every pi ever written; 1.0 at the start, never decreasing).  One update with (alpha, beta, eps_p), the
 * freshly pushed range (fresh_pos, fresh_count) and (seed, tick):
 *   1. the fresh_count slots from fresh_pos (mod capacity) receive pmax[0] before anything is summed; fresh_count >= capacity = all;
 *   2. the slots [0, ring_len) are cut into blocks of 256 (the last zero-padded): S_b = ((s0 + s1) + s2) + s3 over the four chunk sums
 *      of 64 slots, each a balanced pairwise tree; C_b = C_{b-1} + S_b in block order; T = C_last.  No atomics, fixed orders;
 *   3. column m < batch: u_m = (w >> 8) 2^-24 with w = word m & 3 of the Philox4x32-10 block at counter (m >> 2, 0, tick, 0x50455253),
 *      key seed; t_m = (m + u_m) * (T / batch), uncontracted; j_m = the first slot whose running sum exceeds t_m (the first block with
 *      C_b > t_m, then C_{b-1} + pi in slot order inside it; where rounding leaves no such slot, the last slot with pi > 0 of the
 *      block the search ended in), at most ring_len - 1.  Pad columns publish slot -1;
 *   4. w_m = (ring_len pi_{j_m} / T)^(-beta) / max over the live columns (powf: tolerance class; beta = 0 gives exactly 1.0f), pad
 *      columns 0;
 *   5. replay() (DDPG.jl:121-145) on the columns j_m with the critic's head weighted: diff = q - y, dq = 2 w_m diff / batch,
 *      losses[0] = sum w_m diff^2 / batch in head_loss's order; the actor's side, both ADAM steps and the soft updates unchanged;
 *   6. pi_{j_m} <- (|diff_m| + eps_p)^alpha for every live column (the highest column wins a slot drawn twice);
 *      pmax[0] <- max(pmax[0], max_m pi);
 *   7. the beta powers and the tick are host state, as for shems_ddpg_update.
 * Six dependent launches: k_per_sample (steps 1-4, one workgroup), then K1..K5 with K1 and K3 as the instantiations k_fwd_per /
 * k_grad_per, which read the published slots and weights; step 6 rides in k_grad_per's publishing workgroup.
 * ws: shems_per_workspace_floats(capacity) floats; after a draw it holds T, the largest raw weight, the number of blocks (int32), one
 * reserved word, then slots [128] (int32), weights [128], u [128], t [128], S_b [nb], C_b [nb], nb = ceil(ring_len / 256).
 * beta is read on every call, so the host may anneal it. */
typedef struct shems_per {
    float *prio;                 /* [capacity] pi, 16-byte aligned                                   */
    float *pmax;                 /* [1] running maximum, 1.0 at the start                            */
    float *ws;                   /* shems_per_workspace_floats(capacity) floats, 16-byte aligned     */
    float alpha, beta, eps_p;    /* 0.6, 0.4, 1e-6 (the paper's proportional variant)                */
    int32_t reserved;
} shems_per;
int shems_per_workspace_floats(int64_t capacity, int64_t *out);
/* Steps 1-4 alone (tests, a Julia caller).  SHEMS_ERR_ARG as shems_ddpg_update_per's for the ring's own arguments. */
int shems_per_sample_dev(const shems_per *per, int64_t capacity, int64_t ring_len, int64_t fresh_pos, int64_t fresh_count,
                         uint64_t seed, uint32_t tick, int32_t batch, void *stream);
/* Step 5 on slots and weights the caller supplies (d_idx [128] int32, -1 in the pad columns; d_w [128]): no sampler launch, no
 * write-back.  With d_idx = shems_ddpg_sample_indices(seed, tick) and weights of 1.0 it leaves shems_ddpg_update's bits. */
int shems_ddpg_update_given(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, const int32_t *d_idx,
                            const float *d_w, double eta_crit, double bp1_crit, double bp2_crit,
                            double eta_act, double bp1_act, double bp2_act, void *stream);
/* Steps 1-6.  SHEMS_ERR_ARG, nothing launched: whatever shems_ddpg_update refuses; a NULL, misaligned or overlapping prio / pmax /
 * workspace; alpha, beta or eps_p negative or not finite, beta > 1; ring_len outside 1..capacity; capacity above 262144 (the sampler's
 * one workgroup keeps every block sum in LDS); a fresh range that starts outside the ring or, on a ring not yet full, leaves the
 * filled slots.  SHEMS_ERR_STATE: a learner between shems_ddpg_tiled_enter and shems_ddpg_tiled_leave. */
int shems_ddpg_update_per(const shems_ddpg *d, const shems_replay *ring, const shems_per *per, int64_t ring_len,
                          int64_t fresh_pos, int64_t fresh_count, uint64_t seed, uint32_t tick,
                          double eta_crit, double bp1_crit, double bp2_crit,
                          double eta_act, double bp1_act, double bp2_act, void *stream);
/* The minibatch indices of (seed, tick): host helper for tests (same Philox as the device). */
int shems_ddpg_sample_indices(uint64_t seed, uint32_t tick, int32_t batch, int64_t ring_len, int64_t *out);
/* ------------------------------------------ data-parallel replicas -- */
/* One process per GPU, each with its own env shard and ring, one learner replicated: replay() sums the gradients over the replicas at
 * its two exchange points (the reference has no collective: 40 independent processes,
 * RL-SHEMS_bs_scheduler_1179_08_on_01-98.sh:67-87).  shems_dp is one RCCL communicator; its all-reduces are issued IN THE CALLER'S
 * STREAM (no stream of their own, hence no dependency between queues -- 5-10 us each on this stack), RCCL itself is loaded with dlopen
 * at first use.  Rank 0 makes the 128-byte id and hands it to the others by any means (the Python host: torch.distributed broadcast);
 * shems_dp_create is collective (every rank calls it, on its own device). */
enum { SHEMS_DP_ID_BYTES = 128 };
typedef struct shems_dp shems_dp;
int shems_dp_unique_id(char *out128);
int shems_dp_create(const char *id128, int rank, int world, shems_dp **out);
int shems_dp_destroy(shems_dp *dp);
int shems_dp_info(const shems_dp *dp, int *rank, int *world, char *lib, int32_t cap);   /* lib: which librccl was loaded */
int shems_dp_allreduce_sum(shems_dp *dp, float *d_buf, int64_t n, void *stream);        /* in place, float32, in `stream` */
/* replay() of one replica: shems_ddpg_critic_grad_ex, all-reduce(grad_critic), shems_ddpg_critic_apply(grad_scale = 1 / world),
 * shems_ddpg_actor_grad, all-reduce(grad_actor), shems_ddpg_actor_apply_pub -- everything in `stream`.  dp == NULL: a single replica in
 * the split form (the bytes of shems_ddpg_update). */
int shems_ddpg_update_dp(const shems_ddpg *d, const shems_replay *ring, int64_t ring_len, uint64_t seed, uint32_t tick, int64_t excl_pos,
                         int64_t excl_count, double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act,
                         float *d_publish, shems_dp *dp, void *stream);

/* ------------------------------------------------- the training loop -- */
/* The hour loop of episode! (DDPG.jl:195-234) for every env of a view, `k` vector steps enqueued by ONE call:
 *   per step t:  [t > 0 and t % ep_len == 0: episode += 1, reset!(env) with (env_seed, episode)  -- DDPG.jl:189-193]
 *                a = act(normalize(s)); step!(env, s, scale_action(a)); remember(...)               -- shems_act_step_dev
 *                updates_per_step x replay()                                                        -- shems_ddpg_update
 * exactly the calls a host loop over shems_act_step_dev / shems_ddpg_update would make, with the same arguments (the noise tick is
 * t, the ring window rotates by `window` envs per step, the sampler tick is the running update count, ADAM's beta powers advance in
 * Float64 after every update), so a run of the loop leaves the same bytes as that host loop.  What it removes is the host time per
 * launch: a Python / Julia caller pays several microseconds per foreign call, which at <= 8 192 envs is comparable to the kernels.
 *
 * mode SHEMS_LOOP_ORDERED   : program order on `stream` -- the reference's order.
 * mode SHEMS_LOOP_PIPELINED : replay(t) runs on `stream2` while the fused act/step launch of step t runs on `stream`; act(t) reads the
 *                             actor published by replay(t - 1) (actor_pub[t & 1], written by the ADAM sweep), exactly the actor the
 *                             ordered loop would use; the one deviation is that replay(t) samples the ring as it stood BEFORE step
 *                             t's inserts (the window being written is excluded, shems_ddpg_critic_grad_ex).
 * mode SHEMS_LOOP_PIPELINED_EXACT : the envs of step t's ring window are stepped FIRST (their own launch on `stream`), replay(t) then
 *                             runs on `stream2` and samples the ring WITH those inserts while the rest of the batch is stepped on
 *                             `stream`: the same bytes as SHEMS_LOOP_ORDERED.
 * The struct is caller-owned state: fields marked in/out are advanced by the call.  `sync` holds the loop's two signal-memory words (stream memory operations) and is created on
 * first use of a pipelined mode; release it with shems_train_loop_release (it does not touch the device buffers). */
enum { SHEMS_LOOP_ORDERED = 0, SHEMS_LOOP_PIPELINED = 1, SHEMS_LOOP_PIPELINED_EXACT = 2 };
typedef struct shems_train_loop {
    shems_view       view;
    shems_act_params act;            /* .tick is overwritten with t; .actor = the learner's actor (ddpg.actor)                  */
    shems_ddpg       ddpg;
    shems_replay     ring;
    float   *rewards_f32;            /* dev [n] or NULL: Float32(reward) of the last step                                        */
    float   *actor_pub[2];           /* pipelined modes: two dev [129002] copies of the actor, both equal to ddpg.actor on entry of the first call */
    int64_t  window;                 /* envs whose transitions enter the ring per vector step (<= n, <= ring.capacity)            */
    int64_t  ring_pushed;            /* in/out: transitions pushed so far (push position = ring_pushed mod capacity)              */
    int64_t  t;                      /* in/out: vector steps done so far                                                          */
    int64_t  updates;                /* in/out: replay() calls done so far (the sampler's tick)                                   */
    uint64_t env_seed;               /* reset!(env) key (shems_reset_seeded_dev)                                                  */
    uint64_t sample_seed;            /* getData key (shems_ddpg_update's seed)                                                    */
    uint32_t episode;                /* in/out                                                                                    */
    int32_t  ep_len;                 /* steps per episode (EP_LENGTH["train"] = 72)                                              */
    int32_t  updates_per_step;       /* 0 = no learning                                                                           */
    int32_t  mode;                   /* SHEMS_LOOP_*                                                                              */
    double   eta_crit, bp_crit[2];   /* in/out: ADAM(eta_crit) and its beta^t powers for the NEXT critic step                     */
    double   eta_act, bp_act[2];     /* in/out: same for the actor                                                                */
    void    *sync;                   /* opaque, NULL on first use                                                                 */
    shems_dp *dp;                    /* data-parallel replicas (SHEMS_LOOP_ORDERED only): replay() = shems_ddpg_update_dp; NULL = one replica */
} shems_train_loop;
int shems_train_steps(shems_train_loop *loop, int64_t k, void *stream, void *stream2);
/* Pipelined modes: make `stream` wait for everything the loop has in flight on stream2 (the caller then synchronises `stream`). */
int shems_train_loop_join(shems_train_loop *loop, void *stream, void *stream2);
int shems_train_loop_release(shems_train_loop *loop);

/* ------------------------------------------------- learner groups -- */
/* The thesis protocol trains many INDEPENDENT learners (40 seeds x 10 charger profiles, one OS process and one
 * batch-1 GPU stream each: run scripts + DDPG_reinforce_charger_v1.jl:10-47).  A learner
 * group advances `count` independent learners with the same launches: every device buffer of learner l -- all
 * pointers of shems_ddpg, shems_replay and the actor / s_min / s_max of shems_act_params -- is learner 0's pointer
 * plus l * stride_bytes (one slab per learner, carved identically), and learner l owns the envs
 * [l * envs_per_learner, (l + 1) * envs_per_learner) of the view.  Learners never exchange anything: per learner the
 * result is bit-identical to the single-learner entry points run on that learner's buffers with seed + l.
 *   act/step:  env i is driven by learner i / envs_per_learner's actor and normalisation; the ring window applies
 *              inside each learner's env block (n = envs_per_learner) and pushes into that learner's ring.
 *              envs_per_learner must be a multiple of 32 (tiles of 128 / 64 envs are used where they divide it).
 *   update:    grid z = learner; minibatch l is sampled with Philox key seed + l; ADAM scalars are shared (the
 *              learners advance in lockstep). */
typedef struct shems_group {
    int32_t count;             /* learners (>= 1)                                         */
    int32_t reserved;
    int64_t stride_bytes;      /* byte distance between consecutive learners' slabs (multiple of 16) */
    int64_t envs_per_learner;  /* act/step only                                           */
} shems_group;

/* replay() for every learner in the LATENCY form: the five launches of shems_ddpg_update with grid z = learner, or its four parts. */
int shems_ddpg_group_update(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int64_t ring_len,
                            uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit,
                            double eta_act, double bp1_act, double bp2_act, void *stream);
int shems_ddpg_group_critic_grad(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g,
                                 int64_t ring_len, uint64_t seed, uint32_t tick, void *stream);
int shems_ddpg_group_critic_apply(const shems_ddpg *d0, const shems_group *g, double eta, double bp1, double bp2,
                                  void *stream);
int shems_ddpg_group_actor_grad(const shems_ddpg *d0, const shems_group *g, void *stream);
int shems_ddpg_group_actor_apply(const shems_ddpg *d0, const shems_group *g, double eta, double bp1, double bp2,
                                 void *stream);
/* A TILED working layout of the layer-2 state (round 6).  The W2-gradient launches of the throughput form below are its
 * HBM stream -- 32 B in and out per W2 parameter: ADAM moments (Flux.Optimise.ADAM state, DDPG.jl:105-108), parameter and target
 * (soft_update!, DDPG.jl:99-103) -- and in Flux order ([in][out] rows of 500 floats) a 64 x 64 tile of it is 4 x 64 pieces of 256
 * bytes: 3.85 TB/s where one contiguous 64 KB piece per tile reaches 4.78 TB/s (tools/micro/adam_stream.hip).  A tiled region holds,
 * per network, W2 / m / v / target as [4 k-tiles][8 n-tiles][m | v | p | target][64][64] floats (rows / columns padded to 256 / 512
 * with zeros), SHEMS_W2T_FLOATS per learner, at learner 0's pointer + l * stride_bytes like every other block.  While a group
 * trains with t != NULL the tiled regions hold the CURRENT layer-2 state and the W2 ranges of the Flux-order blocks
 * (shems_ddpg.actor / critic / actor_t / critic_t / m_* / v_*) are stale; everything else (layer 1, b2, W3, b3) stays in the
 * Flux-order blocks.  shems_group_w2_to_tiled / _to_flux copy the W2 ranges one way or the other (checkpoints, set / get of
 * parameters, the single-learner entry points and the latency form all speak Flux order).  Same arithmetic and summation order on
 * either layout: the two leave the same values (tests/test_group_gpu.py holds both to the float64 oracle and to each other bit for
 * bit). */
enum { SHEMS_W2T_FLOATS = 32 * 4 * 64 * 64 };
typedef struct shems_group_w2t {
    float *actor;              /* dev [SHEMS_W2T_FLOATS] of learner 0: actor W2, its moments and actor_target W2  */
    float *critic;             /* dev [SHEMS_W2T_FLOATS] of learner 0: critic ...                                   */
} shems_group_w2t;
int shems_group_w2_to_tiled(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, void *stream);
int shems_group_w2_to_flux(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, void *stream);
/* The same working layout for a SINGLE learner.  In Flux order the 250 x 500 layer-2 state has a row pitch of 2 000 bytes and starts at
 * byte 10 000 (actor) / 12 000 (critic) of its block, so every 128-byte row piece a 32 x 32 gradient tile of shems_ddpg_update reads and
 * writes (m, v, parameter, target) straddles two lines; on tiles it is one (tools/micro/w2_single_layout.hip).
 *   shems_ddpg_tiled_enter   copies the W2 ranges of d's eight blocks into the regions t (128-byte aligned, SHEMS_W2T_FLOATS each) on
 *                            `stream` and records d's blocks: from here on the regions hold the current layer-2 state and the W2
 *                            ranges of the Flux-order blocks are stale (the contract above).
 *   shems_ddpg_tiled_leave   copies them back on `stream` and forgets the learner.
 *   shems_ddpg_tiled_current *out = 1 between the two, else 0.
 * Between enter and leave shems_ddpg_update (d_publish must be NULL), shems_act_step_dev and shems_train_steps' ordered loop, called
 * with the same blocks, work on the regions and leave the bits the Flux-order form leaves.  Every other entry point that reads or
 * writes one of the eight blocks in Flux order returns SHEMS_ERR_STATE and launches nothing.  The record is host state of the process,
 * keyed by the blocks' addresses: leave before the blocks are freed. */
int shems_ddpg_tiled_enter(const shems_ddpg *d, const shems_group_w2t *t, void *stream);
int shems_ddpg_tiled_leave(const shems_ddpg *d, void *stream);
int shems_ddpg_tiled_current(const shems_ddpg *d, int32_t *out);
/* ------------------------------------------- per-learner hyper-parameters of a learner group -- */
/* The thesis's experiment is a hyper-parameter grid (input09_08_on_01-09_eval.jl:62-106: BATCH, noise_act, (L1, L2), (eta_act,
 * eta_crit)).  With one record per learner -- a DEVICE array of g->count records, learner l's is d_hp[l] -- one group runs many grid
 * points at once: the group entry points that take d_hp use the record's scalars in place of the shared ones of d0 / p0.  The
 * ADAM beta powers stay shared (the learners advance in lockstep).  A record holding d0's / p0's values gives the bits of
 * d_hp == NULL.  Hidden sizes below (250, 500) need no field: such a learner's networks are zero-padded (ddpg.pad_net) and stay so. */
typedef struct shems_group_hparams {
    double  eta_act, eta_crit;     /* ADAM(eta), DDPG.jl:105-108: the Float64 value of the Float32 literal (as Agent.eta_*)      */
    float   gamma, tau;            /* DDPG.jl:133, 99-103                                                                        */
    float   noise_mu, noise_sigma; /* GNoise of act(), DDPG.jl:151-160                                                           */
    int32_t batch;                 /* BATCH_SIZE, 1..128 (the device clamps it to that range whatever the record holds)          */
    int32_t reserved;              /* 0                                                                                          */
} shems_group_hparams;             /* 40 bytes */
/* Host-side validation of count records in HOST memory: batch in 1..128, eta finite and > 0, 0 < tau <= 1, 0 <= gamma <= 1,
 * noise_sigma >= 0, every value finite.  SHEMS_ERR_ARG names the first bad learner and field. */
int shems_group_hparams_check(const shems_group_hparams *host_hp, int32_t count);
/* replay() for every learner in the THROUGHPUT form (csrc/shems_gupd.hip): for groups wide enough that nothing is latency-bound any
 * more (the thesis protocol runs 40 seeds x 10 chargers = 400 learners, RL-SHEMS_bs_scheduler_1179_08_on_01-98.sh:67-87) -- plain
 * back-propagation on small tiles, 4 workgroups resident per CU, eight launches for the whole group.  Same sampler, same ADAM
 * arithmetic as shems_ddpg_group_update; the products sum in another order, so per learner the two agree to fp32 accumulation
 * accuracy (every gradient block within 2e-6 of its max-abs of a float64 evaluation), not bit for bit.
 *   t:     NULL = every array in Flux order; else the layer-2 state of both networks lives in the tiled regions (both 16-byte
 *          aligned) and the W2 ranges of the Flux-order blocks are neither read nor written.
 *   d_hp:  NULL = d0's batch (1..128) / gamma / tau and eta_crit / eta_act for every learner; else an 8-byte aligned device array,
 *          learner l's batch (the first batch_l draws of the same minibatch stream, masks, divisors, losses), gamma, tau and eta
 *          (k1 = eta_l / (1 - bp1) formed on the device, correctly rounded) from d_hp[l]; d0's three and eta_crit / eta_act are
 *          then ignored.
 *   flags: SHEMS_TP_STORE_GRAD also leaves the gradients in grad_actor / grad_critic (otherwise they are never materialised;
 *          the b3 / layer-1 / W2 / b2 / W3 elements are consumed by ADAM in the lane that finishes them).
 * Uses d0->ws with a layout of its own: do not mix the two forms on one workspace within one update. */
enum { SHEMS_TP_STORE_GRAD = 1 };
int shems_ddpg_group_update_tp(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, const shems_group_w2t *t,
                               const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed, uint32_t tick, double eta_crit,
                               double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act, int32_t flags,
                               void *stream);
/* The fused vector step (shems_act_step_dev) for every learner of a group, one launch: env i is driven by learner
 * i / envs_per_learner, draws its noise keyed by its index in the view, and the ring window applies inside each learner's env block.
 *   t:     NULL = every actor in Flux order; else every learner's actor W2 is read from its tiled region (t->actor, 16-byte
 *          aligned; t->critic is not used).
 *   d_hp:  NULL = p0's noise for every learner; else an 8-byte aligned device array, learner l's envs draw
 *          d_hp[l].noise_mu + d_hp[l].noise_sigma * z (the same z) and p0's noise_mu / noise_sigma are ignored.  Gaussian noise only
 *          then: p0->noise_kind must be SHEMS_NOISE_GAUSS. */
int shems_act_step_group_dev(const shems_view *v, const shems_act_params *p0, const shems_group *g, const shems_group_w2t *t,
                             const shems_group_hparams *d_hp, float *d_a, double *d_returns_acc, const shems_replay *ring0,
                             const shems_ring_window *window, void *stream);
/* ------------------------------------------- the wide group form: learner groups on the layer-by-layer path -- */
/* A learner group whose networks have one padded hidden size (l1, l2) up to 4096 (the tuned grid's (300, 600); smaller learners are
 * zero-padded into it and stay so) and whose learners' batches reach 256.  One update pass holds P = max(128, max_batch rounded up to
 * 32) minibatch rows; learner l's rows batch_l .. P-1 are zero and masked.  Every launch runs all learners (grid z / x = learner),
 * so the launch count does not depend on the group's size.  The shems_ddpg blocks of d0, learner l's at + l * g->stride_bytes,
 * are carved for (l1, l2) by shems_wide_params, ws for P by shems_wide_group_workspace_floats. */
/* shems_group_hparams_check with batch in 1..max_batch, max_batch <= 256. */
int shems_group_hparams_check_wide(const shems_group_hparams *host_hp, int32_t count, int32_t max_batch);
/* Floats of one learner's ws for pass width P (= shems_wide_workspace_floats for max_batch <= 128). */
int shems_wide_group_workspace_floats(int32_t l1, int32_t l2, int32_t max_batch, int64_t *out);
/* replay() (DDPG.jl:121-145) for every learner: the launches of shems_wide_critic_grad_ex, _critic_apply, _actor_grad and
 * _actor_apply_pub, each once for the whole group.  Learner l samples the first batch_l draws of the stream (seed + l, tick) (as
 * shems_ddpg_sample_indices).  d_hp: learner l's batch (clamped to 1..max_batch on the device), gamma, tau and eta (k1 formed on the
 * device); NULL: d0's batch, gamma and tau and eta_crit / eta_act for every learner.  The ADAM beta powers are shared.  At P = 128
 * and without records, learner l's results are bit-identical to the single-learner wide entry points on its blocks with seed + l. */
int shems_wide_group_update(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int32_t l1, int32_t l2,
                            const shems_group_hparams *d_hp, int32_t max_batch, int64_t ring_len, uint64_t seed, uint32_t tick,
                            double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act, void *stream);
/* The fused vector step (shems_wide_act_step_dev) for a group, four launches for all learners: env i is driven by learner
 * i / envs_per_learner; Gaussian noise only, keyed by the global env index, with d_hp[l].noise_mu / noise_sigma (NULL: p0's).  The
 * ring window applies inside each learner's env block, as in shems_act_step_group_dev.  d_ws: 16-byte aligned,
 * shems_wide_act_workspace_floats(l1, l2, n_envs) floats. */
int shems_wide_act_step_group_dev(const shems_view *v, const shems_act_params *p0, const shems_group *g, int32_t l1, int32_t l2,
                                  const shems_group_hparams *d_hp, float *d_ws, float *d_a, double *d_returns_acc, const shems_replay *ring0,
                                  const shems_ring_window *window, void *stream);
/* ------------------------------------------- per-learner exploration and ring size of a learner group -- */
/* The reference's live grid (input.jl:58-100) varies MEM_SIZE and the Ornstein-Uhlenbeck noise's theta per point (all 27 points use
 * noise_type = "ou": OUNoise, DDPG.jl:49-55, 157-158; memory = CircularBuffer{Any}(MEM_SIZE), input.jl:64, 140).  These per-learner
 * values travel beside d_hp in a second, parallel DEVICE array of g->count records, learner l's is d_xp[l], through the *_x entry
 * points below; the entry points without _x are their d_xp == NULL case.  ring0->capacity stays what every learner's ring arrays are
 * carved for: learner l uses slots [0, mem_size_l) of its own. */
typedef struct shems_group_xparams {
    float   ou_theta;              /* OUNoise theta of this learner (used when p0->noise_kind == SHEMS_NOISE_OU), DDPG.jl:49-55      */
    float   ou_dt;                 /* OUNoise dt                                                                                    */
    int32_t mem_size;              /* this learner's ring capacity, 1..ring0->capacity (input.jl:64, 140): slots [0, mem_size)      */
    int32_t reserved;              /* 0                                                                                             */
} shems_group_xparams;             /* 16 bytes */
/* Host-side validation of count records in HOST memory (DDPG.jl:49-55, input.jl:64): ou_theta finite and >= 0, ou_dt finite and > 0,
 * mem_size in 1..capacity, reserved 0.  SHEMS_ERR_ARG names the first bad learner and field, as shems_group_hparams_check does. */
int shems_group_xparams_check(const shems_group_xparams *host_xp, int32_t count, int64_t capacity);
/* shems_act_step_group_dev with per-learner exploration and ring sizes (DDPG.jl:49-55, 157-158; input.jl:64, 140).  d_hp, d_xp (both
 * 8-byte aligned device arrays of g->count records) and d_pushed (device int64 [g->count]: the transitions pushed into learner l's
 * ring so far) are all required.  p0->noise_kind is SHEMS_NOISE_GAUSS (d_hp[l].noise_mu + d_hp[l].noise_sigma * z, as without d_xp)
 * or SHEMS_NOISE_OU: learner l's envs run X += theta_l (mu_l - X) dt_l + sigma_l sqrt(dt_l) z with mu_l / sigma_l from d_hp[l],
 * theta_l / dt_l from d_xp[l], X = p0->ou_state[i] for the global env index i and the draw z of shems_act_step_dev.
 * window->pos is ignored: the env at relative window position rel goes to slot (d_pushed[l] + rel) mod mem_size_l of learner l's
 * ring.  window->count must not exceed the smallest mem_size and every record must have passed shems_group_xparams_check: both are the
 * caller's preconditions (the records are device memory, the entry point cannot read them).  The device clamps mem_size to
 * 1..ring0->capacity and d_pushed[l] to >= 0 only so that no slot outside the ring arrays is written; with a violated precondition
 * the push lands in a wrong slot without any error -- the clamp makes that memory-safe, not right.  The kernels never write d_pushed. */
int shems_act_step_group_x_dev(const shems_view *v, const shems_act_params *p0, const shems_group *g, const shems_group_w2t *t,
                               const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, float *d_a,
                               double *d_returns_acc, const shems_replay *ring0, const shems_ring_window *window, void *stream);
/* shems_wide_act_step_group_dev in the same way (DDPG.jl:49-55, 157-158; input.jl:64, 140). */
int shems_wide_act_step_group_x_dev(const shems_view *v, const shems_act_params *p0, const shems_group *g, int32_t l1, int32_t l2,
                                    const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, float *d_ws,
                                    float *d_a, double *d_returns_acc, const shems_replay *ring0, const shems_ring_window *window,
                                    void *stream);
/* shems_ddpg_group_update_tp with per-learner ring lengths (input.jl:64, 140; getData, MPS:31-42): learner l samples
 * x mod min(d_pushed[l], d_xp[l].mem_size) where shems_ddpg_group_update_tp samples x mod ring_len.  d_hp, d_xp and d_pushed are
 * required.  Every learner's length must be >= 1: that is the caller's precondition (the arrays are device memory; the device clamps
 * the length to 1..ring0->capacity, so a violated precondition samples slot 0 without any error -- memory-safe and free of a division
 * by zero, but not right). */
int shems_ddpg_group_update_tp_x(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, const shems_group_w2t *t,
                                 const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, uint64_t seed,
                                 uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act,
                                 double bp2_act, int32_t flags, void *stream);
/* The supervised update (shems_ddpg_clone_update's definition) for every learner of a group, throughput form, four launches:
 *   loss_l = Flux.mse(actor_l(normalize(s)), a_demo) on the first batch_l draws of the stream (seed + l, tick) from learner l's ring,
 * then ADAM on the actor and the soft update of actor_t (d0->tau or the record's; 1 keeps actor_t == actor bit for bit).  The
 * sampler, a forward launch with the actor(s) job alone, the actor's D1 launch with the cloning head (d3[o][m] = (a_pi - a_demo)
 * (1 - a_pi^2) / batch_l, 0 in the pad columns; losses[1] sums the squared differences per 64-lane wave by butterfly, then
 * ((w0 + w1) + w2) + w3, / (2 batch_l)), and the update's W2-gradient launch.  Only s and a of a slot are read (ring0->r, s2 and done
 * may be NULL); the critic, its target, its moments, grad_critic and losses[0] are not touched.
 *   ring0, ring_stride_bytes: learner l's ring arrays are ring0's + l * ring_stride_bytes -- a stride of the ring's own, which may be
 *          g->stride_bytes (rings inside the slabs) or anything else (demonstrations outside them): a non-negative multiple of 4, not
 *          0 when g->count > 1.  Every learner samples x mod ring_len (1..ring0->capacity).
 *   t, d_hp, flags: as shems_ddpg_group_update_tp (d_hp: the record's batch, eta_act and tau; eta is ignored then).
 * Everything shems_ddpg_group_update_tp refuses for the buffers read here is refused with SHEMS_ERR_ARG before any launch. */
int shems_ddpg_group_clone_update_tp(const shems_ddpg *d0, const shems_replay *ring0, int64_t ring_stride_bytes, const shems_group *g,
                                     const shems_group_w2t *t, const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed,
                                     uint32_t tick, double eta, double bp1, double bp2, int32_t flags, void *stream);
/* The critic-only update (shems_ddpg_critic_update's definition: update_model!(critic), soft_update!(critic_target, critic)) for every
 * learner of a group, throughput form, five launches: the sampler and the first five launches of shems_ddpg_group_update_tp without
 * the actor(s) job.  From the same state, ring, seed and tick it leaves in critic, critic_t, m_critic, v_critic, grad_critic and
 * losses[0] the bits of shems_ddpg_group_update_tp; actor, actor_t, m_actor, v_actor, grad_actor and losses[1] are not touched.
 * The ring needs all five arrays; ring0 / ring_stride_bytes, t, d_hp (batch, gamma, eta_crit, tau) and flags as above. */
int shems_ddpg_group_critic_update_tp(const shems_ddpg *d0, const shems_replay *ring0, int64_t ring_stride_bytes, const shems_group *g,
                                      const shems_group_w2t *t, const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed,
                                      uint32_t tick, double eta, double bp1, double bp2, int32_t flags, void *stream);
/* TD3 for every learner of a group, throughput form: shems_td3_update's definition (steps 1-5 above it) per learner l,
 * with two group conventions: learner l's minibatch is the first batch_l draws of the Philox key seed + l at `tick` (what
 * shems_ddpg_group_update_tp samples), and its target noise is the block (m, 0, tick, 0x5452474E) of the SAME key seed + l.  sigma_trg,
 * clip_trg (t0's) and update_policy are the group's; the beta powers advance in lockstep (the critics' on every update, the actor's
 * on policy steps: host state).  Both critics take an ADAM step on every update; update_policy = 1 adds the actor's step through the
 * UPDATED critic 1 and the three soft updates; update_policy = 0 touches nothing of the actor and both critic targets keep their bytes
 * (the critic launches run with tau = 0: 1 t + 0 p).
 *   t0     learner 0's shems_td3; every block of learner l, critic 2's and ws2 included, lies at + l * g->stride_bytes.  ws2:
 *          shems_td3_group_workspace_floats() floats per learner (it mirrors the throughput carve of ws where critic 2's launches
 *          read it); after an update ws2 + SHEMS_TD3_GROUP_WS2_PUB holds a~' [2][128], y [128], q'_1 [128], q'_2 [128] (columns >=
 *          batch_l are padding).
 *   w, w2t_critic2   NULL, NULL: Flux order.  Else the tiled layout: w as for shems_ddpg_group_update_tp and a third region of
 *          SHEMS_W2T_FLOATS per learner with W2 | m | v | target of critic 2 (shems_group_w2_to_tiled / _to_flux convert it when given
 *          a shems_ddpg whose critic fields name critic 2's blocks and a shems_group_w2t whose critic names this region).
 *   d_hp, d_hp_hold  per-learner records as for shems_ddpg_group_update_tp; d_hp_hold holds the same records with tau = 0 and is what
 *          the critic launches read when update_policy = 0 (required then; the host builds it, shems_group_hparams_check is not asked).
 *   flags  SHEMS_TP_STORE_GRAD also leaves grad_critic2.
 * Seven launches, ten on a policy step (csrc/shems_gupd.hip): the sampler, P1 of shems_ddpg_group_update_tp (without the actor(s) job
 * off a policy step), both target critics on the smoothed action beside critic 2's forward pass, one D1 launch with the twin head per
 * critic, the unchanged W2-gradient / ADAM launch per critic; then P5-P7 of shems_ddpg_group_update_tp.  With sigma_trg = 0 and critic 2
 * a copy of critic 1, update_policy = 1 leaves shems_ddpg_group_update_tp's bits.
 * SHEMS_ERR_ARG, nothing launched: whatever shems_ddpg_group_update_tp refuses; a NULL, misaligned or critic-1-overlapping critic-2
 * block; w2t_critic2 without w or w without w2t_critic2; d_hp_hold missing when d_hp is given and update_policy = 0; sigma_trg or
 * clip_trg negative or not finite; update_policy outside {0, 1}.  SHEMS_ERR_STATE: a learner between shems_ddpg_tiled_enter and
 * shems_ddpg_tiled_leave. */
#define SHEMS_TD3_GROUP_WS2_PUB 31112
int shems_td3_group_workspace_floats(int64_t *out);
int shems_td3_group_update_tp(const shems_td3 *t0, const shems_replay *ring0, const shems_group *g, const shems_group_w2t *w,
                              float *w2t_critic2, const shems_group_hparams *d_hp, const shems_group_hparams *d_hp_hold, int64_t ring_len,
                              uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act,
                              double bp1_act, double bp2_act, int update_policy, int32_t flags, void *stream);
/* Prioritized replay for every learner of a group, throughput form: shems_ddpg_update_per's seven steps per learner l,
 * with the group's conventions.  Learner l's Philox key is seed + l on the stream tag 0x50455253 (what shems_ddpg_group_update_tp's
 * sampler does on its own tag); with records the first batch_l columns are live, t_m = (m + u_m) (T_l / batch_l), and the weight
 * maximum runs over learner l's live columns.  ring_len, fresh_pos and fresh_count are the group's (the rings advance in lockstep);
 * alpha, beta and eps_p are per0's, shared; beta is read on every call.  prio [capacity], pmax [1] (1.0 at the start) and the sampler
 * workspace (shems_per_workspace_floats(capacity) floats) are per learner: per0 names learner 0's, learner l's lie at
 * + l * g->stride_bytes.  Step 5 is shems_ddpg_group_update_tp's critic head with dq = 2 w diff / batch and losses[0] =
 * sum (w diff) diff / batch in that head's summation order: weights of 1.0 leave its bits.  Step 6 (pi <- (|diff| + eps_p)^alpha, the
 * highest column wins a slot drawn twice, pmax only ever raised) is done by each learner's publishing workgroup of the critic's D1
 * launch.  Nine launches: the sampler (one workgroup of 1024 threads per learner), then shems_ddpg_group_update_tp's eight with the
 * sampler role reading the published slots and the critic's D1 launch carrying the weighted head; narrow shapes below 48 learners.
 *   flags: SHEMS_TP_STORE_GRAD as above.  SHEMS_TP_PER_GIVEN: no sampler launch and no write-back -- the caller has filled every
 *          learner's slots (workspace floats 4..131 as int32, -1 in the pad columns) and weights (floats 132..259); prio and pmax keep
 *          their bytes.  With the slots of shems_ddpg_sample_indices(seed + l, tick) and weights of 1.0 the update leaves
 *          shems_ddpg_group_update_tp's bits.
 * SHEMS_ERR_ARG, nothing launched: whatever shems_ddpg_group_update_tp refuses; whatever shems_ddpg_update_per refuses for the
 * prioritized ring's own arguments (with records the batches are the records'); a per0 block that is NULL or misaligned, overlaps
 * one of learner 0's DDPG blocks, its workspace, its tiled regions or its ring, or (more than one learner) ends beyond one stride
 * of the lowest of those blocks; unknown flag bits.  SHEMS_ERR_STATE: a learner between shems_ddpg_tiled_enter and
 * shems_ddpg_tiled_leave.
 * After an update learner l's workspace holds y [128] and q [128] at float SHEMS_TP_PER_PUB (columns >= batch_l are padding): the new
 * priorities are formed from diff = q - y. */
enum { SHEMS_TP_PER_GIVEN = 2 };
#define SHEMS_TP_PER_PUB 165000
int shems_ddpg_group_update_per_tp(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, const shems_group_w2t *t,
                                   const shems_group_hparams *d_hp, const shems_per *per0, int64_t ring_len, int64_t fresh_pos,
                                   int64_t fresh_count, uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit,
                                   double bp2_crit, double eta_act, double bp1_act, double bp2_act, int32_t flags, void *stream);
/* The sampler launch alone (steps 1-4 for every learner; tests, a Julia caller).  d_hp: NULL = `batch` live columns for every
 * learner, else learner l's batch from d_hp[l] (`batch` is ignored).  SHEMS_ERR_ARG as above for g, d_hp and per0; this call is not
 * told where a slab begins, so it holds the three blocks to one stride of the lowest of THEM only: that they lie inside the learner's
 * slab is the caller's to see to. */
int shems_per_group_sample_dev(const shems_per *per0, const shems_group *g, const shems_group_hparams *d_hp, int64_t capacity,
                               int64_t ring_len, int64_t fresh_pos, int64_t fresh_count, uint64_t seed, uint32_t tick,
                               int32_t batch, void *stream);
/* shems_wide_group_update in the same way (input.jl:64, 140; DDPG.jl:121-145). */
int shems_wide_group_update_x(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int32_t l1, int32_t l2,
                              const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, int32_t max_batch,
                              uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act,
                              double bp1_act, double bp2_act, void *stream);
/* min_max_buffer for every learner of the group (learner l: Philox key seed + l). */
int shems_minmax_group_dev(const shems_replay *ring0, const shems_group *g, int64_t ring_len, int64_t count,
                           uint64_t seed, float *d_s_min0, float *d_s_max0, void *stream);
/* The evaluation sweep of run_episodes (DDPG.jl:273-290) for every learner of a group, one launch.  g->envs_per_learner is the eval
 * block E_eval (a multiple of 32); learner l's eval returns are d_returns[l * E_eval + j], j < runs <= E_eval (the rest is padding,
 * never read).  Per learner: d_score[l] = (sum over j = 0 .. runs-1 in ascending order, float64) / runs; if d_score[l] > d_best_score[l]
 * (strict; the caller starts from -100000, DDPG.jl:246) then d_best_score[l] = score, d_best_run[l] = episode, d_improved[l] = 1 and
 * snapshot row l (d_best0 + l * best_stride_bytes: actor | pad to 16 B | s_min[9] | pad | s_max[9] | pad, the row of
 * harness.inference_many) receives the actor in Flux order and the normalisation; else d_improved[l] = 0 and nothing else is written.
 * W2 is read from the actor's p tiles when t != NULL (a group training on the tiled layout), else from d0->actor.  Nothing of the
 * training state is written.  (l1, l2) != (0, 0): the wide form, actors of shems_wide_params(l1, l2) floats; t must be NULL. */
int shems_group_eval_best_dev(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, int32_t l1, int32_t l2,
                              const double *d_returns, int32_t runs, int32_t episode, double *d_score, double *d_best_score,
                              int32_t *d_best_run, uint8_t *d_improved, float *d_best0, int64_t best_stride_bytes, void *stream);

/* Parameter noise, noise_type "pn" (struct ParamNoise input.jl:210-215; add_perturb! DDPG.jl:89-96;
 * adapt_param_noise! DDPG.jl:74-87).  The reference adds ONE scalar draw N(mu, sigma_current) to every parameter
 * array of a copy of the actor (sample_noise(pn, rng) re-seeds before each draw); act() then evaluates the copy
 * without action noise (pass it as shems_act_params.actor with train = 0), and replay() adapts sigma_current from
 * the distance between the two actors' outputs on the sampled minibatch.
 *   perturb:    d_perturbed[i] = d_params[i] + shift, i < n
 *   batch_obs:  the s rows of the minibatch the last shems_ddpg_critic_grad(_ex) sampled -> d_obs [batch][9]
 *   distance:   d_out[0] = sqrt(mean((d_a - d_b)^2)) over `count` floats */
/* BATCH_SIZE above 128 (the tuned template's 150, input.jl's 200): one update pass holds 128 minibatch columns, so replay() runs the
 * gradient calls once per SUB-BATCH (each on its own workspace and gradient buffer, `batch` = the sub-batch size: its gradient is
 * the mean over the sub-batch) and combines them, acc = w_acc * acc + w_g * g with w_g = sub-batch size / BATCH_SIZE, before the one
 * ADAM step -- Flux.mse / -mean(q) over the whole minibatch (DDPG.jl:134-140) is exactly that weighted mean of sub-batch means.
 * w_acc == 0: acc is overwritten (never read). */
int shems_ddpg_combine_dev(float *d_acc, const float *d_g, int64_t n, float w_acc, float w_g, void *stream);

int shems_ddpg_perturb_dev(const float *d_params, float *d_perturbed, int64_t n, float shift, void *stream);
int shems_ddpg_batch_obs_dev(const shems_ddpg *d, const shems_replay *ring, float *d_obs, void *stream);
int shems_action_distance_dev(const float *d_a, const float *d_b, int64_t count, float *d_out, void *stream);
/* min_max_buffer (MPS:50-53): minimum/maximum of s over a bootstrap sample of `count` ring entries. */
int shems_minmax_dev(const shems_replay *ring, int64_t ring_len, int64_t count, uint64_t seed,
                     float *d_s_min, float *d_s_max, void *stream);

/* ------------------------------------------- networks wider than (250, 500) -- */
/* The reference's grids hold one architecture larger than the tuned one: (L1, L2) = (300, 600) (input09_08_on_01-09_eval.jl:62-66,
 * input.jl:58-66; Dense widths of DDPG.jl:30-46).  Smaller networks run on the entry points above zero-padded into the (250, 500)
 * layout; a larger one runs through the entry points below (csrc/shems_wide.hip): the same functions, every layer one fp32-MFMA matrix
 * product as in the reference's Flux / CUBLAS path, parameters in the flat Flux layout OF THAT SIZE
 * (W1[in][l1] b1[l1] W2[l1][l2] b2[l2] W3[l2][out] b3[out]; shems_wide_params gives the counts), the same Philox streams (noise, minibatch
 * slots) as the tuned path.  1 <= l1, l2 <= 4096.  Not the headline path: tolerance-class like the tuned kernels, an order of magnitude
 * slower per update. */
int shems_wide_params(int32_t l1, int32_t l2, int64_t *n_actor, int64_t *n_critic);
/* floats of shems_ddpg.ws for the update entry points / of d_ws for the act entry points with m observations */
int shems_wide_workspace_floats(int32_t l1, int32_t l2, int64_t *out);
int shems_wide_act_workspace_floats(int32_t l1, int32_t l2, int64_t m, int64_t *out);
/* act() (DDPG.jl:148-176) as shems_actor_forward_dev, and the fused vector step of episode! (DDPG.jl:195-234) as shems_act_step_dev
 * (without the per-workgroup reward sums): normalize + three matrix products + one launch for tanh / noise / clamp / scale_action /
 * step! / remember. */
int shems_wide_actor_forward_dev(const shems_act_params *p, int32_t l1, int32_t l2, const float *d_obs, int64_t m, float *d_a, float *d_ws,
                                 void *stream);
int shems_wide_act_step_dev(const shems_view *v, const shems_act_params *p, int32_t l1, int32_t l2, float *d_ws, float *d_a, double *d_rewards,
                            float *d_rewards_f32, double *d_returns_acc, const shems_replay *ring, const shems_ring_window *window,
                            void *stream);
/* replay() (DDPG.jl:121-145) in the split form of shems_ddpg_critic_grad_ex / _critic_apply / _actor_grad / _actor_apply_pub (the
 * caller may all-reduce grad_critic / grad_actor in between); every buffer of shems_ddpg holds the wide network's parameter count. */
int shems_wide_critic_grad_ex(const shems_ddpg *d, int32_t l1, int32_t l2, const shems_replay *ring, int64_t ring_len, uint64_t seed,
                              uint32_t tick, int64_t excl_pos, int64_t excl_count, void *stream);
int shems_wide_critic_apply(const shems_ddpg *d, int32_t l1, int32_t l2, double eta, double bp1, double bp2, double grad_scale, void *stream);
int shems_wide_actor_grad(const shems_ddpg *d, int32_t l1, int32_t l2, void *stream);
int shems_wide_actor_apply_pub(const shems_ddpg *d, int32_t l1, int32_t l2, double eta, double bp1, double bp2, double grad_scale,
                               float *d_publish, void *stream);
/* ring slots [batch] of the minibatch the last shems_wide_critic_grad_ex drew, to host memory (adapt_param_noise!, DDPG.jl:74-87);
 * synchronises the stream */
int shems_wide_batch_slots(const shems_ddpg *d, int32_t l1, int32_t l2, int32_t *out_slots, void *stream);
/* inference(env; track > 0) (memory_plotting_saving.jl:62-89) as shems_track_dev, for actors of hidden sizes (l1, l2) */
int shems_wide_track_dev(const shems_view *v, const shems_act_params *p, int32_t l1, int32_t l2, int64_t actor_stride_bytes,
                         int32_t nsteps, double *d_results, int64_t results_env, double *d_returns, void *stream);

/* ------------------------------------------- the perfect-foresight controller -- */
/* The upper yardstick of the thesis is a perfect-foresight optimiser.  With the series known in advance, the best action sequence of
 * the environment AS WRITTEN -- action (LU1:283-316), step! (LU1:343-485), next_state! (LU1:264-281), scored by the plain sum of
 * rewards (MPS:62-89) -- is a finite-horizon dynamic programme over (Soc_b, Soc_ev); csrc/shems_foresight_core.h holds the recursion.
 * A problem is (table, config, 1-based start row idx0); all problems of one call share the horizon T and the grid counts.
 *   state nodes    nb x ne: Soc_b[i] = (float)(i * hb), Soc_ev[j] = (float)(j * (1.0 / (ne - 1))), the end nodes exactly soc_max and 1;
 *                  node index = i * ne + j
 *   action targets nab x nae in [0, 1]: (float)(a / (double)(count - 1)), 1 for a single point; action index = ab * nae + ae
 *   V              float64 [n_problems][T + 1][nb * ne], V_T = 0; off the nodes bilinear in float64; the maximum over the actions takes
 *                  the SMALLEST index among equal maxima. */
typedef struct shems_foresight_grid {
    int32_t nb, ne;          /* state nodes, each >= 2 (default 65 x 33: 0.5 * soc_max, the start of reset!(rng = -1), is a node) */
    int32_t nab, nae;        /* action targets, each >= 1 (default 17 x 17)                                                        */
} shems_foresight_grid;
typedef struct shems_foresight_problem {
    shems_config cfg;        /* table_row0 / nrow name the problem's table in the uploaded row array                              */
    int32_t idx0;            /* 1-based start row: idx0 >= 1 and idx0 + T <= nrow (a pass of n steps reads row n + 1)              */
    int32_t forecast_off;    /* rows from the table to its forecast table (same nrow, same row array): the forecast of table row r   */
                             /* is array row table_row0 + forecast_off + r; 0: the truth is the forecast; may be negative.  Read by  */
                             /* shems_foresight_solve_forecast_dev only: the other solve calls write 0 into the device copy.         */
    double  scale_b;         /* (nb - 1) / (double)soc_max, formed ONCE on the host in float64: the device never divides.  Filled   */
    double  hb;              /* (double)soc_max / (nb - 1).                        by shems_foresight_solve_dev in the device copy   */
} shems_foresight_problem;   /* 72 bytes */
/* The backward sweep (LU1:283-316, 343-485, 264-281; MPS:62-89): V_t(node) = max_a { reward + V_{t+1}(state') }, t = T - 1 .. 0, one
 * launch per hour on `stream` (hours are separated by launch boundaries only), grid = (node tiles, problems); no host synchronisation.
 * problems: n_problems records in HOST memory, of which cfg and idx0 are read; they are validated here, completed (scale_b, hb) and
 * copied on `stream` into d_problems, n_problems records of DEVICE memory the caller allocates: what the kernels of the sweep and
 * shems_foresight_track_dev read.  `problems` may be reused when the call returns.  d_tables [total_rows][8] as in shems_view.
 * d_V: v_doubles >= n_problems * (T + 1) * nb * ne float64 of device memory, allocated by the caller; d_argmax: int32 [n_problems][T][nb * ne] winning action indices, or NULL.
 * SHEMS_ERR_ARG, nothing launched: a grid count below its minimum (or a V plane beyond the 150 000 bytes of LDS a workgroup stages),
 * T < 1, a window running off its table, soc_max <= 0, a V buffer that is too small. */
int shems_foresight_solve_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                              shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid, int32_t T,
                              double *d_V, int64_t v_doubles, int32_t *d_argmax, void *stream);
/* The receding-horizon controller: the same recursion with a LIMITED forecast.  The reference's optimiser is parameterised for it --
 * `SHEMS python/run_SHEMS.py` builds its model with h_predict (hours forecast) and h_control (hours applied before it re-plans) and is
 * only ever run with both equal to the whole series; `horizon` and `control` restate those two parameters:
 *   horizon H >= 1          hours of forecast, the current hour included;
 *   control c, 1 <= c <= H  a fresh plan every c hours.
 * At decision hour t (0-based) the plan in force was made at j = t - t mod c and sees hours j .. hi - 1, hi = min(j + H, T); the
 * controller takes the first maximum over the action grid of reward_t + U_{t+1}(state'), U_{t+1} = the optimal value of hours
 * t + 1 .. hi - 1 with terminal value 0 (V[0] of shems_foresight_solve_dev on the window (idx0 + t + 1, hi - (t + 1)); zero when that
 * length is 0).  csrc/shems_foresight_core.h holds the definition and the schedule.  The output is laid out as solve_dev's, so
 * shems_foresight_track_dev reads it unchanged: V[p][t] = U_t for t = 1 .. T, V[p][T] = 0, V[p][0] = the value of the first plan at
 * hour 0; d_argmax[p][t][node] (or NULL) = the action the controller takes at hour t from that node.  With horizon >= T every plane
 * and index equals solve_dev's bit for bit; with horizon = 1 every plane t >= 1 is zero (the myopic controller).
 * ONE launch on `stream`, grid = (ceil(T / c) windows, problems): a workgroup runs the sweeps of its window hi - 1 .. j + 1 (and j
 * where V[p][0] or the arg-max needs it) with two V planes in LDS and stores only planes j + 1 .. min(j + c, T).  Few windows
 * (problems x windows below the CU count) under-fill the device; for horizon >= T solve_dev is the tool.
 * Arguments, validation, record completion and upload as shems_foresight_solve_dev; SHEMS_ERR_ARG, nothing launched, also for
 * horizon < 1, control < 1, control > horizon, and a grid whose TWO planes exceed 150 000 bytes of LDS (129 x 65 fits: 134 160). */
int shems_foresight_solve_horizon_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                                      shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid, int32_t T,
                                      int32_t horizon, int32_t control, double *d_V, int64_t v_doubles, int32_t *d_argmax, void *stream);
/* The forward pass (LU1:283-316, 343-485, 264-281; MPS:62-89): the greedy controller on the EXACT env, shaped like shems_track_dev --
 * one workgroup per env, all T hours in one launch.  Env e belongs to problem d_problem_of_env[e] (NULL: problem 0).  At hour t every
 * action is evaluated from the env's true (off-grid) state with the same Q as the sweep, the arg-max is taken, and the env is stepped
 * with that action through the ordinary DRL step (track > 0: penalty kept, 23-column row).  d_returns [n] float64 sums of rewards,
 * d_results [n][T][23] (results_env = -1) or [T][23] of env results_env, d_targets [n][T][2] float32 the chosen (B_target,
 * EV_target); each may be NULL.  The envs end in the state T calls of shems_step_dev with those targets leave them in.  An env whose
 * idx is not its problem's idx0 at entry (or whose problem index is outside 0 .. n_problems - 1) raises view.err = SHEMS_ERR_INDEX
 * and is not stepped. */
int shems_foresight_track_dev(const shems_view *v, const shems_foresight_problem *d_problems /* as solve_dev left them */, int32_t n_problems,
                              const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T, const double *d_V,
                              int64_t v_doubles, double *d_results, int64_t results_env, double *d_returns, float *d_targets, void *stream);
/* The receding-horizon controller planning on a FORECAST that may be wrong.  The reference's optimiser has the knobs (`SHEMS
 * python/run_SHEMS.py`: h_predict, h_control) and is only ever fed the true series; here the plan made at hour j reads the TRUE rows
 * up to j and the rows of the problem's forecast table (forecast_off above) after it: a sweep of hour t inside window j takes its
 * current row from the truth if t == j and from the forecast otherwise, its next row always from the forecast.  Everything
 * shems_foresight_solve_horizon_dev defines holds unchanged on that belief (csrc/shems_foresight_core.h: the definition and
 * fs_belief_off); with forecast_off = 0 in every record, or forecast tables that are byte copies of the truth, every plane and index
 * equals solve_horizon_dev's bit for bit.  Arguments as shems_foresight_solve_horizon_dev, but cfg, idx0 AND forecast_off of the host
 * records are read.  SHEMS_ERR_ARG, nothing launched: everything solve_horizon_dev refuses, and a forecast table that leaves the row
 * array (table_row0 + forecast_off < 0 or table_row0 + forecast_off + nrow > total_rows; the message names the problem and both row
 * numbers).  ONE launch (k_fs_window). */
int shems_foresight_solve_forecast_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                                       shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid, int32_t T,
                                       int32_t horizon, int32_t control, double *d_V, int64_t v_doubles, int32_t *d_argmax, void *stream);
/* The forward pass of that controller (LU1:283-316, 343-485; the arrival overwrite LU1:264-281): as shems_foresight_track_dev, but at
 * hour t the controller does not yet know row t + 1, so the arrival overwrite inside Q takes h_countdown and soc_ev of the next row
 * from the FORECAST row (forecast_off of the device records, as solve_forecast_dev left them); h_cur stays the truth's and the env is
 * stepped on the truth by the ordinary DRL step.  The view's row array must hold the tables the solve call saw, in the same order: an
 * env whose problem's forecast table does not lie inside view.total_rows raises view.err = SHEMS_ERR_INDEX and is not stepped, like
 * one that does not sit on its start row. */
int shems_foresight_track_forecast_dev(const shems_view *v, const shems_foresight_problem *d_problems /* as solve_forecast_dev left them */,
                                       int32_t n_problems, const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T,
                                       const double *d_V, int64_t v_doubles, double *d_results, int64_t results_env, double *d_returns,
                                       float *d_targets, void *stream);
/* The forward pass of the same controller HEDGING over K forecasts (LU1:283-316, 343-485; the arrival overwrite LU1:264-281).  An
 * ensemble problem is one truth (cfg, idx0) with n_scen scenarios, each a forecast table as above with a float64 weight; d_problems
 * holds n_problems * n_scen records, problem-major, scenario-minor, and d_V their planes, as ONE shems_foresight_solve_forecast_dev
 * call over those records left them (no new sweep).  At hour t every action is stepped once from the true state; its value is
 * reward + sum_k w[k] * U^k_{t+1}(Soc_b', Soc_ev'^k), the sum taken in scenario order from +0.0 and the arrival overwrite of scenario k
 * read from ITS row t + 1; the first maximum wins and the env is stepped on the truth (csrc/shems_foresight_core.h: the definition,
 * fs_step / fs_q_ens, and why this two-stage programme is optimistic about what is learnt after the first stage).  With n_scen = 1
 * and weight 1.0 every byte equals shems_foresight_track_forecast_dev's on the same record.
 * weights: HOST [n_problems][n_scen], validated here, copied on `stream` into d_weights (DEVICE, same size, caller-allocated) and read
 * there by the kernel; they are used as given (the caller normalises them to sum 1).  The other arguments as
 * shems_foresight_track_forecast_dev; d_problem_of_env names the PROBLEM (0 .. n_problems - 1), not the record.  ONE launch
 * (k_fs_track_ens), one workgroup per env, no host synchronisation.  An env that does not sit on idx0 of its problem, whose problem's
 * n_scen records do not all carry that idx0, table_row0 and nrow, or one of whose scenario tables leaves view.total_rows raises
 * view.err = SHEMS_ERR_INDEX and is not stepped.  SHEMS_ERR_ARG, nothing launched: everything track_forecast_dev refuses, n_scen
 * outside 1 .. 16, a NULL weight buffer, a weight that is not finite or is <= 0 (the message names the problem and the scenario),
 * v_doubles < n_problems * n_scen * (T + 1) * nb * ne. */
int shems_foresight_track_ensemble_dev(const shems_view *v, const shems_foresight_problem *d_problems /* n_problems * n_scen records as
                                       solve_forecast_dev left them */, int32_t n_problems, int32_t n_scen, const double *weights
                                       /* HOST [n_problems][n_scen] */, double *d_weights /* DEVICE, same size, caller-allocated */,
                                       const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T, const double *d_V,
                                       int64_t v_doubles, double *d_results, int64_t results_env, double *d_returns, float *d_targets,
                                       void *stream);
/* The audit of tracked passes: where does a pass lose against V?  Q_t(state, a) = reward of step! (LU1:283-316, 343-485; the arrival
 * overwrite LU1:264-281) + V_{t+1}(state') is evaluated over the whole action grid from the state a pass was ACTUALLY in, read back from
 * the reference's 23-column result rows (LU1:476-478; MPS:62-89), whichever controller made them.  csrc/shems_foresight_core.h holds
 * the definition (row check, state, best_q / achieved_q / v_state, the telescoping identity, and why regret is not a bound).
 * d_tables / total_rows: the row array the solve call saw; d_problems / n_problems / grid / T / d_V / v_doubles: as that call left
 * them (planes solved on a forecast table have no audit: the host layer refuses them); d_results [n_pass][T][23] float64;
 * d_problem_of_pass [n_pass] int32, or NULL: problem 0.  Outputs, all device memory of the caller: d_out [n_pass][T][3] float64
 * {best_q, achieved_q, v_state}, d_best_action [n_pass][T] int32, d_status [n_pass] int32 -- 0, or SHEMS_ERR_INDEX when a row of the pass
 * does not sit on table row idx0 + t or d_problem_of_pass names no problem; the offending hours hold NaN and -1, the others are
 * audited.  d_status is zeroed on `stream`, then ONE launch, grid = (tiles of 4 hours, passes), a wave per hour, the actions over its
 * lanes; no host synchronisation.  SHEMS_ERR_ARG, nothing launched: what solve_dev refuses of the grid, T < 1, n_problems < 1,
 * n_pass outside 1 .. 65535, a V buffer that is too small, a NULL where a buffer is required. */
int shems_foresight_audit_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems, int32_t n_problems,
                              const shems_foresight_grid *grid, int32_t T, const double *d_V, int64_t v_doubles, const double *d_results,
                              int32_t n_pass, const int32_t *d_problem_of_pass, double *d_out, int32_t *d_best_action, int32_t *d_status,
                              void *stream);
/* Demonstrations from tracked passes: the 23-column rows (LU1:476-478; MPS:62-89) of ANY pass plus a label per hour become
 * (observation, action) pairs in a replay ring, for the supervised update of the actor (shems_ddpg_clone_update).  The definition --
 * fs_demo_hour: the audit's row check and state, observations 6 .. 8 from table row idx as reset! / next_state! leave them
 * (LU1:264-281), the label a = (float)(2.0 * (double)target - 1.0) -- is in csrc/shems_foresight_core.h.
 * d_tables / total_rows / d_problems / n_problems / grid / T / d_results / n_pass / d_problem_of_pass: as shems_foresight_audit_dev
 * takes them (no V is read).  Exactly one label source: d_targets [n_pass][T][2] float32 in [0, 1], as shems_foresight_track_dev
 * writes them, or d_best_action [n_pass][T] int32 action indices, as the audit writes them (the labels at the states ANOTHER
 * controller visited).  Pass e, hour t goes to slot (pos + e * T + t) mod ring->capacity; only s and a of that slot are written,
 * r, s2 and done are not touched.  An hour whose row check fails or whose index label is not an action of the grid (the audit's
 * -1) leaves its slot untouched and sets d_status[e] = SHEMS_ERR_INDEX; the other hours are written.  d_status [n_pass] int32 is
 * zeroed on `stream`, then ONE launch (k_fs_demos, a thread per hour); no host synchronisation.  SHEMS_ERR_ARG, nothing launched:
 * what the audit refuses of the grid, T and n_pass, a NULL where a buffer is required, both label sources or neither,
 * n_pass * T > capacity, pos outside 0 .. capacity - 1. */
int shems_foresight_demos_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems, int32_t n_problems,
                              const shems_foresight_grid *grid, int32_t T, const double *d_results, int32_t n_pass,
                              const int32_t *d_problem_of_pass, const float *d_targets, const int32_t *d_best_action,
                              const shems_replay *ring, int64_t pos, int32_t *d_status, void *stream);
/* Transitions from tracked passes: the rows of DRL-mode passes become full replay slots (s, a, r, s', done), so that a ring can be
 * seeded and a critic fitted from passes that are tracked anyway (shems_ddpg_critic_update).  The definition -- fs_transition_hour,
 * fs_returns -- is in csrc/shems_foresight_core.h: s and s' are the observations of rows t and t + 1, a the labels of the targets the
 * rows record (columns 21 and 2), r = (float)reward; the return-to-go is G[T - 1] = r[T - 1], G[t] = r[t] + (double)gamma * G[t + 1]
 * in float64, in that order.  Rows of a RULE-BASED pass record no targets: they would give wrong actions, and nothing checks it.
 * mode SHEMS_FS_TRANS_TD: the slot holds (s, a, r, s', 0).  SHEMS_FS_TRANS_MC: it holds (s, a, (float)G[t], s', 1), so that the update's
 * y = r + gamma (1 - done) q' is G[t] and no network is bootstrapped from.  tail (1 .. T - 1): hours t >= T - tail give no transition
 * (G still sums over all T hours); pass e, hour t goes to slot (pos + e * (T - tail) + t) mod ring->capacity.
 * d_returns [n_pass][T] float64 receives G (required for MC, optional for TD).  TD: an hour whose row check (hour t or t + 1) fails or
 * whose reward is not finite leaves its slot untouched and sets d_status[e] = SHEMS_ERR_INDEX; the other hours are written.  MC: a pass
 * any of whose T hours fails gives no transition, its status is set and its row of d_returns holds NaN.  d_status [n_pass] int32 is
 * zeroed on `stream`, then k_fs_returns (only with d_returns: a wave per pass) and k_fs_transitions (a thread per hour); no host
 * synchronisation.  SHEMS_ERR_ARG, nothing launched: T < 2, tail outside 1 .. T - 1, an unknown mode, MC without d_returns, gamma
 * outside [0, 1] or not finite, a ring without all five arrays, n_pass * (T - tail) > capacity, pos outside the ring, n_pass outside
 * 1 .. 65535, a NULL where a buffer is required. */
enum { SHEMS_FS_TRANS_TD = 0, SHEMS_FS_TRANS_MC = 1 };
int shems_foresight_transitions_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems,
                                    int32_t n_problems, int32_t T, const double *d_results, int32_t n_pass,
                                    const int32_t *d_problem_of_pass, int32_t mode, float gamma, int32_t tail, double *d_returns,
                                    const shems_replay *ring, int64_t pos, int32_t *d_status, void *stream);

/* ------------------------------------------ multi-step (n-step) returns -- */
/* n-step transitions (s_t, a_t, G_t, s_{t+n}) with G_t = sum_{k<n} gamma^k r_{t+k} and y = G + gamma^n q'(s_{t+n}), as in Rainbow and
 * D4PG (csrc/shems_nstep_core.h holds the arithmetic).  They change only what a ring holds: every update entry point
 * reads such a ring as any other and receives gamma_n in its `gamma` field.
 *   Full windows only.  The env has no terminal state, so an episode of T hours contributes the T - n + 1 transitions that start at
 *     hours 0 .. T - n.  The last n - 1 hours start no transition; their rewards do enter the earlier windows.  Episode starts are drawn
 *     over the whole table, so no table row is lost as a start state.  Every stored transition has the same discount gamma^n.
 *   History is per episode: a window never spans a reset.
 *   The return is evaluated from the ring's own Float32(reward) values by Horner's rule in float64, newest first:
 *       acc = (double) r_{t+n-1};   for k = n-2 .. 0: acc = (double) r_{t+k} + (double) gamma32 * acc;   G32 = (float) acc
 *     (rounded product, then add: no fma; the unit is built with -ffp-contract=off).  gamma32 is the Float32 one-step discount.
 *   The discount is computed on the host, once: gamma_n = float32(g64 * g64 * ... * g64), g64 = float64(gamma32), n factors multiplied
 *     left to right in float64.  There is no device pow.
 *   done of an emitted transition is the newest one-step transition's byte (always 0 in this env).
 *   1 <= n <= SHEMS_NSTEP_MAX and n <= T.  n = 1 reproduces the one-step ring's bytes.
 *
 * The fold, per vector step: the unchanged fused step writes its one-step transitions of the STATIONARY window of households
 * [0, window) -- shems_ring_window{0, window, 0} -- into a staging shems_replay of capacity >= window (slot j = household j).
 * shems_nstep_fold_dev then stores (s, a, r) of hour `hour` (counted from the episode's reset) into history slot hour mod n and, for
 * hour >= n - 1, emits (hist_s[o], hist_a[o], G, stage.s2, stage.done), o = (hour + 1) mod n, of household j into ring slot
 * (ring_pos + j) mod capacity; for hour < n - 1 it emits nothing (the caller advances its push counter by `window` only when
 * hour >= n - 1).  One launch, threads flat over the window's elements.  SHEMS_ERR_ARG, nothing launched: n outside 1 ..
 * SHEMS_NSTEP_MAX, window < 1, hour < 0, ring_pos < 0, a NULL, a ring or staging ring without all five arrays or smaller than the
 * window. */
#define SHEMS_NSTEP_MAX 16
typedef struct shems_nstep {
    int32_t  n;              /* steps per return, 1 .. SHEMS_NSTEP_MAX                  */
    int32_t  reserved;
    int64_t  window;         /* households folded per step                               */
    float    gamma;          /* gamma32: the Float32 ONE-step discount                   */
    int32_t  reserved2;
    float   *hist_s;         /* dev [n][window][9]                                       */
    float   *hist_a;         /* dev [n][window][2]                                       */
    float   *hist_r;         /* dev [n][window]                                          */
} shems_nstep;
int shems_nstep_fold_dev(const shems_nstep *ns, const shems_replay *stage, const shems_replay *ring, int64_t ring_pos, int32_t hour,
                         void *stream);
/* The same for every learner of a group in ONE launch: learner l's history, staging and ring arrays lie at learner 0's pointers
 * + l * g->stride_bytes.  d_gamma1: dev float [g->count] of one-step discounts; NULL = ns0->gamma for all learners. */
int shems_nstep_group_fold_dev(const shems_nstep *ns0, const shems_replay *stage0, const shems_replay *ring0, const shems_group *g,
                               const float *d_gamma1, int64_t ring_pos, int32_t hour, void *stream);
/* The bulk form, for populate_memory: src holds episode e's hour t at slot e * steps + t (what shems_rollout_dev writes into a ring of
 * that capacity from position 0).  With m = steps - n + 1, transition (e, t), t < m, goes to slot (ring_pos + e * m + t) mod capacity;
 * pushes that a later push of the same call would overwrite (order < episodes * m - capacity) are skipped, as in shems_rollout_dev.
 * The caller advances its push counter by episodes * m.  SHEMS_ERR_ARG: n outside 1 .. SHEMS_NSTEP_MAX, steps < n, episodes < 1, a
 * source smaller than episodes * steps, src and ring the same arrays. */
int shems_nstep_from_episodes_dev(const shems_replay *src, int64_t episodes, int64_t steps, int32_t n, float gamma,
                                  const shems_replay *ring, int64_t ring_pos, void *stream);

/* ------------------------------------------ population-based training of a learner group -- */
/* Exploit and explore (Jaderberg et al. 2017) on the device, after an evaluation sweep (csrc/shems_pbt_core.h holds the
 * arithmetic once for host and device).  A POPULATION is the set of learners with the same id in pop[count]; selection never crosses
 * populations.  One ROUND, per population of size P with quota q = (P * permille) / 1000 in integers (permille 1 .. 500, so 2 q <= P):
 *   order    a is better than b if a's score is finite and b's is not, or both are finite and score_a > score_b; on equal scores, or
 *            two non-finite ones, the lower learner index is better.  rank[l] = learners of l's population that are better than l.
 *   exploit  learners with rank >= P - q are children.  Child l draws ONE Philox4x32-10 block, counter (l, round, 0, kStreamPbt), key =
 *            the two halves of seed (low word first); its parent is the learner of rank j = (uint64(x) * q) >> 32 of its population
 *            (always one of the q best).  A parent whose score is not finite: the child keeps itself.  parent[l] = l for every kept
 *            learner; q = 0 changes nothing.  Parents and children are disjoint sets, so nothing is read and written in one round.
 *   explore  the child's record becomes the parent's WHOLE record (eta_*, gamma, tau, noise_mu, noise_sigma, batch); then, for every
 *            field enabled in `fields`, one bit of the block's word y picks the factor f -- set: up, clear: down:
 *                eta' = (double)(float)(eta * f)      (eta is the Float64 value of a Float32)
 *                x'   = (float)((double) x * f)       (tau, noise_sigma)
 *            and the result is clamped to [lo, hi] of that field.  A parent's record is never written in the round.
 * What the copy moves from parent to child is the caller's list of ranges of a learner's slab; the Python group copies the
 * parameters, targets, ADAM moments and tiled regions, s_min and s_max -- never the ring, the priorities, the n-step history, the
 * gradients, the workspaces or the random streams. */
#define SHEMS_PBT_FIELDS 4
#define SHEMS_PBT_MAX_RANGES 8
#define SHEMS_PBT_MAX_COUNT 4096     /* select: the counting loops are O(count^2) per child */
#define SHEMS_PBT_CHUNK_VECS 2048    /* copy: 16-byte vectors one workgroup moves (32 KB)     */
enum { SHEMS_PBT_ETA_ACT = 1, SHEMS_PBT_ETA_CRIT = 2, SHEMS_PBT_TAU = 4, SHEMS_PBT_SIGMA = 8 };
typedef struct shems_pbt_params {
    uint64_t seed;                       /* Philox key                                              */
    uint32_t round;                      /* counter word 1: a round never repeats a draw            */
    int32_t  permille;                   /* truncation in thousandths, 1 .. 500                     */
    uint32_t fields;                     /* SHEMS_PBT_* bits: the fields explore perturbs           */
    int32_t  reserved;                   /* 0                                                       */
    double   down, up;                   /* the two factors, finite and > 0                         */
    double   lo[SHEMS_PBT_FIELDS];       /* clamp bounds per field, in the order of the bits        */
    double   hi[SHEMS_PBT_FIELDS];
} shems_pbt_params;                      /* 104 bytes */
typedef struct shems_pbt_range {
    int64_t offset_floats;               /* from the start of a learner's slab; a multiple of 4     */
    int64_t floats;                      /* a multiple of 4; 0 = nothing                            */
} shems_pbt_range;
/* Host only: permille in 1 .. 500, no unknown bit in fields, reserved 0, down and up finite and > 0, and for all four fields lo <= hi,
 * both finite Float32 values under which a clamped value passes shems_group_hparams_check: eta lo > 0, tau in (0, 1], sigma lo >= 0.
 * SHEMS_ERR_ARG names the first bad item. */
int shems_pbt_params_check(const shems_pbt_params *params);
/* k_pbt_select, one thread per learner: rank, parent and the children's new records IN PLACE in d_hp; d_parent and d_rank [count] int32
 * receive every learner's parent and rank.  d_pop [count] int32, d_score [count] double, d_hp [count] records, all device memory; params
 * is host memory.  SHEMS_ERR_ARG, nothing launched: a NULL, count outside 1 .. SHEMS_PBT_MAX_COUNT, whatever shems_pbt_params_check
 * refuses, d_hp or d_score not 8-byte aligned, d_pop / d_parent / d_rank not 4-byte aligned. */
int shems_pbt_select_dev(const shems_pbt_params *params, int32_t count, const int32_t *d_pop, const double *d_score,
                         shems_group_hparams *d_hp, int32_t *d_parent, int32_t *d_rank, void *stream);
/* k_pbt_copy: for every learner l with d_parent[l] != l, the `n_ranges` ranges (HOST array, passed to the kernel by value) are copied
 * from slab0 + parent * g->stride_bytes to slab0 + l * g->stride_bytes.  grid = (chunks of SHEMS_PBT_CHUNK_VECS vectors over the
 * concatenated ranges, learner); a kept learner's workgroups exit at once; the others move 16-byte vectors with non-temporal loads and
 * stores.  No LDS, no atomics.  A d_parent entry outside 0 .. count - 1, or one that names a learner which is itself a child, leaves that
 * learner untouched (no slab is read and written in one launch).  SHEMS_ERR_ARG, nothing launched: a NULL, g->count outside 1 .. 65535,
 * stride_bytes not a positive multiple of 16, slab0 not 16-byte aligned, n_ranges outside 1 .. SHEMS_PBT_MAX_RANGES, a range with a
 * negative number or one that is no multiple of 4, a range past stride_bytes, all ranges empty. */
int shems_pbt_copy_dev(float *slab0, const shems_group *g, const shems_pbt_range *ranges, int32_t n_ranges, const int32_t *d_parent,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHEMS_HIP_H */
