/*
 * amx_hip.h — C ABI of the MI355X-native learned-dynamics rollout engine.
 *
 * This is the drop-in boundary for ONE hot path of dhruvsreenivas/amp_extensions:
 * the gym_simenv learned-dynamics step (4-model dense-MLP ensemble), the MILO
 * random-Fourier-feature MMD cost + ensemble-disagreement bonus, the AMP/GAIL
 * least-squares discriminator reward and the humanoid3d fall/horizon termination.
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference repository root).
 *
 * Conventions
 *   - Every buffer argument is a DEVICE pointer owned by the caller, except where a
 *     comment says "host".  Nothing is retained after a call returns, except the
 *     small configuration copied by amx_set_* into context-owned device memory.
 *   - Every launching call takes a hipStream_t (passed as void* so this header
 *     needs no HIP include) and is asynchronous on it.  No call allocates, frees
 *     or synchronises on the launch path, so a caller may capture them in a graph.
 *   - Return value: AMX_OK (0) or a negative AMX_E_* code.  No exception crosses
 *     the ABI.  amx_last_error() returns a thread-local message for the last
 *     failing call on the calling thread.
 *   - Thread safety: one amx_ctx per device; calls on one context are not
 *     re-entrant; distinct contexts/devices are independent.
 *   - Row padding: GEMM operands/outputs have a row count that is a multiple of
 *     AMX_ROW_TILE (128); K of every GEMM is a multiple of AMX_K_TILE (32); leading
 *     dimensions are multiples of 4 floats; pointers are 16-byte aligned.
 *     amx_layout() reports the padded widths the engine expects.
 */
#ifndef AMX_HIP_H
#define AMX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMX_ABI_VERSION 2
#define AMX_ROW_TILE 128
#define AMX_K_TILE 32
#define AMX_MAX_MODELS 8
#define AMX_MAX_BODIES 32
#define AMX_MT_STATE_BYTES 2512  /* one numpy-legacy MT19937 state (amx_mt_seed) */

enum {
  AMX_OK = 0,
  AMX_E_INVAL = -1,   /* bad argument (shape, alignment, null pointer) */
  AMX_E_HIP = -2,     /* HIP runtime error (launch, memcpy) */
  AMX_E_NOMEM = -3,   /* device allocation failed */
  AMX_E_STATE = -4    /* context not configured for this call */
};

enum { AMX_SHAPE_SPHERE = 0, AMX_SHAPE_CAPSULE = 1, AMX_SHAPE_BOX = 2 };
enum { AMX_ACT_NONE = 0, AMX_ACT_RELU = 1 };
enum { AMX_IN_F64 = 0, AMX_IN_F32 = 1 };
enum { AMX_DISC_LEAST_SQUARES = 0, AMX_DISC_LOG_LIKELIHOOD = 1 };

typedef struct amx_ctx amx_ctx;

/* ---- context ------------------------------------------------------------------ */

/* Replaces the sizes SimEnv/DynamicsEnsemble read at construction:
 * gym-simenv/gym_simenv/envs/sim_env.py:66-67 (state/action size),
 * milo/milo/dynamics.py:19-79 (num_models, hidden_sizes) and
 * milo/milo/linear_cost.py:23-62 (feature_dim).  n_hidden hidden layers of width
 * `hidden`, dense-connected (BasicMLP, milo/milo/dynamics.py:394-433). */
amx_ctx* amx_create(int device, int S, int A, int n_models, int hidden, int n_hidden, int feat_dim);
/* amx_create with the network's connectivity: AMX_CONNECT_DENSE (amx_create's) or
 * AMX_CONNECT_PLAIN, BasicMLP(dense_connect=False): hidden layer i >= 1 reads layer i-1's output
 * only and the output layer the last hidden one (n_hidden >= 1).  The activation rows keep the
 * dense-concat form [x0 | h0 | h1 | ...] of amx_layout; a plain layer reads the K window
 * [k0_pad + (i-1) hidden, k0_pad + i hidden) of them against a [hidden][hidden] weight (the
 * output layer: [n_out_pad][hidden]).  The connectivity sets what amx_efit_param_count,
 * amx_efit_work_floats, amx_efit_step and amx_split_workspace_floats answer and run. */
enum { AMX_CONNECT_DENSE = 0, AMX_CONNECT_PLAIN = 1 };
amx_ctx* amx_create_ex(int device, int S, int A, int n_models, int hidden, int n_hidden, int feat_dim,
                       int connect);
int amx_destroy(amx_ctx* ctx);
const char* amx_last_error(void);
int amx_abi_version(void);

/* Padded layout the engine expects (host outputs):
 *   k0_pad   = round_up(S + A, 32)   width of the [s~, a~] block of the activation row
 *   ldk      = k0_pad + n_hidden*hidden  activation row length (dense-concat buffer)
 *   n_out_pad= round_up(S, 128)      output rows of the padded last-layer weight
 *   k_rff_pad= round_up(2*S, 32)     width of the float32 [s, s'] cost input row   */
int amx_layout(const amx_ctx* ctx, int* k0_pad, int* ldk, int* n_out_pad, int* k_rff_pad);

/* Normalizers (host pointers, copied).  Contract of AmpDataset.get_transformations,
 * milo/milo/datasets.py:23-43: means and mean-absolute-deviation+1e-8 scales, in
 * the order DynamicsModel.forward consumes them (milo/milo/dynamics.py:225-232). */
int amx_set_normalizers(amx_ctx* ctx, const float* mu_s, const float* sd_s, const float* mu_a,
                        const float* sd_a, const float* mu_d, const float* sd_d);

/* Fall-termination configuration (host pointers, copied).  Replaces SimEnv.__init__'s
 * fall-body tables and ctrl flags, gym-simenv/gym_simenv/envs/sim_env.py:83-115, and
 * is_done/check_velocity's parameters, :164-173, :259-268.  body_id[i] is the
 * character body index; p0/p1 are BodyDefs Param0/Param1 (radius = 0.5*p0, capsule
 * height = p1).  pos_dim/rot_dim: per-body pose feature widths (3 and 6).  With
 * vel_check and record_vel_as_pos every checked body element must lie below vel_offset
 * (check_collision reads ob before check_velocity rescales ob[vel_offset:], :171-172). */
int amx_set_termination(amx_ctx* ctx, int n_bodies, const int32_t* body_id, const int32_t* shape,
                        const double* p0, const double* p1, int record_all_world,
                        int record_world_root_pos, int pos_dim, int rot_dim, int horizon,
                        int vel_check, int vel_offset, double vel_thresh, int record_vel_as_pos,
                        double sampling_rate);

/* ---- ensemble forward --------------------------------------------------------- */

/* State assembly for DynamicsModel.forward, milo/milo/dynamics.py:216-230:
 * x0 = [(float(s)-mu_s)/sd_s, (float(a)-mu_a)/sd_a, 0-pad] written at column 0 of
 * every model's activation row (act_buf[m][b][0:k0_pad], m < n_models).
 * in_dtype = AMX_IN_F64 (SimEnv's float64 ob, sim_env.py:155-156) or AMX_IN_F32. */
int amx_assemble_input(amx_ctx* ctx, const void* ob, const void* act, int in_dtype, float* act_buf,
                       long long stride_m, int ldk, int B, void* stream);
/* The same assembly for the f16x3 GEMM path: also writes slot 0 of the row exponents
 * (row_exp[m][slot][b], slot stride slot_stride >= B, model stride strideRexp; the layout of
 * amx_row_exponents) from max |x0| and resets slots 1..n_slots-1, for rows b < B.
 * stride_m = 0: x0 is written once (model 0's rows) and the f16x3 GEMMs read it for every
 * model (their k_shared); the exponent slots are still written for every model.
 * Member-blocked layout (slot_stride = Bq < B, stride_m = 0, B = M' x Bq with M' <= M): lane b
 * belongs to member block g = b / Bq (the sampler's one-member-per-lane forward), its x0 is row b
 * and its exponents go to row b % Bq of block g's slots only (g * strideRexp + slot * Bq). */
int amx_assemble_input_rexp(amx_ctx* ctx, const void* ob, const void* act, int in_dtype, float* act_buf,
                            long long stride_m, int ldk, int B, int* row_exp, long long strideRexp,
                            long long slot_stride, int n_slots, void* stream);

/* Grouped fp32 GEMM on MFMA with fused bias (+ReLU) epilogue: for g < groups,
 * C_g[r][col_off + n] = act(sum_k A_g[r][k] * W_g[n][k] + bias_g[n]).
 * One dense-connect hidden layer of all ensemble members at once
 * (BasicMLP.forward, milo/milo/dynamics.py:427-430: relu(fc(x)); x = cat[x, h]);
 * also the Discriminator hidden layers, milo/milo/gail_cost.py:18-42.
 * rows % 128 == 0, N % 128 == 0, K % 32 == 0. */
int amx_gemm_bias_act(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                      long long strideA, const float* W, int ldw, long long strideW,
                      const float* bias, long long strideBias, float* C, int ldc, long long strideC,
                      int col_off, int act, void* stream);

/* The same GEMM on 64 x 64 tiles (bit-identical results: every output element runs the same K
 * chain): four times the workgroups of amx_gemm_bias_act, for the few hundred rows of a training
 * step (amx_efit_step's forward), where 128 x 128 tiles leave most of the chip idle.
 * rows % 128 == 0, N % 64 == 0, K % 32 == 0. */
int amx_gemm_bias_act_t64(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                          long long strideA, const float* W, int ldw, long long strideW,
                          const float* bias, long long strideBias, float* C, int ldc,
                          long long strideC, int col_off, int act, void* stream);

/* Last dense layer + output un-normalisation (BasicMLP.forward :432 then
 * DynamicsModel.forward :231-232): preds_g[r][n] = (sum_k A W + b[n]) * sd_d[n] + mu_d[n]
 * for n < n_valid (=S); W_g is padded to round_up(n_valid,128) rows. */
int amx_gemm_out_unnorm(amx_ctx* ctx, int groups, int rows, int n_valid, int K, const float* A,
                        int lda, long long strideA, const float* W, int ldw, long long strideW,
                        const float* bias, long long strideBias, float* preds, int ldp,
                        long long strideP, void* stream);

/* ---- bf16x6: the same fp32 GEMMs on the bf16 matrix pipe ------------------------
 * Each fp32 operand is split exactly into three bf16 limbs (x = x0 + x1 + x2) and a*b is
 * summed as the six limb products of degree <= 2 in fp32 MFMA accumulators: fp32-level
 * error (the dropped terms are <= 2^-23 |ab|), 2.67x fewer matrix-pipe cycles than the f32
 * MFMA.  Same semantics, layouts and epilogues as amx_gemm_bias_act / amx_gemm_out_unnorm
 * (BasicMLP.forward, milo/milo/dynamics.py:422-433 + DynamicsModel.forward :231-232); only
 * the weight operand differs: W3 is the image written by amx_split_bf16x3.  K % 16 == 0.
 *
 * amx_split_bf16x3: W [groups][rows][K] fp32 (row stride ldw, group stride strideW) ->
 * W3 [groups][rows][K/16][3][16] bf16 bits (row stride 3K, group stride strideW3). */
int amx_split_bf16x3(amx_ctx* ctx, int groups, int rows, int K, const float* W, int ldw,
                     long long strideW, uint16_t* W3, long long strideW3, void* stream);
int amx_gemm_bias_act_x6(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                         long long strideA, const uint16_t* W3, long long strideW3, const float* bias,
                         long long strideBias, float* C, int ldc, long long strideC, int col_off,
                         int act, void* stream);
int amx_gemm_out_unnorm_x6(amx_ctx* ctx, int groups, int rows, int n_valid, int K, const float* A,
                           int lda, long long strideA, const uint16_t* W3, long long strideW3,
                           const float* bias, long long strideBias, float* preds, int ldp,
                           long long strideP, void* stream);

/* bf16x6 form of amx_rff_features (RBFLinearCost.get_rep, milo/milo/linear_cost.py:64-71):
 * W3 = amx_split_bf16x3 image of the [F][K] RFF weight; same epilogue and outputs. */
int amx_rff_features_x6(amx_ctx* ctx, int rows, int n_valid, int F, int K, const float* x, int ldx,
                        const uint16_t* W3, const float* b, float scale, float* phi, int ldphi,
                        double* col_partials, const uint8_t* row_mask, void* stream);

/* ---- f16x3: the same fp32 GEMMs as two scaled fp16 limbs, three products ---------------
 * Each fp32 operand is scaled by a power of two (per weight row / per activation row) and
 * split into two fp16 limbs (11 + 11 significant bits); a*b = a0b0 + a0b1 + a1b0 in fp32
 * MFMA accumulators.  The per-term error (<= ~2^-22 |ab|) adds up like sqrt(K) while the
 * fp32 accumulation's grows like K, so the GEMM error equals an fp32 GEMM's for K >= ~64
 * (tools/x6_accuracy.py); 3 MFMA per 32x32x16 block instead of bf16x6's 6.  Same
 * semantics, layouts and epilogues as amx_gemm_bias_act / amx_gemm_out_unnorm
 * (BasicMLP.forward, milo/milo/dynamics.py:422-433 + DynamicsModel.forward :231-232).
 *
 * amx_split_f16x2: W [groups][rows][K] fp32 -> W2 [groups][rows][K/16][2][16] fp16 bits
 * (row stride 2K) scaled by 2^(14 - E_r), E_r = w_exp[g][r] (max_k |W| < 2^E_r).
 * Row exponents of A: row_exp [groups][slots][rows] int32 (group stride strideRexp, slot
 * stride = rows); a GEMM scales row r by 2^(14 - max over slots 0..rexp_slots-1).
 * amx_row_exponents writes slot 0 from A's first K columns and resets slots 1..n_slots-1;
 * amx_gemm_bias_act_h3 with row_exp_out (the slot of the columns it writes; nullable)
 * max-es the exponents of its output rows into it, so a dense-concat chain of layers
 * (layer i reads slots 0..i, writes slot i+1) needs no other pass.  K % 16 == 0.
 * k_shared (multiple of 32, 0 = off): A's first k_shared columns are read from group 0's rows
 * for every group -- the ensemble's x0 slice assembled once (amx_assemble_input_rexp with
 * stride_m = 0) instead of one copy per model; each group's row_exp slot 0 still holds its
 * exponents. */
int amx_split_f16x2(amx_ctx* ctx, int groups, int rows, int K, const float* W, int ldw,
                    long long strideW, uint16_t* W2, long long strideW2, int* w_exp,
                    long long strideWexp, void* stream);
int amx_row_exponents(amx_ctx* ctx, int groups, int rows, int K, const float* A, int lda,
                      long long strideA, int* row_exp, long long strideRexp, int n_slots,
                      void* stream);
int amx_gemm_bias_act_h3(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                         long long strideA, const uint16_t* W2, long long strideW2, const int* w_exp,
                         long long strideWexp, const float* bias, long long strideBias, float* C,
                         int ldc, long long strideC, int col_off, int act, const int* row_exp,
                         long long strideRexp, int rexp_slots, int* row_exp_out, int k_shared,
                         void* stream);
int amx_gemm_out_unnorm_h3(amx_ctx* ctx, int groups, int rows, int n_valid, int K, const float* A,
                           int lda, long long strideA, const uint16_t* W2, long long strideW2,
                           const int* w_exp, long long strideWexp, const float* bias,
                           long long strideBias, float* preds, int ldp, long long strideP,
                           const int* row_exp, long long strideRexp, int rexp_slots, int k_shared,
                           void* stream);

/* The windowed forms, for a plain (AMX_CONNECT_PLAIN) chain: A points at the K window the layer
 * reads (row stride lda still the whole activation row) and the rows are scaled by the one
 * exponent slot `rexp_first` of that window, not by a max over leading slots (row_exp is the
 * base of the [groups][slots][rows] table, strideRexp >= (rexp_first + 1) rows).  `first_layer`
 * (0 / 1) marks the launch at which amx_set_gemm_timer's forward starts; the two-argument
 * forms infer it from rexp_slots == 1, which in a plain chain holds for every layer.  Same
 * tiles, epilogues and split workspace as the forms above (no k_shared: a window past x0 is
 * every group's own). */
int amx_gemm_bias_act_h3_win(amx_ctx* ctx, int groups, int rows, int N, int K, const float* A, int lda,
                             long long strideA, const uint16_t* W2, long long strideW2, const int* w_exp,
                             long long strideWexp, const float* bias, long long strideBias, float* C,
                             int ldc, long long strideC, int col_off, int act, const int* row_exp,
                             long long strideRexp, int rexp_first, int* row_exp_out, int first_layer,
                             void* stream);
int amx_gemm_out_unnorm_h3_win(amx_ctx* ctx, int groups, int rows, int n_valid, int K, const float* A,
                               int lda, long long strideA, const uint16_t* W2, long long strideW2,
                               const int* w_exp, long long strideWexp, const float* bias,
                               long long strideBias, float* preds, int ldp, long long strideP,
                               const int* row_exp, long long strideRexp, int rexp_first, void* stream);

/* f16x3 form of amx_rff_features (RBFLinearCost.get_rep, milo/milo/linear_cost.py:64-71):
 * W2/w_exp = amx_split_f16x2 image of the [F][K] RFF weight, row_exp [rows] = exponents of x's
 * rows (amx_step_rexp, or amx_row_exponents with one slot); same epilogue and outputs. */
int amx_rff_features_h3(amx_ctx* ctx, int rows, int n_valid, int F, int K, const float* x, int ldx,
                        const uint16_t* W2, const int* w_exp, const int* row_exp, const float* b, float scale,
                        float* phi, int ldphi, double* col_partials, const uint8_t* row_mask, void* stream);

/* The feature layer of the MLP-feature MMD cost (MLPCost.get_rep, milo/milo/linear_cost.py:232-237:
 * the net's last Linear, its closing Tanh, then torch.cos(.) * np.sqrt(2/F)): amx_rff_features_h3's
 * arguments, layouts, tile dispatch and outputs (phi rows, one fp64 column partial per
 * AMX_RFF_PART_ROWS rows over the rows below n_valid with row_mask != 0) with
 * phi = cos(tanh(x W^T + b)) * scale, the scalar function evaluated in fp64 and rounded once.
 * x = the last hidden layer's rows (amx_gemm_bias_act_h3 writes their exponents: row_exp_out). */
int amx_mlp_features_h3(amx_ctx* ctx, int rows, int n_valid, int F, int K, const float* x, int ldx,
                        const uint16_t* W2, const int* w_exp, const int* row_exp, const float* b, float scale,
                        float* phi, int ldphi, double* col_partials, const uint8_t* row_mask, void* stream);

/* SimEnv's reset noise (reset_args noise_bef_rot, noise_min, noise_max, radian, rot_vel_w_pose,
 * vel_noise, interp, knee_rot; run.py:113-117) = DeepMimicCore's cKinCharacter::AddNoise
 * (anim/KinCharacter.cpp:340-470) applied to the kinematic pose / velocity at the reset time.
 * The draws come from Philox (the C++ core's std::default_random_engine stream cannot be
 * reproduced) or, for tests, from an injected [B][ld_draws] table of uniforms in [0, 1):
 * RandomRotatePoseVel's draws at [0, AMX_NOISE_ROT_SLOTS), AddNoisePoseVel's (pose elements,
 * then velocity elements) after them. */
#define AMX_NOISE_ROT_SLOTS 48
typedef struct amx_reset_noise {
  int noise_bef_rot;
  double noise_min, noise_max, radian;
  int rot_vel_w_pose, vel_noise;
  double interp;
  int knee_rot;
} amx_reset_noise;
int amx_motion_states_noise(amx_ctx* ctx, const double* times, int B, int flags, const amx_reset_noise* noise,
                            const double* draws, long long ld_draws, uint64_t seed, double* ob, long long ldo,
                            void* stream);
int amx_reset_lanes_motion_noise(amx_ctx* ctx, const uint8_t* mask, const double* times, uint64_t seed,
                                 double time_max, int flags, const amx_reset_noise* noise, const double* draws,
                                 long long ld_draws, const double* ob_src, double* ob_out, int32_t* num_steps,
                                 int32_t* model_idx, int32_t* reset_count, double* t_out, int B, void* stream);
/* ---- reference-motion resets (SimEnv.reset -> DeepMimicCore reset_time, §8f #2) ----------
 * amx_set_motion: host blob (copied; amp_extensions_amd/motion.py build_blob): header[16]
 *   {J, D, F, loop, duration, -, -, -, cycle_delta xyz, ground_pad, ...}, joints [J][8]
 *   {type (0 revolute, 3 fixed, 4 spherical, 5 root), parent, param offset, param size,
 *   attach xyz, -}, bodies [J][8] {shape (0 box, 1 capsule, 2 sphere), attach xyz, Param0-2,
 *   valid}, frame times [F], post-processed frames [F][D], frame velocities [F][D]
 *   (cMotion::Load, deepmimic/deepmimic/DeepMimicCore/anim/Motion.cpp:104-188, 415-442).
 *   Requires S == 1 + 15 J (CtController pose + velocity layout, sim/CtController.cpp:305-319).
 * amx_motion_states: ob[b] = the state recorded after reset_time(times[b]) (motion pose and
 *   velocity at t, plane placement, ground resolve, CtController::BuildStatePose/Vel);
 *   flags: 1 RecordWorldRootPos, 2 RecordWorldRootRot, 4 RecordAllWorld, 8 no ground resolve
 *   (reset_args['resolve'] = False: SceneSimChar::ResetSceneTime skips ResolveCharGroundIntersect,
 *   deepmimic/deepmimic/DeepMimicCore/scenes/SceneSimChar.cpp:714-716).
 * amx_reset_lanes_motion: amx_reset_lanes with those states; t = times[b] or
 *   uniform(0, time_max) from Philox(seed, lane, reset#) (sim_env.py:276); time_max <= 0 means the
 *   clip length (sim_env.py:77; reset_args['time_max'] with custom_time); t_out nullable. */
int amx_set_motion(amx_ctx* ctx, const double* blob, long long n);
double amx_motion_duration(const amx_ctx* ctx);
int amx_motion_states(amx_ctx* ctx, const double* times, int B, int flags, double* ob, long long ldo,
                      void* stream);
int amx_reset_lanes_motion(amx_ctx* ctx, const uint8_t* mask, const double* times, uint64_t seed,
                           double time_max, int flags, const double* ob_src, double* ob_out, int32_t* num_steps,
                           int32_t* model_idx, int32_t* reset_count, double* t_out, int B, void* stream);

/* AMP observation features (SceneImitateAMP::BuildAMPObs, deepmimic/deepmimic/DeepMimicCore/
 * scenes/SceneImitateAMP.cpp:352-475; the discriminator input of the original AMP agent):
 * [pose(cur), pose(prev), vel(cur), vel(prev)] in the current heading frame, amx_amp_obs_size
 * doubles per row (humanoid3d: 226).  Needs amx_set_motion's character tables.
 *   amx_state_amp_obs:  from recorded SimEnv states (s_prev, s_cur) [B][lds] — the agent's
 *                       features of a transition (RecordAMPObsAgent, :154-165);
 *   amx_motion_amp_obs: from the clip at times[b] - dt and times[b] (RecordAMPObsExpert,
 *                       :167-193; dt = 1 / UpdateRate).
 * local_root = enable_amp_obs_local_root (default false, :29). */
int amx_amp_obs_size(const amx_ctx* ctx);
int amx_state_amp_obs(amx_ctx* ctx, const double* s_prev, const double* s_cur, long long lds, int B,
                      int local_root, double* out, long long ldo, void* stream);
int amx_motion_amp_obs(amx_ctx* ctx, const double* times, double dt, int B, int local_root, double* out,
                       long long ldo, void* stream);
/* amx_state_amp_obs written as float32 cost-input rows (the AMP-feature discriminator's
 * input), zero-padded from amx_amp_obs_size up to ldo. */
int amx_state_amp_rows(amx_ctx* ctx, const double* s_prev, const double* s_cur, long long lds, int B,
                       int local_root, float* out, long long ldo, void* stream);

/* ---- DTW evaluation (the 'dtw_cost' of an imitate_amp run; milo/milo/utils.py:115-217) ----
 * Time-warp rows (cSceneImitateAMP::BuildTimeWarpData, scenes/SceneImitateAMP.cpp:537-555):
 * amx_tw_dim = 3 J doubles per row, [(0, root_y, 0), joint_j - root joint (world) for j >= 1].
 *   amx_state_tw_rows:  from recorded SimEnv states s [B][lds]; `flags` are the record flags
 *                       of the states and must be 2 (RecordWorldRootRot only);
 *   amx_motion_tw_rows: of the kinematic character: row t * n + i is the clip pose at
 *                       t0[t] + i / update_rate with lift[t] added to the root height (the
 *                       trajectory's ground-resolve lift; null: none) while a looping clip is
 *                       in the cycle it was reset in (SyncKinCharNewCycle drops it at the next,
 *                       scenes/SceneImitate.cpp:594-607).  out [T * n][ldo]. */
int amx_tw_dim(const amx_ctx* ctx);
int amx_state_tw_rows(amx_ctx* ctx, const double* s, long long lds, int B, int flags, double* out,
                      long long ldo, void* stream);
int amx_motion_tw_rows(amx_ctx* ctx, const double* t0, const double* lift, int T, int n, double update_rate,
                       double* out, long long ldo, void* stream);
/* cDynamicTimeWarper (DeepMimicCore/util/DynamicTimeWarper.cpp: CalcAlignment, CalcIndexBuffer,
 * AddRemainderCost) for T trajectories in one launch, one workgroup each.  `cost_kind` is the cell
 * cost: AMX_DTW_COST_POINTS = cSceneImitateAMP::TimeWarpCost (SceneImitateAMP.cpp:5-25; the
 * mean Euclidean distance of the rows' dim / 3 points, what the scene's warper is built with and
 * the reported 'dtw_cost' uses; dim % 3 == 0), AMX_DTW_COST_SQUARED = the warper's DefaultCost
 * (DynamicTimeWarper.cpp:3-8; the squared distance of the rows).  data0 / data1
 * [T][n_max][ld] fp64 rows of width dim (simulated / kinematic); trajectory t uses its first
 * len[t] rows of both (2 <= len <= n_max <= 513: a thread per row).  len_host is a HOST array the call validates,
 * len the caller's device copy of it the kernel reads (clamped into [2, n_max] there; that
 * the two copies agree is the caller's responsibility: nothing on the launch path can compare them).
 * work: amx_dtw_work(T, n_max) doubles (every trajectory's n_max x n_max cost buffer).
 * Outputs: cost [T] = C(n-1, n-1); dtw_cost [T] (nullable) = cost + remainder, remainder =
 * buffer_size - len (SceneImitateAMP.cpp:261-269); index [T][n_max] int32 and backtrack
 * [T][n_max] (after the remainder; backtrack_raw, nullable: before it), entries [0, len) only.
 * Bad arguments (null pointer, ld < dim, a len outside [2, n_max], buffer_size < len, n_max
 * above 513, an LDS need of (3 n_max + 96 dim) doubles above 64 KiB) return AMX_E_ARG before
 * any launch. */
#define AMX_E_ARG AMX_E_INVAL
enum { AMX_DTW_COST_SQUARED = 0, AMX_DTW_COST_POINTS = 1 };
long long amx_dtw_work(int T, int n_max);
int amx_dtw_align(amx_ctx* ctx, const double* data0, const double* data1, long long ld, int dim, int cost_kind,
                  int n_max,
                  const int32_t* len_host, const int32_t* len, int T, int buffer_size, double* work,
                  double* cost, double* dtw_cost, int32_t* index, double* backtrack_raw, double* backtrack,
                  void* stream);

/* ---- NPG policy update (the rollout's learner; mjrl/mjrl/algos/npg_cg.py:113-199) ----
 * Policy: mjrl MLP(S -> 32 -> 32 -> A, tanh) + log_std (mjrl/mjrl/policies/gaussian_mlp.py),
 * parameters packed in the reference's flat order (W1, b1, W2, b2, W3, b3, log_std; fp32,
 * amx_npg_param_count(S, A) floats).  obs [N][ldo] / act [N][lda] are fp64 or fp32
 * (AMX_IN_*); the policy reads float32(obs) as the reference does (gaussian_mlp.py:112-117).
 * amx_npg_pass writes one fp64 partial per block of rows_per_block rows (multiple of 32):
 *   mode 0 (VPG):  grad of mean(exp(LL_new - LL_old) * adv) at new == old
 *                  (BatchREINFORCE.flat_vpg, batch_reinforce.py:58-62)            -> [blocks][P]
 *   mode 1 (FVP):  J^T diag(2/(2 sigma^2 + 1e-8)) J vec / N, the mean-network block of
 *                  NPG.HVP (npg_cg.py:87-106; log_std block and damping: caller)  -> [blocks][P]
 *   mode 2 (EVAL): sum of exp(LL_vec - LL_theta) * adv and of the per-sample mean_kl
 *                  terms (surr_after / kl_old_new, npg_cg.py:181-183)             -> [blocks][2]
 * amx_npg_reduce sums the partials over blocks in block order (deterministic). */
long long amx_npg_param_count(int S, int A);
int amx_npg_pass(amx_ctx* ctx, int mode, int N, const void* obs, int obs_dtype, long long ldo,
                 const void* act, int act_dtype, long long lda, const double* adv, const float* theta,
                 const float* vec, int rows_per_block, double* partials, void* stream);
int amx_npg_reduce(amx_ctx* ctx, const double* partials, int blocks, int P, double* out, void* stream);
/* The same with a gate: gate = the CG state of amx_npg_cg_init / _step ({rdotr, live}); with
 * live == 0 the pass and the reduction return at once (every block reads the flag), so the FVP
 * products of a solve that stopped early cost two empty launches, not a pass over the batch
 * (cg_solve.py:19-20 breaks the loop there). */
int amx_npg_pass_gated(amx_ctx* ctx, int mode, int N, const void* obs, int obs_dtype, long long ldo,
                       const void* act, int act_dtype, long long lda, const double* adv, const float* theta,
                       const float* vec, int rows_per_block, double* partials, const double* gate, void* stream);
int amx_npg_reduce_gated(amx_ctx* ctx, const double* partials, int blocks, int P, double* out, const double* gate,
                         void* stream);
/* amx_npg_pass_gated with the policy's forward at theta cached per sample: hcache [N][64] fp32
 * (H1 = tanh(W1 x + b1) | H2 = tanh(W2 H1 + b2)), 16-byte aligned.  Mode 0 (VPG) writes it; mode 1
 * (FVP, fp32 observations) reads it instead of recomputing layers 1-2 at theta -- valid only for
 * the theta and observations of the VPG pass that wrote it (npg_cg.py:123-135: the CG's ten
 * Fisher-vector products share them).  The FVP partials are bit-identical to the uncached pass. */
int amx_npg_pass_ex(amx_ctx* ctx, int mode, int N, const void* obs, int obs_dtype, long long ldo, const void* act,
                    int act_dtype, long long lda, const double* adv, const float* theta, const float* vec,
                    int rows_per_block, double* partials, const double* gate, float* hcache, void* stream);
/* amx_npg_pass_ex for one rank of a data-parallel update: the N rows are this rank's share of
 * n_total rows held over all ranks, and the means divide by n_total (VPG: adv / n_total; FVP:
 * J^T D J / n_total), so the ranks' column sums add up to the gradient / Fisher-vector product of
 * the union.  Blocks, row bounds and the hcache are the rank's own (N, rows_per_block); the EVAL
 * partials are plain sums and do not depend on n_total.  n_total == N is amx_npg_pass_ex bit for
 * bit; a power-of-two ratio scales every VPG / FVP partial exactly.  n_total < N or < 1:
 * AMX_E_ARG, nothing launched. */
int amx_npg_pass_dp(amx_ctx* ctx, int mode, int N, const void* obs, int obs_dtype, long long ldo, const void* act,
                    int act_dtype, long long lda, const double* adv, const float* theta, const float* vec,
                    int rows_per_block, double* partials, const double* gate, float* hcache, long long n_total,
                    void* stream);

/* The conjugate-gradient solve of NPG (mjrl/mjrl/utils/cg_solve.py:3-23) on the device, one
 * workgroup per call, fixed-order fp64 reductions, no host round trip between iterations.
 * amx_npg_cg_init: x = 0, r = p = b, p32 = float32(p), state = {r.r, 1 (live)}.
 * amx_npg_cg_step, after h = amx_npg_reduce(amx_npg_pass(FVP, vec = p32)):
 *   z = h + [log_std block: curv * p32] + damping * p   (NPG.HVP's return, npg_cg.py:105)
 *   v = rdotr / p.z; x += v p; r -= v z; rr = r.r; p = r + (rr / rdotr) p; rdotr = rr;
 *   live = rdotr >= residual_tol (cg_solve's break: a finished solve leaves x/r/p unchanged);
 *   p32 = float32(p) for the next product.  curv [A]: d^2 mean_kl / d log_std^2.  P <= 16384. */
/* d^2 mean_kl / d log_std^2 per action at new == old (NPG.HVP's log_std block,
 * gaussian_mlp.py:144-155): curv[d] = (8 s^2 - 4 s 1e-8) / (2 s + 1e-8)^2, s = exp(log_std[d])^2,
 * log_std = theta[P - A ..]. */
int amx_npg_curvature(amx_ctx* ctx, const float* theta, int P, int A, double* curv, void* stream);
/* The NPG step after the CG (npg_cg.py:141-163) in one workgroup: gdot = vpg . npg; use_alpha
 * (const_learn_rate): n_step_size = alpha^2 gdot, else alpha = sqrt(|n_step_size / (gdot + 1e-20)|);
 * new_theta = float32(theta + alpha npg) with the log_std block clamped at min_log_std
 * (gaussian_mlp.py:71-94); scal = {alpha, n_step_size, gdot}.  P <= 16384. */
int amx_npg_apply_step(amx_ctx* ctx, int P, int A, const double* vpg, const double* npg, const float* theta,
                       int use_alpha, double alpha, double n_step_size, float min_log_std, float* new_theta,
                       double* scal, void* stream);
/* amx_npg_reduce (the FVP pass's partials, the same summation order) and amx_npg_cg_step
 * (cg_solve.py:3-23: one iteration after the Fisher-vector product) in two launches over the
 * chip: the column sums with z and the blocks' p.z parts; then x, r, p and the state, every block
 * forming v = rdotr / p.z and r'.r' itself in one fixed order (so p.z and r.r sum in another order
 * than amx_npg_cg_step's).  The residual and the state alternate between two caller buffers
 * (iteration i reads r_in / state_in and writes r_out / state_out; the next swaps them: every
 * block reads all of r); x, p, p32 are updated in place.  A stopped solve (state_in[1] == 0)
 * copies r and the state over and changes nothing else.  work: caller-owned fp64
 * [amx_npg_cg_tail_work(P)], no state kept between calls.  Replaces round 4's
 * amx_npg_reduce_cg_step (one launch, the step by the last-arriving block). */
long long amx_npg_cg_tail_work(int P);
int amx_npg_cg_tail(amx_ctx* ctx, const double* partials, int blocks, int P, int A, const double* curv,
                    double damping, double tol, double* x, const double* r_in, double* r_out, double* p, float* p32,
                    const double* state_in, double* state_out, double* work, void* stream);
/* amx_npg_cg_tail's two launches, separately: amx_npg_cg_reduce (column sums, z and the p.z
 * parts into work; skipped when state[1] == 0) and amx_npg_cg_xrp (the vector step from work:
 * x, r_in -> r_out, p, p32 in place, state_in -> state_out). */
int amx_npg_cg_reduce(amx_ctx* ctx, const double* partials, int blocks, int P, int A, const double* curv,
                      double damping, const double* p, const float* p32, const double* state, double* work,
                      void* stream);
int amx_npg_cg_xrp(amx_ctx* ctx, int P, double tol, double* x, const double* r_in, double* r_out, double* p,
                   float* p32, const double* state_in, double* state_out, const double* work, void* stream);
/* The Fisher-vector pass (mode 1, amx_npg_pass_ex with hcache) with the PREVIOUS CG iteration's
 * vector step folded into its setup: every block forms amx_npg_cg_xrp's v, r' = r_in - v z,
 * r'.r' (xrp's summation orders: the same bits) and p' = r' + (r'.r' / r.r) p_in from work (the
 * previous amx_npg_cg_reduce) and multiplies by float32(p') instead of a vec argument; the blocks
 * write x += v p_in, r_out, p_out, p32_out (their slices) and state_out {r'.r', live}.  A solve
 * stopped before (state_in[1] == 0) or by this step (r'.r' < tol) writes no partials (the gate)
 * and carries r, p and the state over.  r, p and the state alternate buffers (every block reads
 * all of them).  One CG iteration = amx_npg_pass_cg (or, first, amx_npg_pass_gated on p32) +
 * amx_npg_cg_reduce; the solve ends with one amx_npg_cg_xrp: the step's own launch is gone from
 * every iteration but the last.  Actions are not read. */
int amx_npg_pass_cg(amx_ctx* ctx, int N, const void* obs, int obs_dtype, long long ldo, const float* theta,
                    int rows_per_block, double* partials, float* hcache, double tol, double* x, const double* r_in,
                    double* r_out, const double* p_in, double* p_out, float* p32_out, const double* state_in,
                    double* state_out, const double* work, void* stream);
/* amx_npg_pass_cg with amx_npg_pass_dp's divisor: one rank's Fisher-vector pass of a data-parallel
 * solve.  The rank's message of the iteration is amx_npg_reduce_gated(partials, blocks, P, msg,
 * state_out): its column sums as one [P] vector, left alone once the solve has stopped; the caller
 * sums msg over the ranks and hands it to amx_npg_cg_reduce as a one-block partials buffer
 * (blocks = 1: h = msg, the sum of one run of one block).  The fold reads only work, r, p and the
 * state, which are formed from the summed message, so every rank takes the same vector step bit
 * for bit provided the collective leaves the same bits on every rank.  With one rank and no
 * collective the message path gives amx_npg_cg_reduce's bits over the partials themselves (the
 * amx_npg_reduce order).  n_total < N or < 1: AMX_E_ARG, nothing launched. */
int amx_npg_pass_cg_dp(amx_ctx* ctx, int N, const void* obs, int obs_dtype, long long ldo, const float* theta,
                       int rows_per_block, double* partials, float* hcache, double tol, double* x,
                       const double* r_in, double* r_out, const double* p_in, double* p_out, float* p32_out,
                       const double* state_in, double* state_out, const double* work, long long n_total,
                       void* stream);
/* The Fisher-vector pass over an index vector: NPG.HVP with hvp_sample_frac < 1
 * (mjrl/mjrl/algos/npg_cg.py:90-94).  row_idx: device int32 [M], 0 <= row_idx[k] < N (the caller
 * guarantees the range; duplicates are legal, the reference samples with replacement).  The pass
 * runs over the M rows obs[row_idx[k]], divides by M and, with hcache ([N][64], written by the
 * VPG pass over all N rows), reads hcache[row_idx[k]]: the partials ([ceil(M / rows_per_block)][P])
 * are those of amx_npg_pass_ex (mode 1) on the materialised rows, bit for bit.  fp32 observations
 * only (obs_dtype AMX_IN_F32).  prod_count (optional, device double): += 1 when the product is
 * taken (not gated, not stopped) -- the solve's count of index vectors consumed.
 * amx_npg_pass_cg_idx is amx_npg_pass_cg over the index vector. */
int amx_npg_pass_idx(amx_ctx* ctx, int N, int M, const int32_t* row_idx, const void* obs, int obs_dtype,
                     long long ldo, const float* theta, const float* vec, int rows_per_block, double* partials,
                     const double* gate, float* hcache, double* prod_count, void* stream);
int amx_npg_pass_cg_idx(amx_ctx* ctx, int N, int M, const int32_t* row_idx, const void* obs, int obs_dtype,
                        long long ldo, const float* theta, int rows_per_block, double* partials, float* hcache,
                        double tol, double* x, const double* r_in, double* r_out, const double* p_in,
                        double* p_out, float* p32_out, const double* state_in, double* state_out,
                        const double* work, double* prod_count, void* stream);
/* The log-likelihood pass of NPG.CPI_surrogate's BC term and dist-info entries
 * (gaussian_mlp.py:106-122 in fp32): amx_ppo_old_ll's rows and arithmetic (the same LL bits, so
 * equal parameters give LL_new - LL_old == 0 and a likelihood ratio of exactly 1).
 * partials[b] (device fp64 [amx_npg_ll_blocks(ctx, N)]) = the sum of workgroup b's rows' LL;
 * ll (optional, fp32 [N]) and mean (optional, fp32 [N][A]) take every row's LL and policy mean. */
int amx_npg_ll_blocks(amx_ctx* ctx, int N);
int amx_npg_ll(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act, long long lda,
               const float* theta, double* partials, float* ll, float* mean, void* stream);
int amx_npg_cg_init(amx_ctx* ctx, int P, const double* b, double* x, double* r, double* p, float* p32,
                    double* state, void* stream);
/* amx_npg_cg_init + amx_npg_curvature (theta's log_std block -> curv [A]) in one launch. */
int amx_npg_cg_init_ls(amx_ctx* ctx, int P, int A, const float* theta, double* curv, const double* b, double* x,
                       double* r, double* p, float* p32, double* state, void* stream);
int amx_npg_cg_step(amx_ctx* ctx, int P, int A, const double* h, const double* curv, double damping,
                    double residual_tol, double* x, double* r, double* p, float* p32, double* state,
                    void* stream);

/* ---- step + termination ------------------------------------------------------- */

/* One batched SimEnv.step after the forward (gym-simenv/gym_simenv/envs/sim_env.py:140-173):
 * num_steps[b] += 1; ob_next[b] = ob[b] + (double)preds[model_idx[b]][b] (fp64 state,
 * fp32 model, :158); done[b] = horizon | check_collision | check_velocity (:164-268),
 * bit-exact fp64 comparisons.  Fused extras (nullable):
 *   disc[b]   = max over model pairs of ||preds_i - preds_j||_2 (compute_discrepancy,
 *               milo/milo/dynamics.py:134-143) — reuses the step's own forward;
 *   cost_in   = float32 [ob, ob_next] rows, ld = ldc (the 'ss' cost input,
 *               mjrl/mjrl/algos/batch_reinforce.py:107-113);
 *   nonfinite[b] = 1 if ob_next holds a NaN/Inf (diagnostic only; done unchanged). */
int amx_step(amx_ctx* ctx, const float* preds, int ldp, long long strideP, const int32_t* model_idx,
             const double* ob, double* ob_next, int32_t* num_steps, uint8_t* done, float* disc,
             float* cost_in, int ldc, uint8_t* nonfinite, int B, void* stream);
/* amx_step that also writes cost_rexp[b] = the exponent of the [s, s'] cost row's max |x|
 * (max < 2^e, clamped to [-100, 100]): the row_exp operand of amx_rff_features_h3. */
int amx_step_rexp(amx_ctx* ctx, const float* preds, int ldp, long long strideP, const int32_t* model_idx,
                  const double* ob, double* ob_next, int32_t* num_steps, uint8_t* done, float* disc,
                  float* cost_in, int ldc, int* cost_rexp, uint8_t* nonfinite, int B, void* stream);

/* amx_step (cost_rexp nullable: amx_step_rexp) fused with amx_reset_lanes(mask = done,
 * ob_src = ob_next) in one pass: done lanes get reset_count/model_idx/num_steps/row_out
 * and ob_out[b] = table[row] exactly as amx_reset_lanes; the others ob_out[b] = ob_next[b]
 * (from registers, no re-read).  ob_out must differ from ob_next; it may be ob (in place:
 * every lane reads its row before writing it); model_idx is read (the member of this step)
 * and, for reset lanes, rewritten.  ob_rec (nullable, a fourth buffer) receives a copy of ob
 * (a rollout's slot 0 when the carried lane states are read where the last rollout left
 * them, instead of a separate carry copy).  steps0_out (nullable):
 * receives num_steps before this step (the trajectory position of a rollout's first slot).
 * counter (nullable): *counter += counter_delta once per launch (amx_counter_add folded into a
 * captured rollout's last step; no kernel of this launch reads the counter). */
int amx_step_reset(amx_ctx* ctx, const float* preds, int ldp, long long strideP, int32_t* model_idx,
                   const double* ob, double* ob_next, int32_t* num_steps, uint8_t* done, float* disc,
                   float* cost_in, int ldc, int* cost_rexp, uint8_t* nonfinite, const double* table,
                   int R, const int32_t* rows, uint64_t seed, double* ob_out, int32_t* reset_count,
                   int32_t* row_out, int32_t* steps0_out, uint64_t* counter, long long counter_delta,
                   double* ob_rec, int B, void* stream);

/* amx_step_reset of step t (no counter advance) fused with the policy of step t + 1 on the
 * observations it produces (obs[t+1] = ob_out): one launch runs the step of 16 lanes, keeps the
 * float32 of their obs[t+1] rows on chip and runs amx_policy_act on them (Philox noise with
 * policy_seed and counter / counter_dev as amx_policy_act[_dev]; no injected noise), writing
 * act [B][A], mean and the fused x0 / row-exponent assembly exactly as amx_policy_act.  The
 * results are bit-identical to amx_step_reset followed by amx_policy_act on ob_out (the same
 * workgroup decomposition of the policy).  Replaces, per rollout step t + 1 > 0, the reference's
 * get_action call after env.step (mjrl/mjrl/samplers/core.py via milo/milo/sampler.py:48-65).
 * S <= 256 and a policy image of at most 16384 floats. */
int amx_step_reset_act(amx_ctx* ctx, const float* preds, int ldp, long long strideP, int32_t* model_idx,
                       const double* ob, double* ob_next, int32_t* num_steps, uint8_t* done, float* disc,
                       float* cost_in, int ldc, int* cost_rexp, uint8_t* nonfinite, const double* table,
                       int R, const int32_t* rows, uint64_t seed, double* ob_out, int32_t* reset_count,
                       int32_t* row_out, int32_t* steps0_out, double* ob_rec, const float* blob, int H1,
                       int H2, const double* noise_scale, uint64_t policy_seed, uint64_t counter,
                       const uint64_t* counter_dev, int eval_mode, double* act, float* mean,
                       float* x0_buf, long long stride_m, int ldk, int* row_exp, long long stride_rexp,
                       long long slot_stride, int n_slots, int B, void* stream);
/* amx_step_reset_act's occupancy, for A/B measurement: 0 (default) one 1024-thread workgroup
 * per CU at the kernel's natural register count, 1 two per CU (registers capped at 64). */
int amx_set_step_act_occupancy(amx_ctx* ctx, int two_per_cu);

/* Disagreement only (DynamicsEnsemble.get_action_discrepancy / compute_threshold,
 * milo/milo/dynamics.py:145-165). */
int amx_disagreement(amx_ctx* ctx, const float* preds, int ldp, long long strideP, float* disc,
                     int B, void* stream);

/* SimEnv.reset for masked lanes (gym-simenv/gym_simenv/envs/sim_env.py:270-285), with
 * the DeepMimicCore pose replaced by a row of a device reset-state table (documented
 * deviation).  For every lane b with mask[b] != 0 (mask NULL = all lanes):
 *   reset_count[b] += 1; model_idx[b] = reset_count[b] % n_models; num_steps[b] = 0;
 *   row = rows ? rows[b] : philox(seed, b, reset_count[b]) mod R; ob_out[b] = table[row].
 * Lanes with mask 0 copy ob_src[b] into ob_out[b] (carry; ob_src may equal ob_out).
 * row_out (nullable) receives the chosen row (-1 for carried lanes). */
int amx_reset_lanes(amx_ctx* ctx, const uint8_t* mask, const double* table, int R,
                    const int32_t* rows, uint64_t seed, const double* ob_src, double* ob_out,
                    int32_t* num_steps, int32_t* model_idx, int32_t* reset_count, int32_t* row_out,
                    int B, void* stream);

/* ---- device policy ------------------------------------------------------------ */

/* mjrl Gaussian MLP policy action (mjrl/mjrl/policies/gaussian_mlp.py:95-104 over
 * FCNetwork tanh, mjrl/mjrl/utils/fc_network.py:42-55), two hidden layers:
 *   mean = W3 tanh(W2 tanh(W1 float(ob) + b1) + b2) + b3   (float32)
 *   act  = (double)mean + noise_scale * n,  n ~ N(0,1) fp64 (philox(seed, b, counter)
 *          Box-Muller) or injected noise[b][A] (nullable).  eval_mode: act = mean.
 * The weights come as the packed image of amx_policy_pack (re-pack after each policy
 * update, e.g. after the learner's step; not per action).
 * noise_scale = exp(log_std) in fp64 (device, [A]).
 * x0_buf (nullable) fuses the ensemble's state assembly (amx_assemble_input with
 * AMX_IN_F64) for the same lanes: x0 = [(float(ob)-mu_s)/sd_s, (float(act)-mu_a)/sd_a, 0]
 * written to every model's activation row (stride_m, ldk as in amx_assemble_input; stride_m
 * 0: once, model 0's rows, the f16x3 GEMMs' shared x0 slice); row_exp (nullable, needs x0_buf)
 * additionally writes the f16x3 row-exponent slots exactly as amx_assemble_input_rexp (including
 * its member-blocked layout, slot_stride < B). */
int amx_policy_act(amx_ctx* ctx, const double* ob, int B, const float* blob, int H1, int H2,
                   const double* noise_scale, const double* noise, uint64_t seed, uint64_t counter,
                   int eval_mode, double* act, float* mean, float* x0_buf, long long stride_m, int ldk,
                   int* row_exp, long long stride_rexp, long long slot_stride, int n_slots,
                   void* stream);

/* amx_policy_act with the Philox counter = counter[0] (device memory) + counter_offset, so a
 * captured HIP graph of a rollout (step t passes offset t) draws fresh noise on every replay;
 * amx_counter_add(counter, delta) advances it on the stream (one thread, once per rollout). */
int amx_policy_act_dev(amx_ctx* ctx, const double* ob, int B, const float* blob, int H1, int H2,
                       const double* noise_scale, const double* noise, uint64_t seed,
                       const uint64_t* counter, uint64_t counter_offset, int eval_mode, double* act,
                       float* mean, float* x0_buf, long long stride_m, int ldk, int* row_exp,
                       long long stride_rexp, long long slot_stride, int n_slots, void* stream);
int amx_counter_add(amx_ctx* ctx, uint64_t* counter, long long delta, void* stream);

/* GEMM timing that works inside captured HIP graphs (ROCm has no timing-event nodes) and adds
 * no launches: with buf set (4 uint64 of device memory, zeroed by the caller), every f16x3
 * ensemble forward on this context records the device's 100 MHz realtime counter when its
 * first hidden layer starts (amx_gemm_bias_act_h3 with rexp_slots = 1, or the windowed form
 * with first_layer = 1: block 0, buf[0]) and, when the last workgroup of its output layer
 * (amx_gemm_out_unnorm_h3 or its windowed form) finishes, adds the
 * elapsed ticks to buf[2] and 1 to buf[3] (buf[1]: arrival counter, left zero).  The pointer
 * is read when a launch is issued (graph capture bakes it in).  null: off. */
int amx_set_gemm_timer(amx_ctx* ctx, uint64_t* buf);

/* Split workspace of the f16x3 output layer (amx_gemm_out_unnorm_h3): at lane counts whose
 * 128 x 224 output tiles are fewer than the CUs but at least half as many (4096-7168 lanes x 4
 * members), the layer runs stream-K: one workgroup per CU, the tiles' K-tiles dealt out evenly,
 * each tile's 1-3 K segments stored raw and summed in K order by the last arriver
 * (deterministic); the hidden layers' 128 x 256 tiles split the same way below 2048 lanes.
 * amx_split_workspace_floats: floats of scratch (up to 6 partial tiles per tile, the largest
 * of the shapes above) and *n_counters uint32 counters a forward of `rows` padded lanes needs, 0 when that shape
 * does not use it.  amx_set_split_workspace registers caller-owned device memory with the
 * context (counters zeroed by the caller once; each launch leaves them zero); without it the
 * layer runs on row-block tiles.  One launch at a time per context.  The sizes follow the
 * context's connectivity (a plain layer's K is `hidden`). */
long long amx_split_workspace_floats(const amx_ctx* ctx, int groups, int rows, int* n_counters);

int amx_set_split_workspace(amx_ctx* ctx, float* scratch, long long floats, uint32_t* counters,
                            int n_counters);

/* Floats to allocate for the packed policy weight image for hidden widths H1, H2 (host query;
 * -1 on a bad argument): the image rounded up to whole 1-KiB pieces, which
 * amx_step_reset_act copies into LDS by LDS-DMA (amx_policy_pack writes the image, the tail is
 * never read as weights). */
long long amx_policy_blob_floats(const amx_ctx* ctx, int H1, int H2);

/* Pack the policy's three nn.Linear layers (W [out][in] row-major f32, b [out]; the
 * FCNetwork fc_layers, mjrl/mjrl/utils/fc_network.py:24-31) into blob (device, 16-byte
 * aligned, amx_policy_blob_floats floats): zero-padded rows in the layout amx_policy_act
 * copies into LDS with one vector pass. */
int amx_policy_pack(amx_ctx* ctx, const float* W1, const float* b1, int H1, const float* W2,
                    const float* b2, int H2, const float* W3, const float* b3, float* blob,
                    void* stream);

/* ---- MILO RFF MMD cost -------------------------------------------------------- */

/* Rows per fp64 column partial of the RFF features (round 5: 32, was 128): col_partials has
 * rows / AMX_RFF_PART_ROWS rows, so the feature pass may use 160- and 80-row tiles that fill the
 * CUs in whole rounds (40 960 rows: 512 tiles of 160 x 256; 5 120 rows: 256 tiles of 160 x 64). */
#define AMX_RFF_PART_ROWS 32

/* RBFLinearCost.get_rep (milo/milo/linear_cost.py:64-71) on MFMA:
 * phi[r][f] = cos(sum_k x[r][k] W[f][k] + b[f]) * scale, scale = (float)sqrt(2/F),
 * plus fp64 column sums of each 32-row group's valid rows (r < n_valid and (row_mask==NULL or
 * row_mask[r])) into col_partials[r/AMX_RFF_PART_ROWS][f] — the per-rank share of the global
 * feature mean of fit_cost (:84-94); amx_feature_message / amx_sum_partials add the
 * rows / AMX_RFF_PART_ROWS partial rows in order.  rows % 128 == 0, F % 128 == 0. */
int amx_rff_features(amx_ctx* ctx, int rows, int n_valid, int F, int K, const float* x, int ldx,
                     const float* W, int ldw, const float* b, float scale, float* phi, int ldphi,
                     double* col_partials, const uint8_t* row_mask, void* stream);

/* Deterministic ordered sum of n_parts rows of fp64 partials -> out[F] (fp64). */
int amx_sum_partials(amx_ctx* ctx, const double* partials, int n_parts, int F, double* out,
                     void* stream);

/* fit_cost closed form (milo/milo/linear_cost.py:84-94) after the cross-rank sum:
 * phi_pi = (float)(phi_sum / count); w = phi_pi - phi_e; mmd[0] = dot(w, w) (fp32).
 * count = 0: the count is read from phi_sum[F] (the all-reduced [sum phi | count] message). */
int amx_mmd_fit(amx_ctx* ctx, const double* phi_sum, double count, const float* phi_e, int F,
                float* w, float* mmd, void* stream);

/* Per-sample MILO reward with pessimism (RBFLinearCost.get_costs + get_bonus_costs,
 * milo/milo/linear_cost.py:96-103, 111-152; reward = -cost, batch_reinforce.py:144):
 *   v = clamp(phi[n].w, c_min, c_max); dh = min(disc[n]/thr, 1); bonus = dh*c_min;
 *   ipm = (1-lambda)*v; wb = lambda*bonus; reward = -(ipm - wb).
 * ipm/wbonus outputs are nullable (info['ipm'], info['bonus']). */
int amx_mmd_reward(amx_ctx* ctx, const float* phi, int ldphi, const float* w, int F, const float* disc,
                   float thr, double lambda_b, float c_min, float c_max, float* reward, float* ipm,
                   float* wbonus, int n, void* stream);

/* Same with cost_range=None (linear_cost.py:103, 138-139): v = phi[n].w unclamped,
 * bonus = disc[n] (raw disagreement); ipm/wb/reward as above. */
int amx_mmd_reward_raw(amx_ctx* ctx, const float* phi, int ldphi, const float* w, int F, const float* disc,
                       double lambda_b, float* reward, float* ipm, float* wbonus, int n, void* stream);

/* get_expert_cost (milo/milo/linear_cost.py:105-109): partial fp64 sums over row
 * blocks of clamp(phi_E[r].w, c_min, c_max); out[0] = sum (fp64; out holds 1 + 1024
 * doubles).  mean_out (nullable) receives the finished cost in fp32:
 * (float)(1 - lambda_b) * (float)(sum / n).  Uses the resident expert features.
 * phi_e_rows and w are 16-byte aligned, ldphi a multiple of 4 (float4 loads). */
int amx_expert_cost(amx_ctx* ctx, const float* phi_e_rows, int ldphi, const float* w, int F, int n,
                    float c_min, float c_max, double* out, float* mean_out, double lambda_b,
                    void* stream);

/* The relabel's feature message (batch_reinforce.py:110-113 -> fit_cost's mean,
 * linear_cost.py:88): out[0..F) = the ordered fp64 column sums of n_parts rows of RFF
 * partials (as amx_sum_partials), out[F] = count -- the one buffer the cross-rank all-reduce
 * sums and amx_mmd_relabel reads. */
int amx_feature_message(amx_ctx* ctx, const double* partials, int n_parts, int F, double count,
                        double* out, void* stream);

/* The relabel tail in ONE launch (batch_reinforce.py:110-152 with linear_cost.py:84-109):
 * w = (float)(msg[f] / count) - phi_e[f] and mmd[0] = w.w exactly as amx_mmd_fit (count 0:
 * read msg[F]); the per-sample pessimistic reward of rows [0, n) of phi exactly as
 * amx_mmd_reward (clamp = 1: cost_range (c_min, c_max)) or amx_mmd_reward_raw (clamp = 0);
 * and, when expert_rows is given (clamp only), the expert cost exactly as amx_expert_cost
 * (expert_out: 1 + 1024 doubles, expert_mean: (1 - lambda_b) * mean in fp32).  `counter` is
 * one uint32 of device memory, zero before the first launch; the kernel leaves it zero.
 * One launch at a time per counter. */
int amx_mmd_relabel(amx_ctx* ctx, const double* msg, double count, const float* phi_e, int F,
                    float* w, float* mmd, const float* phi, int ldphi, const float* disc, float thr,
                    double lambda_b, int clamp, float c_min, float c_max, float* reward, float* ipm,
                    float* wbonus, int n, const float* expert_rows, int ld_e, int n_e,
                    double* expert_out, float* expert_mean, uint32_t* counter, void* stream);

/* ---- AMP / GAIL least-squares discriminator reward ---------------------------- */

/* Last Discriminator layer (512->1, milo/milo/gail_cost.py:18-42) fused with
 * get_ls_costs (:231-236) and get_bonus_costs (:254-279):
 *   D = h[n].w3 + b3; r = max(0, 1 - 0.25*(1-D)^2); ipm = (1-lambda)*(-r);
 *   bonus = lambda*disc[n] (raw disagreement); reward = -(ipm - bonus).
 * disc NULL -> plain get_costs path: reward = r. logits (nullable) receives D. */
int amx_amp_reward(amx_ctx* ctx, const float* h, int ldh, int Hd, const float* w3, float b3,
                   const float* disc, double lambda_b, float* reward, float* logits, int n,
                   void* stream);

/* amx_amp_reward for either discriminator loss type (GAILCost.get_costs,
 * gail_cost.py:246-251): AMX_DISC_LEAST_SQUARES as above, AMX_DISC_LOG_LIKELIHOOD
 * with input cost logsigmoid(D) (get_ll_costs, :238-244), r = -logsigmoid(D). */
int amx_disc_reward(amx_ctx* ctx, int loss_type, const float* h, int ldh, int Hd, const float* w3, float b3,
                    const float* disc, double lambda_b, float* reward, float* logits, int n, void* stream);

/* Cost-input rows of the non-'ss' input types ('sa', 'sas', 's', or AMP features):
 * out[b] = float32 [x0[b,:w0], x1[b,:w1], x2[b,:w2], 0...] up to ldc, fp64 sources
 * (linear_cost.py:115-127, gail_cost.py:258-268, batch_reinforce.py:107-110).
 * A segment with width 0 is absent (its pointer may be NULL). */
int amx_cost_rows(amx_ctx* ctx, const double* x0, long long ld0, int w0, const double* x1, long long ld1, int w1,
                  const double* x2, long long ld2, int w2, int B, float* out, int ldc, void* stream);

/* ---- returns / value baseline / GAE (the sampler's consumer) ------------------ */

/* Trajectory layout shared by the calls below ("segment grid"): L lanes of up to T
 * rows.  Lane l owns rows r(t, l) = base[l] + t * stride for t < len[l] (base NULL ->
 * base[l] = l; len NULL -> T).  end[r] closes a trajectory at row r: 0 = continues,
 * 1 = terminated (bootstrap 0), 2 = ends without termination (bootstrap with the
 * row's own baseline, mjrl's non-terminated rule); a lane's last row with end 0 is
 * treated as 2.  t0[l] (NULL -> 0) is the position of the lane's first row inside its
 * trajectory.  Engine buffers: base NULL, stride = lanes, end = done flags;
 * concatenated mjrl paths: base = path offsets, stride = 1, end = 1/2 at path ends. */

/* MLPBaseline._features (mjrl/mjrl/baselines/mlp_baseline.py:36-59): row r of feat
 * [.., ldf] f32 = [clip(obs[r], -10, 10) / 10, (tpos/1000)^1..4, 0 ...] computed in
 * fp64 and rounded to f32 (featmat.astype('float32'), :100); tpos = row position in
 * its trajectory.  Columns [S + 4, kf) are zeroed, kf = round_up(S + 4, 32). */
int amx_value_features(amx_ctx* ctx, int T, int L, const int32_t* len, const int32_t* t0,
                       const int64_t* base, long long stride, const uint8_t* end,
                       const double* obs, int ldo, float* feat, int ldf, void* stream);

/* Last Linear(H -> 1) of the MLPBaseline model (mlp_baseline.py:20-27, predict :99-108):
 * v[r] = b[0] + sum_k h[r][k] * w[k] (f32) for r < rows; H a multiple of 4. */
int amx_value_head(amx_ctx* ctx, int rows, const float* h, int ldh, int H, const float* w,
                   const float* b, float* v, void* stream);

/* compute_returns + compute_advantages (mjrl/mjrl/utils/process_samples.py:3-45):
 * per trajectory, in fp64 (numpy 1.21 promotion of the pinned reference env):
 *   ret[t] = rew[t] + gamma * ret[t+1]                            (discount_sum)
 *   GAE (gamma_lambda >= 0): delta[t] = (rew[t] + gamma * b1[t+1]) - b[t],
 *        adv[t] = delta[t] + gamma_lambda * adv[t+1]; b1 = b + [0 | b[-1]] at the end;
 *        delta is float64 for terminated trajectories and float32 arithmetic otherwise
 *        (np.append keeps b1 float32 when the appended value is b[-1])
 *   standard (gamma_lambda < 0): adv[t] = ret[t] - b[t].
 * rew (f32) is read at rbase[l] + t * rstride (rbase NULL -> l); v, ret, adv use r(t, l).
 * gamma_lambda = gamma * gae_lambda formed by the caller in double. */
int amx_gae(amx_ctx* ctx, int T, int L, const int32_t* len, const int64_t* base, long long stride,
            const uint8_t* end, const float* rew, const int64_t* rbase, long long rstride,
            const float* v, double gamma, double gamma_lambda, double* ret, double* adv,
            void* stream);

/* Advantage whitening of BatchREINFORCE.process_paths (mjrl/mjrl/algos/batch_reinforce.py:
 * 280-285): over the grid's rows, out = (adv - mean) / (std + eps) (population std);
 * stats[0..1] = mean, std (fp64, fixed reduction order).  out may alias adv.  Two launches over
 * the chip (per-block count / mean / M2 / residual, then the combine in block order and the apply); the
 * per-block partials live in the context (graph-capturable), so a context runs one whitening
 * at a time: do not issue two on different streams, or a captured one beside an eager one. */
int amx_adv_whiten(amx_ctx* ctx, int T, int L, const int32_t* len, const int64_t* base,
                   long long stride, const double* adv, double eps, double* out, double* stats,
                   void* stream);
/* amx_adv_whiten in two halves, for rows sharded over `world` ranks (statistics over the union).
 * amx_adv_whiten_parts: the rank's rows -> one record {count, mean, M2, residual} in slot `rank`
 * of msg (device fp64 [world][4], zeroed by the caller, so a SUM all-reduce over the ranks is an
 * all-gather): amx_adv_whiten's per-block parts in its block order, combined as it combines them
 * (mean and M2 about that mean as amx_adv_whiten's stats hold them); residual = what the mean's
 * rounding left of the rank's sum, kept only as far as mean + residual / count == mean.
 * amx_adv_whiten_apply: combines the `world` records in rank order with the same combine (the
 * apply kernel of amx_adv_whiten, its parts read from msg), writes stats = {mean, std} and
 * out = (adv - mean) / (std + eps) for the local rows.  world == 1 gives amx_adv_whiten's stats and
 * rows bit for bit.  Same context scratch as amx_adv_whiten (one whitening at a time);
 * 1 <= world <= 1024, 0 <= rank < world. */
int amx_adv_whiten_parts(amx_ctx* ctx, int T, int L, const int32_t* len, const int64_t* base, long long stride,
                         const double* adv, int rank, int world, double* msg, void* stream);
int amx_adv_whiten_apply(amx_ctx* ctx, int T, int L, const int32_t* len, const int64_t* base, long long stride,
                         const double* adv, const double* msg, int world, double eps, double* out, double* stats,
                         void* stream);

/* ---- fitting the value baseline (MLPBaseline.fit) ------------------------------ */

/* The fit supports the (S+4) -> H0 -> H1 -> 1 ReLU MLP with both hidden widths <= 128
 * (padded: H0p = H1p = 128; kf = round_up(S + 4, 32)) and mini-batches of 64 rows.
 * amx_vfit_work: bytes of the opaque fit workspace (the gathered batch, activations, their
 * gradients, the W1 gradient, the loss sum and the step's Adam constants); amx_vfit_param_count: floats of each
 * Adam moment vector, laid out W0 [H0p, kf] | b0 [H0p] | W1 [H1p, H0p] | b1 [H1p] |
 * w2 [H1p] | b2 [1].  Pure host arithmetic; -1 (and amx_last_error) for another shape. */
long long amx_vfit_work(int kf, int H0p, int H1p);
long long amx_vfit_param_count(int kf, int H0p, int H1p);

/* One epoch of mjrl's fit_data (mjrl/mjrl/utils/optimize_model.py:21-35) as
 * MLPBaseline.fit calls it (mjrl/mjrl/baselines/mlp_baseline.py:85): num_steps =
 * n_rows / 64 - 1 mini-batch steps; step mb takes rows perm[64 mb .. 64 mb + 63] of feat
 * [n_rows, ldf] (what amx_value_features writes) and of returns (f32), runs the forward
 * h0 = relu(x W0^T + b0), h1 = relu(h0 W1^T + b1), y^ = h1 . w2 + b2, loss = mean((y^ - y)^2),
 * autograd's backward (dy = 2 (y^ - y) / 64, ReLU mask "output > 0") and torch.optim.Adam
 * (no amsgrad; weight_decay added to every gradient, biases included):
 *   g += wd w;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *   w -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),
 * t = ++adam_step[0] (device memory, persists across epochs and fits like the reference's
 * optimizer; beta^t formed in double).  adam_m / adam_v: amx_vfit_param_count floats each,
 * zero before the first step.  Weights use DeviceMLPBaseline's padded layout (W0 [128, kf],
 * W1 [128, 128] row-major, zero padding); padded entries and their moments stay exactly 0.
 * All arithmetic is fp32, in a fixed order.  epoch_loss[0] (device) = sum of the step
 * losses / num_steps.  Rows past 64 (num_steps) of perm are not used; perm entries must lie
 * in [0, n_rows) (the kernels clamp).  A step is four launches on `stream`; nothing in them
 * waits on another workgroup.  One fit at a time per workspace. */
int amx_vfit_epoch(amx_ctx* ctx, int n_rows, const float* feat, int ldf, const float* returns,
                   const int32_t* perm, int kf, int H0p, int H1p, float* W0, float* b0, float* W1,
                   float* b1, float* w2, float* b2, float* adam_m, float* adam_v,
                   long long* adam_step, double lr, double beta1, double beta2, double eps,
                   double weight_decay, void* work, float* epoch_loss, void* stream);

/* ---- training the dynamics ensemble (DynamicsModel.train_step) ------------------ */

enum { AMX_EFIT_ADAM = 0, AMX_EFIT_SGD = 1 };

/* Sizes of the training vectors of the context's ensemble (host arithmetic; -1 and
 * amx_last_error for an unsupported depth).  amx_efit_param_count: floats per member of the
 * flat gradient and of each optimizer-state vector, laid out layer by layer as
 * W_i [N_i][K_i] | b_i [N_i] in the engine's padded dense-concat layout (N_i = hidden, K_i =
 * k0_pad + i*hidden; the last layer N = n_out_pad, K = ldk; on an AMX_CONNECT_PLAIN context
 * K_0 = k0_pad and K_i = hidden for every later layer).  amx_efit_work_floats: floats of
 * the opaque step workspace for batches padded to Bt rows (Bt % 128 == 0). */
long long amx_efit_param_count(const amx_ctx* ctx);
long long amx_efit_work_floats(const amx_ctx* ctx, int Bt);

/* One step of DynamicsModel.train_step (train = 1) or validate_step (train = 0),
 * milo/milo/dynamics.py:236-261, for all M members at once.  Member g's batch is rows
 * idx[g * strideIdx + r], r < n_b, of the fp32 device arrays states [n_rows][S], actions
 * [n_rows][A], next_states [n_rows][S] (indices are clamped to [0, n_rows)).  Inputs and the
 * target ((s' - s) - mu_d)/sd_d are normalised with the context's normalizers in the
 * reference's op order; the forward is amx_gemm_bias_act on the fp32 master weights W[i], b[i]
 * (host arrays of L + 1 device pointers, each [M][N_i][K_i] / [M][N_i]); loss[g * strideLoss]
 * (device) = nn.MSELoss over n_b x S.  train = 1 continues with autograd's backward (ReLU mask
 * "output > 0"), clip_grad_norm_(grad_clip) when grad_clip > 0 (coef = min(1, grad_clip /
 * (norm + 1e-6))) and the optimizer, torch's op for op:
 *   AMX_EFIT_ADAM (p1 = eps; betas 0.9, 0.999; state1 = exp_avg, state2 = exp_avg_sq):
 *     m += 0.1 (g - m);  v = 0.999 v + 0.001 g g;
 *     w -= (lr / (1 - 0.9^t)) m / (sqrt(v) / sqrt(1 - 0.999^t) + eps)
 *   AMX_EFIT_SGD (p1 = momentum, nesterov, dampening 0; state1 = momentum_buffer, state2 unused):
 *     buf = p1 buf + g;  w -= lr (g + p1 buf)
 * t = ++step[g] (device, one count per member).  grad / state1 / state2: [M][param_count]
 * floats; the states are zero before the first step.  All arithmetic is fp32 in a fixed order;
 * zero-padded weights and their state stay exactly 0.  A step is 3 L + 7 launches on
 * `stream` (3 L + 6 without grad_clip, L + 3 for train = 0); nothing in them waits on another workgroup and nothing is
 * allocated. */
int amx_efit_step(amx_ctx* ctx, int train, int n_b, int Bt, const int32_t* idx, long long strideIdx,
                  int n_rows, const float* states, const float* actions, const float* next_states,
                  float* const* W, float* const* b, float* grad, float* state1, float* state2,
                  long long* step, int optim, double lr, double p1, double grad_clip, float* loss,
                  long long strideLoss, float* work, void* stream);

/* ---- training the AMP/GAIL discriminator (GAILCost.update_disc) ------------------ */

enum { AMX_DFIT_SGD = 0, AMX_DFIT_ADAM = 1 };

/* General fp32 products on v_mfma_f32_32x32x2_f32 (64 x 64 tiles, LDS-staged operands, one
 * fp32 FMA chain per output element in ascending k), the backward products autograd runs for
 * a Linear layer (milo/milo/gail_cost.py:191, total_loss.backward()).  Plain row-major
 * operands with leading dimensions (multiples of 4 floats, 16-byte aligned bases).
 *   amx_gemm_nn_f32: C [M][N] = A [M][K] B [K][N]          (dX = dZ W with B = W [out][in])
 *   amx_gemm_tn_f32: C [M][N] = A^T B, A [R][M], B [R][N]  (dW = dZ^T X), and with colsum != NULL
 *                    colsum[m] = sum_{r < colsum_rows} A[r][m]  (db over a row prefix)
 * M % 64 == 0, N % 4 == 0, the reduction length (K, R) % 32 == 0.  mask != NULL applies the
 * epilogue C[r][n] = mask[r'][n] > 0 ? C[r][n] : 0 with r' = r % mask_mod (mask_mod = 0 and
 * amx_gemm_tn_f32: r' = r): the ReLU backward by the layer's output. */
int amx_gemm_nn_f32(amx_ctx* ctx, int M, int N, int K, const float* A, int lda, const float* B,
                    int ldb, float* C, int ldc, const float* mask, int ldm, int mask_mod,
                    void* stream);
int amx_gemm_tn_f32(amx_ctx* ctx, int R, int M, int N, const float* A, int lda, const float* B,
                    int ldb, float* C, int ldc, const float* mask, int ldm, float* colsum,
                    int colsum_rows, void* stream);

/* Sizes for amx_dfit_step (host arithmetic; -1 and amx_last_error for unsupported shapes; Dp %
 * 32 == 0, H0p and H1p % 128 == 0, Bt % 64 == 0).  amx_dfit_param_count: floats of each
 * optimizer-state vector, laid out W0 [H0p][Dp] | b0 [H0p] | W1 [H1p][H0p] | b1 [H1p] | w2
 * [H1p] | b2 [4].  amx_dfit_work_floats: floats of the opaque step workspace. */
long long amx_dfit_param_count(int Dp, int H0p, int H1p);
long long amx_dfit_work_floats(int Dp, int H0p, int H1p, int Bt);

/* One step of GAILCost.update_disc (milo/milo/gail_cost.py:169-204 with the losses of :104-140,
 * regularizer_loss :142-146 and expert_grad_pen :148-167) for the discriminator x -> relu(x
 * W0^T + b0) -> relu(. W1^T + b1) -> . w2 + b2 on the zero-padded fp32 device tensors W0
 * [H0p][Dp], b0 [H0p], W1 [H1p][H0p], b1 [H1p], w2 [H1p], b2 [4] (b2[1..3] zero).  The expert
 * batch is rows idx_e[r], r < bs, of expert [n_expert][ld_expert]; the agent batch rows idx_m[r]
 * of agent [n_agent][ld_agent] (a replay ring's physical rows), or rows 0 .. bs-1 with idx_m =
 * NULL (an uploaded batch); D valid columns each, indices clamped.  Bt >= bs is the padded
 * batch.  loss_type AMX_DISC_LEAST_SQUARES: e = mean (out_e - 1)^2, m = mean (out_m + 1)^2;
 * AMX_DISC_LOG_LIKELIHOOD: e = -mean log sigmoid(out_e), m = -mean log(1 - sigmoid(out_m)).
 * The gradient is that of scaling_coef e + (1 - scaling_coef) m + grad_lambda/2 mean_e |d out /
 * d x|_2 (the plain norm; rows of zero norm contribute no gradient, as torch's norm backward);
 * the regularizer reg_coef sum 1/2 |W|^2 over W0, W1, w2 is logged only (the reference detaches
 * it).  optim AMX_DFIT_SGD (p1 = momentum; no Nesterov, dampening or weight decay; state1 =
 * momentum_buffer, state2 unused): buf = p1 buf + g; w -= lr buf.  AMX_DFIT_ADAM (p1 = eps,
 * betas 0.9 / 0.999; state1 = exp_avg, state2 = exp_avg_sq), torch's single-tensor path as
 * amx_efit_step.  t = ++step[0] (device).  state1 / state2: amx_dfit_param_count floats, zero
 * before the first step.  metrics (device, 8 doubles) = expert loss, agent loss, gradient
 * penalty (x grad_lambda), regularizer (x reg_coef, of the weights before the step), total,
 * expert accuracy mean(out_e > 0), agent accuracy mean(out_m < 0), t.  All arithmetic is fp32
 * (the metrics' sums fp64) in a fixed order: a step is bit-reproducible; zero-padded weights
 * and their state stay exactly 0.  15 launches on `stream`; nothing in them waits on another
 * workgroup and nothing is allocated. */
int amx_dfit_step(amx_ctx* ctx, int loss_type, int optim, double lr, double p1, double scaling_coef,
                  double reg_coef, double grad_lambda, int bs, int Bt, int D, int Dp, int H0p,
                  int H1p, const int32_t* idx_e, const int32_t* idx_m, const float* expert,
                  long long ld_expert, int n_expert, const float* agent, long long ld_agent,
                  int n_agent, float* W0, float* b0, float* W1, float* b1, float* w2, float* b2,
                  float* state1, float* state2, long long* step, float* work, double* metrics,
                  void* stream);

/* ---- the behaviour-cloning warm start (BC.train) ------------------------------- */

enum { AMX_BC_MSE = 0, AMX_BC_MLE = 1 };

/* The fit supports what amx_npg_pass supports: the context's S -> 32 -> 32 -> A tanh MLP with
 * S <= 256 and A <= 64, theta in the reference's flat order (W1 | b1 | W2 | b2 | W3 | b3 |
 * log_std, amx_npg_param_count floats), and mini-batches of 64 rows.
 * amx_bcfit_work: bytes of amx_bcfit_eval's workspace (one fp64 partial per workgroup, 1024
 * workgroups at most: 8192); amx_bcfit_steps needs none.  Pure host arithmetic; -1 (and
 * amx_last_error) for another shape. */
long long amx_bcfit_work(int S, int A);

/* n_steps consecutive mini-batch steps of BC.fit's training loop
 * (mjrl/mjrl/algos/behavior_cloning.py:121-129) in one launch of one workgroup: step k gathers
 * rows idx[64 k .. 64 k + 63] of obs [N, ldo] and act [N, lda] (fp32, device: the reference's
 * torch.from_numpy(obs[idx]).float() applied to the whole set once), runs the policy's forward
 * mu = W3 tanh(W2 tanh(W1 x + b1) + b2) + b3 (gaussian_mlp.py:117 through FCNetwork with
 * identity transformations), the loss
 *   AMX_BC_MSE  mean over the 64 A elements of (mu - a)^2            (behavior_cloning.py:94-104),
 *   AMX_BC_MLE  -mean over the 64 rows of LL, LL = -0.5 sum z^2 - sum log_std - 0.5 A log(2 pi),
 *               z = (a - mu) / exp(log_std)   (behavior_cloning.py:82-92, gaussian_mlp.py:117-121),
 * autograd's backward and torch.optim.Adam's single-tensor update (no amsgrad; weight_decay
 * added to every gradient) exactly as amx_vfit_epoch states it, t = adam_step[0] + k + 1 with
 * beta^t formed in double.  Under AMX_BC_MSE log_std has no gradient: it, and its entries of
 * adam_m / adam_v, are left untouched (torch's Adam skips parameters whose grad is None).
 * log_std is not clamped.  step_loss[k] (device, n_steps floats) = step k's fp32 loss.
 * theta, adam_m, adam_v (amx_npg_param_count floats each; moments zero before the first step)
 * and adam_step[0] (+= n_steps) are read at the start of the launch and written at its end;
 * in between the parameters live in LDS and each parameter's moments in registers of the
 * thread that owns it.  All arithmetic is fp32 on the f32 matrix pipe in a fixed order, so
 * cutting a run of steps into several calls changes no bit of the result.  idx entries must
 * lie in [0, N) (the kernel clamps).  n_steps = 0 launches nothing.  No workgroup waits on
 * another: there is only one. */
int amx_bcfit_steps(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act,
                    long long lda, const int32_t* idx, int n_steps, float* theta, float* adam_m,
                    float* adam_v, long long* adam_step, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int loss_type, float* step_loss,
                    void* stream);

/* The loss of theta over all N rows, BC.fit's loss_before / loss_after
 * (behavior_cloning.py:115-117, 137-138): the same forward, 64 rows at a time on one workgroup
 * per compute unit; per-row terms in fp32, summed in fp64 per workgroup and then in workgroup
 * order into loss[0] (device).  work: amx_bcfit_work bytes.  Two launches on `stream`. */
int amx_bcfit_eval(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act,
                   long long lda, const float* theta, int loss_type, void* work, double* loss,
                   void* stream);

/* ---- the PPO policy update (PPO.train_from_paths) ------------------------------ */

enum { AMX_PPO_OLD_SNAPSHOT = 0, AMX_PPO_OLD_TRACKS_MEAN = 1 };

/* n_steps consecutive mini-batch steps of PPO.train_from_paths' loop
 * (mjrl/mjrl/algos/ppo_clip.py:88-97) in one launch of one workgroup, by the design and with the
 * shapes, theta / adam_m / adam_v / adam_step and idx of amx_bcfit_steps (its step body: the
 * AMX_BC_MLE forward, backward and Adam).  Step k also gathers adv[idx] (fp32 [N], already
 * whitened) and forms per row
 *   LL_new = (-0.5 sum_c z^2 - sum log_std) - 0.5 A log(2 pi),  z = (a - mu) / exp(log_std),
 *   LL_old: AMX_PPO_OLD_SNAPSHOT     ll_old[idx] (fp32 [N], amx_ppo_old_ll at the old theta);
 *           AMX_PPO_OLD_TRACKS_MEAN  the same sum from the step's own mu with log_std_old [A]
 *                                    (the old mean network shares the new one's storage),
 *   LR = exp(LL_new - LL_old),  lo / hi = float32(1 -/+ clip_coef),
 *   loss = -mean(min(LR adv, clamp(LR, lo, hi) adv))              (ppo_clip.py:48-55),
 * and autograd's gradient: d loss / d LL_new = -(1 / 64) g, g = adv LR pass, pass = 1 for
 * lo <= LR <= hi (min's two arguments are equal there and its halves add up; clamp passes at
 * its bounds), for LR > hi only where adv < 0 and for LR < lo only where adv > 0.  The
 * gradient flows through LL_new only.  All seven tensors take the Adam step (no weight decay);
 * log_std is not clamped.  step_loss[k] = the loss, step_clipped[k] = rows with LR outside
 * [lo, hi] (device, n_steps each).  The sum over c runs in one fixed order in both LLs and in
 * amx_ppo_old_ll, so equal policies give LR == 1 exactly; cutting a run of steps into several
 * calls changes no bit. */
int amx_ppo_steps(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act,
                  long long lda, const float* adv, const float* ll_old, const float* log_std_old,
                  int old_mode, const int32_t* idx, int n_steps, float* theta, float* adam_m,
                  float* adam_v, long long* adam_step, double lr, double beta1, double beta2,
                  double eps, double clip_coef, float* step_loss, int32_t* step_clipped,
                  void* stream);

/* ll_old[r] = LL of row r at theta for all N rows (device, fp32): the step kernel's forward and
 * row arithmetic, 64 rows at a time on one workgroup per compute unit.  One launch. */
int amx_ppo_old_ll(amx_ctx* ctx, int N, const float* obs, long long ldo, const float* act,
                   long long lda, const float* theta, float* ll_old, void* stream);

/* ---- RNG ----------------------------------------------------------------------- */

/* Philox4x32-10 block for (key = seed, counter = {ctr0, ctr1, ctr2, ctr3}), written
 * to out[4*i .. 4*i+3] for i < n with ctr0 += i.  Exposed for parity tests of the
 * device RNG the reset/policy kernels use. */
int amx_philox(amx_ctx* ctx, uint64_t seed, uint32_t ctr1, uint32_t ctr2, uint32_t ctr3,
               uint32_t* out, int n, void* stream);

/* Host-side (no device, no context) policy noise of the reference sampler, bit-exact with
 * numpy's legacy RandomState as mjrl MLP.get_action draws it (mjrl/mjrl/policies/
 * gaussian_mlp.py:95-104: np.random.uniform() for the eps test, then np.random.randn(A), per
 * step) after get_samples' np.random.seed(seed) (milo/milo/sampler.py:39).  `states` is host
 * memory of n_states * AMX_MT_STATE_BYTES; amx_mt_seed seeds states[slots[i]] with seeds[i]
 * (np.random.seed(int)); amx_mt_policy_noise advances states[slots[i]] by `steps` get_action
 * calls, writing the randn values to out[k * ld_step + slots[i] * ld_slot + a] (doubles). */
int amx_mt_seed(void* states, int n_states, const int32_t* slots, const uint32_t* seeds, int n);
int amx_mt_policy_noise(void* states, int n_states, const int32_t* slots, int n, int steps, int A,
                        double* out, long long ld_step, long long ld_slot);

#ifdef __cplusplus
}
#endif
#endif /* AMX_HIP_H */
