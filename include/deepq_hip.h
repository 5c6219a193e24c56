/*
 * deepq_hip.h -- C ABI of the MI355X-native DeepQ-Decoding hot path (libdeepq_hip.so).
 *
 * The reference (R-Sweke/DeepQ-Decoding) is pure Python and has no FFI layer; its boundary for
 * this path is two duck-typed Python protocols: the gym-style environment
 * `Surface_Code_Environment_Multi_Decoding_Cycles` (example_notebooks/Environments.py:10-385) and
 * the keras-rl `DQNAgent` surface used by the driver scripts
 * (cluster_scripts/d5_dp/0.001/Single_Point_Training_Script.py:109-152,206).  Each entry point
 * below names the reference interface it replaces.  The host-side mirror of those protocols
 * lives in `deepq-decoding_amd/` and reaches this library through ctypes.
 *
 * Conventions
 *   - every `*_dev` pointer is DEVICE memory owned by the caller (e.g. a torch tensor's data_ptr);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only ENQUEUES
 *     work on it and returns; nothing here synchronises unless its comment says so;
 *   - no call allocates or frees device memory except *_create / *_destroy / dq_env_build_referee,
 *     so step-type calls are hipGraph-capturable;
 *   - return value 0 = DQ_OK, negative = error; dq_last_error() gives a thread-local message;
 *   - no exceptions cross the ABI; a handle must not be used from two host threads at once.
 *
 * Bit conventions (shared with oracle/lattice.py)
 *   - qubit q = row*d + col is bit q of a "qubit mask";
 *   - stabilizers are numbered in the order generate_faulty_syndrome draws its uniforms
 *     (Function_Library.py:189-221): bulk plaquettes (a,b), 1<=a,b<=d-1 row-major, then row 0
 *     (b=1,3,..), row d (b=2,4,..), column 0 (a=2,4,..), column d (a=1,3,..); stabilizer s is bit s
 *     of a "syndrome word";
 *   - action a is bit a of a 128-bit "action mask" stored as two uint64 (lo, hi);
 *   - referee tables are bit-packed: entry i is bit (i & 31) of word i >> 5; index bit k is the
 *     k-th live plaquette of that type in row-major (a,b) order.
 *
 * Random numbers: Philox4x32-10, key = seed, counter = (t_lo, t_hi, env_id, lane | stream << 16)
 * (SURVEY.md §8c).  Stream 0 = environment noise with t = the lattice's measurement-round counter:
 * word 0 < ceil(p_phys*2^32) <=> qubit `lane` errs, word 1 -> Pauli type 1 + ((w*3) >> 32),
 * word 2 < ceil(p_meas*2^32) <=> stabilizer `lane` is mis-measured.
 */
#ifndef DEEPQ_HIP_H
#define DEEPQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int dq_status;
enum {
    DQ_OK = 0,
    DQ_ERR_INVALID = -1,     /* bad argument */
    DQ_ERR_UNSUPPORTED = -2, /* configuration outside what the kernels implement */
    DQ_ERR_HIP = -3,         /* a HIP runtime call failed */
    DQ_ERR_NOMEM = -4,
    DQ_ERR_STATE = -5,       /* call made in the wrong state (e.g. step before referee is set) */
    DQ_ERR_RANGE = -6        /* a value left the range the arithmetic carries (dq_qnet_range_check) */
};

/* DQ_MODEL_IIDXZ: independent X and Z flips per qubit (generate_IIDXZ_error, Function_Library.py:134-160: two uniforms per qubit, X
 * first) -- the noise channel generate_error() offers besides "X" and "DP" (Function_Library.py:91-92).  The reference's environment
 * constructor does not accept it (Environments.py:66-67 prints and then fails); here it runs with the depolarising model's action
 * layers (X and Z, or X/Y/Z with use_Y) and four homology classes (Function_Library.py:329-330). */
enum { DQ_MODEL_X = 0, DQ_MODEL_DP = 1, DQ_MODEL_IIDXZ = 2 };
enum { DQ_STREAM_ENV = 0, DQ_STREAM_POLICY = 1, DQ_STREAM_REPLAY = 2, DQ_STREAM_DROPOUT = 3, DQ_STREAM_INIT = 4 };

int dq_version(void);
/* sha256 (hex) over the CODE of the kernel sources this library was built from (csrc/, include/deepq_hip.h; comments and whitespace stripped:
 * deepq-decoding_amd/_digest.py): a binding compares it with the tree's, so that a prebuilt .so carried to another box is known to be the one these sources
 * build (tests/test_abi.py, the -m gpu suite). */
const char* dq_build_digest(void);
const char* dq_last_error(void);
/* sizeof() of the public structs as THIS library was compiled: 0 dq_env_cfg, 1 dq_env_info, 2 dq_sample_job, 3 dq_qnet_cfg, 4 dq_qnet_job, 5 dq_td_job,
 * 6 dq_env_step_job, 7 dq_env_ring, 8 dq_decode_cfg (dq_decode_create's and dq_decode_wide_create's); -1 for any other id.  A binding (the ctypes structures of _lib.py) checks its own layouts against it: a struct of the wrong size handed
 * across the boundary is silent memory corruption (tests/test_abi.py).  No reference counterpart. */
long dq_struct_size(int id);
/* Number of visible HIP devices (0 if none / runtime unavailable).  Never fails. */
int dq_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Environment: replaces Surface_Code_Environment_Multi_Decoding_Cycles (Environments.py:10-385),
 * batched over n_envs independent lattices, one lattice per wavefront.
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_env dq_env;

typedef struct {
    int32_t d;            /* code distance: 3, 5 or 7 (Environments.py:45; odd, Function_Library.py:28-29) */
    int32_t error_model;  /* DQ_MODEL_X / DQ_MODEL_DP (Environments.py:56-67) / DQ_MODEL_IIDXZ */
    int32_t use_Y;        /* Environments.py:60-65 */
    int32_t volume_depth; /* 1..16 (Environments.py:52) */
    int32_t n_envs;       /* lattices owned by this handle */
    uint32_t env_id_base; /* global id of lattice 0 (rank * n_local): results do not depend on sharding */
    uint32_t seed[2];     /* Philox key */
} dq_env_cfg;

typedef struct {
    int32_t num_actions;     /* Environments.py:57-64 */
    int32_t n_action_layers; /* Environments.py:58-65 */
    int32_t identity_index;  /* Environments.py:69 */
    int32_t obs_c, obs_h, obs_w; /* observation_space.shape, Environments.py:78-82 */
    int32_t n_stab;          /* d*d - 1 live stabilizers */
    int32_t state_words;     /* uint64 words per lattice in dq_env_export_state */
} dq_env_info;

dq_status dq_env_create(const dq_env_cfg* cfg, dq_env** out);     /* Environments.py:45-97 */
void dq_env_destroy(dq_env* env);
dq_status dq_env_get_info(const dq_env* env, dq_env_info* out);

/* env.p_phys / env.p_meas are plain attributes the drivers mutate between test sweeps
 * (Single_Point_Training_Script.py:200-201); converted to integer thresholds on the host. */
dq_status dq_env_set_rates(dq_env* env, double p_phys, double p_meas);
/* Per-lattice rates: lattice i (local index) runs at p_phys[i], p_meas[i] -- every threshold compare of its steps and of its resets'
 * initialize_state rejection loop (Environments.py:157-172) -- and keeps its own Philox stream, so a lattice's trajectory equals that of a
 * uniform-rate handle at its rates (same seed, env_id_base = its global id).  p_phys / p_meas: HOST arrays of n == n_envs doubles, each
 * finite and in [0, 1] (else DQ_ERR_INVALID, nothing changed); the thresholds are those of dq_env_set_rates.  The handle owns the device
 * table (freed by dq_env_destroy).  The upload is ordered on `stream`: launches on it after the call see the new rates, launches before it
 * finish reading the old ones first; the caller may free its arrays on return.  Satisfies dq_env_set_rates' precondition; a later
 * dq_env_set_rates returns the handle to one pair of rates for all lattices.  The referee is not touched (it is the one installed). */
dq_status dq_env_set_rates_per_lattice(dq_env* env, const double* p_phys, const double* p_meas, int n, void* stream);

/* Referee ("static_decoder", Environments.py:53,144,150).  The reference's Keras referee blobs are
 * not in the checkout; the library builds the deterministic minimum-weight look-up referee defined
 * in oracle/referee.py ON THE GPU (level-synchronous BFS).  Synchronises `stream`. */
dq_status dq_env_build_referee(dq_env* env, void* stream);
/* ... or the maximum-likelihood referee for independent component flips with probability q_flip per qubit: exact
 * class posteriors by one XOR-convolution pass per qubit over the (syndrome, class) space, same table format.  Synchronises `stream`. */
dq_status dq_env_build_referee_ml(dq_env* env, double q_flip, void* stream);
/* ... or installs caller-provided bit-packed tables (device pointers, 2^((d*d-1)/2) bits each; must
 * stay alive while the handle uses them).  lut_z_dev may be NULL for DQ_MODEL_X. */
dq_status dq_env_set_referee(dq_env* env, const uint32_t* lut_x_dev, const uint32_t* lut_z_dev);
/* ... or ONE table over the whole syndrome: entry s (bit i of s = stabilizer i in generate_faulty_syndrome's draw order,
 * Function_Library.py:189-221) holds the class the referee predicts, X + 2 Z (generate_one_hot_labels_surface_code's index,
 * Function_Library.py:329-334), 2 bits per entry, 16 entries per word: 2^n_stab entries, n_stab <= 24 (d <= 5; 4 MB at d = 5).  This is
 * how an arbitrary `static_decoder.predict` object (Environments.py:144,150 -- only argmax of its output is used) runs inside the
 * kernel: the host tabulates it once (deepq-decoding_amd/env.py VectorEnv.set_referee_predict).  Device pointer, caller-owned. */
dq_status dq_env_set_referee_joint(dq_env* env, const uint32_t* lut_dev);
/* A Dense-stack referee evaluated ON THE DEVICE, for lattices whose syndromes no table holds (d = 7: 48 stabilizers) -- the reference's
 * own referee is such a network, "a fast feed-forward NN homology class predictor" loaded with keras load_model and called once per
 * step on the flattened (d+1)^2 syndrome of the state after the agent's move (Environments.py:53,139-144,
 * Single_Point_Training_Script.py:54-57); only the arg-max of its output is used (Environments.py:150).
 *   n_layers     1 .. 6 Dense layers, ReLU between them (the top layer's softmax is monotone and not evaluated)
 *   dims         int32 [n_layers + 1]: (d+1)^2, the hidden widths (<= 2048), then 2 ("X") or 4 classes
 *   weights_dev  float, caller-owned, must outlive its use: per layer the kernel [in][out] row-major (Keras shape), then the bias
 * Arithmetic (fixed, so that a host restatement gives the same bits -- referee.py FeedForwardReferee.predict_exact): float32, bias
 * first, inputs in increasing index order, one rounded multiply and one rounded add per term, first maximum of the outputs.
 * Every step then runs a pre-pass (one wavefront per lattice) before the environment kernel; dq_env_act_step selects the actions with
 * dq_policy_select first (legal_dev must hold the current legal sets, as every reset / step leaves them); the step does not ride on
 * the dense backward (dq_qnet_td_backward_*_env: DQ_ERR_UNSUPPORTED).  n_layers = 0 uninstalls it; installing any table referee does
 * too.  d <= 7. */
dq_status dq_env_set_referee_mlp(dq_env* env, int n_layers, const int32_t* dims, const float* weights_dev);
/* What the Dense-stack referee says about every lattice as it stands after action_dev[i] (int32 [n_envs]; the identity leaves the state as
 * it is): classes_dev uint8 [n_envs] = arg-max class.  The lattices are not stepped.  Tests and diagnostics (the step runs the same
 * pre-pass itself). */
dq_status dq_env_referee_classes(dq_env* env, const int32_t* action_dev, uint8_t* classes_dev, void* stream);

/* Copies the referee tables to host memory as one byte per entry (tests). Synchronises. */
dq_status dq_env_get_referee(dq_env* env, uint8_t* lut_x_host, uint8_t* lut_z_host, size_t entries);

/* reset(): Environments.py:99-115 + initialize_state 206-235 + reset_legal_moves 238-258.
 * which_dev == NULL resets every lattice, else lattice i iff which_dev[i] != 0 (others keep their
 * state; outputs are written for all lattices).  Nullable outputs are skipped.
 *   obs_dev      uint8 [n_envs, C, H, W]   (0/1 cells)
 *   legal_dev    uint64 [n_envs, 2]        action mask of env.legal_actions
 *   lifetime_dev uint32 [n_envs]           env.lifetime */
dq_status dq_env_reset(dq_env* env, const uint8_t* which_dev, uint8_t* obs_dev, uint64_t* legal_dev,
                       uint32_t* lifetime_dev, void* stream);

/* step(action): Environments.py:118-204.  An action outside [0, num_actions) is treated as the
 * identity.  auto_reset != 0: a lattice whose `done` flag is set when the call starts is reset
 * instead of stepped -- its action is ignored, reward 0, done 0 -- which is keras-rl's convention of
 * spending one agent step on the terminal observation before env.reset(); auto_reset == 0 keeps the
 * reference's sticky `done` (Environments.py:151 never clears it).
 *   action_dev    int32 [n_envs]
 *   reward_dev    float [n_envs]     (Environments.py:146-149)
 *   done_dev      uint8 [n_envs]     (Environments.py:150-151)
 *   was_reset_dev uint8 [n_envs]     1 where auto_reset replaced the step */
dq_status dq_env_step(dq_env* env, const int32_t* action_dev, int auto_reset, uint8_t* obs_dev,
                      float* reward_dev, uint8_t* done_dev, uint64_t* legal_dev, uint32_t* lifetime_dev,
                      uint8_t* was_reset_dev, void* stream);

/* dq_policy_select (declared below; same rule, same Philox stream, on the lattices' CURRENT legal sets) followed by dq_env_step,
 * in one launch: keras-rl's `action = policy.select_action(q_values)` + `env.step(action)` of one agent step.  The selected
 * actions are written to action_dev (the replay memory needs them); q_dev == NULL explores always. */
dq_status dq_env_act_step(dq_env* env, const float* q_dev, double eps, int masked_greedy, const uint32_t seed[2], uint64_t t,
                          int32_t* action_dev, int auto_reset, uint8_t* obs_dev, float* reward_dev, uint8_t* done_dev,
                          uint64_t* legal_dev, uint32_t* lifetime_dev, uint8_t* was_reset_dev, void* stream);

/* dq_env_act_step plus the replay sampling (dq_replay_sample's rule, same Philox stream) for a later update, in the same launch: the
 * rule reads terminal flags no newer than slot head_slot - 3, so the job may describe the update that follows this step (head_slot /
 * filled_slots AFTER this step; head_slot = the slot the successor observations go to) or the one after the NEXT step (one more slot;
 * its newest candidate row is then the transition this very launch records). */
typedef struct dq_sample_job {
    const uint8_t* terminal_ring_dev;
    int n_slots, head_slot, filled_slots, batch;
    uint32_t seed[2];
    uint64_t t;                 /* number of the update the minibatch is for (counts from 1) */
    uint32_t sample_base;       /* first global sample id of this rank's minibatch */
    int32_t* index_dev;         /* int32 [batch] out */
} dq_sample_job;
dq_status dq_env_act_step_sample(dq_env* env, const float* q_dev, double eps, int masked_greedy, const uint32_t seed[2], uint64_t t,
                                 int32_t* action_dev, int auto_reset, uint8_t* obs_dev, float* reward_dev, uint8_t* done_dev,
                                 uint64_t* legal_dev, uint32_t* lifetime_dev, uint8_t* was_reset_dev, const dq_sample_job* sample,
                                 void* stream);

/* n_steps consecutive agent steps of an ACTING loop in one launch (round 6; SURVEY.md section 7 "hard parts": a 4096-lattice step is launch-latency-bound):
 * per step s = 0 .. n_steps - 1 -- dq_env_act_step with q_dev == NULL (uniform over the legal moves: keras-rl's warm-up / random policy), policy counter
 * t0 + s -- the transition lands in the caller's replay ring: slot c = (slot0 + s) mod n_slots of action_ring_dev int32 [n_slots][n_envs], reward_ring_dev
 * float [n_slots][n_envs] and done_ring_dev uint8 [n_slots][n_envs] (each nullable but the first), the successor observation in slot c + 1 (mod n_slots) of
 * obs_ring_dev uint8 [n_slots][n_envs][C][H][W] and / or patch_ring_dev uint32 [n_slots][n_envs][patch_stride_words] (nullable).  legal_dev / lifetime_dev /
 * was_reset_dev receive the LAST step's values.  Same bits as n_steps calls of dq_env_act_step(NULL, ...) with the same counters (tests run the C oracle's 60-step
 * comparison through this entry).  d <= 5 runs as ONE launch with the lattices' state in registers from step to step; d = 7 (and a Dense-stack referee) as
 * n_steps launches.  Does not consume a dq_env_patch_output arming. */
typedef struct dq_env_ring {
    int32_t* action_ring_dev;
    float* reward_ring_dev;
    uint8_t* done_ring_dev;
    uint8_t* obs_ring_dev;
    uint32_t* patch_ring_dev;
    int32_t patch_stride_words;
    int32_t n_slots, slot0;
} dq_env_ring;
dq_status dq_env_act_steps(dq_env* env, int n_steps, const uint32_t seed[2], uint64_t t0, const dq_env_ring* ring, int auto_reset, uint64_t* legal_dev,
                           uint32_t* lifetime_dev, uint8_t* was_reset_dev, void* stream);

/* Compact observation ("patch words").  The observation the reference builds -- padding_syndrome / padding_actions,
 * Environments.py:273-314 -- feeds Conv2D(64, 3, strides=2) (Function_Library.py:353): output pixel (oy, ox) of that convolution sees
 * the 3 x 3 patch at padded cell (2 oy, 2 ox), of which only the four CORNERS of every syndrome plane (even-even cells: grid cells
 * (oy + dy, ox + dx) of the faulty syndrome, Environments.py:292-294) and the CENTRE of every action plane (the odd-odd cell of qubit
 * oy d + ox, Environments.py:309-312) are data; every other cell is a constant of the embedding (Environments.py:284-298).  A lattice's
 * observation is therefore d * d words, one per output pixel p = oy d + ox:
 *     bit 4 j + 2 dy + dx   = faulty syndrome plane j (j < volume_depth) at grid cell (oy + dy, ox + dx)
 *     bit 4 volume_depth + l = action plane l (l < n_action_layers) at qubit p
 * (the padded uint8 image is a fixed function of these words and back; 4 volume_depth + n_action_layers <= 32 required, else
 * DQ_ERR_UNSUPPORTED).  This call ARMS the handle: the NEXT launch that resets or steps its lattices -- dq_env_reset, dq_env_step,
 * dq_env_act_step(_sample), or the step riding on dq_qnet_td_backward_*_env -- ALSO writes uint32 patch_dev[i * stride_words + p] for every
 * lattice i (stride_words >= d * d; the words between d * d and the stride are left alone); that launch's obs_dev may then be NULL.
 * One call arms one launch; patch_dev == NULL disarms.  The Q-network reads such rows directly (dq_qnet_job.reserved bit 0,
 * dq_qnet_set_patch_input).  No reference counterpart: the reference stores the padded int64 image (6.8 KB per d = 5 observation). */
dq_status dq_env_patch_output(dq_env* env, uint32_t* patch_dev, int stride_words);

/* Hidden state for tests / checkpointing: uint64 [n_envs, state_words], state_words = 11 + volume_depth:
 *   0 xmask (hidden_state codes 1,2)   1 zmask (codes 2,3)
 *   2 current_true_syndrome word       3 OR of the volume's faulty words (summed_syndrome_volume != 0)
 *     (2 and 3 are recomputed on the device at export and ignored by import)
 *   4 acted_on_qubits   5 measurement-round counter   6,7 completed_actions mask   8,9 legal_actions mask
 *   10 lifetime | done << 32           11.. faulty syndrome words of the current volume. */
dq_status dq_env_export_state(dq_env* env, uint64_t* state_dev, void* stream);
dq_status dq_env_import_state(dq_env* env, const uint64_t* state_dev, void* stream);

/* Static lattice tables as the kernels use them (tests compare them with the reference's
 * generateSurfaceCodeLattice / get_stabilizer_list / get_qubit_neighbour_list outputs).
 * Host pointers, each 64 entries: stab_qmask[s], qubit_smask[q], neigh_qmask[q]; stab_type[s] in {1,3,0}. */
dq_status dq_env_get_tables(const dq_env* env, uint64_t* stab_qmask, uint64_t* qubit_smask,
                            uint64_t* neigh_qmask, uint8_t* stab_type);

/* ---------------------------------------------------------------------------------------------
 * Matching referee: the referee of Environments.py:53,144,150 for lattices whose syndrome space no longer fits
 * a look-up table (d >= 9; README.md:278 allows "any perfect-measurement decoding algorithm").  Same definition as dq_env_build_referee's
 * tables -- class 1 iff the lightest error with that syndrome and class 1 is strictly lighter than the lightest with class 0 -- computed
 * per syndrome: minimum-weight perfect matching of the defects (with each other or a boundary) with class bookkeeping, solved exactly by
 * dynamic programming over defect subsets, one wavefront per syndrome (csrc/match_dev.h; numpy restatement oracle/matching_referee.py).
 * Equals the look-up referee at d <= 7 for every syndrome.  3 <= d <= 15, odd.
 *   defects_dev  uint64 [batch][2 components][2 words]: bit i of a component = its i-th plaquette in row-major (a, b) order (the
 *                look-up referee's index convention); component 0 = type-3 plaquettes (X part), 1 = type-1 plaquettes (Z part)
 *   class_dev    uint8 [batch]: X part (+ 2 * Z part when both_components != 0) -- generate_one_hot_labels_surface_code's index
 *   inexact_dev  uint8 [batch] or NULL: 1 where the answer is not exact.  The defects are split into CLUSTERS (pairs that can never be worth
 *                matching -- two boundary paths of the same total class are no longer -- separate them; the clusters' weights combine exactly) and
 *                a cluster of up to max_defects (20) defects is matched exactly: up to 14 in LDS, beyond that in a scratch table in device
 *                memory (rare, slower).  Inexact: a cluster beyond max_defects (its lowest max_defects matched exactly, the others sent to
 *                their nearer boundary) or more than 32 defects in one component (those beyond the 32nd likewise)
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_match dq_match;
dq_status dq_match_create(int d, dq_match** out);
void dq_match_destroy(dq_match* m);
dq_status dq_match_info(const dq_match* m, int* nodes_per_component, int* max_defects, int* w10);
/* host copies of one component's tables (tests): dist uint8 [n][n][2], distB uint8 [n][2] (255: no such path), w10 */
dq_status dq_match_get_tables(const dq_match* m, int component, uint8_t* dist_host, uint8_t* distB_host, int* w10);
dq_status dq_match_decode(const dq_match* m, const uint64_t* defects_dev, int batch, int both_components, uint8_t* class_dev,
                          uint8_t* inexact_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Wide environment: the same Surface_Code_Environment_Multi_Decoding_Cycles (Environments.py:10-385) for lattices beyond one 64-bit word
 * per bit-plane -- any odd 3 <= d <= 15, i.e. the d >= 9 the dq_env_* kernels (one word per plane, look-up referee) cannot hold
 * (csrc/env_big.hip).  Same configuration struct, same call semantics and Philox streams as dq_env_*; differences:
 *   - legal sets are legal_words = ceil(num_actions / 64) uint64 per lattice (dq_envb_get_info), legal_dev is uint64 [n_envs][legal_words];
 *   - the referee is the matching referee above, built by dq_envb_create and evaluated inside every step (inexact_dev, uint8 [n_envs]
 *     or NULL, reports where its more-than-max_defects fallback was used);
 *   - dq_envb_export_state: uint64 [n_envs][state_words] = x[W] z[W] true_syndrome[W] summed_volume[W] acted[W] round completed[LW]
 *     legal[LW] (lifetime | done << 32) volume[depth][W], W = ceil(d*d / 64), LW = legal_words.
 * At d <= 7 every output equals dq_env_*'s (with its default look-up referee) bit for bit.
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_envb dq_envb;
dq_status dq_envb_create(const dq_env_cfg* cfg, dq_envb** out);
void dq_envb_destroy(dq_envb* env);
dq_status dq_envb_get_info(const dq_envb* env, dq_env_info* out, int* legal_words);
dq_status dq_envb_set_rates(dq_envb* env, double p_phys, double p_meas);
/* dq_env_set_rates_per_lattice for the wide handle (same semantics) */
dq_status dq_envb_set_rates_per_lattice(dq_envb* env, const double* p_phys, const double* p_meas, int n, void* stream);
dq_status dq_envb_reset(dq_envb* env, const uint8_t* which_dev, uint8_t* obs_dev, uint64_t* legal_dev, uint32_t* lifetime_dev, void* stream);
dq_status dq_envb_step(dq_envb* env, const int32_t* action_dev, int auto_reset, uint8_t* obs_dev, float* reward_dev, uint8_t* done_dev,
                       uint64_t* legal_dev, uint32_t* lifetime_dev, uint8_t* was_reset_dev, uint8_t* inexact_dev, void* stream);
/* dq_policy_select_wide on the lattices' current legal sets followed by dq_envb_step, in one launch (cf. dq_env_act_step) */
dq_status dq_envb_act_step(dq_envb* env, const float* q_dev, double eps, int masked_greedy, const uint32_t seed[2], uint64_t t,
                           int32_t* action_dev, int auto_reset, uint8_t* obs_dev, float* reward_dev, uint8_t* done_dev, uint64_t* legal_dev,
                           uint32_t* lifetime_dev, uint8_t* was_reset_dev, uint8_t* inexact_dev, void* stream);
dq_status dq_envb_export_state(dq_envb* env, uint64_t* state_dev, void* stream);
/* The referee of the wide environment's step.  dq_version() stays 8: the capability is the presence of this symbol.
 * DQ_REFEREE_MATCHING (the state after dq_envb_create): the matching referee above.  DQ_REFEREE_UNION_FIND: the union-find referee -- section 20's closed
 * union-find decode of the perfect syndrome on a one-round window, one Pauli component per wavefront (csrc/uf_plane_dev.h; dq_uf_referee_decode below is
 * the same function on given defects): no scratch pool, no lock, no fallback, so inexact_dev receives zeros.  The handle owns the tables it needs (built at
 * the first choice of union-find: DQ_ERR_NOMEM / DQ_ERR_HIP, the setting then stays as it was).  Any other kind, or a null handle, is DQ_ERR_INVALID.  Every
 * later launch that steps the lattices -- dq_envb_step, dq_envb_act_step, and so every selection that rides on them -- follows the setting; resets, exports
 * and the lattices' records do not depend on it, so it may be switched between any two steps. */
#define DQ_REFEREE_MATCHING 0
#define DQ_REFEREE_UNION_FIND 1
dq_status dq_envb_set_referee(dq_envb* env, int kind);
/* dq_policy_select (below) over legal sets of legal_words uint64 per lattice: same rule, same Philox words */
dq_status dq_policy_select_wide(const float* q_dev, const uint64_t* legal_dev, int n, int n_actions, int legal_words, double eps,
                                int masked_greedy, const uint32_t seed[2], uint32_t env_id_base, uint64_t t, int32_t* action_dev,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Action selection: replaces EpsGreedyQPolicy / GreedyQPolicy(masked_greedy=...) of the keras-rl
 * fork (call sites Single_Point_Training_Script.py:110-115,166-167; README.md:168,262).
 *   q_dev      float [n, n_actions] or NULL (then every lattice explores: uniform over legal)
 *   legal_dev  uint64 [n, 2]
 * Per lattice i, words w = Philox(key=seed, ctr=(t_lo, t_hi, env_id_base+i, DQ_STREAM_POLICY<<16)):
 *   explore <=> w[1] < ceil(eps * 2^32);  explore action = k-th smallest legal action,
 *   k = (w[0] * n_legal) >> 32;  otherwise argmax_a q (first maximum), over the legal set only when
 *   masked_greedy != 0.
 * ------------------------------------------------------------------------------------------- */
dq_status dq_policy_select(const float* q_dev, const uint64_t* legal_dev, int n, int n_actions, double eps,
                           int masked_greedy, const uint32_t seed[2], uint32_t env_id_base, uint64_t t,
                           int32_t* action_dev, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Q-network: replaces the Keras model of build_convolutional_nn (Single_Point_Training_Script.py:61-90)
 * under keras-rl's dueling head (DQNAgent(enable_dueling_network=True), :119-127):
 *   Conv2D(valid, channels_first)+ReLU x n_conv -> Flatten -> [Dense+ReLU+Dropout] x n_ff -> Dense(n_actions)
 *   -> (dueling) Dense(n_actions+1), Q = y0 + y[1:] - mean(y[1:]).
 * Parameters live in ONE flat float buffer owned by the caller, in Keras order and Keras shapes (conv
 * kernels HWIO, dense (in,out)), each layer kernel then bias -- the tensors of a Keras .h5f drop in as is.
 * f32 results throughout (the reference is fp32 and the parity bound is 1e-5).  The per-layer path multiplies on the f32-input MFMA;
 * the fused chains carry every f32 operand as two f16 pieces (22 significant bits, round to nearest) and issue three f16 MFMAs per
 * product with f32 accumulation (two where an operand is binary): error below that of an ordinary f32 GEMM's accumulation, different
 * summation order (csrc/qnet.h "f16x2").  Operands of the fused chains must be finite and below 65504 in magnitude.
 * Alignment: params_dev must be 16-byte aligned wherever the fused chains run (they read bias rows as 16-byte words; DQ_ERR_INVALID before any
 * launch otherwise); q_dev, dq_dev, grads_dev, m_dev, v_dev and index_dev need only their element's 4 bytes (where all of grads_dev, m_dev and
 * v_dev are 16-byte aligned the final reduction takes 16-byte accesses: the same bits).
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_qnet dq_qnet;

typedef struct {
    int32_t in_c, in_h, in_w;   /* env.observation_space.shape (Single_Point_Training_Script.py:108) */
    int32_t n_conv;             /* 1..4 */
    int32_t conv[4][3];         /* [filters, kernel, stride]  ("c_layers"); stride > 1 only on the first */
    int32_t n_ff;               /* 0..4 hidden dense layers ("ff_layers") */
    int32_t ff_units[4];
    float ff_dropout[4];
    int32_t n_actions;          /* env.num_actions */
    int32_t dueling;            /* enable_dueling_network */
    int32_t max_batch;          /* workspaces are sized for this many samples */
} dq_qnet_cfg;

dq_status dq_qnet_create(const dq_qnet_cfg* cfg, dq_qnet** out);
void dq_qnet_destroy(dq_qnet* net);
size_t dq_qnet_param_count(const dq_qnet* net);
int dq_qnet_num_layers(const dq_qnet* net);
/* Offsets (in floats) of layer `layer`'s kernel and bias in the flat buffer and the kernel's Keras shape. */
dq_status dq_qnet_layer_info(const dq_qnet* net, int layer, int64_t* kernel_offset, int64_t* bias_offset,
                             int32_t shape[4], int32_t* n_dims);

/* Two forward implementations exist, both HIP: per-layer implicit GEMMs, and (default, when the configuration
 * fits) the fused LDS-resident chains of csrc/fused.hip.  dq_qnet_set_fused(net, 0) selects the per-layer path.  Each path's
 * training forward saves its activations in the form ITS backward reads (the fused one mostly as f16 piece planes), so a backward
 * must run on the path its training forward ran on: switching between the two calls makes the backward return DQ_ERR_STATE. */
dq_status dq_qnet_set_fused(dq_qnet* net, int enable);
/* Where the fused path has several FORMS of a kernel (same results to round-off, different summation order), which one this handle runs; a negative value keeps
 * the current choice.  conv_forward_form: 0 = conv_wave_kernel where it applies (patch words, d = 5), 1 = the workgroup-per-group kernels.  conv_backward_form:
 * 0 = conv_bwd16_kernel where it applies and the minibatch is >= 1024, 1 = conv_bwd_chain_kernel always, 2 = conv_bwd16_kernel whatever the minibatch.
 * conv_backward_a1: 0 = where a conv_wave_kernel training forward is followed by conv_bwd16_kernel, the forward does not save the first convolution's output and
 * the backward recomputes it from the patch words (the forward's own instructions: bit-identical gradients, 52 MB less HBM traffic per update at 4096 samples),
 * 1 = every training forward saves it and every backward reads the saved planes.  Set between a training forward and its backward, a change that makes the
 * backward need what the forward did not save is refused there (DQ_ERR_STATE).  The initial values come from DQ_CONV_FORM (=group -> 1) / DQ_CONV_BWD_FORM
 * (=8 -> 1, =16 -> 2) / DQ_CONV_BWD_A1 (=saved -> 1) read ONCE by dq_qnet_create; nothing re-reads the environment per call, so every rank that created its handle
 * under the same environment sums in the same order.  A/B measurements and tests.  No reference counterpart. */
dq_status dq_qnet_set_kernel_forms(dq_qnet* net, int conv_forward_form, int conv_backward_form, int conv_backward_a1);
/* 1 when the fused chains cover this configuration's FORWARD (inference jobs run on them, dq_qnet_pack applies). */
int dq_qnet_fused_supported(const dq_qnet* net);
/* 1 when they cover its BACKWARD as well -- a narrower set: at most 112 outputs in the widest head layer (111 actions with a dueling head) and observations of
 * at most 2045 bytes.  Only then do training forwards, dq_qnet_backward* and the dq_qnet_td_backward_*_env calls take the fused chains.  Where the forward alone is
 * covered ("mixed": e.g. d = 7 lattices with 10 input planes, 112..127 actions) every inference forward stays fused, every training forward and every backward
 * runs per layer (f32), and the *_env calls return DQ_ERR_UNSUPPORTED.  A dq_qnet_forward_multi call with a training job then runs its inference jobs as ONE
 * fused launch pair (with the packed weights they bring) and the training job per layer: every job gives the bits of a dq_qnet_forward call of its own.
 * dq_qnet_range_check on such a handle reports the fused FORWARD's guard only; dq_qnet_adam_step does not guard there (it propagates like dq_adam_step). */
int dq_qnet_fused_backward_supported(const dq_qnet* net);

/* model.predict_on_batch (training == 0) / the forward half of train_on_batch (training != 0: dropout
 * active, activations kept for dq_qnet_backward).
 *   obs_dev    uint8 [rows, C, H, W]; sample b reads row  b                         if index_dev == NULL,
 *                                                     row (index_dev[b] + index_off) mod index_mod otherwise
 *              (the replay-minibatch gather happens inside the first convolution's loader).  Rows are copied as whole
 *              aligned 16-byte words, so the words that straddle a row's ends are read too: obs_dev must point into an
 *              allocation that starts 16-byte aligned and whose allocated size is a multiple of 16 (any hipMalloc / torch
 *              allocation: both round sizes up to at least 256 bytes; views at arbitrary byte offsets inside it are fine);
 *   q_dev      float [batch, n_actions];
 *   dropout    one Philox call covers eight consecutive units of a sample, 16 bits per decision:
 *              keep(b, j) <=> half-word (j & 7) of Philox(key=seed, ctr=(t_lo, t_hi, sample_base + b, (j>>3) | DQ_STREAM_DROPOUT<<16 | l<<24))
 *              >= ceil(rate * 2^16)   (half-word h = bits 16 (h & 1) .. + 15 of word h >> 1);  kept units are scaled by
 *              1/(1-rate) (Keras K.dropout).  l = the ordinal of the dropout layer among the hidden layers with a rate > 0 (0 for the first, the only
 *              one of the reference's stack): every dropout layer draws a mask of its own, as Keras does. */
dq_status dq_qnet_forward(dq_qnet* net, const float* params_dev, const uint8_t* obs_dev, const int32_t* index_dev,
                          int index_off, int index_mod, int batch, int training, const uint32_t seed[2], uint64_t t,
                          uint32_t sample_base, float* q_dev, void* stream);

/* Several forwards in ONE pair of launches (e.g. Q_target(s1), Q_online(s1) and the training forward on s0 of one DQN
 * update): each job has the meaning of one dq_qnet_forward call; at most 4 jobs, at most one of them training.  With the
 * fused chains a lone 4096-sample forward is one workgroup per CU; sharing a grid lets the jobs' phases overlap. */
typedef struct {
    const float* params_dev;
    const uint8_t* obs_dev;
    const int32_t* index_dev;   /* nullable */
    int32_t index_off, index_mod, batch, training;
    uint32_t seed[2];
    uint64_t t;
    uint32_t sample_base;
    uint32_t reserved;          /* bit 0: obs_dev holds PATCH WORDS (dq_env_patch_output) -- uint32 [rows, stride_words], 16-byte aligned rows -- instead
                                 * of padded uint8 images (needs dq_qnet_set_patch_input; every job of a launch in the same form); other bits 0 */
    float* q_dev;
    const void* packed_dev;     /* dq_qnet_pack(params_dev) output, or NULL: the call packs the weights itself (one extra small launch) */
} dq_qnet_job;
dq_status dq_qnet_forward_multi(dq_qnet* net, int n_jobs, const dq_qnet_job* jobs, void* stream);

/* Patch-word input.  Declares that the network's first `n_syndrome_planes` input planes are padding_syndrome planes and the rest
 * padding_actions planes (Environments.py:273-314; the observation of Surface_Code_Environment_Multi_Decoding_Cycles with
 * volume_depth = n_syndrome_planes), so that Conv2D(64, 3, strides=2) (Function_Library.py:353) can read an observation as the d * d
 * patch words of dq_env_patch_output instead of the (2d+1)^2 uint8 planes: one K = 32 matrix block per tile from the words' bits, the
 * embedding's constant cells folded into a per-pixel bias (forward) / five shared gradient columns (backward).  Same function of the
 * same weights: Q-values and gradients agree with the uint8 path to f32 round-off (both meet the 1e-5 bound against the float64 oracle).
 * stride_words = words per observation row (a power of two, max(4, d * d) <= stride_words <= 64).  Fused chains only, d <= 7,
 * 4 * n_syndrome_planes + action planes <= 32 (DQ_ERR_UNSUPPORTED otherwise); n_syndrome_planes = 0 switches it off.  Call it BEFORE
 * dq_qnet_pack: the packed buffer carries the compact first kernel and the per-pixel bias.  Jobs select the form per launch
 * (dq_qnet_job.reserved bit 0); dq_qnet_forward always reads uint8 images.  No reference counterpart. */
dq_status dq_qnet_set_patch_input(dq_qnet* net, int n_syndrome_planes, int stride_words);

/* The fused chains read the conv kernels and Dense(512) as f16 pieces in matrix-core operand order.  A caller that runs several
 * forwards on the same weights packs them once per parameter change (dq_qnet_packed_bytes(net) bytes of device memory) and
 * passes the buffer in dq_qnet_job.packed_dev; it MUST repack after every change of params_dev (dq_adam_step, weight loading).
 * dq_qnet_forward and jobs with packed_dev == NULL pack on every call.  The backward reuses the training forward's pack.
 * packed_dev must be 16-byte aligned (it is written and read as 16-byte words): DQ_ERR_INVALID otherwise, from dq_qnet_pack and from a job that
 * brings it, before any launch. */
size_t dq_qnet_packed_bytes(const dq_qnet* net);
dq_status dq_qnet_pack(const dq_qnet* net, const float* params_dev, void* packed_dev, void* stream);

/* Backward half of train_on_batch: grads_dev[n_params] = d/dparams sum(dq * Q) for the last training forward
 * (obs_dev / index_dev of that call must still be valid).  Deterministic (fixed-order reductions). */
dq_status dq_qnet_backward(dq_qnet* net, const float* params_dev, const float* dq_dev, float* grads_dev, void* stream);

/* The fused backward carries its gradients multiplied by a power of two S (undone, exactly, by its final reduction) so that they sit in
 * the f16 pieces' range (csrc/fused_bwd.hip "gradient scale").  With the TD step fused in (dq_qnet_td_backward_*), S follows from
 * td->grad_scale.  A backward that is handed dq_dev measures max |dq| on the device first (one small extra launch) -- unless the caller
 * declares here the loss scale its dq was computed with (dq = TD error x grad_scale, as dq_td_update's argument): then the same S as in
 * the fused TD path is used, and the two paths give the same bits.  0 (default) = not declared.  No reference counterpart. */
dq_status dq_qnet_set_grad_scale(dq_qnet* net, double grad_scale);

/* A mark inside the NEXT fused backward of this network (dq_qnet_backward*, dq_qnet_td_backward*): `hip_event` (a hipEvent_t) is recorded on that
 * call's stream right behind the launch of the convolutional backward, i.e. in front of the final reduction / optimizer step and whatever the
 * caller launches next -- the point from which the device has idle capacity until the next forward (the reduction and the weight repacking are a
 * few hundred small workgroups).  A caller with independent work for another stream (the NEXT update's target-network forward: DQNCore's extra
 * updates of a vector step) makes that stream wait for the mark.  One-shot: consumed by one backward; NULL clears it.  Ignored (and cleared)
 * by backwards that do not run the fused convolutional kernel.  No reference counterpart. */
dq_status dq_qnet_mark_conv_backward(dq_qnet* net, void* hip_event);

/* Range guard of the fused backward.  Its gradients travel as f16 pieces (finite up to 65504 after the scale S above): a TD error so
 * large that some S x gradient leaves that range becomes inf / NaN in the weight gradient, where fp32 arithmetic (the reference's
 * TensorFlow) would still be finite.  That is never silent: the final reduction raises a device-side flag for every non-finite
 * gradient element and, when the optimizer step rides on it (dq_qnet_backward_adam, dq_qnet_td_backward_adam*), leaves that element's
 * parameter and moments untouched.  This call synchronises `stream`, returns DQ_ERR_RANGE if the flag was raised since the last call
 * and clears it; DQ_OK otherwise (always on the per-layer f32 path).  The agent loop calls it at its host synchronisation points.  With
 * S x grad_scale in [4, 8) the guard trips for |TD error| of a few thousand (the reference's recorded losses, trained_models/ * / * /
 * training_history.json, stay below 160, i.e. |TD error| ~ 20); with a finite dq_td_job.delta_clip the host picks S from the bound
 * |dq| <= delta_clip x grad_scale and no finite TD error trips it (a NaN one still does).  No reference counterpart. */
/* (round 6) The fused FORWARD is guarded too: its activations travel as f16 pieces as well, and one of 65504 or more would turn into inf, the products it enters
 * into NaN and the next ReLU into 0 -- finite, wrong Q-values.  Every layer's epilogue compares what it splits with the range, the packing launch checks every
 * parameter (finite, < 65504), the dense chain checks the Q-values it stores; any of them raises the same device-side flag and this call returns DQ_ERR_RANGE with
 * a message that starts "dq_qnet_range_check[forward]" (the agent loop treats that one as fatal: no gradient scale helps a diverged network). */
dq_status dq_qnet_range_check(dq_qnet* net, void* stream);
/* How many optimizer steps the guard's early half discarded WHOLE since the last call (the TD step saw a sample beyond the host-known scale's range: the
 * final reduction wrote NaN into every gradient element and moved no parameter -- with several ranks the all-reduce carries the NaNs to all of them and
 * dq_qnet_adam_step counts on each); synchronises `stream`, clears the count.  What the reference (fp32) would have applied and this path did not
 * (with a finite delta_clip only an update whose TD errors include a NaN): the agent loop logs it.  No reference counterpart. */
dq_status dq_qnet_range_discarded(dq_qnet* net, unsigned* count, void* stream);

/* The same backward in two phases, for overlapping the gradient all-reduce with compute on several GPUs (no reference
 * counterpart): phase 0 = dueling + dense layers -> grads_dev[dq_qnet_conv_param_count(net) ..) complete; phase 1 = the
 * convolutions -> grads_dev[0 .. dq_qnet_conv_param_count(net)).  Phase 0 must run first; dq_dev is only read by phase 0.  On the fused
 * chains phase 0 (and dq_qnet_td_backward_phase0[_env]) leaves grads_dev[0 .. dq_qnet_conv_param_count(net)) untouched. */
dq_status dq_qnet_backward_phase(dq_qnet* net, const float* params_dev, const float* dq_dev, float* grads_dev, int phase,
                                 void* stream);
size_t dq_qnet_conv_param_count(const dq_qnet* net);

/* dq_qnet_backward followed by dq_adam_step on the whole parameter vector, with the optimizer step applied by the backward's
 * final reduction launch (one launch fewer; same bits as the two separate calls).  Single-process training only: with several
 * ranks the gradient has to be all-reduced between the two.  grads_dev still receives the gradient. */
dq_status dq_qnet_backward_adam(dq_qnet* net, float* params_dev, const float* dq_dev, float* grads_dev, float* m_dev, float* v_dev,
                                double lr, double beta_1, double beta_2, double epsilon, uint64_t t, void* stream);

/* Episode records of a greedy evaluation -- keras-rl Agent.test's per-episode log (episode_reward, nb_steps, and the fork's
 * episode_lifetime; Single_Point_Training_Script.py:206-207) -- kept on the device, one call per vector step behind the environment
 * step: lattice i's running reward / length advance (not on a step spent being reset); a lattice that ends an episode while
 * quota_dev[i] > 0 appends int32 {step, i, reward bits (float), length, lifetime} to records_dev [capacity][5] (slot = atomic increment
 * of counter_dev[0]; sort by (step, lattice) for the serial loop's order) and pays one unit of quota.  The host only reads counter_dev
 * every few dozen steps to see whether the evaluation is complete.  A full table: a record whose slot is >= capacity is dropped -- nothing
 * is stored past row capacity - 1 --, its unit of quota is paid all the same and counter_dev[0] still counts it, so counter_dev[0] >
 * capacity tells the host how many records were lost.  quota_dev, ep_reward_dev, ep_len_dev int32 / float / int32 [n] and counter_dev int32
 * [1] are read and written; records_dev is only written.  No reference counterpart. */
dq_status dq_test_bookkeeping(const uint8_t* done_dev, const uint8_t* was_reset_dev, const float* reward_dev, const uint32_t* lifetime_dev, int n,
                              int step, int32_t* quota_dev, float* ep_reward_dev, int32_t* ep_len_dev, int32_t* records_dev, int capacity,
                              int32_t* counter_dev, void* stream);

/* dq_adam_step on the network's whole parameter vector, for the several-GPU branch (backward with m_dev == v_dev == NULL, all-reduce of
 * grads_dev, then this): an element whose all-reduced gradient is not finite -- the fused backward's range guard, on whichever rank it
 * tripped: the sum carries it to all of them -- is skipped AND raises this handle's range flag, so that dq_qnet_range_check reports
 * DQ_ERR_RANGE on every rank at the same synchronisation point and the replicas stay identical.  No reference counterpart. */
dq_status dq_qnet_adam_step(dq_qnet* net, float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, double lr, double beta_1,
                            double beta_2, double epsilon, uint64_t t, void* stream);

/* The learner half of one DQNAgent.backward in the fewest launches: dq_td_step (+ dq_episode_stats when n > 0) computed in the
 * dense backward's first kernel, then dq_qnet_backward, then dq_adam_step on the final reduction.  Same y / dq bits as the separate
 * calls; the loss / mean_q partials are summed in a different order (dq_td_metrics reads them the same way).  Gradient, parameters and
 * moments: the separate calls' bits on the per-layer path; on the fused chains the bits of every form of this launch (_adam, _adam_env,
 * _phase0[_env] + phase 1) are equal, and equal to the separate calls' to round-off only (with the TD step fused in, dq has one non-zero
 * per row and the backward forms dq W3^T as a scalar times a table row instead of on the matrix pipe).
 * y_dev, dq_dev (needed only by the per-layer path), metrics_dev nullable.
 * m_dev == v_dev == NULL (dq_qnet_td_backward_adam, _adam_env, dq_qnet_backward_adam): the gradient only, no optimizer step -- the several-GPU
 * path, where the all-reduce of grads_dev comes between the backward and dq_adam_step (one final reduction launch instead of the two of the
 * phase calls). */
typedef struct dq_td_job {
    const float* q_online_s1_dev;
    const float* q_target_s1_dev;
    const float* q_s0_dev;
    const float* reward_dev;        /* replay ring arrays, indexed through index_dev */
    const uint8_t* terminal_dev;
    const int32_t* action_dev;
    const int32_t* index_dev;
    double gamma, grad_scale;
    int batch, n_actions;
    float* y_dev;
    float* dq_dev;
    float* metrics_dev;
    const uint8_t* done_dev;        /* episode bookkeeping of the step just taken (dq_episode_stats arguments); n == 0: none */
    const uint8_t* was_reset_dev;
    const uint32_t* lifetime_dev;
    const float* step_reward_dev;
    int n;
    uint64_t* stats_dev;
    int auto_scale;                 /* fused backward with delta_clip = inf only.  0: its gradients are carried at the power-of-two scale that follows from
                                     * grad_scale (TD errors up to a few thousand; beyond: dq_qnet_range_check).  1: the scale is MEASURED -- max |TD error x
                                     * grad_scale| of this minibatch, by one small launch in front of the backward -- so that any finite TD error fp32 can hold is
                                     * carried, as in the reference's TensorFlow arithmetic (Single_Point_Training_Script.py:119-127).  Ignored with a finite
                                     * delta_clip: the bound on |dq| gives the scale */
    double delta_clip;              /* keras-rl DQNAgent(delta_clip): the Huber loss's delta (dq_td_loss_grad_clip's semantics).  0 (a zero-initialised job) or
                                     * +inf: none, the squared error -- the reference's setting, bit for bit as before this field existed; > 0: Huber, and the
                                     * fused backward's gradient scale S is the largest power of two that keeps both S x grad_scale < 8 and S x grad_scale x
                                     * delta_clip < 64 (no finite TD error can trip the range guard; delta_clip <= 8 keeps the unclipped S).  Negative or NaN:
                                     * DQ_ERR_INVALID.  Read as a float. */
} dq_td_job;
dq_status dq_qnet_td_backward_adam(dq_qnet* net, float* params_dev, const dq_td_job* td, float* grads_dev, float* m_dev, float* v_dev,
                                   double lr, double beta_1, double beta_2, double epsilon, uint64_t t, void* stream);
/* dq_env_act_step(_sample) of the SAME vector step riding on dq_qnet_td_backward_adam's first launch.  The update does not read what
 * the step writes (its minibatch never holds the newest transition, dq_replay_sample's rule) and the step does not read what the
 * update writes (it acts on q_dev, already computed), so the two are one launch: the lattices' blocks fill the idle issue slots of
 * the dense backward chain instead of taking a launch of their own.  The step's episode bookkeeping (dq_episode_stats' sums into
 * stats_dev, nullable) is done by the lattices' blocks themselves; td->n must be 0.  Same bits as the separate calls.  Fused chains
 * only (DQ_ERR_UNSUPPORTED otherwise: make the separate calls).  Replaces, per vector step of the reference's loop,
 * `action = policy.select_action(q)`, `env.step(action)`, `memory.append` and `DQNAgent.backward`
 * (cluster_scripts/d5_dp/0.001/Single_Point_Training_Script.py:138-152 -> keras-rl Agent.fit). */
typedef struct dq_env_step_job {
    const float* q_dev;             /* dq_env_act_step's arguments */
    double eps;
    int masked_greedy;
    uint32_t seed[2];
    uint64_t t;
    int32_t* action_dev;
    int auto_reset;
    uint8_t* obs_dev;
    float* reward_dev;
    uint8_t* done_dev;
    uint64_t* legal_dev;
    uint32_t* lifetime_dev;
    uint8_t* was_reset_dev;
    const dq_sample_job* sample;    /* nullable: dq_env_act_step_sample's look-ahead draw */
    uint64_t* stats_dev;            /* nullable: uint64 [4] accumulators of dq_episode_stats */
} dq_env_step_job;
dq_status dq_qnet_td_backward_adam_env(dq_qnet* net, float* params_dev, const dq_td_job* td, float* grads_dev, float* m_dev, float* v_dev,
                                       double lr, double beta_1, double beta_2, double epsilon, uint64_t t, dq_env* env,
                                       const dq_env_step_job* step, void* stream);
/* The several-GPU form: the TD step + phase 0 of dq_qnet_backward_phase (dueling + dense layers) in one call; phase 1, the gradient
 * all-reduce and dq_adam_step follow as separate calls. */
dq_status dq_qnet_td_backward_phase0(dq_qnet* net, const float* params_dev, const dq_td_job* td, float* grads_dev, void* stream);
/* ... with the vector step's environment launch riding on it (as dq_qnet_td_backward_adam_env). */
dq_status dq_qnet_td_backward_phase0_env(dq_qnet* net, const float* params_dev, const dq_td_job* td, float* grads_dev, dq_env* env,
                                         const dq_env_step_job* step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DQN update: replaces SequentialMemory.sample + DQNAgent.backward + keras Adam of the keras-rl fork
 * (Single_Point_Training_Script.py:109,119-130).
 * Device replay ring: row r = slot*n_envs + env stores (observation, action, reward, terminal) of the
 * step taken from that observation; its successor observation is row r + n_envs (mod n_slots*n_envs).
 * ------------------------------------------------------------------------------------------- */
/* Uniform minibatch rows over exactly the transitions upstream keras-rl 0.4.2 SequentialMemory.sample can return
 * (oracle/memory_oracle.py): idx = sample_batch_indexes(window_length, nb_entries - 1) + 1 and the transition used is idx - 1, i.e.
 * every stored transition except the newest (its successor observation is not in keras-rl's memory yet) and entry 0, redrawing those
 * whose predecessor entry was terminal (terminals[idx - 2]).  head_slot = slot of the newest observation, filled_slots = slots written
 * so far (4 <= filled_slots <= n_slots; nb_entries = filled_slots - 1).
 * As in keras-rl (random.sample, Single_Point_Training_Script.py:109 -> SequentialMemory.sample), the FIRST draws of a minibatch are
 * WITHOUT replacement whenever the M = (filled_slots - 3) * n_envs candidate rows are at least `batch`: sample b takes candidate
 * pi_t((sample_base + b) mod M), pi_t a keyed bijection of [0, M) (four-round Feistel network + cycle walking; round keys =
 * Philox(key=seed, ctr=(t_lo, t_hi, 0xffffffff, 0xffff | DQ_STREAM_REPLAY<<16)); csrc/common.h dq_replay_permute); candidate
 * c = slot head_slot - 2 - c / n_envs, lattice c mod n_envs.  A redraw (attempt >= 1) -- and every draw when batch > M, keras-rl's
 * with-replacement fallback -- is independent: Philox(key=seed, ctr=(t_lo, t_hi, sample_base + b, attempt | DQ_STREAM_REPLAY<<16)),
 * slot = head_slot - 2 - ((w0 * (filled_slots - 3)) >> 32), env = (w1 * n_envs) >> 32.  Terminal flags are read no newer than slot
 * head_slot - 3, so an update's minibatch may be drawn one vector step early (with the head_slot / filled_slots it WILL have). */
dq_status dq_replay_sample(const uint8_t* terminal_ring_dev, int n_envs, int n_slots, int head_slot, int filled_slots,
                           int batch, const uint32_t seed[2], uint64_t t, uint32_t sample_base, int32_t* index_dev,
                           void* stream);

/* The same for n_updates consecutive updates t0, t0 + 1, ... drawn on ONE ring state, in one launch: index_dev int32 [n_updates][batch], row u = what
 * dq_replay_sample gives for t = t0 + u.  (The reference trains one minibatch per environment step, Single_Point_Training_Script.py:119-127; with N
 * lattices per vector step that is several updates per step on the same memory -- their draws do not depend on each other.) */
dq_status dq_replay_sample_multi(const uint8_t* terminal_ring_dev, int n_envs, int n_slots, int head_slot, int filled_slots,
                                 int batch, const uint32_t seed[2], uint64_t t0, int n_updates, uint32_t sample_base,
                                 int32_t* index_dev, void* stream);

/* Double-DQN target: y_b = reward[r_b] + gamma * (1 - terminal[r_b]) * Q_target(s1_b)[argmax_a Q_online(s1_b)[a]],
 * r_b = index_dev ? index_dev[b] : b. */
dq_status dq_td_target(const float* q_online_s1_dev, const float* q_target_s1_dev, const float* reward_dev,
                       const uint8_t* terminal_dev, const int32_t* index_dev, double gamma, int batch, int n_actions,
                       float* y_dev, void* stream);

/* keras-rl clipped_masked_error with delta_clip = inf:  loss = mean_b 0.5 (Q[b,a_b] - y_b)^2.
 *   dq_dev      float [batch, n_actions] = grad_scale * (Q[b,a_b] - y_b) at a_b, 0 elsewhere
 *               (grad_scale = 1 / global batch, so an all-reduce SUM of gradients gives the global mean);
 *   metrics_dev float [DQ_TD_METRICS_FLOATS] (nullable): [0] = loss, [1] = mean_q = mean_b max_a Q[b,a] of this
 *               rank's minibatch; the rest is scratch for the fixed-order two-stage reduction. */
#define DQ_TD_METRICS_FLOATS 2050
dq_status dq_td_loss_grad(const float* q_s0_dev, const int32_t* action_dev, const int32_t* index_dev, const float* y_dev,
                          int batch, int n_actions, double grad_scale, float* dq_dev, float* metrics_dev, void* stream);
/* The same with keras-rl's finite delta_clip (huber_loss / clipped_masked_error of keras-rl 0.4.2), fp32, delta = (float)delta_clip,
 * x_b = Q[b,a_b] - y_b:
 *   loss        mean_b h(x_b),  h(x) = 0.5 x^2 if |x| <= delta, else delta (|x| - 0.5 delta)
 *   dq_dev      grad_scale * c(x_b) at a_b, 0 elsewhere,  c(x) = |x| > delta ? copysign(delta, x) : x
 * The clamp is that compare: a NaN TD error stays NaN (as in TensorFlow; the fused backward's range guard sees it), an infinite one
 * gives +-delta.  delta_clip = +inf is dq_td_loss_grad, bit for bit; delta_clip <= 0 or NaN: DQ_ERR_INVALID (keras-rl asserts > 0). */
dq_status dq_td_loss_grad_clip(const float* q_s0_dev, const int32_t* action_dev, const int32_t* index_dev, const float* y_dev,
                               int batch, int n_actions, double grad_scale, double delta_clip, float* dq_dev, float* metrics_dev,
                               void* stream);

/* dq_td_target + dq_td_loss_grad in one launch (same arithmetic, same per-block metric partials), WITHOUT the final metric
 * reduction: call dq_td_metrics(metrics_dev, batch) before reading metrics_dev[0..1] (the training loop only reads them at its
 * logging interval).  y_dev nullable. */
dq_status dq_td_update(const float* q_online_s1_dev, const float* q_target_s1_dev, const float* q_s0_dev, const float* reward_dev,
                       const uint8_t* terminal_dev, const int32_t* action_dev, const int32_t* index_dev, double gamma, int batch,
                       int n_actions, double grad_scale, float* y_dev, float* dq_dev, float* metrics_dev, void* stream);
/* dq_td_update plus dq_episode_stats of the environment step just taken, in one launch. */
dq_status dq_td_update_stats(const float* q_online_s1_dev, const float* q_target_s1_dev, const float* q_s0_dev, const float* reward_dev,
                             const uint8_t* terminal_dev, const int32_t* action_dev, const int32_t* index_dev, double gamma, int batch,
                             int n_actions, double grad_scale, float* y_dev, float* dq_dev, float* metrics_dev, const uint8_t* done_dev,
                             const uint8_t* was_reset_dev, const uint32_t* lifetime_dev, const float* step_reward_dev, int n,
                             uint64_t* stats_dev, void* stream);
/* dq_td_update (td->n == 0) or dq_td_update_stats (td->n > 0) driven by a dq_td_job, with its delta_clip (dq_td_loss_grad_clip's
 * semantics; 0 / +inf: the squared error, the bits of those calls).  auto_scale is not read.  The per-layer path of the
 * dq_qnet_td_backward_* calls runs this. */
dq_status dq_td_step(const dq_td_job* td, void* stream);
dq_status dq_td_metrics(float* metrics_dev, int batch, void* stream);

/* dq_replay_sample (for the next update) + dq_episode_stats (of the step just taken) in one launch. */
dq_status dq_post_step(const uint8_t* terminal_ring_dev, int n_envs, int n_slots, int head_slot, int filled_slots, int batch,
                       const uint32_t seed[2], uint64_t t, uint32_t sample_base, int32_t* index_dev, const uint8_t* done_dev,
                       const uint8_t* was_reset_dev, const uint32_t* lifetime_dev, const float* reward_dev, int n, uint64_t* stats_dev,
                       void* stream);

/* Episode bookkeeping the keras-rl fork does on the host per step (episode ends, env.lifetime of finished
 * episodes -- Single_Point_Training_Script.py:207 reads their rolling average): accumulates into uint64 stats_dev[4]
 * = {episodes ended, sum of their lifetimes, rewards earned, lattices stepped}.  was_reset_dev nullable. */
dq_status dq_episode_stats(const uint8_t* done_dev, const uint8_t* was_reset_dev, const uint32_t* lifetime_dev,
                           const float* reward_dev, int n, uint64_t* stats_dev, void* stream);

/* keras.optimizers.Adam (Keras 2.2): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMAs; p -= lr_t*m/(sqrt(v)+epsilon).
 * t = 1 for the first update. */
/* (Keras' update as it is: a non-finite gradient element propagates into its parameter and moments -- a diverged run stays visible.  The guarded
 * form -- such elements skipped and flagged -- is dq_qnet_adam_step and the optimizer step riding on the fused backward.) */
dq_status dq_adam_step(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, size_t n, double lr,
                       double beta_1, double beta_2, double epsilon, uint64_t t, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched decoding: replaces the reference's "Using a Trained Decoder in Production" loop (README.md:786-829, notebook 3 section 3b),
 * which calls dqn.forward(input_state) once per action of one volume.  Here n volumes are decoded together on the device.
 *
 * Input: syndromes_dev uint8 [n][volume_depth][d+1][d+1] (4-byte aligned), the faulty syndrome slices of each volume on the reference's
 * (d+1) x (d+1) grid, cells 0 or 1 (the binding rejects other values; the kernels read any nonzero cell as 1).  Cells are copied into the
 * observation exactly as padding_syndrome does (Environments.py:273-299), dead corners included.
 * Per volume, starting with empty action planes and legal set = reset_legal_moves of the summed volume (Environments.py:238-258):
 *   1. observation = the padded slices + the action planes;  2. Q = the network's forward with params_dev;
 *   3. a = first maximum of Q (policy_kernel's rule with eps = 0), over the legal set when cfg.masked_greedy != 0;
 *   4. stop if a is the identity (status DQ_DECODE_IDENTITY) or already completed (DQ_DECODE_REPEAT: Environments.py:131 treats a repeat as
 *      the identity); the stopping action is not recorded;
 *   5. otherwise record a, mark completed_actions[a], add the neighbours x layers of a newly acted-on qubit to the legal set
 *      (Environments.py:186-196), set the action-plane cell; after cfg.max_actions recorded actions stop (DQ_DECODE_STOPPED).
 * That is the sequence of actions a greedy agent takes in the environment on that volume up to its first identity.
 * Action planes: DQ_DECODE_PLANES_ENV marks qubit q of layer l for action l d^2 + q (Environments.py:199-201).  DQ_DECODE_PLANES_README
 * (X model only: one action layer) reproduces README.md:807 statement for statement: `padding_actions(corrections)` with the LIST of action
 * indices, i.e. qubit i is marked iff corrections[i] != 0.
 * Outputs: corrections_dev int32 [n][max_actions] in the order chosen, padded with -1; n_corr_dev int32 [n]; frame_dev uint8 [n][d][d] the
 * net Pauli frame of the recorded corrections as hidden_state codes 0..3 (XOR of index_to_move over them, env.hip's layer -> Pauli map);
 * status_dev uint8 [n].
 * The network: cfg.obs_form DQ_DECODE_OBS_PATCH reads patch words (dq_env_patch_output's layout; needs dq_qnet_set_patch_input(net,
 * volume_depth, stride)), DQ_DECODE_OBS_UINT8 padded uint8 images.  packed_dev: dq_qnet_pack(params_dev) output for this network (NULL:
 * every iteration packs).  n <= min(max_volumes, the network's max_batch).  Lattices: d <= 7 and num_actions <= 128 (DQ_ERR_UNSUPPORTED).
 * Per iteration: one dq_qnet_forward_multi over the volumes still decoding (index gather over the active list), one selection launch and
 * one stable compaction launch; the host then reads the 4-byte active count to size the next launches.  That read is the loop's one host
 * wait, so dq_decode_run SYNCHRONISES `stream` once per iteration (at most max_actions iterations; *iterations receives the number) and is
 * not hipGraph-capturable.  At the end it runs dq_qnet_range_check(net): a forward that met a non-finite value returns DQ_ERR_RANGE
 * ("dq_qnet_range_check[forward]") and its outputs are not to be used.  No reference counterpart beyond the loop above. */
typedef struct dq_decode dq_decode;
enum { DQ_DECODE_ACTIVE = 0, DQ_DECODE_IDENTITY = 1, DQ_DECODE_REPEAT = 2, DQ_DECODE_STOPPED = 3 };
enum { DQ_DECODE_PLANES_ENV = 0, DQ_DECODE_PLANES_README = 1 };
enum { DQ_DECODE_OBS_UINT8 = 0, DQ_DECODE_OBS_PATCH = 1 };
typedef struct {
    int32_t d;              /* 3, 5 or 7 (dq_decode_wide_create: odd, 3 .. 15) */
    int32_t volume_depth;   /* 1..16 */
    int32_t error_model;    /* DQ_MODEL_* */
    int32_t use_Y;
    int32_t masked_greedy;  /* 0: plain argmax (notebook 3b's dqn.forward), 1: argmax over the legal set (test()'s GreedyQPolicy(masked_greedy=True)) */
    int32_t max_actions;    /* 1 .. num_actions - 1 */
    int32_t action_planes;  /* DQ_DECODE_PLANES_ENV / DQ_DECODE_PLANES_README */
    int32_t obs_form;       /* DQ_DECODE_OBS_UINT8 / DQ_DECODE_OBS_PATCH */
} dq_decode_cfg;
/* Owns the per-volume state, observation rows, Q rows and active lists for up to max_volumes volumes. */
dq_status dq_decode_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode** out);
void dq_decode_destroy(dq_decode* dec);
dq_status dq_decode_run(dq_decode* dec, dq_qnet* net, const float* params_dev, const void* packed_dev, const uint8_t* syndromes_dev, int n,
                        int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev, uint8_t* status_dev, int* iterations, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring batched decoding: sample -> dq_decode_run -> verdict -> counts, all on the device (csrc/decode_eval.hip).  The figure it serves is the
 * logical failure probability of decoding ONE volume of volume_depth faulty rounds; the reference only reports mean episode lifetimes.
 *
 * dq_decode_sample: n independent memory experiments from a clean lattice.  Volume i runs volume_depth rounds, each one generate_error
 * (Function_Library.py:67-122 / 134-160) followed by one generate_faulty_syndrome (Function_Library.py:176-223) -- the round of
 * Environments.py:160-170 -- WITHOUT the redraw of all-zero volumes (Environments.py:171).  Random numbers: the environment's Philox convention,
 * key = seed, lattice id = env_id_base + i (mod 2^32), round counter 0 .. volume_depth - 1, lane = site.  Volume i is therefore the first
 * volume_depth rounds of lattice env_id_base + i, and where those are not all zero it is what dq_env_reset produces for that lattice.
 * Rates: p_phys_each / p_meas_each NULL: the scalar pair for every volume; else HOST arrays of n rates, volume i runs at entry i (thresholds as
 * dq_env_set_rates_per_lattice computes them; read before the call returns, uploaded by one copy ordered on `stream`).
 * `env` supplies the lattice (its tables are read in place; its own lattices, rates and seed are not touched) and must be the lattice the handle
 * was created for.  Outputs: volumes_dev uint8 [n][volume_depth][d+1][d+1] (dq_decode_run's input, 4-byte aligned), hidden_dev uint8 [n][d][d]
 * the accumulated error as hidden_state codes 0..3, trivial_dev uint8 [n]: 1 where the whole volume is zero.
 *
 * dq_decode_verdict: per volume the residual error = hidden XOR frame (Pauli components XOR: obtain_new_error_configuration,
 * Function_Library.py:226-241; frame_dev NULL = no correction), then what step() decides on that hidden state (Environments.py:139-151):
 * true = perfect syndrome of the residual, correct = its homology class, decoded = the class the referee INSTALLED ON `env` assigns to true --
 * every referee kind of the handle is honoured with the step's precedence (Dense stack, joint table, component tables), read in place.
 * verdict_dev uint8 [n]: DQ_VERDICT_IN_CODESPACE (true == 0) | correct << DQ_VERDICT_CLASS_SHIFT | DQ_VERDICT_SUCCESS (correct == 0 and
 * true == 0: the step's reward 1) | DQ_VERDICT_ALIVE (success or decoded == correct: the step's done == False) | decoded << DQ_VERDICT_DECODED_SHIFT.
 * dq_decode_run does not record its stopping action, but the environment APPLIES a repeated action before it tests for the repeat
 * (Environments.py:135-136 against :131): the verdict is what the environment returned on the stopping step for volumes of status
 * DQ_DECODE_IDENTITY only.
 *
 * dq_decode_count: adds the flags of n volumes to DQ_EVAL_COUNTERS uint64 counters per contiguous block of `block` volumes: volume i counts into
 * counters_dev[((first + i) / block) * DQ_EVAL_COUNTERS + DQ_EVAL_*] (`first`: the global index of volume 0, so that a chunked caller keeps one
 * table; n_blocks: rows of the table).  trivial_dev / status_dev / n_corr_dev may be NULL (their counters stay).  The caller zeroes the table.
 * No reference counterpart. */
typedef struct dq_decode_eval dq_decode_eval;
enum { DQ_VERDICT_IN_CODESPACE = 1, DQ_VERDICT_CLASS_SHIFT = 1, DQ_VERDICT_SUCCESS = 8, DQ_VERDICT_ALIVE = 16, DQ_VERDICT_DECODED_SHIFT = 5 };
enum { DQ_EVAL_VOLUMES = 0, DQ_EVAL_TRIVIAL, DQ_EVAL_IN_CODESPACE, DQ_EVAL_SUCCESS, DQ_EVAL_ALIVE, DQ_EVAL_IDENTITY, DQ_EVAL_REPEAT, DQ_EVAL_STOPPED,
       DQ_EVAL_CORRECTIONS, DQ_EVAL_COUNTERS };
/* Owns the per-volume threshold table and the Dense-stack referee's scratch for up to max_volumes volumes; of cfg the lattice (d, volume_depth,
 * error_model, use_Y) is read: the same limits as dq_decode_create (DQ_ERR_UNSUPPORTED beyond d = 7 / 128 actions). */
dq_status dq_decode_eval_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode_eval** out);
void dq_decode_eval_destroy(dq_decode_eval* ev);
dq_status dq_decode_sample(dq_decode_eval* ev, const dq_env* env, int n, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                           const double* p_phys_each, const double* p_meas_each, uint8_t* volumes_dev, uint8_t* hidden_dev, uint8_t* trivial_dev,
                           void* stream);
dq_status dq_decode_verdict(dq_decode_eval* ev, dq_env* env, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev,
                            void* stream);
dq_status dq_decode_count(const uint8_t* verdict_dev, const uint8_t* trivial_dev, const uint8_t* status_dev, const int32_t* n_corr_dev, int n,
                          int64_t first, int block, int n_blocks, uint64_t* counters_dev, void* stream);
/* dq_decode_match: the space-time minimum-weight matching baseline (csrc/match_st.hip) on n <= max_volumes volumes in
 * dq_decode_run's input layout.  Per Pauli component (0: type-3 plaquettes / X errors, 1: type-1 / Z errors) the defects are S_t xor S_{t-1}
 * (S_-1 = 0); unit-weight edges: a data error joins its plaquettes of the round (or the spatial boundary), a measurement error joins (s, t) and
 * (s, t + 1), in the last round (s, depth - 1) and the open future boundary.  One matching of minimum total weight over both logical classes is
 * returned: frame_dev uint8 [n][d][d] the XOR of its paths' spatial projections as hidden_state codes (what dq_decode_verdict takes),
 * weight_dev int32 [n][2] its weight per component, n_defects_dev int32 [n][2], inexact_dev uint8 [n]: 1 where a cluster of more than 14 defects
 * or defects beyond the first 32 of a component took the nearest-boundary fallback.  weight_dev / n_defects_dev / inexact_dev may be NULL.
 * Deterministic per volume: no dependence on the batch.  The tables are built at the handle's first call, which therefore MODIFIES the handle: like
 * every call on a dq_decode_eval this one is not thread-safe (one thread at a time per handle, and the first calls of a process serialised).  No reference counterpart (README.md:278
 * names MWPM as the benchmark). */
dq_status dq_decode_match(dq_decode_eval* ev, const uint8_t* volumes_dev, int n, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                          uint8_t* inexact_dev, void* stream);
/* dq_env_match_select: the matching decoder as a policy of the narrow environment (csrc/env_match.hip; dq_version() >= 7).  For
 * every lattice of `env`: F = the frame dq_decode_match returns for the lattice's current faulty volume (the record's volume_depth syndrome words,
 * S_-1 = 0, so residual error of earlier volumes shows up as round-0 defects); wanted = the action indices whose moves XOR to F (X model: component 0
 * on the one layer, component 1 is ignored; DP / IIDXZ with use_Y: code 1 / 2 / 3 -> layer 0 / 1 / 2; without: X part -> layer 0, Z part -> layer 1,
 * a Y cell being both); action_dev[i] = the lowest wanted index not in completed_actions, else the identity; a lattice whose done flag is set gets the
 * identity.  inexact_dev (nullable) uint8 [n_envs]: dq_decode_match's flag for the volume (0 for a done lattice).  A function of the lattice's state
 * alone: nothing is kept between calls and the environment is not modified.  An agent step is this launch followed by
 * dq_env_step(action_dev, auto_reset = 1); the legal set is not consulted (the step applies any action, Environments.py:131-136).  ev must have
 * been created for the environment's d, error model, use_Y (X model: ignored) and volume_depth (DQ_ERR_INVALID otherwise); its matching tables are
 * built at the first call of this or of dq_decode_match (the same thread rule).  One wavefront per lattice; action_dev int32 [n_envs]. */
dq_status dq_env_match_select(dq_env* env, dq_decode_eval* ev, int32_t* action_dev, uint8_t* inexact_dev, void* stream);
/* dq_env_guided_select: epsilon-greedy selection whose exploring lattices follow the matching decoder with probability guide_share (csrc/env_guide.hip;
 * DESIGN.md section 15; dq_version() >= 8).  For lattice i, with w[0..3] the Philox words dq_policy_select draws for (seed, t, the environment's
 * env_id_base + i, DQ_STREAM_POLICY) and T the threshold both rates go through (W / 2^32 < p  <=>  W < ceil(p 2^32)):
 *   explore = q_dev == NULL || w[1] < T(eps);      guided = explore && w[2] < T(guide_share)
 *   guided:        action_dev[i] = what dq_env_match_select writes for the lattice as it stands (the identity for a lattice whose done flag is set; the legal
 *                  set is not consulted)
 *   else explore:  the k-th legal action, k = (w[0] * n_legal) >> 32                                     (dq_policy_select's rule)
 *   else:          the first maximum of row i of q_dev float [n_envs][num_actions], over the legal set when masked_greedy  (dq_policy_select's rule)
 * The legal set is the one the lattice's record holds (what the last dq_env_reset / dq_env_step also wrote to its legal_dev).  guide_share = 0: the actions
 * of dq_policy_select bit for bit; eps = 1 (or q_dev NULL) with guide_share = 1: those of dq_env_match_select.  guided_dev (nullable) uint8 [n_envs]: 1
 * where the lattice followed the matching; inexact_dev (nullable) uint8 [n_envs]: dq_env_match_select's flag for a guided lattice, 0 for every other.  The
 * matching runs only in the wavefronts of guided lattices.  eps and guide_share must lie in [0, 1] (DQ_ERR_INVALID); ev as for dq_env_match_select (same
 * checks, tables and thread rule); the narrow environment, d <= 7, volume_depth <= 16.  Nothing is kept between calls and the environment is not
 * modified: an agent step is this launch followed by dq_env_step(action_dev, auto_reset = 1).  No reference counterpart. */
dq_status dq_env_guided_select(dq_env* env, dq_decode_eval* ev, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                               uint64_t t, int32_t* action_dev, uint8_t* guided_dev, uint8_t* inexact_dev, void* stream);
/* The union-find decoder (Delfosse and Nickerson; csrc/uf_dev.h, csrc/uf_st.hip): the second baseline and a teacher without a
 * cluster-size limit.  dq_version() stays 8: the capability is discovered by the presence of these three symbols.  Per Pauli component, on
 * dq_decode_match's defects and unit-weight graph with the spatial and the open future boundary merged into one boundary node: clusters grow in
 * synchronous half-edge rounds until each holds an even number of defects or the boundary, then a breadth-first forest over the full edges is peeled.
 * There is no fallback: nothing is inexact.
 * dq_decode_uf: dq_decode_match's contract (n <= max_volumes volumes in dq_decode_run's input layout, frame_dev uint8 [n][d][d] as hidden_state codes,
 * weight_dev int32 [n][2] = edges of the correction per component, time edges and the edge to the future boundary included, n_defects_dev int32 [n][2]) with
 * rounds_dev int32 [n][2] = growth rounds per component in place of inexact_dev; weight_dev / n_defects_dev / rounds_dev may be NULL.  Deterministic per
 * volume: no dependence on the batch.
 * dq_env_uf_select: dq_env_match_select with F = dq_decode_uf's frame of the lattice's current volume (no flag output).
 * dq_env_guided_select_uf: dq_env_guided_select whose guided lattices get dq_env_uf_select's action; inexact_dev, if given, is zero-filled.
 * All three make dq_decode_match's / dq_env_match_select's checks of the lattice and the evaluator and return the same error codes (d <= 7,
 * volume_depth <= 16, the narrow environment; an evaluator of another lattice: DQ_ERR_INVALID).  The endpoint tables live in the handle's table blob beside the
 * matching's, built at the handle's first call of any of the six entry points, which therefore MODIFIES the handle: a dq_decode_eval serves one host
 * thread at a time and the calls on it are ordered on one stream at a time; it is not thread-safe. */
dq_status dq_decode_uf(dq_decode_eval* ev, const uint8_t* volumes_dev, int n, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                       int32_t* rounds_dev, void* stream);
dq_status dq_env_uf_select(dq_env* env, dq_decode_eval* ev, int32_t* action_dev, void* stream);
dq_status dq_env_guided_select_uf(dq_env* env, dq_decode_eval* ev, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                                  uint64_t t, int32_t* action_dev, uint8_t* guided_dev, uint8_t* inexact_dev, void* stream);
/* Sliding-window union-find decoding of syndrome streams of any length (csrc/uf_stream.hip).  dq_version() stays 8: the capability is
 * the presence of these two symbols.  Union-find only: the matching's tabulated paths do not say which part of a correction lies in the committed rounds.
 * A stream is T rounds of faulty syndromes of one lattice, 1 <= T <= 2^20, with the defects D_t = S_t xor S_{t-1} (S_-1 = 0).  The window w is the handle's
 * volume_depth, the commit c lies in 1 .. w.  Window k starts at round a = k c, is final iff a + w >= T and has l = T - a rounds when final, else w; its
 * defect rows are D_a xor carry, D_{a+1} .. D_{a+l-1} (carry: empty at the start) and it is decoded by dq_decode_uf's algorithm, unchanged, on the depth-l
 * graph.  With t = e / (d^2 + n) the round of an edge of the correction: the final window commits every edge and carries nothing; any other window commits
 * the edges with t < c, and the next carry is the set of u whose time edge of round c - 1 is in the correction.  A committed space edge XORs its qubit
 * into the frame, every committed edge adds 1 to the weight.  A function of the stream alone: one window (w >= T) is dq_decode_uf at depth T in every field.
 * dq_stream_decode_uf: syndromes_dev uint8 [n][T][d+1][d+1] with 0/1 cells; frame_dev uint8 [n][d][d] as hidden_state codes; weight_dev / n_defects_dev /
 * rounds_dev int32 [n][2], nullable, 4-byte aligned: committed edges, the stream's own defects (carries not counted), growth rounds summed over the windows.
 * dq_stream_run_uf: the same schedule on rounds drawn in the kernel, so that the syndromes never reach memory: stream i is the first T rounds of lattice
 * env_id_base + i under dq_decode_sample's convention (the same key, round counter, thresholds and per-stream rate arrays; for T <= 16 its syndromes are
 * dq_decode_sample's).  hidden_dev uint8 [n][d][d] and trivial_dev uint8 [n] as dq_decode_sample writes them; weight_dev, n_defects_dev, rounds_dev and
 * syndromes_dev (uint8 [n][T][d+1][d+1]) may be NULL.  `env` supplies the lattice tables and must be of the handle's d, error model and use_Y; its
 * volume_depth is not consulted (dq_decode_verdict's check).
 * Both: n in 1 .. max_volumes, T in 1 .. 2^20, commit in 1 .. volume_depth (DQ_ERR_INVALID); d <= 7, volume_depth <= 16 (DQ_ERR_UNSUPPORTED).  One
 * wavefront per stream.  The endpoint tables are dq_decode_uf's, built at the handle's first call, which therefore MODIFIES the handle: a dq_decode_eval
 * serves one host thread at a time and the calls on it are ordered on one stream at a time; it is not thread-safe.  No reference counterpart. */
dq_status dq_stream_decode_uf(dq_decode_eval* ev, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                              int32_t* n_defects_dev, int32_t* rounds_dev, void* stream);
dq_status dq_stream_run_uf(dq_decode_eval* ev, const dq_env* env, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys,
                           double p_meas, const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                           int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);

/* Streams closed by a final round of perfect measurements, as a memory experiment that ends on a data-qubit readout gives them.
 * dq_version() stays 8: the capability is the presence of these four symbols.  The argument lists, the validation, the error codes, the nullable arrays
 * and the one-host-thread, one-stream contract are those of the entry points without the suffix; so are all results but for this rule:
 * decode: in the final window (the one with a + window >= T, of depth l) the time edges of round l - 1, (u, l - 1) -- B, do not exist: they are never grown,
 *   never full and never in the correction.  Edge ids, node ids, the schedule, the commit filter, the carry, the growth rule, the min-labels and the
 *   lowest-edge-id peeling are unchanged, and so is every window but the final one.  Per component the committed frame's syndrome then equals the stream's
 *   last syndrome; with T = 1 the decode is code-capacity union-find on the 2-D graph.  Defined for any input stream.
 * run: the same Philox words for every round j = 0 .. T - 1; in round T - 1 the measurement flip (word 2) is not applied, the data errors land as always.
 *   hidden equals the open run's for the same seed and ids, the syndromes of rounds 0 .. T - 2 too; round T - 1 is the true syndrome, and trivial is
 *   computed from the syndromes as drawn.  The residual of a closed run is therefore always in the code space. */
dq_status dq_stream_decode_uf_closed(dq_decode_eval* ev, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                                     int32_t* n_defects_dev, int32_t* rounds_dev, void* stream);
dq_status dq_stream_run_uf_closed(dq_decode_eval* ev, const dq_env* env, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys,
                                  double p_meas, const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev,
                                  uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);

/* Union-find stream decoding for any odd d in 3 .. 15 with a window of up to 32 rounds (csrc/uf_wide.hip).  dq_version() stays 8: the
 * capability is the presence of these symbols.  The algorithm and the schedule are dq_stream_decode_uf's, word for word (for d <= 7 and window <= 16 every
 * field equals its); what differs is the shape: one workgroup of 256 threads per stream, defect rows and carries of 4 x 32 bits, frames of 4 x 64 bits, and
 * dynamic LDS sized from (d, window) -- at most 64 KiB at d = 15, window 32.  The handle owns the lattice tables (built on the host from d alone): no
 * environment handle is needed, and no referee is consulted.
 * dq_wide_uf_create: d odd in 3 .. 15, error_model a DQ_MODEL_*, window in 1 .. 32, max_streams >= 1 (else DQ_ERR_INVALID, before any device work); an LDS
 * request the device refuses is DQ_ERR_UNSUPPORTED (the kernels' limit is set once per device to the largest shape's, so handles of different shapes live
 * side by side); the table of per-stream rates is allocated for max_streams here (DQ_ERR_NOMEM), so a handle serves any n up to max_streams in any order.
 * dq_wide_uf_decode: dq_stream_decode_uf's arguments and results (syndromes_dev uint8 [n][T][d+1][d+1], 0/1 cells; weight_dev / n_defects_dev / rounds_dev
 * int32 [n][2], nullable, 4-byte aligned).
 * dq_wide_uf_run: dq_stream_run_uf's arguments and results without the environment: stream i is the first T rounds of lattice env_id_base + i under
 * dq_decode_sample's convention -- Philox4x32-10 under `seed` with the counter (round, 0, lattice id, q); for qubit q < d^2 word 0 below the physical
 * threshold is a hit, word 1 gives the Pauli type (DP) or an independent Z flip (IIDXZ); for q < d^2 - 1 word 2 below the measurement threshold flips
 * stabilizer q's measurement.  weight_dev, n_defects_dev, rounds_dev and syndromes_dev may be NULL; the rate arrays come as a pair or not at all.
 * dq_wide_uf_verdict: residual = hidden XOR frame (frame_dev NULL: no correction); the byte is dq_decode_verdict's with no referee: DQ_VERDICT_IN_CODESPACE,
 * the class field (X parity on column 0, + 2 x Z parity on row 0), DQ_VERDICT_SUCCESS = in code space and class 0, DQ_VERDICT_ALIVE := DQ_VERDICT_SUCCESS,
 * decoded field 0.  dq_decode_count sums these bytes as they stand; its "alive" counter then equals "success" by construction and says nothing more.
 * All: n in 1 .. max_streams, T in 1 .. 2^20, commit in 1 .. window; null handles and bad arguments are DQ_ERR_INVALID before any device work.  A
 * dq_wide_uf serves one host thread at a time and its calls are ordered on one stream at a time (dq_wide_uf_run's rate arrays go through a staging buffer
 * of the handle); it is not thread-safe.  No reference counterpart. */
typedef struct dq_wide_uf dq_wide_uf;
dq_status dq_wide_uf_create(int d, int error_model, int window, int max_streams, dq_wide_uf** out);
void dq_wide_uf_destroy(dq_wide_uf* h);
dq_status dq_wide_uf_decode(dq_wide_uf* h, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                            int32_t* n_defects_dev, int32_t* rounds_dev, void* stream);
dq_status dq_wide_uf_run(dq_wide_uf* h, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                         const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                         int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);
dq_status dq_wide_uf_verdict(dq_wide_uf* h, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, void* stream);
/* The refereed verdict at these sizes (csrc/verdict_wide.hip).  dq_version() stays 8: the capability is the presence of this symbol.
 * dq_wide_uf_verdict_refereed: dq_decode_verdict's byte, every field, with the matching referee `m` (dq_match_create of the handle's d) as the referee: residual =
 * hidden XOR frame (frame_dev NULL: no correction), true = its perfect syndrome, correct = its homology class (dq_wide_uf_verdict's two fields, bit for
 * bit), decoded = the referee's class for true -- component 0 always, component 1 unless the handle's error model is DQ_MODEL_X, as the wide environment's
 * step asks it -- DQ_VERDICT_SUCCESS = true == 0 and correct == 0 (the step's reward 1), DQ_VERDICT_ALIVE = success or decoded == correct (the step's
 * done == False).  A residual in the code space is not sent to the referee: decoded = 0, which is the referee's class for the empty syndrome.
 * inexact_dev (nullable) uint8 [n]: 1 where one of the referee's flagged fallbacks fired (a cluster beyond 20 defects, defects beyond the first 32 of a
 * component), as dq_match_decode reports it.  One wavefront per volume.  n in 1 .. max_streams, null handles or arrays, and a referee of another d are
 * DQ_ERR_INVALID before any device work; the referee's scratch-pool locks are re-zeroed on `stream` in front of the launch, as dq_match_decode does.  `m` is
 * used by one stream at a time, like the handle.  dq_decode_count's "alive" counter of these bytes is the number of episodes the environment would not
 * have ended.  No reference counterpart beyond the step's rule (Environments.py:139-151). */
dq_status dq_wide_uf_verdict_refereed(dq_wide_uf* h, const dq_match* m, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev,
                                      uint8_t* inexact_dev, void* stream);
/* The union-find referee (csrc/uf_plane.hip, csrc/uf_plane_dev.h).  dq_version() stays 8: the capability is the presence of these two
 * symbols.  The class of a perfect syndrome by the closed union-find decode of a one-round window: per component only the d^2 space edges exist (edge id =
 * qubit id), growth, min-labels and lowest-edge-id peeling are dq_wide_uf_decode_closed's at T = window = 1, and the class is the parity of the logical bits of
 * the correction's qubits.  The empty syndrome gives class 0.  One wavefront per (syndrome, component), 1520 bytes of LDS each; nothing is inexact.
 * dq_uf_referee_decode: dq_match_decode's layouts without the inexact array -- defects_dev uint64 [batch][2 components][2 words], class_dev uint8 [batch] =
 * X part (+ 2 * Z part when both_components != 0); the handle supplies the lattice (its error model and window are not read).  batch >= 1; a null argument or
 * a batch below 1 is DQ_ERR_INVALID before any device work.
 * dq_wide_uf_verdict_refereed_uf: dq_wide_uf_verdict_refereed's byte, field for field, with this referee in the matching referee's place (component 1 unless
 * the handle's error model is DQ_MODEL_X); a residual in the code space is not sent to the referee.  No referee handle, no flags, and no launch is slow: any
 * n in 1 .. max_streams goes in one launch whatever the density of the residuals. */
dq_status dq_uf_referee_decode(const dq_wide_uf* h, const uint64_t* defects_dev, int batch, int both_components, uint8_t* class_dev, void* stream);
dq_status dq_wide_uf_verdict_refereed_uf(dq_wide_uf* h, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, void* stream);
/* The closed forms (a final round of perfect measurements): dq_stream_decode_uf_closed's and dq_stream_run_uf_closed's rule on this handle, with
 * dq_wide_uf_decode's and dq_wide_uf_run's arguments, validation and contract.  For d <= 7 and window <= 16 every field equals the narrow closed forms'. */
dq_status dq_wide_uf_decode_closed(dq_wide_uf* h, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                                   int32_t* n_defects_dev, int32_t* rounds_dev, void* stream);
dq_status dq_wide_uf_run_closed(dq_wide_uf* h, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                                int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);
/* Weighted union-find.  dq_version() stays 8: the capability is the presence of these two symbols.  The algorithm, the window schedule,
 * the carry and the closed final window are dq_wide_uf_decode's / dq_wide_uf_run's with one change: an edge has an integer weight w and is full when its
 * growth reaches 2 w instead of 2 -- w_space for the space edges (those to the boundary included), w_time for the time edges (the last round's edges to the
 * boundary included).  In a growth round an edge gains 1 per end in an active cluster; rounds_dev counts these unit rounds (the kernel jumps from one filling
 * edge to the next, which changes no result), weight_dev is the sum of the weights of the committed edges.  With (1, 1) every field equals the unweighted
 * forms'; (k w_space, k w_time) gives the frame of (w_space, w_time), k times its rounds and k times its weight.  One pair holds for a whole stream, every
 * window and both components.
 * closed: 0 = dq_wide_uf_decode / dq_wide_uf_run, 1 = their _closed forms.  w_space, w_time: the pair of every stream, each in 1 .. 15.
 * weights_each_dev (nullable): uint8 [n][2] on the device, (w_space, w_time) of stream i; it replaces the uniform pair, which must still be valid.  The
 * caller keeps its bytes in 1 .. 15; the kernel clamps them to that range, so a bad byte changes a result but cannot overrun the growth byte.
 * Every other argument, the validation and the error codes are those of the unweighted forms; closed outside {0, 1} or a uniform weight outside 1 .. 15 is
 * DQ_ERR_INVALID before any device work.  The environment policies (dq_envb_uf_select, dq_envb_guided_select_uf) keep unit weights; their weighted forms are
 * dq_envb_uf_select_weighted and dq_envb_guided_select_uf_weighted. */
dq_status dq_wide_uf_decode_weighted(dq_wide_uf* h, const uint8_t* syndromes_dev, int n, int T, int commit, int closed, int w_space, int w_time,
                                     const uint8_t* weights_each_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev,
                                     void* stream);
dq_status dq_wide_uf_run_weighted(dq_wide_uf* h, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                  const double* p_phys_each, const double* p_meas_each, int closed, int w_space, int w_time, const uint8_t* weights_each_dev,
                                  uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                                  int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);
/* Correlated union-find.  dq_version() stays 8: the capability is the presence of these two symbols.  Under depolarising noise a Y
 * error flips one qubit in both components, so a correction of one component says where the other one's errors are likely.  Per stream and per window, inside
 * the weighted forms' schedule, carry and closed final window, three component decodes are made instead of two:
 *   pass 0  component 0 with (w_space, w_time), dry: nothing is committed; mask A = the space edges (round, qubit) of its correction, in every round of the
 *           window, committed or not
 *   pass 1  component 1, a space edge weighing w_corr where A has it and w_space elsewhere; committed as in the weighted form (frame, carry, weight = the sum
 *           of the weights used, rounds); mask B = the space edges of its whole correction
 *   pass 2  component 0 on pass 0's rows with B in A's place, committed
 * weight_dev and rounds_dev count passes 1 and 2.  A component without defects in the window leaves an empty mask; with w_corr = w_space every field equals the
 * weighted forms'.  The result of a stream is a function of the stream alone.
 * w_corr: in 1 .. w_space, else DQ_ERR_INVALID before any device work.  weights_each_dev (nullable): uint8 [n][3] on the device, (w_space, w_time, w_corr) of
 * stream i; the kernel clamps the pair to 1 .. 15 and w_corr to 1 .. w_space.  Every other argument, the validation and the error codes are those of the
 * weighted forms.  The kernels need 2 x window x 32 bytes of LDS more than the handle's other launches (65 200 bytes at d = 15, window 32). */
dq_status dq_wide_uf_decode_correlated(dq_wide_uf* h, const uint8_t* syndromes_dev, int n, int T, int commit, int closed, int w_space, int w_time, int w_corr,
                                       const uint8_t* weights_each_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev,
                                       void* stream);
dq_status dq_wide_uf_run_correlated(dq_wide_uf* h, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                    const double* p_phys_each, const double* p_meas_each, int closed, int w_space, int w_time, int w_corr,
                                    const uint8_t* weights_each_dev, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev,
                                    int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream);

/* The union-find decoder as a policy and as a teacher of the wide environment, any odd d in 3 .. 15 (csrc/env_wide_uf.hip).
 * dq_version() stays 8: the capability is the presence of these two symbols.  The rules are dq_env_uf_select's and dq_env_guided_select_uf's on the wide
 * handle's lattice records, which are read in place and never written; the decoder is dq_wide_uf's component decode on the lattice's current volume taken
 * as one last window (window = commit = volume_depth), one workgroup of 256 threads per lattice, dynamic LDS sized from (d, volume_depth).
 * dq_envb_uf_select: action_dev[i] = the lowest action index of the union-find frame of lattice i's volume that is not in its completed_actions, else the
 * identity; the identity for a lattice whose done flag is set.  Frame to actions: X model: the X part on layer 0; use_Y: Pauli code 1 / 2 / 3 on layer
 * 0 / 1 / 2; otherwise the X part on layer 0 and the Z part on layer 1.  The legal set is not consulted.
 * dq_envb_guided_select_uf: with w[0..3] the Philox words dq_policy_select_wide draws for (seed, t, the environment's env_id_base + i):
 * explore = q_dev == NULL || w[1] < T(eps); guided = explore && w[2] < T(guide_share); a guided lattice gets dq_envb_uf_select's action, another exploring
 * one the k-th member of the record's legal set, k = umulhi(w[0], n_legal) (-1 for an empty set), the rest the first maximum of their row of q_dev
 * (float32 [n_envs][num_actions]; over the legal set when masked_greedy).  guided_dev uint8 [n_envs] (nullable): 1 where the lattice followed the decoder.
 * Only the guided lattices run the decoder.
 * Both: DQ_ERR_INVALID before any device work for a null handle, action_dev or seed, an action_dev or q_dev that is not 4-byte aligned, eps or guide_share
 * outside [0, 1], a decoder handle of another d or error model, or one whose window is below the environment's volume_depth; DQ_ERR_UNSUPPORTED if the
 * device refuses the LDS.  The dq_wide_uf handle is only read: its max_streams does not bound n_envs.  One host thread and one stream at a time per handle,
 * as for dq_wide_uf_*.  No reference counterpart. */
dq_status dq_envb_uf_select(dq_envb* env, dq_wide_uf* h, int32_t* action_dev, void* stream);
dq_status dq_envb_guided_select_uf(dq_envb* env, dq_wide_uf* h, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                   const uint32_t seed[2], uint64_t t, int32_t* action_dev, uint8_t* guided_dev, void* stream);
/* The weighted forms.  dq_version() stays 8: the capability is the presence of these two symbols.  dq_envb_uf_select's and
 * dq_envb_guided_select_uf's rules, arguments, validation and error codes with one change: the lattice's volume is decoded on dq_wide_uf_decode_weighted's
 * graph -- still one last open window, so the last round's time edges to the boundary cost w_time.  w_space, w_time: the pair of every lattice, each in
 * 1 .. 15.  weights_each_dev (nullable): uint8 [n_envs][2] on the device, (w_space, w_time) of lattice i; it replaces the uniform pair, which is then not
 * read.  The caller keeps its bytes in 1 .. 15; the kernel clamps them to that range (0 decodes as 1, 200 as 15), so a bad byte changes an action but cannot
 * overrun the growth byte.  Without an array a uniform weight outside 1 .. 15 is DQ_ERR_INVALID before any device work.  With (1, 1) every action equals the
 * unweighted forms'; a lattice whose done flag is set gets the identity; in the guided form only the guided lattices run the decoder and every other
 * lattice's action and flag are dq_envb_guided_select_uf's.  The records are read in place and never written. */
dq_status dq_envb_uf_select_weighted(dq_envb* env, dq_wide_uf* h, int w_space, int w_time, const uint8_t* weights_each_dev, int32_t* action_dev,
                                     void* stream);
dq_status dq_envb_guided_select_uf_weighted(dq_envb* env, dq_wide_uf* h, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                            const uint32_t seed[2], uint64_t t, int w_space, int w_time, const uint8_t* weights_each_dev,
                                            int32_t* action_dev, uint8_t* guided_dev, void* stream);
/* The correlated forms.  dq_version() stays 8: the capability is the presence of these two symbols.  The weighted forms' rules,
 * arguments, validation and error codes with one change: the lattice's volume -- still one last open window -- is decoded by dq_wide_uf_decode_correlated's
 * three passes: component 0 dry under (w_space, w_time); component 1 with w_corr on the space edges (t, q) of that correction; component 0 again with w_corr
 * on the space edges of component 1's correction.  The action is then the weighted forms'.  w_corr: in 1 .. w_space.  weights_each_dev (nullable): uint8
 * [n_envs][3] on the device, (w_space, w_time, w_corr) of lattice i; it replaces the uniform triple, which is then not read; the kernel clamps the pair to
 * 1 .. 15 and w_corr to 1 .. w_space.  Without an array a uniform pair outside 1 .. 15 or a w_corr outside 1 .. w_space is DQ_ERR_INVALID before any device
 * work.  With w_corr = w_space every action equals the weighted forms'; under the X model component 1 is not decoded, there is no mask, and every action
 * equals the weighted forms' whatever w_corr.  A lattice whose done flag is set gets the identity; in the guided form only the guided lattices run the
 * decoder.  The records are read in place and never written. */
dq_status dq_envb_uf_select_correlated(dq_envb* env, dq_wide_uf* h, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev,
                                       int32_t* action_dev, void* stream);
dq_status dq_envb_guided_select_uf_correlated(dq_envb* env, dq_wide_uf* h, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                              const uint32_t seed[2], uint64_t t, int w_space, int w_time, int w_corr,
                                              const uint8_t* weights_each_dev, int32_t* action_dev, uint8_t* guided_dev, void* stream);

/* Batched agent decoding for any odd d in 3 .. 15 (csrc/decode_wide.hip).  dq_version() stays 8: the capability is the presence of
 * these symbols.  The semantics are dq_decode_run's, statement for statement, with DQ_DECODE_PLANES_ENV and DQ_DECODE_OBS_UINT8 (patch words and the README
 * quirk stay narrow-only); what differs is the state: LW = ceil(num_actions / 64) <= 11 legal and as many completed words per volume, ceil(d^2 / 64) <= 4
 * words each for the acted-on qubits and the two frame components, grid masks of ceil((d+1)^2 / 64) <= 4 words per slice, one wavefront per volume.  For
 * d <= 7 every output equals dq_decode_run's on uint8 rows, bit for bit (the same forward on the same rows in the same order).  dq_decode_cfg is reused
 * (its d: odd, 3 .. 15), so dq_struct_size has no new id.
 * dq_decode_wide_create: cfg->d odd in 3 .. 15, volume_depth 1 .. 16, a DQ_MODEL_*, max_actions 1 .. num_actions - 1, max_volumes >= 1 (else
 * DQ_ERR_INVALID); action_planes != DQ_DECODE_PLANES_ENV or obs_form != DQ_DECODE_OBS_UINT8: DQ_ERR_UNSUPPORTED; all before any device work.
 * dq_decode_wide_pack: starts a decode of n <= max_volumes volumes (syndromes_dev uint8 [n][volume_depth][d+1][d+1], 4-byte aligned): observation rows
 * with empty action planes, reset_legal_moves' legal set of the summed volume, corrections = -1, the identity active list.  The four output arrays are
 * dq_decode_run's; the handle keeps their pointers, and the steps that follow write them: they must stay valid until the decode ends.
 * dq_decode_wide_step: one selection and one stable compaction over the current active list with the caller's Q rows, q_dev float32 [n_active][num_actions]
 * in active-list order; *n_active_out (nullable) receives the next active count.  It synchronises `stream` (the one host wait of an iteration).  A chosen
 * value that is not finite raises a sticky device word that is read together with the count: DQ_ERR_RANGE, and the decode is over (pack starts the next
 * one).  DQ_ERR_STATE without a pack, with no volume active, or after max_actions steps.
 * dq_decode_wide_run: pack, then dq_qnet_forward_multi (index gather over the active list) and step until no volume is active; dq_decode_run's arguments,
 * checks of the network against the lattice, host waits and final dq_qnet_range_check.
 * The accessors return device pointers of the handle's own buffers for reading (tests, diagnostics): the observation rows uint8 [max_volumes][row_bytes],
 * row_bytes = (volume_depth + layers) (2d+1)^2, row v = volume v; the legal and completed words uint64 [max_volumes][legal_words]; the current active list
 * int32 [n_active].  Out-pointers may be NULL.  One host thread and one stream at a time per handle.  No reference counterpart beyond README.md:786-829. */
typedef struct dq_decode_wide dq_decode_wide;
dq_status dq_decode_wide_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode_wide** out);
void dq_decode_wide_destroy(dq_decode_wide* h);
dq_status dq_decode_wide_pack(dq_decode_wide* h, const uint8_t* syndromes_dev, int n, int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev,
                              uint8_t* status_dev, void* stream);
dq_status dq_decode_wide_step(dq_decode_wide* h, const float* q_dev, int* n_active_out, void* stream);
dq_status dq_decode_wide_run(dq_decode_wide* h, dq_qnet* net, const float* params_dev, const void* packed_dev, const uint8_t* syndromes_dev, int n,
                             int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev, uint8_t* status_dev, int* iterations, void* stream);
dq_status dq_decode_wide_rows(const dq_decode_wide* h, const uint8_t** rows_dev, int* row_bytes);
dq_status dq_decode_wide_words(const dq_decode_wide* h, const uint64_t** legal_dev, const uint64_t** completed_dev, int* legal_words);
dq_status dq_decode_wide_active(const dq_decode_wide* h, const int32_t** active_dev, int* n_active);

/* ---------------------------------------------------------------------------------------------
 * Live kernel timing (measurement only; no reference counterpart).  dq_prof_arm(id, n) times up to n
 * launches of kernel family `id` (0 <= id < dq_prof_kernel_count(), names from dq_prof_kernel_name) with HIP
 * events on the stream they are launched on -- the fused chains and the environment step carry the event pair
 * on the launch itself (the dispatch's own start / end timestamps), the small per-layer kernels are bracketed
 * by one --; dq_prof_collect synchronises on the last recorded event and returns the number of launches
 * recorded since the last collect and the sum of their durations.  dq_prof_stride(s) (s >= 1; reset to 1 by
 * every dq_prof_arm) times only every s-th launch of the armed family: a timed launch costs the stream a few
 * microseconds, a sample of the launches leaves the timed region undisturbed.
 * dq_prof_arm(-1, 0) disarms.  Not thread-safe; one family at a time.
 * ------------------------------------------------------------------------------------------- */
int dq_prof_kernel_count(void);
const char* dq_prof_kernel_name(int kernel_id);
/* The kernel SYMBOL the family's most recent launch used ("" before its first launch): a family has several forms
 * (conv_chain_kernel: conv_wave_kernel / conv_chain_pkernel / conv_chain_kernel; conv_bwd_chain_kernel: conv_bwd16_kernel /
 * conv_bwd_chain_kernel), and a measurement must name the one that ran. */
const char* dq_prof_kernel_symbol(int kernel_id);
dq_status dq_prof_arm(int kernel_id, int max_launches);
dq_status dq_prof_stride(int stride);
dq_status dq_prof_collect(int* launches, double* total_ms);
/* The same with the shortest and the longest of the recorded launches (either pointer may be NULL): the spread a reader needs to tell a
 * slower box from a slower kernel. */
dq_status dq_prof_collect_spread(int* launches, double* total_ms, double* min_ms, double* max_ms);

#ifdef __cplusplus
}
#endif
#endif /* DEEPQ_HIP_H */
