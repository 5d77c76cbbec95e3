/*
 * t2omca.h — C-ABI of the MI355X-native T2OMCA learner hot path.
 *
 * The reference (hj5717/T2OMCA) is pure Python/PyTorch; its "plugin API" for
 * this path is two nn.Module classes driven by PyMARL registries
 * (SURVEY.md §8 b).  Every entry point below replaces one piece of the
 * reference's CPU arithmetic and is bound from Python with ctypes
 * (t2omca_amd/_lib.py; see INTEGRATION.md for the binding a maintainer adds
 * to the reference tree):
 *
 *   t2o_agent_unroll_fwd   TransformerAgent.forward unrolled over t
 *                          (transf_agent.py:54-76, transformer.py:40-178)
 *   t2o_agent_unroll_bwd   BPTT of the above (autograd of the same lines)
 *   t2o_mixer_unroll_fwd   TransformerMixer.forward unrolled over t
 *                          (n_transf_mixer.py:55-91) incl. the learner's
 *                          chosen-Q gather / double-Q argmax
 *   t2o_mixer_unroll_bwd   BPTT of the above
 *   t2o_td_loss            learner.train's TD target / loss / priorities
 *                          (call site per_run.py:224-238; PyMARL2 contract)
 *   t2o_td_stats           the masked sums the learner's log values come from
 *   t2o_episode_stats      the runner's per-run statistics (parallel_runner.py:202-210)
 *   t2o_adam_step          optimiser step with global-norm clipping
 *   t2o_td_qlambda         t2o_td_loss with Peng's Q(λ) targets (q_lambda: True)
 *   t2o_rmsprop_step       the RMSprop optimiser step (optimizer != 'adam')
 *   t2o_noise_normal / t2o_noisy_head_*  the NoisyLinear Q head (action_selector: noisy-new)
 *   t2o_q_select / t2o_qmix_* / t2o_vdn_bwd  the QMIX and VDN mixers (mixer: qmix, vdn)
 *   t2o_qplex_*            the QPLEX duelling mixer (mixer: dmaq)
 *   t2o_env_step / reset   MultiAgvOffloadingEnv.step/reset/get_obs/get_state
 *                          (environment_multi_mec.py:184-366, normalization.py)
 *
 * Conventions (all entry points):
 *   - arguments are raw device pointers + explicit sizes + a hipStream_t
 *     passed as void*; the library never allocates or frees device memory and
 *     never synchronises: the caller owns every buffer, including workspaces;
 *   - return 0 on success, a negative T2O_E* code on a bad argument, or the
 *     positive hipError_t of a failed launch;
 *   - float tensors are fp32, row-major, contiguous unless a stride is given.
 *
 * Memory contract (tests/test_gpu_memory_contract.py holds every entry point to it
 * on tensors carved from a poisoned arena, tests/arena.py):
 *   - strides are in ELEMENTS of the tensor's type, positive, and apply to the two
 *     leading axes only (episode b, step t): what lies inside one (b, t) — [a][...] —
 *     is dense.  sb < st (time-major storage viewed [b][t]) and sb > T * st (a
 *     [:, :T] slice of a longer, padded slab) are both fine; rows must not overlap;
 *   - a kernel never USES a value outside the logical elements [0, B) x [t range]
 *     of a strided input (loads of padding lanes / rows are clamped to in-bounds
 *     duplicates), so the memory between the rows of a view and past its last step
 *     may hold anything, NaNs included;
 *   - a kernel never WRITES outside the stated size of an output or a workspace:
 *     the sizes given here (t2o_bwd_tape_floats, t2o_*_bwd_max_slabs x grad_total,
 *     t2o_mixer_bwd_work_floats, t2o_adam_workspace_floats,
 *     t2o_per_workspace_doubles, t2o_noisy_head_parts, pack_floats) are exact, no
 *     slack is needed behind them.  Partial 16-row tiles mask their stores;
 *   - alignment: every float pointer is 16-byte aligned where the kernels move whole
 *     4-float groups — all dense float outputs, workspaces, packs, h0 / h_seq / hmid /
 *     gh / gcarry, hw / xout / xmid, and the mixers' strided hid_on / hid_tg / hid,
 *     whose hid_sb / hid_st are therefore multiples of 4 floats (T2O_EINVAL
 *     otherwise).  obs, states, reward and the q / qv arrays are read element-wise:
 *     4-byte alignment and any strides; actions 8-byte (int64), avail 4-byte (int32),
 *     masks their element's size.
 */
#ifndef T2OMCA_H
#define T2OMCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2O_MAX_DEPTH 4

/* Bumped whenever an entry point's signature, t2o_layout, or a workspace / tape
 * size or layout formula changes, so a binding built against one header can
 * refuse a library built from another (t2o_abi_version).  History: 3 = round-3
 * library (tuned one-tile mixers write one compact tape stream per block,
 * ceil(B*T*(A+3)/16) tiles; records of 4E + 2HE features); 4 = t2o_td_loss_ex2,
 * t2o_bwd_tape_contract_pair, t2o_abi_version; 5 = the step-range / split-phase
 * entry points; 6 = one argument struct per unroll / BPTT / contraction / TD
 * loss entry point (their _ex / _ex2 / _range / _split / _pair generations
 * folded in), t2o_args_sizeof, t2o_agent_bwd_ranges. */
#define T2O_ABI_VERSION 6
int t2o_abi_version(void);

enum {
  T2O_OK = 0,
  T2O_EINVAL = -1,      /* unsupported size / null pointer */
  T2O_EUNSUPPORTED = -2 /* no kernel instantiated for this (E, H, D, n) */
};

/* Offsets (in elements) of every tensor of one network's device pack.  The pack
 * holds the folded weights the kernels read (M_h = Wk_hᵀWq_h/√E,
 * N_h = U_h·Wv_h, zero-padded embedding / head matrices) plus transposed
 * copies for the backward.  Order: forward matrices [0, vec_lo), forward
 * vectors (biases, LayerNorm) [vec_lo, fwd_total), transposed copies
 * [fwd_total, total).  kind 0 = agent, 1 = mixer.
 * prec 0 (fp32): the pack is `total` floats.  prec 1 (bf16 MFMA operands): the
 * fp32 pack is followed, at float offset `total`, by a bf16 image of it (the
 * kernels read matrices from the image and vectors from the fp32 part); the
 * buffer is `pack_floats` floats.  Activations, LayerNorm, softmax, recurrent
 * state and every accumulation stay fp32 in both modes. */
typedef struct {
  int32_t kind, E, H, D, F, NA, FF, n_ent;
  int32_t prec;
  int32_t generic;            /* 1: no tuned kernel instance for this shape; the
                                 runtime-shaped kernels run (t2o_generic.hip) and the
                                 pack is the reference-order parameters followed by
                                 transposed copies; compact grads = reference order */
  int64_t WeT, We, be;        /* WeT[16][E], We[E][16], be[E] (F <= 16) */
  int64_t Wo, bo, WoT;        /* agent: q_basic padded Wo[16][E], bo[16], WoT[E][16];
                                 mixer: hyper_b2.weight in Wo row 0, bias in bo[0] */
  int64_t M[T2O_MAX_DEPTH], MT[T2O_MAX_DEPTH];   /* [H*E][E], [E][H*E] */
  int64_t N[T2O_MAX_DEPTH], NT[T2O_MAX_DEPTH];   /* [E][H*E], [H*E][E] */
  int64_t bu[T2O_MAX_DEPTH], g1[T2O_MAX_DEPTH], n1[T2O_MAX_DEPTH];
  int64_t W1[T2O_MAX_DEPTH], W1T[T2O_MAX_DEPTH], c1[T2O_MAX_DEPTH]; /* [FF][E],[E][FF],[FF] */
  int64_t W2[T2O_MAX_DEPTH], W2T[T2O_MAX_DEPTH], c2[T2O_MAX_DEPTH]; /* [E][FF],[FF][E],[E] */
  int64_t g2[T2O_MAX_DEPTH], n2[T2O_MAX_DEPTH];
  int64_t fwd_total;          /* elements [0, fwd_total) = every tensor the forward reads */
  int64_t total;              /* elements of the pack */
  int64_t grad_total;         /* size of the compact gradient block (no transposes) */
  int64_t vec_lo;             /* first vector element (see above) */
  int64_t pack_floats;        /* buffer size of a pack in floats (prec 1: fp32 + bf16 image) */
  int32_t n_agents;           /* mixer: agents (hidden tokens, qvals, w1 rows); n_ent = its state
                                 tokens (n_entities_state, or n_agents * n_entities for the obs
                                 branch of n_transf_mixer.py:62-63).  agent: = n_ent */
  int32_t pos_func;           /* mixer head positivity (n_transf_mixer.py:95-103):
                                 T2O_POS_ABS / _SOFTPLUS / _QUADRATIC / _IDENTITY */
  float pos_beta;             /* softplus beta (qmix_pos_func_beta) */
  int32_t reserved_;
} t2o_layout;

#define T2O_POS_ABS 0
#define T2O_POS_SOFTPLUS 1
#define T2O_POS_QUADRATIC 2
#define T2O_POS_IDENTITY 3

/* t2o_layout_init_ex flags */
#define T2O_LAYOUT_FORCE_GENERIC 1  /* use the runtime-shaped kernels even for a tuned shape */

/* Fill *L for a network (prec 0 = fp32, 1 = bf16 MFMA operands); returns 0 or T2O_EINVAL.
 * Shapes with a tuned MFMA kernel instance get the folded MFMA pack: the default
 * network (E 32 / 3 heads / depth 2 / FF 128) at any entity count 1..64 — exact
 * instances at 3, 8, 16 and 64, runtime-entity instances of capacity 8 / 16 / 64
 * (agent) and 8 / 13 / 16 / 32 / 64 (mixer) otherwise (t2o_layout_instance) — and
 * E 16 / 2 heads / depth 1 / FF 64 at 3 (a fixture shape).  Any other shape within
 * the runtime-shaped kernels' limits (E <= 64, H <= 8, H*E <= 512, D <= 4, FF <= 512,
 * F <= 16, NA <= 16, agent entities <= 64, mixer tokens n_ent + n_agents + 3 <= 192
 * with n_agents <= 64), a mixer head other than abs, or n_agents != n_ent, gets
 * generic = 1.  The generic kernels compute in fp32 whatever prec says. */
int t2o_layout_init(t2o_layout* L, int kind, int E, int H, int D, int F, int NA, int FF, int n_ent, int prec);
/* t2o_layout_init with the mixer's agent count (n_agents; 0 = n_ent), its head's
 * positivity function (T2O_POS_*, softplus beta) and flags (T2O_LAYOUT_*). */
int t2o_layout_init_ex(t2o_layout* L, int kind, int E, int H, int D, int F, int NA, int FF, int n_ent, int prec,
                       int n_agents, int pos_func, float pos_beta, int flags);

/* Which kernels a layout runs: T2O_INSTANCE_EXACT (MFMA instance compiled for its
 * entity count), T2O_INSTANCE_RUNTIME (MFMA instance of a capacity class, entity
 * count read at run time), T2O_INSTANCE_GENERIC (runtime-shaped fp32 kernels);
 * negative on a null layout. */
#define T2O_INSTANCE_EXACT 0
#define T2O_INSTANCE_RUNTIME 1
#define T2O_INSTANCE_GENERIC 2
int t2o_layout_instance(const t2o_layout* L);

/* sizeof(t2o_layout), for bindings to check their mirror of the struct. */
int t2o_layout_sizeof(void);

/* Reference parameter order (state_dict order of transf_agent.py /
 * n_transf_mixer.py, SURVEY.md §8 b) flattened into one fp32 buffer:
 *   feat_embedding.{weight[E][F], bias[E]},
 *   per block: tokeys[HE][E], toqueries[HE][E], tovalues[HE][E],
 *              unifyheads.{weight[E][HE], bias[E]}, norm1.{w,b}[E], norm2.{w,b}[E],
 *              ff.0.{weight[FF][E], bias[FF]}, ff.2.{weight[E][FF], bias[E]},
 *   agent: q_basic.{weight[NA][E], bias[NA]};  mixer: hyper_b2.{weight[1][E], bias[1]}.
 * Returns the number of floats. */
int64_t t2o_param_count(int kind, int E, int H, int D, int F, int NA, int FF);

/* params (reference order) -> device pack (folded + padded + transposed). */
int t2o_pack_params(const t2o_layout* L, const float* params, float* pack, void* stream);

/* compact gradient block (pack layout, from the backward kernels) ->
 * gradients in the reference parameter order (accumulated: grad += ...). */
int t2o_unpack_grads(const t2o_layout* L, const float* params, const float* gpack,
                     float* grad, void* stream);

/* ---- The unrolls, their BPTTs, the tape contraction and the TD loss take ONE
 * argument struct each (ABI 6): named fields instead of 25-45 positional
 * arguments, so a binding cannot shift a pointer into the wrong slot unnoticed.
 * Bindings check their mirror of every struct with t2o_args_sizeof. */
#define T2O_ARGS_AGENT_FWD 0
#define T2O_ARGS_AGENT_BWD 1
#define T2O_ARGS_MIXER_FWD 2
#define T2O_ARGS_MIXER_BWD 3
#define T2O_ARGS_TAPE 4
#define T2O_ARGS_TD 5
#define T2O_ARGS_TD_STATS 6
#define T2O_ARGS_TD_QLAMBDA 7
#define T2O_ARGS_NOISE 8
#define T2O_ARGS_NOISY_FWD 9
#define T2O_ARGS_NOISY_BWD 10
#define T2O_ARGS_NOISY_WGRAD 11
/* (12 stays unassigned: it was published as the first unknown id, for which t2o_args_sizeof gives -1) */
#define T2O_ARGS_Q_SELECT 13
#define T2O_ARGS_QMIX_FWD 14
#define T2O_ARGS_QMIX_BWD 15
/* (16 stays unassigned too: published as unknown while 15 was the last id) */
#define T2O_ARGS_QPLEX_SELECT 17
#define T2O_ARGS_QPLEX_FWD 18
#define T2O_ARGS_QPLEX_BWD 19
/* (20 stays unassigned too: published as unknown while 19 was the last id) */
#define T2O_ARGS_RNN_FWD 21
#define T2O_ARGS_RNN_BWD 22
int t2o_args_sizeof(int which); /* sizeof the T2O_ARGS_* struct, -1 for an unknown one */

/* Agent unroll forward (TransformerAgent.forward over t, transf_agent.py:54-76) for
 * up to two networks sharing the observations (online + target). */
typedef struct {
  const t2o_layout* L;
  const float* pack_on;
  const float* pack_tg;       /* NULL: one network (q_tg / h_tg / hmid_tg unused) */
  const float* obs;           /* [b][t][a][n_ent*F], element strides obs_sb, obs_st */
  int64_t obs_sb, obs_st;
  const float* h0_on;         /* [B][A][E]; NULL = zeros (init_hidden) */
  const float* h0_tg;
  float* q_on;                /* out [b][t][a][NA] */
  float* h_on;                /* out [b][t][a][E]: h after step t */
  float* hmid_on;             /* out [b][t][D-1][a][E] block inputs (NULL: not kept) */
  float* q_tg;
  float* h_tg;
  float* hmid_tg;
  int32_t B, T, A;
  int32_t t0, t1;             /* steps [t0, t1) of T (t1 <= 0: T); t0 > 0 continues from h at t0 - 1
                                 (what the range before wrote; outputs are indexed by the full T) */
} t2o_agent_fwd_args;
int t2o_agent_unroll_fwd(const t2o_agent_fwd_args* a, void* stream);

/* Agent BPTT of one network over steps t_hi - 1 .. t_lo (default: T - 1 .. 0). */
typedef struct {
  const t2o_layout* L;
  const float* pack;
  const float* obs;           /* as the forward's */
  int64_t obs_sb, obs_st;
  const float* h0;            /* as the forward's (NULL = zeros) */
  const float* h_seq;         /* forward h [b][h_ts][a][E], h_ts >= T */
  const float* hmid;          /* forward hmid [b][h_ts][D-1][a][E] or NULL (recomputed) */
  int32_t h_ts;
  const float* gq;            /* dL/dq [b][t][a][NA] or NULL */
  const float* gchosen;       /* dL/dq[action] [b][t][a] or NULL (needs actions) */
  const int64_t* actions;     /* [b][t][a], element strides act_sb, act_st, a-stride 1 */
  int64_t act_sb, act_st;
  const float* gh;            /* dL/dh [b][t][a][E] or NULL */
  float* gslabs;              /* out [nslab][grad_total] per-workgroup partial gradients (compact
                                 layout, overwritten); complete after t2o_bwd_tape_contract */
  int32_t max_slabs;          /* >= t2o_agent_bwd_max_slabs(B, A) */
  int32_t* nslab;             /* out: slabs written */
  void* tape;                 /* workspace t2o_bwd_tape_floats(L, t2o_bwd_tape_tiles(L, B, T, A)) floats */
  float* gh0;                 /* out dL/dh0 [B][A][E] or NULL */
  float* gcarry;              /* [B*A][E] dL/dh between step ranges (read at t_hi < T, written at t_lo > 0) */
  int32_t B, T, A;
  int32_t t_lo, t_hi;         /* t_hi <= 0: T.  A partial range needs the pipelined BPTT
                                 (t2o_agent_bwd_ranges; else T2O_EUNSUPPORTED); ranges run from the
                                 last one down on the same slabs (the first clears them) and tape */
} t2o_agent_bwd_args;
int t2o_agent_unroll_bwd(const t2o_agent_bwd_args* a, void* stream);
int t2o_agent_bwd_max_slabs(int B, int A);
/* The record format t2o_agent_unroll_bwd writes to its tape for this layout
 * (has_hmid: the call passes hmid): 0 the full record; 1 (bf16, the pipelined
 * kernel, up to 8 entities) the lean record — dM and dN were accumulated in
 * registers and flushed into the slabs, the tape holds only the FFN / LN1 /
 * unify-bias operands.  Pass it to the contraction (t2o_tape_args.rec_format). */
int t2o_agent_bwd_tape_format(const t2o_layout* L, int has_hmid);
/* 1 when t2o_agent_unroll_bwd accepts a partial step range for this layout
 * (has_hmid: the call passes hmid): the two-wave pipelined BPTT runs it (depth 2,
 * its LDS fits, T2O_AGENT_BWD is not "single").  Otherwise 0, and the one-wave
 * kernel takes only the whole unroll (a partial range returns T2O_EUNSUPPORTED).
 * The learner's pipelined update (step ranges on two streams) asks this first. */
int t2o_agent_bwd_ranges(const t2o_layout* L, int has_hmid);

/* Mixer unroll forward (TransformerMixer.forward over t, n_transf_mixer.py:55-91)
 * for up to two networks (online + target) in one launch, with the learner's
 * chosen-Q gather / double-Q argmax.  qmode: 0 = qvals given (qv_* [B][T][A]);
 * 1 = chosen-action gather from the network's Q array (q_on / q_tg
 * [b][q_ts][a][n_actions] at actions); 2 = double-Q: the network's Q array at
 * argmax_a' of q_on masked by avail (NULL = all available), ties -> lowest index.
 * Limits: with qmode 1 or 2 on either network, 1 <= n_actions <= t2o_mixer_max_actions()
 * (8: each lane of the MFMA instances keeps the Q row of its agent in registers),
 * T2O_EUNSUPPORTED otherwise; the runtime-shaped kernels (generic = 1) read the rows from
 * memory and take n_actions <= 64.  qmode 0 reads no Q array and has no such limit (the
 * agent head's NA <= 16 is the only one).  The flat mixers' selection (t2o_q_select,
 * t2o_qplex_select) takes NA <= 16. */
int t2o_mixer_max_actions(void);
typedef struct {
  const t2o_layout* L;
  const float* pack_on;
  const float* pack_tg;       /* NULL: one network */
  const float* states;        /* [b][t][n_ent*F], element strides st_sb, st_st */
  int64_t st_sb, st_st;
  const float* hid_on;        /* agent hidden states [b][t][a][E], strides hid_sb, hid_st, a-stride E */
  const float* hid_tg;
  int64_t hid_sb, hid_st;     /* tuned kernels load 4 floats at a time: hid_on / hid_tg 16-byte aligned,
                                 hid_sb (B > 1) and hid_st (T > 1) multiples of 4, else T2O_EINVAL */
  const float* hw0_on;        /* initial hyper tokens [B][3][E]; NULL = zeros */
  const float* hw0_tg;
  int32_t qmode_on, qmode_tg;
  const float* qv_on;
  const float* qv_tg;
  const float* q_on;
  const float* q_tg;
  int32_t q_ts, n_actions;
  const int64_t* actions;     /* [b][t][a], strides act_sb, act_st */
  int64_t act_sb, act_st;
  const int32_t* avail;       /* [b][t][a][n_actions], strides av_sb, av_st, or NULL */
  int64_t av_sb, av_st;
  float* y_on;                /* out [B][T] */
  float* hw_on;               /* out [B][T][3][E] hyper tokens after step t */
  float* qvo_on;              /* out [B][T][A] qvals used, or NULL */
  float* xout_on;             /* out [B][T][A+3][E] final query rows, or NULL (the backward needs them,
                                 and a decoupled multi-tile mixer needs them for every network) */
  float* xmid_on;             /* out [B][T][D-1][A+3][E] block inputs, or NULL (recomputed) */
  float* y_tg;
  float* hw_tg;
  float* qvo_tg;
  float* xout_tg;
  float* xmid_tg;
  int32_t B, T_on, T_tg;
  int32_t phase;              /* 0: the whole unroll.  A decoupled mixer (t2o_mixer_split) may run its
                                 phases beside the agent's step ranges on another stream: 1 = the
                                 recurrence over steps [t0, t1) (the window's rows, hw, their xout /
                                 xmid), every range in order; then 2 = every (episode, step)'s other
                                 rows and the mixing head.  T2O_EUNSUPPORTED when it does not run
                                 decoupled. */
  int32_t t0, t1;
} t2o_mixer_fwd_args;
int t2o_mixer_unroll_fwd(const t2o_mixer_fwd_args* a, void* stream);

/* Mixer BPTT of one network over steps T-1..0. */
typedef struct {
  const t2o_layout* L;
  const float* pack;
  const float* states;
  int64_t st_sb, st_st;
  const float* hid;
  int64_t hid_sb, hid_st;     /* aligned as the forward's (T2O_EINVAL otherwise) */
  const float* hw0;
  const float* qv;            /* forward qvo [B][T][A] */
  const float* hw;            /* forward hw */
  const float* xout;          /* forward xout (required) */
  const float* xmid;          /* forward xmid or NULL */
  const float* gy;            /* dL/dy [B][T] */
  const float* ghw_ext;       /* extra dL/dhw [B][T][3][E] or NULL */
  float* gqv;                 /* out dL/dqvals [B][T][A] */
  float* ghid;                /* out dL/dhidden states [B][T][A][E] */
  float* ghw0;                /* out dL/dhw0 [B][3][E] or NULL */
  float* gslabs;              /* out partial weight-grad slabs, as the agent's */
  int32_t max_slabs;          /* >= t2o_mixer_bwd_max_slabs(B) */
  int32_t* nslab;
  void* tape;                 /* t2o_bwd_tape_floats(L, tiles) floats, tiles = t2o_bwd_tape_tiles(L, B, T, A) */
  float* work;                /* t2o_mixer_bwd_work_floats(L, B, T) floats, or NULL: lets a multi-tile
                                 mixer (A + 3 > 16 query rows) at a small batch run its recurrence
                                 decoupled (the window of the last 16 query rows carries the hyper
                                 tokens, every (episode, step)'s other rows run in parallel; the key
                                 gradients sum in another order) */
  int64_t work_floats;
  float* ghw_carry;           /* [B][3][E] hyper grads between phase-2 step ranges */
  int32_t B, T;
  int32_t phase;              /* 0: the whole BPTT; decoupled: 1 = every (episode, step)'s parallel part,
                                 then 2 = the recurrence over steps t_hi - 1 .. t_lo, ranges from the
                                 last one down (*nslab the same for every call) */
  int32_t t_lo, t_hi;         /* t_hi <= 0: T */
} t2o_mixer_bwd_args;
int t2o_mixer_unroll_bwd(const t2o_mixer_bwd_args* a, void* stream);
int t2o_mixer_bwd_max_slabs(int B);
/* Workspace floats t2o_mixer_unroll_bwd can use for this layout and batch
 * (0: the layout has one query tile, nothing to decouple; -1 bad argument). */
int64_t t2o_mixer_bwd_work_floats(const t2o_layout* L, int B, int T);
/* 1 when a mixer of this layout runs decoupled at batch B (forward: when every
 * network's xout is given; backward: with the workspace), else 0.
 * T2O_MIXER_SPLIT=0 / 1 in the environment forces it off / on. */
int t2o_mixer_split(const t2o_layout* L, int B);

/* Tiles of 16 weight-gradient records per block that one backward call writes
 * (agent: T * ceil(B*A/16); mixer, A = L->n_agents: B*T*ceil((A+3)/16), or for
 * a tuned mixer with A+3 > 16 query rows, whose records form one compact stream
 * per block, ceil(B*T*(A+3)/16)).  -1 on a bad argument.  Both the tape size
 * (t2o_bwd_tape_floats) and the contraction's `tiles` take this count. */
int64_t t2o_bwd_tape_tiles(const t2o_layout* L, int B, int T, int A);

/* Floats of backward tape workspace for `tiles` tiles of 16 records:
 * D * tiles * 16 * (4E + 2HE) elements of 4 (fp32) or 2 (bf16) bytes. */
int64_t t2o_bwd_tape_floats(const t2o_layout* L, int64_t tiles);

/* One backward call's weight-gradient tape, to be contracted into its slabs. */
typedef struct {
  const t2o_layout* L;
  const float* pack;          /* the kernel pack the backward used (g1, n1, W1, W2ᵀ, c1 recompute the
                                 FFN operands the tape does not store) */
  const void* tape;
  int64_t tiles;              /* the backward's t2o_bwd_tape_tiles (the tape's per-block stride) */
  float* gslabs;              /* the backward's slabs */
  int32_t nslab;              /* >= the backward's *nslab: slabs past it must be zeroed by the caller
                                 (a small batch's contraction over more workgroups) */
  int32_t rec_format;         /* t2o_agent_bwd_tape_format; 0 = the full record (every mixer's) */
} t2o_tape_args;
/* Contract a backward tape (dM, dN, dW2, P = Σ_records dYᵀ X, split-K over the
 * slabs) into the M/N/W1/W2 regions of its slabs.  The W1 / g1 regions then hold
 * P = Σ gf1 ⊗ x̂1 and Q = Σ gr2 ⊙ x̂1, which t2o_unpack_grads turns into the W1 /
 * norm1 grads.  Format 1 adds only the FFN / LN1 / bu grads (the backward put dM /
 * dN into the slabs).  With `second` (or NULL): BOTH backwards' tapes in one
 * launch — `first` the mixer's (format 0), `second` the agent's — each exactly as
 * alone, one grid of both slab counts (the two share the chip from the start);
 * layouts that are not tuned instances of one network shape and precision run as
 * two launches.  Must follow the t2o_*_unroll_bwd call(s) on the same stream. */
int t2o_bwd_tape_contract(const t2o_tape_args* first, const t2o_tape_args* second, void* stream);

/* Element types of the TD loss's mask inputs. */
#define T2O_DT_F32 0
#define T2O_DT_U8 1   /* uint8 / bool: EpisodeBatch "terminated" */
#define T2O_DT_I32 2
#define T2O_DT_I64 3  /* int64: EpisodeBatch "filled" */

/* TD loss algorithms */
#define T2O_TD_AUTO 0        /* the library's default (currently T2O_TD_WAVE_SCAN, the faster) */
#define T2O_TD_SEQUENTIAL 1  /* one thread per episode, the reference's backward order (t2o_td_loss:
                                T <= 4915; t2o_td_qlambda, one more staged row: T <= 4095) */
#define T2O_TD_WAVE_SCAN 2   /* one wave per episode: suffix scan of the linear TD(λ) recursion
                                (reassociated: fp32 rounding differs by ~1e-7 relative; any T) */

/* TD(λ) targets, masked PER-weighted loss, dL/dQtot and priorities (PyMARL2
 * NQLearner semantics, learner.train at per_run.py:224-238; t2o_learner.hip). */
typedef struct {
  const float* qtot;          /* [B][T] online mixer */
  const float* qtot_tgt;      /* [B][T+1] target mixer */
  const float* reward;        /* [b][t], element strides rw_sb, rw_st */
  int64_t rw_sb, rw_st;
  const void* term;           /* [b][t] 0/1 (NULL: none), element type term_dtype, strides tm_* */
  int64_t tm_sb, tm_st;
  const void* filled;         /* [b][t] 0/1 (NULL: all), element type filled_dtype, strides fl_* */
  int64_t fl_sb, fl_st;
  const float* per_weight;    /* [B] or NULL (= 1) */
  float* gq;                  /* out [B][T] dL/dQtot */
  float* targets;             /* out [B][T] or NULL */
  float* prio;                /* out [B] */
  float* loss;                /* out [2] = {loss, local Σ mask} */
  float* mask_sum_acc;        /* NULL, or += local Σ mask (the learner keeps Σ mask in its flat
                                 gradient's last slot: the data-parallel all-reduce sums it with the
                                 grads and Adam divides by the global value) */
  float gamma, td_lambda;
  float mask_sum;             /* > 0: normalise gq / loss by this global Σ mask; else by the local one */
  int32_t term_dtype, filled_dtype;  /* T2O_DT_*: the EpisodeBatch's own types, read in place */
  int32_t algo;               /* T2O_TD_* */
  int32_t B, T;
} t2o_td_args;
int t2o_td_loss(const t2o_td_args* a, void* stream);

/* Peng's Q(λ) targets (PyMARL2 build_q_lambda_targets, NQLearner q_lambda: True)
 * in place of the TD(λ) ones; everything else — mask m, loss, gq, prio, loss[2],
 * mask_sum / mask_sum_acc, mask dtypes, priority 0 of an all-masked episode,
 * algo — as t2o_td_loss.  With Q' = qtot_tgt, Qk = qtot_taken:
 *   ret_T = Q'_T (1 - Σ_t term_t)
 *   ret_t = λγ ret_{t+1} + m_t (r_t + (Q'_t - Qk_t) + (1-λ)γ Q'_{t+1} (1 - term_t)),  t = T-1 .. 0
 *   targets = ret_{0..T-1}
 * The correction (Q'_t - Qk_t) is formed first and then added to r_t: with
 * qtot_taken equal to qtot_tgt it is an exact zero and the outputs are
 * t2o_td_loss's bit for bit.  T2O_TD_SEQUENTIAL stages one more row per episode
 * in LDS than t2o_td_loss does: T2O_EUNSUPPORTED beyond T = 4095 (there 4915);
 * the wave scan takes any T.  (Added within ABI 6: nothing existing moved.) */
typedef struct {
  const float* qtot;          /* the fields of t2o_td_args, in its order ... */
  const float* qtot_tgt;
  const float* reward;
  int64_t rw_sb, rw_st;
  const void* term;
  int64_t tm_sb, tm_st;
  const void* filled;
  int64_t fl_sb, fl_st;
  const float* per_weight;
  float* gq;
  float* targets;
  float* prio;
  float* loss;
  float* mask_sum_acc;
  float gamma, td_lambda;
  float mask_sum;
  int32_t term_dtype, filled_dtype;
  int32_t algo;
  int32_t B, T;
  const float* qtot_taken;    /* ... then: the target mixer on the target Q at the taken actions;
                                 row b starts at b * qk_sb, steps 0..T-1 are read */
  int64_t qk_sb;              /* >= T (the producer may unroll T or T+1 steps) */
} t2o_td_qlambda_args;
int t2o_td_qlambda(const t2o_td_qlambda_args* a, void* stream);

/* ---- logged statistics (t2o_stats.hip).  Both entry points run one workgroup,
 * accumulate in fp64 without atomics and combine their partial sums in a fixed
 * tree, so a result depends on the inputs and the element count only: it is
 * bit-identical run to run and on any device.  T2O_EINVAL (a null required
 * pointer, a size < 1) is returned before any launch. */

/* The masked sums a PyMARL2 NQLearner logs from, over the TD loss's mask
 * m[b][t] = filled[t] * (t > 0 ? 1 - term[t-1] : 1): out = { Σ m, Σ |qtot - targets| m,
 * Σ qtot m, Σ targets m } (overwritten; every operand converted to fp64 first).
 * td_error_abs = out[1] / out[0]; q_taken_mean = out[2] / (out[0] * n_agents);
 * target_mean = out[3] / (out[0] * n_agents). */
typedef struct {
  const float* qtot;          /* [B][T] online mixer (t2o_td_args.qtot) */
  const float* targets;       /* [B][T] (t2o_td_args.targets) */
  const void* term;           /* as t2o_td_args: [b][t] 0/1 (NULL: none), strides tm_* */
  int64_t tm_sb, tm_st;
  const void* filled;         /* as t2o_td_args: [b][t] 0/1 (NULL: all), strides fl_* */
  int64_t fl_sb, fl_st;
  int32_t term_dtype, filled_dtype;  /* T2O_DT_* */
  int32_t B, T;
  double* out;                /* out [4] */
} t2o_td_stats_args;
int t2o_td_stats(const t2o_td_stats_args* a, void* stream);

/* The runner's statistics of one finished run of n envs (parallel_runner.py:202-210),
 * added to acc:
 *   acc[0] += n; acc[1] += Σ returns[i];
 *   over the envs with terminated[i] != 0 (their info dicts, :169-170):
 *   acc[2] += reward[i]; acc[3..6] += info[i][0..3] (delay_reward, overtime_penalty,
 *   channel_utilization_rate, conflict_ratio); acc[7] += 1 (episode_limit);
 *   acc[8..9] += info[i][4..5] (task_completion_rate, task_completion_delay).
 * reward / terminated / info are t2o_env_run's outputs after the run's last step
 * (info [n][6]); an unterminated env's row (NaN task_completion_*) is never read. */
#define T2O_EP_STATS 10
int t2o_episode_stats(const double* reward, const double* info, const uint8_t* terminated, const double* returns,
                      int64_t n, double* acc, void* stream);

/* clip_grad_norm_(max_grad_norm) + Adam (torch.optim.Adam semantics, L2
 * weight decay) over n floats.  workspace: t2o_adam_workspace_floats() floats
 * (needed when max_grad_norm > 0).  grad_div [1] (may be NULL): device scalar
 * every grad is divided by first (the global Σ mask under data parallelism).
 * grad_norm_out [1] may be NULL. */
int t2o_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  float* workspace, int64_t n, double lr, double beta1, double beta2, float eps,
                  float weight_decay, float max_grad_norm, int64_t step, const float* grad_div,
                  float* grad_norm_out, void* stream);
int t2o_adam_workspace_floats(void);

/* clip_grad_norm_(max_grad_norm) + torch.optim.RMSprop (momentum 0, not centered)
 * over n floats:  g += weight_decay p;  square_avg = α square_avg + (1-α) g²;
 * p -= lr g / (sqrt(square_avg) + eps).  workspace (t2o_adam_workspace_floats()
 * floats), grad_div and grad_norm_out as t2o_adam_step.  T2O_EINVAL before any
 * launch for a null required pointer or n < 1.  (Added within ABI 6.) */
int t2o_rmsprop_step(float* params, const float* grads, float* square_avg, float* workspace, int64_t n,
                     double lr, double alpha, float eps, float weight_decay, float max_grad_norm,
                     const float* grad_div, float* grad_norm_out, void* stream);

/* ---- the NoisyNet Q head (t2o_noisy.hip; transf_agent.py:37-39, args.action_selector
 * == "noisy-new": q_basic is a NoisyLinear).  utils.noisy_liner does not ship with
 * the reference, so the layer is a DECLARED definition (parity-unpinned, DESIGN.md
 * §5): the independent-Gaussian NoisyNet layer as PyMARL2 uses it,
 *   q = (u_w + s_w ⊙ ε_w) h + (u_b + s_b ⊙ ε_b),  ε ~ N(0, 1) per element,
 * u_w [NA][E], u_b [NA] the means (a plain agent's q_basic.weight / bias: the first
 * t2o_param_count floats of a noisy agent's flat parameters are a plain agent), s_w
 * [NA][E], s_b [NA] the sigmas, which follow them.  The head runs beside the fused
 * agent kernels on their h output and overwrites their q; all of it is fp32 in both
 * precisions (h is fp32; bf16 operands stop at the fused kernels).  Limits: E <= 64,
 * NA <= 16, A <= 64.  (Added within ABI 6: nothing existing moved.)  T2O_EINVAL for a
 * null required pointer or a bad size, before any launch; no allocation, no
 * synchronisation, no atomics. */

/* ε of steps [t0, t1) of an unroll of T steps.  Element k of step t (k = n·E + e for
 * ε_w[n][e], k = NA·E + n for ε_b[n]) is Box–Muller on the env_spec.uniforms stream:
 *   u1 = U(seed', env = t, draw = counter·4096 + 2k),  u2 = U(seed', t, counter·4096 + 2k + 1),
 *   seed' = (4·seed + kind) mod 2^64,  z = sqrt(−2 ln(1 − u1)) · cos(2π u2),
 * evaluated in fp64 and rounded once to fp32.  kind: 0 learner online, 1 learner
 * target, 2 runner, 3 module forward; counter: the caller's call count (the learner's
 * step_count, the runner's episode).  Limits: NA·(E+1) <= 2048, T <= 2^24,
 * 0 <= counter < 2^28. */
#define T2O_NOISE_LEARNER_ONLINE 0
#define T2O_NOISE_LEARNER_TARGET 1
#define T2O_NOISE_RUNNER 2
#define T2O_NOISE_MODULE 3
typedef struct {
  float* eps_w;               /* out [T][NA][E]; rows t0 .. t1 - 1 are written */
  float* eps_b;               /* out [T][NA] */
  uint64_t seed;
  int64_t counter;
  int32_t kind;               /* T2O_NOISE_* */
  int32_t E, NA;
  int32_t T, t0, t1;
} t2o_noise_args;
int t2o_noise_normal(const t2o_noise_args* a, void* stream);

/* The head of one network over steps [t0, t1): q[b][t][a][:] = W_t h[b][t][a][:] + b_t,
 * W_t = u_w + s_w ⊙ eps_w[t], b_t = u_b + s_b ⊙ eps_b[t], written over the q the agent
 * unroll left there.  eps_w = eps_b = NULL: the mean head (s_w / s_b unused). */
typedef struct {
  const float* h;             /* [b][h_ts][a][E]: the agent unroll's h */
  const float* u_w;
  const float* u_b;
  const float* s_w;
  const float* s_b;
  const float* eps_w;         /* [>= t1][NA][E] (t2o_noise_normal's), or NULL */
  const float* eps_b;         /* [>= t1][NA], or NULL */
  float* q;                   /* out [b][q_ts][a][NA] */
  int32_t h_ts, q_ts;
  int32_t B, A, E, NA;
  int32_t t0, t1;             /* t1 <= min(h_ts, q_ts) */
} t2o_noisy_fwd_args;
int t2o_noisy_head_fwd(const t2o_noisy_fwd_args* a, void* stream);

/* Backward of the head at the taken actions over steps [t_lo, t_hi), any ranges in
 * any order:
 *   gh_out[b][t][a][:] = gh_in[b][t][a][:] + gchosen[b][t][a] · W_t[action][:]
 *   gpart[t][p][n][0..E) = Σ over the rows (b, a) of part p with action == n of
 *                          gchosen · h,  gpart[t][p][n][E] = Σ gchosen
 * (P = t2o_noisy_head_parts(B, A) row parts per step, each summed in a fixed order
 * that depends on the shape only).  gh_out is what t2o_agent_unroll_bwd takes as gh,
 * with gchosen = gq = NULL there.  An action outside [0, NA) contributes nothing. */
typedef struct {
  const float* gchosen;       /* [B][T][A] dL/dq[action] */
  const int64_t* actions;     /* [b][t][a], element strides act_sb, act_st, a-stride 1 */
  int64_t act_sb, act_st;
  const float* h;             /* [b][h_ts][a][E], h_ts >= T */
  const float* u_w;
  const float* s_w;
  const float* eps_w;         /* as the forward's; NULL: the mean head */
  const float* gh_in;         /* [B][T][A][E] or NULL (zeros) */
  float* gh_out;              /* out [B][T][A][E] (may be gh_in) */
  float* gpart;               /* out [T][P][NA][E+1] */
  int32_t h_ts;
  int32_t B, T, A, E, NA;
  int32_t t_lo, t_hi;         /* t_hi <= 0: T */
} t2o_noisy_bwd_args;
int t2o_noisy_head_bwd(const t2o_noisy_bwd_args* a, void* stream);
int t2o_noisy_head_parts(int B, int A); /* P above (T2O_EINVAL on a bad size) */

/* After the backward has covered every step of [0, T): the head's weight gradients,
 * accumulated (+=, as t2o_unpack_grads) into the caller's slots,
 *   du_w, du_b += Σ_t Σ_p gpart[t][p],   ds_w, ds_b += Σ_t eps[t] ⊙ Σ_p gpart[t][p],
 * one wave per element in a fixed order over (t, p): bit-identical run to run and
 * whatever step ranges the backward ran in.  eps_w = eps_b = NULL: only du_*. */
typedef struct {
  const float* gpart;
  const float* eps_w;
  const float* eps_b;
  float* du_w;                /* [NA][E] */
  float* du_b;                /* [NA] */
  float* ds_w;
  float* ds_b;
  int32_t B, T, A, E, NA;
  int32_t reserved_;
} t2o_noisy_wgrad_args;
int t2o_noisy_head_wgrad(const t2o_noisy_wgrad_args* a, void* stream);

/* ---- the QMIX and VDN mixers (t2o_qmix.hip; TDLearner with mixer: qmix / vdn).
 * Neither ships with the reference (n_transf_mixer.py only): they are DECLARED
 * definitions after PyMARL2's modules/mixers/nmix.py and vdn.py (parity-unpinned,
 * DESIGN.md §5).  Per (episode, step) row, with state s [S] and the agents' q [A]:
 *   w1 = pos(hyper_w1(s)).view(A, M)   hyper_w1 = Linear(S, H), ReLU, Linear(H, A·M)
 *   b1 = hyper_b1(s)                   hyper_b1 = Linear(S, M)
 *   w2 = pos(hyper_w2(s))              hyper_w2 = Linear(S, H), ReLU, Linear(H, M)
 *   b2 = hyper_b2(s)                   hyper_b2 = Linear(S, M), ReLU, Linear(M, 1)
 *   y  = elu(q · w1 + b1) · w2 + b2
 * Parameters are read straight from a flat buffer in that registration order (each
 * Linear its weight [out][in], then its bias): t2o_qmix_param_count floats.  All
 * arithmetic is fp32.  Limits: 1 <= A <= 64, 1 <= S <= 1024, M in {16, 32}, H in
 * {32, 64}, B·T < 2^27, pos_func one of T2O_POS_*.  (Added within ABI 6: nothing existing moved.)
 * T2O_EINVAL for a null required pointer or a bad size, before any launch; no
 * allocation, no synchronisation, no atomics. */

/* The learner's chosen-Q gather and double-Q selection, for up to two networks in
 * one launch (the first over t < T_on, the second over t < T_tg), with the qmode
 * meanings, strides and tie rule of t2o_mixer_unroll_fwd: 1 = the network's Q at
 * `actions`; 2 = the network's Q at the argmax over actions of q_on masked by
 * `avail` (NULL: all available; ties -> the lowest index).  The first network reads
 * q_on, the second q_tg.  y_* (optional) = Σ_a qv: VDN's forward. */
typedef struct {
  const float* q_on;          /* [b][q_ts][a][n_actions], dense; also the argmax's source (qmode 2) */
  const float* q_tg;          /* NULL: one network */
  int32_t q_ts, n_actions;
  const int64_t* actions;     /* [b][t][a], strides act_sb, act_st (qmode 1) */
  int64_t act_sb, act_st;
  const int32_t* avail;       /* [b][t][a][n_actions], strides av_sb, av_st, or NULL */
  int64_t av_sb, av_st;
  int32_t qmode_on, qmode_tg; /* 1 or 2 */
  float* qv_on;               /* out [B][T_on][A] */
  float* qv_tg;               /* out [B][T_tg][A] */
  float* y_on;                /* out [B][T_on] or NULL */
  float* y_tg;                /* out [B][T_tg] or NULL */
  int32_t B, T_on, T_tg, A;
} t2o_q_select_args;
int t2o_q_select(const t2o_q_select_args* a, void* stream);

int64_t t2o_qmix_param_count(int A, int S, int M, int H); /* T2O_EINVAL on a size outside the limits */

/* QMIX forward of up to two networks in one launch on rows (b, t < T_*). */
typedef struct {
  const float* params_on;
  const float* params_tg;     /* NULL: one network */
  const float* states;        /* [b][t][S], element strides st_sb, st_st */
  int64_t st_sb, st_st;
  const float* qv_on;         /* [B][T_on][A] */
  const float* qv_tg;         /* [B][T_tg][A] */
  float* y_on;                /* out [B][T_on] */
  float* y_tg;                /* out [B][T_tg] */
  int32_t B, T_on, T_tg;
  int32_t A, S, M, H;
  int32_t pos_func;           /* T2O_POS_* */
  float pos_beta;
  int32_t reserved_;
} t2o_qmix_fwd_args;
int t2o_qmix_fwd(const t2o_qmix_fwd_args* a, void* stream);

/* QMIX backward of one network.  It recomputes the forward.  phase 1: every row's
 * dL/dqv into gqv and the row's small activations (4H + 4M + 4 floats) into work;
 * phase 2: the weight gradients from work, as t2o_qmix_bwd_slabs(B, T) partial
 * slabs [nslab][t2o_qmix_param_count] in the parameter order, each element written
 * once by one workgroup in a fixed order (sum them with t2o_reduce_slabs).  phase 0:
 * both, in order.  w1 [rows][A·M] is never written to memory: phase 2 recomputes it
 * per agent chunk. */
typedef struct {
  const float* params;
  const float* states;
  int64_t st_sb, st_st;
  const float* qv;            /* [B][T][A] */
  const float* gy;            /* dL/dy [B][T] */
  float* gqv;                 /* out [B][T][A] */
  float* gslabs;              /* out [>= t2o_qmix_bwd_slabs][t2o_qmix_param_count] */
  float* work;                /* t2o_qmix_bwd_work_floats floats, 16-byte aligned */
  int64_t work_floats;
  int32_t max_slabs;
  int32_t phase;
  int32_t B, T;
  int32_t A, S, M, H;
  int32_t pos_func;
  float pos_beta;
} t2o_qmix_bwd_args;
int t2o_qmix_bwd(const t2o_qmix_bwd_args* a, void* stream);
int t2o_qmix_bwd_slabs(int B, int T);                       /* T2O_EINVAL on a bad size */
int64_t t2o_qmix_bwd_work_floats(int B, int T, int M, int H);

/* VDN backward: gqv[b][t][a] = gy[b][t]. */
int t2o_vdn_bwd(const float* gy, float* gqv, int B, int T, int A, void* stream);

/* ---- the QPLEX duelling mixer (t2o_qplex.hip; TDLearner with mixer: dmaq / qplex).
 * It does not ship with the reference: the DECLARED definition after PyMARL2's
 * modules/mixers/dmaq_general.py, dmaq_si_weight.py and dmaq_qatten_learner.py at
 * qplex.yaml's defaults (weighted_head, is_minus_one, adv_hypernet_layers 2;
 * parity-unpinned).  Per (episode, step) row, with state s [S], the
 * agents' q [A], their maxima m [A] and the joint action u [A] (sg: stop-gradient):
 *   w   = |hyper_w_final(s)| + 1e-10        v = V(s)
 *   d   = [s ; onehot(u_0) ; ... ; onehot(u_{A-1})]
 *   κ_k = |key_k(s)| + 1e-10    α_k = sigmoid(agents_k(s))    β_k = sigmoid(action_k(d))
 *   λ   = Σ_k κ_k α_k ⊙ β_k
 *   y_v = Σ_a (w_a q_a + v_a)      y_adv = Σ_a sg[w_a (q_a − m_a)] (λ_a − 1)
 * Every network is Linear(in, Hx), ReLU, Linear(Hx, out), read straight from a flat
 * buffer in the registration order hyper_w_final, V (Hx = H, out = A), then
 * key_extractors[0..K-1] (Hx = HA, out 1), agents_extractors[0..K-1] (out A),
 * action_extractors[0..K-1] (in = S + A·NA, out A): t2o_qplex_param_count floats.  All
 * arithmetic is fp32.  Limits: 1 <= A <= 64, 1 <= S <= 1024, 1 <= NA <= 16, H and HA in
 * {32, 64}, 1 <= K <= 10, B·T < 2^27.  (Added within ABI 6: nothing existing moved.)
 * T2O_EINVAL for a null required pointer or a bad size, before any launch; no
 * allocation, no synchronisation, no atomics. */
int64_t t2o_qplex_param_count(int A, int S, int NA, int H, int HA, int K);

/* t2o_q_select's selection (same qmode meanings, strides and tie rule) that also
 * writes, per (b, t, a), the avail-masked maximum of the network's OWN Q (masked-out
 * entries count as -9999999) and the action index used. */
typedef struct {
  const float* q_on;          /* [b][q_ts][a][n_actions], dense; also the argmax's source (qmode 2) */
  const float* q_tg;          /* NULL: one network */
  int32_t q_ts, n_actions;
  const int64_t* actions;     /* [b][t][a], strides act_sb, act_st (qmode 1) */
  int64_t act_sb, act_st;
  const int32_t* avail;       /* [b][t][a][n_actions], strides av_sb, av_st, or NULL */
  int64_t av_sb, av_st;
  int32_t qmode_on, qmode_tg; /* 1 or 2 */
  float* qv_on;               /* out [B][T_on][A] */
  float* qv_tg;               /* out [B][T_tg][A] */
  float* qmax_on;             /* out [B][T_on][A] */
  float* qmax_tg;             /* out [B][T_tg][A] */
  int32_t* act_on;            /* out [B][T_on][A] */
  int32_t* act_tg;            /* out [B][T_tg][A] */
  int32_t B, T_on, T_tg, A;
} t2o_qplex_select_args;
int t2o_qplex_select(const t2o_qplex_select_args* a, void* stream);

/* QPLEX forward of up to two networks in one launch on rows (b, t < T_*).
 * parts: 1 = y_v, 2 = y_adv, 3 = y_v + y_adv (qmax and act are read with part 2). */
typedef struct {
  const float* params_on;
  const float* params_tg;     /* NULL: one network */
  const float* states;        /* [b][t][S], element strides st_sb, st_st */
  int64_t st_sb, st_st;
  const float* qv_on;         /* [B][T_on][A] */
  const float* qv_tg;         /* [B][T_tg][A] */
  const float* qmax_on;
  const float* qmax_tg;
  const int32_t* act_on;      /* values in [0, NA) */
  const int32_t* act_tg;
  float* y_on;                /* out [B][T_on] */
  float* y_tg;                /* out [B][T_tg] */
  int32_t B, T_on, T_tg, parts;
  int32_t A, S, NA, H, HA, K;
} t2o_qplex_fwd_args;
int t2o_qplex_fwd(const t2o_qplex_fwd_args* a, void* stream);

/* QPLEX backward of one network, of Σ gy · y(parts).  It recomputes the forward.
 * phase 1: every row's dL/dqv = gy · w (0 without part 1) into gqv, and per block its
 * hidden vector and the gradients of its pre-activation and output into work; phase 2:
 * the weight gradients from work, as t2o_qplex_bwd_slabs(B, T) partial slabs
 * [nslab][t2o_qplex_param_count] in the parameter order, each element written once by
 * one workgroup in a fixed order (sum them with t2o_reduce_slabs).  phase 0: both. */
typedef struct {
  const float* params;
  const float* states;
  int64_t st_sb, st_st;
  const float* qv;            /* [B][T][A] */
  const float* qmax;          /* [B][T][A] */
  const int32_t* act;         /* [B][T][A] */
  const float* gy;            /* dL/dy [B][T] */
  float* gqv;                 /* out [B][T][A] */
  float* gslabs;              /* out [>= t2o_qplex_bwd_slabs][t2o_qplex_param_count] */
  float* work;                /* t2o_qplex_bwd_work_floats floats, 16-byte aligned */
  int64_t work_floats;
  int32_t max_slabs;
  int32_t phase;
  int32_t parts;
  int32_t B, T;
  int32_t A, S, NA, H, HA, K;
} t2o_qplex_bwd_args;
int t2o_qplex_bwd(const t2o_qplex_bwd_args* a, void* stream);
int t2o_qplex_bwd_slabs(int B, int T);                       /* T2O_EINVAL on a bad size */
int64_t t2o_qplex_bwd_work_floats(int B, int T, int A, int H, int HA, int K);

/* ---- the GRU agent of the QMIX baselines (t2o_rnn.hip; agent: rnn).  No agent but the
 * transformer ships with the reference: the DECLARED definition after PyMARL2's
 * modules/agents/n_rnn_agent.RNNAgent with use_layer_norm = False (parity-unpinned,
 * DESIGN.md §5).  Per agent row and step, gates in torch.nn.GRUCell's order r, z, n:
 *   x  = relu(fc1 in + b1)
 *   r  = sigmoid(W_ir x + b_ir + W_hr h + b_hr)    z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *   n  = tanh(W_in x + b_in + r * (W_hn h + b_hn))
 *   h' = (1 - z) * n + z * h                       q = fc2 h' + b2
 * in = [obs ; onehot(action at t-1) if last_action ; onehot(agent) if agent_id]
 * (BasicMAC._build_inputs), IN = OBS + NA·[last_action] + A·[agent_id]; it is never
 * written to memory.  Parameters are read straight from a flat buffer in the
 * registration order fc1.weight [H][IN], fc1.bias, rnn.weight_ih [3H][H], rnn.weight_hh,
 * rnn.bias_ih, rnn.bias_hh, fc2.weight [NA][H], fc2.bias: t2o_rnn_param_count floats.
 * All arithmetic is fp32.  Limits: 1 <= A <= 64, 1 <= OBS and IN <= 656, 1 <= NA <= 16, H in
 * {32, 64}, B·T1·A < 2^27.  (Added within ABI 6: nothing existing moved.)
 * T2O_EINVAL for a null required pointer, a bad size or a misaligned buffer, before
 * any launch; no allocation, no synchronisation, no atomics. */
int64_t t2o_rnn_param_count(int IN, int H, int NA); /* T2O_EINVAL on a size outside the limits */

/* GRU agent forward of up to two networks sharing the inputs, over steps t0 <= t < t1
 * of T1 from h0 (the state before step t0; NULL: zeros).  The one-hot of the last
 * action at step t reads actions[b][t - 1 + act_shift] and is zero where that step is
 * negative or actions is NULL (act_shift 0: a whole episode; 1: one rollout step whose
 * actions hold the previous step's).  The float buffers are 16-byte aligned. */
typedef struct {
  const float* params_on;
  const float* params_tg;     /* NULL: one network */
  const float* obs;           /* [b][t][a][OBS], element strides obs_sb, obs_st; [a][OBS] dense */
  int64_t obs_sb, obs_st;
  const int64_t* actions;     /* [b][t][a], strides act_sb, act_st, or NULL */
  int64_t act_sb, act_st;
  const float* h0_on;         /* [b][a][H], episode stride h0_sb (a multiple of 4), or NULL */
  const float* h0_tg;
  int64_t h0_sb;
  float* x_on;                /* out [B][T1][A][H]: relu(fc1), for the backward; or NULL */
  float* gi_on;               /* out [B][T1][A][3H]: W_ih x + b_ih */
  float* gi_tg;
  float* q_on;                /* out [B][T1][A][NA] */
  float* h_on;                /* out [B][T1][A][H] */
  float* q_tg;
  float* h_tg;
  int32_t B, T1, A, OBS, NA, H;
  int32_t last_action, agent_id, act_shift;
  int32_t t0, t1;
  int32_t reserved_;
} t2o_rnn_fwd_args;
int t2o_rnn_fwd(const t2o_rnn_fwd_args* a, void* stream);

/* GRU agent backward of one network over steps t < T of a forward whose buffers have
 * Ts >= T steps.  dL/dq enters either as gchosen [B][T][A], the gradient at
 * actions[b][t][a] (the learner's form), or as gq [B][T][A][NA]: exactly one of them.
 * gh (optional) adds dL/dh[b][t][a][:].  The gates are recomputed from gi, h and W_hh.
 * The weight gradients leave as t2o_rnn_bwd_slabs(B, T, A) partial slabs
 * [nslab][t2o_rnn_param_count] in the parameter order, each element written once by
 * one workgroup in a fixed order (sum them with t2o_reduce_slabs).  work:
 * t2o_rnn_bwd_work_floats floats (per row the gradients of gi, of gh's n gate and of
 * fc1's pre-activation). */
typedef struct {
  const float* params;
  const float* obs;
  int64_t obs_sb, obs_st;
  const int64_t* actions;     /* [b][t][a], strides act_sb, act_st (gchosen, last_action) or NULL */
  int64_t act_sb, act_st;
  const float* h0;            /* [b][a][H], episode stride h0_sb, or NULL: zeros */
  int64_t h0_sb;
  const float* x;             /* the forward's x_on, gi_on, h_on */
  const float* gi;
  const float* h;
  const float* gchosen;       /* [B][T][A] or NULL */
  const float* gq;            /* [B][T][A][NA] or NULL */
  const float* gh;            /* [B][T][A][H] or NULL */
  float* gh0;                 /* out [B][A][H] or NULL */
  float* gslabs;              /* out [>= t2o_rnn_bwd_slabs][t2o_rnn_param_count] */
  float* work;                /* t2o_rnn_bwd_work_floats floats, 16-byte aligned */
  int64_t work_floats;
  int32_t max_slabs;
  int32_t B, T, Ts, A, OBS, NA, H;
  int32_t last_action, agent_id, act_shift;
  int32_t reserved_;
} t2o_rnn_bwd_args;
int t2o_rnn_bwd(const t2o_rnn_bwd_args* a, void* stream);
int t2o_rnn_bwd_slabs(int B, int T, int A);                  /* T2O_EINVAL on a bad size */
int64_t t2o_rnn_bwd_work_floats(int B, int T, int A, int H);

/* Diagnostic: runs the cross-lane primitives the kernels rely on (4-lane
 * all-reduces via ds_bpermute and via gfx950 permlane swaps, 16-lane DPP row
 * sums, the batched all-reduce) on in[64]; writes 20 x 64 results
 * (tests/test_gpu_primitives.py). */
int t2o_probe_lane_ops(const float* in, float* out, void* stream);

/* Diagnostic: the mixing head's positivity function pos_func (T2O_POS_*,
 * n_transf_mixer.py:95-103) with beta on x[n]: out[0:n] posf, out[n:2n] its
 * derivative, out[2n:4n] the fused value / derivative pair the BPTT kernels
 * evaluate (tests/test_gpu_primitives.py checks them element by element). */
int t2o_probe_posf(const float* x, int n, int pos_func, float beta, float* out, void* stream);

/* Diagnostic: the agent softmax's reduce-scatter / broadcast halves of the batched
 * 4-lane all-reduce, the packed 4-feature dot product and the 8-wide bf16
 * conversion with the bit-pattern ReLU, on in[64]; writes 23 x 64 results
 * (tests/test_gpu_primitives.py). */
int t2o_probe_scatter_ops(const float* in, float* out, void* stream);
/* Diagnostic: MFMA result hand-offs after a fixed number of wait states (inline
 * asm, unpadded by the compiler): a 16x16x4 f32 result stored to LDS / global
 * memory from its AGPRs after 10 or 32 states, a 16x16x32 bf16 result read as
 * srcC by a 16x16x16 bf16 MFMA after 0 / 4 / 32 states and by a 16x16x32 after
 * 0 / 32, then the compiler-built references.  in [nwaves][64][12] floats, out
 * [12][nwaves][64][4] floats (t2o_probe.hip). */
int t2o_probe_xdl_hazards(const float* in, float* out, int nwaves, void* stream);

/* Diagnostic: stale-LDS probes (t2o_probe.hip, tests/test_gpu_stale_lds.py).  Each
 * workgroup takes the full 160 KB of dynamic LDS, so one fits per CU.
 * t2o_probe_lds_fill stores `word` into every 32-bit word of its LDS and exits;
 * t2o_probe_lds_census writes nothing to LDS and stores in out[workgroup] (device,
 * int32[workgroups]) how many words of its allocation differ from `word`. */
int t2o_probe_lds_fill(uint32_t word, int workgroups, void* stream);
int t2o_probe_lds_census(uint32_t word, int workgroups, int32_t* out, void* stream);

/* Diagnostic: the XOR (in bf16 elements, a multiple of 8) applied to the
 * columns of row `row` of a bf16 weight-image matrix with row length ld: element
 * (r, col) of the image sits at r*ld + (col ^ t2o_bf_swz(r, ld)). */
int t2o_bf_swz(int row, int ld);

/* Sum nslab partial gradient slabs [nslab][n] into out[n] (out = sum, overwritten). */
int t2o_reduce_slabs(const float* slabs, int nslab, int64_t n, float* out, void* stream);

/* ---- vectorised MEC-offloading environment -------------
 * Replaces MultiAgvOffloadingEnv (environment_multi_mec.py:12-439) driven by
 * parallel_runner.py's env_worker (:224-270): NE envs advance in lock-step, one
 * wave per env, state resident in HBM.  All arrays but spec are device pointers.
 *
 * mode 0  construction (:12-59: mec_index + positions, zeroed queues/normaliser)
 * mode 1  worker 'reset'  (:257-263 -> reset() :219-227, get_state, get_avail_actions, get_obs)
 * mode 2  worker 'step'   (:239-256 -> step() :309-366, get_state, get_avail_actions, get_obs)
 * mode 3  get_env_info's two get_obs calls (:421-439; normaliser updates only)
 *
 * spec[15] (fp64, host memory): mec_radius, computation_cycles, bandwidth, noise_power,
 *   path_loss, channel_gain_linear, mec_compute_cap, agv_transmit_power,
 *   agv_compute_cap, latency_max, t_length, job_size_min, job_size_max,
 *   job_arrival_p, edge_only (0/1)  (t2omca_amd/env_spec.py).  Entity
 *   observations (obs_entity_mode = True).
 * state[17]: mec_index i32[NE][A], x f64[NE][A], y f64[NE][A],
 *   q_size i32[NE][A][QMAX], q_thr i32[NE][A][QMAX], q_head i32[NE][A],
 *   q_len i32[NE][A], task_num i32[NE][A], task_success i32[NE][A],
 *   remain_delay f64[NE][A], last_ack i32[NE][A], time_slot i32[NE],
 *   draw i64[NE], nrm_n i64[NE], nrm_mean f64[NE][9A], nrm_S f64[NE][9A],
 *   nrm_std f64[NE][9A].
 * out[8] (any entry may be NULL except reward/terminated/info in mode 2):
 *   obs f32[NE][A][9A], obs f64[NE][A][9A], state f32[NE][8A],
 *   avail i32[NE][A][C+1], reward f64[NE], terminated u8[NE],
 *   info f64[NE][6] = delay_reward, overtime_penalty, channel_utilization_rate,
 *   conflict_ratio, task_completion_rate, task_completion_delay (NaN unless terminal),
 *   ack i32[NE][A].
 * actions: i64, env e's agent a at actions[e*act_se + a] (values in 0..C).
 * Limits: A <= 64, M <= 16, C <= 16.  Random draws: env_spec.uniforms(seed, env, draw). */
int t2o_env_run(int mode, const double* spec, void* const* state, void* const* out,
                const int64_t* actions, int64_t act_se, int NE, int A, int M, int C, int QMAX, int T,
                uint64_t seed, void* stream);

/* t2o_env_run with spec[16] (host memory): spec[15] = obs_entity_mode (1: the
 * entity observation [A][9A] above; 0: get_obs_agent's flat branch, :172-182,
 * obs f32/f64[NE][A][6] = [last_ack, get_agent_inf], normalised by the env's
 * 6-long running normaliser, which keeps its [9A] row stride in state[14..16]),
 * and n_out = 8 (as above) or 11 output pointers; the extra three
 * carry the compact observation wire format (replaces storing
 * get_obs's dense [A][9A] output, environment_multi_mec.py:148-186):
 *   out[8]  wire i32[NE][A][4], written with every obs the worker returns
 *           (modes 1, 2): per entity j, w0 = job size, w1 = data_delay,
 *           w2 = offload delay x 100 (exact integer: the fp64 value is
 *           rint(x*100)/100), w3 = thr | qlen << 16 | (ack+1) << 24 | mec << 26;
 *           all zero fields when the queue is empty (get_agent_inf :123-146);
 *   out[9]  snap_n i64[NE], out[10] snap f64[NE][2][9A]: the normaliser's
 *           count, mean and S right before the worker's get_obs in mode 1 (the
 *           state the episode's first returned obs is normalised from).
 * out[9] / out[10] are both set or both NULL.  Needs latency_max <= 65535.
 * The wire format needs entity observations (spec[15] = 1). */
int t2o_env_run_ex(int mode, const double* spec, void* const* state, void* const* out, int n_out,
                   const int64_t* actions, int64_t act_se, int NE, int A, int M, int C, int QMAX, int T,
                   uint64_t seed, void* stream);

/* Dense normalised observations from the wire format: for each episode b,
 * starting from (snap_n[b], snap[b]), replays get_obs's sequential normaliser
 * (normalization.py:12-35, agent by agent, t = 0..T1-1) on the observation
 * get_obs_agent (:148-182) builds from wire[b][t] — bit-identical to the env's
 * own obs output.  wire: int32 element strides w_sb / w_st (multiples of 4,
 * 16-B aligned), rows [A][4] dense; obs: f32 element strides o_sb / o_st, each
 * step a dense [A][9A]; obs64 (optional) dense f64 [B][T1][A][9A].  A <= 64. */
int t2o_obs_expand(const int32_t* wire, int64_t w_sb, int64_t w_st, const int64_t* snap_n, const double* snap,
                   float* obs, int64_t o_sb, int64_t o_st, double* obs64, int B, int T1, int A, void* stream);

/* ε-greedy action selection (the reference's controller is
 * absent, contract parallel_runner.py:121 with PyMARL's EpsilonGreedyActionSelector).
 * q f32 [rows][NA], avail i32 [rows][NA] (rows = envs x agents, dense) ->
 * actions i64 [rows]: argmax of q over available actions (first maximum), or
 * with probability epsilon a uniformly drawn available action.  Draws:
 * u1 = U(seed, row, 2*counter), u2 = U(seed, row, 2*counter+1) of the
 * env_spec.uniforms stream; random action = floor(u2 * n_avail)-th available.
 * NA <= 32. */
int t2o_select_actions(const float* q, const int32_t* avail, int64_t* actions, int64_t rows, int NA,
                       double epsilon, uint64_t seed, int64_t counter, void* stream);

/* Prioritized episode replay (the reference's buffer is
 * absent, contract per_run.py:143-146,216-238, PyMARL2 proportional PER).
 * p f32 [n] = stored priority**alpha of the n valid episodes.  Sample batch
 * indices by stratified proportional search (mass_k = (u_k + k) * Σp / batch,
 * u_k = U(seed, k, counter)) with IS weights (p_i/Σp*n)^-beta normalised by
 * the weight of min p; workspace: t2o_per_workspace_doubles(n) doubles. */
int64_t t2o_per_workspace_doubles(int64_t capacity);
int t2o_per_sample(const float* p, int64_t n, int64_t batch, double beta, uint64_t seed, int64_t counter,
                   double* workspace, int64_t* idx_out, float* w_out, void* stream);
/* p[idx[k]] = (prio[k] + eps)**alpha; *max_prio = max(*max_prio, prio[k] + eps). */
int t2o_per_update(float* p, const int64_t* idx, const float* prio, int64_t n, float alpha, float eps,
                   float* max_prio, void* stream);
/* dst + k*dst_stride <- src + idx[k]*src_stride, row_bytes each (rows <= 65535;
 * copied in the widest of 16/8/4/1-byte units the alignment allows): the
 * episode gather of a sampled batch. */
int t2o_gather_rows(const void* src, int64_t src_stride, const int64_t* idx, int64_t rows, void* dst,
                    int64_t dst_stride, int64_t row_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T2OMCA_H */
