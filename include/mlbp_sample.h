/* mlbp_sample.h -- C ABI of libmlbp_sample.so: posterior sampling of whole assignments for batched factor graphs
 * (AMD Instinct MI355X, gfx950, float64).
 *
 * The fourth library of the engine.  libmlbp.so answers "what is each variable's marginal?", libmlbp_map.so "which whole
 * assignment is most probable?", libmlbp_logz.so "how probable is a given assignment?"; this one DRAWS whole assignments by
 * sequential conditioning on top of sum-product sweeps: draw one variable from its marginal, clamp it, run inference again
 * on the clamped model, draw the next.  On a tree the draws follow the model exactly and the log-probability of a draw equals
 * score - log Z; on a loopy graph they follow a proper distribution q whose log-probability log q(x) is returned exactly for
 * every draw (importance weights with score).  It has its own sources (macaronicusermodeling_amd/csrc_sample/), its own
 * kernel inventory and its own error slot; it shares no state with the other three libraries.
 *
 * Conventions, as in mlbp.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_sample_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory unless stated; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may
 * be captured into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64 kernel's
 * dynamic-LDS limit, a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is
 * no CPU fallback: without a device the compute call returns MLBP_ENODEVICE.  The random numbers come from the caller and the
 * kernels hold no generator: a call is a pure function of its arguments.
 *
 * Semantics of one call.  For each graph g and sample s, start with every variable free.  For step k = 0 .. n_vars-1, with
 * v = order[k]:
 *   1. every message is set uniform;
 *   2. the program's sweeps run as mlbp.h defines sum-product (Gauss-Seidel, op by op):
 *        MLBP_OP_UNARY   {kind, u, -, dst}      dst = renorm(unary row of table unary_tab[g][u])
 *        MLBP_OP_VAR     {kind, first, n, dst}  dst = renorm(clamp(uniform * msgs[srcs[first]] * ...)), nan_to_num after every
 *                                               product; clamp: when the source variable slot_var[dst] is clamped to state x the
 *                                               product is multiplied by the indicator of x (zero elsewhere) before renorm
 *        MLBP_OP_PAIR_TM {kind, p, src, dst}    dst[i] = renorm(sum_j T[i][j] * msgs[src][j]),  T = table pair_tab[g][p]
 *        MLBP_OP_PAIR_MT {kind, p, src, dst}    dst[j] = renorm(sum_i msgs[src][i] * T[i][j])
 *      renorm divides by the sum of the vector (normalize_messages != 0); a total that is not positive gives the uniform
 *      message;
 *   3. m = renorm(uniform * msgs[in_slots[in_off[v]]] * ...), nan_to_num after every product, always normalised;
 *   4. x_v = given[g][v] when that is >= 0; otherwise, with c_i the inclusive prefix sum of m in index order,
 *      u = uniforms[s][g][k] and t = u * c_{X-1}:  x_v = the lowest i with c_i > t; when there is none, the highest i with
 *      m_i > 0.  A state of probability zero is never drawn -- except from the empty marginal: when no state has m_i > 0 (every
 *      m_i is 0: with unnormalised messages a +inf table entry survives as DBL_MAX and the total of step 3 overflows),
 *      x_v = 0 and, by step 5, logq = -inf; the later variables are drawn as usual;
 *   5. logq += log m[x_v]  (natural log; -inf for a given state of probability zero, after which step 2's renorm rule makes
 *      the emptied messages uniform);
 *   6. v is clamped to x_v.
 * Every step restarts from uniform messages, so step k is one sum-product call with init_messages on the clamped model.
 * Step 0 does not depend on s: a kernel may compute its m once per graph; the bits are those of computing it per sample.
 * Outputs: samples[s][g][v] = x_v (v in variable-index order), logq[s][g], and optionally cond_marginals[s][g][v][.] = the m
 * variable v was drawn from.
 */
#ifndef MLBP_SAMPLE_H
#define MLBP_SAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes and op kinds: the values of mlbp.h.  A translation unit that uses both headers includes mlbp.h first. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H) && !defined(MLBP_LOGZ_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
enum { MLBP_OP_UNARY = 0, MLBP_OP_PAIR_TM = 1, MLBP_OP_PAIR_MT = 2, MLBP_OP_VAR = 3 };
#endif

/* Which kernel a call enqueues -- a function of (X, n_msgs, n_vars) alone, never a user option:
 *   MLBP_SAMPLE_KERNEL_X64      X == 64 and the graph fits the kernel's LDS budget:
 *                                 n_msgs * 512  (messages)  +  4608  (partial sums and one raw vector)
 *                                 +  512  (the cached marginal of step 0; the draw itself lives in registers)
 *                                 +  4 * round_up(n_vars, 4)  (the clamp state of every variable)  <=  MLBP_SAMPLE_X64_LDS_BYTES
 *                               i.e. up to 149 message slots: two workgroups share a CU's 160 KB.  Messages stay in LDS for the
 *                               whole launch; with P <= 3 the pairwise tables stay in registers (read once per workgroup
 *                               however many steps and samples follow), beyond that they are streamed per update.
 *   MLBP_SAMPLE_KERNEL_GENERIC  every other shape (2 <= X <= 1024): messages in the caller's workspace, tables streamed.
 * mlbp_sample_pick_kernel states the rule (host only).
 *
 * Both kernels run on a grid of (B, C) workgroups, C = mlbp_sample_chunks(B, S) = min(S, ceil(MLBP_SAMPLE_MIN_WORKGROUPS / B)):
 * workgroup (g, c) serves graph g and draws its samples c, c + C, ...  MLBP_SAMPLE_MIN_WORKGROUPS = 256 CUs x the two
 * workgroups a CU's 160 KB holds at the LDS budget: a large batch reads every table once whatever S is, a small one spreads
 * its samples over the machine. */
#define MLBP_SAMPLE_KERNEL_NONE 0
#define MLBP_SAMPLE_KERNEL_X64 1
#define MLBP_SAMPLE_KERNEL_GENERIC 2
#define MLBP_SAMPLE_X64_LDS_BYTES 81920
#define MLBP_SAMPLE_MAX_X 1024
#define MLBP_SAMPLE_MIN_WORKGROUPS 512

typedef struct mlbp_sample_args {
  int32_t B, X, n_msgs, P, U, n_vars;        /* graphs, states, message slots, pairwise / unary factors, variables */
  int32_t n_ops, n_srcs, n_sweeps;
  int32_t n_pair_tables, n_unary_tables;
  int32_t normalize_messages;
  int32_t S;                                 /* samples per graph */
  const int32_t* ops;                        /* device [n_ops][4], validated by mlbp_sample_check_program before upload */
  const int32_t* srcs;                       /* device [n_srcs] (may be NULL when n_srcs == 0) */
  const int32_t* sweeps;                     /* device [n_sweeps][2] = {first op, count} */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const int32_t* in_off;                     /* device [n_vars + 1], validated by mlbp_sample_check_readout */
  const int32_t* in_slots;                   /* device [in_off[n_vars]] incoming factor->variable slots, facset order */
  const int32_t* slot_var;                   /* device [n_msgs]: source variable of a variable->factor slot, -1 otherwise */
  const int32_t* order;                      /* device [n_vars]: a permutation of the variable indices; step k handles order[k] */
  const double* uniforms;                    /* device [S][B][n_vars], each in [0, 1), indexed by step */
  const int32_t* given;                      /* optional device [B][n_vars]: a state in [0, X) fixes the variable, -1 draws it */
  double* workspace;                         /* device, workspace_bytes >= mlbp_sample_workspace_bytes(...): the generic
                                                kernel's messages [B * C][n_msgs][X]; may be NULL on the X = 64 kernel */
  int64_t workspace_bytes;
  int32_t* samples;                          /* device [S][B][n_vars] */
  double* logq;                              /* device [S][B] */
  double* cond_marginals;                    /* optional device [S][B][n_vars][X] */
} mlbp_sample_args;

/* Table indices and `given` are device data and are not checked on the host.  A graph that names a table outside
 * [0, n_pair_tables) / [0, n_unary_tables), or whose `given` holds a value outside [-1, X), is not computed: its samples are
 * -1 everywhere, its logq NaN, its cond_marginals are left as they were. */
int mlbp_sample_f64(const mlbp_sample_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_map_check_program (op kinds; destination, source, table-slot and srcs ranges;
 * sweep ranges) and: every MLBP_OP_VAR destination has slot_var in [0, n_vars), every other destination has slot_var -1,
 * order is a permutation of 0 .. n_vars-1.  Host arrays. */
int mlbp_sample_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                              int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int32_t n_vars, const int32_t* slot_var,
                              const int32_t* order);

/* Host only: validates the read-out arrays (in_off monotone from 0, in_slots < n_msgs).  Host arrays. */
int mlbp_sample_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs);

/* Host only: MLBP_SAMPLE_KERNEL_X64 or MLBP_SAMPLE_KERNEL_GENERIC by the rule above; MLBP_EUNSUPPORTED for
 * X > MLBP_SAMPLE_MAX_X, MLBP_EINVAL for X < 2 or non-positive sizes. */
int mlbp_sample_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars);

/* Host only: C of the grid (B, C) by the rule above; MLBP_EINVAL for non-positive B or S. */
int mlbp_sample_chunks(int32_t B, int32_t S);

/* Host only: bytes of workspace a call needs -- 0 on the X = 64 kernel, B * C * n_msgs * X * 8 on the generic kernel; a
 * negative status as mlbp_sample_pick_kernel / mlbp_sample_chunks give it. */
int64_t mlbp_sample_workspace_bytes(int32_t B, int32_t S, int32_t X, int32_t n_msgs, int32_t n_vars);

/* Host-side record of the kernel the calling thread's last mlbp_sample_f64 enqueued (MLBP_SAMPLE_KERNEL_*; NONE when it was
 * refused before the launch). */
int mlbp_sample_last_kernel(void);

const char* mlbp_sample_arch(void);          /* "gfx950" */
const char* mlbp_sample_last_error(void);    /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
