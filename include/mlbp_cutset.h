/* mlbp_cutset.h -- C ABI of libmlbp_cutset.so: the model's TRUE marginals and log Z of batched factor graphs by cutset
 * conditioning (AMD Instinct MI355X, gfx950, float64).
 *
 * The sixth library of the engine.  The other five run loopy belief propagation: on a graph with a cycle their marginals and
 * log Z are the loopy-BP / Bethe values.  This one sums the model itself,
 *     p(x)  ~  prod_u U_u[x_var(u)]  *  prod_p T_p[x_a][x_b]          (a = the variable on axis 0 of pairwise factor p),
 * so that the distance of those values from the truth can be reported.  It has its own source
 * (macaronicusermodeling_amd/csrc_cutset/), its own kernel inventory (cutset_*) and its own error slot; it shares no state
 * with the other libraries.  It runs no sweep program and reads no messages.
 *
 * Conventions, as in mlbp_sample.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_cutset_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device memory
 * unless stated; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be
 * captured into a HIP graph and replayed (after one eager call: the first call on a device raises the kernels' dynamic-LDS
 * limit, a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is no CPU
 * fallback: without a device the compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, per graph.  The host passes a CUTSET C of variables such that the pairwise factors among the
 * remaining FREE variables form a forest (mlbp_cutset_check_plan).  A configuration c in [0, X^|C|) fixes cutset variable
 * cutset[q] to state s_q = (c / X^q) mod X.  Under c the model is conditioned the way the reference treats given words:
 *   - a pairwise factor between a cutset variable and a free variable becomes the row or column of its table at s_q, a
 *     vector on the free variable;
 *   - a pairwise factor inside C and a unary factor on a cutset variable become constants.
 * The conditioned model is a forest and is solved exactly: one pass from the leaves to the roots gives Z_c (the product of
 * the constants and of every tree's total), one pass back gives every free variable's conditional marginal m_c.  Then
 *   Z                 = sum_c Z_c                          log_z = ln Z
 *   free variable v:    marginal[v] = sum_c Z_c m_c[v] / Z
 *   cutset variable a:  marginal[a][s] = sum_{c : s_a = s} Z_c / Z      (under c a cutset variable is the indicator of its
 *                                                                        state, unconditionally: no uniform rule)
 *   score             = sum over pairwise p of log T_p[x_a][x_b] + sum over unary u of log U_u[x_v]   at x = labels
 *   joint_logp        = score - log_z                      (the score of mlbp_map.h and mlbp_logz.h)
 * Any valid cutset gives the same values up to rounding; the empty cutset on a forest is the exact two-pass algorithm.
 *
 * Range.  Nothing is rescaled but by powers of two, by exponent extraction: every table is used as table * 2^-e with e the
 * exponent of its largest entry; a free variable's vector (the product of its factors' rows and its children's messages), every
 * message and every total is brought back to a largest entry in [1, 2) the same way, and the exponents are tallied in an
 * integer.  Z_c, the partial sums and Z are (mantissa, exponent) pairs through both combine steps; ln is taken once, at the
 * end.  So a table times 2^k (|k| <= 400, tables of normal magnitude) changes no bit of the marginals and moves log_z by
 * k ln 2.  The limit: a free variable's vector is a plain product of rescaled rows before it is rescaled; with dozens of unary
 * factors of 170 decades each on one variable the entries that carry Z can leave the normal range.
 *
 * Edge rules.  Z = 0 (an all-zero table, say): log_z = -inf and every marginal row is uniform 1/X.  A NaN or +inf entry:
 * log_z of that graph is not a finite number, its marginals are unspecified; the call returns and every other graph keeps its
 * bits.  A table index outside its array: the graph is not computed -- log_z (score, joint_logp) NaN, its marginals left as
 * they were.  A label outside [0, X): score and joint_logp NaN; log_z and the marginals are computed.
 *
 * The plan.  One packed int32 array, host-made (cutset.py documents the derivation), validated by mlbp_cutset_check_plan and
 * uploaded:
 *   words 0..15  header: {n_vars, P, U, n_cut, n_free, n_items, n_consts, n_forest, 0...}
 *   cutset  [n_cut]         variable indices; digit q of a configuration is the state of cutset[q]
 *   order   [n_free]        the free variables in elimination order: every variable before its parent
 *   parent  [n_vars][2]     {pairwise factor to the parent, parent variable}; {-1, -1} for a root and for a cutset variable
 *   item_off[n_vars + 1]    per free variable, its range in items (empty for cutset variables)
 *   items   [n_items][3]    {MLBP_CUTSET_ITEM_UNARY, u, 0}: unary factor u on the variable;
 *                           {MLBP_CUTSET_ITEM_COL, p, q}: factor p holds the variable on axis 0 and cutset[q] on axis 1;
 *                           {MLBP_CUTSET_ITEM_ROW, p, q}: the variable on axis 1, cutset[q] on axis 0
 *   consts  [n_consts][4]   {MLBP_CUTSET_CONST_UNARY, u, q, -1}: unary factor u on cutset[q];
 *                           {MLBP_CUTSET_CONST_PAIR, p, q0, q1}: factor p on cutset[q0] (axis 0) and cutset[q1] (axis 1)
 *   pair_axis_var[P][2]     the variable on table axis 0 / 1 of every pairwise factor
 *   unary_var[U]
 *   forest_slot[P]          0 .. n_forest-1 for the parent factors in `order` order, -1 for every other factor
 * n_forest = the number of parent factors = n_free - (number of roots).
 *
 * The cutset is chosen on the host (cutset.choose in Python), deterministically: while the multigraph of pairwise factors
 * over the variables not yet chosen has a cycle, take its 2-core (repeatedly drop variables of degree <= 1) and move the core
 * variable of highest degree into C.  Degree counts factors, so two factors over one pair are a cycle; ties go to the lowest
 * position in var_ids.  K_n gives the first n - 2 variables, a ring its first variable, a tree the empty set.
 */
#ifndef MLBP_CUTSET_H
#define MLBP_CUTSET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: the values of mlbp.h.  A translation unit that uses several headers includes this one last. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H) && !defined(MLBP_LOGZ_H) && !defined(MLBP_SAMPLE_H) && !defined(MLBP_CONVERGE_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
#endif

/* Which kernel a call enqueues -- a function of (X, n_vars, P, U, n_forest) alone, never a user option.  Both keep P + U + 16
 * integers (the exponent of every factor's table) on chip, INTS = 4 * round_up(P + U + 16, 4) bytes:
 *   MLBP_CUTSET_KERNEL_X64      X == 64 and
 *                                 n_forest * 33280  (the forest's tables, rescaled once, rows padded to 65 entries, on chip for
 *                                                    the whole launch)
 *                                 + 21 * n_vars * 512  (the product of every variable's unary rows, and for each of the four
 *                                                       waves: the accumulated marginals, every free variable's own factors
 *                                                       under the configuration, its vector on the way up, its message to
 *                                                       its parent, its parent's message to it)
 *                                 + 64  +  INTS   <=   MLBP_CUTSET_X64_LDS_BYTES
 *                               i.e. K3, K4 and a chain of three (two tables) fit, a chain of four does not; K3 and K4 take
 *                               under 80 KB, so two workgroups share a CU's 160 KB.  Every WAVE walks configurations of its
 *                               own, lane = state, without a workgroup barrier.  Cutset-incident rows and columns are fetched
 *                               per configuration.
 *   MLBP_CUTSET_KERNEL_GENERIC  every other shape (2 <= X <= 1024): the workgroup walks one configuration at a time, tables
 *                               streamed; its 5 n_vars + 2 vectors of X entries (the above and two scratch vectors) in LDS when
 *                                 (5 n_vars + 2) * round_up(X, 2) * 8  +  64  +  INTS  <=  MLBP_CUTSET_GENERIC_LDS_BYTES,
 *                               else in the caller's workspace (64 + INTS beyond the budget: MLBP_EUNSUPPORTED).
 * mlbp_cutset_pick_kernel states the rule (host only).
 *
 * Both run on a grid of (B, C) workgroups, C = mlbp_cutset_chunks(B, n_configs) =
 * min(n_configs, ceil(MLBP_CUTSET_MIN_WORKGROUPS / B)).  Workgroup (g, k) of the generic kernel walks configurations k, k + C,
 * ... of graph g and writes one partial -- {sum of Z_c mantissas, exponent, the accumulated marginal mantissas [n_vars][X]} --
 * to the workspace; wave w of workgroup (g, k) of the X = 64 kernel walks 4 k + w, 4 k + w + 4 C, ... and writes partial
 * 4 k + w.  cutset_combine_kernel, one workgroup per graph, adds the C (4 C) partials in index order and writes the outputs.
 * A large batch reads every table once, a small one spreads its configurations over the machine.  The bits of a graph's
 * results are a function of the graph and of C. */
#define MLBP_CUTSET_KERNEL_NONE 0
#define MLBP_CUTSET_KERNEL_X64 1
#define MLBP_CUTSET_KERNEL_GENERIC 2
#define MLBP_CUTSET_X64_LDS_BYTES 131072
#define MLBP_CUTSET_GENERIC_LDS_BYTES 65536
#define MLBP_CUTSET_MAX_X 1024
#define MLBP_CUTSET_MAX_CONFIGS 65536
#define MLBP_CUTSET_MIN_WORKGROUPS 512
#define MLBP_CUTSET_PLAN_HEADER 16

#define MLBP_CUTSET_ITEM_UNARY 0
#define MLBP_CUTSET_ITEM_COL 1
#define MLBP_CUTSET_ITEM_ROW 2
#define MLBP_CUTSET_CONST_UNARY 0
#define MLBP_CUTSET_CONST_PAIR 1

typedef struct mlbp_cutset_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_cutset_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_cutset_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const int32_t* labels;                     /* optional device [B][n_vars]; needed by score and joint_logp */
  double* workspace;                         /* device, workspace_bytes >= mlbp_cutset_workspace_bytes(...) */
  int64_t workspace_bytes;
  double* log_z;                             /* device [B] */
  double* marginals;                         /* device [B][n_vars][X] */
  double* score;                             /* optional device [B] */
  double* joint_logp;                        /* optional device [B] */
} mlbp_cutset_args;

/* Table indices and labels are device data and are not checked on the host: see the edge rules above. */
int mlbp_cutset_f64(const mlbp_cutset_args* args, void* stream);

/* Host only, no GPU needed: validates a packed plan (host array) for X states so that no launch can index outside a buffer and
 * the factors are each used once.  Refuses with MLBP_EINVAL: a header that disagrees with n_words; cutset entries out of range
 * or repeated; an `order` that is not the free variables once each; a parent link whose factor does not join the variable and
 * its parent or whose parent does not come later; a remainder (the pairwise factors among free variables) with a cycle -- the
 * message names the cycle's variables; items and consts whose factor, cut position or kind disagrees with pair_axis_var /
 * unary_var, or that leave a factor out or use it twice; a forest_slot that is not the numbering above.  X^n_cut above
 * MLBP_CUTSET_MAX_CONFIGS (formed in 64 bits) and X > MLBP_CUTSET_MAX_X: MLBP_EUNSUPPORTED. */
int mlbp_cutset_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: MLBP_CUTSET_KERNEL_X64 or _GENERIC by the rule above; MLBP_EUNSUPPORTED for X > MLBP_CUTSET_MAX_X or integers
 * beyond the LDS budget, MLBP_EINVAL for X < 2, n_vars <= 0 or negative sizes. */
int mlbp_cutset_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest);

/* Host only: C of the grid (B, C) by the rule above; MLBP_EINVAL for non-positive arguments. */
int mlbp_cutset_chunks(int32_t B, int32_t n_configs);

/* Host only: bytes of workspace a call needs -- B * C * (n_vars * X + 2) * 8 for the partials of the generic kernel, four times
 * that on the X = 64 kernel, plus B * C * (5 n_vars + 2) * round_up(X, 2) * 8 when the generic kernel keeps its vectors there; n_configs = X^n_cut; a negative
 * status as mlbp_cutset_pick_kernel / mlbp_cutset_chunks give it, MLBP_EUNSUPPORTED above MLBP_CUTSET_MAX_CONFIGS. */
int64_t mlbp_cutset_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut);

/* Host-side record of the kernel the calling thread's last mlbp_cutset_f64 enqueued (MLBP_CUTSET_KERNEL_*; NONE when it was
 * refused before the launch). */
int mlbp_cutset_last_kernel(void);

const char* mlbp_cutset_arch(void);          /* "gfx950" */
const char* mlbp_cutset_last_error(void);    /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
