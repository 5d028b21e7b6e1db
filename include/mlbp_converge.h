/* mlbp_converge.h -- C ABI of libmlbp_converge.so: sum-product sweeps run to convergence, with a per-graph residual and a
 * per-graph early exit inside one launch (AMD Instinct MI355X, gfx950, float64); the same for max-product sweeps, with the
 * decoded assignment, as a mode of the one compute call.
 *
 * The fifth library of the engine.  libmlbp.so, libmlbp_map.so, libmlbp_logz.so and libmlbp_sample.so all run a FIXED number
 * of sweeps; none tells the caller whether the messages it reads are at a fixed point.  This one repeats the program's sweeps
 * until no message entry moves by more than `tol`, graph by graph, and reports how many rounds that took and the last
 * residual.  It has its own sources (macaronicusermodeling_amd/csrc_converge/), its own kernel inventory and its own error
 * slot; it shares no state with the other four libraries.
 *
 * Conventions, as in mlbp_sample.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_converge_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be captured
 * into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64 kernel's dynamic-LDS
 * limit, a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is no CPU
 * fallback: without a device the compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, for each graph g on its own:
 *   0. init_messages != 0: every message is set uniform; 0: the call continues from what `msgs` holds.
 *   1. A ROUND runs the program's sweeps in order.  The updates are Gauss-Seidel, op by op, with the sum-product rules of
 *      mlbp_sample.h step 2 with no variable clamped:
 *        MLBP_OP_UNARY   {kind, u, -, dst}      dst = renorm(unary row of table unary_tab[g][u])
 *        MLBP_OP_VAR     {kind, first, n, dst}  dst = renorm(uniform * msgs[srcs[first]] * ...), nan_to_num after every product
 *        MLBP_OP_PAIR_TM {kind, p, src, dst}    dst[i] = renorm(sum_j T[i][j] * msgs[src][j]),  T = table pair_tab[g][p]
 *        MLBP_OP_PAIR_MT {kind, p, src, dst}    dst[j] = renorm(sum_i msgs[src][i] * T[i][j])
 *      renorm divides by the sum of the vector; a total that is not positive gives the uniform message.  normalize_messages
 *      must be non-zero: a residual on unnormalised messages has no scale, and the call is refused with MLBP_EINVAL.
 *   2. For every update, delta = max_i |new_i - old_i|, where old is the slot's content immediately before the update.  The
 *      RESIDUAL of a round is the maximum of delta over all updates of the round.  With finite non-negative tables every
 *      message entry is a finite number in [0, 1].  A +inf table entry can leave inf / inf = NaN in one entry of a
 *      factor->variable message (the next product's nan_to_num removes it).  Such an entry is compared like this: NaN before
 *      and after the update has not moved (its difference is 0); NaN on one side only counts as +inf.
 *   3. After each round: residual <= tol stops the graph; otherwise it runs the next round, up to max_rounds.
 * Outputs per graph: rounds[g] (the rounds run, at least 1), residual[g] (the last round's), the final messages in `msgs`,
 * optionally marginals[g][v][.] = renorm(uniform * msgs[in_slots[in_off[v]]] * ...) (nan_to_num after every product, always
 * normalised) and history[g][r] = the residual of round r for r < rounds[g], -1.0 beyond.
 * A UNARY update writes the same value every time.  After the first round of a call the X = 64 kernel skips a UNARY op when
 * every op of the program that names its destination slot is a UNARY op of the same unary slot -- it establishes that from the
 * op list itself at the start of the launch, for programs of up to 2048 ops.  The bits and the residuals are those of running
 * the op.  The generic kernel runs every op of every round.
 *
 * MAX-PRODUCT MODE (max_product != 0): every round runs with the update rules of mlbp_map.h -- a pairwise update takes max_j
 * (max_i) where step 1 takes sum_j (sum_i); the maximum is fmax, which ignores a NaN entry; renorm still divides by the sum of
 * the vector.  Steps 0, 2 and 3, rounds, residual, history, the X = 64 unary skip and the refusal of a graph with a table index
 * out of range are as above, and `marginals` returns the same normalised product of the incoming messages, which is now the
 * max-marginal.  Max-product need not settle: a graph that oscillates runs max_rounds rounds and says so in its residual.
 * With `assignment` and `score` the call also decodes from the final messages, the read-out of mlbp_map.h:
 *   assignment[g][v] = the argmax of v's max-marginal, ties to the lowest index;
 *   score[g]         = sum over factors of log(table entry at the assignment), the tables as given,
 * bit for bit what mlbp_map_sweep_f64 returns from the same messages.  pair_axis_var and unary_var are device data: a call whose
 * arrays name a variable outside [0, n_vars) computes no graph (every graph is refused, below).  A refused graph gets
 * assignment -1 and score NaN beside rounds -1 and residual NaN.
 * Host checks of the new fields, all MLBP_EINVAL: with max_product, `assignment` without `score` or the reverse; either of them
 * with P > 0 and pair_axis_var NULL, or with U > 0 and unary_var NULL; `assignment` or `score` without max_product (this last
 * one is looked at once a device is known to be there: without one the call returns MLBP_ENODEVICE as it always did).  All of
 * the new fields zero or NULL is the sum-product call above, every bit as it was.
 */
#ifndef MLBP_CONVERGE_H
#define MLBP_CONVERGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes and op kinds: the values of mlbp.h.  A translation unit that uses several headers includes mlbp.h first. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H) && !defined(MLBP_LOGZ_H) && !defined(MLBP_SAMPLE_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
enum { MLBP_OP_UNARY = 0, MLBP_OP_PAIR_TM = 1, MLBP_OP_PAIR_MT = 2, MLBP_OP_VAR = 3 };
#endif

/* Which kernel a call enqueues -- a function of (X, n_msgs) alone (n_vars is accepted for symmetry with the other
 * libraries and checked to be positive), never a user option:
 *   MLBP_CONVERGE_KERNEL_X64      X == 64 and the graph fits the kernel's LDS budget:
 *                                   n_msgs * 512  (messages)  +  4608  (partial sums and one raw vector)
 *                                   +  8  (the residual word)  <=  MLBP_CONVERGE_X64_LDS_BYTES
 *                                 i.e. up to 150 message slots: two workgroups share a CU's 160 KB.  256 threads, one workgroup
 *                                 per graph, messages in LDS for the whole launch; with P <= 3 the pairwise tables stay in
 *                                 registers for the whole launch, beyond that they are streamed per update.
 *   MLBP_CONVERGE_KERNEL_GENERIC  every other shape (2 <= X <= 1024): one workgroup per graph, messages in `msgs` in place,
 *                                 tables streamed.
 * In both, the stop decision is workgroup-uniform: the round's residual goes through one LDS word that every thread reads
 * behind a barrier, so a graph leaves the round loop as a whole and costs its neighbours nothing. */
#define MLBP_CONVERGE_KERNEL_NONE 0
#define MLBP_CONVERGE_KERNEL_X64 1
#define MLBP_CONVERGE_KERNEL_GENERIC 2
#define MLBP_CONVERGE_X64_LDS_BYTES 81920
#define MLBP_CONVERGE_MAX_X 1024
#define MLBP_CONVERGE_MAX_ROUNDS 65535

typedef struct mlbp_converge_args {
  int32_t B, X, n_msgs, P, U, n_vars;        /* graphs, states, message slots, pairwise / unary factors, variables */
  int32_t n_ops, n_srcs, n_sweeps;
  int32_t n_pair_tables, n_unary_tables;
  int32_t normalize_messages;                /* must be non-zero */
  int32_t init_messages;                     /* non-zero: start from uniform messages; 0: continue from `msgs` */
  int32_t max_rounds;                        /* 1 .. MLBP_CONVERGE_MAX_ROUNDS: a launch always terminates */
  double tol;                                /* finite, >= 0; 0 stops only at an exact fixed point */
  const int32_t* ops;                        /* device [n_ops][4], validated by mlbp_converge_check_program before upload */
  const int32_t* srcs;                       /* device [n_srcs] (may be NULL when n_srcs == 0) */
  const int32_t* sweeps;                     /* device [n_sweeps][2] = {first op, count} */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const int32_t* in_off;                     /* device [n_vars + 1], validated by mlbp_converge_check_readout */
  const int32_t* in_slots;                   /* device [in_off[n_vars]] incoming factor->variable slots, facset order */
  double* msgs;                              /* device [B][n_msgs][X], in/out */
  int32_t* rounds;                           /* device [B] */
  double* residual;                          /* device [B] */
  double* marginals;                         /* optional device [B][n_vars][X] */
  double* history;                           /* optional device [B][max_rounds] */
  int32_t max_product;                       /* non-zero: the rounds run max-product (see above); 0: sum-product */
  int32_t* assignment;                       /* optional device [B][n_vars]; max_product only, together with score */
  double* score;                             /* optional device [B] */
  const int32_t* pair_axis_var;              /* device [P][2] variable index on table axis 0 / 1 (with assignment, P > 0) */
  const int32_t* unary_var;                  /* device [U] variable index of every unary factor (with assignment, U > 0) */
} mlbp_converge_args;

/* Table indices are device data and are not checked on the host.  A graph that names a table outside [0, n_pair_tables) /
 * [0, n_unary_tables) is not computed: rounds = -1, residual = NaN, its history row all NaN, its messages and marginals left
 * as they were. */
int mlbp_converge_f64(const mlbp_converge_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_map_check_program (op kinds; destination, source, table-slot and srcs ranges;
 * sweep ranges) and: every message slot is the destination of at least one op of the round (an op inside a sweep's range).
 * A slot nobody updates gets MLBP_EINVAL naming it: the residual would say nothing about it.  Host arrays. */
int mlbp_converge_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                                int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U);

/* Host only: validates the read-out arrays (in_off monotone from 0, in_slots < n_msgs).  Host arrays. */
int mlbp_converge_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs);

/* Host only: MLBP_CONVERGE_KERNEL_X64 or MLBP_CONVERGE_KERNEL_GENERIC by the rule above; MLBP_EUNSUPPORTED for
 * X > MLBP_CONVERGE_MAX_X, MLBP_EINVAL for X < 2 or non-positive sizes. */
int mlbp_converge_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars);

/* Host-side record of the kernel the calling thread's last mlbp_converge_f64 enqueued (MLBP_CONVERGE_KERNEL_*; NONE when it
 * was refused before the launch). */
int mlbp_converge_last_kernel(void);

const char* mlbp_converge_arch(void);          /* "gfx950" */
const char* mlbp_converge_last_error(void);    /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
