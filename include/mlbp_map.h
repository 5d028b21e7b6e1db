/* mlbp_map.h -- C ABI of libmlbp_map.so: max-product sweeps and MAP decoding for batched factor graphs
 * (AMD Instinct MI355X, gfx950, float64).
 *
 * The second library of the engine.  libmlbp.so (mlbp.h) answers "what is each variable's marginal?" with sum-product
 * sweeps; this one runs the same compiled schedule with one operator changed -- a pairwise update takes
 * max_j T[i][j] * m[j] instead of sum_j -- and reads the jointly most probable assignment out of the max-marginals.
 * It has its own sources (macaronicusermodeling_amd/csrc_map/), its own kernel inventory and its own error slot; it
 * shares no state with libmlbp.so.
 *
 * Conventions, as in mlbp.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_map_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory unless stated; a compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it
 * may be captured into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64
 * kernel's dynamic-LDS limit, a host-side attribute call); arguments are checked on the host before anything is
 * enqueued.  There is no CPU fallback: without a device a compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call (FactorGraph.treelike_inference with max in place of sum, then the read-out):
 *   for each sweep s, for each op of sweeps[s] in order (Gauss-Seidel: every update sees the latest messages)
 *     MLBP_OP_UNARY   {kind, u, -, dst}      dst = renorm(unary row of table unary_tab[g][u])
 *     MLBP_OP_VAR     {kind, first, n, dst}  dst = renorm(uniform * msgs[srcs[first]] * ... ), nan_to_num after every product
 *     MLBP_OP_PAIR_TM {kind, p, src, dst}    dst[i] = renorm(max_j T[i][j] * msgs[src][j]),  T = table pair_tab[g][p]
 *     MLBP_OP_PAIR_MT {kind, p, src, dst}    dst[j] = renorm(max_i msgs[src][i] * T[i][j])
 *   renorm divides by the SUM of the vector (normalize_messages != 0); a total that is not positive gives the uniform
 *   message.  Dividing by the sum changes no argmax and keeps normalize_messages meaning what it means in mlbp.h.
 *   max-marginal of variable v = renorm(uniform * msgs[in_slots[in_off[v]]] * ...), nan_to_num after every product,
 *   always normalised;  assignment[v] = its argmax, ties to the LOWEST index;
 *   score = sum over pairwise factors p of log T_p[x[pair_axis_var[p][0]]][x[pair_axis_var[p][1]]]
 *         + sum over unary factors u of log row_u[x[unary_var[u]]]      (natural log, tables as given).
 * A maximum ignores NaN table entries (fmax); potentials are exp(.) and never NaN.  The maximum over a row or column that
 * holds no entry other than NaN is unspecified (NaN or -inf, by kernel); with normalize_messages != 0 either has no positive
 * total and gives the uniform message.
 */
#ifndef MLBP_MAP_H
#define MLBP_MAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes and op kinds: the values of mlbp.h.  A translation unit that uses both headers includes mlbp.h first. */
#ifndef MLBP_H
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
enum { MLBP_OP_UNARY = 0, MLBP_OP_PAIR_TM = 1, MLBP_OP_PAIR_MT = 2, MLBP_OP_VAR = 3 };
#endif

/* Which kernel a call enqueues -- a function of (X, n_msgs, n_vars) alone, never a user option:
 *   MLBP_MAP_KERNEL_X64      X == 64 and the graph's messages fit the kernel's LDS budget:
 *                              n_msgs * 512  (messages)  +  4608  (partial maxima and one raw vector)
 *                              +  4 * round_up(n_vars, 4)  (the assignment)   <=   MLBP_MAP_X64_LDS_BYTES
 *                            i.e. up to 150 message slots (151 slots and the assignment make 81 936 bytes): two workgroups
 *                            share a CU's 160 KB.  Messages stay in LDS for the
 *                            whole launch; with P <= 3 the pairwise tables stay in registers (read once per launch),
 *                            beyond that they are streamed per update.
 *   MLBP_MAP_KERNEL_GENERIC  every other shape (2 <= X <= 1024): messages in global memory, tables streamed.
 * mlbp_map_pick_kernel states the rule (host only). */
#define MLBP_MAP_KERNEL_NONE 0
#define MLBP_MAP_KERNEL_X64 1
#define MLBP_MAP_KERNEL_GENERIC 2
#define MLBP_MAP_X64_LDS_BYTES 81920
#define MLBP_MAP_MAX_X 1024

typedef struct mlbp_map_args {
  int32_t B, X, n_msgs, P, U, n_vars;        /* graphs, states, message slots, pairwise / unary factors, variables */
  int32_t n_ops, n_srcs, n_sweeps;
  int32_t n_pair_tables, n_unary_tables;
  int32_t init_messages;                     /* != 0: start from uniform messages (FactorGraph.initialize fused) */
  int32_t normalize_messages;
  int32_t write_messages;                    /* != 0: msgs holds the final messages on return; 0: its contents are undefined */
  const int32_t* ops;                        /* device [n_ops][4], validated by mlbp_map_check_program before upload */
  const int32_t* srcs;                       /* device [n_srcs] (may be NULL when n_srcs == 0) */
  const int32_t* sweeps;                     /* device [n_sweeps][2] = {first op, count} */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  double* msgs;                              /* device [B][n_msgs][X], in/out.  May be NULL on the X = 64 kernel when
                                                init_messages != 0 and write_messages == 0; the generic kernel keeps its
                                                messages there and always needs it. */
  const int32_t* in_off;                     /* device [n_vars + 1], validated by mlbp_map_check_readout */
  const int32_t* in_slots;                   /* device [in_off[n_vars]] incoming factor->variable slots, facset order */
  const int32_t* pair_axis_var;              /* device [P][2] variable on table axis 0 / 1 (NULL when P == 0) */
  const int32_t* unary_var;                  /* device [U] (NULL when U == 0) */
  double* max_marginals;                     /* optional device [B][n_vars][X] */
  int32_t* assignment;                       /* optional device [B][n_vars] */
  double* score;                             /* optional device [B] */
} mlbp_map_args;

/* Table indices are device data and are not checked on the host.  A graph that names a table outside
 * [0, n_pair_tables) / [0, n_unary_tables) is not computed: its assignment is -1 everywhere, its score NaN, its
 * messages and max-marginals are left as they were.  (The Python layer refuses such indices before upload.) */
int mlbp_map_sweep_f64(const mlbp_map_args* args, void* stream);

/* Host only, no GPU needed: validates an op list (op kinds; destination, source, table-slot and srcs ranges; sweep
 * ranges) so that no launch can index outside msgs, srcs, pair_tab or unary_tab.  Host arrays. */
int mlbp_map_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                           int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U);

/* Host only: validates the read-out arrays (in_off monotone from 0, in_slots < n_msgs, pair_axis_var / unary_var <
 * n_vars).  Host arrays; pair_axis_var may be NULL when P == 0, unary_var when U == 0. */
int mlbp_map_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, int32_t P,
                           const int32_t* pair_axis_var, int32_t U, const int32_t* unary_var);

/* Host only: MLBP_MAP_KERNEL_X64 or MLBP_MAP_KERNEL_GENERIC by the rule above; MLBP_EUNSUPPORTED for X > MLBP_MAP_MAX_X,
 * MLBP_EINVAL for X < 2 or non-positive sizes. */
int mlbp_map_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars);

/* Host-side record of the kernel the calling thread's last mlbp_map_sweep_f64 enqueued (MLBP_MAP_KERNEL_*; NONE when it
 * was refused before the launch). */
int mlbp_map_last_kernel(void);

const char* mlbp_map_arch(void);             /* "gfx950" */
const char* mlbp_map_last_error(void);       /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
