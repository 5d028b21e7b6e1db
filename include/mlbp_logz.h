/* mlbp_logz.h -- C ABI of libmlbp_logz.so: the log-partition function and the joint log-likelihood of batched factor
 * graphs (AMD Instinct MI355X, gfx950, float64).
 *
 * The third library of the engine.  libmlbp.so (mlbp.h) gives each variable's marginal, libmlbp_map.so (mlbp_map.h) the
 * jointly most probable assignment; this one reads log Z out of the messages the sweeps leave, so that the log-potential
 * of any assignment becomes a log-probability:  joint_logp(x) = score(x) - log Z.  Exact on trees, the Bethe value on
 * loopy graphs.  It has its own sources (macaronicusermodeling_amd/csrc_logz/), its own kernel inventory and its own
 * error slot; it shares no state with the other two libraries.
 *
 * Conventions, as in mlbp_map.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_logz_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory unless stated; the compute call only ENQUEUES -- no allocation, no copy, no synchronisation and no attribute
 * call inside it, so it may be captured into a HIP graph and replayed; arguments are checked on the host before anything
 * is enqueued.  There is no CPU fallback: without a device the compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, per graph.  Only factor->variable messages are read: m_{f->v} = msgs[in-slot of (f, v)].
 * Products are pure products (no uniform 1/X factor, no nan_to_num); IEEE arithmetic, nothing is clamped.
 *   q_v(x)     = prod over the in-slots of v of m(x)                       Z_v = sum_x q_v(x)
 *   n_{v\f}(x) = the same product without the slot of f                    (empty product = 1)
 *   unary f on v:         Z_f = sum_x row_f(x) n_{v\f}(x)
 *   pairwise f on (a, b): Z_f = sum_{i,j} n_{a\f}(i) T_f[i][j] n_{b\f}(j)  (a = pair_axis_var[f][0] on table axis 0)
 *   log_z      = sum_f log Z_f - sum_v (d_v - 1) log Z_v                   (d_v = number of in-slots of v; natural log)
 *   score      = sum over pairwise f of log T_f[x_a][x_b] + sum over unary f of log row_f[x_v]     at x = labels
 *   joint_logp = score - log_z
 * A variable with one factor has weight d_v - 1 = 0: its Z_v is not computed.
 * The value does not depend on the scale of any message.  A zero table entry at the labels gives score = -inf.
 * Range.  Tables of any normal magnitude are fine: a table times 2^k moves log_z by k ln 2 and nothing else.  The limit is in
 * the messages: q_v and n_{v\f} are plain float64 products of d_v (d_v - 1) NORMALISED messages, and such a product must stay
 * in the normal range for the entries that carry Z_v and Z_f.  With d_v = 12 (seven predicted words) and messages spanning
 * 170 decades each (tables exp(20 N(0,1))) it does not: entries flush to zero, log_z is off by up to 1e-4 or not finite.
 * At d_v = 12 and 85 decades (exp(10 N(0,1))), and at d_v <= 10 and 170 decades, the value is within 4e-12 of a log-domain
 * evaluation (tests/test_range_cpu.py, tests/test_gpu_exponent_range.py).
 */
#ifndef MLBP_LOGZ_H
#define MLBP_LOGZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: the values of mlbp.h / mlbp_map.h.  A translation unit that uses several headers includes this one last. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
#endif

/* Which kernel a call enqueues -- a function of (X, n_in_slots, n_vars, flags) alone, never a user option
 * (n_in_slots = in_off[n_vars] = 2 P + U, the factor->variable slots of one graph):
 *   MLBP_LOGZ_KERNEL_X64_SHARED  X == 64 and MLBP_LOGZ_SHARED_PAIR_TABLES is set: 16 graphs per workgroup.  A pairwise
 *                                table that all graphs of the group name is read ONCE per workgroup and contracted with
 *                                the group's 16 pairs of leave-one-out vectors (16 KiB of LDS, whatever the shape); a
 *                                factor for which the group's graphs name different tables is walked graph by graph in
 *                                the same kernel.  Messages are read from global memory.
 *   MLBP_LOGZ_KERNEL_X64         X == 64 otherwise, when the graph's in-slot messages fit the LDS budget:
 *                                  n_in_slots * 512  (messages)  +  4096  (two leave-one-out vectors per wave)
 *                                  +  64  (per-wave partial sums)   <=   MLBP_LOGZ_X64_LDS_BYTES
 *                                i.e. up to 119 in-slots, inside the 64 KiB a kernel gets without an attribute call.  One
 *                                workgroup per graph; every pairwise table is streamed from HBM once.
 *   MLBP_LOGZ_KERNEL_GENERIC     every other shape (2 <= X <= 1024): messages in global memory, tables streamed.
 * n_vars is validated and does not enter the rule: no kernel keeps per-variable state on chip.
 * mlbp_logz_pick_kernel states the rule (host only). */
#define MLBP_LOGZ_KERNEL_NONE 0
#define MLBP_LOGZ_KERNEL_X64 1
#define MLBP_LOGZ_KERNEL_X64_SHARED 2
#define MLBP_LOGZ_KERNEL_GENERIC 3
#define MLBP_LOGZ_X64_LDS_BYTES 65536
#define MLBP_LOGZ_MAX_X 1024
#define MLBP_LOGZ_GROUP 16                   /* graphs per workgroup of the shared-table kernel */

/* flags: the caller claims that many graphs name the same pairwise tables (the trainer's layout).  The claim is checked
 * on the device per workgroup and factor; where it does not hold the graphs are computed one at a time, same results. */
#define MLBP_LOGZ_SHARED_PAIR_TABLES 1

typedef struct mlbp_logz_args {
  int32_t B, X, n_msgs, P, U, n_vars;        /* graphs, states, message slots, pairwise / unary factors, variables */
  int32_t n_pair_tables, n_unary_tables;
  int32_t flags;                             /* MLBP_LOGZ_SHARED_PAIR_TABLES or 0 */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const double* msgs;                        /* device [B][n_msgs][X], read only */
  const int32_t* in_off;                     /* device [n_vars + 1], validated by mlbp_logz_check_readout */
  const int32_t* in_slots;                   /* device [2 P + U] incoming factor->variable slots, variable by variable */
  const int32_t* pair_axis_var;              /* device [P][2] variable on table axis 0 / 1 (NULL when P == 0) */
  const int32_t* unary_var;                  /* device [U] (NULL when U == 0) */
  const int32_t* pair_in_slot;               /* device [P][2] slot of m_{f -> axis-k variable} (NULL when P == 0) */
  const int32_t* unary_in_slot;              /* device [U] slot of m_{f -> its variable} (NULL when U == 0) */
  const int32_t* labels;                     /* optional device [B][n_vars]; needed by score and joint_logp */
  double* log_z;                             /* optional device [B] */
  double* score;                             /* optional device [B] */
  double* joint_logp;                        /* optional device [B] */
  double* sum_out;                           /* optional device [2]: sum of log_z and of joint_logp over the batch, added in
                                                a fixed order by one more launch behind the main kernel.  Needs log_z;
                                                sum_out[1] is 0 when joint_logp is NULL. */
} mlbp_logz_args;

/* Table indices and labels are device data and are not checked on the host.  A graph that names a table outside
 * [0, n_pair_tables) / [0, n_unary_tables) is not computed: its three outputs are NaN.  A label outside [0, X) makes that
 * graph's score and joint_logp NaN; its log_z is computed. */
int mlbp_logz_f64(const mlbp_logz_args* args, void* stream);

/* Host only, no GPU needed: validates every index array so that no launch can index outside msgs or a table-index row:
 * in_off monotone from 0 with in_off[n_vars] == 2 P + U, in_slots < n_msgs, pair_axis_var / unary_var < n_vars,
 * pair_in_slot[p][k] one of the in-slots of variable pair_axis_var[p][k], unary_in_slot[u] one of those of unary_var[u].
 * Host arrays; the pair arrays may be NULL when P == 0, the unary ones when U == 0. */
int mlbp_logz_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, int32_t P,
                            const int32_t* pair_axis_var, const int32_t* pair_in_slot, int32_t U, const int32_t* unary_var,
                            const int32_t* unary_in_slot);

/* Host only: MLBP_LOGZ_KERNEL_X64, _X64_SHARED or _GENERIC by the rule above; MLBP_EUNSUPPORTED for X > MLBP_LOGZ_MAX_X,
 * MLBP_EINVAL for X < 2, non-positive sizes or unknown flag bits. */
int mlbp_logz_pick_kernel(int32_t X, int32_t n_in_slots, int32_t n_vars, int32_t flags);

/* Host-side record of the kernel the calling thread's last mlbp_logz_f64 enqueued (MLBP_LOGZ_KERNEL_*; NONE when it was
 * refused before the launch). */
int mlbp_logz_last_kernel(void);

const char* mlbp_logz_arch(void);            /* "gfx950" */
const char* mlbp_logz_last_error(void);      /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
