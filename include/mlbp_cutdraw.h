/* mlbp_cutdraw.h -- C ABI of libmlbp_cutdraw.so: a PROPOSAL for cutset importance sampling drawn from held BP messages, one
 * launch per call (AMD Instinct MI355X, gfx950, float64).
 *
 * The twelfth library of the engine.  libmlbp_cutsetis.so (include/mlbp_cutsetis.h) weights a LIST of joint states of the
 * cutset by Z_c / q(c); this library makes such a list -- N joint states per graph and the log-probability log_q the proposal
 * gave each -- from the factor-to-variable messages a sweep left behind, without sweeping again: the cutset variables are
 * drawn one after the other, and the only thing the held messages lack, the clamp of the variables already drawn, is put in
 * exactly as the row (or column) of the pairwise table at the drawn state.  It has its own source
 * (macaronicusermodeling_amd/csrc_cutdraw/), its own kernel inventory (cutdraw_*) and its own error slot; it shares no state
 * with the other libraries and reads no plan but its own.
 *
 * Conventions, as in the siblings: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_cutdraw_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be captured
 * into a HIP graph and replayed (both kernels keep their LDS static: no attribute call, the first call may be the captured
 * one); arguments are checked on the host before anything is enqueued.  There is no CPU fallback: without a device the
 * compute call returns MLBP_ENODEVICE.  There is no workspace.
 *
 * Semantics of one call, per graph g and entry i.  For the positions k = 0 .. n_cut-1 in turn, a = cutset[k], the vector v
 * over the X states s of a is formed in this order:
 *   1. v starts as the first BASE message and the others are multiplied in.  A base message is msgs[g][slot] for the
 *      factor->a slot of each factor of a, in a's facset order, that is unary, or pairwise with its other end not at an
 *      earlier cut position: the in-slots of a that the marginal read-out multiplies, minus the factors that reach an earlier
 *      cutset variable.  (A position without a base message starts from v = 1 in every state.)
 *   2. For each pairwise factor p of a whose other end is cutset[j], j < k, in facset order, v is multiplied by the table
 *      pair_tab[g][p] read at the drawn state c_j: T[c_j][s] when a sits on axis 1 of the table, T[s][c_j] when a sits on
 *      axis 0.  No contraction: a clamped variable's message through a pairwise factor IS that row or column.  Several
 *      factors between the same two variables are several items.
 *   3. After EVERY multiplication v is scaled by 2^-e, e the binary exponent of its largest entry (a NaN entry is passed
 *      over; e = floor(log2) of a normal number, -1023 for a subnormal one); the scaling is skipped when that entry is 0 or
 *      not finite.  This is the only rescaling: nothing else touches the values, nothing is normalised, no nan_to_num.
 *   4. The draw, by the rule mlbp_exactsample.h uses for a free variable: A_s is the inclusive prefix sum of v, total =
 *      A_{X-1}, thr = uniforms[g][i][k] * total; the state is the lowest s with A_s > thr and v_s > 0; if there is none, the
 *      highest s with v_s > 0; if no such s exists either, 0.  log_q[g][i] += ln(v_state / total), and -inf when total is 0
 *      (an empty v).  A later position is then drawn as usual.  (X = 64: the prefix sums are the WAVE sums of
 *      mlbp_exactsample.h; every other X: its SEGMENTED sums.)
 * With `configs_in` given (the second mode) the state of every position is READ from configs_in[g][i][k] instead of drawn:
 * `uniforms` is not read, `configs` is not written, only log_q comes out -- the probability the proposal gives to
 * configurations the caller names, which is what mixtures of proposals need.  log_q of a drawn list, asked for again through
 * the second mode, comes back bit for bit.
 *
 * Position 0 has base messages only, so its q is the loopy-BP marginal of cutset[0].  Three further facts:
 *   - The sum over all X^n_cut configurations of exp(log_q) is 1, for any positive messages: q is a distribution, and
 *     exp(log_z_hat) of mlbp_cutsetis.h stays unbiased wherever q is positive where Z_c is.
 *   - On a tree whose messages are BP's fixed point, with a cutset that is a connected set of variables listed so that
 *     every variable has exactly one earlier neighbour, q(c) = Z_c / Z exactly: every weight of the estimate is Z, ess = N.
 *   - The bits of entry (g, i) are a function of the graph's tables, its messages, the cutset and uniforms[g][i] alone.
 *     They do not depend on B, N, the grid or the wave that drew the entry.
 *
 * Edge rules.  A table index of the graph's row of pair_tab outside its array: that graph's `configs` are -1 and its log_q
 * NaN; every other graph keeps its bits.  A configs_in state outside [0, X): that entry's log_q is NaN.  A NaN in a message
 * or table an entry reads: that entry's log_q is NaN and its states stay inside [0, X).  A uniform outside [0, 1) or NaN
 * needs no special case: the draw rule above gives a state (the highest of positive weight).  An empty conditional -- every
 * v_s zero, as behind an all-zero table row -- gives state 0 and log_q = -inf; mlbp_cutsetis_f64 then refuses that graph by
 * its own rule (a log_q that is no finite number).  n_cut = 0 is valid: no kernel is launched and log_q is set to 0.
 *
 * The draw plan.  A packed int32 array, built on the host (macaronicusermodeling_amd/cutdraw.py plan_words) and validated by
 * mlbp_cutdraw_check_plan before upload:
 *     header[MLBP_CUTDRAW_PLAN_HEADER] = {n_vars, P, n_msgs, n_cut, n_base, n_rows, 0, 0}
 *     cutset[n_cut]            variable index of every position
 *     base_off[n_cut + 1]      position k multiplies base_slots[base_off[k] .. base_off[k + 1])
 *     base_slots[n_base]       message slots
 *     row_off[n_cut + 1]       position k then multiplies rows[row_off[k] .. row_off[k + 1])
 *     rows[n_rows][3]          {pair slot, earlier position j, axis of THIS variable in the table}
 *
 * Kernels.  The pick is a function of X alone:
 *   MLBP_CUTDRAW_KERNEL_X64      X == 64: workgroups of 256 threads, lane = state.  The workgroup forms every position's base
 *                                product once and keeps it in static LDS (n_cut * 512 bytes, at most 8 KiB); then every WAVE
 *                                draws entries of its own, no workgroup barrier after the prologue; the rows or columns of a
 *                                position are loaded together, the draw is a wave scan and a ballot.
 *   MLBP_CUTDRAW_KERNEL_GENERIC  every other X, 2 <= X <= 1024: a workgroup per entry, v in static LDS, base messages and
 *                                table rows streamed (they hit L2 after the first entry), the segmented block scan.
 * Both run on a grid of (B, C) workgroups, C = mlbp_cutdraw_chunks(B, N) = min(N, ceil(MLBP_CUTDRAW_MIN_WORKGROUPS / B)), the
 * rule of mlbp_cutsetis.h: workgroup (g, k) of the generic kernel takes entries k, k + C, ... of graph g; wave w of workgroup
 * (g, k) of the X = 64 kernel takes entries 4 k + w, 4 k + w + 4 C, ...
 */
#ifndef MLBP_CUTDRAW_H
#define MLBP_CUTDRAW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: the values of mlbp.h.  A translation unit that uses several headers includes this one last. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H) && !defined(MLBP_LOGZ_H) && !defined(MLBP_SAMPLE_H) && !defined(MLBP_CONVERGE_H) && !defined(MLBP_CUTSET_H) && !defined(MLBP_CUTSETIS_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
#endif

#define MLBP_CUTDRAW_KERNEL_NONE 0
#define MLBP_CUTDRAW_KERNEL_X64 1
#define MLBP_CUTDRAW_KERNEL_GENERIC 2
#define MLBP_CUTDRAW_MAX_LISTED 65536
#define MLBP_CUTDRAW_MAX_CUT 16
#define MLBP_CUTDRAW_MAX_X 1024
#define MLBP_CUTDRAW_MIN_WORKGROUPS 512
#define MLBP_CUTDRAW_PLAN_HEADER 8

typedef struct mlbp_cutdraw_args {
  int32_t B, X, n_msgs, P;                   /* graphs, states, message slots, pairwise factors */
  int32_t n_cut;                             /* the plan's header, as mlbp_cutdraw_check_plan saw it */
  int32_t n_pair_tables;
  int32_t plan_words;
  int32_t N;                                 /* entries per graph, 1 <= N <= MLBP_CUTDRAW_MAX_LISTED */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_cutdraw_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] */
  const double* msgs;                        /* device [B][n_msgs][X]: the messages as a sweep left them */
  const double* uniforms;                    /* device [B][N][n_cut]; not read (may be NULL) when configs_in is given */
  const int32_t* configs_in;                 /* optional device [B][N][n_cut]: the second mode */
  int32_t* configs;                          /* device [B][N][n_cut]; not written (may be NULL) when configs_in is given */
  double* log_q;                             /* device [B][N] */
} mlbp_cutdraw_args;

/* Table indices, messages, uniforms and configs_in are device data and are not checked on the host: see the edge rules. */
int mlbp_cutdraw_f64(const mlbp_cutdraw_args* args, void* stream);

/* Host only, no GPU needed: MLBP_OK when the packed plan is consistent -- the sizes of the header give n_words, n_msgs is the
 * header's, every cutset variable is in [0, n_vars) and named once (a repeated one: MLBP_EINVAL), both offset arrays start at
 * 0, never decrease and end at n_base / n_rows, every base slot is in [0, n_msgs), every row's pair slot in [0, P), its
 * position strictly earlier than its own, its axis 0 or 1.  n_cut above MLBP_CUTDRAW_MAX_CUT, X above MLBP_CUTDRAW_MAX_X:
 * MLBP_EUNSUPPORTED; X < 2: MLBP_EINVAL. */
int mlbp_cutdraw_check_plan(const int32_t* plan, int32_t n_words, int32_t X, int32_t n_msgs);

/* Host only: MLBP_CUTDRAW_KERNEL_X64 for X == 64, else _GENERIC; MLBP_EINVAL for X < 2, MLBP_EUNSUPPORTED above 1024. */
int mlbp_cutdraw_pick_kernel(int32_t X);

/* Host only: C of the grid (B, C) by the rule above; MLBP_EINVAL for B <= 0 or N outside [1, MLBP_CUTDRAW_MAX_LISTED]. */
int mlbp_cutdraw_chunks(int32_t B, int32_t N);

/* Host-side record of the kernel the calling thread's last mlbp_cutdraw_f64 enqueued (MLBP_CUTDRAW_KERNEL_*; NONE when it
 * was refused before the launch, or launched nothing: n_cut = 0). */
int mlbp_cutdraw_last_kernel(void);

const char* mlbp_cutdraw_arch(void);         /* "gfx950" */
const char* mlbp_cutdraw_last_error(void);   /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
