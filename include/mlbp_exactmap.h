/* mlbp_exactmap.h -- C ABI of libmlbp_exactmap.so: the EXACT jointly most probable assignment (MAP) of batched factor graphs
 * and their max-marginals by cutset conditioning (AMD Instinct MI355X, gfx950, float64).
 *
 * The seventh library of the engine.  libmlbp_map.so runs max-product SWEEPS: exact on a tree, the usual approximation on a
 * graph with a cycle.  This one maximises the model itself, the way libmlbp_cutset.so sums it, so that the distance of the
 * sweeps' decoding from the truth can be reported.  It has its own source (macaronicusermodeling_amd/csrc_exactmap/), its own
 * kernel inventory (exactmap_*) and its own error slot; it shares no state with the other libraries.  It runs no sweep program
 * and reads no messages.  It takes the SAME packed plan as mlbp_cutset_f64 (include/mlbp_cutset.h states its layout, the cutset
 * choice and what the check refuses; the MLBP_CUTSET_* plan constants and limits are the ones used here).
 *
 * Conventions, as in mlbp_cutset.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_exactmap_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device memory
 * unless stated; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be
 * captured into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64 kernels'
 * dynamic-LDS limit, a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is no
 * CPU fallback: without a device the compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, per graph, with
 *     score(x) = sum over pairwise p of log T_p[x_a][x_b] + sum over unary u of log U_u[x_v]
 * (the score of mlbp_map.h and mlbp_cutset.h; a = the variable on axis 0 of factor p):
 *   assignment[v]        an x* that maximises score (int32, var_ids order)
 *   score                score(x*), from the logarithms of the table entries at x*, exactly as mlbp_cutset_f64 computes score
 *                        at `labels`
 *   max_marginals[v][s]  optional (natural log): max over x with x_v = s of score(x); -inf where no such assignment has a
 *                        positive potential.  For every v, max_s max_marginals[v][s] = score up to the rounding of the
 *                        logarithms (1e-12 relative).
 * A configuration c in [0, X^|C|) fixes cutset variable cutset[q] to state (c / X^q) mod X and conditions the model as
 * mlbp_cutset.h says.  The conditioned forest is solved by ONE pass from the leaves to the roots with
 * up[i] = max_j T[i][j] vec[j]; a root takes max_j vec[j]; V_c = the product of the constants and of every tree's maximum =
 * the maximum over the free variables under c.  The best configuration c* is re-solved once and decoded by back-pointers.
 *
 * Tie rule (the result is deterministic).  Among maximisers: (1) the lowest configuration index c wins; (2) within it every
 * forest root takes its lowest maximising state; (3) walking `order` backwards, every child takes its lowest maximising state
 * given its parent's.  Ties are ties of the computed values: exact on tables whose products are exact (powers of two).
 *
 * Range and determinism.  Nothing is rescaled but by powers of two, by exponent extraction, as in mlbp_cutset.h; exponents are
 * tallied in an integer.  V_c is a normalised (mantissa in [1, 2), exponent) pair and is COMPARED as such; no logarithm is taken
 * inside the walk.  A power-of-two rescaling and fmax are both exact, and no sum is formed anywhere, so -- unlike the sums of
 * mlbp_cutset_f64 -- the bits of every output are a function of the graph and the cutset alone: they do not depend on B, on
 * the number of chunks, or on which wave walked which configuration.  So a table times 2^k changes no state, and moves score
 * and the max-marginals by k ln 2 up to the rounding of the logarithm.
 * Max-marginals need the pass back from the roots (max form).  Under c, max over x_v = s is V_c * b[s] / max_s b[s] with b the
 * variable's full max-belief; a cutset variable gets V_c at its state.  The accumulators are mantissas against a running
 * reference exponent (the largest exponent of a V_c so far) and combine with fmax; a value below 2^-1000 of the reference is
 * dropped -- at every step and in the final combine alike, so the rule is a function of the graph too: a max-marginal more than
 * 1000 ln 2 = 693 nats below the graph's maximum reads -inf.  A call without max_marginals runs kernels without this pass.
 *
 * Edge rules.  An all-zero table (any graph whose best V_c is zero): every assignment has potential zero, so every state is a
 * maximiser and the tie rule gives the all-zero assignment; score = -inf and the max-marginals are all -inf.  A table
 * index outside its array: the graph is not computed -- assignment = -1, score = NaN, its max_marginals left as they were.
 * A NaN, negative or +inf entry (a NaN is passed over by fmax, as in mlbp_map.h): that graph's states lie in [0, X), its score
 * and max-marginals are unspecified; the call returns and every other graph keeps its bits.  More than MLBP_CUTSET_MAX_CONFIGS
 * configurations: MLBP_EUNSUPPORTED.
 *
 * The listed mode: the max over LISTED cutset states (N > 0).  Beyond MLBP_CUTSET_MAX_CONFIGS configurations -- K5 and up at
 * X = 64 -- the walk cannot visit every configuration; it can visit a caller's list of them, as mlbp_cutsetis_f64 does for the
 * sum.  With N > 0 the call reads `configs`, N rows of n_cut states per graph (row i, entry q: the state of cutset[q]), and walks
 * those rows in the place of the configurations c in [0, X^|C|).  V_i is the V_c above at configuration configs[g][i]: the
 * conditioned forest is completed optimally for every entry, so the result is the best assignment among ALL assignments whose
 * cutset state is listed -- a guarantee that needs no statistics: a list that holds the cutset state of an assignment x returns
 * an assignment that scores no less than x, and the full list in index order returns the bits of the exact call.
 *   Winner: the entry of largest V_i, compared as a (mantissa, exponent) pair; ties go to the lowest entry index i.  The tie
 *   rule then continues as above: (2) roots take their lowest maximising state, (3) children walking `order` backwards.
 *   assignment, score and entry are those of the winner.  The list may repeat a configuration.  n_cut == 0 is valid: there is
 *   one empty configuration, configs is not read, and the call equals the exact call on a forest.
 *   The bits of every output depend on the graph, the cutset and the list alone -- not on B, on the number of chunks, or on
 *   which wave walked which entry.
 *   Edge rules.  A state outside [0, X) anywhere in the graph's rows of configs: the graph is not computed -- assignment = -1,
 *   score = NaN, entry = -1; every other graph keeps its bits.  A table index outside its array: as above, and entry = -1.
 *   Every listed V_i zero: the all-zero rule above (the all-zero assignment, score = -inf), with entry = 0.
 *   Limits.  0 <= N <= MLBP_EXACTMAP_MAX_LISTED (else MLBP_EINVAL); at most MLBP_EXACTMAP_MAX_CUT cutset variables, and no
 *   bound on X^|C| (MLBP_EUNSUPPORTED beyond); N > 0 with max_marginals is MLBP_EUNSUPPORTED: a max over part of the state space
 *   is no max-marginal.  The kernel pick is the rule below, unchanged.
 *   Grid (B, C), C = mlbp_exactmap_chunks(B, N): workgroup (g, k) of the generic kernel walks entries k, k + C, ..., wave w of
 *   workgroup (g, k) of the X = 64 kernel 4 k + w, 4 k + w + 4 C, ...; word 2 of a partial's header holds the entry index, and
 *   exactmap_final_kernel re-solves the winning entry from its row of configs.
 *   Workspace of a listed call, 8 times
 *     B * parts * MLBP_EXACTMAP_PARTIAL_HEADER                                          parts = C (generic) or 4 C (X = 64)
 *     + B * (2 n_vars + 1) * round_up(X, 2)                                             the final kernel's vectors
 *     + B * C * (5 n_vars + 2) * round_up(X, 2)                                         when the generic kernel keeps its vectors there
 *   mlbp_exactmap_workspace_bytes states the exact call alone; the compute entry checks this formula itself.
 *   Plan.  mlbp_exactmap_check_plan keeps the exact call's bound on X^|C|; validate the plan of a listed call with
 *   mlbp_cutsetis_check_plan (include/mlbp_cutsetis.h), whose bound is the listed one.
 * With N == 0 every field of the listed mode is ignored (entry apart, see the struct) and the call is the exact call.
 */
#ifndef MLBP_EXACTMAP_H
#define MLBP_EXACTMAP_H

#include <stdint.h>

#include "mlbp_cutset.h"                     /* status codes; the plan's layout, constants and limits */

#ifdef __cplusplus
extern "C" {
#endif

/* Which walk kernel a call enqueues -- the rule of mlbp_cutset_pick_kernel, a function of (X, n_vars, P, U, n_forest) alone,
 * with the same constants, whether or not max_marginals is asked for (the instance without the pass back leaves part of its
 * LDS unused):
 *   MLBP_EXACTMAP_KERNEL_X64      X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + INTS <= MLBP_CUTSET_X64_LDS_BYTES
 *                                 (K3, K4 and a chain of three fit, a chain of four does not): exactmap_x64_kernel<MM>.  The
 *                                 forest's tables in LDS, rows of 65, rescaled once; every WAVE walks configurations of its own,
 *                                 lane = state; a contraction is 64 multiplies and 64 fmax per lane against the LDS table with
 *                                 the vector broadcast by v_readlane; no workgroup barrier inside the walk.
 *   MLBP_EXACTMAP_KERNEL_GENERIC  every other shape (2 <= X <= 1024): exactmap_generic_kernel<MM>.  The workgroup walks one
 *                                 configuration at a time, tables streamed with masked tails; its 5 n_vars + 2 vectors in LDS
 *                                 when (5 n_vars + 2) * round_up(X, 2) * 8 + 64 + INTS <= MLBP_CUTSET_GENERIC_LDS_BYTES, else in
 *                                 the caller's workspace.
 * INTS = 4 * round_up(P + U + 16, 4).  MM = max_marginals given.
 *
 * Grid (B, C), C = mlbp_exactmap_chunks(B, n_configs) = min(n_configs, ceil(MLBP_CUTSET_MIN_WORKGROUPS / B)): workgroup (g, k)
 * of the generic kernel walks configurations k, k + C, ..., wave w of workgroup (g, k) of the X = 64 kernel 4 k + w,
 * 4 k + w + 4 C, ...  Each writes one partial: {best mantissa, exponent, configuration index, reference exponent} and, with
 * MM, the accumulators [n_vars][X].  exactmap_final_kernel, one workgroup per graph, picks the best partial (ties: the lowest
 * c), re-solves that configuration with the tables streamed, backtracks the states, takes the logarithms for score and turns
 * the max-marginal accumulators into logarithms. */
#define MLBP_EXACTMAP_KERNEL_NONE 0
#define MLBP_EXACTMAP_KERNEL_X64 1
#define MLBP_EXACTMAP_KERNEL_GENERIC 2
#define MLBP_EXACTMAP_PARTIAL_HEADER 4
#define MLBP_EXACTMAP_DROP_BELOW 1000        /* a max-marginal below 2^-1000 of the graph's maximum reads -inf */
#define MLBP_EXACTMAP_MAX_LISTED 65536       /* the most entries a list holds per graph */
#define MLBP_EXACTMAP_MAX_CUT 16             /* the most cutset variables of a listed call */

typedef struct mlbp_exactmap_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_exactmap_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  int32_t N;                                 /* 0: the exact call; 1 .. MLBP_EXACTMAP_MAX_LISTED: entries listed per graph */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_exactmap_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const int32_t* configs;                    /* listed call: device [B][N][n_cut], the state of cutset[q]; NULL when N == 0 or n_cut == 0 */
  double* workspace;                         /* device, workspace_bytes >= mlbp_exactmap_workspace_bytes(...) */
  int64_t workspace_bytes;
  int32_t* assignment;                       /* device [B][n_vars] */
  double* score;                             /* device [B] */
  double* max_marginals;                     /* optional device [B][n_vars][X] */
  int32_t* entry;                            /* optional device [B]: the index of the winning list entry (listed call) or the
                                                winning configuration index (exact call); -1 for a graph that is not computed */
} mlbp_exactmap_args;

/* Table indices are device data and are not checked on the host: see the edge rules above. */
int mlbp_exactmap_f64(const mlbp_exactmap_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_cutset_check_plan, with its messages. */
int mlbp_exactmap_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: MLBP_EXACTMAP_KERNEL_X64 or _GENERIC by the rule above; statuses as mlbp_cutset_pick_kernel. */
int mlbp_exactmap_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest);

/* Host only: C of the grid (B, C) by the rule above; MLBP_EINVAL for non-positive arguments. */
int mlbp_exactmap_chunks(int32_t B, int32_t n_configs);

/* Host only: bytes of workspace a call needs, 8 times
 *   B * parts * (MLBP_EXACTMAP_PARTIAL_HEADER + (max_marginals ? n_vars * X : 0))     parts = C (generic) or 4 C (X = 64)
 *   + B * (2 n_vars + 1) * round_up(X, 2)                                             the final kernel's vectors
 *   + B * C * (5 n_vars + 2) * round_up(X, 2)                                         when the generic kernel keeps its vectors there
 * with n_configs = X^n_cut; a negative status as pick_kernel / chunks give it, MLBP_EUNSUPPORTED above MLBP_CUTSET_MAX_CONFIGS. */
int64_t mlbp_exactmap_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut,
                                      int32_t max_marginals);

/* Host-side record of the walk kernel the calling thread's last mlbp_exactmap_f64 enqueued (MLBP_EXACTMAP_KERNEL_*; NONE when
 * it was refused before the launch). */
int mlbp_exactmap_last_kernel(void);

const char* mlbp_exactmap_arch(void);        /* "gfx950" */
const char* mlbp_exactmap_last_error(void);  /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
