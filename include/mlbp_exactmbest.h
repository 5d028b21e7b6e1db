/* mlbp_exactmbest.h -- C ABI of libmlbp_exactmbest.so: the EXACT M jointly most probable assignments of batched factor graphs,
 * ranked, by cutset conditioning (AMD Instinct MI355X, gfx950, float64).
 *
 * The tenth library of the engine, a sibling of libmlbp_exactmap.so: that one returns the best whole set of guesses and knows
 * the runner-up only by its score; this one returns the M best sets, best first, each with its score.  It has its own source
 * (macaronicusermodeling_amd/csrc_exactmbest/), its own kernel inventory (exactmbest_*) and its own error slot; it shares no
 * state with the other libraries.  It runs no sweep program and reads no messages.  It takes the SAME packed plan as
 * mlbp_cutset_f64 (include/mlbp_cutset.h states its layout, the cutset choice and what the check refuses; the MLBP_CUTSET_* plan
 * constants and limits are the ones used here).
 *
 * Conventions, as in mlbp_exactmap.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_exactmbest_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be captured into
 * a HIP graph and replayed (after one eager call of an X = 64 shape: the first such call on a device raises the dynamic-LDS
 * limit of both X = 64 kernels, whichever lists kernel it takes itself -- a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is no CPU fallback: without
 * a device the compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, per graph g, with score(x) the score of mlbp_exactmap.h and 1 <= M <= MLBP_EXACTMBEST_MAX_M:
 *   assignments[g][r][v]  int32, var_ids order: the M assignments of largest score among those of positive potential, best
 *                         first, pairwise distinct
 *   scores[g][r]          score(assignments[g][r]), from the logarithms of the table entries at that assignment, exactly as
 *                         exactmap_final_kernel takes score; non-increasing in r up to the rounding of the logarithms
 *   n_found[g]            min(M, the number of assignments of positive potential).  Rows r >= n_found read assignment -1 and
 *                         score -inf.  THIS DIFFERS from mlbp_exactmap_f64, which answers an all-zero table with the all-zero
 *                         assignment: a list does not name assignments the model gives no mass.
 *
 * Two facts make it cheap.
 *   (1) Every assignment under configuration c has a value of at most V_c, the configuration's maximum.  So the M best
 *       assignments lie inside the M configurations of largest V_c (ties: the lower c): only those need more than the max walk.
 *   (2) Under one configuration the remainder is a forest, and its M best are found by the LIST FORM of the pass from the leaves
 *       to the roots: every free variable keeps, per state, an ordered list of at most M best values of its subtree with
 *       back-pointers; a child's lists are contracted through its table into lists per parent state, which are folded into
 *       the parent's, list against list; the roots' lists are folded into one; the assignment is decoded from the back-pointers.
 *
 * Four launches:
 *   values   exact_map's walk without its merge (x64_up<MaxAlg, false> or generic_up<MaxAlg> of csrc/mlbp_cutset_walk.h) over
 *            every configuration, V_c written apart as a normalised (mantissa in [1, 2), exponent) pair.  Grid (B, C),
 *            C = mlbp_exactmbest_chunks(B, n_configs), the kernel by the rule of mlbp_cutset_pick_kernel.
 *   select   one workgroup per graph: the at most M configurations of POSITIVE V_c, by V_c descending, compared as pairs
 *            (exponent, then mantissa), ties to the lower c.
 *   lists    a task per (graph, selected configuration r), taken by a wave (X = 64 form) or a workgroup (generic form): it
 *            solves the configuration in the list form and writes its at most M candidates -- value pair and assignment -- to
 *            the workspace.
 *   merge    one workgroup per graph: the at most M x M candidates down to the best M, the assignments, the scores by
 *            logarithms, n_found.
 *
 * The list form, stated once; tests/test_exactmbest_cpu.py mirrors it line by line in NumPy.  All values of one vector share a
 * power-of-two scale, tallied in an integer, exactly as in the walk.  L[v][j] is the list of free variable v at state j,
 * descending, 0 = no entry.
 *   start     L[v][j] = (local(v, j)): the variable's unary rows times its cutset-incident rows and columns under c.
 *   for v in `order` (children before parents):
 *     rescale L[v] by the exponent of its largest entry.  An entry of rank >= 1 that is then below 2^-MLBP_EXACTMBEST_DROP_BELOW
 *               becomes 0 (dropped); rank 0 is left as the max walk leaves it.  So: a candidate that is not its state's best
 *               and lies more than 2^-1000 below the best value of its conditioned subtree is dropped -- a function of the
 *               graph and the cutset alone.
 *     v has a parent through table T (rescaled by its exponent):
 *       contract  C[i] = the M largest of T[i][j] * L[v][j][k] over (j, k), offered in the order j ascending, then k ascending;
 *                 back-pointer (j, k).  (T[j][i] when v is on axis 0.)
 *       rescale C as above;
 *       fold      L[parent][i] = the M largest of L[parent][i][a] * C[i][b] over (a, b), offered a ascending, then b ascending;
 *                 back-pointer (a, b).
 *     v is a root:
 *       R = the M largest of L[v][j][k] over (j, k), ties to the lower j, then the lower k; back-pointer (j, k);
 *       fold      F = the M largest of F[a] * R[b] over (a, b), offered a ascending, then b ascending.  F holds (mantissa,
 *                 exponent) pairs and starts as the one pair of the configuration's constants; a product is normalised as the
 *                 walk normalises V_c and compared as a pair.
 *   An offer enters a list BEHIND every entry it does not exceed: among equal values the one offered first stays first.
 *   F[k], k < M, are the configuration's candidates.  Rank 0 of every list goes through the operations of the max walk in their
 *   order, so F[0] has the bits generic_up<MaxAlg> gives V_c.
 *   decode    walking `order` backwards, a root takes (state, rank) from F's and R's back-pointers, a child from its parent's
 *             state and rank through the fold's and the contraction's.
 * Only (a, b) with (a + 1) * (b + 1) <= M are offered to a fold: any other has M offers ahead of it that it does not exceed.
 *
 * Order and ties of the result.  Candidates are ordered by value descending, compared as pairs; among equal values the lower
 * configuration index comes first, then the lower rank inside the configuration, which is fixed by the rule above.  With
 * M = 1 the output is mlbp_exactmap_f64's assignment wherever the best set is not tied.  The select compares the values pass's
 * V_c and the merge the lists pass's candidates; where the values pass took the X = 64 kernel and the lists pass the generic one,
 * the two round a configuration's constants in a different order, so they agree to the last bits, not in them.
 *
 * Range and determinism.  Nothing is rescaled but by powers of two; no sum is formed and no logarithm is taken inside the
 * passes; every comparison is of computed values.  So the bits of every output depend on the graph, the cutset and M's prefix
 * alone: rows 0 .. M'-1 of a call with M' < M equal the call with M' (a list's first M' entries depend on the first M' entries
 * of the lists it is made of), and the outputs do not depend on B, the position in the batch, shared or unique tables, the
 * chunk count or which wave walked what.  A table times 2^k changes no state and moves the scores by k ln 2 up to the rounding
 * of the logarithm.
 *
 * Edge rules.  A table index outside its array: the graph is not computed -- n_found = -1, its assignments -1, its scores NaN;
 * every other graph keeps its bits.  A NaN, negative or +inf entry: that graph's states lie in [0, X) or are -1, its scores
 * and n_found are unspecified; the call returns and every other graph keeps its bits.  More than MLBP_CUTSET_MAX_CONFIGS
 * configurations: MLBP_EUNSUPPORTED.  M outside [1, MLBP_EXACTMBEST_MAX_M]: MLBP_EINVAL.
 *
 * The listed mode: the M best over LISTED cutset states (N > 0).  Beyond MLBP_CUTSET_MAX_CONFIGS configurations -- K5 and up at
 * X = 64 -- the walk cannot visit every configuration; it can visit a caller's list of them, as the listed mode of
 * mlbp_exactmap_f64 does for the maximum.  With N > 0 the call reads `configs`, N rows of n_cut states per graph (row i, entry
 * q: the state of cutset[q]), and walks those rows in the place of the configurations c in [0, X^|C|): "configuration" in facts
 * (1) and (2) above reads "entry".  V_i is the V_c above at configuration configs[g][i]; every assignment whose cutset state is
 * entry i scores at most V_i, and under one entry the remainder is a forest, which the list form solves exactly.  So the rows
 * are the TRUE M best among ALL assignments of positive potential whose cutset state equals some listed row -- a guarantee that
 * needs no statistics --, best first and pairwise distinct; n_found = min(M, their number); the rows behind it read -1 / -inf.
 *   Duplicates.  A list may repeat a cutset state (a search list draws with replacement).  An entry whose row equals the row of
 *   an entry of lower index is IGNORED: the first occurrence counts, so no row of the result repeats.  V_i is a function of the
 *   graph, the cutset and the row alone, so equal rows have equal V bits: the select closes the duplicates of a taken entry
 *   inside its scans -- an open entry whose V pair equals the pair of the at most M taken entries is compared with them row
 *   against row, and rows are compared nowhere else.  The select stays at M rounds however many repeats the list holds.
 *   Order.  Candidates go by value descending, compared as (mantissa, exponent) pairs; ties go to the lower entry index, then
 *   to the lower rank inside the entry.  The prefix property in M holds unchanged.  Row 0 is the listed mlbp_exactmap_f64's
 *   answer on the same list wherever the best set is not tied inside its entry, and entries[0] its `entry`.  The full list in
 *   index order returns the exact call's rows, scores and n_found in every bit, and entries equal to the configuration numbers.
 *   The bits of every output depend on the graph, the cutset, the list and M's prefix alone -- not on B, the position in the
 *   batch, shared or unique tables, the chunk count or which wave walked what.
 *   Edge rules.  A state outside [0, X) anywhere in the graph's rows of configs: the graph is not computed -- n_found = -1, its
 *   assignments -1, its scores NaN, its entries -1; every other graph keeps its bits.  A state is validated BEFORE it forms an
 *   address: by a ballot over the packed row in the X = 64 values kernel, by a loop over the row in the generic one; such an entry
 *   gets a marker in the place of its V pair, the select refuses the graph on it, and the lists pass reads rows of graphs that
 *   were not refused alone.  A table index outside its array: as above, and entries -1.  n_cut == 0 is valid: there is one empty
 *   configuration, configs is not read, and the call equals the exact call on a forest (entries 0).
 *   Limits.  0 <= N <= MLBP_EXACTMBEST_MAX_LISTED (else MLBP_EINVAL); at most MLBP_EXACTMBEST_MAX_CUT cutset variables and no
 *   bound on X^|C| (MLBP_EUNSUPPORTED beyond).  The kernel pick is the rule below, unchanged.
 *   Grid of the values pass (B, C), C = mlbp_exactmbest_chunks(B, N): workgroup (g, k) of the generic kernel walks entries k,
 *   k + C, ..., wave w of workgroup (g, k) of the X = 64 kernel 4 k + w, 4 k + w + 4 C, ...; V_i is written apart as a pair into
 *   slot i.  The select runs over the N entries by entry index; both lists kernels read the selected entry's row from configs
 *   where they decode c; the merge breaks ties by entry index and writes `entries`.
 *   Workspace of a listed call: the formula of mlbp_exactmbest_workspace_bytes below with N in the place of n_configs and
 *   C = mlbp_exactmbest_chunks(B, N).  mlbp_exactmbest_workspace_bytes states the exact call alone; the compute entry checks
 *   this formula itself.
 *   Plan.  mlbp_exactmbest_check_plan keeps the exact call's bound on X^|C|; validate the plan of a listed call with
 *   mlbp_cutsetis_check_plan (include/mlbp_cutsetis.h), whose bound is the listed one.
 * With N == 0 every field of the listed mode is ignored (entries apart, see the struct) and the call is the exact call.
 */
#ifndef MLBP_EXACTMBEST_H
#define MLBP_EXACTMBEST_H

#include <stdint.h>

#include "mlbp_cutset.h"                     /* status codes; the plan's layout, constants and limits */

#ifdef __cplusplus
extern "C" {
#endif

/* Which kernels a call enqueues.  mlbp_exactmbest_pick_kernel and _last_kernel return VALUES | LISTS << 4:
 *   VALUES  the rule of mlbp_cutset_pick_kernel, a function of (X, n_vars, P, U, n_forest) alone:
 *     MLBP_EXACTMBEST_KERNEL_X64      X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + INTS <= MLBP_CUTSET_X64_LDS_BYTES:
 *                                     exactmbest_values_x64_kernel (a wave per configuration, lane = state; uses its bel alone)
 *     MLBP_EXACTMBEST_KERNEL_GENERIC  every other shape (2 <= X <= 1024): exactmbest_values_generic_kernel; its 5 n_vars + 2
 *                                     vectors in LDS when (5 n_vars + 2) * round_up(X, 2) * 8 + 64 + INTS <=
 *                                     MLBP_CUTSET_GENERIC_LDS_BYTES, else in the caller's workspace
 *   LISTS   a function of the values kernel, (n_vars, P, U, n_forest) and M:
 *     MLBP_EXACTMBEST_KERNEL_X64      the values pass took its X = 64 kernel and
 *                                     n_forest * 33280 + 21 * n_vars * 512 + 64 + INTS + 4 * n_forest * M * 64 * 12 <=
 *                                     MLBP_CUTSET_X64_LDS_BYTES (K3 and K4 at M = 16 fit; a chain of three fits up to M = 5):
 *                                     exactmbest_lists_x64_kernel, grid (B, min(ceil(M / 4), ceil(MLBP_CUTSET_MIN_WORKGROUPS
 *                                     / B))).  The forest's tables in LDS (x64_open); every WAVE solves selected
 *                                     configurations of its own, lane = state, without a workgroup barrier: a lane keeps its
 *                                     list in registers and inserts into it, the side being contracted is broadcast by
 *                                     v_readlane, the root's list is taken by M rounds of a wave maximum and a ballot; a list
 *                                     that outlives a step (a variable that has had a child folded into it) and the
 *                                     back-pointers go to the wave's own LDS behind x64_open's, 12 bytes per forest factor,
 *                                     rank and state.
 *     MLBP_EXACTMBEST_KERNEL_GENERIC  every other shape: exactmbest_lists_generic_kernel, grid (B, M), a workgroup per
 *                                     (graph, selected configuration), threads stride the states, tables streamed.  Its lists
 *                                     are in LDS when MLBP_EXACTMBEST_LISTS_FIXED + INTS + mlbp_exactmbest_lists_bytes(X,
 *                                     n_vars, M) <= MLBP_CUTSET_GENERIC_LDS_BYTES, else in the caller's workspace.
 *           Both state the list form above; in the X = 64 form rank 0 goes through the operations of x64_up<MaxAlg>, so there
 *           F[0] has the bits the X = 64 values kernel gave V_c.
 * INTS = 4 * round_up(P + U + 16, 4).  exactmbest_select_kernel and exactmbest_merge_kernel run in every call. */
#define MLBP_EXACTMBEST_KERNEL_NONE 0
#define MLBP_EXACTMBEST_KERNEL_X64 1
#define MLBP_EXACTMBEST_KERNEL_GENERIC 2
#define MLBP_EXACTMBEST_MAX_M 16
#define MLBP_EXACTMBEST_DROP_BELOW 1000      /* a list entry of rank >= 1 below 2^-1000 of its vector's largest is dropped */
#define MLBP_EXACTMBEST_LISTS_FIXED 384      /* the lists kernel's LDS beside INTS and its lists: scratch, F, R */
#define MLBP_EXACTMBEST_MAX_LISTED 65536     /* the most entries a list holds per graph */
#define MLBP_EXACTMBEST_MAX_CUT 16           /* the most cutset variables of a listed call */

typedef struct mlbp_exactmbest_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_exactmbest_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  int32_t M;                                 /* rows asked for, 1 .. MLBP_EXACTMBEST_MAX_M */
  int32_t N;                                 /* 0: the exact call; 1 .. MLBP_EXACTMBEST_MAX_LISTED: entries listed per graph */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_exactmbest_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  double* workspace;                         /* device, workspace_bytes >= mlbp_exactmbest_workspace_bytes(...) */
  int64_t workspace_bytes;
  int32_t* assignments;                      /* device [B][M][n_vars] */
  double* scores;                            /* device [B][M] */
  int32_t* n_found;                          /* device [B] */
  const int32_t* configs;                    /* listed call: device [B][N][n_cut], the state of cutset[q]; NULL when N == 0 or n_cut == 0 */
  int32_t* entries;                          /* optional device [B][M]: the index of the list entry every row lies under (listed
                                                call) or its configuration number (exact call); -1 for the rows at or beyond
                                                n_found and for a graph that is not computed */
} mlbp_exactmbest_args;

/* Table indices are device data and are not checked on the host: see the edge rules above. */
int mlbp_exactmbest_f64(const mlbp_exactmbest_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_cutset_check_plan, with its messages. */
int mlbp_exactmbest_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: VALUES | LISTS << 4 by the rules above; statuses as mlbp_cutset_pick_kernel, MLBP_EINVAL for M out of range. */
int mlbp_exactmbest_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t M);

/* Host only: C of the values grid (B, C) = min(n_configs, ceil(MLBP_CUTSET_MIN_WORKGROUPS / B)); MLBP_EINVAL for non-positive
 * arguments. */
int mlbp_exactmbest_chunks(int32_t B, int32_t n_configs);

/* Host only: the bytes of a lists task beside its fixed part, with Xp = round_up(X, 2):
 *   round_up(8 * (n_vars * Xp + n_vars * X * M + X * M) + 4 * M * n_vars + 4 * n_vars * X * M + 4 * n_vars * M, 8)
 * -- base, L, C (doubles); the decode's ranks (int32); the back-pointers of the contractions and folds, and of the roots' two
 * (uint16 each). */
int64_t mlbp_exactmbest_lists_bytes(int32_t X, int32_t n_vars, int32_t M);

/* Host only: bytes of workspace a call needs, 8 times
 *   B * n_configs * 2                            every V_c
 *   + B * (M + 1)                                the selected configurations and their number
 *   + B * M * M * 2                              the candidates' value pairs
 *   + ceil(B * M * M * n_vars / 2)               the candidates' assignments (int32)
 *   + B * C * (5 n_vars + 2) * round_up(X, 2)    when the generic values kernel keeps its vectors there
 *   + B * M * lists_bytes / 8                    when the generic lists kernel runs and keeps its lists there
 * with n_configs = X^n_cut; a negative status as pick_kernel / chunks give it, MLBP_EUNSUPPORTED above MLBP_CUTSET_MAX_CONFIGS. */
int64_t mlbp_exactmbest_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut,
                                        int32_t M);

/* Host-side record of the kernels the calling thread's last mlbp_exactmbest_f64 enqueued (VALUES | LISTS << 4; NONE when it was
 * refused before the launch). */
int mlbp_exactmbest_last_kernel(void);

const char* mlbp_exactmbest_arch(void);       /* "gfx950" */
const char* mlbp_exactmbest_last_error(void); /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
