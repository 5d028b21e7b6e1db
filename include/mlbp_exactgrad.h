/* mlbp_exactgrad.h -- C ABI of libmlbp_exactgrad.so: the model's TRUE pairwise marginals, expected features and likelihood
 * gradient of batched factor graphs by cutset conditioning (AMD Instinct MI355X, gfx950, float64).
 *
 * The eighth library of the engine.  The trainer follows `observed features - expected features` with the expectation taken
 * under loopy-BP beliefs; on a graph with a cycle those beliefs are not the model's.  libmlbp_cutset.so gives the model's log Z
 * and single-variable marginals; the gradient needs the marginal of every pairwise FACTOR, which the single-variable
 * marginals do not determine.  This library walks the same configurations over the same packed plan (include/mlbp_cutset.h:
 * its layout, constants and limits are used as they are) and accumulates, beside Z and the marginals, the X * X numbers of
 * every pairwise factor.  It has its own source (macaronicusermodeling_amd/csrc_exactgrad/), its own kernel inventory
 * (exactgrad_*) and its own error slot; it shares no state with the other libraries, runs no sweep program and reads no
 * messages.  Conventions as in mlbp_cutset.h: statuses and a per-thread last error; `stream` is a hipStream_t passed as void*;
 * every buffer is caller-owned device memory; the compute call only ENQUEUES (no allocation, copy or synchronisation), so it
 * may be captured into a HIP graph after one eager call (the first call on a device raises the X = 64 kernels' dynamic-LDS
 * limit); arguments are checked on the host before anything is enqueued; without a device the compute call returns
 * MLBP_ENODEVICE -- there is no CPU fallback.
 *
 * Definitions, per graph g (notation of mlbp_cutset.h: p(x) ~ prod_u U_u[x_var(u)] * prod_p T_p[x_a][x_b], a the variable on
 * table axis 0 of pairwise factor p, b the one on axis 1):
 *   pair_marginals[g][p][i][j] = sum over x with x_a = i, x_b = j of p(x)       the axes are the table's; every block sums to 1
 *   marginals[g][v][s]           the marginal of mlbp_cutset_f64
 *   log_z[g]                     ln Z
 * Features.  phi_en_en and phi_en_en_w1 are [X][X][F_ee], phi_en_de is [X][Vde][F_ed] (row-major, shared by the batch);
 * pair_phi[P] in {0, 1} selects phi_p = phi_en_en (0) or phi_en_en_w1 (1) for pairwise factor p; unary_kind[U] in {0, 1, 2}
 * selects phi_u = phi_en_en, phi_en_en_w1 or phi_en_de for unary factor u, read at the factor's observed column
 * unary_obs[g][u]: phi_u[i][unary_obs[g][u]][:].  With M_p = pair_marginals[g][p] and m_v = marginals[g][v]:
 *   expect_ee[g][f] = sum_p sum_ij M_p[i][j] phi_p[i][j][f]  +  sum over u with kind in {0, 1} of sum_i m_var(u)[i] phi_u[i][obs][f]
 *   expect_ed[g][f] =                                           sum over u with kind = 2      of sum_i m_var(u)[i] phi_u[i][obs][f]
 *   observed_*      = the same sums with the indicator of labels[g] in place of M and m
 *   grad_*          = observed_* - expect_*
 * When the tables are exp(phi . theta), as the trainer builds them, (grad_ee, grad_ed) is the derivative of mlbp_cutset_f64's
 * joint_logp with respect to (theta_en_en, theta_en_de).
 * The unary term uses the variable's TRUE marginal.  The reference's belief of a unary factor is its normalised table alone
 * (oracle/lbp_oracle.py factor_beliefs), so the reference's unary term is not even the BP gradient; this library does not
 * follow it.
 *
 * How the pair marginals are formed.  Under configuration c of the cutset, with weight Z_c and conditional marginals m_c:
 *   - forest factor p between free variable v and its parent: a_c is v's vector on the way up (its own factors times its
 *     children's messages), b_c the parent's context without v (its own factors, its parent's message, its other children's
 *     messages), T~ the table times 2^-e.  The conditional pair marginal is a_c[i] T~[i][j] b_c[j] / (a_c^T T~ b_c) (v on axis
 *     0; transposed otherwise), and T~ does not depend on c, so
 *         M_p = T~ o sum_c (Z_c / (a_c^T T~ b_c)) a_c b_c^T / Z:
 *     one rank-1 update per configuration; the table is applied once, by the combine kernel.
 *   - factor p between free variable v and cutset[q] (a plan item of kind ROW or COL): row or column s_q of M_p gains
 *     Z_c m_c[v][.].
 *   - factor p inside the cutset (a plan const of kind PAIR): cell (s_q0, s_q1) gains Z_c.
 *
 * Range, as mlbp_cutset.h: nothing is rescaled but by powers of two; Z_c, every accumulator and every sum is a mantissa
 * under a running exponent, rescaled by ldexp when a larger Z_c raises it; one logarithm, at the end.  A table times 2^k
 * (|k| <= 400, tables of normal magnitude) changes no bit of pair_marginals, marginals, expect_* or grad_* and moves log_z
 * by k ln 2.
 *
 * Edge rules.  Z = 0: log_z = -inf, every pair block uniform 1 / X^2, every marginal row uniform 1 / X (expect_* is formed from
 * those).  A NaN or +inf entry: that graph's outputs are unspecified and log_z is not finite; every other graph keeps its
 * bits.  A table index outside its array: the graph is not computed -- log_z, expect_* and grad_* NaN, its pair_marginals
 * and marginals left as they were.  A label outside [0, X), an observed column outside [0, X) (kinds 0, 1) or [0, Vde) (kind
 * 2), a unary_kind outside {0, 1, 2}: grad_* NaN for that graph; log_z, pair_marginals, marginals and expect_* are computed,
 * a unary factor whose column or kind is out of range adding nothing to expect_*.
 *
 * Determinism.  The bits of a graph's outputs are a function of the graph, the cutset and C (below): every partial is
 * written by one wave (X = 64) or one workgroup (generic), the partials are added in index order, every cross-lane sum has a
 * fixed shape, and there is no floating-point atomic.
 *
 * The LISTED mode (mlbp_exactgrad_listed_args below, N > 0): an ESTIMATE of everything above beyond the exact limit.  The call is handed a list of N joint states
 * of the cutset per graph -- configs[g][i][q] the state of cutset[q] in entry i, log_q[g][i] the natural log of the probability
 * a proposal gave the entry; the list libmlbp_cutdraw.so draws and libmlbp_cutsetis.so takes -- and walks the list's entries in
 * the place of the X^n_cut configurations.  The bound is on the cutset's size (MLBP_EXACTGRAD_MAX_CUT) and on N
 * (MLBP_EXACTGRAD_MAX_LISTED), not on X^n_cut; the plan is validated by mlbp_cutsetis_check_plan, which states that bound.
 * Semantics: the self-normalised estimator of mlbp_cutsetis.h applied to every output.  With
 *   w_i = Z_{c_i} exp(-log_q[i])              by the one formula of mlbp_cutsetis.h ("Range"), a (mantissa, exponent) pair
 *   log_z          = log_z_hat = ln(sum_i w_i / N)
 *   marginals, pair_marginals, expect_*  = sum_i w_i (the conditional quantity under c_i) / sum_i w_i
 *   grad_*         = observed_* - expect_*
 * The kernels are the exact call's and do what they do there, with w_i where Z_c stands, entry i's row where the digits of the
 * configuration number stand, and the entry index where the configuration number stands: wave w of workgroup (g, k) of the
 * X = 64 kernel walks entries 4 k + w, 4 k + w + 4 C, ..., workgroup (g, k) of the generic kernel entries k, k + C, ..., C by the
 * chunks rule below with N for n_configs; every walker writes a partial of its own, the combine kernel adds them in index order
 * and divides the sum by N for log_z_hat.  Hence:
 *   - a list that holds every configuration in index order with log_q = 0 returns the exact call's bits in every output but
 *     log_z, which is ln(Z / N) = log_z - ln N up to the rounding of one division and one logarithm;
 *   - a table times 2^k moves no bit of the normalised outputs (log_z_hat moves by k ln 2);
 *   - the bits depend on the graph, the cutset, the list and C -- a function of B and N -- alone: not on the graph's position in
 *     the batch, on the other graphs or on B at an equal C.  At another C the walkers group the entries differently and the
 *     sums are the same numbers added in another order (measured: 1e-16 apart).
 * The walk kernel is the exact call's, by the same rule of (X, n_vars, P, U, n_forest): K5 to K9 at X = 64 run on the X = 64
 * kernel, K10 and up and every other X on the generic one.
 * exp(log_z_hat) is an unbiased estimate of Z for a proposal that is positive wherever Z_c is; the normalised outputs are
 * consistent, not unbiased.  The list may repeat a configuration.  n_cut == 0 is valid: every entry is the one empty
 * configuration and `configs` is not read.
 * Edge rules of a list, as in mlbp_cutsetis.h.  A state outside [0, X) in the graph's rows of `configs`, or a log_q that is no
 * finite number or whose magnitude passes MLBP_CUTSETIS_MAX_ABS_LOG_Q (1e6): the graph is refused alone -- log_z, expect_* and
 * grad_* NaN, its pair_marginals and marginals left as they were; every other graph keeps its bits.  An entry is validated
 * before the first address is formed from it: in the exact call a state is a digit of the configuration number and always in
 * range, here it is caller data that selects rows and cells of the accumulators in global memory.  The walker that meets such
 * an entry stops and leaves a NaN as its partial's sum, which is how the combine kernel learns of it; a NaN or +inf table
 * entry that a listed configuration reads and that makes the sum a NaN is refused the same way (the exact call leaves such a
 * graph's outputs unspecified).  Every weight zero: the Z = 0 rule above, log_z_hat = -inf.  A walker without an entry (N
 * smaller than the walkers of its graph) writes an empty partial and touches nothing else.
 * Workspace of a listed call: the formula below with the listed C.  A partial costs X * X doubles per pairwise factor: K5 at
 * X = 64 (ten factors) is 2 + 320 + 40960 doubles = 330 256 bytes, and with four partials per graph (the X = 64 kernel, B large
 * enough for C = 1) a batch of 8192 graphs needs 10.8 GB.  A caller that cannot spare it splits the batch.
 */
#ifndef MLBP_EXACTGRAD_H
#define MLBP_EXACTGRAD_H

#include <stdint.h>

#include "mlbp_cutset.h"                     /* status codes; the plan's layout, constants and limits */

#ifdef __cplusplus
extern "C" {
#endif

/* Which walk kernel a call enqueues -- a function of (X, n_vars, P, U, n_forest) alone, never a user option:
 *   MLBP_EXACTGRAD_KERNEL_X64      X == 64, n_forest <= MLBP_EXACTGRAD_X64_MAX_FOREST and the LDS rule of
 *                                  mlbp_cutset_pick_kernel: n_forest * 33280 + 21 * n_vars * 512 + 64 + INTS <=
 *                                  MLBP_CUTSET_X64_LDS_BYTES.  exactgrad_x64_kernel<max(n_forest, 1)>: the walk of cutset_x64_kernel,
 *                                  every WAVE its own configurations, lane = state.  A wave keeps the 64 x 64 accumulator of
 *                                  each forest factor in registers -- lane = column, 64 doubles per lane, the rank-1 update
 *                                  is 64 FMAs on v_readlane broadcasts -- so at most two forest factors (256 of a lane's 512
 *                                  registers): K3, K4 (one) and a chain of three (two) run here, a chain of four does not.
 *                                  The accumulators of the other pairwise factors are rows of the wave's own partial in
 *                                  the workspace, lane = the free variable's state.
 *   MLBP_EXACTGRAD_KERNEL_GENERIC  every other shape (2 <= X <= 1024): exactgrad_generic_kernel, the walk of
 *                                  cutset_generic_kernel, the workgroup one configuration at a time, every accumulator in
 *                                  the workgroup's partial; its 5 n_vars + 2 vectors in LDS when they fit
 *                                  MLBP_CUTSET_GENERIC_LDS_BYTES, else in the workspace, as there.
 * INTS = 4 * round_up(P + U + 16, 4).
 *
 * Grid (B, C), C = mlbp_exactgrad_chunks(B, n_configs, kernel) =
 *   min(n_walkers, ceil(MLBP_EXACTGRAD_MIN_WORKGROUPS / B)),   n_walkers = ceil(n_configs / 4) (X = 64) or n_configs (generic):
 * a partial costs X * X doubles per pairwise factor here, so no workgroup is given partials without a configuration, and a graph
 * is spread over one workgroup per CU, not two.  Workgroup (g, k) of the generic kernel walks configurations k, k + C, ...;
 * wave w of workgroup (g, k) of the X = 64 kernel walks 4 k + w, 4 k + w + 4 C, ... and writes partial 4 k + w: the four waves'
 * accumulators are NOT merged on chip.  A partial is
 *   {sum of Z_c mantissas, exponent, marginal accumulators [n_vars][X], pair accumulators [P][X][X]}
 * (a partial whose exponent says "empty" holds nothing else), the pair accumulator of a forest factor and of a factor inside
 * the cutset in table axes, that of a ROW / COL factor as [s_q][state of the free variable].
 * exactgrad_combine_kernel, one workgroup per graph (no (graph, factor) grid), adds the partials in index order, applies T~
 * to the forest factors, divides by Z, writes the requested tensors and contracts the same numbers with phi, eight features
 * at a time: when pair_marginals is not requested only F_ee + F_ed numbers per graph leave it. */
#define MLBP_EXACTGRAD_KERNEL_NONE 0
#define MLBP_EXACTGRAD_KERNEL_X64 1
#define MLBP_EXACTGRAD_KERNEL_GENERIC 2
#define MLBP_EXACTGRAD_X64_MAX_FOREST 2
#define MLBP_EXACTGRAD_MIN_WORKGROUPS 256
#define MLBP_EXACTGRAD_MAX_FEATURES 64       /* F_ee and F_ed, each */
#define MLBP_EXACTGRAD_MAX_LISTED 65536      /* entries per graph of a listed call */
#define MLBP_EXACTGRAD_MAX_CUT 16            /* cutset variables of a listed call: the walk keeps a configuration's states in 16 integers */

typedef struct mlbp_exactgrad_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_exactgrad_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  int32_t F_ee, F_ed, Vde;                   /* features per en_en / en_de factor, columns of phi_en_de */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_exactgrad_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const double* phi_en_en;                   /* device [X][X][F_ee]; the feature inputs are needed by expect_* and grad_* */
  const double* phi_en_en_w1;                /* device [X][X][F_ee] */
  const double* phi_en_de;                   /* device [X][Vde][F_ed] */
  const int32_t* pair_phi;                   /* device [P] in {0, 1} (NULL when P == 0) */
  const int32_t* unary_kind;                 /* device [U] in {0, 1, 2} (NULL when U == 0) */
  const int32_t* unary_obs;                  /* device [B][U] (NULL when U == 0) */
  const int32_t* labels;                     /* device [B][n_vars]; needed by grad_* */
  double* workspace;                         /* device, workspace_bytes >= mlbp_exactgrad_workspace_bytes(...) */
  int64_t workspace_bytes;
  double* log_z;                             /* device [B] */
  double* marginals;                         /* optional device [B][n_vars][X] */
  double* pair_marginals;                    /* optional device [B][P][X][X] */
  double* expect_ee;                         /* optional device [B][F_ee] */
  double* expect_ed;                         /* optional device [B][F_ed] */
  double* grad_ee;                           /* optional device [B][F_ee] */
  double* grad_ed;                           /* optional device [B][F_ed] */
} mlbp_exactgrad_args;

/* The arguments of a LISTED call: the exact call's, and the list behind them.  mlbp_exactgrad_args itself keeps the layout and
 * the size it has always had; a listed call hands mlbp_exactgrad_f64 the address of `args` below with args.plan_words NEGATED
 * (-plan_words: no exact call has one below zero), which tells the library that the list lies behind the struct it was handed.
 * N == 0 there is the exact call once more: configs and log_q are not looked at, whatever they hold. */
typedef struct mlbp_exactgrad_listed_args {
  mlbp_exactgrad_args args;                  /* as in the exact call, but for the sign of plan_words */
  const int32_t* configs;                    /* device [B][N][n_cut], the state of cutset[q] (may be NULL when n_cut == 0) */
  const double* log_q;                       /* device [B][N], ln of the proposal's probability of the entry */
  int32_t N;                                 /* 0: the exact call; 1 .. MLBP_EXACTGRAD_MAX_LISTED: entries listed per graph */
} mlbp_exactgrad_listed_args;

/* Table indices, labels, observed columns and selectors are device data and are not checked on the host: see the edge rules.
 * MLBP_EINVAL: bad sizes, a missing array, a requested expect_* or grad_* without the feature inputs (F_ee, F_ed, Vde >= 1),
 * a requested grad_* without labels, a workspace that is too small, N outside [0, MLBP_EXACTGRAD_MAX_LISTED], a listed call
 * without log_q or (n_cut > 0) without configs.  MLBP_EUNSUPPORTED: X > MLBP_CUTSET_MAX_X, X^n_cut > MLBP_CUTSET_MAX_CONFIGS
 * (the exact call) or n_cut > MLBP_EXACTGRAD_MAX_CUT (a listed call), F_ee or F_ed > MLBP_EXACTGRAD_MAX_FEATURES. */
int mlbp_exactgrad_f64(const mlbp_exactgrad_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_cutset_check_plan, with its messages. */
int mlbp_exactgrad_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: MLBP_EXACTGRAD_KERNEL_X64 or _GENERIC by the rule above; statuses as mlbp_cutset_pick_kernel. */
int mlbp_exactgrad_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest);

/* Host only: C of the grid (B, C) by the rule above for kernel = MLBP_EXACTGRAD_KERNEL_X64 or _GENERIC; MLBP_EINVAL for
 * non-positive sizes or another kernel. */
int mlbp_exactgrad_chunks(int32_t B, int32_t n_configs, int32_t kernel);

/* Host only: bytes of workspace a call needs, 8 times
 *   B * parts * (2 + n_vars * X + P * X * X)            parts = C (generic) or 4 C (X = 64)
 *   + B * C * (5 n_vars + 2) * round_up(X, 2)           when the generic kernel keeps its vectors there
 * with n_configs = X^n_cut; a negative status as pick_kernel / chunks give it, MLBP_EUNSUPPORTED above MLBP_CUTSET_MAX_CONFIGS.
 * This states the exact call; a listed call needs the same formula with C = mlbp_exactgrad_chunks(B, N, kernel). */
int64_t mlbp_exactgrad_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut);

/* Host-side record of the walk kernel the calling thread's last mlbp_exactgrad_f64 enqueued (MLBP_EXACTGRAD_KERNEL_*; NONE
 * when it was refused before the launch). */
int mlbp_exactgrad_last_kernel(void);

const char* mlbp_exactgrad_arch(void);       /* "gfx950" */
const char* mlbp_exactgrad_last_error(void); /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
