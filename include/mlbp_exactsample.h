/* mlbp_exactsample.h -- C ABI of libmlbp_exactsample.so: whole assignments drawn from the MODEL ITSELF for batched factor graphs,
 * by cutset conditioning (AMD Instinct MI355X, gfx950, float64).
 *
 * The ninth library of the engine.  libmlbp_sample.so draws by sequential conditioning on top of loopy sweeps: exact on a
 * tree, a proposal q with its log q on a graph with a cycle.  This one draws from
 *     p(x)  ~  prod_u U_u[x_var(u)]  *  prod_p T_p[x_a][x_b]
 * itself, the way libmlbp_cutset.so sums it and libmlbp_exactmap.so maximises it: the returned logp is log p(x) = score(x) -
 * log Z for every draw, on loopy graphs too.  It has its own source (macaronicusermodeling_amd/csrc_exactsample/), its own
 * kernel inventory (exactsample_*) and its own error slot; it shares no state with the other libraries.  It runs no sweep
 * program and reads no messages.  It takes the SAME packed plan as mlbp_cutset_f64 (include/mlbp_cutset.h states its layout, the
 * cutset choice and what the check refuses; the MLBP_CUTSET_* plan constants and limits are the ones used here).
 *
 * Conventions, as in mlbp_cutset.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_exactsample_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory unless stated; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be
 * captured into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64 kernels'
 * dynamic-LDS limit, a host-side attribute call); arguments are checked on the host before anything is enqueued.  There is no
 * CPU fallback: without a device the compute call returns MLBP_ENODEVICE.  The random numbers come from the caller and the
 * kernels hold no generator: a call is a pure function of its arguments.
 *
 * THE DRAW RULE, used for the configuration and for every free variable alike.  Given weights a_0 .. a_{n-1} >= 0, their
 * inclusive prefix sums A_i, the total A = A_{n-1} and a uniform u in [0, 1): with t = u * A (one rounded product),
 *     the draw is the lowest i with A_i > t and a_i > 0;  when there is none, the highest i with a_i > 0
 * (mlbp_sample.h step 4's rule: an index of weight zero is never drawn); its probability is a_i / A.  The prefix sums are
 * formed in float64 by a procedure that depends on n and on the kernel alone -- never on B, S or the grid:
 *   SEGMENTED (the configurations; a variable's states in the generic kernel): with L = ceil(n / 256), index i belongs to
 *       segment i div L; tot_s = the entries of segment s added left to right; O_0 = 0, O_{s+1} = O_s + tot_s; A_i = O_s +
 *       (a_{sL} + ... + a_i, added left to right).  These A_i never decrease, so "a_i > 0" adds nothing to "A_i > t".  For
 *       n <= 256 this is the plain running sum.
 *   WAVE (a variable's 64 states in the X = 64 kernel): within each row of 16 lanes the Hillis-Steele steps at distances 1, 2,
 *       4, 8 (A_i += A_{i-d}, lanes without a partner add nothing); then row r adds R_0 + .. + R_{r-1}, R the rows' totals,
 *       added left to right.  These A_i may fall short of monotone by a rounding; the condition a_i > 0 keeps the rule's promise.
 *
 * Semantics of one call.  For graph g and sample s, with the plan, Z_c, the power-of-two rescaling and the conditioning rules
 * exactly as mlbp_cutset.h defines them:
 *   1. Configuration.  When n_cut > 0: every Z_c is a (mantissa, exponent) pair; E = the largest exponent of a Z_c with a
 *      positive mantissa; w_c = mantissa_c * 2^max(exponent_c - E, -4000); W_c = their SEGMENTED prefix sums in configuration
 *      order.  c is drawn by the rule above from w with u = uniforms[s][g][0], and logp = log(w_c / W_last).  Every cutset
 *      variable takes its digit of c.  With n_cut == 0 there is the one empty configuration, no uniform is used and logp = 0.
 *      log_z = E ln 2 + log(W_last) either way (-inf when W_last == 0).
 *   2. Free variables.  The conditioned forest is solved by one pass from the leaves to the roots under c.  Then the free
 *      variables are walked in REVERSE `order`, so every variable comes after its parent.  For the k-th one, v:
 *        b = v's vector on the way up (its unary rows, its cutset-incident rows and columns under c, its children's messages;
 *            rescaled by a power of two), and for a non-root v, elementwise times the row or column of its parent factor's
 *            (rescaled) table at the parent's drawn state;
 *        x_v is drawn from b by the rule above with u = uniforms[s][g][n_cut + k];   logp += log(b[x_v] / sum b),
 *      sum b the last prefix sum.
 *   3. Outputs.  samples[s][g][v] (int32, v in variable-index order), logp[s][g], optionally log_z[g] and score[s][g] = the
 *      log-potential of the draw, the score of mlbp_map.h: the sum of the logarithms of the table entries at the draw.
 * The product of the probabilities used is p(x) exactly, so logp = score - log_z up to rounding, for every draw and any valid
 * cutset.  The empty cutset on a forest is the exact forward-filtering / backward-sampling algorithm.
 *
 * Uniforms.  [S][B][n_vars], each in [0, 1): the shape mlbp_sample_f64 takes.  Entry 0 draws the configuration, entries
 * 1 .. n_cut-1 are not read, entry n_cut + k draws the k-th free variable of the reverse order.
 *
 * Range and determinism.  Nothing is rescaled but by powers of two, by exponent extraction, as in mlbp_cutset.h.  So a table
 * times 2^k (|k| <= 400, tables of normal magnitude) changes no sample and no bit of logp, and moves log_z and score by
 * k ln 2 up to the rounding of the logarithm.  Z_c is computed per configuration and never merged across configurations
 * before the scan, and a sample is computed by one wave (X = 64) or one workgroup from its own uniforms: the bits of
 * samples, logp, score and log_z are a function of the graph, the cutset and the sample's uniforms alone -- not of B, S, the
 * graph's position in the batch or the grid.
 *
 * Edge rules.  Z == 0 (an all-zero table, say), a Z that is not finite (a NaN or +inf entry), or a table index outside its
 * array: the graph's samples are -1 everywhere, its logp and score NaN; log_z is -inf, not a finite number, NaN respectively,
 * as mlbp_cutset.h gives it; every other graph keeps its bits.  A uniform outside [0, 1) or NaN still draws a state in range.
 * Limits: X^n_cut <= MLBP_CUTSET_MAX_CONFIGS, X <= MLBP_CUTSET_MAX_X (MLBP_EUNSUPPORTED beyond).
 *
 * THE LISTED MODE (N > 0): draws for the graphs whose cutset has more than MLBP_CUTSET_MAX_CONFIGS configurations, by
 * sampling-importance-resampling over a caller's LIST of cutset states.  The caller lists N joint states of the cutset per
 * graph, configs[g][i][q] = the state of cut position q in entry i, with log_q[g][i] = the natural logarithm of the probability
 * a proposal gave that state (mlbp_cutsetis.h takes the same list; mlbp_cutdraw.h makes one).  N == 0 is the exact call above,
 * whatever configs, log_q, entry and ess hold: they are not looked at.  In a listed call the plan is the one
 * mlbp_cutsetis_check_plan admits: at most 16 cutset variables and no bound on X^n_cut.
 *   1'. Weights.  Entry i has w_i = Z_{c_i} * exp(-log_q[i]), Z_c of the entry's states as above and exp(-log_q) = r 2^k by THE
 *      formula of mlbp_cutsetis.h: k = rint(-log_q / ln 2), r = exp(-log_q - k ln 2); the product's mantissa is brought back to
 *      [1, 2).  Every weight is kept apart as a (mantissa, exponent) pair; none is merged with another before the scan.
 *   2'. Scan.  E = the largest exponent of a positive weight; w_i under E with the floor of step 1 (2^-4000); W_i = their
 *      SEGMENTED prefix sums over n = N, in list order.  log_z reads log_z_hat = E ln 2 + log(W_last / N), the estimate of
 *      mlbp_cutsetis.h (-inf when W_last == 0).  ess = W_last^2 / sum of w_i^2 under the same E (the squares of a thread's
 *      segment added left to right, the segments' sums in order; 0 when W_last == 0): the effective size of the list, N when
 *      every weight is equal.
 *   3'. Draw.  uniforms[s][g][0] picks the entry by the draw rule on w: entry i with probability w_i / W_last; an entry of
 *      weight zero is never drawn; the list may repeat a state.  The cutset variables take the entry's row of configs, the
 *      free variables are drawn as in step 2 from uniforms[s][g][n_cut + k].  logp = log(w_i / W_last) + the sum of the
 *      logarithms of the conditionals: the log-probability of the draw GIVEN THE LIST and the entry, so that
 *          logp = score - log_q[entry] - (log_z_hat + log N)     up to rounding,
 *      and score - log_z_hat is the estimate of log p(x) of the draw.  entry[s][g] is the drawn index.
 *   n_cut == 0: every entry is the one empty configuration; configs is not read, entry 0 is reported, no uniform is spent on
 *      it and samples and logp are the exact call's; log_z_hat and ess come from the listed weights.
 * The draws follow sum_i (w_i / W_last) p(x | c_i), which tends to the model as N grows for a proposal that is positive
 * wherever Z_c is; ess says how far the list is from that.  With the full list in index order and log_q = 0 every bit of
 * samples, logp and score is the exact call's, and log_z_hat = log_z - log N.
 * Edge rules of a listed call.  A state outside [0, X), a log_q that is not finite or beyond MLBP_CUTSETIS_MAX_ABS_LOG_Q in
 * magnitude, a table index outside its array: the entry's weight is marked with a NaN mantissa -- it is never used as an index
 * -- and the graph is refused alone: samples -1, entry -1, logp, score, log_z_hat and ess NaN.  Every listed weight zero:
 * samples -1, entry -1, logp and score NaN, log_z_hat = -inf, ess = 0.  A weight that is no finite number (a NaN or +inf table
 * entry): samples -1, entry -1, logp and score NaN, log_z_hat and ess no finite numbers.  Every other graph keeps its bits.
 * Determinism of a listed call.  The bits of every output are a function of the graph, the cutset, the list and the sample's
 * uniforms alone -- not of B, S, the graph's position in the batch or the grid.  A table times 2^k changes no sample and no bit
 * of logp, entry or ess.
 *
 * Not done: a `given=` argument (clamped variables); float32 tables; one grouped launch over several shapes; the MODEL'S OWN
 * distribution for cutsets beyond MLBP_CUTSET_MAX_CONFIGS configurations -- the listed mode draws from its estimate over a
 * list; a list made inside the call.
 */
#ifndef MLBP_EXACTSAMPLE_H
#define MLBP_EXACTSAMPLE_H

#include <stdint.h>

#include "mlbp_cutset.h"                     /* status codes; the plan's layout, constants and limits */

#ifdef __cplusplus
extern "C" {
#endif

/* A call enqueues three launches, whatever the sizes: the weights pass, the scan, the draw pass.  Which form the first and
 * the third take is the rule of mlbp_cutset_pick_kernel, a function of (X, n_vars, P, U, n_forest) alone, with the same
 * constants (INTS = 4 * round_up(P + U + 16, 4)):
 *   MLBP_EXACTSAMPLE_KERNEL_X64      X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + INTS <= MLBP_CUTSET_X64_LDS_BYTES
 *                                    (the LDS carve-up of the walk the cutset libraries share; the draw pass leaves the
 *                                    accumulator rows unused): K3, K4 and a chain of three fit, a chain of four does not; K3
 *                                    and K4 take under 80 KB, so two workgroups share a CU's 160 KB.  The forest's tables in
 *                                    LDS, rows of 65, rescaled once, for the whole launch; every WAVE walks configurations
 *                                    (exactsample_weights_x64_kernel) or draws samples (exactsample_draw_x64_kernel) of its own,
 *                                    lane = state, without a workgroup barrier.  The configuration is found by a binary search
 *                                    on the scanned weights; a state is drawn by the WAVE scan on DPP, a ballot for the lowest
 *                                    crossing lane and a readlane of the drawn state; the parent factor's row or column comes
 *                                    from the LDS copy.
 *   MLBP_EXACTSAMPLE_KERNEL_GENERIC  every other shape (2 <= X <= 1024): exactsample_weights_generic_kernel and
 *                                    exactsample_draw_generic_kernel, one workgroup per (graph, chunk), tables streamed, the
 *                                    SEGMENTED scan per state draw; its 5 n_vars + 2 vectors of X entries (the shared carve-up)
 *                                    in LDS when (5 n_vars + 2) * round_up(X, 2) * 8 + 64 + INTS <=
 *                                    MLBP_CUTSET_GENERIC_LDS_BYTES, else in the caller's workspace.
 * exactsample_scan_kernel, one workgroup per graph, brings the Z_c to the graph's largest exponent, scans them and writes log_z.
 * A listed call enqueues the same three launches of the same five kernels with n_configs = N: the weights kernels walk the
 * list's entries in a loop of their own, the scan adds ess, the draw kernels read the drawn entry's row.
 *
 * Grids.  With chunks(B, n) = mlbp_exactsample_chunks(B, n) = min(n, ceil(MLBP_CUTSET_MIN_WORKGROUPS / B)):
 *   weights pass  (B, Cw), Cw = chunks(B, n_configs): workgroup (g, k) of the generic kernel walks configurations k, k + Cw, ...,
 *                 wave w of workgroup (g, k) of the X = 64 kernel 4 k + w, 4 k + w + 4 Cw, ...; each writes its Z_c pairs.
 *   draw pass     (B, Cd): generic Cd = chunks(B, S), workgroup (g, k) draws samples k, k + Cd, ...; X = 64
 *                 Cd = chunks(B, ceil(S / 4)), wave w of workgroup (g, k) draws samples 4 k + w, 4 k + w + 4 Cd, ...
 * A large batch reads every table once per pass whatever S is, a small one spreads its work over the machine. */
#define MLBP_EXACTSAMPLE_KERNEL_NONE 0
#define MLBP_EXACTSAMPLE_KERNEL_X64 1
#define MLBP_EXACTSAMPLE_KERNEL_GENERIC 2
#define MLBP_EXACTSAMPLE_HEAD 4              /* doubles per graph between the scan and the draw pass */
#define MLBP_EXACTSAMPLE_MAX_LISTED 65536    /* the most entries a listed call takes per graph */

typedef struct mlbp_exactsample_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_exactsample_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  int32_t S;                                 /* samples per graph */
  int32_t N;                                 /* 0: the exact call; 1 .. MLBP_EXACTSAMPLE_MAX_LISTED: entries listed per graph */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_exactsample_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] table of graph g's pairwise factor p */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const double* uniforms;                    /* device [S][B][n_vars], each in [0, 1) */
  const int32_t* configs;                    /* listed: device [B][N][n_cut] (NULL when n_cut == 0) */
  const double* log_q;                       /* listed: device [B][N] */
  double* workspace;                         /* device, workspace_bytes >= mlbp_exactsample_workspace_bytes(...) */
  int64_t workspace_bytes;
  int32_t* samples;                          /* device [S][B][n_vars] */
  double* logp;                              /* device [S][B] */
  double* log_z;                             /* optional device [B] */
  double* score;                             /* optional device [S][B] */
  int32_t* entry;                            /* listed, optional: device [S][B] the drawn entry */
  double* ess;                               /* listed, optional: device [B] */
} mlbp_exactsample_args;

/* Table indices, and a list's states and log_q, are device data and are not checked on the host: see the edge rules above.
 * Host checks of a listed call: N in [1, MLBP_EXACTSAMPLE_MAX_LISTED] (MLBP_EINVAL), configs non-NULL when n_cut > 0, log_q
 * non-NULL, n_cut <= 16 (MLBP_EUNSUPPORTED), the workspace. */
int mlbp_exactsample_f64(const mlbp_exactsample_args* args, void* stream);

/* Host only, no GPU needed: the checks of mlbp_cutset_check_plan, with its messages. */
int mlbp_exactsample_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: MLBP_EXACTSAMPLE_KERNEL_X64 or _GENERIC by the rule above; statuses as mlbp_cutset_pick_kernel. */
int mlbp_exactsample_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest);

/* Host only: min(n, ceil(MLBP_CUTSET_MIN_WORKGROUPS / B)), the rule of both grids; MLBP_EINVAL for non-positive arguments. */
int mlbp_exactsample_chunks(int32_t B, int32_t n);

/* Host only: bytes of workspace a call needs, 8 times
 *   B * n_configs * 3                                     every Z_c as (mantissa, exponent), and the scanned weights
 *   + B * MLBP_EXACTSAMPLE_HEAD                           per graph {E, W_last, usable, 0}
 *   + B * max(Cw, Cd) * (5 n_vars + 2) * round_up(X, 2)   when the generic kernels keep their vectors there
 * with n_configs = X^n_cut and Cw, Cd as above; a negative status as pick_kernel / chunks give it, MLBP_EINVAL for S <= 0,
 * MLBP_EUNSUPPORTED above MLBP_CUTSET_MAX_CONFIGS.  This is the exact call's; a LISTED call needs the same sum with N in the
 * place of n_configs -- B * N * 3 + B * MLBP_EXACTSAMPLE_HEAD {E, W_last, usable, sum of w^2} + the vectors' share with
 * Cw = chunks(B, N) -- which the compute entry checks (the binding states it: exactsample.listed_workspace_bytes). */
int64_t mlbp_exactsample_workspace_bytes(int32_t B, int32_t S, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest,
                                         int32_t n_cut);

/* Host-side record of the kernel form the calling thread's last mlbp_exactsample_f64 enqueued (MLBP_EXACTSAMPLE_KERNEL_*; NONE
 * when it was refused before the launch). */
int mlbp_exactsample_last_kernel(void);

const char* mlbp_exactsample_arch(void);        /* "gfx950" */
const char* mlbp_exactsample_last_error(void);  /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
