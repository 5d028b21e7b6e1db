/* mlbp_cutsetis.h -- C ABI of libmlbp_cutsetis.so: an ESTIMATE of log Z and of the marginals of batched factor graphs by
 * cutset importance sampling (AMD Instinct MI355X, gfx950, float64).
 *
 * The eleventh library of the engine, a sibling of libmlbp_cutset.so on the same packed plan (include/mlbp_cutset.h: the
 * plan's layout, the item and const kinds, Z_c and m_c).  The sixth library sums every configuration of the cutset and
 * refuses more than 65536 of them; this one is handed a LIST of N configurations per graph with the probability a proposal q
 * gave each, solves the conditioned forest exactly for each entry (the same walk: the Rao-Blackwellised step of w-cutset
 * importance sampling, Bidyuk and Dechter) and weights the results by Z_c / q(c).  It bounds the number of cutset variables
 * (MLBP_CUTSETIS_MAX_CUT) and not X^|C|.  It has its own source (macaronicusermodeling_amd/csrc_cutsetis/), its own kernel
 * inventory (cutsetis_*) and its own error slot; it shares no state with the other libraries.
 *
 * Conventions, as in mlbp_cutset.h: functions return MLBP_OK or a negative status and leave a message for
 * mlbp_cutsetis_last_error() (per thread); `stream` is a hipStream_t passed as void*; every buffer is caller-owned device
 * memory; the compute call only ENQUEUES -- no allocation, no copy and no synchronisation inside it, so it may be captured
 * into a HIP graph and replayed (after one eager call: the first call on a device raises the X = 64 kernel's dynamic-LDS
 * limit); arguments are checked on the host before anything is enqueued.  There is no CPU fallback: without a device the
 * compute call returns MLBP_ENODEVICE.
 *
 * Semantics of one call, per graph.  Entry i of the graph's list is a configuration c_i -- configs[g][i][q] is the state of
 * cutset[q]; the list may repeat a configuration -- and log_q[g][i] = ln q(c_i).  Z_c and m_c are those of mlbp_cutset.h.
 *   w_i                = Z_{c_i} * exp(-log_q[i])            S1 = sum_i w_i        S2 = sum_i w_i^2
 *   log_z_hat          = ln S1 - ln N
 *   ess                = S1^2 / S2                           (0 when S1 = 0)
 *   free variable v:     marginal[v] = sum_i w_i m_{c_i}[v] / S1
 *   cutset variable a:   marginal[a][s] = sum_{i : state of a = s} w_i / S1
 *   log_w[i]           = ln Z_{c_i} - log_q[i]               (optional; -inf for Z_c = 0)
 *   score, joint_logp  = the score of mlbp_cutset.h at `labels`, and score - log_z_hat
 * exp(log_z_hat) is an unbiased estimate of Z for any q that is positive wherever Z_c is.  The marginals are self-normalised:
 * consistent, not unbiased.  ess / N near 1 says the proposal is close to Z_c / Z; the relative standard error of the
 * estimate of Z that ess implies is sqrt(1 / ess - 1 / N).
 *
 * Range.  As in mlbp_cutset.h: nothing is rescaled but by powers of two.  Z_c comes out of the walk as a (mantissa,
 * exponent) pair, and exp(-log_q) is brought into that form by ONE formula,
 *     k = rint(-log_q / ln 2)        r = exp(-log_q - k ln 2)        exp(-log_q) = r * 2^k,   r in [2^-1/2, 2^1/2],
 * so w_i = (Z mantissa * r, renormalised to [1, 2)) * 2^(Z exponent + k).  S1 and the marginal accumulators run under the
 * largest exponent seen, S2 under twice that exponent, through both combine steps; a logarithm is taken once per output:
 *     log_w[i] = e_i ln 2 + ln m_i  of w_i = m_i 2^e_i;     log_z_hat = E ln 2 + ln(M / N)  of S1 = M 2^E.
 * So a table times 2^k changes no bit of `marginals` and `ess` and moves log_z_hat and log_w by k ln 2.
 *
 * Edge rules.  S1 = 0 (every listed Z_c is zero): log_z_hat = -inf, every marginal row uniform 1/X, ess = 0.  A state outside
 * [0, X) in the graph's rows of `configs`, a log_q that is not a finite number or whose magnitude passes
 * MLBP_CUTSETIS_MAX_ABS_LOG_Q, or a table index outside its array: the graph is not computed -- log_z_hat, ess, score and
 * joint_logp NaN, its marginals left as they were, its log_w unspecified (NaN at the offending entries).  A NaN or +inf table
 * entry that a listed configuration reads (a list reads the cutset's rows and constants at its own states only): log_z_hat of
 * that graph is not a finite number, its marginals and ess are unspecified.  A label outside [0, X):
 * score and joint_logp NaN, the rest computed.  In every case the call returns and every other graph keeps its bits.
 * n_cut = 0 (a forest) is valid: every entry is then the one empty configuration, `configs` is not read, and with
 * log_q = 0 log_z_hat is log Z.
 *
 * Kernels.  The pick is the sixth library's, a function of (X, n_vars, P, U, n_forest) alone:
 *   MLBP_CUTSETIS_KERNEL_X64      X == 64 and the LDS rule of MLBP_CUTSET_KERNEL_X64 (on K_n: n <= 9).  The forest's tables
 *                                 are in LDS; every WAVE walks list entries of its own, no workgroup barrier in the walk.
 *   MLBP_CUTSETIS_KERNEL_GENERIC  every other shape, 2 <= X <= 1024: a workgroup per entry, tables streamed, vectors in LDS
 *                                 or in the workspace by the rule of MLBP_CUTSET_KERNEL_GENERIC.
 * Both run on a grid of (B, C) workgroups, C = mlbp_cutsetis_chunks(B, N) = min(N, ceil(MLBP_CUTSETIS_MIN_WORKGROUPS / B)).
 * Workgroup (g, k) of the generic kernel walks entries k, k + C, ... of graph g and writes partial k; wave w of workgroup
 * (g, k) of the X = 64 kernel walks entries 4 k + w, 4 k + w + 4 C, ... and writes partial 4 k + w.  A partial is
 *     {S1 mantissa, exponent E, the accumulated marginal mantissas [n_vars][X] under E, S2 mantissa under 2 E}
 * = n_vars * X + 3 doubles; a walker without an entry writes {0, the empty exponent, zeros, 0}.  log_w[i] is written by the
 * walker as entry i is solved.  cutsetis_combine_kernel, one workgroup per graph, adds the C (4 C) partials in index order and
 * writes the outputs.  The bits of a graph's outputs are a function of the graph, the cutset, its list and C.
 */
#ifndef MLBP_CUTSETIS_H
#define MLBP_CUTSETIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: the values of mlbp.h.  A translation unit that uses several headers includes this one last. */
#if !defined(MLBP_H) && !defined(MLBP_MAP_H) && !defined(MLBP_LOGZ_H) && !defined(MLBP_SAMPLE_H) && !defined(MLBP_CONVERGE_H) && !defined(MLBP_CUTSET_H)
enum { MLBP_OK = 0, MLBP_EINVAL = -1, MLBP_EHIP = -2, MLBP_ENODEVICE = -3, MLBP_ENOMEM = -4, MLBP_EUNSUPPORTED = -5 };
#endif

#define MLBP_CUTSETIS_KERNEL_NONE 0
#define MLBP_CUTSETIS_KERNEL_X64 1
#define MLBP_CUTSETIS_KERNEL_GENERIC 2
#define MLBP_CUTSETIS_MAX_LISTED 65536
#define MLBP_CUTSETIS_MAX_CUT 16
#define MLBP_CUTSETIS_MIN_WORKGROUPS 512
#define MLBP_CUTSETIS_MAX_ABS_LOG_Q 1.0e6

typedef struct mlbp_cutsetis_args {
  int32_t B, X, n_vars, P, U;                /* graphs, states, variables, pairwise / unary factors */
  int32_t n_cut, n_free, n_items, n_consts, n_forest;      /* the plan's header, as mlbp_cutsetis_check_plan saw it */
  int32_t n_pair_tables, n_unary_tables;
  int32_t plan_words;
  int32_t N;                                 /* configurations listed per graph, 1 <= N <= MLBP_CUTSETIS_MAX_LISTED */
  const int32_t* plan;                       /* device [plan_words], validated by mlbp_cutsetis_check_plan before upload */
  const double* pair_tables;                 /* device [n_pair_tables][X][X] row-major (NULL when P == 0) */
  const int32_t* pair_tab;                   /* device [B][P] */
  const double* unary_tables;                /* device [n_unary_tables][X] (NULL when U == 0) */
  const int32_t* unary_tab;                  /* device [B][U] */
  const int32_t* configs;                    /* device [B][N][n_cut]: entry q is the state of cutset[q] (may be NULL when n_cut == 0) */
  const double* log_q;                       /* device [B][N]: ln of the proposal's probability of the configuration */
  const int32_t* labels;                     /* optional device [B][n_vars]; needed by score and joint_logp */
  double* workspace;                         /* device, workspace_bytes >= mlbp_cutsetis_workspace_bytes(...) */
  int64_t workspace_bytes;
  double* log_z_hat;                         /* device [B] */
  double* marginals;                         /* device [B][n_vars][X] */
  double* ess;                               /* device [B] */
  double* log_w;                             /* optional device [B][N] */
  double* score;                             /* optional device [B] */
  double* joint_logp;                        /* optional device [B] */
} mlbp_cutsetis_args;

/* Table indices, states, log_q and labels are device data and are not checked on the host: see the edge rules above. */
int mlbp_cutsetis_f64(const mlbp_cutsetis_args* args, void* stream);

/* Host only, no GPU needed: mlbp_cutset_check_plan without its bound on X^n_cut.  The bound here is the walk's own: n_cut above
 * MLBP_CUTSETIS_MAX_CUT (the generic walker keeps a configuration's states in 16 integers) and X > 1024 are
 * MLBP_EUNSUPPORTED; everything else mlbp_cutset_check_plan refuses is refused with the same words. */
int mlbp_cutsetis_check_plan(const int32_t* plan, int32_t n_words, int32_t X);

/* Host only: MLBP_CUTSETIS_KERNEL_X64 or _GENERIC, the rule and the refusals of mlbp_cutset_pick_kernel. */
int mlbp_cutsetis_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest);

/* Host only: C of the grid (B, C) by the rule above; MLBP_EINVAL for B <= 0 or N outside [1, MLBP_CUTSETIS_MAX_LISTED]. */
int mlbp_cutsetis_chunks(int32_t B, int32_t N);

/* Host only: bytes of workspace a call needs -- B * C * (n_vars * X + 3) * 8 for the partials of the generic kernel, four times
 * that on the X = 64 kernel, plus B * C * (5 n_vars + 2) * round_up(X, 2) * 8 behind the partials when the generic kernel keeps
 * its vectors there; formed in 64 bits; a negative status as mlbp_cutsetis_pick_kernel / mlbp_cutsetis_chunks give it. */
int64_t mlbp_cutsetis_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t N);

/* Host-side record of the kernel the calling thread's last mlbp_cutsetis_f64 enqueued (MLBP_CUTSETIS_KERNEL_*; NONE when it
 * was refused before the launch). */
int mlbp_cutsetis_last_kernel(void);

const char* mlbp_cutsetis_arch(void);        /* "gfx950" */
const char* mlbp_cutsetis_last_error(void);  /* message of the calling thread's last failed call */

#ifdef __cplusplus
}
#endif

#endif
