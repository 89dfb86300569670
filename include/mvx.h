/*
 * mvx.h -- C ABI of the MI355X dense-simplex LP-relaxation engine (libmvolps_amd.so).
 *
 * Drop-in boundary: MVOLPS talks to its LP engine only through the GLPK C API
 * (SURVEY.md section 8(b)).  Every entry point below replaces the glp_* call named next
 * to it (file:line under /root/reference); semantics, 1-based indexing, "element 0
 * ignored" array convention, ownership (opaque handle created/destroyed by the caller,
 * deep copy) and error behaviour (int return codes, never throws; invalid arguments
 * abort, as GLPK does) follow GLPK's.  Enum VALUES are GLPK's public ones so that a
 * caller's GLP_* constants can be passed through unchanged.
 *
 * Plain C: pointers, ints and doubles only; no C++ or torch types cross this boundary.
 * The engine needs a gfx950 device: without one every entry point that touches the
 * engine (mvx_simplex and anything after it) fails loudly (message on stderr + abort).
 * There is no CPU fallback in this library.
 */
#ifndef MVX_H
#define MVX_H

#ifdef __cplusplus
extern "C" {
#endif

/* optimisation direction (glp_set_obj_dir / glp_get_obj_dir) */
#define MVX_MIN 1
#define MVX_MAX 2
/* column kind (glp_get_col_kind) */
#define MVX_CV 1
#define MVX_IV 2
#define MVX_BV 3
/* bound type (glp_set_row_bnds / glp_set_col_bnds) */
#define MVX_FR 1
#define MVX_LO 2
#define MVX_UP 3
#define MVX_DB 4
#define MVX_FX 5
/* basis status (glp_get_row_stat / glp_get_col_stat) */
#define MVX_BS 1
#define MVX_NL 2
#define MVX_NU 3
#define MVX_NF 4
#define MVX_NS 5
/* solution status (glp_get_status) */
#define MVX_UNDEF 1
#define MVX_FEAS 2
#define MVX_INFEAS 3
#define MVX_NOFEAS 4
#define MVX_OPT 5
#define MVX_UNBND 6
#define MVX_OFF 0
#define MVX_ON 1
/* mvx_simplex return codes (glp_simplex) */
#define MVX_EFAIL 5
#define MVX_EITLIM 8
/* mvx_last_error codes */
#define MVX_ENOMEM 0x101 /* the device ran out of memory for a tableau slab */

typedef struct mvx_prob mvx_prob; /* replaces glp_prob */

/* replaces glp_smcp (only the controls this engine honours) */
typedef struct {
  int msg_lev;
  int meth;       /* 1 = automatic (primal / dual / phase 1 from the basis at hand) */
  int it_lim;     /* pivot limit for this call, < 0 = none */
  double tol_bnd; /* primal feasibility tolerance, relative: tol * (1 + |bound|) */
  double tol_dj;  /* dual feasibility tolerance, absolute */
  double tol_piv; /* pivot magnitude tolerance, absolute */
} mvx_smcp;

/* ---- lifecycle ---------------------------------------------------------------- */
mvx_prob *mvx_create_prob(void);   /* glp_create_prob  bs.cpp:89,115; util.cpp:33,281 */
void mvx_erase_prob(mvx_prob *P);  /* glp_erase_prob   bs.cpp:114 */
void mvx_delete_prob(mvx_prob *P); /* glp_delete_prob  util.cpp:41 */
/* glp_copy_prob bs.cpp:116; util.cpp:34 -- deep copy incl. basis, tableau and solution;
   the device tableau is cloned device-to-device */
void mvx_copy_prob(mvx_prob *dst, const mvx_prob *src, int names);

/* ---- build / modify ----------------------------------------------------------- */
void mvx_set_obj_dir(mvx_prob *P, int dir);                                  /* util.cpp:58 */
int mvx_add_rows(mvx_prob *P, int nrs);                                      /* cut.cpp:23 */
/* glp_del_rows' shape: num[1..nrs] are distinct row numbers in 1..m (num[0] is not read).  The rows leave the model, the others
   keep their order and move up.  With a tableau on the device (DESIGN.md "Cut purging (cut_purge)"): when the auxiliary variable
   of every deleted row is basic, the tableau rows leave in place (k_delrows), every other entry keeps its bits, the variable
   numbers follow (an auxiliary k becomes k - #{deleted < k}, a structural one moves down by nrs), the basis stays, the status
   becomes MVX_UNDEF and the next solve takes no pivot; when one is non-basic the tableau is given up and the next solve starts
   from the slack basis.  Returns 0; -1 and nothing changed for a null, nrs < 1, a number out of range or a duplicate. */
int mvx_del_rows(mvx_prob *P, int nrs, const int *num);
/* mvx_del_rows on `count` distinct handles of one column count in one call (DESIGN.md "Cut purging in the tree (node_purge)"):
   handle t loses the model rows rows[off[t] .. off[t+1]-1] (1-based, distinct, any order; off[0] = 0, off ascending).  Every
   handle ends as mvx_del_rows(Ps[t], ...) leaves it, bit for bit -- model, tableau, basis arrays, mirrors, pending bound edits,
   status MVX_UNDEF -- and the device work of all of them is one upload and one k_delrows_many launch.  A handle with an empty
   list is not touched at all (its status stays); one without a tableau gets the model edit only; one in which a listed row's
   auxiliary variable is non-basic has its tableau given up, the others are unaffected.  Returns 0; -1 and no handle changed for
   a null, count < 1, a handle listed twice, differing column counts, a descending off, or a row number out of range or
   duplicated in any handle. */
int mvx_del_rows_many(mvx_prob *const *Ps, int count, const int *off, const int *rows);
int mvx_add_cols(mvx_prob *P, int ncs);                                      /* (readers) */
void mvx_set_row_bnds(mvx_prob *P, int i, int type, double lb, double ub);   /* cut.cpp:43 */
void mvx_set_col_bnds(mvx_prob *P, int j, int type, double lb, double ub);   /* bs.cpp:274,282 */
void mvx_set_obj_coef(mvx_prob *P, int j, double coef);                      /* util.cpp:55 */
void mvx_set_mat_row(mvx_prob *P, int i, int len, const int *ind, const double *val); /* cut.cpp:40 */
void mvx_set_col_kind(mvx_prob *P, int j, int kind);                         /* (readers) */
void mvx_set_col_name(mvx_prob *P, int j, const char *name);                 /* (readers) */
/* dense fast path: max c'x, Ax <= b, x >= 0; A row-major m x n */
int mvx_load_dense(mvx_prob *P, int m, int n, const double *A, const double *b, const double *c);

/* ---- solve -------------------------------------------------------------------- */
void mvx_init_smcp(mvx_smcp *parm);                /* glp_init_smcp */
/* Tolerances used when `parm` is NULL (every glp_simplex call of MVOLPS passes NULL: bs.cpp:117,279,287) and filled in
   by mvx_init_smcp.  Engine defaults: tol_bnd = tol_dj = tol_piv = 1e-9.  GLPK's defaults are tol_bnd = tol_dj = 1e-7,
   tol_piv = 1e-9 [GLPK-recalled]; they are tighter here so that objectives meet 1e-9 relative against independent
   solvers.  Where it matters to MVOLPS: util.cpp:443 tests integrality with no tolerance, so a primal value the
   tolerance lets stop short of its bound by 1e-8 reads as fractional -- the tighter value makes that rarer, not
   different in kind.  A caller that wants GLPK's numbers calls mvx_set_default_tolerances(1e-7, 1e-7, 1e-9) once. */
void mvx_set_default_tolerances(double tol_bnd, double tol_dj, double tol_piv);
int mvx_simplex(mvx_prob *P, const mvx_smcp *parm); /* glp_simplex bs.cpp:117,279,287;
                                                       BranchAndBound.cpp:52,134,141 */

/* batch entry (SURVEY.md section 8(b) "a batch entry for config 5"): `count` independent handles --
   e.g. the two children of a branch (bs.cpp:279,287) or a window of open nodes -- solved
   concurrently, one HIP stream each; results are identical to `count` calls of mvx_simplex.
   rcs[i] (nullable) receives each handle's return code */
int mvx_simplex_batch(mvx_prob **probs, int count, const mvx_smcp *parm, int *rcs);

/* ---- query -------------------------------------------------------------------- */
int mvx_get_obj_dir(const mvx_prob *P);               /* util.cpp:51 */
int mvx_get_num_rows(const mvx_prob *P);              /* gmi.cpp:15 */
int mvx_get_num_cols(const mvx_prob *P);              /* gmi.cpp:16; bs.cpp:181,250 */
int mvx_get_num_int(const mvx_prob *P);               /* util.cpp:299 */
int mvx_get_status(const mvx_prob *P);                /* util.cpp:423 */
double mvx_get_obj_val(const mvx_prob *P);            /* bs.cpp:125,156,190,210,280,288 */
double mvx_get_obj_coef(const mvx_prob *P, int j);    /* bs.cpp:182,190; util.cpp:437,455 */
double mvx_get_col_prim(const mvx_prob *P, int j);    /* bs.cpp:182,232,261; gmi.cpp:37 */
/* extension: glp_get_col_prim for every column in one call, x[1..n] (util.cpp:414-473 reads them all for every node) */
void mvx_get_col_prim_all(const mvx_prob *P, double *x);
double mvx_get_row_prim(const mvx_prob *P, int i);
double mvx_get_col_dual(const mvx_prob *P, int j);
double mvx_get_row_dual(const mvx_prob *P, int i);
int mvx_get_col_stat(const mvx_prob *P, int j);       /* gmi.cpp:23,50 */
int mvx_get_row_stat(const mvx_prob *P, int i);       /* gmi.cpp:45 */
int mvx_get_col_kind(const mvx_prob *P, int j);       /* gmi.cpp:18,51; util.cpp:444 */
int mvx_get_row_type(const mvx_prob *P, int i);       /* util.cpp:377 */
double mvx_get_row_lb(const mvx_prob *P, int i);      /* util.cpp:378 */
double mvx_get_row_ub(const mvx_prob *P, int i);      /* gmi.cpp:47 */
int mvx_get_col_type(const mvx_prob *P, int j);       /* util.cpp:319 */
double mvx_get_col_lb(const mvx_prob *P, int j);      /* util.cpp:320 */
double mvx_get_col_ub(const mvx_prob *P, int j);      /* gmi.cpp:52 */
const char *mvx_get_col_name(const mvx_prob *P, int j);
int mvx_get_mat_row(const mvx_prob *P, int i, int *ind, double *val);  /* gmi.cpp:84 */
int mvx_eval_tab_row(const mvx_prob *P, int k, int *ind, double *val); /* gmi.cpp:36 */
int mvx_get_it_cnt(const mvx_prob *P);
/* diagnostics of the anti-stalling rules.  After 64 + (m+n)/8 consecutive degenerate pivots, primal
   phase 2 first perturbs the bounds of the basic variables (once per solve; true bounds return when the
   phase ends); a second stall, the dual simplex and phase 1 fall back on Bland's smallest-subscript
   rule until a pivot moves again.  Counts: perturbations applied / pivots chosen by Bland's rule */
int mvx_get_pert_cnt(const mvx_prob *P);
/* > 0 overrides the number of consecutive degenerate pivots that arms the rules; 0 = default */
void mvx_set_stall_limit(int limit);
/* diagnostic (MVX_FCS_DBG=1): phase stamps of the lead workgroup of k_pc / k_pr / k_chain, 16 per chain position; returns rows */
int mvx_fcs_debug_stamps(unsigned long long *out);
int mvx_get_bland_cnt(const mvx_prob *P);
int mvx_term_out(int flag);      /* glp_term_out 2test.cpp:45,53,62 */
const char *mvx_version(void);   /* glp_version  util.cpp:278 */

/* generateCut3 (gmi.cpp:11-117) for `count` basic integer columns cols[0..count-1] (1-based) of a solved node in one
   device pass: tableau rows, the coefficient formula and the back-substitution over the model rows run on the GPU.
   vals is count x (n+1), row-major: vals[t][1..n] the cut coefficients, vals[t][0] = rhs[t] = its lower bound
   (the CutContainer of gmi.cpp:91-109); ok[t] = 0 where no cut exists.  repaired = 0: the formula as written, running
   right-hand side and positional back-substitution included; 1: mvx_generateCutGMI's.  Bit-identical to the
   one-column host functions of mvx_bnb.h.  Returns 0, -1 on bad arguments, -2 when the device is out of memory */
int mvx_gmi_cuts(const mvx_prob *P, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok);
/* The same for cuts taken from DIFFERENT solved handles in one call: cut t comes from Ps[t], column cols[t].  The handles
   must share their columns and their first model rows (clones of one root, each with its own bounds, basis and appended
   cut rows): a round of a B&B window takes one cut from each of its branching nodes (bs.cpp:249-258 run for 64 nodes at
   once).  vals is count x (n+1).  Returns -3 when the handles do not share a root (call mvx_gmi_cuts per handle then). */
int mvx_gmi_cuts_many(const mvx_prob *const *Ps, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok);
/* printInfo (util.cpp:414-473) of `count` solved handles with the same columns, one device launch for all of them.  Per
   handle t: status[t] = -1 (NOFEAS / INFEAS / UNBND), 0 (some integer column fractional) or 1; nviol[t] violated columns,
   ascending, in viol[t*cap .. t*cap + nviol[t] - 1] and their primal values (the bits get_col_prim returns) in xviol[same].
   quirks = 1: bug-compatible test (x != 0, objective coefficient != 0, trunc(x) != x); 0: 1e-9 tolerance.
   Returns 0; -1 bad arguments (a handle without a solved tableau, different columns or objective); -2 device out of
   memory; -3 some handle has more than `cap` violated columns. */
int mvx_classify_many(const mvx_prob *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol, int cap);
/* One-step dual penalties (DESIGN.md "Branching on the node LP") of candidate columns of `count` solved handles, one device
   launch for all of them.  The candidates of handle t are cols[col_off[t] .. col_off[t+1]-1] (1-based columns, each one
   basic); the results go to the same indices of pen_down / pen_up (+inf: that child is infeasible) and arg_down / arg_up
   (the non-basic position that attains each side's minimum, the lowest one on ties; 0 when the side is +inf).  A position
   q counts only where |T[i][q]| > tol; the B&B driver passes the pivot tolerance.  Bit-identical to mvx_bnb_penalties
   (mvx_bnb.h).  Returns 0; -1 bad arguments or a column outside 1..n; -2 device out of memory; -3 a handle whose status
   is not MVX_OPT; -4 a column that is not basic. */
int mvx_branch_penalties_many(const mvx_prob *const *Ps, int count, const int *cols, const int *col_off, double tol, double *pen_down,
                              double *pen_up, int *arg_down, int *arg_up);
/* Sensitivity ranges (DESIGN.md "Sensitivity ranges (ranges)") of one solved handle: how far every variable k = 1..m+n
   (auxiliaries first, then the structurals) may move before the basis stops being optimal.  val is (m+n+1) x 6 doubles,
   columns ACT_DN, ACT_UP, OBJ_DN, OBJ_UP, COST_DN, COST_UP; var is (m+n+1) x 4 ints, columns LIM_DN, LIM_UP, ENT_DN, ENT_UP;
   row 0 of both is zero.  A non-basic variable gets its activity range (ratio test down its tableau column: the step in each
   direction, the basic variable that limits it, the size of the objective change there) and the allowable change of its cost
   from its reduced cost; a basic variable gets the allowable change of its cost (ratio test along its tableau row) and the
   non-basic variable that would enter.  An entry counts where it exceeds the default pivot tolerance (mvx_init_smcp); +inf
   means no limit.  Pure: the handle is only read.  Bit-identical to mvx_bnb_ranges (mvx_bnb.h).  Returns 0; -1 a null
   argument; -2 device out of memory (nothing written); -3 the handle's status is not MVX_OPT or it has no tableau. */
int mvx_ranges(const mvx_prob *P, double *val, int *var);
/* the tableau rows one workgroup of the column-wise ratio test (k_rangecols) walks: up to this many rows are one chunk */
int mvx_ranges_chunk(void);
/* KKT check (DESIGN.md "KKT check (kkt)") of `count` solved handles against their own models, in one device call: does what
   the getters publish -- get_col_prim, get_row_prim, get_row_dual, get_col_dual, the statuses and the bounds, read where they
   lie in each handle's tableau slab -- still satisfy xR - A xS = 0 (PE), the variables' bounds (PB), c - A'lambda - d = 0 (DE)
   and the signs of the duals (DB)?  val[8 t ..] holds ae_max, re_max of PE, PB, DE, DB in that order for handle t, ind[8 t ..]
   the row (PE), column (DE) or variable k = 1..m+n, auxiliaries first (PB, DB) where each maximum occurs: the lowest among
   equals, 0 when the maximum is 0.  Every handle has root's n columns and root's m0 rows as its first rows, the same objects
   (clones of root, as for mvx_gmi_cuts_many); rows behind them are cut rows.  Pure: no handle is changed.  Bit-identical to
   mvx_bnb_kkt (mvx_bnb.h).  Returns 0 (count == 0 does nothing); -1 bad arguments (a null, count < 0, differing column
   counts); -2 device out of memory, nothing written; -3 a handle that is MVX_UNDEF or has no tableau (or that
   carries bound edits no solve has taken up yet: such a handle is MVX_UNDEF in any case), or one that does not share root's
   rows. */
int mvx_kkt_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind);
/* The same for one handle against itself; r_pe[0..m] and r_de[0..n] (either may be NULL) receive the residuals
   r_i = xR_i - sum_j a_ij xS_j and r_j = (c_j - sum_i a_ij lambda_i) - d_j, entry 0 of each 0. */
int mvx_kkt(const mvx_prob *P, double *val, int *ind, double *r_pe, double *r_de);
/* glp_check_kkt's shape [GLPK-recalled]: sol must be 1 (the basic solution), cond 1 PE, 2 PB, 3 DE, 4 DB; -1 otherwise. */
#define MVX_KKT_PE 1
#define MVX_KKT_PB 2
#define MVX_KKT_DE 3
#define MVX_KKT_DB 4
int mvx_check_kkt(const mvx_prob *P, int sol, int cond, double *ae_max, int *ae_ind, double *re_max, int *re_ind);
/* Farkas proof (DESIGN.md "Infeasibility and unboundedness proofs (farkas)") of `count` handles against their own models, in one
   device call: is there a weight vector y over the rows for which sum_r y_r (xR_r - a_r xS) -- zero at every feasible point --
   cannot reach zero inside the bounds?  Every tableau row of a handle is tried as a suggestion (one pass over the slab), the best
   one is evaluated on the model (rows 1..m0 from root's device copy, cut rows from the call's upload).  val[4 t ..] holds rel of
   the tableau side, rel of the model side, the model side's Lo or -Hi, and de, the largest relative distance between the
   tableau's and the model's structural coefficients; ind[4 t ..] holds found (0 none, 1 the tableau row only, 2 proved on the
   model), the tableau row, the side (1 lower, 2 upper) and the coefficients the model side dropped under the zero rule; all zero
   when found = 0, as for every MVX_OPT or MVX_FEAS handle.  Handles are related to root as in mvx_kkt_many.  Pure: no handle is
   changed.  Bit-identical to mvx_bnb_farkas (mvx_bnb.h).  Returns 0 (count == 0 does nothing); -1 bad arguments (a null,
   count < 0, differing column counts); -2 device out of memory, nothing written; -3 a handle that is MVX_UNDEF or has no
   tableau, or one that does not share root's rows. */
int mvx_farkas_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind);
/* The same for one handle against itself; y[0..m] (may be NULL) receives the row weights, entry 0 zero. */
int mvx_farkas(const mvx_prob *P, double *val, int *ind, double *y);
/* The ray that proves a handle unbounded (same section of DESIGN.md), a pure function of the end state: the lowest non-basic
   position q whose status allows a direction sigma (+1 up, -1 down) in which the published dual of N(q) improves the objective by
   more than 1e-9 in the LP's own sense, whose own bound on that side is infinite and for which every basic variable, moving by
   sigma alpha_iq, has that side infinite or |alpha_iq| <= 1e-9.  The ray is d_N(q) = sigma, d_B(i) = sigma alpha_iq, 0 elsewhere.
   It is checked on the model: rho_r = dR_r - sum_j a_rj dS_j (ae = |rho_r|, re = ae / (1 + |dR_r|), as PE of mvx_kkt_many), the
   slope sum_j c_j dS_j, and the variables with |d_k| > 1e-9 whose bound on the side d_k points to is finite.  val[4] = the dual,
   ae_max, re_max, the slope; ind[6] = found, the variable N(q) (k = 1..m+n, auxiliaries first), sigma, the blocking variables,
   the rows of ae_max and re_max (the lowest among equals, 0 for a zero maximum); found = 2 when the slope improves the objective,
   re_max <= 1e-9 and nothing blocks, 1 when only the tableau side holds, 0 (everything zero) when there is no such position.
   d[0..m+n] (may be NULL) receives the ray, entry 0 zero.  Pure: the handle is not changed.  Bit-identical to mvx_bnb_ray
   (mvx_bnb.h).  Returns 0; -1 a null argument; -2 device out of memory, nothing written; -3 a handle that is MVX_UNDEF or has no
   tableau. */
int mvx_ray(const mvx_prob *P, double *val, int *ind, double *d);
/* glp_get_unbnd_ray's shape [GLPK-recalled]: the variable k = 1..m+n whose move mvx_ray finds (found >= 1) when the handle's
   status is MVX_UNBND; 0 for any other status, or when none is found. */
int mvx_get_unbnd_ray(const mvx_prob *P);
/* Primal rounding heuristic (DESIGN.md "Primal rounding heuristic") on `count` solved handles, one device launch: each
   handle's column values rounded (mode 1) and filled greedily (mode 2), checked against the model of `root` -- its rows
   1..m0 (m0 = root's row count; rows a handle has beyond them, cut rows, are ignored), row bounds, column bounds and
   objective.  The handles are B&B nodes of root's tree: their own column bounds are tightened, so the root names the
   model.  The model is uploaded once and kept with `root` while root's rows, bounds, objective and kinds stay as they
   are.  obj[t], found[t] (1: feasible) and the candidate x[t*(n+1) + 1 .. t*(n+1) + n] per handle.  Bit-identical to
   mvx_bnb_round (mvx_bnb.h).  Returns 0; -1 bad arguments (mode outside 1..2, a handle with another column count); -2
   device out of memory; -3 a handle whose status is not MVX_OPT; -5 n > 4096 (the kernel keeps a handle's values and
   its sort in LDS). */
int mvx_round_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int mode, double *obj, int *found, double *x);
/* Reduced-cost bound tightening (DESIGN.md "Reduced-cost tightening") of `count` solved handles against cutoff[t] (the
   incumbent's objective), one device launch (k_rcfix) over row 0 of every tableau: a non-basic integer column at an
   integral bound with |d_q| > tol may move at most t = ceil(gap2 / |d_q|) - 1 units off it, gap2 = sg*z - sg*cutoff plus a
   slack of 1e-9 * max(1, |cutoff|).  Handle t's changed columns, ascending, in cols[t*n .. t*n + cnt[t] - 1] with their new
   bounds in lb / ub[same].  Pure: no handle changes.  Bit-identical to mvx_bnb_rc_tighten (mvx_bnb.h).  Returns 0; -1 bad
   arguments (different column counts or kinds); -2 device out of memory; -3 a handle whose status is not MVX_OPT. */
int mvx_rc_tighten_many(const mvx_prob *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb,
                        double *ub);
/* Bound lists of many handles applied with one device launch (k_setbnds): handle t takes the entries off[t] .. off[t+1]-1
   (columns strictly ascending within a handle, finite bounds, lb <= ub).  Afterwards each handle is in the state
   mvx_set_col_bnds(P, col, lb == ub ? MVX_FX : MVX_DB, lb, ub) per entry would leave.  Only for edits that leave a non-basic
   column's resting value where it is: returns -4, nothing changed, when a listed column is basic in its handle or the edit
   would move its value; -1 bad arguments; -2 device out of memory. */
int mvx_tighten_cols_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);
/* Node bound propagation (DESIGN.md "Node bound propagation") of `count` handles, one device launch (k_prop) for all handles and
   all rounds: up to max_rounds Jacobi rounds of activity-based tightening of the integer columns' bounds from rows 1..m0 of
   `root` (m0 = root's row count; cut rows are ignored) and each handle's own column bounds as its host model has them (a
   pending branching edit counts).  The model is uploaded once and kept with `root`, as for mvx_round_many.  infeasible[t],
   rounds[t], and handle t's changed columns, ascending, in cols[t*n .. t*n + cnt[t] - 1] with their bounds in lb / ub[same]
   (+-inf for an absent bound; none for an infeasible handle).  Pure: no handle changes, none need be solved.  Bit-identical to
   mvx_bnb_propagate (mvx_bnb.h).  Returns 0; -1 bad arguments (max_rounds < 1, a handle with another column count); -2 device
   out of memory; -5 n > 4096 (the kernel keeps a handle's bounds in LDS). */
int mvx_propagate_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_rounds, int *infeasible, int *rounds, int *cnt,
                       int *cols, double *lb, double *ub);
/* General bound lists of many handles applied with one device launch (k_setbnds): handle t takes the entries off[t] .. off[t+1]-1
   (columns strictly ascending within a handle, lb <= ub, +-inf for an absent bound; every handle listed once).  The bound type
   follows from which bounds are finite (FX where they are equal, DB, LO, UP, FR), and each handle is left in the state
   mvx_set_col_bnds per entry, in list order, leaves it in: bounds of basic columns wait for the next solve (merged with a
   pending edit of the same row), non-basic positions take their bounds and status, and where a resting value moves column 0 of
   every tableau row follows.  Clones recorded and not yet launched are flushed first.  Returns 0; -1 bad arguments or a bad list
   (nothing is changed); -2 device out of memory. */
int mvx_set_col_bnds_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);
/* LP diving heuristic (DESIGN.md "LP diving heuristic"): the branching pick of `count` (solved handle, rule) pairs, one device
   launch (k_divepick), rules[t] one of 1 fractional, 2 locks, 4 vector length.  The values are each handle's own, the locks,
   column lengths and objective those of rows 1..m0 of `root` (m0 = root's row count; cut rows are ignored); the model is
   uploaded once and kept with `root`, as for mvx_round_many.  nfrac[t] the fractional integer columns of handle t, col[t] the
   one rule rules[t] branches on (0 when there is none), dir[t] 0 down / 1 up, val[t] its value.  Pure: no handle changes.
   Bit-identical to mvx_bnb_dive_pick (mvx_bnb.h).  Returns 0; -1 bad arguments (a rule outside {1, 2, 4}, a handle with
   another column count); -2 device out of memory; -3 a handle whose status is not MVX_OPT; -5 n > 4096, as for
   mvx_round_many, whose model it shares. */
int mvx_dive_pick_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir,
                       double *val);
/* The whole objective of `count` handles replaced, one device launch (k_objrow) for all their cost rows: handle t takes
   c[t*(n+1) + 0 .. n], entry 0 the constant.  The handles have the same n; their row counts may differ (cut rows).  Each is
   left, bit for bit, as mvx_set_obj_coef(P, j, c[j]) for j = 0..n leaves it: the objective replaced, the status MVX_UNDEF, and
   where it has a valid tableau row 0 rebuilt (the basis stays, so a solved handle restarts primal feasible); a handle without
   a tableau only takes its objective.  Pending bound edits stay pending.  Returns 0; -1 bad arguments (a null, count < 0,
   differing column counts, a handle listed twice); -2 device out of memory, nothing changed. */
int mvx_set_obj_many(mvx_prob *const *Ps, int count, const double *c);
/* Feasibility pump (DESIGN.md "Feasibility pump"): the rounding and the distance objective of `count` solved handles, one
   device launch (k_pumpobj).  Values and bounds are each handle's own, the integer flags and the objective c0 those of `root`
   (model kept with it, as for mvx_round_many).  xt[t][1..n] the rounding of the integer columns (nearest integer, clamped to
   the column's integral bounds; 0 for continuous columns); when has_prev[t] is set and it equals xprev[t] on every integer
   column, the up to 10 movable columns farthest from their LP value are moved one unit towards it.  c[t][0..n] the new
   objective in the handle's own direction, c_j = a * (-sg * d_j) + (q * sqrt(nnz(d))) * c0_j with (a, q) = ab[2t], ab[2t+1] and
   d the distance slopes; c[t][0] = 0.  info[4t..] = fractional integer columns, columns moved, stalled (a repeated rounding
   with nothing to move), nnz(d).  xprev may be NULL when no has_prev is set.  Pure: no handle changes.  Bit-identical to
   mvx_bnb_pump_obj (mvx_bnb.h).  Returns 0; -1 bad arguments; -2 device out of memory; -3 a handle whose status is not
   MVX_OPT; -5 n > 4096, as for mvx_round_many, whose model it shares. */
int mvx_pump_obj_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const double *xprev, const int *has_prev,
                      const double *ab, int *info, double *xt, double *c);
/* Root cut rounds (DESIGN.md "Root cut rounds"): the scores of `k` candidate cut rows against a solved handle, one device
   launch (k_cutgram).  vals is k x (n+1) in the layout of mvx_gmi_cuts (entry 0 of a row is not read).  dot[t] = sum_j v_tj x_j
   with x the handle's column values (the bits mvx_get_col_prim returns), gram[t*k + s] = sum_j v_tj v_sj; every sum runs over
   ascending j from +0.0, product and sum rounded separately.  gram is exactly symmetric.  Pure: the handle does not change.
   Bit-identical to mvx_bnb_cut_scores (mvx_bnb.h).  Returns 0; -1 bad arguments or a handle that is not MVX_OPT; -2 device
   out of memory. */
int mvx_cut_scores(const mvx_prob *P, int k, const double *vals, double *dot, double *gram);
/* `k` dense MVX_LO rows appended in one device pass (k_cutrows): row t has the coefficients vals[t*(n+1) + 1 .. n] and the
   lower bound rhs[t].  The handle is left, bit for bit, as k times (mvx_add_rows(P, 1), mvx_set_mat_row with all n indices,
   mvx_set_row_bnds(MVX_LO)) in list order leave it: model, tableau, basis, bounds, status MVX_UNDEF, and a dual warm start
   for the next solve.  Returns 0; -1 bad arguments, nothing changed (k < 1, a null, a NaN, a handle without a valid tableau);
   -2 device out of memory: the model has the rows, the tableau is given up as mvx_add_rows gives it up. */
int mvx_add_cut_rows(mvx_prob *P, int k, const double *vals, const double *rhs);
/* mvx_add_cut_rows on `count` distinct handles of one column count in one call (DESIGN.md "Row append across handles
   (add_cut_rows_many)"): handle t takes rows off[t] .. off[t+1]-1 of vals / rhs (off[0] = 0, off ascending; vals is
   off[count] x (n+1) row-major in the layout of mvx_gmi_cuts, rhs[r] the lower bound of row r).  The handles' row counts may
   differ.  Every handle that is given rows ends as mvx_add_cut_rows(Ps[t], k_t, vals + off[t]*(n+1), rhs + off[t]) leaves it, bit
   for bit -- model, tableau, basis arrays, mirrors, pending bound edits, status MVX_UNDEF, a dual warm start -- and the device
   work of all of them is the recorded clones flushed once, one upload and one k_cutrows_many launch.  A handle that is given no
   rows is not touched at all (its status stays).  Returns 0; -1 and no handle changed for a null, count < 1, a handle listed
   twice, differing column counts, a descending off, a NaN in an entry that is read, or a handle without a valid tableau that is
   given rows (everything is checked before the first handle is edited); -2 device out of memory: the handles that could not
   get their memory have the rows in the model and their tableau given up, as mvx_add_cut_rows leaves them, the others are
   complete, and mvx_last_error reads MVX_ENOMEM. */
int mvx_add_cut_rows_many(mvx_prob *const *Ps, int count, const int *off, const double *vals, const double *rhs);
/* Column append (DESIGN.md "Column append (add_cols)"): `k` dense structural columns join the model as columns n+1..n+k and,
   where the handle has a valid tableau, the tableau and the basis in one device pass (k_addcols): the new columns are
   non-basic at their resting bound, the basis and every other body entry keep their bits.  cols is k x (m+1) row-major:
   cols[t*(m+1) + i] the coefficient of new column t in model row i = 1..m (entry 0 is not read); obj[t] its objective
   coefficient; type[t] in MVX_FR..MVX_FX with lb[t] / ub[t] read as mvx_set_col_bnds reads them; kind[t] MVX_CV or MVX_IV
   (kind == NULL: all MVX_CV).  The model ends as mvx_add_cols(k), mvx_set_mat_col, mvx_set_col_bnds, mvx_set_obj_coef and
   mvx_set_col_kind leave it.  On a handle without a valid tableau only the model is edited (no device is needed).  Returns 0;
   -1 bad arguments, nothing changed (a null, k < 1, a NaN, a type outside FR..FX, lb > ub on a DB column, a kind outside
   CV / IV); -2 device out of memory: the model has the columns and the tableau is given up, as mvx_add_cut_rows gives it up. */
int mvx_add_dense_cols(mvx_prob *P, int k, const double *cols, const double *obj, const int *type, const double *lb, const double *ub,
                       const int *kind);
/* The images mvx_add_dense_cols would write, without appending: dj[t] the reduced cost (row 0 of the image) of candidate column
   t, img (nullable) k x (m+1) the whole images by tableau row 0..m.  With img == NULL only row 0 of the tableau is read.  Pure:
   the handle is only read.  Bit-identical to mvx_bnb_price_cols (mvx_bnb.h).  Returns 0; -1 bad arguments; -2 device out of
   memory, nothing written; -3 the handle has no valid tableau. */
int mvx_price_cols(const mvx_prob *P, int k, const double *cols, const double *obj, double *dj, double *img);
int mvx_price_cols_tile(void); /* candidate columns one k_addcols workgroup carries per pass over its rows */
/* glp_set_mat_col / glp_get_mat_col (model layer, 1-based, element 0 ignored).  mvx_set_mat_col on a handle with a tableau gives
   the tableau up, as mvx_add_cols does; mvx_get_mat_col returns the non-zeros in ascending row order. */
void mvx_set_mat_col(mvx_prob *P, int j, int len, const int *ind, const double *val);
int mvx_get_mat_col(const mvx_prob *P, int j, int *ind, double *val);
/* Column deletion (DESIGN.md "Column deletion (del_cols)"), the shape of glp_del_cols: the distinct columns num[1..ncs] (1-based,
   num[0] is not read) leave the model, the others keep their order.  Where the handle has a valid tableau and every deleted
   column is non-basic, the columns leave the tableau in one device pass (k_delcols): column 0 is shifted for the resting values
   of the deleted columns (a deleted variable counts as 0 from now on), the kept positions close up in their order bit for bit,
   the basis stays and the next solve is warm; the row stride follows the new column count.  Where a deleted column is basic the
   tableau is given up and the next solve starts from the slack basis.  On a handle without a valid tableau only the model is
   edited (no device is needed).  Returns 0; -1 bad arguments, nothing changed (a null, ncs < 1, a number outside 1..n, a
   duplicate, or ncs == n: the engine has no LP without columns, so the last column cannot leave); -2 device out of memory:
   the model has lost the columns and the tableau is given up, as mvx_add_cut_rows gives it up. */
int mvx_del_cols(mvx_prob *P, int ncs, const int *num);
int mvx_del_cols_span(void); /* destination positions a wave of k_delcols moves per batch */
/* Sifting (DESIGN.md "Sifting (sift)"): an LP far wider than the tableau one wants to stream is solved over a narrow working LP and
   a pool of the other columns that lives on the device.
   The pool holds dense columns over m rows, numbered 1..N in the order given.  mvx_pool_add_cols takes exactly the arguments of
   mvx_add_dense_cols (cols is k x (m+1) row-major, entry 0 of a column is not read) and refuses what that call refuses.  It also
   refuses a column that cannot rest at zero: after the bounds are read as mvx_set_col_bnds reads them, the value the column would
   rest at as a new non-basic column must be 0 -- MVX_LO / MVX_DB with lb = 0, MVX_UP with ub = 0, MVX_FR, MVX_FX at 0.  A pool
   column that is absent from the working LP therefore means "at 0", and sifting is sound without shifting right-hand sides.  A
   refused call returns -1 and changes nothing.  The pool keeps a host copy and a device copy; the device copy is made by the
   first call that needs the device (mvx_pool_price, mvx_pool_append on a handle with a tableau, mvx_sift) and extended after
   later mvx_pool_add_cols calls, so create / add / num / get / delete and every refusal run without a device.
   mvx_pool_get_col: column j as it was given (any output may be NULL; col has m+1 entries, col[0] = 0); -1 for j outside 1..N. */
typedef struct mvx_colpool mvx_colpool;
mvx_colpool *mvx_pool_create(int m);
int mvx_pool_add_cols(mvx_colpool *S, int k, const double *cols, const double *obj, const int *type, const double *lb, const double *ub,
                      const int *kind);
int mvx_pool_num_cols(const mvx_colpool *S);
int mvx_pool_num_rows(const mvx_colpool *S);
int mvx_pool_get_col(const mvx_colpool *S, int j, double *col, double *obj, int *type, double *lb, double *ub, int *kind);
void mvx_pool_delete(mvx_colpool *S);
/* The reduced cost of every pool column against the handle's duals, and the K most attractive columns, in one stream over the
   device pool (k_poolprice) and a selection on the device (k_poolsel_*).  y_i, i = 1..m, is the row-0 tableau entry at the
   non-basic position of the auxiliary variable of row i, +0.0 when it is basic (the numbers mvx_price_cols weights by), and
   d_j = obj_j + S_j, S_j = sum_i (-a_ij) y_i in 64 chains: chain l takes i = l+1, l+65, ... ascending with fma(-a_ij, y_i, acc)
   from +0.0, rows with y_i == 0 skipped; the chains are combined by s[l] += s[l+h], h = 32 .. 1; obj_j is added last.
   dj (nullable) [N+1] receives d_j, dj[0] = 0.  Column j is attractive by the engine's primal pricing rule on the status it would
   enter with, sgn = +1 under MVX_MAX and -1 under MVX_MIN: MVX_LO / MVX_DB sgn d_j > tol_dj, MVX_UP sgn d_j < -tol_dj, MVX_FR
   |d_j| > tol_dj, MVX_FX never; tol_dj is mvx_init_smcp's.  A column with skip[j] != 0 is never picked (skip nullable, [N+1],
   skip[0] not read); its d_j is written all the same.  pick[0 .. *npick-1] are the min(K, #attractive) attractive columns of
   largest |d_j| in descending order of |d_j|, ties to the lower j; K >= 0, K = 0 prices only (pick may then be NULL).  Pure: the
   handle is only read.  Bit-identical to mvx_bnb_pool_price_values + mvx_bnb_pool_select (mvx_bnb.h).  Returns 0; -1 a null, K < 0
   or a pool of another row count than the handle; -2 device out of memory, nothing written; -3 the handle has no valid tableau or
   its status is MVX_UNDEF. */
int mvx_pool_price(const mvx_prob *P, const mvx_colpool *S, const unsigned char *skip, int K, double *dj, int *pick, int *npick);
/* The distinct pool columns idx[0..k-1] join the handle exactly as mvx_add_dense_cols(P, k, ...) with those columns' data in that
   order: model, tableau, basis arrays, mirrors and status end with the same bits, and the return codes are the same.  With a
   valid tableau the coefficients do not travel from the host: k_poolgather lays them out from the device pool for k_addcols.
   Without one the call is the model edit only.  -1 also for an index outside 1..N, a duplicate, or another row count. */
int mvx_pool_append(mvx_prob *P, const mvx_colpool *S, int k, const int *idx);
/* The sifting loop.  where[1..N] is in / out: 0, or the column of P that already is pool column j (a first call passes zeros, a
   later call -- after a bound edit, say -- what the last one returned).  Columns of P that no entry names are the caller's own and
   never leave.  A round: mvx_simplex(P, parm) (parm->it_lim limits each solve); unless the status is MVX_OPT the loop ends with
   that status; otherwise mvx_pool_price over the absent columns with K; when nothing is attractive the loop ends, and P is optimal
   for the full LP with every absent column at 0; otherwise the picks are appended (mvx_pool_append) and, with purge = A > 0,
   every pool column of P that the last A solves in a row left non-basic at 0 -- where an absent column rests; a non-basic column at
   a non-zero upper bound is in use and stays -- leaves through one mvx_del_cols call (a column appended in this round stays),
   `where` following the renumbering.
   info->end tells what ended the loop: MVX_OPT -- optimal for the FULL LP; MVX_UNBND -- the working LP is unbounded, and so is the
   full LP; MVX_NOFEAS / MVX_INFEAS / MVX_UNDEF / MVX_FEAS -- the status of the WORKING LP only: it says NOTHING about the full LP
   (an infeasible working LP may become feasible with absent columns; pricing them by a Farkas proof is not built); 0 -- the round
   limit.  Returns 0; -1 a null, another row count, K < 1, max_rounds < 1, purge outside 0..64, or a `where` entry that is out of
   range, names a column twice or names a column of P whose coefficients or objective coefficient differ from the pool's (bounds
   are P's own to edit), nothing changed; -2 device out of memory, the handle as the failing call left it; -4 max_rounds rounds
   ran and attractive columns are still on offer: P is a valid, solved working LP.  sp == NULL: the defaults; info nullable.
   mvx_init_sift_parm fills the defaults for a pool over m rows: K = max(m, 64), max_rounds = 200, purge = 0. */
typedef struct {
  int K;          /* columns appended per round at most */
  int max_rounds; /* rounds (solves) at most */
  int purge;      /* 0: off; A: a pool column non-basic at 0 after A consecutive solves leaves */
} mvx_sift_parm;
typedef struct {
  int rounds, lps;
  long long priced, appended, purged, pivots;
  int n_final; /* P's columns at the end */
  int end;
} mvx_sift_info;
void mvx_init_sift_parm(mvx_sift_parm *sp, int m);
int mvx_sift(mvx_prob *P, const mvx_colpool *S, const mvx_smcp *parm, const mvx_sift_parm *sp, int *where, mvx_sift_info *info);
/* Clique cuts (DESIGN.md "Clique cuts (cut_families)"): the conflict graph of the binary columns of `model` (integer, bounds 0
   and 1 exactly), two device launches (k_conflict_rows, k_conflict).  Columns j < k are adjacent when one of rows 1..m (m the
   handle's row count) forbids x_j = x_k = 1 with every other term at its least: (Lmin_i + a_ij) + a_ik > rub_i + tol(rub_i) on
   the upper side, the mirror on the lower side, the activities those of mvx_propagate_many at the handle's own bounds.  adj
   holds (n+1) rows of W = ceil((n+1)/64) 64-bit words, bit k of row j being bit (k mod 64) of word k/64; row 0 and bit 0 are
   zero, the relation is symmetric.  *edges the number of pairs j < k.  Pure: the handle need not be solved and does not change.
   Bit-identical to mvx_bnb_conflict_graph (mvx_bnb.h).  Returns 0; -1 bad arguments; -2 device out of memory; -5 is kept for a
   kernel with a size limit (the driver then runs the twin): k_conflict has none and never returns it. */
int mvx_conflict_graph(const mvx_prob *model, unsigned long long *adj, long long *edges);
/* Clique cuts in the tree (DESIGN.md "Clique cuts in the tree (node_cliques)"): the separation of mvx_bnb_clique_cuts (mvx_bnb.h)
   for `count` solved handles in one launch (k_cliquesep), against the conflict graph of `root` -- exactly mvx_conflict_graph(root),
   computed on the device on the first call and kept with `root` beside the model of mvx_round_many, checked on every call by the
   same rule -- and each handle's own column values, the bits mvx_get_col_prim returns.  cnt[t] the cliques kept for handle t, in
   the order of the twin; q[(t*max_cuts + c)*W + w] the member set of clique c in the word layout of adj (W = ceil((n+1)/64),
   bit 0 zero); sum[t*max_cuts + c] its s, summed over ascending columns from +0.0.  Slots from cnt[t] on are zero.  Pure: no
   handle changes; the handles may have other row counts than `root` (cut rows).  Bit-identical to mvx_bnb_clique_masks.  Returns
   0 (count == 0 does nothing); -1 bad arguments (a null, count < 0, max_cuts outside 1..64, a handle with another column
   count); -2 device out of memory, nothing written; -3 a handle whose status is not MVX_OPT; -5 more than 4096 columns (the
   driver then runs the twin). */
int mvx_clique_cuts_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q,
                         double *sum);
/* Incumbent polishing (DESIGN.md "Incumbent polishing (polish)"): a best-improvement search over one- and two-column unit moves
   from each of `count` points, against the model of `root` (rows 1..m0, row and column bounds, kinds, objective and sense; kept
   with `root` and checked on every call, as for mvx_round_many, the by-row copy of mvx_propagate_many included).  x is count x
   (n+1) in the layout of mvx_round_many and is edited in place (entry 0 of a point is not read or written).  A point whose
   integer columns are not within 1e-9 of an integer, or that fails the rounding heuristic's check, is refused: ok[t] = 0, its x
   untouched, obj[t] = 0 and moves[t] = 0.  Otherwise ok[t] = 1, x the polished point (integer columns rounded at entry), obj[t]
   its objective and moves[t] the moves taken, at most max_moves (1..100000).  Per iteration two launches (k_lsmove, k_lsapply),
   enqueued eight iterations at a time.  Pure: no handle changes, none need be solved.  Bit-identical to mvx_bnb_polish
   (mvx_bnb.h).  Returns 0; -1 bad arguments (a null, count < 0, max_moves outside 1..100000); -2 device out of memory, nothing
   written; -5 is kept for a kernel with a size limit (the driver then runs the twin): these kernels have none and never
   return it. */
int mvx_polish_many(const mvx_prob *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok);

/* ---- engine-state access (parity tests, visualisers) --------------------------- */
int mvx_get_tableau_ld(const mvx_prob *P);
int mvx_get_tableau(const mvx_prob *P, double *out); /* (m+1) x (n+1), packed row-major */
int mvx_get_basis(const mvx_prob *P, int *head, int *nb, int *flag);

/* ---- device / measurement ------------------------------------------------------ */
/* number of visible HIP devices (0 when none); never aborts */
int mvx_device_count(void);
/* bind this process to device `dev` (one process per GPU); 0 on success */
int mvx_set_device(int dev);
/* HIP-event timing on the engine's own stream: accumulated milliseconds and launch count
   of the rank-1 update kernel since the last reset (only collected while enabled) */
void mvx_profile_enable(int on);
void mvx_profile_reset(void);
double mvx_profile_update_ms(void);
long long mvx_profile_update_launches(void);
/* wall time (ms, HIP events on the engine stream) of the last mvx_simplex call's device work */
double mvx_last_solve_ms(const mvx_prob *P);
/* node migration between ranks: image of bounds + basis + tableau in DEVICE
   memory of this process's GPU, ready for an RCCL send; the receiver rebuilds the handle on top of
   its own copy `base` of the root model.  The `_from` forms also carry the model rows appended since
   `base` (rows base.m+1 .. m: GMI cut rows, cut.cpp:23-43), so that a node with cuts can migrate; the plain
   forms carry none and need a receiver `base` with the same number of rows.  The image also carries the
   tolerances of the solve that produced the status, so a migrated optimal node is not solved again.
   Refusals, all -1: the `_from` forms for a `base` with more rows than P or another number of columns (a
   handle whose columns were edited travels as its own base, mvx_pack); mvx_unpack for dst == base, a buffer
   that holds no image, and an image of another base.m or n than `base` has -- dst is then a model-only copy
   of `base`. */
long long mvx_pack_size(const mvx_prob *P);
int mvx_pack(const mvx_prob *P, void *dev_buf);
long long mvx_pack_size_from(const mvx_prob *P, const mvx_prob *base);
int mvx_pack_from(const mvx_prob *P, const mvx_prob *base, void *dev_buf);
int mvx_unpack(mvx_prob *dst, const mvx_prob *base, const void *dev_buf);
/* streamed-update tuning (row-block depth 8/16/32, batched-load hot loop, non-temporal access);
   for measurement sweeps -- results are identical for every setting */
void mvx_set_tuning(int tr, int hot, int nt);
/* Tableau refresh.  A dense Gauss-Jordan tableau carries the rounding of every pivot it has been through (GLPK
   refactorises its basis behind glp_simplex, bs.cpp:117).  A solve that ends OPTIMAL on a handle with at least
   `check_every` pivots since the last look (default 1024; clones inherit the count) computes the residual of the row
   equations, max_i |sum_j a_ij x_j - x_Ri| / (1 + |x_Ri|), over 32 rows picked from the pivot count (mvx_row_residual
   gives it over all rows); above `tol` (default 1e-9) the tableau
   is rebuilt from the model for the same basis -- slack tableau with the non-basic variables on their bounds, then
   the basic structural variables pivoted back in by ascending variable number, each on the row of largest |entry|
   among the rows whose auxiliary has to leave -- and the simplex carries on.  Same rule, same arithmetic, in the
   CPU oracle.  mvx_get_refresh_cnt: refreshes on this handle's lineage */
void mvx_set_refresh(int check_every, double tol);
int mvx_get_refresh_cnt(const mvx_prob *P);
double mvx_row_residual(const mvx_prob *P);
/* resident-tableau path of primal phase 2 (cache-resident sizes: one launch keeps the tableau in LDS for the whole
   run of pivots): 1 on, 0 off, -1 back to the default (on unless the environment has MVX_PERSIST=0).  Results are
   identical either way.  mvx_persist_stats: launches made / launches that aborted and were redone by the two-kernel path */
void mvx_set_persist(int mode);
/* Pivots one pass over the tableau applies on the fused primal path (the chained selection):
   0 = by tableau size (default), 1 = one pivot per pass, 2..32 = chains of that length.  Results do not depend on it. */
void mvx_set_chain(int len);
/* Who chooses the steps of a chain: 1 (default) one launch per chain -- up to 32 workgroups that stay resident and
   exchange their candidates through the L2 of the XCD they share (k_chain); 0 two launches per step (k_pc / k_pr), which
   also take over by themselves if a cluster launch ever gives up waiting for a peer.  Results do not depend on it.
   mvx_cluster_stats: cluster launches made / launches that gave up */
void mvx_set_cluster(int on);
void mvx_cluster_stats(long long *launches, long long *aborts);
/* the same for the dual simplex steps of the generic path (every warm-started B&B child): 0 = default (8 for launches
   shared by 32 or more node LPs and for tableaux of 16 MB and more, else 4), 1 = off, 2..8 = dual pivots one update
   pass applies */
void mvx_set_dual_chain(int len);
/* Fused dual path (k_dboot / k_da / k_fb<DUAL>) of a single handle's dual simplex: 0 = never, 1 = by tableau size (from
   2 M up to 12 M entries), 2 = always, -1 = back to the default (MVX_DUAL_FUSED if set, else 1).  Results are identical
   either way.  mvx_dual_fused_stats: runs k_dboot started / pivots the fused pair committed, both counted on the device */
void mvx_set_dual_fused(int mode);
void mvx_dual_fused_stats(long long *boots, long long *pivots);
void mvx_persist_stats(long long *launches, long long *aborts);
/* shader-clock cycles workgroup 0 spent per phase of the resident-tableau loop, summed over launches: propose, gather,
   read, apply; out5[4] = pivots */
void mvx_persist_cycles(unsigned long long *out5);
/* number of handles that share one launch in mvx_simplex_batch (default 64, 2..256) */
void mvx_set_batch_slots(int slots);
/* block until all work queued on the engine stream has finished */
void mvx_sync(void);
/* Device out-of-memory never aborts: a solve that cannot get its tableau returns MVX_EFAIL (status MVX_UNDEF), a clone
   that cannot get one keeps the model only, a row append that cannot grow its slab drops the tableau (the next solve
   restarts from the slack basis) -- and this call reads MVX_ENOMEM once (0 = nothing happened since the last call).
   Threads: callers use one host thread at a time per handle (GLPK's contract); the engine itself is safe for the one
   split mvx_branchAndBound makes -- batch solves on a worker thread while the calling thread clones, edits, queries
   and deletes OTHER handles. */
int mvx_last_error(void);
/* HIP's current device is per host thread: a thread other than the one that made the first engine call calls this
   once before it uses handles (0 on success) */
int mvx_bind_thread(void);

#ifdef __cplusplus
}
#endif
#endif
