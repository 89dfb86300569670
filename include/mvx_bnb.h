/*
 * mvx_bnb.h -- C ABI of the branch-and-bound driver that sits on top of the LP engine.
 *
 * The driver is the MI355X-side counterpart of MVOLPS's own code around glp_simplex:
 *   branchAndBound      /root/reference/bs.cpp:54-348      (bs.h:7)
 *   printInfo           /root/reference/util.cpp:414-473
 *   pickNode / pickVar  /root/reference/util.cpp:154-230   (ParameterObj, util.h:61-99)
 *   getFract            /root/reference/util.cpp:11-23
 *   generateCut3        /root/reference/gmi.cpp:11-117     (gmi.h:7)
 *   CutPool             /root/reference/cut.cpp:6-46       (cut.h:15-23)
 *
 * It talks to its LP engine only through `mvx_lp_api`, a table of exactly the GLPK-shaped
 * entry points MVOLPS binds -- that table IS the drop-in boundary.
 * mvx_hip_lp_api() returns the gfx950 engine's table (the only engine this library ships;
 * passing NULL selects it).
 */
#ifndef MVX_BNB_H
#define MVX_BNB_H

#include "mvx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvx_lp_api {
  void *(*create_prob)(void);
  void (*erase_prob)(void *P);
  void (*delete_prob)(void *P);
  void (*copy_prob)(void *dst, const void *src, int names);
  int (*add_rows)(void *P, int nrs);
  void (*set_mat_row)(void *P, int i, int len, const int *ind, const double *val);
  void (*set_row_bnds)(void *P, int i, int type, double lb, double ub);
  void (*set_col_bnds)(void *P, int j, int type, double lb, double ub);
  int (*simplex)(void *P, const void *parm);
  int (*get_status)(const void *P);
  double (*get_obj_val)(const void *P);
  double (*get_obj_coef)(const void *P, int j);
  double (*get_col_prim)(const void *P, int j);
  int (*get_num_rows)(const void *P);
  int (*get_num_cols)(const void *P);
  int (*get_col_kind)(const void *P, int j);
  int (*get_col_stat)(const void *P, int j);
  int (*get_row_stat)(const void *P, int i);
  double (*get_row_ub)(const void *P, int i);
  double (*get_row_lb)(const void *P, int i);
  double (*get_col_ub)(const void *P, int j);
  double (*get_col_lb)(const void *P, int j);
  int (*get_col_type)(const void *P, int j);
  int (*get_mat_row)(const void *P, int i, int *ind, double *val);
  int (*eval_tab_row)(const void *P, int k, int *ind, double *val);
  int (*get_it_cnt)(const void *P);
  /* optional (may be NULL): solve `count` independent handles concurrently, same results as
     `count` simplex calls -- used for the two children of a branch (bs.cpp:279,287) */
  int (*simplex_batch)(void **probs, int count, const void *parm, int *rcs);
  /* optional (may be NULL = maximisation): GLP_MIN / GLP_MAX.  bs.cpp compares bounds as a maximiser
     (bs.cpp:172,210) whatever the direction; with reference_quirks = 0 the driver turns the compares
     round for a minimisation problem */
  int (*get_obj_dir)(const void *P);
  /* optional (may be NULL): generateCut3 / the repaired formula for `count` basic integer columns of a solved node in
     one call (mvx_gmi_cuts: tableau rows, coefficient formula and back-substitution on the device); the driver then
     generates a node's cuts through it instead of one eval_tab_row + m get_mat_row calls per cut */
  int (*gmi_cuts)(const void *P, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok);
  /* optional (may be NULL): one cut from each of `count` different solved handles (mvx_gmi_cuts_many): the window driver
     generates the cuts of a whole round through it */
  int (*gmi_cuts_many)(const void *const *Ps, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok);
  /* optional (may be NULL): get_col_prim for every column at once, x[1..n] -- printInfo (util.cpp:414-473) reads all n
     values of every node */
  void (*get_col_prim_all)(const void *P, double *x);
  /* optional (may be NULL): printInfo (util.cpp:414-473) of `count` solved handles in one call (mvx_classify_many):
     status[t] -1/0/1, nviol[t] violated columns, their indices (ascending) in viol[t*cap ...] and their values in
     xviol[t*cap ...]; non-zero return: the caller classifies on the host */
  int (*classify_many)(const void *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol, int cap);
  /* optional (may be NULL): the solved tableau, (m+1) x (n+1) packed row-major (mvx_get_tableau), and the basis, head[0..m],
     nb[0..n], flag[0..n] (mvx_get_basis); mvx_bnb_penalties computes the branching penalties of var_strat 3 / 4 from them */
  int (*get_tableau)(const void *P, double *out);
  int (*get_basis)(const void *P, int *head, int *nb, int *flag);
  /* optional (may be NULL): the same penalties for the candidates of `count` solved handles in one call
     (mvx_branch_penalties_many); the driver prefers it to the host computation */
  int (*branch_penalties_many)(const void *const *Ps, int count, const int *cols, const int *col_off, double tol, double *pen_down,
                               double *pen_up, int *arg_down, int *arg_up);
  /* optional (may be NULL): the primal rounding heuristic (DESIGN.md "Primal rounding heuristic") on `count` solved handles
     in one call (mvx_round_many), the model taken from `root`; without it, or when it returns -5 (more columns than the
     kernel holds), the driver runs the host twin mvx_bnb_round */
  int (*round_many)(const void *root, const void *const *Ps, int count, int mode, double *obj, int *found, double *x);
  /* optional (may be NULL): reduced-cost bound tightening (DESIGN.md "Reduced-cost tightening") of `count` solved handles
     in one call (mvx_rc_tighten_many): handle t's changed columns, ascending, in cols / lb / ub[t*n .. t*n + cnt[t] - 1];
     without it the driver runs the host twin mvx_bnb_rc_tighten */
  int (*rc_tighten_many)(const void *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb, double *ub);
  /* optional (may be NULL): the bound lists of `count` handles applied in one call (mvx_tighten_cols_many), handle t taking
     entries off[t] .. off[t+1]-1; without it the driver calls set_col_bnds per entry */
  int (*tighten_cols_many)(void *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);
  /* optional (may be NULL): node bound propagation (DESIGN.md "Node bound propagation") of `count` handles over the rows of
     `root` in one call (mvx_propagate_many); without it, or when it returns -5 (more columns than the kernel holds), the
     driver runs the host twin mvx_bnb_propagate */
  int (*propagate_many)(const void *root, const void *const *Ps, int count, int max_rounds, int *infeasible, int *rounds, int *cnt, int *cols,
                        double *lb, double *ub);
  /* optional (may be NULL): general bound lists of `count` handles applied in one call (mvx_set_col_bnds_many), handle t taking
     entries off[t] .. off[t+1]-1, +-inf for an absent bound; without it the driver calls set_col_bnds per entry */
  int (*set_col_bnds_many)(void *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);
  /* optional (may be NULL): the diving heuristic's branching pick (DESIGN.md "LP diving heuristic") for `count` (solved handle,
     rule) pairs in one call (mvx_dive_pick_many), the model taken from `root`; without it, or when it returns -5 (more columns
     than the kernel holds), the driver runs the host twin mvx_bnb_dive_pick */
  int (*dive_pick_many)(const void *root, const void *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir, double *val);
  /* optional (may be NULL): glp_set_obj_coef; on a handle with a tableau the cost row follows.  The feasibility pump applies
     its objectives through it, column by column, where the table has no set_obj_many */
  void (*set_obj_coef)(void *P, int j, double coef);
  /* optional (may be NULL): the whole objective of `count` handles replaced in one call (mvx_set_obj_many), handle t taking
     c[t*(n+1) .. ]; each is left as set_obj_coef per entry leaves it */
  int (*set_obj_many)(void *const *Ps, int count, const double *c);
  /* optional (may be NULL): the feasibility pump's rounding and distance objective (DESIGN.md "Feasibility pump") of `count`
     solved handles in one call (mvx_pump_obj_many), the model taken from `root`; without it, or when it returns -5 (more
     columns than the kernel holds), the host twin mvx_bnb_pump_obj runs */
  int (*pump_obj_many)(const void *root, const void *const *Ps, int count, const double *xprev, const int *has_prev, const double *ab,
                       int *info, double *xt, double *c);
  /* optional (may be NULL): the scores of `k` candidate cut rows against a solved handle in one call (mvx_cut_scores; DESIGN.md
     "Root cut rounds"): dot[t] against the column values and the k x k Gram matrix; without it the host twin mvx_bnb_cut_scores
     runs */
  int (*cut_scores)(const void *P, int k, const double *vals, double *dot, double *gram);
  /* optional (may be NULL): `k` dense MVX_LO rows appended in one call (mvx_add_cut_rows), the handle left as k times add_rows(1),
     set_mat_row, set_row_bnds leave it; without it the root cut loop appends row by row */
  int (*add_cut_rows)(void *P, int k, const double *vals, const double *rhs);
  /* optional (may be NULL): the conflict graph of the binary columns of a handle in one call (mvx_conflict_graph; DESIGN.md
     "Clique cuts (cut_families)"); without it, or when it returns -5, the host twin mvx_bnb_conflict_graph runs */
  int (*conflict_graph)(const void *model, unsigned long long *adj, long long *edges);
  /* optional (may be NULL): rows num[1..nrs] taken out of a handle in one call (mvx_del_rows, glp_del_rows' shape; DESIGN.md "Cut
     purging (cut_purge)"), 0 on success; without it, or when it fails, the root cut loop turns a purged row into a free row */
  int (*del_rows)(void *P, int nrs, const int *num);
  /* optional (may be NULL): the incumbent polishing (DESIGN.md "Incumbent polishing (polish)") of `count` points in one call
     (mvx_polish_many), the model taken from `root`; without it, or when it returns -5, the host twin mvx_bnb_polish runs */
  int (*polish_many)(const void *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok);
  /* optional (may be NULL): del_rows on `count` distinct handles in one call (mvx_del_rows_many; DESIGN.md "Cut purging in the
     tree (node_purge)"): handle t loses the rows rows[off[t] .. off[t+1]-1] (1-based), 0 on success; without it, or when it
     fails, the tree's purge calls del_rows handle by handle, and without that makes each purged row a free row */
  int (*del_rows_many)(void *const *Ps, int count, const int *off, const int *rows);
  /* optional (may be NULL): the clique separation of `count` solved handles against the conflict graph of `root` in one call
     (mvx_clique_cuts_many; DESIGN.md "Clique cuts in the tree (node_cliques)"); without it, or when it returns -5, the host twin
     mvx_bnb_clique_masks runs handle by handle */
  int (*clique_cuts_many)(const void *root, const void *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q, double *sum);
  /* optional (may be NULL): add_cut_rows on `count` distinct handles in one call (mvx_add_cut_rows_many): handle t takes rows
     off[t] .. off[t+1]-1 of vals / rhs; without it, or when it returns -1, the tree's clique rows go through add_cut_rows handle
     by handle, and without that through add_rows / set_mat_row / set_row_bnds row by row.  -2 (device memory) means the rows are
     in every model: nothing is appended again */
  int (*add_cut_rows_many)(void *const *Ps, int count, const int *off, const double *vals, const double *rhs);
  /* optional (may be NULL): the KKT check of `count` solved handles against the rows of `root` in one call (mvx_kkt_many; DESIGN.md
     "KKT check (kkt)"): val / ind take 8 entries per handle; without it the host twin mvx_bnb_kkt runs handle by handle */
  int (*kkt_many)(const void *root, const void *const *Ps, int count, double *val, int *ind);
  /* optional (may be NULL): the Farkas proof of `count` handles against the rows of `root` in one call (mvx_farkas_many; DESIGN.md
     "Infeasibility and unboundedness proofs (farkas)"): val / ind take 4 entries per handle; without it the host twin
     mvx_bnb_farkas runs handle by handle */
  int (*farkas_many)(const void *root, const void *const *Ps, int count, double *val, int *ind);
} mvx_lp_api;

const mvx_lp_api *mvx_hip_lp_api(void);

/* ParameterObj (util.h:61-99); defaults VO / DFS(=FIFO) / no cuts (util.h:65-67) */
typedef struct {
  int var_strat;        /* 0 VO, 1 VFP, 2 VGO   (util.h:30); extensions that read the node LP (DESIGN.md "Branching on
                           the node LP"): 3 largest product of one-step dual penalties, 4 strong branching on the
                           sb_cands best of them.  3 / 4 need get_tableau + get_basis or branch_penalties_many in the
                           table, and are refused (mvx_branchAndBound returns -1) together with best_window > 0 */
  int node_strat;       /* 0 DFS (problems.front(), util.cpp:165), 1 BEST (util.cpp:170-186) */
  int cut_strat;        /* 0 NONE, 1 GMI         (util.h:32) */
  double cut_chance;    /* -cf: stored, never read (util.cpp:259-261) */
  int loop_limit;       /* bs.cpp:320: 200000 branchings */
  int max_nodes;        /* stop after this many loop iterations (<= 0: none) */
  int reference_quirks; /* 1 (default): bug-compatible with bs.cpp / util.cpp;
                           0: children keep the opposite bound (bs.cpp:274,282 drop it), the
                           integrality test has a 1e-9 tolerance, cuts are the repaired GMI of
                           mvx_generateCutGMI and are not carried from node to node, and a
                           minimisation problem is bounded and pruned as one (best_lower is then the
                           best upper bound) */
  int lazy_pool;        /* 1 (default): generate only the cut cut.cpp:20 will actually add (the last
                           eligible column's; with reference_quirks = 0 and cut_select = 0 the last column
                           that yields a cut); 0: generate every cut like bs.cpp:250-255 */
  int cut_select;       /* reference_quirks = 0 only (changes results, hence not the
                           default path).  0: add the last generated cut (cut.cpp:20); 1: add the
                           ceil(cut_chance * k) most effective of the node's k cuts (-cf honoured) */
  int window;           /* FIFO order, engine with a batch entry: solve the front `window` nodes of the deque
                           together and replay bs.cpp's decisions (cuts included: the replay is in queue
                           order, so the persistent pool sees the nodes as bs.cpp does) -- same tree, oids,
                           events and incumbent as node-at-a-time; default 64, 1 = node
                           at a time */
  int best_window;      /* BEST order (node_strat = 1), engine with a batch entry: the top `best_window` open nodes
                           are solved, classified and branched together and their decisions replayed in true
                           best-bound order; the longest prefix the serial loop would also have popped is kept --
                           same tree, oids, events and incumbent as node-at-a-time.  Default 0 = node at a time */
  int sb_cands;         /* var_strat = 4: candidates (best penalty scores first) whose two children are strong-branched;
                           default 2 (CPU sweep) */
  int sb_iters;         /* var_strat = 4: pivot limit of each strong-branching child solve; default 4 */
  int heur;             /* primal rounding heuristic (DESIGN.md "Primal rounding heuristic") on every node that branches, on
                           its LP as solved: 0 off (default), 1 round and check, 2 round, check and fill.  Needs
                           reference_quirks = 0; a better feasible point becomes the incumbent */
  int rc_fix;           /* reduced-cost bound tightening (DESIGN.md "Reduced-cost tightening"): 0 off (default), 1 on every node
                           that reaches the branch decision while an incumbent exists, on its LP as solved; the tightened
                           bounds go to both children.  Needs reference_quirks = 0 and best_window = 0 */
  int prop;             /* node bound propagation (DESIGN.md "Node bound propagation"): 0 off (default), 1..16 the round limit.  The
                           root (behind the rounding of its bounds) and every child (behind its branching bound and its rc_fix
                           list, in front of its first solve) have the bounds of their integer columns tightened from the
                           activities of the root's rows.  Needs reference_quirks = 0 and best_window = 0 */
  int dive;             /* LP diving heuristic (DESIGN.md "LP diving heuristic"): 0 off (default), 1..7 the rules that dive, as bits:
                           1 fractional, 2 locks, 4 vector length.  A node that reaches the branch decision with an OPT LP is
                           dived behind the rounding heuristic and in front of rc_fix, on its LP as solved; a better feasible
                           point becomes the incumbent.  Needs reference_quirks = 0 and best_window = 0 */
  int dive_freq;        /* 0 (default): the root only; F > 0: also every branching node with oid % F == 0 */
  int dive_depth;       /* step limit of one dive; 0 (default): 4 n + 64, a cap against a dive that never ends */
  int pump;             /* feasibility pump (DESIGN.md "Feasibility pump"): 0 off (default), 1..1000 the limit of distance LPs of one
                           pump.  A node that reaches the branch decision with an OPT LP is pumped behind the rounding heuristic
                           and in front of the dives, on its LP as solved; a better feasible point becomes the incumbent.
                           Needs reference_quirks = 0 and best_window = 0 */
  int pump_freq;        /* 0 (default): the root only; F > 0: also every branching node with oid % F == 0 */
  double pump_alpha;    /* 0 (default) the plain pump; up to 1: the weight of the root's objective in the first distance LP, times
                           0.9 with every further one */
  int cut_rounds;       /* root cut rounds (DESIGN.md "Root cut rounds"): 0 off (default), 1..64 the rounds of GMI cuts the root LP
                           takes before the tree starts: per round the repaired cuts of all fractional basic integer columns,
                           ranked by efficacy, filtered by pairwise parallelism and appended together.  Needs reference_quirks = 0;
                           the tree then runs on a copy of the caller's handle.  Independent of cut_strat */
  int cut_round_max;    /* most cuts one round appends, 0..4096; 0 (default): 32 */
  double cut_maxpar;    /* a cut is taken when its cosine to every cut already taken in the round is at most this, in (0, 1];
                           0.0 (default): 0.9.  With cut_rounds = 0 neither this nor cut_round_max is read */
  int cut_families;     /* the cut families of the root cut rounds (DESIGN.md "Clique cuts (cut_families)"), as bits: 1 the repaired
                           GMI cuts, 2 clique cuts from the conflict graph of the binary columns; 0 (default) means 1.  Read only
                           when cut_rounds > 0; a value outside 0..3 is then refused */
  int cut_purge;        /* purging of slack cut rows in the root cut rounds (DESIGN.md "Cut purging (cut_purge)"): 0 (default) no row
                           leaves; A = 1..64: a row the loop appended is taken out again once its auxiliary variable has been basic
                           after A consecutive re-solves.  Read only when cut_rounds > 0; a value outside 0..64 is then refused */
  int polish;           /* incumbent polishing (DESIGN.md "Incumbent polishing (polish)"): 0 off (default), N = 1..100000 the move cap.
                           Every point that becomes the incumbent -- an integral node LP's, the rounding heuristic's, a dive's, a
                           pump's -- is first improved by a best-improvement search over one- and two-column unit moves; the
                           decision whether it becomes the incumbent is taken on the point as found.  Needs reference_quirks = 0;
                           allowed with best_window > 0 */
  int node_purge;       /* purging of slack cut rows in the tree (DESIGN.md "Cut purging in the tree (node_purge)"): 0 (default) no
                           row leaves; A = 1..64: a row behind the caller's rows -- a cut_strat row of an ancestor, or a row of the
                           root cut rounds -- leaves both children of a branching node once its auxiliary variable has been basic
                           at A consecutive branching nodes on the path.  Outside 0..64: refused; A > 0 needs
                           reference_quirks = 0 and best_window = 0, and get_row_stat in the table */
  int node_cliques;     /* clique cuts in the tree (DESIGN.md "Clique cuts in the tree (node_cliques)"): 0 (default) off; K = 1..64:
                           every node that reaches the branch decision with an OPT LP has up to K violated cliques of the model's
                           conflict graph separated against its LP as solved, and their rows go to both children, behind the
                           purge and in front of the rc_fix lists, the propagation and the first solve.  Outside 0..64: refused;
                           K > 0 needs reference_quirks = 0 and best_window = 0.  Independent of cut_strat and of the root cut
                           rounds */
  int kkt;              /* KKT check (DESIGN.md "KKT check (kkt)"): 0 (default) off; 1: every node LP the tree solves -- whatever its end
                           status -- is checked against the model as solved, a window's nodes in one kkt_many call; the tree's worst
                           relative errors go to kkt_re / kkt_oid.  Pure observation: the tree, oids, events, pivots, incumbent
                           and every other counter are those of kkt = 0, and the booked values do not depend on the window.  Outside 0..1: refused; 1 needs best_window = 0; allowed
                           in both quirk modes */
  int farkas;           /* Farkas proof (DESIGN.md "Infeasibility and unboundedness proofs (farkas)"): 0 (default) off; 1: every node LP
                           that ends MVX_NOFEAS is asked for a proof of its infeasibility on the model, a window round's nodes in one
                           farkas_many call; the farkas_* members of the result count what was proved.  Pure observation: the tree,
                           oids, events, pivots, incumbent and every other counter are those of farkas = 0, and the booked values do
                           not depend on the window.  Outside 0..1: refused; 1 needs best_window = 0; allowed in both quirk modes */
} mvx_bnb_params;

/* B&B events at the emit points of bs.cpp (message.h EventType) */
#define MVX_EV_PREGNANT 0   /* bs.cpp:119-129 */
#define MVX_EV_INTEGER 1    /* bs.cpp:163-166 */
#define MVX_EV_INFEASIBLE 2 /* bs.cpp:199-203 */
#define MVX_EV_FATHOMED 3   /* bs.cpp:215-217 */
#define MVX_EV_BRANCHED 4   /* bs.cpp:225-244 */
#define MVX_EV_CANDIDATE 5  /* bs.cpp:300-318 */

typedef struct {
  int type, oid, pid, direction; /* direction 0 M, 1 R, 2 L (bs.cpp:43-52) */
  double lp_bound;               /* field6 */
  double sum_infeas;             /* field7 (bs.cpp:227-241) */
  int n_violated;                /* field8 */
  int pick;                      /* branching variable of a branched event, else 0 */
} mvx_bnb_event;

typedef struct {
  int n_nodes;        /* oids are 1..n_nodes (util.h:17, util.cpp:29-30) */
  int *parent;        /* parent[oid]; 0 for the root (bs.cpp:26-33) */
  int *prune;         /* prune[oid]: 0 INTG, 1 FEAS, 3 BNDS, 4 NONE (util.h:27) */
  double *node_bound; /* NodeData::upperBound */
  int n_events;
  mvx_bnb_event *events;
  int count;          /* loop iterations (bs.cpp:326) */
  int has_incumbent;
  double best_lower;  /* bs.cpp:90,172-174 */
  int incumbent_oid;
  int n;
  double *x;          /* x[1..n] of the incumbent (bs.cpp:181-187) */
  long long total_pivots;
  int hit_limit;
  long long rounds;     /* best_window driver only (0 otherwise): rounds of speculation */
  long long speculated; /* best_window driver only (0 otherwise): nodes taken into a round's window, summed */
  long long sb_lps;     /* var_strat = 4: strong-branching child LPs solved for the nodes that branched */
  long long sb_pivots;  /* their pivots (not part of total_pivots) */
  long long heur_calls;    /* heur > 0: nodes the rounding heuristic ran on (the nodes that branched) */
  long long heur_found;    /* ... of which it returned a feasible point */
  long long heur_improved; /* ... of which the point became the incumbent */
  int incumbent_heur;      /* 1: the final incumbent came from the rounding heuristic, 2: from a dive, 3: from a pump, 0: from an
                              integral node LP (or none) */
  long long rc_calls;      /* rc_fix = 1: branching nodes the reduced-cost tightening ran on */
  long long rc_fixed;      /* ... entries of their lists with lb == ub */
  long long rc_tightened;  /* ... the other entries */
  long long prop_calls;      /* prop > 0: handles the propagation ran on (the root and every child) */
  long long prop_fixed;      /* ... entries of their applied lists with lb == ub */
  long long prop_tightened;  /* ... the other entries */
  long long prop_infeasible; /* ... handles it proved infeasible (a child keeps its bounds and is solved as before) */
  long long dive_calls;    /* dive > 0: nodes dived */
  long long dive_found;    /* ... of which at least one rule's dive returned a feasible point */
  long long dive_improved; /* ... of which the point became the incumbent */
  long long dive_lps;      /* child LPs the dives solved, failed sides included */
  long long dive_pivots;   /* their pivots (not part of total_pivots) */
  long long pump_calls;    /* pump > 0: nodes pumped */
  long long pump_found;    /* ... of which the pump returned a feasible point */
  long long pump_improved; /* ... of which the point became the incumbent */
  long long pump_lps;      /* distance LPs the pumps solved */
  long long pump_pivots;   /* their pivots (not part of total_pivots) */
  long long cutloop_rounds;     /* cut_rounds > 0: rounds that appended cuts and re-solved */
  long long cutloop_candidates; /* ... cuts made for them (one per fractional basic integer column that yields a cut) */
  long long cutloop_rows;       /* ... rows appended */
  long long cutloop_lps;        /* ... LPs solved: the root's first solve and one per round */
  long long cutloop_pivots;     /* their pivots (not part of total_pivots; the root's own LP is among them) */
  double cutloop_bound0;        /* the root LP before the loop */
  double cutloop_bound;         /* the root LP after it (the last one that ended optimal) */
  long long cutloop_conflicts;    /* cut_families & 2: edges of the conflict graph */
  long long cutloop_clique_cands; /* ... violated cliques the separation kept, summed over the rounds (part of cutloop_candidates) */
  long long cutloop_clique_rows;  /* ... clique rows appended (part of cutloop_rows) */
  long long cutloop_purged;       /* cut_purge > 0: rows of the loop taken out again (deleted, or made free rows) */
  long long cutloop_live_rows;    /* rows of the loop the tree starts with: cutloop_rows - cutloop_purged */
  long long polish_calls;    /* polish > 0: points polished (every point that became the incumbent) */
  long long polish_moves;    /* ... moves taken, summed */
  long long polish_improved; /* ... points that came back with a better objective */
  long long node_purge_calls;   /* node_purge > 0: child handles that lost at least one row */
  long long node_purge_rows;    /* ... rows removed, summed over the child handles (deleted, or made free rows) */
  long long node_cut_rows_peak; /* the most live rows behind the caller's rows that any solved node carried (with node_purge = 0 too) */
  long long node_clique_conflicts; /* node_cliques > 0: edges of the conflict graph of the model */
  long long node_clique_calls;     /* ... branching nodes whose LP was separated */
  long long node_clique_rows;      /* ... cliques kept for them, summed: each is one row in both children */
  long long kkt_nodes;             /* kkt = 1: node LPs checked (every node the tree solved) */
  double kkt_re[4];                /* ... the worst re_max over them per condition: PE, PB, DE, DB */
  int kkt_oid[4];                  /* ... the lowest oid at which each worst value occurred, 0 while it is 0 */
  long long farkas_nodes;          /* farkas = 1: node LPs that ended MVX_NOFEAS, each asked for a proof */
  long long farkas_proved;         /* ... found = 2: the proof holds on the model */
  long long farkas_tableau_only;   /* ... found = 1: a tableau row proves, the model does not confirm it */
  long long farkas_none;           /* ... found = 0: no tableau row proves */
  long long farkas_dropped;        /* ... nodes with found > 0 whose model side dropped a coefficient under the zero rule */
  double farkas_rel_min;           /* ... the smallest model-side rel among the proved nodes, 0 while there is none */
  double farkas_de_max;            /* ... the largest de among the nodes with found > 0 */
  int farkas_rel_oid;              /* ... the lowest oid of farkas_rel_min, 0 while there is none */
  int farkas_de_oid;               /* ... the lowest oid of farkas_de_max, 0 while it is 0 */
} mvx_bnb_result;

void mvx_bnb_default_params(mvx_bnb_params *p);
/* int branchAndBound(glp_prob*, MVOLP::ParameterObj&)  bs.h:7.  Returns 0; -1 refused parameters (var_strat outside
   0..4, var_strat >= 3 with best_window > 0, heur outside 0..2, heur > 0 with reference_quirks = 1) -- *res is then
   empty; -2 var_strat >= 3 and the branching penalties could not be computed (the table has neither
   branch_penalties_many nor get_tableau + get_basis, or they failed), or heur > 0 and the heuristic could not run (the
   table has neither round_many nor the accessors of mvx_bnb_round, or they failed) -- *res holds the tree up to that
   node.  rc_fix, prop, dive and pump have the same two codes; their refusals are listed with their host twins below */
int mvx_branchAndBound(const mvx_lp_api *api, void *prob, const mvx_bnb_params *params, mvx_bnb_result *res);
void mvx_bnb_free_result(mvx_bnb_result *res);

double mvx_getFract(double x); /* util.cpp:11-23 */
/* std::pair<int, std::vector<int>> printInfo(glp_prob*, bool)  util.cpp:414 */
int mvx_printInfo(const mvx_lp_api *api, const void *prob, int quirks, int *violated, int *nviolated);
/* CutContainer generateCut3(glp_prob*, int j)  gmi.h:7; inds/vals hold n+1 entries, returns -1 when rejected */
int mvx_generateCut3(const mvx_lp_api *api, const void *prob, int j, int *inds, double *vals, double *lb);

/* Repaired Gomory mixed-integer cut (used when reference_quirks = 0): non-basic variables measured
   from the bound they sit at, f0 from the row's own value, back-substitution by column index.
   Same output layout as mvx_generateCut3; *efficacy = violation / 2-norm at the current vertex */
int mvx_generateCutGMI(const mvx_lp_api *api, const void *prob, int j, int *inds, double *vals, double *lb, double *efficacy);

/* ---- node-level helpers for window drivers (mvolps_amd/dist_bnb.py): one call per node instead of
   one per query.  Same arithmetic, same order as the loop body of bs.cpp. ---- */
/* classification of a solved node (bs.cpp:135-156,227-241,260): out[0] status -1/0/1 (printInfo),
   out[1] objective, out[2] number of violated columns, out[3] sum of their fractional parts,
   out[4] pickVar's choice (0 when none), `root` = ParameterObj::_prob;
   var_strat 0..2 only: -1 (nothing written) for var_strat >= 3, whose choice needs the node LP's penalties */
int mvx_bnb_classify(const mvx_lp_api *api, const void *prob, const void *root, int quirks, int var_strat, double *out);
/* bs.cpp:261-282: bound = col_prim(a, pick); S2/S3 = clones of `a` (created by the caller with
   create_prob) with the branching bounds set; they are NOT solved here (the caller batches them) */
int mvx_bnb_make_children(const mvx_lp_api *api, const void *a, int pick, int quirks, void *S2, void *S3);
/* The repaired mode's rule for integer columns with fractional bounds, which every repaired driver applies to (a copy of)
   its root before the first solve: lb -> ceil(lb), ub -> floor(ub), type FX where they meet; integral bounds are not
   touched.  Edits `prob` in place.  Returns 0 nothing to round, 1 bounds rounded, 2 some column's range holds no integer
   (the model is infeasible; `prob` may be partly edited) */
int mvx_bnb_integral_bounds(const mvx_lp_api *api, void *prob);
/* The same scan without writing anything: what mvx_bnb_integral_bounds would return for `prob` */
int mvx_bnb_fractional_bounds(const mvx_lp_api *api, const void *prob);

/* Host twin of mvx_branch_penalties_many for one solved handle, from get_tableau and get_basis: for each basic column
   cols[t], pen_down[t] / pen_up[t] = fd / fu times the smallest |T[0][q]| / |T[i][q]| over the non-basic positions q that
   move x_j down / up (|T[i][q]| > tol), +inf where none does; arg_down[t] / arg_up[t] the position (lowest on ties, 0 for
   +inf).  Returns 0; -1 bad arguments or a column outside 1..n; -3 the handle is not MVX_OPT; -4 a column that is not
   basic; -5 the table has no get_tableau / get_basis or they failed */
int mvx_bnb_penalties(const mvx_lp_api *api, const void *prob, const int *cols, int count, double tol, double *pen_down, double *pen_up,
                      int *arg_down, int *arg_up);

/* Sensitivity ranges (DESIGN.md "Sensitivity ranges (ranges)"), host twin of mvx_ranges for one solved handle: val
   (m+n+1) x 6 doubles (ACT_DN, ACT_UP, OBJ_DN, OBJ_UP, COST_DN, COST_UP) and var (m+n+1) x 4 ints (LIM_DN, LIM_UP, ENT_DN,
   ENT_UP) by variable number, row 0 zero.  Works through the table only (get_tableau, get_basis, row and column bounds,
   get_obj_dir, get_status, get_num_rows, get_num_cols); the handle is not changed; entries count above the default pivot
   tolerance.  The same bits as mvx_ranges.  Returns 0; -1 a null argument; -2 the table lacks an accessor it needs (or
   get_tableau / get_basis failed); -3 the handle is not MVX_OPT */
int mvx_bnb_ranges(const mvx_lp_api *api, const void *prob, double *val, int *var);

/* KKT check (DESIGN.md "KKT check (kkt)") from numbers only: m rows and n columns, rows m x (n+1) dense by row (entry 0 of each
   unused), c[0..n], the four value vectors xs[0..n] (get_col_prim), xr[0..m] (get_row_prim), lam[0..m] (get_row_dual), dj[0..n]
   (get_col_dual), lb / ub / stat [0..m+n] by variable number, auxiliaries first (+-inf for an absent bound; MVX_BS .. MVX_NS),
   dir MVX_MIN / MVX_MAX.  val[8] = ae_max, re_max of PE, PB, DE, DB, ind[8] where they occur (lowest among equals, 0 for a zero
   maximum); r_pe[0..m] / r_de[0..n] (nullable) the residuals, entry 0 zero.  Sums run in 64 chains with fma, combined by the
   halving tree.  Returns 0; -1 bad arguments (m < 1, n < 1, a null, another dir) */
int mvx_bnb_kkt_values(int m, int n, const double *rows, const double *c, const double *xs, const double *xr, const double *lam,
                       const double *dj, const double *lb, const double *ub, const int *stat, int dir, double *val, int *ind, double *r_pe,
                       double *r_de);
/* Host twin of mvx_kkt for one solved handle, through the table only (get_mat_row, row and column bounds, get_obj_coef,
   get_obj_dir, get_tableau, get_basis, get_status, get_num_rows, get_num_cols): the four vectors are derived by the getters' own
   rule; the handle is not changed.  The same bits as mvx_kkt.  Returns 0; -1 a null argument; -2 the table lacks an accessor it
   needs (or one failed); -3 the handle is MVX_UNDEF.  mvx_branchAndBound returns -1 (*res empty) for kkt outside 0..1 and kkt = 1
   with best_window > 0, and -2, with the tree so far, when a check could not be carried out */
int mvx_bnb_kkt(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *r_pe, double *r_de);

/* Farkas proof (DESIGN.md "Infeasibility and unboundedness proofs (farkas)") from numbers only: T (m+1) x (n+1) the tableau as
   get_tableau packs it, T[i (n+1) + q] = alpha_iq of mvx_eval_tab_row (row 0 and column 0 are not read), head[0..m] the basic
   variable of each row, nb[0..n] the variable at each non-basic position, rows m x (n+1) dense by row (entry 0 of each unused),
   lb / ub [0..m+n] by variable number, auxiliaries first (+-inf for an absent bound).  val[4] = rel of the tableau side, rel of the
   model side, the model side's Lo or -Hi, de; ind[4] = found (0 none, 1 the tableau row only, 2 proved on the model), the row,
   the side (1 lower, 2 upper), the coefficients the model side dropped; all zero when found = 0.  y[0..m] (nullable) the row
   weights, entry 0 zero.  Returns 0; -1 bad arguments (m < 1, n < 1, a null) */
int mvx_bnb_farkas_values(int m, int n, const double *T, const int *head, const int *nb, const double *rows, const double *lb,
                          const double *ub, double *val, int *ind, double *y);
/* Host twin of mvx_farkas for one handle, through the table only (get_mat_row, row and column bounds, get_tableau, get_basis,
   get_status, get_num_rows, get_num_cols); the handle is not changed.  The same bits as mvx_farkas.  Returns 0; -1 a null
   argument; -2 the table lacks an accessor it needs (or one failed); -3 the handle is MVX_UNDEF.  mvx_branchAndBound returns -1
   (*res empty) for farkas outside 0..1 and farkas = 1 with best_window > 0, and -2, with the tree so far, when a proof could not
   be asked for */
int mvx_bnb_farkas(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *y);
/* Host twin of mvx_ray (mvx.h) for one handle, through the table only (get_mat_row, get_obj_coef, get_obj_dir, row and column
   bounds, get_tableau, get_basis, get_status, get_num_rows, get_num_cols): val[4], ind[6] and d[0..m+n] (nullable) as mvx_ray
   gives them, the same bits; the handle is not changed.  Returns 0; -1 a null argument; -2 the table lacks an accessor it needs
   (or one failed); -3 the handle is MVX_UNDEF */
int mvx_bnb_ray(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *d);

/* Column append (DESIGN.md "Column append (add_cols)"), host twin of mvx_price_cols: the images of `k` candidate columns against
   the tableau of `prob` -- cols k x (m+1) by model row, obj[k]; dj[t] row 0 of image t, img (nullable) k x (m+1) by tableau row.
   Works through the table only (get_num_rows, get_num_cols, get_tableau, get_basis); the handle is not changed.  The same bits
   as mvx_price_cols: 64 chains over the non-basic positions, the written tree, the base added last.  Returns 0; -1 bad
   arguments; -2 the table lacks an accessor it needs (or get_tableau / get_basis failed) */
int mvx_bnb_price_cols(const mvx_lp_api *api, const void *prob, int k, const double *cols, const double *obj, double *dj, double *img);

/* Sifting (DESIGN.md "Sifting (sift)"), the host twins of mvx_pool_price from numbers only.  mvx_bnb_pool_price_values: cols is
   N x (m+1) row-major as mvx_pool_add_cols takes it (row t is pool column t + 1, its entry 0 is not read), obj[N] and type[N]
   likewise by t, y[0..m] the row weights (y[0] is not read), dir MVX_MIN or MVX_MAX, tol the dual tolerance.  dj[0..N] receives
   dj[0] = 0 and d_j = obj_j + S_j in the written order of mvx_pool_price (64 chains over the rows with fma(-a_ij, y_i, acc) from
   +0.0, rows with y_i == 0 skipped, s[l] += s[l+h] for h = 32 .. 1, obj_j last); attractive (nullable) [0..N] the rule of
   mvx_pool_price on the status a column of type[t] enters with, attractive[0] = 0.  mvx_bnb_pool_select: of the columns j = 1..N
   with attractive[j] != 0 and skip[j] == 0 (skip nullable) the min(K, count) of largest |dj[j]| (by its bits), descending, ties to
   the lower j, into pick[0 .. *npick-1].  Both return 0, or -1 for bad arguments. */
int mvx_bnb_pool_price_values(int m, int N, const double *cols, const double *obj, const int *type, const double *y, int dir, double tol,
                              double *dj, unsigned char *attractive);
int mvx_bnb_pool_select(int N, const double *dj, const unsigned char *attractive, const unsigned char *skip, int K, int *pick, int *npick);
/* The text report of those tables, one line per variable k = 1..m+n, written to `path` (NULL: stdout):
     k name st value act_dn lim_dn act_up lim_up obj_dn obj_up cost_dn ent_dn cost_up ent_up
   name is R<i> for an auxiliary and the column's name, or C<j> without one, for a structural (names are read from the gfx950
   engine's handles only; another table gives C<j>); st one of B NL NU NF NS; value the variable's value (get_row_prim's /
   get_col_prim's bits, from the tableau and the bounds); doubles as %.17g.  Returns 0; -1 a null argument; -2 the table lacks
   an accessor; -3 the handle is not MVX_OPT; -4 the file cannot be written */
int mvx_bnb_print_ranges(const mvx_lp_api *api, const void *prob, const double *val, const int *var, const char *path);

/* Primal rounding heuristic (DESIGN.md "Primal rounding heuristic"), host twin of mvx_round_many for one solved handle:
   the node LP's column values (get_col_prim) rounded, checked against rows 1..m0 of `root` (m0 = its row count; cut
   rows are ignored), root's column bounds and objective, and with mode 2 filled greedily.  *obj the candidate's
   objective, *found 1 when it is feasible, x[1..n] the candidate (x[0] untouched).  Works through the table only
   (get_col_prim_all / get_col_prim, get_mat_row, bounds, get_obj_coef, get_col_kind, get_obj_dir).  Returns 0; -1 bad
   arguments (mode outside 1..2, another column count); -2 the table lacks an accessor it needs; -3 the handle is not
   MVX_OPT */
int mvx_bnb_round(const mvx_lp_api *api, const void *prob, const void *root, int mode, double *obj, int *found, double *x);

/* Reduced-cost bound tightening (DESIGN.md "Reduced-cost tightening"), host twin of mvx_rc_tighten_many for one solved handle
   against the cutoff (the incumbent's objective): the columns whose bounds change, ascending, in cols[0 .. *cnt - 1] with
   their new bounds in lb / ub (room for n entries each).  Works through the table only (get_tableau, get_basis, get_col_kind,
   column bounds, get_obj_dir, get_obj_val); the handle is not changed.  Returns 0; -1 bad arguments; -3 the handle is not
   MVX_OPT; -5 the table lacks an accessor it needs, or one failed.  mvx_branchAndBound with rc_fix = 1 returns -1 (*res
   empty) for rc_fix outside 0..1, reference_quirks = 1 or best_window > 0, and -2 when neither rc_tighten_many nor this
   twin can run */
int mvx_bnb_rc_tighten(const mvx_lp_api *api, const void *prob, double cutoff, double tol, int *cnt, int *cols, double *lb, double *ub);

/* Node bound propagation (DESIGN.md "Node bound propagation"), host twin of mvx_propagate_many for one handle, which need not
   be solved and is not changed: up to max_rounds Jacobi rounds of activity-based tightening of the integer columns' bounds,
   from rows 1..m0 of `root` (m0 = its row count; cut rows are ignored) and the column bounds of `prob` itself.  *infeasible 1
   when a row is contradictory or a column's bounds cross, *rounds the rounds run, the columns whose bounds changed, ascending,
   in cols[0 .. *cnt - 1] with their bounds in lb / ub (room for n entries each; +-inf for an absent bound; no entries for an
   infeasible handle).  Works through the table only (get_mat_row, row and column bounds, get_col_kind).  Returns 0; -1 bad
   arguments (max_rounds < 1, another column count); -2 the table lacks an accessor it needs.  mvx_branchAndBound returns -1
   (*res empty) for prop outside 0..16 and for prop > 0 with reference_quirks = 1 or best_window > 0, and -2, with the tree so
   far, when the propagation could not be carried out: neither propagate_many nor this twin can run, or one of its calls
   (propagate_many, set_col_bnds_many) failed, whatever that call's own code was */
int mvx_bnb_propagate(const mvx_lp_api *api, const void *prob, const void *root, int max_rounds, int *infeasible, int *rounds, int *cnt,
                      int *cols, double *lb, double *ub);

/* LP diving heuristic (DESIGN.md "LP diving heuristic"), host twin of mvx_dive_pick_many for one solved handle and one rule
   (1 fractional, 2 locks, 4 vector length): *nfrac the number of fractional integer columns, *col the one the rule branches on
   (0 when there is none), *dir 0 down / 1 up, *val its value.  The locks, column lengths and objective are those of rows
   1..m0 of `root` (m0 = its row count; cut rows are ignored).  Works through the table only (get_col_prim_all / get_col_prim,
   get_mat_row, bounds, get_obj_coef, get_col_kind, get_obj_dir).  Returns 0; -1 bad arguments (a rule outside {1, 2, 4},
   another column count); -2 the table lacks an accessor it needs; -3 the handle is not MVX_OPT */
int mvx_bnb_dive_pick(const mvx_lp_api *api, const void *prob, const void *root, int rule, int *nfrac, int *col, int *dir, double *val);
/* The whole dives of one solved node `prob` (left untouched; every clone is freed) under the rules whose bits are set in
   `rules` (1..7), each at most `depth` steps (0: 4 n + 64): per step one pick, one bounded clone solved with the default
   parameters, the opposite side once when that fails.  A dive that ends integral is rounded and checked (mvx_bnb_round, mode
   1).  *found 1 when some rule found a point, *obj / x[1..n] the best of them (ties to the lower rule), *lps / *pivots the
   child LPs solved and their pivots.  Uses the table's batched entries where it has them (dive_pick_many, simplex_batch,
   set_col_bnds_many, round_many) and the twins otherwise.  Returns 0; -1 bad arguments; -2 the table lacks an accessor; -3 the
   handle is not MVX_OPT.  mvx_branchAndBound returns -1 (*res empty) for dive outside 0..7, negative dive_freq / dive_depth and
   dive > 0 with reference_quirks = 1 or best_window > 0, and -2, with the tree so far, when a dive could not be carried out */
int mvx_bnb_dive(const mvx_lp_api *api, const void *prob, const void *root, int rules, int depth, double *obj, int *found, double *x,
                 long long *lps, long long *pivots);

/* Feasibility pump (DESIGN.md "Feasibility pump"), host twin of mvx_pump_obj_many for one solved handle: the rounding of its
   integer columns (xt[0..n]; the move of a repeated rounding when has_prev is set and it equals xprev[1..n]), and the distance
   objective c[0..n] with ab = (a, q); info[0..3] = fractional integer columns, columns moved, stalled, nnz(d).  The column
   bounds are the handle's own, the integer flags and the objective those of `root`.  Works through the table only
   (get_col_prim_all / get_col_prim, get_mat_row, bounds, get_obj_coef, get_col_kind, get_obj_dir).  Returns 0; -1 bad
   arguments; -2 the table lacks an accessor it needs; -3 the handle is not MVX_OPT */
int mvx_bnb_pump_obj(const mvx_lp_api *api, const void *prob, const void *root, const double *xprev, int has_prev, const double *ab,
                     int *info, double *xt, double *c);
/* How a pump ended (mvx_bnb_pump's *end): the LP point became integral; `iters` LPs were solved; a repeated rounding had no
   column to move; a moved rounding repeated an earlier one; a distance LP did not end optimal */
#define MVX_PUMP_INTEGRAL 1
#define MVX_PUMP_LIMIT 2
#define MVX_PUMP_STALLED 3
#define MVX_PUMP_CYCLE 4
#define MVX_PUMP_FAILED 5
/* One whole pump of the solved node `prob` (left untouched; its clone is freed): at most `iters` (1..1000) distance LPs, the
   objective weight alpha (0..1; alpha_k = alpha * 0.9^k, a = 1 - alpha_k, q = alpha_k / ||c0||, 0 for a zero objective).  Per
   LP one step, one objective apply (set_obj_many, else set_obj_coef for the columns whose coefficient differs from
   get_obj_coef) and one solve with the default parameters.  A pump that ends integral is rounded and checked (mvx_bnb_round,
   mode 1).  *found 1 when that point is feasible, *obj / x[1..n] the point, *lps / *pivots the LPs solved and their pivots.
   Uses the table's batched entries where it has them (pump_obj_many, set_obj_many, simplex_batch, round_many) and the twins
   otherwise.  Returns 0; -1 bad arguments; -2 the table lacks an accessor, or can not change an objective; -3 the handle is
   not MVX_OPT.  mvx_branchAndBound returns -1 (*res empty) for pump outside 0..1000, a negative pump_freq, pump_alpha outside
   [0, 1] and pump > 0 with reference_quirks = 1 or best_window > 0, and -2, with the tree so far, when a pump could not be
   carried out */
int mvx_bnb_pump(const mvx_lp_api *api, const void *prob, const void *root, int iters, double alpha, double *obj, int *found, double *x,
                 long long *lps, long long *pivots, int *end);

/* Root cut rounds (DESIGN.md "Root cut rounds"), host twin of mvx_cut_scores through the table (get_col_prim, get_num_cols,
   get_status): dot[t] = sum_j vals[t][j] * x_j and gram[t*k + s] = sum_j vals[t][j] * vals[s][j] over ascending j = 1..n from
   +0.0, product and sum rounded separately.  Returns 0; -1 bad arguments or a handle that is not MVX_OPT */
int mvx_bnb_cut_scores(const mvx_lp_api *api, const void *prob, int k, const double *vals, double *dot, double *gram);
/* The selection of one round, from numbers only: the k cuts are walked by efficacy descending (ties to the lower index) and cut
   t is taken when gram[t][s] <= maxpar * (sqrt(gram[t][t]) * sqrt(gram[s][s])) for every cut s already taken, until K are
   taken or `budget` are.  taken[0 .. *ntaken - 1] the indices in taken order (room for min(k, K) entries).  Returns 0; -1 bad
   arguments (k < 0, K < 1, maxpar outside (0, 1], budget < 0, a null) */
int mvx_bnb_cut_select(int k, const double *eff, const double *gram, int K, double maxpar, int budget, int *taken, int *ntaken);
/* The whole loop on the handle `prob`, which is edited in place: solved with the default parameters, then up to `rounds`
   (1..64) rounds of candidates, scores, selection, append and re-solve with at most K (0: 32) cuts a round and the parallelism
   limit maxpar (0.0: 0.9); the row budget is max(64, rows of `prob` at entry).  Uses gmi_cuts, cut_scores and add_cut_rows
   where the table has them, mvx_generateCutGMI, the twins and the per-row appends otherwise.  counters[0..4] = rounds, cuts
   made, rows appended, LPs solved, their pivots; bounds[0..1] = the LP before the loop and after it.  Returns 0; -1 bad
   arguments; -2 the table lacks an accessor, or a call of the table failed.  mvx_branchAndBound returns -1 (*res empty) for
   cut_rounds outside 0..64, cut_round_max outside 0..4096, cut_maxpar outside (0, 1] other than 0.0, cut_families outside
   0..3, cut_purge outside 0..64 (all four read only with cut_rounds > 0) and cut_rounds > 0 with reference_quirks = 1, and -2, with the unsolved root as the tree, when the loop could not be carried out */
int mvx_bnb_cut_loop(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, long long *counters, double *bounds);
/* The same loop with the cut families chosen (bits: 1 GMI, 2 clique; 0 means 1; outside 0..3: -1): counters[0..7] = the five of
   mvx_bnb_cut_loop, then the edges of the conflict graph, the cliques the separation kept, the clique rows appended.
   mvx_bnb_cut_loop is this function with families = 1.  With bit 2 the graph is computed once at entry from `prob` as it is
   handed in (conflict_graph of the table, the twin without it or on -5; any other failure ends the loop with -2) */
int mvx_bnb_cut_loop_families(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, int families, long long *counters,
                              double *bounds);
/* The same loop with the age limit of the purge (DESIGN.md "Cut purging (cut_purge)"; 0: no purge; outside 0..64: -1): after the
   re-solve of a round that ended MVX_OPT, every live row of the loop whose auxiliary is basic ages by one and every other one
   starts again at 0; the rows that have reached `purge` leave in one del_rows call of the table (without it, or when it fails,
   each becomes a free row), and one more solve follows whose pivots are counted and whose LP is not.  The row budget counts live
   rows.  counters[0..9] = the eight of mvx_bnb_cut_loop_families, then the rows purged and the live rows left.
   mvx_bnb_cut_loop_families is this function with purge = 0 */
int mvx_bnb_cut_loop_purge(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, int families, int purge,
                           long long *counters, double *bounds);

/* The age step of the tree's purge (DESIGN.md "Cut purging in the tree (node_purge)") from numbers only: age[0..k) are the ages
   of a node's rows behind the caller's rows, ascending by row, basic[t] is 1 when row t's auxiliary variable is MVX_BS at the
   node.  A row whose age is 255 is dead (a free row) and is skipped; every other age goes up by one, saturating at 254, when
   the row is basic and becomes 0 otherwise.  out[0..*nout) receives the positions whose age has reached A, ascending.
   Returns 0; -1 for k < 0, A outside 1..64 or a null pointer (age, basic and out may be null when k = 0).  mvx_branchAndBound
   returns -1 (*res empty) for node_purge outside 0..64 and for node_purge > 0 with reference_quirks = 1 or best_window > 0,
   and -2 with the tree so far when a purge could not be carried out on any path */
int mvx_bnb_purge_ages(int k, const int *basic, int A, unsigned char *age, int *out, int *nout);

/* Clique cuts (DESIGN.md "Clique cuts (cut_families)"), host twin of mvx_conflict_graph through the table only (get_mat_row, row
   and column bounds, get_col_kind): the same (n+1) x W words and edge count for the handle `model`, which need not be solved and
   is not changed.  Returns 0; -1 bad arguments; -2 the table lacks an accessor it needs */
int mvx_bnb_conflict_graph(const mvx_lp_api *api, const void *model, unsigned long long *adj, long long *edges);
/* The separation, from numbers only: adj as above for n columns, x[1..n] the LP point.  The columns with a non-empty row of adj
   are ordered by x descending (ties to the lower column); every one of them with x_j > 1e-6 is a seed, in that order.  A seed's
   clique Q starts as {seed} with mask = adj[seed]; the whole order is walked, a column whose bit is set in mask joins Q and mask
   &= adj[column] (zero-valued columns too: Q is maximal).  Q is kept when (sum of x_j over Q, ascending j from +0.0) - 1 > 1e-6
   and no earlier seed gave the same set.  Kept clique t fills row t of vals (n + 1 entries, the layout of mvx_gmi_cuts) with -1
   on Q and 0 elsewhere and rhs[t] = -1: the MVX_LO row sum_{j in Q} x_j <= 1.  Stops at max_cuts; *count the rows written.
   Returns 0; -1 bad arguments (n < 0, max_cuts < 0, a null) */
int mvx_bnb_clique_cuts(int n, const unsigned long long *adj, const double *x, int max_cuts, double *vals, double *rhs, int *count);
/* Clique cuts in the tree (DESIGN.md "Clique cuts in the tree (node_cliques)"), host twin of mvx_clique_cuts_many for one solved
   handle: the separation above against the column values of `prob` (get_col_prim_all / get_col_prim) and the graph adj of n
   columns.  *cnt the cliques kept, q[c*W + w] the member set of clique c in the word layout of adj (W = ceil((n+1)/64)), sum[c]
   its s; the slots from *cnt to max_cuts are zero.  Works through the table only; the handle is not changed.  Returns 0; -1 bad
   arguments (a null, max_cuts outside 1..64, another column count); -2 the table lacks an accessor it needs; -3 the handle is
   not MVX_OPT.  mvx_branchAndBound returns -1 (*res empty) for node_cliques outside 0..64 and for node_cliques > 0 with
   reference_quirks = 1 or best_window > 0, and -2, with the tree so far, when the graph or a separation could not be computed */
int mvx_bnb_clique_masks(const mvx_lp_api *api, const void *prob, int n, const unsigned long long *adj, int max_cuts, int *cnt,
                         unsigned long long *q, double *sum);

/* Incumbent polishing (DESIGN.md "Incumbent polishing (polish)"), host twin of mvx_polish_many for one point x[1..n] (x[0] is not
   touched), edited in place, against the model of `root`: its rows, bounds, kinds, objective and sense.  *ok 0: the point is
   refused (an integer column farther than 1e-9 from an integer, or the rounding heuristic's check fails) and stays as it is,
   *obj = 0, *moves = 0; 1: x the polished point, *obj its objective, *moves the moves taken (at most max_moves, 1..100000).
   Works through the table only (get_mat_row, row and column bounds, get_obj_coef, get_col_kind, get_obj_dir).  Returns 0; -1 bad
   arguments; -2 the table lacks an accessor it needs.  mvx_branchAndBound returns -1 (*res empty) for polish outside 0..100000
   and polish > 0 with reference_quirks = 1, and -2, with the tree so far, when a point could not be polished (polish_many failed
   with a code other than -5, or the twin cannot run) */
int mvx_bnb_polish(const mvx_lp_api *api, const void *root, double *x, int max_moves, double *obj, int *moves, int *ok);

/* bs.cpp:249-258 on one solved node `a` that is about to be branched: generate its GMI cut(s) and append the
   row(s) (cut_strat / reference_quirks / lazy_pool / cut_select / cut_chance of `params`).  Returns the number
   of rows appended.  The pool here holds this node's cuts only; -1 = bug-compatible mode and the node generated
   no cut, where bs.cpp would re-add the last cut pooled by an earlier node (cut.cpp:16-21) --
   a branched node has a fractional, hence basic, integer column and therefore always generates one */
int mvx_bnb_node_cuts(const mvx_lp_api *api, void *a, const mvx_bnb_params *params);

/* ---- callers and data formats either side of the path ---- */
/* glp_read_lp(prob, NULL, fname) util.cpp:284 -- CPLEX LP format; 0 on success */
int mvx_read_lp(mvx_prob *P, const void *parm, const char *fname);
/* glp_read_mps(prob, GLP_MPS_FILE, NULL, fname) util.cpp:290 -- free/fixed MPS; 0 on success */
int mvx_read_mps(mvx_prob *P, int fmt, const void *parm, const char *fname);
/* the B&B event stream of IPCDispatch::write (message.cpp:32-191), one text line per event in the
   format of message.h:141-226, to `path` (NULL = stdout) instead of a ZeroMQ socket; the first field
   (timeSpan) is the event's sequence number so that two runs can be diffed */
int mvx_bnb_write_events(const mvx_bnb_result *res, const char *path);
/* the tree report of bs.cpp:329-343 (PrettyPrintTree, tree_print.h:12-22) */
int mvx_bnb_print_tree(const mvx_bnb_result *res, const char *path);
/* the solution line of bs.cpp:176-191; returns 0, or the needed capacity when `cap` is too small */
int mvx_bnb_solution_string(const mvx_lp_api *api, const void *root, const mvx_bnb_result *res, char *buf, int cap);

#ifdef __cplusplus
}
#endif
#endif
