// engine.hpp -- interface between the C ABI layer (capi.cpp) and the device engine.
#pragma once
#include "mvx_internal.hpp"

namespace mvx {

int device_count();
int set_device(int dev);
void sync_stream();
int take_last_error(); // MVX_ENOMEM ... since the last call; clears it
int bind_thread();

// solve (glp_simplex)
int engine_simplex(mvx_prob *P, const mvx_smcp *parm);
int engine_simplex_batch(mvx_prob **probs, int count, const mvx_smcp *parm, int *rcs);

// tableau maintenance under model edits; all no-ops while !P->valid
void engine_apply_bounds(mvx_prob *P, int k, int type, double old_lb, double old_ub, double lb, double ub);
void engine_add_rows(mvx_prob *P, int first, int nrs); // P->m already updated
// model rows `rows` (ascending, old numbers) are gone, P->m already updated, the mirrors still those of m_old rows; also drops
// the device copies of the model that covered one of them (that part runs without a tableau)
void engine_del_rows(mvx_prob *P, const std::vector<int> &rows, int m_old);
// the same for `count` distinct handles (rows[t] not empty, m_old[t] handle t's row count before): one k_delrows_many launch
void engine_del_rows_many(mvx_prob *const *Ps, int count, const std::vector<int> *rows, const int *m_old);
void engine_row_from_model(mvx_prob *P, int i);      // row i's auxiliary is basic: rebuild its tableau row
void engine_recompute_cost_row(mvx_prob *P);
void engine_invalidate(mvx_prob *P); // drop device state; next solve starts from the slack basis

void engine_copy(mvx_prob *dst, const mvx_prob *src); // device-to-device clone of the slab
void release_device(mvx_prob *P);

// host mirrors of beta / reduced costs / basis (cheap when already fresh)
void refresh_solution(const mvx_prob *P);
int engine_get_tableau(const mvx_prob *P, double *out);
int engine_get_row(const mvx_prob *P, int row, double *out); // out[0..n]

// GMI cuts of a solved node on the device (gmi.cpp:11-117); see engine.cpp
int engine_gmi_cuts(const mvx_prob *P, int mode, const int *cols, int count, double *vals, double *rhs, int *ok);
int engine_gmi_cuts_many(const mvx_prob *const *Ps, int mode, const int *cols, int count, double *vals, double *rhs, int *ok);

// printInfo (util.cpp:414-473) of `count` solved handles in one launch (k_classify); see engine.cpp
int engine_classify_many(const mvx_prob *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol, int cap);
// one-step dual penalties of the candidate columns of `count` solved handles in one launch (k_penalty); see engine.cpp
int engine_penalties_many(const mvx_prob *const *Ps, int count, const int *cols, const int *col_off, double tol, double *pen_down,
                          double *pen_up, int *arg_down, int *arg_up);
// sensitivity ranges of one solved handle: val (m+n+1) x 6, var (m+n+1) x 4 (k_rangecols, k_rangefin, k_rangerows); see engine.cpp
int engine_ranges(const mvx_prob *P, double tol, double *val, int *var);
// KKT check of `count` solved handles over root's rows (k_kkt_vals, k_kkt_rows, k_kkt_cols, k_kkt_fin); see engine.cpp
int engine_kkt_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind, double *r_pe, double *r_de);
// Farkas proof of `count` handles over root's rows (k_farkas_rows .. k_farkas_fin); y (nullable): handle 0's row weights; see engine.cpp
int engine_farkas_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind, double *y);
// the ray that proves a handle unbounded, checked on its own model (k_ray_cols .. k_ray_fin); d (nullable) by variable; see engine.cpp
int engine_ray(const mvx_prob *P, double *val, int *ind, double *d);
// primal rounding heuristic on `count` solved handles against root's model, one launch (k_round); see engine.cpp
int engine_round_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int mode, double *obj, int *found, double *x);
// the diving heuristic's branching pick for `count` (solved handle, rule) pairs against root's model, one launch (k_divepick)
int engine_dive_pick_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir,
                          double *val);
// the whole objective of `count` handles replaced, rows 0 rebuilt in one launch (k_objrow); the feasibility pump's rounding and
// distance objective for `count` solved handles against root's model, one launch (k_pumpobj); see engine.cpp
int engine_set_obj_many(mvx_prob *const *Ps, int count, const double *c);
int engine_pump_obj_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const double *xprev, const int *has_prev,
                         const double *ab, int *info, double *xt, double *c);
// a round of candidate cuts scored against a solved handle in one launch (k_cutgram: dot products with the column values x and
// the Gram matrix), and `k` dense MVX_LO rows appended in one device pass (k_cutrows); see engine.cpp
int engine_cut_scores(const mvx_prob *P, int k, const double *vals, const double *x, double *dot, double *gram);
int engine_add_cut_rows(mvx_prob *P, int k, const double *vals, const double *rhs);
int engine_add_cut_rows_many(mvx_prob *const *Ps, int count, const int *off, const double *vals, const double *rhs);
// `k` dense structural columns appended to the live tableau in one device pass (k_addcols; P->n already updated, flag / lb / ub
// the new positions' statuses and normalised bounds), and the same images without appending; see engine.cpp
// With a pool S the columns are its columns idx[0..k) and their coefficients reach the tableau from the pool's device copy
int engine_add_cols_live(mvx_prob *P, int k, const double *cols, const double *obj, const int *flag, const double *lb, const double *ub,
                         const mvx_colpool *S = nullptr, const int *idx = nullptr);
// sifting over a device-resident column pool (DESIGN.md "Sifting (sift)"): the pool's device copy, the full-pool pricing pass
// with its top-K selection (k_pooly, k_poolprice, k_poolsel_*); see engine.cpp
int engine_pool_sync(const mvx_colpool *S);
void engine_pool_release(mvx_colpool *S);
int engine_pool_price(const mvx_prob *P, const mvx_colpool *S, const unsigned char *skip, int K, double sgn, double tol, double *dj, int *pick,
                      int *npick);
int engine_price_cols(const mvx_prob *P, int k, const double *cols, const double *obj, double *dj, double *img);
// model columns `cols` (ascending, old numbers; lb / ub their normalised bounds) have left the model: where every one of them is
// non-basic they leave the live tableau in one device pass (k_delcols), otherwise the tableau is given up; see engine.cpp
int engine_del_cols(mvx_prob *P, const std::vector<int> &cols, int n_old, const double *lb, const double *ub);
int engine_conflict_graph(const mvx_prob *R, unsigned long long *adj, long long *edges);
// the clique separation of `count` solved handles against root's conflict graph, one launch (k_cliquesep); see engine.cpp
int engine_clique_cuts_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q,
                            double *sum);
// incumbent polishing of `count` points against root's model (k_lsact, k_lsmove, k_lsapply); see engine.cpp
int engine_polish_many(const mvx_prob *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok);
// reduced-cost bound tightening of `count` solved handles, one launch (k_rcfix), and the bound lists of many handles applied
// with one launch (k_setbnds, entries on non-basic positions only); see engine.cpp
int engine_rc_tighten_many(const mvx_prob *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb,
                           double *ub);
int engine_tighten_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);
// node bound propagation of `count` handles over root's rows, one launch for all rounds (k_prop), and general bound lists of
// many handles applied with one launch (k_setbnds)
int engine_propagate_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_rounds, int *infeasible, int *rounds, int *cnt,
                          int *cols, double *lb, double *ub);
int engine_set_bounds_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub);

long long engine_pack_size(const mvx_prob *P, int m_base);
int engine_pack(const mvx_prob *P, int m_base, void *dev_buf);
int engine_unpack(mvx_prob *dst, const void *dev_buf);
void *engine_image_alloc(size_t bytes);
void engine_image_free(void *p);
void tuning(int tr, int hot, int nt);
void set_stall_limit(int limit);
int fcs_debug_stamps(unsigned long long *out);
void set_persist(int mode);
void set_chain(int len);
void set_cluster(int on);
void cluster_stats(long long *launches, long long *aborts);
void set_dual_chain(int len);
void set_dual_fused(int mode);
void dual_fused_stats(long long *boots, long long *pivots);
void set_refresh(int check_every, double tol);
double row_residual(const mvx_prob *P);
void persist_stats(long long *launches, long long *aborts);
void persist_cycles(unsigned long long *out5);
void set_batch_slots(int k);
void profile_enable(int on);
void profile_reset();
double profile_update_ms();
long long profile_update_launches();

} // namespace mvx
