// mvx_internal.hpp -- host-side model + device control block of the MI355X LP engine.
//
// Layout in HBM (one slab per problem handle, see DESIGN.md "Data layout"):
//   T      (m_cap+1) x ld doubles, row-major, ld a multiple of 32 doubles (256 B rows)
//          T[0][0] objective, T[0][j] reduced costs, T[i][0] basic values, T[i][j] body
//   bvar/blb/bub   per tableau row   (basic variable, its bounds)
//   nvar/nflag/nlb/nub per tableau column (non-basic variable, status, bounds)
// Everything position-indexed so that every kernel access is contiguous.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/mvx.h"
#include "sift_host.hpp"

struct DevMatrix;
namespace mvx {

constexpr int ROWCOMB_CHUNK = 64; // rows per partial sum of k_rowcomb (fixed summation order)
constexpr int LD_ALIGN = 32;      // doubles; 256-byte rows
constexpr int ROW_SLACK = 64;     // spare tableau rows per handle for cut appends (cut.cpp:23)
constexpr double DEGEN_TOL = 1e-9; // a step / dual ratio no longer than this counts as degenerate (oracle: DEGEN_TOL)
constexpr double PERT_EPS = 1e-6; // relative size of the anti-stalling bound perturbation (oracle: PERT_EPS)
constexpr size_t NT_THRESHOLD_BYTES = (size_t)320 << 20; // tableaux larger than this stream with non-temporal access (pick_nt)
constexpr size_t WT_MIN_BYTES = (size_t)96 << 20, WT_MAX_BYTES = (size_t)272 << 20; // write-through stores in this band (pick_nt)
constexpr int KCH = 32;          // most steps one bulk launch of the chained primal path applies (chosen by k_pc / k_pr or k_chain, applied by k_fbc3)
constexpr int DCH_MAX = 8;  // most dual pivots one k_update applies (dual_chain)
constexpr int DA_THREADS = 1024; // k_dboot / k_da workgroup size: the O(m) leaving-row pass is redundant per block
constexpr int MAX_EDITS = 8;      // pending bound edits a control block carries (more are flushed by launches)
constexpr int ROW_SPARE = 32;     // rows behind row m that always exist: k_fb streams whole row tiles

// state-machine phases (device-driven; mirrors orc_simplex's round loop)
enum : int { PH_START = 0, PH_PRIMAL2 = 1, PH_DUAL = 2, PH_PHASE1 = 3 };
// done codes
enum : int { D_RUN = 0, D_OPT = 1, D_UNBND = 2, D_NOFEAS = 3, D_ITLIM = 4, D_PFEAS = 5, D_FAIL = 6, D_NEED_PHASE1 = 7 };
// step kinds
enum : int { ST_NONE = 0, ST_PIVOT = 1, ST_FLIP = 2, ST_STOP = 3 };
// fused primal fast path state
enum : int { F_OFF = 0, F_RUN = 1, F_STOP = 2, F_RUN_DUAL = 3 };

// reduction candidate: (k1, k2, idx) is a strict total order, aux rides along
struct Cand {
  double k1, k2;
  int idx, aux;
};


// Device-resident control block.  Kernels take only a pointer to it, so one launch
// sequence serves every problem handle and pivots can be queued ahead of the host.
struct Ctl {
  // geometry + pointers (written by the host before a solve)
  double *T;
  int *bvar; double *blb; double *bub;
  int *nvar; int *nflag; double *nlb; double *nub;
  double *colq;   // [m_cap+1] copy of the pivot column (old values)
  double *srow;   // [ld]      pivot row / pivot
  double *cost1;  // [ld]      phase-1 cost row
  double *wts;    // [m_cap+1] row weights for k_rowcomb
  int *gflag;     // [m_cap+1] phase-1 infeasibility signs
  double *part;   // [nchunks x ld] partial sums of k_rowcomb
  double *rc_base; // [ld] base vector for k_rowcomb (nullable)
  double *rc_out;  // destination of k_rowcomb
  int m, n, ld, m_cap;
  // parameters
  double sgn, tol_bnd, tol_dj, tol_piv;
  // running state
  int phase, done, rounds, budget;
  int it_cnt, n_flips, n_bland;
  int step, p, q, sdir, p_up, leave_flag;
  double piv, bound, xq, delta;
  // fused primal fast path (k_fboot / k_fa / k_fb): ping-pong buffers indexed by parity
  double *colqx[2]; // [m_cap+1] contiguous copy of the NEXT pivot column, exported by k_fb
  double *betac[2]; // [m_cap+1] contiguous copy of column 0 (basic values), exported by k_fb
  Cand *pp[2];      // [npb] pricing partials (one per k_fa block)
  Cand *rp;         // [nrb] ratio-test partials (one per k_fb row block)
  int npb, nrb;
  int fstate, curA, curB, flipflag;
  // anti-cycling (oracle: ctl_t.stall): consecutive degenerate pivots; from stall_limit on every choice
  // follows Bland's smallest-subscript rule until a pivot moves again
  int stall, stall_limit;
  // bound perturbation against stalling (oracle: perturb_basis / restore_bounds): original bounds by
  // variable number, saved when the perturbation is applied
  double *olb, *oub;
  int perturbed, pert_used, n_pert;
  // primal phase 1: the infeasibility-sum cost row lives in tableau row m+1 (first spare row) and is carried
  // through the pivots by k_update; k_p1_head lists the rows whose sign changed (p1_list / wts), k_p1_fix adds them
  int *p1_list;
  int p1_init, p1_nchg, p1_fix_q, p1_fix_g;
  double *pw[2]; // [ld] primal devex reference weights by non-basic position (oracle: ctl_t.pw); the current set
                 // is pw[curA]: the fused path writes the other one and k_fb flips curA, the generic path updates in place
  double *dw; // [m_cap+1] dual devex reference weights by row (oracle: dual_simplex's w), reset on entering the dual phase
  int stall_new; // fused path: k_fa's verdict on the step it prepared, committed by k_fb (k_fa workgroups read `stall`)
  double ent_lb, ent_ub;
  // bound edits of basic variables made since the last solve (glp_set_col_bnds on a branching child, bs.cpp:274,282;
  // glp_set_row_bnds on a fresh cut row, cut.cpp:43): applied by the first k_select of the solve instead of one
  // launch per edit
  int n_edits, edit_row[MAX_EDITS];
  double edit_lb[MAX_EDITS], edit_ub[MAX_EDITS];
  int job; // batched solve: which job of the queue this slot is working on (-1: none)
  // fused dual path (k_dboot / k_da / k_fb<DUAL>): dual devex weights in two sets (the current one is dwx[curA & 1];
  // the generic path updates it in place, k_da writes the other and k_fb flips curA), and the leaving row of the
  // NEXT pivot, chosen by k_da from column 0 before the bulk update (ping-pong like the other fused buffers)
  double *dwx[2];
  int p_nextx[2], p_up_nextx[2];
  int npbd; // number of dual-ratio partials (k_da blocks of DA_THREADS columns)
  // Chained primal path (k_fcc / k_fcr / k_fbc): the pivots after the one k_fa prepared are chosen from O(m + n) slices of the
  // tableau as it stands -- column q_k and row p_k, carried through the earlier pivots of the chain entry by entry --
  // and ONE bulk launch applies the whole chain (each entry read and written once for up to KCH pivots).  Step 0 of a
  // chain is the step k_fa left in the fields above; ch_*[l] describes step l >= 1 (index 0 is filled for uniform loops).
  int chain_max, nch; // chain length allowed by the host (1 = off) / prepared for the coming bulk launch
  int dchain_max;     // the same for the dual steps of the generic path (dual_chain in k_select)
  int n_bulk;         // bulk launches that stepped so far in this solve (one per pivot or flip; one per chain)
  int ch_alive, ch_nrpc; // the chain may still grow / ratio-test partials k_fcc left
  int ch_p[KCH], ch_q[KCH], ch_pup[KCH], ch_lf[KCH], ch_stall[KCH], ch_sdir[KCH], ch_fq[KCH];
  double ch_piv[KCH], ch_bound[KCH], ch_xq[KCH], ch_s0[KCH], ch_dq[KCH], ch_wq[KCH];
  Cand *rpc; // [ceil(m_cap / 256)] ratio-test partials of k_fcc
  double ch_elb[KCH], ch_eub[KCH]; // bounds of the entering variable (become row p's)
  double ch_llb[KCH], ch_lub[KCH]; // bounds of the leaving variable (become column q's)
  double *srowk[KCH], *colqk[KCH]; // scaled pivot row / pivot column of step l
  // Chained primal path (k_pboot / k_pc / k_pr / k_fbc3): what the device decides about the pending chain
  int pc_n;        // steps recorded in the pending chain (k_fbc3 applies them; the next selection starts from 0)
  int pc_epoch;    // chains applied so far + 1
  unsigned pc_arrive; // unused: the first tile block of k_fbc3 commits the chain's bookkeeping, no arrival is counted
  int ch_kind[KCH], ch_cnt[KCH], ch_ok[KCH]; // ST_PIVOT / ST_FLIP; pivots among steps 0..l; == pc_epoch once step l is recorded
  int ch_okc[KCH];  // == pc_epoch once k_pc has chosen step l's entering column
  int hd_q[KCH], hd_sdir[KCH], hd_fq[KCH]; // the entering column of step l as k_pc found it: column, direction, status,
  double hd_dq[KCH], hd_wq[KCH], hd_lbq[KCH], hd_ubq[KCH]; // reduced cost, weight, bounds
  double ch_delta[KCH]; // bound flips: the entering variable's move
  int pc_itlim;         // k_chain: the pivot limit is reached once the pending chain is applied and an entering column is still
                        // on offer: the generic step that closes the batch reports it without pricing again
  int dsel;             // k_dsel has prepared the coming step (a dual phase carrying on): the k_select that follows returns at once
  int cl_abort;         // k_chain gave up waiting for its peer workgroups: the chain was dropped, nothing was changed
  unsigned long long *dbg; // diagnostic phase stamps of k_pc / k_pr / k_chain (MVX_FCS_DBG=1), nullptr otherwise
  int n_dboot, n_dfused;   // fused dual path, this call: times k_dboot started a run / pivots k_fb<DUAL> committed (mvx_dual_fused_stats)
};

// What the host needs after a solve, packed into one staging area:
//   [Ctl][beta (m_cap+1) f64][d (ld) f64][bvar (m_cap+1) i32][nvar (ld) i32][nflag (ld) i32]
// with the handle's own m_cap and ld.  pack_mirrors (k_export, a queue slot of k_select) writes through this view, the
// host reads through it (publish_mirrors); nothing else knows the layout.
struct StageView {
  double *beta, *dj;
  int *bvar, *nvar, *nflag;
  __host__ __device__ StageView(unsigned char *base, int m_cap, int ld) {
    beta = reinterpret_cast<double *>(base + sizeof(Ctl));
    dj = beta + (m_cap + 1);
    bvar = reinterpret_cast<int *>(dj + ld);
    nvar = bvar + (m_cap + 1);
    nflag = nvar + ld;
  }
  static size_t bytes(int m_cap, int ld) { // of one staging area, rounded up to 256
    return (sizeof(Ctl) + (size_t)(m_cap + 1) * (8 + 4) + (size_t)ld * (8 + 4 + 4) + 255) / 256 * 256;
  }
};

// What the kernels of the chained primal path (k_pboot / k_pc / k_pr / k_fbc3) need that the host knows -- pointers,
// geometry, tolerances: passed by value, so that no dependent load stands between a launch and its data; what the
// device decides -- the chain, the counters, the verdicts -- stays in the control block.
// State that a step changes is kept in two sets that alternate with the step index (a launch never writes what a
// workgroup of the same launch may still read); the chain starts from the handle's own arrays ("base").
struct ChainArgs {
  Ctl *c;
  double *T;
  double *blb, *bub, *nlb, *nub; // base: the handle's own arrays (the bulk launch's commit brings them up to date)
  int *nflag;
  double *pw[2];                 // base weights: both sets hold them between chains (the generic step reads pw[curA & 1])
  double *betab;                 // base basic values: column 0, exported contiguously by k_pboot / k_fbc3
  // column side, as of step g in set g & 1: objective row, devex weights, statuses and bounds of the non-basic variables
  double *drowk[2], *pwk[2], *nlbk[2], *nubk[2];
  int *nflagk[2];
  // row side, as of step g in set g & 1: basic values and bounds of the basic variables
  double *betak[2], *blbk[2], *bubk[2];
  double *pp; // pricing partials of k_pr / k_pboot: 8 fields x ppstride (score, q, sdir, d_q, w_q, lb_q, ub_q, flag_q)
  double *rp; // ratio-test partials of k_pc: 4 fields x rpstride (step, |a|, row, to_upper)
  size_t ppstride, rpstride;
  double *srow0, *colq0; // scaled pivot rows / pivot columns of the chain's steps, `sstride` / `cstride` doubles apart
  size_t sstride, cstride;
  int m, n, ld, mcap1, ncb, nrb; // ncb column blocks (k_pr), nrb row blocks (k_pc)
  double tol_dj, tol_piv, tol_bnd, sgn;
  int stall_limit;
  const double *zeros; // max(ld, m_cap + 1) zeros: the operands of a bound flip, and of what fills the chain's last group of steps, in the bulk pass
  // one-XCD cluster selection (k_chain): exchange area, tags, participants, steps this launch may take
  unsigned *xg;
  int xg_bytes;
  unsigned tagbase;
  int nw, kmax;
  int boot; // first chain launch of a batch: k_chain does what k_pboot does for k_pc / k_pr (feasibility of the start, fresh weights)
  int *xabort;
};

// Work queue of a batched solve (mvx_simplex_batch): the host uploads one control block per handle (`jobs`), the slots
// of the launch pull them -- a slot whose solve has ended exports its mirrors into the job's staging area and takes the
// next job in the very launch that finds it idle, instead of idling until the host's next synchronisation point.
struct SlotScratch { // per-slot scratch the pulled control block is pointed at
  double *colq, *srow, *olb, *oub, *dw, *pw;
  double *chain; // DCH_MAX - 1 x (pivot column [m_cap+1 rounded], scaled pivot row [ld]) for dual chains
  size_t chain_col, chain_stride; // bytes: offset of the row part inside one step's pair, size of a pair
};
struct BatchQueue {
  const Ctl *jobs;
  const SlotScratch *scratch;
  int *counters; // [0] next job to hand out, [1] jobs finished and exported, [2] rounds (k_select launches) so far, [3] round of the last job's end
  unsigned char *stage;
  size_t stage_stride;
  int count;
};

// one launch of k_copy_many: up to COPY_BATCH byte ranges (16-byte aligned, sizes multiples of 16)
constexpr int COPY_BATCH = 32;
struct CopyJob {
  const void *src;
  void *dst;
  size_t bytes;
};
struct CopyBatch {
  int count;
  CopyJob jobs[COPY_BATCH];
};

// Where a solved handle's tableau and basis live on the device: the common part of every node-entry descriptor (node_ref
// fills it from the handle; node_col_values in node_kernels.hip walks it)
struct NodeRef {
  const double *T; // tableau
  const int *bvar, *nvar, *nflag;
  const double *nlb, *nub;
  int m, ld; // rows of this handle (cut rows included), its row stride
};

// A handle's slab as a kernel that edits it reads or writes it: the tableau with its row stride, the per-row arrays
// (m_cap + 1 entries) and the per-position arrays (ld entries).  slab_view (engine.cpp) fills it from the handle,
// slab_view_at from a raw slab and its geometry; a kernel that moves a handle to another slab takes two of them
struct SlabView {
  double *T;
  int *bvar;
  double *blb, *bub;
  int *nvar, *nflag;
  double *nlb, *nub;
  int ld;
};

// one cut of a GMI launch: the solved handle it is taken from (a round of a B&B window takes one cut from each of up to
// 64 node LPs: same columns and same first m0 model rows, their own tableaux, bases and appended cut rows)
struct GmiNode : NodeRef {
  int pos, pad; // the tableau row of the cut's basic column
};

// arguments of the GMI cut kernels (k_gmi_work / k_gmi_backsub): `count` cuts, each with its node
struct GmiArgs {
  const GmiNode *nodes; // [count]
  const int *kind;     // [n+1] column kinds of the model (MVX_CV / MVX_IV), device copy
  double *work;        // [count][wld] coefficients by variable number 0..m+n (gmi.cpp:29-32 `work`)
  double *rhs;         // [count]
  int *ok;             // [count] 0 = no valid cut (repaired mode: free non-basic with a non-zero entry)
  const double *A;     // [m0+1][lda] model rows 1..m0: packed non-zeros (bug-compatible) or by column (repaired)
  const int *len;      // [m0+1] non-zeros per row (nullptr: every row dense)
  double *out;         // [count][old] cut coefficients by structural column 1..n after rows 1..m0
  int n, wld, lda, m0, old, count, mode; // mode 0 bug-compatible (gmi.cpp:41-89), 1 repaired
};

// one handle of a classification launch (k_classify, mvx_classify_many)
struct ClsNode : NodeRef {
  int status, pad; // its solve status (MVX_OPT, MVX_NOFEAS, ...)
};

// arguments of k_classify: `count` handles with the same n columns, objective and column kinds
struct ClsArgs {
  const ClsNode *nodes; // [count]
  const double *c;      // [n+1] objective coefficients (util.cpp:437)
  const int *kind;      // [n+1] column kinds (MVX_CV / MVX_IV)
  double *x;            // [count][n+1] scratch: structural values by column
  int *st, *nv;         // [count] printInfo status (-1 / 0 / 1), violated columns
  int *viol;            // [count][cap] violated columns, ascending
  double *xv;           // [count][cap] their values
  int n, cap, quirks, count;
};

// one (handle, candidate) of a penalty launch (k_penalty, mvx_branch_penalties_many): the handle, and the tableau row the
// candidate column is basic in (found by the host from its bvar mirror)
struct PenNode : NodeRef {
  int row, n; // the candidate's tableau row, the non-basic positions
};

// arguments of k_penalty: `count` (handle, candidate) pairs, one workgroup each
struct PenArgs {
  const PenNode *nodes; // [count]
  double *pen_down, *pen_up; // [count]
  int *arg_down, *arg_up;    // [count] arg-min non-basic position of each side (0 when the side is +inf)
  double tol;                // |T[i][q]| must exceed it
  int count, pad;
};

// arguments of k_rangecols / k_rangefin / k_rangerows (mvx_ranges, DESIGN.md "Sensitivity ranges (ranges)"): one solved handle,
// the bounds of its basic variables, the partial records of the column-wise ratio test and the two result tables
constexpr int RANGE_CHUNK = 256; // tableau rows one k_rangecols workgroup walks: m <= RANGE_CHUNK is one chunk
struct RangeArgs {
  NodeRef nd;
  const double *blb, *bub; // [m+1] bounds of the basic variables, +-inf when absent
  double *pt;              // [2][nchunks][n+1] partial minima of part A: side 0 down, side 1 up
  int *pi;                 // [2][nchunks][n+1] their tableau rows (0x7fffffff: none)
  double *val;             // [m+n+1][6] ACT_DN, ACT_UP, OBJ_DN, OBJ_UP, COST_DN, COST_UP
  int *var;                // [m+n+1][4] LIM_DN, LIM_UP, ENT_DN, ENT_UP
  double tol;              // |T[i][q]| must exceed it
  int n, nchunks, maxdir, pad; // maxdir: 1 under MVX_MAX
};

// one handle of a KKT launch (k_kkt_vals / k_kkt_rows / k_kkt_cols / k_kkt_fin; mvx_kkt_many, DESIGN.md "KKT check (kkt)"): the
// handle, the bounds of its basic variables, where its cut rows (rows m0+1..m, dense, n + 1 doubles each) and its own objective
// lie in the call's upload, and where its slice of the by-variable arrays starts (m + n + 1 entries, entry 0 unused)
struct KktNode : NodeRef {
  const double *blb, *bub; // [m+1]
  const double *cuts;      // [m - m0][n+1], nullptr when m == m0
  const double *c;         // [n+1] the handle's objective where it differs from the root's, else nullptr
  size_t voff;
  double sg;               // +1 minimise, -1 maximise
};

// arguments of the KKT kernels: `count` handles over the model of one root in both orientations (k_prop's copies).  The
// by-variable arrays hold one slice per handle (KktNode::voff): x / du / lo / up / st the value, dual, bounds and status of
// variable k, res the residuals (row i at i, column j at m + j), term[c] the ae (2c) and re (2c + 1) of condition c = PE, PB,
// DE, DB by row, variable, column, variable
#define KKT_WAVES 4 // waves of a k_kkt_rows / k_kkt_cols workgroup: a row (a column) each
struct KktArgs {
  const KktNode *nodes; // [count]
  const double *At;     // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j
  const double *Ar;     // [m0][ldn]: Ar[i*ldn + j] = a_(i+1),j
  const double *c0;     // [n+1] the root's objective
  double *x, *du, *lo, *up, *res;
  int *st;
  double *term[8];
  double *val; // [count][8]
  int *ind;    // [count][8]
  int n, m0, ldm, ldn, count, mmax; // mmax: the most rows of a handle
};

// one handle of a Farkas launch (k_farkas_rows / k_farkas_pick / k_farkas_vars / k_farkas_cols / k_farkas_fin; mvx_farkas_many,
// DESIGN.md "Infeasibility and unboundedness proofs (farkas)"): the handle, the bounds of its basic variables, its cut rows in the
// call's upload, where its slice of the by-variable arrays (m + n + 1 entries, entry 0 unused) and of the row records (two per
// tableau row) start
struct FkNode : NodeRef {
  const double *blb, *bub; // [m+1]
  const double *cuts;      // [m - m0][n+1], nullptr when m == m0
  size_t voff, roff;
};

// arguments of the Farkas kernels: `count` handles over the columns of one root's model (k_prop's copy At).  rrel holds rel of the
// lower and of the upper side of every tableau row; f the picked row's form by variable, g the model's form (y, -w), lo / up the
// bounds by variable, dterm the de terms by column (at m + j)
#define FARKAS_WAVES 4 // waves of a k_farkas_rows / k_farkas_cols workgroup: a tableau row (a column) each
#define FARKAS_Z 1e-9   // the zero rule: a coefficient this small on a variable without the bound it needs is dropped
#define FARKAS_REL 1e-9 // a side proves when its rel exceeds this
struct FkArgs {
  const FkNode *nodes; // [count]
  const double *At;    // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j
  double *rrel;
  double *f, *g, *lo, *up, *dterm;
  int *pick;   // [count]: 2 (i - 1) + side - 1 of the candidate, -1 without one
  double *val; // [count][4]
  int *ind;    // [count][4]
  int n, m0, ldm, count, mmax; // mmax: the most rows of a handle
};

// arguments of the ray kernels (k_ray_cols / k_ray_pick / k_ray_vars / k_ray_rows / k_ray_fin; mvx_ray, same section of DESIGN.md):
// one handle against its own rows by row (k_prop's copy Ar) and its objective, which goes up with the call.  open[q] holds the
// direction (+1 / -1) in which position q gives a ray the tableau does not stop, 0 where it gives none; d / lo / up are by variable
// (m + n + 1 entries), rae / rre the rows' ae and re terms
#define RAY_TOL 1e-9 // the published dual must improve by more than this
struct RayArgs {
  NodeRef nd;
  const double *blb, *bub; // [m+1]
  const double *Ar;        // [m][ldn]: Ar[i*ldn + j] = a_(i+1),j
  const double *c;         // [n+1]
  int *open;               // [n+1]
  int *pick;               // [1]: the position, 0 without one
  double *d, *lo, *up, *rae, *rre;
  double *val; // [4]
  int *ind;    // [6]
  double sg;   // +1 minimise, -1 maximise
  int n, ldn;
};

// one handle of a rounding launch (k_round, mvx_round_many)
using RndNode = NodeRef;

// the tree's model for k_round, uploaded once per root (engine_round_many): rows 1..m0 by column, their bounds, the root's
// column bounds, the objective and per-column flags (RND_INT integer, RND_DLOCK / RND_ULOCK a row locks it down / up)
#define RND_INT 1
#define RND_DLOCK 2
#define RND_ULOCK 4
#define RND_NMAX 4096 // columns a k_round workgroup holds in LDS (values and the fill order)
#define RND_RPT 4     // rows per thread k_round's fill keeps in registers (up to RND_RPT * 256 rows; beyond, LDS / scratch)
struct RndArgs {
  const RndNode *nodes;           // [count]
  const double *At;               // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j, rows 0..m0-1
  const double *rlo, *rhi;        // [m0] row bounds, +-inf when absent
  const double *clo, *chi, *c;    // [n+1] root column bounds (+-inf when absent), objective (c[0] the constant)
  const int *flags;               // [n+1] RND_* bits
  double *scratch;                // [count][m0] row activities when m0 > RND_NMAX (else LDS), nullptr otherwise
  double *obj;                    // [count]
  int *found;                     // [count]
  double *x;                      // [count][n+1] the candidates
  double sg;                      // +1 maximise, -1 minimise: the fill's direction sign(sg * c_j)
  int n, m0, ldm, mode, count, pad;
};

// one handle of a reduced-cost tightening launch (k_rcfix, mvx_rc_tighten_many): it reads row 0 of the tableau (reduced costs
// by non-basic position; position q holds structural column nvar[q] - m) and the non-basic arrays; gap2 = sg*z - sg*cutoff
// plus the slack, computed by the host from the handle's objective mirror
struct RcNode : NodeRef {
  double gap2;
};

// arguments of k_rcfix: `count` handles with the same n columns and kinds.  Results by non-basic position (every position
// is written exactly once): code 0 no change, 1 the upper bound becomes val, 2 the lower bound becomes val
struct RcArgs {
  const RcNode *nodes; // [count]
  const int *kind;     // [n+1] column kinds (MVX_CV / MVX_IV)
  int *code;           // [count][n+1]
  double *val;         // [count][n+1]
  double tol;
  int n, count;
};

// arguments of k_prop (mvx_propagate_many): `count` handles over the model of one root -- its rows by column (At, k_round's
// copy) and by row (Ar), the row bounds and the RND_INT flags -- each with its own column bounds.  A handle's final bounds are
// written once per column; the host compares them with what it sent.
struct PropArgs {
  const double *At;        // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j
  const double *Ar;        // [m0][ldn]: Ar[i*ldn + j] = a_(i+1),j
  const double *rlo, *rhi; // [m0] row bounds, +-inf when absent
  const int *flags;        // [n+1] RND_INT: the column is integer
  const double *lb0, *ub0; // [count][n+1] the handles' column bounds, +-inf when absent
  double *lb, *ub;         // [count][n+1] the propagated bounds
  int *info;               // [count][2]: infeasible, rounds run
  double *act;             // [count][2][m0] row activities when m0 > RND_NMAX (else LDS), nullptr otherwise
  int *actk;               // [count][m0] their counts of infinite terms, likewise
  int n, m0, ldm, ldn, max_rounds, count;
};

// one (handle, rule) of a diving pick launch (k_divepick, mvx_dive_pick_many): the handle and the rule (1 fractional,
// 2 locks, 4 vector length)
struct DiveNode : NodeRef {
  int rule, pad;
};

// arguments of k_divepick: `count` (handle, rule) pairs over the model of one root (k_round's copy: objective, RND_INT flags,
// and per column the rows that lock it down / up and its non-zeros in rows 1..m0)
struct DiveArgs {
  const DiveNode *nodes;   // [count]
  const double *c;         // [n+1] objective
  const int *flags;        // [n+1] RND_* bits
  const int *dl, *ul, *len; // [n+1]
  int *nfrac, *col, *dir;  // [count] candidates, the picked column (0: none), 0 down / 1 up
  double *val;             // [count] the picked column's value
  double sg;               // +1 maximise, -1 minimise
  int n, count;
};

// one handle of an objective-row launch (k_objrow, mvx_set_obj_many): its tableau, the weights of its rows (the new cost of each
// row's basic variable, 0 for an auxiliary) and the base of its row 0 (base[0] the constant z, base[q] the new cost of the
// variable at non-basic position q), both in the call's upload
struct ObjNode {
  double *T;
  const double *w;    // [m+1]
  const double *base; // [n+1]
  int m, ld;
};
#define OBJ_COLS 64 // columns per k_objrow workgroup (one per lane; its four waves take a row chunk each)

// one handle of a pump-objective launch (k_pumpobj, mvx_pump_obj_many): the handle, the bounds of its basic variables by
// tableau row, its direction, the weights (a, q) of its new objective and whether xprev holds its last rounding
struct PumpNode : NodeRef {
  const double *blb, *bub; // [m+1]
  double sg, a, q;         // +1 maximise / -1 minimise; c_j = a * (-sg * d_j) + (q * sqrt(nnz(d))) * c0_j
  int has_prev, pad;
};
#define PUMP_MOVES 10 // columns a stalled rounding moves

// arguments of k_pumpobj: `count` solved handles over the model of one root (k_round's copy: objective and RND_INT flags)
struct PumpArgs {
  const PumpNode *nodes; // [count]
  const double *c0;      // [n+1] the root's objective
  const int *flags;      // [n+1] RND_* bits
  const double *xprev;   // [count][n+1] the last roundings (read where has_prev is set)
  const double *sq;      // [n+1] sqrt(k), k = 0..n, from the host
  double *v, *lo, *hi;   // [count][n+1] scratch: column values and clamped bounds
  int *info;             // [count][4]: nfrac, moved, stalled, nnz(d)
  double *xt, *c;        // [count][n+1] the rounding and the new objective
  int n, count;
};

// arguments of k_cutgram (mvx_cut_scores): `k` candidate cut rows of n + 1 doubles each (entry 0 unused), the column values of
// the solved handle they are scored on, and where dot[k] and the k x k Gram matrix go
#define GRAM_TILE 16 // a workgroup holds GRAM_TILE x GRAM_TILE pairs (t, s), one per lane
#define GRAM_COLS 64 // columns staged in LDS per pass
struct CutGramArgs {
  const double *vals; // [k][n+1]
  const double *x;    // [n+1] column values by structural column
  double *dot;        // [k]    sum_j v_tj x_j
  double *gram;       // [k][k] sum_j v_tj v_sj
  int k, n;
};

// arguments of k_cutrows (mvx_add_cut_rows): `k` dense rows appended behind row m of one tableau.  Row t (0-based) is
// base_t + W_t . T over rows 1..m, where W_t[i] = vals[t][rowcol[i]] (0 where row i's basic variable is an auxiliary) and
// base_t[q] = vals[t][nbcol[q]] (0 for a non-basic auxiliary), base_t[0] = vals[t][0], which the host has replaced by the row's
// value at the non-basic point.  The kernel also does what k_add_rows does k times: the new rows' basic auxiliaries and bounds,
// and the structural variable numbers moved up by k
#define CUT_TILE 8 // cuts per lane: each T[i][j] is loaded once for that many new rows
struct CutRowsArgs {
  SlabView v;
  const double *vals;  // [k][n+1]
  const int *rowcol;   // [m+1] structural column basic in row i, 0 for an auxiliary
  const int *nbcol;    // [n+1] structural column at non-basic position q, 0 for an auxiliary
  const double *rowlb; // [k] lower bound of new row t on the device (-inf while its edit is still pending on the host)
  const int *extra;    // [k] 1: the t-th single append would have summed a trailing chunk of zero weights (+0.0 added once more)
  int m, n, k;         // m: rows before the append
};

// one handle of k_cutrows_many (mvx_add_cut_rows_many): k_cutrows' arguments with the pieces as byte offsets into the uploaded
// block that holds the descriptors too (n is the same for all handles and an argument of the launch), and the handle's first
// row tile in the launch's flattened tile index
struct CutRowsHandle {
  SlabView v;
  size_t o_vals, o_rowcol, o_nbcol, o_rowlb, o_extra;
  int m, k;  // m: rows before the append
  int tile0; // tiles of the handles in front of this one (CUT_TILE rows each)
  int pad;
};

// arguments of k_addcols (mvx_add_dense_cols, mvx_price_cols; DESIGN.md "Column append (add_cols)"): `k` dense structural columns
// against one tableau.  Image t, tableau row p, is base + S: S sums w_q * T[p][q] over the non-basic positions q = 1..n that hold
// an auxiliary i <= m (w_q = -cols[t][i]), base is obj[t] in row 0 and cols[t][bvar[p]] where row p's basic variable is an
// auxiliary.  Pricing (img or dj set): the images go to img / dj and nothing of a slab is written.  Append: the images become
// columns n+1..n+k of d (== s in place; another slab with its own stride on a relayout, which the launch then writes whole: old
// entries, new columns, zeros), column 0 is shifted by the new columns' resting values xs, and the blocks of row block 0 write the
// new positions' nvar / nflag / nlb / nub (and carry the per-row and per-position arrays over on a relayout)
#define ADDCOLS_CT 4      // columns per tile: accumulators a lane holds per row
#define ADDCOLS_RW 1      // rows a wave owns
#define ADDCOLS_WAVES 8   // waves per workgroup: ADDCOLS_WAVES * ADDCOLS_RW rows share one gather of the weights
#define ADDCOLS_CHUNK 512 // non-basic positions whose weights one gather stages in LDS: one per thread
struct AddColsArgs {
  SlabView s; // the tableau as it stands; of its arrays pricing and the in-place append read bvar and nvar only
  SlabView d; // append: the destination (s again in place); pricing: all null
  const double *cols;     // [ceil(k / ADDCOLS_CT)][m+1][ADDCOLS_CT]: the columns of a tile side by side, so that the weights of a
                          // position are one 32-byte read; zero behind column k
  const double *obj;      // [k]
  const double *xs;       // [k] resting values of the new columns (append)
  const int *nflag_new;   // [k] their statuses (append)
  const double *nlb_new, *nub_new; // [k] their bounds, +-inf when absent (append)
  double *img, *dj;       // pricing: [k][m+1] (nullable) and [k]
  int m, n, k;
  int rows;     // tableau rows 0..rows-1 get images (m + 1; 1 when only dj is wanted)
  int rows_all; // rows the launch covers: rows, or m_cap + 1 on a relayout
};

// arguments of the sifting kernels (mvx_pool_price, mvx_pool_append; DESIGN.md "Sifting (sift)") over a device-resident column pool:
// column j = 1..N at cols[(j-1)*ldp ..], model row i at entry i-1, zero behind row m (ldp a multiple of 64 doubles).
// k_pooly writes the row weights y (ypos[i] the non-basic position of auxiliary i, 0 when it is basic: y_i = +0.0; zero up to
// ldp), k_poolprice the reduced costs d[1..N] and the selection keys (the bits of |d_j| where column j is attractive and not
// skipped, else 0), k_poolsel_hist one digit of the radix select over (key, N - j), k_poolsel_emit the columns at or above the
// K-th largest, k_poolsel_rank their order
#define POOL_WAVES 4       // waves of a k_poolprice workgroup: a pool column each
#define POOL_Y_LDS 4096    // most rows whose weights a k_poolprice workgroup keeps in LDS; beyond, y is read through L2
#define POOL_AHEAD 8       // loads a lane of k_poolprice has in flight
#define POOLSEL_PASSES 12  // 8-bit digits of the 96-bit selection key: 8 of |d_j|'s bits, 4 of N - j
#define POOLSEL_THREADS 256
#define POOLSEL_COUNT (POOLSEL_PASSES * 256)
#define POOLSEL_STATE (POOLSEL_COUNT + 2)
#define POOLSEL_INTS (POOLSEL_STATE + (POOLSEL_PASSES + 1) * 4)
struct PoolPriceArgs {
  const double *cols, *obj; // the pool: [N][ldp], [N]
  const int *flag;          // [N] the status a column would enter with (std_flag of its type)
  const unsigned char *skip; // [N+1] nullable
  const double *T0;         // row 0 of the handle's tableau
  const int *ypos;          // [m+1]
  double *y;                // [ldp]
  double *d;                // [N+1]
  unsigned long long *key;  // [N+1]
  int *sel;                 // [POOLSEL_INTS], zero before the first pass: POOLSEL_PASSES histograms of 256 bins, then the candidates
                            // emitted so far and the number of picks, then per pass the digits chosen so far and the rank
                            // still to find (4 ints)
  unsigned long long *cand_key; // [K]
  int *cand_j;              // [K]
  int *pick;                // [1 + K]: pick[0] the number of picks, then the picks
  double sgn, tol;
  int m, ldp, N, K;         // K already min(K, N)
};
// arguments of k_poolgather: pool columns idx[0..k) into the tile layout k_addcols reads (AddColsArgs::cols)
struct PoolGatherArgs {
  const double *cols; // the pool
  const int *idx;     // [k] 1-based pool columns
  double *tiles;      // [ceil(k / ADDCOLS_CT)][m+1][ADDCOLS_CT]
  int m, ldp, k;
};

// arguments of k_delrows (mvx_del_rows): rows taken out of one tableau in place.  Tableau rows 0..first-1 stay where they are;
// destination row first + t takes source row src[t] (ascending, src[t] > first + t); rows first + nmove .. m_old (behind the new
// row m = first + nmove - 1) are vacated and zeroed.  del[0..nrs) are the deleted auxiliary variables (= model rows), ascending, for the renumbering
#define DEL_BATCH 8 // source rows a lane holds in registers before it stores them
struct DelRowsArgs {
  SlabView v;
  const int *src; // [nmove]
  const int *del; // [nrs]
  int first, nmove, m_old, nrs, n; // k_delrows_many: nrs = 0 marks a handle the launch leaves alone
};

// arguments of k_delcols (mvx_del_cols; DESIGN.md "Column deletion (del_cols)"): non-basic columns taken out of one tableau.
// Positions 1..first-1 stay where they are; destination position first + t takes source position src[t] (ascending,
// src[t] > first + t), t < nmove, so that the last kept position is n_new = first + nmove - 1; positions n_new+1 .. n_old are
// vacated.  Before any entry of a row moves, its column 0 takes the chain T[p][0] = fma(T[p][sh_pos[s]], sh_negx[s], T[p][0]),
// s = 0 .. nsh-1 (the deleted positions with a non-zero resting value, ascending; sh_negx the negated value), rows 0..m only.
// d == s: in place, rows 0..rows_all-1 are compacted and their vacated positions zeroed.  d != s (another slab, its own
// stride): the launch writes rows 0..rows_all-1 of d over the whole stride -- kept entries, zero padding, zero rows behind row
// m -- and carries the per-row and per-position arrays over.  delc[0..ncs) are the deleted columns, ascending, for the
// renumbering of the structural variables: m + j becomes m + j - #{deleted < j}
#define DELC_BATCH 8 // batches of 64 destinations a lane holds in registers before it stores them
#define DELC_WAVES 8 // waves per workgroup: a wave owns one row
struct DelColsArgs {
  SlabView s, d; // source and destination (the same in place)
  const int *src;        // [nmove]
  const int *sh_pos;     // [nsh]
  const double *sh_negx; // [nsh]
  const int *delc;       // [ncs]
  int m, n_old, ncs, first, nmove, nsh;
  int rows_all; // rows the launch covers: m_cap + 1
};

// arguments of k_conflict_rows / k_conflict (mvx_conflict_graph): the model of one handle as k_prop reads it -- its rows by
// column (At) and by row (Ar), the row bounds, the RND_INT flags and the handle's own column bounds -- the per-row numbers the
// first kernel leaves for the second, and the adjacency words
#define CONF_WAVES 4 // waves of a k_conflict workgroup: one column, CONF_WAVES consecutive words of its row
struct ConflictArgs {
  const double *At;        // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j
  const double *Ar;        // [m0][ldn]: Ar[i*ldn + j] = a_(i+1),j; ldn = 64 * W, the padding is zero
  const double *rlo, *rhi; // [m0] row bounds, +-inf when absent
  const double *clo, *chi; // [n+1] the handle's column bounds, +-inf when absent
  const int *flags;        // [n+1] RND_INT: the column is integer
  double *rowinfo;         // [m0][4]: Lmin, the upper side's threshold (+inf: the side says nothing), Lmax, the lower side's (-inf)
  unsigned long long *adj; // [n+1][W]
  int n, m0, ldm, ldn, W, pad;
};

// arguments of k_cliquemembers / k_cliquesep (mvx_clique_cuts_many): the conflict graph of the root, kept on the device with its
// rounding model, the columns that have a neighbour, and `count` solved handles whose column values are separated against it
#define CLQ_WAVES 4 // waves of a k_cliquesep workgroup: one seed each, the next CLQ_WAVES seeds of the order together
#define CLQ_KMAX 64 // most cliques kept per handle
struct CliqueArgs {
  const NodeRef *nodes;          // [count]
  const unsigned long long *adj; // [n+1][W]
  const int *member;             // [n+1] 1: the column's adjacency row is not empty
  int *cnt;                      // [count] cliques kept
  unsigned long long *q;         // [count][max_cuts][W] their member sets; slots from cnt on are not written
  double *sum;                   // [count][max_cuts] their s
  int n, W, max_cuts, count;
};

// arguments of k_lsact / k_lsmove / k_lsapply (mvx_polish_many): the root's model in both orientations, as k_conflict reads it,
// with the objective, and per point its values, row activities, the records of one iteration and its counters
#define LS_GROUP 8 // iterations the host enqueues between two looks at the done flags
struct LsRec {
  double gain;            // the best feasible candidate's gain, 0.0 when there is none
  unsigned long long key; // single: index(u) << 31; pair: 1 << 62 | index(u) << 31 | index(v); ~0 when there is none
};
struct LsArgs {
  const double *At;        // [n+1][ldm]: At[j*ldm + i] = a_(i+1),j
  const double *Ar;        // [m0][ldn]: Ar[i*ldn + j] = a_(i+1),j; ldn = 64 * W, the padding is zero
  const double *rlo, *rhi; // [m0] row bounds, +-inf when absent
  const double *clo, *chi; // [n+1] the root's column bounds, +-inf when absent
  const double *c;         // [n+1] objective, c[0] the constant
  const int *flags;        // [n+1] RND_INT: the column is integer
  const double *xin;       // [count][n+1] the points as handed in
  double *x;               // [count][n+1] the points at work, and the result
  double *r;               // [count][ldm] row activities
  double *obj, *obj0;      // [count] the result's objective; the entry point's
  int *moves, *ok, *done;  // [count]
  LsRec *rec;              // [count][2n] one record per unit move
  double sg;
  int n, m0, ldm, ldn, count, pad;
};

// k_setbnds (mvx_set_col_bnds_many, mvx_tighten_cols_many): per handle a range of bound writes and a range of shifts of column 0
struct SetbHandle {
  double *T, *blb, *bub, *nlb, *nub;
  int *nflag;
  int ld, m;   // row stride and rows of the tableau (cut rows included)
  int e0, e1;  // its entries [e0, e1)
  int s0, s1;  // its shifts [s0, s1), in list order
};
struct SetbEntry {
  double lb, ub;
  int idx, flag; // flag < 0: row idx of a basic variable (blb / bub); else non-basic position idx with that status
};
struct SetbShift {
  double delta; // T[i][0] = fma(T[i][jj], delta, T[i][0]) for every row i = 0..m
  int jj, pad;
};

// Kernel launch wrappers and launch geometry: defined in kernels.hip and node_kernels.hip (the node-entry kernels), called by
// engine.cpp.  Declared here, where both sides see them, so that a drifted signature does not compile.
void set_tuning(int tr, int hot, int nt);
int fused_npb(int n);
int fused_nrb_max(int m);
int chain_ncb(int n);
int chain_nrb(int m);
void launch_pboot(const ChainArgs &, hipStream_t);
void launch_pstep(const ChainArgs &, int g, hipStream_t);
void launch_pc(const ChainArgs &, int g, hipStream_t);
void launch_fbc3(const ChainArgs &, int steps, hipStream_t);
int launch_chain(const ChainArgs &, hipStream_t);
int chain_cluster_nw(int m, int n);
int chain_cluster_kmax(int m, int n);
void launch_dboot(Ctl *, int n, hipStream_t);
void launch_da(Ctl *, int n, hipStream_t);
void launch_db(Ctl *, int m, int n, hipStream_t);
void launch_select(Ctl *, hipStream_t, int slots = 1);
int launch_dsel(Ctl *, int m, int n, hipStream_t, int slots = 1);
void launch_select_queue(Ctl *, const BatchQueue &q, hipStream_t, int slots);
void launch_update(Ctl *, int m, int n, hipStream_t, int slots = 1, int chained = 0, int busy_slots = 0);
void launch_p1_head(Ctl *, hipStream_t);
void launch_p1_select(Ctl *, hipStream_t);
void launch_p1_fix(Ctl *, int n, hipStream_t);
void launch_scatter_ctl(Ctl *dst, const Ctl *src, const int *idx, int count, hipStream_t);
void launch_copy_many(const CopyBatch &b, hipStream_t);
void launch_gmi(const GmiArgs &a, hipStream_t);
void launch_classify(const ClsArgs &a, hipStream_t);
void launch_penalty(const PenArgs &a, hipStream_t);
void launch_ranges(const RangeArgs &a, hipStream_t);
void launch_kkt(const KktArgs &a, hipStream_t);
void launch_farkas(const FkArgs &a, hipStream_t);
void launch_ray(const RayArgs &a, hipStream_t);
void launch_round(const RndArgs &a, hipStream_t);
void launch_rcfix(const RcArgs &a, hipStream_t);
void launch_prop(const PropArgs &a, hipStream_t);
void launch_divepick(const DiveArgs &a, hipStream_t);
void launch_objrow(const ObjNode *nodes, int n, int count, hipStream_t);
void launch_pumpobj(const PumpArgs &a, hipStream_t);
void launch_cutgram(const CutGramArgs &a, hipStream_t);
void launch_cutrows(const CutRowsArgs &a, hipStream_t);
// hs, tile0s (the handles' first tiles, ascending) and base (what the descriptors' offsets count from): device memory;
// the launch covers tiles [tile_base, tile_base + ntiles) of the flattened index, ntiles <= 65535
void launch_cutrows_many(const CutRowsHandle *hs, const int *tile0s, int handles, const unsigned char *base, int n, int tile_base, int ntiles,
                         hipStream_t);
void launch_addcols(const AddColsArgs &a, hipStream_t);
void launch_delcols(const DelColsArgs &a, hipStream_t);
void launch_pool_price(const PoolPriceArgs &a, hipStream_t); // k_pooly, k_poolprice and, for a.K > 0, the selection
void launch_pool_gather(const PoolGatherArgs &a, hipStream_t);
void launch_delrows(const DelRowsArgs &a, hipStream_t);
void launch_delrows_many(const DelRowsArgs *hs, int handles, int max_ld, hipStream_t); // hs: device memory

void launch_conflict(const ConflictArgs &a, hipStream_t);
void launch_clique_members(const unsigned long long *adj, int *member, int n, int W, hipStream_t);
void launch_cliquesep(const CliqueArgs &a, hipStream_t);
void launch_lsact(const LsArgs &a, int final, hipStream_t);
void launch_lsiter(const LsArgs &a, hipStream_t);
void launch_setbnds(const SetbHandle *hs, const SetbEntry *es, const SetbShift *ss, int handles, hipStream_t);
void launch_refresh_select(Ctl *, const int *tflag, int var, hipStream_t);
size_t persist_lds_bytes(int m, int cpw);
int persist_max_cpw();
int persist_slot_words(int m_cap);
int launch_persist(Ctl *, unsigned long long *head, unsigned long long *slot, int *abort_flag, unsigned long long *dbg, int m, int cpw, int nw,
                   int slot_stride, int max_steps, int head_stride, hipStream_t);
void launch_rowcomb(Ctl *, int m, int n, int respect_done, hipStream_t);
void launch_shift_nonbasic(double *T, int ld, int m, int jj, double delta, hipStream_t);
void launch_set_basic_bounds(double *blb, double *bub, int i, double lb, double ub, hipStream_t);
void launch_set_nonbasic(double *nlb, double *nub, int *nflag, int j, double lb, double ub, int flag, hipStream_t);
void launch_add_rows(double *T, int ld, int n, int *bvar, double *blb, double *bub, int *nvar, int first, int nrs, int m_new,
                     hipStream_t);
void launch_export(Ctl *, unsigned char *stage, int m, int n, int force, hipStream_t, int slots = 1, size_t slot_stride = 0);

// shared immutable matrix row (1-based, n+1 doubles)
using RowPtr = std::shared_ptr<std::vector<double>>;

// A vector a clone shares with its source until one of them writes: B&B clones copy a handle thousands of times a second
// and never touch the row list (a cut appends to it: that node's list parts from its siblings' then) or the names.
// Reads go through operator[] / get(); every write goes through mut(), which parts from the sharers first.
template <class T>
class CowVec {
  std::shared_ptr<std::vector<T>> p_ = std::make_shared<std::vector<T>>();

public:
  const T &operator[](size_t i) const { return (*p_)[i]; }
  size_t size() const { return p_->size(); }
  bool empty() const { return p_->empty(); }
  const std::vector<T> &get() const { return *p_; }
  std::vector<T> &mut() {
    if (p_.use_count() != 1) p_ = std::make_shared<std::vector<T>>(*p_);
    return *p_;
  }
};

// The rows of a model: a frozen head shared by every clone (one reference count) and this handle's own tail.  B&B clones
// copy a handle thousands of times a second; what a node adds to its parent's model is a cut row or two, which goes to
// the tail -- a clone costs one count plus the tail, an append touches nothing shared.  (A plain shared list of 513 row
// pointers cost 513 counts per clone; a copy-on-write list moved the same cost to every node's first cut.)  freeze()
// folds the tail into a new head; the solve entry calls it when the tail has grown long (a freshly loaded model).
class RowList {
  std::shared_ptr<std::vector<RowPtr>> head_ = std::make_shared<std::vector<RowPtr>>();
  std::vector<RowPtr> tail_;

public:
  size_t size() const { return head_->size() + tail_.size(); }
  const RowPtr &operator[](size_t i) const { return i < head_->size() ? (*head_)[i] : tail_[i - head_->size()]; }
  size_t tail_size() const { return tail_.size(); }
  void push_back(RowPtr r) { tail_.push_back(std::move(r)); }
  void set(size_t i, RowPtr r) {
    if (i >= head_->size()) {
      tail_[i - head_->size()] = std::move(r);
      return;
    }
    if (head_.use_count() != 1) head_ = std::make_shared<std::vector<RowPtr>>(*head_);
    (*head_)[i] = std::move(r);
  }
  void resize(size_t n) {
    if (n >= head_->size()) {
      tail_.resize(n - head_->size());
      return;
    }
    if (head_.use_count() != 1) head_ = std::make_shared<std::vector<RowPtr>>(head_->begin(), head_->begin() + (long)n);
    else head_->resize(n);
    tail_.clear();
  }
  // the entries idx (ascending, distinct) leave, the others keep their order.  Entries of the tail (cut rows) leave the tail
  // alone; one in the head gives this handle a head of its own, and the sharers keep theirs
  void erase(const std::vector<size_t> &idx) {
    const size_t nh = head_->size();
    size_t in_head = 0;
    while (in_head < idx.size() && idx[in_head] < nh) in_head++;
    if (in_head > 0) {
      auto h = std::make_shared<std::vector<RowPtr>>();
      h->reserve(nh - in_head);
      for (size_t i = 0, d = 0; i < nh; i++) {
        if (d < in_head && idx[d] == i) d++;
        else h->push_back((*head_)[i]);
      }
      head_ = std::move(h);
    }
    size_t w = 0;
    for (size_t i = 0, d = in_head; i < tail_.size(); i++) {
      if (d < idx.size() && idx[d] == nh + i) d++;
      else {
        if (w != i) tail_[w] = std::move(tail_[i]);
        w++;
      }
    }
    tail_.resize(w);
  }
  void reset(size_t n) { // n empty rows
    head_ = std::make_shared<std::vector<RowPtr>>();
    tail_.assign(n, RowPtr());
  }
  void freeze() {
    if (tail_.empty()) return;
    auto h = std::make_shared<std::vector<RowPtr>>();
    h->reserve(size());
    h->insert(h->end(), head_->begin(), head_->end());
    h->insert(h->end(), tail_.begin(), tail_.end());
    head_ = std::move(h);
    tail_.clear();
  }
};

} // namespace mvx

// A column pool (mvx_pool_create; DESIGN.md "Sifting (sift)"): the host copy, and the device copy of its first dev_n columns, made
// by the first call that needs the device (engine_pool_sync) and released by engine_pool_release
struct mvx_colpool {
  mvx_sifting::PoolHost h;
  mutable double *d_cols = nullptr, *d_obj = nullptr;
  mutable int *d_flag = nullptr;
  mutable int dev_n = 0, dev_cap = 0;
};

struct mvx_prob {
  // ---- model (host) ----
  int m = 0, n = 0;
  int dir = MVX_MIN;
  mvx::RowList A; // A[i], i=1..m; rows are shared between clones (copy-on-write), and so is the list's frozen head
  std::vector<double> c;      // c[0..n]
  std::vector<int> kind;      // kind[1..n]
  mvx::CowVec<std::string> cname;
  std::vector<int> rtype;
  std::vector<double> rlb, rub; // normalised (+-inf when absent)
  std::vector<int> ctype;
  std::vector<double> clb, cub;
  // ---- engine state ----
  bool valid = false;   // device tableau + basis exist
  int status = MVX_UNDEF;
  int it_cnt = 0;
  int pert_cnt = 0;  // bound perturbations applied against stalling, diagnostic
  int bland_cnt = 0; // pivots chosen under the anti-cycling (Bland) rule, diagnostic
  double last_ms = 0.0;
  double last_tol[3] = {0.0, 0.0, 0.0}; // tolerances of the solve that produced `status`
  int piv_since_check = 0; // pivots since the residual of the row equations was last looked at (clones inherit it)
  int refresh_cnt = 0;     // tableau refreshes, diagnostic
  bool hint_dual = false; // last edit made a basic variable infeasible: start in the dual simplex
  // bound edits of basic variables not yet on the device: (row position, lb, ub); the next solve's control block carries them
  struct Edit {
    int row;
    double lb, ub;
  };
  std::vector<Edit> pending;
  // device copy of model rows 1..m0 for the GMI back-substitution (gmi.cpp:81-89), shared by every clone whose first
  // m0 rows are the same objects (B&B nodes share their root's rows); built on first use
  std::shared_ptr<struct DevMatrix> dmat;
  // device copy of this handle's model as the root of a rounding-heuristic tree (mvx_round_many): rows 1..m by column,
  // bounds, objective, lock flags; not passed on by copy_prob, checked against the model before every use
  mutable std::shared_ptr<struct RoundModel> rmod;
  // host mirrors of the basis (always in sync while valid)
  std::vector<int> bvar, nvar, nflag; // [m+1], [n+1], [n+1]
  std::vector<int> pos;               // pos[k], k=1..m+n: +row or -column
  // cached solution vectors (refreshed by export after each solve / modification)
  mutable bool sol_fresh = false;
  // while !sol_fresh: rows 0..fresh_rows of `beta` (and all of `dj`) are still the tableau's -- the only edits since
  // the last export appended rows behind them or rewrote a row behind them (a cut: cut.cpp:40) -- so reading the value
  // of a variable that is basic in one of those rows needs no device export (-1: nothing is known to be current)
  mutable int fresh_rows = -1;
  mutable std::vector<double> beta; // [m+1], beta[0] = objective
  mutable std::vector<double> dj;   // [n+1]
  // ---- device slab ----
  void *slab = nullptr;
  size_t slab_bytes = 0;
  int m_cap = 0, ld = 0;
  double *d_T = nullptr;
  int *d_bvar = nullptr; double *d_blb = nullptr; double *d_bub = nullptr;
  int *d_nvar = nullptr; int *d_nflag = nullptr; double *d_nlb = nullptr; double *d_nub = nullptr;
};
