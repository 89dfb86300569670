// node_kernels.hip -- gfx950 kernels of the batched node entries of branch and bound (engine.cpp: engine_*_many): GMI cuts,
// classification, branching penalties, sensitivity ranges, the rounding heuristic, reduced-cost tightening, bound propagation, bound lists, the
// diving pick, objective replacement, the feasibility pump's step, the scores and the batched append of a cut round, the clique separation of a window, the KKT check, the Farkas proof, the unbounded ray, and the append, pricing and deletion of columns.  Each takes its arguments by value and the handles it works on as an array of descriptors (NodeRef and what
// the kernel needs beyond it, mvx_internal.hpp).  Same flags as kernels.hip: -ffp-contract=off, so every kernel has the bits
// of its host twin.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_common.hpp"

namespace mvx {

// The value of every structural column of a handle, f(j, value) once per column j = 1..n: column 0 of its tableau row when it
// is basic, else the bound its status names -- what get_col_prim reads out of the host mirrors.  A selection, no arithmetic,
// so the bits are the host's.  One workgroup of 256 threads; which thread meets which column is not specified.
template <class F>
__device__ __forceinline__ void node_col_values(const NodeRef &nd, int n, F f) {
  const int m = nd.m;
  for (int i = 1 + TIDX; i <= m; i += 256) {
    const int k = nd.bvar[i];
    if (k > m && k <= m + n) f(k - m, nd.T[(size_t)i * (size_t)nd.ld]);
  }
  for (int q = 1 + TIDX; q <= n; q += 256) {
    const int k = nd.nvar[q];
    if (k > m && k <= m + n) f(k - m, dev_nb_value(nd.nflag[q], nd.nlb[q], nd.nub[q]));
  }
}

// ======================================================================= GMI cuts on the device
// generateCut3 (/root/reference/gmi.cpp:11-117) and its repaired variant, for `count` basic integer columns of one
// solved node at once.  k_gmi_work turns the tableau row of each column into the coefficient vector `work` by
// variable number (gmi.cpp:41-74): the bug-compatible formula threads a RUNNING right-hand side through the
// non-basic columns in ascending position order (gmi.cpp:55,73), so one lane walks the row; everything around
// it (row loads, bound / kind look-ups, the repaired formula's per-column terms) is done by the whole workgroup.
// k_gmi_backsub is gmi.cpp:81-89: out[col] = work[m+col] + sum over model rows i = 1..m0, in that order, of
// work[i] * A[i][col] -- multiply and add rounded separately, as the host loop does (-ffp-contract=off).
// The caller finishes rows m0+1..m (the node's own appended cut rows) on the host, in the same order.
__device__ __forceinline__ double dev_fract(double x) { // util.cpp:11-23
  double ip;
  double f = modf(x, &ip);
  if (f < 0.0) f += 1;
  return f;
}
__device__ __forceinline__ double api_ub(double ub) { return ub == INFINITY ? 1.79769313486231570815e+308 : ub; }
__device__ __forceinline__ double api_lb(double lb) { return lb == -INFINITY ? -1.79769313486231570815e+308 : lb; }

constexpr int GMI_CH = 1024; // non-basic positions staged per pass

__global__ __launch_bounds__(256) void k_gmi_work(GmiArgs a) {
  __shared__ double s_val[GMI_CH], s_aux[GMI_CH];
  __shared__ int s_var[GMI_CH], s_kind[GMI_CH];
  __shared__ double s_rhs, s_temp;
  __shared__ int s_bad;
  const int c = (int)blockIdx.x;
  const GmiNode nd = a.nodes[c];
  const int m = nd.m, n = a.n;
  const double *row = nd.T + (size_t)nd.pos * nd.ld;
  double *work = a.work + (size_t)c * a.wld;
  for (int v = TIDX; v <= m + n; v += 256) work[v] = 0.0;
  const double beta = row[0];
  const double f0 = dev_fract(beta);
  if (TIDX == 0) {
    s_rhs = a.mode == 0 ? beta : 1.0; // gmi.cpp:37 / the repaired cut's right-hand side starts at 1
    s_temp = 0.0;                     // `temp` is uninitialised at gmi.cpp:13; 0 here and in the oracle
    s_bad = 0;
  }
  __syncthreads();
  for (int base = 1; base <= n; base += GMI_CH) {
    const int cnt = (n - base + 1 < GMI_CH) ? n - base + 1 : GMI_CH;
    for (int t = TIDX; t < cnt; t += 256) {
      const int jj = base + t;
      const double val = row[jj];
      const int var = nd.nvar[jj];
      // glp_get_col_kind: an integer column with bounds [0,1] reads as GLP_BV; auxiliaries are continuous
      int kind = MVX_CV;
      const double lb = nd.nlb[jj], ub = nd.nub[jj];
      if (var > m) {
        kind = a.kind[var - m];
        if (kind == MVX_IV && lb == 0.0 && ub == 1.0) kind = MVX_BV;
      }
      s_val[t] = val;
      s_var[t] = var;
      if (a.mode == 0) {
        s_kind[t] = kind;
        s_aux[t] = api_ub(ub); // gmi.cpp:47,52
      } else {
        // repaired: this column's term of the cut and of its right-hand side
        const int stat = nd.nflag[jj];
        int code = 0; // 0 skip, 1 at lower, 2 at upper
        double g = 0.0, term = 0.0;
        if (val != 0.0 && stat != MVX_NS) {
          if (stat == MVX_NF) {
            code = 3;
          } else {
            const double abar = (stat == MVX_NL) ? -val : val;
            if (kind != MVX_CV) {
              const double fj = dev_fract(abar);
              g = (fj <= f0) ? xdiv(fj, f0) : xdiv(1.0 - fj, 1.0 - f0);
            } else {
              g = (abar >= 0.0) ? xdiv(abar, f0) : xdiv(-abar, 1.0 - f0);
            }
            if (stat == MVX_NL) {
              code = 1;
              term = g * api_lb(lb);
            } else {
              code = 2;
              term = -(g * api_ub(ub));
            }
          }
        }
        s_kind[t] = code;
        s_aux[t] = term;
        if (code == 1) work[var] = 0.0 + g;
        if (code == 2) work[var] = 0.0 - g;
      }
    }
    __syncthreads();
    if (TIDX == 0) {
      double rhs = s_rhs;
      if (a.mode == 0) {
        double temp = s_temp;
        for (int t = 0; t < cnt; t++) {
          const double val = s_val[t];
          if (val == 0.0) continue; // glp_eval_tab_row returns the non-zeros only
          const int kind = s_kind[t];
          const double fRhs = dev_fract(rhs); // the RUNNING rhs (gmi.cpp:55,73)
          const double fVal = dev_fract(val);
          if (kind == MVX_IV) temp = (fRhs >= fVal) ? fVal : xdiv(fRhs, 1.0 - fRhs) * (1.0 - fVal);
          if (kind == MVX_CV) temp = (val >= 0.0) ? val : xdiv(fRhs, 1.0 - fRhs) * (-1.0 * val);
          work[s_var[t]] = -1.0 * temp; // gmi.cpp:72
          rhs = rhs - temp * s_aux[t];  // gmi.cpp:73
        }
        s_temp = temp;
      } else {
        int bad = s_bad;
        for (int t = 0; t < cnt; t++) {
          const int code = s_kind[t];
          if (code == 3) bad = 1;
          if (code == 1 || code == 2) rhs = rhs + s_aux[t];
        }
        s_bad = bad;
      }
      s_rhs = rhs;
    }
    __syncthreads();
  }
  if (TIDX == 0) {
    a.rhs[c] = s_rhs;
    a.ok[c] = s_bad ? 0 : 1;
  }
}

constexpr int GMI_CT = 4; // cuts per lane in the back-substitution (each loaded matrix entry serves four cuts)

__global__ __launch_bounds__(256) void k_gmi_backsub(GmiArgs a) {
  __shared__ double s_w[64][GMI_CT];
  const int col = 1 + (int)blockIdx.x * 256 + TIDX;
  const int c0 = (int)blockIdx.y * GMI_CT;
  const bool act = col <= a.n;
  double acc[GMI_CT];
#pragma unroll
  for (int u = 0; u < GMI_CT; u++) acc[u] = (act && c0 + u < a.count) ? a.work[(size_t)(c0 + u) * a.wld + a.nodes[c0 + u].m + col] : 0.0;
  for (int i0 = 1; i0 <= a.m0; i0 += 64) {
    __syncthreads();
    {
      const int r = TIDX >> 2, u = TIDX & 3; // 64 rows x 4 cuts
      const int i = i0 + r;
      s_w[r][u] = (i <= a.m0 && c0 + u < a.count) ? a.work[(size_t)(c0 + u) * a.wld + i] : 0.0;
    }
    __syncthreads();
    const int cnt = (a.m0 - i0 + 1 < 64) ? a.m0 - i0 + 1 : 64;
    if (act) {
      for (int r = 0; r < cnt; r++) {
        const int i = i0 + r;
        const double av = a.A[(size_t)i * a.lda + col];
        if (a.mode == 0) {
          // position `col` of row i's non-zero list (gmi.cpp:87 indexes by position, not by column)
          if (a.len && col > a.len[i]) continue;
#pragma unroll
          for (int u = 0; u < GMI_CT; u++) acc[u] = acc[u] + s_w[r][u] * av;
        } else {
          if (av == 0.0) continue;
#pragma unroll
          for (int u = 0; u < GMI_CT; u++)
            if (s_w[r][u] != 0.0) acc[u] = acc[u] + s_w[r][u] * av;
        }
      }
    }
  }
  if (act) {
#pragma unroll
    for (int u = 0; u < GMI_CT; u++)
      if (c0 + u < a.count) a.out[(size_t)(c0 + u) * a.old + col] = acc[u];
  }
}

void launch_gmi(const GmiArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_gmi_work, dim3((unsigned)a.count), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_gmi_backsub, dim3((unsigned)((a.n + 255) / 256), (unsigned)((a.count + GMI_CT - 1) / GMI_CT)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_classify
// printInfo (util.cpp:414-473) of a batch of solved handles, one workgroup per handle (mvx_classify_many).  The value of
// structural column j is what get_col_prim reads out of the host mirrors: column 0 of its tableau row when it is basic,
// else the bound its status names (dev_nb_value) -- a selection, no arithmetic, so the bits are those of the host.  The
// tests are printInfo's: bug-compatible, x != 0, c_j != 0 and trunc(x) != x (util.cpp:437,443); repaired, a distance
// to the nearest integer above 1e-9; integer columns only.  The violated columns are compacted in ascending order: per
// chunk of 256 columns a ballot in each wave, the waves' counts through LDS, the running base carried across chunks.
__global__ __launch_bounds__(256) void k_classify(ClsArgs a) {
  __shared__ int s_cnt[4];
  const int t = (int)blockIdx.x;
  const ClsNode nd = a.nodes[t];
  const int n = a.n, cap = a.cap;
  const int st = nd.status;
  if (st == MVX_NOFEAS || st == MVX_INFEAS || st == MVX_UNBND) { // util.cpp:423-431
    if (TIDX == 0) {
      a.st[t] = -1;
      a.nv[t] = 0;
    }
    return;
  }
  double *x = a.x + (size_t)t * (size_t)(n + 1);
  node_col_values(nd, n, [&](int j, double v) { x[j] = v; });
  __syncthreads();
  const int lane = TIDX & 63, wv = TIDX >> 6;
  int *viol = a.viol + (size_t)t * (size_t)cap;
  double *xv = a.xv + (size_t)t * (size_t)cap;
  int base = 0;
  for (int j0 = 1; j0 <= n; j0 += 256) {
    const int j = j0 + TIDX;
    bool bad = false;
    double v = 0.0;
    if (j <= n) {
      v = x[j];
      const double tr = fabs(v) < 4503599627370496.0 ? (double)(long long)v : v; // bnb.cpp printInfo's trunc_of
      const bool integer = a.kind[j] != MVX_CV;
      if (a.quirks) {
        bad = v != 0 && a.c[j] != 0 && tr != v && integer;
      } else {
        const double f = fabs(v - tr);
        bad = (f < 1.0 - f ? f : 1.0 - f) > 1e-9 && integer;
      }
    }
    const unsigned long long mask = __ballot(bad);
    if (lane == 0) s_cnt[wv] = __popcll(mask);
    __syncthreads();
    int off = base, tot = 0;
    for (int w = 0; w < 4; w++) {
      if (w < wv) off += s_cnt[w];
      tot += s_cnt[w];
    }
    if (bad) {
      const int o = off + __popcll(mask & ((1ull << lane) - 1ull));
      if (o < cap) {
        viol[o] = j;
        xv[o] = v;
      }
    }
    base += tot;
    __syncthreads(); // s_cnt is written again by the next chunk
  }
  if (TIDX == 0) {
    a.nv[t] = base;
    a.st[t] = base == 0 ? 1 : 0;
  }
}

void launch_classify(const ClsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_classify, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_penalty
// One-step dual penalties of a basic integer column (mvx_branch_penalties_many, DESIGN.md "Branching on the node LP"),
// one workgroup per (handle, candidate).  Row 0 (reduced costs) and the candidate's row i are streamed once, coalesced;
// position q is down-eligible when its variable may move in a direction s that lowers x_j (s * T[i][q] < 0), up-eligible
// when one raises it, and |T[i][q]| > tol; r_q = |T[0][q]| / |T[i][q]| (a true division, xdiv).  Each thread keeps the running
// (r, q) minimum of each side over its strided positions -- q ascending, strict compare, so the lowest q wins a tie -- the
// waves reduce with shuffles, four partials meet in LDS.  min is exact: the result has the host twin's bits.
struct PenMin {
  double r;
  int q;
};
__device__ __forceinline__ PenMin pen_min(PenMin a, PenMin b) { // smaller r; equal r: smaller q (q = INT_MAX: none)
  return (b.r < a.r || (b.r == a.r && b.q < a.q)) ? b : a;
}
__device__ __forceinline__ PenMin pen_wave_min(PenMin v) {
  for (int off = 32; off > 0; off >>= 1) {
    PenMin o;
    o.r = __shfl_xor(v.r, off, 64);
    o.q = __shfl_xor(v.q, off, 64);
    v = pen_min(v, o);
  }
  return v;
}

__global__ __launch_bounds__(256) void k_penalty(PenArgs a) {
  __shared__ double s_r[2][4];
  __shared__ int s_q[2][4];
  const int t = (int)blockIdx.x;
  const PenNode nd = a.nodes[t];
  const double *r0 = nd.T;
  const double *ri = nd.T + (size_t)nd.row * (size_t)nd.ld;
  const double tol = a.tol;
  const double inf = __builtin_huge_val();
  PenMin dn = {inf, 0x7fffffff}, up = {inf, 0x7fffffff};
  for (int q = 1 + TIDX; q <= nd.n; q += 256) {
    const double e = ri[q];
    const double d = r0[q];
    const int f = nd.nflag[q];
    if (!(fabs(e) > tol)) continue;
    const bool inc = f == MVX_NL || f == MVX_NF, dec = f == MVX_NU || f == MVX_NF; // allowed directions s = +1 / -1
    const bool down = (inc && e < 0.0) || (dec && e > 0.0);
    const bool upw = (inc && e > 0.0) || (dec && e < 0.0);
    if (!down && !upw) continue;
    const double r = xdiv(fabs(d), fabs(e)); // the correctly rounded quotient: the host's division
    if (down && r < dn.r) dn = PenMin{r, q};
    if (upw && r < up.r) up = PenMin{r, q};
  }
  dn = pen_wave_min(dn);
  up = pen_wave_min(up);
  const int lane = TIDX & 63, wv = TIDX >> 6;
  if (lane == 0) {
    s_r[0][wv] = dn.r; s_q[0][wv] = dn.q;
    s_r[1][wv] = up.r; s_q[1][wv] = up.q;
  }
  __syncthreads();
  if (TIDX == 0) {
    PenMin bd = {s_r[0][0], s_q[0][0]}, bu = {s_r[1][0], s_q[1][0]};
    for (int w = 1; w < 4; w++) {
      bd = pen_min(bd, PenMin{s_r[0][w], s_q[0][w]});
      bu = pen_min(bu, PenMin{s_r[1][w], s_q[1][w]});
    }
    const double v = ri[0];
    const double fd = v - floor(v), fu = ceil(v) - v;
    const bool hd = bd.q != 0x7fffffff, hu = bu.q != 0x7fffffff;
    a.pen_down[t] = hd ? fd * bd.r : inf;
    a.pen_up[t] = hu ? fu * bu.r : inf;
    a.arg_down[t] = hd ? bd.q : 0;
    a.arg_up[t] = hu ? bu.q : 0;
  }
}

void launch_penalty(const PenArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_penalty, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_rangecols / k_rangefin / k_rangerows
// Sensitivity ranges of a solved LP (mvx_ranges, DESIGN.md "Sensitivity ranges (ranges)").
//
// Part A, activity ranging of the non-basic positions, is a ratio test DOWN every column of the row-major tableau.
// k_rangecols: grid (strips of 64 positions, chunks of RANGE_CHUNK rows), 256 threads.  A lane owns one position, the four
// waves take the rows of the chunk in turn (row i0 + wave, i0 + wave + 4, ...), so a wave's read of a row is 64 consecutive
// doubles and the row's own numbers (basic value, bounds of its basic variable) are the same in every lane.  Per row and
// direction one correctly rounded quotient (xdiv), RANGE_AHEAD rows at a time: their entries are requested together and their
// quotients formed without a branch between them; a lane keeps (t, row) per direction with a strict compare over ascending
// rows; the four waves meet in LDS under the order (t, row) and one record per (chunk, position) goes to scratch.
// k_rangefin: a thread per position takes the chunks in ascending order, strict compare -- the lowest row wins a tie, as in the
// host twin's single walk -- and writes the row of the position's variable in both result tables.
//
// Part B, cost ranging of the basic variables, is k_penalty's test for every tableau row: k_rangerows, one workgroup per row,
// rows 0 and i streamed coalesced, two running (r, q) minima, wave shuffles, four partials through LDS.
//
// min is exact and every quotient and product is rounded once: the tables have the host twin's bits.
constexpr int RANGE_AHEAD = 8; // tableau rows (k_rangecols) / positions (k_rangerows) a thread requests before it uses the first
struct RngMin {
  double t;
  int i;
};
__device__ __forceinline__ RngMin rng_min(RngMin a, RngMin b) { // smaller t; equal t: lower row (0x7fffffff: none)
  return (b.t < a.t || (b.t == a.t && b.i < a.i)) ? b : a;
}

__global__ __launch_bounds__(256) void k_rangecols(RangeArgs a) {
  __shared__ double s_t[2][4][64];
  __shared__ int s_i[2][4][64];
  const int lane = TIDX & 63;
  const int wv = __builtin_amdgcn_readfirstlane(TIDX >> 6);
  const int q = 1 + (int)blockIdx.x * 64 + lane;
  const int m = a.nd.m, ld = a.nd.ld;
  const int i0 = 1 + (int)blockIdx.y * RANGE_CHUNK;
  const int i1 = (i0 + RANGE_CHUNK - 1 < m) ? i0 + RANGE_CHUNK - 1 : m;
  const double inf = __builtin_huge_val();
  const double tol = a.tol;
  RngMin dn = {inf, 0x7fffffff}, up = {inf, 0x7fffffff};
  if (q <= a.n) {
    const double *col = a.nd.T + q;
    // RANGE_AHEAD rows of this wave are requested before the first is used (a row past the chunk reads row i1 and is skipped)
    for (int ib = i0 + wv; ib <= i1; ib += 4 * RANGE_AHEAD) {
      double e[RANGE_AHEAD];
#pragma unroll
      for (int u = 0; u < RANGE_AHEAD; u++) {
        const int i = ib + 4 * u;
        e[u] = col[(size_t)(i <= i1 ? i : i1) * (size_t)ld];
      }
      // the quotients of the RANGE_AHEAD rows do not depend on each other: no branch stands between them, so their division
      // sequences overlap.  A side that does not count divides +inf by 1: +inf never passes the strict compare
      double tu[RANGE_AHEAD], td[RANGE_AHEAD];
#pragma unroll
      for (int u = 0; u < RANGE_AHEAD; u++) {
        const int i = ib + 4 * u, ic = i <= i1 ? i : i1;
        const double beta = a.nd.T[(size_t)ic * (size_t)ld], lb = a.blb[ic], ub = a.bub[ic]; // the same in every lane
        const double su = fmax(ub - beta, 0.0), sl = fmax(beta - lb, 0.0); // room towards the upper / the lower bound
        const bool hu = ub != inf, hl = lb != -inf;
        const double ae = fabs(e[u]);
        const bool counts = i <= i1 && ae > tol;
        const bool pos = e[u] > 0.0;
        // x_k up: the row's basic variable moves towards its upper bound when e > 0, its lower when e < 0; x_k down: the reverse
        const bool oku = counts && (pos ? hu : hl), okd = counts && (pos ? hl : hu);
        const double den = counts ? ae : 1.0;
        tu[u] = xdiv(oku ? (pos ? su : sl) : inf, den);
        td[u] = xdiv(okd ? (pos ? sl : su) : inf, den);
      }
#pragma unroll
      for (int u = 0; u < RANGE_AHEAD; u++) { // ascending rows, strict compare
        const int i = ib + 4 * u;
        if (tu[u] < up.t) up = RngMin{tu[u], i};
        if (td[u] < dn.t) dn = RngMin{td[u], i};
      }
    }
  }
  s_t[0][wv][lane] = dn.t; s_i[0][wv][lane] = dn.i;
  s_t[1][wv][lane] = up.t; s_i[1][wv][lane] = up.i;
  __syncthreads();
  if (TIDX < 128) { // waves 0 and 1: side 0 (down) and side 1 (up) of the 64 positions
    const int side = TIDX >> 6;
    RngMin b = {s_t[side][0][lane], s_i[side][0][lane]};
    for (int w = 1; w < 4; w++) b = rng_min(b, RngMin{s_t[side][w][lane], s_i[side][w][lane]});
    if (q <= a.n) {
      const size_t o = ((size_t)side * (size_t)a.nchunks + blockIdx.y) * (size_t)(a.n + 1) + (size_t)q;
      a.pt[o] = b.t;
      a.pi[o] = b.i;
    }
  }
}

__global__ __launch_bounds__(256) void k_rangefin(RangeArgs a) {
  const int q = 1 + (int)blockIdx.x * 256 + TIDX;
  if (q > a.n) return;
  const double inf = __builtin_huge_val();
  const size_t stride = (size_t)(a.n + 1), side1 = (size_t)a.nchunks * stride;
  RngMin dn = {inf, 0x7fffffff}, up = {inf, 0x7fffffff};
  for (int c = 0; c < a.nchunks; c++) { // ascending chunks hold ascending rows: strict compare keeps the lowest row
    const size_t o = (size_t)c * stride + (size_t)q;
    const double td = a.pt[o], tu = a.pt[side1 + o];
    if (td < dn.t) dn = RngMin{td, a.pi[o]};
    if (tu < up.t) up = RngMin{tu, a.pi[side1 + o]};
  }
  const int k = a.nd.nvar[q], f = a.nd.nflag[q];
  const double d = fabs(a.nd.T[q]);
  // how far c_k may rise / fall: the side the variable rests against, turned round under MIN
  const bool lo = f == MVX_NL || f == MVX_NF, hi = f == MVX_NU || f == MVX_NF;
  const bool cu = a.maxdir ? lo : hi, cd = a.maxdir ? hi : lo;
  const double none = d > 0.0 ? inf : 0.0; // no row limits the move: inf * 0 is never formed
  double *v = a.val + (size_t)k * 6;
  int *w = a.var + (size_t)k * 4;
  v[0] = dn.t;
  v[1] = up.t;
  v[2] = dn.t == inf ? none : d * dn.t;
  v[3] = up.t == inf ? none : d * up.t;
  v[4] = cd ? d : inf;
  v[5] = cu ? d : inf;
  w[0] = dn.i == 0x7fffffff ? 0 : a.nd.bvar[dn.i];
  w[1] = up.i == 0x7fffffff ? 0 : a.nd.bvar[up.i];
  w[2] = 0;
  w[3] = 0;
}

__global__ __launch_bounds__(256) void k_rangerows(RangeArgs a) {
  __shared__ double s_r[2][4];
  __shared__ int s_q[2][4];
  const int i = 1 + (int)blockIdx.x;
  const double *r0 = a.nd.T;
  const double *ri = a.nd.T + (size_t)i * (size_t)a.nd.ld;
  const double tol = a.tol;
  const double inf = __builtin_huge_val();
  PenMin dn = {inf, 0x7fffffff}, up = {inf, 0x7fffffff};
  for (int qb = 1 + TIDX; qb <= a.n; qb += 256 * RANGE_AHEAD) {
    double e[RANGE_AHEAD], d[RANGE_AHEAD];
    int f[RANGE_AHEAD];
#pragma unroll
    for (int u = 0; u < RANGE_AHEAD; u++) { // a position past the row reads position 0 and is skipped
      const int q = qb + 256 * u;
      const int o = q <= a.n ? q : 0;
      e[u] = ri[o];
      d[u] = r0[o];
      f[u] = a.nd.nflag[o];
    }
    // as in k_rangecols: the quotients first, without a branch between them (a position that does not count divides +inf by 1)
    double r[RANGE_AHEAD];
    bool down[RANGE_AHEAD], upw[RANGE_AHEAD];
#pragma unroll
    for (int u = 0; u < RANGE_AHEAD; u++) {
      const int q = qb + 256 * u;
      const bool counts = q <= a.n && fabs(e[u]) > tol;
      const bool inc = f[u] == MVX_NL || f[u] == MVX_NF, dec = f[u] == MVX_NU || f[u] == MVX_NF; // allowed directions s = +1 / -1
      down[u] = counts && ((inc && e[u] < 0.0) || (dec && e[u] > 0.0));
      upw[u] = counts && ((inc && e[u] > 0.0) || (dec && e[u] < 0.0));
      const bool any = down[u] || upw[u];
      r[u] = xdiv(any ? fabs(d[u]) : inf, any ? fabs(e[u]) : 1.0);
    }
#pragma unroll
    for (int u = 0; u < RANGE_AHEAD; u++) { // ascending positions, strict compare
      const int q = qb + 256 * u;
      if (down[u] && r[u] < dn.r) dn = PenMin{r[u], q};
      if (upw[u] && r[u] < up.r) up = PenMin{r[u], q};
    }
  }
  dn = pen_wave_min(dn);
  up = pen_wave_min(up);
  const int lane = TIDX & 63, wv = TIDX >> 6;
  if (lane == 0) {
    s_r[0][wv] = dn.r; s_q[0][wv] = dn.q;
    s_r[1][wv] = up.r; s_q[1][wv] = up.q;
  }
  __syncthreads();
  if (TIDX == 0) {
    PenMin bd = {s_r[0][0], s_q[0][0]}, bu = {s_r[1][0], s_q[1][0]};
    for (int w = 1; w < 4; w++) {
      bd = pen_min(bd, PenMin{s_r[0][w], s_q[0][w]});
      bu = pen_min(bu, PenMin{s_r[1][w], s_q[1][w]});
    }
    const int qd = bd.q == 0x7fffffff ? 0 : a.nd.nvar[bd.q], qu = bu.q == 0x7fffffff ? 0 : a.nd.nvar[bu.q];
    const int k = a.nd.bvar[i];
    double *v = a.val + (size_t)k * 6;
    int *w = a.var + (size_t)k * 4;
    v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0;
    v[4] = a.maxdir ? bd.r : bu.r;
    v[5] = a.maxdir ? bu.r : bd.r;
    w[0] = 0; w[1] = 0;
    w[2] = a.maxdir ? qd : qu;
    w[3] = a.maxdir ? qu : qd;
  }
}

// val / var row 0 is zeroed by the host; every variable 1..m+n is basic in one row or non-basic in one position, so the two
// writers together cover every other row exactly once
void launch_ranges(const RangeArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_rangecols, dim3((unsigned)((a.n + 63) / 64), (unsigned)a.nchunks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_rangefin, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_rangerows, dim3((unsigned)a.nd.m), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_kkt_vals / k_kkt_rows / k_kkt_cols / k_kkt_fin
// KKT check of solved handles against the model (mvx_kkt_many, DESIGN.md "KKT check (kkt)").  Four launches over all handles:
//  1. k_kkt_vals, a thread per (handle, tableau row and non-basic position): value, dual, bounds and status of every variable
//     k = 1..m+n out of the slab -- column 0 and the row bounds where k is basic, the bound its status names, row 0 and the
//     position bounds where it is not: node_col_values' selection, for the auxiliaries too and spread over workgroups -- into
//     the handle's slice of the by-variable arrays.  Selections only: the getters' bits;
//  2. k_kkt_rows, a wave per (handle, row i): s_i = sum_j a_ij xS_j in 64 chains, lane l taking j = l+1, l+65, ... ascending
//     with fma from +0.0 over a coalesced row of Ar (or of the handle's uploaded cut row), the chains combined by the halving
//     tree s[l] += s[l+h], h = 32 .. 1, through __shfl_xor (lanes >= h compute sums nobody reads).  Lane 0 writes r_i, the
//     row's PE terms and the PB and DB terms of auxiliary i;
//  3. k_kkt_cols, a wave per (handle, column j): t_j = sum_i a_ij lambda_i the same way over a column of At and then the cut
//     rows; lane 0 writes r_j, the DE terms and the PB and DB terms of structural j;
//  4. k_kkt_fin, a workgroup per (handle, maximum): a strict compare in ascending index order per thread, combined with
//     "larger wins, equal goes to the lower index" -- exact, so the order of the combination is free.
// No atomics, no LDS beyond k_kkt_fin's wave partials, nothing waits on another workgroup.  Quotients are correctly rounded (xdiv).
__global__ __launch_bounds__(256) void k_kkt_vals(KktArgs a) {
  const KktNode nd = a.nodes[blockIdx.y];
  const int m = nd.m, n = a.n;
  double *x = a.x + nd.voff, *du = a.du + nd.voff, *lo = a.lo + nd.voff, *up = a.up + nd.voff;
  int *st = a.st + nd.voff;
  const int g = (int)blockIdx.x * 256 + TIDX + 1; // tableau row g and non-basic position g
  if (g <= m) {
    const int k = nd.bvar[g];
    if (k >= 1 && k <= m + n) {
      x[k] = nd.T[(size_t)g * (size_t)nd.ld];
      du[k] = 0.0;
      lo[k] = nd.blb[g];
      up[k] = nd.bub[g];
      st[k] = MVX_BS;
    }
  }
  if (g <= n) {
    const int k = nd.nvar[g];
    if (k >= 1 && k <= m + n) {
      const int f = nd.nflag[g];
      const double l = nd.nlb[g], u = nd.nub[g];
      x[k] = dev_nb_value(f, l, u);
      du[k] = nd.T[g];
      lo[k] = l;
      up[k] = u;
      st[k] = f;
    }
  }
}

// the PB and DB terms of the variable at offset o of the by-variable arrays
__device__ __forceinline__ void kkt_var_terms(const KktArgs &a, size_t o, double sg) {
  const double x = a.x[o], l = a.lo[o], u = a.up[o], d = a.du[o];
  double ae = 0.0, re = 0.0;
  if (fabs(l) != INFINITY && x < l) {
    ae = l - x;
    re = xdiv(ae, 1.0 + fabs(l));
  } else if (fabs(u) != INFINITY && x > u) {
    ae = x - u;
    re = xdiv(ae, 1.0 + fabs(u));
  }
  a.term[2][o] = ae;
  a.term[3][o] = re;
  const int s = a.st[o];
  const double e = sg * d;
  double v;
  if (s == MVX_NL) v = -e > 0.0 ? -e : 0.0;
  else if (s == MVX_NU) v = e > 0.0 ? e : 0.0;
  else if (s == MVX_NF) v = fabs(e);
  else if (s == MVX_NS) v = 0.0;
  else v = fabs(d);
  a.term[6][o] = v;
  a.term[7][o] = xdiv(v, 1.0 + fabs(d));
}

// sum_j row[j] v[j], j = 1..n, by one wave: 64 chains, lane l taking j = l+1, l+65, ... ascending with fma from +0.0 over a
// coalesced row, combined by the halving tree.  Every lane returns the sum its part of the tree leaves; lane 0's is the sum
__device__ __forceinline__ double kkt_row_sum(const double *__restrict__ row, const double *__restrict__ v, int n, int lane) {
  double acc = 0.0;
#pragma unroll 4
  for (int j = lane + 1; j <= n; j += 64) acc = fma(row[j], v[j], acc);
  for (int h = 32; h >= 1; h >>= 1) acc = acc + __shfl_xor(acc, h);
  return acc;
}

__global__ __launch_bounds__(64 * KKT_WAVES) void k_kkt_rows(KktArgs a) {
  const KktNode nd = a.nodes[blockIdx.y];
  const int lane = TIDX & 63, i = (int)blockIdx.x * KKT_WAVES + (TIDX >> 6) + 1;
  if (i > nd.m) return;
  const int n = a.n;
  const double *__restrict__ row = i <= a.m0 ? a.Ar + (size_t)(i - 1) * (size_t)a.ldn : nd.cuts + (size_t)(i - a.m0 - 1) * (size_t)(n + 1);
  const double acc = kkt_row_sum(row, a.x + nd.voff + (size_t)nd.m, n, lane);
  if (lane != 0) return;
  const size_t o = nd.voff + (size_t)i;
  const double xr = a.x[o];
  const double r = xr - acc, ae = fabs(r);
  a.res[o] = r;
  a.term[0][o] = ae;
  a.term[1][o] = xdiv(ae, 1.0 + fabs(xr));
  kkt_var_terms(a, o, nd.sg);
}

// sum_i a_ij v_i, i = 1..m, by one wave: column j of the root's rows (col = At + j ldm) and of the handle's cut rows behind them, in
// the 64 chains of k_kkt_rows.  Every lane returns the sum its part of the halving tree leaves; lane 0's is the sum
__device__ __forceinline__ double kkt_col_sum(const double *__restrict__ col, const double *__restrict__ cuts, const double *__restrict__ v,
                                              int j, int n, int m, int m0, int lane) {
  double acc = 0.0;
  int i = lane + 1;
#pragma unroll 4
  for (; i <= m0; i += 64) acc = fma(col[i - 1], v[i], acc);
  for (; i <= m; i += 64) acc = fma(cuts[(size_t)(i - m0 - 1) * (size_t)(n + 1) + (size_t)j], v[i], acc);
  for (int h = 32; h >= 1; h >>= 1) acc = acc + __shfl_xor(acc, h);
  return acc;
}

__global__ __launch_bounds__(64 * KKT_WAVES) void k_kkt_cols(KktArgs a) {
  const KktNode nd = a.nodes[blockIdx.y];
  const int lane = TIDX & 63, j = (int)blockIdx.x * KKT_WAVES + (TIDX >> 6) + 1;
  const int n = a.n, m = nd.m, m0 = a.m0;
  if (j > n) return;
  const double acc = kkt_col_sum(a.At + (size_t)j * (size_t)a.ldm, nd.cuts, a.du + nd.voff, j, n, m, m0, lane);
  if (lane != 0) return;
  const size_t o = nd.voff + (size_t)m + (size_t)j;
  const double cj = nd.c ? nd.c[j] : a.c0[j];
  const double r = (cj - acc) - a.du[o], ae = fabs(r);
  a.res[o] = r;
  a.term[4][o] = ae;
  a.term[5][o] = xdiv(ae, 1.0 + fabs(cj));
  kkt_var_terms(a, o, nd.sg);
}

__global__ __launch_bounds__(256) void k_kkt_fin(KktArgs a) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  const KktNode nd = a.nodes[blockIdx.y];
  const int m = nd.m, n = a.n, lane = TIDX & 63, wave = TIDX >> 6;
  const int t = (int)blockIdx.x, c = t >> 1;
  // PE rows 1..m, PB / DB variables 1..m+n, DE columns 1..n (stored behind the rows)
  const int cnt = c == 0 ? m : c == 2 ? n : m + n;
  const double *__restrict__ v = a.term[t] + nd.voff + (size_t)(c == 2 ? m : 0);
  double best = 0.0;
  int bi = 0;
  int k = 1 + TIDX;
  for (; k + 768 <= cnt; k += 1024) { // four loads in flight, seen in ascending order
    const double w0 = v[k], w1 = v[k + 256], w2 = v[k + 512], w3 = v[k + 768];
    if (w0 > best) { best = w0; bi = k; }
    if (w1 > best) { best = w1; bi = k + 256; }
    if (w2 > best) { best = w2; bi = k + 512; }
    if (w3 > best) { best = w3; bi = k + 768; }
  }
  for (; k <= cnt; k += 256) {
    const double w = v[k];
    if (w > best) {
      best = w;
      bi = k;
    }
  }
  for (int h = 32; h >= 1; h >>= 1) {
    const double w = __shfl_xor(best, h);
    const int wi = __shfl_xor(bi, h);
    if (w > best || (w == best && wi < bi)) {
      best = w;
      bi = wi;
    }
  }
  if (lane == 0) {
    s_v[wave] = best;
    s_i[wave] = bi;
  }
  __syncthreads();
  if (TIDX == 0) {
    for (int w = 1; w < 4; w++)
      if (s_v[w] > best || (s_v[w] == best && s_i[w] < bi)) {
        best = s_v[w];
        bi = s_i[w];
      }
    a.val[(size_t)blockIdx.y * 8 + t] = best;
    a.ind[(size_t)blockIdx.y * 8 + t] = bi;
  }
}

void launch_kkt(const KktArgs &a0, hipStream_t s) {
  for (int t0 = 0; t0 < a0.count; t0 += 32768) { // the handles ride on grid.y
    KktArgs a = a0;
    a.nodes += t0;
    a.val += (size_t)t0 * 8;
    a.ind += (size_t)t0 * 8;
    a.count = a0.count - t0 < 32768 ? a0.count - t0 : 32768;
    const unsigned cnt = (unsigned)a.count;
    const int longest = a.mmax > a.n ? a.mmax : a.n;
    hipLaunchKernelGGL(k_kkt_vals, dim3((unsigned)((longest + 255) / 256), cnt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kkt_rows, dim3((unsigned)((a.mmax + KKT_WAVES - 1) / KKT_WAVES), cnt), dim3(64 * KKT_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_kkt_cols, dim3((unsigned)((a.n + KKT_WAVES - 1) / KKT_WAVES), cnt), dim3(64 * KKT_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_kkt_fin, dim3(8, cnt), dim3(256), 0, s, a);
  }
}

// ------------------------------------------------------------- k_farkas_rows / k_farkas_pick / k_farkas_vars / k_farkas_cols / k_farkas_fin
// Farkas proof of infeasible handles (mvx_farkas_many, DESIGN.md "Infeasibility and unboundedness proofs (farkas)").  Five launches
// over all handles:
//  1. k_farkas_rows, a wave per (handle, tableau row i): the interval rule on the row's form over the slab positions p = 0..n -- p = 0
//     the basic variable with coefficient 1 and the row's bounds, p = q the non-basic position q with -T[i][q] (the slab stores
//     eval_tab_row's alpha itself) and the position's bounds -- lane l taking p = l, l+64, ... ascending over a coalesced row, the
//     chains combined by the halving tree through __shfl_xor.  Lane 0 writes rel of both sides;
//  2. k_farkas_pick, a workgroup per handle: the largest rel above FARKAS_REL, the lowest (row, side) among equals -- exact, so the
//     order of the combination is free;
//  3. k_farkas_vars, a thread per (handle, tableau row and non-basic position): the picked row's form and the bounds by variable;
//  4. k_farkas_cols, a wave per (handle, column j): w_j = sum_r a_rj y_r by kkt_col_sum, g_(m+j) = -w_j and the de term;
//  5. k_farkas_fin, a workgroup per handle: wave 0 the interval rule on g over k = 1..m+n (lane l taking k = l+1, l+65, ...), waves
//     1..3 the largest de term; thread 0 writes the handle's val / ind.
// No atomics, no LDS beyond the wave partials of 2 and 5, nothing waits on another workgroup.  Quotients are correctly rounded (xdiv).

// the two sides of the interval rule as one lane carries them
struct FkAcc {
  double lo = 0.0, alo = 0.0, hi = 0.0, ahi = 0.0;
  int ilo = 0, ihi = 0, dlo = 0, dhi = 0;
};

// one side's term: a bound that is infinite drops the term (|f| <= FARKAS_Z, counted in d) or makes the side infinite (counted in
// i); the fma runs either way, with the bound 0
__device__ __forceinline__ void fk_side(double f, double b, double &sum, double &act, int &i, int &d) {
  if (fabs(b) == INFINITY) {
    if (fabs(f) <= FARKAS_Z) d++;
    else i++;
    b = 0.0;
  }
  sum = fma(f, b, sum);
  act = fma(fabs(f), fabs(b), act);
}

__device__ __forceinline__ void fk_term(FkAcc &s, double f, double l, double u) {
  double bl = f < 0.0 ? u : l, bh = f < 0.0 ? l : u;
  if (f == 0.0) bl = bh = 0.0; // an exact zero takes part with the bound 0
  fk_side(f, bl, s.lo, s.alo, s.ilo, s.dlo);
  fk_side(f, bh, s.hi, s.ahi, s.ihi, s.dhi);
}

// the halving tree over the 64 lanes of a wave; lane 0 holds the result
__device__ __forceinline__ void fk_reduce(FkAcc &s) {
  for (int h = 32; h >= 1; h >>= 1) {
    s.lo = s.lo + __shfl_xor(s.lo, h);
    s.alo = s.alo + __shfl_xor(s.alo, h);
    s.hi = s.hi + __shfl_xor(s.hi, h);
    s.ahi = s.ahi + __shfl_xor(s.ahi, h);
    s.ilo += __shfl_xor(s.ilo, h);
    s.ihi += __shfl_xor(s.ihi, h);
    s.dlo += __shfl_xor(s.dlo, h);
    s.dhi += __shfl_xor(s.dhi, h);
  }
}

__device__ __forceinline__ double fk_rel_lo(const FkAcc &s) { return s.ilo == 0 ? xdiv(s.lo, 1.0 + s.alo) : -INFINITY; }
__device__ __forceinline__ double fk_rel_hi(const FkAcc &s) { return s.ihi == 0 ? xdiv(-s.hi, 1.0 + s.ahi) : -INFINITY; }

__global__ __launch_bounds__(64 * FARKAS_WAVES) void k_farkas_rows(FkArgs a) {
  const FkNode nd = a.nodes[blockIdx.y];
  const int lane = TIDX & 63, i = (int)blockIdx.x * FARKAS_WAVES + (TIDX >> 6) + 1;
  if (i > nd.m) return;
  const int n = a.n;
  const double *__restrict__ Ti = nd.T + (size_t)i * (size_t)nd.ld;
  const double *__restrict__ nlb = nd.nlb, *__restrict__ nub = nd.nub;
  FkAcc s;
  int p = lane;
  if (p == 0) { // the basic variable
    fk_term(s, 1.0, nd.blb[i], nd.bub[i]);
    p = 64;
  }
#pragma unroll 2
  for (; p <= n; p += 64) fk_term(s, -Ti[p], nlb[p], nub[p]);
  fk_reduce(s);
  if (lane != 0) return;
  double *r = a.rrel + nd.roff + 2 * (size_t)(i - 1);
  r[0] = fk_rel_lo(s);
  r[1] = fk_rel_hi(s);
}

__global__ __launch_bounds__(256) void k_farkas_pick(FkArgs a) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  const FkNode nd = a.nodes[blockIdx.x];
  const int cnt = 2 * nd.m, lane = TIDX & 63, wave = TIDX >> 6;
  const double *__restrict__ v = a.rrel + nd.roff;
  double best = FARKAS_REL;
  int bi = 0x7fffffff; // no candidate
  for (int e = TIDX; e < cnt; e += 256) {
    const double w = v[e];
    if (w > best) {
      best = w;
      bi = e;
    }
  }
  for (int h = 32; h >= 1; h >>= 1) {
    const double w = __shfl_xor(best, h);
    const int wi = __shfl_xor(bi, h);
    if (w > best || (w == best && wi < bi)) {
      best = w;
      bi = wi;
    }
  }
  if (lane == 0) {
    s_v[wave] = best;
    s_i[wave] = bi;
  }
  __syncthreads();
  if (TIDX == 0) {
    for (int w = 1; w < 4; w++)
      if (s_v[w] > best || (s_v[w] == best && s_i[w] < bi)) {
        best = s_v[w];
        bi = s_i[w];
      }
    a.pick[blockIdx.x] = bi == 0x7fffffff ? -1 : bi;
    a.val[(size_t)blockIdx.x * 4] = bi == 0x7fffffff ? 0.0 : best;
  }
}

__global__ __launch_bounds__(256) void k_farkas_vars(FkArgs a) {
  const FkNode nd = a.nodes[blockIdx.y];
  const int m = nd.m, n = a.n;
  const int e = a.pick[blockIdx.y], ip = e < 0 ? 0 : (e >> 1) + 1; // the picked row, 0 without one
  double *f = a.f + nd.voff, *gv = a.g + nd.voff, *lo = a.lo + nd.voff, *up = a.up + nd.voff;
  const int g = (int)blockIdx.x * 256 + TIDX + 1; // tableau row g and non-basic position g
  if (g <= m) {
    const int k = nd.bvar[g];
    if (k >= 1 && k <= m + n) {
      const double v = g == ip ? 1.0 : 0.0;
      f[k] = v;
      gv[k] = v;
      lo[k] = nd.blb[g];
      up[k] = nd.bub[g];
    }
  }
  if (g <= n) {
    const int k = nd.nvar[g];
    if (k >= 1 && k <= m + n) {
      const double v = ip > 0 ? -nd.T[(size_t)ip * (size_t)nd.ld + (size_t)g] : 0.0;
      f[k] = v;
      gv[k] = v;
      lo[k] = nd.nlb[g];
      up[k] = nd.nub[g];
    }
  }
}

__global__ __launch_bounds__(64 * FARKAS_WAVES) void k_farkas_cols(FkArgs a) {
  const FkNode nd = a.nodes[blockIdx.y];
  const int lane = TIDX & 63, j = (int)blockIdx.x * FARKAS_WAVES + (TIDX >> 6) + 1;
  const int n = a.n, m = nd.m;
  if (j > n) return;
  const double w = kkt_col_sum(a.At + (size_t)j * (size_t)a.ldm, nd.cuts, a.f + nd.voff, j, n, m, a.m0, lane);
  if (lane != 0) return;
  const size_t o = nd.voff + (size_t)m + (size_t)j;
  const double gj = -w, z = a.f[o];
  a.g[o] = gj;
  a.dterm[o] = xdiv(fabs(gj - z), 1.0 + fabs(z));
}

__global__ __launch_bounds__(256) void k_farkas_fin(FkArgs a) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  const FkNode nd = a.nodes[blockIdx.x];
  const int m = nd.m, n = a.n, lane = TIDX & 63, wave = TIDX >> 6;
  FkAcc s;
  double best = 0.0;
  int bi = 0;
  if (wave == 0) { // the interval rule on g
    const double *__restrict__ gv = a.g + nd.voff, *__restrict__ lo = a.lo + nd.voff, *__restrict__ up = a.up + nd.voff;
#pragma unroll 2
    for (int k = lane + 1; k <= m + n; k += 64) fk_term(s, gv[k], lo[k], up[k]);
    fk_reduce(s);
  } else { // the largest de term, the lowest column among equals
    const double *__restrict__ v = a.dterm + nd.voff + (size_t)m;
    for (int j = TIDX - 63; j <= n; j += 192) {
      const double w = v[j];
      if (w > best) {
        best = w;
        bi = j;
      }
    }
    for (int h = 32; h >= 1; h >>= 1) {
      const double w = __shfl_xor(best, h);
      const int wi = __shfl_xor(bi, h);
      if (w > best || (w == best && wi < bi)) {
        best = w;
        bi = wi;
      }
    }
    if (lane == 0) {
      s_v[wave] = best;
      s_i[wave] = bi;
    }
  }
  __syncthreads();
  if (TIDX != 0) return;
  double *val = a.val + (size_t)blockIdx.x * 4;
  int *ind = a.ind + (size_t)blockIdx.x * 4;
  const int e = a.pick[blockIdx.x];
  if (e < 0) {
    val[0] = val[1] = val[2] = val[3] = 0.0;
    ind[0] = ind[1] = ind[2] = ind[3] = 0;
    return;
  }
  double de = s_v[1];
  int dj = s_i[1];
  for (int w = 2; w < 4; w++)
    if (s_v[w] > de || (s_v[w] == de && s_i[w] < dj)) {
      de = s_v[w];
      dj = s_i[w];
    }
  const double rl = fk_rel_lo(s), rh = fk_rel_hi(s);
  const bool upper = rh > rl; // the lower side before the upper
  const double rel = upper ? rh : rl;
  val[1] = rel;
  val[2] = (upper ? s.ihi : s.ilo) != 0 ? -INFINITY : upper ? -s.hi : s.lo;
  val[3] = de;
  ind[0] = rel > FARKAS_REL ? 2 : 1;
  ind[1] = (e >> 1) + 1;
  ind[2] = (e & 1) + 1;
  ind[3] = upper ? s.dhi : s.dlo;
}

void launch_farkas(const FkArgs &a0, hipStream_t s) {
  for (int t0 = 0; t0 < a0.count; t0 += 32768) { // the handles ride on grid.y
    FkArgs a = a0;
    a.nodes += t0;
    a.pick += t0;
    a.val += (size_t)t0 * 4;
    a.ind += (size_t)t0 * 4;
    a.count = a0.count - t0 < 32768 ? a0.count - t0 : 32768;
    const unsigned cnt = (unsigned)a.count;
    const int longest = a.mmax > a.n ? a.mmax : a.n;
    hipLaunchKernelGGL(k_farkas_rows, dim3((unsigned)((a.mmax + FARKAS_WAVES - 1) / FARKAS_WAVES), cnt), dim3(64 * FARKAS_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_farkas_pick, dim3(cnt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_farkas_vars, dim3((unsigned)((longest + 255) / 256), cnt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_farkas_cols, dim3((unsigned)((a.n + FARKAS_WAVES - 1) / FARKAS_WAVES), cnt), dim3(64 * FARKAS_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_farkas_fin, dim3(cnt), dim3(256), 0, s, a);
  }
}

// ------------------------------------------------------------------ k_ray_cols / k_ray_pick / k_ray_vars / k_ray_rows / k_ray_fin
// The ray of an unbounded handle (mvx_ray, DESIGN.md "Infeasibility and unboundedness proofs (farkas)").  Five launches:
//  1. k_ray_cols, a thread per non-basic position q: the direction its status allows in which the published dual T[0][q] improves
//     by more than RAY_TOL, provided its own bound on that side is infinite and no basic variable with |alpha_iq| > FARKAS_Z meets
//     a finite bound on its way -- one walk down column q of the slab, coalesced across the threads;
//  2. k_ray_pick, one workgroup: the lowest such position;
//  3. k_ray_vars, a thread per (tableau row and non-basic position): the ray and the bounds by variable;
//  4. k_ray_rows, a wave per model row: rho_r = dR_r - sum_j a_rj dS_j by kkt_row_sum, the row's ae and re terms;
//  5. k_ray_fin, one workgroup: wave 0 the slope sum_j c_j dS_j in the same 64 chains, waves 1..3 the largest ae and re (the lowest
//     row among equals) and the variables whose bound blocks the ray; thread 0 writes val / ind.
__global__ __launch_bounds__(256) void k_ray_cols(RayArgs a) {
  const NodeRef nd = a.nd;
  const int q = (int)blockIdx.x * 256 + TIDX + 1;
  if (q > a.n) return;
  const double e = a.sg * nd.T[q];
  const int f = nd.nflag[q];
  int sigma = 0;
  if (e < -RAY_TOL && (f == MVX_NL || f == MVX_NF)) sigma = 1;
  else if (e > RAY_TOL && (f == MVX_NU || f == MVX_NF)) sigma = -1;
  if (sigma != 0 && (sigma > 0 ? nd.nub[q] != INFINITY : nd.nlb[q] != -INFINITY)) sigma = 0;
  if (sigma != 0) {
    const double sd = (double)sigma;
    const double *__restrict__ col = nd.T + (size_t)q;
    for (int i = 1; i <= nd.m; i++) {
      const double al = col[(size_t)i * (size_t)nd.ld], mv = sd * al;
      if (fabs(al) <= FARKAS_Z) continue;
      if (mv > 0.0 ? a.bub[i] != INFINITY : a.blb[i] != -INFINITY) {
        sigma = 0;
        break;
      }
    }
  }
  a.open[q] = sigma;
}

__global__ __launch_bounds__(256) void k_ray_pick(RayArgs a) {
  __shared__ int s_q[4];
  const int lane = TIDX & 63, wave = TIDX >> 6;
  int best = 0x7fffffff;
  for (int q = 1 + TIDX; q <= a.n; q += 256)
    if (a.open[q] != 0 && q < best) best = q;
  for (int h = 32; h >= 1; h >>= 1) {
    const int w = __shfl_xor(best, h);
    if (w < best) best = w;
  }
  if (lane == 0) s_q[wave] = best;
  __syncthreads();
  if (TIDX == 0) {
    for (int w = 1; w < 4; w++)
      if (s_q[w] < best) best = s_q[w];
    a.pick[0] = best == 0x7fffffff ? 0 : best;
  }
}

__global__ __launch_bounds__(256) void k_ray_vars(RayArgs a) {
  const NodeRef nd = a.nd;
  const int m = nd.m, n = a.n, qp = a.pick[0];
  const double sd = qp > 0 ? (double)a.open[qp] : 0.0;
  const int g = (int)blockIdx.x * 256 + TIDX + 1; // tableau row g and non-basic position g
  if (g <= m) {
    const int k = nd.bvar[g];
    if (k >= 1 && k <= m + n) {
      a.d[k] = qp > 0 ? sd * nd.T[(size_t)g * (size_t)nd.ld + (size_t)qp] : 0.0;
      a.lo[k] = a.blb[g];
      a.up[k] = a.bub[g];
    }
  }
  if (g <= n) {
    const int k = nd.nvar[g];
    if (k >= 1 && k <= m + n) {
      a.d[k] = g == qp ? sd : 0.0;
      a.lo[k] = nd.nlb[g];
      a.up[k] = nd.nub[g];
    }
  }
}

__global__ __launch_bounds__(64 * KKT_WAVES) void k_ray_rows(RayArgs a) {
  const int lane = TIDX & 63, i = (int)blockIdx.x * KKT_WAVES + (TIDX >> 6) + 1;
  if (i > a.nd.m) return;
  const double acc = kkt_row_sum(a.Ar + (size_t)(i - 1) * (size_t)a.ldn, a.d + a.nd.m, a.n, lane);
  if (lane != 0) return;
  const double dr = a.d[i], ae = fabs(dr - acc);
  a.rae[i] = ae;
  a.rre[i] = xdiv(ae, 1.0 + fabs(dr));
}

__global__ __launch_bounds__(256) void k_ray_fin(RayArgs a) {
  __shared__ double s_ae[4], s_re[4];
  __shared__ int s_ai[4], s_ri[4], s_bl[4];
  const int m = a.nd.m, n = a.n, lane = TIDX & 63, wave = TIDX >> 6;
  double slope = 0.0;
  if (wave == 0) {
    slope = kkt_row_sum(a.c, a.d + m, n, lane);
  } else {
    double ae = 0.0, re = 0.0;
    int ai = 0, ri = 0, bl = 0;
    for (int i = TIDX - 63; i <= m; i += 192) {
      const double w = a.rae[i], r = a.rre[i];
      if (w > ae) { ae = w; ai = i; }
      if (r > re) { re = r; ri = i; }
    }
    for (int k = TIDX - 63; k <= m + n; k += 192) {
      const double v = a.d[k];
      if (fabs(v) <= FARKAS_Z) continue; // the zero rule
      if (v > 0.0 ? a.up[k] != INFINITY : a.lo[k] != -INFINITY) bl++;
    }
    for (int h = 32; h >= 1; h >>= 1) {
      const double w = __shfl_xor(ae, h), r = __shfl_xor(re, h);
      const int wi = __shfl_xor(ai, h), qi = __shfl_xor(ri, h);
      if (w > ae || (w == ae && wi < ai)) { ae = w; ai = wi; }
      if (r > re || (r == re && qi < ri)) { re = r; ri = qi; }
      bl += __shfl_xor(bl, h);
    }
    if (lane == 0) {
      s_ae[wave] = ae; s_ai[wave] = ai; s_re[wave] = re; s_ri[wave] = ri; s_bl[wave] = bl;
    }
  }
  __syncthreads();
  if (TIDX != 0) return;
  const int qp = a.pick[0];
  if (qp == 0) {
    a.val[0] = a.val[1] = a.val[2] = a.val[3] = 0.0;
    for (int t = 0; t < 6; t++) a.ind[t] = 0;
    return;
  }
  double ae = s_ae[1], re = s_re[1];
  int ai = s_ai[1], ri = s_ri[1], bl = s_bl[1];
  for (int w = 2; w < 4; w++) {
    if (s_ae[w] > ae || (s_ae[w] == ae && s_ai[w] < ai)) { ae = s_ae[w]; ai = s_ai[w]; }
    if (s_re[w] > re || (s_re[w] == re && s_ri[w] < ri)) { re = s_re[w]; ri = s_ri[w]; }
    bl += s_bl[w];
  }
  a.val[0] = a.nd.T[qp];
  a.val[1] = ae;
  a.val[2] = re;
  a.val[3] = slope;
  a.ind[0] = (a.sg * slope < 0.0 && re <= RAY_TOL && bl == 0) ? 2 : 1;
  a.ind[1] = a.nd.nvar[qp];
  a.ind[2] = a.open[qp];
  a.ind[3] = bl;
  a.ind[4] = ai;
  a.ind[5] = ri;
}

void launch_ray(const RayArgs &a, hipStream_t s) {
  const int m = a.nd.m, longest = m > a.n ? m : a.n;
  hipLaunchKernelGGL(k_ray_cols, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ray_pick, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ray_vars, dim3((unsigned)((longest + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ray_rows, dim3((unsigned)((m + KKT_WAVES - 1) / KKT_WAVES)), dim3(64 * KKT_WAVES), 0, s, a);
  hipLaunchKernelGGL(k_ray_fin, dim3(1), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_round
// Primal rounding heuristic (mvx_round_many, DESIGN.md "Primal rounding heuristic"), one workgroup per handle.
//  1. the node LP's column values (node_col_values: get_col_prim's bits) into LDS;
//  2. each integer column rounded (within 1e-9 of an integer: that integer; else away from its locks; else to nearest)
//     and clipped to the root's integer range; the fill order's key, the value's fractional part;
//  3. mode 2: the columns sorted into the fill order (fractional part descending, column ascending) by a bitonic sort in LDS;
//  4. row activities: a row per lane, the columns in ascending order, zero values skipped (they add nothing: a sum started
//     at +0 never holds -0), products and sums rounded one by one -- the host twin's bits;
//  5. mode 2 on a feasible point: one column at a time, the largest step every row allows, a minimum over the rows
//     (correctly rounded quotients, xdiv) by wave shuffles and four partials in LDS; the activities follow the step;
//  6. the objective: the non-zero products in ascending column order, summed by one wave.
// The row activities live in the LDS of the sort keys once the order is taken, or in a global slice when m0 > RND_NMAX.
__device__ __forceinline__ double rnd_tol(double b) { return 1e-9 * fmax(1.0, fabs(b)); } // a row bound's tolerance
__device__ __forceinline__ bool rnd_before(double ka, int ia, double kb, int ib) {          // fill order
  return ka > kb || (ka == kb && ia < ib);
}

__global__ __launch_bounds__(256) void k_round(RndArgs a) {
  __shared__ double s_x[RND_NMAX + 1];
  __shared__ double s_key[RND_NMAX]; // fill-order keys; the row activities once the order is taken (m0 <= RND_NMAX)
  __shared__ int s_idx[RND_NMAX];
  __shared__ double s_red[2][4];
  __shared__ int s_bad;
  const int t = (int)blockIdx.x;
  const RndNode nd = a.nodes[t];
  const int n = a.n, m0 = a.m0;
  const size_t ldm = (size_t)a.ldm;
  const double inf = __builtin_huge_val();
  const int lane = TIDX & 63, wv = TIDX >> 6;
  if (TIDX == 0) s_bad = 0;
  node_col_values(nd, n, [&](int j, double v) { s_x[j] = v; });
  __syncthreads();
  int np = 1;
  while (np < n) np <<= 1;
  bool bad = false;
  for (int j = 1 + TIDX; j <= n; j += 256) {
    const double v = s_x[j];
    const int f = a.flags[j];
    double xr = v, key = -1.0;
    if (f & RND_INT) {
      const double r = rint(v);
      if (fabs(v - r) <= 1e-9) xr = r;
      else if (!(f & RND_DLOCK)) xr = floor(v);
      else if (!(f & RND_ULOCK)) xr = ceil(v);
      else xr = floor(v + 0.5);
      const double lo = ceil(a.clo[j]), hi = floor(a.chi[j]);
      if (xr < lo) xr = lo;
      if (xr > hi) xr = hi;
      key = v - floor(v);
    }
    bad = bad || !(a.clo[j] <= xr && xr <= a.chi[j]);
    s_x[j] = xr;
    s_key[j - 1] = key;
    s_idx[j - 1] = j;
  }
  for (int p = n + TIDX; p < np; p += 256) {
    s_key[p] = -2.0;
    s_idx[p] = 0x7fffffff;
  }
  __syncthreads();
  if (a.mode == 2) {
    for (int k2 = 2; k2 <= np; k2 <<= 1)
      for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
        for (int i = TIDX; i < np; i += 256) {
          const int l = i ^ jj;
          if (l <= i) continue;
          const double ki = s_key[i], kl = s_key[l];
          const int ii = s_idx[i], il = s_idx[l];
          const bool sw = ((i & k2) == 0) ? rnd_before(kl, il, ki, ii) : rnd_before(ki, ii, kl, il);
          if (sw) {
            s_key[i] = kl; s_key[l] = ki;
            s_idx[i] = il; s_idx[l] = ii;
          }
        }
        __syncthreads();
      }
  }
  double *r = m0 <= RND_NMAX ? s_key : a.scratch + (size_t)t * (size_t)m0;
  for (int i = TIDX; i < m0; i += 256) {
    double acc = 0.0;
    for (int j = 1; j <= n; j++) {
      const double xj = s_x[j];
      if (xj != 0.0) acc = __dadd_rn(acc, __dmul_rn(a.At[(size_t)j * ldm + i], xj));
    }
    r[i] = acc;
    const double lo = a.rlo[i], hi = a.rhi[i];
    bad = bad || !(acc >= lo - rnd_tol(lo) && acc <= hi + rnd_tol(hi));
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (a.mode == 2 && !s_bad) {
    // up to RND_RPT * 256 rows: each thread keeps its rows' activities and the column at hand in registers, and loads the
    // next column of the order while this one is reduced (same values, same operations: only the loads move)
    const bool regs = m0 <= RND_RPT * 256;
    double av[RND_RPT], nx[RND_RPT], rr[RND_RPT];
    auto load_col = [&](int jj, double *dst) {
#pragma unroll
      for (int q = 0; q < RND_RPT; q++) {
        const int i = TIDX + 256 * q;
        dst[q] = (jj <= n && i < m0) ? a.At[(size_t)jj * ldm + i] : 0.0;
      }
    };
    if (regs) {
#pragma unroll
      for (int q = 0; q < RND_RPT; q++) rr[q] = TIDX + 256 * q < m0 ? r[TIDX + 256 * q] : 0.0;
      load_col(s_idx[0], nx);
    }
    int ph = 0; // s_red buffer of the next barrier: it flips at every barrier, not at every column (zero-cost columns have none)
    for (int k = 0; k < n; k++) {
      const int j = s_idx[k];
      if (j > n || !(a.flags[j] & RND_INT)) break; // integer columns come first; then the continuous ones, the padding
      if (regs) {
#pragma unroll
        for (int q = 0; q < RND_RPT; q++) av[q] = nx[q];
        load_col(k + 1 < n ? s_idx[k + 1] : n + 1, nx);
      }
      const double sc = a.sg * a.c[j];
      if (!(sc != 0.0)) continue; // uniform: every thread skips the column, and its barrier
      const double d = sc > 0.0 ? 1.0 : -1.0;
      const double *col = a.At + (size_t)j * ldm;
      // x_j and its room are read in front of the barrier: thread 0 writes x_j behind it, in this same interval
      const double xj = s_x[j];
      const double room = d > 0.0 ? floor(a.chi[j]) - xj : xj - ceil(a.clo[j]);
      double q = inf;
      auto limit = [&](double aij, double ri, int i) {
        const double da = d * aij;
        if (da > 0.0) {
          const double hi = a.rhi[i];
          if (hi < inf) q = fmin(q, xdiv(__dsub_rn(__dadd_rn(hi, rnd_tol(hi)), ri), da));
        } else if (da < 0.0) {
          const double lo = a.rlo[i];
          if (lo > -inf) q = fmin(q, xdiv(__dadd_rn(__dsub_rn(ri, lo), rnd_tol(lo)), -da));
        }
      };
      if (regs) {
#pragma unroll
        for (int u = 0; u < RND_RPT; u++)
          if (TIDX + 256 * u < m0) limit(av[u], rr[u], TIDX + 256 * u);
      } else {
        for (int i = TIDX; i < m0; i += 256) limit(col[i], r[i], i);
      }
      for (int off = 32; off > 0; off >>= 1) q = fmin(q, __shfl_xor(q, off, 64));
      // s_red is double-buffered: a wave writes buffer ph only after every wave has passed the barrier that followed the
      // last reads of ph (the one in between), so one barrier per column suffices
      if (lane == 0) s_red[ph][wv] = q;
      __syncthreads();
      const double qm = fmin(fmin(s_red[ph][0], s_red[ph][1]), fmin(s_red[ph][2], s_red[ph][3]));
      ph ^= 1;
      const double tt = fmin(room, floor(qm));
      if (!(tt > 0.0) || isinf(tt)) continue; // no room, or nothing limits the column
      const double step = d * tt;
      if (regs) {
#pragma unroll
        for (int u = 0; u < RND_RPT; u++) rr[u] = __dadd_rn(rr[u], __dmul_rn(step, av[u]));
      } else {
        for (int i = TIDX; i < m0; i += 256) r[i] = __dadd_rn(r[i], __dmul_rn(step, col[i]));
      }
      if (TIDX == 0) s_x[j] = xj + step;
    }
    if (regs) {
#pragma unroll
      for (int u = 0; u < RND_RPT; u++)
        if (TIDX + 256 * u < m0) r[TIDX + 256 * u] = rr[u];
    }
    __syncthreads();
    bad = false; // the filled point, checked again
    for (int j = 1 + TIDX; j <= n; j += 256) bad = bad || !(a.clo[j] <= s_x[j] && s_x[j] <= a.chi[j]);
    for (int i = TIDX; i < m0; i += 256) {
      const double lo = a.rlo[i], hi = a.rhi[i];
      bad = bad || !(r[i] >= lo - rnd_tol(lo) && r[i] <= hi + rnd_tol(hi));
    }
    if (bad) s_bad = 2;
    __syncthreads();
  }
  double *xo = a.x + (size_t)t * (size_t)(n + 1);
  for (int j = 1 + TIDX; j <= n; j += 256) xo[j] = s_x[j];
  if (wv == 0) {
    double s = 0.0;
    for (int j0 = 1; j0 <= n; j0 += 64) {
      const int j = j0 + lane;
      const double p = j <= n ? __dmul_rn(a.c[j], s_x[j]) : 0.0;
      unsigned long long mk = __ballot(p != 0.0);
      while (mk) {
        const int b = __builtin_ctzll(mk);
        mk &= mk - 1ull;
        s = __dadd_rn(s, __shfl(p, b, 64));
      }
    }
    if (lane == 0) {
      xo[0] = 0.0;
      a.obj[t] = __dadd_rn(s, a.c[0]);
      a.found[t] = s_bad == 0 ? 1 : 0;
    }
  }
}

void launch_round(const RndArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_round, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_rcfix
// Reduced-cost bound tightening (mvx_rc_tighten_many, DESIGN.md "Reduced-cost tightening"), one workgroup per handle.  Row 0
// and the position-indexed nvar / nflag / nlb / nub are streamed once, coalesced; each non-basic position is decided on its
// own -- no reduction, so nothing depends on an order -- and written exactly once: code 0 (no change), 1 (upper bound
// becomes val) or 2 (lower bound becomes val).  The host maps positions to columns through its nvar mirror.  The quotient
// is the correctly rounded one (xdiv): the host twin's bits.
__global__ __launch_bounds__(256) void k_rcfix(RcArgs a) {
  const int t = (int)blockIdx.x;
  const RcNode nd = a.nodes[t];
  int *code = a.code + (size_t)t * (size_t)(a.n + 1);
  double *val = a.val + (size_t)t * (size_t)(a.n + 1);
  const double gap2 = nd.gap2;
  const bool live = gap2 > 0.0; // a NaN or a cutoff the node cannot beat: no change anywhere
  for (int q = 1 + TIDX; q <= a.n; q += 256) {
    int cd = 0;
    double v = 0.0;
    const int var = nd.nvar[q];
    const int j = var - nd.m;
    if (live && j >= 1 && j <= a.n && a.kind[j] != MVX_CV) {
      const int f = nd.nflag[q];
      const double d = fabs(nd.T[q]);
      if ((f == MVX_NL || f == MVX_NU) && d > a.tol) {
        const double lb = nd.nlb[q], ub = nd.nub[q];
        const double at = f == MVX_NL ? lb : ub;
        if (at == rint(at)) {
          const double room = __dsub_rn(ceil(xdiv(gap2, d)), 1.0);
          if (f == MVX_NL) {
            v = __dadd_rn(at, room);
            if (v < ub) cd = 1;
          } else {
            v = __dsub_rn(at, room);
            if (v > lb) cd = 2;
          }
        }
      }
    }
    code[q] = cd;
    val[q] = v;
  }
}

void launch_rcfix(const RcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_rcfix, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_prop / k_setbnds
// Node bound propagation (mvx_propagate_many, DESIGN.md "Node bound propagation"), one workgroup per handle, all rounds in
// one launch.  A round is two private serial loops with one barrier between them and one behind:
//  A. rows on lanes: the activities of a row, its non-zeros in ascending column order out of the by-column model (a wave
//     reads one column of consecutive rows), the bounds broadcast from LDS; terms with an infinite bound are counted;
//  B. columns on lanes: the candidates of an integer column, its non-zeros out of the by-row model (a wave reads one row of
//     consecutive columns), the row activities broadcast from LDS (or the handle's global slice when m0 > RND_NMAX).  A
//     column's new bounds are exact minima / maxima of its candidates and depend on the bounds the round started with only
//     (a lane reads no other column's bounds here), so they go to LDS in place.
// Products, sums and quotients are rounded one by one (xdiv): the host twin's bits.  No atomics: the flags are set to 1 by
// whoever has a reason and read behind a barrier.
__global__ __launch_bounds__(256) void k_prop(PropArgs a) {
  __shared__ double s_l[RND_NMAX + 1], s_u[RND_NMAX + 1];
  __shared__ double s_min[RND_NMAX], s_max[RND_NMAX];
  __shared__ int s_k[RND_NMAX];
  __shared__ int s_badrow, s_cross, s_chg[2];
  const int t = (int)blockIdx.x;
  const int n = a.n, m0 = a.m0;
  const size_t ldm = (size_t)a.ldm, ldn = (size_t)a.ldn, base = (size_t)t * (size_t)(n + 1);
  for (int j = TIDX; j <= n; j += 256) {
    s_l[j] = a.lb0[base + j];
    s_u[j] = a.ub0[base + j];
  }
  if (TIDX == 0) {
    s_badrow = 0;
    s_cross = 0;
    s_chg[0] = s_chg[1] = 0;
  }
  const bool lds = m0 <= RND_NMAX;
  double *amin = lds ? s_min : a.act + (size_t)t * 2 * (size_t)m0;
  double *amax = lds ? s_max : amin + m0;
  int *ak = lds ? s_k : a.actk + (size_t)t * (size_t)m0;
  __syncthreads();
  int rounds = 0, infeasible = 0;
  for (int r = 0; r < a.max_rounds; r++) {
    rounds = r + 1;
    if (TIDX == 0) s_chg[r & 1] = 0; // last read two barriers ago; written again behind the next barrier
    for (int i = TIDX; i < m0; i += 256) {
      double lmin = 0.0, lmax = 0.0;
      int kmin = 0, kmax = 0;
      for (int j = 1; j <= n; j++) {
        const double v = a.At[(size_t)j * ldm + i];
        if (v == 0.0) continue;
        const double l = s_l[j], u = s_u[j];
        const double bmin = v > 0.0 ? l : u, bmax = v > 0.0 ? u : l;
        if (isinf(bmin)) kmin++;
        else lmin = __dadd_rn(lmin, __dmul_rn(v, bmin));
        if (isinf(bmax)) kmax++;
        else lmax = __dadd_rn(lmax, __dmul_rn(v, bmax));
      }
      amin[i] = lmin;
      amax[i] = lmax;
      ak[i] = (kmin > 2 ? 2 : kmin) | ((kmax > 2 ? 2 : kmax) << 2);
      const double lo = a.rlo[i], hi = a.rhi[i];
      if ((kmin == 0 && isfinite(hi) && lmin > __dadd_rn(hi, rnd_tol(hi))) || (kmax == 0 && isfinite(lo) && lmax < __dsub_rn(lo, rnd_tol(lo))))
        s_badrow = 1;
    }
    __syncthreads();
    if (s_badrow) {
      infeasible = 1;
      break;
    }
    for (int j = 1 + TIDX; j <= n; j += 256) {
      if (!(a.flags[j] & RND_INT)) continue;
      const double l = s_l[j], u = s_u[j];
      double nl = l, nu = u;
      for (int i = 0; i < m0; i++) {
        const double v = a.Ar[(size_t)i * ldn + j];
        if (v == 0.0) continue;
        const int kk = ak[i], kmin = kk & 3, kmax = kk >> 2;
        const double lo = a.rlo[i], hi = a.rhi[i];
        const double bmin = v > 0.0 ? l : u, bmax = v > 0.0 ? u : l;
        if (isfinite(hi) && (kmin == 0 || (kmin == 1 && isinf(bmin)))) {
          const double res = kmin == 0 ? __dsub_rn(amin[i], __dmul_rn(v, bmin)) : amin[i];
          const double q = xdiv(__dsub_rn(hi, res), v);
          if (isfinite(q)) {
            if (v > 0.0) {
              const double c = floor(__dadd_rn(q, rnd_tol(q)));
              if (c < nu) nu = c;
            } else {
              const double c = ceil(__dsub_rn(q, rnd_tol(q)));
              if (c > nl) nl = c;
            }
          }
        }
        if (isfinite(lo) && (kmax == 0 || (kmax == 1 && isinf(bmax)))) {
          const double res = kmax == 0 ? __dsub_rn(amax[i], __dmul_rn(v, bmax)) : amax[i];
          const double q = xdiv(__dsub_rn(lo, res), v);
          if (isfinite(q)) {
            if (v > 0.0) {
              const double c = ceil(__dsub_rn(q, rnd_tol(q)));
              if (c > nl) nl = c;
            } else {
              const double c = floor(__dadd_rn(q, rnd_tol(q)));
              if (c < nu) nu = c;
            }
          }
        }
      }
      if (nl != l || nu != u) {
        s_l[j] = nl;
        s_u[j] = nu;
        s_chg[r & 1] = 1;
      }
      if (nl > nu) s_cross = 1;
    }
    __syncthreads();
    if (s_cross) {
      infeasible = 1;
      break;
    }
    if (!s_chg[r & 1]) break;
  }
  for (int j = TIDX; j <= n; j += 256) {
    a.lb[base + j] = s_l[j];
    a.ub[base + j] = s_u[j];
  }
  if (TIDX == 0) {
    a.info[2 * t] = infeasible;
    a.info[2 * t + 1] = rounds;
  }
}

void launch_prop(const PropArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_prop, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// General bound lists of many handles in one launch (mvx_set_col_bnds_many; mvx_tighten_cols_many sends lists that touch
// non-basic positions only and move no resting value: entries, no shifts), one workgroup per handle with device work: its
// bound writes (a lane each; the host sends every row / position of a handle at most once), then a lane per tableau row 0..m, cut rows included, applies the
// handle's shifts of column 0 in list order -- the fma k_shift_nonbasic applies per launch, so the bits are the per-entry
// path's.  The shifts read columns jj >= 1 and write column 0 only, the writes touch the bound arrays only: no barrier.
__global__ __launch_bounds__(256) void k_setbnds(const SetbHandle *hs, const SetbEntry *es, const SetbShift *ss) {
  const SetbHandle h = hs[blockIdx.x];
  for (int k = h.e0 + TIDX; k < h.e1; k += 256) {
    const SetbEntry e = es[k];
    if (e.flag < 0) {
      h.blb[e.idx] = e.lb;
      h.bub[e.idx] = e.ub;
    } else {
      h.nlb[e.idx] = e.lb;
      h.nub[e.idx] = e.ub;
      h.nflag[e.idx] = e.flag;
    }
  }
  if (h.s1 <= h.s0) return;
  for (int i = TIDX; i <= h.m; i += 256) {
    double *row = h.T + (size_t)i * (size_t)h.ld;
    double acc = row[0];
    for (int k = h.s0; k < h.s1; k++) acc = fma(row[ss[k].jj], ss[k].delta, acc);
    row[0] = acc;
  }
}

void launch_setbnds(const SetbHandle *hs, const SetbEntry *es, const SetbShift *ss, int handles, hipStream_t s) {
  hipLaunchKernelGGL(k_setbnds, dim3((unsigned)handles), dim3(256), 0, s, hs, es, ss);
}

// ---------------------------------------------------------------------------- k_divepick
// The branching pick of a diving rule (mvx_dive_pick_many, DESIGN.md "LP diving heuristic"), one workgroup per (handle,
// rule).  A lane over the tableau rows takes the basic structural columns' values from column 0, a lane over the non-basic
// positions the bound the status names (dev_nb_value) -- k_classify's selection, get_col_prim's bits -- and evaluates the
// column on the spot from the per-column model arrays: integer and more than 1e-9 off an integer makes it a candidate, its
// key is the rule's.  Each lane keeps the count and the smallest (k1, k2, column) it met; the waves reduce with shuffles,
// four partials meet in LDS.  The order is strict and total, so the winner does not depend on the reduction tree: the host
// twin's bits.  No value array, no atomics.
struct DiveKey {
  double k1, k2, v; // k1 = +inf, j = INT_MAX: none
  int j, dir;
};
__device__ __forceinline__ bool dive_before(const DiveKey &a, const DiveKey &b) {
  return a.k1 < b.k1 || (a.k1 == b.k1 && (a.k2 < b.k2 || (a.k2 == b.k2 && a.j < b.j)));
}
__device__ __forceinline__ void dive_eval(const DiveArgs &a, int rule, int j, double v, DiveKey &best, int &cnt) {
  if (!(a.flags[j] & RND_INT)) return;
  if (!(fabs(v - rint(v)) > 1e-9)) return;
  const double fd = v - floor(v), fu = ceil(v) - v;
  const int near = fd <= fu ? 0 : 1;
  DiveKey k = {0.0, 0.0, v, j, near};
  if (rule == 1) {
    k.k1 = fd <= fu ? fd : fu;
  } else if (rule == 2) {
    const int dl = a.dl[j], ul = a.ul[j];
    k.dir = dl < ul ? 0 : ul < dl ? 1 : near;
    k.k1 = (double)(dl < ul ? dl : ul);
    k.k2 = k.dir ? fu : fd;
  } else {
    const double cj = a.c[j], s = a.sg * cj;
    k.dir = s > 0.0 ? 0 : s < 0.0 ? 1 : near;
    k.k1 = xdiv(fabs(cj) * (k.dir ? fu : fd), (double)(a.len[j] + 1)); // the host's division
  }
  cnt++;
  if (dive_before(k, best)) best = k;
}

__global__ __launch_bounds__(256) void k_divepick(DiveArgs a) {
  __shared__ double s_k1[4], s_k2[4], s_v[4];
  __shared__ int s_j[4], s_dir[4], s_cnt[4];
  const int t = (int)blockIdx.x;
  const DiveNode nd = a.nodes[t];
  const int n = a.n, rule = nd.rule;
  const double inf = __builtin_huge_val();
  DiveKey best = {inf, inf, 0.0, 0x7fffffff, 0};
  int cnt = 0;
  node_col_values(nd, n, [&](int j, double v) { dive_eval(a, rule, j, v, best, cnt); });
  for (int off = 32; off > 0; off >>= 1) {
    DiveKey o;
    o.k1 = __shfl_xor(best.k1, off, 64);
    o.k2 = __shfl_xor(best.k2, off, 64);
    o.v = __shfl_xor(best.v, off, 64);
    o.j = __shfl_xor(best.j, off, 64);
    o.dir = __shfl_xor(best.dir, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
    if (dive_before(o, best)) best = o;
  }
  const int lane = TIDX & 63, wv = TIDX >> 6;
  if (lane == 0) {
    s_k1[wv] = best.k1; s_k2[wv] = best.k2; s_v[wv] = best.v;
    s_j[wv] = best.j; s_dir[wv] = best.dir; s_cnt[wv] = cnt;
  }
  __syncthreads();
  if (TIDX == 0) {
    int total = s_cnt[0];
    for (int w = 1; w < 4; w++) {
      const DiveKey o = {s_k1[w], s_k2[w], s_v[w], s_j[w], s_dir[w]};
      total += s_cnt[w];
      if (dive_before(o, best)) best = o;
    }
    const bool any = best.j != 0x7fffffff;
    a.nfrac[t] = total;
    a.col[t] = any ? best.j : 0;
    a.dir[t] = any ? best.dir : 0;
    a.val[t] = any ? best.v : 0.0;
  }
}

void launch_divepick(const DiveArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_divepick, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_objrow
// Row 0 of many tableaux under a new objective (mvx_set_obj_many, DESIGN.md "Feasibility pump"): T[0][j] = base[j] + the sum
// over 64-row chunks, in chunk order, of the fma chain sum_i w[i] * T[i][j] over the chunk's rows in ascending order, rows of
// weight zero skipped -- the arithmetic of k_rowcomb_partial / k_rowcomb_final, without part[] and the second launch.  One
// workgroup per (64 columns, handle): a lane owns a column, the four waves take one chunk each, their partials meet in LDS
// and wave 0 adds them in chunk order.  Rows 1..m are only read and row 0 only written, so the workgroups of a handle do not
// depend on each other.
__global__ __launch_bounds__(256) void k_objrow(const ObjNode *nodes, int n) {
  __shared__ double s_part[4][OBJ_COLS];
  const ObjNode nd = nodes[blockIdx.y];
  const int lane = TIDX & 63, wv = TIDX >> 6;
  const int j = (int)blockIdx.x * OBJ_COLS + lane;
  const bool live = j <= n;
  const int m = nd.m;
  const size_t ld = (size_t)nd.ld;
  const int nchunks = (m + ROWCOMB_CHUNK - 1) / ROWCOMB_CHUNK;
  double out = (wv == 0 && live) ? nd.base[j] : 0.0;
  for (int g = 0; g < nchunks; g += 4) {
    const int ch = g + wv;
    double acc = 0.0;
    if (ch < nchunks && live) {
      const int i0 = 1 + ch * ROWCOMB_CHUNK;
      int i1 = i0 + ROWCOMB_CHUNK - 1;
      if (i1 > m) i1 = m;
      for (int i = i0; i <= i1; i++) {
        const double w = nd.w[i];
        if (w != 0.0) acc = fma(w, nd.T[(size_t)i * ld + j], acc);
      }
    }
    s_part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0) {
      const int k1 = nchunks - g < 4 ? nchunks - g : 4;
      for (int k = 0; k < k1; k++) out = out + s_part[k][lane];
    }
    __syncthreads();
  }
  if (wv == 0 && live) nd.T[j] = out;
}

void launch_objrow(const ObjNode *nodes, int n, int count, hipStream_t s) {
  hipLaunchKernelGGL(k_objrow, dim3((unsigned)((n + 1 + OBJ_COLS - 1) / OBJ_COLS), (unsigned)count), dim3(256), 0, s, nodes, n);
}

// ---------------------------------------------------------------------------- k_pumpobj
// The feasibility pump's rounding and distance objective (mvx_pump_obj_many, DESIGN.md "Feasibility pump"), one workgroup per
// solved handle.  The walk is k_divepick's -- a lane over the tableau rows takes a basic structural column's value from
// column 0 and its bounds from the row's bound arrays, a lane over the non-basic positions the bound the status names and
// the position's bounds -- and rounds the column on the spot.  A rounding that repeats the last one moves the (at most)
// PUMP_MOVES movable columns that lie farthest from their LP value, found by successive arg-max reductions under the strict
// total key (distance descending, column ascending): the result does not depend on the reduction tree.  Then the slopes, their
// count, and the objective; every operation is rounded on its own (-ffp-contract=off) and sqrt comes from the host's table, so
// the bits are the host twin's.  No atomics.
__device__ __forceinline__ int pump_block_sum(int x, int *s4) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  __syncthreads(); // the readers of the last sum are done with s4
  if ((TIDX & 63) == 0) s4[TIDX >> 6] = x;
  __syncthreads();
  return s4[0] + s4[1] + s4[2] + s4[3];
}

__global__ __launch_bounds__(256) void k_pumpobj(PumpArgs a) {
  __shared__ double s_sig[RND_NMAX + 1]; // the movable columns' distances, then the slopes
  __shared__ double s_bk[4];
  __shared__ int s_bj[4], s_sum[4], s_win;
  const int t = (int)blockIdx.x;
  const PumpNode nd = a.nodes[t];
  const int n = a.n, m = nd.m;
  const size_t o = (size_t)t * (size_t)(n + 1);
  double *v = a.v + o, *lo = a.lo + o, *hi = a.hi + o, *xt = a.xt + o, *c = a.c + o;
  const double *xp = a.xprev + o;
  int nfrac = 0, differs = 0;
  auto column = [&](int j, double vj, double l, double u) {
    double x = 0.0, L = 0.0, U = 0.0;
    if (a.flags[j] & RND_INT) {
      if (fabs(vj - rint(vj)) > 1e-9) nfrac++;
      L = ceil(l);
      U = floor(u);
      x = floor(vj + 0.5); // k_round's nearest integer
      if (x < L) x = L;
      if (x > U) x = U;
      if (nd.has_prev && x != xp[j]) differs = 1;
    }
    v[j] = vj; lo[j] = L; hi[j] = U; xt[j] = x;
  };
  for (int i = 1 + TIDX; i <= m; i += 256) {
    const int k = nd.bvar[i];
    if (k > m && k <= m + n) column(k - m, nd.T[(size_t)i * (size_t)nd.ld], nd.blb[i], nd.bub[i]);
  }
  for (int q = 1 + TIDX; q <= n; q += 256) {
    const int k = nd.nvar[q];
    if (k > m && k <= m + n) column(k - m, dev_nb_value(nd.nflag[q], nd.nlb[q], nd.nub[q]), nd.nlb[q], nd.nub[q]);
  }
  nfrac = pump_block_sum(nfrac, s_sum);
  differs = pump_block_sum(differs, s_sum);
  const bool stall = nd.has_prev && differs == 0;
  int moved = 0;
  if (stall) { // uniform over the workgroup
    for (int j = 1 + TIDX; j <= n; j += 256) {
      double sig = -1.0;
      if (a.flags[j] & RND_INT) {
        const double d = v[j] - xt[j], sd = fabs(d);
        if (sd > 0.0) {
          const double xn = xt[j] + (d > 0.0 ? 1.0 : -1.0);
          if (xn >= lo[j] && xn <= hi[j]) sig = sd;
        }
      }
      s_sig[j] = sig;
    }
    __syncthreads();
    for (int r = 0; r < PUMP_MOVES; r++) {
      double bk = 0.0;
      int bj = 0x7fffffff;
      for (int j = 1 + TIDX; j <= n; j += 256) {
        const double sg = s_sig[j];
        if (sg > 0.0 && (sg > bk || (sg == bk && j < bj))) {
          bk = sg;
          bj = j;
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ok = __shfl_xor(bk, off, 64);
        const int oj = __shfl_xor(bj, off, 64);
        if (ok > bk || (ok == bk && oj < bj)) {
          bk = ok;
          bj = oj;
        }
      }
      if ((TIDX & 63) == 0) {
        s_bk[TIDX >> 6] = bk;
        s_bj[TIDX >> 6] = bj;
      }
      __syncthreads();
      if (TIDX == 0) {
        for (int w = 1; w < 4; w++)
          if (s_bk[w] > bk || (s_bk[w] == bk && s_bj[w] < bj)) {
            bk = s_bk[w];
            bj = s_bj[w];
          }
        const int win = bj != 0x7fffffff ? bj : 0;
        if (win) {
          xt[win] = xt[win] + (v[win] - xt[win] > 0.0 ? 1.0 : -1.0);
          s_sig[win] = -1.0;
        }
        s_win = win;
      }
      __syncthreads();
      if (s_win == 0) break; // uniform
      moved++;
    }
    __syncthreads(); // xt of the moved columns, s_sig before it is reused
  }
  int nnz = 0;
  for (int j = 1 + TIDX; j <= n; j += 256) {
    double d = 0.0;
    if (a.flags[j] & RND_INT) {
      const double L = lo[j], U = hi[j], x = xt[j];
      if (L == U) d = 0.0;
      else if (x == L) d = 1.0;
      else if (x == U) d = -1.0;
      else {
        const double df = v[j] - x;
        d = df > 0.0 ? 1.0 : df < 0.0 ? -1.0 : 0.0;
      }
    }
    s_sig[j] = d;
    if (d != 0.0) nnz++;
  }
  nnz = pump_block_sum(nnz, s_sum);
  const double b = nd.q * a.sq[nnz];
  for (int j = 1 + TIDX; j <= n; j += 256) c[j] = (nd.a * (-nd.sg * s_sig[j])) + (b * a.c0[j]);
  if (TIDX == 0) {
    c[0] = 0.0;
    xt[0] = 0.0;
    int *info = a.info + 4 * (size_t)t;
    info[0] = nfrac;
    info[1] = moved;
    info[2] = (stall && moved == 0) ? 1 : 0;
    info[3] = nnz;
  }
}

void launch_pumpobj(const PumpArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_pumpobj, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_cutgram
// Scores of a round of candidate cuts (mvx_cut_scores, DESIGN.md "Root cut rounds"): dot[t] = sum_j v_tj x_j and the Gram matrix
// G[t][s] = sum_j v_tj v_sj, each sum over ascending j = 1..n from +0.0 with the product and the sum rounded separately -- the
// host's efficacy loop, bit for bit.  One workgroup per GRAM_TILE x GRAM_TILE block of pairs with block row <= block column, one
// lane per pair: the lane runs the whole serial sum of its pair, so nothing is reduced across lanes and there are no atomics.
// The two row groups of the block are staged in LDS GRAM_COLS columns at a time; a row is padded by one double, so the 16
// different rows a wave reads in one step fall on different banks (the row of the other operand is a broadcast).  A product
// commutes, so the lane's sum is G[s][t] too and the same lane writes the mirror entry; on a diagonal block only the lanes with
// t <= s write.  The lanes of the diagonal (t == s) also carry dot[t].
__global__ __launch_bounds__(GRAM_TILE *GRAM_TILE) void k_cutgram(CutGramArgs a) {
  if (blockIdx.y > blockIdx.x) return; // block row <= block column
  __shared__ double s_a[GRAM_TILE][GRAM_COLS + 1], s_b[GRAM_TILE][GRAM_COLS + 1], s_x[GRAM_COLS];
  const int ty = TIDX / GRAM_TILE, tx = TIDX % GRAM_TILE;
  const int t0 = (int)blockIdx.y * GRAM_TILE, s0 = (int)blockIdx.x * GRAM_TILE;
  const int t = t0 + ty, s = s0 + tx;
  const int n = a.n, k = a.k;
  const size_t row = (size_t)n + 1;
  const bool diag = t == s; // only on a diagonal block
  double acc = 0.0, dot = 0.0;
  for (int j0 = 1; j0 <= n; j0 += GRAM_COLS) {
    const int cnt = n - j0 + 1 < GRAM_COLS ? n - j0 + 1 : GRAM_COLS;
    __syncthreads(); // the last pass's readers are done
    for (int e = TIDX; e < GRAM_TILE * GRAM_COLS; e += GRAM_TILE * GRAM_TILE) {
      const int r = e / GRAM_COLS, c = e % GRAM_COLS; // a wave loads 64 consecutive doubles of one row
      const bool in = c < cnt;
      s_a[r][c] = (in && t0 + r < k) ? a.vals[(size_t)(t0 + r) * row + (size_t)(j0 + c)] : 0.0;
      s_b[r][c] = (in && s0 + r < k) ? a.vals[(size_t)(s0 + r) * row + (size_t)(j0 + c)] : 0.0;
    }
    if (TIDX < cnt) s_x[TIDX] = a.x[j0 + TIDX];
    __syncthreads();
    for (int c = 0; c < cnt; c++) {
      const double va = s_a[ty][c];
      acc = acc + va * s_b[tx][c];
      if (diag) dot = dot + va * s_x[c];
    }
  }
  if (t >= k || s >= k) return;
  if (blockIdx.y == blockIdx.x && t > s) return;
  a.gram[(size_t)t * (size_t)k + (size_t)s] = acc;
  if (t != s) a.gram[(size_t)s * (size_t)k + (size_t)t] = acc;
  else a.dot[t] = dot;
}

void launch_cutgram(const CutGramArgs &a, hipStream_t s) {
  const unsigned nt = (unsigned)((a.k + GRAM_TILE - 1) / GRAM_TILE);
  hipLaunchKernelGGL(k_cutgram, dim3(nt, nt), dim3(GRAM_TILE * GRAM_TILE), 0, s, a);
}

// ---------------------------------------------------------------------------- k_cutrows
// k dense rows appended to one tableau in one pass (mvx_add_cut_rows, DESIGN.md "Root cut rounds").  A row that is appended to a
// tableau is the combination base + sum_i w[i] T[i][.] of the rows whose basic variable is a structural column; the appended
// rows are basic auxiliaries themselves, so none of the k rows depends on another and all of them read rows 1..m only.  The
// arithmetic is k_rowcomb's, for every row: per 64-row chunk from row 1 an fma chain from +0.0 in ascending row order that
// skips zero weights, the chunk sums added onto the base in chunk order.  The t-th of k single appends sums ceil((m + t) / 64)
// chunks; those behind row m hold zero weights only and add +0.0, which turns a -0.0 into +0.0 and changes nothing else, so
// one more `+ 0.0` where extra[t] says so leaves the same bits.
// One workgroup per (256 columns, CUT_TILE rows): a lane owns a column and CUT_TILE accumulators, loads each T[i][j] once for
// all of them (coalesced), and reads the chunk's weights from LDS, where the workgroup gathers them from `vals` once per chunk
// (every lane reads the same word: a broadcast).  No partial buffer, no second launch.  The workgroups of the first tile row
// also do the bookkeeping of k_add_rows; they write bvar / nvar / blb / bub, which no workgroup of this kernel reads.
// The work of one workgroup: column tile blockIdx.x and row tile `ty` of the handle whose arguments are `a`.  k_cutrows calls
// it with its own arguments, k_cutrows_many with those of the handle its workgroup belongs to.
__device__ __forceinline__ void cutrows_tile(const CutRowsArgs &a, int ty, double (*s_w)[ROWCOMB_CHUNK]) {
  const int m = a.m, n = a.n, k = a.k;
  const size_t ld = (size_t)a.v.ld, row = (size_t)n + 1;
  const int t0 = ty * CUT_TILE;
  const int nt = k - t0 < CUT_TILE ? k - t0 : CUT_TILE;
  const int j = (int)blockIdx.x * 256 + TIDX;
  const bool live = j <= n;
  double out[CUT_TILE], acc[CUT_TILE];
  {
    const int col = live ? (j == 0 ? 0 : a.nbcol[j]) : 0;
#pragma unroll
    for (int c = 0; c < CUT_TILE; c++) out[c] = (live && c < nt && (j == 0 || col != 0)) ? a.vals[(size_t)(t0 + c) * row + (size_t)col] : 0.0;
  }
  const int nchunks = (m + ROWCOMB_CHUNK - 1) / ROWCOMB_CHUNK;
  for (int ch = 0; ch < nchunks; ch++) {
    const int i0 = 1 + ch * ROWCOMB_CHUNK;
    const int cnt = m - i0 + 1 < ROWCOMB_CHUNK ? m - i0 + 1 : ROWCOMB_CHUNK;
    __syncthreads(); // the last chunk's readers are done
    for (int e = TIDX; e < CUT_TILE * ROWCOMB_CHUNK; e += 256) {
      const int c = e / ROWCOMB_CHUNK, r = e % ROWCOMB_CHUNK;
      double w = 0.0;
      if (r < cnt && c < nt) {
        const int col = a.rowcol[i0 + r];
        if (col != 0) w = a.vals[(size_t)(t0 + c) * row + (size_t)col];
      }
      s_w[c][r] = w;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int c = 0; c < CUT_TILE; c++) acc[c] = 0.0;
      const double *Tj = a.v.T + (size_t)i0 * ld + (size_t)j;
      for (int r = 0; r < cnt; r++) {
        const double v = Tj[(size_t)r * ld];
#pragma unroll
        for (int c = 0; c < CUT_TILE; c++) {
          const double w = s_w[c][r];
          if (w != 0.0) acc[c] = fma(w, v, acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CUT_TILE; c++) out[c] = out[c] + acc[c];
    }
  }
  if (live) {
#pragma unroll
    for (int c = 0; c < CUT_TILE; c++)
      if (c < nt) {
        double o = out[c];
        if (a.extra[t0 + c]) o = o + 0.0;
        a.v.T[(size_t)(m + 1 + t0 + c) * ld + (size_t)j] = o;
      }
  }
  if (ty != 0) return;
  // k_add_rows, k times over: the structural variable numbers move up by k, the new rows hold their own auxiliaries
  const int span = (int)gridDim.x * 256;
  for (int g = j; g <= m || g <= n || g < k; g += span) {
    if (g >= 1 && g <= m && a.v.bvar[g] > m) a.v.bvar[g] += k;
    if (g >= 1 && g <= n && a.v.nvar[g] > m) a.v.nvar[g] += k;
    if (g < k) {
      a.v.bvar[m + 1 + g] = m + 1 + g;
      a.v.blb[m + 1 + g] = a.rowlb[g];
      a.v.bub[m + 1 + g] = INFINITY;
    }
  }
}

__global__ __launch_bounds__(256) void k_cutrows(CutRowsArgs a) {
  __shared__ double s_w[CUT_TILE][ROWCOMB_CHUNK];
  cutrows_tile(a, (int)blockIdx.y, s_w);
}

void launch_cutrows(const CutRowsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cutrows, dim3((unsigned)((a.n + 1 + 255) / 256), (unsigned)((a.k + CUT_TILE - 1) / CUT_TILE)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- shared by the live-edit kernels
// position q of a slab's per-position arrays as a freshly built handle has its padding
__device__ __forceinline__ void slab_pad(const SlabView &d, int q) {
  d.nvar[q] = 0;
  d.nflag[q] = MVX_NS;
  d.nlb[q] = 0.0;
  d.nub[q] = 0.0;
}
// The per-row and per-position arrays of a relayout, by one workgroup of THREADS threads: bvar / blb / bub of rows
// 0..rows_all-1 are carried over; position g <= kept of `d` takes position from(g) of `s` (from(0) == 0), positions from
// pad_from on take the padding, those between are the caller's.  renum rewrites the variable number of rows 1..m and of the
// positions behind 0.
template <int THREADS, class From, class Renum>
__device__ __forceinline__ void slab_carry_over(const SlabView &s, const SlabView &d, int tid, int rows_all, int m, int kept, int pad_from,
                                                From from, Renum renum) {
  for (int g = tid; g < rows_all; g += THREADS) {
    const int k = s.bvar[g];
    d.bvar[g] = (g >= 1 && g <= m) ? renum(k) : k;
    d.blb[g] = s.blb[g];
    d.bub[g] = s.bub[g];
  }
  for (int g = tid; g < d.ld; g += THREADS) {
    if (g <= kept) {
      const int q = from(g);
      d.nvar[g] = g ? renum(s.nvar[q]) : s.nvar[0];
      d.nflag[g] = s.nflag[q];
      d.nlb[g] = s.nlb[q];
      d.nub[g] = s.nub[q];
    } else if (g >= pad_from)
      slab_pad(d, g);
  }
}
// how many entries of the ascending list[0..cnt) lie below k
__device__ __forceinline__ int count_below(const int *list, int cnt, int k) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (list[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------- k_addcols
// k dense structural columns against one tableau in one pass (mvx_add_dense_cols, mvx_price_cols; DESIGN.md "Column append
// (add_cols)"): k_cutrows turned by 90 degrees.  The image of new column t in tableau row p is base + S, S the sum of
// w_q * T[p][q] over the non-basic positions q that hold an auxiliary i (w_q = -cols[t][i]).  The order of S is the definition's:
// 64 chains, chain l over q = l+1, l+65, ... ascending, each an fma chain from +0.0 that skips zero weights; the chains are
// combined by s[l] += s[l+h], h = 32 .. 1; the base is added last.  A chain is a lane: a wave owns ADDCOLS_RW rows and its lanes
// walk each of them with stride 64 (coalesced 512-byte reads), every lane holding one accumulator per (row, tile column) across
// the whole row, so the chains cost nothing and there is no second pass.  The weights of a tile of ADDCOLS_CT columns are gathered
// once per workgroup and chunk of ADDCOLS_CHUNK positions into LDS (nvar[q] -> cols[t][i], or zero: `cols` holds the columns of
// a tile side by side, so the weights of a position are one 32-byte read) and serve all ADDCOLS_WAVES * ADDCOLS_RW rows of the
// block; a chunk without a non-zero weight (positions that hold structurals only) is skipped by the whole workgroup.
// Pricing: grid (row blocks, tiles), the images go to img / dj.  Append: one workgroup carries ALL tiles of its rows, one after
// the other, because the shift of column 0 by the new columns' resting values (k_shift_nonbasic's fma, t ascending) needs the
// finished images of the row: lane 0 of the wave that owns the row keeps the running value.  On a relayout the same workgroups
// first write their rows of the new slab over its whole stride (old entries, zeros; the new columns follow), spare rows included.
// The blocks of row block 0 do the bookkeeping.  Reads (columns 1..n of s.T, bvar, nvar[1..n]) and writes (column 0, columns
// n+1..n+k, nvar[n+1..]) never meet, so no workgroup waits for another.
#define ADDCOLS_THREADS (64 * ADDCOLS_WAVES)
__global__ __launch_bounds__(ADDCOLS_THREADS) void k_addcols(AddColsArgs a) {
  __shared__ double s_w[ADDCOLS_CT][ADDCOLS_CHUNK];
  constexpr int RB = ADDCOLS_WAVES * ADDCOLS_RW;
  const int lane = TIDX & 63, wave = TIDX >> 6;
  const int m = a.m, n = a.n, k = a.k;
  const size_t lds = (size_t)a.s.ld, ldd = (size_t)a.d.ld, crow = (size_t)m + 1;
  const int rb0 = (int)blockIdx.x * RB;
  const bool append = a.d.T != nullptr;
  const bool relayout = append && a.d.T != a.s.T;
  if (append) {
    for (int r = 0; r < RB; r++) {
      const int p = rb0 + r;
      if (p >= a.rows_all) break;
      const bool img_row = p < a.rows;
      double *dst = a.d.T + (size_t)p * ldd;
      if (relayout) {
        const double *src = a.s.T + (size_t)p * lds;
        for (int j = TIDX; j < a.d.ld; j += ADDCOLS_THREADS) {
          if (j == 0 && img_row) continue; // the row's owner writes column 0 behind the shift
          if (j <= n) dst[j] = src[j];
          else if (j > n + k || !img_row) dst[j] = 0.0;
        }
      } else if (!img_row) {
        for (int j = n + 1 + TIDX; j <= n + k; j += ADDCOLS_THREADS) dst[j] = 0.0;
      }
    }
  }
  if (rb0 >= a.rows) return;
  const int p0 = rb0 + wave * ADDCOLS_RW;
  int nr = a.rows - p0;
  nr = nr < 0 ? 0 : (nr > ADDCOLS_RW ? ADDCOLS_RW : nr);
  double c0[ADDCOLS_RW];
  int hv[ADDCOLS_RW];
#pragma unroll
  for (int r = 0; r < ADDCOLS_RW; r++) {
    c0[r] = (append && lane == 0 && r < nr) ? a.s.T[(size_t)(p0 + r) * lds] : 0.0;
    hv[r] = (lane == 0 && r < nr && p0 + r >= 1) ? a.s.bvar[p0 + r] : 0;
  }
  for (int t0 = (int)blockIdx.y * ADDCOLS_CT; t0 < k; t0 += (int)gridDim.y * ADDCOLS_CT) {
    const int nt = k - t0 < ADDCOLS_CT ? k - t0 : ADDCOLS_CT;
    double acc[ADDCOLS_RW][ADDCOLS_CT];
#pragma unroll
    for (int r = 0; r < ADDCOLS_RW; r++)
#pragma unroll
      for (int c = 0; c < ADDCOLS_CT; c++) acc[r][c] = 0.0;
    // the weights of a chunk are gathered one chunk ahead, into registers: the two dependent loads (nvar[q], then cols[t][i])
    // are in flight while the rows of the chunk before are streamed
    const double *tile = a.cols + (size_t)(t0 / ADDCOLS_CT) * crow * ADDCOLS_CT; // [m+1][ADDCOLS_CT]
    double wn[ADDCOLS_CT];
    auto gather = [&](int q0) {
      const int q = q0 + TIDX; // ADDCOLS_CHUNK == workgroup size: one position per thread
      const int v = q <= n ? a.s.nvar[q] : m + 1;
#pragma unroll
      for (int c = 0; c < ADDCOLS_CT; c++) wn[c] = (c < nt && v <= m) ? -tile[(size_t)v * ADDCOLS_CT + c] : 0.0;
    };
    gather(1);
    for (int q0 = 1; q0 <= n; q0 += ADDCOLS_CHUNK) {
      __syncthreads(); // the last chunk's readers are done
      int nz = 0;
#pragma unroll
      for (int c = 0; c < ADDCOLS_CT; c++) {
        s_w[c][TIDX] = wn[c];
        nz |= (wn[c] != 0.0) ? 1 : 0;
      }
      const int any = __syncthreads_or(nz);
      if (q0 + ADDCOLS_CHUNK <= n) gather(q0 + ADDCOLS_CHUNK);
      if (!any) continue; // structurals only: nothing to add, for any row of the block
#pragma unroll
      for (int j = 0; j < ADDCOLS_CHUNK / 64; j++) {
        const int q = q0 + j * 64 + lane;
        double v[ADDCOLS_RW];
#pragma unroll
        for (int r = 0; r < ADDCOLS_RW; r++) v[r] = (q <= n && r < nr) ? a.s.T[(size_t)(p0 + r) * lds + (size_t)q] : 0.0;
#pragma unroll
        for (int c = 0; c < ADDCOLS_CT; c++) {
          const double w = s_w[c][j * 64 + lane];
          if (w != 0.0) {
#pragma unroll
            for (int r = 0; r < ADDCOLS_RW; r++) acc[r][c] = fma(w, v[r], acc[r][c]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < ADDCOLS_RW; r++) {
#pragma unroll
      for (int c = 0; c < ADDCOLS_CT; c++) {
        double s = acc[r][c];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) s = s + __shfl_down(s, h);
        if (lane == 0 && r < nr && c < nt) {
          const int p = p0 + r, t = t0 + c;
          double base;
          if (p == 0) base = a.obj[t];
          else base = hv[r] <= m ? tile[(size_t)hv[r] * ADDCOLS_CT + c] : 0.0;
          const double val = base + s;
          if (append) {
            a.d.T[(size_t)p * ldd + (size_t)(n + 1 + t)] = val;
            const double x = a.xs[t];
            if (x != 0.0) c0[r] = fma(val, x, c0[r]);
          } else {
            if (a.img) a.img[(size_t)t * crow + (size_t)p] = val;
            if (p == 0) a.dj[t] = val;
          }
        }
      }
    }
  }
  if (!append) return;
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ADDCOLS_RW; r++)
      if (r < nr) a.d.T[(size_t)(p0 + r) * ldd] = c0[r];
  }
  if (blockIdx.x != 0) return;
  for (int t = TIDX; t < k; t += ADDCOLS_THREADS) {
    a.d.nvar[n + 1 + t] = m + n + 1 + t;
    a.d.nflag[n + 1 + t] = a.nflag_new[t];
    a.d.nlb[n + 1 + t] = a.nlb_new[t];
    a.d.nub[n + 1 + t] = a.nub_new[t];
  }
  if (!relayout) return;
  slab_carry_over<ADDCOLS_THREADS>(a.s, a.d, TIDX, a.rows_all, m, n, n + k + 1, [](int g) { return g; }, [](int v) { return v; });
}

void launch_addcols(const AddColsArgs &a, hipStream_t s) {
  static_assert(ADDCOLS_CHUNK == ADDCOLS_THREADS, "k_addcols gathers one position per thread");
  constexpr int RB = ADDCOLS_WAVES * ADDCOLS_RW;
  const unsigned nrb = (unsigned)((a.rows_all + RB - 1) / RB);
  unsigned nty = 1;
  if (!a.d.T) { // pricing: the tiles are independent
    const int tiles = (a.k + ADDCOLS_CT - 1) / ADDCOLS_CT;
    nty = (unsigned)(tiles < 65535 ? tiles : 65535);
  }
  hipLaunchKernelGGL(k_addcols, dim3(nrb, nty), dim3(ADDCOLS_THREADS), 0, s, a);
}

// ---------------------------------------------------------------------------- k_pooly, k_poolprice, k_poolsel_*, k_poolgather
// Sifting over a device-resident column pool (mvx_pool_price, mvx_pool_append; DESIGN.md "Sifting (sift)").
// k_pooly: the row weights y_i = T[0][q] at the non-basic position q of auxiliary i, +0.0 where it is basic, zero up to ldp.
__global__ __launch_bounds__(256) void k_pooly(PoolPriceArgs a) {
  const int e = (int)blockIdx.x * 256 + TIDX; // entry e holds model row e + 1
  if (e >= a.ldp) return;
  const int q = e < a.m ? a.ypos[e + 1] : 0;
  a.y[e] = q ? a.T0[q] : 0.0;
}

// k_poolprice: d_j = obj_j + S_j for every pool column in one stream over the pool.  A wave owns a column: its 64 lanes are the
// 64 chains of the definition (lane l takes rows l+1, l+65, ... ascending, fma(-a_ij, y_i, acc) from +0.0, rows with y_i == 0
// skipped), every read is a 512-byte row of a contiguous column, and a lane has POOL_AHEAD loads in flight before the first
// fma.  The chains are combined by s[l] += s[l+h], h = 32 .. 1, in lane 0, which adds obj_j last and writes d_j and the column's
// selection key.  The weights stay in LDS for the whole launch (LDS_Y; beyond POOL_Y_LDS rows they are read through L2); the
// workgroups stride over the columns.  Below 64 rows most lanes idle: such a pool is small.
template <bool LDS_Y>
__global__ __launch_bounds__(64 * POOL_WAVES) void k_poolprice(PoolPriceArgs a) {
  extern __shared__ double s_y[];
  const int lane = TIDX & 63, wave = TIDX >> 6;
  const int ldp = a.ldp;
  if (LDS_Y) {
    for (int i = TIDX; i < ldp; i += 64 * POOL_WAVES) s_y[i] = a.y[i];
    __syncthreads();
  }
  for (int t = (int)blockIdx.x * POOL_WAVES + wave; t < a.N; t += (int)gridDim.x * POOL_WAVES) {
    const double *col = a.cols + (size_t)t * (size_t)ldp;
    double acc = 0.0;
    for (int i0 = lane; i0 < ldp; i0 += 64 * POOL_AHEAD) {
      double v[POOL_AHEAD];
#pragma unroll
      for (int u = 0; u < POOL_AHEAD; u++) v[u] = i0 + u * 64 < ldp ? col[i0 + u * 64] : 0.0;
#pragma unroll
      for (int u = 0; u < POOL_AHEAD; u++) {
        const int i = i0 + u * 64;
        const double yy = i < ldp ? (LDS_Y ? s_y[i] : a.y[i]) : 0.0;
        if (yy != 0.0) acc = fma(-v[u], yy, acc);
      }
    }
    double s = acc;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) s = s + __shfl_down(s, h);
    if (lane == 0) {
      const double d = a.obj[t] + s;
      const int f = a.flag[t];
      const double v = a.sgn * d;
      const bool att = f == MVX_NL ? v > a.tol : f == MVX_NU ? v < -a.tol : f == MVX_NF ? fabs(d) > a.tol : false;
      a.d[t + 1] = d;
      a.key[t + 1] = (att && !(a.skip && a.skip[t + 1])) ? (unsigned long long)__double_as_longlong(fabs(d)) : 0ULL;
    }
  }
}

// The selection: the K-th largest of the keys (bits of |d_j|, then N - j; a column that is not a candidate has no key) by a
// radix select, most significant byte first.  Launch p counts byte p of the keys that agree with the bytes chosen so far
// (integer counts in LDS, then in the launch's own global histogram: a count does not depend on the order of arrival); the
// next launch reads the finished histogram, chooses the byte that holds the rank still to find and carries on.  Every
// workgroup takes the same decision from the same numbers.  st = (low and high word of the bytes of |d|, the bytes of N - j,
// the rank still to find among the keys that agree).
__device__ __forceinline__ void poolsel_advance(const PoolPriceArgs &a, int p, unsigned long long &hi, unsigned &lo, int &kleft) {
  __shared__ int s_suf[POOLSEL_THREADS + 1];
  __shared__ int s_res[2];
  int *st = a.sel + POOLSEL_STATE;
  if (p == 1) {
    hi = 0;
    lo = 0;
    kleft = a.K;
  } else {
    hi = (unsigned long long)(unsigned)st[(p - 1) * 4] | ((unsigned long long)(unsigned)st[(p - 1) * 4 + 1] << 32);
    lo = (unsigned)st[(p - 1) * 4 + 2];
    kleft = st[(p - 1) * 4 + 3];
  }
  if (kleft > 0) { // uniform over the workgroup
    s_suf[TIDX] = a.sel[(p - 1) * 256 + TIDX];
    if (TIDX == 0) s_suf[POOLSEL_THREADS] = 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) { // s_suf[b] becomes the count of bytes >= b
      const int v = TIDX + off < 256 ? s_suf[TIDX + off] : 0;
      __syncthreads();
      s_suf[TIDX] += v;
      __syncthreads();
    }
    if (p == 1) { // every candidate was counted: the picks are min(K, #candidates)
      kleft = kleft < s_suf[0] ? kleft : s_suf[0];
      if (blockIdx.x == 0 && TIDX == 0) a.sel[POOLSEL_COUNT + 1] = kleft;
    }
    if (kleft > 0) {
      if (s_suf[TIDX] >= kleft && s_suf[TIDX + 1] < kleft) {
        s_res[0] = TIDX;
        s_res[1] = kleft - s_suf[TIDX + 1];
      }
      __syncthreads();
      const unsigned dgt = (unsigned)s_res[0];
      kleft = s_res[1];
      if (p - 1 < 8) hi |= (unsigned long long)dgt << (56 - 8 * (p - 1));
      else lo |= dgt << (24 - 8 * (p - 1 - 8));
    }
  }
  if (blockIdx.x == 0 && TIDX == 0) {
    st[p * 4] = (int)(unsigned)(hi & 0xffffffffULL);
    st[p * 4 + 1] = (int)(unsigned)(hi >> 32);
    st[p * 4 + 2] = (int)lo;
    st[p * 4 + 3] = kleft;
  }
}
// does (kh, kl) agree with the first p bytes of (hi, lo)?
__device__ __forceinline__ bool poolsel_agrees(int p, unsigned long long kh, unsigned kl, unsigned long long hi, unsigned lo) {
  if (p == 0) return true;
  if (p < 8) return (kh >> (64 - 8 * p)) == (hi >> (64 - 8 * p));
  if (kh != hi) return false;
  return p == 8 || (kl >> (32 - 8 * (p - 8))) == (lo >> (32 - 8 * (p - 8)));
}
__global__ __launch_bounds__(POOLSEL_THREADS) void k_poolsel_hist(PoolPriceArgs a, int p) {
  __shared__ int s_h[256];
  unsigned long long hi = 0;
  unsigned lo = 0;
  int kleft = a.K;
  if (p > 0) {
    poolsel_advance(a, p, hi, lo, kleft);
    if (kleft == 0) return; // no candidate at all
  }
  s_h[TIDX] = 0;
  __syncthreads();
  for (int j = 1 + (int)blockIdx.x * POOLSEL_THREADS + TIDX; j <= a.N; j += (int)gridDim.x * POOLSEL_THREADS) {
    const unsigned long long kh = a.key[j];
    if (!kh) continue;
    const unsigned kl = (unsigned)(a.N - j);
    if (!poolsel_agrees(p, kh, kl, hi, lo)) continue;
    const unsigned dgt = p < 8 ? (unsigned)(kh >> (56 - 8 * p)) & 255u : (kl >> (24 - 8 * (p - 8))) & 255u;
    atomicAdd(&s_h[dgt], 1);
  }
  __syncthreads();
  if (s_h[TIDX]) atomicAdd(&a.sel[p * 256 + TIDX], s_h[TIDX]);
}
// the columns whose key is at or above the K-th largest, in the order they arrive: k_poolsel_rank puts them in theirs
__global__ __launch_bounds__(POOLSEL_THREADS) void k_poolsel_emit(PoolPriceArgs a) {
  unsigned long long hi;
  unsigned lo;
  int kleft;
  poolsel_advance(a, POOLSEL_PASSES, hi, lo, kleft);
  if (kleft == 0) return;
  for (int j = 1 + (int)blockIdx.x * POOLSEL_THREADS + TIDX; j <= a.N; j += (int)gridDim.x * POOLSEL_THREADS) {
    const unsigned long long kh = a.key[j];
    if (!kh) continue;
    const unsigned kl = (unsigned)(a.N - j);
    if (kh > hi || (kh == hi && kl >= lo)) {
      const int slot = atomicAdd(&a.sel[POOLSEL_COUNT], 1);
      if (slot < a.K) {
        a.cand_key[slot] = kh;
        a.cand_j[slot] = j;
      }
    }
  }
}
// pick[1 + r] = the candidate with r candidates in front of it: larger |d|, or the same |d| and a lower column.  The keys are
// distinct, so every place is written once, whatever order the candidates arrived in.  The work grows with the square of the
// picks; they are a working set's worth, not a pool's
__global__ __launch_bounds__(POOLSEL_THREADS) void k_poolsel_rank(PoolPriceArgs a) {
  __shared__ unsigned long long s_k[POOLSEL_THREADS];
  __shared__ int s_j[POOLSEL_THREADS];
  const int np = a.sel[POOLSEL_COUNT + 1];
  if (blockIdx.x == 0 && TIDX == 0) a.pick[0] = np;
  if ((int)blockIdx.x * POOLSEL_THREADS >= np) return;
  const int t = (int)blockIdx.x * POOLSEL_THREADS + TIDX;
  const unsigned long long mk = t < np ? a.cand_key[t] : 0ULL;
  const int mj = t < np ? a.cand_j[t] : 0;
  int rank = 0;
  for (int s0 = 0; s0 < np; s0 += POOLSEL_THREADS) {
    __syncthreads();
    s_k[TIDX] = s0 + TIDX < np ? a.cand_key[s0 + TIDX] : 0ULL;
    s_j[TIDX] = s0 + TIDX < np ? a.cand_j[s0 + TIDX] : 0;
    __syncthreads();
    const int cnt = np - s0 < POOLSEL_THREADS ? np - s0 : POOLSEL_THREADS;
    for (int u = 0; u < cnt; u++) rank += (s_k[u] > mk || (s_k[u] == mk && s_j[u] < mj)) ? 1 : 0;
  }
  if (t < np) a.pick[1 + rank] = mj;
}

void launch_pool_price(const PoolPriceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_pooly, dim3((unsigned)(a.ldp > 0 ? (a.ldp + 255) / 256 : 1)), dim3(256), 0, s, a);
  const int nb = (a.N + POOL_WAVES - 1) / POOL_WAVES;
  const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
  if (a.ldp <= POOL_Y_LDS) hipLaunchKernelGGL(k_poolprice<true>, grid, dim3(64 * POOL_WAVES), (size_t)a.ldp * 8, s, a);
  else hipLaunchKernelGGL(k_poolprice<false>, grid, dim3(64 * POOL_WAVES), 0, s, a);
  if (a.K < 1) return;
  (void)hipMemsetAsync(a.sel, 0, (size_t)POOLSEL_INTS * 4, s);
  const int sb = (a.N + POOLSEL_THREADS - 1) / POOLSEL_THREADS;
  const dim3 sgrid((unsigned)(sb < 1024 ? sb : 1024));
  for (int p = 0; p < POOLSEL_PASSES; p++) hipLaunchKernelGGL(k_poolsel_hist, sgrid, dim3(POOLSEL_THREADS), 0, s, a, p);
  hipLaunchKernelGGL(k_poolsel_emit, sgrid, dim3(POOLSEL_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_poolsel_rank, dim3((unsigned)((a.K + POOLSEL_THREADS - 1) / POOLSEL_THREADS)), dim3(POOLSEL_THREADS), 0, s, a);
}

// k_poolgather: pool columns idx[0..k) into the layout k_addcols reads -- per tile of ADDCOLS_CT columns (m+1) rows of ADDCOLS_CT
// doubles, row 0 and the columns behind k zero -- so that an append from the pool sends no coefficient over the bus.  One
// workgroup per tile; a thread reads its row of the tile's columns (a coalesced read per column) and writes 32 bytes
__global__ __launch_bounds__(256) void k_poolgather(PoolGatherArgs a) {
  const int t0 = (int)blockIdx.x * ADDCOLS_CT;
  const double *src[ADDCOLS_CT];
#pragma unroll
  for (int c = 0; c < ADDCOLS_CT; c++) src[c] = t0 + c < a.k ? a.cols + (size_t)(a.idx[t0 + c] - 1) * (size_t)a.ldp : nullptr;
  double *tile = a.tiles + (size_t)blockIdx.x * ((size_t)a.m + 1) * ADDCOLS_CT;
  for (int i = TIDX; i <= a.m; i += 256) {
#pragma unroll
    for (int c = 0; c < ADDCOLS_CT; c++) tile[(size_t)i * ADDCOLS_CT + c] = (i >= 1 && src[c]) ? src[c][i - 1] : 0.0;
  }
}
void launch_pool_gather(const PoolGatherArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_poolgather, dim3((unsigned)((a.k + ADDCOLS_CT - 1) / ADDCOLS_CT)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- k_delcols
// Non-basic columns taken out of one tableau in one pass (mvx_del_cols; DESIGN.md "Column deletion (del_cols)"): k_addcols'
// counterpart.  A wave owns one row, DELC_WAVES rows per workgroup; the last workgroup of the grid owns no row and does the
// per-position and per-row arrays.  A wave reads only the uploaded lists (src, sh_pos / sh_negx, delc), never nvar / nflag,
// which that last workgroup rewrites in the same launch.
// Column 0 first: the row's chain T[p][0] = fma(T[p][q], -x_q, T[p][0]) over the deleted positions q with a non-zero resting
// value, ascending (the mirror of k_addcols' shift and of k_shift_nonbasic: a deleted variable counts as 0 from now on).  The
// chain reads positions the compaction overwrites, so it runs before any body store of the row; 64 of its operands are
// gathered at a time, one per lane, and every lane runs the same chain on them.
// Then the row closes up: destination first + t takes source src[t], in batches of 64 * DELC_BATCH destinations, ascending, all
// of a batch's loads in registers before its stores (coalesced 512-byte reads and writes).  Positions in front of `first` are
// not touched.  Why in place is safe: src[t] > first + t and src ascends, so the sources of a later batch lie strictly behind
// every destination stored so far -- a store never lands on an entry that is still to be loaded by a LATER batch.  Within a
// batch a store of one lane may land on the source of another lane, of the same or of another load of the batch, and no store
// depends on every load, so the compiler's own counted waits do not cover it: between the loads and the stores of a batch stands
// a full wait -- every memory counter at zero, then __syncthreads(), as delrows_wave has it for its basis arrays.  All waves of a
// workgroup run the same number of batches (a wave without a row loads and stores nothing), so the barrier is met by all.
// On a relayout source and destination are different slabs and ordering is no concern: the wave writes its row of the new slab
// over the whole stride -- kept entries, zero padding, and zeros in the rows behind row m.
// No atomics, no LDS, no hand-off between workgroups: a row has one owner, and the small arrays have one.
#define DELC_THREADS (64 * DELC_WAVES)
__device__ __forceinline__ int delc_renumber(int k, const int *delc, int ncs, int m) {
  return k <= m ? k : k - count_below(delc, ncs, k - m); // delc does not hold k - m
}
// every load of this wave has returned, and no lane of the workgroup goes on before all have got here
__device__ __forceinline__ void delc_full_wait() {
  __builtin_amdgcn_s_waitcnt(0); // vmcnt(0) expcnt(0) lgkmcnt(0)
  __syncthreads();
}

__global__ __launch_bounds__(DELC_THREADS) void k_delcols(DelColsArgs a) {
  constexpr int SPAN = 64 * DELC_BATCH;
  const int lane = TIDX & 63, wave = TIDX >> 6;
  const int m = a.m, first = a.first, nmove = a.nmove, n_old = a.n_old, ncs = a.ncs;
  const int n_new = first + nmove - 1;
  const bool relayout = a.d.T != a.s.T;
  if (blockIdx.x + 1 == gridDim.x) { // the small arrays
    const int tid = TIDX;
    if (!relayout) {
      for (int g = 1 + tid; g <= m; g += DELC_THREADS) a.d.bvar[g] = delc_renumber(a.s.bvar[g], a.delc, ncs, m);
      for (int q = 1 + tid; q < first; q += DELC_THREADS) a.d.nvar[q] = delc_renumber(a.s.nvar[q], a.delc, ncs, m);
      for (int t0 = 0; t0 < nmove; t0 += DELC_THREADS) {
        const int t = t0 + tid;
        int k = 0, fl = 0;
        double lb = 0.0, ub = 0.0;
        if (t < nmove) {
          const int s = a.src[t];
          k = a.s.nvar[s];
          fl = a.s.nflag[s];
          lb = a.s.nlb[s];
          ub = a.s.nub[s];
        }
        delc_full_wait(); // a destination may be another thread's source
        if (t < nmove) {
          a.d.nvar[first + t] = delc_renumber(k, a.delc, ncs, m);
          a.d.nflag[first + t] = fl;
          a.d.nlb[first + t] = lb;
          a.d.nub[first + t] = ub;
        }
      }
      delc_full_wait();
      for (int q = n_new + 1 + tid; q <= n_old; q += DELC_THREADS) slab_pad(a.d, q);
    } else {
      slab_carry_over<DELC_THREADS>(
          a.s, a.d, tid, a.rows_all, m, n_new, n_new + 1, [&](int g) { return g < first ? g : a.src[g - first]; },
          [&](int k) { return delc_renumber(k, a.delc, ncs, m); });
    }
    return;
  }
  const int p = (int)blockIdx.x * DELC_WAVES + wave;
  const bool live = p < a.rows_all; // wave-uniform
  const bool body = p <= m;         // rows 0..m; the rows behind them are spare (rows_all > m + 1)
  const double *S = a.s.T + (size_t)(live ? p : 0) * (size_t)a.s.ld;
  double *D = a.d.T + (size_t)(live ? p : 0) * (size_t)a.d.ld;
  double c0 = 0.0;
  if (body) {
    c0 = S[0];
    for (int s0 = 0; s0 < a.nsh; s0 += 64) {
      const int cnt = a.nsh - s0 < 64 ? a.nsh - s0 : 64;
      const int s = s0 + (lane < cnt ? lane : cnt - 1);
      const double v = S[a.sh_pos[s]], x = a.sh_negx[s];
      for (int i = 0; i < cnt; i++) c0 = fma(__shfl(v, i), __shfl(x, i), c0);
    }
  }
  if (relayout) {
    if (!live) return;
    if (!body) { // a row behind row m of the new slab: zeros
      for (int j = lane; j < a.d.ld; j += 64) D[j] = 0.0;
      return;
    }
    // the same batches: every load of a batch is issued before its first store, and none of them sits behind a branch (the
    // index is clamped to the kept positions, the padding takes its zero afterwards)
    for (int j0 = 0; j0 < a.d.ld; j0 += SPAN) {
      double v[DELC_BATCH];
#pragma unroll
      for (int b = 0; b < DELC_BATCH; b++) {
        const int j = j0 + b * 64 + lane;
        const int jj = j <= n_new ? j : n_new;
        int s = jj;
        if (nmove > 0) {
          const int t = jj - first;
          const int sm = a.src[t > 0 ? t : 0];
          s = t >= 0 ? sm : jj;
        }
        v[b] = S[s];
      }
#pragma unroll
      for (int b = 0; b < DELC_BATCH; b++) {
        const int j = j0 + b * 64 + lane;
        if (j < a.d.ld) D[j] = j == 0 ? c0 : (j <= n_new ? v[b] : 0.0);
      }
    }
    return;
  }
  for (int t0 = 0; t0 < nmove; t0 += SPAN) {
    double v[DELC_BATCH];
    if (live) {
#pragma unroll
      for (int b = 0; b < DELC_BATCH; b++) {
        const int t = t0 + b * 64 + lane;
        v[b] = S[a.src[t < nmove ? t : nmove - 1]]; // behind the last destination: a load nobody stores
      }
    }
    delc_full_wait();
    if (live) {
#pragma unroll
      for (int b = 0; b < DELC_BATCH; b++) {
        const int t = t0 + b * 64 + lane;
        if (t < nmove) D[first + t] = v[b];
      }
    }
  }
  delc_full_wait(); // the chain's loads and the last batch's: the zeros land on positions they read
  if (!live) return;
  for (int j = n_new + 1 + lane; j <= n_old; j += 64) D[j] = 0.0;
  if (body && lane == 0 && a.nsh > 0) D[0] = c0;
}

void launch_delcols(const DelColsArgs &a, hipStream_t s) {
  const unsigned nrb = (unsigned)((a.rows_all + DELC_WAVES - 1) / DELC_WAVES);
  hipLaunchKernelGGL(k_delcols, dim3(nrb + 1), dim3(DELC_THREADS), 0, s, a);
}

// ---------------------------------------------------------------------------- k_delrows
// Rows taken out of one tableau in place (mvx_del_rows, DESIGN.md "Cut purging (cut_purge)"): the kept rows behind the first
// removed one move towards lower indices, in their order, bit for bit.  A row may land where another kept row still waits to be
// read, so no two workgroups share a column: a workgroup is one wave and owns 64 columns (512 B of every row, coalesced), and
// walks the moved rows in ascending order, DEL_BATCH source rows loaded into registers before the batch is stored.  Within a
// wave that is safe: dst_t < src_t for every moved row and the sources ascend, so a store never lands on a row that is still
// to be loaded.  The map src[t] (the source of destination row first + t) is the same address in every lane: scalar loads.
// The rows the compaction vacates (behind the new row m) are zeroed, which is what k_update / k_fb / k_fbc3 assume of the spare
// rows they stream through.  The wave of the first column tile also moves bvar / blb / bub, 64 rows a step (every lane's load
// is done before any lane's store, a barrier stands between them; the same ordering argument), and rewrites the variable numbers of bvar and nvar:
// an auxiliary k becomes k - #{deleted < k}, a structural one moves down by the number of deleted rows.
// No atomics, no LDS, no hand-off between workgroups.
__device__ __forceinline__ int del_renumber(int k, const int *del, int nrs, int m_old) {
  return k > m_old ? k - nrs : k - count_below(del, nrs, k); // del does not hold k
}

// The work of one wave on one handle: the 64 columns of tile `tile`, and for tile 0 the basis arrays and the variable numbers.
// k_delrows calls it with its own arguments, k_delrows_many with those of the handle its workgroup belongs to.
__device__ __forceinline__ void delrows_wave(const DelRowsArgs &a, int tile, int lane) {
  const int j = tile * 64 + lane;
  const size_t ld = (size_t)a.v.ld;
  const int first = a.first, nmove = a.nmove;
  if (j < a.v.ld) {
    double *Tj = a.v.T + (size_t)j;
    int t0 = 0;
    for (; t0 + DEL_BATCH <= nmove; t0 += DEL_BATCH) {
      double v[DEL_BATCH];
#pragma unroll
      for (int b = 0; b < DEL_BATCH; b++) v[b] = Tj[(size_t)a.src[t0 + b] * ld];
#pragma unroll
      for (int b = 0; b < DEL_BATCH; b++) Tj[(size_t)(first + t0 + b) * ld] = v[b];
    }
    if (t0 < nmove) {
      const int nb = nmove - t0;
      double v[DEL_BATCH];
#pragma unroll
      for (int b = 0; b < DEL_BATCH; b++) v[b] = b < nb ? Tj[(size_t)a.src[t0 + b] * ld] : 0.0;
#pragma unroll
      for (int b = 0; b < DEL_BATCH; b++)
        if (b < nb) Tj[(size_t)(first + t0 + b) * ld] = v[b];
    }
    for (int i = first + nmove; i <= a.m_old; i++) Tj[(size_t)i * ld] = 0.0;
  }
  if (tile != 0) return;
  const int nrs = a.nrs, m_old = a.m_old;
  for (int i = 1 + lane; i < first; i += 64) a.v.bvar[i] = del_renumber(a.v.bvar[i], a.del, nrs, m_old);
  for (int t0 = 0; t0 < nmove; t0 += 64) {
    const int t = t0 + lane;
    int k = 0;
    double lb = 0.0, ub = 0.0;
    if (t < nmove) {
      const int s = a.src[t];
      k = a.v.bvar[s];
      lb = a.v.blb[s];
      ub = a.v.bub[s];
    }
    __syncthreads(); // every lane's loads of this step are done before any lane stores: a destination may be another lane's source
    if (t < nmove) {
      a.v.bvar[first + t] = del_renumber(k, a.del, nrs, m_old);
      a.v.blb[first + t] = lb;
      a.v.bub[first + t] = ub;
    }
  }
  for (int q = 1 + lane; q <= a.n; q += 64) a.v.nvar[q] = del_renumber(a.v.nvar[q], a.del, nrs, m_old);
}

__global__ __launch_bounds__(64) void k_delrows(DelRowsArgs a) { delrows_wave(a, (int)blockIdx.x, TIDX); }

void launch_delrows(const DelRowsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_delrows, dim3((unsigned)((a.v.ld + 63) / 64)), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------- k_delrows_many
// The same deletion on many handles in one launch (mvx_del_rows_many, DESIGN.md "Cut purging in the tree (node_purge)"): the
// grid is (column tiles of the widest handle, handles), a workgroup is one wave and owns 64 columns of ONE handle, which it
// treats exactly as k_delrows treats them (delrows_wave).  hs[blockIdx.y] is the handle's descriptor -- k_delrows' arguments,
// its src and del lists in the uploaded block that holds the descriptors too -- read at one address by the whole wave, and
// copied once: delrows_wave stores through pointers the compiler cannot tell from hs.  (The lists are reached through pointers
// out of memory here, so their entries are vector loads of one address where k_delrows has scalar loads.)  Handles
// differ in m, in ld and in how many rows move: a workgroup whose tile lies beyond its handle's ld, or whose handle has nothing
// to delete, returns at once (the whole wave, so the barrier in delrows_wave is met by all or by none).  Handles own disjoint
// slabs, and within a handle no two workgroups share a column: no atomics, no LDS, no hand-off between workgroups.
__global__ __launch_bounds__(64) void k_delrows_many(const DelRowsArgs *__restrict__ hs) {
  const DelRowsArgs a = hs[blockIdx.y];
  const int tile = (int)blockIdx.x;
  if (a.nrs <= 0 || tile * 64 >= a.v.ld) return;
  delrows_wave(a, tile, TIDX);
}

void launch_delrows_many(const DelRowsArgs *hs, int handles, int max_ld, hipStream_t s) {
  hipLaunchKernelGGL(k_delrows_many, dim3((unsigned)((max_ld + 63) / 64), (unsigned)handles), dim3(64), 0, s, hs);
}

// ---------------------------------------------------------------------------- k_cutrows_many
// The same append on many handles in one launch (mvx_add_cut_rows_many, DESIGN.md "Row append across handles
// (add_cut_rows_many)"): blockIdx.x is the 256-column tile (all handles have n columns), tile_base + blockIdx.y a row tile of
// the launch's flattened index over all handles, CUT_TILE new rows of ONE handle, which the workgroup treats exactly as k_cutrows
// treats them (cutrows_tile).  tile0s[h] is the first tile of handle h, ascending and strictly so (every handle of the launch
// has rows): the workgroup's handle is the last one whose first tile is not behind its own, found with count_below.  The
// descriptors are reached by pointer and hs[h] is read at one address by the whole workgroup; its pieces are offsets into the
// uploaded block `base`, which holds the descriptors too.  It is copied once: cutrows_tile stores through pointers the compiler
// cannot tell from hs.  The first tile of each handle does that handle's bookkeeping, which no workgroup of the launch reads
// (the structural lists come up with the call).  Handles own disjoint slabs, and within a handle a workgroup owns its 256
// columns of its CUT_TILE new rows: no atomics, no hand-off between workgroups.
__global__ __launch_bounds__(256) void k_cutrows_many(const CutRowsHandle *__restrict__ hs, const int *__restrict__ tile0s, int handles,
                                                      const unsigned char *__restrict__ base, int n, int tile_base) {
  __shared__ double s_w[CUT_TILE][ROWCOMB_CHUNK];
  const int tile = tile_base + (int)blockIdx.y;
  const int h = count_below(tile0s, handles, tile + 1) - 1; // tile0s[0] == 0: h >= 0
  const CutRowsHandle d = hs[h];
  CutRowsArgs a;
  a.v = d.v;
  a.vals = (const double *)(base + d.o_vals);
  a.rowcol = (const int *)(base + d.o_rowcol);
  a.nbcol = (const int *)(base + d.o_nbcol);
  a.rowlb = (const double *)(base + d.o_rowlb);
  a.extra = (const int *)(base + d.o_extra);
  a.m = d.m; a.n = n; a.k = d.k;
  const int ty = tile - d.tile0;
  if (ty * CUT_TILE >= d.k) return; // not reached: the tiles of a launch are those of its handles
  cutrows_tile(a, ty, s_w);
}

void launch_cutrows_many(const CutRowsHandle *hs, const int *tile0s, int handles, const unsigned char *base, int n, int tile_base, int ntiles,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_cutrows_many, dim3((unsigned)((n + 1 + 255) / 256), (unsigned)ntiles), dim3(256), 0, s, hs, tile0s, handles, base, n,
                     tile_base);
}

// ---------------------------------------------------------------------------- k_conflict_rows / k_conflict
// The conflict graph of a handle's binary columns (mvx_conflict_graph, DESIGN.md "Clique cuts (cut_families)"), two launches.
// k_conflict_rows, rows on lanes: the activities of a row at the handle's bounds, phase A of k_prop word for word (the by-column
// model, a wave reads one column of consecutive rows; the bounds are the same address in every lane), and what a side needs to
// speak: Lmin and rub + tol(rub) where kmin = 0 and rub is finite, else +inf, which no sum exceeds; the mirror with -inf.
__global__ __launch_bounds__(256) void k_conflict_rows(ConflictArgs a) {
  const int i = (int)blockIdx.x * 256 + TIDX;
  if (i >= a.m0) return;
  const int n = a.n;
  const size_t ldm = (size_t)a.ldm;
  double lmin = 0.0, lmax = 0.0;
  int kmin = 0, kmax = 0;
  for (int j = 1; j <= n; j++) {
    const double v = a.At[(size_t)j * ldm + i];
    if (v == 0.0) continue;
    const double l = a.clo[j], u = a.chi[j];
    const double bmin = v > 0.0 ? l : u, bmax = v > 0.0 ? u : l;
    if (isinf(bmin)) kmin++;
    else lmin = __dadd_rn(lmin, __dmul_rn(v, bmin));
    if (isinf(bmax)) kmax++;
    else lmax = __dadd_rn(lmax, __dmul_rn(v, bmax));
  }
  const double lo = a.rlo[i], hi = a.rhi[i];
  double *out = a.rowinfo + 4 * (size_t)i;
  out[0] = lmin;
  out[1] = (kmin == 0 && isfinite(hi)) ? __dadd_rn(hi, rnd_tol(hi)) : INFINITY;
  out[2] = lmax;
  out[3] = (kmax == 0 && isfinite(lo)) ? __dsub_rn(lo, rnd_tol(lo)) : -INFINITY;
}

// k_conflict: a wave owns one column j and one 64-bit word of its adjacency row, a lane the column k = 64 w + lane.  Per row
// the wave reads a_ij through one address (a scalar load) and skips the row when it is zero or its side says nothing: both
// branches are uniform, which is how a sparse row costs nothing.  Otherwise the lanes read Ar[i][k] coalesced (the row stride
// is 64 W, so k stays inside the row and the padding reads as zero) and test (L + a_lower) + a_higher against the threshold, the
// lower column's coefficient first: wave k's lane j adds the same numbers in the same order, so the relation is symmetric
// without a second write.  The word is the ballot of the lanes' flags, written by lane 0.  No atomics, no LDS, no reduction.
__global__ __launch_bounds__(64 * CONF_WAVES) void k_conflict(ConflictArgs a) {
  const int j = (int)blockIdx.x; // 0..n
  const int w = (int)blockIdx.y * CONF_WAVES + __builtin_amdgcn_readfirstlane(TIDX >> 6);
  if (w >= a.W) return;
  const int lane = TIDX & 63, k = w * 64 + lane;
  const int n = a.n, m0 = a.m0;
  const size_t ldn = (size_t)a.ldn;
  bool flag = false;
  if (j >= 1 && (a.flags[j] & RND_INT) && a.clo[j] == 0.0 && a.chi[j] == 1.0) {
    const bool kB = k >= 1 && k <= n && k != j && (a.flags[k] & RND_INT) && a.clo[k] == 0.0 && a.chi[k] == 1.0;
    const bool jlow = j < k;
    for (int i = 0; i < m0; i++) {
      const double aj = a.Ar[(size_t)i * ldn + (size_t)j];
      if (aj == 0.0) continue;
      const double *info = a.rowinfo + 4 * (size_t)i;
      if (aj > 0.0) {
        const double thr = info[1];
        if (thr == INFINITY) continue;
        const double L = info[0], ak = a.Ar[(size_t)i * ldn + (size_t)k];
        const double s = jlow ? __dadd_rn(__dadd_rn(L, aj), ak) : __dadd_rn(__dadd_rn(L, ak), aj);
        flag = flag || (ak > 0.0 && s > thr);
      } else {
        const double thr = info[3];
        if (thr == -INFINITY) continue;
        const double L = info[2], ak = a.Ar[(size_t)i * ldn + (size_t)k];
        const double s = jlow ? __dadd_rn(__dadd_rn(L, aj), ak) : __dadd_rn(__dadd_rn(L, ak), aj);
        flag = flag || (ak < 0.0 && s < thr);
      }
    }
    flag = flag && kB;
  }
  const unsigned long long word = __ballot(flag);
  if (lane == 0) a.adj[(size_t)j * (size_t)a.W + (size_t)w] = word;
}

void launch_conflict(const ConflictArgs &a, hipStream_t s) {
  if (a.m0 > 0) hipLaunchKernelGGL(k_conflict_rows, dim3((unsigned)((a.m0 + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_conflict, dim3((unsigned)(a.n + 1), (unsigned)((a.W + CONF_WAVES - 1) / CONF_WAVES)), dim3(64 * CONF_WAVES), 0, s, a);
}

// ---------------------------------------------------------------------------- k_cliquemembers / k_cliquesep
// Clique separation in the tree (mvx_clique_cuts_many, DESIGN.md "Clique cuts in the tree (node_cliques)"): the separation of
// mvx_bnb_clique_cuts for a window of solved handles against the root's conflict graph, which stays on the device.
// k_cliquemembers, once per graph: the columns whose adjacency row is not empty, a thread per column.
__global__ __launch_bounds__(256) void k_cliquemembers(const unsigned long long *adj, int *member, int n, int W) {
  const int j = (int)blockIdx.x * 256 + TIDX;
  if (j > n) return;
  unsigned long long any = 0ull;
  for (int w = 0; w < W; w++) any |= adj[(size_t)j * (size_t)W + (size_t)w];
  member[j] = (j >= 1 && any != 0ull) ? 1 : 0;
}

// k_cliquesep, one workgroup per handle.
//  1. the node LP's column values (node_col_values: get_col_prim's bits) into LDS;
//  2. the member columns sorted by value descending, column ascending (k_round's bitonic sort in LDS; the others sink behind
//     them with a key of -inf); the seeds are the prefix of that order with x > 1e-6;
//  3. a wave owns one seed: lane l holds words l and 64 + l of the mask (W <= 128) and of the set Q.  It walks the whole order;
//     the column's mask bit comes from its owner by a lane broadcast, and on a hit mask &= adj[column] is one coalesced load.
//     Once the mask is empty nothing can join any more and the walk ends: the same set as the full walk;
//  4. the CLQ_WAVES waves take the next seeds of the order together and leave their sets in LDS; wave 0 then takes them in seed
//     order: s over ascending columns from +0.0, the test s - 1 > 1e-6, the comparison with the sets already kept, the cap.
// What is kept depends on the seed order only, not on which wave grew which seed.  No atomics, no LDS reduction of doubles,
// nothing shared between workgroups; every loop is bounded by n, W or max_cuts.
static_assert(64 * CLQ_WAVES == 256, "node_col_values walks with 256 threads");
__global__ __launch_bounds__(64 * CLQ_WAVES) void k_cliquesep(CliqueArgs a) {
  __shared__ double s_x[RND_NMAX + 1];
  __shared__ double s_key[RND_NMAX];
  __shared__ int s_idx[RND_NMAX];
  __shared__ unsigned long long s_q[CLQ_WAVES][128];
  __shared__ int s_part[2][CLQ_WAVES];
  __shared__ int s_kept;
  const int t = (int)blockIdx.x;
  const NodeRef nd = a.nodes[t];
  const int n = a.n, W = a.W, max_cuts = a.max_cuts;
  const int lane = TIDX & 63, wv = __builtin_amdgcn_readfirstlane(TIDX >> 6);
  const double inf = __builtin_huge_val();
  if (TIDX == 0) s_kept = 0;
  node_col_values(nd, n, [&](int j, double v) { s_x[j] = v; });
  __syncthreads();
  int np = 1;
  while (np < n) np <<= 1;
  int mem = 0, pos = 0;
  for (int j = 1 + TIDX; j <= n; j += 256) {
    const bool in = a.member[j] != 0;
    const double v = s_x[j];
    s_key[j - 1] = in ? v : -inf;
    s_idx[j - 1] = j;
    mem += in ? 1 : 0;
    pos += (in && v > 1e-6) ? 1 : 0;
  }
  for (int p = n + TIDX; p < np; p += 256) {
    s_key[p] = -inf;
    s_idx[p] = 0x7fffffff;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mem += __shfl_xor(mem, off, 64);
    pos += __shfl_xor(pos, off, 64);
  }
  if (lane == 0) {
    s_part[0][wv] = mem;
    s_part[1][wv] = pos;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= np; k2 <<= 1)
    for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
      for (int i = TIDX; i < np; i += 256) {
        const int l = i ^ jj;
        if (l <= i) continue;
        const double ki = s_key[i], kl = s_key[l];
        const int ii = s_idx[i], il = s_idx[l];
        const bool sw = ((i & k2) == 0) ? rnd_before(kl, il, ki, ii) : rnd_before(ki, ii, kl, il);
        if (sw) {
          s_key[i] = kl; s_key[l] = ki;
          s_idx[i] = il; s_idx[l] = ii;
        }
      }
      __syncthreads();
    }
  int no = 0, ns = 0; // members (the order's length) and seeds (its prefix)
  for (int w = 0; w < CLQ_WAVES; w++) {
    no += s_part[0][w];
    ns += s_part[1][w];
  }
  unsigned long long *qo = a.q + (size_t)t * (size_t)max_cuts * (size_t)W;
  double *so = a.sum + (size_t)t * (size_t)max_cuts;
  const bool has0 = lane < W, has1 = 64 + lane < W;
  for (int b0 = 0; b0 < ns; b0 += CLQ_WAVES) {
    const int k = b0 + wv;
    if (k < ns) {
      const int seed = s_idx[k];
      const unsigned long long *rs = a.adj + (size_t)seed * (size_t)W;
      unsigned long long m0 = has0 ? rs[lane] : 0ull, m1 = has1 ? rs[64 + lane] : 0ull;
      unsigned long long q0 = 0ull, q1 = 0ull;
      if (lane == ((seed >> 6) & 63)) {
        if ((seed >> 6) < 64) q0 |= 1ull << (seed & 63);
        else q1 |= 1ull << (seed & 63);
      }
      for (int p = 0; p < no; p++) {
        const int c = s_idx[p];
        const int wd = c >> 6;
        const unsigned long long word = __shfl(wd < 64 ? m0 : m1, wd & 63, 64);
        if (!((word >> (c & 63)) & 1ull)) continue;
        const unsigned long long *rc = a.adj + (size_t)c * (size_t)W;
        m0 &= has0 ? rc[lane] : 0ull;
        m1 &= has1 ? rc[64 + lane] : 0ull;
        if (lane == (wd & 63)) {
          if (wd < 64) q0 |= 1ull << (c & 63);
          else q1 |= 1ull << (c & 63);
        }
        if (__ballot((m0 | m1) != 0ull) == 0ull) break;
      }
      s_q[wv][lane] = q0;
      s_q[wv][64 + lane] = q1;
    }
    __syncthreads();
    if (wv == 0) {
      int kept = s_kept;
      for (int u = 0; u < CLQ_WAVES && b0 + u < ns && kept < max_cuts; u++) {
        double s = 0.0;
        for (int w = 0; w < W; w++) {
          unsigned long long mk = s_q[u][w];
          while (mk) {
            const int b = __builtin_ctzll(mk);
            mk &= mk - 1ull;
            s = __dadd_rn(s, s_x[64 * w + b]);
          }
        }
        if (!(__dsub_rn(s, 1.0) > 1e-6)) continue;
        const unsigned long long q0 = s_q[u][lane], q1 = s_q[u][64 + lane];
        bool dup = false;
        for (int e = 0; e < kept && !dup; e++) {
          const unsigned long long *qe = qo + (size_t)e * (size_t)W;
          const bool same = (!has0 || qe[lane] == q0) && (!has1 || qe[64 + lane] == q1);
          dup = __ballot(!same) == 0ull;
        }
        if (dup) continue;
        unsigned long long *qk = qo + (size_t)kept * (size_t)W;
        if (has0) qk[lane] = q0;
        if (has1) qk[64 + lane] = q1;
        if (lane == 0) so[kept] = s;
        kept++;
      }
      if (lane == 0) s_kept = kept;
    }
    __syncthreads();
    if (s_kept >= max_cuts) break;
  }
  if (TIDX == 0) a.cnt[t] = s_kept;
}

void launch_clique_members(const unsigned long long *adj, int *member, int n, int W, hipStream_t s) {
  hipLaunchKernelGGL(k_cliquemembers, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, adj, member, n, W);
}
void launch_cliquesep(const CliqueArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cliquesep, dim3((unsigned)a.count), dim3(64 * CLQ_WAVES), 0, s, a);
}

// ---------------------------------------------------------------------------- k_lsact / k_lsmove / k_lsapply
// Incumbent polishing (mvx_polish_many, DESIGN.md "Incumbent polishing (polish)"): a best-improvement search over one- and
// two-column unit moves from a feasible point.  A candidate is (gain, key); the greater gain wins, and on equal gains the
// lower key: a single before a pair, then the lower index(u), then the lower index(v).
__device__ __forceinline__ bool ls_better(double ga, unsigned long long ka, double gb, unsigned long long kb) {
  return ga > gb || (ga == gb && ka < kb);
}
__device__ __forceinline__ void ls_wave_best(double &g, unsigned long long &k) {
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_xor(g, off, 64);
    const unsigned kl = (unsigned)k, kh = (unsigned)(k >> 32);
    const unsigned long long ok = ((unsigned long long)(unsigned)__shfl_xor((int)kh, off, 64) << 32) | (unsigned)__shfl_xor((int)kl, off, 64);
    if (ls_better(og, ok, g, k)) {
      g = og;
      k = ok;
    }
  }
}
__device__ __forceinline__ bool ls_inside(double t, double lo_t, double hi_t) { return t >= lo_t && t <= hi_t; }

// k_lsact, one workgroup per point.  final = 0, the entry: integer columns take rint(x) when they are within 1e-9 of it, the
// activities are summed as k_round sums them (a row per lane, ascending columns, zero values skipped) and the point is refused
// (ok = 0, done = 1) when an integer column is fractional or the rounding heuristic's check fails.  final = 1, the end: the
// same sums and check on the point the moves left; where it fails the entry point returns with moves = 0.  The objective is
// k_round's, by one wave over the products in order.
__global__ __launch_bounds__(256) void k_lsact(LsArgs a, int final) {
  __shared__ int s_bad;
  const int p = (int)blockIdx.x;
  if (final && !a.ok[p]) return;
  const int n = a.n, m0 = a.m0;
  const size_t ldm = (size_t)a.ldm;
  const double *xin = a.xin + (size_t)p * (size_t)(n + 1);
  double *x = a.x + (size_t)p * (size_t)(n + 1);
  double *r = a.r + (size_t)p * ldm;
  const int lane = TIDX & 63;
  if (TIDX == 0) s_bad = 0;
  __syncthreads();
  bool bad = false;
  for (int j = 1 + TIDX; j <= n; j += 256) {
    double v;
    if (final) {
      v = x[j];
    } else {
      v = xin[j];
      if (a.flags[j] & RND_INT) {
        const double ri = rint(v);
        if (fabs(v - ri) <= 1e-9) v = ri;
        else bad = true;
      }
      x[j] = v;
    }
    bad = bad || !(a.clo[j] <= v && v <= a.chi[j]);
  }
  __syncthreads(); // x is read below by every lane
  for (int i = TIDX; i < m0; i += 256) {
    double acc = 0.0;
    for (int j = 1; j <= n; j++) {
      const double xj = x[j];
      if (xj != 0.0) acc = __dadd_rn(acc, __dmul_rn(a.At[(size_t)j * ldm + i], xj));
    }
    r[i] = acc;
    const double lo = a.rlo[i], hi = a.rhi[i];
    bad = bad || !(acc >= lo - rnd_tol(lo) && acc <= hi + rnd_tol(hi));
  }
  if (bad) s_bad = 1;
  __syncthreads();
  const bool refused = s_bad != 0;
  if (final && refused) { // a tolerance edge: the entry point comes back
    for (int j = 1 + TIDX; j <= n; j += 256) x[j] = (a.flags[j] & RND_INT) ? rint(xin[j]) : xin[j];
    if (TIDX == 0) {
      a.obj[p] = a.obj0[p];
      a.moves[p] = 0;
    }
    return;
  }
  if (TIDX < 64) {
    double s = 0.0;
    for (int j0 = 1; j0 <= n; j0 += 64) {
      const int j = j0 + lane;
      const double pr = j <= n ? __dmul_rn(a.c[j], x[j]) : 0.0;
      unsigned long long mk = __ballot(pr != 0.0);
      while (mk) {
        const int b = __builtin_ctzll(mk);
        mk &= mk - 1ull;
        s = __dadd_rn(s, __shfl(pr, b, 64));
      }
    }
    if (lane == 0) {
      const double o = refused ? 0.0 : __dadd_rn(s, a.c[0]);
      a.obj[p] = o;
      if (!final) {
        a.obj0[p] = o;
        a.moves[p] = 0;
        a.ok[p] = refused ? 0 : 1;
        a.done[p] = refused ? 1 : 0;
      }
    }
  }
}

// k_lsmove, one iteration's evaluation: a workgroup owns one unit move u = (j, du) of one point, its four waves the words of
// partner columns from j's own word on, a lane the column k = 64 w + lane > j with both signs.  Per row the wave reads a_ij and
// r_i through one address and Ar[i][k] coalesced (the row stride is 64 W: k stays inside the row, the padding reads as zero),
// and tests t = (r_i + du a_ij) +- a_ik against the row's bounds.  Every row is tested, not only those with a non-zero: r_i
// itself lies within the bounds, and adding a zero leaves it as it is.  A wave leaves a word as soon as no lane has a candidate
// left (a uniform branch), and never starts on a word none of whose lanes can beat what it holds.  The first wave carries the
// single move u along: its test value is the inner sum.  The workgroup's best candidate goes to rec[point][u].
__global__ __launch_bounds__(256) void k_lsmove(LsArgs a) {
  __shared__ double s_g[4];
  __shared__ unsigned long long s_k[4];
  const int p = (int)blockIdx.y;
  if (a.done[p]) return;
  const int u = (int)blockIdx.x;
  const int n = a.n, m0 = a.m0;
  const int j = (u >> 1) + 1;
  const bool neg = (u & 1) != 0;
  const double du = neg ? -1.0 : 1.0;
  const size_t ldn = (size_t)a.ldn;
  const double *x = a.x + (size_t)p * (size_t)(n + 1);
  const double *r = a.r + (size_t)p * (size_t)a.ldm;
  LsRec *out = a.rec + (size_t)p * (size_t)(2 * n) + (size_t)u;
  const double xj = x[j];
  const bool adm = (a.flags[j] & RND_INT) && (xj + du >= ceil(a.clo[j])) && (xj + du <= floor(a.chi[j]));
  if (!adm) {
    if (TIDX == 0) {
      out->gain = 0.0;
      out->key = ~0ull;
    }
    return;
  }
  const double cj = a.c[j];
  const double gu = a.sg * (neg ? -cj : cj);
  const int wave = __builtin_amdgcn_readfirstlane(TIDX >> 6), lane = TIDX & 63;
  const int W = a.ldn >> 6;
  const unsigned long long ukey = (unsigned long long)u << 31;
  double bg = 0.0; // the lane's best: only a gain above 0 counts
  unsigned long long bk = ~0ull;
  bool first = wave == 0; // the single rides with the first word of the first wave
  for (int w = (j >> 6) + wave; w < W; w += 4) { // j <= n < 64 W: the first wave always has a word
    const int k = w * 64 + lane;
    const bool kint = k > j && k <= n && (a.flags[k] & RND_INT);
    double gp = 0.0, gm = 0.0;
    bool ap = false, am = false;
    if (kint) {
      const double xk = x[k], ck = a.c[k];
      gp = __dadd_rn(gu, a.sg * ck);
      gm = __dadd_rn(gu, a.sg * -ck);
      ap = xk + 1.0 <= floor(a.chi[k]) && xk + 1.0 >= ceil(a.clo[k]) && gp > bg;
      am = xk - 1.0 >= ceil(a.clo[k]) && xk - 1.0 <= floor(a.chi[k]) && gm > bg;
    }
    bool sa = first && gu > 0.0;
    if (__any(ap || am) || sa) {
      for (int i = 0; i < m0; i++) {
        const double aj = a.Ar[(size_t)i * ldn + (size_t)j];
        const double lo = a.rlo[i], hi = a.rhi[i];
        const double lo_t = __dsub_rn(lo, rnd_tol(lo)), hi_t = __dadd_rn(hi, rnd_tol(hi));
        const double s = __dadd_rn(r[i], neg ? -aj : aj);
        sa = sa && ls_inside(s, lo_t, hi_t);
        const double ak = a.Ar[(size_t)i * ldn + (size_t)k];
        ap = ap && ls_inside(__dadd_rn(s, ak), lo_t, hi_t);
        am = am && ls_inside(__dadd_rn(s, -ak), lo_t, hi_t);
        if (!(__any(ap || am) || sa)) break;
      }
    }
    // within a lane a later word has the higher index(v): it must be strictly better
    if (ap && gp > bg) {
      bg = gp;
      bk = (1ull << 62) | ukey | (unsigned long long)(2 * (k - 1));
    }
    if (am && gm > bg) {
      bg = gm;
      bk = (1ull << 62) | ukey | (unsigned long long)(2 * (k - 1) + 1);
    }
    if (sa && lane == 0 && ls_better(gu, ukey, bg, bk)) {
      bg = gu;
      bk = ukey;
    }
    first = false;
  }
  ls_wave_best(bg, bk);
  if (lane == 0) {
    s_g[wave] = bg;
    s_k[wave] = bk;
  }
  __syncthreads();
  if (TIDX == 0) {
    for (int q = 1; q < 4; q++)
      if (ls_better(s_g[q], s_k[q], bg, bk)) {
        bg = s_g[q];
        bk = s_k[q];
      }
    out->gain = bg;
    out->key = bk;
  }
}

// k_lsapply, one workgroup per point: the best of the 2n records, the move applied to x and r (every row takes its tested
// value; a zero coefficient leaves it as it is), the move counted; a point without a candidate is done, and every later
// launch of k_lsmove / k_lsapply returns at once for it.
__global__ __launch_bounds__(256) void k_lsapply(LsArgs a) {
  __shared__ double s_g[4];
  __shared__ unsigned long long s_k[4];
  const int p = (int)blockIdx.x;
  if (a.done[p]) return;
  const int n = a.n, m0 = a.m0;
  const size_t ldn = (size_t)a.ldn;
  const LsRec *rec = a.rec + (size_t)p * (size_t)(2 * n);
  double bg = 0.0;
  unsigned long long bk = ~0ull;
  for (int u = TIDX; u < 2 * n; u += 256) {
    const double g = rec[u].gain;
    const unsigned long long k = rec[u].key;
    if (ls_better(g, k, bg, bk)) {
      bg = g;
      bk = k;
    }
  }
  ls_wave_best(bg, bk);
  if ((TIDX & 63) == 0) {
    s_g[TIDX >> 6] = bg;
    s_k[TIDX >> 6] = bk;
  }
  __syncthreads();
  bg = s_g[0];
  bk = s_k[0];
  for (int q = 1; q < 4; q++)
    if (ls_better(s_g[q], s_k[q], bg, bk)) {
      bg = s_g[q];
      bk = s_k[q];
    }
  if (!(bg > 0.0)) {
    if (TIDX == 0) a.done[p] = 1;
    return;
  }
  const bool pair = (bk >> 62) != 0;
  const int u = (int)((bk >> 31) & 0x7fffffffull), v = (int)(bk & 0x7fffffffull);
  const int ju = (u >> 1) + 1, jv = pair ? (v >> 1) + 1 : 0;
  const bool nu = (u & 1) != 0, nv = (v & 1) != 0;
  double *x = a.x + (size_t)p * (size_t)(n + 1);
  double *r = a.r + (size_t)p * (size_t)a.ldm;
  for (int i = TIDX; i < m0; i += 256) {
    const double au = a.Ar[(size_t)i * ldn + (size_t)ju];
    double t = __dadd_rn(r[i], nu ? -au : au);
    if (pair) {
      const double av = a.Ar[(size_t)i * ldn + (size_t)jv];
      t = __dadd_rn(t, nv ? -av : av);
    }
    r[i] = t;
  }
  if (TIDX == 0) {
    x[ju] = x[ju] + (nu ? -1.0 : 1.0);
    if (pair) x[jv] = x[jv] + (nv ? -1.0 : 1.0);
    a.moves[p] = a.moves[p] + 1;
  }
}

void launch_lsact(const LsArgs &a, int final, hipStream_t s) {
  hipLaunchKernelGGL(k_lsact, dim3((unsigned)a.count), dim3(256), 0, s, a, final);
}

// one iteration: the evaluation and the move
void launch_lsiter(const LsArgs &a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_lsmove, dim3((unsigned)(2 * a.n), (unsigned)a.count), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_lsapply, dim3((unsigned)a.count), dim3(256), 0, s, a);
}

} // namespace mvx
