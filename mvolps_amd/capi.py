"""ctypes binding for a GLPK-shaped LP-engine C ABI (include/mvx.h).

The same signature table serves any library that exports the ABI under a prefix
(`mvx_` for the HIP engine).  The surface is exactly what MVOLPS binds from GLPK
(/root/reference/bs.cpp:89,114-117,274-288; cut.cpp:23,40,43;
gmi.cpp:15-52,84; util.cpp:33-41,423-455).
"""
import ctypes as C

import numpy as np

MIN, MAX = 1, 2
CV, IV, BV = 1, 2, 3
FR, LO, UP, DB, FX = 1, 2, 3, 4, 5
BS, NL, NU, NF, NS = 1, 2, 3, 4, 5
UNDEF, FEAS, INFEAS, NOFEAS, OPT, UNBND = 1, 2, 3, 4, 5, 6
OFF, ON = 0, 1
EFAIL, EITLIM = 5, 8


class Smcp(C.Structure):
    _fields_ = [
        ("msg_lev", C.c_int),
        ("meth", C.c_int),
        ("it_lim", C.c_int),
        ("tol_bnd", C.c_double),
        ("tol_dj", C.c_double),
        ("tol_piv", C.c_double),
    ]


class SiftParm(C.Structure):
    _fields_ = [("K", C.c_int), ("max_rounds", C.c_int), ("purge", C.c_int)]


class SiftInfo(C.Structure):
    _fields_ = [
        ("rounds", C.c_int),
        ("lps", C.c_int),
        ("priced", C.c_longlong),
        ("appended", C.c_longlong),
        ("purged", C.c_longlong),
        ("pivots", C.c_longlong),
        ("n_final", C.c_int),
        ("end", C.c_int),
    ]


_P = C.c_void_p
_I = C.c_int
_D = C.c_double
_IP = C.POINTER(C.c_int)
_DP = C.POINTER(C.c_double)

# name -> (restype, argtypes)
SIGNATURES = {
    "create_prob": (_P, []),
    "erase_prob": (None, [_P]),
    "delete_prob": (None, [_P]),
    "copy_prob": (None, [_P, _P, _I]),
    "set_obj_dir": (None, [_P, _I]),
    "add_rows": (_I, [_P, _I]),
    "add_cols": (_I, [_P, _I]),
    "set_row_bnds": (None, [_P, _I, _I, _D, _D]),
    "set_col_bnds": (None, [_P, _I, _I, _D, _D]),
    "set_obj_coef": (None, [_P, _I, _D]),
    "set_mat_row": (None, [_P, _I, _I, _IP, _DP]),
    "set_col_kind": (None, [_P, _I, _I]),
    "set_col_name": (None, [_P, _I, C.c_char_p]),
    "load_dense": (_I, [_P, _I, _I, _DP, _DP, _DP]),
    "init_smcp": (None, [C.POINTER(Smcp)]),
    "set_default_tolerances": (None, [_D, _D, _D]),
    "simplex": (_I, [_P, C.POINTER(Smcp)]),
    "get_obj_dir": (_I, [_P]),
    "get_num_rows": (_I, [_P]),
    "get_num_cols": (_I, [_P]),
    "get_num_int": (_I, [_P]),
    "get_status": (_I, [_P]),
    "get_obj_val": (_D, [_P]),
    "get_obj_coef": (_D, [_P, _I]),
    "get_col_prim": (_D, [_P, _I]),
    "get_row_prim": (_D, [_P, _I]),
    "get_col_dual": (_D, [_P, _I]),
    "get_row_dual": (_D, [_P, _I]),
    "get_col_stat": (_I, [_P, _I]),
    "get_row_stat": (_I, [_P, _I]),
    "get_col_kind": (_I, [_P, _I]),
    "get_row_type": (_I, [_P, _I]),
    "get_row_lb": (_D, [_P, _I]),
    "get_row_ub": (_D, [_P, _I]),
    "get_col_type": (_I, [_P, _I]),
    "get_col_lb": (_D, [_P, _I]),
    "get_col_ub": (_D, [_P, _I]),
    "get_col_name": (C.c_char_p, [_P, _I]),
    "get_mat_row": (_I, [_P, _I, _IP, _DP]),
    "eval_tab_row": (_I, [_P, _I, _IP, _DP]),
    "get_it_cnt": (_I, [_P]),
    "get_bland_cnt": (_I, [_P]),
    "get_pert_cnt": (_I, [_P]),
    "set_stall_limit": (None, [_I]),
    "term_out": (_I, [_I]),
    "version": (C.c_char_p, []),
    "get_tableau_ld": (_I, [_P]),
    "get_tableau": (_I, [_P, _DP]),
    "get_basis": (_I, [_P, _IP, _IP, _IP]),
}


def _dp(a):
    return a.ctypes.data_as(_DP)


def _ip(a):
    return a.ctypes.data_as(_IP)


def _cols_block(cols, k, m):
    """k candidate columns as the C layout k x (m+1), entry 0 of each unused: from (k, m), (k, m+1) or, for k = 1, one vector."""
    cols = np.asarray(cols, dtype=np.float64)
    if cols.ndim == 1:
        cols = cols.reshape(1, -1)
    if cols.shape == (k, m):
        cols = np.hstack([np.zeros((k, 1)), cols])
    if cols.shape != (k, m + 1):
        raise ValueError("columns need shape (%d, %d) or (%d, %d), got %r" % (k, m, k, m + 1, cols.shape))
    return np.ascontiguousarray(cols, dtype=np.float64)


class LpApi:
    """Function table of one engine library."""

    def __init__(self, lib, prefix, extra=None):
        self.lib = lib
        self.prefix = prefix
        sigs = dict(SIGNATURES)
        if extra:
            sigs.update(extra)
        for name, (res, args) in sigs.items():
            fn = getattr(lib, prefix + name)
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def create(self):
        return Prob(self)


class Pool:
    """mvx_colpool (the gfx950 engine's library only): a pool of dense columns over m rows for sifting (DESIGN.md "Sifting (sift)").
    Its model layer -- add_cols, n, get_col -- needs no device."""

    def __init__(self, api, m):
        self.api = api
        self.h = api.pool_create(m)
        if not self.h:
            raise ValueError("pool_create: m must not be negative")

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.api.pool_delete(self.h)
            except Exception:
                pass
            self.h = None

    @property
    def m(self):
        return self.api.pool_num_rows(self.h)

    @property
    def n(self):
        return self.api.pool_num_cols(self.h)

    def add_cols(self, cols, obj, types, lb, ub, kinds=None):
        """mvx_pool_add_cols: the arguments of Prob.add_dense_cols.  Returns 0, or -1 with nothing changed."""
        obj = np.ascontiguousarray(np.atleast_1d(obj), dtype=np.float64)
        k = len(obj)
        cols = _cols_block(cols, k, self.m)
        types = np.ascontiguousarray(np.atleast_1d(types), dtype=np.int32)
        lb = np.ascontiguousarray(np.atleast_1d(lb), dtype=np.float64)
        ub = np.ascontiguousarray(np.atleast_1d(ub), dtype=np.float64)
        if not (len(types) == len(lb) == len(ub) == k):
            raise ValueError("add_cols: obj, types, lb and ub need one entry per column")
        kp = None
        if kinds is not None:
            kinds = np.ascontiguousarray(np.atleast_1d(kinds), dtype=np.int32)
            if len(kinds) != k:
                raise ValueError("add_cols: kinds needs one entry per column")
            kp = _ip(kinds)
        return self.api.pool_add_cols(self.h, k, _dp(cols), _dp(obj), _ip(types), _dp(lb), _dp(ub), kp)

    def get_col(self, j):
        """mvx_pool_get_col: (rc, col[0..m], obj, type, lb, ub, kind) of pool column j as it was given."""
        col = np.zeros(self.m + 1, dtype=np.float64)
        obj, lb, ub = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        ty, kind = C.c_int(0), C.c_int(0)
        rc = self.api.pool_get_col(self.h, j, _dp(col), C.byref(obj), C.byref(ty), C.byref(lb), C.byref(ub), C.byref(kind))
        return rc, col, obj.value, ty.value, lb.value, ub.value, kind.value


class Prob:
    """Thin object wrapper; index conventions stay GLPK's (1-based)."""

    def __init__(self, api, handle=None):
        self.api = api
        self.h = handle if handle is not None else api.create_prob()
        self._own = True

    def __del__(self):
        if getattr(self, "_own", False) and self.h:
            try:
                self.api.delete_prob(self.h)
            except Exception:
                pass
            self.h = None

    def copy(self, names=ON):
        q = Prob(self.api)
        self.api.copy_prob(q.h, self.h, names)
        return q

    # --- build
    def load_dense(self, A, b, c):
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        m, n = A.shape
        assert b.shape == (m,) and c.shape == (n,)
        rc = self.api.load_dense(self.h, m, n, _dp(A), _dp(b), _dp(c))
        if rc != 0:
            raise RuntimeError("load_dense failed rc=%d" % rc)

    def load_general(self, A, row_bnds, col_bnds, c, c0=0.0, kinds=None, direction=MAX):
        """row_bnds / col_bnds: lists of (type, lb, ub)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        m, n = A.shape
        api, h = self.api, self.h
        api.erase_prob(h)
        api.set_obj_dir(h, direction)
        api.add_cols(h, n)
        api.add_rows(h, m)
        api.set_obj_coef(h, 0, float(c0))
        for j in range(n):
            api.set_obj_coef(h, j + 1, float(c[j]))
            t, lb, ub = col_bnds[j]
            api.set_col_bnds(h, j + 1, t, float(lb), float(ub))
            if kinds is not None:
                api.set_col_kind(h, j + 1, int(kinds[j]))
        ind = np.arange(n + 1, dtype=np.int32)
        for i in range(m):
            val = np.concatenate([[0.0], A[i]])
            nz = np.nonzero(val)[0]
            ii = np.concatenate([[0], ind[nz]]).astype(np.int32)
            vv = np.concatenate([[0.0], val[nz]])
            api.set_mat_row(h, i + 1, len(nz), _ip(ii), _dp(vv))
            t, lb, ub = row_bnds[i]
            api.set_row_bnds(h, i + 1, t, float(lb), float(ub))

    def set_mat_row(self, i, ind, val):
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.api.set_mat_row(self.h, i, len(ind) - 1, _ip(ind), _dp(val))

    def del_rows(self, rows):
        """mvx_del_rows (the gfx950 engine's library only): the distinct 1-based row numbers `rows` leave the model and, where
        their auxiliary variables are basic, the device tableau in place.  Returns 0, or -1 with nothing changed."""
        num = np.concatenate([[0], np.asarray(list(rows), dtype=np.int32)]).astype(np.int32)
        return self.api.del_rows(self.h, len(num) - 1, _ip(num))

    def del_cols(self, cols):
        """mvx_del_cols (the gfx950 engine's library only): the distinct 1-based column numbers `cols` leave the model and, where
        the handle has a tableau and they are all non-basic, the live tableau in one device pass (DESIGN.md "Column deletion
        (del_cols)"); a basic one gives the tableau up.  Returns 0, -1 with nothing changed, or -2 (device out of memory)."""
        num = np.concatenate([[0], np.asarray(list(cols), dtype=np.int32)]).astype(np.int32)
        return self.api.del_cols(self.h, len(num) - 1, _ip(num))

    def add_dense_cols(self, cols, obj, types, lb, ub, kinds=None):
        """mvx_add_dense_cols (the gfx950 engine's library only): k dense columns join the model as columns n+1..n+k and, where
        the handle has a tableau, the live tableau (DESIGN.md "Column append (add_cols)").  cols is (k, m) -- cols[t, i-1] the
        coefficient of new column t in model row i -- or (k, m+1) in the C layout (entry 0 unused).  Returns the return code."""
        m = self.m
        obj = np.ascontiguousarray(np.atleast_1d(obj), dtype=np.float64)
        k = len(obj)
        cols = _cols_block(cols, k, m)
        types = np.ascontiguousarray(np.atleast_1d(types), dtype=np.int32)
        lb = np.ascontiguousarray(np.atleast_1d(lb), dtype=np.float64)
        ub = np.ascontiguousarray(np.atleast_1d(ub), dtype=np.float64)
        if not (len(types) == len(lb) == len(ub) == k):
            raise ValueError("add_dense_cols: obj, types, lb and ub need one entry per column")
        kp = None
        if kinds is not None:
            kinds = np.ascontiguousarray(np.atleast_1d(kinds), dtype=np.int32)
            if len(kinds) != k:
                raise ValueError("add_dense_cols: kinds needs one entry per column")
            kp = _ip(kinds)
        return self.api.add_dense_cols(self.h, k, _dp(cols), _dp(obj), _ip(types), _dp(lb), _dp(ub), kp)

    def price_cols(self, cols, obj, images=False):
        """mvx_price_cols (the gfx950 engine's library only): the reduced costs, and with images=True the whole images (k, m+1) by
        tableau row, that add_dense_cols would write for the candidate columns, without appending them.  Returns (rc, dj) or
        (rc, dj, img)."""
        m = self.m
        obj = np.ascontiguousarray(np.atleast_1d(obj), dtype=np.float64)
        k = len(obj)
        cols = _cols_block(cols, k, m)
        dj = np.zeros(k, dtype=np.float64)
        if not images:
            return self.api.price_cols(self.h, k, _dp(cols), _dp(obj), _dp(dj), None), dj
        img = np.zeros((k, m + 1), dtype=np.float64)
        rc = self.api.price_cols(self.h, k, _dp(cols), _dp(obj), _dp(dj), _dp(img))
        return rc, dj, img

    def pool_price(self, pool, K=0, skip=None, want_dj=True):
        """mvx_pool_price (the gfx950 engine's library only): the reduced costs dj[0..N] of every column of `pool` against this
        handle's duals (None with want_dj=False) and the K most attractive columns, in descending |dj|.  skip: N+1 flags, entry 0
        unused.  Returns (rc, dj, picks)."""
        N = pool.n
        dj = np.zeros(N + 1, dtype=np.float64) if want_dj else None
        pick = np.zeros(max(min(K, N), 1), dtype=np.int32)
        npick = C.c_int(0)
        sp = None
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            if len(skip) != N + 1:
                raise ValueError("pool_price: skip needs N + 1 entries")
            sp = skip.ctypes.data_as(C.POINTER(C.c_ubyte))
        rc = self.api.pool_price(self.h, pool.h, sp, K, _dp(dj) if want_dj else None, _ip(pick), C.byref(npick))
        return rc, dj, pick[: npick.value].copy()

    def pool_append(self, pool, idx):
        """mvx_pool_append: the distinct 1-based pool columns idx join the handle as add_dense_cols would append them."""
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int32)
        return self.api.pool_append(self.h, pool.h, len(idx), _ip(idx))

    def sift(self, pool, where=None, K=None, max_rounds=None, purge=None, it_lim=None):
        """mvx_sift: solves this working LP plus the columns of `pool` by sifting.  where: N+1 ints (entry 0 unused), 0 or the column
        of this handle that already is pool column j; None: zeros.  Returns (rc, where, info) with info a SiftInfo."""
        N = pool.n
        where = np.zeros(N + 1, dtype=np.int32) if where is None else np.ascontiguousarray(where, dtype=np.int32).copy()
        if len(where) != N + 1:
            raise ValueError("sift: where needs N + 1 entries")
        sp = SiftParm()
        self.api.init_sift_parm(C.byref(sp), self.m)
        if K is not None:
            sp.K = K
        if max_rounds is not None:
            sp.max_rounds = max_rounds
        if purge is not None:
            sp.purge = purge
        parm = None
        if it_lim is not None:
            parm = Smcp()
            self.api.init_smcp(C.byref(parm))
            parm.it_lim = it_lim
        info = SiftInfo()
        rc = self.api.sift(self.h, pool.h, C.byref(parm) if parm is not None else None, C.byref(sp), _ip(where), C.byref(info))
        return rc, where, info

    def set_mat_col(self, j, ind, val):
        """mvx_set_mat_col: GLPK's shape, ind[0] / val[0] ignored."""
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.api.set_mat_col(self.h, j, len(ind) - 1, _ip(ind), _dp(val))

    def get_mat_col(self, j):
        m = self.m
        ind = np.zeros(m + 1, dtype=np.int32)
        val = np.zeros(m + 1, dtype=np.float64)
        ln = self.api.get_mat_col(self.h, j, _ip(ind), _dp(val))
        return ind[1 : ln + 1].copy(), val[1 : ln + 1].copy()

    # --- solve
    def simplex(self, it_lim=None, meth=None, tol=None):
        if it_lim is None and meth is None and tol is None:
            return self.api.simplex(self.h, None)
        parm = Smcp()
        self.api.init_smcp(C.byref(parm))
        if it_lim is not None:
            parm.it_lim = it_lim
        if meth is not None:
            parm.meth = meth
        if tol is not None:
            parm.tol_bnd, parm.tol_dj, parm.tol_piv = tol
        return self.api.simplex(self.h, C.byref(parm))

    # --- query
    @property
    def m(self):
        return self.api.get_num_rows(self.h)

    @property
    def n(self):
        return self.api.get_num_cols(self.h)

    @property
    def status(self):
        return self.api.get_status(self.h)

    @property
    def obj(self):
        return self.api.get_obj_val(self.h)

    @property
    def it_cnt(self):
        return self.api.get_it_cnt(self.h)

    @property
    def bland_cnt(self):
        return self.api.get_bland_cnt(self.h)

    @property
    def pert_cnt(self):
        return self.api.get_pert_cnt(self.h)

    def col_prim(self):
        return np.array([self.api.get_col_prim(self.h, j) for j in range(1, self.n + 1)])

    def row_prim(self):
        return np.array([self.api.get_row_prim(self.h, i) for i in range(1, self.m + 1)])

    def col_dual(self):
        return np.array([self.api.get_col_dual(self.h, j) for j in range(1, self.n + 1)])

    def row_dual(self):
        return np.array([self.api.get_row_dual(self.h, i) for i in range(1, self.m + 1)])

    def col_stat(self):
        return np.array([self.api.get_col_stat(self.h, j) for j in range(1, self.n + 1)], dtype=np.int32)

    def row_stat(self):
        return np.array([self.api.get_row_stat(self.h, i) for i in range(1, self.m + 1)], dtype=np.int32)

    def tableau(self):
        m, n = self.m, self.n
        out = np.empty((m + 1, n + 1), dtype=np.float64)
        rc = self.api.get_tableau(self.h, _dp(out))
        if rc != 0:
            raise RuntimeError("no tableau")
        return out

    def basis(self):
        m, n = self.m, self.n
        head = np.zeros(m + 1, dtype=np.int32)
        nb = np.zeros(n + 1, dtype=np.int32)
        flag = np.zeros(n + 1, dtype=np.int32)
        rc = self.api.get_basis(self.h, _ip(head), _ip(nb), _ip(flag))
        if rc != 0:
            raise RuntimeError("no basis")
        return head, nb, flag

    def ranges(self):
        """mvx_ranges (the gfx950 engine's library only): the sensitivity ranges of the solved handle.  Returns (rc, val, var):
        val (m + n + 1, 6) doubles and var (m + n + 1, 4) ints by variable number, row 0 zero (columns: bnb.RANGE_VAL / RANGE_VAR)."""
        rows = self.m + self.n + 1
        val = np.zeros((rows, 6), dtype=np.float64)
        var = np.zeros((rows, 4), dtype=np.int32)
        rc = self.api.ranges(self.h, _dp(val), _ip(var))
        return rc, val, var

    def kkt(self, residuals=True):
        """mvx_kkt (the gfx950 engine's library only): the KKT check of the solved handle against its own model.  Returns (rc, val,
        ind, r_pe, r_de): val[8] = ae_max, re_max of PE, PB, DE, DB, ind[8] where they occur, r_pe[0..m] / r_de[0..n] the residuals
        (None with residuals=False)."""
        val = np.zeros(8, dtype=np.float64)
        ind = np.zeros(8, dtype=np.int32)
        r_pe = np.zeros(self.m + 1, dtype=np.float64) if residuals else None
        r_de = np.zeros(self.n + 1, dtype=np.float64) if residuals else None
        rc = self.api.kkt(self.h, _dp(val), _ip(ind), _dp(r_pe) if residuals else None, _dp(r_de) if residuals else None)
        return rc, val, ind, r_pe, r_de

    def farkas(self, weights=True):
        """mvx_farkas (the gfx950 engine's library only): a proof that the handle's LP is infeasible, evaluated on its own model.
        Returns (rc, val, ind, y): val[4] = rel of the tableau side, rel of the model side, the model side's Lo or -Hi, de; ind[4] =
        found (0 none, 1 the tableau row only, 2 proved on the model), the row, the side, the dropped coefficients; y[0..m] the row
        weights (None with weights=False)."""
        val = np.zeros(4, dtype=np.float64)
        ind = np.zeros(4, dtype=np.int32)
        y = np.zeros(self.m + 1, dtype=np.float64) if weights else None
        rc = self.api.farkas(self.h, _dp(val), _ip(ind), _dp(y) if weights else None)
        return rc, val, ind, y

    def ray(self, direction=True):
        """mvx_ray (the gfx950 engine's library only): the ray that proves the handle unbounded, checked on its own model.  Returns
        (rc, val, ind, d): val[4] = the dual, ae_max, re_max, the slope; ind[6] = found (0 / 1 / 2), the variable, the direction,
        the blocking variables, the rows of ae_max and re_max; d[0..m+n] the ray by variable (None with direction=False)."""
        val = np.zeros(4, dtype=np.float64)
        ind = np.zeros(6, dtype=np.int32)
        d = np.zeros(self.m + self.n + 1, dtype=np.float64) if direction else None
        rc = self.api.ray(self.h, _dp(val), _ip(ind), _dp(d) if direction else None)
        return rc, val, ind, d

    def get_unbnd_ray(self):
        """mvx_get_unbnd_ray, glp_get_unbnd_ray's shape: the variable whose move proves MVX_UNBND, 0 otherwise."""
        return self.api.get_unbnd_ray(self.h)

    def check_kkt(self, cond, sol=1):
        """mvx_check_kkt, glp_check_kkt's shape: (rc, ae_max, ae_ind, re_max, re_ind) of condition cond = 1 PE, 2 PB, 3 DE, 4 DB."""
        ae, re = C.c_double(0.0), C.c_double(0.0)
        ai, ri = C.c_int(0), C.c_int(0)
        rc = self.api.check_kkt(self.h, sol, cond, C.byref(ae), C.byref(ai), C.byref(re), C.byref(ri))
        return rc, ae.value, ai.value, re.value, ri.value

    def eval_tab_row(self, k):
        n = self.n
        ind = np.zeros(n + 1, dtype=np.int32)
        val = np.zeros(n + 1, dtype=np.float64)
        ln = self.api.eval_tab_row(self.h, k, _ip(ind), _dp(val))
        return ind[1 : ln + 1].copy(), val[1 : ln + 1].copy()

    def get_mat_row(self, i):
        n = self.n
        ind = np.zeros(n + 1, dtype=np.int32)
        val = np.zeros(n + 1, dtype=np.float64)
        ln = self.api.get_mat_row(self.h, i, _ip(ind), _dp(val))
        return ind[1 : ln + 1].copy(), val[1 : ln + 1].copy()
