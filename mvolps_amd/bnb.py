"""Python binding of the branch-and-bound driver (include/mvx_bnb.h).

branch_and_bound(prob, ...) mirrors `int branchAndBound(glp_prob*, MVOLP::ParameterObj&)`
(/root/reference/bs.h:7); the strategy arguments are ParameterObj's (-vs / -bs / -cm flags,
/root/reference/2test.cpp:85-149).
"""
import ctypes as C
import os

from . import capi

_FIELDS = [
    "create_prob", "erase_prob", "delete_prob", "copy_prob", "add_rows", "set_mat_row", "set_row_bnds", "set_col_bnds",
    "simplex", "get_status", "get_obj_val", "get_obj_coef", "get_col_prim", "get_num_rows", "get_num_cols", "get_col_kind",
    "get_col_stat", "get_row_stat", "get_row_ub", "get_row_lb", "get_col_ub", "get_col_lb", "get_col_type", "get_mat_row", "eval_tab_row",
    "get_it_cnt",
]
_OPTIONAL = ["simplex_batch", "get_obj_dir", "gmi_cuts", "gmi_cuts_many", "get_col_prim_all", "classify_many", "get_tableau", "get_basis",
             "branch_penalties_many", "round_many", "rc_tighten_many", "tighten_cols_many", "propagate_many", "set_col_bnds_many",
             "dive_pick_many", "set_obj_coef", "set_obj_many", "pump_obj_many", "cut_scores", "add_cut_rows", "conflict_graph", "del_rows",
             "polish_many", "del_rows_many"]
# What the C structs have gained behind the fields listed in this file's three classes.  The classes keep their lists (code that
# walks _fields_ or _OPTIONAL sees what it saw before); an instance made by calling the class is allocated over the WHOLE C
# struct, zeroed, and the appended part is reached by name: tail_get / tail_set for any of them, table_entry / set_table_entry
# for the table, attributes for the parameters and counters.  Views on memory the library owns (from_address, pointers) are
# whole structs already.
_TABLE_TAIL = ["clique_cuts_many", "add_cut_rows_many"]
# ... and behind that tail: a further list per class (_more_), reached by name in the same way, so that `_tail_` keeps the
# members it had; `_full_` covers the fields, the tail and this list -- the whole C struct
_TABLE_MORE = ["kkt_many"]
# ... and behind that one, in the same way (_extra_): members later changes append, so that `_more_` keeps the members it had
_TABLE_EXTRA = ["farkas_many"]


def _with_tail(cls, tail, more=(), extra=()):
    """Gives cls the layout of the whole C struct (its own fields, then `tail`, `more` and `extra`) for allocation and for access by
    name."""
    cls._full_ = type(cls.__name__ + "Whole", (C.Structure,), {"_fields_": list(cls._fields_) + list(tail) + list(more) + list(extra)})
    cls._tail_ = {name: (getattr(cls._full_, name).offset, ctype) for name, ctype in tail}
    cls._more_ = {name: (getattr(cls._full_, name).offset, ctype) for name, ctype in more}
    cls._extra_ = {name: (getattr(cls._full_, name).offset, ctype) for name, ctype in extra}
    for name, ctype in cls._fields_:  # the listed fields sit where the C struct has them
        assert getattr(cls, name).offset == getattr(cls._full_, name).offset


def _behind(obj, name):
    cls = type(obj)
    return cls._tail_[name] if name in cls._tail_ else cls._more_[name] if name in cls._more_ else cls._extra_[name]


def tail_get(obj, name):
    off, ctype = _behind(obj, name)
    at = ctype.from_address(C.addressof(obj) + off)
    return list(at) if isinstance(at, C.Array) else at.value


def tail_set(obj, name, value):
    off, ctype = _behind(obj, name)
    ctype.from_address(C.addressof(obj) + off).value = value


def _tail_attr(name):
    return property(lambda self: tail_get(self, name), lambda self, value: tail_set(self, name, value))


class _WholeStruct(C.Structure):
    def __new__(cls, *args, **kw):
        return cls.from_buffer(cls._full_())


class LpApiTable(_WholeStruct):
    """struct mvx_lp_api: the GLPK-shaped function table the driver calls through."""

    _fields_ = [(name, C.c_void_p) for name in _FIELDS + _OPTIONAL]


_with_tail(LpApiTable, [(name, C.c_void_p) for name in _TABLE_TAIL], [(name, C.c_void_p) for name in _TABLE_MORE],
           [(name, C.c_void_p) for name in _TABLE_EXTRA])


def table_entry(table, name):
    """An entry of the table by name, appended ones (_TABLE_TAIL) included: its address, or None."""
    return tail_get(table, name) if name in _TABLE_TAIL + _TABLE_MORE + _TABLE_EXTRA else getattr(table, name)


def set_table_entry(table, name, value):
    if name in _TABLE_TAIL + _TABLE_MORE + _TABLE_EXTRA:
        tail_set(table, name, value)
    else:
        setattr(table, name, value)


class BnbParams(_WholeStruct):
    _fields_ = [
        ("var_strat", C.c_int),
        ("node_strat", C.c_int),
        ("cut_strat", C.c_int),
        ("cut_chance", C.c_double),
        ("loop_limit", C.c_int),
        ("max_nodes", C.c_int),
        ("reference_quirks", C.c_int),
        ("lazy_pool", C.c_int),
        ("cut_select", C.c_int),
        ("window", C.c_int),
        ("best_window", C.c_int),
        ("sb_cands", C.c_int),
        ("sb_iters", C.c_int),
        ("heur", C.c_int),
        ("rc_fix", C.c_int),
        ("prop", C.c_int),
        ("dive", C.c_int),
        ("dive_freq", C.c_int),
        ("dive_depth", C.c_int),
        ("pump", C.c_int),
        ("pump_freq", C.c_int),
        ("pump_alpha", C.c_double),
        ("cut_rounds", C.c_int),
        ("cut_round_max", C.c_int),
        ("cut_maxpar", C.c_double),
        ("cut_families", C.c_int),
        ("cut_purge", C.c_int),
        ("polish", C.c_int),
        ("node_purge", C.c_int),
    ]
    node_cliques = _tail_attr("node_cliques")
    kkt = _tail_attr("kkt")
    farkas = _tail_attr("farkas")


_with_tail(BnbParams, [("node_cliques", C.c_int)], [("kkt", C.c_int)], [("farkas", C.c_int)])


class BnbEvent(C.Structure):
    _fields_ = [
        ("type", C.c_int),
        ("oid", C.c_int),
        ("pid", C.c_int),
        ("direction", C.c_int),
        ("lp_bound", C.c_double),
        ("sum_infeas", C.c_double),
        ("n_violated", C.c_int),
        ("pick", C.c_int),
    ]


class BnbResult(_WholeStruct):
    _fields_ = [
        ("n_nodes", C.c_int),
        ("parent", C.POINTER(C.c_int)),
        ("prune", C.POINTER(C.c_int)),
        ("node_bound", C.POINTER(C.c_double)),
        ("n_events", C.c_int),
        ("events", C.POINTER(BnbEvent)),
        ("count", C.c_int),
        ("has_incumbent", C.c_int),
        ("best_lower", C.c_double),
        ("incumbent_oid", C.c_int),
        ("n", C.c_int),
        ("x", C.POINTER(C.c_double)),
        ("total_pivots", C.c_longlong),
        ("hit_limit", C.c_int),
        ("rounds", C.c_longlong),
        ("speculated", C.c_longlong),
        ("sb_lps", C.c_longlong),
        ("sb_pivots", C.c_longlong),
        ("heur_calls", C.c_longlong),
        ("heur_found", C.c_longlong),
        ("heur_improved", C.c_longlong),
        ("incumbent_heur", C.c_int),
        ("rc_calls", C.c_longlong),
        ("rc_fixed", C.c_longlong),
        ("rc_tightened", C.c_longlong),
        ("prop_calls", C.c_longlong),
        ("prop_fixed", C.c_longlong),
        ("prop_tightened", C.c_longlong),
        ("prop_infeasible", C.c_longlong),
        ("dive_calls", C.c_longlong),
        ("dive_found", C.c_longlong),
        ("dive_improved", C.c_longlong),
        ("dive_lps", C.c_longlong),
        ("dive_pivots", C.c_longlong),
        ("pump_calls", C.c_longlong),
        ("pump_found", C.c_longlong),
        ("pump_improved", C.c_longlong),
        ("pump_lps", C.c_longlong),
        ("pump_pivots", C.c_longlong),
        ("cutloop_rounds", C.c_longlong),
        ("cutloop_candidates", C.c_longlong),
        ("cutloop_rows", C.c_longlong),
        ("cutloop_lps", C.c_longlong),
        ("cutloop_pivots", C.c_longlong),
        ("cutloop_bound0", C.c_double),
        ("cutloop_bound", C.c_double),
        ("cutloop_conflicts", C.c_longlong),
        ("cutloop_clique_cands", C.c_longlong),
        ("cutloop_clique_rows", C.c_longlong),
        ("cutloop_purged", C.c_longlong),
        ("cutloop_live_rows", C.c_longlong),
        ("polish_calls", C.c_longlong),
        ("polish_moves", C.c_longlong),
        ("polish_improved", C.c_longlong),
        ("node_purge_calls", C.c_longlong),
        ("node_purge_rows", C.c_longlong),
        ("node_cut_rows_peak", C.c_longlong),
    ]
    node_clique_conflicts = _tail_attr("node_clique_conflicts")
    node_clique_calls = _tail_attr("node_clique_calls")
    node_clique_rows = _tail_attr("node_clique_rows")
    kkt_nodes = _tail_attr("kkt_nodes")
    kkt_re = _tail_attr("kkt_re")
    kkt_oid = _tail_attr("kkt_oid")
    farkas_nodes = _tail_attr("farkas_nodes")
    farkas_proved = _tail_attr("farkas_proved")
    farkas_tableau_only = _tail_attr("farkas_tableau_only")
    farkas_none = _tail_attr("farkas_none")
    farkas_dropped = _tail_attr("farkas_dropped")
    farkas_rel_min = _tail_attr("farkas_rel_min")
    farkas_de_max = _tail_attr("farkas_de_max")
    farkas_rel_oid = _tail_attr("farkas_rel_oid")
    farkas_de_oid = _tail_attr("farkas_de_oid")


NODE_CLIQUE_COUNTERS = ("node_clique_conflicts", "node_clique_calls", "node_clique_rows")
# kkt = 1: node LPs checked; the worst re_max per condition (KKT_CONDS) over the tree, a list of 4; the lowest oid of each
KKT_COUNTERS = ("kkt_nodes", "kkt_re", "kkt_oid")
KKT_CONDS = ("PE", "PB", "DE", "DB")
# farkas = 1: the node LPs that ended NOFEAS; those proved on the model (found = 2), by the tableau row only (1), not at all (0);
# those whose model side dropped a coefficient; the smallest model-side rel among the proved and the largest de, with their oids
FARKAS_COUNTERS = ("farkas_nodes", "farkas_proved", "farkas_tableau_only", "farkas_none", "farkas_dropped", "farkas_rel_min",
                   "farkas_de_max", "farkas_rel_oid", "farkas_de_oid")
_with_tail(BnbResult, [(name, C.c_longlong) for name in NODE_CLIQUE_COUNTERS],
           [("kkt_nodes", C.c_longlong), ("kkt_re", C.c_double * 4), ("kkt_oid", C.c_int * 4)],
           [(name, C.c_longlong) for name in FARKAS_COUNTERS[:5]] + [(name, C.c_double) for name in FARKAS_COUNTERS[5:7]]
           + [(name, C.c_int) for name in FARKAS_COUNTERS[7:]])


def table_from(api):
    """Build an mvx_lp_api table out of any library that exports the ABI under api.prefix."""
    t = LpApiTable()
    for name in _FIELDS:
        fn = getattr(api.lib, api.prefix + name)
        setattr(t, name, C.cast(fn, C.c_void_p).value)
    for name in _OPTIONAL + _TABLE_TAIL + _TABLE_MORE + _TABLE_EXTRA:  # optional entries stay NULL when the library does not export them
        fn = getattr(api.lib, api.prefix + name, None) if hasattr(api.lib, api.prefix + name) else None
        set_table_entry(t, name, C.cast(fn, C.c_void_p).value if fn is not None else None)
    return t


def _bind(lib):
    lib.mvx_hip_lp_api.restype = C.c_void_p
    lib.mvx_bnb_default_params.argtypes = [C.POINTER(BnbParams)]
    lib.mvx_branchAndBound.restype = C.c_int
    lib.mvx_branchAndBound.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BnbParams), C.POINTER(BnbResult)]
    lib.mvx_bnb_free_result.argtypes = [C.POINTER(BnbResult)]
    lib.mvx_getFract.restype = C.c_double
    lib.mvx_getFract.argtypes = [C.c_double]
    lib.mvx_printInfo.restype = C.c_int
    lib.mvx_printInfo.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mvx_bnb_classify.restype = C.c_int
    lib.mvx_bnb_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.mvx_bnb_make_children.restype = C.c_int
    lib.mvx_bnb_make_children.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.mvx_bnb_integral_bounds.restype = C.c_int
    lib.mvx_bnb_integral_bounds.argtypes = [C.c_void_p, C.c_void_p]
    lib.mvx_bnb_fractional_bounds.restype = C.c_int
    lib.mvx_bnb_fractional_bounds.argtypes = [C.c_void_p, C.c_void_p]
    lib.mvx_bnb_node_cuts.restype = C.c_int
    lib.mvx_bnb_node_cuts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BnbParams)]
    lib.mvx_classify_many.restype = C.c_int
    lib.mvx_classify_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_double), C.c_int]
    _DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.mvx_branch_penalties_many.restype = C.c_int
    lib.mvx_branch_penalties_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, _IP, _IP, C.c_double, _DP, _DP, _IP, _IP]
    lib.mvx_bnb_penalties.restype = C.c_int
    lib.mvx_bnb_penalties.argtypes = [C.c_void_p, C.c_void_p, _IP, C.c_int, C.c_double, _DP, _DP, _IP, _IP]
    lib.mvx_round_many.restype = C.c_int
    lib.mvx_round_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, _DP, _IP, _DP]
    lib.mvx_bnb_round.restype = C.c_int
    lib.mvx_bnb_round.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _DP, _IP, _DP]
    lib.mvx_rc_tighten_many.restype = C.c_int
    lib.mvx_rc_tighten_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, _DP, C.c_double, _IP, _IP, _DP, _DP]
    lib.mvx_tighten_cols_many.restype = C.c_int
    lib.mvx_tighten_cols_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, _IP, _IP, _DP, _DP]
    lib.mvx_bnb_rc_tighten.restype = C.c_int
    lib.mvx_bnb_rc_tighten.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, _IP, _IP, _DP, _DP]
    lib.mvx_propagate_many.restype = C.c_int
    lib.mvx_propagate_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, _IP, _IP, _IP, _IP, _DP, _DP]
    lib.mvx_bnb_propagate.restype = C.c_int
    lib.mvx_bnb_propagate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _IP, _IP, _IP, _IP, _DP, _DP]
    lib.mvx_set_col_bnds_many.restype = C.c_int
    lib.mvx_set_col_bnds_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, _IP, _IP, _DP, _DP]
    lib.mvx_dive_pick_many.restype = C.c_int
    lib.mvx_dive_pick_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, _IP, _IP, _IP, _IP, _DP]
    lib.mvx_bnb_dive_pick.restype = C.c_int
    lib.mvx_bnb_dive_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _IP, _IP, _IP, _DP]
    lib.mvx_bnb_dive.restype = C.c_int
    lib.mvx_bnb_dive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _DP, _IP, _DP, C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_longlong)]
    lib.mvx_set_obj_many.restype = C.c_int
    lib.mvx_set_obj_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, _DP]
    lib.mvx_pump_obj_many.restype = C.c_int
    lib.mvx_pump_obj_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, _DP, _IP, _DP, _IP, _DP, _DP]
    lib.mvx_bnb_pump_obj.restype = C.c_int
    lib.mvx_bnb_pump_obj.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _DP, C.c_int, _DP, _IP, _DP, _DP]
    lib.mvx_bnb_pump.restype = C.c_int
    lib.mvx_bnb_pump.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, _DP, _IP, _DP, C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_longlong), _IP]
    lib.mvx_cut_scores.restype = C.c_int
    lib.mvx_cut_scores.argtypes = [C.c_void_p, C.c_int, _DP, _DP, _DP]
    lib.mvx_add_cut_rows.restype = C.c_int
    lib.mvx_add_cut_rows.argtypes = [C.c_void_p, C.c_int, _DP, _DP]
    lib.mvx_bnb_cut_scores.restype = C.c_int
    lib.mvx_bnb_cut_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _DP, _DP, _DP]
    lib.mvx_bnb_cut_select.restype = C.c_int
    lib.mvx_bnb_cut_select.argtypes = [C.c_int, _DP, _DP, C.c_int, C.c_double, C.c_int, _IP, _IP]
    lib.mvx_bnb_cut_loop.restype = C.c_int
    lib.mvx_bnb_cut_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_longlong), _DP]
    _UP, _LP = C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong)
    lib.mvx_bnb_cut_loop_families.restype = C.c_int
    lib.mvx_bnb_cut_loop_families.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, _LP, _DP]
    lib.mvx_bnb_cut_loop_purge.restype = C.c_int
    lib.mvx_bnb_cut_loop_purge.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _LP, _DP]
    lib.mvx_del_rows.restype = C.c_int
    lib.mvx_del_rows.argtypes = [C.c_void_p, C.c_int, _IP]
    lib.mvx_conflict_graph.restype = C.c_int
    lib.mvx_conflict_graph.argtypes = [C.c_void_p, _UP, _LP]
    lib.mvx_bnb_conflict_graph.restype = C.c_int
    lib.mvx_bnb_conflict_graph.argtypes = [C.c_void_p, C.c_void_p, _UP, _LP]
    lib.mvx_bnb_clique_cuts.restype = C.c_int
    lib.mvx_bnb_clique_cuts.argtypes = [C.c_int, _UP, _DP, C.c_int, _DP, _DP, _IP]
    lib.mvx_clique_cuts_many.restype = C.c_int
    lib.mvx_clique_cuts_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, _IP, _UP, _DP]
    lib.mvx_bnb_clique_masks.restype = C.c_int
    lib.mvx_bnb_clique_masks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _UP, C.c_int, _IP, _UP, _DP]
    lib.mvx_del_rows_many.restype = C.c_int
    lib.mvx_del_rows_many.argtypes = [C.c_void_p, C.c_int, _IP, _IP]
    lib.mvx_add_cut_rows_many.restype = C.c_int
    lib.mvx_add_cut_rows_many.argtypes = [C.c_void_p, C.c_int, _IP, _DP, _DP]
    lib.mvx_bnb_purge_ages.restype = C.c_int
    lib.mvx_bnb_purge_ages.argtypes = [C.c_int, _IP, C.c_int, C.POINTER(C.c_ubyte), _IP, _IP]
    lib.mvx_polish_many.restype = C.c_int
    lib.mvx_polish_many.argtypes = [C.c_void_p, C.c_int, _DP, C.c_int, _DP, _IP, _IP]
    lib.mvx_bnb_polish.restype = C.c_int
    lib.mvx_bnb_polish.argtypes = [C.c_void_p, C.c_void_p, _DP, C.c_int, _DP, _IP, _IP]
    lib.mvx_ranges.restype = C.c_int
    lib.mvx_ranges.argtypes = [C.c_void_p, _DP, _IP]
    lib.mvx_kkt_many.restype = C.c_int
    lib.mvx_kkt_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, _DP, _IP]
    lib.mvx_kkt.restype = C.c_int
    lib.mvx_kkt.argtypes = [C.c_void_p, _DP, _IP, _DP, _DP]
    lib.mvx_check_kkt.restype = C.c_int
    lib.mvx_check_kkt.argtypes = [C.c_void_p, C.c_int, C.c_int, _DP, _IP, _DP, _IP]
    lib.mvx_bnb_kkt.restype = C.c_int
    lib.mvx_bnb_kkt.argtypes = [C.c_void_p, C.c_void_p, _DP, _IP, _DP, _DP]
    lib.mvx_bnb_kkt_values.restype = C.c_int
    lib.mvx_bnb_kkt_values.argtypes = [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, _DP, _DP, _IP, C.c_int, _DP, _IP, _DP, _DP]
    lib.mvx_farkas_many.restype = C.c_int
    lib.mvx_farkas_many.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, _DP, _IP]
    lib.mvx_farkas.restype = C.c_int
    lib.mvx_farkas.argtypes = [C.c_void_p, _DP, _IP, _DP]
    lib.mvx_bnb_farkas.restype = C.c_int
    lib.mvx_bnb_farkas.argtypes = [C.c_void_p, C.c_void_p, _DP, _IP, _DP]
    lib.mvx_bnb_farkas_values.restype = C.c_int
    lib.mvx_bnb_farkas_values.argtypes = [C.c_int, C.c_int, _DP, _IP, _IP, _DP, _DP, _DP, _DP, _IP, _DP]
    lib.mvx_ray.restype = C.c_int
    lib.mvx_ray.argtypes = [C.c_void_p, _DP, _IP, _DP]
    lib.mvx_get_unbnd_ray.restype = C.c_int
    lib.mvx_get_unbnd_ray.argtypes = [C.c_void_p]
    lib.mvx_bnb_ray.restype = C.c_int
    lib.mvx_bnb_ray.argtypes = [C.c_void_p, C.c_void_p, _DP, _IP, _DP]
    lib.mvx_ranges_chunk.restype = C.c_int
    lib.mvx_ranges_chunk.argtypes = []
    lib.mvx_bnb_ranges.restype = C.c_int
    lib.mvx_bnb_ranges.argtypes = [C.c_void_p, C.c_void_p, _DP, _IP]
    lib.mvx_bnb_print_ranges.restype = C.c_int
    lib.mvx_bnb_print_ranges.argtypes = [C.c_void_p, C.c_void_p, _DP, _IP, C.c_char_p]
    lib.mvx_price_cols.restype = C.c_int
    lib.mvx_price_cols.argtypes = [C.c_void_p, C.c_int, _DP, _DP, _DP, _DP]
    lib.mvx_bnb_price_cols.restype = C.c_int
    lib.mvx_bnb_price_cols.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _DP, _DP, _DP, _DP]
    lib.mvx_del_cols.restype = C.c_int
    lib.mvx_del_cols.argtypes = [C.c_void_p, C.c_int, _IP]
    _UP = C.POINTER(C.c_ubyte)
    lib.mvx_bnb_pool_price_values.restype = C.c_int
    lib.mvx_bnb_pool_price_values.argtypes = [C.c_int, C.c_int, _DP, _DP, _IP, _DP, C.c_int, C.c_double, _DP, _UP]
    lib.mvx_bnb_pool_select.restype = C.c_int
    lib.mvx_bnb_pool_select.argtypes = [C.c_int, _DP, _UP, _UP, C.c_int, _IP, _IP]
    lib.mvx_del_cols_span.restype = C.c_int
    lib.mvx_del_cols_span.argtypes = []
    lib.mvx_generateCutGMI.restype = C.c_int
    lib.mvx_generateCutGMI.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _IP, _DP, _DP, _DP]
    lib.mvx_generateCut3.restype = C.c_int
    lib.mvx_generateCut3.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        from . import load_library

        _lib = _bind(load_library())
    return _lib


def result_to_dict(res):
    nn = res.n_nodes
    return {
        "n_nodes": nn,
        "parent": [res.parent[i] for i in range(1, nn + 1)],
        "prune": [res.prune[i] for i in range(1, nn + 1)],
        "node_bound": [res.node_bound[i] for i in range(1, nn + 1)],
        "events": [
            (e.type, e.oid, e.pid, e.direction, e.lp_bound, e.sum_infeas, e.n_violated, e.pick)
            for e in (res.events[k] for k in range(res.n_events))
        ],
        "count": res.count,
        "has_incumbent": res.has_incumbent,
        "best_lower": res.best_lower,
        "incumbent_oid": res.incumbent_oid,
        "x": [res.x[j] for j in range(1, res.n + 1)],
        "total_pivots": res.total_pivots,
        "hit_limit": res.hit_limit,
        "rounds": res.rounds,
        "speculated": res.speculated,
        "sb_lps": res.sb_lps,
        "sb_pivots": res.sb_pivots,
        "heur_calls": res.heur_calls,
        "heur_found": res.heur_found,
        "heur_improved": res.heur_improved,
        "incumbent_heur": res.incumbent_heur,
        "rc_calls": res.rc_calls,
        "rc_fixed": res.rc_fixed,
        "rc_tightened": res.rc_tightened,
        "prop_calls": res.prop_calls,
        "prop_fixed": res.prop_fixed,
        "prop_tightened": res.prop_tightened,
        "prop_infeasible": res.prop_infeasible,
        "dive_calls": res.dive_calls,
        "dive_found": res.dive_found,
        "dive_improved": res.dive_improved,
        "dive_lps": res.dive_lps,
        "dive_pivots": res.dive_pivots,
        "pump_calls": res.pump_calls,
        "pump_found": res.pump_found,
        "pump_improved": res.pump_improved,
        "pump_lps": res.pump_lps,
        "pump_pivots": res.pump_pivots,
        "cutloop_rounds": res.cutloop_rounds,
        "cutloop_candidates": res.cutloop_candidates,
        "cutloop_rows": res.cutloop_rows,
        "cutloop_lps": res.cutloop_lps,
        "cutloop_pivots": res.cutloop_pivots,
        "cutloop_bound0": res.cutloop_bound0,
        "cutloop_bound": res.cutloop_bound,
        "cutloop_conflicts": res.cutloop_conflicts,
        "cutloop_clique_cands": res.cutloop_clique_cands,
        "cutloop_clique_rows": res.cutloop_clique_rows,
        "cutloop_purged": res.cutloop_purged,
        "cutloop_live_rows": res.cutloop_live_rows,
        "polish_calls": res.polish_calls,
        "polish_moves": res.polish_moves,
        "polish_improved": res.polish_improved,
        "node_purge_calls": res.node_purge_calls,
        "node_purge_rows": res.node_purge_rows,
        "node_cut_rows_peak": res.node_cut_rows_peak,
        "node_clique_conflicts": res.node_clique_conflicts,
        "node_clique_calls": res.node_clique_calls,
        "node_clique_rows": res.node_clique_rows,
        "kkt_nodes": res.kkt_nodes,
        "kkt_re": res.kkt_re,
        "kkt_oid": res.kkt_oid,
        **{name: getattr(res, name) for name in FARKAS_COUNTERS},
    }


def make_params(var_strat=0, node_strat=0, cut_strat=0, max_nodes=0, quirks=1, lazy_pool=1, window=None, cut_select=0, cut_chance=1.0,
                best_window=None, sb_cands=None, sb_iters=None, heur=None, rc_fix=None, prop=None, dive=None, dive_freq=None,
                dive_depth=None, pump=None, pump_freq=None, pump_alpha=None, cut_rounds=None, cut_round_max=None, cut_maxpar=None,
                cut_families=None, cut_purge=None, polish=None, node_purge=None, node_cliques=None, kkt=None,
                farkas=None):
    """mvx_bnb_params with ParameterObj's defaults (util.h:65-67) overridden by the arguments (None: the default)."""
    pr = BnbParams()
    lib().mvx_bnb_default_params(C.byref(pr))
    pr.var_strat, pr.node_strat, pr.cut_strat, pr.max_nodes = var_strat, node_strat, cut_strat, max_nodes
    pr.reference_quirks, pr.lazy_pool = quirks, lazy_pool
    pr.cut_select, pr.cut_chance = cut_select, cut_chance
    if window is not None:
        pr.window = window
    if best_window is not None:
        pr.best_window = best_window
    if sb_cands is not None:
        pr.sb_cands = sb_cands
    if sb_iters is not None:
        pr.sb_iters = sb_iters
    if heur is not None:
        pr.heur = heur
    if rc_fix is not None:
        pr.rc_fix = rc_fix
    if prop is not None:
        pr.prop = prop
    if dive is not None:
        pr.dive = dive
    if dive_freq is not None:
        pr.dive_freq = dive_freq
    if dive_depth is not None:
        pr.dive_depth = dive_depth
    if pump is not None:
        pr.pump = pump
    if pump_freq is not None:
        pr.pump_freq = pump_freq
    if pump_alpha is not None:
        pr.pump_alpha = pump_alpha
    if cut_rounds is not None:
        pr.cut_rounds = cut_rounds
    if cut_round_max is not None:
        pr.cut_round_max = cut_round_max
    if cut_maxpar is not None:
        pr.cut_maxpar = cut_maxpar
    if cut_families is not None:
        pr.cut_families = cut_families
    if cut_purge is not None:
        pr.cut_purge = cut_purge
    if polish is not None:
        pr.polish = polish
    if node_purge is not None:
        pr.node_purge = node_purge
    if node_cliques is not None:
        pr.node_cliques = node_cliques
    if kkt is not None:
        pr.kkt = kkt
    if farkas is not None:
        pr.farkas = farkas
    return pr


def branch_and_bound(prob, var_strat=0, node_strat=0, cut_strat=0, max_nodes=0, quirks=1, lazy_pool=1, table=None, window=None,
                     cut_select=0, cut_chance=1.0, best_window=None, sb_cands=None, sb_iters=None, heur=None, rc_fix=None, prop=None,
                     dive=None, dive_freq=None, dive_depth=None, pump=None, pump_freq=None, pump_alpha=None, cut_rounds=None,
                     cut_round_max=None, cut_maxpar=None, cut_families=None, cut_purge=None, polish=None, node_purge=None,
                     node_cliques=None, kkt=None, farkas=None):
    """Run the driver on `prob` (a capi.Prob).  table=None uses the gfx950 engine's own table.  best_window > 1 with
    node_strat=1: the speculative best-bound window (mvx_bnb_params.best_window).  var_strat 3 / 4: branching on the node
    LP's penalties / strong branching (sb_cands candidates, sb_iters pivots per child).  heur 1 / 2: the primal rounding
    heuristic on every branching node (round and check / round, check and fill; quirks=0 only).  rc_fix 1: reduced-cost bound
    tightening on every branching node once an incumbent exists (quirks=0, not with best_window).  prop 1..16: node bound
    propagation of the root and of every child with that round limit (quirks=0, not with best_window).  dive 1..7: the LP
    diving heuristic with those rules (bits 1 fractional, 2 locks, 4 vector length) at the root and, with dive_freq = F > 0,
    at every branching node whose oid F divides; dive_depth limits a dive's steps (quirks=0, not with best_window).  pump 1..1000: the
    feasibility pump with that limit of distance LPs at the root and, with pump_freq = F > 0, at every branching node whose oid F
    divides, behind the rounding heuristic and in front of the dives; pump_alpha (0..1) weighs the model's objective into the
    distance LPs (quirks=0, not with best_window).  cut_rounds 1..64: that many rounds of GMI cuts on the root LP before the
    tree starts, at most cut_round_max (default 32) cuts a round, none more than cut_maxpar (default 0.9) parallel to one
    taken before it in the round (quirks=0; every single-GPU driver); cut_families chooses the families of those rounds as bits, 1 GMI
    (the default), 2 clique cuts from the conflict graph of the binary columns; cut_purge = A in 1..64 takes a row of those rounds
    out again once its auxiliary variable has been basic after A consecutive re-solves (0, the default: no row leaves).
    polish = N in 1..100000: every point that becomes the incumbent is first improved by a best-improvement search over one- and
    two-column unit moves, at most N of them (quirks=0; every single-GPU driver, best_window included).  node_purge = A in
    1..64: a cut row behind the caller's rows leaves both children of a branching node once its auxiliary variable has been basic
    at A branching nodes in a row on the path (quirks=0, not with best_window; NODE_PURGE_COUNTERS in the dictionary).
    node_cliques = K in 1..64: up to K violated cliques of the model's conflict graph are separated at every branching node and
    appended to both children (quirks=0, not with best_window; NODE_CLIQUE_COUNTERS in the dictionary).  kkt = 1: every node LP the
    tree solves is checked against the model (DESIGN.md "KKT check (kkt)"), pure observation, in both quirk modes, not with
    best_window; KKT_COUNTERS in the dictionary.  farkas = 1: every node LP that ends NOFEAS is asked for a proof of its
    infeasibility on the model (DESIGN.md "Infeasibility and unboundedness proofs (farkas)"), pure observation, in both quirk modes,
    not with best_window; FARKAS_COUNTERS in the dictionary.  The
    dictionary's "rc" is mvx_branchAndBound's return code (-1 refused parameters, -2 penalties, heuristic, tightening,
    propagation, pumps or dives unavailable)."""
    L = lib()
    pr = make_params(var_strat, node_strat, cut_strat, max_nodes, quirks, lazy_pool, window, cut_select, cut_chance, best_window, sb_cands,
                     sb_iters, heur, rc_fix, prop, dive, dive_freq, dive_depth, pump, pump_freq, pump_alpha, cut_rounds, cut_round_max,
                     cut_maxpar, cut_families, cut_purge, polish, node_purge, node_cliques, kkt, farkas)
    res = BnbResult()
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = L.mvx_branchAndBound(tptr, prob.h, C.byref(pr), C.byref(res))
    out = result_to_dict(res)
    out["rc"] = rc
    L.mvx_bnb_free_result(C.byref(res))
    return out


def print_info(prob, quirks=1, table=None):
    import numpy as np

    L = lib()
    n = prob.n
    buf = np.zeros(n + 1, dtype=np.int32)
    cnt = C.c_int(0)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    st = L.mvx_printInfo(tptr, prob.h, quirks, buf.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cnt))
    return st, buf[: cnt.value].tolist()


def generate_cut3(prob, j, table=None):
    import numpy as np

    L = lib()
    n = prob.n
    inds = np.zeros(n + 1, dtype=np.int32)
    vals = np.zeros(n + 1, dtype=np.float64)
    lb = C.c_double(0.0)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = L.mvx_generateCut3(tptr, prob.h, j, inds.ctypes.data_as(C.POINTER(C.c_int)), vals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lb))
    if rc != 0:
        return None
    return inds, vals, lb.value


def node_cuts(a, params, table=None):
    """bs.cpp:249-258 on one solved node about to be branched: append its GMI cut row(s); returns their number
    (-1: bug-compatible mode and the node generated none).  `params`: keyword arguments of make_params."""
    pr = make_params(**params)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    return lib().mvx_bnb_node_cuts(tptr, a.h, C.byref(pr))


def classify(prob, root, quirks=1, var_strat=0, table=None):
    """(status, objective, n_violated, sum_fract, pick) of a solved node in one call."""
    out = (C.c_double * 5)()
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    lib().mvx_bnb_classify(tptr, prob.h, root.h, quirks, var_strat, out)
    return int(out[0]), out[1], int(out[2]), out[3], int(out[4])


def make_children(a, pick, quirks=1, table=None):
    """The two branching clones of bs.cpp:269-282 (bounds set, not yet solved)."""
    S2, S3 = a.api.create(), a.api.create()
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    lib().mvx_bnb_make_children(tptr, a.h, pick, quirks, S2.h, S3.h)
    return S2, S3


def integral_bounds(prob, table=None):
    """mvx_bnb_integral_bounds: round the bounds of `prob`'s integer columns inward, in place (what the repaired drivers do to
    a copy of their root).  Returns 0 nothing to round, 1 rounded, 2 a column's range holds no integer."""
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    return lib().mvx_bnb_integral_bounds(tptr, prob.h)


def fractional_bounds(prob, table=None):
    """mvx_bnb_fractional_bounds: what integral_bounds would return, nothing written."""
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    return lib().mvx_bnb_fractional_bounds(tptr, prob.h)


def classify_many(probs, quirks=1, cap=None):
    """mvx_classify_many over capi.Prob handles: (rc, [(status, violated columns, their values) per handle])."""
    import numpy as np

    k = len(probs)
    n = probs[0].n if k else 0
    cap = max(1, n) if cap is None else cap
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    st = np.zeros(max(1, k), dtype=np.int32)
    nv = np.zeros(max(1, k), dtype=np.int32)
    viol = np.zeros(max(1, k) * max(1, cap), dtype=np.int32)
    xv = np.zeros(max(1, k) * max(1, cap), dtype=np.float64)
    rc = lib().mvx_classify_many(hs, k, quirks, st.ctypes.data_as(C.POINTER(C.c_int)), nv.ctypes.data_as(C.POINTER(C.c_int)),
                                 viol.ctypes.data_as(C.POINTER(C.c_int)), xv.ctypes.data_as(C.POINTER(C.c_double)), cap)
    if rc != 0:
        return rc, None
    out = []
    for t in range(k):
        c = int(nv[t])
        out.append((int(st[t]), viol[t * cap: t * cap + c].tolist(), xv[t * cap: t * cap + c].tolist()))
    return rc, out


def _flat(probs, cols):
    import numpy as np

    hs = (C.c_void_p * max(1, len(probs)))(*[p.h for p in probs])
    off = np.zeros(len(probs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in cols])
    flat = np.array([j for c in cols for j in c] or [0], dtype=np.int32)
    return hs, off, flat


def _pen_out(k):
    import numpy as np

    k = max(1, k)
    return np.zeros(k), np.zeros(k), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)


def _ptrs(pd, pu, ad, au):
    return (pd.ctypes.data_as(C.POINTER(C.c_double)), pu.ctypes.data_as(C.POINTER(C.c_double)), ad.ctypes.data_as(C.POINTER(C.c_int)),
            au.ctypes.data_as(C.POINTER(C.c_int)))


def branch_penalties_many(probs, cols, tol=1e-9):
    """mvx_branch_penalties_many over capi.Prob handles of the gfx950 engine; cols[t] lists handle t's candidate columns.
    Returns (rc, [(pen_down, pen_up, arg_down, arg_up) arrays per handle])."""
    hs, off, flat = _flat(probs, cols)
    pd, pu, ad, au = _pen_out(int(off[-1]))
    rc = lib().mvx_branch_penalties_many(hs, len(probs), flat.ctypes.data_as(C.POINTER(C.c_int)), off.ctypes.data_as(C.POINTER(C.c_int)), tol,
                                         *_ptrs(pd, pu, ad, au))
    if rc != 0:
        return rc, None
    return rc, [(pd[off[t]:off[t + 1]], pu[off[t]:off[t + 1]], ad[off[t]:off[t + 1]], au[off[t]:off[t + 1]]) for t in range(len(probs))]


def penalties(prob, cols, tol=1e-9, table=None):
    """mvx_bnb_penalties (the host twin, from get_tableau / get_basis of `table`; None = the gfx950 engine's table).
    Returns (rc, (pen_down, pen_up, arg_down, arg_up))."""
    import numpy as np

    cs = np.array(list(cols) or [0], dtype=np.int32)
    pd, pu, ad, au = _pen_out(len(cols))
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_penalties(tptr, prob.h, cs.ctypes.data_as(C.POINTER(C.c_int)), len(cols), tol, *_ptrs(pd, pu, ad, au))
    k = len(cols)
    return rc, (pd[:k], pu[:k], ad[:k], au[:k])


def round_many(root, probs, mode=2):
    """mvx_round_many over capi.Prob handles of the gfx950 engine against the model of `root`: one launch for all of them.
    Returns (rc, obj array, found array, x array of shape (len(probs), n + 1); x[:, 0] unused)."""
    import numpy as np

    k = len(probs)
    n = root.n
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    obj = np.zeros(max(1, k))
    found = np.zeros(max(1, k), dtype=np.int32)
    x = np.zeros((max(1, k), n + 1))
    rc = lib().mvx_round_many(root.h, hs, k, mode, obj.ctypes.data_as(C.POINTER(C.c_double)), found.ctypes.data_as(C.POINTER(C.c_int)),
                              x.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, obj[:k], found[:k], x[:k]


def round_node(prob, root, mode=2, table=None):
    """mvx_bnb_round (the host twin, through `table`; None = the gfx950 engine's table) on one solved node against the model
    of `root`.  Returns (rc, obj, found, x array of n + 1 entries; x[0] unused)."""
    import numpy as np

    n = root.n
    obj = C.c_double(0.0)
    found = C.c_int(0)
    x = np.zeros(n + 1)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_round(tptr, prob.h, root.h, mode, C.byref(obj), C.byref(found), x.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, obj.value, found.value, x


POLISH_COUNTERS = ("polish_calls", "polish_moves", "polish_improved")


def polish_many(root, xs, max_moves=1000, table=False):
    """The incumbent polishing (DESIGN.md "Incumbent polishing (polish)") of the points xs, shape (count, n + 1) with entry 0 of a
    point unused, against the model of the handle `root`.  table=False: mvx_polish_many, the gfx950 engine's kernels, one call for
    all points; otherwise the host twin mvx_bnb_polish through `table` (None = the gfx950 engine's table), point by point.
    Returns (rc, x array (count, n + 1), obj array, moves array, ok array); the input is not modified."""
    import numpy as np

    x = np.array(xs, dtype=np.float64, order="C", copy=True)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    k = x.shape[0]
    if x.shape[1] != root.n + 1:
        raise ValueError("polish_many: points need n + 1 = %d entries, got %d" % (root.n + 1, x.shape[1]))
    obj = np.zeros(max(1, k))
    moves = np.zeros(max(1, k), dtype=np.int32)
    ok = np.zeros(max(1, k), dtype=np.int32)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    if table is False:
        rc = lib().mvx_polish_many(root.h, k, x.ctypes.data_as(DP), max_moves, obj.ctypes.data_as(DP), moves.ctypes.data_as(IP),
                                   ok.ctypes.data_as(IP))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = 0
        for t in range(k):
            o, mv, good = C.c_double(0.0), C.c_int(0), C.c_int(0)
            rc = lib().mvx_bnb_polish(tptr, root.h, x[t].ctypes.data_as(DP), max_moves, C.byref(o), C.byref(mv), C.byref(good))
            if rc != 0:
                break
            obj[t], moves[t], ok[t] = o.value, mv.value, good.value
    return rc, x, obj[:k], moves[:k], ok[:k]


RANGE_VAL = ("ACT_DN", "ACT_UP", "OBJ_DN", "OBJ_UP", "COST_DN", "COST_UP")
RANGE_VAR = ("LIM_DN", "LIM_UP", "ENT_DN", "ENT_UP")


def ranges(prob, table=False):
    """The sensitivity ranges (DESIGN.md "Sensitivity ranges (ranges)") of the solved handle `prob`.  table=False: mvx_ranges, the
    gfx950 engine's kernels; otherwise the host twin mvx_bnb_ranges through `table` (None = the gfx950 engine's table).
    Returns (rc, val, var): val (m + n + 1, 6) doubles with the columns RANGE_VAL, var (m + n + 1, 4) ints with the columns
    RANGE_VAR, by variable number (auxiliaries 1..m, then the structurals); row 0 is zero."""
    import numpy as np

    rows = prob.m + prob.n + 1
    val = np.zeros((rows, 6), dtype=np.float64)
    var = np.zeros((rows, 4), dtype=np.int32)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    if table is False:
        rc = lib().mvx_ranges(prob.h, val.ctypes.data_as(DP), var.ctypes.data_as(IP))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_ranges(tptr, prob.h, val.ctypes.data_as(DP), var.ctypes.data_as(IP))
    return rc, val, var


def pool_price_values(cols, obj, types, y, direction, tol):
    """mvx_bnb_pool_price_values, the host twin of mvx_pool_price's pricing pass, from numbers only: cols (N, m) or (N, m+1) as
    Pool.add_cols takes them, obj / types one entry per column, y[0..m] the row weights (y[0] unused).  Returns (rc, dj[0..N],
    attractive[0..N])."""
    import numpy as np

    obj = np.ascontiguousarray(np.atleast_1d(obj), dtype=np.float64)
    N = len(obj)
    y = np.ascontiguousarray(y, dtype=np.float64)
    m = len(y) - 1
    cols = np.asarray(cols, dtype=np.float64).reshape(N, -1)
    if cols.shape[1] == m:
        cols = np.hstack([np.zeros((N, 1)), cols])
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    assert cols.shape == (N, m + 1)
    types = np.ascontiguousarray(np.atleast_1d(types), dtype=np.int32)
    dj = np.zeros(N + 1, dtype=np.float64)
    att = np.zeros(N + 1, dtype=np.uint8)
    DP, IP, UP = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    rc = lib().mvx_bnb_pool_price_values(m, N, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), types.ctypes.data_as(IP), y.ctypes.data_as(DP),
                                         int(direction), float(tol), dj.ctypes.data_as(DP), att.ctypes.data_as(UP))
    return rc, dj, att


def pool_select(dj, attractive, K, skip=None):
    """mvx_bnb_pool_select, the host twin of mvx_pool_price's selection: dj / attractive / skip [0..N].  Returns (rc, picks)."""
    import numpy as np

    dj = np.ascontiguousarray(dj, dtype=np.float64)
    N = len(dj) - 1
    att = np.ascontiguousarray(attractive, dtype=np.uint8)
    DP, IP, UP = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    sp = None
    if skip is not None:
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        sp = skip.ctypes.data_as(UP)
    pick = np.zeros(max(K, 1), dtype=np.int32)
    npick = C.c_int(0)
    rc = lib().mvx_bnb_pool_select(N, dj.ctypes.data_as(DP), att.ctypes.data_as(UP), sp, K, pick.ctypes.data_as(IP), C.byref(npick))
    return rc, pick[: npick.value].copy()


def price_cols(prob, cols, obj, table=False):
    """The images of candidate columns against the tableau of `prob` (DESIGN.md "Column append (add_cols)").  table=False:
    mvx_price_cols, the gfx950 engine's k_addcols; otherwise the host twin mvx_bnb_price_cols through `table` (None = the gfx950
    engine's table).  cols is (k, m) or (k, m+1) as Prob.add_dense_cols takes it.  Returns (rc, dj array of k, img array (k, m+1))."""
    import numpy as np

    m = prob.m
    obj = np.ascontiguousarray(np.atleast_1d(obj), dtype=np.float64)
    k = len(obj)
    cols = capi._cols_block(cols, k, m)
    dj = np.zeros(k, dtype=np.float64)
    img = np.zeros((k, m + 1), dtype=np.float64)
    DP = C.POINTER(C.c_double)
    if table is False:
        rc = lib().mvx_price_cols(prob.h, k, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), dj.ctypes.data_as(DP), img.ctypes.data_as(DP))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_price_cols(tptr, prob.h, k, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), dj.ctypes.data_as(DP),
                                      img.ctypes.data_as(DP))
    return rc, dj, img


def del_cols_span():
    """mvx_del_cols_span: the destination positions a wave of k_delcols moves per batch."""
    return lib().mvx_del_cols_span()


def _kkt_out(m, n, residuals):
    import numpy as np

    val, ind = np.zeros(8, dtype=np.float64), np.zeros(8, dtype=np.int32)
    r_pe = np.zeros(m + 1, dtype=np.float64) if residuals else None
    r_de = np.zeros(n + 1, dtype=np.float64) if residuals else None
    return val, ind, r_pe, r_de


def kkt(prob, table=False, residuals=True):
    """KKT check of one solved handle (DESIGN.md "KKT check (kkt)"): (rc, val[8], ind[8], r_pe[0..m], r_de[0..n]); val holds ae_max,
    re_max of PE, PB, DE, DB (KKT_CONDS), ind where they occur; the residual vectors are None with residuals=False.  table=False:
    mvx_kkt, the gfx950 engine's kernels.  Otherwise the host twin mvx_bnb_kkt through `table` (None: the engine's own table) --
    the same bits."""
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    val, ind, r_pe, r_de = _kkt_out(prob.m, prob.n, residuals)
    pe = r_pe.ctypes.data_as(DP) if residuals else None
    de = r_de.ctypes.data_as(DP) if residuals else None
    if table is False:
        rc = lib().mvx_kkt(prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), pe, de)
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_kkt(tptr, prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), pe, de)
    return rc, val, ind, r_pe, r_de


def kkt_many(root, nodes, table=False):
    """KKT check of the solved handles `nodes` over the rows of `root`: (rc, val (count, 8), ind (count, 8)).  table=False:
    mvx_kkt_many, one device call for all of them.  Otherwise the host twin mvx_bnb_kkt handle by handle through `table`; rc is
    then the first failing call's."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    count = len(nodes)
    val, ind = np.zeros((count, 8), dtype=np.float64), np.zeros((count, 8), dtype=np.int32)
    if table is False:
        hs = (C.c_void_p * max(1, count))(*[p.h for p in nodes])
        return lib().mvx_kkt_many(root.h, hs, count, val.ctypes.data_as(DP), ind.ctypes.data_as(IP)), val, ind
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    for t, p in enumerate(nodes):
        rc = lib().mvx_bnb_kkt(tptr, p.h, val[t].ctypes.data_as(DP), ind[t].ctypes.data_as(IP), None, None)
        if rc != 0:
            return rc, val, ind
    return 0, val, ind


def kkt_values(rows, c, xs, xr, lam, dj, lb, ub, stat, direction=capi.MAX):
    """mvx_bnb_kkt_values, the check from numbers only: rows (m, n) the dense model rows, c (n,) the objective, xs / dj (n,) and
    xr / lam (m,) the four value vectors, lb / ub / stat (m + n,) by variable with the auxiliaries first (+-inf for an absent
    bound).  Returns (rc, val[8], ind[8], r_pe[0..m], r_de[0..n])."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rows = np.asarray(rows, dtype=np.float64)
    m, n = rows.shape

    def lead(v, k, dtype=np.float64):  # the C layout: entry 0 unused
        v = np.asarray(v, dtype=dtype)
        assert v.shape == (k,), (v.shape, k)
        return np.ascontiguousarray(np.concatenate([np.zeros(1, dtype=dtype), v]))

    R = np.ascontiguousarray(np.hstack([np.zeros((m, 1)), rows]))
    args = [lead(c, n), lead(xs, n), lead(xr, m), lead(lam, m), lead(dj, n), lead(lb, m + n), lead(ub, m + n)]
    st = lead(stat, m + n, np.int32)
    val, ind, r_pe, r_de = _kkt_out(m, n, True)
    rc = lib().mvx_bnb_kkt_values(m, n, R.ctypes.data_as(DP), *[a.ctypes.data_as(DP) for a in args], st.ctypes.data_as(IP), int(direction),
                                  val.ctypes.data_as(DP), ind.ctypes.data_as(IP), r_pe.ctypes.data_as(DP), r_de.ctypes.data_as(DP))
    return rc, val, ind, r_pe, r_de


def farkas(prob, table=False, weights=True):
    """Farkas proof of one handle (DESIGN.md "Infeasibility and unboundedness proofs (farkas)"): (rc, val[4], ind[4], y[0..m]); val
    holds rel of the tableau side, rel of the model side, the model side's Lo or -Hi, and de; ind holds found (0 / 1 / 2), the
    tableau row, the side (1 lower, 2 upper) and the coefficients the model side dropped; y (None with weights=False) the row
    weights.  table=False: mvx_farkas, the gfx950 engine's kernels.  Otherwise the host twin mvx_bnb_farkas through `table` (None:
    the engine's own table) -- the same bits."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    val, ind = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.int32)
    y = np.zeros(prob.m + 1, dtype=np.float64) if weights else None
    yp = y.ctypes.data_as(DP) if weights else None
    if table is False:
        rc = lib().mvx_farkas(prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), yp)
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_farkas(tptr, prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), yp)
    return rc, val, ind, y


def farkas_many(root, nodes, table=False):
    """Farkas proofs of the handles `nodes` over the rows of `root`: (rc, val (count, 4), ind (count, 4)).  table=False:
    mvx_farkas_many, one device call for all of them.  Otherwise the host twin mvx_bnb_farkas handle by handle through `table`; rc
    is then the first failing call's."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    count = len(nodes)
    val, ind = np.zeros((count, 4), dtype=np.float64), np.zeros((count, 4), dtype=np.int32)
    if table is False:
        hs = (C.c_void_p * max(1, count))(*[p.h for p in nodes])
        return lib().mvx_farkas_many(root.h, hs, count, val.ctypes.data_as(DP), ind.ctypes.data_as(IP)), val, ind
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    for t, p in enumerate(nodes):
        rc = lib().mvx_bnb_farkas(tptr, p.h, val[t].ctypes.data_as(DP), ind[t].ctypes.data_as(IP), None)
        if rc != 0:
            return rc, val, ind
    return 0, val, ind


def farkas_values(T, head, nb, rows, lb, ub):
    """mvx_bnb_farkas_values, the proof from numbers only: T (m, n) the tableau in eval_tab_row's convention (row i of T the
    coefficients of the basic variable head[i] on the non-basic variables nb[0..n-1]), rows (m, n) the dense model rows, lb / ub
    (m + n,) by variable with the auxiliaries first (+-inf for an absent bound).  Returns (rc, val[4], ind[4], y[0..m])."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rows = np.asarray(rows, dtype=np.float64)
    m, n = rows.shape
    T = np.asarray(T, dtype=np.float64)
    assert T.shape == (m, n), (T.shape, m, n)

    def lead(v, k, dtype=np.float64):  # the C layout: entry 0 unused
        v = np.asarray(v, dtype=dtype)
        assert v.shape == (k,), (v.shape, k)
        return np.ascontiguousarray(np.concatenate([np.zeros(1, dtype=dtype), v]))

    R = np.ascontiguousarray(np.hstack([np.zeros((m, 1)), rows]))
    Tp = np.zeros((m + 1, n + 1))
    Tp[1:, 1:] = T
    hd, nbp, lo, up = lead(head, m, np.int32), lead(nb, n, np.int32), lead(lb, m + n), lead(ub, m + n)
    val, ind, y = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.int32), np.zeros(m + 1, dtype=np.float64)
    rc = lib().mvx_bnb_farkas_values(m, n, Tp.ctypes.data_as(DP), hd.ctypes.data_as(IP), nbp.ctypes.data_as(IP), R.ctypes.data_as(DP),
                                     lo.ctypes.data_as(DP), up.ctypes.data_as(DP), val.ctypes.data_as(DP), ind.ctypes.data_as(IP),
                                     y.ctypes.data_as(DP))
    return rc, val, ind, y


def ray(prob, table=False, direction=True):
    """The ray that proves a handle unbounded (DESIGN.md "Infeasibility and unboundedness proofs (farkas)"): (rc, val[4], ind[6],
    d[0..m+n]); val holds the dual, ae_max, re_max and the slope, ind found (0 / 1 / 2), the variable, the direction, the blocking
    variables and the rows of ae_max and re_max; d (None with direction=False) the ray by variable.  table=False: mvx_ray, the
    gfx950 engine's kernels.  Otherwise the host twin mvx_bnb_ray through `table` (None: the engine's own table) -- the same
    bits."""
    import numpy as np

    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    val, ind = np.zeros(4, dtype=np.float64), np.zeros(6, dtype=np.int32)
    d = np.zeros(prob.m + prob.n + 1, dtype=np.float64) if direction else None
    dp = d.ctypes.data_as(DP) if direction else None
    if table is False:
        rc = lib().mvx_ray(prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), dp)
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_ray(tptr, prob.h, val.ctypes.data_as(DP), ind.ctypes.data_as(IP), dp)
    return rc, val, ind, d


def ranges_chunk():
    """mvx_ranges_chunk: the tableau rows one workgroup of k_rangecols walks."""
    return lib().mvx_ranges_chunk()


def print_ranges(prob, val, var, path=None, table=None):
    """mvx_bnb_print_ranges: the text report of ranges() for `prob` (through `table`; None = the gfx950 engine's table), one line
    per variable, to `path` (None: stdout).  Returns the return code."""
    import numpy as np

    val = np.ascontiguousarray(val, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.int32)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    return lib().mvx_bnb_print_ranges(tptr, prob.h, val.ctypes.data_as(C.POINTER(C.c_double)), var.ctypes.data_as(C.POINTER(C.c_int)),
                                      os.fsencode(path) if path is not None else None)


def rc_tighten_many(probs, cutoffs, tol=1e-9):
    """mvx_rc_tighten_many over solved capi.Prob handles of the gfx950 engine, cutoffs[t] the incumbent's objective for
    handle t: one launch for all of them.  Returns (rc, [[(column, lb, ub), ...] per handle]), columns ascending."""
    import numpy as np

    k = len(probs)
    n = probs[0].n if k else 0
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    cut = np.array(list(cutoffs) or [0.0], dtype=np.float64)
    cnt = np.zeros(max(1, k), dtype=np.int32)
    cols = np.zeros(max(1, k * n), dtype=np.int32)
    lb, ub = np.zeros(max(1, k * n)), np.zeros(max(1, k * n))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().mvx_rc_tighten_many(hs, k, cut.ctypes.data_as(DP), tol, cnt.ctypes.data_as(IP), cols.ctypes.data_as(IP), lb.ctypes.data_as(DP),
                                   ub.ctypes.data_as(DP))
    if rc != 0:
        return rc, None
    return rc, [[(int(cols[t * n + i]), float(lb[t * n + i]), float(ub[t * n + i])) for i in range(int(cnt[t]))] for t in range(k)]


def rc_tighten_node(prob, cutoff, tol=1e-9, table=None):
    """mvx_bnb_rc_tighten (the host twin, through `table`; None = the gfx950 engine's table) on one solved node.
    Returns (rc, [(column, lb, ub), ...]), columns ascending."""
    import numpy as np

    n = prob.n
    cnt = C.c_int(0)
    cols = np.zeros(max(1, n), dtype=np.int32)
    lb, ub = np.zeros(max(1, n)), np.zeros(max(1, n))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_rc_tighten(tptr, prob.h, cutoff, tol, C.byref(cnt), cols.ctypes.data_as(IP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP))
    return rc, [(int(cols[i]), float(lb[i]), float(ub[i])) for i in range(cnt.value)]


def tighten_cols_many(probs, lists):
    """mvx_tighten_cols_many: handle t of the gfx950 engine takes the (column, lb, ub) entries of lists[t], all of them in
    one launch.  Returns the call's code (0; -4 and nothing changed when an entry's column is basic or would move)."""
    hs, off, flat = _flat(probs, [[e[0] for e in l] for l in lists])
    import numpy as np

    lb = np.array([e[1] for l in lists for e in l] or [0.0], dtype=np.float64)
    ub = np.array([e[2] for l in lists for e in l] or [0.0], dtype=np.float64)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    return lib().mvx_tighten_cols_many(hs, len(probs), off.ctypes.data_as(IP), flat.ctypes.data_as(IP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP))


def _prop_lists(k, n, inf, rounds, cnt, cols, lb, ub):
    return [(int(inf[t]), int(rounds[t]), [(int(cols[t * n + i]), float(lb[t * n + i]), float(ub[t * n + i])) for i in range(int(cnt[t]))])
            for t in range(k)]


def propagate_many(root, probs, max_rounds=8):
    """mvx_propagate_many over capi.Prob handles of the gfx950 engine (solved or not) against the rows of `root`: one launch
    for all handles and all rounds.  Returns (rc, [(infeasible, rounds, [(column, lb, ub), ...]) per handle]), columns
    ascending, +-inf for an absent bound."""
    import numpy as np

    k = len(probs)
    n = root.n
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    inf, rounds, cnt = (np.zeros(max(1, k), dtype=np.int32) for _ in range(3))
    cols = np.zeros(max(1, k * n), dtype=np.int32)
    lb, ub = np.zeros(max(1, k * n)), np.zeros(max(1, k * n))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().mvx_propagate_many(root.h, hs, k, max_rounds, inf.ctypes.data_as(IP), rounds.ctypes.data_as(IP), cnt.ctypes.data_as(IP),
                                  cols.ctypes.data_as(IP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP))
    if rc != 0:
        return rc, None
    return rc, _prop_lists(k, n, inf, rounds, cnt, cols, lb, ub)


def propagate_node(prob, root, max_rounds=8, table=None):
    """mvx_bnb_propagate (the host twin, through `table`; None = the gfx950 engine's table) on one handle against the rows of
    `root`.  Returns (rc, (infeasible, rounds, [(column, lb, ub), ...]))."""
    import numpy as np

    n = root.n
    inf, rounds, cnt = (np.zeros(1, dtype=np.int32) for _ in range(3))
    cols = np.zeros(max(1, n), dtype=np.int32)
    lb, ub = np.zeros(max(1, n)), np.zeros(max(1, n))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_propagate(tptr, prob.h, root.h, max_rounds, inf.ctypes.data_as(IP), rounds.ctypes.data_as(IP), cnt.ctypes.data_as(IP),
                                 cols.ctypes.data_as(IP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP))
    if rc != 0:
        return rc, None
    return rc, _prop_lists(1, n, inf, rounds, cnt, cols, lb, ub)[0]


def set_col_bnds_many(probs, lists):
    """mvx_set_col_bnds_many: handle t of the gfx950 engine takes the (column, lb, ub) entries of lists[t] (+-inf for an absent
    bound), all of them in one launch; every handle is left as mvx_set_col_bnds per entry would leave it.  Returns the call's
    code (0; -1 and nothing changed for a bad list)."""
    hs, off, flat = _flat(probs, [[e[0] for e in l] for l in lists])
    import numpy as np

    lb = np.array([e[1] for l in lists for e in l] or [0.0], dtype=np.float64)
    ub = np.array([e[2] for l in lists for e in l] or [0.0], dtype=np.float64)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    return lib().mvx_set_col_bnds_many(hs, len(probs), off.ctypes.data_as(IP), flat.ctypes.data_as(IP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP))


def dive_pick_many(root, probs, rules):
    """mvx_dive_pick_many over solved capi.Prob handles of the gfx950 engine against the model of `root`, rules[t] (1, 2 or 4)
    the rule of handle t: one launch for all of them.  Returns (rc, [(nfrac, col, dir, val) per handle])."""
    import numpy as np

    k = len(probs)
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    rl = np.array(list(rules) or [0], dtype=np.int32)
    nfrac, col, dr = (np.zeros(max(1, k), dtype=np.int32) for _ in range(3))
    val = np.zeros(max(1, k))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().mvx_dive_pick_many(root.h, hs, k, rl.ctypes.data_as(IP), nfrac.ctypes.data_as(IP), col.ctypes.data_as(IP), dr.ctypes.data_as(IP),
                                  val.ctypes.data_as(DP))
    if rc != 0:
        return rc, None
    return rc, [(int(nfrac[t]), int(col[t]), int(dr[t]), float(val[t])) for t in range(k)]


def dive_pick_node(prob, root, rule, table=None):
    """mvx_bnb_dive_pick (the host twin, through `table`; None = the gfx950 engine's table) on one solved node against the
    model of `root`.  Returns (rc, (nfrac, col, dir, val))."""
    nfrac, col, dr, val = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_dive_pick(tptr, prob.h, root.h, rule, C.byref(nfrac), C.byref(col), C.byref(dr), C.byref(val))
    return rc, (nfrac.value, col.value, dr.value, val.value)


def dive_node(prob, root, rules=7, depth=0, table=None):
    """mvx_bnb_dive: the whole dives of one solved node under the rules whose bits are set, through `table` (None = the gfx950
    engine's table, whose batched entries then run).  Returns (rc, obj, found, x array of n + 1 entries, lps, pivots)."""
    import numpy as np

    n = root.n
    obj, found = C.c_double(0.0), C.c_int(0)
    lps, piv = C.c_longlong(0), C.c_longlong(0)
    x = np.zeros(n + 1)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_dive(tptr, prob.h, root.h, rules, depth, C.byref(obj), C.byref(found), x.ctypes.data_as(C.POINTER(C.c_double)),
                            C.byref(lps), C.byref(piv))
    return rc, obj.value, found.value, x, lps.value, piv.value


PUMP_ENDS = {1: "integral", 2: "limit", 3: "stalled", 4: "cycle", 5: "failed"}


def set_obj_many(probs, c):
    """mvx_set_obj_many: handle t of the gfx950 engine takes the objective c[t] (n + 1 entries, entry 0 the constant), the cost
    rows of all handles rebuilt in one launch; every handle is left as set_obj_coef per entry would leave it.  Returns the
    call's code (0; -1 bad arguments; -2 device out of memory, nothing changed)."""
    import numpy as np

    k = len(probs)
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    flat = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1)) if k else np.zeros(1)
    return lib().mvx_set_obj_many(hs, k, flat.ctypes.data_as(C.POINTER(C.c_double)))


def pump_obj_many(root, probs, xprev=None, ab=None):
    """mvx_pump_obj_many over solved capi.Prob handles of the gfx950 engine against the model of `root`: one launch for all of
    them.  xprev[t]: handle t's last rounding (n + 1 entries) or None; ab[t] = (a, q), default (1, 0), the plain pump.  Returns
    (rc, info array (k, 4): nfrac, moved, stalled, nnz; xt array (k, n + 1); c array (k, n + 1))."""
    import numpy as np

    k = len(probs)
    n = root.n
    hs = (C.c_void_p * max(1, k))(*[p.h for p in probs])
    xp = np.zeros((max(1, k), n + 1))
    hp = np.zeros(max(1, k), dtype=np.int32)
    for t in range(k):
        if xprev is not None and xprev[t] is not None:
            xp[t] = xprev[t]
            hp[t] = 1
    w = np.array([(1.0, 0.0)] * max(1, k) if ab is None else list(ab), dtype=np.float64).reshape(-1)
    info = np.zeros((max(1, k), 4), dtype=np.int32)
    xt, c = np.zeros((max(1, k), n + 1)), np.zeros((max(1, k), n + 1))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().mvx_pump_obj_many(root.h, hs, k, xp.ctypes.data_as(DP), hp.ctypes.data_as(IP), w.ctypes.data_as(DP), info.ctypes.data_as(IP),
                                 xt.ctypes.data_as(DP), c.ctypes.data_as(DP))
    if rc != 0:
        return rc, None, None, None
    return rc, info[:k], xt[:k], c[:k]


def pump_obj_node(prob, root, xprev=None, ab=(1.0, 0.0), table=None):
    """mvx_bnb_pump_obj (the host twin, through `table`; None = the gfx950 engine's table) on one solved node against the
    model of `root`.  Returns (rc, info array of 4, xt array of n + 1, c array of n + 1)."""
    import numpy as np

    n = root.n
    xp = np.zeros(n + 1) if xprev is None else np.ascontiguousarray(xprev, dtype=np.float64)
    w = np.array(ab, dtype=np.float64)
    info = np.zeros(4, dtype=np.int32)
    xt, c = np.zeros(n + 1), np.zeros(n + 1)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_pump_obj(tptr, prob.h, root.h, xp.ctypes.data_as(DP), 0 if xprev is None else 1, w.ctypes.data_as(DP),
                                info.ctypes.data_as(IP), xt.ctypes.data_as(DP), c.ctypes.data_as(DP))
    return rc, info, xt, c


def pump_node(prob, root, iters=30, alpha=0.0, table=None):
    """mvx_bnb_pump: one whole feasibility pump of the solved node `prob`, at most `iters` distance LPs, objective weight
    `alpha`, through `table` (None = the gfx950 engine's table, whose batched entries then run).  Returns (rc, obj, found,
    x array of n + 1 entries, lps, pivots, end) with end a key of PUMP_ENDS."""
    import numpy as np

    n = root.n
    obj, found, end = C.c_double(0.0), C.c_int(0), C.c_int(0)
    lps, piv = C.c_longlong(0), C.c_longlong(0)
    x = np.zeros(n + 1)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_bnb_pump(tptr, prob.h, root.h, iters, alpha, C.byref(obj), C.byref(found), x.ctypes.data_as(C.POINTER(C.c_double)),
                            C.byref(lps), C.byref(piv), C.byref(end))
    return rc, obj.value, found.value, x, lps.value, piv.value, end.value


CUTLOOP_COUNTERS = ("cutloop_rounds", "cutloop_candidates", "cutloop_rows", "cutloop_lps", "cutloop_pivots")
CLIQUE_COUNTERS = ("cutloop_conflicts", "cutloop_clique_cands", "cutloop_clique_rows")


def cut_scores(prob, vals, table=False):
    """The scores of the candidate cut rows `vals` (k x (n + 1), entry 0 of a row unused) against the solved handle `prob`:
    (rc, dot array of k, gram array (k, k)).  table=False: mvx_cut_scores, one launch of the gfx950 engine; otherwise the host
    twin mvx_bnb_cut_scores through `table` (None = the gfx950 engine's table)."""
    import numpy as np

    v = np.ascontiguousarray(np.asarray(vals, dtype=np.float64))
    k = v.shape[0] if v.ndim == 2 else 0
    dot, gram = np.zeros(max(1, k)), np.zeros((max(1, k), max(1, k)))
    DP = C.POINTER(C.c_double)
    if table is False:
        rc = lib().mvx_cut_scores(prob.h, k, v.ctypes.data_as(DP), dot.ctypes.data_as(DP), gram.ctypes.data_as(DP))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_cut_scores(tptr, prob.h, k, v.ctypes.data_as(DP), dot.ctypes.data_as(DP), gram.ctypes.data_as(DP))
    return rc, dot[:k], gram[:k, :k]


def cut_select(eff, gram, K=32, maxpar=0.9, budget=1 << 30):
    """mvx_bnb_cut_select, the selection of one round from numbers only: (rc, indices in taken order)."""
    import numpy as np

    e = np.ascontiguousarray(np.asarray(eff, dtype=np.float64))
    g = np.ascontiguousarray(np.asarray(gram, dtype=np.float64))
    k = len(e)
    taken = np.zeros(max(1, k), dtype=np.int32)
    nt = C.c_int(0)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().mvx_bnb_cut_select(k, e.ctypes.data_as(DP), g.ctypes.data_as(DP), K, maxpar, budget, taken.ctypes.data_as(IP), C.byref(nt))
    return rc, taken[: nt.value].tolist()


def add_cut_rows(prob, vals, rhs):
    """mvx_add_cut_rows: the rows `vals` (k x (n + 1), entry 0 of a row unused) appended to the handle `prob` of the gfx950 engine
    as MVX_LO rows with the bounds `rhs`, in one device pass; the handle is left as k single appends leave it.  Returns the
    call's code (0; -1 bad arguments, nothing changed; -2 device out of memory)."""
    import numpy as np

    v = np.ascontiguousarray(np.asarray(vals, dtype=np.float64))
    r = np.ascontiguousarray(np.asarray(rhs, dtype=np.float64))
    k = v.shape[0] if v.ndim == 2 else 0
    if k and (v.shape[1] != prob.n + 1 or len(r) != k):
        return -1
    DP = C.POINTER(C.c_double)
    return lib().mvx_add_cut_rows(prob.h, k, v.ctypes.data_as(DP), r.ctypes.data_as(DP))


def add_cut_rows_many(handles, vals_list, rhs_list):
    """mvx_add_cut_rows_many: handle t of the gfx950 engine takes the rows vals_list[t] (k_t x (n + 1), entry 0 of a row unused;
    k_t = 0: an empty list, the handle is not touched) as MVX_LO rows with the bounds rhs_list[t]; every handle is left as
    mvx_add_cut_rows leaves it, the device work of all of them in one upload and one launch.  Returns the call's code (0; -1 bad
    arguments, no handle changed; -2 device out of memory for some handle)."""
    import numpy as np

    if len(vals_list) != len(handles) or len(rhs_list) != len(handles):
        return -1
    n1 = handles[0].n + 1 if handles else 1
    vs, rs = [], []
    for v, r in zip(vals_list, rhs_list):
        v = np.asarray(v, dtype=np.float64).reshape(-1, n1) if np.size(v) else np.zeros((0, n1))
        r = np.asarray(r, dtype=np.float64).reshape(-1)
        if len(r) != v.shape[0]:
            return -1
        vs.append(v)
        rs.append(r)
    hs = (C.c_void_p * max(1, len(handles)))(*[p.h for p in handles])
    off = np.zeros(len(handles) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rs])
    vals = np.ascontiguousarray(np.concatenate(vs + [np.zeros((1, n1))]))
    rhs = np.ascontiguousarray(np.concatenate(rs + [np.zeros(1)]))
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    return lib().mvx_add_cut_rows_many(hs, len(handles), off.ctypes.data_as(IP), vals.ctypes.data_as(DP), rhs.ctypes.data_as(DP))


PURGE_COUNTERS = ("cutloop_purged", "cutloop_live_rows")


NODE_PURGE_COUNTERS = ("node_purge_calls", "node_purge_rows", "node_cut_rows_peak")


def del_rows_many(handles, lists, table=None):
    """mvx_del_rows_many: handle t loses the model rows lists[t] (1-based, distinct, any order), every handle left as mvx_del_rows
    leaves it, the device work of all of them in one launch.  table=None: the gfx950 engine's own entry point; otherwise the
    del_rows_many entry of `table` (None when the table has none).  Returns the call's code (0; -1 and nothing changed)."""
    hs, off, flat = _flat(handles, lists)
    IP = C.POINTER(C.c_int)
    if table is None:
        return lib().mvx_del_rows_many(hs, len(handles), off.ctypes.data_as(IP), flat.ctypes.data_as(IP))
    if not table.del_rows_many:
        return None
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, IP, IP)(table.del_rows_many)
    return fn(C.cast(hs, C.c_void_p), len(handles), off.ctypes.data_as(IP), flat.ctypes.data_as(IP))


def purge_ages(basic, A, age):
    """mvx_bnb_purge_ages, the age step of the tree's purge from numbers only: (rc, the new ages as a list, the positions whose
    age has reached A)."""
    import numpy as np

    b = np.ascontiguousarray(np.asarray(basic, dtype=np.int32))
    a = np.ascontiguousarray(np.asarray(age, dtype=np.uint8)).copy()
    k = len(a)
    out = np.zeros(max(1, k), dtype=np.int32)
    nout = C.c_int(0)
    IP = C.POINTER(C.c_int)
    rc = lib().mvx_bnb_purge_ages(k, b.ctypes.data_as(IP), A, a.ctypes.data_as(C.POINTER(C.c_ubyte)), out.ctypes.data_as(IP), C.byref(nout))
    return rc, a.tolist(), out[: nout.value].tolist()


def cut_loop(prob, rounds=5, K=0, maxpar=0.0, table=None, families=None, purge=None):
    """mvx_bnb_cut_loop: the root cut loop on the handle `prob`, which is edited in place, through `table` (None = the gfx950
    engine's table, whose batched entries then run).  Returns (rc, dictionary of the cutloop_* counters and bounds).
    families (bits: 1 GMI, 2 clique) goes through mvx_bnb_cut_loop_families, and the dictionary then has CLIQUE_COUNTERS too.
    purge (the age limit A of DESIGN.md "Cut purging (cut_purge)", 0..64) goes through mvx_bnb_cut_loop_purge, with families or 1,
    and the dictionary then has PURGE_COUNTERS as well."""
    cnt = (C.c_longlong * 10)()
    bnd = (C.c_double * 2)()
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    names = CUTLOOP_COUNTERS
    if purge is not None:
        rc = lib().mvx_bnb_cut_loop_purge(tptr, prob.h, rounds, K, maxpar, 1 if families is None else families, purge, cnt, bnd)
        names = CUTLOOP_COUNTERS + CLIQUE_COUNTERS + PURGE_COUNTERS
    elif families is None:
        rc = lib().mvx_bnb_cut_loop(tptr, prob.h, rounds, K, maxpar, cnt, bnd)
    else:
        rc = lib().mvx_bnb_cut_loop_families(tptr, prob.h, rounds, K, maxpar, families, cnt, bnd)
        names = CUTLOOP_COUNTERS + CLIQUE_COUNTERS
    out = {name: int(cnt[i]) for i, name in enumerate(names)}
    out["cutloop_bound0"], out["cutloop_bound"] = bnd[0], bnd[1]
    return rc, out


def conflict_graph(prob, table=False):
    """The conflict graph of the binary columns of the handle `prob` (DESIGN.md "Clique cuts (cut_families)"): (rc, boolean
    (n + 1) x (n + 1) array, edges); row 0 and column 0 are empty.  table=False: mvx_conflict_graph, the gfx950 engine's kernels;
    otherwise the host twin mvx_bnb_conflict_graph through `table` (None = the gfx950 engine's table)."""
    rc, words, edges = conflict_words(prob, table)
    return rc, words_to_bool(words, prob.n), edges


def conflict_words(prob, table=False):
    """conflict_graph's words as the library writes them: (rc, uint64 array (n + 1, W), edges)."""
    import numpy as np

    n = prob.n
    words = np.zeros((n + 1, (n + 1 + 63) // 64), dtype=np.uint64)
    edges = C.c_longlong(0)
    UP = C.POINTER(C.c_ulonglong)
    if table is False:
        rc = lib().mvx_conflict_graph(prob.h, words.ctypes.data_as(UP), C.byref(edges))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = lib().mvx_bnb_conflict_graph(tptr, prob.h, words.ctypes.data_as(UP), C.byref(edges))
    return rc, words, edges.value


def words_to_bool(words, n):
    import numpy as np

    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    return bits[:, : n + 1].astype(bool)


def bool_to_words(adj):
    import numpy as np

    a = np.asarray(adj, dtype=bool)
    W = (a.shape[1] + 63) // 64
    padded = np.zeros((a.shape[0], W * 64), dtype=np.uint8)
    padded[:, : a.shape[1]] = a
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64)


def clique_cuts(adj, x, max_cuts):
    """mvx_bnb_clique_cuts, the clique separation from numbers only: adj the boolean (n + 1) x (n + 1) array of conflict_graph,
    x the LP point (n + 1 entries, entry 0 unused).  Returns (rc, vals array (count, n + 1), rhs array of count)."""
    import numpy as np

    words = bool_to_words(adj)
    n = words.shape[0] - 1
    xs = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    vals, rhs = np.zeros((max(1, max_cuts), n + 1)), np.zeros(max(1, max_cuts))
    cnt = C.c_int(0)
    DP = C.POINTER(C.c_double)
    rc = lib().mvx_bnb_clique_cuts(n, words.ctypes.data_as(C.POINTER(C.c_ulonglong)), xs.ctypes.data_as(DP), max_cuts, vals.ctypes.data_as(DP),
                                   rhs.ctypes.data_as(DP), C.byref(cnt))
    return rc, vals[: cnt.value], rhs[: cnt.value]


def clique_cuts_many(root, probs, max_cuts, table=False, adj=None):
    """The clique separation of the solved handles `probs` against the conflict graph of `root` (DESIGN.md "Clique cuts in the
    tree (node_cliques)"): (rc, cnt int32 array of count, q uint64 array (count, max_cuts, W), sum array (count, max_cuts)).
    table=False: mvx_clique_cuts_many, the gfx950 engine's kernel.  Otherwise the host twin mvx_bnb_clique_masks handle by handle
    through `table` (None = the gfx950 engine's table), the graph taken by conflict_words(root, table) unless `adj` gives its
    words; rc is then the first failing call's code."""
    import numpy as np

    n, count = root.n, len(probs)
    W = (n + 1 + 63) // 64
    k = max(1, max_cuts)
    cnt = np.zeros(max(1, count), dtype=np.int32)
    q = np.zeros((max(1, count), k, W), dtype=np.uint64)
    s = np.zeros((max(1, count), k), dtype=np.float64)
    IP, UP, DP = C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    if table is False:
        hs = (C.c_void_p * max(1, count))(*[P.h for P in probs])
        rc = lib().mvx_clique_cuts_many(root.h, hs, count, max_cuts, cnt.ctypes.data_as(IP), q.ctypes.data_as(UP), s.ctypes.data_as(DP))
    else:
        tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
        rc = 0
        if adj is None:
            rc, adj, _edges = conflict_words(root, table)
        words = np.ascontiguousarray(adj, dtype=np.uint64)
        for t, P in enumerate(probs):
            if rc != 0:
                break
            one = C.c_int(0)
            rc = lib().mvx_bnb_clique_masks(tptr, P.h, n, words.ctypes.data_as(UP), max_cuts, C.byref(one), q[t].ctypes.data_as(UP),
                                            s[t].ctypes.data_as(DP))
            cnt[t] = one.value
    return rc, cnt[:count], q[:count], s[:count]


def generate_cut_gmi(prob, j, table=None):
    """mvx_generateCutGMI, the repaired cut of the basic integer column j of a solved handle: (vals array of n + 1, lb, efficacy),
    or None when there is none."""
    import numpy as np

    n = prob.n
    inds = np.zeros(n + 1, dtype=np.int32)
    vals = np.zeros(n + 1, dtype=np.float64)
    lb, eff = C.c_double(0.0), C.c_double(0.0)
    tptr = C.cast(C.pointer(table), C.c_void_p) if table is not None else None
    rc = lib().mvx_generateCutGMI(tptr, prob.h, j, inds.ctypes.data_as(C.POINTER(C.c_int)), vals.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.byref(lb), C.byref(eff))
    return None if rc != 0 else (vals, lb.value, eff.value)


def node_sample(root, count, quirks=0, table=None):
    """Solved OPT node LPs below `root` (a capi.Prob that is left as it is), breadth first: a solved clone of the root,
    then children and grandchildren (each node branched on one of its violated columns, in turn), at most `count` of them.
    Real B&B nodes for exercising and timing the per-node entries (mvx_round_many, the branching penalties)."""
    first = root.copy()
    first.simplex()
    out, queue = [], [first]
    while queue and len(out) < count:
        P = queue.pop(0)
        if P.status != capi.OPT:
            continue
        out.append(P)
        _st, viol = print_info(P, quirks=quirks, table=table)
        if viol:
            S2, S3 = make_children(P, viol[len(out) % len(viol)], quirks=quirks, table=table)
            S2.simplex()
            S3.simplex()
            queue += [S2, S3]
    return out
