"""mvolps_amd -- MI355X-native dense-simplex LP-relaxation engine behind MVOLPS's node solve.

The product is libmvolps_amd.so (C ABI in include/mvx.h, hand-written gfx950 kernels).
This package is the thin Python binding used by the tests, bench.py and the multi-GPU
branch-and-bound coordinator.  There is no CPU fallback: engine calls need a HIP device.
"""
import ctypes as C
import os

from . import capi
from .capi import Pool, SiftInfo, SiftParm  # noqa: F401  (sifting: a column pool and the loop's parameters and counters)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmvolps_amd.so")

_EXTRA = {
    "del_rows": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "del_rows_many": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "add_cut_rows_many": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ranges": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "ranges_chunk": (C.c_int, []),
    "kkt": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "kkt_many": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "check_kkt": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                            C.POINTER(C.c_int)]),
    "ray": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "get_unbnd_ray": (C.c_int, [C.c_void_p]),
    "farkas": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "farkas_many": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "add_dense_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "price_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_double)]),
    "price_cols_tile": (C.c_int, []),
    "del_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "del_cols_span": (C.c_int, []),
    "pool_create": (C.c_void_p, [C.c_int]),
    "pool_add_cols": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "pool_num_cols": (C.c_int, [C.c_void_p]),
    "pool_num_rows": (C.c_int, [C.c_void_p]),
    "pool_get_col": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "pool_delete": (None, [C.c_void_p]),
    "pool_price": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_ubyte), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                             C.POINTER(C.c_int)]),
    "pool_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "init_sift_parm": (None, [C.POINTER(capi.SiftParm), C.c_int]),
    "sift": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(capi.Smcp), C.POINTER(capi.SiftParm), C.POINTER(C.c_int),
                       C.POINTER(capi.SiftInfo)]),
    "set_mat_col": (None, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "get_mat_col": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "device_count": (C.c_int, []),
    "set_device": (C.c_int, [C.c_int]),
    "profile_enable": (None, [C.c_int]),
    "profile_reset": (None, []),
    "profile_update_ms": (C.c_double, []),
    "profile_update_launches": (C.c_longlong, []),
    "last_solve_ms": (C.c_double, [C.c_void_p]),
    "sync": (None, []),
    "set_tuning": (None, [C.c_int, C.c_int, C.c_int]),
    "set_batch_slots": (None, [C.c_int]),
    "set_persist": (None, [C.c_int]),
    "set_chain": (None, [C.c_int]),
    "set_cluster": (None, [C.c_int]),
    "cluster_stats": (None, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "set_dual_chain": (None, [C.c_int]),
    "set_dual_fused": (None, [C.c_int]),
    "dual_fused_stats": (None, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "set_refresh": (None, [C.c_int, C.c_double]),
    "get_refresh_cnt": (C.c_int, [C.c_void_p]),
    "row_residual": (C.c_double, [C.c_void_p]),
    "persist_stats": (None, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "last_error": (C.c_int, []),
    "bind_thread": (C.c_int, []),
    "persist_cycles": (None, [C.POINTER(C.c_ulonglong)]),
    "simplex_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "pack_size": (C.c_longlong, [C.c_void_p]),
    "pack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pack_size_from": (C.c_longlong, [C.c_void_p, C.c_void_p]),
    "pack_from": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

_api = None


def load_library():
    """dlopen the engine; raises if it has not been built (python -m mvolps_amd.build)."""
    # torch bundles its own HIP runtime; whichever libamdhip64 is loaded first serves the whole
    # process, and torch cannot find the GPU when it is not its own.  Load torch's first so that
    # the engine, torch.cuda and torch.distributed (RCCL) share one runtime.
    if os.environ.get("MVX_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmvolps_amd.so is missing (%s): build it with `python -m mvolps_amd.build`; "
            "there is no fallback path" % LIB_PATH
        )
    return C.CDLL(LIB_PATH)


def api():
    """Function table of the HIP engine (prefix mvx_)."""
    global _api
    if _api is None:
        _api = capi.LpApi(load_library(), "mvx_", _EXTRA)
    return _api


def require_device():
    a = api()
    n = a.device_count()
    if n <= 0:
        raise RuntimeError("no HIP device visible: the gfx950 engine cannot run and there is no CPU fallback")
    return n


def create_prob():
    require_device()
    return api().create()


def create_pool(m):
    """A column pool over m rows (capi.Pool); its model layer needs no device."""
    return capi.Pool(api(), m)
