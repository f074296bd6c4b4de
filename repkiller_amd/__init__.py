"""repkiller_amd -- MI355X-native repeat-fragment classifier (estebanpw/repkiller hot path).

Python binding over the C ABI in ``include/repkiller_amd.h`` (``librepkiller_amd.so``,
built in-tree by ``make -C repkiller_amd/csrc``).  The classification runs only
on a gfx950 GPU through hand-written HIP kernels; there is no CPU fallback --
:class:`Context` raises if the library or the device is missing.

Mapping to the reference (``/root/reference/src``):

=====================================  ============================================
reference                              here
=====================================  ============================================
``FragmentsDatabase(ifstream&, ...)``  :class:`FragmentsDatabase` (``rk_db_load_csv``;
                                       with ``ctx=`` parsed on the GPU,
                                       ``rk_db_load_csv_device``)
``generate_fragment_groups`` +         :meth:`Context.classify` /
``generate_diagonal_func`` +           :meth:`Context.classify_device`
``sort_groups`` + repeat flag          (``rk_classify`` / ``rk_classify_device``)
``save_all_frag_pairs``                :meth:`FragmentsDatabase.save_all_frag_pairs`
                                       (on the GPU: ``save_all_frag_pairs_device``,
                                       ``rk_db_write_csv_device``)
``SaverQueue``                         :class:`SaverQueue` (``rk_saver_*``)
one ``FragmentsDatabase`` per file of  :class:`FragmentsDatabaseSet` (``rk_dbset_*``: parsed,
an all-against-all run                 classified and saved on the GPU as one batch)
=====================================  ============================================
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RK_LIB=<path>: load another build of the library (A/B measurements)
LIB_PATH = os.environ.get("RK_LIB") or os.path.join(_HERE, "librepkiller_amd.so")
CLI_PATH = os.path.join(_HERE, "bin", "rk_repkiller")

RK_OK = 0
N_PHASES = 10  # RK_N_PHASES
STATUS = {
    0: "RK_OK", -1: "RK_E_ARG", -2: "RK_E_IO", -3: "RK_E_COUNT", -4: "RK_E_UB_BUCKET",
    -5: "RK_E_UB_CENTER", -6: "RK_E_NOMEM", -7: "RK_E_HIP", -8: "RK_E_NODEVICE",
    -9: "RK_E_TOO_MANY", -10: "RK_E_INTERNAL", -11: "RK_E_PEER",
}

# every symbol include/repkiller_amd.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "rk_create", "rk_destroy", "rk_last_error", "rk_classify", "rk_classify_device",
    "rk_classify_pairs", "rk_classify_device_pairs",
    "rk_get_stats", "rk_std_sort_segments", "rk_set_profiling", "rk_get_phase_ms", "rk_reset_phases", "rk_phase_name",
    "rk_get_kernel_timing", "rk_kernel_count", "rk_kernel_name",
    "rk_db_load_csv", "rk_db_free", "rk_db_view", "rk_db_write_csv",
    "rk_db_save_soa", "rk_db_load_soa", "rk_saver_start", "rk_saver_add", "rk_saver_stop", "rk_synth_generate",
    "rk_synth_write_csv", "rk_comm_create_host", "rk_comm_rccl_id", "rk_comm_create_rccl",
    "rk_comm_destroy", "rk_comm_last_error", "rk_classify_sharded", "rk_get_shard_stats",
    "rk_shard_copy_result", "rk_comm_create_local", "rk_classify_sharded_host",
    "rk_comm_abandon", "rk_set_pipeline",
    "rk_classify_batch", "rk_classify_device_batch", "rk_batch_layout", "rk_get_batch_stats",
    "rk_db_load_csv_device", "rk_db_device_view", "rk_classify_db_pairs", "rk_get_ingress_stats",
    "rk_db_write_csv_device", "rk_classify_db_pairs_to_csv", "rk_get_egress_stats",
    "rk_dbset_load_csv_device", "rk_dbset_free", "rk_dbset_view", "rk_classify_dbset",
    "rk_dbset_write_csv_device", "rk_classify_dbset_to_csv", "rk_dbset_write_csv",
    "rk_result_select", "rk_batch_result_select", "rk_get_select_stats",
    "rk_classify_db_pairs_to_csv_keep", "rk_classify_dbset_to_csv_keep",
)
# declared too, returning uint32_t (sizes the device CSV parser was built with)
EXPORTS_U32 = ("rk_csv_max_line", "rk_csv_tile", "rk_select_tile")
RK_DB_KEEP_DEVICE = 1
RK_DB_KEEP_ROWS = 3  # all nine columns resident: the device egress formats from them
RK_RES_DEVICE = 1    # rk_db_write_csv_device: the result arrays are device pointers
# selection by repeat flag (RK_KEEP_*): bit f keeps the rows whose flag is f
KEEP_SINGLETON, KEEP_REPRESENTATIVE, KEEP_REPEATED = 1, 2, 4
KEEP_UNIQUE = 3  # the repeat-free set: one row per group
KEEP_ALL = 7


class RkError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"{STATUS.get(code, code)}{': ' + msg if msg else ''}")


_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


class FragsSoA(ctypes.Structure):
    _fields_ = [("x_start", ctypes.c_void_p), ("y_start", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("strand", ctypes.c_void_p), ("n", ctypes.c_uint64)]


class Params(ctypes.Structure):
    _fields_ = [("len_x_hdr", ctypes.c_uint64), ("len_y_hdr", ctypes.c_uint64),
                ("len_ratio", ctypes.c_double), ("pos_ratio", ctypes.c_double)]


class Result(ctypes.Structure):
    _fields_ = [("out_order", ctypes.c_void_p), ("gid", ctypes.c_void_p),
                ("repval", ctypes.c_void_p), ("n_out", ctypes.c_uint64),
                ("n_groups", ctypes.c_uint64)]


class Stats(ctypes.Structure):
    _fields_ = [("n_in", ctypes.c_uint64), ("n_proc", ctypes.c_uint64),
                ("n_groups", ctypes.c_uint64), ("x_sweeps", ctypes.c_uint32),
                ("y_sweeps", ctypes.c_uint32), ("jump_rounds", ctypes.c_uint32),
                ("x_hits", ctypes.c_uint64), ("y_hits", ctypes.c_uint64),
                ("device_ms", ctypes.c_double), ("pipeline", ctypes.c_uint32),
                ("record_fallback", ctypes.c_uint32), ("h2d_ms", ctypes.c_double),
                ("d2h_ms", ctypes.c_double), ("wire", ctypes.c_uint32),
                ("sweep_repeats", ctypes.c_uint32), ("numa_input", ctypes.c_int32),
                ("numa_threads", ctypes.c_int32), ("numa_staging", ctypes.c_int32),
                ("numa_gpu", ctypes.c_int32)]


class BatchParams(ctypes.Structure):
    _fields_ = [("nsets", ctypes.c_uint32), ("set_off", ctypes.c_void_p),
                ("len_x_hdr", ctypes.c_void_p), ("len_y_hdr", ctypes.c_void_p),
                ("len_ratio", ctypes.c_double), ("pos_ratio", ctypes.c_double)]


class BatchResult(ctypes.Structure):
    _fields_ = [("out_order", ctypes.c_void_p), ("gid", ctypes.c_void_p),
                ("repval", ctypes.c_void_p), ("n_out", ctypes.c_void_p),
                ("n_groups", ctypes.c_void_p)]


class BatchStats(ctypes.Structure):
    _fields_ = [("sub_batches", ctypes.c_uint32), ("looped_sets", ctypes.c_uint32),
                ("batched_sets", ctypes.c_uint32), ("device_ms", ctypes.c_double)]


class IngressStats(ctypes.Structure):
    _fields_ = [("body_bytes", ctypes.c_uint64), ("lines", ctypes.c_uint64),
                ("accepted", ctypes.c_uint64), ("host_lines", ctypes.c_uint64),
                ("windows", ctypes.c_uint32), ("h2d_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double), ("host_fix_ms", ctypes.c_double),
                ("d2h_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class EgressStats(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("host_rows", ctypes.c_uint64), ("chunks", ctypes.c_uint32),
                ("upload_ms", ctypes.c_double), ("device_ms", ctypes.c_double),
                ("host_fix_ms", ctypes.c_double), ("d2h_write_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class SelectStats(ctypes.Structure):
    _fields_ = [("rows_in", ctypes.c_uint64), ("by_flag", ctypes.c_uint64 * 4),
                ("kept", ctypes.c_uint64), ("sets", ctypes.c_uint32),
                ("device_ms", ctypes.c_double)]


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_uint64)
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_uint64))


class CommHostOps(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allgather", ALLGATHER_FN),
                ("alltoallv", ALLTOALLV_FN)]


class ShardResult(ctypes.Structure):
    _fields_ = [("out_order", ctypes.c_void_p), ("gid", ctypes.c_void_p),
                ("repval", ctypes.c_void_p), ("n_out", ctypes.c_uint64),
                ("out_offset", ctypes.c_uint64), ("n_out_total", ctypes.c_uint64),
                ("n_groups", ctypes.c_uint64)]


class ShardStats(ctypes.Structure):
    _fields_ = [("n_in", ctypes.c_uint64), ("n_total", ctypes.c_uint64),
                ("n_slice", ctypes.c_uint64), ("x_ghosts", ctypes.c_uint64),
                ("y_entries", ctypes.c_uint64), ("x_rounds", ctypes.c_uint32),
                ("y_rounds", ctypes.c_uint32), ("x_reruns", ctypes.c_uint32),
                ("y_reruns", ctypes.c_uint32), ("root_rounds", ctypes.c_uint32),
                ("bytes_sent", ctypes.c_uint64), ("ms_total", ctypes.c_double),
                ("ms_ingress", ctypes.c_double), ("ms_x", ctypes.c_double),
                ("ms_y", ctypes.c_double), ("ms_roots", ctypes.c_double),
                ("ms_members", ctypes.c_double), ("generic_driver", ctypes.c_uint32),
                ("order_split", ctypes.c_uint32), ("gathers", ctypes.c_uint32),
                ("exchanges", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
                ("agree_skipped", ctypes.c_uint32), ("fast_path", ctypes.c_uint32),
                ("fast_retry", ctypes.c_uint32), ("fast_stages", ctypes.c_uint32)]


class SynthParams(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("genome_len", ctypes.c_uint64),
                ("seed", ctypes.c_uint64), ("family_frac", ctypes.c_double),
                ("copies_lo", ctypes.c_uint32), ("copies_hi", ctypes.c_uint32)]


_lib = None


def load_library() -> ctypes.CDLL:
    """Load librepkiller_amd.so; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; when it is imported AFTER this library
    # the process ends up with two HIP runtimes and torch.cuda cannot initialise.
    # Importing it first makes both share one runtime (SONAME match).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} missing: run `make -C repkiller_amd/csrc` "
                           "(or __graft_entry__.build())")
    lib = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    sig = {
        "rk_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int]),
        "rk_destroy": (None, [vp]),
        "rk_last_error": (ctypes.c_char_p, [vp]),
        "rk_classify": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA), ctypes.POINTER(Params),
                                       ctypes.POINTER(Result)]),
        "rk_classify_device": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA),
                                              ctypes.POINTER(Params), ctypes.POINTER(Result)]),
        "rk_classify_pairs": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA),
                                             ctypes.POINTER(Params), ctypes.c_uint32,
                                             ctypes.POINTER(Result)]),
        "rk_classify_device_pairs": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA),
                                                    ctypes.POINTER(Params), ctypes.c_uint32,
                                                    ctypes.POINTER(Result)]),
        "rk_get_stats": (ctypes.c_int, [vp, ctypes.POINTER(Stats)]),
        "rk_set_profiling": (ctypes.c_int, [vp, ctypes.c_int]),
        "rk_std_sort_segments": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32,
                                                vp]),
        "rk_get_phase_ms": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), _u32p]),
        "rk_reset_phases": (ctypes.c_int, [vp]),
        "rk_get_kernel_timing": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double), _u64p]),
        "rk_kernel_count": (ctypes.c_int, []),
        "rk_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
        "rk_phase_name": (ctypes.c_char_p, [ctypes.c_int]),
        "rk_db_load_csv": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(vp)]),
        "rk_db_free": (None, [vp]),
        "rk_db_save_soa": (ctypes.c_int, [vp, ctypes.c_char_p]),
        "rk_db_load_soa": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(vp)]),
        "rk_db_view": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA), _u64p, _u64p, _u64p]),
        "rk_db_write_csv": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.POINTER(Result)]),
        "rk_saver_start": (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
        "rk_saver_add": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.POINTER(Result),
                                        ctypes.c_uint64]),
        "rk_saver_stop": (ctypes.c_int, [vp]),
        "rk_synth_generate": (ctypes.c_int, [ctypes.POINTER(SynthParams), vp, vp, vp, vp, vp]),
        "rk_synth_write_csv": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, vp, vp, vp, vp,
                                              vp, ctypes.c_uint64, ctypes.c_uint64]),
        "rk_comm_create_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(CommHostOps), ctypes.POINTER(vp)]),
        "rk_comm_rccl_id": (ctypes.c_int, [vp]),
        "rk_comm_create_rccl": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                               ctypes.POINTER(vp)]),
        "rk_comm_destroy": (None, [vp]),
        "rk_comm_last_error": (ctypes.c_char_p, [vp]),
        "rk_comm_abandon": (ctypes.c_int, [vp, ctypes.c_int]),
        "rk_set_pipeline": (ctypes.c_int, [vp, ctypes.c_int]),
        "rk_classify_sharded": (ctypes.c_int, [vp, vp, ctypes.POINTER(FragsSoA),
                                               ctypes.POINTER(Params), ctypes.c_int32,
                                               ctypes.POINTER(ShardResult)]),
        "rk_get_shard_stats": (ctypes.c_int, [vp, ctypes.POINTER(ShardStats)]),
        "rk_comm_create_local": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp)]),
        "rk_classify_sharded_host": (ctypes.c_int, [vp, vp, ctypes.POINTER(FragsSoA),
                                                    ctypes.POINTER(Params), ctypes.c_int32,
                                                    ctypes.POINTER(ShardResult)]),
        "rk_shard_copy_result": (ctypes.c_int, [vp, ctypes.POINTER(ShardResult), vp, vp, vp]),
        "rk_classify_batch": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA),
                                             ctypes.POINTER(BatchParams),
                                             ctypes.POINTER(BatchResult)]),
        "rk_classify_device_batch": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA),
                                                    ctypes.POINTER(BatchParams),
                                                    ctypes.POINTER(BatchResult)]),
        "rk_batch_layout": (ctypes.c_int, [ctypes.c_uint32, vp, vp, vp, vp]),
        "rk_get_batch_stats": (ctypes.c_int, [vp, ctypes.POINTER(BatchStats)]),
        "rk_db_load_csv_device": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_uint32,
                                                 ctypes.POINTER(vp)]),
        "rk_db_device_view": (ctypes.c_int, [vp, ctypes.POINTER(FragsSoA)]),
        "rk_classify_db_pairs": (ctypes.c_int, [vp, vp, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double), ctypes.c_uint32,
                                                ctypes.POINTER(Result)]),
        "rk_get_ingress_stats": (ctypes.c_int, [vp, ctypes.POINTER(IngressStats)]),
        "rk_db_write_csv_device": (ctypes.c_int, [vp, vp, ctypes.c_char_p, ctypes.POINTER(Result),
                                                  ctypes.c_uint32]),
        "rk_classify_db_pairs_to_csv": (ctypes.c_int, [vp, vp, ctypes.POINTER(ctypes.c_double),
                                                       ctypes.POINTER(ctypes.c_double),
                                                       ctypes.c_uint32,
                                                       ctypes.POINTER(ctypes.c_char_p), _u64p,
                                                       _u64p]),
        "rk_get_egress_stats": (ctypes.c_int, [vp, ctypes.POINTER(EgressStats)]),
        "rk_dbset_load_csv_device": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p),
                                                    ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.POINTER(vp)]),
        "rk_dbset_free": (None, [vp]),
        "rk_dbset_view": (ctypes.c_int, [vp, _u32p, ctypes.POINTER(_u64p), ctypes.POINTER(_u64p),
                                         ctypes.POINTER(_u64p), ctypes.POINTER(_u64p),
                                         ctypes.POINTER(FragsSoA), ctypes.POINTER(FragsSoA)]),
        "rk_classify_dbset": (ctypes.c_int, [vp, vp, ctypes.c_double, ctypes.c_double,
                                             ctypes.POINTER(BatchResult)]),
        "rk_dbset_write_csv": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_char_p,
                                              ctypes.POINTER(Result)]),
        "rk_dbset_write_csv_device": (ctypes.c_int, [vp, vp, ctypes.POINTER(ctypes.c_char_p),
                                                     ctypes.POINTER(BatchResult),
                                                     ctypes.c_uint32]),
        "rk_classify_dbset_to_csv": (ctypes.c_int, [vp, vp, ctypes.c_double, ctypes.c_double,
                                                    ctypes.POINTER(ctypes.c_char_p), _u64p,
                                                    _u64p]),
        "rk_result_select": (ctypes.c_int, [vp, ctypes.POINTER(Result), ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.POINTER(Result)]),
        "rk_batch_result_select": (ctypes.c_int, [vp, ctypes.c_uint32, vp,
                                                  ctypes.POINTER(BatchResult), ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.POINTER(BatchResult)]),
        "rk_get_select_stats": (ctypes.c_int, [vp, ctypes.POINTER(SelectStats)]),
        "rk_classify_db_pairs_to_csv_keep": (ctypes.c_int, [vp, vp, ctypes.POINTER(ctypes.c_double),
                                                            ctypes.POINTER(ctypes.c_double),
                                                            ctypes.c_uint32,
                                                            ctypes.POINTER(ctypes.c_char_p),
                                                            ctypes.c_uint32, _u64p, _u64p, _u64p]),
        "rk_classify_dbset_to_csv_keep": (ctypes.c_int, [vp, vp, ctypes.c_double, ctypes.c_double,
                                                         ctypes.POINTER(ctypes.c_char_p),
                                                         ctypes.c_uint32, _u64p, _u64p, _u64p]),
        "rk_select_tile": (ctypes.c_uint32, []),
        "rk_csv_max_line": (ctypes.c_uint32, []),
        "rk_csv_tile": (ctypes.c_uint32, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def _check(rc: int, msg: str = ""):
    if rc != RK_OK:
        raise RkError(rc, msg)


# --------------------------------------------------------------- synthetic --

@dataclass
class Frags:
    """Fragments in FILE order (what FragmentsDatabase reads, SoA)."""
    x_start: np.ndarray
    y_start: np.ndarray
    length: np.ndarray
    strand: np.ndarray
    ident: np.ndarray | None = None

    @property
    def n(self) -> int:
        return int(self.x_start.shape[0])


def synth(n: int, genome_len: int, seed: int, family_frac: float = 0.8,
          copies: tuple[int, int] = (2, 30), with_ident: bool = True) -> Frags:
    """Deterministic synthetic fragment set (SURVEY.md §8d generator).
    with_ident=False skips the identity column (only the CSV writer reads it)."""
    lib = load_library()
    f = Frags(np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint64),
              np.empty(n, np.uint8), np.empty(n, np.uint64) if with_ident else None)
    p = SynthParams(n, genome_len, seed, family_frac, copies[0], copies[1])
    _check(lib.rk_synth_generate(ctypes.byref(p), _ptr(f.x_start), _ptr(f.y_start),
                                 _ptr(f.length), _ptr(f.strand),
                                 _ptr(f.ident) if f.ident is not None else 0))
    return f


def write_input_csv(path: str, f: Frags, len_x_hdr: int, len_y_hdr: int) -> None:
    lib = load_library()
    ident = f.ident if f.ident is not None else f.length
    _check(lib.rk_synth_write_csv(path.encode(), f.n, _ptr(f.x_start), _ptr(f.y_start),
                                  _ptr(f.length), _ptr(f.strand), _ptr(ident),
                                  len_x_hdr, len_y_hdr))


# ------------------------------------------------------------------ ingress --

@dataclass
class ClassifyResult:
    """All arrays in OUTPUT order (length n_out): row k of the reference's CSV is
    input row out_order[k], with group id gid[k] and repeat flag repval[k]."""
    gid: np.ndarray        # uint32 group id (block column, creation order)
    repval: np.ndarray     # uint8 0 singleton / 1 representative / 2 repeated
    out_order: np.ndarray  # uint32 input row
    n_groups: int

    def as_struct(self) -> Result:
        return Result(_ptr(self.out_order), _ptr(self.gid), _ptr(self.repval),
                      int(self.out_order.shape[0]), self.n_groups)


def select(res: ClassifyResult, keep: int) -> ClassifyResult:
    """The rows of `res` whose repeat flag is in `keep` (KEEP_*), in res's order
    (rk_result_select on the host: no device is touched).  Group ids are not
    renumbered; KEEP_UNIQUE keeps one row per group."""
    n = int(res.out_order.shape[0])
    src = ClassifyResult(np.ascontiguousarray(res.gid, np.uint32),
                         np.ascontiguousarray(res.repval, np.uint8),
                         np.ascontiguousarray(res.out_order, np.uint32), res.n_groups)
    gid, rep, order = np.empty(n, np.uint32), np.empty(n, np.uint8), np.empty(n, np.uint32)
    r, out = src.as_struct(), Result(_ptr(order), _ptr(gid), _ptr(rep), 0, 0)
    _check(load_library().rk_result_select(None, ctypes.byref(r), keep, 0, ctypes.byref(out)),
           "rk_result_select")
    k = int(out.n_out)
    return ClassifyResult(gid[:k].copy(), rep[:k].copy(), order[:k].copy(), int(out.n_groups))


def select_tile() -> int:
    """Slots of a tile of the device selection (rk_select_tile)."""
    return int(load_library().rk_select_tile())


class FragmentsDatabase:
    """Parsed fragment CSV (FragmentsDatabase.cpp:17-101 acceptance rules)."""

    def __init__(self, path: str, soa: bool = False, ctx: "Context | None" = None,
                 keep_device: bool = False, keep_rows: bool = False):
        """path: the fragment CSV, or with soa=True a binary SoA cache written by
        save_soa (the parsed columns: no parse at all).  With ctx the CSV is
        parsed on that context's GPU (rk_db_load_csv_device); keep_device=True
        also keeps the four classification columns in HBM (device_view,
        Context.classify_db); keep_rows=True keeps all nine (RK_DB_KEEP_ROWS:
        save_all_frag_pairs_device, Context.classify_db_to_csv)."""
        lib = load_library()
        h = ctypes.c_void_p()
        if ctx is None and (keep_device or keep_rows):
            raise ValueError("keep_device / keep_rows need ctx (the device parse)")
        if ctx is not None:
            if soa:
                raise ValueError("a SoA cache is not parsed: ctx does not apply")
            rc = lib.rk_db_load_csv_device(ctx._h, path.encode(),
                                           RK_DB_KEEP_ROWS if keep_rows else
                                           RK_DB_KEEP_DEVICE if keep_device else 0,
                                           ctypes.byref(h))
            if rc not in (0, -2, -3):
                raise RkError(rc, ctx.last_error())
        else:
            rc = (lib.rk_db_load_soa if soa else lib.rk_db_load_csv)(path.encode(),
                                                                     ctypes.byref(h))
        if rc == -2:
            raise RkError(rc, f"Could not open input file {path}.")
        if rc == -3:
            raise RkError(rc, "Unexpected number of fragments")
        if rc == -1 and soa:
            raise RkError(rc, f"{path} is not a complete SoA cache file")
        _check(rc)
        self._h = h
        soa = FragsSoA()
        lx, ly, tot = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib.rk_db_view(h, ctypes.byref(soa), ctypes.byref(lx), ctypes.byref(ly),
                              ctypes.byref(tot)))
        self.len_x_hdr, self.len_y_hdr, self.total_hdr = lx.value, ly.value, tot.value
        n = soa.n

        def view(ptr, dtype, count):
            if count == 0:
                return np.empty(0, dtype)
            buf = (ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype).copy()

        self.frags = Frags(view(soa.x_start, np.uint64, n), view(soa.y_start, np.uint64, n),
                           view(soa.length, np.uint64, n), view(soa.strand, np.uint8, n))

    @classmethod
    def load_soa(cls, path: str) -> "FragmentsDatabase":
        """A database from a binary SoA cache (rk_db_load_soa)."""
        return cls(path, soa=True)

    def save_soa(self, path: str) -> None:
        """The parsed columns as a binary SoA cache (rk_db_save_soa)."""
        rc = load_library().rk_db_save_soa(self._h, path.encode())
        if rc == -2:
            raise RkError(rc, f"Could not write {path}")
        _check(rc)

    def device_view(self) -> dict:
        """The resident columns of a database loaded with keep_device=True
        (rk_db_device_view): device addresses of x_start, y_start, length,
        strand and the row count n, valid until close()."""
        soa = FragsSoA()
        _check(load_library().rk_db_device_view(self._h, ctypes.byref(soa)),
               "the database was not loaded with keep_device=True")
        return {"x_start": soa.x_start or 0, "y_start": soa.y_start or 0,
                "length": soa.length or 0, "strand": soa.strand or 0, "n": int(soa.n)}

    def getTotalFrags(self) -> int:  # FragmentsDatabase.h:32
        return self.frags.n

    def getA(self) -> int:  # FragmentsDatabase.h:23 (vsize)
        return 1 + (self.len_x_hdr + 1) // 10

    def save_all_frag_pairs(self, path: str, res: ClassifyResult) -> None:
        """commonFunctions.cpp:131-146 (header echo + one line per member)."""
        r = res.as_struct()
        rc = load_library().rk_db_write_csv(self._h, path.encode(), ctypes.byref(r))
        if rc == -2:
            raise RkError(rc, "Could not open output directory " + path)
        _check(rc)

    def save_all_frag_pairs_device(self, ctx: "Context", path: str, res) -> None:
        """save_all_frag_pairs formatted on the GPU (rk_db_write_csv_device) from
        the columns a keep_rows=True database keeps resident.  res: a
        ClassifyResult (host arrays, uploaded first), or a tuple of three device
        tensors (out_order, gid, repval) whose length is the row count."""
        if isinstance(res, ClassifyResult):
            r, flags = res.as_struct(), 0
        else:
            order, gid, rep = res
            r = Result(order.data_ptr(), gid.data_ptr(), rep.data_ptr(), int(order.shape[0]), 0)
            flags = RK_RES_DEVICE
        rc = load_library().rk_db_write_csv_device(ctx._h, self._h, path.encode(),
                                                   ctypes.byref(r), flags)
        if rc == -2:
            raise RkError(rc, "Could not open output directory " + path)
        if rc != RK_OK:
            raise RkError(rc, ctx.last_error())

    def close(self):
        if getattr(self, "_h", None):
            load_library().rk_db_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FragmentsDatabaseSet:
    """One FragmentsDatabase per listed CSV, parsed on the GPU as one combined
    database (rk_dbset_load_csv_device): set k's rows are rows
    [set_off[k], set_off[k + 1]) of the combined columns, in file order."""

    def __init__(self, paths, ctx: "Context", keep_device: bool = False,
                 keep_rows: bool = False):
        """keep_device=True keeps the four classification columns in HBM
        (Context.classify_dbset); keep_rows=True keeps all nine
        (save_all_device, Context.classify_dbset_to_csv)."""
        lib = load_library()
        self.paths = [str(p) for p in paths]
        ns = len(self.paths)
        arr = (ctypes.c_char_p * max(ns, 1))(*[p.encode() for p in self.paths])
        h = ctypes.c_void_p()
        rc = lib.rk_dbset_load_csv_device(ctx._h, arr, ns,
                                          RK_DB_KEEP_ROWS if keep_rows else
                                          RK_DB_KEEP_DEVICE if keep_device else 0,
                                          ctypes.byref(h))
        if rc != RK_OK:
            raise RkError(rc, ctx.last_error())
        self._h = h
        n = ctypes.c_uint32()
        off, lx, ly, tot = _u64p(), _u64p(), _u64p(), _u64p()
        soa = FragsSoA()
        _check(lib.rk_dbset_view(h, ctypes.byref(n), ctypes.byref(off), ctypes.byref(lx),
                                 ctypes.byref(ly), ctypes.byref(tot), ctypes.byref(soa), None))
        self.nsets = int(n.value)

        def arr64(p, count):
            if count == 0:
                return np.empty(0, np.uint64)
            return np.ctypeslib.as_array(p, shape=(count,)).copy()

        self.set_off = arr64(off, self.nsets + 1)
        self.len_x_hdr = arr64(lx, self.nsets)
        self.len_y_hdr = arr64(ly, self.nsets)
        self.total_hdr = arr64(tot, self.nsets)
        rows = int(soa.n)

        def view(ptr, dtype, count):
            if count == 0:
                return np.empty(0, dtype)
            buf = (ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype)

        # the combined host columns, borrowed from the library until close()
        # (not copied: a batch's columns are gigabytes)
        self._host = Frags(view(soa.x_start, np.uint64, rows), view(soa.y_start, np.uint64, rows),
                           view(soa.length, np.uint64, rows), view(soa.strand, np.uint8, rows))

    @property
    def n(self) -> int:
        """Rows of the combined database (= set_off[nsets])."""
        return self._host.n

    def frags(self, k: int) -> Frags:
        """Host rows of set k (what FragmentsDatabase(paths[k]).frags holds), copied."""
        a, b = int(self.set_off[k]), int(self.set_off[k + 1])
        h = self._host
        return Frags(h.x_start[a:b].copy(), h.y_start[a:b].copy(), h.length[a:b].copy(),
                     h.strand[a:b].copy())

    def device_view(self) -> dict:
        """The resident combined columns of a set loaded with keep_device=True:
        device addresses of x_start, y_start, length, strand and the row count."""
        soa = FragsSoA()
        _check(load_library().rk_dbset_view(self._h, None, None, None, None, None, None,
                                            ctypes.byref(soa)),
               "the set was not loaded with keep_device=True")
        return {"x_start": soa.x_start or 0, "y_start": soa.y_start or 0,
                "length": soa.length or 0, "strand": soa.strand or 0, "n": int(soa.n)}

    def save_set(self, k: int, path: str, res: ClassifyResult) -> None:
        """The host save of set k (rk_dbset_write_csv): save_all_frag_pairs from
        the combined host columns under the set's own header."""
        r = res.as_struct()
        rc = load_library().rk_dbset_write_csv(self._h, k, str(path).encode(), ctypes.byref(r))
        if rc == -2:
            raise RkError(rc, "Could not open output directory " + str(path))
        _check(rc)

    def save_all_device(self, ctx: "Context", paths, results) -> None:
        """save_all_frag_pairs for every set, formatted on the GPU
        (rk_dbset_write_csv_device): results[k] is set k's ClassifyResult and goes
        to paths[k].  Needs keep_rows=True."""
        paths, results = [str(p) for p in paths], list(results)
        if len(paths) != self.nsets or len(results) != self.nsets:
            raise ValueError("save_all_device: one path and one result per set")
        n = self.n
        order, gid, rep = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        n_out = np.zeros(max(self.nsets, 1), np.uint64)
        for k, r in enumerate(results):
            a, m = int(self.set_off[k]), int(r.out_order.shape[0])
            if a + m > int(self.set_off[k + 1]):
                raise ValueError(f"save_all_device: set {k}'s result has more rows than the set")
            order[a:a + m], gid[a:a + m], rep[a:a + m] = r.out_order, r.gid, r.repval
            n_out[k] = m
        res = BatchResult(_ptr(order), _ptr(gid), _ptr(rep), n_out.ctypes.data, 0)
        arr = (ctypes.c_char_p * max(self.nsets, 1))(*[p.encode() for p in paths])
        rc = load_library().rk_dbset_write_csv_device(ctx._h, self._h, arr, ctypes.byref(res), 0)
        if rc != RK_OK:
            raise RkError(rc, ctx.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._host = Frags(np.empty(0, np.uint64), np.empty(0, np.uint64),
                               np.empty(0, np.uint64), np.empty(0, np.uint8))
            load_library().rk_dbset_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SaverQueue:
    """SaverQueue.h:37-41 -- background CSV writer (start / addRequest / stop)."""

    def __init__(self, db: FragmentsDatabase):
        self._db = db
        self._h = ctypes.c_void_p()
        _check(load_library().rk_saver_start(db._h, ctypes.byref(self._h)))

    def addRequest(self, path: str, res: ClassifyResult) -> None:
        r = res.as_struct()
        _check(load_library().rk_saver_add(self._h, path.encode(), ctypes.byref(r),
                                           int(res.gid.shape[0])))

    def stop(self) -> None:
        if self._h:
            rc = load_library().rk_saver_stop(self._h)
            self._h = None
            _check(rc)


# ----------------------------------------------------------- classification --

class Context:
    """One device + stream + workspace (rk_ctx).  GPU only."""

    def __init__(self, device: int = 0):
        lib = load_library()
        self._h = ctypes.c_void_p()
        rc = lib.rk_create(ctypes.byref(self._h), device)
        if rc != RK_OK:
            raise RkError(rc, f"rk_create(device={device}) failed: a gfx950 GPU is required "
                              "(no CPU fallback)")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load_library().rk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return load_library().rk_last_error(self._h).decode()

    def stats(self) -> dict:
        s = Stats()
        _check(load_library().rk_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def set_pipeline(self, pipeline: str) -> None:
        """'auto' (the record pipeline where rows pack into 16-B records) or
        'generic' (rk_set_pipeline)."""
        _check(load_library().rk_set_pipeline(self._h, {"auto": 0, "generic": 1}[pipeline]))

    def set_profiling(self, on: bool = True, only: str | None = None) -> None:
        """Phase events and launch timing on/off; `only` = a kernel name
        (rk_kernel_name) restricts the launch timing to that kernel."""
        lib = load_library()
        mode = int(bool(on))
        if on and only:
            names = [lib.rk_kernel_name(k).decode() for k in range(lib.rk_kernel_count())]
            mode = 2 + names.index(only)
        _check(lib.rk_set_profiling(self._h, mode))

    def reset_phases(self) -> None:
        _check(load_library().rk_reset_phases(self._h))

    def phases(self) -> dict:
        """{phase name: (accumulated device ms, calls)} since the last reset."""
        lib = load_library()
        ms = (ctypes.c_double * N_PHASES)()
        calls = (ctypes.c_uint32 * N_PHASES)()
        _check(lib.rk_get_phase_ms(self._h, ms, calls))
        return {lib.rk_phase_name(i).decode(): (ms[i], calls[i]) for i in range(N_PHASES)}

    def std_sort_segments(self, keys: np.ndarray, seg_off: np.ndarray) -> np.ndarray:
        """libstdc++ std::sort permutation of every segment of `keys`, on the GPU."""
        k = np.ascontiguousarray(keys, np.uint64)
        off = np.ascontiguousarray(seg_off, np.uint32)
        perm = np.empty(k.shape[0], np.uint32)
        rc = load_library().rk_std_sort_segments(self._h, _ptr(k), k.shape[0], _ptr(off),
                                                 off.shape[0] - 1, _ptr(perm))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return perm

    def kernel_timing(self) -> dict:
        """Per-kernel HIP-event timing while profiling:
        {name: {"total_ms", "algo_bytes", "launches"}} for kernels that ran."""
        lib = load_library()
        out = {}
        for k in range(lib.rk_kernel_count()):
            ms, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
            _check(lib.rk_get_kernel_timing(self._h, k, ctypes.byref(ms), ctypes.byref(by),
                                            ctypes.byref(n)))
            if n.value:
                out[lib.rk_kernel_name(k).decode()] = {"total_ms": ms.value, "algo_bytes": by.value,
                                                       "launches": n.value}
        return out

    def classify(self, f: Frags, len_x_hdr: int, len_y_hdr: int, len_ratio: float = 0.3,
                 pos_ratio: float = 0.3) -> ClassifyResult:
        """Host arrays in, host arrays out (rk_classify)."""
        n = f.n
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((f.x_start, np.uint64), (f.y_start, np.uint64), (f.length, np.uint64),
                 (f.strand, np.uint8))]
        soa = FragsSoA(_ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]), n)
        gid = np.empty(n, np.uint32)
        rep = np.empty(n, np.uint8)
        order = np.empty(n, np.uint32)
        res = Result(_ptr(order), _ptr(gid), _ptr(rep), 0, 0)
        prm = Params(len_x_hdr, len_y_hdr, len_ratio, pos_ratio)
        rc = load_library().rk_classify(self._h, ctypes.byref(soa), ctypes.byref(prm),
                                        ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        k = res.n_out
        return ClassifyResult(gid[:k].copy(), rep[:k].copy(), order[:k].copy(), int(res.n_groups))

    def classify_db(self, db: "FragmentsDatabase", len_ratio: float = 0.3,
                    pos_ratio: float = 0.3) -> ClassifyResult:
        """Classify a database loaded with keep_device=True from its resident
        columns: no upload (rk_classify_db_pairs)."""
        n = db.frags.n
        gid = np.empty(n, np.uint32)
        rep = np.empty(n, np.uint8)
        order = np.empty(n, np.uint32)
        res = Result(_ptr(order), _ptr(gid), _ptr(rep), 0, 0)
        lr, pr = ctypes.c_double(len_ratio), ctypes.c_double(pos_ratio)
        rc = load_library().rk_classify_db_pairs(self._h, db._h, ctypes.byref(lr),
                                                 ctypes.byref(pr), 1, ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        k = res.n_out
        return ClassifyResult(gid[:k].copy(), rep[:k].copy(), order[:k].copy(), int(res.n_groups))

    def classify_db_to_csv(self, db: "FragmentsDatabase", pairs, paths,
                           keep: int = KEEP_ALL, with_kept: bool = False) -> list:
        """Classify a keep_rows=True database at every (len_ratio, pos_ratio) of
        `pairs` and write pair i to paths[i] from the device: the result arrays
        never come to the host (rk_classify_db_pairs_to_csv_keep).  keep: the
        repeat flags whose rows are written (KEEP_*).  Returns [(n_out, n_groups)]
        per pair, or with with_kept=True [(n_out, n_groups, n_kept)], n_kept the
        rows written."""
        pairs, paths = list(pairs), list(paths)
        q = len(pairs)
        if q != len(paths):
            raise ValueError("classify_db_to_csv: one path per pair")
        lr = (ctypes.c_double * max(q, 1))(*[p[0] for p in pairs])
        pr = (ctypes.c_double * max(q, 1))(*[p[1] for p in pairs])
        ps = (ctypes.c_char_p * max(q, 1))(*[p.encode() for p in paths])
        n_out, n_groups = np.zeros(max(q, 1), np.uint64), np.zeros(max(q, 1), np.uint64)
        n_kept = np.zeros(max(q, 1), np.uint64)
        rc = load_library().rk_classify_db_pairs_to_csv_keep(
            self._h, db._h, lr, pr, q, ps, keep, n_out.ctypes.data_as(_u64p),
            n_groups.ctypes.data_as(_u64p), n_kept.ctypes.data_as(_u64p))
        if rc == -2:
            raise RkError(rc, "Could not open an output path of " + ", ".join(paths))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        if with_kept:
            return [(int(n_out[i]), int(n_groups[i]), int(n_kept[i])) for i in range(q)]
        return [(int(n_out[i]), int(n_groups[i])) for i in range(q)]

    def classify_dbset(self, dbs: "FragmentsDatabaseSet", len_ratio: float = 0.3,
                       pos_ratio: float = 0.3) -> list:
        """Classify every set of a keep_device=True FragmentsDatabaseSet from its
        resident columns in one batched call (rk_classify_dbset); one
        ClassifyResult per set, as classify_batch returns them."""
        n, ns = dbs.n, dbs.nsets
        gid, rep, order = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        n_out, n_groups = np.zeros(max(ns, 1), np.uint64), np.zeros(max(ns, 1), np.uint64)
        res = BatchResult(_ptr(order), _ptr(gid), _ptr(rep), n_out.ctypes.data,
                          n_groups.ctypes.data)
        rc = load_library().rk_classify_dbset(self._h, dbs._h, len_ratio, pos_ratio,
                                              ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        out = []
        for k in range(ns):
            a = int(dbs.set_off[k])
            b = a + int(n_out[k])
            out.append(ClassifyResult(gid[a:b].copy(), rep[a:b].copy(), order[a:b].copy(),
                                      int(n_groups[k])))
        return out

    def classify_dbset_to_csv(self, dbs: "FragmentsDatabaseSet", paths, len_ratio: float = 0.3,
                              pos_ratio: float = 0.3, keep: int = KEEP_ALL,
                              with_kept: bool = False) -> tuple:
        """Classify a keep_rows=True FragmentsDatabaseSet and write set k to
        paths[k] from the device (rk_classify_dbset_to_csv_keep): the result arrays
        never come to the host.  keep: the repeat flags whose rows are written
        (KEEP_*).  Returns (n_out, n_groups) as uint64 arrays, or with
        with_kept=True (n_out, n_groups, n_kept), n_kept the rows written per set."""
        paths = [str(p) for p in paths]
        ns = dbs.nsets
        if len(paths) != ns:
            raise ValueError("classify_dbset_to_csv: one path per set")
        arr = (ctypes.c_char_p * max(ns, 1))(*[p.encode() for p in paths])
        n_out, n_groups = np.zeros(max(ns, 1), np.uint64), np.zeros(max(ns, 1), np.uint64)
        kept = np.zeros(max(ns, 1), np.uint64)
        rc = load_library().rk_classify_dbset_to_csv_keep(
            self._h, dbs._h, len_ratio, pos_ratio, arr, keep, n_out.ctypes.data_as(_u64p),
            n_groups.ctypes.data_as(_u64p), kept.ctypes.data_as(_u64p))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        if with_kept:
            return n_out[:ns], n_groups[:ns], kept[:ns]
        return n_out[:ns], n_groups[:ns]

    def select_device(self, out_order, gid, repval, n_out: int, keep: int, out_order_out,
                      gid_out, repval_out) -> int:
        """The device selection of one result (rk_result_select, RK_RES_DEVICE):
        device tensors in, the kept rows into the first entries of the three
        output tensors (n_out entries each; the rest is not written).  Returns
        the kept count."""
        r = Result(out_order.data_ptr(), gid.data_ptr(), repval.data_ptr(), int(n_out), 0)
        o = Result(out_order_out.data_ptr(), gid_out.data_ptr(), repval_out.data_ptr(), 0, 0)
        rc = load_library().rk_result_select(self._h, ctypes.byref(r), keep, RK_RES_DEVICE,
                                             ctypes.byref(o))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return int(o.n_out)

    def select_batch(self, set_off, n_out, out_order, gid, repval, keep: int, out_order_out,
                     gid_out, repval_out) -> np.ndarray:
        """The selection per set of a result in rk_batch_result layout
        (rk_batch_result_select): numpy arrays (selected on the host) or device
        tensors.  Set k's kept rows go to set_off[k] on in the output arrays;
        returns the kept counts per set (uint64)."""
        off = np.ascontiguousarray(set_off, np.uint64)
        ns = off.shape[0] - 1
        no = np.ascontiguousarray(n_out, np.uint64)
        kept = np.zeros(max(ns, 1), np.uint64)
        arrs = (out_order, gid, repval, out_order_out, gid_out, repval_out)
        dev = not isinstance(out_order, np.ndarray)
        p = [a.data_ptr() if dev else _ptr(a) for a in arrs]
        res = BatchResult(p[0], p[1], p[2], _ptr(no), 0)
        out = BatchResult(p[3], p[4], p[5], kept.ctypes.data, 0)
        rc = load_library().rk_batch_result_select(self._h, ns, off.ctypes.data, ctypes.byref(res),
                                                   keep, RK_RES_DEVICE if dev else 0,
                                                   ctypes.byref(out))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return kept[:ns]

    def select_stats(self) -> dict:
        """The last selection on this context (rk_get_select_stats)."""
        s = SelectStats()
        _check(load_library().rk_get_select_stats(self._h, ctypes.byref(s)))
        return {"rows_in": s.rows_in, "by_flag": [int(v) for v in s.by_flag], "kept": s.kept,
                "sets": s.sets, "device_ms": s.device_ms}

    def egress_stats(self) -> dict:
        """The last device CSV save on this context (rk_get_egress_stats)."""
        s = EgressStats()
        _check(load_library().rk_get_egress_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in EgressStats._fields_}

    def ingress_stats(self) -> dict:
        """The last device CSV load on this context (rk_get_ingress_stats)."""
        s = IngressStats()
        _check(load_library().rk_get_ingress_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in IngressStats._fields_}

    def classify_into(self, f: Frags, len_x_hdr: int, len_y_hdr: int, len_ratio: float,
                      pos_ratio: float, gid: np.ndarray, rep: np.ndarray,
                      order: np.ndarray) -> tuple:
        """rk_classify into caller-owned host arrays (no copies; the arrays may
        be page-locked, e.g. views of pinned torch tensors).  Returns
        (n_out, n_groups)."""
        n = f.n
        for a, t in ((f.x_start, np.uint64), (f.y_start, np.uint64), (f.length, np.uint64),
                     (f.strand, np.uint8), (gid, np.uint32), (rep, np.uint8), (order, np.uint32)):
            if a.dtype != t or not a.flags.c_contiguous or a.shape[0] < n:
                raise ValueError("classify_into: contiguous arrays of the ABI dtypes required")
        soa = FragsSoA(_ptr(f.x_start), _ptr(f.y_start), _ptr(f.length), _ptr(f.strand), n)
        res = Result(_ptr(order), _ptr(gid), _ptr(rep), 0, 0)
        prm = Params(len_x_hdr, len_y_hdr, len_ratio, pos_ratio)
        rc = load_library().rk_classify(self._h, ctypes.byref(soa), ctypes.byref(prm),
                                        ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return int(res.n_out), int(res.n_groups)

    def classify_pairs(self, f: Frags, len_x_hdr: int, len_y_hdr: int,
                       pairs) -> list:
        """Several (len_ratio, pos_ratio) pairs over one fragment set
        (rk_classify_pairs; the pair loop of repkiller.cpp:60-72)."""
        pairs = list(pairs)
        n, q = f.n, len(pairs)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((f.x_start, np.uint64), (f.y_start, np.uint64), (f.length, np.uint64),
                 (f.strand, np.uint8))]
        soa = FragsSoA(_ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]), n)
        gid = np.empty((q, n), np.uint32)
        rep = np.empty((q, n), np.uint8)
        order = np.empty((q, n), np.uint32)
        res = (Result * max(q, 1))()
        prm = (Params * max(q, 1))()
        for i, (lr, pr) in enumerate(pairs):
            res[i] = Result(_ptr(order[i]), _ptr(gid[i]), _ptr(rep[i]), 0, 0)
            prm[i] = Params(len_x_hdr, len_y_hdr, lr, pr)
        rc = load_library().rk_classify_pairs(self._h, ctypes.byref(soa), prm, q, res)
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        out = []
        for i in range(q):
            k = res[i].n_out
            out.append(ClassifyResult(gid[i, :k].copy(), rep[i, :k].copy(), order[i, :k].copy(),
                                      int(res[i].n_groups)))
        return out

    def classify_device(self, x, y, length, strand, gid, repval, out_order, len_x_hdr: int,
                        len_y_hdr: int, len_ratio: float = 0.3, pos_ratio: float = 0.3):
        """Device tensors (torch, on this context's GPU) in and out (rk_classify_device).

        Returns (n_out, n_groups).  Inputs: uint64/int64 x, y, length and uint8 strand;
        outputs: int32/uint32 gid and out_order, uint8 repval, all of length n, the
        first n_out entries filled in output order.
        """
        n = int(x.shape[0])
        soa = FragsSoA(x.data_ptr(), y.data_ptr(), length.data_ptr(), strand.data_ptr(), n)
        res = Result(out_order.data_ptr(), gid.data_ptr(), repval.data_ptr(), 0, 0)
        prm = Params(len_x_hdr, len_y_hdr, len_ratio, pos_ratio)
        rc = load_library().rk_classify_device(self._h, ctypes.byref(soa), ctypes.byref(prm),
                                               ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return int(res.n_out), int(res.n_groups)


    def classify_batch(self, sets, len_ratio: float = 0.3, pos_ratio: float = 0.3,
                       set_off=None) -> list:
        """Many fragment sets in one call (rk_classify_batch).  ``sets``: a list of
        ``(Frags, len_x_hdr, len_y_hdr)``; returns one :class:`ClassifyResult` per
        set, each what :meth:`classify` returns for that set alone.  ``set_off``
        (tests): the row offsets handed to the library instead of the sets' own."""
        sets = list(sets)
        ns = len(sets)
        cols = []
        for name, t in (("x_start", np.uint64), ("y_start", np.uint64), ("length", np.uint64),
                        ("strand", np.uint8)):
            parts = [np.ascontiguousarray(getattr(f, name), dtype=t) for f, _, _ in sets]
            cols.append(np.concatenate(parts) if parts else np.empty(0, t))
        off = np.zeros(ns + 1, np.uint64)
        if ns:
            off[1:] = np.cumsum([f.n for f, _, _ in sets], dtype=np.uint64)
        if set_off is not None:
            off = np.ascontiguousarray(set_off, np.uint64)
        n = int(cols[0].shape[0])
        lx = np.array([s[1] for s in sets], np.uint64)
        ly = np.array([s[2] for s in sets], np.uint64)
        gid, rep, order = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        n_out, n_groups = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
        soa = FragsSoA(_ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), n)
        prm = BatchParams(ns, off.ctypes.data, _ptr(lx), _ptr(ly), len_ratio, pos_ratio)
        res = BatchResult(_ptr(order), _ptr(gid), _ptr(rep), _ptr(n_out), _ptr(n_groups))
        rc = load_library().rk_classify_batch(self._h, ctypes.byref(soa), ctypes.byref(prm),
                                              ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        out = []
        for k in range(ns):
            a = int(off[k])
            b = a + int(n_out[k])
            out.append(ClassifyResult(gid[a:b].copy(), rep[a:b].copy(), order[a:b].copy(),
                                      int(n_groups[k])))
        return out

    def classify_device_batch(self, x, y, length, strand, gid, repval, out_order, set_off,
                              len_x_hdr, len_y_hdr, len_ratio: float = 0.3,
                              pos_ratio: float = 0.3):
        """Device tensors in and out (rk_classify_device_batch): the concatenated
        rows of all sets, ``set_off`` / ``len_x_hdr`` / ``len_y_hdr`` host sequences.
        Set k's result is entries [set_off[k], set_off[k] + n_out[k]) of the output
        tensors.  Returns (n_out, n_groups) as uint64 arrays."""
        off = np.ascontiguousarray(set_off, np.uint64)
        ns = off.shape[0] - 1
        lx = np.ascontiguousarray(len_x_hdr, np.uint64)
        ly = np.ascontiguousarray(len_y_hdr, np.uint64)
        n_out, n_groups = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
        soa = FragsSoA(x.data_ptr(), y.data_ptr(), length.data_ptr(), strand.data_ptr(),
                       int(x.shape[0]))
        prm = BatchParams(ns, off.ctypes.data, _ptr(lx), _ptr(ly), len_ratio, pos_ratio)
        res = BatchResult(out_order.data_ptr(), gid.data_ptr(), repval.data_ptr(), _ptr(n_out),
                          _ptr(n_groups))
        rc = load_library().rk_classify_device_batch(self._h, ctypes.byref(soa),
                                                     ctypes.byref(prm), ctypes.byref(res))
        if rc != RK_OK:
            raise RkError(rc, self.last_error())
        return n_out, n_groups

    def batch_stats(self) -> dict:
        """Counters of the last classify*_batch call (rk_get_batch_stats)."""
        s = BatchStats()
        _check(load_library().rk_get_batch_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in BatchStats._fields_}


def batch_layout(len_x, len_y):
    """The windows of a batch (rk_batch_layout): (base_x, base_y), nsets + 1
    entries each, in coordinates; set k's rows are translated by base[k]."""
    lx = np.ascontiguousarray(len_x, np.uint64)
    ly = np.ascontiguousarray(len_y, np.uint64)
    ns = lx.shape[0]
    bx, by = np.zeros(ns + 1, np.uint64), np.zeros(ns + 1, np.uint64)
    _check(load_library().rk_batch_layout(ns, _ptr(lx), _ptr(ly), bx.ctypes.data, by.ctypes.data),
           "rk_batch_layout")
    return bx, by


# ---------------------------------------------------- one set over many GPUs --

class Comm:
    """rk_comm: the collectives rk_classify_sharded runs on.

    ``Comm.rccl(rank, size, device)`` -- RCCL over xGMI (production); the unique
    id is broadcast with the default torch.distributed process group.
    ``Comm.torch_host(rank, size)`` -- host callbacks over the default
    torch.distributed group (gloo): device blocks are staged through host memory.
    """

    def __init__(self, handle, rank: int, size: int, keep=None):
        self._h = handle
        self.rank, self.size = rank, size
        self._keep = keep  # ctypes callbacks must outlive the comm

    @classmethod
    def rccl(cls, rank: int, size: int, device: int) -> "Comm":
        import torch
        import torch.distributed as dist
        lib = load_library()
        ident = (ctypes.c_uint8 * 128)()
        if rank == 0:
            _check(lib.rk_comm_rccl_id(ident), "rk_comm_rccl_id")
        t = torch.tensor(list(bytes(ident)), dtype=torch.uint8)
        if size > 1:
            dist.broadcast(t, src=0)
        ident = (ctypes.c_uint8 * 128)(*t.tolist())
        h = ctypes.c_void_p()
        # RCCL prints an init banner on stdout: keep stdout for the caller's output
        import sys
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            rc = lib.rk_comm_create_rccl(rank, size, device, ident, ctypes.byref(h))
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        _check(rc, "rk_comm_create_rccl")
        return cls(h, rank, size)

    @classmethod
    def torch_host(cls, rank: int, size: int, group=None) -> "Comm":
        import torch
        import torch.distributed as dist

        def allgather(_user, send, recv, nbytes):
            try:
                src = torch.empty(nbytes, dtype=torch.uint8)
                if nbytes:
                    ctypes.memmove(src.data_ptr(), send, nbytes)
                outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(size)]
                dist.all_gather(outs, src, group=group)
                for q, o in enumerate(outs):
                    if nbytes:
                        ctypes.memmove(recv + q * nbytes, o.data_ptr(), nbytes)
                return 0
            except Exception as e:  # noqa: BLE001 -- reported as a status code
                print(f"rk host allgather failed: {e!r}")
                return 1

        def alltoallv(_user, send, sb, recv, rb):
            try:
                sbl = [int(sb[q]) for q in range(size)]
                rbl = [int(rb[q]) for q in range(size)]
                src = torch.empty(sum(sbl), dtype=torch.uint8)
                if sum(sbl):
                    ctypes.memmove(src.data_ptr(), send, sum(sbl))
                dst = torch.empty(sum(rbl), dtype=torch.uint8)
                dist.all_to_all_single(dst, src, rbl, sbl, group=group)
                if sum(rbl):
                    ctypes.memmove(recv, dst.data_ptr(), sum(rbl))
                return 0
            except Exception as e:  # noqa: BLE001
                print(f"rk host alltoallv failed: {e!r}")
                return 1

        ag, a2a = ALLGATHER_FN(allgather), ALLTOALLV_FN(alltoallv)
        ops = CommHostOps(None, ag, a2a)
        h = ctypes.c_void_p()
        _check(load_library().rk_comm_create_host(rank, size, ctypes.byref(ops),
                                                  ctypes.byref(h)))
        return cls(h, rank, size, keep=(ag, a2a, ops))

    @classmethod
    def local(cls, size: int) -> list["Comm"]:
        """``size`` ranks inside this process (one thread per rank,
        rk_comm_create_local): device blocks move by device copies."""
        hs = (ctypes.c_void_p * size)()
        _check(load_library().rk_comm_create_local(size, hs), "rk_comm_create_local")
        return [cls(ctypes.c_void_p(hs[r]), r, size) for r in range(size)]

    def last_error(self) -> str:
        return load_library().rk_comm_last_error(self._h).decode()

    def close(self):
        if getattr(self, "_h", None):
            load_library().rk_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ShardOutput:
    """This rank's share of the global output: rows [out_offset, out_offset + n_out)."""
    result: ClassifyResult | None  # host copies (None when not copied)
    out_offset: int
    n_out: int
    n_out_total: int
    n_groups: int
    raw: ShardResult


def classify_sharded(ctx: "Context", comm: Comm, x, y, length, strand, len_x_hdr: int,
                     len_y_hdr: int, len_ratio: float = 0.3, pos_ratio: float = 0.3,
                     lead_in: int = -1, copy: bool = True) -> ShardOutput:
    """rk_classify_sharded on device tensors holding this rank's block of input rows."""
    lib = load_library()
    n = int(x.shape[0])
    soa = FragsSoA(x.data_ptr(), y.data_ptr(), length.data_ptr(), strand.data_ptr(), n)
    prm = Params(len_x_hdr, len_y_hdr, len_ratio, pos_ratio)
    res = ShardResult()
    rc = lib.rk_classify_sharded(ctx._h, comm._h, ctypes.byref(soa), ctypes.byref(prm),
                                 lead_in, ctypes.byref(res))
    if rc != RK_OK:
        raise RkError(rc, ctx.last_error())
    out = ShardOutput(None, int(res.out_offset), int(res.n_out), int(res.n_out_total),
                      int(res.n_groups), res)
    if copy:
        out.result = shard_copy(ctx, out)
    return out


def shard_copy(ctx: "Context", out: ShardOutput) -> ClassifyResult:
    """Host copies of this rank's output share (rk_shard_copy_result) of the last
    rk_classify_sharded call on ``ctx``; global file rows and group ids."""
    k = out.n_out
    order, gid, rep = np.empty(k, np.uint32), np.empty(k, np.uint32), np.empty(k, np.uint8)
    _check(load_library().rk_shard_copy_result(ctx._h, ctypes.byref(out.raw), _ptr(order),
                                               _ptr(gid), _ptr(rep)), ctx.last_error())
    return ClassifyResult(gid, rep, order, out.n_groups)


def classify_sharded_threads(f: Frags, ranks: int, len_x_hdr: int, len_y_hdr: int,
                             len_ratio: float = 0.3, pos_ratio: float = 0.3,
                             devices: list[int] | None = None) -> ClassifyResult:
    """ONE host fragment set over ``ranks`` ranks of this process (the CLI's
    ``--gpus P`` path, rk_cli.cpp): rank r holds the file-order rows
    [n r / P, n (r + 1) / P), runs rk_classify_sharded_host on its own context
    (device ``devices[r]``, default 0 for every rank) and copies its output
    share into the whole result at its offset."""
    import threading
    lib = load_library()
    n = f.n
    devices = devices or [0] * ranks
    comms = Comm.local(ranks)
    order, gid, rep = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8)
    status, errs, totals = [0] * ranks, [""] * ranks, [None] * ranks
    prm = Params(len_x_hdr, len_y_hdr, len_ratio, pos_ratio)

    def rank_body(r):
        h = ctypes.c_void_p()
        status[r] = lib.rk_create(ctypes.byref(h), devices[r])
        if status[r]:
            errs[r] = f"rk_create(device {devices[r]})"
            lib.rk_comm_abandon(comms[r]._h, status[r])
            return
        try:
            a, b = n * r // ranks, n * (r + 1) // ranks
            soa = FragsSoA(*[int(c.ctypes.data) + a * c.itemsize
                             for c in (f.x_start, f.y_start, f.length, f.strand)], b - a)
            res = ShardResult()
            status[r] = lib.rk_classify_sharded_host(h, comms[r]._h, ctypes.byref(soa),
                                                     ctypes.byref(prm), -1, ctypes.byref(res))
            if not status[r]:
                o = int(res.out_offset)
                status[r] = lib.rk_shard_copy_result(
                    h, ctypes.byref(res), order.ctypes.data + 4 * o, gid.ctypes.data + 4 * o,
                    rep.ctypes.data + o)
                totals[r] = (int(res.n_out_total), int(res.n_groups))
            if status[r]:
                errs[r] = lib.rk_last_error(h).decode()
        finally:
            lib.rk_destroy(h)

    threads = [threading.Thread(target=rank_body, args=(r,)) for r in range(ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in comms:
        c.close()
    for r in range(ranks):
        if status[r]:
            raise RkError(status[r], f"rank {r}: {errs[r]}")
    n_out, ng = totals[0]
    assert all(t == totals[0] for t in totals), totals
    return ClassifyResult(gid[:n_out], rep[:n_out], order[:n_out], ng)


def shard_stats(ctx: "Context") -> dict:
    s = ShardStats()
    _check(load_library().rk_get_shard_stats(ctx._h, ctypes.byref(s)))
    return {k: getattr(s, k) for k, _ in ShardStats._fields_}


def build(jobs: int = 8) -> None:
    """Compile librepkiller_amd.so + the CLI for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), f"-j{jobs}"], check=True)
