"""ctypes binding of libfruits_hip.so (the C ABI of include/fruits_hip.h).

This is the only door between the Python host code and the HIP kernels.  There
is NO CPU fallback: if the library is missing or no HIP device is present every
compute entry raises.  PyTorch is used for plumbing only - device memory
(``torch.empty(..., device="cuda")``), the current HIP stream and, in
``fruits_amd.parallel``, ``torch.distributed``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRUITS_HIP_LIB: an experiment build of the same sources (fruits_amd.build --variant=...)
LIB_PATH = os.path.join(_HERE, os.environ.get("FRUITS_HIP_LIB", "libfruits_hip.so"))

FR_W_NONE, FR_W_NONTOTAL, FR_W_TOTAL = 0, 1, 2
FR_SIEVE_NPI, FR_SIEVE_MPI, FR_SIEVE_END = 0, 1, 2
FR_SIEVE_MAX, FR_SIEVE_MIN, FR_SIEVE_XPI, FR_SIEVE_LPI, FR_SIEVE_CUR = 3, 4, 5, 6, 7
FR_SIEVE_PPV, FR_SIEVE_CPV = 16, 17   # numbers of their own: fr_sieve_implicit only
FR_SIEVE_SEGMENTS = 0x200   # OR-ed into PPV / CPV at fr_pipeline_create: bands q_j <= v < q_(j+1)
MAX_INC = 8   # the largest differencing order of a sieve's rows (csrc/kernels.h, kMaxInc)
FR_SIEVE_SERIES_CUTS = 0x100   # OR-ed into a kind: the sieve's cuts are slots of a per-series table
(FR_INFO_ROWS, FR_INFO_NODES, FR_INFO_LEVELS, FR_INFO_DIMS_USED, FR_INFO_MAX_DIM,
 FR_INFO_ALPHAS, FR_INFO_GROUPS, FR_INFO_SHARED, FR_INFO_STAGED_ROWS, FR_INFO_JIT_PROGRAMS,
 FR_INFO_AOT_PROGRAM, FR_INFO_STATIC_TAIL, FR_INFO_LAST_LAUNCH, FR_INFO_LAST_WHOLE,
 FR_INFO_GRAD_ROWS) = range(15)
# kernel families of FR_INFO_LAST_LAUNCH (csrc/plan.h, WalkFamily)
WALK_FAMILIES = (None, "interpreter", "static_aot", "static_jit", "lean", "packed", "fused",
                 "fused_packed", "fused_jit", "fused_pieces")
FR_E_ARG, FR_E_DIM, FR_E_HIP, FR_E_NOMEM, FR_E_LIMIT, FR_E_INDEX = -1, -2, -3, -4, -5, -6

EXPORTS = [
    "fr_last_error", "fr_version", "fr_device_count", "fr_malloc", "fr_free",
    "fr_memcpy_h2d", "fr_memcpy_d2h", "fr_stream_sync", "fr_plan_create",
    "fr_plan_destroy", "fr_plan_info", "fr_plan_dump", "fr_plan_records", "fr_plan_static_schedule", "fr_plan_pieces", "fr_plan_jit", "fr_plan_workspace_bytes",
    "fr_iss_run", "fr_iterated_sum_fast_host", "fr_increments",
    "fr_pathlen_lookup", "fr_sieve", "fr_sieve_implicit", "fr_pre_transform", "fr_standardize",
    "fr_pipeline_create", "fr_pipeline_destroy", "fr_pipeline_info",
    "fr_pipeline_workspace_bytes", "fr_pipeline_run", "fr_pipeline_set_quantiles",
    "fr_select_ranks", "fr_select_ranks_begin", "fr_select_ranks_end", "fr_coswiss_combine", "fr_plan_create_coswiss", "fr_nan_to_num",
    "fr_plan_prepare", "fr_pipeline_prepare", "fr_pipeline_compile_plan", "fr_pipeline_prepare_cached", "fr_pipeline_bundle", "fr_plan_fits", "fr_release_scratch",
    "fr_pipeline_set_preparation", "fr_pipeline_set_series_cuts", "fr_pipeline_set_argmax", "fr_arctic_argmax", "fr_coswiss_set_dropout",
    "fr_coswiss_set_input_stride", "fr_coswiss_ffn",
    "fr_prep_fir", "fr_prep_project", "fr_prep_normalize", "fr_prep_leadlag",
    "fr_prep_mask", "fr_prep_pointwise",
    "fr_letter_rows", "fr_rows_unshift",
    "fr_pipeline_set_lengths", "fr_sieve_implicit_lengths", "fr_standardize_lengths",
    "fr_iss_backward", "fr_iss_backward_max", "fr_iss_backward_weighted",
    "fr_sieve_pick", "fr_iss_backward_picked", "fr_plan_set_grad_lengths",
    "fr_plan_set_grad_pathlen", "fr_sieve_heads", "fr_sieve_heads_adjoint",
]
FR_ROW_DIM, FR_ROW_ABS, FR_ROW_EXT, FR_ROW_ONE = range(4)
FR_PW_MUL, FR_PW_ADD, FR_PW_ROTATE, FR_PW_POW, FR_PW_SHIFT, FR_PW_CLIP = range(6)
FR_PW_FLAG_SIN = FR_PW_FLAG_LOWER = 1

_lib = None
_torch = None


class NativeError(RuntimeError):
    pass


def torch():
    """torch is imported before the library so both share ONE HIP runtime
    (torch bundles libamdhip64.so.7; the loader resolves our DT_NEEDED entry to
    the copy that is already mapped)."""
    global _torch
    if _torch is None:
        import torch as _t
        _torch = _t
    return _torch


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "fruits_amd/libfruits_hip.so is missing - build it with "
            "`python -m fruits_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    torch()
    L = C.CDLL(LIB_PATH)
    L.fr_last_error.restype = C.c_char_p
    L.fr_plan_create.restype = C.c_void_p
    L.fr_plan_create_coswiss.restype = C.c_void_p
    L.fr_plan_destroy.restype = None
    L.fr_plan_destroy.argtypes = [C.c_void_p]
    L.fr_plan_info.restype = C.c_int64
    L.fr_plan_info.argtypes = [C.c_void_p, C.c_int32]
    L.fr_plan_dump.restype = C.c_int32
    L.fr_plan_records.restype = C.c_int32
    L.fr_plan_jit.restype = C.c_int32
    L.fr_plan_jit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    L.fr_plan_static_schedule.restype = C.c_int32
    L.fr_plan_pieces.restype = C.c_int64
    L.fr_plan_static_schedule.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.fr_plan_records.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.fr_plan_workspace_bytes.restype = C.c_int64
    L.fr_plan_workspace_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    L.fr_pipeline_create.restype = C.c_void_p
    L.fr_pipeline_destroy.restype = None
    L.fr_pipeline_destroy.argtypes = [C.c_void_p]
    L.fr_pipeline_info.restype = C.c_int64
    L.fr_pipeline_info.argtypes = [C.c_void_p, C.c_int32]
    L.fr_pipeline_workspace_bytes.restype = C.c_int64
    L.fr_pipeline_workspace_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.fr_plan_fits.restype = C.c_int32
    L.fr_plan_fits.argtypes = [C.c_void_p, C.c_int64]
    L.fr_plan_prepare.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32]
    L.fr_pipeline_prepare.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    L.fr_pipeline_compile_plan.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    L.fr_pipeline_prepare_cached.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    L.fr_pipeline_set_series_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    L.fr_pipeline_set_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.fr_plan_set_grad_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.fr_plan_set_grad_pathlen.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                           C.c_void_p]
    L.fr_pipeline_set_argmax.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fr_select_ranks_begin.restype = C.c_void_p
    L.fr_select_ranks_end.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.fr_pipeline_set_preparation.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_double]
    _lib = L
    return L


def last_error() -> str:
    return lib().fr_last_error().decode()


def check(rc: int, what: str = "") -> None:
    if rc >= 0:
        return
    msg = last_error()
    if rc in (FR_E_DIM, FR_E_INDEX):
        raise IndexError(msg)
    if rc in (FR_E_ARG, FR_E_LIMIT):
        raise ValueError(msg)
    if rc == FR_E_NOMEM:
        raise MemoryError(msg)
    raise NativeError(f"{what}: {msg}" if what else msg)


def device_count() -> int:
    return int(lib().fr_device_count())


def require_device():
    """Returns the torch device to run on; raises when there is no GPU."""
    t = torch()
    if not t.cuda.is_available() or device_count() == 0:
        raise NativeError(
            "fruits_amd needs a HIP device (MI355X / gfx950); none is visible and "
            "there is deliberately no CPU fallback")
    return t.device("cuda", t.cuda.current_device())


_PREPARE_POOL = None


def _prepare_pool():
    """One helper thread for compilations nobody should wait for."""
    global _PREPARE_POOL
    if _PREPARE_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _PREPARE_POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="fruits-prepare")
    return _PREPARE_POOL


def stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch().cuda.current_stream().cuda_stream)


def dptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def to_device(arr, dtype=None):
    """numpy (or torch) -> contiguous device tensor (float64 unless given)."""
    t = torch()
    dev = require_device()
    if isinstance(arr, t.Tensor):
        x = arr.to(device=dev)
        if dtype is not None:
            x = x.to(dtype)
        return x.contiguous()
    a = np.ascontiguousarray(arr, dtype=dtype or np.float64)
    # The copy from pageable memory is synchronous with the stream it is queued on - on the
    # caller's stream it would wait for everything queued there (Fruit.fit: the selection of the
    # slice before).  It goes through a stream of its own; the caller's stream waits for it on
    # the device.
    cur = t.cuda.current_stream(dev)
    if t.cuda.is_current_stream_capturing():
        return t.from_numpy(a).to(dev)
    up = _upload_stream(dev)
    with t.cuda.stream(up):
        x = t.from_numpy(a).to(dev)
    cur.wait_stream(up)
    x.record_stream(cur)
    return x


_upload_streams: dict = {}


def _upload_stream(dev):
    key = str(dev)
    st = _upload_streams.get(key)
    if st is None:
        st = _upload_streams[key] = torch().cuda.Stream(device=dev)
    return st


# Downloads of at least this many bytes land in page-locked memory from torch's caching host
# allocator (the array keeps its block; a freed one is reused): 72 MB of features come down at the
# link's rate instead of through the runtime's bounce buffers.  FRUITS_AMD_PINNED_MB = 0: never.
_PINNED_FROM = 1 << 20


def to_host(x) -> np.ndarray:
    x = x.detach()
    limit = int(os.environ.get("FRUITS_AMD_PINNED_MB", "4096")) << 20
    nbytes = x.numel() * x.element_size()
    if x.is_cuda and _PINNED_FROM <= nbytes <= limit:
        t = torch()
        try:
            h = t.empty(x.shape, dtype=x.dtype, pin_memory=True)
        except RuntimeError:       # (no page-locked memory left: the pageable path)
            return x.cpu().numpy()
        h.copy_(x.contiguous(), non_blocking=True)
        t.cuda.current_stream(x.device).synchronize()
        return h.numpy()
    return x.cpu().numpy()


# ----------------------------------------------------------------------- plan
class Plan:
    """Compiled device program of a word list (fr_plan_create)."""

    def __init__(self, words: Sequence[np.ndarray], depths: Sequence[int],
                 alphas: Optional[Sequence[np.ndarray]] = None, weighting: int = FR_W_NONE,
                 share_prefixes: bool = True, arctic: bool = False, bayesian: bool = False,
                 letter_sum: bool = False):
        L = lib()
        self._h = None
        mats = [np.ascontiguousarray(w, dtype=np.int32) for w in words]
        for m in mats:
            if m.ndim != 2:
                raise ValueError("word tables must be (L, Dw) int32")
        W = len(mats)
        exps = (np.concatenate([m.ravel() for m in mats]) if W else
                np.zeros(0, np.int32)).astype(np.int32)
        Ls = np.array([m.shape[0] for m in mats], dtype=np.int32)
        Dws = np.array([m.shape[1] for m in mats], dtype=np.int32)
        dep = np.asarray(depths, dtype=np.int32)
        if dep.shape != (W,):
            raise ValueError("one depth per word")
        al = None
        if weighting != FR_W_NONE:
            if alphas is None:
                raise ValueError("weighted plan needs alphas")
            al = np.concatenate([np.asarray(a, dtype=np.float32).ravel()
                                 for a in alphas]).astype(np.float32)
            if al.size != int(Ls.sum()):
                raise ValueError("Size of alpha array does not match word length")
        ip = C.POINTER(C.c_int32)
        h = L.fr_plan_create(
            C.c_int32(W), exps.ctypes.data_as(ip), Ls.ctypes.data_as(ip),
            Dws.ctypes.data_as(ip),
            al.ctypes.data_as(C.POINTER(C.c_float)) if al is not None else None,
            dep.ctypes.data_as(ip), C.c_int32(weighting),
            C.c_int32((1 if share_prefixes else 0) | (2 if arctic else 0)
                      | (4 if bayesian else 0) | (8 if letter_sum else 0)))
        if not h:
            raise ValueError(last_error())
        self._h = C.c_void_p(h)
        self.weighting = weighting
        self.n_words = W

    def __del__(self):
        try:
            if self._h is not None and _lib is not None:
                _lib.fr_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def info(self, what: int) -> int:
        return int(lib().fr_plan_info(self._h, C.c_int32(what)))

    @property
    def rows(self) -> int:
        return self.info(FR_INFO_ROWS)

    @property
    def nodes(self) -> int:
        return self.info(FR_INFO_NODES)

    @property
    def max_dim(self) -> int:
        return self.info(FR_INFO_MAX_DIM)

    @property
    def staged_rows(self) -> int:
        return self.info(FR_INFO_STAGED_ROWS)

    def fits(self, T: int) -> bool:
        """Whether a workgroup can stage the plan's rows (input dimensions + exp
        tables) of one time chunk in LDS (fr_plan_fits: the library's own rule)."""
        rc = int(lib().fr_plan_fits(self._h, int(T)))
        check(rc, "fr_plan_fits")
        return rc == 1

    def prepare(self, N: int, T: int, groups: int = 0) -> None:
        """One-time upload of the device tables for (N, T) batches (fr_plan_prepare):
        afterwards ``run`` only enqueues work and may be captured into a hipGraph."""
        check(lib().fr_plan_prepare(self._h, int(N), int(T), int(groups)), "fr_plan_prepare")

    @property
    def dims_used(self) -> int:
        return self.info(FR_INFO_DIMS_USED)

    def dump(self) -> np.ndarray:
        n = self.nodes
        buf = np.zeros((max(n, 1), 8), dtype=np.int32)
        got = lib().fr_plan_dump(self._h, buf.ctypes.data_as(C.POINTER(C.c_int32)),
                                 C.c_int32(buf.size))
        return buf[:got]

    def records(self, groups: int = 1) -> np.ndarray:
        """The device program for ``groups`` groups per series: (records, 16) int32."""
        n = int(lib().fr_plan_records(self._h, groups, None, 0))
        buf = np.zeros((max(n, 1), 16), dtype=np.int32)
        check(lib().fr_plan_records(self._h, groups, buf.ctypes.data, buf.size))
        return buf[:n]

    def jit(self, groups: int = 1, compile_only: bool = False):
        """fr_plan_jit: (count or code size, message)."""
        buf = C.create_string_buffer(8192)
        rc = lib().fr_plan_jit(self._h, int(groups), 1 if compile_only else 0, buf, len(buf))
        check(rc, "fr_plan_jit")
        return int(rc), buf.value.decode(errors="replace")

    def static_program_index(self, groups: int = 1) -> int:
        """1 + index of the pre-compiled static program this plan's records equal (0: none)."""
        return int(lib().fr_plan_info(self._h, FR_INFO_AOT_PROGRAM))

    def static_tail_series(self) -> int:
        """Series that the most recent ``run`` launched as the finer units of the static program's
        tail program, behind the whole-series units (0: no mixed launch)."""
        return int(lib().fr_plan_info(self._h, FR_INFO_STATIC_TAIL))

    def last_launch(self) -> dict:
        """How the most recent ``run`` of this plan - or of a pipeline over it - launched its walk
        (fr_plan_info, FR_INFO_LAST_LAUNCH): ``family`` (one of WALK_FAMILIES; None: no walk
        yet), ``G`` groups per series, ``persistent``, ``xcd_map``, ``nt_input``, ``wt``,
        ``lds_pad`` (one was asked for), ``carry_in_lds``, ``tail_series`` and ``n_whole`` of a
        mixed static launch, and the resident rounds the choice was made from: ``resident`` (the
        groups) and ``mixed_resident`` (the tail), 0 where they were not asked."""
        w = int(lib().fr_plan_info(self._h, FR_INFO_LAST_LAUNCH))
        return {"family": WALK_FAMILIES[w & 15], "G": w >> 4 & 255, "persistent": w >> 12 & 15,
                "xcd_map": w >> 16 & 1, "nt_input": w >> 17 & 1, "wt": w >> 18 & 1,
                "lds_pad": w >> 19 & 1, "carry_in_lds": w >> 20 & 1,
                "resident": w >> 21 & 0xfffff, "mixed_resident": w >> 41 & 0xfffff,
                "tail_series": self.static_tail_series(),
                "n_whole": int(lib().fr_plan_info(self._h, FR_INFO_LAST_WHOLE))}

    def jit_loaded(self) -> int:
        """Number of run-time compiled static programs this plan holds on the device."""
        return int(lib().fr_plan_info(self._h, FR_INFO_JIT_PROGRAMS))

    def pieces(self, max_piece: int = 0):
        """The plan in pieces (fr_plan_pieces; csrc/plan.h, PiecedProgram) as a dict, or None when
        the plan has no such cover: ``types`` - per piece type its body / chain records
        ((records, 16) int32), items ((items, 4): chain byte offset, walk position of the body's
        first row, nodes of the unit in front), ``unit_begin``, ``unit_row0`` - and
        ``row_of_walk``, the output row at every walk position."""
        L = lib()
        n = int(L.fr_plan_pieces(self._h, C.c_int32(max_piece), None, C.c_int64(0)))
        if n <= 0:
            return None
        buf = np.zeros(n, dtype=np.int32)
        L.fr_plan_pieces(self._h, C.c_int32(max_piece), buf.ctypes.data_as(C.POINTER(C.c_int32)),
                         C.c_int64(n))
        n_types, K, chain_nodes, nodes = (int(v) for v in buf[:4])
        at, types = 4, []
        for _ in range(n_types):
            (body_nodes, body_rows, levels, units, n_items, max_unit_nodes, n_recs,
             max_unit_rows) = (int(v) for v in buf[at:at + 8])
            at += 8
            recs = buf[at:at + 16 * n_recs].reshape(n_recs, 16).copy()
            at += 16 * n_recs
            items = buf[at:at + 4 * n_items].reshape(n_items, 4).copy()
            at += 4 * n_items
            unit_begin = buf[at:at + units + 1].copy()
            at += units + 1
            unit_row0 = buf[at:at + units].copy()
            at += units
            types.append(dict(body_nodes=body_nodes, body_rows=body_rows, levels=levels, units=units,
                              max_unit_nodes=max_unit_nodes, max_unit_rows=max_unit_rows, recs=recs,
                              items=items, unit_begin=unit_begin, unit_row0=unit_row0))
        return dict(types=types, K=K, chain_nodes=chain_nodes, nodes=nodes,
                    row_of_walk=buf[at:at + K].copy())

    def static_schedule(self, groups: int = 1):
        """(header dict, (entries, 16) int32) of the plan's static schedule, or None."""
        n = int(lib().fr_plan_static_schedule(self._h, groups, None, 0))
        if n <= 0:
            return None
        buf = np.zeros(32 + n * 16, dtype=np.int32)
        check(lib().fr_plan_static_schedule(self._h, groups, buf.ctypes.data, buf.size))
        rows, G = int(buf[1]), int(buf[3])
        head = {"entries": n, "rows": rows, "frames": int(buf[2]), "groups": G,
                "row_src": [int(v) for v in buf[4:4 + rows]],
                "group_begin": [int(v) for v in buf[8:8 + G]],
                "group_rows": [int(v) for v in buf[16:16 + G]]}
        return head, buf[32:].reshape(n, 16)

    def workspace_bytes(self, N: int, T: int, lookup_rows: int) -> int:
        return int(lib().fr_plan_workspace_bytes(self._h, N, T, lookup_rows))

    def run(self, Xd, lookup_d=None, out=None, layout: str = "KNT", groups: int = 0,
            work=None, strides=None):
        """Launches the trie walk on the current stream.

        Xd (N,D,T) f64 cuda; lookup_d (1|N, T) f64 cuda or None.
        layout "KNT" -> (K,N,T) (fruits/iss/iss.py:46), "NKT" -> (N,K,T)
        (fruits/iss/semiring.py:177)."""
        t = torch()
        if Xd.dtype != t.float64 or Xd.dim() != 3 or not Xd.is_contiguous():
            raise TypeError("X must be a contiguous float64 (N, D, T) device tensor")
        N, D, T = Xd.shape
        K = self.rows
        if out is None:
            shape = (K, N, T) if layout == "KNT" else (N, K, T)
            out = t.empty(shape, dtype=t.float64, device=Xd.device)
        if strides is not None:
            sk, sn = strides   # caller-laid-out buffer (element strides of k and n)
        elif layout == "KNT":
            sk, sn = N * T, T
        else:
            sk, sn = T, K * T
        rows = 0
        if self.weighting != FR_W_NONE:
            if lookup_d is None:
                raise ValueError("weighted plan needs a lookup")
            rows = int(lookup_d.shape[0])
            if lookup_d.shape[-1] != T or not lookup_d.is_contiguous():
                raise ValueError("lookup must be contiguous (1|N, T)")
        wb = self.workspace_bytes(N, T, rows)
        if wb > 0 and (work is None or work.numel() < wb):
            work = t.empty(wb, dtype=t.uint8, device=Xd.device)
        rc = lib().fr_iss_run(
            self._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
            dptr(lookup_d if self.weighting != FR_W_NONE else None), C.c_int64(rows),
            dptr(out), C.c_int64(sk), C.c_int64(sn), dptr(work),
            C.c_int64(work.numel() if work is not None else 0), C.c_int32(groups),
            stream_ptr())
        check(rc, "fr_iss_run")
        return out


class CosPlan(Plan):
    """Device program of a cosine weighted ISS (fr_plan_create_coswiss): rows
    word-major, ``len(freqs)`` rows per word."""

    MAX_EXPONENT = 8
    MAX_LETTERS = 16

    def __init__(self, words: Sequence[np.ndarray], freqs, exponent: int, total: bool):
        L = lib()
        self._h = None
        mats = [np.ascontiguousarray(w, dtype=np.int32) for w in words]
        W = len(mats)
        exps = (np.concatenate([m.ravel() for m in mats]) if W else
                np.zeros(0, np.int32)).astype(np.int32)
        Ls = np.array([m.shape[0] for m in mats], dtype=np.int32)
        Dws = np.array([m.shape[1] for m in mats], dtype=np.int32)
        fq = np.asarray(freqs, dtype=np.float32).ravel()
        ip = C.POINTER(C.c_int32)
        h = L.fr_plan_create_coswiss(
            C.c_int32(W), exps.ctypes.data_as(ip), Ls.ctypes.data_as(ip), Dws.ctypes.data_as(ip),
            C.c_int32(fq.size), fq.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(exponent),
            C.c_int32(1 if total else 0))
        if not h:
            raise ValueError(last_error())
        self._h = C.c_void_p(h)
        self.weighting = FR_W_NONE
        self.n_words = W


def coswiss_set_dropout(plan: "CosPlan", indices, T: int) -> None:
    """fr_coswiss_set_dropout: ``indices`` (W, F, Lmax, rate) int32 as drawn by CosWISS._fit;
    ``None`` switches the mask off."""
    if indices is None:
        check(lib().fr_coswiss_set_dropout(plan._h, None, C.c_int32(0), C.c_int32(0),
                                           C.c_int64(max(int(T), 1))), "fr_coswiss_set_dropout")
        return
    idx = np.ascontiguousarray(indices, dtype=np.int32)
    check(lib().fr_coswiss_set_dropout(plan._h, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.c_int32(idx.shape[2]), C.c_int32(idx.shape[3]),
                                       C.c_int64(int(T))), "fr_coswiss_set_dropout")


def coswiss_ffn(Xd, A, b, Cm, out):
    """fr_coswiss_ffn: out (N, D, T) = C relu(A x + b) per time step; A (hidden, D), b
    (hidden), Cm (D, hidden) host arrays."""
    N, D, T = (int(v) for v in Xd.shape)
    Ad = to_device(np.ascontiguousarray(A, dtype=np.float64))
    bd = to_device(np.ascontiguousarray(b, dtype=np.float64))
    Cd = to_device(np.ascontiguousarray(Cm, dtype=np.float64))
    check(lib().fr_coswiss_ffn(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(Ad),
                               dptr(bd), dptr(Cd), C.c_int32(int(A.shape[0])), dptr(out),
                               stream_ptr()), "fr_coswiss_ffn")
    return out


class Pipeline:
    """ISS + sieves fused into one launch (fr_pipeline_*): the (K, N, T) tensor is
    never written.  ``sieves`` is a list of ``(kind, inc, cut_row, Q1)`` with
    ``cut_row`` the transformed int64 cuts (sorted, leading 0) for length ``T``.
    Raises ValueError when a sieve is outside the fused set."""

    def __init__(self, plan: Plan, sieves, T: int, argmax_lengths=None):
        """``argmax_lengths``: the plan holds every prefix of words of these lengths and the
        pipeline's rows are those of Arctic(argmax=True) (fr_pipeline_set_argmax)."""
        L = lib()
        self._h = None
        self.plan = plan
        self.T = int(T)
        n = len(sieves)
        kinds = np.array([s[0] for s in sieves], dtype=np.int32)
        incs = np.array([s[1] for s in sieves], dtype=np.int32)
        C1 = np.array([len(s[2]) for s in sieves], dtype=np.int32)
        Q1 = np.array([s[3] for s in sieves], dtype=np.int32)
        cuts = np.concatenate([np.asarray(s[2], dtype=np.int64) for s in sieves]).astype(np.int64)
        ip = C.POINTER(C.c_int32)
        h = L.fr_pipeline_create(plan._h, C.c_int32(n), kinds.ctypes.data_as(ip),
                                 incs.ctypes.data_as(ip), C1.ctypes.data_as(ip),
                                 Q1.ctypes.data_as(ip),
                                 cuts.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(self.T))
        if not h:
            msg = last_error()
            raise (IndexError if "out of bounds" in msg else ValueError)(msg)
        self._h = C.c_void_p(h)
        self.raw_dims = 0    # > 0: fused preparation, run() takes the raw input
        self._preparation = None     # the arguments of the last set_preparation (ensure_preparation)
        self.rows = plan.rows
        if argmax_lengths is not None:
            lens = np.ascontiguousarray(argmax_lengths, dtype=np.int32)
            rc = L.fr_pipeline_set_argmax(self._h, C.c_int32(len(lens)), lens.ctypes.data_as(ip))
            if rc != 0:
                msg = last_error()
                L.fr_pipeline_destroy(self._h)
                self._h = None
                raise ValueError(msg)
            self.rows = int(sum(int(n) + int(n) * (int(n) + 1) // 2 for n in lens))
        self.per_sum = int(L.fr_pipeline_info(self._h, 0))
        self.q_stride = int(L.fr_pipeline_info(self._h, 1))
        self.n_features = int(L.fr_pipeline_info(self._h, 2))

    def __del__(self):
        try:
            if self._h is not None and _lib is not None:
                _lib.fr_pipeline_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_quantiles(self, quant: np.ndarray) -> None:
        """``quant`` (K, q_stride) host array: the sorted thresholds of every
        iterated sum's band sieves, in sieve order."""
        q = np.ascontiguousarray(quant, dtype=np.float64)
        if q.shape != (self.rows, self.q_stride):
            raise ValueError("quantile table must be (K, q_stride)")
        check(lib().fr_pipeline_set_quantiles(self._h, q.ctypes.data_as(C.POINTER(C.c_double))),
              "fr_pipeline_set_quantiles")

    def set_series_cuts(self, table) -> None:
        """``table`` (N, slots) int32 device tensor: the per-series boundaries of the sieves
        created with FR_SIEVE_SERIES_CUTS, for the following runs on exactly N series."""
        t = torch()
        if table.dtype != t.int32 or table.dim() != 2 or not table.is_contiguous():
            raise TypeError("the cut table must be a contiguous int32 (N, slots) device tensor")
        check(lib().fr_pipeline_set_series_cuts(self._h, C.c_void_p(table.data_ptr()),
                                                C.c_int64(table.shape[0]), C.c_int32(table.shape[1])),
              "fr_pipeline_set_series_cuts")
        self._series_cuts = table    # (keeps the tensor alive while the pipeline points at it)

    def set_lengths(self, lengths) -> None:
        """``lengths`` (N,) int32 device tensor: the per-series lengths of the following runs on
        exactly N series (fr_pipeline_set_lengths); None: every series is T long again."""
        t = torch()
        if lengths is None:
            check(lib().fr_pipeline_set_lengths(self._h, None, 0), "fr_pipeline_set_lengths")
        else:
            if lengths.dtype != t.int32 or lengths.dim() != 1 or not lengths.is_contiguous():
                raise TypeError("the lengths must be a contiguous int32 (N,) device tensor")
            check(lib().fr_pipeline_set_lengths(self._h, C.c_void_p(lengths.data_ptr()),
                                                C.c_int64(lengths.shape[0])),
                  "fr_pipeline_set_lengths")
        self._lengths = lengths      # (keeps the tensor alive while the pipeline points at it)

    def set_preparation(self, D: int, inc_lag: int = 0, as_new: bool = False,
                        standardize: int = 0, std_eps: float = 1e-5) -> bool:
        """fr_pipeline_set_preparation: ``run`` then takes the RAW (N, D, T) input and forms
        INC / NEW(INC) / STD rows while staging.  False when this plan's kernel has no fused
        staging (the caller keeps materialising the prepared input)."""
        asked = (int(D), int(inc_lag), bool(as_new), int(standardize), float(std_eps))
        self._preparation = None     # (a call that raises leaves nothing remembered)
        rc = lib().fr_pipeline_set_preparation(self._h, asked[0], asked[1], 1 if as_new else 0,
                                               asked[3], asked[4])
        if rc == FR_E_LIMIT:
            self.raw_dims = 0
            self._preparation = asked     # (remembered as "nothing fused": asking again changes nothing)
            return False
        check(rc, "fr_pipeline_set_preparation")
        self._preparation = asked
        self.raw_dims = int(D) if (inc_lag or standardize) else 0
        return self.raw_dims > 0

    def ensure_preparation(self, D: int, inc_lag: int = 0, as_new: bool = False,
                           standardize: int = 0, std_eps: float = 1e-5) -> bool:
        """``set_preparation`` unless the pipeline is configured for these arguments already (the
        library call frees and uploads the preparation table and waits for the device: not per
        call for a table that has not changed).  The pipeline remembers the arguments of the last
        ``set_preparation`` it accepted or refused with FR_E_LIMIT.  Without a chain
        (``inc_lag == 0 and standardize == 0``) nothing is done while nothing is fused, whatever
        ``D``.  Returns ``raw_dims > 0``."""
        if inc_lag or standardize:
            stale = self._preparation != (D, inc_lag, as_new, standardize, std_eps)
        else:
            stale = self.raw_dims > 0
        if stale:
            self.set_preparation(D, inc_lag, as_new, standardize, std_eps)
        return self.raw_dims > 0

    # plans up to this size are compiled as straight-line code by a prepare nobody waits for, and
    # the node shapes of plans beyond 128 nodes (a few seconds of compiler either way; the
    # interpreter joins its helper threads at exit) - between, ten seconds and more
    QUICK_PLAN_NODES = 48

    def prepare(self, N: int, groups: int = 0, plan_too: bool = True) -> None:
        """fr_pipeline_prepare: uploads the plan's tables for batches of N series so
        that ``run`` only enqueues work (hipGraph capture), and compiles the pipeline's own
        kernel - the fused walk with its sieves as compile-time constants (hipRTC, cached on disk;
        FRUITS_HIP_JIT=0: not); ``plan_too``: also the variant that knows the plan
        (fr_pipeline_compile_plan: a plan of at most 128 nodes as straight-line code, of a larger
        one the node shapes - seconds to tens of seconds the first time on a machine)."""
        check(lib().fr_pipeline_prepare(self._h, int(N), int(groups)), "fr_pipeline_prepare")
        if plan_too:
            check(lib().fr_pipeline_compile_plan(self._h, int(N), int(groups)), "fr_pipeline_compile_plan")

    def prepare_cached(self, N: int, groups: int = 0) -> int:
        """fr_pipeline_prepare_cached: the uploads, and the pipeline's own kernels if an earlier
        process on this machine compiled them (the disk cache: milliseconds; nothing is
        compiled).  Returns the number of kernels the pipeline now holds."""
        check(lib().fr_pipeline_prepare_cached(self._h, int(N), int(groups)), "fr_pipeline_prepare_cached")
        return self.jit_loaded()

    def prepare_in_background(self, N: int, groups: int = 0):
        """``prepare`` on a helper thread: the caller goes on with the generic kernel and a later
        ``run`` picks the pipeline's own kernel up once it is compiled and loaded (the library
        guards the pipeline's compiled kernels with a lock).  Returns the future; a failure to
        compile is not an error - the generic kernel stays - anything else is re-raised by
        ``future.result()``."""
        device = torch().cuda.current_device()

        def work():
            torch().cuda.set_device(device)      # (the current device is per thread)
            # (self: the pipeline outlives the compilation)
            nodes = self.plan.nodes
            self.prepare(N, groups, plan_too=nodes <= self.QUICK_PLAN_NODES or nodes > 128)
        self._pending = _prepare_pool().submit(work)

        def report(fut):     # (nobody may ever call result(): a failure is said once, not swallowed)
            err = fut.exception()
            if err is not None:
                import warnings
                warnings.warn(f"fruits_amd: compiling a pipeline's own kernels failed ({err}); "
                              "the generic kernel keeps running it", RuntimeWarning)
        self._pending.add_done_callback(report)
        return self._pending

    def jit_loaded(self, static_only: bool = False) -> int:
        """Run-time compiled kernels this pipeline holds (``static_only``: those with the plan
        as straight-line code)."""
        return int(lib().fr_pipeline_info(self._h, 4 if static_only else 3))

    def bundle(self, quant: np.ndarray, out_dir: str, groups: int = 1) -> int:
        """fr_pipeline_bundle: compiles this pipeline's kernels (the sieves as immediates; the
        plan as straight-line code or in pieces) into ``out_dir`` without a device; ``quant``
        (K, q_stride) carries the infinities of the thresholds (finite values are placeholders)."""
        q = np.ascontiguousarray(quant, dtype=np.float64)
        if q.shape != (self.plan.rows, self.q_stride):
            raise ValueError("quantile table must be (K, q_stride)")
        buf = C.create_string_buffer(4096)
        L = lib()
        L.fr_pipeline_bundle.restype = C.c_int32
        rc = L.fr_pipeline_bundle(self._h, q.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(groups),
                                  os.fsencode(out_dir), buf, C.c_int64(len(buf)))
        if rc < 0:
            raise NativeError(f"fr_pipeline_bundle: {last_error()}")
        return int(rc)

    def fully_compiled(self) -> bool:
        """Whether the pipeline already holds the kernels a ``prepare`` would give it: the plan's
        own (in pieces, or as straight-line code) - nothing left for a compiler to do."""
        return self.pieces_loaded() > 0 or self.jit_loaded(static_only=True) > 0

    def pieces_loaded(self) -> int:
        """Kernels of piece types this pipeline holds (a large plan in pieces)."""
        return int(lib().fr_pipeline_info(self._h, 5))

    def last_launch(self) -> dict:
        """``Plan.last_launch`` of the pipeline's plan: ``run`` launches its walk."""
        return self.plan.last_launch()

    def run(self, Xd, lookup_d, feats=None, groups: int = 0, work=None):
        t = torch()
        if Xd.dtype != t.float64 or Xd.dim() != 3 or not Xd.is_contiguous():
            raise TypeError("X must be a contiguous float64 (N, D, T) device tensor")
        N, D, T = Xd.shape
        if feats is None:
            feats = t.empty((N, self.n_features), dtype=t.float64, device=Xd.device)
        rows = 0
        if self.plan.weighting != FR_W_NONE:
            if lookup_d is None:
                raise ValueError("weighted plan needs a lookup")
            rows = int(lookup_d.shape[0])
        wb = int(lib().fr_pipeline_workspace_bytes(self._h, N, rows))
        if wb > 0 and (work is None or work.numel() < wb):
            work = t.empty(wb, dtype=t.uint8, device=Xd.device)
        rc = lib().fr_pipeline_run(
            self._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
            dptr(lookup_d if self.plan.weighting != FR_W_NONE else None), C.c_int64(rows),
            dptr(feats), C.c_int64(feats.stride(0)), dptr(work),
            C.c_int64(work.numel() if work is not None else 0), C.c_int32(groups), stream_ptr())
        check(rc, "fr_pipeline_run")
        return feats


# ----------------------------------------------------------------------- kernels
def iterated_sum_fast_host(Z, word, alpha, lookup, extended, total_weighting, arctic=False,
                           bayesian=False):
    """fr_iterated_sum_fast_host: host arrays in / out (the literal drop-in of
    Semiring.iterated_sum_fast, fruits/iss/semiring.py:43-52)."""
    require_device()
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    word = np.ascontiguousarray(word, dtype=np.int32)
    N, D, T = Z.shape
    Lw, Dw = word.shape
    out = np.zeros((N, int(extended), T))
    al = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.float32)
    lk = None if lookup is None else np.ascontiguousarray(lookup, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    rc = lib().fr_iterated_sum_fast_host(
        Z.ctypes.data_as(dp), C.c_int64(N), C.c_int64(D), C.c_int64(T),
        word.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(Lw), C.c_int32(Dw),
        al.ctypes.data_as(C.POINTER(C.c_float)) if al is not None else None,
        lk.ctypes.data_as(dp) if lk is not None else None, C.c_int64(int(extended)),
        C.c_int32((1 if total_weighting else 0) | (2 if arctic else 0) | (4 if bayesian else 0)),
        out.ctypes.data_as(dp))
    check(rc, "fr_iterated_sum_fast_host")
    return out


def increments(Xd, shift: int, head_src=None, head: int = 0, out=None):
    t = torch()
    if out is None:
        out = t.empty_like(Xd)
    T = Xd.shape[-1]
    rows = Xd.numel() // T if T else 0
    rc = lib().fr_increments(dptr(Xd), C.c_int64(rows), C.c_int64(T), C.c_int64(shift),
                             dptr(out), dptr(head_src), C.c_int64(head), stream_ptr())
    check(rc, "fr_increments")
    return out


FR_LOOKUP_FAST = 16


def pathlen_lookup(Xd, norm: int = 1, relative: int = 0, scale: float = 50.0,
                   exact: bool = True):
    """relative: 0 plain, 1 divide by (last + 1e-5) first, 2 = raw cumulative
    path length without normalisation (the SharedSeedCache entry)."""
    t = torch()
    N, D, T = Xd.shape
    out = t.empty((N, T), dtype=t.float64, device=Xd.device)
    rc = lib().fr_pathlen_lookup(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
                                 C.c_int32(norm | (0 if exact else FR_LOOKUP_FAST)),
                                 C.c_int32(relative), C.c_double(scale), dptr(out), stream_ptr())
    check(rc, "fr_pathlen_lookup")
    return out


def sieve(kind: int, Ad, inc: int, cuts_d, q_d, out, out_col: int = 0):
    """Writes the features of one sieve on a (N, T) device array into columns
    [out_col, out_col + nfeatures) of the (N, F) device tensor ``out``."""
    N, T = Ad.shape
    C1 = int(cuts_d.shape[1])
    Q1 = int(q_d.numel()) if q_d is not None else 0
    base = out.data_ptr() + 8 * out_col
    rc = lib().fr_sieve(C.c_int32(kind), dptr(Ad), C.c_int64(N), C.c_int64(T),
                        C.c_int64(Ad.stride(0)), C.c_int32(inc), dptr(cuts_d),
                        C.c_int64(cuts_d.shape[0]), C.c_int32(C1), dptr(q_d), C.c_int32(Q1),
                        C.c_void_p(base), C.c_int64(out.stride(0)), stream_ptr())
    check(rc, "fr_sieve")
    return out


def sieve_implicit(kind: int, Ad, q_d, segments: bool, out, out_col: int = 0, lengths_d=None):
    """Writes the features of a PPV / CPV sieve (fr_sieve_implicit) on a (N, T) device array
    into columns [out_col, out_col + nfeatures) of the (N, F) device tensor ``out``; ``q_d``
    holds the sieve's thresholds in its own order.  ``lengths_d``: (N,) int32 device tensor,
    series n is its first ``lengths_d[n]`` elements (fr_sieve_implicit_lengths)."""
    N, T = Ad.shape
    base = out.data_ptr() + 8 * out_col
    if lengths_d is not None:
        _check_lengths_d(lengths_d, N)
        rc = lib().fr_sieve_implicit_lengths(
            C.c_int32(kind), dptr(Ad), C.c_int64(N), C.c_int64(T), C.c_int64(Ad.stride(0)),
            dptr(lengths_d), dptr(q_d), C.c_int32(int(q_d.numel())),
            C.c_int32(1 if segments else 0), C.c_void_p(base), C.c_int64(out.stride(0)),
            stream_ptr())
        check(rc, "fr_sieve_implicit_lengths")
        return out
    rc = lib().fr_sieve_implicit(C.c_int32(kind), dptr(Ad), C.c_int64(N), C.c_int64(T),
                                 C.c_int64(Ad.stride(0)), dptr(q_d), C.c_int32(int(q_d.numel())),
                                 C.c_int32(1 if segments else 0), C.c_void_p(base),
                                 C.c_int64(out.stride(0)), stream_ptr())
    check(rc, "fr_sieve_implicit")
    return out


def pre_transform(Ad, inc: int):
    """IncrementSieve._pre_transform for inc >= 0 on a (N, T) device array."""
    t = torch()
    out = t.empty_like(Ad)
    N, T = Ad.shape
    rc = lib().fr_pre_transform(dptr(Ad), C.c_int64(N), C.c_int64(T), C.c_int64(Ad.stride(0)),
                                C.c_int32(inc), dptr(out), stream_ptr())
    check(rc, "fr_pre_transform")
    return out


def select_ranks(block, job_row, job_inc, job_rank, stream=None) -> np.ndarray:
    """Order statistics of differenced (N, T) blocks of the (rows, N, T) device
    tensor ``block`` (fr_select_ranks); exact.  ``stream``: the HIP stream ``block`` was written
    on, when the call comes from another thread than the one that wrote it (the current device
    and stream are per thread)."""
    if stream is not None:
        torch().cuda.set_device(block.device)
    rows, N, T = block.shape
    jr = np.ascontiguousarray(job_row, dtype=np.int32)
    ji = np.ascontiguousarray(job_inc, dtype=np.int32)
    jk = np.ascontiguousarray(job_rank, dtype=np.int64)
    out = np.zeros(len(jr))
    if not block.is_contiguous():
        raise ValueError("block must be contiguous")
    rc = lib().fr_select_ranks(
        dptr(block), C.c_int64(rows), C.c_int64(N), C.c_int64(T), C.c_int32(len(jr)),
        jr.ctypes.data_as(C.POINTER(C.c_int32)), ji.ctypes.data_as(C.POINTER(C.c_int32)),
        jk.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_double)),
        stream_ptr() if stream is None else stream)
    check(rc, "fr_select_ranks")
    return out


class Selection:
    """fr_select_ranks_begin / _end: the selection is queued on the current stream and the call
    returns; ``result()`` waits for it and returns the values (once)."""

    def __init__(self, block, job_row, job_inc, job_rank):
        rows, N, T = block.shape
        if not block.is_contiguous():
            raise ValueError("block must be contiguous")
        jr = np.ascontiguousarray(job_row, dtype=np.int32)
        ji = np.ascontiguousarray(job_inc, dtype=np.int32)
        jk = np.ascontiguousarray(job_rank, dtype=np.int64)
        self._n = len(jr)
        self._block = block      # (read by the passes until result())
        self._vals = None
        L = lib()
        h = L.fr_select_ranks_begin(
            dptr(block), C.c_int64(rows), C.c_int64(N), C.c_int64(T), C.c_int32(self._n),
            jr.ctypes.data_as(C.POINTER(C.c_int32)), ji.ctypes.data_as(C.POINTER(C.c_int32)),
            jk.ctypes.data_as(C.POINTER(C.c_int64)), stream_ptr())
        if not h:
            raise NativeError(f"fr_select_ranks_begin: {last_error()}")
        self._h = C.c_void_p(h)

    def result(self) -> np.ndarray:
        if self._vals is None:
            out = np.zeros(self._n)
            h, self._h = self._h, None
            check(lib().fr_select_ranks_end(h, out.ctypes.data_as(C.POINTER(C.c_double))),
                  "fr_select_ranks_end")
            self._vals, self._block = out, None
        return self._vals

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and _lib is not None:
                _lib.fr_select_ranks_end(self._h, None)     # (waits, frees the handle and its scratch)
                self._h = None
        except Exception:
            pass


def _check_lengths_d(lengths_d, N: int) -> None:
    if (lengths_d.dtype != torch().int32 or lengths_d.dim() != 1 or int(lengths_d.shape[0]) != N
            or not lengths_d.is_contiguous()):
        raise TypeError("the lengths must be a contiguous int32 (N,) device tensor")


def standardize(Xd, div_std: bool, eps: float, lengths_d=None):
    """STD per row; ``lengths_d``: (N,) int32 device tensor for an (N, D, T) ``Xd`` - the
    statistics of series n are those of its first ``lengths_d[n]`` elements
    (fr_standardize_lengths)."""
    t = torch()
    out = t.empty_like(Xd)
    T = Xd.shape[-1]
    rows = Xd.numel() // T if T else 0
    if lengths_d is not None:
        if Xd.dim() != 3 or not Xd.is_contiguous():
            raise TypeError("X must be a contiguous (N, D, T) device tensor")
        _check_lengths_d(lengths_d, int(Xd.shape[0]))
        rc = lib().fr_standardize_lengths(dptr(Xd), C.c_int64(Xd.shape[0]), C.c_int64(Xd.shape[1]),
                                          C.c_int64(T), dptr(lengths_d),
                                          C.c_int32(1 if div_std else 0), C.c_double(eps),
                                          dptr(out), stream_ptr())
        check(rc, "fr_standardize_lengths")
        return out
    rc = lib().fr_standardize(dptr(Xd), C.c_int64(rows), C.c_int64(T),
                              C.c_int32(1 if div_std else 0), C.c_double(eps), dptr(out),
                              stream_ptr())
    check(rc, "fr_standardize")
    return out


def coswiss_combine(terms_d, begin_d, coeff_d, desc_d, trig_d, out, out_row_stride: int):
    """out[j] = sum of the weighted terms of output row j (fr_coswiss_combine);
    ``out`` is a device view whose rows are ``out_row_stride`` doubles apart."""
    n_terms, N, T = (int(v) for v in terms_d.shape)
    n_out = int(begin_d.shape[0]) - 1
    rc = lib().fr_coswiss_combine(dptr(terms_d), C.c_int64(n_terms), C.c_int64(N), C.c_int64(T),
                                  C.c_int32(n_out), dptr(begin_d), dptr(coeff_d), dptr(desc_d),
                                  dptr(trig_d), dptr(out), C.c_int64(out_row_stride),
                                  stream_ptr())
    check(rc, "fr_coswiss_combine")
    return out


def release_scratch() -> None:
    """Frees the grow-only device scratch of fr_select_ranks (kept between the calls of one fit)."""
    check(lib().fr_release_scratch(), "fr_release_scratch")


def nan_to_num(xd):
    """In place np.nan_to_num(x, nan=0.0) of a contiguous float64 device tensor."""
    if not xd.is_contiguous():
        raise TypeError("nan_to_num needs a contiguous tensor")
    check(lib().fr_nan_to_num(dptr(xd), C.c_int64(xd.numel()), stream_ptr()), "fr_nan_to_num")
    return xd


def arctic_argmax(Vd, word_lengths) -> "object":
    """fr_arctic_argmax: the rows of Arctic(argmax=True) from the running maxima ``Vd``
    (sum(L), N, T) of all prefixes of all words (lengths ``word_lengths``)."""
    t = torch()
    rows, N, T = (int(v) for v in Vd.shape)
    jobs, v0, o0 = [], 0, 0
    for L in word_lengths:
        for k in range(L):
            jobs.append((v0, k, o0 + k + k * (k + 1) // 2))
        v0 += L
        o0 += L + L * (L + 1) // 2
    if v0 != rows:
        raise ValueError("Vd must hold one row per prefix of every word")
    if max(word_lengths, default=0) > 63:
        raise NotImplementedError("Arctic argmax: words of more than 63 letters")
    out = t.empty((o0, N, T), dtype=t.float64, device=Vd.device)
    if not jobs or N == 0 or T == 0:
        return out
    jd = to_device(np.asarray(jobs, dtype=np.int32), dtype=np.int32)
    P = t.empty_like(Vd)
    check(lib().fr_arctic_argmax(dptr(Vd), C.c_int64(rows), C.c_int64(N), C.c_int64(T),
                                 C.c_int32(len(jobs)), dptr(jd), dptr(P), dptr(out), stream_ptr()),
          "fr_arctic_argmax")
    return out


# ----------------------------------------------------------------------- preparateurs
def _rows3(Xd):
    t = torch()
    if Xd.dtype != t.float64 or Xd.dim() != 3 or not Xd.is_contiguous():
        raise TypeError("X must be a contiguous float64 (N, D, T) device tensor")
    return (int(v) for v in Xd.shape)


def _prep_out(out, shape, like):
    """The output tensor of a preparateur entry: ``out`` if given (checked), else a new one."""
    t = torch()
    if out is None:
        return t.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or not out.is_contiguous() \
            or out.device != like.device:
        raise TypeError(f"out must be a contiguous float64 device tensor of shape {tuple(shape)}")
    return out


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def prep_fir(Xd, kernel_d, w: int, ndim_d, dims_d, ndim_h, dims_h, adaptive: bool = False,
             out=None):
    """fr_prep_fir, mode 0 (RIN): ``kernel_d`` (J, w), ``ndim_d`` (O) and ``dims_d`` (J) device
    tensors, ``ndim_h`` / ``dims_h`` the same tables as int32 host arrays (checked by the
    library).  Returns (N, O, T)."""
    N, D, T = _rows3(Xd)
    nh = np.ascontiguousarray(ndim_h, dtype=np.int32)
    dh = np.ascontiguousarray(dims_h, dtype=np.int32)
    out = _prep_out(out, (N, nh.size, T), Xd)
    check(lib().fr_prep_fir(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(kernel_d),
                            C.c_int32(dh.size), C.c_int32(int(w)), dptr(ndim_d), C.c_int32(nh.size),
                            dptr(dims_d), _i32p(nh), _i32p(dh), C.c_int32(0),
                            C.c_int32(1 if adaptive else 0), dptr(out), stream_ptr()), "fr_prep_fir")
    return out


def prep_moving_average(Xd, w: int, out=None):
    """fr_prep_fir, mode 1 (MAV): 1 <= w <= T."""
    N, D, T = _rows3(Xd)
    out = _prep_out(out, (N, D, T), Xd)
    check(lib().fr_prep_fir(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), None, C.c_int32(0),
                            C.c_int32(int(w)), None, C.c_int32(0), None, None, None, C.c_int32(1),
                            C.c_int32(0), dptr(out), stream_ptr()), "fr_prep_fir")
    return out


def prep_project(Xd, kernel_d, bias_d, ndim_d, dims_d, ndim_h, dims_h, out=None):
    """fr_prep_project without a hidden layer (JLD); tables as in ``prep_fir``."""
    N, D, T = _rows3(Xd)
    nh = np.ascontiguousarray(ndim_h, dtype=np.int32)
    dh = np.ascontiguousarray(dims_h, dtype=np.int32)
    out = _prep_out(out, (N, nh.size, T), Xd)
    check(lib().fr_prep_project(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(kernel_d),
                                dptr(bias_d), dptr(ndim_d), C.c_int32(nh.size), dptr(dims_d),
                                C.c_int32(dh.size), _i32p(nh), _i32p(dh), None, None, None,
                                C.c_int32(0), C.c_int32(0), dptr(out), stream_ptr()),
          "fr_prep_project")
    return out


def prep_ffn(Xd, W1_d, b1_d, W2_d, center: bool, relu_out: bool, out=None):
    """fr_prep_project with a hidden layer (FFN): ``W1_d`` (hidden, D), ``b1_d`` (hidden),
    ``W2_d`` (O, hidden) device tensors."""
    N, D, T = _rows3(Xd)
    hidden, O = int(W1_d.shape[0]), int(W2_d.shape[0])
    if tuple(W1_d.shape) != (hidden, D) or tuple(b1_d.shape) != (hidden,) \
            or tuple(W2_d.shape) != (O, hidden) or hidden < 1:
        raise ValueError("FFN weights do not match the input dimensions")
    out = _prep_out(out, (N, O, T), Xd)
    check(lib().fr_prep_project(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), None, None, None,
                                C.c_int32(O), None, C.c_int32(0), None, None, dptr(W1_d), dptr(b1_d),
                                dptr(W2_d), C.c_int32(hidden),
                                C.c_int32((1 if center else 0) | (2 if relu_out else 0)), dptr(out),
                                stream_ptr()), "fr_prep_project")
    return out


def prep_normalize(Xd, scale_dim: bool, out=None):
    N, D, T = _rows3(Xd)
    out = _prep_out(out, (N, D, T), Xd)
    check(lib().fr_prep_normalize(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
                                  C.c_int32(1 if scale_dim else 0), dptr(out), stream_ptr()),
          "fr_prep_normalize")
    return out


def prep_leadlag(Xd, out=None):
    N, D, T = _rows3(Xd)
    out = _prep_out(out, (N, 2 * D, 2 * T - 1), Xd)
    check(lib().fr_prep_leadlag(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(out),
                                stream_ptr()), "fr_prep_leadlag")
    return out


def prep_mask(Xd, mask_d=None, cs_d=None, ce_d=None, out=None):
    """fr_prep_mask: ``out = keep ? X : +0.0``.  ``mask_d``: ceil(T / 32) 32-bit words (an int32
    device tensor, bit ``t % 32`` of word ``t // 32`` keeps time step ``t``) shared by all series;
    ``cs_d`` / ``ce_d``: int64 device tensors of at least N counts, series n keeps the slice
    ``[cs[n] - 1 : ce[n]]``.  Either source may be absent."""
    t = torch()
    N, D, T = _rows3(Xd)
    words = 0
    if mask_d is not None:
        if mask_d.dtype != t.int32 or mask_d.dim() != 1 or not mask_d.is_contiguous():
            raise TypeError("the time mask must be a contiguous int32 device tensor of words")
        words = int(mask_d.numel())
    windows = 0
    if cs_d is not None or ce_d is not None:
        for c in (cs_d, ce_d):
            if c is None or c.dtype != t.int64 or c.dim() != 1 or not c.is_contiguous():
                raise TypeError("window counts must be contiguous int64 (N) device tensors")
        windows = min(int(cs_d.numel()), int(ce_d.numel()))
    out = _prep_out(out, (N, D, T), Xd)
    check(lib().fr_prep_mask(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(mask_d),
                             C.c_int64(words), dptr(cs_d), dptr(ce_d), C.c_int64(windows),
                             dptr(out), stream_ptr()), "fr_prep_mask")
    return out


def prep_pointwise(mode: int, Xd, w_d=None, w2_d=None, shift: int = 0, q: float = 0.0,
                   v: float = 0.0, flags: int = 0, out=None):
    """fr_prep_pointwise.  FR_PW_MUL / FR_PW_ADD: ``w_d`` (Nw, T), the result has
    ``max(N, Nw)`` series; FR_PW_ROTATE: ``w_d`` / ``w2_d`` the (T) cosines / sines; FR_PW_POW:
    ``w_d`` (D) exponents; FR_PW_SHIFT: ``shift``; FR_PW_CLIP: ``q``, ``v``."""
    t = torch()
    N, D, T = _rows3(Xd)
    Nw, n_out = 0, N
    for tab in (w_d, w2_d):
        if tab is not None and (tab.dtype != t.float64 or not tab.is_contiguous()):
            raise TypeError("tables must be contiguous float64 device tensors")
    if mode in (FR_PW_MUL, FR_PW_ADD):
        if w_d is None or w_d.dim() != 2 or int(w_d.shape[1]) != T:
            raise ValueError("the table of FR_PW_MUL / FR_PW_ADD must be (Nw, T)")
        Nw = int(w_d.shape[0])
        if N and Nw and (N == Nw or N == 1 or Nw == 1):
            n_out = max(N, Nw)
    elif mode == FR_PW_ROTATE:
        if w_d is None or w2_d is None or w_d.numel() != T or w2_d.numel() != T:
            raise ValueError("a rotation needs (T) cosines and (T) sines")
    elif mode == FR_PW_POW:
        if w_d is None or w_d.numel() != D:
            raise ValueError("one exponent per dimension")
    out = _prep_out(out, (n_out, D, T), Xd)
    check(lib().fr_prep_pointwise(C.c_int32(int(mode)), dptr(Xd), C.c_int64(N), C.c_int64(D),
                                  C.c_int64(T), dptr(w_d), C.c_int64(Nw), dptr(w2_d),
                                  C.c_int64(int(shift)), C.c_double(float(q)), C.c_double(float(v)),
                                  C.c_int32(int(flags)), dptr(out), stream_ptr()),
          "fr_prep_pointwise")
    return out


# ----------------------------------------------------------------------- generic words
def letter_rows(Xd, spec, ext_d=None, one_is_zero: bool = False, out=None, spec_d=None):
    """fr_letter_rows: the ``(N, Dv, T)`` virtual input rows of lowered generic words
    (fruits_amd/iss/lowering.py).  ``spec``: ``(Dv, 3)`` int32 host array of
    ``(kind, source, shift)``, kinds ``FR_ROW_*``; ``ext_d``: ``(N, H, T)`` device tensor of the
    values the Python letters gave, for the ``FR_ROW_EXT`` rows; ``spec_d``: the device copy of
    ``spec`` if the caller keeps one (else it is uploaded here)."""
    t = torch()
    N, D, T = _rows3(Xd)
    sp = np.ascontiguousarray(spec, dtype=np.int32)
    if sp.ndim != 2 or sp.shape[1] != 3 or sp.shape[0] < 1:
        raise ValueError("the row specification must be (Dv, 3) int32")
    H = 0
    if ext_d is not None:
        if ext_d.dtype != t.float64 or ext_d.dim() != 3 or not ext_d.is_contiguous() \
                or int(ext_d.shape[0]) != N or int(ext_d.shape[2]) != T:
            raise TypeError("letter values must be a contiguous float64 (N, H, T) device tensor")
        H = int(ext_d.shape[1])
    out = _prep_out(out, (N, sp.shape[0], T), Xd)
    sp_d = spec_d if spec_d is not None else to_device(sp, dtype=np.int32)
    if sp_d.dtype != t.int32 or tuple(sp_d.shape) != sp.shape or not sp_d.is_contiguous():
        raise TypeError("the device copy of the row specification must be (Dv, 3) int32")
    check(lib().fr_letter_rows(dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
                               dptr(ext_d if H else None), C.c_int64(H), dptr(sp_d), _i32p(sp),
                               C.c_int32(sp.shape[0]), C.c_int32(1 if one_is_zero else 0),
                               dptr(out), stream_ptr()), "fr_letter_rows")
    return out


def rows_unshift(Ad, shifts, out=None, shifts_d=None):
    """fr_rows_unshift: ``out[k, n, t] = A[k, n, t - shifts[k]]`` for ``t >= shifts[k]``, +0.0
    in front; ``Ad`` ``(K, N, T)``, ``out`` a distinct buffer of the same shape."""
    t = torch()
    if Ad.dtype != t.float64 or Ad.dim() != 3 or not Ad.is_contiguous():
        raise TypeError("A must be a contiguous float64 (K, N, T) device tensor")
    K, N, T = (int(v) for v in Ad.shape)
    sh = np.ascontiguousarray(shifts, dtype=np.int32)
    if sh.shape != (K,):
        raise ValueError("one shift per row")
    out = _prep_out(out, (K, N, T), Ad)
    sh_d = shifts_d if shifts_d is not None else to_device(sh, dtype=np.int32)
    if sh_d.dtype != t.int32 or tuple(sh_d.shape) != (K,) or not sh_d.is_contiguous():
        raise TypeError("the device copy of the shifts must be (K) int32")
    check(lib().fr_rows_unshift(dptr(Ad), C.c_int64(K), C.c_int64(N), C.c_int64(T), dptr(sh_d),
                                _i32p(sh), dptr(out), stream_ptr()), "fr_rows_unshift")
    return out


# ----------------------------------------------------------------------- backward pass
def _backward_args(prefix_plan: Plan, Xd, G, row_prefix):
    """What the backward entries share: ``(N, D, T, K, V)``, the row map as a contiguous int32
    host array and the strides of the checked upstream gradient."""
    t = torch()
    N, D, T = _rows3(Xd)
    rp = np.ascontiguousarray(row_prefix, dtype=np.int32)
    K = int(rp.shape[0])
    if G.dtype != t.float64 or tuple(G.shape) != (N, K, T) or G.device != Xd.device:
        raise TypeError("the upstream gradient must be a float64 (N, K, T) tensor on the input's device")
    return (N, D, T, K, prefix_plan.rows), rp, [C.c_int64(int(s)) for s in G.stride()]


class _grad_lengths:
    """Set, call, clear: the plan is armed with the ``(N,)`` int32 device lengths
    (fr_plan_set_grad_lengths) for the one ABI call inside the block; None arms nothing.  The
    entry reads the pointer once and hands it to its kernels by value, so clearing it behind the
    call is safe; the caller keeps the tensor alive, as it keeps ``Xd``."""

    def __init__(self, prefix_plan: "Plan", lengths_d, Xd) -> None:
        self.plan, self.lengths_d = prefix_plan, lengths_d
        if lengths_d is not None:
            t = torch()
            if (lengths_d.dtype != t.int32 or tuple(lengths_d.shape) != (int(Xd.shape[0]),)
                    or not lengths_d.is_contiguous() or lengths_d.device != Xd.device):
                raise TypeError("the lengths must be a contiguous int32 (N,) tensor on the input's device")

    def __enter__(self):
        if self.lengths_d is not None:
            check(lib().fr_plan_set_grad_lengths(self.plan._h, C.c_void_p(self.lengths_d.data_ptr()),
                                                 C.c_int64(int(self.lengths_d.shape[0]))),
                  "fr_plan_set_grad_lengths")
        return self

    def __exit__(self, *exc):
        if self.lengths_d is not None:
            check(lib().fr_plan_set_grad_lengths(self.plan._h, None, 0), "fr_plan_set_grad_lengths")
        return False


def _backward_scratch(work, need: int, what: str, Xd):
    """The caller's scratch if it holds ``need`` doubles (``what``: that number in words), or a
    fresh one."""
    t = torch()
    if work is None:
        return t.empty((need,), dtype=t.float64, device=Xd.device)
    if work.dtype != t.float64 or work.numel() < need or not work.is_contiguous():
        raise TypeError(f"the scratch must be a contiguous float64 device tensor of {what} elements")
    return work


def iss_backward(prefix_plan: Plan, Xd, Sd, G, row_prefix, work=None, entry="fr_iss_backward",
                 lengths_d=None):
    """fr_iss_backward: the gradient ``(N, D, T)`` of unweighted Reals iterated sums with respect
    to ``Xd``.  ``prefix_plan``: the plan of the distinct prefixes, each with depth 1; ``Sd``
    ``(V, N, T)`` its output on ``Xd``; ``G`` the upstream gradient as an ``(N, K, T)`` device
    tensor of any strides; ``row_prefix`` ``(K)`` int32 host array, the row of ``Sd`` that output
    row k is; ``work``: a ``(V, N, T)`` scratch if the caller keeps one.  ``entry``: the ABI
    entry that takes these arguments (``iss_backward_max``).  ``lengths_d``: ``(N,)`` int32
    device lengths in ``1..T`` - series n is its first ``lengths_d[n]`` steps, the gradient behind
    them is +0.0 and ``G`` is not read there (fr_plan_set_grad_lengths around the call)."""
    t = torch()
    (N, D, T, K, V), rp, (sn, sk, st) = _backward_args(prefix_plan, Xd, G, row_prefix)
    if Sd.dtype != t.float64 or tuple(Sd.shape) != (V, N, T) or not Sd.is_contiguous():
        raise TypeError("the prefix sums must be a contiguous float64 (V, N, T) device tensor")
    work = _backward_scratch(work, V * N * T, "V * N * T", Xd)
    dX = t.empty((N, D, T), dtype=t.float64, device=Xd.device)
    with _grad_lengths(prefix_plan, lengths_d, Xd):
        check(getattr(lib(), entry)(prefix_plan._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T),
                                    dptr(Sd), dptr(G), C.c_int64(K), sn, sk, st, _i32p(rp), dptr(work),
                                    dptr(dX), stream_ptr()),
              entry)
    return dX


def iss_backward_max(prefix_plan: Plan, Xd, Sd, G, row_prefix, work=None, lengths_d=None):
    """fr_iss_backward_max: the gradient ``(N, D, T)`` of unweighted Arctic or Bayesian iterated
    sums with respect to ``Xd``; the arguments of ``iss_backward``, ``prefix_plan`` created with
    ``arctic=True`` or ``bayesian=True``."""
    return iss_backward(prefix_plan, Xd, Sd, G, row_prefix, work, entry="fr_iss_backward_max",
                        lengths_d=lengths_d)


class _grad_pathlen:
    """Set, call, clear, as ``_grad_lengths``: the plan is armed with the path-length lookup's
    ``(norm, scale)`` and its scratches (fr_plan_set_grad_pathlen) for the one ABI call inside
    the block; ``pathlen=None`` arms nothing."""

    def __init__(self, prefix_plan: "Plan", pathlen, N: int, dg, R) -> None:
        self.plan, self.pathlen, self.N, self.dg, self.R = prefix_plan, pathlen, N, dg, R

    def __enter__(self):
        if self.pathlen is not None:
            norm, scale = self.pathlen
            check(lib().fr_plan_set_grad_pathlen(self.plan._h, C.c_int64(self.N), C.c_int32(int(norm)),
                                                 C.c_double(float(scale)), dptr(self.dg),
                                                 dptr(self.R) if self.R is not None else None),
                  "fr_plan_set_grad_pathlen")
        return self

    def __exit__(self, *exc):
        if self.pathlen is not None:
            rc = lib().fr_plan_set_grad_pathlen(self.plan._h, C.c_int64(0), C.c_int32(0), C.c_double(0.0),
                                                None, None)
            if exc[0] is None:          # (an error of the armed call is the one to report)
                check(rc, "fr_plan_set_grad_pathlen")
        return False


def iss_backward_weighted(prefix_plan: Plan, Xd, lookup_d, G, row_prefix, work=None, lengths_d=None,
                          pathlen=None, return_dg: bool = False):
    """fr_iss_backward_weighted: the gradient ``(N, D, T)`` of weighted Reals iterated sums with
    respect to ``Xd``, the lookup being a constant.  ``prefix_plan``: the weighted plan of the
    distinct (letters, alphas) prefixes, each with depth 1; ``lookup_d`` ``(1 | N, T)`` the
    weighting's device lookup; ``G`` and ``row_prefix`` as in ``iss_backward``.  The entry forms
    the carried sums itself: it takes no output of the plan.  ``work``: a scratch of
    ``2 V N T + 2 alphas rows T`` doubles if the caller keeps one.  ``lengths_d`` as in
    ``iss_backward``; row n of an ``(N, T)`` lookup is then the row of a series of that length.

    ``pathlen=(norm, scale)``: ``lookup_d`` ``(N, T)`` is the path-length lookup of ``Xd`` itself -
    ``pathlen_lookup(Xd, norm, relative, scale)`` - and the gradient flows through it into
    dimension 0 too (fr_plan_set_grad_pathlen around the call).  The ``(N, T)``
    scratch ``dg = dL/dg`` is allocated here and a non-total plan's ``work`` holds ``V N T`` more
    doubles; ``return_dg=True`` hands back ``(dX, dg)``."""
    t = torch()
    (N, D, T, K, V), rp, (sn, sk, st) = _backward_args(prefix_plan, Xd, G, row_prefix)
    if (lookup_d is None or lookup_d.dtype != t.float64 or lookup_d.dim() != 2
            or int(lookup_d.shape[1]) != T or int(lookup_d.shape[0]) not in (1, N)
            or not lookup_d.is_contiguous() or lookup_d.device != Xd.device):
        raise TypeError("the lookup must be a contiguous float64 (1 | N, T) tensor on the input's device")
    rows = int(lookup_d.shape[0])
    cells, aux = V * N * T, 2 * prefix_plan.info(FR_INFO_ALPHAS) * rows * T
    dg = R = None
    need, what = 2 * cells + aux, "2 V N T + 2 alphas rows T"
    keeps_r = pathlen is not None and prefix_plan.weighting != FR_W_TOTAL
    if keeps_r:
        # (+ 1: an empty batch still gets an address, here and for dg)
        need, what = need + cells + 1, "3 V N T + 2 alphas rows T + 1"
    work = _backward_scratch(work, need, what, Xd).view(-1)
    if pathlen is not None:
        dg = t.empty((N * T + 1,), dtype=t.float64, device=Xd.device)
        R = work[2 * cells + aux:] if keeps_r else None
    dX = t.empty((N, D, T), dtype=t.float64, device=Xd.device)
    # (the scratch in three parts; an empty part still gets a distinct address)
    parts = [C.c_void_p(work.data_ptr() + 8 * o) for o in (0, cells, 2 * cells)]
    with _grad_lengths(prefix_plan, lengths_d, Xd), _grad_pathlen(prefix_plan, pathlen, N, dg, R):
        check(lib().fr_iss_backward_weighted(
            prefix_plan._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), dptr(lookup_d),
            C.c_int64(rows), dptr(G), C.c_int64(K), sn, sk, st,
            _i32p(rp), parts[0], parts[1], parts[2], dptr(dX), stream_ptr()), "fr_iss_backward_weighted")
    if pathlen is not None and return_dg:
        return dX, dg[:N * T].view(N, T)
    return dX


def coswiss_grad_rows(plan: "CosPlan"):
    """(rows of d_S, rows of d_A): the scratch ``fr_iss_backward`` needs for a CosWISS plan, in
    rows of ``N * T`` doubles (fr_plan_info, FR_INFO_GRAD_ROWS)."""
    word = int(plan.info(FR_INFO_GRAD_ROWS))
    return word >> 32, word & 0xffffffff


def iss_backward_cos(plan: "CosPlan", Xd, G, row_unit, work=None):
    """fr_iss_backward with a CosWISS plan: the gradient ``(N, D, T)`` of the plan's rows with
    respect to ``Xd``.  ``plan``: the CosWISS plan itself; ``G`` the upstream gradient as an
    ``(N, K, T)`` device tensor of any strides; ``row_unit`` ``(K)`` int32 host array, the row of
    the plan (word-major, F rows per word) that row k of ``G`` belongs to - several k may name one
    row, a row none.  ``work``: a scratch of ``(rows of d_S + rows of d_A) * N * T`` doubles
    (``coswiss_grad_rows``) if the caller keeps one."""
    t = torch()
    (N, D, T, K, _), rp, (sn, sk, st) = _backward_args(plan, Xd, G, row_unit)
    rows_s, rows_a = coswiss_grad_rows(plan)
    cells = N * T
    work = _backward_scratch(work, (rows_s + rows_a) * cells, "(rows of d_S + rows of d_A) * N * T", Xd).view(-1)
    dX = t.empty((N, D, T), dtype=t.float64, device=Xd.device)
    # (the scratch in two parts; an empty part still gets a distinct address)
    parts = [C.c_void_p(work.data_ptr() + 8 * o) for o in (rows_a * cells, 0)]
    check(lib().fr_iss_backward(plan._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), parts[0],
                                dptr(G), C.c_int64(K), sn, sk, st, _i32p(rp), parts[1], dptr(dX),
                                stream_ptr()), "fr_iss_backward")
    return dX


# ----------------------------------------------------------------------- differentiable features
def _head_tables(spec, spec_d, cuts_d, q_d, N: int, cols: int = 7):
    """The spec table ``(n_sieves, cols)`` of fr_sieve_pick (6) or fr_sieve_heads (7) as a
    contiguous int32 host array, after the checks of its device tables."""
    t = torch()
    sp = np.ascontiguousarray(spec, dtype=np.int32)
    if sp.ndim != 2 or sp.shape[1] != cols:
        raise ValueError(f"the spec table is (n_sieves, {cols})")
    if (spec_d.dtype != t.int32 or tuple(spec_d.shape) != sp.shape or not spec_d.is_contiguous()
            or cuts_d.dtype != t.int64 or not cuts_d.is_contiguous()
            or (sp.shape[0] > 0 and (sp[0, 0] & FR_SIEVE_SERIES_CUTS)
                and (cuts_d.dim() != 2 or int(cuts_d.shape[0]) != N))
            or (q_d is not None and (q_d.dtype != t.float64 or not q_d.is_contiguous()))):
        raise TypeError("the device tables must be contiguous: spec int32 like the host table, "
                        "cuts int64 (per-series cuts: (N, row)), thresholds float64")
    return sp


def sieve_pick(Ad, spec, spec_d, cuts_d, q_d, F: int):
    """fr_sieve_pick: the selecting sieves END / MAX / MIN over every row of the contiguous
    ``(K, N, T)`` device tensor ``Ad`` in one launch.  ``spec`` ``(n_sieves, 6)`` int32 host
    array ``{kind, cut_begin, C1, q_begin, Q1, feat_begin}`` per sieve (checked by the library),
    ``spec_d`` its device copy, ``cuts_d`` int64 and ``q_d`` float64 the flat device tables the
    spec indexes.  Per-series cuts: every kind of the spec carries ``FR_SIEVE_SERIES_CUTS`` and
    ``cuts_d`` is the contiguous ``(N, row)`` table whose row n holds the cut rows of series n,
    which the spec's ``cut_begin`` index.  Returns ``(features (N, K, F) float64, positions (N, K, F) int32)``: of every
    feature its value and the step of its row that it selects, -1 where it selects none."""
    t = torch()
    if Ad.dtype != t.float64 or Ad.dim() != 3 or not Ad.is_contiguous():
        raise TypeError("A must be a contiguous float64 (K, N, T) device tensor")
    K, N, T = (int(v) for v in Ad.shape)
    sp = _head_tables(spec, spec_d, cuts_d, q_d, N, 6)
    feat = t.empty((N, K, int(F)), dtype=t.float64, device=Ad.device)
    pos = t.empty((N, K, int(F)), dtype=t.int32, device=Ad.device)
    check(lib().fr_sieve_pick(dptr(Ad), C.c_int64(K), C.c_int64(N), C.c_int64(T), dptr(spec_d),
                              _i32p(sp), C.c_int32(sp.shape[0]), dptr(cuts_d),
                              C.c_int64(int(cuts_d.numel())), dptr(q_d),
                              C.c_int64(int(q_d.numel()) if q_d is not None else 0),
                              C.c_int32(int(F)), dptr(feat), dptr(pos), stream_ptr()),
          "fr_sieve_pick")
    return feat, pos


def iss_backward_picked(prefix_plan: Plan, Xd, pos_d, w_d, row_prefix, Sd=None, lookup_d=None,
                        lengths_d=None):
    """fr_iss_backward_picked: the gradient ``(N, D, T)`` of picked features of iterated sums
    with respect to ``Xd`` - the adjoint the plan's kind names, with a sparse upstream.
    ``pos_d`` ``(N, K, F)`` int32 and ``w_d`` ``(N, K, F)`` float64, contiguous: the weight
    ``w_d[n, k, f]`` reaches step ``pos_d[n, k, f]`` of row k, nothing where that is negative.
    ``Sd``: an unweighted plan's output on ``Xd`` ``(V, N, T)``; ``lookup_d``: a weighted plan's
    ``(1 | N, T)`` lookup.  ``row_prefix`` and ``lengths_d`` as in ``iss_backward``."""
    t = torch()
    N, D, T = _rows3(Xd)
    rp = np.ascontiguousarray(row_prefix, dtype=np.int32)
    K, V = int(rp.shape[0]), prefix_plan.rows
    if (pos_d.dtype != t.int32 or pos_d.dim() != 3 or tuple(pos_d.shape[:2]) != (N, K)
            or not pos_d.is_contiguous() or pos_d.device != Xd.device):
        raise TypeError("the positions must be a contiguous int32 (N, K, F) tensor on the input's device")
    F = int(pos_d.shape[2])
    if (w_d.dtype != t.float64 or tuple(w_d.shape) != (N, K, F) or not w_d.is_contiguous()
            or w_d.device != Xd.device):
        raise TypeError("the weights must be a contiguous float64 (N, K, F) tensor on the input's device")
    cells = V * N * T
    dX = t.empty((N, D, T), dtype=t.float64, device=Xd.device)
    null = C.c_void_p(0)
    if prefix_plan.weighting != FR_W_NONE:
        if (lookup_d is None or lookup_d.dtype != t.float64 or lookup_d.dim() != 2
                or int(lookup_d.shape[1]) != T or int(lookup_d.shape[0]) not in (1, N)
                or not lookup_d.is_contiguous() or lookup_d.device != Xd.device):
            raise TypeError("the lookup must be a contiguous float64 (1 | N, T) tensor on the input's device")
        rows = int(lookup_d.shape[0])
        aux = 2 * prefix_plan.info(FR_INFO_ALPHAS) * rows * T
        work = _backward_scratch(None, 2 * cells + aux, "2 V N T + 2 alphas rows T", Xd)
        # (the scratch in three parts; an empty part still gets a distinct address)
        Cs, A, ax = (C.c_void_p(work.data_ptr() + 8 * o) for o in (0, cells, 2 * cells))
        S, lk = null, dptr(lookup_d)
    else:
        if Sd is None or Sd.dtype != t.float64 or tuple(Sd.shape) != (V, N, T) or not Sd.is_contiguous():
            raise TypeError("the prefix sums must be a contiguous float64 (V, N, T) device tensor")
        work = _backward_scratch(None, cells, "V * N * T", Xd)
        Cs, A, ax, S, lk, rows = null, dptr(work), null, dptr(Sd), null, 0
    with _grad_lengths(prefix_plan, lengths_d, Xd):
        check(lib().fr_iss_backward_picked(
            prefix_plan._h, dptr(Xd), C.c_int64(N), C.c_int64(D), C.c_int64(T), S, lk, C.c_int64(rows),
            dptr(pos_d), dptr(w_d), C.c_int64(K), C.c_int32(F), _i32p(rp), Cs, A, ax, dptr(dX),
            stream_ptr()), "fr_iss_backward_picked")
    return dX


def sieve_heads(Ad, spec, spec_d, cuts_d, q_d, F: int):
    """fr_sieve_heads: the heads END / MAX / MIN / MPI / CUR over every row of the contiguous
    ``(K, N, T)`` device tensor ``Ad`` in one launch.  The tables are ``sieve_pick``'s with a
    seventh spec column, the differencing order ``{kind, cut_begin, C1, q_begin, Q1, feat_begin,
    inc}``.  Returns ``(features (N, K, F) float64, companion (N, K, F) int32)``: the position of
    a selecting feature, the in-band count of an ``MPI`` / ``CUR`` one."""
    t = torch()
    if Ad.dtype != t.float64 or Ad.dim() != 3 or not Ad.is_contiguous():
        raise TypeError("A must be a contiguous float64 (K, N, T) device tensor")
    K, N, T = (int(v) for v in Ad.shape)
    sp = _head_tables(spec, spec_d, cuts_d, q_d, N)
    feat = t.empty((N, K, int(F)), dtype=t.float64, device=Ad.device)
    comp = t.empty((N, K, int(F)), dtype=t.int32, device=Ad.device)
    check(lib().fr_sieve_heads(dptr(Ad), C.c_int64(K), C.c_int64(N), C.c_int64(T), dptr(spec_d),
                               _i32p(sp), C.c_int32(sp.shape[0]), dptr(cuts_d),
                               C.c_int64(int(cuts_d.numel())), dptr(q_d),
                               C.c_int64(int(q_d.numel()) if q_d is not None else 0),
                               C.c_int32(int(F)), dptr(feat), dptr(comp), stream_ptr()),
          "fr_sieve_heads")
    return feat, comp


def sieve_heads_adjoint(rows_d, spec, spec_d, cuts_d, q_d, comp_d, g_d, row_map=None, row_map_d=None,
                        lengths_d=None):
    """fr_sieve_heads_adjoint: the dense gradient ``(N, K, T)`` of the rows that the feature
    gradients ``g_d`` ``(N, K, F)`` float64 are, every element written.  ``rows_d``: the
    contiguous ``(V, N, T)`` device tensor that holds the rows ``sieve_heads`` saw; ``row_map``
    ``(K)`` int32 host array with its device copy ``row_map_d``: row k of the features is row
    ``row_map[k]`` of ``rows_d`` (neither: ``V == K``, row k).  ``comp_d``: the companion
    ``sieve_heads`` returned; the tables as there.  ``lengths_d``: the ``(N,)`` int32 device
    lengths of a ragged batch, or None."""
    t = torch()
    if rows_d.dtype != t.float64 or rows_d.dim() != 3 or not rows_d.is_contiguous():
        raise TypeError("the rows must be a contiguous float64 (V, N, T) device tensor")
    V, N, T = (int(v) for v in rows_d.shape)
    sp = _head_tables(spec, spec_d, cuts_d, q_d, N)
    if (comp_d.dtype != t.int32 or comp_d.dim() != 3 or int(comp_d.shape[0]) != N
            or not comp_d.is_contiguous() or comp_d.device != rows_d.device):
        raise TypeError("the companion must be a contiguous int32 (N, K, F) tensor on the rows' device")
    K, F = int(comp_d.shape[1]), int(comp_d.shape[2])
    if (g_d.dtype != t.float64 or tuple(g_d.shape) != (N, K, F) or not g_d.is_contiguous()
            or g_d.device != rows_d.device):
        raise TypeError("the feature gradients must be a contiguous float64 (N, K, F) tensor on the rows' device")
    rm = None
    if row_map is not None:
        rm = np.ascontiguousarray(row_map, dtype=np.int32)
        if (rm.shape != (K,) or row_map_d is None or row_map_d.dtype != t.int32
                or tuple(row_map_d.shape) != (K,) or not row_map_d.is_contiguous()):
            raise TypeError("the row map is a (K,) int32 host array with a contiguous device copy")
    if lengths_d is not None and (lengths_d.dtype != t.int32 or tuple(lengths_d.shape) != (N,)
                                  or not lengths_d.is_contiguous() or lengths_d.device != rows_d.device):
        raise TypeError("the lengths must be a contiguous int32 (N,) tensor on the rows' device")
    G = t.empty((N, K, T), dtype=t.float64, device=rows_d.device)
    check(lib().fr_sieve_heads_adjoint(
        dptr(rows_d), C.c_int64(V), dptr(row_map_d) if rm is not None else None,
        _i32p(rm) if rm is not None else None, C.c_int64(K), C.c_int64(N), C.c_int64(T), dptr(spec_d),
        _i32p(sp), C.c_int32(sp.shape[0]), dptr(cuts_d), C.c_int64(int(cuts_d.numel())), dptr(q_d),
        C.c_int64(int(q_d.numel()) if q_d is not None else 0), C.c_int32(F), dptr(comp_d), dptr(g_d),
        dptr(lengths_d) if lengths_d is not None else None, dptr(G), stream_ptr()),
        "fr_sieve_heads_adjoint")
    return G
