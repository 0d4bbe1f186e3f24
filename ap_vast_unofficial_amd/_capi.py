"""ctypes binding of libapvast_hip.so (contract: include/apvast_hip.h).

No fallback: if the HIP library is missing or a call fails this module raises.
"""
import ctypes as C
import os
import sys

import numpy as np

ABI_VERSION = 2
MAX_RANKS = 64        # ranks the config struct carries (longer lists: Engine.set_rank_list / apv_set_rank_list)
MAX_N = 64            # largest order of apv_jdiag_batched and of the on-chip per-bin kernels
MAX_STAT_HOPS = 64    # longest statistics window of the subband stream, in hops (apv_stream_set_stat_hops)
MAX_SRCS = 128        # largest n_srcs of a handle (orders 65..128: csrc/kernels_gevd128.hip, float64 arithmetic)

F32, F64 = 0, 1
REG_ABS, REG_REL = 0, 1
NORM2_METHODS = {"auto": 0, "one_wg": 1, "grid": 2}    # APV_NORM2_AUTO / _ONE_WG / _GRID
HANKEL_FORMS = {"auto": 0, "displacement": 1, "dense": 2}    # APV_HANKEL_AUTO / _DISPLACEMENT / _DENSE

OK = 0
ERR_ARG, ERR_HIP, ERR_NOT_PD, ERR_NO_CONVERGE, ERR_RCCL, ERR_STATE = -1, -2, -3, -4, -5, -6

LIB_NAME = "libapvast_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

# every symbol include/apvast_hip.h declares
EXPORTS = (
    "apv_create", "apv_destroy", "apv_last_error", "apv_abi_version",
    "apv_dev_alloc", "apv_dev_free", "apv_memcpy_h2d", "apv_memcpy_d2h", "apv_sync",
    "apv_timer_start", "apv_timer_stop",
    "apv_set_rank_list", "apv_update_dev", "apv_set_update_streams", "apv_update", "apv_corr_dev", "apv_corr_bf16_dev", "apv_to_bf16_dev", "apv_gevd_vast_dev", "apv_jdiag_batched", "apv_jdiag_large", "apv_jdiag_leading", "apv_jdiag_large_c128", "apv_norm2",
    "apv_stft_analysis_dev", "apv_istft_ola_dev", "apv_analysis_dev", "apv_analysis_jobs_dev", "apv_synthesis_dev",
    "apv_stream_set_stat_hops", "apv_stream_set_stat_forgetting", "apv_stream_set_filter_taps", "apv_constrain_filters", "apv_stream_set_synthesis", "apv_fir_synthesis", "apv_stream_set_evaluation", "apv_stream_set_evaluation_spectra", "apv_eval_spectrum_step", "apv_stream_set_evaluation_detectability", "apv_eval_detect_step", "apv_stream_reset_evaluation", "apv_eval_pressure", "apv_eval_energies", "apv_stream_init", "apv_stream_set_perceptual", "apv_process_block", "apv_process_block_f64", "apv_process_signal", "apv_process_signal_f64", "apv_stream_is_f64", "apv_stream_get_statistics", "apv_stream_not_converged", "apv_stream_set_rirs", "apv_set_mu", "apv_set_span", "apv_get_span", "apv_stream_set_effort_limit", "apv_get_effort", "apv_limit_effort", "apv_stream_set_validation_span", "apv_get_validation_span", "apv_validation_span", "apv_state_bytes", "apv_get_state", "apv_set_state",
    "apv_bb_set_rank_list", "apv_bb_init", "apv_bb_set_perceptual", "apv_bb_process_block", "apv_bb_process_signal", "apv_bb_set_rirs", "apv_bb_get_state", "apv_bb_set_state", "apv_bb_set_evaluation", "apv_bb_reset_evaluation", "apv_bb_set_evaluation_spectra", "apv_eval_spectra_hops", "apv_bb_set_evaluation_detectability", "apv_eval_detect_hops",
    "apv_host_alloc", "apv_host_free",
    "apv_predict_pressure", "apv_vast_static", "apv_hankel_statistics",
    "apv_comm_unique_id", "apv_comm_init", "apv_allgather_filters_dev", "apv_comm_count", "apv_comm_last_gather", "apv_comm_barrier",
    "apv_debug_set_stamps", "apv_debug_live_resources", "apv_device_sync", "apv_device_info",
)


class _PinnedBlock:
    """Owner of one apv_host_alloc block; numpy arrays made from it (and their views) keep it alive through .base."""

    def __init__(self, lib, ptr, nbytes):
        self._lib, self._ptr = lib, ptr
        self.__array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        try:
            self._lib.apv_host_free(self._ptr)
        except Exception:           # interpreter shutdown: the library may be gone, and so is the process's memory
            pass


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("n_bins", C.c_int32), ("n_srcs", C.c_int32),
        ("n_mics", C.c_int32), ("n_ranks", C.c_int32), ("ranks", C.c_int32 * MAX_RANKS),
        ("compute_dtype", C.c_int32), ("out_c128", C.c_int32), ("reg_mode", C.c_int32),
        ("reg_dark", C.c_double), ("reg_bright", C.c_double), ("mu", C.c_double),
        ("max_sweeps", C.c_int32), ("block_size", C.c_int32), ("hop_size", C.c_int32), ("n_zones", C.c_int32),
        ("debug_stop", C.c_int32),
        ("dialect", C.c_int32),
        ("frontend", C.c_int32),
        ("out_layout", C.c_int32),
        ("reserved", C.c_int32 * 4),
        ("sweep_tol2", C.c_double),
    ]


SYNTHESIS = {"wola": 0, "fir": 1}     # APV_SYNTH_WOLA, APV_SYNTH_FIR


class ApvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libapvast_hip: {msg} (code {code})")
        self.code = code


class ConvergenceWarning(RuntimeWarning):
    """A hop in which some bin's eigen-iteration stopped at its sweep cap (APV_ERR_NO_CONVERGE).  The C contract
    (include/apvast_hip.h) returns that code AFTER every output has been written and the stream has advanced, so the streaming
    entry points hand the outputs over and warn; ``Engine.stream_not_converged()`` counts such hops.  (The reference's
    schur-based jdiag, apvast.py:30, has no such exit; only a non-positive-definite dark matrix raises there, apvast.py:21-24,
    and here.)"""


_lib = None


def load():
    """dlopen the in-tree HIP library; raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ap_vast_unofficial_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    lib.apv_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.apv_destroy.argtypes = [vp]
    lib.apv_last_error.argtypes = [vp]
    lib.apv_last_error.restype = C.c_char_p
    lib.apv_abi_version.argtypes = []
    lib.apv_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.apv_dev_free.argtypes = [vp, vp]
    lib.apv_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    lib.apv_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    lib.apv_sync.argtypes = [vp]
    lib.apv_timer_start.argtypes = [vp]
    lib.apv_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.apv_update_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.apv_set_update_streams.argtypes = [vp, C.c_int32]
    lib.apv_update.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.apv_corr_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.apv_corr_bf16_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.apv_to_bf16_dev.argtypes = [vp, sz, vp, vp]
    lib.apv_gevd_vast_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.apv_jdiag_batched.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.apv_jdiag_large.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.apv_jdiag_leading.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.apv_jdiag_large_c128.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.apv_norm2.argtypes = [vp, i32, i32, vp, vp, i32]
    lib.apv_stft_analysis_dev.argtypes = [vp, i32, vp, vp]
    lib.apv_istft_ola_dev.argtypes = [vp, i32, vp, vp, vp]
    i64 = C.c_int64
    lib.apv_analysis_dev.argtypes = [vp, i32, i32, vp, i64, i32, i32, i32, vp, i64, i64]
    lib.apv_analysis_jobs_dev.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i64, i64, vp]
    lib.apv_synthesis_dev.argtypes = [vp, i32, i32, vp, i64, i64, vp, vp, i32, i64]
    lib.apv_stream_init.argtypes = [vp, i32, vp, vp, i32, i32, i32]
    lib.apv_stream_set_perceptual.argtypes = [vp, i32, vp, C.c_double, C.c_double, C.c_double, i32]
    lib.apv_process_block.argtypes = [vp, vp, vp, vp]
    lib.apv_process_block_f64.argtypes = [vp, vp, vp, vp]
    lib.apv_process_signal.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.apv_process_signal_f64.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.apv_stream_is_f64.argtypes = [vp]
    lib.apv_stream_get_statistics.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.apv_stream_not_converged.argtypes = [vp]
    lib.apv_stream_set_rirs.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.apv_set_mu.argtypes = [vp, C.c_double]
    lib.apv_set_span.argtypes = [vp, vp, vp, C.c_double]
    lib.apv_get_span.argtypes = [vp, i32, vp, vp]
    lib.apv_stream_set_effort_limit.argtypes = [vp, vp]
    lib.apv_get_effort.argtypes = [vp, i32, vp, vp, vp]
    lib.apv_limit_effort.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.apv_stream_set_validation_span.argtypes = [vp, vp, vp, vp]
    lib.apv_get_validation_span.argtypes = [vp, i32, i32, vp]
    lib.apv_validation_span.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.apv_state_bytes.argtypes = [vp, C.c_char_p, C.POINTER(sz)]
    lib.apv_get_state.argtypes = [vp, C.c_char_p, vp, sz]
    lib.apv_set_state.argtypes = [vp, C.c_char_p, vp, sz]
    lib.apv_bb_init.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32]
    lib.apv_bb_set_rank_list.argtypes = [vp, i32, vp]
    lib.apv_set_rank_list.argtypes = [vp, i32, vp]
    lib.apv_stream_set_stat_hops.argtypes = [vp, i32]
    lib.apv_stream_set_stat_forgetting.argtypes = [vp, C.c_double]
    lib.apv_stream_set_filter_taps.argtypes = [vp, i32]
    lib.apv_constrain_filters.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.apv_stream_set_synthesis.argtypes = [vp, i32]
    lib.apv_fir_synthesis.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.apv_stream_set_evaluation.argtypes = [vp, i32, i32, vp, vp, i32, vp]
    lib.apv_stream_reset_evaluation.argtypes = [vp]
    lib.apv_eval_pressure.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.apv_stream_set_evaluation_spectra.argtypes = [vp, i32]
    lib.apv_eval_spectrum_step.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.apv_stream_set_evaluation_detectability.argtypes = [vp, i32, vp, C.c_double, C.c_double, C.c_double]
    lib.apv_eval_detect_step.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, C.c_double, C.c_double, C.c_double, vp, vp]
    lib.apv_bb_set_perceptual.argtypes = [vp, i32, vp, C.c_double, C.c_double, C.c_double, i32]
    lib.apv_bb_process_block.argtypes = [vp, vp, vp, vp]
    lib.apv_bb_process_signal.argtypes = [vp, i32, vp, vp, vp]
    lib.apv_bb_set_rirs.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.apv_bb_get_state.argtypes = [vp, C.c_char_p, vp, sz]
    lib.apv_host_alloc.argtypes = [C.POINTER(vp), sz]
    lib.apv_host_free.argtypes = [vp]
    lib.apv_bb_set_state.argtypes = [vp, C.c_char_p, vp, sz]
    lib.apv_bb_set_evaluation.argtypes = [vp, i32, i32, vp, vp, i32, vp]
    lib.apv_bb_reset_evaluation.argtypes = [vp]
    lib.apv_eval_energies.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.apv_bb_set_evaluation_spectra.argtypes = [vp, i32]
    lib.apv_eval_spectra_hops.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.apv_bb_set_evaluation_detectability.argtypes = [vp, i32, vp, C.c_double, C.c_double, C.c_double]
    lib.apv_eval_detect_hops.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, C.c_double, C.c_double, C.c_double, vp, vp]
    lib.apv_predict_pressure.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    lib.apv_vast_static.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_double, vp, vp, vp]
    lib.apv_hankel_statistics.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp]
    lib.apv_comm_unique_id.argtypes = [C.c_char_p]
    lib.apv_comm_init.argtypes = [vp, C.c_char_p, i32, i32]
    lib.apv_allgather_filters_dev.argtypes = [vp, vp, vp]
    lib.apv_comm_count.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.apv_comm_last_gather.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(sz)]
    lib.apv_comm_barrier.argtypes = [vp]
    lib.apv_debug_set_stamps.argtypes = [vp, vp]
    lib.apv_debug_live_resources.argtypes = [C.POINTER(i32)]
    lib.apv_device_sync.argtypes = [vp]
    lib.apv_device_info.argtypes = [vp, C.c_char_p, C.POINTER(i32), C.POINTER(i32)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name == "apv_stream_not_converged":
            fn.restype = C.c_long
        elif name != "apv_last_error":
            fn.restype = C.c_int
    if lib.apv_abi_version() != ABI_VERSION:
        raise RuntimeError("libapvast_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def contrast_floor(floor_db):
    """phi = 10^(floor_db / 10) as apv_set_span takes it.  ValueError where it leaves the doubles: phi = 0 means "no floor" there,
    so a floor that underflows would silently remove the part."""
    try:
        phi = 10.0 ** (float(floor_db) / 10.0)
    except OverflowError:
        phi = float("inf")
    if not 0.0 < phi < float("inf"):
        raise ValueError(f"contrast_floor_db = {floor_db}: 10^(dB / 10) must be a positive, finite double")
    return phi


STFT_MAX_JOBS = 8     # channel sets of one analysis launch (APV_STFT_MAX_JOBS)
SPECTRUM_LAYOUTS = ("channel", "bin", "grouped")


def transform_dtypes(dtype):
    """(f64 flag, real dtype, complex dtype) of Engine.analysis / analysis_jobs / synthesize"""
    if dtype in ("f32", F32, np.float32):
        return 0, np.float32, np.complex64
    if dtype in ("f64", F64, np.float64):
        return 1, np.float64, np.complex128
    raise ValueError(f"dtype must be 'f32' or 'f64', not {dtype!r}")


def spectrum_layout(layout, n_ch, K, group=4):
    """Where spectrum element (c, k) of a set of n_ch channels and K bins lies: (stride_c, stride_k, elements of the set,
    (n_ch, K) array of element offsets).  "channel": [C][K]; "bin": [K][C]; "grouped": [ceil(K / g)][C][g], g neighbouring bins of
    a channel contiguous (the last group may be partial: its tail elements belong to no bin)."""
    c, k = np.arange(n_ch)[:, None], np.arange(K)[None, :]
    if layout == "channel":
        return K, 1, n_ch * K, c * K + k
    if layout == "bin":
        return 1, max(n_ch, 1), n_ch * K, k * n_ch + c
    if layout == "grouped":
        g = int(group)
        if g < 2:
            raise ValueError("a grouped layout needs group >= 2")
        return g, max(n_ch, 1), -(-K // g) * n_ch * g, (k // g) * g * n_ch + c * g + k % g
    raise ValueError(f"layout must be one of {SPECTRUM_LAYOUTS}, not {layout!r}")


def check_analysis_args(N, in_len, x_stride, ring_off):
    """The argument rules of apv_analysis_dev (include/apvast_hip.h), raised here as ValueError before anything is uploaded"""
    if not 0 <= in_len <= N:
        raise ValueError(f"in_len = {in_len} must be in 0..block_size = {N}")
    if x_stride < in_len:
        raise ValueError(f"x_stride = {x_stride} must be at least in_len = {in_len}")
    if ring_off % N != 0 and (in_len != N or x_stride < N):
        raise ValueError("a ring offset needs in_len == block_size and x_stride >= block_size")


def check_jobs_args(N, n_jobs, n_hops, ring_off, x_stride, x_hop):
    """The argument rules of apv_analysis_jobs_dev"""
    if not 1 <= n_jobs <= STFT_MAX_JOBS:
        raise ValueError(f"between 1 and {STFT_MAX_JOBS} channel sets per launch, not {n_jobs}")
    if not 0 <= n_hops <= 65535:
        raise ValueError(f"n_hops = {n_hops} must be in 0..65535")
    if n_hops >= 1:
        if ring_off != 0:
            raise ValueError("the chunk form reads linear rows: ring_off must be 0")
        if x_hop < 0 or x_stride < N + (n_hops - 1) * x_hop:
            raise ValueError("x_stride must hold block_size + (n_hops - 1) x_hop samples")


class DeviceBuffer:
    """A hipMalloc'd block owned through the C ABI."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        engine._chk(engine.lib.apv_dev_alloc(engine.h, self.nbytes, C.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        e = self.engine
        e._chk(e.lib.apv_memcpy_h2d(e.h, self.ptr, _ptr(arr), arr.nbytes))
        e.sync()                                   # arr may be a temporary
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        e = self.engine
        e._chk(e.lib.apv_memcpy_d2h(e.h, _ptr(out), self.ptr, out.nbytes))
        e.sync()
        return out

    def free(self):
        if self.ptr is not None and self.engine.h is not None:
            self.engine.lib.apv_dev_free(self.engine.h, self.ptr)
        self.ptr = None


class Engine:
    """One handle = one GPU, one stream, one shard of K bins."""

    def __init__(self, n_bins, n_srcs, n_mics, ranks=(1,), mu=1.0, compute_dtype="f64", out_c128=None,
                 reg_mode=REG_ABS, reg_dark=1e-7, reg_bright=0.0, device=0, max_sweeps=0,
                 block_size=0, hop_size=0, n_zones=1, debug_stop=0, dialect="python", frontend=None, sweep_tol2=0.0,
                 out_layout=0, stat_hops=1, stat_forgetting=None, filter_taps=0, synthesis="wola", evaluation=None,
                 evaluation_spectra=False, span=None, effort_limit=None, evaluation_detectability=None,
                 validation_span=None):
        self.lib = load()
        self.h = None
        ranks = [int(v) for v in ranks]
        if int(n_srcs) > MAX_N:
            # orders 65..128: up to n_srcs ranks, the tail beyond the config struct's MAX_RANKS through apv_set_rank_list
            if not 1 <= len(ranks) <= int(n_srcs):
                raise ValueError(f"between 1 and n_srcs = {int(n_srcs)} ranks per launch")
        elif not 1 <= len(ranks) <= MAX_RANKS:
            raise ValueError(f"between 1 and {MAX_RANKS} ranks per launch")
        cfg = Config()
        cfg.abi_version = ABI_VERSION
        cfg.device = device
        cfg.n_bins, cfg.n_srcs, cfg.n_mics = int(n_bins), int(n_srcs), int(n_mics)
        cfg.n_ranks = min(len(ranks), MAX_RANKS)
        for i, v in enumerate(ranks[:MAX_RANKS]):
            cfg.ranks[i] = v
        self.f64 = compute_dtype in ("f64", F64, np.float64)
        cfg.compute_dtype = F64 if self.f64 else F32
        self.out_c128 = self.f64 if out_c128 is None else bool(out_c128)
        cfg.out_c128 = int(self.out_c128)
        cfg.reg_mode, cfg.reg_dark, cfg.reg_bright, cfg.mu = reg_mode, reg_dark, reg_bright, mu
        cfg.max_sweeps = max_sweeps
        cfg.block_size, cfg.hop_size, cfg.n_zones = block_size, hop_size, n_zones
        cfg.debug_stop = debug_stop           # profiling aid (kernels_gevd16m.hip), 0 in normal use
        cfg.dialect = 1 if dialect == "matlab" else 0
        cfg.sweep_tol2 = float(sweep_tol2)    # Jacobi stop threshold (0 = default)
        # streaming front-end precision: None follows compute_dtype; "f32" / "f64" force it
        cfg.frontend = {None: 0, "f32": 1, "f64": 2}[frontend]
        self.frontend_f64 = self.f64 if frontend is None else frontend == "f64"
        # streaming outputs: 0 = channel-major (n_out, H); 1 = sample-major groups (n_out / L, H, L), see include/apvast_hip.h
        cfg.out_layout = int(out_layout)
        self.out_layout = int(out_layout)
        self.pooled_results = os.environ.get("APV_RESULT_POOL", "1") != "0"
        self._pin_pool = {}
        self.cfg = cfg
        self.K, self.L, self.M, self.nV = cfg.n_bins, cfg.n_srcs, cfg.n_mics, cfg.n_ranks
        h = C.c_void_p()
        rc = self.lib.apv_create(C.byref(cfg), C.byref(h))
        if rc != OK:
            raise ApvError(rc, self.lib.apv_last_error(None).decode())
        self.h = h
        if len(ranks) > MAX_RANKS:
            self.set_rank_list(ranks)
        self.stat_hops = 1
        if int(stat_hops) != 1:
            self.set_stat_hops(stat_hops)
        self.stat_forgetting = None
        if stat_forgetting is not None:
            self.set_stat_forgetting(stat_forgetting)
        self.filter_taps = 0
        if int(filter_taps) != 0:
            self.set_filter_taps(filter_taps)
        self.synthesis = "wola"
        if synthesis != "wola":
            self.set_synthesis(synthesis)
        self.evaluation = None
        if evaluation is not None:
            self.set_evaluation(*evaluation)
        self.evaluation_spectra = False
        if evaluation_spectra:
            self.set_evaluation_spectra(True)
        self.span_parts = None
        if span is not None:
            self.set_span(**span)
        self.effort_limited = False
        if effort_limit is not None:
            self.set_effort_limit(effort_limit)
        self.evaluation_detectability = False
        if evaluation_detectability is not None:
            self.set_evaluation_detectability(evaluation_detectability)
        self.validation_span_on = False
        if validation_span is not None:
            self.set_validation_span(*validation_span)

    def set_evaluation_detectability(self, tables):
        """Perceptual detectability of the evaluated pressures, before stream_init (apv_stream_set_evaluation_detectability); needs
        set_evaluation_spectra.  tables: ap_vast_unofficial_amd.perceptual.PerceptualTables of the block size, or None (off)."""
        if tables is None:
            self._chk(self.lib.apv_stream_set_evaluation_detectability(self.h, 0, None, 0.0, 0.0, 0.0))
            self.evaluation_detectability = False
            return
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        if G2.ndim != 2 or G2.shape[0] != self.K:
            raise ValueError("the tables' G2 must be (n_bins, n_channels)")
        self._chk(self.lib.apv_stream_set_evaluation_detectability(self.h, G2.shape[1], _ptr(G2), float(tables.Cs), float(tables.Ca),
                                                                   float(tables.Leff)))
        self.evaluation_detectability = True

    def eval_detect_step(self, spec, tables, totals, Z, E):
        """One step of the detectability stage alone (apv_eval_detect_step): spec (N/2 + 1, Z (2 E + 1), Mv) complex128, the bin-major
        spectra of the pressure sets (per program: bright of the E ranks, dark of the E ranks, target); tables: PerceptualTables of
        N (or any object with G2 (N/2 + 1, C), Cs, Ca, Leff); totals (Z, 6 E, Mv) float64.  Returns the hop's values (Z, 2 E, Mv)
        -- per program the error of the E ranks, then the leak -- and the new totals."""
        spec = np.ascontiguousarray(spec, dtype=np.complex128)
        totals = np.ascontiguousarray(totals, dtype=np.float64)
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        Z, E = int(Z), int(E)
        if spec.ndim != 3 or G2.ndim != 2:
            raise ValueError("spec must be (N/2 + 1, Z (2 E + 1), Mv) and the tables' G2 (N/2 + 1, C)")
        K, sets, Mv = spec.shape
        if sets != Z * (2 * E + 1) or G2.shape[0] != K or totals.shape != (Z, 6 * E, Mv):
            raise ValueError("spec (N/2 + 1, Z (2 E + 1), Mv), G2 (N/2 + 1, C) and totals (Z, 6 E, Mv) do not agree")
        ds, dt = self.to_device(spec), self.to_device(totals)
        dh = DeviceBuffer(self, 8 * Z * 2 * E * Mv)
        try:
            self._chk(self.lib.apv_eval_detect_step(self.h, ds.ptr, 2 * (K - 1), Z, E, Mv, G2.shape[1], _ptr(G2), float(tables.Cs),
                                                    float(tables.Ca), float(tables.Leff), dh.ptr, dt.ptr))
            return dh.download((Z, 2 * E, Mv), np.float64), dt.download(totals.shape, np.float64)
        finally:
            for b in (ds, dt, dh):
                b.free()

    def set_evaluation_spectra(self, on):
        """Per-bin spectra of the evaluation stage, before stream_init (apv_stream_set_evaluation_spectra); needs set_evaluation."""
        self._chk(self.lib.apv_stream_set_evaluation_spectra(self.h, int(bool(on))))
        self.evaluation_spectra = bool(on)

    def eval_spectrum_step(self, pressure, ring, ring_off, totals, Z, E):
        """One step of the per-bin spectra alone (apv_eval_spectrum_step): pressure (Z (2 E + 1), H, Mv) float64 into ring
        (Z (2 E + 1), Mv, N) as stored -- logical sample n at (n + ring_off) mod N, the hop in the last H logical samples; advance
        ring_off by H mod N before each call -- then |rfft(window * frame)|^2 added to totals (Z, 3 E + 1, N/2 + 1, Mv).  Returns
        the new (ring, totals)."""
        pressure = np.ascontiguousarray(pressure, dtype=np.float64)
        ring = np.ascontiguousarray(ring, dtype=np.float64)
        totals = np.ascontiguousarray(totals, dtype=np.float64)
        Z, E = int(Z), int(E)
        if pressure.ndim != 3 or ring.ndim != 3:
            raise ValueError("pressure must be (Z (2 E + 1), H, Mv) and ring (Z (2 E + 1), Mv, N)")
        sets, H, Mv = pressure.shape
        N = ring.shape[2]
        if sets != Z * (2 * E + 1) or ring.shape != (sets, Mv, N) or totals.shape != (Z, 3 * E + 1, N // 2 + 1, Mv):
            raise ValueError("pressure (Z (2 E + 1), H, Mv), ring (Z (2 E + 1), Mv, N) and totals (Z, 3 E + 1, N/2 + 1, Mv) do not agree")
        dp, dr, dt = self.to_device(pressure), self.to_device(ring), self.to_device(totals)
        try:
            self._chk(self.lib.apv_eval_spectrum_step(self.h, dp.ptr, dr.ptr, int(ring_off), N, H, Z, E, Mv, dt.ptr))
            return dr.download(ring.shape, np.float64), dt.download(totals.shape, np.float64)
        finally:
            for b in (dp, dr, dt):
                b.free()

    def set_evaluation(self, rv_A, rv_B, ranks):
        """Evaluation stage of the subband stream, before stream_init (apv_stream_set_evaluation): rv_A / rv_B (Pv, L, Mv) float64,
        the responses to the validation microphones of zone A / B; ranks: the evaluated ranks, ascending, from the rank list."""
        rv_A = np.ascontiguousarray(rv_A, dtype=np.float64)
        rv_B = np.ascontiguousarray(rv_B, dtype=np.float64)
        if rv_A.ndim != 3 or rv_A.shape != rv_B.shape or rv_A.shape[1] != self.L:
            raise ValueError("rv_A and rv_B must both be (Pv, n_srcs, Mv)")
        r = np.ascontiguousarray(ranks, dtype=np.int32).ravel()
        Pv, _, Mv = rv_A.shape
        self._chk(self.lib.apv_stream_set_evaluation(self.h, Pv, Mv, _ptr(rv_A), _ptr(rv_B), int(r.size), _ptr(r) if r.size else None))
        self.evaluation = (Pv, Mv, [int(v) for v in r])

    def reset_evaluation(self):
        """Totals and output histories of the evaluation stage to zero (apv_stream_reset_evaluation)."""
        self._chk(self.lib.apv_stream_reset_evaluation(self.h))

    def eval_pressure(self, y, rv, H):
        """The pressure kernel alone (apv_eval_pressure): y (G, Pv - 1 + H, L) samples -- per group the Pv - 1 in front of the
        hop, then the hop -- in s_dtype, rv (Pv, L, Mv) float64 -> (G, H, Mv) float64, p[g, n, m] = sum_l sum_j rv[j, l, m]
        y[g, Pv - 1 + n - j, l]."""
        rv = np.ascontiguousarray(rv, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=self.s_dtype)
        if rv.ndim != 3 or y.ndim != 3:
            raise ValueError("y must be (G, Pv - 1 + H, L) and rv (Pv, L, Mv)")
        Pv, L, Mv = rv.shape
        G, H = y.shape[0], int(H)
        if Pv >= 1 and H >= 1 and y.shape[1:] != (Pv - 1 + H, L):
            raise ValueError("y must hold Pv - 1 + H samples of L loudspeakers per group")
        dy, dr = self.alloc(max(y.nbytes, 8)), self.alloc(max(rv.nbytes, 8))
        dp = self.alloc(max(G * H * Mv, 1) * 8)
        try:
            if y.size:
                dy.upload(y)
            if rv.size:
                dr.upload(rv)
            self._chk(self.lib.apv_eval_pressure(self.h, dy.ptr, dr.ptr, G, L, Pv, H, Mv, dp.ptr))
            return dp.download((G, H, Mv), np.float64)
        finally:
            for b in (dy, dr, dp):
                b.free()

    def eval_energies(self, p, H, record=None, totals=None):
        """The energy reduction of the broadband stream's evaluation stage alone (apv_eval_energies): p (Z, 2 E + 1, n H, Mv)
        float64 pressures of n consecutive hops -> (record (n, Z, 3 E + 1, Mv), totals (Z, 3 E + 1, Mv)): per hop [bright of the E
        ranks | dark | error | target], and totals = totals + record[i], i ascending, starting from `totals` (None: zeros).
        `record`: what the record holds before the launch (None: zeros)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.ndim != 4 or p.shape[1] % 2 != 1 or p.shape[1] < 3:
            raise ValueError("p must be (Z, 2 E + 1, n H, Mv)")
        Z, E, Mv, H = p.shape[0], (p.shape[1] - 1) // 2, p.shape[3], int(H)
        if H < 1 or p.shape[2] % H or p.shape[2] < H:
            raise ValueError("p must hold a whole number of hops of H samples")
        n = p.shape[2] // H
        rec = np.zeros((n, Z, 3 * E + 1, Mv)) if record is None else np.ascontiguousarray(record, dtype=np.float64)
        tot = np.zeros((Z, 3 * E + 1, Mv)) if totals is None else np.ascontiguousarray(totals, dtype=np.float64)
        if rec.shape != (n, Z, 3 * E + 1, Mv) or tot.shape != (Z, 3 * E + 1, Mv):
            raise ValueError("record must be (n, Z, 3 E + 1, Mv) and totals (Z, 3 E + 1, Mv)")
        dp, dr, dt = self.to_device(p), self.to_device(rec), self.to_device(tot)
        try:
            self._chk(self.lib.apv_eval_energies(self.h, dp.ptr, Z, E, H, Mv, n, dr.ptr, dt.ptr))
            return dr.download(rec.shape, np.float64), dt.download(tot.shape, np.float64)
        finally:
            for b in (dp, dr, dt):
                b.free()

    def bb_set_evaluation(self, rv_A, rv_B, ranks):
        """Evaluation stage of the broadband stream, after bb_init (apv_bb_set_evaluation): rv_A / rv_B (Pv, L, Mv) float64, the
        responses to the validation microphones of zone A / B; ranks: the evaluated ranks, ascending, among the stream's."""
        rv_A = np.ascontiguousarray(rv_A, dtype=np.float64)
        rv_B = np.ascontiguousarray(rv_B, dtype=np.float64)
        if rv_A.ndim != 3 or rv_A.shape != rv_B.shape or rv_A.shape[1] != self.L:
            raise ValueError("rv_A and rv_B must both be (Pv, n_srcs, Mv)")
        r = np.ascontiguousarray(ranks, dtype=np.int32).ravel()
        Pv, _, Mv = rv_A.shape
        self._chk(self.lib.apv_bb_set_evaluation(self.h, Pv, Mv, _ptr(rv_A), _ptr(rv_B), int(r.size), _ptr(r) if r.size else None))

    def bb_reset_evaluation(self):
        """Totals and output histories of the broadband stream's evaluation stage to zero (apv_bb_reset_evaluation)."""
        self._chk(self.lib.apv_bb_reset_evaluation(self.h))

    def bb_set_evaluation_spectra(self):
        """Per-bin spectra of the broadband stream's evaluation stage, after bb_set_evaluation, once, at any hop boundary
        (apv_bb_set_evaluation_spectra): ring and spectra start from zero here."""
        self._chk(self.lib.apv_bb_set_evaluation_spectra(self.h, 1))

    def bb_set_evaluation_detectability(self, tables):
        """Perceptual detectability of the broadband stream's evaluated pressures, after bb_set_evaluation_spectra, once, at any
        hop boundary (apv_bb_set_evaluation_detectability): the totals start from zero here.  tables:
        ap_vast_unofficial_amd.perceptual.PerceptualTables of the block size."""
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        if G2.ndim != 2 or G2.shape[0] != self.K:
            raise ValueError("the tables' G2 must be (n_bins, n_channels)")
        self._chk(self.lib.apv_bb_set_evaluation_detectability(self.h, G2.shape[1], _ptr(G2), float(tables.Cs), float(tables.Ca),
                                                               float(tables.Leff)))

    def eval_detect_hops(self, spec, tables, Z, E, totals=None, hops_per_launch=None):
        """The three hop-batched launches of the broadband stream's detectability stage alone (apv_eval_detect_hops): spec
        (n, N/2 + 1, Z (2 E + 1), Mv) complex128, the bin-major spectra of n consecutive hops (per program: bright of the E ranks,
        dark of the E ranks, target); tables: PerceptualTables of N (or any object with G2 (N/2 + 1, C), Cs, Ca, Leff); totals
        (Z, 6 E, Mv) float64 (None: zeros); hops_per_launch: at most that many hops per sub-launch (None: all n in one).  Returns
        the hops' values (n, Z, 2 E, Mv) -- per program the error of the E ranks, then the leak -- and the new totals."""
        spec = np.ascontiguousarray(spec, dtype=np.complex128)
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        Z, E = int(Z), int(E)
        if spec.ndim != 4 or G2.ndim != 2 or spec.shape[0] < 1:
            raise ValueError("spec must be (n, N/2 + 1, Z (2 E + 1), Mv) and the tables' G2 (N/2 + 1, C)")
        n, K, sets, Mv = spec.shape
        totals = np.zeros((Z, 6 * E, Mv)) if totals is None else np.ascontiguousarray(totals, dtype=np.float64)
        if sets != Z * (2 * E + 1) or G2.shape[0] != K or totals.shape != (Z, 6 * E, Mv):
            raise ValueError("spec (n, N/2 + 1, Z (2 E + 1), Mv), G2 (N/2 + 1, C) and totals (Z, 6 E, Mv) do not agree")
        per = n if hops_per_launch is None else int(hops_per_launch)
        ds, dt = self.to_device(spec), self.to_device(totals)
        dh = DeviceBuffer(self, 8 * n * Z * 2 * E * Mv)
        try:
            self._chk(self.lib.apv_eval_detect_hops(self.h, ds.ptr, n, per, 2 * (K - 1), Z, E, Mv, G2.shape[1], _ptr(G2),
                                                    float(tables.Cs), float(tables.Ca), float(tables.Leff), dh.ptr, dt.ptr))
            return dh.download((n, Z, 2 * E, Mv), np.float64), dt.download(totals.shape, np.float64)
        finally:
            for b in (ds, dt, dh):
                b.free()

    def eval_spectra_hops(self, p, tail, N, H, totals=None, hops_per_launch=0):
        """The three launches of the broadband stream's per-bin spectra alone (apv_eval_spectra_hops): p (Z, 2 E + 1, n H, Mv)
        float64 pressures of n consecutive hops, tail (Z, 2 E + 1, Mv, N - H) the newest N - H samples in front of them, oldest
        first (None: silence).  Every hop's frame of N samples is windowed and transformed and |P|^2 added to totals
        (Z, 3 E + 1, N/2 + 1, Mv) (None: zeros) in hop order; hops_per_launch = 0: as many hops per sub-launch as the scratch budget
        allows, otherwise at most that many.  Returns (totals, tail), the tail behind the last hop."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        N, H = int(N), int(H)
        if p.ndim != 4 or p.shape[1] % 2 != 1 or p.shape[1] < 3:
            raise ValueError("p must be (Z, 2 E + 1, n H, Mv)")
        Z, E, Mv = p.shape[0], (p.shape[1] - 1) // 2, p.shape[3]
        if H < 1 or H > N or p.shape[2] % H or p.shape[2] < H:
            raise ValueError("p must hold a whole number of hops of H <= N samples")
        n = p.shape[2] // H
        tail = np.zeros((Z, 2 * E + 1, Mv, N - H)) if tail is None else np.ascontiguousarray(tail, dtype=np.float64)
        tot = np.zeros((Z, 3 * E + 1, N // 2 + 1, Mv)) if totals is None else np.ascontiguousarray(totals, dtype=np.float64)
        if tail.shape != (Z, 2 * E + 1, Mv, N - H) or tot.shape != (Z, 3 * E + 1, N // 2 + 1, Mv):
            raise ValueError("tail must be (Z, 2 E + 1, Mv, N - H) and totals (Z, 3 E + 1, N/2 + 1, Mv)")
        dp, dt = self.to_device(p), self.to_device(tot)
        dl = self.to_device(tail) if tail.size else None
        try:
            self._chk(self.lib.apv_eval_spectra_hops(self.h, dp.ptr, dl.ptr if dl else None, N, H, Z, E, Mv, n, int(hops_per_launch),
                                                     dt.ptr))
            return dt.download(tot.shape, np.float64), dl.download(tail.shape, np.float64) if dl else tail
        finally:
            for b in (dp, dt, dl):
                if b is not None:
                    b.free()

    def set_synthesis(self, mode):
        """Synthesis of the subband stream, before stream_init (apv_stream_set_synthesis): "wola" (the reference's overlap-add)
        or "fir" (the constrained stream's taps as zero-latency time-domain FIR filters; needs filter_taps)."""
        if mode not in SYNTHESIS:
            raise ValueError("synthesis must be 'wola' or 'fir'")
        self._chk(self.lib.apv_stream_set_synthesis(self.h, SYNTHESIS[mode]))
        self.synthesis = mode

    def fir_synthesis(self, x, taps_prev, taps_cur, H):
        """The FIR synthesis kernel alone (apv_fir_synthesis): x (J - 1 + H,) samples of one signal -- the J - 1 in front of the
        hop, then the hop -- in s_dtype, taps_prev / taps_cur (nV, J, L) in lam_dtype -> (nV, H, L) of s_dtype: sample t takes
        (1 - a) * (taps_prev applied) + a * (taps_cur applied), a = (t + 1) / H."""
        taps_prev = np.ascontiguousarray(taps_prev, dtype=self.lam_dtype)
        taps_cur = np.ascontiguousarray(taps_cur, dtype=self.lam_dtype)
        if taps_prev.ndim != 3 or taps_prev.shape != taps_cur.shape:
            raise ValueError("taps_prev and taps_cur must both be (nV, J, L)")
        nV, J, L = taps_prev.shape
        H = int(H)
        x = np.ascontiguousarray(x, dtype=self.s_dtype).ravel()
        if J >= 1 and H >= 1 and x.size != J - 1 + H:
            raise ValueError("x must hold J - 1 + H samples")
        isz = np.dtype(self.s_dtype).itemsize
        dx, dp, dc = self.to_device(x) if x.size else self.alloc(isz), self.alloc(max(taps_prev.nbytes, 8)), self.alloc(max(taps_cur.nbytes, 8))
        dout = self.alloc(max(nV * H * L, 1) * isz)
        try:
            if taps_prev.size:
                dp.upload(taps_prev)
                dc.upload(taps_cur)
            self._chk(self.lib.apv_fir_synthesis(self.h, dx.ptr, dp.ptr, dc.ptr, nV, L, J, H, dout.ptr))
            return dout.download((nV, H, L), self.s_dtype)
        finally:
            for b in (dx, dp, dc, dout):
                b.free()

    def set_filter_taps(self, J):
        """Filter-length constraint of the subband stream: J taps (1..block_size; 0 = off), before stream_init
        (apv_stream_set_filter_taps)."""
        self._chk(self.lib.apv_stream_set_filter_taps(self.h, int(J)))
        self.filter_taps = int(J)

    def constrain_filters(self, w, N, J):
        """The projection alone (apv_constrain_filters): w (N/2 + 1, nV, L) complex -> (w', taps), w' = rfft(g, N) with
        g = irfft(w, N) cut to J taps along axis 0, in the handle's filter dtype (w_dtype); taps = g[:J] as (nV, J, L) of lam_dtype."""
        w = np.ascontiguousarray(w, dtype=self.w_dtype)
        if w.ndim != 3 or w.shape[0] != int(N) // 2 + 1:
            raise ValueError("w must be (N / 2 + 1, nV, L)")
        K, nV, L = w.shape
        dw = self.to_device(w)
        dt = self.alloc(nV * int(J) * L * np.dtype(self.lam_dtype).itemsize)
        try:
            self._chk(self.lib.apv_constrain_filters(self.h, dw.ptr, K, nV, L, int(N), int(J), dt.ptr))
            return dw.download((K, nV, L), self.w_dtype), dt.download((nV, int(J), L), self.lam_dtype)
        finally:
            dw.free()
            dt.free()

    def set_stat_hops(self, n_hops):
        """Statistics window of the subband stream, in hops (1..MAX_STAT_HOPS), before stream_init (apv_stream_set_stat_hops)."""
        self._chk(self.lib.apv_stream_set_stat_hops(self.h, int(n_hops)))
        self.stat_hops = int(n_hops)

    def set_stat_forgetting(self, beta):
        """Forgetting factor in (0, 1] of the subband stream's statistics, before stream_init (apv_stream_set_stat_forgetting)."""
        self._chk(self.lib.apv_stream_set_stat_forgetting(self.h, float(beta)))
        self.stat_forgetting = float(beta)

    def set_rank_list(self, ranks):
        """Replace the handle's rank list (ascending, each 1..n_srcs, at most n_srcs of them) before stream_init: the way to
        more than MAX_RANKS ranks at orders above 64 (apv_set_rank_list)."""
        r = np.ascontiguousarray(ranks, dtype=np.int32)
        self._chk(self.lib.apv_set_rank_list(self.h, int(r.size), _ptr(r) if r.size else None))
        self.nV = int(r.size)
        self.cfg.n_ranks = min(self.nV, MAX_RANKS)

    # -- plumbing -----------------------------------------------------------
    def _chk(self, rc):
        if rc == OK:
            return
        msg = self.lib.apv_last_error(self.h).decode()
        if rc in (ERR_NOT_PD, ERR_NO_CONVERGE):
            # apvast.py:21,24 (cholesky); LAPACK's eigensolvers raise the same class when they do not converge
            raise np.linalg.LinAlgError(msg)
        raise ApvError(rc, msg)

    def _chk_stream(self, rc):
        """Status of a streaming entry point: APV_ERR_NO_CONVERGE is a warning (the outputs are complete and the stream state has
        moved on: raising would lose both), everything else as _chk."""
        if rc == ERR_NO_CONVERGE:
            import warnings
            warnings.warn(ConvergenceWarning(self.lib.apv_last_error(self.h).decode()), stacklevel=3)
            return
        self._chk(rc)

    def stream_not_converged(self):
        """Hops so far in which some bin reached the Jacobi sweep cap (subband stream)."""
        return int(self.lib.apv_stream_not_converged(self.h))

    def close(self):
        if self.h is not None:
            self.lib.apv_destroy(self.h)
            self.h = None
        self._pin_pool = {}          # the page-locked blocks go when their last array goes

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.lib.apv_sync(self.h))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    @property
    def w_dtype(self):
        return np.complex128 if self.out_c128 else np.complex64

    @property
    def lam_dtype(self):
        return np.float64 if self.out_c128 else np.float32

    @property
    def c_dtype(self):
        return np.complex128 if self.f64 else np.complex64

    def timer_start(self):
        self._chk(self.lib.apv_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.lib.apv_timer_stop(self.h, C.byref(ms)))
        return ms.value

    # -- hot path -----------------------------------------------------------
    def update(self, XB, XD, d, raise_on_status=True):
        """One block of subband filter updates from host arrays.

        XB, XD: (K, M, L) complex64; d: (K, M) complex64.
        Returns w (K, nV, L), lam (K, L), status (K,).
        """
        K, M, L = self.K, self.M, self.L
        XB = np.ascontiguousarray(XB, dtype=np.complex64)
        XD = np.ascontiguousarray(XD, dtype=np.complex64)
        d = np.ascontiguousarray(d, dtype=np.complex64)
        if XB.shape != (K, M, L) or XD.shape != (K, M, L) or d.shape != (K, M):
            raise ValueError("expected XB, XD of shape (K, M, L) and d of shape (K, M)")
        w = np.empty((K, self.nV, L), dtype=self.w_dtype)
        lam = np.empty((K, L), dtype=self.lam_dtype)
        status = np.empty(K, dtype=np.int32)
        rc = self.lib.apv_update(self.h, _ptr(XB), _ptr(XD), _ptr(d), _ptr(w), _ptr(lam), _ptr(status))
        if rc in (ERR_NOT_PD, ERR_NO_CONVERGE) and not raise_on_status:
            return w, lam, status
        self._chk(rc)
        return w, lam, status

    def set_update_streams(self, n):
        """n = 2: consecutive update_dev launches alternate between two streams of the handle's (the tail of one launch beside the head
        of the next); the library orders them against each other, copies and the all-gather (include/apvast_hip.h)."""
        self._chk(self.lib.apv_set_update_streams(self.h, int(n)))

    def update_dev(self, dXB, dXD, dd, dw, dlam=None, dstatus=None):
        self._chk(self.lib.apv_update_dev(self.h, dXB.ptr, dXD.ptr, dd.ptr, dw.ptr,
                                          dlam.ptr if dlam else None, dstatus.ptr if dstatus else None))

    def corr(self, XB, XD, d):
        """K5' alone: returns R_B, R_D (K, L, L) and r (K, L) in the compute dtype."""
        K, L = self.K, self.L
        bufs = [self.to_device(np.ascontiguousarray(a, dtype=np.complex64)) for a in (XB, XD, d)]
        cs = np.dtype(self.c_dtype).itemsize
        dRB, dRD, dr = self.alloc(K * L * L * cs), self.alloc(K * L * L * cs), self.alloc(K * L * cs)
        self._chk(self.lib.apv_corr_dev(self.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dRB.ptr, dRD.ptr, dr.ptr))
        out = (dRB.download((K, L, L), self.c_dtype), dRD.download((K, L, L), self.c_dtype),
               dr.download((K, L), self.c_dtype))
        for b in bufs + [dRB, dRD, dr]:
            b.free()
        return out

    def corr_bf16(self, XB, XD, d):
        """K5' from bf16-rounded inputs (converted on the device), f32 accumulation: R_B, R_D, r as complex64."""
        K, L, M = self.K, self.L, self.M
        src = [self.to_device(np.ascontiguousarray(a, dtype=np.complex64)) for a in (XB, XD, d)]
        counts = (K * M * L, K * M * L, K * M)
        bf = [self.alloc(c * 4) for c in counts]
        for s_, b_, c_ in zip(src, bf, counts):
            self._chk(self.lib.apv_to_bf16_dev(self.h, c_, s_.ptr, b_.ptr))
        dRB, dRD, dr = self.alloc(K * L * L * 8), self.alloc(K * L * L * 8), self.alloc(K * L * 8)
        self._chk(self.lib.apv_corr_bf16_dev(self.h, bf[0].ptr, bf[1].ptr, bf[2].ptr, dRB.ptr, dRD.ptr, dr.ptr))
        out = (dRB.download((K, L, L), np.complex64), dRD.download((K, L, L), np.complex64),
               dr.download((K, L), np.complex64))
        for b in src + bf + [dRB, dRD, dr]:
            b.free()
        return out

    def gevd_vast(self, RB, RD, r, raise_on_status=True):
        """K6-K10 alone from explicit matrices (compute dtype)."""
        K, L = self.K, self.L
        bufs = [self.to_device(np.ascontiguousarray(a, dtype=self.c_dtype)) for a in (RB, RD, r)]
        dw = self.alloc(K * self.nV * L * np.dtype(self.w_dtype).itemsize)
        dl = self.alloc(K * L * np.dtype(self.lam_dtype).itemsize)
        ds = self.alloc(K * 4)
        self._chk(self.lib.apv_gevd_vast_dev(self.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dw.ptr, dl.ptr, ds.ptr))
        w = dw.download((K, self.nV, L), self.w_dtype)
        lam = dl.download((K, L), self.lam_dtype)
        status = ds.download((K,), np.int32)
        for b in bufs + [dw, dl, ds]:
            b.free()
        if raise_on_status and (status == 1).any():
            raise np.linalg.LinAlgError("Matrix is not positive definite (bin %d)" % int(np.argmax(status == 1)))
        return w, lam, status

    def jdiag_batched(self, A, B):
        """Batched jdiag (apvast.py:20-36) in c128: returns U (batch, n, n), lam (batch, n)."""
        A = np.ascontiguousarray(A, dtype=np.complex128)
        B = np.ascontiguousarray(B, dtype=np.complex128)
        if A.ndim != 3 or A.shape != B.shape or A.shape[1] != A.shape[2]:
            raise ValueError("A, B must be (batch, n, n)")
        batch, n, _ = A.shape
        U = np.empty_like(A)
        lam = np.empty((batch, n))
        status = np.empty(batch, dtype=np.int32)
        self._chk(self.lib.apv_jdiag_batched(self.h, n, batch, _ptr(A), _ptr(B), _ptr(U), _ptr(lam), _ptr(status)))
        return U, lam

    def jdiag_large(self, A, B):
        """Real symmetric pairs of broadband order (n <= 4096): U (batch, n, n), lam (batch, n), float64."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        if A.ndim != 3 or A.shape != B.shape or A.shape[1] != A.shape[2]:
            raise ValueError("A, B must be (batch, n, n)")
        batch, n, _ = A.shape
        U = np.empty_like(A)
        lam = np.empty((batch, n))
        status = np.empty(batch, dtype=np.int32)
        self._chk(self.lib.apv_jdiag_large(self.h, n, batch, _ptr(A), _ptr(B), _ptr(U), _ptr(lam), _ptr(status)))
        return U, lam

    def jdiag_leading(self, A, B, rank):
        """The leading `rank` eigenpairs of real symmetric pairs (what apvast.py:406-414 consumes of jdiag's result):
        U (batch, n, rank), lam (batch, rank), info (batch,) -- 0: subspace iteration, 1: fell back to the complete solve."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        if A.ndim != 3 or A.shape != B.shape or A.shape[1] != A.shape[2]:
            raise ValueError("A, B must be (batch, n, n)")
        batch, n, _ = A.shape
        U = np.empty((batch, n, int(rank)))
        lam = np.empty((batch, int(rank)))
        info = np.empty(batch, dtype=np.int32)
        self._chk(self.lib.apv_jdiag_leading(self.h, n, batch, int(rank), _ptr(A), _ptr(B), _ptr(U), _ptr(lam), _ptr(info)))
        return U, lam, info

    def norm2(self, mats, method="auto"):
        """||M||_2 of symmetric positive semi-definite matrices (count, n, n) float64, n <= 4096, by the Lanczos kernels of the
        relative loading (apVast.m:552-569): (count,) float64.  method: "auto" (what a hop runs), "one_wg" (one workgroup per
        matrix) or "grid" (each step's matrix-vector product over the whole chip)."""
        M = np.ascontiguousarray(mats, dtype=np.float64)
        if M.ndim != 3 or M.shape[1] != M.shape[2]:
            raise ValueError("mats must be (count, n, n)")
        if method not in NORM2_METHODS:
            raise ValueError(f"method must be one of {sorted(NORM2_METHODS)}")
        out = np.empty(M.shape[0])
        self._chk(self.lib.apv_norm2(self.h, M.shape[1], M.shape[0], _ptr(M), _ptr(out), NORM2_METHODS[method]))
        return out

    def jdiag_large_complex(self, A, B):
        """Complex Hermitian pairs of order 65..1024: U (batch, n, n) complex128, lam (batch, n) float64."""
        A = np.ascontiguousarray(A, dtype=np.complex128)
        B = np.ascontiguousarray(B, dtype=np.complex128)
        if A.ndim != 3 or A.shape != B.shape or A.shape[1] != A.shape[2]:
            raise ValueError("A, B must be (batch, n, n)")
        batch, n, _ = A.shape
        U = np.empty_like(A)
        lam = np.empty((batch, n))
        status = np.empty(batch, dtype=np.int32)
        self._chk(self.lib.apv_jdiag_large_c128(self.h, n, batch, _ptr(A), _ptr(B), _ptr(U), _ptr(lam), _ptr(status)))
        return U, lam

    # -- STFT stages ----------------------------------------------------------
    def stft_analysis(self, x):
        """x: (n_ch, N) float32 -> (n_ch, N/2+1) complex64."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n_ch, N = x.shape
        K = N // 2 + 1
        dx = self.to_device(x)
        ds = self.alloc(n_ch * K * 8)
        self._chk(self.lib.apv_stft_analysis_dev(self.h, n_ch, dx.ptr, ds.ptr))
        out = ds.download((n_ch, K), np.complex64)
        dx.free()
        ds.free()
        return out

    def istft_ola(self, spec, overlap):
        """spec: (n_ch, N/2+1) c64, overlap: (n_ch, N) f32 -> (new overlap, out (n_ch, H))."""
        spec = np.ascontiguousarray(spec, dtype=np.complex64)
        overlap = np.ascontiguousarray(overlap, dtype=np.float32)
        n_ch, N = overlap.shape
        H = self.cfg.hop_size
        dsp, dov = self.to_device(spec), self.to_device(overlap)
        dout = self.alloc(n_ch * H * 4)
        self._chk(self.lib.apv_istft_ola_dev(self.h, n_ch, dsp.ptr, dov.ptr, dout.ptr))
        ov = dov.download((n_ch, N), np.float32)
        out = dout.download((n_ch, H), np.float32)
        for b in (dsp, dov, dout):
            b.free()
        return ov, out

    # -- the transforms as the streams launch them ------------------------------
    # (any precision, zero padding, ring offset, strides, channel sets, chunk form: include/apvast_hip.h).  Host arrays in, arrays
    # in natural (channel, bin) / (channel, sample) order out; the device layouts are built and undone here.  Row padding on the
    # device is NaN and spectra / output buffers are pre-filled with `sentinel`, so that a read or a write in the wrong place shows.
    def _rows_to_device(self, x, stride, rdt):
        n_ch, W = x.shape
        rows = np.full((n_ch + 1, stride) if stride else (1, 1), np.nan, dtype=rdt)      # one spare row behind the last
        if stride:
            rows[:n_ch, :W] = x
        return self.to_device(rows)

    def analysis(self, x, dtype="f32", in_len=None, ring_off=0, window=True, x_stride=None, layout="channel"):
        """x: (n_ch, W) rows as stored -> (n_ch, N/2+1) spectra of rfft(w * y), y[n] = row[(n + ring_off) mod N] for n < in_len
        (default W) and 0 up to N; rows lie x_stride (default W) samples apart on the device.  layout: "channel" or "bin"."""
        f64, rdt, cdt = transform_dtypes(dtype)
        x = np.asarray(x, dtype=rdt)
        if x.ndim != 2:
            raise ValueError("x must be (n_ch, samples)")
        N = int(self.cfg.block_size)
        n_ch, W = x.shape
        in_len = W if in_len is None else int(in_len)
        x_stride = W if x_stride is None else int(x_stride)
        if x_stride < W or in_len > W:
            raise ValueError("rows of x must hold in_len samples and fit x_stride")
        if layout not in ("channel", "bin"):
            raise ValueError("layout must be 'channel' or 'bin' (the grouped layout belongs to analysis_jobs)")
        check_analysis_args(N, in_len, x_stride, int(ring_off))
        K = N // 2 + 1
        sc, sk, size, index = spectrum_layout(layout, n_ch, K)
        dx = self._rows_to_device(x, x_stride, rdt)
        ds = self.to_device(np.full(size + 1, np.nan, dtype=cdt))
        try:
            self._chk(self.lib.apv_analysis_dev(self.h, f64, n_ch, dx.ptr, x_stride, in_len, int(ring_off), int(bool(window)),
                                                ds.ptr, sc, sk))
            return ds.download((size + 1,), cdt)[index]
        finally:
            dx.free()
            ds.free()

    def analysis_jobs(self, sets, dtype="f32", ring_off=0, layouts=None, group=4, n_hops=0, x_stride=None, x_hop=None,
                      sentinel=12345.5 + 67.25j, hop_gap=5):
        """Windowed full-length analysis of up to 8 channel sets in one launch.  sets[j]: (n_ch_j, N) rings read at ring_off
        (n_hops = 0), or (n_ch_j, W) linear rows of which hop i takes samples [i x_hop, i x_hop + N) (n_hops >= 1: the chunk form;
        x_hop defaults to the handle's hop size, rows lie x_stride >= W apart).  layouts[j]: "channel", "bin" or "grouped" (groups of
        `group` bins).  Returns (spectra, stray): spectra[j] is (n_ch_j, K), or (n_hops, n_ch_j, K) in the chunk form; stray[j] counts
        the elements of set j's buffer that no (hop, channel, bin) maps to -- the tails of partial groups, hop_gap elements between
        hops and behind the last -- which no longer hold `sentinel`."""
        f64, rdt, cdt = transform_dtypes(dtype)
        N = int(self.cfg.block_size)
        K = N // 2 + 1
        sets = [np.asarray(s, dtype=rdt) for s in sets]
        n_jobs, n_hops, ring_off = len(sets), int(n_hops), int(ring_off)
        layouts = ["channel"] * n_jobs if layouts is None else list(layouts)
        if len(layouts) != n_jobs or any(s.ndim != 2 for s in sets):
            raise ValueError("one layout per set, sets of shape (n_ch, samples)")
        W = sets[0].shape[1] if sets else N
        if any(s.shape[1] != W for s in sets) or (n_hops == 0 and W != N):
            raise ValueError("rows of every set must be equally long (block_size samples for one hop)")
        x_stride = W if x_stride is None else int(x_stride)
        x_hop = int(self.cfg.hop_size) if x_hop is None else int(x_hop)
        if x_stride < W or (n_hops == 0 and x_stride != N):
            raise ValueError("x_stride must hold the rows (one hop: rows lie block_size apart)")
        check_jobs_args(N, n_jobs, n_hops, ring_off, x_stride, x_hop)
        hops = max(n_hops, 1)
        lay = [spectrum_layout(l, s.shape[0], K, group) for l, s in zip(layouts, sets)]
        spec_hop = [size + int(hop_gap) for _, _, size, _ in lay]
        dx = [self._rows_to_device(s, x_stride, rdt) for s in sets]
        ds = [self.to_device(np.full(hops * sh + 1, sentinel, dtype=cdt)) for sh in spec_hop]
        vpa, i64a = C.c_void_p * n_jobs, C.c_int64 * n_jobs
        try:
            self._chk(self.lib.apv_analysis_jobs_dev(
                self.h, f64, n_jobs, vpa(*[b.ptr.value for b in dx]), (C.c_int32 * n_jobs)(*[s.shape[0] for s in sets]),
                vpa(*[b.ptr.value for b in ds]), i64a(*[l[0] for l in lay]), i64a(*[l[1] for l in lay]), ring_off, n_hops,
                x_stride if n_hops else 0, x_hop if n_hops else 0, i64a(*spec_hop)))
            spectra, stray = [], []
            for b, sh, (_, _, size, index) in zip(ds, spec_hop, lay):
                raw = b.download((hops * sh + 1,), cdt)
                at = np.arange(hops)[:, None, None] * sh + index[None]
                spectra.append(raw[at] if n_hops else raw[at[0]])
                free = np.ones(raw.size, dtype=bool)
                free[at.ravel()] = False
                stray.append(int(np.count_nonzero(raw[free] != cdt(sentinel))))
            return spectra, stray
        finally:
            for b in dx + ds:
                b.free()

    def synthesize(self, spec, overlap, dtype="f32", layout="channel", out_group=0, out_gstride=0, emit=True, sentinel=-54321.25):
        """spec (n_ch, N/2+1), overlap (n_ch, N) -> (new overlap (n_ch, N), out (n_ch, H) or None with emit=False, details).
        layout: "channel" or "bin" spectra on the device.  out_group > 0: the hop is emitted sample-major in groups of out_group
        channels, out_gstride elements apart (0: H * out_group) -- channel-major when out_group does not divide n_ch;
        details["emit"] names the form the output was read back in ("grouped" / "channel"), details["stray"] counts the elements
        of the output buffer outside the emitted hop that no longer hold `sentinel`."""
        f64, rdt, cdt = transform_dtypes(dtype)
        N, H = int(self.cfg.block_size), int(self.cfg.hop_size)
        K = N // 2 + 1
        spec = np.asarray(spec, dtype=cdt)
        overlap = np.ascontiguousarray(overlap, dtype=rdt)
        n_ch = overlap.shape[0]
        if spec.shape != (n_ch, K) or overlap.shape != (n_ch, N):
            raise ValueError("spec must be (n_ch, N/2+1) and overlap (n_ch, N)")
        if layout not in ("channel", "bin"):
            raise ValueError("layout must be 'channel' or 'bin'")
        out_group, out_gstride = int(out_group), int(out_gstride)
        if out_group < 0 or (out_gstride != 0 and out_gstride < H * out_group):
            raise ValueError("out_group >= 0, and out_gstride 0 or at least hop_size * out_group")
        sc, sk, size, index = spectrum_layout(layout, n_ch, K)
        raw = np.full(size + 1, np.nan, dtype=cdt)
        raw[index] = spec
        grouped = out_group > 0 and n_ch % out_group == 0
        gs = out_gstride if out_gstride else H * out_group
        c, n = np.arange(n_ch)[:, None], np.arange(H)[None, :]
        at = (c // out_group) * gs + n * out_group + c % out_group if grouped else c * H + n
        n_out = max(int(at.max()) + 1 if at.size else 0, n_ch * H, (n_ch // max(out_group, 1)) * gs) + 1
        bufs = [self.to_device(raw), self.to_device(overlap)]
        if emit:
            bufs.append(self.to_device(np.full(n_out, sentinel, dtype=rdt)))
        try:
            self._chk(self.lib.apv_synthesis_dev(self.h, f64, n_ch, bufs[0].ptr, sc, sk, bufs[1].ptr, bufs[2].ptr if emit else None,
                                                 out_group, out_gstride))
            ov = bufs[1].download((n_ch, N), rdt)
            details = {"emit": "grouped" if grouped else "channel", "stray": 0}
            out = None
            if emit:
                o = bufs[2].download((n_out,), rdt)
                out = o[at]
                free = np.ones(n_out, dtype=bool)
                free[at.ravel()] = False
                details["stray"] = int(np.count_nonzero(o[free] != rdt(sentinel)))
            return ov, out, details
        finally:
            for b in bufs:
                b.free()

    # -- streaming ------------------------------------------------------------
    def stream_init(self, rir_A, rir_B, reference_index_A, reference_index_B, modeling_delay):
        rir_A = np.ascontiguousarray(rir_A, dtype=np.float64)
        rir_B = np.ascontiguousarray(rir_B, dtype=np.float64)
        self._chk(self.lib.apv_stream_init(self.h, rir_A.shape[0], _ptr(rir_A), _ptr(rir_B),
                                           int(reference_index_A), int(reference_index_B), int(modeling_delay)))

    def _set_rirs(self, fn, rir_len, rirs):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in rirs]
        self._chk(fn(self.h, int(rir_len), *[None if a is None else _ptr(a) for a in arrs]))

    def stream_set_rirs(self, rir_len, rir_A=None, rir_B=None, target_rir_A=None, target_rir_B=None):
        """New responses between two hops (None = unchanged): rir_* (rir_len, L, M), target_rir_* (rir_len, M), float64."""
        self._set_rirs(self.lib.apv_stream_set_rirs, rir_len, (rir_A, rir_B, target_rir_A, target_rir_B))

    def set_mu(self, mu):
        """mu of the next hop on (either stream mode)."""
        self._chk(self.lib.apv_set_mu(self.h, float(mu)))

    def set_span(self, mu_profile=None, rank_cap=None, contrast_floor_db=None):
        """The per-bin span (apv_set_span): mu_profile (K,) or (2, K) floats, mu of bin k = mu * profile; rank_cap (K,) or (2, K)
        ints in 1..L; contrast_floor_db a float.  Row 0 of a (2, K) table is zone program A and every kernel-level call (update,
        gevd_vast), row 1 program B.  The first call fixes which parts exist (before stream_init); later calls change their
        values from the next launch or hop on."""
        def table(a, dtype):
            if a is None:
                return None
            a = np.asarray(a, dtype=dtype)
            if a.shape == (self.K,):
                a = np.stack([a, a])
            if a.shape != (2, self.K):
                raise ValueError(f"a span table has shape ({self.K},) or (2, {self.K}), got {a.shape}")
            return np.ascontiguousarray(a)
        m, c = table(mu_profile, np.float64), table(rank_cap, np.int32)
        phi = 0.0 if contrast_floor_db is None else contrast_floor(contrast_floor_db)
        self._chk(self.lib.apv_set_span(self.h, None if m is None else _ptr(m), None if c is None else _ptr(c), phi))
        self.span_parts = (m is not None, c is not None, contrast_floor_db is not None)

    def span(self, zone):
        """Outputs of the span of the last launch or hop for zone program `zone` (apv_get_span): (rank (K,) int32, contrast (K, L)
        float64 or None without a contrast floor)."""
        rank = np.empty(self.K, dtype=np.int32)
        con = np.empty((self.K, self.L), dtype=np.float64) if self.span_parts and self.span_parts[2] else None
        self._chk(self.lib.apv_get_span(self.h, int(zone), _ptr(rank), None if con is None else _ptr(con)))
        return rank, con

    def set_effort_limit(self, limit):
        """The per-bin array-effort limit of the stream's filters (apv_stream_set_effort_limit): linear values > 0, +inf = no limit
        in that bin, as (K,) (both zone programs) or (2, K) (row 0 = program A).  The first call comes before stream_init; later
        calls change the values from the next hop on."""
        a = np.asarray(limit, dtype=np.float64)
        if a.shape == (self.K,):
            a = np.stack([a, a])
        if a.shape != (2, self.K):
            raise ValueError(f"the effort limit has shape ({self.K},) or (2, {self.K}), got {a.shape}")
        a = np.ascontiguousarray(a)
        self._chk(self.lib.apv_stream_set_effort_limit(self.h, _ptr(a)))
        self.effort_limited = True

    def effort(self, zone):
        """Outputs of the effort limit of the last hop for zone program `zone` (apv_get_effort): (effort (K, nV) float64, the
        filters' efforts before the stage; rank (K,) int32, the rank the top slot was taken from; gain (K,) float64 of the top slot)."""
        eff = np.empty((self.K, self.nV), dtype=np.float64)
        rank = np.empty(self.K, dtype=np.int32)
        gain = np.empty(self.K, dtype=np.float64)
        self._chk(self.lib.apv_get_effort(self.h, int(zone), _ptr(eff), _ptr(rank), _ptr(gain)))
        return eff, rank, gain

    def limit_effort(self, w, limit):
        """The stage alone (apv_limit_effort): w (K, nV, L) or (hops, K, nV, L), complex64 or complex128 (anything else is taken as
        complex128), limit (K,) linear -> (w', effort (.., K, nV) float64, src_top (.., K) int32, gain (.., K) float64); src_top is
        the index of the slot the top slot was taken from (its own where it was scaled, -1 where its effort was not finite)."""
        w = np.asarray(w)
        dt = np.complex64 if w.dtype == np.complex64 else np.complex128
        w = np.array(w, dtype=dt, order="C")                 # a copy: the call works in place
        if w.ndim not in (3, 4):
            raise ValueError("w must be (K, nV, L) or (hops, K, nV, L)")
        lead = w.shape[:-2]
        hops = 1 if w.ndim == 3 else w.shape[0]
        K, nV, L = w.shape[-3:]
        lim = np.ascontiguousarray(limit, dtype=np.float64)
        if lim.shape != (K,):
            raise ValueError(f"limit must have shape ({K},), got {lim.shape}")
        eff = np.empty(lead + (nV,), dtype=np.float64)
        src = np.empty(lead, dtype=np.int32)
        gain = np.empty(lead, dtype=np.float64)
        self._chk(self.lib.apv_limit_effort(self.h, int(dt == np.complex128), hops, K, nV, L, _ptr(w), _ptr(lim), _ptr(eff),
                                            _ptr(src), _ptr(gain)))
        return w, eff, src, gain

    def set_validation_span(self, floor, G_A=None, G_B=None):
        """The rank choice by the contrast at the validation microphones (apv_stream_set_validation_span): floor, linear phi >= 0
        (0 = no floor in that bin) as (K,) (both zone programs) or (2, K) (row 0 = program A); G_A, G_B (K, Mv, L) complex128, the
        transfer functions of the validation responses of zone A and zone B at the bin centres.  The first call comes after
        set_evaluation and before stream_init and needs both; later calls without them change the floor from the next hop on."""
        a = np.asarray(floor, dtype=np.float64)
        if a.shape == (self.K,):
            a = np.stack([a, a])
        if a.shape != (2, self.K):
            raise ValueError(f"the validation floor has shape ({self.K},) or (2, {self.K}), got {a.shape}")
        a = np.ascontiguousarray(a)
        g = [None, None]
        for i, G in enumerate((G_A, G_B)):
            if G is None:
                continue
            G = np.ascontiguousarray(G, dtype=np.complex128)
            if G.ndim != 3 or G.shape[0] != self.K or G.shape[2] != self.L or (self.evaluation and G.shape[1] != self.evaluation[1]):
                raise ValueError(f"a validation transfer function has shape ({self.K}, Mv, {self.L}), Mv that of set_evaluation; got {G.shape}")
            g[i] = G
        self._chk(self.lib.apv_stream_set_validation_span(self.h, None if g[0] is None else _ptr(g[0]),
                                                          None if g[1] is None else _ptr(g[1]), _ptr(a)))
        self.validation_span_on = True

    def validation_span(self, zone, what):
        """An output of the validation span of the last hop for zone program `zone` (apv_get_validation_span): what = 0 bright,
        1 dark ((K, nV) float64, before the choice), 2 source ((K, nV) int32, -1: left as it is), 3 rank ((K,) int32)."""
        what = int(what)
        out = np.empty(self.K if what == 3 else (self.K, self.nV), dtype=np.float64 if what < 2 else np.int32)
        self._chk(self.lib.apv_get_validation_span(self.h, int(zone), what, _ptr(out)))
        return out

    def validation_span_kernel(self, w, G_bright, G_dark, phi, timed=False):
        """The stage alone for one program (apv_validation_span): w (K, nV, L) complex64 or complex128 (anything else is taken as
        complex128), G_bright, G_dark (K, Mv, L) complex128, phi (K,) linear -> (w', bright (K, nV), dark (K, nV), src (K, nV)
        int32, rank (K,) int32 = src of the top slot + 1, guard = the guard bytes around the call's device buffers that changed);
        timed=True appends the time of the launch alone (HIP events), in milliseconds."""
        w = np.asarray(w)
        dt = np.complex64 if w.dtype == np.complex64 else np.complex128
        w = np.array(w, dtype=dt, order="C")                 # a copy: the call works in place
        if w.ndim != 3:
            raise ValueError("w must be (K, nV, L)")
        K, nV, L = w.shape
        gb, gd = (np.ascontiguousarray(g, dtype=np.complex128) for g in (G_bright, G_dark))
        if gb.ndim != 3 or gb.shape != gd.shape or gb.shape[0] != K or gb.shape[2] != L:
            raise ValueError(f"G_bright and G_dark must have one shape ({K}, Mv, {L}), got {gb.shape} and {gd.shape}")
        p = np.ascontiguousarray(phi, dtype=np.float64)
        if p.shape != (K,):
            raise ValueError(f"phi must have shape ({K},), got {p.shape}")
        bright, dark = np.empty((K, nV), dtype=np.float64), np.empty((K, nV), dtype=np.float64)
        src, rank = np.empty((K, nV), dtype=np.int32), np.empty(K, dtype=np.int32)
        guard, ms = C.c_int64(-1), C.c_float(-1.0)
        self._chk(self.lib.apv_validation_span(self.h, int(dt == np.complex128), K, nV, L, gb.shape[1], _ptr(w), _ptr(gb), _ptr(gd),
                                               _ptr(p), _ptr(bright), _ptr(dark), _ptr(src), _ptr(rank), C.byref(guard),
                                               C.byref(ms) if timed else None))
        out = (w, bright, dark, src, rank, int(guard.value))
        return out + (float(ms.value),) if timed else out

    def stream_set_perceptual(self, tables, normalisation):
        """tables: ap_vast_unofficial_amd.perceptual.PerceptualTables (or None to switch the weighting off)."""
        if tables is None:
            self._chk(self.lib.apv_stream_set_perceptual(self.h, 0, None, 0.0, 0.0, 0.0, 0))
            return
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        self._chk(self.lib.apv_stream_set_perceptual(self.h, G2.shape[1], _ptr(G2), float(tables.Cs), float(tables.Ca),
                                                     float(tables.Leff), 1 if normalisation == "matlab" else 0))

    def process_block(self, in_A, in_B, n_out):
        """One hop; samples cross the boundary in the front-end's own precision (float64 in, float64 out with the
        float64 front-end)."""
        dt = np.float64 if self.frontend_f64 else np.float32
        in_A = np.ascontiguousarray(in_A, dtype=dt).ravel()
        in_B = np.ascontiguousarray(in_B, dtype=dt).ravel()
        H = self.cfg.hop_size
        out = np.empty((n_out // self.L, H, self.L) if self.out_layout == 1 else (n_out, H), dtype=dt)
        fn = self.lib.apv_process_block_f64 if self.frontend_f64 else self.lib.apv_process_block
        self._chk_stream(fn(self.h, _ptr(in_A), _ptr(in_B), _ptr(out)))
        return out

    def process_signal(self, in_A, in_B, n_out, out=None):
        """Whole signals (a multiple of hop_size samples each) in one call, hops pipelined on the device; returns
        (n_hops, n_out, hop_size) -- with out_layout = 1: (n_out / L, n_hops * hop_size, L).  Sample for sample what n_hops
        calls of process_block return.  `out`: a C-contiguous array of that shape and the front-end's dtype to write into
        (saves the page faults of a fresh one)."""
        dt = np.float64 if self.frontend_f64 else np.float32
        in_A = np.ascontiguousarray(in_A, dtype=dt).ravel()
        in_B = np.ascontiguousarray(in_B, dtype=dt).ravel()
        H = self.cfg.hop_size
        if in_A.size != in_B.size or in_A.size % H:
            raise RuntimeError("invalid input size")
        n_hops = in_A.size // H
        shape = (n_out // self.L, n_hops * H, self.L) if self.out_layout == 1 else (n_hops, n_out, H)
        if out is None:
            out = np.empty(shape, dtype=dt)
        elif out.shape != shape or out.dtype != dt or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of shape %r" % (np.dtype(dt).name, shape))
        fn = self.lib.apv_process_signal_f64 if self.frontend_f64 else self.lib.apv_process_signal
        self._chk_stream(fn(self.h, n_hops, _ptr(in_A), _ptr(in_B), _ptr(out)))
        return out

    def stream_statistics(self, zone, want_U=True):
        """R_B, R_D (K, L, L), r (K, L), U (K, L, L), lam (K, L) of the current hop for zone 0 (A) / 1 (B), float64."""
        K, L = self.K, self.L
        RB, RD = np.empty((K, L, L), np.complex128), np.empty((K, L, L), np.complex128)
        r = np.empty((K, L), np.complex128)
        U = np.empty((K, L, L), np.complex128) if want_U else None
        lam = np.empty((K, L)) if want_U else None
        self._chk(self.lib.apv_stream_get_statistics(self.h, int(zone), _ptr(RB), _ptr(RD), _ptr(r), _ptr(U), _ptr(lam)))
        return RB, RD, r, U, lam

    @property
    def stat_dtype(self):
        """dtype of the statistics window's ring (states "stat_window<z>"): that of the joint diagonalisation's arithmetic."""
        return np.complex128 if (self.f64 or self.L > MAX_N) else np.complex64

    @property
    def s_dtype(self):
        """dtype of the stream's real state arrays."""
        return np.float64 if self.frontend_f64 else np.float32

    @property
    def sc_dtype(self):
        """dtype of the stream's spectra."""
        return np.complex128 if self.frontend_f64 else np.complex64

    def state_bytes(self, name):
        """Size in bytes of a named state array of the subband stream (apv_state_bytes)."""
        n = C.c_size_t()
        self._chk(self.lib.apv_state_bytes(self.h, name.encode(), C.byref(n)))
        return n.value

    def get_state(self, name, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._chk(self.lib.apv_get_state(self.h, name.encode(), _ptr(out), out.nbytes))
        return out

    def set_state(self, name, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.apv_set_state(self.h, name.encode(), _ptr(arr), arr.nbytes))

    # -- broadband streaming ------------------------------------------------------
    def bb_init(self, rir_A, rir_B, reference_index_A, reference_index_B, modeling_delay, filter_length,
                statistics_buffer_length, number_of_eigenvectors):
        rir_A = np.ascontiguousarray(rir_A, dtype=np.float64)
        rir_B = np.ascontiguousarray(rir_B, dtype=np.float64)
        self._chk(self.lib.apv_bb_init(self.h, rir_A.shape[0], _ptr(rir_A), _ptr(rir_B), int(reference_index_A),
                                       int(reference_index_B), int(modeling_delay), int(filter_length),
                                       int(statistics_buffer_length), int(number_of_eigenvectors)))

    def bb_set_rank_list(self, ranks):
        r = np.ascontiguousarray(ranks, dtype=np.int32)
        self._chk(self.lib.apv_bb_set_rank_list(self.h, int(r.size), _ptr(r) if r.size else None))

    def bb_set_perceptual(self, tables, normalisation):
        G2 = np.ascontiguousarray(tables.G2, dtype=np.float64)
        self._chk(self.lib.apv_bb_set_perceptual(self.h, G2.shape[1], _ptr(G2), float(tables.Cs), float(tables.Ca),
                                                 float(tables.Leff), 1 if normalisation == "matlab" else 0))

    def pinned_empty(self, shape, dtype=np.float64):
        """An uninitialised array in page-locked host memory (apv_host_alloc): the library's copies into it are DMA transfers that
        run while the device computes.  Freed when the array and every view of it are gone.  None when the runtime refuses."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        p = C.c_void_p()
        if self.lib.apv_host_alloc(C.byref(p), max(nbytes, 1)) != 0 or not p.value:
            return None
        return np.asarray(_PinnedBlock(self.lib, p.value, nbytes)).view(dtype).reshape(shape)

    def bb_process_block(self, in_A, in_B, n_out):
        """One hop: (n_out, H) float64, or with out_layout = 1 (n_out / L, H, L)."""
        in_A = np.ascontiguousarray(in_A, dtype=np.float64).ravel()
        in_B = np.ascontiguousarray(in_B, dtype=np.float64).ravel()
        H = self.cfg.hop_size
        out = self._result_array((n_out // self.L, H, self.L) if self.out_layout == 1 else (n_out, H))
        self._chk_stream(self.lib.apv_bb_process_block(self.h, _ptr(in_A), _ptr(in_B), _ptr(out)))
        return out

    def _result_array(self, shape):
        """A float64 array for one hop's outputs.  Large hops (the reference's test parameters return 5.2 MB) come from a small pool of
        page-locked blocks, which the device fills by DMA: a block is handed out again once nothing refers to the array made
        from it or to any slice of it; otherwise, and for small hops, an ordinary fresh array."""
        nbytes = int(np.prod(shape)) * 8
        if nbytes < (1 << 20) or not self.pooled_results or not hasattr(sys, "getrefcount"):
            return np.empty(shape, dtype=np.float64)          # (the pool tells an idle block by its reference counts: CPython)
        pool = self._pin_pool.setdefault(tuple(shape), [])
        for ent in pool:
            # [array, references to the array when idle, references to its owner block when idle]
            if sys.getrefcount(ent[0]) == ent[1] and sys.getrefcount(ent[0].base) == ent[2]:
                return ent[0]
        if len(pool) < 4:
            a = self.pinned_empty(shape)
            if a is not None:
                ent = [a, 0, 0]
                pool.append(ent)
                del a
                ent[1], ent[2] = sys.getrefcount(ent[0]), sys.getrefcount(ent[0].base)
                return ent[0]
        return np.empty(shape, dtype=np.float64)

    def bb_signal_shape(self, n_hops, n_out):
        H = self.cfg.hop_size
        return (n_out // self.L, n_hops * H, self.L) if self.out_layout == 1 else (n_hops, n_out, H)

    def bb_process_signal(self, in_A, in_B, n_out, out=None):
        """n_hops hops in one call: (n_hops, n_out, H) float64 -- with out_layout = 1 (n_out / L, n_hops * H, L); the joint
        diagonalisations of up to 16 consecutive hops are one batch.  `out`: a C-contiguous float64 array of that shape to write
        into (one from pinned_empty is filled by DMA; any other through the library's staging buffers)."""
        in_A = np.ascontiguousarray(in_A, dtype=np.float64).ravel()
        in_B = np.ascontiguousarray(in_B, dtype=np.float64).ravel()
        H = self.cfg.hop_size
        if in_A.size != in_B.size or in_A.size % H:
            raise ValueError("inputs must hold a whole number of hops")
        n_hops = in_A.size // H
        shape = self.bb_signal_shape(n_hops, n_out)
        if out is None:
            out = np.empty(shape, dtype=np.float64)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape %r" % (shape,))
        self._chk_stream(self.lib.apv_bb_process_signal(self.h, n_hops, _ptr(in_A), _ptr(in_B), _ptr(out)))
        return out

    def bb_set_rirs(self, rir_len, rir_A=None, rir_B=None, target_rir_A=None, target_rir_B=None):
        """apv_bb_set_rirs: as stream_set_rirs, for the broadband stream."""
        self._set_rirs(self.lib.apv_bb_set_rirs, rir_len, (rir_A, rir_B, target_rir_A, target_rir_B))

    def bb_get_state(self, name, shape):
        out = np.empty(shape, dtype=np.float64)
        self._chk(self.lib.apv_bb_get_state(self.h, name.encode(), _ptr(out), out.size))
        return out

    def bb_set_state(self, name, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self._chk(self.lib.apv_bb_set_state(self.h, name.encode(), _ptr(arr), arr.size))

    # -- evaluation / static solver ------------------------------------------------
    def predict_pressure(self, x, rirs):
        """predictPressure.m: x (T, L), rirs (P, L, M) -> (T, M), float64."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        rirs = np.ascontiguousarray(rirs, dtype=np.float64)
        T, L = x.shape
        P, L2, M = rirs.shape
        if L2 != L:
            raise ValueError("x and rirs disagree on the number of loudspeakers")
        out = np.empty((T, M))
        self._chk(self.lib.apv_predict_pressure(self.h, T, L, M, P, _ptr(x), _ptr(rirs), _ptr(out)))
        return out

    def vast_static(self, gB, gD, filter_length, modeling_delay, reference_index, number_of_eigenvectors, mu):
        """vast.m: gB (Nb, P, L), gD (Nd, P, L) -> w (J*L,), float64; reference_index is 0-based here."""
        gB = np.ascontiguousarray(gB, dtype=np.float64)
        gD = np.ascontiguousarray(gD, dtype=np.float64)
        Nb, P, L = gB.shape
        Nd = gD.shape[0]
        w = np.empty(filter_length * L)
        self._chk(self.lib.apv_vast_static(self.h, Nb, Nd, P, L, int(filter_length), int(modeling_delay),
                                           int(reference_index), int(number_of_eigenvectors), float(mu),
                                           _ptr(gB), _ptr(gD), _ptr(w)))
        return w

    def hankel_statistics(self, stats, tstats=None, *, J, L, M, off=0, skip=1, ncols=None, toff=None, form="auto"):
        """The broadband Hankel statistics alone (apvast.py:329-364, unscaled), as a hop and vast_static launch them.
        stats (njobs, M*L, S) or (M*L, S) float64 rings, row m*L + s, read from ring offset `off`; tstats (M, S) pairs with
        job 0.  skip=1 drops sample J (the python dialect), skip=0 is the contiguous matrix (MATLAB dialect, static solver).
        ncols and toff default to the python dialect's S - J + (0 if skip else 1) and J if skip else J - 1.
        form: "auto" (what a hop runs), "displacement" or "dense".  Returns (R (njobs, n, n), r (n,) or None, form_taken)."""
        st = np.ascontiguousarray(stats, dtype=np.float64)
        if st.ndim == 2:
            st = st[None]
        if st.ndim != 3 or st.shape[1] != M * L:
            raise ValueError("stats must be (njobs, M*L, S)")
        if form not in HANKEL_FORMS:
            raise ValueError(f"form must be one of {sorted(HANKEL_FORMS)}")
        njobs, _, S = st.shape
        skip = 1 if skip else 0
        if ncols is None:
            ncols = S - J + (0 if skip else 1)
        if toff is None:
            toff = J if skip else J - 1
        ts = None
        if tstats is not None:
            ts = np.ascontiguousarray(tstats, dtype=np.float64)
            if ts.shape != (M, S):
                raise ValueError("tstats must be (M, S)")
        n = J * L
        R = np.empty((njobs, n, n))
        r = np.empty(n) if ts is not None else None
        taken = C.c_int32(0)
        self._chk(self.lib.apv_hankel_statistics(self.h, int(J), int(L), int(M), S, int(off), skip, int(ncols), int(toff), njobs,
                                                 _ptr(st), _ptr(ts), HANKEL_FORMS[form], _ptr(R), _ptr(r), C.byref(taken)))
        return R, r, {v: k for k, v in HANKEL_FORMS.items()}[taken.value]

    # -- multi-GPU --------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = load()
        buf = C.create_string_buffer(128)
        rc = lib.apv_comm_unique_id(buf)
        if rc != OK:
            raise ApvError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, uid, rank, world):
        self._chk(self.lib.apv_comm_init(self.h, uid, rank, world))

    def allgather_filters_dev(self, dw_shard, dw_all):
        self._chk(self.lib.apv_allgather_filters_dev(self.h, dw_shard.ptr, dw_all.ptr))

    def comm_count(self):
        """(ranks, this rank) as the RCCL communicator reports them."""
        n, r = C.c_int32(), C.c_int32()
        self._chk(self.lib.apv_comm_count(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_last_gather(self):
        """(device milliseconds, bytes contributed by this rank) of the latest all-gather."""
        ms, nb = C.c_float(), C.c_size_t()
        self._chk(self.lib.apv_comm_last_gather(self.h, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def comm_barrier(self):
        self._chk(self.lib.apv_comm_barrier(self.h))

    def debug_set_stamps(self, dbuf):
        """Diagnostics: register (or, with None, remove) the stage-stamp buffer of the order-16 kernel's diagnostic instantiation."""
        self._chk(self.lib.apv_debug_set_stamps(self.h, dbuf.ptr if dbuf is not None else None))

    @staticmethod
    def debug_live_resources():
        """Diagnostics: (device buffers, pinned blocks, events, streams) the stream states of this process hold now."""
        counts = (C.c_int32 * 4)()
        load().apv_debug_live_resources(counts)
        return tuple(counts)

    def device_sync(self):
        self._chk(self.lib.apv_device_sync(self.h))

    def device_info(self):
        buf = C.create_string_buffer(128)
        cus, mhz = C.c_int32(), C.c_int32()
        self._chk(self.lib.apv_device_info(self.h, buf, C.byref(cus), C.byref(mhz)))
        return {"name": buf.value.decode(), "compute_units": cus.value, "clock_mhz": mhz.value}
