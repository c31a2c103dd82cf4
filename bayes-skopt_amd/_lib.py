"""ctypes binding of libbgp.so (the C-ABI declared in include/bgp.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C bayes-skopt_amd/csrc``.
There is NO CPU fallback: if the shared object is missing, or no gfx950 device is visible when
a context is created, the product path raises.
"""
import atexit
import weakref
import ctypes as C
import os

import numpy as np

# Kernel arguments in device memory instead of host memory (a HIP runtime switch, read when the runtime initialises: it only
# takes effect if nothing in the process has touched the GPU before this import; an explicit setting of the user's wins).  The
# launch schedule is a few dozen dependent launches per factorisation, each of which otherwise starts with a read of its
# arguments across PCIe: measured on MI355X (tools/persist_probe.py, bench.py) 0.666 -> 0.627 ms for 32 matrices of n = 1024,
# 2.22 -> 2.03 ms for one of n = 4096, 15.64 -> 15.47 ms per step at config C, results identical.
# It is a PROCESS-WIDE setting (every HIP user of the process and its children inherit it): BGP_NO_ENV_DEFAULTS=1 leaves the
# environment alone; `env_defaults()` says what this import did, bench.py records it in its line.
_ENV_DEFAULTS = {}
if os.environ.get("BGP_NO_ENV_DEFAULTS", "0") in ("", "0"):
    for _k, _v in (("HIP_FORCE_DEV_KERNARG", "1"),):
        if _k not in os.environ:
            os.environ[_k] = _v
            _ENV_DEFAULTS[_k] = _v


def env_defaults():
    """Environment variables this import set because the user had not (none with BGP_NO_ENV_DEFAULTS=1), and the value of the
    HIP runtime switch the process runs with."""
    return {"set_by_import": dict(_ENV_DEFAULTS), "HIP_FORCE_DEV_KERNARG": os.environ.get("HIP_FORCE_DEV_KERNARG")}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbgp.so")

FORM = {"product": 0, "sum": 1}
STATIONARY = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}


class BgpError(RuntimeError):
    pass


class NotPositiveDefinite(BgpError):
    """bgp_sample_y: predictive covariance (+ jitter) is not numerically positive definite."""


BGP_ERR_NOTPD = 5


class KernelSpecStruct(C.Structure):
    _fields_ = [("form", C.c_int), ("stationary", C.c_int), ("d", C.c_int)]


PLAN_REPORT_COLS = 256  # include/bgp.h BGP_PLAN_REPORT_COLS


class LmlPlanQuery(C.Structure):
    """include/bgp.h bgp_lml_plan_query"""
    _fields_ = [(k, C.c_int) for k in ("nb", "warped", "n", "d", "stationary", "form", "ncu", "timing", "persist", "panel_fused",
                                       "panels", "nstreams", "ps_permitted")]


class LmlPlanReport(C.Structure):
    """include/bgp.h bgp_lml_plan_report"""
    _fields_ = [(k, C.c_int) for k in ("nblk", "ncu", "fits", "path", "share", "gsz", "ngroups", "nb_last", "P", "gen_first",
                                       "gen_last", "gen_groups", "pair", "Bpad", "nchain", "psplit", "dsplit", "ncrit_stream",
                                       "ncrit", "ps_gen", "total", "tile_wgs", "gram_front", "kbuild", "potrf", "trsm", "syrk",
                                       "columns", "fused", "generating", "launch_free")] + \
               [("fused_wgs", C.c_int * PLAN_REPORT_COLS), ("fused_wgs_last", C.c_int * PLAN_REPORT_COLS)]


PLAN_PATHS = ("small", "launch_free", "launches")  # bgp_lml_plan_report.path

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

# name -> (restype, argtypes): every symbol include/bgp.h declares
SIGNATURES = {
    "bgp_device_count": (C.c_int, []),
    "bgp_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "bgp_last_error": (C.c_char_p, []),
    "bgp_version": (C.c_char_p, []),
    "bgp_ctx_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(KernelSpecStruct), C.c_int,
                                 C.POINTER(_vp)]),
    "bgp_ctx_update_data": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "bgp_ctx_destroy": (None, [_vp]),
    "bgp_lml_batch": (C.c_int, [_vp, C.c_int, _dp, _dp, _ip]),
    "bgp_lml_batch_submit": (C.c_int, [_vp, C.c_int, _dp]),
    "bgp_lml_batch_warped_submit": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "bgp_lml_batch_wait": (C.c_int, [_vp, _dp, _ip]),
    "bgp_lml_batch_warped": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _ip]),
    "bgp_ctx_set_warp": (C.c_int, [_vp, _dp]),
    "bgp_beta_cdf": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "bgp_lml_grad_batch": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _ip]),
    "bgp_kernel_matrix": (C.c_int, [_vp, _dp, _dp]),
    "bgp_posterior_batch": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip]),
    "bgp_predict_batch": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "bgp_posterior_batch_warped": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "bgp_predict_batch_warped": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]),
    "bgp_acq_batch": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, C.c_int, _dp]),
    "bgp_acq_values": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, _ip, _dp, C.c_int, _dp]),
    "bgp_predict_mixture": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp,
                                      _ip]),
    "bgp_predict_mixture_warped": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp,
                                             _dp, _ip]),
    "bgp_mixture_values": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp,
                                     _ip]),
    "bgp_mixture_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_pvrs": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, _dp]),
    "bgp_pvrs_prepare": (C.c_int, [_vp, _dp, C.c_int, _ip]),
    "bgp_fantasy_begin": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, C.c_int,
                                    C.c_int]),
    "bgp_fantasy_step": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _ip, _dp]),
    "bgp_fantasy_moments": (C.c_int, [_vp, _dp, _dp]),
    "bgp_fantasy_end": (C.c_int, [_vp]),
    "bgp_fantasy_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_paths_begin": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "bgp_paths_eval": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "bgp_paths_end": (C.c_int, [_vp]),
    "bgp_paths_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_chunk_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_paths_minimize": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _ip, _ip, _ip]),
    "bgp_paths_select": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _ip, C.c_int, _ip, _dp, _dp]),
    "bgp_predict_grad_batch": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "bgp_minimize_starts": (C.c_int, [_vp, C.c_int, _dp, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, C.c_double,
                                      C.c_int, _dp, _dp, _dp, _ip, _ip, _ip]),
    "bgp_partial_dependence": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.c_int, _ip, _dp, C.c_int, _ip, _dp]),
    "bgp_sobol_indices": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.POINTER(C.c_uint), _dp, _dp, _dp, _dp]),
    "bgp_grad_cov": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "bgp_knowledge_gradient": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_double, C.c_int, _dp, _dp]),
    "bgp_joint_entropy": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp]),
    "bgp_cross_validate": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _ip]),
    "bgp_sample_y": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, C.c_double, _dp]),
    "bgp_sample_y_batch": (C.c_int, [_vp, C.c_int, _ip, _dp, C.c_int, _dp, _dp, C.c_double, _dp, _ip]),
    "bgp_lml_batch_gram": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _ip]),
    "bgp_posterior_batch_gram": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "bgp_predict_batch_gram": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bgp_comm_abort": (C.c_int, [_vp]),
    "bgp_mcmc_begin": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _dp]),
    "bgp_mcmc_begin_ex": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _dp]),
    "bgp_mcmc_progress": (C.c_int, [_vp, _ip]),
    "bgp_mcmc_form": (C.c_int, [_vp, _ip]),
    "bgp_comm_init_loopback": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(_vp)]),
    "bgp_comm_bench_lml_gather": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp]),
    "bgp_mcmc_steps": (C.c_int, [_vp, C.c_int, _ip, _ip, _dp, _dp, _dp]),
    "bgp_mcmc_end": (C.c_int, [_vp, _dp, _dp, _dp, _dp, C.POINTER(C.c_longlong), _ip]),
    "bgp_mcmc_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp,
                               _dp, C.POINTER(C.c_longlong), _ip]),
    "bgp_comm_available": (C.c_int, []),
    "bgp_comm_unique_id": (C.c_int, [_vp]),
    "bgp_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "bgp_comm_destroy": (None, [_vp]),
    "bgp_comm_allgather": (C.c_int, [_vp, _dp, C.c_size_t, _dp]),
    "bgp_comm_allreduce_max": (C.c_int, [_vp, _dp, C.c_size_t]),
    "bgp_comm_broadcast": (C.c_int, [_vp, _dp, C.c_size_t, C.c_int]),
    "bgp_comm_barrier": (C.c_int, [_vp]),
    "bgp_comm_nranks": (C.c_int, [_vp, _ip]),
    "bgp_lml_batch_wait_allgather": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _ip]),
    "bgp_device_synchronize": (C.c_int, [C.c_int]),
    "bgp_set_streams": (C.c_int, [_vp, C.c_int]),
    "bgp_last_timing": (C.c_int, [_vp, _dp, _ip]),
    "bgp_set_timing": (C.c_int, [_vp, C.c_int]),
    "bgp_set_persist": (C.c_int, [_vp, C.c_int]),
    "bgp_set_panel_fused": (C.c_int, [_vp, C.c_int]),
    "bgp_panel_fused_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_last_timing_columns": (C.c_int, [_vp, _dp, _ip]),
    "bgp_debug_workspace": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "bgp_debug_cov_factor": (C.c_int, [_vp, _ip, _dp]),
    "bgp_persist_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_lml_gen_stats": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bgp_debug_ps_trace": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "bgp_debug_lml_plan": (C.c_int, [_vp, C.POINTER(LmlPlanQuery), C.POINTER(LmlPlanReport)]),
    "bgp_debug_pivot_root": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp]),
    "bgp_bench_mfma_f64": (C.c_int, [C.c_int, C.c_int, _dp]),
    "bgp_bench_hbm_copy": (C.c_int, [C.c_int, C.c_longlong, C.c_int, _dp]),
    "bgp_mfma_f64_layout": (C.c_int, [C.c_int, _ip, _ip]),
}

_lib = None


def load():
    """Load libbgp.so (once) and declare every prototype.  Raises BgpError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BgpError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C bayes-skopt_amd/csrc`). "
            "There is no CPU fallback."
        )
    # multi-process GPU work on this platform needs dmabuf IPC (RCCL's ncclCommInitRank fails with
    # "hipIpcGetMemHandle: invalid argument" otherwise); the runtime reads the switch when it initialises, i.e. at the
    # first HIP call of the process, so it is set before the library is even loaded
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise BgpError(f"{what} failed (code {rc}): {load().bgp_last_error().decode()}")


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return a.ctypes.data_as(_dp if a.dtype == np.float64 else _ip)


def device_count():
    return int(load().bgp_device_count())


def _lml_plan(handle, query):
    rep = LmlPlanReport()
    _check(load().bgp_debug_lml_plan(handle, C.byref(query), C.byref(rep)), "bgp_debug_lml_plan")
    out = {k: int(getattr(rep, k)) for k, _ in LmlPlanReport._fields_[:-2]}
    out["path"] = PLAN_PATHS[rep.path]
    cols = min(rep.nblk, PLAN_REPORT_COLS)
    out["fused_wgs"], out["fused_wgs_last"] = list(rep.fused_wgs[:cols]), list(rep.fused_wgs_last[:cols])
    return out


def lml_plan(n, nb, ncu, d=4, warped=False, form="product", stationary="matern52", timing=False, persist=-1, panel_fused=-1,
             panels=0, nstreams=0, ps_permitted=True):
    """``bgp_debug_lml_plan`` without a context (no device is touched): what the library would launch for an LML batch of ``nb``
    matrices of ``n`` rows on a device of ``ncu`` CUs under the given modes (``panels`` / ``nstreams`` 0: the defaults) -- the
    planner's fields and launch counts as a dict (include/bgp.h bgp_lml_plan_report; ``path`` by name)."""
    q = LmlPlanQuery(nb=int(nb), warped=int(bool(warped)), n=int(n), d=int(d), stationary=STATIONARY[stationary], form=FORM[form],
                     ncu=int(ncu), timing=int(bool(timing)), persist=int(persist), panel_fused=int(panel_fused), panels=int(panels),
                     nstreams=int(nstreams), ps_permitted=int(bool(ps_permitted)))
    return _lml_plan(None, q)


def device_identity(device=0):
    """PCI bus id of a visible device (``bgp_device_pci_bus_id``): what tells ranks that all see "device 0" apart."""
    buf = C.create_string_buffer(64)
    _check(load().bgp_device_pci_bus_id(int(device), buf, 64), "bgp_device_pci_bus_id")
    return buf.value.decode()


ACQ_EI, ACQ_MEAN, ACQ_LCB, ACQ_STD = 0, 1, 2, 3  # include/bgp.h BGP_ACQ_*
ACQ_MAX = 8
BGP_LIE_VALUE, BGP_LIE_KB = 0, 1  # include/bgp.h BGP_LIE_* (bgp_fantasy_step)
SELECT_KINDS = {"improvement": 0, "thompson": 1}  # include/bgp.h BGP_SELECT_* (bgp_paths_select)
SELECT_MAX_DOUBLES = 1 << 27  # include/bgp.h BGP_SELECT_MAX_DOUBLES: the resident draw matrix, paths x candidates padded to 256
MCMC_FORMS = ("step_lds", "step_hbm", "fused")  # include/bgp.h bgp_mcmc_form


_live_contexts = weakref.WeakSet()


@atexit.register
def _close_live_contexts():
    # contexts still alive when the interpreter goes down are closed while the HIP runtime is still there (the last one
    # takes the library's process-wide streams with it: left alive they crashed a profiler's teardown)
    for ctx in list(_live_contexts):
        try:
            ctx.close()
        except Exception:
            pass


class Context:
    """Owns one device context: training set resident in HBM + the batched-Cholesky workspace."""

    def __init__(self, X, y, alpha_diag, form="product", stationary="matern52", max_batch=64, device=0):
        lib = load()
        X = _c(np.atleast_2d(X))
        n, d = X.shape
        y = _c(y).reshape(n)
        alpha_diag = _c(np.broadcast_to(np.asarray(alpha_diag, dtype=np.float64), (n,)))
        self.n, self.d, self.p = n, d, d + 2
        self.form, self.stationary = form, stationary
        self.max_batch = int(max_batch)
        self.device = int(device)
        spec = KernelSpecStruct(FORM[form], STATIONARY[stationary], d)
        h = _vp()
        if device_count() <= 0:
            raise BgpError("no HIP device visible: the BayesGPR hot path needs an MI355X (no CPU fallback)")
        _check(lib.bgp_ctx_create(self.device, n, d, _p(X), _p(y), _p(alpha_diag), C.byref(spec), self.max_batch,
                                  C.byref(h)), "bgp_ctx_create")
        self._h = h
        self._lib = lib
        _live_contexts.add(self)
        self._pending, self._pending_H = 0, None  # batch handed to lml_submit and not yet collected
        self._timing = False
        self._paths_P = 0           # open pathwise draws (paths_begin .. paths_end / update_data)
        self._fantasy_shape = None  # (B, m, n_acq) of the last fantasy_begin
        self._drop_resident()

    def _drop_resident(self):
        # resident_H: canonical vectors of the posteriors whose K^-1 / alpha are resident on the device; None after a call that
        # overwrites them (gradient / pvrs_prepare / update_data / set_warp / any build: posterior() alone sets it again)
        self.resident_H = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bgp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_data(self, X, y, alpha_diag):
        X = _c(np.atleast_2d(X))
        n, d = X.shape
        if d != self.d:
            raise ValueError("input dimension changed")
        y = _c(y).reshape(n)
        alpha_diag = _c(np.broadcast_to(np.asarray(alpha_diag, dtype=np.float64), (n,)))
        _check(self._lib.bgp_ctx_update_data(self._h, n, _p(X), _p(y), _p(alpha_diag)), "bgp_ctx_update_data")
        self.n = n
        self._drop_resident()
        self._paths_P = 0  # (bgp_ctx_update_data drops the pathwise draws)

    def _H(self, H):
        H = _c(np.atleast_2d(H))
        if H.shape[1] != self.p:
            raise ValueError(f"canonical hyper-parameter vectors must have length d+2={self.p}, got {H.shape[1]}")
        return H

    def lml(self, H, return_status=False):
        H = self._H(H)
        B = H.shape[0]
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        _check(self._lib.bgp_lml_batch(self._h, B, _p(H), _p(out), _p(st)), "bgp_lml_batch")
        return (out, st) if return_status else out

    def lml_submit(self, H):
        """Enqueue ``lml(H)`` on the device and return at once (False when the batch cannot go asynchronously: larger
        than max_batch, or per-launch timing on); ``lml_wait()`` collects the result."""
        H = self._H(H)
        if H.shape[0] > self.max_batch or H.shape[0] == 0 or self._timing:
            return False  # (per-launch timing synchronises inside the call: the caller uses the synchronous form)
        _check(self._lib.bgp_lml_batch_submit(self._h, H.shape[0], _p(H)), "bgp_lml_batch_submit")
        self._pending, self._pending_H = H.shape[0], H  # (H stays alive until the upload has certainly happened)
        return True

    def mcmc_begin(self, coords, logp, nsteps, h_src, h_fixed, prior_kind, prior_par, comm=None, nwarp=0):
        """``bgp_mcmc_begin_ex``: open a device-resident run of the ensemble sampler (``nsteps`` steps of the (W, p) ensemble
        ``coords`` with log-probabilities ``logp``); the plan follows in segments through ``mcmc_steps``, ``mcmc_end`` collects.
        ``comm``: a ``Comm`` whose ranks share every half-step's proposal block (the sharded ensemble; every rank calls with the
        same arguments); ``nwarp`` = 2 d: the walkers' last 2 d entries are their own input-warp parameters."""
        coords = _c(np.asarray(coords, dtype=np.float64))
        W, p = coords.shape
        logp = _c(np.asarray(logp, dtype=np.float64))
        h_src = np.ascontiguousarray(h_src, dtype=np.int32)
        h_fixed = _c(np.asarray(h_fixed, dtype=np.float64))
        prior_kind = np.ascontiguousarray(prior_kind, dtype=np.int32)
        prior_par = _c(np.asarray(prior_par, dtype=np.float64))
        if h_src.shape != (self.d + 2,) or h_fixed.shape != (self.d + 2,) or prior_kind.shape != (p,) or prior_par.shape != (p, 5):
            raise ValueError("canonical map / prior tables have the wrong shape")
        _check(self._lib.bgp_mcmc_begin_ex(self._h, comm._h if comm is not None else None, int(nwarp), W, p, int(nsteps), _p(h_src),
                                           _p(h_fixed), _p(prior_kind), _p(prior_par), _p(coords), _p(logp)), "bgp_mcmc_begin")
        self._mcmc = (W, p, int(nsteps))
        form = C.c_int(-1)
        _check(self._lib.bgp_mcmc_form(self._h, C.byref(form)), "bgp_mcmc_form")
        self.mcmc_form = MCMC_FORMS[form.value]  # (of the run opened last: what the tests read)

    def mcmc_progress(self):
        """Steps of the open run the device has worked through (``bgp_mcmc_progress``; never blocks)."""
        v = C.c_int(0)
        _check(self._lib.bgp_mcmc_progress(self._h, C.byref(v)), "bgp_mcmc_progress")
        return int(v.value)

    def mcmc_steps(self, plan):
        """``bgp_mcmc_steps``: hand over the next segment of the plan -- (movers, partners, zz, factors, logu), each
        (2 * nseg, W / 2) -- and return at once; the device works through it while the caller draws the next segment."""
        W, p, _ = self._mcmc
        movers, partners, zz, factors, logu = plan
        movers = np.ascontiguousarray(movers, dtype=np.int32)
        partners = np.ascontiguousarray(partners, dtype=np.int32)
        zz, factors, logu = (_c(np.asarray(a, dtype=np.float64)) for a in (zz, factors, logu))
        nhalf = movers.shape[0]
        if nhalf % 2 or any(a.shape != (nhalf, W // 2) for a in (movers, partners, zz, factors, logu)):
            raise ValueError("a plan segment must hold (2 * nseg, W / 2) rows of every array")
        try:
            _check(self._lib.bgp_mcmc_steps(self._h, nhalf // 2, _p(movers), _p(partners), _p(zz), _p(factors), _p(logu)), "bgp_mcmc_steps")
        except BaseException:
            self.mcmc_abandon()
            raise

    def mcmc_abandon(self):
        """Drop an open run (an exception between ``mcmc_begin`` and ``mcmc_end``): ``bgp_mcmc_end`` with nothing to
        collect closes it on the C side."""
        if getattr(self, "_mcmc", None) is not None:
            self._mcmc = None
            self._lib.bgp_mcmc_end(self._h, None, None, None, None, None, None)

    def mcmc_end(self):
        """``bgp_mcmc_end``: wait for the run and collect chain (nsteps, W, p), logp (nsteps, W), the final ensemble and its
        log-probabilities, accept counts (W,) and the four info words (non-finite proposal seen; run redone on the launch
        schedule; half-step of the first non-finite proposal; whether it was a NaN)."""
        W, p, nsteps = self._mcmc
        self._mcmc = None
        chain = np.empty((nsteps, W, p))
        lps = np.empty((nsteps, W))
        cout, lout = np.empty((W, p)), np.empty(W)
        nacc = np.zeros(W, dtype=np.int64)
        info = np.zeros(4, dtype=np.int32)
        _check(self._lib.bgp_mcmc_end(self._h, _p(chain), _p(lps), _p(cout), _p(lout), nacc.ctypes.data_as(C.POINTER(C.c_longlong)),
                                      _p(info)), "bgp_mcmc_end")
        return chain, lps, cout, lout, nacc, info

    def mcmc_run(self, coords, logp, plan, h_src, h_fixed, prior_kind, prior_par, comm=None, nwarp=0):
        """``bgp_mcmc_run``: the same run with the whole plan handed over at once."""
        self.mcmc_begin(coords, logp, np.asarray(plan[0]).shape[0] // 2, h_src, h_fixed, prior_kind, prior_par, comm=comm, nwarp=nwarp)
        self.mcmc_steps(plan)
        return self.mcmc_end()

    def _HW(self, H, W):
        """The (B, p) hyper-parameters and their (B, 2d) per-walker warp parameters of a warped LML batch."""
        H = self._H(H)
        W = _c(np.atleast_2d(W))
        B = H.shape[0]
        if W.shape != (B, 2 * self.d):
            raise ValueError(f"warp parameters must be (B, 2d) = ({B}, {2 * self.d}), got {W.shape}")
        return H, W, B

    def lml_warped_submit(self, H, W):
        """Asynchronous ``lml_warped``: False when the batch cannot go asynchronously (see ``lml_submit``)."""
        H, W, B = self._HW(H, W)
        if B > self.max_batch or B == 0 or self._timing:
            return False
        _check(self._lib.bgp_lml_batch_warped_submit(self._h, B, _p(H), _p(W)), "bgp_lml_batch_warped_submit")
        self._pending, self._pending_H = B, (H, W)
        return True

    def lml_wait(self, return_status=False):
        B = self._pending  # (0: the C layer answers BGP_ERR_STATE, "nothing submitted")
        self._pending, self._pending_H = 0, None
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        _check(self._lib.bgp_lml_batch_wait(self._h, _p(out), _p(st)), "bgp_lml_batch_wait")
        return (out, st) if return_status else out

    def lml_warped(self, H, W, return_status=False):
        """Per-walker warp: W is (B, 2d) log-space Beta parameters [wa_1..wa_d, wb_1..wb_d]."""
        H, W, B = self._HW(H, W)
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        _check(self._lib.bgp_lml_batch_warped(self._h, B, _p(H), _p(W), _p(out), _p(st)), "bgp_lml_batch_warped")
        return (out, st) if return_status else out

    def set_warp(self, w):
        """Context-level warp (2d log-space parameters) or None to clear."""
        self._drop_resident()
        if w is None:
            _check(self._lib.bgp_ctx_set_warp(self._h, C.cast(None, _dp)), "bgp_ctx_set_warp")
            return
        w = _c(w).reshape(2 * self.d)
        _check(self._lib.bgp_ctx_set_warp(self._h, _p(w)), "bgp_ctx_set_warp")

    def beta_cdf(self, X, w):
        X = _c(np.atleast_2d(X))
        w = _c(w).reshape(2 * self.d)
        out = np.empty_like(X)
        _check(self._lib.bgp_beta_cdf(self._h, X.shape[0], _p(X), _p(w), _p(out)), "bgp_beta_cdf")
        return out

    def lml_grad(self, H):
        H = self._H(H)
        B = H.shape[0]
        out = np.empty(B)
        grad = np.empty((B, self.p))
        st = np.zeros(B, dtype=np.int32)
        self._drop_resident()
        _check(self._lib.bgp_lml_grad_batch(self._h, B, _p(H), _p(out), _p(grad), _p(st)), "bgp_lml_grad_batch")
        return out, grad, st

    def kernel_matrix(self, h):
        H = self._H(h)
        K = np.empty((self.n, self.n))
        _check(self._lib.bgp_kernel_matrix(self._h, _p(H), _p(K)), "bgp_kernel_matrix")
        return K

    def _posterior(self, name, B, head, want_L, want_alpha, want_K_inv):
        """Outputs and the call of a posterior build ``name(ctx, B, *head, L, alpha, K_inv, lml, status)``, NULL for what is not wanted."""
        n = self.n
        L = np.empty((B, n, n)) if want_L else None
        a = np.empty((B, n)) if want_alpha else None
        Ki = np.empty((B, n, n)) if want_K_inv else None
        lml = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        nul = C.cast(None, _dp)
        self._drop_resident()  # (set by posterior() alone: posteriors of host matrices belong to no canonical vector)
        _check(getattr(self._lib, name)(self._h, B, *head, _p(L) if want_L else nul, _p(a) if want_alpha else nul,
                                        _p(Ki) if want_K_inv else nul, _p(lml), _p(st)), name)
        return {"L": L, "alpha": a, "K_inv": Ki, "lml": lml, "status": st}

    def posterior(self, H, want_L=False, want_alpha=True, want_K_inv=False, warps=None):
        """Batched posterior build; the posteriors stay resident.  ``warps`` (B, 2d): row b is built from the training inputs
        through its OWN warp (``bgp_posterior_batch_warped``); such posteriors are read by ``predict_warped`` alone and
        ``resident_H`` stays None, so the next plain consumer rebuilds."""
        if warps is not None:
            H, W, B = self._HW(H, warps)
            return self._posterior("bgp_posterior_batch_warped", B, (_p(H), _p(W)), want_L, want_alpha, want_K_inv)
        H = self._H(H)
        res = self._posterior("bgp_posterior_batch", H.shape[0], (_p(H),), want_L, want_alpha, want_K_inv)
        if np.all(res["status"] == 0):
            self.resident_H = H.copy()
        return res

    # ---- generic kernel expression trees: host-evaluated kernel matrices in, device arithmetic behind them
    def _Kstack(self, K):
        K = _c(K)
        if K.ndim == 2:
            K = K[None, :, :]
        if K.ndim != 3 or K.shape[1:] != (self.n, self.n):
            raise ValueError(f"kernel matrices must be (B, {self.n}, {self.n}), got {K.shape}")
        return K

    def lml_gram(self, K, use_alpha=True, return_status=False):
        """Log-marginal likelihood of B host-evaluated kernel matrices ``kernel_(X_train)`` (alpha added on the device)."""
        K = self._Kstack(K)
        B = K.shape[0]
        lml = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        _check(self._lib.bgp_lml_batch_gram(self._h, B, _p(K), int(bool(use_alpha)), _p(lml), _p(st)), "bgp_lml_batch_gram")
        return (lml, st) if return_status else lml

    def posterior_gram(self, K, use_alpha=True, want_L=False, want_alpha=True, want_K_inv=False):
        K = self._Kstack(K)
        return self._posterior("bgp_posterior_batch_gram", K.shape[0], (_p(K), int(bool(use_alpha))), want_L, want_alpha, want_K_inv)

    def predict_gram(self, Ks, kss, Kss=None):
        """Predict for the B resident posteriors from host-evaluated ``Ks`` (B, m, n) = kernel_(Xq, X_train),
        ``kss`` (B, m) = kernel_.diag(Xq) and, for the full covariance, ``Kss`` (B, m, m) = kernel_(Xq)."""
        Ks = _c(Ks)
        if Ks.ndim == 2:
            Ks = Ks[None]
        B, m, n = Ks.shape
        if n != self.n:
            raise ValueError(f"Ks must have {self.n} columns, got {n}")
        kss = _c(np.broadcast_to(np.asarray(kss, dtype=np.float64), (B, m)))
        mean = np.empty((B, m))
        var = np.empty((B, m))
        nul = C.cast(None, _dp)
        cov = None
        if Kss is not None:
            Kss = _c(np.broadcast_to(np.asarray(Kss, dtype=np.float64), (B, m, m)))
            cov = np.empty((B, m, m))
        _check(self._lib.bgp_predict_batch_gram(self._h, B, m, _p(Ks), _p(kss), _p(Kss) if Kss is not None else nul,
                                                _p(mean), _p(var), _p(cov) if cov is not None else nul),
               "bgp_predict_batch_gram")
        return (mean, var, cov) if cov is not None else (mean, var)

    def has_pending(self):
        """A batch handed to ``lml_submit`` has not been collected yet."""
        return bool(self._pending)

    def predict(self, H_kernel, Xq, return_cov=False):
        H = self._H(H_kernel)
        B = H.shape[0]
        Xq = _c(np.atleast_2d(Xq))
        m = Xq.shape[0]
        mean = np.empty((B, m))
        var = np.empty((B, m))
        cov = np.empty((B, m, m)) if return_cov else None
        nul = C.cast(None, _dp)
        _check(self._lib.bgp_predict_batch(self._h, B, _p(H), m, _p(Xq), _p(mean), _p(var),
                                           _p(cov) if return_cov else nul), "bgp_predict_batch")
        return (mean, var, cov) if return_cov else (mean, var)

    def predict_warped(self, H_kernel, Xq):
        """(mean, var), each (B, m), of the first B per-row-warped resident posteriors (``posterior(H, warps=W)``): row b sees the
        un-warped ``Xq`` through its own warp."""
        H = self._H(H_kernel)
        B = H.shape[0]
        Xq = _c(np.atleast_2d(Xq))
        m = Xq.shape[0]
        mean = np.empty((B, m))
        var = np.empty((B, m))
        _check(self._lib.bgp_predict_batch_warped(self._h, B, _p(H), m, _p(Xq), _p(mean), _p(var)), "bgp_predict_batch_warped")
        return mean, var

    def acq(self, H_kernel, Xq, y_mean, y_std, kinds, params, n_samples):
        """Closed-form acquisitions (ACQ_EI / ACQ_MEAN / ACQ_LCB / ACQ_STD) of the resident posteriors at Xq, averaged
        over the draws on the device (bgp_acq_batch): (len(kinds), m)."""
        H = self._H(H_kernel)
        Xq = _c(np.atleast_2d(Xq))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = _c(np.asarray(params, dtype=np.float64))
        out = np.empty((len(kinds), Xq.shape[0]))
        _check(self._lib.bgp_acq_batch(self._h, H.shape[0], _p(H), Xq.shape[0], _p(Xq), float(y_mean), float(y_std),
                                       len(kinds), _p(kinds), _p(params), int(n_samples), _p(out)), "bgp_acq_batch")
        return out

    def acq_values(self, mu, std, kinds, params, n_samples):
        """The same closed forms on given (B, m) mean / standard deviation rows (bgp_acq_values)."""
        mu = _c(np.atleast_2d(mu))
        std = _c(np.atleast_2d(std))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = _c(np.asarray(params, dtype=np.float64))
        out = np.empty((len(kinds), mu.shape[1]))
        _check(self._lib.bgp_acq_values(self._h, mu.shape[0], mu.shape[1], _p(mu), _p(std), len(kinds), _p(kinds),
                                        _p(params), int(n_samples), _p(out)), "bgp_acq_values")
        return out

    def _mixture(self, m, B, probs, at, weights, want, call):
        """Arguments and outputs shared by ``predict_mixture`` and ``mixture_values``; ``call(tail)`` issues the C call with the
        common argument tail.  ``want``: which of "moments", "quantiles", "at" to compute (None: whatever the arguments allow)."""
        probs = _c(np.asarray(probs if probs is not None else [], dtype=np.float64).ravel())
        Q = len(probs)
        if want is None:
            want = ("moments",) + (("quantiles",) if Q else ()) + (("at",) if at is not None else ())
        nul = C.cast(None, _dp)
        t = None
        if at is not None:
            t = _c(np.broadcast_to(np.asarray(at, dtype=np.float64), (m,)))
        w = None
        if weights is not None:
            w = _c(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (B,):
                raise ValueError("weights: one per row expected (%d), got %d" % (B, len(w)))
        mom = np.empty((3, m)) if "moments" in want else None
        qu = np.empty((Q, m)) if "quantiles" in want else None
        att = np.empty((3, m)) if "at" in want else None
        nu = np.zeros(1, dtype=np.int32)
        opt = lambda a: _p(a) if a is not None else nul  # noqa: E731
        call((Q, _p(probs) if Q else nul, opt(t), opt(mom), opt(qu), opt(att), _p(nu)), opt(w))
        out = {"n_used": int(nu[0]), "probs": probs}
        if mom is not None:
            out.update(mean=mom[0], within=mom[1], between=mom[2])
        if qu is not None:
            out["quantiles"] = qu
        if att is not None:
            out.update(cdf=att[0], sf=att[1], logpdf=att[2])
        return out

    def predict_mixture(self, H_kernel, Xq, y_mean, y_std, probs, at=None, weights=None, warped=False, want=None):
        """The hyper-posterior mixture ``sum_b w_b N(mu_b, sd_b^2)`` of the first B resident posteriors at Xq, on the device behind
        the batched predict (bgp_predict_mixture; ``warped``: bgp_predict_mixture_warped on per-row-warped posteriors).  A dict in y
        units: ``mean``, ``within``, ``between`` (m,), ``quantiles`` (Q, m) at ``probs``, with ``at`` (a value per point) ``cdf``,
        ``sf``, ``logpdf``, and ``n_used``, the rows that counted (positive weight, finite moments)."""
        H = self._H(H_kernel)
        Xq = _c(np.atleast_2d(Xq))
        B, m = H.shape[0], Xq.shape[0]
        name = "bgp_predict_mixture_warped" if warped else "bgp_predict_mixture"
        fn = getattr(self._lib, name)
        return self._mixture(m, B, probs, at, weights, want, lambda tail, w: _check(
            fn(self._h, B, _p(H), w, m, _p(Xq), float(y_mean), float(y_std), *tail), name))

    def mixture_values(self, mean, var, y_mean, y_std, probs, at=None, weights=None, want=None):
        """The same pass on given normalised (B, m) means / variances (bgp_mixture_values): no resident posterior is read."""
        mean, var = _c(np.atleast_2d(mean)), _c(np.atleast_2d(var))
        if mean.shape != var.shape:
            raise ValueError("mean and var differ in shape")
        B, m = mean.shape
        return self._mixture(m, B, probs, at, weights, want, lambda tail, w: _check(
            self._lib.bgp_mixture_values(self._h, B, m, _p(mean), _p(var), w, float(y_mean), float(y_std), *tail),
            "bgp_mixture_values"))

    def mixture_stats(self):
        """(largest solver iteration count, largest number of bracket moves) of the last mixture call."""
        out = (C.c_longlong * 2)()
        _check(self._lib.bgp_mixture_stats(self._h, out), "bgp_mixture_stats")
        return int(out[0]), int(out[1])

    def pvrs_prepare(self, h_kernel, has_alpha_vec):
        H = self._H(h_kernel)
        st = np.zeros(1, dtype=np.int32)
        self._drop_resident()
        _check(self._lib.bgp_pvrs_prepare(self._h, _p(H), int(bool(has_alpha_vec)), _p(st)), "bgp_pvrs_prepare")
        return int(st[0])

    def pvrs(self, h_kernel, Xcand, Xthompson):
        H = self._H(h_kernel)
        Xc = _c(np.atleast_2d(Xcand))
        Xt = _c(np.atleast_2d(Xthompson))
        covs = np.empty(Xc.shape[0])
        _check(self._lib.bgp_pvrs(self._h, _p(H), Xc.shape[0], _p(Xc), Xt.shape[0], _p(Xt), _p(covs)), "bgp_pvrs")
        return covs

    # ---- batch proposals by fantasy conditioning (bgp_fantasy_*)
    def fantasy_begin(self, H_kernel, noise, Xcand, y_mean, y_std, kinds, params, n_samples, qmax):
        """Start a batch over the resident posteriors (built with the draws' h): H_kernel with the white level at -inf,
        ``noise`` (B,) the variance of a fantasy observation per draw."""
        H = self._H(H_kernel)
        noise = _c(np.asarray(noise, dtype=np.float64).reshape(H.shape[0]))
        Xc = _c(np.atleast_2d(Xcand))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = _c(np.asarray(params, dtype=np.float64))
        self._fantasy_shape = (H.shape[0], Xc.shape[0], len(kinds))
        _check(self._lib.bgp_fantasy_begin(self._h, H.shape[0], _p(H), _p(noise), Xc.shape[0], _p(Xc), float(y_mean),
                                           float(y_std), len(kinds), _p(kinds), _p(params), int(n_samples), int(qmax)),
               "bgp_fantasy_begin")

    def fantasy_step(self, p, lie, want_values=False):
        """Condition on candidate ``p`` with ``lie`` (a normalised value, or None for the kriging believer); returns
        (next index, averaged values (n_acq, m) or None)."""
        _B, m, n_acq = self._fantasy_shape
        nxt = np.zeros(1, dtype=np.int32)
        vals = np.empty((n_acq, m)) if want_values else None
        kind = BGP_LIE_KB if lie is None else BGP_LIE_VALUE
        _check(self._lib.bgp_fantasy_step(self._h, int(p), kind, 0.0 if lie is None else float(lie), _p(nxt),
                                          _p(vals) if want_values else C.cast(None, _dp)), "bgp_fantasy_step")
        return int(nxt[0]), vals

    def fantasy_moments(self):
        B, m, _ = self._fantasy_shape
        mean, var = np.empty((B, m)), np.empty((B, m))
        _check(self._lib.bgp_fantasy_moments(self._h, _p(mean), _p(var)), "bgp_fantasy_moments")
        return mean, var

    def fantasy_end(self):
        _check(self._lib.bgp_fantasy_end(self._h), "bgp_fantasy_end")

    def fantasy_stats(self):
        out = (C.c_longlong * 2)()
        _check(self._lib.bgp_fantasy_stats(self._h, out), "bgp_fantasy_stats")
        return {"begins": int(out[0]), "steps": int(out[1])}

    # ---- prediction gradients and the device-resident optimum search (bgp_predgrad.hip)
    def predict_grad(self, H_kernel, Xq, want_dvar=True):
        """(mean (B, m), var (B, m), dmean (B, m, d), dvar (B, m, d) | None) of the resident posteriors at the rows of ``Xq``
        (``bgp_predict_grad_batch``; normalised-target units).  Needs d <= 32 and no context-level warp."""
        H = self._H(H_kernel)
        B = H.shape[0]
        Xq = _c(np.atleast_2d(Xq))
        if Xq.shape[1] != self.d:
            raise ValueError(f"query points must have {self.d} columns, got {Xq.shape[1]}")
        m = Xq.shape[0]
        mean, var = np.empty((B, m)), np.empty((B, m))
        dmean = np.empty((B, m, self.d))
        dvar = np.empty((B, m, self.d)) if want_dvar else None
        _check(self._lib.bgp_predict_grad_batch(self._h, B, _p(H), m, _p(Xq), _p(mean), _p(var), _p(dmean),
                                                _p(dvar) if want_dvar else C.cast(None, _dp)), "bgp_predict_grad_batch")
        return mean, var, dmean, dvar

    def minimize_starts(self, b, H_kernel, y_mean, y_std, kappa, X0, lo, hi, gtol=1e-5, max_iter=200):
        """``bgp_minimize_starts``: minimise ``y_mean + y_std mean(x) + kappa y_std sqrt(var(x))`` of resident posterior ``b``
        (``H_kernel``: its d + 2 kernel parameters, or the block of all resident posteriors) over the box [lo, hi] from every row
        of ``X0``, in one launch.  Returns a dict: x (S, d), mean, var (S,; normalised units, the bits of ``predict_grad`` at x),
        iters, evals, status (S,; 0 converged to ``gtol``, 1 ``max_iter`` reached, 2 no decrease found or a non-finite objective / gradient)."""
        H = self._H(H_kernel)
        h = _c(H[int(b)] if H.shape[0] > 1 else H[0])
        X0 = _c(np.atleast_2d(X0))
        S, d = X0.shape
        lo = _c(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.d,)))
        hi = _c(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.d,)))
        if d != self.d:
            raise ValueError(f"start points must have {self.d} columns, got {d}")
        x = np.empty((S, d))
        mean, var = np.empty(S), np.empty(S)
        iters, evals, status = (np.zeros(S, dtype=np.int32) for _ in range(3))
        _check(self._lib.bgp_minimize_starts(self._h, int(b), _p(h), float(y_mean), float(y_std), float(kappa), S, _p(X0), _p(lo),
                                             _p(hi), float(gtol), int(max_iter), _p(x), _p(mean), _p(var), _p(iters), _p(evals),
                                             _p(status)), "bgp_minimize_starts")
        return {"x": x, "mean": mean, "var": var, "iters": iters, "evals": evals, "status": status}

    # ---- partial dependence of the surrogate mean (bgp_pdep.hip)
    def partial_dependence(self, H_kernel, Xs, grids, panels):
        """``bgp_partial_dependence``: the mean of the resident posteriors 0 .. B-1 (``H_kernel`` (B, d + 2)) averaged over the sample
        rows ``Xs`` (S, d) with the panel's coordinates replaced by grid values.  ``grids``: d 1-D arrays (1 .. 256 values each);
        ``panels``: ``(k1, -1)`` / ``(k1,)`` / ``k1`` for a curve, ``(k1, k2)`` for a map.  Returns one array per panel, (B, G1) or
        (B, G1, G2), in normalised-target units.  Needs d <= 32."""
        H = self._H(H_kernel)
        B = H.shape[0]
        Xs = _c(np.atleast_2d(Xs))
        if Xs.shape[1] != self.d:
            raise ValueError(f"sample rows must have {self.d} columns, got {Xs.shape[1]}")
        grids = [_c(np.asarray(g, dtype=np.float64).reshape(-1)) for g in grids]
        if len(grids) != self.d:
            raise ValueError(f"one grid per dimension: {self.d} expected, got {len(grids)}")
        ng = np.array([len(g) for g in grids], dtype=np.int32)
        gmax = max(int(ng.max()), 1)
        grid = np.empty((gmax, self.d))
        for k, g in enumerate(grids):  # (rows past a dimension's grid are not read: its last value, so that a warp sees a number)
            grid[:len(g), k] = g
            grid[len(g):, k] = g[-1] if len(g) else 0.5
        pan = np.empty((len(panels), 2), dtype=np.int32)
        for i, pnl in enumerate(panels):
            pnl = tuple(np.atleast_1d(pnl).astype(int))
            pan[i] = (pnl[0], pnl[1] if len(pnl) > 1 else -1)
        shapes = [(int(ng[a]),) if b < 0 else (int(ng[a]), int(ng[b])) for a, b in pan
                  if 0 <= a < self.d and -1 <= b < self.d] if len(pan) else []
        total = int(sum(int(np.prod(s)) for s in shapes))
        out = np.empty((B, max(total, 1)))
        _check(self._lib.bgp_partial_dependence(self._h, B, _p(H), Xs.shape[0], _p(Xs), gmax, _p(ng), _p(grid), len(pan), _p(pan),
                                                _p(out)), "bgp_partial_dependence")
        res, o = [], 0
        for s in shapes:
            sz = int(np.prod(s))
            res.append(out[:, o:o + sz].reshape((B,) + s).copy())
            o += sz
        return res

    # ---- Sobol' sensitivity of the surrogate mean (bgp_sobol.hip)
    def sobol_indices(self, H_kernel, A, Bm, masks):
        """``bgp_sobol_indices``: the pick-freeze sums of the mean of the resident posteriors 0 .. B-1 (``H_kernel`` (B, d + 2)) over
        the sample matrices ``A``, ``Bm`` (N, d) for the terms ``masks`` (T,; bit k set: dimension k is taken from ``Bm``).  Returns
        ``(f0 (B,), V (B,), closed (B, T), total (B, T))`` in normalised-target units: the mean and the variance of the surrogate
        over the 2N rows, the closed (Saltelli 2010) and the total (Jansen 1999) effect of every term, not yet divided by V.
        Needs d <= 32."""
        H = self._H(H_kernel)
        B = H.shape[0]
        A, Bm = _c(np.atleast_2d(A)), _c(np.atleast_2d(Bm))
        if A.shape[1] != self.d or Bm.shape != A.shape:
            raise ValueError(f"A and Bm must both be (N, {self.d}), got {A.shape} and {Bm.shape}")
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1), dtype=np.uint32)
        T = len(masks)
        if T == 0:
            masks = np.zeros(1, dtype=np.uint32)  # (a pointer to hand over; the C layer names the fault)
        f0, V = np.empty(B), np.empty(B)
        closed, total = np.empty((B, T)), np.empty((B, T))
        up = C.POINTER(C.c_uint)
        _check(self._lib.bgp_sobol_indices(self._h, B, _p(H), A.shape[0], _p(A), _p(Bm), T, masks.ctypes.data_as(up), _p(f0), _p(V),
                                           _p(closed), _p(total)), "bgp_sobol_indices")
        return f0, V, closed, total

    # ---- posterior covariance of the gradient and the active-subspace sums (bgp_gcov.hip)
    def grad_cov(self, H_kernel, Xq, want_dmean=True, want_cov=True, want_csum=False):
        """``bgp_grad_cov``: for the resident posteriors 0 .. B-1 (``H_kernel`` (B, d + 2)) at the rows of ``Xq`` (m, d) the gradient of
        the mean ``dmean`` (B, m, d), the posterior covariance of the latent function's gradient ``cov`` (B, m, d, d; exactly
        symmetric, diagonal clipped at 0) and ``csum`` (B, 2, d, d): the averages over the rows of ``dmean dmean^T`` and of ``cov``
        (C_mean, C_cov of the active-subspace matrix).  Normalised-target units; an output that is not wanted is None and is
        neither downloaded nor, where nothing needs it, computed.  Needs d <= 32, m d <= 2^24, a differentiable family (not
        Matern 1/2) and no context-level warp."""
        H = self._H(H_kernel)
        B = H.shape[0]
        Xq = _c(np.atleast_2d(Xq))
        if Xq.shape[1] != self.d:
            raise ValueError(f"query points must have {self.d} columns, got {Xq.shape[1]}")
        m, d = Xq.shape[0], self.d
        dmean = np.empty((B, m, d)) if want_dmean else None
        cov = np.empty((B, m, d, d)) if want_cov else None
        csum = np.empty((B, 2, d, d)) if want_csum else None
        null = C.cast(None, _dp)
        _check(self._lib.bgp_grad_cov(self._h, B, _p(H), m, _p(Xq), _p(dmean) if want_dmean else null,
                                      _p(cov) if want_cov else null, _p(csum) if want_csum else null), "bgp_grad_cov")
        return dmean, cov, csum

    # ---- knowledge-gradient acquisition (bgp_kg.hip)
    def knowledge_gradient(self, H_kernel, noise, Xcand, Xref, y_std, n_samples, want_rows=True):
        """``bgp_knowledge_gradient``: for the resident posteriors 0 .. B-1 (``H_kernel`` (B, d + 2), white level at -inf) the expected
        decrease of the minimum of the posterior mean over ``Xref`` (M, d; 0 <= M <= 255) and the candidate itself after one
        observation with variance ``var(x) + noise[b]`` at each row of ``Xcand`` (m, d).  Returns ``(kg (B, m) | None, avg (m,))``
        in y units (``y_std`` times the normalised value); ``avg`` adds the rows in order, each divided by ``n_samples``.  Needs
        d <= 32 and no context-level warp."""
        H = self._H(H_kernel)
        B = H.shape[0]
        noise = _c(np.asarray(noise, dtype=np.float64).reshape(B))
        Xc = _c(np.atleast_2d(Xcand))
        Xr = _c(np.asarray(Xref, dtype=np.float64).reshape(-1, self.d))
        if Xc.shape[1] != self.d:
            raise ValueError(f"candidates must have {self.d} columns, got {Xc.shape[1]}")
        m, M = Xc.shape[0], Xr.shape[0]
        kg = np.empty((B, m)) if want_rows else None
        avg = np.empty(m)
        null = C.cast(None, _dp)
        _check(self._lib.bgp_knowledge_gradient(self._h, B, _p(H), _p(noise), m, _p(Xc), M, _p(Xr) if M else null, float(y_std),
                                                int(n_samples), _p(kg) if want_rows else null, _p(avg)), "bgp_knowledge_gradient")
        return kg, avg

    # ---- joint entropy search acquisition (bgp_jes.hip)
    def joint_entropy(self, H_kernel, noise, Xcand, Xopt, fopt, tau, n_samples, want_rows=True):
        """``bgp_joint_entropy``: for the resident posteriors 0 .. B-1 (``H_kernel`` (B, d + 2), white level at -inf) the moment-matched
        drop of the entropy of an observation (variance ``var(x) + noise[b]``) at each row of ``Xcand`` (m, d) once the optimum is
        known, averaged over posterior b's OWN optimum samples ``Xopt`` (B, R, d) / ``fopt`` (B, R), 1 <= R <= 255; ``tau`` >= 0 is
        the jitter on the noiseless optimum observation.  Returns ``(gain (B, m) | None, avg (m,))`` in nats; ``avg`` adds the rows
        in order, each divided by ``n_samples``.  Needs d <= 32 and no context-level warp."""
        H = self._H(H_kernel)
        B = H.shape[0]
        noise = _c(np.asarray(noise, dtype=np.float64).reshape(B))
        Xc = _c(np.atleast_2d(Xcand))
        if Xc.shape[1] != self.d:
            raise ValueError(f"candidates must have {self.d} columns, got {Xc.shape[1]}")
        fo = _c(np.asarray(fopt, dtype=np.float64).reshape(B, -1))
        R = fo.shape[1]
        Xo = np.asarray(Xopt, dtype=np.float64)
        if Xo.size != B * R * self.d:
            raise ValueError(f"optimum points must be ({B}, {R}, {self.d}), got {Xo.shape}")
        Xo = _c(Xo.reshape(B, R, self.d))
        m = Xc.shape[0]
        gain = np.empty((B, m)) if want_rows else None
        avg = np.empty(m)
        null = C.cast(None, _dp)
        _check(self._lib.bgp_joint_entropy(self._h, B, _p(H), _p(noise), m, _p(Xc), R, _p(Xo), _p(fo), float(tau), int(n_samples),
                                           _p(gain) if want_rows else null, _p(avg)), "bgp_joint_entropy")
        return gain, avg

    # ---- cross-validation from the resident inverses (bgp_cv.hip)
    def cross_validate(self, B, folds):
        """``bgp_cross_validate``: the predictive of the held-out observations of every fold (``folds``: index arrays, disjoint,
        1 .. 128 points each) under the first ``B`` resident posteriors, without a refit.  Returns ``(mean (B, n), var (B, n),
        fold_lpd (B, K), status (B, K))`` in normalised-target units; mean / var are NaN at points no fold covers, and
        ``status != 0`` marks a (posterior, fold) whose block of the inverse is not positive definite (its outputs are NaN)."""
        folds = [np.ascontiguousarray(np.asarray(f).reshape(-1), dtype=np.int32) for f in folds]
        K = len(folds)
        ptr = np.zeros(K + 1, dtype=np.int32)
        if K:
            ptr[1:] = np.cumsum([len(f) for f in folds])
        idx = np.ascontiguousarray(np.concatenate(folds) if K else np.zeros(0), dtype=np.int32)
        if len(idx) == 0:
            idx = np.zeros(1, dtype=np.int32)  # (a pointer to hand over; the C layer names the fault)
        B = int(B)
        mean, var = np.empty((max(B, 0), self.n)), np.empty((max(B, 0), self.n))
        lpd = np.empty((max(B, 0), K))
        st = np.zeros((max(B, 0), K), dtype=np.int32)
        _check(self._lib.bgp_cross_validate(self._h, B, K, _p(ptr), _p(idx), _p(mean), _p(var), _p(lpd), _p(st)),
               "bgp_cross_validate")
        return mean, var, lpd, st

    # ---- pathwise posterior function draws (bgp_paths_*)
    def paths_begin(self, pidx, H_kernel, log_s2, omega, phase, w, eps):
        """``bgp_paths_begin``: P paths over the resident posteriors ``pidx`` (P,) with kernel parameters ``H_kernel`` (P, d + 2;
        white level -inf), the posteriors' log white levels ``log_s2`` (P,) and the host-drawn ``omega`` (P, F, d), ``phase``
        (P, F), ``w`` (P, F + 1), ``eps`` (P, n)."""
        H = self._H(H_kernel)
        P = H.shape[0]
        omega = _c(omega)
        if omega.ndim != 3 or omega.shape[0] != P or omega.shape[2] != self.d:
            raise ValueError(f"omega must be (P, F, d) = ({P}, F, {self.d}), got {omega.shape}")
        F = omega.shape[1]
        pidx = np.ascontiguousarray(pidx, dtype=np.int32)
        log_s2, phase, w, eps = _c(log_s2), _c(phase), _c(w), _c(eps)
        if pidx.shape != (P,) or log_s2.shape != (P,) or phase.shape != (P, F) or w.shape != (P, F + 1) or eps.shape != (P, self.n):
            raise ValueError("pidx / log_s2 must be (P,), phase (P, F), w (P, F + 1) and eps (P, n)")
        _check(self._lib.bgp_paths_begin(self._h, P, _p(pidx), _p(H), _p(log_s2), F, _p(omega), _p(phase), _p(w), _p(eps)),
               "bgp_paths_begin")
        self._paths_P = P

    def paths_eval(self, Xq, want_grad=False):
        """``bgp_paths_eval``: (values (P, m), gradients (P, m, d) | None) of the open paths at the rows of ``Xq``."""
        Xq = _c(np.atleast_2d(Xq))
        if Xq.shape[1] != self.d:
            raise ValueError(f"query points must have {self.d} columns, got {Xq.shape[1]}")
        P, m = self._paths_P, Xq.shape[0]
        out = np.empty((P, m))
        dout = np.empty((P, m, self.d)) if want_grad else None
        _check(self._lib.bgp_paths_eval(self._h, m, _p(Xq), _p(out), _p(dout) if want_grad else C.cast(None, _dp)), "bgp_paths_eval")
        return out, dout

    def paths_minimize(self, X0, lo, hi, gtol=1e-5, max_iter=200, want_grad=False):
        """``bgp_paths_minimize``: minimise every open path over the box [lo, hi] from its own starts ``X0`` (P, S, d), one
        workgroup per (start, path) in one launch.  Returns a dict: x (P, S, d; inside the box exactly), fun (P, S; normalised
        units) and grad (P, S, d | None): the search's evaluator at x; iters, evals, status (P, S; 0 converged to ``gtol``, 1
        ``max_iter`` reached, 2 no decrease found or a non-finite objective / gradient).  ``max_iter=0`` evaluates the clipped starts."""
        X0 = _c(X0)
        P = self._paths_P
        if X0.ndim != 3 or X0.shape[2] != self.d or (P and X0.shape[0] != P):
            raise ValueError(f"X0 must be (P, S, d) = ({P}, S, {self.d}), got {X0.shape}")
        S = X0.shape[1]
        shape = (max(P, X0.shape[0]), S)
        lo = _c(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.d,)))
        hi = _c(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.d,)))
        x, fun = np.empty(shape + (self.d,)), np.empty(shape)
        grad = np.empty(shape + (self.d,)) if want_grad else None
        iters, evals, status = (np.zeros(shape, dtype=np.int32) for _ in range(3))
        _check(self._lib.bgp_paths_minimize(self._h, S, _p(X0), _p(lo), _p(hi), float(gtol), int(max_iter), _p(x), _p(fun),
                                            _p(grad) if want_grad else C.cast(None, _dp), _p(iters), _p(evals), _p(status)),
               "bgp_paths_minimize")
        return {"x": x, "fun": fun, "grad": grad, "iters": iters, "evals": evals, "status": status}

    def paths_select(self, Xcand, q, kind="improvement", incumbent=None, forced=(), want_values=True, want_incumbents=True):
        """``bgp_paths_select``: ``q`` greedy picks among the rows of ``Xcand`` on the joint draw of the open
        paths, in normalised-y units.  ``kind``: "improvement" (Monte-Carlo q-EI gains) or "thompson" (step j is path j mod P's
        minimiser).  ``incumbent``: None -- every path's own minimum over the training inputs -- or a number, the same for every path.
        ``forced``: candidate indices taken as chosen before the first step.  Returns (picks (q,), values (q, m) | None, incumbents
        (P,) | None).  ``ValueError`` when paths x candidates (padded to 256) exceed ``SELECT_MAX_DOUBLES``."""
        Xcand = _c(np.atleast_2d(Xcand))
        if Xcand.shape[1] != self.d:
            raise ValueError(f"candidates must have {self.d} columns, got {Xcand.shape[1]}")
        if isinstance(kind, str) and kind not in SELECT_KINDS:
            raise ValueError(f"kind must be one of {tuple(SELECT_KINDS)}, got {kind!r}")
        kind = SELECT_KINDS[kind] if isinstance(kind, str) else int(kind)  # (a number goes to the C layer as it is)
        P, m, q = self._paths_P, Xcand.shape[0], int(q)
        if P * (-(-m // 256) * 256) > SELECT_MAX_DOUBLES:
            raise ValueError(f"{P} paths x {m} candidates exceed the {SELECT_MAX_DOUBLES} doubles of the resident draw matrix")
        forced = np.ascontiguousarray(forced, dtype=np.int32).ravel()
        picks = np.full(max(q, 0), -1, dtype=np.int32)
        values = np.empty((max(q, 0), m)) if want_values else None
        inc = np.empty(P) if want_incumbents else None
        null = C.cast(None, _dp)
        _check(self._lib.bgp_paths_select(self._h, m, _p(Xcand), kind, 0 if incumbent is not None else 1,
                                          float(incumbent) if incumbent is not None else 0.0, len(forced),
                                          _p(forced) if len(forced) else C.cast(None, _ip), q, _p(picks),
                                          _p(values) if want_values else null, _p(inc) if want_incumbents else null),
               "bgp_paths_select")
        return picks, values, inc

    def paths_end(self):
        self._paths_P = 0
        _check(self._lib.bgp_paths_end(self._h), "bgp_paths_end")

    def paths_stats(self):
        out = (C.c_longlong * 2)()
        _check(self._lib.bgp_paths_stats(self._h, out), "bgp_paths_stats")
        return {"begins": int(out[0]), "evals": int(out[1])}

    def chunk_stats(self):
        """Chunks of the last budget-chunked posterior call: posteriors, and query rows / candidates / starts."""
        out = (C.c_longlong * 2)()
        _check(self._lib.bgp_chunk_stats(self._h, out), "bgp_chunk_stats")
        return {"items": int(out[0]), "rows": int(out[1])}

    def sample_y(self, b, h_kernel, Xq, z, jitter=0.0):
        H = self._H(h_kernel)
        Xq = _c(np.atleast_2d(Xq))
        z = _c(np.atleast_2d(z))
        m = Xq.shape[0]
        if z.shape[1] != m:
            raise ValueError("z must be (n_draws, m)")
        out = np.empty_like(z)
        rc = self._lib.bgp_sample_y(self._h, int(b), _p(H), m, _p(Xq), z.shape[0], _p(z), float(jitter), _p(out))
        if rc == BGP_ERR_NOTPD:
            raise NotPositiveDefinite(self._lib.bgp_last_error().decode())
        _check(rc, "bgp_sample_y")
        return out

    def sample_y_batch(self, pidx, H_kernel, Xq, z, jitter=0.0):
        """One draw per resident posterior pidx[i]: returns (out (B, m), status (B,))."""
        H = self._H(H_kernel)
        Xq = _c(np.atleast_2d(Xq))
        z = _c(np.atleast_2d(z))
        pidx = np.ascontiguousarray(pidx, dtype=np.int32)
        B, m = H.shape[0], Xq.shape[0]
        if z.shape != (B, m) or pidx.shape != (B,):
            raise ValueError("z must be (B, m) and pidx (B,)")
        out = np.empty_like(z)
        st = np.zeros(B, dtype=np.int32)
        _check(self._lib.bgp_sample_y_batch(self._h, B, _p(pidx), _p(H), m, _p(Xq), _p(z), float(jitter), _p(out),
                                            _p(st)), "bgp_sample_y_batch")
        return out, st

    def debug_workspace(self, b):
        """(L, z) of batch slot b as the last ``lml`` call left them: the (npad, npad) working matrix (factor in its lower
        triangle) and the working right-hand side."""
        npad = -(-self.n // 128) * 128
        L = np.empty((npad, npad))
        z = np.empty(npad)
        _check(self._lib.bgp_debug_workspace(self._h, int(b), _p(L), _p(z)), "bgp_debug_workspace")
        return L, z

    def debug_cov_factor(self):
        """The (mpad, mpad) factor of the predictive covariance the last ``sample_y`` left (lower triangle); None without one."""
        mp = C.c_int(0)
        _check(self._lib.bgp_debug_cov_factor(self._h, C.byref(mp), C.cast(None, _dp)), "bgp_debug_cov_factor")
        if mp.value == 0:
            return None
        L = np.empty((mp.value, mp.value))
        _check(self._lib.bgp_debug_cov_factor(self._h, C.byref(mp), _p(L)), "bgp_debug_cov_factor")
        return L

    def lml_plan(self, B, warped=False):
        """What ``lml`` / ``lml_warped`` of ``B`` rows would launch on this context as it stands (``bgp_debug_lml_plan``; nothing is
        enqueued): see ``_lib.lml_plan``."""
        return _lml_plan(self._h, LmlPlanQuery(nb=int(B), warped=int(bool(warped))))

    def persist_stats(self):
        """Launch-free path bookkeeping (bgp_persist_stats): calls enqueued, time-outs, whether a time-out keeps the path off
        and for how many eligible calls."""
        v = (C.c_longlong * 4)()
        _check(self._lib.bgp_persist_stats(self._h, v), "bgp_persist_stats")
        return {"calls": int(v[0]), "timeouts": int(v[1]), "disabled": bool(v[2]), "cooldown_left": int(v[3])}

    def gen_stats(self):
        """LML batches whose kernel-matrix blocks (all but block column 0) were generated inside the trailing update of the first
        panel group, and the generating launches among their updates (bgp_lml_gen_stats)."""
        v = (C.c_longlong * 2)()
        _check(self._lib.bgp_lml_gen_stats(self._h, v), "bgp_lml_gen_stats")
        return {"batches": int(v[0]), "launches": int(v[1])}

    def ps_trace(self):
        """In-kernel timeline of the last launch-free call (needs BGP_PS_TRACE=1 at context creation): (chain, tile) --
        wall-clock stamps (100 MHz), 8 per (matrix, block column) of the chain role and 8 per tile task; None without a
        trace (bgp_debug_ps_trace)."""
        dims = (C.c_int * 3)()
        _check(self._lib.bgp_debug_ps_trace(self._h, dims, None, 0), "bgp_debug_ps_trace")
        B, nblk, total = dims[0], dims[1], dims[2]
        if B * nblk == 0:
            return None
        buf = np.zeros(B * nblk * 8 + total * 8, dtype=np.uint64)
        _check(self._lib.bgp_debug_ps_trace(self._h, dims, buf.ctypes.data_as(C.POINTER(C.c_ulonglong)), buf.size),
               "bgp_debug_ps_trace")
        return buf[: B * nblk * 8].reshape(B, nblk, 8), buf[B * nblk * 8:].reshape(total, 8)

    def set_streams(self, nstreams):
        _check(self._lib.bgp_set_streams(self._h, int(nstreams)), "bgp_set_streams")

    def set_persist(self, mode):
        """Launch-free factorisation of small batches: 1 on, 0 off, -1 as BGP_PERSIST says (bgp_set_persist)."""
        _check(self._lib.bgp_set_persist(self._h, int(mode)), "bgp_set_persist")

    def set_panel_fused(self, mode):
        """Diagonal block and panel solve of a block column in one launch on the launch schedule's LML path: 1 on, 0 off, -1 as
        BGP_PANEL_FUSED says (bgp_set_panel_fused)."""
        _check(self._lib.bgp_set_panel_fused(self._h, int(mode)), "bgp_set_panel_fused")

    def panel_fused_stats(self):
        """Fused panel launches enqueued by this context (bgp_panel_fused_stats)."""
        v = (C.c_longlong * 1)()
        _check(self._lib.bgp_panel_fused_stats(self._h, v), "bgp_panel_fused_stats")
        return {"launches": int(v[0])}

    def set_timing(self, enable):
        _check(self._lib.bgp_set_timing(self._h, int(bool(enable))), "bgp_set_timing")
        self._timing = bool(enable)

    def lml_wait_allgather(self, comm, per_rank, local_error=0):
        """Collective form of ``lml_wait`` for the exact single-ensemble sharding: every rank has submitted its own rows
        (possibly none) of the half-step's block; returns ((world, per_rank) log-likelihoods of all ranks, (world,) status
        words), gathered device to device over RCCL out of the contexts' resident result vectors
        (bgp_lml_batch_wait_allgather).  ``local_error`` > 0: this rank's own work failed -- it still takes part (its peers
        would block in the collective otherwise) and every rank finds the code in the status words."""
        out = np.empty((comm.world, int(per_rank)))
        errs = np.zeros(comm.world, dtype=np.int32)
        try:
            rc = self._lib.bgp_lml_batch_wait_allgather(self._h, comm._h, int(per_rank), int(local_error), _p(out), _p(errs))
        finally:
            self._pending, self._pending_H = 0, None  # (the C call consumes the pending batch whatever its outcome)
        _check(rc, "bgp_lml_batch_wait_allgather")
        return out, errs

    def last_timing(self):
        ms = np.zeros(5)
        cnt = np.zeros(4, dtype=np.int32)
        _check(self._lib.bgp_last_timing(self._h, _p(ms), _p(cnt)), "bgp_last_timing")
        names = ("kbuild", "potrf", "trsm", "syrk")
        out = {k: {"ms": float(ms[i]), "launches": int(cnt[i])} for i, k in enumerate(names)}
        out["device_total_ms"] = float(ms[4])
        cms, cn = C.c_double(0.0), C.c_int(0)
        _check(self._lib.bgp_last_timing_columns(self._h, C.byref(cms), C.byref(cn)), "bgp_last_timing_columns")
        # the look-ahead column launches inside "syrk" (K = 128 .. 128 (P-1) on one block column)
        out["syrk_columns"] = {"ms": float(cms.value), "launches": int(cn.value)}
        return out


COMM_ID_BYTES = 128


def comm_available(load_it=False):
    """True when librccl.so is there for the native multi-GPU backend.  By default the library is only LOOKED for (the paths
    bgp_comm.hip tries): loading the system's librccl into a process that may still fall back to torch's gloo group -- torch
    brings an RCCL of its own -- ends in a double free at exit.  ``load_it=True`` really dlopens it (bgp_comm_available)."""
    if load_it:
        return bool(load().bgp_comm_available())
    import ctypes.util

    return any(os.path.exists(p) for p in ("/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so")) \
        or ctypes.util.find_library("rccl") is not None


def comm_unique_id():
    """ncclGetUniqueId through libbgp (rank 0): 128 opaque bytes every rank needs for ``Comm``."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().bgp_comm_unique_id(C.cast(buf, _vp)), "bgp_comm_unique_id")
    return buf.raw


class Comm:
    """RCCL communicator of this process (one process per GPU) behind the C-ABI: host arrays in, host arrays out."""

    def __init__(self, device, rank, world, unique_id):
        self._lib = load()
        self.rank, self.world = int(rank), int(world)
        h = _vp()
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _check(self._lib.bgp_comm_init(int(device), self.rank, self.world, C.cast(buf, _vp), C.byref(h)), "bgp_comm_init")
        self._h = h

    @classmethod
    def loopback(cls, device, rank, world, key):
        """Loop-back communicator (``bgp_comm_init_loopback``): rank ``rank`` of ``world`` communicators of THIS process on one
        device, one per host thread; serves the in-stream exchange of a sharded resident sampler run only (tests)."""
        self = cls.__new__(cls)
        self._lib = load()
        self.rank, self.world = int(rank), int(world)
        h = _vp()
        _check(self._lib.bgp_comm_init_loopback(int(device), self.rank, self.world, int(key), C.byref(h)), "bgp_comm_init_loopback")
        self._h = h
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bgp_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def allgather(self, a):
        a = _c(a)
        out = np.empty((self.world,) + a.shape)
        _check(self._lib.bgp_comm_allgather(self._h, _p(a), a.size, _p(out)), "bgp_comm_allgather")
        return out

    def allreduce_max(self, a):
        a = _c(np.array(a, dtype=np.float64, copy=True))
        _check(self._lib.bgp_comm_allreduce_max(self._h, _p(a), a.size), "bgp_comm_allreduce_max")
        return a

    def broadcast(self, a, root=0):
        a = _c(np.array(a, dtype=np.float64, copy=True))
        _check(self._lib.bgp_comm_broadcast(self._h, _p(a), a.size, int(root)), "bgp_comm_broadcast")
        return a

    def barrier(self):
        _check(self._lib.bgp_comm_barrier(self._h), "bgp_comm_barrier")

    def abort(self):
        """ncclCommAbort: the peers' collectives fail at once instead of waiting for this rank."""
        if getattr(self, "_h", None):
            self._lib.bgp_comm_abort(self._h)

    def bench_lml_gather(self, ctx, per, reps=200):
        """ms per round of the sharded resident sampler's in-stream exchange (``bgp_comm_bench_lml_gather``; every rank calls)."""
        v = C.c_double(0.0)
        _check(self._lib.bgp_comm_bench_lml_gather(ctx._h, self._h, int(per), int(reps), C.byref(v)), "bgp_comm_bench_lml_gather")
        return float(v.value)

    def nranks(self):
        """Ranks RCCL itself counts in the communicator (ncclCommCount)."""
        v = C.c_int(0)
        _check(self._lib.bgp_comm_nranks(self._h, C.byref(v)), "bgp_comm_nranks")
        return int(v.value)


def device_synchronize(device=0):
    _check(load().bgp_device_synchronize(int(device)), "bgp_device_synchronize")


def bench_mfma_f64(device=0, iters=20000):
    v = C.c_double(0.0)
    _check(load().bgp_bench_mfma_f64(device, iters, C.byref(v)), "bgp_bench_mfma_f64")
    return v.value


def bench_hbm_copy(device=0, nbytes=1 << 30, iters=10):
    v = C.c_double(0.0)
    _check(load().bgp_bench_hbm_copy(device, nbytes, iters, C.byref(v)), "bgp_bench_hbm_copy")
    return v.value


def pivot_root(x, device=0):
    """(sqrt(x), 1 / sqrt(x)) as the diagonal-block factorisation forms its pivots (bgp_debug_pivot_root)."""
    x = _c(x).ravel()
    s, r = np.empty_like(x), np.empty_like(x)
    _check(load().bgp_debug_pivot_root(int(device), x.size, _p(x), _p(s), _p(r)), "bgp_debug_pivot_root")
    return s, r


def mfma_f64_layout(device=0):
    rows = np.zeros(256, dtype=np.int32)
    cols = np.zeros(256, dtype=np.int32)
    _check(load().bgp_mfma_f64_layout(device, _p(rows), _p(cols)), "bgp_mfma_f64_layout")
    return rows.reshape(64, 4), cols.reshape(64, 4)
