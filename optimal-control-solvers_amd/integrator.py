"""Integrator plugin (reference: Integrator/Integrator.m, Integrator/RK4Integrator.m).

Host calls take numpy arrays in MATLAB shapes with the batch as an optional trailing
dimension; `*_dev` calls take torch CUDA tensors in the device-native batch-minor layout
and run asynchronously on torch's current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import check, dp, lib
from .problem import _f, _p


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dptr(t):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


# ---- the tiled device layout (include/ocs.h, ocs_integrator_set_layout) ----------------------
TILE = 16


def tiled_doubles(rows, cols, batch):
    """doubles of a tiled array of `cols` columns x `rows` rows x `batch` trajectories (whole tiles of 16)"""
    return int(check(lib.ocs_tiled_doubles(rows, cols, batch)))


def tiled_index(rows, cols, batch):
    """The index map of the tiled layout, in NumPy: an int64 array [cols][rows][batch] whose entry (i, r, b) is the
    position of that element in the flat tiled array, ((b // 16) * cols + i) * rows * 16 + r * 16 + b % 16."""
    i = np.arange(cols, dtype=np.int64)[:, None, None]
    r = np.arange(rows, dtype=np.int64)[None, :, None]
    b = np.arange(batch, dtype=np.int64)[None, None, :]
    return ((b // TILE) * cols + i) * rows * TILE + r * TILE + b % TILE


def to_tiled(src, out=None):
    """batch-minor device tensor [cols][rows][B] -> flat tiled tensor (pad lanes: copies of the last trajectory)"""
    cols, rows, B = src.shape
    assert src.is_cuda and src.dtype == torch.float64 and src.is_contiguous()
    if out is None:
        out = torch.empty(tiled_doubles(rows, cols, B), dtype=torch.float64, device=src.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == tiled_doubles(rows, cols, B)
    check(lib.ocs_to_tiled_dev(_dptr(src), _dptr(out), rows, cols, B, _stream()))
    return out


def from_tiled(src, rows, cols, batch, out=None):
    """flat tiled device tensor -> batch-minor [cols][rows][batch]"""
    assert src.is_cuda and src.dtype == torch.float64 and src.is_contiguous() and src.numel() == tiled_doubles(rows, cols, batch)
    if out is None:
        out = torch.empty((cols, rows, batch), dtype=torch.float64, device=src.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (cols, rows, batch)
    check(lib.ocs_from_tiled_dev(_dptr(src), _dptr(out), rows, cols, batch, _stream()))
    return out


class Integrator:
    """Integrator/Integrator.m:6-15: property t, compute_states, compute_adjoints."""
    t = None

    def compute_states(self, prob, x0, u):
        raise NotImplementedError

    def compute_adjoints(self, prob, u, lamT=None):
        raise NotImplementedError


class RK4Integrator(Integrator):
    """Integrator/RK4Integrator.m:16-25: obj = RK4Integrator(tspan)."""

    def __init__(self, tspan):
        self.tspan = _f(tspan).ravel()
        h = C.c_void_p()
        check(lib.ocs_rk4_create(C.byref(h), _p(self.tspan), self.tspan.size))
        self._finish_init(h)

    def _finish_init(self, h):
        self._h = h
        n = C.c_int()
        check(lib.ocs_integrator_nsteps(h, C.byref(n)))
        self.nSTEPS = n.value
        self.t = np.empty(2 * self.nSTEPS + 1)
        self.h = np.empty(self.nSTEPS)
        check(lib.ocs_integrator_t(h, _p(self.t)))
        check(lib.ocs_integrator_h(h, _p(self.h)))
        self._batch_shape = None
        self._layout = "batch_minor"

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ocs_integrator_destroy(h)
            self._h = None

    def set_mapping(self, mapping):
        """Thread mapping of the RK4 kernels: "auto", "lane" (lane per trajectory) or "rowsplit"."""
        code = mapping if isinstance(mapping, int) else {"auto": 0, "lane": 1, "rowsplit": 2, "pipeline": 3, "scan": 4}[mapping]
        check(lib.ocs_integrator_set_mapping(self._h, code))
        return self

    def set_layout(self, layout):
        """Device layout of the per-step arrays of compute_states_dev / compute_adjoints_dev: "batch_minor" (default,
        [cols][rows][B]) or "tiled" (flat tensors of tiled_doubles(rows, cols, B) doubles; see to_tiled / from_tiled)."""
        code = layout if isinstance(layout, int) else {"batch_minor": 0, "tiled": 1}[layout]
        check(lib.ocs_integrator_set_layout(self._h, code))
        self._layout = "tiled" if code == 1 else "batch_minor"
        return self

    @property
    def layout(self):
        return self._layout

    # ---- host path (MATLAB shapes) -------------------------------------------------
    def compute_states(self, prob, x0, u):
        """[x, J] = compute_states(obj, prob, x0, u)   RK4Integrator.m:28-56.
        x0: nS (x batch); u: nC x (2N+1) (x batch).  Returns x nAug x (N+1) (x batch), J."""
        N = self.nSTEPS
        u = np.asarray(u, dtype=np.float64)
        batched = u.ndim == 3
        batch = u.shape[2] if batched else 1
        u = _f(u, (prob.nC, 2 * N + 1, batch))
        x0 = _f(x0, (prob.nS, batch))
        x = np.empty((prob.nAug, N + 1, batch), order="F")
        J = np.empty(batch)
        self.status = check(lib.ocs_compute_states(self._h, prob._h, batch, _p(x0), _p(u), _p(x), _p(J)))
        return (x, J) if batched else (x[:, :, 0], float(J[0]))

    def compute_adjoints(self, prob, u, lamT=None, nargout=2):
        """[lam, dJdu] = compute_adjoints(obj, prob, u, lamT)   RK4Integrator.m:59-121."""
        N = self.nSTEPS
        u = np.asarray(u, dtype=np.float64)
        batched = u.ndim == 3
        batch = u.shape[2] if batched else 1
        u = _f(u, (prob.nC, 2 * N + 1, batch))
        lt = None if lamT is None else _f(lamT, (prob.nAug, batch))
        lam = np.empty((prob.nAug, N + 1, batch), order="F")
        dJdu = np.empty((prob.nC, 2 * N + 1, batch), order="F") if nargout > 1 else None
        check(lib.ocs_compute_adjoints(self._h, prob._h, batch, _p(u), _p(lt), _p(lam), _p(dJdu)))
        if not batched:
            lam = lam[:, :, 0]
            dJdu = None if dJdu is None else dJdu[:, :, 0]
        return (lam, dJdu) if nargout > 1 else lam

    # ---- device path (batch-minor torch tensors, async on the current stream) --------
    @staticmethod
    def _chk(name, t, shape, dev, tiled=False):
        """a wrongly sized or misplaced device tensor is an out-of-bounds access inside a kernel, i.e. a GPU fault:
        check shape, dtype, contiguity and device here.  tiled: the per-step array [cols][rows][B] named by `shape` is
        held in the tiled layout, a flat tensor of whole tiles"""
        if t is None:
            return
        if tiled:
            shape = (tiled_doubles(shape[1], shape[0], shape[2]),)
        if tuple(t.shape) != tuple(shape) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name}: expected a contiguous float64 tensor of shape {tuple(shape)} on {dev}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")

    def compute_states_dev(self, prob, x0, u, x=None, J=None):
        """x0 [nS][B], u [2N+1][nC][B] -> x [N+1][nAug][B] (optional), J [B]."""
        N = self.nSTEPS
        B = x0.shape[-1]
        nS, nC, dev = prob.nS, prob.ControlBounds.shape[0], x0.device
        if J is None:
            J = torch.empty(B, dtype=torch.float64, device=dev)
        self._chk("x0", x0, (nS, B), dev)
        tl = self._layout == "tiled"
        self._chk("u", u, (2 * N + 1, nC, B), dev, tiled=tl)
        self._chk("x", x, (N + 1, nS + 1, B), dev, tiled=tl)
        self._chk("J", J, (B,), dev)
        check(lib.ocs_compute_states_dev(self._h, prob._h, B, _dptr(x0), _dptr(u), _dptr(x), _dptr(J),
                                         _stream()))
        self._ck_ref = x   # the adjoint pass re-reads it (the xK contract): keep it alive until then
        return x, J

    def compute_adjoints_dev(self, prob, u, lamT=None, lam=None, dJdu=None, batch=None):
        """batch: needed on a handle set to the tiled layout, whose flat u does not tell it"""
        N = self.nSTEPS
        B = u.shape[-1] if batch is None else batch
        nS, nC, dev = prob.nS, prob.ControlBounds.shape[0], u.device
        tl = self._layout == "tiled"
        self._chk("u", u, (2 * N + 1, nC, B), dev, tiled=tl)
        self._chk("lamT", lamT, (nS + 1, B), dev)
        self._chk("lam", lam, (N + 1, nS + 1, B), dev, tiled=tl)
        self._chk("dJdu", dJdu, (2 * N + 1, nC, B), dev, tiled=tl)
        check(lib.ocs_compute_adjoints_dev(self._h, prob._h, B, _dptr(u), _dptr(lamT), _dptr(lam),
                                           _dptr(dJdu), _stream()))
        return lam, dJdu

    def trajectory_status(self, batch):
        """per-trajectory flags of the last host compute_states / nlp_objective call on this handle
        (OCS_NUM_NONFINITE = 1 where the objective is NaN/Inf)"""
        st = np.zeros(batch, dtype=np.int32)
        check(lib.ocs_integrator_trajectory_status(self._h, batch, st.ctypes.data_as(C.POINTER(C.c_int))))
        return st


def trajectory_status_dev(J, status=None):
    """device: status [B] int32 from J [B] (asynchronous on the current stream)"""
    if status is None:
        status = torch.empty(J.shape[0], dtype=torch.int32, device=J.device)
    check(lib.ocs_trajectory_status_dev(J.shape[0], _dptr(J), C.c_void_p(status.data_ptr()), _stream()))
    return status


def split_uStar(uStar):
    """What RK4InfiniteIntegrator's constructor makes of its uStar argument (no device needed): (shared, batch).
    A scalar, a vector or a single column is the reference's uStar, nC values shared by every trajectory: (that vector,
    None).  A matrix with more than one column is nC x B, a uStar per trajectory: (its column 0, the matrix)."""
    a = np.asarray(uStar, dtype=np.float64)
    if a.ndim > 2:
        raise ValueError(f"uStar: expected nC values or an nC x B matrix, got shape {a.shape}")
    if a.ndim == 2 and a.shape[1] > 1:
        return _f(a[:, 0]).ravel(), _f(a)
    if a.size < 1:
        raise ValueError("uStar is empty")
    return _f(np.atleast_1d(a)).ravel(), None


def batch_uStar_host(U, nC):
    """The host argument of set_batch_uStar as the library takes it: nC x B, column-major (no device needed).  A 1-D
    array is refused: it does not say whether it is one trajectory's nC values or nC = 1 for B trajectories."""
    a = np.asarray(U, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"uStar per trajectory: expected an nC x B matrix ({nC} x B), got {a.ndim}-D input of shape {a.shape}")
    if a.shape[0] != nC or a.shape[1] < 1:
        raise ValueError(f"uStar per trajectory: expected {nC} x B (nC of the integrator's uStar), got {a.shape[0]} x {a.shape[1]}")
    return _f(a)


class RK4InfiniteIntegrator(RK4Integrator):
    """Integrator/RK4InfiniteIntegrator.m:12-30: RK4 on tspan, then a tail leg on tspanExtra under
    the constant control uStar; J = J1 + J2, terminal adjoint of leg 1 = lam2(:,1).

    uStar: the reference's nC values, shared by every trajectory of a call -- or (batch extension, no counterpart in the
    reference) an nC x B matrix with B > 1 columns, a constant tail control per trajectory: trajectory b is then integrated
    as RK4InfiniteIntegrator(tspan, tspanExtra, uStar[:, b]) would, and calls must use batch B (see set_batch_uStar)."""

    def __init__(self, tspan, tspanExtra, uStar):
        self.tspan = _f(tspan).ravel()
        self.tspanExtra = _f(tspanExtra).ravel()
        shared, batch = split_uStar(uStar)
        self.uStar = shared if batch is None else batch
        self.batch_uStar = None
        h = C.c_void_p()
        check(lib.ocs_rk4inf_create(C.byref(h), _p(self.tspan), self.tspan.size, _p(self.tspanExtra),
                                    self.tspanExtra.size, _p(shared), shared.size))
        self._finish_init(h)
        self._nC = shared.size
        if batch is not None:
            self.set_batch_uStar(batch)

    def set_batch_uStar(self, U=None):
        """A constant tail control of its own per trajectory (e.g. the uStar of each instance's compute_equilibrium under
        per-trajectory parameters): U is nC x B, a numpy array (host call) or a CUDA float64 tensor [nC][B] (device call,
        asynchronous on the current stream; the values are copied into a buffer of the handle).  Compute calls on this
        integrator must then use batch B.  No argument or None clears it: back to the shared uStar of the constructor."""
        if U is None:
            check(lib.ocs_rk4inf_set_batch_ustar(self._h, 0, None))
            self.batch_uStar = None
            return self
        if torch.is_tensor(U):
            if U.ndim != 2 or U.shape[0] != self._nC or U.shape[1] < 1 or not U.is_cuda or U.dtype != torch.float64 \
                    or not U.is_contiguous():
                raise ValueError(f"uStar per trajectory: expected a contiguous float64 CUDA tensor [{self._nC}][B], got "
                                 f"{tuple(U.shape)} {U.dtype} on {U.device}")
            check(lib.ocs_rk4inf_set_batch_ustar_dev(self._h, U.shape[1], _dptr(U), _stream()))
        else:
            U = batch_uStar_host(U, self._nC)
            check(lib.ocs_rk4inf_set_batch_ustar(self._h, U.shape[1], _p(U)))
        self.batch_uStar = U
        return self

    def compute_adjoints(self, prob, u, nargout=2):
        return super().compute_adjoints(prob, u, None, nargout)
