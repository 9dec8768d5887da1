"""CPU reference of the prediction covariance / leverage call (calico_prediction_covariance), shared by
test_prediction_host.py and test_gpu_prediction_covariance.py.

Recipe (include/calico_hip.h, "prediction covariance and leverage of the observations"): the oracle's dense Jacobian J at
the given values (rows: every sensor's residual blocks in insertion order, sensor after sensor; the loss through the
corrector), H = JᵀJ, exactly-zero diagonal columns dropped, S = H⁻¹ in numpy, P_i = J_i S J_iᵀ. For apply_loss = 0 the rows
J_i come from a second oracle problem built from a copy of the scene with every sensor's loss switched off, at the same
values; S stays the first one's."""
import copy
import ctypes as C

import numpy as np

import helpers
from calico_amd import synthetic as syn
from helpers import copy_values  # noqa: F401  (the tests reach it through this module)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def oracle_lib():
    helpers.build_oracle()
    L = helpers.oracle_lib()
    L.oracle_num_residuals.restype = C.c_int64
    return L


def dense_jacobian(ref):
    """The oracle's dense Jacobian (n_res x n_eff) at its current values."""
    L = oracle_lib()
    P = ref.problem
    n = P.num_effective_parameters()
    nres = L.oracle_num_residuals(P.h)
    J = np.zeros((nres, n))
    st = L.oracle_evaluate_jacobian(P.h, None, _dp(J))
    assert st == 0, st
    return J


def without_loss(scene):
    s2 = copy.deepcopy(scene)
    for s in s2.sensors:
        s.loss = 0
    return s2


def sensor_rows(scene):
    """[(first row, n, d)] of every sensor's blocks in the dense Jacobian."""
    out, r = [], 0
    for s in scene.sensors:
        out.append((r, s.n, s.dim))
        r += s.n * s.dim
    return out


class Reference:
    """S = (JᵀJ)⁻¹ on the kept columns (zeros elsewhere) from the problem `ref_fit` -- the observations that are in the fit --
    and, for rows J of the same column order, P_i and the bound's β per row."""

    def __init__(self, ref_fit):
        J = dense_jacobian(ref_fit)
        self.J_fit = J
        self._invert(J.T @ J)

    @classmethod
    def from_normal_matrix(cls, H):
        """From a dense JᵀJ alone (problem.evaluate()): S, H and the trace bound, no rows."""
        self = cls.__new__(cls)
        self.J_fit = None
        self._invert(np.asarray(H))
        return self

    def _invert(self, H):
        self.H = H
        self.keep = np.diag(H) != 0.0
        idx = np.nonzero(self.keep)[0]
        self.S = np.zeros_like(H)
        self.S[np.ix_(idx, idx)] = np.linalg.inv(H[np.ix_(idx, idx)])
        self.sd = np.sqrt(np.abs(np.diag(self.S)))

    @property
    def n_kept(self):
        return int(self.keep.sum())

    def blocks(self, J, first, n, d):
        """P (n, d, d) and β (n, d) of the n blocks of dimension d whose rows start at `first` in J."""
        Jb = J[first:first + n * d].reshape(n, d, -1)
        T = Jb @ self.S
        P = np.einsum("nac,nbc->nab", T, Jb)
        beta = np.abs(Jb) @ self.sd
        return P, beta

    def trace_bound(self, tol=1e-7):
        """The per-entry guarantee on Σ pushed through trace(Σ H): tol (Σ_j sqrt(S_jj H_jj))²."""
        return tol * float(np.sum(np.sqrt(np.abs(np.diag(self.S) * np.diag(self.H)))) ** 2)


def build_pair(oracle_api, scene):
    """The scene in the oracle with and without the sensors' loss functions."""
    return syn.build_problem(oracle_api, scene), syn.build_problem(oracle_api, without_loss(scene))
