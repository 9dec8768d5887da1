"""The Levenberg-Marquardt step restated in numpy: what the linear solve of one iteration must produce.

A plain module (numpy only), shared by tests/test_lm_step_reference.py, which proves it on the CPU oracle, and the GPU step
tests, which hold the device's step against it. Columns are in calico_evaluate's order unless a caller says otherwise.

- damping: ceres::LevenbergMarquardtStrategy with Jacobi scaling (TrustRegionMinimizer: s_j = 1 / (1 + sqrt(H0_jj)) from the
  Jacobian at the solve's starting point, 1 without scaling), d_j = clamp(H_jj s_j^2, min_lm_diagonal, max_lm_diagonal) / (mu s_j^2)
  -- the damping of the scaled system taken back to the parameters' own units.
- reference_step: A delta = -g with A = H + diag(d), solved in float64 on the equilibrated system and refined with residuals in
  long double.
- backward_error / forward_error / kappa2: how close a given step is to solving that system.
- plus: Plus(x, delta) of the parameter blocks (Euclidean, EigenQuaternion) as the update stage forms it.
"""
import numpy as np

MANIFOLD_EUCLIDEAN, MANIFOLD_EIGEN_QUATERNION = 0, 1


def jacobi_scale(H0, jacobi_scaling=True):
    """s_j = 1 / (1 + sqrt(H0_jj)) (Ceres: from the first Jacobian of the solve), or 1 without scaling."""
    h = np.diag(H0)
    return 1.0 / (1.0 + np.sqrt(h)) if jacobi_scaling else np.ones_like(h)


def damping(H, scale, mu, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """d_j = clamp(H_jj s_j^2, min, max) / (mu s_j^2)."""
    s2 = np.asarray(scale, float) ** 2
    return np.minimum(np.maximum(np.diag(H) * s2, min_lm_diagonal), max_lm_diagonal) / (mu * s2)


def clamp_binds(H, scale, min_lm_diagonal, max_lm_diagonal):
    """Columns where the damping's clamp is active (the scaled diagonal lies outside [min, max])."""
    v = np.diag(H) * np.asarray(scale, float) ** 2
    return (v < min_lm_diagonal) | (v > max_lm_diagonal)


def _system(H, d):
    A = np.array(H, dtype=float, copy=True)
    A[np.diag_indices_from(A)] += d
    e = 1.0 / np.sqrt(np.diag(A))
    return A, e


def _residual_ld(A, g, delta):
    """A delta + g in long double."""
    Al = np.asarray(A, np.longdouble)
    return Al @ np.asarray(delta, np.longdouble) + np.asarray(g, np.longdouble)


def reference_step(H, g, d, refine=2):
    """delta with (H + diag(d)) delta = -g: float64 solve of E A E (E = diag(A_jj^-1/2)), `refine` steps of iterative
    refinement with long-double residuals."""
    A, e = _system(H, d)
    EAE = A * np.outer(e, e)
    delta = e * np.linalg.solve(EAE, -e * g)
    for _ in range(refine):
        r = -_residual_ld(A, g, delta)
        delta = delta + e * np.linalg.solve(EAE, e * np.asarray(r, float))
    return delta


def backward_error(H, g, d, delta):
    """Normwise backward error of delta for the equilibrated system:
    ||E (A delta + g)||_inf / (||E A E||_inf ||E^-1 delta||_inf + ||E g||_inf), residual in long double."""
    A, e = _system(H, d)
    r = np.abs(np.asarray(e, np.longdouble) * _residual_ld(A, g, delta)).max()
    EAE = np.abs(A * np.outer(e, e))
    den = EAE.sum(axis=1).max() * np.abs(delta / e).max() + np.abs(e * g).max()
    return float(r / den) if den > 0 else float(r)


def backward_error_f64(H, g, d, delta):
    """The same with a float64 residual (the single long case, whose dense long-double product would take too long)."""
    A, e = _system(H, d)
    r = np.abs(e * (A @ delta + g)).max()
    den = np.abs(A * np.outer(e, e)).sum(axis=1).max() * np.abs(delta / e).max() + np.abs(e * g).max()
    return float(r / den) if den > 0 else float(r)


def forward_error(H, d, delta, delta_ref):
    """||E^-1 (delta - delta_ref)||_inf / ||E^-1 delta_ref||_inf."""
    _, e = _system(H, d)
    den = np.abs(delta_ref / e).max()
    return float(np.abs((delta - delta_ref) / e).max() / den) if den > 0 else float(np.abs((delta - delta_ref) / e).max())


def kappa2(H, d):
    """2-norm condition number of E A E (symmetric positive definite: ratio of its extreme eigenvalues)."""
    A, e = _system(H, d)
    w = np.linalg.eigvalsh(A * np.outer(e, e))
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def model_cost_change(H, g, delta):
    """-(g^T delta + 1/2 delta^T H delta): the decrease the linear model predicts."""
    return float(-(g @ delta + 0.5 * delta @ (H @ delta)))


def quat_plus(x, dphi):
    """EigenQuaternion Plus, storage (x, y, z, w): [sin|d| d / |d|, cos|d|] * x."""
    d0, d1, d2 = dphi
    nd = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
    if not nd > 0.0:
        return np.array(x, float)
    sd, qw = np.sin(nd) / nd, np.cos(nd)
    qx, qy, qz = sd * d0, sd * d1, sd * d2
    px, py, pz, pw = x
    return np.array([qw * px + qx * pw + qy * pz - qz * py,
                     qw * py + qy * pw + qz * px - qx * pz,
                     qw * pz + qz * pw + qx * py - qy * px,
                     qw * pw - qx * px - qy * py - qz * pz])


def plus(blocks, delta):
    """Plus(x, delta) block by block. `blocks`: [(values, manifold)] in column order; delta holds 3 columns per quaternion,
    the ambient size for every other block. Returns the new values, one array per block."""
    out, c = [], 0
    for v, manifold in blocks:
        v = np.asarray(v, float)
        if manifold == MANIFOLD_EIGEN_QUATERNION:
            out.append(quat_plus(v, delta[c:c + 3]))
            c += 3
        else:
            out.append(v + delta[c:c + v.size])
            c += v.size
    assert c == len(delta), (c, len(delta))
    return out


def step_norm(blocks, new_values):
    """||Plus(x, delta) - x||_2 over the ambient values (the log's step_norm)."""
    return float(np.sqrt(sum(((np.asarray(v, float) - w) ** 2).sum() for (v, _), w in zip(blocks, new_values))))


# ---- column layout of a synthetic scene (calico_amd.synthetic.build_problem): which parameter block each column belongs to ----
def control_points_observed(scene):
    """Per control point: touched by some observation (segment i of a stamp reaches control points i .. i + order - 1)."""
    from calico_amd import synthetic as syn
    n_cp = len(scene.ctrl)
    act = np.zeros(n_cp, bool)
    for s in scene.sensors:
        if s.n:
            for seg in np.unique(syn.spline_index(scene.knots, scene.order, s.stamps)):
                act[seg:seg + scene.order] = True
    return act


def column_blocks(built, scene):
    """[(block id, manifold)] in calico_evaluate's column order: the observed control points, then the free blocks that
    some residual uses, in the order they were added (Problem's tangent order)."""
    from calico_amd import synthetic as syn
    quat = MANIFOLD_EIGEN_QUATERNION
    cols = [(int(b), MANIFOLD_EUCLIDEAN) for b, a in zip(built.ctrl_blocks, control_points_observed(scene)) if a]
    calib = []
    for k, (spec, b) in enumerate(zip(scene.bodies, built.bodies)):      # (body 0 first; most scenes have just that one)
        n_pts = len(spec.points)
        pc = np.broadcast_to(np.asarray(spec.points_constant, bool), (n_pts,))
        seen = np.zeros(n_pts, bool)
        cams = False
        for s in scene.sensors:
            if s.kind == 0 and s.n:
                mine = syn.body_indices(s) == k
                seen[np.asarray(s.point_idx)[mine]] = True
                cams = cams or bool(mine.any())
        calib += [(int(b["point_blocks"][i]), MANIFOLD_EUCLIDEAN) for i in range(n_pts) if seen[i] and not pc[i]]
        if cams and not spec.pose_constant:
            calib += [(b["t"], MANIFOLD_EUCLIDEAN), (b["q"], quat)]
    for s, b in zip(scene.sensors, built.sensor_blocks):
        if not s.n:
            continue
        if s.enable_intrinsics:
            calib.append((b["intrinsics"], MANIFOLD_EUCLIDEAN))
        if s.enable_extrinsics:
            calib += [(b["t"], MANIFOLD_EUCLIDEAN), (b["q"], quat)]
        if s.enable_latency:
            calib.append((b["latency"], MANIFOLD_EUCLIDEAN))
    # (blocks are numbered in the order they were added: sorting by id is the library's tangent order)
    return cols + sorted(calib)


def block_values(problem, cols):
    """[(values, manifold)] of the blocks of `cols` at the problem's current parameter values."""
    return [(problem.get_param_block(b, problem._sizes[b]), man) for b, man in cols]
