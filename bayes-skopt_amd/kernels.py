"""Kernel objects on the host and their mapping to the device's canonical hyper-parameter vector.

The reference builds its GP kernels from skopt's kernel classes, which are scikit-learn's kernels
plus ``gradient_x`` (``bask/utils.py:6``, ``bask/bayesgpr.py:12``); scikit-learn ships in the image,
skopt does not, so the host-side kernel *objects* (theta get/set in log space, bounds,
``clone_with_theta``; ``sklearn/kernels.py:285-338, 733-760``) are scikit-learn's.  No kernel
*arithmetic* runs on the host for the canonical forms: a kernel expression tree is analysed once into a
``KernelPlan`` that maps its ``theta`` to the canonical device vector ``h = [log c, log l_1..log l_d, log s2]``
(``include/bgp.h``), and every K(X, X) / K(X*, X) is evaluated by the HIP kernels.

Canonical expression trees (device Gram build):
    [ConstantKernel *] S(length_scale) [+ WhiteKernel]        form "product"
    [ConstantKernel +] S(length_scale) [+ WhiteKernel]        form "sum"
with S in {RBF, Matern(nu = 0.5 | 1.5 | 2.5)}, isotropic or anisotropic, in any operand order, any
hyper-parameter optionally "fixed".

Every OTHER tree scikit-learn can evaluate (two stationary terms, products of stationaries, general Matern nu,
RationalQuadratic, ExpSineSquared, DotProduct, ... -- the reference accepts any kernel, ``bask/bayesgpr.py:148-159``)
gets a ``GramPlan``: the host evaluates ``kernel_(X)`` with the kernel object, exactly as the reference does
(``sklearn/_gpr.py:582``), and the device does the factorisation, the solves, the log-likelihood, the inverse and
the predictive products (``bgp_lml_batch_gram`` / ``bgp_posterior_batch_gram`` / ``bgp_predict_batch_gram``).
There is still no CPU path for the factorisation.  Where ``compile_tree`` covers such a tree (everything but Matern with a
general nu and trees beyond the program's limits), the kernel arithmetic runs on the device too: the ``GramPlan`` carries a
``TreeProgram`` and the ``bgp_*_tree`` entry points take a ``(B, P)`` block of log-space parameters (``csrc/bgp_tree.hip``).
"""
import numpy as np
from sklearn.gaussian_process.kernels import (  # noqa: F401  (re-exported: the bask kernel vocabulary)
    RBF,
    ConstantKernel,
    Kernel,
    Matern,
    Product,
    Sum,
    WhiteKernel,
)

__all__ = ["RBF", "ConstantKernel", "Matern", "WhiteKernel", "Sum", "Product", "KernelPlan", "GramPlan", "analyse_kernel",
           "param_for_white_kernel_in_sum", "gradient_x", "compile_tree"]


def gradient_x(kernel, x, X_train):
    """``d k(x, X_train_i) / d x`` for every training point: (n, d).  The method skopt's kernel classes add to scikit-learn's
    (``kernel_.gradient_x(X[0], self.X_train_)`` in skopt's ``predict(return_mean_grad=True)``, the routine
    ``bask/bayesgpr.py:633`` forwards to, used by ``bask/optimizer.py:494`` through ``expected_minimum``), restated for
    scikit-learn kernel objects by recursion over the expression tree: Sum -> sum of the children's gradients, Product ->
    product rule with the children's cross-covariance rows, Exponentiation -> chain rule; leaves RBF, Matern (0.5 / 1.5 / 2.5 in
    closed form as skopt has them, any other nu through ``d/dz [z^nu K_nu(z)] = -z^nu K_{nu-1}(z)``), RationalQuadratic,
    ExpSineSquared, DotProduct; ConstantKernel and WhiteKernel contribute zeros."""
    from scipy.special import gamma, kv
    from sklearn.gaussian_process.kernels import DotProduct, Exponentiation, ExpSineSquared, RationalQuadratic

    x = np.asarray(x, dtype=np.float64).ravel()
    X_train = np.atleast_2d(np.asarray(X_train, dtype=np.float64))
    n, d = X_train.shape
    if isinstance(kernel, Sum):
        return gradient_x(kernel.k1, x, X_train) + gradient_x(kernel.k2, x, X_train)
    if isinstance(kernel, Product):
        f = kernel.k1(x[None, :], X_train)[0]
        g = kernel.k2(x[None, :], X_train)[0]
        return f[:, None] * gradient_x(kernel.k2, x, X_train) + g[:, None] * gradient_x(kernel.k1, x, X_train)
    if isinstance(kernel, Exponentiation):
        base = kernel.kernel(x[None, :], X_train)[0]
        return (kernel.exponent * base ** (kernel.exponent - 1.0))[:, None] * gradient_x(kernel.kernel, x, X_train)
    if isinstance(kernel, (ConstantKernel, WhiteKernel)):
        return np.zeros((n, d))
    if isinstance(kernel, DotProduct):
        return X_train.copy()
    if isinstance(kernel, ExpSineSquared):
        diff = x[None, :] - X_train
        dist = np.sqrt(np.sum(diff * diff, axis=1))
        arg = np.pi * dist / kernel.periodicity
        k = np.exp(-2.0 * (np.sin(arg) / kernel.length_scale) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            # d/dx exp(-2 sin^2(pi r / p) / l^2) = k * (-2 sin(2 pi r / p) / l^2) * (pi / p) * diff / r
            fac = np.where(dist > 0, k * (-2.0 * np.sin(2.0 * arg) / kernel.length_scale**2) * (np.pi / kernel.periodicity) / dist, 0.0)
        return fac[:, None] * diff
    if isinstance(kernel, (Matern, RBF, RationalQuadratic)):
        ell = np.broadcast_to(np.asarray(kernel.length_scale, dtype=np.float64), (d,))
        diff = (x[None, :] - X_train) / ell           # (x - X_i) / l
        r2 = np.sum(diff * diff, axis=1)
        if isinstance(kernel, RationalQuadratic):
            fac = -((1.0 + r2 / (2.0 * kernel.alpha)) ** (-kernel.alpha - 1.0))
        elif isinstance(kernel, Matern) and not np.isinf(kernel.nu):
            r = np.sqrt(r2)
            nu = float(kernel.nu)
            with np.errstate(divide="ignore", invalid="ignore"):
                if nu == 0.5:
                    fac = np.where(r > 0, -np.exp(-r) / r, 0.0)
                elif nu == 1.5:
                    fac = -3.0 * np.exp(-np.sqrt(3.0) * r)
                elif nu == 2.5:
                    fac = -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)
                else:
                    # k = c z^nu K_nu(z), z = sqrt(2 nu) r, c = 2^(1 - nu) / Gamma(nu);  dk/dr = -c sqrt(2 nu) z^nu K_{nu-1}(z)
                    z = np.sqrt(2.0 * nu) * r
                    dk_dr = -(2.0 ** (1.0 - nu) / gamma(nu)) * np.sqrt(2.0 * nu) * z**nu * kv(nu - 1.0, z)
                    fac = np.where(r > 0, dk_dr / r, 0.0)
                    if nu > 1.0:  # (the limit r -> 0 of (dk/dr) / r is finite for nu > 1: -nu / (nu - 1))
                        fac = np.where(r > 0, fac, -nu / (nu - 1.0))
        else:  # RBF (and Matern with nu = inf)
            fac = -np.exp(-0.5 * r2)
        return fac[:, None] * diff / ell
    raise NotImplementedError("gradient_x is not implemented for %s" % type(kernel).__name__)


def param_for_white_kernel_in_sum(kernel, kernel_str=""):
    """Locate a WhiteKernel inside (nested) Sum kernels; returns (present, param_name).

    Same contract as skopt's ``_param_for_white_kernel_in_Sum`` imported at
    ``bask/bayesgpr.py:9-11`` and used at ``:328-333``.
    """
    if kernel_str != "":
        kernel_str = kernel_str + "__"
    if isinstance(kernel, Sum):
        for param, child in kernel.get_params(deep=False).items():
            if isinstance(child, WhiteKernel):
                return True, kernel_str + param
            present, child_str = param_for_white_kernel_in_sum(child, kernel_str + param)
            if present:
                return True, child_str
    return False, "_"


def _stationary_name(k):
    if isinstance(k, Matern):  # NB: sklearn's Matern subclasses RBF -- test it first
        nu = float(k.nu)
        for val, name in ((0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52")):
            if nu == val:
                return name
        if np.isinf(nu):
            return "rbf"
        raise NotImplementedError(f"Matern nu={nu} has no device kernel (supported: 0.5, 1.5, 2.5, inf)")
    if isinstance(k, RBF):
        return "rbf"
    return None


TREE_STACK, TREE_MAXMET, TREE_MAXINS, TREE_MAXIMM, TREE_MAXP, TREE_MAXD = 8, 4, 32, 8, 256, 32  # csrc/bgp_tree.h
TM_ISO, TM_ARD, TM_EUCL, TM_DOT = range(4)
(TO_CONST, TO_WHITE, TO_RBF, TO_M12, TO_M32, TO_M52, TO_RQ, TO_ESS, TO_DOT, TO_ADD, TO_MUL, TO_POW) = range(12)


class TreeProgram:
    """A kernel expression tree compiled for the device (``csrc/bgp_tree.hip``): ``ops`` (int32: the metric
    table and the postfix instructions, ``include/bgp.h``), ``imm`` (the exponents of ``Exponentiation``), ``P`` parameter slots and
    ``depth``, the deepest the value stack gets.  ``params`` maps theta to the slots."""

    def __init__(self, ops, imm, theta_index, fixed, white_slots, n_theta, depth):
        self.ops = np.ascontiguousarray(ops, dtype=np.int32)
        self.imm = np.ascontiguousarray(imm, dtype=np.float64)
        self._theta_index = np.asarray(theta_index, dtype=np.int64)  # per slot: where in theta, or -1 for a fixed value
        self._fixed = np.asarray(fixed, dtype=np.float64)            # per slot: the fixed log value
        self._white_slots = list(white_slots)  # slots of the WhiteKernel that param_for_white_kernel_in_sum finds
        self.P, self.n_theta, self.depth = len(self._fixed), n_theta, depth

    def params(self, thetas, noise_zero=False):
        """(B, p) or (p,) theta -> (B, P) log-space parameter rows: free entries gathered from theta, fixed ones filled in.
        ``noise_zero``: the white level ``noise_set_to_zero`` drops is -inf (``_posterior._with_white_zeroed``, vectorised)."""
        T = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        if T.shape[1] != self.n_theta:
            raise ValueError(f"theta has {T.shape[1]} entries, kernel has {self.n_theta} free hyper-parameters")
        out = np.empty((T.shape[0], self.P))
        free = self._theta_index >= 0
        out[:, free] = T[:, self._theta_index[free]]
        out[:, ~free] = self._fixed[~free]
        if noise_zero:
            out[:, self._white_slots] = -np.inf
        return out


def compile_tree(kernel, d):
    """``kernel`` as a ``TreeProgram`` for inputs of ``d`` columns, or None when a node has no device form (Matern with a general
    nu, a kernel class the device does not know), d > 32, the tree needs a deeper stack than ``TREE_STACK`` or more metrics,
    instructions, immediates or slots than the device program holds.  Leaves that read the same length-scale entries of theta (or
    the same fixed values) share one scaled squared distance of the metric table."""
    from sklearn.gaussian_process.kernels import DotProduct, Exponentiation, ExpSineSquared, RationalQuadratic

    if not 1 <= d <= TREE_MAXD:
        return None
    theta_index, fixed, metrics, met_keys, ins, imm, slots_of = [], [], [], {}, [], [], {}
    cursor = [0]

    def alloc(leaf):
        """name -> first slot of every hyper-parameter of a leaf, in theta order (``Kernel.theta``: the non-fixed ones in
        ``hyperparameters`` order)."""
        out = {}
        for hp in leaf.hyperparameters:
            with np.errstate(divide="ignore"):
                val = np.log(np.atleast_1d(np.asarray(getattr(leaf, hp.name), dtype=np.float64)))
            out[hp.name] = (len(fixed), len(val))
            for v in val:
                theta_index.append(-1 if hp.fixed else cursor[0])
                fixed.append(v)
                cursor[0] += 0 if hp.fixed else 1
        slots_of[id(leaf)] = out
        return out

    def metric(kind, slot=0, width=0):
        idx = tuple(theta_index[slot : slot + width])
        key = (kind, idx if all(i >= 0 for i in idx) else tuple(fixed[slot : slot + width]))
        if key not in met_keys:
            met_keys[key] = len(metrics)
            metrics.append((kind, slot))
        return met_keys[key]

    def emit(k):
        """Append the postfix code of ``k``; returns the stack depth it needs."""
        if isinstance(k, (Sum, Product)):
            d1 = emit(k.k1)
            d2 = emit(k.k2)
            ins.append((TO_ADD if isinstance(k, Sum) else TO_MUL, 0, 0, 0))
            return max(d1, 1 + d2)
        if isinstance(k, Exponentiation):
            d1 = emit(k.kernel)
            imm.append(float(k.exponent))
            ins.append((TO_POW, len(imm) - 1, 0, 0))
            return d1
        if not isinstance(k, (ConstantKernel, WhiteKernel, RBF, RationalQuadratic, ExpSineSquared, DotProduct)):
            raise NotImplementedError(type(k).__name__)
        s = alloc(k)
        if isinstance(k, ConstantKernel):
            ins.append((TO_CONST, s["constant_value"][0], 0, 0))
        elif isinstance(k, WhiteKernel):
            ins.append((TO_WHITE, s["noise_level"][0], 0, 0))
        elif isinstance(k, DotProduct):
            ins.append((TO_DOT, metric(TM_DOT), s["sigma_0"][0], 0))
        elif isinstance(k, ExpSineSquared):
            ins.append((TO_ESS, metric(TM_EUCL), s["length_scale"][0], s["periodicity"][0]))
        else:
            slot, width = s["length_scale"]
            if width not in (1, d):
                raise NotImplementedError(f"anisotropic length scale has {width} entries but X has {d} columns")
            m = metric(TM_ARD if width > 1 else TM_ISO, slot, width)
            if isinstance(k, RationalQuadratic):
                ins.append((TO_RQ, m, s["alpha"][0], 0))
            else:
                name = _stationary_name(k)  # (raises for a general nu)
                ins.append(({"rbf": TO_RBF, "matern12": TO_M12, "matern32": TO_M32, "matern52": TO_M52}[name], m, 0, 0))
        return 1

    try:
        depth = emit(kernel)
    except NotImplementedError:
        return None
    if (depth > TREE_STACK or len(metrics) > TREE_MAXMET or len(ins) > TREE_MAXINS or len(imm) > TREE_MAXIMM
            or len(fixed) > TREE_MAXP):
        return None
    white = kernel if isinstance(kernel, WhiteKernel) else None
    present, name = param_for_white_kernel_in_sum(kernel)
    if present:
        white = kernel
        for part in name.split("__"):
            white = getattr(white, part)
    white_slots = [slots_of[id(white)]["noise_level"][0]] if white is not None else []
    ops = [len(metrics), len(ins)] + [v for mt in metrics for v in mt] + [v for i in ins for v in i]
    return TreeProgram(ops, imm, theta_index, fixed, white_slots, cursor[0], depth)


class GramPlan:
    """A kernel expression tree without a canonical device form.  With a ``program`` (``compile_tree``) the device evaluates the
    tree itself (``bgp_tree.hip``); without one its matrices are evaluated on the host with the scikit-learn kernel object (what
    the reference does for every kernel, ``sklearn/_gpr.py:582``) and handed to the device.  Either way the device does everything
    behind the matrices.  ``why`` keeps the reason the canonical analysis gave."""

    generic = True
    form, stationary = "product", "matern52"  # (what the device context is created with; its Gram build is never used)

    def __init__(self, n_theta, why, program=None):
        self.n_theta = n_theta
        self.why = why
        self.program = program

    def canonical(self, theta, d):
        raise NotImplementedError("this kernel has no canonical device form (%s): its matrices come from the host" % self.why)


class KernelPlan:
    """theta (p,) of one kernel expression tree  <->  canonical h (d+2,)."""

    generic = False

    def __init__(self, form, stationary, const, ell, white, n_theta, ard):
        self.form = form  # "product" | "sum"
        self.stationary = stationary
        # each of const / white: ("free", theta_index) | ("fixed", log_value) | ("absent", log_value)
        # ell: ("free", [theta indices]) | ("fixed", log_values array)
        self.const, self.ell, self.white = const, ell, white
        self.n_theta = n_theta
        self.ard = ard
        # theta IS the canonical vector already (every component free, anisotropic length scales, theta order = h order: the
        # reference's default kernel, bask/utils.py:144-150 + WhiteKernel): the sampler's per-half-step mapping is a no-op
        self._identity_d = None
        if const[0] == "free" and white[0] == "free" and ell[0] == "free" and len(ell[1]) > 1:
            idx = [const[1]] + list(ell[1]) + [white[1]]
            if idx == list(range(n_theta)):
                self._identity_d = len(ell[1])

    def canonical(self, theta, d):
        """(B, p) or (p,) theta -> (B, d+2) canonical vectors."""
        T = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if T.shape[1] != self.n_theta:
            raise ValueError(f"theta has {T.shape[1]} entries, kernel has {self.n_theta} free hyper-parameters")
        if self._identity_d == d:
            return np.ascontiguousarray(T)
        B = T.shape[0]
        H = np.empty((B, d + 2))
        kind, v = self.const
        H[:, 0] = T[:, v] if kind == "free" else v
        kind, v = self.ell
        if kind == "free":
            if len(v) == 1:
                H[:, 1 : d + 1] = T[:, v[0]][:, None]
            else:
                if len(v) != d:
                    raise ValueError(f"anisotropic length scale has {len(v)} entries but X has {d} columns")
                H[:, 1 : d + 1] = T[:, v]
        else:
            v = np.asarray(v, dtype=np.float64)
            if v.size not in (1, d):
                raise ValueError(f"anisotropic length scale has {v.size} entries but X has {d} columns")
            H[:, 1 : d + 1] = v
        kind, v = self.white
        H[:, d + 1] = T[:, v] if kind == "free" else v
        return H

    def grad_to_theta(self, G, d):
        """Chain rule: dLML/dh (B, d+2) -> dLML/dtheta (B, p) (fixed entries dropped, isotropic
        length scale = sum over the replicated columns)."""
        G = np.atleast_2d(G)
        out = np.zeros((G.shape[0], self.n_theta))
        if self.const[0] == "free":
            out[:, self.const[1]] += G[:, 0]
        if self.ell[0] == "free":
            idx = self.ell[1]
            if len(idx) == 1:
                out[:, idx[0]] += G[:, 1 : d + 1].sum(axis=1)
            else:
                out[:, idx] += G[:, 1 : d + 1]
        if self.white[0] == "free":
            out[:, self.white[1]] += G[:, d + 1]
        return out

    def jacobian(self, d):
        """dh / dtheta (d + 2, p): the linear map behind ``canonical`` (``grad_to_theta`` is its transpose applied to a gradient)."""
        J = np.zeros((d + 2, self.n_theta))
        if self.const[0] == "free":
            J[0, self.const[1]] = 1.0
        if self.ell[0] == "free":
            idx = self.ell[1]
            if len(idx) == 1:
                J[1 : d + 1, idx[0]] = 1.0
            else:
                J[np.arange(1, d + 1), idx] = 1.0
        if self.white[0] == "free":
            J[d + 1, self.white[1]] = 1.0
        return J

    def hess_to_theta(self, Hc, d):
        """d2LML / dh2 (d + 2, d + 2) -> d2LML / dtheta2 (p, p): ``J^T Hc J`` (isotropic length scales sum over the replicated rows
        and columns, fixed entries drop out; the map is linear, so no gradient term enters)."""
        J = self.jacobian(d)
        return J.T @ np.asarray(Hc, dtype=np.float64) @ J


def _flatten(kernel, cls):
    if isinstance(kernel, cls):
        return _flatten(kernel.k1, cls) + _flatten(kernel.k2, cls)
    return [kernel]


def _leaves_in_theta_order(kernel, start=0):
    """Leaves of the tree in ``KernelOperator.theta`` order (k1 then k2, kernels.py:747) with the
    index of their first free hyper-parameter in theta."""
    if isinstance(kernel, (Sum, Product)):
        left, nxt = _leaves_in_theta_order(kernel.k1, start)
        right, nxt = _leaves_in_theta_order(kernel.k2, nxt)
        return left + right, nxt
    n_free = int(kernel.n_dims)
    return [(kernel, start, n_free)], start + n_free


def analyse_kernel(kernel, strict=False, d=None):
    """Analyse a kernel expression tree: a ``KernelPlan`` for the canonical forms (device Gram build), a ``GramPlan``
    for every other tree scikit-learn can evaluate (``bask/bayesgpr.py:148-159`` accepts any kernel) -- with the input
    dimension ``d`` given, its ``program`` is the tree compiled for the device where ``compile_tree`` covers it.
    ``strict=True`` raises ``NotImplementedError`` instead of returning a ``GramPlan``."""
    if not isinstance(kernel, Kernel):
        raise TypeError(f"expected a scikit-learn kernel object, got {type(kernel)}")
    try:
        return _analyse_canonical(kernel)
    except NotImplementedError as exc:
        if strict:
            raise
        with np.errstate(divide="ignore"):
            return GramPlan(len(kernel.theta), str(exc), None if d is None else compile_tree(kernel, int(d)))


def _analyse_canonical(kernel):
    with np.errstate(divide="ignore"):  # a zeroed WhiteKernel has theta = log(0)
        leaves, n_theta = _leaves_in_theta_order(kernel)
    index_of = {id(k): (i0, nf) for k, i0, nf in leaves}

    def slot(k):
        i0, nf = index_of[id(k)]
        return i0, nf

    terms = _flatten(kernel, Sum)
    white = ("absent", -np.inf)
    const_add = None
    stat_term = None
    for t in terms:
        if isinstance(t, WhiteKernel):
            if white[0] != "absent":
                raise NotImplementedError("more than one WhiteKernel in the kernel")
            i0, nf = slot(t)
            white = ("free", i0) if nf == 1 else ("fixed", float(np.log(t.noise_level)) if t.noise_level > 0 else -np.inf)
        elif isinstance(t, ConstantKernel):
            if const_add is not None:
                raise NotImplementedError("more than one additive ConstantKernel")
            const_add = t
        else:
            if stat_term is not None:
                raise NotImplementedError(f"more than one non-constant term in the sum: {kernel}")
            stat_term = t
    if stat_term is None:
        raise NotImplementedError(f"kernel has no stationary (RBF/Matern) component: {kernel}")

    factors = _flatten(stat_term, Product)
    const_mul = None
    stat = None
    for f in factors:
        if isinstance(f, ConstantKernel):
            if const_mul is not None:
                raise NotImplementedError("more than one multiplicative ConstantKernel")
            const_mul = f
        elif _stationary_name(f) is not None:
            if stat is not None:
                raise NotImplementedError("product of two stationary kernels is not supported")
            stat = f
        else:
            raise NotImplementedError(f"unsupported kernel component {type(f).__name__} in {kernel}")
    if stat is None:
        raise NotImplementedError(f"kernel has no stationary (RBF/Matern) component: {kernel}")
    if const_mul is not None and const_add is not None:
        raise NotImplementedError("kernel with both a multiplicative and an additive constant is not supported")

    def const_slot(ck):
        i0, nf = slot(ck)
        return ("free", i0) if nf == 1 else ("fixed", float(np.log(ck.constant_value)))

    if const_add is not None:
        form, const = "sum", const_slot(const_add)
    elif const_mul is not None:
        form, const = "product", const_slot(const_mul)
    else:
        form, const = "product", ("absent", 0.0)  # c = 1

    i0, nf = slot(stat)
    ard = bool(stat.anisotropic)
    if nf > 0:
        ell = ("free", list(range(i0, i0 + nf)))
    else:
        ell = ("fixed", np.log(np.atleast_1d(np.asarray(stat.length_scale, dtype=np.float64))))
    return KernelPlan(form, _stationary_name(stat), const, ell, white, n_theta, ard)
