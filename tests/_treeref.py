"""A scikit-learn kernel tree evaluated in ``np.longdouble`` straight from the kernel object: the reference of the device kernel
programs (tests/test_gpu_tree.py) and of ``kernels.compile_tree`` (tests/test_cpu_tree_reference.py).  Recursion over Sum / Product /
Exponentiation, the closed forms of the leaves (sklearn/gaussian_process/kernels.py)."""
import numpy as np
from sklearn.gaussian_process import kernels as sk

LD = np.longdouble


def tree_ref(kernel, X, Y=None):
    """``kernel(X)`` (Y None: WhiteKernel on the diagonal) or ``kernel(X, Y)`` as a longdouble array."""
    if isinstance(kernel, sk.Sum):
        return tree_ref(kernel.k1, X, Y) + tree_ref(kernel.k2, X, Y)
    if isinstance(kernel, sk.Product):
        return tree_ref(kernel.k1, X, Y) * tree_ref(kernel.k2, X, Y)
    if isinstance(kernel, sk.Exponentiation):
        return tree_ref(kernel.kernel, X, Y) ** LD(kernel.exponent)
    A = np.asarray(X, dtype=LD)
    Bm = A if Y is None else np.asarray(Y, dtype=LD)
    shape = (A.shape[0], Bm.shape[0])
    if isinstance(kernel, sk.ConstantKernel):
        return np.full(shape, LD(kernel.constant_value))
    if isinstance(kernel, sk.WhiteKernel):
        return LD(kernel.noise_level) * np.eye(shape[0], dtype=LD) if Y is None else np.zeros(shape, dtype=LD)
    if isinstance(kernel, sk.DotProduct):
        return A @ Bm.T + LD(kernel.sigma_0) ** 2
    diff = A[:, None, :] - Bm[None, :, :]
    if isinstance(kernel, sk.ExpSineSquared):
        r = np.sqrt((diff * diff).sum(axis=2))
        s = np.sin(4 * np.arctan(LD(1)) * r / LD(kernel.periodicity)) / LD(kernel.length_scale)  # (pi in long double)
        return np.exp(-2 * s * s)
    diff = diff / np.asarray(kernel.length_scale, dtype=LD)
    r2 = (diff * diff).sum(axis=2)
    if isinstance(kernel, sk.RationalQuadratic):
        return (1 + r2 / (2 * LD(kernel.alpha))) ** (-LD(kernel.alpha))
    if isinstance(kernel, sk.Matern) and not np.isinf(kernel.nu):
        r = np.sqrt(r2)
        if kernel.nu == 0.5:
            return np.exp(-r)
        t = np.sqrt(LD(2 * kernel.nu)) * r
        if kernel.nu == 1.5:
            return (1 + t) * np.exp(-t)
        if kernel.nu == 2.5:
            return (1 + t + t * t / 3) * np.exp(-t)
        raise NotImplementedError("Matern nu=%r" % kernel.nu)
    if isinstance(kernel, sk.RBF):
        return np.exp(-r2 / 2)
    raise NotImplementedError(type(kernel).__name__)
