"""``kernels.compile_tree`` on the host: what it refuses, what it accepts, ``params()`` against ``clone_with_theta``, and the
long-double reference of tests/_treeref.py against scikit-learn itself (the reference is the same function)."""
import numpy as np
import pytest
from sklearn.gaussian_process import kernels as sk

from _treeref import tree_ref


@pytest.fixture(scope="module")
def K():
    import bayes_skopt_amd as bask

    return bask.kernels


def _right_nested(leaves):
    k = sk.RBF(1.0)
    for _ in range(leaves - 1):
        k = sk.Sum(sk.ConstantKernel(0.5), k)
    return k


TREES = [
    sk.Matern(0.4, nu=2.5) * sk.RBF(0.7) + sk.WhiteKernel(0.05),
    sk.Matern(0.3, nu=2.5) + sk.Matern(1.1, nu=1.5),
    sk.ConstantKernel(0.8) * sk.RationalQuadratic(0.5, alpha=1.3) + sk.WhiteKernel(0.03),
    sk.Exponentiation(sk.RBF(0.8), 2) * sk.DotProduct(0.5),
    sk.ExpSineSquared(0.9, periodicity=0.7) + sk.Matern([0.5, 0.6, 0.7], nu=0.5) * sk.ConstantKernel(2.0, "fixed"),
    sk.Matern(0.5, nu=np.inf) + sk.WhiteKernel(0.1, "fixed"),
    _right_nested(8),
]


def test_compile_tree_refuses_and_accepts(K):
    for bad, d in ((sk.Matern(nu=0.7), 3), (sk.RBF() * sk.RBF(), 33), (_right_nested(9), 3), (sk.RBF([1.0, 2.0]), 3)):
        assert K.compile_tree(bad, d) is None
    for k in TREES:
        prog = K.compile_tree(k, 3)
        assert prog is not None and prog.depth <= 8 and prog.n_theta == len(k.theta) and prog.ops.dtype == np.int32
        plan = K.analyse_kernel(k, d=3)
        if plan.generic:  # (a canonical tree keeps its KernelPlan)
            assert plan.program is not None and K.analyse_kernel(k).program is None
    assert K.compile_tree(_right_nested(8), 3).depth == 8
    shared = K.compile_tree(sk.Matern([0.4, 0.5], "fixed", nu=2.5) * sk.RBF([0.4, 0.5], "fixed"), 2)
    assert shared.ops[0] == 1  # one metric for both leaves


def _slots(prog, kernel):
    """The log-space values ``params`` must produce, read off the kernel object leaf by leaf in slot order."""
    if isinstance(kernel, (sk.Sum, sk.Product)):
        return _slots(prog, kernel.k1) + _slots(prog, kernel.k2)
    if isinstance(kernel, sk.Exponentiation):
        return _slots(prog, kernel.kernel)
    with np.errstate(divide="ignore"):
        return [v for hp in kernel.hyperparameters for v in np.log(np.atleast_1d(getattr(kernel, hp.name)))]


@pytest.mark.parametrize("k", TREES, ids=[str(i) for i in range(len(TREES))])
def test_params_reproduce_clone_with_theta(K, k):
    prog = K.compile_tree(k, 3)
    T = k.theta + 0.3 * np.random.RandomState(0).randn(4, len(k.theta))
    Pm = prog.params(T)
    assert Pm.shape == (4, prog.P)
    for b, t in enumerate(T):
        np.testing.assert_allclose(Pm[b], _slots(prog, k.clone_with_theta(t)), rtol=1e-15, atol=1e-15)
    present, name = K.param_for_white_kernel_in_sum(k)
    Pz = prog.params(T, noise_zero=True)
    assert np.isinf(Pz).sum() == (4 if present else 0) and np.array_equal(Pz[np.isfinite(Pz)], Pm[np.isfinite(Pz)])
    if present:  # a -inf white level in theta passes through as it is
        kz = k.clone_with_theta(T[0])
        kz.set_params(**{name: sk.WhiteKernel(noise_level=0.0)})
        with np.errstate(divide="ignore"):
            if len(kz.theta) == prog.n_theta:
                np.testing.assert_allclose(prog.params(kz.theta), Pz[:1], rtol=1e-15, atol=1e-15)  # (theta is re-logged)


@pytest.mark.parametrize("k", TREES, ids=[str(i) for i in range(len(TREES))])
def test_long_double_reference_is_scikit_learns_function(k):
    rng = np.random.RandomState(1)
    X, Y = rng.uniform(size=(23, 3)), rng.uniform(size=(11, 3))
    X[5] = X[2]
    for args in ((X,), (X, Y)):
        ref, got = tree_ref(k, *args), k(*args)
        np.testing.assert_allclose(got, ref.astype(np.float64), rtol=64 * np.finfo(np.float64).eps, atol=1e-15)
