"""The host restatement of the joint batch selection (tests/_qselref.py) against the definition of
Monte-Carlo q-EI, its exact properties in fp64, and the case list of the device test.  No GPU."""
import math

import numpy as np
import pytest

import _pathref as PR
import _qselref as Q
from test_cpu_paths_reference import MOMENT_F, MOMENT_PATHS, MOMENT_SEED, moment_problem


def _draws(seed, P, m, twins=True):
    """A draw matrix with the features of a real one: correlated columns, a twin column, incumbents inside the range."""
    rng = np.random.RandomState(seed)
    base = rng.standard_normal((P, 3))
    F = base @ rng.standard_normal((3, m)) + 0.3 * rng.standard_normal((P, m))
    if twins and m >= 6:
        F[:, 4] = F[:, 1]
    inc = F.min(axis=1) + np.abs(rng.standard_normal(P))
    return F, inc


SHAPES = [(1, 1), (2, 6), (63, 17), (257, 40)]


@pytest.mark.parametrize("P,m", SHAPES)
def test_step_values_are_the_gain_of_the_definition(P, m):
    """a_j(i) = qei_mc(C + {i}) - qei_mc(C) at every step, for every candidate, within 2 (P + 2) eps64 mean_s(|c_s| + |F[s, i]|)."""
    F, inc = _draws(10 + P, P, m)
    forced = [m - 1] if m > 2 else []
    q = min(4, m - len(forced))
    picks, values = Q.select(F, inc, forced, q, "improvement")
    chosen, worst = list(forced), 0.0
    for j in range(q):
        base = Q.qei_mc(F, inc, chosen)
        c = np.minimum(inc, F[:, chosen].min(axis=1)) if chosen else inc
        for i in range(m):
            want = Q.qei_mc(F, inc, chosen + [i]) - base
            err, bound = abs(float(np.longdouble(values[j, i]) - want)), Q.definition_bound(F, c, i)
            worst = max(worst, err / bound)
            assert err <= bound, (j, i, err, bound)
        chosen.append(int(picks[j]))
    print("P = %d, m = %d: worst error / bound %.3f" % (P, m, worst))
    assert len(set(chosen)) == len(chosen)


@pytest.mark.parametrize("P,m", SHAPES[1:])
def test_values_never_increase_and_chosen_rows_and_twins_are_exactly_zero(P, m):
    F, inc = _draws(20 + P, P, m)
    q = min(6, m)
    picks, values = Q.select(F, inc, [], q, "improvement")
    assert np.all(values >= 0.0)
    assert np.all(values[1:] <= values[:-1])  # exactly: rounding is monotone and the order of the sum is fixed
    for j in range(q):
        assert np.all(values[j + 1 :, picks[j]] == 0.0)
    picks, values = Q.select(F, inc, [1], 3, "improvement")  # column 4 is a twin of the forced column 1
    assert np.all(values[:, 1] == 0.0) and np.all(values[:, 4] == 0.0)


def test_ties_go_to_the_lower_index():
    F, inc = _draws(5, 7, 9, twins=False)
    F[:, 6] = F[:, 2]
    F[:, 8] = F[:, 2]
    inc = F[:, 2] + 1.0  # columns 2, 6 and 8 gain 1 on every path
    F[:, [0, 1, 3, 4, 5, 7]] = inc[:, None] + 1.0  # ... and nobody else gains anything
    picks, values = Q.select(F, inc, [], 4, "improvement")
    assert values[0, 2] == values[0, 6] == values[0, 8] > 0.0
    assert list(picks) == [2, 0, 1, 3]  # after column 2 every value is exactly 0: the lowest indices left, in order
    assert np.all(values[1:] == 0.0)
    picks, _ = Q.select(F, inc, [0, 2], 3, "improvement")
    assert list(picks) == [1, 3, 4]
    picks, values = Q.select(F, inc, [], 9, "thompson")  # nine steps on seven paths: the path index wraps around
    assert picks[0] == 2 and picks[1] == 6 and picks[2] == 8
    assert np.array_equal(values[7], -F[0]) and np.array_equal(values[8], -F[1])
    assert sorted(picks) == list(range(9))


def test_a_scalar_incumbent_below_every_draw_gives_zeros_and_index_order():
    F, _ = _draws(6, 5, 11)
    picks, values = Q.select(F, np.full(5, F.min() - 1.0), [3], 10, "improvement")
    assert np.all(values == 0.0)
    assert list(picks) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]


def test_one_step_with_a_scalar_incumbent_is_closed_form_ei():
    """4096 restated paths of one GP (the ensemble of test_cpu_paths_reference.py): the step-0 values under a scalar incumbent
    agree with EI from the predictive mean and latent std within 5 Monte-Carlo standard errors (the project's bound for path
    moments), at every row."""
    from oracle import gp_oracle as O

    stationary, form = "matern52", "product"
    X, y, alpha, h, Xq = moment_problem(stationary, form)
    F = PR.moments_restated(X, y, alpha, h, stationary, form, Xq, MOMENT_PATHS, MOMENT_F, MOMENT_SEED)
    mean, std = O.predict(X, y, np.full(len(X), alpha), h, Xq, stationary, form, noise_zero=True)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    y_opt = float(np.median(mean))  # (an incumbent in the middle: some rows gain on most paths, some on few)
    _, values = Q.select(F, np.full(len(F), y_opt), [], 1, "improvement")
    z = (y_opt - mean) / std
    ei = (y_opt - mean) * 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0))) + std * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    se = np.maximum(0.0, y_opt - F).std(axis=0, ddof=1) / math.sqrt(len(F))
    dev = np.abs(values[0] - ei) / se
    print("worst deviation of Monte-Carlo EI from the closed form: %.2f standard errors" % dev.max())
    assert np.all(se > 0.0) and dev.max() <= 5.0, dev


def test_cases_cover_the_edges():
    get = lambda k: {c[k] for c in Q.CASES}  # noqa: E731
    assert get("m") >= {1, 2, 255, 256, 257, 513, Q.SEL_NT - 1, Q.SEL_NT, Q.SEL_NT + 1}
    assert get("P") >= {1, 2, 63, 64, 65, 257, Q.SEL_TC - 1, Q.SEL_TC, Q.SEL_TC + 1}
    assert get("n") == {1, 65} and get("d") == {1, 8, 32}
    assert {(c["stationary"], c["form"]) for c in Q.CASES} == {(s, f) for s in ("rbf", "matern52") for f in ("product", "sum")}
    for c in Q.CASES:
        pr = Q.problem(c["id"])
        assert pr["Xc"].shape == (c["m"], c["d"]) and pr["eps"].shape == (c["P"], c["n"])
