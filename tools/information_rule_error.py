"""What the Gauss-Hermite rule of bgp_info.hip costs in accuracy (CPU only): the rule restated in numpy against
adaptive quadrature (``scipy.integrate.quad`` per component, on +-40 sd with the other components' means as break points) of the
same integrals, over a family of two- and three-component mixtures that span what a chain produces -- equal rows; means apart by 0, 1,
4 and 20 sd; sd ratios 1, 2, 3, 10 and 1e3; weights from uniform to one row at 1e-6.  Prints the worst absolute error of the information,
in nats, per family member group and for Q = 8, 16, 32, 64."""
import itertools

import numpy as np
from scipy.integrate import quad
from scipy.special import logsumexp


RATIOS = (1.0, 2.0, 3.0, 10.0, 1e3)  # (2 and 3: where between 1 and 10 the rule starts to miss)


def by_rule(mu, sd, w, Q):
    t, om = np.polynomial.hermite.hermgauss(Q)
    L = np.log(w) - np.log(sd)
    y = mu[:, None] + np.sqrt(2.0) * sd[:, None] * t[None, :]
    lse = logsumexp(L[None, None, :] - 0.5 * ((y[:, :, None] - mu[None, None, :]) / sd[None, None, :]) ** 2, axis=2)
    g = L[:, None] - t[None, :] ** 2 - lse
    return float((w[:, None] * (g - np.log(w)[:, None]) * (om / np.sqrt(np.pi))[None, :]).sum())


def by_quad(mu, sd, w):
    L = np.log(w) - np.log(sd)
    total = 0.0
    for b in range(len(mu)):
        def f(y):
            own = -np.log(sd[b]) - 0.5 * ((y - mu[b]) / sd[b]) ** 2
            mix = logsumexp(L - 0.5 * ((y - mu) / sd) ** 2)
            return np.exp(own - 0.5 * np.log(2.0 * np.pi)) * (own - mix)
        lo, hi = mu[b] - 40.0 * sd[b], mu[b] + 40.0 * sd[b]
        pts = sorted({float(p) for c in range(len(mu)) for p in (mu[c] - 6 * sd[c], mu[c], mu[c] + 6 * sd[c]) if lo < p < hi})
        total += w[b] * quad(f, lo, hi, points=pts, limit=400, epsabs=1e-13, epsrel=1e-13)[0]
    return total


def main():
    worst = {}
    for B, gap, ratio, wmin in itertools.product((2, 3), (0.0, 1.0, 4.0, 20.0), RATIOS, (None, 1e-2, 1e-6)):
        sd = ratio ** (-np.arange(B) / (B - 1.0))  # the first row the widest
        mu = gap * sd.max() * np.arange(B)
        w = np.ones(B) if wmin is None else np.array([1.0] * (B - 1) + [wmin])
        w = w / w.sum()
        ref = by_quad(mu, sd, w)
        for Q in (8, 16, 32, 64):
            key = ("ratio %g" % ratio, Q)
            worst[key] = max(worst.get(key, 0.0), abs(by_rule(mu, sd, w, Q) - ref))
    for ratio in RATIOS:
        print("sd ratio %-5g worst |error| (nats): " % ratio + "  ".join("Q=%d %.2e" % (Q, worst[("ratio %g" % ratio, Q)]) for Q in (8, 16, 32, 64)))


if __name__ == "__main__":
    main()
