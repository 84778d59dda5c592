"""The three pairs of bivariate normal clouds behind the decision tests of erpl_mc_compare (1500 against 1000 points), with
their frozen seeds: shared by tests/test_compare_abi.py, where the yardstick alone decides them, and tests/test_gpu_compare.py."""
import numpy as np

DECISION_P = 999
DECISION_SEED = 11          # of the permutations
DRAW_SEED = 3           # of the clouds


def law(name, m_a=1500, m_b=1000):
    """(xa, ya, xb, yb).  'same': one law, unit normal; 'shift': the mean of B's x moved by 0.3 sigma; 'corr': the same
    marginals, correlation + 0.5 in A and - 0.5 in B."""
    rng = np.random.default_rng(DRAW_SEED)
    za, zb = rng.standard_normal((2, m_a)), rng.standard_normal((2, m_b))
    rho_a, rho_b = (0.5, -0.5) if name == "corr" else (0.0, 0.0)
    xa, ya = za[0], rho_a * za[0] + np.sqrt(1.0 - rho_a * rho_a) * za[1]
    xb, yb = zb[0], rho_b * zb[0] + np.sqrt(1.0 - rho_b * rho_b) * zb[1]
    if name == "shift":
        xb = xb + 0.3
    return xa, ya, xb, yb
