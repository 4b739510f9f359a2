"""The statement of the accuracy tests (tests/test_gpu_rk4_accuracy.py, tests/test_gpu_fbs_accuracy.py), in one place:

    err_gpu <= K * max(err_oracle, 8 eps),      eps = 2^-53,  K = 8

per output, over every trajectory of a run.  K and the floor are explained in tests/test_gpu_rk4_accuracy.py; neither is fitted
to a run."""
import numpy as np

from tests import rk4_twin as tw

K = 8.0
FLOOR = 8 * tw.EPS


def check_ratios(what, e, err_oracle, factor=None, subset=None):
    """e, err_oracle {output: [B]}: the errors of a run and of the oracle over the same trajectories.  `factor` [B]: a derived
    loss of the mapping per trajectory, the bound of trajectory b is then K * factor[b] * yardstick.  `subset` {output:
    positions}: outputs whose yardstick exists on some trajectories only are compared over exactly those.  Prints one
    ACCURACY line of ratios err / max(err_oracle, 8 eps) and asserts the bound; returns the ratios."""
    ratios, bad = {}, []
    for k, v in e.items():
        yard_all = err_oracle[k]
        if subset and k in subset:
            v, yard_all = v[subset[k]], yard_all[subset[k]]
        yard = max(float(np.max(yard_all)), FLOOR)
        ratios[k] = float(np.max(v)) / yard
        if not np.all(v <= K * yard * (1.0 if factor is None else factor)):
            bad.append((k, float(np.max(v)), yard))
    print("ACCURACY", what, " ".join(f"{k}={r:.2f}" for k, r in ratios.items()) +
          ("" if factor is None else f" (factor {np.min(factor):.0f}..{np.max(factor):.0f})"))
    assert not bad, (what, "err_gpu > K * max(err_oracle, 8 eps) for (output, err_gpu, yardstick):", bad)
    return ratios
