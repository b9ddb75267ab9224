"""The outlier data set of tests/test_gpu_cglm.py's robustness test, on the host (no GPU): by quadrature over the NumPy
models (tests/_cglm.py's student_t, tests/_glm_disp.py's normal) the robust fit holds the true slope 2 well inside 3 of
its posterior sd and the normal fit misses it by well over 3 of its own -- the data set separates the two by a wide
margin, whatever the sampler does."""
import math

import numpy as np

import _cglm as cg
import _glm_disp as gd


def _posterior(model, centre, half, k=(41, 41, 33)):
    """Mean and sd of (b_0, b_1, tau) by the midpoint rule on a grid of k points around `centre`."""
    g = [np.linspace(centre[i] - half[i], centre[i] + half[i], k[i]) for i in range(3)]
    G = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    lp = np.concatenate([model.logpdf(G[i:i + 20000]) for i in range(0, len(G), 20000)])
    w = np.exp(lp - lp.max())
    w /= w.sum()
    W = w.reshape(k)
    assert max(W[[0, -1]].max(), W[:, [0, -1]].max(), W[:, :, [0, -1]].max()) < 1e-7
    mean = w @ G
    return mean, np.sqrt(w @ (G - mean) ** 2)


def test_outlier_data_separates_robust_from_linear():
    x, y = cg.outlier_data()
    n = x.size
    assert n == 200 and np.sum(y - (1.0 + 2.0 * x) > 40.0) == 10         # 10 rows, 50 sd up
    mr, sr = _posterior(cg.ContGLMNumpy(x, y, "student_t", 2.5, (0.0, 2.5), True, df=4.0), (1.0, 2.0, 0.0), (0.6, 0.6, 0.5))
    A = np.column_stack([np.ones(n), x])
    b = np.linalg.lstsq(A, y, rcond=None)[0]
    s = float(np.std(y - A @ b))
    ml, sl = _posterior(gd.GLMDispNumpy(x, y, "normal", 2.5, (0.0, 2.5), True), (b[0], b[1], math.log(s)),
                        (7 * s / math.sqrt(n),) * 2 + (0.4,))
    print("robust slope", mr[1], sr[1], "linear slope", ml[1], sl[1])
    assert abs(mr[1] - 2.0) < 1.5 * sr[1] and sr[1] < 0.12               # 1.88 +- 0.09
    assert abs(ml[1] - 2.0) > 6.0 * sl[1] > 6.0 * sr[1]                  # 6.31 +- 0.65
