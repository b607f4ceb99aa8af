"""No GPU: the long-double reference of tests/test_gpu_dense_factor.py against mpmath at 50 digits on a sample of each matrix set,
and the exactness the verdict tests rely on (L·diag(d)·Lᵀ has pivots exactly d)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_reference as R  # noqa: E402

mp = pytest.importorskip("mpmath")


def _mpf(v):
    p, q = v.as_integer_ratio()
    return mp.mpf(p) / q


def _mp_solve(A, b):
    with mp.workdps(50):
        x = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix(b.tolist()))
        return [x[i] for i in range(len(b))]


@pytest.mark.parametrize("kind", ["graded", "band"])
@pytest.mark.parametrize("kappa", [1e2, 1e8, 1e14])
def test_long_double_reference_against_mpmath(kind, kappa):
    R.check_longdouble()
    rng = np.random.default_rng(int(np.log10(kappa)) + (kind == "band") * 100)
    n = 24
    A = R.graded_spd(rng, 2, n, kappa) if kind == "graded" else R.band_spd(rng, 2, n, 5, 4, kappa)
    b = rng.standard_normal((2, n))
    x = R.ref_solve(A, b)
    kap = R.cond2(A)
    assert np.all(kap < 1e3 * kappa)
    for i in range(2):
        xm = _mp_solve(A[i], b[i])
        scale = max(abs(v) for v in xm)
        with mp.workdps(50):
            err = max(abs(_mpf(x[i, j]) - xm[j]) for j in range(n))
        # the reference's own error (κ · n · 2⁻⁶³ at most) far below what the kernels are held to (c · n · κ · 2⁻⁵³)
        assert err <= kap[i] * n * 2.0 ** -63 * scale, (kind, kappa, float(err / scale))
        # and in long double itself (the residual with the exact A), far inside double precision
        res = np.abs(A[i].astype(R.LD) @ x[i] - b[i].astype(R.LD)).max()
        assert res <= 64 * n * 2.0 ** -63 * (np.abs(A[i]).sum(axis=1).max() * np.abs(x[i]).max() + np.abs(b[i]).max())


def test_ldl_pivots_are_exact():
    rng = np.random.default_rng(5)
    for w, b in ((32, 0), (5, 4)):
        for special in (0.0, 2.0 ** -1000, 2.0 ** -1040, np.nextafter(1e300, 0.0)):
            A = R.ldl(rng, 32, w, b, special_k=9, special=special)
            # elimination in double: every pivot is exactly a power of 4, and the special one reaches step 9 as it is
            M = A.copy()
            piv = []
            for k in range(32):
                piv.append(M[k, k])
                if M[k, k] != 0:
                    f = M[k + 1:, k] / M[k, k]
                    M[k + 1:, k + 1:] -= np.outer(f, M[k, k + 1:])
            piv = np.array(piv)
            assert piv[9] == special or (special == 0.0 and piv[9] == 0.0)
            others = np.delete(piv, 9)
            assert np.all(np.log2(others) % 2 == 0), others
            assert np.all(np.isfinite(A))
            assert np.array_equal(A, A.T)
            # structural zeros outside the band stay exact zeros
            assert np.all(A[~(R.in_band(32, w, b) | R.in_band(32, w, b).T | np.eye(32, dtype=bool))] == 0.0)


def test_verdict_rule():
    f64, f32 = np.float64, np.float32
    assert R.expected_bad(0.0, 3, 31, f64) and R.expected_bad(-0.0, 3, 31, f64) and R.expected_bad(-1.0, 3, 31, f64)
    assert R.expected_bad(np.nan, 3, 31, f64) and R.expected_bad(np.inf, 3, 31, f64) and R.expected_bad(1e300, 3, 31, f64)
    assert not R.expected_bad(np.nextafter(1e300, 0.0), 3, 31, f64)
    assert not R.expected_bad(2.0 ** -1000, 3, 31, f64)  # 1/p = 2^1000: finite, above huge
    assert R.expected_bad(2.0 ** -1040, 3, 31, f64) and not R.expected_bad(2.0 ** -1040, 31, 31, f64)
    assert R.expected_bad(2.0 ** -1000, 3, 31, f32) and R.expected_bad(np.nextafter(1e300, 0.0), 3, 31, f32)
    assert R.expected_bad(None, 31, 31, f64)
