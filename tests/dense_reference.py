"""The high-precision reference and the matrix sets of tests/test_gpu_dense_factor.py (and of its CPU check,
tests/test_dense_reference.py): batched elimination in np.longdouble, SPD matrices graded in condition, band-profiled ones, and
L·diag(d)·Lᵀ matrices whose pivots are exactly d."""
import numpy as np

LD = np.longdouble
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
HUGE = {np.float64: 1e300, np.float32: 1e30}  # fx_wave.h: Lim<T>::huge()


def check_longdouble():
    assert np.finfo(LD).nmant >= 63, "the reference needs an 80-bit (or wider) long double"


def ref_solve(A, b):
    """x = A⁻¹ b for a batch of SPD matrices, Gaussian elimination without pivoting in long double (the matrices are SPD, so no
    pivot is needed; with 64 mantissa bits the reference's own error stays 2¹¹ below the kernels' u at any κ tested)."""
    M = np.array(A, dtype=LD)
    y = np.array(b, dtype=LD)
    n = M.shape[-1]
    for k in range(n - 1):
        f = M[:, k + 1:, k] / M[:, k, k][:, None]
        M[:, k + 1:, k + 1:] -= f[:, :, None] * M[:, None, k, k + 1:]
        y[:, k + 1:] -= f * y[:, k][:, None]
    x = np.zeros_like(y)
    for k in range(n - 1, -1, -1):
        x[:, k] = (y[:, k] - np.einsum("bj,bj->b", M[:, k, k + 1:], x[:, k + 1:])) / M[:, k, k]
    return x


def symmetric(A):
    """The lower triangle mirrored: exactly symmetric, as the kernels read it (a packed triangle)."""
    low = np.tril(A)
    return low + np.swapaxes(np.tril(A, -1), -1, -2)


def graded_spd(rng, count, n, kappa):
    """JᵀJ + λI with J = diag(s) Vᵀ (V a random orthogonal matrix, s² geometric from 1 down to 1/κ) and λ = 1/κ · 1e-3:
    condition about κ, of the form the LM step factors."""
    out = np.empty((count, n, n))
    for i in range(count):
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        s2 = np.geomspace(1.0, 1.0 / kappa, n) if n > 1 else np.ones(1)
        out[i] = (V * s2) @ V.T + (1e-3 / kappa) * np.eye(n)
    return symmetric(out)


def band_spd(rng, count, n, w, b, kappa):
    """B Bᵀ with B = diag(g) (I + E): E strictly lower of the band profile (row i: columns i - w ... i - 1, every column for the
    last b rows), each row's entries of total size ½ at most, so that I + E is well conditioned, and g geometric from 1 down to
    κ^-½ in random order: condition about κ. The Cholesky factor is B up to rounding, its rows reach the band edge
    (E[i, i - w] != 0), and A's envelope is the factor's, so a band build holds it."""
    out = np.empty((count, n, n))
    for t in range(count):
        E = np.zeros((n, n))
        for i in range(1, n):
            j0 = 0 if i >= n - b else max(0, i - w)
            E[i, j0:i] = rng.uniform(0.5, 1.0, i - j0) * rng.choice([-1.0, 1.0], i - j0) * (0.5 / (i - j0))
        g = rng.permutation(np.geomspace(1.0, kappa ** -0.5, n))
        Bm = g[:, None] * (np.eye(n) + E)
        out[t] = Bm @ Bm.T
    return symmetric(out)


def in_band(n, w, b):
    """mask of the factor's possible non-zeros below the diagonal (RBand: i - j <= w or i >= n - b)"""
    i, j = np.indices((n, n))
    return (j < i) & ((i - j <= w) | (i >= n - b))


def ldl(rng, n, w, b, special_k=None, special=0.0):
    """A = L diag(d) Lᵀ, L unit lower with entries in {0, ±½, ±1} inside the band, d powers of 4: every pivot of the factor is
    exactly d (the arithmetic stays exact). special_k: that step's row and column of L are cleared and its pivot is `special`, so
    the pivot reaches the factor exactly whatever it is (0, NaN, a denormal ...), and the other entries stay finite."""
    L = np.where(in_band(n, w, b), rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (n, n)), 0.0)
    d = 4.0 ** rng.integers(-2, 3, n)
    if special_k is not None:
        L[special_k, :] = 0.0
        L[:, special_k] = 0.0
        d[special_k] = 1.0
    L[np.arange(n), np.arange(n)] = 1.0
    A = symmetric((L * d) @ L.T)
    if special_k is not None:
        A[special_k, :] = 0.0
        A[:, special_k] = 0.0
        A[special_k, special_k] = special
    return A


def expected_bad(special, k, last, dtype):
    """THE verdict rule, for every build: the factor says singular when a pivot p (in the build's type) is not in (0, huge), or
    when 1/p overflows to +inf at a step that is not the last one (the dense factor's next pivot is then NaN or -inf; a band
    factor checks 1/p itself). `special` None: a NaN or inf off the diagonal, always bad."""
    if special is None:
        return True
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        p = dtype(special)
        if not (p > 0 and p < dtype(HUGE[dtype])):
            return True
        return bool(k < last and np.isinf(dtype(1) / p))


def backward_error(A, x, b):
    """‖A x̂ - b‖∞ / (‖A‖∞ ‖x̂‖∞ + ‖b‖∞), per matrix, in long double"""
    Al, xl, bl = A.astype(LD), x.astype(LD), b.astype(LD)
    r = np.einsum("bij,bj->bi", Al, xl) - bl
    nA = np.abs(Al).sum(axis=2).max(axis=1)
    return (np.abs(r).max(axis=1) / (nA * np.abs(xl).max(axis=1) + np.abs(bl).max(axis=1))).astype(np.float64)


def forward_error(x, xref):
    xl = x.astype(LD)
    return (np.abs(xl - xref).max(axis=1) / np.abs(xref).max(axis=1)).astype(np.float64)


def cond2(A):
    ev = np.linalg.eigvalsh(A)
    return ev[:, -1] / np.maximum(ev[:, 0], np.finfo(np.float64).tiny)
