"""The LM step's register Cholesky, build by build (fx_debug_dense_solve: every instantiation the kernels use, fiksi_amd/abi.py:
DENSE_VARIANTS), against a long-double reference (tests/dense_reference.py; itself checked against mpmath by
tests/test_dense_reference.py).

  * accuracy: SPD matrices JᵀJ + λI graded to κ = 1e2 ... 1e14 (f32: 1e2 ... 1e5), band-profiled ones for the band builds:
    backward error ≤ C·n·u, forward error ≤ C·n·κ·u;
  * the SinglePass builds (BOUNDED) on every size 1 ... N in the four rows of a wavefront, kmax = ceil8(largest), and the wide
    kernel's second block (nb < 64);
  * verdicts, exactly: L·diag(d)·Lᵀ with one special pivot (0, -0, -1, NaN, +inf, 1e300, the double below it, 2⁻¹⁰⁰⁰, 2⁻¹⁰⁴⁰) or a
    non-finite entry off the diagonal at step K, in each of the four rows: `bad` follows dense_reference.expected_bad, the rows
    next to a bad one solve bit for bit as in a wavefront without it, and the band builds give the dense build's bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

C_BACKWARD = 4.0  # backward error ≤ C·n·u
C_FORWARD = 4.0  # forward error ≤ C·n·κ·u

SPECIALS = [0.0, -0.0, -1.0, np.nan, np.inf, 1e300, float(np.nextafter(1e300, 0.0)), 2.0 ** -1000, 2.0 ** -1040, "nan_off", "inf_off"]
STEPS = (0, 1, 7, 8, 15, 16, 17, 31)

WORST = {}  # variant name -> worst (backward, forward) error-to-bound ratio, printed at the end of the module


@pytest.fixture(scope="module")
def variants(fiksi):
    return fiksi.abi.DENSE_VARIANTS


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst error / bound per variant (backward, forward):")
        for k in sorted(WORST):
            print(f"  {k:36s} {WORST[k][0]:.3g} {WORST[k][1]:.3g}")


def _size(v):
    return v.n  # the size each variant factors (wide: 64, its first block)


def _round(v, a):
    return a.astype(np.float32).astype(np.float64) if v.dtype == np.float32 else a


def _accuracy(ctx, v, A, b, kmax=0, sizes=None):
    """Solve, compare with the reference; returns the worst ratios. sizes: the size of each matrix's real block (identity past it)."""
    A, b = _round(v, A), _round(v, b)
    x, bad = ctx.dense_solve(v.id, A, b, kmax)
    n = b.shape[1]
    u = R.U[v.dtype]
    kap = R.cond2(A)
    nn = np.full(len(b), n) if sizes is None else np.asarray(sizes)
    # a factor may break down where κ·n·u nears 1 (f64 near 1e14 at 64 columns): such matrices may say `bad`, no others may
    may_fail = kap * nn * u > 1e-2
    assert not np.any(bad & ~may_fail), (v.name, kap[bad & ~may_fail])
    assert np.count_nonzero(bad) <= len(bad) // 2, v.name
    ok = ~bad
    xref = R.ref_solve(A[ok], b[ok])
    be = R.backward_error(A[ok], x[ok], b[ok]) / (C_BACKWARD * nn[ok] * u)
    fe = R.forward_error(x[ok], xref) / (C_FORWARD * nn[ok] * kap[ok] * u)
    assert np.all(np.isfinite(x[ok])), v.name
    wb, wf = float(be.max()), float(fe.max())
    old = WORST.get(v.name, (0.0, 0.0))
    WORST[v.name] = (max(old[0], wb), max(old[1], wf))
    assert wb <= 1.0, (v.name, "backward error / bound", wb)
    assert wf <= 1.0, (v.name, "forward error / bound", wf)


def _kappas(v):
    return (1e2, 1e4, 1e5) if v.dtype == np.float32 else (1e2, 1e6, 1e10, 1e14)


def test_accuracy_on_graded_spd_matrices(ctx, variants):
    rng = np.random.default_rng(1)
    for v in variants:
        n = _size(v)
        if v.kind == "rows" and v.w < v.n:
            continue  # the band builds take band-profiled matrices only (below)
        for kappa in _kappas(v):
            A = R.graded_spd(rng, 8, n, kappa)
            b = rng.standard_normal((8, n))
            _accuracy(ctx, v, A, b, kmax=n)


def test_accuracy_on_band_matrices(ctx, variants):
    """Band-profiled matrices whose every row reaches the band edge: the band builds, and the dense builds of the same size."""
    rng = np.random.default_rng(2)
    bands = sorted({(v.w, v.b) for v in variants if v.kind == "rows" and v.w < v.n})
    for w, bb in bands:
        for kappa in (1e2, 1e6, 1e10, 1e14):
            A = R.band_spd(rng, 8, 32, w, bb, kappa)
            b = rng.standard_normal((8, 32))
            for v in variants:
                if v.n == 32 and v.dtype == np.float64 and (v.w == 32 or (v.w, v.b) == (w, bb)) and v.kind != "wide":
                    _accuracy(ctx, v, A, b, kmax=32)


def test_bounded_every_size_in_one_wavefront(ctx, variants):
    """SinglePass: four Systems of sizes 1 ... N in the rows of one wavefront (identity past each), kmax = ceil8(largest)."""
    rng = np.random.default_rng(3)
    for v in variants:
        if not v.bounded:
            continue
        N = v.n
        kappa = 1e4 if v.dtype == np.float32 else 1e8
        sizes = list(range(1, N + 1))
        for w0 in range(0, N, 4):
            group = sizes[w0:w0 + 4]
            m = max(group)  # (the entry pads to N with the identity)
            A = np.zeros((len(group), m, m))
            b = np.zeros((len(group), m))
            for t, k in enumerate(group):
                A[t] = np.eye(m)
                A[t, :k, :k] = R.graded_spd(rng, 1, k, kappa)[0]
                b[t, :k] = rng.standard_normal(k)
            kmax = (max(group) + 7) // 8 * 8
            _accuracy(ctx, v, A, b, kmax=kmax, sizes=group)
            # the first k entries are the System's; the kernel skipped the blocks past kmax: the same x with kmax = N
            A2, b2 = _round(v, A), _round(v, b)
            x1, _ = ctx.dense_solve(v.id, A2, b2, kmax)
            x2, _ = ctx.dense_solve(v.id, A2, b2, N)
            for t, k in enumerate(group):
                assert np.array_equal(x1[t, :k], x2[t, :k]), (v.name, k)


def test_wide_second_block_below_64(ctx, variants):
    rng = np.random.default_rng(4)
    for v in variants:
        if v.kind != "wide":
            continue
        for nb in (1, 2, 17, 33, 63, 64):
            for kappa in (1e2, 1e10):
                A = R.graded_spd(rng, 4, nb, kappa)
                b = rng.standard_normal((4, nb))
                _accuracy(ctx, v, A, b)


def _special_matrix(rng, n, w, bb, k, s):
    if isinstance(s, str):  # a NaN or inf off the diagonal, inside the band, in row / column k
        A = R.ldl(rng, n, w, bb)
        i, j = (k + 1, k) if k + 1 < n else (k, k - 1)
        A[i, j] = A[j, i] = np.nan if s == "nan_off" else np.inf
        return A
    return R.ldl(rng, n, w, bb, special_k=k, special=s)


def _special_value(s):
    return None if isinstance(s, str) else s


def _verdict_batch(rng, v, n, w, bb):
    """per (special, K, row r): four matrices, row r special, the others good; plus the same four with row r good"""
    steps = sorted({k for k in STEPS if k < n} | {n - 1})
    per_wave = 4 if v.kind == "rows" else 1
    A, Aclean, meta = [], [], []
    for s in SPECIALS:
        for k in steps:
            if n == 1 and isinstance(s, str):
                continue
            for r in range(per_wave):
                good = [R.ldl(rng, n, w, bb) for _ in range(per_wave)]
                spec = _special_matrix(rng, n, w, bb, k, s)
                wave = list(good)
                wave[r] = spec
                A += wave
                Aclean += good
                meta.append((s, k, r))
    b = rng.choice([-1.0, -0.5, 0.5, 1.0], (len(A), n))
    return np.array(A), np.array(Aclean), b, meta, per_wave


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def test_verdicts_exactly_and_row_isolation(ctx, variants):
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        for v in variants:
            if v.kind == "wide":
                cases = [(64, 64, 0), (33, 33, 0)]
            elif v.kind == "rows" and v.w < v.n:
                cases = [(v.n, v.w, v.b)]
            else:
                cases = [(v.n, v.n, 0)]
            for n, w, bb in cases:
                A, Aclean, b, meta, pw = _verdict_batch(rng, v, n, w, bb)
                A, Aclean, b = _round(v, A), _round(v, Aclean), _round(v, b)
                kmax = n
                x, bad = ctx.dense_solve(v.id, A, b, kmax)
                xc, badc = ctx.dense_solve(v.id, Aclean, b, kmax)
                assert not badc.any(), (v.name, "a matrix with pivots that are powers of 4 said singular")
                for t, (s, k, r) in enumerate(meta):
                    i = pw * t + r
                    want = R.expected_bad(_special_value(s), k, n - 1, v.dtype)
                    assert bool(bad[i]) == want, (v.name, n, "special", s, "step", k, "row", r, "bad", bool(bad[i]))
                    for o in range(pw):
                        if o == r:
                            continue
                        j = pw * t + o
                        assert not bad[j], (v.name, "a good row next to a bad one said singular", s, k, r, o)
                        assert np.array_equal(_bits(x[j]), _bits(xc[j])), (v.name, "row isolation", s, k, r, o)


def test_band_builds_give_the_dense_bits_and_verdicts(ctx, variants):
    """same bits. The band builds against the dense two-column build (and the general build, and the one-column
    chol<32>) on the verdict matrices of each band, singular ones included: the same `bad`, the same x where it is not bad."""
    rng = np.random.default_rng(6)
    dense = [v for v in variants if v.n == 32 and v.dtype == np.float64 and v.kind in ("rows", "chol") and v.w == 32 and not v.bounded]
    assert len(dense) == 3
    with np.errstate(all="ignore"):
        for vb in variants:
            if not (vb.kind == "rows" and vb.w < vb.n):
                continue
            A, _, b, meta, _ = _verdict_batch(rng, vb, 32, vb.w, vb.b)
            xb, badb = ctx.dense_solve(vb.id, A, b, 32)
            for vd in dense:
                xd, badd = ctx.dense_solve(vd.id, A, b, 32)
                assert np.array_equal(badb, badd), (vb.name, vd.name, [meta[i // 4] for i in np.nonzero(badb != badd)[0][:4]])
                ok = ~badb
                if vd.kind == "chol":
                    # (the one-column build's broadcasts are v_readlane, not DPP: a NaN that an inf step makes may carry
                    # another sign there; the finite solutions carry the same bits)
                    ok &= np.isfinite(xd).all(axis=1)
                assert np.array_equal(_bits(xb[ok]), _bits(xd[ok])), (vb.name, vd.name)
