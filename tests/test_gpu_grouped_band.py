"""The band-factor builds of the one-structure kernel (fx_grouped_band.hip) on the GPU: every bit of the dense factor's solve (a
context created under FIKSI_AMD_GC_BAND=0), for each build, at a band edge and just past it, and on a batch whose trials meet
singular factors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_grouped_band import distance_sketch, strip  # noqa: E402


@pytest.fixture(scope="module")
def ctx_dense(fiksi):
    """A context whose one-structure build always factors densely (FIKSI_AMD_GC_BAND is read when a context is created)."""
    old = os.environ.get("FIKSI_AMD_GC_BAND")
    os.environ["FIKSI_AMD_GC_BAND"] = "0"
    try:
        c = fiksi.Context(0)
    finally:
        if old is None:
            del os.environ["FIKSI_AMD_GC_BAND"]
        else:
            os.environ["FIKSI_AMD_GC_BAND"] = old
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _solve(ctx, b, o, want_factor):
    db = ctx.upload(b)
    try:
        assert db.grouped_build(o) == 1
        assert db.grouped_factor(o) == want_factor, (db.grouped_factor(o), want_factor)
        db.system_solve(o)
        return db.get_vars(), db.get_results()
    finally:
        db.free()


def _cases():
    from fiksi_amd import workloads

    b = workloads.ring16(2000, seed0=77)
    b["var_fixed"][:] = np.tile(np.r_[np.zeros(16, np.uint8), np.ones(2, np.uint8), np.zeros(14, np.uint8)], 2000)
    return {"ring16": (lambda: workloads.ring16(4099), {}, 2),
            "ring16_inconsistent": (lambda: workloads.ring16(3000, inconsistent=True), {}, 2),
            "ring16_trial_cap": (lambda: workloads.ring16(2000), {"max_trials": 21}, 2),
            "ring16_fixed_gauge": (lambda: workloads.ring16(3001, fix_gauge=True), {}, 1),
            "ring16_point8_fixed": (lambda: b, {}, 3),
            "strip16_at_the_edge": (lambda: distance_sketch(1500, 16, strip(16)), {}, 1),
            "strip16_past_the_edge": (lambda: distance_sketch(1500, 16, strip(16, [(2, 5)])), {}, 0),
            # trials on a matrix that is singular but for lambda: a lambda of 1e-300 leaves pivots of round-off size and sign,
            # so trials end LC_SINGULAR (lambda x singular_factor) until lambda has grown
            "ring16_near_singular": (lambda: workloads.ring16(2000), {"lambda0": 1e-300}, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_cases()))
def test_same_bits_as_the_dense_factor(fiksi, ctx, ctx_dense, case):
    from fiksi_amd import abi

    make, kw, want = _cases()[case]
    b = make()
    o = abi.solving_opts(**kw)
    v1, r1 = _solve(ctx, b, o, want)
    v0, r0 = _solve(ctx_dense, b, o, 0)
    assert np.array_equal(_bits(v1), _bits(v0)), case
    assert r1.tobytes() == r0.tobytes(), case
    # the one-shot path takes the same kernels
    v2, r2 = ctx.system_solve_batch(b, o)
    assert np.array_equal(_bits(v2), _bits(v0)) and r2.tobytes() == r0.tobytes(), case


@pytest.mark.gpu
def test_ring16_takes_the_band_build_and_the_switch_keeps_it_dense(fiksi, ctx, ctx_dense):
    from fiksi_amd import abi, workloads

    for c, want in ((ctx, 2), (ctx_dense, 0)):
        db = c.upload(workloads.ring16(1000))
        try:
            assert db.grouped_build() == 1 and db.grouped_factor() == want
            assert db.grouped_factor(abi.solving_opts(f32=True)) == -1  # (the f32 kernel factors densely)
        finally:
            db.free()
