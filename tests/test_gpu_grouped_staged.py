"""The staged set-up and closing check of the one-structure kernel's two-column f64 build (fx_grouped_c.hip: gc_stage_kernel,
gc_close_kernel) on the GPU: every bit of the solve in which the kernel sets up and checks each System itself (a context created
under FIKSI_AMD_GC_STAGED=0) — one structure and two interleaved structures, with and without the longest-first order, with the
lambda ladder off, at the tail and everywhere, under the trial cap — and the scale of the reference."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def ctx_inline(fiksi):
    """A context whose one-structure kernel sets up and checks every System itself (FIKSI_AMD_GC_STAGED is read when a context
    is created)."""
    old = os.environ.get("FIKSI_AMD_GC_STAGED")
    os.environ["FIKSI_AMD_GC_STAGED"] = "0"
    try:
        c = fiksi.Context(0)
    finally:
        if old is None:
            del os.environ["FIKSI_AMD_GC_STAGED"]
        else:
            os.environ["FIKSI_AMD_GC_STAGED"] = old
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cases():
    from fiksi_amd import workloads

    return {"ring16": (lambda: workloads.ring16(4099, seed0=31), {}, 1),
            "ring16_fix_gauge": (lambda: workloads.ring16(3001, fix_gauge=True), {}, 1),
            "ring16_inconsistent": (lambda: workloads.ring16(3000, inconsistent=True), {}, 1),
            "ring16_trial_cap": (lambda: workloads.ring16(2500), {"max_trials": 21}, 1),
            "ring16_no_perturbation": (lambda: workloads.ring16(2100), {"perturb": False}, 1),
            "ring16_singular_trials": (lambda: workloads.ring16(2100), {"lambda0": 1e-300}, 1),
            "two_interleaved_structures": (lambda: workloads.ring16_two_structures(6000), {}, 3)}


def _resident(ctx, b, o, build, staged):
    db = ctx.upload(b)
    try:
        assert db.grouped_build(o) == build
        assert db.grouped_staged(o) == staged, (db.grouped_staged(o), staged)
        db.system_solve(o)
        db.system_solve(o)  # (a second solve on the same staging area)
        return db.get_vars(), db.get_results()
    finally:
        db.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_cases()))
def test_same_bits_as_the_inline_set_up(fiksi, ctx, ctx_inline, case):
    from fiksi_amd import abi

    make, kw, build = _cases()[case]
    b = make()
    o = abi.solving_opts(**kw)
    v0, r0 = _resident(ctx_inline, b, o, build, 0)
    try:
        for ladder in ((True, 0xFFFFFFFF, 8, True), (False, 0, 16, False), (True, 1 << 30, 0, True)):
            ctx.set_ladder(*ladder)
            for presort in (True, False):
                ctx.set_presort(presort, 1)
                v1, r1 = _resident(ctx, b, o, build, 1)
                assert np.array_equal(_bits(v1), _bits(v0)), (case, ladder, presort)
                assert r1.tobytes() == r0.tobytes(), (case, ladder, presort)
        # the one-shot path stages too
        v2, r2 = ctx.system_solve_batch(b, o)
        assert np.array_equal(_bits(v2), _bits(v0)) and r2.tobytes() == r0.tobytes(), case
    finally:
        ctx.set_ladder()
        ctx.set_presort(True, 8192)


@pytest.mark.gpu
def test_which_solves_stage(fiksi, ctx, ctx_inline):
    from fiksi_amd import abi, workloads

    db = ctx.upload(workloads.ring16(4096))
    try:
        assert db.grouped_staged() == 1
        assert db.grouped_staged(abi.solving_opts(f32=True)) == 0  # (f32 sets up inside the kernel)
        assert db.grouped_staged(abi.solving_opts(decomposer=1)) == -1  # (not the one-structure build)
    finally:
        db.free()
    db = ctx.upload(workloads.ring16(1000))  # (below the size the two extra passes pay off from)
    try:
        assert db.grouped_build() == 1 and db.grouped_staged() == 0
    finally:
        db.free()
    db = ctx_inline.upload(workloads.ring16(4096))
    try:
        assert db.grouped_build() == 1 and db.grouped_staged() == 0
    finally:
        db.free()


@pytest.mark.gpu
def test_staged_set_up_and_closing_check_match_the_oracle(fiksi, ctx, oracle):
    """The staged passes against the CPU oracle: the scale bit for bit and the solves it starts agreeing as the kernel's own set-up
    does (System::solve semantics, smoke()); the closing check against the oracle's residuals of the solved variables."""
    from fiksi_amd import workloads

    b = workloads.ring16(2048, seed0=5)
    db = ctx.upload(b)
    try:
        assert db.grouped_staged() == 1
        db.system_solve()
        v, res = db.get_vars(), db.get_results()
    finally:
        db.free()
    _, res_o = oracle.solve_batch(b, mode=3, nthreads=8)
    assert np.array_equal(_bits(res["scale"]), _bits(res_o["scale"]))
    assert np.mean(res["accepted"] == res_o["accepted"]) >= 0.95
    ok = np.abs(res["sse"] - res_o["sse"]) <= 1e-9 + 1e-5 * np.abs(res_o["sse"])
    assert np.mean(ok) >= 0.95
    bs = dict(b)
    bs["vars"] = np.asarray(v, dtype=np.float64)
    r_o, _ = oracle.eval_batch(bs)
    off = np.asarray(b["expr_off"], dtype=np.int64)
    sse_u = np.add.reduceat(np.asarray(r_o, dtype=np.float64) ** 2, off[:-1])
    assert np.allclose(res["sse_unscaled"], sse_u, rtol=1e-6, atol=1e-15)
