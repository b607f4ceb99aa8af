"""A context keeps state from one call to the next: the sparse path's plans per structure (fx_ctx::plan_for, eight of them),
freed device blocks, the zero-copy block and the pinned staging of small one-shot calls, a resident batch's plans. None of it
may show in a result. Every test here makes its own contexts and compares a call on a context with history, bit for bit,
with the same call on a FRESH context: a new one with the same settings, used for that one call only. The oracle is the
absolute check where it is affordable, with the sparse path's bars (the oracle's accepted / trial counts and exit code, its
scale, positions within 1e-8 of it)."""
import ctypes as C

import numpy as np
import pytest

import fiksi_amd
from fiksi_amd import abi, workloads
from helpers import random_big_sketch

pytestmark = pytest.mark.gpu


def _call(c, b, opts=None, register=False):
    """fx_system_solve_batch on copies of the value arrays; register: those copies and the results page-locked first."""
    from fiksi_amd._lib import check, lib

    a = abi.normalize_batch({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()})
    res = np.zeros(len(a["var_off"]) - 1, dtype=abi.RESULT_DTYPE)
    o = opts if opts is not None else abi.solving_opts()
    locked = [a["vars"], a["expr_param"], res]
    if register:
        c.host_register(*locked)
    try:
        check(lib.fx_system_solve_batch(c.handle, C.byref(abi.as_struct(a)), C.byref(o), res.ctypes.data), "fx_system_solve_batch")
    finally:
        if register:
            c.host_unregister(*locked)
    return a["vars"], res


def _apply(c, settings):
    for name, args in settings:
        getattr(c, name)(*args)


def _fresh(b, opts=None, settings=()):
    with fiksi_amd.Context(0) as c:
        _apply(c, settings)
        return _call(c, b, opts)


def _same(got, want, what):
    """Every variable and every field of every result record, bit for bit."""
    (v, r), (v0, r0) = got, want
    assert v.shape == v0.shape and len(r) == len(r0), what
    bad = np.nonzero(v.view(np.uint64) != v0.view(np.uint64))[0]
    assert not len(bad), f"{what}: {len(bad)} variables differ, first at {bad[0]}: {v[bad[0]]!r} != {v0[bad[0]]!r}"
    for f in r.dtype.names:
        x, y = r[f], r0[f]
        bad = np.nonzero(x.view(np.uint64) != y.view(np.uint64) if x.dtype.kind == "f" else x != y)[0]
        assert not len(bad), f"{what}: result field {f} differs for System {bad[0]}: {x[bad[0]]!r} != {y[bad[0]]!r}"


def _at(b, s):
    return int(b["var_off"][s]), int(b["var_off"][s + 1])


def _like_oracle(v, r, s, v0, v1, vo, ro, what, flat=None):
    """System s of a call (variables v0:v1) against the oracle's solve of that System alone (vo, ro[0]). flat = (oracle, the
    one-System batch): a sketch free to move as a whole (no fixed point), solved as one SinglePass block — the residuals
    compared instead of the positions, with the bar of helpers.compare_outcomes for Systems on the oracle's path."""
    for f in ("accepted", "trials", "exit", "ncomp"):
        assert r[f][s] == ro[f][0], f"{what}: System {s} {f} {r[f][s]} != the oracle's {ro[f][0]}"
    assert r["scale"][s] == ro["scale"][0], what
    if flat is None:
        err = float(np.max(np.abs(v[v0:v1] - vo)))
        assert err < 1e-8 * max(1.0, float(ro["scale"][0])), f"{what}: System {s} positions {err:.3g} from the oracle's"
    else:
        oracle, b = flat
        res, res_o = oracle.residuals_batch(b, v[v0:v1]), oracle.residuals_batch(b, vo)
        err = float(np.max(np.abs(np.abs(res) - np.abs(res_o))))
        assert err <= 1e-7 * max(1.0, float(ro["scale"][0])) + 1e-4 * np.sqrt(ro["sse"][0]), f"{what}: System {s} residuals {err:.3g} from the oracle's"


def _oracle(oracle, b, opts):
    """The oracle's solve of a one-System batch in the mode `opts` asks for."""
    o = opts or {}
    if o.get("decomposer") == 1:
        return oracle.solve_single_pass_batch(b, lbfgs=o.get("optimizer") == 1)
    return oracle.solve_batch(b, mode=7 if o.get("optimizer") == 1 else 3)


# ---- a. the reproducer: one large structure at the same index behind Systems of other sizes ------------------------------
#
# On one context: [quad, B], [ring16, B], the same again, [quad, B, B, B], [ring16, B, B, B]. Before the fix the second and
# the fifth call found the offset table of the call before it (same index list) and solved B at the quadrilateral's offsets:
# wrong variables for B and for the ring. The prefixes only grow from one call to the next (variables and expressions), so
# a stale table still points inside the batch.

_B = {
    # name: (B, solving options, context settings, oracle: None / "positions" / "residuals")
    "walkers": (lambda: random_big_sketch(9301, 150).flatten(), {}, (("set_sparse_fronts", (False,)),), "positions"),
    "fronts_solo": (lambda: workloads.hinged_triangles(1, 64), {}, (), "positions"),
    "parts_top": (lambda: workloads.large_sketch(1500), {}, (), None),
    "single_pass": (lambda: workloads.ring_chords(1, n_points=100), {"decomposer": 1}, (), "residuals"),  # (one block of 200 columns)
    "lbfgs": (lambda: workloads.hinged_triangles(1, 64), {"optimizer": 1}, (), "positions"),
    "qr_refined": (lambda: random_big_sketch(9302, 140).flatten(), {"solver": 2}, (), "positions"),  # (FX_STEP_QR: the refined step here)
    "team_65_128": (lambda: workloads.hinged_triangles(1, 16), {}, (("set_wide_routing", (0,)),), "positions"),
}


def _prefix_sequence(units):
    """The five calls of the reproducer around `units` (the large Systems of one call, in order)."""
    quad, ring = workloads.quadrilateral(), workloads.ring16(1, seed0=77)
    assert int(ring["var_off"][-1]) >= int(quad["var_off"][-1]) and int(ring["expr_off"][-1]) >= int(quad["expr_off"][-1])
    return [workloads.concat([quad] + units), workloads.concat([ring] + units), workloads.concat([ring] + units),
            workloads.concat([quad] + units * 3), workloads.concat([ring] + units * 3)]


def _run_sequence(calls, opts, settings, what):
    o = abi.solving_opts(**opts)
    with fiksi_amd.Context(0) as c:
        _apply(c, settings)
        out = []
        for i, b in enumerate(calls):
            got = _call(c, b, o)
            _same(got, _fresh(b, o, settings), f"{what}, call {i + 1}")
            out.append(got)
    return out


@pytest.mark.parametrize("case", list(_B))
def test_a_large_system_behind_different_prefixes(fiksi, oracle, case):
    make, opts, settings, bar = _B[case]
    B = make()
    calls = _prefix_sequence([B])
    out = _run_sequence(calls, opts, settings, case)
    if bar:
        vo, ro = _oracle(oracle, B, opts)
        for i, (b, (v, r)) in enumerate(zip(calls, out)):
            for s in range(1, len(r)):
                _like_oracle(v, r, s, *_at(b, s), vo, ro, f"{case}, call {i + 1}", flat=(oracle, B) if bar == "residuals" else None)


def test_two_large_structures_per_call_on_one_host_thread(fiksi, oracle):
    """With one host thread every group of large Systems is solved on the context's stream and may return with its launches in
    flight (stay_async): both structures' offset tables are kept with their plans."""
    B1, B2 = workloads.hinged_triangles(1, 64), random_big_sketch(9303, 130).flatten()
    calls = _prefix_sequence([B1, B2])
    out = _run_sequence(calls, {}, (("set_host_threads", (1,)),), "two structures, one host thread")
    for B, first in ((B1, 1), (B2, 2)):
        vo, ro = oracle.solve_batch(B, mode=3)
        for i, (b, (v, r)) in enumerate(zip(calls, out)):
            for s in range(first, len(r), 2):
                _like_oracle(v, r, s, *_at(b, s), vo, ro, f"two structures, call {i + 1}")


# ---- b. the plans' device memory stays bounded when a structure's position changes -----------------------------------------

def test_plan_memory_stays_bounded_when_positions_change(fiksi):
    small, B = workloads.quadrilateral(), workloads.hinged_triangles(1, 64)
    layouts = [workloads.concat([small, B]), workloads.concat([small, small, B])]
    others = [workloads.large_sketch(60 + 5 * k, seed=200 + k) for k in range(10)]  # ten structures > the eight kept plans
    with fiksi_amd.Context(0) as c:
        for round_ in range(2):
            for i in range(4):
                _call(c, layouts[i % 2])
            settled = c.plan_bytes()
            assert settled > 0
            for i in range(500):
                _call(c, layouts[i % 2])
            assert c.plan_bytes() == settled, f"round {round_}: {c.plan_bytes() - settled} bytes more after 500 calls"
            for o in others:  # B's plan is evicted: the next round plans it anew
                _call(c, o)


# ---- c. a used context gives a fresh context's bits ----------------------------------------------------------------------

_SMALL = [lambda: workloads.quadrilateral(), lambda: workloads.quadrilateral(consistent=False), lambda: workloads.ring16(1, seed0=31),
          lambda: workloads.hinged_triangles(1, 4)]
_LARGE = {
    "h64": lambda: workloads.hinged_triangles(1, 64),
    "h40": lambda: workloads.hinged_triangles(1, 40),
    "h24": lambda: workloads.hinged_triangles(1, 24),
    "h16": lambda: workloads.hinged_triangles(1, 16),
    "rb0": lambda: random_big_sketch(9400, 110).flatten(),
    "rb1": lambda: random_big_sketch(9401, 125).flatten(),
    "rb2": lambda: random_big_sketch(9402, 140).flatten(),
    "ls150": lambda: workloads.large_sketch(150, seed=3),
    "ls90": lambda: workloads.large_sketch(90, seed=4),
    "ls400": lambda: workloads.large_sketch(400, seed=5),
}
_OPTS = [{}, {}, {"decomposer": 1}, {"optimizer": 1}, {"solver": 2}, {"solver": 1}]
_SETTINGS = {
    "set_sparse_fronts": [(True,), (False,)],
    "set_host_threads": [(1,), (8,)],
    "set_ladder": [(True,), (False,)],
    "set_presort": [(True,), (False,)],
    "set_wide_routing": [(-1,), (0,), (1,)],
}
SEEDS = [20261016, 7, 1234]


class _Menu:
    """The parts of the sequence's batches, made once; a batch is named by its layout, a tuple of part names."""

    def __init__(self):
        self.parts = {f"s{i}": f() for i, f in enumerate(_SMALL)}
        self.parts.update({k: f() for k, f in _LARGE.items()})
        self.batches = {}

    def part(self, name):
        if name not in self.parts:  # ("ring:<n>:<seed>": a few thousand ring16 sketches)
            _, n, seed = name.split(":")
            self.parts[name] = workloads.ring16(int(n), seed0=int(seed))
        return self.parts[name]

    def batch(self, layout):
        if layout not in self.batches:
            self.batches[layout] = workloads.concat([self.part(p) for p in layout])
        return self.batches[layout]


@pytest.mark.parametrize("seed", SEEDS)
def test_a_used_context_gives_a_fresh_context_s_bits(fiksi, oracle, seed):
    rng = np.random.default_rng(seed)
    menu = _Menu()
    fresh = {}
    settings = {}   # the setters called on the used context so far, their last arguments
    opts = {}
    first_default = {}  # large structure -> its variables and result from a call with the default options
    log = []

    def state():
        return tuple(sorted(settings.items())), tuple(sorted(opts.items()))

    def want(layout, params=None):
        """The fresh context's result of the batch `layout` (expr_param and vars replaced by `params`) in the current state."""
        key = (layout, None if params is None else params[0], state())
        if key not in fresh:
            b = menu.batch(layout)
            if params is not None:
                b = dict(b, expr_param=params[1], vars=params[2])
            fresh[key] = _fresh(b, abi.solving_opts(**opts), tuple(sorted(settings.items())))
        return fresh[key]

    def one_shot(c, layout, register=False):
        got = _call(c, menu.batch(layout), abi.solving_opts(**opts), register=register)
        what = f"seed {seed}, step {len(log)}: {log[-1]}"
        _same(got, want(layout), what)
        if not opts:
            b = menu.batch(layout)
            for s, p in enumerate(layout):
                if p in _LARGE and p not in first_default:
                    v0, v1 = _at(b, s)
                    first_default[p] = (got[0][v0:v1].copy(), got[1][s:s + 1].copy(), what)

    def large_layout(n_large, n_prefix):
        names = [str(x) for x in rng.choice(list(_LARGE), size=n_large, replace=True)]
        prefix = [f"s{i}" for i in rng.integers(0, len(_SMALL), size=n_prefix)]
        layout = prefix + names
        if rng.random() < 0.3:
            rng.shuffle(layout)
        return tuple(layout)

    with fiksi_amd.Context(0) as c:
        for step in range(48):
            kind = rng.choice(["zero_copy", "pinned", "large", "large", "large", "many_large", "resident", "register", "opts", "setting"],
                              p=[0.1, 0.06, 0.14, 0.14, 0.14, 0.06, 0.08, 0.06, 0.11, 0.11])
            if kind == "zero_copy":
                layout = tuple(f"s{i}" for i in rng.integers(0, len(_SMALL), size=int(rng.integers(1, 6))))
                log.append(f"one-shot {layout}")
                one_shot(c, layout)
            elif kind == "pinned":
                layout = (f"ring:{int(rng.integers(1500, 3000))}:{int(rng.integers(0, 3)) * 4000}",) + tuple(
                    f"s{i}" for i in rng.integers(0, len(_SMALL), size=int(rng.integers(0, 3))))
                log.append(f"one-shot {layout}")
                one_shot(c, layout)
            elif kind == "large":
                layout = large_layout(int(rng.integers(1, 4)), int(rng.integers(0, 4)))
                log.append(f"one-shot {layout}")
                one_shot(c, layout)
            elif kind == "many_large":  # more structures than the context keeps plans: eviction
                names = list(_LARGE)
                rng.shuffle(names)
                layout = tuple([f"s{int(rng.integers(0, len(_SMALL)))}"] + names[: int(rng.integers(9, len(names) + 1))])
                log.append(f"one-shot {layout}")
                one_shot(c, layout)
            elif kind == "register":
                layout = (f"s{int(rng.integers(0, len(_SMALL)))}",) + large_layout(1, 0)
                log.append(f"registered one-shot {layout}")
                one_shot(c, layout, register=True)
            elif kind == "resident":
                layout = large_layout(int(rng.integers(1, 3)), int(rng.integers(1, 3)))
                b = menu.batch(layout)
                o = abi.solving_opts(**opts)
                log.append(f"resident {layout}")
                what = f"seed {seed}, step {len(log)}: {log[-1]}"
                db = c.upload(b)
                try:
                    db.system_solve(o)
                    got = (db.get_vars(), db.get_results())
                    _same(got, want(layout), what + ", first solve")
                    log.append(f"one-shot {layout[::-1]} between resident solves")
                    one_shot(c, layout[::-1])
                    params = b["expr_param"] * np.where(b["expr_tag"] == abi.POINT_POINT_DISTANCE, 1.02, 1.0)
                    db.set_params(params)
                    db.set_vars(got[0])
                    for k in range(2):  # (the second: the batch's plans and offset tables as the first left them)
                        db.system_solve(o)
                        _same((db.get_vars(), db.get_results()), want(layout, (f"step {step}", params, got[0])), what + f", solve {k + 2}")
                        log.append(f"one-shot {layout} between resident solves")
                        one_shot(c, layout)
                finally:
                    db.free()
            elif kind == "opts":
                opts = dict(_OPTS[int(rng.integers(0, len(_OPTS)))])
                log.append(f"options {opts}")
            else:
                name = list(_SETTINGS)[int(rng.integers(0, len(_SETTINGS)))]
                args = _SETTINGS[name][int(rng.integers(0, len(_SETTINGS[name])))]
                settings[name] = args
                getattr(c, name)(*args)
                log.append(f"{name}{args}")
    # the absolute check: one solve of every large structure that came up, against the oracle
    for name, (v, r, what) in first_default.items():
        if name == "ls400":
            continue  # (800 variables: the oracle's sparse QR takes long; its neighbours of this family are checked)
        vo, ro = oracle.solve_batch(menu.parts[name], mode=3)
        _like_oracle(v, r, 0, 0, len(v), vo, ro, f"{name} ({what})")
    assert len(first_default) >= 5, f"seed {seed}: the sequence solved only {sorted(first_default)} with the default options"
