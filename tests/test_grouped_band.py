"""The band-factor builds of the one-structure kernel (fx_grouped_band.hip; fx_grouped_rows.h: RBand), CPU only: the host's row
profile of the Cholesky factor and its choice of build (fx_programs.cpp, through fx_gc_factor_profile) against a symbolic
Cholesky written here, and the ISA of the new object scanned for the DPP hazard of tests/test_dpp_hazards.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = [(5, 0), (5, 4), (5, 6)]  # fx_device.h: GC_BANDS, cheapest first
NVARS = {0: 2, 1: 4, 2: 6, 3: 6, 4: 6, 5: 5, 10: 7}  # fx_expr.h: tag_nvars (8 otherwise)
PPD = 1


def _expr_vars(tag, f):
    a, b, c, d = (int(x) for x in f)
    return [a, b if tag == 0 else a + 1, b, b + 1, c, c + 1, d, d + 1][:NVARS.get(tag, 8)]


def symbolic_profile(batch, n, system=0):
    """first[i] of the factor of Jt J over the free variables in ascending order, padded with identity columns to n (the
    build's 16, 32 or 48): a dense boolean elimination, fill included."""
    v0, v1 = int(batch["var_off"][system]), int(batch["var_off"][system + 1])
    e0, e1 = int(batch["expr_off"][system]), int(batch["expr_off"][system + 1])
    col = {}
    for i in range(v1 - v0):
        if not batch["var_fixed"][v0 + i]:
            col[i] = len(col)
    assert len(col) <= n
    m = np.eye(n, dtype=bool)
    for r in range(e0, e1):
        cs = [col[v] for v in _expr_vars(int(batch["expr_tag"][r]) & 0x7F, batch["expr_idx"][4 * r:4 * r + 4]) if v in col]
        for a in cs:
            for b in cs:
                m[a, b] = True
    for k in range(n):
        rows = np.nonzero(m[k + 1:, k])[0] + k + 1
        m[np.ix_(rows, rows)] = True
    return [int(np.nonzero(m[i, :i + 1])[0][0]) for i in range(n)]


def expected_band(first):
    if len(first) != 32:
        return 0
    for t, (w, b) in enumerate(BANDS):
        if all(i - first[i] <= w for i in range(32 - b)):
            return t + 1
    return 0


def distance_sketch(n_systems, n_points, pairs, fixed_points=(), seed=7):
    """n Systems of one structure: points on a jittered circle, a distance per pair (consistent targets)."""
    rng = np.random.default_rng(seed)
    P, m = n_points, len(pairs)
    ang = 2 * np.pi * np.arange(P) / P
    pts = np.stack([np.cos(ang), np.sin(ang)], -1)[None] * 10.0 + rng.uniform(-0.5, 0.5, (n_systems, P, 2))
    start = pts + rng.uniform(-0.2, 0.2, pts.shape)
    idx = np.zeros((n_systems, m, 4), dtype=np.uint32)
    par = np.zeros((n_systems, m))
    for r, (a, b) in enumerate(pairs):
        idx[:, r, 0], idx[:, r, 1] = 2 * a, 2 * b
        par[:, r] = np.linalg.norm(pts[:, a] - pts[:, b], axis=-1)
    fixed = np.zeros((n_systems, 2 * P), dtype=np.uint8)
    for p in fixed_points:
        fixed[:, 2 * p:2 * p + 2] = 1
        start[:, p] = pts[:, p]
    return {
        "var_off": (np.arange(n_systems + 1) * 2 * P).astype(np.uint32),
        "expr_off": (np.arange(n_systems + 1) * m).astype(np.uint32),
        "vars": start.reshape(-1).copy(),
        "var_fixed": fixed.reshape(-1),
        "expr_tag": np.full(n_systems * m, PPD, dtype=np.uint8),
        "expr_idx": idx.reshape(-1),
        "expr_param": par.reshape(-1),
        "var_comp": np.zeros(n_systems * 2 * P, dtype=np.uint16),
        "expr_comp": np.zeros(n_systems * m, dtype=np.uint16),
    }


def strip(n_points, extra=()):
    """A strip of triangles: distances (i, i + 1) and (i, i + 2) — exactly half-band 5 in the kernel's column order — plus `extra`."""
    return [(i, i + 1) for i in range(n_points - 1)] + [(i, i + 2) for i in range(n_points - 2)] + list(extra)


def _random_structure(rng):
    n_points = int(rng.integers(9, 17))
    pairs = {(i, i + 1) for i in range(n_points - 1)}
    kind = int(rng.integers(0, 3))
    if kind == 0:  # local chords only: a band
        for _ in range(int(rng.integers(0, 8))):
            a = int(rng.integers(0, n_points - 2))
            pairs.add((a, a + 2))
    elif kind == 1:  # a closed ring with local chords: band + border
        pairs.add((0, n_points - 1))
        for _ in range(int(rng.integers(0, 6))):
            a = int(rng.integers(0, n_points - 2))
            pairs.add((a, a + 2))
    else:  # anything
        for _ in range(int(rng.integers(1, 10))):
            a, b = sorted(int(x) for x in rng.choice(n_points, 2, replace=False))
            pairs.add((a, b))
    fixed = [int(rng.integers(0, n_points))] if rng.random() < 0.4 else []
    return distance_sketch(2, n_points, sorted(pairs), fixed, seed=int(rng.integers(0, 1 << 30)))


def _cases():
    from fiksi_amd import workloads

    out = [("ring16", workloads.ring16(2), 2), ("ring16_fixed_gauge", workloads.ring16(2, fix_gauge=True), 1),
           ("strip16", distance_sketch(2, 16, strip(16)), 1), ("strip16_past_the_edge", distance_sketch(2, 16, strip(16, [(2, 5)])), 0)]
    b = workloads.ring16(2)  # a ring whose free variables stop at 30: the border ends at row 29, two padding rows behind it
    b["var_fixed"][16:18] = 1
    out.append(("ring16_point8_fixed", b, 3))
    rng = np.random.default_rng(20261016)
    out += [("random%d" % k, _random_structure(rng), None) for k in range(20)]
    return out


def test_the_host_profile_and_band_choice_match_a_symbolic_cholesky(fiksi):
    from fiksi_amd import abi

    seen = set()
    for name, b, want in _cases():
        first, band = abi.gc_factor_profile(b)
        assert len(first) in (16, 32, 48), (name, len(first))
        ref = symbolic_profile(b, len(first))
        assert first == ref, (name, first, ref)
        assert band == expected_band(ref), (name, band, expected_band(ref))
        if want is not None:
            assert band == want, (name, band, want)
        seen.add(band)
    assert seen >= {0, 1, 2, 3}  # (every build, and the dense factor, chosen somewhere)


def _device_asm(tmp_path, name):
    src = os.path.join(ROOT, "fiksi_amd", "csrc", name + ".hip")
    out = tmp_path / (name + ".s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
           "-I", os.path.join(ROOT, "include"), src, "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=str(tmp_path), timeout=900)
    return out


def _per_kernel(path, op):
    counts, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            counts[cur] = 0
        elif cur and line.strip().startswith(op):
            counts[cur] += 1
    return counts


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_band_builds_have_no_dpp_hazard_and_fewer_updates(tmp_path):
    band = _device_asm(tmp_path, "fx_grouped_band")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_hazards.py"), str(band)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    dense = _per_kernel(_device_asm(tmp_path, "fx_grouped_c"), "v_fmac_f64_dpp")
    d = [v for k, v in dense.items() if "lm_solve_grouped_c_kernel" in k]
    assert len(d) == 1
    got = {k: v for k, v in _per_kernel(band, "v_fmac_f64_dpp").items() if "band_kernel" in k}
    assert len(got) == len(BANDS)
    # the factor's multiply-adds per trial: dense 856, (5, 0) 220, (5, 4) 378, (5, 6) 451; the substitutions are the same
    for (w, b), fewer in zip(BANDS, (636, 478, 405)):
        k = [v for n, v in got.items() if "ILi%dELi%dE" % (w, b) in n]
        assert k and d[0] - k[0] == fewer, ((w, b), d[0], k)
