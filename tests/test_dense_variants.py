"""No GPU: fx_debug_dense_solve's variant table (fx_debug_chol.hip, fiksi_amd/abi.py: DENSE_VARIANTS) holds every instantiation of
the LM step's register Cholesky that the kernels use — read off their call sites and launchers with a grep — and the two copies of
the table agree. A build added to a kernel without a variant here fails this test, so that tests/test_gpu_dense_factor.py sees it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fiksi_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _table():
    # abi.py's table without loading the library (a CPU box may have none built)
    src = open(os.path.join(ROOT, "fiksi_amd", "abi.py")).read()
    ns = {"np": np, "namedtuple": __import__("collections").namedtuple}
    exec(src[src.index("class DenseVariant"):src.index("_FIELDS = {")], ns)
    return ns["DENSE_VARIANTS"]


def _switch():
    """fx_debug_chol.hip's switch: id -> the tuple the variant stands for."""
    out = {}
    for m in re.finditer(r"case (\d+): return (rows|chol|wide)<([^>]*)>", _src("fx_debug_chol.hip")):
        args = [a.strip() for a in m.group(3).split(",")]
        out[int(m.group(1))] = (m.group(2), tuple(args))
    return out


def _key(v):
    t = "float" if v.dtype == np.float32 else "double"
    if v.kind == "rows":
        return ("rows", (str(v.n // 16), t, str(v.bounded).lower(), str(v.w), str(v.b), str(v.fwd).lower(),
                         "SITE_GENERAL" if v.site == "general" else "SITE_ONE"))
    if v.kind == "chol":
        return ("chol", (str(v.n), t))
    return ("wide", ("true" if v.site == "b2" else "false",))


def test_the_python_table_is_the_switch():
    table, sw = _table(), _switch()
    assert sorted(sw) == [v.id for v in table] == list(range(len(table)))
    for v in table:
        assert sw[v.id] == _key(v), (v.name, sw[v.id])
    assert len({v.name for v in table}) == len(table)


def _general_rows():
    """fx_grouped.hip: launch_grouped_t<NC, T[, PROF[, UNITS]]> -> (NC, T, BOUNDED = UNITS); PROF changes no arithmetic."""
    src = _src("fx_grouped.hip")
    assert "RBlock<NC, T, 0, UNITS>::template factor<false>(a, invd, acc, bad, hl, kmax);" in src
    assert "RBlock<NC, T, 0, UNITS>::forward(a, invd, acc, hl, kmax);" in src
    found = set()
    for m in re.finditer(r"launch_grouped_t<(\d), (float|double)(?:, (true|false))?(?:, (true|false))?>", src):
        found.add((int(m.group(1)), m.group(2), m.group(4) == "true"))
    return found


def _one_structure_rows():
    """fx_grouped_c.hip / fx_grouped_band.hip: grouped_c_body<NC, RC, T[, W, B[, STAGED]]>, the band kernels' <W, B>; FWD = NC == 2."""
    assert "constexpr bool FWD = NC == 2;" in _src("fx_grouped_c.h")
    assert "RBlock<NC, T, 0, false, W, B>::template factor<FWD>(a, invd, acc, bad, hl, N);" in _src("fx_grouped_c.h")
    found = set()
    for m in re.finditer(r"grouped_c_body<(\d), \d, (float|double)(?:, ([^,>]+), ([^,>]+))?", _src("fx_grouped_c.hip")):
        nc = int(m.group(1))
        w = eval(m.group(3).replace("RS", "16")) if m.group(3) else 16 * nc
        b = int(m.group(4)) if m.group(4) else 0
        found.add((nc, m.group(2), w, b))
    band = _src("fx_grouped_band.hip")
    assert "grouped_c_body<2, 2, double, W, B>" in band
    for m in re.finditer(r"lm_solve_grouped_c_band(?:_staged)?_kernel<(\d+), (\d+)>", band):
        found.add((2, "double", int(m.group(1)), int(m.group(2))))
    return found


def _chol_sizes():
    """fx_kernels.hip: launch_solve_n<N, T, ...> over launch_solve_t<T, ...>, launch_solve_global_n<N> (f64)."""
    src = _src("fx_kernels.hip")
    assert "chol_factor<N, T>(a, invd, lane)" in src and "chol_solve<N, T>(a, invd, rhs_l, lane)" in src
    ns = {int(n) for n in re.findall(r"launch_solve(?:_global)?_n<(\d+)", src)}
    ts = set(re.findall(r"launch_solve_t<(float|double)", src))
    return {(n, t) for n in ns for t in ts}


def test_every_register_cholesky_instantiation_has_a_variant():
    table = _table()
    rows_general = {(v.n // 16, "float" if v.dtype == np.float32 else "double", v.bounded)
                    for v in table if v.kind == "rows" and v.site == "general"}
    assert _general_rows() == rows_general
    rows_one = {(v.n // 16, "float" if v.dtype == np.float32 else "double", v.w, v.b)
                for v in table if v.kind == "rows" and v.site == "one"}
    assert _one_structure_rows() == rows_one
    for v in table:
        if v.kind == "rows" and v.site == "one":
            assert v.fwd == (v.n == 32)
    chol = {(v.n, "float" if v.dtype == np.float32 else "double") for v in table if v.kind == "chol"}
    assert _chol_sizes() == chol
    wide = _src("fx_wide.hip")
    assert "chol_factor<64, double>(a, invd, lane, (int)nb)" in wide
    assert "chol_forward<64, double>" in wide and "chol_backward<64, double>" in wide
    assert "chol_solve<64, double>(a, invd, t, lane, (int)n2)" in wide
    assert {v.site for v in table if v.kind == "wide"} == {"b1", "b2"}


def test_no_other_source_runs_the_register_cholesky():
    """The factor templates are called from the files above only: a new call site must join the table."""
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h", ".cpp")) or f in ("fx_chol.h", "fx_grouped_rows.h", "fx_debug_chol.hip"):
            continue
        s = _src(f)
        if re.search(r"RBlock<[^>]*>::(?:template )?factor", s):
            assert f in ("fx_grouped.hip", "fx_grouped_c.h"), f
        if re.search(r"\bchol_factor<", s):
            assert f in ("fx_kernels.hip", "fx_wide.hip"), f
