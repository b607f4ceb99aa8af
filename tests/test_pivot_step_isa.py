"""The pivot step of the band builds' register Cholesky (fx_grouped_rows.h: RStep::factor, RStep::pivots_close), CPU only: the ISA
of fx_grouped_band.hip, cross-compiled with the Makefile's flags, between the first and the last v_fmac_f64_dpp of each kernel
(the factor with the forward substitution fused in, the closing pivot checks and the backward substitution).

* The fused build checks the pivots once after the last step, so the stretch holds a handful of f64 compares instead of three
  per step, and no chain of selects that picks invd out of 32 live rsqrt results.
* One family of lane masks (hl > k) is left, so the masks fit in SGPRs: the staged build (the headline's) reads almost none of
  them back from VGPR lanes.
* The non-DPP VALU count of the stretch stays below the figure after the change (parent: 871 in the staged <5, 4> build)."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = [(5, 0), (5, 4), (5, 6)]


@pytest.fixture(scope="module")
def band_asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    d = tmp_path_factory.mktemp("pivot_isa")
    out = d / "fx_grouped_band.s"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "fiksi_amd", "csrc", "fx_grouped_band.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=str(d), timeout=900)
    return out.read_text()


def _stretch(text, staged, w, b):
    kernel = "lm_solve_grouped_c_band_staged_kernel" if staged else "lm_solve_grouped_c_band_kernel"
    name = r"_ZN2fx%d%sILi%dELi%dE\S*" % (len(kernel), kernel, w, b)
    m = re.search(r"^(%s):(.*?)^\s*s_endpgm" % name, text, re.S | re.M)
    assert m, name
    ins = [l.split()[0] for l in m.group(2).split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))]
    first = ins.index("v_fmac_f64_dpp")
    last = len(ins) - 1 - ins[::-1].index("v_fmac_f64_dpp")
    return collections.Counter(ins[first:last + 1])


@pytest.mark.parametrize("w, b", BANDS)
@pytest.mark.parametrize("staged", [True, False])
def test_pivot_step_bookkeeping(band_asm, staged, w, b):
    c = _stretch(band_asm, staged, w, b)
    assert c["v_fmac_f64_dpp"] > 300, c  # the scan sees the factor
    f64_cmps = sum(v for k, v in c.items() if k.startswith("v_cmp_") and "_f64" in k)
    assert f64_cmps <= 8, c  # parent: 92, three per step
    non_dpp_valu = sum(v for k, v in c.items() if k.startswith("v_") and "_dpp" not in k)
    assert non_dpp_valu <= (760 if staged else 800), non_dpp_valu  # parent: 871 / 882 (<5, 4>); now 742 / 784
    if staged:
        assert c["v_readlane_b32"] <= 8, c  # parent: 71; now 6 or 7, in the backward substitution and the closing check
