"""CPU suite: guards of the build and of the source layout.

* csrc/ holds the product only.  Ablations and timing mocks compute WRONG results (SFL_PROBE_*, SEAM_MOCK_NO_P): no such flag
  changes one token of what the compiler sees of the product, none of their names occurs under csrc/, and csrc/ includes nothing
  from tools/.
* The trace harness tools/sor_clock_probe.hip (which brings its own backend and kernel, tools/probe/) compiles, plain and with each
  of its switches.
* No translation unit or header under csrc/ grows past 900 lines again (round 4's sfl_api.cpp had reached 2710).
* The stencils of the sim step are written once (advect_math.h); the kernels call them."""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
PRODUCT_DEFINES = ["-DSFL_NS_GROUP=2", "-DSFL_DX_PART=0", "-DSFL_FOLD_PART=0"]
PROBE_TOKENS = ["SFL_PROBE", "SFL_SOR_TRACE", "SEAM_MOCK", "SFL_ALLOW_TIMING_MOCKS", "coop_mock", "coop_mem", "WaveTrace", "g_sor_trace"]


def _preprocessed(source, flags):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-ffp-contract=off", "-E", "-P", *PRODUCT_DEFINES,
                        *flags, os.path.join(CSRC, source), "-o", "-"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert len(r.stdout) > 10000
    return r.stdout


@pytest.mark.parametrize("flag", ["-DSFL_PROBE_NO_LOAD=1", "-DSFL_PROBE_SHIFT=1", "-DSFL_PROBE_COOP=3", "-DSFL_PROBE_NO_STORE=1", "-DSEAM_MOCK_NO_P=1"])
def test_no_diagnostic_switch_changes_the_product_source(flag):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    source = "advect_tiled.hip" if "SEAM" in flag else "sor_fused.hip"
    assert _preprocessed(source, [flag]) == _preprocessed(source, [])


def test_csrc_holds_no_probe_code():
    files = [f for f in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True) if os.path.isfile(f)]
    assert len(files) > 20
    assert not [f for f in files if os.path.basename(f) == "sor_probe_mocks.inc"]
    for f in files:
        text = open(f, errors="replace").read()
        assert not [t for t in PROBE_TOKENS if t in text], f
        assert not [inc for inc in re.findall(r'#\s*include\s*"([^"]+)"', text) if "tools/" in inc.replace("\\", "/")], f


# every remaining switch of tools/probe/sor_probe.h is set in at least one run (the two load / store switches of a pair exclude
# each other: NO_LOAD hides what P_LOAD_AUX changes)
PROBE_BUILDS = [
    [],
    ["-DSFL_PROBE_NO_LOAD=1", "-DSFL_PROBE_NO_STORE=1", "-DSFL_PROBE_SHIFT=1", "-DSFL_PROBE_NO_LDS=1"],
    ["-DSFL_PROBE_P_LOAD_AUX=16", "-DSFL_PROBE_P_STORE_AUX=16", "-DSFL_PROBE_SHIFT=2", "-DSFL_PROBE_NO_EDGE=1"],
]


@pytest.mark.parametrize("flags", PROBE_BUILDS, ids=lambda f: "+".join(x[12:] for x in f) or "plain")
def test_the_probe_compiles(flags):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    header = open(os.path.join(ROOT, "tools", "probe", "sor_probe.h")).read()
    switches = set(re.findall(r"#ifndef (SFL_PROBE_\w+)", header))
    assert switches and switches == {x[2:].split("=")[0] for build in PROBE_BUILDS for x in build}
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsyntax-only",
                        "-DSFL_NS_GROUP=5", "-DPROBE_NS=16", *flags, os.path.join(ROOT, "tools", "sor_clock_probe.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_no_source_file_outgrows_900_lines():
    long = {os.path.basename(f): sum(1 for _ in open(f)) for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f)}
    assert long and max(long.values()) <= 900, {k: v for k, v in long.items() if v > 900}


def test_each_step_stencil_is_written_once():
    """Divergence, v - grad p and the four-texel mix carry the numerics contract (operation order, the -0.0f rules, where a UQ32
    narrows): one copy each, in advect_math.h, so that a change cannot reach some kernels and miss others."""
    text = {os.path.basename(f): open(f, errors="replace").read() for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f)}
    assert len(text) > 20

    def where(pattern):
        return {name: len(re.findall(pattern, body)) for name, body in text.items() if re.search(pattern, body)}

    assert where(r"\(pe - pw\)") == {"advect_math.h": 1}                      # the gradient difference
    assert where(r"\? *-\w+(\[[^\]]*\])*\.x *: *\w+\.x") == {"advect_math.h": 1}  # div_expr_safe: (i > 0) ? -west.x : own.x
    assert where(r": *-own\.x") == {"advect_math.h": 1}                       # ... and its ghost on the other side
    # the nested mix of four texels: the one of advect_math.h (mix4) and advect_generic.hip's per-channel one
    assert where(r"mix1\(s\.di, *mix1\(s\.dj,") == {"advect_math.h": 1, "advect_generic.hip": 1}
    # a closed experiment's switch: nowhere but in the records of its measurements
    closed = "SEAM_DYE_" + "LOADS"
    kept = (os.path.join(ROOT, "profiles") + os.sep, os.path.join(ROOT, "DESIGN.md"), os.path.join(ROOT, "build") + os.sep,
            os.path.join(ROOT, ".git") + os.sep)
    hits = []
    for folder, _, names in os.walk(ROOT):
        for name in names:
            f = os.path.join(folder, name)
            if f.startswith(kept) or not name.endswith((".h", ".hip", ".inc", ".cpp", ".c", ".py", ".sh", ".md", ".txt", ".json", "Makefile")):
                continue
            if closed in open(f, errors="replace").read():
                hits.append(os.path.relpath(f, ROOT))
    assert not hits, hits
