"""Histories, the CPU side: sfl_history_* and sfl_batch_history_* (include/sfl.h "HISTORIES") as the binding sees them --
symbols, signatures, the Python methods, the record's 64 bytes -- every refusal that needs no device with its own message,
and the host unit (csrc/history.cpp and its hooks in the step calls) run through by tests/cpp/history_driver.cpp over a
runtime that lives on the host.  tests/test_history_gpu.py has the kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CALLS = ["start", "stop", "info", "read"]
METHODS = ["history_start", "history", "history_info", "history_stop"]
FIELDS = ["max_abs_vx", "max_abs_vy", "max_abs_div", "what", "dye_sum", "update_norm", "iterations", "step", "dt", "dx"]
OFFSETS = [0, 4, 8, 12, 16, 40, 44, 48, 56, 60]


def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, p64, rec = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(cap.HistoryRecord)
    want = {"sfl_batch_history_start": [vp, i, i, i, i], "sfl_batch_history_stop": [vp], "sfl_batch_history_info": [vp, pi, pi, p64],
            "sfl_batch_history_read": [vp, i, i, i, i, rec, sz],
            "sfl_history_start": [vp, i, i], "sfl_history_stop": [vp], "sfl_history_info": [vp, pi, pi, p64],
            "sfl_history_read": [vp, i, i, rec, sz]}
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for prefix, handle in (("sfl_history_", "sfl_context *ctx"), ("sfl_batch_history_", "sfl_batch *b")):
        for call in CALLS:
            name = prefix + call
            assert hasattr(lib, name), name
            assert cap.SIGNATURES[name] == (C.c_int, want[name]), name
            assert getattr(lib, name).argtypes == want[name] and getattr(lib, name).restype == C.c_int
            assert re.search(r"SFL_API int %s\(%s[,)]" % (name, re.escape(handle)), header), name
    assert "int every, int first, int count, int capacity)" in header and "sfl_history_start(sfl_context *ctx, int every, int capacity)" in header
    assert re.search(r"sfl_batch_history_read\(sfl_batch \*b, int first_sample, int samples, int first, int count,\s+struct sfl_history_record \*host, size_t bytes\)", header)
    for cls in (sfl.Solver, sfl.BatchSolver):
        for name in METHODS:
            assert callable(getattr(cls, name, None)), (cls, name)
    assert lib.sfl_abi_version() == 1
    text = open(os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "history_kernels.h")).read()
    assert int(re.search(r"constexpr int kHistoryThreads = (\d+);", text).group(1)) == sfl.HISTORY_THREADS


def test_the_record_is_64_bytes_at_the_headers_offsets(sfl):
    """Three views of one layout: the header's struct as the binding's numpy dtype, as its ctypes structure, and as the
    header's own text; a C compiler's view is tests/cpp/history_layout.c (below).  The first 40 bytes are a flow-statistics
    record."""
    dt = sfl.HISTORY_DTYPE
    assert dt.itemsize == 64 and list(dt.names) == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == OFFSETS
    assert [dt.fields[n][0].str for n in FIELDS if n != "dye_sum"] == ["<f4", "<f4", "<f4", "<u4", "<f4", "<i4", "<i8", "<f4", "<f4"]
    assert dt.fields["dye_sum"][0].shape == (3,) and dt.fields["dye_sum"][0].base == np.dtype("<u8")
    rec = sfl.capi.HistoryRecord
    assert C.sizeof(rec) == 64 and [getattr(rec, n).offset for n in FIELDS] == OFFSETS
    flow = sfl.FLOW_STATS_DTYPE
    assert flow.itemsize == dt.fields["update_norm"][1] and all(flow.fields[n][1] == dt.fields[n][1] and flow.fields[n][0] == dt.fields[n][0] for n in flow.names)
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    body = re.search(r"struct sfl_history_record \{(.*?)\};\s*/\* 64 bytes: offsets 0, 4, 8, 12, 16, 40, 44, 48, 56, 60 \*/", header, re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[3\])?[,;]", body) == FIELDS


def test_a_c_compiler_sees_the_same_layout():
    if not (shutil.which(os.environ.get("CC", "cc")) and shutil.which("make")):
        pytest.skip("no C compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "history.mk", os.path.join(cpp, "history_layout")], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, "history_layout")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "sfl_history_record: 64 0 4 8 12 16 40 44 48 56 60\n0 mismatches" in r.stdout, r.stdout


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    """The checks that need no device: a value that is wrong whatever the handle first, then NULL."""
    lib, cap = sfl.capi.lib(), sfl.capi
    rec, w, a = (cap.HistoryRecord * 4)(), C.c_int(5), C.c_int64(5)
    big = 2 ** 31 - 1
    b, c = "sfl_batch_history_", "sfl_history_"
    refusals = [
        (lambda: lib.sfl_batch_history_start(None, 0, 0, 1, 4), b + "start: every must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_history_start(None, -3, 0, 1, 4), "every must be >= 1 (got -3)"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, 1, 0), b + "start: capacity must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, 1, -1), "capacity must be >= 1 (got -1)"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, 0, 4), b + "start: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, -2, 4), "count must be >= 1 (got -2)"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, big, big), f"capacity {big} samples of {big * 64} bytes each exceed the address space"),
        (lambda: lib.sfl_batch_history_start(None, 1, 0, 1, 4), b + "start: batch is NULL"),
        (lambda: lib.sfl_history_start(None, 0, 4), c + "start: every must be >= 1 (got 0)"),
        (lambda: lib.sfl_history_start(None, 1, 0), c + "start: capacity must be >= 1 (got 0)"),
        (lambda: lib.sfl_history_start(None, 1, 4), c + "start: ctx is NULL"),
        (lambda: lib.sfl_batch_history_stop(None), b + "stop: batch is NULL"),
        (lambda: lib.sfl_history_stop(None), c + "stop: ctx is NULL"),
        (lambda: lib.sfl_batch_history_info(None, C.byref(w), C.byref(w), C.byref(a)), b + "info: batch is NULL"),
        (lambda: lib.sfl_history_info(None, C.byref(w), C.byref(w), C.byref(a)), c + "info: ctx is NULL"),
        (lambda: lib.sfl_batch_history_read(None, -1, 1, 0, 1, rec, 64), "first_sample and samples must be >= 0"),
        (lambda: lib.sfl_batch_history_read(None, 0, -2, 0, 1, rec, 64), "first_sample and samples must be >= 0"),
        (lambda: lib.sfl_batch_history_read(None, 0, 1, 0, 0, rec, 0), b + "read: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_history_read(None, 0, 2, 0, 2, rec, 255), "2 samples of 2 records of 64 bytes are 256 bytes, got 255"),
        (lambda: lib.sfl_batch_history_read(None, 0, 2, 0, 2, rec, 256), b + "read: batch is NULL"),
        (lambda: lib.sfl_history_read(None, -1, 1, rec, 64), c + "read: samples [-1, -1 + 1)"),
        (lambda: lib.sfl_history_read(None, 0, 3, rec, 128), "3 samples of 1 records of 64 bytes are 192 bytes, got 128"),
        (lambda: lib.sfl_history_read(None, 0, 3, rec, 192), c + "read: ctx is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert (w.value, a.value) == (5, 5)


def test_the_python_front_end_checks_the_range_of_a_context(sfl):
    class Fake(sfl.Solver):
        def __init__(self):   # (no library, no device: the check comes first)
            self._h, self._lib = None, None

        def __del__(self):
            pass

    with pytest.raises(ValueError):
        Fake().history_start(1, 4, first=1)
    with pytest.raises(ValueError):
        Fake().history_start(1, 4, count=2)


def test_the_host_side_of_the_histories():
    """`make -C tests/cpp -f history.mk`: tests/cpp/history_driver.cpp, a stand-alone program under AddressSanitizer + UBSan.
    Steps count across calls and across the three step calls; solves and setups do not; a call one sample too long is refused
    whole, with the step count, the force timeline and the recorder's frames untouched; a timeline call is cut at the steps
    whose sample is due, with a recorder on at either's; a sample is handed the fields its step left, the call's member table
    and, under the stopping rule, the iteration counts; a context steps without seams while a history is on, its two passes
    pointed into the record, the host's words merged at read time; restart, stop, read ranges; destroy with a live history
    leaves no allocation."""
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "history.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "history_driver")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
