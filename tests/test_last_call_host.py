"""CPU (-m "not gpu"): the "last call" record type of csrc/last_call.h - a ThreadSanitizer run of Last<> and TimedCall in a program of its
own (tests/last_call_tsan_main.cpp), and a source check of the rule it serves: a unit learns a sub-call's time from the sub-call's
out-parameter, never from another unit's getter, and keeps no bare float record at namespace scope."""
import glob
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celo-bls-snark-rs_amd", "csrc")
# the getters of a record that a composed call used to read after its sub-call had returned: the C API's alone now
CAPI_ONLY = ("hash_last_ms", "hash_last_rounds", "wire_last_ms", "wire_encode_last_ms", "pairing_timings_377")
GONE = ("pairing_timings_761",)              # the BW6-761 engine's record had no reader besides the staged product: removed, and never to be called


def test_records_under_thread_sanitizer_in_a_program_of_its_own(tmp_path):
    """its own main, built with -fsanitize=thread (the runtime linked into the program), run as a subprocess, nothing preloaded for it: four
    noting threads, one updating, two reading, 100 000 iterations each - every record read is whole - and the guard's three exits.  No
    sanitizer enters this process."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to build tests/last_call_tsan_main.cpp")
    exe = str(tmp_path / "last_call_tsan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "last_call_tsan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "last_call ok" in run.stdout and "ThreadSanitizer" not in run.stderr, run.stdout[-2000:] + run.stderr[-4000:]


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.cpp")))


def test_no_unit_reads_another_units_record():
    """outside capi.hip the six getters appear only where they are declared (units.h) and defined (their unit): nothing calls them"""
    assert len(sources()) > 80
    names = "|".join(CAPI_ONLY + GONE)
    decl = re.compile(r"^(?:int|float|void)\s+(?:%s)\(" % "|".join(CAPI_ONLY))
    calls = []
    for path in sources():
        if os.path.basename(path) == "capi.hip":
            continue
        for no, line in enumerate(open(path), 1):
            code = line.split("//")[0]
            if re.search(r"\b(?:%s)\(" % names, code) and not decl.match(code):
                calls.append("%s:%d" % (os.path.basename(path), no))
    assert not calls, calls
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert all(re.search(r"\b%s\(" % name, capi) for name in CAPI_ONLY) and not any(name in capi for name in GONE)
    units = open(os.path.join(CSRC, "units.h")).read()
    assert "timings(float" not in re.search(r"struct Pairing377 \{.*?\n\};", units, re.S).group(0) + re.search(r"struct Pairing761 \{.*?\n\};", units, re.S).group(0)


def test_no_unit_keeps_a_bare_float_record():
    """no unit_*.hip declares a float or atomic float variable at namespace scope: the records are Last<> instances"""
    units = sorted(glob.glob(os.path.join(CSRC, "unit_*.hip")))
    assert len(units) > 30
    bare = re.compile(r"^static\s+(?:float|std::atomic<float>)\s+\w+\s*(?:\[|=|;|\{)")
    found = ["%s:%d" % (os.path.basename(p), no) for p in units for no, line in enumerate(open(p), 1) if bare.match(line)]
    assert not found, found
    assert bare.match("static float g_x_ms[8] = {};") and bare.match("static std::atomic<float> g_x{0.f};") and not bare.match("static float f(int x) {")
    assert sum(len(re.findall(r"^static Last<", open(p).read(), re.M)) for p in units) >= 14


def test_the_header_needs_no_device_runtime():
    text = open(os.path.join(CSRC, "last_call.h")).read()
    assert "hip" not in text.lower()
    assert re.findall(r"#include\s+(\S+)", text) == ["<chrono>", "<mutex>"]
