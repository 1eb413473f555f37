"""CPU: the device slice parser's source under AddressSanitizer and UndefinedBehaviorSanitizer.

tests/fuzz/device_parse_fuzz.cpp, a program of its own, is compiled with g++
-fsanitize=address,undefined together with the scan and the CPU twin (parse.cpp, tables.cpp; the
twin runs csrc/slice_parse.h, the very source parse.hip compiles for the device).  It pushes
mutated golden streams, one per chroma format, through scan + twin with every buffer a heap block
of exactly the device's size: the bitstream span plus 16 zero bytes, the counted records, the
counted coefficient words.  An access one byte too far, undefined behaviour, a slice that runs
past its iteration bound, an emit pass that differs from its count pass, a mutant the twin accepts
and the host emitter does not (or the reverse), or accepted records that differ, fail the run."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
STREAMS = os.path.join(REPO, "tests", "golden", "streams")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san_dp") / "device_parse_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", CSRC, "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "fuzz", "device_parse_fuzz.cpp"), os.path.join(CSRC, "parse.cpp"),
           os.path.join(CSRC, "tables.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_mutated_streams_through_scan_and_twin_under_asan_ubsan(harness):
    man = {m["name"]: m for m in json.load(open(os.path.join(STREAMS, "manifest.json")))}
    args = []
    for n in ("ipb420_field", "ipb422_field", "ipb444_field"):
        m = man[n]
        args += [os.path.join(STREAMS, m["file"]), str(m["width"]), str(m["height"]), str(m["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, "1000", "11"] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mutants_parsed"] > 0 and res["mutants_rejected"] > 1000
