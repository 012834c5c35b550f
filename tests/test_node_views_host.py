"""csrc/node_views.h, the one place that converts between the caller's node ids and the library's: a stand-alone
program (tests/host_node_views.cpp) that includes nothing but the header, built with plain g++ under AddressSanitizer
and UBSan.  Host only; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_views_under_sanitizers(tmp_path):
    """to_library / to_caller for N in {1, 7}, identity / reversed / scrambled numbering, (width, stride) in
    {(1,1), (3,3), (3,4), (6,6)}, double and int, owned ranges empty / all / interior / touching either end: every lane
    where perm[caller id] = library id puts it, pad lanes exactly zero over a NaN-filled destination, the round trip bit
    for bit, +0 (sign bit checked) outside the owned range; buffers sized exactly, so an overrun is a report."""
    exe = str(tmp_path / "host_node_views")
    cmd = ["g++", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
           "-I" + os.path.join(ROOT, "fea-large_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_node_views.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    # 2 sizes x 3 numberings x 4 shapes x 2 types, each 3 checks and 2 per owned range (N = 1 has 4 ranges, N = 7 five)
    assert "node views: %d checks, 0 failures" % (3 * 4 * 2 * ((3 + 2 * 4) + (3 + 2 * 5))) in r.stdout, r.stdout[-2000:]
