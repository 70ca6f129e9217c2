"""Every DuckDB glue file of duckdb_shim/ on a recording mock of the C ABI, as one stand-alone program under ASan / UBSan
(tests/tools/glue_transcript.cpp): what it registers, what it binds, and what Update -> Combine -> Finalize -> Destroy hand to
the ABI and write into the result, compared byte for byte with tests/golden/glue_transcript.txt.  The golden file was recorded
from the glue as it stood before its Update / Bind / registration code was folded into row_shapes.hpp: the program uses the
public Register...Function entry points and the stand-in DuckDB API only, so building it on that earlier tree reproduces the
file."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

SHIM = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
TOOLS = os.path.join(ROOT, "tests", "tools")
GOLDEN = os.path.join(ROOT, "tests", "golden", "glue_transcript.txt")
GLUE = ["fit_agg_hip", "family_agg_hip", "elasticnet_agg_hip", "elasticnet_family_hip", "rls_family_hip", "bls_family_hip", "quantile_family_hip",
        "glm_family_hip"]


def test_the_glue_reproduces_the_recorded_transcript(tmp_path):
    """The child inherits the environment unchanged; a process-wide preload would sit in front of the sanitizer's runtime, so
    the test does not run under one."""
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: a sanitizer build must be the first runtime a process loads")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    flags = ["-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(TOOLS, "duckdb_stub"),
             "-I" + os.path.join(ROOT, "include"), "-I" + SHIM, "-I" + TOOLS]
    sources = [os.path.join(TOOLS, "glue_transcript.cpp")] + [os.path.join(SHIM, name + ".cpp") for name in GLUE]

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        return obj, subprocess.run(["g++", *flags, "-c", src, "-o", obj], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(len(sources), os.cpu_count() or 1)) as pool:  # (the files are independent translation units)
        built = list(pool.map(compile_one, sources))
    for _, r in built:
        assert r.returncode == 0, r.stderr
    exe = str(tmp_path / "glue_transcript")
    r = subprocess.run(["g++", *sanitize, *[obj for obj, _ in built], "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True)
    stderr = r.stderr.decode(errors="replace")
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace") + stderr
    assert "ERROR" not in stderr and "runtime error" not in stderr, stderr
    with open(GOLDEN, "rb") as f:
        want = f.read()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.split(b"\n"), want.split(b"\n")
        first = next((k for k, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b), min(len(got_lines), len(want_lines)))
        pytest.fail("the transcript differs from tests/golden/glue_transcript.txt at line %d:\n  got  %r\n  want %r"
                    % (first + 1, got_lines[first][:300] if first < len(got_lines) else None, want_lines[first][:300] if first < len(want_lines) else None))
