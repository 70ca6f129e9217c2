"""CPU tier of the one-group scaffolding and the batch argument check: csrc/scalar_fit.h and csrc/context.h in
tests/tools/scalar_fit_host.cpp, a program of its own compiled by g++ under ASan / UBSan and never loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
input 2 3 3 0 3 nan=1 valid=1 w=0
weighted valid=1 w=1
one 1 2 2 len=2 pad_nan=1 1 xp=1
status 10 -> 10 All rows filtered due to NULL/NaN values
status 6 -> 6 Insufficient data: 1 rows, 2 features (need rows > features)
status 1 -> 1 Some fit failed on the GPU path
lengths 1 0 -> 9 Dimension mismatch: y has 3 elements, X has 2 rows
result 0.25 -0.5 2 1 0.9 0.8 0.1 3 2
args 0 1 negative n_groups or n_rows
args 0 1 x is NULL or empty
args 0 1 n_features = 3 exceeds the supported maximum of 2
args 0 1 an array is NULL
args 0 1 x column pointer is NULL
args 1 0 
args 0 1 x column pointer is NULL
args 0 1 an array is NULL
args 1 0 
args 0 1 negative n_groups or n_rows
fmt -1 1.5
"""


def test_scalar_fit_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "scalar_fit_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "tools", "scalar_fit_host.cpp"), "-o", exe,
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout == EXPECTED
