"""CPU tier of the randomised sweep of the five test families on the launch driver (tests/stat_fuzz_cases.py).

The first 6 seeds of every family run through the family's stand-alone host program (tests/tools/{cor,rank_test,sample_test,
normality_test,categorical_test}_host.cpp, built exactly as tests/test_*_restate_cpu.py and tests/test_*_abi_cpu.py build them: a
program of its own under ASan / UBSan, never loaded into python), at the default cap and at one drawn cap, and are held to the
restatements with check_records.  All five families have such a program; none is skipped.  assert_input_conditions (the float64
restatement against its higher-precision form, at a tenth of the bounds) runs for every seed the GPU module uses and for every
call its other tests state (stat_fuzz_cases.stated_calls), and the two
properties of the generator that the GPU tier relies on are asserted: the coverage of the sizes and kinds, and the pool strides
being coprime to the grids."""
import os
import subprocess

import numpy as np
import pytest

import stat_fuzz_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SEEDS = list(range(6))
GPU_SEEDS = list(range(12 * fc.SCALE))           # tests/test_gpu_fuzz_stat_tests.py: the same list
SOURCES = {"cor": "cor_host", "rank": "rank_test_host", "sample": "sample_test_host", "normality": "normality_test_host",
           "categorical": "categorical_test_host"}

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """family -> its host program.  Where a process-wide LD_PRELOAD is set a sanitizer's runtime could not be the first one loaded,
    so there the same programs are built without them and the cases still run."""
    folder = tmp_path_factory.mktemp("stat_fuzz")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    out = {}
    for family, name in SOURCES.items():
        out[family] = str(folder / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                            os.path.join(ROOT, "tests", "tools", name + ".cpp"), "-o", out[family]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return out


def _level(o):
    level = o.get("confidence_level", 0.95)
    return float("nan") if level is None else level


def host_input(call, cap):
    """The doubles a family's host program reads: the layouts of the per-family CPU tiers."""
    f, t, o = call["family"], call["test"], call["opts"]
    G, f64 = len(call["off"]) - 1, lambda a: np.asarray(a, np.float64)   # noqa: E731
    if f == "cor":
        head, cols = [t, o.get("alternative", 0), o.get("tau_type", 1), _level(o), cap, G, len(call["x"])], ("x", "y")
    elif f == "rank":
        head = [t, o.get("alternative", 0), int(o.get("correction", True)), o.get("mu", 0.0), cap, G, len(call["v"])]
        cols = ("v", "y", "sample")
    elif f == "sample":
        head = [t, o.get("alternative", 0), o.get("kind", 0), o.get("mu", 0.0), o.get("trim", 0.2), _level(o), cap, G, len(call["v"])]
        cols = ("v", "y", "sample")
    elif f == "normality":
        head, cols = [t, cap, G, len(call["v"])], ("v",)
    else:
        head = [t, o.get("alternative", 0), o.get("correction", False), o.get("exact", False), _level(o), cap, G, len(call["a"])]
        cols = ("a", "b")
    return np.concatenate([f64(head), f64(call["off"])] + [f64(call[c]) for c in cols])


def run_host(programs, call, cap=1462):
    out = subprocess.run([programs[call["family"]]], input=host_input(call, cap).tobytes(), capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, fc.WIDTH[call["family"]])


def drawn_cap(family, seed):
    return fc.CAPS[int(fc._rng(family, seed, 3).integers(len(fc.CAPS)))]


@pytest.mark.parametrize("seed", HOST_SEEDS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fuzz_host_build(host_programs, family, seed, record_property):
    call = fc.case(family, seed)
    ref = fc.reference(call)
    errs = {}
    for cap in (1462, drawn_cap(family, seed)):
        fc.check(call, run_host(host_programs, call, cap), ref, errs)
    for k, e in errs.items():
        record_property("worst_" + k, e)
    print(family, "test", call["test"], "seed", seed, {k: "%.2e" % e for k, e in errs.items()})


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_input_conditions_of_every_gpu_seed(family, record_property):
    errs = {}
    for seed in GPU_SEEDS:
        fc.assert_input_conditions(fc.case(family, seed), errs=errs)
    for k, e in errs.items():
        record_property("restatement_spread_" + k, e)
    print(family, {k: "%.2e" % e for k, e in errs.items()})


def test_input_conditions_of_the_stated_calls():
    """The cap ladder, the pools of the many-group tests, the stride sizes and the special values of the GPU tier."""
    seen = 0
    for name, call in fc.stated_calls():
        try:
            fc.assert_input_conditions(call)
        except AssertionError as e:
            raise AssertionError(name + ": " + str(e)) from None
        seen += 1
    assert seen == 5 * len(fc.CAPS) + len(fc.SMALL_TILED) + 2 * len(fc.EVERY_STAGED) + len(fc.EVERY_TEST)


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_gpu_seeds_cover_every_size_and_kind(family):
    cases = [fc.case(family, seed) for seed in range(12)]
    sizes = {n for c in cases for n in c["sizes"]}
    assert sizes >= set(fc.SMALL_SIZES) | set(fc.BOUNDARY_SIZES) | {fc.STRIDE_SIZE}, sorted(
        (set(fc.SMALL_SIZES) | set(fc.BOUNDARY_SIZES)) - sizes)
    assert all(c["sizes"].count(fc.STRIDE_SIZE) <= 1 and 8 <= len(c["sizes"]) <= 40 for c in cases)
    assert {c["test"] for c in cases} == set(fc.TESTS[family])
    assert {k for c in cases for k in c["kinds"]} == set(fc.KINDS[family])
    for c in cases:                     # a kind reaches only the tests of its table
        assert all(c["test"] in fc.KINDS[family][k] for k in c["kinds"])


def test_pool_strides_are_coprime_to_the_grids():
    """A workgroup that comes back after 65536 (1024) groups meets another pool member."""
    for n_pool in (fc.SMALL_POOL, fc.LARGE_POOL):
        assert 65536 % n_pool != 0 and 1024 % n_pool != 0
        assert np.gcd(65536, n_pool) == 1 and np.gcd(1024, n_pool) == 1


def test_tiled_call_repeats_its_pool():
    call, index, pool = fc.tiled_call("sample", 1, 7, 24, test=fc.ST.BRUNNER_MUNZEL)
    assert len(call["off"]) == 25 and list(index[:9]) == [0, 1, 2, 3, 4, 5, 6, 0, 1]
    for g in range(24):
        for name in ("v", "y", "sample"):
            mine = call[name][call["off"][g]:call["off"][g + 1]]
            assert mine.tobytes() == pool[name][pool["off"][index[g]]:pool["off"][index[g] + 1]].tobytes()
    assert len({pool["v"][pool["off"][i]:pool["off"][i + 1]].tobytes() for i in range(7) if pool["sizes"][i]}) == sum(n > 0 for n in pool["sizes"])
