"""CPU suite: the lazy residue arithmetic of csrc/ntt_conv.hpp (ntt_mul, ntt_red, ntt_canon, ntt_reg_levels) on the host.

The four functions are `__host__ __device__`; tests/ntt_lazy_arith.hip is a stand-alone program (own main, no HIP API call) that
calls them at the inputs where the uncorrected quotient estimate is tightest and compares with 128-bit integers -- see its
header for the families.  This test builds it with hipcc (host side only: no device code is needed to run it) and runs it; the
contract asserted is the header's |a| < 2^39, b < 2^32 (ntt_mul), |v| < 2^40 (ntt_red) and magnitudes below 2^39 after the seven
levels of a 128-point transform.  The head room the program measures beyond that contract is printed, and only required not to
be negative: the number recorded in ntt_conv.hpp (2^41) is a measurement, not part of the contract."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
SRC = os.path.join(ROOT, "tests", "ntt_lazy_arith.hip")


def test_lazy_arithmetic_keeps_its_contract_on_the_host(tmp_path):
    exe = str(tmp_path / "ntt_lazy_arith")
    cmd = ["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off",
           "-I", os.path.join(ROOT, PKG, "csrc"), "-o", exe, SRC]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS") and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
    # every family ran, for both primes, with the numbers of inputs the program is written for
    for name, least in (("ntt_mul", 10_000_000), ("ntt_red", 3_000_000)):
        counts = [int(n) for n in re.findall(name + r" prime \d+: (\d+) inputs", run.stdout)]
        assert len(counts) == 2 and min(counts) >= least, (name, counts)
    peaks = [float(p) for p in re.findall(r"largest magnitude (\d+) ", run.stdout)]
    # all inputs 2 P - 1: the zero frequency is 128 (2 P - 1), the most seven levels can reach -- seen, and below 2^39
    assert peaks == [128.0 * (2 * 2013265921 - 1), 128.0 * (2 * 1811939329 - 1)] and max(peaks) < 2.0 ** 39, peaks
    head = int(re.search(r"headroom_log2 (\d+)", run.stdout).group(1))
    print("measured head room of ntt_mul: |a| < 2^%d" % head)
    assert head >= 39
