"""CPU replay of the pairing-free radix-16 norm and of the register file the mod-switch prep kernels hand it
(helib_amd/csrc/norm_r16.h "the direct form", ntt_kernels.hip PrepFuseIO; no GPU needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_direct_norm_and_the_prep_register_file_replayed_on_cpu(tmp_path):
    """tests/cpp/norm_direct_replay.cpp: the load twist (f_p + i f_(p+M)) W^p, passes A / B / C, the transposes, the lane
    exchange and the per-thread maxima run thread by thread against the long-double definition over ALL N = 2^14
    evaluation points, for single monomials at p = 0, 1, M-1, M, N-1 (every output compared, not only the maximum: a
    monomial's modulus is the same everywhere, its phase is what a wrong twist or a wrong pairing of the halves moves)
    and for dense random input, at the project's NORM_RTOL = 1e-9; and the inverse row transform of ntt_core.h,
    replayed into a store-all functor in both arithmetics (Shoup pairs and the Proth form the benchmark's primes take),
    leaves coefficient tid + 512 e in register e of thread tid -- what lets the
    prep kernels go from their last phase into pass A without a data exchange."""
    exe = str(tmp_path / "norm_direct_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-DHX_CHECK_BOUNDS",
                           os.path.join(ROOT, "tests", "cpp", "norm_direct_replay.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "norm_direct_replay OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("rel. error of the norm") == 8
