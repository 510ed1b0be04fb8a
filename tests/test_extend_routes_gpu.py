"""What each route of the exact basis extension (engine.hip: launch_extend over rns_plan.h's extend_route) launches.

addPrimes, toPolyMod, the generic and several-primes mod-switch and both digit breakers build one plan per (sources,
targets) and send it down one of five routes: the fast kernels in Garner form, in HPS form, in HPS form with the
target sums on the matrix cores, the wide kernels (VALU or matrix cores), and the generic kernel.  As
test_modswitch_routes_gpu.py does for the mod-switch, this file pins the launches of each: the full table of (kernel,
workgroups, workgroup_size, calls) that hx.profileBegin() / profileEnd() report, next to every output word against
the oracle.  The tables are literals (EXPECTED below), recorded with this file's own helper,

    python -m tests.test_extend_routes_gpu

on the commit before get_plan was split into the host-only builder of rns_plan.h and launch_extend into a route
function and a launch switch; the split had to reproduce them exactly.  A change of the host code that keeps the
launches leaves them as they are; a change of a kernel's grid is a change of this table, made on purpose and recorded
again.  Shapes: m = 256 (N = 128, the ring of the boundary tests) and a batch of 3, so that a row is 384 words -- two
256-thread workgroups, the second one partial.  Ten cases, each well under a second on an MI355X."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import rns_boundary_ref as R
from tests.test_rns_boundary_gpu import Pair

pytestmark = pytest.mark.gpu

M, B = 256, 3
SWITCHES = ("HX_HPS_MIN_N", "HX_NO_MFMA_EXT", "HX_NO_PROTH_RNS", "HX_HPS_EPS", "HX_MFMA_MIN_N", "HX_NO_PROTH")
VALU, MFMA4 = {"HX_NO_MFMA_EXT": "1"}, {"HX_MFMA_MIN_N": "4"}

EXPECTED = {'add_primes_n1': [('hx::copy_words_kernel', 1, 256, 2),
                   ('hx::ntt_small_kernel<false>', 33, 64, 1),
                   ('hx::ntt_small_kernel<true>', 3, 64, 1),
                   ('hx::rns_extend_fast_kernel<1, false>', 2, 256, 1)],
 'add_primes_n17': [('hx::copy_words_kernel', 13, 256, 2),
                    ('hx::ntt_small_kernel<false>', 33, 64, 1),
                    ('hx::ntt_small_kernel<true>', 51, 64, 1),
                    ('hx::rns_extend_kernel<40>', 64, 256, 1),
                    ('hx::rns_extend_mfma_kernel<5>', 3, 256, 1)],
 'add_primes_n17_no_mfma_ext': [('hx::copy_words_kernel', 13, 256, 2),
                                ('hx::ntt_small_kernel<false>', 33, 64, 1),
                                ('hx::ntt_small_kernel<true>', 51, 64, 1),
                                ('hx::rns_extend_kernel<40>', 64, 256, 1),
                                ('hx::rns_extend_wide_kernel<20>', 1, 1024, 1)],
 'add_primes_n41': [('hx::copy_words_kernel', 31, 256, 2),
                    ('hx::ntt_small_kernel<false>', 33, 64, 1),
                    ('hx::ntt_small_kernel<true>', 123, 64, 1),
                    ('hx::rns_extend_kernel<64>', 2, 256, 1)],
 'add_primes_n4_mfma_min_n_4': [('hx::copy_words_kernel', 3, 256, 2),
                                ('hx::ntt_small_kernel<false>', 33, 64, 1),
                                ('hx::ntt_small_kernel<true>', 12, 64, 1),
                                ('hx::rns_extend_fast_kernel<4, false>', 64, 256, 1),
                                ('hx::rns_extend_mfma_kernel<2>', 3, 256, 1)],
 'add_primes_n8': [('hx::copy_words_kernel', 6, 256, 2),
                   ('hx::ntt_small_kernel<false>', 33, 64, 1),
                   ('hx::ntt_small_kernel<true>', 24, 64, 1),
                   ('hx::rns_extend_fast_kernel<8, false>', 2, 256, 1)],
 'add_primes_n9': [('hx::copy_words_kernel', 7, 256, 2),
                   ('hx::ntt_small_kernel<false>', 33, 64, 1),
                   ('hx::ntt_small_kernel<true>', 27, 64, 1),
                   ('hx::rns_extend_fast_kernel<9, false>', 64, 256, 1),
                   ('hx::rns_extend_mfma_kernel<3>', 3, 256, 1)],
 'add_primes_n9_no_mfma_ext': [('hx::copy_words_kernel', 7, 256, 2),
                               ('hx::ntt_small_kernel<false>', 33, 64, 1),
                               ('hx::ntt_small_kernel<true>', 27, 64, 1),
                               ('hx::rns_extend_fast_kernel<9, false>', 64, 256, 1),
                               ('hx::rns_extend_fast_kernel<9, true>', 2, 256, 1)],
 'break_into_digits_9_prime_digit': [('hx::copy_words_kernel', 10, 256, 1),
                                     ('hx::ntt_small_kernel<false>', 120, 64, 1),
                                     ('hx::ntt_small_kernel<true>', 39, 64, 1),
                                     ('hx::rns_extend_fast_kernel<4, false>', 2, 256, 1),
                                     ('hx::rns_extend_fast_kernel<9, false>', 2, 256, 1)],
 'to_poly_mod_7_n3': [('hx::copy_words_kernel', 3, 256, 1),
                      ('hx::ntt_small_kernel<true>', 9, 64, 1),
                      ('hx::rns_extend_kernel<8>', 2, 256, 1)]}


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the extension route tests run on an MI355X (pytest -m gpu)")
    return capi


def launches(hx, fn):
    """fn's result and its launch table: sorted (kernel, workgroups, workgroup_size, calls)"""
    hx.profileBegin()
    out = fn()
    prof = hx.profileEnd()
    assert prof["dropped"] == 0
    return out, sorted((k["kernel"], k["workgroups"], k["workgroup_size"], k["calls"]) for k in prof["kernels"])


# ---------------------------------------------------------------- the cases: each returns its launch table
def add_primes(hx, n):
    """addPrimes from n 60-bit sources onto six 60-bit, three 56-bit and two 45-bit targets"""
    P = Pair(hx, M, R.many_source_chain(O, n, M))
    src, tgt = list(range(n)), list(range(n, n + 11))
    x = P.rand(src, 40 + n, batch=B)
    d = hx.DoubleCRT(P.g, src, B, x)
    _, table = launches(hx, lambda: d.addPrimes(tgt))
    got = d.download()
    assert d.getIndexSet() == src + tgt
    for b in range(B):
        assert np.array_equal(got[:n, b], x[:, b]), b
        assert np.array_equal(got[n:, b], P.o.add_primes(src, x[:, b], tgt)), b
    return table


def to_poly_mod(hx, n, t):
    """toPolyMod(t), t below 2^32: a plan with an explicit target modulus, which the fast kernels refuse"""
    P = Pair(hx, M, R.many_source_chain(O, n, M))
    src = list(range(n))
    x = P.rand(src, 60 + n, batch=B)
    d = hx.DoubleCRT(P.g, src, B, x)
    got, table = launches(hx, lambda: d.toPolyMod(t))
    assert np.array_equal(d.download(), x)
    for b in range(B):
        assert [int(v) for v in got[b]] == [int(v) % t for v in P.o.to_poly(src, x[:, b])], b
    return table


def break_digits(hx, n):
    """hx_break_into_digits with an n-prime digit in front of a 4-prime one: the first launch updates the later digit's
    rows in place (ExtArgs::upd), which has no HPS form below 17 sources"""
    P = Pair(hx, M, R.many_source_chain(O, n, M))
    src, four, sp = list(range(n)), list(range(n, n + 4)), list(range(n + 4, n + 11))
    own, digits = src + four, [src, four]
    x = P.rand(own, 80 + n, batch=B)
    d = hx.DoubleCRT(P.g, own, B, x)
    dg, table = launches(hx, lambda: d.breakIntoDigits(digits, sp))
    got = dg.download()
    for b in range(B):
        want = P.o.break_into_digits(own, x[:, b], digits, own + sp)
        assert np.array_equal(got[:, b].reshape(len(digits), len(own + sp), P.N), want), b
    return table


CASES = {"add_primes_n1": ({}, lambda hx: add_primes(hx, 1)),
         "add_primes_n8": ({}, lambda hx: add_primes(hx, 8)),
         "add_primes_n9": ({}, lambda hx: add_primes(hx, 9)),
         "add_primes_n9_no_mfma_ext": (VALU, lambda hx: add_primes(hx, 9)),
         "add_primes_n17": ({}, lambda hx: add_primes(hx, 17)),
         "add_primes_n17_no_mfma_ext": (VALU, lambda hx: add_primes(hx, 17)),
         "add_primes_n41": ({}, lambda hx: add_primes(hx, 41)),
         "add_primes_n4_mfma_min_n_4": (MFMA4, lambda hx: add_primes(hx, 4)),
         "to_poly_mod_7_n3": ({}, lambda hx: to_poly_mod(hx, 3, 7)),
         "break_into_digits_9_prime_digit": ({}, lambda hx: break_digits(hx, 9))}


@pytest.mark.parametrize("name", list(CASES))
def test_route_launches_and_words(hx, monkeypatch, name):
    env, case = CASES[name]
    for k in SWITCHES:      # (a context snapshots the switches when it is created: the case creates its own)
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    table = case(hx)
    assert table == EXPECTED[name], (name, table)


def test_tables_read_as_the_routes_they_stand_for():
    """the recorded tables name the route of each case: Garner, HPS on the matrix cores or on the VALU with the Garner
    pass over the redo list behind it (64 workgroups), wide likewise, generic; 384 words are 2 workgroups of 256"""
    def row(name, kernel):
        hit = [r for r in EXPECTED[name] if r[0].startswith("hx::" + kernel)]
        assert len(hit) == 1, (name, kernel, EXPECTED[name])
        return hit[0][1:]

    assert row("add_primes_n1", "rns_extend_fast_kernel<1, false>") == (2, 256, 1)
    assert row("add_primes_n8", "rns_extend_fast_kernel<8, false>") == (2, 256, 1)
    assert row("add_primes_n9", "rns_extend_mfma_kernel")[2] == 1
    assert row("add_primes_n9", "rns_extend_fast_kernel<9, false>") == (64, 256, 1)
    assert row("add_primes_n9_no_mfma_ext", "rns_extend_fast_kernel<9, true>") == (2, 256, 1)
    assert row("add_primes_n9_no_mfma_ext", "rns_extend_fast_kernel<9, false>") == (64, 256, 1)
    assert row("add_primes_n17", "rns_extend_mfma_kernel")[2] == 1
    assert row("add_primes_n17", "rns_extend_kernel<40>") == (64, 256, 1)
    assert row("add_primes_n17_no_mfma_ext", "rns_extend_wide_kernel<20>")[2] == 1
    assert row("add_primes_n17_no_mfma_ext", "rns_extend_kernel<40>") == (64, 256, 1)
    assert row("add_primes_n41", "rns_extend_kernel<64>") == (2, 256, 1)
    assert row("add_primes_n4_mfma_min_n_4", "rns_extend_mfma_kernel")[2] == 1
    assert row("add_primes_n4_mfma_min_n_4", "rns_extend_fast_kernel<4, false>") == (64, 256, 1)
    assert row("to_poly_mod_7_n3", "rns_extend_kernel<8>") == (2, 256, 1)
    assert row("break_into_digits_9_prime_digit", "rns_extend_fast_kernel<9, false>") == (2, 256, 1)
    assert row("break_into_digits_9_prime_digit", "rns_extend_fast_kernel<4, false>") == (2, 256, 1)


if __name__ == "__main__":   # the recording helper: prints the table of every case as the EXPECTED literal
    import pprint
    import torch  # noqa: F401   (before this library touches the device, as in the fixture)
    from helib_amd import capi
    seen = {}
    for case_name, (case_env, run) in CASES.items():
        for key in SWITCHES:
            os.environ.pop(key, None)
        os.environ.update(case_env)
        seen[case_name] = run(capi)
    print("EXPECTED = " + pprint.pformat(seen, width=118))
