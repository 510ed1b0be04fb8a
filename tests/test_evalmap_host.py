"""The powerful basis, the tables over supplied generators and EvalMap on the CPU: helib_amd/csrc/powerful.h's tables and
the pass list the device kernel runs (replayed on the host by tests/cpp/powerful_dump.cpp) against tests/powerful_ref.py,
build_gf over supplied generators, helib_amd.evalmap on the plain side against F(eta^(1/t_i)) by Horner, and the whole
map homomorphically over the CPU oracle backend.  No GPU."""
import functools
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bgv_gr_tables as T
from tests import evalmap_tables as E
from tests import powerful_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "powerful_dump.cpp")
# the last five are not squarefree or not odd: e > 1 in a per-factor dimension, and the factors 4 and 8, whose reduction
# is a reversal, a copy and a subtraction (no binomial of theirs is short enough to act)
MVECS = [(3, 5), (3, 35), (3, 19), (7, 3, 65), (17, 257), (7, 3, 221), (31,), (9, 5), (4, 5), (25, 3), (8, 15), (7, 5, 9, 13)]
Q60 = (1 << 60) - 93                                                    # a 60-bit prime
MODULI = (2, 49, Q60)


@functools.lru_cache(maxsize=None)
def _exe(sanitize=False):
    exe = os.path.join(tempfile.mkdtemp(prefix="powerful_dump_"), "powerful_dump")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe])
    return exe


def _run(args, text=None, sanitize=False):
    return subprocess.run([_exe(sanitize)] + [str(x) for x in args], input=text, capture_output=True, text=True, timeout=300,
                          check=True).stdout.splitlines()


def _rows(mvec, q):
    n = PR.indexes(mvec).phim
    rng = random.Random(n + q % 1000)
    return [[rng.randrange(q) for _ in range(n)], [q - 1] * n, [0] * (n - 1) + [1]]


def _convert(mvec, q, to_powerful, rows, sanitize=False):
    text = "\n".join(" ".join(map(str, r)) for r in rows) + "\n"
    return [[int(x) for x in line.split()] for line in _run(["conv", int(to_powerful), q, *mvec], text, sanitize)]


# ---- (a) the tables and both conversions ----
def test_the_60_bit_modulus_is_a_prime():
    from helib_amd import hostnt
    assert Q60.bit_length() == 60 and hostnt.is_prime(Q60)


@pytest.mark.parametrize("mvec", MVECS)
def test_tables_are_the_reference_maps(mvec):
    ix = PR.indexes(mvec)
    out = _run(["tables", *mvec])
    assert out[0].split() == ["ok", str(ix.m), str(ix.phim), str(len(mvec))]
    body = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out[1:5]}
    assert body["phivec"] == ix.phivec
    assert body["s2e"] == ix.shortToExp                                 # cubeToPolyMap o shortToLongMap
    assert body["p2c"] == ix.polyToCubeMap
    assert body["s2l"] == ix.shortToLongMap
    for line, n in zip(out[5:], list(mvec) + [ix.m]):
        mt = re.fullmatch(r"(\d+) num((?: \d+)*) den((?: \d+)*)", line)
        num, den = PR.binomials(n)
        assert int(mt.group(1)) == n and [int(x) for x in mt.group(2).split()] == num and [int(x) for x in mt.group(3).split()] == den
        # the lists do give Phi_n: prod_num (x^e - 1) = Phi_n prod_den (x^e - 1) / (x^n - 1) over the integers
        lhs, rhs = [1], list(PR.cyclotomic(n))
        for e in num + [n]:
            lhs = _times_binomial(lhs, e)
        for e in den:
            rhs = _times_binomial(rhs, e)
        assert lhs == rhs
    assert out[5 + len(mvec) + 1].startswith("passes ")


def _times_binomial(f, e):
    out = [0] * (len(f) + e)
    for i, c in enumerate(f):
        out[i + e] += c
        out[i] -= c
    return out


@pytest.mark.parametrize("mvec", MVECS)
def test_the_pass_list_converts_as_the_definition_does(mvec):
    from helib_amd import powerful as PW
    conv = PW.PowerfulConversion(mvec)
    pix = conv.indexes
    ix = PR.indexes(mvec)
    assert (pix.m, pix.phim, pix.phivec) == (ix.m, ix.phim, ix.phivec)
    assert pix.polyToCubeMap.tolist() == ix.polyToCubeMap and pix.cubeToPolyMap.tolist() == ix.cubeToPolyMap
    assert pix.shortToLongMap.tolist() == ix.shortToLongMap
    for q in MODULI:
        rows = _rows(mvec, q)
        cubes = [PR.poly_to_powerful(r, mvec, q) for r in rows]
        assert _convert(mvec, q, True, rows) == cubes, q
        assert conv.polyToPowerful(np.array(rows, dtype=np.int64), q).tolist() == cubes, q          # the numpy form
        polys = [PR.powerful_to_poly(r, mvec, q) for r in rows]
        assert _convert(mvec, q, False, rows) == polys, q
        assert conv.powerfulToPoly(np.array(rows, dtype=np.int64), q).tolist() == polys, q
        assert _convert(mvec, q, False, cubes) == rows, q                                          # the round trip


def test_the_replay_is_clean_under_the_sanitizers():
    for mvec in ((3, 35), (7, 3, 65), (17, 257), (31,), (9, 5), (4, 5), (7, 5, 9, 13)):
        q = Q60
        rows = _rows(mvec, q)
        assert _run(["tables", *mvec], sanitize=True) == _run(["tables", *mvec])
        cubes = _convert(mvec, q, True, rows, sanitize=True)
        assert cubes == [PR.poly_to_powerful(r, mvec, q) for r in rows]
        assert _convert(mvec, q, False, cubes, sanitize=True) == rows


def test_census_of_the_division_passes_the_device_tests_run():
    """Which forms of the "divide by 1 - x^e" pass, and which degenerate pass lists, the factorisations of
    tests/test_evalmap_gpu.py reach between them -- derived from the definition of the conversions
    (tests/powerful_ref.py: reductions, remainder_steps), with the kernel's figures restated: a workgroup of 1024 threads;
    chains = fibres x e running sums; at 1024 chains or more a thread walks a chain, below that a chain is cut into
    S = floor(1024 / chains) segments and the threads past S x chains idle."""
    from tests import test_evalmap_gpu as G
    T = 1024
    assert [mv for mv, _ in PR.DEVICE_MVECS] == G.MVECS and set(MVECS) >= set(G.MVECS)
    seen = set()
    for mvec in G.MVECS:
        counts = {"to_powerful": 0, "to_poly": 0}
        for direction, n, ph, stride, nouter in PR.reductions(mvec):
            steps = PR.remainder_steps(n)
            counts[direction] += len(steps)
            acting = [st for st in steps if st[1] in ("MUL", "DIV")]
            if not any(st[1] == "DIV" for st in acting if st[0] == "quotient"):
                seen.add("no DIV in the quotient half")
            if not acting:
                seen.add("a reduction without MUL or DIV: n = %d" % n)
            for half, op, e, L in steps:
                if op != "DIV":
                    continue
                assert 1 <= e < L <= n
                chains = nouter * stride * e
                if direction == "to_powerful" and e > 1 and len(PR.binomials(n)[1]) == 1:
                    seen.add("e > 1 in the dimension of a prime power")
                if chains >= T:
                    seen.add("a thread walks a chain")
                    continue
                S = T // chains
                longest = -(-L // e)                                     # the words of the longest chain
                if S == 1 and T - chains > 0:
                    seen.add("S = 1 with an idle tail")
                if S > longest:
                    seen.add("more segments than words")
                if S == T:
                    seen.add("one chain: the scan of a single fibre")
                if 1 < S <= longest and T - S * chains > 0:
                    seen.add("segments of several words with an idle tail")
        # the pass list that the kernel runs has exactly these steps (tests/cpp/powerful_dump.cpp prints its lengths)
        assert _run(["tables", *mvec])[-1].split() == ["passes", str(counts["to_powerful"]), str(counts["to_poly"])], mvec
    assert seen == {"no DIV in the quotient half", "a reduction without MUL or DIV: n = 4", "a reduction without MUL or DIV: n = 8",
                    "e > 1 in the dimension of a prime power", "a thread walks a chain", "S = 1 with an idle tail",
                    "more segments than words", "one chain: the scan of a single fibre",
                    "segments of several words with an idle tail"}, sorted(seen)
    # the two that tests/test_evalmap_gpu.py converts with more items than workgroups: the smallest, and the one that
    # walks chains
    assert PR.MANY_ITEMS == [G.MVECS[0], (7, 3, 221)] and min(G.MVECS, key=lambda mv: PR.indexes(mv).m) == (3, 5)
    assert any(nouter * stride * e >= T for _, n, _, stride, nouter in PR.reductions((7, 3, 221))
               for _, op, e, _ in PR.remainder_steps(n) if op == "DIV")


def test_bad_factorisations_are_refused():
    from helib_amd import powerful as PW
    from helib_amd.ckks import LogicError
    assert "not coprime" in _run(["tables", 3, 15])[0]
    assert "at least 2" in _run(["tables", 1, 15])[0]
    with pytest.raises(LogicError, match="not coprime"):
        PW.PowerfulTranslationIndexes((3, 15))
    with pytest.raises(LogicError, match="at least 2"):
        PW.PowerfulTranslationIndexes((1, 15))
    conv = PW.PowerfulConversion((3, 5))
    for q in (1, 1 << 62):
        with pytest.raises(LogicError, match="not in"):
            conv.polyToPowerful(np.zeros((1, 8), dtype=np.int64), q)
    with pytest.raises(LogicError, match="capi.Context"):
        PW.PowerfulDCRT(None, (3, 5))


# ---- (b) build_gf over supplied generators ----
@pytest.mark.parametrize("ring", E.RINGS, ids=lambda x: "m%d" % int(np.prod(x[2])))
def test_supplied_generators_order_the_slots(ring):
    from helib_amd import hostnt
    p, rs, mvec, gens, ords = ring
    m = int(np.prod(mvec))
    z = hostnt.ZmStar(m, p, gens, ords)
    for r in rs:
        t = E.dump(m, p, r, tuple(gens), tuple(ords))
        assert "error" not in t, t
        assert t["gens"] == list(gens) and t["ords"] == z.signedOrds() and t["nslots"] == z.getNSlots() and t["d"] == z.ordP
        # the sign is recomputed, not trusted
        flipped = E.raw(m, p, r, gens, [-o for o in ords], "geom").splitlines()
        assert [int(x) for x in flipped[2].split()] == z.signedOrds()
        # factor i is the minimal polynomial of eta^(1/t_i): slot i belongs to the representative ith_rep(i)
        G, P, d = t["G"], p ** r, t["d"]
        for i, ti in enumerate(z.reps()):
            root = E.eta_pow(pow(ti, -1, m), G, P)
            acc = [0] * d
            for c in reversed(t["F"][i]):
                acc = E.ring_mul(acc, root, G, P)
                acc[0] = (acc[0] + c) % P
            assert not any(acc), (r, i)


@pytest.mark.parametrize("m,p,r", [(85, 2, 4), (57, 7, 2), (15, 2, 1)])
def test_no_generators_are_the_tables_of_today(m, p, r):
    assert E.raw(m, p, r, (), ()) == T.raw(m, p, r)


def test_generators_that_do_not_enumerate_the_quotient_are_refused():
    def err(m, p, gens, ords):
        line = E.raw(m, p, 1, gens, ords, "geom").splitlines()[0]
        assert line.startswith("error generators: "), line
        return line
    assert "enumerate" in err(85, 2, (52, 52), (4, 2))                  # the same generator twice
    assert "enumerate" in err(85, 2, (52, 16), (4, 2))                  # 16 = 2^4 lies in <p>
    assert "not coprime" in err(85, 2, (5,), (8,)) and "m = 85" in err(85, 2, (5,), (8,))
    assert "multiply to 16" in err(85, 2, (52, 71), (4, 4))
    assert "9 generators" in err(85, 2, (3,) * 9, (1,) * 9)
    assert "does not fit" in err(85, 2, (52, 71), (4, 0))


# ---- (c) EvalMap on the plain side ----
@pytest.mark.parametrize("ring", E.RINGS, ids=lambda x: "m%d" % int(np.prod(x[2])))
def test_forward_map_gives_the_slots_of_F_and_the_inverse_the_cube(ring):
    from helib_amd import evalmap, intraslot
    p, rs, mvec, gens, ords = ring
    m = int(np.prod(mvec))
    for r in rs:
        P = p ** r
        ea = E.plain_ea(m, p, r, gens, ords)
        n, d = ea.size(), ea.getDegree()
        F = [int(x) for x in np.random.default_rng(m + r).integers(0, P, size=n * d)]
        cube = np.array(PR.poly_to_powerful(F, mvec, P), dtype=np.int64).reshape(1, n, d)
        slots = evalmap.EvalMap(ea, mvec).applyPlain(cube)
        assert slots[0].tolist() == E.slots_of(F, ea.zMStar, ea.G, P), r
        assert np.array_equal(evalmap.EvalMap(ea, mvec, invert=True).applyPlain(slots), cube), r
        CB = intraslot.normalBasisMatrices(ea)[0]
        nb = evalmap.EvalMap(ea, mvec, invert=True, normal_basis=True).applyPlain(slots)
        assert np.array_equal(nb, np.array(cube.astype(object) @ CB.astype(object) % P, dtype=np.int64)), r


def test_evalmap_refusals():
    from helib_amd import bgv_gr_matmul, evalmap
    from helib_amd.ckks import LogicError
    ea = E.plain_ea(85, 2, 4, (), ())                                   # the library's own generators: one of order 8
    with pytest.raises(LogicError, match=r"sig->getDim\(dim\) must equal reps.length\(\)"):
        evalmap.EvalMap(ea, (5, 17))
    ea = E.plain_ea(85, 2, 4, (52, 71), (4, -2))
    with pytest.raises(LogicError, match="pairwise co-prime"):
        evalmap.EvalMap(ea, (5, 85))
    with pytest.raises(LogicError, match="does not match ea.zMStar.getM"):
        evalmap.EvalMap(ea, (5, 19))
    with pytest.raises(LogicError, match="must not be empty"):
        evalmap.EvalMap(ea, ())
    with pytest.raises(LogicError, match="bad inertPrefix"):
        evalmap.EvalMap(ea, (17, 5))                                    # the factor that carries d has to come last
    with pytest.raises(LogicError, match="bad inertPrefix"):
        evalmap.EvalMap(E.plain_ea(35, 2, 1, (), ()), (7, 5))           # d = 12 is split 3 x 4 over the two factors
    for name in ("ThinEvalMap", "RecryptData", "reCrypt"):
        with pytest.raises(LogicError, match="not built"):
            getattr(evalmap, name)()
    with pytest.raises(LogicError, match="EvalMap is not built"):
        bgv_gr_matmul.EvalMap()                                         # the old stub stays
    with pytest.raises(LogicError, match="injected"):
        from helib_amd import bgv_gr
        bgv_gr.EncryptedArray(ea.cc, None, encoder=ea.enc, gens=(52, 71), ords=(4, -2))


# ---- (d) the whole map over the CPU oracle backend ----
# The chain: on this code isCorrect() holds after the last step from bits = 100 on (the smallest multiple of 100) at both
# rings and in both directions; the tests (and tests/test_evalmap_gpu.py) run at that plus 100.
BITS_MIN, BITS = 100, 200


@pytest.mark.parametrize("m,r", [(15, 4), (105, 3)])
def test_whole_map_over_the_oracle_backend(m, r):
    from helib_amd import evalmap
    p, _, mvec, gens, ords = E.ring(m)
    S = E.setup(m, p, r, gens, ords, BITS)
    ea, P = S.ea, p ** r
    assert ea.zMStar.gens == list(gens) and ea.zMStar.signedOrds() == E.dump(m, p, r, tuple(gens), tuple(ords))["ords"]
    n, d = ea.size(), ea.getDegree()
    F = [int(x) for x in np.random.default_rng(m).integers(0, P, size=n * d)]
    cube = np.array(PR.poly_to_powerful(F, mvec, P), dtype=np.int64).reshape(1, n, d)
    fw = evalmap.EvalMap(ea, mvec)
    ct = ea.encrypt(S.sk, cube)
    fw.apply(ct, pk=S.sk)
    assert ct.isCorrect()
    slots = ea.decrypt_batch(ct, S.sk)
    assert np.array_equal(slots, fw.applyPlain(cube)) and slots[0].tolist() == E.slots_of(F, ea.zMStar, ea.G, P)
    inv = evalmap.EvalMap(ea, mvec, invert=True)
    inv.apply(ct, pk=S.sk)
    assert ct.isCorrect()
    assert np.array_equal(ea.decrypt_batch(ct, S.sk), cube)
    assert not fw.mat1.onDevice and fw.mat1.fusedConstants is False     # the table encoder has no device path


# ---- (e) declarations ----
NAMES = {"hx_bgv_gf_create_gens": 7, "hx_powerful_create": 4, "hx_powerful_destroy": 1, "hx_poly_to_powerful": 2,
         "hx_powerful_to_poly": 2, "hx_powerful_words": 6}


def test_symbols_are_declared_listed_and_exported():
    from helib_amd import build, capi
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    for name, nargs in NAMES.items():
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS, name
        assert re.search(r" T %s$" % name, dyn, re.M), name
        assert len(getattr(lib, name).argtypes) == nargs
    for cite in ("src/powerful.cpp:22-190", "src/powerful.cpp:354-383", "src/PAlgebra.cpp:476-509", "src/EvalMap.cpp:42-105"):
        assert cite in header, cite
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "powerful_kernel" in text
    assert len(lib.hx_bgv_gf_create_pr.argtypes) == 4 and len(lib.hx_bgv_gf_create.argtypes) == 3           # left alone
