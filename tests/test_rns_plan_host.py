"""The exact-RNS plan builder and route function (helib_amd/csrc/rns_plan.h) on the CPU, word for word.

tests/cpp/rns_plan_test.cpp prints every section, scalar and flag of the plan rns_plan.h builds for a case given on
its command line, the matrix-core table read back through mfma_ext.h's own index functions, and the route of a launch.
Here every word is recomputed from Python integers and compared exactly: P mod t, P^-1 mod t, the Garner inverses,
(P - 1)/2 in mixed radix, every Shoup companion as floor(w 2^64 / q), the Barrett constants, the HPS inverses and
multipliers, the Montgomery forms of a Proth-form target's record, the 30-bit limb pairs of the wide record, the flags.
The program is built with plain g++ -std=c++17 -Wall -Werror (the header may not need HIP), and once more with
-fsanitize=address,undefined, which runs the same cases."""
import itertools
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rns_plan_test.cpp")
R64 = 1 << 64
ERRORS = {"OUT_OF_RANGE": 1, "NOT_COPRIME": 2, "NOT_INVERTIBLE_TGT": 3, "NOT_INVERTIBLE_PTXT": 4}
MAX_ROWS = 160   # dev_common.h


# ---------------------------------------------------------------- primes
def is_prime(n):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in small:
        if n % b == 0:
            return n == b
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for b in small:   # deterministic below 3.3e24
        x = pow(b, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_below(top, count, step=2, skip=()):
    out, q = [], top - 1 if top % 2 == 0 else top - 2
    while len(out) < count:
        if is_prime(q) and q not in skip:
            out.append(q)
        q -= step
    return out


def proth_primes(count, start=(1 << 28) - 1):
    """q = qh 2^32 + 1 below 2^60 (ntt_core.h is_proth32), descending from the largest"""
    out, qh = [], start
    while len(out) < count:
        q = (qh << 32) + 1
        if is_prime(q):
            out.append(q)
        qh -= 1
    return out


P60 = primes_below(1 << 60, 48)            # context-sized primes, descending: P60[::-1] ascends
P56 = primes_below(1 << 56, 3)
P45 = primes_below(1 << 45, 2)
PROTH = proth_primes(12)
SMALL = primes_below(1 << 32, 1)[0]        # one prime below 2^32
P38 = primes_below(1 << 38, 1)[0]
EXPLICIT = [2, 7, (1 << 60) - 1]


def sources(n, ordering):
    asc = sorted(P60[:n])
    if ordering == "ascending":
        return asc
    if ordering == "proth":               # all Proth-form, descending (within a factor of two: garner_cs holds)
        return PROTH[:n]
    # neither ascending nor within a factor of two: a 38-bit prime behind 60-bit ones (garner_cs off)
    return (asc[:-1] + [P38]) if n > 1 else asc


TARGET_KINDS = {"context": lambda src: [q for q in P60[::-1] if q not in src][:6] + P56 + P45,
                "proth": lambda src: [q for q in PROTH[::-1] if q not in src][:3] + [q for q in P60 if q not in src][:2],
                "small": lambda src: [q for q in P60 if q not in src][:2] + [SMALL],
                "explicit": lambda src: list(EXPLICIT)}
DEFAULT = dict(no_proth=0, no_proth_rns=0, no_mfma_ext=0, mfma_min_n=9)
SWITCHES = {"default": DEFAULT, "no_proth_rns": dict(DEFAULT, no_proth_rns=1), "no_mfma_ext": dict(DEFAULT, no_mfma_ext=1),
            "mfma_min_n=4": dict(DEFAULT, mfma_min_n=4)}
NS = (1, 2, 8, 9, 16, 17, 40, 41)


def all_cases():
    """(id, scaled, ptxt, switches, sources, targets).  The full product of the issue's table is 8 x 4 x 2 x 8 x 4; what
    runs is every n with every target kind and both orderings at ptxt 0 and the defaults, and for every n every ptxt,
    plain and scaled, and every switch against the target kind it bears on (Proth-form targets for no_proth_rns, context
    ones for the matrix-core switches), plus Proth-form sources."""
    out = []
    for n, kind, ordering in itertools.product(NS, TARGET_KINDS, ("ascending", "unordered")):
        src = sources(n, ordering)
        out.append(("n%d-%s-%s" % (n, kind, ordering), 0, 0, DEFAULT, src, TARGET_KINDS[kind](src)))
    for n in NS:
        src = sources(n, "ascending")
        for kind in ("context", "proth"):
            tgt = TARGET_KINDS[kind](src)
            for ptxt in (2, 4, 65537, 1 << 40):
                out.append(("n%d-%s-plain-ptxt%d" % (n, kind, ptxt), 0, ptxt, DEFAULT, src, tgt))
            for ptxt in (0, 2, 65537):
                out.append(("n%d-%s-scaled-ptxt%d" % (n, kind, ptxt), 1, ptxt, DEFAULT, src, tgt))
        out.append(("n%d-small-scaled-ptxt2" % n, 1, 2, DEFAULT, src, TARGET_KINDS["small"](src)))
        for name, sw in SWITCHES.items():
            if name == "default":
                continue
            kind = "proth" if name == "no_proth_rns" else "context"
            for scaled, ptxt in ((0, 0), (1, 65537)):
                out.append(("n%d-%s-%s-%d" % (n, kind, name, scaled), scaled, ptxt, sw, src, TARGET_KINDS[kind](src)))
        if n <= 8:
            src = sources(n, "proth")
            for name in ("default", "no_proth_rns"):
                out.append(("n%d-proth-sources-%s" % (n, name), 0, 65537, SWITCHES[name], src, TARGET_KINDS["proth"](src)))
    out.append(("n3-no_proth", 0, 0, dict(DEFAULT, no_proth=1), sources(3, "ascending"), TARGET_KINDS["proth"](sources(3, "ascending"))))
    return out


ERROR_CASES = [("not_coprime", "NOT_COPRIME", 0, 0, [P60[0], 3 * 5, 5 * 7], [P60[1]]),
               ("not_invertible_tgt", "NOT_INVERTIBLE_TGT", 1, 0, [P45[0], P60[0]], [3 * P45[0]]),
               ("not_invertible_ptxt", "NOT_INVERTIBLE_PTXT", 0, 3 * P56[0], [P60[0], P56[0]], [P60[1]]),
               ("source_2^60", "OUT_OF_RANGE", 0, 0, [P60[0], (1 << 60) + 33], [P60[1]]),
               ("target_2^60", "OUT_OF_RANGE", 0, 0, [P60[0]], [1 << 60]),
               ("target_1", "OUT_OF_RANGE", 0, 0, [P60[0]], [1])]


# ---------------------------------------------------------------- the program
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rns_plan") / ("rns_plan_test_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def plan(exe, scaled, ptxt, sw, src, tgt):
    lines = run(exe, "plan", scaled, ptxt, sw["no_proth"], sw["no_proth_rns"], sw["no_mfma_ext"], sw["mfma_min_n"],
                len(src), *src, len(tgt), *tgt)
    got = {"scalar": {}, "section": {}, "offset": {}, "mfma_w": {}, "mfma_x": {}}
    for line in lines:
        f = line.split()
        if f[0] == "err":
            got["err"] = int(f[1])
        elif f[0] == "scalar":
            got["scalar"][f[1]] = int(f[2])
        elif f[0] == "section":
            assert int(f[3]) == len(f) - 4
            got["offset"][f[1]] = int(f[2])
            got["section"][f[1]] = [int(x, 16) for x in f[4:]]
        elif f[0] == "mfma":
            got["mfma_bytes"] = int(f[1])
        elif f[0] == "mfma_w":
            got["mfma_w"][tuple(int(x) for x in f[1:4])] = [int(x) for x in f[4:]]
        elif f[0] == "mfma_x":
            got["mfma_x"][int(f[1])] = [int(x) for x in f[2:]]
        elif f[0] == "mfma_stray":
            got["mfma_stray"] = int(f[1])
    return got


# ---------------------------------------------------------------- the expectation, from Python integers
def shoup(w, q):
    return (w << 64) // q


def tw(ws, q):
    return [x for w in ws for x in (w, shoup(w, q))]


def inv(a, q):
    try:
        return pow(a, -1, q)
    except ValueError:
        return 0


def u32s(vals):
    vals = list(vals)
    vals += [0] * (len(vals) % 2)
    return [vals[i] | (vals[i + 1] << 32) for i in range(0, len(vals), 2)]


def is_proth(q):
    return q & 0xffffffff == 1 and q >> 32 != 0 and q < 1 << 60


def prod(xs):
    r = 1
    for x in xs:
        r *= x
    return r


def balanced_limbs(v):
    """v < 2^63 as seven signed 8-bit digits and a small non-negative top one (mfma_ext.h pack_balanced)"""
    out = []
    for _ in range(7):
        d = (v + 128) % 256 - 128
        out.append(d)
        v = (v - d) >> 8
    assert 0 <= v <= 127
    return out + [v]


def expected(scaled, ptxt, sw, p, tq):
    n, nt = len(p), len(tq)
    P = prod(p)
    wide_cand = 16 < n <= 40
    mfma_small = sw["mfma_min_n"] <= n <= 16 and n >= 4 and not sw["no_mfma_ext"]
    rns_proth = not sw["no_proth"] and not sw["no_proth_rns"] and n <= 16
    hps_tables = n >= 2 and n <= 40 and (ptxt <= 1 or ptxt < 1 << (56 if wide_cand else 58))
    mont = [rns_proth and is_proth(t) for t in tq]
    sec, sc = {}, {}
    sec["src_q"] = list(p)
    sec["src_mu64"] = [R64 // q for q in p]
    sec["src_rq"] = [struct.unpack("<Q", struct.pack("<d", 1.0 / float(q)))[0] for q in p]
    ginv = [[inv(p[l], p[k]) if l < k else 0 for l in range(n)] for k in range(n)]
    sec["ginv"] = [x for k in range(n) for x in tw(ginv[k], p[k])]
    sec["ginv_m"] = [(ginv[k][l] << 64) % p[k] for k in range(n) for l in range(n)]
    half, h = [], (P - 1) // 2
    for q in p:
        half.append(h % q)
        h //= q
    sec["half"] = half
    sec["tgt_q"] = list(tq)
    sec["tgt_mu64"] = [R64 // t for t in tq]
    sec["tgt_mu"] = [(1 << (2 * t.bit_length())) // t for t in tq]
    sec["tgt_k"] = u32s(t.bit_length() for t in tq)
    sec["tgt_lazy"] = u32s(int(sum(p) <= 8 * t) for t in tq)
    pinv = [inv(P, t) for t in tq]
    fac = [pinv[i] if scaled else 1 for i in range(nt)]
    pmod = [(1 if scaled else P) % t for t in tq]
    garner = [[prod(p[:k]) * fac[i] % t for k in range(n)] for i, t in enumerate(tq)]
    hps = [[P // p[k] * fac[i] % t for k in range(n)] for i, t in enumerate(tq)]
    sec["pmod"] = pmod
    sec["W"] = [x for i, t in enumerate(tq) for x in tw(garner[i], t)]
    sec["upd"] = [x for i, t in enumerate(tq) for x in tw([pinv[i]], t)]
    live = ptxt > 1
    sec["Wp"] = tw([prod(p[:k]) % ptxt for k in range(n)], ptxt) if live else [0] * (2 * n)
    sec["hps_inv"] = [x for k in range(n) for x in tw([inv(P // p[k], p[k])], p[k])] if hps_tables else [0] * (2 * n)
    sec["Wp_hps"] = tw([P // p[k] % ptxt for k in range(n)], ptxt) if hps_tables and live else [0] * (2 * n)

    def record(i, mult, slack):
        t, k = tq[i], tq[i].bit_length()
        lazy, chunk7 = int(sum(p) + slack <= 8 * t), int(max(p) <= t)
        m64 = (lambda x: (x << 64) % t) if mont[i] else (lambda x: x)
        return ([t, pmod[i], m64((t - pmod[i]) % t) if mont[i] else (1 << (63 + k)) // t % R64, R64 // t,
                 k | lazy << 8 | chunk7 << 9 | int(mont[i]) << 10, pinv[i], shoup(pinv[i], t), (1 << (2 * k)) // t]
                + [m64(w) for w in mult] + [shoup(w, t) for w in mult]
                + [m64(pinv[i]) if mont[i] else R64 % t, shoup(R64 % t, t)])

    stride = 10 + 2 * n
    sec["tgt_pack"] = [x for i in range(nt) for x in record(i, garner[i], 0)]
    sec["tgt_pack_hps"] = ([x for i in range(nt) for x in record(i, hps[i], 32)] if hps_tables and not wide_cand
                           else [0] * (nt * stride))
    wide_rec = wide_cand or mfma_small
    wstride = 8 + (n + 3) // 4 * 4
    if not wide_rec:
        sec["wide_pack"] = []
    elif not hps_tables:
        sec["wide_pack"] = [0] * (nt * wstride)
    else:
        sec["wide_pack"] = [x for i, t in enumerate(tq) for x in
                            [t, pmod[i], R64 % t, shoup(R64 % t, t), R64 // t, pinv[i], shoup(pinv[i], t), shoup(pmod[i], t)]
                            + [(w & 0x3fffffff) | (w >> 30) << 32 for w in hps[i]] + [0] * (wstride - 8 - n)]
    big = min(p) >> 32 != 0 and all(t >> 32 != 0 for t in tq)
    garner_cs = max(p) // 2 < min(p) or list(p) == sorted(p)
    fast16 = garner_cs and big and n <= 16
    hps_ok = fast16 and hps_tables
    wide_ok = big and wide_cand and hps_tables
    mfma = not sw["no_mfma_ext"] and (wide_ok or (hps_ok and mfma_small))
    sc.update(n=n, nt=nt, garner_cs=int(garner_cs), fast_ok=int(fast16 and n <= 8), fast16_ok=int(fast16), hps_ok=int(hps_ok),
              wide_ok=int(wide_ok), mfma_steps=(n + 4) // 4 if mfma else 0,
              lazy_tight_ok=int(bool(sw["no_proth"]) or rns_proth or not any(is_proth(t) for t in tq)),
              src_mont=int(rns_proth and all(is_proth(q) for q in p)),
              corr_unit=int(bool(scaled) and live and all(ptxt <= t for t in tq)),
              hps_eps=struct.unpack("<Q", struct.pack("<d", 2.0 ** -30))[0])
    k = ptxt.bit_length()
    sc.update(ptxt=ptxt, ptxt_mu64=R64 // ptxt, ptxt_k=k, ptxt_mu=(1 << (2 * k)) // ptxt, pinv_ptxt=inv(P, ptxt), pmod_ptxt=P % ptxt) \
        if live else sc.update(ptxt=0, ptxt_mu64=0, ptxt_k=0, ptxt_mu=0, pinv_ptxt=0, pmod_ptxt=0)
    return sec, sc, (hps, pmod, pinv) if mfma else None


def check_mfma(got, n, tq, hps, pmod, pinv):
    steps = (n + 4) // 4
    slots, base = 4 * steps, steps * 32 * 16384
    assert got["mfma_bytes"] == (len(tq) + 3) // 4 * (steps * 64 + 16) * 16
    assert got["mfma_stray"] == 0
    for i, t in enumerate(tq):
        for k in range(slots):
            m = hps[i][k] if k < n else (t - pmod[i]) % t if k == slots - 1 else 0
            for a in range(8):
                assert got["mfma_w"][(i, k, a)] == balanced_limbs((m << (8 * a)) % t), (i, k, a)
        D = -(base * sum(1 << (8 * b) for b in range(8))) % t
        init = [base + ((D >> (8 * b)) & 0xff if b < 7 else D >> 56) for b in range(8)]
        s = shoup(pinv[i], t)
        want = init + [(1 << 80) // t if t >> 48 else 0, t & 0xffffffff, t >> 32,
                       pinv[i] & 0xffffffff, pinv[i] >> 32, s & 0xffffffff, s >> 32]
        assert got["mfma_x"][i] == want, i


# ---------------------------------------------------------------- the tests
CASES = all_cases()


def test_case_table_covers_what_it_says():
    assert len({c[0] for c in CASES}) == len(CASES)
    assert {len(c[4]) for c in CASES} >= set(NS)
    assert all(is_proth(q) for q in PROTH) and SMALL < 1 << 32 and not is_proth(P60[0])
    assert all(q.bit_length() == 60 for q in P60)


@pytest.mark.parametrize("chunk", range(8))
def test_every_word_of_the_plan_from_python_integers(exe, chunk):
    """one eighth of the case table per test, every case one run of the program"""
    for name, scaled, ptxt, sw, src, tgt in CASES[chunk::8]:
        got = plan(exe, scaled, ptxt, sw, src, tgt)
        assert got["err"] == 0, name
        sec, sc, mfma = expected(scaled, ptxt, sw, src, tgt)
        assert got["scalar"] == sc, (name, {k: (got["scalar"].get(k), v) for k, v in sc.items() if got["scalar"].get(k) != v})
        assert set(got["section"]) == set(sec), name
        for s, want in sec.items():
            assert got["section"][s] == want, (name, s, [i for i, (a, b) in enumerate(zip(got["section"][s], want)) if a != b][:8])
        # the sections tile the blob in 16-byte steps, in order, and nothing overlaps
        at = 0
        for s, words in got["section"].items():
            if words:
                assert got["offset"][s] == at and at % 2 == 0, (name, s)
                at += len(words) + len(words) % 2
        if mfma:
            check_mfma(got, len(src), tgt, *mfma)
        else:
            assert got["mfma_bytes"] == 0, name


@pytest.mark.parametrize("case", ERROR_CASES, ids=[c[0] for c in ERROR_CASES])
def test_arithmetic_errors_and_the_precondition(exe, case):
    _, want, scaled, ptxt, src, tgt = case
    got = plan(exe, scaled, ptxt, DEFAULT, src, tgt)
    assert got["err"] == ERRORS[want] and not got["section"]


def old_launch_extend(fast16_ok, hps_ok, wide_ok, mfma_steps, n, nt, upd, row_words, hps_min_n):
    """launch_extend's decision as it stood before the route function existed, branch for branch"""
    if fast16_ok:
        mfma = hps_ok and mfma_steps != 0 and not upd and row_words < 1 << 32
        hps = mfma or (hps_ok and n >= hps_min_n and not upd and row_words < 1 << 32)
        return "FAST_MFMA" if mfma else "FAST_HPS" if hps else "FAST_GARNER"
    wide_lds = nt * (8 + (n + 3) // 4 * 4) * 8
    if wide_ok and row_words < 1 << 32 and wide_lds <= 160 * 1024:
        return "WIDE_MFMA" if mfma_steps else "WIDE_VALU"
    return "GENERIC"


ROUTE_ROWS = [  # fast16_ok hps_ok wide_ok mfma_steps n nt upd row_words hps_min_n -> route
    ((1, 0, 0, 0, 1, 11, 0, 384, 9), "FAST_GARNER"),          # no HPS tables
    ((1, 1, 0, 0, 8, 11, 0, 384, 9), "FAST_GARNER"),          # below hps_min_n
    ((1, 1, 0, 0, 8, 11, 0, 384, 2), "FAST_HPS"),             # HX_HPS_MIN_N=2
    ((1, 1, 0, 0, 9, 11, 0, 384, 9), "FAST_HPS"),             # HX_NO_MFMA_EXT: no table
    ((1, 1, 0, 3, 9, 11, 0, 384, 9), "FAST_MFMA"),
    ((1, 1, 0, 2, 4, 11, 0, 384, 9), "FAST_MFMA"),            # HX_MFMA_MIN_N=4: below hps_min_n too
    ((1, 1, 0, 3, 9, 11, 1, 384, 9), "FAST_GARNER"),          # args.upd set: no HPS form ...
    ((1, 1, 0, 0, 9, 11, 1, 384, 2), "FAST_GARNER"),          # ... with or without the matrix-core table
    ((1, 1, 0, 3, 9, 11, 0, 1 << 32, 9), "FAST_GARNER"),      # row_words >= 2^32: no redo list
    ((1, 1, 0, 0, 9, 11, 0, 1 << 32, 9), "FAST_GARNER"),
    ((1, 1, 0, 3, 9, 11, 0, (1 << 32) - 1, 9), "FAST_MFMA"),
    ((0, 0, 1, 5, 17, 11, 0, 384, 9), "WIDE_MFMA"),
    ((0, 0, 1, 0, 17, 11, 0, 384, 9), "WIDE_VALU"),
    ((0, 0, 1, 5, 17, 11, 1, 384, 9), "WIDE_MFMA"),           # the wide route takes in-place updates
    ((0, 0, 1, 0, 40, 11, 1, 384, 9), "WIDE_VALU"),
    ((0, 0, 1, 5, 17, 11, 0, 1 << 32, 9), "GENERIC"),         # row_words >= 2^32
    ((0, 0, 1, 0, 17, 11, 0, 1 << 32, 9), "GENERIC"),
    ((0, 0, 1, 11, 40, 426, 0, 384, 9), "WIDE_MFMA"),         # 426 * 48 * 8 = 163584 bytes of LDS: the last that fits
    ((0, 0, 1, 11, 40, 427, 0, 384, 9), "GENERIC"),           # the LDS fallthrough (beyond MAX_ROWS: unreachable today)
    ((0, 0, 1, 0, 40, 427, 0, 384, 9), "GENERIC"),
    ((0, 0, 0, 0, 3, 1, 0, 384, 9), "GENERIC"),               # a target below 2^32
    ((0, 0, 0, 0, 41, 11, 0, 384, 9), "GENERIC"),
    ((0, 0, 0, 0, 17, 11, 1, 384, 9), "GENERIC")]


def test_route_table(exe):
    flags = [(0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 5), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 3)]
    # the rows above, then the whole small product against the old decision (the flags as plans can carry them)
    rows = [a for a, _ in ROUTE_ROWS] + [(*f, n, 11, upd, rw, hmin) for f, n, upd, rw, hmin in
                                         itertools.product(flags, (1, 9, 17), (0, 1), (384, 1 << 32), (2, 9))]
    got = run(exe, "route", *[x for a in rows for x in a])
    assert len(got) == len(rows)
    for (args, want), line in zip(ROUTE_ROWS, got):
        assert line == "route " + want and old_launch_extend(*args) == want, args
    for args, line in zip(rows, got):
        assert line == "route " + old_launch_extend(*args), args
    # MAX_ROWS keeps the LDS fallthrough out of reach: the largest wide plan asks for 61440 bytes
    assert MAX_ROWS * (8 + 40) * 8 <= 160 * 1024
