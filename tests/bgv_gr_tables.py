"""TEST INFRASTRUCTURE shared by tests/test_bgv_gr_host.py and tests/test_intraslot_host.py: the tables that
helib_amd/csrc/bgv_gf.h builds on the CPU for (m, p, r) (printed by tests/cpp/bgv_gr_dump.cpp), an encoder that runs the
device kernels' steps on them in exact integers -- c = alpha A, the sliding window over E, the fold with T, u over Rx and
alpha = M u -- and a fixture that drives helib_amd.bgv_gr / bgv_gf over the oracle backend with that encoder and with
hx_mul_add_circulant stated in python integers (tests/intraslot_ref.circulant)."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests import intraslot_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bgv_gr_dump.cpp")


@functools.lru_cache(maxsize=None)
def _exe():
    exe = os.path.join(tempfile.mkdtemp(prefix="bgv_gr_dump_"), "bgv_gr_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", exe])
    return exe


def raw(m, p, r):
    """the program's output, as text (r = 0: build_gf's default argument)"""
    return subprocess.run([_exe(), str(m), str(p), str(r)], capture_output=True, text=True, timeout=300, check=True).stdout


@functools.lru_cache(maxsize=None)
def dump(m, p, r):
    out = raw(m, p, r).splitlines()
    head = out[0].split()
    if head[0] != "ok":
        return {"error": out[0][6:]}
    t = dict(zip(("m", "p", "r", "P", "d", "nslots", "phim", "ld", "ldr", "limit"), map(int, head[1:])))
    rows = [[int(x) for x in line.split()] for line in out[1:]]
    t["gens"], t["ords"], t["G"] = rows[0], rows[1], rows[2]
    n, d = t["nslots"], t["d"]
    at = 3
    for name, count in (("F", n), ("A", n), ("M", n), ("E", n), ("T", d - 1), ("Rx", n)):
        t[name] = rows[at:at + count]
        at += count
    assert at == len(rows)
    return t


class TableEncoder:
    """GrEncoder's members over the printed tables, in exact integer arithmetic (int64 where no sum can leave it)"""

    def __init__(self, m, p, r, be=None):
        t = self.t = dump(m, p, r)
        assert "error" not in t, t
        self.P, self.d, self.n, self.phim = t["P"], t["d"], t["nslots"], t["phim"]
        d = self.d
        self.G = list(t["G"])
        # int64 where no sum can leave it (every term is below p^2r), python integers otherwise
        terms = max(self.phim, self.n * d, 1)
        self.dt = dt = np.int64 if self.P * self.P * terms < 2 ** 62 else object
        self.A = np.array(t["A"], dtype=dt).reshape(self.n, d, d)
        self.M = np.array(t["M"], dtype=dt).reshape(self.n, d, d)
        self.E = np.array(t["E"], dtype=dt)
        self.T = np.array(t["T"], dtype=dt).reshape(max(d - 1, 0), self.phim)
        self.Rx = [np.lib.stride_tricks.sliding_window_view(np.array(row, dtype=dt), self.phim) for row in t["Rx"]]   # [d, phim]
        self.be = be

    def dims(self):
        return self.t["gens"], self.t["ords"]

    def _mod(self, x):
        x = np.asarray(x)
        if x.dtype == object or self.dt is object:
            return np.array([int(v) % self.P for v in x.reshape(-1)], dtype=self.dt).reshape(x.shape)
        return (x.astype(np.int64) % self.P).astype(self.dt)

    def coeffs(self, v, mul=1):
        """-> balanced(mul * H mod p^r) [B, phim]; +p^r / 2 at an even modulus, as the device"""
        P, d, n, N = self.P, self.d, self.n, self.phim
        v = self._mod(v)
        if v.ndim == 2:
            v = v[:, :, None]
        a = np.zeros((v.shape[0], n, d), dtype=self.dt)
        a[:, :v.shape[1], :v.shape[2]] = v
        out = []
        for row in a:
            W = np.zeros(N + d - 1, dtype=self.dt)
            for i in range(n):
                c = row[i].dot(self.A[i]) % P
                for j in range(d):
                    if c[j]:
                        W[j:j + N] += c[j] * self.E[i]
            W %= P
            H = W[:N]
            for u in range(d - 1):
                H = (H + W[N + u] * self.T[u]) % P
            H = H * (mul % P) % P
            out.append([int(x) - P if int(x) > P // 2 else int(x) for x in H])
        return np.array(out, dtype=np.int64)

    def slots(self, coeffs, Pk=None):
        P, n = self.P, self.n
        out = []
        for row in np.atleast_2d(np.asarray(coeffs)):
            w = self._mod(row)
            out.append([self.M[i].dot(self.Rx[i].dot(w) % P) % P for i in range(n)])
        return np.array(out, dtype=np.int64)

    # ---- the encoder's interface ----
    def encode(self, v, mul, idx, coeffs=False):
        cf = self.coeffs(v, mul)
        dd = None
        if idx:
            assert cf.shape[0] == 1, "the CPU backend takes one vector at a time"
            dd = self.be.fromCoeffs(idx, [int(x) for x in cf[0]])
            dd.batch = 1
        return (dd, cf) if coeffs else dd

    def embed(self, coeffs):
        return self.slots(coeffs)

    def decode(self, acc, factor_inv):
        P = self.P
        return self.slots([[int(x) % P * factor_inv % P for x in self.be.toPoly(acc)]])

    def norm(self, coeffs):
        return np.array([self.be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])


class Setup:
    """a context, the oracle backend, keys (1D and Frobenius matrices) and an EncryptedArray -- helib_amd.bgv_gr's, or
    bgv_gf's with gf=True (r = 1) -- over TableEncoder.  circ lists the mulAddCirculant calls (d, nout)."""

    def __init__(self, m, p, r, bits=300, seed=3, gf=False, circulant=True):
        from oracle import oracle as O
        from oracle.backend import OracleBackend, OracleOps, OPoly
        from helib_amd import bgv_gf, bgv_gr, ctxt as hc, keys as hk
        self.m, self.p, self.r, self.P = m, p, r, p ** r
        cc = self.cc = hc.ChainContext(m, p, r, bits=bits, c=2)
        o = self.o = O.Ctx(m)
        for q in cc.primes:
            o.add_prime(q)
        circ = self.circ = []

        class Ops(OracleOps):
            pass

        def mulAddCirculant(self_, out0, out1, consts, in0, in1):
            d, nout = len(consts), len(out0)
            circ.append((d, nout))
            idx = in0[0].idx
            for part in list(in0) + (list(in1) if in1 is not None else []) + list(out0) + (list(out1) if out1 is not None else []):
                assert isinstance(part, OPoly) and part.idx == idx
            ids = [id(x) for x in list(out0) + (list(out1) if out1 is not None else [])]
            assert len(set(ids)) == len(ids) and not set(ids) & {id(x) for x in list(in0) + list(consts)}
            qs = [o.primes[i] for i in idx]
            crow = [np.stack([c.rows[c.idx.index(i)] for i in idx]) for c in consts]
            for outs, ins in ((out0, in0), (out1, in1)):
                if outs is None:
                    continue
                got = IR.circulant(crow, [x.rows for x in ins], qs, nout)
                for dst, rows in zip(outs, got):
                    dst.rows = np.array(rows, dtype=np.uint64)
        if circulant:
            Ops.mulAddCirculant = mulAddCirculant

        class Backend(OracleBackend):
            def fromCoeffsBatch(self, idx, polys):
                assert len(polys) == 1
                d = self.fromCoeffs(idx, polys[0])
                d.batch = 1
                return d
        be = self.be = Backend(o, cc)
        be.ops = Ops(o)
        self.enc = TableEncoder(m, p, r, be)
        self.ref = IR.tables(m, p, r)
        self.sk = hk.SecKey(cc, be, seed=seed)
        self.sk.GenSecKey()
        self.ea = (bgv_gf if gf else bgv_gr).EncryptedArray(cc, None, encoder=self.enc)
        self.sk.zMStar = self.ea.zMStar
        hk.add1DMatrices(self.sk)
        hk.addFrbMatrices(self.sk)

    def slots(self, seed, B=1):
        return np.random.default_rng(seed).integers(0, self.P, size=(B, self.ea.size(), self.ea.getDegree()))


def state(ct):
    return ({h: part.rows.copy() for h, part in ct.parts.items()}, {h: list(part.idx) for h, part in ct.parts.items()},
            ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag)


def same(a, b):
    assert a[1:] == b[1:], (a[1:], b[1:])
    assert a[0].keys() == b[0].keys() and all(np.array_equal(a[0][h], b[0][h]) for h in a[0])
