"""MatMul1D_CKKS / MatMul1DExec (src/matmul.cpp:695-884 construction; :973-1110, :1220-1322 mul) for CKKS, whose one
dimension is native: a plaintext matrix times the slot vector of a (batched) ciphertext,
w[j] = sum_r get(r, j) * v[r]  (mul(PlaintextArray, MatMul1D), src/matmul.cpp:2673-2696).

The inner loop  acc += diag_i * rot^j(ct)  (MulAdd, src/matmul.cpp:391-408) runs as ONE device call per accumulator
(capi.mulAddMany: hx_mul_add_many) when the bookkeeping allows it; the bookkeeping itself -- lnNoise, ptxtMag,
lnRatFactor, prime sets -- is the reference's, term by term, run by the real Ctxt methods on data-less stand-ins
of the operands first.  The fused call is taken when that run never had to touch data other than by `*=
constant` and `+=` (no equalizeRationalFactors multiplier other than 1, no mod-switch) and the backend offers it;
otherwise the run goes term by term.  The class counter MatMul1DExec.fallbacks, and the timing statistic of the same
name while timing.fhe_stats is set, count the runs that did not fuse.  HX_MATMUL_TERMWISE=1 (or fused=False) forces
term by term.
The BGV classes (helib_amd.bgv_matmul) run the same mul with multByConstant as the multiply and their own dimension.
Out of scope: BlockMatMul1D, MatMulFull for CKKS, non-native dimensions.  Nothing here imports oracle/."""
import os
import time

import numpy as np

from . import ctxt as hc
from . import keys as hk
from . import timing


class MatMul1D_CKKS:
    """get(i, j) -> complex, or a dense [D, D] array A with get(i, j) = A[i, j]"""

    def __init__(self, ea, mat):
        self.ea = ea
        self.dense = None if callable(mat) else np.asarray(mat, dtype=np.complex128)
        self.get = mat if callable(mat) else (lambda i, j: self.dense[i, j])

    def processDiagonal(self, i):
        """MatMul1D_CKKS::processDiagonal (src/matmul.cpp:695-708): diag[j] = get((j - i) mod D, j)"""
        D = self.ea.size()
        j = np.arange(D)
        if self.dense is not None:
            return self.dense[(j - i) % D, j]
        return np.array([self.get(int((jj - i) % D), int(jj)) for jj in j], dtype=np.complex128)


class _NeedsData(Exception):
    pass


class _NoData:
    """a part without rows: `*= constant`, `+=` and copies are bookkeeping-neutral, anything else needs the data"""

    def copy(self):
        return self

    def __imul__(self, o):
        if isinstance(o, (int, float, complex)):      # a number changes the words: that needs the data
            raise _NeedsData("*= number")
        return self

    def __iadd__(self, o):
        if isinstance(o, (int, float, complex)):
            raise _NeedsData("+= number")
        return self

    def __getattr__(self, name):
        raise _NeedsData(name)


def _like(ct, parts):
    c = hc.Ctxt(ct.context, ct.ops, ct.ksw, ct.ksw_ptxtSpace, ct.ksw_lnNoise)
    c.ksw_auto, c.ksw_pow, c.ksw_map = ct.ksw_auto, ct.ksw_pow, ct.ksw_map
    c.primeSet, c.ptxtSpace, c.intFactor = ct.primeSet, ct.ptxtSpace, ct.intFactor
    c.lnNoise, c.ptxtMag, c.lnRatFactor = ct.lnNoise, ct.ptxtMag, ct.lnRatFactor
    c.parts = parts
    return c


def _shadow(ct):
    return _like(ct, {h: _NoData() for h in ct.parts})


def _empty(ct):
    """Ctxt(ZeroCtxtLike, ct)"""
    c = _like(ct, {})
    c.lnNoise, c.ptxtMag, c.lnRatFactor, c.intFactor = -float("inf"), 1.0, 0.0, 1
    return c


def _cleanUp(ct):
    if ct.parts:
        ct.cleanUp()
    return ct


class MatMul1DExec:
    fallbacks = 0      # groups that ran term by term although fusing was asked for (all instances)
    dim = 0            # the dimension the rotations run along: CKKS has one; helib_amd.bgv_matmul sets it

    def __init__(self, ea, mat, minimal=False):
        mat = mat if isinstance(mat, MatMul1D_CKKS) else MatMul1D_CKKS(ea, mat)
        self.ea, self.minimal = ea, minimal
        self.D = D = ea.size()
        bsgs = D > hk.HELIB_KEYSWITCH_THRESH or (minimal and D > hk.HELIB_KEYSWITCH_MIN_THRESH)
        self.g = g = hk.KSGiantStepSize(D) if bsgs else 0
        self.times = {"construct": 0.0, "baby": 0.0, "muladd": 0.0, "giant": 0.0}
        self.sync = None       # a callable that waits for the device: the phases of `times` are then device time
        self.fused = os.environ.get("HX_MATMUL_TERMWISE", "0") in ("", "0")
        t0 = time.perf_counter()
        # MatMul1DExec_construct_CKKS (src/matmul.cpp:792-822): diagonal i, rotated by -g * floor(i / g)
        # (build_ConstMultiplier_CKKS, :770-789: diag1[(j + amt) mod D] = diag[j]); a zero diagonal is no multiplier
        self.rotation = [(-g * (i // g)) if g else 0 for i in range(D)]
        vecs, where = [], []
        for i in range(D):
            diag = mat.processDiagonal(i)
            if not np.any(diag):
                continue
            d1 = np.empty(D, dtype=np.complex128)
            d1[(np.arange(D) + self.rotation[i]) % D] = diag
            vecs.append(d1)
            where.append(i)
        self.multiplier = [None] * D
        # hoisted rotations (the g = 0 form) stay on the ctxt and special primes: their constants must too
        cc = ea.cc
        idx = list(cc.ctxtPrimes) + (list(cc.specialPrimes) if g == 0 else [])
        err = ea.defaultErr()
        scale = ea.defaultScale(err)
        step = max(1, int(getattr(ea.enc, "max_batch", 1)))
        for lo in range(0, len(vecs), step):
            chunk = np.stack(vecs[lo:lo + step])
            polys = ea.enc.split(ea.enc.encode(chunk, scale, idx))     # one device encode per chunk
            for v, i, d in zip(chunk, where[lo:lo + step], polys):
                self.multiplier[i] = (d, float(np.max(np.abs(v))), scale, err)
        self._tick("construct", t0)

    def _tick(self, name, t0):
        if self.sync is not None:
            self.sync()
        self.times[name] += time.perf_counter() - t0

    # ---- x += sum a_i * b_i ----
    @staticmethod
    def _mulAdd(x, a, b):
        """MulAdd (src/matmul.cpp:391-399)"""
        tmp = b.clone()
        tmp.multByConstantCKKS(*a)
        x += tmp

    def _group(self, x, terms, fused):
        """x += sum_t a_t * b_t over terms [(multiplier, Ctxt)], in order.  Consecutive terms on one prime set are
        one fused call each (the g = 0 hoisted form mixes the unrotated term, on the ctxt primes, with hoisted ones
        on ctxt + special primes)."""
        terms = [(a, b) for a, b in terms if a is not None and b.parts]
        if not terms:
            return
        t0 = time.perf_counter()
        runs = []
        for a, b in terms:
            if runs and runs[-1][0][1].primeSet == b.primeSet:
                runs[-1].append((a, b))
            else:
                runs.append([(a, b)])
        for run in runs:
            if not (fused and hasattr(run[0][1].ops, "mulAddMany") and self._fusedRun(x, run)):
                if fused and hasattr(run[0][1].ops, "mulAddMany"):
                    MatMul1DExec.fallbacks += 1
                    timing.STATS_UPDATE("MatMul1DExec.fallbacks", 1)
                for a, b in run:
                    self._mulAdd(x, a, b)
        self._tick("muladd", t0)

    def _fusedRun(self, x, run):
        """one hx_mul_add_many for the run if its bookkeeping needs no data; False (x untouched) otherwise"""
        ops = run[0][1].ops
        handles = set(run[0][1].parts)
        if handles not in ({"1"}, {"1", "s"}) or any(set(b.parts) != handles for _, b in run) \
                or (x.parts and set(x.parts) != handles):
            return False
        sx = _shadow(x)
        grow = frozenset(run[0][1].primeSet) - sx.primeSet if sx.parts else frozenset()
        if grow:
            # addCtxt's first step (src/Ctxt.cpp:1470-1478): x goes up to the union of the prime sets.  It does not
            # depend on the term, so it is done on x itself, once, where term by term would do it at the first term
            sx.primeSet = sx.primeSet | grow
            sx.lnNoise = sx.lnNoise + x.context.logOfProduct(sorted(grow))
            sx.lnRatFactor += x.context.logOfProduct(sorted(grow))
        try:
            for a, b in run:
                self._mulAdd(sx, a, _shadow(b))
        except _NeedsData:
            return False
        if grow:
            x.modUpToSet(x.primeSet | grow)
        accumulate = bool(x.parts)
        if not accumulate:
            x.parts = {h: ops.zerosLike(run[0][1].parts[h]) for h in sorted(handles)}
        two = "s" in handles
        ops.mulAddMany(x.parts["1"], x.parts["s"] if two else None, [a[0] for a, _ in run],
                       [b.parts["1"] for _, b in run], [b.parts["s"] for _, b in run] if two else None,
                       accumulate=accumulate)
        x.primeSet, x.ptxtSpace, x.intFactor = sx.primeSet, sx.ptxtSpace, sx.intFactor
        x.lnNoise, x.ptxtMag, x.lnRatFactor = sx.lnNoise, sx.ptxtMag, sx.lnRatFactor
        return True

    def _babySteps(self, ct, need, strategy):
        """GenBabySteps(v, ctxt, dim, clean = true) (src/matmul.cpp:926-969) for the j in `need`"""
        z = self.ea.zMStar
        out = {}
        if self.g == 1 or strategy == hk.HELIB_KSS_UNKNOWN:
            ct0 = _cleanUp(ct.clone())
            for j in need:
                out[j] = ct0.clone()
                if j:
                    out[j].smartAutomorph(z.genToPow(self.dim, j))
                _cleanUp(out[j])
            return out
        precon = hc.BasicAutomorphPrecon(ct)
        for j in need:
            out[j] = _cleanUp(precon.automorph(z.genToPow(self.dim, j)))
        return out

    def mul(self, ct, pk=None, strategy=None, fused=None):
        """MatMul1DExec::mul, native dimension.  The key-switching strategy of the dimension is read from the key
        `pk` (keys.getKSStrategy) unless given."""
        fused = self.fused if fused is None else fused
        if strategy is None:
            strategy = hk.getKSStrategy(pk, self.dim) if pk is not None else hk.HELIB_KSS_UNKNOWN
        z, D, g, M = self.ea.zMStar, self.D, self.g, self.multiplier
        _cleanUp(ct)
        iterative = strategy == hk.HELIB_KSS_MIN
        live = [i for i in range(D) if M[i] is not None]
        if g != 0:
            h = -(-D // g)
            need = sorted({i % g for i in live})
            if iterative:
                t0 = time.perf_counter()
                baby, cur = {}, ct.clone()
                for j in range((need[-1] + 1) if need else 0):
                    if j:
                        cur = cur.clone()
                        cur.smartAutomorph(z.genToPow(self.dim, 1))
                        _cleanUp(cur)
                    baby[j] = cur
                self._tick("baby", t0)
                acc = _empty(ct)
                for k in range(h - 1, -1, -1):
                    if k < h - 1 and acc.parts:
                        t0 = time.perf_counter()
                        acc.smartAutomorph(z.genToPow(self.dim, g))
                        _cleanUp(acc)
                        self._tick("giant", t0)
                    self._group(acc, [(M[i], baby[i % g]) for i in range(g * k, min(g * k + g, D)) if M[i]], fused)
            else:
                t0 = time.perf_counter()
                baby = self._babySteps(ct, need, strategy)
                self._tick("baby", t0)
                acc = _empty(ct)
                for k in range(h):
                    inner = _empty(ct)
                    self._group(inner, [(M[i], baby[i % g]) for i in range(g * k, min(g * k + g, D)) if M[i]], fused)
                    if not inner.parts:
                        continue
                    t0 = time.perf_counter()
                    if k > 0:
                        inner.smartAutomorph(z.genToPow(self.dim, g * k))
                    acc += inner
                    self._tick("giant", t0)
        elif not iterative:
            # buildGeneralAutomorphPrecon (src/matmul.cpp:186-300)
            t0 = time.perf_counter()
            terms = []
            if strategy == hk.HELIB_KSS_FULL:
                precon = hc.BasicAutomorphPrecon(ct)
                terms = [(M[i], precon.automorph(z.genToPow(self.dim, i))) for i in live]
            elif strategy == hk.HELIB_KSS_BSGS:
                gg = hk.KSGiantStepSize(D)
                p0, pre = hc.BasicAutomorphPrecon(ct), {}
                for i in live:
                    k = i // gg
                    if k not in pre:
                        pre[k] = hc.BasicAutomorphPrecon(p0.automorph(z.genToPow(self.dim, gg * k)))
                    terms.append((M[i], pre[k].automorph(z.genToPow(self.dim, i % gg))))
            else:
                ct0 = _cleanUp(ct.clone())
                for i in live:
                    r = ct0.clone()
                    if i:
                        r.smartAutomorph(z.genToPow(self.dim, i))
                    terms.append((M[i], r))
            self._tick("baby", t0)
            acc = _empty(ct)
            self._group(acc, terms, fused)
        else:
            t0 = time.perf_counter()
            sh, terms = ct.clone(), []
            for i in range((live[-1] + 1) if live else 0):
                if i > 0:
                    sh = sh.clone()
                    sh.smartAutomorph(z.genToPow(self.dim, 1))
                    _cleanUp(sh)
                if M[i]:
                    terms.append((M[i], sh))
            self._tick("baby", t0)
            acc = _empty(ct)
            self._group(acc, terms, fused)
        ct.__dict__.update(acc.__dict__)
        return ct
