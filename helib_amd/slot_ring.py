"""The ring of a slot, R = Z_P[X] / G with P = p^r and G the (Hensel-lifted) first factor of Phi_m mod p, d = deg G =
ord_m(p): the plain-side arithmetic of helib_amd.bgv_gf (r = 1, R = GF(p^d)) and helib_amd.bgv_gr (any r, R a Galois
ring), and the linear maps on such slots that helib_amd.bgv_gf_matmul, bgv_gr_matmul, intraslot and evalmap put in front
of their own checks.  Everything reads the array it is given -- ea.P (the modulus of the slot words), ea.p (the prime),
ea.G, ea.getDegree() -- and never asks which class it is; at r = 1 "unit" and "non-zero" coincide and sigma: X -> X^p is
alpha -> alpha^p.  The device has had one body for both rings all along (helib_amd/csrc/bgv_gf.h, bgv_gf_linalg.h); this is
its counterpart on the host.

  _matmod / _invmod   a @ b mod P; the inverse mod P by Gauss-Jordan with unit pivots (None when singular mod p)
  SlotEncoder         slot vectors [B, nslots, d] <-> polynomials on the device over a capi.BgvGf table
  SlotRing            the mixin of both EncryptedArray classes: the check of G, getG / getDegree, _slots, the tail of
                      decrypt_batch, frobeniusAutomorph, and the plain-side truths _mul / mulPlain / _frobenius /
                      frobeniusPlain
  _tables(ea)         frob (the powers of sigma), K (the inverse Moore matrix) and the flat d^2 x d^2 table, built once
                      per array
  buildLinPolyCoeffs / evalLinPoly / applyLinPolyLL / applyLinPoly1 / applyLinPolyMany
                      linearized polynomials (src/EncryptedArray.cpp:740-879): a Z_P-linear map of a slot is
                      alpha -> sum_k C[k] sigma^k(alpha)
  slotAutomorph / frobEach          the plaintext automorphism X -> X^k: a permutation of the slots and a power of
                      sigma in every slot
  mulPlain / hostConstant           the plain-side truth of MatMul1D / BlockMatMul1D, and one constant of an exec

Nothing here imports the modules it serves, or oracle/."""
import numpy as np

from . import bgv, capi, linalg
from .ckks import LogicError


# ---- arithmetic modulo P ----
def _matmod(a, b, P):
    """a @ b mod P, through Python integers when the sums could leave int64"""
    a, b = np.asarray(a, dtype=np.int64) % P, np.asarray(b, dtype=np.int64) % P
    if P * P * max(1, a.shape[-1]) < 2 ** 63:
        return a @ b % P
    return np.array((a.astype(object) @ b.astype(object)) % P, dtype=np.int64)


def _invmod(a, p, P):
    """the inverse of a square matrix modulo P = p^r by Gauss-Jordan on Python integers, every pivot a unit (non-zero
    mod p: one exists in each column exactly when the matrix is invertible mod p); None when it is singular mod p"""
    n = a.shape[0]
    w = np.concatenate([np.asarray(a).astype(object) % P, np.eye(n, dtype=object)], axis=1)
    for c in range(n):
        piv = next((r for r in range(c, n) if int(w[r, c]) % p), None)
        if piv is None:
            return None
        if piv != c:
            w[[c, piv]] = w[[piv, c]]
        w[c] = w[c] * pow(int(w[c, c]), -1, P) % P
        for r in range(n):
            if r != c and w[r, c]:
                w[r] = (w[r] - w[r, c] * w[c]) % P
    return np.array(w[:, n:], dtype=np.int64)


# ---- the encoder ----
class SlotEncoder:
    """slot vectors in R <-> polynomials on the device (hx_bgv_gf_* over table, a capi.BgvGf): CrtEncoder's members, and
    G (d + 1 integers in [0, P))"""

    def __init__(self, hxctx, table):
        self.g = hxctx
        self.table = table
        self.G = list(table.G)

    def dims(self):
        """(gens, signed ords) of the hypercube of Z_m^* / <p>"""
        return self.table.gens, self.table.ords

    def encode(self, v, mul, idx, coeffs=False):
        return capi.bgvGfEncode(self.table, v, idx, mul, coeffs=coeffs)

    def split(self, poly):
        return capi.splitBatch(poly)

    def embed(self, coeffs):
        return capi.bgvGfEmbed(self.table, coeffs)

    def decode(self, acc, factor_inv):
        return capi.bgvGfDecode(self.table, acc, factor_inv)

    def norm(self, coeffs):
        """embeddingLargestCoeff of every zzX [B, phi(m)]"""
        return capi.embeddingLargestCoeff(self.g, np.asarray(coeffs, dtype=np.float64))


# ---- the array ----
class SlotRing:
    """What an EncryptedArray with slots in R has beyond its integer-slot base class.  The subclass sets self.P, self.p,
    self.enc and self.zMStar (its base class's constructor does), then calls _initRing(G)."""

    # the refusal of a G of degree d other than the encoder's; the subclass says what its G is
    _otherG = "EncryptedArray: another G needs a root of G in R (the reference's FindRoots branch of mapToSlots), which is not built"

    def _initRing(self, G):
        P, d = self.P, self.zMStar.ordP
        self.G = [int(x) % P for x in self.enc.G]
        if len(self.G) != d + 1 or self.G[d] != 1:
            raise LogicError("EncryptedArray: the encoder's G is not monic of degree d = %d" % d)
        if G is not None:
            g = [int(x) % P for x in G]
            while g and g[-1] == 0:
                g.pop()
            if len(g) - 1 < d:
                raise LogicError("EncryptedArray: deg G = %d < d = %d is not built (only G = F_0, of degree d)" % (len(g) - 1, d))
            if g != self.G:
                raise LogicError(self._otherG)
        self._G = np.array(self.G[:d], dtype=np.int64)
        self._frob = None

    def getG(self):
        return list(self.G)

    def getDegree(self):
        return self.zMStar.ordP

    def _slots(self, v):
        """-> int64 [B, nslots, d].  One axis: one vector of constants; two: [B, <= nslots] constants; three:
        [B, <= nslots, <= d]; what is missing is zero."""
        a = np.asarray(v)
        if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
            a = np.array([int(x) % self.P for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
        a = a.astype(np.int64)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim == 2:
            a = a[:, :, None]
        n, d = self.size(), self.getDegree()
        if a.ndim != 3 or a.shape[1] > n or a.shape[2] > d:
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "more values than slots, or more coefficients than d")
        out = np.zeros((a.shape[0], n, d), dtype=np.int64)
        out[:, :a.shape[1], :a.shape[2]] = a
        return out

    def decrypt_batch(self, ct, sk):
        """SecKey::Decrypt + decode for every element of a batched Ctxt -> int64 [B, nslots, d] in [0, p^k), p^k the
        ciphertext's space (k <= r)"""
        out = super().decrypt_batch(ct, sk)
        return out if out.ndim == 3 else self._slots(out)

    def frobeniusAutomorph(self, ct, j):
        """EncryptedArray::frobeniusAutomorph: every slot alpha -> sigma^j(alpha) = alpha(X^(p^j)) mod G (alpha^(p^j) at
        r = 1), by Ctxt::frobeniusAutomorph (X -> X^(p^j) maps Phi_m's lifted factor F_i to itself, so it acts slot by
        slot, and the slot maps are ring maps); j counts mod d"""
        ct.frobeniusAutomorph(j % self.getDegree())
        return ct

    # ---- the plain side ----
    def _mul(self, a, b):
        """the product in R along the last axis of two arrays [..., d] with entries in [0, P)"""
        P, d = self.P, self.getDegree()
        w = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1] + (2 * d - 1,), dtype=np.int64)
        for l in range(d):                                  # every product is below P^2 < 2^62 and reduced at once
            w[..., l:l + d] = (w[..., l:l + d] + a[..., l:l + 1] * b % P) % P
        for k in range(2 * d - 2, d - 1, -1):               # X^k = -X^(k - d) (G - X^d)
            w[..., k - d:k] = (w[..., k - d:k] - w[..., k:k + 1] * self._G % P) % P
        return np.ascontiguousarray(w[..., :d])

    def mulPlain(self, a, b):
        """the slot-wise product in R -> int64 [B, nslots, d]"""
        return self._mul(self._slots(a) % self.P, self._slots(b) % self.P)

    def _frobenius(self):
        """row l = X^(l p) mod G: sigma(alpha) = sum_l alpha_l X^(l p), sigma fixing the coefficients.  (At r > 1 sigma is
        not alpha -> alpha^p: that map is not additive modulo p^2.)"""
        if self._frob is None:
            P, p, d = self.P, self.p, self.getDegree()
            one, x = np.zeros((1, 1, d), dtype=np.int64), np.zeros((1, 1, d), dtype=np.int64)
            one[0, 0, 0] = 1
            if d == 1:
                x[0, 0, 0] = -self.G[0] % P                 # X mod the linear G
            else:
                x[0, 0, 1] = 1
            xp, e = one, p                                  # X^p by square and multiply
            while e:
                if e & 1:
                    xp = self._mul(xp, x)
                x = self._mul(x, x)
                e >>= 1
            rows, cur = [], one
            for _ in range(d):
                rows.append(cur[0, 0])
                cur = self._mul(cur, xp)
            self._frob = np.stack(rows)
        return self._frob

    def frobeniusPlain(self, a, j):
        """every slot alpha -> sigma^j(alpha) = alpha(X^(p^j)) mod G -> int64 [B, nslots, d]"""
        a, P, d = self._slots(a) % self.P, self.P, self.getDegree()
        F = self._frobenius()
        for _ in range(j % d):
            nxt = np.zeros_like(a)
            for l in range(d):
                nxt = (nxt + a[:, :, l:l + 1] * F[l] % P) % P
            a = nxt
        return a


# ---- linearized polynomials ----
class _Tables:
    """frob[e][l] = sigma^e(X^l); M[i][j] = sigma^i(X^j) = frob[i][j] (buildLinPolyMatrix, a Moore matrix); K = M^-1 over
    the ring, K[j][k] = sigma^k(beta_j) with beta the dual basis of the powers of X under the trace Tr = sum_e sigma^e
    ((K M)[j][j'] = sum_k sigma^k(beta_j X^j') = Tr(beta_j X^j')); beta = the inverse of the Gram matrix Tr(X^(i + j))
    over Z_P, which is invertible because it is invertible mod p"""

    def __init__(self, ea):
        p, P, d = ea.p, ea.P, ea.getDegree()
        S = ea._frobenius()
        self.frob = np.zeros((d, d, d), dtype=np.int64)
        self.frob[0] = np.eye(d, dtype=np.int64)
        for e in range(1, d):
            self.frob[e] = _matmod(self.frob[e - 1], S, P)
        tr = self.frob[:, :, 0].sum(axis=0) % P                     # Tr(X^l) = sum_e [X^0] sigma^e(X^l), l < d
        x = np.zeros(d, dtype=np.int64)
        x[0] = 1
        step = np.zeros(d, dtype=np.int64)
        if d > 1:
            step[1] = 1
        pw = []
        for _ in range(2 * d - 1):                                  # X^s mod G, s <= 2 d - 2
            pw.append(x)
            x = ea._mul(x, step) if d > 1 else x
        trs = _matmod(np.stack(pw), tr[:, None], P)[:, 0]
        gram = np.array([[trs[i + j] for j in range(d)] for i in range(d)], dtype=np.int64)
        beta = _invmod(gram, p, P)
        if beta is None:
            raise LogicError("internal: the Gram matrix of traces is singular mod p")
        self.K = np.stack([np.stack([_matmod(beta[j][None, :], self.frob[k], P)[0] for k in range(d)]) for j in range(d)])
        self.ea, self._T = ea, None

    def flat(self):
        """T[(j, b)][(k, c)] = [X^c](X^b K[j][k] mod G), [d^2, d^2]: C = E T is buildLinPolyCoeffs as the device forms it"""
        if self._T is None:
            d = self.K.shape[0]
            eye = np.eye(d, dtype=np.int64)
            T = np.stack([self.ea._mul(eye[:, None, :], self.K[j][None, :, :]) for j in range(d)])      # [j, b, k, c]
            self._T = np.ascontiguousarray(T.reshape(d * d, d * d))
        return self._T


def _tables(ea):
    t = ea.__dict__.get("_linpoly")
    if t is None:
        t = ea.__dict__["_linpoly"] = _Tables(ea)
    return t


def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs: L [..., d, d], row j the coefficients of the image of X^j -> C
    [..., d, d], row k the coefficients of C[k] = sum_j L[j] K[j][k]; the Z_P-linear map is alpha -> sum_k C[k]
    sigma^k(alpha)"""
    P, d = ea.P, ea.getDegree()
    L = np.asarray(L, dtype=np.int64) % P
    if L.ndim < 2 or L.shape[-2:] != (d, d):
        raise LogicError("buildLinPolyCoeffs takes [..., d, d] with d = %d" % d)
    K = _tables(ea).K
    Lf = L.reshape(-1, d, d)
    C = np.zeros_like(Lf)
    for k in range(d):
        C[:, k, :] = ea._mul(Lf, K[None, :, k, :]).sum(axis=1) % P
    return C.reshape(L.shape)


def linPolyFlat(ea, E):
    """buildLinPolyCoeffs through the flat table: what the device computes"""
    d = ea.getDegree()
    E = np.asarray(E, dtype=np.int64) % ea.P
    return _matmod(E.reshape(-1, d * d), _tables(ea).flat(), ea.P).reshape(E.shape)


def evalLinPoly(ea, C, a):
    """sum_k C[k] sigma^k(alpha) slot by slot: C [d, d] (one map) or [nslots, d, d], a slots -> [B, nslots, d]"""
    P, d = ea.P, ea.getDegree()
    a = ea._slots(a) % P
    C = np.asarray(C, dtype=np.int64) % P
    C = np.broadcast_to(C, (ea.size(), d, d)) if C.ndim == 2 else C
    out = np.zeros_like(a)
    for k in range(d):
        out = (out + ea._mul(ea.frobeniusPlain(a, k), C[None, :, k, :])) % P
    return out


def applyLinPolyLL(ct, encodedC):
    """applyLinPolyLL (src/EncryptedArray.cpp:855-870): encodedC[j] is an EncodedPtxt (EncryptedArray.encodePtxt) holding
    C[j] of every slot's map, or (DoubleCRT, size); the Frobenius keys come from keys.addFrbMatrices"""
    def times(c, k):
        if isinstance(k, bgv.EncodedPtxt):
            k.ea.multByConstant(c, k)
        else:
            c.multByConstant(*k)
    linalg._cleanUp(ct)
    tmp = ct.clone()
    times(ct, encodedC[0])
    for j in range(1, len(encodedC)):
        tmp1 = tmp.clone()
        tmp1.frobeniusAutomorph(j)
        times(tmp1, encodedC[j])
        ct += tmp1
    return ct


def applyLinPoly1(ea, ct, C):
    """the same map in every slot (:802-821): C [d, d] from buildLinPolyCoeffs"""
    d = ea.getDegree()
    C = np.asarray(C, dtype=np.int64)
    if C.shape != (d, d):
        raise LogicError("ea's degree does not match the size of C")
    return applyLinPolyLL(ct, [ea.encodePtxt(np.broadcast_to(C[j], (1, ea.size(), d))) for j in range(d)])


def applyLinPolyMany(ea, ct, Cvec):
    """another map in every slot (:826-850): Cvec [nslots, d, d], row i from buildLinPolyCoeffs for slot i"""
    d = ea.getDegree()
    Cvec = np.asarray(Cvec, dtype=np.int64)
    if Cvec.shape != (ea.size(), d, d):
        raise LogicError("Number of slots does not match size of Cvec, or an entry's size is unequal to the degree of ea")
    return applyLinPolyLL(ct, [ea.encodePtxt(Cvec[None, :, j, :]) for j in range(d)])


# ---- plaintext automorphisms ----
def slotAutomorph(ea, k):
    """X -> X^k on the slots -> (perm, frob): the new slot j is sigma^frob[j] of the old slot perm[j].  Slot j reads the
    plaintext at zeta^(1 / t_j) (zeta = X mod G, t_j = reps()[j]); after the automorphism that is its value at
    zeta^(k / t_j) = zeta^(p^e / t_i) for the slot i whose coset holds t_j / k, with t_i k = t_j p^e (mod m), and H(y^(p^e))
    = sigma^e(H(y)) over Z_P because sigma fixes the lifted F_0 (H(y)^(p^e) at r = 1)."""
    m = ea.m
    k %= m
    cache = ea.__dict__.setdefault("_slotAut", {})
    if k not in cache:
        kinv, p, d = pow(k, -1, m), ea.p % m, ea.getDegree()
        log = {pow(p, e, m): e for e in range(d)}
        cos, reps = ea._cosets(), ea.zMStar.reps()
        perm = np.array([cos[t * kinv % m] for t in reps], dtype=np.int64)
        frob = np.array([log[reps[i] * k % m * pow(t, -1, m) % m] for i, t in zip(perm, reps)], dtype=np.int64)
        cache[k] = (perm, frob)
    return cache[k]


def frobEach(ea, a, e):
    """slot s of a [B, n, d] -> its sigma^e[s]"""
    fr, out = _tables(ea).frob, a.copy()
    for x in np.unique(e):
        if x:
            w = e == x
            out[:, w] = _matmod(a[:, w], fr[x], ea.P)
    return out


def automorphPlain(ea, a, k):
    """the slots of the plaintext with X -> X^k applied -> int64 [B, nslots, d]"""
    perm, frob = slotAutomorph(ea, k)
    return frobEach(ea, (ea._slots(a) % ea.P)[:, perm], frob)


# ---- the plain side of the matrices ----
def mulPlain(ea, v, mat):
    """mul(PlaintextArray, MatMul1D / BlockMatMul1D) on slots v -> int64 [B, nslots, d]: along mat's dimension and for
    every transform k, w[k][j] = sum_i v[k][i] * A_k[i][j] -- the product in R for a ring entry, the coefficient row
    vector times the d x d block for a block entry"""
    P = ea.P
    v, d, D = ea._slots(v) % P, ea.getDegree(), mat.D
    B, n = v.shape[0], ea.size()
    order = np.argsort(mat.blk * D + mat.col, kind="stable")           # slot of (transform, coordinate)
    x = v[:, order].reshape(B, n // D, D, d)
    A = mat.dense if mat.multiple else np.broadcast_to(mat.dense, (n // D,) + mat.dense.shape[1:])
    w = np.zeros_like(x)
    if mat.block:
        xo, Ao = (x.astype(object), A.astype(object)) if P * P * d >= 2 ** 63 else (x, A)
        terms = (xo[:, :, :, None, None, :] @ Ao[None])[..., 0, :] % P                     # [B, k, i, j, c]
        w = np.array(terms.sum(axis=2) % P, dtype=np.int64)
    else:
        for j in range(D):
            w[:, :, j] = ea._mul(x.reshape(B, -1, d), A[:, :, j].reshape(1, -1, d)).reshape(B, n // D, D, d).sum(axis=2) % P
    out = np.zeros_like(v)
    out[:, order] = w.reshape(B, n, d)
    return out


def hostConstant(ea, mat, i, k, row):
    """one constant on the host: slot s = sigma^e(coefficient k of the entry the slot src[s] reads on diagonal i), row
    [n, 2] the (src, e) of every slot, src < 0 for a zero"""
    src, e = row[:, 0].astype(np.int64), row[:, 1].astype(np.int64)
    val = mat.slotValues(i, k)
    out = np.where((src >= 0)[:, None], val[np.maximum(src, 0)], 0)
    return frobEach(ea, out[None], e)[0]
