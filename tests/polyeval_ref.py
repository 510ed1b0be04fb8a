"""Plain-integer references for helib_amd.polyeval and hx_lin_comb, shared by the host and the device tests:

  lin_comb   hx_lin_comb in python integers, word by word; lin_comb_packed: the same sums a row at a time
  replay     the recursion of src/polyEval.cpp:129-389 on integers modulo p^r (the reference's own `#if 0` debugging
             copy, :415-863, does the same): the value per slot, the set of powers formed and the number of products
  digits     the balanced (p odd) or [0, 1] (p = 2) digits of an integer
"""
import math

import numpy as np


def lin_comb(ins, term_idx, out_idx, w, addend, primes):
    """ins[t]: uint64 [rows(t), B, N], the rows of term t on the prime indices term_idx[t] (any order); -> uint64
    [len(out_idx), B, N]: row r is (sum over the terms holding prime out_idx[r] of w[t][r] * their row + addend[r])
    modulo primes[out_idx[r]], or the addend alone where no term holds it"""
    B, N = ins[0].shape[1:]
    out = np.zeros((len(out_idx), B, N), dtype=np.uint64)
    for r, i in enumerate(out_idx):
        q = primes[i]
        acc = np.full((B, N), int(addend[r]) if addend is not None else 0, dtype=object)
        for t, rows in enumerate(ins):
            if i in term_idx[t]:
                acc = acc + rows[term_idx[t].index(i)].astype(object) * int(w[t][r])
        out[r] = (acc % q).astype(np.uint64)
    return out


def lin_comb_packed(ins, term_idx, out_idx, w, addend, primes):
    """lin_comb for the shapes of the device tests: a row of words becomes one python integer with a 192-bit field per
    word, so a term's row enters the sum by one multiplication of that integer by its weight (256 products below 2^120
    and an addend stay inside a field); the fields are reduced modulo the row's prime at the end"""
    B, N = ins[0].shape[1:]
    L = B * N
    out = np.zeros((len(out_idx), B, N), dtype=np.uint64)
    assert len(ins) <= 256

    def pack(row):
        a = np.zeros((L, 3), dtype="<u8")
        a[:, 0] = row.reshape(-1)
        return int.from_bytes(a.tobytes(), "little")
    ones = pack(np.ones((B, N), dtype=np.uint64))
    for r, i in enumerate(out_idx):
        q = primes[i]
        acc = ones * (int(addend[r]) if addend is not None else 0)
        for t, rows in enumerate(ins):
            if i in term_idx[t]:
                acc += pack(rows[term_idx[t].index(i)]) * int(w[t][r])
        f = np.frombuffer(acc.to_bytes(L * 24, "little"), dtype="<u8").reshape(L, 3).astype(object)
        out[r] = ((f[:, 0] + (f[:, 1] << 64) + (f[:, 2] << 128)) % q).astype(np.uint64).reshape(B, N)
    return out


def _npt(n):
    return max(n - 1, 0).bit_length()


def _divc(a, b):
    return -(-a // b)


def _norm(f):
    f = list(f)
    while f and f[-1] == 0:
        f.pop()
    return f


class _Powers:
    def __init__(self, x, n, P, st, name):
        self.v, self.P, self.st, self.name = [None] * n, P, st, name
        self.v[0] = x

    def size(self):
        return len(self.v)

    def get(self, e):
        if self.v[e - 1] is None:
            k = 1 << (_npt(e) - 1)
            self.v[e - 1] = [a * b % self.P for a, b in zip(self.get(e - k), self.get(k))]
            self.st["mults"] += 1
            self.st["powers"].add((self.name, e))
        return self.v[e - 1]


def replay(xs, poly, P, k=0):
    """-> (values per x, {"mults", "powers", "leaves"}): polyEval's steps on the integers xs modulo P"""
    st = {"mults": 0, "powers": set(), "leaves": 0}
    xs = [int(v) % P for v in xs]
    n_x = len(xs)

    def mul(a, b):
        st["mults"] += 1
        return [u * v % P for u, v in zip(a, b)]

    def add(a, b):
        return [(u + v) % P for u, v in zip(a, b)]

    def simple(f, baby):
        if len(f) - 1 >= 0:
            st["leaves"] += 1
        ret = [(f[0] if f else 0) % P] * n_x
        for i in range(1, len(f)):
            ret = add(ret, [f[i] * v for v in baby.get(i)])
        return ret

    def ps(f, k, t, delta, baby, giant):
        if len(f) - 1 <= baby.size():
            return simple(f, baby)
        r, q = _norm(f[:k * t]), _norm(f[k * t:])
        dq = len(q) - 1
        r = r + [0] * (dq + 1 - len(r))
        r[dq] -= 1
        r = _norm(r)
        c = [0] * max(len(r) - dq, 0)                    # r = c q + s, q monic
        s = list(r)
        for i in range(len(s) - 1, dq - 1, -1):
            c[i - dq] = s[i]
            for j in range(dq + 1):
                s[i - dq + j] -= c[i - dq] * q[j]
        s = s[:dq] + [0] * (dq - len(s[:dq])) + [1]
        c, s = _norm([v % P for v in c]), _norm([v % P for v in s])
        ret = ps(q, k, t // 2, delta, baby, giant)
        ret = mul(ret, add(simple(c, baby), giant.get(t)))
        return add(ret, ps(s, k, t // 2, delta, baby, giant))

    def dp2(f, k, baby, giant):
        if len(f) - 1 <= baby.size():
            return simple(f, baby)
        n = 1 << _npt((len(f) - 1) // k)
        r, q = f[:(n - 1) * k] + [1], list(f[(n - 1) * k:])
        q[0] -= 1
        q = _norm(q)
        ret = ps(r, k, n // 2, 0, baby, giant)
        tmp = simple(q, baby)
        i = 1
        while i < n:
            g = giant.get(i)
            if any(c % P for c in q):                # (an empty ciphertext stays empty)
                tmp = mul(tmp, g)
            i *= 2
        return add(ret, tmp)

    def rec(f, k, baby, giant):
        d = len(f) - 1
        if d <= baby.size():
            return simple(f, baby)
        delta, n = d % k, _divc(d, k)
        t = 1 << _npt(n)
        if n == t:
            return dp2(f, k, baby, giant)
        if n == t - 1 and delta == 0:
            return ps(f, k, t // 2, delta, baby, giant)
        t //= 2
        u = d - k * (t - 1)
        r, q = f[:u] + [1], list(f[u:])
        q[0] -= 1
        ret = ps(_norm(q), k, t // 2, 0, baby, giant)
        tmp = giant.get(u // k)
        if delta:
            tmp = mul(tmp, baby.get(delta))
        ret = mul(ret, tmp)
        return add(ret, rec(r, k, baby, giant))

    f = _norm([int(c) for c in poly])
    d = len(f) - 1
    if d <= 2:
        if d < 1:
            return [(f[0] if f else 0) % P] * n_x, st
        return simple(f, _Powers(xs, d, P, st, "baby")), st
    if k <= 0:
        kk = int(math.sqrt(d / 2.0))
        k = 1 << _npt(kk)
        if (k == 16 and d > 167) or (k > 16 and k > 1.44 * kk):
            k //= 2
    n = _divc(d, k)
    baby = _Powers(xs, k, P, st, "baby")
    x2k = baby.get(k)
    if n == 1 << _npt(n):
        return dp2(f, k, baby, _Powers(x2k, n // 2, P, st, "giant")), st
    top = f[-1]
    inv = math.gcd(top % P, P) == 1
    topInv = pow(top % P, -1, P) if inv else 0
    extra = 0
    if n * k != d or not inv:
        top = topInv = 1
        f = f + [0] * (n * k + 1 - len(f))
        extra = (1 - f[n * k]) % P
        f[n * k] = 1
    giant = _Powers(x2k, _divc(n, 2) if extra == 0 else n, P, st, "giant")
    if top != 1:
        f = _norm([c * topInv % P for c in f])
    ret = rec(f, k, baby, giant)
    if top != 1:
        ret = [v * top % P for v in ret]
    if extra:
        ret = [(v - extra * g) % P for v, g in zip(ret, giant.get(n))]
    return ret, st


def plain(xs, poly, P):
    """sum_i poly[i] x^i modulo P, by Horner"""
    out = []
    for x in xs:
        r = 0
        for c in reversed(list(poly)):
            r = (r * int(x) + int(c)) % P
        out.append(r)
    return out


def digits(v, p, r):
    """the first r digits of v in base p: in [0, 1] for p = 2, balanced in (-p/2, p/2) otherwise"""
    out = []
    for _ in range(r):
        d = v % p
        if p > 2 and d > p // 2:
            d -= p
        out.append(d)
        v = (v - d) // p
    return out
