"""The single-prime mod-switch with S -- and, at N = 2^14, the canonical-embedding norm of delta/qd -- formed in the
prep kernels' own workgroups (helib_amd/csrc/ntt_kernels.hip PrepFuseIO, norm_r16.h "the direct form", engine.hip
scale_down_impl / embed_norms).

Every case runs on two contexts of the same binary: the default one and its twin created under HX_NO_PREP_FUSE=1
(moddown_S_kernel behind the prep kernel, the (x, S) norm by a norm kernel, the radix-16 norm in its paired form).
Output words must be equal word for word, norms must meet the oracle's embedding_largest_coeff within NORM_RTOL on
both, and the in-situ profiler says which kernels ran, so a case that silently took the other route fails."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
NORM_RTOL = 1e-9   # double-precision FFT vs the oracle's long-double evaluation (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401  (before the library touches the device: tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU parity tests run on an MI355X (pytest -m gpu)")
    return capi


class Pair:
    """A device context and an oracle context with the same primes / roots (as tests/test_gpu_parity.py)."""

    def __init__(self, hx, m, primes, oracle=None):
        self.g = hx.Context(m)
        self.o = oracle or O.Ctx(m)
        for n, q in enumerate(primes):
            i = n if oracle else self.o.add_prime(q)
            assert self.g.add_prime(q, self.o.roots[i]) == i
        self.N = self.o.N
        self.primes = list(primes)

    def rand(self, idx, seed, batch):
        out = np.zeros((len(idx), batch, self.N), dtype=np.uint64)
        for r, i in enumerate(idx):
            for b in range(batch):
                out[r, b] = O.fill_uniform(self.N, self.primes[i], seed * 100003 + i * 131 + b)
        return out


def chain(m, L=3, small=1):
    """L 60-bit ctxt primes and `small` 45-bit primes (what a fresh multiply's mod-up adds)."""
    g60, g45 = O.PrimeGen(60, m), O.PrimeGen(45, m)
    return [g60.next() for _ in range(L)] + [g45.next() for _ in range(small)]


def kernels_of(hx, fn):
    hx.profileBegin()
    out = fn()
    return out, {k["kernel"] for k in hx.profileEnd()["kernels"]}


def twins(hx, monkeypatch, m, primes):
    """(default context, HX_NO_PREP_FUSE=1 context) over one oracle; the switch is read when a context is created."""
    monkeypatch.delenv("HX_NO_PREP_FUSE", raising=False)
    Pf = Pair(hx, m, primes)
    monkeypatch.setenv("HX_NO_PREP_FUSE", "1")
    Pc = Pair(hx, m, primes, oracle=Pf.o)
    monkeypatch.delenv("HX_NO_PREP_FUSE", raising=False)
    return Pf, Pc


def has(names, piece):
    return any(piece in k for k in names)


def check_routes(kf, kc, prep, norm_in_prep):
    """prep = "ntt_moddown_prep_kernel<" or "ntt_moddown_prep_tensor_kernel<"; names as rocprofv3 prints them."""
    assert not has(kf, "moddown_S_kernel"), sorted(kf)
    assert has(kc, "moddown_S_kernel"), sorted(kc)
    assert any(prep in k and k.rstrip().endswith(", 0>") for k in kc), sorted(kc)
    if norm_in_prep:
        assert any(prep in k and k.rstrip().endswith(", 2>") for k in kf), sorted(kf)
        assert not has(kf, "embed_norm_r16_kernel<hx::NormSrcXS>"), sorted(kf)
        assert has(kc, "embed_norm_r16_paired_kernel<hx::NormSrcXS>"), sorted(kc)
    else:
        assert any(prep in k and k.rstrip().endswith(", 1>") for k in kf), sorted(kf)


def oracle_bring(P, own, add, drop, ptxt, rows):
    """addPrimesAndScale + scaleDownToSet of one element: (rows on own + add - drop, fdelta)."""
    cur = own + add
    up = np.vstack([P.o.scale_by_primes(own, rows, add)] + [np.zeros((1, P.N), dtype=np.uint64)] * len(add)) if add else rows
    return P.o.scale_down(cur, up, drop, ptxt, want_fdelta=True)


def by_prime(poly, keep):
    """the poly's rows in the order of `keep` (the last row moves into the dropped row's slot)"""
    idx, d = poly.getIndexSet(), poly.download()
    assert sorted(idx) == sorted(keep)
    return np.stack([d[idx.index(i)] for i in keep])


# ---------------------------------------------------------------- 1. hx_bring_to_set_multi_norms, N = 2^14
@pytest.mark.parametrize("ptxt", [65537, 2, 1])
@pytest.mark.parametrize("modup", [True, False])
@pytest.mark.parametrize("nparts", [4, 2])
def test_bring_to_set_norms_in_the_prep_workgroup(hx, monkeypatch, nparts, modup, ptxt):
    """m = 32768 (the radix-16 ring), batch 3, 3 ctxt primes + 1 small prime: 4 and 2 parts, with and without the
    folded mod-up, an odd prime, an even and no plaintext space.  Words against the twin and the oracle, norms against
    the oracle on both; then the fdelta variant of the same mod-down (hx_scale_down_multi_norms), which reads S back
    (flush_xs -> frac_from_xs_kernel): x and S in scratch are not observable otherwise; then the call without norms
    (S alone in the prep store)."""
    m, B = 32768, 3
    primes = chain(m)
    own, add = [0, 1, 2], ([3] if modup else [])
    drop = [1]
    keep = [i for i in own + add if i not in drop]
    Pf, Pc = twins(hx, monkeypatch, m, primes)
    parts = [Pf.rand(own, 40 + i, B) for i in range(nparts)]

    def run(P):
        polys = [hx.DoubleCRT(P.g, own, B, x) for x in parts]
        norms = hx.bringToSetMulti(polys, add, keep, ptxt, norms=True)
        return norms, [by_prime(d, keep) for d in polys]

    def run_fdelta(P):
        polys = [hx.DoubleCRT(P.g, own, B, x) for x in parts]
        norms, fd = hx.scaleDownToSetMulti(polys, [0, 2], ptxt, norms=True, fdelta=True)
        return norms, fd, [by_prime(d, [0, 2]) for d in polys]

    def run_plain(P):
        polys = [hx.DoubleCRT(P.g, own, B, x) for x in parts]
        hx.bringToSetMulti(polys, add, keep, ptxt)
        return [by_prime(d, keep) for d in polys]

    (nf, wf), kf = kernels_of(hx, lambda: run(Pf))
    (nc, wc), kc = kernels_of(hx, lambda: run(Pc))
    check_routes(kf, kc, "ntt_moddown_prep_kernel<", norm_in_prep=True)
    assert nf.shape == (nparts, B) == nc.shape
    for k in range(nparts):
        assert np.array_equal(wf[k], wc[k]), k
        for b in range(B):
            want, wfd = oracle_bring(Pf, own, add, drop, ptxt, parts[k][:, b])
            assert np.array_equal(wf[k][:, b], want), (k, b)
            ref = O.embedding_largest_coeff(m, wfd)
            print("part %d element %d: norm %.17g (fused) %.17g (twin) %.17g (oracle)" % (k, b, nf[k, b], nc[k, b], ref))
            assert nf[k, b] == pytest.approx(ref, rel=NORM_RTOL)
            assert nc[k, b] == pytest.approx(ref, rel=NORM_RTOL)
    if not modup:
        (n2, fd2, w2), kf2 = kernels_of(hx, lambda: run_fdelta(Pf))
        n3, fd3, w3 = run_fdelta(Pc)
        assert not has(kf2, "moddown_S_kernel") and has(kf2, "frac_from_xs_kernel"), sorted(kf2)
        assert any("ntt_moddown_prep_kernel<" in k and k.rstrip().endswith(", 1>") for k in kf2), sorted(kf2)
        assert np.array_equal(fd2, fd3)                        # x / qd - S, the same arithmetic on the same x and S
        for k in range(nparts):
            assert np.array_equal(w2[k], w3[k]) and np.array_equal(w2[k], wf[k]), k
            for b in range(B):
                _, wfd = oracle_bring(Pf, own, [], drop, ptxt, parts[k][:, b])
                assert np.abs(fd2[k, b] - wfd).max() <= 1e-9 * (ptxt / 2 + 1)
                ref = O.embedding_largest_coeff(m, wfd)
                assert n2[k, b] == pytest.approx(ref, rel=NORM_RTOL) and n3[k, b] == pytest.approx(ref, rel=NORM_RTOL)
    pf, kp = kernels_of(hx, lambda: run_plain(Pf))
    assert not has(kp, "moddown_S_kernel"), sorted(kp)
    for k in range(nparts):
        assert np.array_equal(pf[k], wf[k]), k


# ---------------------------------------------------------------- 2. hx_tensor_bring_to_set_norms
@pytest.mark.parametrize("ptxt", [65537, 2, 1])
@pytest.mark.parametrize("modup", [True, False])
def test_tensor_bring_to_set_norms_in_the_prep_workgroup(hx, monkeypatch, modup, ptxt):
    """The three product parts formed on load (ntt_moddown_prep_tensor_kernel): words against the twin and the oracle's
    tensor product + addPrimesAndScale + scaleDownToSet, norms against the oracle on both contexts."""
    m, B = 32768, 3
    primes = chain(m)
    own, add = [0, 1, 2], ([3] if modup else [])
    drop = [2]
    keep = [i for i in own + add if i not in drop]
    Pf, Pc = twins(hx, monkeypatch, m, primes)
    ops = [Pf.rand(own, 700 + i, B) for i in range(4)]

    def run(P):
        c0, c1, d0, d1 = (hx.DoubleCRT(P.g, own, B, x) for x in ops)
        outs, norms = hx.tensorBringToSet(c0, c1, d0, d1, add, keep, ptxt, norms=True)
        return norms, [by_prime(d, keep) for d in outs]

    (nf, wf), kf = kernels_of(hx, lambda: run(Pf))
    (nc, wc), kc = kernels_of(hx, lambda: run(Pc))
    check_routes(kf, kc, "ntt_moddown_prep_tensor_kernel<", norm_in_prep=True)
    for part in range(3):
        assert np.array_equal(wf[part], wc[part]), part
    for b in range(B):
        w = Pf.o.tensor(own, *(x[:, b] for x in ops))
        for part in range(3):
            want, wfd = oracle_bring(Pf, own, add, drop, ptxt, w[part])
            assert np.array_equal(wf[part][:, b], want), (part, b)
            ref = O.embedding_largest_coeff(m, wfd)
            print("part %d element %d: norm %.17g (fused) %.17g (twin) %.17g (oracle)" % (part, b, nf[part, b], nc[part, b], ref))
            assert nf[part, b] == pytest.approx(ref, rel=NORM_RTOL)
            assert nc[part, b] == pytest.approx(ref, rel=NORM_RTOL)


# ---------------------------------------------------------------- 3. chosen coefficients in the dropped row
@pytest.mark.parametrize("ptxt", [65537, 2])
def test_chosen_coefficients_at_the_edges_of_the_register_file(hx, monkeypatch, ptxt):
    """The dropped row's x is chosen: 0, 1, (qd-1)/2, (qd-1)/2 + 1, qd - 1 at positions 0, 511, 512, 8191, 8192, 16383
    (first and last register of the first and last thread, the two halves' seam), random elsewhere, forward-transformed
    on the device into the row -- the centring edge, and with ptxt = 2 the even-p tie of the balanced remainder."""
    m, B = 32768, 3
    primes = chain(m)
    own, drop = [0, 1, 2], [1]
    keep = [0, 2]
    qd = primes[1]
    Pf, Pc = twins(hx, monkeypatch, m, primes)
    vals = [0, 1, (qd - 1) // 2, (qd - 1) // 2 + 1, qd - 1]
    pos = [0, 511, 512, 8191, 8192, 16383]
    parts = []
    for k in range(2):
        x = Pf.rand(own, 60 + k, B)
        coef = Pf.rand([1], 90 + k, B)
        for b in range(B):
            for j, p in enumerate(pos):
                coef[0, b, p] = vals[(j + b + 3 * k) % len(vals)]   # (every value at every position)
        row = hx.DoubleCRT(Pf.g, [1], B, coef).FFT().download()
        x[1] = row[0]
        parts.append((x, coef))

    def run(P):
        polys = [hx.DoubleCRT(P.g, own, B, x) for x, _ in parts]
        norms = hx.scaleDownToSetMulti(polys, keep, ptxt, norms=True)
        return norms, [by_prime(d, keep) for d in polys]

    (nf, wf), kf = kernels_of(hx, lambda: run(Pf))
    (nc, wc), kc = kernels_of(hx, lambda: run(Pc))
    check_routes(kf, kc, "ntt_moddown_prep_kernel<", norm_in_prep=True)
    for k, (x, coef) in enumerate(parts):
        assert np.array_equal(wf[k], wc[k]), k
        for b in range(B):
            assert np.array_equal(Pf.o.ifft([1], x[1:2, b])[0], coef[0, b])     # the row is the transform of the chosen x
            want, wfd = Pf.o.scale_down(own, x[:, b], drop, ptxt, want_fdelta=True)
            assert np.array_equal(wf[k][:, b], want), (k, b)
            ref = O.embedding_largest_coeff(m, wfd)
            assert nf[k, b] == pytest.approx(ref, rel=NORM_RTOL) and nc[k, b] == pytest.approx(ref, rel=NORM_RTOL)


# ---------------------------------------------------------------- 4. the other ring sizes: S in the prep store only
@pytest.mark.parametrize("m", [16384, 65536])
@pytest.mark.parametrize("tensor", [False, True])
def test_other_ring_sizes_form_S_in_the_prep_store(hx, monkeypatch, m, tensor):
    """N = 2^13 and 2^15, batch 2: S in the prep store, the norm by the kernels of before.  Words equal the twin's and
    the oracle's; norms meet the oracle."""
    B, ptxt = 2, 65537
    primes = chain(m)
    own, add, drop = [0, 1, 2], [3], [2]
    keep = [0, 1, 3]
    Pf, Pc = twins(hx, monkeypatch, m, primes)
    ops = [Pf.rand(own, 300 + i, B) for i in range(4)]

    def run(P):
        if tensor:
            c0, c1, d0, d1 = (hx.DoubleCRT(P.g, own, B, x) for x in ops)
            outs, norms = hx.tensorBringToSet(c0, c1, d0, d1, add, keep, ptxt, norms=True)
        else:
            outs = [hx.DoubleCRT(P.g, own, B, x) for x in ops[:3]]
            norms = hx.bringToSetMulti(outs, add, keep, ptxt, norms=True)
        return norms, [by_prime(d, keep) for d in outs]

    (nf, wf), kf = kernels_of(hx, lambda: run(Pf))
    (nc, wc), kc = kernels_of(hx, lambda: run(Pc))
    check_routes(kf, kc, "ntt_moddown_prep_tensor_kernel<" if tensor else "ntt_moddown_prep_kernel<", norm_in_prep=False)
    for part in range(3):
        assert np.array_equal(wf[part], wc[part]), part
    w = Pf.o.tensor(own, *(x[:, 0] for x in ops)) if tensor else [x[:, 0] for x in ops[:3]]
    for part in range(3):
        want, wfd = oracle_bring(Pf, own, add, drop, ptxt, w[part])
        assert np.array_equal(wf[part][:, 0], want), part
        ref = O.embedding_largest_coeff(m, wfd)
        assert nf[part, 0] == pytest.approx(ref, rel=NORM_RTOL) and nc[part, 0] == pytest.approx(ref, rel=NORM_RTOL)


# ---------------------------------------------------------------- 5. the digit fractions (NormSrcF64)
def test_digit_norms_in_the_direct_form(hx, monkeypatch):
    """hx_break_into_digits_norms at m = 32768: embed_norm_r16_kernel<NormSrcF64> in the direct form (the twin: the
    paired kernel) against the oracle's breakIntoDigits norms; the digit words equal the twin's."""
    m, B = 32768, 3
    g60, g56 = O.PrimeGen(60, m), O.PrimeGen(56, m)
    primes = [g60.next() for _ in range(5)] + [g56.next() for _ in range(2)]
    own, sp = [0, 1, 2, 3, 4], [5, 6]
    digits = [[0, 1], [2, 3], [4]]
    Pf, Pc = twins(hx, monkeypatch, m, primes)
    a = Pf.rand(own, 80, B)

    def run(P):
        dg, nrm = hx.DoubleCRT(P.g, own, B, a).breakIntoDigits(digits, sp, norms=True)
        return nrm, dg.download()

    (nf, wf), kf = kernels_of(hx, lambda: run(Pf))
    (nc, wc), kc = kernels_of(hx, lambda: run(Pc))
    assert has(kf, "embed_norm_r16_kernel<hx::NormSrcF64>") and not has(kf, "embed_norm_r16_paired_kernel"), sorted(kf)
    assert has(kc, "embed_norm_r16_paired_kernel<hx::NormSrcF64>") and not has(kc, "embed_norm_r16_kernel<"), sorted(kc)
    assert np.array_equal(wf, wc)
    for b in range(B):
        want = Pf.o.break_into_digits(own, a[:, b], digits, own + sp, want_norms=True)[1]
        for k in range(len(digits)):
            print("digit %d element %d: norm %.17g (direct) %.17g (paired) %.17g (oracle)" % (k, b, nf[k, b], nc[k, b], want[k]))
            assert nf[k, b] == pytest.approx(want[k], rel=NORM_RTOL)
            assert nc[k, b] == pytest.approx(want[k], rel=NORM_RTOL)
