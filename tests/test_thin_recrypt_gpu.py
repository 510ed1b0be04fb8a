"""thinReCrypt on the device at the rings of tests/test_thin_recrypt_host.py, with its assertions, batch 2: thinly packed
slots come back, isCorrect(), the capacity grows, the plaintext space is p^r, the scaled noise of the raw mod-switch is
within its bound; once more after another multiplication; the packed reCrypt of the same thin input decrypts to the same
slots; and the hoisted sum in one device call leaves the words of the loop.  Every comparison is exact."""
import numpy as np
import pytest

from tests import thin_ref as TR

pytestmark = pytest.mark.gpu

BITS = 400       # tests/test_thin_recrypt_host.py: the smallest multiple of 100 at which thinReCrypt holds, plus 100


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU tests run on an MI355X (pytest -m gpu)")
    return capi


@pytest.mark.parametrize("m,r", TR.THIN_RINGS)
def test_thin_recrypt_on_the_device(hx, m, r):
    from helib_amd import ctxt as hc, keys as hk, recryption as RC, thin_evalmap as TE, timing
    from tests import evalmap_tables as E
    p, _, mvec, gens, ords = E.ring(m)
    cc = hc.ChainContext(m, p, r, bits=BITS, c=2, bootstrappable=True)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    rc = RC.ThinRecryptData(cc, g, mvec, gens=gens, ords=ords, alsoThick=True)
    ea = rc.ea
    assert rc.ea_boot.P == p ** (cc.e - cc.ePrime + r) and ea.P == p ** r and rc.ea_boot.cc is cc
    assert rc.coeffToSlot.ea is rc.ea_boot and rc.slotToCoeff.ea is ea and rc.firstMap is not None
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    hk.addFrbMatrices(sk)
    assert sk.genRecryptData(rc) == 1 and sk.recryptEkey.ptxtSpace == rc.ea_boot.P
    v = np.random.default_rng(m + r).integers(0, p ** r, size=(2, ea.size()))        # one integer per slot
    want = ea._slots(v)
    ct = ea.encrypt_batch(sk, v)
    while ct.bitCapacity() > 60:                                         # use the capacity up
        ct.multiplyBy(ea.encrypt_batch(sk, v))
        want = ea.mulPlain(want, v)
    if p > 2:
        ct.mulIntFactor(3)                                               # intFactor != 1: lost and restored
        assert ct.intFactor != 1
    before = ct.bitCapacity()
    assert not want[:, :, 1:].any() and np.array_equal(ea.decrypt_batch(ct, sk), want)
    thick, again = ct.clone(), ct.clone()
    timing.resetAllTimers()
    stats = {}
    assert hc.Ctxt.fuseHoistedSum is True
    assert RC.thinReCrypt(ct, sk, rc, seed=5, stats=stats) is ct
    assert TE.traceMap.last == "hoisted"
    assert 0 < stats["raw-mod-switch-noise"][0] <= 1
    for name in ("AAA_slotToCoeff", "AAA_bootKeySwitch", "AAA_coeffToSlot", "AAA_extractDigitsThin"):
        assert timing.getTimerByName(name).numCalls == 1, name
    assert ct.isCorrect() and ct.bitCapacity() > before and ct.ptxtSpace == p ** r
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)                # exact, both batch elements
    # with the hoisted sum as the reference's loop: the same ciphertext, word for word
    try:
        hc.Ctxt.fuseHoistedSum = False
        RC.thinReCrypt(again, sk, rc, seed=5)
    finally:
        hc.Ctxt.fuseHoistedSum = True
    assert (again.lnNoise, again.primeSet, again.ptxtSpace, again.intFactor) == (ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor)
    assert sorted(again.parts, key=str) == sorted(ct.parts, key=str)
    assert all(np.array_equal(again.parts[h].download(), ct.parts[h].download()) for h in ct.parts)
    ct.multiplyBy(ea.encrypt_batch(sk, v))                               # one more multiplication, and again
    want2 = ea.mulPlain(want, v)
    stats = {}
    RC.thinReCrypt(ct, sk, rc, seed=6, stats=stats)
    assert 0 < stats["raw-mod-switch-noise"][0] <= 1
    assert ct.isCorrect() and ct.ptxtSpace == p ** r and np.array_equal(ea.decrypt_batch(ct, sk), want2)
    RC.reCrypt(thick, sk, rc, seed=5)                                    # the packed form on the same thin input
    assert thick.isCorrect() and np.array_equal(ea.decrypt_batch(thick, sk), want)
