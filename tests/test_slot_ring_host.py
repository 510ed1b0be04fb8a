"""helib_amd.slot_ring is the one plain-side implementation of the ring of a slot (no GPU): bgv_gf and bgv_gr run the same
members, the linear-map modules reach the same functions and share one table cache per array, and the two array classes
stay unrelated.  m = 13, p = 3: d = 3, 4 slots; r = 1 and r = 2."""
import numpy as np
import pytest

from tests import intraslot_ref as IR


def _arrays(r):
    """the arrays over an encoder that only knows the geometry (the plain side needs no more): bgv_gr at p^r, and
    bgv_gf beside it at r = 1"""
    from helib_amd import bgv_gf, bgv_gr, ctxt as hc
    ref = IR.tables(13, 3, r)

    class Enc:
        G = [int(x) for x in ref.G]

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()
    cc = hc.ChainContext(13, 3, r, bits=100, c=2)
    out = [bgv_gr.EncryptedArray(cc, None, encoder=Enc())]
    if r == 1:
        out.append(bgv_gf.EncryptedArray(cc, None, encoder=Enc()))
    return out


def test_both_array_classes_run_one_body():
    from helib_amd import bgv_gf, bgv_gr, slot_ring
    for name in ("_mul", "_frobenius", "frobeniusPlain", "_slots", "mulPlain", "getG", "getDegree", "decrypt_batch",
                 "frobeniusAutomorph"):
        assert getattr(bgv_gf.EncryptedArray, name) is getattr(bgv_gr.EncryptedArray, name), name
        assert getattr(bgv_gf.EncryptedArray, name) is getattr(slot_ring.SlotRing, name), name
    assert not issubclass(bgv_gf.EncryptedArray, bgv_gr.EncryptedArray)
    assert not issubclass(bgv_gr.EncryptedArray, bgv_gf.EncryptedArray)
    assert issubclass(bgv_gf.GfEncoder, slot_ring.SlotEncoder) and issubclass(bgv_gr.GrEncoder, slot_ring.SlotEncoder)
    assert not hasattr(bgv_gf.GfEncoder, "encodeGathered") and hasattr(bgv_gr.GrEncoder, "encodeGathered")


@pytest.mark.parametrize("r", [1, 2])
def test_the_fronts_reach_one_function_and_one_cache(r, monkeypatch):
    from helib_amd import bgv_gf_matmul as GM, bgv_gr_matmul as RM, intraslot, slot_ring
    d, P = 3, 3 ** r
    L = np.random.default_rng(r).integers(0, P, size=(d, d))
    for ea in _arrays(r):
        ring = type(ea).__module__.endswith("bgv_gr")
        M = RM if ring else GM
        assert ea.P == P and (ea.size(), ea.getDegree()) == (4, d)
        before = set(ea.__dict__)
        M.linPolyMatrix(ea)
        want = intraslot.buildLinPolyCoeffs(ea, L)
        Tf = M.linPolyTable(ea)
        # one cache, holding what every module reads
        assert set(ea.__dict__) - before == {"_linpoly"}
        assert intraslot._tables(ea) is slot_ring._tables(ea) is ea.__dict__["_linpoly"]
        assert Tf is slot_ring._tables(ea).flat()
        assert np.array_equal(M.buildLinPolyCoeffs(ea, L), want) and np.array_equal(M.linPolyFlat(ea, L), want)
        # one function behind both names
        calls = []
        real = slot_ring.buildLinPolyCoeffs
        monkeypatch.setattr(slot_ring, "buildLinPolyCoeffs", lambda e, x: calls.append(e) or real(e, x))
        assert np.array_equal(M.buildLinPolyCoeffs(ea, L), want) and np.array_equal(intraslot.buildLinPolyCoeffs(ea, L), want)
        assert calls == [ea, ea]
        monkeypatch.undo()
        # each front keeps its own check
        other = GM if ring else RM
        with pytest.raises(Exception, match="r > 1" if r > 1 else "bgv_g[fr].EncryptedArray"):
            other.buildLinPolyCoeffs(ea, L)
