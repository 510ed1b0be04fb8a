"""Writes tests/golden/gr_641_2_2.json: the factors of Phi_641 Hensel-lifted modulo 4 and their idempotents, as
tests/intraslot_ref.tables(641, 2, 2) computes them (tests/bgv_pr_ref.py: Hensel's lemma and Newton's iteration in python
integers; no code of the product).  Run from the repository root:  python -m tests.golden.make_intraslot_golden"""
import json
import os

from tests import intraslot_ref as IR

if __name__ == "__main__":
    m, p, r = 641, 2, 2
    t = IR.tables(m, p, r)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gr_641_2_2.json")
    with open(out, "w") as fh:
        json.dump({"m": m, "p": p, "r": r, "F": [list(map(int, f)) for f in t.F], "E": [list(map(int, e)) for e in t.base.E]}, fh,
                  separators=(",", ":"))
        fh.write("\n")
    print(out)
