"""What each route of the mod-switch host path (engine.hip: scale_down_impl and its three paths) launches.

scaleDownToSet, bringToSet and tensorProduct + bringToSet all go through one dispatcher that picks the fused
single-prime path, the several-primes path or the generic per-polynomial path.  Every other device test checks the
words that come out; this file also pins the launches: for each route the full table of (kernel, workgroups,
workgroup_size, calls) that hx.profileBegin() / profileEnd() report, next to the result word for word against the
oracle.  The tables are literals (EXPECTED below), recorded with this file's own helper,

    python -m tests.test_modswitch_routes_gpu

which runs every route and prints the dict; they were recorded on the commit before the host path was split into
ModSwitch and its three paths, and that split had to reproduce them exactly.  A change of the host code that keeps
the launches leaves them as they are; a change of a kernel's grid is a change of this table, made on purpose and
recorded again.  The whole file takes under 3 s on an MI355X (11 tests, the module's set-up included).  Shapes are the
smallest at which each route exists: m = 16384 is the smallest ring the fused kernels are built for, m = 256 lies
below them, m = 32768 is where the noise norm rides in the prep workgroups."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import NORM_RTOL, setup_rns

pytestmark = pytest.mark.gpu

PTXT = 65537

EXPECTED = {'fused1_in_place': [('hx::ntt_moddown_apply_kernel<13, false>', 48, 256, 1),
                                ('hx::ntt_moddown_prep_kernel<13, 1>', 2, 256, 1)],
            'fused1_mod_up_3_parts': [('hx::ntt_moddown_apply_kernel<13, false>', 40, 256, 1),
                                      ('hx::ntt_moddown_prep_kernel<13, 1>', 6, 256, 1)],
            'fusedN_3_parts': [('hx::ntt_moddown_apply_kernel<13, true>', 24, 256, 1),
                               ('hx::ntt_moddown_prep_multi_kernel<13>', 12, 256, 1),
                               ('hx::rns_extend_fast_kernel<2, false>', 64, 256, 3)],
            'fusedN_3_parts_mod_up': [('hx::ntt_moddown_apply_kernel<13, true>', 32, 256, 1),
                                      ('hx::ntt_moddown_prep_multi_kernel<13>', 12, 256, 1),
                                      ('hx::rns_extend_fast_kernel<2, false>', 64, 256, 3)],
            'generic_3_separate_runs': [('hx::ntt_small_kernel<false>', 8, 64, 3),
                                        ('hx::ntt_small_kernel<true>', 2, 64, 3),
                                        ('hx::rns_extend_fast_kernel<1, false>', 1, 256, 3),
                                        ('hx::sub_scale_from_kernel', 4, 256, 3)],
            'generic_one_poly': [('hx::ntt_small_kernel<false>', 10, 64, 1),
                                 ('hx::ntt_small_kernel<true>', 4, 64, 1),
                                 ('hx::rns_extend_fast_kernel<2, false>', 1, 256, 1),
                                 ('hx::sub_scale_from_kernel', 5, 256, 1)],
            'norms_all_parts_in_one_call': [('hx::ntt_moddown_apply_kernel<14, false>', 32, 512, 1),
                                            ('hx::ntt_moddown_prep_kernel<14, 2>', 6, 512, 1)],
            'norms_parts_one_by_one': [('hx::embed_norm_r16_kernel<hx::NormSrcF64>', 6, 512, 1),
                                       ('hx::frac_from_xs_kernel', 128, 256, 3),
                                       ('hx::ntt_moddown_apply_kernel<14, false>', 32, 512, 3),
                                       ('hx::ntt_moddown_prep_kernel<14, 1>', 2, 512, 2),
                                       ('hx::ntt_moddown_prep_kernel<14, 2>', 2, 512, 1)],
            'tensor_add1_drop1': [('hx::ntt_moddown_apply_tensor_kernel<13, false>', 80, 256, 1),
                                  ('hx::ntt_moddown_prep_tensor_kernel<13, 1>', 9, 256, 1)],
            'tensor_drop1': [('hx::ntt_moddown_apply_tensor_kernel<13, false>', 64, 256, 1),
                             ('hx::ntt_moddown_prep_tensor_kernel<13, 1>', 9, 256, 1)],
            'tensor_drop2': [('hx::ntt_moddown_apply_tensor_kernel<13, true>', 48, 256, 1),
                             ('hx::ntt_moddown_prep_multi_tensor_kernel<13>', 18, 256, 1),
                             ('hx::rns_extend_fast_kernel<2, false>', 96, 256, 3)],
            'tensor_nothing_to_drop': [('hx::tensor_kernel', 128, 256, 1)],
            'wrapped_generic': [('hx::copy_words_kernel', 160, 256, 1),
                                ('hx::ntt_row_kernel<13, false, 1>', 10, 256, 1),
                                ('hx::ntt_row_kernel<13, true, 1>', 4, 256, 1),
                                ('hx::rns_extend_fast_kernel<2, false>', 64, 256, 1),
                                ('hx::sub_scale_from_kernel', 160, 256, 1)]}


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the mod-switch route tests run on an MI355X (pytest -m gpu)")
    return capi


def launches(hx, fn):
    """fn's result and its launch table: sorted (kernel, workgroups, workgroup_size, calls)"""
    hx.profileBegin()
    out = fn()
    prof = hx.profileEnd()
    assert prof["dropped"] == 0
    return out, sorted((k["kernel"], k["workgroups"], k["workgroup_size"], k["calls"]) for k in prof["kernels"])


def names(table):
    return [row[0] for row in table]


def rows_equal(d, keep, want):
    """d's rows, matched by prime (the fused single-prime path moves the last row into the freed slot), equal
    want[keep.index(prime)] for every batch element; want: [batch][len(keep)][N]"""
    idx, got = d.getIndexSet(), d.download()
    assert sorted(idx) == sorted(keep), (idx, keep)
    for b in range(got.shape[1]):
        for r, i in enumerate(idx):
            assert np.array_equal(got[r, b], want[b][keep.index(i)]), (i, b)


def want_switch(P, cur, x, add, drop, ptxt=PTXT):
    """oracle: addPrimesAndScale(add) then scaleDownToSet dropping `drop`, per batch element of x [rows][batch][N]"""
    out = []
    for b in range(x.shape[1]):
        up = x[:, b]
        if add:
            up = np.vstack([P.o.scale_by_primes(cur, up, add), np.zeros((len(add), P.N), dtype=np.uint64)])
        out.append(P.o.scale_down(cur + add, up, drop, ptxt))
    return out


# ---------------------------------------------------------------- the routes: each returns {name: launch table}
def route_fused1_in_place(hx):
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    allp = own + sp
    drop = allp[2]
    keep = [i for i in allp if i != drop]
    x = P.rand(allp, 12, batch=2)
    d = hx.DoubleCRT(P.g, allp, 2, x)
    _, t = launches(hx, lambda: d.scaleDownToSet(keep, PTXT))
    rows_equal(d, keep, want_switch(P, allp, x, [], [drop]))
    return {"fused1_in_place": t}


def route_fused1_mod_up_several_parts(hx):
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    add, drop = [sp[0]], [own[-1]]
    keep = [i for i in own + add if i not in drop]
    xs = [P.rand(own, 50 + i, batch=2) for i in range(3)]
    holder = hx.DoubleCRT(P.g, own, 2, xs[2])
    polys = [hx.DoubleCRT(P.g, own, 2, xs[0]), hx.DoubleCRT(P.g, own, 2, xs[1]), holder.copy()]  # the last: shared slab
    _, t = launches(hx, lambda: hx.bringToSetMulti(polys, add, keep, PTXT))
    for x, d in zip(xs, polys):
        rows_equal(d, keep, want_switch(P, own, x, add, drop))
    assert holder.getIndexSet() == own and np.array_equal(holder.download(), xs[2])   # the surviving holder
    return {"fused1_mod_up_3_parts": t}


def several_primes_once(hx, P, own, add, seed):
    drop = own[-2:]
    keep = [i for i in own + add if i not in drop]
    xs = [P.rand(own, seed + i, batch=2) for i in range(3)]
    polys = [hx.DoubleCRT(P.g, own, 2, x) for x in xs]
    if add:
        _, t = launches(hx, lambda: hx.bringToSetMulti(polys, add, keep, PTXT))
    else:
        _, t = launches(hx, lambda: hx.scaleDownToSetMulti(polys, keep, PTXT))
    for x, d in zip(xs, polys):
        assert d.getIndexSet() == keep
        rows_equal(d, keep, want_switch(P, own, x, add, drop))
    for d in polys:
        d.close()
    return t


def route_several_primes(hx):
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    return {"fusedN_3_parts": several_primes_once(hx, P, own, [], 20),
            "fusedN_3_parts_mod_up": several_primes_once(hx, P, own, [sp[0]], 30)}


def route_second_identical_call(hx):
    """the cached tables (extension plan, per-row constants) are found, not built again"""
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    tables, reserved = [], []
    for _ in range(3):
        tables.append(several_primes_once(hx, P, own, [sp[0]], 30))
        reserved.append(P.g.arenaStats()["reserved"])
    assert reserved[2] == reserved[1], reserved
    assert tables[0] == tables[1] == tables[2]
    return {"fusedN_3_parts_mod_up": tables[2]}


def route_generic_one_poly(hx):
    P, own, sp = setup_rns(hx, m=256, L=5, K=2)
    allp = own + sp
    x = P.rand(allp, 5, batch=2)
    d = hx.DoubleCRT(P.g, allp, 2, x)
    _, t = launches(hx, lambda: d.scaleDownToSet(own, PTXT))
    assert d.getIndexSet() == own
    rows_equal(d, own, want_switch(P, allp, x, [], sp))
    return {"generic_one_poly": t}


def route_generic_fallback_from_multi(hx):
    P, own, sp = setup_rns(hx, m=256, L=5, K=2)
    keep = own[:-1]
    xs = [P.rand(own, 40 + i, batch=2) for i in range(3)]
    polys = [hx.DoubleCRT(P.g, own, 2, x) for x in xs]
    _, t = launches(hx, lambda: hx.scaleDownToSetMulti(polys, keep, PTXT))
    for x, d in zip(xs, polys):
        assert d.getIndexSet() == keep
        rows_equal(d, keep, want_switch(P, own, x, [], own[-1:]))
    return {"generic_3_separate_runs": t}


def route_wrapped_storage(hx):
    import torch
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    allp = own + sp
    x = P.rand(allp, 71, batch=2)
    buf = torch.from_numpy(x.view(np.int64).copy()).to("cuda:0")
    w = hx.DoubleCRT.wrap(P.g, allp, 2, buf.data_ptr())
    _, t = launches(hx, lambda: w.scaleDownToSet(own, PTXT))
    assert w.getIndexSet() == own
    want = want_switch(P, allp, x, [], sp)
    rows_equal(w, own, want)
    torch.cuda.synchronize()
    back = buf.cpu().numpy().view(np.uint64).reshape(len(allp), 2, P.N)
    for b in range(2):
        assert np.array_equal(back[:len(own), b], want[b])       # the result lives in the caller's tensor
    w.close()
    return {"wrapped_generic": t}


def route_tensor_folded_in(hx):
    P, own, sp = setup_rns(hx, m=16384, L=5, K=2)
    B = 3
    ops = [P.rand(own, 700 + i, batch=B) for i in range(4)]
    c0, c1, d0, d1 = (hx.DoubleCRT(P.g, own, B, x) for x in ops)
    w = [P.o.tensor(own, *(x[:, b] for x in ops)) for b in range(B)]
    out = {}
    for name, add, drop in (("tensor_add1_drop1", [sp[0]], [own[2]]), ("tensor_drop1", [], [own[1]]),
                            ("tensor_drop2", [], [own[0], own[4]])):
        keep = [i for i in own + add if i not in drop]
        parts, out[name] = launches(hx, lambda: hx.tensorBringToSet(c0, c1, d0, d1, add, keep, PTXT))
        for part in range(3):
            prod = np.stack([w[b][part] for b in range(B)], axis=1)
            rows_equal(parts[part], keep, want_switch(P, own, prod, add, drop))
    for d, x in zip((c0, c1, d0, d1), ops):
        assert np.array_equal(d.download(), x)               # operands untouched
    return out


def route_tensor_unsupported_fold(hx):
    P, own, sp = setup_rns(hx, m=16384, L=4, K=2)
    B = 2
    ops = [P.rand(own, 900 + i, batch=B) for i in range(4)]
    c0, c1, d0, d1 = (hx.DoubleCRT(P.g, own, B, x) for x in ops)
    outs = [hx.DoubleCRT(P.g, own, B, zero=False) for _ in range(3)]
    drop = hx._i32([sp[0], sp[1]])
    _, t = launches(hx, lambda: hx._chk(hx.lib().hx_tensor_bring_to_set(
        c0.h, c1.h, d0.h, d1.h, outs[0].h, outs[1].h, outs[2].h, None, 0, hx._p(drop), 2, PTXT)))
    for b in range(B):
        w = P.o.tensor(own, *(x[:, b] for x in ops))
        for part in range(3):
            assert outs[part].getIndexSet() == own
            assert np.array_equal(outs[part].download()[:, b], w[part]), (part, b)
    return {"tensor_nothing_to_drop": t}


def route_norms(hx):
    P, own, sp = setup_rns(hx, m=32768, L=4, K=1)
    allp = own + sp
    out = {}
    orders = {"norms_all_parts_in_one_call": [allp, allp, allp],
              "norms_parts_one_by_one": [allp, [allp[1], allp[0]] + allp[2:], allp[::-1][1:] + [allp[-1]]]}
    for name, order in orders.items():
        xs = [P.rand(o, 90 + i, batch=2) for i, o in enumerate(order)]
        polys = [hx.DoubleCRT(P.g, o, 2, x) for o, x in zip(order, xs)]
        norms, out[name] = launches(hx, lambda: hx.scaleDownToSetMulti(polys, own, PTXT, norms=True))
        for k, (o, x, d) in enumerate(zip(order, xs, polys)):
            kept = [i for i in o if i in own]
            want = []
            for b in range(2):
                rows, wfd = P.o.scale_down(o, x[:, b], sp, PTXT, want_fdelta=True)
                want.append(rows)
                assert norms[k, b] == pytest.approx(O.embedding_largest_coeff(P.o.m, wfd), rel=NORM_RTOL)
            rows_equal(d, kept, want)
    assert "frac_from_xs_kernel" not in " ".join(names(out["norms_all_parts_in_one_call"]))
    assert "frac_from_xs_kernel" in " ".join(names(out["norms_parts_one_by_one"]))
    return out


ROUTES = [route_fused1_in_place, route_fused1_mod_up_several_parts, route_several_primes, route_second_identical_call,
          route_generic_one_poly, route_generic_fallback_from_multi, route_wrapped_storage, route_tensor_folded_in,
          route_tensor_unsupported_fold, route_norms]


@pytest.mark.parametrize("route", ROUTES, ids=lambda f: f.__name__[len("route_"):])
def test_route_launches_and_words(hx, route):
    for name, table in route(hx).items():
        assert table == EXPECTED[name], (name, table)


def test_several_primes_launch_plan():
    """the several-primes table read as the plan it stands for: one prep launch per group of MD_MAXDROP dropped
    primes (2 dropped: one), the extension kernel once per poly, one apply launch -- and nothing else"""
    for name in ("fusedN_3_parts", "fusedN_3_parts_mod_up"):
        table = EXPECTED[name]
        prep = [r for r in table if "prep" in r[0]]
        ext = [r for r in table if "rns_extend" in r[0]]
        apply_ = [r for r in table if "apply" in r[0]]
        assert sum(r[3] for r in prep) == 1 and sum(r[3] for r in ext) == 3 and sum(r[3] for r in apply_) == 1, table
        assert len(prep) + len(ext) + len(apply_) == len(table), table


if __name__ == "__main__":   # the recording helper: prints the tables of every route as the EXPECTED literal
    import pprint
    import torch  # noqa: F401   (before this library touches the device, as in the fixture)
    from helib_amd import capi
    seen = {}
    for f in ROUTES:
        seen.update(f(capi))
    print("EXPECTED = " + pprint.pformat(seen, width=118))
