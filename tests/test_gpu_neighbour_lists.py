"""The neighbour stores (umi_data_new[_wide]: HipNaive), whole rows with their distances.  A store answers
only by removing entries, so a row is read whole only from a store nothing has been removed from: for every
entry q of a case a fresh store is built, and remove_near(q, d, 2^31 - 1) for d = 0, 1, .., max_edits must
return exactly q's neighbours at distance d (tests/pair_list_model.py), q itself in call 0.  That pins every
edge, its distance byte, the absence of every other pair and the host's CSR build.  The inputs and what makes
them worth running are checked without a GPU in tests/test_pair_list_model_cpu.py."""
import numpy as np
import pytest

import oracle as orc
import pair_list_model as plm

pytestmark = pytest.mark.gpu

ANY_FREQ = 2 ** 31 - 1
ROWS_PER_ID = 400  # (every store of these cases is smaller: one id per case)


def context_of(st):
    import umi_collapse_rs_amd as umi
    ctx = umi.Context([0, 0]) if st.ctx == "multi" else umi.Context(0)
    for o, v in st.opts.items():
        ctx.set_option(o, v)
    return ctx


def new_store(st, ctx):
    import umi_collapse_rs_amd as umi
    if st.ctx == "grow":  # the library's list starts at 1,024 entries again and the pair work is redone
        ctx.set_option("edge_capacity", 1)
    return umi.HipNaive.new(dict(zip(st.umis, st.freq)), st.L, st.max_edits, ctx=ctx)


def check_row(st, ctx, q):
    d = new_store(st, ctx)
    want = {}
    for o, dist in st.rows[q]:
        want.setdefault(dist, set()).add(st.umis[o])
    want.setdefault(0, set()).add(st.umis[q])
    gone = set()
    for k in range(min(st.max_edits, plm.BATCH_MAX_K) + 1):
        got = d.remove_near(st.umis[q], k, ANY_FREQ)
        exp = want.get(k, set())
        assert got == exp, "%s row %d (%s) at distance %d: missing %s, extra %s" % (
            st.name, q, st.umis[q], k, sorted(exp - got)[:5], sorted(got - exp)[:5])
        gone |= got
    assert all(d.contains(u) == (u not in gone) for u in st.umis), "%s row %d: contains" % (st.name, q)


@pytest.mark.parametrize("name", plm.STORES)
def test_every_row_of_a_fresh_store(name):
    st = plm.store(name)
    assert len(st.umis) <= ROWS_PER_ID
    ctx = context_of(st)
    try:
        for q in range(len(st.umis)):
            check_row(st, ctx, q)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", plm.STORES)
def test_a_query_sequence_and_the_edge_calls(name):
    """100 random queries with random k <= max_edits and random max_freq on one store against orc.Naive; then
    k = -1, and stores of no, one and two entries."""
    import umi_collapse_rs_amd as umi
    st = plm.store(name)
    rng = np.random.default_rng(plm._seed("queries" + name))
    n = len(st.umis)
    ctx = context_of(st)
    try:
        d, o = new_store(st, ctx), orc.Naive(st.umis, st.freq)
        for q in rng.integers(0, n, 100):
            k = int(rng.integers(0, st.max_edits + 1))
            mf = int(rng.choice([0, 1, 2, 3, 5, ANY_FREQ]))
            got = d.remove_near(st.umis[q], k, mf)
            assert got == {st.umis[i] for i in o.remove_near(int(q), k, mf)}, (name, int(q), k, mf)
        assert all(d.contains(u) == o.contains(i) for i, u in enumerate(st.umis))
        d = new_store(st, ctx)
        assert d.remove_near(st.umis[0], -1, ANY_FREQ) == set() and all(d.contains(u) for u in st.umis)
        for m in (0, 1, 2):
            sub = umi.HipNaive.new(dict(zip(st.umis[:m], st.freq[:m])), st.L, st.max_edits, ctx=ctx)
            so = orc.Naive(st.umis[:m], st.freq[:m]) if m else None
            for q in range(m):
                got = sub.remove_near(st.umis[q], st.max_edits, ANY_FREQ)
                assert got == {st.umis[i] for i in so.remove_near(q, st.max_edits, ANY_FREQ)}, (name, m, q)
            assert m == n or not sub.contains(st.umis[m])  # (not a member)
            assert all(not sub.contains(u) for u in st.umis[:m])
    finally:
        ctx.close()
