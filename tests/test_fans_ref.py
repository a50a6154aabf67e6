"""The closed forms of tests/fans.py against the literal host restatements, on a small list of lengths: the closed form is not its own
oracle.  No GPU."""
import numpy as np
import pytest

from tests import betweenness_ref as bref
from tests import distance_ref as dref
from tests import fans, graphs

SMALL = (0, 1, 3, 4, 5, 9, 17)


def _graph(fan, flipped=False):
    ids, row_ptr, src = graphs.dense_from_tuples(fan.tuples(flipped))
    assert len(ids) == fan.n and ids["lo"].tolist() == list(range(1, fan.n + 1))  # sid == node index
    return row_ptr, src


def _source_sets(fan):
    yield [fan.r2, fan.x, fan.r]
    yield [fan.r]
    yield [fan.r2, fan.x, fan.r] + [fan.hub_of(K) for K in (1, 4, 5, 9, 17)] + [int(fan.leaves(17)[3])]
    if fan.diamond:
        yield [fan.x, int(fan.mid[3, 0]), int(fan.mid[3, 1]), fan.hub_of(4), fan.n - 1]


@pytest.mark.parametrize("diamond", [False, True])
def test_brandes_closed_form_against_the_literal_restatement(diamond):
    fan = fans.Fan(SMALL, diamond=diamond)
    row_ptr, src = _graph(fan)
    assert fan.n == 3 + (3 if diamond else 1) * len(SMALL) + sum(SMALL) + int(fan.tips_of_leaf.sum())
    for sources in _source_sets(fan):
        res = bref.literal(fan.n, row_ptr, src, sources)
        assert res.sources == sorted(sources)
        for k, s in enumerate(res.sources):
            dist, sigma, delta = fan.brandes(s)
            assert np.array_equal(dist, res.dist[k]), s
            assert sigma.tolist() == res.sigma[k], s
            assert delta.tobytes() == res.delta[k].tobytes(), s
        total, reached = fan.sums(sources)
        assert np.array_equal(reached, res.reached) and total.tobytes() == res.sums.tobytes()
        assert res.max_dist == max(int(fan.brandes(s)[0].max()) for s in sources)
    # the coefficients are what the flavour promises: integers on the tree, half-integers under the diamond
    _, sigma, delta = fan.brandes(fan.r2)
    coef = (1.0 + delta) / sigma.astype(np.float64)
    assert np.array_equal(coef * 2, np.round(coef * 2)) and (np.any(coef != np.round(coef)) == diamond)


@pytest.mark.parametrize("diamond", [False, True])
def test_descendants_and_depths_against_a_bfs(diamond):
    fan = fans.Fan(SMALL, diamond=diamond)
    row_ptr, src = _graph(fan)
    for v in range(fan.n):
        d = dref.bfs(fan.n, row_ptr, src, [v])
        assert np.array_equal(d, fan.dist_from([v])), v
        assert int((d != dref.UNREACHED).sum()) - 1 == fan.desc[v], v
    tips = [fan.n - 1, fan.tip_first, int(fan.leaves(9)[2]), fan.hub_of(0)]
    for targets in ([t] for t in tips + [fan.r2, fan.r]):
        assert np.array_equal(dref.bfs(fan.n, row_ptr, src, targets, reversed=True), fan.dist_to(targets)), targets
    assert np.array_equal(dref.bfs(fan.n, row_ptr, src, tips, reversed=True), fan.dist_to(tips))
    assert np.array_equal(dref.dijkstra(fan.n, row_ptr, src, [fan.r2]), fan.dist_from([fan.r2]))
    # the flipped graph: the same distances the other way round
    frow_ptr, fsrc = _graph(fan, flipped=True)
    assert np.array_equal(dref.bfs(fan.n, frow_ptr, fsrc, tips), fan.dist_to(tips))
    assert np.array_equal(dref.bfs(fan.n, frow_ptr, fsrc, [fan.r2], reversed=True), fan.dist_from([fan.r2]))
    assert np.array_equal(np.diff(np.asarray(frow_ptr, dtype=np.int64))[fan.hub], np.array(SMALL))  # the in-lists carry the lengths


def test_the_full_family():
    fan = fans.Fan()
    assert fan.Ks == fans.KS and 120_000 < fan.n < 135_000 and len(fan.frm) == fan.n - 1
    outdeg = np.bincount(fan.frm, minlength=fan.n)
    assert np.array_equal(outdeg[fan.hub], np.array(fans.KS)) and fan.hub.tolist() == list(range(3, 3 + len(fans.KS)))
    assert int(np.bincount(fan.to, minlength=fan.n).max()) == 1  # a tree
    assert fan.desc[fan.r2] == fan.n - 1
    # neighbouring leaves differ, and the tip counts repeat with none of the kernels' step sizes
    t = fans.w(12289, np.arange(12289))
    assert set(t.tolist()) == {0, 1, 2, 3} and np.count_nonzero(np.diff(t)) > 6000
    for period in (4, 16, 64, 256, 4096):
        assert np.count_nonzero(t[period:] != t[:-period]) > (len(t) - period) // 2, period
    dia = fans.Fan(diamond=True)
    assert dia.n == fan.n + 2 * len(fans.KS) and int(np.bincount(dia.to, minlength=dia.n).max()) == 2
    assert dia.desc[dia.r2] == dia.n - 1
